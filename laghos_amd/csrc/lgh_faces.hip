// lgh_faces.hip — surface and slice sampling: the fields of a state, and their derivatives, on the lattices of a list of zone faces.
//
// A face is (zone e, local face f = 2a + s): the side xi_a = s of the zone.  Its lattice is the zone's volume lattice of
// lgh_sample_fields / lgh_sample_derived with ONE abscissa on axis a - R1^(dim-1) points over the other axes in ascending
// order - so nothing has to be located: a logical plane of a structured mesh is a list of whole faces.
//
// Every output but the area vector has the bits the two volume kernels give at the same lattice point.  That holds by
// construction: the contraction is sample_stage / sample_last of lgh_sample.hpp with the axes in the volume kernels'
// order, every sum their sample_dot; on the normal axis a stage takes ONE lattice point and the table row of abscissa s,
// copied out of the table (R1 = 1, T = the row: T[0 + 1 * d] is T[r + R1 * d] of the volume kernel at r = s (R1 - 1)), so
// every sum has the terms of the volume kernel's sum in its order.  The stages before the last are faces_stage below:
// sample_stage for one zone and one field per face, the faces of a workgroup side by side (their axes differ, so their
// point counts do); the last is sample_last itself.  p, cs, det J, adj(J), L and what follows from L are the functions
// of lgh_sample.hpp the volume kernels call.  The whole nodal basis of the zone is contracted, not the face's dofs alone:
// a Gauss-Lobatto basis function that vanishes on the face still enters the sums with its exact or rounded zero, and
// its derivative along the normal does not vanish at all.
//
// Shape: 256 threads; FPB faces per workgroup (as many as fit 256 lattice points and 48 KB of LDS); each face gathers
// the dofs of its own zone through h1_map (the zones of a list are neither consecutive nor distinct).  The scalar
// fields - dim components of x, dim of v, e, rho - go one per pass through the same LDS, as in lgh_derived.hip, and a
// thread keeps the value and the dim derivatives of each at its ONE lattice point (NPF <= 81 < 256) in registers.  A
// workgroup's points are one contiguous range of every output array; consecutive lanes store consecutive doubles.
// Every sum runs ascending in one thread, no atomics.  Reads S, rho_l2, h1_map, gamma and the face list; writes its
// outputs.  Output-bound, off the timed path.
#include "lgh_common.hpp"
#include "lgh_sample.hpp"

#include <algorithm>
#include <numeric>

namespace lgh
{

struct FacesArgs
{
   double Th[kSampleMaxTab]; // H1 lattice table [r + R1*d]
   double Gh[kSampleMaxTab]; // its derivative
   double Tl[kSampleMaxTab]; // L2 lattice table [r + R1*l]
   const double *x, *v, *e, *rho; // the blocks of S (component c of x at x + c*N) and the density dofs
   double *xo, *vo, *eo, *rhoo, *po, *detj, *gradv, *div, *vort, *cs, *an;
   const int *map;
   const double *gamma;
   const int *faces;         // device copy of the list: faces[2k] = e, faces[2k+1] = f
   long N, NPt;
   int nfaces, D, L, R1, FPB;
   int stride;               // doubles of LDS per face
   int val_x, val_v, der_x, der_v, need_e, need_rho;
};

// the tables in LDS: whole, and the rows of the two sides' abscissae (r = 0 and r = R1 - 1) as tables of one lattice point
struct FaceTabs
{
   const double *Th, *Gh, *Tl, *ThR, *GhR, *TlR; // rows: side s at + s * D (H1), + s * L (L2)
};

// A face's region of LDS: one word with its (zone, local face), then the stages of the field in flight
__device__ __forceinline__ const int *face_meta(const double *buf, const int ZS, const int z) { return reinterpret_cast<const int *>(buf + (size_t)z * ZS); }
__device__ __forceinline__ double *face_data(double *buf, const int ZS, const int z) { return buf + (size_t)z * ZS + 1; }

// Stage st (0: the first axis, 1: the second of three) of one field of EVERY face of the workgroup: per face what sample_stage
// does for one zone and one field (nz = nf = 1) - the same index split, the same sample_dot - with the face's own point count on
// the axis (one on its normal axis, with the row of its side as the table), so the faces of a workgroup run side by side
// whatever their axes.  n dofs per direction; T whole table, TR its two rows; in / out: offsets inside a face's data.
template <int DIM>
__device__ __forceinline__ void faces_stage(const int nf, const int st, const int n, const int R1, const double *__restrict__ T,
                                            const double *__restrict__ TR, double *buf, const int ZS, const int in, const int out)
{
   int post = 1;
   for (int k = st + 1; k < DIM; k++) { post *= n; }
   const int cmax = post * R1 * (st == 0 ? 1 : R1); // a face's entries of this stage where no axis so far is its normal one
   for (int i = threadIdx.x; i < nf * cmax; i += kSampleThreads)
   {
      const int z = i / cmax, o = i - z * cmax;
      const int f = face_meta(buf, ZS, z)[1], ax = f >> 1, s = f & 1;
      const int R = (ax == st) ? 1 : R1, pre = (st == 0 || ax == 0) ? 1 : R1;
      if (o >= post * R * pre) { continue; }
      const int lo = o % pre, r = (o / pre) % R, hi = o / (pre * R);
      double *U = face_data(buf, ZS, z);
      const double *u = U + in + (size_t)hi * n * pre + lo;
      U[out + o] = sample_dot(n, R, pre, ((ax == st) ? TR + s * n : T) + r, u);
   }
}

// One H1 component of the workgroup's faces at this thread's lattice point: the value and, with `der`, the dim derivatives
// d u / d xi_j.  Per face in LDS: U | B1 G1 | BB GB BG as in lgh_derived.hip (sized for R1 points on every axis).
// Gathers through buf; synchronises before it returns.
template <int DIM>
__device__ __forceinline__ void faces_h1_component(const FacesArgs &a, const double *__restrict__ src, const int nf, const FaceTabs &tb,
                                                   double *buf, const bool der, double &val, double (&g)[DIM])
{
   const int D = a.D, R1 = a.R1, ZS = a.stride, t = threadIdx.x;
   const int ND = (DIM == 3) ? D * D * D : D * D;
   const int NPF = (DIM == 3) ? R1 * R1 : R1;
   for (int i = t; i < nf * ND; i += kSampleThreads)
   {
      const int z = i / ND, d = i - z * ND;
      const long e = face_meta(buf, ZS, z)[0];
      face_data(buf, ZS, z)[d] = src[a.map[e * ND + d]];
   }
   __syncthreads();
   const int oB1 = ND, oG1 = oB1 + R1 * (ND / D), oBB = oG1 + R1 * (ND / D), oGB = oBB + R1 * R1 * D, oBG = oGB + R1 * R1 * D;
   faces_stage<DIM>(nf, 0, D, R1, tb.Th, tb.ThR, buf, ZS, 0, oB1);
   if (der) { faces_stage<DIM>(nf, 0, D, R1, tb.Gh, tb.GhR, buf, ZS, 0, oG1); }
   __syncthreads();
   if constexpr (DIM == 3)
   {
      faces_stage<DIM>(nf, 1, D, R1, tb.Th, tb.ThR, buf, ZS, oB1, oBB);
      if (der)
      {
         faces_stage<DIM>(nf, 1, D, R1, tb.Th, tb.ThR, buf, ZS, oG1, oGB);
         faces_stage<DIM>(nf, 1, D, R1, tb.Gh, tb.GhR, buf, ZS, oB1, oBG);
      }
      __syncthreads();
   }
   if (t < nf * NPF)
   {
      const int z = t / NPF, p = t - z * NPF;
      const int f = face_meta(buf, ZS, z)[1], ax = f >> 1, s = f & 1;
      const double *U = face_data(buf, ZS, z);
      constexpr int last = DIM - 1;
      const int Rl = (ax == last) ? 1 : R1, pre = NPF / Rl; // the points of the axes before the last
      const double *Tn = (ax == last) ? tb.ThR + s * D : tb.Th, *Gn = (ax == last) ? tb.GhR + s * D : tb.Gh;
      if constexpr (DIM == 2)
      {
         val = sample_last(D, Rl, pre, p, Tn, U + oB1);
         if (der)
         {
            g[0] = sample_last(D, Rl, pre, p, Tn, U + oG1);
            g[1] = sample_last(D, Rl, pre, p, Gn, U + oB1);
         }
      }
      else
      {
         val = sample_last(D, Rl, pre, p, Tn, U + oBB);
         if (der)
         {
            g[0] = sample_last(D, Rl, pre, p, Tn, U + oGB);
            g[1] = sample_last(D, Rl, pre, p, Tn, U + oBG);
            g[2] = sample_last(D, Rl, pre, p, Gn, U + oBB);
         }
      }
   }
   __syncthreads(); // the next pass gathers into the same LDS
}

// One L2 field the same way (values only): U | first stage | second stage per face.
template <int DIM>
__device__ __forceinline__ double faces_l2_field(const FacesArgs &a, const double *__restrict__ src, const int nf, const FaceTabs &tb, double *buf)
{
   const int L = a.L, R1 = a.R1, ZS = a.stride, t = threadIdx.x;
   const int NL = (DIM == 3) ? L * L * L : L * L;
   const int NPF = (DIM == 3) ? R1 * R1 : R1;
   for (int i = t; i < nf * NL; i += kSampleThreads)
   {
      const int z = i / NL, l = i - z * NL;
      const long e = face_meta(buf, ZS, z)[0];
      face_data(buf, ZS, z)[l] = src[e * NL + l];
   }
   __syncthreads();
   const int o1 = NL, o2 = o1 + R1 * (NL / L);
   faces_stage<DIM>(nf, 0, L, R1, tb.Tl, tb.TlR, buf, ZS, 0, o1);
   __syncthreads();
   if constexpr (DIM == 3)
   {
      faces_stage<DIM>(nf, 1, L, R1, tb.Tl, tb.TlR, buf, ZS, o1, o2);
      __syncthreads();
   }
   double val = 0.0;
   if (t < nf * NPF)
   {
      const int z = t / NPF, p = t - z * NPF;
      const int f = face_meta(buf, ZS, z)[1], ax = f >> 1, s = f & 1;
      const double *U = face_data(buf, ZS, z);
      constexpr int last = DIM - 1;
      const int Rl = (ax == last) ? 1 : R1, pre = NPF / Rl;
      val = sample_last(L, Rl, pre, p, (ax == last) ? tb.TlR + s * L : tb.Tl, U + ((DIM == 3) ? o2 : o1));
   }
   __syncthreads();
   return val;
}

template <int DIM>
__global__ void __launch_bounds__(kSampleThreads) sample_faces_k(const FacesArgs a)
{
   extern __shared__ double sm[];
   const int D = a.D, L = a.L, R1 = a.R1, t = threadIdx.x;
   const int NPF = (DIM == 3) ? R1 * R1 : R1;
   double *Th = sm, *Gh = Th + R1 * D, *Tl = Gh + R1 * D, *ThR = Tl + R1 * L, *GhR = ThR + 2 * D, *TlR = GhR + 2 * D, *buf = TlR + 2 * L;
   const long k0 = (long)blockIdx.x * a.FPB;
   const int nf = (int)min((long)a.FPB, (long)a.nfaces - k0); // faces of this workgroup (the last one may hold fewer)
   for (int i = t; i < R1 * D; i += kSampleThreads) { Th[i] = a.Th[i]; Gh[i] = a.Gh[i]; }
   for (int i = t; i < R1 * L; i += kSampleThreads) { Tl[i] = a.Tl[i]; }
   for (int i = t; i < 2 * D; i += kSampleThreads)
   {
      const int s = i / D, d = i - s * D, r = s * (R1 - 1);
      ThR[i] = a.Th[r + R1 * d];
      GhR[i] = a.Gh[r + R1 * d];
   }
   for (int i = t; i < 2 * L; i += kSampleThreads)
   {
      const int s = i / L, l = i - s * L;
      TlR[i] = a.Tl[s * (R1 - 1) + R1 * l];
   }
   if (t < nf) // the faces of the workgroup, kept in front of their data
   {
      int *m = reinterpret_cast<int *>(buf + (size_t)t * a.stride);
      m[0] = a.faces[2 * (k0 + t)];
      m[1] = a.faces[2 * (k0 + t) + 1];
   }
   __syncthreads();
   const FaceTabs tb = {Th, Gh, Tl, ThR, GhR, TlR};
   double X[DIM], Vv[DIM], J[DIM][DIM], V[DIM][DIM], ev = 0.0, rv = 0.0;
#pragma unroll
   for (int c = 0; c < DIM; c++)
   {
      X[c] = 0.0; Vv[c] = 0.0;
#pragma unroll
      for (int j = 0; j < DIM; j++) { J[c][j] = 0.0; V[c][j] = 0.0; }
   }
   if (a.val_x || a.der_x)
   {
#pragma unroll
      for (int c = 0; c < DIM; c++)
      {
         double g[DIM] = {};
         faces_h1_component<DIM>(a, a.x + (size_t)c * a.N, nf, tb, buf, a.der_x != 0, X[c], g);
#pragma unroll
         for (int j = 0; j < DIM; j++) { J[c][j] = g[j]; }
      }
   }
   if (a.val_v || a.der_v)
   {
#pragma unroll
      for (int c = 0; c < DIM; c++)
      {
         double g[DIM] = {};
         faces_h1_component<DIM>(a, a.v + (size_t)c * a.N, nf, tb, buf, a.der_v != 0, Vv[c], g);
#pragma unroll
         for (int j = 0; j < DIM; j++) { V[c][j] = g[j]; }
      }
   }
   if (a.need_e) { ev = faces_l2_field<DIM>(a, a.e, nf, tb, buf); }
   if (a.need_rho) { rv = faces_l2_field<DIM>(a, a.rho, nf, tb, buf); }
   // the point values: LDS is done with, registers -> global
   if (t >= nf * NPF) { return; }
   const size_t NPt = (size_t)a.NPt, pt = (size_t)k0 * NPF + t;
   const int z = t / NPF;
   const long e = face_meta(buf, a.stride, z)[0];
   const int f = face_meta(buf, a.stride, z)[1], ax = f >> 1;
   if (a.xo)
   {
#pragma unroll
      for (int c = 0; c < DIM; c++) { a.xo[c * NPt + pt] = X[c]; }
   }
   if (a.vo)
   {
#pragma unroll
      for (int c = 0; c < DIM; c++) { a.vo[c * NPt + pt] = Vv[c]; }
   }
   if (a.eo) { a.eo[pt] = ev; }
   if (a.rhoo) { a.rhoo[pt] = rv; }
   if (a.po) { a.po[pt] = sample_pressure(a.gamma[e], rv, ev); }
   if (a.cs)
   {
      const double gz = a.gamma[e];
      a.cs[pt] = derived_cs(gz, ev);
   }
   if (!a.der_x) { return; }
   double A[DIM][DIM];
   const double det = derived_adj<DIM>(J, A);
   if (a.detj) { a.detj[pt] = det; }
   if (a.an)
   {
      // Nanson: the outward area vector per unit reference area, N_i = sgn adj(J)_{a i}
      const double sgn = (f & 1) ? 1.0 : -1.0;
#pragma unroll
      for (int c = 0; c < DIM; c++)
      {
         double r = A[0][c];
#pragma unroll
         for (int m = 1; m < DIM; m++) { r = (ax == m) ? A[m][c] : r; }
         a.an[c * NPt + pt] = sgn * r;
      }
   }
   if (!a.der_v) { return; }
   derived_grad<DIM>(V, A, det, pt, NPt, a.gradv, a.div, a.vort);
}

// what the launch is sized with: doubles of tables and of one face in LDS
static void faces_lds(const int dim, const int D, const int L, const int R1, size_t *tab_bytes, size_t *face_bytes)
{
   const int h1 = ipow(D, dim) + 2 * R1 * ipow(D, dim - 1) + (dim == 3 ? 3 * R1 * R1 * D : 0);
   const int l2 = ipow(L, dim) + R1 * ipow(L, dim - 1) + (dim == 3 ? R1 * R1 * L : 0);
   *face_bytes = (size_t)(1 + std::max(h1, l2)) * sizeof(double); // (one word in front: the face's zone and local face)
   *tab_bytes = (size_t)(R1 + 2) * (2 * D + L) * sizeof(double);
}

} // namespace lgh

using namespace lgh;

extern "C"
{

int lgh_sample_faces_fpb(lgh_ctx *c, int R1, int *fpb)
{
   LGH_CHECK_ARG(c && fpb);
   if (c->dim == 1 || lattice_refusal(c, R1) != LGH_OK)
   {
      set_error("lgh_sample_faces_fpb: dim = %d, R1 = %d: lgh_sample_faces refuses these", c->dim, R1);
      return LGH_ERR_ARG;
   }
   size_t tab_bytes, face_bytes;
   faces_lds(c->dim, c->D1D, c->L1D, R1, &tab_bytes, &face_bytes);
   *fpb = patches_per_group(kSampleThreads, ipow(R1, c->dim - 1), tab_bytes, face_bytes);
   return LGH_OK;
}

int lgh_sample_faces(lgh_ctx *c, const double *S, const double *rho_l2, int R1, const double *B_h1_lat, const double *G_h1_lat,
                     const double *B_l2_lat, int nfaces, const int *faces, double *x_out, double *v_out, double *e_out, double *rho_out,
                     double *p_out, double *detj_out, double *gradv_out, double *div_out, double *vort_out, double *cs_out, double *an_out)
{
   LGH_CHECK_ARG(c && S);
   const int dim = c->dim, D = c->D1D, L = c->L1D;
   if (dim == 1)
   {
      set_error("lgh_sample_faces: dim = 1: faces are sampled in 2D and 3D");
      return LGH_ERR_ARG;
   }
   LGH_PASS(lattice_r1("lgh_sample_faces", R1));
   if (nfaces < 0)
   {
      set_error("lgh_sample_faces: nfaces = %d", nfaces);
      return LGH_ERR_ARG;
   }
   const bool der = detj_out || gradv_out || div_out || vort_out || an_out;
   const bool h1 = der || x_out || v_out, l2 = e_out || rho_out || p_out || cs_out;
   if ((h1 && !B_h1_lat) || (der && !G_h1_lat) || (l2 && !B_l2_lat))
   {
      set_error("lgh_sample_faces: %s is NULL and an output needs it", (h1 && !B_h1_lat) ? "B_h1_lat" : ((der && !G_h1_lat) ? "G_h1_lat" : "B_l2_lat"));
      return LGH_ERR_ARG;
   }
   if (!rho_l2 && (rho_out || p_out))
   {
      set_error("lgh_sample_faces: %s needs the density dofs, but rho_l2 is NULL", rho_out ? "rho_out" : "p_out");
      return LGH_ERR_ARG;
   }
   if (nfaces > 0 && !faces)
   {
      set_error("lgh_sample_faces: faces is NULL with nfaces = %d", nfaces);
      return LGH_ERR_ARG;
   }
   for (int k = 0; k < nfaces; k++)
   {
      const int e = faces[2 * k], f = faces[2 * k + 1];
      if (e < 0 || e >= c->NE)
      {
         set_error("lgh_sample_faces: faces[%d]: zone %d is outside 0..%d", 2 * k, e, c->NE - 1);
         return LGH_ERR_ARG;
      }
      if (f < 0 || f >= 2 * dim)
      {
         set_error("lgh_sample_faces: faces[%d]: local face %d is outside 0..%d", 2 * k + 1, f, 2 * dim - 1);
         return LGH_ERR_ARG;
      }
   }
   FacesArgs a;
   memset(&a, 0, sizeof(a));
   LGH_PASS(lattice_tables("lgh_sample_faces", c, R1, h1 ? B_h1_lat : nullptr, der ? G_h1_lat : nullptr, l2 ? B_l2_lat : nullptr, a.Th, a.Gh, a.Tl, true));
   size_t tab_bytes, face_bytes;
   faces_lds(dim, D, L, R1, &tab_bytes, &face_bytes);
   LGH_PASS(lattice_lds_fits("lgh_sample_faces", "face of a zone", c, R1, tab_bytes + face_bytes));
   if (nfaces == 0 || !(h1 || l2)) { return LGH_OK; }
   // the list on the device: a buffer of the context, regrown when a longer list comes.  The copy is ordered on the
   // context's stream behind the kernel of an earlier call, which may still read the buffer (a copy from pageable host
   // memory has read its source when the call returns: the runtime stages it).
   if (nfaces > c->faces_cap)
   {
      LGH_PASS(c->faces_dev.alloc(2 * (size_t)nfaces));
      c->faces_cap = nfaces;
   }
   LGH_HIP_CHECK(hipMemcpyAsync(c->faces_dev.p, faces, 2 * (size_t)nfaces * sizeof(int), hipMemcpyHostToDevice, c->stream));
   a.x = S; a.v = S + (size_t)c->H1V; a.e = S + 2 * (size_t)c->H1V; a.rho = rho_l2;
   a.xo = x_out; a.vo = v_out; a.eo = e_out; a.rhoo = rho_out; a.po = p_out;
   a.detj = detj_out; a.gradv = gradv_out; a.div = div_out; a.vort = vort_out; a.cs = cs_out; a.an = an_out;
   a.der_v = (gradv_out || div_out || vort_out) ? 1 : 0;
   a.der_x = der ? 1 : 0;
   a.val_x = x_out ? 1 : 0;
   a.val_v = v_out ? 1 : 0;
   a.need_e = (e_out || p_out || cs_out) ? 1 : 0;
   a.need_rho = (rho_out || p_out) ? 1 : 0;
   a.map = c->h1map;
   a.gamma = c->gamma;
   a.faces = c->faces_dev;
   const int NPF = ipow(R1, dim - 1);
   a.N = c->N; a.NPt = (long)nfaces * NPF;
   a.nfaces = nfaces; a.D = D; a.L = L; a.R1 = R1;
   a.stride = (int)(face_bytes / sizeof(double));
   a.FPB = std::min(patches_per_group(kSampleThreads, NPF, tab_bytes, face_bytes), nfaces);
   const size_t lds = tab_bytes + (size_t)a.FPB * face_bytes;
   const unsigned grid = (unsigned)ceil_div(nfaces, a.FPB);
   KtScope kt(c, LGH_KERNEL_FACES);
   if (dim == 3) { hipLaunchKernelGGL(sample_faces_k<3>, dim3(grid), dim3(kSampleThreads), lds, c->stream, a); }
   else { hipLaunchKernelGGL(sample_faces_k<2>, dim3(grid), dim3(kSampleThreads), lds, c->stream, a); }
   LGH_HIP_CHECK(hipGetLastError());
   return LGH_OK;
}

// The faces whose node set is the node set of no other zone's face, in ascending (e, f).  Host only: no context, no GPU.
int lgh_mesh_boundary_faces_host(int dim, int NE, int N, int D1D, const int *h1_map, int *faces_out, int *nfaces)
{
   LGH_CHECK_ARG(h1_map && faces_out && nfaces && dim >= 1 && dim <= 3 && NE > 0 && N > 0 && D1D >= 2);
   const int D = D1D, ND = ipow(D, dim), NFN = ipow(D, dim - 1), nloc = 2 * dim;
   for (size_t i = 0; i < (size_t)NE * ND; i++)
   {
      if (h1_map[i] < 0 || h1_map[i] >= N)
      {
         set_error("lgh_mesh_boundary_faces_host: h1_map[%zu] = %d is outside 0..%d", i, h1_map[i], N - 1);
         return LGH_ERR_ARG;
      }
   }
   // the sorted nodes of every face, then the faces sorted by them: equal sets stand side by side
   const size_t NFc = (size_t)NE * nloc;
   std::vector<int> nodes(NFc * NFN);
   for (int e = 0; e < NE; e++)
   {
      for (int f = 0; f < nloc; f++)
      {
         const int ax = f >> 1, fix = (f & 1) * (D - 1);
         int *out = nodes.data() + ((size_t)e * nloc + f) * NFN, n = 0;
         for (int d = 0; d < ND; d++)
         {
            const int idx[3] = {d % D, (d / D) % D, d / (D * D)};
            if (idx[ax] == fix) { out[n++] = h1_map[(size_t)e * ND + d]; }
         }
         std::sort(out, out + NFN);
      }
   }
   std::vector<size_t> ord(NFc);
   std::iota(ord.begin(), ord.end(), (size_t)0);
   auto cmp = [&](const size_t x, const size_t y) {
      return std::lexicographical_compare(nodes.begin() + x * NFN, nodes.begin() + (x + 1) * NFN, nodes.begin() + y * NFN, nodes.begin() + (y + 1) * NFN);
   };
   std::sort(ord.begin(), ord.end(), cmp);
   std::vector<char> shared(NFc, 0);
   for (size_t i = 1; i < NFc; i++)
   {
      if (!cmp(ord[i - 1], ord[i])) { shared[ord[i - 1]] = shared[ord[i]] = 1; } // (sorted: not less means equal)
   }
   int n = 0;
   for (size_t i = 0; i < NFc; i++)
   {
      if (shared[i]) { continue; }
      faces_out[2 * n] = (int)(i / nloc);
      faces_out[2 * n + 1] = (int)(i % nloc);
      n++;
   }
   *nfaces = n;
   return LGH_OK;
}
}
