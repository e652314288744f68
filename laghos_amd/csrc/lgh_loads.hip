// lgh_loads.hip — pressure loads on lists of zone faces (lgh_loads; the driver's `-loads`): per row of the caller's choosing the
// count, the area, the force sum w p N, sum w p |N|, the power sum w p (v.N), the swept volume sum w (v.N), sum w (x.N) and
// the extremes of p over the tensor Gauss points of the context's own 1-D rule on the faces listed under that row.
//
// Point evaluation: both 1-D bases interpolate at the end points of the reference interval (Gauss-Lobatto Lagrange for H1,
// Bernstein for L2), so on the side xi_a = s of a zone every trace is a contraction of the FACE LAYER of dofs alone -
// D1D^(dim-1) per H1 component, L1D^(dim-1) for e and rho - over the dim - 1 tangential axes, and the area vector needs
// tangential derivatives only: N = sgn t_b (x) t_c in 3D (b < c the tangential axes; the sign flips for a = 1, whose pair
// (0, 2) is an odd permutation), sgn (t_y, -t_x) turned with the axis in 2D - row a of adj(J), Nanson, with no branch on a
// determinant.  The tangents are formed from the offsets x - x_first of the face's nodes, as ZoneEval forms its Jacobian.
// A workgroup of 256 threads takes FPB faces (as many as fit 256 points and 48 KB of LDS) without gathering a whole zone;
// the fields - dim components of x, dim of v, e, rho - go one per pass through the same LDS and a thread keeps the values
// of its ONE point in registers, as in lgh_faces.hip.
//
// Reduction: the exact binned sums of lgh_binsum.hpp, which describes the scheme, with eight sum columns.  With at most 64
// rows nearly every wavefront holds one row, so the wavefront scatters by row as lgh_map.hip does by cell
// (prof_scatter_cells); after kLoadsFold distinct rows the lanes left send their own atomics.  p may be negative or zero (a
// projected density can undershoot), so the extremes go through the key that orders ALL doubles (ProfKeyOrdered) where the
// profiles take the bits of a positive density as they are.  No floating-point atomic: the same bits for every face order,
// numbering, launch grid and rank count.
#include "lgh_binsum.hpp"
#include "lgh_sample.hpp"

#include <cmath>

namespace lgh
{

constexpr int kLoadsSums = 8; // area force_x force_y force_z pa power flux xn: columns 1..8 of a row
constexpr int kLoadsFold = 8; // distinct rows a wavefront folds before its remaining lanes send their own atomics
constexpr int kLoadsThreads = 256;
static_assert(kLoadsSums + 3 == LGH_LOADS_COLS, "a row: n, the sums, p_min, p_max");

struct LoadsArgs
{
   const double *S, *rho, *B, *G, *Bl, *w1, *gamma;
   const int *map, *faces; // faces: the device copy of the list, 3 ints per face: zone, local face, row
   long N;
   int nfaces, D, Q, L, FPB, stride;
   ProfScratch s;
};

struct LoadsTabs { const double *B, *G, *Bl; };

// the zone-local dof (n per direction) of entry i = i_b + n i_c of the face layer on side s of axis ax
template <int DIM>
__device__ __forceinline__ int loads_face_dof(const int n, const int ax, const int s, const int i)
{
   const int fix = s * (n - 1);
   if (DIM == 2) { return (ax == 0) ? fix + n * i : i + n * fix; }
   const int ib = i % n, ic = i / n;
   return (ax == 0) ? fix + n * (ib + n * ic) : ((ax == 1) ? ib + n * (fix + n * ic) : ib + n * (ic + n * fix));
}

// One field of the workgroup's faces at this thread's point.  kind 0: a component of x, as offsets from the face's first
// node, with its derivatives gb, gc along the tangential axes; 1: a component of v; 2: an L2 field (e, rho).  Per face in
// LDS: the face layer | B u | G u over the first tangential axis (3D).  Ends with a barrier: the next pass reuses the LDS.
template <int DIM>
__device__ __forceinline__ void loads_field(const LoadsArgs &a, const LoadsTabs &tb, const int *meta, double *buf, const int nf, const int kind,
                                            const double *__restrict__ src, double &val, double &gb, double &gc)
{
   const int t = threadIdx.x, Q = a.Q, ZS = a.stride, n = (kind == 2) ? a.L : a.D;
   const int NF = (DIM == 3) ? n * n : n, NZ = NF * n;
   const int oB = (DIM == 3) ? a.D * a.D : a.D, oG = oB + Q * a.D;
   const double *T = (kind == 2) ? tb.Bl : tb.B;
   for (int i = t; i < nf * NF; i += kLoadsThreads)
   {
      const int z = i / NF, d = i - z * NF;
      const long e = meta[4 * z];
      const int f = meta[4 * z + 1], ax = f >> 1, s = f & 1;
      const int loc = loads_face_dof<DIM>(n, ax, s, d);
      double u;
      if (kind == 2) { u = src[(size_t)e * NZ + loc]; }
      else
      {
         const int *zm = a.map + (size_t)e * NZ;
         u = src[zm[loc]];
         if (kind == 0) { u -= src[zm[loads_face_dof<DIM>(n, ax, s, 0)]]; }
      }
      buf[(size_t)z * ZS + d] = u;
   }
   __syncthreads();
   if (DIM == 3)
   {
      const int S1 = Q * n;
      for (int i = t; i < nf * S1; i += kLoadsThreads)
      {
         const int z = i / S1, o = i - z * S1, qb = o % Q, ic = o / Q;
         double *U = buf + (size_t)z * ZS;
         const double *u = U + n * ic;
         double sb = 0.0, sg = 0.0;
         for (int ib = 0; ib < n; ib++) { sb += T[qb + Q * ib] * u[ib]; }
         U[oB + o] = sb;
         if (kind == 0)
         {
            for (int ib = 0; ib < n; ib++) { sg += tb.G[qb + Q * ib] * u[ib]; }
            U[oG + o] = sg;
         }
      }
      __syncthreads();
   }
   val = 0.0; gb = 0.0; gc = 0.0;
   const int NPF = (DIM == 3) ? Q * Q : Q;
   if (t < nf * NPF)
   {
      const int z = t / NPF, p = t - z * NPF;
      const double *U = buf + (size_t)z * ZS;
      if (DIM == 2)
      {
         for (int d = 0; d < n; d++) { val += T[p + Q * d] * U[d]; }
         if (kind == 0)
         {
            for (int d = 0; d < n; d++) { gb += tb.G[p + Q * d] * U[d]; }
         }
      }
      else
      {
         const int qb = p % Q, qc = p / Q;
         const double *uB = U + oB + qb, *uG = U + oG + qb;
         for (int ic = 0; ic < n; ic++) { val += T[qc + Q * ic] * uB[Q * ic]; }
         if (kind == 0)
         {
            for (int ic = 0; ic < n; ic++) { gb += T[qc + Q * ic] * uG[Q * ic]; }
            for (int ic = 0; ic < n; ic++) { gc += tb.G[qc + Q * ic] * uB[Q * ic]; }
         }
      }
   }
   __syncthreads();
}

template <int DIM, int PASS>
__global__ void __launch_bounds__(kLoadsThreads) loads_faces_k(const LoadsArgs a)
{
   extern __shared__ double sm[];
   const int D = a.D, Q = a.Q, L = a.L, t = threadIdx.x, lane = t & 63;
   const int NPF = (DIM == 3) ? Q * Q : Q;
   double *B = sm, *G = B + Q * D, *Bl = G + Q * D, *w1 = Bl + Q * L, *red = w1 + Q;
   int *meta = reinterpret_cast<int *>(red + kProfRed); // per face of the workgroup: zone, local face, row, -
   double *buf = red + kProfRed + 2 * a.FPB;
   const long k0 = (long)blockIdx.x * a.FPB;
   const int nf = (int)min((long)a.FPB, (long)a.nfaces - k0); // >= 1: the grid covers the list and no more
   for (int i = t; i < Q * D; i += kLoadsThreads) { B[i] = a.B[i]; G[i] = a.G[i]; }
   for (int i = t; i < Q * L; i += kLoadsThreads) { Bl[i] = a.Bl[i]; }
   for (int i = t; i < Q; i += kLoadsThreads) { w1[i] = a.w1[i]; }
   if (t < nf)
   {
      for (int j = 0; j < 3; j++) { meta[4 * t + j] = a.faces[3 * (k0 + t) + j]; }
      meta[4 * t + 3] = 0;
   }
   __syncthreads();
   const LoadsTabs tb = {B, G, Bl};
   double X[DIM], Tb[DIM], Tc[DIM], V[DIM], ev, rv, dum0, dum1;
#pragma unroll
   for (int c = 0; c < DIM; c++) { loads_field<DIM>(a, tb, meta, buf, nf, 0, a.S + (size_t)c * a.N, X[c], Tb[c], Tc[c]); }
#pragma unroll
   for (int c = 0; c < DIM; c++) { loads_field<DIM>(a, tb, meta, buf, nf, 1, a.S + (size_t)(DIM + c) * a.N, V[c], dum0, dum1); }
   loads_field<DIM>(a, tb, meta, buf, nf, 2, a.S + (size_t)2 * DIM * a.N, ev, dum0, dum1);
   loads_field<DIM>(a, tb, meta, buf, nf, 2, a.rho, rv, dum0, dum1);
   // ---- the point: every thread of a wavefront goes on (the folds below need all 64 lanes)
   const bool live = t < nf * NPF;
   const int z = live ? t / NPF : 0, p = live ? t - z * NPF : 0;
   const long e = meta[4 * z];
   const int f = meta[4 * z + 1], ax = f >> 1, row = meta[4 * z + 2];
   const double sgn = (f & 1) ? 1.0 : -1.0;
   const double w = (DIM == 3) ? w1[p % Q] * w1[p / Q] : w1[p];
   double Nv[DIM];
   {
      const int *zm = a.map + (size_t)e * ((DIM == 3) ? D * D * D : D * D);
      const int first = zm[loads_face_dof<DIM>(D, ax, f & 1, 0)];
#pragma unroll
      for (int c = 0; c < DIM; c++) { X[c] += a.S[(size_t)c * a.N + first]; }
   }
   if constexpr (DIM == 2)
   {
      // a = 0: the tangent runs along y, N = sgn (J11, -J01); a = 1: along x, N = sgn (-J10, J00)
      const double o = (ax == 0) ? sgn : -sgn;
      Nv[0] = o * Tb[1];
      Nv[1] = -o * Tb[0];
   }
   else
   {
      const double o = (ax == 1) ? -sgn : sgn;
      Nv[0] = o * (Tb[1] * Tc[2] - Tb[2] * Tc[1]);
      Nv[1] = o * (Tb[2] * Tc[0] - Tb[0] * Tc[2]);
      Nv[2] = o * (Tb[0] * Tc[1] - Tb[1] * Tc[0]);
   }
   bool fin = isfinite(ev) && isfinite(rv);
   double n2 = 0.0, vn = 0.0, xn = 0.0;
#pragma unroll
   for (int c = 0; c < DIM; c++)
   {
      fin = fin && isfinite(X[c]) && isfinite(V[c]) && isfinite(Nv[c]);
      n2 += Nv[c] * Nv[c];
      vn += V[c] * Nv[c];
      xn += X[c] * Nv[c];
   }
   const bool ok = live && fin;
   const double nrm = sqrt(n2), pr = sample_pressure(a.gamma[e], rv, ev), wp = w * pr;
   double ad[kLoadsSums];
   ad[0] = w * nrm;
#pragma unroll
   for (int c = 0; c < 3; c++) { ad[1 + c] = (c < DIM) ? wp * Nv[c < DIM ? c : 0] : 0.0; }
   ad[4] = wp * nrm;
   ad[5] = wp * vn;
   ad[6] = w * vn;
   ad[7] = w * xn;
   if (PASS == 0)
   {
      double mx[kLoadsSums];
#pragma unroll
      for (int k = 0; k < kLoadsSums; k++)
      {
         const double m = fabs(ad[k]);
         mx[k] = (ok && m < INFINITY) ? m : 0.0;
      }
      prof_store_maxima<kLoadsSums>(a.s, mx, red);
      return;
   }
   int E[kLoadsSums];
#pragma unroll
   for (int k = 0; k < kLoadsSums; k++) { E[k] = prof_window(a.s.neg[k]); }
   const bool ext = ok && pr == pr; // (a NaN pressure - an overflowed product times zero - has no place in an order)
   const unsigned long long key = ProfKeyOrdered::key(pr);
   // (columns 1 + DIM .. 3: a force component above the dimension, nothing but zeros)
   prof_scatter_cells<kLoadsSums, 1 + DIM, 4>(a.s, ok, row, ext ? ~key : 0ULL, ext ? key : 0ULL, ad, E, kLoadsFold, lane);
   const long long n = wave_sum_i64((live && !ok) ? 1LL : 0LL);
   if (lane == 0 && n != 0) { prof_add((long long *)a.s.excl, n); }
}

// what the launch is sized with: the bytes of the tables (with the kProfRed doubles of the reduction) and of one face in LDS
static void loads_lds(const int dim, const int D, const int Q, const int L, size_t *tab_bytes, size_t *face_bytes)
{
   *tab_bytes = ((size_t)Q * (2 * D + L) + Q + kProfRed) * sizeof(double);
   *face_bytes = (size_t)(2 + ipow(D, dim - 1) + (dim == 3 ? 2 * Q * D : 0)) * sizeof(double); // (two words in front: zone, face, row)
}
// faces per workgroup: as many as fit 256 points and 48 KB of LDS, one where they do not
static int loads_fpb(const int dim, const int Q, const size_t tab_bytes, const size_t face_bytes)
{
   return patches_per_group(kLoadsThreads, ipow(Q, dim - 1), tab_bytes, face_bytes);
}

// why a context cannot take the call at all, or LGH_OK
static int loads_supported(lgh_ctx *c, const char *who, size_t *tab_bytes, size_t *face_bytes)
{
   if (c->dim == 1)
   {
      set_error("%s: dim = 1: loads are taken on the faces of 2D and 3D zones", who);
      return LGH_ERR_ARG;
   }
   if (!c->w1d)
   {
      set_error("%s: the quadrature rule of this context (Q1D = %d) is not a tensor product of a 1-D rule (w1d is not set)", who, c->Q1D);
      return LGH_ERR_UNSUPPORTED;
   }
   loads_lds(c->dim, c->D1D, c->Q1D, c->L1D, tab_bytes, face_bytes);
   if (*tab_bytes + *face_bytes > 64 * 1024 || ipow(c->Q1D, c->dim - 1) > kLoadsThreads)
   {
      set_error("%s: one face of a zone of D1D = %d on Q1D = %d points needs %zu bytes of LDS and %d threads", who, c->D1D, c->Q1D,
                *tab_bytes + *face_bytes, ipow(c->Q1D, c->dim - 1));
      return LGH_ERR_UNSUPPORTED;
   }
   return LGH_OK;
}

} // namespace lgh

using namespace lgh;

extern "C"
{

int lgh_loads_fpb(lgh_ctx *c, int *fpb)
{
   LGH_CHECK_ARG(c && fpb);
   size_t tab_bytes, face_bytes;
   LGH_PASS(loads_supported(c, "lgh_loads_fpb", &tab_bytes, &face_bytes));
   *fpb = loads_fpb(c->dim, c->Q1D, tab_bytes, face_bytes);
   return LGH_OK;
}

int lgh_loads(lgh_ctx *c, const double *S, const double *rho_l2, int nrows, int nfaces, const int *faces, double *out, long *n_excluded)
{
   LGH_CHECK_ARG(c);
   const int dim = c->dim;
   if (dim == 1)
   {
      set_error("lgh_loads: dim = 1: loads are taken on the faces of 2D and 3D zones");
      return LGH_ERR_ARG;
   }
   if (!S || !rho_l2 || !out || !n_excluded)
   {
      set_error("lgh_loads: %s is NULL", !S ? "S" : (!rho_l2 ? "rho_l2" : (!out ? "out" : "n_excluded")));
      return LGH_ERR_ARG;
   }
   if (nrows < 1 || nrows > LGH_LOADS_MAX_ROWS)
   {
      set_error("lgh_loads: nrows = %d is outside 1..%d", nrows, LGH_LOADS_MAX_ROWS);
      return LGH_ERR_ARG;
   }
   if (nfaces < 0)
   {
      set_error("lgh_loads: nfaces = %d", nfaces);
      return LGH_ERR_ARG;
   }
   if (nfaces > 0 && !faces)
   {
      set_error("lgh_loads: faces is NULL with nfaces = %d", nfaces);
      return LGH_ERR_ARG;
   }
   for (int k = 0; k < nfaces; k++)
   {
      const int e = faces[3 * k], f = faces[3 * k + 1], r = faces[3 * k + 2];
      if (e < 0 || e >= c->NE)
      {
         set_error("lgh_loads: faces[%d]: zone %d is outside 0..%d", 3 * k, e, c->NE - 1);
         return LGH_ERR_ARG;
      }
      if (f < 0 || f >= 2 * dim)
      {
         set_error("lgh_loads: faces[%d]: local face %d is outside 0..%d", 3 * k + 1, f, 2 * dim - 1);
         return LGH_ERR_ARG;
      }
      if (r < 0 || r >= nrows)
      {
         set_error("lgh_loads: faces[%d]: row %d is outside 0..%d", 3 * k + 2, r, nrows - 1);
         return LGH_ERR_ARG;
      }
   }
   size_t tab_bytes, face_bytes;
   LGH_PASS(loads_supported(c, "lgh_loads", &tab_bytes, &face_bytes));
   // scratch for the most rows a call may ask for, allocated at the first call; the list on the device, regrown for a longer one
   LoadsArgs a;
   LGH_PASS(prof_scratch<kLoadsSums>(c->loads_dev, c->loads_rows, LGH_LOADS_MAX_ROWS, a.s));
   if (nfaces > c->loads_cap)
   {
      c->loads_cap = 0;
      LGH_PASS(c->loads_faces.alloc(3 * (size_t)nfaces));
      c->loads_cap = nfaces;
   }
   if (nfaces > 0) { LGH_HIP_CHECK(hipMemcpyAsync(c->loads_faces.p, faces, 3 * (size_t)nfaces * sizeof(int), hipMemcpyHostToDevice, c->stream)); }
   a.S = S; a.rho = rho_l2; a.B = c->B; a.G = c->G; a.Bl = c->Bl; a.w1 = c->w1d; a.gamma = c->gamma;
   a.map = c->h1map; a.faces = c->loads_faces;
   a.N = c->N; a.nfaces = nfaces; a.D = c->D1D; a.Q = c->Q1D; a.L = c->L1D;
   a.FPB = std::max(1, std::min(loads_fpb(dim, c->Q1D, tab_bytes, face_bytes), nfaces));
   a.stride = (int)(face_bytes / sizeof(double)) - 2;
   const size_t lds = tab_bytes + (size_t)a.FPB * face_bytes;
   const unsigned grid = (unsigned)ceil_div(nfaces, a.FPB);
   auto launch = [&](const int pass) {
      if (dim == 3) { hipLaunchKernelGGL((pass ? loads_faces_k<3, 1> : loads_faces_k<3, 0>), dim3(grid), dim3(kLoadsThreads), lds, c->stream, a); }
      else { hipLaunchKernelGGL((pass ? loads_faces_k<2, 1> : loads_faces_k<2, 0>), dim3(grid), dim3(kLoadsThreads), lds, c->stream, a); }
   };
   return prof_run<kLoadsSums, ProfKeyOrdered>(c, a.s, nrows, LGH_KERNEL_LOADS, nfaces > 0, launch, out, n_excluded);
}
}
