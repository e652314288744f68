// lgh_derived.hip — derived flow fields on the visualisation lattice: det J, grad v, div v, vorticity, sound speed.
//
//   grad v ................ L = dv/dx = (dv/dxi) J^-1, the reference's sgrad_v before Symmetrize: Mult(dV, Jinv) in QUpdateBody,
//                          laghos_solver.cpp:1069-1168
//   sound speed ........... sqrt(gamma (gamma - 1) max(e, 0)), the S of QUpdateBody
//
// A ParaView gradient filter differentiates the piecewise-linear resampling of a dump, not the Q_k fields; the
// derivatives are formed here, where the state and the basis are, on the lattice of lgh_sample_fields (lgh_sample.hip)
// and with its structure: ZPB consecutive zones of the caller's order per workgroup, tables as kernel arguments, every
// sum over its dofs in ascending order in one thread.  What is new is the LDS a component needs - values AND
// derivatives per direction (B, G after the first axis; BB, GB, BG after the second) - so the 2 dim H1 components
// (x_0.., v_0..) are taken one per pass through the same LDS, and the dim derivatives of each at a thread's lattice
// points stay in registers (J and dv/dxi: 2 dim^2 doubles per point, at most 3 points per thread).  A last pass
// contracts e with the stages of lgh_sample_fields in its order: the same bits.  Then every thread forms det J,
// adj(J), L = (dv/dxi) adj(J) / det J and what follows from L for its points and stores them: (zone, point) is the
// fastest index, a workgroup's points are one contiguous range of every output array.  No branch looks at the sign of
// det J.  Output-bound, off the timed path.
#include "lgh_common.hpp"
#include "lgh_sample.hpp"

#include <algorithm>

namespace lgh
{

struct DerivedArgs
{
   double Th[kSampleMaxTab]; // H1 lattice table [r + R1*d]
   double Gh[kSampleMaxTab]; // its derivative
   double Tl[kSampleMaxTab]; // L2 lattice table [r + R1*l]
   const double *x, *v, *e;  // the blocks of S: component c of x at x + c*N
   double *detj, *gradv, *div, *vort, *cs;
   const int *map;
   const double *gamma;
   long N, NP;
   int NE, D, L, R1, ZPB;
   int stride;               // doubles of LDS per zone
   int need_x, need_v, need_e;
};

// The dim derivatives d u / d xi_j of one H1 component of the workgroup's zones at the lattice points of this thread,
// into g[k][j] (point i = t + k * 256 of the workgroup).  Gathers through sm; synchronises before it returns.
template <int DIM, int KMAX>
__device__ __forceinline__ void derived_component(const DerivedArgs &a, const double *__restrict__ src, const long e0, const int nz,
                                                  const double *Th, const double *Gh, double *buf, double (&g)[KMAX][DIM])
{
   const int D = a.D, R1 = a.R1, ZS = a.stride, t = threadIdx.x;
   const int ND = (DIM == 3) ? D * D * D : (DIM == 2 ? D * D : D);
   const int NPZ = (DIM == 3) ? R1 * R1 * R1 : (DIM == 2 ? R1 * R1 : R1);
   for (int i = t; i < nz * ND; i += kSampleThreads)
   {
      const int z = i / ND, d = i - z * ND;
      buf[(size_t)z * ZS + d] = src[a.map[e0 * ND + i]];
   }
   __syncthreads();
   // per zone: U | B1 G1 | BB GB BG
   double *U = buf, *B1 = U + ND, *G1 = B1 + R1 * (ND / D), *BB = G1 + R1 * (ND / D);
   double *GB = BB + R1 * R1 * D, *BG = GB + R1 * R1 * D;
   if (DIM >= 2)
   {
      sample_stage(nz, 1, 0, 1, D, R1, 1, ND / D, Th, U, ZS, B1, ZS);
      sample_stage(nz, 1, 0, 1, D, R1, 1, ND / D, Gh, U, ZS, G1, ZS);
      __syncthreads();
   }
   if (DIM == 3)
   {
      sample_stage(nz, 1, 0, 1, D, R1, R1, D, Th, B1, ZS, BB, ZS);
      sample_stage(nz, 1, 0, 1, D, R1, R1, D, Th, G1, ZS, GB, ZS);
      sample_stage(nz, 1, 0, 1, D, R1, R1, D, Gh, B1, ZS, BG, ZS);
      __syncthreads();
   }
   const int npts = nz * NPZ;
#pragma unroll
   for (int k = 0; k < KMAX; k++)
   {
      const int i = t + k * kSampleThreads;
      if (i < npts)
      {
         const int z = i / NPZ, p = i - z * NPZ;
         const size_t zo = (size_t)z * ZS;
         if constexpr (DIM == 1) { g[k][0] = sample_last(D, R1, 1, p, Gh, U + zo); }
         else if constexpr (DIM == 2)
         {
            g[k][0] = sample_last(D, R1, R1, p, Th, G1 + zo);
            g[k][1] = sample_last(D, R1, R1, p, Gh, B1 + zo);
         }
         else
         {
            g[k][0] = sample_last(D, R1, R1 * R1, p, Th, GB + zo);
            g[k][1] = sample_last(D, R1, R1 * R1, p, Th, BG + zo);
            g[k][2] = sample_last(D, R1, R1 * R1, p, Gh, BB + zo);
         }
      }
   }
   __syncthreads(); // the next pass gathers into the same LDS
}

// (det J and adj(J), the sound speed and L with what follows from it: derived_adj, derived_cs, derived_grad of lgh_sample.hpp,
// shared with the face kernel)

template <int DIM>
__global__ void __launch_bounds__(kSampleThreads) sample_derived_k(const DerivedArgs a)
{
   constexpr int KMAX = (DIM == 3) ? 3 : 1; // lattice points per thread: 9^3 points of one zone on 256 threads
   extern __shared__ double sm[];
   const int D = a.D, L = a.L, R1 = a.R1, t = threadIdx.x;
   const int NL = (DIM == 3) ? L * L * L : (DIM == 2 ? L * L : L);
   const int NPZ = (DIM == 3) ? R1 * R1 * R1 : (DIM == 2 ? R1 * R1 : R1);
   double *Th = sm, *Gh = Th + R1 * D, *Tl = Gh + R1 * D, *buf = Tl + R1 * L;
   const long e0 = (long)blockIdx.x * a.ZPB;
   const int nz = (int)min((long)a.ZPB, (long)a.NE - e0); // zones of this workgroup (the last one may hold fewer)
   const int npts = nz * NPZ;
   for (int i = t; i < R1 * D; i += kSampleThreads) { Th[i] = a.Th[i]; Gh[i] = a.Gh[i]; }
   for (int i = t; i < R1 * L; i += kSampleThreads) { Tl[i] = a.Tl[i]; }
   // (the first gather's barrier covers the tables)
   double J[KMAX][DIM][DIM], V[KMAX][DIM][DIM], ev[KMAX];
#pragma unroll
   for (int k = 0; k < KMAX; k++)
   {
      ev[k] = 0.0;
#pragma unroll
      for (int c = 0; c < DIM; c++)
      {
#pragma unroll
         for (int j = 0; j < DIM; j++) { J[k][c][j] = 0.0; V[k][c][j] = 0.0; }
      }
   }
   if (a.need_x)
   {
#pragma unroll
      for (int c = 0; c < DIM; c++)
      {
         double g[KMAX][DIM] = {};
         derived_component<DIM, KMAX>(a, a.x + (size_t)c * a.N, e0, nz, Th, Gh, buf, g);
#pragma unroll
         for (int k = 0; k < KMAX; k++)
         {
#pragma unroll
            for (int j = 0; j < DIM; j++) { J[k][c][j] = g[k][j]; }
         }
      }
   }
   if (a.need_v)
   {
#pragma unroll
      for (int c = 0; c < DIM; c++)
      {
         double g[KMAX][DIM] = {};
         derived_component<DIM, KMAX>(a, a.v + (size_t)c * a.N, e0, nz, Th, Gh, buf, g);
#pragma unroll
         for (int k = 0; k < KMAX; k++)
         {
#pragma unroll
            for (int j = 0; j < DIM; j++) { V[k][c][j] = g[k][j]; }
         }
      }
   }
   if (a.need_e)
   {
      // e as lgh_sample_fields contracts it: A holds the dofs (and, in 3D, the second stage), B the first stage
      const int ZS = a.stride, sA = max(NL, DIM == 3 ? L * R1 * R1 : 0);
      const double *src = a.e + e0 * NL;
      for (int i = t; i < nz * NL; i += kSampleThreads)
      {
         const int z = i / NL, l = i - z * NL;
         buf[(size_t)z * ZS + l] = src[i];
      }
      __syncthreads();
      const double *in = buf;
      int pre = 1, post = NL / L;
      for (int ax = 0; ax < DIM - 1; ax++)
      {
         double *out = (ax & 1) ? buf : buf + sA;
         sample_stage(nz, 1, 0, 1, L, R1, pre, post, Tl, in, ZS, out, ZS);
         __syncthreads();
         in = out;
         pre *= R1;
         post /= L;
      }
#pragma unroll
      for (int k = 0; k < KMAX; k++)
      {
         const int i = t + k * kSampleThreads;
         if (i < npts)
         {
            const int z = i / NPZ, p = i - z * NPZ;
            ev[k] = sample_last(L, R1, pre, p, Tl, in + (size_t)z * ZS);
         }
      }
   }
   // the point values: LDS is done with, registers -> global
   const size_t p0 = (size_t)e0 * NPZ, NP = (size_t)a.NP;
#pragma unroll
   for (int k = 0; k < KMAX; k++)
   {
      const int i = t + k * kSampleThreads;
      if (i >= npts) { continue; }
      const size_t pt = p0 + i;
      if (a.cs)
      {
         const double gz = a.gamma[e0 + i / NPZ];
         a.cs[pt] = derived_cs(gz, ev[k]);
      }
      if (!a.need_x) { continue; }
      double A[DIM][DIM];
      const double det = derived_adj<DIM>(J[k], A);
      if (a.detj) { a.detj[pt] = det; }
      if (!a.need_v) { continue; }
      derived_grad<DIM>(V[k], A, det, pt, NP, a.gradv, a.div, a.vort);
   }
}

} // namespace lgh

using namespace lgh;

extern "C"
{

int lgh_sample_derived(lgh_ctx *c, const double *S, int R1, const double *B_h1_lat, const double *G_h1_lat, const double *B_l2_lat,
                       double *detj_out, double *gradv_out, double *div_out, double *vort_out, double *cs_out)
{
   LGH_CHECK_ARG(c && S);
   if (!B_h1_lat || !G_h1_lat || !B_l2_lat)
   {
      set_error("lgh_sample_derived: %s is NULL", !B_h1_lat ? "B_h1_lat" : (!G_h1_lat ? "G_h1_lat" : "B_l2_lat"));
      return LGH_ERR_ARG;
   }
   LGH_PASS(lattice_r1("lgh_sample_derived", R1));
   const int dim = c->dim, D = c->D1D, L = c->L1D;
   if (dim == 1 && vort_out)
   {
      set_error("lgh_sample_derived: vort_out: there is no vorticity in 1D");
      return LGH_ERR_ARG;
   }
   DerivedArgs a;
   memset(&a, 0, sizeof(a));
   LGH_PASS(lattice_tables("lgh_sample_derived", c, R1, B_h1_lat, G_h1_lat, B_l2_lat, a.Th, a.Gh, a.Tl));
   if (!detj_out && !gradv_out && !div_out && !vort_out && !cs_out) { return LGH_OK; }
   const int NPZ = ipow(R1, dim);
   a.x = S; a.v = S + (size_t)c->H1V; a.e = S + 2 * (size_t)c->H1V;
   a.detj = detj_out; a.gradv = gradv_out; a.div = div_out; a.vort = vort_out; a.cs = cs_out;
   a.need_v = (gradv_out || div_out || vort_out) ? 1 : 0;
   a.need_x = (a.need_v || detj_out) ? 1 : 0;
   a.need_e = cs_out ? 1 : 0;
   a.map = c->h1map;
   a.gamma = c->gamma;
   a.N = c->N; a.NP = (long)c->NE * NPZ;
   a.NE = c->NE; a.D = D; a.L = L; a.R1 = R1;
   // LDS per zone: one H1 component with its stages - the dofs, B and G after the first axis, BB, GB and BG after the
   // second - or e with the two buffers of lgh_sample_fields, whichever is larger
   const int h1 = ipow(D, dim) + (dim >= 2 ? 2 * R1 * ipow(D, dim - 1) : 0) + (dim == 3 ? 3 * R1 * R1 * D : 0);
   const int l2 = std::max(ipow(L, dim), dim == 3 ? L * R1 * R1 : 0) + (dim >= 2 ? ipow(L, dim - 1) * R1 : 0);
   a.stride = std::max(h1, l2);
   const size_t zone_bytes = (size_t)a.stride * sizeof(double), tab_bytes = (size_t)R1 * (2 * D + L) * sizeof(double);
   LGH_PASS(lattice_lds_fits("lgh_sample_derived", "zone", c, R1, zone_bytes + tab_bytes));
   // several zones per workgroup where a zone's lattice is smaller than the workgroup, as far as 48 KB of LDS go
   a.ZPB = std::min(patches_per_group(kSampleThreads, NPZ, tab_bytes, zone_bytes), c->NE);
   const size_t lds = tab_bytes + (size_t)a.ZPB * zone_bytes;
   const unsigned grid = (unsigned)ceil_div(c->NE, a.ZPB);
   KtScope kt(c, LGH_KERNEL_DERIVED);
   if (dim == 3) { hipLaunchKernelGGL(sample_derived_k<3>, dim3(grid), dim3(kSampleThreads), lds, c->stream, a); }
   else if (dim == 2) { hipLaunchKernelGGL(sample_derived_k<2>, dim3(grid), dim3(kSampleThreads), lds, c->stream, a); }
   else { hipLaunchKernelGGL(sample_derived_k<1>, dim3(grid), dim3(kSampleThreads), lds, c->stream, a); }
   LGH_HIP_CHECK(hipGetLastError());
   return LGH_OK;
}
}
