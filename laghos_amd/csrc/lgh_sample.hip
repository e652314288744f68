// lgh_sample.hip — visualisation sampling: the fields of a state on a lattice of R1 points per direction in every zone.
//
//   stands in for ........ VisItDataCollection::Save and the refresh of rho_gf in front of it,
//                          /root/reference/laghos.cpp:691-701 (cycle 0), :819-871 (every vis_steps steps)
//   pressure .............. the equation of state of QUpdateBody, /root/reference/laghos_solver.cpp:1069-1168:
//                          p = (gamma_z - 1) rho max(e, 0)
//
// The reference hands its grid functions to MFEM's data collections, which evaluate them on the host when a file is
// written.  Here the state lives on the GPU and the lattice values are what a VTK file of linear cells needs (points
// duplicated zone by zone, laghos_amd/host/vtk_output.cpp), so they are formed where the state is: one kernel gathers
// the zone's dofs - 2 dim H1 components (x, v) and two L2 fields (e, rho) - into LDS and contracts them with the 1-D
// tables direction by direction (sum factorisation: D^dim -> R1 D^(dim-1) -> ... -> R1^dim, n multiply-adds per entry
// of every stage instead of D^dim per point).  Zones are taken in the caller's order, ZPB consecutive ones per
// workgroup where a zone's lattice is smaller than the workgroup: the lattice points of a workgroup are then one
// contiguous range of every output array and consecutive lanes store consecutive doubles.  Every sum runs over its
// dofs in ascending order in one thread: the same input gives the same bits.  Output-bound, off the timed path.
#include "lgh_common.hpp"
#include "lgh_sample.hpp"

#include <algorithm>

namespace lgh
{

// Everything one launch needs, by value: the tables travel as kernel arguments (2 x 648 bytes), so nothing is uploaded,
// nothing is kept between calls and nothing is remembered about the caller's arrays.
struct SampleArgs
{
   double Th[kSampleMaxTab]; // H1 lattice table [r + R1*d]
   double Tl[kSampleMaxTab]; // L2 lattice table [r + R1*l]
   const double *h1src[6];   // scalar node arrays: x_0.., v_0..
   double *h1out[6];         // their lattice arrays (NP each)
   const double *l2src[2];   // e, rho dofs
   double *e_out, *rho_out, *p_out;
   const int *map;
   const double *gamma;
   int nh, nl;               // H1 / L2 fields in flight
   int NE, D, L, R1, ZPB;
   int strideA, strideB;     // doubles per (zone, field) in the two LDS buffers
};

template <int DIM>
__global__ void __launch_bounds__(kSampleThreads) sample_fields_k(const SampleArgs a)
{
   extern __shared__ double sm[];
   const int D = a.D, L = a.L, R1 = a.R1, nh = a.nh, nl = a.nl, NF = nh + nl;
   const int ND = (DIM == 3) ? D * D * D : (DIM == 2 ? D * D : D), NL = (DIM == 3) ? L * L * L : (DIM == 2 ? L * L : L);
   const int NPZ = (DIM == 3) ? R1 * R1 * R1 : (DIM == 2 ? R1 * R1 : R1);
   double *Th = sm, *Tl = Th + R1 * D, *bufA = Tl + R1 * L, *bufB = bufA + (size_t)a.ZPB * NF * a.strideA;
   const int t = threadIdx.x;
   const long e0 = (long)blockIdx.x * a.ZPB;
   const int nz = (int)min((long)a.ZPB, (long)a.NE - e0); // zones of this workgroup (the last one may hold fewer)
   for (int i = t; i < R1 * D; i += kSampleThreads) { Th[i] = a.Th[i]; }
   for (int i = t; i < R1 * L; i += kSampleThreads) { Tl[i] = a.Tl[i]; }
   // gather: the map entries of the workgroup's zones are one contiguous range
   if (nh > 0)
   {
      for (int i = t; i < nz * ND; i += kSampleThreads)
      {
         const int z = i / ND, d = i - z * ND;
         const int node = a.map[e0 * ND + i];
         for (int f = 0; f < nh; f++) { bufA[(size_t)(z * NF + f) * a.strideA + d] = a.h1src[f][node]; }
      }
   }
   for (int f = 0; f < nl; f++)
   {
      const double *src = a.l2src[f] + e0 * NL;
      for (int i = t; i < nz * NL; i += kSampleThreads)
      {
         const int z = i / NL, l = i - z * NL;
         bufA[(size_t)(z * NF + nh + f) * a.strideA + l] = src[i];
      }
   }
   __syncthreads();
   // all axes but the last: LDS -> LDS, the two buffers alternate
   const double *in = bufA;
   int sin = a.strideA;
   int preH = 1, postH = (DIM == 3) ? D * D : (DIM == 2 ? D : 1), postL = (DIM == 3) ? L * L : (DIM == 2 ? L : 1);
   for (int ax = 0; ax < DIM - 1; ax++)
   {
      double *out = (ax & 1) ? bufA : bufB;
      const int sout = (ax & 1) ? a.strideA : a.strideB;
      sample_stage(nz, nh, 0, NF, D, R1, preH, postH, Th, in, sin, out, sout);
      sample_stage(nz, nl, nh, NF, L, R1, preH, postL, Tl, in, sin, out, sout);
      __syncthreads();
      in = out;
      sin = sout;
      preH *= R1;
      postH /= D;
      postL /= L;
   }
   // last axis: LDS -> global; (zone, point) is the fastest index and a contiguous range of every output
   const size_t p0 = (size_t)e0 * NPZ;
   const int npts = nz * NPZ;
   for (int i = t; i < nh * npts; i += kSampleThreads)
   {
      const int f = i / npts, zp = i - f * npts, z = zp / NPZ, p = zp - z * NPZ;
      a.h1out[f][p0 + zp] = sample_last(D, R1, preH, p, Th, in + (size_t)(z * NF + f) * sin);
   }
   if (nl > 0)
   {
      for (int zp = t; zp < npts; zp += kSampleThreads)
      {
         const int z = zp / NPZ, p = zp - z * NPZ;
         const double ev = sample_last(L, R1, preH, p, Tl, in + (size_t)(z * NF + nh) * sin);
         if (a.e_out) { a.e_out[p0 + zp] = ev; }
         if (nl > 1)
         {
            const double rv = sample_last(L, R1, preH, p, Tl, in + (size_t)(z * NF + nh + 1) * sin);
            if (a.rho_out) { a.rho_out[p0 + zp] = rv; }
            if (a.p_out) { a.p_out[p0 + zp] = sample_pressure(a.gamma[e0 + z], rv, ev); }
         }
      }
   }
}

} // namespace lgh

using namespace lgh;

extern "C"
{

int lgh_sample_fields(lgh_ctx *c, const double *S, const double *rho_l2, int R1, const double *B_h1_lat, const double *B_l2_lat,
                      double *x_out, double *v_out, double *e_out, double *rho_out, double *p_out)
{
   LGH_CHECK_ARG(c && S && B_h1_lat && B_l2_lat);
   LGH_PASS(lattice_r1("lgh_sample_fields", R1));
   if (!rho_l2 && (rho_out || p_out))
   {
      set_error("lgh_sample_fields: %s needs the density dofs, but rho_l2 is NULL", rho_out ? "rho_out" : "p_out");
      return LGH_ERR_ARG;
   }
   const int dim = c->dim, D = c->D1D, L = c->L1D;
   SampleArgs a;
   memset(&a, 0, sizeof(a));
   LGH_PASS(lattice_tables("lgh_sample_fields", c, R1, B_h1_lat, nullptr, B_l2_lat, a.Th, nullptr, a.Tl));
   if (!x_out && !v_out && !e_out && !rho_out && !p_out) { return LGH_OK; }
   const int NPZ = ipow(R1, dim);
   const size_t NP = (size_t)c->NE * NPZ;
   for (int k = 0; k < dim; k++)
   {
      if (x_out) { a.h1src[a.nh] = S + (size_t)k * c->N; a.h1out[a.nh++] = x_out + k * NP; }
   }
   for (int k = 0; k < dim; k++)
   {
      if (v_out) { a.h1src[a.nh] = S + (size_t)(dim + k) * c->N; a.h1out[a.nh++] = v_out + k * NP; }
   }
   if (e_out || rho_out || p_out)
   {
      a.l2src[a.nl++] = S + 2 * (size_t)c->H1V;
      if (rho_out || p_out) { a.l2src[a.nl++] = rho_l2; }
   }
   a.e_out = e_out; a.rho_out = rho_out; a.p_out = p_out;
   a.map = c->h1map;
   a.gamma = c->gamma;
   a.NE = c->NE; a.D = D; a.L = L; a.R1 = R1;
   // LDS per (zone, field): A holds the dofs (n^dim, n = max(D1D, L1D)) and, in 3D, the result of the second stage (n R1^2); B the result of the first
   const int nmax = std::max(D, L);
   a.strideA = std::max(ipow(nmax, dim), dim == 3 ? nmax * R1 * R1 : 0);
   a.strideB = (dim >= 2) ? ipow(nmax, dim - 1) * R1 : 0;
   const int NF = a.nh + a.nl;
   const size_t zone_bytes = (size_t)NF * (a.strideA + a.strideB) * sizeof(double);
   const size_t tab_bytes = (size_t)R1 * (D + L) * sizeof(double);
   LGH_PASS(lattice_lds_fits("lgh_sample_fields", "zone", c, R1, zone_bytes + tab_bytes));
   // several zones per workgroup where a zone's lattice is smaller than the workgroup, as far as 48 KB of LDS go
   a.ZPB = std::min(patches_per_group(kSampleThreads, NPZ, tab_bytes, zone_bytes), c->NE);
   const size_t lds = tab_bytes + (size_t)a.ZPB * zone_bytes;
   const unsigned grid = (unsigned)ceil_div(c->NE, a.ZPB);
   KtScope kt(c, LGH_KERNEL_SAMPLE);
   if (dim == 3) { hipLaunchKernelGGL(sample_fields_k<3>, dim3(grid), dim3(kSampleThreads), lds, c->stream, a); }
   else if (dim == 2) { hipLaunchKernelGGL(sample_fields_k<2>, dim3(grid), dim3(kSampleThreads), lds, c->stream, a); }
   else { hipLaunchKernelGGL(sample_fields_k<1>, dim3(grid), dim3(kSampleThreads), lds, c->stream, a); }
   LGH_HIP_CHECK(hipGetLastError());
   return LGH_OK;
}
}
