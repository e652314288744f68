// lgh_1d.hip — the 1D path of liblaghos_hip.so (README run 5, 1D Sedov).
//
// The reference runs every 1D problem with full assembly: `-pa` with dim 1 switches to FA (laghos.cpp:454-462).  In 1D the
// FA operators are the PA ones with one exception, the energy solve: FA inverts the zone mass matrices Me(z) once at set-up
// (laghos_solver.cpp:203-215) and applies them zone by zone (:501-515) instead of running an energy CG.  This file holds
// every kernel of that path; the C entry points of lgh_api.hip / lgh_velocity.hip / lgh_energy.hip / lgh_sedov.hip send a context with dim == 1 here and the
// 2D/3D kernels never see one.
//
// Layouts (include/laghos_hip.h): S = [x | v | e] with offsets {0, N, 2N}; stressJinvT[e*NQ + q], Jac0inv[e*NQ + q],
// rho0DetJ0w[e*NQ + q]; L2 dofs e*L1D + l; H1 element dofs e*D1D + d through h1_map.
//
// Kept simple on purpose (tuning 1D is out of scope): fp64, wave64, 256-thread workgroups, one zone or one point per lane,
// tables read from global memory with compile-time sizes so that every small array lives in registers.  Every sum runs in
// a fixed order and there are no floating-point atomics: a node takes its element contributions in ascending E-vector
// position (an interior vertex: the last dof of the zone on its left, then the first dof of the zone on its right), the
// reductions go through the library's fixed-order block / grid trees (lgh_common.hpp), and the velocity CG runs in ONE
// workgroup with block-tree dot products - the same input gives the same bits on every run.
#include <algorithm>
#include <cmath>
#include <limits>
#include <type_traits>

#include "lgh_common.hpp"

namespace lgh
{

// (kernel ids: (1<<8)|(D1D<<4)|Q1D, the orders of the 2D/3D tables - visit_order, lgh_common.hpp)

static int zone_grid(const lgh_ctx *c) { return ceil_div(c->NE, 256); }

// sum over the (256-thread) workgroup, returned in every thread; red >= 17 doubles of LDS
__device__ __forceinline__ double all_sum(const double v, double *red)
{
   const double s = block_sum(v, red); // (valid in thread 0)
   if (threadIdx.x == 0) { red[16] = s; }
   __syncthreads();
   const double r = red[16];
   __syncthreads();
   return r;
}

// smooth_step_01 of laghos_solver.cpp:797-805
__device__ __forceinline__ double smooth_step_01(const double x, const double eps)
{
   const double y = (x + eps) / (2.0 * eps);
   if (y < 0.0) { return 0.0; }
   if (y > 1.0) { return 1.0; }
   return (3.0 - 2.0 * y) * y * y;
}

// In-register Cholesky factor of the n x n SPD matrix M (row-major): F[i][j] (j < i) the factor, F[j][j] = 1 / L_jj.
template <int n> __device__ __forceinline__ void cholesky(const double (&M)[n][n], double (&F)[n][n])
{
#pragma unroll
   for (int j = 0; j < n; j++)
   {
      double d = M[j][j];
#pragma unroll
      for (int k = 0; k < j; k++) { d -= F[j][k] * F[j][k]; }
      const double r = 1.0 / sqrt(d); // (d <= 0: not SPD - NaN, which every consumer then shows)
      F[j][j] = r;
#pragma unroll
      for (int i = j + 1; i < n; i++)
      {
         double s = M[i][j];
#pragma unroll
         for (int k = 0; k < j; k++) { s -= F[i][k] * F[j][k]; }
         F[i][j] = s * r;
      }
   }
}
// x = (L L^T)^-1 b with the factor of cholesky()
template <int n> __device__ __forceinline__ void cholesky_solve(const double (&F)[n][n], const double (&b)[n], double (&x)[n])
{
   double z[n];
#pragma unroll
   for (int i = 0; i < n; i++)
   {
      double s = b[i];
#pragma unroll
      for (int k = 0; k < i; k++) { s -= F[i][k] * z[k]; }
      z[i] = s * F[i][i];
   }
#pragma unroll
   for (int i = n - 1; i >= 0; i--)
   {
      double s = z[i];
#pragma unroll
      for (int k = i + 1; k < n; k++) { s -= F[k][i] * x[k]; }
      x[i] = s * F[i][i];
   }
}

// ---- Rho0DetJ0Vol (laghos_solver.cpp:223-250, the branch 1D takes): Jac0inv, rho0DetJ0w, the mass data, the volume -------
template <int D, int Q>
__global__ void __launch_bounds__(256)
setup_1d_k(const int NE, const int *__restrict__ map, const double *__restrict__ G, const double *__restrict__ Bl,
           const double *__restrict__ W, const double *__restrict__ x0, const double *__restrict__ rho0_l2,
           const double *__restrict__ rho0_q, double *__restrict__ Jac0inv, double *__restrict__ rdw, double *__restrict__ massD,
           double *partials, unsigned int *ticket, double *vol_out)
{
   constexpr int L = D - 1;
   __shared__ double red[17];
   const int e = blockIdx.x * 256 + threadIdx.x;
   double part = 0.0;
   if (e < NE)
   {
      double xe[D], re[L];
#pragma unroll
      for (int d = 0; d < D; d++) { xe[d] = x0[map[(size_t)e * D + d]]; }
#pragma unroll
      for (int l = 0; l < L; l++) { re[l] = rho0_l2[(size_t)e * L + l]; }
#pragma unroll
      for (int q = 0; q < Q; q++)
      {
         double J = 0.0, rv = 0.0;
#pragma unroll
         for (int d = 0; d < D; d++) { J += G[q + Q * d] * xe[d]; }
#pragma unroll
         for (int l = 0; l < L; l++) { rv += Bl[q + Q * l] * re[l]; }
         const size_t eq = (size_t)e * Q + q;
         const double w = W[q];
         Jac0inv[eq] = 1.0 / J;
         rdw[eq] = w * rv * J;           // rho0 grid function (L2) at the point
         massD[eq] = w * J * rho0_q[eq]; // rho0 coefficient at the point (the mass integrators' rho0_coeff)
         part += w * J;
      }
   }
   const double bsum = block_sum(part, red);
   double total;
   if (grid_sum_last_block(bsum, partials, ticket, red, total))
   {
      if (threadIdx.x == 0) { *vol_out = total; }
   }
}

// ---- H1 mass: element contributions, and the node sum in ascending E-vector order -----------------------------------------
template <int D, int Q>
__global__ void __launch_bounds__(256)
h1_mass_e_1d_k(const int NE, const int *__restrict__ map, const double *__restrict__ B, const double *__restrict__ massD,
               const double *__restrict__ x, double *__restrict__ yE)
{
   const int e = blockIdx.x * 256 + threadIdx.x;
   if (e >= NE) { return; }
   double xe[D], ye[D];
#pragma unroll
   for (int d = 0; d < D; d++) { xe[d] = x[map[(size_t)e * D + d]]; ye[d] = 0.0; }
#pragma unroll
   for (int q = 0; q < Q; q++)
   {
      double u = 0.0;
#pragma unroll
      for (int d = 0; d < D; d++) { u += B[q + Q * d] * xe[d]; }
      u *= massD[(size_t)e * Q + q];
#pragma unroll
      for (int d = 0; d < D; d++) { ye[d] += B[q + Q * d] * u; }
   }
#pragma unroll
   for (int d = 0; d < D; d++) { yE[(size_t)e * D + d] = ye[d]; }
}
// Jacobi diagonal contributions: sum_q B(q,d)^2 D(q)
template <int D, int Q>
__global__ void __launch_bounds__(256)
h1_diag_e_1d_k(const int NE, const double *__restrict__ B, const double *__restrict__ massD, double *__restrict__ yE)
{
   const int e = blockIdx.x * 256 + threadIdx.x;
   if (e >= NE) { return; }
#pragma unroll
   for (int d = 0; d < D; d++)
   {
      double s = 0.0;
#pragma unroll
      for (int q = 0; q < Q; q++) { s += B[q + Q * d] * B[q + Q * d] * massD[(size_t)e * Q + q]; }
      yE[(size_t)e * D + d] = s;
   }
}
// y[n] = sum of the E-vector entries of node n in ascending position (CSR transpose of h1_map); ess rows -> 0
__global__ void __launch_bounds__(256)
gather_1d_k(const int N, const int *__restrict__ off, const int *__restrict__ idx, const double *__restrict__ yE,
            const uint8_t *__restrict__ ess, double *__restrict__ y)
{
   const int n = blockIdx.x * 256 + threadIdx.x;
   if (n >= N) { return; }
   double s = 0.0;
   for (int k = off[n]; k < off[n + 1]; k++) { s += yE[idx[k]]; }
   if (ess && ess[n]) { s = 0.0; }
   y[n] = s;
}
__global__ void __launch_bounds__(256) reciprocal_1d_k(const int n, const double *__restrict__ x, double *__restrict__ y)
{
   const int i = blockIdx.x * 256 + threadIdx.x;
   if (i < n) { y[i] = 1.0 / x[i]; }
}

// ---- L2 mass: apply, and the Cholesky factors of the zone matrices Me(z) (laghos_solver.cpp:203-215) ------------------------
template <int L, int Q>
__global__ void __launch_bounds__(256)
l2_mass_1d_k(const int NE, const double *__restrict__ Bl, const double *__restrict__ massD, const double *__restrict__ x,
             double *__restrict__ y)
{
   const int e = blockIdx.x * 256 + threadIdx.x;
   if (e >= NE) { return; }
   double xe[L], ye[L];
#pragma unroll
   for (int l = 0; l < L; l++) { xe[l] = x[(size_t)e * L + l]; ye[l] = 0.0; }
#pragma unroll
   for (int q = 0; q < Q; q++)
   {
      double u = 0.0;
#pragma unroll
      for (int l = 0; l < L; l++) { u += Bl[q + Q * l] * xe[l]; }
      u *= massD[(size_t)e * Q + q];
#pragma unroll
      for (int l = 0; l < L; l++) { ye[l] += Bl[q + Q * l] * u; }
   }
#pragma unroll
   for (int l = 0; l < L; l++) { y[(size_t)e * L + l] = ye[l]; }
}
template <int L, int Q>
__global__ void __launch_bounds__(256)
l2_factor_1d_k(const int NE, const double *__restrict__ Bl, const double *__restrict__ massD, double *__restrict__ fac)
{
   const int e = blockIdx.x * 256 + threadIdx.x;
   if (e >= NE) { return; }
   double M[L][L], F[L][L];
#pragma unroll
   for (int i = 0; i < L; i++)
#pragma unroll
      for (int j = 0; j < L; j++) { M[i][j] = 0.0; F[i][j] = 0.0; }
#pragma unroll
   for (int q = 0; q < Q; q++)
   {
      const double m = massD[(size_t)e * Q + q];
#pragma unroll
      for (int i = 0; i < L; i++)
#pragma unroll
         for (int j = 0; j < L; j++) { M[i][j] += Bl[q + Q * i] * Bl[q + Q * j] * m; }
   }
   cholesky<L>(M, F);
#pragma unroll
   for (int i = 0; i < L; i++)
#pragma unroll
      for (int j = 0; j < L; j++) { fac[(size_t)e * L * L + i * L + j] = F[i][j]; }
}
// de_z = Me(z)^-1 rhs_z (laghos_solver.cpp:501-515).  FORM: rhs_z = (F^T v)_z [+ e_source_z] formed here from the stress
// (ForceIntegrator, laghos_assembly.cpp:43-78, transposed) and written to e_rhs; otherwise rhs = b.
template <int D, int Q, bool FORM>
__global__ void __launch_bounds__(256)
energy_solve_1d_k(const int NE, const int *__restrict__ map, const double *__restrict__ G, const double *__restrict__ Bl,
                  const double *__restrict__ sJ, const double *__restrict__ v, const double *__restrict__ src,
                  const double *__restrict__ b, double *__restrict__ e_rhs, const double *__restrict__ fac, double *__restrict__ x)
{
   constexpr int L = D - 1;
   const int e = blockIdx.x * 256 + threadIdx.x;
   if (e >= NE) { return; }
   double rhs[L];
   if constexpr (FORM)
   {
      double ve[D];
#pragma unroll
      for (int d = 0; d < D; d++) { ve[d] = v[map[(size_t)e * D + d]]; }
#pragma unroll
      for (int l = 0; l < L; l++) { rhs[l] = 0.0; }
#pragma unroll
      for (int q = 0; q < Q; q++)
      {
         double g = 0.0;
#pragma unroll
         for (int d = 0; d < D; d++) { g += G[q + Q * d] * ve[d]; }
         const double s = sJ[(size_t)e * Q + q] * g;
#pragma unroll
         for (int l = 0; l < L; l++) { rhs[l] += Bl[q + Q * l] * s; }
      }
#pragma unroll
      for (int l = 0; l < L; l++)
      {
         if (src) { rhs[l] += src[(size_t)e * L + l]; }
         e_rhs[(size_t)e * L + l] = rhs[l];
      }
   }
   else
   {
#pragma unroll
      for (int l = 0; l < L; l++) { rhs[l] = b[(size_t)e * L + l]; }
   }
   double F[L][L], out[L];
#pragma unroll
   for (int i = 0; i < L; i++)
#pragma unroll
      for (int j = 0; j < L; j++) { F[i][j] = fac[(size_t)e * L * L + i * L + j]; }
   cholesky_solve<L>(F, rhs, out);
#pragma unroll
   for (int l = 0; l < L; l++) { x[(size_t)e * L + l] = out[l]; }
}

// ---- ForceIntegrator (laghos_assembly.cpp:43-78): F x as element contributions, F^T v -----------------------------------
template <int D, int Q>
__global__ void __launch_bounds__(256)
force_e_1d_k(const int NE, const double *__restrict__ G, const double *__restrict__ Bl, const double *__restrict__ sJ,
             const double *__restrict__ x_l2, double *__restrict__ yE)
{
   constexpr int L = D - 1;
   const int e = blockIdx.x * 256 + threadIdx.x;
   if (e >= NE) { return; }
   double xl[L], yd[D];
#pragma unroll
   for (int l = 0; l < L; l++) { xl[l] = x_l2[(size_t)e * L + l]; }
#pragma unroll
   for (int d = 0; d < D; d++) { yd[d] = 0.0; }
#pragma unroll
   for (int q = 0; q < Q; q++)
   {
      double u = 0.0;
#pragma unroll
      for (int l = 0; l < L; l++) { u += Bl[q + Q * l] * xl[l]; }
      const double s = sJ[(size_t)e * Q + q] * u;
#pragma unroll
      for (int d = 0; d < D; d++) { yd[d] += G[q + Q * d] * s; }
   }
#pragma unroll
   for (int d = 0; d < D; d++) { yE[(size_t)e * D + d] = yd[d]; }
}
template <int D, int Q>
__global__ void __launch_bounds__(256)
force_t_1d_k(const int NE, const int *__restrict__ map, const double *__restrict__ G, const double *__restrict__ Bl,
             const double *__restrict__ sJ, const double *__restrict__ v, double *__restrict__ y)
{
   constexpr int L = D - 1;
   const int e = blockIdx.x * 256 + threadIdx.x;
   if (e >= NE) { return; }
   double ve[D], yl[L];
#pragma unroll
   for (int d = 0; d < D; d++) { ve[d] = v[map[(size_t)e * D + d]]; }
#pragma unroll
   for (int l = 0; l < L; l++) { yl[l] = 0.0; }
#pragma unroll
   for (int q = 0; q < Q; q++)
   {
      double g = 0.0;
#pragma unroll
      for (int d = 0; d < D; d++) { g += G[q + Q * d] * ve[d]; }
      const double s = sJ[(size_t)e * Q + q] * g;
#pragma unroll
      for (int l = 0; l < L; l++) { yl[l] += Bl[q + Q * l] * s; }
   }
#pragma unroll
   for (int l = 0; l < L; l++) { y[(size_t)e * L + l] = yl[l]; }
}

// ---- UpdateQuadratureData: the point physics of QUpdateBody (laghos_solver.cpp:1069-1168) with the 1D details of the
// FA loop (:807-985): e clamped at 0, the trivial eigen-decomposition, h = h0 |Jpi dir| / |dir|, h_min = |J| / order_v,
// dt_est = 0 wherever detJ < 0.  One zone per lane; the estimate is folded into qdata.dt_est by a grid minimum.
struct QArgs1D
{
   int NE, N, visc;
   const int *map;
   const double *G, *Bl, *W, *gamma, *rdw, *Jac0inv, *S;
   double h0, cfl, h1order;
   double *sJ, *partials, *dt_est;
   unsigned int *ticket;
};
template <int D, int Q>
__global__ void __launch_bounds__(256) qupdate_1d_k(const QArgs1D a)
{
   constexpr int L = D - 1;
   __shared__ double red[17];
   const int e = blockIdx.x * 256 + threadIdx.x;
   double cand = __builtin_inf();
   if (e < a.NE)
   {
      const double *x = a.S, *v = a.S + a.N, *en = a.S + 2 * (size_t)a.N;
      double xe[D], ve[D], ee[L];
#pragma unroll
      for (int d = 0; d < D; d++)
      {
         const int n = a.map[(size_t)e * D + d];
         xe[d] = x[n];
         ve[d] = v[n];
      }
#pragma unroll
      for (int l = 0; l < L; l++) { ee[l] = en[(size_t)e * L + l]; }
      const double gamma = a.gamma[e];
#pragma unroll
      for (int q = 0; q < Q; q++)
      {
         double J = 0.0, dv = 0.0, ev = 0.0;
#pragma unroll
         for (int d = 0; d < D; d++)
         {
            J += a.G[q + Q * d] * xe[d];
            dv += a.G[q + Q * d] * ve[d];
         }
#pragma unroll
         for (int l = 0; l < L; l++) { ev += a.Bl[q + Q * l] * ee[l]; }
         const size_t eq = (size_t)e * Q + q;
         const double weight = a.W[q];
         const double detJ = J, Jinv = 1.0 / J;
         const double R = (1.0 / weight) * a.rdw[eq] / detJ;
         const double E = fmax(0.0, ev);
         const double P = (gamma - 1.0) * R * E;
         const double S = sqrt(gamma * (gamma - 1.0) * E);
         double stress = -P, visc_coeff = 0.0;
         if (a.visc)
         {
            const double sgrad_v = dv * Jinv; // (symmetric already; its eigenvalue is itself, eigenvector 1, vorticity_coeff 1)
            const double mu = sgrad_v;
            const double Jpi = J * a.Jac0inv[eq];
            const double H = a.h0 * fabs(Jpi); // h0 |Jpi dir| / |dir| with dir = 1
            visc_coeff = 2.0 * R * H * H * fabs(mu);
            const double eps = 1e-12;
            visc_coeff += 0.5 * R * H * S * (1.0 - smooth_step_01(mu - 2.0 * eps, eps));
            stress += visc_coeff * sgrad_v;
         }
         const double h_min = fabs(J) / a.h1order;
         const double ih_min = 1.0 / h_min;
         const double irho_ih_min_sq = ih_min * ih_min / R;
         const double idt = S * ih_min + 2.5 * visc_coeff * irho_ih_min_sq;
         if (detJ < 0.0) { cand = 0.0; } // forces the repetition of the step with a smaller dt
         else if (idt > 0.0) { cand = fmin(cand, a.cfl / idt); }
         a.sJ[eq] = (stress * Jinv) * (weight * detJ);
      }
   }
   const double bmin = block_min(cand, red);
   double total;
   if (grid_min_last_block(bmin, a.partials, a.ticket, red, total))
   {
      if (threadIdx.x == 0) { *a.dt_est = fmin(*a.dt_est, total); }
   }
}

// ---- ComputeDensity (laghos_solver.cpp:542-563): rho_z = M_z^-1 b_z on the current mesh, b_i = sum_q rho0DetJ0w psi_i ---
template <int D, int Q>
__global__ void __launch_bounds__(256)
density_1d_k(const int NE, const int *__restrict__ map, const double *__restrict__ G, const double *__restrict__ Bl,
             const double *__restrict__ W, const double *__restrict__ x, const double *__restrict__ rdw, double *__restrict__ rho)
{
   constexpr int L = D - 1;
   const int e = blockIdx.x * 256 + threadIdx.x;
   if (e >= NE) { return; }
   double xe[D], M[L][L], F[L][L], b[L], out[L];
#pragma unroll
   for (int d = 0; d < D; d++) { xe[d] = x[map[(size_t)e * D + d]]; }
#pragma unroll
   for (int i = 0; i < L; i++)
   {
      b[i] = 0.0;
#pragma unroll
      for (int j = 0; j < L; j++) { M[i][j] = 0.0; F[i][j] = 0.0; }
   }
#pragma unroll
   for (int q = 0; q < Q; q++)
   {
      double J = 0.0;
#pragma unroll
      for (int d = 0; d < D; d++) { J += G[q + Q * d] * xe[d]; }
      const double wd = W[q] * J, r = rdw[(size_t)e * Q + q];
#pragma unroll
      for (int i = 0; i < L; i++)
      {
         const double pi = Bl[q + Q * i];
#pragma unroll
         for (int j = 0; j < L; j++) { M[i][j] += pi * Bl[q + Q * j] * wd; }
         b[i] += pi * r;
      }
   }
   cholesky<L>(M, F);
   cholesky_solve<L>(F, b, out);
#pragma unroll
   for (int l = 0; l < L; l++) { rho[(size_t)e * L + l] = out[l]; }
}

// ---- InternalEnergy / KineticEnergy (laghos_solver.cpp:581-595, :640-697): sum_q rho0DetJ0w f(q), f = e or |v|^2 --------
template <int D, int Q, int WHICH>
__global__ void __launch_bounds__(256)
energy_1d_k(const int NE, const int *__restrict__ map, const double *__restrict__ B, const double *__restrict__ Bl,
            const double *__restrict__ rdw, const double *__restrict__ vec, double *partials, unsigned int *ticket, double *out)
{
   constexpr int L = D - 1;
   __shared__ double red[17];
   const int e = blockIdx.x * 256 + threadIdx.x;
   double part = 0.0;
   if (e < NE)
   {
      if (WHICH == 0)
      {
         double ee[L];
#pragma unroll
         for (int l = 0; l < L; l++) { ee[l] = vec[(size_t)e * L + l]; }
#pragma unroll
         for (int q = 0; q < Q; q++)
         {
            double f = 0.0;
#pragma unroll
            for (int l = 0; l < L; l++) { f += Bl[q + Q * l] * ee[l]; }
            part += f * rdw[(size_t)e * Q + q];
         }
      }
      else
      {
         double ve[D];
#pragma unroll
         for (int d = 0; d < D; d++) { ve[d] = vec[map[(size_t)e * D + d]]; }
#pragma unroll
         for (int q = 0; q < Q; q++)
         {
            double f = 0.0;
#pragma unroll
            for (int d = 0; d < D; d++) { f += B[q + Q * d] * ve[d]; }
            part += (f * f) * rdw[(size_t)e * Q + q];
         }
      }
   }
   const double bsum = block_sum(part, red);
   double total;
   if (grid_sum_last_block(bsum, partials, ticket, red, total))
   {
      if (threadIdx.x == 0) { *out = total; }
   }
}

// ---- `-err` (laghos.cpp:1027-1080) in 1D: the points of the error rule, then the integrand zone by zone -------------------
// point p of zone e at [e*n1 + p]: r = |x(p) - x0|, rho_h(p), w_p detJ(p); the exact density at those radii comes from
// lgh_sedov_eval (the GPU evaluator of SedovSol::EvalSol) in between.
template <int D>
__global__ void __launch_bounds__(256)
sedov_points_1d_k(const int NE, const int n1, const int *__restrict__ map, const double *__restrict__ Bt,
                  const double *__restrict__ Gt, const double *__restrict__ Blt, const double *__restrict__ w1,
                  const double *__restrict__ x, const double *__restrict__ rho_l2, const double ox, double *__restrict__ r,
                  double *__restrict__ rho_h, double *__restrict__ wdet)
{
   constexpr int L = D - 1;
   const long i = (long)blockIdx.x * 256 + threadIdx.x;
   if (i >= (long)NE * n1) { return; }
   const int e = (int)(i / n1), p = (int)(i - (long)e * n1);
   double X = 0.0, J = 0.0, rh = 0.0;
#pragma unroll
   for (int d = 0; d < D; d++)
   {
      const double xd = x[map[(size_t)e * D + d]];
      X += xd * Bt[p + n1 * d];
      J += xd * Gt[p + n1 * d];
   }
#pragma unroll
   for (int l = 0; l < L; l++) { rh += rho_l2[(size_t)e * L + l] * Blt[p + n1 * l]; }
   r[i] = fabs(X - ox);
   rho_h[i] = rh;
   wdet[i] = w1[p] * J;
}
__global__ void __launch_bounds__(256)
sedov_err_1d_k(const int NE, const int n1, const double *__restrict__ rho_x, const double *__restrict__ rho_h,
               const double *__restrict__ wdet, double *partials, unsigned int *ticket, double *out)
{
   __shared__ double red[17];
   const int e = blockIdx.x * 256 + threadIdx.x;
   double part = 0.0;
   if (e < NE)
   {
      for (int p = 0; p < n1; p++)
      {
         const size_t i = (size_t)e * n1 + p;
         const double diff = rho_x[i] - rho_h[i];
         part += wdet[i] * (diff * diff);
      }
   }
   const double bsum = block_sum(part, red);
   double total;
   if (grid_sum_last_block(bsum, partials, ticket, red, total))
   {
      if (threadIdx.x == 0) { *out = total; }
   }
}

// ---- CG (upstream CGSolver::Mult) in ONE workgroup: no host look until it has finished ----------------------
// H1: MassPAOperator::Mult with the essential rows of the active component eliminated, Jacobi preconditioner (the FA solve's
// HypreSmoother Jacobi, one sweep, on the system FormLinearSystem eliminated - laghos_solver.cpp:418-433 - gives the same
// iterates: the essential entries of r, z and d stay 0); L2: plain CG.  Dot products: each lane sums its strided entries in
// order, then the fixed wave / block tree.
struct Cg1dArgs
{
   int NE, n;
   const int *map, *off, *idx;   // H1 only
   const double *T, *massD;      // basis table (B or Bl), mass data
   const uint8_t *ess;           // essential rows (H1) or nullptr
   const double *dinv;           // Jacobi or nullptr
   const double *b;
   double *x, *r, *z, *d, *y, *yE;
   double rel_tol2;
   int max_iter, x_zero;
   CgScalars *cgs;
};
// out = A in; ends with a barrier
template <int NN, int Q, bool H1> __device__ void cg1d_apply(const Cg1dArgs &a, const double *in, double *out)
{
   __syncthreads();
   for (int e = threadIdx.x; e < a.NE; e += 256)
   {
      double xe[NN], ye[NN];
#pragma unroll
      for (int i = 0; i < NN; i++)
      {
         xe[i] = H1 ? in[a.map[(size_t)e * NN + i]] : in[(size_t)e * NN + i];
         ye[i] = 0.0;
      }
#pragma unroll
      for (int q = 0; q < Q; q++)
      {
         double u = 0.0;
#pragma unroll
         for (int i = 0; i < NN; i++) { u += a.T[q + Q * i] * xe[i]; }
         u *= a.massD[(size_t)e * Q + q];
#pragma unroll
         for (int i = 0; i < NN; i++) { ye[i] += a.T[q + Q * i] * u; }
      }
#pragma unroll
      for (int i = 0; i < NN; i++) { (H1 ? a.yE : out)[(size_t)e * NN + i] = ye[i]; }
   }
   if (H1)
   {
      __syncthreads();
      for (int n = threadIdx.x; n < a.n; n += 256)
      {
         double s = 0.0;
         for (int k = a.off[n]; k < a.off[n + 1]; k++) { s += a.yE[a.idx[k]]; }
         if (a.ess && a.ess[n]) { s = 0.0; }
         out[n] = s;
      }
   }
   __syncthreads();
}
template <int NN, int Q, bool H1>
__global__ void __launch_bounds__(256) cg1d_k(const Cg1dArgs a)
{
   __shared__ double red[17];
   const int t = threadIdx.x, n = a.n;
   const bool prec = (a.dinv != nullptr);
   // r = b - A x (iterative_mode), or r = b and x = 0
   if (a.x_zero)
   {
      for (int i = t; i < n; i += 256) { a.x[i] = 0.0; a.r[i] = a.b[i]; }
   }
   else
   {
      cg1d_apply<NN, Q, H1>(a, a.x, a.y);
      for (int i = t; i < n; i += 256) { a.r[i] = a.b[i] - a.y[i]; }
   }
   double p = 0.0;
   for (int i = t; i < n; i += 256)
   {
      const double zi = prec ? a.r[i] * a.dinv[i] : a.r[i];
      a.z[i] = zi;
      a.d[i] = zi;
      p += zi * a.r[i];
   }
   double nom = all_sum(p, red);
   const double r0 = fmax(nom * a.rel_tol2, 0.0);
   int fin = 0;
   if (!(nom < 0.0) && !(nom <= r0))
   {
      cg1d_apply<NN, Q, H1>(a, a.d, a.y);
      p = 0.0;
      for (int i = t; i < n; i += 256) { p += a.y[i] * a.d[i]; }
      double den = all_sum(p, red);
      if (den != 0.0)
      {
         fin = a.max_iter;
         for (int it = 1;;)
         {
            const double alpha = nom / den;
            p = 0.0;
            for (int i = t; i < n; i += 256)
            {
               a.x[i] = a.x[i] + alpha * a.d[i];
               const double ri = a.r[i] - alpha * a.y[i];
               a.r[i] = ri;
               const double zi = prec ? ri * a.dinv[i] : ri;
               a.z[i] = zi;
               p += ri * zi;
            }
            const double betanom = all_sum(p, red);
            if (betanom < 0.0 || betanom <= r0) { fin = it; break; }
            if (++it > a.max_iter) { break; }
            const double beta = betanom / nom;
            for (int i = t; i < n; i += 256) { a.d[i] = a.z[i] + beta * a.d[i]; }
            cg1d_apply<NN, Q, H1>(a, a.d, a.y);
            p = 0.0;
            for (int i = t; i < n; i += 256) { p += a.d[i] * a.y[i]; }
            den = all_sum(p, red);
            if (den == 0.0) { fin = it; break; }
            nom = betanom;
         }
      }
   }
   if (t == 0)
   {
      a.cgs->iters = fin;
      a.cgs->done = 1;
   }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
// lgh_create for dim == 1 (the arguments have been checked there).  What a 2D/3D context builds beyond this
// (lockstep solve tables, fused force products, second stream) has no 1D use.
int create_1d(const lgh_config *cfg, lgh_ctx *c)
{
   std::vector<int> off, idx; // (the transpose of the restriction on the host: no use here)
   LGH_PASS(create_common(cfg, c, off, idx));
   const int L = c->L1D, NE = c->NE, N = c->N;
   const size_t nq = (size_t)NE * c->Q1D;
   LGH_PASS(ctx_buffer(c->stressJinvT, nq));
   LGH_PASS(ctx_buffer(c->Jac0inv, nq));
   LGH_PASS(ctx_buffer(c->rho0DetJ0w, nq));
   LGH_PASS(ctx_buffer(c->massD, nq));
   LGH_PASS(ctx_buffer(c->me_fac, (size_t)NE * L * L));
   LGH_PASS(ctx_buffer(c->diagV, (size_t)N));
   LGH_PASS(ctx_buffer(c->dinvV, (size_t)N));
   LGH_PASS(ctx_buffer(c->dev_flags, (size_t)8));
   LGH_PASS(ctx_buffer(c->YE, std::max((size_t)NE * c->D1D, (size_t)c->L2V)));
   const size_t nv = std::max<size_t>((size_t)N, (size_t)c->L2V);
   LGH_PASS(ctx_buffer(c->cg_r, nv));
   LGH_PASS(ctx_buffer(c->cg_z, nv));
   LGH_PASS(ctx_buffer(c->cg_d0, nv));
   LGH_PASS(ctx_buffer(c->cg_y, nv));
   return LGH_OK;
}

// the Jacobi diagonal of the H1 mass and the factors of the zone mass matrices, from the current mass data
int mass_changed_1d(lgh_ctx *c)
{
   return visit_order(c->kid, [&](auto Dc, auto Qc, auto) {
      constexpr int D = decltype(Dc)::value, Q = decltype(Qc)::value;
      hipLaunchKernelGGL((h1_diag_e_1d_k<D, Q>), dim3(zone_grid(c)), dim3(256), 0, c->stream, c->NE, c->B, c->massD, c->YE);
      hipLaunchKernelGGL(gather_1d_k, dim3(ceil_div(c->N, 256)), dim3(256), 0, c->stream, c->N, c->t_off, c->t_idx, c->YE,
                         (const uint8_t *)nullptr, c->diagV);
      hipLaunchKernelGGL(reciprocal_1d_k, dim3(ceil_div(c->N, 256)), dim3(256), 0, c->stream, c->N, c->diagV, c->dinvV);
      hipLaunchKernelGGL((l2_factor_1d_k<D - 1, Q>), dim3(zone_grid(c)), dim3(256), 0, c->stream, c->NE, c->Bl, c->massD,
                         c->me_fac);
      LGH_HIP_CHECK(hipGetLastError());
      c->mass_gen++;
      return LGH_OK;
   });
}

int setup_1d(lgh_ctx *c, const double *x0, const double *rho0_l2, const double *rho0_q, double *volume)
{
   const int rc = visit_order(c->kid, [&](auto Dc, auto Qc, auto) {
      constexpr int D = decltype(Dc)::value, Q = decltype(Qc)::value;
      hipLaunchKernelGGL((setup_1d_k<D, Q>), dim3(zone_grid(c)), dim3(256), 0, c->stream, c->NE, c->h1map, c->G, c->Bl, c->W,
                         x0, rho0_l2, rho0_q, c->Jac0inv, c->rho0DetJ0w, c->massD, c->partials, c->tickets, c->scal);
      LGH_HIP_CHECK(hipGetLastError());
      return LGH_OK;
   });
   if (rc) { return rc; }
   LGH_HIP_CHECK(hipMemcpyAsync(c->host_pinned + kPinResult, c->scal, sizeof(double), hipMemcpyDeviceToHost, c->stream));
   const int rc2 = mass_changed_1d(c);
   if (rc2) { return rc2; }
   LGH_HIP_CHECK(hipStreamSynchronize(c->stream));
   *volume = c->host_pinned[kPinResult];
   c->stress_current = 0;
   return LGH_OK;
}

int force_mult_1d(lgh_ctx *c, const double *x_l2, double *y_h1)
{
   return visit_order(c->kid, [&](auto Dc, auto Qc, auto) {
      constexpr int D = decltype(Dc)::value, Q = decltype(Qc)::value;
      hipLaunchKernelGGL((force_e_1d_k<D, Q>), dim3(zone_grid(c)), dim3(256), 0, c->stream, c->NE, c->G, c->Bl, c->stressJinvT,
                         x_l2, c->YE);
      hipLaunchKernelGGL(gather_1d_k, dim3(ceil_div(c->N, 256)), dim3(256), 0, c->stream, c->N, c->t_off, c->t_idx, c->YE,
                         (const uint8_t *)nullptr, y_h1);
      LGH_HIP_CHECK(hipGetLastError());
      return LGH_OK;
   });
}

int force_mult_t_1d(lgh_ctx *c, const double *v_h1, double *y_l2)
{
   return visit_order(c->kid, [&](auto Dc, auto Qc, auto) {
      constexpr int D = decltype(Dc)::value, Q = decltype(Qc)::value;
      hipLaunchKernelGGL((force_t_1d_k<D, Q>), dim3(zone_grid(c)), dim3(256), 0, c->stream, c->NE, c->h1map, c->G, c->Bl,
                         c->stressJinvT, v_h1, y_l2);
      LGH_HIP_CHECK(hipGetLastError());
      return LGH_OK;
   });
}

int mass_apply_1d(lgh_ctx *c, int space, const double *x, double *y, bool eliminate)
{
   return visit_order(c->kid, [&](auto Dc, auto Qc, auto) {
      constexpr int D = decltype(Dc)::value, Q = decltype(Qc)::value;
      if (space == LGH_SPACE_H1)
      {
         hipLaunchKernelGGL((h1_mass_e_1d_k<D, Q>), dim3(zone_grid(c)), dim3(256), 0, c->stream, c->NE, c->h1map, c->B, c->massD,
                            x, c->YE);
         const uint8_t *ess = (eliminate && c->cur_ess >= 0) ? c->essmask[c->cur_ess] : nullptr;
         hipLaunchKernelGGL(gather_1d_k, dim3(ceil_div(c->N, 256)), dim3(256), 0, c->stream, c->N, c->t_off, c->t_idx, c->YE, ess, y);
      }
      else
      {
         hipLaunchKernelGGL((l2_mass_1d_k<D - 1, Q>), dim3(zone_grid(c)), dim3(256), 0, c->stream, c->NE, c->Bl, c->massD, x, y);
      }
      LGH_HIP_CHECK(hipGetLastError());
      return LGH_OK;
   });
}

int l2_solve_local_1d(lgh_ctx *c, const double *b, double *x)
{
   return visit_order(c->kid, [&](auto Dc, auto Qc, auto) {
      constexpr int D = decltype(Dc)::value, Q = decltype(Qc)::value;
      hipLaunchKernelGGL((energy_solve_1d_k<D, Q, false>), dim3(zone_grid(c)), dim3(256), 0, c->stream, c->NE, c->h1map, c->G,
                         c->Bl, c->stressJinvT, (const double *)nullptr, (const double *)nullptr, b, (double *)nullptr, c->me_fac, x);
      LGH_HIP_CHECK(hipGetLastError());
      return LGH_OK;
   });
}

int cg_1d(lgh_ctx *c, int space, const double *b, double *x, double rel_tol, int max_iter, int *iters, bool x_is_zero)
{
   const bool h1 = (space == LGH_SPACE_H1);
   Cg1dArgs a;
   memset(&a, 0, sizeof(a));
   a.NE = c->NE;
   a.n = h1 ? c->N : c->L2V;
   a.map = c->h1map;
   a.off = c->t_off;
   a.idx = c->t_idx;
   a.T = h1 ? c->B : c->Bl;
   a.massD = c->massD;
   a.ess = (h1 && c->cur_ess >= 0) ? c->essmask[c->cur_ess] : nullptr;
   a.dinv = h1 ? c->dinvV : nullptr;
   a.b = b;
   a.x = x;
   a.r = c->cg_r;
   a.z = c->cg_z;
   a.d = c->cg_d0;
   a.y = c->cg_y;
   a.yE = c->YE;
   a.rel_tol2 = rel_tol * rel_tol;
   a.max_iter = max_iter;
   a.x_zero = (x_is_zero || !h1) ? 1 : 0; // (the L2 solve starts from x = 0: CG_EMass.iterative_mode = false)
   a.cgs = c->cgs;
   const int rc = visit_order(c->kid, [&](auto Dc, auto Qc, auto) {
      constexpr int D = decltype(Dc)::value, Q = decltype(Qc)::value;
      if (h1) { hipLaunchKernelGGL((cg1d_k<D, Q, true>), dim3(1), dim3(256), 0, c->stream, a); }
      else { hipLaunchKernelGGL((cg1d_k<D - 1, Q, false>), dim3(1), dim3(256), 0, c->stream, a); }
      LGH_HIP_CHECK(hipGetLastError());
      return LGH_OK;
   });
   if (rc) { return rc; }
   CgScalars *hs = (CgScalars *)c->host_pinned;
   LGH_HIP_CHECK(hipMemcpyAsync(hs, c->cgs, sizeof(CgScalars), hipMemcpyDeviceToHost, c->stream));
   LGH_HIP_CHECK(hipStreamSynchronize(c->stream));
   if (iters) { *iters = hs->iters; }
   return LGH_OK;
}

int qupdate_1d(lgh_ctx *c, const double *S)
{
   QArgs1D a;
   a.NE = c->NE; a.N = c->N; a.visc = c->visc ? 1 : 0;
   a.map = c->h1map;
   a.G = c->G; a.Bl = c->Bl; a.W = c->W; a.gamma = c->gamma; a.rdw = c->rho0DetJ0w; a.Jac0inv = c->Jac0inv; a.S = S;
   a.h0 = c->h0; a.cfl = c->cfl; a.h1order = c->h1order;
   a.sJ = c->stressJinvT; a.partials = c->partials; a.ticket = c->tickets; a.dt_est = c->dt_est_dev;
   const int rc = visit_order(c->kid, [&](auto Dc, auto Qc, auto) {
      constexpr int D = decltype(Dc)::value, Q = decltype(Qc)::value;
      hipLaunchKernelGGL((qupdate_1d_k<D, Q>), dim3(zone_grid(c)), dim3(256), 0, c->stream, a);
      LGH_HIP_CHECK(hipGetLastError());
      return LGH_OK;
   });
   if (rc) { return rc; }
   c->stress_current = 1;
   return LGH_OK;
}

// SolveVelocity, FA branch (laghos_solver.cpp:400-439): rhs = -F 1 with the essential rows zeroed (FormLinearSystem with
// dv = 0), dv from the Jacobi CG started at 0
int solve_velocity_1d(lgh_ctx *c, const double *ones, double *dv, double *rhs, double rel_tol, int max_iter, int *h1_iters)
{
   int rc = vec_set(c, dv, 0.0, c->N); // :338
   if (rc) { return rc; }
   RoctxRange range("SolveVelocity-Force"); // :404
   timer_start(c);
   rc = force_mult_1d(c, ones, rhs); // :405
   timer_stop(c, 2);
   if (rc) { return rc; }
   rc = vec_neg_inplace(c, rhs, c->N); // :409
   if (rc) { return rc; }
   rc = vec_zero_list(c, rhs, c->ess[0], c->ess_count[0]); // :419
   if (rc) { return rc; }
   c->cur_ess = 0;
   int it = 0;
   timer_start(c);
   rc = cg_1d(c, LGH_SPACE_H1, rhs, dv, rel_tol, max_iter, &it, true); // :433
   timer_stop(c, 0);
   if (rc) { return rc; }
   c->timers.c[0] += it; // :437
   if (h1_iters) { *h1_iters += it; }
   return LGH_OK;
}

// SolveEnergy, FA branch (laghos_solver.cpp:491-516): e_rhs = F^T v (+ source) and de_z = Me(z)^-1 e_rhs_z in one kernel;
// L2iter goes up by one per zone (:513).  (The force product is timed inside the L2 region.)
int solve_energy_1d(lgh_ctx *c, const double *v_h1, double *de, double *e_rhs, const double *e_source, int *l2_iters)
{
   RoctxRange range("SolveEnergy-MeInv"); // :508
   timer_start(c);
   const int rc = visit_order(c->kid, [&](auto Dc, auto Qc, auto) {
      constexpr int D = decltype(Dc)::value, Q = decltype(Qc)::value;
      hipLaunchKernelGGL((energy_solve_1d_k<D, Q, true>), dim3(zone_grid(c)), dim3(256), 0, c->stream, c->NE, c->h1map, c->G, c->Bl,
                         c->stressJinvT, v_h1, e_source, (const double *)nullptr, e_rhs, c->me_fac, de);
      LGH_HIP_CHECK(hipGetLastError());
      return LGH_OK;
   });
   timer_stop(c, 1);
   if (rc) { return rc; }
   c->timers.c[1] += c->NE;
   if (l2_iters) { *l2_iters += c->NE; }
   return LGH_OK;
}

int density_1d(lgh_ctx *c, const double *x_h1, double *rho_l2)
{
   const int rc = visit_order(c->kid, [&](auto Dc, auto Qc, auto) {
      constexpr int D = decltype(Dc)::value, Q = decltype(Qc)::value;
      hipLaunchKernelGGL((density_1d_k<D, Q>), dim3(zone_grid(c)), dim3(256), 0, c->stream, c->NE, c->h1map, c->G, c->Bl, c->W,
                         x_h1, c->rho0DetJ0w, rho_l2);
      LGH_HIP_CHECK(hipGetLastError());
      return LGH_OK;
   });
   if (rc) { return rc; }
   LGH_HIP_CHECK(hipStreamSynchronize(c->stream)); // (as the 2D/3D projection: complete on return)
   return LGH_OK;
}

int energy_1d(lgh_ctx *c, int which, const double *vec, double *result)
{
   const int rc = visit_order(c->kid, [&](auto Dc, auto Qc, auto) {
      constexpr int D = decltype(Dc)::value, Q = decltype(Qc)::value;
      if (which == 0)
      {
         hipLaunchKernelGGL((energy_1d_k<D, Q, 0>), dim3(zone_grid(c)), dim3(256), 0, c->stream, c->NE, c->h1map, c->B, c->Bl,
                            c->rho0DetJ0w, vec, c->partials, c->tickets, c->scal);
      }
      else
      {
         hipLaunchKernelGGL((energy_1d_k<D, Q, 1>), dim3(zone_grid(c)), dim3(256), 0, c->stream, c->NE, c->h1map, c->B, c->Bl,
                            c->rho0DetJ0w, vec, c->partials, c->tickets, c->scal);
      }
      LGH_HIP_CHECK(hipGetLastError());
      return LGH_OK;
   });
   if (rc) { return rc; }
   LGH_HIP_CHECK(hipMemcpyAsync(c->host_pinned + kPinResult, c->scal, sizeof(double), hipMemcpyDeviceToHost, c->stream));
   LGH_HIP_CHECK(hipStreamSynchronize(c->stream));
   *result = (which == 0) ? c->host_pinned[kPinResult] : 0.5 * c->host_pinned[kPinResult];
   return LGH_OK;
}

int sedov_density_error_1d(lgh_ctx *c, const double *x_h1, const double *rho_l2, const double par[21], double t,
                           const double origin[3], int n1d, const double *weights, const double *B_h1, const double *G_h1,
                           const double *B_l2, double *err2)
{
   const int D = c->D1D, L = c->L1D;
   const size_t np = (size_t)c->NE * n1d;
   std::vector<double> tab;
   tab.insert(tab.end(), weights, weights + n1d);
   tab.insert(tab.end(), B_h1, B_h1 + (size_t)n1d * D);
   tab.insert(tab.end(), G_h1, G_h1 + (size_t)n1d * D);
   tab.insert(tab.end(), B_l2, B_l2 + (size_t)n1d * L);
   DevPtr<double> buf; // [tables | r | rho_h | w detJ | rho_exact | v | P]
   LGH_PASS(buf.alloc(tab.size() + 6 * np));
   LGH_HIP_CHECK(hipMemcpy(buf, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
   const double *dw = buf, *dB = dw + n1d, *dG = dB + (size_t)n1d * D, *dBl = dG + (size_t)n1d * D;
   double *r = buf + tab.size(), *rh = r + np, *wd = rh + np, *rx = wd + np, *vx = rx + np, *px = vx + np;
   int rc = visit_order(c->kid, [&](auto Dc, auto, auto) {
      constexpr int Dt = decltype(Dc)::value;
      hipLaunchKernelGGL((sedov_points_1d_k<Dt>), dim3(ceil_div((long)np, 256)), dim3(256), 0, c->stream, c->NE, n1d, c->h1map,
                         dB, dG, dBl, dw, x_h1, rho_l2, origin[0], r, rh, wd);
      LGH_HIP_CHECK(hipGetLastError());
      return LGH_OK;
   });
   if (rc) { return rc; }
   rc = lgh_sedov_eval(c, par, t, (long)np, r, rx, vx, px);
   if (rc) { return rc; }
   hipLaunchKernelGGL(sedov_err_1d_k, dim3(zone_grid(c)), dim3(256), 0, c->stream, c->NE, n1d, (const double *)rx,
                      (const double *)rh, (const double *)wd, c->partials, c->tickets, c->scal);
   LGH_HIP_CHECK(hipGetLastError());
   LGH_HIP_CHECK(hipMemcpyAsync(c->host_pinned + kPinResult, c->scal, sizeof(double), hipMemcpyDeviceToHost, c->stream));
   LGH_HIP_CHECK(hipStreamSynchronize(c->stream)); // (the scratch is released on return)
   *err2 = c->host_pinned[kPinResult];
   return LGH_OK;
}

} // namespace lgh
