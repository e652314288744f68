// lgh_mass.hip — MassPAOperator action and Jacobi diagonal for gfx950: the element kernels and their dispatch, the mass
// data, the node gather.  The device-resident CG solves written on them are in lgh_scg.hip.
//
// Replaces MassPAOperator::{Mult,MultFull,EliminateRHS}
// (/root/reference/laghos_assembly.cpp:80-121; the contraction itself is upstream
// MFEM MassIntegrator::AddMultPA, same math as amr/laghos_assembly.cpp:878-963) and
// OperatorJacobiSmoother (laghos_solver.cpp:266-270).
#include "lgh_mass.hpp"

namespace lgh
{

template <int D, int Q, int NEB, int MODE>
__global__ void __launch_bounds__(Q *Q *NEB)
mass_apply_3d(const MassArgs a)
{
   constexpr int NQ = Q * Q * Q, ND = D * D * D;
   constexpr int SX = (ND > D * Q * Q) ? ND : D * Q * Q; // X then C[dz][qy][qx]
   constexpr int SA = D * D * Q;                         // A[dz][dy][qx] then E[dz][qy][dx]
   constexpr int SAE = (SA > D * Q * D) ? SA : D * Q * D;
   constexpr int PER = SX + SAE + 1;
   __shared__ double smem[NEB * PER];
   __shared__ double red[16];

   const int tid = threadIdx.x;
   const int tx = tid % Q, ty = (tid / Q) % Q, eb = tid / (Q * Q);
   const int nblocks = gridDim.x;
   const int blk = (MODE == 2 || MODE == 1) ? xcd_swizzle(blockIdx.x, nblocks) : blockIdx.x;
   const int e0 = blk * NEB;
   const int e = e0 + eb;
   const bool active = (e < a.NE);
   double *sX = smem + eb * PER;
   double *sA = sX + SX;

   double beta = 0.0;
   bool first = false;
   if (MODE >= 2)
   {
      if (a.cgs->done) { return; }
      first = a.cgs->first != 0;
      if (a.multi && !first && cg_pending_update(a.cgs, a.iter, blockIdx.x == 0 && threadIdx.x == 0)) { return; }
      beta = first ? 0.0 : a.cgs->rz / a.cgs->rz_prev;
   }

   // ---- cooperative load of the block's element dofs
   {
      const int nthr = Q * Q * NEB;
      const int nel = min(NEB, a.NE - e0);
      for (int i = tid; i < nel * ND; i += nthr)
      {
         const int el = i / ND, d = i - el * ND;
         const size_t p = (size_t)(e0 + el) * ND + d;
         double val;
         if (MODE == 0) { val = a.x[p]; }
         else if (MODE == 1) { val = a.x[a.map[p]]; }
         else if (MODE == 2)
         {
            const int n = a.map[p];
            val = a.x[n]; // K2 stores the same value later
            if (!first) { val += beta * a.d[n]; }
         }
         else
         {
            val = a.x[p];
            if (!first) { val += beta * a.d[p]; }
            a.d[p] = val;
         }
         smem[el * PER + d] = val;
      }
   }
   double bx[D], by[D];
#pragma unroll
   for (int d = 0; d < D; d++)
   {
      bx[d] = a.B[tx + Q * d];
      by[d] = a.B[ty + Q * d];
   }
   // quadrature data of this column, issued early
   double dq[Q];
   if (active)
   {
      const double *p = a.Dq + (size_t)e * NQ + tx + Q * ty;
#pragma unroll
      for (int qz = 0; qz < Q; qz++) { dq[qz] = p[Q * Q * qz]; }
   }
   else
   {
#pragma unroll
      for (int qz = 0; qz < Q; qz++) { dq[qz] = 0.0; }
   }
   __syncthreads();

   // E-level dot needs x_e for the (dx,dy) threads: keep the column in registers
   double xcol[D];
   if (MODE >= 2)
   {
#pragma unroll
      for (int dz = 0; dz < D; dz++) { xcol[dz] = (tx < D && ty < D) ? sX[tx + D * (ty + D * dz)] : 0.0; }
   }

   // forward x: thread (qx = tx, dy = ty < D)
   if (ty < D)
   {
#pragma unroll
      for (int dz = 0; dz < D; dz++)
      {
         double u = 0.0;
#pragma unroll
         for (int dx = 0; dx < D; dx++) { u += bx[dx] * sX[dx + D * (ty + D * dz)]; }
         sA[tx + Q * (ty + D * dz)] = u;
      }
   }
   __syncthreads();
   // forward y (registers per dz), forward z, scale, backward z
   double r[D];
   {
      double bb[D];
#pragma unroll
      for (int dz = 0; dz < D; dz++)
      {
         double u = 0.0;
#pragma unroll
         for (int dy = 0; dy < D; dy++) { u += by[dy] * sA[tx + Q * (dy + D * dz)]; }
         bb[dz] = u;
      }
      double qv[Q];
#pragma unroll
      for (int qz = 0; qz < Q; qz++)
      {
         double u = 0.0;
#pragma unroll
         for (int dz = 0; dz < D; dz++) { u += a.B[qz + Q * dz] * bb[dz]; }
         qv[qz] = u * dq[qz];
      }
#pragma unroll
      for (int dz = 0; dz < D; dz++)
      {
         double u = 0.0;
#pragma unroll
         for (int qz = 0; qz < Q; qz++) { u += a.B[qz + Q * dz] * qv[qz]; }
         r[dz] = u;
      }
   }
   // sX is dead (read before the previous barrier): reuse as C[dz][qy][qx]
#pragma unroll
   for (int dz = 0; dz < D; dz++) { sX[tx + Q * (ty + Q * dz)] = r[dz]; }
   __syncthreads();
   // backward x: thread (dx = tx < D, qy = ty)
   if (tx < D)
   {
      double brow[Q];
#pragma unroll
      for (int q = 0; q < Q; q++) { brow[q] = a.B[q + Q * tx]; }
#pragma unroll
      for (int dz = 0; dz < D; dz++)
      {
         double u = 0.0;
#pragma unroll
         for (int qx = 0; qx < Q; qx++) { u += brow[qx] * sX[qx + Q * (ty + Q * dz)]; }
         sA[tx + D * (ty + Q * dz)] = u;
      }
   }
   __syncthreads();
   // backward y: thread (dx = tx < D, dy = ty < D)
   double dot = 0.0;
   if (tx < D && ty < D && active)
   {
      double brow[Q];
#pragma unroll
      for (int q = 0; q < Q; q++) { brow[q] = a.B[q + Q * ty]; }
#pragma unroll
      for (int dz = 0; dz < D; dz++)
      {
         double u = 0.0;
#pragma unroll
         for (int qy = 0; qy < Q; qy++) { u += brow[qy] * sA[tx + D * (qy + Q * dz)]; }
         const size_t po = tx + D * (ty + D * dz) + (size_t)ND * e;
         a.y[po] = u;
         if (MODE >= 2) { dot += xcol[dz] * u; }
      }
   }
   if (MODE >= 2)
   {
      const double bsum = block_sum(dot, red);
      double total;
      if (grid_sum_last_block(bsum, a.partials, a.ticket, red, total))
      {
         if (tid == 0)
         {
            a.cgs->den = total;
            if (a.cgs->first) { a.cgs->first = 0; }
            if (total == 0.0 && !a.multi) { a.cgs->done = 1; } // breakdown (den == 0): stop, as upstream
         }
      }
   }
}

// ---------------------------------------------------------------------------
// L2 mass apply for the high orders (Q1D >= 8: Q4Q3, Q5Q4), plane-per-thread form.
// The column form above keeps Q*Q threads per element and the quadrature data of one z-column per thread:
// at Q1D = 10 that is one wave per SIMD (NEB = 2 elements per workgroup) and the kernel reaches 1.7 TB/s,
// and the unpreconditioned energy CG (237 iterations per solve at Q5Q4) makes it the dominant kernel of
// BASELINE config 5.  Here a thread owns one x-index qx of an element and keeps (y, z) data of that index in
// registers (as vcg_apply_plane does for the H1 solve): only the two x contractions go through LDS, and
// 256 / (Q HY) elements share a workgroup, two workgroups per CU.
// Register budget: the plane w[qy][dz] (Q*L doubles) AND the 1-D table (Q*L doubles - too large for the
// scalar registers at 50 entries, and re-reading it from LDS per use would make the kernel LDS-issue bound)
// both want registers.  At Q = 10 that is 2 x 100 VGPRs and does not fit, so the qy rows of a plane are split
// over HY = 2 threads: thread (qx, h) runs the rows qy in [h Q/HY, (h+1) Q/HY) through the z stage (the rows are
// independent there) and contributes a partial sum to the backward y contraction; the HY partial planes are
// summed by the backward x contraction, which reads them from LDS anyway.
// The quadrature data is read straight from memory, one qy row of Q values ahead of its use (each value is
// needed by exactly one thread: LDS staging would only add traffic); rows of Q consecutive doubles.
// MODE 0: y = M x.  MODE 3: CG K1 of the L2 solve (d = r + beta d stored in place, den = (d, M d)).
// value of the other lane of an adjacent pair (quad_perm [1,0,3,2], as lane_pair_swap of lgh_vcg_k1.hip)
__device__ __forceinline__ double pair_swap(const double v)
{
   int lo = __double2loint(v), hi = __double2hiint(v);
   lo = __builtin_amdgcn_mov_dpp(lo, 0xB1, 0xF, 0xF, true);
   hi = __builtin_amdgcn_mov_dpp(hi, 0xB1, 0xF, 0xF, true);
   return __hiloint2double(hi, lo);
}

template <int L, int Q, int HY, int NEB, int MODE, bool SEP>
__global__ void __launch_bounds__(Q *HY *NEB, 2)
mass_apply_l2_plane(const MassArgs a)
{
   constexpr int NQ = Q * Q * Q, NL = L * L * L, LL = L * L;
   constexpr int TE = Q * HY, NT = TE * NEB, QH = Q / HY;
   static_assert(Q % HY == 0, "qy rows split evenly");
   constexpr int CS = NL | 1;            // odd strides: the broadcast reads of different elements hit different banks
   static_assert(HY == 1 || HY == 2, "one lane or a pair of adjacent lanes per plane");
   constexpr int CE = (LL * Q) | 1; // [dy,dz][qx]: the two lanes of a pair (HY = 2) hand over one summed plane (lane_pair_swap)
   __shared__ double sIn[NEB * CS], sE[NEB * CE], sB[Q * L];
   __shared__ double red[16];
   const int tid = threadIdx.x;
   const int eb = tid / TE, lt = tid - eb * TE;
   const int qx = lt / HY, h = lt - qx * HY; // (the lanes of a pair are adjacent: TE is even, so h is the parity of the lane)
   const int e0 = blockIdx.x * NEB, e = e0 + eb;
   const bool active = (e < a.NE);
   double beta = 0.0;
   bool first = false;
   if (MODE == 3)
   {
      if (a.cgs->done) { return; }
      first = a.cgs->first != 0;
      if (a.multi && !first && cg_pending_update(a.cgs, a.iter, blockIdx.x == 0 && threadIdx.x == 0)) { return; }
      beta = first ? 0.0 : a.cgs->rz / a.cgs->rz_prev;
   }
   for (int i = tid; i < Q * L; i += NT) { sB[i] = a.B[i]; }
   {
      const int nel = min(NEB, a.NE - e0);
      for (int i = tid; i < nel * NL; i += NT)
      {
         const int el = i / NL, d = i - el * NL;
         const size_t p = (size_t)e0 * NL + i;
         double val = a.x[p];
         if (MODE == 3)
         {
            if (!first) { val += beta * a.d[p]; }
            a.d[p] = val;
         }
         sIn[el * CS + d] = val;
      }
   }
   // first row of this thread's quadrature data, in flight across the barrier
   const double *Dp = a.Dq + (size_t)(active ? e : 0) * a.dqs + qx + Q * (h * QH);
   const double se = a.Se[active ? e : 0];
   double dq[SEP ? 1 : Q];
   if (!SEP)
   {
#pragma unroll
      for (int qz = 0; qz < Q; qz++) { dq[qz] = Dp[Q * Q * qz] * se; }
   }
   // SEP: value(q, e) = se w[qx] w[qy] w[qz] - the weights in scalar registers, no loads and no row held ahead
   double ws[SEP ? (Q + 1) / 2 : 1]; // (mirror symmetric, checked by lgh_create: w[q] = w[Q - 1 - q])
   auto wq = [&](const int q) -> double { return ws[SEP ? (q < (Q + 1) / 2 ? q : Q - 1 - q) : 0]; };
   double wxe = 0.0;
   if (SEP)
   {
#pragma unroll
      for (int q = 0; q < (Q + 1) / 2; q++) { ws[q] = uniform_f64(a.w1[q]); }
      wxe = a.w1[qx] * se;
   }
   __syncthreads();
   const double *sI = sIn + eb * CS;
   // the 1-D table in scalar registers, in half: the Bernstein basis at Gauss-Legendre points is mirror symmetric,
   // B[q,l] = B[Q-1-q, L-1-l] (checked by lgh_create; the column form runs otherwise)
   constexpr int QL = Q * L, HB = (QL + 1) / 2;
   double Bh[HB];
#pragma unroll
   for (int i = 0; i < HB; i++) { Bh[i] = uniform_f64(a.B[i]); }
   auto Bt = [&](const int idx) -> double { return idx < HB ? Bh[idx] : Bh[QL - 1 - idx]; };
   // forward x: t[dy,dz] = sum_dx B[qx,dx] d[dx,dy,dz]   (the HY threads of a plane each form it)
   double t[LL];
   {
      double bx[L];
#pragma unroll
      for (int dx = 0; dx < L; dx++) { bx[dx] = sB[qx + Q * dx]; }
#pragma unroll
      for (int k = 0; k < LL; k++)
      {
         double u = 0.0;
#pragma unroll
         for (int dx = 0; dx < L; dx++) { u = fma(bx[dx], sI[dx + L * k], u); }
         t[k] = u;
      }
   }
   // this thread's rows: forward y, then per row forward z, scaling, backward z; partial backward y on the fly
   double acc[LL]; // [dy + L*dz]: sum over this thread's qy rows of B[qy,dy] w[qy][dz]
#pragma unroll
   for (int k = 0; k < LL; k++) { acc[k] = 0.0; }
#pragma unroll
   for (int r = 0; r < QH; r++)
   {
      double dn[SEP ? 1 : Q];
      if (!SEP && r + 1 < QH)
      {
#pragma unroll
         for (int qz = 0; qz < Q; qz++) { dn[qz] = Dp[Q * (r + 1) + Q * Q * qz] * se; }
      }
      double wrow = 0.0; // SEP: se w[qx] w[qy] of this row
      if (SEP)
      {
         double wy = wq(r);
#pragma unroll
         for (int hh = 1; hh < HY; hh++) { wy = (h == hh) ? wq(hh * QH + r) : wy; }
         wrow = wxe * wy;
      }
      // the table row of qy = h*QH + r (h differs between lanes: select, not index)
      double by[L];
#pragma unroll
      for (int dy = 0; dy < L; dy++)
      {
         double v = Bt(r + Q * dy);
#pragma unroll
         for (int hh = 1; hh < HY; hh++) { v = (h == hh) ? Bt(hh * QH + r + Q * dy) : v; }
         by[dy] = v;
      }
      double wr[L];
#pragma unroll
      for (int dz = 0; dz < L; dz++)
      {
         double u = 0.0;
#pragma unroll
         for (int dy = 0; dy < L; dy++) { u = fma(by[dy], t[dy + L * dz], u); }
         wr[dz] = u;
      }
      double cz[Q];
#pragma unroll
      for (int qz = 0; qz < Q; qz++)
      {
         double u = 0.0;
#pragma unroll
         for (int dz = 0; dz < L; dz++) { u = fma(Bt(qz + Q * dz), wr[dz], u); }
         cz[qz] = SEP ? (u * wrow) * wq(qz) : u * dq[SEP ? 0 : qz];
      }
#pragma unroll
      for (int dz = 0; dz < L; dz++)
      {
         double u = 0.0;
#pragma unroll
         for (int qz = 0; qz < Q; qz++) { u = fma(Bt(qz + Q * dz), cz[qz], u); }
#pragma unroll
         for (int dy = 0; dy < L; dy++) { acc[dy + L * dz] = fma(by[dy], u, acc[dy + L * dz]); }
      }
      if (!SEP && r + 1 < QH)
      {
#pragma unroll
         for (int qz = 0; qz < Q; qz++) { dq[qz] = dn[qz]; }
      }
   }
   // hand the plane over; HY = 2: lane h of a pair delivers the (dy,dz) entries k = h (mod 2), summed over both lanes
   double *sEe = sE + eb * CE;
   if (HY == 1)
   {
#pragma unroll
      for (int k = 0; k < LL; k++) { sEe[qx + Q * k] = acc[k]; }
   }
   else
   {
#pragma unroll
      for (int k = 0; k + 1 < LL; k += 2)
      {
         const double give = h ? acc[k] : acc[k + 1];
         const double keep = h ? acc[k + 1] : acc[k];
         sEe[qx + Q * (k + h)] = keep + pair_swap(give);
      }
      if (LL & 1)
      {
         const double tot = acc[LL - 1] + pair_swap(acc[LL - 1]);
         if (h == 0) { sEe[qx + Q * (LL - 1)] = tot; }
      }
   }
   __syncthreads();
   // backward x: thread (lx = qx < L, h) sums the Q planes of both halves for its share of the (dy,dz) pairs
   double dot = 0.0;
   if (qx < L && active)
   {
      const double *sEa = sE + eb * CE;
      double bt[Q];
#pragma unroll
      for (int q = 0; q < Q; q++) { bt[q] = sB[q + Q * qx]; }
      constexpr int KH = (LL + HY - 1) / HY;
#pragma unroll
      for (int kk = 0; kk < KH; kk++)
      {
         const int k = h * KH + kk;
         if (k < LL)
         {
            double u = 0.0;
#pragma unroll
            for (int q = 0; q < Q; q++) { u = fma(bt[q], sEa[q + Q * k], u); }
            a.y[(size_t)e * NL + qx + L * k] = u;
            if (MODE == 3) { dot = fma(sI[qx + L * k], u, dot); }
         }
      }
   }
   if (MODE == 3)
   {
      const double bsum = block_sum(dot, red);
      double total;
      if (grid_sum_last_block(bsum, a.partials, a.ticket, red, total))
      {
         if (tid == 0)
         {
            a.cgs->den = total;
            if (a.cgs->first) { a.cgs->first = 0; }
            if (total == 0.0 && !a.multi) { a.cgs->done = 1; } // breakdown (den == 0): stop, as upstream
         }
      }
   }
}

// 2D: one thread per quadrature point; same MODE semantics.
template <int D, int Q, int NEB, int MODE>
__global__ void __launch_bounds__(Q *Q *NEB)
mass_apply_2d(const MassArgs a)
{
   constexpr int NQ = Q * Q, ND = D * D;
   constexpr int PER = ND + D * Q + NQ + 1;
   __shared__ double smem[NEB * PER];
   __shared__ double red[16];
   const int tid = threadIdx.x;
   const int tx = tid % Q, ty = (tid / Q) % Q, eb = tid / (Q * Q);
   const int e0 = blockIdx.x * NEB;
   const int e = e0 + eb;
   const bool active = (e < a.NE);
   double *sX = smem + eb * PER; // [dy][dx]
   double *sA = sX + ND;         // [dy][qx] / [qy][dx]
   double *sQ = sA + D * Q;      // [qy][qx]
   double beta = 0.0;
   bool first = false;
   if (MODE >= 2)
   {
      if (a.cgs->done) { return; }
      first = a.cgs->first != 0;
      if (a.multi && !first && cg_pending_update(a.cgs, a.iter, blockIdx.x == 0 && threadIdx.x == 0)) { return; }
      beta = first ? 0.0 : a.cgs->rz / a.cgs->rz_prev;
   }
   {
      const int nthr = Q * Q * NEB;
      const int nel = min(NEB, a.NE - e0);
      for (int i = tid; i < nel * ND; i += nthr)
      {
         const int el = i / ND, d = i - el * ND;
         const size_t p = (size_t)(e0 + el) * ND + d;
         double val;
         if (MODE == 0) { val = a.x[p]; }
         else if (MODE == 1) { val = a.x[a.map[p]]; }
         else if (MODE == 2)
         {
            const int n = a.map[p];
            val = a.x[n];
            if (!first) { val += beta * a.d[n]; }
         }
         else
         {
            val = a.x[p];
            if (!first) { val += beta * a.d[p]; }
            a.d[p] = val;
         }
         smem[el * PER + d] = val;
      }
   }
   __syncthreads();
   if (ty < D)
   {
      double u = 0.0;
      for (int dx = 0; dx < D; dx++) { u += a.B[tx + Q * dx] * sX[dx + D * ty]; }
      sA[tx + Q * ty] = u;
   }
   __syncthreads();
   {
      double u = 0.0;
      for (int dy = 0; dy < D; dy++) { u += a.B[ty + Q * dy] * sA[tx + Q * dy]; }
      sQ[tx + Q * ty] = active ? u * a.Dq[(size_t)e * NQ + tx + Q * ty] : 0.0;
   }
   __syncthreads();
   if (tx < D)
   {
      double u = 0.0;
      for (int qx = 0; qx < Q; qx++) { u += a.B[qx + Q * tx] * sQ[qx + Q * ty]; }
      sA[tx + D * ty] = u;
   }
   __syncthreads();
   double dot = 0.0;
   if (tx < D && ty < D && active)
   {
      double u = 0.0;
      for (int qy = 0; qy < Q; qy++) { u += a.B[qy + Q * ty] * sA[tx + D * qy]; }
      const size_t po = tx + D * ty + (size_t)ND * e;
      a.y[po] = u;
      if (MODE >= 2) { dot = sX[tx + D * ty] * u; }
   }
   if (MODE >= 2)
   {
      const double bsum = block_sum(dot, red);
      double total;
      if (grid_sum_last_block(bsum, a.partials, a.ticket, red, total))
      {
         if (tid == 0)
         {
            a.cgs->den = total;
            if (a.cgs->first) { a.cgs->first = 0; }
            if (total == 0.0 && !a.multi) { a.cgs->done = 1; }
         }
      }
   }
}

// ---- L2 mass apply, Kronecker form (3D; compact mass data on a tensor-product rule: lgh_create's 1-D mass tile M1l)
// B^T diag(s_e w (x) w (x) w) B = s_e M1 (x) M1 (x) M1 with M1 = B^T diag(w) B (L x L): three contractions of L on the
// element's L^3 dofs - 3 L^4 FMAs instead of ~2 (L^3 Q + L^2 Q^2 + L Q^3) + Q^3 through the quadrature points (L = 5,
// Q = 10: 1 875 against 18 500) and no quadrature-point values at all: the kernel moves its vectors and nothing else.
// Same operator in exact arithmetic (the compact form itself is accepted to 1e-12, mass_data); rounding differs.
// MODE 0: y = M x.  MODE 3: CG K1 of the L2 solve (d = r + beta d stored in place, den = (d, M d)), as the plane form; with
// a.no_y the product itself is not stored.  MODE 4 (round 6): the UPDATE of the same iteration, for the launch after it -
// M d is formed again from the stored d (same code, same bits) and x += alpha d, r -= alpha M d, (r, r) follow with the
// expressions, the scalars and the convergence logic of cg_update_k: the product never travels through memory.
// One workgroup of 256 threads takes NEB consecutive elements (their dofs are one contiguous run of the L2 vector);
// a thread owns one row of L values per stage: x rows (e, lz, ly), y rows (e, lz, lx), z rows (e, ly, lx).
template <int L, int NEB, int MODE>
__global__ void __launch_bounds__(256)
mass_apply_l2_kron(const MassArgs a)
{
   constexpr int NL = L * L * L, LL = L * L, NT = 256;
   __shared__ double sIn[NEB * NL], sT1[NEB * NL], sT2[NEB * NL];
   __shared__ double red[16];
   const int tid = threadIdx.x;
   const int e0 = blockIdx.x * NEB;
   const int nel = min(NEB, a.NE - e0);
   double beta = 0.0, alpha = 0.0;
   bool first = false;
   if (MODE == 3)
   {
      if (a.cgs->done) { return; }
      first = a.cgs->first != 0;
      if (a.ls_on && !first)
      {
         const double rz = lockstep_rz(a.ls);
         if (lockstep_pending_update(a.cgs, a.iter, rz, blockIdx.x == 0 && threadIdx.x == 0)) { return; }
         beta = rz / a.cgs->rz_prev;
      }
      else
      {
         if (a.multi && !first && cg_pending_update(a.cgs, a.iter, blockIdx.x == 0 && threadIdx.x == 0)) { return; }
         beta = first ? 0.0 : a.cgs->rz / a.cgs->rz_prev;
      }
   }
   if (MODE == 4)
   {
      if (a.cgs->done) { return; }
      if (a.ls_on)
      {
         const double den = *a.ls_den_src; // (summed over the ranks by the halo exchange of this iteration)
         if (den == 0.0) // breakdown, as cg_pending_den
         {
            if (blockIdx.x == 0 && threadIdx.x == 0)
            {
               __hip_atomic_store(&a.cgs->done, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
               __hip_atomic_store(&a.cgs->rz, 0.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            return;
         }
         alpha = a.cgs->rz / den;
      }
      else
      {
         if (a.multi && cg_pending_den(a.cgs, blockIdx.x == 0 && threadIdx.x == 0)) { return; } // (as cg_update_k)
         alpha = a.cgs->rz / a.cgs->den;
      }
   }
   double M[LL]; // M[i + L j], symmetric, in scalar registers
#pragma unroll
   for (int i = 0; i < LL; i++) { M[i] = uniform_f64(a.M1[i]); }
   // MODE 4: the r and x values of the places this thread updates in the last stage, asked for now
   constexpr int ZR = (NEB * LL + NT - 1) / NT; // rows (e, ly, lx) per thread in the z stage
   double ro[MODE == 4 ? ZR : 1][L], xo[MODE == 4 ? ZR : 1][L];
   if (MODE == 4)
   {
#pragma unroll
      for (int k = 0; k < ZR; k++)
      {
         const int r = tid + k * NT;
         const int yx = r % LL, el = r / LL;
         const bool ok = r < nel * LL;
#pragma unroll
         for (int i = 0; i < L; i++)
         {
            const size_t p = (size_t)e0 * NL + (ok ? el * NL + yx + LL * i : 0);
            ro[k][i] = a.ur[p];
            xo[k][i] = a.ux[p];
         }
      }
   }
   for (int i = tid; i < nel * NL; i += NT)
   {
      const size_t p = (size_t)e0 * NL + i;
      double val = (MODE == 4) ? a.d[p] : a.x[p];
      if (MODE == 3)
      {
         if (!first) { val += beta * a.d[p]; }
         a.d[p] = val;
      }
      sIn[i] = val;
   }
   __syncthreads();
   // x: rows of L consecutive values
   for (int r = tid; r < nel * LL; r += NT)
   {
      double u[L];
#pragma unroll
      for (int j = 0; j < L; j++) { u[j] = sIn[r * L + j]; }
#pragma unroll
      for (int i = 0; i < L; i++)
      {
         double s = M[i] * u[0];
#pragma unroll
         for (int j = 1; j < L; j++) { s = fma(M[i + L * j], u[j], s); }
         sT1[r * L + i] = s;
      }
   }
   __syncthreads();
   // y: rows (e, lz, lx), stride L
   for (int r = tid; r < nel * LL; r += NT)
   {
      const int lx = r % L, ez = r / L; // ez = lz + L e
      const int base = ez * LL + lx;
      double u[L];
#pragma unroll
      for (int j = 0; j < L; j++) { u[j] = sT1[base + L * j]; }
#pragma unroll
      for (int i = 0; i < L; i++)
      {
         double s = M[i] * u[0];
#pragma unroll
         for (int j = 1; j < L; j++) { s = fma(M[i + L * j], u[j], s); }
         sT2[base + L * i] = s;
      }
   }
   __syncthreads();
   // z: rows (e, ly, lx), stride L^2; the element factor; out (and the partial of (d, M d))
   double dot = 0.0;
#pragma unroll
   for (int k = 0; k < ZR; k++)
   {
      const int r = tid + k * NT;
      if (r >= nel * LL) { break; }
      const int yx = r % LL, el = r / LL;
      const int base = el * NL + yx;
      const double se = a.Se[e0 + el];
      double u[L];
#pragma unroll
      for (int j = 0; j < L; j++) { u[j] = sT2[base + LL * j]; }
#pragma unroll
      for (int i = 0; i < L; i++)
      {
         double s = M[i] * u[0];
#pragma unroll
         for (int j = 1; j < L; j++) { s = fma(M[i + L * j], u[j], s); }
         s *= se;
         if (MODE == 4)
         {
            // cg_update_k's expressions: x += alpha d, r -= alpha (M d), (r, r)
            const double dv = sIn[base + LL * i];
            const double xv = xo[MODE == 4 ? k : 0][i] + alpha * dv;
            const double rv = ro[MODE == 4 ? k : 0][i] - alpha * s;
            a.ux[(size_t)e0 * NL + base + LL * i] = xv;
            a.ur[(size_t)e0 * NL + base + LL * i] = rv;
            dot += rv * rv;
            continue;
         }
         if (!(MODE == 3 && a.no_y)) { a.y[(size_t)e0 * NL + base + LL * i] = s; }
         if (MODE == 3) { dot = fma(sIn[base + LL * i], s, dot); }
      }
   }
   if (MODE == 4)
   {
      const double bsum = block_sum(dot, red);
      double total;
      if (grid_sum_last_block(bsum, a.partials, a.ticket, red, total))
      {
         if (tid == 0)
         {
            CgScalars *sc = a.cgs;
            sc->rz_prev = sc->rz;
            sc->rz = total; // betanom
            if (a.ls_on) { a.ls_word_out[kLsWord] = __double_as_longlong(total); } // (its sum over the ranks: the next apply, or l2_lockstep_fold)
            if (!a.multi)
            {
               sc->iters = a.iter;
               if (total < 0.0 || total <= sc->r0) { sc->done = 1; }
            }
         }
      }
   }
   if (MODE == 3)
   {
      const double bsum = block_sum(dot, red);
      double total;
      if (grid_sum_last_block(bsum, a.partials, a.ticket, red, total))
      {
         if (tid == 0)
         {
            a.cgs->den = total;
            if (a.ls_on && a.ls_den_mirror) { *a.ls_den_mirror = total; } // (lockstep: behind the halo messages of the velocity iteration)
            if (a.cgs->first) { a.cgs->first = 0; }
            if (total == 0.0 && !a.multi) { a.cgs->done = 1; } // breakdown (den == 0): stop, as upstream
         }
      }
   }
}

static bool l2_one_round(const lgh_ctx *c)
{
   return c->L1D >= 5 && c->sw.l2_neb;
}

// Which kernel the L2 mass apply (modes 0 / 3: the energy CG) launches, decided in ONE place for the dispatch below
// and for lgh_l2_mass_form(): 2 = mass_apply_l2_kron (needs compact data on a tensor-product rule), 1 = the plane form,
// 0 = the column form.  `compact`: whether the kernel reads one factor per element instead of the NQ-entry table.
static int l2_mass_kernel(lgh_ctx *c, int *form, int *compact)
{
   const double *Dq, *Se;
   int dqs = 1;
   *form = 0;
   *compact = 0;
   const bool kron_ok = c->dim == 3 && c->M1l && c->w1d && c->L1D <= 5;
   const bool plane_ok = c->b_l2_sym && c->dim == 3 && c->L1D >= 3 && c->sw.l2_plane; // (LGH_L2_PLANE=0: column form)
   if (kron_ok || plane_ok)
   {
      const int rc = mass_data(c, &Dq, &dqs, &Se);
      if (rc) { return rc; }
   }
   if (kron_ok && dqs == 0) { *form = 2; *compact = 1; }
   else if (plane_ok) { *form = 1; *compact = (dqs == 0); }
   return LGH_OK;
}
int l2_mass_form(lgh_ctx *c, int *form, int *compact) { return l2_mass_kernel(c, form, compact); }

// The Kronecker kernel in mode M (0 / 3: launch_mass, 4: the fused update of the energy CG), zones per workgroup by L.
// L = 5 (round 6): ten, so that every thread has ONE row of a stage (25 rows per zone) and five workgroups fit a CU's LDS,
// instead of sixteen (400 rows: a second round with 144 of 256 threads, three workgroups per CU): 53 -> 46 us per apply at
// config 5, the leg 501 -> 534 (profiles/r6_l2_neb.txt); at L = 3 the same choice (28 zones instead of 64) changes nothing.
// LGH_L2_NEB=0: sixteen.
template <int M> static int launch_l2_kron(lgh_ctx *c, const MassArgs &a)
{
   return visit_order_2d3d(c, [&](auto, auto, auto Lc) {
      constexpr int L = Lc, NEB = 512 >> L; // 256, 128, 64, 32, 16
      if (L == 5 && l2_one_round(c)) { hipLaunchKernelGGL((mass_apply_l2_kron<5, 10, M>), dim3(ceil_div(c->NE, 10)), dim3(256), 0, c->stream, a); }
      else { hipLaunchKernelGGL((mass_apply_l2_kron<L, NEB, M>), dim3(ceil_div(c->NE, NEB)), dim3(256), 0, c->stream, a); }
      LGH_HIP_CHECK(hipGetLastError());
      return LGH_OK;
   });
}

template <int MODE> static int launch_mass(lgh_ctx *c, int space, const MassArgs &a0)
{
   int l2form = 0, l2compact = 0;
   if ((MODE == 0 || MODE == 3) && space == LGH_SPACE_L2) { LGH_PASS(l2_mass_kernel(c, &l2form, &l2compact)); }
   constexpr int M = (MODE == 3 ? 3 : 0); // (the mode of the L2 forms)
   MassArgs a = a0;
   if (l2form) { LGH_PASS(mass_data(c, &a.Dq, &a.dqs, &a.Se)); } // (the Kronecker and plane forms take the mass data in its compact form where it has one)
   if (l2form == 2)
   {
      // compact mass data on a tensor-product rule: the Kronecker form (LGH_MASS_KRON=0: no tiles, see lgh_create)
      a.M1 = c->M1l;
      return launch_l2_kron<M>(c, a);
   }
   return visit_order_2d3d(c, [&](auto Dc, auto Qc, auto Lc) {
      constexpr int Q = Qc, L = Lc;
      // the column form on the n1d = D (H1) or L (L2) basis functions of the space
      auto column = [&](auto Nc) {
         constexpr int N1 = Nc, NEB = zones_per_wg(Q);
         const dim3 grid(ceil_div(c->NE, NEB)), block(Q * Q * NEB);
         if (c->dim == 2) { hipLaunchKernelGGL((mass_apply_2d<N1, Q, NEB, MODE>), grid, block, 0, c->stream, a); }
         else { hipLaunchKernelGGL((mass_apply_3d<N1, Q, NEB, MODE>), grid, block, 0, c->stream, a); }
      };
      if constexpr (L >= 3)
      {
         if (l2form == 1)
         {
            // the plane form (L = 3, 4, 5 in 3-D: l2_mass_kernel): lanes per plane and zones per workgroup (1, 42), (1, 32), (2, 12)
            constexpr int HY = (L == 5) ? 2 : 1, NEB = (L == 3) ? 42 : (L == 4) ? 32 : 12;
            const dim3 grid(ceil_div(c->NE, NEB)), block(Q * HY * NEB);
            a.w1 = (a.dqs == 0) ? c->w1d : nullptr;
            if (a.w1) { hipLaunchKernelGGL((mass_apply_l2_plane<L, Q, HY, NEB, M, true>), grid, block, 0, c->stream, a); }
            else { hipLaunchKernelGGL((mass_apply_l2_plane<L, Q, HY, NEB, M, false>), grid, block, 0, c->stream, a); }
            LGH_HIP_CHECK(hipGetLastError());
            return LGH_OK;
         }
      }
      if (space == LGH_SPACE_H1) { column(Dc); }
      else { column(Lc); }
      LGH_HIP_CHECK(hipGetLastError());
      return LGH_OK;
   });
}
// D[q, e] = W[q] s_e ?  In exact arithmetic the data of laghos_assembly.cpp:92-95, w_q detJ0(x_q) rho0(x_q), has this
// form whenever the initial element is affine and rho0 constant in it; the stored entries carry the rounding of the
// Jacobian and density evaluation at each point (measured: 220 ulp at Q3Q2 on the 8^3 box mesh, it grows like 1 / h).
// One thread per element: s_e = mean of D / W over the points (the centre of that rounding cloud), every point within
// tol (relative; kMassRank1Tol unless LGH_MASS_RANK1_TOL) or the stored table stays in use.
__global__ void __launch_bounds__(256)
mass_rank1_k(const int NE, const int NQ, const double tol, const double *__restrict__ D, const double *__restrict__ W, double *__restrict__ S,
             double *__restrict__ ones, int *flag)
{
   const int e = blockIdx.x * blockDim.x + threadIdx.x;
   if (e >= NE) { return; }
   const double *De = D + (size_t)e * NQ;
   double s = 0.0;
   for (int q = 0; q < NQ; q++) { s += De[q] / W[q]; }
   s /= NQ;
   bool ok = isfinite(s);
   for (int q = 0; q < NQ; q++) { ok = ok && fabs(De[q] - W[q] * s) <= tol * fabs(De[q]); }
   S[e] = s;
   ones[e] = 1.0;
   if (!ok) { *flag = 1; }
}
int mass_data(lgh_ctx *c, const double **Dq, int *dqs, const double **Se)
{
   if (c->mass_rank1 < 0)
   {
      if (!c->ones_ne)
      {
         LGH_PASS(c->massS.alloc((size_t)c->NE));
         LGH_PASS(c->ones_ne.alloc((size_t)c->NE));
      }
      int *flag = c->dev_flags + 3, h = 1;
      LGH_HIP_CHECK(hipMemsetAsync(flag, 0, sizeof(int), c->stream));
      hipLaunchKernelGGL(mass_rank1_k, dim3(ceil_div(c->NE, 256)), dim3(256), 0, c->stream, c->NE, c->NQ, c->sw.mass_rank1_tol, c->massD, c->W, c->massS, c->ones_ne, flag);
      LGH_HIP_CHECK(hipMemcpyAsync(&h, flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
      LGH_HIP_CHECK(hipStreamSynchronize(c->stream));
      c->mass_rank1 = (h == 0 && c->sw.mass_rank1) ? 1 : 0;
   }
   if (c->mass_rank1 == 1) { *Dq = c->W; *dqs = 0; *Se = c->massS; }
   else { *Dq = c->massD; *dqs = c->NQ; *Se = c->ones_ne; }
   return LGH_OK;
}

MassArgs base_args(lgh_ctx *c, int space)
{
   MassArgs a;
   memset(&a, 0, sizeof(a));
   a.NE = c->NE;
   a.B = (space == LGH_SPACE_H1) ? c->B : c->Bl;
   a.Dq = c->massD; // (every kernel but mass_apply_l2_plane reads the stored table; launch_mass fills Se / dqs)
   return a;
}

int mass_apply_cg(lgh_ctx *c, int space, const MassArgs &m)
{
   return (space == LGH_SPACE_H1) ? launch_mass<2>(c, space, m) : launch_mass<3>(c, space, m);
}
bool l2_fused_update(lgh_ctx *c)
{
   int form = 0, compact = 0;
   return c->sw.l2_fused && l2_mass_kernel(c, &form, &compact) == LGH_OK && form == 2;
}
int mass_l2_fused_update(lgh_ctx *c, const MassArgs &m, double *ux, double *ur, double *partials, unsigned int *ticket)
{
   MassArgs a = m;
   const int rc = mass_data(c, &a.Dq, &a.dqs, &a.Se);
   if (rc) { return rc; }
   a.M1 = c->M1l;
   a.ux = ux;
   a.ur = ur;
   a.partials = partials;
   a.ticket = ticket;
   return launch_l2_kron<4>(c, a);
}

int mass_apply_E(lgh_ctx *c, int space, const double *xE, double *yE)
{
   MassArgs a = base_args(c, space);
   a.x = xE;
   a.y = yE;
   return launch_mass<0>(c, space, a);
}

// ---- node kernels -----------------------------------------------------------
// y[n] = sum of element contributions; optional essential-row elimination.
// ELL transpose: t_ell[k*N + n] = E-vector position of the k-th contribution to
// node n (ascending element order), -1 when the node has fewer than k+1.
__device__ __forceinline__ double ell_gather(const int n, const int N, const int deg,
                                             const int *__restrict__ ell, const double *__restrict__ YE)
{
   double s = 0.0;
#pragma unroll 8
   for (int k = 0; k < deg; k++)
   {
      const int p = ell[(size_t)k * N + n];
      if (p >= 0) { s += YE[p]; }
   }
   return s;
}

__global__ void __launch_bounds__(256)
mass_gather_k(const int N, const int deg, const int *__restrict__ ell,
              const double *__restrict__ YE, const uint8_t *__restrict__ ess, double *__restrict__ y)
{
   const int n = blockIdx.x * blockDim.x + threadIdx.x;
   if (n >= N) { return; }
   double s = ell_gather(n, N, deg, ell, YE);
   if (ess && ess[n]) { s = 0.0; }
   y[n] = s;
}

int mass_gather(lgh_ctx *c, const double *YE, const uint8_t *ess, double *y)
{
   hipLaunchKernelGGL(mass_gather_k, dim3(ceil_div(c->N, 256)), dim3(256), 0, c->stream, c->N, c->t_deg, c->t_ell, YE, ess, y);
   LGH_HIP_CHECK(hipGetLastError());
   return LGH_OK;
}

int mass_apply_h1(lgh_ctx *c, const double *x, double *y, bool eliminate)
{
   MassArgs a = base_args(c, LGH_SPACE_H1);
   a.x = x;
   a.map = c->h1map;
   a.y = c->YE;
   int rc = launch_mass<1>(c, LGH_SPACE_H1, a);
   if (rc) { return rc; }
   const bool multi = (c->multi != 0);
   const uint8_t *ess = (eliminate && c->cur_ess >= 0 && !multi) ? c->essmask[c->cur_ess] : nullptr;
   rc = mass_gather(c, c->YE, ess, y);
   if (rc) { return rc; }
   if (multi)
   {
      rc = halo_sum(c, y, 1);
      if (rc) { return rc; }
      if (eliminate && c->cur_ess >= 0 && c->ess_count[c->cur_ess] > 0)
      {
         rc = vec_zero_list(c, y, c->ess[c->cur_ess], c->ess_count[c->cur_ess]);
      }
   }
   return rc;
}

int mass_apply_l2(lgh_ctx *c, const double *x, double *y)
{
   MassArgs a = base_args(c, LGH_SPACE_L2);
   a.x = x;
   a.y = y;
   return launch_mass<0>(c, LGH_SPACE_L2, a);
}

// ---- Jacobi diagonal: diag_e[d] = sum_q prod_a B(q_a,d_a)^2 D_e[q] ---------------
template <int DIM>
__global__ void __launch_bounds__(256)
mass_diag_k(const int NE, const int D, const int Q, const double *__restrict__ B,
            const double *__restrict__ Dq, double *__restrict__ yE)
{
   const int ND = (DIM == 2) ? D * D : D * D * D;
   const int NQ = (DIM == 2) ? Q * Q : Q * Q * Q;
   const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
   if (i >= (size_t)NE * ND) { return; }
   const int e = (int)(i / ND), d = (int)(i - (size_t)e * ND);
   const int dx = d % D, dy = (d / D) % D, dz = d / (D * D);
   const double *De = Dq + (size_t)e * NQ;
   double s = 0.0;
   if (DIM == 2)
   {
      for (int qy = 0; qy < Q; qy++)
         for (int qx = 0; qx < Q; qx++)
         {
            const double bxv = B[qx + Q * dx], byv = B[qy + Q * dy];
            s += bxv * bxv * byv * byv * De[qx + Q * qy];
         }
   }
   else
   {
      for (int qz = 0; qz < Q; qz++)
         for (int qy = 0; qy < Q; qy++)
            for (int qx = 0; qx < Q; qx++)
            {
               const double bxv = B[qx + Q * dx], byv = B[qy + Q * dy], bzv = B[qz + Q * dz];
               s += bxv * bxv * byv * byv * bzv * bzv * De[qx + Q * (qy + Q * qz)];
            }
   }
   yE[i] = s;
}

__global__ void __launch_bounds__(256)
reciprocal_k(const int n, const double *__restrict__ x, double *__restrict__ y)
{
   const int i = blockIdx.x * blockDim.x + threadIdx.x;
   if (i < n) { y[i] = 1.0 / x[i]; }
}

int mass_assemble_diag(lgh_ctx *c)
{
   const size_t tot = (size_t)c->NE * c->ND;
   if (c->dim == 2)
   {
      hipLaunchKernelGGL(mass_diag_k<2>, dim3(ceil_div(tot, 256)), dim3(256), 0, c->stream, c->NE,
                         c->D1D, c->Q1D, c->B, c->massD, c->YE);
   }
   else
   {
      hipLaunchKernelGGL(mass_diag_k<3>, dim3(ceil_div(tot, 256)), dim3(256), 0, c->stream, c->NE,
                         c->D1D, c->Q1D, c->B, c->massD, c->YE);
   }
   LGH_HIP_CHECK(hipGetLastError());
   int rc = mass_gather(c, c->YE, nullptr, c->diagV);
   if (rc) { return rc; }
   if (c->multi != 0)
   {
      rc = halo_sum(c, c->diagV, 1);
      if (rc) { return rc; }
   }
   hipLaunchKernelGGL(reciprocal_k, dim3(ceil_div(c->N, 256)), dim3(256), 0, c->stream, c->N,
                      c->diagV, c->dinvV);
   LGH_HIP_CHECK(hipGetLastError());
   c->mass_gen++; // (the velocity solve keeps 1/diag in its own node numbering: lgh_vcg.hip)
   return LGH_OK;
}

} // namespace lgh
