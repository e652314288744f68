// lgh_vcg_k1.hip — K1 of the lockstep velocity solve (lgh_vcg.hip): y_e^c = B^T D_e B d_e^c for the unconverged components,
// d^c = z^c + beta_c d^c, in its column, plane and Kronecker forms (the slab form: lgh_vcg_slab.hip), their launchers and
// the one place that says which of them a context runs (vcg_resolve_k1).
#include "lgh_vcg.hpp"

namespace lgh
{

// ---- K1: y_e^c = B^T D_e B d_e^c for the unconverged components, d^c = z^c + beta_c d^c.
// Persistent workgroups: the grid is one resident wave of workgroups; each walks
// batches b, b+G, ... of NEB elements.  Profiling the one-batch-per-workgroup form
// showed it bound by the per-workgroup latency chain (map -> gather -> 4 barriers
// -> store -> partial/ticket round trip) times 2.3 waves of workgroups, not by
// bytes or FMAs.  Here the map entries, the gathers of all components and the
// quadrature data of batch i+1 are in flight while batch i is contracted, and
// the dot-product partials are published once per workgroup.
template <int D, int Q, int NEB>
__global__ void __launch_bounds__(Q *Q *NEB, (Q >= 8) ? 1 : 2)
vcg_apply_3d(const VcgArgs a, const int nbatch)
{
   constexpr int NQ = Q * Q * Q, ND = D * D * D;
   constexpr int SX = (ND > D * Q * Q) ? ND : D * Q * Q;
   constexpr int SA = D * D * Q;
   constexpr int SAE = (SA > D * Q * D) ? SA : D * Q * D;
   constexpr int OFF_A = kVC * SX, OFF_IN = OFF_A + kVC * SAE;
   constexpr int PER = OFF_IN + kVC * ND + 1; // per component: C, A/E work buffers, gathered direction
   constexpr int NT = Q * Q * NEB;
   constexpr int GPT = (NEB * ND + NT - 1) / NT; // gather items per thread
   __shared__ double smem[NEB * PER];
   __shared__ double red[48];

   if (a.s->all_done) { return; }
   const int tid = threadIdx.x;
   const int tx = tid % Q, ty = (tid / Q) % Q, eb = tid / (Q * Q);
   const int G = gridDim.x;
   double *sX = smem + eb * PER;  // [c][SX]
   double *sA = sX + OFF_A;       // [c][SAE]
   double *sIn = sX + OFF_IN;     // [c][ND]
   const bool first = a.s->first != 0;
   bool todo[kVC];
   double beta[kVC];
#pragma unroll
   for (int c = 0; c < kVC; c++) { todo[c] = a.s->done[c] == 0; }
   if (a.multi && !first && !vcg_pending_update(a.s, a.iter, blockIdx.x == 0 && tid == 0, todo)) { return; }
#pragma unroll
   for (int c = 0; c < kVC; c++) { beta[c] = (first || !todo[c]) ? 0.0 : a.s->rz[c] / a.s->rz_prev[c]; }
   // the 1-D table lives in LDS (thread-dependent rows are read at use: the
   // persistent kernel is register-, not LDS-limited)
   __shared__ double sB[Q * D];
   for (int i = tid; i < Q * D; i += NT) { sB[i] = a.B[i]; }
   const double *bxp = sB + tx;         // B[tx + Q*d]
   const double *byp = sB + ty;         // B[ty + Q*d]
   const double *brxp = sB + Q * (tx < D ? tx : 0); // B[q + Q*tx]
   const double *bryp = sB + Q * (ty < D ? ty : 0); // B[q + Q*ty]

   // in-flight state of the NEXT batch
   int mi[GPT];
   double gz[kVC][GPT], gd[kVC][GPT], gi[GPT], dqn[Q];
   auto load_map = [&](const int b) {
      const int e0 = b * NEB, nel = min(NEB, a.NE - e0);
#pragma unroll
      for (int k = 0; k < GPT; k++)
      {
         const int i = tid + k * NT;
         mi[k] = (i < nel * ND) ? a.map[(size_t)e0 * ND + i] : -1;
      }
   };
   auto load_data = [&](const int b) {
      const int e = b * NEB + eb;
#pragma unroll
      for (int k = 0; k < GPT; k++) { gi[k] = (mi[k] >= 0) ? a.dinv[mi[k]] : 0.0; }
#pragma unroll
      for (int c = 0; c < kVC; c++)
      {
         if (!todo[c]) { continue; }
#pragma unroll
         for (int k = 0; k < GPT; k++)
         {
            gz[c][k] = (mi[k] >= 0) ? a.r[(size_t)c * a.N + mi[k]] : 0.0;
            gd[c][k] = (mi[k] >= 0 && !first) ? a.d[(size_t)c * a.N + mi[k]] : 0.0;
         }
      }
      if (e < a.NE)
      {
         const double *p = a.DqFull + (size_t)e * NQ + tx + Q * ty;
#pragma unroll
         for (int qz = 0; qz < Q; qz++) { dqn[qz] = p[Q * Q * qz]; }
      }
      else
      {
#pragma unroll
         for (int qz = 0; qz < Q; qz++) { dqn[qz] = 0.0; }
      }
   };

   double dots[kVC] = {0.0, 0.0, 0.0};
   int b = xcd_swizzle(blockIdx.x, G);
   if (b < nbatch)
   {
      load_map(b);
      load_data(b);
   }
   for (; b < nbatch; b += G)
   {
      const int e0 = b * NEB;
      const int e = e0 + eb;
      const bool active = (e < a.NE);
      // take ownership of the prefetched batch: quadrature data to registers, the
      // directions d = z + beta d of every active component to LDS (K2 stores the
      // same values later); after that the prefetch registers are free again
      double dq[Q];
#pragma unroll
      for (int qz = 0; qz < Q; qz++) { dq[qz] = dqn[qz]; }
      __syncthreads(); // previous batch finished with the LDS buffers
#pragma unroll
      for (int c = 0; c < kVC; c++)
      {
         if (!todo[c]) { continue; }
#pragma unroll
         for (int k = 0; k < GPT; k++)
         {
            const int i = tid + k * NT;
            if (mi[k] >= 0)
            {
               const int el = i / ND, dd = i - el * ND;
               smem[el * PER + OFF_IN + c * ND + dd] = fma(beta[c], gd[c][k], __dmul_rn(gz[c][k], gi[k]));
            }
         }
      }
      const int bn = b + G;
      const bool have_next = bn < nbatch;
      if (have_next) { load_map(bn); } // its gathers are issued one stage later
      __syncthreads();
      // All active components advance through each stage together: 5 barriers per
      // batch instead of 5 per component.
      // forward x: thread (qx = tx, dy = ty < D)
      double xcol[kVC][D];
#pragma unroll
      for (int c = 0; c < kVC; c++)
      {
         if (!todo[c]) { continue; }
         const double *sXc = sIn + c * ND;
         double *sAc = sA + c * SAE;
#pragma unroll
         for (int dz = 0; dz < D; dz++) { xcol[c][dz] = (tx < D && ty < D) ? sXc[tx + D * (ty + D * dz)] : 0.0; }
         if (ty < D)
         {
#pragma unroll
            for (int dz = 0; dz < D; dz++)
            {
               double u = 0.0;
#pragma unroll
               for (int dx = 0; dx < D; dx++) { u += bxp[Q * dx] * sXc[dx + D * (ty + D * dz)]; }
               sAc[tx + Q * (ty + D * dz)] = u;
            }
         }
      }
      __syncthreads();
      if (have_next) { load_data(bn); } // map entries have had a stage to arrive
      // forward y, z; scale by the quadrature data; backward z (registers)
#pragma unroll
      for (int c = 0; c < kVC; c++)
      {
         if (!todo[c]) { continue; }
         const double *sAc = sA + c * SAE;
         double *sCc = sX + c * SX;
         double bb[D];
#pragma unroll
         for (int dz = 0; dz < D; dz++)
         {
            double u = 0.0;
#pragma unroll
            for (int dy = 0; dy < D; dy++) { u += byp[Q * dy] * sAc[tx + Q * (dy + D * dz)]; }
            bb[dz] = u;
         }
         double qv[Q];
#pragma unroll
         for (int qz = 0; qz < Q; qz++)
         {
            double u = 0.0;
#pragma unroll
            for (int dz = 0; dz < D; dz++) { u += sB[qz + Q * dz] * bb[dz]; }
            qv[qz] = u * dq[qz];
         }
#pragma unroll
         for (int dz = 0; dz < D; dz++)
         {
            double u = 0.0;
#pragma unroll
            for (int qz = 0; qz < Q; qz++) { u += sB[qz + Q * dz] * qv[qz]; }
            sCc[tx + Q * (ty + Q * dz)] = u;
         }
      }
      __syncthreads();
      // backward x: thread (dx = tx < D, qy = ty)
      if (tx < D)
      {
#pragma unroll
         for (int c = 0; c < kVC; c++)
         {
            if (!todo[c]) { continue; }
            const double *sCc = sX + c * SX;
            double *sEc = sA + c * SAE;
#pragma unroll
            for (int dz = 0; dz < D; dz++)
            {
               double u = 0.0;
#pragma unroll
               for (int qx = 0; qx < Q; qx++) { u += brxp[qx] * sCc[qx + Q * (ty + Q * dz)]; }
               sEc[tx + D * (ty + Q * dz)] = u;
            }
         }
      }
      __syncthreads();
      // backward y: thread (dx = tx < D, dy = ty < D)
      if (tx < D && ty < D && active)
      {
#pragma unroll
         for (int c = 0; c < kVC; c++)
         {
            if (!todo[c]) { continue; }
            const double *sEc = sA + c * SAE;
            double *yc = a.YE + (size_t)c * a.ye_stride;
            double dot = 0.0;
#pragma unroll
            for (int dz = 0; dz < D; dz++)
            {
               double u = 0.0;
#pragma unroll
               for (int qy = 0; qy < Q; qy++) { u += bryp[qy] * sEc[tx + D * (qy + Q * dz)]; }
               yc[tx + D * (ty + D * dz) + (size_t)ND * e] = u;
               dot += xcol[c][dz] * u;
            }
            dots[c] += dot;
         }
      }
   }
   double bp[kVC];
   block_sum3(dots[0], dots[1], dots[2], red, bp);
   double total[kVC];
   if (grid_sum3_last_block(bp, a.partials, a.stride, a.ticket, red, total))
   {
      if (tid == 0)
      {
         VcgScalars *s = a.s;
         for (int c = 0; c < kVC; c++)
         {
            if (!todo[c]) { continue; }
            s->den[c] = total[c];
            if (total[c] == 0.0 && !a.multi) { s->done[c] = 1; } // breakdown, as upstream
         }
         s->first = 0;
      }
   }
}

// ---- K1, plane-per-thread form --------------------------------------------------
// The (qx, qy)-column form above is bound by LDS bandwidth: every contraction
// stage re-reads its operands (and the 1-D table) from LDS, 474 doubles per thread
// and batch, 80 % of its run time.  Here a thread owns one x-index of one
// component of one element and keeps the whole (y, z) plane of that index in
// registers: only the two x contractions exchange data through LDS (64 + 96
// doubles read per thread), the y and z contractions and the scaling by the
// quadrature data run on registers with the 1-D table in scalar registers (its
// indices are loop constants there), i.e. as FMAs with an SGPR operand.
// The quadrature data of a batch is staged through LDS (NQ/TE values in flight per
// thread, shared by the three components), which keeps the register count low
// enough for two workgroups per CU.
// Software pipeline: the element->node map runs two batches ahead, the gathers and
// the quadrature data one batch ahead.

template <int D, int Q, int NEB, bool SYM>
__global__ void __launch_bounds__(kVC *Q *NEB, 2)
vcg_apply_plane(const VcgArgs a, const int nbatch)
{
   constexpr int NQ = Q * Q * Q, ND = D * D * D, DD = D * D;
   constexpr int TE = kVC * Q; // threads per element
   constexpr int NT = TE * NEB;
   // LDS strides: consecutive (element, component) groups of a wave are skewed by
   // 16 B modulo 128 B, so the broadcast reads of different groups hit different banks
   constexpr int CS = (ND + 3) & ~1;     // direction d of one component
   constexpr int CE = (DD * Q + 3) & ~1; // x-contracted result of one component, [dy,dz][qx]
   constexpr int PER0 = kVC * (CS + CE);
   constexpr int PER = PER0 + ((6 - PER0 % 16) + 16) % 16;
   constexpr int GPT = (NEB * ND + NT - 1) / NT; // gather items per thread
   constexpr int DPT = (NQ + TE - 1) / TE;       // quadrature values staged per thread
   constexpr int DSTR = (NQ + 7) & ~1;
   __shared__ double smem[NEB * (PER + DSTR)];
   __shared__ double red[48];

   const int tid = threadIdx.x;
   unsigned long long t_start = 0, t_loop = 0;
   unsigned long long c_start = 0;
   if (a.trace) { t_start = wall_clock64(); c_start = clock64(); }
   const int eb = tid / TE, lt = tid - eb * TE;
   const int c = lt / Q, qx = lt - c * Q;
   const int G = gridDim.x;
   double *sIn = smem + eb * PER + c * CS;           // [dx + D*(dy + D*dz)]
   double *sE = smem + eb * PER + kVC * CS + c * CE; // [qx + Q*(dy + D*dz)]
   double *sD = smem + NEB * PER + eb * DSTR;        // [qx + Q*(qy + Q*qz)]

   int mi[GPT];
   auto load_map = [&](const int b) {
      // (no predicates on the loads of the pipeline: items beyond a ragged last batch read a valid entry, their values
      // are never written to LDS - predicated loads cost a branch each and cut the loop into 40 basic blocks that the
      // scheduler cannot interleave with the contractions)
      const int e0 = b * NEB, last = min(NEB, a.NE - e0) * ND - 1;
#pragma unroll
      for (int k = 0; k < GPT; k++)
      {
         const int i = tid + k * NT;
         mi[k] = a.map[(size_t)e0 * ND + min(i, last)];
      }
   };
   int b = xcd_swizzle(blockIdx.x, G);
   if (b < nbatch) { load_map(b); } // in flight while the scalars are read

   if (a.s->all_done) { return; }
   const bool first = a.s->first != 0;
   bool todo[kVC];
   double beta[kVC];
#pragma unroll
   for (int k = 0; k < kVC; k++) { todo[k] = a.s->done[k] == 0; }
   if (a.multi && !first && !vcg_pending_update(a.s, a.iter, blockIdx.x == 0 && tid == 0, todo)) { return; }
#pragma unroll
   for (int k = 0; k < kVC; k++) { beta[k] = (first || !todo[k]) ? 0.0 : a.s->rz[k] / a.s->rz_prev[k]; }
   const bool mine = (c == 0) ? todo[0] : (c == 1) ? todo[1] : todo[2];
   // 1-D table: scalar registers for the register-resident contractions, this
   // thread's row / column for the two x contractions
   // SYM: the table is mirror symmetric, B[q,d] = B[Q-1-q, D-1-d] (Gauss-Lobatto or Bernstein basis at Gauss-Legendre
   // points; checked by lgh_create), and half of it serves all indices - 24 scalar registers less, without which
   // the kernel spills 40 of them to vector lanes and reads them back ~50 times per batch
   constexpr int QD = Q * D, HB = SYM ? (QD + 1) / 2 : QD;
   double Bsr[HB];
#pragma unroll
   for (int i = 0; i < HB; i++) { Bsr[i] = uniform_f64(a.B[i]); }
   auto Bs = [&](const int idx) -> double { return (SYM && idx >= HB) ? Bsr[QD - 1 - idx] : Bsr[idx]; };
   double bx[D], bt[Q];
#pragma unroll
   for (int dx = 0; dx < D; dx++) { bx[dx] = a.B[qx + Q * dx]; }
#pragma unroll
   for (int q = 0; q < Q; q++) { bt[q] = a.B[q + Q * (qx < D ? qx : 0)]; }
   // Everything loaded so far (map, scalars, tables) is complete before the pipelined
   // loop starts: the compiler's wait-count analysis is loop-conservative and otherwise
   // treats these one-time loads as possibly outstanding in EVERY iteration, which with
   // in-order vmcnt put an s_waitcnt vmcnt(6) - i.e. a wait for the next batch's
   // gathers - ahead of the first FMA of each batch.
   __builtin_amdgcn_s_waitcnt(0x0F70); // vmcnt(0)

   double gz[kVC][GPT], gd[kVC][GPT], gi[GPT], dq[DPT];
   auto load_gather = [&]() { // nodes of mi[]: residual r, direction d, 1/diag
#pragma unroll
      for (int k = 0; k < GPT; k++) { gi[k] = a.dinv[mi[k]]; }
#pragma unroll
      for (int k2 = 0; k2 < kVC; k2++)
      {
#pragma unroll
         for (int k = 0; k < GPT; k++)
         {
            gz[k2][k] = a.r[(size_t)k2 * a.N + mi[k]];
            gd[k2][k] = first ? 0.0 : a.d[(size_t)k2 * a.N + mi[k]];
         }
      }
   };
   auto load_dq = [&](const int bb) {
      const int e = min(bb * NEB + eb, a.NE - 1);
      const double se = a.Se[e];
#pragma unroll
      for (int k = 0; k < DPT; k++)
      {
         const int j = lt + k * TE;
         dq[k] = a.Dq[(size_t)e * a.dqs + ((DPT * TE == NQ) ? j : min(j, NQ - 1))] * se;
      }
   };

   double dot = 0.0;
   if (b < nbatch)
   {
      load_gather();
      load_dq(b);
      if (b + G < nbatch) { load_map(b + G); }
   }
   for (; b < nbatch; b += G)
   {
      const int e = b * NEB + eb;
      const bool active = (e < a.NE) && mine;
      const int nit = min(NEB, a.NE - b * NEB) * ND;
      __syncthreads(); // previous batch finished with the LDS buffers
      // directions d = z + beta d of every active component (K2 stores the same
      // values), quadrature data
#pragma unroll
      for (int k = 0; k < GPT; k++)
      {
         const int i = tid + k * NT;
         if (i < nit)
         {
            const int el = i / ND, dd = i - el * ND;
#pragma unroll
            for (int k2 = 0; k2 < kVC; k2++)
            {
               smem[el * PER + k2 * CS + dd] = fma(beta[k2], gd[k2][k], __dmul_rn(gz[k2][k], gi[k]));
            }
         }
      }
#pragma unroll
      for (int k = 0; k < DPT; k++)
      {
         const int j = lt + k * TE;
         if ((DPT * TE == NQ) || j < NQ) { sD[j] = dq[k]; }
      }
      // next batch: gathers and quadrature data now, the map of the one after
      const int bn = b + G;
      if (bn < nbatch)
      {
         load_gather();
         load_dq(bn);
         if (bn + G < nbatch) { load_map(bn + G); }
      }
      __syncthreads();
      // forward x: t[dy,dz] = sum_dx B[qx,dx] d[dx,dy,dz]
      double t[DD];
#pragma unroll
      for (int k = 0; k < DD; k++)
      {
         double u = 0.0;
#pragma unroll
         for (int dx = 0; dx < D; dx++) { u = fma(bx[dx], sIn[dx + D * k], u); }
         t[k] = u;
      }
      // forward y: w[qy][dz] = sum_dy B[qy,dy] t[dy,dz]
      double w[Q][D];
#pragma unroll
      for (int qy = 0; qy < Q; qy++)
      {
#pragma unroll
         for (int dz = 0; dz < D; dz++)
         {
            double u = 0.0;
#pragma unroll
            for (int dy = 0; dy < D; dy++) { u = fma(Bs(qy + Q * dy), t[dy + D * dz], u); }
            w[qy][dz] = u;
         }
      }
      // per qy row: forward z, scale by the quadrature data, backward z (in place)
#pragma unroll
      for (int qy = 0; qy < Q; qy++)
      {
         double cz[Q];
#pragma unroll
         for (int qz = 0; qz < Q; qz++)
         {
            double u = 0.0;
#pragma unroll
            for (int dz = 0; dz < D; dz++) { u = fma(Bs(qz + Q * dz), w[qy][dz], u); }
            cz[qz] = u * sD[qx + Q * (qy + Q * qz)];
         }
#pragma unroll
         for (int dz = 0; dz < D; dz++)
         {
            double u = 0.0;
#pragma unroll
            for (int qz = 0; qz < Q; qz++) { u = fma(Bs(qz + Q * dz), cz[qz], u); }
            w[qy][dz] = u;
         }
      }
      // backward y: sum_qy B[qy,dy] w[qy][dz]; hand the plane over
#pragma unroll
      for (int dz = 0; dz < D; dz++)
      {
#pragma unroll
         for (int dy = 0; dy < D; dy++)
         {
            double u = 0.0;
#pragma unroll
            for (int qy = 0; qy < Q; qy++) { u = fma(Bs(qy + Q * dy), w[qy][dz], u); }
            sE[qx + Q * (dy + D * dz)] = u;
         }
      }
      __syncthreads();
      // backward x: thread dx = qx < D sums over the Q planes
      if (qx < D && active)
      {
         double *yc = a.YE + (size_t)c * a.ye_stride + (size_t)ND * e;
#pragma unroll
         for (int k = 0; k < DD; k++)
         {
            double u = 0.0;
#pragma unroll
            for (int q = 0; q < Q; q++) { u = fma(bt[q], sE[q + Q * k], u); }
            yc[qx + D * k] = u;
            dot = fma(sIn[qx + D * k], u, dot);
         }
      }
   }
   if (a.trace) { t_loop = wall_clock64(); }
   double bp[kVC];
   block_sum3(c == 0 ? dot : 0.0, c == 1 ? dot : 0.0, c == 2 ? dot : 0.0, red, bp);
   double total[kVC];
   if (grid_sum3_last_block_flat(bp, a.partials, a.stride, a.ticket, red, total))
   {
      if (tid == 0)
      {
         VcgScalars *s = a.s;
         for (int k = 0; k < kVC; k++)
         {
            if (!todo[k]) { continue; }
            s->den[k] = total[k];
            if (total[k] == 0.0 && !a.multi) { s->done[k] = 1; } // breakdown, as upstream
         }
         s->first = 0;
      }
   }
   if (a.trace && tid == 0)
   {
      unsigned xcc = 0, hwid = 0;
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
      a.trace[kTraceRec * blockIdx.x + 0] = t_start;
      a.trace[kTraceRec * blockIdx.x + 1] = t_loop;
      a.trace[kTraceRec * blockIdx.x + 2] = wall_clock64();
      a.trace[kTraceRec * blockIdx.x + 3] = clock64() - c_start; // shader cycles between the two wall-clock stamps 0 and 2
   }
}

// ---- K1, plane form for D1D >= 5 (Q4Q3 0x358, Q5Q4 0x36A) ------------------------
// Same thread layout as vcg_apply_plane, sized for the larger planes: at Q1D = 10 the
// (y, z) plane of one x-index is 100 doubles, so HY = 2 threads (adjacent lanes) share
// it, each taking Q/HY of its qy rows; their partial backward-y sums are combined with
// one DPP lane swap per pair of values.  The 1-D table sits in scalar registers in
// half: the Gauss-Lobatto basis at Gauss-Legendre points is mirror symmetric,
// B[q,d] = B[Q-1-q, D-1-d], so Q*D/2 values serve all Q*D indices (60 doubles would
// not fit the scalar file, 30 do).  One batch of NEB elements per workgroup; its
// quadrature data is fetched in one coalesced sweep at the start (when the registers
// are still free) into the LDS region that later takes the x-contracted planes.
__device__ __forceinline__ double lane_pair_swap(const double v)
{
   int lo = __double2loint(v), hi = __double2hiint(v);
   lo = __builtin_amdgcn_mov_dpp(lo, 0xB1, 0xF, 0xF, true); // quad_perm [1,0,3,2]
   hi = __builtin_amdgcn_mov_dpp(hi, 0xB1, 0xF, 0xF, true);
   return __hiloint2double(hi, lo);
}

template <int D, int Q, int HY, int NEB, bool SEP>
__global__ void __launch_bounds__(kVC *Q *HY *NEB, 2)
vcg_apply_plane_ho(const VcgArgs a)
{
   constexpr int NQ = Q * Q * Q, ND = D * D * D, DD = D * D, QD = Q * D, HB = QD / 2;
   constexpr int TE = kVC * Q * HY, NT = TE * NEB, QH = Q / HY;
   static_assert(Q % HY == 0 && (HY == 1 || HY == 2), "qy rows split evenly over one or two lanes");
   static_assert(QD % 2 == 0 && TE % 2 == 0, "mirror-symmetric table, lane pairs inside a wave");
   constexpr int CS = (ND + 3) & ~1;
   constexpr int CE = (DD * Q + 3) & ~1;
   constexpr int PER0 = kVC * (CS + CE);
   constexpr int PER = PER0 + ((6 - PER0 % 16) + 16) % 16;
   constexpr int GPT = (NEB * ND + NT - 1) / NT;
   constexpr int DPT = (NEB * NQ + NT - 1) / NT;
   static_assert(kVC * CE >= NQ, "the quadrature data of an element is staged where its x-contracted planes go later");
   // SEP (compact mass data of a tensor-product rule): value(q, e) = Se[e] w[qx] w[qy] w[qz] with the weights in scalar
   // registers - no sweep over the quadrature data, nothing staged in LDS, one barrier less
   __shared__ double smem[NEB * PER];
   __shared__ double sB[QD];
   __shared__ double red[48];

   const int tid = threadIdx.x;
   const int eb = tid / TE, lt = tid - eb * TE;
   const int c = lt / (Q * HY), r2 = lt - c * (Q * HY);
   const int qx = r2 / HY, h = r2 - qx * HY;
   const int e0 = xcd_swizzle(blockIdx.x, gridDim.x) * NEB, e = e0 + eb;
   const int nel = min(NEB, a.NE - e0);
   double *sIn = smem + eb * PER + c * CS;           // [dx + D*(dy + D*dz)]
   double *sE = smem + eb * PER + kVC * CS + c * CE; // [qx + Q*(dy + D*dz)]
   const double *sD = smem + eb * PER + kVC * CS;    // [qx + Q*(qy + Q*qz)] until the planes are handed over

   int mi[GPT];
#pragma unroll
   for (int k = 0; k < GPT; k++)
   {
      const int i = tid + k * NT;
      mi[k] = (i < nel * ND) ? a.map[(size_t)e0 * ND + i] : -1;
   }
   if (a.s->all_done) { return; }
   // quadrature data of the batch: one coalesced sweep while the registers are still free
   double dst[SEP ? 1 : DPT];
   if (!SEP)
   {
#pragma unroll
      for (int k = 0; k < DPT; k++)
      {
         const int i = tid + k * NT, ei = i / NQ;
         dst[k] = (i < nel * NQ) ? a.Dq[(size_t)(e0 + ei) * a.dqs + (i - ei * NQ)] * a.Se[e0 + ei] : 0.0;
      }
   }
   double ws[SEP ? (Q + 1) / 2 : 1]; // (mirror symmetric, checked by lgh_create: w[q] = w[Q - 1 - q])
   auto wq = [&](const int q) -> double { return ws[SEP ? (q < (Q + 1) / 2 ? q : Q - 1 - q) : 0]; };
   double wxe = 0.0;
   if (SEP)
   {
#pragma unroll
      for (int q = 0; q < (Q + 1) / 2; q++) { ws[q] = uniform_f64(a.w1[q]); }
      wxe = a.w1[qx] * a.Se[min(e, a.NE - 1)];
   }
   const bool first = a.s->first != 0;
   bool todo[kVC];
   double beta[kVC];
#pragma unroll
   for (int k = 0; k < kVC; k++) { todo[k] = a.s->done[k] == 0; }
   if (a.multi && !first && !vcg_pending_update(a.s, a.iter, blockIdx.x == 0 && tid == 0, todo)) { return; }
#pragma unroll
   for (int k = 0; k < kVC; k++) { beta[k] = (first || !todo[k]) ? 0.0 : a.s->rz[k] / a.s->rz_prev[k]; }
   const bool active = (e < a.NE) && ((c == 0) ? todo[0] : (c == 1) ? todo[1] : todo[2]);
   double Bs[HB];
#pragma unroll
   for (int i = 0; i < HB; i++) { Bs[i] = uniform_f64(a.B[i]); }
   auto Bc = [&](const int q, const int d) -> double {
      const int idx = q + Q * d;
      return idx < HB ? Bs[idx] : Bs[QD - 1 - idx];
   };
   for (int i = tid; i < QD; i += NT) { sB[i] = a.B[i]; }
   if (!SEP)
   {
#pragma unroll
      for (int k = 0; k < DPT; k++)
      {
         const int i = tid + k * NT;
         if (i < NEB * NQ)
         {
            const int el = i / NQ, j = i - el * NQ;
            smem[el * PER + kVC * CS + j] = dst[k];
         }
      }
   }
   // directions d = z + beta d of the three components (K2 stores the same values)
#pragma unroll
   for (int k = 0; k < GPT; k++)
   {
      const int i = tid + k * NT;
      if (i < nel * ND)
      {
         const int el = i / ND, dd = i - el * ND;
         const int n = mi[k];
         const double gi = a.dinv[n];
#pragma unroll
         for (int k2 = 0; k2 < kVC; k2++)
         {
            const double gz = a.r[(size_t)k2 * a.N + n];
            const double gd = first ? 0.0 : a.d[(size_t)k2 * a.N + n];
            smem[el * PER + k2 * CS + dd] = fma(beta[k2], gd, __dmul_rn(gz, gi));
         }
      }
   }
   __syncthreads();
   // forward x: t[dy,dz] = sum_dx B[qx,dx] d[dx,dy,dz] (each lane of a pair forms it)
   double t[DD];
   {
      double bx[D];
#pragma unroll
      for (int dx = 0; dx < D; dx++) { bx[dx] = sB[qx + Q * dx]; }
#pragma unroll
      for (int k = 0; k < DD; k++)
      {
         double u = 0.0;
#pragma unroll
         for (int dx = 0; dx < D; dx++) { u = fma(bx[dx], sIn[dx + D * k], u); }
         t[k] = u;
      }
   }
   // this lane's qy rows: forward y, then per row forward z, scaling, backward z; backward y accumulated
   double acc[DD];
#pragma unroll
   for (int k = 0; k < DD; k++) { acc[k] = 0.0; }
#pragma unroll
   for (int r = 0; r < QH; r++)
   {
      double by[D]; // table row of qy = h*QH + r
#pragma unroll
      for (int dy = 0; dy < D; dy++)
      {
         double v = Bc(r, dy);
         if (HY == 2) { v = h ? Bc(QH + r, dy) : v; }
         by[dy] = v;
      }
      double wr[D];
#pragma unroll
      for (int dz = 0; dz < D; dz++)
      {
         double u = 0.0;
#pragma unroll
         for (int dy = 0; dy < D; dy++) { u = fma(by[dy], t[dy + D * dz], u); }
         wr[dz] = u;
      }
      double wrow = 0.0; // SEP: s_e w[qx] w[qy] of this row
      if (SEP)
      {
         double wy = wq(r);
         if (HY == 2) { wy = h ? wq(QH + r) : wy; }
         wrow = wxe * wy;
      }
      double cz[Q];
#pragma unroll
      for (int qz = 0; qz < Q; qz++)
      {
         double u = 0.0;
#pragma unroll
         for (int dz = 0; dz < D; dz++) { u = fma(Bc(qz, dz), wr[dz], u); }
         cz[qz] = SEP ? (u * wrow) * wq(qz) : u * sD[qx + Q * (h * QH + r) + Q * Q * qz];
      }
#pragma unroll
      for (int dz = 0; dz < D; dz++)
      {
         double u = 0.0;
#pragma unroll
         for (int qz = 0; qz < Q; qz++) { u = fma(Bc(qz, dz), cz[qz], u); }
#pragma unroll
         for (int dy = 0; dy < D; dy++) { acc[dy + D * dz] = fma(by[dy], u, acc[dy + D * dz]); }
      }
   }
   if (!SEP) { __syncthreads(); } // every lane of the element has read its quadrature data
   // hand the plane over: lane h of a pair delivers the (dy,dz) entries k = h (mod 2)
   if (HY == 1)
   {
#pragma unroll
      for (int k = 0; k < DD; k++) { sE[qx + Q * k] = acc[k]; }
   }
   else
   {
#pragma unroll
      for (int k = 0; k + 1 < DD; k += 2)
      {
         const double give = h ? acc[k] : acc[k + 1];
         const double keep = h ? acc[k + 1] : acc[k];
         sE[qx + Q * (k + h)] = keep + lane_pair_swap(give);
      }
      if (DD & 1)
      {
         const double tot = acc[DD - 1] + lane_pair_swap(acc[DD - 1]);
         if (h == 0) { sE[qx + Q * (DD - 1)] = tot; }
      }
   }
   __syncthreads();
   // backward x: lane (dx = qx < D, h) sums the Q planes for its share of the (dy,dz) pairs
   double dot = 0.0;
   if (qx < D && active)
   {
      double bt[Q];
#pragma unroll
      for (int q = 0; q < Q; q++) { bt[q] = sB[q + Q * qx]; }
      double *yc = a.YE + (size_t)c * a.ye_stride + (size_t)ND * e;
      constexpr int KH = (DD + HY - 1) / HY;
#pragma unroll
      for (int kk = 0; kk < KH; kk++)
      {
         const int k = h * KH + kk;
         if (k < DD)
         {
            double u = 0.0;
#pragma unroll
            for (int q = 0; q < Q; q++) { u = fma(bt[q], sE[q + Q * k], u); }
            yc[qx + D * k] = u;
            dot = fma(sIn[qx + D * k], u, dot);
         }
      }
   }
   double bp[kVC];
   block_sum3(c == 0 ? dot : 0.0, c == 1 ? dot : 0.0, c == 2 ? dot : 0.0, red, bp);
   double total[kVC];
   if (grid_sum3_last_block(bp, a.partials, a.stride, a.ticket, red, total))
   {
      if (tid == 0)
      {
         VcgScalars *s = a.s;
         for (int k = 0; k < kVC; k++)
         {
            if (!todo[k]) { continue; }
            s->den[k] = total[k];
            if (total[k] == 0.0 && !a.multi) { s->done[k] = 1; } // breakdown, as upstream
         }
         s->first = 0;
      }
   }
}

// ---- K1, Kronecker form, any order (compact mass data on a tensor-product rule; a.M1 = 1-D mass tile B^T diag(w) B):
// A_e = s_e M1 (x) M1 (x) M1 - three contractions of D on the D^3 dofs of an (element, component) item instead of the
// six of D x Q and the pass over the quadrature points: 3 D^4 FMAs per item (D = 6: 3 888 against ~21 000), no
// quadrature-point values; what is left is the traffic: the gathers of r, d_old, 1/diag and the E-vector out.  The
// Q3Q2 meshes of 20 000 zones and more take the slab form of the same operator (lgh_vcg_slab.hip), everything else
// this kernel.  One workgroup of 256 threads = NEB consecutive elements x 3 components; a thread owns one row of D
// values per stage (x rows (item, dz, dy), y rows (item, dz, dx), z rows (item, dy, dx)); (d, A d) = sum over the item's
// dofs of d y.  Same operator in exact arithmetic as vcg_apply_plane(_ho); rounding differs (tests/test_gpu_k1.py).
template <int D, int NEB>
__global__ void __launch_bounds__(256)
vcg_apply_kron(const VcgArgs a)
{
   constexpr int ND = D * D * D, DD = D * D, NT = 256, NI = NEB * kVC;
   __shared__ double sIn[NI * ND], sT1[NI * ND], sT2[NI * ND];
   __shared__ double red[48];
   const int tid = threadIdx.x;
   const int e0 = xcd_swizzle(blockIdx.x, gridDim.x) * NEB;
   const int nel = min(NEB, a.NE - e0);
   constexpr int GPT = (NEB * ND + NT - 1) / NT;
   int mi[GPT];
#pragma unroll
   for (int k = 0; k < GPT; k++)
   {
      const int i = tid + k * NT;
      mi[k] = (i < nel * ND) ? a.map[(size_t)e0 * ND + i] : -1;
   }
   if (a.s->all_done) { return; }
   const bool first = a.s->first != 0;
   bool todo[kVC];
   double beta[kVC];
#pragma unroll
   for (int k = 0; k < kVC; k++) { todo[k] = a.s->done[k] == 0; }
   if (a.multi && !first && !vcg_pending_update(a.s, a.iter, blockIdx.x == 0 && tid == 0, todo)) { return; }
#pragma unroll
   for (int k = 0; k < kVC; k++) { beta[k] = (first || !todo[k]) ? 0.0 : a.s->rz[k] / a.s->rz_prev[k]; }
   double M[DD]; // M[i + D j], symmetric, in scalar registers
#pragma unroll
   for (int i = 0; i < DD; i++) { M[i] = uniform_f64(a.M1[i]); }
   // directions d = z + beta d of the three components (K2 stores the same values); item = k2 * NEB + el
#pragma unroll
   for (int k = 0; k < GPT; k++)
   {
      const int i = tid + k * NT;
      if (i < nel * ND)
      {
         const int el = i / ND, dd = i - el * ND;
         const int n = mi[k];
         const double gi = a.dinv[n];
#pragma unroll
         for (int k2 = 0; k2 < kVC; k2++)
         {
            const double gz = a.r[(size_t)k2 * a.N + n];
            const double gd = first ? 0.0 : a.d[(size_t)k2 * a.N + n];
            sIn[(k2 * NEB + el) * ND + dd] = fma(beta[k2], gd, __dmul_rn(gz, gi));
         }
      }
   }
   __syncthreads();
   auto live = [&](const int item) -> bool {
      const int k2 = item / NEB, el = item - k2 * NEB;
      return el < nel && ((k2 == 0) ? todo[0] : (k2 == 1) ? todo[1] : todo[2]);
   };
   auto row = [&](const double (&u)[D], double (&o)[D]) {
#pragma unroll
      for (int i = 0; i < D; i++)
      {
         double t = M[i] * u[0];
#pragma unroll
         for (int j = 1; j < D; j++) { t = fma(M[i + D * j], u[j], t); }
         o[i] = t;
      }
   };
   // x: rows of D consecutive values
   for (int r = tid; r < NI * DD; r += NT)
   {
      if (!live(r / DD)) { continue; }
      double u[D], o[D];
#pragma unroll
      for (int j = 0; j < D; j++) { u[j] = sIn[r * D + j]; }
      row(u, o);
#pragma unroll
      for (int i = 0; i < D; i++) { sT1[r * D + i] = o[i]; }
   }
   __syncthreads();
   // y: rows (item, dz, dx), stride D
   for (int r = tid; r < NI * DD; r += NT)
   {
      if (!live(r / DD)) { continue; }
      const int dx = r % D, iz = r / D; // iz = dz + D item
      const int base = iz * DD + dx;
      double u[D], o[D];
#pragma unroll
      for (int j = 0; j < D; j++) { u[j] = sT1[base + D * j]; }
      row(u, o);
#pragma unroll
      for (int i = 0; i < D; i++) { sT2[base + D * i] = o[i]; }
   }
   __syncthreads();
   // z: rows (item, dy, dx), stride D^2; the element factor; E-vector out and the partials of (d, A d)
   double dot[kVC] = {0.0, 0.0, 0.0};
   for (int r = tid; r < NI * DD; r += NT)
   {
      const int item = r / DD;
      if (!live(item)) { continue; }
      const int yx = r - item * DD;
      const int k2 = item / NEB, el = item - k2 * NEB;
      const int base = item * ND + yx;
      const double se = a.Se[e0 + el];
      double u[D], o[D];
#pragma unroll
      for (int j = 0; j < D; j++) { u[j] = sT2[base + DD * j]; }
      row(u, o);
      double *yc = a.YE + (size_t)k2 * a.ye_stride + (size_t)(e0 + el) * ND + yx;
      double part = 0.0;
#pragma unroll
      for (int i = 0; i < D; i++)
      {
         const double v = o[i] * se;
         yc[DD * i] = v;
         part = fma(sIn[base + DD * i], v, part);
      }
      dot[0] += (k2 == 0) ? part : 0.0;
      dot[1] += (k2 == 1) ? part : 0.0;
      dot[2] += (k2 == 2) ? part : 0.0;
   }
   double bp[kVC];
   block_sum3(dot[0], dot[1], dot[2], red, bp);
   double total[kVC];
   if (grid_sum3_last_block(bp, a.partials, a.stride, a.ticket, red, total))
   {
      if (tid == 0)
      {
         VcgScalars *s = a.s;
         for (int k = 0; k < kVC; k++)
         {
            if (!todo[k]) { continue; }
            s->den[k] = total[k];
            if (total[k] == 0.0 && !a.multi) { s->done[k] = 1; } // breakdown, as upstream
         }
         s->first = 0;
      }
   }
}

// ---- host side -----------------------------------------------------------------------
int vcg_ncu(lgh_ctx *c)
{
   if (c->ncu <= 0) // (per context: contexts of one process may sit on different devices)
   {
      hipDeviceProp_t prop;
      c->ncu = (hipGetDeviceProperties(&prop, c->device) == hipSuccess) ? prop.multiProcessorCount : 256;
   }
   return c->ncu;
}

// Persistent forms: one resident wave of workgroups of `kernel` (the occupancy query is cached per context), at most
// one workgroup per batch
template <typename K> static int vcg_resident_grid(lgh_ctx *c, K kernel, const int block, const int nbatch)
{
   if (c->vcg_grid <= 0)
   {
      int per_cu = 0;
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, block, 0) != hipSuccess || per_cu <= 0) { per_cu = 2; }
      c->vcg_grid = per_cu * vcg_ncu(c);
   }
   return std::min(nbatch, c->vcg_grid);
}

template <int D, int Q> static void launch_vcg_plane(lgh_ctx *c, const VcgArgs &a)
{
   // 160 KB of LDS per CU: with the staged quadrature data one element less per
   // workgroup keeps two workgroups resident for Q = 6
   constexpr int NEB0 = (256 / (kVC * Q)) > 0 ? (256 / (kVC * Q)) : 1;
   constexpr int NEB = (Q == 6) ? NEB0 - 1 : NEB0;
   const int nbatch = ceil_div(c->NE, NEB);
   const int grid = vcg_resident_grid(c, vcg_apply_plane<D, Q, NEB, true>, kVC * Q * NEB, nbatch);
   if (c->b_h1_sym) { hipLaunchKernelGGL((vcg_apply_plane<D, Q, NEB, true>), dim3(grid), dim3(kVC * Q * NEB), 0, c->stream, a, nbatch); }
   else { hipLaunchKernelGGL((vcg_apply_plane<D, Q, NEB, false>), dim3(grid), dim3(kVC * Q * NEB), 0, c->stream, a, nbatch); }
}

template <int D, int Q, int HY, int NEB> static void launch_vcg_plane_ho(lgh_ctx *c, const VcgArgs &a)
{
   if (a.w1) { hipLaunchKernelGGL((vcg_apply_plane_ho<D, Q, HY, NEB, true>), dim3(ceil_div(c->NE, NEB)), dim3(kVC * Q * HY * NEB), 0, c->stream, a); }
   else { hipLaunchKernelGGL((vcg_apply_plane_ho<D, Q, HY, NEB, false>), dim3(ceil_div(c->NE, NEB)), dim3(kVC * Q * HY * NEB), 0, c->stream, a); }
}

template <int D, int Q> static void launch_vcg_apply(lgh_ctx *c, const VcgArgs &a)
{
   constexpr int NEB = zones_per_wg(Q);
   const int nbatch = ceil_div(c->NE, NEB);
   const int grid = vcg_resident_grid(c, vcg_apply_3d<D, Q, NEB>, Q * Q * NEB, nbatch);
   hipLaunchKernelGGL((vcg_apply_3d<D, Q, NEB>), dim3(grid), dim3(Q * Q * NEB), 0, c->stream, a, nbatch);
}

template <int D, int NEB> static void launch_vcg_kron(lgh_ctx *c, const VcgArgs &a) { hipLaunchKernelGGL((vcg_apply_kron<D, NEB>), dim3(ceil_div(c->NE, NEB)), dim3(256), 0, c->stream, a); }

bool vcg_available(const lgh_ctx *c)
{
   return c->dim == 3 && order_supported(c->kid);
}

// f(IC<D>, IC<Q>) for the order of a context that has the lockstep solve (vcg_available)
template <class F> static VcgK1 visit_k1(const lgh_ctx *c, F &&f)
{
   return order_row(c->kid, [&](auto Dc, auto Qc, auto) { return f(Dc, Qc); }, [] { return VcgK1{kK1None, nullptr}; });
}

// The form of K1 and its launcher.  LGH_VCG_VARIANT (sw.vcg_variant): 0 = (qx,qy)-column K1, otherwise the plane-per-thread
// K1; 4 / 5 ask for the slab / Kronecker form where they exist; < 0: the defaults below.
VcgK1 vcg_resolve_k1(lgh_ctx *c)
{
   if (!vcg_available(c)) { return {kK1None, nullptr}; }
   const int v = c->sw.vcg_variant;
   // Slab form (all in registers, lgh_vcg_slab.hip).  Default at Q3Q2 from kSlabMinElements zones per rank: 40.6 vs 48.5 us
   // per launch at 32^3 zones, 316 vs 383 at 64^3 (profiles/README.md); smaller meshes do not fill its one workgroup per CU.
   if (c->kid == 0x346 && (v == 4 || (v < 0 && c->NE >= kSlabMinElements)) && vcg_slab_available(c)) { return {kK1Slab, launch_vcg_slab}; }
   // default at D1D >= 5 when the mass data is compact on a tensor-product rule: the Kronecker form (vcg_apply_kron;
   // config 5: 438 against 585 us).  At Q3Q2 the plane form stays the default below the slab threshold (32^3 zones:
   // plane 49.9, generic Kronecker 55.3 us - its LDS stages and one-node gathers cost more than the FMAs it saves,
   // profiles/r4_k1_forms.txt); LGH_VCG_VARIANT=5 selects it at any order (tests)
   if (((v < 0 && c->D1D >= 5) || v == 5) && c->M1h && c->w1d)
   {
      const double *Dq, *Se;
      int dqs = 1;
      if (mass_data(c, &Dq, &dqs, &Se) == LGH_OK && dqs == 0)
      {
         // (zones per workgroup at D = 5, 6, round 6: three / two - every thread at most one row of a stage and five workgroups
         //  in a CU's LDS - instead of eight / four (two workgroups per CU): 433 -> 345 us per launch at config 5, Q4Q3 steps
         //  - 2 %, profiles/r6_kron_neb.txt; LGH_KRON_NEB=0: eight / four)
         const bool kron_small = c->sw.kron_neb != 0;
         return visit_k1(c, [&](auto Dc, auto) -> VcgK1 {
            constexpr int D = Dc, NEB = 256 >> D, SMALL = (D == 5) ? 3 : (D == 6) ? 2 : NEB; // zones per workgroup: 64, 32, 16, 8 or 3, 4 or 2
            return {kK1Kron, kron_small ? launch_vcg_kron<D, SMALL> : launch_vcg_kron<D, NEB>};
         });
      }
   }
   if (v == 0 || (c->D1D >= 5 && !c->b_h1_sym)) // (the plane form for D1D >= 5 uses half a table)
   {
      return visit_k1(c, [](auto Dc, auto Qc) -> VcgK1 {
         constexpr int D = Dc, Q = Qc;
         return {kK1Column, launch_vcg_apply<D, Q>};
      });
   }
   return visit_k1(c, [&](auto Dc, auto Qc) -> VcgK1 {
      constexpr int D = Dc, Q = Qc;
      // LGH_VCG_VARIANT=1: the two-lanes-per-plane split at Q1D = 8 as well (A/B, tests)
      if constexpr (D == 5) { return {kK1Plane, v == 1 ? launch_vcg_plane_ho<D, Q, 2, 5> : launch_vcg_plane_ho<D, Q, 1, 5>}; }
      else if constexpr (D == 6) { return {kK1Plane, launch_vcg_plane_ho<D, Q, 2, 4>}; }
      else { return {kK1Plane, launch_vcg_plane<D, Q>}; }
   });
}
int vcg_k1_form(lgh_ctx *c) { return vcg_resolve_k1(c).form; }

// one launch of K1 in the form the plan names (a.iter, a.partials, a.ticket set by the caller)
void vcg_launch_k1(lgh_ctx *c, const VcgPlan &plan, const VcgArgs &a) { plan.k1.launch(c, a); }

} // namespace lgh
