// ORACLE — TEST INFRASTRUCTURE ONLY.
//
// CPU restatement of the Laghos partial-assembly hot path.  Only tests/,
// __graft_entry__.smoke() and bench.py's cpu_baseline leg may load this
// library; the product (laghos_amd/) never links, imports or calls it.
//
// What is restated, and from where (all paths relative to /root/reference):
//   ForceMult{2D,3D}            laghos_assembly.cpp:145-294, :296-514
//   ForceMultTranspose{2D,3D}   laghos_assembly.cpp:567-713, :715-924
//   ForcePAOperator::Mult/T     laghos_assembly.cpp:557-565, :965-973
//   MassPAOperator              laghos_assembly.cpp:80-121  (PA mass apply itself
//                               is upstream MFEM MassIntegrator::AddMultPA; the
//                               math is cross-checked with amr/laghos_assembly.cpp:878-963)
//   QUpdateBody / QKernel       laghos_solver.cpp:1042-1168, :1263-1352
//   QUpdate::UpdateQuadratureData laghos_solver.cpp:1354-1411 (E-restriction +
//                               QuadratureInterpolator::Derivatives/Values are upstream)
//   Rho0DetJ0Vol                laghos_solver.cpp:1170-1261
//   CGSolver / Jacobi           configured laghos_solver.cpp:264-284 (algorithm
//                               upstream MFEM linalg/solvers.cpp, restated)
//   ComputeVolumeIntegral etc.  laghos_solver.cpp:565-697
//
// Upstream MFEM (branch master, unpinned: makefile:307-314) is not available in
// this image, so this oracle is pinned end-to-end against the reference's own
// golden values: the `--checks` table (laghos.cpp:1441-1463, rel 1e-13 there)
// and the README / `make tests` runs (README.md:225-235, makefile:271-278).
// See tests/test_oracle_golden.py.  The reference itself is unbuildable here
// (needs mfem.hpp + hypre + MPI); no stand-in headers are written.
//
// Loop structure follows the host expansion of the reference's MFEM_FORALL
// kernels (MFEM_FOREACH_THREAD -> plain for), so operation order inside an
// element matches the reference CPU `-pa` path.  Elements are independent and
// are distributed over OpenMP threads (one thread plays one MPI rank's loop).

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>
#ifdef _OPENMP
#include <omp.h>
#endif

#include "smallmat.hpp"

namespace
{

// ---------------------------------------------------------------------------
// Force kernels.  Tables: B_l2 (Q1D x L1D, q fastest), Bt/Gt of H1 (D1D x Q1D,
// d fastest), B/G of H1 (Q1D x D1D, q fastest), Bt_l2 (L1D x Q1D).
// sJit(q, e, gd, c) = stressJinvT[q + NQ*(e + NE*(gd + DIM*c))].
// ---------------------------------------------------------------------------

// laghos_assembly.cpp:145-294
template <int D1D, int Q1D, int L1D>
void ForceMult2D(const int NE, const double *b_, const double *bt_, const double *gt_,
                 const double *sJit_, const double *x, double *y)
{
   constexpr int DIM = 2, NQ = Q1D * Q1D;
   const double eps1 = std::numeric_limits<double>::epsilon();
   const double eps2 = eps1 * eps1;
#pragma omp parallel for schedule(static)
   for (int e = 0; e < NE; e++)
   {
      double B[Q1D][L1D], Bt[D1D][Q1D], Gt[D1D][Q1D];
      double E[L1D][L1D], LQ0[D1D][Q1D], LQ1[D1D][Q1D];
      double QQ[Q1D][Q1D], QQ0[Q1D][Q1D], QQ1[Q1D][Q1D];
      for (int q = 0; q < Q1D; q++)
      {
         for (int l = 0; l < L1D; l++) { B[q][l] = b_[q + Q1D * l]; }
         for (int d = 0; d < D1D; d++)
         {
            Bt[d][q] = bt_[d + D1D * q];
            Gt[d][q] = gt_[d + D1D * q];
         }
      }
      for (int lx = 0; lx < L1D; lx++)
         for (int ly = 0; ly < L1D; ly++) { E[lx][ly] = x[lx + L1D * (ly + L1D * e)]; }
      for (int ly = 0; ly < L1D; ly++)
         for (int qx = 0; qx < Q1D; qx++)
         {
            double u = 0.0;
            for (int lx = 0; lx < L1D; ++lx) { u += B[qx][lx] * E[lx][ly]; }
            LQ0[ly][qx] = u;
         }
      for (int qy = 0; qy < Q1D; qy++)
         for (int qx = 0; qx < Q1D; qx++)
         {
            double u = 0.0;
            for (int ly = 0; ly < L1D; ++ly) { u += B[qy][ly] * LQ0[ly][qx]; }
            QQ[qy][qx] = u;
         }
      for (int c = 0; c < DIM; ++c)
      {
         for (int qy = 0; qy < Q1D; qy++)
            for (int qx = 0; qx < Q1D; qx++)
            {
               const int q = qx + Q1D * qy;
               const double s0 = sJit_[q + NQ * (e + (size_t)NE * (0 + DIM * c))];
               const double s1 = sJit_[q + NQ * (e + (size_t)NE * (1 + DIM * c))];
               QQ0[qy][qx] = QQ[qy][qx] * s0;
               QQ1[qy][qx] = QQ[qy][qx] * s1;
            }
         for (int qy = 0; qy < Q1D; qy++)
            for (int dx = 0; dx < D1D; dx++)
            {
               double u = 0.0, v = 0.0;
               for (int qx = 0; qx < Q1D; ++qx)
               {
                  u += Gt[dx][qx] * QQ0[qy][qx];
                  v += Bt[dx][qx] * QQ1[qy][qx];
               }
               LQ0[dx][qy] = u;
               LQ1[dx][qy] = v;
            }
         for (int dy = 0; dy < D1D; dy++)
            for (int dx = 0; dx < D1D; dx++)
            {
               double u = 0.0, v = 0.0;
               for (int qy = 0; qy < Q1D; ++qy)
               {
                  u += LQ0[dx][qy] * Bt[dy][qy];
                  v += LQ1[dx][qy] * Gt[dy][qy];
               }
               y[dx + D1D * (dy + D1D * (c + DIM * (size_t)e))] = u + v;
            }
      }
      for (int c = 0; c < DIM; ++c)
         for (int dy = 0; dy < D1D; dy++)
            for (int dx = 0; dx < D1D; dx++)
            {
               double &v = y[dx + D1D * (dy + D1D * (c + DIM * (size_t)e))];
               if (std::fabs(v) < eps2) { v = 0.0; }
            }
   }
}

// laghos_assembly.cpp:296-514
template <int D1D, int Q1D, int L1D>
void ForceMult3D(const int NE, const double *b_, const double *bt_, const double *gt_,
                 const double *sJit_, const double *x, double *y)
{
   constexpr int DIM = 3, NQ = Q1D * Q1D * Q1D;
   const double eps1 = std::numeric_limits<double>::epsilon();
   const double eps2 = eps1 * eps1;
#pragma omp parallel for schedule(static)
   for (int e = 0; e < NE; e++)
   {
      double B[Q1D][L1D], Bt[D1D][Q1D], Gt[D1D][Q1D];
      double E[L1D][L1D][L1D];
      double sm0[3][Q1D * Q1D * Q1D], sm1[3][Q1D * Q1D * Q1D];
      double(*MMQ0)[D1D][Q1D] = (double(*)[D1D][Q1D])(sm0 + 0);
      double(*MMQ1)[D1D][Q1D] = (double(*)[D1D][Q1D])(sm0 + 1);
      double(*MMQ2)[D1D][Q1D] = (double(*)[D1D][Q1D])(sm0 + 2);
      double(*MQQ0)[Q1D][Q1D] = (double(*)[Q1D][Q1D])(sm1 + 0);
      double(*MQQ1)[Q1D][Q1D] = (double(*)[Q1D][Q1D])(sm1 + 1);
      double(*MQQ2)[Q1D][Q1D] = (double(*)[Q1D][Q1D])(sm1 + 2);
      double QQQ[Q1D][Q1D][Q1D];
      double(*QQQ0)[Q1D][Q1D] = (double(*)[Q1D][Q1D])(sm0 + 0);
      double(*QQQ1)[Q1D][Q1D] = (double(*)[Q1D][Q1D])(sm0 + 1);
      double(*QQQ2)[Q1D][Q1D] = (double(*)[Q1D][Q1D])(sm0 + 2);
      for (int q = 0; q < Q1D; q++)
      {
         for (int l = 0; l < L1D; l++) { B[q][l] = b_[q + Q1D * l]; }
         for (int d = 0; d < D1D; d++)
         {
            Bt[d][q] = bt_[d + D1D * q];
            Gt[d][q] = gt_[d + D1D * q];
         }
      }
      for (int lx = 0; lx < L1D; lx++)
         for (int ly = 0; ly < L1D; ly++)
            for (int lz = 0; lz < L1D; lz++)
            {
               E[lx][ly][lz] = x[lx + L1D * (ly + L1D * (lz + L1D * (size_t)e))];
            }
      for (int lz = 0; lz < L1D; lz++)
         for (int ly = 0; ly < L1D; ly++)
            for (int qx = 0; qx < Q1D; qx++)
            {
               double u = 0.0;
               for (int lx = 0; lx < L1D; ++lx) { u += B[qx][lx] * E[lx][ly][lz]; }
               MMQ0[lz][ly][qx] = u;
            }
      for (int lz = 0; lz < L1D; lz++)
         for (int qy = 0; qy < Q1D; qy++)
            for (int qx = 0; qx < Q1D; qx++)
            {
               double u = 0.0;
               for (int ly = 0; ly < L1D; ++ly) { u += B[qy][ly] * MMQ0[lz][ly][qx]; }
               MQQ0[lz][qy][qx] = u;
            }
      for (int qz = 0; qz < Q1D; qz++)
         for (int qy = 0; qy < Q1D; qy++)
            for (int qx = 0; qx < Q1D; qx++)
            {
               double u = 0.0;
               for (int lz = 0; lz < L1D; ++lz) { u += B[qz][lz] * MQQ0[lz][qy][qx]; }
               QQQ[qz][qy][qx] = u;
            }
      for (int c = 0; c < 3; ++c)
      {
         for (int qz = 0; qz < Q1D; qz++)
            for (int qy = 0; qy < Q1D; qy++)
               for (int qx = 0; qx < Q1D; qx++)
               {
                  const int q = qx + Q1D * (qy + Q1D * qz);
                  const double s0 = sJit_[q + NQ * (e + (size_t)NE * (0 + DIM * c))];
                  const double s1 = sJit_[q + NQ * (e + (size_t)NE * (1 + DIM * c))];
                  const double s2 = sJit_[q + NQ * (e + (size_t)NE * (2 + DIM * c))];
                  QQQ0[qz][qy][qx] = QQQ[qz][qy][qx] * s0;
                  QQQ1[qz][qy][qx] = QQQ[qz][qy][qx] * s1;
                  QQQ2[qz][qy][qx] = QQQ[qz][qy][qx] * s2;
               }
         for (int qz = 0; qz < Q1D; qz++)
            for (int qy = 0; qy < Q1D; qy++)
               for (int hx = 0; hx < D1D; hx++)
               {
                  double u = 0.0, v = 0.0, w = 0.0;
                  for (int qx = 0; qx < Q1D; ++qx)
                  {
                     u += Gt[hx][qx] * QQQ0[qz][qy][qx];
                     v += Bt[hx][qx] * QQQ1[qz][qy][qx];
                     w += Bt[hx][qx] * QQQ2[qz][qy][qx];
                  }
                  MQQ0[hx][qy][qz] = u;
                  MQQ1[hx][qy][qz] = v;
                  MQQ2[hx][qy][qz] = w;
               }
         for (int qz = 0; qz < Q1D; qz++)
            for (int hy = 0; hy < D1D; hy++)
               for (int hx = 0; hx < D1D; hx++)
               {
                  double u = 0.0, v = 0.0, w = 0.0;
                  for (int qy = 0; qy < Q1D; ++qy)
                  {
                     u += MQQ0[hx][qy][qz] * Bt[hy][qy];
                     v += MQQ1[hx][qy][qz] * Gt[hy][qy];
                     w += MQQ2[hx][qy][qz] * Bt[hy][qy];
                  }
                  MMQ0[hx][hy][qz] = u;
                  MMQ1[hx][hy][qz] = v;
                  MMQ2[hx][hy][qz] = w;
               }
         for (int hz = 0; hz < D1D; hz++)
            for (int hy = 0; hy < D1D; hy++)
               for (int hx = 0; hx < D1D; hx++)
               {
                  double u = 0.0, v = 0.0, w = 0.0;
                  for (int qz = 0; qz < Q1D; ++qz)
                  {
                     u += MMQ0[hx][hy][qz] * Bt[hz][qz];
                     v += MMQ1[hx][hy][qz] * Bt[hz][qz];
                     w += MMQ2[hx][hy][qz] * Gt[hz][qz];
                  }
                  y[hx + D1D * (hy + D1D * (hz + D1D * (c + DIM * (size_t)e)))] = u + v + w;
               }
      }
      for (int i = 0; i < D1D * D1D * D1D * DIM; i++)
      {
         double &v = y[i + (size_t)D1D * D1D * D1D * DIM * e];
         if (std::fabs(v) < eps2) { v = 0.0; }
      }
   }
}

// laghos_assembly.cpp:567-713
template <int D1D, int Q1D, int L1D>
void ForceMultTranspose2D(const int NE, const double *bt_, const double *b_, const double *g_,
                          const double *sJit_, const double *x, double *y)
{
   constexpr int DIM = 2, NQ = Q1D * Q1D;
#pragma omp parallel for schedule(static)
   for (int e = 0; e < NE; e++)
   {
      double Bt[L1D][Q1D], B[Q1D][D1D], G[Q1D][D1D];
      double V[D1D][D1D], DQ0[D1D][Q1D], DQ1[D1D][Q1D];
      double QQ[Q1D][Q1D], QQ0[Q1D][Q1D], QQ1[Q1D][Q1D], QL[Q1D][L1D];
      for (int q = 0; q < Q1D; q++)
      {
         for (int h = 0; h < D1D; h++)
         {
            B[q][h] = b_[q + Q1D * h];
            G[q][h] = g_[q + Q1D * h];
         }
         for (int l = 0; l < L1D; l++) { Bt[l][q] = bt_[l + L1D * q]; }
      }
      for (int qy = 0; qy < Q1D; qy++)
         for (int qx = 0; qx < Q1D; qx++) { QQ[qy][qx] = 0.0; }
      for (int c = 0; c < DIM; ++c)
      {
         for (int dx = 0; dx < D1D; dx++)
            for (int dy = 0; dy < D1D; dy++)
            {
               V[dx][dy] = x[dx + D1D * (dy + D1D * (c + DIM * (size_t)e))];
            }
         for (int dy = 0; dy < D1D; dy++)
            for (int qx = 0; qx < Q1D; qx++)
            {
               double u = 0.0, v = 0.0;
               for (int dx = 0; dx < D1D; ++dx)
               {
                  const double input = V[dx][dy];
                  u += B[qx][dx] * input;
                  v += G[qx][dx] * input;
               }
               DQ0[dy][qx] = u;
               DQ1[dy][qx] = v;
            }
         for (int qy = 0; qy < Q1D; qy++)
            for (int qx = 0; qx < Q1D; qx++)
            {
               double u = 0.0, v = 0.0;
               for (int dy = 0; dy < D1D; ++dy)
               {
                  u += DQ1[dy][qx] * B[qy][dy];
                  v += DQ0[dy][qx] * G[qy][dy];
               }
               QQ0[qy][qx] = u;
               QQ1[qy][qx] = v;
            }
         for (int qy = 0; qy < Q1D; qy++)
            for (int qx = 0; qx < Q1D; qx++)
            {
               const int q = qx + Q1D * qy;
               const double esx = QQ0[qy][qx] * sJit_[q + NQ * (e + (size_t)NE * (0 + DIM * c))];
               const double esy = QQ1[qy][qx] * sJit_[q + NQ * (e + (size_t)NE * (1 + DIM * c))];
               QQ[qy][qx] += esx + esy;
            }
      }
      for (int qy = 0; qy < Q1D; qy++)
         for (int lx = 0; lx < L1D; lx++)
         {
            double u = 0.0;
            for (int qx = 0; qx < Q1D; ++qx) { u += QQ[qy][qx] * Bt[lx][qx]; }
            QL[qy][lx] = u;
         }
      for (int ly = 0; ly < L1D; ly++)
         for (int lx = 0; lx < L1D; lx++)
         {
            double u = 0.0;
            for (int qy = 0; qy < Q1D; ++qy) { u += QL[qy][lx] * Bt[ly][qy]; }
            y[lx + L1D * (ly + L1D * (size_t)e)] = u;
         }
   }
}

// laghos_assembly.cpp:715-924
template <int D1D, int Q1D, int L1D>
void ForceMultTranspose3D(const int NE, const double *bt_, const double *b_, const double *g_,
                          const double *sJit_, const double *v_, double *e_)
{
   constexpr int DIM = 3, NQ = Q1D * Q1D * Q1D;
#pragma omp parallel for schedule(static)
   for (int e = 0; e < NE; e++)
   {
      double Bt[L1D][Q1D], B[Q1D][D1D], G[Q1D][D1D];
      double sm0[3][Q1D * Q1D * Q1D], sm1[3][Q1D * Q1D * Q1D];
      double(*V)[D1D][D1D] = (double(*)[D1D][D1D])(sm0 + 0);
      double(*MMQ0)[D1D][Q1D] = (double(*)[D1D][Q1D])(sm0 + 1);
      double(*MMQ1)[D1D][Q1D] = (double(*)[D1D][Q1D])(sm0 + 2);
      double(*MQQ0)[Q1D][Q1D] = (double(*)[Q1D][Q1D])(sm1 + 0);
      double(*MQQ1)[Q1D][Q1D] = (double(*)[Q1D][Q1D])(sm1 + 1);
      double(*MQQ2)[Q1D][Q1D] = (double(*)[Q1D][Q1D])(sm1 + 2);
      double(*QQQ0)[Q1D][Q1D] = (double(*)[Q1D][Q1D])(sm0 + 0);
      double(*QQQ1)[Q1D][Q1D] = (double(*)[Q1D][Q1D])(sm0 + 1);
      double(*QQQ2)[Q1D][Q1D] = (double(*)[Q1D][Q1D])(sm0 + 2);
      double QQQ[Q1D][Q1D][Q1D];
      // The reference reuses sm1 (MQQ0 as [Q][Q][L], sm0+1 as MMQ0 [Q][L][L]) in
      // the final L2 test stage; separate scratch here is value-identical.
      double T1[Q1D][Q1D][L1D], T2[Q1D][L1D][L1D];
      for (int q = 0; q < Q1D; q++)
      {
         for (int h = 0; h < D1D; h++)
         {
            B[q][h] = b_[q + Q1D * h];
            G[q][h] = g_[q + Q1D * h];
         }
         for (int l = 0; l < L1D; l++) { Bt[l][q] = bt_[l + L1D * q]; }
      }
      for (int qz = 0; qz < Q1D; qz++)
         for (int qy = 0; qy < Q1D; qy++)
            for (int qx = 0; qx < Q1D; qx++) { QQQ[qz][qy][qx] = 0.0; }
      for (int c = 0; c < DIM; ++c)
      {
         for (int dx = 0; dx < D1D; dx++)
            for (int dy = 0; dy < D1D; dy++)
               for (int dz = 0; dz < D1D; dz++)
               {
                  V[dx][dy][dz] = v_[dx + D1D * (dy + D1D * (dz + D1D * (c + DIM * (size_t)e)))];
               }
         for (int dz = 0; dz < D1D; dz++)
            for (int dy = 0; dy < D1D; dy++)
               for (int qx = 0; qx < Q1D; qx++)
               {
                  double u = 0.0, v = 0.0;
                  for (int dx = 0; dx < D1D; ++dx)
                  {
                     const double input = V[dx][dy][dz];
                     u += G[qx][dx] * input;
                     v += B[qx][dx] * input;
                  }
                  MMQ0[dz][dy][qx] = u;
                  MMQ1[dz][dy][qx] = v;
               }
         for (int dz = 0; dz < D1D; dz++)
            for (int qy = 0; qy < Q1D; qy++)
               for (int qx = 0; qx < Q1D; qx++)
               {
                  double u = 0.0, v = 0.0, w = 0.0;
                  for (int dy = 0; dy < D1D; ++dy)
                  {
                     u += MMQ0[dz][dy][qx] * B[qy][dy];
                     v += MMQ1[dz][dy][qx] * G[qy][dy];
                     w += MMQ1[dz][dy][qx] * B[qy][dy];
                  }
                  MQQ0[dz][qy][qx] = u;
                  MQQ1[dz][qy][qx] = v;
                  MQQ2[dz][qy][qx] = w;
               }
         for (int qz = 0; qz < Q1D; qz++)
            for (int qy = 0; qy < Q1D; qy++)
               for (int qx = 0; qx < Q1D; qx++)
               {
                  double u = 0.0, v = 0.0, w = 0.0;
                  for (int dz = 0; dz < D1D; ++dz)
                  {
                     u += MQQ0[dz][qy][qx] * B[qz][dz];
                     v += MQQ1[dz][qy][qx] * B[qz][dz];
                     w += MQQ2[dz][qy][qx] * G[qz][dz];
                  }
                  QQQ0[qz][qy][qx] = u;
                  QQQ1[qz][qy][qx] = v;
                  QQQ2[qz][qy][qx] = w;
               }
         for (int qz = 0; qz < Q1D; qz++)
            for (int qy = 0; qy < Q1D; qy++)
               for (int qx = 0; qx < Q1D; qx++)
               {
                  const int q = qx + Q1D * (qy + Q1D * qz);
                  const double esx = QQQ0[qz][qy][qx] * sJit_[q + NQ * (e + (size_t)NE * (0 + DIM * c))];
                  const double esy = QQQ1[qz][qy][qx] * sJit_[q + NQ * (e + (size_t)NE * (1 + DIM * c))];
                  const double esz = QQQ2[qz][qy][qx] * sJit_[q + NQ * (e + (size_t)NE * (2 + DIM * c))];
                  QQQ[qz][qy][qx] += esx + esy + esz;
               }
      }
      for (int qz = 0; qz < Q1D; qz++)
         for (int qy = 0; qy < Q1D; qy++)
            for (int lx = 0; lx < L1D; lx++)
            {
               double u = 0.0;
               for (int qx = 0; qx < Q1D; ++qx) { u += QQQ[qz][qy][qx] * Bt[lx][qx]; }
               T1[qz][qy][lx] = u;
            }
      for (int qz = 0; qz < Q1D; qz++)
         for (int ly = 0; ly < L1D; ly++)
            for (int lx = 0; lx < L1D; lx++)
            {
               double u = 0.0;
               for (int qy = 0; qy < Q1D; ++qy) { u += T1[qz][qy][lx] * Bt[ly][qy]; }
               T2[qz][ly][lx] = u;
            }
      for (int lz = 0; lz < L1D; lz++)
         for (int ly = 0; ly < L1D; ly++)
            for (int lx = 0; lx < L1D; lx++)
            {
               double u = 0.0;
               for (int qz = 0; qz < Q1D; ++qz) { u += T2[qz][ly][lx] * Bt[lz][qz]; }
               e_[lx + L1D * (ly + L1D * (lz + L1D * (size_t)e))] = u;
            }
   }
}

// ---------------------------------------------------------------------------
// PA mass apply y_e = B^T diag(D_e) B x_e (upstream MassIntegrator::AddMultPA;
// contraction order x, y, z then back as in MFEM's PAMassApply; the same math
// is written out in amr/laghos_assembly.cpp:878-963).  B is (Q1D x N1D), q
// fastest.  Works for the scalar H1 space (N1D=D1D) and for L2 (N1D=L1D).
// ---------------------------------------------------------------------------
template <int DIM, int N1D, int Q1D>
void MassApplyE(const int NE, const double *b_, const double *D, const double *x, double *y)
{
   constexpr int ND = (DIM == 2) ? N1D * N1D : N1D * N1D * N1D;
   constexpr int NQ = (DIM == 2) ? Q1D * Q1D : Q1D * Q1D * Q1D;
#pragma omp parallel for schedule(static)
   for (int e = 0; e < NE; e++)
   {
      double B[Q1D][N1D];
      for (int q = 0; q < Q1D; q++)
         for (int d = 0; d < N1D; d++) { B[q][d] = b_[q + Q1D * d]; }
      const double *X = x + (size_t)ND * e;
      const double *De = D + (size_t)NQ * e;
      double *Y = y + (size_t)ND * e;
      if (DIM == 2)
      {
         double DQ[N1D][Q1D], QQ[Q1D][Q1D];
         for (int dy = 0; dy < N1D; dy++)
            for (int qx = 0; qx < Q1D; qx++)
            {
               double u = 0.0;
               for (int dx = 0; dx < N1D; dx++) { u += B[qx][dx] * X[dx + N1D * dy]; }
               DQ[dy][qx] = u;
            }
         for (int qy = 0; qy < Q1D; qy++)
            for (int qx = 0; qx < Q1D; qx++)
            {
               double u = 0.0;
               for (int dy = 0; dy < N1D; dy++) { u += B[qy][dy] * DQ[dy][qx]; }
               QQ[qy][qx] = u * De[qx + Q1D * qy];
            }
         for (int qy = 0; qy < Q1D; qy++)
            for (int dx = 0; dx < N1D; dx++)
            {
               double u = 0.0;
               for (int qx = 0; qx < Q1D; qx++) { u += B[qx][dx] * QQ[qy][qx]; }
               DQ[dx][qy] = u;
            }
         for (int dy = 0; dy < N1D; dy++)
            for (int dx = 0; dx < N1D; dx++)
            {
               double u = 0.0;
               for (int qy = 0; qy < Q1D; qy++) { u += B[qy][dy] * DQ[dx][qy]; }
               Y[dx + N1D * dy] = u;
            }
      }
      else
      {
         double DDQ[N1D][N1D][Q1D], DQQ[N1D][Q1D][Q1D], QQQ[Q1D][Q1D][Q1D];
         for (int dz = 0; dz < N1D; dz++)
            for (int dy = 0; dy < N1D; dy++)
               for (int qx = 0; qx < Q1D; qx++)
               {
                  double u = 0.0;
                  for (int dx = 0; dx < N1D; dx++) { u += B[qx][dx] * X[dx + N1D * (dy + N1D * dz)]; }
                  DDQ[dz][dy][qx] = u;
               }
         for (int dz = 0; dz < N1D; dz++)
            for (int qy = 0; qy < Q1D; qy++)
               for (int qx = 0; qx < Q1D; qx++)
               {
                  double u = 0.0;
                  for (int dy = 0; dy < N1D; dy++) { u += B[qy][dy] * DDQ[dz][dy][qx]; }
                  DQQ[dz][qy][qx] = u;
               }
         for (int qz = 0; qz < Q1D; qz++)
            for (int qy = 0; qy < Q1D; qy++)
               for (int qx = 0; qx < Q1D; qx++)
               {
                  double u = 0.0;
                  for (int dz = 0; dz < N1D; dz++) { u += B[qz][dz] * DQQ[dz][qy][qx]; }
                  QQQ[qz][qy][qx] = u * De[qx + Q1D * (qy + Q1D * qz)];
               }
         // back: x, then y, then z
         double QQD[Q1D][Q1D][N1D], QDD[Q1D][N1D][N1D];
         for (int qz = 0; qz < Q1D; qz++)
            for (int qy = 0; qy < Q1D; qy++)
               for (int dx = 0; dx < N1D; dx++)
               {
                  double u = 0.0;
                  for (int qx = 0; qx < Q1D; qx++) { u += B[qx][dx] * QQQ[qz][qy][qx]; }
                  QQD[qz][qy][dx] = u;
               }
         for (int qz = 0; qz < Q1D; qz++)
            for (int dy = 0; dy < N1D; dy++)
               for (int dx = 0; dx < N1D; dx++)
               {
                  double u = 0.0;
                  for (int qy = 0; qy < Q1D; qy++) { u += B[qy][dy] * QQD[qz][qy][dx]; }
                  QDD[qz][dy][dx] = u;
               }
         for (int dz = 0; dz < N1D; dz++)
            for (int dy = 0; dy < N1D; dy++)
               for (int dx = 0; dx < N1D; dx++)
               {
                  double u = 0.0;
                  for (int qz = 0; qz < Q1D; qz++) { u += B[qz][dz] * QDD[qz][dy][dx]; }
                  Y[dx + N1D * (dy + N1D * dz)] = u;
               }
      }
   }
}

// diag_e[d] = sum_q B(q,d)^2 D_e[q]   (upstream MassIntegrator::AssembleDiagonalPA)
template <int DIM, int N1D, int Q1D>
void MassDiagE(const int NE, const double *b_, const double *D, double *y)
{
   constexpr int ND = (DIM == 2) ? N1D * N1D : N1D * N1D * N1D;
   constexpr int NQ = (DIM == 2) ? Q1D * Q1D : Q1D * Q1D * Q1D;
#pragma omp parallel for schedule(static)
   for (int e = 0; e < NE; e++)
   {
      const double *De = D + (size_t)NQ * e;
      double *Y = y + (size_t)ND * e;
      if (DIM == 2)
      {
         for (int dy = 0; dy < N1D; dy++)
            for (int dx = 0; dx < N1D; dx++)
            {
               double s = 0.0;
               for (int qy = 0; qy < Q1D; qy++)
                  for (int qx = 0; qx < Q1D; qx++)
                  {
                     const double bx = b_[qx + Q1D * dx], by = b_[qy + Q1D * dy];
                     s += bx * bx * by * by * De[qx + Q1D * qy];
                  }
               Y[dx + N1D * dy] = s;
            }
      }
      else
      {
         for (int dz = 0; dz < N1D; dz++)
            for (int dy = 0; dy < N1D; dy++)
               for (int dx = 0; dx < N1D; dx++)
               {
                  double s = 0.0;
                  for (int qz = 0; qz < Q1D; qz++)
                     for (int qy = 0; qy < Q1D; qy++)
                        for (int qx = 0; qx < Q1D; qx++)
                        {
                           const double bx = b_[qx + Q1D * dx], by = b_[qy + Q1D * dy],
                                        bz = b_[qz + Q1D * dz];
                           s += bx * bx * by * by * bz * bz * De[qx + Q1D * (qy + Q1D * qz)];
                        }
                  Y[dx + N1D * (dy + N1D * dz)] = s;
               }
      }
   }
}

// ---------------------------------------------------------------------------
// QuadratureInterpolator (upstream) restated.  E-vector X(d, c, e) with d
// lexicographic; outputs byVDIM:
//   values       q_val[c + VDIM*(q + NQ*e)]
//   derivatives  q_der[c + VDIM*(dd + DIM*(q + NQ*e))] = d u_c / d xi_dd
// (laghos_solver.cpp:1366-1373; consumers :1077, :1094).
// ---------------------------------------------------------------------------
template <int DIM, int N1D, int Q1D>
void InterpE(const int NE, const int VDIM, const double *b_, const double *g_, const double *x,
             double *q_val, double *q_der)
{
   constexpr int ND = (DIM == 2) ? N1D * N1D : N1D * N1D * N1D;
   constexpr int NQ = (DIM == 2) ? Q1D * Q1D : Q1D * Q1D * Q1D;
#pragma omp parallel for schedule(static)
   for (int e = 0; e < NE; e++)
   {
      double B[Q1D][N1D], G[Q1D][N1D];
      for (int q = 0; q < Q1D; q++)
         for (int d = 0; d < N1D; d++)
         {
            B[q][d] = b_[q + Q1D * d];
            G[q][d] = g_ ? g_[q + Q1D * d] : 0.0;
         }
      for (int c = 0; c < VDIM; c++)
      {
         const double *X = x + (size_t)ND * (c + VDIM * (size_t)e);
         if (DIM == 2)
         {
            double Bx[N1D][Q1D], Gx[N1D][Q1D];
            for (int dy = 0; dy < N1D; dy++)
               for (int qx = 0; qx < Q1D; qx++)
               {
                  double u = 0.0, v = 0.0;
                  for (int dx = 0; dx < N1D; dx++)
                  {
                     const double s = X[dx + N1D * dy];
                     u += B[qx][dx] * s;
                     v += G[qx][dx] * s;
                  }
                  Bx[dy][qx] = u;
                  Gx[dy][qx] = v;
               }
            for (int qy = 0; qy < Q1D; qy++)
               for (int qx = 0; qx < Q1D; qx++)
               {
                  double val = 0.0, d0 = 0.0, d1 = 0.0;
                  for (int dy = 0; dy < N1D; dy++)
                  {
                     val += B[qy][dy] * Bx[dy][qx];
                     d0 += B[qy][dy] * Gx[dy][qx];
                     d1 += G[qy][dy] * Bx[dy][qx];
                  }
                  const size_t q = qx + Q1D * qy;
                  if (q_val) { q_val[c + VDIM * (q + NQ * (size_t)e)] = val; }
                  if (q_der)
                  {
                     q_der[c + VDIM * (0 + DIM * (q + NQ * (size_t)e))] = d0;
                     q_der[c + VDIM * (1 + DIM * (q + NQ * (size_t)e))] = d1;
                  }
               }
         }
         else
         {
            double Bx[N1D][N1D][Q1D], Gx[N1D][N1D][Q1D];
            double BB[N1D][Q1D][Q1D], GB[N1D][Q1D][Q1D], BG[N1D][Q1D][Q1D];
            for (int dz = 0; dz < N1D; dz++)
               for (int dy = 0; dy < N1D; dy++)
                  for (int qx = 0; qx < Q1D; qx++)
                  {
                     double u = 0.0, v = 0.0;
                     for (int dx = 0; dx < N1D; dx++)
                     {
                        const double s = X[dx + N1D * (dy + N1D * dz)];
                        u += B[qx][dx] * s;
                        v += G[qx][dx] * s;
                     }
                     Bx[dz][dy][qx] = u;
                     Gx[dz][dy][qx] = v;
                  }
            for (int dz = 0; dz < N1D; dz++)
               for (int qy = 0; qy < Q1D; qy++)
                  for (int qx = 0; qx < Q1D; qx++)
                  {
                     double bb = 0.0, gb = 0.0, bg = 0.0;
                     for (int dy = 0; dy < N1D; dy++)
                     {
                        bb += B[qy][dy] * Bx[dz][dy][qx];
                        gb += B[qy][dy] * Gx[dz][dy][qx];
                        bg += G[qy][dy] * Bx[dz][dy][qx];
                     }
                     BB[dz][qy][qx] = bb;
                     GB[dz][qy][qx] = gb;
                     BG[dz][qy][qx] = bg;
                  }
            for (int qz = 0; qz < Q1D; qz++)
               for (int qy = 0; qy < Q1D; qy++)
                  for (int qx = 0; qx < Q1D; qx++)
                  {
                     double val = 0.0, d0 = 0.0, d1 = 0.0, d2 = 0.0;
                     for (int dz = 0; dz < N1D; dz++)
                     {
                        val += B[qz][dz] * BB[dz][qy][qx];
                        d0 += B[qz][dz] * GB[dz][qy][qx];
                        d1 += B[qz][dz] * BG[dz][qy][qx];
                        d2 += G[qz][dz] * BB[dz][qy][qx];
                     }
                     const size_t q = qx + Q1D * (qy + Q1D * qz);
                     if (q_val) { q_val[c + VDIM * (q + NQ * (size_t)e)] = val; }
                     if (q_der)
                     {
                        q_der[c + VDIM * (0 + DIM * (q + NQ * (size_t)e))] = d0;
                        q_der[c + VDIM * (1 + DIM * (q + NQ * (size_t)e))] = d1;
                        q_der[c + VDIM * (2 + DIM * (q + NQ * (size_t)e))] = d2;
                     }
                  }
         }
      }
   }
}

// laghos_solver.cpp:799-805
inline double smooth_step_01(double x, double eps)
{
   const double y = (x + eps) / (2.0 * eps);
   if (y < 0.0) { return 0.0; }
   if (y > 1.0) { return 1.0; }
   return (3.0 - 2.0 * y) * y * y;
}
// laghos_solver.cpp:987-1040
template <int N> inline double Trace(const double *d)
{
   double t = 0.0;
   for (int i = 0; i < N; i++) { t += d[i + i * N]; }
   return t;
}
template <int N> inline double FNorm(const double *data)
{
   constexpr int hw = N * N;
   double max_norm = 0.0, entry, fnorm2;
   for (int i = 0; i < hw; i++)
   {
      entry = std::fabs(data[i]);
      if (entry > max_norm) { max_norm = entry; }
   }
   if (max_norm == 0.0) { return 0.0; }
   fnorm2 = 0.0;
   for (int i = 0; i < hw; i++)
   {
      entry = data[i] / max_norm;
      fnorm2 += entry * entry;
   }
   return max_norm * std::sqrt(fnorm2);
}

// laghos_solver.cpp:1042-1168 (QUpdateBody) driven as QKernel :1263-1352
template <int DIM>
void QKernel(const int NE, const int NQ, const bool use_viscosity, const bool use_vorticity,
             const double h0, const double h1order, const double cfl, const double infinity,
             const double *d_gamma, const double *d_weights, const double *d_Jacobians,
             const double *d_rho0DetJ0w, const double *d_e_quads, const double *d_grad_v_ext,
             const double *d_Jac0inv, double *d_dt_est, double *d_stressJinvT)
{
   constexpr int DIM2 = DIM * DIM;
#pragma omp parallel for schedule(static)
   for (int e = 0; e < NE; e++)
   {
      double Jinv[DIM2], stress[DIM2], sgrad_v[DIM2], eig_val_data[3], eig_vec_data[9];
      double compr_dir[DIM], Jpi[DIM2], ph_dir[DIM], stressJiT[DIM2];
      for (int q = 0; q < NQ; q++)
      {
         double min_detJ = infinity;
         const size_t eq = (size_t)e * NQ + q;
         const double gamma = d_gamma[e];
         const double weight = d_weights[q];
         const double inv_weight = 1. / weight;
         const double *J = d_Jacobians + DIM2 * eq;
         const double detJ = sm::Det<DIM>(J);
         min_detJ = std::fmin(min_detJ, detJ);
         sm::CalcInverse<DIM>(J, Jinv);
         const double R = inv_weight * d_rho0DetJ0w[eq] / detJ;
         const double E = std::fmax(0.0, d_e_quads[eq]);
         const double P = (gamma - 1.0) * R * E;
         const double S = std::sqrt(gamma * (gamma - 1.0) * E);
         for (int k = 0; k < DIM2; k++) { stress[k] = 0.0; }
         for (int d = 0; d < DIM; d++) { stress[d * DIM + d] = -P; }
         double visc_coeff = 0.0;
         if (use_viscosity)
         {
            const double *dV = d_grad_v_ext + DIM2 * eq;
            sm::Mult(DIM, DIM, DIM, dV, Jinv, sgrad_v);
            double vorticity_coeff = 1.0;
            if (use_vorticity)
            {
               const double grad_norm = FNorm<DIM>(sgrad_v);
               const double div_v = std::fabs(Trace<DIM>(sgrad_v));
               vorticity_coeff = (grad_norm > 0.0) ? div_v / grad_norm : 1.0;
            }
            sm::Symmetrize(DIM, sgrad_v);
            sm::CalcEigenvalues<DIM>(sgrad_v, eig_val_data, eig_vec_data);
            for (int k = 0; k < DIM; k++) { compr_dir[k] = eig_vec_data[k]; }
            sm::Mult(DIM, DIM, DIM, J, d_Jac0inv + eq * DIM * DIM, Jpi);
            sm::MultV(DIM, DIM, Jpi, compr_dir, ph_dir);
            const double ph_dir_nl2 = sm::Norml2(DIM, ph_dir);
            const double compr_dir_nl2 = sm::Norml2(DIM, compr_dir);
            const double H = h0 * ph_dir_nl2 / compr_dir_nl2;
            const double mu = eig_val_data[0];
            visc_coeff = 2.0 * R * H * H * std::fabs(mu);
            const double eps = 1e-12;
            visc_coeff += 0.5 * R * H * S * vorticity_coeff * (1.0 - smooth_step_01(mu - 2.0 * eps, eps));
            sm::Add(DIM, DIM, visc_coeff, stress, sgrad_v, stress);
         }
         const double sv = sm::CalcSingularvalue<DIM>(J, DIM - 1);
         const double h_min = sv / h1order;
         const double ih_min = 1. / h_min;
         const double irho_ih_min_sq = ih_min * ih_min / R;
         const double idt = S * ih_min + 2.5 * visc_coeff * irho_ih_min_sq;
         if (min_detJ < 0.0) { d_dt_est[eq] = 0.0; }
         else
         {
            if (idt > 0.0)
            {
               const double cfl_inv_dt = cfl / idt;
               d_dt_est[eq] = std::fmin(d_dt_est[eq], cfl_inv_dt);
            }
         }
         sm::MultABt(DIM, DIM, DIM, stress, Jinv, stressJiT);
         for (int k = 0; k < DIM2; k++) { stressJiT[k] *= weight * detJ; }
         for (int vd = 0; vd < DIM; vd++)
            for (int gd = 0; gd < DIM; gd++)
            {
               const size_t offset = eq + (size_t)NQ * NE * (gd + vd * DIM);
               d_stressJinvT[offset] = stressJiT[vd + gd * DIM];
            }
      }
   }
}

// ---------------------------------------------------------------------------
// Context: plays the role of LagrangianHydroOperator's owned state
// (laghos_solver.hpp:97-205): spaces (as dof maps), tables, QuadratureData,
// PA operators, CG work vectors.
// ---------------------------------------------------------------------------
struct Ctx
{
   int dim, NE, D1D, Q1D, L1D, ND, NQ, NL;
   int N;           // scalar H1 nodes (local)
   int H1V, L2V;    // vector sizes
   std::vector<int> h1map;             // NE x ND -> scalar node
   std::vector<int> t_off, t_idx;      // transpose of h1map (CSR by node, ascending e*ND+d)
   std::vector<double> B, G, Bt, Gt;   // H1: B,G (Q x D, q fastest), Bt,Gt (D x Q)
   std::vector<double> Bl, Blt;        // L2: B (Q x L), Bt (L x Q)
   std::vector<double> W;              // NQ weights
   std::vector<double> gamma;          // NE
   std::vector<int> ess[3];            // essential scalar nodes per component
   std::vector<double> owner;          // N: 1.0 if this rank owns the node (dot products)
   bool visc, vort;
   double cfl, h0;
   int order_v;
   // QuadratureData (laghos_assembly.hpp:31-62)
   std::vector<double> Jac0inv, stressJinvT, rho0DetJ0w;
   double dt_est;
   // mass PA data D = w*detJ0*rho0(x_q) (laghos_assembly.cpp:92-95), shared by H1c and L2
   std::vector<double> massD;
   std::vector<double> diagV;          // Jacobi diagonal of the scalar H1 mass
   int cur_ess;                        // component whose ess list is active (-1 none)
   // scratch
   std::vector<double> XE, YE, q_dx, q_dv, q_e, q_dt, e_vec;
   std::vector<double> cg_r, cg_z, cg_d;
   double cg_last[4] = {0, 0, 0, 0}; // lgo_cg: nom, den, alpha, betanom of the last iteration performed (lgo_cg_scalars)
   // timers (laghos_solver.hpp:39-56)
   double t_force, t_cgH1, t_cgL2, t_qdata;
   long H1iter, L2iter, quad_tstep;
   // dim == 1: the full-assembly branch (see the FA section below)
   std::vector<int> mv_off, mv_col;    // Mv: CSR by node, columns ascending
   std::vector<double> mv_val;
   std::vector<double> Fe;             // ForceIntegrator element matrices, Fe[(e*ND + i)*NL + l]
   std::vector<double> Me_inv;         // DenseMatrixInverse of Me(e), row-major NL x NL per zone
};

double now()
{
#ifdef _OPENMP
   return omp_get_wtime();
#else
   return (double)clock() / CLOCKS_PER_SEC;
#endif
}

[[noreturn]] void unknown_kernel(int id)
{
   // laghos_assembly.cpp:549-553
   std::fprintf(stderr, "Unknown kernel 0x%x\n", id);
   std::abort();
}

#define LGO_DISPATCH_2D(FN, id, ...)                                   \
   switch (id)                                                         \
   {                                                                   \
      case 0x222: FN<2, 2, 1>(__VA_ARGS__); break;                     \
      case 0x234: FN<3, 4, 2>(__VA_ARGS__); break;                     \
      case 0x246: FN<4, 6, 3>(__VA_ARGS__); break;                     \
      case 0x258: FN<5, 8, 4>(__VA_ARGS__); break;                     \
      case 0x26A: FN<6, 10, 5>(__VA_ARGS__); break;                    \
      default: unknown_kernel(id);                                     \
   }
// 0x36A (Q5/Q4 in 3D) is NOT instantiated by the reference
// (laghos_assembly.cpp:544-547); it is an extension here for BASELINE config 5.
#define LGO_DISPATCH_3D(FN, id, ...)                                   \
   switch (id)                                                         \
   {                                                                   \
      case 0x322: FN<2, 2, 1>(__VA_ARGS__); break;                     \
      case 0x334: FN<3, 4, 2>(__VA_ARGS__); break;                     \
      case 0x346: FN<4, 6, 3>(__VA_ARGS__); break;                     \
      case 0x358: FN<5, 8, 4>(__VA_ARGS__); break;                     \
      case 0x36A: FN<6, 10, 5>(__VA_ARGS__); break;                    \
      default: unknown_kernel(id);                                     \
   }

void force_mult_E(const Ctx &c, const double *sJit, const double *XE, double *YE)
{
   const int id = (c.dim << 8) | (c.D1D << 4) | c.Q1D;
   if (c.dim == 2) { LGO_DISPATCH_2D(ForceMult2D, id, c.NE, c.Bl.data(), c.Bt.data(), c.Gt.data(), sJit, XE, YE); }
   else { LGO_DISPATCH_3D(ForceMult3D, id, c.NE, c.Bl.data(), c.Bt.data(), c.Gt.data(), sJit, XE, YE); }
}
void force_mult_t_E(const Ctx &c, const double *sJit, const double *YE, double *XE)
{
   const int id = (c.dim << 8) | (c.D1D << 4) | c.Q1D;
   if (c.dim == 2) { LGO_DISPATCH_2D(ForceMultTranspose2D, id, c.NE, c.Blt.data(), c.B.data(), c.G.data(), sJit, YE, XE); }
   else { LGO_DISPATCH_3D(ForceMultTranspose3D, id, c.NE, c.Blt.data(), c.B.data(), c.G.data(), sJit, YE, XE); }
}

template <int DIM> void mass_apply_dispatch(int N1D, int Q1D, int NE, const double *b, const double *D, const double *x, double *y)
{
   const int id = (N1D << 4) | Q1D;
   switch (id)
   {
      case 0x12: MassApplyE<DIM, 1, 2>(NE, b, D, x, y); break;
      case 0x22: MassApplyE<DIM, 2, 2>(NE, b, D, x, y); break;
      case 0x24: MassApplyE<DIM, 2, 4>(NE, b, D, x, y); break;
      case 0x34: MassApplyE<DIM, 3, 4>(NE, b, D, x, y); break;
      case 0x36: MassApplyE<DIM, 3, 6>(NE, b, D, x, y); break;
      case 0x46: MassApplyE<DIM, 4, 6>(NE, b, D, x, y); break;
      case 0x48: MassApplyE<DIM, 4, 8>(NE, b, D, x, y); break;
      case 0x58: MassApplyE<DIM, 5, 8>(NE, b, D, x, y); break;
      case 0x5A: MassApplyE<DIM, 5, 10>(NE, b, D, x, y); break;
      case 0x6A: MassApplyE<DIM, 6, 10>(NE, b, D, x, y); break;
      default: unknown_kernel(id);
   }
}
template <int DIM> void mass_diag_dispatch(int N1D, int Q1D, int NE, const double *b, const double *D, double *y)
{
   const int id = (N1D << 4) | Q1D;
   switch (id)
   {
      case 0x22: MassDiagE<DIM, 2, 2>(NE, b, D, y); break;
      case 0x34: MassDiagE<DIM, 3, 4>(NE, b, D, y); break;
      case 0x46: MassDiagE<DIM, 4, 6>(NE, b, D, y); break;
      case 0x58: MassDiagE<DIM, 5, 8>(NE, b, D, y); break;
      case 0x6A: MassDiagE<DIM, 6, 10>(NE, b, D, y); break;
      default: unknown_kernel(id);
   }
}
template <int DIM> void interp_dispatch(int N1D, int Q1D, int NE, int VDIM, const double *b, const double *g, const double *x, double *qv, double *qd)
{
   const int id = (N1D << 4) | Q1D;
   switch (id)
   {
      case 0x12: InterpE<DIM, 1, 2>(NE, VDIM, b, g, x, qv, qd); break;
      case 0x22: InterpE<DIM, 2, 2>(NE, VDIM, b, g, x, qv, qd); break;
      case 0x24: InterpE<DIM, 2, 4>(NE, VDIM, b, g, x, qv, qd); break;
      case 0x34: InterpE<DIM, 3, 4>(NE, VDIM, b, g, x, qv, qd); break;
      case 0x36: InterpE<DIM, 3, 6>(NE, VDIM, b, g, x, qv, qd); break;
      case 0x46: InterpE<DIM, 4, 6>(NE, VDIM, b, g, x, qv, qd); break;
      case 0x48: InterpE<DIM, 4, 8>(NE, VDIM, b, g, x, qv, qd); break;
      case 0x58: InterpE<DIM, 5, 8>(NE, VDIM, b, g, x, qv, qd); break;
      case 0x5A: InterpE<DIM, 5, 10>(NE, VDIM, b, g, x, qv, qd); break;
      case 0x6A: InterpE<DIM, 6, 10>(NE, VDIM, b, g, x, qv, qd); break;
      default: unknown_kernel(id);
   }
}

void mass_apply_E(const Ctx &c, int space, const double *x, double *y)
{
   const int N1D = space == 0 ? c.D1D : c.L1D;
   const double *b = space == 0 ? c.B.data() : c.Bl.data();
   if (c.dim == 2) { mass_apply_dispatch<2>(N1D, c.Q1D, c.NE, b, c.massD.data(), x, y); }
   else { mass_apply_dispatch<3>(N1D, c.Q1D, c.NE, b, c.massD.data(), x, y); }
}

// ElementRestriction (upstream), lexicographic: L -> E gather, byNODES L-vector.
void h1_gather(const Ctx &c, int vdim, const double *xL, double *XE)
{
#pragma omp parallel for schedule(static)
   for (int e = 0; e < c.NE; e++)
      for (int cc = 0; cc < vdim; cc++)
         for (int d = 0; d < c.ND; d++)
         {
            XE[d + c.ND * (cc + vdim * (size_t)e)] = xL[(size_t)cc * c.N + c.h1map[(size_t)e * c.ND + d]];
         }
}
// E -> L transpose: sums element contributions in ascending element order
// (the order of MFEM's offsets/indices table).
void h1_scatter_add(const Ctx &c, int vdim, const double *YE, double *yL)
{
   // gather form over the transposed map: per node the contributions are added
   // in ascending (element, local dof) order, i.e. exactly the order of the
   // serial `for e: for d: y[map] += Y` loop, but nodes run in parallel.
#pragma omp parallel for schedule(static)
   for (int n = 0; n < c.N; n++)
      for (int cc = 0; cc < vdim; cc++)
      {
         double s = 0.0;
         for (int k = c.t_off[n]; k < c.t_off[n + 1]; k++)
         {
            const int p = c.t_idx[k], e = p / c.ND, d = p - e * c.ND;
            s += YE[d + c.ND * (cc + vdim * (size_t)e)];
         }
         yL[(size_t)cc * c.N + n] = s;
      }
}

double dot_owned(const Ctx &c, const double *a, const double *b)
{
   double s = 0.0;
#pragma omp parallel for reduction(+ : s) schedule(static)
   for (int i = 0; i < c.N; i++) { s += c.owner[i] * a[i] * b[i]; }
   return s;
}
double dot_plain(size_t n, const double *a, const double *b)
{
   double s = 0.0;
#pragma omp parallel for reduction(+ : s) schedule(static)
   for (size_t i = 0; i < n; i++) { s += a[i] * b[i]; }
   return s;
}

// ---------------------------------------------------------------------------
// dim == 1: the full-assembly (FA) branch.  The reference takes it for every
// 1D run (laghos.cpp:454-462 switches -pa to -fa there); restated from:
//   set-up           laghos_solver.cpp:203-221 (Me(e) by MassIntegrator, LU
//                    inverse by DenseMatrixInverse; Mv by VectorMassIntegrator),
//                    :231-262 (Jac0inv, rho0DetJ0w, volume, h0)
//   quadrature data  laghos_solver.cpp:816-985 (batches of 3 zones)
//   Force            ForceIntegrator, laghos_assembly.cpp:43-78, assembled
//   SolveVelocity    laghos_solver.cpp:400-439 (Force 1, Neg, FormLinearSystem,
//                    Jacobi PCG: lgo_cg with space 0)
//   SolveEnergy      laghos_solver.cpp:491-516 (Force^T v, Me_inv(e) per zone)
// Sparse products run row by row with ascending columns, as SparseMatrix::Mult.
// ---------------------------------------------------------------------------

// x at the quadrature points of zone e (1D: ND = D1D, NQ = Q1D, NL = L1D)
inline double fa_interp(const std::vector<double> &T, int Q, int q, int n, const double *xe)
{
   double s = 0.0;
   for (int d = 0; d < n; d++) { s += T[q + Q * d] * xe[d]; }
   return s;
}

// LU factorisation with partial pivoting, then the inverse column by column
// (DenseMatrixInverse::Factor + GetInverseMatrix: LUFactors).  A is n x n row-major.
void lu_inverse(int n, const double *A, double *Ainv)
{
   std::vector<double> LU(A, A + n * n);
   std::vector<int> piv(n);
   for (int i = 0; i < n; i++)
   {
      int p = i;
      double m = std::fabs(LU[i * n + i]);
      for (int j = i + 1; j < n; j++)
         if (std::fabs(LU[j * n + i]) > m) { m = std::fabs(LU[j * n + i]); p = j; }
      piv[i] = p;
      if (p != i)
         for (int k = 0; k < n; k++) { std::swap(LU[i * n + k], LU[p * n + k]); }
      const double d = 1.0 / LU[i * n + i];
      for (int j = i + 1; j < n; j++)
      {
         LU[j * n + i] *= d;
         for (int k = i + 1; k < n; k++) { LU[j * n + k] -= LU[j * n + i] * LU[i * n + k]; }
      }
   }
   std::vector<double> col(n);
   for (int c = 0; c < n; c++)
   {
      for (int i = 0; i < n; i++) { col[i] = (i == c) ? 1.0 : 0.0; }
      for (int i = 0; i < n; i++) { std::swap(col[i], col[piv[i]]); }
      for (int i = 0; i < n; i++)
         for (int k = 0; k < i; k++) { col[i] -= LU[i * n + k] * col[k]; }
      for (int i = n - 1; i >= 0; i--)
      {
         for (int k = i + 1; k < n; k++) { col[i] -= LU[i * n + k] * col[k]; }
         col[i] /= LU[i * n + i];
      }
      for (int i = 0; i < n; i++) { Ainv[i * n + c] = col[i]; }
   }
}

// laghos_solver.cpp:203-221, :231-250
double fa_setup(Ctx &c, const double *x0, const double *rho0_l2, const double *rho0_q)
{
   const int NE = c.NE, D = c.D1D, Q = c.Q1D, L = c.L1D;
   std::vector<double> Mv_e((size_t)NE * D * D, 0.0), Me(L * L);
   c.Me_inv.assign((size_t)NE * L * L, 0.0);
   double vol = 0.0;
   for (int e = 0; e < NE; e++)
   {
      double xe[16], re[16];
      for (int d = 0; d < D; d++) { xe[d] = x0[c.h1map[(size_t)e * D + d]]; }
      for (int l = 0; l < L; l++) { re[l] = rho0_l2[(size_t)e * L + l]; }
      std::fill(Me.begin(), Me.end(), 0.0);
      double *mv = Mv_e.data() + (size_t)e * D * D;
      for (int q = 0; q < Q; q++)
      {
         const size_t eq = (size_t)e * Q + q;
         const double J = fa_interp(c.G, Q, q, D, xe);
         c.Jac0inv[eq] = 1.0 / J;                                  // DenseMatrixInverse of the 1 x 1 Jacobian
         const double rho0DetJ0 = J * fa_interp(c.Bl, Q, q, L, re); // Tr.Weight() * rho_vals(q)
         c.rho0DetJ0w[eq] = rho0DetJ0 * c.W[q];
         // MassIntegrator / VectorMassIntegrator: w = Tr.Weight() * ip.weight * Q(x)
         const double w = J * c.W[q] * rho0_q[eq];
         c.massD[eq] = w;
         for (int i = 0; i < L; i++)
            for (int j = 0; j < L; j++) { Me[i * L + j] += w * c.Bl[q + Q * i] * c.Bl[q + Q * j]; }
         for (int i = 0; i < D; i++)
            for (int j = 0; j < D; j++) { mv[i * D + j] += w * c.B[q + Q * i] * c.B[q + Q * j]; }
      }
      lu_inverse(L, Me.data(), c.Me_inv.data() + (size_t)e * L * L);
      vol += xe[D - 1] - xe[0];                                    // GetElementVolume
   }
   // Mv.Assemble(): element matrices summed in ascending element order into CSR rows
   const int N = c.N;
   std::vector<std::vector<std::pair<int, double>>> rows(N);
   for (int e = 0; e < NE; e++)
      for (int i = 0; i < D; i++)
         for (int j = 0; j < D; j++)
         {
            const int r = c.h1map[(size_t)e * D + i], col = c.h1map[(size_t)e * D + j];
            const double v = Mv_e[((size_t)e * D + i) * D + j];
            auto it = std::find_if(rows[r].begin(), rows[r].end(), [&](const std::pair<int, double> &p) { return p.first == col; });
            if (it == rows[r].end()) { rows[r].push_back({col, v}); }
            else { it->second += v; }
         }
   c.mv_off.assign((size_t)N + 1, 0);
   c.mv_col.clear();
   c.mv_val.clear();
   for (int r = 0; r < N; r++)
   {
      std::sort(rows[r].begin(), rows[r].end(), [](const std::pair<int, double> &a, const std::pair<int, double> &b) { return a.first < b.first; });
      for (auto &p : rows[r]) { c.mv_col.push_back(p.first); c.mv_val.push_back(p.second); }
      c.mv_off[(size_t)r + 1] = (int)c.mv_col.size();
   }
   return vol;
}

// Jacobi diagonal: the diagonal of the assembled Mv.  (The FA solve's HypreSmoother
// reads the diagonal of the eliminated matrix, 1 on the essential rows; the residual
// is 0 there, so either gives the same iterates.)
void fa_diag(Ctx &c)
{
   for (int r = 0; r < c.N; r++)
   {
      c.diagV[r] = 0.0;
      for (int k = c.mv_off[r]; k < c.mv_off[(size_t)r + 1]; k++)
         if (c.mv_col[k] == r) { c.diagV[r] = c.mv_val[k]; }
   }
}

void fa_mv_mult(const Ctx &c, const double *x, double *y)
{
   for (int r = 0; r < c.N; r++)
   {
      double s = 0.0;
      for (int k = c.mv_off[r]; k < c.mv_off[(size_t)r + 1]; k++) { s += c.mv_val[k] * x[c.mv_col[k]]; }
      y[r] = s;
   }
}

// y_e = Me(e) x_e, Me(e) formed again from the mass data (the L2 mass operator of the tests)
void fa_me_mult(const Ctx &c, const double *x, double *y)
{
   const int NE = c.NE, Q = c.Q1D, L = c.L1D;
   for (int e = 0; e < NE; e++)
   {
      for (int i = 0; i < L; i++)
      {
         double s = 0.0;
         for (int j = 0; j < L; j++)
         {
            double m = 0.0;
            for (int q = 0; q < Q; q++) { m += c.massD[(size_t)e * Q + q] * c.Bl[q + Q * i] * c.Bl[q + Q * j]; }
            s += m * x[(size_t)e * L + j];
         }
         y[(size_t)e * L + i] = s;
      }
   }
}

void fa_me_inv_mult(const Ctx &c, const double *b, double *x)
{
   const int L = c.L1D;
   for (int e = 0; e < c.NE; e++)
   {
      const double *Mi = c.Me_inv.data() + (size_t)e * L * L;
      for (int i = 0; i < L; i++)
      {
         double s = 0.0;
         for (int j = 0; j < L; j++) { s += Mi[i * L + j] * b[(size_t)e * L + j]; }
         x[(size_t)e * L + i] = s;
      }
   }
}

// laghos_solver.cpp:816-985, then the ForceIntegrator element matrices (AssembleForceMatrix)
void fa_qupdate(Ctx &c, const double *S)
{
   const int NE = c.NE, D = c.D1D, Q = c.Q1D, L = c.L1D, N = c.N;
   const double *x = S, *v = S + N, *en = S + 2 * (size_t)N;
   const int nbatch = 3;
   std::vector<double> J((size_t)nbatch * Q), rho(J.size()), E(J.size()), dvq(J.size());
   for (int z0 = 0; z0 < NE; z0 += nbatch)
   {
      const int nz = std::min(nbatch, NE - z0);
      double min_detJ = std::numeric_limits<double>::infinity();
      for (int z = 0; z < nz; z++)
      {
         const int e = z0 + z;
         double xe[16], ve[16], ee[16];
         for (int d = 0; d < D; d++) { xe[d] = x[c.h1map[(size_t)e * D + d]]; ve[d] = v[c.h1map[(size_t)e * D + d]]; }
         for (int l = 0; l < L; l++) { ee[l] = en[(size_t)e * L + l]; }
         for (int q = 0; q < Q; q++)
         {
            const int i = z * Q + q;
            J[i] = fa_interp(c.G, Q, q, D, xe);
            dvq[i] = fa_interp(c.G, Q, q, D, ve);
            min_detJ = std::fmin(min_detJ, J[i]);
            rho[i] = c.rho0DetJ0w[(size_t)e * Q + q] / J[i] / c.W[q];
            E[i] = std::fmax(0.0, fa_interp(c.Bl, Q, q, L, ee));
         }
      }
      for (int z = 0; z < nz; z++)
      {
         const int e = z0 + z;
         const double gamma = c.gamma[e];
         for (int q = 0; q < Q; q++)
         {
            const int i = z * Q + q;
            const size_t eq = (size_t)e * Q + q;
            const double detJ = J[i], Jinv = 1.0 / J[i], r = rho[i];
            const double p = (gamma - 1.0) * r * E[i];                   // ComputeMaterialProperties
            const double sound_speed = std::sqrt(gamma * (gamma - 1.0) * E[i]);
            double stress = -p, visc_coeff = 0.0;
            if (c.visc)
            {
               const double sgrad_v = dvq[i] * Jinv;                      // GetVectorGradient; Symmetrize: itself
               const double eig_val = sgrad_v, eig_vec = 1.0;             // dim == 1
               const double Jpi = detJ * c.Jac0inv[eq];
               const double ph_dir = Jpi * eig_vec;
               const double h = c.h0 * std::fabs(ph_dir) / std::fabs(eig_vec);
               const double mu = eig_val;
               visc_coeff = 2.0 * r * h * h * std::fabs(mu);
               const double eps = 1e-12;
               visc_coeff += 0.5 * r * h * sound_speed * 1.0 * (1.0 - smooth_step_01(mu - 2.0 * eps, eps));
               stress += visc_coeff * sgrad_v;
            }
            const double h_min = std::fabs(detJ) / (double)c.order_v;     // CalcSingularvalue(0) of 1 x 1
            const double inv_dt = sound_speed / h_min + 2.5 * visc_coeff / r / h_min / h_min;
            if (min_detJ < 0.0) { c.dt_est = 0.0; }
            else if (inv_dt > 0.0) { c.dt_est = std::fmin(c.dt_est, c.cfl * (1.0 / inv_dt)); }
            double sJ = stress * Jinv;                                    // MultABt(stress, Jinv)
            sJ *= c.W[q] * detJ;
            c.stressJinvT[eq] = sJ;
         }
      }
   }
}

// ForceIntegrator::AssembleElementMatrix2 (laghos_assembly.cpp:43-78), 1D:
// elmat(i, l) += (stressJinvT * dshape(i)) * shape(l)
void fa_force_assemble(Ctx &c)
{
   const int NE = c.NE, D = c.D1D, Q = c.Q1D, L = c.L1D;
   c.Fe.assign((size_t)NE * D * L, 0.0);
   for (int e = 0; e < NE; e++)
      for (int q = 0; q < Q; q++)
      {
         const double sJ = c.stressJinvT[(size_t)e * Q + q];
         for (int i = 0; i < D; i++)
         {
            const double lf = sJ * c.G[q + Q * i];
            for (int l = 0; l < L; l++) { c.Fe[((size_t)e * D + i) * L + l] += lf * c.Bl[q + Q * l]; }
         }
      }
}

// Force.Mult: row n of the assembled matrix, columns (e, l) ascending
void fa_force_mult(const Ctx &c, const double *xl, double *y)
{
   const int D = c.D1D, L = c.L1D;
   for (int n = 0; n < c.N; n++)
   {
      double s = 0.0;
      for (int k = c.t_off[n]; k < c.t_off[n + 1]; k++)
      {
         const int p = c.t_idx[k], e = p / D, i = p - e * D;
         for (int l = 0; l < L; l++) { s += c.Fe[((size_t)e * D + i) * L + l] * xl[(size_t)e * L + l]; }
      }
      y[n] = s;
   }
}

// Force.MultTranspose: column (e, l) takes its rows in ascending node order
void fa_force_mult_t(const Ctx &c, const double *v, double *y)
{
   const int D = c.D1D, L = c.L1D;
   for (int e = 0; e < c.NE; e++)
      for (int l = 0; l < L; l++)
      {
         double s = 0.0;
         for (int i = 0; i < D; i++) { s += c.Fe[((size_t)e * D + i) * L + l] * v[c.h1map[(size_t)e * D + i]]; }
         y[(size_t)e * L + l] = s;
      }
}

} // namespace

extern "C"
{

// Optional hooks for multi-rank runs (tests drive them from Python over gloo):
// sum the shared H1 nodes across ranks in-place; all-reduce a scalar (0 sum, 1 min).
typedef void (*lgo_halo_fn)(double *vec_L, int ncomp, void *user);
typedef double (*lgo_allreduce_fn)(double v, int op, void *user);
static lgo_halo_fn g_halo = nullptr;
static lgo_allreduce_fn g_allreduce = nullptr;
static void *g_user = nullptr;
void lgo_set_comm_hooks(lgo_halo_fn h, lgo_allreduce_fn a, void *user)
{
   g_halo = h;
   g_allreduce = a;
   g_user = user;
}
static double allreduce(double v, int op) { return g_allreduce ? g_allreduce(v, op, g_user) : v; }
static void halo(double *v, int nc)
{
   if (g_halo) { g_halo(v, nc, g_user); }
}

void *lgo_create(int dim, int NE, int D1D, int Q1D, int L1D, int N, const int *h1map,
                 const double *B, const double *G, const double *Bl, const double *W,
                 const double *gamma, const int *ess_counts, const int *ess0, const int *ess1,
                 const int *ess2, const double *owner, int visc, int vort, double cfl, int order_v)
{
   Ctx *c = new Ctx;
   c->dim = dim; c->NE = NE; c->D1D = D1D; c->Q1D = Q1D; c->L1D = L1D; c->N = N;
   c->ND = dim == 1 ? D1D : dim == 2 ? D1D * D1D : D1D * D1D * D1D;
   c->NQ = dim == 1 ? Q1D : dim == 2 ? Q1D * Q1D : Q1D * Q1D * Q1D;
   c->NL = dim == 1 ? L1D : dim == 2 ? L1D * L1D : L1D * L1D * L1D;
   c->H1V = dim * N;
   c->L2V = NE * c->NL;
   c->h1map.assign(h1map, h1map + (size_t)NE * c->ND);
   {
      const size_t nmap = (size_t)NE * c->ND;
      c->t_off.assign((size_t)N + 1, 0);
      c->t_idx.resize(nmap);
      for (size_t i = 0; i < nmap; i++) { c->t_off[(size_t)h1map[i] + 1]++; }
      for (int n = 0; n < N; n++) { c->t_off[(size_t)n + 1] += c->t_off[n]; }
      std::vector<int> pos(c->t_off.begin(), c->t_off.end() - 1);
      for (size_t i = 0; i < nmap; i++) { c->t_idx[pos[h1map[i]]++] = (int)i; }
   }
   c->B.assign(B, B + Q1D * D1D);
   c->G.assign(G, G + Q1D * D1D);
   c->Bt.resize(Q1D * D1D);
   c->Gt.resize(Q1D * D1D);
   for (int q = 0; q < Q1D; q++)
      for (int d = 0; d < D1D; d++)
      {
         c->Bt[d + D1D * q] = B[q + Q1D * d];
         c->Gt[d + D1D * q] = G[q + Q1D * d];
      }
   c->Bl.assign(Bl, Bl + Q1D * L1D);
   c->Blt.resize(Q1D * L1D);
   for (int q = 0; q < Q1D; q++)
      for (int l = 0; l < L1D; l++) { c->Blt[l + L1D * q] = Bl[q + Q1D * l]; }
   c->W.assign(W, W + c->NQ);
   c->gamma.assign(gamma, gamma + NE);
   const int *ess[3] = {ess0, ess1, ess2};
   for (int k = 0; k < dim; k++) { c->ess[k].assign(ess[k], ess[k] + ess_counts[k]); }
   c->owner.assign(owner, owner + N);
   c->visc = visc; c->vort = vort; c->cfl = cfl; c->order_v = order_v;
   c->h0 = 0.0;
   const size_t nq = (size_t)NE * c->NQ;
   c->Jac0inv.assign(nq * dim * dim, 0.0);
   c->stressJinvT.assign(nq * dim * dim, 0.0);
   c->rho0DetJ0w.assign(nq, 0.0);
   c->massD.assign(nq, 0.0);
   c->diagV.assign(N, 0.0);
   c->dt_est = std::numeric_limits<double>::infinity();
   c->cur_ess = -1;
   c->XE.assign(std::max((size_t)c->L2V, (size_t)NE * c->ND * dim), 0.0);
   c->YE.assign((size_t)NE * c->ND * dim, 0.0);
   c->e_vec.assign((size_t)NE * c->ND * dim, 0.0);
   c->q_dx.assign(nq * dim * dim, 0.0);
   c->q_dv.assign(nq * dim * dim, 0.0);
   c->q_e.assign(nq, 0.0);
   c->q_dt.assign(nq, 0.0);
   c->cg_r.assign(std::max(N, c->L2V), 0.0);
   c->cg_z.assign(std::max(N, c->L2V), 0.0);
   c->cg_d.assign(std::max(N, c->L2V), 0.0);
   c->t_force = c->t_cgH1 = c->t_cgL2 = c->t_qdata = 0.0;
   c->H1iter = c->L2iter = c->quad_tstep = 0;
   return c;
}
void lgo_destroy(void *h) { delete (Ctx *)h; }

double *lgo_stressJinvT(void *h) { return ((Ctx *)h)->stressJinvT.data(); }
double *lgo_Jac0inv(void *h) { return ((Ctx *)h)->Jac0inv.data(); }
double *lgo_rho0DetJ0w(void *h) { return ((Ctx *)h)->rho0DetJ0w.data(); }
double *lgo_massD(void *h) { return ((Ctx *)h)->massD.data(); }
double *lgo_diagV(void *h) { return ((Ctx *)h)->diagV.data(); }
double *lgo_q_dx(void *h) { return ((Ctx *)h)->q_dx.data(); }
double *lgo_q_dv(void *h) { return ((Ctx *)h)->q_dv.data(); }
double *lgo_q_e(void *h) { return ((Ctx *)h)->q_e.data(); }
double lgo_get_h0(void *h) { return ((Ctx *)h)->h0; }
void lgo_set_h0(void *h, double v) { ((Ctx *)h)->h0 = v; }
double lgo_get_dt_est(void *h) { return ((Ctx *)h)->dt_est; }
void lgo_set_dt_est(void *h, double v) { ((Ctx *)h)->dt_est = v; }
void lgo_get_timers(void *h, double *t4, long *c3)
{
   Ctx *c = (Ctx *)h;
   t4[0] = c->t_cgH1; t4[1] = c->t_cgL2; t4[2] = c->t_force; t4[3] = c->t_qdata;
   c3[0] = c->H1iter; c3[1] = c->L2iter; c3[2] = c->quad_tstep;
}
void lgo_reset_timers(void *h)
{
   Ctx *c = (Ctx *)h;
   c->t_force = c->t_cgH1 = c->t_cgL2 = c->t_qdata = 0.0;
   c->H1iter = c->L2iter = c->quad_tstep = 0;
}

// --- E-vector level kernels (for kernel-granularity parity tests) ----------
void lgo_force_mult_E(void *h, const double *sJit, const double *XE, double *YE) { force_mult_E(*(Ctx *)h, sJit, XE, YE); }
void lgo_force_mult_t_E(void *h, const double *sJit, const double *YE, double *XE) { force_mult_t_E(*(Ctx *)h, sJit, YE, XE); }
void lgo_mass_apply_E(void *h, int space, const double *XE, double *YE) { mass_apply_E(*(Ctx *)h, space, XE, YE); }
void lgo_h1_gather(void *h, int vdim, const double *xL, double *XE) { h1_gather(*(Ctx *)h, vdim, xL, XE); }
void lgo_h1_scatter_add(void *h, int vdim, const double *YE, double *yL) { h1_scatter_add(*(Ctx *)h, vdim, YE, yL); }
void lgo_qkernel(void *h, const double *q_dx, const double *q_e, const double *q_dv, double *q_dt, double *sJit)
{
   Ctx *c = (Ctx *)h;
   const double inf = std::numeric_limits<double>::infinity();
   if (c->dim == 2) { QKernel<2>(c->NE, c->NQ, c->visc, c->vort, c->h0, (double)c->order_v, c->cfl, inf, c->gamma.data(), c->W.data(), q_dx, c->rho0DetJ0w.data(), q_e, q_dv, c->Jac0inv.data(), q_dt, sJit); }
   else { QKernel<3>(c->NE, c->NQ, c->visc, c->vort, c->h0, (double)c->order_v, c->cfl, inf, c->gamma.data(), c->W.data(), q_dx, c->rho0DetJ0w.data(), q_e, q_dv, c->Jac0inv.data(), q_dt, sJit); }
}
// dim == 1: x = Me_inv(e) b zone by zone (the FA energy solve, laghos_solver.cpp:501-515)
void lgo_l2_solve_local(void *h, const double *b, double *x) { fa_me_inv_mult(*(Ctx *)h, b, x); }
// small-matrix probes for tests (vs numpy)
void lgo_eig3(const double *A, double *lam, double *vec) { sm::CalcEigenvalues<3>(A, lam, vec); }
void lgo_eig2(const double *A, double *lam, double *vec) { sm::CalcEigenvalues<2>(A, lam, vec); }
double lgo_sv3(const double *A, int i) { return sm::CalcSingularvalue<3>(A, i); }
double lgo_sv2(const double *A, int i) { return sm::CalcSingularvalue<2>(A, i); }

// --- operator level (L-vectors), mirroring the reference classes -----------

// ForcePAOperator::Mult (laghos_assembly.cpp:557-565): x L2 L-vector, y H1 L-vector (byNODES)
void lgo_force_mult(void *h, const double *x, double *y)
{
   Ctx *c = (Ctx *)h;
   if (c->dim == 1) { fa_force_assemble(*c); fa_force_mult(*c, x, y); return; } // Force.Mult (FA)
   // L2R->Mult is the identity copy for lexicographic L2
   force_mult_E(*c, c->stressJinvT.data(), x, c->YE.data());
   h1_scatter_add(*c, c->dim, c->YE.data(), y);
   halo(y, c->dim);
}
// ForcePAOperator::MultTranspose (laghos_assembly.cpp:965-973)
void lgo_force_mult_transpose(void *h, const double *v, double *y)
{
   Ctx *c = (Ctx *)h;
   if (c->dim == 1) { fa_force_assemble(*c); fa_force_mult_t(*c, v, y); return; } // Force.MultTranspose (FA)
   h1_gather(*c, c->dim, v, c->YE.data());
   force_mult_t_E(*c, c->stressJinvT.data(), c->YE.data(), y);
}
// MassPAOperator::SetEssentialTrueDofs (laghos_assembly.cpp:98-110) with c_tdofs[comp]
void lgo_mass_set_ess(void *h, int comp) { ((Ctx *)h)->cur_ess = comp; }
// MassPAOperator::EliminateRHS (laghos_assembly.cpp:112-115)
void lgo_mass_eliminate_rhs(void *h, double *b)
{
   Ctx *c = (Ctx *)h;
   if (c->cur_ess >= 0)
      for (int i : c->ess[c->cur_ess]) { b[i] = 0.0; }
}
// MassPAOperator::MultFull / Mult (laghos_assembly.cpp:117-121; hpp:127)
void lgo_mass_mult(void *h, int space, int full, const double *x, double *y)
{
   Ctx *c = (Ctx *)h;
   if (c->dim == 1) // FA: the assembled Mv, and Me(e) zone by zone
   {
      if (space == 0)
      {
         fa_mv_mult(*c, x, y);
         if (!full && c->cur_ess >= 0)
            for (int i : c->ess[c->cur_ess]) { y[i] = 0.0; }
      }
      else { fa_me_mult(*c, x, y); }
      return;
   }
   if (space == 0)
   {
      h1_gather(*c, 1, x, c->XE.data());
      mass_apply_E(*c, 0, c->XE.data(), c->YE.data());
      h1_scatter_add(*c, 1, c->YE.data(), y);
      halo(y, 1);
      if (!full && c->cur_ess >= 0)
         for (int i : c->ess[c->cur_ess]) { y[i] = 0.0; }
   }
   else { mass_apply_E(*c, 1, x, y); }
}
// Jacobi diagonal for OperatorJacobiSmoother (laghos_solver.cpp:266-270), empty ess list
void lgo_mass_assemble_diag(void *h)
{
   Ctx *c = (Ctx *)h;
   if (c->dim == 1) { fa_diag(*c); return; }
   if (c->dim == 2) { mass_diag_dispatch<2>(c->D1D, c->Q1D, c->NE, c->B.data(), c->massD.data(), c->YE.data()); }
   else { mass_diag_dispatch<3>(c->D1D, c->Q1D, c->NE, c->B.data(), c->massD.data(), c->YE.data()); }
   h1_scatter_add(*c, 1, c->YE.data(), c->diagV.data());
   halo(c->diagV.data(), 1);
}

// Rho0DetJ0Vol (laghos_solver.cpp:1170-1261).  x0: H1 L-vector of initial node
// positions; rho0_l2: rho0 grid function (Bernstein L2 dofs) -> rho0DetJ0w and
// Jac0inv; rho0_q: the *function* rho0 at the physical quadrature points ->
// mass PA data (laghos_assembly.cpp:92-95).  Returns local volume.
double lgo_setup_rho0detj0(void *h, const double *x0, const double *rho0_l2, const double *rho0_q)
{
   Ctx *c = (Ctx *)h;
   if (c->dim == 1) { return fa_setup(*c, x0, rho0_l2, rho0_q); }
   const int dim = c->dim, NQ = c->NQ, NE = c->NE;
   h1_gather(*c, dim, x0, c->e_vec.data());
   if (dim == 2) { interp_dispatch<2>(c->D1D, c->Q1D, NE, dim, c->B.data(), c->G.data(), c->e_vec.data(), nullptr, c->q_dx.data()); }
   else { interp_dispatch<3>(c->D1D, c->Q1D, NE, dim, c->B.data(), c->G.data(), c->e_vec.data(), nullptr, c->q_dx.data()); }
   if (dim == 2) { interp_dispatch<2>(c->L1D, c->Q1D, NE, 1, c->Bl.data(), nullptr, rho0_l2, c->q_e.data(), nullptr); }
   else { interp_dispatch<3>(c->L1D, c->Q1D, NE, 1, c->Bl.data(), nullptr, rho0_l2, c->q_e.data(), nullptr); }
   double vol = 0.0;
   for (int e = 0; e < NE; e++)
      for (int q = 0; q < NQ; q++)
      {
         const size_t eq = (size_t)e * NQ + q;
         const double *J = c->q_dx.data() + eq * dim * dim; // J(i,j) at i + dim*j
         double *Ji = c->Jac0inv.data() + eq * dim * dim;
         double det;
         if (dim == 2)
         {
            const double J11 = J[0], J12 = J[1], J21 = J[2], J22 = J[3]; // names as reference :1209-1212
            det = sm::Det<2>(J);
            const double r = 1.0 / det;
            Ji[0] = J22 * r;
            Ji[1] = -J12 * r;
            Ji[2] = -J21 * r;
            Ji[3] = J11 * r;
         }
         else
         {
            // reference :1237-1251 with J(q,i,j,e): Jab = J(q,a-1,b-1,e)
            const double J11 = J[0], J12 = J[3], J13 = J[6];
            const double J21 = J[1], J22 = J[4], J23 = J[7];
            const double J31 = J[2], J32 = J[5], J33 = J[8];
            det = sm::Det<3>(J);
            const double r = 1.0 / det;
            Ji[0] = r * ((J22 * J33) - (J23 * J32));
            Ji[1] = r * ((J32 * J13) - (J33 * J12));
            Ji[2] = r * ((J12 * J23) - (J13 * J22));
            Ji[3] = r * ((J23 * J31) - (J21 * J33));
            Ji[4] = r * ((J33 * J11) - (J31 * J13));
            Ji[5] = r * ((J13 * J21) - (J11 * J23));
            Ji[6] = r * ((J21 * J32) - (J22 * J31));
            Ji[7] = r * ((J31 * J12) - (J32 * J11));
            Ji[8] = r * ((J11 * J22) - (J12 * J21));
         }
         c->rho0DetJ0w[eq] = c->W[q] * c->q_e[eq] * det;
         c->massD[eq] = c->W[q] * det * rho0_q[eq];
         vol += c->W[q] * det;
      }
   return vol;
}

// QUpdate::UpdateQuadratureData (laghos_solver.cpp:1354-1411); S = [x | v | e]
void lgo_qupdate(void *h, const double *S)
{
   Ctx *c = (Ctx *)h;
   const double t0 = now();
   const int dim = c->dim, NE = c->NE;
   if (dim == 1)
   {
      fa_qupdate(*c, S);
      c->t_qdata += now() - t0;
      c->quad_tstep += NE;
      return;
   }
   const double *x = S, *v = S + c->H1V, *e = S + 2 * (size_t)c->H1V;
   h1_gather(*c, dim, x, c->e_vec.data());
   if (dim == 2) { interp_dispatch<2>(c->D1D, c->Q1D, NE, dim, c->B.data(), c->G.data(), c->e_vec.data(), nullptr, c->q_dx.data()); }
   else { interp_dispatch<3>(c->D1D, c->Q1D, NE, dim, c->B.data(), c->G.data(), c->e_vec.data(), nullptr, c->q_dx.data()); }
   h1_gather(*c, dim, v, c->e_vec.data());
   if (dim == 2) { interp_dispatch<2>(c->D1D, c->Q1D, NE, dim, c->B.data(), c->G.data(), c->e_vec.data(), nullptr, c->q_dv.data()); }
   else { interp_dispatch<3>(c->D1D, c->Q1D, NE, dim, c->B.data(), c->G.data(), c->e_vec.data(), nullptr, c->q_dv.data()); }
   if (dim == 2) { interp_dispatch<2>(c->L1D, c->Q1D, NE, 1, c->Bl.data(), nullptr, e, c->q_e.data(), nullptr); }
   else { interp_dispatch<3>(c->L1D, c->Q1D, NE, 1, c->Bl.data(), nullptr, e, c->q_e.data(), nullptr); }
   std::fill(c->q_dt.begin(), c->q_dt.end(), c->dt_est); // :1374
   lgo_qkernel(h, c->q_dx.data(), c->q_e.data(), c->q_dv.data(), c->q_dt.data(), c->stressJinvT.data());
   double m = std::numeric_limits<double>::infinity();
   for (double d : c->q_dt) { m = std::fmin(m, d); }
   c->dt_est = m; // :1406
   c->t_qdata += now() - t0;
   c->quad_tstep += NE;
}

// CGSolver::Mult (upstream MFEM linalg/solvers.cpp, restated).
// space 0: scalar H1 mass with the active essential list, Jacobi
// preconditioner, iterative_mode=true (X holds the initial guess);
// space 1: L2 mass, no preconditioner, iterative_mode=false.
// Dot products count shared dofs once (owner mask) and are all-reduced.
int lgo_cg(void *h, int space, const double *b, double *x, double rel_tol, int max_iter)
{
   Ctx *c = (Ctx *)h;
   const double t0 = now();
   const int n = space == 0 ? c->N : c->L2V;
   double *r = c->cg_r.data(), *z = c->cg_z.data(), *d = c->cg_d.data();
   auto dot = [&](const double *a, const double *bb) {
      const double s = space == 0 ? dot_owned(*c, a, bb) : dot_plain(n, a, bb);
      return allreduce(s, 0);
   };
   int final_iter = 0;
   const bool prec = (space == 0);
   if (space == 0)
   {
      lgo_mass_mult(h, 0, 0, x, r);
      for (int i = 0; i < n; i++) { r[i] = b[i] - r[i]; }
   }
   else
   {
      for (int i = 0; i < n; i++) { r[i] = b[i]; x[i] = 0.0; }
   }
   if (prec)
   {
      for (int i = 0; i < n; i++) { z[i] = r[i] / c->diagV[i]; d[i] = z[i]; }
   }
   else
   {
      for (int i = 0; i < n; i++) { d[i] = r[i]; }
   }
   double nom = dot(d, r);
   if (nom < 0.0) { final_iter = 0; goto done; }
   {
      const double r0 = std::max(nom * rel_tol * rel_tol, 0.0);
      if (nom <= r0) { final_iter = 0; goto done; }
      lgo_mass_mult(h, space, 0, d, z);
      double den = dot(z, d);
      if (den <= 0.0 && den == 0.0) { final_iter = 0; goto done; }
      final_iter = max_iter;
      for (int i = 1; true;)
      {
         const double alpha = nom / den;
         c->cg_last[0] = nom; c->cg_last[1] = den; c->cg_last[2] = alpha;
#pragma omp parallel for schedule(static)
         for (int k = 0; k < n; k++)
         {
            x[k] = x[k] + alpha * d[k];
            r[k] = r[k] - alpha * z[k];
         }
         double betanom;
         if (prec)
         {
#pragma omp parallel for schedule(static)
            for (int k = 0; k < n; k++) { z[k] = r[k] / c->diagV[k]; }
            betanom = dot(r, z);
         }
         else { betanom = dot(r, r); }
         c->cg_last[3] = betanom;
         if (betanom < 0.0) { final_iter = i; break; }
         if (betanom <= r0) { final_iter = i; break; }
         if (++i > max_iter) { break; }
         const double beta = betanom / nom;
         if (prec)
         {
#pragma omp parallel for schedule(static)
            for (int k = 0; k < n; k++) { d[k] = z[k] + beta * d[k]; }
         }
         else
         {
#pragma omp parallel for schedule(static)
            for (int k = 0; k < n; k++) { d[k] = r[k] + beta * d[k]; }
         }
         lgo_mass_mult(h, space, 0, d, z);
         den = dot(d, z);
         if (den <= 0.0 && den == 0.0) { final_iter = i; break; }
         nom = betanom;
      }
   }
done:
   if (space == 0) { c->t_cgH1 += now() - t0; c->H1iter += final_iter; }
   else { c->t_cgL2 += now() - t0; c->L2iter += (final_iter == 0) ? 1 : final_iter; } // laghos_solver.cpp:486
   return final_iter;
}

// The recurrence as the last lgo_cg call left it (tests/test_gpu_k2.py holds ONE launch of the HIP path's node kernel
// against one iteration of THIS loop): which = 0: r, 1: z (space 0: r / diag; space 1: the last A d), 2: d - the
// direction of the last iteration performed; out[4] = (r, z) before that iteration, (d, A d), alpha, (r, z) after it.
const double *lgo_cg_vec(void *h, int which)
{
   Ctx *c = (Ctx *)h;
   return which == 0 ? c->cg_r.data() : which == 1 ? c->cg_z.data() : c->cg_d.data();
}
void lgo_cg_scalars(void *h, double out[4])
{
   Ctx *c = (Ctx *)h;
   for (int k = 0; k < 4; k++) { out[k] = c->cg_last[k]; }
}

// LagrangianHydroOperator::Mult (laghos_solver.cpp:308-327) with
// SolveVelocity (:329-399) and SolveEnergy (:442-490), PA branch, no sources.
// S = [x|v|e], dS = [dx|dv|de].  The caller owns the qdata_is_current flag
// (laghos_solver.cpp:809-812, :326): when set, UpdateQuadratureData is skipped.
// SolveVelocity (laghos_solver.cpp:328-398): dv_dt block of dS
static const double *g_accel_src = nullptr; // set per call by lgo_solve_velocity_src
void lgo_solve_velocity(void *h, const double *S, double *dS, double cg_tol, int cg_max_iter,
                        int qdata_is_current /* :809 early return */)
{
   Ctx *c = (Ctx *)h;
   const int dim = c->dim, N = c->N, H1V = c->H1V, L2V = c->L2V;
   double *dv = dS + H1V;
   if (!qdata_is_current) { lgo_qupdate(h, S); } // :332, :809
   std::fill(dv, dv + H1V, 0.0);
   std::vector<double> one(L2V, 1.0), rhs(H1V), Bv(N);
   double t0 = now();
   lgo_force_mult(h, one.data(), rhs.data()); // :354
   c->t_force += now() - t0;
   for (int i = 0; i < H1V; i++) { rhs[i] = -rhs[i]; } // :358
   for (int cc = 0; cc < dim; cc++)
   {
      std::memcpy(Bv.data(), rhs.data() + (size_t)cc * N, sizeof(double) * N); // :368-369
      if (g_accel_src) // source_type == 2: B += VMassPA->MultFull(accel_c) (:371-380)
      {
         std::vector<double> BA(N);
         lgo_mass_mult(h, 0, 1, g_accel_src + (size_t)cc * N, BA.data());
         for (int i = 0; i < N; i++) { Bv[i] += BA[i]; }
      }
      double *X = dv + (size_t)cc * N;                                           // :382 (dv = 0)
      lgo_mass_set_ess(h, cc);                                                   // :383
      lgo_mass_eliminate_rhs(h, Bv.data());                                      // :384
      lgo_cg(h, 0, Bv.data(), X, cg_tol, cg_max_iter);                           // :388
   }
}

// SolveVelocity with the acceleration source of problem 7 (source_type 2, :340-347:
// accel = nodal projection of RTCoefficient = (0, -1))
void lgo_solve_velocity_src(void *h, const double *S, double *dS, double cg_tol, int cg_max_iter,
                            int qdata_is_current, const double *accel_h1)
{
   g_accel_src = accel_h1;
   lgo_solve_velocity(h, S, dS, cg_tol, cg_max_iter, qdata_is_current);
   g_accel_src = nullptr;
}

// SolveEnergy (laghos_solver.cpp:400-493) with the velocity v (RK2Avg passes the
// half-step average V, Mult passes the v block of S); the quadrature data is current
void lgo_solve_energy(void *h, const double *v, double *dS, double cg_tol, int cg_max_iter,
                      const double *e_source /* optional L2 L-vector or NULL */)
{
   Ctx *c = (Ctx *)h;
   const int H1V = c->H1V, L2V = c->L2V;
   double *de = dS + 2 * (size_t)H1V;
   std::vector<double> e_rhs(L2V);
   double t0 = now();
   lgo_force_mult_transpose(h, v, e_rhs.data()); // :473
   c->t_force += now() - t0;
   if (e_source)
      for (int i = 0; i < L2V; i++) { e_rhs[i] += e_source[i]; } // :477
   if (c->dim == 1) // FA: Me_inv(e).Mult zone by zone, L2iter += 1 per zone (:501-515)
   {
      t0 = now();
      fa_me_inv_mult(*c, e_rhs.data(), de);
      c->t_cgL2 += now() - t0;
      c->L2iter += c->NE;
      return;
   }
   lgo_cg(h, 1, e_rhs.data(), de, cg_tol, cg_max_iter); // :481
}

// LagrangianHydroOperator::Mult (laghos_solver.cpp:308-326)
void lgo_hydro_mult(void *h, const double *S, double *dS, double cg_tol, int cg_max_iter,
                    const double *e_source /* optional L2 L-vector or NULL */,
                    int qdata_is_current /* :809 early return */)
{
   Ctx *c = (Ctx *)h;
   const int H1V = c->H1V;
   const double *v = S + H1V;
   std::memcpy(dS, v, sizeof(double) * H1V); // :323
   lgo_solve_velocity(h, S, dS, cg_tol, cg_max_iter, qdata_is_current); // g_accel_src: see lgo_hydro_mult_src
   lgo_solve_energy(h, v, dS, cg_tol, cg_max_iter, e_source);
}

// ComputeVolumeIntegral users (laghos_solver.cpp:640-697): internal and kinetic energy
double lgo_internal_energy(void *h, const double *e)
{
   Ctx *c = (Ctx *)h;
   if (c->dim == 1)
      for (int el = 0; el < c->NE; el++)
         for (int q = 0; q < c->Q1D; q++) { c->q_e[(size_t)el * c->Q1D + q] = fa_interp(c->Bl, c->Q1D, q, c->L1D, e + (size_t)el * c->L1D); }
   else if (c->dim == 2) { interp_dispatch<2>(c->L1D, c->Q1D, c->NE, 1, c->Bl.data(), nullptr, e, c->q_e.data(), nullptr); }
   else { interp_dispatch<3>(c->L1D, c->Q1D, c->NE, 1, c->Bl.data(), nullptr, e, c->q_e.data(), nullptr); }
   double s = 0.0;
   for (size_t i = 0; i < (size_t)c->NE * c->NQ; i++) { s += c->q_e[i] * c->rho0DetJ0w[i]; }
   return allreduce(s, 0);
}
double lgo_kinetic_energy(void *h, const double *v)
{
   Ctx *c = (Ctx *)h;
   const int dim = c->dim;
   std::vector<double> qv((size_t)c->NE * c->NQ * dim);
   h1_gather(*c, dim, v, c->e_vec.data());
   if (dim == 1)
      for (int el = 0; el < c->NE; el++)
         for (int q = 0; q < c->Q1D; q++) { qv[(size_t)el * c->Q1D + q] = fa_interp(c->B, c->Q1D, q, c->D1D, c->e_vec.data() + (size_t)el * c->D1D); }
   else if (dim == 2) { interp_dispatch<2>(c->D1D, c->Q1D, c->NE, dim, c->B.data(), c->G.data(), c->e_vec.data(), qv.data(), nullptr); }
   else { interp_dispatch<3>(c->D1D, c->Q1D, c->NE, dim, c->B.data(), c->G.data(), c->e_vec.data(), qv.data(), nullptr); }
   double s = 0.0;
   for (size_t i = 0; i < (size_t)c->NE * c->NQ; i++)
   {
      double vm = 0.0;
      for (int k = 0; k < dim; k++) { vm += qv[k + dim * i] * qv[k + dim * i]; }
      s += vm * c->rho0DetJ0w[i];
   }
   return 0.5 * allreduce(s, 0);
}

// 2D Taylor-Green energy source (laghos_solver.cpp:454-465, TaylorCoefficient
// laghos_solver.hpp:208-218): e_src_i = sum_q w_q detJ(q) f(x_q) phi_i(q) on the
// CURRENT mesh.  Uses q_dx (Jacobians) left by the last lgo_qupdate(S).
void lgo_tg_source_2d(void *h, const double *S, double *out)
{
   Ctx *c = (Ctx *)h;
   if (c->dim != 2) { std::abort(); }
   const int NQ = c->NQ, NE = c->NE, L = c->L1D, Q = c->Q1D;
   std::vector<double> xq((size_t)NE * NQ * 2);
   h1_gather(*c, 2, S, c->e_vec.data());
   interp_dispatch<2>(c->D1D, c->Q1D, NE, 2, c->B.data(), c->G.data(), c->e_vec.data(), xq.data(), c->q_dx.data());
   for (int e = 0; e < NE; e++)
   {
      for (int l = 0; l < c->NL; l++) { out[l + (size_t)c->NL * e] = 0.0; }
      for (int qy = 0; qy < Q; qy++)
         for (int qx = 0; qx < Q; qx++)
         {
            const size_t eq = (size_t)e * NQ + qx + Q * qy;
            const double x0 = xq[0 + 2 * eq], x1 = xq[1 + 2 * eq];
            const double f = 3.0 / 8.0 * M_PI * (std::cos(3.0 * M_PI * x0) * std::cos(M_PI * x1) - std::cos(M_PI * x0) * std::cos(3.0 * M_PI * x1));
            const double wdet = c->W[qx + Q * qy] * sm::Det<2>(c->q_dx.data() + 4 * eq);
            for (int ly = 0; ly < L; ly++)
               for (int lx = 0; lx < L; lx++)
               {
                  out[lx + L * ly + (size_t)c->NL * e] += wdet * f * c->Bl[qx + Q * lx] * c->Bl[qy + Q * ly];
               }
         }
   }
}

int lgo_num_threads()
{
#ifdef _OPENMP
   return omp_get_max_threads();
#else
   return 1;
#endif
}
void lgo_set_num_threads(int n)
{
#ifdef _OPENMP
   omp_set_num_threads(n);
#else
   (void)n;
#endif
}

} // extern "C"
