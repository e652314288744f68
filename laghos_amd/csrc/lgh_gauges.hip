// lgh_gauges.hip — time series at material points (the driver's `-gauges`): x, v, rho, e, p, cs, det J and
// div v of the state at a few points given as (zone, reference coordinates), appended sample by sample to a device buffer.
//
// Replaces nothing in the reference: /root/reference/laghos.cpp writes snapshots only (VisItDataCollection::Save,
// laghos.cpp:845-871).  A point (zone, xi) is the same particle in every cycle, so nothing is located after t = 0; the caller
// hands over the 1-D basis values at xi (the library holds no basis definition, as with the lattice tables).
//
// One wavefront per gauge, kGaugesPerGroup gauges per workgroup.  The wave gathers the zone's dofs into its slice of LDS - the
// dim components of x (with e), then those of v through the same LDS - and contracts them with the stages of lgh_sample.hpp
// for a lattice of ONE point whose table row is the gauge's: x axis first, then y, then z, every sum over d ascending in one
// thread, B or G per axis as derived_component (lgh_derived.hip) takes them.  A gauge at a lattice point therefore has the
// bits lgh_sample_fields / lgh_sample_derived hold there.  The dim (dim + 1) values and derivatives of a pass go to a small
// result block in LDS; every lane then forms the point values with the shared expressions (derived_adj, derived_grad,
// derived_cs, sample_pressure) and lanes 0..11 store the row: one 96-byte store per gauge.  The density is the scheme's own
// pointwise one, rho = m_g / det J with m_g = rho0(xi) det J0(xi) formed once by the same kernel on (x0, rho0_l2): no
// projection.  No branch looks at the sign of det J, no atomics, no scratch.  A gauge another rank owns (zone -1) gets a row
// of -0.0: x + (-0.0) has the bits of x, so the ranks' SUM all-reduce at the drain is an exact gather.
#include "lgh_common.hpp"
#include "lgh_sample.hpp"

#include <algorithm>
#include <cmath>

namespace lgh
{

constexpr int kGaugesPerGroup = 4; // one wavefront each
constexpr size_t kGaugeLdsBudget = 48 * 1024;

struct GaugeArgs
{
   const int *zone;           // n: the caller's zone id, -1: not this rank's
   const double *Bh, *Gh, *Bl; // [(g*dim + a)*D + d], the same, [(g*dim + a)*L + l]
   const double *x, *v, *e;   // component c of x at x + c*N; e: the L2 dofs (mass mode: x0, unused, rho0_l2)
   const double *mass;        // n: m_g (sample mode)
   double *out;               // sample mode: n rows of LGH_GAUGE_COLS; mass mode: n values
   const int *map;
   const double *gamma;
   long N;
   int n, D, L;
   int stride;                // doubles of LDS per gauge
   int mass_mode;
};

// LDS of one gauge, in doubles: the tables, the result block, dim H1 components with their stages, e with its stages
template <int DIM> struct GaugeLayout
{
   int D, L, ND, NL, h1, l2;
   __host__ __device__ GaugeLayout(const int D_, const int L_) : D(D_), L(L_)
   {
      ND = (DIM == 3) ? D * D * D : (DIM == 2 ? D * D : D);
      NL = (DIM == 3) ? L * L * L : (DIM == 2 ? L * L : L);
      h1 = ND + (DIM >= 2 ? 2 * (ND / D) : 0) + (DIM == 3 ? 3 * D : 0); // U | B1 G1 | BB GB BG
      l2 = NL + (DIM >= 2 ? NL / L : 0) + (DIM == 3 ? L : 0);           // E | E1 | E2
   }
   __host__ __device__ int tables() const { return DIM * (2 * D + L); }
   __host__ __device__ static constexpr int results() { return 2 * DIM * (DIM + 1) + 1; }
   __host__ __device__ int total() const { return tables() + results() + DIM * h1 + l2; }
};

// The dim components of one H1 field of the wave's zone (component c at src + c*N): their dim derivatives and their value at
// the gauge into res[c*(DIM+1) + j], j < DIM the derivative along xi_j, j == DIM the value.  Synchronises before it returns.
template <int DIM>
__device__ __forceinline__ void gauge_h1_pass(const GaugeArgs &a, const GaugeLayout<DIM> &ly, const double *__restrict__ src, const bool live, const int zone,
                                              const int lane, const double *Th, const double *Gh, double *H, double *res)
{
   const int D = ly.D, ND = ly.ND, HS = ly.h1, P1 = ND / D;
   if (live)
   {
      for (int i = lane; i < DIM * ND; i += kWave)
      {
         const int c = i / ND, d = i - c * ND;
         H[c * HS + d] = src[(size_t)c * a.N + a.map[(size_t)zone * ND + d]];
      }
   }
   __syncthreads();
   // per component: U | B1 G1 | BB GB BG (the stages of derived_component on a lattice of one point)
   if (DIM >= 2 && live)
   {
      for (int i = lane; i < DIM * 2 * P1; i += kWave)
      {
         const int hi = i % P1, k = (i / P1) & 1, c = i / (2 * P1);
         const double *U = H + c * HS;
         double *o = H + c * HS + ND + k * P1;
         o[hi] = sample_dot(D, 1, 1, k ? Gh : Th, U + hi * D);
      }
   }
   if (DIM >= 2) { __syncthreads(); }
   if (DIM == 3 && live)
   {
      for (int i = lane; i < DIM * 3 * D; i += kWave)
      {
         const int hi = i % D, k = (i / D) % 3, c = i / (3 * D);
         const double *B1 = H + c * HS + ND, *G1 = B1 + P1;
         double *o = H + c * HS + ND + 2 * P1 + k * D;
         // BB = B_y B1, GB = B_y G1, BG = G_y B1
         o[hi] = sample_dot(D, 1, 1, (k == 2 ? Gh : Th) + D, (k == 1 ? G1 : B1) + hi * D);
      }
   }
   if (DIM == 3) { __syncthreads(); }
   if (live && lane < DIM * (DIM + 1))
   {
      const int c = lane / (DIM + 1), j = lane - c * (DIM + 1);
      const double *U = H + c * HS, *B1 = U + ND, *G1 = B1 + P1, *BB = G1 + P1, *GB = BB + D, *BG = GB + D;
      double s;
      if constexpr (DIM == 1) { s = sample_last(D, 1, 1, 0, j == 0 ? Gh : Th, U); }
      else if constexpr (DIM == 2) { s = sample_last(D, 1, 1, 0, (j == 1 ? Gh : Th) + D, j == 0 ? G1 : B1); }
      else { s = sample_last(D, 1, 1, 0, (j == 2 ? Gh : Th) + 2 * D, j == 0 ? GB : (j == 1 ? BG : BB)); }
      res[lane] = s;
   }
   __syncthreads(); // the next pass gathers into the same LDS
}

template <int DIM>
__global__ void __launch_bounds__(kGaugesPerGroup *kWave) gauges_k(const GaugeArgs a)
{
   extern __shared__ double sm[];
   const GaugeLayout<DIM> ly(a.D, a.L);
   const int D = a.D, L = a.L, NL = ly.NL;
   const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
   const int g = blockIdx.x * (blockDim.x / kWave) + w;
   const int zone = (g < a.n) ? a.zone[g] : -1; // (the same in every lane of the wave)
   const bool live = zone >= 0;
   double *Th = sm + (size_t)w * a.stride, *Gh = Th + DIM * D, *Tl = Gh + DIM * D, *res = Tl + DIM * L;
   double *H = res + ly.results(), *E = H + DIM * ly.h1;
   if (live)
   {
      for (int i = lane; i < DIM * D; i += kWave)
      {
         Th[i] = a.Bh[(size_t)g * DIM * D + i];
         Gh[i] = a.Gh[(size_t)g * DIM * D + i];
      }
      for (int i = lane; i < DIM * L; i += kWave) { Tl[i] = a.Bl[(size_t)g * DIM * L + i]; }
      for (int i = lane; i < NL; i += kWave) { E[i] = a.e[(size_t)zone * NL + i]; }
   }
   // (the first gather's barrier covers the tables and e)
   gauge_h1_pass<DIM>(a, ly, a.x, live, zone, lane, Th, Gh, H, res);
   if (!a.mass_mode) { gauge_h1_pass<DIM>(a, ly, a.v, live, zone, lane, Th, Gh, H, res + DIM * (DIM + 1)); }
   // e as lgh_sample_fields contracts it
   double *E1 = E + NL, *E2 = E1 + NL / L;
   if (DIM >= 2)
   {
      if (live)
      {
         for (int i = lane; i < NL / L; i += kWave) { E1[i] = sample_dot(L, 1, 1, Tl, E + i * L); }
      }
      __syncthreads();
   }
   if (DIM == 3)
   {
      if (live)
      {
         for (int i = lane; i < L; i += kWave) { E2[i] = sample_dot(L, 1, 1, Tl + L, E1 + i * L); }
      }
      __syncthreads();
   }
   if (live && lane == 0) { res[2 * DIM * (DIM + 1)] = sample_last(L, 1, 1, 0, Tl + (DIM - 1) * L, DIM == 3 ? E2 : (DIM == 2 ? E1 : E)); }
   __syncthreads();
   if (g >= a.n) { return; }
   // the point values: every lane forms them, lanes 0 .. LGH_GAUGE_COLS - 1 store one column each
   double row[LGH_GAUGE_COLS];
   if (live)
   {
      double J[DIM][DIM], V[DIM][DIM], A[DIM][DIM];
#pragma unroll
      for (int k = 0; k < LGH_GAUGE_COLS; k++) { row[k] = 0.0; }
#pragma unroll
      for (int c = 0; c < DIM; c++)
      {
#pragma unroll
         for (int j = 0; j < DIM; j++)
         {
            J[c][j] = res[c * (DIM + 1) + j];
            V[c][j] = a.mass_mode ? 0.0 : res[(DIM + c) * (DIM + 1) + j];
         }
         row[c] = res[c * (DIM + 1) + DIM];
         row[3 + c] = a.mass_mode ? 0.0 : res[(DIM + c) * (DIM + 1) + DIM];
      }
      const double ev = res[2 * DIM * (DIM + 1)];
      const double det = derived_adj<DIM>(J, A);
      if (a.mass_mode)
      {
         if (lane == 0) { a.out[g] = ev * det; } // m_g = rho0(xi) det J0(xi)
         return;
      }
      double div = 0.0;
      derived_grad<DIM>(V, A, det, 0, 1, nullptr, &div, nullptr);
      const double gz = a.gamma[zone];
      const double rho = a.mass[g] / det;
      row[6] = rho;
      row[7] = ev;
      row[8] = sample_pressure(gz, rho, ev);
      row[9] = derived_cs(gz, ev);
      row[10] = det;
      row[11] = div;
   }
   else
   {
      if (a.mass_mode)
      {
         if (lane == 0) { a.out[g] = -0.0; }
         return;
      }
#pragma unroll
      for (int k = 0; k < LGH_GAUGE_COLS; k++) { row[k] = -0.0; }
   }
   double mine = row[0];
#pragma unroll
   for (int k = 1; k < LGH_GAUGE_COLS; k++) { mine = (lane == k) ? row[k] : mine; }
   if (lane < LGH_GAUGE_COLS) { a.out[(size_t)g * LGH_GAUGE_COLS + lane] = mine; }
}

// gauges per workgroup - one wavefront each - and the LDS of one gauge for this context (one that does not fit kGaugeLdsBudget
// is refused at create)
static void gauge_shape(const lgh_ctx *c, int *per_group, size_t *gauge_bytes)
{
   const int D = c->D1D, L = c->L1D;
   const int doubles = c->dim == 3 ? GaugeLayout<3>(D, L).total() : (c->dim == 2 ? GaugeLayout<2>(D, L).total() : GaugeLayout<1>(D, L).total());
   *gauge_bytes = (size_t)doubles * sizeof(double);
   *per_group = patches_per_group(kGaugesPerGroup * kWave, kWave, 0, *gauge_bytes);
}

static int gauge_launch(lgh_ctx *c, const GaugeSet &s, const double *x, const double *v, const double *e, double *out, const bool mass_mode)
{
   int G;
   size_t bytes;
   gauge_shape(c, &G, &bytes);
   GaugeArgs a;
   memset(&a, 0, sizeof(a));
   a.zone = s.zone; a.Bh = s.Bh; a.Gh = s.Gh; a.Bl = s.Bl;
   a.x = x; a.v = v; a.e = e;
   a.mass = s.mass; a.out = out;
   a.map = c->h1map; a.gamma = c->gamma;
   a.N = c->N; a.n = s.n; a.D = c->D1D; a.L = c->L1D;
   a.stride = (int)(bytes / sizeof(double));
   a.mass_mode = mass_mode ? 1 : 0;
   const dim3 grid((unsigned)ceil_div(s.n, G)), block((unsigned)(G * kWave));
   const size_t lds = (size_t)G * bytes;
   if (c->dim == 3) { hipLaunchKernelGGL(gauges_k<3>, grid, block, lds, c->stream, a); }
   else if (c->dim == 2) { hipLaunchKernelGGL(gauges_k<2>, grid, block, lds, c->stream, a); }
   else { hipLaunchKernelGGL(gauges_k<1>, grid, block, lds, c->stream, a); }
   LGH_HIP_CHECK(hipGetLastError());
   return LGH_OK;
}

static GaugeSet *gauge_set(lgh_ctx *c, const int handle, const char *who)
{
   if (!c)
   {
      set_error("%s: the context is NULL", who);
      return nullptr;
   }
   if (handle < 0 || handle >= (int)c->gauges.size() || !c->gauges[handle])
   {
      set_error("%s: handle %d names no gauge set of this context", who, handle);
      return nullptr;
   }
   return c->gauges[handle].get();
}

} // namespace lgh

using namespace lgh;

extern "C"
{

int lgh_gauges_create(lgh_ctx *c, int n, const int *zone, const double *Bh, const double *Gh, const double *Bl, const double *x0_h1,
                      const double *rho0_l2, int capacity, int *handle)
{
   LGH_CHECK_ARG(c);
   // what every rank sees alike: refused at once
   if (n < 1 || capacity < 1)
   {
      set_error("lgh_gauges_create: %s = %d (at least 1)", n < 1 ? "n" : "capacity", n < 1 ? n : capacity);
      return LGH_ERR_ARG;
   }
   const void *ptrs[7] = {zone, Bh, Gh, Bl, x0_h1, rho0_l2, handle};
   const char *names[7] = {"zone", "Bh", "Gh", "Bl", "x0_h1", "rho0_l2", "handle"};
   for (int i = 0; i < 7; i++)
   {
      if (!ptrs[i])
      {
         set_error("lgh_gauges_create: %s is NULL", names[i]);
         return LGH_ERR_ARG;
      }
   }
   if (!c->setup_done)
   {
      set_error("lgh_gauges_create: called before lgh_setup_rho0detj0 (the initial density and mesh are not known)");
      return LGH_ERR_ARG;
   }
   const int dim = c->dim, D = c->D1D, L = c->L1D;
   int G;
   size_t bytes;
   gauge_shape(c, &G, &bytes);
   if (bytes > kGaugeLdsBudget)
   {
      set_error("lgh_gauges_create: one gauge of D1D = %d needs %zu bytes of LDS (at most %zu)", D, bytes, kGaugeLdsBudget);
      return LGH_ERR_UNSUPPORTED;
   }
   if ((long)capacity * n > LGH_GAUGE_MAX_ROWS)
   {
      set_error("lgh_gauges_create: capacity = %d samples of n = %d gauges are %ld rows (at most %ld)", capacity, n, (long)capacity * n, (long)LGH_GAUGE_MAX_ROWS);
      return LGH_ERR_ARG;
   }
   // what a rank sees of its own: the ranks agree on the outcome before anything is kept
   int bad = 0;
   for (int g = 0; g < n && !bad; g++)
   {
      if (zone[g] < -1 || zone[g] >= c->NE)
      {
         set_error("lgh_gauges_create: zone[%d] = %d is outside -1..%d", g, zone[g], c->NE - 1);
         bad = 1;
      }
   }
   const auto table_ok = [&](const double *T, const int per, const char *name) {
      for (size_t i = 0; i < (size_t)n * dim * per; i++)
      {
         if (!std::isfinite(T[i]))
         {
            set_error("lgh_gauges_create: %s[%zu] = %g is not finite (gauge %zu)", name, i, T[i], i / ((size_t)dim * per));
            return false;
         }
      }
      return true;
   };
   if (!bad && !(table_ok(Bh, D, "Bh") && table_ok(Gh, D, "Gh") && table_ok(Bl, L, "Bl"))) { bad = 1; }
   std::vector<double> owners((size_t)n + 1);
   for (int g = 0; g < n; g++) { owners[g] = (!bad && zone[g] >= 0) ? 1.0 : 0.0; }
   owners[n] = bad ? 1.0 : 0.0;
   if (c->multi != 0 && c->comm)
   {
      DevPtr<double> od;
      LGH_PASS(od.upload(owners.data(), owners.size()));
      LGH_PASS(allreduce_dev_n(c, od, (long)owners.size(), 0));
      LGH_HIP_CHECK(hipStreamSynchronize(c->stream));
      LGH_HIP_CHECK(hipMemcpy(owners.data(), od, owners.size() * sizeof(double), hipMemcpyDeviceToHost));
   }
   if (bad) { return LGH_ERR_ARG; }
   if (owners[n] != 0.0)
   {
      set_error("lgh_gauges_create: refused on another rank (%g ranks found a bad zone or table entry)", owners[n]);
      return LGH_ERR_ARG;
   }
   for (int g = 0; g < n; g++)
   {
      if (owners[g] != 1.0)
      {
         set_error("lgh_gauges_create: gauge %d is owned by %g ranks (exactly one must give its zone)", g, owners[g]);
         return LGH_ERR_ARG;
      }
   }
   auto s = std::make_unique<GaugeSet>();
   s->n = n;
   s->capacity = capacity;
   LGH_PASS(s->zone.upload(zone, (size_t)n));
   LGH_PASS(s->Bh.upload(Bh, (size_t)n * dim * D));
   LGH_PASS(s->Gh.upload(Gh, (size_t)n * dim * D));
   LGH_PASS(s->Bl.upload(Bl, (size_t)n * dim * L));
   LGH_PASS(s->mass.alloc((size_t)n));
   LGH_PASS(s->rows.alloc((size_t)capacity * n * LGH_GAUGE_COLS));
   LGH_PASS(gauge_launch(c, *s, x0_h1, nullptr, rho0_l2, s->mass, true));
   LGH_HIP_CHECK(hipStreamSynchronize(c->stream)); // (x0_h1 and rho0_l2 are the caller's: done with them on return)
   int h = 0;
   while (h < (int)c->gauges.size() && c->gauges[h]) { h++; }
   if (h == (int)c->gauges.size()) { c->gauges.emplace_back(); }
   c->gauges[h] = std::move(s);
   *handle = h;
   return LGH_OK;
}

int lgh_gauges_sample(lgh_ctx *c, int handle, const double *S)
{
   GaugeSet *s = gauge_set(c, handle, "lgh_gauges_sample");
   if (!s) { return LGH_ERR_ARG; }
   if (!S)
   {
      set_error("lgh_gauges_sample: S is NULL");
      return LGH_ERR_ARG;
   }
   if (s->pending >= s->capacity)
   {
      set_error("lgh_gauges_sample: the buffer holds %d samples of capacity = %d: drain it first", s->pending, s->capacity);
      return LGH_ERR_ARG;
   }
   KtScope kt(c, LGH_KERNEL_GAUGES);
   LGH_PASS(gauge_launch(c, *s, S, S + (size_t)c->H1V, S + 2 * (size_t)c->H1V, s->rows + (size_t)s->pending * s->n * LGH_GAUGE_COLS, false));
   s->pending++;
   return LGH_OK;
}

int lgh_gauges_pending(lgh_ctx *c, int handle, int *samples)
{
   GaugeSet *s = gauge_set(c, handle, "lgh_gauges_pending");
   if (!s) { return LGH_ERR_ARG; }
   LGH_CHECK_ARG(samples);
   *samples = s->pending;
   return LGH_OK;
}

int lgh_gauges_drain(lgh_ctx *c, int handle, double *host_out, int max_samples, int *samples)
{
   GaugeSet *s = gauge_set(c, handle, "lgh_gauges_drain");
   if (!s) { return LGH_ERR_ARG; }
   if (!samples || (!host_out && s->pending > 0))
   {
      set_error("lgh_gauges_drain: %s is NULL", !samples ? "samples" : "host_out");
      return LGH_ERR_ARG;
   }
   if (max_samples < s->pending)
   {
      set_error("lgh_gauges_drain: max_samples = %d, but %d samples are pending", max_samples, s->pending);
      return LGH_ERR_ARG;
   }
   const long count = (long)s->pending * s->n * LGH_GAUGE_COLS;
   if (count > 0)
   {
      // every rank holds -0.0 where it owns nothing: the sum is a gather, whatever route a piece takes - the transport's
      // all-reduce, or allreduce_dev's exchange with every peer for pieces of one to three values - since both add in rank order
      if (c->multi != 0 && c->comm) { LGH_PASS(allreduce_dev_n(c, s->rows, count, 0)); }
      LGH_HIP_CHECK(hipStreamSynchronize(c->stream));
      LGH_HIP_CHECK(hipMemcpy(host_out, s->rows, (size_t)count * sizeof(double), hipMemcpyDeviceToHost));
   }
   *samples = s->pending;
   s->pending = 0;
   return LGH_OK;
}

int lgh_gauges_mass(lgh_ctx *c, int handle, double *host_m)
{
   GaugeSet *s = gauge_set(c, handle, "lgh_gauges_mass");
   if (!s) { return LGH_ERR_ARG; }
   LGH_CHECK_ARG(host_m);
   LGH_HIP_CHECK(hipStreamSynchronize(c->stream));
   LGH_HIP_CHECK(hipMemcpy(host_m, s->mass, (size_t)s->n * sizeof(double), hipMemcpyDeviceToHost));
   return LGH_OK;
}

int lgh_gauges_shape(lgh_ctx *c, int handle, long out[4])
{
   GaugeSet *s = gauge_set(c, handle, "lgh_gauges_shape");
   if (!s) { return LGH_ERR_ARG; }
   LGH_CHECK_ARG(out);
   int G;
   size_t bytes;
   gauge_shape(c, &G, &bytes);
   out[0] = G;
   out[1] = ceil_div(s->n, G);
   out[2] = (long)(G * bytes);
   out[3] = G * kWave;
   return LGH_OK;
}

int lgh_gauges_destroy(lgh_ctx *c, int handle)
{
   GaugeSet *s = gauge_set(c, handle, "lgh_gauges_destroy");
   if (!s) { return LGH_ERR_ARG; }
   LGH_HIP_CHECK(hipStreamSynchronize(c->stream)); // (a sample may still be on its way into the buffer)
   c->gauges[handle].reset();
   return LGH_OK;
}
}
