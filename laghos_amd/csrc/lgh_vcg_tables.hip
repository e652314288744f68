// lgh_vcg_tables.hip — the tables of the lockstep velocity solve (lgh_vcg.hip): the kernels that fill them, their host
// builders, the merged E-vector layout of the slab K1 and the solve's own zone / node order; VcgAux (lgh_vcg.hpp) is built
// here, published to the context when it is complete, and dropped here.
#include <memory>
#include "lgh_vcg.hpp"

namespace lgh
{

// ---- table kernels ------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
vcg_ellf_k(const int *__restrict__ ell, unsigned *__restrict__ ellf, const size_t n_have, const size_t n_all, const int ND, const int NE)
{
   const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
   if (i >= n_all) { return; }
   const int p = (i < n_have) ? ell[i] : -1; // e*ND + d
   const int e = p / ND;
   ellf[i] = 8u * (unsigned)(p < 0 ? kVC * ND * NE : kVC * ND * e + (p - e * ND));
}
__global__ void __launch_bounds__(256)
vcg_mapb_k(const int *__restrict__ map, unsigned *__restrict__ mapb, const size_t n)
{
   const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
   if (i < n) { mapb[i] = 8u * (unsigned)map[i]; }
}
// flag = 1 unless the D nodes of every x-row of every element are consecutive node numbers
__global__ void __launch_bounds__(256)
vcg_map_xrows_k(const int *__restrict__ map, const size_t nrows, const int D, int *flag)
{
   const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
   if (i >= nrows) { return; }
   const int *p = map + i * D;
   bool ok = true;
   for (int k = 1; k < D; k++) { ok = ok && p[k] == p[0] + k; }
   if (!ok) { *flag = 1; }
}
// ---- tables of the node kernel K2 ---------------------------------------------------------
__global__ void __launch_bounds__(256)
vcg_essbits_k(const uint8_t *e0, const uint8_t *e1, const uint8_t *e2, const uint8_t *hmask, const double *owner, uint8_t *bits,
              const int N)
{
   const int n = blockIdx.x * blockDim.x + threadIdx.x;
   if (n >= N) { return; }
   // bits 0-2: essential for component k; several ranks: bit 3 = shared with another rank (its A d comes halo-summed
   // from the L-vector), bit 4 = owned by another rank (weight 0 in the dot products)
   bits[n] = (uint8_t)(((e0 && e0[n]) ? 1 : 0) | ((e1 && e1[n]) ? 2 : 0) | ((e2 && e2[n]) ? 4 : 0) | ((hmask && hmask[n]) ? 8 : 0) |
                       ((owner && owner[n] == 0.0) ? 16 : 0));
}
__global__ void __launch_bounds__(256)
vcg_ellz_k(const int *__restrict__ ell, unsigned *__restrict__ ellz, const size_t n_have, const size_t n_all, const int zslot)
{
   const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
   if (i >= n_all) { return; }
   const int p = (i < n_have) ? ell[i] : -1; // rows beyond the mesh's valence: absent
   // in: slot-major (slot j of node n at j * N + n); out: two tables of four slots per node, [n][j] for j < 4 and, behind
   // it, [n][j - 4] for the rest (vcg_update_p_k reads a table entry as one 16-byte load)
   const size_t N = n_all / 8, j = i / N, n = i - j * N;
   ellz[(j < 4 ? 0 : 4 * N) + 4 * n + (j & 3)] = 8u * (unsigned)(p < 0 ? zslot : p);
}

// Node phase: a node costs a fixed part (its vectors, the ELL row) plus a part per element contribution
// (measured: t = 4.2..5.3 ns + 1.7..1.8 ns * valence per node and workgroup, the traces of the persistent-solve experiment, profiles/r2_pcg_trace_*.txt); with equal
// node counts the workgroups whose range covers element-boundary planes take 40 % longer and every barrier
// waits for them.  Ranges of equal cost instead, boundaries rounded to 16 nodes (128 B).
int partition_nodes_by_cost(lgh_ctx *c, const int W, DevPtr<int> &out, const std::vector<int> *valence)
{
   const int N = c->N;
   std::vector<int> off((size_t)N + 1);
   if (valence) // (the merged layout of the slab K1: contributions per node as THAT layout has them)
   {
      off[0] = 0;
      for (int n = 0; n < N; n++) { off[(size_t)n + 1] = off[n] + (*valence)[n]; }
   }
   else { LGH_HIP_CHECK(hipMemcpy(off.data(), c->t_off, off.size() * sizeof(int), hipMemcpyDeviceToHost)); }
   const long fixed = c->sw.k2_node_weight; // fixed part in units of half a contribution; <0: equal counts
   std::vector<long> cum((size_t)N + 1, 0);
   for (int n = 0; n < N; n++) { cum[(size_t)n + 1] = cum[n] + (fixed < 0 ? 1 : fixed + 2 * (long)(off[(size_t)n + 1] - off[n])); }
   std::vector<int> ns((size_t)std::max(W, 1) + 1, N);
   ns[0] = 0;
   int n = 0;
   for (int w = 1; w < W; w++)
   {
      const long target = cum[N] * w / W;
      while (n < N && cum[n] < target) { n++; }
      int nb = (n + 8) & ~15; // nearest multiple of 16
      nb = std::max(nb, ns[(size_t)w - 1]);
      ns[w] = std::min(nb, N);
   }
   ns[std::max(W, 1)] = N;
   return out.upload(ns.data(), ns.size());
}
// ELL transpose of the restriction as byte offsets into a Y_E plane of NE*ND + pad doubles whose slot NE*ND is
// zero: absent contributions point there, so the gather needs no predicate
int make_ellz(lgh_ctx *c, DevPtr<unsigned> &out, const int *ell, const int deg)
{
   const size_t ell_n = (size_t)8 * c->N;
   LGH_PASS(out.alloc(ell_n));
   hipLaunchKernelGGL(vcg_ellz_k, dim3((unsigned)((ell_n + 255) / 256)), dim3(256), 0, nullptr, ell ? ell : c->t_ell.p, out.p,
                      (size_t)(ell ? deg : c->t_deg) * c->N, ell_n, c->NE * c->ND);
   LGH_HIP_CHECK(hipGetLastError());
   return LGH_OK;
}

// ---- merged E-vector layout of the slab-form K1 (round 5) ---------------------------------------------------------
// K1 hands K2 the element contributions A_e d_e; in the element-local layout [e][dz][dy][dx] every node of an x-face
// between two zones travels twice (64 values per zone for 27 nodes) and a wavefront of K2 - consecutive nodes of an
// x-line - uses one y-row (32 bytes) of every 128-byte line it touches.  The slab K1 works on sets of five consecutive
// zones; where those are x-neighbours ("x-chain": zone i + 1's dx = 0 nodes ARE zone i's dx = 3 nodes, read off the
// element -> node map, nothing about the mesh is assumed) the set is stored as 16 rows (dz, dy) of the set's 16 x-nodes
// with the four shared faces summed by K1: 256 instead of 320 doubles per component, every row one cache line.  Sets
// that are not chains (a row of zones ends inside them; the short last set; any unstructured numbering) keep the
// element-local layout.  The plane of a component is the concatenation of the sets' slices; everything K2 and the
// several-rank gathers know about the layout is the ELL table built here.
//   pos[e * ND + d]: where the entry lives in a plane;  sec[...] = 1: the right-hand member of a merged pair
//   settab[s]: (offset of the set's slice / 64) | chain << 31
// x: the tables the layout is for (the map of the order the solve runs in: the caller's, or the library's own)
int slab_merge_layout(lgh_ctx *c, const VcgAux *x, SlabLayout &L)
{
   constexpr int ES = 5, D = 4, ND = 64;
   if (c->D1D != D || c->dim != 3) { set_error("slab_merge_layout: Q3 only"); return LGH_ERR_UNSUPPORTED; }
   const int NE = c->NE, nset = ceil_div(NE, ES);
   std::vector<int> map((size_t)NE * ND);
   LGH_HIP_CHECK(hipMemcpy(map.data(), x->o_map ? x->o_map : c->h1map, map.size() * sizeof(int), hipMemcpyDeviceToHost));
   L.settab.assign((size_t)nset, 0u);
   L.pos.assign((size_t)NE * ND, 0);
   L.sec.assign((size_t)NE * ND, 0);
   L.n_merged = 0;
   size_t off = 0; // doubles
   for (int s = 0; s < nset; s++)
   {
      const int e0 = ES * s, nel = std::min(ES, NE - e0);
      bool chain = (nel == ES);
      for (int i = 0; chain && i + 1 < ES; i++)
      {
         const int *ma = &map[(size_t)(e0 + i) * ND], *mb = &map[(size_t)(e0 + i + 1) * ND];
         for (int k = 0; chain && k < D * D; k++) { chain = (ma[D * k + (D - 1)] == mb[D * k]); }
      }
      if (off % 64 != 0 || off / 64 > 0x7fffffffull) { set_error("slab_merge_layout: plane offset out of range"); return LGH_ERR_UNSUPPORTED; }
      L.settab[s] = (unsigned)(off / 64) | (chain ? 0x80000000u : 0u);
      for (int i = 0; i < nel; i++)
      {
         for (int d = 0; d < ND; d++)
         {
            const size_t idx = (size_t)(e0 + i) * ND + d;
            if (!chain) { L.pos[idx] = (int)(off + (size_t)i * ND + d); continue; }
            const int dx = d % D, row = d / D; // row = dy + 4 dz
            L.pos[idx] = (int)(off + (size_t)row * 16 + 3 * i + dx);
            if (i > 0 && dx == 0) { L.sec[idx] = 1; L.n_merged++; }
         }
      }
      off += chain ? 256 : (size_t)nel * ND;
   }
   return LGH_OK;
}
// bit k of entry n: node n is essential for component k
int make_essbits(lgh_ctx *c, DevPtr<uint8_t> &out)
{
   LGH_PASS(out.alloc((size_t)c->N));
   const uint8_t *hmask = nullptr;
   const int *sh_node = nullptr;
   int n_shared = 0;
   if (c->multi) { comm_shared_nodes(c, &hmask, &sh_node, &n_shared); }
   hipLaunchKernelGGL(vcg_essbits_k, dim3((unsigned)((c->N + 255) / 256)), dim3(256), 0, nullptr, c->essmask[0], c->essmask[1],
                      c->essmask[2], hmask, c->multi ? c->owner.p : nullptr, out.p, c->N);
   LGH_HIP_CHECK(hipGetLastError());
   return LGH_OK;
}

// ---- VcgAux -------------------------------------------------------------------------------
// the tables of K2 (and of the several-rank gathers) for the merged layout: the ELL transpose with every merged pair as
// ONE entry, its byte-offset form, node ranges balanced by the contributions that are left
static int vcg_build_merged_tables(lgh_ctx *c, VcgAux *x)
{
   SlabLayout L;
   LGH_PASS(slab_merge_layout(c, x, L));
   const size_t N = (size_t)c->N;
   const int deg = c->t_deg;
   std::vector<int> ell((size_t)deg * N), ellm((size_t)8 * N, -1), val(N, 0);
   LGH_HIP_CHECK(hipMemcpy(ell.data(), x->o_ell ? x->o_ell : c->t_ell, ell.size() * sizeof(int), hipMemcpyDeviceToHost));
   int degm = 0;
   for (size_t n = 0; n < N; n++)
   {
      int cnt = 0;
      for (int j = 0; j < deg; j++)
      {
         const int p = ell[(size_t)j * N + n];
         if (p < 0 || L.sec[p]) { continue; } // (the right-hand member of a merged pair: summed into its partner's entry by K1)
         ellm[(size_t)cnt * N + n] = L.pos[p];
         cnt++;
      }
      val[n] = cnt;
      degm = std::max(degm, cnt);
   }
   x->degm = degm;
   LGH_PASS(x->settab.upload(L.settab.data(), L.settab.size()));
   LGH_PASS(x->ellm.upload(ellm.data(), ellm.size()));
   LGH_PASS(make_ellz(c, x->ellzm, x->ellm, 8));
   return partition_nodes_by_cost(c, x->grid2, x->nstartm, &val);
}

// The order the lockstep solve runs in: the library's own (lgh_order.hip) unless it is the caller's anyway.  Several ranks:
// every rank orders its own block; the node lists of the exchanges (lgh_comm.hip: the caller's numbering) are translated
// once (HaloNodeAlias) - which nodes travel, in which order and how they are summed does not depend on their numbers.
static const MeshOrder *vcg_order_for(const lgh_ctx *c)
{
   if (c->multi != 0 && !c->sw.order_multi) { return nullptr; } // (LGH_ORDER_MULTI=0, A/B: several ranks keep the caller's numbering in the solve)
   return mesh_order(c);
}
// Tables and vectors of the solve in the internal order (VcgAux::o_*): the element -> node map (internal zone i, internal
// node numbers), its transpose for the solve's own E-vector and for an E-vector in the caller's zone order, essential masks,
// room for 1/diag, the mass data and the solution.
static int vcg_build_internal_tables(lgh_ctx *c, VcgAux *x)
{
   const MeshOrder *o = x->ord;
   const size_t N = (size_t)c->N, NE = (size_t)c->NE, ND = (size_t)c->ND, nmap = NE * ND;
   const int deg = c->t_deg;
   std::vector<int> hm(nmap), om(nmap);
   LGH_HIP_CHECK(hipMemcpy(hm.data(), c->h1map, nmap * sizeof(int), hipMemcpyDeviceToHost));
   for (size_t i = 0; i < NE; i++)
   {
      const size_t e = (size_t)o->zorder[i];
      for (size_t d = 0; d < ND; d++) { om[i * ND + d] = o->nnum[hm[e * ND + d]]; }
   }
   LGH_PASS(x->o_map.upload(om.data(), nmap));
   // transpose, ascending E-position per node (as lgh_create builds the caller's)
   std::vector<int> off(N + 1, 0);
   for (size_t i = 0; i < nmap; i++) { off[(size_t)om[i] + 1]++; }
   x->o_valence.assign(N, 0);
   for (size_t n = 0; n < N; n++) { x->o_valence[n] = off[n + 1]; off[n + 1] += off[n]; }
   std::vector<int> pos(off.begin(), off.end() - 1), ell((size_t)deg * N, -1);
   for (size_t i = 0; i < nmap; i++)
   {
      const size_t n = (size_t)om[i];
      const int k = pos[n]++ - off[n];
      if (k >= deg) { set_error("vcg_build_internal_tables: valence above the mesh's"); return LGH_ERR_ARG; }
      ell[(size_t)k * N + n] = (int)i;
   }
   LGH_PASS(x->o_ell.upload(ell.data(), ell.size()));
   // the caller's transpose, rows taken in internal node order: positions in an E-vector of the CALLER's zone order, in the
   // caller's (ascending) order of contributions - the right-hand side has the bits of the unfused E -> L sum
   std::vector<int> tell((size_t)deg * N);
   LGH_HIP_CHECK(hipMemcpy(tell.data(), c->t_ell, tell.size() * sizeof(int), hipMemcpyDeviceToHost));
   for (int k = 0; k < deg; k++)
      for (size_t m = 0; m < N; m++) { ell[(size_t)k * N + m] = tell[(size_t)k * N + (size_t)o->ncaller[m]]; }
   LGH_PASS(x->o_ellc.upload(ell.data(), ell.size()));
   for (int k = 0; k < kVC; k++)
   {
      if (!c->essmask[k]) { continue; }
      LGH_PASS(x->o_ess[k].alloc(N));
      LGH_PASS(order_gather_bytes(c, c->essmask[k], x->o_ess[k]));
   }
   if (c->multi != 0)
   {
      if (c->owner)
      {
         LGH_PASS(x->o_owner.alloc(N));
         LGH_PASS(order_gather_nodes(c, c->owner, x->o_owner, 1));
      }
      const uint8_t *hmask = nullptr;
      const int *sh_node = nullptr, *nodes = nullptr;
      int n_shared = 0, total = 0;
      comm_shared_nodes(c, &hmask, &sh_node, &n_shared);
      if (hmask)
      {
         LGH_PASS(x->o_hmask.alloc(N));
         LGH_PASS(order_gather_bytes(c, hmask, x->o_hmask));
      }
      comm_node_lists(c, &nodes, &total, &sh_node, &n_shared);
      auto translate = [&](const int *src, const int n, DevPtr<int> &dst) -> int {
         std::vector<int> h((size_t)std::max(n, 1), 0);
         if (n > 0) { LGH_HIP_CHECK(hipMemcpy(h.data(), src, (size_t)n * sizeof(int), hipMemcpyDeviceToHost)); }
         for (int i = 0; i < n; i++) { h[i] = o->nnum[h[i]]; }
         return dst.upload(h.data(), h.size());
      };
      if (nodes && sh_node)
      {
         LGH_PASS(translate(nodes, total, x->o_nodes));
         LGH_PASS(translate(sh_node, n_shared, x->o_shnode));
         x->o_alias = {x->o_nodes, x->o_shnode};
      }
   }
   LGH_PASS(x->o_dinv.alloc(N));
   LGH_PASS(x->o_Se.alloc(NE));
   LGH_PASS(x->o_x.alloc(kVC * N, true));
   LGH_HIP_CHECK(hipStreamSynchronize(c->stream));
   x->o_mass_gen = ~0ul;
   return LGH_OK;
}

// The tables of a context, built on the first solve (or the first after the communicator has changed: lgh_comm_init /
// lgh_comm_set_neighbors drop them).  Built into a local owner and published as the last statement: an error on the way
// frees what exists and leaves c->vcg_aux null - the next call builds again.
int vcg_build_aux(lgh_ctx *c)
{
   std::unique_ptr<VcgAux> owner(new VcgAux());
   VcgAux *x = owner.get();
   // the CG's own E-vector (the force E-vector of the fused init stays in c->YE) and the tables of K2
   const size_t ye_n = (size_t)kVC * ((size_t)c->NE * c->ND + kYePad);
   LGH_PASS(x->ye.alloc(ye_n, true));
   // The library's own order of zones and nodes (lgh_order.hip), when the caller's is another one: the solve's tables are
   // built for THAT order.  (Several ranks: the exchange tables of lgh_comm.hip are in the caller's numbering - see
   // vcg_order_for.)
   x->ord = vcg_order_for(c);
   if (x->ord) { LGH_PASS(vcg_build_internal_tables(c, x)); }
   const int *v_map = x->o_map ? x->o_map : c->h1map;
   if (c->t_deg <= 8 && (size_t)c->N * 8 * kVC < 0xffffffffull && ((size_t)c->NE * c->ND + kYePad) * 8 < 0xffffffffull)
   {
      const int ncu = vcg_ncu(c);
      // node ranges (= workgroups) of vcg_update_p_k: four per CU, and not more than ~1000 nodes (two passes) each -
      // on large meshes long static ranges lose to the hardware's dynamic distribution of many short ones
      // (64^3 zones: 367 vs 424 us; 128^3: H1 CG 2.72 vs 3.04 s).  LGH_K2_GRID=<ranges per CU> for A/B.
      if (c->sw.k2_grid > 0) { x->grid2 = c->sw.k2_grid * ncu; }
      else { x->grid2 = (int)std::max<long>(4L * ncu, (((long)c->N + 1023) / 1024 + 7) & ~7L); }
      x->grid2 = std::min<long>(x->grid2, (long)c->vcg_stride - (long)kShards); // (one partial per workgroup in a reduction slot)
      LGH_PASS(make_ellz(c, x->ellz, x->o_ell, x->o_ell ? c->t_deg : 0));
      LGH_PASS(make_essbits(c, x->essbits));
      if (x->ord)
      {
         // (the flag bytes were built from the caller's masks: into the internal numbering)
         DevPtr<uint8_t> tmp;
         LGH_PASS(tmp.alloc((size_t)c->N));
         LGH_HIP_CHECK(hipStreamSynchronize(nullptr));
         LGH_PASS(order_gather_bytes(c, x->essbits, tmp));
         LGH_HIP_CHECK(hipStreamSynchronize(c->stream));
         x->essbits = std::move(tmp);
      }
      LGH_PASS(partition_nodes_by_cost(c, x->grid2, x->nstart, x->ord ? &x->o_valence : nullptr));
      if ((size_t)kVC * (c->NE + 1) * c->ND * 8 < 0xffffffffull)
      {
         // (the FORCE E-vector is in the caller's zone order: o_ellc)
         const size_t ell_n = (size_t)8 * c->N;
         LGH_PASS(x->ellf.alloc(ell_n));
         hipLaunchKernelGGL(vcg_ellf_k, dim3((unsigned)((ell_n + 255) / 256)), dim3(256), 0, nullptr, x->o_ellc ? x->o_ellc : c->t_ell, x->ellf,
                            (size_t)c->t_deg * c->N, ell_n, c->ND, c->NE);
         LGH_HIP_CHECK(hipGetLastError());
      }
   }
   if (vcg_resolve_k1(c).form == kK1Slab) // what the slab form reads: whoever dispatches it (vcg_resolve_k1) finds it here
   {
      const size_t nm = (size_t)c->NE * c->ND;
      LGH_PASS(x->mapb.alloc(nm));
      hipLaunchKernelGGL(vcg_mapb_k, dim3((unsigned)((nm + 255) / 256)), dim3(256), 0, nullptr, v_map, x->mapb, nm);
      LGH_HIP_CHECK(hipGetLastError());
      int *flag = (int *)c->scal.p, h = 1;
      LGH_HIP_CHECK(hipMemset(flag, 0, sizeof(int)));
      hipLaunchKernelGGL(vcg_map_xrows_k, dim3((unsigned)((nm / c->D1D + 255) / 256)), dim3(256), 0, nullptr, v_map, nm / c->D1D, c->D1D, flag);
      LGH_HIP_CHECK(hipMemcpy(&h, flag, sizeof(int), hipMemcpyDeviceToHost));
      x->map_xrows = (h == 0) ? 1 : 0;
      LGH_PASS(x->limbs.alloc(2 * kLimbWords + 8 * 16 + 32 * 4096, true)); // accumulators, set counters, queue
      LGH_PASS(x->rzl.alloc(3 * kLimbWords, true));
      // (LGH_SLAB_MERGE=0, A/B: element-local E-vector for every set, the layout of rounds 3 and 4)
      if (x->ellz && c->sw.slab_merge) { LGH_PASS(vcg_build_merged_tables(c, x)); }
   }
   LGH_HIP_CHECK(hipStreamSynchronize(nullptr)); // the fills run asynchronously on the null stream
   c->vcg_aux = std::move(owner);
   return LGH_OK;
}

void vcg_free(lgh_ctx *c)
{
   c->vcg_aux.reset();
}

} // namespace lgh
