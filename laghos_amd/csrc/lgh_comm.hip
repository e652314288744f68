// lgh_comm.hip — multi-GPU support: element blocks per rank, shared H1 nodes
// summed across ranks and scalar all-reduces, over the context's transport (RCCL on the
// context stream; lgh_comm_transport.hip).
//
// Replaces what the reference gets from MFEM's ParFiniteElementSpace /
// GroupCommunicator over MPI (call-site inventory in SURVEY §2): the conforming
// prolongation P^T (sum of shared dofs, inside mass->Mult laghos_assembly.cpp:119
// and Pconf->MultTranspose laghos_solver.cpp:368), CGSolver::Dot's MPI_Allreduce
// and the MIN reduction of the time-step estimate (laghos_solver.cpp:533).
//
// Every operation is written once: checks, choice of channel, pack, transport, combine.
// Pack and unpack-add are single kernels over all neighbours; how a message reaches the
// peer is the transport's business alone.
#include <unistd.h>
#include <cmath>

#include <algorithm>
#include <chrono>
#include <utility>

#include "lgh_comm_transport.hpp"

namespace lgh
{

// Buffers: neighbour k owns the contiguous block starting at base_k = 3*off_k +
// kHaloSlack*k: ncomp*cnt_k node values, component-major, then (optionally) nextra
// piggy-backed scalars - so every neighbour is ONE send and ONE recv.
// pos[j] = base_k + i for entry j = off_k + i of the concatenated node lists;
// cnt[j] = cnt_k.
// nextra > 0: the first n_nbr*nextra threads also put the piggy-backed scalars behind every
// neighbour's node block.
__global__ void __launch_bounds__(256)
halo_pack_k(const int total, const int ncomp, const int N, const int *__restrict__ nodes,
            const int *__restrict__ pos, const int *__restrict__ cnt, const double *__restrict__ v,
            double *__restrict__ buf, const int n_nbr, const int nextra, const int *__restrict__ base,
            const int *__restrict__ ncnt, const double *__restrict__ extra)
{
   const int i = blockIdx.x * blockDim.x + threadIdx.x;
   if (i < n_nbr * nextra)
   {
      const int k = i / nextra, e = i - k * nextra;
      buf[(size_t)base[k] + (size_t)ncomp * ncnt[k] + e] = extra[e];
   }
   if (i >= total * ncomp) { return; }
   const int c = i / total, j = i - c * total;
   buf[(size_t)pos[j] + (size_t)c * cnt[j]] = v[(size_t)c * N + nodes[j]];
}
// Canonical sum of a shared node: contributions are added in ascending rank
// order (own value at its rank's position), so every rank holding the node
// computes bit-identical results, as MFEM's GroupCommunicator does.  CSR over the
// unique shared nodes; src >= 0: entry j of the concatenated lists, -1: own value.
// nextra > 0: threads e < nextra of the launch also sum the piggy-backed scalars over all ranks in
// ascending rank order (own value at its rank's position): bit-identical on every rank.
__global__ void __launch_bounds__(256)
halo_combine_k(const int n_shared, const int ncomp, const int N, const int *__restrict__ sh_node,
               const int *__restrict__ sh_off, const int *__restrict__ sh_src,
               const int *__restrict__ pos, const int *__restrict__ cnt,
               const double *__restrict__ buf, double *__restrict__ v, const int nranks, const int nextra,
               const int *__restrict__ rank_src, const int *__restrict__ base, const int *__restrict__ ncnt,
               double *__restrict__ extra)
{
   const int i = blockIdx.x * blockDim.x + threadIdx.x;
   if (i < nextra)
   {
      double s = 0.0;
      for (int r = 0; r < nranks; r++)
      {
         const int k = rank_src[r];
         const double val = (k < 0) ? extra[i] : buf[(size_t)base[k] + (size_t)ncomp * ncnt[k] + i];
         s = (r == 0) ? val : s + val;
      }
      extra[i] = s;
   }
   if (i >= n_shared * ncomp) { return; }
   const int c = i / n_shared, u = i - c * n_shared;
   const int node = sh_node[u];
   double s = 0.0;
   for (int k = sh_off[u]; k < sh_off[u + 1]; k++)
   {
      const int j = sh_src[k];
      const double val = (j < 0) ? v[(size_t)c * N + node] : buf[(size_t)pos[j] + (size_t)c * cnt[j]];
      s = (k == sh_off[u]) ? val : s + val;
   }
   v[(size_t)c * N + node] = s;
}

bool halo_can_piggyback(const lgh_ctx *c)
{
   return c->sw.halo_piggyback && c->comm && c->comm->tab.allpairs;
}

// extra != nullptr (device, nextra <= 3 doubles, requires halo_can_piggyback): replaced
// by its sum over all ranks, carried by the same messages
// alias (optional): v is numbered otherwise than the caller's vectors (the velocity solve's own node numbering,
// lgh_order.hip) - the same node lists in THAT numbering; everything else of the exchange does not know about numbers
int halo_sum(lgh_ctx *c, double *v, int ncomp, double *extra, int nextra, bool packed, const HaloNodeAlias *alias)
{
   Comm *cm = c->comm.get();
   if (!cm || cm->tab.n_nbr == 0) { return LGH_OK; }
   const HaloTables &t = cm->tab;
   const int *const l_nodes = alias ? alias->nodes : t.nodes.p, *const l_sh_node = alias ? alias->sh_node : t.sh_node.p;
   if (ncomp > 3 || ncomp < 0 || (ncomp == 0 && !extra)) { set_error("halo_sum: bad ncomp"); return LGH_ERR_ARG; }
   if (extra && (!t.allpairs || nextra < 1 || nextra > kHaloSlack)) { set_error("halo_sum: cannot piggy-back"); return LGH_ERR_ARG; }
   const int nx = extra ? nextra : 0;
   const int ch = c->on_stream2 ? 1 : 0;
   if (ch && (!cm->channel2 || ncomp != 0)) { set_error("halo_sum: the second channel carries scalars only"); return LGH_ERR_ARG; }
   if (packed && ch) { set_error("halo_sum: pre-packed messages use the main channel"); return LGH_ERR_ARG; }
   if (!cm->transport) { set_error("halo_sum: neighbour lists without a communicator (lgh_comm_init)"); return LGH_ERR_COMM; }
   KtScope sample(c, LGH_KERNEL_HALO); // (sampling on: one event pair around pack + exchange + combine, closed on error returns too)
   // ncomp == 0 (v unused): the messages carry the scalars only - a sum over the ranks as one
   // exchange with every peer (allreduce_dev uses it in all-pairs partitions)
   if (!packed)
   {
      const long npack = std::max((long)t.total * ncomp, (long)t.n_nbr * nx);
      hipLaunchKernelGGL(halo_pack_k, dim3(ceil_div(npack, 256)), dim3(256), 0, c->stream, t.total,
                         ncomp, c->N, l_nodes, t.pos.p, t.cnt.p, v, t.sendbuf[ch].p, t.n_nbr, nx, t.d_base.p, t.d_cnt.p,
                         extra);
      LGH_HIP_CHECK(hipGetLastError());
   }
   LGH_PASS(cm->transport->exchange_blocks(c, ch, ncomp, nx));
   const long ncomb = std::max((long)t.n_shared * ncomp, (long)nx);
   hipLaunchKernelGGL(halo_combine_k, dim3(ceil_div(ncomb, 256)), dim3(256), 0,
                      c->stream, t.n_shared, ncomp, c->N, l_sh_node, t.sh_off.p, t.sh_src.p, t.pos.p,
                      t.cnt.p, t.recvbuf[ch].p, v, c->nranks, nx, t.rank_src.p, t.d_base.p, t.d_cnt.p, extra);
   LGH_HIP_CHECK(hipGetLastError());
   return LGH_OK;
}

// may the energy solve run its reductions on the context's second stream?
bool comm_second_channel(const lgh_ctx *c) { return c->comm && c->comm->channel2; }

bool comm_pack_tables(const lgh_ctx *c, HaloPackTables *t)
{
   const Comm *cm = c->comm.get();
   if (!cm || cm->tab.n_nbr == 0 || !cm->tab.sh_off || !cm->tab.sendbuf[0]) { return false; }
   t->sh_off = cm->tab.sh_off; t->sh_src = cm->tab.sh_src; t->pos = cm->tab.pos; t->cnt = cm->tab.cnt;
   t->base = cm->tab.d_base; t->ncnt = cm->tab.d_cnt; t->sbuf = cm->tab.sendbuf[0]; t->n_nbr = cm->tab.n_nbr;
   return true;
}

// the node lists of the exchanges (device, the caller's numbering): concatenated neighbour lists, unique shared nodes
void comm_node_lists(const lgh_ctx *c, const int **nodes, int *total, const int **sh_node, int *n_shared)
{
   const Comm *cm = c->comm.get();
   *nodes = cm ? cm->tab.nodes.p : nullptr;
   *total = cm ? cm->tab.total : 0;
   *sh_node = cm ? cm->tab.sh_node.p : nullptr;
   *n_shared = (cm && cm->tab.sh_node) ? cm->tab.n_shared : 0;
}
// neighbours of lower rank, or -1 when the neighbour list is not in ascending rank order (a sum "own value between the
// lower and the higher peers' blocks" is then not the rank-ordered sum every rank must form alike)
int comm_ranks_before(const lgh_ctx *c)
{
   const Comm *cm = c->comm.get();
   int n = 0;
   if (cm)
   {
      for (int k = 0; k < cm->tab.n_nbr; k++)
      {
         if (k > 0 && cm->tab.nbr_rank[k] <= cm->tab.nbr_rank[k - 1]) { return -1; }
         n += (cm->tab.nbr_rank[k] < c->rank) ? 1 : 0;
      }
   }
   return n;
}
void comm_shared_nodes(const lgh_ctx *c, const uint8_t **hmask, const int **sh_node, int *n_shared)
{
   const Comm *cm = c->comm.get();
   *hmask = cm ? cm->tab.hmask.p : nullptr;
   *sh_node = cm ? cm->tab.sh_node.p : nullptr;
   *n_shared = (cm && cm->tab.hmask) ? cm->tab.n_shared : 0;
}

int comm_word_peers(lgh_ctx *c, int nwords, const long long **peers, int *n_peers)
{
   Comm *cm = c->comm.get();
   *peers = nullptr;
   *n_peers = 0;
   if (!cm || cm->tab.n_nbr == 0) { return LGH_OK; } // (a communicator of size 1: nobody to hear from)
   const int n_nbr = cm->tab.n_nbr;
   if (!cm->tab.allpairs) { set_error("comm_word_peers: all-pairs partitions only"); return LGH_ERR_ARG; }
   if (cm->wordcap != nwords || cm->wordnbr != n_nbr) // (sized by BOTH factors)
   {
      cm->wordcap = 0;
      LGH_PASS(cm->wordbuf.alloc((size_t)n_nbr * nwords, true));
      cm->wordcap = nwords;
      cm->wordnbr = n_nbr;
   }
   *peers = cm->wordbuf;
   *n_peers = n_nbr;
   return LGH_OK;
}

int exchange_words(lgh_ctx *c, const long long *src, int nwords)
{
   Comm *cm = c->comm.get();
   if (!cm || cm->tab.n_nbr == 0) { return LGH_OK; }
   if (!cm->tab.allpairs || !cm->wordbuf || cm->wordcap != nwords || cm->wordnbr != cm->tab.n_nbr || c->on_stream2) { set_error("exchange_words: all-pairs partition, main channel, peer buffer of %d words", nwords); return LGH_ERR_ARG; }
   if (!cm->transport) { set_error("exchange_words: neighbour lists without a communicator (lgh_comm_init)"); return LGH_ERR_COMM; }
   KtScope sample(c, LGH_KERNEL_ALLREDUCE); // (counted with the small sums it replaces)
   return cm->transport->exchange_words(c, src, nwords);
}

int allreduce_dev(lgh_ctx *c, double *dev, int count, int op, bool packed)
{
   Comm *cm = c->comm.get();
   // Sums of up to three scalars in an all-pairs partition (the CG dot products on <= 2x2x2 ranks):
   // one grouped exchange with every peer and a sum in rank order, the transport of the halo
   // messages, instead of a ring / tree all-reduce - one hop, bit-identical on every rank.
   if (op == 0 && count >= 1 && count <= 3 && cm && cm->tab.n_nbr > 0 && halo_can_piggyback(c))
   {
      return halo_sum(c, nullptr, 0, dev, count, packed && !c->on_stream2);
   }
   if (packed) { set_error("allreduce_dev: pre-packed sums need the all-pairs exchange"); return LGH_ERR_ARG; }
   if (!cm || !cm->transport) { return LGH_OK; }
   return cm->transport->allreduce(c, c->on_stream2 ? 1 : 0, dev, count, op);
}

// Any number of values, in pieces of what the transport takes at a time
int allreduce_dev_n(lgh_ctx *c, double *dev, long count, int op)
{
   const Comm *cm = c->comm.get();
   const long piece = (cm && cm->transport) ? cm->transport->allreduce_max() : (1L << 24);
   for (long i = 0; i < count; i += piece)
   {
      const long n = std::min(piece, count - i);
      const int rc = allreduce_dev(c, dev + i, (int)n, op);
      if (rc) { return rc; }
   }
   return LGH_OK;
}

// at least one element is allocated: an empty list still has an address the kernels may be handed
template <typename T> static int upload_list(DevPtr<T> &d, const std::vector<T> &h)
{
   LGH_PASS(d.alloc(std::max<size_t>(h.size(), 1)));
   if (!h.empty()) { LGH_HIP_CHECK(hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice)); }
   return LGH_OK;
}

// The tables of one lgh_comm_set_neighbors call, built into t - an object of the caller's, published only when every rank
// has built its own.  t.allpairs is this rank's view (the ranks agree on it afterwards); rank_src (per rank: neighbour
// index, -1 for this rank) is uploaded after that agreement.  Requires the rank: lgh_comm_init comes first.
static int build_tables(const lgh_ctx *c, const bool channel2, const int n_nbr, const int *nbr_rank, const int *nbr_count,
                        const int *const *nbr_nodes, HaloTables &t, std::vector<int> &rank_src)
{
   LGH_CHECK_ARG(n_nbr == 0 || (nbr_rank && nbr_count && nbr_nodes));
   if (n_nbr == 0 && c->nranks > 1)
   {
      // every exchange is a rendezvous of all ranks (process-wide barriers on the loopback transports): a rank of a
      // connected partition always has a neighbour, and one without would return from halo_sum before the others arrive
      set_error("lgh_comm_set_neighbors: rank %d of %d has no neighbour (disconnected partition)", c->rank, c->nranks);
      return LGH_ERR_ARG;
   }
   for (int k = 0; k < n_nbr; k++)
   {
      LGH_CHECK_ARG(nbr_count[k] >= 0 && (nbr_count[k] == 0 || nbr_nodes[k]));
      for (int i = 0; i < nbr_count[k]; i++)
      {
         if (nbr_nodes[k][i] < 0 || nbr_nodes[k][i] >= c->N) { set_error("neighbour node out of range"); return LGH_ERR_ARG; }
      }
   }
   t.n_nbr = n_nbr;
   t.nbr_rank.assign(nbr_rank, nbr_rank + n_nbr);
   t.nbr_count.assign(nbr_count, nbr_count + n_nbr);
   t.nbr_off.resize(n_nbr);
   t.nbr_base.resize(n_nbr);
   std::vector<int> all;
   int tot = 0;
   for (int k = 0; k < n_nbr; k++)
   {
      t.nbr_off[k] = tot;
      t.nbr_base[k] = 3 * tot + kHaloSlack * k;
      all.insert(all.end(), nbr_nodes[k], nbr_nodes[k] + nbr_count[k]);
      tot += nbr_count[k];
   }
   t.total = tot;
   // canonical-order combine lists
   {
      std::vector<std::vector<std::pair<int, int>>> per_node; // (rank, recv index)
      std::vector<int> uniq;
      std::vector<int> slot((size_t)c->N, -1);
      for (int k = 0; k < n_nbr; k++)
      {
         for (int i = 0; i < nbr_count[k]; i++)
         {
            const int n = nbr_nodes[k][i];
            if (slot[n] < 0)
            {
               slot[n] = (int)uniq.size();
               uniq.push_back(n);
               per_node.emplace_back();
               per_node.back().push_back({c->rank, -1});
            }
            per_node[slot[n]].push_back({nbr_rank[k], t.nbr_off[k] + i});
         }
      }
      std::vector<int> off(uniq.size() + 1, 0), src;
      for (size_t u = 0; u < uniq.size(); u++)
      {
         std::sort(per_node[u].begin(), per_node[u].end());
         for (auto &pr : per_node[u]) { src.push_back(pr.second); }
         off[u + 1] = (int)src.size();
      }
      t.n_shared = (int)uniq.size();
      LGH_PASS(upload_list(t.sh_node, uniq));
      LGH_PASS(upload_list(t.sh_off, off));
      LGH_PASS(upload_list(t.sh_src, src));
      std::vector<uint8_t> hm((size_t)c->N, 0);
      for (int n : uniq) { hm[n] = 1; }
      LGH_PASS(upload_list(t.hmask, hm));
   }
   {
      std::vector<int> pos(std::max(tot, 1)), cnt(std::max(tot, 1));
      for (int k = 0; k < n_nbr; k++)
      {
         for (int i = 0; i < nbr_count[k]; i++)
         {
            pos[t.nbr_off[k] + i] = t.nbr_base[k] + i;
            cnt[t.nbr_off[k] + i] = nbr_count[k];
         }
      }
      LGH_PASS(upload_list(t.pos, pos));
      LGH_PASS(upload_list(t.cnt, cnt));
   }
   LGH_PASS(upload_list(t.nodes, all));
   t.bufsize = 3 * std::max(tot, 1) + kHaloSlack * n_nbr;
   for (int ch = 0; ch < (channel2 ? 2 : 1); ch++)
   {
      LGH_PASS(t.sendbuf[ch].alloc((size_t)t.bufsize, true));
      LGH_PASS(t.recvbuf[ch].alloc((size_t)t.bufsize, true));
   }
   LGH_HIP_CHECK(hipStreamSynchronize(nullptr)); // the fills run asynchronously on the null stream
   // the rank -> neighbour map of the piggy-backed scalars; all-pairs: every other rank is a neighbour
   rank_src.assign((size_t)std::max(c->nranks, 1), -2);
   rank_src[c->rank] = -1;
   for (int k = 0; k < n_nbr; k++)
   {
      if (nbr_rank[k] >= 0 && nbr_rank[k] < c->nranks) { rank_src[nbr_rank[k]] = k; }
   }
   t.allpairs = (n_nbr > 0 && n_nbr == c->nranks - 1);
   for (int r : rank_src) { if (r == -2) { t.allpairs = false; } }
   return LGH_OK;
}

} // namespace lgh

using namespace lgh;

extern "C"
{

int lgh_comm_unique_id(char id_out[128])
{
   LGH_CHECK_ARG(id_out);
   return rccl_unique_id(id_out);
}

int lgh_comm_unique_id_shm(char id_out[128])
{
   LGH_CHECK_ARG(id_out);
   memset(id_out, 0, 128);
   unsigned long long r = (unsigned long long)getpid() * 0x9E3779B97F4A7C15ull ^ (unsigned long long)std::chrono::steady_clock::now().time_since_epoch().count();
   snprintf(id_out, 64, "LGHSHM_%d_%016llx", (int)getpid(), r);
   return LGH_OK;
}

int lgh_comm_init(lgh_ctx *c, int nranks, int rank, const char unique_id[128])
{
   LGH_CHECK_ARG(c && nranks >= 1 && rank >= 0 && rank < nranks && unique_id);
   if (c->dim == 1)
   {
      set_error("lgh_comm_init: a 1D context runs on one rank (several ranks are not supported in 1D)");
      return LGH_ERR_UNSUPPORTED;
   }
   if (!c->comm) { c->comm.reset(new Comm()); }
   OpenedTransport o;
   if (memcmp(unique_id, "LGHSHM", 6) == 0) { LGH_PASS(open_shm(c, nranks, rank, unique_id, o)); } // cross-process loopback (bench.py --transport shm, tests)
   else if (memcmp(unique_id, "LGHLOCAL", 8) == 0) { LGH_PASS(open_local(c, nranks, rank, unique_id, o)); } // in-process loopback (tests)
   else { LGH_PASS(open_rccl(c, nranks, rank, unique_id, o)); }
   c->comm->transport = std::move(o.transport);
   c->comm->channel2 = o.channel2;
   c->nranks = nranks;
   c->rank = rank;
   c->multi = o.multi;
   vcg_free(c); // the tables of the node kernel K2 carry the shared-node / owner flags of the previous communicator
   return c->comm->transport->rendezvous(nranks);
}

int lgh_comm_stats(lgh_ctx *c, int *n_neighbours, long *max_nodes_per_neighbour, long *shared_nodes, int *all_pairs, int *second_channel)
{
   LGH_CHECK_ARG(c && n_neighbours && max_nodes_per_neighbour && shared_nodes && all_pairs && second_channel);
   const Comm *cm = c->comm.get();
   *n_neighbours = cm ? cm->tab.n_nbr : 0;
   long mx = 0;
   if (cm) { for (int k = 0; k < cm->tab.n_nbr; k++) { mx = std::max(mx, (long)cm->tab.nbr_count[k]); } }
   *max_nodes_per_neighbour = mx;
   *shared_nodes = cm ? cm->tab.n_shared : 0;
   *all_pairs = (cm && cm->tab.allpairs) ? 1 : 0;
   *second_channel = (cm && cm->channel2) ? 1 : 0;
   return LGH_OK;
}

int lgh_comm_set_neighbors(lgh_ctx *c, int n_nbr, const int *nbr_rank, const int *nbr_count,
                           const int *const *nbr_nodes)
{
   LGH_CHECK_ARG(c && n_nbr >= 0);
   if (!c->comm) { c->comm.reset(new Comm()); }
   Comm *cm = c->comm.get();
   // Everything that can fail locally (argument checks, allocations) runs first and its status is folded
   // into the collective below: a rank that fails must not leave its peers blocked in the all-reduce.
   HaloTables t;
   std::vector<int> rank_src;
   const int rc_local = build_tables(c, cm->channel2, n_nbr, nbr_rank, nbr_count, nbr_nodes, t, rank_src);
   if (cm->transport) { LGH_PASS(cm->transport->publish_tables(c->rank, rc_local ? nullptr : &t)); }
   // the message sizes depend on it: every rank must come to the same decision (in a 3x1x1 partition
   // only the middle rank sees all others); a local failure travels in the same MIN-reduction
   if (c->multi != 0 && cm->transport)
   {
      double flag = rc_local ? -1.0 : (t.allpairs ? 1.0 : 0.0);
      LGH_PASS(lgh_allreduce(c, &flag, 1));
      if (flag < 0.0)
      {
         if (!rc_local) { set_error("lgh_comm_set_neighbors failed on another rank"); }
         return rc_local ? rc_local : LGH_ERR_COMM;
      }
      t.allpairs = (flag > 0.5);
   }
   else if (rc_local) { return rc_local; }
   LGH_PASS(upload_list(t.d_base, t.nbr_base));
   LGH_PASS(upload_list(t.d_cnt, t.nbr_count));
   LGH_PASS(upload_list(t.rank_src, rank_src));
   // Publication: the tables change hands whole (the previous ones leave with t), and what was built for them goes -
   // the peer buffer of exchange_words, sized by the neighbour count, and the flag bytes of the node kernel K2
   cm->tab = std::move(t);
   cm->wordbuf.reset();
   cm->wordcap = 0;
   cm->word_src = nullptr;
   vcg_free(c);
   return LGH_OK;
}

int lgh_test_set_rank(lgh_ctx *c, int nranks, int rank)
{
   LGH_CHECK_ARG(c && nranks >= 1 && rank >= 0 && rank < nranks);
   c->nranks = nranks;
   c->rank = rank;
   return LGH_OK;
}
int lgh_test_word_peers(lgh_ctx *c, int nwords, long *capacity_words)
{
   LGH_CHECK_ARG(c && nwords > 0 && capacity_words);
   const long long *peers = nullptr;
   int n_peers = 0;
   const int rc = comm_word_peers(c, nwords, &peers, &n_peers);
   if (rc) { return rc; }
   const Comm *cm = c->comm.get();
   *capacity_words = (cm && cm->wordbuf) ? (long)cm->wordnbr * cm->wordcap : 0;
   if (peers) { LGH_HIP_CHECK(hipMemset((void *)peers, 0, (size_t)n_peers * nwords * sizeof(long long))); } // (writes the whole buffer: a short one faults here)
   return (cm && cm->wordbuf && cm->wordnbr == n_peers && cm->wordcap == nwords) || n_peers == 0 ? LGH_OK : LGH_ERR_COMM;
}
int lgh_test_halo_pack(lgh_ctx *c, const double *v, int ncomp, double *out)
{
   LGH_CHECK_ARG(c && v && out && c->comm && ncomp >= 1 && ncomp <= 3);
   const HaloTables &t = c->comm->tab;
   if (t.total == 0) { return LGH_OK; }
   hipLaunchKernelGGL(halo_pack_k, dim3(ceil_div((long)t.total * ncomp, 256)), dim3(256), 0, c->stream,
                      t.total, ncomp, c->N, t.nodes.p, t.pos.p, t.cnt.p, v, t.sendbuf[0].p, 0, 0, nullptr, nullptr, nullptr);
   LGH_HIP_CHECK(hipGetLastError());
   LGH_HIP_CHECK(hipMemcpyAsync(out, t.sendbuf[0], (size_t)t.bufsize * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
   return LGH_OK;
}
int lgh_test_halo_combine(lgh_ctx *c, const double *in, double *v, int ncomp)
{
   LGH_CHECK_ARG(c && v && in && c->comm && ncomp >= 1 && ncomp <= 3);
   const HaloTables &t = c->comm->tab;
   if (t.total == 0) { return LGH_OK; }
   LGH_HIP_CHECK(hipMemcpyAsync(t.recvbuf[0], in, (size_t)t.bufsize * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
   hipLaunchKernelGGL(halo_combine_k, dim3(ceil_div((long)t.n_shared * ncomp, 256)), dim3(256), 0, c->stream,
                      t.n_shared, ncomp, c->N, t.sh_node.p, t.sh_off.p, t.sh_src.p, t.pos.p, t.cnt.p,
                      t.recvbuf[0].p, v, c->nranks, 0, nullptr, nullptr, nullptr, nullptr);
   LGH_HIP_CHECK(hipGetLastError());
   return LGH_OK;
}

// Probe of the transport used by halo_sum on the REAL communicator (not the loopback one):
// a grouped ncclSend / ncclRecv of n doubles from this rank to itself, the only
// peer a one-GPU box offers.  *max_abs_diff = max |received - sent|.
int lgh_test_rccl_self_sendrecv(lgh_ctx *c, int n, double *max_abs_diff)
{
   LGH_CHECK_ARG(c && n > 0 && max_abs_diff);
   std::vector<double> h(2 * (size_t)n, 0.0);
   for (int i = 0; i < n; i++) { h[i] = 1.0 + 0.5 * i; }
   DevPtr<double> buf;
   LGH_PASS(buf.upload(h.data(), h.size()));
   LGH_PASS(rccl_self_sendrecv(c, buf, n));
   LGH_HIP_CHECK(hipStreamSynchronize(c->stream));
   LGH_HIP_CHECK(hipMemcpy(h.data(), buf, h.size() * sizeof(double), hipMemcpyDeviceToHost));
   double d = 0.0;
   for (int i = 0; i < n; i++) { d = std::max(d, std::fabs(h[(size_t)n + i] - h[i])); }
   *max_abs_diff = d;
   return LGH_OK;
}

int lgh_groups_to_neighbors(int my_rank, int N, int n_groups, const int *group_off, const int *group_ranks,
                            const int *group_master, const int *ldof_off, const int *ldofs, double *owner,
                            int *n_nbr, int *nbr_rank, int *nbr_count, int cap_nbr, int *nbr_nodes, long cap_nodes)
{
   LGH_CHECK_ARG(my_rank >= 0 && N >= 0 && n_groups >= 0 && owner && n_nbr);
   LGH_CHECK_ARG(n_groups == 0 || (group_off && group_ranks && ldof_off && ldofs));
   for (int i = 0; i < N; i++) { owner[i] = 1.0; }
   // groups ordered by their sorted rank sets: the same sequence on every member
   std::vector<std::vector<int>> sets((size_t)n_groups);
   std::vector<int> order((size_t)n_groups);
   for (int g = 0; g < n_groups; g++)
   {
      LGH_CHECK_ARG(group_off[g + 1] - group_off[g] >= 2 && ldof_off[g + 1] >= ldof_off[g]);
      sets[g].assign(group_ranks + group_off[g], group_ranks + group_off[g + 1]);
      std::sort(sets[g].begin(), sets[g].end());
      if (std::adjacent_find(sets[g].begin(), sets[g].end()) != sets[g].end() ||
          !std::binary_search(sets[g].begin(), sets[g].end(), my_rank) || sets[g].front() < 0)
      {
         set_error("lgh_groups_to_neighbors: group %d must list distinct ranks including this one", g);
         return LGH_ERR_ARG;
      }
      order[g] = g;
      const int master = group_master ? group_master[g] : sets[g].front();
      if (!std::binary_search(sets[g].begin(), sets[g].end(), master)) { set_error("lgh_groups_to_neighbors: master of group %d is not a member", g); return LGH_ERR_ARG; }
      for (int k = ldof_off[g]; k < ldof_off[g + 1]; k++)
      {
         if (ldofs[k] < 0 || ldofs[k] >= N) { set_error("lgh_groups_to_neighbors: dof out of range in group %d", g); return LGH_ERR_ARG; }
         if (master != my_rank) { owner[ldofs[k]] = 0.0; }
      }
   }
   std::sort(order.begin(), order.end(), [&](int a, int b) { return sets[a] < sets[b]; });
   for (int i = 0; i + 1 < n_groups; i++)
   {
      if (sets[order[i]] == sets[order[i + 1]]) { set_error("lgh_groups_to_neighbors: two groups with the same rank set"); return LGH_ERR_ARG; }
   }
   std::vector<int> peers;
   for (int g = 0; g < n_groups; g++) { for (int r : sets[g]) { if (r != my_rank) { peers.push_back(r); } } }
   std::sort(peers.begin(), peers.end());
   peers.erase(std::unique(peers.begin(), peers.end()), peers.end());
   if ((int)peers.size() > cap_nbr) { set_error("lgh_groups_to_neighbors: %d peers, room for %d", (int)peers.size(), cap_nbr); return LGH_ERR_ARG; }
   LGH_CHECK_ARG(peers.empty() || (nbr_rank && nbr_count && nbr_nodes));
   long pos = 0;
   for (size_t k = 0; k < peers.size(); k++)
   {
      nbr_rank[k] = peers[k];
      int cnt = 0;
      for (int i = 0; i < n_groups; i++)
      {
         const int g = order[i];
         if (!std::binary_search(sets[g].begin(), sets[g].end(), peers[k])) { continue; }
         const int nd = ldof_off[g + 1] - ldof_off[g];
         if (pos + nd > cap_nodes) { set_error("lgh_groups_to_neighbors: node list capacity %ld too small", cap_nodes); return LGH_ERR_ARG; }
         for (int j = 0; j < nd; j++) { nbr_nodes[pos + j] = ldofs[ldof_off[g] + j]; }
         pos += nd;
         cnt += nd;
      }
      nbr_count[k] = cnt;
   }
   *n_nbr = (int)peers.size();
   return LGH_OK;
}

int lgh_halo_sum(lgh_ctx *c, double *v_h1, int ncomp)
{
   LGH_CHECK_ARG(c && v_h1 && ncomp >= 1 && ncomp <= 3);
   return halo_sum(c, v_h1, ncomp, nullptr, 0);
}

int lgh_allreduce(lgh_ctx *c, double *value, int op)
{
   LGH_CHECK_ARG(c && value);
   if (!c->multi || !c->comm) { return LGH_OK; }
   // through the pinned staging area: an async copy from pageable memory is not ordered
   // with the stream
   c->host_pinned[kPinReduceIn] = *value;
   LGH_HIP_CHECK(hipMemcpyAsync(c->scal + 2, c->host_pinned + kPinReduceIn, sizeof(double), hipMemcpyHostToDevice, c->stream));
   int rc = allreduce_dev(c, c->scal + 2, 1, op);
   if (rc) { return rc; }
   LGH_HIP_CHECK(hipMemcpyAsync(c->host_pinned + kPinReduceOut, c->scal + 2, sizeof(double), hipMemcpyDeviceToHost, c->stream));
   LGH_HIP_CHECK(hipStreamSynchronize(c->stream));
   *value = c->host_pinned[kPinReduceOut];
   return LGH_OK;
}

} // extern "C"
