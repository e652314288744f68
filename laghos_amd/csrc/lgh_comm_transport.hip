// lgh_comm_transport.hip — how the messages of lgh_comm.hip travel: RCCL on the context stream (the product), and the two
// loop-backs that let several ranks run on one GPU (test vehicles).
//
// MI355X design: xGMI is point-to-point, and a 2x2x2 block partition gives every
// GPU 7 neighbours = its 7 links, so the halo is one grouped ncclSend/ncclRecv
// per neighbour (<= 75 KB each at 32^3 Q3 elements) rather than a ring collective.
// RCCL is resolved with dlopen at lgh_comm_init time so that the same library
// loads on a host without RCCL (and reuses torch's copy when already loaded).
#include <dlfcn.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <cstdlib>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <map>
#include <memory>
#include <mutex>
#include <string>

#include "lgh_comm_transport.hpp"

namespace lgh
{

// ---- RCCL ---------------------------------------------------------------------------------------------------------
// minimal NCCL ABI (rccl.h): opaque handles + the enums used here
typedef struct ncclComm *ncclComm_t;
typedef struct { char internal[128]; } ncclUniqueId;
enum { ncclSuccess = 0 };
enum { ncclFloat64 = 8 };
enum { ncclSum = 0, ncclMin = 3 };

struct NcclApi
{
   void *lib = nullptr;
   int (*GetUniqueId)(ncclUniqueId *) = nullptr;
   int (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
   int (*CommDestroy)(ncclComm_t) = nullptr;
   int (*AllReduce)(const void *, void *, size_t, int, int, ncclComm_t, hipStream_t) = nullptr;
   int (*Broadcast)(const void *, void *, size_t, int, int, ncclComm_t, hipStream_t) = nullptr; // optional
   int (*Send)(const void *, size_t, int, int, ncclComm_t, hipStream_t) = nullptr;
   int (*Recv)(void *, size_t, int, int, ncclComm_t, hipStream_t) = nullptr;
   int (*GroupStart)() = nullptr;
   int (*GroupEnd)() = nullptr;
   const char *(*GetErrorString)(int) = nullptr;
};
static NcclApi g_nccl;

static int load_nccl()
{
   if (g_nccl.lib) { return LGH_OK; }
   const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
   void *h = nullptr;
   for (const char *n : names) { h = dlopen(n, RTLD_NOW | RTLD_NOLOAD); if (h) { break; } }
   if (!h) { for (const char *n : names) { h = dlopen(n, RTLD_NOW | RTLD_LOCAL); if (h) { break; } } }
   if (!h)
   {
      set_error("cannot load RCCL: %s", dlerror());
      return LGH_ERR_COMM;
   }
   g_nccl.lib = h;
#define LGH_SYM(field, name)                                                        \
   *(void **)(&g_nccl.field) = dlsym(h, name);                                     \
   if (!g_nccl.field) { set_error("RCCL symbol %s missing", name); g_nccl.lib = nullptr; return LGH_ERR_COMM; }
   LGH_SYM(GetUniqueId, "ncclGetUniqueId");
   LGH_SYM(CommInitRank, "ncclCommInitRank");
   LGH_SYM(CommDestroy, "ncclCommDestroy");
   LGH_SYM(AllReduce, "ncclAllReduce");
   LGH_SYM(Send, "ncclSend");
   LGH_SYM(Recv, "ncclRecv");
   LGH_SYM(GroupStart, "ncclGroupStart");
   LGH_SYM(GroupEnd, "ncclGroupEnd");
   LGH_SYM(GetErrorString, "ncclGetErrorString");
#undef LGH_SYM
   *(void **)(&g_nccl.Broadcast) = dlsym(h, "ncclBroadcast");
   return LGH_OK;
}

#define LGH_NCCL_CHECK(expr)                                                             \
   do                                                                                    \
   {                                                                                     \
      int r_ = (expr);                                                                   \
      if (r_ != ncclSuccess)                                                             \
      {                                                                                  \
         set_error("RCCL error %s at %s:%d", g_nccl.GetErrorString(r_), __FILE__, __LINE__); \
         return LGH_ERR_COMM;                                                            \
      }                                                                                  \
   } while (0)

struct RcclTransport : Transport
{
   ncclComm_t comm[2] = {nullptr, nullptr}; // per channel: one communicator must not be driven from two streams
   ~RcclTransport() override
   {
      if (comm[1]) { g_nccl.CommDestroy(comm[1]); }
      if (comm[0]) { g_nccl.CommDestroy(comm[0]); }
   }
   int exchange_blocks(lgh_ctx *c, int ch, int ncomp, int nextra) override
   {
      const HaloTables &t = c->comm->tab;
      LGH_NCCL_CHECK(g_nccl.GroupStart());
      for (int k = 0; k < t.n_nbr; k++)
      {
         const size_t o = (size_t)t.nbr_base[k], n = t.block_len(k, ncomp, nextra);
         LGH_NCCL_CHECK(g_nccl.Send(t.sendbuf[ch] + o, n, ncclFloat64, t.nbr_rank[k], comm[ch], c->stream));
         LGH_NCCL_CHECK(g_nccl.Recv(t.recvbuf[ch] + o, n, ncclFloat64, t.nbr_rank[k], comm[ch], c->stream));
      }
      LGH_NCCL_CHECK(g_nccl.GroupEnd());
      return LGH_OK;
   }
   int exchange_words(lgh_ctx *c, const long long *src, int nwords) override
   {
      const Comm *cm = c->comm.get();
      LGH_NCCL_CHECK(g_nccl.GroupStart());
      for (int k = 0; k < cm->tab.n_nbr; k++)
      {
         // (send / recv move bytes: the words travel under the 8-byte type the halo messages already use)
         LGH_NCCL_CHECK(g_nccl.Send(src, (size_t)nwords, ncclFloat64, cm->tab.nbr_rank[k], comm[0], c->stream));
         LGH_NCCL_CHECK(g_nccl.Recv(cm->wordbuf + (size_t)k * nwords, (size_t)nwords, ncclFloat64, cm->tab.nbr_rank[k], comm[0], c->stream));
      }
      LGH_NCCL_CHECK(g_nccl.GroupEnd());
      return LGH_OK;
   }
   int allreduce(lgh_ctx *c, int ch, double *dev, int count, int op) override
   {
      if (ch && !comm[1]) { set_error("all-reduce on the second stream without a second communicator"); return LGH_ERR_COMM; }
      kt_begin(c, LGH_KERNEL_ALLREDUCE);
      LGH_NCCL_CHECK(g_nccl.AllReduce(dev, dev, (size_t)count, ncclFloat64, op == 0 ? ncclSum : ncclMin, comm[ch], c->stream));
      kt_end(c, LGH_KERNEL_ALLREDUCE);
      return LGH_OK;
   }
   long allreduce_max() const override { return 1L << 24; }
};

// Second communicator (same ranks) for the second stream, so that the energy solve can run beside the velocity solve
// on several ranks too.  Its id is drawn by rank 0 and travels over the first one TOGETHER with rank 0's verdict (a
// rank that got no id must not leave the others blocked in CommInitRank); the outcome is then agreed on by a MIN over
// the ranks, so either every rank has the channel or none does.
// Two communicators driven from two streams of one device have only ever run on a communicator of size 1 and on the
// in-process loopback here (no multi-GPU box): collectives of different communicators that the ranks happen to
// schedule in different orders can block each other.  Until a real multi-GPU run has validated it, the channel is
// therefore opt-in on more than one rank: LGH_COMM2=1 on every rank (LGH_COMM2=0 switches it off everywhere).
static int negotiate_second_channel(lgh_ctx *c, int nranks, int rank, RcclTransport &t, bool *channel2)
{
   DevPtr<char> dbuf;
   LGH_PASS(dbuf.alloc(128 + 2 * sizeof(double)));
   char hbuf[128 + sizeof(double)];
   ncclUniqueId id2;
   memset(&id2, 0, sizeof(id2));
   double ok = 1.0;
   if (rank == 0 && g_nccl.GetUniqueId(&id2) != ncclSuccess) { ok = 0.0; }
   memcpy(hbuf, id2.internal, 128);
   memcpy(hbuf + 128, &ok, sizeof(double));
   LGH_HIP_CHECK(hipMemcpy(dbuf, hbuf, sizeof(hbuf), hipMemcpyHostToDevice));
   LGH_NCCL_CHECK(g_nccl.Broadcast(dbuf, dbuf, sizeof(hbuf), /* ncclChar */ 0, 0, t.comm[0], c->stream));
   LGH_HIP_CHECK(hipStreamSynchronize(c->stream));
   LGH_HIP_CHECK(hipMemcpy(hbuf, dbuf, sizeof(hbuf), hipMemcpyDeviceToHost));
   memcpy(id2.internal, hbuf, 128);
   memcpy(&ok, hbuf + 128, sizeof(double)); // rank 0's verdict: nobody calls CommInitRank when it is 0
   if (ok != 0.0 && g_nccl.CommInitRank(&t.comm[1], nranks, id2, rank) != ncclSuccess) { ok = 0.0; t.comm[1] = nullptr; }
   double *dok = (double *)(dbuf.p + 128 + sizeof(double));
   LGH_HIP_CHECK(hipMemcpy(dok, &ok, sizeof(double), hipMemcpyHostToDevice));
   LGH_NCCL_CHECK(g_nccl.AllReduce(dok, dok, 1, ncclFloat64, ncclMin, t.comm[0], c->stream));
   LGH_HIP_CHECK(hipStreamSynchronize(c->stream));
   LGH_HIP_CHECK(hipMemcpy(&ok, dok, sizeof(double), hipMemcpyDeviceToHost));
   *channel2 = (ok != 0.0);
   if (!*channel2 && t.comm[1]) { g_nccl.CommDestroy(t.comm[1]); t.comm[1] = nullptr; }
   return LGH_OK;
}

int open_rccl(lgh_ctx *c, int nranks, int rank, const char unique_id[128], OpenedTransport &out)
{
   LGH_PASS(load_nccl());
   LGH_HIP_CHECK(hipSetDevice(c->device));
   auto t = std::make_unique<RcclTransport>();
   ncclUniqueId id;
   memcpy(id.internal, unique_id, 128);
   LGH_NCCL_CHECK(g_nccl.CommInitRank(&t->comm[0], nranks, id, rank));
   out.multi = (nranks > 1 || c->sw.force_multi) ? 1 : 0;
   const bool want2 = c->sw.comm2 >= 0 ? c->sw.comm2 == 1 : (nranks == 1);
   if (out.multi && g_nccl.Broadcast && want2) { LGH_PASS(negotiate_second_channel(c, nranks, rank, *t, &out.channel2)); }
   out.transport = std::move(t);
   return LGH_OK;
}

int rccl_unique_id(char id_out[128])
{
   LGH_PASS(load_nccl());
   ncclUniqueId id;
   LGH_NCCL_CHECK(g_nccl.GetUniqueId(&id));
   memcpy(id_out, id.internal, 128);
   return LGH_OK;
}

int rccl_self_sendrecv(lgh_ctx *c, double *buf, int n)
{
   const RcclTransport *t = c->comm ? dynamic_cast<const RcclTransport *>(c->comm->transport.get()) : nullptr;
   LGH_CHECK_ARG(t && t->comm[0]);
   if (g_nccl.GroupStart() != ncclSuccess || g_nccl.Send(buf, (size_t)n, ncclFloat64, c->rank, t->comm[0], c->stream) != ncclSuccess ||
       g_nccl.Recv(buf + n, (size_t)n, ncclFloat64, c->rank, t->comm[0], c->stream) != ncclSuccess ||
       g_nccl.GroupEnd() != ncclSuccess)
   {
      set_error("RCCL self send/recv failed");
      return LGH_ERR_COMM;
   }
   return LGH_OK;
}

// ---- what the two loop-backs share ----------------------------------------------------------------------------------
// Every exchange is carried out on the host, between two meetings of all ranks: the stream is drained (what this rank
// sends is complete) and `post` makes it visible; all ranks meet; `fetch` takes the peers' data; all ranks meet again,
// after which the peers may overwrite what they sent.  The order of these steps is what makes the emulation correct.
struct Loopback : Transport
{
   int n = 0, rank = 0;
   virtual const char *name() const = 0;
   virtual bool barrier() = 0;
   virtual double *slots() = 0; // all-reduce staging: 8 doubles per rank, rank after rank
   int meet(const char *what, const char *hint = "")
   {
      if (barrier()) { return LGH_OK; }
      set_error("%s: barrier timed out (%s)%s", name(), what, hint);
      return LGH_ERR_COMM;
   }
   template <class Post, class Fetch> int bracket(lgh_ctx *c, const char *what, const char *hint, Post post, Fetch fetch)
   {
      LGH_HIP_CHECK(hipStreamSynchronize(c->stream));
      LGH_PASS(post());
      LGH_PASS(meet(what, hint));
      LGH_PASS(fetch());
      return meet(what);
   }
   // where a peer keeps the block of rank `me` (index into the peer's neighbour list); -1: it has none, or of another size
   static int peer_block(const int *peer_rank, const int *peer_count, int peer_n, int me, int count)
   {
      int kk = -1;
      for (int j = 0; j < peer_n; j++) { if (peer_rank[j] == me) { kk = j; } }
      return (kk >= 0 && peer_count[kk] == count) ? kk : -1;
   }
   int no_match(int me, int peer)
   {
      set_error("%s: neighbour lists of ranks %d and %d do not match", name(), me, peer);
      return LGH_ERR_COMM;
   }
   int rendezvous(int nranks) override
   {
      if (barrier()) { return LGH_OK; }
      set_error("%s: not all %d ranks arrived", name(), nranks);
      return LGH_ERR_COMM;
   }
   int allreduce(lgh_ctx *c, int ch, double *dev, int count, int op) override
   {
      if (count > 8) { set_error("%s: count > 8", name()); return LGH_ERR_ARG; }
      // `mine` / `res` are pageable: an async copy to or from pageable memory is not
      // ordered with the kernels of the stream (observed: stale sums, run-to-run different
      // results), so drain the stream first and copy synchronously
      double mine[8], res[8];
      LGH_PASS(bracket(c, "all-reduce", "",
         [&]() -> int {
            LGH_HIP_CHECK(hipMemcpy(mine, dev, count * sizeof(double), hipMemcpyDeviceToHost));
            for (int i = 0; i < count; i++) { slots()[(size_t)rank * 8 + i] = mine[i]; }
            return LGH_OK;
         },
         [&]() -> int {
            for (int i = 0; i < count; i++)
            {
               double r = slots()[i];
               for (int k = 1; k < n; k++)
               {
                  const double x = slots()[(size_t)k * 8 + i];
                  r = (op == 0) ? r + x : std::min(r, x); // rank order: identical on every rank
               }
               res[i] = r;
            }
            return LGH_OK;
         }));
      LGH_HIP_CHECK(hipMemcpy(dev, res, count * sizeof(double), hipMemcpyHostToDevice));
      return LGH_OK;
   }
   long allreduce_max() const override { return 8; }
};

// ---- in-process loopback communicator (test vehicle) -------------------------------
// A unique id that starts with "LGHLOCAL" selects it: the ranks are contexts of ONE
// process (one host thread each, any devices that can copy to each other - in the
// tests all on the single GPU of the box) and the collectives are carried out
// with stream synchronisation, host barriers and device-to-device copies.  Everything
// else - owner masks, pack / canonical combine kernels, the separate-gather CG
// sequencing, finish kernels, dt and norm reductions - is the code that runs over RCCL
// on a node, so a multi-rank run can be checked against a single-rank one without a
// multi-GPU machine.  Not a product path: RCCL over xGMI is.
struct LocalGroup
{
   int n = 0;
   std::mutex m;
   std::condition_variable cv;
   int arrived = 0;
   long gen = 0;
   bool broken = false;
   std::vector<lgh_ctx *> ctx;   // by rank
   std::vector<double> slots;    // n * 8 doubles of all-reduce staging
   bool barrier()
   {
      std::unique_lock<std::mutex> lk(m);
      if (broken) { return false; }
      const long g = gen;
      if (++arrived == n)
      {
         arrived = 0;
         gen++;
         cv.notify_all();
         return true;
      }
      // a rank that never arrives (diverged control flow) must fail the test, not hang it
      if (!cv.wait_for(lk, std::chrono::seconds(60), [&] { return gen != g || broken; }))
      {
         broken = true;
         cv.notify_all();
         return false;
      }
      return !broken;
   }
};
static std::mutex g_local_m;
static std::map<std::string, std::shared_ptr<LocalGroup>> g_local;

struct LocalTransport : Loopback
{
   std::shared_ptr<LocalGroup> g;
   const char *name() const override { return "local communicator"; }
   bool barrier() override { return g->barrier(); }
   double *slots() override { return g->slots.data(); }
   ~LocalTransport() override
   {
      if (!g) { return; } // (never registered)
      std::lock_guard<std::mutex> lk(g_local_m);
      g->ctx[rank] = nullptr;
      bool any = false;
      for (lgh_ctx *p : g->ctx) { any = any || p; }
      for (auto it = g_local.begin(); !any && it != g_local.end();) { it = (it->second == g) ? g_local.erase(it) : std::next(it); }
   }
   int exchange_blocks(lgh_ctx *c, int ch, int ncomp, int nextra) override
   {
      const HaloTables &t = c->comm->tab;
      return bracket(c, "halo", "", [] { return LGH_OK; }, [&]() -> int {
         for (int k = 0; k < t.n_nbr; k++)
         {
            const HaloTables &pt = g->ctx[t.nbr_rank[k]]->comm->tab;
            const int kk = peer_block(pt.nbr_rank.data(), pt.nbr_count.data(), pt.n_nbr, c->rank, t.nbr_count[k]);
            if (kk < 0) { return no_match(c->rank, t.nbr_rank[k]); }
            LGH_HIP_CHECK(hipMemcpyAsync(t.recvbuf[ch] + t.nbr_base[k], pt.sendbuf[ch] + pt.nbr_base[kk],
                                         t.block_len(k, ncomp, nextra) * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
         }
         LGH_HIP_CHECK(hipStreamSynchronize(c->stream));
         return LGH_OK;
      }); // (second meeting: the peers may repack)
   }
   int exchange_words(lgh_ctx *c, const long long *src, int nwords) override
   {
      Comm *cm = c->comm.get();
      cm->word_src = src;
      return bracket(c, "words", "", [] { return LGH_OK; }, [&]() -> int {
         for (int k = 0; k < cm->tab.n_nbr; k++)
         {
            const Comm *pc = g->ctx[cm->tab.nbr_rank[k]]->comm.get();
            if (!pc->word_src) { set_error("local communicator: rank %d exchanges no words", cm->tab.nbr_rank[k]); return LGH_ERR_COMM; }
            LGH_HIP_CHECK(hipMemcpyAsync(cm->wordbuf + (size_t)k * nwords, pc->word_src, (size_t)nwords * sizeof(long long), hipMemcpyDeviceToDevice, c->stream));
         }
         LGH_HIP_CHECK(hipStreamSynchronize(c->stream));
         return LGH_OK;
      }); // (second meeting: the peers may go on adding)
   }
};

int open_local(lgh_ctx *c, int nranks, int rank, const char unique_id[128], OpenedTransport &out)
{
   auto t = std::make_unique<LocalTransport>();
   {
      std::lock_guard<std::mutex> lk(g_local_m);
      const std::string key(unique_id, 128);
      auto &slot = g_local[key];
      if (!slot)
      {
         slot = std::make_shared<LocalGroup>();
         slot->n = nranks;
         slot->ctx.assign(nranks, nullptr);
         slot->slots.assign((size_t)nranks * 8, 0.0);
      }
      if (slot->n != nranks || slot->ctx[rank]) { set_error("local communicator: rank %d registered twice", rank); return LGH_ERR_ARG; }
      slot->ctx[rank] = c;
      t->g = slot;
   }
   t->n = nranks;
   t->rank = rank;
   out.transport = std::move(t);
   out.channel2 = c->sw.comm2 != 0;
   return LGH_OK;
}

// ---- cross-process loopback communicator (test vehicle, bench.py --transport shm) ---------------
// A unique id that starts with "LGHSHM" names a POSIX shared-memory segment: the ranks are PROCESSES (what torchrun
// starts: one per rank, as on a multi-GPU node) that may all sit on one GPU - RCCL refuses two ranks on one device, so
// the one-GPU box cannot run the product transport with N > 1.  The exchanges are staged through the segment (device ->
// segment -> device) between process-shared barriers with a time-out.  Everything above the transport - torchrun
// rendezvous, broadcast of the id, lgh_comm_init / lgh_comm_set_neighbors, partition, owner masks, pack / canonical
// combine, piggy-backed sums, the sequencing of the solves, bench.py's rank-0 line - is the code a node runs.
// Not a product path: RCCL over xGMI is.
struct ShmHeader
{
   std::atomic<unsigned> magic;    // kShmMagic once rank 0 has initialised the segment
   std::atomic<int> arrived;       // sense-reversing barrier
   std::atomic<int> gen;
   std::atomic<int> broken;
   int nranks;
   size_t cap;                     // bytes of message area per rank and channel
   size_t off_slots, off_tables, off_msg;
};
constexpr unsigned kShmMagic = 0x4C474853u; // "LGHS"
static std::chrono::seconds shm_timeout() // how long a rank waits for its peers (LGH_SHM_TIMEOUT seconds, default 120)
{
   const char *e = getenv("LGH_SHM_TIMEOUT");
   return std::chrono::seconds((e && atoi(e) > 0) ? atoi(e) : 120);
}
constexpr int kShmMaxNbr = 32;
struct ShmTable // what a rank publishes about its send buffer: where the block of each neighbour starts
{
   int n_nbr;
   int nbr_rank[kShmMaxNbr], nbr_base[kShmMaxNbr], nbr_count[kShmMaxNbr];
};
struct ShmGroup
{
   std::string name;
   void *base = nullptr;
   size_t bytes = 0;
   int n = 0, rank = 0;
   ShmHeader *hdr() const { return (ShmHeader *)base; }
   double *slots(int r) const { return (double *)((char *)base + hdr()->off_slots) + (size_t)r * 8; }
   ShmTable *table(int r) const { return (ShmTable *)((char *)base + hdr()->off_tables) + r; }
   double *msg(int r, int ch) const { return (double *)((char *)base + hdr()->off_msg + ((size_t)r * 2 + ch) * hdr()->cap); }
   bool barrier()
   {
      ShmHeader *h = hdr();
      if (h->broken.load()) { return false; }
      const int g = h->gen.load();
      if (h->arrived.fetch_add(1) + 1 == n)
      {
         h->arrived.store(0);
         h->gen.fetch_add(1);
         return true;
      }
      const auto t0 = std::chrono::steady_clock::now();
      long spins = 0;
      while (h->gen.load() == g)
      {
         if (h->broken.load()) { return false; }
         if ((++spins & 1023) == 0)
         {
            // a rank that never arrives (diverged control flow, dead process) must fail the run, not hang it
            if (std::chrono::steady_clock::now() - t0 > shm_timeout()) { h->broken.store(1); return false; }
            usleep(50);
         }
      }
      return !h->broken.load();
   }
   int open(const char unique_id[128], int nranks, int rank_);
   ~ShmGroup()
   {
      if (base) { munmap(base, bytes); }
      if (rank == 0 && !name.empty()) { shm_unlink(name.c_str()); }
   }
};
int ShmGroup::open(const char unique_id[128], int nranks, int rank_)
{
   name = std::string("/") + std::string(unique_id, strnlen(unique_id, 64));
   n = nranks;
   rank = rank_;
   const char *menv = getenv("LGH_SHM_MB"); // message area per rank and channel (a 32^3 Q3Q2 block sends 1.4 MB per exchange)
   const size_t cap = (size_t)std::max(1, menv ? atoi(menv) : 16) << 20;
   const size_t off_slots = 4096, off_tables = off_slots + ((size_t)nranks * 8 * sizeof(double) + 4095) / 4096 * 4096;
   const size_t off_msg = off_tables + ((size_t)nranks * sizeof(ShmTable) + 4095) / 4096 * 4096;
   bytes = off_msg + (size_t)nranks * 2 * cap;
   int fd = -1;
   if (rank == 0)
   {
      shm_unlink(name.c_str());
      fd = shm_open(name.c_str(), O_CREAT | O_EXCL | O_RDWR, 0600);
      if (fd < 0 || ftruncate(fd, (off_t)bytes) != 0) { set_error("shm transport: cannot create %s", name.c_str()); if (fd >= 0) { close(fd); } return LGH_ERR_COMM; }
   }
   else
   {
      const auto t0 = std::chrono::steady_clock::now();
      while (true)
      {
         fd = shm_open(name.c_str(), O_RDWR, 0600);
         struct stat st;
         // (the size is rank 0's: its LGH_SHM_MB decides, whatever this rank's environment says)
         if (fd >= 0 && fstat(fd, &st) == 0 && (size_t)st.st_size >= off_msg) { bytes = (size_t)st.st_size; break; }
         if (fd >= 0) { close(fd); fd = -1; }
         if (std::chrono::steady_clock::now() - t0 > shm_timeout()) { set_error("shm transport: %s did not appear (rank 0 missing?)", name.c_str()); return LGH_ERR_COMM; }
         usleep(2000);
      }
   }
   base = mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
   close(fd);
   if (base == MAP_FAILED) { base = nullptr; set_error("shm transport: mmap failed"); return LGH_ERR_COMM; }
   ShmHeader *h = hdr();
   if (rank == 0)
   {
      h->arrived.store(0); h->gen.store(0); h->broken.store(0);
      h->nranks = nranks; h->cap = cap; h->off_slots = off_slots; h->off_tables = off_tables; h->off_msg = off_msg;
      h->magic.store(kShmMagic);
   }
   else
   {
      const auto t0 = std::chrono::steady_clock::now();
      while (h->magic.load() != kShmMagic)
      {
         if (std::chrono::steady_clock::now() - t0 > shm_timeout()) { set_error("shm transport: segment never initialised"); return LGH_ERR_COMM; }
         usleep(1000);
      }
      if (h->nranks != nranks) { set_error("shm transport: segment is for %d ranks, not %d", h->nranks, nranks); return LGH_ERR_COMM; }
   }
   return LGH_OK;
}

struct ShmTransport : Loopback
{
   ShmGroup g;
   std::vector<double> stage;     // host staging of one receive buffer
   std::vector<long long> wstage; // ... of the peers' words
   const char *name() const override { return "shm transport"; }
   bool barrier() override { return g.barrier(); }
   double *slots() override { return g.slots(0); }
   static constexpr const char *kHint = ": a rank is missing or the ranks do not call the same exchanges";
   int exchange_blocks(lgh_ctx *c, int ch, int ncomp, int nextra) override
   {
      const HaloTables &t = c->comm->tab;
      const size_t bytes = (size_t)t.bufsize * sizeof(double);
      if (bytes > g.hdr()->cap) { set_error("shm transport: message of %zu bytes, room for %zu (LGH_SHM_MB)", bytes, g.hdr()->cap); return LGH_ERR_COMM; }
      return bracket(c, "halo", kHint,
         [&]() -> int { LGH_HIP_CHECK(hipMemcpy(g.msg(c->rank, ch), t.sendbuf[ch], bytes, hipMemcpyDeviceToHost)); return LGH_OK; },
         [&]() -> int {
            stage.resize((size_t)t.bufsize);
            for (int k = 0; k < t.n_nbr; k++)
            {
               const ShmTable *pt = g.table(t.nbr_rank[k]);
               const int kk = peer_block(pt->nbr_rank, pt->nbr_count, pt->n_nbr, c->rank, t.nbr_count[k]);
               if (kk < 0) { return no_match(c->rank, t.nbr_rank[k]); }
               memcpy(stage.data() + t.nbr_base[k], g.msg(t.nbr_rank[k], ch) + pt->nbr_base[kk], t.block_len(k, ncomp, nextra) * sizeof(double));
            }
            LGH_HIP_CHECK(hipMemcpy(t.recvbuf[ch], stage.data(), bytes, hipMemcpyHostToDevice));
            return LGH_OK;
         }); // (second meeting: the peers may repack)
   }
   int exchange_words(lgh_ctx *c, const long long *src, int nwords) override
   {
      const Comm *cm = c->comm.get();
      const int n_nbr = cm->tab.n_nbr;
      const size_t bytes = (size_t)nwords * sizeof(long long);
      if (bytes > g.hdr()->cap) { set_error("shm transport: %zu bytes of words, room for %zu", bytes, g.hdr()->cap); return LGH_ERR_COMM; }
      return bracket(c, "words", kHint,
         [&]() -> int { LGH_HIP_CHECK(hipMemcpy(g.msg(c->rank, 0), src, bytes, hipMemcpyDeviceToHost)); return LGH_OK; },
         [&]() -> int {
            wstage.resize((size_t)n_nbr * nwords);
            for (int k = 0; k < n_nbr; k++) { memcpy(wstage.data() + (size_t)k * nwords, g.msg(cm->tab.nbr_rank[k], 0), bytes); }
            LGH_HIP_CHECK(hipMemcpy(cm->wordbuf, wstage.data(), (size_t)n_nbr * bytes, hipMemcpyHostToDevice));
            return LGH_OK;
         }); // (second meeting: the peers may reuse their message area)
   }
   int publish_tables(int rank_, const HaloTables *t) override
   {
      if (t && t->n_nbr > kShmMaxNbr) { set_error("shm transport: more than %d neighbours", kShmMaxNbr); return LGH_ERR_ARG; }
      ShmTable *st = g.table(rank_);
      st->n_nbr = t ? t->n_nbr : 0;
      for (int k = 0; k < st->n_nbr; k++) { st->nbr_rank[k] = t->nbr_rank[k]; st->nbr_base[k] = t->nbr_base[k]; st->nbr_count[k] = t->nbr_count[k]; }
      return LGH_OK;
   }
};

int open_shm(lgh_ctx *c, int nranks, int rank, const char unique_id[128], OpenedTransport &out)
{
   auto t = std::make_unique<ShmTransport>();
   LGH_PASS(t->g.open(unique_id, nranks, rank));
   t->n = nranks;
   t->rank = rank;
   out.transport = std::move(t);
   // (the exchanges are synchronous on the host: the energy solve's sums may use the second channel's buffers safely)
   out.channel2 = c->sw.comm2 != 0;
   return LGH_OK;
}

} // namespace lgh
