// lgh_comm_transport.hpp — several ranks: what the operations (lgh_comm.hip) and the ways the data travels
// (lgh_comm_transport.hip) share - the neighbour tables of a context, the transport interface and Comm.
#pragma once
#include <memory>

#include "lgh_common.hpp"

namespace lgh
{

constexpr int kHaloSlack = 4; // doubles of room behind every neighbour's block (<= 4 scalars: (d, A d) of the three velocity components and, in lockstep, of the energy CG)

// The neighbour tables of one lgh_comm_set_neighbors call: built into a local object (build_tables, lgh_comm.hip) and
// move-assigned into Comm when complete, so a context holds the tables of ONE call or none.
// (The layout of the buffers: at halo_pack_k, lgh_comm.hip.)
struct HaloTables
{
   int n_nbr = 0;
   std::vector<int> nbr_rank, nbr_count, nbr_off, nbr_base; // node offsets / buffer bases of the neighbours
   int total = 0;    // sum of nbr_count
   int n_shared = 0; // unique shared nodes
   int bufsize = 0;  // doubles in a send / receive buffer
   // piggy-backed scalars: when every other rank is a neighbour (block partitions of up to 2x2x2) a few doubles ride on
   // each halo message and are summed in rank order by the combine kernel - one collective less per CG iteration
   bool allpairs = false;
   DevPtr<int> nodes;                   // concatenated neighbour node lists
   DevPtr<int> pos, cnt;                // per concatenated entry: buffer position, neighbour count
   DevPtr<int> sh_node, sh_off, sh_src; // CSR over the unique shared nodes (see halo_combine_k)
   DevPtr<uint8_t> hmask;               // 1 for every shared node
   DevPtr<int> d_base, d_cnt;           // per neighbour: block base, node count
   DevPtr<int> rank_src;                // per rank: neighbour index or -1 (self)
   // per channel (0 main, 1 second): bufsize doubles.  The second channel has message buffers of its own for the stream
   // the energy solve runs on beside the velocity solve (lgh_solve_energy_begin/_end); it only ever carries sums of scalars.
   DevPtr<double> sendbuf[2], recvbuf[2];
   size_t block_len(const int k, const int ncomp, const int nextra) const { return (size_t)ncomp * nbr_count[k] + nextra; }
};

// How the messages of a context travel: RCCL over xGMI (the product), or one of the two loop-backs the tests run several
// ranks with on one GPU (unique ids "LGHLOCAL..." / "LGHSHM...").  Everything else - tables, pack and combine kernels, the
// choice of channel, what is timed - is lgh_comm.hip and the same over each of them.  ch: 0 main channel, 1 second.
struct Transport
{
   virtual ~Transport() = default;
   // with every neighbour k: block [base_k, base_k + ncomp*cnt_k + nextra) of the channel's send buffer goes out, the
   // same block of its receive buffer comes in
   virtual int exchange_blocks(lgh_ctx *c, int ch, int ncomp, int nextra) = 0;
   // nwords accumulator words at src go to every neighbour; theirs arrive in Comm::wordbuf, block k = neighbour k
   virtual int exchange_words(lgh_ctx *c, const long long *src, int nwords) = 0;
   // count doubles on the device, in place; op 0: SUM, otherwise MIN
   virtual int allreduce(lgh_ctx *c, int ch, double *dev, int count, int op) = 0;
   virtual long allreduce_max() const = 0; // values one all-reduce takes
   virtual int rendezvous(int nranks) { return LGH_OK; } // end of lgh_comm_init: every rank has opened its end
   // lgh_comm_set_neighbors, before the ranks agree on the outcome: what the peers have to know of this rank's new
   // tables (nullptr: the build failed)
   virtual int publish_tables(int rank, const HaloTables *t) { return LGH_OK; }
};

struct Comm
{
   HaloTables tab;
   // Second channel: present on every rank or on none (decided collectively, lgh_comm_init); its buffers are in the tables
   bool channel2 = false;
   // exchange_words: the peers' accumulator words (n_nbr blocks of wordcap words), and where this rank's own words are
   // (the in-process transport copies device to device out of the peer's accumulators)
   DevPtr<long long> wordbuf;
   int wordcap = 0, wordnbr = 0; // words per peer and peers the buffer was allocated for
   const long long *word_src = nullptr;
   // (last member: closed first - the in-process peers must not find this rank any more when its buffers go)
   std::unique_ptr<Transport> transport;
};

// lgh_comm_init: this rank's end of a transport, opened
struct OpenedTransport
{
   std::unique_ptr<Transport> transport;
   bool channel2 = false; // the energy solve's sums may use the second channel
   int multi = 1;         // the context takes the several-rank path (RCCL on one rank: only when forced)
};
int open_rccl(lgh_ctx *c, int nranks, int rank, const char unique_id[128], OpenedTransport &out);
int open_local(lgh_ctx *c, int nranks, int rank, const char unique_id[128], OpenedTransport &out);
int open_shm(lgh_ctx *c, int nranks, int rank, const char unique_id[128], OpenedTransport &out);
int rccl_unique_id(char id_out[128]);
// a grouped send / recv of n doubles from buf to buf + n on this rank itself, over the context's RCCL communicator
int rccl_self_sendrecv(lgh_ctx *c, double *buf, int n);

} // namespace lgh
