// comm_local.hip -- the in-process transport (Comm::kind == 3): the ranks are threads of one process, so a rank's
// kernel stores its operand straight into its peers' device memory.  No host staging, no RCCL.
//
// Every rank owns two device mailboxes of one common capacity.  One collective, on every rank:
//   1. k_comm_put on the rank's own stream: the payload into the mailbox of every peer that gets it
//   2. hipStreamSynchronize: the rank's stores have landed (and everything it queued before them is done)
//   3. the host barrier of the group: everybody's stores have landed
//   4. k_comm_reduce / k_comm_unpack on the own stream: own mailbox -> the operand, in place
// The put never goes into a peer's live vector: a faster rank arrives while the peer's earlier kernels (an SpMV
// reading p, say) still read it.  It goes into the mailbox, which nothing but step 4 reads.
#include "comm.hpp"
#include "devmem.hpp"

#include <algorithm>

namespace sim3opt {

#include "comm_kernels.hpp"

namespace {

LocalRank& self(Comm& c) { return c.local->ranks[c.rank]; }

// Which of the two mailboxes collective `seq` uses: they alternate.  A put of collective k + 2 must not overwrite
// what a peer's step 4 of collective k still reads.  It cannot: the put is launched after this rank left barrier
// k + 1, the peer entered barrier k + 1 after its own step 2 of collective k + 1, and that synchronisation of its
// stream covers its step 4 of collective k, queued there earlier.  (With ONE mailbox the put of k + 1 would race the
// peer's step 4 of k: nothing but the stream orders a rank's step 4, and a peer does not wait for that stream.)
int parity(const LocalRank& me) { return (int)(me.seq & 1u); }

int barrier_wait(Comm& c, std::string& err) {
  LocalRank& me = self(c);
  const uint64_t seq = me.seq++;
  const RankBarrier::Result how = c.local->barrier.wait(c.local->timeout_s);
  if (how == RankBarrier::PASSED) return SIM3OPT_OK;
  err = rank_barrier_message(how, c.rank, c.local->timeout_s, seq);
  return SIM3OPT_ERR_COMM;
}

// Mailboxes of at least `need` doubles on every rank.  Every rank calls this with the same `need` at the same
// collective, so all of them grow together: own stream synchronised (own step 4 of earlier collectives is done with
// the old blocks; the peers' puts into them landed before the last barrier), new blocks, a barrier, and only then
// does anybody read a peer's pointers.
int ensure_capacity(Comm& c, int64_t need, hipStream_t stream, std::string& err) {
  LocalRank& me = self(c);
  if (need <= me.cap) return SIM3OPT_OK;
  int64_t cap = std::max<int64_t>(me.cap, 64);
  while (cap < need) cap *= 2;
  HIPCHK(hipStreamSynchronize(stream));
  for (double*& m : me.mbox) {
    dev_free(m);
    m = nullptr;
  }
  me.cap = 0;
  for (double*& m : me.mbox) HIPCHK(dev_malloc_of((void**)&m, sizeof(double) * (size_t)cap, true));
  me.cap = cap;
  return barrier_wait(c, err);
}

int launch_spans(bool put, const CommSpans& s, hipStream_t stream, std::string& err) {
  if (s.count == 0) return SIM3OPT_OK;
  long long nmax = 0;
  for (int i = 0; i < s.count; ++i) nmax = std::max(nmax, s.n[i]);
  const int gx = (int)std::min<long long>(COMM_MAX_GRID_X, std::max<long long>(1, (nmax / 2 + COMM_WG - 1) / COMM_WG));
  if (put) hipLaunchKernelGGL(k_comm_put, dim3(gx, s.count), dim3(COMM_WG), 0, stream, s);
  else hipLaunchKernelGGL(k_comm_unpack, dim3(gx, s.count), dim3(COMM_WG), 0, stream, s);
  HIPCHK(hipGetLastError());
  return SIM3OPT_OK;
}

void add_span(CommSpans& s, double* dst, const double* src, int64_t n) {
  if (n <= 0) return;
  s.dst[s.count] = dst;
  s.src[s.count] = src;
  s.n[s.count] = n;
  ++s.count;
}

}  // namespace

void comm_init_local(Comm& c, LocalGroup* group, int32_t rank) {
  c.release();
  c.kind = 3;
  c.local = group;
  c.rank = rank;
  c.world = group->world;
}

int comm_local_connect(Comm& c, std::string& err) {
  const LocalGroup& G = *c.local;
  const int mine = G.ranks[c.rank].device;
  for (int p = 0; p < G.world; ++p) {
    const int dev = G.ranks[p].device;
    bool seen = dev == mine;  // (a repeated ordinal: ordinary pointers, nothing to enable)
    for (int q = 0; q < p; ++q) seen = seen || G.ranks[q].device == dev;
    if (seen) continue;
    int can = 0;
    HIPCHK(hipDeviceCanAccessPeer(&can, mine, dev));
    if (!can) {
      err = "device " + std::to_string(mine) + " has no peer access to device " + std::to_string(dev) +
            " (ranks " + std::to_string(c.rank) + " and " + std::to_string(p) + "): the in-process transport needs it";
      return SIM3OPT_ERR_COMM;
    }
    const hipError_t e = hipDeviceEnablePeerAccess(dev, 0);
    if (e == hipErrorPeerAccessAlreadyEnabled) (void)hipGetLastError();
    else HIPCHK(e);
  }
  return SIM3OPT_OK;
}

// slot r of every mailbox = rank r's operand; every rank folds its own mailbox in rank order
int comm_local_allreduce(Comm& c, double* dptr, int n, int op, hipStream_t stream, std::string& err) {
  LocalGroup& G = *c.local;
  const int64_t slot = ((int64_t)n + 1) & ~(int64_t)1;  // (even: every slot starts 16-byte aligned)
  int rc = ensure_capacity(c, slot * G.world, stream, err);
  if (rc) return rc;
  LocalRank& me = self(c);
  const int par = parity(me);
  CommSpans s{};
  for (int p = 0; p < G.world; ++p) add_span(s, G.ranks[p].mbox[par] + slot * c.rank, dptr, n);
  rc = launch_spans(true, s, stream, err);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(stream));
  rc = barrier_wait(c, err);
  if (rc) return rc;
  const int gx = std::min(COMM_MAX_GRID_X, std::max(1, (n + COMM_WG - 1) / COMM_WG));
  hipLaunchKernelGGL(k_comm_reduce, dim3(gx), dim3(COMM_WG), 0, stream, (const double*)me.mbox[par], (int)G.world,
                     (long long)slot, n, op, dptr);
  HIPCHK(hipGetLastError());
  return SIM3OPT_OK;
}

// the mailbox is laid out like the vector: rank r's span goes to offs[r] of every other rank's mailbox
int comm_local_allgatherv(Comm& c, double* dvec, const std::vector<int64_t>& offs, hipStream_t stream,
                          std::string& err) {
  LocalGroup& G = *c.local;
  const int64_t lo = offs[c.rank], hi = offs[c.rank + 1], total = offs[G.world];
  int rc = ensure_capacity(c, total, stream, err);
  if (rc) return rc;
  LocalRank& me = self(c);
  const int par = parity(me);
  CommSpans s{};
  for (int p = 0; p < G.world; ++p)
    if (p != c.rank) add_span(s, G.ranks[p].mbox[par] + lo, dvec + lo, hi - lo);
  rc = launch_spans(true, s, stream, err);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(stream));
  rc = barrier_wait(c, err);
  if (rc) return rc;
  CommSpans u{};  // everything but the own span: two contiguous pieces
  add_span(u, dvec, me.mbox[par], lo);
  add_span(u, dvec + hi, me.mbox[par] + hi, total - hi);
  return launch_spans(false, u, stream, err);
}

// The inbox is the mailbox cut into `world` equal slots, slot p for what rank p sends: a sender needs nothing of the
// receiver's plan.  A slot must hold the largest segment of ANY pair, which a rank cannot know: it publishes what its
// own segments ask for and, if that is beyond the capacity, holds its put back; after the barrier every rank sees
// every request, and if one is beyond the capacity all of them grow the mailboxes and run the collective again.
int comm_local_exchange(Comm& c, const double* sbuf, const std::vector<int64_t>& soffs, double* rbuf,
                        const std::vector<int64_t>& roffs, hipStream_t stream, std::string& err) {
  LocalGroup& G = *c.local;
  LocalRank& me = self(c);
  int64_t longest = 0;
  for (int p = 0; p < G.world; ++p)
    longest = std::max(longest, std::max(soffs[p + 1] - soffs[p], roffs[p + 1] - roffs[p]));
  const int64_t need = G.world * ((longest + 1) & ~(int64_t)1);
  for (int round = 0; round < 2; ++round) {
    const int par = parity(me);
    const int64_t slot = (me.cap / G.world) & ~(int64_t)1;
    const bool fits = need <= me.cap;
    if (round == 0) me.need[par] = need;  // (read by the peers after this collective's barrier, written again two later)
    if (fits) {
      CommSpans s{};
      for (int p = 0; p < G.world; ++p)
        add_span(s, G.ranks[p].mbox[par] + slot * c.rank, sbuf + soffs[p], soffs[p + 1] - soffs[p]);
      const int rc = launch_spans(true, s, stream, err);
      if (rc) return rc;
    }
    HIPCHK(hipStreamSynchronize(stream));
    int rc = barrier_wait(c, err);
    if (rc) return rc;
    int64_t asked = need;
    if (round == 0)
      for (int p = 0; p < G.world; ++p) asked = std::max(asked, G.ranks[p].need[par]);
    if (asked > me.cap) {  // (the same verdict on every rank; in the second round everything fits)
      rc = ensure_capacity(c, asked, stream, err);
      if (rc) return rc;
      continue;
    }
    CommSpans u{};
    for (int p = 0; p < G.world; ++p)
      add_span(u, rbuf + roffs[p], me.mbox[par] + slot * p, roffs[p + 1] - roffs[p]);
    return launch_spans(false, u, stream, err);
  }
  err = "exchange: the mailboxes did not grow to what the ranks asked for";
  return SIM3OPT_ERR_COMM;
}

void comm_local_release(Comm& c) {
  if (!c.local) return;
  LocalRank& me = self(c);
  for (double*& m : me.mbox) {
    dev_free(m);
    m = nullptr;
  }
  me.cap = 0;
}

}  // namespace sim3opt
