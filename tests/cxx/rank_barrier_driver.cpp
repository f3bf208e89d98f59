// rank_barrier_driver.cpp -- the host side of the in-process transport under ThreadSanitizer: the fail-fast barrier
// (sim3opt_amd/csrc/rank_barrier.hpp) and the two-mailbox parity scheme of comm_local.hip, with host arrays in the
// place of the device mailboxes and plain stores in the place of the kernels.  No GPU, no library.
//   g++ -std=c++17 -O1 -g -fsanitize=thread -pthread -Isim3opt_amd/csrc tests/cxx/rank_barrier_driver.cpp
// Prints "N passed, M failed"; a data race makes ThreadSanitizer report and the exit status non-zero.
#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "rank_barrier.hpp"

using sim3opt::RankBarrier;

static int n_pass = 0, n_fail = 0;
static void check(bool ok, const char* what) {
  std::printf("%s %s\n", ok ? "ok  " : "FAIL", what);
  (ok ? n_pass : n_fail)++;
}

constexpr int WORLD = 8;

// one collective as comm_local.hip orders it: put into every peer's mailbox of this parity, (stream synchronise: the
// stores are plain here), barrier, fold the own mailbox in rank order.  ONE barrier per collective: the parity is what
// keeps the put of collective k + 2 off the slots a slower peer still folds for collective k.
struct Mailboxes {
  double slot[WORLD][2][WORLD];  // [owner][parity][sender]
};

static double operand(int rank, int round) { return 1.0 / (1.0 + rank) + 1e-3 * round + 1e-9 * rank * round; }

// returns the round at which this rank left with an error (rounds when none)
static int all_reduce_rounds(Mailboxes& M, RankBarrier& bar, int rank, int rounds, double timeout_s, int abort_at,
                             int abort_rank, bool* sums_ok, RankBarrier::Result* how) {
  *sums_ok = true;
  *how = RankBarrier::PASSED;
  for (int k = 0; k < rounds; ++k) {
    if (k == abort_at && rank == abort_rank) {  // this rank's "engine call failed"
      bar.abort();
      *how = RankBarrier::ABORTED;
      return k;
    }
    const int par = k & 1;
    for (int p = 0; p < WORLD; ++p) M.slot[p][par][rank] = operand(rank, k);
    const RankBarrier::Result r = bar.wait(timeout_s);
    if (r != RankBarrier::PASSED) {
      *how = r;
      return k;
    }
    double acc = M.slot[rank][par][0];
    for (int s = 1; s < WORLD; ++s) acc = acc + M.slot[rank][par][s];
    double want = operand(0, k);
    for (int s = 1; s < WORLD; ++s) want = want + operand(s, k);
    if (std::memcmp(&acc, &want, sizeof(double)) != 0) *sums_ok = false;
  }
  return rounds;
}

int main() {
  using clock = std::chrono::steady_clock;
  {  // 1. 2000 rounds, every rank the rank-order sum bit for bit
    Mailboxes M{};
    RankBarrier bar(WORLD);
    bool ok[WORLD];
    int done[WORLD];
    RankBarrier::Result how[WORLD];
    std::vector<std::thread> ts;
    for (int r = 0; r < WORLD; ++r)
      ts.emplace_back([&, r] { done[r] = all_reduce_rounds(M, bar, r, 2000, 30.0, -1, -1, &ok[r], &how[r]); });
    for (auto& t : ts) t.join();
    bool all = true;
    for (int r = 0; r < WORLD; ++r) all = all && ok[r] && done[r] == 2000 && how[r] == RankBarrier::PASSED;
    check(all, "8 ranks, 2000 all-reduces over two mailboxes: the rank-order sum on every rank, every round");
    check(!bar.aborted(), "... and the barrier is whole");
  }
  {  // 2. one rank fails in round 1000: everybody else leaves its wait with the error, all threads join
    Mailboxes M{};
    RankBarrier bar(WORLD);
    bool ok[WORLD];
    int done[WORLD];
    RankBarrier::Result how[WORLD];
    const auto t0 = clock::now();
    std::vector<std::thread> ts;
    for (int r = 0; r < WORLD; ++r)
      ts.emplace_back([&, r] { done[r] = all_reduce_rounds(M, bar, r, 2000, 30.0, 1000, 3, &ok[r], &how[r]); });
    for (auto& t : ts) t.join();
    const double secs = std::chrono::duration<double>(clock::now() - t0).count();
    bool all = true;
    for (int r = 0; r < WORLD; ++r) all = all && ok[r] && done[r] == 1000 && how[r] == RankBarrier::ABORTED;
    check(all, "abort() in round 1000: every rank leaves round 1000 with ABORTED, the sums before it exact");
    check(secs < 30.0, "... well within the timeout");
    check(bar.aborted() && bar.wait(30.0) == RankBarrier::ABORTED, "... and the barrier stays aborted");
  }
  {  // 3. one rank never arrives: the first waiter to run out of time aborts, the others follow
    RankBarrier bar(WORLD);
    RankBarrier::Result how[WORLD];
    std::string msg[WORLD];
    const unsigned long long seq = 41;  // (the collective's sequence number, as comm_local.hip counts it)
    const auto t0 = clock::now();
    std::vector<std::thread> ts;
    for (int r = 0; r < WORLD - 1; ++r)
      ts.emplace_back([&, r] {
        how[r] = bar.wait(0.2);
        msg[r] = sim3opt::rank_barrier_message(how[r], r, 0.2, seq + r);
      });
    for (auto& t : ts) t.join();
    const double secs = std::chrono::duration<double>(clock::now() - t0).count();
    int timed_out = 0, aborted = 0;
    bool named = true;
    for (int r = 0; r < WORLD - 1; ++r) {
      timed_out += how[r] == RankBarrier::TIMED_OUT;
      aborted += how[r] == RankBarrier::ABORTED;
      const std::string want = "collective " + std::to_string(seq + r);
      named = named && msg[r].find(want) != std::string::npos && msg[r].find("rank " + std::to_string(r)) == 0;
      if (how[r] == RankBarrier::TIMED_OUT) named = named && msg[r].find("waited longer than 0.2") != std::string::npos;
    }
    check(timed_out >= 1 && timed_out + aborted == WORLD - 1, "a rank that never arrives: time-out on the waiters, nobody hangs");
    check(named, "... every message names its rank and its collective, the time-out its limit");
    check(secs >= 0.2 && secs < 5.0, "... after the timeout, not before and not much later");
    check(bar.aborted(), "... and the barrier is aborted");
  }
  std::printf("%d passed, %d failed\n", n_pass, n_fail);
  return n_fail == 0 ? 0 : 1;
}
