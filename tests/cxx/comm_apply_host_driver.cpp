// comm_apply_host_driver.cpp -- the host half of the transport's diagnostic read-outs (csrc/comm_apply_host.hpp: argument
// checks, offset checks, the agreement of the ranks' exchange plans, where each rank's buffers start) as a stand-alone
// program for AddressSanitizer + UndefinedBehaviorSanitizer: no GPU and no HIP.  Plans are heap blocks of exactly the size
// handed over, so that a read past an end is the sanitizer's to find; every message is compared as a whole string.
#include <cstdio>
#include <string>
#include <vector>

#include "../../sim3opt_amd/csrc/comm_apply_host.hpp"

using namespace sim3opt;

static int failed = 0, checks = 0;
#define CHECK(c)                                                      \
  do {                                                                \
    ++checks;                                                         \
    if (!(c)) { ++failed; std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); } \
  } while (0)

using V = std::vector<int64_t>;

// counts[p][q] doubles from p to q, first segments at send_lead[r] / recv_lead[r]: the two tables of world x (world + 1)
static void plans(const std::vector<V>& counts, const V& send_lead, const V& recv_lead, V& soffs, V& roffs) {
  const size_t w = counts.size();
  soffs.assign(w * (w + 1), 0);
  roffs.assign(w * (w + 1), 0);
  for (size_t r = 0; r < w; ++r) {
    soffs[r * (w + 1)] = send_lead[r];
    roffs[r * (w + 1)] = recv_lead[r];
    for (size_t p = 0; p < w; ++p) {
      soffs[r * (w + 1) + p + 1] = soffs[r * (w + 1) + p] + counts[r][p];
      roffs[r * (w + 1) + p + 1] = roffs[r * (w + 1) + p] + counts[p][r];
    }
  }
  soffs.shrink_to_fit();
  roffs.shrink_to_fit();
}

int main() {
  const double x = 0.0;
  const void* p = &x;

  // ---- offsets
  for (int32_t w : {1, 2, 8}) {
    V o((size_t)w + 1, 0);
    o.shrink_to_fit();
    CHECK(comm_offsets_ok(o.data(), w));  // all empty
    for (int32_t r = 0; r <= w; ++r) o[r] = 3 * r + 1;
    CHECK(comm_offsets_ok(o.data(), w));  // (may start above 0)
    o[w] = o[w - 1] - 1;
    CHECK(!comm_offsets_ok(o.data(), w));  // the last one decreases
    o[w] = o[w - 1];
    o[0] = -1;
    CHECK(!comm_offsets_ok(o.data(), w));
  }

  // ---- all-reduce
  CHECK(comm_check_allreduce(0, 0, 0, p, p) == "");
  CHECK(comm_check_allreduce((int64_t)1 << 30, 1, 1, p, p) == "");
  CHECK(comm_check_allreduce(-1, 0, 0, p, p) == "comm_apply_allreduce: n must be in 0 .. 2^30");
  CHECK(comm_check_allreduce(((int64_t)1 << 30) + 1, 0, 0, p, p) == "comm_apply_allreduce: n must be in 0 .. 2^30");
  CHECK(comm_check_allreduce(INT64_MIN, 0, 0, p, p) == "comm_apply_allreduce: n must be in 0 .. 2^30");
  CHECK(comm_check_allreduce(4, 2, 0, p, p) == "comm_apply_allreduce: op is 0 (sum) or 1 (max)");
  CHECK(comm_check_allreduce(4, -1, 0, p, p) == "comm_apply_allreduce: op is 0 (sum) or 1 (max)");
  CHECK(comm_check_allreduce(4, 0, 2, p, p) == "comm_apply_allreduce: phase is 0 or 1");
  CHECK(comm_check_allreduce(4, 0, -1, p, p) == "comm_apply_allreduce: phase is 0 or 1");
  CHECK(comm_check_allreduce(4, 0, 0, nullptr, p) == "comm_apply_allreduce: null argument");
  CHECK(comm_check_allreduce(4, 0, 0, p, nullptr) == "comm_apply_allreduce: null argument");

  // ---- all-gather
  {
    V o{0, 2, 2, 7};
    o.shrink_to_fit();
    CHECK(comm_check_allgatherv(o.data(), 3, 0, p, p) == "");
    CHECK(comm_check_allgatherv(o.data(), 3, 1, p, p) == "");
    CHECK(comm_check_allgatherv(o.data(), 3, 2, p, p) == "comm_apply_allgatherv: phase is 0 or 1");
    CHECK(comm_check_allgatherv(nullptr, 3, 0, p, p) == "comm_apply_allgatherv: null argument");
    CHECK(comm_check_allgatherv(o.data(), 3, 0, nullptr, p) == "comm_apply_allgatherv: null argument");
    CHECK(comm_check_allgatherv(o.data(), 3, 0, p, nullptr) == "comm_apply_allgatherv: null argument");
    V late{1, 2, 2, 7}, down{0, 3, 2, 7}, zero{0, 0, 0, 0};
    CHECK(comm_check_allgatherv(late.data(), 3, 0, p, p) == "comm_apply_allgatherv: offsets start at 0 and never decrease");
    CHECK(comm_check_allgatherv(down.data(), 3, 0, p, p) == "comm_apply_allgatherv: offsets start at 0 and never decrease");
    CHECK(comm_check_allgatherv(zero.data(), 3, 0, p, p) == "");
  }

  // ---- exchange
  {
    const std::vector<V> counts{{9, 0, 1}, {2, 0, 7}, {0, 0, 3}};  // (self-sends, a pair one way only, an empty column)
    V so, ro, sb, rb;
    plans(counts, {0, 1, 0}, {1, 0, 1}, so, ro);
    CHECK(comm_check_exchange(so.data(), ro.data(), 3, 0, 1, p, p, sb, rb) == "");
    CHECK((sb == V{0, 10, 20, 23}) && (rb == V{0, 12, 12, 24}));  // (buffer lengths include what lies before the first segment)
    CHECK(comm_check_exchange(so.data(), ro.data(), 3, 2, 0, p, p, sb, rb) == "comm_apply_exchange: a phase is 0 or 1");
    CHECK(comm_check_exchange(so.data(), ro.data(), 3, 0, -1, p, p, sb, rb) == "comm_apply_exchange: a phase is 0 or 1");
    CHECK(comm_check_exchange(nullptr, ro.data(), 3, 0, 0, p, p, sb, rb) == "comm_apply_exchange: null argument");
    CHECK(comm_check_exchange(so.data(), nullptr, 3, 0, 0, p, p, sb, rb) == "comm_apply_exchange: null argument");
    CHECK(comm_check_exchange(so.data(), ro.data(), 3, 0, 0, nullptr, p, sb, rb) == "comm_apply_exchange: null argument");
    CHECK(comm_check_exchange(so.data(), ro.data(), 3, 0, 0, p, nullptr, sb, rb) == "comm_apply_exchange: null argument");
    V ro_bad(ro);
    for (size_t k = 2 * 4 + 1; k < 3 * 4; ++k) ro_bad[k] += 1;  // rank 2 expects one more double from rank 0
    CHECK(comm_check_exchange(so.data(), ro_bad.data(), 3, 0, 0, p, p, sb, rb) ==
          "comm_apply_exchange: the plans disagree: rank 0 sends 1 doubles to rank 2, which receives 2 from it");
    V so_bad(so);
    so_bad[1 * 4 + 3] += 5;  // rank 1 sends 12 to rank 2
    CHECK(comm_check_exchange(so_bad.data(), ro.data(), 3, 0, 0, p, p, sb, rb) ==
          "comm_apply_exchange: the plans disagree: rank 1 sends 12 doubles to rank 2, which receives 7 from it");
    V so_down(so);
    so_down[1 * 4 + 2] = so_down[1 * 4 + 1] - 1;
    CHECK(comm_check_exchange(so_down.data(), ro.data(), 3, 0, 0, p, p, sb, rb) ==
          "comm_apply_exchange: rank 1: offsets must start at 0 or above and never decrease");
    V ro_neg(ro);
    ro_neg[2 * 4] = -1;
    CHECK(comm_check_exchange(so.data(), ro_neg.data(), 3, 0, 0, p, p, sb, rb) ==
          "comm_apply_exchange: rank 2: offsets must start at 0 or above and never decrease");
    const std::vector<V> none{{0, 0}, {0, 0}};
    plans(none, {0, 0}, {0, 0}, so, ro);
    CHECK(comm_check_exchange(so.data(), ro.data(), 2, 1, 1, p, p, sb, rb) == "" && (sb == V{0, 0, 0}) && (rb == V{0, 0, 0}));
    std::vector<V> eight(8, V(8, 0));  // the full table of 8 ranks
    for (int a = 0; a < 8; ++a)
      for (int b = 0; b < 8; ++b) eight[a][b] = (3 * a + b) % 5;
    plans(eight, V(8, 1), V(8, 0), so, ro);
    CHECK(comm_check_exchange(so.data(), ro.data(), 8, 0, 0, p, p, sb, rb) == "" && sb.size() == 9 && rb.size() == 9);
    int64_t all = 0;
    for (const V& row : eight)
      for (int64_t c : row) all += c;
    CHECK(sb[8] == all + 8 && rb[8] == all);
  }

  std::printf("%d checks, %d failed\n", checks, failed);
  if (failed) return 1;
  std::printf("comm apply host ok\n");
  return 0;
}
