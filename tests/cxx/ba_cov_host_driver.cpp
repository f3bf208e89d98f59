// ba_cov_host_driver.cpp -- the host logic of sim3opt_ba_covariances (sim3opt_amd/csrc/ba_cov_host.hpp) as a stand-alone
// program for the host sanitizers: the tables of a problem and the index lists of a request on a hand-built map of four
// cameras whose factor is a chain (so some camera pairs are outside its pattern): empty requests, duplicates,
// out-of-range indices, pairs outside the pattern and a point whose observers include a fixed camera.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "../../sim3opt_amd/csrc/ba_cov_host.hpp"

using namespace sim3opt_bundle;

static int g_checked = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    ++g_checked;                                                           \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #cond);       \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

int main() {
  // cameras 0 .. 3, camera 1 fixed.  Points: 0 seen by cameras 3, 1; 1 by 1, 0; 2 by 0, 2; 3 twice by 0 and once by 2;
  // 4 by the fixed camera 1 alone.
  const int32_t nc = 4, np = 5;
  const std::vector<int32_t> oc = {3, 1, 1, 0, 0, 2, 0, 0, 2, 1};
  const std::vector<int32_t> op = {0, 0, 1, 1, 2, 2, 3, 3, 3, 4};
  const std::vector<uint8_t> fixed = {0, 1, 0, 0};
  // the reduced system's pattern: cameras that share a point, the diagonal first, then ascending
  std::vector<std::set<int32_t>> nb(nc);
  for (size_t a = 0; a < oc.size(); ++a)
    for (size_t b = 0; b < oc.size(); ++b)
      if (op[a] == op[b] && oc[a] != oc[b]) nb[oc[a]].insert(oc[b]);
  std::vector<int32_t> rptr(1, 0), bcol;
  for (int32_t i = 0; i < nc; ++i) {
    bcol.push_back(i);
    for (int32_t j : nb[i]) bcol.push_back(j);
    rptr.push_back((int32_t)bcol.size());
  }
  // the factor: elimination order 3, 1, 0, 2 and a chain pattern (column j holds rows j and j + 1): exactly the pairs
  // (3, 1), (1, 0), (0, 2) and the diagonal
  const std::vector<int32_t> perm = {3, 1, 0, 2}, colptr = {0, 2, 4, 6, 7}, lrow = {0, 1, 1, 2, 2, 3, 3};
  const CovFactorPattern F{nc, perm.data(), colptr.data(), lrow.data()};

  CovTables T;
  CHECK(cov_build_tables(nc, np, oc, op, fixed, rptr, bcol, F, T).empty());
  CHECK((T.pptr == std::vector<int32_t>{0, 2, 4, 6, 9, 10}));
  CHECK((T.pobs == std::vector<int32_t>{0, 1, 2, 3, 4, 5, 6, 7, 8, 9}));
  CHECK((T.pos == std::vector<int32_t>{2, 1, 3, 0}));
  CHECK(T.sslot.size() == bcol.size());
  for (int32_t i = 0; i < nc; ++i)
    for (int32_t k = rptr[i]; k < rptr[i + 1]; ++k) {
      const int32_t j = bcol[k], hi = std::max(T.pos[i], T.pos[j]), lo = std::min(T.pos[i], T.pos[j]);
      CHECK(lrow[T.sslot[k]] == hi && T.sslot[k] >= colptr[lo] && T.sslot[k] < colptr[lo + 1]);
      CHECK(T.strans[k] == (T.pos[i] < T.pos[j] ? 1 : 0));
      CHECK(T.smask[k] == ((i == 1 || j == 1) ? 1 : 0));
    }
  // a pattern the factor does not cover is an internal error, said so
  {
    const std::vector<int32_t> colptr2 = {0, 1, 2, 3, 4}, lrow2 = {0, 1, 2, 3};
    const CovFactorPattern G{nc, perm.data(), colptr2.data(), lrow2.data()};
    CovTables U;
    CHECK(!cov_build_tables(nc, np, oc, op, fixed, rptr, bcol, G, U).empty());
    const CovFactorPattern H{3, perm.data(), colptr.data(), lrow.data()};
    CHECK(!cov_build_tables(nc, np, oc, op, fixed, rptr, bcol, H, U).empty());
  }

  CovRequest R;
  // ---- empty requests (NULL arrays) ----
  CHECK(cov_plan_request(T, F, oc, fixed, 0, nullptr, nullptr, 0, nullptr, 0, nullptr, nullptr, R).empty());
  CHECK(R.slot.empty() && R.upoint.empty() && R.xptr == std::vector<int32_t>{0} && R.xobs.empty() && R.pair_terms == 0);
  CHECK(R.cc_where.empty() && R.pp_where.empty() && R.pc_where.empty());

  // ---- camera pairs: duplicates share a pick, the reversed pair is the same slot read transposed, a pair with a
  // fixed camera is masked whether the factor stores it or not ----
  {
    const int32_t a[] = {0, 0, 2, 1, 1, 3, 0}, b[] = {2, 2, 0, 2, 0, 3, 0};
    CHECK(cov_plan_request(T, F, oc, fixed, 7, a, b, 0, nullptr, 0, nullptr, nullptr, R).empty());
    CHECK((R.cc_where == std::vector<int32_t>{0, 0, 1, 2, 3, 4, 5}));
    CHECK(R.slot.size() == 6 && R.slot[0] == R.slot[1] && R.trans[0] != R.trans[1]);
    CHECK(R.trans[0] == 1 && lrow[R.slot[0]] == 3);  // (0, 2): positions 2 < 3
    CHECK((R.mask == std::vector<int32_t>{0, 0, 1, 1, 0, 0}));
    CHECK(R.slot[4] == colptr[0] && R.slot[5] == colptr[2]);  // diagonal blocks of cameras 3 and 0
  }
  // ---- a pair outside the pattern, unknown cameras ----
  {
    const int32_t a[] = {0, 3}, b[] = {0, 2};
    const std::string why = cov_plan_request(T, F, oc, fixed, 2, a, b, 0, nullptr, 0, nullptr, nullptr, R);
    CHECK(why.find("camera pair 1 (3, 2)") != std::string::npos && why.find("outside the pattern") != std::string::npos);
    for (int32_t bad : {-1, 4, 1 << 30, -(1 << 30)}) {
      const int32_t x[] = {0, bad}, y[] = {bad, 0};
      CHECK(cov_plan_request(T, F, oc, fixed, 2, x, y, 0, nullptr, 0, nullptr, nullptr, R).find("unknown camera") !=
            std::string::npos);
    }
  }
  // ---- points: duplicates, the pairs a point sums (fixed observers left out), unknown points ----
  {
    const int32_t p[] = {3, 0, 3, 4};
    CHECK(cov_plan_request(T, F, oc, fixed, 0, nullptr, nullptr, 4, p, 0, nullptr, nullptr, R).empty());
    CHECK((R.upoint == std::vector<int32_t>{3, 0, 4}) && (R.pp_where == std::vector<int32_t>{0, 1, 0, 2}));
    CHECK(R.pair_terms == 9 + 1 + 0);
    for (int32_t bad : {-1, 5, 1 << 30}) {
      const int32_t q[] = {0, bad};
      CHECK(cov_plan_request(T, F, oc, fixed, 0, nullptr, nullptr, 2, q, 0, nullptr, nullptr, R).find("unknown point") !=
            std::string::npos);
    }
  }
  // ---- point-camera blocks: a point whose observers include a fixed camera, a fixed camera asked for, a camera that
  // does not observe the point (on the pattern, and outside it), duplicates, unknown indices ----
  {
    const int32_t p[] = {0, 0, 1, 0, 3}, c[] = {3, 1, 2, 3, 0};
    CHECK(cov_plan_request(T, F, oc, fixed, 0, nullptr, nullptr, 0, nullptr, 5, p, c, R).empty());
    CHECK((R.pc_where == std::vector<int32_t>{0, -1, 1, 0, 2}));
    CHECK((R.xptr == std::vector<int32_t>{0, 2, 4, 7}));
    CHECK((R.xobs == std::vector<int32_t>{0, 1, 2, 3, 6, 7, 8}));
    CHECK(R.xpick[0] >= 0 && R.xpick[1] == -1);  // point 0: camera 3 free, camera 1 fixed
    CHECK(R.xpick[2] == -1 && R.xpick[3] >= 0);  // point 1: camera 1 fixed, then (0, 2)
    CHECK(R.xpick[4] == R.xpick[5] && R.xpick[4] >= 0 && R.xpick[6] >= 0 && R.xpick[6] != R.xpick[4]);  // (0,0) twice, (2,0)
    for (int32_t w : R.xpick) CHECK(w < (int32_t)R.slot.size());
    CHECK(R.slot.size() == R.trans.size() && R.slot.size() == R.mask.size());
    const int32_t p2[] = {2}, c2[] = {3};  // point 2 is seen by cameras 0 and 2: (0, 3) is outside the chain
    const std::string why = cov_plan_request(T, F, oc, fixed, 0, nullptr, nullptr, 0, nullptr, 1, p2, c2, R);
    CHECK(why.find("outside the pattern") != std::string::npos);
    const int32_t bp[] = {5, 0, -1, 0}, bc[] = {0, 4, 0, -1};
    for (int k = 0; k < 4; ++k)
      CHECK(cov_plan_request(T, F, oc, fixed, 0, nullptr, nullptr, 0, nullptr, 1, bp + k, bc + k, R)
                .find("unknown point or camera") != std::string::npos);
  }
  // ---- the three kinds together share the pick list ----
  {
    const int32_t a[] = {0}, b[] = {2}, pt[] = {1}, p[] = {1}, c[] = {2};
    CHECK(cov_plan_request(T, F, oc, fixed, 1, a, b, 1, pt, 1, p, c, R).empty());
    CHECK(R.slot.size() == 1 && R.cc_where[0] == 0 && R.xpick[1] == 0 && R.xpick[0] == -1 && R.pair_terms == 1);
  }
  std::printf("%d checks\nba cov host ok\n", g_checked);
  return 0;
}
