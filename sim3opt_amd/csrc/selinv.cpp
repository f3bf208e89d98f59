// selinv.cpp -- product lists of the block selected inversion (see direct.hpp, selinv_kernels.hpp).  Host only.
//
// (H + lambda I) = L L^T in elimination order; S_j = the below-diagonal rows of block column j.  Let
// Z = (H + lambda I)^-1.  From Z L = L^-T, whose blocks below the diagonal vanish and whose diagonal block j
// is L(j,j)^-T, column j of Z L reads
//   i in S_j:  Z(i,j) L(j,j) + sum_{k in S_j} Z(i,k) L(k,j) = 0
//   i = j:     Z(j,j) L(j,j) + sum_{k in S_j} Z(j,k) L(k,j) = L(j,j)^-T
// so, with Z(i,k) = Z(k,i)^T where k > i,
//   Z(i,j) = -( sum_k Z(i,k) L(k,j) ) L(j,j)^-1
//   Z(j,j) = ( L(j,j)^-T - sum_k Z(k,j)^T L(k,j) ) L(j,j)^-1     (needs the column's off-diagonal blocks first)
// Every Z(i,k) read has i, k in S_j: both are ancestors of j in the elimination tree and S_j is a clique of
// the filled pattern, so the blocks of Z on the pattern of L are closed under the recursion and the walk is
// the backward solve's: levels top-down, columns of a level independent.
#include <algorithm>

#include "direct.hpp"

namespace sim3opt {

bool build_selinv_plan(const DirectPlan& P, SelinvPlan& S, std::string& why) {
  S = SelinvPlan();
  const int32_t nb = P.nb;
  auto slot = [&](int32_t i, int32_t j) -> int32_t {  // block (i, j), i >= j; -1 if not stored
    if (i == j) return P.colptr[j];
    const auto b = P.lrow.begin() + P.colptr[j] + 1, e = P.lrow.begin() + P.colptr[j + 1];
    const auto it = std::lower_bound(b, e, i);
    return it == e || *it != i ? -1 : (int32_t)(it - P.lrow.begin());
  };
  S.zptr.assign(P.nL + 1, 0);
  for (int32_t j = 0; j < nb; ++j) {
    const int32_t n = P.colptr[j + 1] - P.colptr[j] - 1;  // |S_j|: every block of the column has that many
    for (int32_t s = P.colptr[j]; s < P.colptr[j + 1]; ++s) S.zptr[s + 1] = n;
  }
  for (int64_t s = 0; s < P.nL; ++s) S.zptr[s + 1] += S.zptr[s];
  S.nprod = S.zptr[P.nL];
  S.za.resize(S.nprod);
  S.zt.resize(S.nprod);
  S.zl.resize(S.nprod);
  for (int32_t j = 0; j < nb; ++j) {
    const int32_t s0 = P.colptr[j], s1 = P.colptr[j + 1];
    for (int32_t s = s0; s < s1; ++s) {
      const int32_t i = P.lrow[s];
      int32_t p = S.zptr[s];
      for (int32_t t = s0 + 1; t < s1; ++t) {  // k in the backward solve's order (bord / brow)
        const int32_t k = P.brow[t], lk = P.bord[t];
        int32_t z;
        bool tr;
        if (i == j) { z = lk; tr = true; }            // Z(k,j)^T
        else if (k == i) { z = P.colptr[i]; tr = false; }  // Z(i,i)
        else if (k < i) { z = slot(i, k); tr = false; }
        else { z = slot(k, i); tr = true; }
        if (z < 0) { why = "internal: the selected inverse reads a block outside the pattern of L"; return false; }
        S.za[p] = z;
        S.zt[p] = tr ? 1 : 0;
        S.zl[p] = lk;
        ++p;
      }
    }
  }
  return true;
}

}  // namespace sim3opt
