// ba_cov_host.hpp -- the host side of sim3opt_ba_covariances (ba.hip): the tables a problem needs once and the index
// lists of one request.  Plain C++ with no HIP in it, so tests/cxx/ba_cov_host_driver.cpp runs it under the host
// sanitizers.
//
// The selected inversion leaves Z = S^-1 on the pattern of the factor L, stored as the lower triangle in elimination
// order (direct.hpp: colptr / lrow, positions through perm).  Block (a, b) of Sigma_cc is slot (max(pos a, pos b),
// min(pos a, pos b)), transposed when pos a < pos b.
//   once per problem   CovTables: the points' observation lists and, for every block of the reduced system S
//                      (block-CSR rptr / bcol, the diagonal block first in every row), its slot, whether it is read
//                      transposed, and whether a fixed camera masks it
//   per request        CovRequest: the distinct points asked for; one pick list (slot, transposed, masked) for the
//                      camera pairs asked for and for the terms of the point-camera blocks, which may lie in the
//                      factor's fill where S has no block; the terms of every distinct point-camera block.  Everything
//                      is proportional to the request, nothing to the number of points.
#pragma once

#include <algorithm>
#include <cstdint>
#include <string>
#include <unordered_map>
#include <vector>

namespace sim3opt_bundle {

struct CovFactorPattern {  // views into a DirectPlan
  int32_t nb = 0;
  const int32_t* perm = nullptr;    // perm[j] = camera eliminated at position j
  const int32_t* colptr = nullptr;  // nb + 1
  const int32_t* lrow = nullptr;    // rows of a column ascending, the diagonal first
};

struct CovTables {
  int32_t nc = 0, np = 0;
  std::vector<int32_t> pptr, pobs;  // observations of point p: pobs[pptr[p] .. pptr[p + 1]), ascending
  std::vector<int32_t> pos;         // elimination position of a camera
  std::vector<int32_t> sslot, strans, smask;  // per block of S
};

// slot of Z(a, b), or false when the pair is outside the factor's pattern
inline bool cov_find_slot(const CovFactorPattern& F, const std::vector<int32_t>& pos, int32_t a, int32_t b, int32_t& slot,
                          int32_t& trans) {
  const int32_t pa = pos[a], pb = pos[b];
  const int32_t i = std::max(pa, pb), j = std::min(pa, pb);
  const int32_t* first = F.lrow + F.colptr[j];
  const int32_t* last = F.lrow + F.colptr[j + 1];
  const int32_t* it = std::lower_bound(first, last, i);
  if (it == last || *it != i) return false;
  slot = (int32_t)(it - F.lrow);
  trans = pa < pb ? 1 : 0;
  return true;
}

// "" or what is wrong (an internal error: every block of S is a block of the factor)
inline std::string cov_build_tables(int32_t nc, int32_t np, const std::vector<int32_t>& oc, const std::vector<int32_t>& op,
                                    const std::vector<uint8_t>& fixed, const std::vector<int32_t>& rptr,
                                    const std::vector<int32_t>& bcol, const CovFactorPattern& F, CovTables& T) {
  T = CovTables();
  T.nc = nc;
  T.np = np;
  const size_t no = oc.size();
  T.pptr.assign((size_t)np + 1, 0);
  T.pobs.resize(no);
  for (size_t o = 0; o < no; ++o) ++T.pptr[(size_t)op[o] + 1];
  for (int32_t p = 0; p < np; ++p) T.pptr[(size_t)p + 1] += T.pptr[p];
  {
    std::vector<int32_t> fill(T.pptr.begin(), T.pptr.end() - 1);
    for (size_t o = 0; o < no; ++o) T.pobs[fill[op[o]]++] = (int32_t)o;
  }
  if (F.nb != nc) return "the factor's plan has another number of columns than the problem has cameras";
  T.pos.assign(nc, 0);
  for (int32_t j = 0; j < nc; ++j) T.pos[F.perm[j]] = j;
  const size_t nblk = bcol.size();
  T.sslot.resize(nblk);
  T.strans.resize(nblk);
  T.smask.resize(nblk);
  for (int32_t i = 0; i < nc; ++i)
    for (int32_t k = rptr[i]; k < rptr[i + 1]; ++k) {
      if (!cov_find_slot(F, T.pos, i, bcol[k], T.sslot[k], T.strans[k]))
        return "a block of the reduced system is not on the factor's pattern";
      T.smask[k] = (fixed[i] | fixed[bcol[k]]) ? 1 : 0;
    }
  return "";
}

struct CovRequest {
  // points: the distinct ones in order of first use; request q is upoint[pp_where[q]]
  std::vector<int32_t> upoint, pp_where;
  // the pick list: blocks of Z the call reads besides those of S
  std::vector<int32_t> slot, trans, mask;
  std::vector<int32_t> cc_where;  // camera-pair request q is pick cc_where[q]
  // point-camera blocks: the distinct ones; block u sums terms xptr[u] .. xptr[u + 1): observation xobs[t] with pick
  // xpick[t] (-1: a fixed camera, the term contributes nothing); request q is block pc_where[q], -1: c is fixed (+0)
  std::vector<int32_t> xptr, xobs, xpick, pc_where;
  int64_t pair_terms = 0;  // ordered observation pairs the distinct points sum (fixed cameras left out)
};

// Plans one request.  "" when it can be answered; else the message of SIM3OPT_ERR_ARG (nothing is written then).
inline std::string cov_plan_request(const CovTables& T, const CovFactorPattern& F, const std::vector<int32_t>& oc,
                                    const std::vector<uint8_t>& fixed, int32_t n_cc, const int32_t* cam_a,
                                    const int32_t* cam_b, int32_t n_pp, const int32_t* point, int32_t n_pc,
                                    const int32_t* pc_point, const int32_t* pc_cam, CovRequest& R) {
  R = CovRequest();
  const int64_t nc = T.nc, np = T.np;
  for (int32_t q = 0; q < n_cc; ++q)
    if (cam_a[q] < 0 || cam_a[q] >= nc || cam_b[q] < 0 || cam_b[q] >= nc)
      return "camera pair " + std::to_string(q) + ": unknown camera";
  for (int32_t q = 0; q < n_pp; ++q)
    if (point[q] < 0 || point[q] >= np) return "point request " + std::to_string(q) + ": unknown point";
  for (int32_t q = 0; q < n_pc; ++q)
    if (pc_point[q] < 0 || pc_point[q] >= np || pc_cam[q] < 0 || pc_cam[q] >= nc)
      return "point-camera request " + std::to_string(q) + ": unknown point or camera";

  std::unordered_map<int64_t, int32_t> picked;  // a * nc + b -> pick
  auto pick = [&](int32_t a, int32_t b, int32_t& out) {
    if (fixed[a] | fixed[b]) {  // masked: exactly +0 whatever the factor holds there
      const auto ins = picked.emplace((int64_t)a * nc + b, (int32_t)R.slot.size());
      if (ins.second) { R.slot.push_back(0); R.trans.push_back(0); R.mask.push_back(1); }
      out = ins.first->second;
      return true;
    }
    const auto found = picked.find((int64_t)a * nc + b);
    if (found != picked.end()) { out = found->second; return true; }
    int32_t s = 0, t = 0;
    if (!cov_find_slot(F, T.pos, a, b, s, t)) return false;
    out = (int32_t)R.slot.size();
    picked.emplace((int64_t)a * nc + b, out);
    R.slot.push_back(s); R.trans.push_back(t); R.mask.push_back(0);
    return true;
  };

  R.cc_where.resize(n_cc > 0 ? n_cc : 0);
  for (int32_t q = 0; q < n_cc; ++q)
    if (!pick(cam_a[q], cam_b[q], R.cc_where[q]))
      return "camera pair " + std::to_string(q) + " (" + std::to_string(cam_a[q]) + ", " + std::to_string(cam_b[q]) +
             "): outside the pattern of the factor (not a camera with itself, nor two cameras that share a point)";

  std::unordered_map<int32_t, int32_t> upos;
  R.pp_where.resize(n_pp > 0 ? n_pp : 0);
  for (int32_t q = 0; q < n_pp; ++q) {
    const auto ins = upos.emplace(point[q], (int32_t)R.upoint.size());
    if (ins.second) {
      R.upoint.push_back(point[q]);
      int64_t nfree = 0;
      for (int32_t k = T.pptr[point[q]]; k < T.pptr[point[q] + 1]; ++k) nfree += fixed[oc[T.pobs[k]]] ? 0 : 1;
      R.pair_terms += nfree * nfree;
    }
    R.pp_where[q] = ins.first->second;
  }

  std::unordered_map<int64_t, int32_t> xpos;  // p * nc + c -> block
  R.xptr.assign(1, 0);
  R.pc_where.resize(n_pc > 0 ? n_pc : 0);
  for (int32_t q = 0; q < n_pc; ++q) {
    const int32_t p = pc_point[q], c = pc_cam[q];
    if (fixed[c]) { R.pc_where[q] = -1; continue; }
    const auto found = xpos.find((int64_t)p * nc + c);
    if (found != xpos.end()) { R.pc_where[q] = found->second; continue; }
    for (int32_t k = T.pptr[p]; k < T.pptr[p + 1]; ++k) {
      const int32_t o = T.pobs[k], a = oc[o];
      int32_t w = -1;
      if (!fixed[a] && !pick(a, c, w))
        return "point-camera request " + std::to_string(q) + " (" + std::to_string(p) + ", " + std::to_string(c) +
               "): the pair of cameras (" + std::to_string(a) + ", " + std::to_string(c) +
               ") is outside the pattern of the factor";
      R.xobs.push_back(o);
      R.xpick.push_back(fixed[a] ? -1 : w);
    }
    R.pc_where[q] = (int32_t)R.xptr.size() - 1;
    xpos.emplace((int64_t)p * nc + c, R.pc_where[q]);
    R.xptr.push_back((int32_t)R.xobs.size());
  }
  return "";
}

}  // namespace sim3opt_bundle
