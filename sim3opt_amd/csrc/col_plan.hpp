// col_plan.hpp -- which vertices' columns of (H + lambda I)^-1 a request of blocks needs (host only; shared by
// capi.cpp's diagnostic sim3opt_covariance_columns_plan and Engine::cov_blocks_columns, engine_columns.hip).
// Block (a, b) of the inverse is rows a of the seven columns of b -- or, transposed, rows b of the columns of a -- so
// every requested unordered pair {a, b} needs ONE of its endpoints solved and a pair (a, a) needs a: a vertex cover of
// the request's pair graph.  Greedy and deterministic: repeatedly the vertex that covers the most pairs not yet
// covered, ties to the lowest block row.  A full block column (every vertex against b) costs the one vertex b.
#pragma once

#include <algorithm>
#include <cstdint>
#include <queue>
#include <unordered_map>
#include <utility>
#include <vector>

namespace sim3opt {

struct ColumnCover {
  std::vector<int32_t> chosen;                     // block rows whose columns are solved, in the order chosen
  std::vector<std::pair<int32_t, int32_t>> pairs;  // distinct unordered pairs (lo, hi) of block rows, first use
  std::vector<int32_t> owner;                      // per pair: position in `chosen` of the endpoint that covers it
  std::vector<int32_t> pair_of;                    // per request entry: its pair, -1 for an entry with a row < 0
};

// rows < 0 (a fixed endpoint of a gate candidate: a zero block) take no part
inline void covariance_columns_cover(int32_t nb, int32_t n, const int32_t* row_a, const int32_t* row_b, ColumnCover& C) {
  C = ColumnCover();
  C.pair_of.assign(std::max(n, 0), -1);
  std::unordered_map<int64_t, int32_t> index;
  for (int32_t q = 0; q < n; ++q) {
    if (row_a[q] < 0 || row_b[q] < 0) continue;
    const int32_t lo = std::min(row_a[q], row_b[q]), hi = std::max(row_a[q], row_b[q]);
    const auto ins = index.emplace((int64_t)lo * nb + hi, (int32_t)C.pairs.size());
    if (ins.second) C.pairs.push_back({lo, hi});
    C.pair_of[q] = ins.first->second;
  }
  const int32_t np = (int32_t)C.pairs.size();
  C.owner.assign(np, -1);
  // pairs incident to a vertex (a pair (a, a) once), and how many of them are not covered yet
  std::vector<int32_t> cnt(nb, 0), ptr(nb + 1, 0), inc;
  for (const auto& p : C.pairs) {
    ++cnt[p.first];
    if (p.second != p.first) ++cnt[p.second];
  }
  for (int32_t v = 0; v < nb; ++v) ptr[v + 1] = ptr[v] + cnt[v];
  inc.resize(ptr[nb]);
  {
    std::vector<int32_t> fill(ptr.begin(), ptr.end() - 1);
    for (int32_t k = 0; k < np; ++k) {
      inc[fill[C.pairs[k].first]++] = k;
      if (C.pairs[k].second != C.pairs[k].first) inc[fill[C.pairs[k].second]++] = k;
    }
  }
  // (count, -row): the largest count first, the lowest row among equals; an entry whose count is out of date is dropped
  std::priority_queue<std::pair<int32_t, int32_t>> heap;
  for (int32_t v = 0; v < nb; ++v)
    if (cnt[v] > 0) heap.push({cnt[v], -v});
  while (!heap.empty()) {
    const int32_t c = heap.top().first, v = -heap.top().second;
    heap.pop();
    if (c != cnt[v] || c == 0) continue;
    const int32_t pos = (int32_t)C.chosen.size();
    C.chosen.push_back(v);
    for (int32_t i = ptr[v]; i < ptr[v + 1]; ++i) {
      const int32_t k = inc[i];
      if (C.owner[k] >= 0) continue;
      C.owner[k] = pos;
      const int32_t u = C.pairs[k].first == v ? C.pairs[k].second : C.pairs[k].first;
      if (u != v && --cnt[u] > 0) heap.push({cnt[u], -u});
    }
    cnt[v] = 0;
  }
}

}  // namespace sim3opt
