// vocab_host.hpp -- the host half of the batched vocabulary training (vocab_train.hip): the tile sizes, the checks of
// the options and of the frames with their messages, the tables of a level (its nodes, their chunks), the assembly of
// the per-level results into the four arrays sim3opt_place_batch_set_vocabulary takes, the weights, and the file a
// trained tree is saved in.  Plain C++ with no HIP in it, so tests/cxx/vocab_host_driver.cpp runs it under the host
// sanitizers.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/sim3opt.h"
#include "handle_host.hpp"
#include "place_host.hpp"

#if defined(__HIP__)
#include <hip/hip_runtime.h>
#define SIM3OPT_VOCAB_HD __host__ __device__ inline
#else
#define SIM3OPT_VOCAB_HD inline
#endif

namespace sim3opt_vocab {

constexpr int DESC = sim3opt_place::DESC;
constexpr int CHUNK = 256;        // members of a node one workgroup takes (a lane each): assignment, seeding, partition
constexpr int MEAN_CHUNK = 1024;  // members of a node whose coordinates one wavefront adds one after the other
constexpr int MAX_K = 64;         // options.k's upper limit: the children of a node in sim3opt_place_batch_set_vocabulary
constexpr int MAX_LEVELS = 8;     // options.levels' upper limit

// every refusal, word for word
constexpr const char* MSG_K = "k outside 2..64";
constexpr const char* MSG_LEVELS = "levels outside 1..8";
constexpr const char* MSG_ITERS = "max_iters < 1";
constexpr const char* MSG_IDF = "idf is neither 0 nor 1";
constexpr const char* MSG_DISTINCT = "fewer than two distinct descriptors";
constexpr const char* MSG_TOO_MANY_NODES = "the tree would hold more nodes than an index of sim3opt_place_batch_set_vocabulary allows";
constexpr const char* MSG_FILE_OPEN = "cannot open the file";
constexpr const char* MSG_FILE_MAGIC = "not a sim3opt vocabulary file (magic)";
constexpr const char* MSG_FILE_VERSION = "a sim3opt vocabulary file of another version";
constexpr const char* MSG_FILE_COUNTS = "a sim3opt vocabulary file with impossible counts";
constexpr const char* MSG_FILE_TRUNCATED = "a truncated sim3opt vocabulary file";
constexpr const char* MSG_FILE_WRITE = "cannot write the file";

enum Kind : int32_t { LEAF = 0, SMALL = 1, BIG = 2 };  // of a node at its level: no split, n <= k, k-means

inline std::string validate_options(const sim3opt_vocabulary_options& o) {
  if (o.k < 2 || o.k > MAX_K) return MSG_K;
  if (o.levels < 1 || o.levels > MAX_LEVELS) return MSG_LEVELS;
  if (o.max_iters < 1) return MSG_ITERS;
  if (o.idf != 0 && o.idf != 1) return MSG_IDF;
  return "";
}

// the set_frames refusals of place recognition, and a training set in which a tree of two nodes exists
inline std::string validate_frames(int32_t n_frames, const int32_t* kp_ptr, const float* desc) {
  const std::string e = sim3opt_place::validate_frames(n_frames, kp_ptr, desc);
  if (!e.empty()) return e;
  const size_t n = (size_t)kp_ptr[n_frames];
  for (size_t i = 1; i < n; ++i)
    if (std::memcmp(desc, desc + i * DESC, sizeof(float) * DESC) != 0) {
      // (+0 and -0 differ as bytes and not as numbers: d2 between them is 0)
      for (int k = 0; k < DESC; ++k)
        if (desc[k] != desc[i * DESC + k]) return "";
    }
  return MSG_DISTINCT;
}

// The seeding's draw for (seed, node, c): the key holds those three only.
SIM3OPT_VOCAB_HD uint64_t seed_key(uint64_t seed, int32_t node, int32_t c) {
  return seed + ((uint64_t)MAX_K * (uint64_t)node + (uint64_t)c + 1) * 0x9E3779B97F4A7C15ull;
}

// The nodes of one level as the kernels read them.  The members of node t are perm[start[t] .. start[t] + count[t]) in
// ascending descriptor index; a node is cut into chunks of CHUNK members and into mean chunks of MEAN_CHUNK members.
struct Level {
  int32_t first_node = 0;                  // the output index of node 0 of the level
  std::vector<int32_t> start, count, kind;  // per node
  std::vector<int32_t> chunk_node, chunk_start, chunk_len, node_chunk0, node_nchunks;
  std::vector<int32_t> mchunk_node, mchunk_start, mchunk_len, mchunk_slot, node_mchunk0, node_nmchunks;
  std::vector<int32_t> multi;  // the nodes of more than one mean chunk; their chunks own the slots of the partial sums
  int32_t n_slots = 0, n_members = 0;
  int32_t T() const { return (int32_t)count.size(); }
};

// start, the kinds and both chunk tables from the counts (level == levels: every node is a leaf)
inline void plan_level(Level& V, int32_t level, int32_t levels, int32_t k) {
  const size_t T = V.count.size();
  V.start.assign(T, 0); V.kind.assign(T, LEAF);
  V.node_chunk0.assign(T, 0); V.node_nchunks.assign(T, 0); V.node_mchunk0.assign(T, 0); V.node_nmchunks.assign(T, 0);
  V.chunk_node.clear(); V.chunk_start.clear(); V.chunk_len.clear();
  V.mchunk_node.clear(); V.mchunk_start.clear(); V.mchunk_len.clear(); V.mchunk_slot.clear(); V.multi.clear();
  V.n_slots = 0;
  int32_t pos = 0;
  for (size_t t = 0; t < T; ++t) {
    const int32_t n = V.count[t];
    V.start[t] = pos;
    V.kind[t] = (n <= 1 || level >= levels) ? LEAF : n <= k ? SMALL : BIG;
    V.node_chunk0[t] = (int32_t)V.chunk_node.size();
    for (int32_t o = 0; o < n; o += CHUNK) {
      V.chunk_node.push_back((int32_t)t); V.chunk_start.push_back(pos + o); V.chunk_len.push_back(n - o < CHUNK ? n - o : CHUNK);
    }
    V.node_nchunks[t] = (int32_t)V.chunk_node.size() - V.node_chunk0[t];
    V.node_mchunk0[t] = (int32_t)V.mchunk_node.size();
    if (V.kind[t] == BIG) {
      const bool multi = n > MEAN_CHUNK;
      if (multi) V.multi.push_back((int32_t)t);
      for (int32_t o = 0; o < n; o += MEAN_CHUNK) {
        V.mchunk_node.push_back((int32_t)t); V.mchunk_start.push_back(pos + o);
        V.mchunk_len.push_back(n - o < MEAN_CHUNK ? n - o : MEAN_CHUNK);
        V.mchunk_slot.push_back(multi ? V.n_slots++ : -1);
      }
    }
    V.node_nmchunks[t] = (int32_t)V.mchunk_node.size() - V.node_mchunk0[t];
    pos += n;
  }
  V.n_members = pos;
}

// The tree as it grows, level by level, in the output's numbering (breadth first; within a level by parent, then cluster).
struct Tree {
  std::vector<int32_t> parent, word_id, level;
  std::vector<float> centre;
  std::vector<double> weight;
  int32_t n_nodes() const { return (int32_t)parent.size(); }
  void start() {
    parent.assign(1, -1); level.assign(1, 0); centre.assign(DESC, 0.f);
    word_id.clear(); weight.clear();
  }
};

// Appends the children of level V: child (t, c) exists when child_count[t * k + c] > 0 and its centre is
// centres[(t * k + c) * DESC ..].  Returns the counts of the next level's nodes in their order; "" or a refusal in err.
inline std::vector<int32_t> append_children(Tree& R, const Level& V, int32_t level, int32_t k,
                                            const std::vector<int32_t>& child_count, const std::vector<float>& centres,
                                            std::vector<int32_t>& child_start, std::string& err) {
  std::vector<int32_t> next;
  child_start.assign(child_count.size(), 0);
  int32_t pos = 0;
  for (int32_t t = 0; t < V.T(); ++t) {
    if (V.kind[(size_t)t] == LEAF) continue;
    for (int32_t c = 0; c < k; ++c) {
      const size_t s = (size_t)t * k + c;
      child_start[s] = pos;
      if (child_count[s] <= 0) continue;
      if (R.parent.size() >= (size_t)(INT32_MAX / DESC)) { err = MSG_TOO_MANY_NODES; return {}; }
      R.parent.push_back(V.first_node + t);
      R.level.push_back(level + 1);
      R.centre.insert(R.centre.end(), centres.begin() + (ptrdiff_t)(s * DESC), centres.begin() + (ptrdiff_t)((s + 1) * DESC));
      next.push_back(child_count[s]);
      pos += child_count[s];
    }
  }
  return next;
}

// word_id: the leaves counted in ascending node index, -1 at inner nodes; the children tables place recognition's
// descent reads (the numbering is breadth first already, so a node's children are consecutive).  Returns n_words.
inline int32_t finish_tree(Tree& R, std::vector<int32_t>& first_child, std::vector<int32_t>& n_child, int32_t& depth) {
  const size_t N = R.parent.size();
  first_child.assign(N, 0); n_child.assign(N, 0);
  for (size_t i = 1; i < N; ++i) {
    const size_t p = (size_t)R.parent[i];
    if (n_child[p]++ == 0) first_child[p] = (int32_t)i;
  }
  R.word_id.assign(N, -1);
  R.weight.assign(N, 0.0);
  int32_t w = 0;
  depth = 0;
  for (size_t i = 0; i < N; ++i)
    if (n_child[i] == 0) {
      R.word_id[i] = w++;
      if (R.level[i] > depth) depth = R.level[i];
    }
  return w;
}

// weight = log(N / N_i): N the frames with a descriptor, N_i those with a descriptor whose descent ends in leaf i
// (descent_node: per descriptor, the node place recognition's descent reaches); 0 for a leaf no descent reaches; 1 at
// every leaf with idf == 0.
inline void idf_weights(Tree& R, int32_t n_frames, const int32_t* kp_ptr, const int32_t* descent_node, int32_t idf) {
  const size_t N = R.parent.size();
  std::vector<int32_t> seen(N, -1), ni(N, 0);
  int32_t n_with = 0;
  for (int32_t f = 0; f < n_frames; ++f) {
    if (kp_ptr[f + 1] > kp_ptr[f]) ++n_with;
    for (int32_t d = kp_ptr[f]; d < kp_ptr[f + 1]; ++d) {
      const size_t i = (size_t)descent_node[d];
      if (seen[i] != f) { seen[i] = f; ++ni[i]; }
    }
  }
  for (size_t i = 0; i < N; ++i) {
    if (R.word_id[i] < 0) { R.weight[i] = 0.0; continue; }
    R.weight[i] = !idf ? 1.0 : ni[i] > 0 ? std::log((double)n_with / (double)ni[i]) : 0.0;
  }
}

// ---- the file: "SIM3VOC\0", version, n_nodes, DESC (int32 each), then parent, centre, weight, word_id as they are
constexpr char FILE_MAGIC[8] = {'S', 'I', 'M', '3', 'V', 'O', 'C', '\0'};
constexpr int32_t FILE_VERSION = 1;

inline std::string save_file(const char* path, int32_t n_nodes, const int32_t* parent, const float* centre,
                             const double* weight, const int32_t* word_id) {
  if (!path || !parent || !centre || !weight || !word_id) return "a NULL argument";
  if (n_nodes < 2 || n_nodes > INT32_MAX / DESC) return MSG_FILE_COUNTS;
  std::FILE* f = std::fopen(path, "wb");
  if (!f) return MSG_FILE_OPEN;
  const size_t N = (size_t)n_nodes;
  const int32_t head[3] = {FILE_VERSION, n_nodes, DESC};
  bool ok = std::fwrite(FILE_MAGIC, 1, 8, f) == 8 && std::fwrite(head, sizeof(int32_t), 3, f) == 3 &&
            std::fwrite(parent, sizeof(int32_t), N, f) == N && std::fwrite(centre, sizeof(float), N * DESC, f) == N * DESC &&
            std::fwrite(weight, sizeof(double), N, f) == N && std::fwrite(word_id, sizeof(int32_t), N, f) == N;
  ok = (std::fclose(f) == 0) && ok;
  return ok ? "" : MSG_FILE_WRITE;
}

inline std::string load_file(const char* path, std::vector<int32_t>& parent, std::vector<float>& centre,
                             std::vector<double>& weight, std::vector<int32_t>& word_id) {
  if (!path) return "a NULL argument";
  std::FILE* f = std::fopen(path, "rb");
  if (!f) return MSG_FILE_OPEN;
  char magic[8];
  int32_t head[3];
  std::string e;
  if (std::fread(magic, 1, 8, f) != 8) e = MSG_FILE_TRUNCATED;
  else if (std::memcmp(magic, FILE_MAGIC, 8) != 0) e = MSG_FILE_MAGIC;
  else if (std::fread(head, sizeof(int32_t), 3, f) != 3) e = MSG_FILE_TRUNCATED;
  else if (head[0] != FILE_VERSION) e = MSG_FILE_VERSION;
  else if (head[1] < 2 || head[1] > INT32_MAX / DESC || head[2] != DESC) e = MSG_FILE_COUNTS;
  if (e.empty()) {
    // the length the counts promise, before anything of that size is reserved
    const size_t N = (size_t)head[1];
    const long want = (long)(20 + N * (sizeof(int32_t) * 2 + sizeof(double) + sizeof(float) * DESC));
    if (std::fseek(f, 0, SEEK_END) != 0 || std::ftell(f) < want) e = MSG_FILE_TRUNCATED;
    else if (std::ftell(f) != want) e = MSG_FILE_COUNTS;
    else {
      std::fseek(f, 20, SEEK_SET);
      std::vector<int32_t> p(N), w(N);
      std::vector<float> c(N * DESC);
      std::vector<double> g(N);
      if (std::fread(p.data(), sizeof(int32_t), N, f) != N || std::fread(c.data(), sizeof(float), N * DESC, f) != N * DESC ||
          std::fread(g.data(), sizeof(double), N, f) != N || std::fread(w.data(), sizeof(int32_t), N, f) != N)
        e = MSG_FILE_TRUNCATED;
      else { parent.swap(p); centre.swap(c); weight.swap(g); word_id.swap(w); }
    }
  }
  std::fclose(f);
  return e;
}

}  // namespace sim3opt_vocab
