// vocab_host_driver.cpp -- the host half of the batched vocabulary training (csrc/vocab_host.hpp: the checks of the
// options and of the frames with every message as an exact string, the tables of a level, the assembly of the levels
// into the four arrays, the weights, and the file with its refusals) as a stand-alone program for AddressSanitizer +
// UndefinedBehaviorSanitizer: no GPU and no HIP.  The arrays are sized exactly, so that a read past an end is the
// sanitizer's to find.  argv[1]: a directory for the files it writes.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "../../sim3opt_amd/csrc/vocab_host.hpp"

using namespace sim3opt_vocab;

static int failed = 0, checks = 0;
#define CHECK(c)                                                      \
  do {                                                                \
    ++checks;                                                         \
    if (!(c)) { ++failed; std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); } \
  } while (0)

static void write_bytes(const std::string& path, const std::vector<char>& b, size_t n) {
  std::FILE* f = std::fopen(path.c_str(), "wb");
  if (f) { std::fwrite(b.data(), 1, n, f); std::fclose(f); }
}

int main(int argc, char** argv) {
  const std::string dir = argc > 1 ? argv[1] : ".";
  const float nan = std::numeric_limits<float>::quiet_NaN();
  // ---- options
  sim3opt_vocabulary_options o{0, 10, 5, 100, 1, -1};
  CHECK(validate_options(o).empty());
  { auto p = o; p.k = 1; CHECK(validate_options(p) == "k outside 2..64"); }
  { auto p = o; p.k = 65; CHECK(validate_options(p) == "k outside 2..64"); }
  { auto p = o; p.k = 2; CHECK(validate_options(p).empty()); p.k = 64; CHECK(validate_options(p).empty()); }
  { auto p = o; p.levels = 0; CHECK(validate_options(p) == "levels outside 1..8"); }
  { auto p = o; p.levels = 9; CHECK(validate_options(p) == "levels outside 1..8"); }
  { auto p = o; p.levels = 8; CHECK(validate_options(p).empty()); }
  { auto p = o; p.max_iters = 0; CHECK(validate_options(p) == "max_iters < 1"); }
  { auto p = o; p.idf = 2; CHECK(validate_options(p) == "idf is neither 0 nor 1"); }
  { auto p = o; p.idf = -1; CHECK(validate_options(p) == "idf is neither 0 nor 1"); }
  // ---- frames: the refusals of place recognition's set_frames, and two distinct descriptors
  {
    const size_t n = 5;
    std::unique_ptr<float[]> d(new float[DESC * n]);
    for (size_t i = 0; i < DESC * n; ++i) d[i] = 0.5f;
    d[DESC * 4 + 63] = 0.25f;
    std::unique_ptr<int32_t[]> ptr(new int32_t[4]{0, 2, 2, 5});
    CHECK(validate_frames(3, ptr.get(), d.get()).empty());
    CHECK(validate_frames(0, ptr.get(), d.get()) == "n_frames < 1");
    CHECK(validate_frames(SIM3OPT_PLACE_MAX_FRAMES + 1, ptr.get(), d.get()) == "n_frames above SIM3OPT_PLACE_MAX_FRAMES");
    CHECK(validate_frames(3, nullptr, d.get()) == "a NULL array" && validate_frames(3, ptr.get(), nullptr) == "a NULL array");
    ptr[0] = 1;
    CHECK(validate_frames(3, ptr.get(), d.get()) == "kp_ptr[0] must be 0");
    ptr[0] = 0; ptr[1] = 3;
    CHECK(validate_frames(3, ptr.get(), d.get()) == "kp_ptr is not monotone at frame 1");
    ptr[1] = 2;
    d[DESC * 2 + 1] = nan;
    CHECK(validate_frames(3, ptr.get(), d.get()) == "a non-finite descriptor");
    d[DESC * 2 + 1] = 0.5f;
    d[DESC * 4 + 63] = 0.5f;  // all equal
    CHECK(validate_frames(3, ptr.get(), d.get()) == "fewer than two distinct descriptors");
    d[DESC * 3] = -0.0f; d[0] = 0.0f; d[DESC] = 0.0f; d[DESC * 2] = 0.0f; d[DESC * 4] = 0.0f;  // +0 and -0 are one value
    CHECK(validate_frames(3, ptr.get(), d.get()) == "fewer than two distinct descriptors");
    std::unique_ptr<int32_t[]> one(new int32_t[2]{0, 1}), none(new int32_t[2]{0, 0});
    CHECK(validate_frames(1, one.get(), d.get()) == "fewer than two distinct descriptors");
    CHECK(validate_frames(1, none.get(), d.get()) == "fewer than two distinct descriptors");
  }
  // ---- the key of the seeding's draws holds the seed, the node and c only; c stays below 64, so no two draws share one
  CHECK(seed_key(7, 0, 0) == 7 + 0x9E3779B97F4A7C15ull && seed_key(7, 1, 0) == seed_key(7, 0, 64));
  CHECK(seed_key(0, 3, 63) + 0x9E3779B97F4A7C15ull == seed_key(0, 4, 0));
  // ---- the tables of a level
  {
    Level V;
    V.first_node = 4;
    V.count = {1, 3, 4, 5, 255, 256, 257, 1024, 1025, 2049};
    plan_level(V, 1, 3, 4);
    const std::vector<int32_t> kinds = {LEAF, SMALL, SMALL, BIG, BIG, BIG, BIG, BIG, BIG, BIG};
    CHECK(V.kind == kinds && V.T() == 10 && V.start[0] == 0 && V.start[3] == 8 && V.n_members == 4879);
    const std::vector<int32_t> nch = {1, 1, 1, 1, 1, 1, 2, 4, 5, 9}, nm = {0, 0, 0, 1, 1, 1, 1, 1, 2, 3};
    CHECK(V.node_nchunks == nch && V.node_nmchunks == nm && V.multi == std::vector<int32_t>({8, 9}) && V.n_slots == 5);
    size_t members = 0;
    for (size_t c = 0; c < V.chunk_node.size(); ++c) {
      CHECK(V.chunk_len[c] >= 1 && V.chunk_len[c] <= CHUNK && V.chunk_start[c] == (int32_t)members);
      members += (size_t)V.chunk_len[c];
    }
    CHECK(members == 4879 && V.chunk_len[V.node_chunk0[6] + 1] == 1 && V.mchunk_len.back() == 1);
    CHECK(V.mchunk_slot[V.node_mchunk0[7]] == -1 && V.mchunk_slot[V.node_mchunk0[8]] == 0 && V.mchunk_slot[V.node_mchunk0[9]] == 2);
    plan_level(V, 3, 3, 4);  // the last level: every node a leaf
    CHECK(V.kind == std::vector<int32_t>(10, LEAF) && V.mchunk_node.empty() && V.chunk_node.size() == 26);
  }
  // ---- the assembly: a root of three clusters (the middle one empty), then a node of two members beside two leaves
  {
    const int32_t k = 3;
    Tree R;
    R.start();
    Level V;
    V.count = {6};
    plan_level(V, 0, 2, k);
    std::vector<float> cw((size_t)k * DESC);
    for (size_t i = 0; i < cw.size(); ++i) cw[i] = (float)i;
    std::vector<int32_t> child_start;
    std::string err;
    Level N;
    N.first_node = R.n_nodes();
    N.count = append_children(R, V, 0, k, {3, 0, 3}, cw, child_start, err);
    CHECK(err.empty() && N.count == std::vector<int32_t>({3, 3}) && child_start == std::vector<int32_t>({0, 3, 3}));
    CHECK(R.n_nodes() == 3 && R.parent == std::vector<int32_t>({-1, 0, 0}) && R.centre[DESC] == 0.f && R.centre[2 * DESC] == 128.f);
    plan_level(N, 1, 2, k);
    CHECK(N.kind == std::vector<int32_t>({SMALL, SMALL}));
    N.kind[1] = LEAF;  // (as after a seeding that found its members equal)
    std::vector<float> cw2((size_t)2 * k * DESC, 1.f);
    Level M;
    M.first_node = R.n_nodes();
    M.count = append_children(R, N, 1, k, {1, 1, 1, 0, 0, 0}, cw2, child_start, err);
    CHECK(err.empty() && M.count == std::vector<int32_t>({1, 1, 1}) && R.parent == std::vector<int32_t>({-1, 0, 0, 1, 1, 1}));
    std::vector<int32_t> first_child, n_child;
    int32_t depth = 0;
    CHECK(finish_tree(R, first_child, n_child, depth) == 4 && depth == 2);
    CHECK(R.word_id == std::vector<int32_t>({-1, -1, 0, 1, 2, 3}) && n_child == std::vector<int32_t>({2, 3, 0, 0, 0, 0}) &&
          first_child[0] == 1 && first_child[1] == 3);
    // the weights: three frames, the middle one empty; leaf 2 in both others, leaf 3 in one, leaf 5 in none
    const std::unique_ptr<int32_t[]> kp(new int32_t[4]{0, 3, 3, 6});
    const std::unique_ptr<int32_t[]> leaf(new int32_t[6]{2, 3, 3, 2, 4, 2});
    idf_weights(R, 3, kp.get(), leaf.get(), 1);
    CHECK(R.weight[0] == 0 && R.weight[1] == 0 && R.weight[2] == 0 && R.weight[3] == std::log(2.0) && R.weight[4] == std::log(2.0) &&
          R.weight[5] == 0);
    idf_weights(R, 3, kp.get(), leaf.get(), 0);
    CHECK(R.weight == std::vector<double>({0, 0, 1, 1, 1, 1}));
    // ---- the file
    const std::string path = dir + "/tree.bin";
    CHECK(save_file(path.c_str(), R.n_nodes(), R.parent.data(), R.centre.data(), R.weight.data(), R.word_id.data()).empty());
    std::vector<int32_t> p, w;
    std::vector<float> c;
    std::vector<double> g;
    CHECK(load_file(path.c_str(), p, c, g, w).empty() && p == R.parent && c == R.centre && g == R.weight && w == R.word_id);
    CHECK(save_file(path.c_str(), 1, R.parent.data(), R.centre.data(), R.weight.data(), R.word_id.data()) == "a sim3opt vocabulary file with impossible counts");
    CHECK(save_file(nullptr, 6, R.parent.data(), R.centre.data(), R.weight.data(), R.word_id.data()) == "a NULL argument");
    CHECK(save_file((dir + "/no/such/dir/x.bin").c_str(), 6, R.parent.data(), R.centre.data(), R.weight.data(), R.word_id.data()) == "cannot open the file");
    CHECK(load_file((dir + "/absent.bin").c_str(), p, c, g, w) == "cannot open the file" && p == R.parent);
    // truncated at every interesting length, a wrong magic, another version, impossible counts, a longer file
    std::vector<char> bytes;
    {
      std::FILE* f = std::fopen(path.c_str(), "rb");
      int ch;
      while (f && (ch = std::fgetc(f)) != EOF) bytes.push_back((char)ch);
      if (f) std::fclose(f);
    }
    CHECK(bytes.size() == 20 + 6 * (4 + 4 + 8 + 4 * (size_t)DESC));
    const std::string cut = dir + "/cut.bin";
    for (size_t n : {(size_t)0, (size_t)7, (size_t)8, (size_t)19, (size_t)20, bytes.size() / 2, bytes.size() - 1}) {
      write_bytes(cut, bytes, n);
      CHECK(load_file(cut.c_str(), p, c, g, w) == "a truncated sim3opt vocabulary file" && p == R.parent);
    }
    std::vector<char> b = bytes;
    b[3] = 'X';
    write_bytes(cut, b, b.size());
    CHECK(load_file(cut.c_str(), p, c, g, w) == "not a sim3opt vocabulary file (magic)");
    b = bytes; b[8] = 2;
    write_bytes(cut, b, b.size());
    CHECK(load_file(cut.c_str(), p, c, g, w) == "a sim3opt vocabulary file of another version");
    b = bytes; b[12] = 1;
    write_bytes(cut, b, b.size());
    CHECK(load_file(cut.c_str(), p, c, g, w) == "a sim3opt vocabulary file with impossible counts");
    b = bytes; b[15] = 0x7f;  // a count the file cannot hold
    write_bytes(cut, b, b.size());
    CHECK(load_file(cut.c_str(), p, c, g, w) != "" && p == R.parent);
    b = bytes; b[16] = 32;
    write_bytes(cut, b, b.size());
    CHECK(load_file(cut.c_str(), p, c, g, w) == "a sim3opt vocabulary file with impossible counts");
    b = bytes; b.push_back(0);
    write_bytes(cut, b, b.size());
    CHECK(load_file(cut.c_str(), p, c, g, w) == "a sim3opt vocabulary file with impossible counts" && p == R.parent && w == R.word_id);
  }
  std::printf("%d checks, %d failed\n", checks, failed);
  if (failed) return 1;
  std::printf("vocab host ok\n");
  return 0;
}
