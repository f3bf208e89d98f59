// Conformance program of include/sim3opt_vocabulary.hpp (VocabularyTrainer over sim3opt_vocabulary_*), the batched
// replacement of DBoW2's voc.create(features), composed with include/sim3opt_place.hpp as a call site composes them:
// features -> tree -> the detector's vocabulary.
//   vocabulary_conformance host        argument checks of the helper and of the C-ABI, save / load; needs no GPU
//   vocabulary_conformance run FILE    the images of FILE through VocabularyTrainer::create(features); the expected
//                                      parent, word id, weight and centre of every node come back; the tree survives
//                                      save / load and becomes a LoopDetectorBatch's vocabulary, which detects on the
//                                      same images; exit 3 with the library's message when there is no GPU
// FILE: "n_images k L seed n_nodes", per image "count" and count rows "d0 .. d63", then per node
// "parent word_id weight c0 .. c63".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "sim3opt_place.hpp"
#include "sim3opt_vocabulary.hpp"

namespace {
int g_checks = 0, g_failed = 0;
void check(bool ok, const char* what) {
  ++g_checks;
  if (!ok) {
    ++g_failed;
    std::printf("FAILED: %s\n", what);
  }
}
#define CHECK(x) check((x), #x)

typedef std::vector<std::vector<std::vector<float>>> Features;

int host_part(const char* dir) {
  using sim3opt_shim::VocabularyTrainer;
  // ---- the helper ----
  {
    VocabularyTrainer voc(9, 3);
    const sim3opt_vocabulary_options& o = voc.options();
    CHECK(o.k == 9 && o.levels == 3 && o.max_iters == 100 && o.idf == 1 && o.seed == 0 && o.device == -1);
    CHECK(voc.empty() && voc.size() == 0 && voc.words() == 0);
    sim3opt_shim::LoopDetectorBatch places;
    CHECK(voc.feed(places) == SIM3OPT_ERR_STATE && voc.save(std::string(dir) + "/none.bin") == SIM3OPT_ERR_STATE);
    Features f(2);
    f[0].push_back(std::vector<float>(63, 0.f));
    CHECK(voc.create(f) == SIM3OPT_ERR_ARG && voc.last_error() == "create: a descriptor that is not 64 floats");
    f[0][0].assign(64, 0.25f);
    f[0].push_back(std::vector<float>(64, 0.25f));
    CHECK(voc.create(f) == SIM3OPT_ERR_ARG && voc.last_error() == "vocabulary_set_frames: fewer than two distinct descriptors");
    voc.options().k = 1;
    CHECK(voc.create(f) == SIM3OPT_ERR_ARG && voc.last_error() == "vocabulary_set_options: k outside 2..64");
    VocabularyTrainer defaults;
    CHECK(defaults.options().k == 10 && defaults.options().levels == 5);
  }
  // ---- the C-ABI: every refusal leaves the handle as it was ----
  {
    sim3opt_vocabulary* h = sim3opt_vocabulary_create();
    CHECK(h != nullptr);
    CHECK(sim3opt_vocabulary_train(h) == SIM3OPT_ERR_STATE);  // nothing set
    CHECK(sim3opt_vocabulary_get_vocabulary(h, nullptr, nullptr, nullptr, nullptr) == SIM3OPT_ERR_STATE);
    CHECK(sim3opt_vocabulary_get_assignment(h, nullptr, nullptr) == SIM3OPT_ERR_STATE);
    std::vector<float> d(5 * 64, 0.5f);
    d[64 * 4] = 0.75f;
    int32_t ptr[4] = {0, 2, 2, 5}, back[4] = {0, 3, 2, 5}, off[4] = {1, 2, 2, 5};
    CHECK(sim3opt_vocabulary_set_frames(h, 3, ptr, d.data()) == SIM3OPT_OK);
    auto unchanged = [&]() {
      int32_t nn = -1, nw = -1, de = -1, nu = -1, nf = 0, nd = 0, p[8], t[2] = {0, 0};
      return sim3opt_vocabulary_dims(h, &nn, &nw, &de, &nu, &nf, &nd, p, t) == SIM3OPT_OK && nn == 0 && nw == 0 && de == 0 &&
             nu == 0 && nf == 3 && nd == 5 && p[0] == 0 && p[7] == 0 && t[0] == 256 && t[1] == 1024;
    };
    CHECK(unchanged());
    CHECK(sim3opt_vocabulary_set_frames(h, 0, ptr, d.data()) == SIM3OPT_ERR_ARG && unchanged());
    CHECK(sim3opt_vocabulary_set_frames(h, SIM3OPT_PLACE_MAX_FRAMES + 1, ptr, d.data()) == SIM3OPT_ERR_ARG && unchanged());
    CHECK(sim3opt_vocabulary_set_frames(h, 3, back, d.data()) == SIM3OPT_ERR_ARG && unchanged());
    CHECK(sim3opt_vocabulary_set_frames(h, 3, off, d.data()) == SIM3OPT_ERR_ARG && unchanged());
    CHECK(sim3opt_vocabulary_set_frames(h, 3, nullptr, d.data()) == SIM3OPT_ERR_ARG && unchanged());
    CHECK(sim3opt_vocabulary_set_frames(h, 3, ptr, nullptr) == SIM3OPT_ERR_ARG && unchanged());
    {
      std::vector<float> bad = d;
      bad.back() = NAN;
      CHECK(sim3opt_vocabulary_set_frames(h, 3, ptr, bad.data()) == SIM3OPT_ERR_ARG && unchanged());
      bad = d;
      bad[64 * 4] = 0.5f;  // all five equal
      CHECK(sim3opt_vocabulary_set_frames(h, 3, ptr, bad.data()) == SIM3OPT_ERR_ARG && unchanged());
      CHECK(std::string(sim3opt_vocabulary_last_error(h)) == "vocabulary_set_frames: fewer than two distinct descriptors");
    }
    sim3opt_vocabulary_options o;
    sim3opt_vocabulary_options_default(&o);
    o.levels = 9;
    CHECK(sim3opt_vocabulary_set_options(h, &o) == SIM3OPT_ERR_ARG);
    CHECK(std::string(sim3opt_vocabulary_last_error(h)) == "vocabulary_set_options: levels outside 1..8");
    o.levels = 5; o.max_iters = 0;
    CHECK(sim3opt_vocabulary_set_options(h, &o) == SIM3OPT_ERR_ARG);
    o.max_iters = 3; o.idf = -1;
    CHECK(sim3opt_vocabulary_set_options(h, &o) == SIM3OPT_ERR_ARG && unchanged());
    o.idf = 0;
    CHECK(sim3opt_vocabulary_set_options(h, &o) == SIM3OPT_OK);
    CHECK(sim3opt_vocabulary_set_options(h, nullptr) == SIM3OPT_ERR_ARG && sim3opt_vocabulary_set_options(nullptr, &o) == SIM3OPT_ERR_ARG);
    int32_t n = 0;
    CHECK(sim3opt_vocabulary_debug_seeding(h, 0, &n, nullptr, nullptr, nullptr, nullptr) == SIM3OPT_ERR_STATE);
    CHECK(sim3opt_vocabulary_debug_lloyd(h, 0, 0, &n, &n, nullptr, nullptr) == SIM3OPT_ERR_STATE);
    sim3opt_vocabulary_destroy(h);
    sim3opt_vocabulary_destroy(nullptr);
  }
  // ---- save and load: host only
  {
    const int32_t parent[3] = {-1, 0, 0}, word_id[3] = {-1, 0, 1};
    const double weight[3] = {0, 0.5, 1.25};
    std::vector<float> centre(3 * 64, 0.f);
    centre[64] = -1.f; centre[128 + 63] = 2.5f;
    const std::string path = std::string(dir) + "/tree.bin";
    CHECK(sim3opt_vocabulary_save(path.c_str(), 3, parent, centre.data(), weight, word_id) == SIM3OPT_OK);
    CHECK(sim3opt_vocabulary_save(path.c_str(), 1, parent, centre.data(), weight, word_id) == SIM3OPT_ERR_ARG);
    CHECK(sim3opt_vocabulary_save(path.c_str(), 3, nullptr, centre.data(), weight, word_id) == SIM3OPT_ERR_ARG);
    CHECK(sim3opt_vocabulary_save((std::string(dir) + "/no/such/dir/tree.bin").c_str(), 3, parent, centre.data(), weight, word_id) == SIM3OPT_ERR_IO);
    VocabularyTrainer voc;
    CHECK(voc.load(path) == SIM3OPT_OK && voc.size() == 3 && voc.words() == 2);
    CHECK(voc.parent() == std::vector<int32_t>(parent, parent + 3) && voc.word_id() == std::vector<int32_t>(word_id, word_id + 3));
    CHECK(voc.weight() == std::vector<double>(weight, weight + 3) && voc.centre() == centre);
    CHECK(voc.load(std::string(dir) + "/absent.bin") == SIM3OPT_ERR_IO && voc.size() == 3);
    sim3opt_shim::LoopDetectorBatch places;
    CHECK(voc.feed(places) == SIM3OPT_OK);  // a loaded tree is the detector's vocabulary
    CHECK(voc.save(std::string(dir) + "/again.bin") == SIM3OPT_OK);
  }
  std::printf("vocabulary_conformance host: %d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}

int run_part(const char* path, const char* dir) {
  FILE* f = std::fopen(path, "r");
  if (!f) { std::fprintf(stderr, "cannot open %s\n", path); return 2; }
  int n_images = 0, k = 0, L = 0, n_nodes = 0;
  unsigned long long seed = 0;
  if (std::fscanf(f, "%d %d %d %llu %d", &n_images, &k, &L, &seed, &n_nodes) != 5 || n_images < 1 || n_nodes < 2) {
    std::fclose(f);
    return 2;
  }
  Features features((size_t)n_images);
  bool ok = true;
  for (int i = 0; i < n_images && ok; ++i) {
    int count = 0;
    ok = std::fscanf(f, "%d", &count) == 1 && count >= 0;
    features[(size_t)i].assign((size_t)(ok ? count : 0), std::vector<float>(64));
    for (auto& d : features[(size_t)i])
      for (int j = 0; j < 64 && ok; ++j) ok = std::fscanf(f, "%f", &d[(size_t)j]) == 1;
  }
  std::vector<int32_t> parent((size_t)n_nodes), word_id((size_t)n_nodes);
  std::vector<double> weight((size_t)n_nodes);
  std::vector<float> centre(64 * (size_t)n_nodes);
  for (int i = 0; i < n_nodes && ok; ++i) {
    ok = std::fscanf(f, "%d %d %lf", &parent[(size_t)i], &word_id[(size_t)i], &weight[(size_t)i]) == 3;
    for (int j = 0; j < 64 && ok; ++j) ok = std::fscanf(f, "%f", &centre[64 * (size_t)i + j]) == 1;
  }
  std::fclose(f);
  if (!ok) { std::fprintf(stderr, "malformed file %s\n", path); return 2; }
  sim3opt_shim::VocabularyTrainer voc(k, L);
  voc.options().seed = seed;
  const int rc = voc.create(features);
  if (rc < 0) {
    std::fprintf(stderr, "create failed (%d): %s\n", rc, voc.last_error().c_str());
    return 3;
  }
  CHECK(rc == n_nodes && voc.size() == n_nodes);
  CHECK(voc.parent() == parent && voc.word_id() == word_id && voc.centre() == centre);
  bool near = voc.weight().size() == weight.size();
  for (size_t i = 0; near && i < weight.size(); ++i) near = std::fabs(voc.weight()[i] - weight[i]) <= 1e-14;
  CHECK(near);
  // the tree survives the process's end ...
  const std::string file = std::string(dir) + "/trained.bin";
  sim3opt_shim::VocabularyTrainer back;
  CHECK(voc.save(file) == SIM3OPT_OK && back.load(file) == SIM3OPT_OK);
  CHECK(back.parent() == voc.parent() && back.centre() == voc.centre() && back.weight() == voc.weight() &&
        back.word_id() == voc.word_id() && back.words() == voc.words());
  // ... and is the detector's vocabulary, with no conversion
  sim3opt_shim::LoopDetectorBatch places;
  CHECK(back.feed(places) == SIM3OPT_OK);
  for (const auto& image : features) {
    std::vector<float> rows;
    for (const auto& d : image) rows.insert(rows.end(), d.begin(), d.end());
    places.add_frame(rows.data(), (int)image.size());
  }
  const int rd = places.detect();
  if (rd < 0) {
    std::fprintf(stderr, "detect failed (%d): %s\n", rd, places.last_error().c_str());
    return 3;
  }
  CHECK(places.n_frames() == n_images && places.result(0).status == SIM3OPT_PLACE_CLOSE_MATCHES_ONLY);
  std::printf("vocabulary_conformance run: %d nodes, %d words, %d checks, %d failed\n", voc.size(), voc.words(), g_checks,
              g_failed);
  return g_failed ? 1 : 0;
}
}  // namespace

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "host" && argc > 2) return host_part(argv[2]);
  if (mode == "run" && argc > 3) return run_part(argv[2], argv[3]);
  std::fprintf(stderr, "usage: %s host DIR | run FILE DIR   (DIR: where the files it writes go)\n", argv[0]);
  return 2;
}
