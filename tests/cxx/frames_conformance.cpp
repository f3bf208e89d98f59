// Conformance program of include/sim3opt_frames.hpp (FrameStore over sim3opt_frames_*) and of the FrameStore overloads of
// SurfExtractorBatch, VocabularyTrainer, LoopDetectorBatch and LoopMatchBatch, composed as a call site composes them:
// images -> one store -> tree, detector, matcher.
//   frames_conformance host        argument checks of the helper and of the C-ABI; needs no GPU
//   frames_conformance run FILE    the images of FILE through extract(store); then every stage once from the store and
//                                  once from host arrays (extract() and the array overloads): the results are equal to
//                                  the bit; exit 3 with the library's message when there is no GPU
// FILE: "n_images width height", then the pixels row by row.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "sim3opt_frames.hpp"
#include "sim3opt_match.hpp"
#include "sim3opt_place.hpp"
#include "sim3opt_surf.hpp"
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

struct Pt { float x, y; };

int host_part() {
  using sim3opt_shim::FrameStore;
  // ---- the helper ----
  {
    FrameStore store;
    CHECK(store.options().device == -1 && store.handle() != nullptr);
    CHECK(store.n_frames() == 0 && store.total_keypoints() == 0 && !store.filled());
    CHECK(store.kp_ptr() == std::vector<int32_t>(1, 0));
    std::vector<float> kp, desc;
    CHECK(store.get(kp, desc) == SIM3OPT_ERR_STATE && store.last_error() == "get: the store is not filled");
    const int32_t ptr[3] = {0, 1, 2}, down[3] = {0, 2, 1};
    const float k[4] = {1, 2, 3, 4};
    std::vector<float> d(128, 0.25f);
    CHECK(store.set(0, ptr, k, d.data()) == SIM3OPT_ERR_ARG && store.last_error() == "frames_set: n_frames < 1");
    CHECK(store.set(2, nullptr, k, d.data()) == SIM3OPT_ERR_ARG && store.last_error() == "frames_set: a NULL array");
    CHECK(store.set(2, down, k, d.data()) == SIM3OPT_ERR_ARG && store.last_error() == "frames_set: kp_ptr is not monotone at frame 1");
    d[100] = std::numeric_limits<float>::infinity();
    CHECK(store.set(2, ptr, k, d.data()) == SIM3OPT_ERR_ARG && store.last_error() == "frames_set: a non-finite descriptor");
    store.options().device = -7;
    CHECK(store.prepare() == SIM3OPT_ERR_ARG && store.last_error() == "frames_set_options: device below -1");
    CHECK(!store.filled());
  }
  // ---- the C-ABI: a NULL or an unfilled store is refused by every stage, which stays as it was ----
  {
    sim3opt_frames* s = sim3opt_frames_create();
    CHECK(s != nullptr);
    int32_t n = -1, total = -1, device = 0, tiles[2] = {0, 0};
    int64_t bytes = -1;
    CHECK(sim3opt_frames_get_dims(s, &n, &total, &device, &bytes, tiles) == SIM3OPT_OK && n == 0 && total == 0 && device == -1 &&
          bytes == 0 && tiles[0] == 256 && tiles[1] == 16);
    CHECK(sim3opt_frames_get_dims(nullptr, &n, &total, &device, &bytes, tiles) == SIM3OPT_ERR_ARG);
    CHECK(sim3opt_frames_get(s, &n, nullptr, nullptr) == SIM3OPT_ERR_STATE);
    CHECK(std::string(sim3opt_frames_last_error(s)) == "frames_get: the store is not filled");
    CHECK(std::string(sim3opt_frames_last_error(nullptr)) == "null store");
    sim3opt_vocabulary* v = sim3opt_vocabulary_create();
    sim3opt_place_batch* p = sim3opt_place_batch_create();
    sim3opt_match_batch* m = sim3opt_match_batch_create();
    sim3opt_surf_batch* b = sim3opt_surf_batch_create();
    CHECK(sim3opt_vocabulary_set_frames_from(v, nullptr) == SIM3OPT_ERR_ARG);
    CHECK(std::string(sim3opt_vocabulary_last_error(v)) == "vocabulary_set_frames_from: NULL store");
    CHECK(sim3opt_vocabulary_set_frames_from(v, s) == SIM3OPT_ERR_STATE);
    CHECK(std::string(sim3opt_vocabulary_last_error(v)) == "vocabulary_set_frames_from: the store is not filled");
    CHECK(sim3opt_vocabulary_train(v) == SIM3OPT_ERR_STATE);  // (still no frames)
    CHECK(sim3opt_place_batch_set_frames_from(p, nullptr) == SIM3OPT_ERR_ARG && sim3opt_place_batch_set_frames_from(p, s) == SIM3OPT_ERR_STATE);
    const int32_t obs_ptr[2] = {0, 0};
    const float none = 0.f;
    CHECK(sim3opt_match_batch_set_frames_from(m, nullptr, 1, obs_ptr, &none, &none, 500, 10, 10, 20, 20) == SIM3OPT_ERR_ARG);
    CHECK(sim3opt_match_batch_set_frames_from(m, s, 1, obs_ptr, &none, &none, 500, 10, 10, 20, 20) == SIM3OPT_ERR_STATE);
    CHECK(std::string(sim3opt_match_batch_last_error(m)) == "match_batch_set_frames_from: the store is not filled");
    int32_t nf = -1;
    CHECK(sim3opt_match_batch_dims(m, &nf, nullptr, nullptr, nullptr, nullptr) == SIM3OPT_OK && nf == 0);
    CHECK(sim3opt_surf_batch_solve_into(b, nullptr) == SIM3OPT_ERR_ARG);
    CHECK(sim3opt_surf_batch_solve_into(b, s) == SIM3OPT_ERR_STATE);  // no images set
    CHECK(sim3opt_surf_batch_solve_into(nullptr, s) == SIM3OPT_ERR_ARG);
    sim3opt_vocabulary_destroy(v); sim3opt_place_batch_destroy(p); sim3opt_match_batch_destroy(m); sim3opt_surf_batch_destroy(b);
    sim3opt_frames_destroy(s);
    sim3opt_frames_destroy(nullptr);
  }
  // ---- the overloads refuse an unfilled store with the library's words ----
  {
    FrameStore store;
    sim3opt_shim::VocabularyTrainer voc(3, 2);
    CHECK(voc.create(store) == SIM3OPT_ERR_STATE && voc.last_error() == "vocabulary_set_frames_from: the store is not filled" && voc.empty());
    sim3opt_shim::LoopDetectorBatch places;
    CHECK(places.detect(store) == SIM3OPT_ERR_STATE && places.n_frames() == 0);
    const double K[9] = {500, 0, 10, 0, 500, 10, 0, 0, 1};
    sim3opt_shim::LoopMatchBatch matches(K, 20, 20);
    CHECK(matches.solve(store) == SIM3OPT_ERR_STATE);
    sim3opt_shim::SurfExtractorBatch surf;
    CHECK(surf.extract(store) == SIM3OPT_ERR_STATE && surf.last_error() == "extract: no image added");
  }
  std::printf("frames_conformance host: %d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}

// every result of a solved matcher, flat
std::vector<double> flat(const sim3opt_shim::LoopMatchBatch& m) {
  std::vector<double> out;
  for (int k = 0; k < m.n_pairs(); ++k) {
    out.push_back(m.status(k)); out.push_back(m.n_matches(k));
    for (int i = 0; i < m.n_matches(k); ++i) {
      const sim3opt_shim::LoopMatchBatch::P3 p = m.surf_point(k, i);
      for (double v : {(double)m.query_idx(k, i), (double)m.train_idx(k, i), (double)m.distance(k, i), m.point1(k, i).x,
                       m.point1(k, i).y, m.point2(k, i).x, m.point2(k, i).y, m.depth(k, 0, i), m.depth(k, 1, i), p.x, p.y, p.z})
        out.push_back(v);
    }
  }
  return out;
}

int run_part(const char* path) {
  FILE* f = std::fopen(path, "r");
  if (!f) { std::fprintf(stderr, "cannot open %s\n", path); return 2; }
  int n_images = 0, w = 0, h = 0;
  if (std::fscanf(f, "%d %d %d", &n_images, &w, &h) != 3 || n_images < 1 || w < 1 || h < 1) {
    std::fclose(f);
    return 2;
  }
  bool ok = true;
  std::vector<std::vector<unsigned char>> images((size_t)n_images, std::vector<unsigned char>((size_t)w * (size_t)h, 0));
  for (auto& im : images)
    for (size_t i = 0; i < im.size() && ok; ++i) {
      int v = 0;
      ok = std::fscanf(f, "%d", &v) == 1 && v >= 0 && v <= 255;
      im[i] = (unsigned char)v;
    }
  std::fclose(f);
  if (!ok) { std::fprintf(stderr, "malformed file %s\n", path); return 2; }

  // the host-array chain
  sim3opt_shim::SurfExtractorBatch surf_a, surf_b;
  surf_a.options().images_per_pass = surf_b.options().images_per_pass = 2;  // (more images than a pass)
  for (const auto& im : images) CHECK(surf_a.add(im.data(), w, h, w) == SIM3OPT_OK && surf_b.add(im.data(), w, h, w) == SIM3OPT_OK);
  const int ra = surf_a.extract();
  if (ra < 0) { std::fprintf(stderr, "extract failed (%d): %s\n", ra, surf_a.last_error().c_str()); return 3; }
  // ... and the store's
  sim3opt_shim::FrameStore store;
  const int rb = surf_b.extract(store);
  if (rb < 0) { std::fprintf(stderr, "extract(store) failed (%d): %s\n", rb, surf_b.last_error().c_str()); return 3; }
  CHECK(ra == rb && surf_a.kp_ptr() == surf_b.kp_ptr() && surf_a.kp() == surf_b.kp() && surf_b.desc().empty());
  CHECK(store.filled() && store.n_frames() == n_images && store.total_keypoints() == surf_a.kp_ptr().back());
  CHECK(store.kp_ptr() == surf_a.kp_ptr());
  std::vector<float> kp, desc;
  CHECK(store.get(kp, desc) == SIM3OPT_OK && kp == surf_a.kp() && desc == surf_a.desc());
  for (int i = 0; i < n_images; ++i) {
    const std::vector<sim3opt_shim::SurfKey> ka = surf_a.keys(i), kb = surf_b.keys(i);
    bool same = ka.size() == kb.size();
    for (size_t k = 0; same && k < ka.size(); ++k)
      same = ka[k].x == kb[k].x && ka[k].y == kb[k].y && ka[k].size == kb[k].size && ka[k].angle == kb[k].angle &&
             ka[k].response == kb[k].response && ka[k].octave == kb[k].octave && ka[k].laplacian == kb[k].laplacian;
    CHECK(same && surf_b.descriptors(i).empty());
  }

  sim3opt_shim::VocabularyTrainer voc_a(3, 2), voc_b(3, 2);
  const int na = voc_a.create(surf_a.n_frames(), surf_a.kp_ptr().data(), surf_a.desc().data());
  const int nb = voc_b.create(store);
  if (na < 0 || nb < 0) { std::fprintf(stderr, "create failed: %s%s\n", voc_a.last_error().c_str(), voc_b.last_error().c_str()); return 3; }
  CHECK(na == nb && na > 1 && voc_a.parent() == voc_b.parent() && voc_a.centre() == voc_b.centre() &&
        voc_a.weight() == voc_b.weight() && voc_a.word_id() == voc_b.word_id());

  sim3opt_shim::LoopDetectorBatch places_a, places_b;
  CHECK(voc_a.feed(places_a) == SIM3OPT_OK && voc_b.feed(places_b) == SIM3OPT_OK);
  for (int i = 0; i < surf_a.n_frames(); ++i) places_a.add_frame(surf_a.frame_desc(i), surf_a.count(i));
  const int da = places_a.detect(), db = places_b.detect(store);
  if (da < 0 || db < 0) { std::fprintf(stderr, "detect failed: %s%s\n", places_a.last_error().c_str(), places_b.last_error().c_str()); return 3; }
  CHECK(da == db && places_b.n_frames() == n_images);
  for (int i = 0; i < n_images; ++i) {
    const sim3opt_shim::LoopDetectorBatch::DetectionResult x = places_a.result(i), y = places_b.result(i);
    CHECK(x.status == y.status && x.match == y.match && x.score == y.score && x.ns_factor == y.ns_factor &&
          x.n_consistent == y.n_consistent && x.island_first == y.island_first && x.island_last == y.island_last);
  }

  // the matcher: the same map observations on both sides; the store's side adds them without keys
  const double K[9] = {300, 0, 0.5 * w, 0, 300, 0.5 * h, 0, 0, 1};
  sim3opt_shim::LoopMatchBatch match_a(K, w, h), match_b(K, w, h);
  unsigned rng = 99u;
  auto next = [&]() { rng = rng * 1664525u + 1013904223u; return (float)((rng >> 8) & 0xFFFF) / 65536.f; };
  for (int i = 0; i < n_images; ++i) {
    std::vector<Pt> keys, no_keys, obs;
    std::vector<float> depths;
    for (int k = 0; k < surf_a.count(i); ++k) {
      const size_t at = (size_t)(surf_a.kp_ptr()[(size_t)i] + k);
      keys.push_back(Pt{surf_a.kp()[2 * at], surf_a.kp()[2 * at + 1]});
    }
    for (int k = 0; k < 25 + i; ++k) { obs.push_back(Pt{next() * (float)w, next() * (float)h}); depths.push_back(5.f + 40.f * next()); }
    CHECK(match_a.add_frame(keys, surf_a.frame_desc(i), obs, depths) == i);
    CHECK(match_b.add_frame(no_keys, nullptr, obs, depths) == i);
  }
  places_a.feed(match_a); places_b.feed(match_b);
  for (int i = 0; i + 1 < n_images; ++i) { match_a.add_pair(i, n_images - 1 - i); match_b.add_pair(i, n_images - 1 - i); }
  const int ma = match_a.solve(), mb = match_b.solve(store);
  if (ma < 0 || mb < 0) { std::fprintf(stderr, "solve failed: %s%s\n", match_a.last_error().c_str(), match_b.last_error().c_str()); return 3; }
  const std::vector<double> fa = flat(match_a), fb = flat(match_b);
  CHECK(ma == mb && fa == fb && fa.size() > 2 * (size_t)match_a.n_pairs());  // (some pair has matches)
  std::printf("frames_conformance run: %d images, %d keypoints, %d nodes, %d pairs, %d checks, %d failed\n", n_images,
              store.total_keypoints(), na, match_a.n_pairs(), g_checks, g_failed);
  return g_failed ? 1 : 0;
}
}  // namespace

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "host") return host_part();
  if (mode == "run" && argc > 2) return run_part(argv[2]);
  std::fprintf(stderr, "usage: %s host | run FILE\n", argv[0]);
  return 2;
}
