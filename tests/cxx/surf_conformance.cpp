// Conformance program of include/sim3opt_surf.hpp (SurfExtractorBatch over sim3opt_surf_batch_*), the batched
// replacement of SurfExtractor::operator() (kitti_surf.cpp:501-523), composed with include/sim3opt_vocabulary.hpp and
// include/sim3opt_place.hpp as a call site composes them: images -> keypoints and descriptors -> tree -> detector.
//   surf_conformance host        argument checks of the helper and of the C-ABI, the host restatement; needs no GPU
//   surf_conformance run FILE    the images of FILE through add() and extract(); the expected keypoints and descriptors
//                                come back to the bit, in the shapes operator() fills; kp_ptr and desc go to a
//                                VocabularyTrainer and a LoopDetectorBatch as they are; exit 3 with the library's
//                                message when there is no GPU
// FILE: "n_images width height", the pixels row by row, then per image "count" and count rows
// "x y size angle response octave laplacian d0 .. d63".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

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

std::vector<unsigned char> blob_image(int w, int h, int stride) {
  std::vector<unsigned char> p((size_t)stride * (size_t)h, 7);
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      const double f = 110 + 100 * std::exp(-((x - 0.4 * w) * (x - 0.4 * w) + (y - 0.5 * h) * (y - 0.5 * h)) / (2 * 3.0 * 3.0)) -
                       90 * std::exp(-((x - 0.7 * w) * (x - 0.7 * w) + (y - 0.4 * h) * (y - 0.4 * h)) / (2 * 4.0 * 4.0));
      p[(size_t)y * (size_t)stride + (size_t)x] = (unsigned char)std::lrint(f);
    }
  return p;
}

int host_part() {
  using sim3opt_shim::SurfExtractorBatch;
  // ---- the helper ----
  {
    SurfExtractorBatch surf;
    const sim3opt_surf_batch_options& o = surf.options();
    CHECK(o.hessian_threshold == 400 && o.n_octaves == 4 && o.n_octave_layers == 3 && o.upright == 0 && o.max_keypoints == 0 &&
          o.images_per_pass == 64 && o.device == -1);
    CHECK(surf.n_frames() == 0 && surf.kp_ptr() == std::vector<int32_t>(1, 0) && surf.keys(0).empty() && surf.descriptors(0).empty());
    CHECK(surf.extract() == SIM3OPT_ERR_STATE && surf.last_error() == "extract: no image added");
    const std::vector<unsigned char> im = blob_image(64, 48, 70);
    CHECK(surf.add(nullptr, 64, 48, 70) == SIM3OPT_ERR_ARG && surf.last_error() == "add: data is NULL");
    CHECK(surf.add(im.data(), 0, 48, 70) == SIM3OPT_ERR_ARG && surf.add(im.data(), 64, 0, 70) == SIM3OPT_ERR_ARG);
    CHECK(surf.add(im.data(), 64, 48, 63) == SIM3OPT_ERR_ARG && surf.last_error() == "add: stride < width" && surf.n_frames() == 0);
    CHECK(surf.add(im.data(), 64, 48, 70) == SIM3OPT_OK && surf.n_frames() == 1);
    CHECK(surf.add(im.data(), 60, 48, 70) == SIM3OPT_ERR_ARG && surf.n_frames() == 1);
    CHECK(surf.last_error() == "add: an image of another size (one size per batch)");
    surf.options().n_octaves = 7;
    CHECK(surf.extract() == SIM3OPT_ERR_ARG && surf.last_error() == "surf_batch_set_options: n_octaves outside 1..6");
    surf.clear();
    CHECK(surf.n_frames() == 0 && surf.add(im.data(), 60, 48, 70) == SIM3OPT_OK);
  }
  // ---- the C-ABI: every refusal leaves the handle as it was ----
  {
    sim3opt_surf_batch* h = sim3opt_surf_batch_create();
    CHECK(h != nullptr);
    CHECK(sim3opt_surf_batch_solve(h) == SIM3OPT_ERR_STATE);  // nothing set
    CHECK(std::string(sim3opt_surf_batch_last_error(h)) == "surf_batch_solve: no images set");
    int32_t ptr[2];
    CHECK(sim3opt_surf_batch_get_kp_ptr(h, ptr) == SIM3OPT_ERR_STATE);
    CHECK(sim3opt_surf_batch_get_keypoints(h, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == SIM3OPT_ERR_STATE);
    CHECK(sim3opt_surf_batch_get_summary(h, nullptr, nullptr, nullptr, nullptr) == SIM3OPT_ERR_STATE);
    const std::vector<unsigned char> im = blob_image(64, 48, 64);
    CHECK(sim3opt_surf_batch_set_images(h, 1, 64, 48, 64, im.data()) == SIM3OPT_OK);
    auto unchanged = [&]() {
      int32_t n = 0, w = 0, hh = 0, t = -1, tiles[3] = {0, 0, 0};
      return sim3opt_surf_batch_dims(h, &n, &w, &hh, &t, tiles) == SIM3OPT_OK && n == 1 && w == 64 && hh == 48 && t == 0 &&
             tiles[0] == 32 && tiles[1] == 256 && tiles[2] == 64;
    };
    CHECK(unchanged());
    CHECK(sim3opt_surf_batch_set_images(h, 0, 64, 48, 64, im.data()) == SIM3OPT_ERR_ARG && unchanged());
    CHECK(sim3opt_surf_batch_set_images(h, 1, 64, 48, 64, nullptr) == SIM3OPT_ERR_ARG && unchanged());
    CHECK(sim3opt_surf_batch_set_images(h, 1, 0, 48, 64, im.data()) == SIM3OPT_ERR_ARG && unchanged());
    CHECK(sim3opt_surf_batch_set_images(h, 1, 64, 48, 63, im.data()) == SIM3OPT_ERR_ARG && unchanged());
    CHECK(std::string(sim3opt_surf_batch_last_error(h)) == "surf_batch_set_images: row_stride < width");
    CHECK(sim3opt_surf_batch_set_images(h, 1, 4096, 2057, 4096, im.data()) == SIM3OPT_ERR_ARG && unchanged());
    sim3opt_surf_batch_options o;
    sim3opt_surf_batch_options_default(&o);
    o.hessian_threshold = -0.5;
    CHECK(sim3opt_surf_batch_set_options(h, &o) == SIM3OPT_ERR_ARG);
    CHECK(std::string(sim3opt_surf_batch_last_error(h)) == "surf_batch_set_options: hessian_threshold is negative or not finite");
    o.hessian_threshold = 400; o.n_octave_layers = 0;
    CHECK(sim3opt_surf_batch_set_options(h, &o) == SIM3OPT_ERR_ARG);
    o.n_octave_layers = 3; o.images_per_pass = 0;
    CHECK(sim3opt_surf_batch_set_options(h, &o) == SIM3OPT_ERR_ARG && unchanged());
    o.images_per_pass = 2;
    CHECK(sim3opt_surf_batch_set_options(h, &o) == SIM3OPT_OK);
    CHECK(sim3opt_surf_batch_set_options(h, nullptr) == SIM3OPT_ERR_ARG && sim3opt_surf_batch_set_options(nullptr, &o) == SIM3OPT_ERR_ARG);
    int32_t n = 0;
    float patch[441];
    CHECK(sim3opt_surf_batch_debug_integral(h, 0, &n) == SIM3OPT_ERR_STATE);
    CHECK(sim3opt_surf_batch_debug_candidates(h, 0, &n, nullptr, nullptr, nullptr, nullptr, nullptr) == SIM3OPT_ERR_STATE);
    CHECK(sim3opt_surf_batch_debug_responses(h, 0, 0, 0, &n, &n, nullptr, nullptr) == SIM3OPT_ERR_STATE);
    CHECK(sim3opt_surf_batch_debug_patch(h, 0, patch) == SIM3OPT_ERR_STATE);
    CHECK(sim3opt_surf_batch_debug_orientation(h, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == SIM3OPT_ERR_STATE);
    sim3opt_surf_batch_destroy(h);
    sim3opt_surf_batch_destroy(nullptr);
  }
  // ---- the host restatement, the test aid: the two blobs, and the stride does not matter
  {
    sim3opt_surf_batch_options o;
    sim3opt_surf_batch_options_default(&o);
    const std::vector<unsigned char> a = blob_image(64, 48, 64), b = blob_image(64, 48, 81);
    float kpa[2 * 16], kpb[2 * 16], da[64 * 16], db[64 * 16];
    int32_t counts[3] = {0, 0, 0};
    const int na = sim3opt_surf_reference_image(&o, 64, 48, 64, a.data(), 16, kpa, da, nullptr, nullptr, nullptr, nullptr, nullptr,
                                                counts, nullptr, 0, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr);
    const int nb = sim3opt_surf_reference_image(&o, 64, 48, 81, b.data(), 16, kpb, db, nullptr, nullptr, nullptr, nullptr, nullptr,
                                                nullptr, nullptr, 0, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr);
    CHECK(na >= 2 && na <= 16 && na == nb && counts[0] >= counts[1] && counts[1] - counts[2] == na);
    bool same = na == nb;
    for (int i = 0; same && i < 2 * na; ++i) same = kpa[i] == kpb[i];
    for (int i = 0; same && i < 64 * na; ++i) same = da[i] == db[i];
    CHECK(same);
    bool found = false;
    for (int i = 0; i < na; ++i) found = found || (std::fabs(kpa[2 * i] - 0.4f * 64) < 1.5f && std::fabs(kpa[2 * i + 1] - 24.f) < 1.5f);
    CHECK(found);
    o.n_octaves = 0;
    CHECK(sim3opt_surf_reference_image(&o, 64, 48, 64, a.data(), 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                       nullptr, 0, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == SIM3OPT_ERR_ARG);
  }
  std::printf("surf_conformance host: %d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
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
  const int stride = w + 5;  // (rows apart by more than their width, as a cv::Mat's may be)
  std::vector<std::vector<unsigned char>> images((size_t)n_images, std::vector<unsigned char>((size_t)stride * (size_t)h, 0xEE));
  for (auto& im : images)
    for (int y = 0; y < h && ok; ++y)
      for (int x = 0; x < w && ok; ++x) {
        int v = 0;
        ok = std::fscanf(f, "%d", &v) == 1 && v >= 0 && v <= 255;
        im[(size_t)y * (size_t)stride + (size_t)x] = (unsigned char)v;
      }
  std::vector<std::vector<sim3opt_shim::SurfKey>> keys((size_t)n_images);
  std::vector<std::vector<std::vector<float>>> desc((size_t)n_images);
  for (int i = 0; i < n_images && ok; ++i) {
    int count = 0;
    ok = std::fscanf(f, "%d", &count) == 1 && count >= 0;
    for (int k = 0; k < count && ok; ++k) {
      sim3opt_shim::SurfKey q;
      ok = std::fscanf(f, "%f %f %f %f %f %d %d", &q.x, &q.y, &q.size, &q.angle, &q.response, &q.octave, &q.laplacian) == 7;
      std::vector<float> d(64);
      for (int j = 0; j < 64 && ok; ++j) ok = std::fscanf(f, "%f", &d[(size_t)j]) == 1;
      keys[(size_t)i].push_back(q);
      desc[(size_t)i].push_back(d);
    }
  }
  std::fclose(f);
  if (!ok) { std::fprintf(stderr, "malformed file %s\n", path); return 2; }
  sim3opt_shim::SurfExtractorBatch surf;
  surf.options().images_per_pass = 2;  // (more images than a pass)
  for (const auto& im : images) CHECK(surf.add(im.data(), w, h, stride) == SIM3OPT_OK);
  const int rc = surf.extract();
  if (rc < 0) {
    std::fprintf(stderr, "extract failed (%d): %s\n", rc, surf.last_error().c_str());
    return 3;
  }
  int with_keys = 0, total = 0;
  for (int i = 0; i < n_images; ++i) {
    const std::vector<sim3opt_shim::SurfKey> got = surf.keys(i);
    const std::vector<std::vector<float>> gd = surf.descriptors(i);
    const std::vector<sim3opt_shim::SurfKey>& want = keys[(size_t)i];
    bool same = got.size() == want.size() && gd == desc[(size_t)i];
    for (size_t k = 0; same && k < got.size(); ++k)
      same = got[k].x == want[k].x && got[k].y == want[k].y && got[k].size == want[k].size && got[k].angle == want[k].angle &&
             got[k].response == want[k].response && got[k].octave == want[k].octave && got[k].laplacian == want[k].laplacian;
    CHECK(same);
    CHECK(surf.count(i) == (int)want.size() && surf.kp_ptr()[(size_t)i] == total);
    with_keys += !want.empty();
    total += (int)want.size();
  }
  CHECK(rc == with_keys && surf.kp_ptr().back() == total && surf.desc().size() == 64 * (size_t)total && surf.kp().size() == 2 * (size_t)total);
  // the next stages take kp_ptr and desc as they are
  sim3opt_shim::VocabularyTrainer voc(3, 2);
  const int nodes = voc.create(surf.n_frames(), surf.kp_ptr().data(), surf.desc().data());
  if (nodes < 0) {
    std::fprintf(stderr, "create failed (%d): %s\n", nodes, voc.last_error().c_str());
    return 3;
  }
  CHECK(nodes > 1 && voc.words() >= 2);
  sim3opt_shim::LoopDetectorBatch places;
  CHECK(voc.feed(places) == SIM3OPT_OK);
  for (int i = 0; i < surf.n_frames(); ++i) places.add_frame(surf.frame_desc(i), surf.count(i));
  const int rd = places.detect();
  if (rd < 0) {
    std::fprintf(stderr, "detect failed (%d): %s\n", rd, places.last_error().c_str());
    return 3;
  }
  CHECK(places.n_frames() == n_images);
  std::printf("surf_conformance run: %d images, %d keypoints, %d nodes, %d checks, %d failed\n", n_images, total, nodes, g_checks,
              g_failed);
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
