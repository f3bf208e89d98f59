// Stand-alone driver of sim3opt_amd/csrc/surf_host.hpp, the host half of the batched SURF-64 extraction: every refusal
// message as an exact string, the tables, the pattern resizing, the interpolation's solve, the angle and sin / cos
// functions, and the complete serial restatement on small images (a padded row stride, images no layer fits, a cap on
// the keypoints, upright).  Compiled with -fsanitize=address,undefined and run as a child program by
// tests/test_surf_conformance.py: no device, nothing preloaded.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../sim3opt_amd/csrc/surf_host.hpp"

namespace S = sim3opt_surf;

static int failed = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++failed; } \
  } while (0)

// blobs on grey 110 with a deterministic ripple, rows of `stride` bytes (the padding holds 0xEE)
static std::vector<uint8_t> image(int w, int h, int stride) {
  std::vector<uint8_t> p((size_t)stride * (size_t)h, 0xEE);
  const double bx[4] = {0.25 * w, 0.7 * w, 0.4 * w, 0.8 * w}, by[4] = {0.3 * h, 0.35 * h, 0.72 * h, 0.75 * h};
  const double bs[4] = {2.6, 4.0, 3.3, 5.0}, ba[4] = {100, -90, 95, 110};
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      double f = 110 + 3 * std::sin(0.7 * x + 0.3 * y) + 2 * std::cos(0.23 * x - 0.9 * y);
      for (int k = 0; k < 4; ++k) f += ba[k] * std::exp(-((x - bx[k]) * (x - bx[k]) + (y - by[k]) * (y - by[k])) / (2 * bs[k] * bs[k]));
      p[(size_t)y * (size_t)stride + (size_t)x] = (uint8_t)std::lrint(f < 0 ? 0 : f > 255 ? 255 : f);
    }
  return p;
}

static bool same(const S::ImageResult& a, const S::ImageResult& b) {
  if (a.kp.size() != b.kp.size() || a.S != b.S || a.cand.size() != b.cand.size()) return false;
  for (size_t i = 0; i < a.kp.size(); ++i)
    if (std::memcmp(&a.kp[i], &b.kp[i], sizeof(S::Keypoint)) != 0) return false;
  return true;
}

int main() {
  sim3opt_surf_batch_options o;
  S::default_options(o);
  CHECK(o.hessian_threshold == 400 && o.n_octaves == 4 && o.n_octave_layers == 3 && o.upright == 0 && o.max_keypoints == 0 &&
        o.images_per_pass == 64 && o.device == -1);
  CHECK(S::validate_options(o).empty());
  {  // every refusal, word for word
    auto with = [&](auto set) { sim3opt_surf_batch_options q = o; set(q); return S::validate_options(q); };
    CHECK(with([](auto& q) { q.hessian_threshold = -1; }) == "hessian_threshold is negative or not finite");
    CHECK(with([](auto& q) { q.hessian_threshold = std::numeric_limits<double>::quiet_NaN(); }) == S::MSG_THRESHOLD);
    CHECK(with([](auto& q) { q.hessian_threshold = std::numeric_limits<double>::infinity(); }) == S::MSG_THRESHOLD);
    CHECK(with([](auto& q) { q.hessian_threshold = 0; }).empty());
    CHECK(with([](auto& q) { q.n_octaves = 0; }) == "n_octaves outside 1..6" && with([](auto& q) { q.n_octaves = 7; }) == S::MSG_OCTAVES);
    CHECK(with([](auto& q) { q.n_octave_layers = 0; }) == "n_octave_layers outside 1..6");
    CHECK(with([](auto& q) { q.n_octave_layers = 7; }) == S::MSG_LAYERS && with([](auto& q) { q.n_octave_layers = 6; }).empty());
    CHECK(with([](auto& q) { q.upright = 2; }) == "upright is neither 0 nor 1");
    CHECK(with([](auto& q) { q.max_keypoints = -1; }) == "max_keypoints < 0");
    CHECK(with([](auto& q) { q.images_per_pass = 0; }) == "images_per_pass < 1");
    const uint8_t px[4] = {0, 0, 0, 0};
    CHECK(S::validate_images(0, 2, 2, 2, px) == "n_images < 1");
    CHECK(S::validate_images(1, 2, 2, 2, nullptr) == "pixels is NULL");
    CHECK(S::validate_images(1, 0, 2, 2, px) == "width or height < 1" && S::validate_images(1, 2, 0, 2, px) == S::MSG_SIZE);
    CHECK(S::validate_images(1, 2, 2, 1, px) == "row_stride < width");
    CHECK(S::validate_images(1, 4096, 2057, 4096, px) == "255 * width * height does not fit the int32 integral image");
    CHECK(S::validate_images(1, 4096, 2056, 4096, px).empty() && S::validate_images(1, 2, 2, 2, px).empty());
  }
  S::Tables T;
  S::make_tables(T);
  {  // the tables: 113 offsets, i outer; weights symmetric and summing to the disc's share; dw an outer product of sum 1
    CHECK(T.ori_dx[0] == -6 && T.ori_dy[0] == 0 && T.ori_dx[S::ORI_N - 1] == 6 && T.ori_dy[S::ORI_N - 1] == 0);
    CHECK(T.ori_dx[56] == 0 && T.ori_dy[56] == 0);
    double sw = 0, sd = 0;
    for (int k = 0; k < S::ORI_N; ++k) {
      CHECK(T.ori_dx[k] * T.ori_dx[k] + T.ori_dy[k] * T.ori_dy[k] <= 36 && T.ori_w[k] == T.ori_w[S::ORI_N - 1 - k]);
      sw += T.ori_w[k];
    }
    for (int k = 0; k < S::PATCH_SZ * S::PATCH_SZ; ++k) sd += T.dw[k];
    CHECK(sw > 0.9 && sw < 1.0 && std::fabs(sd - 1.0) < 1e-6 && T.dw[0] == T.dw[S::PATCH_SZ * S::PATCH_SZ - 1]);
  }
  {  // resizing: the size-9 patterns at 15 and at 264; the Haar pair at 8
    int src[5];
    S::hessian_pattern(1, src);
    S::Box b = S::resize_box(src, 9, 15);
    CHECK(b.x1 == 5 && b.y1 == 3 && b.x2 == 10 && b.y2 == 12 && b.w == -2.f / 45.f);
    S::hessian_pattern(9, src);
    b = S::resize_box(src, 9, 264);
    CHECK(b.x1 == 147 && b.y1 == 147 && b.x2 == 235 && b.y2 == 235 && b.w == 1.f / (88.f * 88.f));
    S::haar_pattern(3, src);
    b = S::resize_box(src, 4, 8);
    CHECK(b.x1 == 0 && b.y1 == 4 && b.x2 == 8 && b.y2 == 8 && b.w == -1.f / 32.f);
    CHECK(S::layer_size(0, 0) == 9 && S::layer_size(2, 3) == 108 && S::layer_size(3, 4) == 264);
  }
  {  // the solve: a permuted system, a zero pivot, the kept rule
    float A[3][3] = {{0, 2, 0}, {4, 0, 0}, {0, 0, 8}}, b[3] = {2, 4, 8}, x[3];
    CHECK(S::solve3(A, b, x) && x[0] == 1.f && x[1] == 1.f && x[2] == 1.f);
    float Z[3][3] = {{1, 2, 3}, {2, 4, 6}, {1, 1, 1}}, bz[3] = {1, 2, 3};
    CHECK(!S::solve3(Z, bz, x));
    float N[3][9];
    for (int l = 0; l < 3; ++l)
      for (int k = 0; k < 9; ++k) N[l][k] = 0.f;
    CHECK(!S::is_strict_max(N) && !S::interpolate(N, x));  // flat: singular
    N[1][4] = 10.f;
    CHECK(S::is_strict_max(N) && !S::interpolate(N, x));  // symmetric peak: x = 0 is refused
    N[1][5] = 4.f;
    CHECK(S::interpolate(N, x) && x[0] > 0.f && x[0] <= 1.f && x[1] == 0.f && x[2] == 0.f);
    N[1][3] = 10.f;
    CHECK(!S::is_strict_max(N));
  }
  {  // the angle function against atan2 (0.01 degree), sin / cos against libm in double
    const double deg = 180.0 / 3.14159265358979323846;
    for (int k = 0; k < 720; ++k) {
      const double a = k * 0.5 / deg;
      const float y = (float)(7.5 * std::sin(a)), x = (float)(7.5 * std::cos(a));
      double want = std::atan2((double)y, (double)x) * deg;
      if (want < 0) want += 360;
      double d = std::fabs(S::fast_atan2(y, x) - want);
      if (d > 180) d = 360 - d;
      CHECK(d < 0.02);
      float sn, cs;
      S::sincos_deg((float)(k * 0.5), sn, cs);
      CHECK(std::fabs(sn - std::sin(a)) < 1e-7 && std::fabs(cs - std::cos(a)) < 1e-7);
    }
    float sn, cs;
    S::sincos_deg(360.f, sn, cs);
    CHECK(sn == 0.f && cs == 1.f);
    CHECK(S::fast_atan2(0.f, 0.f) == 0.f && S::in_window(359.6f, 0) && S::in_window(29.4f, 0) && !S::in_window(30.f, 0) &&
          S::in_window(2.f, 355));
  }
  // the restatement: blobs are found; the order; unit descriptors; the row stride does not matter
  const int w = 96, h = 80;
  const std::vector<uint8_t> tight = image(w, h, w), padded = image(w, h, w + 13);
  S::ImageResult R, Rp;
  S::reference_image(tight.data(), w, h, w, o, T, R);
  S::reference_image(padded.data(), w, h, w + 13, o, T, Rp);
  CHECK(R.kp.size() >= 4 && R.n_candidates >= R.n_interpolated && (size_t)(R.n_interpolated - R.n_dropped) == R.kp.size());
  CHECK(same(R, Rp));
  CHECK(R.S.size() == (size_t)(w + 1) * (h + 1) && R.S[0] == 0 && R.S[(size_t)w + 1] == 0 && R.S[(size_t)w + 2] == tight[0]);
  for (size_t i = 0; i < R.kp.size(); ++i) {
    const S::Keypoint& k = R.kp[i];
    if (i) CHECK(S::ranks_before(R.kp[i - 1].response, 0, k.response, 1));
    double n2 = 0;
    for (float v : k.desc) { CHECK(std::isfinite(v)); n2 += (double)v * v; }
    CHECK(std::fabs(std::sqrt(n2) - 1) < 1e-5 && k.response > 400 && k.angle >= 0 && k.angle <= 360 && k.size >= 9);
    CHECK(k.x >= 0 && k.x < w && k.y >= 0 && k.y < h && k.laplacian >= -1 && k.laplacian <= 1 && k.octave >= 0 && k.octave < 4);
  }
  for (size_t i = 1; i < R.cand.size(); ++i) CHECK(R.cand[i - 1].key < R.cand[i].key);  // scan order
  {  // a cap keeps the strongest, in order; upright leaves 270
    sim3opt_surf_batch_options q = o;
    q.max_keypoints = 2;
    S::ImageResult C;
    S::reference_image(tight.data(), w, h, w, q, T, C);
    CHECK(C.kp.size() == 2 && std::memcmp(&C.kp[0], &R.kp[0], sizeof(S::Keypoint)) == 0 &&
          std::memcmp(&C.kp[1], &R.kp[1], sizeof(S::Keypoint)) == 0);
    q = o;
    q.upright = 1;
    S::reference_image(tight.data(), w, h, w, q, T, C);
    CHECK(C.kp.size() == R.kp.size());
    for (const S::Keypoint& k : C.kp) CHECK(k.angle == 270.f);
  }
  {  // images no layer fits, one pixel, one row, one column, the most octaves and layers
    sim3opt_surf_batch_options q = o;
    q.n_octaves = 6; q.n_octave_layers = 6; q.hessian_threshold = 0;
    const int dims[6][2] = {{12, 12}, {1, 1}, {40, 1}, {1, 40}, {40, 36}, {33, 65}};
    for (const auto& d : dims) {
      const std::vector<uint8_t> im = image(d[0], d[1], d[0]);
      S::ImageResult E;
      S::reference_image(im.data(), d[0], d[1], d[0], q, T, E);
      CHECK(E.S.size() == (size_t)(d[0] + 1) * (d[1] + 1));
      if (d[0] < 15 || d[1] < 15) CHECK(E.kp.empty() && E.n_candidates == 0);
    }
    // a keypoint at the border: orientation samples outside, a clamped descriptor window
    float angle, desc[S::DESC], patch[S::PATCH * S::PATCH];
    S::OrientationTrace tr;
    CHECK(S::describe(tight.data(), R.S.data(), w, h, T, 0, 1.5f, 2.25f, 40.f, angle, desc, &tr, patch));
    int valid = 0;
    for (int k = 0; k < S::ORI_N; ++k) valid += tr.valid[k];
    CHECK(valid > 0 && valid < S::ORI_N);
    CHECK(!S::describe(tight.data(), R.S.data(), w, h, T, 0, 40.f, 40.f, 400.f, angle, desc));  // a Haar window larger than the image
    CHECK(!S::describe(tight.data(), R.S.data(), w, h, T, 1, 40.f, 40.f, 400.f, angle, desc));
  }
  if (failed) {
    std::printf("%d failed\n", failed);
    return 1;
  }
  std::printf("surf host ok\n");
  return 0;
}
