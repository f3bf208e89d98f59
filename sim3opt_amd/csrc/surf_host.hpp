// surf_host.hpp -- the host half of the batched SURF-64 extraction (surf_batch.hip): the tile sizes, the checks of the
// options and of the images with their messages, the tables (the two Gaussians, the 113 orientation offsets), the
// per-item arithmetic of include/sim3opt.h's definition ("batched SURF-64 extraction") as functions the kernels call as
// well, and a complete serial restatement of the definition for one image (reference_image).  Every floating-point
// step is FP32, rounded once and never fused; nothing here calls a libm function whose last bit may differ between the
// host and the device (the tables are made once on the host in double).  Plain C++ with no HIP in it, so
// tests/cxx/surf_host_driver.cpp runs it under the host sanitizers.
#pragma once

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/sim3opt.h"
#include "handle_host.hpp"

#if defined(__HIP__)
#include <hip/hip_runtime.h>
#define SIM3OPT_SURF_HD __host__ __device__ inline
#else
#define SIM3OPT_SURF_HD inline
#endif

// the definition's arithmetic is written out operation by operation: the device rounds every one as the host does
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace sim3opt_surf {

constexpr int DESC = 64;
constexpr int MAX_OCTAVES = 6, MAX_OCTAVE_LAYERS = 6, MAX_LAYERS = MAX_OCTAVE_LAYERS + 2;
constexpr int TILE = 32;         // the detection kernel's tile of an octave's plane (a one-sample halo around it in LDS)
constexpr int DET_THREADS = 256;
constexpr int RANK_TILE = 256;   // keys of an image staged in LDS at a time by the ranking
constexpr int KP_LANES = 64;     // the lanes that work on one keypoint's orientation and descriptor
constexpr int ORI_TAPS = 13, ORI_RADIUS = 6, ORI_N = 113, ORI_WINDOWS = 72;  // [upstream recall]
constexpr int PATCH_SZ = 20, PATCH = PATCH_SZ + 1;                            // [upstream recall]
constexpr int N_BOXES = 10;      // Dxx 3, Dyy 3, Dxy 4

// every refusal, word for word
constexpr const char* MSG_THRESHOLD = "hessian_threshold is negative or not finite";
constexpr const char* MSG_OCTAVES = "n_octaves outside 1..6";
constexpr const char* MSG_LAYERS = "n_octave_layers outside 1..6";
constexpr const char* MSG_UPRIGHT = "upright is neither 0 nor 1";
constexpr const char* MSG_MAX_KP = "max_keypoints < 0";
constexpr const char* MSG_PER_PASS = "images_per_pass < 1";
constexpr const char* MSG_N_IMAGES = "n_images < 1";
constexpr const char* MSG_NULL = "pixels is NULL";
constexpr const char* MSG_SIZE = "width or height < 1";
constexpr const char* MSG_STRIDE = "row_stride < width";
constexpr const char* MSG_TOO_LARGE = "255 * width * height does not fit the int32 integral image";

inline std::string validate_options(const sim3opt_surf_batch_options& o) {
  if (!(o.hessian_threshold >= 0) || !std::isfinite(o.hessian_threshold)) return MSG_THRESHOLD;
  if (o.n_octaves < 1 || o.n_octaves > MAX_OCTAVES) return MSG_OCTAVES;
  if (o.n_octave_layers < 1 || o.n_octave_layers > MAX_OCTAVE_LAYERS) return MSG_LAYERS;
  if (o.upright != 0 && o.upright != 1) return MSG_UPRIGHT;
  if (o.max_keypoints < 0) return MSG_MAX_KP;
  if (o.images_per_pass < 1) return MSG_PER_PASS;
  return "";
}

inline std::string validate_images(int32_t n_images, int32_t width, int32_t height, int32_t row_stride,
                                   const uint8_t* pixels) {
  if (n_images < 1) return MSG_N_IMAGES;
  if (!pixels) return MSG_NULL;
  if (width < 1 || height < 1) return MSG_SIZE;
  if (row_stride < width) return MSG_STRIDE;
  if ((int64_t)255 * width * height >= ((int64_t)1 << 31)) return MSG_TOO_LARGE;
  return "";
}

inline void default_options(sim3opt_surf_batch_options& o) {
  o.hessian_threshold = 400;  // the call site: SURF::create(400), kitti_surf.cpp:501-523
  o.n_octaves = 4;            // [upstream recall]
  o.n_octave_layers = 3;      // [upstream recall]
  o.upright = 0;
  o.max_keypoints = 0;
  o.images_per_pass = 64;
  o.device = -1;
}

// ---- tables ----------------------------------------------------------------------------------------------------------
// n taps of exp(-x^2 / (2 sigma^2)), x = i - (n - 1) / 2, scaled to sum 1: in double, rounded once to FP32  [upstream recall]
inline void gaussian_taps(int n, double sigma, float* out) {
  std::vector<double> t((size_t)n);
  double sum = 0;
  for (int i = 0; i < n; ++i) {
    const double x = i - (n - 1) * 0.5;
    t[(size_t)i] = std::exp(-0.5 / (sigma * sigma) * x * x);
    sum += t[(size_t)i];
  }
  for (int i = 0; i < n; ++i) out[i] = (float)(t[(size_t)i] / sum);
}

// what the orientation and descriptor steps read: a plain aggregate, uploaded as it is
struct Tables {
  int32_t ori_dx[ORI_N], ori_dy[ORI_N];  // the grid points i^2 + j^2 <= 36, i outer and j inner; dx = i, dy = j
  float ori_w[ORI_N];                    // G13[i + 6] * G13[j + 6], an FP32 product
  float dw[PATCH_SZ * PATCH_SZ];         // G20[row] * G20[column]
};

inline void make_tables(Tables& T, double ori_sigma = 2.5, double desc_sigma = 3.3) {
  float g13[ORI_TAPS], g20[PATCH_SZ];
  gaussian_taps(ORI_TAPS, ori_sigma, g13);
  gaussian_taps(PATCH_SZ, desc_sigma, g20);
  int n = 0;
  for (int i = -ORI_RADIUS; i <= ORI_RADIUS; ++i)
    for (int j = -ORI_RADIUS; j <= ORI_RADIUS; ++j)
      if (i * i + j * j <= ORI_RADIUS * ORI_RADIUS) {
        T.ori_dx[n] = i; T.ori_dy[n] = j;
        T.ori_w[n] = g13[i + ORI_RADIUS] * g13[j + ORI_RADIUS];
        ++n;
      }
  for (int i = 0; i < PATCH_SZ; ++i)
    for (int j = 0; j < PATCH_SZ; ++j) T.dw[i * PATCH_SZ + j] = g20[i] * g20[j];
}

// ---- the box patterns ------------------------------------------------------------------------------------------------
struct Box {
  int32_t x1, y1, x2, y2;
  float w;
};

// size 9: Dxx (3), Dyy (3, the transpose), Dxy (4); {x1, y1, x2, y2, weight}
SIM3OPT_SURF_HD void hessian_pattern(int k, int src[5]) {
  const int P[N_BOXES][5] = {{0, 2, 3, 7, 1}, {3, 2, 6, 7, -2}, {6, 2, 9, 7, 1},  {2, 0, 7, 3, 1},   {2, 3, 7, 6, -2},
                             {2, 6, 7, 9, 1}, {1, 1, 4, 4, 1},  {5, 1, 8, 4, -1}, {1, 5, 4, 8, -1}, {5, 5, 8, 8, 1}};
  for (int q = 0; q < 5; ++q) src[q] = P[k][q];
}
// size 4: the Haar pair in x (2), then in y (2)
SIM3OPT_SURF_HD void haar_pattern(int k, int src[5]) {
  const int P[4][5] = {{0, 0, 2, 4, -1}, {2, 0, 4, 4, 1}, {0, 0, 4, 2, 1}, {0, 2, 4, 4, -1}};
  for (int q = 0; q < 5; ++q) src[q] = P[k][q];
}
// every corner coordinate c becomes rint(fl(new_size / old_size) * c) (half to even; no half occurs for the sizes of
// the definition), the weight fl(w / fl(area))
SIM3OPT_SURF_HD Box resize_box(const int src[5], int old_size, int new_size) {
  const float ratio = (float)new_size / (float)old_size;
  Box b;
  b.x1 = (int32_t)rintf(ratio * (float)src[0]); b.y1 = (int32_t)rintf(ratio * (float)src[1]);
  b.x2 = (int32_t)rintf(ratio * (float)src[2]); b.y2 = (int32_t)rintf(ratio * (float)src[3]);
  b.w = (float)src[4] / ((float)(b.x2 - b.x1) * (float)(b.y2 - b.y1));
  return b;
}

SIM3OPT_SURF_HD int layer_size(int octave, int layer) { return (9 + 6 * layer) << octave; }

// S: (h + 1) x (w + 1), stride w + 1.  Sum of `n` boxes anchored at (y, x): int32 box sum -> float, times the weight,
// added in pattern order.
SIM3OPT_SURF_HD float box_response(const int32_t* S, int stride, int y, int x, const Box* b, int n) {
  float d = 0.f;
  for (int k = 0; k < n; ++k) {
    const int32_t* p = S + (size_t)(y + b[k].y1) * (size_t)stride + (size_t)x;
    const int32_t* q = S + (size_t)(y + b[k].y2) * (size_t)stride + (size_t)x;
    const int32_t sum = p[b[k].x1] + q[b[k].x2] - q[b[k].x1] - p[b[k].x2];
    d = d + (float)sum * b[k].w;
  }
  return d;
}

SIM3OPT_SURF_HD void hessian_at(const int32_t* S, int stride, int y, int x, const Box* b, float& det, float& trace) {
  const float dx = box_response(S, stride, y, x, b, 3);
  const float dy = box_response(S, stride, y, x, b + 3, 3);
  const float dxy = box_response(S, stride, y, x, b + 6, 4);
  const float t = (0.81f * dxy) * dxy;
  det = dx * dy - t;
  trace = dx + dy;
}

// Entry (i, j) of the response plane of a layer of filter size `size` at sample step `step`: 0 outside the samples
// that fit (and everywhere when the filter does not fit the image).
SIM3OPT_SURF_HD bool plane_sample(int w, int h, int size, int step, int i, int j, int& y, int& x) {
  if (size > h || size > w) return false;
  const int margin = (size / 2) / step, si = i - margin, sj = j - margin;
  if (si < 0 || sj < 0 || si >= 1 + (h - size) / step || sj >= 1 + (w - size) / step) return false;
  y = si * step; x = sj * step;
  return true;
}

// ---- interpolation ---------------------------------------------------------------------------------------------------
// A x = b by elimination with partial pivoting (the first row of largest magnitude in the column), FP32: false on a
// zero pivot
SIM3OPT_SURF_HD bool solve3(float A[3][3], float b[3], float x[3]) {
  for (int c = 0; c < 3; ++c) {
    int p = c;
    for (int r = c + 1; r < 3; ++r)
      if (fabsf(A[r][c]) > fabsf(A[p][c])) p = r;
    if (A[p][c] == 0.f || !(fabsf(A[p][c]) > 0.f)) return false;
    if (p != c) {
      for (int k = 0; k < 3; ++k) { const float t = A[c][k]; A[c][k] = A[p][k]; A[p][k] = t; }
      const float t = b[c]; b[c] = b[p]; b[p] = t;
    }
    for (int r = c + 1; r < 3; ++r) {
      const float f = A[r][c] / A[c][c];
      for (int k = c + 1; k < 3; ++k) A[r][k] = A[r][k] - f * A[c][k];
      b[r] = b[r] - f * b[c];
    }
  }
  x[2] = b[2] / A[2][2];
  x[1] = (b[1] - A[1][2] * x[2]) / A[1][1];
  x[0] = ((b[0] - A[0][1] * x[1]) - A[0][2] * x[2]) / A[0][0];
  return true;
}

// N[l][3 (di + 1) + (dj + 1)]: the 27 values around a maximum, l = 0 the layer below.  x = (d column, d row, d layer).
SIM3OPT_SURF_HD bool interpolate(const float N[3][9], float x[3]) {
  float b[3] = {-((N[1][5] - N[1][3]) / 2.f), -((N[1][7] - N[1][1]) / 2.f), -((N[2][4] - N[0][4]) / 2.f)};
  const float c2 = 2.f * N[1][4];
  const float axy = (((N[1][8] - N[1][6]) - N[1][2]) + N[1][0]) / 4.f;
  const float axs = (((N[2][5] - N[2][3]) - N[0][5]) + N[0][3]) / 4.f;
  const float ays = (((N[2][7] - N[2][1]) - N[0][7]) + N[0][1]) / 4.f;
  float A[3][3] = {{(N[1][3] - c2) + N[1][5], axy, axs}, {axy, (N[1][1] - c2) + N[1][7], ays}, {axs, ays, (N[0][4] - c2) + N[2][4]}};
  if (!solve3(A, b, x)) return false;
  if (x[0] == 0.f && x[1] == 0.f && x[2] == 0.f) return false;
  return fabsf(x[0]) <= 1.f && fabsf(x[1]) <= 1.f && fabsf(x[2]) <= 1.f;  // (false for a NaN)
}

// what the detection writes per strict maximum above the threshold
struct Cand {
  int32_t key;             // the scan index: ((octave * n_octave_layers + layer - 1) * h + i) * w + j
  float x0, y0, size0;     // the centre and size before interpolation
  float response;
  float x, y, size;        // after (as before where the candidate is not kept)
  int32_t octave, layer, laplacian, kept;
};

// The candidate at (i, j) of middle layer `layer`, from its 27 values and the trace at the maximum.
SIM3OPT_SURF_HD Cand make_candidate(const float N[3][9], float trace, int octave, int layer, int n_octave_layers, int i, int j,
                                    int w, int h) {
  const int step = 1 << octave, size = layer_size(octave, layer), ds = size - layer_size(octave, layer - 1);
  Cand c;
  c.key = ((octave * n_octave_layers + layer - 1) * h + i) * w + j;
  c.x0 = (float)(step * (j - (size / 2) / step)) + (float)(size - 1) * 0.5f;
  c.y0 = (float)(step * (i - (size / 2) / step)) + (float)(size - 1) * 0.5f;
  c.size0 = (float)size;
  c.response = N[1][4];
  c.octave = octave; c.layer = layer;
  c.laplacian = (trace > 0.f) - (trace < 0.f);
  c.x = c.x0; c.y = c.y0; c.size = c.size0;
  float x[3];
  c.kept = interpolate(N, x) ? 1 : 0;
  if (c.kept) {
    c.x = c.x0 + x[0] * (float)step;
    c.y = c.y0 + x[1] * (float)step;
    c.size = rintf(c.size0 + x[2] * (float)ds);
  }
  return c;
}

// strictly greater than the 26 others
SIM3OPT_SURF_HD bool is_strict_max(const float N[3][9]) {
  const float v = N[1][4];
  for (int l = 0; l < 3; ++l)
    for (int k = 0; k < 9; ++k)
      if (!(l == 1 && k == 4) && !(v > N[l][k])) return false;
  return true;
}

// a ranks before b: response descending, then scan index ascending
SIM3OPT_SURF_HD bool ranks_before(float ra, int32_t ka, float rb, int32_t kb) { return ra > rb || (ra == rb && ka < kb); }

// ---- orientation -----------------------------------------------------------------------------------------------------
// degrees in [0, 360]: the odd degree-7 polynomial in min / max of |x|, |y| with the octant fix-ups  [upstream recall]
SIM3OPT_SURF_HD float fast_atan2(float y, float x) {
  const float scale = (float)(180.0 / 3.14159265358979323846);
  const float p1 = 0.9997878412794807f * scale, p3 = -0.3258083974640975f * scale, p5 = 0.1555786518463281f * scale,
              p7 = -0.04432655554792128f * scale;
  const float ax = fabsf(x), ay = fabsf(y);
  float a, c, c2;
  if (ax >= ay) {
    c = ay / (ax + (float)DBL_EPSILON);
    c2 = c * c;
    a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
  } else {
    c = ax / (ay + (float)DBL_EPSILON);
    c2 = c * c;
    a = 90.f - (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
  }
  if (x < 0.f) a = 180.f - a;
  if (y < 0.f) a = 360.f - a;
  return a;
}

// sin and cos of an angle in degrees as plain arithmetic (ours: upstream calls libm).  The quadrant q = (int)(a / 90)
// comes off exactly in double, the rest r in [0, 90) goes to radians, and sin r, cos r are the Taylor polynomials to
// r^19 and r^18 by Horner in double, neither fused; the quadrant turns them, and each is rounded once to FP32.
SIM3OPT_SURF_HD void sincos_deg(float angle, float& s, float& c) {
  double a = (double)angle;
  int q = (int)(a / 90.0);
  if (q < 0) q = 0;
  const double r = (a - 90.0 * (double)q) * (3.14159265358979323846 / 180.0), r2 = r * r;
  double sn = 1.0, cs = 1.0;
  for (int k = 9; k >= 1; --k) {
    sn = 1.0 - sn * r2 / (double)((2 * k) * (2 * k + 1));
    cs = 1.0 - cs * r2 / (double)((2 * k - 1) * (2 * k));
  }
  sn = sn * r;
  double ss, cc;
  switch (q & 3) {
    case 0: ss = sn; cc = cs; break;
    case 1: ss = cs; cc = -sn; break;
    case 2: ss = -sn; cc = -cs; break;
    default: ss = -cs; cc = sn; break;
  }
  s = (float)ss; c = (float)cc;
}

struct KpGeometry {
  float s;       // size * 1.2 / 9
  int32_t g;     // the Haar size, 2 rint(2 s)
  int32_t win;   // (int)(21 s)
  Box haar[4];
};

SIM3OPT_SURF_HD KpGeometry kp_geometry(float size) {
  KpGeometry G;
  G.s = size * 1.2f / 9.0f;
  G.g = 2 * (int32_t)rintf(2.f * G.s);
  G.win = (int32_t)((float)PATCH * G.s);
  for (int k = 0; k < 4; ++k) {
    int src[5];
    haar_pattern(k, src);
    G.haar[k] = resize_box(src, 4, G.g > 0 ? G.g : 4);
  }
  return G;
}

// orientation sample k of a keypoint at (cx, cy): false when its Haar window leaves the integral image
SIM3OPT_SURF_HD bool ori_sample(const int32_t* S, int w, int h, float cx, float cy, const KpGeometry& G, const Tables& T, int k,
                                float& vx, float& vy) {
  if (G.g < 2) return false;
  const float off = (float)(G.g - 1) / 2.f;
  const int x = (int)rintf((cx + (float)T.ori_dx[k] * G.s) - off), y = (int)rintf((cy + (float)T.ori_dy[k] * G.s) - off);
  if (y < 0 || y >= h + 1 - G.g || x < 0 || x >= w + 1 - G.g) return false;
  vx = box_response(S, w + 1, y, x, G.haar, 2) * T.ori_w[k];
  vy = box_response(S, w + 1, y, x, G.haar + 2, 2) * T.ori_w[k];
  return true;
}

// is a sample of angle `ang` (degrees) inside the 60-degree window centred at c
SIM3OPT_SURF_HD bool in_window(float ang, int c) {
  int d = (int)rintf(ang) - c;
  if (d < 0) d = -d;
  return d < 30 || d > 330;
}

// ---- descriptor ------------------------------------------------------------------------------------------------------
// Window sample (row i, column j) of the win x win window turned by (sin_dir, cos_dir) about (cx, cy): the bilinear
// value rounded to an integer where the four taps exist, else the pixel at the clamped rounded coordinate.
SIM3OPT_SURF_HD int win_sample(const uint8_t* img, int w, int h, float cx, float cy, float sin_dir, float cos_dir, int win, int i,
                               int j) {
  const float off = -(float)(win - 1) / 2.f;
  const float fj = (float)j + off, fi = (float)i + off;
  const float px = (cx + fj * cos_dir) + fi * sin_dir;
  const float py = (cy - fj * sin_dir) + fi * cos_dir;
  const float flx = floorf(px), fly = floorf(py);
  if (flx >= 0.f && fly >= 0.f && flx < (float)(w - 1) && fly < (float)(h - 1)) {
    const int ix = (int)flx, iy = (int)fly;
    const float a = px - flx, b = py - fly;
    const uint8_t* p = img + (size_t)iy * (size_t)w + (size_t)ix;
    const float v = (((float)p[0] * (1.f - a)) * (1.f - b) + ((float)p[1] * a) * (1.f - b)) + ((float)p[w] * (1.f - a)) * b +
                    ((float)p[w + 1] * a) * b;
    return (int)rintf(v);
  }
  float rx = rintf(px), ry = rintf(py);
  rx = rx < 0.f ? 0.f : rx > (float)(w - 1) ? (float)(w - 1) : rx;  // (a NaN cannot occur: the centre is finite)
  ry = ry < 0.f ? 0.f : ry > (float)(h - 1) ? (float)(h - 1) : ry;
  return (int)img[(size_t)(int)ry * (size_t)w + (size_t)(int)rx];
}

// Patch cell (row u, column v) of 21 x 21: the area average of the window over [u win/21, (u+1) win/21) x [v ...),
// row-major within the cell, divided by the cell's area, rounded to an integer.
SIM3OPT_SURF_HD float patch_cell(const uint8_t* img, int w, int h, float cx, float cy, float sin_dir, float cos_dir, int win, int u,
                                 int v) {
  const float scale = (float)win / (float)PATCH;
  const float ya = (float)u * scale, yb = (float)(u + 1) * scale, xa = (float)v * scale, xb = (float)(v + 1) * scale;
  int i0 = (int)floorf(ya), i1 = (int)ceilf(yb) - 1, j0 = (int)floorf(xa), j1 = (int)ceilf(xb) - 1;
  if (i1 > win - 1) i1 = win - 1;
  if (j1 > win - 1) j1 = win - 1;
  float acc = 0.f;
  for (int i = i0; i <= i1; ++i) {
    const float lo = ya > (float)i ? ya : (float)i, hi = yb < (float)(i + 1) ? yb : (float)(i + 1);
    const float wy = hi - lo;
    if (!(wy > 0.f)) continue;
    for (int j = j0; j <= j1; ++j) {
      const float l2 = xa > (float)j ? xa : (float)j, h2 = xb < (float)(j + 1) ? xb : (float)(j + 1);
      const float wx = h2 - l2;
      if (!(wx > 0.f)) continue;
      acc = acc + (wy * wx) * (float)win_sample(img, w, h, cx, cy, sin_dir, cos_dir, win, i, j);
    }
  }
  float r = rintf(acc / (scale * scale));
  return r < 0.f ? 0.f : r > 255.f ? 255.f : r;
}

// the two gradients at (row y, column x) of the 20 x 20 interior of the patch
SIM3OPT_SURF_HD void patch_gradient(const float* patch, const Tables& T, int y, int x, float& vx, float& vy) {
  const float p00 = patch[y * PATCH + x], p01 = patch[y * PATCH + x + 1], p10 = patch[(y + 1) * PATCH + x],
              p11 = patch[(y + 1) * PATCH + x + 1], dw = T.dw[y * PATCH_SZ + x];
  vx = (((p01 - p00) + p11) - p10) * dw;
  vy = (((p10 - p00) + p11) - p01) * dw;
}

// the four sums of sub-region r (row-major of 4 x 4), its 25 samples row-major
SIM3OPT_SURF_HD void subregion_sums(const float* patch, const Tables& T, int r, float out[4]) {
  const int i = r / 4, j = r % 4;
  out[0] = out[1] = out[2] = out[3] = 0.f;
  for (int y = i * 5; y < i * 5 + 5; ++y)
    for (int x = j * 5; x < j * 5 + 5; ++x) {
      float vx, vy;
      patch_gradient(patch, T, y, x, vx, vy);
      out[0] = out[0] + vx; out[1] = out[1] + vy; out[2] = out[2] + fabsf(vx); out[3] = out[3] + fabsf(vy);
    }
}

// 1 / (sqrt(sum of the 64 squares in ascending index) + FLT_EPSILON)
SIM3OPT_SURF_HD float descriptor_scale(const float* d) {
  float sq = 0.f;
  for (int k = 0; k < DESC; ++k) sq = sq + d[k] * d[k];
  return 1.f / (sqrtf(sq) + FLT_EPSILON);
}

// ---- the serial restatement ------------------------------------------------------------------------------------------
struct Keypoint {
  float x, y, size, angle, response;
  int32_t octave, laplacian;
  int32_t rank;  // its place in the response order before the orientation step dropped any
  float desc[DESC];
};

struct OrientationTrace {
  int32_t valid[ORI_N];
  float vx[ORI_N], vy[ORI_N], angle[ORI_N], window[ORI_WINDOWS];
};

struct ImageResult {
  std::vector<int32_t> S;
  std::vector<Cand> cand;  // scan order
  std::vector<Keypoint> kp;
  int32_t n_candidates = 0, n_interpolated = 0, n_dropped = 0;
};

inline void integral_image(const uint8_t* img, int w, int h, int stride, std::vector<int32_t>& S) {
  S.assign((size_t)(w + 1) * (size_t)(h + 1), 0);
  for (int y = 0; y < h; ++y) {
    int32_t run = 0;
    for (int x = 0; x < w; ++x) {
      run += img[(size_t)y * (size_t)stride + (size_t)x];
      S[(size_t)(y + 1) * (size_t)(w + 1) + (size_t)(x + 1)] = S[(size_t)y * (size_t)(w + 1) + (size_t)(x + 1)] + run;
    }
  }
}

// det and trace planes of one layer: (h / step) x (w / step), zero outside the samples
inline void response_plane(const int32_t* S, int w, int h, int octave, int layer, std::vector<float>& det,
                           std::vector<float>& trace) {
  const int step = 1 << octave, size = layer_size(octave, layer), rows = h / step, cols = w / step;
  det.assign((size_t)rows * (size_t)cols, 0.f);
  trace.assign((size_t)rows * (size_t)cols, 0.f);
  Box b[N_BOXES];
  for (int k = 0; k < N_BOXES; ++k) { int src[5]; hessian_pattern(k, src); b[k] = resize_box(src, 9, size); }
  for (int i = 0; i < rows; ++i)
    for (int j = 0; j < cols; ++j) {
      int y, x;
      if (plane_sample(w, h, size, step, i, j, y, x))
        hessian_at(S, w + 1, y, x, b, det[(size_t)i * (size_t)cols + (size_t)j], trace[(size_t)i * (size_t)cols + (size_t)j]);
    }
}

// Orientation and descriptor of one keypoint (x, y, size): false when the orientation step drops it.  `tight` is the
// image with rows of w bytes.
inline bool describe(const uint8_t* tight, const int32_t* S, int w, int h, const Tables& T, int upright, float x, float y,
                     float size, float& angle, float* desc, OrientationTrace* trace = nullptr, float* patch_out = nullptr) {
  const KpGeometry G = kp_geometry(size);
  angle = 270.f;  // [upstream recall] what upright leaves
  if (!upright) {
    float vx[ORI_N], vy[ORI_N], ang[ORI_N];
    bool ok[ORI_N];
    int n = 0;
    for (int k = 0; k < ORI_N; ++k) {
      vx[k] = vy[k] = ang[k] = 0.f;
      ok[k] = ori_sample(S, w, h, x, y, G, T, k, vx[k], vy[k]);
      if (ok[k]) { ang[k] = fast_atan2(vy[k], vx[k]); ++n; }
      if (trace) { trace->valid[k] = ok[k]; trace->vx[k] = vx[k]; trace->vy[k] = vy[k]; trace->angle[k] = ang[k]; }
    }
    if (n == 0) return false;
    float best = 0.f, bx = 0.f, by = 0.f;
    for (int c = 0; c < ORI_WINDOWS; ++c) {
      float sx = 0.f, sy = 0.f;
      for (int k = 0; k < ORI_N; ++k)
        if (ok[k] && in_window(ang[k], 5 * c)) { sx = sx + vx[k]; sy = sy + vy[k]; }
      const float m = sx * sx + sy * sy;
      if (trace) trace->window[c] = m;
      if (m > best) { best = m; bx = sx; by = sy; }
    }
    angle = fast_atan2(-by, bx);
  } else if (G.g > h + 1 || G.g > w + 1) {
    return false;
  }
  if (G.win < 1) return false;
  float sn, cs;
  sincos_deg(angle, sn, cs);
  const float sin_dir = -sn, cos_dir = cs;
  float patch[PATCH * PATCH];
  for (int u = 0; u < PATCH; ++u)
    for (int v = 0; v < PATCH; ++v) patch[u * PATCH + v] = patch_cell(tight, w, h, x, y, sin_dir, cos_dir, G.win, u, v);
  if (patch_out) std::copy(patch, patch + PATCH * PATCH, patch_out);
  for (int r = 0; r < 16; ++r) subregion_sums(patch, T, r, desc + 4 * r);
  const float sc = descriptor_scale(desc);
  for (int k = 0; k < DESC; ++k) desc[k] = desc[k] * sc;
  return true;
}

inline void reference_image(const uint8_t* img, int w, int h, int stride, const sim3opt_surf_batch_options& o, const Tables& T,
                            ImageResult& R) {
  std::vector<uint8_t> tight((size_t)w * (size_t)h);
  for (int y = 0; y < h; ++y) std::copy(img + (size_t)y * (size_t)stride, img + (size_t)y * (size_t)stride + (size_t)w, tight.begin() + (size_t)y * (size_t)w);
  integral_image(img, w, h, stride, R.S);
  const int32_t* S = R.S.data();
  const float thr = (float)o.hessian_threshold;
  const int nl = o.n_octave_layers;
  R.cand.clear(); R.kp.clear();
  std::vector<std::vector<float>> det((size_t)nl + 2), tr((size_t)nl + 2);
  for (int oc = 0; oc < o.n_octaves; ++oc) {
    const int step = 1 << oc, rows = h / step, cols = w / step;
    for (int l = 0; l < nl + 2; ++l) response_plane(S, w, h, oc, l, det[(size_t)l], tr[(size_t)l]);
    for (int l = 1; l <= nl; ++l) {
      const int margin = (layer_size(oc, l + 1) / 2) / step + 1;
      for (int i = margin; i < rows - margin; ++i)
        for (int j = margin; j < cols - margin; ++j) {
          const float v = det[(size_t)l][(size_t)i * (size_t)cols + (size_t)j];
          if (!(v > thr)) continue;
          float N[3][9];
          for (int q = 0; q < 3; ++q)
            for (int di = -1; di <= 1; ++di)
              for (int dj = -1; dj <= 1; ++dj)
                N[q][3 * (di + 1) + dj + 1] = det[(size_t)(l - 1 + q)][(size_t)(i + di) * (size_t)cols + (size_t)(j + dj)];
          if (!is_strict_max(N)) continue;
          R.cand.push_back(make_candidate(N, tr[(size_t)l][(size_t)i * (size_t)cols + (size_t)j], oc, l, nl, i, j, w, h));
        }
    }
  }
  R.n_candidates = (int32_t)R.cand.size();
  std::vector<const Cand*> kept;
  for (const Cand& c : R.cand)
    if (c.kept) kept.push_back(&c);
  R.n_interpolated = (int32_t)kept.size();
  std::stable_sort(kept.begin(), kept.end(),
                   [](const Cand* a, const Cand* b) { return ranks_before(a->response, a->key, b->response, b->key); });
  if (o.max_keypoints > 0 && kept.size() > (size_t)o.max_keypoints) kept.resize((size_t)o.max_keypoints);
  R.n_dropped = 0;
  for (size_t r = 0; r < kept.size(); ++r) {
    const Cand& c = *kept[r];
    Keypoint k;
    k.x = c.x; k.y = c.y; k.size = c.size; k.response = c.response; k.octave = c.octave; k.laplacian = c.laplacian;
    k.rank = (int32_t)r;
    if (describe(tight.data(), S, w, h, T, o.upright, k.x, k.y, k.size, k.angle, k.desc)) R.kp.push_back(k);
    else ++R.n_dropped;
  }
}

}  // namespace sim3opt_surf
