// track_math.hpp -- the arithmetic of the loop-track stage that the host restatement (track_host.hpp) and the kernels
// (track_batch.hip) share: the frame of a global observation index, the depth an observation carries, the point of a
// track and its status.  include/sim3opt.h ("batched loop tracks") is the specification.  Compiled for host and device
// with contraction off, like pnp_math.hpp and essential_math.hpp: the same operations in the same order round alike, so
// the device's points equal the restatement's to the bit.  Plain C++; no array is indexed by a run-time value, so
// nothing of it lands in scratch.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define SIM3OPT_TRACK_HD __host__ __device__
#else
#define SIM3OPT_TRACK_HD
#endif
#if defined(__clang__)
#define SIM3OPT_TRACK_NO_FMA _Pragma("clang fp contract(off)")
#else
#define SIM3OPT_TRACK_NO_FMA
#endif

namespace sim3opt_track {

constexpr int32_t NONE = INT32_MAX;  // no label, no match, no depth key

enum : int32_t { TRACK_OK = 0, TRACK_CONFLICT = 1, TRACK_NO_DEPTH = 2, TRACK_BEHIND = 3, TRACK_REPROJECTION = 4 };

// the sizes at which a kernel takes another path (sim3opt_track_batch_dims, tiles[])
constexpr int WORKGROUP = 256;  // lanes of every workgroup
constexpr int SCAN_TILE = 256;  // entries a workgroup of the scans covers; the carry crosses tiles
constexpr int LANE_MAX = 8;     // a segment of up to LANE_MAX observations is ordered by one lane
constexpr int WAVE_MAX = 64;    // ... of up to WAVE_MAX by one wavefront, a longer one by a workgroup

// a depth that is finite and > 0 is present (NaN fails the first comparison, +inf the second)
SIM3OPT_TRACK_HD inline bool depth_present(double d) { return d > 0.0 && d <= 1.7976931348623157e308; }

// the frame that owns global observation g: kp_ptr[f] <= g < kp_ptr[f + 1] (frames that own nothing are passed over)
SIM3OPT_TRACK_HD inline int32_t frame_of(const int32_t* kp_ptr, int32_t n_frames, int32_t g) {
  int32_t lo = 0, hi = n_frames;  // the first f in (lo, hi] with kp_ptr[f] > g, minus one
  while (hi - lo > 1) {
    const int32_t mid = lo + (hi - lo) / 2;
    if (kp_ptr[mid] <= g) lo = mid; else hi = mid;
  }
  return lo;
}

struct Rot { double r00, r01, r02, r10, r11, r12, r20, r21, r22; };

// the rotation matrix of the unit quaternion q = [x y z w]
SIM3OPT_TRACK_HD inline Rot rot_of(const double* q) {
  SIM3OPT_TRACK_NO_FMA
  const double x = q[0], y = q[1], z = q[2], w = q[3];
  Rot R;
  R.r00 = 1.0 - 2.0 * (y * y + z * z); R.r01 = 2.0 * (x * y - z * w); R.r02 = 2.0 * (x * z + y * w);
  R.r10 = 2.0 * (x * y + z * w); R.r11 = 1.0 - 2.0 * (x * x + z * z); R.r12 = 2.0 * (y * z - x * w);
  R.r20 = 2.0 * (x * z - y * w); R.r21 = 2.0 * (y * z + x * w); R.r22 = 1.0 - 2.0 * (x * x + y * y);
  return R;
}

// what the point of a track is computed from; every pointer is the host's on the host and the device's on the device
struct PointArgs {
  const int32_t* kp_ptr;   // n_frames + 1
  int32_t n_frames;
  const float* kp;         // pixels of the observations, by g
  const int32_t* dkey;     // per g: 2 * match + side of the lowest kept match that gives g a depth, or NONE
  const double *depth0, *depth1;  // per match (NULL: absent)
  const double* states;    // n_frames x 8, [qx qy qz qw tx ty tz s] of S_iw
  double focal, cx, cy, max_reproj_px;
};

// The point X and the status of the track whose observations seg[0 .. len) are ascending in g.  n_depths: the
// observations with a depth, whose back-projections X averages (X = 0 when there is none).
SIM3OPT_TRACK_HD inline int32_t track_point(const PointArgs& A, const int32_t* seg, int32_t len, double X[3],
                                            int32_t& n_depths) {
  SIM3OPT_TRACK_NO_FMA
  double sx = 0.0, sy = 0.0, sz = 0.0;
  int32_t n = 0, prev = -1;
  bool conflict = false;
  for (int32_t i = 0; i < len; ++i) {
    const int32_t g = seg[i];
    const int32_t f = frame_of(A.kp_ptr, A.n_frames, g);
    conflict = conflict || f == prev;  // (ascending g: the observations of one frame are neighbours)
    prev = f;
    const int32_t key = A.dkey[g];
    if (key == NONE) continue;
    const double d = (key & 1) ? A.depth1[key >> 1] : A.depth0[key >> 1];
    const double u = (double)A.kp[2 * (size_t)g], v = (double)A.kp[2 * (size_t)g + 1];
    const double* st = A.states + 8 * (size_t)f;
    const Rot R = rot_of(st);
    const double a0 = d * ((u - A.cx) / A.focal) - st[4], a1 = d * ((v - A.cy) / A.focal) - st[5], a2 = d - st[6];
    sx += (R.r00 * a0 + R.r10 * a1 + R.r20 * a2) / st[7];
    sy += (R.r01 * a0 + R.r11 * a1 + R.r21 * a2) / st[7];
    sz += (R.r02 * a0 + R.r12 * a1 + R.r22 * a2) / st[7];
    ++n;
  }
  n_depths = n;
  X[0] = n ? sx / (double)n : 0.0;
  X[1] = n ? sy / (double)n : 0.0;
  X[2] = n ? sz / (double)n : 0.0;
  if (conflict) return TRACK_CONFLICT;
  if (!n) return TRACK_NO_DEPTH;
  bool behind = false, far = false;
  const double max2 = A.max_reproj_px * A.max_reproj_px;
  for (int32_t i = 0; i < len; ++i) {
    const int32_t g = seg[i];
    const double* st = A.states + 8 * (size_t)frame_of(A.kp_ptr, A.n_frames, g);
    const Rot R = rot_of(st);
    const double x = st[7] * (R.r00 * X[0] + R.r01 * X[1] + R.r02 * X[2]) + st[4];
    const double y = st[7] * (R.r10 * X[0] + R.r11 * X[1] + R.r12 * X[2]) + st[5];
    const double z = st[7] * (R.r20 * X[0] + R.r21 * X[1] + R.r22 * X[2]) + st[6];
    if (!(z > 0.0)) { behind = true; continue; }
    if (A.max_reproj_px > 0.0) {
      const double du = A.focal * x / z + A.cx - (double)A.kp[2 * (size_t)g];
      const double dv = A.focal * y / z + A.cy - (double)A.kp[2 * (size_t)g + 1];
      far = far || du * du + dv * dv > max2;
    }
  }
  return behind ? TRACK_BEHIND : far ? TRACK_REPROJECTION : TRACK_OK;
}

}  // namespace sim3opt_track
