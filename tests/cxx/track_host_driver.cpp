// track_host_driver.cpp -- the host logic of the loop-track stage (csrc/track_host.hpp, track_math.hpp) as a stand-alone
// program: no GPU and no HIP runtime is linked.  Built with -fsanitize=address,undefined and run by
// tests/test_track_host.py.
//   - every refusal of the argument checks as an exact string;
//   - frame_of on frames that own nothing, depth_present on every kind of absent depth;
//   - the serial restatement (union-find) against a second, independent one (label propagation to a fixed point, then
//     sorting) on random ragged batches with masks, repeated matches and absent depths: tracks, their order, their
//     observations, the track of every match; and the statuses and points of small planted tracks.
// Ends with "track host ok".
#include <cassert>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <map>
#include <random>

#include "../../sim3opt_amd/csrc/track_host.hpp"

using namespace sim3opt_track;

static const double NaN = std::numeric_limits<double>::quiet_NaN(), Inf = std::numeric_limits<double>::infinity();

static void validation() {
  const int32_t ptr[4] = {0, 2, 2, 5}, not0[4] = {1, 2, 2, 5}, down[4] = {0, 2, 1, 5};
  std::vector<float> kp(10, 1.f);
  assert(validate_frames(3, ptr, kp.data()).empty());
  assert(validate_frames(0, ptr, kp.data()) == "n_frames < 1");
  assert(validate_frames(3, nullptr, kp.data()) == "a NULL array");
  assert(validate_frames(3, ptr, nullptr) == "a NULL array");
  assert(validate_frames(3, not0, kp.data()) == "kp_ptr[0] must be 0");
  assert(validate_frames(3, down, kp.data()) == "kp_ptr is not monotone at frame 1");
  kp[9] = std::numeric_limits<float>::infinity();
  assert(validate_frames(3, ptr, kp.data()) == "a non-finite keypoint");

  const int32_t pairs[4] = {0, 2, 2, 0}, mp[3] = {0, 2, 3}, q[3] = {0, 1, 2}, t[3] = {2, 0, 1};
  const uint8_t mask[3] = {1, 0, 1};
  std::vector<int32_t> ga, gb;
  assert(validate_matches(3, ptr, 2, pairs, mp, q, t, mask, ga, gb).empty());
  assert((ga == std::vector<int32_t>{0, -1, 4}) && (gb == std::vector<int32_t>{4, 2, 1}));
  assert(validate_matches(3, ptr, 2, pairs, mp, q, t, nullptr, ga, gb).empty() && ga[1] == 1);
  assert(validate_matches(3, ptr, 0, pairs, mp, q, t, mask, ga, gb) == "n_pairs < 1");
  assert(validate_matches(3, ptr, 2, nullptr, mp, q, t, mask, ga, gb) == "a NULL array");
  assert(validate_matches(3, ptr, 2, pairs, mp, q, nullptr, mask, ga, gb) == "a NULL array");
  const int32_t mp1[3] = {1, 2, 3}, mpd[3] = {0, 2, 1};
  assert(validate_matches(3, ptr, 2, pairs, mp1, q, t, mask, ga, gb) == "match_ptr[0] must be 0");
  assert(validate_matches(3, ptr, 2, pairs, mpd, q, t, mask, ga, gb) == "match_ptr is not monotone at pair 1");
  const int32_t pbad[4] = {0, 2, 3, 0}, pneg[4] = {0, -1, 2, 0};
  assert(validate_matches(3, ptr, 2, pbad, mp, q, t, mask, ga, gb) == "pair 1: no such frame");
  assert(validate_matches(3, ptr, 2, pneg, mp, q, t, mask, ga, gb) == "pair 0: no such frame");
  const int32_t qbad[3] = {0, 2, 2}, tneg[3] = {2, 0, -1}, pempty[4] = {0, 1, 2, 0};
  assert(validate_matches(3, ptr, 2, pairs, mp, qbad, t, mask, ga, gb) == "match 1 of pair 0: an index outside its frame");
  assert(validate_matches(3, ptr, 2, pairs, mp, q, tneg, mask, ga, gb) == "match 2 of pair 1: an index outside its frame");
  assert(validate_matches(3, ptr, 2, pempty, mp, q, t, mask, ga, gb) == "match 0 of pair 0: an index outside its frame");
  const int32_t none[3] = {0, 0, 0};  // no match at all is no error
  assert(validate_matches(3, ptr, 2, pairs, none, q, t, mask, ga, gb).empty() && ga.empty());

  std::vector<double> st(24, 0.0);
  for (int f = 0; f < 3; ++f) st[8 * f + 3] = st[8 * f + 7] = 1.0;
  assert(validate_cameras(3, 3, st.data(), 700.0, 600.0, 180.0).empty());
  assert(validate_cameras(3, 3, nullptr, 700.0, 600.0, 180.0) == "a NULL array");
  assert(validate_cameras(2, 3, st.data(), 700.0, 600.0, 180.0) == "states are of 2 frames, the handle holds 3");
  assert(validate_cameras(3, 3, st.data(), 0.0, 600.0, 180.0) == "focal <= 0");
  assert(validate_cameras(3, 3, st.data(), 700.0, NaN, 180.0) == "non-finite intrinsics");
  st[15] = 0.0;
  assert(validate_cameras(3, 3, st.data(), 700.0, 600.0, 180.0) == "frame 1: s <= 0");
  st[15] = 1.0; st[20] = Inf;
  assert(validate_cameras(3, 3, st.data(), 700.0, 600.0, 180.0) == "a non-finite state");
}

static void small_things() {
  const int32_t ptr[6] = {0, 0, 3, 3, 3, 7};  // frames 0, 2 and 3 own nothing
  const int32_t want[7] = {1, 1, 1, 4, 4, 4, 4};
  for (int32_t g = 0; g < 7; ++g) assert(frame_of(ptr, 5, g) == want[g]);
  const int32_t one[2] = {0, 4};
  for (int32_t g = 0; g < 4; ++g) assert(frame_of(one, 1, g) == 0);
  assert(depth_present(1e-300) && depth_present(1.7e308));
  assert(!depth_present(0.0) && !depth_present(-1.0) && !depth_present(NaN) && !depth_present(Inf) && !depth_present(-Inf));
}

// the components by label propagation over the matches until nothing changes: no union-find, no roots
static void second_restatement(size_t N, const std::vector<int32_t>& ga, const std::vector<int32_t>& gb, Tracks& out) {
  std::vector<int32_t> label(N);
  for (size_t g = 0; g < N; ++g) label[g] = (int32_t)g;
  for (bool changed = true; changed;) {
    changed = false;
    for (size_t m = 0; m < ga.size(); ++m) {
      if (ga[m] < 0) continue;
      const int32_t lo = std::min(label[ga[m]], label[gb[m]]);
      if (label[ga[m]] != lo || label[gb[m]] != lo) { label[ga[m]] = label[gb[m]] = lo; changed = true; }
    }
  }
  std::map<int32_t, int32_t> first;  // label -> smallest kept match
  for (size_t m = 0; m < ga.size(); ++m)
    if (ga[m] >= 0) first.emplace(label[ga[m]], (int32_t)m);
  std::vector<std::pair<int32_t, int32_t>> order;  // (first match, label)
  for (const auto& kv : first) order.push_back({kv.second, kv.first});
  std::sort(order.begin(), order.end());
  out = Tracks{};
  out.track_ptr.push_back(0);
  std::map<int32_t, int32_t> number;
  for (const auto& o : order) {
    number[o.second] = (int32_t)out.first_match.size();
    out.first_match.push_back(o.first);
    for (size_t g = 0; g < N; ++g)
      if (label[g] == o.second && first.count(label[g])) out.obs_g.push_back((int32_t)g);
    out.track_ptr.push_back((int32_t)out.obs_g.size());
  }
  for (size_t m = 0; m < ga.size(); ++m) out.match_track.push_back(ga[m] < 0 ? -1 : number[label[ga[m]]]);
}

static void random_batches() {
  std::mt19937 rng(7);
  for (int trial = 0; trial < 60; ++trial) {
    const int32_t nf = 1 + (int32_t)(rng() % 9);
    std::vector<int32_t> ptr(1, 0);
    for (int32_t f = 0; f < nf; ++f) ptr.push_back(ptr.back() + (int32_t)(rng() % 7));  // (some own nothing)
    const size_t N = (size_t)ptr.back();
    std::vector<float> kp(2 * std::max<size_t>(N, 1));
    for (auto& v : kp) v = (float)(rng() % 1200);
    const int32_t np = 1 + (int32_t)(rng() % 12);
    std::vector<int32_t> pairs, mp(1, 0), q, t;
    std::vector<uint8_t> mask;
    std::vector<double> d0, d1;
    const double absent[4] = {NaN, 0.0, -2.0, Inf};
    for (int32_t p = 0; p < np; ++p) {
      const int32_t f0 = (int32_t)(rng() % nf), f1 = (int32_t)(rng() % nf);
      pairs.push_back(f0); pairs.push_back(f1);
      const int32_t n0 = ptr[f0 + 1] - ptr[f0], n1 = ptr[f1 + 1] - ptr[f1];
      const int32_t nm = n0 && n1 ? (int32_t)(rng() % 6) : 0;
      for (int32_t k = 0; k < nm; ++k) {
        q.push_back((int32_t)(rng() % n0)); t.push_back((int32_t)(rng() % n1));
        mask.push_back(rng() % 4 != 0);
        d0.push_back(rng() % 3 ? 1.0 + (double)(rng() % 40) : absent[rng() % 4]);
        d1.push_back(rng() % 3 ? 1.0 + (double)(rng() % 40) : absent[rng() % 4]);
      }
      mp.push_back((int32_t)q.size());
    }
    q.push_back(0); t.push_back(0);  // (never read: the arrays are not NULL when there is no match)
    std::vector<int32_t> ga, gb;
    const bool with_mask = trial % 3 != 0;
    assert(validate_matches(nf, ptr.data(), np, pairs.data(), mp.data(), q.data(), t.data(), with_mask ? mask.data() : nullptr,
                            ga, gb).empty());
    std::vector<double> st(8 * (size_t)nf, 0.0);
    for (int32_t f = 0; f < nf; ++f) { st[8 * f + 3] = 1.0; st[8 * f + 7] = 0.5 + 0.25 * (double)(rng() % 5); st[8 * f + 6] = -1.0; }
    Tracks a, b;
    reference_tracks(nf, ptr.data(), kp.data(), ga, gb, trial % 2 ? d0.data() : nullptr, d1.data(), st.data(), 700.0, 600.0,
                     180.0, trial % 5 ? 0.0 : 300.0, a);
    second_restatement(N, ga, gb, b);
    assert(a.track_ptr == b.track_ptr && a.obs_g == b.obs_g && a.first_match == b.first_match && a.match_track == b.match_track);
    assert(a.points.size() == 3 * a.status.size() && a.n_depths.size() == a.status.size());
    for (int32_t k = 0; k < a.n_tracks(); ++k) {
      assert(a.status[k] >= TRACK_OK && a.status[k] <= TRACK_REPROJECTION);
      assert((a.n_depths[k] == 0) == (a.status[k] == TRACK_NO_DEPTH) || a.status[k] == TRACK_CONFLICT);
      for (int i = 0; i < 3; ++i) assert(std::isfinite(a.points[3 * (size_t)k + i]));
    }
    std::vector<int32_t> fr(a.obs_g.size() + 1), ky(a.obs_g.size() + 1);
    split_observations(nf, ptr.data(), a.obs_g.data(), a.obs_g.size(), fr.data(), ky.data());
    for (size_t i = 0; i < a.obs_g.size(); ++i) assert(ptr[fr[i]] + ky[i] == a.obs_g[i] && ky[i] < ptr[fr[i] + 1] - ptr[fr[i]]);
  }
}

static void planted_tracks() {
  // two frames, two keypoints each: track 0 is exact by construction, track 1 has no depth
  const int32_t ptr[3] = {0, 2, 4};
  const float kp[8] = {700.f, 200.f, 10.f, 20.f, 630.f, 200.f, 30.f, 40.f};  // f = 700, c = (600, 180)
  const std::vector<int32_t> ga = {0, 1}, gb = {2, 3};
  const double d0[2] = {7.0, NaN}, d1[2] = {NaN, -1.0};
  double st[16] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, -0.7, 0, 0, 1};  // frame 1 sits 0.7 to the right
  Tracks r;
  reference_tracks(2, ptr, kp, ga, gb, d0, d1, st, 700.0, 600.0, 180.0, 0.5, r);
  assert((r.status == std::vector<int32_t>{TRACK_OK, TRACK_NO_DEPTH}) && (r.n_depths == std::vector<int32_t>{1, 0}));
  // 7 * (100 / 700, 20 / 700, 1)
  assert(std::fabs(r.points[0] - 1.0) < 1e-15 && std::fabs(r.points[1] - 0.2) < 1e-15 && r.points[2] == 7.0 && r.points[3] == 0.0);
  st[12] = -0.8;  // the projection into frame 1 moves by 10 px: the gate of 0.5 px fails, one of 11 holds
  reference_tracks(2, ptr, kp, ga, gb, d0, d1, st, 700.0, 600.0, 180.0, 0.5, r);
  assert(r.status[0] == TRACK_REPROJECTION);
  reference_tracks(2, ptr, kp, ga, gb, d0, d1, st, 700.0, 600.0, 180.0, 11.0, r);
  assert(r.status[0] == TRACK_OK);
  st[14] = -8.0;  // frame 1 eight ahead of the point
  reference_tracks(2, ptr, kp, ga, gb, d0, d1, st, 700.0, 600.0, 180.0, 0.0, r);
  assert(r.status[0] == TRACK_BEHIND);
  const std::vector<int32_t> ca = {0, 0}, cb = {2, 3};  // keypoint 0 of frame 0 matched twice into frame 1
  reference_tracks(2, ptr, kp, ca, cb, d0, d1, st, 700.0, 600.0, 180.0, 0.0, r);
  assert(r.n_tracks() == 1 && r.status[0] == TRACK_CONFLICT && (r.obs_g == std::vector<int32_t>{0, 2, 3}));
}

int main() {
  validation();
  small_things();
  random_batches();
  planted_tracks();
  std::printf("track host ok\n");
  return 0;
}
