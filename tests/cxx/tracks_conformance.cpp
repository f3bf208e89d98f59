// tracks_conformance.cpp -- conformance program of include/sim3opt_tracks.hpp (sim3opt_shim::LoopTrackBatch).
//   tracks_conformance host        the helper's and the C-ABI's refusals; needs no GPU
//   tracks_conformance run FILE    the batch of FILE through add_pair / solve on the device against
//                                  sim3opt_track_reference on the host, byte for byte, and append_to behind a small map;
//                                  exit 3 with the library's message when there is no device
// FILE: "n_frames focal cx cy max_reproj_px", n_frames lines "n_keypoints qx qy qz qw tx ty tz s", the pixels "u v" of
// every keypoint, "n_pairs", and per pair "frame0 frame1 n_matches" followed by n_matches lines
// "query train depth0 depth1 mask" (a depth of 0: none).
#include <cstdio>
#include <cstring>
#include <vector>

#include "sim3opt_tracks.hpp"

static int g_checks = 0, g_failed = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    ++g_checks;                                                            \
    if (!(cond)) { ++g_failed; std::printf("FAILED line %d: %s\n", __LINE__, #cond); } \
  } while (0)

using sim3opt_shim::LoopMatch;
using sim3opt_shim::LoopTrackBatch;

static int host() {
  LoopTrackBatch t;
  CHECK(t.solve() == SIM3OPT_ERR_STATE && t.last_error() == "solve: no frames set");
  const int32_t ptr[3] = {0, 2, 3}, bad_ptr[3] = {0, 2, 1};
  const float kp[6] = {1, 2, 3, 4, 5, 6};
  CHECK(t.set_frames(2, bad_ptr, kp) == SIM3OPT_ERR_ARG && t.last_error() == "track_batch_set_frames: kp_ptr is not monotone at frame 1");
  CHECK(t.set_frames(0, ptr, kp) == SIM3OPT_ERR_ARG);
  CHECK(t.set_frames(2, ptr, kp) == SIM3OPT_OK);
  CHECK(t.solve() == SIM3OPT_ERR_STATE && t.last_error() == "solve: no pair added");
  CHECK(t.add_pair(0, 1, {LoopMatch(0, 0, 2.0, 2.0), LoopMatch(5, 0)}) == 0 && t.n_pairs() == 1);
  CHECK(t.solve() == SIM3OPT_ERR_STATE && t.last_error() == "solve: no cameras set");
  std::vector<double> st = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1};
  t.set_cameras(st, 700, 600, 180);
  CHECK(t.solve() == SIM3OPT_ERR_ARG && t.last_error() == "track_batch_set_matches: match 1 of pair 0: an index outside its frame");
  t.clear_pairs();
  CHECK(t.add_pair(0, 2, {LoopMatch(0, 0)}) == 0);
  CHECK(t.solve() == SIM3OPT_ERR_ARG && t.last_error() == "track_batch_set_matches: pair 0: no such frame");
  t.clear_pairs();
  t.add_pair(0, 1, {LoopMatch(0, 0, 2.0, 2.0)});
  st[7] = 0.0;
  t.set_cameras(st, 700, 600, 180);
  CHECK(t.solve() == SIM3OPT_ERR_ARG && t.last_error() == "track_batch_set_cameras: frame 0: s <= 0");
  st[7] = 1.0;
  t.set_cameras(st, 0.0, 600, 180);
  CHECK(t.solve() == SIM3OPT_ERR_ARG && t.last_error() == "track_batch_set_cameras: focal <= 0");
  t.options().max_rounds = 0;
  CHECK(t.solve() == SIM3OPT_ERR_ARG && t.last_error() == "track_batch_set_options: max_rounds < 1");
  std::vector<int32_t> a, b, c, d;
  CHECK(t.tracks(a, b, c, d) == SIM3OPT_ERR_STATE && t.last_error() == "track_batch_get_tracks: no solve yet");
  std::vector<double> cams(14, 0.0), pts, uv;
  CHECK(t.append_to(cams, pts, a, b, uv) == SIM3OPT_ERR_STATE && pts.empty());
  cams.resize(7);
  CHECK(t.append_to(cams, pts, a, b, uv) == SIM3OPT_ERR_ARG && t.last_error() == "append_to: one camera per frame");
  sim3opt_shim::FrameStore store;
  CHECK(t.set_frames(store) == SIM3OPT_ERR_ARG);  // (max_rounds = 0 is still in the options)
  t.options().max_rounds = 64;
  CHECK(t.set_frames(store) == SIM3OPT_ERR_STATE && t.last_error() == "track_batch_set_frames_from: the store is not filled");
  CHECK(sim3opt_track_batch_solve(nullptr) == SIM3OPT_ERR_ARG && sim3opt_track_batch_set_frames(nullptr, 2, ptr, kp) == SIM3OPT_ERR_ARG);
  CHECK(std::strcmp(sim3opt_track_batch_last_error(nullptr), "null batch") == 0);
  std::printf("tracks_conformance host: %d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}

static int run(const char* path) {
  std::FILE* f = std::fopen(path, "r");
  if (!f) { std::fprintf(stderr, "cannot read %s\n", path); return 2; }
  int nf = 0, np = 0;
  double focal, cx, cy, max_px;
  if (std::fscanf(f, "%d %lf %lf %lf %lf", &nf, &focal, &cx, &cy, &max_px) != 5 || nf < 1) return 2;
  std::vector<int32_t> kp_ptr(1, 0);
  std::vector<double> states(8 * (size_t)nf);
  for (int i = 0; i < nf; ++i) {
    int n = 0;
    if (std::fscanf(f, "%d", &n) != 1) return 2;
    kp_ptr.push_back(kp_ptr.back() + n);
    for (int k = 0; k < 8; ++k)
      if (std::fscanf(f, "%lf", &states[8 * (size_t)i + k]) != 1) return 2;
  }
  std::vector<float> kp(2 * (size_t)kp_ptr.back() + 1);
  for (int i = 0; i < 2 * kp_ptr.back(); ++i)
    if (std::fscanf(f, "%f", &kp[i]) != 1) return 2;
  if (std::fscanf(f, "%d", &np) != 1) return 2;
  LoopTrackBatch t;
  t.options().max_reproj_px = max_px;
  CHECK(t.set_frames(nf, kp_ptr.data(), kp.data()) == SIM3OPT_OK);
  std::vector<int32_t> pairs, match_ptr(1, 0), q, tr;
  std::vector<uint8_t> mask;
  std::vector<double> d0, d1;
  for (int p = 0; p < np; ++p) {
    int f0, f1, nm;
    if (std::fscanf(f, "%d %d %d", &f0, &f1, &nm) != 3) return 2;
    std::vector<LoopMatch> ms;
    std::vector<uint8_t> mk;
    for (int k = 0; k < nm; ++k) {
      LoopMatch m;
      int keep;
      if (std::fscanf(f, "%d %d %lf %lf %d", &m.query, &m.train, &m.depth0, &m.depth1, &keep) != 5) return 2;
      ms.push_back(m); mk.push_back((uint8_t)keep);
      q.push_back(m.query); tr.push_back(m.train); d0.push_back(m.depth0); d1.push_back(m.depth1); mask.push_back((uint8_t)keep);
    }
    CHECK(t.add_pair(f0, f1, ms, &mk) == p);
    pairs.push_back(f0); pairs.push_back(f1); match_ptr.push_back((int32_t)q.size());
  }
  std::fclose(f);
  t.set_cameras(states, focal, cx, cy);
  const int kept = t.solve();
  if (kept == SIM3OPT_ERR_NO_DEVICE) { std::fprintf(stderr, "%s\n", t.last_error().c_str()); return 3; }
  CHECK(kept >= 0);
  if (kept < 0) { std::printf("solve: %s\n", t.last_error().c_str()); return 1; }
  // the host restatement of the same batch
  const size_t M = q.size();
  q.push_back(0); tr.push_back(0);
  int32_t nt = 0, no = 0;
  std::vector<int32_t> rp(M + 1), rf(2 * M + 1), rk(2 * M + 1), rs(M + 1), rfirst(M + 1), rmt(M + 1), rnd(M + 1);
  std::vector<double> rpts(3 * M + 3);
  CHECK(sim3opt_track_reference(nf, kp_ptr.data(), kp.data(), np, pairs.data(), match_ptr.data(), q.data(), tr.data(), mask.data(),
                                d0.data(), d1.data(), states.data(), focal, cx, cy, max_px, &nt, &no, rp.data(), rf.data(),
                                rk.data(), rs.data(), rfirst.data(), rmt.data(), rpts.data(), rnd.data()) == SIM3OPT_OK);
  std::vector<int32_t> tp, of, ok, st;
  CHECK(t.tracks(tp, of, ok, st) == SIM3OPT_OK);
  CHECK(t.n_tracks() == nt && (int)of.size() == no && t.rounds() >= 1);
  rp.resize((size_t)nt + 1); rs.resize((size_t)nt); rf.resize((size_t)no); rk.resize((size_t)no);
  CHECK(tp == rp && of == rf && ok == rk && st == rs);
  std::vector<double> pts((size_t)3 * nt);
  CHECK(sim3opt_track_batch_get_points(t.handle(), pts.data(), nullptr) == SIM3OPT_OK);
  CHECK(nt == 0 || std::memcmp(pts.data(), rpts.data(), sizeof(double) * 3 * (size_t)nt) == 0);
  // behind a map of two points and one observation
  std::vector<double> cams(7 * (size_t)nf, 0.0), points = {1, 2, 3, 4, 5, 6}, uv = {10, 20};
  std::vector<int32_t> oc = {0}, op = {1};
  CHECK(t.append_to(cams, points, oc, op, uv) == SIM3OPT_OK);
  int want_kept = 0, want_obs = 0;
  for (int k = 0; k < nt; ++k)
    if (rs[k] == SIM3OPT_TRACK_OK) { ++want_kept; want_obs += rp[k + 1] - rp[k]; }
  CHECK(kept == want_kept && (int)points.size() == 3 * (2 + want_kept) && (int)oc.size() == 1 + want_obs);
  CHECK(op.size() == oc.size() && uv.size() == 2 * oc.size() && points[0] == 1 && oc[0] == 0 && op[0] == 1 && uv[1] == 20);
  size_t row = 1;
  int rank = 0;
  for (int k = 0; k < nt; ++k) {
    if (rs[k] != SIM3OPT_TRACK_OK) continue;
    CHECK(std::memcmp(&points[3 * (size_t)(2 + rank)], &rpts[3 * (size_t)k], 3 * sizeof(double)) == 0);
    for (int i = rp[k]; i < rp[k + 1]; ++i, ++row) {
      const int g = kp_ptr[rf[i]] + rk[i];
      CHECK(oc[row] == rf[i] && op[row] == 2 + rank && uv[2 * row] == (double)kp[2 * g] && uv[2 * row + 1] == (double)kp[2 * g + 1]);
    }
    ++rank;
  }
  std::printf("tracks_conformance run: %d pairs, %d matches, %d tracks, %d kept, %d rounds, %d checks, %d failed\n", np, (int)M, nt,
              kept, t.rounds(), g_checks, g_failed);
  return g_failed ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc >= 2 && std::strcmp(argv[1], "host") == 0) return host();
  if (argc >= 3 && std::strcmp(argv[1], "run") == 0) return run(argv[2]);
  std::fprintf(stderr, "usage: tracks_conformance host | run FILE\n");
  return 2;
}
