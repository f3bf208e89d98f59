// frames_host_driver.cpp -- the host logic of the frame store (csrc/frames_host.hpp) as a stand-alone program: no GPU and
// no HIP runtime is linked.  Built with -fsanitize=address,undefined and run by tests/test_frames_host.py.
//   - every refusal of the argument checks as an exact string, in the words of the consumers' set_frames;
//   - the snapshot's holder counting against a stub allocator: the blocks go back exactly once, when the last holder --
//     the store or a consumer -- lets go, whatever the order; a refill leaves a consumer's snapshot alone;
//   - the compaction's offsets restated serially against a second, independent restatement, on segments on both sides
//     of the tile.
// Ends with "frames host ok".
#include <cassert>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <set>

#include "../../sim3opt_amd/csrc/frames_host.hpp"

using namespace sim3opt_fstore;

static std::set<void*> live;
static int freed = 0;
static void* stub_alloc(size_t bytes) {
  void* p = std::malloc(bytes ? bytes : 1);
  live.insert(p);
  return p;
}
static void stub_free(void* p) {
  if (!p) return;
  assert(live.erase(p) == 1);  // (never twice, never a stranger)
  std::free(p);
  ++freed;
}

static std::shared_ptr<Snapshot> stub_snapshot(const std::vector<int32_t>& kp_ptr) {
  auto s = std::make_shared<Snapshot>();
  s->free_block = stub_free;
  s->device = 0;
  s->kp_ptr = kp_ptr;
  s->d_kp_ptr = (int32_t*)stub_alloc(sizeof(int32_t) * kp_ptr.size());
  s->d_kp = (float*)stub_alloc(sizeof(float) * 2 * s->N());
  s->d_desc = (float*)stub_alloc(sizeof(float) * DESC * s->N());
  return s;
}

static void validation() {
  const int32_t ptr[4] = {0, 2, 2, 3}, not0[4] = {1, 2, 2, 3}, down[4] = {0, 2, 1, 3};
  std::vector<float> kp(6, 1.f), desc(64 * 3, 0.5f);
  assert(validate_frames(3, ptr, kp.data(), desc.data()).empty());
  assert(validate_frames(0, ptr, kp.data(), desc.data()) == "n_frames < 1");
  assert(validate_frames(3, nullptr, kp.data(), desc.data()) == "a NULL array");
  assert(validate_frames(3, ptr, nullptr, desc.data()) == "a NULL array");
  assert(validate_frames(3, ptr, kp.data(), nullptr) == "a NULL array");
  assert(validate_frames(3, not0, kp.data(), desc.data()) == "kp_ptr[0] must be 0");
  assert(validate_frames(3, down, kp.data(), desc.data()) == "kp_ptr is not monotone at frame 1");
  const int32_t big[2] = {0, INT32_MAX / 64 + 1};
  assert(validate_frames(1, big, kp.data(), desc.data()) == "too many keypoints");  // (before an array is read)
  kp[5] = std::numeric_limits<float>::infinity();
  assert(validate_frames(3, ptr, kp.data(), desc.data()) == "a non-finite keypoint");
  kp[5] = 1.f;
  desc[64 * 2 + 63] = std::nanf("");
  assert(validate_frames(3, ptr, kp.data(), desc.data()) == "a non-finite descriptor");
  assert(validate_frames(2, ptr, kp.data(), desc.data()).empty());  // (the rows past kp_ptr[n_frames] are not looked at)
  desc[64 * 2 + 63] = 0.5f;

  const int32_t state[3] = {2, 0, 3}, bad[3] = {2, 4, 3}, neg[3] = {-1, 2, 2};
  assert(validate_slots(3, ptr, state, kp.data(), desc.data()).empty());
  assert(validate_slots(0, ptr, state, kp.data(), desc.data()) == "n_images < 1");
  assert(validate_slots(3, ptr, nullptr, kp.data(), desc.data()) == "a NULL array");
  assert(validate_slots(3, down, state, kp.data(), desc.data()) == "cand_ptr is not monotone at frame 1");
  assert(validate_slots(3, ptr, bad, kp.data(), desc.data()) == "slot 1: no such state");
  assert(validate_slots(3, ptr, neg, kp.data(), desc.data()) == "slot 0: no such state");
  assert(validate_slots(1, big, state, kp.data(), desc.data()) == "too many slots");

  assert(check_total(0, 0).empty() && check_total((size_t)INT32_MAX / 64, 0).empty());
  assert(check_total((size_t)INT32_MAX / 64, 1) == "more keypoints than an int32 offset counts");
  assert(check_total((size_t)INT32_MAX / 64 - 5, 6) == "more keypoints than an int32 offset counts");
}

static void holders() {
  {  // the store alone
    SnapshotRef store = stub_snapshot({0, 3, 3, 7});
    assert(live.size() == 3 && store->n_frames() == 3 && store->N() == 7);
  }
  assert(live.empty() && freed == 3);
  {  // a consumer outlives the store
    SnapshotRef store = stub_snapshot({0, 5});
    SnapshotRef consumer = store;
    store.reset();
    assert(live.size() == 3 && consumer->N() == 5);
    consumer.reset();
    assert(live.empty() && freed == 6);
  }
  {  // the store outlives three consumers, let go in another order than they took it
    SnapshotRef store = stub_snapshot({0, 1, 2});
    SnapshotRef a = store, b = store, c = store;
    assert(store.use_count() == 4);
    b.reset(); a.reset();
    assert(live.size() == 3);
    c.reset();
    assert(live.size() == 3 && store.use_count() == 1);
    store.reset();
    assert(live.empty() && freed == 9);
  }
  {  // a refill: the consumer keeps the old blocks, unchanged; a second consumer sees the new ones
    SnapshotRef store = stub_snapshot({0, 4});
    SnapshotRef first = store;
    const float* old_desc = first->d_desc;
    store = stub_snapshot({0, 2, 9});
    SnapshotRef second = store;
    assert(live.size() == 6 && first->d_desc == old_desc && first->N() == 4 && second->N() == 9 && second->d_desc != old_desc);
    first.reset();
    assert(live.size() == 3 && freed == 12);
    store.reset();
    assert(live.size() == 3);
    second.reset();
    assert(live.empty() && freed == 15);
  }
  {  // an empty store (N = 0) owns blocks too, and gives them back; a snapshot without an allocator frees nothing
    SnapshotRef store = stub_snapshot({0, 0, 0});
    assert(store->N() == 0 && live.size() == 3);
    Snapshot none;
  }
  assert(live.empty() && freed == 18);
}

// a second restatement: an exclusive scan in tiles with a carry, as the kernels are organised
static void tiled_offsets(int32_t n_images, const int32_t* cand_ptr, const int32_t* state, int32_t base,
                          std::vector<int32_t>& kp_ptr, std::vector<int32_t>& src) {
  std::vector<int32_t> count((size_t)n_images, 0);
  std::vector<std::vector<int32_t>> tile_base((size_t)n_images);
  for (int32_t i = 0; i < n_images; ++i) {
    int32_t run = 0;
    for (int32_t first = cand_ptr[i]; first < cand_ptr[i + 1]; first += COMPACT_TILE) {
      tile_base[(size_t)i].push_back(run);
      for (int32_t s = first; s < first + COMPACT_TILE && s < cand_ptr[i + 1]; ++s) run += state[s] == KEPT;
    }
    count[(size_t)i] = run;
  }
  kp_ptr.assign(1, base);
  for (int32_t i = 0; i < n_images; ++i) kp_ptr.push_back(kp_ptr.back() + count[(size_t)i]);
  src.assign((size_t)(kp_ptr.back() - base), -1);
  for (int32_t i = 0; i < n_images; ++i)
    for (size_t t = 0; t < tile_base[(size_t)i].size(); ++t) {
      int32_t excl = 0;
      const int32_t first = cand_ptr[i] + (int32_t)t * COMPACT_TILE;
      for (int32_t s = first; s < first + COMPACT_TILE && s < cand_ptr[i + 1]; ++s)
        if (state[s] == KEPT) src[(size_t)(kp_ptr[(size_t)i] - base + tile_base[(size_t)i][t] + excl++)] = s;
    }
}

static void offsets() {
  const int T = COMPACT_TILE;
  const int32_t lengths[] = {0, 1, T - 1, T, T + 1, 2 * T + 1, 0, 3 * T, 0};
  const int32_t n = (int32_t)(sizeof(lengths) / sizeof(lengths[0]));
  std::vector<int32_t> cand_ptr(1, 0);
  for (int32_t l : lengths) cand_ptr.push_back(cand_ptr.back() + l);
  assert(max_tiles(n, cand_ptr.data()) == 3);
  const int32_t one[2] = {0, 0};
  assert(max_tiles(1, one) == 0);
  uint32_t rng = 12345u;
  for (int round = 0; round < 4; ++round) {
    std::vector<int32_t> state((size_t)cand_ptr.back());
    for (int32_t& s : state) {
      rng = rng * 1664525u + 1013904223u;
      const int pick = (int)((rng >> 16) % 3u);
      s = round == 1 ? 2 : round == 2 ? (pick == 0 ? 0 : 3) : (pick == 0 ? 0 : pick == 1 ? 2 : 3);
    }
    std::vector<int32_t> p0, s0, p1, s1;
    const int32_t base = round == 3 ? 777 : 0;
    compact_offsets(n, cand_ptr.data(), state.data(), base, p0, s0);
    tiled_offsets(n, cand_ptr.data(), state.data(), base, p1, s1);
    assert(p0 == p1 && s0 == s1 && p0.front() == base && (int32_t)s0.size() == p0.back() - base);
    if (round == 1) assert(p0.back() == cand_ptr.back());
    if (round == 2) assert(p0.back() == 0 && s0.empty());
    for (size_t r = 1; r < s0.size(); ++r) assert(s0[r - 1] < s0[r]);  // slot order
    for (int32_t i = 0; i < n; ++i)
      for (int32_t r = p0[(size_t)i] - base; r < p0[(size_t)i + 1] - base; ++r)
        assert(s0[(size_t)r] >= cand_ptr[(size_t)i] && s0[(size_t)r] < cand_ptr[(size_t)i + 1] && state[(size_t)s0[(size_t)r]] == KEPT);
  }
}

int main() {
  validation();
  holders();
  offsets();
  std::printf("frames host ok\n");
  return 0;
}
