"""Times the detector chain as a whole, from images to matches, two ways in one process: through host arrays (solve,
get_keypoints, set_frames of every consumer: the entries that exist without the frame store; the baseline) and through
one FrameStore (solve_into, set_frames_from).  Inputs: the 64 synthetic 1241 x 376 images of scripts/surf_batch.py, then
k = 10, L = 4 training, place recognition, and matching on the pairs found.  Host wall clock, warm, median of 11; per
stage (extract, hand-over, train, detect, match), the largest sim3opt_device_memory_in_use seen after a stage, and each consumer's time on
frames that are already resident (a second train / solve on the same handle), whose kernels and operands are the same
in both legs.  Prints one JSON line (profiles/frame_chain.json).  No target is set.

    python scripts/frame_chain.py
"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("SIM3OPT_PRELOAD_TORCH", "1")
import numpy as np
from sim3opt_amd import lib as L
import surf_cases as SC

REPS = 11
W, H, N_IMG = 1241, 376, 64
rng = np.random.default_rng(0)
sm = SC.smooth(rng.normal(0, 1, (H + 64, W + 64)), 2.5)
sm = (sm - sm.min()) / (sm.max() - sm.min())
big = np.clip(np.rint(255 * sm), 0, 255).astype(np.uint8)
imgs = np.stack([big[k:k + H, k:k + W] for k in range(N_IMG)])
obs_rng = np.random.default_rng(1)
obs_ptr = (300 * np.arange(N_IMG + 1)).astype(np.int32)
obs_uv = obs_rng.uniform([0, 0], [W, H], (obs_ptr[-1], 2)).astype(np.float32)
obs_depth = obs_rng.uniform(5, 50, obs_ptr[-1]).astype(np.float32)
VOC = dict(k=10, levels=4, seed=0)


class Clock:
    def __init__(self):
        self.ms, self.peak = {}, 0

    def __call__(self, name, fn):
        t0 = time.perf_counter()
        out = fn()
        self.ms[name] = 1e3 * (time.perf_counter() - t0)
        self.peak = max(self.peak, L.device_memory_in_use()[1])
        return out


def fallback_pairs(pairs):
    return pairs if len(pairs) else np.array([(i, i - 8) for i in range(8, N_IMG)], dtype=np.int32)


def leg(from_store, surf):
    """One repetition: fresh consumers (and a fresh store), the extractor reused with its images set."""
    c = Clock()
    voc, place, match = L.VocabularyTrainer(**VOC), L.PlaceBatch(), L.MatchBatch()
    store = L.FrameStore() if from_store else None
    if from_store:
        c("extract", lambda: surf.solve_into(store))

        def hand_over():
            voc.set_frames_from(store); place.set_frames_from(store)
            match.set_frames_from(store, obs_ptr, obs_uv, obs_depth, image_width=W, image_height=H)
    else:
        ptr, kp = c("extract", lambda: (surf.solve(), surf.kp_ptr(), surf.keypoints())[1:])

        def hand_over():
            voc.set_frames(ptr, kp["desc"]); place.set_frames(ptr, kp["desc"])
            match.set_frames(ptr, obs_ptr, kp["kp"], kp["desc"], obs_uv, obs_depth, image_width=W, image_height=H)
    c("hand_over", hand_over)
    c("train", voc.train)
    tree = voc.vocabulary()
    c("detect", lambda: (place.set_vocabulary(*tree), place.solve()))
    pairs = fallback_pairs(place.pairs())
    c("match", lambda: (match.set_pairs(pairs), match.solve()))
    # the frames are resident now: the same kernels on the same operands in both legs
    c("train_resident", voc.train)
    c("detect_resident", place.solve)
    c("match_resident", match.solve)
    c.ms["chain"] = sum(c.ms[k] for k in ("extract", "hand_over", "train", "detect", "match"))
    check = dict(keypoints=int(surf.kp_ptr()[-1]), nodes=len(tree[0]), pairs=int(len(pairs)), matches=int(match.match_ptr()[-1]),
                 tree=tree, match_ptr=match.match_ptr(), matches_all=match.matches())
    for h in (voc, place, match) + ((store,) if store else ()):
        h.close()
    return c, check


def run(from_store):
    surf = L.SurfBatch(images_per_pass=64)
    surf.set_images(imgs)
    base = L.device_memory_in_use()[1]
    leg(from_store, surf)  # warm
    runs = [leg(from_store, surf) for _ in range(REPS)]
    out = {}
    for name in runs[0][0].ms:
        v = [c.ms[name] for c, _ in runs]
        out[name + "_ms"] = dict(median=float(np.median(v)), min=min(v), max=max(v))
    out["peak_device_bytes"] = max(c.peak for c, _ in runs) - base
    check = runs[-1][1]
    out.update({k: check[k] for k in ("keypoints", "nodes", "pairs", "matches")})
    surf.close()
    return out, check


def same(a, b):
    if isinstance(a, dict):
        return sorted(a) == sorted(b) and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


host, check_host = run(False)
store, check_store = run(True)
out = dict(reps=REPS, images=[N_IMG, W, H], vocabulary=VOC, host_array_leg=host, store_leg=store,
           desc_bytes=256 * host["keypoints"],
           legs_equal=bool(same({k: check_host[k] for k in ("tree", "match_ptr", "matches_all")},
                                {k: check_store[k] for k in ("tree", "match_ptr", "matches_all")})))
print(json.dumps(out))
