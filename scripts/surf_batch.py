"""Times the batched SURF-64 extraction (lib.SurfBatch) at KITTI-00's image size: 64 synthetic textured images of
1241 x 376, images_per_pass 64 and 16, host wall clock, warm, median of 5; and the serial host restatement of one image.
Prints one JSON line (profiles/surf_batch.json).  No target is set for this stage.

    python scripts/surf_batch.py
"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("SIM3OPT_PRELOAD_TORCH", "1")
import numpy as np
from sim3opt_amd import lib as L
rng = np.random.default_rng(0)
base = rng.normal(0, 1, (376 + 64, 1241 + 64))
import surf_cases as SC
sm = SC.smooth(base, 2.5)
sm = (sm - sm.min()) / (sm.max() - sm.min())
big = np.clip(np.rint(255 * sm), 0, 255).astype(np.uint8)
imgs = np.stack([big[k:k + 376, k:k + 1241] for k in range(64)])
out = {}
for per in (64, 16):
    b = L.SurfBatch(images_per_pass=per)
    t0 = time.perf_counter(); b.set_images(imgs); t_set = time.perf_counter() - t0
    b.solve()
    ts = []
    for _ in range(5):
        t0 = time.perf_counter(); n = b.solve(); ts.append(time.perf_counter() - t0)
    s = b.summary()
    out[f"per_pass_{per}"] = dict(set_images_ms=1e3 * t_set, solve_ms_median=1e3 * float(np.median(ts)), solve_ms_all=[1e3 * t for t in ts],
                                  images_ok=n, keypoints=int(b.kp_ptr()[-1]), candidates=int(s["n_candidates"].sum()),
                                  interpolated=int(s["n_interpolated"].sum()), dropped=int(s["n_dropped"].sum()))
t0 = time.perf_counter(); r = L.SurfBatch.reference_image(imgs[0]); out["host_restatement_one_image_ms"] = 1e3 * (time.perf_counter() - t0)
kp = b.keypoints(); p = b.kp_ptr()
out["image0_equals_restatement"] = bool(kp["desc"][p[0]:p[1]].tobytes() == r["desc"].tobytes() and kp["kp"][p[0]:p[1]].tobytes() == r["kp"].tobytes())
print(json.dumps(out))
