"""The batched SURF-64 extraction on the device (sim3opt_amd/csrc/surf_batch.hip) against the definition of
include/sim3opt.h: bit for bit against the library's serial restatement of it (lib.SurfBatch.reference_image, the same
FP32 operations in the same orders), stage by stage through the read-outs, and against the independent numpy
restatement (tests/surf_ref.py) where the restatement is not exposed.  The images are those of tests/surf_cases.py."""
import numpy as np
import pytest

import surf_cases as SC
import surf_ref as R
from sim3opt_amd import lib as L

pytestmark = pytest.mark.gpu
FIELDS = L.SurfBatch.FIELDS


def solved(images, **options):
    b = L.SurfBatch(**options)
    b.set_images(images)
    n_ok = b.solve()
    return b, n_ok


def assert_image_equals(b, f, ref, what):
    """image f of a solved batch against a reference_image result: every byte"""
    ptr, kp, s = b.kp_ptr(), b.keypoints(), b.summary()
    lo, hi = ptr[f], ptr[f + 1]
    assert hi - lo == len(ref["size"]), (what, hi - lo, len(ref["size"]))
    for k in FIELDS:
        assert kp[k][lo:hi].tobytes() == ref[k].tobytes(), (what, k)
    assert [s["n_candidates"][f], s["n_interpolated"][f], s["n_dropped"][f]] == list(ref["counts"]), what
    assert s["status"][f] == (L.SURF_OK if hi > lo else L.SURF_NO_KEYPOINTS), what


@pytest.mark.parametrize("name", SC.SINGLE)
def test_every_output_byte_is_the_restatements(name):
    img = SC.image(name)
    b, n_ok = solved(img)
    ref = L.SurfBatch.reference_image(img)
    assert_image_equals(b, 0, ref, name)
    assert n_ok == (1 if len(ref["size"]) else 0)
    d = b.dims()
    assert (d["n_images"], d["width"], d["height"], d["total_keypoints"]) == (1, img.shape[1], img.shape[0], len(ref["size"]))
    assert (d["detect_tile"], d["rank_tile"], d["keypoint_lanes"]) == (32, 256, 64)


def test_layers_that_do_not_fit_give_no_keypoints_and_no_fault():
    """(d): 12 x 12 fits no layer of any octave; 40 x 36 fits octave 0 only; a constant image has nothing above the
    threshold: empty work at every later stage"""
    for name in ("tiny", "constant", "noise"):
        b, n_ok = solved(SC.image(name))
        assert n_ok == 0 and list(b.kp_ptr()) == [0, 0] and b.summary()["status"][0] == L.SURF_NO_KEYPOINTS
        assert b.keypoints()["desc"].shape == (0, 64)
        assert b.debug_candidates(0)["response"].shape == (0,)
    b, n_ok = solved(SC.image("small"))
    assert n_ok == 1 and np.all(b.keypoints()["octave"] == 0)


def test_the_ranking_crosses_its_tile_and_ties_go_by_scan_index():
    """(e): more candidates than two of the ranking's LDS tiles, so a rank accumulates over three stagings and the grid
    of the ranking has three workgroups for the image"""
    b, _ = solved(SC.image("textured_large"))
    kp, s = b.keypoints(), b.summary()
    assert s["n_candidates"][0] > 2 * b.dims()["rank_tile"] and s["n_interpolated"][0] > 2 * b.dims()["rank_tile"]
    assert s["n_candidates"][0] > s["n_interpolated"][0] == len(kp["size"])
    assert np.all(np.diff(kp["response"]) <= 0)
    # (f) six equal squares: equal responses to the bit, so the order within a response is the scan's: row, then column
    b, _ = solved(SC.image("squares"))
    kp = b.keypoints()
    same = kp["response"] == kp["response"][0]
    assert same.sum() >= len(SC.SQUARES)
    first = kp["kp"][:len(SC.SQUARES)]
    assert [tuple(p) for p in np.rint(first).astype(int)] == list(SC.SQUARES)


@pytest.mark.parametrize("per_pass", [1, 3, 64])
def test_an_images_result_does_not_depend_on_its_company(per_pass):
    """(h): seven images of one size, more than images_per_pass; every image as on its own.  One of them has more than
    two ranking tiles of candidates and the others a handful or none: in a pass that holds both, the ranking's later
    workgroups return at once for the small images."""
    batch = SC.mixed_batch()
    b, n_ok = solved(batch, images_per_pass=per_pass)
    refs = [L.SurfBatch.reference_image(im) for im in batch]
    counts = [int(r["counts"][0]) for r in refs]
    assert max(counts) > 2 * b.dims()["rank_tile"] and 0 < sorted(counts)[-2] < b.dims()["rank_tile"] and min(counts) == 0
    assert n_ok == sum(len(r["size"]) > 0 for r in refs)
    for f, (name, r) in enumerate(zip(SC.MIXED, refs)):
        assert_image_equals(b, f, r, (name, per_pass))
    assert b.kp_ptr()[-1] == sum(len(r["size"]) for r in refs)


@pytest.mark.parametrize("options", [dict(max_keypoints=50), dict(upright=1), dict(n_octaves=2, n_octave_layers=2),
                                     dict(n_octaves=6, n_octave_layers=6, hessian_threshold=100.0)])
def test_options(options):
    img = SC.image("textured_large")
    b, _ = solved(img, **options)
    ref = L.SurfBatch.reference_image(img, **options)
    assert_image_equals(b, 0, ref, options)
    kp = b.keypoints()
    if "max_keypoints" in options:
        full = L.SurfBatch.reference_image(img)
        assert len(kp["size"]) == 50 and kp["response"].tobytes() == full["response"][:50].tobytes()
    if "upright" in options:
        assert np.all(kp["angle"] == 270.0)


def test_read_outs_stage_by_stage():
    img = SC.image("odd")  # partial tiles in both axes, an octave-1 plane of odd size
    b, _ = solved(img)
    before = {k: v.copy() for k, v in b.keypoints().items()}
    assert np.array_equal(b.debug_integral(0), R.integral(img))
    for octave, layer in ((0, 0), (0, 2), (1, 1), (1, 4), (2, 0), (3, 4)):
        ref = L.SurfBatch.reference_image(img, responses=(octave, layer))
        det, tr = b.debug_responses(0, octave, layer)
        assert det.shape == (img.shape[0] >> octave, img.shape[1] >> octave)
        assert det.tobytes() == ref["det"].tobytes() and tr.tobytes() == ref["trace"].tobytes(), (octave, layer)
    c, rc = b.debug_candidates(0), L.SurfBatch.reference_image(img)["candidates"]
    assert len(rc["response"]) > 0
    for k in rc:
        assert c[k].tobytes() == rc[k].tobytes(), k
    # The orientation samples of every keypoint against the numpy restatement.  A box sum over its area is at most 255
    # / 2 per Haar half and exact as an integer, so vx, vy differ by the FP32 roundings of the weight, two products, a
    # sum and the Gaussian's product: 8 x 2^-24 of 127.5 x the largest Gaussian weight, absolute.  A sample's angle
    # differs by the polynomial's 0.01 degree where the sample is not near zero.  The windows are held to the
    # definition applied to the device's own samples (a membership can flip between the polynomial and arctan2): 114
    # FP32 roundings of the sums of magnitudes, squared.
    kp = b.keypoints()
    S = R.integral(img)
    bound = 8 * 2.0 ** -24 * 127.5 * R.gaussian(13, 2.5)[6] ** 2
    for k in range(len(kp["size"])):
        o = b.debug_orientation(k)
        ro = R.orientation(S, float(kp["kp"][k, 0]), float(kp["kp"][k, 1]), float(kp["size"][k]))
        valid = o["valid"].astype(bool)
        assert np.array_equal(valid, ro["valid"])
        assert np.abs(o["vx"] - ro["vx"]).max() <= bound and np.abs(o["vy"] - ro["vy"]).max() <= bound, k
        strong = valid & (np.hypot(ro["vx"], ro["vy"]) > 1e3 * bound)
        assert np.abs((o["angle"] - ro["angle"] + 180) % 360 - 180)[strong].max() < 0.02
        vx, vy = o["vx"].astype(float), o["vy"].astype(float)
        for c in range(72):
            d = np.abs(np.rint(o["angle"]) - 5 * c)
            m = valid & ((d < 30) | (d > 330))
            mag = vx[m].sum() ** 2 + vy[m].sum() ** 2
            tol = 4 * 114 * 2.0 ** -24 * (np.abs(vx[m]).sum() ** 2 + np.abs(vy[m]).sum() ** 2)
            assert abs(float(o["window"][c]) - mag) <= tol + 1e-30, (k, c)
        p = b.debug_patch(k)
        rp = R.patch_of(img, float(kp["kp"][k, 0]), float(kp["kp"][k, 1]), float(kp["angle"][k]), R.geometry(float(kp["size"][k]))[2])
        assert np.abs(p - rp).max() <= 1 and (p != rp).mean() <= 0.05, k
    after = b.keypoints()
    assert all(after[k].tobytes() == before[k].tobytes() for k in FIELDS)


def test_outputs_feed_the_next_stages_without_conversion():
    b, _ = solved(SC.mixed_batch())
    ptr, kp = b.kp_ptr(), b.keypoints()
    assert ptr.dtype == np.int32 and kp["desc"].dtype == np.float32 and kp["kp"].dtype == np.float32
    assert np.all(np.isfinite(kp["desc"])) and np.abs(np.linalg.norm(kp["desc"], axis=1) - 1).max() < 1e-5
    v = L.VocabularyTrainer(k=3, levels=2)
    v.set_frames(ptr, kp["desc"])
    assert v.train() > 1
    p = L.PlaceBatch()
    p.set_vocabulary(*v.vocabulary())
    p.set_frames(ptr, kp["desc"])
    assert p.solve() >= 0


def test_call_order_and_handles_reuse():
    b = L.SurfBatch()
    with pytest.raises(L.Sim3OptError) as e:
        b.solve()
    assert e.value.code == L.ERR_STATE
    b.set_images(SC.image("blobs"))
    with pytest.raises(L.Sim3OptError) as e:
        b.debug_integral(0)
    assert e.value.code == L.ERR_STATE
    assert b.solve() == 1
    first = b.keypoints()["desc"].copy()
    with pytest.raises(L.Sim3OptError):
        b.debug_integral(1)
    with pytest.raises(L.Sim3OptError):
        b.debug_patch(len(first))
    b.set_images(SC.image("odd"))  # another size on the same handle
    assert b.solve() == 1
    assert_image_equals(b, 0, L.SurfBatch.reference_image(SC.image("odd")), "odd after blobs")
    b.set_images(SC.image("blobs"))
    assert b.solve() == 1 and b.keypoints()["desc"].tobytes() == first.tobytes()


def test_every_block_of_a_pass_and_of_a_read_out_is_handed_back():
    """Between calls the handle keeps one block, the tables; close() gives that back too."""
    before = L.device_memory_in_use()[0]
    b, _ = solved(SC.mixed_batch(), images_per_pass=3)
    assert L.device_memory_in_use()[0] == before + 1
    b.debug_integral(1), b.debug_responses(1, 1, 2), b.debug_candidates(1), b.debug_orientation(5), b.debug_patch(5)
    assert L.device_memory_in_use()[0] == before + 1
    b.set_images(SC.image("large"))
    assert b.solve() == 1 and L.device_memory_in_use()[0] == before + 1
    b.close()
    assert L.device_memory_in_use()[0] == before


def test_on_poisoned_device_memory_with_guarded_tails():
    """The block cache's test mode: every floating-point block starts as NaN and ends in a canary.  The results are
    the restatement's all the same (nothing is read before it is written) and no tail is overwritten."""
    batch = SC.mixed_batch()
    refs = [L.SurfBatch.reference_image(im) for im in batch]
    L.debug_device_memory(True)
    try:
        b, _ = solved(batch, images_per_pass=3)
        for f, r in enumerate(refs):
            assert_image_equals(b, f, r, ("poisoned", f))
        det, tr = b.debug_responses(0, 0, 1)
        assert np.all(np.isfinite(det)) and np.all(np.isfinite(tr)) and np.all(np.isfinite(b.debug_patch(0)))
        o = b.debug_orientation(0)
        assert all(np.all(np.isfinite(o[k])) for k in ("vx", "vy", "angle", "window"))
        b.close()
        rep = L.debug_device_memory_report()
    finally:
        L.debug_device_memory(False)
    assert rep["filled"] > 0 and rep["checked"] > 0 and rep["overwritten"] == 0, rep
