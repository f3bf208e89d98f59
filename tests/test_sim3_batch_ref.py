"""The batched Sim(3) stage without a GPU: the conditions the GPU comparisons rest on, the restatement
(tests/sim3_batch_ref.py) against the planted truth and against seeded defects, the host build of
sim3opt_amd/csrc/sim3_batch_math.hpp (tests/cxx/sim3_batch_math_driver.cpp, a stand-alone program under the address and
undefined-behaviour sanitizers) against the restatement, and every argument check of the C entries.

PARITY UNPINNED: the reference has no such step, so there is no oracle; what stands in is the independent restatement
(Umeyama through numpy's SVD, long-double sums, Jacobians by central differences) and the planted C*.

Limits.  Measured from the host build against the restatement over sim3_batch_cases.RUNS and the status-4 run, never
against the device; each is 32 times the worst deviation, floored at 1e-8:
  MODEL_LIMIT    sim3_deviation of a well-conditioned valid hypothesis (2216 of them): worst 1.59e-12, median 8.8e-16,
                 99th percentile 4.4e-14 -> the floor, 1e-8
  REFINED_LIMIT  sim3_deviation of the refined C (27 solves): worst 2.23e-12, median 7.6e-15, 99th percentile 1.7e-12
                 -> the floor, 1e-8
  OMEGA_LIMIT    |Omega_host - Omega_restatement| over the largest diagonal entry: worst 9.73e-11, median 2.5e-11,
                 99th percentile 9.7e-11 (the restatement's central differences, not the closed form, set this) -> the
                 floor, 1e-8
  CHI2_LIMIT     |chi2_host - chi2_restatement| / max(chi2, 1), before and after the refinement (21 solves): worst
                 4.83e-13, median 2.3e-13, 99th percentile 4.7e-13 -> the floor, 1e-8
Hypotheses are left out of MODEL_LIMIT only for conditioning: the second singular value of the sample's
cross-covariance below 1e-10 of the first.  None of the valid hypotheses of RUNS is (the triangle test removes
them first); the bound of 5 % is asserted.
The refinement's iteration and trial counts and its chi2 are compared only where chi2 before the refinement is above
1e-12: on noise-free pixels chi2 is 1e-20 and whether a step is accepted is decided by rounding (the refined C is
compared all the same: every path stays at C*).

The planted truth.  Over the noisy cases of SIZE_CASES the restatement's refined C deviates from C* by at most 1.07e-3
rad of rotation and 1.77e-2 of |t| (the scene with repeated matches, which has the fewest distinct inliers; t is a
lever of the rotation about the cloud's centre, 15 map units away) and 5.24e-4 of log-scale (the 63-match scene); the
bounds asserted are twice those.  On
noise-free pixels C* is found to 1e-12."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import sim3_batch_cases as SC
import sim3_batch_ref as SR
from conftest import gpu_available
from sim3opt_amd import lib as L
from sim3opt_amd import sim3np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR = 1e-8
MODEL_MEASURED, REFINED_MEASURED, OMEGA_MEASURED, CHI2_MEASURED = 1.59e-12, 2.23e-12, 9.73e-11, 4.83e-13
MODEL_LIMIT = max(32 * MODEL_MEASURED, FLOOR)
REFINED_LIMIT = max(32 * REFINED_MEASURED, FLOOR)
OMEGA_LIMIT = max(32 * OMEGA_MEASURED, FLOOR)
CHI2_LIMIT = max(32 * CHI2_MEASURED, FLOOR)
TRUTH_ROT, TRUTH_T, TRUTH_SCALE = 2 * 1.07e-3, 2 * 1.77e-2, 2 * 5.24e-4
SV_RATIO_MIN = 1e-10   # a hypothesis below is left out of MODEL_LIMIT
CHI2_COMPARED = 1e-12  # the LM's path is compared where chi2 before it is above this
MARGIN = 1e-9          # no compared quantity lies within this, relative, of the value it is tested against
STATUS4_ITEMS = SC.opt_items(pixel_noise=1e200)  # Omega underflows to zero: its Cholesky fails
RUNS = SC.RUNS + (((65, 3, "noisy"), STATUS4_ITEMS),)
EXPECTED_STATUS = {((9, 1, "exact"), ()): 3, ((10, 2, "exact"), SC.opt_items(min_inliers=11)): 3,
                   ((65, 3, "noisy"), STATUS4_ITEMS): 4}
S3B_SYMBOLS = [s for s in L.SYMBOLS if s.startswith("sim3opt_sim3_batch_")]
RUN_IDS = lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else None


def off(values, at, rel=MARGIN):
    v = np.asarray(values, dtype=float)
    v = v[np.isfinite(v)]
    return bool((np.abs(v - at) > rel * at).all()) if at else bool((np.abs(v) > rel).all())


def rel_chi2(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=float) - b) / np.maximum(np.abs(b), 1.0)))


def omega_dev(a, b):
    scale = float(np.max(np.diag(b)))
    return float(np.abs(a - b).max() / scale) if scale > 0 else float(np.abs(a).max())


# ---- the host build ---------------------------------------------------------------------------------------------
def compile_cxx(tmp_path, name, flags=(), link=True):
    exe = str(tmp_path / name)
    libdir = os.path.join(ROOT, "sim3opt_amd")
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cxx", name + ".cpp")]
    if link:
        cmd += ["-L" + libdir, "-lsim3opt", "-Wl,-rpath," + libdir]
    subprocess.check_call(cmd + ["-o", exe])
    return exe


SANITIZED_FLAGS = ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wno-unknown-pragmas")
PLAIN_FLAGS = ("-O2", "-Wno-unknown-pragmas")


@functools.lru_cache(maxsize=None)
def driver_exe(sanitized=True):
    """tests/cxx/sim3_batch_math_driver.cpp as a stand-alone program, built once per process and kind: under the
    address and undefined-behaviour sanitizers for this file, plain for tests/test_gpu_sim3_batch.py (no sanitizer
    build runs from a test that has the GPU open)"""
    import pathlib
    import tempfile
    d = pathlib.Path(tempfile.mkdtemp(prefix="sim3_batch_driver_"))
    return compile_cxx(d, "sim3_batch_math_driver", flags=SANITIZED_FLAGS if sanitized else PLAIN_FLAGS, link=False)


def head_of(o, n):
    return (f"{SC.FOCAL!r} {SC.CX!r} {SC.CY!r} {o['seed']} {o['iterations']} {n} {o['max_pixel_error']!r} "
            f"{o['huber_delta']!r} {o['pixel_noise']!r} {o['min_triangle_sin2']!r} {o['tau']!r} {o['min_points']} "
            f"{o['min_inliers']} {o['refine_iters']} {o['max_trials']}")


def points_text(c):
    cols = np.column_stack([c["uv0"], c["depth0"], c["uv1"], c["depth1"]])
    return "\n".join(" ".join(repr(float(x)) for x in row) for row in cols)


def run_driver(mode, c, o, extra="", sanitized=True):
    text = head_of(o, len(c["uv0"])) + "\n" + points_text(c) + "\n" + extra
    out = subprocess.run([driver_exe(sanitized), mode], input=text, capture_output=True, text=True)
    assert out.returncode == 0 and not out.stderr, out.stderr  # (a sanitizer report lands in stderr)
    return [[float(x) for x in ln.split()] for ln in out.stdout.splitlines()]


def supplied_text(C, mask):
    return " ".join(repr(float(x)) for x in C) + "\n" + " ".join(str(int(m)) for m in mask) + "\n"


@functools.lru_cache(maxsize=None)
def host_hypotheses(case, items=(), sanitized=True):
    """the host build's hypotheses of a run: dict of sample (H, 3), valid, sim3 (H, 8), count, cost"""
    rows = np.array(run_driver("hyp", SC.make_case(*case), SC.merged(items), sanitized=sanitized))
    return dict(sample=rows[:, :3].astype(np.int32), valid=rows[:, 3].astype(np.int32), sim3=rows[:, 4:12].copy(),
                count=rows[:, 12].astype(np.int32), cost=rows[:, 13].copy())


@functools.lru_cache(maxsize=None)
def host_solve(case, items=(), sanitized=True):
    """the host build's solve of a run, keyed as sim3_batch_ref.solve's"""
    c, o = SC.make_case(*case), SC.merged(items)
    rows = run_driver("solve", c, o, sanitized=sanitized)
    n = len(c["uv0"])
    out = dict(status=int(rows[0][0]), best=int(rows[0][1]), n_hyp=int(rows[0][2]), cost_hyp=rows[0][3])
    if out["status"] in (1, 2):
        out.update(sim3=sim3np.identity(), information=np.zeros((7, 7)), mask=np.zeros(n, dtype=bool), n_inliers=0,
                   rms=0.0, iterations=0, chi2=np.zeros(2), trials=np.zeros(o["refine_iters"], dtype=np.int32),
                   mask_hyp=np.zeros(n, dtype=bool))
        return out
    out.update(mask_hyp=np.array(rows[1]) != 0, sim3=np.array(rows[2]), iterations=int(rows[3][0]),
               chi2=np.array(rows[3][1:]), trials=np.array(rows[4], dtype=np.int32), mask=np.array(rows[5]) != 0,
               n_inliers=int(rows[6][0]), rms=rows[6][1], information=np.array(rows[7]).reshape(7, 7).T.copy())
    return out


def host_refine(case, o, C, mask, sanitized=True):
    rows = run_driver("refine", SC.make_case(*case), o, supplied_text(C, mask), sanitized)
    return dict(sim3=np.array(rows[0]), iterations=int(rows[1][0]), chi2=np.array(rows[1][1:]),
                trials=np.array(rows[2], dtype=np.int32))


def host_information(case, o, C, mask, sanitized=True):
    rows = run_driver("info", SC.make_case(*case), o, supplied_text(C, mask), sanitized)
    return dict(positive_definite=int(rows[0][0]), information=np.array(rows[1]).reshape(7, 7).T.copy(),
                weights=np.array(rows[2:]))


def well_conditioned(ref):
    return (ref["hyp"]["valid"] != 0) & (ref["hyp"]["sv_ratio"] >= SV_RATIO_MIN)


def best_is_unique(ref):
    """whether the restatement's best hypothesis leads the next of the same count by MARGIN of its cost; if not,
    whether every such rival is a twin: the same model within MODEL_LIMIT"""
    h, b = ref["hyp"], ref["best"]
    rivals = [k for k in range(len(h["valid"])) if k != b and h["valid"][k] and h["count"][k] == h["count"][b] and
              not float(h["cost"][k] - h["cost"][b]) > MARGIN * max(float(h["cost"][b]), 1.0)]
    return not rivals, all(SC.sim3_deviation(h["sim3"][k], h["sim3"][b]) < MODEL_LIMIT for k in rivals)


# ---- the conditions the GPU comparisons rest on -----------------------------------------------------------------------
@pytest.mark.parametrize("case,items", RUNS, ids=RUN_IDS)
def test_conditions_of_the_comparisons(case, items):
    """No error within 1e-9 relative of the threshold and no depth within 1e-9 of zero, for every valid hypothesis and
    for the refined C; no triangle within 1e-9 of the degeneracy threshold; the best hypothesis unique in (count, cost)
    or a twin of the same model; at least min_inliers inliers where status 0 is expected."""
    o, ref, D = SC.merged(items), SC.reference(case, items), SC.data_of(case)
    max2 = o["max_pixel_error"] ** 2
    sims = [ref["hyp"]["sim3"][h] for h in np.flatnonzero(ref["hyp"]["valid"])] + [ref["sim3"]]
    for C in sims:
        e1, e0, _ = SR.errors(C, D)
        A, t, Ai, ti = SR.both_ways(C)
        assert off(e1, max2) and off(e0, max2)
        assert off((D["X0"] @ A.T + t)[:, 2], 0.0) and off((D["X1"] @ Ai.T + ti)[:, 2], 0.0)
    for idx in ref["hyp"]["sample"]:
        assert off([SR.triangle_sin2(D["X0"][idx]), SR.triangle_sin2(D["X1"][idx])], o["min_triangle_sin2"])
    unique, twins = best_is_unique(ref)
    assert unique or twins
    assert unique or case[2] in ("exact", "behind")  # (noise-free pixels: every all-inlier sample gives C*)
    expected = EXPECTED_STATUS.get((case, items), 0)
    assert ref["status"] == expected
    if expected == 0:
        assert ref["n_inliers"] >= o["min_inliers"]
    # Huber on both sides of its width, where it is on
    if o["huber_delta"] > 0 and case[2] in ("noisy", "dup") and ref["status"] == 0:
        w = SR.information(ref["sim3"], D, ref["mask"], o)["weights"][ref["mask"]]
        if (case, items) == ((257, 3, "noisy"), SC.opt_items(huber_delta=0.4)):
            assert (w < 1.0).sum() > 20 and (w == 1.0).sum() > 20


def test_the_listed_cases_cover_the_kernel_paths():
    sizes = {c[0] for c in SC.MIXED}
    assert {3, 8, 9, 10, 63, 64, 65, 255, 256, 257, SC.LDS_POINTS - 1, SC.LDS_POINTS, SC.LDS_POINTS + 1} <= sizes
    assert {c[2] for c in SC.MIXED} == {"exact", "noisy", "dup", "line", "behind"}
    assert {SC.make_case(*c)["C_true"][7] for c in SC.SIZE_CASES} == set(SC.SCALES)
    angles = [2 * np.arccos(min(1.0, SC.make_case(*c)["C_true"][3])) for c in SC.SIZE_CASES]
    assert min(angles) < 0.15 and max(angles) > 1.7
    assert {dict(i).get("iterations") for _, i in SC.RUNS} >= set(SC.ITERATION_COUNTS)
    c = SC.make_case(80, 9, "behind")
    assert (~c["front"]).sum() == 32 and (c["depth1"] > 0).all() and (c["depth0"] > 0).all()
    c = SC.make_case(66, 2, "dup")
    assert (c["uv0"][0] == c["uv0"][1]).all() and (c["depth1"][4] == c["depth1"][5])


# ---- the restatement --------------------------------------------------------------------------------------------------
def test_restatement_finds_the_planted_truth_and_reaches_every_status():
    seen, worst = set(), np.zeros(3)
    for case, items in RUNS:
        ref = SC.reference(case, items)
        seen.add(ref["status"])
        if ref["status"] != 0 or SC.merged(items)["iterations"] < 64:  # (fewer hypotheses need not hold an all-inlier sample)
            continue
        c = SC.make_case(*case)
        err = np.array(SC.truth_errors(ref["sim3"], c))
        if case[2] in ("exact", "behind"):
            assert err.max() < 1e-12, (case, err)
            assert (ref["mask"] == c["front"]).all()
        else:
            worst = np.maximum(worst, err)
            assert err[0] < TRUTH_ROT and err[1] < TRUTH_T and err[2] < TRUTH_SCALE, (case, items, err)
            assert not (ref["mask"] & c["outlier"]).any() and ref["n_inliers"] >= 0.9 * (~c["outlier"]).sum()
    for case in SC.SMALL_CASES + (SC.LINE_CASE,):
        seen.add(SC.reference(case)["status"])
    assert SC.reference(SC.LINE_CASE)["status"] == 2 and SC.reference((8, 2, "exact"))["status"] == 1
    assert seen == {0, 1, 2, 3, 4}
    print("planted truth, worst over the noisy runs (rotation, t / |t|, log-scale):", worst)
    assert (worst > np.array([TRUTH_ROT, TRUTH_T, TRUTH_SCALE]) / 4).all()  # (the bounds are twice a measurement of this)


# (more than one pass of the 256-thread stride; a weak best hypothesis, whose inlier set the refinement changes)
DEFECT_CASE = {"lane_stride_once": ((257, 3, "noisy"), {}), "mask_not_rederived": ((66, 2, "dup"), dict(iterations=3))}


@pytest.mark.parametrize("defect", SR.DEFECTS)
def test_restatement_notices_a_seeded_defect(defect):
    """One wrong line moves the refined C, Omega or the mask by far more than the limits."""
    case, extra = DEFECT_CASE.get(defect, ((65, 3, "noisy"), {}))
    o = SC.merged(SC.opt_items(huber_delta=0.4, **extra))  # (Huber binds: its weight is part of what is seeded)
    good, bad = SC.run_reference(SC.make_case(*case), o), SC.run_reference(SC.make_case(*case), o, defect)
    dC = SC.sim3_deviation(bad["sim3"], good["sim3"])
    dO = omega_dev(bad["information"], good["information"])
    dM = int((bad["mask"] != good["mask"]).sum())
    print(defect, dC, dO, dM, bad["status"], bad["n_inliers"])
    assert dC > 100 * REFINED_LIMIT or dO > 100 * OMEGA_LIMIT or dM > 0, (defect, dC, dO, dM)
    if defect == "mask_not_rederived":
        assert dM > 0
    if defect in ("omega_transposed", "huber_squared", "lane_stride_once"):
        assert dO > 100 * OMEGA_LIMIT
    # the Jacobian defects leave the minimiser where it is but not the information: the convergence test of
    # tests/test_gpu_sim3_batch.py rests on this
    if defect in ("tangent_order", "right_perturbation"):
        assert dO > 1e-3


# ---- the host build against the restatement ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def measured():
    """the deviations of the host build from the restatement over RUNS: dict of arrays"""
    dev = dict(model=[], refined=[], omega=[], chi2=[])
    left_out = total = 0
    for case, items in RUNS:
        ref, got, sol = SC.reference(case, items), host_hypotheses(case, items), host_solve(case, items)
        assert (got["sample"] == ref["hyp"]["sample"]).all() and (got["valid"] == ref["hyp"]["valid"]).all(), (case, items)
        assert (got["count"] == ref["hyp"]["count"]).all(), (case, items)
        ok = well_conditioned(ref)
        total += int((ref["hyp"]["valid"] != 0).sum())
        left_out += int(((ref["hyp"]["valid"] != 0) & ~ok).sum())
        dev["model"] += [SC.sim3_deviation(got["sim3"][h], ref["hyp"]["sim3"][h]) for h in np.flatnonzero(ok)]
        d = np.abs(got["cost"] - ref["hyp"]["cost"].astype(float)) / np.maximum(ref["hyp"]["cost"].astype(float), 1.0)
        assert d.max() < CHI2_LIMIT, (case, items, d.max())
        assert sol["status"] == ref["status"] and sol["n_hyp"] == ref["n_hyp"], (case, items, sol["status"])
        unique, _ = best_is_unique(ref)
        assert sol["best"] == ref["best"] or not unique, (case, items)
        assert (sol["mask_hyp"] == ref["mask_hyp"]).all() and (sol["mask"] == ref["mask"]).all(), (case, items)
        assert sol["n_inliers"] == ref["n_inliers"] and abs(sol["rms"] - ref["rms"]) < REFINED_LIMIT
        dev["refined"].append(SC.sim3_deviation(sol["sim3"], ref["sim3"]))
        dev["omega"].append(omega_dev(sol["information"], ref["information"]))
        if ref["chi2"][0] > CHI2_COMPARED:
            assert sol["iterations"] == ref["iterations"] and (sol["trials"] == ref["trials"]).all(), (case, items)
            dev["chi2"].append(rel_chi2(sol["chi2"], ref["chi2"]))
    out = {k: np.array(v) for k, v in dev.items()}
    out.update(left_out=left_out, total=total)
    return out


def test_host_build_agrees_with_the_restatement_within_the_limits():
    """Every run: samples, validity, counts, statuses and masks equal; models, refined C, Omega and chi2 within the
    limits, which are 32 times what this test measures (printed)."""
    m = measured()
    for k, lim, meas in (("model", MODEL_LIMIT, MODEL_MEASURED), ("refined", REFINED_LIMIT, REFINED_MEASURED),
                         ("omega", OMEGA_LIMIT, OMEGA_MEASURED), ("chi2", CHI2_LIMIT, CHI2_MEASURED)):
        v = m[k]
        print(f"{k}: n {len(v)} worst {v.max():.3g} median {np.median(v):.3g} p99 {np.percentile(v, 99):.3g}")
        assert v.max() < lim, (k, v.max())
        assert v.max() > meas / 32, (k, v.max())  # (the limit rests on a measurement of this code)
    print("valid hypotheses", m["total"], "left out for conditioning", m["left_out"])
    assert m["total"] > 1000 and m["left_out"] <= 0.05 * m["total"]


def test_plain_host_build_has_the_sanitized_builds_bits():
    """tests/test_gpu_sim3_batch.py compares the device with the plain (-O2) build of the driver, this file measures the
    limits with the sanitized (-O1) one: both print the same numbers."""
    for case, items in (((65, 3, "noisy"), ()), ((257, 3, "noisy"), SC.opt_items(huber_delta=0.4)),
                        ((256, 2, "exact"), ())):
        c, o = SC.make_case(*case), SC.merged(items)
        for mode in ("hyp", "solve"):
            assert run_driver(mode, c, o, sanitized=False) == run_driver(mode, c, o), (case, mode)


def test_host_build_refines_and_informs_as_the_restatement_from_supplied_input():
    """debug_refine's and debug_information's statements from a supplied C on a supplied mask: the planted C* moved by
    a known delta, on every match that is not a planted outlier."""
    for case, items in (((65, 3, "noisy"), ()), ((257, 3, "noisy"), SC.opt_items(huber_delta=0.4)),
                        ((256, 2, "exact"), SC.opt_items(huber_delta=0.0))):
        c, o, D = SC.make_case(*case), SC.merged(items), SC.data_of(case)
        C = SR.perturbed(c["C_true"], np.array([2e-3, -1e-3, 1.5e-3, 0.02, -0.01, 0.03, 4e-3]))
        mask = ~c["outlier"]
        a, b = host_refine(case, o, C, mask), SR.refine(C, D, mask, o)
        assert SC.sim3_deviation(a["sim3"], b["sim3"]) < REFINED_LIMIT
        assert rel_chi2(a["chi2"][:1], b["chi2"][:1]) < CHI2_LIMIT and b["chi2"][0] > 1.0
        if b["chi2"][1] > CHI2_COMPARED:
            assert a["iterations"] == b["iterations"] and (a["trials"] == b["trials"]).all()
            assert rel_chi2(a["chi2"], b["chi2"]) < CHI2_LIMIT
        a, b = host_information(case, o, C, mask), SR.information(C, D, mask, o)
        assert omega_dev(a["information"], b["information"]) < OMEGA_LIMIT and a["positive_definite"] == 1
        assert np.abs(a["weights"] - b["weights"]).max() < OMEGA_LIMIT
        assert (a["information"] == a["information"].T).all()


# ---- the helper's conformance program ----------------------------------------------------------------------------------
CONFORMANCE_CASES = ((65, 3, "noisy"), (257, 3, "noisy"), (120, 4, "exact"))


def compile_conformance(tmp_path):
    return compile_cxx(tmp_path, "sim3_batch_conformance")


def write_conformance_file(path, cases):
    with open(path, "w") as fp:
        fp.write(f"{len(cases)} {SC.FOCAL!r} {SC.CX!r} {SC.CY!r} {SC.OPTS['iterations']} {TRUTH_ROT!r} {TRUTH_T!r} "
                 f"{TRUTH_SCALE!r}\n")
        for case in cases:
            c = SC.make_case(*case)
            fp.write(f"{case[0]}\n{points_text(c)}\n" + " ".join(repr(float(x)) for x in c["C_true"]) + "\n")


def test_conformance_host_part(tmp_path):
    """include/sim3opt_sim3_batch.hpp compiles -Werror beside sim3opt_homography.hpp without Eigen or OpenCV; its add() /
    feed() / solve() refusals and the C-ABI's leave everything as it was."""
    exe = compile_conformance(tmp_path)
    r = subprocess.run([exe, "host"], capture_output=True, text=True)
    assert r.returncode == 0 and " 0 failed" in r.stdout, r.stdout + r.stderr


def test_conformance_fails_loudly_without_gpu(tmp_path):
    if gpu_available():
        pytest.skip("GPU present: covered by the gpu tests")
    exe = compile_conformance(tmp_path)
    path = str(tmp_path / "candidates.txt")
    write_conformance_file(path, CONFORMANCE_CASES[:2])
    r = subprocess.run([exe, "run", path], capture_output=True, text=True)
    assert r.returncode == 3 and "no usable HIP device" in r.stderr, r.stdout + r.stderr


# ---- the C entries without a GPU --------------------------------------------------------------------------------------
def test_symbols_and_options_struct():
    assert len(S3B_SYMBOLS) == 15
    o = L.Sim3BatchOptions()
    L.load().sim3opt_sim3_batch_options_default(ctypes.byref(o))
    got = {k: getattr(o, k) for k, _ in L.Sim3BatchOptions._fields_ if k != "device"}
    assert got == SR.DEFAULTS and o.device == -1
    assert (L.SIM3_OK, L.SIM3_FEW_POINTS, L.SIM3_NO_HYPOTHESIS, L.SIM3_FEW_INLIERS, L.SIM3_NOT_POSITIVE) == (0, 1, 2, 3, 4)


def small_batch():
    a = SC.batch_arrays(((10, 2, "exact"),))
    a = dict(point_ptr=np.array([0, 9, 12, 15], dtype=np.int32),
             **{k: np.concatenate([a[k], a[k]])[:15] for k in ("uv0", "uv1", "depth0", "depth1")})
    b = L.Sim3Batch()
    b.set_problems(**a)
    return a, b


@pytest.mark.parametrize("what", ["no_problem", "empty_problem", "not_monotone", "ptr0", "nan_uv0", "inf_uv1", "focal",
                                  "nan_cx", "zero_depth0", "negative_depth1", "nan_depth0"])
def test_set_problems_refuses_and_changes_nothing(what):
    a, b = small_batch()
    assert b.dims() == (3, 15)  # (problems of fewer than min_points matches are accepted: they end with status 1)
    bad = {k: np.array(v) for k, v in a.items()}
    kw = {}
    if what == "no_problem":
        bad["point_ptr"] = np.array([0], dtype=np.int32)
    elif what == "empty_problem":
        bad["point_ptr"] = np.array([0, 9, 9, 15], dtype=np.int32)
    elif what == "not_monotone":
        bad["point_ptr"] = np.array([0, 10, 9, 15], dtype=np.int32)
    elif what == "ptr0":
        bad["point_ptr"] = np.array([1, 9, 12, 15], dtype=np.int32)
    elif what == "nan_uv0":
        bad["uv0"][7, 1] = np.nan
    elif what == "inf_uv1":
        bad["uv1"][14, 0] = -np.inf
    elif what == "focal":
        kw["focal"] = 0.0
    elif what == "nan_cx":
        kw["cx"] = float("nan")
    elif what == "zero_depth0":
        bad["depth0"][3] = 0.0
    elif what == "negative_depth1":
        bad["depth1"][14] = -2.0
    elif what == "nan_depth0":
        bad["depth0"][0] = np.nan
    with pytest.raises(L.Sim3OptError) as e:
        b.set_problems(**bad, **kw)
    assert e.value.code == L.ERR_ARG and "sim3_batch_set_problems" in str(e.value)
    if "depth" in what and "nan" not in what:
        assert "not positive" in str(e.value)
    assert b.dims() == (3, 15)


@pytest.mark.parametrize("kw", [dict(iterations=0), dict(iterations=4097), dict(max_pixel_error=0.0),
                                dict(max_pixel_error=float("inf")), dict(huber_delta=-1.0),
                                dict(huber_delta=float("nan")), dict(pixel_noise=0.0), dict(pixel_noise=float("inf")),
                                dict(min_triangle_sin2=-1e-3), dict(min_triangle_sin2=1.0), dict(tau=0.0),
                                dict(min_points=2), dict(min_inliers=-1), dict(refine_iters=-1), dict(max_trials=0)])
def test_set_options_refuses_and_changes_nothing(kw):
    _, b = small_batch()
    before = b.options()
    with pytest.raises(L.Sim3OptError) as e:
        b.set_options(**kw)
    assert e.value.code == L.ERR_ARG and "value out of range" in str(e.value)
    assert b.options() == before and b.dims() == (3, 15)
    b.set_options(iterations=4096, min_points=3, huber_delta=0.0, min_triangle_sin2=0.0, refine_iters=0,
                  seed=2 ** 64 - 1)  # the ends of the ranges are taken
    assert b.options()["seed"] == 2 ** 64 - 1 and b.tiles() == (SC.LDS_POINTS, SC.CHUNK)


def test_state_and_argument_errors_before_a_solve():
    _, b = small_batch()
    for call in (b.sim3, b.information, b.inliers, b.summary, lambda: b.debug_hypotheses(0)):
        with pytest.raises(L.Sim3OptError) as e:
            call()
        assert e.value.code == L.ERR_STATE
    with pytest.raises(L.Sim3OptError) as e:
        L.Sim3Batch().solve()
    assert e.value.code == L.ERR_STATE and "no problems set" in str(e.value)
    lib, nul = L.load(), None
    assert lib.sim3opt_sim3_batch_debug_score(b._b, 0, nul, nul, nul) == L.ERR_ARG
    assert lib.sim3opt_sim3_batch_debug_refine(b._b, nul, nul, nul, nul, nul, nul) == L.ERR_ARG
    assert lib.sim3opt_sim3_batch_debug_information(b._b, nul, nul, nul, nul, nul) == L.ERR_ARG
    assert lib.sim3opt_sim3_batch_get_sim3(b._b, nul, nul) == L.ERR_ARG
    assert lib.sim3opt_sim3_batch_get_inliers(b._b, nul, nul) == L.ERR_ARG
    assert lib.sim3opt_sim3_batch_solve(nul) == L.ERR_ARG and lib.sim3opt_sim3_batch_set_options(nul, nul) == L.ERR_ARG
    bad = sim3np.identity(3)
    bad[1, 7] = 0.0  # a scale that is not positive
    with pytest.raises(L.Sim3OptError) as e:
        b.debug_information(bad, np.ones(15, dtype=np.uint8))
    assert e.value.code == L.ERR_ARG and "not a similarity" in str(e.value)
    bad[1, 7], bad[2, 4] = 1.0, np.nan
    with pytest.raises(L.Sim3OptError) as e:
        b.debug_refine(bad, np.ones(15, dtype=np.uint8))
    assert e.value.code == L.ERR_ARG
    with pytest.raises(ValueError):
        b.debug_refine(sim3np.identity(2), np.ones(15, dtype=np.uint8))


def test_no_device_is_an_error_not_a_fallback():
    if gpu_available():
        pytest.skip("GPU present: covered by the gpu tests")
    _, b = small_batch()
    with pytest.raises(L.Sim3OptError) as e:
        b.solve()
    assert e.value.code == L.ERR_NO_DEVICE and "no CPU fallback" in str(e.value)
    for call in (lambda: b.debug_score(sim3np.identity(3)),
                 lambda: b.debug_refine(sim3np.identity(3), np.ones(15, dtype=np.uint8)),
                 lambda: b.debug_information(sim3np.identity(3), np.ones(15, dtype=np.uint8))):
        with pytest.raises(L.Sim3OptError) as e:
            call()
        assert e.value.code == L.ERR_NO_DEVICE
