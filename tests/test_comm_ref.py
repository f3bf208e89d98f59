"""CPU tests of tests/comm_ref.py and tests/comm_cases.py, the yardstick and the cases of
tests/test_gpu_comm_operators.py: the model of the transport (comm_ref.Transport) agrees with the plain restatement
bit for bit on every case, every case meets the path condition it is there for, and -- the SENSITIVITY of the GPU
comparisons -- every defect of comm_ref.DEFECTS, switched on in the model, changes at least one bit of at least one
case's result (or a guard double) in every family CATCHES names for it.  CATCHES names every family at least once, so
a family that goes missing from comm_cases.py fails here.  Nothing needs a GPU.
"""
import os
import subprocess

import numpy as np
import pytest

from sim3opt_amd import lib as L
from test_devmem_owners import ROOT, SAN
import comm_cases as C
import comm_ref as R

# defect -> the families whose cases must see it
CATCHES = {
    "fold_right": ("allreduce_small",),
    "fold_pairwise": ("allreduce_small",),
    "head_dropped": ("allgather_small",),
    "tail_dropped": ("allreduce_small", "allgather_small", "exchange_small"),
    "pairs_one_short": ("allreduce_small", "allgather_small", "exchange_small"),
    "one_past": ("allgather_small", "exchange_small"),
    "slot_by_n": ("allreduce_small",),
    "max_loses_nan": ("allreduce_small",),
    "max_positive_zero": ("allreduce_small",),
    "other_parity": ("sequences",),
    "old_slot_after_growth": ("growth",),
    "no_second_round_put": ("growth",),
    "one_sweep": ("allreduce_long", "allgather_long"),
}
MODEL_CAP = 4096  # mailboxes that hold every small case: only the growth family starts smaller


def model_for(sc, defect=None):
    return R.Transport(sc["world"], cap=sc.get("cap", MODEL_CAP), seq=0, defect=defect)


def run(sc, defect=None):
    """-> (per step: per-rank results, guards intact, the model afterwards)"""
    T = model_for(sc, defect)
    return [C.run_on_model(T, st) for st in sc["steps"]], T.guards_ok, T


def sees(sc, defect):
    outs, guards, _ = run(sc, defect)
    if not guards:
        return True
    for st, out in zip(sc["steps"], outs):
        if not all(R.same_bits(a, b) for a, b in zip(out, C.expected(st))):
            return True
    return False


def test_tables_are_complete():
    assert set(CATCHES) == set(R.DEFECTS)
    assert {f for fams in CATCHES.values() for f in fams} == set(C.FAMILIES)
    for fam in C.FAMILIES:
        assert C.scenarios(fam), fam


def test_guard_and_sentinel_patterns_survive_numpy():
    o = R.Operand(np.full(5, C.SENTINEL), 1)
    assert o.guards_ok() and o.lead == R.GUARD_DOUBLES + 1 and len(o.a) == 5 + 2 * R.GUARD_DOUBLES + 1
    assert (R.bits(o.data()) == 0x7FF85E4711E15E47).all() and (R.bits(o.a[:5]) == 0x7FF4C0DEDBADF00D).all()
    o.a[o.lead + 5] = 0.0
    assert not o.guards_ok()


def test_the_maximum_is_the_stated_rule_and_the_sum_is_a_left_fold():
    """The rule is acc if (acc >= v or acc != acc) else v, element by element in plain Python here.  numpy.maximum
    agrees with it everywhere but in the sign of a zero: for (-0.0, +0.0) the rule keeps -0.0, numpy.maximum answers
    whatever its vector path gives (+0.0 in some builds), so it is compared away from zeros only."""
    for world in C.WORLDS:
        rows = C.operand_rows(world, 64, 9)
        ref, acc = rows[0], [float(x) for x in rows[0]]
        for r in rows[1:]:
            ref = np.maximum(ref, r)
            acc = [a if (a >= float(v) or a != a) else float(v) for a, v in zip(acc, r)]
        got = R.fold(list(rows), 1)
        assert R.same_bits(got, np.array(acc))
        nz = ref != 0.0
        assert nz.sum() >= 60 and R.same_bits(got[nz], ref[nz]) and (got[~nz] == 0.0).all()
        acc = rows[0].copy()
        for r in range(1, world):
            for i in range(64):
                acc[i] = float(acc[i]) + float(rows[r][i])
        assert R.same_bits(R.fold(list(rows), 0), acc)
    assert R.same_bits(R.fold([np.array([-0.0]), np.array([0.0])], 1), np.array([-0.0]))
    assert np.isnan(R.fold([np.array([1.0]), np.array([np.nan]), np.array([2.0])], 1)[0])


@pytest.mark.parametrize("family", list(C.FAMILIES))
def test_model_agrees_with_the_yardstick(family):
    for sc in C.scenarios(family):
        outs, guards, _ = run(sc)
        assert guards, sc["name"]
        for st, out in zip(sc["steps"], outs):
            exp = C.expected(st)
            assert len(out) == len(exp) == sc["world"]
            for r, (a, b) in enumerate(zip(out, exp)):
                assert R.same_bits(a, b), (sc["name"], st["kind"], r)


@pytest.mark.parametrize("defect,family", [(d, f) for d, fams in CATCHES.items() for f in fams])
def test_every_defect_changes_a_bit_of_some_case(defect, family):
    seen = [sc["name"] for sc in C.scenarios(family) if sees(sc, defect)]
    print(f"{defect}: seen by {len(seen)} of {len(C.scenarios(family))} cases of {family}")
    assert seen, (defect, family)


# ------------------------------------------------------------------------------------------------ path conditions
def test_allreduce_paths():
    ns = set(C.ALLREDUCE_NS)
    assert {0, 1, 2, 3} <= ns and any(n % 2 for n in ns if n > 3) and {255, 256, 257} <= ns
    for n in C.ALLREDUCE_NS:  # put: mailbox slot r * slot (even) <- operand at GUARD_DOUBLES + phase
        gx = R.copy_grid(n)
        p0, p1 = R.span_path(0, R.GUARD_DOUBLES, n, gx), R.span_path(0, R.GUARD_DOUBLES + 1, n, gx)
        assert p0["same_phase"] and p0["head"] == 0 and p0["tail"] == n % 2 and not p1["same_phase"]
    assert R.span_path(0, 5, 513, R.copy_grid(513))["sweeps"] == 3  # (the scalar loop goes round at 513 already)
    n = C.ALLREDUCE_LONG_N
    assert n > R.reduce_grid(n) * R.COMM_WG and R.reduce_grid(n) == R.COMM_MAX_GRID_X
    assert R.span_path(0, 5, n, R.copy_grid(n))["sweeps"] == 2 and R.span_path(0, 4, n, R.copy_grid(n))["sweeps"] == 1
    assert [(s["steps"][0]["phase"], s["steps"][0]["op"]) for s in C.allreduce_long(3)] == [(0, 0), (1, 1)]


def put_paths(offs, phase):
    """span_path of every rank's put of an all-gather (mailbox + lo <- vector + lo)"""
    out = []
    for r in range(len(offs) - 1):
        lo, n = offs[r], offs[r + 1] - offs[r]
        if n:
            out.append((n, R.span_path(lo, R.GUARD_DOUBLES + phase + lo, n, R.copy_grid(n))))
    return out


@pytest.mark.parametrize("world", C.WORLDS)
def test_allgather_paths(world):
    plans = C.allgather_plans(world)
    eq = plans["engine's equal plan, short tail"]
    rb = L.partition_rows_equal(2 * world - 1, world)
    assert eq == [7 * int(x) for x in rb] and 0 < eq[-1] - eq[-2] < eq[1] - eq[0]
    assert plans["empty first rank"][1] == 0 and plans["empty last rank"][-1] == plans["empty last rank"][-2]
    own = np.diff(plans["one rank owns everything"])
    assert (own > 0).sum() == 1
    if world > 2:
        mid = np.diff(plans["empty middle rank"])
        assert mid[world // 2] == 0 and mid[0] > 0 and mid[-1] > 0
    shapes = set()
    for offs in plans.values():
        for n, p in put_paths(offs, 0):
            assert p["same_phase"]
            shapes.add((min(n, 4), p["head"], p["tail"]))
        for n, p in put_paths(offs, 1):
            assert not p["same_phase"]
    if world > 2:  # a head alone, a pair alone, a tail alone, head + pair, pair + tail
        assert {(1, 1, 0), (1, 0, 1), (2, 0, 0), (3, 1, 0), (3, 0, 1)} <= shapes, shapes
    assert any(p["head"] and p["pairs"] and p["tail"] for offs in plans.values() for _, p in put_paths(offs, 0))
    wg = plans["more than one workgroup"]
    assert max(R.copy_grid(n) for n in np.diff(wg)) > 1


def test_allgather_long_wraps_the_pair_loop():
    even, odd = [s["steps"][0] for s in C.allgather_long(2)]
    for st, head in ((even, 0), (odd, 1)):
        assert st["phase"] == 0
        (n, p), = [x for x in put_paths(st["offs"], 0) if x[0] > 5]
        assert n == C.ALLGATHER_LONG_SPAN and p["head"] == head and p["sweeps"] == 2 and R.copy_grid(n) == R.COMM_MAX_GRID_X


@pytest.mark.parametrize("world", C.WORLDS)
def test_exchange_paths(world):
    lens, same, paths = set(), set(), []
    for sc in C.exchange_small(world):
        st = sc["steps"][0]
        for r in range(world):
            assert st["soffs"][r][0] == r % 2 and st["roffs"][r][0] == (r + 1) % 2
            for p in range(world):
                n = st["roffs"][r][p + 1] - st["roffs"][r][p]
                lens.add(n)
                if n:  # unpack: receive buffer <- mailbox slot (even)
                    q = R.span_path(R.GUARD_DOUBLES + st["recv_phase"] + st["roffs"][r][p], 0, n, 1)
                    assert q["head"] == 0
                    same.add((sc["name"], r, q["same_phase"]))
                    paths.append(q)
    assert ({0, 1, 2, 7, 9} if world > 2 else {0, 1, 7, 9}) <= lens, lens
    assert any(q["tail"] for q in paths) and any(q["same_phase"] and not q["tail"] for q in paths)
    # one launch with both paths: some rank of some case has spans of either kind
    both = {(name, r) for name, r, s in same if s} & {(name, r) for name, r, s in same if not s}
    assert both
    phases = {(sc["steps"][0]["send_phase"], sc["steps"][0]["recv_phase"]) for sc in C.exchange_small(world)}
    assert phases == {(0, 0), (0, 1), (1, 0), (1, 1)}
    one_way = C.exchange_plans(world)["one pair, one way"]
    assert one_way[0][world - 1] > 0 and one_way[world - 1][0] == 0
    assert not np.asarray(C.exchange_plans(world)["all empty"]).any()


@pytest.mark.parametrize("world", [w for w in C.WORLDS if C.growth(w)])
def test_growth_takes_the_second_round(world):
    sc, = C.growth(world)
    cap = sc["cap"]
    f = C.growth_facts(sc["steps"][0], world, cap)
    assert f["fits"].count(False) == 2 and f["fits"].count(True) == world - 2  # the long segment's sender and receiver
    counts = C.growth_counts(world, cap)
    assert (counts > 2).sum() == 1 and counts.max() == cap // world + 2 > ((cap // world) & ~1)
    T = model_for(sc)
    out = C.run_on_model(T, sc["steps"][0])
    assert all(R.same_bits(a, b) for a, b in zip(out, C.expected(sc["steps"][0])))
    assert T.seq == 3 and T.cap > cap  # round 0's barrier, the growth's, round 1's
    C.run_on_model(T, sc["steps"][1])
    assert T.seq == 4


@pytest.mark.parametrize("world", C.WORLDS)
def test_sequences_shrink_and_start_at_both_parities(world):
    even, odd = C.sequences(world)
    assert len(even["steps"]) == 5 and len(odd["steps"]) == 6 and odd["steps"][0]["rows"].shape == (world, 1)
    assert {s["kind"] for s in even["steps"]} == {"allreduce", "allgatherv", "exchange"}
    for sc, first in ((even, 0), (odd, 1)):
        _, _, T = run(dict(sc, steps=sc["steps"][:first]))
        assert T.seq & 1 == sc["start_parity"] == first
    size = lambda st: (st["rows"].shape[1] if st["kind"] != "exchange" else max(len(s) for s in st["send"]))
    sizes = [size(st) for st in even["steps"]]
    assert sizes[0] > sizes[2] > sizes[3] > sizes[4] and sizes[1] > sizes[2]


# ------------------------------------------------------------------------------- the host half of the read-outs
def test_argument_and_plan_checks_under_asan_ubsan(tmp_path):
    """csrc/comm_apply_host.hpp -- what sim3opt_comm_apply_* decides for all ranks before any of them enters a
    collective: arguments, offsets, the agreement of the exchange plans, where each rank's buffers start -- stand-alone
    (tests/cxx/comm_apply_host_driver.cpp), every message as an exact string."""
    exe = str(tmp_path / "comm_apply_host_san")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + SAN +
                          [os.path.join(ROOT, "tests", "cxx", "comm_apply_host_driver.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.strip().endswith("comm apply host ok"), r.stdout[-2000:]
