"""The host logic of the frame store (sim3opt_amd/csrc/frames_host.hpp) on the CPU, under AddressSanitizer +
UndefinedBehaviorSanitizer: a stand-alone program (tests/cxx/frames_host_driver.cpp) checks every refusal message of the
argument checks as an exact string, counts the snapshot's holders against a stub allocator (the blocks go back once,
with the last holder, whatever the order; a refill leaves a consumer's snapshot alone) and holds the serial restatement
of the compaction's offsets against a second one organised in tiles with a carry, as the kernels are.  And what needs
no device of the library itself: the entries exist, and the refusals that come before the device is touched."""
import os
import subprocess

import numpy as np

from sim3opt_amd import lib as L
from test_devmem_owners import SAN
from test_example_cpp import ROOT


def test_host_logic_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "frames_host_san")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + SAN +
                          [os.path.join(ROOT, "tests", "cxx", "frames_host_driver.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.strip().endswith("frames host ok"), r.stdout[-2000:]


def test_refusals_that_need_no_device():
    before = L.device_memory_in_use()
    s = L.FrameStore()
    d = s.dims()
    assert (d["n_frames"], d["total_keypoints"], d["device"], d["desc_bytes"]) == (0, 0, -1, 0)
    assert (d["compact_tile"], d["row_lanes"]) == (256, 16)
    lib = L.load()
    assert lib.sim3opt_frames_get(s._b, None, None, None) == L.ERR_STATE
    assert lib.sim3opt_frames_last_error(s._b) == b"frames_get: the store is not filled"
    ptr, kp, desc = np.array([0, 2], np.int32), np.zeros((2, 2), np.float32), np.zeros((2, 64), np.float32)
    desc[1, 7] = np.nan
    assert lib.sim3opt_frames_set(s._b, 1, L._p(ptr, L._ip), L._p(kp, L._fp), L._p(desc, L._fp)) == L.ERR_ARG
    assert lib.sim3opt_frames_last_error(s._b) == b"frames_set: a non-finite descriptor"
    assert lib.sim3opt_frames_set(None, 1, L._p(ptr, L._ip), L._p(kp, L._fp), L._p(desc, L._fp)) == L.ERR_ARG
    state = np.array([2, 5], np.int32)
    assert lib.sim3opt_frames_debug_compact(s._b, 1, L._p(ptr, L._ip), L._p(state, L._ip), L._p(kp, L._fp),
                                            L._p(kp, L._fp)) == L.ERR_ARG
    assert lib.sim3opt_frames_last_error(s._b) == b"frames_debug_compact: slot 1: no such state"
    o = L.FrameStoreOptions(device=-2)
    assert lib.sim3opt_frames_set_options(s._b, L.C.byref(o)) == L.ERR_ARG
    # a consumer or an extractor handed no store, or an unfilled one: refused before anything else is looked at
    t, p, m, b = L.VocabularyTrainer(), L.PlaceBatch(), L.MatchBatch(), L.SurfBatch()
    assert lib.sim3opt_vocabulary_set_frames_from(t._b, None) == L.ERR_ARG
    assert lib.sim3opt_vocabulary_last_error(t._b) == b"vocabulary_set_frames_from: NULL store"
    assert lib.sim3opt_place_batch_set_frames_from(p._b, s._b) == L.ERR_STATE
    assert lib.sim3opt_place_batch_last_error(p._b) == b"place_batch_set_frames_from: the store is not filled"
    assert lib.sim3opt_match_batch_set_frames_from(m._b, None, 1, None, None, None, 1.0, 0.0, 0.0, 8, 8) == L.ERR_ARG
    assert lib.sim3opt_surf_batch_solve_into(b._b, None) == L.ERR_ARG
    assert lib.sim3opt_surf_batch_last_error(b._b) == b"surf_batch_solve_into: NULL store"
    assert L.device_memory_in_use() == before
    for h in (s, t, p, m, b):
        h.close()
