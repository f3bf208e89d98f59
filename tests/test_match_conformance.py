"""tests/cxx/match_conformance.cpp, the conformance program of include/sim3opt_match.hpp (LoopMatchBatch), compiled
-Werror: its host part (argument refusals of the helper and the C-ABI) needs no GPU; its run part takes planted
matches through match -> PnP -> two-view refinement and recovers the planted pose and depth ratio.  And
tests/cxx/match_host_driver.cpp: the host-side checks and the tile-table builder (csrc/match_host.hpp) as a
stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer on the CPU."""
import os
import subprocess

import numpy as np
import pytest

import pnp_cases as PC
import test_pnp_ref as TP
from oracle import ba_oracle as BO
from test_devmem_owners import SAN
from test_example_cpp import ROOT

W, H = 1241, 376
CASES = ((300, 31, 1.0), (90, 32, 1.7), (513, 33, 0.6))  # (points, seed of pnp_cases.make_case, scale of keyframe 1's map)


def compile_conformance(tmp_path):
    return TP.compile_cxx(tmp_path, "match_conformance")


def write_conformance_file(path, cases):
    """Noise-free planted candidates: a point's pixel and depth in either keyframe (keyframe 1's depths times the
    candidate's scale), whether the border and skew filters keep the match, the expected sloop, camera 1's pose; the
    bounds tests/test_pnp_ref.py holds the PnP -> refinement chain to in the first line."""
    f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
    with open(path, "w") as f:
        w = lambda *v: f.write(" ".join(repr(float(x)) if not isinstance(x, (int, np.integer)) else str(x)
                                        for x in v) + "\n")
        w(len(cases), PC.FOCAL, PC.CX, PC.CY, W, H, TP.REFINED_ROT, TP.REFINED_T)
        for n, seed, scale in cases:
            case = PC.make_case(n, seed)
            P, cam1 = case["points"], case["cam1_true"]
            R1, t1 = BO.quat_to_R(cam1[None, :4])[0], cam1[4:]
            X1 = P @ R1.T + t1
            a, b = f32(PC._project(np.eye(3), np.zeros(3), P)), f32(PC._project(R1, t1, P))
            z0, z1 = f32(P[:, 2]), f32(scale * X1[:, 2])
            kept = (np.abs(b[:, 0] - a[:, 0]) < (1.0 / 3.0) * W) & (np.abs(b[:, 1] - a[:, 1]) < (1.0 / 4.0) * H)
            for uv in (a, b):
                kept &= (uv[:, 0] >= 0.1 * W) & (uv[:, 0] <= (1 - 0.1) * W) & (uv[:, 1] >= 0.1 * H) & \
                    (uv[:, 1] <= (1 - 0.1) * H)
            assert kept.sum() > 40
            mid = int(0.5 * kept.sum())
            w(n, float(np.sort(z1[kept])[mid]) / float(np.sort(z0[kept])[mid]))
            for i in range(n):
                w(*a[i], z0[i], *b[i], z1[i], int(kept[i]))
            w(*cam1)


def test_match_conformance_host_part(tmp_path):
    exe = compile_conformance(tmp_path)
    r = subprocess.run([exe, "host"], capture_output=True, text=True)
    assert r.returncode == 0 and " 0 failed" in r.stdout, r.stdout + r.stderr


def test_match_conformance_without_a_gpu_fails_loudly(tmp_path):
    """No CPU fallback: exit 3 and the library's message.  (With a GPU the run succeeds; the gpu test below looks at it.)"""
    import torch
    exe = compile_conformance(tmp_path)
    path = str(tmp_path / "candidates.txt")
    write_conformance_file(path, CASES[1:2])
    r = subprocess.run([exe, "run", path], capture_output=True, text=True)
    if torch.cuda.is_available():
        assert r.returncode == 0, r.stdout + r.stderr
    else:
        assert r.returncode == 3 and "no usable HIP device" in r.stderr, r.stdout + r.stderr


@pytest.mark.gpu
def test_match_conformance_chain(tmp_path):
    exe = compile_conformance(tmp_path)
    path = str(tmp_path / "candidates.txt")
    write_conformance_file(path, CASES)
    r = subprocess.run([exe, "run", path], capture_output=True, text=True)
    assert r.returncode == 0 and " 0 failed" in r.stdout and f"{len(CASES)} candidates" in r.stdout, r.stdout + r.stderr


def test_host_checks_and_tile_table_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "match_host_san")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + SAN +
                          [os.path.join(ROOT, "tests", "cxx", "match_host_driver.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.strip().endswith("match host ok"), r.stdout[-2000:]


def test_handle_host_frame_under_asan_ubsan(tmp_path):
    """csrc/handle_host.hpp -- all_finite, the two ragged-pointer checks with every message as an exact string, the guard
    of the C boundary -- and match_host.hpp's use of it, stand-alone (tests/cxx/handle_host_driver.cpp)."""
    exe = str(tmp_path / "handle_host_san")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + SAN +
                          [os.path.join(ROOT, "tests", "cxx", "handle_host_driver.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.strip().endswith("handle host ok"), r.stdout[-2000:]
