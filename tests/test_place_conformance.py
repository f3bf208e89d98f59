"""tests/cxx/place_conformance.cpp, the conformance program of include/sim3opt_place.hpp (LoopDetectorBatch), compiled
-Werror: its host part (argument refusals of the helper and the C-ABI) needs no GPU; its run part takes the planted
revisit through detect() and feed(LoopMatchBatch) and gets the restatement's status and match for every keyframe.  And
tests/cxx/place_host_driver.cpp: the vocabulary validation with every message as an exact string, the breadth-first
renumbering and the temporal recurrence (csrc/place_host.hpp) as a stand-alone program under AddressSanitizer +
UndefinedBehaviorSanitizer on the CPU."""
import os
import subprocess

import pytest

import place_cases as PCS
import place_ref as PR
import test_pnp_ref as TP
from test_devmem_owners import SAN
from test_example_cpp import ROOT


def compile_conformance(tmp_path):
    return TP.compile_cxx(tmp_path, "place_conformance")


def write_conformance_file(path, n_frames=None):
    """The chain case of tests/place_cases.py (the planted revisit with pixels and depths), cut to its first n_frames,
    and what the restatement says of every keyframe."""
    case = PCS.chain_case()
    voc, ptr = case["voc"], case["kp_ptr"]
    n = len(ptr) - 1 if n_frames is None else n_frames
    R = PR.detect(voc, ptr[:n + 1], case["desc"][:ptr[n]])
    num = lambda a: " ".join(repr(float(x)) for x in a)
    with open(path, "w") as f:
        f.write(f"{len(voc.parent)} {n}\n")
        for i in range(len(voc.parent)):
            f.write(f"{voc.parent[i]} {voc.word_id[i]} {float(voc.weight[i])!r} {num(voc.centre[i])}\n")
        for k in range(n):
            f.write(f"{ptr[k + 1] - ptr[k]}\n")
            for r in range(ptr[k], ptr[k + 1]):
                f.write(f"{num(case['kp'][r])} {float(case['obs_depth'][r])!r} {num(case['desc'][r])}\n")
        for k in range(n):
            f.write(f"{R.status[k]} {R.match[k]}\n")
    return R


def test_place_conformance_host_part(tmp_path):
    exe = compile_conformance(tmp_path)
    r = subprocess.run([exe, "host"], capture_output=True, text=True)
    assert r.returncode == 0 and " 0 failed" in r.stdout, r.stdout + r.stderr


def test_place_conformance_without_a_gpu_fails_loudly(tmp_path):
    """No CPU fallback: exit 3 and the library's message.  (With a GPU the run succeeds; the gpu test below looks at it.)"""
    import torch
    exe = compile_conformance(tmp_path)
    path = str(tmp_path / "keyframes.txt")
    write_conformance_file(path, 24)
    r = subprocess.run([exe, "run", path], capture_output=True, text=True)
    if torch.cuda.is_available():
        assert r.returncode == 0, r.stdout + r.stderr
    else:
        assert r.returncode == 3 and "no usable HIP device" in r.stderr, r.stdout + r.stderr


@pytest.mark.gpu
def test_place_conformance_run(tmp_path):
    exe = compile_conformance(tmp_path)
    path = str(tmp_path / "keyframes.txt")
    R = write_conformance_file(path)
    assert len(R.pairs) >= 9
    r = subprocess.run([exe, "run", path], capture_output=True, text=True)
    assert r.returncode == 0 and " 0 failed" in r.stdout and f"{len(R.pairs)} candidates" in r.stdout, r.stdout + r.stderr


def test_host_checks_and_temporal_window_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "place_host_san")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + SAN +
                          [os.path.join(ROOT, "tests", "cxx", "place_host_driver.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.strip().endswith("place host ok"), r.stdout[-2000:]
