"""tests/cxx/surf_conformance.cpp, the conformance program of include/sim3opt_surf.hpp (SurfExtractorBatch), compiled
-Werror: its host part (argument refusals of the helper and of the C-ABI, the host restatement) needs no GPU; its run
part takes the mixed batch of tests/surf_cases.py through add() and extract(), gets the library's restatement of every
image to the bit and hands kp_ptr / desc to a VocabularyTrainer and a LoopDetectorBatch.  And
tests/cxx/surf_host_driver.cpp: every refusal message as an exact string, the tables, the pattern resizing, the solve,
the angle functions and the serial restatement on small images (csrc/surf_host.hpp) as a stand-alone program under
AddressSanitizer + UndefinedBehaviorSanitizer on the CPU."""
import os
import subprocess

import pytest

import surf_cases as SC
import test_pnp_ref as TP
from sim3opt_amd import lib as L
from test_devmem_owners import SAN
from test_example_cpp import ROOT


def compile_conformance(tmp_path):
    return TP.compile_cxx(tmp_path, "surf_conformance")


def write_conformance_file(path):
    """The mixed batch and what the library's restatement finds in every image of it."""
    batch = SC.mixed_batch()
    n, h, w = batch.shape
    total = 0
    with open(path, "w") as f:
        f.write(f"{n} {w} {h}\n")
        for im in batch:
            for row in im:
                f.write(" ".join(str(int(v)) for v in row) + "\n")
        for im in batch:
            r = L.SurfBatch.reference_image(im)
            f.write(f"{len(r['size'])}\n")
            total += len(r["size"])
            for k in range(len(r["size"])):
                head = [r["kp"][k, 0], r["kp"][k, 1], r["size"][k], r["angle"][k], r["response"][k]]
                f.write(" ".join(repr(float(x)) for x in head) + f" {r['octave'][k]} {r['laplacian'][k]} " +
                        " ".join(repr(float(x)) for x in r["desc"][k]) + "\n")
    return n, total


def test_surf_conformance_host_part(tmp_path):
    exe = compile_conformance(tmp_path)
    r = subprocess.run([exe, "host"], capture_output=True, text=True)
    assert r.returncode == 0 and " 0 failed" in r.stdout, r.stdout + r.stderr


def test_surf_conformance_without_a_gpu_fails_loudly(tmp_path):
    """No CPU fallback: exit 3 and the library's message.  (With a GPU the run succeeds; the gpu test below looks at it.)"""
    import torch
    exe = compile_conformance(tmp_path)
    path = str(tmp_path / "images.txt")
    write_conformance_file(path)
    r = subprocess.run([exe, "run", path], capture_output=True, text=True)
    if torch.cuda.is_available():
        assert r.returncode == 0, r.stdout + r.stderr
    else:
        assert r.returncode == 3 and "no usable HIP device" in r.stderr, r.stdout + r.stderr


@pytest.mark.gpu
def test_surf_conformance_run(tmp_path):
    exe = compile_conformance(tmp_path)
    path = str(tmp_path / "images.txt")
    n, total = write_conformance_file(path)
    r = subprocess.run([exe, "run", path], capture_output=True, text=True)
    assert r.returncode == 0 and " 0 failed" in r.stdout, r.stdout + r.stderr
    assert f"{n} images, {total} keypoints" in r.stdout and total > 100, r.stdout


def test_host_checks_tables_and_restatement_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "surf_host_san")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + SAN +
                          [os.path.join(ROOT, "tests", "cxx", "surf_host_driver.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.strip().endswith("surf host ok"), r.stdout[-2000:]
