"""tests/cxx/vocabulary_conformance.cpp, the conformance program of include/sim3opt_vocabulary.hpp (VocabularyTrainer),
compiled -Werror: its host part (argument refusals of the helper and the C-ABI, save and load) needs no GPU; its run
part takes a case of tests/vocab_cases.py through create(features), gets the restatement's tree, saves, loads and feeds
it to a LoopDetectorBatch.  And tests/cxx/vocab_host_driver.cpp: every refusal message as an exact string, the tables of
a level, the assembly, the weights and the file with truncated and wrong-magic inputs (csrc/vocab_host.hpp) as a
stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer on the CPU."""
import os
import subprocess

import pytest

import test_pnp_ref as TP
import vocab_cases as VC
from test_devmem_owners import SAN
from test_example_cpp import ROOT


def compile_conformance(tmp_path):
    return TP.compile_cxx(tmp_path, "vocabulary_conformance")


def write_conformance_file(path, name="k2_L3"):
    """A case of tests/vocab_cases.py and the tree the restatement trains on it."""
    case = next(c for c in VC.all_cases() if c["name"] == name)
    R, ptr, o = VC.reference(name), case["kp_ptr"], case["options"]
    assert set(o) == {"k", "levels", "seed"}
    num = lambda a: " ".join(repr(float(x)) for x in a)
    with open(path, "w") as f:
        f.write(f"{len(ptr) - 1} {o['k']} {o['levels']} {o['seed']} {len(R.parent)}\n")
        for k in range(len(ptr) - 1):
            f.write(f"{ptr[k + 1] - ptr[k]}\n")
            for r in range(ptr[k], ptr[k + 1]):
                f.write(num(case["desc"][r]) + "\n")
        for i in range(len(R.parent)):
            f.write(f"{R.parent[i]} {R.word_id[i]} {float(R.weight[i])!r} {num(R.centre[i])}\n")
    return R


def test_vocabulary_conformance_host_part(tmp_path):
    exe = compile_conformance(tmp_path)
    r = subprocess.run([exe, "host", str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and " 0 failed" in r.stdout, r.stdout + r.stderr


def test_vocabulary_conformance_without_a_gpu_fails_loudly(tmp_path):
    """No CPU fallback: exit 3 and the library's message.  (With a GPU the run succeeds; the gpu test below looks at it.)"""
    import torch
    exe = compile_conformance(tmp_path)
    path = str(tmp_path / "images.txt")
    write_conformance_file(path)
    r = subprocess.run([exe, "run", path, str(tmp_path)], capture_output=True, text=True)
    if torch.cuda.is_available():
        assert r.returncode == 0, r.stdout + r.stderr
    else:
        assert r.returncode == 3 and "no usable HIP device" in r.stderr, r.stdout + r.stderr


@pytest.mark.gpu
def test_vocabulary_conformance_run(tmp_path):
    exe = compile_conformance(tmp_path)
    path = str(tmp_path / "images.txt")
    R = write_conformance_file(path)
    r = subprocess.run([exe, "run", path, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and " 0 failed" in r.stdout and f"{len(R.parent)} nodes" in r.stdout, r.stdout + r.stderr


def test_host_checks_assembly_and_file_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "vocab_host_san")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + SAN +
                          [os.path.join(ROOT, "tests", "cxx", "vocab_host_driver.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.strip().endswith("vocab host ok"), r.stdout[-2000:]
