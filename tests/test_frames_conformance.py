"""tests/cxx/frames_conformance.cpp, the conformance program of include/sim3opt_frames.hpp (FrameStore) and of the
FrameStore overloads of SurfExtractorBatch, VocabularyTrainer, LoopDetectorBatch and LoopMatchBatch, compiled -Werror:
its host part (the refusals of the helper, of the C-ABI and of the overloads) needs no GPU; its run part takes the mixed
batch of tests/surf_cases.py through extract(store) and then every stage once from the store and once from host arrays,
and finds the two chains equal to the bit."""
import subprocess

import pytest

import surf_cases as SC
import test_pnp_ref as TP


def compile_conformance(tmp_path):
    return TP.compile_cxx(tmp_path, "frames_conformance")


def write_images(path):
    batch = SC.mixed_batch()
    n, h, w = batch.shape
    with open(path, "w") as f:
        f.write(f"{n} {w} {h}\n")
        for im in batch:
            for row in im:
                f.write(" ".join(str(int(v)) for v in row) + "\n")
    return n


def test_frames_conformance_host_part(tmp_path):
    exe = compile_conformance(tmp_path)
    r = subprocess.run([exe, "host"], capture_output=True, text=True)
    assert r.returncode == 0 and " 0 failed" in r.stdout, r.stdout + r.stderr


def test_frames_conformance_without_a_gpu_fails_loudly(tmp_path):
    """No CPU fallback: exit 3 and the library's message.  (With a GPU the run succeeds; the gpu test below looks at it.)"""
    import torch
    exe = compile_conformance(tmp_path)
    path = str(tmp_path / "images.txt")
    write_images(path)
    r = subprocess.run([exe, "run", path], capture_output=True, text=True)
    if torch.cuda.is_available():
        assert r.returncode == 0, r.stdout + r.stderr
    else:
        assert r.returncode == 3 and "no usable HIP device" in r.stderr, r.stdout + r.stderr


@pytest.mark.gpu
def test_frames_conformance_run(tmp_path):
    exe = compile_conformance(tmp_path)
    path = str(tmp_path / "images.txt")
    n = write_images(path)
    r = subprocess.run([exe, "run", path], capture_output=True, text=True)
    assert r.returncode == 0 and " 0 failed" in r.stdout, r.stdout + r.stderr
    assert f"{n} images, " in r.stdout, r.stdout
