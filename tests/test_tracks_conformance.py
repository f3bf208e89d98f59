"""tests/cxx/tracks_conformance.cpp, the conformance program of include/sim3opt_tracks.hpp (LoopTrackBatch), compiled
-Werror: its host part (the refusals of the helper and of the C-ABI) needs no GPU; its run part takes the mixed batch of
tests/track_cases.py with planted poses through add_pair / solve / append_to on the device and finds tracks, statuses,
points and rows equal to the host restatement's to the bit."""
import subprocess

import pytest

import test_pnp_ref as TP
from test_track_ref import posed_mixed


def compile_conformance(tmp_path):
    return TP.compile_cxx(tmp_path, "tracks_conformance")


def write_case(path, c):
    with open(path, "w") as f:
        nf = len(c["kp_ptr"]) - 1
        f.write(f"{nf} {c['focal']!r} {c['cx']!r} {c['cy']!r} {c['options'].get('max_reproj_px', 0.0)!r}\n")
        for i in range(nf):
            f.write(f"{c['kp_ptr'][i + 1] - c['kp_ptr'][i]} " + " ".join(repr(float(v)) for v in c["states"][i]) + "\n")
        for u, v in c["kp"]:
            f.write(f"{float(u)!r} {float(v)!r}\n")
        f.write(f"{len(c['pairs'])}\n")
        for p, (a, b) in enumerate(c["pairs"]):
            lo, hi = c["match_ptr"][p], c["match_ptr"][p + 1]
            f.write(f"{a} {b} {hi - lo}\n")
            for m in range(lo, hi):
                f.write(f"{c['query_idx'][m]} {c['train_idx'][m]} {float(c['depth0'][m])!r} {float(c['depth1'][m])!r} "
                        f"{c['mask'][m]}\n")
    return len(c["pairs"])


def test_tracks_conformance_host_part(tmp_path):
    exe = compile_conformance(tmp_path)
    r = subprocess.run([exe, "host"], capture_output=True, text=True)
    assert r.returncode == 0 and " 0 failed" in r.stdout, r.stdout + r.stderr


def test_tracks_conformance_without_a_gpu_fails_loudly(tmp_path):
    """No CPU fallback: exit 3 and the library's message.  (With a GPU the run succeeds; the gpu test below looks at it.)"""
    import torch
    exe = compile_conformance(tmp_path)
    path = str(tmp_path / "case.txt")
    write_case(path, posed_mixed())
    r = subprocess.run([exe, "run", path], capture_output=True, text=True)
    if torch.cuda.is_available():
        assert r.returncode == 0, r.stdout + r.stderr
    else:
        assert r.returncode == 3 and "no usable HIP device" in r.stderr, r.stdout + r.stderr


@pytest.mark.gpu
def test_tracks_conformance_run(tmp_path):
    exe = compile_conformance(tmp_path)
    path = str(tmp_path / "case.txt")
    n = write_case(path, posed_mixed())
    r = subprocess.run([exe, "run", path], capture_output=True, text=True)
    assert r.returncode == 0 and " 0 failed" in r.stdout, r.stdout + r.stderr
    assert f"{n} pairs, 24 matches, 10 tracks, " in r.stdout, r.stdout
