"""Gauss-Newton and dogleg options, host side (no GPU): g2o's defaults, the C-ABI's range checks, the Python mirror
of the new structs, and the host part of the g2o-named shim (tests/cxx/algorithms_conformance.cpp)."""
import ctypes as C
import math
import os
import subprocess

import pytest

from sim3opt_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_version_and_constants():
    assert hasattr(L.load(), "sim3opt_get_trust_region_stats")
    assert (L.ALGORITHM_LM, L.ALGORITHM_GAUSS_NEWTON, L.ALGORITHM_DOGLEG) == (0, 1, 2)
    assert (L.STEP_UNDEFINED, L.STEP_SD, L.STEP_GN, L.STEP_DL) == (0, 1, 2, 3)  # g2o's numbering
    assert C.sizeof(L.TrustRegionStats) == 6 * 8 + 2 * 4


def test_defaults_are_g2os():
    o = L.default_options()
    assert o.algorithm == L.ALGORITHM_LM
    assert o.dl_delta_init == 1e4 and o.dl_max_trials == 100
    assert o.dl_lambda_init == 1e-7 and o.dl_lambda_factor == 10.0
    # the new fields sit at the end of the struct, after an unchanged prefix, with explicit alignment
    assert L.Options.algorithm.offset == L.Options.jacobians.offset + 4
    assert L.Options.dl_delta_init.offset % 8 == 0 and C.sizeof(L.Options) % 8 == 0


def test_options_round_trip():
    G = L.Graph(algorithm=L.ALGORITHM_DOGLEG, dl_delta_init=0.25, dl_max_trials=7, dl_lambda_init=1e-4,
                dl_lambda_factor=3.0)
    o = G.options()
    assert (o.algorithm, o.dl_delta_init, o.dl_max_trials, o.dl_lambda_init, o.dl_lambda_factor) == \
        (2, 0.25, 7, 1e-4, 3.0)
    G.set_options(algorithm=L.ALGORITHM_GAUSS_NEWTON)
    assert G.options().algorithm == 1 and G.options().dl_delta_init == 0.25
    G.close()


@pytest.mark.parametrize("field,value", [
    ("algorithm", 3), ("algorithm", -1),
    ("dl_delta_init", 0.0), ("dl_delta_init", -1.0), ("dl_delta_init", math.inf), ("dl_delta_init", math.nan),
    ("dl_lambda_init", 0.0), ("dl_lambda_init", math.inf), ("dl_lambda_init", math.nan),
    ("dl_lambda_factor", 0.0), ("dl_lambda_factor", -10.0), ("dl_lambda_factor", math.inf),
    ("dl_max_trials", 0),
])
def test_set_options_refuses_bad_values(field, value):
    G = L.Graph()
    before = G.options()
    with pytest.raises(L.Sim3OptError) as ei:
        G.set_options(**{field: value})
    assert ei.value.code == L.ERR_ARG
    after = G.options()
    assert all(getattr(after, f) == getattr(before, f) for f in
               ("algorithm", "dl_delta_init", "dl_max_trials", "dl_lambda_init", "dl_lambda_factor"))
    G.close()


def test_trust_region_stats_without_a_dogleg_run():
    G = L.Graph()
    st = L.TrustRegionStats()
    assert L.load().sim3opt_get_trust_region_stats(G._g, 0, C.byref(st)) == L.ERR_STATE
    assert G.trust_region_stats() == []
    G.close()


def compile_program(tmp_path):
    exe = str(tmp_path / "algorithms_conformance")
    libdir = os.path.join(ROOT, "sim3opt_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-DSIM3OPT_G2O_NAMES",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "mock_eigen"),
                           os.path.join(ROOT, "tests", "cxx", "algorithms_conformance.cpp"), "-L" + libdir,
                           "-lsim3opt", "-Wl,-rpath," + libdir, "-o", exe])
    return exe


def test_algorithm_shim_host_part(tmp_path):
    r = subprocess.run([compile_program(tmp_path), "host"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout
