"""The device memory of TrackBatch: everything goes back at close(), and the stage run on poisoned device memory with
guarded block tails (sim3opt_debug_device_memory; tests/test_gpu_stale_memory.py's method) gives the bytes of a plain
run with no overwritten tail -- no kernel reads a block before its owner wrote it, none writes past what was asked for."""
import gc

import numpy as np
import pytest

from sim3opt_amd import lib as L
import track_cases as TC
from test_gpu_stale_memory import held, three_runs

pytestmark = pytest.mark.gpu


def solve_all(T, c):
    fr, mt, cam, camkw = TC.arrays(c)
    T.set_frames(*fr)
    T.set_matches(**mt)
    T.set_cameras(*cam, **camkw)
    return [("solve", T.solve()), ("dims", T.dims()), ("tracks", T.tracks()), ("points", T.points()),
            ("ba_rows", T.ba_rows(point_base=3))]


def test_everything_goes_back_at_close():
    gc.collect()
    L.release_device_cache()
    start = L.device_memory_in_use()
    T = L.TrackBatch(device=0)
    a = solve_all(T, TC.mixed())
    during = L.device_memory_in_use()
    assert during[0] > start[0] and during[1] > start[1]
    assert solve_all(T, TC.mixed())[0] == a[0] and L.device_memory_in_use() == during  # the same sizes: the same blocks
    solve_all(T, TC.segments((7, 9, 65, 257)))  # another size: the work blocks are made anew, none is left behind
    S = L.FrameStore(device=0)
    c = TC.mixed()
    S.set(c["kp_ptr"], c["kp"], np.ones((len(c["kp"]), 64), dtype=np.float32))
    T.set_frames_from(S)
    S.close()
    T.close()
    assert L.device_memory_in_use() == start


@pytest.mark.parametrize("make", [TC.mixed, lambda: TC.geometry()[1], lambda: TC.segments((7, 9, 65, 257)),
                                  lambda: TC.one_to_one(TC.SCAN_TILE + 1), lambda: TC.path("bit_reversed")],
                         ids=["mixed", "gate", "segments", "scan_carry", "path"])
def test_poisoned_memory_and_guarded_tails(make):
    c = make()

    def scenario():
        T = L.TrackBatch(**c["options"])
        rec = solve_all(T, c)
        held()
        rec += [("again", T.solve()), ("tracks_again", T.tracks()), ("points_again", T.points())]
        T.close()
        return rec

    three_runs("track_batch_" + c["name"], scenario)
