"""The references of the bundle-adjustment covariance tests against each other, on the host: the long-double
restatement of the Schur route (tests/ba_cov_ref.py) equals the definition -- the dense inverse -- on every accuracy
scene by the comparison rule the GPU test uses, every named defect of the restatement is noticed by that rule on at
least one scene, and the scenes meet the conditions they exist for."""
import numpy as np
import pytest

import ba_cov_cases as CC
import ba_cov_ref as CR

_defs = {}


def definition(name, lam):
    if (name, lam) not in _defs:
        _defs[(name, lam)] = CR.Definition(CC.problem(name), lam)
    return _defs[(name, lam)]


def test_scenes_meet_their_conditions():
    P = CC.problem("cov_tracks")
    CC.check_tracks(P)
    assert (P.cams.shape[0], P.points.shape[0]) == (12, 60) and P.fixed[:2].all() and P.fixed.sum() == 2
    Q = CC.problem("cov_small")
    assert (Q.cams.shape[0], Q.points.shape[0]) == (6, 30)
    assert sorted(set(np.bincount(Q.op).tolist())) == sorted(CC.SMALL_LENGTHS)
    # lists is singular at lambda = 0 (a point seen once), the track scenes are not
    assert CR.point_pivot_fails(CC.problem("lists"), 0.0) and not CR.point_pivot_fails(CC.problem("lists"), 1.0)
    assert not CR.point_pivot_fails(P, 0.0) and not CR.point_pivot_fails(Q, 0.0)


@pytest.mark.parametrize("name,lam", CC.ACCURACY)
def test_restatement_equals_the_definition(name, lam):
    P = CC.problem(name)
    D = definition(name, lam)
    print(f"[ba-cov] {name} lambda={lam:g}: n {D.n}, cond2 of the equilibrated system {D.cond:.3e}, bound {D.bound:.2e}")
    assert D.bound < 1e-3  # the comparison rule's condition on its inputs
    cam_pairs, points, pc = CC.requests(P)
    cc, pp, pcb = CR.restate(P, lam, cam_pairs, points, pc)
    w = D.worst(cam_pairs, cc, points, pp, pc, pcb)
    print(f"[ba-cov] {name} lambda={lam:g}: worst block ratio of the restatement {w:.2e}")
    assert w <= 1e-3  # long double against long double: decades inside the bound


def test_every_defect_is_noticed():
    scenes = (("cov_small", 1.0), ("cov_small", 0.0), ("cov_tracks", 1.0))
    for defect in CR.DEFECTS:
        seen = []
        for name, lam in scenes:
            P = CC.problem(name)
            cam_pairs, points, pc = CC.requests(P)
            cc, pp, pcb = CR.restate(P, lam, cam_pairs, points, pc, defect=defect)
            seen.append(definition(name, lam).worst(cam_pairs, cc, points, pp, pc, pcb))
            if seen[-1] > 1.0:
                break
        print(f"[ba-cov] defect {defect}: ratios {['%.2e' % s for s in seen]}")
        assert max(seen) > 1.0, defect
