"""The exact lidar classifier (tests/lidar_scenes.py) against the CPU oracle, on every scene family at its decision boundaries.

Every CLEAR beam must show the classifier's one reading (to the f64 evaluation's rounding), every BAND beam one of its candidate
readings; every family must have beams of both kinds, so that a scene generator that drifts cannot quietly test nothing.
"""
import collections

import numpy as np
import pytest

import lidar_scenes as LS


@pytest.mark.parametrize("n_beams", [7, 16])
def test_classifier_agrees_with_the_oracle(oracle, n_beams):
    lay, hulls, scenes = LS.build_scenes(oracle, n_beams)
    cls = LS.classify_scenes(oracle, lay, hulls, scenes, n_beams)
    ref = LS.run_oracle(oracle, lay, scenes, n_beams, history=2)
    prev = np.full((len(scenes), n_beams), -1.0)  # models.py:36: lidar_vals start at -1
    cur = [LS.lidar_cols(ref["obs1"], n_beams, 2), LS.lidar_cols(ref["obs2"], n_beams, 2)]
    count, bad = collections.Counter(), []
    for step in (0, 1):
        pv = prev if step == 0 else cur[0]
        for e, s in enumerate(scenes):
            for i, (clear, cands) in enumerate(cls[e][step]):
                r = cur[step][e, i]
                if clear:
                    assert len(cands) == 1
                if not LS.accepts(cands, r, pv[e, i], tol=0.0 if clear else 1e-9):
                    bad.append((s.tag, step, i, clear, cands, r))
                if i == s.beam:
                    count[(s.family, clear)] += 1
    print({f: (count[(f, True)], count[(f, False)]) for f in LS.FAMILIES}, "(clear, band) target beams per family")
    assert not bad, bad[:10]
    for f in LS.FAMILIES:
        assert count[(f, True)] >= 10 and count[(f, False)] >= 10, (f, count[(f, True)], count[(f, False)])


def test_scene_geometry(oracle):
    """The layouts hold hulls of 3, 4, 5, 8, 9 and 12 planes on both sides; some origins sit exactly on the bank corners."""
    lay, hulls, scenes = LS.build_scenes(oracle, 10)
    for s in (0, 1):
        assert {h[s].count for h in hulls} >= {3, 4, 5, 8, 9, 12}
    lid = LS.Lidar(oracle, 10)
    on = collections.Counter(lid.origin(*sc.pose1) for sc in scenes if sc.family == "inside")
    assert on[(0.0, 0.0)] >= 4 and on[(LS.W, 0.0)] >= 4
    assert len(scenes) < 4096
