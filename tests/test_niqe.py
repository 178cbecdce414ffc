"""tests/niqe_oracle.py against numbers recorded from the reference's own ``calculate_niqe``
(tests/golden/niqe.json / .npz, written by tests/golden/make_golden_niqe.py), ``metrics.finish_niqe`` against the
oracle, and the conditions the GPU test (tests/test_niqe_gpu.py) relies on.  CPU only, no scipy.

Bars:
* ``like_reference`` mode against the recorded score and features: 8 x the gap between the reference and the
  oracle's float64 mode measured at recording, floor 1e-9 relative (features: relative to max(|value|, 0.01));
* the MSCN fields: bit for bit (sha256);
* ``finish_niqe`` on the oracle's moments against the oracle's float64 score: 1e-12 relative;
* the GPU test's score tolerance is the recorded 8 x (worst score change under a 1e-11 relative perturbation of
  the moments); the inputs' argmin margins must exceed 1e-9, a hundred times that perturbation, so that no
  alpha can flip within it;
* every mutant moves a quantity the GPU test compares by more than ten of its tolerances.
"""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

from rethink_acoustic_image_enhancement_amd import metrics
from tests import niqe_oracle as no

META = json.load(open(os.path.join(no.GOLDEN, "niqe.json")))
FEATS = np.load(os.path.join(no.GOLDEN, "niqe.npz"))
SUM_TOL = 1e-11
SCORE_TOL = float(META["perturbation"]["gpu_score_tolerance"])
MARGIN = 1e-9


def _items():
    items = dict(no.cases())
    for i, x in enumerate(no.batch()):
        items[f"batch3_{i}"] = (x, 0, False)
    return items


def test_recorded_cases_are_the_oracles_cases():
    assert sorted(META["cases"]) == sorted(_items())
    for name, (x, cb, use_image) in _items().items():
        rec = META["cases"][name]
        assert rec["crop_border"] == cb and rec["use_image"] == use_image
    assert "unpinned" in META["cv2"]


@pytest.mark.parametrize("name", sorted(META["cases"]))
def test_like_reference_mode_reproduces_the_recorded_numbers(name):
    x, cb, use_image = _items()[name]
    rec = META["cases"][name]
    s, feat, (f1, f2), _ = no.niqe(x, cb, use_image, mode="like_reference", detail=True)
    for f, want in zip((f1, f2), rec["field_sha256"]):
        assert f.dtype == np.float32
        assert hashlib.sha256(np.ascontiguousarray(f).tobytes()).hexdigest() == want
    ref_s, ref_f = float(rec["niqe"]), FEATS[name]
    tol_s = max(8.0 * float(rec["score_gap_to_float64"]), 1e-9 * abs(ref_s))
    tol_f = max(8.0 * float(rec["feature_gap_to_float64"]), 1e-9)
    print(f"{name}: score {s!r} vs {ref_s!r} (tol {tol_s:.3e})")
    assert abs(s - ref_s) <= tol_s
    assert feat.shape == ref_f.shape == (rec["blocks"], 36)
    assert np.array_equal(np.isnan(feat), np.isnan(ref_f))
    ok = ~np.isnan(ref_f)
    err = np.abs(feat[ok] - ref_f[ok]) / np.maximum(np.abs(ref_f[ok]), META["feature_floor"])
    print(f"{name}: worst feature error {err.max():.3e} (tol {tol_f:.3e})")
    assert err.max() <= tol_f


@pytest.mark.parametrize("name", sorted(no.cases()))
def test_finish_niqe_on_the_oracles_moments(name):
    s, feat, _, margin, (m1, m2) = no.reference(name)
    assert abs(s - float(META["cases"][name]["oracle_float64"])) <= 1e-12 * abs(s)
    got = metrics.finish_niqe(np.stack([m1, m2]), no.params())
    assert isinstance(got, float) and abs(got - s) <= 1e-12 * abs(s)
    both = metrics.finish_niqe(np.stack([np.stack([m1, m2])] * 2), no.params())
    assert both.shape == (2,) and both[0] == got and both[1] == got
    # the condition on the inputs: no argmin within reach of the perturbation
    print(f"{name}: argmin margin {margin:.3e}")
    assert margin > MARGIN


def test_sonar_case_has_a_block_without_features():
    for name in ("sonar_c1_200x300_cb0", "sonar_c1_200x300_cb4"):
        _, feat, (f1, f2), _, (m1, m2) = no.reference(name)
        assert not f1[:96, :96].any() and not f2[:48, :48].any()
        assert (m1[0, :, :2] == 0).all() and (m2[0, :, :2] == 0).all()
        bad = np.isnan(feat).any(axis=1)
        assert bad[0] and bad.sum() == 1
        assert feat[0, 0] == 0.2   # np.argmin over NaNs: the first table entry, which the nanmean then includes


def test_fewer_than_two_complete_blocks_give_nan():
    _, _, _, _, (m1, m2) = no.reference("noise_c1_192x96")
    one = np.stack([m1[:1], m2[:1]])
    assert np.isnan(metrics.finish_niqe(one, no.params()))
    assert np.isnan(no.score_from_moments(m1[:1], m2[:1], no.params()))
    _, _, _, _, (s1, s2) = no.reference("sonar_c1_200x300_cb0")
    assert np.isnan(metrics.finish_niqe(np.stack([s1[:2], s2[:2]]), no.params()))   # one of the two is the empty block


def test_recorded_score_tolerance_is_the_measured_one():
    worst = max(no.perturbed_score_change(name) for name in no.cases())
    print(f"worst score change under a 1e-11 perturbation: {worst:.3e}; recorded tolerance {SCORE_TOL:.3e}")
    assert 0 < 8.0 * worst <= 2.0 * SCORE_TOL and SCORE_TOL <= 16.0 * 8.0 * worst
    assert SCORE_TOL < 1e-6


# ------------------------------------------------------------------ mutants
MUTANT_CASE = {"clamp_storage": "sonar_c1_200x300_cb0", "crop_ignored": "sonar_c1_200x300_cb4",
               "roll_nowrap": "noise_c1_192x96", "shift_sign": "noise_c1_192x96",
               "block_order": "sat_c3_200x300_cb4_u8", "products_fp64": "noise_c3_192x96",
               "zeros_positive": "sonar_c1_200x300_cb0", "abs_nonzero": "sonar_c1_200x300_cb0",
               "scale2_unscaled": "ramp_c3_192x192_u8", "scale2_block96": "sat_c1_192x192_u8"}


def _moved(name, mutant):
    """By how many tolerances the mutant moves what the GPU test compares (inf where the bar is exact)."""
    x, cb, use_image = no.cases()[name]
    s, _, (f1, f2), _, (m1, m2) = no.reference(name)
    ms, _, (g1, g2), _ = no.niqe(x, cb, use_image, mutant=mutant, detail=True)
    moved = {"field": 0.0, "count": 0.0, "sum": 0.0, "score": abs(ms - s) / SCORE_TOL if ms == ms else np.inf}
    for f, g in ((f1, g1), (f2, g2)):
        if f.shape != g.shape or f.tobytes() != np.ascontiguousarray(g).tobytes():
            moved["field"] = np.inf
    for scale, m, g in ((1, m1, g1), (2, m2, g2)):
        q = no.moments(g, scale, mutant)
        if q.shape != m.shape:
            moved["count"] = np.inf
            continue
        if not np.array_equal(q[..., :2], m[..., :2]):
            moved["count"] = np.inf
        with np.errstate(all="ignore"):
            rel = np.abs(q[..., 2:] - m[..., 2:]) / (SUM_TOL * m[..., 2:])
        moved["sum"] = max(moved["sum"], float(np.nanmax(rel)))
    return moved


@pytest.mark.parametrize("mutant", no.MUTANTS)
def test_each_mutant_moves_a_compared_quantity_by_more_than_ten_tolerances(mutant):
    assert sorted(MUTANT_CASE) == sorted(no.MUTANTS)
    moved = _moved(MUTANT_CASE[mutant], mutant)
    print(mutant, moved)
    assert max(moved.values()) > 10.0
