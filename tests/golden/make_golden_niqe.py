#!/usr/bin/env python
"""Record tests/golden/niqe.json / niqe.npz from the reference's own ``calculate_niqe``.

    python tests/golden/make_golden_niqe.py <reference checkout>/Train

Nothing of the reference is restated here: ``basicsr.metrics.niqe.calculate_niqe`` is imported and called (from
inside ``<Train>``, where its relative ``basicsr/metrics/niqe_pris_params.npz`` resolves) with scipy's own
``convolve`` and ``gamma``.  Its module-level ``compute_feature`` is wrapped by a spy that hands every block on
unchanged and keeps the block and the 18 features that come back; the two MSCN fields are put together again from
the blocks, so the features and the fields recorded are the ones the reference itself formed.

Modules that are not installed get inert stand-ins as in make_golden_metrics.py.  cv2 is among them here, and one
stand-in is not inert, because ``niqe`` calls it: ``cv2.resize(img, (w // 2, h // 2), interpolation=INTER_LINEAR)``
is tests/niqe_oracle.py::half's 2 x 2 mean, OpenCV's DOCUMENTED semantics at exactly one half on even sizes, not
measured ones: the goldens leave PARITY UNPINNED AGAINST REAL cv2, and the json says which route recorded it.

Inputs are the seeded cases of tests/niqe_oracle.py (RGB [C, H, W]; the reference gets them as BGR with
``input_order='CHW'``, uint8 cases quantised the way tensor2img does).  Recorded per case: the score, the
[blocks, 36] features, sha256 of both fields, the argmin margin of the oracle, and the gaps between the reference
and the oracle's float64 mode (score: absolute; features: largest |difference| / max(|reference|, 0.01)).
Both fields are compared bit for bit with the oracle's before anything is written.  Also recorded: the score
tolerance of the GPU test, 8 x the worst score change under a seeded 1e-11 relative perturbation of the moments.
"""
import hashlib
import importlib
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
from make_golden_metrics import _Inert, _InertFinder  # noqa: E402
from tests import niqe_oracle as no  # noqa: E402

FEATURE_FLOOR = 0.01


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float32).tobytes()).hexdigest()


def feature_gap(ref, got):
    if not np.array_equal(np.isnan(ref), np.isnan(got)):
        return float("inf")
    ok = ~np.isnan(ref)
    return float(np.max(np.abs(ref[ok] - got[ok]) / np.maximum(np.abs(ref[ok]), FEATURE_FLOOR)))


def main():
    train_dir = os.path.abspath(sys.argv[1])
    missing = []
    for root in ("cv2", "skimage", "lmdb", "tqdm", "yaml", "torchvision", "tensorboard", "requests", "einops",
                 "natsort"):
        try:
            importlib.import_module(root)
        except Exception:
            missing.append(root)
    sys.meta_path.append(_InertFinder(missing))
    import cv2
    if "cv2" in missing:
        assert isinstance(cv2, _Inert)
        cv2.INTER_LINEAR = 1

        def resize(img, dsize, interpolation=None):
            assert interpolation == cv2.INTER_LINEAR and img.dtype == np.float32
            assert dsize == (img.shape[1] // 2, img.shape[0] // 2) and img.shape[0] % 2 == 0 and img.shape[1] % 2 == 0
            h = (img[:, 0::2] + img[:, 1::2]) * np.float32(0.5)
            return (h[0::2] + h[1::2]) * np.float32(0.5)
        cv2.resize = resize
    sys.path.insert(0, train_dir)
    os.chdir(train_dir)
    warnings.simplefilter("ignore")
    import scipy
    nq = importlib.import_module("basicsr.metrics.niqe")

    seen = []
    inner = nq.compute_feature

    def spy(block):
        feat = inner(block)
        seen.append((np.array(block, dtype=np.float32), [float(v) for v in feat]))
        return feat
    nq.compute_feature = spy

    p = no.params(os.path.join(train_dir, "basicsr", "metrics", "niqe_pris_params.npz"))
    items = dict(no.cases())
    for i, x in enumerate(no.batch()):
        items[f"batch3_{i}"] = (x, 0, False)
    meta = {"source": "basicsr.metrics.niqe.calculate_niqe(img BGR, crop_border, input_order='CHW', convert_to='y')",
            "scipy": scipy.__version__, "numpy": np.__version__,
            "cv2": "numpy stand-in for resize (documented semantics; parity unpinned against real cv2)"
            if "cv2" in missing else "real cv2 " + str(getattr(cv2, "__version__", "")),
            "stand_ins": missing, "feature_floor": FEATURE_FLOOR, "cases": {}}
    arrays = {}
    for name, (x, cb, use_image) in items.items():
        img = no.to_uint8(x).astype(np.uint8) if use_image else x
        del seen[:]
        with np.errstate(all="ignore"):
            ref = float(np.asarray(nq.calculate_niqe(np.ascontiguousarray(img[::-1]), cb, input_order="CHW",
                                                     convert_to="y")).reshape(-1)[0])
        Hc, Wc = ((s - 2 * cb) // 96 * 96 for s in x.shape[1:])
        nblk = (Hc // 96) * (Wc // 96)
        assert len(seen) == 2 * nblk
        ref_fields, feats = [], []
        for scale in (1, 2):
            part = seen[(scale - 1) * nblk:scale * nblk]
            f = np.zeros((Hc // scale, Wc // scale), dtype=np.float32)
            grid, bs = no.block_grid(f.shape, scale)
            for (y0, x0), (blk, _) in zip(grid, part):
                f[y0:y0 + bs, x0:x0 + bs] = blk
            ref_fields.append(f)
            feats.append(np.array([ft for _, ft in part], dtype=np.float64))
        ref_feat = np.concatenate(feats, axis=1)
        s64, feat64, (f1, f2), margin = no.niqe(x, cb, use_image, p, "float64", detail=True)
        for f, g, tag in ((ref_fields[0], f1, "scale 1"), (ref_fields[1], f2, "scale 2")):
            if f.tobytes() != np.ascontiguousarray(g).tobytes():
                raise SystemExit(f"{name}: the oracle's {tag} field differs from the reference's in "
                                 f"{int((f != g).sum())} of {f.size} entries: nothing written")
        rec = {"crop_border": cb, "use_image": use_image, "niqe": repr(ref), "blocks": nblk,
               "field_sha256": [digest(ref_fields[0]), digest(ref_fields[1])],
               "score_gap_to_float64": repr(abs(ref - s64)), "feature_gap_to_float64": repr(feature_gap(ref_feat, feat64)),
               "oracle_float64": repr(s64), "argmin_margin": repr(float(margin))}
        meta["cases"][name] = rec
        arrays[name] = ref_feat
        print(name, rec)
    worst = max(no.perturbed_score_change(name) for name in no.cases())
    meta["perturbation"] = {"relative": 1e-11, "seed": 7, "worst_score_change": repr(worst),
                            "gpu_score_tolerance": repr(8.0 * worst)}
    print(meta["perturbation"])
    np.savez_compressed(os.path.join(HERE, "niqe.npz"), **arrays)
    with open(os.path.join(HERE, "niqe.json"), "w") as f:
        json.dump(meta, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
