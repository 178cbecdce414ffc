#!/usr/bin/env python
"""Record tests/golden/metrics_ssim.json from the reference's own SSIM functions.

    python tests/golden/make_golden_ssim.py <reference checkout>/Train

``basicsr`` numbers come from ``basicsr.metrics.psnr_ssim.calculate_ssim`` (-> ``_ssim_3d``), ``valid`` numbers
from ``calculate_ssim`` of ``Train/utils.py``; modules that are not installed get inert stand-ins as in
make_golden_metrics.py, so the reference functions themselves run.  Three stand-ins are not inert, because the
functions call them (listed under ``"stand_ins"`` in the file):

* ``cv2.getGaussianKernel(ksize, sigma)``: exp(-(i - (ksize - 1) / 2)^2 / (2 sigma^2)), normalised, float64,
  shape (ksize, 1), the documented formula;
* ``cv2.filter2D(src, -1, kernel)``: ``scipy.ndimage.correlate`` (cv2 correlates too); its border mode does not
  matter, the reference cuts ``[5:-5, 5:-5]`` from every result;
* ``.cuda()`` of tensors and modules: the identity, so ``_ssim_3d`` runs its fp32 Conv3d on the CPU.

Float cases go in as tensors (``basicsr``; the ``use_image: false`` route) or as HWC float arrays (``valid``),
uint8 cases through the reference's ``tensor2img`` first.  Train/utils.py's ``calculate_ssim`` knows one and
three channels only; for other counts its per-channel ``ssim`` is called on each channel and averaged, which is
what it does for three.  Inputs come from tests/ssim_oracle.py::cases and ::batch.

``basicsr`` is fp32 in the reference and float64 in the oracle: each case records the reference's number and
its gap to the oracle, and tests/test_ssim.py bounds the difference by 8 x that gap (floor 1e-7).  The gap
is capped: if any exceeds 1e-4 nothing is written (a wrong border mode or a mix-before-square mistake moves
these cases by far more; fp32 rounding does not).
"""
import importlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
from make_golden_metrics import _Inert, _InertFinder  # noqa: E402
from tests import ssim_oracle as so  # noqa: E402

GAP_CAP = 1e-4


def _get_gaussian_kernel(ksize, sigma, ktype=None):
    i = np.arange(ksize, dtype=np.float64) - (ksize - 1) / 2.0
    g = np.exp(-(i * i) / (2.0 * sigma * sigma))
    return (g / g.sum()).reshape(ksize, 1)


def _filter2d(src, ddepth, kernel, **kw):
    from scipy import ndimage
    assert ddepth == -1
    return ndimage.correlate(src, kernel, mode="reflect")


def main():
    train_dir = sys.argv[1]
    missing = []
    for root in ("cv2", "skimage", "lmdb", "tqdm", "yaml", "torchvision", "tensorboard", "requests", "einops",
                 "natsort"):
        try:
            importlib.import_module(root)
        except Exception:
            missing.append(root)
    if "cv2" not in missing:
        raise SystemExit("cv2 is installed: record with it and drop the two cv2 stand-ins from this script")
    sys.meta_path.append(_InertFinder(missing))
    cv2 = importlib.import_module("cv2")
    assert isinstance(cv2, _Inert)
    cv2.getGaussianKernel, cv2.filter2D = _get_gaussian_kernel, _filter2d
    sys.path.insert(0, train_dir)
    import torch
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.nn.Module.cuda = lambda self, *a, **k: self
    from basicsr.metrics.psnr_ssim import calculate_ssim
    from basicsr.utils.img_util import tensor2img
    import utils as train_utils   # <reference>/Train/utils.py

    def ref_basicsr(a, b, cb, use_image):
        ta, tb = torch.from_numpy(a).unsqueeze(0), torch.from_numpy(b).unsqueeze(0)
        if use_image:
            return float(calculate_ssim(tensor2img([ta], rgb2bgr=False), tensor2img([tb], rgb2bgr=False),
                                        crop_border=cb, test_y_channel=False))
        return float(calculate_ssim(ta, tb, crop_border=cb, test_y_channel=False))

    def ref_valid(a, b, cb, use_image):
        if use_image:
            ia = tensor2img([torch.from_numpy(a).unsqueeze(0)], rgb2bgr=False)
            ib = tensor2img([torch.from_numpy(b).unsqueeze(0)], rgb2bgr=False)
        else:
            ia, ib = a.transpose(1, 2, 0), b.transpose(1, 2, 0)
        if ia.ndim == 2 or ia.shape[2] in (1, 3):
            return float(train_utils.calculate_ssim(ia, ib, border=cb)), "calculate_ssim"
        h, w = ia.shape[:2]
        ia, ib = ia[cb:h - cb, cb:w - cb], ib[cb:h - cb, cb:w - cb]
        return float(np.mean([train_utils.ssim(ia[:, :, i], ib[:, :, i]) for i in range(ia.shape[2])])), \
            "mean of ssim per channel"

    out = {"source": {"basicsr": "basicsr.metrics.psnr_ssim.calculate_ssim (+ basicsr.utils.img_util.tensor2img "
                                 "for *_u8), its Conv3d in fp32 on the CPU",
                      "valid": "Train/utils.py calculate_ssim (ssim per channel where it has no branch for the "
                               "channel count)"},
           "stand_ins": {"inert_modules": missing,
                         "cv2.getGaussianKernel": "exp(-(i - (k - 1) / 2)^2 / (2 sigma^2)) / sum, float64",
                         "cv2.filter2D": "scipy.ndimage.correlate (border mode irrelevant after the [5:-5] cut)",
                         ".cuda()": "identity (no GPU where this was recorded)"},
           "gap_cap": GAP_CAP, "seed": 20250820, "cases": {}}
    items = {k: v for k, v in so.cases().items()}
    ba, bb = so.batch()
    for i in range(ba.shape[0]):
        items[f"batch3_{i}"] = (ba[i], bb[i], 0, False, ("basicsr", "valid"))
    worst = 0.0
    for name, (a, b, cb, use_image, variants) in items.items():
        rec = {"crop_border": cb, "use_image": use_image}
        if "basicsr" in variants:
            ref = ref_basicsr(a, b, cb, use_image)
            gap = abs(ref - so.ssim(a, b, None, cb, use_image, "basicsr"))
            worst = max(worst, gap)
            rec["basicsr"] = {"ssim": repr(ref), "gap_to_oracle": repr(gap)}
        if "valid" in variants:
            ref, via = ref_valid(a, b, cb, use_image)
            rec["valid"] = {"ssim": repr(ref), "via": via}
        out["cases"][name] = rec
    print(json.dumps(out["cases"], indent=1))
    print(f"worst basicsr gap to the float64 oracle: {worst:.3e} (cap {GAP_CAP:g})")
    if worst > GAP_CAP:
        raise SystemExit("a basicsr gap exceeds the cap: nothing written")
    with open(os.path.join(HERE, "metrics_ssim.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
