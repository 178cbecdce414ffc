#!/usr/bin/env python
"""Record tests/golden/metrics_psnr.json from the reference's own ``calculate_psnr``.

    python tests/golden/make_golden_metrics.py <reference checkout>/Train

``basicsr/metrics/psnr_ssim.py`` imports cv2 and skimage at module level (and ``basicsr.metrics`` pulls in
niqe, ``basicsr.utils`` much more); ``calculate_psnr`` and ``tensor2img(rgb2bgr=False)`` use neither.  Modules
that are not installed get inert stand-ins, so the reference functions themselves run.  Float cases go in
as tensors (the ``use_image: false`` route, image_restoration_model.py:333-336), uint8 cases through the
reference's ``tensor2img`` first (:291-293,327-331).  Inputs come from tests/metrics_oracle.py::cases.
"""
import importlib
import importlib.abc
import importlib.machinery
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import metrics_oracle  # noqa: E402


class _Inert(types.ModuleType):
    """A module whose every attribute is another inert object (callable, subscriptable, importable)."""

    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Inert(self.__name__ + "." + name)

    def __call__(self, *a, **k):
        return self


class _InertFinder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    def __init__(self, roots):
        self.roots = tuple(roots)

    def find_spec(self, name, path=None, target=None):
        if name.split(".")[0] in self.roots:
            return importlib.machinery.ModuleSpec(name, self, is_package=True)
        return None

    def create_module(self, spec):
        return _Inert(spec.name)

    def exec_module(self, module):
        pass


def main():
    train_dir = sys.argv[1]
    missing = []
    for root in ("cv2", "skimage", "scipy", "lmdb", "tqdm", "yaml", "torchvision", "tensorboard", "requests",
                 "einops", "natsort"):
        try:
            importlib.import_module(root)
        except Exception:
            missing.append(root)
    sys.meta_path.append(_InertFinder(missing))
    sys.path.insert(0, train_dir)
    import torch
    from basicsr.metrics.psnr_ssim import calculate_psnr
    from basicsr.utils.img_util import tensor2img

    out = {"source": "basicsr.metrics.psnr_ssim.calculate_psnr (+ basicsr.utils.img_util.tensor2img for *_u8)",
           "stand_ins": missing, "seed": 20250819, "cases": {}}
    for name, (a, b, cb, use_image) in metrics_oracle.cases().items():
        ta, tb = torch.from_numpy(a).unsqueeze(0), torch.from_numpy(b).unsqueeze(0)
        if use_image:
            ia, ib = tensor2img([ta], rgb2bgr=False), tensor2img([tb], rgb2bgr=False)
            v = calculate_psnr(ia, ib, crop_border=cb, test_y_channel=False)
        else:
            v = calculate_psnr(ta, tb, crop_border=cb, test_y_channel=False)
        out["cases"][name] = {"crop_border": cb, "use_image": use_image, "psnr": repr(float(v))}
    with open(os.path.join(HERE, "metrics_psnr.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out["cases"], indent=1))


if __name__ == "__main__":
    main()
