"""Validation metrics on the MI355X HIP path (``kdlae_metric_psnr`` in include/kdlae.h).

* ``calculate_psnr`` — the reference's ``basicsr.metrics.calculate_psnr`` (Train/basicsr/metrics/
  psnr_ssim.py:9-70) for ``cuda`` tensors: same signature, same Python float.
* ``psnr_batch`` — the same number for every image of a batch in one launch, over a top-left valid
  window of a padded output (``pad_test``'s crop, image_restoration_model.py:236-237), as a device tensor
  and without a host synchronisation.
* ``finish_psnr`` — the host end of ``calculate_psnr`` (:66-70) from the kernel's two reductions.

* ``calculate_ssim`` / ``ssim_batch`` / ``finish_ssim`` — the same three for the reference's
  ``basicsr.metrics.calculate_ssim`` (psnr_ssim.py:240-318, the 11^3 replicate-padded window over the
  (H, W, C) volume) through ``kdlae_metric_ssim``; ``calculate_ssim_valid`` is the classic per-channel SSIM
  over valid positions (Train/utils.py:31-78).

There is no CPU fallback: CPU tensors and ndarrays raise, like every other entry point of this package.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib

__all__ = ["calculate_psnr", "psnr_batch", "psnr_reduce", "finish_psnr",
           "ssim_reduce", "ssim_batch", "finish_ssim", "calculate_ssim", "calculate_ssim_valid"]


def finish_psnr(sse: float, max_pred: float, n: int) -> float:
    """psnr_ssim.py:66-70 from sum((img1 - img2)^2), max(img1) and the element count: ``inf`` when the
    mean is 0, and the peak is 1 or 255 by the first operand's maximum alone (the reference's rule)."""
    mse = np.float64(sse) / n
    if mse == 0:
        return float("inf")
    max_value = 1.0 if max_pred <= 1 else 255.0
    return float(20.0 * np.log10(max_value / np.sqrt(mse)))  # numpy's log10, as the reference calls it


_SCRATCH = {}


def _scratch(dev):
    # one per device and stream: launches on one stream are ordered, so they may share it
    key = (dev.index, torch.cuda.current_stream(dev).cuda_stream)
    buf = _SCRATCH.get(key)
    if buf is None:
        buf = _SCRATCH[key] = torch.empty(int(_lib.lib().kdlae_metric_scratch_bytes()) // 8, dtype=torch.float64,
                                          device=dev)
    return buf


def psnr_reduce(pred, gt, valid_hw=None, crop_border=0, use_image=False):
    """The kernel's raw result: ``([B, 2] float64 device tensor of (sse, max pred), n)`` with ``n`` the
    number of compared elements per image.  No host synchronisation."""
    for t in (pred, gt):
        if not torch.is_tensor(t) or t.device.type != "cuda":
            raise RuntimeError("PSNR (MI355X build) runs on ROCm device tensors only; there is no CPU fallback")
    if pred.dim() != 4 or gt.dim() != 4 or pred.shape[:2] != gt.shape[:2] or pred.device != gt.device or \
            (valid_hw is None and pred.shape != gt.shape):
        raise ValueError(f"expected pred, gt [B,C,H,W] on one device, of equal shape or with a valid_hw window "
                         f"inside both, got {tuple(pred.shape)}, {tuple(gt.shape)}")
    pred = pred.detach().to(torch.float32).contiguous()
    gt = gt.detach().to(torch.float32).contiguous()
    B, C, Hs, Ws = pred.shape
    Hg, Wg = gt.shape[2:]
    h, w = (Hs, Ws) if valid_hw is None else (int(valid_hw[0]), int(valid_hw[1]))
    cb = int(crop_border)
    dev = pred.device
    out = torch.empty((B, 2), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.lib().kdlae_metric_psnr(
            ctypes.c_void_p(pred.data_ptr()), ctypes.c_void_p(gt.data_ptr()), B, C, Hs, Ws, Hg, Wg, h, w, cb,
            1 if use_image else 0, ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(_scratch(dev).data_ptr()),
            ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    _lib.check(rc, "kdlae_metric_psnr")
    return out, C * (h - 2 * cb) * (w - 2 * cb)


def psnr_batch(pred, gt, valid_hw=None, crop_border=0, use_image=False):
    """PSNR of each image of ``pred`` against ``gt`` ([B,C,Hs,Ws] ``cuda`` tensors) -> [B] float64 device tensor.

    ``valid_hw=(h, w)``: compare the top-left h x w window only (``pred`` and ``gt`` may then be stored at
    different sizes, e.g. a padded output against its unpadded target); ``crop_border`` pixels are then removed
    from its four sides; ``use_image=True`` quantises both operands to uint8 as ``tensor2img`` does and
    compares on the 0..255 scale.  The call does not synchronise: read the tensor when you need it."""
    red, n = psnr_reduce(pred, gt, valid_hw, crop_border, use_image)
    mse = red[:, 0] / n
    peak = torch.where(red[:, 1] <= 1, 1.0, 255.0).to(torch.float64)
    psnr = 20.0 * torch.log10(peak / torch.sqrt(mse))
    return torch.where(mse == 0, torch.full_like(psnr, float("inf")), psnr)


def calculate_psnr(img1, img2, crop_border, input_order="HWC", test_y_channel=False):
    """``basicsr.metrics.calculate_psnr`` for ``cuda`` tensors of shape [C,H,W] or [1,C,H,W] (a tensor is
    taken as CHW whatever ``input_order`` says, psnr_ssim.py:38-51; of a larger batch the first image is
    used, :42-43).  Returns the reference's Python float."""
    if input_order not in ["HWC", "CHW"]:
        raise ValueError(f'Wrong input_order {input_order}. Supported input_orders are "HWC" and "CHW"')
    for t in (img1, img2):
        if not torch.is_tensor(t) or t.device.type != "cuda":
            raise RuntimeError("calculate_psnr (MI355X build) takes ROCm device tensors only; there is no CPU "
                               "fallback (ndarrays and CPU tensors: use the reference's numpy function)")
    assert img1.shape == img2.shape, f"Image shapes are differnet: {img1.shape}, {img2.shape}."
    if test_y_channel:
        raise NotImplementedError("test_y_channel=True is not used by the reference configs (and needs cv2)")

    def chw(t):
        if t.dim() == 4:
            t = t.squeeze(0)
        if t.dim() == 4:
            t = t[0]
        if t.dim() != 3:
            raise ValueError(f"expected a [C,H,W] or [1,C,H,W] tensor, got {tuple(t.shape)}")
        return t.unsqueeze(0)

    red, n = psnr_reduce(chw(img1), chw(img2), None, crop_border, False)
    sse, mx = red[0].tolist()
    return finish_psnr(sse, mx, n)


# ------------------------------------------------------------------ SSIM (kdlae_metric_ssim, csrc/ssim.hip)
_VARIANTS = {"basicsr": 0, "valid": 1}
_SSIM_SCRATCH = {}


def _variant(variant) -> int:
    if variant not in _VARIANTS:
        raise ValueError(f"unknown SSIM variant {variant!r}: expected one of {sorted(_VARIANTS)}")
    return _VARIANTS[variant]


def _ssim_scratch(dev):
    key = (dev.index, torch.cuda.current_stream(dev).cuda_stream)
    buf = _SSIM_SCRATCH.get(key)
    if buf is None:
        buf = _SSIM_SCRATCH[key] = torch.empty(int(_lib.lib().kdlae_metric_ssim_scratch_bytes()) // 8,
                                               dtype=torch.float64, device=dev)
    return buf


def finish_ssim(sum_l1: float, sum_l255: float, max_pred: float, n: float, variant="basicsr") -> float:
    """The host end of the SSIM from the kernel's four doubles: the mean of the map, taken with the L = 1
    constants when the first operand's maximum is <= 1 (psnr_ssim.py:307) and with the L = 255 ones
    otherwise; the ``valid`` flavour always uses L = 255 (Train/utils.py:59-60)."""
    use_l1 = _variant(variant) == 0 and max_pred <= 1
    return float(np.float64(sum_l1 if use_l1 else sum_l255) / np.float64(n))


def ssim_reduce(pred, gt, valid_hw=None, crop_border=0, use_image=False, variant="basicsr"):
    """The kernel's raw result: a [B, 4] float64 device tensor of (sum of the map with the L = 1 constants,
    sum with the L = 255 constants, max pred, number of map entries) per image.  No host synchronisation."""
    v = _variant(variant)
    for t in (pred, gt):
        if not torch.is_tensor(t) or t.device.type != "cuda":
            raise RuntimeError("SSIM (MI355X build) runs on ROCm device tensors only; there is no CPU fallback")
    if pred.dim() != 4 or gt.dim() != 4 or pred.shape[:2] != gt.shape[:2] or pred.device != gt.device or \
            (valid_hw is None and pred.shape != gt.shape):
        raise ValueError(f"expected pred, gt [B,C,H,W] on one device, of equal shape or with a valid_hw window "
                         f"inside both, got {tuple(pred.shape)}, {tuple(gt.shape)}")
    pred = pred.detach().to(torch.float32).contiguous()
    gt = gt.detach().to(torch.float32).contiguous()
    B, C, Hs, Ws = pred.shape
    Hg, Wg = gt.shape[2:]
    h, w = (Hs, Ws) if valid_hw is None else (int(valid_hw[0]), int(valid_hw[1]))
    dev = pred.device
    out = torch.empty((B, 4), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.lib().kdlae_metric_ssim(
            ctypes.c_void_p(pred.data_ptr()), ctypes.c_void_p(gt.data_ptr()), B, C, Hs, Ws, Hg, Wg, h, w,
            int(crop_border), 1 if use_image else 0, v, ctypes.c_void_p(out.data_ptr()),
            ctypes.c_void_p(_ssim_scratch(dev).data_ptr()),
            ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    _lib.check(rc, "kdlae_metric_ssim")
    return out


def ssim_batch(pred, gt, valid_hw=None, crop_border=0, use_image=False, variant="basicsr"):
    """SSIM of each image of ``pred`` against ``gt`` ([B,C,Hs,Ws] ``cuda`` tensors) -> [B] float64 device tensor.

    ``valid_hw``, ``crop_border`` and ``use_image`` as in ``psnr_batch``; the window's replicate border is the
    edge of the compared region, never the storage around it.  ``variant``: ``"basicsr"`` (the reference's
    ``calculate_ssim``, 1 <= C <= 4) or ``"valid"`` (Train/utils.py's, 0..255 scale, at least 11 x 11 pixels).
    The call does not synchronise: the L = 1 or L = 255 sum is picked on the device."""
    red = ssim_reduce(pred, gt, valid_hw, crop_border, use_image, variant)
    if _variant(variant) == 0:
        return torch.where(red[:, 2] <= 1, red[:, 0], red[:, 1]) / red[:, 3]
    return red[:, 1] / red[:, 3]


def calculate_ssim(img1, img2, crop_border, input_order="HWC", test_y_channel=False):
    """``basicsr.metrics.calculate_ssim`` for ``cuda`` tensors of shape [C,H,W] or [1,C,H,W] (a tensor is
    taken as CHW whatever ``input_order`` says, psnr_ssim.py:276-283; a larger batch fails there at the
    transpose and raises ``ValueError`` here).  Returns a Python float."""
    if input_order not in ["HWC", "CHW"]:
        raise ValueError(f'Wrong input_order {input_order}. Supported input_orders are "HWC" and "CHW"')
    for t in (img1, img2):
        if not torch.is_tensor(t) or t.device.type != "cuda":
            raise RuntimeError("calculate_ssim (MI355X build) takes ROCm device tensors only; there is no CPU "
                               "fallback (ndarrays and CPU tensors: use the reference's function)")
    assert img1.shape == img2.shape, f"Image shapes are differnet: {img1.shape}, {img2.shape}."
    if test_y_channel:
        raise NotImplementedError("test_y_channel=True is not used by the reference configs (and needs cv2)")

    def chw(t):
        if t.dim() == 4:
            t = t.squeeze(0)
        if t.dim() != 3:
            raise ValueError(f"expected a [C,H,W] or [1,C,H,W] tensor, got {tuple(t.shape)}")
        return t.unsqueeze(0)

    s1, s255, mx, n = ssim_reduce(chw(img1), chw(img2), None, crop_border, False, "basicsr")[0].tolist()
    return finish_ssim(s1, s255, mx, n, "basicsr")


def calculate_ssim_valid(img1, img2, border=0):
    """``calculate_ssim`` of Train/utils.py:31-78 for ``cuda`` tensors [C,H,W] on the 0..255 scale: per channel
    over valid positions, the mean over channels.  Returns a Python float."""
    for t in (img1, img2):
        if not torch.is_tensor(t) or t.device.type != "cuda":
            raise RuntimeError("calculate_ssim_valid (MI355X build) takes ROCm device tensors only; there is no CPU "
                               "fallback (ndarrays and CPU tensors: use the reference's function)")
    if not img1.shape == img2.shape:
        raise ValueError("Input images must have the same dimensions.")
    if img1.dim() != 3:
        raise ValueError(f"expected [C,H,W] tensors, got {tuple(img1.shape)}")
    s1, s255, mx, n = ssim_reduce(img1.unsqueeze(0), img2.unsqueeze(0), None, border, False, "valid")[0].tolist()
    return finish_ssim(s1, s255, mx, n, "valid")
