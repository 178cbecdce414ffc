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

* ``calculate_niqe`` / ``niqe_batch`` / ``niqe_reduce`` / ``finish_niqe`` — the reference's
  ``basicsr.metrics.calculate_niqe`` (niqe.py:10-205) through ``kdlae_metric_niqe``: the MSCN fields of both
  scales and the per-block moments on the device, the AGGD fits and the multivariate-Gaussian distance on the
  host in float64.  The pristine model (``niqe_pris_params.npz``) is the reference's data and is not part of
  this package: pass its path or its three arrays as ``params``.

There is no CPU fallback: CPU tensors and ndarrays raise, like every other entry point of this package.
"""
from __future__ import annotations

import ctypes
import functools
import math
import os

import numpy as np
import torch

from . import _lib

__all__ = ["calculate_psnr", "psnr_batch", "psnr_reduce", "finish_psnr",
           "ssim_reduce", "ssim_batch", "finish_ssim", "calculate_ssim", "calculate_ssim_valid",
           "niqe_reduce", "niqe_batch", "finish_niqe", "calculate_niqe", "load_niqe_params"]


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


# ------------------------------------------------------------------ NIQE (kdlae_metric_niqe, csrc/niqe.hip)
NIQE_PARAMS = "basicsr/metrics/niqe_pris_params.npz"   # the reference's own relative path (niqe.py:186)
_NIQE_BLOCK = 96
_NIQE_SCRATCH = {}
_NIQE_KEYS = ("mu_pris_param", "cov_pris_param", "gaussian_window")


def load_niqe_params(params=None) -> dict:
    """The pristine model as float64 arrays: ``params`` is a path to the reference's ``niqe_pris_params.npz``
    (default: the reference's relative path, resolved against the working directory as there) or a mapping
    with ``mu_pris_param`` [1, 36], ``cov_pris_param`` [36, 36] and ``gaussian_window`` [7, 7]."""
    if params is None or isinstance(params, (str, os.PathLike)):
        path = NIQE_PARAMS if params is None else params
        if not os.path.exists(path):
            raise FileNotFoundError(f"NIQE needs the reference's pristine model, not found at {os.fspath(path)!r}: it "
                                    f"is not part of this package; pass params=<path to niqe_pris_params.npz>")
        with np.load(path) as d:
            params = {k: d[k] for k in _NIQE_KEYS}
    out = {k: np.ascontiguousarray(np.asarray(params[k], dtype=np.float64)) for k in _NIQE_KEYS}
    if out["mu_pris_param"].size != 36 or out["cov_pris_param"].shape != (36, 36) or \
            out["gaussian_window"].shape != (7, 7):
        raise ValueError("NIQE params: expected mu_pris_param of 36 entries, cov_pris_param [36, 36] and "
                         "gaussian_window [7, 7]")
    return out


def _niqe_scratch(dev, nbytes):
    key = (dev.index, torch.cuda.current_stream(dev).cuda_stream)
    buf = _NIQE_SCRATCH.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = _NIQE_SCRATCH[key] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    return buf


def niqe_reduce(x, valid_hw=None, crop_border=0, use_image=True, params=None, fields=False):
    """The kernel's raw result for ``x`` [B, C, Hs, Ws] (C = 1, or 3 in RGB order; values on the 0..255 scale, or
    on 0..1 with ``use_image=True``, which quantises as ``tensor2img`` does): a [B, 2, blocks, 5, 5] float64
    device tensor, per scale, block (in the reference's order, idx_w outer) and map (the field and its four
    rolled products) of (n_neg, n_pos, sum x^2 over x < 0, sum x^2 over x > 0, sum |x|).  ``fields=True``
    also returns the two MSCN fields ([B, H', W'] and [B, H'/2, W'/2] float32).  No host synchronisation."""
    if not torch.is_tensor(x) or x.device.type != "cuda":
        raise RuntimeError("NIQE (MI355X build) runs on ROCm device tensors only; there is no CPU fallback")
    if x.dim() != 4:
        raise ValueError(f"expected x [B,C,H,W], got {tuple(x.shape)}")
    window = load_niqe_params(params)["gaussian_window"]
    x = x.detach().to(torch.float32).contiguous()
    B, C, Hs, Ws = x.shape
    h, w = (Hs, Ws) if valid_hw is None else (int(valid_hw[0]), int(valid_hw[1]))
    cb = int(crop_border)
    nbh, nbw = max(h - 2 * cb, 0) // _NIQE_BLOCK, max(w - 2 * cb, 0) // _NIQE_BLOCK
    dev = x.device
    L = _lib.lib()
    out = torch.empty((B, 2, max(nbh * nbw, 1), 5, 5), dtype=torch.float64, device=dev)
    f1 = torch.empty((B, nbh * _NIQE_BLOCK, nbw * _NIQE_BLOCK), dtype=torch.float32, device=dev) if fields else None
    f2 = torch.empty((B, nbh * _NIQE_BLOCK // 2, nbw * _NIQE_BLOCK // 2), dtype=torch.float32, device=dev) \
        if fields else None
    win = np.ascontiguousarray(window, dtype=np.float64)
    with torch.cuda.device(dev):
        nbytes = max(int(L.kdlae_metric_niqe_scratch_bytes(B, max(h, 1), max(w, 1))), 256)
        scratch = _niqe_scratch(dev, nbytes)
        rc = L.kdlae_metric_niqe(
            ctypes.c_void_p(x.data_ptr()), B, C, Hs, Ws, h, w, cb, 1 if use_image else 0, 0,
            win.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.c_void_p(out.data_ptr()),
            ctypes.c_void_p(f1.data_ptr()) if fields else None, ctypes.c_void_p(f2.data_ptr()) if fields else None,
            ctypes.c_void_p(scratch.data_ptr()), scratch.numel(),
            ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    _lib.check(rc, "kdlae_metric_niqe")
    return (out, f1, f2) if fields else out


@functools.lru_cache(maxsize=None)
def _aggd_table():
    """niqe.py:21-24 once: gam = arange(0.2, 10.001, 0.001), r(gam) = Gamma(2/gam)^2 / (Gamma(1/gam) Gamma(3/gam))
    and log Gamma(k / gam) for k = 1, 2, 3, through math.lgamma (no scipy)."""
    gam = np.arange(0.2, 10.001, 0.001)
    rec = np.reciprocal(gam)
    r = np.array([math.exp(2.0 * math.lgamma(2.0 * t) - math.lgamma(t) - math.lgamma(3.0 * t)) for t in rec])
    lg = np.array([[math.lgamma(k / a) for a in gam] for k in (1.0, 2.0, 3.0)])
    if not np.all(np.diff(r) > 0):
        raise AssertionError("the AGGD ratio table is not increasing")
    return gam, r, lg


def _aggd_fit(mom, n):
    """estimate_aggd_param (niqe.py:10-37) for every row of ``mom`` [..., 5] over ``n`` samples each
    -> (index into gam, left_std, right_std)."""
    gam, r_gam, _ = _aggd_table()
    with np.errstate(all="ignore"):
        left = np.sqrt(mom[..., 2] / mom[..., 0])
        right = np.sqrt(mom[..., 3] / mom[..., 1])
        gammahat = left / right
        rhat = (mom[..., 4] / n) ** 2 / ((mom[..., 2] + mom[..., 3]) / n)
        rhatnorm = (rhat * (gammahat ** 3 + 1) * (gammahat + 1)) / ((gammahat ** 2 + 1) ** 2)
        # argmin((r_gam - rhatnorm)^2): r_gam increases, so the minimum is next to where rhatnorm would be
        # inserted; the same squares decide and the first smallest wins
        r = np.where(np.isfinite(rhatnorm), rhatnorm, 0.0)
        lo = np.clip(np.searchsorted(r_gam, r) - 2, 0, len(gam) - 4)
        cand = lo[..., None] + np.arange(4)
        sq = (r_gam[cand] - r[..., None]) ** 2
        pos = np.take_along_axis(cand, np.argmin(sq, axis=-1)[..., None], -1)[..., 0]
        # all squares equal (NaN, or infinite after overflow): np.argmin returns the first table entry
        pos = np.where(np.isfinite(rhatnorm) & ~np.isinf(sq).all(axis=-1), pos, 0)
    return pos, left, right


def _niqe_features(mom, n):
    """compute_feature (niqe.py:40-64) for moments [..., blocks, 5, 5] of n-sample blocks -> [..., blocks, 18]."""
    gam, _, lg = _aggd_table()
    pos, left, right = _aggd_fit(mom, n)
    with np.errstate(all="ignore"):
        alpha = gam[pos]
        scale = np.sqrt(np.exp(lg[0][pos] - lg[2][pos]))
        bl, br = left * scale, right * scale
        mean = (br - bl) * np.exp(lg[1][pos] - lg[0][pos])
    cols = [alpha[..., 0], (bl[..., 0] + br[..., 0]) / 2]
    for m in range(1, 5):
        cols += [alpha[..., m], mean[..., m], bl[..., m], br[..., m]]
    return np.stack(cols, axis=-1)


def finish_niqe(moments, params=None):
    """The host end of NIQE in numpy float64, from ``niqe_reduce``'s moments ([B, 2, blocks, 5, 5], or one
    image's [2, blocks, 5, 5]; a tensor is copied to the host, which synchronises): the AGGD fits, the 36
    features per block, their nanmean, the covariance over the blocks without NaN, the pseudo-inverse and
    the distance to the pristine model (niqe.py:10-64,140-155).  -> float64 array [B] (a Python float for one
    image).  With fewer than two NaN-free blocks the result is ``nan``; the reference raises from ``pinv``
    there (the covariance of one row is NaN)."""
    p = load_niqe_params(params)
    if torch.is_tensor(moments):
        moments = moments.detach().cpu().numpy()
    mom = np.asarray(moments, dtype=np.float64)
    single = mom.ndim == 4
    if single:
        mom = mom[None]
    if mom.ndim != 5 or mom.shape[1] != 2 or mom.shape[3:] != (5, 5):
        raise ValueError(f"expected moments [B, 2, blocks, 5, 5], got {mom.shape}")
    feat = np.concatenate([_niqe_features(mom[:, 0], float(_NIQE_BLOCK ** 2)),
                           _niqe_features(mom[:, 1], float((_NIQE_BLOCK // 2) ** 2))], axis=-1)
    mu_p, cov_p = p["mu_pris_param"].reshape(1, 36), p["cov_pris_param"]
    out = np.full(mom.shape[0], np.nan, dtype=np.float64)
    for b in range(mom.shape[0]):
        f = feat[b]
        good = f[~np.isnan(f).any(axis=1)]
        if good.shape[0] < 2:
            continue
        with np.errstate(all="ignore"):
            mu = np.nanmean(f, axis=0)   # every column has a value: a NaN-free row exists
        d = mu_p - mu
        inv = np.linalg.pinv((cov_p + np.cov(good, rowvar=False)) / 2)
        out[b] = np.sqrt(np.matmul(np.matmul(d, inv), np.transpose(d)))[0, 0]
    return float(out[0]) if single else out


def niqe_batch(x, valid_hw=None, crop_border=0, use_image=True, convert_to="y", params=None):
    """NIQE of each image of ``x`` ([B,C,Hs,Ws] ``cuda`` tensor, C = 1 or 3 in RGB order) -> [B] float64 CPU tensor.

    ``valid_hw`` and ``crop_border`` as in ``psnr_batch``; the remaining window is cropped to multiples of 96
    (at least one 96 x 96 block must remain) and the filter's replicate border is its edge, never the storage
    around it.  ``use_image=True`` (the default: NIQE is defined on 0..255 images, and the reference's function
    takes ``tensor2img``'s) quantises 0..1 values to uint8; ``False`` takes the floats as they are, on the 0..255
    scale.  Unlike the PSNR / SSIM calls this one synchronises: the fits are finished on the host."""
    if convert_to != "y":
        if convert_to == "gray":
            raise NotImplementedError("convert_to='gray' is cv2's BGR2GRAY conversion, which this build does not have")
        raise ValueError(f"unknown convert_to {convert_to!r}: expected 'y'")
    p = load_niqe_params(params)
    return torch.from_numpy(np.atleast_1d(finish_niqe(niqe_reduce(x, valid_hw, crop_border, use_image, p), p)))


def calculate_niqe(img, crop_border, input_order="HWC", convert_to="y", params=None):
    """``basicsr.metrics.calculate_niqe`` for ``cuda`` tensors of shape [C,H,W] or [1,C,H,W] on the 0..255 scale,
    C = 1 or 3 in RGB order (the reference takes BGR arrays; a tensor is taken as CHW whatever ``input_order``
    says, as in ``calculate_ssim``).  ``params``: see ``load_niqe_params``.  Returns a Python float."""
    if input_order not in ["HWC", "CHW"]:
        raise ValueError(f'Wrong input_order {input_order}. Supported input_orders are "HWC" and "CHW"')
    if not torch.is_tensor(img) or img.device.type != "cuda":
        raise RuntimeError("calculate_niqe (MI355X build) takes ROCm device tensors only; there is no CPU "
                           "fallback (ndarrays and CPU tensors: use the reference's function)")
    if img.dim() == 4:
        img = img.squeeze(0)
    if img.dim() != 3:
        raise ValueError(f"expected a [C,H,W] or [1,C,H,W] tensor, got {tuple(img.shape)}")
    return float(niqe_batch(img.unsqueeze(0), None, crop_border, False, convert_to, params)[0])
