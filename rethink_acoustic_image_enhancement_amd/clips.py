"""Clip inference for KDLAE-S: overlapping windows of consecutive frames of a clip, blended on the device.

Thin wrappers of ``kdlae_clip_plan`` / ``kdlae_clip_gather`` / ``kdlae_clip_blend`` / ``kdlae_clip_blend_u8``
(include/kdlae.h states the semantics) on the current stream.  ``KDLAE_student.forward_clip`` and
``pipeline.enhance_clip_u8`` are built on them.  The plan is tiling.py's on the frame axis: windows of
``f = min(frames, T)`` frames starting at ``range(0, T - f, f - overlap) + [T - f]``, a plain sum over the covering
windows in window order and a division by their count.  ``clip_window`` builds the table of the other blend
windows (``"ramp"``, ``"hann"``, a given table), which both blends take as ``window=``: a weighted mean whose
weights fall towards the window's first and last frame, so that a window fades out where its neighbour fades in.

The student's 3-D convolutions zero-pad along the frame axis, so a window's output depends on the window alone and
a windowed result is a different function of the clip from one forward over all T frames: it is not an
approximation of that forward that carries an error bound."""
from __future__ import annotations

import ctypes
from typing import NamedTuple

import torch

from . import _lib, tiling
from .tiling import _stream

WINDOWS = tiling.WINDOWS


class ClipPlan(NamedTuple):
    f: int
    n: int
    stride: int

    def starts(self, T: int):
        """Window starts along the frame axis."""
        return [i * self.stride for i in range(self.n - 1)] + [T - self.f]


class ClipWindow(NamedTuple):
    """What ``clip_window`` returns: a checked fp32 device table of length ``f``.  Passed as ``window`` it is taken
    as it is, so a caller with several blends builds its table once."""
    wt: torch.Tensor


def clip_plan(T: int, frames: int = 7, overlap: int = 2) -> ClipPlan:
    """``kdlae_clip_plan``: host only.  RuntimeError unless T >= 1, frames >= 1 and 0 <= overlap < min(frames, T)."""
    out = [ctypes.c_int() for _ in range(3)]
    rc = _lib.lib().kdlae_clip_plan(int(T), int(frames), int(overlap), *[ctypes.byref(v) for v in out])
    _lib.check(rc, "kdlae_clip_plan")
    return ClipPlan(*[v.value for v in out])


def _check_f32_cuda(t: torch.Tensor, what: str):
    if t.device.type != "cuda" or t.dtype != torch.float32 or t.dim() != 4:
        raise RuntimeError(f"{what} expects a cuda float32 tensor with 4 dimensions, got {t.dtype} "
                           f"{tuple(t.shape)} on {t.device}")


def _check_out(out, shape, dtype, device, what: str):
    if tuple(out.shape) != shape or out.dtype != dtype or out.device != device or not out.is_contiguous():
        raise RuntimeError(f"{what}: out must be a contiguous {str(dtype).replace('torch.', '')} {shape} on {device}")


def clip_gather(src: torch.Tensor, frames: int = 7, overlap: int = 2, first: int = 0, count: int | None = None,
                out: torch.Tensor | None = None) -> torch.Tensor:
    """Windows ``first .. first + count - 1`` (flat index ``b n + i``; default: all of them) of ``src`` [B,T,H,W]
    -> dense [count,f,H,W].  ``out``: a contiguous destination of that shape."""
    _check_f32_cuda(src, "clip_gather")
    src = src.contiguous()
    B, T, H, W = src.shape
    p = clip_plan(T, frames, overlap)
    if count is None:
        count = B * p.n - first
    shape = (count, p.f, H, W)
    if out is None:
        out = torch.empty(shape, device=src.device, dtype=torch.float32)
    else:
        _check_out(out, shape, torch.float32, src.device, "clip_gather")
    rc = _lib.lib().kdlae_clip_gather(ctypes.c_void_p(src.data_ptr()), B, T, H, W, int(frames), int(overlap),
                                      int(first), int(count), ctypes.c_void_p(out.data_ptr()), _stream(src.device))
    _lib.check(rc, "kdlae_clip_gather")
    return out


def clip_window(window, T: int, frames: int = 7, overlap: int = 2, device="cuda"):
    """The blend window of a plan as one fp32 device table ``wt [f]``, or ``None`` for ``"uniform"`` / ``None``
    (the plain mean).  A frame's weight under a window is ``wt[p]`` at its position ``p`` inside the window;
    ``kdlae_clip_blend`` (include/kdlae.h) states the sum.

    ``"ramp"`` and ``"hann"`` are ``tiling.tile_window``'s tables for an axis with tile ``f``: ``min(p + 1, f - p,
    max(overlap, 1))`` (ones when the clip is one window) and ``sin^2(pi (p + 1/2) / f)``.  A 1-D floating-point
    tensor of length ``f`` (CPU or device) is checked on the host: length, finite, > 0 in fp32."""
    if window is None or (isinstance(window, str) and window == "uniform"):
        return None
    p = clip_plan(T, frames, overlap)
    if isinstance(window, ClipWindow):
        if tuple(window.wt.shape) != (p.f,):
            raise RuntimeError(f"clip_window: a table of length {p.f} expected, got {tuple(window.wt.shape)}")
        return window
    if isinstance(window, str):
        if window not in WINDOWS:
            raise RuntimeError(f"clip_window: window must be one of {WINDOWS} or a 1-D tensor, got {window!r}")
        wt = tiling._named_axis(window, p.f, p.n, overlap, 1).to(torch.float32)
    else:
        if not isinstance(window, torch.Tensor) or not window.dtype.is_floating_point:
            raise RuntimeError(f"clip_window: window must be one of {WINDOWS} or a floating-point 1-D tensor, got "
                               f"{window.dtype if isinstance(window, torch.Tensor) else type(window).__name__}")
        if window.dim() != 1 or window.shape[0] != p.f:
            raise RuntimeError(f"clip_window: the table must have the window's length {p.f}, got shape "
                               f"{tuple(window.shape)}")
        wt = window.detach().to(device="cpu", dtype=torch.float32)
        if not bool(torch.isfinite(wt).all()) or not bool((wt > 0).all()):
            raise RuntimeError("clip_window: every entry of the table must be finite and greater than 0 in float32")
    return ClipWindow(wt.to(device).contiguous())


def _blend_args(windows: torch.Tensor, B: int, T: int, frames: int, overlap: int, window, what: str):
    _check_f32_cuda(windows, what)
    windows = windows.contiguous()
    p = clip_plan(T, frames, overlap)
    H, W = windows.shape[-2:]
    want = (int(B) * p.n, p.f, H, W)
    if tuple(windows.shape) != want:
        raise RuntimeError(f"{what}: expected windows {want}, got {tuple(windows.shape)}")
    table = clip_window(window, T, frames, overlap, windows.device)
    return windows, H, W, ctypes.c_void_p(table.wt.data_ptr() if table is not None else 0), table


def clip_blend(windows: torch.Tensor, B: int, T: int, frames: int = 7, overlap: int = 2, window="uniform",
               out: torch.Tensor | None = None) -> torch.Tensor:
    """``windows`` [B n, f, H, W] of a [B,T,H,W] clip's plan -> [B,T,H,W]: per element the fp32 sum of the covering
    windows in window order over their fp32 count.  ``window``: a name or a table as ``clip_window`` takes it;
    anything but ``"uniform"`` is the weighted mean of ``kdlae_clip_blend`` with a table."""
    windows, H, W, wt, table = _blend_args(windows, B, T, frames, overlap, window, "clip_blend")
    shape = (int(B), int(T), H, W)
    if out is None:
        out = torch.empty(shape, device=windows.device, dtype=torch.float32)
    else:
        _check_out(out, shape, torch.float32, windows.device, "clip_blend")
    rc = _lib.lib().kdlae_clip_blend(ctypes.c_void_p(windows.data_ptr()), int(B), int(T), H, W, int(frames),
                                     int(overlap), wt, ctypes.c_void_p(out.data_ptr()), _stream(windows.device))
    _lib.check(rc, "kdlae_clip_blend")
    return out


def clip_blend_u8(windows: torch.Tensor, B: int, T: int, h: int, w: int, frames: int = 7, overlap: int = 2,
                  window="uniform", out: torch.Tensor | None = None) -> torch.Tensor:
    """``clip_blend`` and ``pipeline.postprocess_u8``'s rule in one launch: ``windows`` [B n, f, H, W] -> u8
    [B,T,h,w] in frame order (clamp to [0, 1], ``rint(x 255)``, crop to ``h <= H``, ``w <= W``): the bytes of
    ``postprocess_u8(clip_blend(...), h, w)`` without the float clip in between."""
    windows, H, W, wt, table = _blend_args(windows, B, T, frames, overlap, window, "clip_blend_u8")
    shape = (int(B), int(T), int(h), int(w))
    if out is None:
        out = torch.empty(shape, device=windows.device, dtype=torch.uint8)
    else:
        _check_out(out, shape, torch.uint8, windows.device, "clip_blend_u8")
    rc = _lib.lib().kdlae_clip_blend_u8(ctypes.c_void_p(windows.data_ptr()), int(B), int(T), H, W, int(h), int(w),
                                        int(frames), int(overlap), wt, ctypes.c_void_p(out.data_ptr()),
                                        _stream(windows.device))
    _lib.check(rc, "kdlae_clip_blend_u8")
    return out
