"""Tiled inference: overlapping tiles of an image too large for one forward, blended on the device.

Thin wrappers of ``kdlae_tile_plan`` / ``kdlae_tile_gather`` / ``kdlae_tile_blend`` (include/kdlae.h states the
semantics) on the current stream.  ``KDLAE_teacher.forward_tiled`` and ``pipeline.enhance_tiled_u8`` are built
on them; ``tile_blend_rates`` (``kdlae_tile_blend_rates``) is the blend of the tiled rate sweep
(``KDLAE_teacher.forward_rates_tiled``, ``pipeline.enhance_auto_tiled_u8``).  The plan follows upstream Restormer's demo (``--tile`` / ``--tile_overlap``): starts
``range(0, L - t, t - tile_overlap) + [L - t]`` per axis, a plain sum over the covering tiles in tile order and
a division by their count; the tile is clamped per axis (``th = min(tile, H)``, ``tw = min(tile, W)``).
``tile_window`` builds the tables of the other blend windows (``"ramp"``, ``"hann"``, a given pair), which both
blends take as ``window=`` and hand to ``kdlae_tile_blend_w`` / ``kdlae_tile_blend_rates_w``: a weighted mean
whose weights fall towards the tile edge, so that a tile fades out where its neighbour fades in.

MDTA's channel attention is global over the pixels of whatever it is given, so a tile's output depends on the
tile alone and a tiled result is a different function of the image from the untiled forward, exactly as it is
upstream: it is not an approximation of the untiled result that carries an error bound."""
from __future__ import annotations

import ctypes
import math
from typing import NamedTuple

import torch

from . import _lib


class TilePlan(NamedTuple):
    th: int
    tw: int
    ni: int
    nj: int
    stride_y: int
    stride_x: int

    def starts(self, H: int, W: int):
        """Tile starts along y and x."""
        return ([i * self.stride_y for i in range(self.ni - 1)] + [H - self.th],
                [j * self.stride_x for j in range(self.nj - 1)] + [W - self.tw])


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def tile_plan(H: int, W: int, tile: int = 512, tile_overlap: int = 32) -> TilePlan:
    """``kdlae_tile_plan``: host only.  RuntimeError unless H % 8 == W % 8 == tile % 8 == 0, tile >= 16 and
    0 <= tile_overlap < tile."""
    out = [ctypes.c_int() for _ in range(6)]
    rc = _lib.lib().kdlae_tile_plan(int(H), int(W), int(tile), int(tile_overlap), *[ctypes.byref(v) for v in out])
    _lib.check(rc, "kdlae_tile_plan")
    return TilePlan(*[v.value for v in out])


def _check_f32_cuda(t: torch.Tensor, what: str):
    if t.device.type != "cuda" or t.dtype != torch.float32 or t.dim() != 4:
        raise RuntimeError(f"{what} expects a cuda float32 tensor with 4 dimensions, got {t.dtype} "
                           f"{tuple(t.shape)} on {t.device}")


def tile_gather(src: torch.Tensor, tile: int = 512, tile_overlap: int = 32, first: int = 0, count: int | None = None,
                out: torch.Tensor | None = None) -> torch.Tensor:
    """Tiles ``first .. first + count - 1`` (flat index ``(b ni + i) nj + j``; default: all of them) of
    ``src`` [B,C,H,W] -> dense [count,C,th,tw].  ``out``: a contiguous destination of that shape."""
    _check_f32_cuda(src, "tile_gather")
    src = src.contiguous()
    B, C, H, W = src.shape
    p = tile_plan(H, W, tile, tile_overlap)
    if count is None:
        count = B * p.ni * p.nj - first
    shape = (count, C, p.th, p.tw)
    if out is None:
        out = torch.empty(shape, device=src.device, dtype=torch.float32)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or out.device != src.device or \
            not out.is_contiguous():
        raise RuntimeError(f"tile_gather: out must be a contiguous float32 {shape} on {src.device}")
    rc = _lib.lib().kdlae_tile_gather(ctypes.c_void_p(src.data_ptr()), B, C, H, W, int(tile), int(tile_overlap),
                                      int(first), int(count), ctypes.c_void_p(out.data_ptr()), _stream(src.device))
    _lib.check(rc, "kdlae_tile_gather")
    return out


WINDOWS = ("uniform", "ramp", "hann")


class WindowTables(NamedTuple):
    """What ``tile_window`` returns: checked fp32 device tables of lengths ``scale th`` and ``scale tw``.  Passed
    as ``window`` it is taken as it is, so a caller with several blends builds its tables once."""
    wy: torch.Tensor
    wx: torch.Tensor


def _named_axis(name: str, t: int, n: int, overlap: int, s: int) -> torch.Tensor:
    """One axis of a named window in float64: tile t, n tiles along the axis, scale s -> [s t]."""
    p = torch.arange(s * t, dtype=torch.float64)
    if name == "hann":
        return torch.sin(math.pi * (p + 0.5) / (s * t)) ** 2
    if n == 1:   # nothing to fade into
        return torch.ones(s * t, dtype=torch.float64)
    m = max(int(overlap), 1)
    return torch.minimum(torch.minimum(p + 1, s * t - p), torch.full_like(p, s * m))


def _given_axis(w, t: int, s: int, what: str) -> torch.Tensor:
    if not isinstance(w, torch.Tensor) or not w.dtype.is_floating_point:
        raise RuntimeError(f"tile_window: {what} must be a floating-point tensor, got "
                           f"{w.dtype if isinstance(w, torch.Tensor) else type(w).__name__}")
    if w.dim() != 1 or w.shape[0] != t:
        raise RuntimeError(f"tile_window: {what} must have the tile's length {t}, got shape {tuple(w.shape)}")
    w = w.detach().to(device="cpu", dtype=torch.float32)
    if not bool(torch.isfinite(w).all()) or not bool((w > 0).all()):
        raise RuntimeError(f"tile_window: every entry of {what} must be finite and greater than 0 in float32")
    return w.repeat_interleave(s)


def tile_window(window, H: int, W: int, tile: int = 512, tile_overlap: int = 32, scale: int = 1, device="cuda"):
    """The blend window of a plan as two fp32 device tables ``(wy [scale th], wx [scale tw])``, or ``None`` for
    ``"uniform"`` / ``None`` (the plain mean: ``kdlae_tile_blend``).  A pixel's weight under a tile is
    ``wy[yt] * wx[xt]`` at its tile-local coordinate; ``kdlae_tile_blend_w`` (include/kdlae.h) states the sum.

    ``"ramp"``: per axis with tile ``t``, ``m = max(tile_overlap, 1)`` and scale ``s``, ``w(p) = min(p + 1,
    s t - p, s m)``: integers, so two regular neighbours sum to ``s m + 1`` across their overlap, a linear
    cross-fade; an axis with one tile gets ones.  ``"hann"``: ``sin^2(pi (p + 1/2) / (s t))``, strictly
    positive.  A pair ``(wy, wx)`` of 1-D floating-point tensors of lengths ``th`` and ``tw`` (CPU or device):
    checked on the host (length, finite, > 0 in fp32), every entry repeated ``scale`` times.  Named tables are
    built in float64 on the host and rounded once."""
    if window is None or (isinstance(window, str) and window == "uniform"):
        return None
    if int(scale) not in (1, 2):
        raise RuntimeError(f"tile_window: scale must be 1 or 2, got {scale}")
    s = int(scale)
    p = tile_plan(H, W, tile, tile_overlap)
    if isinstance(window, WindowTables):
        if tuple(window.wy.shape) != (s * p.th,) or tuple(window.wx.shape) != (s * p.tw,):
            raise RuntimeError(f"tile_window: tables of lengths {s * p.th} and {s * p.tw} expected, got "
                               f"{tuple(window.wy.shape)} and {tuple(window.wx.shape)}")
        return window
    if isinstance(window, str):
        if window not in WINDOWS:
            raise RuntimeError(f"tile_window: window must be one of {WINDOWS} or a pair (wy, wx), got {window!r}")
        wy = _named_axis(window, p.th, p.ni, tile_overlap, s).to(torch.float32)
        wx = _named_axis(window, p.tw, p.nj, tile_overlap, s).to(torch.float32)
    else:
        if not isinstance(window, (tuple, list)) or len(window) != 2:
            raise RuntimeError(f"tile_window: window must be one of {WINDOWS} or a pair (wy, wx), got "
                               f"{type(window).__name__}")
        wy = _given_axis(window[0], p.th, s, "wy")
        wx = _given_axis(window[1], p.tw, s, "wx")
    return WindowTables(wy.to(device).contiguous(), wx.to(device).contiguous())


def tile_blend(tiles: torch.Tensor, B: int, H: int, W: int, tile: int = 512, tile_overlap: int = 32, scale: int = 1,
               out: torch.Tensor | None = None, window="uniform") -> torch.Tensor:
    """``tiles`` [B ni nj, C, scale th, scale tw] of a [B,C,H,W] image's plan -> [B, C, scale H, scale W]: per
    pixel the fp32 sum of the covering tiles in flat-index order over their fp32 count.  ``window``: a name or a
    pair as ``tile_window`` takes it; anything but ``"uniform"`` is the weighted mean of ``kdlae_tile_blend_w``."""
    _check_f32_cuda(tiles, "tile_blend")
    tiles = tiles.contiguous()
    p = tile_plan(H, W, tile, tile_overlap)
    tables = tile_window(window, H, W, tile, tile_overlap, scale, tiles.device) if scale in (1, 2) else None
    C = tiles.shape[1]
    want = (B * p.ni * p.nj, C, scale * p.th, scale * p.tw)
    if scale in (1, 2) and tuple(tiles.shape) != want:
        raise RuntimeError(f"tile_blend: expected tiles {want}, got {tuple(tiles.shape)}")
    shape = (B, C, scale * H, scale * W)
    if out is None:
        out = torch.empty(shape, device=tiles.device, dtype=torch.float32)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or out.device != tiles.device or \
            not out.is_contiguous():
        raise RuntimeError(f"tile_blend: out must be a contiguous float32 {shape} on {tiles.device}")
    if tables is not None:
        rc = _lib.lib().kdlae_tile_blend_w(ctypes.c_void_p(tiles.data_ptr()), int(B), C, int(H), int(W), int(tile),
                                           int(tile_overlap), int(scale), ctypes.c_void_p(tables[0].data_ptr()),
                                           ctypes.c_void_p(tables[1].data_ptr()), ctypes.c_void_p(out.data_ptr()),
                                           _stream(tiles.device))
        _lib.check(rc, "kdlae_tile_blend_w")
        return out
    rc = _lib.lib().kdlae_tile_blend(ctypes.c_void_p(tiles.data_ptr()), int(B), C, int(H), int(W), int(tile),
                                     int(tile_overlap), int(scale), ctypes.c_void_p(out.data_ptr()),
                                     _stream(tiles.device))
    _lib.check(rc, "kdlae_tile_blend")
    return out


def staged_slots(index: torch.Tensor, tiles_per_image: int, R: int, tile_batch: int) -> torch.Tensor:
    """Where a tiled rate sweep staged each tile at its image's rate ``index[b]`` (device, integer [B]): for tile
    ``t`` of the ``n = B tiles_per_image`` the position, in tiles, inside ``kdlae_tile_blend_rates``' chunk-major
    buffer: chunk ``k = t // tile_batch`` starts at ``k tile_batch R`` and holds rate ``r``, tile ``q = t - k
    tile_batch`` at ``r count_k + q``.  int64 [n] on the device, no host synchronisation."""
    n = index.shape[0] * int(tiles_per_image)
    tb = min(int(tile_batch), n)
    t = torch.arange(n, device=index.device)
    k = t // tb
    count_k = (n - k * tb).clamp(max=tb)
    return k * tb * int(R) + index.long()[t // int(tiles_per_image)] * count_k + (t - k * tb)


def tile_blend_rates(staged: torch.Tensor, R: int, B: int, H: int, W: int, tile: int = 512, tile_overlap: int = 32,
                     tile_batch: int = 16, scale: int = 1, out: torch.Tensor | None = None,
                     window="uniform") -> torch.Tensor:
    """``kdlae_tile_blend_rates``: the chunk-major staging of a tiled rate sweep (``kdlae_t_forward_rates`` on the
    ``n = B ni nj`` tiles ``tile_batch`` at a time; include/kdlae.h states the layout) -> ``[R, B, C, scale H,
    scale W]`` in one launch; ``out[r]`` has the bits ``tile_blend`` gives for the r-th slice.  ``staged``: a
    contiguous cuda float32 tensor of any shape with ``n R C scale^2 th tw`` elements (``C`` follows from that).
    ``window``: as in ``tile_blend`` (``kdlae_tile_blend_rates_w``)."""
    if staged.device.type != "cuda" or staged.dtype != torch.float32 or not staged.is_contiguous():
        raise RuntimeError(f"tile_blend_rates expects a contiguous cuda float32 tensor, got {staged.dtype} "
                           f"{tuple(staged.shape)} on {staged.device}")
    p = tile_plan(H, W, tile, tile_overlap)
    R, B, scale = int(R), int(B), int(scale)
    if not 1 <= R <= 64 or B < 1 or int(tile_batch) < 1 or scale not in (1, 2):
        raise RuntimeError(f"tile_blend_rates: need 1 <= R <= 64, B >= 1, tile_batch >= 1 and a scale of 1 or 2, got "
                           f"R {R}, B {B}, tile_batch {tile_batch}, scale {scale}")
    per_c = B * p.ni * p.nj * R * scale * scale * p.th * p.tw   # floats per channel
    C = staged.numel() // per_c
    if C < 1 or staged.numel() != per_c * C:
        raise RuntimeError(f"tile_blend_rates: expected {per_c} floats per channel ({B * p.ni * p.nj} tiles, {R} "
                           f"rates), got {staged.numel()}")
    shape = (R, B, C, scale * H, scale * W)
    if out is None:
        out = torch.empty(shape, device=staged.device, dtype=torch.float32)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or out.device != staged.device or \
            not out.is_contiguous():
        raise RuntimeError(f"tile_blend_rates: out must be a contiguous float32 {shape} on {staged.device}")
    tables = tile_window(window, H, W, tile, tile_overlap, scale, staged.device)
    if tables is not None:
        rc = _lib.lib().kdlae_tile_blend_rates_w(ctypes.c_void_p(staged.data_ptr()), R, B, C, int(H), int(W),
                                                 int(tile), int(tile_overlap), int(tile_batch), scale,
                                                 ctypes.c_void_p(tables[0].data_ptr()),
                                                 ctypes.c_void_p(tables[1].data_ptr()),
                                                 ctypes.c_void_p(out.data_ptr()), _stream(staged.device))
        _lib.check(rc, "kdlae_tile_blend_rates_w")
        return out
    rc =_lib.lib().kdlae_tile_blend_rates(ctypes.c_void_p(staged.data_ptr()), R, B, C, int(H), int(W), int(tile),
                                           int(tile_overlap), int(tile_batch), scale,
                                           ctypes.c_void_p(out.data_ptr()), _stream(staged.device))
    _lib.check(rc, "kdlae_tile_blend_rates")
    return out
