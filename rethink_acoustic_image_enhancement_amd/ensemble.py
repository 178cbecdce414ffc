"""Geometric self-ensemble: the eight dihedral views of an image gathered and merged on the device.

Thin wrappers of ``kdlae_ens_gather`` / ``kdlae_ens_merge`` (include/kdlae_ensemble.h states the rule) on the
current stream, and the chunk plan ``forward_ensemble`` of the three modules runs the views through.

Mode ``m`` in 0..7 is ``T_m(x) = flipud^(m % 2)(rot90ccw^(m // 2)(x))`` on the last two axes: the
``data_augmentation`` modes of dataset.py, under which all three networks are trained.  Modes 0, 1, 4, 5 keep
``[H, W]``, modes 2, 3, 6, 7 give ``[W, H]``.  For a set of modes ``M``

    y = ((((0 + U_m0) + U_m1) + ...)) / float(|M|),      U_m = T_m^-1(f(T_m(x), T_m(rate)))

with the modes ascending and every fp32 add and the one divide rounded on their own: the host loop
``torch.rot90`` / ``torch.flip``, forward, inverse, ``E.add_``, one ``E.div_``, bit for bit.

The views sit in one flat buffer, one dense block ``[N, C, H', W']`` per mode in ascending order, slot ``s`` at
float ``s N C H W``.  The mean over the views is a different function of the image from ``forward``: it is not an
approximation of ``forward`` that carries an error bound (``M = {0}`` alone equals it)."""
from __future__ import annotations

import ctypes

import torch

from . import _lib

MODES = tuple(range(8))
_NAMED = {"d8": MODES, "flips": (0, 1, 4, 5)}    # "flips": the four views that keep the shape


def mode_mask(modes="d8") -> int:
    """``"d8"`` (all eight), ``"flips"`` ({0, 1, 4, 5}: identity, the two flips and their product) or an iterable
    of modes 0..7 -> the 8-bit mask with bit ``m`` set for mode ``m``."""
    if isinstance(modes, str):
        if modes not in _NAMED:
            raise RuntimeError(f"ensemble modes must be one of {tuple(_NAMED)} or an iterable of modes 0..7, got "
                               f"{modes!r}")
        modes = _NAMED[modes]
    mask = 0
    try:
        items = list(modes)
    except TypeError:
        raise RuntimeError(f"ensemble modes must be one of {tuple(_NAMED)} or an iterable of modes 0..7, got "
                           f"{type(modes).__name__}") from None
    for m in items:
        if isinstance(m, bool) or not isinstance(m, int) or m not in MODES:
            raise RuntimeError(f"ensemble modes are integers 0..7, got {m!r}")
        mask |= 1 << m
    if mask == 0:
        raise RuntimeError("ensemble modes: at least one mode is needed")
    return mask


def mask_modes(mask: int):
    """The modes of a mask in ascending order: slot ``s`` of the layout holds mode ``mask_modes(mask)[s]``."""
    if not 1 <= int(mask) <= 255:
        raise RuntimeError(f"ensemble mask must be 1..255, got {mask}")
    return [m for m in MODES if (int(mask) >> m) & 1]


def transposes(m: int) -> bool:
    """Whether mode ``m`` turns ``[H, W]`` into ``[W, H]``."""
    return bool((m >> 1) & 1)


def view_shape(m: int, H: int, W: int):
    return (W, H) if transposes(m) else (H, W)


def ens_chunks(mask: int, H: int, W: int, ens_batch: int = 8):
    """The forwards of a mask: ``(first slot, slots, (H', W'))`` runs of at most ``ens_batch`` consecutive slots of
    one shape, so that every run is one dense ``[slots N, C, H', W']`` batch of the layout.  With H == W all views
    have one shape and a run may hold any of them."""
    if int(ens_batch) < 1:
        raise RuntimeError(f"ens_batch must be at least 1, got {ens_batch}")
    shapes = [view_shape(m, H, W) for m in mask_modes(mask)]
    chunks, s = [], 0
    while s < len(shapes):
        n = 1
        while s + n < len(shapes) and n < int(ens_batch) and shapes[s + n] == shapes[s]:
            n += 1
        chunks.append((s, n, shapes[s]))
        s += n
    return chunks


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _check_out(out, numel, dev, what):
    if out.dtype != torch.float32 or out.device != dev or out.numel() != numel or not out.is_contiguous():
        raise RuntimeError(f"{what}: out must be a contiguous float32 tensor of {numel} elements on {dev}")


def ens_gather(src: torch.Tensor, modes="d8", out: torch.Tensor | None = None) -> torch.Tensor:
    """``kdlae_ens_gather``: ``src`` [N,C,H,W] -> the views of ``modes`` in the slot layout, a flat tensor of
    ``|M| N C H W`` floats (``ens_views`` cuts it).  One launch.  ``out``: a contiguous destination of that size."""
    if src.device.type != "cuda" or src.dtype != torch.float32 or src.dim() != 4:
        raise RuntimeError(f"ens_gather expects a cuda float32 tensor with 4 dimensions, got {src.dtype} "
                           f"{tuple(src.shape)} on {src.device}")
    mask = modes if isinstance(modes, int) and not isinstance(modes, bool) else mode_mask(modes)
    n_modes = len(mask_modes(mask))
    src = src.contiguous()
    N, C, H, W = src.shape
    if out is None:
        out = torch.empty(n_modes * src.numel(), device=src.device, dtype=torch.float32)
    else:
        _check_out(out, n_modes * src.numel(), src.device, "ens_gather")
    rc = _lib.lib().kdlae_ens_gather(ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(out.data_ptr()), N, C, H, W,
                                     mask, _stream(src.device))
    _lib.check(rc, "kdlae_ens_gather")
    return out


def ens_views(buf: torch.Tensor, N: int, C: int, H: int, W: int, modes="d8"):
    """The slots of a layout buffer as ``[N, C, H', W']`` views of it, in ascending mode order."""
    mask = modes if isinstance(modes, int) and not isinstance(modes, bool) else mode_mask(modes)
    per = N * C * H * W
    flat = buf.reshape(-1)
    return [flat[s * per:(s + 1) * per].view(N, C, *view_shape(m, H, W)) for s, m in enumerate(mask_modes(mask))]


def ens_merge(staged: torch.Tensor, N: int, H: int, W: int, modes="d8", out: torch.Tensor | None = None):
    """``kdlae_ens_merge``: the views' outputs in the slot layout (any shape, ``|M| N C H W`` floats; ``C``
    follows from that) -> ``[N, C, H, W]``: per pixel the inverse-transformed values added in ascending mode order
    to 0 and divided by ``|M|``.  One launch."""
    if staged.device.type != "cuda" or staged.dtype != torch.float32 or not staged.is_contiguous():
        raise RuntimeError(f"ens_merge expects a contiguous cuda float32 tensor, got {staged.dtype} "
                           f"{tuple(staged.shape)} on {staged.device}")
    mask = modes if isinstance(modes, int) and not isinstance(modes, bool) else mode_mask(modes)
    n_modes = len(mask_modes(mask))
    N, H, W = int(N), int(H), int(W)
    if N < 1 or H < 1 or W < 1:
        raise RuntimeError(f"ens_merge: N, H and W must be positive, got {N}, {H}, {W}")
    per_c = n_modes * N * H * W
    C = staged.numel() // per_c
    if C < 1 or staged.numel() != per_c * C:
        raise RuntimeError(f"ens_merge: expected {per_c} floats per channel ({n_modes} views of {N} x {H} x {W}), "
                           f"got {staged.numel()}")
    if out is None:
        out = torch.empty((N, C, H, W), device=staged.device, dtype=torch.float32)
    else:
        _check_out(out, N * C * H * W, staged.device, "ens_merge")
    rc = _lib.lib().kdlae_ens_merge(ctypes.c_void_p(staged.data_ptr()), ctypes.c_void_p(out.data_ptr()), N, C, H, W,
                                    mask, _stream(staged.device))
    _lib.check(rc, "kdlae_ens_merge")
    return out


def run_views(forward, mask: int, B: int, H: int, W: int, ens_batch: int, inputs, out_channels, scales):
    """The forwards of ``forward_ensemble``.  ``inputs``: the gathered layout buffers of the model's inputs with
    their channel counts ``[(buf, C), ...]`` (``buf`` None: an input the model does not take); ``out_channels`` /
    ``scales``: per output its channels and its size relative to the input (1, or 2 for sr; channels None: an output
    the model does not have).  ``forward(ins, outs)`` runs the model's inference forward on the dense batches
    ``ins`` into the dense destinations ``outs``.  Returns the staged outputs, one layout buffer each."""
    n_modes = len(mask_modes(mask))
    dev = next(b for b, _ in inputs if b is not None).device
    staged = [torch.empty(n_modes * B * c * s * s * H * W, device=dev, dtype=torch.float32) if c else None
              for c, s in zip(out_channels, scales)]
    for first, count, (h, w) in ens_chunks(mask, H, W, ens_batch):
        def cut(buf, c, s):
            per = B * c * s * s * H * W
            return buf[first * per:(first + count) * per].view(count * B, c, s * h, s * w)
        ins = [cut(b, c, 1) if b is not None else None for b, c in inputs]
        outs = [cut(b, c, s) if b is not None else None for b, c, s in zip(staged, out_channels, scales)]
        forward(ins, outs)
    return staged
