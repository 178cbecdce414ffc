"""Distillation labels: KDLAE-T (or Restormer) outputs as the targets of KDLAE-S training, made on the device.

The reference's ``KDLAES.yml`` trains the student against a folder of teacher outputs (``dataroot_gt``) that
``Dataset_PairedMutiImage`` reads back as grayscale float32 images.  ``teacher_labels`` gives the same targets for
a stack of frames without the folder: per chunk of ``teacher_batch`` frames one ``kdlae_distill_expand_*`` launch
(gray frame -> the teacher's three-channel input and its rate map), the teacher's own inference forward, and one
``kdlae_distill_collapse`` launch (three channels -> one gray target); include/kdlae.h states the semantics.

* ``mode="file"``: the round trip through a lossless image file, bit for bit the hand-written loop per frame
  (replicate the gray frame to three channels, ``pipeline.enhance_u8``, the 8-bit gray rule on the result, / 255).
  Parity with a real cv2 encode / decode is not pinned, as everywhere else in this project.
* ``mode="mean"``: ``((c0 + c1) + c2) / 3`` of the teacher's float output, no quantisation: for online training.

With ``tile=`` the chunk goes through the teacher's tiled forward.  As with ``forward_tiled``, that is a different
function of the frame from the untiled route (MDTA's channel attention is global over the pixels of each tile), not
an approximation of it that carries a bound.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from .pipeline import padded_size
from .tiling import _stream

MODES = {"file": 0, "mean": 1}   # KDLAE_DISTILL_FILE, KDLAE_DISTILL_MEAN


def _vp(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def item_rates(denoise_rate, B: int, F: int, device) -> torch.Tensor:
    """A scalar, ``[B]`` or ``[B,F]`` denoise rate -> contiguous f32 ``[B F]`` on ``device``, item order j = b F + f."""
    rt = torch.as_tensor(denoise_rate, dtype=torch.float32)
    if rt.dim() == 1 and rt.shape[0] == B:
        rt = rt[:, None]
    elif rt.dim() != 0 and tuple(rt.shape) != (B, F):
        raise RuntimeError(f"denoise_rate must be a scalar, [{B}] or [{B},{F}], got {tuple(rt.shape)}")
    return rt.to(device).expand(B, F).contiguous().view(B * F)


def chunks(total: int, teacher_batch: int):
    """The chunk schedule: ``(j0, n)`` over ``total`` items, ``teacher_batch`` at a time, the rest last."""
    tb = int(teacher_batch)
    if tb < 1:
        raise RuntimeError(f"teacher_batch must be at least 1, got {teacher_batch}")
    return [(j0, min(tb, total - j0)) for j0 in range(0, total, tb)]


def distill_expand(frames: torch.Tensor, rate, j0: int, n: int, img: torch.Tensor, rate_map, multiple: int = 8):
    """``kdlae_distill_expand_u8`` / ``_f32`` (by ``frames.dtype``) for items ``j0 .. j0 + n - 1`` of ``frames``
    u8 [B,F,h,w(,C)] or f32 [B,F,H,W] into ``img`` [n,3,H,W] and ``rate_map`` [n,1,H,W] (both None: no map)."""
    B, F, h, w = frames.shape[:4]
    L = _lib.lib()
    if frames.dtype == torch.uint8:
        C = frames.shape[4] if frames.dim() == 5 else 1
        rc = L.kdlae_distill_expand_u8(_vp(frames), B, F, h, w, C, int(multiple), _vp(rate), int(j0), int(n),
                                       _vp(img), _vp(rate_map), _stream(frames.device))
        _lib.check(rc, "kdlae_distill_expand_u8")
    else:
        rc = L.kdlae_distill_expand_f32(_vp(frames), B, F, h, w, _vp(rate), int(j0), int(n), _vp(img),
                                        _vp(rate_map), _stream(frames.device))
        _lib.check(rc, "kdlae_distill_expand_f32")


def distill_collapse(hq: torch.Tensor, out: torch.Tensor, j0: int, n: int, mode: str = "file", src=None):
    """``kdlae_distill_collapse``: ``hq`` [n,3,Hp,Wp] -> items ``j0 .. j0 + n - 1`` of ``out`` [B,F,h,w] (f32 or u8);
    ``src``: the u8 source frames [B,F,h,w(,C)] of the black mask, or None."""
    if mode not in MODES:
        raise RuntimeError(f"mode must be one of {sorted(MODES)}, got {mode!r}")
    B, F, h, w = out.shape
    Hp, Wp = hq.shape[-2:]
    C = 0 if src is None else (src.shape[4] if src.dim() == 5 else 1)
    rc = _lib.lib().kdlae_distill_collapse(_vp(hq), B, F, Hp, Wp, h, w, int(j0), int(n), MODES[mode], _vp(src), C,
                                           _vp(out), int(out.dtype == torch.uint8), _stream(hq.device))
    _lib.check(rc, "kdlae_distill_collapse")


def _labels(teacher, frames, denoise_rate, mode, teacher_batch, tile, tile_overlap, window, out, out_dtype, what):
    from .KDLAE_model import KDLAE_teacher
    if not isinstance(teacher, KDLAE_teacher):
        raise RuntimeError(f"{what}: the teacher must be a KDLAE_teacher or a Restormer")
    if mode not in MODES:
        raise RuntimeError(f"{what}: mode must be one of {sorted(MODES)}, got {mode!r}")
    if not isinstance(frames, torch.Tensor) or frames.device.type != "cuda":
        raise RuntimeError(f"{what} runs on ROCm devices only; move the frames to 'cuda' (no CPU fallback)")
    u8 = frames.dtype == torch.uint8
    if not ((u8 and frames.dim() in (4, 5)) or (frames.dtype == torch.float32 and frames.dim() == 4)):
        raise RuntimeError(f"{what} expects cuda uint8 frames [B,F,h,w] or [B,F,h,w,C] or float32 frames [B,F,H,W], "
                           f"got {frames.dtype} {tuple(frames.shape)}")
    teacher._check_inference_input(frames, what)   # a teacher in .train() mode is refused here
    cfg = teacher._cfg
    if cfg["inp_channels"] != 3 or cfg["out_channels"] != 3:
        raise RuntimeError(f"{what}: the teacher must take and give 3 channels")
    dev = frames.device
    if next(teacher.parameters()).device != dev:
        raise RuntimeError(f"{what}: the teacher and the frames must be on the same device")
    B, F, h, w = frames.shape[:4]
    if u8:
        H, W = padded_size(h, w, 8)
        if H - h >= h or W - w >= w:
            raise RuntimeError(f"{what}: a {h}x{w} frame is smaller than its reflect padding")
    else:
        H, W = h, w
        if H % 8 or W % 8:
            raise RuntimeError(f"{what}: float32 frames are network inputs, H and W divisible by 8; got {H}x{W}")
    plan = chunks(B * F, teacher_batch)
    shape = (B, F, h, w)
    if out is not None and (tuple(out.shape) != shape or out.dtype != out_dtype or out.device != dev
                            or not out.is_contiguous()):
        raise RuntimeError(f"{what}: out must be a contiguous {str(out_dtype).replace('torch.', '')} {shape} on {dev}")
    cat = cfg["params"] == "cat"
    if cat and denoise_rate is None:
        raise RuntimeError(f"{what}: this teacher takes a denoise_rate")
    rate = item_rates(denoise_rate, B, F, dev) if cat else None
    if tile is not None:   # a bad tile / overlap / window is refused before any launch
        from . import tiling
        tiling.tile_plan(H, W, tile, tile_overlap)
        tiling.tile_window(window, H, W, tile, tile_overlap, 1, dev)
    frames = frames.contiguous()
    if out is None:
        out = torch.empty(shape, device=dev, dtype=out_dtype)
    # the staging of one chunk, reused by every chunk of the call; the forward writes sr only with the sr head
    tb = plan[0][1]
    img = torch.empty((tb, 3, H, W), device=dev, dtype=torch.float32)
    rmap = torch.empty((tb, 1, H, W), device=dev, dtype=torch.float32) if cat else None
    untiled = tile is None
    hq = torch.empty((tb, 3, H, W), device=dev, dtype=torch.float32) if untiled else None
    sr = torch.empty((tb, 3, 2 * H, 2 * W), device=dev, dtype=torch.float32) \
        if untiled and teacher.static == "train" else None
    src = frames if u8 and mode == "file" else None
    with torch.no_grad():
        for j0, n in plan:
            c_img, c_map = img[:n], (rmap[:n] if cat else None)
            distill_expand(frames, rate, j0, n, c_img, c_map)
            if untiled:
                c_hq = teacher._forward_eager(c_img, c_map, out=(hq[:n], sr[:n] if sr is not None else None))["hq"]
            else:
                c_hq = teacher._forward_tiled(c_img, c_map, tile, tile_overlap, int(teacher_batch),
                                              window=window)["hq"]
            distill_collapse(c_hq, out, j0, n, mode, src)
    return out


def teacher_labels(teacher, frames: torch.Tensor, denoise_rate, mode: str = "file", teacher_batch: int = 16,
                   tile=None, tile_overlap: int = 32, window="uniform", out: torch.Tensor | None = None):
    """Targets for a KDLAE-S training step from a teacher, on the device: ``frames`` cuda u8 ``[B,F,h,w]`` (gray) or
    ``[B,F,h,w,C]`` (cv2 BGR / BGRA), or f32 ``[B,F,H,W]`` network inputs (H, W divisible by 8) -> f32 ``[B,F,h,w]``.

    ``denoise_rate``: a scalar, ``[B]`` or ``[B,F]``; ``None`` for a ``Restormer`` (ignored by a teacher without the
    rate input).  ``teacher_batch`` frames at a time are expanded into staging tensors that every chunk reuses, go
    through the teacher's own inference forward under ``no_grad`` (through its tiled forward with ``tile``,
    ``tile_overlap`` and ``window`` when ``tile`` is set) and are collapsed into ``out``; beyond ``out`` (when not
    given) nothing the size of the stack is allocated.  The teacher's parameters and mode are not touched; a
    teacher in ``.train()`` mode, a CPU tensor or another dtype is refused before any launch.

    ``mode="file"`` is bit for bit the per-frame loop: replicate the gray frame to three channels,
    ``pipeline.enhance_u8`` (``model({...})["hq"]``, clamp and ``round(x 255)`` for f32 frames), the 8-bit gray rule
    on the R, G, B bytes, / 255; for every ``teacher_batch``.  ``mode="mean"`` is ``((c0 + c1) + c2) / 3`` of the
    float output, cropped.  The tiled route equals the same loop over ``pipeline.enhance_tiled_u8``; it is a
    different function of the frame from the untiled one, not an approximation with a bound."""
    return _labels(teacher, frames, denoise_rate, mode, teacher_batch, tile, tile_overlap, window, out,
                   torch.float32, "teacher_labels")


def teacher_labels_u8(teacher, clip: torch.Tensor, denoise_rate, teacher_batch: int = 16, tile=None,
                      tile_overlap: int = 32, window="uniform", out: torch.Tensor | None = None):
    """The offline label generator: a cuda u8 clip ``[B,T,h,w]`` or ``[B,T,h,w,C]`` of any length T -> u8 ``[B,T,h,w]``
    in frame order: the gray bytes an image file of the teacher's output holds (``mode="file"``; ``teacher_labels``
    states the rule and the arguments).  ``teacher_labels(...)`` of the same clip is these bytes / 255."""
    if not isinstance(clip, torch.Tensor) or clip.dtype != torch.uint8:
        raise RuntimeError("teacher_labels_u8 expects a cuda uint8 clip [B,T,h,w] or [B,T,h,w,C]")
    return _labels(teacher, clip, denoise_rate, "file", teacher_batch, tile, tile_overlap, window, out,
                   torch.uint8, "teacher_labels_u8")
