"""The steps either side of the forward, on the GPU.

* ``enhance_u8`` — KDLAE/KDLAE_T.ipynb's inference cell for a batch of equally sized uint8 images:
  ``load_image_as_tensor`` (u8 -> /255, alpha dropped, optional BGR->RGB), reflect pad to a
  multiple of 8, constant ``denoise_rate`` map, forward, then clamp / crop / ``img_as_ubyte`` and the
  zero-mask of input-black pixels (x2 nearest for ``sr``).  Pre and post are HIP kernels
  (``kdlae_preprocess_u8`` / ``kdlae_postprocess_u8``); images never round-trip through the host.
* ``enhance_tiled_u8`` — the same cell for images too large for one forward: ``KDLAE_teacher.forward_tiled``
  between the same pre and post kernels (tiling.py).
* ``enhance_ensemble_u8`` — the same cell with geometric self-ensemble: ``forward_ensemble`` (the eight dihedral
  views, merged on the device; ensemble.py) between the same pre and post kernels.
* ``enhance_rates_u8`` / ``enhance_auto_u8`` — the notebook's "pick a rate, look, pick again" loop as one
  call: R rates of the same images through ``KDLAE_teacher.forward_rates`` (the rate-independent trunk runs
  once), every candidate post-processed as the notebook saves it, and — ``enhance_auto_u8`` — scored by
  ASDQE against the input and the candidate picked per image on the device (``kdlae_rate_select``).
* ``enhance_rates_tiled_u8`` / ``enhance_auto_tiled_u8`` — the same two calls for images too large for one
  forward: the sweep runs on tiles (``KDLAE_teacher.forward_rates_tiled``), the blended candidates are scored.
* ``frames_preprocess_u8`` / ``enhance_frames_u8`` — KDLAE/KDLAE-S.ipynb's cell: F frames (gray or
  cv2 BGR/BGRA u8) -> COLOR_BGR2GRAY -> /255 -> [B,F,H,W] reflect-padded to a multiple of 32 ->
  KDLAE_student -> clamp / crop / permute to [h,w,F] / ``img_as_ubyte``, pre and post on the GPU.
* ``enhance_clip_u8`` — the same cell for a whole clip of T frames: one ``frames_preprocess_u8``, overlapping
  windows of ``frames`` frames through KDLAE_student (``forward_clip``'s loop), and one launch that blends the
  windows and writes the u8 clip in frame order (clips.py).
* ``enhance_stream_u8`` — the same cell for a source that delivers one frame at a time: a generator over the
  arriving frames that yields every frame enhanced, in order, at a fixed latency (streams.py: the window lives in
  a ring on the device and the steady state replays one HIP graph).
* ``distill_clip_u8`` — KDLAE-T's output for every frame of a clip as the gray u8 labels KDLAE-S trains against
  (distill.py: what the reference keeps as a folder of saved teacher images).
* ``asdqe_scores`` / ``score_statistics`` / ``write_statistics_csv`` — ASDQE/ASDQE_test.py's
  ``infer`` + ``calculate_statistics`` + ``visualize_comparison`` CSV (:87-133).
"""
from __future__ import annotations

import ctypes
import csv

import numpy as np
import torch

from . import _lib


def padded_size(h: int, w: int, multiple: int = 8):
    H, W = ctypes.c_int(), ctypes.c_int()
    _lib.lib().kdlae_padded_size(h, w, multiple, ctypes.byref(H), ctypes.byref(W))
    return H.value, W.value


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def preprocess_u8(images: torch.Tensor, denoise_rate=None, multiple: int = 8, bgr: bool = False):
    """u8 [B,h,w,C] (cuda) -> (img f32 [B,min(C,3),H,W], rate map f32 [B,1,H,W] or None)."""
    if images.device.type != "cuda" or images.dtype != torch.uint8 or images.dim() != 4:
        raise RuntimeError("preprocess_u8 expects a cuda uint8 tensor [B,h,w,C]")
    images = images.contiguous()
    B, h, w, C = images.shape
    H, W = padded_size(h, w, multiple)
    dev = images.device
    img = torch.empty((B, min(C, 3), H, W), device=dev, dtype=torch.float32)
    rate = rmap = None
    if denoise_rate is not None:
        rate = torch.as_tensor(denoise_rate, dtype=torch.float32).to(dev).expand(B).contiguous()
        rmap = torch.empty((B, 1, H, W), device=dev, dtype=torch.float32)
    rc = _lib.lib().kdlae_preprocess_u8(
        ctypes.c_void_p(images.data_ptr()), B, h, w, C, int(bgr), multiple,
        ctypes.c_void_p(rate.data_ptr() if rate is not None else 0), ctypes.c_void_p(img.data_ptr()),
        ctypes.c_void_p(rmap.data_ptr() if rmap is not None else 0), _stream(dev))
    _lib.check(rc, "kdlae_preprocess_u8")
    return img, rmap


def postprocess_u8(out: torch.Tensor, h: int, w: int, scale: int = 1, lq_u8: torch.Tensor | None = None):
    """Model output f32 [B,C,Hs,Ws] -> u8 [B,h*scale,w*scale,C] (clamp, crop, img_as_ubyte, black mask)."""
    out = out.contiguous()
    B, C, Hs, Ws = out.shape
    dst = torch.empty((B, h * scale, w * scale, C), device=out.device, dtype=torch.uint8)
    lq = lq_u8.contiguous() if lq_u8 is not None else None
    rc = _lib.lib().kdlae_postprocess_u8(
        ctypes.c_void_p(out.data_ptr()), B, C, Hs, Ws, h, w, scale,
        ctypes.c_void_p(lq.data_ptr() if lq is not None else 0), lq.shape[-1] if lq is not None else 0,
        ctypes.c_void_p(dst.data_ptr()), _stream(out.device))
    _lib.check(rc, "kdlae_postprocess_u8")
    return dst


def _is_restormer(model) -> bool:
    from .KDLAE_model import Restormer
    return isinstance(model, Restormer)


def enhance_u8(model, images: torch.Tensor, denoise_rate, bgr: bool = False, multiple: int = 8):
    """KDLAE_T.ipynb inference for u8 images [B,h,w,C] on the model's device -> (hq u8, sr u8 or None).
    A ``KDLAE_model.Restormer`` takes the image alone: ``denoise_rate`` is ignored (pass None), no rate map is
    made and ``sr`` is None."""
    B, h, w, C = images.shape
    if _is_restormer(model):
        img, _ = preprocess_u8(images, None, multiple, bgr)
        with torch.no_grad():
            return postprocess_u8(model(img), h, w, 1, images), None
    img, rmap = preprocess_u8(images, denoise_rate, multiple, bgr)
    with torch.no_grad():
        pred = model({"img": img, "denoise_rate": rmap})
    hq = postprocess_u8(pred["hq"], h, w, 1, images)
    sr = postprocess_u8(pred["sr"], h, w, 2, images) if pred.get("sr") is not None else None
    return hq, sr


def enhance_tiled_u8(model, images: torch.Tensor, denoise_rate, tile: int = 512, tile_overlap: int = 32,
                     tile_batch: int = 16, bgr: bool = False, multiple: int = 8, window="uniform"):
    """``enhance_u8`` for images larger than one forward can hold: the same pre- and post-processing around
    ``KDLAE_teacher.forward_tiled`` (overlapping tiles blended on the device) -> (hq u8, sr u8 or None).  A tiled
    result is a different function of the image from ``enhance_u8``'s (MDTA's channel attention is global over
    the pixels of each tile), as it is in upstream Restormer's tiled demo; it equals it when one tile covers
    the padded image.  ``window``: the blend window, as ``KDLAE_teacher.forward_tiled`` takes it."""
    B, h, w, C = images.shape
    if _is_restormer(model):
        img, _ = preprocess_u8(images, None, multiple, bgr)
        return postprocess_u8(model.forward_tiled(img, tile, tile_overlap, tile_batch, window), h, w, 1,
                              images), None
    img, rmap = preprocess_u8(images, denoise_rate, multiple, bgr)
    pred = model.forward_tiled({"img": img, "denoise_rate": rmap}, tile, tile_overlap, tile_batch, window)
    hq = postprocess_u8(pred["hq"], h, w, 1, images)
    sr = postprocess_u8(pred["sr"], h, w, 2, images) if pred.get("sr") is not None else None
    return hq, sr


def enhance_ensemble_u8(model, images: torch.Tensor, denoise_rate, modes="d8", ens_batch: int = 8,
                        bgr: bool = False, multiple: int = 8):
    """``enhance_u8`` with geometric self-ensemble: the same pre- and post-processing around
    ``forward_ensemble`` on the padded tensor (the dihedral views gathered, batched through the forward and merged
    on the device; ensemble.py) -> (hq u8, sr u8 or None).  Serves ``KDLAE_teacher`` and ``Restormer`` (which
    ignores ``denoise_rate``).  The mean over the views is a different function of the image from ``enhance_u8``'s
    output, not an approximation of it; ``modes=(0,)`` equals it."""
    B, h, w, C = images.shape
    if _is_restormer(model):
        img, _ = preprocess_u8(images, None, multiple, bgr)
        return postprocess_u8(model.forward_ensemble(img, modes, ens_batch), h, w, 1, images), None
    img, rmap = preprocess_u8(images, denoise_rate, multiple, bgr)
    pred = model.forward_ensemble({"img": img, "denoise_rate": rmap}, modes, ens_batch)
    hq = postprocess_u8(pred["hq"], h, w, 1, images)
    sr = postprocess_u8(pred["sr"], h, w, 2, images) if pred.get("sr") is not None else None
    return hq, sr


def _rates_rb(rates, B: int, dev) -> torch.Tensor:
    """R scalars (shared by the batch) or [R, B] -> contiguous f32 [R, B] on ``dev``."""
    rt = torch.as_tensor(rates, dtype=torch.float32).to(dev)
    if rt.dim() == 1:
        rt = rt[:, None].expand(-1, B)
    if rt.dim() != 2 or rt.shape[1] != B:
        raise RuntimeError(f"rates must be R scalars or [R,{B}], got {tuple(rt.shape)}")
    return rt.contiguous()


def _sweep_u8(model, images: torch.Tensor, rates, bgr: bool, multiple: int):
    B, h, w, _ = images.shape
    img, _ = preprocess_u8(images, None, multiple, bgr)
    rt = _rates_rb(rates, B, images.device)
    with torch.no_grad():
        hq = model.forward_rates(img, rt, sr=False)["hq"]
    cands = torch.stack([postprocess_u8(hq[r], h, w, 1, images) for r in range(rt.shape[0])])
    return rt, hq, cands


def enhance_rates_u8(model, images: torch.Tensor, rates, bgr: bool = False, multiple: int = 8) -> torch.Tensor:
    """``enhance_u8``'s hq for every rate of a sweep: u8 [B,h,w,C], R rates (scalars or [R,B]) -> u8 [R,B,h,w,C].
    Candidate r is byte for byte ``enhance_u8(model, images, rates[r])[0]``."""
    return _sweep_u8(model, images, rates, bgr, multiple)[2]


_SELECT_MODES = {"closest": 0, "max": 1, "min": 2}


def rate_select(scores: torch.Tensor, hq: torch.Tensor, select: str = "closest", target=None):
    """``kdlae_rate_select``: device scores [R,B] and candidates [R,B,...] (f32) -> (index i32 [B], chosen [B,...]).
    ``closest``: argmin |score - target| (target a float or [B]); ``max`` / ``min``: argmax / argmin.  Ties go to
    the lowest r, a NaN score is never chosen.  No host synchronisation."""
    if select not in _SELECT_MODES:
        raise RuntimeError(f"select must be one of {sorted(_SELECT_MODES)}, got {select!r}")
    if scores.device.type != "cuda" or hq.device != scores.device or scores.dim() != 2 or hq.dim() < 3 or \
            tuple(hq.shape[:2]) != tuple(scores.shape):
        raise RuntimeError("rate_select expects cuda scores [R,B] and candidates [R,B,...] on the same device")
    R, B = scores.shape
    dev = scores.device
    scores = scores.detach().to(torch.float32).contiguous()
    hq = hq.detach().to(torch.float32).contiguous()
    tgt = None
    if select == "closest":
        if target is None:
            raise RuntimeError("select='closest' needs a target score")
        tgt = torch.as_tensor(target, dtype=torch.float32).to(dev).expand(B).contiguous()
    index = torch.empty((B,), device=dev, dtype=torch.int32)
    out = torch.empty(hq.shape[1:], device=dev, dtype=torch.float32)
    rc = _lib.lib().kdlae_rate_select(
        ctypes.c_void_p(scores.data_ptr()), R, B, _SELECT_MODES[select],
        ctypes.c_void_p(tgt.data_ptr() if tgt is not None else 0), ctypes.c_void_p(hq.data_ptr()),
        hq[0, 0].numel(), ctypes.c_void_p(index.data_ptr()), ctypes.c_void_p(out.data_ptr()), _stream(dev))
    _lib.check(rc, "kdlae_rate_select")
    return index, out


def enhance_auto_u8(model, scorer, images: torch.Tensor, rates, target=None, select: str = "closest",
                    want_sr: bool = False, bgr: bool = False) -> dict:
    """Sweep ``rates`` over u8 images [B,h,w,C], score every post-processed candidate against its input with
    ASDQE (``scorer``: a DenoiseRatePredictor in eval mode) and keep, per image, the candidate ``select``
    names.  ``scores[r]`` is what ``asdqe_scores(scorer, images, enhance_rates_u8(...)[r])`` gives; the sr head
    runs only on the chosen float hq, and only with ``want_sr``.  Everything stays on the device, with one
    synchronisation before the results are returned:
    ``{"hq": u8 [B,h,w,C], "rate": f32 [B], "index": i32 [B], "scores": f32 [R,B], "sr": u8 [B,2h,2w,C] | None}``."""
    if select not in _SELECT_MODES:
        raise RuntimeError(f"select must be one of {sorted(_SELECT_MODES)}, got {select!r}")
    B, h, w, _ = images.shape
    dev = images.device
    rt, hq, cands = _sweep_u8(model, images, rates, bgr, 8)
    R = rt.shape[0]
    scores = torch.empty((R, B), device=dev, dtype=torch.float32)
    with torch.no_grad():
        for c0 in range(0, B, 64):  # asdqe_scores' chunking: every pair is scored independently
            lq = to_tensor_u8(images[c0:c0 + 64])
            for r in range(R):
                scores[r, c0:c0 + 64] = scorer(lq, to_tensor_u8(cands[r, c0:c0 + 64])).view(-1)
    index, hq_sel = rate_select(scores, hq, select, target)
    pick = (index.long(), torch.arange(B, device=dev))
    sr = None
    if want_sr:
        with torch.no_grad():
            sr = postprocess_u8(model.forward_sr(hq_sel), h, w, 2, images)
    out = {"hq": cands[pick], "rate": rt[pick], "index": index, "scores": scores, "sr": sr}
    torch.cuda.current_stream(dev).synchronize()
    return out


def _sweep_tiled_u8(model, images: torch.Tensor, rates, tile: int, tile_overlap: int, tile_batch: int, bgr: bool,
                    multiple: int, window="uniform"):
    """-> (rates [R,B], tile plan, hq staging (``kdlae_tile_blend_rates``' layout), blended hq f32 [R,B,C,H,W],
    candidates u8 [R,B,h,w,C])."""
    from . import tiling
    B, h, w, _ = images.shape
    img, _ = preprocess_u8(images, None, multiple, bgr)
    rt = _rates_rb(rates, B, images.device)
    H, W = img.shape[-2:]
    with torch.no_grad():
        plan, rt, st_hq, _ = model._sweep_tiles(img, rt, False, tile, tile_overlap, tile_batch)
    hq = tiling.tile_blend_rates(st_hq, rt.shape[0], B, H, W, tile, tile_overlap, tile_batch, 1, window=window)
    cands = torch.stack([postprocess_u8(hq[r], h, w, 1, images) for r in range(rt.shape[0])])
    return rt, plan, st_hq, hq, cands


def enhance_rates_tiled_u8(model, images: torch.Tensor, rates, tile: int = 512, tile_overlap: int = 32,
                           tile_batch: int = 16, bgr: bool = False, multiple: int = 8,
                           window="uniform") -> torch.Tensor:
    """``enhance_tiled_u8``'s hq for every rate of a sweep, for images larger than one forward can hold: u8
    [B,h,w,C], R rates (scalars or [R,B]) -> u8 [R,B,h,w,C] through ``KDLAE_teacher.forward_rates_tiled``'s
    sweep.  Candidate r is byte for byte ``enhance_tiled_u8(model, images, rates[r], ...)[0]`` with the same
    ``window``."""
    return _sweep_tiled_u8(model, images, rates, tile, tile_overlap, tile_batch, bgr, multiple, window)[4]


_SCORE_CHUNK_PIXELS = 1 << 22   # pixels of one ASDQE scoring chunk: 64 images up to 256^2, one image from 2048^2


def enhance_auto_tiled_u8(model, scorer, images: torch.Tensor, rates, target=None, select: str = "closest",
                          want_sr: bool = False, tile: int = 512, tile_overlap: int = 32, tile_batch: int = 16,
                          bgr: bool = False, window="uniform") -> dict:
    """``enhance_auto_u8`` for images larger than one forward can hold: the sweep runs tiled
    (``KDLAE_teacher.forward_rates_tiled``), every post-processed full-size candidate — the blended image, not a
    tile — is scored against its input with ASDQE, and ``kdlae_rate_select`` picks per image.  With ``want_sr``
    the sr head runs on the staged, unclamped hq tiles of each image's chosen rate only (never on R times the
    tiles), ``tile_batch`` at a time, and is blended at scale 2.  ``hq`` and ``sr`` equal byte for byte
    ``enhance_tiled_u8`` called with the per-image chosen rates and the same ``window`` (it shapes both blends,
    so also the candidates that are scored).  Returns ``enhance_auto_u8``'s dict; one
    synchronisation, before the results are returned."""
    from . import tiling
    if select not in _SELECT_MODES:
        raise RuntimeError(f"select must be one of {sorted(_SELECT_MODES)}, got {select!r}")
    B, h, w, _ = images.shape
    dev = images.device
    rt, plan, st_hq, hq, cands = _sweep_tiled_u8(model, images, rates, tile, tile_overlap, tile_batch, bgr, 8,
                                                 window)
    R = rt.shape[0]
    H, W = hq.shape[-2:]
    scores = torch.empty((R, B), device=dev, dtype=torch.float32)
    chunk = max(1, min(64, _SCORE_CHUNK_PIXELS // (h * w)))   # asdqe_scores' 64, lowered for large images
    with torch.no_grad():
        for c0 in range(0, B, chunk):   # every pair is scored independently
            lq = to_tensor_u8(images[c0:c0 + chunk])
            for r in range(R):
                scores[r, c0:c0 + chunk] = scorer(lq, to_tensor_u8(cands[r, c0:c0 + chunk])).view(-1)
    index, _ = rate_select(scores, hq, select, target)
    pick = (index.long(), torch.arange(B, device=dev))
    sr = None
    if want_sr:
        n = B * plan.ni * plan.nj
        tb = min(int(tile_batch), n)
        C = hq.shape[2]
        slot = tiling.staged_slots(index, plan.ni * plan.nj, R, tile_batch)
        chosen = st_hq.view(n * R, C, plan.th, plan.tw).index_select(0, slot)
        st_sr = torch.empty((n, C, 2 * plan.th, 2 * plan.tw), device=dev, dtype=torch.float32)
        with torch.no_grad():
            for first in range(0, n, tb):
                st_sr[first:first + tb] = model.forward_sr(chosen[first:first + tb])
        sr = postprocess_u8(tiling.tile_blend(st_sr, B, H, W, tile, tile_overlap, 2, window=window), h, w, 2,
                            images)
    out = {"hq": cands[pick], "rate": rt[pick], "index": index, "scores": scores, "sr": sr}
    torch.cuda.current_stream(dev).synchronize()
    return out


def frames_preprocess_u8(frames: torch.Tensor, multiple: int = 32) -> torch.Tensor:
    """u8 frames (cuda) [B,F,h,w] (gray) or [B,F,h,w,C] (cv2 BGR / BGRA) -> f32 [B,F,H,W]."""
    if frames.device.type != "cuda" or frames.dtype != torch.uint8 or frames.dim() not in (4, 5):
        raise RuntimeError("frames_preprocess_u8 expects a cuda uint8 tensor [B,F,h,w] or [B,F,h,w,C]")
    frames = frames.contiguous()
    B, F, h, w = frames.shape[:4]
    C = frames.shape[4] if frames.dim() == 5 else 1
    H, W = padded_size(h, w, multiple)
    x = torch.empty((B, F, H, W), device=frames.device, dtype=torch.float32)
    rc = _lib.lib().kdlae_frames_preprocess_u8(ctypes.c_void_p(frames.data_ptr()), B, F, h, w, C, multiple,
                                               ctypes.c_void_p(x.data_ptr()), _stream(frames.device))
    _lib.check(rc, "kdlae_frames_preprocess_u8")
    return x


def enhance_frames_u8(model, frames: torch.Tensor, multiple: int = 32) -> torch.Tensor:
    """KDLAE-S.ipynb inference for u8 frame stacks [B,F,h,w(,C)] -> u8 [B,h,w,F] (restored frames)."""
    h, w = frames.shape[2], frames.shape[3]
    x = frames_preprocess_u8(frames, multiple)
    with torch.no_grad():
        y = model(x)
    return postprocess_u8(y, h, w, 1, None)


def enhance_clip_u8(model, clip: torch.Tensor, frames: int = 7, overlap: int = 2, window_batch: int = 8,
                    window="uniform", multiple: int = 32) -> torch.Tensor:
    """``enhance_frames_u8`` for a whole clip: u8 [B,T,h,w] (gray) or [B,T,h,w,C] (cv2 BGR / BGRA) -> u8 [B,T,h,w]
    in frame order.  One ``frames_preprocess_u8`` over the clip, ``KDLAE_student.forward_clip``'s window loop
    (``frames``, ``overlap``, ``window_batch``, ``window`` as it takes them), then ``clips.clip_blend_u8``: the
    blend, the clamp, the crop and ``img_as_ubyte`` in one launch, with no float clip-sized output and no permute.
    Byte for byte the per-window host loop followed by ``postprocess_u8`` and a permute."""
    from . import clips
    if clip.dim() not in (4, 5):
        raise RuntimeError("enhance_clip_u8 expects a cuda uint8 tensor [B,T,h,w] or [B,T,h,w,C]")
    B, T, h, w = clip.shape[:4]
    if int(window_batch) < 1:
        raise RuntimeError(f"window_batch must be at least 1, got {window_batch}")
    plan = clips.clip_plan(T, frames, overlap)   # refuses a bad T / frames / overlap before any launch
    table = clips.clip_window(window, T, frames, overlap, clip.device)   # a bad window is refused here
    x = frames_preprocess_u8(clip, multiple)
    model._check_input(x)
    with torch.no_grad():
        return clips.clip_blend_u8(model._clip_windows(x, plan, frames, overlap, window_batch), B, T, h, w, frames,
                                   overlap, table)


def distill_clip_u8(teacher, clip: torch.Tensor, denoise_rate, teacher_batch: int = 16, tile=None,
                    tile_overlap: int = 32, window="uniform") -> torch.Tensor:
    """The label folder of KDLAES.yml for one clip, without the folder: u8 [B,T,h,w] (gray) or [B,T,h,w,C] (cv2 BGR /
    BGRA) -> u8 [B,T,h,w], the gray bytes an image file of the teacher's ``enhance_u8`` output of every frame holds
    (``distill.teacher_labels_u8``: ``teacher_batch`` frames a forward, expanded and collapsed on the device)."""
    from . import distill
    return distill.teacher_labels_u8(teacher, clip, denoise_rate, teacher_batch, tile, tile_overlap, window)


def enhance_stream_u8(model, frames_iter, frames: int = 7, emit: int | None = None, multiple: int = 32):
    """``enhance_frames_u8`` for a live source: a generator over an iterable of cuda u8 frames ``[B,h,w]`` (gray) or
    ``[B,h,w,C]`` (cv2 BGR / BGRA) that yields u8 ``[B,h,w]`` frames in order, each from the window of ``frames``
    frames in which it sits at position ``emit`` (default ``frames // 2``; streams.py states the rule), with the
    flush when the iterable is exhausted: as many frames come out as went in.  The first frame fixes the shape;
    a frame that differs, a CPU tensor or another dtype raises before any launch.  ``emit = frames - 1`` yields
    every frame as it arrives."""
    from .streams import StudentStream, _check_rule
    _check_rule(frames, emit)
    stream = None
    for frame in frames_iter:
        if stream is None:
            if not isinstance(frame, torch.Tensor) or frame.device.type != "cuda" or frame.dtype != torch.uint8 or \
                    frame.dim() not in (3, 4):
                raise RuntimeError("enhance_stream_u8 expects cuda uint8 frames [B,h,w] or [B,h,w,C]")
            B, h, w = frame.shape[:3]
            stream = StudentStream(model, B, h, w, frames, emit, frame.shape[3] if frame.dim() == 4 else 1, multiple,
                                   "u8", device=frame.device)
        out = stream.push(frame)
        for k in range(out.shape[1]):
            yield out[:, k]
    if stream is not None:
        out = stream.flush()
        for k in range(out.shape[1]):
            yield out[:, k]


def to_tensor_u8(images: torch.Tensor) -> torch.Tensor:
    """torchvision ToTensor for u8 [B,h,w,C] RGB on the GPU: f32 [B,C,h,w] / 255 (no padding)."""
    img, _ = preprocess_u8(images, None, multiple=1)
    return img


def asdqe_scores(model, lq_u8: torch.Tensor, gt_u8: torch.Tensor, chunk: int = 64) -> np.ndarray:
    """ASDQE_test.py ``infer`` (:87-104) for equally sized RGB pairs u8 [N,h,w,3] -> float32 scores [N].
    The script scores one pair per forward; every pair is independent (GAP slots depend on the image
    size only), so scoring ``chunk`` pairs per forward gives the same values."""
    out = []
    with torch.no_grad():
        for c0 in range(0, lq_u8.shape[0], chunk):
            s = model(to_tensor_u8(lq_u8[c0:c0 + chunk]), to_tensor_u8(gt_u8[c0:c0 + chunk]))
            out.append(s.float().cpu().numpy().reshape(-1))
    return np.concatenate(out)


def score_statistics(values) -> dict:
    """ASDQE_test.py ``calculate_statistics`` (:107-120), on the float32 predictions as the script
    has them (np.mean / np.std of a float32 array accumulate in float32, pairwise)."""
    v = np.asarray(values)
    return {"mean": float(np.mean(v)), "std": float(np.std(v)), "min": float(np.min(v)),
            "25%": float(np.percentile(v, 25)), "50%": float(np.percentile(v, 50)),
            "75%": float(np.percentile(v, 75)), "max": float(np.max(v))}


def write_statistics_csv(stats_by_method: dict, path: str) -> None:
    """``visualize_comparison``'s transposed CSV (:123-133): rows = statistic, columns = method, %.6f."""
    methods = list(stats_by_method)
    keys = list(next(iter(stats_by_method.values())))
    with open(path, "w", newline="") as f:
        wr = csv.writer(f, lineterminator="\n")  # pandas DataFrame.to_csv line endings
        wr.writerow([""] + methods)
        for k in keys:
            wr.writerow([k] + [f"{stats_by_method[m][k]:.6f}" for m in methods])
