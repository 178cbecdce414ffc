"""Progressive-learning batch preparation on the GPU: stage schedule, sub-batch, crop, Bernoulli input mask.

Replaces the host block of the reference's training loop between the data loader and ``feed_train_data``
(Train/basicsr/train.py:374-448) and the per-frame mask rule of its KDLAE-S dataset
(Train/basicsr/data/paired_image_dataset.py:19-36,219-272).  The stage rule and every host draw (``random.sample``,
the two ``random.random()`` of the crop window, with ``rng="numpy"`` also the mask) follow the reference call for
call, so a run seeded like a reference run prepares the same batches bit for bit; gather, crop and mask are one
launch of ``kdlae_train_prepare`` (csrc/augment.hip).  There is no CPU fallback: CPU tensors raise.

    schedule = ProgressiveSchedule(iters, gt_sizes, mini_batch_sizes, probs, gt_size, batch_size, prob)
    batcher = ProgressiveBatcher(schedule)
    for it, (lq, gt) in enumerate(loader, 1):
        trainer.update_learning_rate(it)
        trainer.optimize_parameters(*trainer.feed_train_data(*batcher(it, lq, gt)))
"""
from __future__ import annotations

import ctypes
import random

import numpy as np
import torch

from . import _lib
from ._lib import PrepSeg

__all__ = ["ProgressiveSchedule", "ProgressiveBatcher", "train_prepare", "mask_frames", "interpolation_inputs",
           "test1_inputs", "train_inputs", "choice_threshold"]


def _vp(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _check(t, what, ndim=4, dtype=torch.float32):
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise RuntimeError(f"{what}: batch preparation runs on ROCm tensors only; there is no CPU fallback")
    if t.dtype != dtype or t.dim() != ndim or not t.is_contiguous():
        raise RuntimeError(f"{what}: expected a contiguous {ndim}-D {dtype} tensor, got {tuple(t.shape)} {t.dtype}"
                           f"{'' if t.is_contiguous() else ' (not contiguous)'}")
    return t


def choice_threshold(p: float) -> float:
    """The uniform draw at and above which ``np.random.choice([0, 1], p=[p, 1 - p])`` returns 1 (keep): it
    searches ``cdf = cumsum(p) / cdf[-1]`` from the right, so the threshold is ``cdf[0]`` (= p whenever
    p + (1 - p) rounds to 1.0).  ``p > 1`` is clamped like ``input_mask`` clamps it."""
    p = min(float(p), 1.0)
    cdf = np.cumsum(np.array([p, 1.0 - p], dtype=np.float64))
    cdf /= cdf[-1]
    return float(cdf[0])


def _numpy_keep(planes: int, h: int, w: int, p: float) -> np.ndarray:
    """The reference's mask draws: h * w doubles of the legacy ``numpy.random`` stream per plane, plane by plane."""
    thr = choice_threshold(p)
    return np.stack([np.random.random_sample(h * w) >= thr for _ in range(planes)]).astype(np.uint8)


class ProgressiveSchedule:
    """The progressive-learning lists of a training yml (``datasets.train``: iters, gt_sizes, mini_batch_sizes,
    probs, prob, gt_size, batch_size_per_gpu) and ``scale``.  ``stage(current_iter)`` is the reference's rule:
    ``groups = cumsum(iters)``, the first j with ``current_iter <= groups[j]``, else the last stage."""

    def __init__(self, iters, gt_sizes, mini_batch_sizes, probs, gt_size, batch_size, prob=0.0, scale=1):
        n = len(iters)
        if n == 0 or not (len(gt_sizes) == len(mini_batch_sizes) == len(probs) == n):
            raise ValueError(f"ProgressiveSchedule: iters, gt_sizes, mini_batch_sizes and probs must be non-empty lists "
                             f"of one length, got {n}, {len(gt_sizes)}, {len(mini_batch_sizes)}, {len(probs)}")
        self.iters, self.gt_sizes = list(iters), list(gt_sizes)
        self.mini_batch_sizes, self.probs = list(mini_batch_sizes), list(probs)
        self.gt_size, self.batch_size, self.prob, self.scale = gt_size, batch_size, prob, scale
        self.groups = np.cumsum(np.asarray(self.iters, dtype=np.int64))

    def stage(self, current_iter: int):
        """(j, mini_gt_size, mini_batch_size, mask_prob); mask_prob = probs[j] - prob where positive, else 0."""
        hit = np.nonzero(current_iter <= self.groups)[0]
        j = int(hit[0]) if len(hit) else len(self.groups) - 1
        mask_prob = self.probs[j] - self.prob if self.probs[j] > self.prob else 0.0
        return j, self.gt_sizes[j], self.mini_batch_sizes[j], mask_prob


def train_prepare(segments, index=None, B=None, value=0.1, seed=0, call=0):
    """One ``kdlae_train_prepare`` launch.  ``segments``: up to four dicts with ``src`` [B_src, C, Hs, Ws], ``dst``
    [B, C, h, w] (contiguous fp32 ROCm tensors; the window size is dst's), ``y0`` / ``x0`` (window offset along dim 2 /
    dim 3, default 0), ``prob`` (default 0) and ``keep`` (uint8 [B, C, h, w] or None: Philox).  ``index``: None
    (identity), a host sequence of B ints, or an int32 device tensor [B].  A host sequence is checked against every
    source's image count here and then uploaded.  A device tensor is NOT validated (reading it back would
    synchronise) and neither does the kernel: an entry outside ``[0, B_src)`` of any segment reads outside that
    source, so only hand over a device index whose range is known.  Enqueued on the current stream of dst's
    device; nothing synchronises."""
    segs = (PrepSeg * len(segments))()
    dev = None
    host_index = None
    if index is not None and not isinstance(index, torch.Tensor):
        host_index = [int(i) for i in index]
    for s, g in zip(segs, segments):
        src, dst = _check(g["src"], "train_prepare src"), _check(g["dst"], "train_prepare dst")
        keep = g.get("keep")
        if keep is not None:
            _check(keep, "train_prepare keep", dtype=torch.uint8)
            if keep.shape != dst.shape:
                raise RuntimeError(f"train_prepare: keep {tuple(keep.shape)} must have dst's shape {tuple(dst.shape)}")
        dev = dst.device if dev is None else dev
        if any(t is not None and t.device != dev for t in (src, dst, keep)):
            raise RuntimeError("train_prepare: every tensor of a call must live on one device")
        if src.shape[1] != dst.shape[1]:
            raise RuntimeError(f"train_prepare: src has {src.shape[1]} channels, dst {dst.shape[1]}")
        B = dst.shape[0] if B is None else B
        if dst.shape[0] != B:
            raise RuntimeError(f"train_prepare: every dst must hold B = {B} images, got {dst.shape[0]}")
        s.src, s.dst, s.keep = src.data_ptr(), dst.data_ptr(), keep.data_ptr() if keep is not None else None
        s.B_src, s.C, s.Hs, s.Ws = src.shape
        s.h, s.w = dst.shape[2:]
        s.y0, s.x0, s.prob = int(g.get("y0", 0)), int(g.get("x0", 0)), float(g.get("prob", 0.0))
    if host_index is not None:
        if len(host_index) != B:
            raise ValueError(f"train_prepare: index must hold B = {B} entries, got {len(host_index)}")
        for s, g in zip(segs, segments):
            bad = [i for i in host_index if not 0 <= i < s.B_src]
            if bad:
                raise IndexError(f"train_prepare: index {bad[0]} is out of range for a source of {s.B_src} images "
                                 f"{tuple(g['src'].shape)}")
        index = torch.tensor(host_index, dtype=torch.int32, device=dev)
    elif index is not None:
        if index.device != dev or index.dtype != torch.int32 or index.dim() != 1 or not index.is_contiguous() \
                or index.numel() != B:
            raise RuntimeError(f"train_prepare: index must be a contiguous int32 tensor of {B} entries on {dev}")
    with torch.cuda.device(dev):
        rc = _lib.lib().kdlae_train_prepare(segs, len(segments), _vp(index), int(B or 0), float(value), int(seed),
                                            int(call), _stream(dev))
    _lib.check(rc, "kdlae_train_prepare")


class ProgressiveBatcher:
    """``batcher(current_iter, lq, gt) -> (lq, gt)``: the progressive block of the reference's loop.

    Dict batches are the teacher's (``lq = {'img', 'denoise_rate'}``, ``gt = {'hq', 'sr'}``), tensor batches the
    student's (``[B, F, H, W]``).  In the reference's order and under its conditions: ``random.sample`` picks the
    sub-batch when ``mini_batch_size < batch_size``; two ``random.random()`` calls pick one crop window for the
    whole batch when ``mini_gt_size < gt_size`` (``x0`` along dim 2, ``y0`` along dim 3; ``hq`` is cropped at
    ``scale``, ``sr`` at 2); ``img`` (or the lq tensor) is masked with ``probs[j] - prob`` when that is positive;
    ``denoise_rate`` is cropped, never masked.  Everything lands in one ``kdlae_train_prepare`` launch.

    ``rng="numpy"`` draws the mask on the host as the reference does (``np.random.random_sample(h * w)`` per
    (image, channel) plane, in that order) and uploads it: with ``random`` and ``numpy.random`` seeded as in a
    reference run the prepared batch equals the reference's bit for bit.  ``rng="philox"`` draws nothing on the
    host: the kernel evaluates Philox4x32-10 keyed by ``seed`` with ``call = current_iter * 8`` (+ the segment
    number), reproducible but not comparable with a seeded reference run.

    The outputs are new tensors; the inputs are never written.  (The reference mutates ``train_data`` in place
    when neither the sub-batch nor the crop replaces its tensors; do not rely on that here.)
    ``last_draw = (stage, indices, x0, y0, mask_prob)`` keeps the last call's draws for logging."""

    def __init__(self, schedule: ProgressiveSchedule, rng: str = "philox", seed: int = 0, value: float = 0.1):
        if rng not in ("philox", "numpy"):
            raise ValueError(f"ProgressiveBatcher: rng must be 'philox' or 'numpy', got {rng!r}")
        self.schedule, self.rng, self.seed, self.value = schedule, rng, int(seed), float(value)
        self.last_draw = None

    def __call__(self, current_iter: int, lq, gt):
        sch = self.schedule
        j, mgs, mbs, mask_prob = sch.stage(current_iter)
        # every tensor is validated before the first draw, so a refused batch leaves the host generators alone
        if isinstance(lq, dict):
            named = [("lq['img']", lq["img"], 1)] + ([("lq['denoise_rate']", lq["denoise_rate"], 1)]
                                                     if "denoise_rate" in lq else [])
        else:
            named = [("lq", lq, 1)]
        named += [("gt['hq']", gt["hq"], sch.scale), ("gt['sr']", gt["sr"], 2)] if isinstance(gt, dict) \
            else [("gt", gt, sch.scale)]
        dev = _check(named[0][1], named[0][0]).device
        for what, t, s in named:
            if _check(t, what).device != dev:
                raise RuntimeError(f"ProgressiveBatcher: {what} is on {t.device}, the batch on {dev}")
            if t.shape[0] != sch.batch_size:    # the sub-batch indices are drawn from range(batch_size)
                raise ValueError(f"ProgressiveBatcher: the schedule's batch_size is {sch.batch_size}, {what} holds "
                                 f"{t.shape[0]} images")
            # the largest offset a draw can give is gt_size - mini_gt_size - 1: refuse a tensor that only some draws fit
            if mgs < sch.gt_size and min(t.shape[2:]) < (sch.gt_size - 1) * s:
                raise ValueError(f"ProgressiveBatcher: a {mgs * s}-pixel window drawn for gt_size {sch.gt_size} leaves "
                                 f"{what} {tuple(t.shape)}")
        indices = random.sample(range(0, sch.batch_size), k=mbs) if mbs < sch.batch_size else None
        crop = mgs < sch.gt_size
        x0 = y0 = 0
        if crop:
            x0 = int((sch.gt_size - mgs) * random.random())
            y0 = int((sch.gt_size - mgs) * random.random())
        self.last_draw = (j, indices, x0, y0, mask_prob)
        B = len(indices) if indices is not None else sch.batch_size

        segments = []

        def seg(src, s=1, prob=0.0):
            h, w = (mgs * s, mgs * s) if crop else src.shape[2:]
            dst = torch.empty((B, src.shape[1], h, w), dtype=torch.float32, device=dev)
            keep = None
            if prob > 0 and self.rng == "numpy":
                keep = torch.from_numpy(_numpy_keep(B * src.shape[1], h, w, prob).reshape(dst.shape)).to(dev)
            # the reference's x0 runs along dim 2 (rows), its y0 along dim 3 (columns)
            segments.append(dict(src=src, dst=dst, y0=x0 * s, x0=y0 * s, prob=min(prob, 1.0), keep=keep))
            return dst

        if isinstance(lq, dict):
            out_lq = {"img": seg(lq["img"], 1, mask_prob)}
            if "denoise_rate" in lq:
                out_lq["denoise_rate"] = seg(lq["denoise_rate"])
        else:
            out_lq = seg(lq, 1, mask_prob)
        if isinstance(gt, dict):
            out_gt = {"hq": seg(gt["hq"], sch.scale), "sr": seg(gt["sr"], 2)}
        else:
            out_gt = seg(gt, sch.scale)
        train_prepare(segments, indices, B, self.value, self.seed, int(current_iter) * 8)
        return out_lq, out_gt


def mask_frames(frames, probs, interpolate=False, keep=None, seed=0, call=0, value=0.1, out=None):
    """The KDLAE-S per-frame input mask over ``frames`` [B, F, H, W] (F <= 16), one ``kdlae_train_mask_frames`` launch:
    frame f is masked with ``probs[f]`` (<= 0 copies it, >= 1 masks every pixel).  ``interpolate``: F must be odd,
    and an odd frame f becomes the mask of ``0.5 * (masked[f-1] + frames[f+1])``: the reference processes the
    frames in place in increasing order, so frame f-1 is already masked when f reads it and f+1 is not.
    ``keep``: uint8 [B, F, H, W] mask (1 = keep) or None for Philox (``seed``, ``call``).  Returns a new tensor, or
    ``out`` (same shape, not ``frames``) when given; ``frames`` is never written."""
    frames = _check(frames, "mask_frames")
    B, F, H, W = frames.shape
    if len(probs) != F:
        raise ValueError(f"mask_frames: {F} frames need {F} probabilities, got {len(probs)}")
    if keep is not None:
        _check(keep, "mask_frames keep", dtype=torch.uint8)
        if keep.shape != frames.shape or keep.device != frames.device:
            raise RuntimeError(f"mask_frames: keep must be a uint8 tensor of shape {tuple(frames.shape)} on {frames.device}")
    if out is None:
        out = torch.empty_like(frames)
    elif _check(out, "mask_frames out").shape != frames.shape or out.device != frames.device:
        raise RuntimeError(f"mask_frames: out must be a tensor of shape {tuple(frames.shape)} on {frames.device}")
    cp = (ctypes.c_float * max(F, 1))(*[float(p) for p in probs])
    with torch.cuda.device(frames.device):
        rc = _lib.lib().kdlae_train_mask_frames(_vp(frames), _vp(out), B, F, H, W, cp, int(bool(interpolate)),
                                                float(value), _vp(keep), int(seed), int(call), _stream(frames.device))
    _lib.check(rc, "kdlae_train_mask_frames")
    return out


def _frames_by_item(frames, item_probs, interpolate, rng, seed, call, value, per_item):
    """The frame rule with one row of probabilities per item.  ``rng="numpy"``: one ``np.random.random_sample(H * W)``
    draw per (item, frame) in that order, as a single-worker loader running the dataset's ``__getitem__`` item after
    item draws them (a negative probability draws nothing: ``input_mask`` returns the frame unchanged).
    ``per_item`` False: every row is the same and the batch is one launch with ``call``.  ``per_item`` True: one
    launch per item into its slice of the output, item b with ``call + b``, whatever the rows turn out to be;
    ``interpolate`` may then be one flag per item."""
    if rng not in ("philox", "numpy"):
        raise ValueError(f"rng must be 'philox' or 'numpy', got {rng!r}")
    frames = _check(frames, "frames")
    B, F, H, W = frames.shape
    keep = None
    if rng == "numpy":
        keep = np.ones((B, F, H, W), np.uint8)
        for b in range(B):
            for f in range(F):
                if item_probs[b][f] >= 0:
                    keep[b, f] = _numpy_keep(1, H, W, item_probs[b][f])[0].reshape(H, W)
        keep = torch.from_numpy(keep).to(frames.device)
    rows = [[min(max(p, 0.0), 1.0) for p in row] for row in item_probs]
    if not per_item:
        return mask_frames(frames, rows[0], interpolate, keep, seed, call, value)
    out = torch.empty_like(frames)
    for b in range(B):
        mask_frames(frames[b:b + 1], rows[b], interpolate[b] if isinstance(interpolate, (list, tuple)) else interpolate,
                    keep[b:b + 1] if keep is not None else None, seed, call + b, value, out=out[b:b + 1])
    return out


def interpolation_inputs(frames, prob, rng="philox", seed=0, call=0, value=0.1):
    """Inputs of the dataset's ``interpolation`` phase (paired_image_dataset.py:260-272) for ``frames`` [B, F, H, W],
    F odd: even frames masked with ``prob``, odd frames rebuilt from their neighbours' mean and masked with
    ``prob + 0.5`` (see ``mask_frames``).  This is how KDLAE-S is evaluated as a frame interpolator.  One launch for
    the batch; ``rng="philox"`` uses ``call``."""
    F = _check(frames, "frames").shape[1]
    row = [prob + 0.5 if f % 2 == 1 else prob for f in range(F)]
    return _frames_by_item(frames, [row] * frames.shape[0], True, rng, seed, call, value, per_item=False)


def test1_inputs(frames, prob, rng="philox", seed=0, call=0, value=0.1):
    """Inputs of the dataset's ``test1`` phase (paired_image_dataset.py:253-258): per item and frame one
    ``random.random() < 0.2`` draw on the host, in the reference's order (before that frame's mask draw), picks
    ``prob + 0.6`` instead of ``prob``.  (Branch and mask draws come from different generators, so only the
    order within each matters: (item, frame) for both.)  The items differ in their probabilities, so each is a
    launch of its own; with ``rng="philox"`` item b always uses ``call + b``."""
    B, F = _check(frames, "frames").shape[:2]
    rows = [[prob + 0.6 if random.random() < 0.2 else prob for _ in range(F)] for _ in range(B)]
    return _frames_by_item(frames, rows, False, rng, seed, call, value, per_item=True)


def _train_row(F, prob):
    """One item's draws of the ``train`` phase: (per-frame probabilities, interpolate)."""
    if random.random() < 0.64:
        return [prob + 0.5 if random.random() > 0.64 else prob for _ in range(F)], False
    return [prob + 0.5 if f % 2 == 1 else prob for f in range(F)], True


def train_inputs(frames, prob, rng="philox", seed=0, call=0, value=0.1):
    """Inputs of the dataset's ``train`` phase (paired_image_dataset.py:219-241), the rule KDLAES.yml trains with, for
    ``frames`` [B, F, H, W]: per item one ``random.random() < 0.64`` draw on the host; when it holds, one
    ``random.random() > 0.64`` per frame picks ``prob + 0.5`` instead of ``prob``; otherwise the item goes through
    the interpolation rule (see ``interpolation_inputs``).  F must be odd: the reference asserts it in the
    interpolation branch, which any item may take, and here it is checked before the first draw.  The draws come
    in the reference's order, (item, frame); each item is a launch of its own, item b with ``call + b``."""
    B, F = _check(frames, "frames").shape[:2]
    if rng not in ("philox", "numpy"):
        raise ValueError(f"rng must be 'philox' or 'numpy', got {rng!r}")
    if F % 2 == 0:
        raise ValueError(f"train_inputs: the interpolation branch needs an odd frame count, got {F}")
    rows = [_train_row(F, prob) for _ in range(B)]
    return _frames_by_item(frames, [r for r, _ in rows], [i for _, i in rows], rng, seed, call, value, per_item=True)


test1_inputs.__test__ = False  # the name is the reference's phase; keep pytest from collecting it where imported
