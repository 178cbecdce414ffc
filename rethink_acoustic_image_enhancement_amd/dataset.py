"""Dataset sample transforms on the GPU: pad, crop, noise, flips / rotations, layout, normalisation.

Replaces the per-sample numpy / cv2 work of the reference's two training datasets between image decode and the
batch (Train/basicsr/data/paired_image_dataset.py: ``Dataset_SuperRestoration_param.__getitem__`` :902-982 for the
teacher, ``Dataset_PairedMutiImage.__getitem__`` :160-294 for the student) for decoded frames that are resident
on the device.  Every host draw (``random`` and ``numpy.random``) is made sample by sample in the reference's
order, so with ``rng="numpy"`` a run seeded like a reference run yields the same batches bit for bit; the pixels
move in ``kdlae_data_sample`` / ``kdlae_data_count`` / ``kdlae_data_finish`` (csrc/data.hip).  There is no CPU
fallback: CPU tensors raise.

    teacher = TeacherSampleTransform(gt_size=128)
    lq, gt = teacher(lq_u8, gt_u8, sr_u8, rates)          # lists of [H, W, 3] u8 BGR ROCm tensors
    trainer.feed_train_data(*batcher(it, lq, gt))         # augment.ProgressiveBatcher
"""
from __future__ import annotations

import ctypes
import random

import numpy as np
import torch

from . import _lib, augment
from ._lib import DataItem

__all__ = ["sample_transform", "count_zeros_ones", "finish", "TeacherSampleTransform", "StudentSampleTransform",
           "lower_ops", "lower_data_augmentation", "lower_sync_augment", "dihedral_code", "PAD_MODES"]

PAD_MODES = {"none": 0, "reflect101": 1, "symmetric": 2}


# ------------------------------------------------------------------ the dihedral vocabulary
def lower_ops(ops):
    """A chain of ``flipud`` / ``fliplr`` / ``transpose`` / ``rot90ccw`` (np.rot90) / ``rot90cw`` / ``rot180`` applied
    left to right -> the one (transpose, flip_rows, flip_cols) triple with
    ``out = transpose?(flip_cols?(flip_rows?(window)))``."""
    t = fr = fc = False
    for op in ops:
        for prim in {"rot90ccw": ("fliplr", "transpose"), "rot90cw": ("transpose", "fliplr"),
                     "rot180": ("flipud", "fliplr")}.get(op, (op,)):
            if prim == "transpose":
                t = not t
            elif prim == "flipud":        # rows of a transposed array are the window's columns
                fr, fc = (fr, not fc) if t else (not fr, fc)
            elif prim == "fliplr":
                fr, fc = (not fr, fc) if t else (fr, not fc)
            else:
                raise ValueError(f"lower_ops: unknown operation {op!r}")
    return t, fr, fc


def lower_data_augmentation(mode: int):
    """``data_augmentation(image, mode)`` (data/transforms.py:223-268), modes 0..7."""
    if mode not in range(8):
        raise ValueError(f"data_augmentation mode must be 0..7, got {mode!r}")
    return lower_ops(((), ("rot90ccw",), ("rot180",), ("rot90cw",))[mode // 2] + (("flipud",) if mode % 2 else ()))


def lower_sync_augment(hflip: bool, vflip: bool, rot):
    """``sync_augment`` (paired_image_dataset.py:1056-1082): cv2.flip(.., 1)?, cv2.flip(.., 0)?, then a rotation by
    ``rot`` in (None, 90 clockwise, 180, 270 = 90 counter-clockwise)."""
    if rot not in (None, 90, 180, 270):
        raise ValueError(f"sync_augment rotation must be None, 90, 180 or 270, got {rot!r}")
    return lower_ops((("fliplr",) if hflip else ()) + (("flipud",) if vflip else ())
                     + {None: (), 90: ("rot90cw",), 180: ("rot180",), 270: ("rot90ccw",)}[rot])


def dihedral_code(transpose, flip_rows, flip_cols) -> int:
    return 4 * bool(transpose) + 2 * bool(flip_rows) + bool(flip_cols)


# ------------------------------------------------------------------ checked wrappers over the three entry points
def _vp(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _dev(t, what):
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise RuntimeError(f"{what}: the dataset transforms run on ROCm tensors only; there is no CPU fallback")
    return t


def _vec(t, what, n, dev, dtype=torch.float32):
    if t is None:
        return None
    if _dev(t, what).device != dev or t.dtype != dtype or t.numel() != n or not t.is_contiguous():
        raise RuntimeError(f"{what}: expected {n} contiguous {dtype} entries on {dev}, got {tuple(t.shape)} {t.dtype} "
                           f"on {t.device}")
    return t


def sample_transform(items, seed=0, call=0):
    """One ``kdlae_data_sample`` launch.  ``items``: dicts, one source image and one destination slot each:

    * ``src``: u8 or fp32 ROCm tensor, ``[H, W, C]`` / ``[H, W]`` with ``layout="hwc"`` (default for u8) or
      ``[C, H, W]`` / ``[H, W]`` with ``layout="chw"`` (default for fp32); any strides (views are fine);
    * ``dst``: contiguous fp32 ``[C, h', w']`` (a view into a batch is fine), not overlapping ``src``;
    * ``canvas`` (Hc, Wc): centre zero pad, default the source size; ``padded`` (Hp, Wp) with ``pad_mode``
      ``"reflect101"`` / ``"symmetric"``: bottom / right pad of that canvas, default none;
    * ``window`` (top, left, h, w) on the padded canvas, default all of it;
    * ``dihedral``: a (transpose, flip_rows, flip_cols) triple (``lower_*``) or its code 0..7; ``bgr2rgb``;
    * ``noise``: None or a dict ``loc``, ``scale``, ``div`` (default 1): ``x + (loc + scale * z / div)`` in fp64,
      clipped to [0, 1]; ``z``: fp64 ``[h, w, C]`` at the window coordinates before the dihedral map, or absent for
      Philox (``seed``, ``call`` + item number); ``counts`` (int32 [2] of ``count_zeros_ones``), ``thr``, ``n``:
      apply only when ``max(counts) / n > thr``, decided on the device;
    * ``mean`` / ``std``: fp32 ``[C]`` ROCm tensors or None, by destination channel.

    Everything is validated before the launch (the tensors here, the geometry by the entry point); enqueued on the
    current stream of the first dst's device; nothing synchronises."""
    if len(items) == 0:
        raise ValueError("sample_transform: no items")
    table = (DataItem * len(items))()
    dev = _dev(items[0]["dst"], "sample_transform dst").device
    for k, (it, g) in enumerate(zip(table, items)):
        what = f"sample_transform item {k}"
        src, dst = _dev(g["src"], what + " src"), _dev(g["dst"], what + " dst")
        if src.device != dev or dst.device != dev:
            raise RuntimeError(f"{what}: every tensor of a call must live on one device")
        if src.dtype not in (torch.uint8, torch.float32) or src.dim() not in (2, 3):
            raise RuntimeError(f"{what}: src must be a 2-D or 3-D u8 or fp32 tensor, got {tuple(src.shape)} {src.dtype}")
        layout = g.get("layout", "hwc" if src.dtype == torch.uint8 else "chw")
        if layout not in ("hwc", "chw"):
            raise ValueError(f"{what}: layout must be 'hwc' or 'chw', got {layout!r}")
        s3 = src.unsqueeze(2 if layout == "hwc" else 0) if src.dim() == 2 else src
        (Hs, Ws, C), (sy, sx, sc) = (s3.shape, s3.stride()) if layout == "hwc" else \
            ((s3.shape[1], s3.shape[2], s3.shape[0]), (s3.stride(1), s3.stride(2), s3.stride(0)))
        Hc, Wc = g.get("canvas", (Hs, Ws))
        Hp, Wp = g.get("padded", (Hc, Wc))
        mode = g.get("pad_mode", "none")
        if mode not in PAD_MODES:
            raise ValueError(f"{what}: pad_mode must be one of {sorted(PAD_MODES)}, got {mode!r}")
        top, left, h, w = g.get("window", (0, 0, Hp, Wp))
        d = g.get("dihedral", 0)
        code = dihedral_code(*d) if isinstance(d, (tuple, list)) else int(d)
        if not 0 <= code <= 7:
            raise ValueError(f"{what}: dihedral code must be 0..7, got {code}")
        ho, wo = (w, h) if code & 4 else (h, w)
        if dst.dtype != torch.float32 or tuple(dst.shape) != (C, ho, wo) or not dst.is_contiguous():
            raise RuntimeError(f"{what}: dst must be a contiguous fp32 tensor of shape {(C, ho, wo)}, got "
                               f"{tuple(dst.shape)} {dst.dtype}")
        it.src, it.dst = src.data_ptr(), dst.data_ptr()
        it.sy, it.sx, it.sc = sy, sx, sc
        it.src_u8 = int(src.dtype == torch.uint8)
        it.Hs, it.Ws, it.C, it.Hc, it.Wc, it.Hp, it.Wp = Hs, Ws, C, int(Hc), int(Wc), int(Hp), int(Wp)
        it.pad_mode, it.top, it.left, it.h, it.w = PAD_MODES[mode], int(top), int(left), int(h), int(w)
        it.dihedral, it.reverse_c = code, int(bool(g.get("bgr2rgb", False)))
        nz = g.get("noise")
        if nz is not None:
            z = nz.get("z")
            if z is not None and (_dev(z, what + " z").device != dev or z.dtype != torch.float64
                                  or tuple(z.shape) != (h, w, C) or not z.is_contiguous()):
                raise RuntimeError(f"{what}: z must be a contiguous fp64 tensor of shape {(h, w, C)} on {dev}, got "
                                   f"{tuple(z.shape)} {z.dtype}")
            it.noise, it.z = (1, z.data_ptr()) if z is not None else (2, None)
            it.loc, it.scale, it.div = float(nz.get("loc", 0.0)), float(nz["scale"]), float(nz.get("div", 1.0))
            counts = _vec(nz.get("counts"), what + " counts", 2, dev, torch.int32)
            if counts is not None:
                it.counts, it.count_thr, it.count_n = counts.data_ptr(), float(nz["thr"]), int(nz["n"])
        mean, std = _vec(g.get("mean"), what + " mean", C, dev), _vec(g.get("std"), what + " std", C, dev)
        it.mean, it.std = (mean.data_ptr() if mean is not None else None), (std.data_ptr() if std is not None else None)
    dtab = torch.empty(ctypes.sizeof(table), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.lib().kdlae_data_sample(table, _vp(dtab), len(items), int(seed), int(call), _stream(dev))
    _lib.check(rc, "kdlae_data_sample")


def count_zeros_ones(x, out=None):
    """int32 ``[B, 2]``: per sample of the contiguous fp32 ``x [B, ...]`` the number of elements == 0 and == 1
    (``kdlae_data_count``; -0.0 counts as zero, as ``== 0`` does in numpy).  ``out`` is overwritten when given."""
    if _dev(x, "count_zeros_ones").dtype != torch.float32 or x.dim() < 2 or not x.is_contiguous():
        raise RuntimeError(f"count_zeros_ones: expected a contiguous fp32 tensor [B, ...], got {tuple(x.shape)} {x.dtype}")
    B = x.shape[0]
    out = torch.empty((B, 2), dtype=torch.int32, device=x.device) if out is None else \
        _vec(out, "count_zeros_ones out", 2 * B, x.device, torch.int32)
    with torch.cuda.device(x.device):
        rc = _lib.lib().kdlae_data_count(_vp(x), B, x.numel() // max(B, 1), _vp(out), _stream(x.device))
    _lib.check(rc, "kdlae_data_count")
    return out


def finish(x, counts, thr, nudge=1e-14, mean=None, std=None):
    """In place over the contiguous fp32 ``x [B, C, H, W]`` (``kdlae_data_finish``): a sample with
    ``max(counts[b]) / (C * H * W) > thr`` gets ``x + nudge`` (one fp32 add), then ``(x - mean[c]) / std[c]``."""
    if _dev(x, "finish").dtype != torch.float32 or x.dim() != 4 or not x.is_contiguous():
        raise RuntimeError(f"finish: expected a contiguous fp32 tensor [B, C, H, W], got {tuple(x.shape)} {x.dtype}")
    B, C, H, W = x.shape
    counts = _vec(counts, "finish counts", 2 * B, x.device, torch.int32)
    if counts is None:
        raise RuntimeError("finish: counts is None")
    mean, std = _vec(mean, "finish mean", C, x.device), _vec(std, "finish std", C, x.device)
    with torch.cuda.device(x.device):
        rc = _lib.lib().kdlae_data_finish(_vp(x), B, C, H * W, _vp(counts), float(thr), float(nudge), _vp(mean),
                                          _vp(std), _stream(x.device))
    _lib.check(rc, "kdlae_data_finish")
    return x


def _rng(rng, who):
    if rng not in ("philox", "numpy"):
        raise ValueError(f"{who}: rng must be 'philox' or 'numpy', got {rng!r}")
    return rng


def _images(lst, what, ndim, dev=None):
    for k, t in enumerate(lst):
        if _dev(t, f"{what}[{k}]").dtype != torch.uint8 or t.dim() != ndim or (ndim == 3 and t.shape[2] != 3):
            raise RuntimeError(f"{what}[{k}]: expected a u8 tensor {'[H, W, 3]' if ndim == 3 else '[H, W]'}, got "
                               f"{tuple(t.shape)} {t.dtype}")
        dev = t.device if dev is None else dev
        if t.device != dev:
            raise RuntimeError(f"{what}[{k}] is on {t.device}, the batch on {dev}")
    return dev


# ------------------------------------------------------------------ teacher
class TeacherSampleTransform:
    """``Dataset_SuperRestoration_param.__getitem__`` (train phase) for a batch of decoded samples.

    ``transform(lq_u8, gt_u8, sr_u8, denoise_rate)``: lists of per-sample ``[H, W, 3]`` u8 ROCm tensors in BGR as
    ``imfrombytes`` yields them (``sr`` at twice the size) and one float (or None: 1) per sample; returns
    ``({'img', 'denoise_rate'}, {'hq', 'sr'})`` batched, ready for ``ProgressiveBatcher`` / ``feed_train_data``.
    Per sample, in the reference's order: reflect-101 pad up to ``gt_size``; ``random.randint(1, h - 1 - gt_size)``
    twice (the offsets start at 1; an image smaller than ``gt_size + 2`` is refused, as ``randint`` refuses it);
    ``np.random.uniform() < 0.1`` -> ``np.random.uniform(1, 30)`` and Gaussian noise on ``lq`` at the pre-flip
    coordinates; with ``geometric_augs`` ``random.random()`` twice and ``random.choice([None, 90, 180, 270])``; the
    all-0 / all-1 nudge; BGR -> RGB, CHW; ``(x - mean) / std``.  ``rng="numpy"`` draws ``np.random.randn(h, w, 3)`` on
    the host as the reference does and uploads it; ``rng="philox"`` draws only the scalars.  One
    ``kdlae_data_sample`` launch for the batch, then ``kdlae_data_count`` and ``kdlae_data_finish`` on ``img``; nothing
    synchronises.  ``last_draw`` keeps the per-sample draws (top, left, sigma | None, hflip, vflip, rot)."""

    def __init__(self, gt_size, geometric_augs=True, mean=None, std=None, rng="philox", seed=0):
        self.rng = _rng(rng, "TeacherSampleTransform")
        if int(gt_size) <= 0:
            raise ValueError(f"TeacherSampleTransform: gt_size must be positive, got {gt_size}")
        for name, v in (("mean", mean), ("std", std)):
            if v is not None and len(v) != 3:
                raise ValueError(f"TeacherSampleTransform: {name} must hold 3 entries, got {len(v)}")
        self.gt_size, self.geometric_augs, self.seed = int(gt_size), bool(geometric_augs), int(seed)
        self.mean, self.std = mean, std
        self.calls, self.last_draw, self._stats = 0, None, {}

    def _stat(self, v, dev):
        if v is None:
            return None
        if (id(v), dev) not in self._stats:
            self._stats[(id(v), dev)] = torch.tensor([float(a) for a in v], dtype=torch.float32, device=dev)
        return self._stats[(id(v), dev)]

    def __call__(self, lq_u8, gt_u8, sr_u8, denoise_rate):
        g, B = self.gt_size, len(gt_u8)
        if B == 0 or not (len(lq_u8) == len(sr_u8) == len(denoise_rate) == B):
            raise ValueError(f"TeacherSampleTransform: lq, gt, sr and denoise_rate must be non-empty lists of one length, "
                             f"got {len(lq_u8)}, {B}, {len(sr_u8)}, {len(denoise_rate)}")
        dev = _images(gt_u8, "gt", 3)
        _images(lq_u8, "lq", 3, dev)
        _images(sr_u8, "sr", 3, dev)
        for b in range(B):
            H, W = gt_u8[b].shape[:2]
            if tuple(lq_u8[b].shape) != (H, W, 3) or tuple(sr_u8[b].shape) != (2 * H, 2 * W, 3):
                raise ValueError(f"TeacherSampleTransform: sample {b}: gt is {H}x{W}, so lq must be {H}x{W} and sr "
                                 f"{2 * H}x{2 * W}, got {tuple(lq_u8[b].shape[:2])} and {tuple(sr_u8[b].shape[:2])}")
            if max(H, g) - 1 - g < 1 or max(W, g) - 1 - g < 1:
                raise ValueError(f"TeacherSampleTransform: sample {b} is {H}x{W}; random.randint(1, size - 1 - gt_size) "
                                 f"needs at least {g + 2} pixels each way")
        rates = torch.tensor([1.0 if r is None else float(r) for r in denoise_rate], dtype=torch.float64)
        mean, std = self._stat(self.mean, dev), self._stat(self.std, dev)
        img = torch.empty((B, 3, g, g), dtype=torch.float32, device=dev)
        hq, sr = torch.empty_like(img), torch.empty((B, 3, 2 * g, 2 * g), dtype=torch.float32, device=dev)
        items, draws = [], []
        for b in range(B):
            H, W = gt_u8[b].shape[:2]
            Hp, Wp = max(H, g), max(W, g)
            top, left = random.randint(1, Hp - 1 - g), random.randint(1, Wp - 1 - g)
            noise = sigma = None
            if np.random.uniform() < 0.1:
                sigma = np.random.uniform(1, 30)
                noise = dict(loc=0.0, scale=sigma, div=255.0)
                if self.rng == "numpy":
                    noise["z"] = torch.from_numpy(np.random.randn(g, g, 3)).to(dev)
            hflip = vflip = False
            rot = None
            if self.geometric_augs:
                hflip, vflip = random.random() < 0.5, random.random() < 0.5
                rot = random.choice([None, 90, 180, 270])
            d = lower_sync_augment(hflip, vflip, rot)
            draws.append((top, left, sigma, hflip, vflip, rot))
            for src, dst, s, nz, m, sd in ((lq_u8[b], img[b], 1, noise, None, None), (gt_u8[b], hq[b], 1, None, mean, std),
                                           (sr_u8[b], sr[b], 2, None, mean, std)):
                items.append(dict(src=src, dst=dst, padded=(Hp * s, Wp * s), dihedral=d, bgr2rgb=True, noise=nz,
                                  pad_mode="reflect101" if (Hp, Wp) != (H, W) else "none", mean=m, std=sd,
                                  window=(top * s, left * s, g * s, g * s)))
        self.last_draw = draws
        sample_transform(items, self.seed, self.calls << 16)
        self.calls += 1
        finish(img, count_zeros_ones(img), 0.10, 1e-14, mean, std)
        rate = rates.to(torch.float32).to(dev).view(B, 1, 1, 1).expand(B, 1, g, g).contiguous()
        return {"img": img, "denoise_rate": rate}, {"hq": hq, "sr": sr}


# ------------------------------------------------------------------ student
class StudentSampleTransform:
    """``Dataset_PairedMutiImage.__getitem__`` (train phase) for a batch of decoded bursts.

    ``transform(lq_frames, gt_frames)``: per sample a list of F grey u8 ``[H_f, W_f]`` ROCm tensors each; returns
    ``(lq, gt)`` fp32 ``[B, F, gt_size, gt_size]``.  Per sample, in the reference's order: centre zero pad of every
    frame to the burst's largest gt frame (``pad_image``); symmetric pad up to ``gt_size`` (``padding``);
    ``paired_random_crop`` (``random.randint`` twice); the train-phase frame mask rule (as ``augment.train_inputs``);
    ``add_random_noise`` (loc 0.3, scale 0.7) when more than 64 % of the stack is exactly 0 or exactly 1; with
    ``geometric_augs`` ``random.randint(0, 7)`` and that ``data_augmentation`` mode on both stacks.  Two
    ``kdlae_data_sample`` launches (u8 frames -> cropped planes; noise + dihedral map), ``kdlae_train_mask_frames`` and
    ``kdlae_data_count`` between them.

    ``rng="philox"`` synchronises nowhere: the noise condition is evaluated on the device from the counts.
    ``rng="numpy"`` reproduces a seeded reference run bit for bit, and for that it works sample by sample and READS
    THE COUNTS BACK (one synchronisation per sample): the host generator advances only when the noise is drawn,
    and the next sample's mask draws come after it in the same stream.  ``last_draw``: per sample (top, left, mode)."""

    def __init__(self, gt_size, prob, geometric_augs=True, rng="philox", seed=0):
        self.rng = _rng(rng, "StudentSampleTransform")
        if int(gt_size) <= 0:
            raise ValueError(f"StudentSampleTransform: gt_size must be positive, got {gt_size}")
        self.gt_size, self.prob, self.geometric_augs, self.seed = int(gt_size), float(prob), bool(geometric_augs), int(seed)
        self.calls, self.last_draw = 0, None

    def __call__(self, lq_frames, gt_frames):
        B = len(gt_frames)
        if B == 0 or len(lq_frames) != B:
            raise ValueError(f"StudentSampleTransform: lq and gt must be non-empty lists of one length, got "
                             f"{len(lq_frames)} and {B}")
        F, dev, sizes = len(gt_frames[0]), None, []
        if F % 2 == 0 or F > 16:
            raise ValueError(f"StudentSampleTransform: the train-phase frame rule needs an odd number of frames <= 16, "
                             f"got {F}")
        for b in range(B):
            if len(gt_frames[b]) != F or len(lq_frames[b]) != F:
                raise ValueError(f"StudentSampleTransform: sample {b} holds {len(lq_frames[b])} lq and "
                                 f"{len(gt_frames[b])} gt frames, the batch {F}")
            dev = _images(gt_frames[b], f"gt[{b}]", 2, dev)
            _images(lq_frames[b], f"lq[{b}]", 2, dev)
            Hc, Wc = max(t.shape[0] for t in gt_frames[b]), max(t.shape[1] for t in gt_frames[b])
            if any(t.shape[0] > Hc or t.shape[1] > Wc for t in lq_frames[b]):
                raise ValueError(f"StudentSampleTransform: sample {b}: an lq frame is larger than the largest gt frame "
                                 f"{Hc}x{Wc}")
            sizes.append((Hc, Wc))
        self.last_draw = []
        groups = [[b] for b in range(B)] if self.rng == "numpy" else [list(range(B))]
        lq = torch.empty((B, F, self.gt_size, self.gt_size), dtype=torch.float32, device=dev)
        gt = torch.empty_like(lq)
        for grp in groups:
            self._run(grp, lq_frames, gt_frames, sizes, lq, gt, dev)
        self.calls += 1
        return lq, gt

    def _run(self, grp, lq_frames, gt_frames, sizes, lq_out, gt_out, dev):
        g, n, F = self.gt_size, len(grp), lq_out.shape[1]
        x1 = torch.empty((n, F, g, g), dtype=torch.float32, device=dev)
        y1 = torch.empty_like(x1)
        items, rows, modes = [], [], []
        for k, b in enumerate(grp):
            # this sample's `random` draws, in the reference's order: crop, frame rule, augmentation mode
            Hc, Wc = sizes[b]
            Hp, Wp = max(Hc, g), max(Wc, g)
            top, left = random.randint(0, Hp - g), random.randint(0, Wp - g)
            rows.append(augment._train_row(F, self.prob))
            modes.append(random.randint(0, 7) if self.geometric_augs else 0)
            self.last_draw.append((top, left, modes[-1]))
            for frames, dst in ((lq_frames[b], x1[k]), (gt_frames[b], y1[k])):
                for f in range(F):
                    items.append(dict(src=frames[f], dst=dst[f:f + 1], canvas=(Hc, Wc), padded=(Hp, Wp),
                                      pad_mode="symmetric" if (Hp, Wp) != (Hc, Wc) else "none", window=(top, left, g, g)))
        base = (self.calls << 20) + (grp[0] << 8)
        sample_transform(items, self.seed, base)
        masked = augment._frames_by_item(x1, [r for r, _ in rows], [i for _, i in rows], self.rng, self.seed,
                                         base + (1 << 19), 0.1, per_item=True)
        counts = count_zeros_ones(masked)
        host = counts.cpu().tolist() if self.rng == "numpy" else None   # the documented read-back
        items = []
        for k, b in enumerate(grp):
            noise = dict(loc=0.3, scale=0.7, counts=counts[k], thr=0.64, n=F * g * g)
            if host is not None:
                noise = None
                if max(host[k]) / (F * g * g) > 0.64:
                    noise = dict(loc=0.3, scale=0.7, z=torch.from_numpy(np.random.standard_normal((g, g, F))).to(dev))
            d = lower_data_augmentation(modes[k])
            items.append(dict(src=masked[k], dst=lq_out[b], dihedral=d, noise=noise))
            items.append(dict(src=y1[k], dst=gt_out[b], dihedral=d))
        sample_transform(items, self.seed, base + (1 << 18))
