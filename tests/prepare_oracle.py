"""numpy model of the progressive-learning batch preparation (Train/basicsr/train.py:374-448) and of the KDLAE-S
per-frame input mask (Train/basicsr/data/paired_image_dataset.py:19-36,219-272).

Pinned to goldens recorded from the reference's own statements (tests/golden/make_golden_prepare.py) by
tests/test_prepare.py; the GPU tests compare ``kdlae_train_prepare`` / ``kdlae_train_mask_frames`` with it bit for
bit.  Everything a kernel computes is modelled in fp32 (the only arithmetic is the interpolation's add and
multiply); the reference's float64 detour ``x * m - 0.1 + 0.1 * m`` rounds back to the fp32 ``x`` for a kept pixel
and to ``float32(-0.1)`` for a masked one, which the goldens confirm.
"""
import random

import numpy as np

from rethink_acoustic_image_enhancement_amd.hashweights import hash_images

VALUE = 0.1


# ------------------------------------------------------------------ stage rule and host draws
def stage(iters, gt_sizes, mini_batch_sizes, probs, prob, current_iter):
    """(j, mini_gt_size, mini_batch_size, mask_prob): groups = cumsum(iters), the first j with
    current_iter <= groups[j], else the last; mask_prob = probs[j] - prob where that is positive, else 0."""
    groups = np.cumsum(np.asarray(iters, dtype=np.int64))
    hit = np.nonzero(current_iter <= groups)[0]
    j = int(hit[0]) if len(hit) else len(groups) - 1
    mask_prob = probs[j] - prob if probs[j] > prob else 0.0
    return j, gt_sizes[j], mini_batch_sizes[j], mask_prob


def draw(mini_gt_size, mini_batch_size, gt_size, batch_size):
    """The reference's ``random`` calls, in its order and under its conditions: (indices | None, x0, y0).
    x0 is the offset along dim 2 and y0 the one along dim 3 (the reference's names)."""
    indices = random.sample(range(0, batch_size), k=mini_batch_size) if mini_batch_size < batch_size else None
    x0 = y0 = 0
    if mini_gt_size < gt_size:
        x0 = int((gt_size - mini_gt_size) * random.random())
        y0 = int((gt_size - mini_gt_size) * random.random())
    return indices, x0, y0


def choice_threshold(p):
    """``np.random.choice([0, 1], p=[p, 1 - p])`` keeps a pixel when ``u >= cdf[0]`` with cdf = cumsum(p) / cdf[-1]
    (searchsorted side='right'); cdf[-1] is 1.0 for every probability of the released configs, so this is p."""
    p = min(float(p), 1.0)
    cdf = np.cumsum(np.array([p, 1.0 - p], dtype=np.float64))
    cdf /= cdf[-1]
    return cdf[0]


def numpy_keep(planes, h, w, p):
    """One ``np.random.random_sample`` draw of h * w doubles per plane, in plane order: uint8 [planes, h, w]."""
    thr = choice_threshold(p)
    return np.stack([(np.random.random_sample(h * w) >= thr).reshape(h, w) for _ in range(planes)]).astype(np.uint8)


# ------------------------------------------------------------------ Philox4x32-10
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: uint32 array [..., 4], key: two uint32 -> uint32 array [..., 4] (Random123's Philox4x32-10)."""
    c = [np.asarray(counter)[..., i].astype(np.uint64) for i in range(4)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & _MASK, p1 >> np.uint64(32), p1 & _MASK
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return np.stack(c, axis=-1).astype(np.uint32)


def philox_words(n, seed, call):
    """Word of every element e < n: block q = e // 4 with counter (q lo, q hi, call lo, call hi), word e % 4."""
    q = np.arange((n + 3) // 4, dtype=np.uint64)
    ctr = np.stack([q & _MASK, q >> np.uint64(32), np.full_like(q, call & 0xFFFFFFFF),
                    np.full_like(q, (call >> 32) & 0xFFFFFFFF)], axis=-1)
    return philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)).reshape(-1)[:n]


def philox_keep(shape, prob, seed, call):
    """uint8 keep mask of a dst of ``shape``: u = (word >> 8) * 2^-24 and u >= prob, both in fp32."""
    n = int(np.prod(shape))
    u = (philox_words(n, seed, call) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return (u >= np.float32(prob)).astype(np.uint8).reshape(shape)


# ------------------------------------------------------------------ gather / crop / mask
def _resolve_keep(shape, prob, keep, seed, call):
    """The kernels' mode rule: prob <= 0 keeps all, prob >= 1 none, else the given bytes or Philox."""
    prob = np.float32(prob)
    if not prob > 0:
        return np.ones(shape, np.uint8)
    if prob >= 1:
        return np.zeros(shape, np.uint8)
    return (np.asarray(keep) != 0).astype(np.uint8).reshape(shape) if keep is not None \
        else philox_keep(shape, prob, seed, call)


def prepare(src, index, y0, x0, h, w, prob=0.0, keep=None, value=VALUE, seed=0, call=0):
    """dst[b, c, i, j] = keep ? src[index[b], c, y0 + i, x0 + j] : float32(-value) for one segment."""
    src = np.asarray(src, np.float32)
    sub = src if index is None else src[np.asarray(index, np.int64)]
    win = np.ascontiguousarray(sub[:, :, y0:y0 + h, x0:x0 + w])
    assert win.shape[2:] == (h, w), "window leaves the source"
    k = _resolve_keep(win.shape, prob, keep, seed, call)
    return np.where(k != 0, win, -np.float32(value)).astype(np.float32)


def mask_frames(src, probs, interpolate=False, keep=None, value=VALUE, seed=0, call=0):
    """[B, F, H, W]: frame f masked with probs[f]; interpolating, an odd f starts from
    float32(masked[f-1] + src[f+1]) * 0.5 (frames are processed in place in increasing order)."""
    src = np.asarray(src, np.float32)
    B, F, H, W = src.shape
    assert not interpolate or F % 2 == 1
    fill = -np.float32(value)
    u = None  # the Philox uniforms of every element, drawn on first use
    out = src.copy()
    for f in range(F):
        p = np.float32(probs[f])
        if not p > 0:
            k = np.ones((B, H, W), np.uint8)
        elif p >= 1:
            k = np.zeros((B, H, W), np.uint8)
        elif keep is not None:
            k = (np.asarray(keep).reshape(src.shape)[:, f] != 0).astype(np.uint8)
        else:
            if u is None:
                u = ((philox_words(src.size, seed, call) >> np.uint32(8)).astype(np.float32)
                     * np.float32(2.0 ** -24)).reshape(src.shape)
            k = (u[:, f] >= p).astype(np.uint8)
        base = out[:, f]
        if interpolate and f % 2 == 1:
            base = (out[:, f - 1] + src[:, f + 1]).astype(np.float32) * np.float32(0.5)
        out[:, f] = np.where(k != 0, base, fill)
    return out


# ------------------------------------------------------------------ the whole progressive block, numpy route
def progressive(cfg, current_iter, lq, gt, value=VALUE):
    """The reference block with ``random`` / ``numpy.random`` as they are seeded by the caller.
    cfg: dict(iters, gt_sizes, mini_batch_sizes, probs, prob, gt_size, batch_size, scale).
    lq / gt: dict of arrays ({'img', 'denoise_rate'}, {'hq', 'sr'}) or plain arrays.  Returns
    (lq, gt, (j, indices, x0, y0, mask_prob)); the inputs are not written."""
    j, mgs, mbs, mp = stage(cfg["iters"], cfg["gt_sizes"], cfg["mini_batch_sizes"], cfg["probs"], cfg["prob"],
                            current_iter)
    indices, x0, y0 = draw(mgs, mbs, cfg["gt_size"], cfg["batch_size"])
    crop = mgs < cfg["gt_size"]

    def seg(a, s, prob=0.0, keep=None):
        a = np.asarray(a, np.float32)
        h, w = (mgs * s, mgs * s) if crop else a.shape[2:]
        return prepare(a, indices, x0 * s, y0 * s, h, w, prob, keep, value)

    def masked(a):
        a = np.asarray(a, np.float32)
        B = a.shape[0] if indices is None else len(indices)
        h, w = (mgs, mgs) if crop else a.shape[2:]
        keep = numpy_keep(B * a.shape[1], h, w, mp).reshape(B, a.shape[1], h, w) if mp > 0 else None
        return seg(a, 1, min(mp, 1.0) if keep is not None else 0.0, keep)

    if isinstance(lq, dict):
        out_lq = {"img": masked(lq["img"])}
        if "denoise_rate" in lq:
            out_lq["denoise_rate"] = seg(lq["denoise_rate"], 1)
    else:
        out_lq = masked(lq)
    if isinstance(gt, dict):
        out_gt = {"hq": seg(gt["hq"], cfg["scale"]), "sr": seg(gt["sr"], 2)}
    else:
        out_gt = seg(gt, cfg["scale"])
    return out_lq, out_gt, (j, indices, x0, y0, mp)


# ------------------------------------------------------------------ golden cases (tests/golden/make_golden_prepare.py)
def _img(tag, shape):
    return hash_images("prepare/" + tag, shape)


def progressive_cases():
    """name -> (cfg, current_iter, py_seed, np_seed, lq, gt); small tensors, every branch of the block."""
    def dict_batch(tag, B, S):
        return ({"img": _img(tag + "/img", (B, 3, S, S)), "denoise_rate": _img(tag + "/rate", (B, 1, S, S))},
                {"hq": _img(tag + "/hq", (B, 3, S, S)), "sr": _img(tag + "/sr", (B, 3, 2 * S, 2 * S))})

    base = dict(iters=[2, 3, 4], gt_sizes=[8, 12, 12], mini_batch_sizes=[2, 4, 3], probs=[0.3, 0.2, 0.1], prob=0,
                gt_size=12, batch_size=4, scale=1)
    out = {}
    for name, cfg, it, py_seed, np_seed in (
            ("dict_sub_crop_mask", base, 2, 11, 12),                       # stage 0: 4 -> 2 images, 12 -> 8, p 0.3
            ("dict_full", base, 3, 13, 14),                                # stage 1: nothing drawn by `random`
            ("dict_sub_only", base, 9, 15, 16),                            # stage 2: 4 -> 3 images, no crop
            ("dict_beyond_last", base, 100, 17, 18),                       # past the last group: stage 2
            ("dict_nomask", dict(base, prob=0.3), 1, 19, 20),              # probs[0] == prob: crop, no mask
            ("dict_prob_offset", dict(base, prob=0.1), 1, 21, 22),         # masked with 0.3 - 0.1
            ("dict_prob_above_one", dict(base, probs=[1.5, 0.2, 0.1]), 1, 23, 24)):
        out[name] = (cfg, it, py_seed, np_seed, *dict_batch(name, 4, 12))
    # the trainer-integration shape (6 -> 2 images, 32^2 -> 16^2)
    integ = dict(iters=[5, 5], gt_sizes=[16, 32], mini_batch_sizes=[2, 6], probs=[0.2, 0.1], prob=0, gt_size=32,
                 batch_size=6, scale=1)
    out["dict_trainer_step"] = (integ, 1, 25, 26, *dict_batch("dict_trainer_step", 6, 32))
    tens = dict(iters=[4, 4], gt_sizes=[8, 12], mini_batch_sizes=[2, 4], probs=[0.25, 0.4], prob=0, gt_size=12,
                batch_size=4, scale=1)
    out["tensor_sub_crop_mask"] = (tens, 4, 27, 28, _img("tensor_sub_crop_mask/lq", (4, 3, 12, 12)),
                                   _img("tensor_sub_crop_mask/gt", (4, 3, 12, 12)))
    out["tensor_full"] = (tens, 5, 29, 30, _img("tensor_full/lq", (4, 7, 12, 12)),
                          _img("tensor_full/gt", (4, 7, 12, 12)))
    return out


def frame_cases():
    """name -> (phase, prob, py_seed, np_seed, frames [B, F, H, W]); each item goes through the dataset block on
    its own HWC stack, one after the other, as a single-worker loader would fetch them."""
    out = {}
    for phase in ("interpolation", "test1"):
        for F in (1, 3, 7):
            for (H, W) in ((4, 5), (8, 8)):
                name = f"{phase}_f{F}_{H}x{W}"
                out[name] = (phase, 0.3, 100 + len(out), 200 + len(out), _img(name, (2, F, H, W)))
        for tag, prob, shape in (("clamped_f3_8x8", 0.6, (2, 3, 8, 8)), ("prob0_f3_4x5", 0.0, (2, 3, 4, 5))):
            out[f"{phase}_{tag}"] = (phase, prob, 100 + len(out), 200 + len(out),
                                     _img(f"{phase}_{tag.split('_')[0]}", shape))
    return out
