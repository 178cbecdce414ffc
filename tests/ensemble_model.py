"""The self-ensemble rule of include/kdlae_ensemble.h in numpy: the transforms, the slot layout of
kdlae_ens_gather / kdlae_ens_merge, the chunk plan, and the mistakes a hand-written loop makes.

Mode m: T_m(x) = flipud^(m % 2)(rot90ccw^(m // 2)(x)) on the last two axes.  Slots: one dense [N, C, H', W'] block
per mode of the mask in ascending order, flat, slot s at float s N C H W.  Merge: per pixel 0 + U_m0 + U_m1 + ... in
ascending mode order, every add rounded to fp32, then one fp32 division by float(|M|)."""
import numpy as np

MODES = tuple(range(8))
NAMED = {"d8": MODES, "flips": (0, 1, 4, 5)}


def mask_of(modes):
    modes = NAMED[modes] if isinstance(modes, str) else modes
    mask = 0
    for m in modes:
        assert m in MODES
        mask |= 1 << m
    return mask


def modes_of(mask):
    assert 1 <= mask <= 255
    return [m for m in MODES if (mask >> m) & 1]


def transform(x, m):
    """T_m on the last two axes."""
    out = np.rot90(x, k=m // 2, axes=(-2, -1))
    return np.flip(out, axis=-2) if m % 2 else out


def inverse(u, m):
    """T_m^-1: undo the flip, then turn back."""
    out = np.flip(u, axis=-2) if m % 2 else u
    return np.rot90(out, k=-(m // 2), axes=(-2, -1))


def view_shape(m, H, W):
    return (W, H) if (m // 2) % 2 else (H, W)


def gather(x, mask):
    """x [N, C, H, W] float32 -> the flat slot layout."""
    return np.concatenate([np.ascontiguousarray(transform(x, m)).reshape(-1) for m in modes_of(mask)])


def views(buf, N, C, H, W, mask):
    per = N * C * H * W
    return [buf[s * per:(s + 1) * per].reshape(N, C, *view_shape(m, H, W)) for s, m in enumerate(modes_of(mask))]


def merge(buf, N, C, H, W, mask, order="ascending", inverse_fn=inverse, divisor=None):
    """The flat slot layout of per-view outputs -> [N, C, H, W].  `order`, `inverse_fn` and `divisor` exist for
    the planted mistakes: the rule is the defaults."""
    modes = modes_of(mask)
    us = [np.ascontiguousarray(inverse_fn(v, m)) for v, m in zip(views(buf, N, C, H, W, mask), modes)]
    if order == "descending":
        us = us[::-1]
    acc = np.zeros((N, C, H, W), np.float32)
    for u in us:
        assert u.dtype == np.float32 and u.shape == acc.shape
        acc = (acc + u).astype(np.float32)
    return (acc / np.float32(len(modes) if divisor is None else divisor)).astype(np.float32)


def chunks(mask, H, W, ens_batch):
    """(first slot, slots, view shape): runs of at most ens_batch consecutive slots of one shape."""
    shapes = [view_shape(m, H, W) for m in modes_of(mask)]
    out, s = [], 0
    while s < len(shapes):
        n = 1
        while s + n < len(shapes) and n < ens_batch and shapes[s + n] == shapes[s]:
            n += 1
        out.append((s, n, shapes[s]))
        s += n
    return out


def ensemble(f, x, rate, mask, transform_rate=True, transform_fn=transform, **merge_kw):
    """The whole rule for a model f(img, rate) -> output of the image's shape, through gather / merge."""
    N, C, H, W = x.shape
    outs = []
    for m in modes_of(mask):
        a = np.ascontiguousarray(transform_fn(x, m))
        if transform_rate:
            r = np.ascontiguousarray(transform(rate, m))
        else:   # the mistake: the map as it came (a square image, or it would not even fit)
            assert a.shape[-2:] == rate.shape[-2:]
            r = rate
        outs.append(np.ascontiguousarray(f(a, r), dtype=np.float32).reshape(-1))
    return merge(np.concatenate(outs), N, C, H, W, mask, **merge_kw)


# ------------------------------------------------------------------ the planted mistakes
def inverse_wrong_way(u, m):
    """The inverse rotation taken the same way as the forward one."""
    out = np.flip(u, axis=-2) if m % 2 else u
    return np.rot90(out, k=m // 2, axes=(-2, -1))


def transform_flip_first(x, m):
    """The flip applied before the rotation."""
    out = np.flip(x, axis=-2) if m % 2 else x
    return np.rot90(out, k=m // 2, axes=(-2, -1))


def planted_sum_order(N=1, C=1, H=3, W=5):
    """Staged outputs for the mask {0, 3, 6} (one shape-preserving and two transposing modes) holding 1, 1e8 and
    -1e8 at every pixel.  Ascending: fl(fl(fl(0 + 1) + 1e8) - 1e8) = 0 (the 1 is below half an ulp of 1e8), so
    the answer is 0 / 3 = 0.  Descending: fl(fl(fl(0 - 1e8) + 1e8) + 1) = 1, so 1 / 3.  Returns (mask, flat
    staged buffer)."""
    mask = mask_of((0, 3, 6))
    vals = (np.float32(1.0), np.float32(1e8), np.float32(-1e8))
    return mask, np.concatenate([np.full(N * C * H * W, v, np.float32) for v in vals])
