"""numpy model of the reference's NIQE (test infrastructure, CPU only, no scipy).

``calculate_niqe`` of Train/basicsr/metrics/niqe.py:10-205 (with ``to_y_channel``, metric_util.py:34-47, and
``bgr2ycbcr``, utils/matlab_functions.py:207-238) for [C, H, W] float32 images in RGB order, in two arithmetic
modes:

* ``like_reference``  the per-block statistics as numpy forms them there: float32 means of float32 maps;
* ``float64``         the statistics from exact fp64 moments of the same float32 maps (counts, sums of squares on
                      either side of zero, sum of magnitudes): what csrc/niqe.hip returns and
                      ``metrics.finish_niqe`` finishes.

The MSCN field is the same in both modes and is written out tap by tap: scipy's ``convolve`` walks the flipped
7 x 7 window in row-major order, multiplies and adds in float64 (two roundings per tap) and rounds the sum once
to float32; ``mode='nearest'`` is an index clamp.  The 2 x rescale between the scales is the 2 x 2 mean OpenCV
documents for INTER_LINEAR at exactly one half (``half``); parity with a real cv2 build is not pinned.

``mutant=`` switches in one deliberate mistake (tests/test_niqe.py shows that each moves a compared quantity).
tests/test_niqe.py pins this file to numbers recorded from the reference's own function (tests/golden/niqe.*).
"""
import functools
import math
import os

import numpy as np

BLOCK = 96
SHIFTS = ((0, 1), (1, 0), (1, 1), (1, -1))
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MUTANTS = ("clamp_storage", "crop_ignored", "roll_nowrap", "shift_sign", "block_order", "products_fp64",
           "zeros_positive", "abs_nonzero", "scale2_unscaled", "scale2_block96")


def params(path=None):
    d = np.load(path or os.path.join(GOLDEN, "niqe_pris_params.npz"))
    return {k: np.asarray(d[k]) for k in ("mu_pris_param", "cov_pris_param", "gaussian_window")}


# ------------------------------------------------------------------ image -> Y -> field
def to_uint8(x):
    """tensor2img's quantisation (clamp to [0, 1], * 255 in fp32, round half to even), kept as float32."""
    return np.rint(np.clip(x, 0, 1).astype(np.float32) * np.float32(255.0)).astype(np.float32)


def to_y(x):
    """[C, H, W] float32 on the 0..255 scale, RGB -> the float32 Y of ``to_y_channel``: / 255 in fp32, the
    BT.601 row over (B, G, R) in float64 (products added left to right), + 16, / 255, rounded to fp32, * 255."""
    x = x.astype(np.float32) / np.float32(255.0)
    if x.shape[0] == 3:
        r, g, b = (x[c].astype(np.float64) for c in range(3))
        y = ((b * 24.966 + g * 128.553) + r * 65.481 + 16.0) / 255.0
        x = y.astype(np.float32)
    elif x.shape[0] == 1:
        x = x[0]
    else:
        raise ValueError("NIQE takes 1 or 3 channels")
    return x * np.float32(255.0)


def prepare(x, crop_border=0, use_image=False, mutant=None):
    """-> the [H', W'] float32 image the two scales start from (H', W' multiples of 96)."""
    x = np.asarray(x, dtype=np.float32)
    y = to_y(to_uint8(x) if use_image else x)
    cb = 0 if mutant == "crop_ignored" else int(crop_border)
    y = y[cb:y.shape[0] - cb, cb:y.shape[1] - cb]
    return np.ascontiguousarray(y[:y.shape[0] // BLOCK * BLOCK, :y.shape[1] // BLOCK * BLOCK])


def _filter(img, window):
    """scipy.ndimage.convolve(img, window, mode='nearest') for float32 ``img``: see the module docstring."""
    w = np.asarray(window, dtype=np.float64)[::-1, ::-1]
    H, W = img.shape
    x = img.astype(np.float64)
    acc = np.zeros((H, W), dtype=np.float64)
    for a in range(7):
        rows = np.clip(np.arange(H) + a - 3, 0, H - 1)
        for b in range(7):
            cols = np.clip(np.arange(W) + b - 3, 0, W - 1)
            acc = acc + w[a, b] * x[rows][:, cols]
    return acc.astype(np.float32)


def mscn(img, window):
    """niqe.py:111-117: (img - mu) / (sigma + 1), float32 throughout after the two filters."""
    img = np.asarray(img, dtype=np.float32)
    mu = _filter(img, window)
    sigma = np.sqrt(np.abs(_filter(np.square(img), window) - np.square(mu)))
    return (img - mu) / (sigma + np.float32(1.0))


def half(img, mutant=None):
    """The stand-in for cv2.resize(img / 255., (w // 2, h // 2), INTER_LINEAR) * 255. on even sizes: the mean
    of each 2 x 2 cell, horizontal pairs first, every operation rounded once in fp32."""
    y = img.astype(np.float32) / np.float32(255.0)
    h = (y[:, 0::2] + y[:, 1::2]) * np.float32(0.5)
    v = (h[0::2] + h[1::2]) * np.float32(0.5)
    return v if mutant == "scale2_unscaled" else v * np.float32(255.0)


def fields(x, crop_border=0, use_image=False, window=None, mutant=None, storage=None):
    """-> (field at scale 1 [H', W'], field at scale 2 [H'/2, W'/2]).  ``storage`` (mutant clamp_storage only):
    the larger array the image sits in, top-left."""
    y = prepare(x, crop_border, use_image, mutant)
    if mutant == "clamp_storage":
        full = to_y(to_uint8(storage if storage is not None else x) if use_image else
                    np.asarray(storage if storage is not None else x, dtype=np.float32))
        cb = int(crop_border)
        with np.errstate(all="ignore"):
            f1 = mscn(full, window)[cb:cb + y.shape[0], cb:cb + y.shape[1]]
        return np.ascontiguousarray(f1), mscn(half(y), window)
    return mscn(y, window), mscn(half(y, mutant), window)


# ------------------------------------------------------------------ blocks and maps
def block_grid(shape, scale, mutant=None):
    """Block origins in the reference's order (idx_w outer) and the block side at this scale."""
    bs = BLOCK if mutant == "scale2_block96" else BLOCK // scale
    nbh, nbw = shape[0] * scale // BLOCK, shape[1] * scale // BLOCK
    if mutant == "scale2_block96" and scale == 2:
        nbh, nbw = shape[0] // BLOCK, shape[1] // BLOCK
    if mutant == "block_order":
        return [(i * bs, j * bs) for i in range(nbh) for j in range(nbw)], bs
    return [(i * bs, j * bs) for j in range(nbw) for i in range(nbh)], bs


def block_maps(f, y0, x0, bs, mutant=None):
    """The five float32 maps of one block: the field and its products with itself rolled inside the block."""
    blk = f[y0:y0 + bs, x0:x0 + bs]
    out = [blk]
    for (s0, s1) in SHIFTS:
        if mutant == "shift_sign" and (s0, s1) == (1, -1):
            s1 = 1
        if mutant == "roll_nowrap":
            rows = np.clip(np.arange(y0, y0 + bs) - s0, 0, f.shape[0] - 1)
            cols = np.clip(np.arange(x0, x0 + bs) - s1, 0, f.shape[1] - 1)
            other = f[rows][:, cols]
        else:
            other = np.roll(blk, (s0, s1), axis=(0, 1))
        if mutant == "products_fp64":
            out.append(blk.astype(np.float64) * other.astype(np.float64))
        else:
            out.append(blk * other)
    return out


def moments(f, scale, mutant=None):
    """[blocks][5 maps][n_neg, n_pos, sum x^2 over x < 0, sum x^2 over x > 0, sum |x|] in float64, and the
    sum of the magnitudes of the terms of each sum ([blocks][5][3]; here the sums themselves, all terms being
    >= 0)."""
    grid, bs = block_grid(f.shape, scale, mutant)
    out = np.zeros((len(grid), 5, 5), dtype=np.float64)
    for k, (y0, x0) in enumerate(grid):
        for m, x in enumerate(block_maps(f, y0, x0, bs, mutant)):
            x = x.astype(np.float64).ravel()
            neg, pos = x[x < 0], x[x >= 0] if mutant == "zeros_positive" else x[x > 0]
            out[k, m] = (neg.size, pos.size, np.sum(neg * neg), np.sum(pos * pos), np.sum(np.abs(x)))
    return out


# ------------------------------------------------------------------ the AGGD fit
@functools.lru_cache(maxsize=None)
def gamma_table():
    """gam = arange(0.2, 10.001, 0.001) and Gamma(2/g)^2 / (Gamma(1/g) Gamma(3/g)), through math.lgamma."""
    gam = np.arange(0.2, 10.001, 0.001)
    rec = np.reciprocal(gam)
    r = np.array([math.exp(2.0 * math.lgamma(2.0 * t) - math.lgamma(t) - math.lgamma(3.0 * t)) for t in rec])
    return gam, r


def _g(a):
    return math.exp(math.lgamma(a))


def _fit(left_std, right_std, mean_abs, mean_sq):
    """estimate_aggd_param from the four statistics (numpy scalars of the mode's precision) -> alpha, beta_l,
    beta_r and the margin of the argmin (distance of rhatnorm from the nearer midpoint between table entries,
    relative to rhatnorm)."""
    gam, r_gam = gamma_table()
    with np.errstate(all="ignore"):
        gammahat = left_std / right_std
        rhat = mean_abs ** 2 / mean_sq
        rhatnorm = (rhat * (gammahat ** 3 + 1) * (gammahat + 1)) / ((gammahat ** 2 + 1) ** 2)
        pos = int(np.argmin((r_gam - rhatnorm) ** 2))
        alpha = gam[pos]
        scale = np.sqrt(_g(1 / alpha) / _g(3 / alpha))
        margin = np.inf
        if np.isfinite(rhatnorm):
            r = float(rhatnorm)
            mids = [(r_gam[p] + r_gam[p + 1]) / 2 for p in (pos - 1, pos) if 0 <= p < len(gam) - 1]
            margin = min(abs(r - m) for m in mids) / abs(r)
        return alpha, left_std * scale, right_std * scale, margin


def _stats_like_reference(x, mutant=None):
    x = x.ravel()
    with np.errstate(all="ignore"):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            pos = x[x >= 0] if mutant == "zeros_positive" else x[x > 0]
            mean_abs = np.mean(np.abs(x[x != 0])) if mutant == "abs_nonzero" else np.mean(np.abs(x))
            return (np.sqrt(np.mean(x[x < 0] ** 2)), np.sqrt(np.mean(pos ** 2)), mean_abs, np.mean(x ** 2))


def _stats_from_moments(row, n, mutant=None):
    n_neg, n_pos, s_neg, s_pos, s_abs = (np.float64(v) for v in row)
    with np.errstate(all="ignore"):
        n_abs = n_neg + n_pos if mutant == "abs_nonzero" else np.float64(n)
        return (np.sqrt(s_neg / n_neg), np.sqrt(s_pos / n_pos), s_abs / n_abs, (s_neg + s_pos) / np.float64(n))


def _features(stats5):
    """18 features of one block from the statistics of its five maps -> (features, smallest margin)."""
    feat, margin = [], np.inf
    for m, st in enumerate(stats5):
        alpha, bl, br, mg = _fit(*st)
        margin = min(margin, mg)
        if m == 0:
            feat += [alpha, (bl + br) / 2]
        else:
            feat += [alpha, (br - bl) * (_g(2 / alpha) / _g(1 / alpha)), bl, br]
    return feat, margin


def features_from_moments(mom, bs, mutant=None):
    """[blocks, 18] float64 from [blocks, 5, 5] moments of bs x bs blocks, and the smallest argmin margin."""
    rows, margin = [], np.inf
    for k in range(mom.shape[0]):
        feat, mg = _features([_stats_from_moments(mom[k, m], bs * bs, mutant) for m in range(5)])
        rows.append([float(v) for v in feat])
        margin = min(margin, mg)
    return np.array(rows, dtype=np.float64).reshape(mom.shape[0], 18), margin


def features(f, scale, mode="float64", mutant=None):
    """[blocks, 18] float64 for one scale's field and the smallest argmin margin over blocks and maps."""
    grid, bs = block_grid(f.shape, scale, mutant)
    if mode == "float64":
        return features_from_moments(moments(f, scale, mutant), bs, mutant)
    rows, margin = [], np.inf
    for (y0, x0) in grid:
        feat, mg = _features([_stats_like_reference(x, mutant) for x in block_maps(f, y0, x0, bs, mutant)])
        rows.append([float(v) for v in feat])
        margin = min(margin, mg)
    return np.array(rows, dtype=np.float64).reshape(len(grid), 18), margin


def score(feat36, p):
    """niqe.py:142-153 from the [blocks, 36] features; nan when fewer than two rows are free of NaN (the
    reference raises from pinv there)."""
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        mu = np.nanmean(feat36, axis=0)
    good = feat36[~np.isnan(feat36).any(axis=1)]
    if good.shape[0] < 2 or np.isnan(mu).any():
        return float("nan")
    cov = np.cov(good, rowvar=False)
    inv = np.linalg.pinv((p["cov_pris_param"] + cov) / 2)
    d = p["mu_pris_param"] - mu
    return float(np.sqrt(np.matmul(np.matmul(d, inv), np.transpose(d))).reshape(-1)[0])


def niqe(x, crop_border=0, use_image=False, p=None, mode="float64", mutant=None, storage=None, detail=False):
    p = p or params()
    f1, f2 = fields(x, crop_border, use_image, p["gaussian_window"], mutant, storage)
    a, m1 = features(f1, 1, mode, mutant)
    b, m2 = features(f2, 2, mode, mutant)
    n = min(a.shape[0], b.shape[0])
    feat = np.concatenate([a[:n], b[:n]], axis=1)
    s = score(feat, p)
    return (s, feat, (f1, f2), min(m1, m2)) if detail else s


def score_from_moments(m1, m2, p):
    """The float64 mode's score from the two scales' moments ([blocks, 5, 5] each)."""
    a, _ = features_from_moments(np.asarray(m1, dtype=np.float64), BLOCK)
    b, _ = features_from_moments(np.asarray(m2, dtype=np.float64), BLOCK // 2)
    return score(np.concatenate([a, b], axis=1), p)


# ------------------------------------------------------------------ the GPU test's inputs
def _noise(rng, shape, lo=0.0, hi=255.0):
    return rng.uniform(lo, hi, size=shape).astype(np.float32)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (x [C, H, W] float32, crop_border, use_image).  use_image cases are on the 0..1 scale (they go
    through the uint8 quantisation), the others on 0..255."""
    rng = np.random.RandomState(20251020)
    out = {}
    out["noise_c1_192x96"] = (_noise(rng, (1, 192, 96)), 0, False)
    yy, xx = np.mgrid[0:192, 0:192].astype(np.float32)
    ramp = (0.2 + 0.6 * (0.7 * xx + 0.3 * yy) / 192.0)[None] + rng.normal(0, 0.04, (3, 192, 192))
    out["ramp_c3_192x192_u8"] = (ramp.astype(np.float32), 0, True)
    for cb in (0, 4):
        # sonar-like: speckle over a dark fan, one whole block (and its halo) of exact zeros
        yy, xx = np.mgrid[0:200, 0:300].astype(np.float32)
        fan = 90.0 + 70.0 * np.sin(xx / 23.0) * np.cos(yy / 31.0)
        img = np.clip(fan * rng.rayleigh(0.8, (200, 300)), 0, 255).astype(np.float32)
        img[:108, :108] = 0.0
        out[f"sonar_c1_200x300_cb{cb}"] = (img[None], cb, False)
    sat = np.clip(0.45 + 0.2 * rng.standard_normal((3, 200, 300)), 0, 1).astype(np.float32)
    sat[:, 60:150, 100:220] = 1.0 + rng.uniform(0, 0.2, (3, 90, 120))   # saturates at 255 in every channel
    out["sat_c3_200x300_cb4_u8"] = (sat.astype(np.float32), 4, True)
    out["noise_c3_192x96"] = (_noise(rng, (3, 192, 96)), 0, False)
    out["sat_c1_192x192_u8"] = (np.clip(0.5 + 0.3 * rng.standard_normal((1, 192, 192)), -0.2, 1.2).astype(np.float32),
                                0, True)
    return out


@functools.lru_cache(maxsize=None)
def batch():
    """Three distinct [1, 192, 96] images on the 0..255 scale."""
    rng = np.random.RandomState(20251021)
    x = _noise(rng, (3, 1, 192, 96))
    x[1] = np.clip(x[1] * 0.3 + 100.0, 0, 255)
    x[2, :, 40:90, 10:70] = 255.0
    return x


@functools.lru_cache(maxsize=None)
def reference(name):
    """(score, features, (f1, f2), margin, (m1, m2)) of a case in the float64 mode, computed once."""
    x, cb, use_image = cases()[name]
    s, feat, (f1, f2), margin = niqe(x, cb, use_image, detail=True)
    return s, feat, (f1, f2), margin, (moments(f1, 1), moments(f2, 2))


def perturbed_score_change(name, rel=1e-11, seed=7):
    """|score change| when every sum of the case's moments moves by up to ``rel`` relative (seeded)."""
    s, _, _, _, (m1, m2) = reference(name)
    rng = np.random.RandomState(seed)
    p = params()
    worst = 0.0
    for _ in range(4):
        q = []
        for m in (m1, m2):
            m = m.copy()
            m[..., 2:] *= 1.0 + rel * rng.choice([-1.0, 1.0], size=m[..., 2:].shape)
            q.append(m)
        worst = max(worst, abs(score_from_moments(q[0], q[1], p) - s))
    return worst
