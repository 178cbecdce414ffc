"""numpy float64 restatement of the reference's two SSIM flavours (test infrastructure, CPU only).

``ssim_basicsr`` restates ``calculate_ssim`` -> ``_ssim_3d`` (Train/basicsr/metrics/psnr_ssim.py:146-197,
240-318): an 11 x 11 x 11 Gaussian Conv3d with replicate padding over the (H, W, C) volume, written here as
three separable passes with clamped indices (along C that is a C x C matrix).  ``ssim_valid`` restates
``calculate_ssim`` of Train/utils.py:31-78: per channel, valid positions only, L = 255.  ``reduce`` gives the
four numbers the HIP kernel returns over the window it is asked for.  tests/test_ssim.py pins both to numbers
recorded from the reference's own functions (tests/golden/metrics_ssim.json).

The reference runs ``_ssim_3d`` in fp32; everything here is float64, like the kernel.
"""
import numpy as np

from tests.metrics_oracle import to_uint8, window

TILE = 16   # csrc/ssim.hip kTile: one block's tile of map positions


def taps():
    """cv2.getGaussianKernel(11, 1.5): exp(-(i - 5)^2 / (2 * 1.5^2)), normalised to sum 1."""
    i = np.arange(11, dtype=np.float64) - 5.0
    g = np.exp(-(i * i) / (2.0 * 1.5 * 1.5))
    return g / g.sum()


def channel_matrix(C):
    """The Conv3d along a replicate-padded axis of length C: M[c][c'] = sum of g[t], clamp(c + t - 5) == c'."""
    g, M = taps(), np.zeros((C, C), dtype=np.float64)
    for c in range(C):
        for t in range(11):
            M[c, min(max(c + t - 5, 0), C - 1)] += g[t]
    return M


def _filter_axis(x, axis, replicate):
    """11 taps along ``axis``: replicate-padded (same length) or valid positions only (length - 10)."""
    g, n = taps(), x.shape[axis]
    x = np.moveaxis(x, axis, -1)
    if replicate:
        idx = np.clip(np.arange(n)[:, None] + np.arange(11)[None, :] - 5, 0, n - 1)
    else:
        idx = np.arange(n - 10)[:, None] + np.arange(11)[None, :]
    return np.moveaxis(x[..., idx] @ g, -1, axis)


def _map(f, a, b, L):
    """The SSIM map from a moment operator ``f`` (linear, applied to x, y, x^2, y^2, xy)."""
    C1, C2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    mu1, mu2 = f(a), f(b)
    mu1_sq, mu2_sq, mu1_mu2 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1, s2, s12 = f(a * a) - mu1_sq, f(b * b) - mu2_sq, f(a * b) - mu1_mu2
    return ((2 * mu1_mu2 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))


def map_basicsr(a, b, L):
    """[C, H, W] float64 -> the [C, H, W] map of _ssim_3d with the constants of peak ``L``."""
    M = channel_matrix(a.shape[0])

    def f(x):  # squares and products come in already formed: the mix is applied to them, not squared itself
        x = _filter_axis(_filter_axis(x, 1, True), 2, True)
        return np.einsum("cd,dhw->chw", M, x)

    return _map(f, a, b, L)


def map_valid(a, b):
    """[C, H, W] float64 -> the [C, H - 10, W - 10] map of Train/utils.py's ssim, L = 255."""
    return _map(lambda x: _filter_axis(_filter_axis(x, 1, False), 2, False), a, b, 255.0)


def _operands(pred, gt, valid_hw, crop_border, use_image):
    a, b = window(np.asarray(pred), valid_hw, crop_border), window(np.asarray(gt), valid_hw, crop_border)
    if use_image:
        a, b = to_uint8(a), to_uint8(b)
    return a.astype(np.float64), b.astype(np.float64)


def reduce(pred, gt, valid_hw=None, crop_border=0, use_image=False, variant="basicsr"):
    """One image [C, Hs, Ws] -> (sum of the map with L = 1, sum with L = 255, max of pred, entries)."""
    a, b = _operands(pred, gt, valid_hw, crop_border, use_image)
    if variant == "basicsr":
        m1, m255 = map_basicsr(a, b, 1.0), map_basicsr(a, b, 255.0)
        return float(m1.sum()), float(m255.sum()), float(a.max()), float(m1.size)
    m = map_valid(a, b)
    return 0.0, float(m.sum()), float(a.max()), float(m.size)


def ssim(pred, gt, valid_hw=None, crop_border=0, use_image=False, variant="basicsr"):
    """What the reference's function returns for one image [C, Hs, Ws] over the window (and what validate()
    reports): ``basicsr`` picks L by the first operand's maximum, ``valid`` averages the channels' means."""
    a, b = _operands(pred, gt, valid_hw, crop_border, use_image)
    if variant == "basicsr":
        return float(map_basicsr(a, b, 1.0 if a.max() <= 1 else 255.0).mean())
    return float(np.mean([map_valid(a[c:c + 1], b[c:c + 1]).mean() for c in range(a.shape[0])]))


def cases(seed=20250820):
    """The seeded inputs of the golden file: name -> (img1 [C,H,W] float32, img2, crop_border, use_image,
    variants).  Textured operands (rand, and rand + 0.05 randn clipped); ``*_u8`` twins go through the uint8
    route.  ``variants`` lists the flavours a case is defined for (``valid`` needs 11 x 11 after the crop)."""
    rng = np.random.RandomState(seed)
    out = {}
    both = ("basicsr", "valid")
    for name, (c, h, w), cb, var in (
            ("c1_1x1", (1, 1, 1), 0, ("basicsr",)),                  # everything is replicate
            ("c1_7x13", (1, 7, 13), 0, ("basicsr",)),                # window smaller than the halo
            ("c3_7x13", (3, 7, 13), 0, ("basicsr",)),
            ("c1_11x11", (1, 11, 11), 0, both),                      # valid: exactly one map entry
            ("c3_40x56_cb4", (3, 40, 56), 4, both),
            ("c3_tile_plus_1", (3, TILE + 1, TILE + 1), 0, both),    # basicsr: 2 x 2 tiles, the last 1 wide
            ("c3_tile_plus_11", (3, TILE + 11, TILE + 11), 0, both),  # valid: a 17 x 17 map, 2 x 2 tiles
            ("c4_19x23", (4, 19, 23), 0, both),
            ("c2_12x30", (2, 12, 30), 0, both)):
        a = rng.rand(c, h, w).astype(np.float32)
        b = np.clip(a + 0.05 * rng.randn(c, h, w), 0, 1).astype(np.float32)
        if (h, w) == (1, 1):
            # A single map entry with variance exactly 0: SSIM = (2ab + C1) / (a^2 + b^2 + C1) in closed form
            # (tests/test_ssim.py checks the oracle against that).  The reference's fp32 Conv3d leaves about
            # 1e-6 x^2 of noise where the 0 should be, against C2 = 9e-4, and nothing averages it out: at
            # x near 1 its own number is off by 7e-3.  A dark pixel keeps that noise at 1e-6 relative, so the
            # recorded golden is meaningful (0.1 and 0.08: the two pixels stay apart after the uint8 route).
            a, b = (a * np.float32(0.1)).astype(np.float32), (b * np.float32(0.08)).astype(np.float32)
        out[name] = (a, b, cb, False, var)
        out[name + "_u8"] = (a, b, cb, True, var)
    a = rng.rand(3, 12, 16).astype(np.float32)
    out["equal"] = (a, a.copy(), 0, False, both)
    b = np.clip(a * 0.5 + 0.05 * rng.randn(3, 12, 16), 0, 1).astype(np.float32)
    a1 = a.copy()
    a1[0, 0, 0] = 1.0
    a1 = np.minimum(a1, np.float32(1.0))
    out["max_one"] = (a1, b, 0, False, both)        # L = 1 ...
    a2 = a1.copy()
    a2[0, 0, 0] = np.nextafter(np.float32(1.0), np.float32(2.0))
    out["max_above_one"] = (a2, b, 0, False, both)  # ... and one ulp later L = 255
    for name in ("equal", "max_one", "max_above_one"):
        x, y, cb, _, var = out[name]
        out[name + "_u8"] = (x, y, cb, True, var)
    return out


def batch(seed=20250821):
    """A B = 3 batch of distinct images: ([3, 3, 20, 28] float32, same)."""
    rng = np.random.RandomState(seed)
    a = rng.rand(3, 3, 20, 28).astype(np.float32)
    b = np.clip(a + np.array([0.02, 0.05, 0.1]).reshape(3, 1, 1, 1) * rng.randn(3, 3, 20, 28), 0, 1).astype(np.float32)
    return a, b
