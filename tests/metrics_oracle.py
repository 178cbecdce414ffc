"""numpy float64 restatement of the reference's PSNR (test infrastructure, CPU only).

``psnr`` restates Train/basicsr/metrics/psnr_ssim.py:53-70 for CHW float arrays, ``to_uint8``
tensor2img's quantisation (Train/basicsr/utils/img_util.py:67-68,91-94).  ``reduce`` gives the two
reductions the HIP kernel returns (sum of squared differences and the first operand's maximum) over the
window the kernel is asked for.  tests/test_metrics.py pins ``psnr`` to numbers recorded from the
reference's own ``calculate_psnr`` (tests/golden/metrics_psnr.json).
"""
import numpy as np


def to_uint8(x):
    """clamp_(0, 1) in fp32, * 255.0 in fp32, np.round (half to even), astype(uint8)."""
    x = np.clip(np.asarray(x, dtype=np.float32), np.float32(0), np.float32(1))
    return (x * 255.0).round().astype(np.uint8)


def window(x, valid_hw=None, crop_border=0):
    """[..., Hs, Ws] -> the top-left valid window minus crop_border on its four sides."""
    h, w = x.shape[-2:] if valid_hw is None else valid_hw
    x = x[..., :h, :w]
    if crop_border != 0:
        x = x[..., crop_border:-crop_border, crop_border:-crop_border]
    return x


def reduce(pred, gt, valid_hw=None, crop_border=0, use_image=False):
    """One image [C, Hs, Ws] -> (sse, max of pred, n) in float64."""
    a, b = window(np.asarray(pred), valid_hw, crop_border), window(np.asarray(gt), valid_hw, crop_border)
    if use_image:
        a, b = to_uint8(a), to_uint8(b)
    a, b = a.astype(np.float64), b.astype(np.float64)
    return float(np.sum((a - b) ** 2)), float(a.max()), a.size


def psnr(img1, img2, crop_border=0):
    """calculate_psnr (psnr_ssim.py:53-70) on [C, H, W] arrays (float, or uint8 after ``to_uint8``)."""
    img1 = np.asarray(img1).transpose(1, 2, 0).astype(np.float64)
    img2 = np.asarray(img2).transpose(1, 2, 0).astype(np.float64)
    if crop_border != 0:
        img1 = img1[crop_border:-crop_border, crop_border:-crop_border, ...]
        img2 = img2[crop_border:-crop_border, crop_border:-crop_border, ...]
    mse = np.mean((img1 - img2) ** 2)
    if mse == 0:
        return float("inf")
    max_value = 1. if img1.max() <= 1 else 255.
    return float(20. * np.log10(max_value / np.sqrt(mse)))


def psnr_windowed(pred, gt, valid_hw=None, crop_border=0, use_image=False):
    """What validate() reports for one image: crop to the valid window, optionally quantise, then ``psnr``."""
    a, b = window(np.asarray(pred), valid_hw), window(np.asarray(gt), valid_hw)
    if use_image:
        a, b = to_uint8(a), to_uint8(b)
    return psnr(a, b, crop_border)


def cases(seed=20250819):
    """The seeded inputs of the golden file: name -> (img1 [C,H,W] float32, img2, crop_border, use_image)."""
    rng = np.random.RandomState(seed)
    out = {}
    for name, (c, h, w), cb in (("c1_1x1", (1, 1, 1), 0), ("c1_7x13", (1, 7, 13), 0), ("c3_7x13", (3, 7, 13), 0),
                                ("c3_40x56_cb4", (3, 40, 56), 4), ("c3_96x160", (3, 96, 160), 0)):
        a = rng.rand(c, h, w).astype(np.float32)
        b = np.clip(a + 0.05 * rng.randn(c, h, w), 0, 1).astype(np.float32)
        out[name] = (a, b, cb, False)
        out[name + "_u8"] = (a, b, cb, True)
    a = rng.rand(3, 8, 16).astype(np.float32)
    out["equal"] = (a, a.copy(), 0, False)
    b = (a * 0.5).astype(np.float32)
    a1 = a.copy()
    a1[0, 0, 0] = 1.0
    a1 = np.minimum(a1, np.float32(1.0))
    out["max_one"] = (a1, b, 0, False)
    a2 = a1.copy()
    a2[0, 0, 0] = np.nextafter(np.float32(1.0), np.float32(2.0))
    out["max_above_one"] = (a2, b, 0, False)
    # uint8 ties: k/255 +- 0.5/255 land on .5 after * 255 (where fp32 allows), plus out-of-range values
    k = np.arange(0, 256, dtype=np.float64)
    t = np.concatenate([(k + 0.5) / 255.0, (k - 0.5) / 255.0, [-0.25, -1e-9, 1.0 + 1e-6, 1.75]]).astype(np.float32)
    t = np.resize(t, (1, 12, 43)).astype(np.float32)
    out["ties_u8"] = (t, np.roll(t, 7, axis=2), 0, True)
    return out
