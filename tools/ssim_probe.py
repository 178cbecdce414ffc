#!/usr/bin/env python
"""Time of the SSIM kernel pair (csrc/ssim.hip) through ``metrics.ssim_batch``, against (a) a torch restatement
of the reference's route on the same card — per image: device -> host, host -> device, five fp32 11^3
``Conv3d`` calls with replicate padding, the map, its mean (psnr_ssim.py:160-197,276-318) — and (b)
``metrics.psnr_batch`` on the same tensors.

Shapes: [16, 3, 512, 512] and [16, 3, 1024, 1024], the headline workload's ``hq`` and ``sr``.  hipEvent timing,
the median of per-call times (5 warm-up + 30 timed for the two HIP legs; 1 + 3 for the reference route, which
takes seconds).  Bytes are the algorithmic ones for every leg: each operand read once (2 * numel * 4), so the
rates compare as time.  Writes one JSON line to profiles/ssim_probe.json.  Needs a GPU.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rethink_acoustic_image_enhancement_amd import metrics  # noqa: E402


def _median_ms(fn, warmup=5, steps=30):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return ms[len(ms) // 2], ms[0], ms[-1]


def _conv3d(dev):
    i = np.arange(11, dtype=np.float64) - 5.0
    g = np.exp(-(i * i) / 4.5)
    g /= g.sum()
    conv = torch.nn.Conv3d(1, 1, 11, padding=5, bias=False, padding_mode="replicate")
    with torch.no_grad():
        conv.weight[0, 0] = torch.from_numpy(np.einsum("i,j,k->ijk", g, g, g))
    return conv.to(dev).requires_grad_(False)


@torch.no_grad()
def reference_route(a, b, conv):
    """The reference's calculate_ssim per image of a [B, C, H, W] pair, its data movement included."""
    vals = []
    for i in range(a.shape[0]):
        x = a[i].detach().cpu().numpy().transpose(1, 2, 0).astype(np.float64)
        y = b[i].detach().cpu().numpy().transpose(1, 2, 0).astype(np.float64)
        L = 1.0 if x.max() <= 1 else 255.0
        c1, c2 = (0.01 * L) ** 2, (0.03 * L) ** 2
        x, y = torch.tensor(x).float().to(a.device), torch.tensor(y).float().to(a.device)
        f = lambda t: conv(t[None, None])[0, 0]  # noqa: E731
        mu1, mu2 = f(x), f(y)
        s1, s2, s12 = f(x * x) - mu1 * mu1, f(y * y) - mu2 * mu2, f(x * y) - mu1 * mu2
        m = ((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s1 + s2 + c2))
        vals.append(float(m.mean()))
    return vals


def probe(shape, dev, conv):
    g = torch.Generator(device=dev).manual_seed(0)
    a = torch.rand(shape, device=dev, generator=g)
    b = (a + 0.05 * torch.randn(shape, device=dev, generator=g)).clamp_(0, 1).contiguous()
    nbytes = 2 * a.numel() * 4
    out = {"shape": list(shape), "bytes": nbytes}
    legs = (("ssim_batch", lambda: metrics.ssim_batch(a, b), 5, 30),
            ("ssim_batch_uint8", lambda: metrics.ssim_batch(a, b, use_image=True), 5, 30),
            ("ssim_batch_valid", lambda: metrics.ssim_batch(a, b, variant="valid"), 5, 30),
            ("psnr_batch", lambda: metrics.psnr_batch(a, b), 5, 30),
            ("reference_route_torch", lambda: reference_route(a, b, conv), 1, 3))
    for name, fn, warmup, steps in legs:
        med, lo, hi = _median_ms(fn, warmup, steps)
        out[name] = {"ms": med, "ms_min": lo, "ms_max": hi, "gb_per_s": nbytes / med / 1e6, "steps": steps}
        print(name, out[name], flush=True)
    ours = metrics.ssim_batch(a, b).cpu().numpy()
    ref = np.array(reference_route(a, b, conv))
    out["max_abs_diff_vs_reference_route_fp32"] = float(np.abs(ours - ref).max())
    out["ssim_over_psnr_time"] = out["ssim_batch"]["ms"] / out["psnr_batch"]["ms"]
    out["reference_route_over_ssim_time"] = out["reference_route_torch"]["ms"] / out["ssim_batch"]["ms"]
    return out


def main():
    if not torch.cuda.is_available():
        raise SystemExit("ssim_probe: no GPU")
    dev = torch.device("cuda", 0)
    conv = _conv3d(dev)
    res = {"probe": "metric_ssim", "device": torch.cuda.get_device_name(0),
           "statistic": "median of per-call hipEvent times",
           "shapes": [probe((16, 3, 512, 512), dev, conv), probe((16, 3, 1024, 1024), dev, conv)]}
    line = json.dumps(res)
    print(line)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "ssim_probe.json")
    with open(path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
