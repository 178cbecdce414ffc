#!/usr/bin/env python
"""Achieved HBM rate of the PSNR kernel pair (csrc/metrics.hip) through ``metrics.psnr_batch`` (and through the
bare ``kdlae_metric_psnr`` call on preallocated buffers), against the plain torch expression ``((a.double() - b.double()) ** 2).flatten(1).sum(1)`` on the same tensors.

Shapes: [16, 3, 512, 512] and [16, 3, 1024, 1024], the headline workload's ``hq`` and ``sr``.  hipEvent timing,
5 warm-up + 30 timed launches each, the median reported.  Bytes are the algorithmic ones: each operand read
once (2 * numel * 4; the torch expression moves several times that through its fp64 temporaries, but is
charged the same bytes so the two rates compare as time).  A third line times the kernel on a 509 x 1021
window of the large shape: row starts off the 16-byte grid, so the head / float4 / tail path.
Writes one JSON line to profiles/metric_probe.json.  Needs a GPU.
"""
from __future__ import annotations

import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rethink_acoustic_image_enhancement_amd import _lib, metrics  # noqa: E402


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


def probe(shape, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    a = torch.rand(shape, device=dev, generator=g)
    b = (a + 0.05 * torch.randn(shape, device=dev, generator=g)).contiguous()
    nbytes = 2 * a.numel() * 4
    out = {"shape": list(shape), "bytes": nbytes}
    # the bare C call on preallocated buffers: the two launches without the Python wrapper's allocations
    L = _lib.lib()
    red = torch.empty((shape[0], 2), dtype=torch.float64, device=dev)
    scratch = torch.empty(int(L.kdlae_metric_scratch_bytes()), dtype=torch.uint8, device=dev)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    B, C, H, W = shape

    def c_call():
        _lib.check(L.kdlae_metric_psnr(vp(a), vp(b), B, C, H, W, H, W, H, W, 0, 0, vp(red), vp(scratch), stream),
                   "kdlae_metric_psnr")

    legs = (("psnr_batch", lambda: metrics.psnr_batch(a, b)),
            ("hip_psnr_c_call", c_call),
            ("psnr_batch_uint8", lambda: metrics.psnr_batch(a, b, use_image=True)),
            ("torch_expr", lambda: ((a.double() - b.double()) ** 2).flatten(1).sum(1)))
    for name, fn in legs:
        med, lo, hi = _median_ms(fn)
        out[name] = {"ms": med, "ms_min": lo, "ms_max": hi, "gb_per_s": nbytes / med / 1e6}
    h, w = shape[2] - 3, shape[3] - 3
    med, lo, hi = _median_ms(lambda: metrics.psnr_reduce(a, b, (h, w), 1))
    wbytes = 2 * shape[0] * shape[1] * (h - 2) * (w - 2) * 4
    out["hip_psnr_unaligned_window"] = {"window": [h, w], "crop_border": 1, "bytes": wbytes, "ms": med, "ms_min": lo,
                                        "ms_max": hi, "gb_per_s": wbytes / med / 1e6}
    sse = metrics.psnr_reduce(a, b)[0][:, 0]
    ref = ((a.double() - b.double()) ** 2).flatten(1).sum(1)
    out["max_rel_diff_vs_torch"] = float(((sse - ref).abs() / ref).max())
    return out


def main():
    if not torch.cuda.is_available():
        raise SystemExit("metric_probe: no GPU")
    dev = torch.device("cuda", 0)
    res = {"probe": "metric_psnr", "device": torch.cuda.get_device_name(0), "warmup": 5, "steps": 30,
           "statistic": "median of per-launch hipEvent times",
           "shapes": [probe((16, 3, 512, 512), dev), probe((16, 3, 1024, 1024), dev)]}
    line = json.dumps(res)
    print(line)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "metric_probe.json")
    with open(path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
