#!/usr/bin/env python
"""Time of the progressive-learning batch preparation (csrc/augment.hip) through ``augment.ProgressiveBatcher``
against the reference's host route on the same machine.

Workloads (one stage of each released schedule, cropped 128^2 -> 64^2):
  kdlaet: lq = {img [6, 3, 128, 128], denoise_rate [6, 1, 128, 128]}, gt = {hq [6, 3, 128, 128], sr [6, 3, 256, 256]}
  kdlaes: lq, gt = [32, 7, 128, 128]
Legs, each the whole ``batcher(it, lq, gt)`` call (host draws, output allocation, the one launch):
  philox      device-resident batch, mask from Philox in the kernel;
  numpy       device-resident batch, mask drawn on the host per plane as the reference draws it, uploaded as bytes;
  launch      ``kdlae_train_prepare`` alone on preallocated outputs (Philox);
  host_route  the reference's way: the batch on the host, crop, per (image, channel) plane a numpy mask and the
              float64 ``x * m - 0.1 + 0.1 * m`` written back to fp32, then the prepared batch copied to the device;
  upload      copying the unprepared host batch to the device, which the device legs need first and the host
              route does not (it uploads the smaller prepared batch instead).
hipEvent timing around each call (the events bracket host work too, so the host legs are wall times), median of
per-call times, 10 warm-up + 100 timed calls (host_route: 2 + 20).  Bytes are the algorithmic ones: every output
element read once and written once.  Writes one JSON line to profiles/prepare_probe.json.  Needs a GPU.
"""
from __future__ import annotations

import json
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rethink_acoustic_image_enhancement_amd import augment  # noqa: E402


def _median_ms(fn, warmup, steps):
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
    return {"ms": ms[len(ms) // 2], "ms_min": ms[0], "ms_max": ms[-1], "steps": steps, "warmup": warmup}


def _tensors(v):
    return list(v.values()) if isinstance(v, dict) else [v]


def host_route(lq, gt, mgs, p, dev):
    """Crop, mask per plane in float64 as input_mask does, copy the prepared batch to the device."""
    x0, y0 = int((128 - mgs) * random.random()), int((128 - mgs) * random.random())

    def crop(t, s=1):
        return t[:, :, x0 * s:(x0 + mgs) * s, y0 * s:(y0 + mgs) * s]

    def mask(t):
        t = crop(t).clone()
        for i in range(t.size(0)):
            for j in range(t.shape[1]):
                m = np.random.choice([0, 1], size=(mgs, mgs), p=[p, 1 - p])
                t[i, j] = torch.from_numpy(np.multiply(t[i, j].numpy(), m) - 0.1 + 0.1 * m)
        return t

    if isinstance(lq, dict):
        out = [mask(lq["img"]), crop(lq["denoise_rate"]), crop(gt["hq"]), crop(gt["sr"], 2)]
    else:
        out = [mask(lq), crop(gt)]
    return [t.contiguous().to(dev) for t in out]


def probe(name, lq, gt, mgs, p, dev):
    bs = _tensors(lq)[0].shape[0]
    sch = augment.ProgressiveSchedule([10 ** 9], [mgs], [bs], [p], 128, bs)
    dlq = {k: v.to(dev) for k, v in lq.items()} if isinstance(lq, dict) else lq.to(dev)
    dgt = {k: v.to(dev) for k, v in gt.items()} if isinstance(gt, dict) else gt.to(dev)
    ph, nu = augment.ProgressiveBatcher(sch, rng="philox", seed=1), augment.ProgressiveBatcher(sch, rng="numpy")
    o_lq, o_gt = ph(1, dlq, dgt)
    nbytes = 2 * 4 * sum(t.numel() for t in _tensors(o_lq) + _tensors(o_gt))
    segs = [dict(src=s, dst=d, y0=3, x0=5, prob=p if i == 0 else 0.0) for i, (s, d) in
            enumerate(zip(_tensors(dlq) + _tensors(dgt), _tensors(o_lq) + _tensors(o_gt)))]
    for g, s in zip(segs, (1, 1, 1, 2) if isinstance(lq, dict) else (1, 1)):
        g["y0"], g["x0"] = g["y0"] * s, g["x0"] * s
    it = [0]

    def call(b):
        it[0] += 1
        return b(it[0], dlq, dgt)

    out = {"workload": name, "bytes": nbytes, "crop": [128, mgs], "prob": p,
           "philox": _median_ms(lambda: call(ph), 10, 100),
           "numpy": _median_ms(lambda: call(nu), 10, 100),
           "launch": _median_ms(lambda: augment.train_prepare(segs, None, bs, 0.1, 1, 8), 10, 100),
           "host_route": _median_ms(lambda: host_route(lq, gt, mgs, p, dev), 2, 20),
           "upload": _median_ms(lambda: [t.to(dev) for t in _tensors(lq) + _tensors(gt)], 10, 100)}
    for leg in ("philox", "numpy", "launch", "host_route"):
        out[leg]["gb_per_s"] = nbytes / out[leg]["ms"] / 1e6
    out["host_route_over_philox_time"] = out["host_route"]["ms"] / out["philox"]["ms"]
    print(json.dumps(out), flush=True)
    return out


def main():
    if not torch.cuda.is_available():
        raise SystemExit("prepare_probe: no GPU")
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    random.seed(0)
    np.random.seed(0)
    t_lq = {"img": torch.rand(6, 3, 128, 128, generator=g), "denoise_rate": torch.rand(6, 1, 128, 128, generator=g)}
    t_gt = {"hq": torch.rand(6, 3, 128, 128, generator=g), "sr": torch.rand(6, 3, 256, 256, generator=g)}
    s_lq, s_gt = torch.rand(32, 7, 128, 128, generator=g), torch.rand(32, 7, 128, 128, generator=g)
    res = {"probe": "train_prepare", "device": torch.cuda.get_device_name(0),
           "statistic": "median of per-call hipEvent times",
           "workloads": [probe("kdlaet", t_lq, t_gt, 64, 0.1, dev), probe("kdlaes", s_lq, s_gt, 64, 0.1, dev)]}
    line = json.dumps(res)
    print(line)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "prepare_probe.json")
    with open(path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
