#!/usr/bin/env python
"""Time of the dataset sample transforms (csrc/data.hip) through ``dataset.TeacherSampleTransform`` /
``dataset.StudentSampleTransform`` against the numpy oracle's host route on the same inputs, and the error of the
kernel's fp32 Philox / Box-Muller normals against the float64 model.

Workloads (the released training configs):
  kdlaet: 6 samples of u8 BGR lq / gt [600, 800, 3] and sr [1200, 1600, 3], gt_size 128 (KDLAET.yml);
  kdlaes: 4 bursts of 7 grey u8 frames [600, 800], gt_size 384, prob 0 (KDLAES.yml).
Legs, each the whole transform call (host draws, output allocation, every launch):
  philox      decoded frames resident on the device, normals from Philox in the kernel, no synchronisation inside;
  numpy       the same with the reference's host draws uploaded (the student route reads the counts back);
  host_route  tests/dataset_oracle.py on the host arrays (numpy: float32 conversion of the whole image, np.pad,
              slicing, float64 noise, flips), then the batch copied to the device.
hipEvent timing around each call (the events bracket host work too, so the host legs are wall times), median of
per-call times, 10 warm-up + 100 timed calls (host_route: 2 + 10).  The Philox error is the largest
|z_gpu - z_model| over one 64 x 64 x 3 draw, the kernel's z recovered exactly (tests/dataset_oracle.py::gpu_philox_z).
Writes one JSON line to profiles/dataset_probe.json.  Needs a GPU.
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
from rethink_acoustic_image_enhancement_amd import dataset  # noqa: E402
from tests import dataset_oracle as do  # noqa: E402


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


def main():
    if not torch.cuda.is_available():
        raise SystemExit("dataset_probe: no GPU")
    dev = torch.device("cuda", 0)
    rs = np.random.RandomState(0)
    random.seed(0)
    np.random.seed(0)
    res = {"probe": "dataset_sample", "device": torch.cuda.get_device_name(0),
           "statistic": "median of per-call hipEvent times", "workloads": []}

    h, w, C, seed, call = 64, 64, 3, 0x123456789ABCDEF, 5
    zg, zm = do.gpu_philox_z(h, w, C, seed, call), do.philox_normal(h, w, C, seed, call)
    err = np.abs(zg.astype(np.float64) - zm)
    res["philox_normal"] = {"draw": [h, w, C], "max_abs_z_err": float(err.max()), "mean_abs_z_err": float(err.mean()),
                            "max_abs_z": float(np.abs(zm).max()), "model": "float64 sqrt(-2 ln u1) cos(2 pi u2)"}
    print(json.dumps(res["philox_normal"]), flush=True)

    # ---- KDLAET.yml
    B, g = 6, 128
    lq = [rs.randint(0, 256, (600, 800, 3)).astype(np.uint8) for _ in range(B)]
    gt = [rs.randint(0, 256, (600, 800, 3)).astype(np.uint8) for _ in range(B)]
    sr = [rs.randint(0, 256, (1200, 1600, 3)).astype(np.uint8) for _ in range(B)]
    d = [[torch.from_numpy(a).to(dev) for a in v] for v in (lq, gt, sr)]
    rates = [0.5] * B
    legs = {}
    for rng in ("philox", "numpy"):
        t = dataset.TeacherSampleTransform(g, rng=rng, seed=1)
        legs[rng] = _median_ms(lambda: t(*d, rates), 10, 100)

    def host_teacher():
        outs = [do.teacher_sample(lq[b], gt[b], sr[b], rates[b], g) for b in range(B)]
        return [torch.from_numpy(np.stack([o[k] for o in outs])).to(dev) for k in range(4)]
    legs["host_route"] = _median_ms(host_teacher, 2, 10)
    out_bytes = 4 * B * (3 * g * g * 2 + g * g + 3 * 4 * g * g)
    res["workloads"].append({"workload": "kdlaet", "samples": B, "gt_size": g, "source": [600, 800, 3],
                             "launches_per_call": 3, "output_bytes": out_bytes, **legs,
                             "host_route_over_philox_time": legs["host_route"]["ms"] / legs["philox"]["ms"]})
    print(json.dumps(res["workloads"][-1]), flush=True)

    # ---- KDLAES.yml
    B, F, g, prob = 4, 7, 384, 0.0
    lqf = [[rs.randint(0, 256, (600, 800)).astype(np.uint8) for _ in range(F)] for _ in range(B)]
    gtf = [[rs.randint(0, 256, (600, 800)).astype(np.uint8) for _ in range(F)] for _ in range(B)]
    dl = [[torch.from_numpy(a).to(dev) for a in v] for v in lqf]
    dg = [[torch.from_numpy(a).to(dev) for a in v] for v in gtf]
    legs = {}
    for rng in ("philox", "numpy"):
        t = dataset.StudentSampleTransform(g, prob, rng=rng, seed=1)
        legs[rng] = _median_ms(lambda: t(dl, dg), 10 if rng == "philox" else 2, 100 if rng == "philox" else 10)

    def host_student():
        outs = [do.student_sample(lqf[b], gtf[b], g, prob) for b in range(B)]
        return [torch.from_numpy(np.stack([o[k] for o in outs])).to(dev) for k in range(2)]
    legs["host_route"] = _median_ms(host_student, 2, 10)
    res["workloads"].append({"workload": "kdlaes", "samples": B, "frames": F, "gt_size": g, "source": [600, 800],
                             "launches_per_call": 2 + B + 1, "output_bytes": 4 * 2 * B * F * g * g, **legs,
                             "host_route_over_philox_time": legs["host_route"]["ms"] / legs["philox"]["ms"]})
    print(json.dumps(res["workloads"][-1]), flush=True)

    line = json.dumps(res)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "dataset_probe.json")
    with open(path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
