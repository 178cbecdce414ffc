#!/usr/bin/env python
"""Time of NIQE on the HIP path (csrc/niqe.hip through ``metrics.niqe_batch``) against the host route the
reference takes, modelled by tests/niqe_oracle.py's ``like_reference`` mode (numpy on the CPU; kinder than the
reference itself, which also rebuilds its 9801-entry gamma table for every block and map).

Shapes: [16, 3, 512, 512] and [16, 3, 1024, 1024], the headline workload's ``hq`` and ``sr``.  Per shape:
* ``niqe_reduce``: the four launches alone, hipEvent timing, median of per-call times (5 warm-up + 30 timed);
* ``finish_niqe``: the host finish alone on moments already on the host, wall clock, median of 5 + 30;
* ``niqe_batch``: the whole call, device-to-host copy and host finish included, wall clock around a
  synchronised call, median of 5 + 30;
* ``host_route_per_image``: one image through the oracle (device -> host copy included), wall clock, median of
  3 after 1 warm-up; ``host_route_batch_estimate`` is that times the batch.
Bytes are the algorithmic ones: the input read once (numel * 4); the kernel's own traffic on top is one read of
the Y image per scale.  Writes one JSON line to profiles/niqe_probe.json (or argv[1]).  Needs a GPU.
"""
from __future__ import annotations

import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rethink_acoustic_image_enhancement_amd import metrics  # noqa: E402
from tests import niqe_oracle as no  # noqa: E402


def _median(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


def _event_ms(fn, warmup=5, steps=30):
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
    return _median(ms)


def _wall_ms(fn, warmup=5, steps=30):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) * 1e3)
    return _median(ms)


def probe(shape, dev, p):
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.rand(shape, device=dev, generator=g)
    nbytes = x.numel() * 4
    out = {"shape": list(shape), "bytes": nbytes, "blocks_per_image": (shape[2] // 96) * (shape[3] // 96)}
    mom = metrics.niqe_reduce(x, params=p).cpu()
    legs = (("niqe_reduce", _event_ms, lambda: metrics.niqe_reduce(x, params=p), 5, 30),
            ("finish_niqe", _wall_ms, lambda: metrics.finish_niqe(mom, p), 5, 30),
            ("niqe_batch", _wall_ms, lambda: metrics.niqe_batch(x, params=p), 5, 30),
            ("host_route_per_image", _wall_ms,
             lambda: no.niqe(x[0].cpu().numpy(), 0, True, p, mode="like_reference"), 1, 3))
    for name, timer, fn, warmup, steps in legs:
        med, lo, hi = timer(fn, warmup, steps)
        out[name] = {"ms": med, "ms_min": lo, "ms_max": hi, "steps": steps}
        if name == "niqe_reduce":
            out[name]["gb_per_s"] = nbytes / med / 1e6
        print(name, out[name], flush=True)
    out["host_route_batch_estimate_ms"] = out["host_route_per_image"]["ms"] * shape[0]
    out["host_route_over_niqe_batch_time"] = out["host_route_batch_estimate_ms"] / out["niqe_batch"]["ms"]
    ours = float(metrics.niqe_batch(x[:1], params=p)[0])
    ref = no.niqe(x[0].cpu().numpy(), 0, True, p, mode="like_reference")
    out["first_image"] = {"niqe_batch": ours, "host_route": ref, "abs_diff": abs(ours - ref)}
    return out


def main():
    if not torch.cuda.is_available():
        raise SystemExit("niqe_probe: no GPU")
    dev = torch.device("cuda", 0)
    p = metrics.load_niqe_params(os.path.join(no.GOLDEN, "niqe_pris_params.npz"))
    res = {"probe": "metric_niqe", "device": torch.cuda.get_device_name(0),
           "statistic": "median of per-call times (hipEvent for niqe_reduce, wall clock for the legs with host work)",
           "shapes": [probe((16, 3, 512, 512), dev, p), probe((16, 3, 1024, 1024), dev, p)]}
    line = json.dumps(res)
    print(line)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "niqe_probe.json")
    with open(path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
