#!/usr/bin/env python
"""Achieved HBM rate of the four BatchNorm training kernels (bn_train.hip), one launch at a time through
the ``kdlae_debug_bn`` self-test entry: hipEvent timing, 3 warm-up + 10 timed launches per kernel.

Shapes: the level-0 layers of a B = 32, 256^2 micro-batch (P = 2097152 pixels): C = 64 contiguous, C = 64
as a slice of the 128-wide concat buffer, and a 16-channel extractor slice of the 48-wide merged buffer.
Bytes are the algorithmic ones (every operand once): stats P C 4, apply 2 P C 4, reduce 3 P C 4, dx 4 P C 4.
Writes one JSON line to profiles/asdqe_bn_probe.json.  Needs a GPU.
"""
from __future__ import annotations

import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rethink_acoustic_image_enhancement_amd import _lib  # noqa: E402

c_int, c_int64, c_float, c_void_p = ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p


class BnDesc(ctypes.Structure):  # kdlae_debug_bn_desc (include/kdlae.h)
    _fields_ = [("op", c_int), ("x", c_void_p), ("ldx", c_int), ("y", c_void_p), ("ldy", c_int),
                ("dy", c_void_p), ("ldd", c_int), ("out", c_void_p), ("ldo", c_int),
                ("mean", c_void_p), ("rstd", c_void_p), ("running_mean", c_void_p), ("running_var", c_void_p),
                ("momentum", c_float), ("gamma", c_void_p), ("beta", c_void_p), ("dgamma", c_void_p),
                ("dbeta", c_void_p), ("C", c_int), ("P", c_int64), ("N", c_int), ("h", c_int), ("w", c_int),
                ("part", c_void_p), ("part_floats", c_int64)]


def _time(d, warmup=3, steps=10):
    L = _lib.lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for _ in range(warmup):
        _lib.check(L.kdlae_debug_bn(ctypes.byref(d), stream), "kdlae_debug_bn")
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _lib.check(L.kdlae_debug_bn(ctypes.byref(d), stream), "kdlae_debug_bn")
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return ms[len(ms) // 2]


def probe(P, C, ld, dev):
    z = torch.randn(P, ld, device=dev)
    y = torch.empty(P, ld, device=dev)
    dy = torch.randn(P, ld, device=dev)
    dz = torch.empty(P, ld, device=dev)
    vec = lambda v: torch.full((C,), v, device=dev)  # noqa: E731
    mean, rstd, gamma, beta, dgam, dbet = vec(0.0), vec(1.0), vec(1.0), vec(0.0), vec(0.0), vec(0.0)
    part = torch.empty(2048 * C, device=dev)
    out = {"P": P, "C": C, "ld": ld}
    for name, op, passes in (("bn_stats", 0, 1), ("bn_apply_relu", 1, 2), ("bn_bwd_reduce", 2, 3), ("bn_bwd_dx", 3, 4)):
        d = BnDesc()
        d.op, d.C, d.P = op, C, P
        d.x, d.ldx, d.y, d.ldy, d.dy, d.ldd = z.data_ptr(), ld, y.data_ptr(), ld, dy.data_ptr(), ld
        d.out, d.ldo = (y if op == 1 else dz).data_ptr(), ld
        d.mean, d.rstd, d.gamma, d.beta = mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), beta.data_ptr()
        d.dgamma, d.dbeta, d.part, d.part_floats = dgam.data_ptr(), dbet.data_ptr(), part.data_ptr(), part.numel()
        ms = _time(d)
        out[name] = {"ms": ms, "gb_per_s": passes * P * C * 4 / ms / 1e6}
    return out


def main():
    if not torch.cuda.is_available():
        raise SystemExit("asdqe_bn_probe: no GPU")
    dev = torch.device("cuda", 0)
    P = 32 * 256 * 256
    res = {"probe": "asdqe_bn_kernels", "device": torch.cuda.get_device_name(0),
           "shapes": [probe(P, 64, 64, dev), probe(P, 64, 128, dev), probe(P, 16, 48, dev)]}
    line = json.dumps(res)
    print(line)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "asdqe_bn_probe.json")
    with open(path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
