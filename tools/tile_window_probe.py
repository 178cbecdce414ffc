#!/usr/bin/env python
"""What a weighted blend window costs a tiled KDLAE-T call: 1 x 3 x 2048^2 and 1 x 3 x 1024 x 4096 on the released
config (``[4,6,6,8]`` blocks, 4 refinement blocks, dim 48, hash weights), tile 512, overlap 32, tile_batch 16.

  (a) ``KDLAE_teacher.forward_tiled`` as a whole, ``window`` = uniform, ramp, hann;
  (b) the two blend launches of such a call alone (hq at scale 1, sr at scale 2), tables built beforehand;
  (c) the blend a user writes by hand, on the same card and the same staged tiles: per tile
      ``E[...].add_(patch * w)``, ``S[...].add_(w)``, then ``E.div_(S)``, for hq and sr.

hipEvent pairs around each; three warm-up passes of (a) per window (launch by launch, capture, replay), then
alternating timed repeats, so a drift of the card hits every window; median, min, max and spread = max - min.

Acceptance (DESIGN states it): the baseline is the uniform whole-call time of the parent commit, whose blend this
change does not touch.  ``--uniform-only OUT`` times nothing but (a) with the default window and runs on a tree
that has no ``window`` keyword; run it on the parent's tree first and hand its JSON over with ``--parent FILE``.
A weighted call may exceed that baseline's median by the baseline's own spread and no more.  Without ``--parent``
the uniform time of this run stands in and the JSON says so.  Writes one JSON line to
profiles/tile_window_probe.json.  Needs a GPU.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("KDLAE_PROBE_ROOT") or ROOT)   # the tree whose package is measured
from rethink_acoustic_image_enhancement_amd import _lib, tiling  # noqa: E402
from rethink_acoustic_image_enhancement_amd.hashweights import hash_images, load_hash_weights  # noqa: E402
from rethink_acoustic_image_enhancement_amd.KDLAE_model import KDLAE_teacher  # noqa: E402

TILE, OVERLAP, TILE_BATCH = 512, 32, 16
SHAPES = [(2048, 2048), (1024, 4096)]
WINDOWS = ("uniform", "ramp", "hann")
REPEATS = 5


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def _stats(ms):
    s = sorted(ms)
    return {"ms": s[len(s) // 2], "ms_min": s[0], "ms_max": s[-1], "spread_ms": s[-1] - s[0], "repeats": len(s)}


def _model(dev):
    m = KDLAE_teacher()
    load_hash_weights(m)
    return m.to(dev).eval()


def _inputs(H, W, dev):
    img = torch.from_numpy(hash_images(f"tile_probe:{H}x{W}", (1, 3, H, W))).to(dev)
    ramp = torch.linspace(0.1, 0.9, H * W, device=dev).view(1, 1, H, W).contiguous()
    return img, ramp


def whole_call(m, inp, windows):
    """(a): {window: stats}; ``None`` in ``windows`` is a call without the keyword."""
    calls = {w: ((lambda: m.forward_tiled(inp, TILE, OVERLAP, TILE_BATCH)) if w is None else
                 (lambda w=w: m.forward_tiled(inp, TILE, OVERLAP, TILE_BATCH, window=w))) for w in windows}
    for _ in range(3):   # eager, capture, replay
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    ms = {w: [] for w in windows}
    for _ in range(REPEATS):
        for w, fn in calls.items():
            ms[w].append(_timed(fn)[0])
    return {("uniform" if w is None else w): _stats(v) for w, v in ms.items()}


def blends_alone(st_hq, st_sr, H, W):
    """(b): {window: stats} of the two blend launches, tables built beforehand."""
    dev = st_hq.device
    calls = {}
    for w in WINDOWS:
        t1 = tiling.tile_window(w, H, W, TILE, OVERLAP, 1, dev)
        t2 = tiling.tile_window(w, H, W, TILE, OVERLAP, 2, dev)
        calls[w] = lambda t1=t1, t2=t2: (tiling.tile_blend(st_hq, 1, H, W, TILE, OVERLAP, 1, window=t1),
                                         tiling.tile_blend(st_sr, 1, H, W, TILE, OVERLAP, 2, window=t2))
    for fn in calls.values():
        fn()
    torch.cuda.synchronize()
    ms = {w: [] for w in WINDOWS}
    for _ in range(REPEATS):
        for w, fn in calls.items():
            ms[w].append(_timed(fn)[0])
    return {w: _stats(v) for w, v in ms.items()}


def host_blend(st_hq, st_sr, H, W, p):
    """(c) with the ramp tables -> (stats, hq, sr)."""
    dev = st_hq.device
    ys, xs = p.starts(H, W)

    def one(st, s):
        wy, wx = tiling.tile_window("ramp", H, W, TILE, OVERLAP, s, dev)
        w = (wy[:, None] * wx[None, :]).contiguous()
        E = torch.zeros((1, 3, s * H, s * W), device=dev)
        S = torch.zeros((1, 1, s * H, s * W), device=dev)
        k = 0
        for y in ys:
            for x in xs:
                sl = (slice(None), slice(None), slice(s * y, s * (y + p.th)), slice(s * x, s * (x + p.tw)))
                E[sl].add_(st[k] * w)
                S[sl].add_(w)
                k += 1
        return E.div_(S)

    def both():
        return one(st_hq, 1), one(st_sr, 2)
    both()
    torch.cuda.synchronize()
    ms, out = [], None
    for _ in range(REPEATS):
        t, out = _timed(both)
        ms.append(t)
    return _stats(ms), out[0], out[1]


@torch.no_grad()
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--uniform-only", metavar="OUT", help="time (a) with the default window only and write OUT")
    ap.add_argument("--parent", metavar="FILE", help="the --uniform-only JSON of the parent commit's tree")
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "tile_window_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tile_window_probe: no GPU")
    dev = torch.device("cuda", 0)
    m = _model(dev)
    sha = hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()
    if args.uniform_only:
        cases = []
        for H, W in SHAPES:
            img, rate = _inputs(H, W, dev)
            cases.append({"shape": [1, 3, H, W],
                          "forward_tiled": whole_call(m, {"img": img, "denoise_rate": rate}, [None])["uniform"]})
            print(cases[-1], flush=True)
        with open(args.uniform_only, "w") as f:
            f.write(json.dumps({"probe": "tile_window:uniform_only", "library_sha256": sha, "cases": cases}) + "\n")
        return
    parent = json.load(open(args.parent)) if args.parent else None
    cases = []
    for ci, (H, W) in enumerate(SHAPES):
        img, rate = _inputs(H, W, dev)
        p = tiling.tile_plan(H, W, TILE, OVERLAP)
        n = p.ni * p.nj
        whole = whole_call(m, {"img": img, "denoise_rate": rate}, WINDOWS)
        st_hq = torch.rand((n, 3, p.th, p.tw), device=dev) * 2 - 1
        st_sr = torch.rand((n, 3, 2 * p.th, 2 * p.tw), device=dev) * 2 - 1
        blend = blends_alone(st_hq, st_sr, H, W)
        host, h_hq, h_sr = host_blend(st_hq, st_sr, H, W, p)
        k_hq = tiling.tile_blend(st_hq, 1, H, W, TILE, OVERLAP, 1, window="ramp")
        k_sr = tiling.tile_blend(st_sr, 1, H, W, TILE, OVERLAP, 2, window="ramp")
        # the host loop has no copy rule: compare where it matters, as a largest difference
        diff = max(float((k_hq - h_hq).abs().max()), float((k_sr - h_sr).abs().max()))
        del h_hq, h_sr, k_hq, k_sr, st_hq, st_sr
        base = parent["cases"][ci]["forward_tiled"] if parent else whole["uniform"]
        assert parent is None or parent["cases"][ci]["shape"] == [1, 3, H, W]
        case = {"shape": [1, 3, H, W], "tile": TILE, "tile_overlap": OVERLAP, "tile_batch": TILE_BATCH,
                "plan": p._asdict(), "tiles": n,
                "forward_tiled": whole, "blend_launches": blend, "host_loop_blend_ramp": host,
                "host_loop_blend_over_kernel_blend_ramp": host["ms"] / blend["ramp"]["ms"],
                "kernel_vs_host_loop_largest_difference_ramp": diff,
                "baseline": {"source": "parent commit, uniform, a process of its own before this run" if parent else
                             "this run's uniform (the parent commit was not measured)", **base},
                "within_baseline_plus_its_spread": {w: bool(whole[w]["ms"] <= base["ms"] + base["spread_ms"])
                                                    for w in ("ramp", "hann")},
                "blend_share_of_forward_tiled": {w: blend[w]["ms"] / whole[w]["ms"] for w in WINDOWS}}
        print(case, flush=True)
        cases.append(case)
        del img, rate
    res = {"probe": "tile_window", "device": torch.cuda.get_device_name(0),
           "config": "KDLAE_teacher() defaults: num_blocks [4,6,6,8], 4 refinement blocks, dim 48, hash weights",
           "statistic": "hipEvent time; 3 warm-up passes of the whole call per window, then %d alternating timed "
                        "repeats: median, min, max, spread = max - min" % REPEATS,
           "host_loop_blend": "per tile E[...].add_(patch * w), S[...].add_(w), then E.div_(S), hq and sr, ramp",
           "library_sha256": sha, "parent_library_sha256": parent["library_sha256"] if parent else None,
           "cases": cases}
    with open(args.out, "w") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
