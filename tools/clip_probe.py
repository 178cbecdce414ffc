#!/usr/bin/env python
"""KDLAE-S on whole clips: u8 gray clips of 64 frames, 1 x 64 x 512^2 and 1 x 64 x 256 x 1024, on the S8 config
(hidden [16,32,64], residual, hash weights), windows of 7 frames, overlap 2, window_batch 8.

  (a) ``pipeline.enhance_clip_u8``: windows gathered, blended and turned into bytes by the library's kernels;
  (b) the loop a user writes without it, on the same card: ``frames_preprocess_u8`` once, torch slicing, the
      module's ``forward`` at batch 1 per window, ``E[:, s:s+f].add_``, ``W[s:s+f].add_(1)``, ``E.div_(W)``,
      ``postprocess_u8`` and the permute back into frame order.

hipEvent timing around the whole call, three warm-up passes per route, then alternating timed repeats of (a) and
(b); the median per route, and for (b) the run-to-run spread (max - min) that the acceptance uses: (a) may not be
slower than (b) by more than that spread, and (a)'s bytes must be ``torch.equal`` to (b)'s.  Also recorded: the
summed device time of the gather and blend launches of one (a) call (each launch bracketed by events in a pass of
its own) as a share of (a), and the staging bytes.  Writes one JSON line to profiles/clip_probe.json (or to the
path given).  Needs a GPU.
"""
from __future__ import annotations

import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rethink_acoustic_image_enhancement_amd import _lib, clips  # noqa: E402
from rethink_acoustic_image_enhancement_amd.hashweights import load_hash_weights  # noqa: E402
from rethink_acoustic_image_enhancement_amd.KDLAE_model import KDLAE_student  # noqa: E402
from rethink_acoustic_image_enhancement_amd.pipeline import (enhance_clip_u8, frames_preprocess_u8,  # noqa: E402
                                                             postprocess_u8)

FRAMES, OVERLAP, WINDOW_BATCH = 7, 2, 8
SHAPES = [(64, 512, 512), (64, 256, 1024)]
REPEATS = 7


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


def host_loop(m, clip):
    B, T, h, w = clip.shape
    p = clips.clip_plan(T, FRAMES, OVERLAP)
    x = frames_preprocess_u8(clip, 32)
    E = torch.zeros_like(x)
    Wt = torch.zeros((T, 1, 1), device=x.device)
    for b in range(B):
        for s in p.starts(T):
            y = m(x[b:b + 1, s:s + p.f])
            E[b:b + 1, s:s + p.f].add_(y)
            if b == 0:
                Wt[s:s + p.f].add_(1)
    return postprocess_u8(E.div_(Wt), h, w, 1, None).permute(0, 3, 1, 2).contiguous()


def mover_ms(x, h, w, p):
    """Device time of the gather and blend launches of one enhance_clip_u8 call, each bracketed on its own."""
    B, T, H, W = x.shape
    n = B * p.n
    staged = torch.rand((n, p.f, H, W), device=x.device)
    calls = []
    for first in range(0, n, WINDOW_BATCH):
        count = min(WINDOW_BATCH, n - first)
        calls.append(("gather", lambda f=first, c=count: clips.clip_gather(x, FRAMES, OVERLAP, f, c)))
    calls.append(("blend", lambda: clips.clip_blend_u8(staged, B, T, h, w, FRAMES, OVERLAP)))
    for _, fn in calls:
        fn()
    torch.cuda.synchronize()
    tot = {"gather": [], "blend": []}
    for _ in range(REPEATS):
        acc = {"gather": 0.0, "blend": 0.0}
        for kind, fn in calls:
            acc[kind] += _timed(fn)[0]
        for k in acc:
            tot[k].append(acc[k])
    return {k: sorted(v)[len(v) // 2] for k, v in tot.items()}, len(calls)


@torch.no_grad()
def main():
    if not torch.cuda.is_available():
        raise SystemExit("clip_probe: no GPU")
    dev = torch.device("cuda", 0)
    m = KDLAE_student(residual=True, hidden_channels=[16, 32, 64])
    load_hash_weights(m)
    m = m.to(dev).eval()
    cases = []
    for T, h, w in SHAPES:
        clip = torch.randint(0, 256, (1, T, h, w), dtype=torch.uint8,
                             generator=torch.Generator().manual_seed(T + h)).to(dev)
        p = clips.clip_plan(T, FRAMES, OVERLAP)

        def call():
            return enhance_clip_u8(m, clip, FRAMES, OVERLAP, WINDOW_BATCH)

        def loop():
            return host_loop(m, clip)
        for _ in range(3):
            out_a = call()
            out_b = loop()
        torch.cuda.synchronize()
        same = bool(torch.equal(out_a, out_b))
        del out_a, out_b
        ms_a, ms_b = [], []
        for _ in range(REPEATS):   # alternating, so a drift of the card hits both routes
            ms_a.append(_timed(call)[0])
            ms_b.append(_timed(loop)[0])
        a, b = _stats(ms_a), _stats(ms_b)
        x = frames_preprocess_u8(clip, 32)
        movers, launches = mover_ms(x, h, w, p)
        case = {"shape": [1, T, h, w], "frames": FRAMES, "overlap": OVERLAP, "window_batch": WINDOW_BATCH,
                "plan": p._asdict(), "windows": p.n,
                "enhance_clip_u8": a, "host_loop": b,
                "host_loop_over_enhance_clip_u8": b["ms"] / a["ms"],
                "outputs_equal": same,
                "not_slower_than_host_loop_by_more_than_its_spread": bool(a["ms"] <= b["ms"] + b["spread_ms"]),
                "gather_ms": movers["gather"], "blend_ms": movers["blend"], "mover_launches": launches,
                "mover_share_of_enhance_clip_u8": (movers["gather"] + movers["blend"]) / a["ms"],
                "staging_bytes": p.n * p.f * x.shape[2] * x.shape[3] * 4}
        print(case, flush=True)
        cases.append(case)
        del clip, x
    res = {"probe": "clip", "device": torch.cuda.get_device_name(0),
           "config": "KDLAE_student(residual=True, hidden_channels=[16,32,64]), hash weights",
           "statistic": "hipEvent time of the whole call; 3 warm-up passes per route, then %d alternating timed "
                        "repeats: median, min, max, spread = max - min" % REPEATS,
           "host_loop": "frames_preprocess_u8 once, torch slicing, forward at batch 1 per window, add_ / add_(1) / "
                        "div_, postprocess_u8, permute",
           "library_sha256": hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest(), "cases": cases}
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "clip_probe.json")
    with open(path, "w") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps(res))
    if not all(c["outputs_equal"] for c in cases):
        raise SystemExit("clip_probe: enhance_clip_u8 and the host loop differ")


if __name__ == "__main__":
    main()
