#!/usr/bin/env python
"""KDLAE-S on a live stream: gray u8 frames of 512^2 arriving one at a time, batch 1 and batch 4, windows of 7
frames, emit 3, on the S8 config (hidden [16,32,64], residual, hash weights).  Three routes per arriving frame:

  (a) ``StudentStream.push`` with the HIP graph replayed (``hip_graphs = True``);
  (b) ``StudentStream.push`` launch by launch (``hip_graphs = False``);
  (c) the loop a user writes without it, on the same card: ``torch.cat`` of the last six frames and the new one,
      ``pipeline.enhance_frames_u8`` on the stack of 7, the centre frame sliced out.

Per-push wall latency: ``time.perf_counter`` around the call and a device synchronise, the three routes taking
the same frame in turn (the order rotates every frame, so a drift of the card or the host hits all three),
WARMUP frames first, then PUSHES timed ones per route.  Per route: the median and the spread, which is defined
here, before any number is read, as p90 - p10 of the timed pushes (max - min over hundreds of host-timed samples is
one scheduler hiccup); min and max are recorded too.  The acceptance: (a)'s median may not exceed (c)'s by more
than (c)'s spread; ``hip_graphs`` defaults to on only if (b)'s median exceeds (a)'s by more than (b)'s spread.
Also recorded: frames per second without the per-push synchronise (RUN pushes, one synchronise at the end, three
alternating rounds per route, the median), and whether the three routes returned equal bytes for every frame.
Writes one JSON line to profiles/stream_probe.json (or to the path given).  Needs a GPU.
"""
from __future__ import annotations

import hashlib
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rethink_acoustic_image_enhancement_amd import _lib  # noqa: E402
from rethink_acoustic_image_enhancement_amd.hashweights import load_hash_weights  # noqa: E402
from rethink_acoustic_image_enhancement_amd.KDLAE_model import KDLAE_student  # noqa: E402
from rethink_acoustic_image_enhancement_amd.pipeline import enhance_frames_u8  # noqa: E402

FRAMES, EMIT = 7, 3
SHAPES = [(1, 512, 512), (4, 512, 512)]
WARMUP, PUSHES, RUN, ROUNDS = 30, 300, 200, 3
POOL = 16   # distinct input frames, cycled


class HostRoute:
    """The "before" loop: a fresh stack per frame, every frame preprocessed again, the centre frame returned."""

    def __init__(self, model):
        self.model, self.buf = model, None

    def push(self, frame):
        if self.buf is None:
            self.buf = frame[:, None].repeat(1, FRAMES, 1, 1)
        self.buf = torch.cat([self.buf[:, 1:], frame[:, None]], 1)
        return enhance_frames_u8(self.model, self.buf)[..., EMIT]


def _stats(ms):
    s = sorted(ms)
    q = lambda p: s[min(len(s) - 1, int(p * len(s)))]   # noqa: E731
    return {"ms": q(0.5), "p10_ms": q(0.1), "p90_ms": q(0.9), "spread_ms": q(0.9) - q(0.1), "ms_min": s[0],
            "ms_max": s[-1], "pushes": len(s)}


@torch.no_grad()
def main():
    if not torch.cuda.is_available():
        raise SystemExit("stream_probe: no GPU")
    dev = torch.device("cuda", 0)
    m = KDLAE_student(residual=True, hidden_channels=[16, 32, 64])
    load_hash_weights(m)
    m = m.to(dev).eval()
    cases = []
    for B, h, w in SHAPES:
        pool = torch.randint(0, 256, (POOL, B, h, w), dtype=torch.uint8,
                             generator=torch.Generator().manual_seed(B + h)).to(dev)
        a, b, c = m.stream(B, h, w, FRAMES, EMIT), m.stream(B, h, w, FRAMES, EMIT), HostRoute(m)
        a.hip_graphs, b.hip_graphs = True, False
        routes = {"graph_replay": a, "stream_eager": b, "host_route": c}
        names = list(routes)
        # the three routes lag differently (the streams return frame t - 3 at push t, the host route too once its
        # stack is full), so from push FRAMES - 1 on all three return the same frame: compare them
        equal, compared = True, 0
        lat = {n: [] for n in names}
        for i in range(WARMUP + PUSHES):
            frame = pool[i % POOL]
            outs = {}
            for k in range(3):
                n = names[(i + k) % 3]
                t0 = time.perf_counter()
                outs[n] = routes[n].push(frame)
                torch.cuda.synchronize(dev)
                if i >= WARMUP:
                    lat[n].append((time.perf_counter() - t0) * 1e3)
            if i >= FRAMES:
                ya, yb, yc = outs["graph_replay"][:, 0], outs["stream_eager"][:, 0], outs["host_route"]
                equal = equal and bool(torch.equal(ya, yb)) and bool(torch.equal(ya, yc))
                compared += 1
        replays = a.graph_replays
        fps = {n: [] for n in names}
        for r in range(ROUNDS):
            for k in range(3):
                n = names[(r + k) % 3]
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                for i in range(RUN):
                    routes[n].push(pool[i % POOL])
                torch.cuda.synchronize(dev)
                fps[n].append(RUN / (time.perf_counter() - t0))
        st = {n: _stats(v) for n, v in lat.items()}
        ga, eb, hc = st["graph_replay"], st["stream_eager"], st["host_route"]
        case = {"shape": [B, h, w], "frames": FRAMES, "emit": EMIT, "latency": st,
                "frames_per_s_unsynchronised": {n: sorted(v)[len(v) // 2] for n, v in fps.items()},
                "graph_replays": replays, "graph_captures": a.graph_captures,
                "outputs_equal": equal, "frames_compared": compared,
                "host_route_over_graph_replay": hc["ms"] / ga["ms"],
                "stream_eager_over_graph_replay": eb["ms"] / ga["ms"],
                "graph_not_slower_than_host_route_by_more_than_its_spread":
                    bool(ga["ms"] <= hc["ms"] + hc["spread_ms"]),
                "graph_beats_eager_by_more_than_its_spread": bool(eb["ms"] - ga["ms"] > eb["spread_ms"])}
        print(case, flush=True)
        cases.append(case)
        del a, b, c, routes, pool
    res = {"probe": "stream", "device": torch.cuda.get_device_name(0),
           "config": "KDLAE_student(residual=True, hidden_channels=[16,32,64]), hash weights",
           "statistic": "host wall time of one push ending in a device synchronise; %d warm-up frames, then %d timed "
                        "pushes per route, the routes taking each frame in rotating order; median, p10, p90, "
                        "spread = p90 - p10, min, max.  frames_per_s_unsynchronised: %d pushes and one synchronise, "
                        "median of %d alternating rounds" % (WARMUP, PUSHES, RUN, ROUNDS),
           "host_route": "torch.cat of the last 6 frames and the new one, enhance_frames_u8 on the 7, [..., 3]",
           "library_sha256": hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest(), "cases": cases}
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "stream_probe.json")
    with open(path, "w") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps(res))
    if not all(c["outputs_equal"] for c in cases):
        raise SystemExit("stream_probe: the routes differ")


if __name__ == "__main__":
    main()
