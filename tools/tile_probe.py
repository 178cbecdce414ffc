#!/usr/bin/env python
"""Tiled KDLAE-T inference on images one forward was not sized for: 1 x 3 x 2048^2 and 1 x 3 x 1024 x 4096 on the
released config (``[4,6,6,8]`` blocks, 4 refinement blocks, dim 48, hash weights), tile 512, overlap 32.

  (a) ``KDLAE_teacher.forward_tiled`` at tile_batch 16: tiles gathered and blended by the library's kernels;
  (b) the loop a user writes without it, on the same card: torch slicing, the module's ``forward`` at batch 1 per
      tile (graph replay on, as the module has it by default), ``E[...].add_``, ``W[...].add_(1)``, ``E.div_(W)``;
  (c) the untiled ``forward`` of the whole image, in a fresh child process after everything else (its workspace
      is sized from the full image): its time if it runs, the error text otherwise.

hipEvent timing around the whole call, three warm-up passes per route (launch by launch, capture, replay), then alternating
timed repeats of (a) and (b); the median per route, and for (b) the run-to-run spread (max - min) that the
acceptance uses: (a) may not be slower than (b) by more than that spread, and (a)'s outputs must be
``torch.equal`` to (b)'s.  Also recorded: the summed device time of the gather and blend launches of one (a) call
(each launch bracketed by events in a pass of its own) as a share of (a), and the staging bytes.  Writes one JSON
line to profiles/tile_probe.json.  Needs a GPU.
"""
from __future__ import annotations

import hashlib
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rethink_acoustic_image_enhancement_amd import _lib, tiling  # noqa: E402
from rethink_acoustic_image_enhancement_amd.hashweights import hash_images, load_hash_weights  # noqa: E402
from rethink_acoustic_image_enhancement_amd.KDLAE_model import KDLAE_teacher  # noqa: E402

TILE, OVERLAP, TILE_BATCH = 512, 32, 16
SHAPES = [(2048, 2048), (1024, 4096)]
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


def host_loop(m, img, rate):
    """Upstream Restormer's tiled demo loop around this module, per-axis tile clamp as the library has it."""
    B, _, H, W = img.shape
    p = tiling.tile_plan(H, W, TILE, OVERLAP)
    ys, xs = p.starts(H, W)
    E = torch.zeros((B, 3, H, W), device=img.device)
    Wt = torch.zeros_like(E)
    E2 = torch.zeros((B, 3, 2 * H, 2 * W), device=img.device)
    W2 = torch.zeros_like(E2)
    for b in range(B):
        for y in ys:
            for x in xs:
                o = m({"img": img[b:b + 1, :, y:y + p.th, x:x + p.tw],
                       "denoise_rate": rate[b:b + 1, :, y:y + p.th, x:x + p.tw]})
                E[b:b + 1, :, y:y + p.th, x:x + p.tw].add_(o["hq"])
                Wt[b:b + 1, :, y:y + p.th, x:x + p.tw].add_(1)
                E2[b:b + 1, :, 2 * y:2 * (y + p.th), 2 * x:2 * (x + p.tw)].add_(o["sr"])
                W2[b:b + 1, :, 2 * y:2 * (y + p.th), 2 * x:2 * (x + p.tw)].add_(1)
    return {"hq": E.div_(Wt), "sr": E2.div_(W2)}


def mover_ms(img, rate, p):
    """Device time of the gather and blend launches of one forward_tiled call, each bracketed on its own."""
    B, _, H, W = img.shape
    n = B * p.ni * p.nj
    st_hq = torch.rand((n, 3, p.th, p.tw), device=img.device)
    st_sr = torch.rand((n, 3, 2 * p.th, 2 * p.tw), device=img.device)
    calls = []
    for first in range(0, n, TILE_BATCH):
        count = min(TILE_BATCH, n - first)
        calls.append(("gather", lambda f=first, c=count: tiling.tile_gather(img, TILE, OVERLAP, f, c)))
        calls.append(("gather", lambda f=first, c=count: tiling.tile_gather(rate, TILE, OVERLAP, f, c)))
    calls.append(("blend", lambda: tiling.tile_blend(st_hq, B, H, W, TILE, OVERLAP, 1)))
    calls.append(("blend", lambda: tiling.tile_blend(st_sr, B, H, W, TILE, OVERLAP, 2)))
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
def untiled_child(H, W):
    """(c), in a process of its own: prints one JSON line."""
    dev = torch.device("cuda", 0)
    m = _model(dev)
    img, rate = _inputs(H, W, dev)
    try:
        need = _lib.lib().kdlae_t_workspace_bytes(m.engine(dev).handle, 1, H, W)
        m({"img": img, "denoise_rate": rate})   # sizes the workspace; the second call captures the graph
        m({"img": img, "denoise_rate": rate})
        torch.cuda.synchronize()
        ms = [_timed(lambda: m({"img": img, "denoise_rate": rate}))[0] for _ in range(REPEATS)]
        res = dict(_stats(ms), workspace_gib=need / 2**30)
    except RuntimeError as e:
        res = {"error": str(e).splitlines()[0][:400]}
    print("UNTILED " + json.dumps(res), flush=True)


@torch.no_grad()
def main():
    if not torch.cuda.is_available():
        raise SystemExit("tile_probe: no GPU")
    if len(sys.argv) == 4 and sys.argv[1] == "--untiled":
        return untiled_child(int(sys.argv[2]), int(sys.argv[3]))
    dev = torch.device("cuda", 0)
    m = _model(dev)
    cases = []
    for H, W in SHAPES:
        img, rate = _inputs(H, W, dev)
        p = tiling.tile_plan(H, W, TILE, OVERLAP)
        n = p.ni * p.nj
        inp = {"img": img, "denoise_rate": rate}

        def tiled():
            return m.forward_tiled(inp, TILE, OVERLAP, TILE_BATCH)

        def loop():
            return host_loop(m, img, rate)
        for _ in range(3):   # eager, capture, replay: every chunk shape of both routes has its graph
            out_a = tiled()
            out_b = loop()
        torch.cuda.synchronize()
        same = bool(torch.equal(out_a["hq"], out_b["hq"]) and torch.equal(out_a["sr"], out_b["sr"]))
        del out_a, out_b
        ms_a, ms_b = [], []
        for _ in range(REPEATS):   # alternating, so a drift of the card hits both routes
            ms_a.append(_timed(tiled)[0])
            ms_b.append(_timed(loop)[0])
        a, b = _stats(ms_a), _stats(ms_b)
        movers, launches = mover_ms(img, rate, p)
        case = {"shape": [1, 3, H, W], "tile": TILE, "tile_overlap": OVERLAP, "tile_batch": TILE_BATCH,
                "plan": p._asdict(), "tiles": n,
                "forward_tiled": a, "host_loop": b,
                "host_loop_over_forward_tiled": b["ms"] / a["ms"],
                "outputs_equal": same,
                "not_slower_than_host_loop_by_more_than_its_spread": bool(a["ms"] <= b["ms"] + b["spread_ms"]),
                "gather_ms": movers["gather"], "blend_ms": movers["blend"], "mover_launches": launches,
                "mover_share_of_forward_tiled": (movers["gather"] + movers["blend"]) / a["ms"],
                "staging_bytes": n * 3 * p.th * p.tw * 4 * 5}
        print(case, flush=True)
        cases.append(case)
        del img, rate, inp
    res = {"probe": "tile", "device": torch.cuda.get_device_name(0),
           "config": "KDLAE_teacher() defaults: num_blocks [4,6,6,8], 4 refinement blocks, dim 48, hash weights",
           "statistic": "hipEvent time of the whole call; 3 warm-up passes per route, then %d alternating timed "
                        "repeats: median, min, max, spread = max - min" % REPEATS,
           "host_loop": "torch slicing, forward at batch 1 per tile (graph replay on), add_ / add_(1) / div_",
           "library_sha256": hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest(), "cases": cases}
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "tile_probe.json")

    def write():
        with open(path, "w") as f:
            f.write(json.dumps(res) + "\n")
    write()
    # (c) last, each in a fresh process, with this process's device memory given back first
    m = None
    torch.cuda.empty_cache()
    for case in cases:
        _, _, H, W = case["shape"]
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--untiled", str(H), str(W)],
                               capture_output=True, text=True, timeout=240)
            lines = [ln for ln in r.stdout.splitlines() if ln.startswith("UNTILED ")]
            ok = r.returncode == 0 and bool(lines)
            case["untiled_forward"] = json.loads(lines[-1][len("UNTILED "):]) if ok else \
                {"error": f"child exit status {r.returncode}: " + r.stderr.strip()[-300:]}
        except subprocess.TimeoutExpired:
            ok = False
            case["untiled_forward"] = {"error": "no result within 240 s"}
        print(case["untiled_forward"], flush=True)
        write()
        if not ok:
            break   # nothing more on the device after an abnormal end
    print(json.dumps(res))
    if not all(c["outputs_equal"] for c in cases):
        raise SystemExit("tile_probe: forward_tiled and the host loop differ")


if __name__ == "__main__":
    main()
