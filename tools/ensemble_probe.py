#!/usr/bin/env python
"""Self-ensemble KDLAE-T inference (``"d8"``, ``ens_batch`` 8) at 1 x 3 x 512^2 and 16 x 3 x 512^2 (and that
batch at ``ens_batch`` 1) on the released config (``[4,6,6,8]`` blocks, 4 refinement blocks, dim 48, hash weights),
one MI355X.

  (a) ``KDLAE_teacher.forward_ensemble``: views gathered and merged by the library's kernels, the eight views of
      the whole batch in one forward;
  (b) the loop a user writes without it, same module, same card: ``torch.rot90`` / ``torch.flip`` of image and rate
      map, the module's ``forward`` at batch B per view (graph replay on, as the module has it by default), the
      inverse ``rot90`` / ``flip`` of ``hq`` and ``sr``, ``E.add_``, one ``E.div_``.

hipEvent timing around the whole call, three warm-up passes per route (launch by launch, capture, replay), then
alternating timed repeats of (a) and (b) in one process; the median per route and each route's run-to-run spread
(max - min).  The acceptance: (a) may not be slower than (b) by more than (b)'s spread, and (a)'s outputs must be
``torch.equal`` to (b)'s.  Also recorded: the summed device time of the gather and merge launches of one (a) call
(each launch bracketed by events in a pass of its own) as a share of (a).  Writes one JSON line to
profiles/ensemble_probe.json.  Needs a GPU."""
from __future__ import annotations

import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rethink_acoustic_image_enhancement_amd import ensemble  # noqa: E402
from rethink_acoustic_image_enhancement_amd.hashweights import hash_images, load_hash_weights  # noqa: E402
from rethink_acoustic_image_enhancement_amd.KDLAE_model import KDLAE_teacher  # noqa: E402

MODES = "d8"
# (B, H, W, ens_batch).  The first two are the stated cases.  At 16 x 3 x 512^2 eight views of the whole batch are one
# forward at batch 128, whose workspace does not fit the card: that case records the refusal, and the third row
# (one view of the batch a forward, the host loop's own batch) is there beside it, not in its place.
CASES = [(1, 512, 512, 8), (16, 512, 512, 8), (16, 512, 512, 1)]
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


def host_loop(m, img, rate):
    E = E2 = None
    for mode in ensemble.MODES:
        k = mode // 2
        a, r = torch.rot90(img, k, (-2, -1)), torch.rot90(rate, k, (-2, -1))
        if mode % 2:
            a, r = a.flip(-2), r.flip(-2)
        o = m({"img": a.contiguous(), "denoise_rate": r.contiguous()})
        hq, sr = o["hq"], o["sr"]
        if mode % 2:
            hq, sr = hq.flip(-2), sr.flip(-2)
        hq, sr = torch.rot90(hq, -k, (-2, -1)), torch.rot90(sr, -k, (-2, -1))
        if E is None:
            E, E2 = torch.zeros_like(hq), torch.zeros_like(sr)
        E.add_(hq)
        E2.add_(sr)
    return {"hq": E.div_(len(ensemble.MODES)), "sr": E2.div_(len(ensemble.MODES))}


def glue_ms(img, rate, oc):
    """Device time of the launches forward_ensemble adds to its forwards: two gathers, two merges."""
    B, C, H, W = img.shape
    mask = ensemble.mode_mask(MODES)
    st_hq = torch.randn(8 * B * oc * H * W, device=img.device)
    st_sr = torch.randn(8 * B * oc * 4 * H * W, device=img.device)
    steps = [lambda: ensemble.ens_gather(img, mask), lambda: ensemble.ens_gather(rate, mask),
             lambda: ensemble.ens_merge(st_hq, B, H, W, mask), lambda: ensemble.ens_merge(st_sr, B, 2 * H, 2 * W, mask)]
    for s in steps:
        s()
    torch.cuda.synchronize()
    return sum(sorted(_timed(s)[0] for _ in range(REPEATS))[REPEATS // 2] for s in steps)


def main():
    dev = torch.device("cuda", 0)
    m = KDLAE_teacher()
    load_hash_weights(m)
    m = m.to(dev).eval()
    rows = []
    with torch.no_grad():
        for B, H, W, ENS_BATCH in CASES:
            img = torch.from_numpy(hash_images(f"ensemble_probe:{B}x{H}x{W}", (B, 3, H, W))).to(dev)
            rate = torch.linspace(0.1, 0.9, H * W, device=dev).view(1, 1, H, W).repeat(B, 1, 1, 1).contiguous()
            call = lambda: m.forward_ensemble({"img": img, "denoise_rate": rate}, MODES, ENS_BATCH)   # noqa: E731
            loop = lambda: host_loop(m, img, rate)                                                    # noqa: E731
            try:
                for _ in range(3):
                    a, b = call(), loop()
            except torch.OutOfMemoryError as e:
                rows.append({"shape": [B, 3, H, W], "modes": MODES, "ens_batch": ENS_BATCH, "measured": False,
                             "error": str(e).split(". GPU")[0]})
                print(json.dumps(rows[-1]), flush=True)
                torch.cuda.empty_cache()
                continue
            torch.cuda.synchronize()
            equal = torch.equal(a["hq"], b["hq"]) and torch.equal(a["sr"], b["sr"])
            del a, b
            t_call, t_loop = [], []
            for _ in range(REPEATS):
                t_call.append(_timed(call)[0])
                t_loop.append(_timed(loop)[0])
            glue = glue_ms(img, rate, 3)
            sc, sl = _stats(t_call), _stats(t_loop)
            rows.append({"shape": [B, 3, H, W], "modes": MODES, "ens_batch": ENS_BATCH, "forward_ensemble": sc,
                         "host_loop": sl, "outputs_equal": bool(equal), "gather_merge_ms": glue,
                         "gather_merge_share": glue / sc["ms"],
                         "accepted": bool(equal and sc["ms"] <= sl["ms"] + sl["spread_ms"])})
            print(json.dumps(rows[-1]), flush=True)
            torch.cuda.empty_cache()
    rec = {"probe": "ensemble_probe", "device": torch.cuda.get_device_name(0), "cases": rows}
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "ensemble_probe.json"), "w") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
