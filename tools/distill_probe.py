#!/usr/bin/env python
"""Distillation labels on the device against the loop they replace, on the same card, in one process.

Case "labels": a gray u8 clip 1 x 64 x 512^2 through the paper's KDLAE-T (default constructor, hash weights, eval,
denoise_rate 0.6):

  (a) ``distill.teacher_labels_u8`` (``teacher_batch`` 16: one expand launch, one forward, one collapse per chunk);
  (b) the loop a user writes without it: per frame, replicate the gray frame to three channels,
      ``pipeline.enhance_u8``, the 8-bit gray rule on the R, G, B bytes with integer torch ops on the device.  The
      loop is given every advantage: no copy to the host and no image file is written or read.

Case "step": one optimisation step at KDLAES.yml's first stage, 4 x 7 x 128^2, student hidden [16,32,64]:

  (a) ``DistillTrainer.optimize_parameters(lq)`` (labels made by the teacher inside the step, ``label_mode`` mean);
  (b) ``KDLAESTrainer.optimize_parameters(lq, labels)`` with the labels ready: the step without its label cost.

Wall time of one call ending in a device synchronise (``time.perf_counter``); WARMUP untimed calls per route, then
ROUNDS timed ones per route, the two routes alternating and swapping order every round.  Per route every sample, the
median, and the spread, which is defined here, before any number is read, as max - min of the route's samples.  The
only claim checked for "labels": (a)'s median may not exceed (b)'s by more than (b)'s spread.  Also recorded: the
device time (HIP events) of the expand and collapse launches of one (a) call run on their own, and their share of
(a)'s median; and whether both routes returned equal bytes.  "step" records what online labels cost a step; (a)
contains 28 teacher forwards that (b) does not, so no claim is made about it.
Writes one JSON line to profiles/distill_probe.json (or to the path given).  Needs a GPU.
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
from rethink_acoustic_image_enhancement_amd import _lib, distill  # noqa: E402
from rethink_acoustic_image_enhancement_amd.hashweights import hash_images, load_hash_weights  # noqa: E402
from rethink_acoustic_image_enhancement_amd.KDLAE_model import KDLAE_student, KDLAE_teacher  # noqa: E402
from rethink_acoustic_image_enhancement_amd.pipeline import enhance_u8, padded_size  # noqa: E402
from rethink_acoustic_image_enhancement_amd.train import DistillTrainer, KDLAESTrainer  # noqa: E402

RATE = 0.6
CLIP = (1, 64, 512, 512)
STEP = (4, 7, 128, 128)
TEACHER_BATCH = 16
WARMUP, ROUNDS = 2, 7


def host_loop_u8(teacher, clip, rate):
    B, T, h, w = clip.shape
    out = torch.empty_like(clip)
    for b in range(B):
        for t in range(T):
            rep = clip[b, t][None, :, :, None].expand(1, h, w, 3).contiguous()
            v = enhance_u8(teacher, rep, rate)[0][0].to(torch.int32)
            out[b, t] = ((1868 * v[..., 2] + 9617 * v[..., 1] + 4899 * v[..., 0] + 8192) >> 14).to(torch.uint8)
    return out


def _stats(ms):
    s = sorted(ms)
    return {"samples_ms": ms, "ms": s[len(s) // 2], "ms_min": s[0], "ms_max": s[-1], "spread_ms": s[-1] - s[0]}


def _alternate(routes, dev):
    """routes: {name: callable} -> ({name: stats}, {name: last result})."""
    names = list(routes)
    last = {}
    for n in names:
        for _ in range(WARMUP):
            last[n] = routes[n]()
    torch.cuda.synchronize(dev)
    ms = {n: [] for n in names}
    for r in range(ROUNDS):
        for k in range(len(names)):
            n = names[(r + k) % len(names)]
            t0 = time.perf_counter()
            last[n] = routes[n]()
            torch.cuda.synchronize(dev)
            ms[n].append((time.perf_counter() - t0) * 1e3)
    return {n: _stats(v) for n, v in ms.items()}, last


def _launch_share(clip, rate_items, dev):
    """Device time of the expand and collapse launches of one teacher_labels_u8 call, run without the forwards."""
    B, T, h, w = clip.shape
    H, W = padded_size(h, w, 8)
    plan = distill.chunks(B * T, TEACHER_BATCH)
    tb = plan[0][1]
    img = torch.empty((tb, 3, H, W), device=dev)
    rmap = torch.empty((tb, 1, H, W), device=dev)
    hq = torch.rand((tb, 3, H, W), device=dev)
    out = torch.empty((B, T, h, w), dtype=torch.uint8, device=dev)
    samples = []
    for i in range(WARMUP + ROUNDS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for j0, n in plan:
            distill.distill_expand(clip, rate_items, j0, n, img[:n], rmap[:n])
            distill.distill_collapse(hq[:n], out, j0, n, "file", clip)
        e1.record()
        torch.cuda.synchronize(dev)
        if i >= WARMUP:
            samples.append(e0.elapsed_time(e1))
    return samples, 2 * len(plan)


@torch.no_grad()
def main():
    if not torch.cuda.is_available():
        raise SystemExit("distill_probe: no GPU")
    dev = torch.device("cuda", 0)
    teacher = KDLAE_teacher()
    load_hash_weights(teacher)
    teacher = teacher.to(dev).eval()

    clip = torch.randint(0, 256, CLIP, dtype=torch.uint8, generator=torch.Generator().manual_seed(64)).to(dev)
    st, last = _alternate({"device_route": lambda: distill.teacher_labels_u8(teacher, clip, RATE, TEACHER_BATCH),
                           "host_loop": lambda: host_loop_u8(teacher, clip, RATE)}, dev)
    equal = bool(torch.equal(last["device_route"], last["host_loop"]))
    launch_ms, launches = _launch_share(clip, distill.item_rates(RATE, CLIP[0], CLIP[1], dev), dev)
    lm = sorted(launch_ms)[len(launch_ms) // 2]
    a, b = st["device_route"], st["host_loop"]
    labels = {"shape": list(CLIP), "teacher_batch": TEACHER_BATCH, "routes": st, "outputs_equal": equal,
              "expand_collapse": {"launches": launches, "samples_ms": launch_ms, "ms": lm, "share_of_device_route": lm / a["ms"]},
              "host_loop_over_device_route": b["ms"] / a["ms"],
              "device_route_not_slower_than_host_loop_by_more_than_its_spread": bool(a["ms"] <= b["ms"] + b["spread_ms"])}
    print(labels, flush=True)

    def student():
        m = KDLAE_student(hidden_channels=[16, 32, 64])
        load_hash_weights(m)
        return m.to(dev)

    lq = torch.from_numpy(hash_images("distill_probe:lq", STEP, 0.0, 1.0)).to(dev)
    with torch.enable_grad():
        dt = DistillTrainer(student(), teacher, RATE, teacher_batch=TEACHER_BATCH)
        kt = KDLAESTrainer(student())
        ready = distill.teacher_labels(teacher, lq, RATE, mode="mean", teacher_batch=TEACHER_BATCH)
        st2, _ = _alternate({"distill_step": lambda: dt.optimize_parameters(lq),
                             "step_with_ready_labels": lambda: kt.optimize_parameters(lq, ready)}, dev)
    same = bool(torch.equal(dt.theta, kt.theta))
    step = {"shape": list(STEP), "teacher_batch": TEACHER_BATCH, "label_mode": "mean", "routes": st2,
            "parameters_equal_after_the_same_steps": same,
            "distill_step_over_step_with_ready_labels": st2["distill_step"]["ms"] / st2["step_with_ready_labels"]["ms"]}
    print(step, flush=True)

    res = {"probe": "distill", "device": torch.cuda.get_device_name(0),
           "config": "KDLAE_teacher() (dim 48, blocks [4,6,6,8], 4 refinement blocks), KDLAE_student(hidden [16,32,64]), "
                     "hash weights, denoise_rate 0.6",
           "statistic": "host wall time of one call ending in a device synchronise; %d warm-up calls per route, then %d "
                        "timed ones, the routes alternating and swapping order every round; median, min, max, spread = "
                        "max - min.  expand_collapse: HIP-event time of those launches alone" % (WARMUP, ROUNDS),
           "host_loop": "per frame: replicate to [1,h,w,3], enhance_u8, the gray rule in integer torch ops on the "
                        "device; no host copy, no image file",
           "library_sha256": hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest(),
           "labels": labels, "step": step}
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "distill_probe.json")
    with open(path, "w") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps(res))
    if not equal or not same:
        raise SystemExit("distill_probe: the routes differ")


if __name__ == "__main__":
    main()
