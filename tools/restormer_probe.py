#!/usr/bin/env python3
"""Plain Restormer beside the KDLAE_teacher(params='none', static='none') route it shares its kernels with.

    python tools/restormer_probe.py [--out profiles/restormer_probe.json] [--repeats 5]

Two workloads at the released width (dim 48, [4,6,6,8] blocks, BiasFree), each timed for both models on the
same card in the same process, interleaved, ``--repeats`` times (a repeat = the mean of ``--iters`` calls between
two device synchronisations, after a warm-up):

* forward: ``Restormer`` at 16 x 3 x 512^2 (eval, HIP-graph replay) / the teacher's dict forward;
* training step: ``RestormerTrainer`` at 6 x 3 x 128^2 (Restomer.yml's batch; forward, L1LossSonar, backward,
  clip + AdamW) / ``KDLAETrainer`` (L1LossSr on hq only).

The record holds every repeat, the median, the spread (max - min) / median per model and the ratio of the
medians.  The two routes launch the same network kernels, so a ratio outside the spreads is a finding."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rethink_acoustic_image_enhancement_amd.hashweights import hash_images, load_hash_weights  # noqa: E402
from rethink_acoustic_image_enhancement_amd.KDLAE_model import KDLAE_teacher, Restormer  # noqa: E402
from rethink_acoustic_image_enhancement_amd.train import KDLAETrainer, RestormerTrainer  # noqa: E402

DEV = torch.device("cuda", 0)
KW = dict(dim=48, num_blocks=[4, 6, 6, 8], num_refinement_blocks=4, heads=[1, 2, 4, 8], ffn_expansion_factor=2.66,
          bias=False, LayerNorm_type="BiasFree")


def _timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def _compare(fns, repeats, iters, warmup):
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    ms = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            ms[k].append(_timed(fn, iters))
    out = {}
    for k, v in ms.items():
        med = statistics.median(v)
        out[k] = {"ms": [round(x, 4) for x in v], "median_ms": round(med, 4), "spread": round((max(v) - min(v)) / med, 5)}
    out["ratio_restormer_over_teacher"] = round(out["restormer"]["median_ms"] / out["teacher"]["median_ms"], 5)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/restormer_probe.json")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()

    r = Restormer(**KW)
    load_hash_weights(r)
    r = r.to(DEV)
    t = KDLAE_teacher(params="none", static="none", **KW).to(DEV)
    load_hash_weights(t)
    t.load_state_dict(r.state_dict(), strict=False)
    res = {"device": torch.cuda.get_device_name(0), "config": KW, "repeats": a.repeats, "iters": a.iters}

    x = torch.from_numpy(hash_images("probe:restormer:fwd", (16, 3, 512, 512))).to(DEV)
    r.eval(), t.eval()
    with torch.no_grad():
        same = torch.equal(r(x), t({"img": x, "denoise_rate": None})["hq"])
        res["forward_16x3x512x512"] = _compare(
            {"restormer": lambda: r(x), "teacher": lambda: t({"img": x, "denoise_rate": None})}, a.repeats, a.iters,
            a.warmup)
    res["forward_16x3x512x512"]["outputs_bit_equal"] = bool(same)
    del x
    torch.cuda.empty_cache()

    lq = torch.from_numpy(hash_images("probe:restormer:lq", (6, 3, 128, 128))).to(DEV)
    gt = torch.from_numpy(hash_images("probe:restormer:gt", (6, 3, 128, 128))).to(DEV)
    rt, tt = RestormerTrainer(r.train()), KDLAETrainer(t.train())
    res["train_step_6x3x128x128"] = _compare(
        {"restormer": lambda: rt.optimize_parameters(lq, gt),
         "teacher": lambda: tt.optimize_parameters({"img": lq, "denoise_rate": None}, {"hq": gt})}, a.repeats,
        max(a.iters, 5), a.warmup)
    res["train_step_6x3x128x128"]["backward_launches"] = {"restormer": rt.engine.backward_launches(),
                                                          "teacher": tt.engine.backward_launches()}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
