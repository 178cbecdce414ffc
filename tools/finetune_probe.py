"""Fine-tuning regimes of the KDLAE-T training step: ms per optimisation step, backward launches, workspace.

    python tools/finetune_probe.py [--steps 20] [--warmup 5] [--parent parent_train.json ...]
        > profiles/finetune_probe.json

Shape: the KDLAET.yml setting of `bench.py --workload train` (6 x 3 x 128^2, the full config, mixup, clip + AdamW).
Regimes: all parameters trainable; the reference's fine-tune regime (freeze_except_patch_embed_and_enhance:
patch_embed + the sr head); the sr head alone; the rate tail (output_param, refinement_out, output2) + the sr head.

Every regime runs in a child process of its own under `timeout`, one after the other; the first failure ends the
probe (nothing more is started on the device after a fault or a time limit).  A regime is timed like the benchmark:
warm-up steps, then `steps` steps between two device events and a host clock that ends in a synchronise; the window
is repeated three times and the spread of the three is recorded.  `--parent`: result lines of
`bench.py --workload train` taken on the parent commit on the same card in the same call; the all-trainable row
is then compared with them."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REGIMES = ("all", "reference", "sr_head", "rate_tail_sr_head")
SR = ("cen.", "upen.", "enhance.", "outputen.")
TAIL = ("output_param.", "refinement_out.", "output2.")


def run_regime(regime, steps, warmup, repeats=3):
    import numpy as np
    import torch

    import bench
    from rethink_acoustic_image_enhancement_amd.hashweights import hash_images, load_hash_weights
    from rethink_acoustic_image_enhancement_amd.KDLAE_model import KDLAE_teacher
    from rethink_acoustic_image_enhancement_amd.train import KDLAETrainer, freeze_except_patch_embed_and_enhance

    dev = torch.device("cuda", 0)
    B, H, W = 6, 128, 128
    model = KDLAE_teacher(**bench.KW)
    load_hash_weights(model)
    model = model.to(dev)
    if regime == "reference":
        freeze_except_patch_embed_and_enhance(model)
    img, rate = bench.make_inputs(1000, B, H, W)
    gt = {"hq": torch.from_numpy(np.stack([hash_images(f"train_gt:{i}", (3, H, W)) for i in range(B)])).to(dev),
          "sr": torch.from_numpy(np.stack([hash_images(f"train_gtsr:{i}", (3, 2 * H, 2 * W)) for i in range(B)])).to(dev)}
    batch = {"img": img.to(dev), "denoise_rate": rate.to(dev)}
    trainer = KDLAETrainer(model, mixing_augs={"mixup": True, "mixup_beta": 1.2, "use_identity": True})
    if regime == "sr_head":
        trainer.set_trainable(lambda k: k.startswith(SR))
    elif regime == "rate_tail_sr_head":
        trainer.set_trainable(lambda k: k.startswith(SR + TAIL))
    import random
    random.seed(0)
    torch.manual_seed(0)

    def step():
        lq_m, gt_m = trainer.feed_train_data(batch, gt)
        return trainer.optimize_parameters(lq_m, gt_m)

    for _ in range(warmup):
        step()
    torch.cuda.synchronize(dev)
    host_ms, dev_ms = [], []
    for _ in range(repeats):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        ev0.record()
        for _ in range(steps):
            loss = step()
        ev1.record()
        torch.cuda.synchronize(dev)
        host_ms.append((time.perf_counter() - t0) / steps * 1e3)
        dev_ms.append(ev0.elapsed_time(ev1) / steps)
    eng = trainer.engine
    n_train = sum(n for (_, n, _), t, u in zip(eng.keys, eng.trainable, eng.used) if t and u)
    return {"regime": regime, "ms_per_step": round(min(host_ms), 3),
            "ms_per_step_windows": [round(v, 3) for v in host_ms],
            "device_ms_per_step_windows": [round(v, 3) for v in dev_ms],
            "backward_launches": eng.backward_launches(),
            "workspace_bytes": int(eng._L.kdlae_tt_workspace_bytes(eng.handle, B, H, W)),
            "trainable_floats": n_train, "total_floats": sum(n for _, n, _ in eng.keys),
            "loss": float(loss), "steps": steps, "warmup": warmup}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regime", choices=REGIMES, help="(child) time one regime and print its JSON line")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=150, help="seconds per regime")
    ap.add_argument("--parent", nargs="*", default=[], help="parent-commit bench.py --workload train result files")
    args = ap.parse_args()
    if args.regime:
        print(json.dumps(run_regime(args.regime, args.steps, args.warmup)), flush=True)
        return 0
    rows = []
    for regime in REGIMES:   # one child per regime under its own time limit; stop at the first failure
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--regime", regime,
               "--steps", str(args.steps), "--warmup", str(args.warmup)]
        p = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            sys.stderr.write(f"finetune_probe: regime {regime} ended with status {p.returncode}; stopping\n")
            return p.returncode
        rows.append(json.loads(p.stdout.strip().splitlines()[-1]))
    base = rows[0]["ms_per_step"]
    for r in rows:
        r["speedup_vs_all"] = round(base / r["ms_per_step"], 3)
    out = {"shape": "6 x 3 x 128 x 128, full config (bench.py KW), mixup, L1LossSr, clip_grad_norm_ 0.01, AdamW",
           "timing": "host clock around `steps` steps ending in a device synchronise; best of three windows",
           "regimes": rows}
    parent = []
    for f in args.parent:
        with open(f) as fh:
            line = [ln for ln in fh.read().splitlines() if ln.startswith("{")][-1]
        parent.append(json.loads(line)["ms_per_step"])
    if parent:
        spread = max(parent) - min(parent)
        out["parent_commit"] = {"bench_train_ms_per_step": parent, "spread_ms": round(spread, 3),
                                "all_trainable_ms_per_step": base,
                                "all_trainable_minus_parent_best_ms": round(base - min(parent), 3),
                                "within_parent_spread": bool(min(parent) - spread <= base <= max(parent) + spread)}
    print(json.dumps(out, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
