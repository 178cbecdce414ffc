#!/usr/bin/env python
"""Record tests/golden/prepare_train.npz / .json from the reference's own statements.

    python tests/golden/make_golden_prepare.py <reference checkout>/Train

Nothing of the reference is restated here; its statements are located in its source through ``ast`` and executed:

* ``input_mask`` is imported from ``basicsr.data.paired_image_dataset`` (modules that are not installed get inert
  stand-ins as in make_golden_metrics.py);
* the progressive-learning block of ``basicsr/train.py`` is the run of statements of the training ``while`` body
  between the ``model.update_learning_rate(...)`` call and the ``model.feed_train_data(...)`` call.  It runs in a
  namespace that holds what ``main()`` has defined by then (``groups`` built as main() builds it, the yml lists,
  ``train_data``, ``logger_j`` all False so that the log line is skipped) with ``random`` and ``numpy.random``
  seeded;
* the ``phase == 'interpolation'`` and ``phase == 'test1'`` statements of ``Dataset_PairedMutiImage.__getitem__``
  run the same way on an HWC stack, with ``self.opt`` a two-key dict.

If a block is not found where described the script stops and writes nothing.  Cases, seeds and inputs come
from tests/prepare_oracle.py::progressive_cases / ::frame_cases (inputs are hash-generated, so they are not
stored); recorded per case: the seeds, the draws (stage, indices, x0, y0; for the frame rule the per-frame
probabilities and the keep masks, re-drawn from the same seeds) and the outputs.  Before anything is written
every output is compared with tests/prepare_oracle.py bit for bit, and so are the generator states afterwards.
"""
import ast
import importlib
import json
import os
import random
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
from make_golden_metrics import _InertFinder  # noqa: E402
from tests import prepare_oracle as po  # noqa: E402


def _calls(node, dotted):
    """Is ``node`` an expression statement calling ``dotted`` (e.g. 'model.feed_train_data')?"""
    if not (isinstance(node, ast.Expr) and isinstance(node.value, ast.Call)):
        return False
    try:
        return ast.unparse(node.value.func) == dotted
    except Exception:
        return False


def locate_progressive_block(train_py):
    tree = ast.parse(open(train_py).read(), train_py)
    for node in ast.walk(tree):
        if not isinstance(node, ast.While):
            continue
        lo = [i for i, s in enumerate(node.body) if _calls(s, "model.update_learning_rate")]
        hi = [i for i, s in enumerate(node.body) if _calls(s, "model.feed_train_data")]
        if len(lo) == 1 and len(hi) == 1 and lo[0] + 1 < hi[0]:
            mod = ast.Module(body=node.body[lo[0] + 1:hi[0]], type_ignores=[])
            return compile(mod, train_py, "exec"), (node.body[lo[0] + 1].lineno, node.body[hi[0] - 1].end_lineno)
    raise SystemExit("progressive block not found between update_learning_rate and feed_train_data: nothing written")


def locate_phase_block(dataset_py, phase):
    tree = ast.parse(open(dataset_py).read(), dataset_py)
    for cls in ast.walk(tree):
        if not (isinstance(cls, ast.ClassDef) and cls.name == "Dataset_PairedMutiImage"):
            continue
        for fn in cls.body:
            if not (isinstance(fn, ast.FunctionDef) and fn.name == "__getitem__"):
                continue
            hits = [s for s in fn.body if isinstance(s, ast.If) and isinstance(s.test, ast.Compare)
                    and ast.unparse(s.test.left) == "self.opt['phase']" and len(s.test.comparators) == 1
                    and isinstance(s.test.comparators[0], ast.Constant) and s.test.comparators[0].value == phase]
            if len(hits) == 1:
                mod = ast.Module(body=[hits[0]], type_ignores=[])
                return compile(mod, dataset_py, "exec"), (hits[0].lineno, hits[0].end_lineno)
    raise SystemExit(f"phase == {phase!r} block of Dataset_PairedMutiImage.__getitem__ not found: nothing written")


class _Logger:
    def info(self, *a, **k):
        pass


def main():
    train_dir = sys.argv[1]
    missing = []
    for root in ("cv2", "skimage", "scipy", "lmdb", "tqdm", "yaml", "torchvision", "tensorboard", "requests",
                 "einops", "natsort"):
        try:
            importlib.import_module(root)
        except Exception:
            missing.append(root)
    sys.meta_path.append(_InertFinder(missing))
    sys.path.insert(0, train_dir)
    import torch
    from basicsr.data.paired_image_dataset import input_mask

    train_py = os.path.join(train_dir, "basicsr", "train.py")
    dataset_py = os.path.join(train_dir, "basicsr", "data", "paired_image_dataset.py")
    block, block_lines = locate_progressive_block(train_py)
    arrays, meta = {}, {"source": {"progressive": f"basicsr/train.py:{block_lines[0]}-{block_lines[1]} (located "
                                                  "through ast, executed)",
                                   "input_mask": "basicsr.data.paired_image_dataset.input_mask (imported)"},
                        "stand_ins": missing, "progressive": {}, "frames": {}}

    def same(a, b):
        return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))

    for name, (cfg, it, py_seed, np_seed, lq, gt) in po.progressive_cases().items():
        def t(v):
            return {k: torch.from_numpy(a.copy()) for k, a in v.items()} if isinstance(v, dict) \
                else torch.from_numpy(v.copy())
        iters = cfg["iters"]
        ns = {"current_iter": it,
              "groups": np.array([sum(iters[0:i + 1]) for i in range(0, len(iters))]),
              "mini_gt_sizes": cfg["gt_sizes"], "mini_batch_sizes": cfg["mini_batch_sizes"], "probs": cfg["probs"],
              "prob": cfg["prob"], "gt_size": cfg["gt_size"], "batch_size": cfg["batch_size"], "scale": cfg["scale"],
              "logger_j": [False] * len(iters), "logger": _Logger(),
              "train_data": {"lq": t(lq), "gt": t(gt)},
              "random": random, "np": np, "torch": torch, "input_mask": input_mask}
        random.seed(py_seed)
        np.random.seed(np_seed)
        exec(block, ns)
        r_state, n_state = random.getstate(), np.random.get_state()[1].copy()
        ref_lq, ref_gt = ns["lq"], ns["gt"]

        def arr(v):
            return {k: a.numpy().copy() for k, a in v.items()} if isinstance(v, dict) else v.numpy().copy()
        ref_lq, ref_gt = arr(ref_lq), arr(ref_gt)
        draws = {"stage": int(ns["bs_j"]), "indices": [int(i) for i in ns["indices"]] if "indices" in ns else None,
                 "x0": int(ns.get("x0", 0)), "y0": int(ns.get("y0", 0))}
        # the oracle on the same seeds: same tensors, same draws, same generator states afterwards
        random.seed(py_seed)
        np.random.seed(np_seed)
        o_lq, o_gt, (j, indices, x0, y0, mp) = po.progressive(cfg, it, lq, gt)
        assert (j, indices, x0, y0) == (draws["stage"], draws["indices"], draws["x0"], draws["y0"]), (name, draws)
        assert random.getstate() == r_state and np.array_equal(np.random.get_state()[1], n_state), name
        for tag, ref, got in (("lq", ref_lq, o_lq), ("gt", ref_gt, o_gt)):
            for k in (ref if isinstance(ref, dict) else [None]):
                a, b = (ref[k], got[k]) if k is not None else (ref, got)
                assert same(a, b), f"{name}: oracle differs from the reference in {tag}{'.' + k if k else ''}"
        draws["mask_prob"] = repr(float(mp))
        for tag, v in (("out_lq", ref_lq), ("out_gt", ref_gt)):
            for k in (v if isinstance(v, dict) else [None]):
                arrays[f"progressive/{name}/{tag}" + (f"/{k}" if k else "")] = v[k] if k else v
        meta["progressive"][name] = {"cfg": cfg, "current_iter": it, "py_seed": py_seed, "np_seed": np_seed,
                                     "dict": isinstance(lq, dict), "draws": draws}
        print(name, draws)

    for phase in ("interpolation", "test1"):
        blk, lines = locate_phase_block(dataset_py, phase)
        meta["source"][phase] = f"basicsr/data/paired_image_dataset.py:{lines[0]}-{lines[1]} (located through ast, executed)"
        for name, (ph, prob, py_seed, np_seed, frames) in po.frame_cases().items():
            if ph != phase:
                continue
            B, F, H, W = frames.shape
            random.seed(py_seed)
            np.random.seed(np_seed)
            outs = []
            for b in range(B):
                ns = {"self": types.SimpleNamespace(opt={"phase": phase, "prob": prob}),
                      "lq_images_stacked": np.ascontiguousarray(frames[b].transpose(1, 2, 0)).copy(),
                      "random": random, "np": np, "input_mask": input_mask}
                exec(blk, ns)
                outs.append(ns["lq_images_stacked"].transpose(2, 0, 1).copy())
            ref = np.stack(outs).astype(np.float32)
            assert ref.dtype == np.float32 and outs[0].dtype == np.float32
            r_state, n_state = random.getstate(), np.random.get_state()[1].copy()
            # re-draw on the same seeds what the block drew: the test1 branches and the keep masks
            random.seed(py_seed)
            np.random.seed(np_seed)
            probs, keep = [], np.zeros((B, F, H, W), np.uint8)
            for b in range(B):
                row = []
                for f in range(F):
                    if phase == "test1":
                        row.append(prob + 0.6 if random.random() < 0.2 else prob)
                    else:
                        row.append(prob + 0.5 if f % 2 == 1 else prob)
                    keep[b, f] = po.numpy_keep(1, H, W, row[-1])[0]
                probs.append(row)
            assert random.getstate() == r_state and np.array_equal(np.random.get_state()[1], n_state), name
            got = np.stack([po.mask_frames(frames[b:b + 1], [min(p, 1.0) for p in probs[b]], phase == "interpolation",
                                           keep[b:b + 1])[0] for b in range(B)])
            assert same(ref, got), f"{name}: oracle differs from the reference"
            arrays[f"frames/{name}/out"], arrays[f"frames/{name}/keep"] = ref, keep
            meta["frames"][name] = {"phase": phase, "prob": prob, "py_seed": py_seed, "np_seed": np_seed,
                                    "probs": [[repr(float(p)) for p in row] for row in probs]}
            print(name, meta["frames"][name]["probs"])

    np.savez_compressed(os.path.join(HERE, "prepare_train.npz"), **arrays)
    with open(os.path.join(HERE, "prepare_train.json"), "w") as f:
        json.dump(meta, f, indent=1)
        f.write("\n")
    print("written:", len(arrays), "arrays")


if __name__ == "__main__":
    main()
