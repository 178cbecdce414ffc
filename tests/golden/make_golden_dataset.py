#!/usr/bin/env python
"""Record tests/golden/dataset_sample.npz / .json from the reference's own dataset code.

    python tests/golden/make_golden_dataset.py <reference checkout>/Train

Nothing of the reference is restated here.  Its functions are imported and called (``paired_random_crop``,
``data_augmentation``, ``random_augmentation``, ``add_random_noise``, ``pad_image``, ``padding``), its methods are called
on an instance built without ``__init__`` (``multi_scale_padding``, ``multi_scale_crop``, ``sync_augment``,
``add_gaussian_noise``), the ``random.random() < 0.64`` mask block of ``Dataset_PairedMutiImage.__getitem__`` and the
``zero_ratio`` nudge statements of ``Dataset_SuperRestoration_param.__getitem__`` are located through ``ast`` inside
their ``phase == 'train'`` blocks and executed, and both ``__getitem__`` run whole on decoded images (file access
and decode, which are out of scope, are replaced: ``_read_img`` / ``_read_json`` of a subclass, and the module's
``imfrombytes`` handed the frame a fake file client returns).  Modules that are not installed get inert stand-ins
as in make_golden_metrics.py.

cv2 is among them where it is not installed.  The inert ``cv2`` is then given numpy stand-ins for the calls these
paths make: ``flip`` (np.flip), ``rotate`` (np.rot90), ``copyMakeBorder`` for BORDER_REFLECT_101 / BORDER_REFLECT
(np.pad 'reflect' / 'symmetric'), the constants, and ``cvtColor(.., COLOR_BGR2RGB)`` (channel reversal, reached through
``img2tensor`` by the whole teacher ``__getitem__`` only).  These are OpenCV's DOCUMENTED semantics, not measured
ones: the goldens recorded this way leave PARITY UNPINNED AGAINST REAL cv2; the json says which route recorded it.

Inputs are hash-generated (tests/dataset_oracle.py), so only outputs are stored.  Recorded per case: seeds, every
draw, generator states afterwards (as digests), outputs.  Every output is compared bit for bit with
tests/dataset_oracle.py before anything is written.
"""
import ast
import hashlib
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
from tests import dataset_oracle as do  # noqa: E402


state_digest = do.state_digest


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def cv2_stand_ins(cv2):
    cv2.BORDER_REFLECT, cv2.BORDER_REFLECT_101 = 2, 4
    cv2.ROTATE_90_CLOCKWISE, cv2.ROTATE_180, cv2.ROTATE_90_COUNTERCLOCKWISE = 0, 1, 2
    cv2.COLOR_BGR2RGB = 4
    cv2.flip = lambda img, code: np.ascontiguousarray(np.flip(img, 1 if code == 1 else 0))
    cv2.rotate = lambda img, code: np.ascontiguousarray(np.rot90(img, k={0: -1, 1: 2, 2: 1}[code]))

    def copy_make_border(img, top, bottom, left, right, mode):
        pad = ((top, bottom), (left, right)) + ((0, 0),) * (img.ndim - 2)
        return np.pad(img, pad, mode={2: "symmetric", 4: "reflect"}[mode])

    def cvt_color(img, code):
        assert code == cv2.COLOR_BGR2RGB
        return np.ascontiguousarray(img[:, :, ::-1])
    cv2.copyMakeBorder, cv2.cvtColor = copy_make_border, cvt_color


def train_if(tree, cls_name):
    for cls in ast.walk(tree):
        if isinstance(cls, ast.ClassDef) and cls.name == cls_name:
            for fn in cls.body:
                if isinstance(fn, ast.FunctionDef) and fn.name == "__getitem__":
                    hits = [s for s in fn.body if isinstance(s, ast.If) and ast.unparse(s.test) == "self.opt['phase'] == 'train'"]
                    if len(hits) == 1:
                        return hits[0]
    raise SystemExit(f"phase == 'train' block of {cls_name}.__getitem__ not found: nothing written")


def compiled(stmts, path, what):
    if not stmts:
        raise SystemExit(f"{what} not found: nothing written")
    return compile(ast.Module(body=stmts, type_ignores=[]), path, "exec"), f"{stmts[0].lineno}-{stmts[-1].end_lineno}"


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
    import cv2
    if "cv2" in missing:
        cv2_stand_ins(cv2)
    import basicsr.data.paired_image_dataset as pid
    from basicsr.data.transforms import data_augmentation, paired_random_crop, random_augmentation
    from basicsr.utils.img_util import padding

    dataset_py = os.path.join(train_dir, "basicsr", "data", "paired_image_dataset.py")
    tree = ast.parse(open(dataset_py).read(), dataset_py)
    s_train = train_if(tree, "Dataset_PairedMutiImage")
    mask_blk, mask_lines = compiled([s for s in s_train.body if isinstance(s, ast.If)
                                     and ast.unparse(s.test) == "random.random() < 0.64"], dataset_py, "train mask block")
    t_train = train_if(tree, "Dataset_SuperRestoration_param")
    idx = [i for i, s in enumerate(t_train.body) if isinstance(s, ast.Assign) and ast.unparse(s.targets[0]) == "zero_ratio"]
    nudge_blk, nudge_lines = compiled(t_train.body[idx[0]:idx[0] + 2] if len(idx) == 1 else [], dataset_py, "nudge statements")

    arrays = {}
    meta = {"cv2": "numpy stand-ins (documented semantics; parity unpinned against real cv2)" if "cv2" in missing
            else "real cv2 " + str(getattr(cv2, "__version__", "")), "stand_ins": missing,
            "source": {"train_mask": f"basicsr/data/paired_image_dataset.py:{mask_lines} (located through ast, executed)",
                       "nudge": f"basicsr/data/paired_image_dataset.py:{nudge_lines} (located through ast, executed)"},
            "steps": {}, "train": {}}
    f32 = do.to_float

    # ---- single steps
    img = f32(do.hash_u8("step/hwc", (13, 6, 3)))
    grey = f32(do.hash_u8("step/grey", (5, 7)))
    for mode in range(8):
        ref = data_augmentation(img, mode)
        code = do.code_of(lambda a, m=mode: do.data_augmentation_model(a, m))
        assert same(ref, do.dihedral(img, code)), mode
        arrays[f"steps/data_augmentation/{mode}"] = np.ascontiguousarray(ref)
    random.seed(5)
    a, b = random_augmentation(img, img[::-1])
    random.seed(5)
    flag = random.randint(0, 7)
    assert same(a, do.data_augmentation_model(img, flag)) and same(b, do.data_augmentation_model(img[::-1], flag))
    meta["steps"]["random_augmentation"] = {"py_seed": 5, "flag": flag, "state": state_digest()}
    arrays["steps/random_augmentation/0"] = a
    for (H, W) in ((8, 8), (11, 9)):
        ref = pid.pad_image(grey, H, W)
        assert same(ref, do.centre_pad(grey, H, W))
        arrays[f"steps/pad_image/{H}x{W}"] = ref
    for g in (6, 8, 14):     # pads of 0.., up to more than the image
        stack = np.ascontiguousarray(img[:, :, :])
        a, b = padding(stack, stack[::-1].copy(), g)
        Hp, Wp = max(13, g), max(6, g)
        assert same(a, do.edge_pad(stack, Hp, Wp, "symmetric")) and same(b, do.edge_pad(stack[::-1], Hp, Wp, "symmetric"))
        arrays[f"steps/padding/{g}"] = a
    random.seed(6)
    gt2 = f32(do.hash_u8("step/gt2", (26, 12, 3)))
    a, b = paired_random_crop(gt2, img, 5, 2, "p")
    random.seed(6)
    top, left = random.randint(0, 13 - 5), random.randint(0, 6 - 5)
    assert same(b, img[top:top + 5, left:left + 5]) and same(a, gt2[2 * top:2 * top + 10, 2 * left:2 * left + 10])
    meta["steps"]["paired_random_crop"] = {"py_seed": 6, "top": top, "left": left, "state": state_digest()}
    arrays["steps/paired_random_crop/gt"], arrays["steps/paired_random_crop/lq"] = np.ascontiguousarray(a), np.ascontiguousarray(b)
    np.random.seed(7)
    ref = pid.add_random_noise(img)
    np.random.seed(7)
    z = np.random.standard_normal(img.shape)
    assert same(ref, do.add_noise(img, z, 0.3, 0.7)), "add_random_noise: loc + scale * z differs from numpy's normal"
    meta["steps"]["add_random_noise"] = {"np_seed": 7, "state": state_digest()}
    arrays["steps/add_random_noise/out"] = ref

    T = pid.Dataset_SuperRestoration_param
    t = object.__new__(T)
    t.gt_size, t.lq_size, t.sr_size, t.sr_scale = 8, 8, 16, 2
    sr = f32(do.hash_u8("step/sr", (26, 12, 3)))
    a, b, c = t.multi_scale_padding(img, img[::-1].copy(), sr)          # 13x6 -> 13x8, 26x12 -> 26x16
    assert same(a, do.edge_pad(img, 13, 8, "reflect101")) and same(c, do.edge_pad(sr, 26, 16, "reflect101"))
    arrays["steps/multi_scale_padding/gt"], arrays["steps/multi_scale_padding/sr"] = a, c
    random.seed(8)
    big, big_sr = f32(do.hash_u8("step/big", (12, 14, 3))), f32(do.hash_u8("step/big_sr", (24, 28, 3)))
    a, b, c = t.multi_scale_crop(big, big[::-1].copy(), big_sr, "p")
    random.seed(8)
    top, left = random.randint(1, 12 - 1 - 8), random.randint(1, 14 - 1 - 8)
    assert same(a, big[top:top + 8, left:left + 8]) and same(c, big_sr[2 * top:2 * top + 16, 2 * left:2 * left + 16])
    meta["steps"]["multi_scale_crop"] = {"py_seed": 8, "top": top, "left": left, "state": state_digest()}
    arrays["steps/multi_scale_crop/gt"], arrays["steps/multi_scale_crop/sr"] = np.ascontiguousarray(a), np.ascontiguousarray(c)
    np.random.seed(9)
    ref = t.add_gaussian_noise(img)
    np.random.seed(9)
    sigma = np.random.uniform(1, 30)
    assert same(ref, do.add_noise(img, np.random.randn(*img.shape), 0.0, sigma, 255.0))
    meta["steps"]["add_gaussian_noise"] = {"np_seed": 9, "sigma": repr(float(sigma)), "state": state_digest()}
    arrays["steps/add_gaussian_noise/out"] = ref
    meta["steps"]["sync_augment"] = {}
    seen = set()
    for seed in range(400):  # the first seed of each of the 16 (hflip, vflip, rot) combinations
        if len(seen) == 16:
            break
        random.seed(seed)
        if (random.random() < 0.5, random.random() < 0.5, random.choice([None, 90, 180, 270])) in seen:
            continue
        random.seed(seed)
        a, b, c = t.sync_augment(img, img[::-1].copy(), sr)
        random.seed(seed)
        hf, vf = random.random() < 0.5, random.random() < 0.5
        rot = random.choice([None, 90, 180, 270])
        assert same(a, do.sync_augment_model(img, hf, vf, rot)) and same(c, do.sync_augment_model(sr, hf, vf, rot)), seed
        seen.add((hf, vf, rot))
        meta["steps"]["sync_augment"][str(seed)] = {"hflip": hf, "vflip": vf, "rot": rot, "state": state_digest()}
        arrays[f"steps/sync_augment/{seed}"] = np.ascontiguousarray(a)
    assert len({(v["hflip"], v["vflip"], v["rot"]) for v in meta["steps"]["sync_augment"].values()}) == 16
    for name, zf in (("below", 0.05), ("above", 0.2)):
        x = f32(do.hash_u8("step/nudge/" + name, (9, 8, 3), zf))
        ns = {"img_lq": x.copy(), "np": np}
        exec(nudge_blk, ns)
        got = do.finish(x.transpose(2, 0, 1), 0.10).transpose(1, 2, 0)
        assert ns["img_lq"].dtype == np.float32 and same(ns["img_lq"], got), name
        arrays[f"steps/nudge/{name}"] = ns["img_lq"]

    # ---- the train-phase mask rule, item after item
    for name, (prob, py_seed, np_seed, frames) in do.train_cases().items():
        for route in ("ref", "oracle"):
            random.seed(py_seed)
            np.random.seed(np_seed)
            outs, rows = [], []
            for b in range(frames.shape[0]):
                if route == "ref":
                    ns = {"self": types.SimpleNamespace(opt={"phase": "train", "prob": prob}), "random": random, "np": np,
                          "lq_images_stacked": np.ascontiguousarray(frames[b].transpose(1, 2, 0)).copy(),
                          "input_mask": pid.input_mask}
                    exec(mask_blk, ns)
                    assert ns["lq_images_stacked"].dtype == np.float32
                    outs.append(ns["lq_images_stacked"].transpose(2, 0, 1).copy())
                else:
                    o, row, interp = do.train_phase(frames[b], prob)
                    outs.append(o)
                    rows.append({"probs": [repr(float(p)) for p in row], "interpolate": interp})
            if route == "ref":
                ref, digest = np.stack(outs), state_digest()
            else:
                assert same(ref, np.stack(outs)) and digest == state_digest(), f"{name}: oracle differs from the reference"
        arrays[f"train/{name}"] = ref
        meta["train"][name] = {"prob": prob, "py_seed": py_seed, "np_seed": np_seed, "rows": rows, "state": digest}

    # ---- whole __getitem__, teacher
    py_seed, np_seed, g, samples = do.teacher_batch()

    class Teacher(T):
        def __init__(self):
            self.opt = {"phase": "train"}
            self.file_client, self.denoise_rate, self.mean, self.std, self.geometric_augs = True, True, None, None, True
            self.gt_size, self.lq_size, self.sr_size, self.sr_scale = g, g, 2 * g, 2
            self.paths = [{"gt_path": (b, 1), "lq_path": (b, 0), "sr_path": (b, 2), "param_path": b}
                          for b in range(len(samples))]

        def _read_img(self, path, key):
            return f32(samples[path[0]][path[1]])

        def _read_json(self, path, key):
            return {"denoise_rate": samples[path][3]}

    ds = Teacher()
    random.seed(py_seed)
    np.random.seed(np_seed)
    ref = [ds[b] for b in range(len(samples))]
    digest = state_digest()
    random.seed(py_seed)
    np.random.seed(np_seed)
    draws = []
    for b, (lq, gt, sr_, rate) in enumerate(samples):
        img_, rate_, hq_, sr_o, d = do.teacher_sample(lq, gt, sr_, rate, g)
        for tag, r, o in (("img", ref[b]["lq"]["img"], img_), ("denoise_rate", ref[b]["lq"]["denoise_rate"], rate_),
                          ("hq", ref[b]["gt"]["hq"], hq_), ("sr", ref[b]["gt"]["sr"], sr_o)):
            assert same(r.numpy(), o), f"teacher sample {b}: oracle differs from the reference in {tag}"
            arrays[f"teacher/{b}/{tag}"] = o
        draws.append({"top": d[0], "left": d[1], "sigma": None if d[2] is None else repr(float(d[2])), "hflip": d[3],
                      "vflip": d[4], "rot": d[5]})
    assert digest == state_digest(), "teacher: generator states differ"
    assert draws[0]["sigma"] is not None, "teacher sample 0 must draw the noise"
    meta["teacher"] = {"py_seed": py_seed, "np_seed": np_seed, "gt_size": g, "draws": draws, "state": digest}

    # ---- whole __getitem__, student
    py_seed, np_seed, g, prob, bursts = do.student_batch()
    F = len(bursts[0][0])
    pid.imfrombytes = lambda content, flag="color", float32=False: f32(bursts[content[0]][content[1]][content[2]])

    class Student(pid.Dataset_PairedMutiImage):
        def __init__(self):
            self.opt = {"phase": "train", "scale": 1, "gt_size": g, "prob": prob}
            self.file_client = types.SimpleNamespace(get=lambda path, key: path)
            self.mean = self.std = None
            self.geometric_augs = True
            self.paths = [[{"gt_path": (b, 1, f), "lq_path": (b, 0, f)} for f in range(F)] for b in range(len(bursts))]

    ds = Student()
    random.seed(py_seed)
    np.random.seed(np_seed)
    ref = [ds[b] for b in range(len(bursts))]
    digest = state_digest()
    random.seed(py_seed)
    np.random.seed(np_seed)
    draws = []
    for b, (lqf, gtf) in enumerate(bursts):
        lq_, gt_, d = do.student_sample(lqf, gtf, g, prob)
        assert same(ref[b]["lq"].numpy(), lq_) and same(ref[b]["gt"].numpy(), gt_), f"student sample {b}: oracle differs"
        arrays[f"student/{b}/lq"], arrays[f"student/{b}/gt"] = lq_, gt_
        draws.append({"top": d[0], "left": d[1], "probs": [repr(float(p)) for p in d[2]], "interpolate": d[3],
                      "noise": bool(d[4]), "mode": d[5]})
    assert digest == state_digest(), "student: generator states differ"
    assert [d["noise"] for d in draws] == [False, True], draws
    meta["student"] = {"py_seed": py_seed, "np_seed": np_seed, "gt_size": g, "prob": prob, "draws": draws, "state": digest}

    np.savez_compressed(os.path.join(HERE, "dataset_sample.npz"), **arrays)
    with open(os.path.join(HERE, "dataset_sample.json"), "w") as f:
        json.dump(meta, f, indent=1)
        f.write("\n")
    print("written:", len(arrays), "arrays")


if __name__ == "__main__":
    main()
