"""numpy model of the dataset sample transforms (csrc/data.hip, rethink_acoustic_image_enhancement_amd/dataset.py):
the per-sample steps of Dataset_SuperRestoration_param / Dataset_PairedMutiImage
(Train/basicsr/data/paired_image_dataset.py:902-982, 160-294) by direct indexing: ``np.pad``, slicing, ``np.rot90`` /
``np.flip``, float64 noise arithmetic.  Pinned to goldens recorded from the reference's own statements
(tests/golden/make_golden_dataset.py) by tests/test_dataset.py; the GPU tests compare the kernels with it bit for
bit.  The Philox / Box-Muller normals are modelled in float64 (the kernel evaluates them in fp32).
"""
import hashlib
import random

import numpy as np

from tests import prepare_oracle as po


# ------------------------------------------------------------------ inputs (hash-generated, never stored)
def hash_u8(tag, shape, zero_frac=0.0, one_frac=0.0):
    """Deterministic u8 array; ``zero_frac`` / ``one_frac`` of the pixels are forced to 0 / 255."""
    n = int(np.prod(shape))
    buf = b""
    i = 0
    while len(buf) < 2 * n:
        buf += hashlib.sha256(f"dataset/{tag}/{i}".encode()).digest()
        i += 1
    a = np.frombuffer(buf[:2 * n], np.uint8).reshape(n, 2)
    v, sel = a[:, 0].copy(), a[:, 1].astype(np.float64) / 256.0
    v[sel < zero_frac] = 0
    v[(sel >= zero_frac) & (sel < zero_frac + one_frac)] = 255
    return v.reshape(shape)


def state_digest():
    """sha256 over both host generators' states."""
    h = hashlib.sha256(repr(random.getstate()).encode())
    s = np.random.get_state()
    h.update(s[1].tobytes() + repr(s[2:]).encode())
    return h.hexdigest()


# ------------------------------------------------------------------ steps
def to_float(img):
    """imfrombytes(float32=True): ``astype(np.float32) / 255.``"""
    return img.astype(np.float32) / np.float32(255.0) if img.dtype == np.uint8 else np.asarray(img, np.float32)


def centre_pad(img, Hc, Wc):
    """pad_image: zeros around, top = (Hc - H) // 2, left = (Wc - W) // 2."""
    H, W = img.shape[:2]
    t, l = (Hc - H) // 2, (Wc - W) // 2
    return np.pad(img, ((t, Hc - H - t), (l, Wc - W - l)) + ((0, 0),) * (img.ndim - 2), mode="constant")


def edge_pad(img, Hp, Wp, mode):
    """Bottom / right pad: 'reflect101' = numpy 'reflect' (cv2.BORDER_REFLECT_101), 'symmetric' = numpy 'symmetric'
    (cv2.BORDER_REFLECT)."""
    H, W = img.shape[:2]
    if (Hp, Wp) == (H, W):
        return img
    return np.pad(img, ((0, Hp - H), (0, Wp - W)) + ((0, 0),) * (img.ndim - 2),
                  mode={"reflect101": "reflect", "symmetric": "symmetric"}[mode])


def dihedral(win, code):
    """[h, w, C] -> transpose?(flip_cols?(flip_rows?(win))); code = 4 transpose + 2 flip_rows + flip_cols."""
    if code & 2:
        win = np.flip(win, 0)
    if code & 1:
        win = np.flip(win, 1)
    if code & 4:
        win = win.transpose(1, 0, 2)
    return win


def add_noise(x, z, loc, scale, div=1.0):
    """float32(clip(float64(x) + (loc + scale * z / div), 0, 1))"""
    return np.clip(x.astype(np.float64) + (loc + scale * np.asarray(z, np.float64) / div), 0, 1).astype(np.float32)


def condition(c0, c1, n, thr):
    return max(int(c0), int(c1)) / n > thr


def counts(x):
    return int(np.sum(x == 0)), int(np.sum(x == 1))


def philox_normal(h, w, C, seed, call):
    """The kernel's normals in float64: element e = (i * w + j) * C + c, block e // 2, words (0, 1) for an even e and
    (2, 3) for an odd one; u1 = ((w0 >> 8) + 1) * 2^-24, u2 = (w1 >> 8) * 2^-24, z = sqrt(-2 ln u1) cos(2 pi u2)."""
    n = h * w * C
    words = po.philox_words(4 * ((n + 1) // 2), seed, call).reshape(-1, 2)[:n].astype(np.uint64)
    u1 = ((words[:, 0] >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24
    u2 = (words[:, 1] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    return (np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)).reshape(h, w, C)


def gpu_philox_draw(h, w, C, seed, call, loc, scale, x, extra_items=0):
    """GPU: [h, w, C] (as z is indexed) of clip(x + (loc + scale * z)) with the kernel's Philox normals over a constant
    fp32 source.  The probed item is item 0; ``extra_items`` small items after it shrink every item's grid."""
    import torch

    from rethink_acoustic_image_enhancement_amd import dataset
    src = torch.full((C, h, w), x, dtype=torch.float32, device="cuda:0")
    dst = torch.empty((C, h, w), device="cuda:0")
    items = [dict(src=src, dst=dst, noise=dict(loc=loc, scale=scale))]
    small = torch.zeros((1, 2, 2), device="cuda:0")
    items += [dict(src=small, dst=torch.empty((1, 2, 2), device="cuda:0")) for _ in range(extra_items)]
    dataset.sample_transform(items, seed=seed, call=call)
    return dst.cpu().numpy().transpose(1, 2, 0)


def gpu_philox_z(h, w, C, seed, call):
    """GPU: the kernel's fp32 normals themselves.  clip(0 + z / 8) is exact for z >= 0 (a power-of-two scale of an
    fp32 number below 8) and clip(0 - z / 8) for z < 0, so two launches on the same counter give every z exactly."""
    pos, neg = gpu_philox_draw(h, w, C, seed, call, 0.0, 0.125, 0.0), gpu_philox_draw(h, w, C, seed, call, 0.0, -0.125, 0.0)
    assert not np.any((pos > 0) & (neg > 0)) and pos.max() < 1 and neg.max() < 1
    return np.where(pos > 0, pos * np.float32(8), -neg * np.float32(8)).astype(np.float32)


def sample(src, canvas=None, padded=None, pad_mode="none", window=None, code=0, bgr2rgb=False, z=None, loc=0.0,
           scale=1.0, div=1.0, mean=None, std=None):
    """One item: ``src`` [Hs, Ws, C] (u8 or fp32) -> fp32 [C, h', w'].  ``z`` None: no noise."""
    x = to_float(src if src.ndim == 3 else src[:, :, None])
    Hc, Wc = canvas or x.shape[:2]
    Hp, Wp = padded or (Hc, Wc)
    x = edge_pad(centre_pad(x, Hc, Wc), Hp, Wp, pad_mode)
    t, l, h, w = window or (0, 0, Hp, Wp)
    win = x[t:t + h, l:l + w]
    assert win.shape[:2] == (h, w), "window leaves the canvas"
    if z is not None:
        win = add_noise(win, z, loc, scale, div)
    out = dihedral(win, code)
    if bgr2rgb:
        out = out[:, :, ::-1]
    out = np.ascontiguousarray(out.transpose(2, 0, 1))
    if mean is not None:
        out = out - np.asarray(mean, np.float32).reshape(-1, 1, 1)
    if std is not None:
        out = out / np.asarray(std, np.float32).reshape(-1, 1, 1)
    return out.astype(np.float32)


def finish(x, thr, nudge=1e-14, mean=None, std=None):
    """[C, H, W] of one sample: the nudge when max(count) / n > thr (one fp32 add), then the normalisation."""
    x = np.asarray(x, np.float32)
    if condition(*counts(x), x.size, thr):
        x = x + np.float32(nudge)
    if mean is not None:
        x = x - np.asarray(mean, np.float32).reshape(-1, 1, 1)
    if std is not None:
        x = x / np.asarray(std, np.float32).reshape(-1, 1, 1)
    return x.astype(np.float32)


# ------------------------------------------------------------------ lowering, the slow way (tests only)
def code_of(fn):
    """The dihedral code whose map equals ``fn`` on a non-square index image."""
    probe = np.arange(3 * 5).reshape(3, 5, 1)
    want = fn(probe)
    hits = [c for c in range(8) if dihedral(probe, c).shape == want.shape and np.array_equal(dihedral(probe, c), want)]
    assert len(hits) == 1, hits
    return hits[0]


def data_augmentation_model(img, mode):
    out = np.rot90(img, k=mode // 2)
    return np.flipud(out) if mode % 2 else out


def sync_augment_model(img, hflip, vflip, rot):
    """cv2.flip(img, 1) = np.flip(axis 1), cv2.flip(img, 0) = np.flip(axis 0), ROTATE_90_CLOCKWISE = np.rot90(k=-1),
    ROTATE_180 = k=2, ROTATE_90_COUNTERCLOCKWISE = k=1 (OpenCV's documented semantics)."""
    if hflip:
        img = np.flip(img, 1)
    if vflip:
        img = np.flip(img, 0)
    return img if rot is None else np.rot90(img, k={90: -1, 180: 2, 270: 1}[rot])


# ------------------------------------------------------------------ the two datasets, with the host generators as seeded
def teacher_sample(lq, gt, sr, rate, gt_size, geometric_augs=True, mean=None, std=None):
    """One ``__getitem__`` of the teacher's dataset on decoded u8 BGR [H, W, 3] images; draws as the reference.
    Returns (img, denoise_rate, hq, sr, draws)."""
    g = gt_size
    H, W = gt.shape[:2]
    Hp, Wp = max(H, g), max(W, g)
    top, left = random.randint(1, Hp - 1 - g), random.randint(1, Wp - 1 - g)
    z = sigma = None
    if np.random.uniform() < 0.1:
        sigma = np.random.uniform(1, 30)
        z = np.random.randn(g, g, 3)
    hflip = vflip = False
    rot = None
    if geometric_augs:
        hflip, vflip = random.random() < 0.5, random.random() < 0.5
        rot = random.choice([None, 90, 180, 270])
    code = code_of(lambda a: sync_augment_model(a, hflip, vflip, rot))
    mode = "reflect101" if (Hp, Wp) != (H, W) else "none"

    def one(src, s, z=None, **kw):
        return sample(src, padded=(Hp * s, Wp * s), pad_mode=mode, window=(top * s, left * s, g * s, g * s), code=code,
                      bgr2rgb=True, z=z, scale=sigma, div=255.0, **kw)
    img = finish(one(lq, 1, z), 0.10, 1e-14, mean, std)
    rate_plane = np.full((1, g, g), 1 if rate is None else rate, np.float64).astype(np.float32)
    return img, rate_plane, one(gt, 1, mean=mean, std=std), one(sr, 2, mean=mean, std=std), \
        (top, left, sigma, hflip, vflip, rot)


def train_rows(F, prob):
    if random.random() < 0.64:
        return [prob + 0.5 if random.random() > 0.64 else prob for _ in range(F)], False
    return [prob + 0.5 if f % 2 == 1 else prob for f in range(F)], True


def train_phase(stack, prob):
    """The train-phase mask rule on one item's planes [F, H, W] (fp32): host draws as the reference (`random` for
    the branches, one numpy mask per frame)."""
    F, H, W = stack.shape
    row, interp = train_rows(F, prob)
    keep = np.stack([po.numpy_keep(1, H, W, p)[0] for p in row])
    return po.mask_frames(stack[None], [min(max(p, 0.0), 1.0) for p in row], interp, keep[None])[0], row, interp


def student_sample(lq_frames, gt_frames, gt_size, prob, geometric_augs=True):
    """One ``__getitem__`` of the student's dataset (train phase) on lists of decoded grey u8 frames.
    `random` draws are made in the reference's order.  Returns (lq [F, g, g], gt, draws)."""
    g, F = gt_size, len(gt_frames)
    Hc, Wc = max(f.shape[0] for f in gt_frames), max(f.shape[1] for f in gt_frames)
    Hp, Wp = max(Hc, g), max(Wc, g)
    mode = "symmetric" if (Hp, Wp) != (Hc, Wc) else "none"
    top, left = random.randint(0, Hp - g), random.randint(0, Wp - g)

    def crop(frames):
        return np.concatenate([sample(f, canvas=(Hc, Wc), padded=(Hp, Wp), pad_mode=mode, window=(top, left, g, g))
                               for f in frames])
    lq, gt = crop(lq_frames), crop(gt_frames)
    lq, row, interp = train_phase(lq, prob)
    noisy = condition(*counts(lq), lq.size, 0.64)
    z = np.random.standard_normal((g, g, F)) if noisy else None
    aug = random.randint(0, 7) if geometric_augs else 0
    code = code_of(lambda a: data_augmentation_model(a, aug))
    lq = sample(lq.transpose(1, 2, 0), code=code, z=z, loc=0.3, scale=0.7)
    gt = sample(gt.transpose(1, 2, 0), code=code)
    return lq, gt, (top, left, row, interp, noisy, aug)


# ------------------------------------------------------------------ golden cases (tests/golden/make_golden_dataset.py)
def teacher_batch():
    """(py_seed, np_seed, gt_size, samples): two samples; np_seed is chosen so that sample 0 draws the noise."""
    samples = []
    for b, (H, W) in enumerate(((12, 14), (11, 10))):
        samples.append((hash_u8(f"teacher/{b}/lq", (H, W, 3), 0.2 if b else 0.0, 0.05), hash_u8(f"teacher/{b}/gt", (H, W, 3)),
                        hash_u8(f"teacher/{b}/sr", (2 * H, 2 * W, 3)), None if b else 0.75))
    return 41, 62, 8, samples


def student_batch():
    """(py_seed, np_seed, gt_size, prob, samples): two bursts of three frames of mixed sizes, the first needing the
    symmetric pad, the second mostly zeros (so that the noise condition holds)."""
    out = []
    for b, (sizes, zf) in enumerate(((((9, 12), (11, 10), (10, 12)), 0.0), (((16, 15), (16, 15), (14, 13)), 0.9))):
        out.append(([hash_u8(f"student/{b}/lq{f}", s, zf) for f, s in enumerate(sizes)],
                    [hash_u8(f"student/{b}/gt{f}", s) for f, s in enumerate(sizes)]))
    return 43, 44, 12, 0.05, out


def train_cases():
    """name -> (prob, py_seed, np_seed, frames [B, F, H, W]) for the train-phase rule."""
    out = {}
    for F, (H, W), prob in ((1, (4, 5), 0.3), (3, (8, 8), 0.3), (7, (4, 5), 0.3), (3, (4, 5), 0.6), (5, (8, 8), 0.0)):
        name = f"train_f{F}_{H}x{W}_p{prob}"
        out[name] = (prob, 300 + len(out), 400 + len(out), po._img(name, (4, F, H, W)))
    return out
