"""``kdlae_train_prepare`` / ``kdlae_train_mask_frames`` (csrc/augment.hip) and the Python surface of
rethink_acoustic_image_enhancement_amd.augment against the numpy oracle (tests/prepare_oracle.py) and the
reference-recorded goldens (tests/golden/prepare_train.*).

Every comparison is bit for bit: the kernels copy and select, and the one add and one multiply of the
interpolating frame rule are fp32 on both sides.  Every launch writes into an interior slice of a buffer filled
with 1e30 and reads from one, at each float offset 0..3 (offset 0 takes the 16-byte store path where the row
length allows it, 1..3 the element path), and every sentinel must survive."""
import functools
import itertools
import json
import os
import random

import numpy as np
import pytest
import torch

from rethink_acoustic_image_enhancement_amd import augment
from rethink_acoustic_image_enhancement_amd.hashweights import hash_images, load_hash_weights
from tests import prepare_oracle as po

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = np.float32(1e30)
PAD = 8   # sentinel floats on each side of an embedded tensor (before adding the offset)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
META = json.load(open(os.path.join(GOLDEN, "prepare_train.json")))
ARRAYS = np.load(os.path.join(GOLDEN, "prepare_train.npz"))
P_CASES = po.progressive_cases()
F_CASES = po.frame_cases()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def embed(arr_or_shape, off):
    """A 1e30-filled device buffer and the contiguous view of it that starts ``off`` floats past a 16-byte
    boundary, holding ``arr`` (or left at 1e30 when only a shape is given)."""
    shape = arr_or_shape if isinstance(arr_or_shape, tuple) else arr_or_shape.shape
    n = int(np.prod(shape))
    host = np.full(n + 2 * PAD + 4, SENTINEL, np.float32)
    if not isinstance(arr_or_shape, tuple):
        host[PAD + off:PAD + off + n] = np.asarray(arr_or_shape, np.float32).reshape(-1)
    buf = torch.from_numpy(host).to(DEV)
    view = buf[PAD + off:PAD + off + n].view(shape)
    assert view.data_ptr() % 16 == 4 * off and view.is_contiguous()
    return buf, view, host


def check_embedded(buf, off, want, what):
    got = buf.cpu().numpy()
    n = want.size
    inner = got[PAD + off:PAD + off + n].reshape(want.shape)
    assert np.array_equal(bits(inner), bits(want)), what
    assert np.all(got[:PAD + off] == SENTINEL) and np.all(got[PAD + off + n:] == SENTINEL), f"{what}: sentinel overwritten"
    return got


@functools.lru_cache(maxsize=None)
def sources(C):
    """The 12 x 12 batch of three images (img / hq), its one-channel rate map and the 24 x 24 sr."""
    return (hash_images(f"prepare_gpu/img{C}", (3, C, 12, 12)), hash_images("prepare_gpu/rate", (3, 1, 12, 12)),
            hash_images(f"prepare_gpu/hq{C}", (3, C, 12, 12)), hash_images(f"prepare_gpu/sr{C}", (3, C, 24, 24)))


def geometries():
    """Every window of the list that fits a 12 x 12 source (h or w = 12 only at offset 0: the uncropped case)."""
    for w, h, x0, y0 in itertools.product((4, 5, 8, 12), (1, 5, 12), (0, 1, 3), (0, 2)):
        if x0 + w <= 12 and y0 + h <= 12:
            yield w, h, x0, y0


PROBS = (0.0, 0.3, 1.0, 1.7)


def run_prepare(specs, index, B, seed, call, off, what):
    """specs: (src array, scale, y0, x0, h, w, prob, keep | None) per segment; off: the float offset of every dst,
    or one per segment.  Launches twice into fresh embedded buffers, compares both with the oracle and the
    sources with themselves."""
    idx = torch.tensor(index, dtype=torch.int32, device=DEV) if index is not None else None
    offs = [off] * len(specs) if isinstance(off, int) else list(off)
    srcs = [embed(s[0], (o + 1 + i) % 4) for i, (s, o) in enumerate(zip(specs, offs))]
    first = None
    for rep in range(2):
        dsts, segs = [], []
        for (src, sc, y0, x0, h, w, prob, keep), (_, sview, _), o in zip(specs, srcs, offs):
            d = embed((B, src.shape[1], h * sc, w * sc), o)
            dsts.append(d)
            k = torch.from_numpy(keep).to(DEV) if keep is not None else None
            segs.append(dict(src=sview, dst=d[1], y0=y0 * sc, x0=x0 * sc, prob=prob, keep=k))
        augment.train_prepare(segs, idx, B, 0.1, seed, call)
        outs = []
        for s, ((src, sc, y0, x0, h, w, prob, keep), d) in enumerate(zip(specs, dsts)):
            want = po.prepare(src, index, y0 * sc, x0 * sc, h * sc, w * sc, prob, keep, 0.1, seed, call + s)
            outs.append(check_embedded(d[0], offs[s], want, f"{what} segment {s} run {rep}"))
        if first is None:
            first = outs
        else:
            assert all(a.tobytes() == b.tobytes() for a, b in zip(first, outs)), f"{what}: two runs differ"
    for (sbuf, _, shost) in srcs:
        assert sbuf.cpu().numpy().tobytes() == shost.tobytes(), f"{what}: src was written"


@pytest.mark.parametrize("index", [None, [2, 0]], ids=["identity", "gather"])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("route", ["keep", "philox"])
def test_one_segment_every_window_offset_and_probability(index, C, route):
    """The whole grid: every window that fits x every dst offset x every probability."""
    img = sources(C)[0]
    B = 3 if index is None else 2
    for n, (w, h, x0, y0) in enumerate(geometries()):
        keep = po.philox_keep((B, C, h, w), 0.35, 77, n) if route == "keep" else None
        for off, prob in itertools.product(range(4), PROBS):
            run_prepare([(img, 1, y0, x0, h, w, prob, keep)], index, B, 1234 + n, 5 * n, off,
                        f"{route} C{C} w{w} h{h} x{x0} y{y0} off{off} p{prob}")


@pytest.mark.parametrize("index", [None, [2, 0]], ids=["identity", "gather"])
@pytest.mark.parametrize("route", ["keep", "philox"])
def test_four_segments_one_launch_only_img_is_masked(index, route):
    """img, denoise_rate, hq and the 24 x 24 sr at doubled offsets in one launch; with Philox each segment has its
    own call number, and a probability on img never touches the other three."""
    C = 3
    img, rate, hq, sr = sources(C)
    B = 3 if index is None else 2
    for n, (w, h, x0, y0) in enumerate(geometries()):
        off, prob = n % 4, PROBS[(n // 4) % 4]
        keep = po.philox_keep((B, C, h, w), 0.35, 78, n) if route == "keep" else None
        specs = [(img, 1, y0, x0, h, w, prob, keep), (rate, 1, y0, x0, h, w, 0.0, None),
                 (hq, 1, y0, x0, h, w, 0.0, None), (sr, 2, y0, x0, h, w, 0.0, None)]
        run_prepare(specs, index, B, 99, 8 * n, off, f"4seg {route} w{w} h{h} x{x0} y{y0} off{off} p{prob}")
    # unmasked segments equal the plain crop whatever the call number
    for s, src, sc in ((1, rate, 1), (2, hq, 1), (3, sr, 2)):
        a = po.prepare(src, index, 2 * sc, 3 * sc, 8 * sc, 8 * sc, 0.0, None, 0.1, 99, s)
        assert np.array_equal(a, (src if index is None else src[index])[:, :, 2 * sc:10 * sc, 3 * sc:11 * sc])


@pytest.mark.parametrize("index", [None, [2, 0]], ids=["identity", "gather"])
@pytest.mark.parametrize("route", ["keep", "philox"])
def test_one_launch_mixes_vector_and_element_segments(index, route):
    """Segments of one launch on different store paths, in every order: the unit count of a vector segment is
    n / 4 and of an element segment n, and a unit must find its segment across both kinds.  Each segment has its
    own window; widths 8 and 4 at dst offset 0 are vector segments, width 5 or a dst offset of 1..3 is not."""
    C = 3
    img, rate, hq, sr = sources(C)
    B = 3 if index is None else 2
    # (src, scale, y0, x0, h, w, dst offset, vector?)
    vec_img, vec_sr = (img, 1, 2, 3, 5, 8, 0, True), (sr, 2, 1, 1, 5, 4, 0, True)
    el_rate, el_hq, el_img = (rate, 1, 0, 1, 12, 5, 0, False), (hq, 1, 2, 0, 1, 8, 2, False), (img, 1, 0, 3, 5, 4, 3, False)
    layouts = [(vec_img, el_rate, el_hq, vec_sr), (el_img, vec_sr, el_rate, vec_img), (vec_sr, el_hq),
               (el_rate, vec_img), (vec_img, vec_sr, el_hq), (el_hq, el_rate, vec_img)]
    for n, layout in enumerate(layouts):
        assert {g[7] for g in layout} == {True, False}
        for g in layout:
            assert g[7] == ((g[5] * g[1]) % 4 == 0 and g[6] == 0)
        for prob in PROBS:
            specs = []
            for i, (src, sc, y0, x0, h, w, _, _) in enumerate(layout):
                p = prob if i == 0 else 0.0
                keep = po.philox_keep((B, src.shape[1], h * sc, w * sc), 0.35, 79, n) if route == "keep" and i == 0 else None
                specs.append((src, sc, y0, x0, h, w, p, keep))
            run_prepare(specs, index, B, 555, 16 * n, [g[6] for g in layout], f"mixed {route} layout {n} p{prob}")


def _philox_segment(prob, seed, call, off=0):
    src = hash_images("prepare_gpu/philox64", (2, 3, 64, 64))
    _, sview, _ = embed(src, 0)
    buf, dview, _ = embed((2, 3, 64, 64), off)
    augment.train_prepare([dict(src=sview, dst=dview, prob=prob)], None, 2, 0.1, seed, call)
    want = po.prepare(src, None, 0, 0, 64, 64, prob, None, 0.1, seed, call)
    check_embedded(buf, off, want, f"philox 2x3x64x64 off{off}")
    return want != src


def test_philox_segment_matches_host_model_and_masks_the_expected_fraction():
    p, N = 0.2, 2 * 3 * 64 * 64
    bound = 5 * np.sqrt(p * (1 - p) / N)
    masks = []
    for seed, call in ((0, 0), (20250821, 8), (20250821, 9), (2 ** 63 + 5, 2 ** 40 + 3)):
        host = po.philox_keep((2, 3, 64, 64), p, seed, call) == 0       # the host model alone meets the bound
        assert abs(host.mean() - p) <= bound, (seed, call, host.mean())
        for off in ((0, 1) if call == 8 else (0,)):
            masked = _philox_segment(p, seed, call, off)
            assert np.array_equal(masked, host)
            frac = masked.mean()
            print(f"seed {seed} call {call}: masked fraction {frac:.5f}, p {p}, bound {bound:.5f}")
            assert abs(frac - p) <= bound
        masks.append(host)
    assert not np.array_equal(masks[1], masks[2])                        # call and call + 1 differ
    assert abs((masks[1] & masks[2]).mean() - p * p) <= 5 * np.sqrt(p * p * (1 - p * p) / N)


def test_philox_known_answer_in_the_kernel():
    """Counter 0, key 0 is elements 0..3 of a segment with seed 0, call 0.  Element k is kept at prob = u_k and
    masked at the next float above, which pins the upper 24 bits of each word of the known answer (the keep rule
    uses no more of a word: u = (word >> 8) * 2^-24).

    The other two known answers are held on the host model only (tests/test_prepare.py): their counters have
    q = 2^64 - 1 and q = 0x85a308d3243f6a88, and the kernel forms q = e / 4 from a non-negative signed 64-bit
    element index, so no q >= 2^61 can be reached through the ABI.  The kernel is tied to that host model bit for
    bit instead, high key and call words included (seed 2^63 + 5, call 2^40 + 3 in the test above)."""
    words = (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)
    src = np.array([0.5, 0.25, 0.75, 0.125], np.float32).reshape(1, 1, 1, 4)
    for off in (0, 1):
        _, sview, _ = embed(src, 0)
        for k, word in enumerate(words):
            u = np.float32(word >> 8) * np.float32(2.0 ** -24)
            for prob, kept in ((u, True), (np.nextafter(u, np.float32(2)), False)):
                buf, dview, _ = embed((1, 1, 1, 4), off)
                augment.train_prepare([dict(src=sview, dst=dview, prob=float(prob))], None, 1, 0.1, 0, 0)
                got = dview.cpu().numpy().reshape(-1)
                assert (got[k] == src.reshape(-1)[k]) == kept and (got[k] == np.float32(-0.1)) == (not kept), (k, prob)
                check_embedded(buf, off, po.prepare(src, None, 0, 0, 1, 4, float(prob), None, 0.1, 0, 0), "kat")


# ------------------------------------------------------------------ kdlae_train_mask_frames
def run_frames(frames, probs, interpolate, keep, seed, call, off, want, what):
    sbuf, sview, shost = embed(frames, (off + 2) % 4)
    k = torch.from_numpy(np.ascontiguousarray(keep)).to(DEV) if keep is not None else None
    first = None
    for rep in range(2):
        buf, dview, _ = embed(frames.shape, off)
        out = augment.mask_frames(sview, probs, interpolate, k, seed, call, 0.1, out=dview)
        assert out is dview
        got = check_embedded(buf, off, want, f"{what} off{off} run {rep}")
        assert first is None or first.tobytes() == got.tobytes()
        first = got
    assert sbuf.cpu().numpy().tobytes() == shost.tobytes(), f"{what}: src was written"


@pytest.mark.parametrize("name", sorted(F_CASES))
def test_mask_frames_reproduces_the_reference_with_its_keep_masks(name):
    phase, prob, _, _, frames = F_CASES[name]
    keep, want = ARRAYS[f"frames/{name}/keep"], ARRAYS[f"frames/{name}/out"]
    rows = [[min(float(p), 1.0) for p in row] for row in META["frames"][name]["probs"]]
    for off in range(4):
        if all(r == rows[0] for r in rows):
            run_frames(frames, rows[0], phase == "interpolation", keep, 0, 0, off, want, name)
        for b, row in enumerate(rows):
            run_frames(frames[b:b + 1], row, phase == "interpolation", keep[b:b + 1], 0, 0, off, want[b:b + 1],
                       f"{name}[{b}]")


@pytest.mark.parametrize("F", [1, 3, 7])
@pytest.mark.parametrize("hw", [(4, 5), (8, 8)], ids=["4x5", "8x8"])
@pytest.mark.parametrize("interpolate", [False, True])
def test_mask_frames_philox_matches_host_model(F, hw, interpolate):
    frames = hash_images(f"prepare_gpu/frames{F}", (2, F) + hw)
    for n, probs in enumerate(([0.3 if f % 2 == 0 else 0.8 for f in range(F)], [0.0, 0.5, 1.0, 1.7, 0.2, 0.9, 0.4][:F])):
        for off in range(4):
            seed, call = 4242 + n, 3 * off + n
            want = po.mask_frames(frames, probs, interpolate, None, 0.1, seed, call)
            run_frames(frames, probs, interpolate, None, seed, call, off, want, f"philox F{F} {hw} i{interpolate}")


def test_interpolation_helpers_follow_the_reference_draws():
    for name in ("interpolation_f7_8x8", "test1_f7_8x8", "test1_clamped_f3_8x8", "test1_prob0_f3_4x5"):
        phase, prob, py_seed, np_seed, frames = F_CASES[name]
        random.seed(py_seed)
        np.random.seed(np_seed)
        fn = augment.interpolation_inputs if phase == "interpolation" else augment.test1_inputs
        x = torch.from_numpy(frames).to(DEV)
        out = fn(x, prob, rng="numpy")
        assert np.array_equal(bits(out.cpu().numpy()), bits(ARRAYS[f"frames/{name}/out"])), name
        assert np.array_equal(bits(x.cpu().numpy()), bits(frames))
        # Philox route: reproducible (test1's branch draws included), and a different call draws a different mask
        outs = []
        for call in (4, 4, 40):
            random.seed(py_seed)
            outs.append(fn(x, 0.3, seed=1, call=call))
        assert torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], outs[2])
        # the call rule does not depend on the draws: interpolation is one launch with `call`, test1 one launch per
        # item with call + b, also when every item happens to draw the same branches
        if phase == "interpolation":
            want = po.mask_frames(frames, [0.3 if f % 2 == 0 else 0.8 for f in range(frames.shape[1])], True, None, 0.1, 1, 4)
        else:
            random.seed(py_seed)
            rows = [[0.3 + 0.6 if random.random() < 0.2 else 0.3 for _ in range(frames.shape[1])] for _ in frames]
            want = np.concatenate([po.mask_frames(frames[b:b + 1], [min(p, 1.0) for p in rows[b]], False, None, 0.1, 1, 4 + b)
                                   for b in range(frames.shape[0])])
        assert np.array_equal(bits(outs[0].cpu().numpy()), bits(want)), name
    # test1 where every item draws the same branches (a seed without a draw below 0.2): still call + b per item
    frames = F_CASES["test1_f3_8x8"][4]

    def draws(seed):
        random.seed(seed)
        return [[0.9 if random.random() < 0.2 else 0.3 for _ in range(3)] for _ in range(2)]

    seed = next(s for s in range(1000) if draws(s) == [[0.3] * 3] * 2)
    random.seed(seed)
    a = augment.test1_inputs(torch.from_numpy(frames).to(DEV), 0.3, seed=1, call=4).cpu().numpy()
    for b in range(2):
        assert np.array_equal(bits(a[b:b + 1]), bits(po.mask_frames(frames[b:b + 1], [0.3] * 3, False, None, 0.1, 1, 4 + b)))
    assert not np.array_equal(bits(a), bits(po.mask_frames(frames, [0.3] * 3, False, None, 0.1, 1, 4)))


# ------------------------------------------------------------------ ProgressiveBatcher
def _to_dev(v):
    return {k: torch.from_numpy(a).to(DEV) for k, a in v.items()} if isinstance(v, dict) else torch.from_numpy(v).to(DEV)


def _schedule(cfg):
    return augment.ProgressiveSchedule(cfg["iters"], cfg["gt_sizes"], cfg["mini_batch_sizes"], cfg["probs"],
                                       cfg["gt_size"], cfg["batch_size"], prob=cfg["prob"], scale=cfg["scale"])


def _items(v):
    return v.items() if isinstance(v, dict) else [(None, v)]


@pytest.mark.parametrize("name", sorted(P_CASES))
def test_batcher_numpy_route_reproduces_the_reference_batch_and_draws(name):
    cfg, it, py_seed, np_seed, lq, gt = P_CASES[name]
    d = META["progressive"][name]["draws"]
    batcher = augment.ProgressiveBatcher(_schedule(cfg), rng="numpy")
    dlq, dgt = _to_dev(lq), _to_dev(gt)
    random.seed(py_seed)
    np.random.seed(np_seed)
    before = random.getstate()
    o_lq, o_gt = batcher(it, dlq, dgt)
    j, indices, x0, y0, mp = batcher.last_draw
    assert (j, indices, x0, y0, repr(float(mp))) == (d["stage"], d["indices"], d["x0"], d["y0"], d["mask_prob"])
    if name in ("dict_full", "tensor_full"):     # nothing to sample and nothing to crop: no `random` call at all
        assert cfg["mini_batch_sizes"][j] == cfg["batch_size"] and cfg["gt_sizes"][j] == cfg["gt_size"]
        assert random.getstate() == before
    assert isinstance(o_lq, dict) == isinstance(lq, dict) and isinstance(o_gt, dict) == isinstance(gt, dict)
    for tag, got, src in (("out_lq", o_lq, lq), ("out_gt", o_gt, gt)):
        assert (set(got) == set(src)) if isinstance(src, dict) else True
        for k, t in _items(got):
            want = ARRAYS[f"progressive/{name}/{tag}" + (f"/{k}" if k else "")]
            assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
            assert t.shape == want.shape and np.array_equal(bits(t.cpu().numpy()), bits(want)), (name, tag, k)
    # new tensors; the inputs keep their bits
    for dv, hv in ((dlq, lq), (dgt, gt)):
        for k, t in _items(dv):
            assert np.array_equal(bits(t.cpu().numpy()), bits(hv[k] if k else hv))
    for (k, t), (_, s) in zip(list(_items(o_lq)) + list(_items(o_gt)), list(_items(dlq)) + list(_items(dgt))):
        assert t.data_ptr() != s.data_ptr()


def test_batcher_philox_route_is_reproducible_and_masks_only_img():
    cfg, it, py_seed, _, lq, gt = P_CASES["dict_sub_crop_mask"]
    dlq, dgt = _to_dev(lq), _to_dev(gt)
    outs = []
    for seed, cur in ((7, it), (7, it), (8, it), (7, it - 1)):    # it - 1 is in the same stage
        random.seed(py_seed)
        b = augment.ProgressiveBatcher(_schedule(cfg), rng="philox", seed=seed)
        st = np.random.get_state()[1].copy()
        outs.append(b(cur, dlq, dgt))
        assert np.array_equal(np.random.get_state()[1], st)       # nothing drawn from numpy on the host
        j, indices, x0, y0, mp = b.last_draw
        want_img = po.prepare(lq["img"], indices, x0, y0, 8, 8, mp, None, 0.1, seed, cur * 8)
        assert np.array_equal(bits(outs[-1][0]["img"].cpu().numpy()), bits(want_img))
        for k, src, sc in (("denoise_rate", lq["denoise_rate"], 1), ("hq", gt["hq"], 1), ("sr", gt["sr"], 2)):
            got = (outs[-1][0] if k == "denoise_rate" else outs[-1][1])[k].cpu().numpy()
            assert np.array_equal(bits(got), bits(po.prepare(src, indices, x0 * sc, y0 * sc, 8 * sc, 8 * sc)))
    assert torch.equal(outs[0][0]["img"], outs[1][0]["img"])
    assert not torch.equal(outs[0][0]["img"], outs[2][0]["img"]) and not torch.equal(outs[0][0]["img"], outs[3][0]["img"])


def test_batcher_refuses_a_batch_that_does_not_fit_the_schedule():
    cfg, it, _, _, lq, gt = P_CASES["tensor_sub_crop_mask"]
    b = augment.ProgressiveBatcher(_schedule(cfg))
    random.seed(1)
    state = random.getstate()
    with pytest.raises(ValueError, match="batch_size"):
        b(it, _to_dev(lq[:3]), _to_dev(gt[:3]))
    # a gt (or rate, hq, sr) with fewer images than lq: the drawn indices would reach past its end
    with pytest.raises(ValueError, match="gt holds 3"):
        b(it, _to_dev(lq), _to_dev(gt[:3]))
    dcfg, dit, _, _, dlq, dgt = P_CASES["dict_sub_crop_mask"]
    db = augment.ProgressiveBatcher(_schedule(dcfg))
    for key in ("denoise_rate", "hq", "sr"):
        bad_lq = {k: v[:3] if k == key else v for k, v in dlq.items()}
        bad_gt = {k: v[:3] if k == key else v for k, v in dgt.items()}
        with pytest.raises(ValueError, match=f"{key}.* holds 3"):
            db(dit, _to_dev(bad_lq), _to_dev(bad_gt))
    with pytest.raises(ValueError, match="leaves"):               # an 8 x 8 window at gt_size 12 offsets in a 6 x 6 tensor
        b(it, _to_dev(np.ascontiguousarray(lq[:, :, :6, :6])), _to_dev(gt))
    with pytest.raises(ValueError, match="leaves gt"):
        b(it, _to_dev(lq), _to_dev(np.ascontiguousarray(gt[:, :, :, :10])))
    with pytest.raises(RuntimeError, match="contiguous"):
        b(it, _to_dev(lq).transpose(2, 3), _to_dev(gt))
    with pytest.raises(RuntimeError, match="contiguous"):
        b(it, _to_dev(lq), _to_dev(gt).transpose(2, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        b(it, _to_dev(lq), torch.from_numpy(gt))
    assert random.getstate() == state                             # every refusal came before the first draw
    # the low-level call checks a host index against every source and says so; nothing is launched
    src3, src2 = _to_dev(lq[:3]), _to_dev(gt[:2])
    dst = [torch.empty((2, 3, 12, 12), device=DEV) for _ in range(2)]
    for bad in ([0, 2], [-1, 0], [0, 3]):
        with pytest.raises(IndexError, match="out of range"):
            augment.train_prepare([dict(src=src3, dst=dst[0]), dict(src=src2, dst=dst[1])], bad)
    with pytest.raises(ValueError, match="entries"):
        augment.train_prepare([dict(src=src3, dst=dst[0])], [0, 1, 2])
    augment.train_prepare([dict(src=src3, dst=dst[0]), dict(src=src2, dst=dst[1])], [1, 0])
    assert torch.equal(dst[0], src3[[1, 0]]) and torch.equal(dst[1], src2[[1, 0]])


# ------------------------------------------------------------------ trainer integration
def test_trainer_step_on_a_prepared_batch_equals_the_step_on_the_oracle_batch():
    from rethink_acoustic_image_enhancement_amd.KDLAE_model import KDLAE_teacher
    from rethink_acoustic_image_enhancement_amd.train import KDLAETrainer

    name = "dict_trainer_step"                     # 6 -> 2 images, 32^2 -> 16^2, p = 0.2
    cfg, it, py_seed, np_seed, lq, gt = P_CASES[name]

    def trainer():
        m = KDLAE_teacher(dim=16, num_blocks=[1, 1, 1, 1], num_refinement_blocks=1, LayerNorm_type="BiasFree")
        load_hash_weights(m)
        return KDLAETrainer(m.to(DEV), lr=1e-3)

    random.seed(py_seed)
    np.random.seed(np_seed)
    want_lq, want_gt, _ = po.progressive(cfg, it, lq, gt)
    assert want_lq["img"].shape == (2, 3, 16, 16) and want_gt["sr"].shape == (2, 3, 32, 32)
    tr_o = trainer()
    loss_o = tr_o.optimize_parameters(_to_dev(want_lq), _to_dev(want_gt))

    batcher = augment.ProgressiveBatcher(_schedule(cfg), rng="numpy")
    random.seed(py_seed)
    np.random.seed(np_seed)
    tr = trainer()
    loss = tr.optimize_parameters(*batcher(it, _to_dev(lq), _to_dev(gt)))
    torch.cuda.synchronize()
    a, b = np.float32(float(loss)), np.float32(float(loss_o))
    print(f"loss {a!r} (prepared on the GPU) vs {b!r} (oracle batch)")
    assert np.isfinite(a) and a.view(np.uint32) == b.view(np.uint32)
    assert torch.equal(tr.theta, tr_o.theta)
