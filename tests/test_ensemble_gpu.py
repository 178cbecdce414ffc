"""Self-ensemble on the GPU: kdlae_ens_gather / kdlae_ens_merge against the numpy model (tests/ensemble_model.py),
forward_ensemble of the three modules against the hand-written torch loop, pipeline.enhance_ensemble_u8,
validate(ensemble=) and the caller's-stream contract of the two entries.

The kernels copy, add in a fixed order and divide, and batch rows of the forwards are bit for bit independent of the
batch size (test_kdlae_gpu.test_batch_invariance_and_determinism), so every comparison here is on the bits: no
tolerance anywhere in this file.  The host loop divides by 8, 4 or 1 only (torch divides by a host scalar through its
reciprocal, which is the same rounding for a power of two and no other divisor)."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from rethink_acoustic_image_enhancement_amd import _lib, ensemble
from rethink_acoustic_image_enhancement_amd.hashweights import hash_images, load_hash_weights
from rethink_acoustic_image_enhancement_amd.KDLAE_model import KDLAE_student, KDLAE_teacher, Restormer
from rethink_acoustic_image_enhancement_amd.metrics import psnr_batch
from rethink_acoustic_image_enhancement_amd.pipeline import enhance_ensemble_u8, postprocess_u8, preprocess_u8
from rethink_acoustic_image_enhancement_amd.train import KDLAETrainer, RestormerTrainer
from tests import ensemble_model as em
from tests.stream_harness import check_async_and_order, check_capture
from tests.test_caller_stream_gpu import Simple, _f
from tests.workspace_harness import stream, vp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BIG = 1e30
G = 64   # guard floats (256 bytes) either side of a buffer under test

SHAPES = [(1, 1), (1, 7), (5, 3), (31, 33), (32, 32), (33, 65), (8, 40), (64, 36)]
MASKS = [1 << m for m in em.MODES] + [em.mask_of("d8"), em.mask_of("flips"), em.mask_of((2, 5, 7))]
# (source offset, destination offset) in floats from a 16-byte boundary; (0, 0) with W % 4 == 0 is the float4
# path, everything else the scalar one
OFFSETS = [(0, 0), (1, 1), (2, 2), (3, 3), (0, 2), (3, 0)]


def _c(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _stored(values, off):
    """`values` (numpy) inside BIG-filled device storage at float offset `off` from a 16-byte boundary ->
    (storage, view of the values)."""
    n = values.size
    store = torch.full((G + off + n + G,), BIG, device=DEV)
    assert store.data_ptr() % 16 == 0
    view = store[G + off:G + off + n]
    view.copy_(torch.from_numpy(np.ascontiguousarray(values).reshape(-1)))
    return store, view


def _expect_store(values, off):
    exp = torch.full((G + off + values.size + G,), BIG)
    exp[G + off:G + off + values.size] = torch.from_numpy(np.ascontiguousarray(values).reshape(-1))
    return exp.to(DEV)


def _twice(entry, src_view, n_out, do, N, C, H, W, mask):
    """Two calls into BIG-filled storage at destination offset `do` -> the storage (equal bits asserted)."""
    got = []
    for _ in range(2):
        dst_store = torch.full((G + do + n_out + G,), BIG, device=DEV)
        rc = getattr(_lib.lib(), entry)(_c(src_view), _c(dst_store[G + do:]), N, C, H, W, mask, None)
        assert rc == 0, _lib.last_error()
        got.append(dst_store)
    assert _same_bits(got[0], got[1])
    return got[0]


def _values(key, shape):
    return hash_images(key, shape, -1.0, 1.0)


# ------------------------------------------------------------------ the kernels through the C entries
@pytest.mark.parametrize("hw", SHAPES)
@pytest.mark.parametrize("C", [1, 3])
def test_gather_equals_the_model(C, hw):
    N, (H, W) = 2, hw
    x = _values(f"ens:g:{C}:{H}x{W}", (N, C, H, W))
    for so, do in OFFSETS:
        src_store, src = _stored(x, so)
        src0 = src_store.clone()
        for mask in MASKS:
            want = em.gather(x, mask)
            got = _twice("kdlae_ens_gather", src, want.size, do, N, C, H, W, mask)
            assert _same_bits(got, _expect_store(want, do)), (mask, so, do)
        assert _same_bits(src_store, src0)


@pytest.mark.parametrize("hw", SHAPES)
@pytest.mark.parametrize("C", [1, 3])
def test_merge_equals_the_model(C, hw):
    N, (H, W) = 2, hw
    for mask in MASKS:
        k = len(em.modes_of(mask))
        staged = _values(f"ens:m:{C}:{H}x{W}:{mask}", (k * N * C * H * W,))
        want = em.merge(staged, N, C, H, W, mask)
        for so, do in OFFSETS:
            src_store, src = _stored(staged, so)
            src0 = src_store.clone()
            got = _twice("kdlae_ens_merge", src, want.size, do, N, C, H, W, mask)
            assert _same_bits(got, _expect_store(want, do)), (mask, so, do)
            assert _same_bits(src_store, src0)


@pytest.mark.parametrize("hw", [(1100, 1001), (1001, 1100)])
def test_past_the_block_cap(hw):
    """35 x 32 = 1120 tiles of 32 x 32 are more than the 1024 blocks a launch gets: the grid-stride loop takes
    the rest.  1001 columns is the scalar path, 1100 the float4 one."""
    H, W = hw
    mask = em.mask_of("d8")
    x = _values(f"ens:cap:{H}x{W}", (1, 1, H, W))
    want = em.gather(x, mask)
    _, src = _stored(x, 0)
    got = _twice("kdlae_ens_gather", src, want.size, 0, 1, 1, H, W, mask)
    assert _same_bits(got, _expect_store(want, 0))
    # merging the views of one image: eight equal terms per pixel, in the model's arithmetic
    merged = em.merge(want, 1, 1, H, W, mask)
    got = _twice("kdlae_ens_merge", got[G:G + want.size], x.size, 0, 1, 1, H, W, mask)
    assert _same_bits(got, _expect_store(merged, 0))


@pytest.mark.parametrize("hw", [(3, 5), (32, 36)])
def test_planted_sum_order_comes_out_with_the_models_bits(hw):
    H, W = hw
    mask, staged = em.planted_sum_order(1, 2, H, W)
    want = em.merge(staged, 1, 2, H, W, mask)
    assert np.all(want == 0) and np.all(em.merge(staged, 1, 2, H, W, mask, order="descending") != 0)
    for off in (0, 1):
        _, src = _stored(staged, off)
        got = _twice("kdlae_ens_merge", src, want.size, off, 1, 2, H, W, mask)
        assert _same_bits(got, _expect_store(want, off))
    # a mask of three divides by 3, in fp32, once
    x = _values(f"ens:div3:{H}x{W}", (1, 2, H, W))
    m3 = em.mask_of((0, 1, 5))
    buf = em.gather(x, m3)
    _, src = _stored(buf, 0)
    got = _twice("kdlae_ens_merge", src, x.size, 0, 1, 2, H, W, m3)
    assert _same_bits(got, _expect_store(em.merge(buf, 1, 2, H, W, m3), 0))


def test_argument_refusals_launch_nothing():
    L = _lib.lib()
    N, C, H, W = 2, 3, 8, 12
    src = torch.from_numpy(_values("ens:refuse", (8 * N * C * H * W,))).to(DEV)
    for name in _lib.ENSEMBLE_EXPORTS:
        dst = torch.full((8 * N * C * H * W,), BIG, device=DEV)
        s, d = src.data_ptr(), dst.data_ptr()
        for args in ((None, d, N, C, H, W, 255), (s, None, N, C, H, W, 255), (s, d, 0, C, H, W, 255),
                     (s, d, N, 0, H, W, 255), (s, d, N, C, 0, W, 255), (s, d, N, C, H, -3, 255),
                     (s, d, N, C, H, W, 0), (s, d, N, C, H, W, 256), (s, d, N, C, H, W, -1)):
            rc = getattr(L, name)(*args, None)
            assert rc == 1 and name in _lib.last_error(), (name, args, rc)
        torch.cuda.synchronize()
        assert bool((dst == BIG).all()), name


def test_wrappers():
    N, C, H, W = 2, 3, 24, 40
    x = _values("ens:wrap", (N, C, H, W))
    xd = torch.from_numpy(x).to(DEV)
    for modes in ("d8", "flips", (2, 5, 7), [0]):
        mask = em.mask_of(modes)
        buf = ensemble.ens_gather(xd, modes)
        assert buf.shape == (len(em.modes_of(mask)) * x.size,)
        assert np.array_equal(buf.cpu().numpy(), em.gather(x, mask))
        for v, w in zip(ensemble.ens_views(buf, N, C, H, W, modes), em.views(em.gather(x, mask), N, C, H, W, mask)):
            assert v.shape == w.shape and np.array_equal(v.cpu().numpy(), w)
        out = ensemble.ens_merge(buf, N, H, W, modes)
        assert out.shape == (N, C, H, W)
        assert np.array_equal(out.cpu().numpy().view(np.int32), em.merge(em.gather(x, mask), N, C, H, W, mask)
                              .view(np.int32))
    # a non-contiguous source is gathered as its values; out= is written in place
    xt = xd.transpose(-1, -2)
    assert np.array_equal(ensemble.ens_gather(xt, (3,)).cpu().numpy(),
                          em.gather(np.ascontiguousarray(x.swapaxes(-1, -2)), 1 << 3))
    out = torch.empty(x.size, device=DEV)
    assert ensemble.ens_gather(xd, (6,), out=out) is out
    with pytest.raises(RuntimeError, match="out must be"):
        ensemble.ens_gather(xd, "d8", out=out)
    with pytest.raises(RuntimeError, match="floats per channel"):
        ensemble.ens_merge(out[:-1].contiguous(), N, H, W, (6,))
    with pytest.raises(RuntimeError, match="cuda float32"):
        ensemble.ens_gather(xd.cpu(), "d8")


# ------------------------------------------------------------------ the modules against the hand-written loop
T_KW = dict(dim=48, num_blocks=[1, 1, 1, 1], num_refinement_blocks=1, LayerNorm_type="BiasFree")
S_KW = dict(residual=True, hidden_channels=[16, 32, 64])
MODULE_SHAPES = [(24, 40), (16, 16)]
MODE_SETS = ["d8", "flips", (0,)]


def _turn(x, m):
    x = torch.rot90(x, m // 2, (-2, -1))
    return x.flip(-2) if m % 2 else x


def _turn_back(u, m):
    u = u.flip(-2) if m % 2 else u
    return torch.rot90(u, -(m // 2), (-2, -1))


def host_loop(forward, inputs, modes):
    """What a user writes without the feature.  `forward(*views)` -> tuple of outputs (None entries kept)."""
    modes = em.modes_of(em.mask_of(modes))
    acc = None
    with torch.no_grad():
        for m in modes:
            outs = forward(*[_turn(t, m).contiguous() if t is not None else None for t in inputs])
            us = [_turn_back(o, m) if o is not None else None for o in outs]
            if acc is None:
                acc = [torch.zeros_like(u) if u is not None else None for u in us]
            for a, u in zip(acc, us):
                if a is not None:
                    a.add_(u)
        for a in acc:
            if a is not None:
                a.div_(len(modes))
    return acc


def _ramp_rate(B, h, w):
    """A per-pixel ramp, different for every image and for every flip and turn of it."""
    ramp = torch.linspace(0.05, 0.95, h * w, device=DEV).view(1, 1, h, w)
    return torch.cat([ramp if b % 2 == 0 else ramp.flip(-1) * 0.5 for b in range(B)]).contiguous()


@functools.lru_cache(maxsize=None)
def _teacher(graphs=False):
    m = KDLAE_teacher(**T_KW)
    load_hash_weights(m)
    m.hip_graphs = graphs
    return m.to(DEV).eval()


@functools.lru_cache(maxsize=None)
def _restormer():
    m = Restormer(**T_KW)
    load_hash_weights(m)
    m.hip_graphs = False
    return m.to(DEV).eval()


@functools.lru_cache(maxsize=None)
def _student():
    m = KDLAE_student(**S_KW)
    load_hash_weights(m)
    return m.to(DEV).eval()


def _t_forward(m):
    def f(img, rate):
        o = m({"img": img, "denoise_rate": rate})
        return o["hq"], o["sr"]
    return f


@functools.lru_cache(maxsize=None)
def _teacher_case(hw, modes):
    """(img, rate, loop hq, loop sr), computed once and shared; nothing below writes to them."""
    h, w = hw
    img = torch.from_numpy(hash_images(f"ens:t:{h}x{w}", (2, 3, h, w))).to(DEV)
    rate = _ramp_rate(2, h, w)
    return (img, rate) + tuple(host_loop(_t_forward(_teacher()), (img, rate), modes))


@pytest.mark.parametrize("modes", MODE_SETS, ids=str)
@pytest.mark.parametrize("hw", MODULE_SHAPES, ids=str)
def test_teacher_forward_ensemble_equals_the_host_loop(hw, modes):
    m = _teacher()
    img, rate, l_hq, l_sr = _teacher_case(hw, modes)
    h, w = hw
    for ens_batch in (1, 3, 8, 16):
        out = m.forward_ensemble({"img": img, "denoise_rate": rate}, modes, ens_batch)
        assert out["hq"].shape == (2, 3, h, w) and out["sr"].shape == (2, 3, 2 * h, 2 * w)
        assert _same_bits(out["hq"], l_hq), f"hq at ens_batch {ens_batch}"
        assert _same_bits(out["sr"], l_sr), f"sr at ens_batch {ens_batch}"
    if modes == (0,):
        with torch.no_grad():
            ref = m({"img": img, "denoise_rate": rate})
        assert _same_bits(out["hq"], ref["hq"]) and _same_bits(out["sr"], ref["sr"])
    else:   # a different function of the image, and the rate map does reach the views turned with them
        assert not torch.equal(l_hq, _teacher_case(hw, (0,))[2])
        flat = m.forward_ensemble({"img": img, "denoise_rate": torch.full_like(rate, 0.6)}, modes)
        assert not torch.equal(flat["hq"], l_hq)


def test_teacher_forward_ensemble_with_graph_replay_gives_the_same_bits():
    m = _teacher(graphs=True)
    assert m.hip_graphs
    for hw in MODULE_SHAPES:
        img, rate, l_hq, l_sr = _teacher_case(hw, "d8")
        # 16 x 16: one chunk of eight views, eager, then captured, then replayed; 24 x 40: four chunks of two
        for _ in range(3):
            out = m.forward_ensemble({"img": img, "denoise_rate": rate})
            assert _same_bits(out["hq"], l_hq) and _same_bits(out["sr"], l_sr)
    assert len(m.__dict__.get("_graphs", {})) >= 1


def test_teacher_variants_and_refusals():
    img, rate, _, _ = _teacher_case((24, 40), "d8")
    nosr = KDLAE_teacher(**T_KW, static="no", params="plus")
    load_hash_weights(nosr)
    nosr.hip_graphs = False
    nosr = nosr.to(DEV).eval()
    want = host_loop(lambda a: (nosr({"img": a, "denoise_rate": None})["hq"],), (img,), "d8")[0]
    out = nosr.forward_ensemble({"img": img, "denoise_rate": None}, "d8", 3)
    assert out["sr"] is None and _same_bits(out["hq"], want)
    m = _teacher()
    with pytest.raises(RuntimeError, match="ens_batch"):
        m.forward_ensemble({"img": img, "denoise_rate": rate}, "d8", 0)
    with pytest.raises(RuntimeError, match="modes"):
        m.forward_ensemble({"img": img, "denoise_rate": rate}, "d4")
    with pytest.raises(RuntimeError, match="denoise_rate must be"):
        m.forward_ensemble({"img": img, "denoise_rate": rate[:1]})
    with pytest.raises(RuntimeError, match="divisible by 8"):
        m.forward_ensemble({"img": img[..., :20, :], "denoise_rate": rate[..., :20, :]})
    m.train()
    try:
        with pytest.raises(RuntimeError, match="inference-only"):
            m.forward_ensemble({"img": img, "denoise_rate": rate})
    finally:
        m.eval()


@pytest.mark.parametrize("modes", MODE_SETS, ids=str)
@pytest.mark.parametrize("hw", MODULE_SHAPES, ids=str)
def test_restormer_forward_ensemble_equals_the_host_loop(hw, modes):
    m = _restormer()
    h, w = hw
    x = torch.from_numpy(hash_images(f"ens:r:{h}x{w}", (2, 3, h, w))).to(DEV)
    want = host_loop(lambda a: (m(a),), (x,), modes)[0]
    for ens_batch in (1, 3, 8, 16):
        got = m.forward_ensemble(x, modes, ens_batch)
        assert got.shape == (2, 3, h, w) and _same_bits(got, want), f"ens_batch {ens_batch}"
    if modes == (0,):
        with torch.no_grad():
            assert _same_bits(got, m(x))


@pytest.mark.parametrize("modes", MODE_SETS, ids=str)
def test_student_forward_ensemble_equals_the_host_loop(modes):
    m = _student()
    x = torch.from_numpy(hash_images("ens:s", (2, 4, 24, 40))).to(DEV)
    want = host_loop(lambda a: (m(a),), (x,), modes)[0]
    for ens_batch in (1, 3, 8, 16):
        got = m.forward_ensemble(x, modes, ens_batch)
        assert got.shape == x.shape and _same_bits(got, want), f"ens_batch {ens_batch}"
    if modes == (0,):
        with torch.no_grad():
            assert _same_bits(got, m(x))
    else:
        with torch.no_grad():
            assert not torch.equal(got, m(x))
    with pytest.raises(RuntimeError, match="ens_batch"):
        m.forward_ensemble(x, modes, 0)


# ------------------------------------------------------------------ pipeline and validation
def test_enhance_ensemble_u8_equals_pre_and_post_around_the_host_loop():
    """21 x 37 images: reflect-padded to 24 x 40, the eight views, merged, cropped back."""
    m = _teacher()
    B, h, w = 2, 21, 37
    x = np.random.default_rng(21).integers(0, 256, (B, h, w, 3), dtype=np.uint8)
    x[:, : h // 3, : w // 4] = 0   # an all-black region: masked in the output
    images = torch.from_numpy(x).to(DEV)
    img, rmap = preprocess_u8(images, 0.6, 8, False)
    assert img.shape == (B, 3, 24, 40)
    l_hq, l_sr = host_loop(_t_forward(m), (img, rmap), "d8")
    want_hq, want_sr = postprocess_u8(l_hq, h, w, 1, images), postprocess_u8(l_sr, h, w, 2, images)
    for ens_batch in (8, 3):
        hq, sr = enhance_ensemble_u8(m, images, 0.6, "d8", ens_batch)
        assert hq.dtype == torch.uint8 and hq.shape == (B, h, w, 3) and sr.shape == (B, 2 * h, 2 * w, 3)
        assert torch.equal(hq, want_hq) and torch.equal(sr, want_sr)
    assert bool((hq[:, : h // 3, : w // 4] == 0).all())
    r = _restormer()
    r_img, _ = preprocess_u8(images, None, 8, True)
    want = postprocess_u8(host_loop(lambda a: (r(a),), (r_img,), "flips")[0], h, w, 1, images)
    hq, sr = enhance_ensemble_u8(r, images, None, "flips", 8, bgr=True)
    assert sr is None and torch.equal(hq, want)


# the smallest teacher the training and the inference engine both take (tests/test_validate_gpu.py)
V_CFG = dict(dim=16, num_blocks=[1, 1, 1, 1], num_refinement_blocks=1, LayerNorm_type="BiasFree")
VH, VW = 20, 28   # pads to 24 x 32


def _vimg(tag, shape):
    return torch.from_numpy(hash_images(tag, shape)).to(DEV)


def _v_batch(i):
    lq = {"img": _vimg(f"ens:v:img{i}", (2, 3, 32, 32)), "denoise_rate": torch.full((2, 1, 32, 32), 0.6, device=DEV)}
    gt = {"hq": _vimg(f"ens:v:hq{i}", (2, 3, 32, 32)), "sr": _vimg(f"ens:v:sr{i}", (2, 3, 64, 64))}
    return lq, gt


def _v_trainer():
    m = KDLAE_teacher(**V_CFG)
    load_hash_weights(m)
    return KDLAETrainer(m.to(DEV), lr=1e-3, ema_decay=0.999)


def _snap(tr, loss):
    torch.cuda.synchronize()
    return {"theta": tr.theta.cpu().clone(), "exp_avg": tr.exp_avg.cpu().clone(),
            "exp_avg_sq": tr.exp_avg_sq.cpu().clone(), "loss": float(loss)}


def test_validate_ensemble_is_psnr_of_forward_ensemble_and_training_continues():
    plain = _v_trainer()
    for i in range(3):
        loss = plain.optimize_parameters(*_v_batch(i))
    want_state = _snap(plain, loss)
    tr = _v_trainer()
    for i in range(2):
        tr.optimize_parameters(*_v_batch(i))
    items = []
    for i in range(2):
        lq = {"img": _vimg(f"ens:v:vimg{i}", (1, 3, VH, VW)), "denoise_rate": _vimg(f"ens:v:vrate{i}", (1, 1, VH, VW))}
        gt = {"hq": _vimg(f"ens:v:vhq{i}", (1, 3, VH, VW)), "sr": _vimg(f"ens:v:vsr{i}", (1, 3, 2 * VH, 2 * VW))}
        items.append((lq, gt))
    before = tr.validate(items)
    # a fresh module with the evaluated (EMA) weights is the reference
    ref = KDLAE_teacher(**V_CFG)
    ref.load_state_dict({k: v.detach().cpu().clone() for k, v in tr.ema_state_dict().items()})
    ref = ref.to(DEV).eval()
    ref.hip_graphs = False
    p_hq, p_sr = [], []
    for lq, gt in items:
        img = F.pad(lq["img"], (0, 32 - VW, 0, 24 - VH), "reflect")
        rate = F.pad(lq["denoise_rate"], (0, 32 - VW, 0, 24 - VH), "reflect")
        out = ref.forward_ensemble({"img": img, "denoise_rate": rate}, "d8", 3)
        tr.validate([(lq, gt)], ensemble="d8", ens_batch=3)
        assert _same_bits(tr.val_output["hq"], out["hq"][..., :VH, :VW])
        assert _same_bits(tr.val_output["sr"], out["sr"][..., :2 * VH, :2 * VW])
        p_hq.append(psnr_batch(out["hq"], gt["hq"], (VH, VW), 0, False))
        p_sr.append(psnr_batch(out["sr"], gt["sr"], (2 * VH, 2 * VW), 0, False))
    res = tr.validate(items, ensemble="d8", ens_batch=3)
    assert set(res) == {"psnr_hq", "psnr_sr"}
    assert res["psnr_hq"] == float(torch.cat(p_hq).mean()) and res["psnr_sr"] == float(torch.cat(p_sr).mean())
    assert res == tr.validate(items, ensemble="d8", ens_batch=8)
    assert res != before and before == tr.validate(items)          # the default is what it was
    with pytest.raises(RuntimeError, match="cannot be combined"):
        tr.validate(items, ensemble="d8", tile=16)
    # the third step equals the third step of a run that never validated
    got = _snap(tr, tr.optimize_parameters(*_v_batch(2)))
    for k in ("theta", "exp_avg", "exp_avg_sq"):
        assert torch.equal(got[k], want_state[k]), k
    assert got["loss"] == want_state["loss"]


def test_restormer_validate_ensemble():
    m = Restormer(**V_CFG)
    load_hash_weights(m)
    tr = RestormerTrainer(m.to(DEV), lr=1e-3)
    lq, gt = _vimg("ens:rv:lq", (2, 3, VH, VW)), _vimg("ens:rv:gt", (2, 3, VH, VW))
    ref = Restormer(**V_CFG)
    ref.load_state_dict({k: v.detach().cpu().clone() for k, v in tr.model.state_dict().items()})
    ref = ref.to(DEV).eval()
    ref.hip_graphs = False
    out = ref.forward_ensemble(F.pad(lq, (0, 32 - VW, 0, 24 - VH), "reflect"), "flips")
    res = tr.validate([(lq, gt)], ensemble="flips")
    assert _same_bits(tr.val_output["hq"], out[..., :VH, :VW])
    assert res == {"psnr_hq": float(psnr_batch(out, gt, (VH, VW), 0, False).mean())}
    with pytest.raises(RuntimeError, match="cannot be combined"):
        tr.validate([(lq, gt)], ensemble="flips", tile=16)


# ------------------------------------------------------------------ the caller's-stream contract of the two entries
ENS = dict(N=2, C=3, H=24, W=40, mask=255)


def ens_gather_call(off):
    N, C, H, W, mask = (ENS[k] for k in ("N", "C", "H", "W", "mask"))
    o = {"src": _f("ens:src", (N, C, H, W), off=off)}

    def make(o, outs, ws):
        return [("kdlae_ens_gather", lambda: _lib.lib().kdlae_ens_gather(
            vp(o["src"]), vp(outs[0]), N, C, H, W, mask, stream()))]
    return Simple(o, (8 * N * C * H * W,), make)


def ens_merge_call(off):
    N, C, H, W, mask = (ENS[k] for k in ("N", "C", "H", "W", "mask"))
    o = {"staged": _f("ens:staged", (8, N * C * H * W), -1.0, 1.0, off=off)}

    def make(o, outs, ws):
        return [("kdlae_ens_merge", lambda: _lib.lib().kdlae_ens_merge(
            vp(o["staged"]), vp(outs[0]), N, C, H, W, mask, stream()))]
    return Simple(o, (N * C * H * W,), make)


# "vec" = every pointer on 16 bytes (the float4 launch), "elem" = a source 4 bytes past it
STREAM_CASES = [("ens-gather-vec", lambda: ens_gather_call(0)), ("ens-gather-elem", lambda: ens_gather_call(1)),
                ("ens-merge-vec", lambda: ens_merge_call(0)), ("ens-merge-elem", lambda: ens_merge_call(1))]


@pytest.mark.parametrize("factory", [pytest.param(f, id=i) for i, f in STREAM_CASES])
def test_asynchrony_and_order_on_a_side_stream(factory):
    check_async_and_order(factory())


@pytest.mark.parametrize("factory", [pytest.param(f, id=i) for i, f in STREAM_CASES])
def test_graph_capture_on_a_side_stream(factory):
    check_capture(factory())
