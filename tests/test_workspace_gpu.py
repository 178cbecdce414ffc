"""The workspace contract (include/kdlae.h) on every engine, through the C ABI on handles of the Python engines:

P1  exact fit: workspace_bytes - 1 is refused before anything is launched; in exactly workspace_bytes no word outside
    the workspace and the outputs changes (guards of 64 KiB on every side, workspace base at 256 mod 512 bytes),
    and the read-only operands keep their bits;
P2  the outputs do not depend on what the workspace and the output buffers held on entry: zero bytes, 0xFFFFFFFF
    (NaN) and 1e30 give the same bits, finite, and the bits of the ordinary Python path;
P3  a backward overwrites `grad`: NaN-prefilled it comes back finite, +0.0 in the pad floats between keys and in
    the keys the model does not use, bit-equal to the trainer's own path; asdqe_train_backward(accumulate=1) is
    one fp32 add on top of what was there;
P4  a smaller call on the workspace a larger call just used gives the bits it gives on a zeroed workspace.

Every comparison is bit equality or finiteness: no tolerance in this file (tests/workspace_harness.py)."""
import functools
import os

import pytest
import torch

from rethink_acoustic_image_enhancement_amd import _lib
from rethink_acoustic_image_enhancement_amd.ASDQE_model import DenoiseRatePredictor
from rethink_acoustic_image_enhancement_amd.hashweights import hash_images, load_hash_weights
from rethink_acoustic_image_enhancement_amd.KDLAE_model import KDLAE_student, KDLAE_teacher
from rethink_acoustic_image_enhancement_amd.train import AsdqeTrainEngine, StudentTrainEngine, TrainEngine
from tests.util import load_fixture
from tests.workspace_harness import (DEV, ONES, Arena, Call, bits, check_exact_fit, check_scratch_independence,
                                     check_small_after_large, same_bits, stream, vp)

pytestmark = pytest.mark.gpu


def _images(key, shape, lo=0.0, hi=1.0):
    return torch.from_numpy(hash_images(key, shape, lo, hi)).to(DEV)


# ----------------------------------------------------------------------------- KDLAE-T inference
KW = dict(dim=48, LayerNorm_type="BiasFree", num_blocks=[2, 1, 1, 1], num_refinement_blocks=1)
T_CONFIGS = {
    "default": KW,                                                        # BiasFree, static='train', params='cat'
    "withbias": {**KW, "LayerNorm_type": "WithBias", "bias": True},
    "dim16": dict(dim=16, bias=True, num_blocks=[1, 1, 1, 1], num_refinement_blocks=1),   # the unfused paths
    "nosr": {**KW, "static": "no"},
    "plus": {**KW, "params": "plus"},
    "nofold": KW,                                                         # under KDLAE_DEBUG=no_sr_fold: cenb planned
}
# 24 x 16: the smallest H != W, W % 16 == 0 (strip Gram); 16 x 24: W % 16 != 0 (generic Gram partition), three
# images; 40 x 48: H no multiple of the 32-row Gram segment; 64 x 64: every fused C = 48 / 96 kernel applies
T_SHAPES = [(1, 24, 16), (3, 16, 24), (2, 40, 48), (1, 64, 64)]


@functools.lru_cache(maxsize=None)
def _teacher(name):
    m = KDLAE_teacher(**T_CONFIGS[name])
    load_hash_weights(m)
    m.hip_graphs = False
    m = m.to(DEV).eval()
    old = os.environ.get("KDLAE_DEBUG")
    try:   # the flag is read when the handle builds its pack program (tests/test_sr_fold_gpu.py does the same)
        if name == "nofold":
            os.environ["KDLAE_DEBUG"] = "no_sr_fold"
        else:
            os.environ.pop("KDLAE_DEBUG", None)
        m.engine(DEV)
    finally:
        if old is None:
            os.environ.pop("KDLAE_DEBUG", None)
        else:
            os.environ["KDLAE_DEBUG"] = old
    return m


class TForward(Call):
    """kdlae_t_forward"""

    def __init__(self, m, B, H, W, key="ws:t"):
        self.m, self.shape = m, (B, H, W)
        c = m._cfg
        self.eng = m.engine(DEV)
        self.eng.sync_params(m, stream().value or 0)
        self.img = _images(f"{key}:img:{B}x{H}x{W}", (B, c["inp_channels"], H, W))
        self.rate = _images(f"{key}:rate:{B}x{H}x{W}", (B, 1, H, W))
        self.cat, self.has_sr = c["params"] == "cat", c["static"] == "train"
        n = B * c["out_channels"] * H * W
        self.out_numels = (n, 4 * n if self.has_sr else 0)
        self.ws_bytes = _lib.lib().kdlae_t_workspace_bytes(self.eng.handle, B, H, W)
        self.operands = {"img": self.img, "rate": self.rate, "params": self.eng.flat}

    def steps(self, arena):
        B, H, W = self.shape
        hq, sr = arena.outs
        return [("kdlae_t_forward", lambda nbytes: _lib.lib().kdlae_t_forward(
            self.eng.handle, vp(self.img), vp(self.rate if self.cat else None), B, H, W, vp(hq),
            vp(sr if self.has_sr else None), vp(arena.ws), nbytes, stream()))]

    def reference(self):
        with torch.no_grad():
            out = self.m({"img": self.img, "denoise_rate": self.rate})
        torch.cuda.synchronize()
        return [out["hq"], out["sr"]]


class TSr(Call):
    """kdlae_t_forward_sr on an unclamped hq"""

    def __init__(self, m, B, H, W):
        self.m, self.shape = m, (B, H, W)
        oc = m._cfg["out_channels"]
        self.eng = m.engine(DEV)
        self.eng.sync_params(m, stream().value or 0)
        self.hq = _images(f"ws:sr:hq:{B}x{H}x{W}", (B, oc, H, W), -0.25, 1.25)
        self.out_numels = (4 * B * oc * H * W,)
        self.ws_bytes = _lib.lib().kdlae_t_sr_workspace_bytes(self.eng.handle, B, H, W)
        self.operands = {"hq": self.hq, "params": self.eng.flat}

    def steps(self, arena):
        B, H, W = self.shape
        return [("kdlae_t_forward_sr", lambda nbytes: _lib.lib().kdlae_t_forward_sr(
            self.eng.handle, vp(self.hq), B, H, W, vp(arena.outs[0]), vp(arena.ws), nbytes, stream()))]

    def reference(self):
        with torch.no_grad():
            sr = self.m.forward_sr(self.hq)
        torch.cuda.synchronize()
        return [sr]


T_CASES = [(name, shape) for name in T_CONFIGS for shape in T_SHAPES]
T_IDS = [f"{name}-{B}x{H}x{W}" for name, (B, H, W) in T_CASES]
SR_CASES = [(name, shape) for name in ("default", "withbias", "dim16", "plus", "nofold") for shape in T_SHAPES]
SR_IDS = [f"{name}-{B}x{H}x{W}" for name, (B, H, W) in SR_CASES]


@pytest.mark.parametrize("name,shape", T_CASES, ids=T_IDS)
def test_t_forward_exact_fit(name, shape):
    check_exact_fit(TForward(_teacher(name), *shape))


@pytest.mark.parametrize("name,shape", T_CASES, ids=T_IDS)
def test_t_forward_scratch_independence(name, shape):
    call = TForward(_teacher(name), *shape)
    check_scratch_independence(call, call.reference())


@pytest.mark.parametrize("name,shape", SR_CASES, ids=SR_IDS)
def test_t_forward_sr_exact_fit(name, shape):
    check_exact_fit(TSr(_teacher(name), *shape))


@pytest.mark.parametrize("name,shape", SR_CASES, ids=SR_IDS)
def test_t_forward_sr_scratch_independence(name, shape):
    call = TSr(_teacher(name), *shape)
    check_scratch_independence(call, call.reference())


class TRates(Call):
    """kdlae_t_forward_rates with the sr head: R rates of B images, scalars (is_map 0) or maps (is_map 1)"""

    def __init__(self, m, B, R, H, W, is_map):
        self.m, self.shape, self.is_map = m, (B, R, H, W), is_map
        self.eng = m.engine(DEV)
        self.eng.sync_params(m, stream().value or 0)
        self.img = _images("ws:rates:img", (B, 3, H, W))
        self.rates = _images(f"ws:rates:{is_map}", (R, B, 1, H, W) if is_map else (R, B))
        n = R * B * 3 * H * W
        self.out_numels = (n, 4 * n)
        self.ws_bytes = _lib.lib().kdlae_t_rates_workspace_bytes(self.eng.handle, B, R, H, W, 1)
        self.operands = {"img": self.img, "rates": self.rates}

    def steps(self, arena):
        B, R, H, W = self.shape
        return [("kdlae_t_forward_rates", lambda nbytes: _lib.lib().kdlae_t_forward_rates(
            self.eng.handle, vp(self.img), vp(self.rates), self.is_map, B, R, H, W, vp(arena.outs[0]),
            vp(arena.outs[1]), vp(arena.ws), nbytes, stream()))]

    def reference(self):
        with torch.no_grad():
            ref = self.m.forward_rates(self.img, self.rates, sr=True)
        torch.cuda.synchronize()
        return [ref["hq"], ref["sr"]]


def test_t_forward_rates_scratch_independence():
    """kdlae_t_forward_rates (its exact fit: test_rate_sweep_gpu.test_no_overrun_at_64_rates_and_short_workspace_
    refused): three rates of three 16 x 24 images, scalars and maps."""
    m = _teacher("default")
    for is_map in (0, 1):
        call = TRates(m, 3, 3, 16, 24, is_map)
        ref = call.reference()
        check_exact_fit(call)
        check_scratch_independence(call, ref)


@pytest.mark.parametrize("name", ["default", "dim16"])
def test_t_forward_small_after_large(name):
    m = _teacher(name)
    check_small_after_large(TForward(m, 3, 16, 24), TForward(m, 1, 16, 24))      # the last, smaller tile chunk
    check_small_after_large(TForward(m, 2, 40, 48), TForward(m, 2, 24, 16))
    check_small_after_large(TForward(m, 3, 64, 64), TForward(m, 1, 24, 16))


# ----------------------------------------------------------------------------- KDLAE-S inference
S_CONFIGS = ("s_default_b2", "s_nores_3lvl")   # the two configurations of tests/test_kdlae_s_gpu.py's fixtures


@functools.lru_cache(maxsize=None)
def _student(name):
    _, kw = load_fixture(name)
    m = KDLAE_student(**kw)
    load_hash_weights(m)
    return m.to(DEV).eval()


def _student_shapes(m):
    """The smallest H, W the model takes (2^levels) with one frame; two bursts of four frames with H != W."""
    k = 1 << m.num_levels
    return list(dict.fromkeys([(1, 1, k, k), (2, 4, 2 * k, 3 * k), (2, 4, 16, 24)]))


class SForward(Call):
    """kdlae_s_forward"""

    def __init__(self, m, B, F, H, W):
        self.m, self.shape = m, (B, F, H, W)
        self.eng = m.engine(DEV)
        self.eng.sync_params(m, stream().value or 0)
        self.x = _images(f"ws:s:{B}x{F}x{H}x{W}", (B, F, H, W))
        self.out_numels = (B * F * H * W,)
        self.ws_bytes = _lib.lib().kdlae_s_workspace_bytes(self.eng.handle, B, F, H, W)
        self.operands = {"x": self.x, "params": self.eng.flat}

    def steps(self, arena):
        B, F, H, W = self.shape
        return [("kdlae_s_forward", lambda nbytes: _lib.lib().kdlae_s_forward(
            self.eng.handle, vp(self.x), B, F, H, W, vp(arena.outs[0]), vp(arena.ws), nbytes, stream()))]

    def reference(self):
        with torch.no_grad():
            y = self.m(self.x)
        torch.cuda.synchronize()
        return [y]


@pytest.mark.parametrize("name", S_CONFIGS)
def test_s_forward_exact_fit_and_scratch_independence(name):
    m = _student(name)
    for shape in _student_shapes(m):
        call = SForward(m, *shape)
        check_exact_fit(call)
        check_scratch_independence(call, call.reference())


@pytest.mark.parametrize("name", S_CONFIGS)
def test_s_forward_small_after_large(name):
    m = _student(name)
    check_small_after_large(SForward(m, 3, 4, 16, 24), SForward(m, 1, 4, 16, 24))
    check_small_after_large(SForward(m, 2, 3, 40, 48), SForward(m, 2, 3, 24, 16))


# ----------------------------------------------------------------------------- ASDQE inference
@functools.lru_cache(maxsize=None)
def _asdqe(ci=3):
    m = DenoiseRatePredictor(in_channels=ci)
    load_hash_weights(m)
    return m.to(DEV).eval()


class AForward(Call):
    """asdqe_forward; with_feat: the optional UNet output map as a second output"""

    def __init__(self, m, B, H, W, with_feat):
        self.m, self.shape, self.with_feat = m, (B, H, W), with_feat
        ci, d = m._cfg["in_channels"], m._cfg["dim"]
        self.eng = m.engine(DEV)
        self.eng.sync_params(m, stream().value or 0)
        self.lq = _images(f"ws:a:lq:{B}x{H}x{W}", (B, ci, H, W))
        self.gt = _images(f"ws:a:gt:{B}x{H}x{W}", (B, ci, H, W))
        Hp, Wp = -(-H // d) * d, -(-W // d) * d
        self.out_numels = (B, B * Hp * Wp * 3 * d if with_feat else 0)
        self.ws_bytes = _lib.lib().asdqe_workspace_bytes(self.eng.handle, B, H, W)
        self.operands = {"lq": self.lq, "gt": self.gt, "params": self.eng.flat}

    def steps(self, arena):
        B, H, W = self.shape
        return [("asdqe_forward", lambda nbytes: _lib.lib().asdqe_forward(
            self.eng.handle, vp(self.lq), vp(self.gt), B, H, W, vp(arena.outs[0]),
            vp(arena.outs[1] if self.with_feat else None), vp(arena.ws), nbytes, stream()))]

    def reference(self):
        with torch.no_grad():
            if self.with_feat:
                score, feat = self.m(self.lq, self.gt, return_features=True)
                ref = [score, feat.permute(0, 2, 3, 1)]    # back to the NHWC the entry point writes
            else:
                ref = [self.m(self.lq, self.gt), None]
        torch.cuda.synchronize()
        return ref


# 37 x 50: the odd size tests/test_abi.py queries; 1 x 1: the smallest size accepted (padded to 16 x 16)
@pytest.mark.parametrize("B,H,W,with_feat", [(2, 37, 50, True), (2, 37, 50, False), (1, 1, 1, False), (1, 1, 1, True)])
def test_asdqe_forward_exact_fit_and_scratch_independence(B, H, W, with_feat):
    call = AForward(_asdqe(), B, H, W, with_feat)
    check_exact_fit(call)
    check_scratch_independence(call, call.reference())


# ----------------------------------------------------------------------------- training: shared checks
def _grad_checks(eng, grad, unused_prefixes=()):
    """P3 on a gradient buffer that held NaN on entry."""
    assert bool(torch.isfinite(grad).all()), "grad was accumulated into, or only partly written"
    pad = torch.ones(eng.numel, dtype=torch.bool, device=grad.device)
    for k, n, off in eng.keys:
        pad[off:off + n] = False
        if unused_prefixes and k.startswith(unused_prefixes):
            assert bool((bits(grad[off:off + n]) == 0).all()), f"unused key {k} is not +0.0"
    assert bool((bits(grad)[pad] == 0).all()), "a pad float between keys is not +0.0"


def _signed(key, shape, scale):
    return _images(key, shape, -scale, scale)


# ----------------------------------------------------------------------------- KDLAE-T training
TT_CONFIGS = {
    "dim16": (T_CONFIGS["dim16"], (2, 48, 40)),
    "default": (KW, (2, 32, 32)),
    "plus_nosr": (dict(dim=16, num_blocks=[1, 1, 1, 1], num_refinement_blocks=1, static="no", params="plus"),
                  (1, 24, 16)),
}


@functools.lru_cache(maxsize=None)
def _tt(name):
    m = KDLAE_teacher(**TT_CONFIGS[name][0])
    load_hash_weights(m)
    m = m.to(DEV)
    return m, TrainEngine(m, torch.device(DEV))


class TTStep(Call):
    """kdlae_tt_forward + kdlae_tt_backward (or _marked) on one workspace; outputs hq, sr, grad"""

    def __init__(self, name, B, H, W, marked=False):
        self.m, self.eng = _tt(name)
        c = self.m._cfg
        self.shape, self.marked = (B, H, W), marked
        self.theta = self.eng.flatten(self.m.parameters())
        self.img = _images(f"ws:tt:img:{B}x{H}x{W}", (B, c["inp_channels"], H, W))
        self.rate = _images(f"ws:tt:rate:{B}x{H}x{W}", (B, 1, H, W)) if self.eng.params_cat else None
        n = B * c["out_channels"] * H * W
        self.has_sr = self.eng.static_train
        self.dhq = _signed(f"ws:tt:dhq:{B}x{H}x{W}", (n,), 1.0 / n)
        self.dsr = _signed(f"ws:tt:dsr:{B}x{H}x{W}", (4 * n,), 0.25 / n) if self.has_sr else None
        self.out_numels = (n, 4 * n if self.has_sr else 0, self.eng.numel)
        self.ws_bytes = int(_lib.lib().kdlae_tt_workspace_bytes(self.eng.handle, B, H, W))
        self.operands = {"theta": self.theta, "img": self.img, "rate": self.rate, "dhq": self.dhq, "dsr": self.dsr}

    def steps(self, arena):
        L, h = _lib.lib(), self.eng.handle
        B, H, W = self.shape
        hq, sr, grad = arena.outs
        bwd_name = "kdlae_tt_backward_marked" if self.marked else "kdlae_tt_backward"
        bwd = getattr(L, bwd_name)
        return [("kdlae_tt_forward", lambda nbytes: L.kdlae_tt_forward(
                    h, vp(self.theta), vp(self.img), vp(self.rate), B, H, W, vp(hq), vp(sr if self.has_sr else None),
                    vp(arena.ws), nbytes, stream())),
                (bwd_name, lambda nbytes: bwd(h, vp(self.theta), vp(self.dhq), vp(self.dsr), vp(grad),
                                                  vp(arena.ws), nbytes, stream()))]

    def reference(self):
        """The trainer's own path: TrainEngine.forward / backward on its torch.empty workspace."""
        hq, sr = self.eng.forward(self.theta, self.img, self.rate)
        grad = torch.full((self.eng.numel,), float("nan"), device=DEV)
        self.eng.backward(self.theta, self.dhq, self.dsr, grad, marked=self.marked)
        torch.cuda.synchronize()
        return [hq, sr, grad]


TT_CASES = [(name, marked) for name in TT_CONFIGS for marked in (False, True)]
TT_IDS = [f"{name}-{'marked' if marked else 'plain'}" for name, marked in TT_CASES]


@pytest.mark.parametrize("name,marked", TT_CASES, ids=TT_IDS)
def test_tt_exact_fit(name, marked):
    check_exact_fit(TTStep(name, *TT_CONFIGS[name][1], marked=marked))


@pytest.mark.parametrize("name,marked", TT_CASES, ids=TT_IDS)
def test_tt_scratch_independence_and_grad_overwritten(name, marked):
    """P2 with the poison applied before the forward only, and P3: the 0xFFFFFFFF run prefilled `grad` with NaN."""
    call = TTStep(name, *TT_CONFIGS[name][1], marked=marked)
    hq, sr, grad = check_scratch_independence(call, call.reference())
    unused = ("output_param.", "refinement_out.") if not call.eng.params_cat else ()
    _grad_checks(call.eng, grad, unused)
    assert bool(grad.abs().max() > 0)


def test_tt_small_after_large():
    check_small_after_large(TTStep("dim16", 3, 16, 24), TTStep("dim16", 1, 16, 24))
    check_small_after_large(TTStep("dim16", 2, 40, 48), TTStep("dim16", 2, 24, 16))
    check_small_after_large(TTStep("default", 2, 40, 48, marked=True), TTStep("default", 2, 24, 16, marked=True))


# ----------------------------------------------------------------------------- KDLAE-S training
ST_CONFIGS = {
    "s3": dict(residual=True, hidden_channels=[16, 32, 64]),        # 16 -> 16 convs: the dX path with the zero bias
    "s4": dict(residual=False, hidden_channels=[8, 16, 16, 32]),
}
# 16 x 16: level 0 is 16 wide (direct convs), the deeper levels are not (column matrices); 32 x 24: no level is
ST_SHAPES = [(1, 3, 16, 16), (2, 4, 32, 24)]


@functools.lru_cache(maxsize=None)
def _st(name):
    m = KDLAE_student(**ST_CONFIGS[name])
    load_hash_weights(m)
    m = m.to(DEV)
    return m, StudentTrainEngine(m, torch.device(DEV))


class STStep(Call):
    """kdlae_st_forward + kdlae_st_backward on one workspace; outputs out, grad"""

    def __init__(self, name, B, F, H, W):
        self.m, self.eng = _st(name)
        self.shape = (B, F, H, W)
        self.theta = self.eng.flatten(self.m.parameters())
        n = B * F * H * W
        self.x = _images(f"ws:st:x:{B}x{F}x{H}x{W}", (B, F, H, W))
        self.dout = _signed(f"ws:st:dout:{B}x{F}x{H}x{W}", (B, F, H, W), 1.0 / n)
        self.out_numels = (n, self.eng.numel)
        self.ws_bytes = int(_lib.lib().kdlae_st_workspace_bytes(self.eng.handle, B, F, H, W))
        self.operands = {"theta": self.theta, "x": self.x, "dout": self.dout}

    def steps(self, arena):
        L, h = _lib.lib(), self.eng.handle
        B, F, H, W = self.shape
        out, grad = arena.outs
        return [("kdlae_st_forward", lambda nbytes: L.kdlae_st_forward(
                    h, vp(self.theta), vp(self.x), B, F, H, W, vp(out), vp(arena.ws), nbytes, stream())),
                ("kdlae_st_backward", lambda nbytes: L.kdlae_st_backward(
                    h, vp(self.theta), vp(self.dout), vp(grad), vp(arena.ws), nbytes, stream()))]

    def reference(self):
        out = self.eng.forward(self.theta, self.x)
        grad = torch.full((self.eng.numel,), float("nan"), device=DEV)
        self.eng.backward(self.theta, self.dout, grad)
        torch.cuda.synchronize()
        return [out, grad]


ST_CASES = [(name, shape) for name in ST_CONFIGS for shape in ST_SHAPES]
ST_IDS = [f"{name}-{B}x{F}x{H}x{W}" for name, (B, F, H, W) in ST_CASES]


@pytest.mark.parametrize("name,shape", ST_CASES, ids=ST_IDS)
def test_st_exact_fit(name, shape):
    check_exact_fit(STStep(name, *shape))


@pytest.mark.parametrize("name,shape", ST_CASES, ids=ST_IDS)
def test_st_scratch_independence_and_grad_overwritten(name, shape):
    call = STStep(name, *shape)
    out, grad = check_scratch_independence(call, call.reference())
    _grad_checks(call.eng, grad)
    assert bool(grad.abs().max() > 0)


# ----------------------------------------------------------------------------- ASDQE training
@functools.lru_cache(maxsize=None)
def _at():
    m = DenoiseRatePredictor()
    load_hash_weights(m)
    m = m.to(DEV).train()
    return m, AsdqeTrainEngine(m, torch.device(DEV))


class ATStep(Call):
    """asdqe_train_forward + asdqe_train_backward on one workspace; outputs score, grad.  The running statistics
    are in/out: every run starts from the same copy, and `stats` after the last run is kept for comparison."""

    def __init__(self, B, H, W, masks, accumulate=0):
        self.m, self.eng = _at()
        self.shape, self.accumulate = (B, H, W), accumulate
        self.theta = self.eng.flatten(self.m.parameters())
        self.stats0 = self.eng.flatten_stats(self.m)
        self.stats = self.stats0.clone()
        self.lq = _images(f"ws:at:lq:{B}x{H}x{W}", (B, 3, H, W))
        self.gt = _images(f"ws:at:gt:{B}x{H}x{W}", (B, 3, H, W))
        self.m1 = (_images("ws:at:m1", (B, 256)) >= 0.5).float() * 2.0 if masks else None
        self.m2 = (_images("ws:at:m2", (B, 64)) >= 0.3).float() * (1.0 / 0.7) if masks else None
        self.dscore = _signed("ws:at:dscore", (B, 1), 1.0)
        self.out_numels = (B, self.eng.numel)
        self.ws_bytes = int(_lib.lib().asdqe_train_workspace_bytes(self.eng.handle, B, H, W))
        self.operands = {"theta": self.theta, "lq": self.lq, "gt": self.gt, "m1": self.m1, "m2": self.m2,
                         "dscore": self.dscore}

    def prepare(self):
        self.stats.copy_(self.stats0)

    def steps(self, arena):
        L, h = _lib.lib(), self.eng.handle
        B, H, W = self.shape
        score, grad = arena.outs
        return [("asdqe_train_forward", lambda nbytes: L.asdqe_train_forward(
                    h, vp(self.theta), vp(self.stats), vp(self.lq), vp(self.gt), B, H, W, vp(self.m1), vp(self.m2),
                    vp(score), vp(arena.ws), nbytes, stream())),
                ("asdqe_train_backward", lambda nbytes: L.asdqe_train_backward(
                    h, vp(self.theta), vp(self.dscore), vp(grad), self.accumulate, vp(arena.ws), nbytes, stream()))]

    def reference(self):
        stats = self.stats0.clone()
        score = self.eng.forward(self.theta, stats, self.lq, self.gt, self.m1, self.m2)
        grad = torch.full((self.eng.numel,), float("nan"), device=DEV)
        self.eng.backward(self.theta, self.dscore, grad, accumulate=False)
        torch.cuda.synchronize()
        return [score, grad], stats


@pytest.mark.parametrize("masks", [True, False], ids=["masks", "nomasks"])
def test_asdqe_train_exact_fit(masks):
    call = ATStep(2, 40, 56, masks)
    check_exact_fit(call)
    assert not same_bits(call.stats, call.stats0)    # the running statistics did move


@pytest.mark.parametrize("masks", [True, False], ids=["masks", "nomasks"])
def test_asdqe_train_scratch_independence_and_grad_overwritten(masks):
    call = ATStep(2, 40, 56, masks)
    ref, stats = call.reference()
    score, grad = check_scratch_independence(call, ref)
    assert same_bits(call.stats, stats)
    _grad_checks(call.eng, grad)
    assert bool(grad.abs().max() > 0)


@pytest.mark.parametrize("masks", [True, False], ids=["masks", "nomasks"])
def test_asdqe_train_backward_accumulates_with_one_add(masks):
    """accumulate=1 is grad_commit's out = out + x: g0 + g, one fp32 add per element, g the accumulate=0 result."""
    plain = ATStep(2, 40, 56, masks)
    arena = Arena(plain.out_numels, plain.ws_bytes)
    arena.fill(ONES)
    _, g = plain.run(arena)
    acc = ATStep(2, 40, 56, masks, accumulate=1)
    g0 = _signed("ws:at:g0", (acc.eng.numel,), 1e-3)
    arena.fill(ONES)
    arena.outs[1].copy_(g0)
    _, got = acc.run(arena)
    arena.assert_guards("accumulate")
    assert same_bits(got, g0 + g)
    assert not same_bits(got, g)
