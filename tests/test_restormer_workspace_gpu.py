"""The workspace contract of include/kdlae.h on the plain-Restormer handles (kdlae_t_create_restormer /
kdlae_tt_create_restormer), with the guarded, poisoned workspaces of tests/workspace_harness.py: exact fit,
independence of the scratch contents, gradients overwritten, a small call after a large one."""
import functools

import pytest
import torch

from rethink_acoustic_image_enhancement_amd import _lib
from rethink_acoustic_image_enhancement_amd.hashweights import hash_images, load_hash_weights
from rethink_acoustic_image_enhancement_amd.KDLAE_model import Restormer
from rethink_acoustic_image_enhancement_amd.train import RestormerTrainEngine
from tests.workspace_harness import (DEV, Call, bits, check_exact_fit, check_scratch_independence,
                                     check_small_after_large, stream, vp)

pytestmark = pytest.mark.gpu

CONFIGS = {
    "dim48": dict(dim=48, LayerNorm_type="BiasFree", num_blocks=[2, 1, 1, 1], num_refinement_blocks=1),
    "dim16": dict(dim=16, bias=True, num_blocks=[1, 1, 1, 1], num_refinement_blocks=1),      # the unfused paths
}
# 24 x 16: H != W, W % 16 == 0 (strip Gram); 16 x 24: W % 16 != 0 (generic Gram partition), three images;
# 64 x 64: every fused C = 48 / 96 kernel applies
SHAPES = [(1, 24, 16), (3, 16, 24), (1, 64, 64)]


def _images(key, shape, lo=0.0, hi=1.0):
    return torch.from_numpy(hash_images(key, shape, lo, hi)).to(DEV)


@functools.lru_cache(maxsize=None)
def _model(name):
    m = Restormer(**CONFIGS[name])
    load_hash_weights(m)
    m.hip_graphs = False
    return m.to(DEV).eval()


class RForward(Call):
    """kdlae_t_forward on a Restormer handle: one output, rate and sr NULL"""

    def __init__(self, m, B, H, W):
        self.m, self.shape = m, (B, H, W)
        c = m._cfg
        self.eng = m.engine(DEV)
        self.eng.sync_params(m, stream().value or 0)
        self.img = _images(f"ws:r:img:{B}x{H}x{W}", (B, c["inp_channels"], H, W))
        self.out_numels = (B * c["out_channels"] * H * W,)
        self.ws_bytes = _lib.lib().kdlae_t_workspace_bytes(self.eng.handle, B, H, W)
        self.operands = {"img": self.img, "params": self.eng.flat}

    def steps(self, arena):
        B, H, W = self.shape
        return [("kdlae_t_forward", lambda nbytes: _lib.lib().kdlae_t_forward(
            self.eng.handle, vp(self.img), None, B, H, W, vp(arena.outs[0]), None, vp(arena.ws), nbytes, stream()))]

    def reference(self):
        with torch.no_grad():
            out = self.m(self.img)
        torch.cuda.synchronize()
        return [out]


CASES = [(n, s) for n in CONFIGS for s in SHAPES]
IDS = [f"{n}-{s[0]}x{s[1]}x{s[2]}" for n, s in CASES]


@pytest.mark.parametrize("name,shape", CASES, ids=IDS)
def test_forward_exact_fit(name, shape):
    check_exact_fit(RForward(_model(name), *shape))


@pytest.mark.parametrize("name,shape", CASES, ids=IDS)
def test_forward_scratch_independence(name, shape):
    call = RForward(_model(name), *shape)
    check_scratch_independence(call, call.reference())


def test_forward_small_after_large():
    m = _model("dim48")
    check_small_after_large(RForward(m, 2, 40, 48), RForward(m, 1, 24, 16))


# ----------------------------------------------------------------------------- training
@functools.lru_cache(maxsize=None)
def _tt(name):
    m = Restormer(**CONFIGS[name])
    load_hash_weights(m)
    m = m.to(DEV)
    return m, RestormerTrainEngine(m, torch.device(DEV))


class RStep(Call):
    """kdlae_tt_forward + kdlae_tt_backward (or _marked) on a Restormer handle; outputs out, grad"""

    def __init__(self, name, B, H, W, marked=False):
        self.m, self.eng = _tt(name)
        c = self.m._cfg
        self.shape, self.marked = (B, H, W), marked
        self.theta = self.eng.flatten(self.m.parameters())
        self.img = _images(f"ws:rt:img:{B}x{H}x{W}", (B, c["inp_channels"], H, W))
        n = B * c["out_channels"] * H * W
        self.dhq = _images(f"ws:rt:dhq:{B}x{H}x{W}", (n,), -1.0 / n, 1.0 / n)
        self.out_numels = (n, self.eng.numel)
        self.ws_bytes = int(_lib.lib().kdlae_tt_workspace_bytes(self.eng.handle, B, H, W))
        self.operands = {"theta": self.theta, "img": self.img, "dhq": self.dhq}

    def steps(self, arena):
        L, h = _lib.lib(), self.eng.handle
        B, H, W = self.shape
        out, grad = arena.outs
        bwd_name = "kdlae_tt_backward_marked" if self.marked else "kdlae_tt_backward"
        bwd = getattr(L, bwd_name)
        return [("kdlae_tt_forward", lambda nbytes: L.kdlae_tt_forward(
                    h, vp(self.theta), vp(self.img), None, B, H, W, vp(out), None, vp(arena.ws), nbytes, stream())),
                (bwd_name, lambda nbytes: bwd(h, vp(self.theta), vp(self.dhq), None, vp(grad), vp(arena.ws), nbytes,
                                              stream()))]

    def reference(self):
        out, _ = self.eng.forward(self.theta, self.img, None)
        grad = torch.full((self.eng.numel,), float("nan"), device=DEV)
        self.eng.backward(self.theta, self.dhq, None, grad, marked=self.marked)
        torch.cuda.synchronize()
        return [out, grad]


TT_SHAPES = {"dim16": (2, 48, 40), "dim48": (2, 32, 32)}
TT_CASES = [(name, marked) for name in CONFIGS for marked in (False, True)]
TT_IDS = [f"{name}-{'marked' if marked else 'plain'}" for name, marked in TT_CASES]


@pytest.mark.parametrize("name,marked", TT_CASES, ids=TT_IDS)
def test_step_exact_fit(name, marked):
    check_exact_fit(RStep(name, *TT_SHAPES[name], marked=marked))


@pytest.mark.parametrize("name,marked", TT_CASES, ids=TT_IDS)
def test_step_scratch_independence_and_grad_overwritten(name, marked):
    call = RStep(name, *TT_SHAPES[name], marked=marked)
    out, grad = check_scratch_independence(call, call.reference())
    assert bool(torch.isfinite(grad).all()), "grad was accumulated into, or only partly written"
    pad = torch.ones(call.eng.numel, dtype=torch.bool, device=grad.device)
    for k, n, off in call.eng.keys:
        pad[off:off + n] = False
        assert bool(grad[off:off + n].abs().max() > 0), k
    assert bool((bits(grad)[pad] == 0).all()), "a pad float between keys is not +0.0"


def test_step_small_after_large():
    check_small_after_large(RStep("dim16", 3, 16, 24), RStep("dim16", 1, 16, 24))
