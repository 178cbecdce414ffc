"""Fine-tuning with frozen parameters on the HIP training path (kdlae_tt_set_trainable), on the tiny configs of the
train_* goldens.

Under every mask: hq / sr have the bits of the all-trainable forward; the trainable ranges of `grad` have the bits
of the all-trainable backward (which is deterministic); frozen ranges and pad floats are +0.0; a second run gives
the same bits; the same with dsr = None.  The backward's launch count falls with the regime, the workspace contract
holds in a guarded exact-fit workspace, the trainer leaves frozen weights and moments alone, and the drop-in returns
None for frozen parameters.  All comparisons are of bits, except the drop-in's gradients against the CPU oracle
(the 2e-3 per-key rule of tests/test_train_gpu.py)."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

from oracle.kdlae_oracle import TeacherCfg, teacher_param_shapes
from oracle.train_oracle import loss_and_grads
from rethink_acoustic_image_enhancement_amd import _lib
from rethink_acoustic_image_enhancement_amd.hashweights import hash_images, load_hash_weights
from rethink_acoustic_image_enhancement_amd.KDLAE_model import KDLAE_teacher
from rethink_acoustic_image_enhancement_amd.train import (KDLAETrainer, L1LossSr, TrainEngine,
                                                           freeze_except_patch_embed_and_enhance)
from tests.util import GOLDEN, hash_sd_for
from tests.workspace_harness import Call, bits, check_exact_fit, check_scratch_independence, same_bits, stream, vp

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
CASES = ("train_tiny_biasfree", "train_tiny_withbias", "train_nocat_nosr")
ESTATE = 6
SR = ("cen.", "upen.", "enhance.", "outputen.")
TAIL = ("output_param.", "refinement_out.", "output2.")
# single keys in forward order (the last one: a temperature late in the decoder)
SINGLE = ("encoder_level1.0.norm1.body.weight", "latent.0.ffn.project_out.weight",
          "decoder_level2.0.attn.qkv_dwconv.weight", "decoder_level1.0.attn.temperature")


def _cfg(name):
    d = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    return json.loads(bytes(d["cfg"]).decode())


def _has(name):
    c = _cfg(name)
    return c.get("static", "train") == "train", c.get("params", "cat") == "cat"


def masks_for(name):
    """mask id -> predicate over key names, for the masks that apply to this config"""
    has_sr, has_cat = _has(name)
    m = {"ones": lambda k: True,
         "reference": lambda k: k.startswith(("patch_embed.",) + (SR if has_sr else ())),
         "every_second": None,          # by index, below
         "all_but_patch_embed": lambda k: k != "patch_embed.proj.weight"}
    if has_sr:
        m["sr_head"] = lambda k: k.startswith(SR)
    if has_cat:
        m["rate_tail"] = lambda k: k.startswith(TAIL)
    for key in SINGLE:
        m["only:" + key] = lambda k, key=key: k == key
    return m


MASK_CASES = [(n, mid) for n in CASES for mid in masks_for(n)]


@functools.lru_cache(maxsize=None)
def _case(name):
    """model, operands and the all-trainable (NULL mask) results: computed once, never written afterwards"""
    d = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    cfg = _cfg(name)
    m = KDLAE_teacher(**cfg)
    load_hash_weights(m)
    m = m.to(DEV)
    eng = TrainEngine(m, DEV)
    img, rate = torch.from_numpy(d["img"]).to(DEV), torch.from_numpy(d["rate"]).to(DEV)
    B, _, H, W = img.shape
    n = B * cfg.get("out_channels", 3) * H * W
    lo = lambda key, shape, s: torch.from_numpy(hash_images(key, shape, -s, s)).to(DEV)   # noqa: E731
    c = dict(name=name, model=m, names=[k for k, _, _ in eng.keys], keys=eng.keys, numel=eng.numel,
             theta=eng.flatten(m.parameters()), img=img, rate=rate, shape=(B, H, W), has_sr=eng.static_train,
             dhq=lo("ft:dhq:" + name, (B, n // B // H // W, H, W), 1.0 / n),
             dsr=lo("ft:dsr:" + name, (B, n // B // H // W, 2 * H, 2 * W), 0.25 / n) if eng.static_train else None)
    c["full"] = _run(eng, c, None, True)
    c["full_nodsr"] = _run(eng, c, None, False)
    return c


def _mask(c, mid):
    pred = masks_for(c["name"])[mid]
    if pred is None:
        return [i % 2 == 0 for i in range(len(c["names"]))]
    return [bool(pred(k)) for k in c["names"]]


def _run(eng, c, mask, with_dsr):
    """forward + backward under `mask` on a NaN-prefilled grad -> (hq, sr, grad, backward launches)"""
    if mask != eng.trainable and not (mask is None and all(eng.trainable)):
        eng.set_trainable(mask)
    hq, sr = eng.forward(c["theta"], c["img"], c["rate"])
    grad = torch.full((c["numel"],), float("nan"), device=DEV)
    eng.backward(c["theta"], c["dhq"], c["dsr"] if with_dsr else None, grad)
    torch.cuda.synchronize()
    return hq, sr, grad, eng.backward_launches()


def _expected_grad(c, mask, full_grad):
    """the all-trainable gradient on the trainable keys, +0.0 everywhere else (frozen keys and pad floats)"""
    want = torch.zeros_like(full_grad)
    for (k, n, off), t in zip(c["keys"], mask):
        if t:
            want[off:off + n] = full_grad[off:off + n]
    return want


@pytest.mark.parametrize("name,mid", MASK_CASES, ids=[f"{n}-{m}" for n, m in MASK_CASES])
def test_masked_step_has_the_all_trainable_bits(name, mid):
    c = _case(name)
    mask = _mask(c, mid)
    eng = TrainEngine(c["model"], DEV)
    for with_dsr, base in ((True, c["full"]), (False, c["full_nodsr"])):
        want = _expected_grad(c, mask, base[2])
        runs = [_run(eng, c, mask, with_dsr) for _ in range(2)]
        for hq, sr, grad, _ in runs:
            assert same_bits(hq, base[0]), "hq differs from the all-trainable forward's"
            assert (sr is None and base[1] is None) or same_bits(sr, base[1]), "sr differs"
            assert bool(torch.isfinite(grad).all())
            if not same_bits(grad, want):
                bad = (bits(grad) != bits(want)).nonzero().view(-1)
                i = int(bad[0])
                key = [k for k, n, off in c["keys"] if off <= i < off + ((n + 3) & ~3)]
                raise AssertionError(f"dsr={with_dsr}: {bad.numel()} floats differ, first at {i} in {key}: "
                                     f"{float(grad[i])} vs {float(want[i])}")
        assert runs[0][3] == runs[1][3]
    assert [bool(eng._L.kdlae_tt_is_trainable(eng.handle, i)) for i in range(len(mask))] == mask


@pytest.mark.parametrize("name", CASES)
def test_backward_launch_counts_fall_with_the_regime(name):
    c = _case(name)
    has_sr, has_cat = _has(name)
    eng = TrainEngine(c["model"], DEV)
    n = {mid: _run(eng, c, _mask(c, mid), True)[3] for mid in masks_for(name)}
    print(name, "backward launches:", {"null": c["full"][3], **n})
    assert n["ones"] == c["full"][3]                      # all ones takes the NULL mask's launches
    assert n["ones"] > n["reference"]
    if has_sr and has_cat:
        assert n["reference"] > n["rate_tail"] > n["sr_head"]
    singles = [n["only:" + k] for k in SINGLE]            # a later key never costs more launches
    assert all(a >= b for a, b in zip(singles, singles[1:])), singles
    assert n["ones"] > singles[0]
    if has_sr:
        # only sr-head keys trainable and no dsr: the backward is the zero fill of grad
        hq, sr, grad, launches = _run(eng, c, _mask(c, "sr_head"), False)
        assert launches == 1 and bool((bits(grad) == 0).all())
    # only latent.0.ffn.project_out.weight: that block launches one dW GEMM and nothing else.  With only
    # up4_3.body.0.weight (the layer after `latent`) the backward is the same down to up4_3, which then launches its
    # dW GEMM; here up4_3 launches its dX instead (weight repack + GEMM) and the block adds its one GEMM: + 2
    n_up = _run(eng, c, [k == "up4_3.body.0.weight" for k in c["names"]], True)[3]
    assert n["only:latent.0.ffn.project_out.weight"] - n_up == 2, (n, n_up)


class MaskedStep(Call):
    """kdlae_tt_forward + kdlae_tt_backward under a mask on one guarded workspace; outputs hq, sr, grad"""

    def __init__(self, c, eng, mask):
        self.c, self.eng = c, eng
        eng.set_trainable(mask)
        B, H, W = c["shape"]
        n = c["dhq"].numel()
        self.out_numels = (n, 4 * n if c["has_sr"] else 0, c["numel"])
        self.ws_bytes = int(_lib.lib().kdlae_tt_workspace_bytes(eng.handle, B, H, W))
        self.operands = {k: c[k] for k in ("theta", "img", "rate", "dhq", "dsr")}

    def steps(self, arena):
        L, h, c = _lib.lib(), self.eng.handle, self.c
        B, H, W = c["shape"]
        hq, sr, grad = arena.outs
        rate = c["rate"] if self.eng.params_cat else None
        return [("kdlae_tt_forward", lambda nbytes: L.kdlae_tt_forward(
                    h, vp(c["theta"]), vp(c["img"]), vp(rate), B, H, W, vp(hq), vp(sr if c["has_sr"] else None),
                    vp(arena.ws), nbytes, stream())),
                ("kdlae_tt_backward", lambda nbytes: L.kdlae_tt_backward(
                    h, vp(c["theta"]), vp(c["dhq"]), vp(c["dsr"]), vp(grad), vp(arena.ws), nbytes, stream()))]


WS_CASES = [(n, mid) for n in CASES for mid in ("reference", "sr_head", "only:" + SINGLE[2]) if mid in masks_for(n)]


@pytest.mark.parametrize("name,mid", WS_CASES, ids=[f"{n}-{m}" for n, m in WS_CASES])
def test_masked_step_in_a_guarded_exact_fit_workspace(name, mid):
    c = _case(name)
    mask = _mask(c, mid)
    eng = TrainEngine(c["model"], DEV)
    call = MaskedStep(c, eng, mask)
    full_eng = TrainEngine(c["model"], DEV)      # (kept alive: its handle is destroyed with it)
    full_bytes = int(_lib.lib().kdlae_tt_workspace_bytes(full_eng.handle, *c["shape"]))
    assert 0 < call.ws_bytes <= full_bytes and call.ws_bytes % 256 == 0
    if mid == "sr_head":
        assert call.ws_bytes < full_bytes
    want = [c["full"][0].reshape(-1), c["full"][1].reshape(-1) if c["has_sr"] else None,
            _expected_grad(c, mask, c["full"][2])]
    arena = check_exact_fit(call)            # one byte less is refused before any launch; guards intact
    torch.cuda.synchronize()
    for got, ref in zip(arena.outs, want):
        assert ref is None or same_bits(got, ref)
    check_scratch_independence(call, want)   # zero / NaN / 1e30 poison: the same bits, the guards intact


@pytest.mark.parametrize("name", CASES[:1])
def test_setter_between_forward_and_backward_is_refused(name):
    c = _case(name)
    eng = TrainEngine(c["model"], DEV)
    L = eng._L
    eng.forward(c["theta"], c["img"], c["rate"])
    buf = (ctypes.c_ubyte * len(c["names"]))(*([1] * len(c["names"])))
    assert L.kdlae_tt_set_trainable(eng.handle, buf, len(c["names"])) == ESTATE
    assert L.kdlae_tt_set_trainable(eng.handle, None, 0) == ESTATE
    grad = torch.empty(c["numel"], device=DEV)
    eng.backward(c["theta"], c["dhq"], c["dsr"], grad)
    assert L.kdlae_tt_set_trainable(eng.handle, buf, len(c["names"])) == 0
    # a mask change invalidates the last forward: the next backward needs a new one
    rc = L.kdlae_tt_backward(eng.handle, vp(c["theta"]), vp(c["dhq"]), vp(c["dsr"]), vp(grad), vp(eng.ws),
                             eng.ws.numel(), stream())
    assert rc == ESTATE
    torch.cuda.synchronize()
    assert same_bits(grad, c["full"][2])


def _load_case(name):
    d = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    cfg, opt = _cfg(name), json.loads(bytes(d["opt"]).decode())
    keys = json.loads(bytes(d["keys"]).decode())
    img, rate = torch.from_numpy(d["img"]), torch.from_numpy(d["rate"])
    gt = {"hq": torch.from_numpy(d["gt_hq"]), "sr": torch.from_numpy(d["gt_sr"])}
    if cfg.get("static", "train") != "train":
        gt = {"hq": gt["hq"]}
    return cfg, opt, keys, img, rate, gt


def _fresh_model(cfg):
    m = KDLAE_teacher(**cfg)
    load_hash_weights(m)
    return m.to(DEV)


@pytest.mark.parametrize("name", CASES)
def test_trainer_leaves_frozen_parameters_alone(name):
    cfg, opt, keys, img, rate, gt = _load_case(name)
    kw = dict(lr=opt["lr"], weight_decay=opt["weight_decay"], betas=tuple(opt["betas"]), max_norm=opt["clip"])
    lq = {"img": img.to(DEV), "denoise_rate": rate.to(DEV)}
    gtd = {k: v.to(DEV) for k, v in gt.items()}
    tr = KDLAETrainer(freeze_except_patch_embed_and_enhance(_fresh_model(cfg)), **kw)   # mask read at construction
    mask = [p.requires_grad for p in tr.model.parameters()]
    assert tr.engine.trainable == mask and not all(mask)
    # the same sequence by hand: the all-trainable backward, frozen gradients zeroed, clip + AdamW on the ranges
    ref = KDLAETrainer(_fresh_model(cfg), **kw)
    ref._ranges, ref._nranges = tr._ranges, tr._nranges
    theta0 = tr.theta.clone()
    assert same_bits(theta0, ref.theta)
    frozen = torch.ones(tr.engine.numel, dtype=torch.bool, device=DEV)
    for (k, n, off), t in zip(tr.engine.keys, mask):
        if t:
            frozen[off:off + n] = False
    for _ in range(2):
        tr.optimize_parameters(lq, gtd)
        ref.forward_backward(lq, gtd)
        ref.grad[frozen] = 0.0
        ref.step()
        torch.cuda.synchronize()
        assert same_bits(tr.grad, ref.grad)
        assert same_bits(tr.grad_norm(), ref.grad_norm())
        norm = float(torch.linalg.vector_norm(tr.grad[~frozen].double()))
        # fp32 tree sum of squares against float64: a few ulps of the fp32 result
        assert abs(float(tr.grad_norm()) - norm) <= 1e-5 * norm
        assert norm > 0
    assert same_bits(tr.theta[frozen], theta0[frozen])
    assert bool((bits(tr.exp_avg[frozen]) == 0).all()) and bool((bits(tr.exp_avg_sq[frozen]) == 0).all())
    assert same_bits(tr.theta, ref.theta) and same_bits(tr.exp_avg, ref.exp_avg)
    assert not same_bits(tr.theta[~frozen], theta0[~frozen])
    # the state lists the trainable parameters only, in named_parameters() order, and resumes
    st = tr.training_state(0, 2)
    named = [k for k, p in tr.model.named_parameters() if p.requires_grad]
    assert st["optimizers"][0]["param_groups"][0]["params"] == list(range(len(named)))
    tr.resume_training(st)
    assert same_bits(tr.exp_avg, ref.exp_avg) and tr.step_count == 2
    with pytest.raises(ValueError, match="trainable"):
        ref.resume_training(st)
    # set_trainable by predicate: everything again
    tr.set_trainable(None)
    assert all(p.requires_grad for p in tr.model.parameters()) and all(tr.engine.trainable)
    assert list(tr._ranges) == [v for r in ref.engine.used_ranges() for v in r]


@pytest.mark.parametrize("name", CASES)
def test_dropin_after_the_reference_freeze(name):
    cfg, opt, keys, img, rate, gt = _load_case(name)
    m = _fresh_model(cfg)
    freeze_except_patch_embed_and_enhance(m)
    m.train()
    out = m({"img": img.to(DEV), "denoise_rate": rate.to(DEV)})
    loss = L1LossSr()(out, {k: v.to(DEV) for k, v in gt.items()})
    loss.backward()
    torch.cuda.synchronize()
    sd = hash_sd_for(teacher_param_shapes(TeacherCfg(**cfg)))
    loss_ref, grads_ref = loss_and_grads({k: sd[k] for k in keys}, img, rate, gt, TeacherCfg(**cfg))
    assert abs(float(loss.detach()) - float(loss_ref)) <= 1e-5 * abs(float(loss_ref))
    seen = 0
    for k, p in m.named_parameters():
        if not p.requires_grad:
            assert p.grad is None, k
            continue
        assert p.grad is not None, k
        r = grads_ref[k].double()
        err = float((p.grad.cpu().double() - r).abs().max())
        assert err <= 2e-3 * float(r.abs().max()) + 1e-8, k
        seen += 1
    assert seen > 0
    # BasicSR's optimizer over the requires_grad parameters steps them
    opt_t = torch.optim.AdamW([p for p in m.parameters() if p.requires_grad], lr=1e-3)
    torch.nn.utils.clip_grad_norm_(m.parameters(), 0.01)
    opt_t.step()
