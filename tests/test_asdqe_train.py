"""ASDQE training, CPU side: the tests' restatement (tests/asdqe_train_oracle.py) against the goldens
recorded from the imported reference (tests/golden/atrain_*.npz), and the training handle's parameter
layout.  No GPU call: the handle's enumeration and its workspace query are host code."""
import ctypes
import json

import numpy as np
import pytest
import torch

from oracle.asdqe_oracle import AsdqeCfg, asdqe_param_shapes
from rethink_acoustic_image_enhancement_amd import _lib
from rethink_acoustic_image_enhancement_amd.ASDQE_model import DenoiseRatePredictor
from tests.asdqe_train_oracle import CASES, SMALL, SUB, case_tensors, packed, param_keys, train_step
from tests.util import GOLDEN, hash_sd_for, load_fixture


def _load(name):
    d, kw = load_fixture(name)
    keys = json.loads(bytes(d["param_keys"]).decode())
    bkeys = json.loads(bytes(d["buffer_keys"]).decode())
    return d, kw, keys, bkeys


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_reproduces_reference_fp64(name):
    d, kw, keys, bkeys = _load(name)
    kw0, shape, use_masks = CASES[name]
    assert kw == kw0 and tuple(d["shape"]) == shape and int(d["use_masks"]) == int(use_masks)
    cfg = AsdqeCfg(**kw)
    assert keys == param_keys(cfg)
    lq, gt, target, m1, m2 = case_tensors(name, shape, int(d["suffix"]), use_masks)
    r = train_step(hash_sd_for(asdqe_param_shapes(cfg)), lq, gt, target, cfg, m1, m2, dtype=torch.float64)
    e_loss = abs(float(r["loss"]) - float(d["loss64"]))
    e_score = float(np.abs(r["score"].numpy() - d["score64"]).max())
    gmax = float(d["key_stats64"][:, 2].max())
    e_grad = float(np.abs(packed(r["grads"], keys)[::SUB].numpy() - d["grad_sub64"]).max())
    e_small = max(float(np.abs(r["grads"][k].numpy() - d["g:" + k]).max()) for k in keys
                  if r["grads"][k].numel() <= SMALL)
    e_buf = float(np.abs(torch.cat([r["buffers"][k] for k in bkeys]).numpy() - d["buffers64"]).max())
    print(f"{name}: loss {e_loss:.2e} score {e_score:.2e} grad {e_grad:.2e} small {e_small:.2e} "
          f"(max |g| {gmax:.2e}) buffers {e_buf:.2e}")
    assert e_loss <= 1e-9 and e_score <= 1e-9
    assert e_grad <= 1e-9 * gmax and e_small <= 1e-9 * gmax
    assert e_buf <= 1e-12
    stats = np.array([[float(r["grads"][k].sum()), float(r["grads"][k].abs().sum()), float(r["grads"][k].abs().max())]
                      for k in keys])
    assert np.abs(stats - d["key_stats64"]).max() <= 1e-9 * max(1.0, float(d["key_stats64"][:, 1].max()))


def test_goldens_are_small_and_conditioned():
    import os
    for name in CASES:
        assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) < 1_000_000
        d, kw, keys, _ = _load(name)
        from tests.asdqe_train_oracle import bn_fed_bias_keys
        zero = bn_fed_bias_keys(AsdqeCfg(**kw))
        assert len(zero) == 20
        live = [k not in zero for k in keys]
        assert d["e32"][live].max() <= 2e-4  # the generator's conditioning gate (the reference's own fp32 error)
        assert d["probe"][live].max() <= 1e-3  # ... and its three robustness probes


def _handle(kw):
    L = _lib.lib()
    cfg = _lib.AConfig()
    cfg.in_channels, cfg.dim = kw.get("in_channels", 3), kw.get("dim", 16)
    h = ctypes.c_void_p()
    _lib.check(L.asdqe_train_create(ctypes.byref(cfg), 0, ctypes.byref(h)), "asdqe_train_create")
    return L, h


@pytest.mark.parametrize("kw", [dict(), dict(in_channels=1, dim=32), dict(in_channels=2), dict(in_channels=4)])
def test_handle_layout_matches_named_parameters(kw):
    L, h = _handle(kw)
    try:
        m = DenoiseRatePredictor(**kw)
        named = list(m.named_parameters())
        assert L.asdqe_train_num_params(h) == len(named)
        end = 0
        for i, (k, p) in enumerate(named):
            name, numel, off = ctypes.c_char_p(), ctypes.c_int64(), ctypes.c_int64()
            _lib.check(L.asdqe_train_param_info(h, i, ctypes.byref(name), ctypes.byref(numel), ctypes.byref(off)), "info")
            assert name.value.decode() == k and numel.value == p.numel()
            assert off.value % 4 == 0 and off.value == end  # 16-byte aligned, back to back
            end = off.value + (p.numel() + 3) // 4 * 4
        assert L.asdqe_train_num_floats(h) == end
        bns = [x for x in m.modules() if isinstance(x, torch.nn.BatchNorm2d)]
        assert L.asdqe_train_num_stat_floats(h) == sum(2 * b.num_features for b in bns)
        assert [k for k, _ in named] == param_keys(AsdqeCfg(**m._cfg))
    finally:
        L.asdqe_train_destroy(h)


def test_workspace_bytes_positive_and_monotone_and_refuses_unindexable():
    L, h = _handle(dict())
    try:
        sizes = [L.asdqe_train_workspace_bytes(h, B, 40, 56) for B in (1, 2, 3, 8)]
        assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:]))
        assert L.asdqe_train_workspace_bytes(h, 0, 40, 56) < 0
        # 128 x 512^2 padded pixels x 128 channels passes 2^31 elements: refused before anything launches
        assert L.asdqe_train_workspace_bytes(h, 128, 512, 512) < 0
        assert "2^31" in _lib.last_error()
        assert L.asdqe_train_workspace_bytes(h, 32, 512, 512) > 0  # the reference's own micro-batch
    finally:
        L.asdqe_train_destroy(h)


def test_bad_config_is_refused():
    L = _lib.lib()
    cfg = _lib.AConfig()
    cfg.in_channels, cfg.dim = 3, 24
    h = ctypes.c_void_p()
    assert L.asdqe_train_create(ctypes.byref(cfg), 0, ctypes.byref(h)) == 2


def test_null_handle_and_null_argument_returns():
    """What every asdqe_train_* entry answers without a device: return value, KDLAE_E* code, error text."""
    from tests.util import FAKE, failed, silent
    L, h = _handle(dict())
    try:
        cfg = _lib.AConfig()
        cfg.in_channels, cfg.dim = 3, 16
        failed(L.asdqe_train_create(None, 0, ctypes.byref(h)), 6, "null argument")
        failed(L.asdqe_train_create(ctypes.byref(cfg), 0, None), 6, "null argument")
        silent(lambda: L.asdqe_train_destroy(None), 0)
        silent(lambda: L.asdqe_train_num_params(None), -1)
        silent(lambda: L.asdqe_train_num_floats(None), -1)
        silent(lambda: L.asdqe_train_num_stat_floats(None), -1)
        silent(lambda: L.asdqe_train_workspace_bytes(None, 2, 40, 56), -1)
        failed(L.asdqe_train_param_info(None, 0, None, None, None), 4, "param index out of range")
        failed(L.asdqe_train_param_info(h, L.asdqe_train_num_params(h), None, None, None), 4,
               "param index out of range")
        big = 1 << 40
        fwd = lambda a, B=2, ws_bytes=0: L.asdqe_train_forward(h, a[0], a[1], a[2], a[3], B, 40, 56, None, None,
                                                               a[4], a[5], ws_bytes, None)
        failed(L.asdqe_train_forward(None, FAKE, FAKE, FAKE, FAKE, 2, 40, 56, None, None, FAKE, FAKE, 0, None), 6,
               "null argument")
        failed(L.asdqe_train_backward(None, FAKE, FAKE, FAKE, 0, FAKE, 0, None), 6, "null argument")
        for miss in range(6):  # theta, stats, lq, gt, score, workspace
            a = [FAKE] * 6
            a[miss] = None
            failed(fwd(a), 6, "null argument")
        for miss in range(4):  # theta, dscore, grad, workspace
            a = [FAKE] * 4
            a[miss] = None
            failed(L.asdqe_train_backward(h, a[0], a[1], a[2], 0, a[3], 0, None), 6, "null argument")
        failed(fwd([FAKE] * 6, B=0), 1, "B, H, W must be positive")
        failed(L.asdqe_train_workspace_bytes(h, 0, 40, 56), -1, "B, H, W must be positive")
        failed(fwd([FAKE] * 6), 6, "training workspace too small")
        for miss in (0, 1, 5):
            a = [FAKE] * 6
            a[miss] = FAKE + 8
            failed(fwd(a, ws_bytes=big), 6, "theta, stats and the workspace must be 16-byte aligned")
        failed(L.asdqe_train_backward(h, FAKE, FAKE, FAKE, 0, FAKE, big, None), 6,
               "asdqe_train_backward needs a preceding asdqe_train_forward on the same workspace")
    finally:
        L.asdqe_train_destroy(h)
    cfg.dim = 24
    failed(L.asdqe_train_create(ctypes.byref(cfg), 0, ctypes.byref(h)), 2,
           "dim must be a multiple of 16 in 16..256 on the HIP path")
    assert h.value is None


# asdqe_train_workspace_bytes of commit e977bd4 (make_plan is host code) at 2 x 40 x 56: the default
# dim (16) and dim 32
@pytest.mark.parametrize("dim,want", [(16, 102514688), (32, 126239488)])
def test_workspace_bytes_pinned(dim, want):
    L, h = _handle(dict(dim=dim))
    try:
        assert L.asdqe_train_workspace_bytes(h, 2, 40, 56) == want
    finally:
        L.asdqe_train_destroy(h)
