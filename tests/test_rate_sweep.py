"""Rate sweep (kdlae_t_forward_rates, kdlae_t_forward_sr, kdlae_rate_select): what holds without a GPU.
The header declares and the library exports the entry points, every argument check that comes before
the packed parameters are needed refuses with its code and message, and the numpy model of the select
rule the GPU tests compare against agrees with the rule spelled out one score at a time."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from rethink_acoustic_image_enhancement_amd import _lib
from rethink_acoustic_image_enhancement_amd.KDLAE_model import KDLAE_teacher
from tests.rate_select_model import select_cases, select_loop, select_model
from tests.util import FAKE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("kdlae_t_rates_workspace_bytes", "kdlae_t_forward_rates", "kdlae_t_sr_workspace_bytes", "kdlae_t_forward_sr",
       "kdlae_rate_select")
P = ctypes.c_void_p(FAKE)
TINY = dict(dim=16, num_blocks=[1, 1, 1, 1], num_refinement_blocks=1)


def test_header_declares_and_library_exports_the_entry_points():
    src = open(os.path.join(ROOT, "include", "kdlae.h")).read()
    L = _lib.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert hasattr(L, name) and name in _lib.EXPORTS, name
    assert L.kdlae_abi_version() == 1
    for name in ("forward_rates", "forward_sr"):
        assert callable(getattr(KDLAE_teacher, name))


def _handle(**kw):
    h = ctypes.c_void_p()
    assert _lib.lib().kdlae_t_create(ctypes.byref(KDLAE_teacher(**{**TINY, **kw})._c_config()), 0, ctypes.byref(h)) == 0
    return h


def _rates(h, img=P, rates=P, is_map=0, B=2, R=3, H=16, W=24, hq=P, sr=P, ws=P, nbytes=1 << 40):
    return _lib.lib().kdlae_t_forward_rates(h, img, rates, is_map, B, R, H, W, hq, sr, ws, nbytes, None)


def test_forward_rates_argument_checks_need_no_launch():
    L = _lib.lib()
    h = _handle()
    assert _rates(None) == 6 and "null handle" in _lib.last_error()
    for kw in (dict(img=None), dict(rates=None), dict(hq=None)):
        assert _rates(h, **kw) == 6 and "required" in _lib.last_error()
    assert _rates(h, is_map=2) == 2 and "rate_is_map" in _lib.last_error()
    for R in (0, 65, -1):
        assert _rates(h, R=R) == 1 and "1 <= R <= 64" in _lib.last_error()
        assert L.kdlae_t_rates_workspace_bytes(h, 2, R, 16, 24, 1) == -1 and "1 <= R <= 64" in _lib.last_error()
    for kw in (dict(H=20), dict(W=12), dict(B=0), dict(H=0)):
        assert _rates(h, **kw) == 1 and "H % 8" in _lib.last_error()
    assert L.kdlae_t_rates_workspace_bytes(h, 2, 3, 20, 24, 0) == -1 and "H % 8" in _lib.last_error()
    # every argument is fine: what is missing is the packed parameters
    assert _rates(h) == 6 and "before kdlae_t_commit_params" in _lib.last_error()
    assert L.kdlae_t_rates_workspace_bytes(h, 2, 3, 16, 24, 1) == -1 and "committed" in _lib.last_error()
    L.kdlae_t_destroy(h)


def test_forward_rates_config_refusals():
    L = _lib.lib()
    h = _handle(params="plus")
    assert _rates(h) == 2 and "params=='cat'" in _lib.last_error()
    assert L.kdlae_t_rates_workspace_bytes(h, 2, 3, 16, 24, 0) == -1 and "params=='cat'" in _lib.last_error()
    L.kdlae_t_destroy(h)
    h = _handle(static="no")
    assert _rates(h) == 2 and "no sr head" in _lib.last_error()
    assert L.kdlae_t_rates_workspace_bytes(h, 2, 3, 16, 24, 1) == -1 and "no sr head" in _lib.last_error()
    assert _rates(h, sr=None) == 6 and "before kdlae_t_commit_params" in _lib.last_error()   # sr = NULL is allowed
    assert L.kdlae_t_forward_sr(h, P, 2, 16, 24, P, P, 1 << 40, None) == 2 and "no sr head" in _lib.last_error()
    assert L.kdlae_t_sr_workspace_bytes(h, 2, 16, 24) == -1
    L.kdlae_t_destroy(h)


def test_forward_sr_argument_checks_need_no_launch():
    L = _lib.lib()
    h = _handle()
    assert L.kdlae_t_forward_sr(None, P, 2, 16, 24, P, P, 1 << 40, None) == 6
    assert L.kdlae_t_forward_sr(h, None, 2, 16, 24, P, P, 1 << 40, None) == 6 and "required" in _lib.last_error()
    assert L.kdlae_t_forward_sr(h, P, 2, 16, 24, None, P, 1 << 40, None) == 6 and "required" in _lib.last_error()
    assert L.kdlae_t_forward_sr(h, P, 2, 12, 24, P, P, 1 << 40, None) == 1 and "H % 8" in _lib.last_error()
    assert L.kdlae_t_forward_sr(h, P, 2, 16, 24, P, P, 1 << 40, None) == 6
    assert "before kdlae_t_commit_params" in _lib.last_error()
    assert L.kdlae_t_sr_workspace_bytes(h, 2, 16, 24) == -1 and "committed" in _lib.last_error()
    L.kdlae_t_destroy(h)


def _select(scores=P, R=3, B=2, mode=0, target=P, hq=P, per_image=7, index=P, out=P):
    return _lib.lib().kdlae_rate_select(scores, R, B, mode, target, hq, per_image, index, out, None)


def test_rate_select_argument_checks_need_no_launch():
    for kw in (dict(scores=None), dict(hq=None), dict(index=None), dict(out=None)):
        assert _select(**kw) == 2 and "null argument" in _lib.last_error()
    for mode in (-1, 3):
        assert _select(mode=mode) == 2 and "mode must be" in _lib.last_error()
    assert _select(target=None) == 2 and "needs a target" in _lib.last_error()
    for kw in (dict(R=0), dict(B=0), dict(per_image=0), dict(R=-2)):
        assert _select(**kw) == 2 and "R >= 1" in _lib.last_error()


def test_module_refusals_without_a_device():
    m = KDLAE_teacher(**TINY).eval()
    img = torch.zeros(1, 3, 16, 24)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.forward_rates(img, [0.1, 0.2])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.forward_sr(img)
    m.train()
    with pytest.raises(RuntimeError, match="eval"):
        m.forward_rates(img, [0.1, 0.2])
    with pytest.raises(RuntimeError, match="eval"):
        m.forward_sr(img)


@pytest.mark.parametrize("R,B", [(1, 1), (1, 5), (3, 1), (3, 5), (64, 1), (64, 5), (7, 33)])
def test_numpy_select_model_equals_the_rule_spelled_out(R, B):
    for seed in range(3):
        for name, scores, target in select_cases(R, B, seed):
            for mode in (0, 1, 2):
                got, want = select_model(scores, mode, target), select_loop(scores, mode, target)
                assert got.dtype == np.int32 and np.array_equal(got, want), (name, mode)


def test_numpy_select_model_on_hand_cases():
    nan, inf = np.nan, np.inf
    s = np.array([[0.75, nan, nan, -0.0, nan], [0.25, nan, 2.0, 0.0, inf], [0.25, nan, 2.0, -0.0, inf]], np.float32)
    t = np.full(5, 0.5, np.float32)
    assert select_model(s, 0, t).tolist() == [0, 0, 1, 0, 1]   # midway tie -> lowest r; all NaN -> 0; NaN skipped
    assert select_model(s, 1).tolist() == [0, 0, 1, 0, 1]      # +0 == -0: a tie
    assert select_model(s, 2).tolist() == [1, 0, 1, 0, 1]
