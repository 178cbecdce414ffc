"""The three training workspace queries that are host code (kdlae_tt_, kdlae_st_, asdqe_train_workspace_bytes):
positive, a multiple of the workspace alignment include/kdlae.h documents (256 bytes), the same on a repeated
query, and never smaller for more images or a larger frame.  No GPU here; tests/test_workspace_gpu.py runs the
engines inside exactly these sizes."""
import ctypes

import pytest

from rethink_acoustic_image_enhancement_amd import _lib
from rethink_acoustic_image_enhancement_amd.ASDQE_model import DenoiseRatePredictor
from rethink_acoustic_image_enhancement_amd.KDLAE_model import KDLAE_student, KDLAE_teacher

ALIGN = 256   # include/kdlae.h, "Workspace contract"
BATCHES = (1, 2, 3, 8)
# Chains of nested shapes: each shape contains the one before it on both axes, and every H, W is a multiple of 8
# (all three models take them).  The KDLAE-S plan keeps a forward column matrix for each Conv3d whose level is not
# a multiple of 16 wide and none for one that is (kdlae_st.cpp, conv_direct), so a wider frame can need LESS than a
# narrower one across that switch: 8 x 16 needs less than 8 x 8 with hidden [16, 32, 64].  That is the kernel
# choice, not a sizing error, so "never smaller for a larger frame" is asked within one choice: a chain whose
# widths are 8 times an odd number (no level of any model here is a multiple of 16 wide) and a chain whose widths
# are multiples of 128 (every level of up to three poolings is).
CHAINS = (((8, 8), (8, 24), (16, 24), (24, 40), (40, 56), (64, 72), (64, 136), (128, 136)),
          ((8, 128), (16, 128), (24, 128), (24, 256), (64, 256)))
NESTED = tuple(s for chain in CHAINS for s in chain)

TEACHERS = {
    "default": dict(dim=48, LayerNorm_type="BiasFree", num_blocks=[2, 1, 1, 1], num_refinement_blocks=1),
    "dim16": dict(dim=16, bias=True, num_blocks=[1, 1, 1, 1], num_refinement_blocks=1),
    "plus_nosr": dict(dim=16, num_blocks=[1, 1, 1, 1], num_refinement_blocks=1, static="no", params="plus"),
}
STUDENTS = {
    "s3": dict(residual=True, hidden_channels=[16, 32, 64]),
    "s4": dict(residual=False, hidden_channels=[8, 16, 16, 32]),
}


def _handle(create, destroy, cfg):
    h = ctypes.c_void_p()
    _lib.check(create(ctypes.byref(cfg), 0, ctypes.byref(h)), "create")
    return h, destroy


def _queries():
    """(id, handle factory, query(handle, B, H, W))"""
    L = _lib.lib()
    out = []
    for name, kw in TEACHERS.items():
        out.append((f"tt-{name}", lambda kw=kw: _handle(L.kdlae_tt_create, L.kdlae_tt_destroy, KDLAE_teacher(**kw)._c_config()),
                    lambda h, B, H, W: L.kdlae_tt_workspace_bytes(h, B, H, W)))
    for name, kw in STUDENTS.items():
        for F in (1, 3, 4):
            out.append((f"st-{name}-F{F}",
                        lambda kw=kw: _handle(L.kdlae_st_create, L.kdlae_st_destroy, KDLAE_student(**kw)._c_config()),
                        lambda h, B, H, W, F=F: L.kdlae_st_workspace_bytes(h, B, F, H, W)))
    for dim in (16, 32):
        out.append((f"asdqe-dim{dim}", lambda dim=dim: _handle(L.asdqe_train_create, L.asdqe_train_destroy,
                                                               DenoiseRatePredictor(dim=dim)._c_config()),
                    lambda h, B, H, W: L.asdqe_train_workspace_bytes(h, B, H, W)))
    return out


QUERIES = _queries()


@pytest.mark.parametrize("make,query", [q[1:] for q in QUERIES], ids=[q[0] for q in QUERIES])
def test_training_workspace_query(make, query):
    h, destroy = make()
    try:
        sizes = {}
        for H, W in NESTED:
            for B in BATCHES:
                n = query(h, B, H, W)
                assert n > 0, (B, H, W, _lib.last_error())
                assert n % ALIGN == 0, (B, H, W, n)
                sizes[B, H, W] = n
        for key, n in sizes.items():     # a repeated query, after every other shape went through the handle
            assert query(h, *key) == n, key
        for H, W in NESTED:              # more images never need less
            per_b = [sizes[B, H, W] for B in BATCHES]
            assert per_b == sorted(per_b), (H, W, per_b)
        for B in BATCHES:                # a frame that contains another never needs less (see CHAINS)
            for shapes in CHAINS:
                chain = [sizes[B, H, W] for H, W in shapes]
                assert chain == sorted(chain), (B, chain)
                assert chain[-1] > chain[0]
    finally:
        destroy(h)


def test_asdqe_ragged_sizes_take_the_padded_frames_workspace():
    """ASDQE pads to a multiple of dim: 37 x 50 and 40 x 56 (the pinned-size test's shape) are both 48 x 64."""
    L = _lib.lib()
    h, destroy = _handle(L.asdqe_train_create, L.asdqe_train_destroy, DenoiseRatePredictor()._c_config())
    try:
        n = L.asdqe_train_workspace_bytes(h, 2, 48, 64)
        assert n > 0 and n % ALIGN == 0
        assert L.asdqe_train_workspace_bytes(h, 2, 37, 50) == n
        assert L.asdqe_train_workspace_bytes(h, 2, 40, 56) == n
        assert L.asdqe_train_workspace_bytes(h, 2, 33, 49) == n
        assert L.asdqe_train_workspace_bytes(h, 2, 32, 48) < n
    finally:
        destroy(h)
