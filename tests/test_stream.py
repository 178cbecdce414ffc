"""Streaming inference without a GPU: streams.stream_schedule against the rule (tests/stream_model.py), the
refusals of the Python entries that need no launch, and every KDLAE_EINVAL_* path of the new C entries (the
pointers there are never dereferenced: every check comes before the launch)."""
import ctypes

import pytest
import torch

from rethink_acoustic_image_enhancement_amd import _lib, streams
from rethink_acoustic_image_enhancement_amd.KDLAE_model import KDLAE_student
from rethink_acoustic_image_enhancement_amd.pipeline import enhance_stream_u8
from tests import stream_model as sm


# ------------------------------------------------------------------ the schedule
@pytest.mark.parametrize("F", sm.FRAMES)
def test_schedule_follows_the_rule(F):
    for emit in range(F):
        for T in sm.LENGTHS(F):
            got = streams.stream_schedule(T, F, emit)
            assert len(got) == T + 1 and [c for c, _, _ in got] == list(range(T)) + ["flush"]
            # every frame exactly once and in order, from the rule's window at the rule's position
            emitted = []
            for call, s, ps in got:
                assert (s is None) == (len(ps) == 0), (T, emit, call)
                for p in ps:
                    emitted.append((s + p, s, p))
                    if call != "flush":   # a push knows the frames up to its own only
                        assert s + min(F, T) - 1 == call
            assert [t for t, _, _ in emitted] == list(range(T)), (T, emit)
            for t, s, p in emitted:
                assert (s, p) == sm.window_of(t, T, F, emit)[1:], (T, emit, t)
            # k per push as stated, the flush takes the rest
            assert [len(ps) for _, _, ps in got[:-1]] == sm.count_per_push(T, F, emit)
            assert len(got[-1][2]) == (T if T < F else F - 1 - emit)
            # and the model's own derivation agrees entry by entry
            assert got == sm.schedule(T, F, emit), (T, emit)


def test_schedule_defaults_and_refusals():
    assert streams.stream_schedule(9) == streams.stream_schedule(9, 7, 3)
    assert streams.stream_schedule(4, 4, None) == streams.stream_schedule(4, 4, 2)
    assert streams.stream_schedule(3, 1) == [(0, 0, [0]), (1, 1, [0]), (2, 2, [0]), ("flush", None, [])]
    assert streams.stream_schedule(5, 3, 2)[-1] == ("flush", None, [])   # causal: nothing left
    for kw, text in ((dict(T=3, frames=0), "frames must be"), (dict(T=3, frames=3, emit=3), "emit"),
                     (dict(T=3, frames=3, emit=-1), "emit"), (dict(T=-1), "T must not")):
        with pytest.raises(RuntimeError, match=text):
            streams.stream_schedule(**kw)


# ------------------------------------------------------------------ refusals of the Python entries, no launch
def test_python_entries_refuse_before_any_launch():
    m = KDLAE_student()
    cpu_frame = torch.zeros(1, 20, 27, dtype=torch.uint8)
    for call, text in ((lambda: streams.StudentStream(m, 1, 20, 27, frames=7, emit=7), "emit"),
                       (lambda: m.stream(1, 20, 27, frames=3, emit=3), "emit"),
                       (lambda: m.stream(1, 20, 27, frames=0), "frames must be"),
                       (lambda: m.stream(1, 20, 27, channels=2), "channels"),
                       (lambda: m.stream(1, 32, 32, channels=3, dtype="f32"), "channels"),
                       (lambda: m.stream(1, 20, 27, dtype="f16"), "dtype"),
                       (lambda: m.stream(0, 20, 27), "at least 1"),
                       (lambda: m.stream(1, 20, 27, multiple=0), "at least 1"),
                       (lambda: m.stream(1, 20, 27, multiple=1), "divisible by 4"),
                       (lambda: m.stream(1, 30, 30, dtype="f32"), "divisible by 4"),
                       (lambda: m.stream(1, 3, 40), "reflect padding"),
                       (lambda: m.stream(1, 20, 27), "no CPU fallback"),           # the module is on the CPU
                       (lambda: list(enhance_stream_u8(m, [cpu_frame])), "cuda uint8"),
                       (lambda: list(enhance_stream_u8(m, [cpu_frame.float()])), "cuda uint8"),
                       (lambda: list(enhance_stream_u8(m, [cpu_frame[0]])), "cuda uint8"),
                       (lambda: list(enhance_stream_u8(m, [], frames=3, emit=5)), "emit")):
        with pytest.raises(RuntimeError, match=text):
            call()
    assert list(enhance_stream_u8(m, [])) == []


# ------------------------------------------------------------------ refusals of the C entries, no launch
def test_c_entries_refuse_bad_arguments():
    """1 = KDLAE_EINVAL_SHAPE, 2 = KDLAE_EINVAL_CONFIG."""
    L = _lib.lib()
    P = 0x1000   # a non-null, 16-byte aligned "device pointer"
    assert L.kdlae_stream_state_bytes(2, 7, 32, 32) == 16 + 2 * 7 * 32 * 32 * 4
    assert L.kdlae_stream_state_bytes(1, 1, 1, 1) == 20
    for bad in ((0, 7, 32, 32), (1, 0, 32, 32), (1, 7, 0, 32), (1, 7, 32, 0), (-1, 7, 32, 32)):
        assert L.kdlae_stream_state_bytes(*bad) == -1 and "kdlae_stream_state_bytes" in _lib.last_error()
    assert L.kdlae_stream_state_bytes(1, 1, 1 << 16, 1 << 16) == -1   # more than 2^31 - 1 pixels of a frame

    assert L.kdlae_stream_reset(None, None) == 2 and L.kdlae_stream_advance(None, None) == 2
    assert L.kdlae_stream_advance(P + 4, None) == 1

    def u8(frame=P, B=1, h=20, w=27, channels=1, multiple=32, frames=7, state=P, stack=P):
        return L.kdlae_stream_push_u8(frame, B, h, w, channels, multiple, frames, state, stack, None)

    for kw in (dict(frame=None), dict(state=None), dict(stack=None), dict(B=0), dict(h=0), dict(w=0), dict(frames=0),
               dict(B=-2), dict(channels=0), dict(channels=2), dict(channels=5), dict(multiple=0), dict(multiple=-8)):
        assert u8(**kw) == 2, kw
        assert "kdlae_stream_push_u8" in _lib.last_error()
    assert u8(h=3, w=40) == 1 and "reflect" in _lib.last_error()    # 3 rows padded to 32
    assert u8(h=20, w=10) == 1                                      # 10 columns padded to 32
    assert u8(state=P + 4) == 1 and u8(stack=P + 2) == 1
    assert u8(h=1 << 16, w=1 << 16, multiple=1) == 1 and "2^31" in _lib.last_error()
    assert u8(h=20, w=27, multiple=(1 << 31) - 8) == 1

    def f32(frame=P, B=1, H=32, W=32, frames=7, state=P, stack=P):
        return L.kdlae_stream_push_f32(frame, B, H, W, frames, state, stack, None)

    for kw in (dict(frame=None), dict(state=None), dict(stack=None), dict(B=0), dict(H=0), dict(W=0), dict(frames=0)):
        assert f32(**kw) == 2, kw
        assert "kdlae_stream_push_f32" in _lib.last_error()
    assert f32(frame=P + 2) == 1 and f32(state=P + 4) == 1 and f32(stack=P + 1) == 1
    assert f32(H=1 << 16, W=1 << 16) == 1
    assert ctypes.c_int(L.kdlae_abi_version()).value == 1
