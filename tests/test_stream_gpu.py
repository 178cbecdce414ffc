"""Streaming inference on the GPU: kdlae_stream_push_u8 / kdlae_stream_push_f32 / kdlae_stream_advance /
kdlae_stream_reset against ``frames_preprocess_u8`` and slicing, then ``StudentStream`` and
``pipeline.enhance_stream_u8`` against the host loop they replace (tests/stream_model.py: per frame, the module's
own ``enhance_frames_u8`` / ``forward`` on the frame's window).

The kernels copy and convert by the rule ``frames_preprocess_u8`` uses, the student's forward is deterministic and a
replayed graph runs the launches it captured, so every comparison here is bit for bit or byte for byte: no
tolerance anywhere in this file."""
import ctypes
import functools

import pytest
import torch

from rethink_acoustic_image_enhancement_amd import _lib
from rethink_acoustic_image_enhancement_amd.hashweights import hash_images, load_hash_weights
from rethink_acoustic_image_enhancement_amd.KDLAE_model import KDLAE_student
from rethink_acoustic_image_enhancement_amd.pipeline import enhance_stream_u8, frames_preprocess_u8, padded_size
from rethink_acoustic_image_enhancement_amd.streams import StudentStream
from tests import stream_model as sm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BIG = 1e30
GUARD = 0xAB    # the byte either side of the state under test
G = 64          # guard floats either side of the stack under test
UH, UW = 20, 27   # reflect-padded to 32 x 32


def _c(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _u8_clip(seed, shape):
    return torch.randint(0, 256, shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _at_byte_offset(t, off):
    """A contiguous copy of ``t`` whose first byte sits ``off`` bytes past a 16-byte boundary."""
    store = torch.empty(off + t.numel() * t.element_size(), dtype=torch.uint8, device=DEV)
    assert store.data_ptr() % 16 == 0
    view = store[off:].view(t.dtype).view(t.shape)
    view.copy_(t)
    return view


# ------------------------------------------------------------------ 1. the kernels against preprocess and slicing
class _Ring:
    """State and stack in guarded, poisoned storage at the given offsets from a 16-byte boundary."""

    def __init__(self, B, F, H, W, state_off, stack_off):
        self.B, self.F, self.H, self.W = B, F, H, W
        nbytes = _lib.lib().kdlae_stream_state_bytes(B, F, H, W)
        assert nbytes == 16 + B * F * H * W * 4
        self.state_store = torch.full((256 + state_off + nbytes + 256,), GUARD, dtype=torch.uint8, device=DEV)
        self.state = self.state_store[256 + state_off:256 + state_off + nbytes]
        self.state[16:].view(torch.float32).fill_(float("nan"))    # the ring: arbitrary, must never reach an output
        n = B * F * H * W
        self.stack_store = torch.full((G + stack_off + n + G,), BIG, device=DEV)
        self.stack = self.stack_store[G + stack_off:G + stack_off + n].view(B, F, H, W)
        assert self.state_store.data_ptr() % 16 == 0 and self.stack_store.data_ptr() % 16 == 0
        assert _lib.lib().kdlae_stream_reset(_c(self.state), None) == 0, _lib.last_error()

    def ring(self):
        return self.state[16:].view(torch.float32).view(self.B, self.F, self.H, self.W)

    def count(self):
        return int(self.state[:8].view(torch.int64).item())

    def check(self, x, t):
        """After push t and its advance: the stack holds frames t - F + 1 .. t in time order (as many as have
        arrived), the ring frame c in slot c % F, the counter t + 1, and the guards are whole."""
        F = self.F
        k = min(t + 1, F)
        assert _same_bits(self.stack[:, F - k:], x[:, t + 1 - k:t + 1]), t
        for c in range(t + 1 - k, t + 1):
            assert _same_bits(self.ring()[:, c % F], x[:, c]), (t, c)
        assert self.count() == t + 1
        n = self.stack.numel()
        assert bool((self.stack_store[:-(G + n)] == BIG).all()) and bool((self.stack_store[-G:] == BIG).all())
        assert bool((self.state_store[:256] == GUARD).all()) and bool((self.state_store[-256:] == GUARD).all())


# (state offset in bytes, stack offset in floats): both on 16 bytes is the 16-byte path, anything else the 4-byte one
RING_OFFSETS = [(0, 0), (8, 0), (0, 1), (8, 3)]


@pytest.mark.parametrize("channels", [1, 3, 4])
@pytest.mark.parametrize("hwm", [(UH, UW, 32), (32, 32, 32), (UH, UW, 1), (8, 12, 8)])
def test_push_u8_equals_preprocess(hwm, channels):
    """w = 27 reads single bytes, w = 32 gray on 4 bytes reads 4 bytes a load; multiple 1 keeps W = 27: 4-byte float
    accesses; a source at byte offset 1 everywhere."""
    L = _lib.lib()
    h, w, mult = hwm
    H, W = padded_size(h, w, mult)
    B = 2
    for F in (1, 3):
        T = 2 * F + 3
        clip = _u8_clip(100 * h + channels, (B, T, h, w) + ((channels,) if channels > 1 else ()))
        x = frames_preprocess_u8(clip, mult)
        assert x.shape == (B, T, H, W)
        for src_off in (0, 1):
            frames = [_at_byte_offset(clip[:, t].contiguous(), src_off) for t in range(T)]
            assert frames[0].data_ptr() % 16 == src_off
            for state_off, stack_off in RING_OFFSETS:
                r = _Ring(B, F, H, W, state_off, stack_off)
                for t in range(T):
                    for _ in range(2):   # a push without an advance lands in the same slot again
                        rc = L.kdlae_stream_push_u8(_c(frames[t]), B, h, w, channels, mult, F, _c(r.state),
                                                    _c(r.stack), None)
                        assert rc == 0, _lib.last_error()
                    assert L.kdlae_stream_advance(_c(r.state), None) == 0, _lib.last_error()
                    r.check(x, t)
                assert torch.equal(frames[-1], clip[:, -1])
                # a reset starts over: the first push of the next stream lands in slot 0
                assert L.kdlae_stream_reset(_c(r.state), None) == 0 and r.count() == 0


@pytest.mark.parametrize("hw", [(5, 7), (4, 6), (8, 8)])
def test_push_f32_is_a_bit_copy(hw):
    L = _lib.lib()
    H, W = hw
    B = 2
    for F in (1, 3):
        T = 2 * F + 3
        x = torch.from_numpy(hash_images(f"stream:f32:{H}x{W}:{F}", (B, T, H, W), -1.0, 1.0)).to(DEV)
        x[0, 0, 0, :3] = torch.tensor([float("inf"), -0.0, 1e-42], device=DEV)
        for src_off in (0, 4):
            frames = [_at_byte_offset(x[:, t].contiguous(), src_off) for t in range(T)]
            for state_off, stack_off in RING_OFFSETS:
                r = _Ring(B, F, H, W, state_off, stack_off)
                for t in range(T):
                    rc = L.kdlae_stream_push_f32(_c(frames[t]), B, H, W, F, _c(r.state), _c(r.stack), None)
                    assert rc == 0, _lib.last_error()
                    assert L.kdlae_stream_advance(_c(r.state), None) == 0, _lib.last_error()
                    r.check(x, t)


# ------------------------------------------------------------------ 2. StudentStream against the host loop
def _fresh_model():
    """A module (and so an engine, a workspace) of its own, with the shared model's weights."""
    m = KDLAE_student()   # hidden [16, 32, 64]
    load_hash_weights(m)
    return m.to(DEV).eval()


@functools.lru_cache(maxsize=None)
def _model():
    return _fresh_model()


@functools.lru_cache(maxsize=None)
def _clip(B, channels, h=UH, w=UW):
    """The longest stream of the tests; shorter ones are its first T frames."""
    return _u8_clip(7 * B + channels + h, (B, 2 * 7 + 3, h, w) + ((channels,) if channels > 1 else ()))


_WINDOWS = {}   # (kind, B, channels, h, w) -> {(f, s): the shared model's output for that window}; never written twice


def _want(kind, B, channels, T, F, emit, h=UH, w=UW):
    cache = _WINDOWS.setdefault((kind, B, channels, h, w), {})
    clip = _clip(B, channels, h, w)[:, :T]
    if kind == "u8":
        return sm.reference_u8(_model(), clip, F, emit, cache=cache)
    return sm.reference_f32(_model(), frames_preprocess_u8(_clip(B, channels, h, w), 32)[:, :T], F, emit, cache=cache)


def _new_stream(kind, B, F, emit, channels=1, h=UH, w=UW, graphs=True, model=None):
    m = model if model is not None else _model()
    if kind == "u8":
        s = m.stream(B, h, w, F, emit, channels)
    else:
        H, W = padded_size(h, w, 32)
        s = m.stream(B, H, W, F, emit, dtype="f32")
    s.hip_graphs = graphs
    return s


def _input(kind, B, channels, T, h=UH, w=UW):
    clip = _clip(B, channels, h, w)
    return clip[:, :T] if kind == "u8" else frames_preprocess_u8(clip, 32)[:, :T]


def _equal(kind, a, b):
    return torch.equal(a, b) if kind == "u8" else _same_bits(a, b)


@pytest.mark.parametrize("channels", [1, 4])
@pytest.mark.parametrize("F", sm.FRAMES)
@pytest.mark.parametrize("B", [1, 2])
def test_u8_stream_equals_the_host_loop(B, F, channels):
    for emit in sm.EMITS(F):
        s = _new_stream("u8", B, F, emit, channels)
        assert isinstance(s, StudentStream) and (s.H, s.W) == (32, 32)
        for rep in range(2):   # the same stream again after its flush: equal bytes
            for T in sm.LENGTHS(F):
                got = sm.run_stream(s, _input("u8", B, channels, T))
                assert got.dtype == torch.uint8 and got.shape == (B, T, UH, UW)
                assert torch.equal(got, _want("u8", B, channels, T, F, emit)), (emit, rep, T)


@pytest.mark.parametrize("F", sm.FRAMES)
@pytest.mark.parametrize("B", [1, 2])
def test_f32_stream_equals_forward_per_window(B, F):
    for emit in sm.EMITS(F):
        s = _new_stream("f32", B, F, emit)
        for rep in range(2):
            for T in sm.LENGTHS(F):
                got = sm.run_stream(s, _input("f32", B, 1, T))
                assert got.dtype == torch.float32 and got.shape == (B, T, 32, 32)
                assert _same_bits(got, _want("f32", B, 1, T, F, emit)), (emit, rep, T)


@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_three_modes_give_equal_bytes(kind):
    """Eager, the capturing push and the replays; on the graph run a silent eager fallback shows in the counters."""
    B, F, emit = 2, 3, 1
    T = 2 * F + 3
    full = T - F + 1
    x = _input(kind, B, 1, T)
    want = _want(kind, B, 1, T, F, emit)
    eager, graph = _new_stream(kind, B, F, emit, graphs=False), _new_stream(kind, B, F, emit, graphs=True)
    assert _equal(kind, sm.run_stream(eager, x), want)
    assert (eager.graph_replays, eager.graph_captures) == (0, 0)
    assert _equal(kind, sm.run_stream(graph, x), want)
    assert (graph.graph_replays, graph.graph_captures) == (full - 2, 1)
    assert _equal(kind, sm.run_stream(graph, x), want)          # after the flush every full push replays
    assert (graph.graph_replays, graph.graph_captures) == (2 * full - 2, 1)
    graph.hip_graphs = False                                    # and off again
    assert _equal(kind, sm.run_stream(graph, x), want)
    assert (graph.graph_replays, graph.graph_captures) == (2 * full - 2, 1)
    # what push returns is the caller's: writing to it does not reach the next result
    a = graph.push(x[:, 0])
    assert a.shape[1] == 0
    b = graph.push(x[:, 1]), graph.push(x[:, 2])
    keep = b[1].clone()
    b[1].fill_(0)
    c = graph.push(x[:, 3])
    assert _equal(kind, keep, want[:, :2]) and _equal(kind, c, want[:, 2:3])
    graph.reset()


def _poison(s):
    s._state[:16].fill_(0xFF)
    s._state[16:].view(torch.float32).fill_(float("nan"))
    s._stack.fill_(float("nan"))
    s._y.fill_(BIG)
    if s._u8 is not None:
        s._u8.fill_(GUARD)
    s._frame.fill_(GUARD if s.kind == "u8" else float("nan"))


@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_poisoned_storage_never_reaches_an_output(kind):
    B, F, emit = 1, 7, 3
    s = _new_stream(kind, B, F, emit)
    for T in (3, F - 1, 1, F, 2 * F + 3):     # T < F through flush first, then full windows, twice over
        _poison(s)
        s.reset()
        got = sm.run_stream(s, _input(kind, B, 1, T))
        assert _equal(kind, got, _want(kind, B, 1, T, F, emit)), T
        if kind == "f32":
            assert bool(torch.isfinite(got).all()) and float(got.abs().max()) < 1e6
    # a reset in mid-stream discards what was pushed, whatever the ring holds
    x = _input(kind, B, 1, F + 2)
    for t in range(F + 1):
        s.push(x[:, t])
    _poison(s)
    s.reset()
    assert _equal(kind, sm.run_stream(s, x), _want(kind, B, 1, F + 2, F, emit))
    assert s.flush().shape[1] == 0    # T == 0


def test_workspace_growth_in_mid_stream():
    """A larger forward on the same module moves the engine's workspace between two pushes: the graph, which baked
    the old pointer in, is captured again and the bytes still match."""
    m = _fresh_model()   # an engine of its own, so the workspace starts at this stream's size
    B, F, emit = 1, 3, 1
    T = 2 * F + 3
    s = _new_stream("u8", B, F, emit, h=32, w=32, model=m)
    x = _input("u8", B, 1, T, 32, 32)
    want = _want("u8", B, 1, T, F, emit, 32, 32)
    parts = [s.push(x[:, t]) for t in range(F + 2)]
    assert (s.graph_replays, s.graph_captures) == (1, 1)
    ws0 = m.engine(torch.device(DEV)).ws
    before = (ws0.data_ptr(), ws0.numel())
    with torch.no_grad():
        m(torch.rand(2, F, 64, 64, device=DEV))
    ws1 = m.engine(torch.device(DEV)).ws
    assert ws1.numel() > before[1]
    parts += [s.push(x[:, t]) for t in range(F + 2, T)] + [s.flush()]
    assert torch.equal(torch.cat(parts, 1), want)
    assert s.graph_captures == 2 and s.graph_replays == 1 + (T - F - 2) - 1


def test_two_streams_on_one_module():
    B, F = 1, 3
    T = 2 * F + 3
    a, b = _new_stream("u8", B, F, 0), _new_stream("u8", B, F, F - 1, channels=4)
    xa, xb = _input("u8", B, 1, T), _input("u8", B, 4, T)
    pa, pb = [], []
    for t in range(T):
        pa.append(a.push(xa[:, t]))
        pb.append(b.push(xb[:, t]))
    pa.append(a.flush())
    pb.append(b.flush())
    assert pb[-1].shape[1] == 0   # the causal setting leaves nothing for the flush
    assert torch.equal(torch.cat(pa, 1), _want("u8", B, 1, T, F, 0))
    assert torch.equal(torch.cat(pb, 1), _want("u8", B, 4, T, F, F - 1))
    assert a.graph_replays > 0 and b.graph_replays > 0


def test_parameter_update_between_pushes_is_seen():
    m = _fresh_model()
    B, F, emit = 1, 3, 1
    T = 2 * F + 3
    x = _input("u8", B, 1, T)
    s = _new_stream("u8", B, F, emit, model=m)
    old = sm.reference_u8(m, x, F, emit)
    cut = F + 3                       # pushes 0 .. cut - 1 run with the old weights: eager, capture, replays
    parts = [s.push(x[:, t]) for t in range(cut)]
    n_old = sum(p.shape[1] for p in parts)
    assert s.graph_replays >= 1
    with torch.no_grad():
        m.encoders[0][0].weight.mul_(1.25)
        m.out_conv.bias.add_(0.03125)
    new = sm.reference_u8(m, x, F, emit)
    assert not torch.equal(old[:, n_old:], new[:, n_old:])
    parts += [s.push(x[:, t]) for t in range(cut, T)] + [s.flush()]
    assert s.graph_captures == 1      # the storages did not move: no new capture, the pack program is in the graph
    assert torch.equal(torch.cat(parts, 1), torch.cat([old[:, :n_old], new[:, n_old:]], 1))


@pytest.mark.parametrize("graphs", [False, True])
@pytest.mark.parametrize("hw", [(UH, UW), (32, 32)])
def test_u8_source_at_byte_offset_one(hw, graphs):
    h, w = hw
    B, F, emit = 1, 3, 1
    T = F + 3
    x = _input("u8", B, 1, T, h, w)
    want = _want("u8", B, 1, T, F, emit, h, w)
    for off in (1, 0):
        s = _new_stream("u8", B, F, emit, h=h, w=w, graphs=graphs)
        parts = []
        for t in range(T):
            frame = _at_byte_offset(x[:, t].contiguous(), off)
            assert frame.data_ptr() % 16 == off
            parts.append(s.push(frame))
        parts.append(s.flush())
        assert torch.equal(torch.cat(parts, 1), want), off


def test_enhance_stream_u8_yields_every_frame_in_order():
    m = _model()
    B, T = 2, 2 * 7 + 3
    for channels in (1, 4):
        x = _input("u8", B, channels, T)
        got = list(enhance_stream_u8(m, (x[:, t] for t in range(T))))
        assert len(got) == T and all(g.shape == (B, UH, UW) and g.dtype == torch.uint8 for g in got)
        assert torch.equal(torch.stack(got, 1), _want("u8", B, channels, T, 7, 3))
    x = _input("u8", B, 1, 4)
    got = list(enhance_stream_u8(m, [x[:, t] for t in range(4)], frames=3, emit=2))
    assert torch.equal(torch.stack(got, 1), _want("u8", B, 1, 4, 3, 2))
    got = list(enhance_stream_u8(m, [x[:, 0][..., None], x[:, 1][..., None]]))   # [B,h,w,1] is gray too; T < frames
    assert torch.equal(torch.stack(got, 1), _want("u8", B, 1, 2, 7, 3))


def test_push_refusals_come_before_any_launch():
    m = _model()
    s = _new_stream("u8", 1, 3, 1)
    f = _new_stream("f32", 1, 3, 1)
    ok = torch.zeros(1, UH, UW, dtype=torch.uint8, device=DEV)
    for call, text in ((lambda: s.push(ok.cpu()), "expects a cuda uint8"),
                       (lambda: s.push(ok.float()), "expects a cuda uint8"),
                       (lambda: s.push(ok[:, :-1]), "expects a cuda uint8"),
                       (lambda: s.push(ok[0]), "expects a cuda uint8"),
                       (lambda: s.push(ok[..., None].expand(-1, -1, -1, 3)), "expects a cuda uint8"),
                       (lambda: s.push(None), "expects a cuda uint8"),
                       (lambda: f.push(ok), "expects a cuda float32"),
                       (lambda: f.push(torch.zeros(1, UH, UW, device=DEV)), "expects a cuda float32")):
        with pytest.raises(RuntimeError, match=text):
            call()
    assert s._t == 0 and int(s._state[:8].view(torch.int64).item()) == 0   # nothing was taken in
    t = _fresh_model().train()
    st = _new_stream("u8", 1, 3, 1, model=t)
    with pytest.raises(RuntimeError, match="inference only"):
        st.push(ok)
    with torch.no_grad():
        assert st.push(ok).shape == (1, 0, UH, UW)
    out = s.push(ok)
    assert out.shape == (1, 0, UH, UW) and not out.requires_grad
