"""The caller's-stream contract of include/kdlae.h, checked on a `Call` of tests/workspace_harness.py: every entry
that takes a `stream` orders all its device work on that stream, sends nothing to the null stream, makes the
streams the library owns wait on it and joins them into it before returning, and neither waits on the host nor
allocates, so that the call can be captured into a HIP graph.

Terms.  The reference of a call is its outputs when it runs on the null stream of an idle device, followed by a
synchronise.  The stale inputs are a second valid set of operand contents of the same shapes and dtypes (hash
images in another order, parameters at half their size: finite, and as safe to run on as the real ones).  `s` is a
stream that does not synchronise with the null stream.

S1  asynchrony: the operands hold the stale contents and the device is idle.  On `s`: a spin, the fill of the
    arena, copies of the real contents into the operand buffers, the call's steps, an event.  Right after the last step has returned on the
    host the event has not completed: the call returned while its stream was still held.
S2  order: after a synchronise the outputs have the reference's bits (a launch that went to the null stream, or to
    a library stream that did not wait for `s`, ran during the spin on stale inputs or unwritten scratch), the
    guards of the arena are whole, and one more call on the null stream leaves the read-only operands as they were.
S3  capture: after two warm-up runs on `s` the steps are captured into a graph on `s` with the outputs and the
    workspace filled; nothing ran eagerly (every word still holds the fill); a replay gives the reference's bits;
    with the stale contents in the operand buffers a second replay gives the stale set's own reference.

Every comparison is bit equality or an event query: no tolerance in this file."""
import ctypes
import functools

import torch

from rethink_acoustic_image_enhancement_amd import _lib
from tests.workspace_harness import BIG, DEV, Arena, bits, same_bits

SPIN = 1_000_000_000          # cycles: the spin tests/test_train_gpu.py holds the device with while the host enqueues
HIP_STREAM_NON_BLOCKING = 1   # hipStreamNonBlocking
PARAM_OPERANDS = ("params", "theta")


@functools.lru_cache(maxsize=None)
def _hip():
    """The HIP runtime torch has loaded (the same library object: dlopen by its path in this process)."""
    with open("/proc/self/maps") as f:
        paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line})
    assert paths, "torch has not loaded libamdhip64"
    hip = ctypes.CDLL(paths[0])
    hip.hipStreamGetFlags.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint)]
    hip.hipStreamCreateWithFlags.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint]
    return hip


def stream_flags(s):
    flags = ctypes.c_uint(0xFFFFFFFF)
    rc = _hip().hipStreamGetFlags(ctypes.c_void_p(s.cuda_stream), ctypes.byref(flags))
    assert rc == 0, f"hipStreamGetFlags: error {rc}"
    return flags.value


@functools.lru_cache(maxsize=None)
def side_stream():
    """`s`: one stream per session that does not synchronise with the null stream (asserted through
    hipStreamGetFlags; a torch stream that turned out blocking is replaced by one created non-blocking)."""
    torch.cuda.init()
    s = torch.cuda.Stream(device=DEV)
    if stream_flags(s) & HIP_STREAM_NON_BLOCKING:
        return s
    raw = ctypes.c_void_p()
    rc = _hip().hipStreamCreateWithFlags(ctypes.byref(raw), HIP_STREAM_NON_BLOCKING)
    assert rc == 0 and raw.value, f"hipStreamCreateWithFlags: error {rc}"
    s = torch.cuda.ExternalStream(raw.value, device=DEV)
    assert stream_flags(s) & HIP_STREAM_NON_BLOCKING
    return s


def arena_for(call):
    """The guarded allocation of a call; a call without a workspace gets a 256-byte one that no step is given."""
    return Arena(call.out_numels, call.ws_bytes if call.ws_bytes else 256)


def stale_of(name, t):
    """A second valid content for operand `name`: parameters at half their size (signs, zeros and positive
    statistics stay what they are), anything else with its elements in reverse order."""
    if name in PARAM_OPERANDS:
        return t * 0.5
    return t.reshape(-1).flip(0).reshape(t.shape).contiguous()


def same_contents(a, b):
    """Bit equality for an operand of any dtype (u8 frames and int32 tables as well as floats)."""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.element_size() == 4:
        return same_bits(a, b)
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _operands(call):
    return {k: t for k, t in call.operands.items() if t is not None and t.numel()}


def _stale(call, real):
    own = getattr(call, "stale", None)
    return own(real) if own is not None else {k: stale_of(k, t) for k, t in real.items()}


def _put(call, contents):
    for k, t in _operands(call).items():
        t.copy_(contents[k])


def _enqueue(call, arena, what):
    call.prepare()
    for name, fn in call.steps(arena):
        rc = fn(arena.ws_bytes)
        assert rc == 0, f"{what} {name}: rc {rc}, '{_lib.last_error()}'"


def _differs(got, want):
    for i, (g, w) in enumerate(zip(got, want)):
        if not same_bits(g, w):
            bad = (bits(g) != bits(w)).nonzero().view(-1)
            return (f"output {i}: {bad.numel()} of {w.numel()} words differ, first at {int(bad[0])} "
                    f"({float(g.reshape(-1)[bad[0]])} vs {float(w.reshape(-1)[bad[0]])})")
    return None


def references(call, arena):
    """(real contents, stale contents, reference, the stale set's reference); the operands hold the real contents
    afterwards.  The two references must differ, or no check below could tell which inputs a launch read."""
    torch.cuda.synchronize()
    real = {k: t.clone() for k, t in _operands(call).items()}
    stale = _stale(call, real)
    assert set(stale) == set(real)
    arena.fill(BIG)
    ref = call.run(arena, "reference")
    _put(call, stale)
    arena.fill(BIG)
    ref_stale = call.run(arena, "stale reference")
    _put(call, real)
    torch.cuda.synchronize()
    assert _differs(ref_stale, ref) is not None, "the stale inputs give the reference's bits: the case checks nothing"
    return real, stale, ref, ref_stale


def check_async_and_order(call, check_async=True):
    """S1 + S2 (check_async=False: S2 alone, for an entry documented to wait on the host)."""
    s = side_stream()
    arena = arena_for(call)
    real, stale, ref, _ = references(call, arena)
    _put(call, stale)
    arena.fill(BIG)
    torch.cuda.synchronize()
    done = torch.cuda.Event()
    with torch.cuda.stream(s):
        torch.cuda._sleep(SPIN)
        arena.fill(BIG)      # behind the spin: what a stray null-stream memset or launch wrote meanwhile is undone
        for k, t in _operands(call).items():
            t.copy_(real[k], non_blocking=True)
        _enqueue(call, arena, "on the side stream")
        done.record()
    in_flight = not done.query()
    torch.cuda.synchronize()
    if check_async:
        assert in_flight, "S1: the stream had drained when the last step returned: a step waited on the host"
    got = [o.clone() for o in arena.outs]
    diff = _differs(got, ref)
    assert diff is None, f"S2: the side-stream run differs from the null-stream reference: {diff}"
    arena.assert_guards("S2")
    call.run(arena, "null stream again")
    for k, t in _operands(call).items():
        assert same_contents(t, real[k]), f"S2: read-only operand {k} was written"
    return got


def check_capture(call):
    """S3."""
    s = side_stream()
    arena = arena_for(call)
    real, stale, ref, ref_stale = references(call, arena)
    with torch.cuda.stream(s):
        for _ in range(2):      # attribute setting, lazily created streams and events, workspace sizing
            _enqueue(call, arena, "warm-up")
    torch.cuda.synchronize()
    arena.fill(BIG)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s, capture_error_mode="thread_local"):
        _enqueue(call, arena, "under capture")
    torch.cuda.synchronize()
    assert arena.holds_fill(), "S3: a step ran eagerly during the capture: the outputs or the workspace were written"
    g.replay()
    torch.cuda.synchronize()
    diff = _differs(arena.outs, ref)
    assert diff is None, f"S3: the replay differs from the null-stream reference: {diff}"
    arena.assert_guards("S3")
    _put(call, stale)
    g.replay()
    torch.cuda.synchronize()
    diff = _differs(arena.outs, ref_stale)
    _put(call, real)
    del g
    call.run(arena, "null stream again")      # a handle's packed weights follow the operands back
    assert diff is None, f"S3: the replay on new operand contents differs from their own reference: {diff}"
