"""Streaming inference for KDLAE-S: one frame in, one enhanced frame out at a fixed latency, the window kept on the
device and the steady state replayed as one HIP graph.

The rule (include/kdlae.h states it too).  A stream has ``B`` parallel sources, ``frames = F >= 1`` and ``emit``
with ``0 <= emit < F`` (default ``F // 2``).  Frame ``t`` of a stream of ``T`` frames is

    f = min(F, T);  s_t = min(max(t - emit, 0), T - f);  out[:, t] = forward(x[:, s_t : s_t + f])[:, t - s_t]

Every frame comes from the window in which it sits at position ``emit``; the first ``emit`` frames come from the
first window, the last ``F - 1 - emit`` from the last, and a stream shorter than ``F`` is one window and equals
``forward`` on it.  ``emit = F - 1`` is the causal setting: no latency, nothing left for ``flush``.  The student's 3-D
convolutions zero-pad along the frame axis, so, as with ``forward_clip``, this is a different function of the stream
from one forward over all ``T`` frames, not an approximation of it that carries an error bound.

The schedule: push number ``t`` (0-based) returns nothing while ``t < F - 1``, frames ``0 .. emit`` at ``t = F - 1``
and frame ``t - (F - 1 - emit)`` afterwards; ``flush()`` returns the last window's remaining ``F - 1 - emit`` frames
(all ``T`` frames through one eager forward when ``T < F``, nothing when ``T == 0``) and resets the stream.  Every
frame is emitted exactly once, in order.  ``stream_schedule`` is that schedule as a pure host function.

``StudentStream`` owns the ring of converted frames (``kdlae_stream_push_u8`` / ``kdlae_stream_push_f32`` take the
new frame in and write the time-ordered stack), the static stack and outputs, and the graph of
push -> student forward -> u8 frames -> advance.  ``pipeline.enhance_stream_u8`` is the generator on top."""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from .tiling import _stream

KINDS = ("u8", "f32")


def _check_rule(frames, emit):
    """-> (F, emit) as ints.  RuntimeError unless frames >= 1 and 0 <= emit < frames (emit None: frames // 2)."""
    F = int(frames)
    if F < 1:
        raise RuntimeError(f"stream: frames must be at least 1, got {frames}")
    e = F // 2 if emit is None else int(emit)
    if not 0 <= e < F:
        raise RuntimeError(f"stream: need 0 <= emit < frames = {F}, got {emit}")
    return F, e


def stream_schedule(T: int, frames: int = 7, emit: int | None = None):
    """The emission schedule of a stream of ``T`` frames, host only: a list with one entry per push, in order, and
    a last entry for the flush, each ``(t or "flush", window start, positions)``: the call returns the window's
    output at ``positions`` (frame ``start + p`` of the stream for each ``p``); ``(t, None, [])`` for a call that
    returns nothing.  The window of an entry has ``min(frames, T)`` frames."""
    F, e = _check_rule(frames, emit)
    T = int(T)
    if T < 0:
        raise RuntimeError(f"stream: T must not be negative, got {T}")
    out = []
    for t in range(T):
        if t < F - 1:
            out.append((t, None, []))
        elif t == F - 1:
            out.append((t, 0, list(range(e + 1))))
        else:
            out.append((t, t - (F - 1), [e]))
    if T == 0 or (T >= F and e == F - 1):
        out.append(("flush", None, []))
    elif T < F:
        out.append(("flush", 0, list(range(T))))
    else:
        out.append(("flush", T - F, list(range(e + 1, F))))
    return out


class StudentStream:
    """``KDLAE_student`` on a live stream of ``batch`` parallel sources of ``h x w`` frames (module docstring: the
    rule and the schedule).

    ``dtype="u8"``: ``push`` takes a cuda uint8 frame ``[B,h,w]`` (``channels=1``) or ``[B,h,w,channels]`` (3 / 4:
    cv2 BGR / BGRA) and returns uint8 ``[B,k,h,w]``: the bytes ``pipeline.enhance_frames_u8`` gives for the frame's
    window.  ``dtype="f32"``: ``push`` takes a cuda float32 frame ``[B,H,W]`` the caller has preprocessed
    (``h, w`` are then ``H, W`` and ``multiple`` is not used) and returns float32 ``[B,k,H,W]``: the bits of
    ``forward``.  ``k`` is 0, 1 or ``emit + 1``; what is returned is a fresh tensor, never a view of the stream's
    static storage.

    With ``hip_graphs = True`` (the default is off until ``tools/stream_probe.py`` has shown replay to beat the eager
    stream on the card: DESIGN §22) the steady state replays a HIP graph, as ``KDLAE_teacher`` does: the first push
    with a full window runs launch by
    launch (it sizes the engine's workspace and builds the pack program), the second captures
    push -> forward -> u8 conversion -> advance on one stream, a linear chain, and the rest replay it.  The weight
    pack program is inside the graph, so an in-place parameter update between pushes is seen.  The graph is
    captured again when the engine's workspace or flat parameter buffer moved or a parameter's storage changed;
    a failed capture leaves the stream eager for good.  ``graph_replays``
    counts the pushes served by replaying an earlier capture and ``graph_captures`` the captures.  The bytes are
    the same in all three modes.

    Inference only: no autograd graph, and a module in training mode with grad enabled is refused."""

    hip_graphs = False

    def __init__(self, model, batch: int, h: int, w: int, frames: int = 7, emit: int | None = None,
                 channels: int = 1, multiple: int = 32, dtype: str = "u8", device=None):
        from .pipeline import padded_size
        self.frames, self.emit = _check_rule(frames, emit)
        if dtype not in KINDS:
            raise RuntimeError(f"stream: dtype must be one of {KINDS}, got {dtype!r}")
        if int(channels) not in (1, 3, 4) or (dtype == "f32" and int(channels) != 1):
            raise RuntimeError(f"stream: channels must be 1, 3 or 4 (1 for dtype 'f32'), got {channels}")
        if int(batch) < 1 or int(h) < 1 or int(w) < 1 or int(multiple) < 1:
            raise RuntimeError(f"stream: batch, h, w and multiple must be at least 1, got {batch}, {h}, {w}, "
                               f"{multiple}")
        self.model, self.kind = model, dtype
        self.batch, self.h, self.w, self.channels, self.multiple = int(batch), int(h), int(w), int(channels), \
            int(multiple)
        self.H, self.W = padded_size(self.h, self.w, self.multiple) if dtype == "u8" else (self.h, self.w)
        if self.H - self.h >= self.h or self.W - self.w >= self.w:
            raise RuntimeError(f"stream: a {self.h}x{self.w} frame is smaller than its reflect padding to "
                               f"{self.H}x{self.W}")
        m = 1 << model.num_levels
        if self.H % m or self.W % m:
            raise RuntimeError(f"KDLAE_student needs H and W divisible by {m}, got {self.H}x{self.W}")
        if device is None:
            device = next(model.parameters()).device
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("StudentStream (MI355X build) runs on ROCm devices only; there is no CPU fallback: "
                               "move the model with .to()")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        B, F, H, W = self.batch, self.frames, self.H, self.W
        nbytes = _lib.lib().kdlae_stream_state_bytes(B, F, H, W)
        if nbytes < 0:
            _lib.check(2, "kdlae_stream_state_bytes")
        self._state = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
        self._stack = torch.empty((B, F, H, W), dtype=torch.float32, device=self.device)
        self._y = torch.empty((B, F, H, W), dtype=torch.float32, device=self.device)
        self._u8 = torch.empty((B, F, self.h, self.w), dtype=torch.uint8, device=self.device) if dtype == "u8" \
            else None
        fshape = (B, self.h, self.w) + ((self.channels,) if self.channels > 1 else ())
        self._frame = torch.empty(fshape, dtype=torch.uint8 if dtype == "u8" else torch.float32, device=self.device)
        self._frame_shapes = (fshape, fshape + (1,)) if self.channels == 1 and dtype == "u8" else (fshape,)
        self._graph = None         # (CUDAGraph, the pointers it baked in)
        self._graph_failed = False
        self._ran_eager = False    # a full-window push has run launch by launch
        self.graph_replays = 0
        self.graph_captures = 0
        self._t = 0
        self.reset()

    # ------------------------------------------------------------------ the three launches of a push
    def _push_kernel(self, frame):
        L = _lib.lib()
        st = _stream(self.device)
        if self.kind == "u8":
            rc = L.kdlae_stream_push_u8(ctypes.c_void_p(frame.data_ptr()), self.batch, self.h, self.w, self.channels,
                                        self.multiple, self.frames, ctypes.c_void_p(self._state.data_ptr()),
                                        ctypes.c_void_p(self._stack.data_ptr()), st)
            _lib.check(rc, "kdlae_stream_push_u8")
        else:
            rc = L.kdlae_stream_push_f32(ctypes.c_void_p(frame.data_ptr()), self.batch, self.H, self.W, self.frames,
                                         ctypes.c_void_p(self._state.data_ptr()),
                                         ctypes.c_void_p(self._stack.data_ptr()), st)
            _lib.check(rc, "kdlae_stream_push_f32")

    def _advance(self):
        _lib.check(_lib.lib().kdlae_stream_advance(ctypes.c_void_p(self._state.data_ptr()), _stream(self.device)),
                   "kdlae_stream_advance")

    def _to_u8(self, y, out=None):
        from . import clips
        B, f = y.shape[:2]
        return clips.clip_blend_u8(y, B, f, self.h, self.w, f, 0, None, out=out)   # one window: postprocess_u8's rule

    def _chain(self, frame):
        """push -> forward into the static output -> u8 frames -> advance, on the current stream."""
        self._push_kernel(frame)
        self.model._forward_eager(self._stack, out=self._y)
        if self.kind == "u8":
            self._to_u8(self._y, out=self._u8)
        self._advance()

    # ------------------------------------------------------------------ the graph
    def _baked(self):
        eng = self.model.engine(self.device)
        return (eng.ws.data_ptr() if eng.ws is not None else 0, eng.ws.numel() if eng.ws is not None else 0,
                eng.flat.data_ptr() if eng.flat is not None else 0,
                torch.cuda.current_stream(self.device).cuda_stream,
                tuple(t.data_ptr() for t in list(self.model.parameters()) + list(self.model.buffers())))

    def _full_push(self, frame):
        graphed = self.hip_graphs and not self._graph_failed and not torch.cuda.is_current_stream_capturing()
        if not graphed or not self._ran_eager:
            self._chain(frame)
            self._ran_eager = True
            return
        self._frame.copy_(frame.view(self._frame.shape))
        if self._graph is not None and self._graph[1] == self._baked():
            self._graph[0].replay()
            self.graph_replays += 1
            return
        self._graph = None   # never captured, or a pointer the graph baked in has changed since
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize(self.device)
        try:
            # thread_local: HIP calls other threads of the process make meanwhile are not captured and do not fail
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                self._chain(self._frame)
        except RuntimeError:
            self._graph_failed = True   # this stream stays eager; nothing of the capture ran
            torch.cuda.synchronize(self.device)
            self._chain(frame)
            return
        self._graph = (g, self._baked())
        self.graph_captures += 1
        g.replay()

    # ------------------------------------------------------------------ the public calls
    def _check_frame(self, frame):
        want = torch.uint8 if self.kind == "u8" else torch.float32
        if not isinstance(frame, torch.Tensor) or frame.device.type != "cuda" or frame.dtype != want or \
                tuple(frame.shape) not in self._frame_shapes:
            got = f"{frame.dtype} {tuple(frame.shape)} on {frame.device}" if isinstance(frame, torch.Tensor) \
                else type(frame).__name__
            raise RuntimeError(f"StudentStream.push expects a cuda {str(want).replace('torch.', '')} frame "
                               f"{self._frame_shapes[0]}, got {got}")
        if frame.device != self.device:
            raise RuntimeError(f"StudentStream.push: the frame is on {frame.device}, the stream on {self.device}")
        if self.model.training and torch.is_grad_enabled():
            raise RuntimeError("StudentStream is inference only: the module is in training mode with grad enabled "
                               "(call .eval() or push under torch.no_grad())")
        return frame.detach().contiguous()

    def _empty(self):
        shape = (self.batch, 0, self.h, self.w)
        return torch.empty(shape, dtype=torch.uint8 if self.kind == "u8" else torch.float32, device=self.device)

    def push(self, frame: torch.Tensor) -> torch.Tensor:
        """Take the stream's next frame in; return the frames the schedule emits at this push, ``[B,k,h,w]``."""
        frame = self._check_frame(frame)
        F, e, t = self.frames, self.emit, self._t
        with torch.no_grad():
            if t < F - 1:
                self._push_kernel(frame)
                self._advance()
                self._t = t + 1
                return self._empty()
            self._full_push(frame)
            self._t = t + 1
            out = self._u8 if self.kind == "u8" else self._y
            return out[:, :e + 1].clone() if t == F - 1 else out[:, e:e + 1].clone()

    def flush(self) -> torch.Tensor:
        """The frames the stream still owes, ``[B,k,h,w]``, and a reset."""
        F, e, T = self.frames, self.emit, self._t
        with torch.no_grad():
            if T == 0:
                out = self._empty()
            elif T < F:
                # the T frames sit at the stack's last T positions in time order: one forward at T frames
                y = self.model._forward_eager(self._stack[:, F - T:].contiguous())
                out = self._to_u8(y) if self.kind == "u8" else y
            else:
                out = (self._u8 if self.kind == "u8" else self._y)[:, e + 1:].clone()
            self.reset()
        return out

    def reset(self) -> None:
        """Discard the stream's frames: the next push is frame 0.  A captured graph is kept."""
        _lib.check(_lib.lib().kdlae_stream_reset(ctypes.c_void_p(self._state.data_ptr()), _stream(self.device)),
                   "kdlae_stream_reset")
        self._t = 0
