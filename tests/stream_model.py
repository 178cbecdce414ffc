"""Model of streaming inference (include/kdlae.h, streams.py): the rule, the emission schedule derived from it, and
the host loop a user writes without the feature, built from the module's own ``forward`` / ``enhance_frames_u8``.

The rule: frame t of a stream of T frames, with frames = F and 0 <= emit < F, is

    f = min(F, T);  s_t = min(max(t - emit, 0), T - f);  out[:, t] = forward(x[:, s_t : s_t + f])[:, t - s_t]

``schedule`` does not restate streams.stream_schedule's case analysis: it asks, for every frame, at which push its
window is complete (the window's last frame has arrived, and not before the first full window), and groups the
frames by that push; what is left when the stream ends belongs to the flush."""
import torch

EMITS = lambda F: sorted({0, F // 2, F - 1})            # noqa: E731
LENGTHS = lambda F: sorted({0, 1, F - 1, F, F + 1, 2 * F + 3})   # noqa: E731   the ring wraps more than twice
FRAMES = (1, 3, 7)


def window_of(t: int, T: int, F: int, emit: int):
    """-> (f, s_t, position of frame t in its window)."""
    f = min(F, T)
    s = min(max(t - emit, 0), T - f)
    return f, s, t - s


def schedule(T: int, F: int, emit: int):
    """[(push index or "flush", window start or None, positions)], one entry per push and one for the flush."""
    by_call = {}
    for t in range(T):
        f, s, p = window_of(t, T, F, emit)
        # a push can only emit from the window that ends with its frame; the stream's end is not known to a push,
        # so a frame whose window is cut short by the end (or that sits behind position emit of the last window)
        # waits for the flush
        call = s + F - 1 if T >= F and (p == emit or (s == 0 and p < emit)) else "flush"
        assert call == "flush" or t <= call < T
        by_call.setdefault(call, (s, []))
        assert by_call[call][0] == s, "one call emits from one window"
        by_call[call][1].append(p)
    out = []
    for t in range(T):
        s, ps = by_call.get(t, (None, []))
        out.append((t, s, ps))
    s, ps = by_call.get("flush", (None, []))
    out.append(("flush", s, ps))
    return out


def count_per_push(T: int, F: int, emit: int):
    """k of every push as the issue states it: 0 while t < F - 1, emit + 1 at t = F - 1, 1 afterwards."""
    return [0 if t < F - 1 else (emit + 1 if t == F - 1 else 1) for t in range(T)]


# ------------------------------------------------------------------ the host loop (needs the GPU: it runs the module)
def reference_u8(model, clip_u8: torch.Tensor, F: int, emit: int, multiple: int = 32, cache=None) -> torch.Tensor:
    """clip u8 [B,T,h,w(,C)] -> u8 [B,T,h,w]: per frame, ``enhance_frames_u8`` on its window, the frame's position
    taken.  ``cache``: a dict shared between calls on the same clip and weights, keyed by (f, s)."""
    from rethink_acoustic_image_enhancement_amd.pipeline import enhance_frames_u8
    B, T, h, w = clip_u8.shape[:4]
    cache = {} if cache is None else cache
    out = torch.empty((B, T, h, w), dtype=torch.uint8, device=clip_u8.device)
    for t in range(T):
        f, s, p = window_of(t, T, F, emit)
        if (f, s) not in cache:
            cache[(f, s)] = enhance_frames_u8(model, clip_u8[:, s:s + f].contiguous(), multiple)   # [B,h,w,f]
        out[:, t] = cache[(f, s)][..., p]
    return out


def reference_f32(model, x: torch.Tensor, F: int, emit: int, cache=None) -> torch.Tensor:
    """x f32 [B,T,H,W] -> f32 [B,T,H,W]: per frame, ``forward`` on its window, the frame's position taken."""
    B, T, H, W = x.shape
    cache = {} if cache is None else cache
    out = torch.empty_like(x)
    with torch.no_grad():
        for t in range(T):
            f, s, p = window_of(t, T, F, emit)
            if (f, s) not in cache:
                cache[(f, s)] = model(x[:, s:s + f].contiguous())
            out[:, t] = cache[(f, s)][:, p]
    return out


def run_stream(stream, clip) -> torch.Tensor:
    """Push the clip's frames one by one and flush -> every returned tensor concatenated along the frame axis; the
    count of every push is checked against ``count_per_push``."""
    T = clip.shape[1]
    ks = count_per_push(T, stream.frames, stream.emit)
    parts = []
    for t in range(T):
        got = stream.push(clip[:, t])
        assert got.shape[1] == ks[t], (t, got.shape, ks[t])
        parts.append(got)
    parts.append(stream.flush())
    return torch.cat(parts, dim=1)
