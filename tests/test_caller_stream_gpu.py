"""The caller's-stream contract (include/kdlae.h, opening paragraph) on every entry that takes a `stream`:

S1  the call returns while its stream is still held by earlier work: no host wait inside;
S2  run on a non-blocking side stream behind a spin and behind the copies that bring its inputs, it gives the bits
    of a null-stream run: every launch, memset and copy is ordered on the caller's stream, the library's own
    streams wait on it and are joined into it; guards whole, read-only operands unchanged;
S3  the call can be captured into a HIP graph on that stream: nothing runs eagerly, a replay gives the reference's
    bits and a replay on new operand contents gives theirs.

CASES is the table: (id, the entries the case stands for, a factory of its `Call`, the checks, KDLAE_DEBUG).  EXEMPT
names every other entry with the line of the header that states its host wait or host copy;
tests/test_caller_stream.py holds the two against the header.  The checks live in tests/stream_harness.py: bit
equality and event queries, no tolerance."""
import contextlib
import ctypes
import os

import pytest
import torch

from rethink_acoustic_image_enhancement_amd import _lib
from tests import test_workspace_gpu as W
from tests.stream_harness import SPIN, arena_for, check_async_and_order, check_capture, side_stream
from tests.workspace_harness import BIG, DEV, Call, same_bits, stream, vp

pytestmark = pytest.mark.gpu

S12, S3 = "S1+S2", "S3"
DEBUG_REASON = "not on a forward or training path (kdlae.h:877)"

# entries with host operands, or documented to wait: name -> the header line that says so
EXEMPT = {
    "kdlae_t_commit_params": "packs the staged host set, synchronous (kdlae.h:141-142)",
    "kdlae_s_commit_params": "same semantics as the kdlae_t_* calls (kdlae.h:446-447): synchronous (kdlae.h:141-142)",
    "asdqe_commit_params": "same contract as kdlae_t_* (kdlae.h:478-481): synchronous (kdlae.h:141-142)",
    "kdlae_t_set_param": "stages one entry from host memory (kdlae.h:141)",
    "kdlae_s_set_param": "stages one entry from host memory (kdlae.h:141, 446-447)",
    "asdqe_set_param": "stages one entry from host memory (kdlae.h:141, 478-481)",
    "kdlae_t_prepare": "device allocation + one synchronous copy (kdlae.h:146-149)",
    "kdlae_s_prepare": "as kdlae_t_prepare (kdlae.h:451)",
    "asdqe_prepare": "as kdlae_t_prepare (kdlae.h:485)",
    "kdlae_tt_mark_sync": "waits on the host (kdlae.h:571)",
    **{name: "allocates, frees or waits: the promise covers entries that take a stream (kdlae.h:20-21)" for name in (
        "kdlae_t_create", "kdlae_t_create_restormer", "kdlae_t_destroy", "kdlae_s_create", "kdlae_s_destroy",
        "asdqe_create", "asdqe_destroy", "kdlae_tt_create", "kdlae_tt_create_restormer", "kdlae_tt_destroy",
        "kdlae_st_create", "kdlae_st_destroy", "asdqe_train_create", "asdqe_train_destroy")},
    "kdlae_data_sample": "copies its host item table to the device and may wait for the stream (kdlae.h:842-845); "
                         "S2 only: the case data_sample",
    "kdlae_t_debug_sr_fold": "diagnostics of tests/test_sr_fold_gpu.py (kdlae.h:419), " + DEBUG_REASON,
    **{name: DEBUG_REASON for name in (
        "kdlae_debug_tgemm", "kdlae_debug_gemm", "kdlae_debug_gram", "kdlae_debug_ln", "kdlae_debug_small_in",
        "kdlae_debug_bn", "kdlae_debug_head_train", "kdlae_debug_train", "kdlae_debug_train_s", "kdlae_debug_infer")},
}


def L():
    return _lib.lib()


@contextlib.contextmanager
def kdlae_debug(flag):
    """KDLAE_DEBUG set (or unset, flag None) for the block and put back as tests/test_train_s_gpu.py does."""
    old = os.environ.get("KDLAE_DEBUG")
    try:
        if flag:
            os.environ["KDLAE_DEBUG"] = flag
        else:
            os.environ.pop("KDLAE_DEBUG", None)
        yield
    finally:
        if old is None:
            os.environ.pop("KDLAE_DEBUG", None)
        else:
            os.environ["KDLAE_DEBUG"] = old


# ----------------------------------------------------------------------------- operands
def _f(key, shape, lo=0.0, hi=1.0, off=0):
    """A float operand of hash values; off: its base sits `off` floats past a 256-byte boundary (the element paths)."""
    n = 1
    for d in shape:
        n *= d
    buf = torch.empty(n + off, dtype=torch.float32, device=DEV)
    t = buf[off:].view(shape)
    t.copy_(W._images("cs:" + key, shape, lo, hi))
    return t


def _u8(key, shape, off=0):
    n = 1
    for d in shape:
        n *= d
    buf = torch.empty(n + off, dtype=torch.uint8, device=DEV)
    t = buf[off:].view(shape)
    t.copy_(W._images("cs:" + key, shape, 0.0, 256.0).floor().clamp(0, 255).to(torch.uint8))
    return t


def _i32(values):
    return torch.tensor(values, dtype=torch.int32, device=DEV)


def _words(nbytes):
    return (nbytes + 3) // 4


def _padded(h, w, multiple):
    H, Wd = ctypes.c_int(), ctypes.c_int()
    L().kdlae_padded_size(h, w, multiple, ctypes.byref(H), ctypes.byref(Wd))
    return H.value, Wd.value


class Simple(Call):
    """A stateless entry (or a short sequence of them): `make(operands, outs, ws)` lists (name, thunk -> rc)."""

    def __init__(self, operands, out_numels, make, ws_bytes=0):
        self.operands, self.out_numels, self.make = operands, tuple(out_numels), make
        self.ws_bytes = (ws_bytes + 255) // 256 * 256

    def steps(self, arena):
        return [(name, (lambda nbytes, fn=fn: fn())) for name, fn in self.make(self.operands, arena.outs, arena.ws)]


def _copy(dst, src):
    """In/out state is put back to its start as a step of its own, on the stream (and in the graph) of the call."""
    def step():
        dst.copy_(src.reshape(dst.shape), non_blocking=True)
        return 0
    return ("restore", step)


# ----------------------------------------------------------------------------- handle-based calls
class TPackForward(W.TForward):
    """kdlae_t_pack_device from the device parameter vector, then kdlae_t_forward: the Python path's forward"""

    def steps(self, arena):
        return [("kdlae_t_pack_device", lambda nbytes: L().kdlae_t_pack_device(
            self.eng.handle, vp(self.eng.flat), self.eng.numel, stream()))] + super().steps(arena)


class SPackForward(W.SForward):
    def steps(self, arena):
        return [("kdlae_s_pack_device", lambda nbytes: L().kdlae_s_pack_device(
            self.eng.handle, vp(self.eng.flat), self.eng.numel, stream()))] + super().steps(arena)


class APackForward(W.AForward):
    def steps(self, arena):
        return [("asdqe_pack_device", lambda nbytes: L().asdqe_pack_device(
            self.eng.handle, vp(self.eng.flat), self.eng.numel, stream()))] + super().steps(arena)


def _s_model():
    return W._student("s_default_b2")                  # hidden_channels [16, 32, 64]


def _s_smallest():
    return W._student_shapes(_s_model())[0]


# ----------------------------------------------------------------------------- stateless calls
def rate_select(mode, per, off):
    R, B = 3, 2
    o = {"scores": _f("rs:scores", (R, B)), "target": _f("rs:target", (B,)), "hq": _f("rs:hq", (R, B, per), off=off)}

    def make(o, outs, ws):
        return [("kdlae_rate_select", lambda: L().kdlae_rate_select(
            vp(o["scores"]), R, B, mode, vp(o["target"]) if mode == 0 else None, vp(o["hq"]), per, vp(outs[0]),
            vp(outs[1]), stream()))]
    return Simple(o, (B, B * per), make)


TILE = dict(B=1, C=3, H=24, W=40, tile=16, overlap=8)      # 2 x 4 tiles of 16 x 16, two of them share every seam


def _tile_plan():
    v = [ctypes.c_int() for _ in range(6)]
    rc = L().kdlae_tile_plan(TILE["H"], TILE["W"], TILE["tile"], TILE["overlap"], *[ctypes.byref(x) for x in v])
    assert rc == 0, _lib.last_error()
    th, tw, ni, nj = (x.value for x in v[:4])
    return th, tw, ni, nj


def tile_gather(off):
    B, C, H, Wd, tile, ov = (TILE[k] for k in ("B", "C", "H", "W", "tile", "overlap"))
    th, tw, ni, nj = _tile_plan()
    first, count = 1, B * ni * nj - 2
    o = {"src": _f("tile:src", (B, C, H, Wd), off=off)}

    def make(o, outs, ws):
        return [("kdlae_tile_gather", lambda: L().kdlae_tile_gather(
            vp(o["src"]), B, C, H, Wd, tile, ov, first, count, vp(outs[0]), stream()))]
    return Simple(o, (count * C * th * tw,), make)


def tile_blend(kind, scale, off):
    """kind: '', 'rates', 'w', 'rates_w'"""
    B, C, H, Wd, tile, ov = (TILE[k] for k in ("B", "C", "H", "W", "tile", "overlap"))
    th, tw, ni, nj = _tile_plan()
    R, tb = (2, 3) if "rates" in kind else (1, 0)
    n, T = B * ni * nj, C * scale * scale * th * tw
    o = {"tiles": _f(f"tile:{kind}:tiles", (R * n, T), off=off)}
    if kind.endswith("w"):
        o["wy"] = _f("tile:wy", (scale * th,), 0.25, 1.0)
        o["wx"] = _f("tile:wx", (scale * tw,), 0.25, 1.0)
    name = "kdlae_tile_blend" + ("_" + kind if kind else "")

    def make(o, outs, ws):
        head = (vp(o["tiles"]),) + ((R,) if R > 1 else ()) + (B, C, H, Wd, tile, ov) + ((tb,) if R > 1 else ())
        tables = (vp(o["wy"]), vp(o["wx"])) if "wy" in o else ()
        return [(name, lambda: getattr(L(), name)(*head, scale, *tables, vp(outs[0]), stream()))]
    return Simple(o, (R * B * C * scale * H * scale * Wd,), make)


CLIP = dict(B=1, T=7, H=8, W=12, frames=3, overlap=1)      # three windows of three frames, one shared frame a seam


def _clip_plan():
    v = [ctypes.c_int() for _ in range(3)]
    assert L().kdlae_clip_plan(CLIP["T"], CLIP["frames"], CLIP["overlap"], *[ctypes.byref(x) for x in v]) == 0
    return v[0].value, v[1].value


def clip_gather(off):
    B, T, H, Wd, fr, ov = (CLIP[k] for k in ("B", "T", "H", "W", "frames", "overlap"))
    f, n = _clip_plan()
    o = {"src": _f("clip:src", (B, T, H, Wd), off=off)}

    def make(o, outs, ws):
        return [("kdlae_clip_gather", lambda: L().kdlae_clip_gather(
            vp(o["src"]), B, T, H, Wd, fr, ov, 0, B * n, vp(outs[0]), stream()))]
    return Simple(o, (B * n * f * H * Wd,), make)


def clip_blend(weighted, off):
    B, T, H, Wd, fr, ov = (CLIP[k] for k in ("B", "T", "H", "W", "frames", "overlap"))
    f, n = _clip_plan()
    o = {"windows": _f("clip:windows", (B * n, f, H, Wd), off=off)}
    if weighted:
        o["wt"] = _f("clip:wt", (f,), 0.25, 1.0)

    def make(o, outs, ws):
        return [("kdlae_clip_blend", lambda: L().kdlae_clip_blend(
            vp(o["windows"]), B, T, H, Wd, fr, ov, vp(o.get("wt")), vp(outs[0]), stream()))]
    return Simple(o, (B * T * H * Wd,), make)


def clip_blend_u8(h, w, off):
    B, T, H, Wd, fr, ov = (CLIP[k] for k in ("B", "T", "H", "W", "frames", "overlap"))
    f, n = _clip_plan()
    o = {"windows": _f("clip:windows8", (B * n, f, H, Wd), -0.25, 1.25, off=off), "wt": _f("clip:wt", (f,), 0.25, 1.0)}

    def make(o, outs, ws):
        return [("kdlae_clip_blend_u8", lambda: L().kdlae_clip_blend_u8(
            vp(o["windows"]), B, T, H, Wd, h, w, fr, ov, vp(o["wt"]), vp(outs[0]), stream()))]
    return Simple(o, (_words(B * T * h * w),), make)


def live_stream():
    """reset, then F + 2 pushes (u8 and f32 in turn), each followed by an advance: the device counter picks the ring
    slot, so the final ring and stack depend on every launch having run in order."""
    B, F, h, w, ch, mult = 2, 3, 13, 16, 3, 8
    H, Wd = _padded(h, w, mult)
    pushes = F + 2
    o = {"u8": _u8("live:u8", (pushes, B, h, w, ch)), "f32": _f("live:f32", (pushes, B, H, Wd))}
    nstate = int(L().kdlae_stream_state_bytes(B, F, H, Wd))
    assert nstate > 0 and nstate % 4 == 0

    def make(o, outs, ws):
        state, stack = outs
        steps = [("kdlae_stream_reset", lambda: L().kdlae_stream_reset(vp(state), stream()))]
        for i in range(pushes):
            if i % 2 == 0:
                steps.append(("kdlae_stream_push_u8", lambda i=i: L().kdlae_stream_push_u8(
                    vp(o["u8"][i]), B, h, w, ch, mult, F, vp(state), vp(stack), stream())))
            else:
                steps.append(("kdlae_stream_push_f32", lambda i=i: L().kdlae_stream_push_f32(
                    vp(o["f32"][i]), B, H, Wd, F, vp(state), vp(stack), stream())))
            steps.append(("kdlae_stream_advance", lambda: L().kdlae_stream_advance(vp(state), stream())))
        return steps
    return Simple(o, (nstate // 4, B * F * H * Wd), make)


def distill_expand_u8(w, mult, off):
    """(16, 8): W = 16, the float4 launch; (15, 1): no padding, W = 15, the element launch"""
    B, F, h, ch = 1, 2, 13, 3
    H, Wd = _padded(h, w, mult)
    n = B * F
    o = {"frames": _u8("dist:frames", (B, F, h, w, ch), off=off), "rate": _f("dist:rate", (n,))}

    def make(o, outs, ws):
        return [("kdlae_distill_expand_u8", lambda: L().kdlae_distill_expand_u8(
            vp(o["frames"]), B, F, h, w, ch, mult, vp(o["rate"]), 0, n, vp(outs[0]), vp(outs[1]), stream()))]
    return Simple(o, (n * 3 * H * Wd, n * H * Wd), make)


def distill_expand_f32(off):
    B, F, H, Wd = 1, 2, 16, 16
    n = B * F
    o = {"frames": _f("dist:frames32", (B, F, H, Wd), off=off), "rate": _f("dist:rate", (n,))}

    def make(o, outs, ws):
        return [("kdlae_distill_expand_f32", lambda: L().kdlae_distill_expand_f32(
            vp(o["frames"]), B, F, H, Wd, vp(o["rate"]), 0, n, vp(outs[0]), vp(outs[1]), stream()))]
    return Simple(o, (n * 3 * H * Wd, n * H * Wd), make)


def distill_collapse(mode, dst_u8, w, off):
    """mode 0 = KDLAE_DISTILL_FILE (with the black mask of a BGR source), 1 = KDLAE_DISTILL_MEAN"""
    B, F, Hp, Wp, h = 1, 2, 16, 16, 13
    n = B * F
    o = {"hq": _f("dist:hq", (n, 3, Hp, Wp), -0.25, 1.25, off=off)}
    if mode == 0:
        o["src"] = _u8("dist:src", (B, F, h, w, 3))
        o["src"][:, :, ::3, 1::2] = 0               # black source pixels: the mask has something to do

    def make(o, outs, ws):
        return [("kdlae_distill_collapse", lambda: L().kdlae_distill_collapse(
            vp(o["hq"]), B, F, Hp, Wp, h, w, 0, n, mode, vp(o.get("src")), 3 if mode == 0 else 1, vp(outs[0]), dst_u8,
            stream()))]
    return Simple(o, (_words(n * h * w) if dst_u8 else n * h * w,), make)


def preprocess_u8():
    B, h, w, ch, mult = 2, 13, 16, 3, 8
    H, Wd = _padded(h, w, mult)
    o = {"images": _u8("pre:images", (B, h, w, ch)), "rate": _f("pre:rate", (B,))}

    def make(o, outs, ws):
        return [("kdlae_preprocess_u8", lambda: L().kdlae_preprocess_u8(
            vp(o["images"]), B, h, w, ch, 1, mult, vp(o["rate"]), vp(outs[0]), vp(outs[1]), stream()))]
    return Simple(o, (B * 3 * H * Wd, B * H * Wd), make)


def frames_preprocess_u8():
    B, F, h, w, ch, mult = 1, 3, 13, 16, 3, 8
    H, Wd = _padded(h, w, mult)
    o = {"frames": _u8("pre:frames", (B, F, h, w, ch))}

    def make(o, outs, ws):
        return [("kdlae_frames_preprocess_u8", lambda: L().kdlae_frames_preprocess_u8(
            vp(o["frames"]), B, F, h, w, ch, mult, vp(outs[0]), stream()))]
    return Simple(o, (B * F * H * Wd,), make)


def postprocess_u8():
    B, C, Hs, Ws, h, w = 1, 3, 16, 16, 13, 16
    o = {"out": _f("post:out", (B, C, Hs, Ws), -0.25, 1.25), "lq": _u8("post:lq", (B, h, w, 3))}
    o["lq"][:, ::3, 1::2] = 0

    def make(o, outs, ws):
        return [("kdlae_postprocess_u8", lambda: L().kdlae_postprocess_u8(
            vp(o["out"]), B, C, Hs, Ws, h, w, 1, vp(o["lq"]), 3, vp(outs[0]), stream()))]
    return Simple(o, (_words(B * h * w * C),), make)


def metric_psnr():
    B, C, Hs, Ws, Hg, Wg, h, w = 2, 3, 16, 16, 13, 16, 13, 16
    o = {"pred": _f("psnr:pred", (B, C, Hs, Ws)), "gt": _f("psnr:gt", (B, C, Hg, Wg))}

    def make(o, outs, ws):
        return [("kdlae_metric_psnr", lambda: L().kdlae_metric_psnr(
            vp(o["pred"]), vp(o["gt"]), B, C, Hs, Ws, Hg, Wg, h, w, 1, 1, vp(outs[0]), vp(ws), stream()))]
    return Simple(o, (2 * B * 2,), make, int(L().kdlae_metric_scratch_bytes()))


def metric_ssim(variant):
    B, C, Hs, Ws, Hg, Wg, h, w = 2, 3, 16, 16, 13, 16, 13, 16
    o = {"pred": _f("ssim:pred", (B, C, Hs, Ws)), "gt": _f("ssim:gt", (B, C, Hg, Wg))}

    def make(o, outs, ws):
        return [("kdlae_metric_ssim", lambda: L().kdlae_metric_ssim(
            vp(o["pred"]), vp(o["gt"]), B, C, Hs, Ws, Hg, Wg, h, w, 0, 0, variant, vp(outs[0]), vp(ws), stream()))]
    return Simple(o, (2 * B * 4,), make, int(L().kdlae_metric_ssim_scratch_bytes()))


def metric_niqe():
    """96 x 96: the smallest image the entry takes (one block at each scale)"""
    B, C, n = 1, 1, 96
    o = {"x": _f("niqe:x", (B, C, n, n), 0.0, 255.0)}
    taps = [2.718281828 ** (-((i - 3) ** 2 + (j - 3) ** 2) / (2 * (7 / 6) ** 2)) for i in range(7) for j in range(7)]
    window = (ctypes.c_double * 49)(*[t / sum(taps) for t in taps])      # host operand, read inside the call
    nbytes = int(L().kdlae_metric_niqe_scratch_bytes(B, n, n))

    def make(o, outs, ws):
        return [("kdlae_metric_niqe", lambda: L().kdlae_metric_niqe(
            vp(o["x"]), B, C, n, n, n, n, 0, 0, 0, window, vp(outs[0]), vp(outs[1]), vp(outs[2]), vp(ws), nbytes,
            stream()))]
    return Simple(o, (2 * B * 2 * 5 * 5, B * n * n, B * n * n // 4), make, nbytes)


def train_l1sr():
    n = 2 * 3 * 16 * 16
    o = {"pred_hq": _f("l1sr:p", (n,)), "gt_hq": _f("l1sr:g", (n,)), "pred_sr": _f("l1sr:ps", (4 * n,)),
         "gt_sr": _f("l1sr:gs", (4 * n,))}

    def make(o, outs, ws):
        return [("kdlae_train_l1sr", lambda: L().kdlae_train_l1sr(
            vp(o["pred_hq"]), vp(o["gt_hq"]), n, vp(o["pred_sr"]), vp(o["gt_sr"]), 4 * n, vp(outs[0]), vp(outs[1]),
            vp(outs[2]), vp(ws), stream()))]
    return Simple(o, (n, 4 * n, 1), make, 4 * int(L().kdlae_train_l1sr_scratch_floats()))


def train_l1sonar(n, off):
    o = {"pred": _f("sonar:p", (n,), off=off), "target": _f("sonar:t", (n,))}

    def make(o, outs, ws):
        return [("kdlae_train_l1sonar", lambda: L().kdlae_train_l1sonar(
            vp(o["pred"]), vp(o["target"]), n, 1.0, 0.1, 0, None, vp(outs[0]), vp(outs[1]), vp(ws), stream()))]
    return Simple(o, (n, 1), make, 4 * int(L().kdlae_train_l1sonar_scratch_floats()))


def train_l1frames():
    N, frames, hw = 2, 3, 64
    o = {"pred": _f("l1f:p", (N, frames, hw)), "target": _f("l1f:t", (N, frames, hw))}

    def make(o, outs, ws):
        return [("kdlae_train_l1frames", lambda: L().kdlae_train_l1frames(
            vp(o["pred"]), vp(o["target"]), N, frames, hw, 0.9, 0.1, 0.1, 0, vp(outs[0]), vp(outs[1]), vp(ws),
            stream()))]
    return Simple(o, (N * frames * hw, 1), make, 4 * int(L().kdlae_train_l1frames_scratch_floats()))


def train_mse():
    n = 5
    o = {"score": _f("mse:s", (n,), -1.0, 1.0), "target": _f("mse:t", (n,))}

    def make(o, outs, ws):
        return [("kdlae_train_mse", lambda: L().kdlae_train_mse(
            vp(o["score"]), vp(o["target"]), n, 0.5, vp(outs[0]), vp(outs[1]), stream()))]
    return Simple(o, (n, 2), make)


def train_clip_adamw(n):
    """theta, exp_avg and exp_avg_sq are in/out: they are the outputs, restored from read-only copies first"""
    o = {"theta0": _f("adamw:theta", (n,), -1.0, 1.0), "m0": _f("adamw:m", (n,), -0.01, 0.01),
         "v0": _f("adamw:v", (n,), 0.0, 1e-4), "grad": _f("adamw:g", (n,), -0.1, 0.1)}

    def make(o, outs, ws):
        theta, m, v = outs
        return [_copy(theta, o["theta0"]), _copy(m, o["m0"]), _copy(v, o["v0"]),
                ("kdlae_train_clip_adamw", lambda: L().kdlae_train_clip_adamw(
                    vp(theta), vp(o["grad"]), vp(m), vp(v), n, 0.5, 0.01, 3e-4, 0.9, 0.999, 1e-8, 1e-4, 3, None, 0,
                    vp(ws), stream()))]
    return Simple(o, (n, n, n), make, 4 * int(L().kdlae_train_adamw_scratch_floats()))


def train_mixup():
    B, per = 3, 3 * 16 * 16
    o = {"in": _f("mix:in", (B, per)), "perm": _i32([2, 0, 1])}

    def make(o, outs, ws):
        return [("kdlae_train_mixup", lambda: L().kdlae_train_mixup(
            vp(o["in"]), vp(outs[0]), B, per, vp(o["perm"]), 0.3, stream()))]
    return Simple(o, (B * per,), make)


def train_ema(n):
    o = {"ema0": _f("ema:ema", (n,), -1.0, 1.0), "theta": _f("ema:theta", (n,), -1.0, 1.0)}

    def make(o, outs, ws):
        return [_copy(outs[0], o["ema0"]),
                ("kdlae_train_ema", lambda: L().kdlae_train_ema(vp(outs[0]), vp(o["theta"]), n, 0.9, stream()))]
    return Simple(o, (n,), make)


def train_prepare():
    """one segment: two of three source images, an 8 x 8 window at (3, 5), the Philox input mask at 0.5"""
    Bs, C, Hs, Ws, B, h, w = 3, 3, 16, 16, 2, 8, 8
    o = {"src": _f("prep:src", (Bs, C, Hs, Ws)), "index": _i32([2, 0])}
    segs = (_lib.PrepSeg * 1)()                                           # host operand, read inside the call

    def make(o, outs, ws):
        def call():
            segs[0] = _lib.PrepSeg(o["src"].data_ptr(), outs[0].data_ptr(), Bs, C, Hs, Ws, h, w, 3, 5, 0.5, None)
            return L().kdlae_train_prepare(segs, 1, vp(o["index"]), B, 0.5, 1234, 7, stream())
        return [("kdlae_train_prepare", call)]
    return Simple(o, (B * C * h * w,), make)


def train_mask_frames():
    B, F, H, Wd = 1, 3, 8, 8
    o = {"src": _f("maskf:src", (B, F, H, Wd))}
    probs = (ctypes.c_float * F)(0.3, 0.0, 0.6)                           # host operand, read inside the call

    def make(o, outs, ws):
        return [("kdlae_train_mask_frames", lambda: L().kdlae_train_mask_frames(
            vp(o["src"]), vp(outs[0]), B, F, H, Wd, probs, 1, 0.5, None, 99, 3, stream()))]
    return Simple(o, (B * F * H * Wd,), make)


def data_count_finish():
    """x is in/out: restored, counted (the zero fill of counts and the count kernel), finished with counts' verdict.
    B = 3: counts is 24 bytes, no multiple of 16, so its zero fill is the library's 4-byte one (every other zero
    fill in the suite is the 16-byte one)"""
    B, C, hw = 3, 3, 64
    x0 = _f("data:x", (B, C, hw))
    x0[0] = (x0[0] > 0.3).float()                                         # mostly exact ones and zeros: above thr
    o = {"x0": x0, "mean": _f("data:mean", (C,)), "std": _f("data:std", (C,), 0.5, 1.5)}

    def make(o, outs, ws):
        x, counts = outs
        return [_copy(x, o["x0"]),
                ("kdlae_data_count", lambda: L().kdlae_data_count(vp(x), B, C * hw, vp(counts), stream())),
                ("kdlae_data_finish", lambda: L().kdlae_data_finish(
                    vp(x), B, C, hw, vp(counts), 0.5, 0.25, vp(o["mean"]), vp(o["std"]), stream()))]
    return Simple(o, (B * C * hw, 2 * B), make)


def data_sample():
    """one CHW fp32 item: a 12 x 10 window of a 16 x 16 image, flipped and transposed, channels reversed"""
    C, Hs, Ws, h, w = 3, 16, 16, 12, 10
    o = {"src": _f("data:src", (C, Hs, Ws))}
    items = (_lib.DataItem * 1)()                                         # host table, copied inside the call

    def make(o, outs, ws):
        def call():
            it = _lib.DataItem()
            it.src, it.dst = o["src"].data_ptr(), outs[0].data_ptr()
            it.sy, it.sx, it.sc = Ws, 1, Hs * Ws
            it.Hs, it.Ws, it.C, it.Hc, it.Wc, it.Hp, it.Wp = Hs, Ws, C, Hs, Ws, Hs, Ws
            it.top, it.left, it.h, it.w, it.dihedral, it.reverse_c = 2, 3, h, w, 5, 1
            items[0] = it
            return L().kdlae_data_sample(items, vp(ws), 1, 5, 9, stream())
        return [("kdlae_data_sample", call)]
    return Simple(o, (C * h * w,), make, ctypes.sizeof(_lib.DataItem))


# ----------------------------------------------------------------------------- the table
def _case(cid, names, factory, checks=(S12, S3), debug=None):
    return (cid, tuple(names.split()), factory, checks, debug)


def _train_cases():
    """The training steps whose backward forks a library stream, with the fork (the default) and without it.  Under
    capture the default backward keeps every launch on the caller's stream, as train_serial does (the side stream
    and the handle's events are never drawn into a caller's graph, include/kdlae.h), so S3 of the default variant
    captures the one-stream launches between eager runs that fork."""
    out = []
    for tag, debug in (("fork", None), ("serial", "train_serial")):
        out += [
            _case(f"tt-default-{tag}", "kdlae_tt_forward kdlae_tt_backward",
                  lambda: W.TTStep("default", *W.TT_CONFIGS["default"][1]), debug=debug),
            _case(f"tt-dim16-{tag}", "kdlae_tt_forward kdlae_tt_backward",
                  lambda: W.TTStep("dim16", *W.TT_CONFIGS["dim16"][1]), debug=debug),
            # the marks are handle-owned events for the host and other streams: capture is refused
            # (test_marked_backward_refuses_capture)
            _case(f"tt-default-marked-{tag}", "kdlae_tt_forward kdlae_tt_backward_marked",
                  lambda: W.TTStep("default", *W.TT_CONFIGS["default"][1], marked=True), checks=(S12,), debug=debug),
            _case(f"st-s3-{tag}", "kdlae_st_forward kdlae_st_backward",
                  lambda: W.STStep("s3", *W.ST_SHAPES[0]), debug=debug),
        ]
    return out


CASES = [
    # KDLAE-T: 24 x 16 is the smallest H != W; at 64 x 64 every fused C = 48 / 96 kernel applies
    _case("t-default-1x24x16", "kdlae_t_forward", lambda: W.TForward(W._teacher("default"), 1, 24, 16)),
    _case("t-default-1x64x64", "kdlae_t_forward", lambda: W.TForward(W._teacher("default"), 1, 64, 64)),
    _case("t-dim16-1x24x16", "kdlae_t_forward", lambda: W.TForward(W._teacher("dim16"), 1, 24, 16)),
    _case("t-dim16-1x64x64", "kdlae_t_forward", lambda: W.TForward(W._teacher("dim16"), 1, 64, 64)),
    _case("t-pack-forward-1x64x64", "kdlae_t_pack_device kdlae_t_forward",
          lambda: TPackForward(W._teacher("default"), 1, 64, 64)),
    _case("t-sr-1x24x16", "kdlae_t_forward_sr", lambda: W.TSr(W._teacher("default"), 1, 24, 16)),
    _case("t-rates-scalars", "kdlae_t_forward_rates", lambda: W.TRates(W._teacher("default"), 3, 3, 16, 24, 0)),
    _case("t-rates-maps", "kdlae_t_forward_rates", lambda: W.TRates(W._teacher("default"), 3, 3, 16, 24, 1)),
    _case("s-forward", "kdlae_s_forward", lambda: W.SForward(_s_model(), *_s_smallest())),
    _case("s-pack-forward", "kdlae_s_pack_device kdlae_s_forward", lambda: SPackForward(_s_model(), *_s_smallest())),
    _case("a-forward-2x37x50", "asdqe_forward", lambda: W.AForward(W._asdqe(), 2, 37, 50, True)),
    _case("a-pack-forward-2x37x50", "asdqe_pack_device asdqe_forward",
          lambda: APackForward(W._asdqe(), 2, 37, 50, False)),
    *_train_cases(),
    _case("at-2x40x56", "asdqe_train_forward asdqe_train_backward", lambda: W.ATStep(2, 40, 56, True)),
    # stateless entries: "vec" = every pointer on 16 bytes (the float4 launch), "elem" = a source 4 bytes past it
    _case("rate-select-nearest-vec", "kdlae_rate_select", lambda: rate_select(0, 3 * 16 * 16, 0)),
    _case("rate-select-argmax-elem", "kdlae_rate_select", lambda: rate_select(1, 37, 1)),
    _case("tile-gather-vec", "kdlae_tile_gather", lambda: tile_gather(0)),
    _case("tile-gather-elem", "kdlae_tile_gather", lambda: tile_gather(1)),
    _case("tile-blend-vec", "kdlae_tile_blend", lambda: tile_blend("", 2, 0)),
    _case("tile-blend-elem", "kdlae_tile_blend", lambda: tile_blend("", 1, 1)),
    _case("tile-blend-rates-vec", "kdlae_tile_blend_rates", lambda: tile_blend("rates", 1, 0)),
    _case("tile-blend-rates-elem", "kdlae_tile_blend_rates", lambda: tile_blend("rates", 2, 1)),
    _case("tile-blend-w-vec", "kdlae_tile_blend_w", lambda: tile_blend("w", 2, 0)),
    _case("tile-blend-w-elem", "kdlae_tile_blend_w", lambda: tile_blend("w", 1, 1)),
    _case("tile-blend-rates-w-vec", "kdlae_tile_blend_rates_w", lambda: tile_blend("rates_w", 1, 0)),
    _case("tile-blend-rates-w-elem", "kdlae_tile_blend_rates_w", lambda: tile_blend("rates_w", 2, 1)),
    _case("clip-gather-vec", "kdlae_clip_gather", lambda: clip_gather(0)),
    _case("clip-gather-elem", "kdlae_clip_gather", lambda: clip_gather(1)),
    _case("clip-blend-uniform-vec", "kdlae_clip_blend", lambda: clip_blend(False, 0)),
    _case("clip-blend-weighted-elem", "kdlae_clip_blend", lambda: clip_blend(True, 1)),
    _case("clip-blend-u8-vec", "kdlae_clip_blend_u8", lambda: clip_blend_u8(8, 12, 0)),
    _case("clip-blend-u8-elem", "kdlae_clip_blend_u8", lambda: clip_blend_u8(7, 11, 1)),
    _case("live-stream", "kdlae_stream_reset kdlae_stream_push_u8 kdlae_stream_push_f32 kdlae_stream_advance",
          live_stream),
    _case("distill-expand-u8-vec", "kdlae_distill_expand_u8", lambda: distill_expand_u8(16, 8, 0)),
    _case("distill-expand-u8-elem", "kdlae_distill_expand_u8", lambda: distill_expand_u8(15, 1, 1)),
    _case("distill-expand-f32-vec", "kdlae_distill_expand_f32", lambda: distill_expand_f32(0)),
    _case("distill-expand-f32-elem", "kdlae_distill_expand_f32", lambda: distill_expand_f32(1)),
    _case("distill-collapse-file-u8-vec", "kdlae_distill_collapse", lambda: distill_collapse(0, 1, 16, 0)),
    _case("distill-collapse-file-f32-elem", "kdlae_distill_collapse", lambda: distill_collapse(0, 0, 15, 1)),
    _case("distill-collapse-mean-vec", "kdlae_distill_collapse", lambda: distill_collapse(1, 0, 16, 0)),
    _case("preprocess-u8", "kdlae_preprocess_u8", preprocess_u8),
    _case("frames-preprocess-u8", "kdlae_frames_preprocess_u8", frames_preprocess_u8),
    _case("postprocess-u8", "kdlae_postprocess_u8", postprocess_u8),
    _case("metric-psnr", "kdlae_metric_psnr", metric_psnr),
    _case("metric-ssim-3d", "kdlae_metric_ssim", lambda: metric_ssim(0)),
    _case("metric-ssim-2d", "kdlae_metric_ssim", lambda: metric_ssim(1)),
    _case("metric-niqe", "kdlae_metric_niqe", metric_niqe),
    _case("train-l1sr", "kdlae_train_l1sr", train_l1sr),
    _case("train-l1sonar-vec", "kdlae_train_l1sonar", lambda: train_l1sonar(1536, 0)),
    _case("train-l1sonar-elem", "kdlae_train_l1sonar", lambda: train_l1sonar(1537, 1)),
    _case("train-l1frames", "kdlae_train_l1frames", train_l1frames),
    _case("train-mse", "kdlae_train_mse", train_mse),
    _case("train-clip-adamw-vec", "kdlae_train_clip_adamw", lambda: train_clip_adamw(4096)),
    _case("train-clip-adamw-elem", "kdlae_train_clip_adamw", lambda: train_clip_adamw(4099)),
    _case("train-mixup", "kdlae_train_mixup", train_mixup),
    _case("train-ema-vec", "kdlae_train_ema", lambda: train_ema(4096)),
    _case("train-ema-elem", "kdlae_train_ema", lambda: train_ema(4099)),
    _case("train-prepare", "kdlae_train_prepare", train_prepare),
    _case("train-mask-frames", "kdlae_train_mask_frames", train_mask_frames),
    _case("data-count-finish", "kdlae_data_count kdlae_data_finish", data_count_finish),
    # documented to copy a host table on the stream (EXEMPT): its result must not depend on the stream it is given
    _case("data-sample", "kdlae_data_sample", data_sample, checks=("S2",)),
]
# the marked backward's suffix invariant on a side stream: test_marks_fire_after_their_suffix_is_final_on_a_side_stream
MARK_CASE = ("tt-marks-1x64x64", ("kdlae_tt_forward", "kdlae_tt_backward_marked", "kdlae_tt_mark_wait"))


def covered():
    """Every entry the table (and the mark case) stands for."""
    return {n for _, names, _, checks, _ in CASES if checks != ("S2",) for n in names} | set(MARK_CASE[1])


def _ids(check):
    return [pytest.param(c, id=c[0]) for c in CASES if check in c[3]]


@pytest.mark.parametrize("case", _ids(S12))
def test_asynchrony_and_order_on_a_side_stream(case):
    _, _, factory, _, debug = case
    with kdlae_debug(debug):
        check_async_and_order(factory())


@pytest.mark.parametrize("case", _ids("S2"))
def test_order_on_a_side_stream_of_an_entry_that_may_wait(case):
    _, _, factory, _, debug = case
    with kdlae_debug(debug):
        check_async_and_order(factory(), check_async=False)


@pytest.mark.parametrize("case", _ids(S3))
def test_graph_capture_on_a_side_stream(case):
    _, _, factory, _, debug = case
    with kdlae_debug(debug):
        check_capture(factory())


@pytest.mark.parametrize("debug", [None, "train_serial"], ids=["fork", "serial"])
def test_marks_fire_after_their_suffix_is_final_on_a_side_stream(debug):
    """test_train_gpu.test_mark_events_fire_after_their_suffix_is_final with the caller's stream a non-blocking side
    stream held by a spin: a second stream waits on every gradient-ready event (kdlae_tt_mark_wait) and copies the
    suffix at that moment; every snapshot equals the finished gradient, which has the null-stream reference's
    bits, and the snapshots were enqueued while the backward was still in flight."""
    with kdlae_debug(debug):
        call = W.TTStep("default", 1, 64, 64, marked=True)
        arena = arena_for(call)
        arena.fill(BIG)
        ref = call.run(arena, "reference")                 # also sizes the marks
        h, grad = call.eng.handle, arena.outs[2]
        n = L().kdlae_tt_mark_count(h)
        los = [int(L().kdlae_tt_mark_lo(h, j)) for j in range(n)]
        assert n > 0 and los[-1] == 0
        snaps = [torch.empty(call.eng.numel - lo, device=DEV) for lo in los]
        s, reader = side_stream(), torch.cuda.Stream(device=DEV)
        done = torch.cuda.Event()
        arena.fill(BIG)
        grad.fill_(float("nan"))         # a snapshot of a not-yet-zeroed or unwritten range shows up as NaN
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            torch.cuda._sleep(SPIN)
            for name, fn in call.steps(arena):
                rc = fn(arena.ws_bytes)
                assert rc == 0, f"{name}: {_lib.last_error()}"
            done.record()
        for j, lo in enumerate(los):
            _lib.check(L().kdlae_tt_mark_wait(h, j, ctypes.c_void_p(reader.cuda_stream)), "kdlae_tt_mark_wait")
            with torch.cuda.stream(reader):
                snaps[j].copy_(grad[lo:], non_blocking=True)
        in_flight = not done.query()
        torch.cuda.synchronize()
        assert same_bits(grad, ref[2]), "the gradient on the side stream differs from the null-stream reference"
        bad = [j for j, lo in enumerate(los) if not same_bits(snaps[j], grad[lo:])]
        assert not bad, f"marks {bad[:5]} of {n} fired before their suffix was final"
        assert in_flight
        arena.assert_guards("marked backward")


def test_marked_backward_refuses_capture():
    """kdlae_tt_backward_marked records handle-owned events; under capture it is refused with KDLAE_ESTATE before it
    launches or records anything, and the handle then runs an eager step with the reference's bits."""
    call = W.TTStep("default", 1, 24, 16, marked=True)
    arena = arena_for(call)
    arena.fill(BIG)
    ref = call.run(arena, "reference")
    s = side_stream()
    arena.fill(BIG)
    torch.cuda.synchronize()
    (fwd_name, fwd), (bwd_name, bwd) = call.steps(arena)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s, capture_error_mode="thread_local"):
        assert fwd(arena.ws_bytes) == 0, _lib.last_error()
        rc = bwd(arena.ws_bytes)
        err = _lib.last_error()
    torch.cuda.synchronize()
    assert rc == 6 and "cannot be captured" in err, (rc, err)
    assert arena.holds_fill(), "the refused call, or the captured forward, wrote to the allocation"
    del g
    got = call.run(arena, "eager again")
    assert all(same_bits(a, b) for a, b in zip(got, ref))

