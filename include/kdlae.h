/*
 * kdlae.h — C ABI of the MI355X-native KDLAE path (libkdlae.so).
 *
 * The reference exposes no FFI: its boundary is the PyTorch nn.Module API
 * (SURVEY.md §8b).  These entry points are what a ctypes/cffi binding of
 * that module API binds; each one replaces the reference interface cited
 * beside it.  All pointers are device pointers unless marked host; tensors
 * are fp32, contiguous NCHW exactly as the reference consumes/produces them.
 * `stream` is a hipStream_t (0 = null stream).  Nothing here allocates,
 * frees or synchronises inside *_forward / *_pack_device: activations,
 * outputs, the flat parameter vector and the workspace are caller-owned;
 * the handle owns only the packed weights and their pack program.  Every
 * call makes the handle's device current and restores the caller's device
 * before returning.
 *
 * Caller's stream, for every entry that takes a `stream`: all its device
 * work (kernels, zero fills, device copies) is ordered on that stream and
 * nothing goes to the null stream; a stream the library owns (the training
 * backwards' side stream) waits on `stream` before its first launch and is
 * joined back into it before the call returns; the call neither waits on
 * the host nor allocates, so it returns while `stream` is still busy and
 * can be captured into a HIP graph on it (memory is zeroed by a kernel of
 * the library's own, so every node of such a graph is a kernel).  While
 * `stream` is being captured, kdlae_tt_backward and kdlae_st_backward keep
 * every launch on it, as under KDLAE_DEBUG=train_serial (same bits): the
 * side stream and the handle's events outlive any graph and are never
 * drawn into a caller's capture.  The exceptions: kdlae_*_set_param,
 * *_commit_params, *_prepare, *_create and *_destroy (host data,
 * allocation, synchronous), kdlae_data_sample (may wait on the host, not
 * for capture), kdlae_tt_mark_sync (a host wait), kdlae_tt_backward_marked
 * (asynchronous and ordered, but its marks are handle-owned events: under
 * capture it is refused with KDLAE_ESTATE before any launch) and the
 * kdlae_debug_* / kdlae_t_debug_* self-test entries.
 * tests/test_caller_stream_gpu.py holds every entry to this.
 *
 * Error handling: every call returns KDLAE_OK (0) or one of the codes
 * below; kdlae_last_error() returns a thread-local message describing the
 * last failure on the calling thread.
 *
 * Environment: the library reads two variables, neither of which changes
 * results.  KDLAE_DEBUG (comma-separated flags, read when a KDLAE-T handle
 * builds its pack program: kdlae_t_prepare or the first pack) selects between kernel schedules that produce
 * the same bits: "no_attn_in_fusion" keeps the attention-output GEMM and the
 * LN + ffn.project_in GEMM separate (every block); "no_attn_in_split" keeps
 * them separate for the C = 96 blocks only (by default their first
 * project_in weight group is fused as well); "no_attn_out_dw" keeps the
 * v-writing Gram ring and the per-image attention-output GEMM on the C = 48 /
 * 96 blocks; "gdfn_split" runs the C = 192 / 384 GDFN tails as C / 96 blocks
 * per pixel tile (gdfn_out_kernel<6, 8>) instead of gdfn_once_kernel, which
 * stages and gates a pixel tile once per 192 output channels.  One flag selects between two
 * evaluation orders that agree to fp32 rounding, not to the bit: "no_sr_fold"
 * keeps the sr head's cen and upen convs as two launches instead of the one
 * composed 5x5 conv (csrc/sr_fold.hip).  KDLAE_PROBE_DUMP
 * names a CSV file kdlae_t_probe_read writes per-launch timings to.
 * One more KDLAE_DEBUG flag is read on EVERY training call (kdlae_tt_forward /
 * kdlae_tt_backward / kdlae_tt_backward_marked), not at pack time:
 * "train_trace" brackets each training launch with a pair of HIP events and
 * synchronises the stream at the end of the call to dump them to
 * KDLAE_PROBE_DUMP.  It does not change results, but the synchronisation
 * removes the overlap of the bucketed all-reduce with the backward that the
 * gradient-ready marks exist for: diagnostics only, never in production.
 * "train_serial" (read by kdlae_tt_backward / kdlae_tt_backward_marked) keeps
 * every backward launch on the caller's stream; by default the weight-gradient
 * GEMMs and bias column sums run on a library-owned non-blocking side stream
 * that is forked from and joined back into the caller's stream inside the call
 * (every gradient-ready mark and the call's end follow a join), with the same
 * results either way.  "train_keep_yd" (read by kdlae_tt_forward; the backward
 * follows what the forward kept) stores the GDFN dwconv output for the
 * backward instead of having the backward recompute it from its input (A/B
 * only: same gradients bit for bit, 1 KiB per pixel more traffic each way);
 * "train_w3_raw" (read on every training call) has the 3x3 convs' implicit
 * GEMMs read the OIHW weights directly instead of a per-call [9 Cin][Cout]
 * repack (A/B only: same bits).
 */
#ifndef KDLAE_H_
#define KDLAE_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  KDLAE_OK = 0,
  KDLAE_EINVAL_SHAPE = 1,   /* e.g. H or W not divisible by 8 (reference: RuntimeError from pixel_unshuffle) */
  KDLAE_EINVAL_CONFIG = 2,  /* ctor kwargs the HIP path does not support (message says which) */
  KDLAE_EHIP = 3,           /* a HIP runtime call failed; message carries hipGetErrorString */
  KDLAE_EPARAM = 4,         /* unknown / missing / wrongly sized state_dict entry */
  KDLAE_ENOTIMPL = 5,       /* dual_pixel_task=True: NameError in the reference (KDLAE_model.py:305-321) */
  KDLAE_ESTATE = 6          /* forward before commit_params, workspace too small, ... */
};

const char* kdlae_last_error(void);
int kdlae_abi_version(void);

/* ------------------------------------------------------------------ KDLAE-T
 * Ctor kwargs of KDLAE_teacher (KDLAE/KDLAE_model.py:205-218).  Strings are
 * mapped to flags: LayerNorm_type=='BiasFree' -> layernorm_biasfree=1,
 * static=="train" -> static_train=1, params=='cat' -> params_cat=1.
 */
typedef struct kdlae_t_config {
  int inp_channels;
  int out_channels;
  int dim;
  int num_blocks[4];
  int num_refinement_blocks;
  int heads[4];
  double ffn_expansion_factor;
  int bias;
  int layernorm_biasfree;
  int dual_pixel_task;
  int static_train;
  int params_cat;
} kdlae_t_config;

typedef struct kdlae_t_handle kdlae_t_handle;

/* replaces KDLAE_teacher.__init__ (KDLAE_model.py:205-268): validates the config, binds `device`. */
int kdlae_t_create(const kdlae_t_config* cfg, int device, kdlae_t_handle** out);
/* replaces Restormer.__init__ (Train/basicsr/models/archs/restormer_arch.py:471-546): a kdlae_t_handle whose
 * parameter list is Restormer's own state_dict, in its order: patch_embed ... refinement, then output; none of
 * output_param.*, refinement_out.*, output2.* or the sr head.  static_train and params_cat of `cfg` are ignored
 * (Restormer has neither kwarg).  inp_channels != out_channels is KDLAE_EINVAL_CONFIG (the residual
 * output(...) + inp_img, :559, is undefined), dual_pixel_task is KDLAE_ENOTIMPL (its 6-channel patch embed is
 * wider than the narrow-input conv takes).  Every kdlae_t_* entry works on the handle: kdlae_t_forward computes
 * hq = output(refinement(...)) + img with the launches of a KDLAE_teacher handle with params != 'cat' and
 * static != 'train', bit for bit; `rate` and `sr` must be NULL (KDLAE_ESTATE otherwise, nothing launched);
 * the rate sweep and the sr head are refused as on that teacher handle; the workspace holds no tail or sr-head
 * buffer. */
int kdlae_t_create_restormer(const kdlae_t_config* cfg, int device, kdlae_t_handle** out);
int kdlae_t_destroy(kdlae_t_handle* h);

/* state_dict surface (KDLAE_model.py:220-268 key layout; load_state_dict at KDLAE_T.ipynb:1074-1075).
 * kdlae_t_num_params / kdlae_t_param_info enumerate the expected keys and element counts, in
 * state_dict order.  The packed device layout (LN weight folded into 1x1 weights, NHWC/MFMA
 * fragment order) is produced ON THE DEVICE by the handle's pack program from the flat fp32
 * parameter vector (every key in that order, back to back; kdlae_t_params_numel floats):
 *   kdlae_t_pack_device(params = DEVICE flat vector) enqueues the pack on `stream` (no sync) and
 *     is what the nn.Module calls before every forward, so the packed copy never goes stale;
 *   kdlae_t_set_param stages one entry from HOST memory (strict: unknown key or numel mismatch
 *     -> KDLAE_EPARAM) and kdlae_t_commit_params packs the staged set (synchronous). */
int kdlae_t_num_params(const kdlae_t_handle* h);
int kdlae_t_param_info(const kdlae_t_handle* h, int index, const char** name, int64_t* numel);
int64_t kdlae_t_params_numel(const kdlae_t_handle* h);
/* Builds and uploads the handle's pack program (device allocation + one synchronous copy; the
 * program depends on the config only).  Optional: the first pack_device / commit_params does it
 * otherwise.  Call it once before capturing forwards into a HIP graph, so that no call inside the
 * capture allocates or synchronises. */
int kdlae_t_prepare(kdlae_t_handle* h);
int kdlae_t_pack_device(kdlae_t_handle* h, const float* params, int64_t numel, void* stream);
int kdlae_t_set_param(kdlae_t_handle* h, const char* name, const float* host_data, int64_t numel);
int kdlae_t_commit_params(kdlae_t_handle* h, void* stream);

/* Workspace contract, for every *_workspace_bytes query and every entry point that takes a `workspace` in this
 * header (kdlae_t_forward / _forward_rates / _forward_sr (Restormer handles included), kdlae_s_forward, asdqe_forward, kdlae_tt_*, kdlae_st_*,
 * asdqe_train_*):
 *   - the query's answer is positive (-1 with kdlae_last_error for arguments the entry point would refuse) and a
 *     multiple of 256; `workspace` must be 256-byte aligned (every buffer the plan carves out of it then is);
 *   - the contents of the workspace on entry are arbitrary: it needs no initialisation, may be reused across
 *     shapes, calls and handles, and may hold anything (another call's leftovers, NaNs); whatever a call reads
 *     from it, that call (or, for a backward, its forward) wrote first, so no output depends on them;
 *   - the output buffers' contents on entry are arbitrary too: outputs are overwritten (`grad` as well, unless
 *     an `accumulate` argument says otherwise);
 *   - workspace_bytes below the query's answer is refused with KDLAE_ESTATE ("... workspace too small") before
 *     anything is launched; with the answer itself the call writes nothing outside [workspace, workspace + bytes)
 *     and its outputs, and never writes a read-only operand;
 *   - a training forward leaves its activations in the workspace: the same pointer, with its contents unchanged,
 *     must reach the matching backward.
 * tests/test_workspace_gpu.py holds every entry point to this with guarded, poisoned workspaces.
 *
 * Device bytes of caller-owned scratch needed by kdlae_t_forward for a B x H x W batch. */
int64_t kdlae_t_workspace_bytes(const kdlae_t_handle* h, int B, int H, int W);

/* replaces KDLAE_teacher.forward (KDLAE_model.py:270-336):
 *   img  [B, inp_channels, H, W]   ({"img"})
 *   rate [B, 1, H, W]              ({"denoise_rate"}; read only when params_cat)
 *   hq   [B, out_channels, H, W]   (out["hq"])
 *   sr   [B, out_channels, 2H, 2W] (out["sr"]; must be NULL iff static_train == 0)
 * H % 8 == 0 and W % 8 == 0 are required (else KDLAE_EINVAL_SHAPE).  Enqueued on `stream`. */
int kdlae_t_forward(kdlae_t_handle* h, const float* img, const float* rate, int B, int H, int W,
                    float* hq, float* sr, void* workspace, int64_t workspace_bytes, void* stream);

/* Rate sweep: R denoise rates of the same B images in one call.  Everything up to and including the
 * `output` conv (KDLAE_model.py:275-314) sees only the image and runs once at batch B; its result is
 * fanned out into R B rows that differ in the rate channel only, and output_param / refinement_out /
 * output2 (+ the sr head when `sr` is given) run at batch R B.  Row r B + b is bit for bit what
 * kdlae_t_forward gives for image b at rate r.
 *   rates  DEVICE; rate_is_map == 0: [R][B] scalars, rate_is_map == 1: [R][B][1][H][W] maps
 *   hq     [R][B][out_channels][H][W]    (hq[r] is a contiguous batch)
 *   sr     [R][B][out_channels][2H][2W], or NULL to skip the sr head (allowed with static_train == 1;
 *          non-NULL with static_train == 0 is KDLAE_EINVAL_CONFIG)
 * Needs params_cat == 1 (else KDLAE_EINVAL_CONFIG), 1 <= R <= 64 and H % 8 == 0, W % 8 == 0 (else
 * KDLAE_EINVAL_SHAPE); refused (KDLAE_ESTATE) while debug taps are armed.  Every check comes before the
 * first launch.  kdlae_t_rates_workspace_bytes sizes the scratch: trunk buffers for B images, tail
 * buffers for R B, the sr head's for R B only when with_sr. */
int64_t kdlae_t_rates_workspace_bytes(const kdlae_t_handle* h, int B, int R, int H, int W, int with_sr);
int kdlae_t_forward_rates(kdlae_t_handle* h, const float* img, const float* rates, int rate_is_map, int B, int R,
                          int H, int W, float* hq, float* sr, void* workspace, int64_t workspace_bytes,
                          void* stream);

/* The sr head alone (cen -> upen -> enhance -> outputen, KDLAE_model.py:326-329; cen and upen run as one
 * composed 5x5 conv) on a given UNclamped
 * hq [B][out_channels][H][W] -> sr [B][out_channels][2H][2W]: the last four steps of kdlae_t_forward.
 * static_train == 0: KDLAE_EINVAL_CONFIG. */
int64_t kdlae_t_sr_workspace_bytes(const kdlae_t_handle* h, int B, int H, int W);
int kdlae_t_forward_sr(kdlae_t_handle* h, const float* hq, int B, int H, int W, float* sr, void* workspace,
                       int64_t workspace_bytes, void* stream);

/* Picks one of R candidates per image from device scores [R][B] and copies it out, without a host
 * round trip: mode 0 = argmin_r |score[r][b] - target[b]| (target: device [B], fp32 arithmetic),
 * mode 1 = argmax, mode 2 = argmin (target unused, may be NULL).  Ties go to the lowest r; a NaN score
 * is never chosen, and index 0 is chosen when all R are NaN.  Writes index_out[b] (int32) and copies
 * hq[index][b] (per_image floats; hq is [R][B][per_image]) into hq_out[b].  No atomics, so the result
 * is a function of the inputs alone; any float alignment of hq / hq_out is accepted.  Null pointers,
 * R, B or per_image < 1, or a mode outside 0..2: KDLAE_EINVAL_CONFIG before any launch. */
int kdlae_rate_select(const float* scores, int R, int B, int mode, const float* target, const float* hq,
                      int64_t per_image, int32_t* index_out, float* hq_out, void* stream);

/* Tiled inference: overlapping tiles of an image too large for one forward, blended on the device.
 * The plan (fixed by H, W, tile, overlap; H % 8 == 0, W % 8 == 0, tile % 8 == 0, tile >= 16,
 * 0 <= overlap < tile, anything else KDLAE_EINVAL_SHAPE):
 *   th = min(tile, H), tw = min(tile, W)                       (per axis, not min(tile, H, W))
 *   starts along an axis of length L with tile t: range(0, L - t, t - overlap) + [L - t], so tile i of n
 *   starts at i stride for i < n - 1 and at L - t for the last; n = 1 when L == t (stride is then
 *   reported as t and unused)
 *   tile (b, i, j) has flat index (b ni + i) nj + j
 * kdlae_tile_plan is host only and returns the plan.  kdlae_tile_gather copies tiles first .. first + count - 1
 * of src [B][C][H][W] into dst [count][C][th][tw] (the image and, at C = 1, the rate map).  kdlae_tile_blend
 * takes tiles [B ni nj][C][scale th][scale tw] (scale 1: hq, scale 2: sr, every coordinate doubled) and writes
 * dst [B][C][scale H][scale W]: per pixel 0 + o1 + o2 + ... over the covering tiles in ascending flat index,
 * in fp32, divided by the fp32 count of covering tiles; E.add_(patch), W.add_(1), E.div_(W) of the usual host
 * loop, bit for bit (so a lone -0 comes out +0, as it does there).  One thread per output pixel group loops
 * over its tiles: no atomics, the result is a function of the inputs alone.  Any float alignment of src, tiles
 * and dst is accepted (16-byte accesses where pointers and starts allow, 4-byte otherwise).
 * Null pointers, B, C, H, W or count < 1, first < 0, first + count > B ni nj, scale outside {1, 2}:
 * KDLAE_EINVAL_CONFIG.  Every check comes before the launch. */
int kdlae_tile_plan(int H, int W, int tile, int overlap, int* th, int* tw, int* ni, int* nj, int* stride_y,
                    int* stride_x);
int kdlae_tile_gather(const float* src, int B, int C, int H, int W, int tile, int overlap, int first, int count,
                      float* dst, void* stream);
int kdlae_tile_blend(const float* tiles, int B, int C, int H, int W, int tile, int overlap, int scale, float* dst,
                     void* stream);

/* The blend of a tiled rate sweep: all R outputs in one launch, read from the staging layout the sweep leaves.
 * kdlae_t_forward_rates at batch `count` writes [R][count][C][th][tw]; run over the n = B ni nj tiles of the plan
 * tile_batch at a time, each chunk into its own block, it leaves the chunk-major buffer `staged`
 * (T = C scale^2 th tw floats per tile; scale 1: hq, scale 2: sr):
 *   chunk k holds tiles k tile_batch .. k tile_batch + count_k - 1, count_k = min(tile_batch, n - k tile_batch),
 *   and starts at float k tile_batch R T;
 *   inside chunk k, rate r and tile q (flat index k tile_batch + q) sit at (r count_k + q) T;
 *   n R T floats in all, no padding (tile_batch >= n is the one chunk [R][n][C][scale th][scale tw]).
 * Writes dst [R][B][C][scale H][scale W]: per output pixel 0 + o1 + o2 + ... over the covering tiles in ascending
 * flat tile index, in fp32, divided by the fp32 count, so dst[r] has exactly the bits kdlae_tile_blend gives for
 * the r-th slice re-laid out as [n][C][scale th][scale tw], for every tile_batch.  One thread per output pixel
 * group, no atomics; 16-byte accesses where both pointers and the x stride allow, 4-byte otherwise.
 * Null pointers, R outside 1..64, B, C or tile_batch < 1, scale outside {1, 2}: KDLAE_EINVAL_CONFIG; the plan's
 * refusals as above.  Every check comes before the launch. */
int kdlae_tile_blend_rates(const float* staged, int R, int B, int C, int H, int W, int tile, int overlap,
                           int tile_batch, int scale, float* dst, void* stream);

/* The two blends with a separable window that falls towards the tile edge, so that a tile fades out where its
 * neighbour fades in.  Same arguments, plan, tile order and alignment rule as kdlae_tile_blend /
 * kdlae_tile_blend_rates, plus two device tables wy [scale th] and wx [scale tw], indexed by the tile-local
 * coordinate of the (scaled) output pixel.  Per output pixel, over the covering tiles in ascending flat index:
 *   w = fl(wy[yt] wx[xt]);  E = fl(E + fl(w o));  S = fl(S + w);  cnt = cnt + 1
 *   out = cnt == 1 ? o : E / S                                  (fp32, no fused multiply-add, true division)
 * A pixel under exactly one tile takes that tile's value untouched (fl(fl(w o) / w) != o for about one fp32 o in
 * ten), so tile interiors and a one-tile image keep the tile's bits.  With tables of ones the result has the bits
 * of the uniform entries (but for a lone -0, which stays -0 here).  16-byte accesses also need wx on 16 bytes; 4-byte accesses otherwise.
 * Precondition (the entries cannot inspect device values): every table entry is finite and greater than 0.
 * A null wy or wx is KDLAE_EINVAL_CONFIG; every other refusal as for the uniform entries, all before any launch. */
int kdlae_tile_blend_w(const float* tiles, int B, int C, int H, int W, int tile, int overlap, int scale,
                       const float* wy, const float* wx, float* dst, void* stream);
int kdlae_tile_blend_rates_w(const float* staged, int R, int B, int C, int H, int W, int tile, int overlap,
                             int tile_batch, int scale, const float* wy, const float* wx, float* dst, void* stream);

/* Clip inference for KDLAE-S: overlapping windows of `frames` consecutive frames of a clip [B][T][H][W], run
 * through the student one window at a time and blended on the device.  The tile plan on the frame axis (fixed by
 * T, frames, overlap; T >= 1, frames >= 1, else KDLAE_EINVAL_CONFIG; 0 <= overlap < f, else KDLAE_EINVAL_SHAPE):
 *   f = min(frames, T), stride = f - overlap
 *   starts range(0, T - f, stride) + [T - f]: window i of n starts at i stride for i < n - 1 and at T - f for
 *   the last; n = ceil((T - f) / stride) + 1, which is 1 when T == f
 *   window (b, i) has flat index b n + i
 * The kernels know nothing of the model: any H, W >= 1.  kdlae_clip_plan is host only.  kdlae_clip_gather copies
 * windows first .. first + count - 1 of src into dense dst [count][f][H][W] (16-byte accesses when both pointers
 * sit on 16 bytes and H W % 4 == 0, 4-byte accesses otherwise).  kdlae_clip_blend takes windows [B n][f][H][W]
 * and writes dst [B][T][H][W] (the same access rule).  With wt == NULL, per output element: 0 + o1 + o2 + ... over
 * the covering windows in ascending index, in fp32, divided by the fp32 count: E[:, s:s+f].add_(y),
 * W[s:s+f].add_(1), E.div_(W) of the usual host loop, bit for bit (so a lone -0 comes out +0, as it does there).
 * With a device table wt [f], indexed by the frame's position p inside its window, kdlae_tile_blend_w's rule on
 * one axis:
 *   w = wt[p];  E = fl(E + fl(w o));  S = fl(S + w);  cnt = cnt + 1
 *   out = cnt == 1 ? o : E / S                                  (fp32, no fused multiply-add, true division)
 * so a frame under exactly one window keeps that window's bits.  Precondition (the entries cannot inspect device
 * values): every table entry is finite and greater than 0.  One thread per output pixel group loops over its
 * windows: no atomics, the result is a function of the inputs alone.
 * kdlae_clip_blend_u8 runs the same blend and applies kdlae_postprocess_u8's rule to the blended value in the
 * same thread: clamp to [0, 1], rint(x 255), cropped to h <= H, w <= W, written as dst u8 [B][T][h][w] in frame
 * order: the bytes of kdlae_postprocess_u8 on kdlae_clip_blend's output, with no black-pixel mask, no limit on T
 * and no float clip in between.  Any byte alignment of dst (4-byte stores when dst sits on 4 bytes, w % 4 == 0,
 * windows sits on 16 bytes and W % 4 == 0; single bytes otherwise).
 * Null pointers (wt excepted), B, H, W or count < 1, first < 0, first + count > B n, h or w < 1, h > H, w > W:
 * KDLAE_EINVAL_CONFIG.  Every check comes before the launch. */
int kdlae_clip_plan(int T, int frames, int overlap, int* f, int* n, int* stride);
int kdlae_clip_gather(const float* src, int B, int T, int H, int W, int frames, int overlap, int first, int count,
                      float* dst, void* stream);
int kdlae_clip_blend(const float* windows, int B, int T, int H, int W, int frames, int overlap, const float* wt,
                     float* dst, void* stream);
int kdlae_clip_blend_u8(const float* windows, int B, int T, int H, int W, int h, int w, int frames, int overlap,
                        const float* wt, uint8_t* dst, void* stream);

/* Streaming inference for KDLAE-S: B parallel sources deliver one frame at a time and every frame comes back
 * enhanced at a fixed latency.  The rule (fixed by frames = F >= 1 and emit, 0 <= emit < F; streams.py's default
 * emit is F / 2).  Frame t of a stream of T frames is
 *   f = min(F, T);  s_t = min(max(t - emit, 0), T - f);  out[:, t] = forward(x[:, s_t : s_t + f])[:, t - s_t]
 * so every frame comes from the window in which it sits at position emit, but for the first emit frames (the
 * first window) and the last F - 1 - emit (the last window); a stream shorter than F is one window.  emit = F - 1
 * is the causal setting with no latency.  As with the clip entries, the zero padding along the frame axis makes
 * this a different function of the stream from one forward over all T frames: there is no error bound to state.
 * The schedule (push t, 0-based, returns nothing while t < F - 1, frames 0 .. emit at t = F - 1, frame
 * t - (F - 1 - emit) afterwards; the flush returns the rest) lives in streams.py; the entries below keep the
 * window on the device.
 *
 * state: kdlae_stream_state_bytes(B, frames, H, W) bytes of device memory (-1 for sizes < 1): a 16-byte header
 * whose first 8 bytes are the push counter, then the ring [B][frames][H][W] fp32 of converted frames; frame number
 * c lives in slot c % frames.  kdlae_stream_reset sets the counter to 0 and leaves the ring as it is: a slot's old
 * contents are only ever read into stack positions that have no frame yet, which are unspecified until `frames`
 * pushes have been made and must not be used.
 * kdlae_stream_push_u8: frame u8 [B][h][w][channels] (channels 1 = gray, 3 / 4 = BGR / BGRA) is converted by
 * exactly kdlae_frames_preprocess_u8's rule (cv2 COLOR_BGR2GRAY in 8-bit fixed point, / 255, reflect-padded on the
 * bottom/right to (H, W) = kdlae_padded_size(h, w, multiple)) and, with count the counter's value read on the
 * device, stored in ring slot count % frames; stack f32 [B][frames][H][W] receives the window in time order:
 * positions 0 .. frames - 2 from the ring's other slots, oldest first, position frames - 1 the new frame.  One
 * launch, one thread per pixel group; the slot written is the one whose frame drops out, so no thread reads
 * what another writes.  The counter is not a launch argument: a captured graph of the launch serves every push.
 * kdlae_stream_push_f32: the same for a frame f32 [B][H][W] the caller has preprocessed: a bit copy, no padding.
 * kdlae_stream_advance: count = count + 1, one thread with a plain store, stream-ordered after the launches that
 * read the counter.  A push without an advance overwrites the same slot again.
 * Access widths: 16-byte accesses of ring, stack and an fp32 frame when state, stack (and the fp32 frame) sit on
 * 16 bytes and W % 4 == 0, 4-byte accesses otherwise.  The u8 source may sit at any byte offset and is read one
 * byte at a time, but for a gray source on 4 bytes with w % 4 == 0 under 16-byte accesses: 4 bytes a load.
 * Null pointers, B, h, w, H, W or frames < 1, channels outside {1, 3, 4}, multiple < 1: KDLAE_EINVAL_CONFIG.  A
 * frame smaller than its reflect padding, state off 8 bytes, stack or an fp32 frame off 4 bytes, more than
 * 2^31 - 1 pixels of a frame or rows of all sources: KDLAE_EINVAL_SHAPE.  Every check comes before the launch. */
int64_t kdlae_stream_state_bytes(int B, int frames, int H, int W);
int kdlae_stream_reset(void* state, void* stream);
int kdlae_stream_push_u8(const uint8_t* frame, int B, int h, int w, int channels, int multiple, int frames,
                         void* state, float* stack, void* stream);
int kdlae_stream_push_f32(const float* frame, int B, int H, int W, int frames, void* state, float* stack,
                          void* stream);
int kdlae_stream_advance(void* state, void* stream);

/* Distillation labels: KDLAE-T (or Restormer) outputs as the targets of a KDLAE-S training step, without the
 * folder of saved teacher images the reference's KDLAES.yml reads back.  The three entries move the data either
 * side of a forward that stays untouched.  Items are the frames of a stack [B][F] in flat order j = b F + f; every
 * entry works on the chunk j0 .. j0 + n - 1 (q = j - j0 below), so the teacher runs n frames at a time.  frames,
 * rate, src and dst point at the whole stack, img, rate_map and hq at the chunk.
 *
 * kdlae_distill_expand_u8: frames u8 [B][F][h][w][channels] (channels 1 = gray, 3 / 4 = BGR / BGRA, alpha
 * ignored) -> img f32 [n][3][H][W] and rate_map f32 [n][1][H][W], (H, W) = kdlae_padded_size(h, w, multiple), in one
 * launch.  The gray value y of a pixel is its byte (channels 1) or cv2's 8-bit COLOR_BGR2GRAY,
 *   y = (1868 B + 9617 G + 4899 R + 8192) >> 14,
 * and all three channels of img hold (float)y / 255.0f, reflect-padded on the bottom/right: bit for bit
 * kdlae_preprocess_u8 on the gray frame replicated to [h][w][3].  rate_map[q] is the constant rate[j], rate a device
 * array of B F floats; rate and rate_map may both be null (a Restormer teacher takes no rate), then no map is written.
 * kdlae_distill_expand_f32: the same for frames f32 [B][F][H][W] that are network inputs already (training crops; H
 * and W multiples of 8): a bit copy into the three channels, and the rate map.  No padding, no clamp, no scale.
 * kdlae_distill_collapse: hq f32 [n][3][Hp][Wp] -> items j0 .. of dst [B][F][h][w] (h <= Hp, w <= Wp: the top-left
 * crop), f32 or, with dst_u8 != 0, u8; one launch either way.
 *   mode KDLAE_DISTILL_FILE: the round trip through a lossless image file.  Per channel v = rintf(clamp(x, 0, 1) 255)
 *     as kdlae_postprocess_u8 does; with src u8 [B][F][h][w][src_channels] (nullable), all three bytes become 0 where
 *     the source pixel's gray value y is 0 (the black mask of kdlae_postprocess_u8 when its lq is the replicated
 *     gray frame); then the three bytes, read as R, G, B, give g = (1868 v2 + 9617 v1 + 4899 v0 + 8192) >> 14.
 *     dst = g (u8) or (float)g / 255.0f (f32).  The f32 form is what a grayscale float32 decode of the saved image
 *     (the reference's imfrombytes(flag='grayscale', float32=True)) is modelled as: parity with a real cv2 encode /
 *     decode is not pinned anywhere in this project.
 *   mode KDLAE_DISTILL_MEAN: dst = ((x0 + x1) + x2) / 3.0f, every operation rounded on its own in fp32, no fused
 *     multiply-add, no clamp, no mask (src is ignored); f32 output only.
 * One thread per group of output pixels, no atomics: the result is a function of the inputs alone.  16-byte
 * accesses of the fp32 tensors (4-byte stores of a u8 dst) when img and rate_map (expand_f32: and frames) sit on 16
 * bytes and W % 4 == 0, or hq sits on 16 bytes, Wp % 4 == 0, w % 4 == 0 and dst sits on 16 (u8: 4) bytes; 4-byte
 * (u8: single-byte) accesses otherwise, with the same bits.  A u8 frames / src may sit at any byte offset.
 * Null frames, img, hq or dst, rate without rate_map or the reverse, n < 1, j0 < 0, j0 + n > B F, any size < 1,
 * channels or src_channels outside {1, 3, 4}, an unknown mode, mode mean with dst_u8: KDLAE_EINVAL_CONFIG.  A frame
 * smaller than its reflect padding, f32 H or W not a multiple of 8, h > Hp or w > Wp, an fp32 pointer off 4 bytes,
 * more than 2^31 - 1 frames or pixels of one frame (the kernels keep a position inside a frame in 32 bits and
 * everything else in 64): KDLAE_EINVAL_SHAPE.  Every check comes before the launch. */
#define KDLAE_DISTILL_FILE 0
#define KDLAE_DISTILL_MEAN 1
int kdlae_distill_expand_u8(const uint8_t* frames, int B, int F, int h, int w, int channels, int multiple,
                            const float* rate, int j0, int n, float* img, float* rate_map, void* stream);
int kdlae_distill_expand_f32(const float* frames, int B, int F, int H, int W, const float* rate, int j0, int n,
                             float* img, float* rate_map, void* stream);
int kdlae_distill_collapse(const float* hq, int B, int F, int Hp, int Wp, int h, int w, int j0, int n, int mode,
                           const uint8_t* src, int src_channels, void* dst, int dst_u8, void* stream);

/* Measurement hook for bench.py (no effect on results).  When a probe class is armed, every
 * launch of that kernel class inside kdlae_t_forward is bracketed by a pair of HIP events on
 * `stream`; kdlae_t_probe_read synchronises those events and returns the summed device time (ms),
 * launch count and the algorithmic HBM bytes / FLOPs of the probed launches (SURVEY.md §8d model).
 * Classes: 0 = off, 1 = 1x1/implicit-GEMM conv (MFMA), 2 = dwconv+Gram (MDTA pass 1),
 * 3 = dwconv+GELU gate (GDFN).  A non-zero `level_filter` limits probing to blocks whose channel
 * count equals it.  */
int kdlae_t_probe_arm(kdlae_t_handle* h, int kernel_class, int level_filter);
int kdlae_t_probe_read(kdlae_t_handle* h, double* ms, int64_t* launches, double* bytes, double* flops);

/* Diagnostics (tools/config1_taps.py; not part of the drop-in boundary): activations at every
 * TransformerBlock stage in execution order — per stage its input ("<stage>.in"), then per block the
 * attention half's output x1 = x + attn(norm1 x) ("<stage>.<i>.attn", KDLAE_model.py:160) and the
 * block output ("<stage>.<i>", :161).  kdlae_t_debug_tap_info names tap i, its channel count C and its
 * resolution relative to the forward's input, H * num / den.  While kdlae_t_debug_taps(h, n, dst) is
 * armed (n = 0 disarms), every kdlae_t_forward copies tap i (i < n, dst[i] != NULL) into the device
 * buffer dst[i] as compact NHWC [B][H_i][W_i][C] on the forward's stream.  Results are unchanged. */
int kdlae_t_debug_tap_count(const kdlae_t_handle* h);
int kdlae_t_debug_tap_info(const kdlae_t_handle* h, int i, char* name, int name_len, int* C, int* num, int* den);
int kdlae_t_debug_taps(kdlae_t_handle* h, int n, float* const* dst);

/* Diagnostics (tests/test_sr_fold_gpu.py): the sr head's folded-conv record as the last pack left it,
 * [9 border classes][out_tiles = 8 dim / 16][ksteps = (25 out_channels + 4) / 4][64 lanes] floats (layout:
 * csrc/pack.hip, pack_fold_kernel), copied into the device buffer dst on `stream`.  Returns the record's
 * float count (dst == NULL: the count alone), 0 when the handle runs the unfolded sr head (static != 'train'
 * or KDLAE_DEBUG=no_sr_fold), -1 on error. */
int64_t kdlae_t_debug_sr_fold(const kdlae_t_handle* h, float* dst, int64_t capacity, void* stream);

/* ------------------------------------------------------------------ KDLAE-S
 * Ctor kwargs of KDLAE_student (KDLAE/KDLAE_model.py:340-384): a 3-D U-Net over a burst of frames.
 * hidden_channels has num_hidden entries (default [8, 16, 16, 32]); levels = num_hidden - 1.
 * The HIP path supports inp_channels == out_channels == 1 (forward unsqueezes a [B,F,H,W] input,
 * :397) and kernel_size == 3.
 */
typedef struct kdlae_s_config {
  int inp_channels;
  int out_channels;
  int residual;
  int num_hidden;
  int hidden_channels[8];
  int kernel_size;
} kdlae_s_config;

typedef struct kdlae_s_handle kdlae_s_handle;

/* replaces KDLAE_student.__init__ (KDLAE_model.py:341-384). */
int kdlae_s_create(const kdlae_s_config* cfg, int device, kdlae_s_handle** out);
int kdlae_s_destroy(kdlae_s_handle* h);
/* state_dict surface: encoders.{i}.{0,2}, st_fusion.{0,2}, upconv_layers.{j}, decoders.{j}.{0,2},
 * out_conv (same semantics as the kdlae_t_* calls). */
int kdlae_s_num_params(const kdlae_s_handle* h);
int kdlae_s_param_info(const kdlae_s_handle* h, int index, const char** name, int64_t* numel);
int64_t kdlae_s_params_numel(const kdlae_s_handle* h);
int kdlae_s_prepare(kdlae_s_handle* h);  /* as kdlae_t_prepare */
int kdlae_s_pack_device(kdlae_s_handle* h, const float* params, int64_t numel, void* stream);
int kdlae_s_set_param(kdlae_s_handle* h, const char* name, const float* host_data, int64_t numel);
int kdlae_s_commit_params(kdlae_s_handle* h, void* stream);
int64_t kdlae_s_workspace_bytes(const kdlae_s_handle* h, int B, int F, int H, int W);
/* replaces KDLAE_student.forward (KDLAE_model.py:395-431):
 *   x   [B, F, H, W]  (F = frames, the burst axis)
 *   out [B, F, H, W]  (= out_conv(...) + x when residual, squeezed)
 * H and W must be divisible by 2^levels (else KDLAE_EINVAL_SHAPE). */
int kdlae_s_forward(kdlae_s_handle* h, const float* x, int B, int F, int H, int W, float* out,
                    void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ ASDQE
 * Ctor kwargs of DenoiseRatePredictor (ASDQE/ASDQE_model.py:127).  The HIP path supports
 * in_channels 1..4 and dim a multiple of 16 (16..256).  Eval-mode semantics only: BatchNorm uses
 * its running statistics (folded into the conv weights at commit), Dropout is the identity.
 */
typedef struct asdqe_config {
  int in_channels;
  int dim;
} asdqe_config;

typedef struct asdqe_handle asdqe_handle;

/* replaces DenoiseRatePredictor.__init__ (ASDQE_model.py:127-156). */
int asdqe_create(const asdqe_config* cfg, int device, asdqe_handle** out);
int asdqe_destroy(asdqe_handle* h);
/* state_dict surface incl. BatchNorm buffers (num_batches_tracked: 1 element, ignored).  The
 * reference loads its checkpoint with strict=False (ASDQE_test.py:79); this surface is strict.
 * The BatchNorm fold (W' = W g / sqrt(var + 1e-5), b' = (b - mean) g / sqrt(var + 1e-5) + beta) is
 * part of the device pack program (asdqe_pack_device, same contract as kdlae_t_pack_device). */
int asdqe_num_params(const asdqe_handle* h);
int asdqe_param_info(const asdqe_handle* h, int index, const char** name, int64_t* numel);
int64_t asdqe_params_numel(const asdqe_handle* h);
int asdqe_prepare(asdqe_handle* h);  /* as kdlae_t_prepare */
int asdqe_pack_device(asdqe_handle* h, const float* params, int64_t numel, void* stream);
int asdqe_set_param(asdqe_handle* h, const char* name, const float* host_data, int64_t numel);
int asdqe_commit_params(asdqe_handle* h, void* stream);
int64_t asdqe_workspace_bytes(const asdqe_handle* h, int B, int H, int W);
/* replaces DenoiseRatePredictor.forward (ASDQE_model.py:158-171) in eval mode:
 *   lq, gt [B, in_channels, H, W]  (any H, W: zero-padded bottom/right to a multiple of dim)
 *   score  [B, 1]                   (tanh output)
 *   feat   optional (NULL to skip): the UNet output map, NHWC [B, H', W', 3*dim] — an inspection
 *          hook; the score path folds the 1x1 outc after the pool and does not need it. */
int asdqe_forward(asdqe_handle* h, const float* lq, const float* gt, int B, int H, int W, float* score,
                  float* feat, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ pre/post-processing
 * The steps either side of the forward in KDLAE/KDLAE_T.ipynb (load_image_as_tensor, reflect pad,
 * denoise_rate map; clamp, crop, img_as_ubyte, zero-mask of black input pixels) and ASDQE's
 * ToTensor, on device buffers.
 */
#include <stdint.h>

/* (H, W) the notebook pads (h, w) to: ((h + m) / m) * m when h % m != 0, else h (same for w). */
void kdlae_padded_size(int h, int w, int multiple, int* H, int* W);

/* images u8 [B, h, w, channels] (channels 1, 3 or 4; alpha dropped; bgr != 0 swaps B and R like
 * cv2.cvtColor(BGR2RGB)) -> img f32 [B, min(channels, 3), H, W] = x / 255, reflect-padded on the
 * bottom/right to kdlae_padded_size(h, w, multiple) (multiple 1 = no padding: ASDQE ToTensor).
 * rate f32 [B] (nullable) -> rate_map f32 [B, 1, H, W] (nullable): the constant denoise_rate map. */
int kdlae_preprocess_u8(const uint8_t* images, int B, int h, int w, int channels, int bgr, int multiple,
                        const float* rate, float* img, float* rate_map, void* stream);

/* KDLAE/KDLAE-S.ipynb load_consecutive_stack + padding cell: frames u8 [B, F, h, w, channels]
 * (channels 1 = gray, 3 / 4 = BGR / BGRA as cv2.imread returns them) -> x f32 [B, F, H, W] =
 * cv2 COLOR_BGR2GRAY (8-bit fixed point) / 255, reflect-padded on the bottom/right to
 * kdlae_padded_size(h, w, multiple) (the notebook uses multiple 32).  Frames of one call share h, w
 * (the notebook cv2.resizes odd-sized frames first; that resize stays on the host). */
int kdlae_frames_preprocess_u8(const uint8_t* frames, int B, int F, int h, int w, int channels, int multiple,
                               float* x, void* stream);

/* out f32 [B, C, Hs, Ws] (model output, C <= 64: image channels, or the F frames of KDLAE-S) ->
 * dst u8 [B, h*scale, w*scale, C]:
 * clamp(0, 1), crop, rint(x * 255) (skimage img_as_ubyte), and 0 where the input pixel
 * lq u8 [B, h, w, lq_channels] (nullable) is black in every colour channel; scale 2 maps each
 * output pixel to its nearest input pixel (the notebook's np.repeat x2 mask for sr). */
int kdlae_postprocess_u8(const float* out, int B, int C, int Hs, int Ws, int h, int w, int scale,
                         const uint8_t* lq, int lq_channels, uint8_t* dst, void* stream);

/* ------------------------------------------------------------------ KDLAE-T training
 * One optimisation step of BasicSR's ImageCleanModel on KDLAE_teacher
 * (Train/basicsr/models/image_restoration_model.py:198-218): forward with saved activations,
 * L1LossSr (Train/basicsr/models/losses/losses.py:135-194), backward of every layer,
 * clip_grad_norm_(0.01) and AdamW.  Parameters and gradients are two flat caller-owned device
 * buffers of kdlae_tt_num_floats floats in state_dict order (offsets from kdlae_tt_param_info; each key
 * starts on a 16-byte boundary and the pad floats between keys must be zero);
 * weights are read in their OIHW state_dict layout, so an optimizer update needs no repacking.
 * The DDP gradient all-reduce (base_model.py:76-82) is done by the caller between the backward and
 * kdlae_train_clip_adamw: one collective over the flat gradient buffer, or bucketed and overlapped
 * with the backward through kdlae_tt_backward_marked's gradient-ready marks.
 */
typedef struct kdlae_tt_handle kdlae_tt_handle;

/* replaces KDLAE_teacher.__init__ for training (same config struct; dual_pixel_task -> ENOTIMPL). */
int kdlae_tt_create(const kdlae_t_config* cfg, int device, kdlae_tt_handle** out);
/* replaces Restormer.__init__ for training: as kdlae_t_create_restormer, for a kdlae_tt_handle.  rate, sr and
 * dsr must be NULL in kdlae_tt_forward / _backward / _backward_marked (KDLAE_ESTATE otherwise, nothing launched). */
int kdlae_tt_create_restormer(const kdlae_t_config* cfg, int device, kdlae_tt_handle** out);
int kdlae_tt_destroy(kdlae_tt_handle* h);
/* net_g.state_dict() layout: key, element count and offset (floats) in the flat buffers. */
int kdlae_tt_num_params(const kdlae_tt_handle* h);
int kdlae_tt_param_info(const kdlae_tt_handle* h, int index, const char** name, int64_t* numel, int64_t* offset);
int64_t kdlae_tt_num_floats(const kdlae_tt_handle* h);
/* Device bytes of the caller-owned workspace (saved activations + backward scratch) for B x H x W. */
int64_t kdlae_tt_workspace_bytes(kdlae_tt_handle* h, int B, int H, int W);
/* replaces `preds = self.net_g(self.lq)` in optimize_parameters (image_restoration_model.py:200):
 * same tensors as kdlae_t_forward; theta = flat parameters.  Activations needed by the backward
 * stay in `workspace`, which must be passed unchanged to kdlae_tt_backward. */
int kdlae_tt_forward(kdlae_tt_handle* h, const float* theta, const float* img, const float* rate, int B, int H,
                     int W, float* hq, float* sr, void* workspace, size_t workspace_bytes, void* stream);
/* replaces `l_pix.backward()` (:213): dhq [B,C,H,W] / dsr [B,C,2H,2W] (nullable: zero) are the loss
 * gradients; grad (flat, overwritten) receives d loss / d theta.  Inputs get no gradient. */
int kdlae_tt_backward(kdlae_tt_handle* h, const float* theta, const float* dhq, const float* dsr, float* grad,
                      void* workspace, size_t workspace_bytes, void* stream);
/* kdlae_tt_backward plus gradient-ready marks for a bucketed DDP all-reduce that overlaps the backward
 * (DistributedDataParallel's gradient buckets, reducer.cpp behind base_model.py:76-82): the backward
 * walks the network deepest-first, i.e. the flat buffer from the end, and records event j when the
 * suffix [kdlae_tt_mark_lo(h, j), num_floats) of `grad` is final (offsets decrease with j).
 * kdlae_tt_mark_wait makes another stream wait for event j (enqueue that bucket's all-reduce behind
 * it); kdlae_tt_mark_sync waits on the host.  Marks stay valid until the next marked backward. */
int kdlae_tt_backward_marked(kdlae_tt_handle* h, const float* theta, const float* dhq, const float* dsr, float* grad,
                             void* workspace, size_t workspace_bytes, void* stream);
int kdlae_tt_mark_count(const kdlae_tt_handle* h);
int64_t kdlae_tt_mark_lo(const kdlae_tt_handle* h, int j);
int kdlae_tt_mark_wait(kdlae_tt_handle* h, int j, void* stream);
int kdlae_tt_mark_sync(kdlae_tt_handle* h, int j);
/* Fine-tuning with frozen parameters (the reference's freeze_except_patch_embed_and_enhance,
 * Train/basicsr/train.py:24-55, and the requires_grad filter of ImageCleanModel.setup_optimizers).
 * mask: host array of kdlae_tt_num_params(h) bytes in state_dict order, nonzero = trainable; NULL = all
 * (the default: exactly the launches of a handle that never saw a mask).  n != num_params, or a mask
 * that marks no key the forward uses, is KDLAE_EINVAL_CONFIG; a call between a kdlae_tt_forward and its
 * backward is KDLAE_ESTATE.  Keys the forward never touches (output_param.*, refinement_out.* when
 * params != 'cat') are ignored.  The mask holds for every later forward and backward until it is
 * changed; a change invalidates the last forward (a backward needs a new one).
 * Under a mask, with the layers in forward order (patch_embed, encoder_level1, ..., refinement, output,
 * output_param, refinement_out, output2, cen, upen, enhance, outputen; inside a TransformerBlock norm1,
 * attn.qkv, attn.qkv_dwconv, attn.temperature, attn.project_out, norm2, ffn.project_in, ffn.dwconv,
 * ffn.project_out): a layer's weight gradient is computed iff its key is trainable, its input gradient
 * iff a trainable key belongs to an earlier layer; the forward keeps no activations of the
 * TransformerBlocks before the first trainable key, and kdlae_tt_workspace_bytes answers for the
 * current mask (the workspace contract above holds under every mask).  After a backward every float of
 * a frozen key and every pad float of `grad` is +0.0f, so kdlae_train_clip_adamw's norm over all n
 * floats is the norm over the trainable ones, and every float of a trainable key has the bits the
 * all-trainable backward gives on the same inputs; hq / sr have the same bits under every mask.  The
 * gradient-ready marks stay valid: a frozen key holds the zero fill, which precedes every mark.
 * kdlae_tt_is_trainable: 1 / 0 for key `index` under the current mask, -1 for a bad index. */
int kdlae_tt_set_trainable(kdlae_tt_handle* h, const unsigned char* mask, int n);
int kdlae_tt_is_trainable(const kdlae_tt_handle* h, int index);
/* Launch calls the last kdlae_tt_backward / _backward_marked issued: kernels (a split-K GEMM with its
 * reduction counts once), memsets and memcpys, the zero fill of `grad` included.  For tests and probes. */
int64_t kdlae_tt_debug_backward_launches(const kdlae_tt_handle* h);

/* replaces self.cri_pix(pred, self.gt) with L1LossSr(loss_weight=1, reduction='mean') (losses.py:159-170):
 * loss[0] = 0.5 l1(hq) + 0.25 l1(sr) + 0.25 (shadow(hq) + shadow(sr)); dhq / dsr receive its gradient
 * (the shadow terms binarise at 0.1 and carry none).  pred_sr NULL = no sr term.  dhq / dsr NULL =
 * loss only: that gradient is not written.  pred_sr with gt_sr NULL or n_sr <= 0 is
 * KDLAE_EINVAL_CONFIG, as is any other null required pointer or n_hq <= 0; nothing is launched.
 * scratch: device buffer of kdlae_train_l1sr_scratch_floats() floats. */
int64_t kdlae_train_l1sr_scratch_floats(void);
int kdlae_train_l1sr(const float* pred_hq, const float* gt_hq, int64_t n_hq, const float* pred_sr,
                     const float* gt_sr, int64_t n_sr, float* dhq, float* dsr, float* loss, float* scratch,
                     void* stream);
/* replaces self.cri_pix(pred, self.gt) with L1LossSonar(loss_weight, reduction, binary)
 * (Train/basicsr/models/losses/losses.py:25-65, Restomer.yml) over n floats:
 *   reduction 0 = 'mean': loss[0] = loss_weight (mean|p - t| + mean|[p > binary] - [t > binary]|)
 *   reduction 1 = 'sum':  both terms are sums
 * The binarised term carries no gradient: dpred = sign(p - t) float32(loss_weight / n) ('mean') or
 * sign(p - t) float32(loss_weight) ('sum'), exactly 0.0 on a tie; the comparison with `binary` is strictly >.
 * dpred NULL = loss only.  `weight` is the loss's element-weight argument and must be NULL (ImageCleanModel
 * never passes one, image_restoration_model.py:212).  reduction outside {0, 1} ('none'), a non-null weight, a null
 * pred / target / loss / scratch or n <= 0: KDLAE_EINVAL_CONFIG; nothing is launched.  Two stages in a fixed order
 * (per-block partials of at most 1024 blocks, one double sum over them in block order), no atomics: equal
 * inputs give equal bits.  scratch: device buffer of kdlae_train_l1sonar_scratch_floats() floats. */
int64_t kdlae_train_l1sonar_scratch_floats(void);
int kdlae_train_l1sonar(const float* pred, const float* target, int64_t n, float loss_weight, float binary,
                        int reduction, const float* weight, float* dpred, float* loss, float* scratch, void* stream);
/* replaces torch.nn.utils.clip_grad_norm_(params, max_norm) + torch.optim.AdamW.step (:215-218) over
 * flat buffers: g = gscale * grad (gscale = 1/world_size after a summing all-reduce), clipped to
 * max_norm (<= 0: no clip); `step` counts from 1.  The norm covers all n gradients; the update
 * covers the host array `ranges` of nranges [begin, end) pairs (nranges 0: all n), mirroring
 * torch.optim skipping parameters whose .grad is None.  scratch: kdlae_train_adamw_scratch_floats()
 * floats; after the call scratch[2048] holds the gradient norm (after gscale, before clipping). */
int64_t kdlae_train_adamw_scratch_floats(void);
int kdlae_train_clip_adamw(float* theta, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                           float gscale, float max_norm, float lr, float beta1, float beta2, float eps,
                           float weight_decay, int step, const int64_t* ranges, int nranges, float* scratch,
                           void* stream);
/* replaces Mixing_Augment.mixup (image_restoration_model.py:25-61, KDLAET.yml mixing_augs):
 * out[b] = lam * in[b] + (1 - lam) * in[perm[b]] over B samples of per_sample floats; perm is a
 * device int[B]; lam and perm are drawn on the host exactly as the reference draws them. */
int kdlae_train_mixup(const float* in, float* out, int B, int64_t per_sample, const int* perm, float lam,
                      void* stream);
/* replaces BaseModel.model_ema(decay) (Train/basicsr/models/base_model.py:54-62) over the flat buffers. */
int kdlae_train_ema(float* ema, const float* theta, int64_t n, float decay, void* stream);

/* ------------------------------------------------------------------ KDLAE-S training
 * One optimisation step of BasicSR's ImageCleanModel on KDLAE_student with KDLAES.yml
 * (Train/Denoising/Options/paper202508/KDLAES.yml: L1LossForVideoFrames, clip_grad_norm_, AdamW):
 * forward with saved activations and the backward of every layer (Conv3d 3x3x3 + ReLU, MaxPool3d
 * (1,2,2), ConvTranspose3d (1,2,2) + skip, out_conv + residual; KDLAE/KDLAE_model.py:395-431).
 * Parameters / gradients: flat caller-owned buffers of kdlae_st_num_floats floats in state_dict order,
 * every key 16-byte aligned (pads zero), as for kdlae_tt_*; kdlae_train_clip_adamw / _ema / _mixup
 * apply unchanged. */
typedef struct kdlae_st_handle kdlae_st_handle;
/* replaces KDLAE_student.__init__ for training (KDLAE_model.py:341-384); inp/out_channels 1, kernel_size 3,
 * hidden_channels divisible by 4 (KDLAE_EINVAL_CONFIG otherwise) */
int kdlae_st_create(const kdlae_s_config* cfg, int device, kdlae_st_handle** out);
int kdlae_st_destroy(kdlae_st_handle* h);
int kdlae_st_num_params(const kdlae_st_handle* h);
int kdlae_st_param_info(const kdlae_st_handle* h, int index, const char** name, int64_t* numel, int64_t* offset);
int64_t kdlae_st_num_floats(const kdlae_st_handle* h);
int64_t kdlae_st_workspace_bytes(const kdlae_st_handle* h, int B, int F, int H, int W);
/* replaces `preds = self.net_g(self.lq)` (image_restoration_model.py:200) for KDLAE_student: x, out [B, F, H, W];
 * activations stay in `workspace` for kdlae_st_backward */
int kdlae_st_forward(kdlae_st_handle* h, const float* theta, const float* x, int B, int F, int H, int W, float* out,
                     void* workspace, int64_t workspace_bytes, void* stream);
/* replaces `l_pix.backward()` (:213): dout [B, F, H, W] -> grad (flat, overwritten); x gets no gradient */
int kdlae_st_backward(kdlae_st_handle* h, const float* theta, const float* dout, float* grad, void* workspace,
                      int64_t workspace_bytes, void* stream);
/* replaces L1LossForVideoFrames(l1loss_weight, reduction, temporal_weight, binary)(pred, target)
 * (Train/basicsr/models/losses/losses.py:409-526) for pred / target [N, frames, H, W] (hw = H W):
 * loss[0] = l1loss_weight (mean|p - t| + mean|bin(p) - bin(t)|) + temporal_weight mean|dp - dt| (frame
 * differences; frames == 1: no temporal term); reduction 0 = 'mean', 1 = 'sum' ('max' / 'mix': EINVAL_CONFIG).
 * dpred receives d loss / d pred.  scratch: kdlae_train_l1frames_scratch_floats() floats. */
int64_t kdlae_train_l1frames_scratch_floats(void);
int kdlae_train_l1frames(const float* pred, const float* target, int N, int frames, int64_t hw, float l1loss_weight,
                         float temporal_weight, float binary, int reduction, float* dpred, float* loss, float* scratch,
                         void* stream);

/* ------------------------------------------------------------------ ASDQE training
 * One micro-batch of Train/ASDQE.py:95-122 on DenoiseRatePredictor in train mode: BatchNorm2d uses
 * batch statistics over all B x H' x W' pixels (the zero-padded ones of pad_to_multiple included) and
 * updates its running statistics (momentum 0.1), Dropout multiplies by caller-supplied masks.
 * fp32 throughout.  Parameters / gradients: flat caller-owned buffers of asdqe_train_num_floats floats in
 * named_parameters() order, every key 16-byte aligned (pads zero), as for kdlae_tt_* / kdlae_st_*;
 * kdlae_train_clip_adamw / _ema apply unchanged.  BatchNorm running statistics: a second flat buffer
 * of asdqe_train_num_stat_floats floats, per BatchNorm [running_mean | running_var] in state_dict
 * order. */
typedef struct asdqe_train_handle asdqe_train_handle;
/* replaces DenoiseRatePredictor.__init__ for training (ASDQE_model.py:127-156); same limits as asdqe_create */
int asdqe_train_create(const asdqe_config* cfg, int device, asdqe_train_handle** out);
int asdqe_train_destroy(asdqe_train_handle* h);
int asdqe_train_num_params(const asdqe_train_handle* h);
int asdqe_train_param_info(const asdqe_train_handle* h, int index, const char** name, int64_t* numel, int64_t* offset);
int64_t asdqe_train_num_floats(const asdqe_train_handle* h);
int64_t asdqe_train_num_stat_floats(const asdqe_train_handle* h);
/* Device bytes of the caller-owned workspace (saved activations + backward scratch); -1 (and
 * kdlae_last_error) for a batch whose buffers cannot be indexed: B * H' * W' * 128 must be < 2^31. */
int64_t asdqe_train_workspace_bytes(const asdqe_train_handle* h, int B, int H, int W);
/* replaces `pred = model(lq, gt)` under model.train() (Train/ASDQE.py:103): lq, gt [B, in_channels, H, W];
 * score [B, 1]; stats: the running statistics, updated in place; mask1 [B, 256] / mask2 [B, 64]: the two
 * Dropouts' masks, already scaled (0 or 1 / (1 - p)), NULL = identity.  Activations stay in `workspace`
 * for asdqe_train_backward. */
int asdqe_train_forward(asdqe_train_handle* h, const float* theta, float* stats, const float* lq, const float* gt,
                        int B, int H, int W, const float* mask1, const float* mask2, float* score, void* workspace,
                        int64_t workspace_bytes, void* stream);
/* replaces `loss.backward()` (:107): dscore [B, 1] -> grad (flat; accumulate != 0: grad += d loss / d theta,
 * else grad = ...; the reference accumulates over 32 micro-batches, :101-112).  The conv biases that feed a
 * BatchNorm get exact zeros (their gradient is mathematically zero).  The images get no gradient.  One
 * backward per forward: KDLAE_ESTATE when no forward is live. */
int asdqe_train_backward(asdqe_train_handle* h, const float* theta, const float* dscore, float* grad, int accumulate,
                         void* workspace, int64_t workspace_bytes, void* stream);
/* replaces nn.MSELoss()(pred, score) / accumulation_steps (Train/ASDQE.py:88,104-105) over n scores:
 * loss[0] = mean((s - t)^2) (unscaled), loss[1] = mean |s - t| (the loop's MAE); dscore = scale 2 (s - t) / n. */
int kdlae_train_mse(const float* score, const float* target, int n, float scale, float* dscore, float* loss,
                    void* stream);

/* ---- Validation metric (metrics.hip).  Replaces the two reductions of calculate_psnr
 * (Train/basicsr/metrics/psnr_ssim.py:53-70) over contiguous fp32 device tensors pred [B, C, Hs, Ws] and
 * gt [B, C, Hg, Wg]: the compared region is the top-left h x w window of both (pad_test's crop,
 * image_restoration_model.py:236-237, so neither the padded output nor the unpadded target needs a copy)
 * minus crop_border pixels on all four sides (:58-60).
 *   mode 0: the floats as they are (val.use_image: false, every yml under paper202508/);
 *   mode 1: both operands through tensor2img's uint8 route first (img_util.py:67-68,91-94: clamp to
 *           [0, 1], * 255 in fp32, round half to even), compared on the 0..255 scale.
 * out [B][2] (device, fp64): out[b][0] = sum of (pred - gt)^2 over image b's region, out[b][1] = max of pred
 * over it (after the quantisation in mode 1; psnr_ssim.py:69 looks at the first operand only).  fp64
 * accumulation in a fixed two-stage order without atomics: equal inputs give equal bits.  The host
 * finishes: mse = sse / n, inf when 0, else 20 log10((max <= 1 ? 1 : 255) / sqrt(mse)).  Nothing here
 * synchronises; the result stays on the device.  2 crop_border >= h or w: KDLAE_EINVAL_SHAPE.
 * scratch: device buffer of kdlae_metric_scratch_bytes() bytes (8-byte aligned). */
int64_t kdlae_metric_scratch_bytes(void);
int kdlae_metric_psnr(const float* pred, const float* gt, int B, int C, int Hs, int Ws, int Hg, int Wg, int h, int w,
                      int crop_border, int mode, double* out, void* scratch, void* stream);

/* ---- SSIM (ssim.hip).  The other metric of the reference's val.metrics block, over the same geometry and
 * with the same `mode` as the PSNR entry above: the top-left h x w window of both stored tensors minus
 * crop_border on the four sides; mode 1 quantises both operands as tensor2img does.  Five windowed means
 * (mu1, mu2, E[x^2], E[y^2], E[xy]; the 11 taps g[i] = exp(-(i - 5)^2 / (2 * 1.5^2)) / sum on each axis) and the
 * map (2 mu1 mu2 + C1)(2 s12 + C2) / ((mu1^2 + mu2^2 + C1)(s1^2 + s2^2 + C2)), C1 = (0.01 L)^2, C2 = (0.03 L)^2.
 *   variant 0: calculate_ssim -> _ssim_3d (Train/basicsr/metrics/psnr_ssim.py:146-197,240-318): the 11^3 Conv3d
 *              over the (H, W, C) volume with replicate padding, i.e. filter indices clamped to the edge of the
 *              compared window on H and W (never to stored pixels beyond it) and a C x C mix along the channels
 *              (the squares and the product are formed before the mix).  h * w * C map entries; L = 1 when
 *              max(pred) <= 1, else 255 (:307).  1 <= C <= 4.
 *   variant 1: Train/utils.py:31-78 (= _ssim, psnr_ssim.py:73-114): per channel, valid positions only, so
 *              (h' - 10)(w' - 10) entries per channel of the cropped h' x w' window; L = 255.  h', w' >= 11.
 * out [B][4] (device, fp64): out[b][0] = sum of the map with the L = 1 constants (variant 1: 0), out[b][1] =
 * the sum with the L = 255 constants, out[b][2] = max of pred over the region (after the quantisation in
 * mode 1), out[b][3] = the number of map entries.  SSIM = out[b][max <= 1 ? 0 : 1] / out[b][3] (variant 0),
 * out[b][1] / out[b][3] (variant 1): both sums come from one pass, so nothing synchronises and the result
 * stays on the device.  Taps, moments, map and sums are fp64 (E[x^2] - mu^2 against C2 = 9e-4 L^2 is where fp32
 * loses its digits); fixed two-stage order without atomics: equal inputs give equal bits, and equal
 * operands give exactly 1.  Nothing outside the compared region is read.  Errors are found before any launch:
 * window / crop_border as above, variant 1 under 11 pixels or variant 0 with C > 4: KDLAE_EINVAL_SHAPE.
 * scratch: device buffer of the size the first function below returns, in bytes (8-byte aligned). */
int64_t kdlae_metric_ssim_scratch_bytes(void);
int kdlae_metric_ssim(const float* pred, const float* gt, int B, int C, int Hs, int Ws, int Hg, int Wg,
                      int h, int w, int crop_border, int mode, int variant,
                      double* out, void* scratch, void* stream);

/* ---- NIQE (niqe.hip).  The no-reference metric of Train/basicsr/metrics/niqe.py:10-205, up to the per-block
 * moments its AGGD fits need, over the geometry and with the `mode` of the two entries above: the top-left h x w
 * window of the stored x [B, C, Hs, Ws] minus crop_border on the four sides, then the largest multiple of 96 on
 * each axis (H' x W'; nbh = H' / 96, nbw = W' / 96 blocks).  Values are on the 0..255 scale: mode 0 takes the floats
 * as they are, mode 1 quantises as tensor2img does.  C = 3 is RGB and becomes the Y of MATLAB's YCbCr in the
 * reference's operation order (/ 255 in fp32; 24.966 B + 128.553 G + 65.481 R + 16 in fp64, each product and sum
 * rounded, / 255; to fp32; * 255); C = 1 takes the same / 255, * 255 in fp32.  convert: 0 ('y') only.
 *   MSCN field f = (x - mu) / (sqrt|E[x^2] - mu^2| + 1): mu and E over window49 (host pointer, 7 x 7 doubles,
 *   row-major, the `gaussian_window` of niqe_pris_params.npz) the way scipy.ndimage.convolve(mode='nearest')
 *   forms them: the flipped window in row-major order, an fp64 multiply and an fp64 add per tap (nothing fused),
 *   one rounding to fp32, indices clamped to the edge of the H' x W' image (never to stored pixels beyond it,
 *   which are not read).  The rest is correctly rounded fp32.  Scale 2 repeats this on the 2 x 2 mean of the
 *   image (((a + b) / 2 + (c + d) / 2) / 2 of the / 255 values, * 255, each step rounded in fp32; it stands for
 *   cv2.resize(.., INTER_LINEAR) at one half) with 48 x 48 blocks.
 *   Per block five maps: f and the fp32 products f * roll(f, s) for s = (0,1), (1,0), (1,1), (1,-1), the roll
 *   wrapping inside the block.
 * out [B][2 scales][nbw * nbh blocks][5 maps][5] (device, fp64), blocks in the reference's order (index
 * bx * nbh + by): n_neg, n_pos, sum of x^2 over x < 0, sum of x^2 over x > 0, sum of |x|; zeros are on neither
 * side.  fp64 sums in a fixed order without atomics: equal inputs give equal bits.
 * field_s1 [B][H'][W'] / field_s2 [B][H'/2][W'/2] (device, may be NULL): the two fields, for tests.
 * scratch: device buffer of at least kdlae_metric_niqe_scratch_bytes(B, h, w) bytes (4-byte aligned), its size in
 * scratch_bytes.  Nothing synchronises.  Errors are found before any launch: C not 1 or 3, crop_border leaving
 * no pixel, fewer than 96 pixels left on an axis, a window outside the storage, scratch too small:
 * KDLAE_EINVAL_SHAPE; null pointers, mode or convert out of range: KDLAE_EINVAL_CONFIG. */
int64_t kdlae_metric_niqe_scratch_bytes(int B, int h, int w);
int kdlae_metric_niqe(const float* x, int B, int C, int Hs, int Ws, int h, int w, int crop_border, int mode,
                      int convert, const double* window49, double* out, float* field_s1, float* field_s2,
                      void* scratch, int64_t scratch_bytes, void* stream);

/* ---- Progressive-learning batch preparation (augment.hip).  Replaces the host loop between the data loader and
 * feed_train_data (Train/basicsr/train.py:374-448): the stage's sub-batch (random.sample), one crop window for
 * the whole batch, and the Bernoulli input mask of paired_image_dataset.py:19-36 (a kept pixel comes back bit
 * for bit, a masked one becomes -value, not 0).  The stage rule and the host draws stay with the caller
 * (augment.py); one launch serves every tensor of the batch (img, denoise_rate, hq, sr):
 *   dst[b, c, i, j] = keep ? src[index[b], c, y0 + i, x0 + j] : -value
 * The mask bit is keep[b, c, i, j] when `keep` is given (the bit-comparable route: the caller draws it as the
 * reference does), else Philox4x32-10 with key = (seed lo, seed hi) and counter = (q lo, q hi, call lo, call hi),
 * q = e / 4 for the linear index e into that segment's dst; element e takes word e % 4, u = (word >> 8) * 2^-24
 * and keep = u >= prob, both in fp32.  Segment s of one call uses call + s.  Nothing synchronises, allocates or
 * uses atomics; element indices are 64-bit; src is never written.  An index entry outside [0, B_src) is the
 * caller's responsibility.  Errors are found before any launch. */
typedef struct {
  const float* src;      /* [B_src, C, Hs, Ws] contiguous fp32 */
  float* dst;            /* [B, C, h, w] contiguous */
  int B_src, C, Hs, Ws, h, w, y0, x0;   /* window rows y0..y0+h of dim 2, cols x0..x0+w of dim 3 */
  float prob;            /* <= 0: plain copy; >= 1: every pixel masked */
  const uint8_t* keep;   /* nullable [B, C, h, w], 1 = keep; null with prob > 0: Philox */
} kdlae_prep_seg;
int kdlae_train_prepare(const kdlae_prep_seg* segs, int nseg /* 1..4 */, const int* index /* device int[B], null = identity */,
                        int B, float value, uint64_t seed, uint64_t call, void* stream);
/* The per-frame rule of Dataset_PairedMutiImage (paired_image_dataset.py:219-272) over src, dst [B, F, H, W]
 * (dst != src, F <= 16): frame f is masked with probs[f] as above (<= 0 copies, >= 1 masks every pixel; keep
 * [B, F, H, W] or Philox over the linear index into dst).  interpolate != 0 (F odd): an odd frame f is the mask
 * of 0.5f * (masked[f-1] + src[f+1]), one fp32 add then the multiply: the reference works in place in frame
 * order, so frame f-1 is already masked when f reads it and frame f+1 is not.  masked[f-1] is recomputed from
 * src and frame f-1's own mask bit; dst is never read. */
int kdlae_train_mask_frames(const float* src, float* dst, int B, int F, int H, int W,
                            const float* probs /* host float[F] */, int interpolate, float value,
                            const uint8_t* keep /* nullable [B, F, H, W] */, uint64_t seed, uint64_t call, void* stream);

/* ---- Dataset sample transforms (csrc/data.hip): the per-sample work of Dataset_SuperRestoration_param and
 * Dataset_PairedMutiImage (Train/basicsr/data/paired_image_dataset.py:902-982, 160-294) between image decode and
 * the batch: pad, crop, noise, flips / rotations, layout, normalisation.  Plain streaming kernels; nothing
 * synchronises or allocates; element indices are 64-bit; errors are found before any launch.
 *
 * One item = one source image and one destination slot.  The source (u8 or fp32, element strides sy, sx, sc, so
 * HWC-interleaved and CHW-planar both fit) sits on a virtual canvas: centred on Hc x Wc with zeros around it
 * (top = (Hc - Hs) / 2, left = (Wc - Ws) / 2: pad_image), then extended at the bottom / right to Hp x Wp by
 * reflect101 (cv2.BORDER_REFLECT_101, numpy 'reflect') or symmetric (cv2.BORDER_REFLECT, numpy 'symmetric'); the
 * reflection sees the zero-padded canvas and repeats for pads longer than the canvas.  Window (top, left, h, w)
 * on that canvas; the dihedral code (bit 2 transpose, bit 1 flip rows, bit 0 flip columns) maps it to dst
 * [C, h', w'] = transpose?(flip_cols?(flip_rows?(window))), (h', w') = (w, h) with a transpose; reverse_c stores
 * source channel c at C - 1 - c.  Value: u8 -> float(v) / 255.0f (one fp32 division); with noise
 * float(clip(double(x) + (loc + scale * z / div), 0, 1)), every step a rounded fp64 operation in this order, z
 * taken at the window coordinate (i, j, c) BEFORE the dihedral map and the channel reversal from the fp64 array z
 * [h, w, C] (noise = 1) or from Philox4x32-10 (noise = 2: key = seed, counter = (e / 2, call + item number),
 * e = (i * w + j) * C + c, words (0, 1) for an even e and (2, 3) for an odd one, u1 = ((w0 >> 8) + 1) * 2^-24,
 * u2 = (w1 >> 8) * 2^-24, z = sqrtf(-2 logf(u1)) * cosf(2 pi u2) in fp32); with `counts` the noise applies only
 * when (double)max(counts[0], counts[1]) / count_n > count_thr, decided on the device; then (x - mean[c']) / std[c']
 * in fp32 by destination channel where given (each nullable).  dst must not overlap src.  `items` is a host
 * table; it is validated, copied to `table` (device, n_items * sizeof(kdlae_data_item) bytes) on the stream and
 * served by one launch.  The copy reads pageable host memory, so this one entry may wait on the host until the
 * stream has reached it, and is not for graph capture; its result does not depend on the stream it is given. */
typedef struct {
  const void* src;        /* device, u8 or fp32 */
  float* dst;             /* device fp32 [C, h', w'] contiguous */
  const double* z;        /* device fp64 [h, w, C], noise == 1 */
  const int32_t* counts;  /* nullable device int32[2] of kdlae_data_count: the noise is conditional */
  const float* mean;      /* nullable device fp32 [C] */
  const float* std;       /* nullable device fp32 [C] */
  int64_t sy, sx, sc;     /* source element strides of row, column, channel */
  int64_t count_n;
  double count_thr;
  double loc, scale, div;
  int src_u8;             /* 1: u8 source, 0: fp32 */
  int Hs, Ws, C;
  int Hc, Wc, Hp, Wp;
  int pad_mode;           /* 0 none (Hp x Wp == Hc x Wc), 1 reflect101, 2 symmetric */
  int top, left, h, w;
  int dihedral;           /* 0..7 */
  int reverse_c;
  int noise;              /* 0 off, 1 z array, 2 Philox */
  int reserved;
} kdlae_data_item;
int kdlae_data_sample(const kdlae_data_item* items /* host */, void* table /* device */, int n_items, uint64_t seed,
                      uint64_t call, void* stream);
/* counts[b] = (number of x[b, :] == 0.0f, number == 1.0f) over x [B, n_per_sample]; integer adds only, so the
 * result does not depend on the order; counts is zeroed here.  -0.0f counts as zero. */
int kdlae_data_count(const float* x, int B, int64_t n_per_sample, int32_t* counts /* device [B][2] */, void* stream);
/* In place over x [B, C, hw]: where (double)max(counts[b]) / (C * hw) > thr, x = x + nudge (one fp32 add: the
 * reference's `img_lq + 1e-14` moves exact zeros only); then (x - mean[c]) / std[c] where given (device, nullable). */
int kdlae_data_finish(float* x, int B, int C, int64_t hw, const int32_t* counts, double thr, float nudge,
                      const float* mean, const float* std, void* stream);

/* ---- Kernel self-test entry points (not part of the drop-in boundary; nothing here is on a forward
 * or training path).  tests/test_kernel_variants*_gpu.py: kdlae_debug_tgemm, kdlae_debug_gemm,
 * kdlae_debug_gram, kdlae_debug_ln, kdlae_debug_small_in, kdlae_debug_bn;
 * tests/test_narrow_kernels_gpu.py: kdlae_debug_small_in (2-D, transposed), kdlae_debug_bn ops 6-9,
 * kdlae_debug_head_train, kdlae_debug_train_s ops 6-7; tests/test_bn_kernels_gpu.py: kdlae_debug_bn ops 0-5 (the
 * batch-statistics BatchNorm kernels and the bilinear x2 pair, float64 with counted bounds);
 * tests/test_train_kernels_gpu.py: kdlae_debug_train, kdlae_debug_train_s (the training steps'
 * non-GEMM kernels); tests/test_infer_kernels_gpu.py: kdlae_debug_infer (the forward paths' other kernels).
 * One launch of the training GEMM family on caller device buffers:
 *   C(m, n) = sum_k A(m, k) B(k, n) [+ bias[n]] [+ rs[n] R(m, n)], batch z = z1 * nz2 + z2, every
 *   operand offset by z1 * b?1 + z2 * b?2 (floats); amode 1 = implicit 3x3 im2col of the NHWC view A
 *   (pixel stride lda, k = tap * Cg + c, dilation dil, zero padding), bmode 1 = the NHWC view B shifted
 *   by tap z2 (conv weight gradient), bmode 2 / 3 = a 3x3 OIHW weight as the forward / transposed
 *   conv operand, bmode 4 = implicit 3x3x3 im2col of the NDHWC view B, n = tap * Cg + c (Conv3d weight
 *   gradient; pixel-reduction kernel) (see train_kernels.h TGemm).  route: 0 = the engine's own dispatch, 1 = the
 *   row-streaming kernel, 2 = the pixel-reduction kernel (needs partial), 3 = the tiled kernels. */
typedef struct kdlae_debug_tgemm_desc {
  const float* A; int64_t sam, sak; int amode;
  const float* B; int64_t sbk, sbn; int bmode;
  float* C; int64_t scm, scn;
  const float* bias;
  const float* R; int64_t srm, srn;
  const float* rs;
  int M, N, K, nz1, nz2;
  int64_t bA1, bA2, bB1, bB2, bC1, bC2, bR1, bR2, brs1, brs2;
  int Bn, H, W, Cg, dil;
  int64_t lda, ldb;
  float* partial; int64_t partial_floats;
  int route;
  int c_pad_ok;
  int F;  /* frames of the bmode 4 (implicit 3x3x3) B view; 0 = 1 */
} kdlae_debug_tgemm_desc;
int kdlae_debug_tgemm(const kdlae_debug_tgemm_desc* d, void* stream);

/* One launch of the inference implicit-GEMM family (gemm.hip) with the tile shape forced:
 *   out[b][p][n] = relu?( sum_k A'[b][p][k] Wp(n, k) + bias[n] (+ R) ), A' = A or LN(A) over ln_C
 *   (ln 1 BiasFree, 2 WithBias, unit weight); ksize 3: implicit 3x3 (kt 3: 3x3x3 over F frames),
 *   k = tap * 16 cg_per_tap + c, zero padding = dil; out_mode 1 / 2 stores through PixelUnshuffle(2)
 *   / PixelShuffle(2) (R then in the output geometry).  Wp: fragment-packed [ntiles][kgroups][64][4],
 *   element (l, e) of (t, g) = W(16 t + l % 16, 16 g + 4 (l / 16) + e); + b * w_img_stride per image.
 *   Wm != 0: fused attention output, x1 = R + Wm v (+ bias_m) stored to out1, then out = LN(x1) W.
 *   stats: [pixels][2] scratch when LN meets a chunked K.  group_tiles > 0: resident schedule.
 *   tiles_per_block 0: the engine's grid rule.  route 0: production dispatch; 1: the r01
 *   conv_gemm_kernel of (NT, KG) (the fallback for ld % 4 != 0 views). */
typedef struct kdlae_debug_gemm_desc {
  const float* A; int lda;
  int Bn, F, H, W;
  int ksize, kt, dil, cg_per_tap, kgroups;
  const float* Wp; int64_t w_img_stride; int ntiles, N;
  const float* bias;
  float* out; int ldo;
  const float* R; int ldr;
  int ln, ln_C, relu, out_mode;
  float* stats;
  const float* Wm; int64_t wm_img_stride; const float* bias_m; float* out1; int ldo1;
  int NT, KG, wpe, group_tiles, tiles_per_block;
  int route;
} kdlae_debug_gemm_desc;
int kdlae_debug_gemm(const kdlae_debug_gemm_desc* d, void* stream);
/* Entry i of a compiled variant table: family 0 conv_gemm_kernel (NT, KG, CONV3, OUT, PF, WPE, RES),
 * 1 gemm_res_kernel (NT, KG, NCH, PF), 2 gemm_chunk_kernel (NT, KG, CONV3, OUT), 3 gemm_attn_in_kernel
 * (NT, KG, NCH).  Fills v[0..6]; returns 1, or 0 past the end. */
int kdlae_debug_gemm_variant(int family, int i, int* v);

/* MDTA pass 1 + 2 (mdta.hip): depthwise 3x3 of qkv ([P][ld], wdw [9][3C] tap-major, bdw [3C]), v
 * stored to v_out, per (image, head) the Gram q k^T and the squared norms summed into
 * reduced[Bn * heads][Ch^2 + 2 Ch] (Gram in accumulator order: element (i * CT + j) * 256 + 4 l + e =
 * G[16 i + 4 (l / 16) + e][16 j + l % 16], CT = Ch / 16; then |q_c|^2, |k_c|^2).  partial: scratch of
 * partial_floats.  route 0: production (ring kernel where it applies), 1: without the ring kernel
 * (zeros ignored), 2: the generic 64-pixel-step kernel, 3: the ring kernel without v (q | k only: v_out
 * may be null and is not written; KDLAE_EINVAL_SHAPE where the ring kernel does not apply). */
typedef struct kdlae_debug_gram_desc {
  const float* qkv; int ld;
  const float* wdw; const float* bdw;
  float* v_out; int ldv;
  float* partial; int64_t partial_floats;
  float* reduced;
  const float* zeros;
  int C, heads, Bn, H, W;
  int route;
} kdlae_debug_gram_desc;
int kdlae_debug_gram(const kdlae_debug_gram_desc* d, void* stream);

/* Training LayerNorm (train.hip) over P pixels of C channels: dir 0 forward y = LN(x) w (+ b),
 * stats[P][2]; dir 1 backward dx = R + dLN(dy), part[nblk][C | 2 C] the per-block weight (and bias)
 * gradient partials.  route 0: production dispatch, 1: the one-wave-per-pixel kernels. */
typedef struct kdlae_debug_ln_desc {
  int dir;
  const float* x; int ldx;
  const float* w; const float* b;
  int C; int64_t P; int biasfree;
  float* y; int ldy;
  float* stats;
  const float* dy; int ldd;
  const float* R; int ldr;
  float* dx; int lddx;
  float* part; int nblk;
  int route;
} kdlae_debug_ln_desc;
int kdlae_debug_ln(const kdlae_debug_ln_desc* d, void* stream);

/* Small-input 3x3 / 3x3x3 conv (conv_small.hip), Cin * 9 * kt <= 36, Cout % 16 == 0: input element
 * (b, frame t, y, x, c) at in[b sb + t st + y sy + x sx + c sc] (minus in_sub at the same offset),
 * w [Cout][Cin][kt][3][3], NHWC output [Bn * F * H * W][ldo] (16-byte aligned, ldo % 4 == 0); valid input
 * extent vh x vw (0 = H, W).  wt > 0 (kt 1, wt >= Cout): the conv is the transpose (the input gradient) of a
 * Cout' = Cin, Cin' = wt conv whose weight w is [Cin][wt][3][3]: out[p][n] = sum_{c, tap} in[p + off(tap)][c]
 * w[c][n][8 - tap], n < Cout. */
typedef struct kdlae_debug_small_in_desc {
  const float* in; int64_t sb, sc, sy, sx, st;
  const float* in_sub;
  int Cin, Cout, dil, kt, F;
  const float* w; const float* bias;
  float* out; int ldo;
  int Bn, H, W, vh, vw, relu;
  int wt;
} kdlae_debug_small_in_desc;
int kdlae_debug_small_in(const kdlae_debug_small_in_desc* d, void* stream);

/* ASDQE training kernels (bn_train.hip) over NHWC views (C % 4 == 0, every ld % 4 == 0), one op per call:
 *   0 bn_stats: x [P][ldx] -> mean, rstd [C] (+ the running update of running_mean / running_var when given)
 *   1 bn_apply_relu: out = relu((x - mean) rstd gamma + beta)
 *   2 bn_bwd_reduce: (dy, y, x) -> dgamma, dbeta [C]
 *   3 bn_bwd_dx: out = gamma rstd (dy [y > 0] - dbeta / P - xhat dgamma / P)
 *   4 upsample2x_bwd: x = the [N][2h][2w] gradient -> out [N][h][w]       5 upsample2x: x [N][h][w] -> out
 *   6 asdqe_pack_inputs: x = lq, y = gt, both NCHW [N][C = ci <= 4][h][w] -> out = xin [N Hp Wp][12] (16-byte
 *     aligned): lq, gt, lq - gt at 4 channels each, zero past ci and past h x w; Hp >= h, Wp >= w
 *   7 narrow_w_copy: x = src [N = Cout][4][9] -> out = dst [N][C = ci <= 4][9]
 *   8 bcast_rows: x = N rows of C floats at row stride ldx -> out[(n P + p) ldo + c] = x[n ldx + c] scale, p < P
 *   9 grad_commit: out[i] = (accumulate ? out[i] : 0) + x[i], i < P (P % 4 == 0, both 16-byte aligned)
 * part: scratch of >= 2048 C floats (ops 0, 2).  A bad argument of ops 5-9 is KDLAE_EINVAL_* before any launch (op 5:
 * C >= 4, C % 4 == 0, ldx, ldo >= C and % 4 == 0, 16-byte aligned views); ops 0-4 are refused by the launchers' own
 * check, KDLAE_EHIP "invalid argument", before any launch as well. */
typedef struct kdlae_debug_bn_desc {
  int op;
  const float* x; int ldx;
  const float* y; int ldy;
  const float* dy; int ldd;
  float* out; int ldo;
  float* mean; float* rstd;
  float* running_mean; float* running_var; float momentum;
  const float* gamma; const float* beta;
  float* dgamma; float* dbeta;
  int C; int64_t P;
  int N, h, w;
  float* part; int64_t part_floats;
  int Hp, Wp;       /* op 6 */
  int accumulate;   /* op 9 */
  float scale;      /* op 8 */
} kdlae_debug_bn_desc;
int kdlae_debug_bn(const kdlae_debug_bn_desc* d, void* stream);

/* ASDQE train-mode regressor head (bn_train.hip; csrc/train_a.h HeadTrain), one image per block:
 *   g = inv_hw sum_slots partial [B][slots][C]; f = wo g + bo [M]; a1 = w1 f + b1 [N1]; h1 = relu(a1) mask1;
 *   a2 = w2 h1 + b2 [N2]; h2 = relu(a2) mask2; score = tanh(w3 . h2 + b3).  masks [B][N1] / [B][N2] or null.
 * dir 0: forward -> score [B], save [B][2 (C + M + N1 + N2) + 4] (g, f, a1, a2, then the backward's rows).
 * dir 1: backward from dscore [B] and the save of a dir 0 call with the same operands -> the eight gradients
 *   (each a sum over the images) and, per image, dgap [C] at save row offset C + 2 (M + N1 + N2) + 4.
 * C, M, N1, N2 <= 1024; save_floats >= B (2 (C + M + N1 + N2) + 4); a bad argument is KDLAE_EINVAL_* before
 * any launch. */
typedef struct kdlae_debug_head_train_desc {
  int dir;
  const float* partial; int slots, C; float inv_hw;
  const float* wo; const float* bo; int M;
  const float* w1; const float* b1; int N1;
  const float* w2; const float* b2; int N2;
  const float* w3; const float* b3;
  const float* mask1; const float* mask2;
  float* score; int B;
  float* save; int64_t save_floats;
  const float* dscore;
  float* gwo; float* gbo; float* gw1; float* gb1; float* gw2; float* gb2; float* gw3; float* gb3;
} kdlae_debug_head_train_desc;
int kdlae_debug_head_train(const kdlae_debug_head_train_desc* d, void* stream);

/* Non-GEMM kernels of the KDLAE-T training step (train.hip, train_dwg.hip, train_small.hip; launch
 * interface and operand meaning: csrc/train_kernels.h), one launch per call on caller buffers
 * (tests/test_train_kernels_gpu.py).  NHWC views of Bn x H x W pixels at the pixel stride given
 * beside each pointer; geometry that a kernel cannot take (null operand, ld < width, Ch > 128, a
 * partial buffer too small, dw3_small_ok false, ...) returns KDLAE_EINVAL_* before any launch.
 *   op  0 attn_softmax  in0 = G [Bn heads][Ch][Ch], in1 = sumsq [Bn][2 C], w = temp [heads] -> out0 = Attn
 *   op  1 attn_bwd      + in2 = Attn, in3 = dAttn -> out0 = Mq, out1 = cq, out2 = ck [Bn heads][Ch],
 *                       out3 = dtemp partials [Bn heads]; Ch <= 127 (its Ch x Ch tile + 4 floats of LDS
 *                       must fit the 64 KiB a launch gets without opting in to more; the engine stops at 120)
 *   op  2 dw_fwd        in0 (C channels), w [C][9], bias (or null), flag = flip -> out0
 *   op  3 dwgate_fwd    in0 = y (2 C channels, C = hid), w [2 C][9], bias -> out0 = g (C), out1 = yd (2 C; or null)
 *   op  4 dwgate_bwd    in0 = dg, in1 = yd, in2 = y, w -> out0 = dy, part [blocks][10 * 2 C]
 *   op  5 dwgate_bwd_rc in0 = dg, in1 = y, w, bias -> out0 = dy, part (as op 4)
 *   op  6 dw_bwd        in0 = dyd, in1 = y (C channels), w -> out0 = dy, part [blocks][10 C]
 *                       (ops 4-6: blocks = kdlae_debug_train_blocks(0, Bn, H, W, 0))
 *   op  7 dw3_small     in0 = dY (C2 = Cout), in1 = X (C = Cin), flag = dil, nblk -> part [nblk][Cout Cin 9]
 *   op  8 colsum        in0 = x [nseg * P rows][ldi0], C = ncols, flag = square, nblk -> part [nseg][nblk][C]
 *   op  9 part_reduce   in0 = partials [nseg][nblk][pstride (0 = C)] -> out0 [nseg][C] (accumulate, scale)
 *   op 10 part_reduce_multi  red[0 .. nred) -> red[j].out [ncols]
 *   op 11 shuffle       flag = dir (0: PixelUnshuffle [Bn, 2H, 2W, C] -> [Bn, H, W, 4 C]; 1: PixelShuffle back)
 *   op 12 copy_cols     in0 [P][ldi0] -> out0 [P][ldo0], C columns (accumulate), zero_to
 *   op 13 nchw_to_nhwc  in0 [Bn][C][P] -> out0 [Bn P][ldo0] (accumulate)
 *   op 14 nhwc_to_nchw  in0 [Bn P][ldi0] (+ in1 = add [Bn][C][P] or null) -> out0 [Bn][C][P]
 *   op 15 pack_w3       w = OIHW 3x3 weight, C = Cg, C2 = N, flag = mode (2 or 3) -> out0 [9 Cg][N]
 *   op 16 dwgate_bwd_dx, 17 dwgate_bwd_rc_dx, 18 dw_bwd_dx: the operands of ops 4, 5, 6 -> out0 = dy alone, by
 *                       the kernels' dx-only variants (frozen dwconv weights: no weight-gradient partials;
 *                       same dy bits); part is ignored and may be null; op 18 does not read in1
 *   op 19 ln_bwd_dx     in0 = dy, in1 = x, in2 = stats [P][2], in3 = R (or null), w, C <= 512, P, nblk = blocks
 *                       -> out0 = dx (+ R): LayerNorm backward without the weight / bias partials (same dx bits
 *                       as kdlae_debug_ln dir 1); flag bit 0 = biasfree, bit 1 = route 1 (the generic kernel) */
typedef struct kdlae_debug_train_red {
  const float* part; float* out;
  int nblk, ncols, pstride;
  float scale;
} kdlae_debug_train_red;
typedef struct kdlae_debug_train_desc {
  int op;
  const float* in[4]; int ldi[4];
  const float* w; const float* bias;
  float* out[4]; int ldo[4];
  float* part; int64_t part_floats;
  int C, C2, heads, Bn, H, W;
  int64_t P;
  int flag, accumulate, zero_to;
  int nblk, nseg, pstride;
  float scale;
  int nred;
  kdlae_debug_train_red red[8];
} kdlae_debug_train_desc;
int kdlae_debug_train(const kdlae_debug_train_desc* d, void* stream);
/* Partial-buffer sizing of the kernels above: which 0 = spatial blocks of ops 4-6 for an n x a x b
 * (Bn x H x W) batch; which 1 = blocks op 7 uses for n pixels, Cin = a, Cout = b and a partial buffer
 * of cap floats.  -1 on bad arguments. */
int kdlae_debug_train_blocks(int which, int64_t n, int a, int b, int64_t cap);

/* Non-GEMM kernels of the KDLAE-S training step (train_s.hip; csrc/train_s.h) over NDHWC views of
 * B x F x H x W pixels, one launch per call:
 *   op 0 im2col3d      in0 = x (C) -> out = Xcol [pixels][27 C]
 *   op 1 col2im3d      in0 = dcol [pixels][27 C] -> out = dx (C % 4 == 0, ldo % 4 == 0, 16-byte aligned; accumulate)
 *   op 2 wperm         in0 [O][C][27] -> out [O][27][C] (dir 0) or back (dir 1)
 *   op 3 relu_mask     out = dy (in place) *= (in0 = y > 0)
 *   op 4 maxpool2_bwd  in0 = the pool's input [B, F, 2H, 2W], in1 = dout [B, F, H, W], in2 = dskip (or null) -> out = din
 *   op 5 upshuffle_add in0 = U [B, F, H/2, W/2] (4 C), in1 = skip [B, F, H, W], bias (or null) -> out = D
 *   op 6 pack_conv     in0 = w [O = cout][C = cin][27], dir = dx -> out = fragment order [ntiles][kgroups][64][4],
 *                      element (l, e) of (t, g) = Wm(16 t + l % 16, 16 g + 4 (l / 16) + e), k = tap in_pad + c;
 *                      dx 0: Wm(o, k) = w[o][c][tap] (nout = cout, nin = cin); dx 1: Wm(c, tap in_pad + o) =
 *                      w[o][c][26 - tap] (nout = cin, nin = cout); in_pad = nin rounded up to 16, ntiles =
 *                      ceil(nout / 16), kgroups = 27 in_pad / 16; zero past nout and nin
 *   op 7 relu          out = max(out, 0) in place over C of its ldo columns */
typedef struct kdlae_debug_train_s_desc {
  int op;
  const float* in[3]; int ldi[3];
  const float* bias;
  float* out; int ldo;
  int C, O, B, F, H, W;
  int accumulate, dir;
} kdlae_debug_train_s_desc;
int kdlae_debug_train_s(const kdlae_debug_train_s_desc* d, void* stream);

/* The forward paths' kernels outside the GEMM / Gram families, one launch sequence per call on caller
 * buffers (tests/test_infer_kernels_gpu.py; launch interface and operand meaning: csrc/kernels.h).
 * NHWC views of Bn x F x H x W pixels (F = 0 means 1) at the pixel stride given beside each pointer.
 * Every launcher precondition (null operand, ld < width, a misaligned float4 view, an unsupported
 * channel count, scratch too small, ...) returns KDLAE_EINVAL_* before any launch.  Weights that a
 * kernel reads as split records (mfma3.h) are handed in f32 fragment order [ntiles][kgroups][64][4]
 * (element (l, e) of (t, g) = W(16 t + l % 16, 16 g + 4 (l / 16) + e)) and converted into scratch the
 * call owns.  dw blocks: per 16-channel chunk g 512 floats, weight of tap t, half h (0 = x1, 1 = x2),
 * channel c at 32 t + 16 h + c, bias at 288 + 16 h + c (gdfn.hip).
 *   op 0 gdfn_out       in0 = project_in rows [P][2 hidS] chunk-interleaved (ldi0 == 2 hidS), w0 = dw blocks,
 *                       w1 = project_out [C/16][hidS/16] fragments, bias0 [C] (or null), R / ldr (or null; may be
 *                       out0), zeros (>= 16 zero floats) -> out0 (C); out_mode 0 = the default launches, 1 = C = 192 /
 *                       384 as C / 96 blocks per pixel tile (what KDLAE_DEBUG=gdfn_split selects; the same bits)
 *   op 1 ffn_fused      in0 = x (C), ln, w0 = project_in [2 hidS/16][C/16] fragments (chunk-interleaved rows),
 *                       bias0 [2 hidS] (chunk-interleaved, or null), w1 = dw blocks, w2 = project_out fragments,
 *                       bias1 [C] (or null) -> out0 = x + ffn(LN(x)) (must not overlap in0)
 *   op 2 mdta_fused     in0 = x (C), ln, w0 = qkv [3C/16][C/16] fragments, bias0 [3C] (or null), w1 = wdw [9][3C],
 *                       bias1 = bdw [3C] (or null), nseg, seg_rows, scratch = the Gram slots (Bn * (W/16) * nseg *
 *                       (C^2 + 2C) floats) -> out0 = v (C), out1 = reduced [Bn][C^2 + 2C] (layout: kdlae_debug_gram)
 *   op 3 attn_fold      in0 = reduced [Bn heads][Ch^2 + 2 Ch], w0 = project_out weight [C][C], w1 = temperature [heads]
 *                       -> out0 = M per image as split records [C/16][ceil(C/32)][3][64] x 16 B
 *   op 4 dwconv_gate    in0 = x (x1 at [0, hidS), x2 at [hidS, 2 hidS)), w0 [9][2 hidS], bias0 [2 hidS] (or null)
 *                       -> out0 (hidS); hidS % 4 == 0
 *   op 5 conv_lds       in0 (cin_pad), w0 = [ntiles][9 kt cin_pad/16] fragments (k = tap cin_pad + c), bias0
 *                       [16 ntiles] (or null), kt, relu, out_mode 0 / 1 (PixelUnshuffle) / 2 (PixelShuffle), nout;
 *                       use_wp3: also hand the kernel split records (kt 1: of w0; kt 3: of w1, the same weights
 *                       in k-group order c * 28 + tap, tap 27 zero) -> out0
 *   op 6 conv_small_out in0 (C = Cin, a multiple of 16), C2 = Cout <= 4, ks, w0 [Cout][Cin][ks][ks] (wt: the
 *                       transposed conv's [Cin][Cout][3][3]), bias0 (or null); out_nchw: out0 [Bn][Cout][F H W],
 *                       in1 = res of that shape (or null); else out0 NHWC (ldo0), R / ldr = NHWC residual (may be
 *                       out0), in2 = extra [Bn][F H W] copied into channel Cout (or null)
 *   op 7 conv3d_c16     in0 (16), w0 = [9 kt][64][4] fragments, bias0 [16], kt 1 / 3, relu -> out0 (16)
 *   op 8 maxpool2       in0 [Bn frames][H][W] (C) -> out0 [Bn][H/2][W/2] (C); C % 4 == 0
 *   op 9 gap + head     in0 [Bn][H W] (C), slots, scratch (Bn slots C floats), w0 [M][C], bias0 [M], w1 [N1][M],
 *                       bias1, w2 [N2][N1], bias2, w3 [N2], bias3 [1] -> out0 = score [Bn]
 *   op 10 attn_out_dw   in0 = v (C channels, ldi0 = its pixel stride, e.g. qkv + 2C with 3C), w0 = wdw [9][3C] and
 *                       bias0 = bdw [3C] (or null) of the whole qkv_dwconv (v's part at channel 2C), w1 = M per image
 *                       as attn_fold's split records, bias1 = project_out bias [C] (or null), R / ldr (may be out0),
 *                       zeros (>= 16 zero floats) -> out0 = R + bias1 + M dw3x3(v); C in {48, 96}, W % 16 == 0, every
 *                       view 16-byte aligned with ld % 4 == 0, out0 must not overlap in0 */
typedef struct kdlae_debug_infer_desc {
  int op;
  const float* in[3]; int ldi[3];
  const float* w[4];
  const float* bias[4];
  const float* R; int ldr;
  float* out[2]; int ldo[2];
  float* scratch; int64_t scratch_floats;
  const float* zeros;
  int C, C2, heads, Bn, F, H, W;
  int hidS, ln, nseg, seg_rows;
  int ntiles, cin_pad, kt, ks, relu, out_mode, nout, use_wp3;
  int out_nchw, wt, slots;
  int M, N1, N2;
} kdlae_debug_infer_desc;
int kdlae_debug_infer(const kdlae_debug_infer_desc* d, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* KDLAE_H_ */
