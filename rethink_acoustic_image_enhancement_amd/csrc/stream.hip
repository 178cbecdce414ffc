// Streaming inference for KDLAE-S (kdlae_stream_state_bytes, kdlae_stream_reset, kdlae_stream_push_u8,
// kdlae_stream_push_f32, kdlae_stream_advance): a device-resident ring of the last `frames` converted frames of B
// parallel sources, and the time-ordered stack the student's forward reads.  The kernels move bytes; the u8 push
// also converts by preprocess_u8_kernel's rule (pipeline.hip).
//
//   state               16 bytes of header (the push counter, a 64-bit integer, in the first 8) followed by the ring
//                       [B][F][H][W] fp32.  Frame number c of the stream lives in slot c % F.
//   stream_push_kernel  one thread per V consecutive pixels of a padded frame row.  With count = the counter's
//                       value and slot = count % F, the thread
//                         reads   ring slots slot + 1, slot + 2, ... (mod F): the F - 1 frames that stay, oldest first
//                         writes  stack positions 0 .. F - 2 with them, the new frame at position F - 1 and into
//                                 ring slot `slot`, which held the frame that drops out
//                       so within a launch the slots read and the slot written never meet, and a thread touches
//                       its own pixels only.  The counter is read from device memory: one captured graph of the
//                       launch serves every slot.
//   stream_advance_kernel  one thread: count = count + 1, stream-ordered after every launch that read it.
//
// V = 4 (float4 accesses of ring, stack and an fp32 frame) when those pointers sit on 16 bytes and W % 4 == 0, V = 1
// otherwise.  The u8 source is read one byte at a time, at any byte offset, except that a gray source on 4 bytes
// with w % 4 == 0 is read four pixels a load by the V = 4 threads left of the reflect padding.  Flat 64-bit item
// index with a grid-stride loop.  No atomics: the result is a function of the inputs alone.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "runtime.h"

namespace kdlae {

constexpr int kStreamHeader = 16;          // bytes in front of the ring: keeps it on 16 bytes when the state is
constexpr long long kStreamMaxBlocks = 4096;  // clip.hip's cap; the loop takes the rest

// B sources, a ring of F frames of H rows of W floats; the u8 source has h rows of w pixels of cin bytes and src4
// says that it may be read four gray pixels a load
struct StreamGeo {
  int B, F, H, W, h, w, cin, src4;
};

namespace {

// pipeline.hip's two rules, restated: torch's reflect index for a pad shorter than the input, and cv2's 8-bit
// COLOR_BGR2GRAY, Y = (1868 B + 9617 G + 4899 R + 2^13) >> 14
__device__ __forceinline__ int stream_reflect(int i, int n) { return i < n ? i : 2 * (n - 1) - i; }
__device__ __forceinline__ uint8_t stream_gray(const uint8_t* px, int cin) {
  return cin >= 3 ? (uint8_t)((1868u * px[0] + 9617u * px[1] + 4899u * px[2] + 8192u) >> 14) : px[0];
}

template <int V, bool U8>
__global__ __launch_bounds__(256) void stream_push_kernel(const void* __restrict__ frame,
                                                          const unsigned long long* __restrict__ count,
                                                          float* __restrict__ ring, float* __restrict__ stack,
                                                          StreamGeo g, long long total) {
  const int slot = (int)(*count % (unsigned long long)g.F);
  const int wq = g.W / V;
  const long long HW = (long long)g.H * g.W;
  for (long long idx = blockIdx.x * 256LL + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
    const long long row = idx / wq;  // over B H
    const int x = (int)(idx - row * wq) * V;
    const int y = (int)(row % g.H), b = (int)(row / g.H);
    float v[V];
    if constexpr (U8) {
      const uint8_t* src = static_cast<const uint8_t*>(frame);
      const long long line = ((long long)b * g.h + stream_reflect(y, g.h)) * g.w;
      bool loaded = false;
      if constexpr (V == 4) {
        if (g.src4 && x < g.w) {  // w % 4 == 0: the four pixels lie left of the padding
          const uchar4 q = *reinterpret_cast<const uchar4*>(src + line + x);
          v[0] = (float)q.x / 255.0f, v[1] = (float)q.y / 255.0f, v[2] = (float)q.z / 255.0f, v[3] = (float)q.w / 255.0f;
          loaded = true;
        }
      }
      if (!loaded) {
#pragma unroll
        for (int e = 0; e < V; ++e)
          v[e] = (float)stream_gray(src + (line + stream_reflect(x + e, g.w)) * g.cin, g.cin) / 255.0f;
      }
    } else {
      const float* src = static_cast<const float*>(frame) + (long long)b * HW + (long long)y * g.W + x;
      if constexpr (V == 4) {
        const float4 q = *reinterpret_cast<const float4*>(src);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
      } else {
        v[0] = *src;
      }
    }
    const long long at = (long long)b * g.F * HW + (long long)y * g.W + x;  // this thread's pixels in frame 0 of b
    int s = slot;
    for (int p = 0; p < g.F - 1; ++p) {
      s = s + 1 == g.F ? 0 : s + 1;
      if constexpr (V == 4)
        *reinterpret_cast<float4*>(stack + at + p * HW) = *reinterpret_cast<const float4*>(ring + at + s * HW);
      else
        stack[at + p * HW] = ring[at + s * HW];
    }
    if constexpr (V == 4) {
      const float4 q = make_float4(v[0], v[1], v[2], v[3]);
      *reinterpret_cast<float4*>(stack + at + (g.F - 1) * HW) = q;
      *reinterpret_cast<float4*>(ring + at + slot * HW) = q;
    } else {
      stack[at + (g.F - 1) * HW] = v[0];
      ring[at + slot * HW] = v[0];
    }
  }
}

__global__ void stream_advance_kernel(unsigned long long* count) { *count = *count + 1; }

template <bool U8>
int launch_stream_push(const char* who, const void* frame, const StreamGeo& g, void* state, float* stack, bool vec,
                       void* stream) {
  const auto* count = static_cast<const unsigned long long*>(state);
  float* ring = reinterpret_cast<float*>(static_cast<char*>(state) + kStreamHeader);
  const long long total = (long long)g.B * g.H * (g.W / (vec ? 4 : 1));
  const dim3 grid((unsigned)std::min(ceil_div(total, 256), kStreamMaxBlocks)), block(256);
  const hipStream_t st = (hipStream_t)stream;
  if (vec)
    hipLaunchKernelGGL((stream_push_kernel<4, U8>), grid, block, 0, st, frame, count, ring, stack, g, total);
  else
    hipLaunchKernelGGL((stream_push_kernel<1, U8>), grid, block, 0, st, frame, count, ring, stack, g, total);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(KDLAE_EHIP, std::string(who) + ": " + hipGetErrorString(e));
  return KDLAE_OK;
}

// the checks every entry with a ring shares: sizes and the index ranges the kernel keeps in an int
int check_stream(const char* who, int B, int frames, int H, int W) {
  const std::string w(who);
  if (B < 1 || frames < 1 || H < 1 || W < 1) return fail(KDLAE_EINVAL_CONFIG, w + ": need B, frames, H and W >= 1");
  if ((long long)B * H > INT_MAX || (long long)H * W > INT_MAX)
    return fail(KDLAE_EINVAL_SHAPE, w + ": more than 2^31 - 1 rows of all frames or pixels of a frame");
  return KDLAE_OK;
}

}  // namespace

}  // namespace kdlae

using namespace kdlae;

extern "C" int64_t kdlae_stream_state_bytes(int B, int frames, int H, int W) {
  if (check_stream("kdlae_stream_state_bytes", B, frames, H, W) != KDLAE_OK) return -1;
  return kStreamHeader + (int64_t)B * frames * H * W * 4;
}

extern "C" int kdlae_stream_reset(void* state, void* stream) {
  if (!state) return fail(KDLAE_EINVAL_CONFIG, "kdlae_stream_reset: null argument");
  if (((uintptr_t)state & 7) != 0) return fail(KDLAE_EINVAL_SHAPE, "kdlae_stream_reset: state must sit on 8 bytes");
  HIPCHK(zero_fill(state, kStreamHeader, (hipStream_t)stream));
  return KDLAE_OK;
}

extern "C" int kdlae_stream_push_u8(const uint8_t* frame, int B, int h, int w, int channels, int multiple, int frames,
                                    void* state, float* stack, void* stream) {
  const char* who = "kdlae_stream_push_u8";
  if (!frame || !state || !stack) return fail(KDLAE_EINVAL_CONFIG, "kdlae_stream_push_u8: null argument");
  if (B < 1 || h < 1 || w < 1 || frames < 1 || multiple < 1)
    return fail(KDLAE_EINVAL_CONFIG, "kdlae_stream_push_u8: need B, h, w, frames and multiple >= 1");
  if (channels != 1 && channels != 3 && channels != 4)
    return fail(KDLAE_EINVAL_CONFIG, "kdlae_stream_push_u8: channels must be 1, 3 or 4");
  if ((long long)h + multiple > INT_MAX || (long long)w + multiple > INT_MAX)
    return fail(KDLAE_EINVAL_SHAPE, "kdlae_stream_push_u8: the padded size passes 2^31 - 1");
  int H, W;
  kdlae_padded_size(h, w, multiple, &H, &W);
  if (H - h >= h || W - w >= w)
    return fail(KDLAE_EINVAL_SHAPE, "kdlae_stream_push_u8: frame smaller than its reflect padding");
  TRY(check_stream(who, B, frames, H, W));
  if (((uintptr_t)state & 7) != 0 || ((uintptr_t)stack & 3) != 0)
    return fail(KDLAE_EINVAL_SHAPE, "kdlae_stream_push_u8: state must sit on 8 bytes and stack on 4");
  const bool vec = al16(state) && al16(stack) && W % 4 == 0;
  const int src4 = vec && channels == 1 && ((uintptr_t)frame & 3) == 0 && w % 4 == 0;
  const StreamGeo g{B, frames, H, W, h, w, channels, src4};
  return launch_stream_push<true>(who, frame, g, state, stack, vec, stream);
}

extern "C" int kdlae_stream_push_f32(const float* frame, int B, int H, int W, int frames, void* state, float* stack,
                                     void* stream) {
  const char* who = "kdlae_stream_push_f32";
  if (!frame || !state || !stack) return fail(KDLAE_EINVAL_CONFIG, "kdlae_stream_push_f32: null argument");
  TRY(check_stream(who, B, frames, H, W));
  if (((uintptr_t)state & 7) != 0 || ((uintptr_t)stack & 3) != 0 || ((uintptr_t)frame & 3) != 0)
    return fail(KDLAE_EINVAL_SHAPE, "kdlae_stream_push_f32: state must sit on 8 bytes, frame and stack on 4");
  const bool vec = al16(frame) && al16(state) && al16(stack) && W % 4 == 0;
  const StreamGeo g{B, frames, H, W, H, W, 1, 0};
  return launch_stream_push<false>(who, frame, g, state, stack, vec, stream);
}

extern "C" int kdlae_stream_advance(void* state, void* stream) {
  if (!state) return fail(KDLAE_EINVAL_CONFIG, "kdlae_stream_advance: null argument");
  if (((uintptr_t)state & 7) != 0) return fail(KDLAE_EINVAL_SHAPE, "kdlae_stream_advance: state must sit on 8 bytes");
  hipLaunchKernelGGL(stream_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream,
                     static_cast<unsigned long long*>(state));
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(KDLAE_EHIP, std::string("kdlae_stream_advance: ") + hipGetErrorString(e));
  return KDLAE_OK;
}
