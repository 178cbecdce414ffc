// Shared host runtime (see runtime.h).
#include "runtime.h"

#include <cstdio>
#include <cstdlib>
#include <map>
#include <mutex>
#include <tuple>

namespace kdlae {

thread_local std::string g_err;
int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

template <typename T>
__global__ void zero_fill_kernel(T* p, long long n) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    p[i] = T{};
}

hipError_t zero_fill(void* p, size_t bytes, hipStream_t stream) {
  if (bytes == 0) return hipSuccess;
  if (!p || ((uintptr_t)p & 3) || (bytes & 3)) return hipErrorInvalidValue;
  const bool vec = !((uintptr_t)p & 15) && !(bytes & 15);
  const long long n = (long long)(bytes / (vec ? 16 : 4));
  const unsigned blocks = (unsigned)std::min<long long>((n + 255) / 256, 4096);
  if (vec) hipLaunchKernelGGL(zero_fill_kernel<uint4>, dim3(blocks), dim3(256), 0, stream, static_cast<uint4*>(p), n);
  else hipLaunchKernelGGL(zero_fill_kernel<uint32_t>, dim3(blocks), dim3(256), 0, stream, static_cast<uint32_t*>(p), n);
  return hipGetLastError();
}

bool debug_flag(const char* name) {
  const char* e = getenv("KDLAE_DEBUG");
  if (!e) return false;
  const std::string s(e), n(name);
  size_t i = 0;
  while (i <= s.size()) {
    size_t j = s.find(',', i);
    if (j == std::string::npos) j = s.size();
    if (s.compare(i, j - i, n) == 0 && j - i == n.size()) return true;
    i = j + 1;
  }
  return false;
}

// Tile-shape selection.  Resident schedule when a variant with KG == kgroups exists: the weights
// are split into groups that fit the LDS budget (one group per grid.y), and NT (accumulator tiles
// per pass) minimises padding inside a group.  Otherwise the chunked schedule over (NT, KG).
// Weights sit in LDS in split fragment order (mfma3.h): 3 KiB per output tile and k-group pair.
static constexpr int kLdsBudgetKB = 152;
static long long tile_lds_bytes(int kgroups) { return (long long)((kgroups + 1) / 2) * 3072 + 64; }

void choose_variant(Gemm& g, bool /*prefer_single_k*/) {
  static const int nts[] = {1, 2, 3, 4, 6, 8, 9, 12};
  static const int kgs[] = {2, 3, 4, 6, 8, 9, 12, 16};  // (12 x 8 and wider only on the r01 chunked kernel)
  g.group_tiles = 0;
  g.WPE = 2;
  if (g.ksize == 1) {
    int best_nt = 0, best_w = 2;
    double best = 1e30;
// r05: weigh one or two more weight groups than the LDS budget needs, counting every computed tile
// (the last group's padding too).  A/B (profiles/r05zx_gemm_groups_ab.txt): C192 qkv (36 tiles) as
// 6 groups of 6 instead of 5 of 8 (the last half empty): 588 -> 382 us per launch at 16 x 128^2.
constexpr auto KDLAE_GEMM_GROUPS_ALT = 1;
    int best_groups = 0;
    for (int w : {2}) {
      // two resident blocks per CU at 4 waves/SIMD -> half the LDS budget each
      const int budget_kb = w == 4 ? 76 : kLdsBudgetKB;
      const int budget = (int)std::max<long long>(1, budget_kb * 1024LL / tile_lds_bytes(g.kgroups));
      const int ngroups0 = (int)ceil_div(g.ntiles, budget);
      for (int ngroups = ngroups0; ngroups <= ngroups0 + (KDLAE_GEMM_GROUPS_ALT ? 2 : 0); ++ngroups) {
      const int gt = (int)ceil_div(g.ntiles, ngroups);
      if (ngroups > ngroups0 && (int)ceil_div(g.ntiles, gt) != ngroups) continue;
      for (int nt : nts) {
        if (!gemm_has_variant(nt, g.kgroups, false, w, true, g.out_mode)) continue;
        const long long padded = ceil_div(gt, nt) * nt;
        // split weights + the group's bias (64 B per tile) must fit 160 KiB
        if (padded * tile_lds_bytes(g.kgroups) > (w == 4 ? 80 : 158) * 1024LL) continue;
        // default policy: 2 waves/SIMD.  4 waves/SIMD used to win on the store-heavy K <= 48 shapes
        // while every epilogue load drained the stores; with that fixed, 2 waves measure 10-15%
        // faster on all of them (r01 probe: C48 project_in @1024^2 5864 -> 5099 us)
        double cost = (double)padded / gt + 0.01 * (12 - nt) + (ngroups - 1) * 0.05;
        // an odd NT leaves each k-group's last tile alone with 2 independent accumulator chains:
        // C96 qkv (18 tiles) measured 2% faster as 3 chunks of 6 than as 2 chunks of 9 on two boxes
        // (profiles/r02_gemm_odd_nt_probe.txt); riding that tile along with the first pair instead
        // measured no gain
        if (nt % 2) cost += 0.05;
        if (KDLAE_GEMM_GROUPS_ALT) {
          // (with an odd-NT penalty of 0.10 the C96 qkv took 3 groups of 6 and lost 2-8%)
          const double computed = (double)ngroups * padded / g.ntiles;
          cost = computed * (1.0 + 0.05 * (ngroups - 1)) + 0.01 * (12 - nt) + ((nt % 2) ? 0.05 : 0.0);
        }
        if (cost < best) {
          best = cost;
          best_nt = nt;
          best_w = w;
          best_groups = ngroups;
        }
      }
      }
    }
    if (best_nt) {
      g.NT = best_nt;
      g.KG = g.kgroups;
      g.WPE = best_w;
      g.group_tiles = (int)ceil_div(g.ntiles, best_groups);
      return;
    }
  }
  double best = 1e30;
  for (int nt : nts)
    for (int kg : kgs) {
      if (!gemm_has_variant2(nt, kg, g.ksize == 3, g.out_mode) || (g.has_res && nt * kg >= 36)) continue;
      const long long nch = ceil_div(g.ntiles, nt), kch = ceil_div(g.kgroups, kg);
      if (kch > 1 && kg % 2) continue;  // split pairs may not straddle k-chunks (mfma3.h)
      const double waste = (double)(nch * nt) * (kch * kg) / ((double)g.ntiles * g.kgroups);
      // every k-chunk restages weights behind two barriers; every n-chunk re-reads A.
      // 1x1 (r01 v15 probe): n-chunks cost more than k-chunks; with penalties 0.06 / 0.02 the
      // K = 510/1021 FFN project_out and the C384 GEMMs take 12x8 chunks (72 -> 85 and 76 -> 90 TF/s)
      // 3x3 (r01 probe): an n-chunk re-gathers the whole im2col A (12x3 beat 6x12 at N = 384, 768);
      // with 12-tile chunks, halving the k-chunks (12x6) saved 2%; with 3-tile chunks 3x6 lost 12%
constexpr auto KDLAE_NPEN_1X1 = 0.06;
constexpr auto KDLAE_NPEN_3X3 = 0.12;
      const double npen = g.ksize == 3 ? KDLAE_NPEN_3X3 : KDLAE_NPEN_1X1;
constexpr auto KDLAE_KPEN_1X1 = 0.02;
      const double kpen = g.ksize == 3 ? (nt >= 12 ? 0.01 : 0.0) : KDLAE_KPEN_1X1;
      double cost = waste * (1.0 + npen * (nch - 1) + kpen * (kch - 1));
      if (cost < best - 1e-9) {
        best = cost;
        g.NT = nt;
        g.KG = kg;
      }
    }
}


int run_gemm(const GemmCall& c, hipStream_t s) {
  const Gemm& g = *c.g;
  const long long HW = (long long)c.F * c.H * c.Wd;
  const int ldmax = std::max({c.in.ld, c.out.ld, c.ldr, c.out1.ld});
  if (HW * ldmax * (c.out_mode == 2 ? 4 : 1) >= (1LL << 31))
    return fail(KDLAE_EINVAL_SHAPE, "image too large for 32-bit in-image offsets");
  GemmParams p{};
  p.A = c.in.p;
  p.lda = c.in.ld;
  p.cg_per_tap = g.cg_per_tap;
  p.kgroups = g.kgroups;
  p.ksize = g.ksize;
  p.dil = 1;
  p.Wp = c.W;
  p.w_img_stride = c.w_img_stride;
  p.ntiles = g.ntiles;
  p.N = g.N;
  p.bias = c.bias;
  p.out = c.out.p;
  p.ldo = c.out.ld;
  p.R = c.R;
  p.ldr = c.ldr;
  p.ln = c.ln;
  p.ln_C = c.ln_C;
  p.relu = c.relu;
  p.Bn = c.B;
  p.H = c.H;
  p.W = c.Wd;
  p.F = c.F;
  p.kt = g.kt;
  p.out_mode = c.out_mode;
  p.tiles_per_img = (int)ceil_div(HW, kGemmRows);
  p.total_tiles = c.B * p.tiles_per_img;
  p.kchunks = g.group_tiles ? 1 : (int)ceil_div(g.kgroups, g.KG);
  p.group_tiles = g.group_tiles;
  p.Wm = c.Wm;
  p.wm_img_stride = c.wm_img_stride;
  p.bias_m = c.bias_m;
  p.out1 = c.out1.p;
  p.ldo1 = c.out1.ld;
  p.stats = nullptr;
  if (c.ln && (p.kchunks > 1 || g.kgroups * 16 != c.ln_C)) {
    if (!c.stats_buf) return fail(KDLAE_ESTATE, "LN GEMM needs a stats buffer");
    HIPCHK(launch_ln_stats(c.in.p, c.in.ld, c.ln_C, (long long)c.B * HW, c.stats_buf, s));
    p.stats = c.stats_buf;
  }
  const int gy = g.group_tiles ? (int)ceil_div(g.ntiles, g.group_tiles) : (int)ceil_div(g.ntiles, g.NT);
  p.tiles_per_block = gemm_tiles_per_block(p.total_tiles, gy, g.group_tiles != 0, g.WPE);
  const int gx = (int)ceil_div(p.total_tiles, p.tiles_per_block);
  HIPCHK(launch_gemm(p, g.NT, g.KG, g.WPE, gx, s));
  return KDLAE_OK;
}

// Which kernel a conv / GEMM layer runs on.  One rule for the three models, merged from the `conv`
// lambdas of kdlae_s_forward and asdqe_forward and the lds_conv branch of KDLAE-T's Fwd::gemm:
//   c16   3x3(x3) conv 16 -> 16 channels with a plain store (kgroups = 9 kt, one tile): KDLAE-S kt = 3,
//         ASDQE kt = 1.  KDLAE-T's 3x3 convs all store through a (un)shuffle map, so none qualifies,
//         dim = 16 (Downsample 16 -> 8) included.
//   lds   any other 3x3(x3) conv that conv_lds.hip supports, without residual or LN: the plain store of
//         KDLAE-S (kt = 3, tap-pair split records w3t) and ASDQE (kt = 1, w3), and KDLAE-T's Downsample
//         (out_mode 1) and Upsample (out_mode 2) convs (w3, outputs n < n_true only).
//   gemm  everything else: every 1x1, and 3x3 shapes outside conv_lds_supported.
constexpr auto KDLAE_T_DOWN_LDS = 1;  // Downsample convs on conv_lds (0: the implicit GEMM)
constexpr auto KDLAE_T_UP_LDS = 1;  // Upsample convs on conv_lds (0: the implicit GEMM)
ConvKernel conv_kernel(const Gemm& g, const GemmCall& c) {
  if (g.ksize != 3 || c.R || c.ln) return ConvKernel::gemm;
  if (c.out_mode == 0 && g.ntiles == 1 && g.cg_per_tap == 1 && g.kgroups == 9 * g.kt) return ConvKernel::c16;
  const bool mode_ok = c.out_mode == 0 || (KDLAE_T_DOWN_LDS && c.out_mode == 1) || (KDLAE_T_UP_LDS && c.out_mode == 2);
  return mode_ok && conv_lds_supported(g.kt, g.ntiles, g.cg_per_tap * 16) ? ConvKernel::lds : ConvKernel::gemm;
}

int run_conv(const DeviceWeights& D, const Gemm& g, GemmCall c, hipStream_t s) {
  c.g = &g;
  c.bias = D.P(g.bias);
  if (!c.W) c.W = D.P3(g.w3);
  switch (conv_kernel(g, c)) {
    case ConvKernel::c16: {  // LDS-tiled kernel with the weights held in VGPRs (conv3d_c16.hip)
      Conv3dC16Params q{};
      q.in = c.in.p;
      q.ldi = c.in.ld;
      q.wp = D.P(g.w);
      q.bias = c.bias;
      q.out = c.out.p;
      q.ldo = c.out.ld;
      q.Bn = c.B;
      q.F = c.F;
      q.H = c.H;
      q.W = c.Wd;
      q.relu = c.relu;
      q.kt = g.kt;
      HIPCHK(launch_conv3d_c16(q, s));
      return KDLAE_OK;
    }
    case ConvKernel::lds: {  // LDS-tiled implicit GEMM (conv_lds.hip): halo staged once, no per-tap L1 re-reads
      ConvLdsParams q{};
      q.in = c.in.p;
      q.ldi = c.in.ld;
      q.cin_pad = g.cg_per_tap * 16;
      q.wp = D.P(g.w);
      q.wp3 = g.kt == 3 ? D.P3(g.w3t) : c.W;
      q.ntiles = g.ntiles;
      q.kgroups = g.kgroups;
      q.bias = c.bias;
      q.out = c.out.p;
      q.ldo = c.out.ld;
      q.Bn = c.B;
      q.F = c.F;
      q.H = c.H;
      q.W = c.Wd;
      q.kt = g.kt;
      q.relu = c.relu;
      q.out_mode = c.out_mode;
      q.nout = c.out_mode ? g.n_true : 0;
      HIPCHK(launch_conv_lds(q, s));
      return KDLAE_OK;
    }
    case ConvKernel::gemm: break;
  }
  return run_gemm(c, s);
}

// ----------------------------------------------------------------------------- handle lifecycle
int handle_param_info(const HandleBase* h, int index, const char** name, int64_t* numel) {
  if (!h) return fail(KDLAE_ESTATE, "null handle");
  return h->ps.lay.info(index, name, numel, nullptr);
}

int handle_set_param(HandleBase* h, const char* name, const float* host_data, int64_t numel) {
  if (!h || !name || !host_data) return fail(KDLAE_ESTATE, "null argument");
  return h->ps.set(name, host_data, numel);
}

int handle_prepare(HandleBase* h, RecordFn record) {
  if (!h) return fail(KDLAE_ESTATE, "null handle");
  if (h->built) return KDLAE_OK;
  PackProgram prog;
  prog.nsrc = h->ps.lay.total;
  TRY(record(h, prog));
  DeviceGuard g(h->device);
  TRY(h->dw.upload_program(prog));
  h->built = true;
  return KDLAE_OK;
}

int handle_commit(HandleBase* h, RecordFn record, void* stream) {
  if (!h) return fail(KDLAE_ESTATE, "null handle");
  TRY(h->ps.check_complete());
  TRY(handle_prepare(h, record));
  DeviceGuard g(h->device);
  TRY(h->dw.run_host(h->ps.flat(), reinterpret_cast<hipStream_t>(stream)));
  h->committed = true;
  return KDLAE_OK;
}

int handle_pack_device(HandleBase* h, RecordFn record, const float* params, int64_t numel, void* stream) {
  if (!h) return fail(KDLAE_ESTATE, "null handle");
  if (numel != h->ps.lay.total)
    return fail(KDLAE_EPARAM, "flat parameter vector has " + std::to_string(numel) + " floats, expected " +
                                  std::to_string(h->ps.lay.total));
  TRY(handle_prepare(h, record));  // no-op after *_prepare
  DeviceGuard g(h->device);
  TRY(h->dw.run(params, reinterpret_cast<hipStream_t>(stream)));
  h->committed = true;
  return KDLAE_OK;
}

void handle_release(HandleBase* h) {
  DeviceGuard g(h->device);
  h->dw.release();
}

int device_cu_count() {
  static std::mutex mu;
  static std::map<int, int> per_device;  // a process may drive several GPUs (nn.DataParallel-style)
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 256;
  std::lock_guard<std::mutex> lock(mu);
  auto it = per_device.find(dev);
  if (it != per_device.end()) return it->second;
  int v = 0;
  if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256;
  per_device[dev] = v;
  return v;
}

// Tiles per block for a GEMM grid of ceil(T / tpb) x gy equal-work blocks.  One 8-wave block fills
// a CU at 2 waves/SIMD (two at 4), so the launch runs in ceil(blocks / slots) rounds and its
// makespan is rounds x tpb tile-times.  The old "about 512 blocks" rule could land a handful of
// blocks past a round (C192 project_in: 516 blocks = 3 rounds of 12 tiles for 24 tiles of work per
// CU).  Resident blocks also restage their weight group once (about half a tile-time, from L2).
int gemm_tiles_per_block(int total_tiles, int gy, bool resident, int wpe) {
  thread_local std::map<std::tuple<int, int, bool, int, int>, int> memo;  // a forward repeats ~30 shapes
  const int cus = device_cu_count();
  const auto key = std::make_tuple(total_tiles, gy, resident, wpe, cus);
  auto it = memo.find(key);
  if (it != memo.end()) return it->second;
  const long long slots = (long long)cus * (wpe == 4 ? 2 : 1);
  const int target = resident ? 256 * wpe : 1024;  // previous heuristic: the tie-break
  const int gx0 = (int)std::min<long long>(total_tiles, std::max<long long>(1, ceil_div(target, gy)));
  int best = (int)ceil_div(total_tiles, gx0);
  auto cost = [&](int tpb) {
    const long long blocks = ceil_div(total_tiles, tpb) * gy;
    const long long rounds = ceil_div(blocks, slots);
    return (double)rounds * (tpb + (resident ? 0.5 : 0.0));
  };
  double best_cost = cost(best);
  for (int tpb = 1; tpb <= total_tiles; ++tpb) {
    const double c = cost(tpb);
    if (c < best_cost * 0.98) {
      best_cost = c;
      best = tpb;
    }
  }
  memo[key] = best;
  return best;
}

}  // namespace kdlae
