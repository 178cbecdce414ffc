// Flat parameter layouts and the per-model key enumerators (see param_layout.h).
#include "param_layout.h"

#include <algorithm>

#include "runtime.h"

namespace kdlae {

int ParamLayout::info(int i, const char** name, int64_t* n, int64_t* off) const {
  if (i < 0 || i >= size()) return fail(KDLAE_EPARAM, "param index out of range");
  if (name) *name = names[i].c_str();
  if (n) *n = numel[i];
  if (off) *off = offset[i];
  return KDLAE_OK;
}

int ParamStore::set(const char* name, const float* data, int64_t numel) {
  auto it = lay.index.find(name);
  if (it == lay.index.end()) return fail(KDLAE_EPARAM, std::string("unexpected key in state_dict: ") + name);
  if (lay.numel[it->second] != numel)
    return fail(KDLAE_EPARAM, std::string("size mismatch for ") + name + ": expected " +
                                  std::to_string(lay.numel[it->second]) + " got " + std::to_string(numel));
  staged[name].assign(data, data + numel);
  return KDLAE_OK;
}

int ParamStore::check_complete() const {
  for (auto& k : lay.names)
    if (!staged.count(k)) return fail(KDLAE_EPARAM, "missing state_dict entry: " + k);
  return KDLAE_OK;
}

int32_t ParamStore::base(const std::string& k, int* err) const {
  const int64_t off = lay.find(k);
  if (off < 0 && err && *err == KDLAE_OK) *err = fail(KDLAE_EPARAM, "missing state_dict entry: " + k);
  return (int32_t)off;
}

std::vector<float> ParamStore::flat() const {
  std::vector<float> v((size_t)lay.total, 0.f);
  for (int i = 0; i < lay.size(); ++i) {
    auto it = staged.find(lay.names[i]);
    if (it != staged.end()) std::copy(it->second.begin(), it->second.end(), v.begin() + lay.offset[i]);
  }
  return v;
}

// KDLAE_teacher (KDLAE_model.py:220-268, TransformerBlock :150-157, Attention :113-120,
// FeedForward :90-99, LayerNorm :73-79)
static void trunk_and_tail(const kdlae_t_config& c, bool tail, ParamLayout& out) {
  auto conv = [&](const std::string& n, int co, int ci, int k, bool b) {
    out.add(n + ".weight", (int64_t)co * ci * k * k);
    if (b) out.add(n + ".bias", co);
  };
  auto block = [&](const std::string& p, int dim, int heads) {
    const int hid = hid_of(c, dim);
    out.add(p + ".norm1.body.weight", dim);
    if (!c.layernorm_biasfree) out.add(p + ".norm1.body.bias", dim);
    out.add(p + ".attn.temperature", heads);
    conv(p + ".attn.qkv", 3 * dim, dim, 1, c.bias);
    conv(p + ".attn.qkv_dwconv", 3 * dim, 1, 3, c.bias);
    conv(p + ".attn.project_out", dim, dim, 1, c.bias);
    out.add(p + ".norm2.body.weight", dim);
    if (!c.layernorm_biasfree) out.add(p + ".norm2.body.bias", dim);
    conv(p + ".ffn.project_in", 2 * hid, dim, 1, c.bias);
    conv(p + ".ffn.dwconv", 2 * hid, 1, 3, c.bias);
    conv(p + ".ffn.project_out", dim, hid, 1, c.bias);
  };
  auto stage = [&](const std::string& n, int cnt, int dim, int heads) {
    for (int i = 0; i < cnt; ++i) block(n + "." + std::to_string(i), dim, heads);
  };
  const int d = c.dim, *nb = c.num_blocks, *hd = c.heads, nr = c.num_refinement_blocks;
  conv("patch_embed.proj", d, c.inp_channels, 3, false);
  stage("encoder_level1", nb[0], d, hd[0]);
  conv("down1_2.body.0", d / 2, d, 3, false);
  stage("encoder_level2", nb[1], 2 * d, hd[1]);
  conv("down2_3.body.0", d, 2 * d, 3, false);
  stage("encoder_level3", nb[2], 4 * d, hd[2]);
  conv("down3_4.body.0", 2 * d, 4 * d, 3, false);
  stage("latent", nb[3], 8 * d, hd[3]);
  conv("up4_3.body.0", 16 * d, 8 * d, 3, false);
  conv("reduce_chan_level3", 4 * d, 8 * d, 1, c.bias);
  stage("decoder_level3", nb[2], 4 * d, hd[2]);
  conv("up3_2.body.0", 8 * d, 4 * d, 3, false);
  conv("reduce_chan_level2", 2 * d, 4 * d, 1, c.bias);
  stage("decoder_level2", nb[1], 2 * d, hd[1]);
  conv("up2_1.body.0", 4 * d, 2 * d, 3, false);
  stage("decoder_level1", nb[0], 2 * d, hd[0]);
  stage("refinement", nr, 2 * d, hd[0]);
  conv("output", c.out_channels, 2 * d, 3, c.bias);
  if (!tail) return;
  conv("output_param", 2 * d, c.out_channels + 1, 3, c.bias);
  stage("refinement_out", nr, 2 * d, hd[0]);
  conv("output2", c.out_channels, 2 * d, 3, c.bias);
  if (c.static_train) {
    const int hc = 2 * d;
    conv("cen", hc, c.out_channels, 3, c.bias);
    conv("upen.body.0", 2 * hc, hc, 3, false);
    stage("enhance", nr, hc / 2, hd[0]);
    conv("outputen", c.out_channels, hc / 2, 3, c.bias);
  }
}

void teacher_keys(const kdlae_t_config& c, ParamLayout& out) { trunk_and_tail(c, true, out); }

// Restormer (Train/basicsr/models/archs/restormer_arch.py:471-546): the teacher's keys up to and including
// `output`; no output_param / refinement_out / output2 and no sr head (dual_pixel_task's skip_conv is refused)
void restormer_keys(const kdlae_t_config& c, ParamLayout& out) { trunk_and_tail(c, false, out); }

// KDLAE_student (KDLAE_model.py:359-384).  The reference registers encoders, pooling, st_fusion,
// upconv_layers, decoders, out_conv in that attribute order; state_dict() lists encoders.*, st_fusion.*,
// upconv_layers.*, decoders.*, out_conv.*
void student_keys(const kdlae_s_config& c, ParamLayout& out) {
  const int* hc = c.hidden_channels;
  const int L = c.num_hidden - 1;  // levels
  auto blk = [&](const std::string& p, int cin, int cout) {
    out.add(p + ".0.weight", (int64_t)cout * cin * 27);
    out.add(p + ".0.bias", cout);
    out.add(p + ".2.weight", (int64_t)cout * cout * 27);
    out.add(p + ".2.bias", cout);
  };
  int cin = c.inp_channels;
  for (int i = 0; i < L; ++i) {
    blk("encoders." + std::to_string(i), cin, hc[i]);
    cin = hc[i];
  }
  blk("st_fusion", cin, hc[L]);
  for (int j = 0, i = L - 1; i >= 0; --i, ++j) {
    out.add("upconv_layers." + std::to_string(j) + ".weight", (int64_t)hc[i + 1] * hc[i] * 4);
    out.add("upconv_layers." + std::to_string(j) + ".bias", hc[i]);
  }
  for (int j = 0, i = L - 1; i >= 0; --i, ++j) blk("decoders." + std::to_string(j), hc[i], hc[i]);
  out.add("out_conv.weight", (int64_t)c.out_channels * hc[0]);
  out.add("out_conv.bias", c.out_channels);
}

// DenoiseRatePredictor, registration order (ASDQE_model.py:127-156): three DoubleConv extractors, the
// UNet (inc, down1..3, up1..3, outc), the regressor (Linear 3 dim -> 256 -> 64 -> 1, :144-154)
int64_t asdqe_keys(const asdqe_config& c, bool buffers, ParamLayout& out) {
  int64_t nstat = 0;
  auto dc = [&](const std::string& p, int cin, int cout) {
    for (int i : {0, 3}) {
      out.add(p + "." + std::to_string(i) + ".weight", (int64_t)cout * (i == 0 ? cin : cout) * 9);
      out.add(p + "." + std::to_string(i) + ".bias", cout);
      const std::string bn = p + "." + std::to_string(i + 1) + ".";
      out.add(bn + "weight", cout);
      out.add(bn + "bias", cout);
      nstat += 2 * cout;
      if (!buffers) continue;
      out.add(bn + "running_mean", cout);
      out.add(bn + "running_var", cout);
      out.add(bn + "num_batches_tracked", 1);
    }
  };
  const int d = c.dim, m = 3 * d;
  for (const char* e : {"lq_extractor", "gt_extractor", "diff_extractor"})
    dc(std::string(e) + ".double_conv", c.in_channels, d);
  dc("unet.inc.double_conv", m, 64);
  dc("unet.down1.maxpool_conv.1.double_conv", 64, 128);
  dc("unet.down2.maxpool_conv.1.double_conv", 128, 256);
  dc("unet.down3.maxpool_conv.1.double_conv", 256, 256);
  dc("unet.up1.conv.double_conv", 512, 128);
  dc("unet.up2.conv.double_conv", 256, 64);
  dc("unet.up3.conv.double_conv", 128, 64);
  out.add("unet.outc.conv.weight", (int64_t)m * 64);
  out.add("unet.outc.conv.bias", m);
  out.add("regressor.2.weight", (int64_t)256 * m);
  out.add("regressor.2.bias", 256);
  out.add("regressor.5.weight", 256 * 64);
  out.add("regressor.5.bias", 64);
  out.add("regressor.8.weight", 64);
  out.add("regressor.8.bias", 1);
  return nstat;
}

}  // namespace kdlae
