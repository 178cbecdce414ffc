// The flat parameter layout of a model: its state_dict keys in order, each with its numel and its
// offset in the flat vector.  One key enumerator per model feeds both of the model's handles, so the
// inference handle and the training handle cannot disagree about a key.  Host code only.
#pragma once
#include <cstdint>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/kdlae.h"

namespace kdlae {

struct ParamLayout {
  // per-key alignment in floats: 1 = keys back to back (the inference handles' flat vector), 4 = every
  // key starts on a 16-byte boundary (the training handles' theta / grad buffers; pad floats stay zero,
  // so temperature [heads] and ffn.dwconv [2 hid * 9] do not break the float4 paths of the GEMMs)
  int64_t align;
  std::vector<std::string> names;
  std::vector<int64_t> numel, offset;
  std::unordered_map<std::string, int> index;
  int64_t total = 0;
  explicit ParamLayout(int64_t align_floats) : align(align_floats) {}
  int size() const { return (int)names.size(); }
  void add(const std::string& k, int64_t n) {
    index[k] = size();
    names.push_back(k);
    numel.push_back(n);
    offset.push_back(total);
    total += (n + align - 1) / align * align;
  }
  int64_t find(const std::string& k) const {  // flat offset of a key, -1 when the layout has no such key
    auto it = index.find(k);
    return it == index.end() ? -1 : offset[it->second];
  }
  int64_t at(const std::string& k) const { return offset[index.at(k)]; }  // throws on an unknown key
  int info(int i, const char** name, int64_t* numel, int64_t* offset) const;  // the *_param_info entry points
};

// expected state_dict keys (packed layout) + host copies staged through *_set_param
struct ParamStore {
  ParamLayout lay{1};
  std::unordered_map<std::string, std::vector<float>> staged;
  int set(const char* name, const float* data, int64_t numel);
  int check_complete() const;
  int32_t base(const std::string& k, int* err) const;  // flat offset of a key (-1 + err if unknown)
  std::vector<float> flat() const;                       // staged entries in key order
};

// hidden width of a TransformerBlock's FeedForward (KDLAE_model.py:90-92)
inline int hid_of(const kdlae_t_config& c, int dim) { return (int)((double)dim * c.ffn_expansion_factor); }

// The key enumerators: state_dict order of the reference modules.  KDLAE_teacher and KDLAE_student have
// no buffers, so state_dict() and named_parameters() list the same keys.
void teacher_keys(const kdlae_t_config& c, ParamLayout& out);
// plain Restormer: patch_embed ... refinement, output (the teacher's list without the rate tail and the sr head)
void restormer_keys(const kdlae_t_config& c, ParamLayout& out);
void student_keys(const kdlae_s_config& c, ParamLayout& out);
// DenoiseRatePredictor: with `buffers` the BatchNorm running_mean / running_var / num_batches_tracked
// entries are included (state_dict order, the inference handle); without, the parameters alone
// (named_parameters order, the training handle).  Returns the summed numel of the running_mean and
// running_var entries: the floats of the training handle's statistics buffer.
int64_t asdqe_keys(const asdqe_config& c, bool buffers, ParamLayout& out);

}  // namespace kdlae
