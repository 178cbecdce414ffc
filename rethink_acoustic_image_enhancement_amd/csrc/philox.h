// Philox4x32-10 (Random123), the one generator of the batch-preparation (augment.hip) and dataset-sample
// (data.hip) kernels: key = (seed lo, seed hi), counter = (block lo, block hi, call lo, call hi).
#pragma once
#include <hip/hip_runtime.h>

namespace kdlae {

__device__ __forceinline__ uint4 philox4x32_10(uint4 c, unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
    c = make_uint4(hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c;
}

}  // namespace kdlae
