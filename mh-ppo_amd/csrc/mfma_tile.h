// mfma_tile.h — the f32-MFMA tile primitives of the forward-only nets (device): the one copy that
// the rollout's actor tile (rollout_policy.h, namespace pol) and the batched head forward
// (mlp_infer_tile.h, namespace infer) both use, so the two stay bit-identical by construction.
//
// The layout: rows on the lanes (lane j of both halves = tile row j), v_mfma_f32_32x32x2_f32 with
// the weights as the A operand and the inputs as B.  C register r of lane half kh holds tile row
// i = (r & 3) + 8 (r >> 2) + 4 kh of the layer's output, and the weight rows are staged in LDS
// permuted so that this row is neuron 2 r + kh, i.e. row i carries neuron
// 2 ((i & 3) + 4 (i >> 3)) + ((i >> 2) & 1); row_of_neuron is the inverse.  k-step s of the next
// layer then consumes inputs 2 s, 2 s + 1 straight from register s: every chain runs in ascending
// input order.
#pragma once
#include <hip/hip_runtime.h>

#include "rollout_dev.h"  // relu

namespace mhppo {
namespace mfma_tile {

typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int S2 = 33, S3 = 65;  // odd LDS row strides of W2 / W3: conflict-free operand reads

__device__ __forceinline__ f32x16 mfma(float a, float b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x16 zero16() {
  f32x16 z;
#pragma unroll
  for (int i = 0; i < 16; i++) z[i] = 0.0f;
  return z;
}
// v[r] = relu(v[r] + b[row(r)]) with the oracle's relu (x < 0 ? 0 : x)
__device__ __forceinline__ void bias_relu(f32x16 &v, const float *b, int kh) {
  const float4 *b4 = reinterpret_cast<const float4 *>(b);
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const float4 c = b4[2 * q + kh];
    v[4 * q + 0] = relu(v[4 * q + 0] + c.x);
    v[4 * q + 1] = relu(v[4 * q + 1] + c.y);
    v[4 * q + 2] = relu(v[4 * q + 2] + c.z);
    v[4 * q + 3] = relu(v[4 * q + 3] + c.w);
  }
}
// LDS row holding neuron n (0..31) in the permuted staging above
__device__ __forceinline__ int row_of_neuron(int n) {
  const int m = n >> 1;
  return (m & 3) + 8 * (m >> 2) + 4 * (n & 1);
}

}  // namespace mfma_tile
}  // namespace mhppo
