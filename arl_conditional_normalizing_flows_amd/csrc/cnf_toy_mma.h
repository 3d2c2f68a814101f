// cnf_toy_mma.h — the fp32 matrix-core tile the toy flow's kernels share (k_toy_bwd in cnf_toy_train.hip,
// k_toy_sample in cnf_toy_sample.hip): one definition, so the two agree on the operand maps and the k order.
#pragma once

#include <hip/hip_runtime.h>

namespace cnf {

typedef float v4f __attribute__((ext_vector_type(4)));

// one 16x16 output tile of v_mfma_f32_16x16x4_f32 over K (a multiple of 4 after padding): lane l
// supplies A[row l & 15][k = k0 + (l >> 4)] and B[k][col l & 15]; it receives
// C[row 4 (l >> 4) + r][col l & 15] in element r. fa / fb return 0 outside the operand.
template <class FA, class FB>
__device__ __forceinline__ v4f mma_tile(int K, FA fa, FB fb, v4f acc) {
    const int lane = threadIdx.x & 63;
    const int rc = lane & 15, kq = lane >> 4;
    for (int k0 = 0; k0 < K; k0 += 4) {
        const float av = fa(rc, k0 + kq);
        const float bv = fb(k0 + kq, rc);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
    }
    return acc;
}

}  // namespace cnf
