// cnf_toy_device.h — what the toy flow's kernels share on the device (k_toy in cnf_toy.hip, k_toy_bwd in
// cnf_toy_train.hip, k_toy_sample in cnf_toy_sample.hip, k_toy_density in cnf_toy_density.hip): the coupling masks, LeakyReLU and the fp32
// matrix-core tile. One definition each, so the kernels agree on the index sets, the operand maps and the k order.
#pragma once

#include <hip/hip_runtime.h>

#include "cnf_kernels.h"

namespace cnf {

// the reference graph's LeakyReLU as a select (cnf_device.h's lrelu is a v_max: other bits for a NaN)
__device__ __forceinline__ float toy_lrelu(float x) { return x >= 0.f ? x : LRELU_ALPHA * x; }

// u1 / u2 index sets of coupling network j's mask, one of six types t (:149-163): the nets read the n1
// components i1 and write the n2 = 3 - n1 components i2 (an unused second entry is 0). A kernel that
// indexes the sets by a run-time k copies them into arrays of its own: the struct indexed so lives in scratch
struct ToyMask {
    int n1, n2, i1[2], i2[2];
};
__device__ __forceinline__ ToyMask toy_mask(int j) {
    const int t = j % 6;
    ToyMask m;
    if (t < 3) {
        m.n1 = 1;
        m.n2 = 2;
        m.i1[0] = t;
        m.i1[1] = 0;
        m.i2[0] = t == 0 ? 1 : 0;
        m.i2[1] = t == 2 ? 1 : 2;
    } else {
        m.n1 = 2;
        m.n2 = 1;
        m.i1[0] = t == 5 ? 1 : 0;
        m.i1[1] = t == 3 ? 1 : 2;
        m.i2[0] = 5 - t;   // t=3 -> 2, t=4 -> 1, t=5 -> 0
        m.i2[1] = 0;
    }
    return m;
}

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
