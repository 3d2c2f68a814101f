// cnf_sample.hip — conditional sampling around the inverse (cnf_flow_sample, include/cnf.h): the recipe of
// TOYcINN.py:807-817 (z from the prior, concat the condition y, the model in the generative direction,
// conv_cINN_make_model.py:1774-1798) with its post-transforms and the statistics over the draws.
//   k_latent       one chunk of zy: temperature * N(0,1) on the x channels, y[b] on the rest
//   k_sample_fold  one pass over a chunk's xy_hat: post-transform, samples, running (K, S1, S2), mean / std
//   k_sample_ydev  per image sum |y_hat - y|
//   k_sample_logp  per image log-density of the draw: the prior's log N(z; 0, I) plus the inverse's log-det slots
// All HBM-bound element / reduction kernels; no atomics, every sum in a fixed order.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "cnf_device.h"

namespace cnf {

namespace {

// VEC (D % 4 == 0): one thread per channel quad of a pixel, one 16-byte store; otherwise one thread per
// element. The normal is instance_noise_value's (renew_noise form) of stream element
// offset + (g * HW + p) * x_d + c: what k_noise writes into a [B][S][HW][x_d] tensor.
template <bool VEC>
__global__ __launch_bounds__(256) void k_latent(SampleChunk q, const float* __restrict__ y, float* __restrict__ zy,
                                                float temperature, uint64_t seed, uint64_t offset) {
    constexpr int V = VEC ? 4 : 1;
    const int units = q.D / V, yd = q.D - q.x_d;   // per pixel
    const long long n = (long long)q.n * q.HW * units;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
        const int cu = (int)(e % units);
        const long long ip = e / units;   // (image of the chunk, pixel)
        const int p = (int)(ip % q.HW);
        const long long g = q.g0 + ip / q.HW;
        const long long b = g / q.S;
        const float* __restrict__ yp = y + ((size_t)b * q.HW + p) * yd;
        const uint64_t z0 = offset + ((uint64_t)g * q.HW + p) * q.x_d;
        float v[V];
#pragma unroll
        for (int j = 0; j < V; j++) {
            const int c = cu * V + j;
            v[j] = c < q.x_d ? temperature * instance_noise_value(0.f, false, 0.f, seed, z0 + c) : yp[c - q.x_d];
        }
        if constexpr (VEC)
            *reinterpret_cast<f4*>(zy + (size_t)e * 4) = f4{v[0], v[1], v[2], v[3]};
        else
            zy[e] = v[0];
    }
}

// k_sample_fold's workgroup: FOLD_E consecutive elements of one condition x FOLD_L draw lanes; the draws of
// the chunk go through LDS in batches of FOLD_BATCH
constexpr int FOLD_E = 32, FOLD_L = 8, FOLD_BATCH = 64;

// A workgroup owns FOLD_E elements (p, c) of one condition b of those the chunk touches (b0 .. b0 + nb - 1;
// bpc workgroups per condition). The post-transform of a value does not depend on the other draws, so all
// 256 threads apply it, thread (e, l) to the draws l, l + FOLD_L, ... of a batch (their loads in flight
// together: the draws are an image apart), store the sample and leave the value in LDS; the fold is a
// serial chain per element, three operations a draw, which thread (e, 0) runs over the batch in draw order.
// The draws s0 .. s1 - 1 of b in the chunk are the same for the whole workgroup: the barriers sit in
// uniform control flow.
__global__ __launch_bounds__(256) void k_sample_fold(SampleChunk q, SampleFoldArgs a, long long b0, int bpc) {
    __shared__ float sh[FOLD_BATCH][FOLD_E];
    const int per = q.HW * q.x_d;   // elements per condition
    const long long b = b0 + blockIdx.x / bpc;
    const int e = threadIdx.x % FOLD_E, l = threadIdx.x / FOLD_E;
    const int pc = (blockIdx.x % bpc) * FOLD_E + e;
    const bool valid = pc < per;
    const int p = pc / q.x_d, c = pc - p * q.x_d;
    const long long gb = b * q.S, g1 = q.g0 + q.n;
    const int s0 = (int)((q.g0 > gb ? q.g0 : gb) - gb);
    const int s1 = (int)((g1 < gb + q.S ? g1 : gb + q.S) - gb);
    const size_t plane = (size_t)a.B * per;   // state: [3][B][HW][x_d]
    const size_t se = (size_t)b * per + pc;
    const bool stats = a.state != nullptr;
    const bool folds = stats && valid && l == 0;
    const float yv = a.residual && valid ? a.y[se] : 0.f;   // (D - x_d == x_d: y[b] has x's shape)
    float K = 0.f, S1 = 0.f, S2 = 0.f;
    if (folds && s0 > 0) {
        K = a.state[se];
        S1 = a.state[plane + se];
        S2 = a.state[2 * plane + se];
    }
    const size_t img = (size_t)q.HW * q.D;
    const float* __restrict__ src = a.xy_hat + (size_t)p * q.D + c;   // the element in image 0 of the chunk
    for (int sb = s0; sb < s1; sb += FOLD_BATCH) {
        float w[FOLD_BATCH / FOLD_L];
#pragma unroll
        for (int j = 0; j < FOLD_BATCH / FOLD_L; j++) {
            const int s = sb + l + j * FOLD_L;
            w[j] = valid && s < s1 ? src[(size_t)(gb + s - q.g0) * img] : 0.f;   // (s >= s0: image gb + s - g0 >= 0)
        }
#pragma unroll
        for (int j = 0; j < FOLD_BATCH / FOLD_L; j++) {
            const int s = sb + l + j * FOLD_L;
            float v = w[j];
            if (a.logit) v = delogit_value(v, a.lk);
            if (a.residual) v = v + yv;
            if (valid && s < s1 && a.samples != nullptr) a.samples[(size_t)(gb + s) * per + pc] = v;
            if (stats) sh[l + j * FOLD_L][e] = v;
        }
        if (!stats) continue;
        __syncthreads();
        if (folds) {
            const int nk = s1 - sb < FOLD_BATCH ? s1 - sb : FOLD_BATCH;
#pragma unroll 8
            for (int k = 0; k < nk; k++) sample_fold(sh[k][e], sb + k == 0, K, S1, S2);
        }
        __syncthreads();
    }
    if (!folds) return;
    if (s1 < q.S) {
        a.state[se] = K;
        a.state[plane + se] = S1;
        a.state[2 * plane + se] = S2;
    } else {
        float mean, sd;
        sample_finish(K, S1, S2, (float)q.S, mean, sd);
        if (a.mean != nullptr) a.mean[se] = mean;
        if (a.std != nullptr) a.std[se] = sd;
    }
}

// one wave per image of the chunk; lane sums in fp64 over its elements in order, then the wave sum
__global__ __launch_bounds__(256) void k_sample_ydev(SampleChunk q, const float* __restrict__ xy_hat,
                                                     const float* __restrict__ y, float* __restrict__ y_dev) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= q.n) return;   // (whole waves)
    const long long g = q.g0 + i;
    const long long b = g / q.S;
    const int yd = q.D - q.x_d, n = q.HW * yd;
    const float* __restrict__ xi = xy_hat + (size_t)i * q.HW * q.D;
    const float* __restrict__ yb = y + (size_t)b * n;
    double s = 0.0;
    for (int e = lane; e < n; e += 64) {
        const int p = e / yd, c = e - p * yd;
        s += (double)fabsf(xi[(size_t)p * q.D + q.x_d + c] - yb[e]);
    }
    s = wave_sum(s);
    if (lane == 0) y_dev[g] = (float)s;
}

// one wave per image of the chunk: log_prob[g] = log N(z; 0, I) + sum over couplings of sum s, from the
// chunk's latent (the x channels of zy as stored) and the log-det partial slots part[nl][n][np] the
// chunk's inverse left in its workspace. q = sum z^2: fp64 lane sums over the image's HW * x_d latent
// elements in element order, then the wave sum; L: the slots in k_ld_reduce's order (ld_slot_sum).
__global__ __launch_bounds__(256) void k_sample_logp(SampleChunk q, const float* __restrict__ zy,
                                                     const double* __restrict__ part, int nl, int np,
                                                     float* __restrict__ log_prob) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= q.n) return;   // (whole waves)
    const int n = q.HW * q.x_d;
    const float* __restrict__ zi = zy + (size_t)i * q.HW * q.D;
    double s = 0.0;
    for (int e = lane; e < n; e += 64) {
        const int p = e / q.x_d, c = e - p * q.x_d;
        const double z = (double)zi[(size_t)p * q.D + c];
        s += z * z;
    }
    s = wave_sum(s);
    const double L = ld_slot_sum(part, q.n, i, nl, np, lane);
    if (lane == 0) log_prob[q.g0 + i] = (float)(-0.5 * s - 0.5 * (double)n * LOG_2PI_D + L);
}

int grid_for(long long n) {
    const long long g = (n + 255) / 256;
    return (int)(g < 1 ? 1 : (g > 65536 ? 65536 : g));
}

}  // namespace

void launch_latent(const SampleChunk& c, const float* y, float* zy, float temperature, unsigned long long seed,
                   unsigned long long offset, hipStream_t st) {
    if (c.D % 4 == 0) {
        const long long n = (long long)c.n * c.HW * (c.D / 4);
        CNF_LAUNCH(k_latent<true>, dim3(grid_for(n)), dim3(256), 0, st, c, y, zy, temperature, (uint64_t)seed,
                   (uint64_t)offset);
    } else {
        const long long n = (long long)c.n * c.HW * c.D;
        CNF_LAUNCH(k_latent<false>, dim3(grid_for(n)), dim3(256), 0, st, c, y, zy, temperature, (uint64_t)seed,
                   (uint64_t)offset);
    }
}

void launch_sample_fold(const SampleChunk& c, const SampleFoldArgs& a, hipStream_t st) {
    const long long b0 = c.g0 / c.S, b1 = (c.g0 + c.n - 1) / c.S;
    const int nb = (int)(b1 - b0 + 1);
    const int bpc = (c.HW * c.x_d + FOLD_E - 1) / FOLD_E;   // workgroups per condition
    CNF_LAUNCH(k_sample_fold, dim3((unsigned)nb * bpc), dim3(256), 0, st, c, a, b0, bpc);
}

void launch_sample_ydev(const SampleChunk& c, const float* xy_hat, const float* y, float* y_dev, hipStream_t st) {
    CNF_LAUNCH(k_sample_ydev, dim3((c.n + 3) / 4), dim3(256), 0, st, c, xy_hat, y, y_dev);
}

void launch_sample_logp(const SampleChunk& c, const float* zy, const double* ld_part, int nl, int np, float* log_prob,
                        hipStream_t st) {
    CNF_LAUNCH(k_sample_logp, dim3((c.n + 3) / 4), dim3(256), 0, st, c, zy, ld_part, nl, np, log_prob);
}

}  // namespace cnf
