// cnf_logprob.hip — the density of given images around the forward (cnf_flow_log_prob, include/cnf.h): the
// counterpart of cnf_sample.hip, an image x in the space of the returned samples back to the flow's input and
// the terms of its log-density per (image, condition) pair.
//   k_logp_gather     one chunk of xy = concat(logit_value(x - y), y) and the pairs' log-Jacobian partials
//   k_logp_finish     per pair: llz and y_dev from one pass over zy, + the forward's log-det + log_jac
//   k_logp_posterior  per image: softmax over the conditions of log_prob + log_prior, and its log-sum-exp
// All HBM-bound element / reduction kernels; no atomics and no counters, every floating-point sum in the
// fixed order cnf_kernels.h states (per-thread fp64 folds in element order, wave_sum, waves in order).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <stdexcept>

#include "cnf_device.h"

namespace cnf {

namespace {

// the flow-space value of one x element and its log-Jacobian term (into acc): sample_post_value's inverse,
// with logit_value's own e deciding the domain
__device__ __forceinline__ float logp_value(float x, float yv, const LogpGatherArgs& a, double& acc) {
    float v = a.residual ? x - yv : x;
    if (a.logit) {
        const float e = fmaf(a.lk.c1, v, a.lk.a);
        if (e > 0.f && e < 1.f) {
            acc += -log((double)e * (1.0 - (double)e));
            v = logit_value(v, a.lk);
        } else {   // (NaN too)
            acc += -(double)INFINITY;
            v = 0.f;
        }
    }
    return v;
}

// the workgroup's sum of acc: the wave butterfly, then the waves in order; valid in thread 0
__device__ __forceinline__ double block_sum(double acc, double* sh) {
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    const double s = ((sh[0] + sh[1]) + sh[2]) + sh[3];
    __syncthreads();
    return s;
}

// Workgroup blockIdx.x takes work item w = (tile, pair of the chunk), tile-major, so that items next to each
// other are pairs of one image reading the same tile of x. Workgroups are dealt round-robin over the 8 XCDs
// (observed, not promised: only speed depends on it), so XCD j gets the contiguous range
// [j per_xcd, (j + 1) per_xcd) of the items and a tile of x is fetched into one L2, once.
__device__ __forceinline__ bool logp_item(const LogpChunk& q, int parts, int per_xcd, int& part, int& i) {
    const int w = (int)(blockIdx.x & 7) * per_xcd + (int)(blockIdx.x >> 3);
    if (w >= q.n * parts) return false;   // (the whole workgroup)
    part = w / q.n;
    i = w - part * q.n;
    return true;
}

// XD x channels, YD condition channels, HW % 4 == 0 and 16-byte aligned tensors: a thread's quad of pixels is
// XD + YD 16-byte loads and XD + YD 16-byte stores of contiguous NHWC rows
template <int XD, int YD>
__global__ __launch_bounds__(256) void k_logp_gather(LogpChunk q, LogpGatherArgs a, int parts, int per_xcd) {
    constexpr int D = XD + YD;
    __shared__ double sh[4];
    int part, i;
    if (!logp_item(q, parts, per_xcd, part, i)) return;
    const long long g = q.g0 + i;
    const long long img = q.K > 0 ? g / q.K : g, cond = q.K > 0 ? g % q.K : g;
    const int quad = part * LOGP_QUADS + (int)threadIdx.x;
    double acc = 0.0;
    if (quad < q.HW / 4) {
        const f4* __restrict__ xp = reinterpret_cast<const f4*>(a.x + ((size_t)img * q.HW + 4 * (size_t)quad) * XD);
        const f4* __restrict__ yp = reinterpret_cast<const f4*>(a.y + ((size_t)cond * q.HW + 4 * (size_t)quad) * YD);
        f4* __restrict__ op = reinterpret_cast<f4*>(a.xy + ((size_t)i * q.HW + 4 * (size_t)quad) * D);
        float xf[4 * XD], yf[4 * YD], of[4 * D];
#pragma unroll
        for (int j = 0; j < XD; j++) {
            const f4 t = xp[j];
            xf[4 * j] = t.x, xf[4 * j + 1] = t.y, xf[4 * j + 2] = t.z, xf[4 * j + 3] = t.w;
        }
#pragma unroll
        for (int j = 0; j < YD; j++) {
            const f4 t = yp[j];
            yf[4 * j] = t.x, yf[4 * j + 1] = t.y, yf[4 * j + 2] = t.z, yf[4 * j + 3] = t.w;
        }
#pragma unroll
        for (int p = 0; p < 4; p++) {
#pragma unroll
            for (int c = 0; c < XD; c++)   // (residual: XD == YD, checked on the host)
                of[p * D + c] = logp_value(xf[p * XD + c], XD == YD ? yf[p * YD + c] : 0.f, a, acc);
#pragma unroll
            for (int c = 0; c < YD; c++) of[p * D + XD + c] = yf[p * YD + c];
        }
#pragma unroll
        for (int j = 0; j < D; j++) op[j] = f4{of[4 * j], of[4 * j + 1], of[4 * j + 2], of[4 * j + 3]};
    }
    const double s = block_sum(acc, sh);
    if (threadIdx.x == 0) a.lj[(size_t)i * parts + part] = s;
}

// any shape and alignment: the same quads and the same element order, element by element
__global__ __launch_bounds__(256) void k_logp_gather_any(LogpChunk q, LogpGatherArgs a, int parts, int per_xcd) {
    __shared__ double sh[4];
    int part, i;
    if (!logp_item(q, parts, per_xcd, part, i)) return;
    const long long g = q.g0 + i;
    const long long img = q.K > 0 ? g / q.K : g, cond = q.K > 0 ? g % q.K : g;
    const int yd = q.D - q.x_d;
    const int quad = part * LOGP_QUADS + (int)threadIdx.x;
    double acc = 0.0;
    for (int j = 0; j < 4; j++) {
        const int p = 4 * quad + j;
        if (p >= q.HW) break;
        const float* __restrict__ xp = a.x + ((size_t)img * q.HW + p) * q.x_d;
        const float* __restrict__ yp = a.y + ((size_t)cond * q.HW + p) * yd;
        float* __restrict__ op = a.xy + ((size_t)i * q.HW + p) * q.D;
        for (int c = 0; c < q.x_d; c++) op[c] = logp_value(xp[c], a.residual ? yp[c] : 0.f, a, acc);
        for (int c = 0; c < yd; c++) op[q.x_d + c] = yp[c];
    }
    const double s = block_sum(acc, sh);
    if (threadIdx.x == 0) a.lj[(size_t)i * parts + part] = s;
}

// one workgroup per pair of the chunk. Thread t owns the element groups 4 (t + 256 j) .. + 3 of the image's
// HW * D floats, one 16-byte load each (H and W are even, so HW * D % 4 == 0, and zy is the workspace's).
__global__ __launch_bounds__(256) void k_logp_finish(LogpChunk q, LogpFinishArgs a, int parts) {
    __shared__ double sh[4];
    const int i = blockIdx.x;
    const long long g = q.g0 + i;
    const long long cond = q.K > 0 ? g % q.K : g;
    const int n = q.HW * q.D, yd = q.D - q.x_d;
    const float* __restrict__ zi = a.zy + (size_t)i * n;
    const float* __restrict__ yc = a.y + (size_t)cond * q.HW * yd;
    double zz = 0.0, dev = 0.0;
    for (int e0 = 4 * (int)threadIdx.x; e0 < n; e0 += LOGP_FINISH_STEP) {
        const f4 t = *reinterpret_cast<const f4*>(zi + e0);
        const float z[4] = {t.x, t.y, t.z, t.w};
        int p = e0 / q.D, c = e0 - p * q.D;
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (c < q.x_d)
                zz += (double)z[u] * (double)z[u];
            else
                dev += (double)fabsf(z[u] - yc[(size_t)p * yd + (c - q.x_d)]);
            if (++c == q.D) c = 0, p++;
        }
    }
    zz = block_sum(zz, sh);
    dev = block_sum(dev, sh);
    if (threadIdx.x != 0) return;
    double J = a.lj_const;
    for (int k = 0; k < parts; k++) J += a.lj[(size_t)i * parts + k];
    const bool ok = J > -(double)INFINITY;   // (false for NaN too)
    const double llz = -0.5 * zz - 0.5 * (double)(q.HW * q.x_d) * LOG_2PI_D;
    const float ld = a.ld[i];
    const float nanv = __builtin_nanf(""), ninf = -INFINITY;
    if (a.log_prob != nullptr) a.log_prob[g] = ok ? (float)(llz + (double)ld + J) : ninf;
    if (a.llz != nullptr) a.llz[g] = ok ? (float)llz : nanv;
    if (a.logdet != nullptr) a.logdet[g] = ok ? ld : nanv;
    if (a.log_jac != nullptr) a.log_jac[g] = ok ? (float)J : ninf;
    if (a.y_dev != nullptr) a.y_dev[g] = ok ? (float)dev : nanv;
}

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

// WAVE: four rows per workgroup, one wave each (K <= 64: one entry per lane); otherwise one row per
// workgroup, thread t folding entries t, t + 256, ... in order
template <bool WAVE>
__global__ __launch_bounds__(256) void k_logp_posterior(const float* __restrict__ log_prob,
                                                        const float* __restrict__ log_prior,
                                                        float* __restrict__ posterior,
                                                        float* __restrict__ log_evidence, int B, int K) {
    __shared__ double sh[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int row = WAVE ? (int)blockIdx.x * 4 + wv : (int)blockIdx.x;
    if (row >= B) return;   // (WAVE: whole waves, and no barrier below; otherwise never)
    const int t = WAVE ? lane : (int)threadIdx.x, T = WAVE ? 64 : 256;
    const float* __restrict__ r = log_prob + (size_t)row * K;
    auto entry = [&](int k) { return (double)r[k] + (log_prior != nullptr ? (double)log_prior[k] : 0.0); };
    double m = -(double)INFINITY;
    for (int k = t; k < K; k += T) m = fmax(m, entry(k));
    m = wave_max(m);
    if (!WAVE) {
        if (lane == 0) sh[wv] = m;
        __syncthreads();
        m = fmax(fmax(sh[0], sh[1]), fmax(sh[2], sh[3]));
        __syncthreads();
    }
    double s = 0.0;
    for (int k = t; k < K; k += T) s += exp(entry(k) - m);
    s = wave_sum(s);
    if (!WAVE) {
        if (lane == 0) sh[wv] = s;
        __syncthreads();
        s = ((sh[0] + sh[1]) + sh[2]) + sh[3];
    }
    const bool none = m == -(double)INFINITY;   // every entry -inf: no condition explains the image
    const double lse = none ? m : m + log(s);
    if (posterior != nullptr)
        for (int k = t; k < K; k += T)
            posterior[(size_t)row * K + k] = none ? __builtin_nanf("") : (float)exp(entry(k) - lse);
    if (log_evidence != nullptr && t == 0) log_evidence[row] = (float)lse;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

void launch_logp_gather(const LogpChunk& c, const LogpGatherArgs& a, hipStream_t st) {
    const int parts = logp_parts(c.HW);
    const int per_xcd = logp_per_xcd(c.n, parts);
    const dim3 grid((unsigned)per_xcd * 8);
    void (*k)(LogpChunk, LogpGatherArgs, int, int) = nullptr;
    switch (logp_gather_choice(c.x_d, c.D - c.x_d, c.HW, aligned16(a.x) && aligned16(a.y) && aligned16(a.xy))) {
        case LOGP_GATHER_ANY: k = k_logp_gather_any; break;
        case LOGP_GATHER_1_1: k = k_logp_gather<1, 1>; break;
        case LOGP_GATHER_3_1: k = k_logp_gather<3, 1>; break;
        case LOGP_GATHER_3_3: k = k_logp_gather<3, 3>; break;
    }
    if (k == nullptr) throw std::logic_error("k_logp_gather: no kernel for the choice");
    CNF_LAUNCH(k, grid, dim3(256), 0, st, c, a, parts, per_xcd);
}

void launch_logp_finish(const LogpChunk& c, const LogpFinishArgs& a, hipStream_t st) {
    if ((c.HW * c.D) % 4 != 0 || !aligned16(a.zy)) throw std::logic_error("k_logp_finish: zy is not a row of float4");
    CNF_LAUNCH(k_logp_finish, dim3((unsigned)c.n), dim3(256), 0, st, c, a, logp_parts(c.HW));
}

void launch_logp_posterior(const float* log_prob, const float* log_prior, float* posterior, float* log_evidence,
                           int B, int K, hipStream_t st) {
    if (K <= 64)
        CNF_LAUNCH(k_logp_posterior<true>, dim3((unsigned)(B + 3) / 4), dim3(256), 0, st, log_prob, log_prior,
                   posterior, log_evidence, B, K);
    else
        CNF_LAUNCH(k_logp_posterior<false>, dim3((unsigned)B), dim3(256), 0, st, log_prob, log_prior, posterior,
                   log_evidence, B, K);
}

}  // namespace cnf
