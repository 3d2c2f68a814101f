// cnf_score.hip — the kernels around the data-gradient-only backward (cnf_flow_score, cnf_flow_ascend,
// include/cnf.h): the input gradients of the log-density and the ascent on it.
//   k_score_seed    one pass over a chunk's zy: the backward's seed dzy and each image's llz
//   k_score_finish  the flow-input gradient through the gather's logit / residual map: grad_x, grad_y, log_prob
//   k_ascend_step   one Keras Adam step up the gradient on the x channels of the chunk's xy, in place
//   k_ascend_out    the ascent's iterate through the sampler's post-transform
// All HBM-bound element / reduction kernels; no atomics and no counters, every floating-point sum in the
// fixed order cnf_kernels.h states (per-thread fp64 folds in element order, wave_sum, waves in order).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <stdexcept>

#include "cnf_device.h"

namespace cnf {

namespace {

// the workgroup's sum of acc: the wave butterfly, then the waves in order; valid in thread 0 (cnf_logprob.hip's)
__device__ __forceinline__ double block_sum(double acc, double* sh) {
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    const double s = ((sh[0] + sh[1]) + sh[2]) + sh[3];
    __syncthreads();
    return s;
}

// the image's lj slots in slot order (every thread that needs it: the same order, the same value)
__device__ __forceinline__ double lj_sum(const double* __restrict__ lj, int i, int parts, double base) {
    double J = base;
    for (int k = 0; k < parts; k++) J += lj[(size_t)i * parts + k];
    return J;
}

// one workgroup per image of the chunk; thread t owns the float4 groups 4 (t + 256 j) of the image's HW * D
// floats, as k_logp_finish
__global__ __launch_bounds__(256) void k_score_seed(LogpChunk q, ScoreSeedArgs a, int parts) {
    __shared__ double sh[4];
    const int i = blockIdx.x;
    const int n = q.HW * q.D;
    const float* __restrict__ zi = a.zy + (size_t)i * n;
    float* __restrict__ di = a.dzy != nullptr ? a.dzy + (size_t)i * n : nullptr;
    double zz = 0.0;
    for (int e0 = 4 * (int)threadIdx.x; e0 < n; e0 += LOGP_FINISH_STEP) {
        const f4 t = *reinterpret_cast<const f4*>(zi + e0);
        const float z[4] = {t.x, t.y, t.z, t.w};
        float d[4];
        int c = e0 % q.D;
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const bool xc = c < q.x_d;
            if (xc) zz += (double)z[u] * (double)z[u];
            d[u] = xc ? -z[u] : 0.f;
            if (++c == q.D) c = 0;
        }
        if (di != nullptr) *reinterpret_cast<f4*>(di + e0) = f4{d[0], d[1], d[2], d[3]};
    }
    zz = block_sum(zz, sh);
    if (threadIdx.x != 0) return;
    const double llz = -0.5 * zz - 0.5 * (double)(q.HW * q.x_d) * LOG_2PI_D;
    a.llz[i] = llz;
    if (a.trace != nullptr) {
        const bool ok = a.lj == nullptr || lj_sum(a.lj, i, parts, 0.0) > -(double)INFINITY;
        a.trace[q.g0 + i] = ok ? (float)(llz + (double)a.ld[i]) : -INFINITY;
    }
}

// grid (trips, n): thread t of workgroup (j, i) owns the float4 group 4 (t + 256 j) of image i's HW * D floats
__global__ __launch_bounds__(256) void k_score_finish(LogpChunk q, ScoreFinishArgs a, int parts) {
    const int i = blockIdx.y;
    const long long g = q.g0 + i;
    const int n = q.HW * q.D, yd = q.D - q.x_d;
    const double J = lj_sum(a.lj, i, parts, a.lj_const);
    const bool ok = J > -(double)INFINITY;   // (false for NaN too)
    if (blockIdx.x == 0 && threadIdx.x == 0 && a.log_prob != nullptr)
        a.log_prob[g] = ok ? (float)(a.llz[i] + (double)a.ld[i] + J) : -INFINITY;
    if (a.g == nullptr) return;
    const int e0 = 4 * ((int)blockIdx.x * 256 + (int)threadIdx.x);
    if (e0 >= n) return;
    const f4 t4 = *reinterpret_cast<const f4*>(a.g + (size_t)i * n + e0);
    const float gv[4] = {t4.x, t4.y, t4.z, t4.w};
    const float* __restrict__ xi = a.x + (size_t)g * q.HW * q.x_d;
    const float* __restrict__ yi = a.y + (size_t)g * q.HW * yd;
    float* __restrict__ gx = a.grad_x != nullptr ? a.grad_x + (size_t)g * q.HW * q.x_d : nullptr;
    float* __restrict__ gy = a.grad_y != nullptr ? a.grad_y + (size_t)g * q.HW * yd : nullptr;
    const float nanv = __builtin_nanf("");
    int p = e0 / q.D, c = e0 - p * q.D;
    // with residual, channel c of y pairs with channel c of x (D == 2 x_d): its element computes that x
    // channel's t again from g (the same expression, the same bits) rather than pass it between threads
    for (int u = 0; u < 4; u++) {
        if (c < q.x_d) {
            float t = gv[u];
            if (a.logit) {
                const float v = a.residual ? xi[(size_t)p * q.x_d + c] - yi[(size_t)p * yd + c] : xi[(size_t)p * q.x_d + c];
                const float e = fmaf(a.lk.c1, v, a.lk.a);
                const float r = a.lk.c1 / (e * (1.f - e));
                t = gv[u] * (r / a.lk.span) - r * (1.f - 2.f * e);
            }
            if (gx != nullptr) gx[(size_t)p * q.x_d + c] = ok ? t : nanv;
        } else if (gy != nullptr) {
            const int cy = c - q.x_d;
            float o = gv[u];
            if (a.residual) {
                float t = a.g[(size_t)i * n + (size_t)p * q.D + cy];
                if (a.logit) {
                    const float v = xi[(size_t)p * q.x_d + cy] - yi[(size_t)p * yd + cy];
                    const float e = fmaf(a.lk.c1, v, a.lk.a);
                    const float r = a.lk.c1 / (e * (1.f - e));
                    t = t * (r / a.lk.span) - r * (1.f - 2.f * e);
                }
                o -= t;
            }
            gy[(size_t)p * yd + cy] = ok ? o : nanv;
        }
        if (++c == q.D) c = 0, p++;
    }
}

// one thread per x element of the chunk
__global__ __launch_bounds__(256) void k_ascend_step(LogpChunk q, AscendStepArgs a, long long total) {
    for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < total; k += (long long)gridDim.x * 256) {
        const long long px = k / q.x_d;
        const int c = (int)(k - px * q.x_d);
        const size_t e = (size_t)px * q.D + c;
        const float gi = -a.g[e];
        const float mi = a.m[k] + (gi - a.m[k]) * (1.f - a.b1);
        const float vi = a.v[k] + (gi * gi - a.v[k]) * (1.f - a.b2);
        a.m[k] = mi;
        a.v[k] = vi;
        a.xy[e] -= a.alpha * mi / (sqrtf(vi) + a.eps);
    }
}

// grid (blocks, n): the x elements of image i, one per thread
__global__ __launch_bounds__(256) void k_ascend_out(LogpChunk q, AscendOutArgs a, int parts) {
    const int i = blockIdx.y;
    const long long g = q.g0 + i;
    const int nx = q.HW * q.x_d, yd = q.D - q.x_d;
    const bool ok = lj_sum(a.lj, i, parts, 0.0) > -(double)INFINITY;
    for (int k = (int)blockIdx.x * 256 + (int)threadIdx.x; k < nx; k += (int)gridDim.x * 256) {
        const int p = k / q.x_d, c = k - p * q.x_d;
        const size_t o = (size_t)g * nx + k;
        const float yv = a.residual ? a.y[((size_t)g * q.HW + p) * yd + c] : 0.f;
        const float v = sample_post_value(a.xy[((size_t)i * q.HW + p) * q.D + c], a.logit, a.lk, a.residual, yv);
        a.x_out[o] = ok ? v : a.x0[o];
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

void launch_score_seed(const LogpChunk& c, const ScoreSeedArgs& a, hipStream_t st) {
    if ((c.HW * c.D) % 4 != 0 || !aligned16(a.zy) || !aligned16(a.dzy))
        throw std::logic_error("k_score_seed: zy is not a row of float4");
    CNF_LAUNCH(k_score_seed, dim3((unsigned)c.n), dim3(256), 0, st, c, a, logp_parts(c.HW));
}

void launch_score_finish(const LogpChunk& c, const ScoreFinishArgs& a, hipStream_t st) {
    if ((c.HW * c.D) % 4 != 0 || !aligned16(a.g)) throw std::logic_error("k_score_finish: g is not a row of float4");
    if (a.residual && c.D != 2 * c.x_d) throw std::logic_error("k_score_finish: residual needs D == 2 x_d");
    const int trips = logp_finish_trips(c.HW, c.D);
    CNF_LAUNCH(k_score_finish, dim3((unsigned)trips, (unsigned)c.n), dim3(256), 0, st, c, a, logp_parts(c.HW));
}

void launch_ascend_step(const LogpChunk& c, const AscendStepArgs& a, hipStream_t st) {
    const long long total = (long long)c.n * c.HW * c.x_d;
    const long long gx = std::min<long long>(8192, (total + 255) / 256);
    CNF_LAUNCH(k_ascend_step, dim3((unsigned)gx), dim3(256), 0, st, c, a, total);
}

void launch_ascend_out(const LogpChunk& c, const AscendOutArgs& a, hipStream_t st) {
    if (a.residual && c.D != 2 * c.x_d) throw std::logic_error("k_ascend_out: residual needs D == 2 x_d");
    const int gx = std::min(64, (c.HW * c.x_d + 255) / 256);
    CNF_LAUNCH(k_ascend_out, dim3((unsigned)gx, (unsigned)c.n), dim3(256), 0, st, c, a, logp_parts(c.HW));
}

}  // namespace cnf
