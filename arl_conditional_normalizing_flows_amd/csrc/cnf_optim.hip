// cnf_optim.hip — the clipped, guarded Adam step (cnf_optim_step, include/cnf.h; host side: cnf_optim.cpp).
//   k_optim_stats   per slab: the fp64 sums of g^2 and of h^2 (h = g clamped to +-clipvalue), the count of NaN / inf
//   k_optim_finish  one workgroup: the tensors' s_t, the global N and S, scale_t, skip or apply, the counters, alpha
//   k_optim_step    per slab: clamp, scale, k_adam's update, the EMA; returns at once on a skipped step
// All HBM-bound passes over the flat vectors: 16-byte accesses on the part of a slab that is 16-byte aligned, scalar
// on its head and tail. Plain vector stores, no atomics, no counters between workgroups: every sum has one fixed
// order (a thread's elements in order, wave_sum, the waves in order; a tensor's slabs in slab order; the tensors in
// table order), and every workspace word a kernel reads was written earlier in the same step.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "cnf_device.h"

namespace cnf {

namespace {

__device__ __forceinline__ bool nonfinite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

// a * b rounded to fp32 on its own: never contracted into the operation that uses it
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}

// The parts of a slab: `head` scalar elements up to the first 16-byte boundary (all of it when the vectors
// are not 16-byte aligned), `quads` float4 groups, then the scalar tail from `tail`.
struct SlabParts {
    int head, quads, tail;
};
__device__ __forceinline__ SlabParts slab_parts(const OptimSlab& e, bool vec) {
    SlabParts s;
    s.head = vec ? min(e.count, (int)((4 - (e.start & 3)) & 3)) : e.count;
    s.quads = (e.count - s.head) >> 2;
    s.tail = s.head + 4 * s.quads;
    return s;
}

__global__ __launch_bounds__(256) void k_optim_stats(const float* __restrict__ g, const OptimSlab* __restrict__ slabs,
                                                     long long num_slabs, float cv, bool vec,
                                                     double* __restrict__ sum_g, double* __restrict__ sum_h,
                                                     unsigned* __restrict__ bad) {
    __shared__ double sh[8];
    __shared__ unsigned shc[4];
    const int tid = threadIdx.x;
    for (long long s = blockIdx.x; s < num_slabs; s += gridDim.x) {
        const OptimSlab e = slabs[s];
        const SlabParts sp = slab_parts(e, vec);
        const float* __restrict__ gs = g + e.start;
        double a = 0.0, b = 0.0;
        unsigned c = 0;
        auto one = [&](float x) {
            a += (double)x * (double)x;
            if (cv > 0.f) {
                const float h = fminf(fmaxf(x, -cv), cv);
                b += (double)h * (double)h;
            }
            c += nonfinite(x) ? 1u : 0u;
        };
        for (int i = tid; i < sp.head; i += 256) one(gs[i]);
        for (int i = tid; i < sp.quads; i += 256) {
            const f4 t = *reinterpret_cast<const f4*>(gs + sp.head + 4 * i);
            one(t.x);
            one(t.y);
            one(t.z);
            one(t.w);
        }
        for (int i = sp.tail + tid; i < e.count; i += 256) one(gs[i]);
        a = wave_sum(a);
        b = wave_sum(b);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
        if ((tid & 63) == 0) {
            sh[2 * (tid >> 6)] = a;
            sh[2 * (tid >> 6) + 1] = b;
            shc[tid >> 6] = c;
        }
        __syncthreads();
        if (tid == 0) {
            const double A = ((sh[0] + sh[2]) + sh[4]) + sh[6];
            sum_g[s] = A;
            sum_h[s] = cv > 0.f ? ((sh[1] + sh[3]) + sh[5]) + sh[7] : A;
            bad[s] = shc[0] + shc[1] + shc[2] + shc[3];
        }
        __syncthreads();
    }
}

constexpr int FINISH_THREADS = 1024;                        // k_optim_finish's one workgroup
constexpr int FINISH_PER = 2;                               // tensors per thread and pass
constexpr int FINISH_CHUNK = FINISH_THREADS * FINISH_PER;   // tensors per pass (40 KiB of LDS)

// One workgroup. Pass 1, FINISH_CHUNK tensors at a time: each thread folds its tensors' slabs in slab order and
// takes s_t; thread 0 then adds the chunk's tensors to the global sums in table order. Thread 0 decides the step;
// pass 2 multiplies every s_t by S.
__global__ __launch_bounds__(FINISH_THREADS) void k_optim_finish(const int* __restrict__ first, int T, cnf_optim_desc d,
                                                      OptimWs ws, long long* __restrict__ state,
                                                      float* __restrict__ stats, float* __restrict__ scales_out) {
    __shared__ double sg[FINISH_CHUNK], sh[FINISH_CHUNK];
    __shared__ unsigned sc[FINISH_CHUNK];
    __shared__ float S_sh;
    const int tid = threadIdx.x;
    double G = 0.0, N2 = 0.0;      // thread 0: sum of g^2, sum of s_t^2 * sum_t h^2
    unsigned long long NF = 0;     // thread 0: non-finite elements of g
    for (int base = 0; base < T; base += FINISH_CHUNK) {
        const int end = min(T, base + FINISH_CHUNK);
        // a thread's tensors of the chunk side by side, so that their loads are in flight together: the
        // slab ranges, then each tensor's first slab, then the rest of its slabs in slab order
        int k0[FINISH_PER], k1[FINISH_PER];
        double a[FINISH_PER], b[FINISH_PER];
        unsigned c[FINISH_PER];
#pragma unroll
        for (int j = 0; j < FINISH_PER; j++) {
            const int t = base + tid + FINISH_THREADS * j;
            k0[j] = t < end ? first[t] : 0;
            k1[j] = t < end ? first[t + 1] : 0;
        }
#pragma unroll
        for (int j = 0; j < FINISH_PER; j++) {
            const bool has = k1[j] > k0[j];
            a[j] = has ? ws.sum_g[k0[j]] : 0.0;
            b[j] = has ? ws.sum_h[k0[j]] : 0.0;
            c[j] = has ? ws.nonfinite[k0[j]] : 0u;
        }
#pragma unroll
        for (int j = 0; j < FINISH_PER; j++) {
            for (int k = k0[j] + 1; k < k1[j]; k += 8) {   // eight slabs' loads ahead of the adds, which stay in order
                double x[8], y[8];
                unsigned z[8];
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    const int kk = min(k + u, k1[j] - 1);
                    x[u] = ws.sum_g[kk];
                    y[u] = ws.sum_h[kk];
                    z[u] = ws.nonfinite[kk];
                }
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    if (k + u < k1[j]) {
                        a[j] += x[u];
                        b[j] += y[u];
                        c[j] += z[u];
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < FINISH_PER; j++) {
            const int t = base + tid + FINISH_THREADS * j;
            if (t < end) {
                float s = 1.f;
                if (d.clipnorm > 0.f) {
                    const double cn = (double)d.clipnorm;
                    s = (float)(cn / fmax(sqrt(b[j]), cn));   // fmax drops a NaN norm: s = 1
                }
                ws.scale[t] = s;
                sg[t - base] = a[j];
                sh[t - base] = (double)s * (double)s * b[j];
                sc[t - base] = c[j];
            }
        }
        __syncthreads();
        if (tid == 0) {   // table order; eight LDS reads at a time ahead of the dependent adds
            const int cnt = end - base;
            int i = 0;
            for (; i + 8 <= cnt; i += 8) {
                double x[8], y[8];
                unsigned z[8];
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    x[u] = sg[i + u];
                    y[u] = sh[i + u];
                    z[u] = sc[i + u];
                }
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    G += x[u];
                    N2 += y[u];
                    NF += z[u];
                }
            }
            for (; i < cnt; i++) {
                G += sg[i];
                N2 += sh[i];
                NF += sc[i];
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        const double N = sqrt(N2);
        float S = 1.f;
        if (d.global_clipnorm > 0.f) {
            const double cn = (double)d.global_clipnorm;
            S = (float)(cn / fmax(N, cn));
        }
        const bool skip = d.skip_nonfinite != 0 && NF != 0;
        const long long applied = state[0];
        if (skip)
            state[1] = state[1] + 1;
        else
            state[0] = applied + 1;
        const double t = (double)(applied + 1);
        const float alpha =
            (float)((double)d.lr * sqrt(1.0 - pow((double)d.beta_2, t)) / (1.0 - pow((double)d.beta_1, t)));
        ws.ctrl->alpha = alpha;
        ws.ctrl->skip = skip ? 1 : 0;
        if (stats != nullptr) {
            stats[0] = (float)sqrt(G);
            stats[1] = (float)N;
            stats[2] = (float)NF;
            stats[3] = skip ? 1.f : 0.f;
            stats[4] = alpha;
            stats[5] = S;
            stats[6] = 0.f;
            stats[7] = 0.f;
        }
        S_sh = S;
    }
    __syncthreads();
    const float S = S_sh;
    for (int t = tid; t < T; t += FINISH_THREADS) {   // each thread: the tensors it wrote in pass 1
        const float sc_t = mul_rn(ws.scale[t], S);
        ws.scale[t] = sc_t;
        if (scales_out != nullptr) scales_out[t] = sc_t;
    }
}

struct StepArgs {
    float* p;
    const float* g;
    float* m;
    float* v;
    float* ema;
    const OptimSlab* slabs;
    long long num_slabs;
    const float* scale;
    const OptimCtrl* ctrl;
    float b1, b2, eps, cv, ema_momentum;
    bool vec;
};

// k_adam's update on g' = fl32(h * scale), then the EMA line. The compiler is free to contract a * b + c or not,
// and it chooses differently for the scalar and the packed form of the same expression; m and v must come out
// bit-equal to cnf_adam_step's on every path, so each operation is spelled out here as k_adam is built: the m line
// as a product and a sum, both v lines fused, nothing else fused.
template <bool EMA>
__device__ __forceinline__ void optim_elem(float& p, float g, float& m, float& v, float& e, float scale, float alpha,
                                           const StepArgs& a) {
#pragma clang fp contract(off)
    const float h = a.cv > 0.f ? fminf(fmaxf(g, -a.cv), a.cv) : g;
    const float gi = h * scale;
    const float mi = m + (gi - m) * (1.f - a.b1);
    const float vi = fmaf(fmaf(gi, gi, -v), 1.f - a.b2, v);
    m = mi;
    v = vi;
    p = p - alpha * mi / (sqrtf(vi) + a.eps);
    if (EMA) e = fmaf(p - e, 1.f - a.ema_momentum, e);
}

template <bool EMA>
__global__ __launch_bounds__(256) void k_optim_step(StepArgs a) {
    const OptimCtrl ctrl = *a.ctrl;
    if (ctrl.skip != 0) return;
    const float alpha = ctrl.alpha;
    const int tid = threadIdx.x;
    for (long long s = blockIdx.x; s < a.num_slabs; s += gridDim.x) {
        const OptimSlab e = a.slabs[s];
        const SlabParts sp = slab_parts(e, a.vec);
        const float scale = a.scale[e.tensor];
        float* __restrict__ p = a.p + e.start;
        const float* __restrict__ g = a.g + e.start;
        float* __restrict__ m = a.m + e.start;
        float* __restrict__ v = a.v + e.start;
        float* __restrict__ em = EMA ? a.ema + e.start : nullptr;
        auto scalar = [&](int i) {
            float pi = p[i], mi = m[i], vi = v[i], ei = EMA ? em[i] : 0.f;
            optim_elem<EMA>(pi, g[i], mi, vi, ei, scale, alpha, a);
            m[i] = mi;
            v[i] = vi;
            p[i] = pi;
            if (EMA) em[i] = ei;
        };
        for (int i = tid; i < sp.head; i += 256) scalar(i);
        for (int i = tid; i < sp.quads; i += 256) {
            const int o = sp.head + 4 * i;
            f4 pq = *reinterpret_cast<const f4*>(p + o);
            const f4 gq = *reinterpret_cast<const f4*>(g + o);
            f4 mq = *reinterpret_cast<const f4*>(m + o);
            f4 vq = *reinterpret_cast<const f4*>(v + o);
            f4 eq = {0.f, 0.f, 0.f, 0.f};
            if (EMA) eq = *reinterpret_cast<const f4*>(em + o);
#pragma unroll
            for (int u = 0; u < 4; u++) {
                float pi = pq[u], mi = mq[u], vi = vq[u], ei = eq[u];
                optim_elem<EMA>(pi, gq[u], mi, vi, ei, scale, alpha, a);
                pq[u] = pi;
                mq[u] = mi;
                vq[u] = vi;
                eq[u] = ei;
            }
            *reinterpret_cast<f4*>(m + o) = mq;
            *reinterpret_cast<f4*>(v + o) = vq;
            *reinterpret_cast<f4*>(p + o) = pq;
            if (EMA) *reinterpret_cast<f4*>(em + o) = eq;
        }
        for (int i = sp.tail + tid; i < e.count; i += 256) scalar(i);
    }
}

}  // namespace

void launch_optim(const OptimArgs& a, hipStream_t st) {
    const unsigned gx = (unsigned)std::min<long long>(a.num_slabs, 8192);
    hipLaunchKernelGGL(k_optim_stats, dim3(gx), dim3(256), 0, st, a.g, a.slabs, a.num_slabs, a.d.clipvalue, a.vec,
                       a.ws.sum_g, a.ws.sum_h, a.ws.nonfinite);
    hipLaunchKernelGGL(k_optim_finish, dim3(1), dim3(FINISH_THREADS), 0, st, a.first, a.T, a.d, a.ws, a.state, a.stats,
                       a.scales_out);
    StepArgs s;
    s.p = a.p;
    s.g = a.g;
    s.m = a.m;
    s.v = a.v;
    s.ema = a.ema;
    s.slabs = a.slabs;
    s.num_slabs = a.num_slabs;
    s.scale = a.ws.scale;
    s.ctrl = a.ws.ctrl;
    s.b1 = a.d.beta_1;
    s.b2 = a.d.beta_2;
    s.eps = a.d.epsilon;
    s.cv = a.d.clipvalue;
    s.ema_momentum = a.d.ema_momentum;
    s.vec = a.vec;
    if (a.ema != nullptr && a.d.ema_momentum > 0.f)
        hipLaunchKernelGGL(k_optim_step<true>, dim3(gx), dim3(256), 0, st, s);
    else
        hipLaunchKernelGGL(k_optim_step<false>, dim3(gx), dim3(256), 0, st, s);
}

}  // namespace cnf
