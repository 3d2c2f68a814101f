// cnf_sample.hip — conditional sampling around the inverse (cnf_flow_sample, include/cnf.h): the recipe of
// TOYcINN.py:807-817 (z from the prior, concat the condition y, the model in the generative direction,
// conv_cINN_make_model.py:1774-1798) with its post-transforms and the statistics over the draws.
//   k_latent       one chunk of zy: temperature * N(0,1) on the x channels, y[b] on the rest
//   k_sample_fold  one pass over a chunk's xy_hat: post-transform, samples, running (K, S1, S2), mean / std
//   k_sample_ydev  per image sum |y_hat - y|
//   k_sample_logp  per image log-density of the draw: the prior's log N(z; 0, I) plus the inverse's log-det slots
//   k_sample_score      the draws against a truth per element: rank, mean |error|, histogram (cnf_flow_sample_score)
//   k_sample_sqerr      per image sum (sample - truth)^2
//   k_sample_quantiles  per element quantiles from the finished histogram
//   k_child_latent      one chunk of a cascade's child stage: `up` of the parent chunk's sample values on the y
//                       channels, k_latent's normals on the x channels (cnf_flow_sample_cascade)
//   k_block_dev         per image sum over 2x2 pixel blocks of |block mean of (sample - condition)|
// k_sample_fold, k_sample_ydev, k_sample_score and k_sample_sqerr are templates on where an image's condition
// comes from (NODE; DrawView, cnf_kernels.h).
// All HBM-bound element / reduction kernels; no global atomics (k_sample_score counts with integer LDS adds
// inside the tile its workgroup owns), every floating-point sum in a fixed order.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

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

// What a thread of k_sample_fold / k_sample_score owns. A workgroup owns FOLD_E elements (p, c) of one
// condition b of those the chunk touches (b0 .. b0 + nb - 1; bpc workgroups per condition); thread (e, l)
// takes the draws l, l + FOLD_L, ... of a batch (their loads in flight together: the draws are an image
// apart). The draws s0 .. s1 - 1 of b in the chunk are the same for the whole workgroup, so barriers inside
// the batch loop sit in uniform control flow.
// NODE: the residual's y is the draw's own condition, the y channel of its image of the chunk's zy, loaded
// next to the value; otherwise y[b]'s element, loaded once (D - x_d == x_d: y[b] has x's shape).
template <bool NODE>
struct FoldTile {
    static constexpr int NJ = FOLD_BATCH / FOLD_L;
    int per, e, l, pc0, pc, p, c, s0, s1;   // per: elements per condition
    long long b, gb;                        // the condition, its first image
    bool valid;
    size_t plane, se, img;   // the elements of a [B][HW][x_d] tensor (B given), this thread's; of an image
    const float *__restrict__ src, *__restrict__ ysrc;   // in image 0 of the chunk: the element, its condition
    float yv, w[NJ], yw[NODE ? NJ : 1];                  // y[b]'s value; the batch as loaded

    __device__ __forceinline__ FoldTile(const SampleChunk& q, const DrawView& v, long long b0, int bpc, int B = 0) {
        per = q.HW * q.x_d;
        b = b0 + blockIdx.x / bpc;
        e = threadIdx.x % FOLD_E, l = threadIdx.x / FOLD_E;
        pc0 = (blockIdx.x % bpc) * FOLD_E, pc = pc0 + e;
        valid = pc < per;
        p = pc / q.x_d, c = pc - p * q.x_d;
        gb = b * q.S;
        const long long g1 = q.g0 + q.n;
        s0 = (int)((q.g0 > gb ? q.g0 : gb) - gb);
        s1 = (int)((g1 < gb + q.S ? g1 : gb + q.S) - gb);
        plane = (size_t)B * per;
        se = (size_t)b * per + pc;
        yv = !NODE && v.residual && valid ? v.y[se] : 0.f;
    }
    // before the batch loop (after the kernel's own loads and barriers, where the kernels have always done it)
    __device__ __forceinline__ void sources(const SampleChunk& q, const DrawView& v) {
        img = (size_t)q.HW * q.D;
        src = v.xy_hat + (size_t)p * q.D + c;
        ysrc = NODE ? v.zy + (size_t)p * q.D + q.x_d + c : nullptr;
    }
    // the batch that starts at draw sb: every load first
    __device__ __forceinline__ void load(const SampleChunk& q, const DrawView& v, int sb) {
#pragma unroll
        for (int j = 0; j < NJ; j++) {
            const int s = sb + l + j * FOLD_L;
            w[j] = valid && s < s1 ? src[(size_t)(gb + s - q.g0) * img] : 0.f;   // (s >= s0: image gb + s - g0 >= 0)
            if constexpr (NODE) yw[j] = v.residual && valid && s < s1 ? ysrc[(size_t)(gb + s - q.g0) * img] : 0.f;
        }
    }
    // the sample value of the batch's draw sb + l + j * FOLD_L
    __device__ __forceinline__ float value(const DrawView& v, int j) const {
        return sample_post_value(w[j], v.logit, v.lk, v.residual, NODE ? yw[j] : yv);
    }
};

// The post-transform of a value does not depend on the other draws, so all 256 threads apply it, store the
// sample and leave the value in LDS; the fold is a serial chain per element, three operations a draw, which
// thread (e, 0) runs over the batch in draw order.
template <bool NODE>
__global__ __launch_bounds__(256) void k_sample_fold(SampleChunk q, SampleFoldArgs a, long long b0, int bpc) {
    __shared__ float sh[FOLD_BATCH][FOLD_E];
    FoldTile<NODE> t(q, a.v, b0, bpc, a.B);
    const size_t plane = t.plane;   // state: [3][B][HW][x_d]
    const size_t se = t.se;
    const bool stats = a.state != nullptr;
    const bool folds = stats && t.valid && t.l == 0;
    float K = 0.f, S1 = 0.f, S2 = 0.f;
    if (folds && t.s0 > 0) {
        K = a.state[se];
        S1 = a.state[plane + se];
        S2 = a.state[2 * plane + se];
    }
    t.sources(q, a.v);
    for (int sb = t.s0; sb < t.s1; sb += FOLD_BATCH) {
        t.load(q, a.v, sb);
#pragma unroll
        for (int j = 0; j < t.NJ; j++) {
            const int s = sb + t.l + j * FOLD_L;
            const float v = t.value(a.v, j);
            if (t.valid && s < t.s1 && a.samples != nullptr) a.samples[(size_t)(t.gb + s) * t.per + t.pc] = v;
            if (stats) sh[t.l + j * FOLD_L][t.e] = v;
        }
        if (!stats) continue;
        __syncthreads();
        if (folds) {
            const int nk = t.s1 - sb < FOLD_BATCH ? t.s1 - sb : FOLD_BATCH;
#pragma unroll 8
            for (int k = 0; k < nk; k++) sample_fold(sh[k][t.e], sb + k == 0, K, S1, S2);
        }
        __syncthreads();
    }
    if (!folds) return;
    if (t.s1 < q.S) {
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

// The wave-per-image kernels: one wave per image of the chunk (whole waves past it leave); lane sums in fp64 over
// the image's elements in order, then the wave sum: wave_image_sum (cnf_device.h) of a term per element in
// k_sample_logp and k_block_dev; k_sample_ydev and k_sample_sqerr spell the same loop out, because through the
// helper the compiler schedules their prologues differently. The wave's image:
__device__ __forceinline__ int wave_image() { return blockIdx.x * 4 + (threadIdx.x >> 6); }

// y_dev: |y_hat - condition| over the image's HW * (D - x_d) condition elements
template <bool NODE>
__global__ __launch_bounds__(256) void k_sample_ydev(SampleChunk q, DrawView v, float* __restrict__ y_dev) {
    const int lane = threadIdx.x & 63, i = wave_image();
    if (i >= q.n) return;
    const long long g = q.g0 + i;
    const long long b = g / q.S;
    const int yd = q.D - q.x_d, n = q.HW * yd;
    const float* __restrict__ xi = v.xy_hat + (size_t)i * q.HW * q.D;
    const float* __restrict__ yb = NODE ? v.zy + (size_t)i * q.HW * q.D : v.y + (size_t)b * n;
    double s = 0.0;
    for (int e = lane; e < n; e += 64) {
        const int p = e / yd, c = e - p * yd;
        const float yv = NODE ? yb[(size_t)p * q.D + q.x_d + c] : yb[e];
        s += (double)fabsf(xi[(size_t)p * q.D + q.x_d + c] - yv);
    }
    s = wave_sum(s);
    if (lane == 0) y_dev[g] = (float)s;
}

// log_prob[g] = log N(z; 0, I) + sum over couplings of sum s, from the chunk's latent (the x channels of zy as
// stored) and the log-det partial slots part[nl][n][np] the chunk's inverse left in its workspace. q = sum z^2
// over the image's HW * x_d latent elements; L: the slots in k_ld_reduce's order (ld_slot_sum).
__global__ __launch_bounds__(256) void k_sample_logp(SampleChunk q, const float* __restrict__ zy,
                                                     const double* __restrict__ part, int nl, int np,
                                                     float* __restrict__ log_prob) {
    const int lane = threadIdx.x & 63, i = wave_image();
    if (i >= q.n) return;
    const int n = q.HW * q.x_d;
    const float* __restrict__ zi = zy + (size_t)i * q.HW * q.D;
    const double s = wave_image_sum(n, lane, [=](int e) {
        const int p = e / q.x_d, c = e - p * q.x_d;
        const double z = (double)zi[(size_t)p * q.D + c];
        return z * z;
    });
    const double L = ld_slot_sum(part, q.n, i, nl, np, lane);
    if (lane == 0) log_prob[q.g0 + i] = (float)(-0.5 * s - 0.5 * (double)n * LOG_2PI_D + L);
}

// k_sample_score's LDS: the histogram tile [bins][SCORE_EP], a bin's FOLD_E counters side by side and one pad
// word per row (the adds of a half wave go to FOLD_E different banks whatever their bins, and the write-out,
// which walks the tile in the output's [element][bin] order, meets a bank twice at the most); then the batch's
// values [FOLD_BATCH][FOLD_E] for the serial abs_err fold and the draw lanes' counts [FOLD_L][FOLD_E]
constexpr int SCORE_EP = FOLD_E + 1;
size_t score_lds_bytes(int bins) { return ((size_t)bins * SCORE_EP + FOLD_BATCH * FOLD_E + FOLD_L * FOLD_E) * 4; }

// k_sample_fold's ownership and batches (FoldTile). Every thread (e, l) counts its draws of a batch
// below the truth and adds their bins to the LDS tile (integer LDS adds: order-free);
// thread (e, 0) folds |v - truth| over the batch in draw order. The chunk's counts then go to the outputs,
// which the workgroup owns: added to what the earlier chunks left there, or stored when the chunk holds
// b's first draw. s0, s1 and the null tests are the same for the whole workgroup: the barriers are uniform.
template <bool NODE>
__global__ __launch_bounds__(256) void k_sample_score(SampleChunk q, SampleScoreArgs a, long long b0, int bpc) {
    extern __shared__ __align__(16) int score_lds[];
    int* hs = score_lds;
    float* sh = reinterpret_cast<float*>(score_lds + a.bins * SCORE_EP);
    int* rk = score_lds + a.bins * SCORE_EP + FOLD_BATCH * FOLD_E;
    FoldTile<NODE> t(q, a.v, b0, bpc);
    const int per = t.per, e = t.e, l = t.l, pc0 = t.pc0, s1 = t.s1;
    const bool valid = t.valid;
    const long long b = t.b;
    const bool first = t.s0 == 0;
    const size_t se = t.se;
    const bool owner = valid && l == 0;
    const bool errs = a.abs_err != nullptr, hist = a.hist != nullptr;
    const float tv = a.truth != nullptr && valid ? a.truth[se] : 0.f;
    float acc = errs && owner && !first ? a.abs_err[se] : 0.f;
    int below = 0;
    if (hist) {
        for (int i = threadIdx.x; i < a.bins * SCORE_EP; i += 256) hs[i] = 0;
        __syncthreads();
    }
    t.sources(q, a.v);
    for (int sb = t.s0; sb < s1; sb += FOLD_BATCH) {
        t.load(q, a.v, sb);
#pragma unroll
        for (int j = 0; j < t.NJ; j++) {
            const int s = sb + l + j * FOLD_L;
            const float v = t.value(a.v, j);
            if (valid && s < s1) {
                below += v < tv ? 1 : 0;
                if (hist) {
                    // k_toy_sample's expression; a NaN or an infinity fails the comparisons
                    const float k = floorf((v - a.lo) * a.scale);
                    if (k >= 0.f && k < (float)a.bins) atomicAdd(&hs[(int)k * SCORE_EP + e], 1);
                }
            }
            if (errs) sh[(l + j * FOLD_L) * FOLD_E + e] = v;
        }
        if (!errs) continue;
        __syncthreads();
        if (owner) {
            const int nk = s1 - sb < FOLD_BATCH ? s1 - sb : FOLD_BATCH;
#pragma unroll 8
            for (int k = 0; k < nk; k++) acc += fabsf(sh[k * FOLD_E + e] - tv);
        }
        __syncthreads();
    }
    if (errs && owner) a.abs_err[se] = s1 < q.S ? acc : acc / (float)q.S;
    if (a.rank != nullptr) {
        rk[l * FOLD_E + e] = below;
        __syncthreads();
        if (owner) {
            int r = first ? 0 : a.rank[se];
#pragma unroll
            for (int k = 0; k < FOLD_L; k++) r += rk[k * FOLD_E + e];
            a.rank[se] = r;
        }
    }
    if (!hist) return;
    __syncthreads();
    // the tile's elements pc0 .. pc0 + ne - 1 are ne * bins consecutive counters of the output
    const int ne = per - pc0 < FOLD_E ? per - pc0 : FOLD_E;
    int* __restrict__ out = a.hist + ((size_t)b * per + pc0) * a.bins;
    for (int i = threadIdx.x; i < ne * a.bins; i += 256) {
        const int ee = i / a.bins, k = i - ee * a.bins;
        int h = hs[k * SCORE_EP + ee];
        if (!first) h += out[i];
        out[i] = h;
    }
}

// sq_err: (sample value - truth)^2 over the image's HW * x_d elements
template <bool NODE>
__global__ __launch_bounds__(256) void k_sample_sqerr(SampleChunk q, SampleSqerrArgs a) {
    const int lane = threadIdx.x & 63, i = wave_image();
    if (i >= q.n) return;
    const long long g = q.g0 + i;
    const long long b = g / q.S;
    const int n = q.HW * q.x_d;
    const float* __restrict__ xi = a.v.xy_hat + (size_t)i * q.HW * q.D;
    const float* __restrict__ tb = a.truth + (size_t)b * n;
    // (read with residual only: y[b] has x's shape)
    const float* __restrict__ yb = NODE ? a.v.zy + (size_t)i * q.HW * q.D : a.v.y + (size_t)b * n;
    double s = 0.0;
    for (int e = lane; e < n; e += 64) {
        const int p = e / q.x_d, c = e - p * q.x_d;
        const float yv = a.v.residual ? (NODE ? yb[(size_t)p * q.D + q.x_d + c] : yb[e]) : 0.f;
        const float v = sample_post_value(xi[(size_t)p * q.D + c], a.v.logit, a.v.lk, a.v.residual, yv);
        const double d = (double)v - (double)tb[e];
        s += d * d;
    }
    s = wave_sum(s);
    if (lane == 0) a.sq_err[g] = (float)s;
}

// One thread per element: N, then one walk over the bins that serves every level. Level q's bin is the first
// with cumulative count C_k >= q N and C_k > 0 (so hist[k] > 0), its value the point of that bin where a
// uniform spread of the bin's draws reaches q N; clamped to [lo, hi], which only the rounding of the
// edges can leave. q <= 1 keeps q N <= N, so every level is met at the last occupied bin at the latest.
__global__ __launch_bounds__(256) void k_sample_quantiles(SampleQuantileArgs a) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (long long)gridDim.x * 256) {
        const int* __restrict__ h = a.hist + (size_t)i * a.bins;
        int N = 0;
        for (int k = 0; k < a.bins; k++) N += h[k];
        if (N == 0) {
            for (int j = 0; j < a.nq; j++) a.quantiles[(size_t)j * a.n + i] = __builtin_nanf("");
            continue;
        }
        float target[SCORE_MAX_QUANTILES];
#pragma unroll
        for (int j = 0; j < SCORE_MAX_QUANTILES; j++) target[j] = a.q[j] * (float)N;
        unsigned done = 0;
        int C = 0;
        for (int k = 0; k < a.bins; k++) {
            const int hk = h[k];
            if (hk == 0) continue;
#pragma unroll
            for (int j = 0; j < SCORE_MAX_QUANTILES; j++) {
                if (j < a.nq && !(done >> j & 1u) && (float)(C + hk) >= target[j]) {
                    const float v = a.lo + ((float)k + (target[j] - (float)C) / (float)hk) * (a.hi - a.lo) / (float)a.bins;
                    a.quantiles[(size_t)j * a.n + i] = fminf(fmaxf(v, a.lo), a.hi);
                    done |= 1u << j;
                }
            }
            C += hk;
        }
    }
}

// k_latent's threads and stores for one chunk of a child stage of a cascade. The x channels: k_latent's
// normal. A y channel cy: the parent's sample value at pixel (h / 2, w / 2) -- the parent chunk's draw through
// its view, with the parent's own condition -- i.e. cnf_up of the value k_sample_fold would have stored for the
// parent, which is never written. D == 2 x_d.
template <bool VEC>
__global__ __launch_bounds__(256) void k_child_latent(SampleChunk q, ChildLatentArgs a) {
    constexpr int V = VEC ? 4 : 1;
    const int units = q.D / V;   // per pixel
    const int pW = a.W / 2;
    const size_t pimg = (size_t)(q.HW / 4) * q.D;   // a parent image
    const long long n = (long long)q.n * q.HW * units;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
        const int cu = (int)(e % units);
        const long long ip = e / units;   // (image of the chunk, pixel)
        const int p = (int)(ip % q.HW);
        const long long g = q.g0 + ip / q.HW;
        const int h = p / a.W, w = p - h * a.W;
        // the parent's image in its chunk (g / Sc >= pg0: the chunk holds children of that chunk's nodes only)
        const size_t pe = (size_t)(g / a.Sc - a.pg0) * pimg + (size_t)((h / 2) * pW + w / 2) * q.D;
        const uint64_t z0 = a.offset + ((uint64_t)g * q.HW + p) * q.x_d;
        float v[V];
#pragma unroll
        for (int j = 0; j < V; j++) {
            const int c = cu * V + j;
            if (c < q.x_d) {
                v[j] = a.temperature * instance_noise_value(0.f, false, 0.f, a.seed, z0 + c);
            } else {
                const int cy = c - q.x_d;
                const float yv = a.parent.residual ? a.parent.zy[pe + q.x_d + cy] : 0.f;
                v[j] = sample_post_value(a.parent.xy_hat[pe + cy], a.parent.logit, a.parent.lk, a.parent.residual, yv);
            }
        }
        if constexpr (VEC)
            *reinterpret_cast<f4*>(a.zy + (size_t)e * 4) = f4{v[0], v[1], v[2], v[3]};
        else
            a.zy[e] = v[0];
    }
}

// block_dev over the image's (2x2 block, channel) elements. An element: the four pixels of the block in
// row-major order, each (double)v - (double)y (exact), added in that order, times 0.25 (exact), its absolute value.
__global__ __launch_bounds__(256) void k_block_dev(SampleChunk q, BlockDevArgs a) {
    const int lane = threadIdx.x & 63, i = wave_image();
    if (i >= q.n) return;
    const int bw = a.W / 2, n = (q.HW / 4) * q.x_d;
    const float* __restrict__ xi = a.v.xy_hat + (size_t)i * q.HW * q.D;
    const float* __restrict__ zi = a.v.zy + (size_t)i * q.HW * q.D;
    const double s = wave_image_sum(n, lane, [=](int e) {
        const int blk = e / q.x_d, c = e - blk * q.x_d;
        const int bh = blk / bw, bx = blk - bh * bw;
        double d = 0.0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const size_t o = (size_t)((2 * bh + (k >> 1)) * a.W + 2 * bx + (k & 1)) * q.D + c;
            const float yv = zi[o + q.x_d];
            const float v = sample_post_value(xi[o], a.v.logit, a.v.lk, a.v.residual, yv);
            d += (double)v - (double)yv;
        }
        return fabs(0.25 * d);
    });
    if (lane == 0) a.block_dev[q.g0 + i] = (float)s;
}

int grid_for(long long n) {
    const long long g = (n + 255) / 256;
    return (int)(g < 1 ? 1 : (g > 65536 ? 65536 : g));
}

// The one dispatch on a view's source: f(std::true_type) for the image's own zy (NODE), f(std::false_type) for
// the table y[b]. The two instantiations of a kernel stay separate kernels.
template <class F>
void by_source(const DrawView& v, F f) {
    v.node() ? f(std::true_type{}) : f(std::false_type{});
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
    by_source(a.v, [&](auto node) {
        CNF_LAUNCH(k_sample_fold<decltype(node)::value>, dim3((unsigned)nb * bpc), dim3(256), 0, st, c, a, b0, bpc);
    });
}

void launch_sample_ydev(const SampleChunk& c, const DrawView& v, float* y_dev, hipStream_t st) {
    by_source(v, [&](auto node) {
        CNF_LAUNCH(k_sample_ydev<decltype(node)::value>, dim3((c.n + 3) / 4), dim3(256), 0, st, c, v, y_dev);
    });
}

void launch_sample_logp(const SampleChunk& c, const float* zy, const double* ld_part, int nl, int np, float* log_prob,
                        hipStream_t st) {
    CNF_LAUNCH(k_sample_logp, dim3((c.n + 3) / 4), dim3(256), 0, st, c, zy, ld_part, nl, np, log_prob);
}

void launch_sample_score(const SampleChunk& c, const SampleScoreArgs& a, hipStream_t st) {
    const long long b0 = c.g0 / c.S, b1 = (c.g0 + c.n - 1) / c.S;
    const int nb = (int)(b1 - b0 + 1);
    const int bpc = (c.HW * c.x_d + FOLD_E - 1) / FOLD_E;   // workgroups per condition
    by_source(a.v, [&](auto node) {
        CNF_LAUNCH(k_sample_score<decltype(node)::value>, dim3((unsigned)nb * bpc), dim3(256), score_lds_bytes(a.bins), st, c, a,
                   b0, bpc);
    });
}

void launch_sample_sqerr(const SampleChunk& c, const SampleSqerrArgs& a, hipStream_t st) {
    by_source(a.v, [&](auto node) {
        CNF_LAUNCH(k_sample_sqerr<decltype(node)::value>, dim3((c.n + 3) / 4), dim3(256), 0, st, c, a);
    });
}

void launch_sample_quantiles(const SampleQuantileArgs& a, hipStream_t st) {
    CNF_LAUNCH(k_sample_quantiles, dim3(grid_for(a.n)), dim3(256), 0, st, a);
}

void launch_child_latent(const SampleChunk& c, const ChildLatentArgs& a, hipStream_t st) {
    if (c.D % 4 == 0) {
        const long long n = (long long)c.n * c.HW * (c.D / 4);
        CNF_LAUNCH(k_child_latent<true>, dim3(grid_for(n)), dim3(256), 0, st, c, a);
    } else {
        const long long n = (long long)c.n * c.HW * c.D;
        CNF_LAUNCH(k_child_latent<false>, dim3(grid_for(n)), dim3(256), 0, st, c, a);
    }
}

void launch_block_dev(const SampleChunk& c, const BlockDevArgs& a, hipStream_t st) {
    CNF_LAUNCH(k_block_dev, dim3((c.n + 3) / 4), dim3(256), 0, st, c, a);
}

}  // namespace cnf
