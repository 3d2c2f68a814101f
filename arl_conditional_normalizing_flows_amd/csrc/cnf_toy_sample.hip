// cnf_toy_sample.hip — posterior draws of the TOYcINN dense flow (cnf_toy_sample, include/cnf.h): the recipe of
// TOYcINN.py:807-817 (z from the prior, concatenate y, model(zy, direction=1)) and the statistics of the
// cloud per condition (:823-...), from latent to result in one launch.
//
//   k_toy_sample        one workgroup owns one tile of TOY_SAMPLE_TS consecutive draws of one condition. The
//                       tile's state [TS][3] lives in LDS from the Philox latent to the epilogue: no zy or
//                       xy_hat in global memory. Coupling layers run in direction +1 (index order,
//                       u2 = (v2 - b) / exp(tanh A), TOYcINN_make_model.py:370-375). Per layer and net the
//                       hidden activations ping-pong between two [TS][HP] LDS images; the H x H Dense layers
//                       run on v_mfma_f32_16x16x4_f32 (mma_tile, cnf_toy_device.h; bias = the accumulator's
//                       start, zero operands pad H to 16 / 4): a wave loads the B fragments of its 16-column
//                       tile from global memory (L2-resident weights) into registers once per Dense layer and
//                       reuses them over its row tiles, so per MFMA only the A element comes from LDS. The
//                       1- / 2-wide first and last Dense layers and the coupling law run on the vector ALUs
//                       in k_toy's fmaf order. An MFMA row is a dot product in a fixed k order and every
//                       vector-ALU step is per draw, so a draw's bits depend on (params, y[b], seed, stream
//                       index, temperature) alone. Epilogue per draw: samples, y_dev, the histogram count
//                       (integer atomics); per tile and component the shifted partial (n, K, S1, S2) in draw
//                       order (sample_fold, cnf_device.h).
//   k_toy_sample_stats  one wave per (condition, component): the tile partials merged in tile order in fp64,
//                       rounded once to mean / std (the formula: include/cnf.h). No atomics.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "cnf_device.h"
#include "cnf_toy_device.h"

namespace cnf {

namespace {

constexpr int TS = TOY_SAMPLE_TS;
constexpr int BT = 256;   // threads per workgroup (4 waves)
constexpr int NW = BT / 64;
constexpr int RT = TS / 16;   // 16-row tiles of a draw tile
static_assert(TS % 16 == 0 && TS <= BT, "one epilogue thread per draw");

}  // namespace

// KS: k steps of the H x H MFMA layers (H <= 4 KS), the bound of the B-fragment register array
template <int KS>
__global__ __launch_bounds__(BT) void k_toy_sample(ToySampleArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int H = a.flow.H, L = a.flow.L, HP = a.HP;
    float* act = sm;                   // [2][TS][HP] post-activation hidden vectors, ping-pong
    float* su = act + 2 * TS * HP;     // [TS][3] the draws' state: zy, then each layer's output, then xy_hat
    float* bo = su + 3 * TS;           // [TS][2] the b net's output
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int b = blockIdx.x / a.tiles, tile = blockIdx.x - b * a.tiles;
    const int s0 = tile * TS;
    const int cnt = a.S - s0 < TS ? a.S - s0 : TS;   // draws of this tile (>= 1); rows past them are zeros
    const int HT = (H + 15) / 16;
    const int yd = 3 - a.flow.x_d;
    const float* __restrict__ yb = a.y + (size_t)b * yd;
    const int fd_s = tid / H, fd_o = tid - fd_s * H;   // the first Dense's element walk: start and step of (s, o)
    const int fd_ds = BT / H, fd_do = BT - fd_ds * H;

    // latent: temperature * N(0,1) of stream element offset + (b S + s) x_d + c, then y[b]
    for (int e = tid; e < 3 * TS; e += BT) {
        const int s = e / 3, c = e - 3 * s;
        float v = 0.f;
        if (s < cnt) {
            if (c < a.flow.x_d) {
                const uint64_t g = (uint64_t)a.offset + ((uint64_t)b * (uint64_t)a.S + (uint64_t)(s0 + s)) * (uint64_t)a.flow.x_d + c;
                v = a.temperature * instance_noise_value(0.f, false, 0.f, (uint64_t)a.seed, g);
            } else {
                v = yb[c - a.flow.x_d];
            }
        }
        su[e] = v;
    }

    for (int step = 0; step < a.flow.nl; step++) {
        const int j = a.flow.order[step];
        const ToyMask m = toy_mask(j);   // u1 / u2 index sets (:149-163), as k_toy
        const int n1 = m.n1, n2 = m.n2;
        const int i1[2] = {m.i1[0], m.i1[1]}, i2[2] = {m.i2[0], m.i2[1]};
        const int net_floats = (a.flow.net_off[j + 1] - a.flow.net_off[j]) / 2;
        __syncthreads();   // su of the previous layer (or the latent) complete

        for (int net = 0; net < 2; net++) {   // b, then A
            const float* __restrict__ p = a.params + a.flow.net_off[j] + net * net_floats;
            const int off_hid = n1 * H + H;
            const int off_last = off_hid + L * (H * H + H);

            // first Dense on the vector ALUs (the fmaf order of k_toy)
            // (element e = s H + o for e = tid, tid + BT, ...: stepped without a division per element)
            for (int s = fd_s, o = fd_o; s < TS;) {
                float y = p[n1 * H + o];
                y = fmaf(su[3 * s + i1[0]], p[o], y);
                if (n1 > 1) y = fmaf(su[3 * s + i1[1]], p[H + o], y);
                act[s * HP + o] = toy_lrelu(y);
                s += fd_ds;
                o += fd_do;
                if (o >= H) {
                    o -= H;
                    s++;
                }
            }
            __syncthreads();
            // hidden Dense layers [TS x H][H x H] + bias: the wave's share of the HT x RT output tiles is a
            // run of the column-major tile list, so it changes its B fragments at most twice per layer
            for (int k = 1; k <= L; k++) {
                const float* __restrict__ W = p + off_hid + (k - 1) * (H * H + H);
                const float* __restrict__ bias = W + H * H;
                const float* in = act + ((k - 1) & 1) * TS * HP;
                float* out = act + (k & 1) * TS * HP;
                const int items = HT * RT, per = (items + NW - 1) / NW;
                int q = wave * per;
                const int qe = q + per < items ? q + per : items;
                while (q < qe) {
                    const int ct = q / RT, rt0 = q - ct * RT;
                    const int n = RT - rt0 < qe - q ? RT - rt0 : qe - q;
                    const int col = ct * 16 + (lane & 15);
                    float bf[KS];
#pragma unroll
                    for (int ks = 0; ks < KS; ks++) {
                        const int kk = 4 * ks + (lane >> 4);
                        bf[ks] = (kk < H && col < H) ? W[kk * H + col] : 0.f;
                    }
                    const float bz = col < H ? bias[col] : 0.f;
                    for (int r = 0; r < n; r++) {
                        const int rt = rt0 + r;
                        v4f acc = {bz, bz, bz, bz};
                        acc = mma_tile(
                            4 * KS, [&](int row, int kk) { return kk < H ? in[(rt * 16 + row) * HP + kk] : 0.f; },
                            [&](int kk, int) { return bf[kk >> 2]; }, acc);
                        if (col < H) {
#pragma unroll
                            for (int i = 0; i < 4; i++) out[(rt * 16 + (lane >> 4) * 4 + i) * HP + col] = toy_lrelu(acc[i]);
                        }
                    }
                    q += n;
                }
                __syncthreads();
            }
            // last Dense on the vector ALUs; the coupling law once both nets are known
            const float* hl = act + (L & 1) * TS * HP;
            const float* __restrict__ Wl = p + off_last;
            for (int e = tid; e < TS * n2; e += BT) {
                const int s = n2 == 2 ? e >> 1 : e, q = e - s * n2;
                float y = Wl[H * n2 + q];
                for (int k = 0; k < H; k++) y = fmaf(hl[s * HP + k], Wl[k * n2 + q], y);
                if (net == 0) {
                    bo[2 * s + q] = y;
                } else {
                    const float A = tanhf(y);
                    su[3 * s + i2[q]] = (su[3 * s + i2[q]] - bo[2 * s + q]) / expf(A);   // :370-375
                }
            }
            __syncthreads();
        }
    }
    __syncthreads();   // (nl == 0 is refused by the host; keeps the latent visible all the same)

    // epilogue: one thread per draw
    if (tid < cnt) {
        const int s = tid;
        const size_t g = (size_t)b * a.S + (size_t)(s0 + s);
        if (a.samples != nullptr)
            for (int c = 0; c < a.flow.x_d; c++) a.samples[g * a.flow.x_d + c] = su[3 * s + c];
        if (a.y_dev != nullptr) {
            float d = 0.f;
            for (int c = a.flow.x_d; c < 3; c++) d += fabsf(su[3 * s + c] - yb[c - a.flow.x_d]);
            a.y_dev[g] = d;
        }
        if (a.hist != nullptr) {
            // bin_c = (int)floorf((v_c - lo_c) * scale_c); counted only with every component inside [0, G)
            // (a NaN or an infinity fails the comparisons)
            bool in = true;
            size_t idx = (size_t)b;
            for (int c = 0; c < a.flow.x_d; c++) {
                const float w = floorf((su[3 * s + c] - a.lo[c]) * a.scale[c]);
                in = in && w >= 0.f && w < (float)a.G;
                idx = idx * (size_t)a.G + (size_t)(in ? (int)w : 0);
            }
            if (in) atomicAdd(a.hist + idx, 1u);
        }
    }
    // the tile's shifted partial per component, folded in draw order
    if (tid < a.flow.x_d) {
        const int c = tid;
        float K = 0.f, S1 = 0.f, S2 = 0.f;
#pragma unroll 8
        for (int s = 0; s < cnt; s++) sample_fold(su[3 * s + c], s == 0, K, S1, S2);
        float* dst = a.part + (((size_t)b * a.tiles + tile) * a.flow.x_d + c) * TOY_SAMPLE_PART;
        *reinterpret_cast<f4*>(dst) = f4{(float)cnt, K, S1, S2};
    }
}

// One wave per (b, c). Tile t's partial (n, K, S1, S2) gives, in fp64, its mean's offset from the first
// tile's shift K_0 and its centred second moment about its own K:
//   o_t = (K_t - K_0) + S1_t / n_t,   q_t = max(0, S2_t - S1_t (S1_t / n_t))
// The lanes compute (n_t, o_t, q_t) of 64 tiles at a time; lane 0 adds them up in tile order:
//   T = sum n_t o_t,  mean = K_0 + T / S,  M2 = sum (q_t + n_t (o_t - T / S)^2),  std = sqrt(max(0, M2 / S))
__global__ __launch_bounds__(64) void k_toy_sample_stats(const float* __restrict__ part, int tiles, int S, int x_d,
                                                         float* __restrict__ mean, float* __restrict__ std) {
    __shared__ double sn[64], so[64], sq[64];
    __shared__ double sh_o;
    const int lane = threadIdx.x;
    const int bc = blockIdx.x;   // b * x_d + c
    const int b = bc / x_d, c = bc - b * x_d;
    const float* __restrict__ p = part + ((size_t)b * tiles * x_d + c) * TOY_SAMPLE_PART;
    const size_t stride = (size_t)x_d * TOY_SAMPLE_PART;
    const double K0 = (double)p[1];
    double T = 0.0, M2 = 0.0, o = 0.0;
    for (int pass = 0; pass < 2; pass++) {
        for (int base = 0; base < tiles; base += 64) {
            const int t = base + lane;
            if (t < tiles) {
                const f4 v = *reinterpret_cast<const f4*>(p + (size_t)t * stride);
                const double n = (double)v[0], r = (double)v[2] / n;
                sn[lane] = n;
                so[lane] = ((double)v[1] - K0) + r;
                sq[lane] = fmax(0.0, (double)v[3] - (double)v[2] * r);
            }
            __syncthreads();
            if (lane == 0) {
                const int m = tiles - base < 64 ? tiles - base : 64;
                if (pass == 0) {
                    for (int i = 0; i < m; i++) T += sn[i] * so[i];
                } else {
                    for (int i = 0; i < m; i++) {
                        const double d = so[i] - o;
                        M2 += sq[i] + sn[i] * (d * d);
                    }
                }
            }
            __syncthreads();
        }
        if (pass == 0) {
            if (lane == 0) sh_o = T / (double)S;
            __syncthreads();
            o = sh_o;
        }
    }
    if (lane == 0) {
        if (mean != nullptr) mean[bc] = (float)(K0 + o);
        if (std != nullptr) std[bc] = (float)sqrt(fmax(0.0, M2 / (double)S));
    }
}

size_t toy_sample_lds_bytes(int H) { return ((size_t)2 * TS * toy_bwd_hp(H) + 5 * TS) * sizeof(float); }

void launch_toy_sample(const ToySampleArgs& a, hipStream_t st) {
    const dim3 g((unsigned)a.B * (unsigned)a.tiles), b(BT);
    const size_t lds = toy_sample_lds_bytes(a.flow.H);
    if (a.flow.H <= 16)
        hipLaunchKernelGGL(k_toy_sample<4>, g, b, lds, st, a);
    else if (a.flow.H <= 32)
        hipLaunchKernelGGL(k_toy_sample<8>, g, b, lds, st, a);
    else if (a.flow.H <= 48)
        hipLaunchKernelGGL(k_toy_sample<12>, g, b, lds, st, a);
    else
        hipLaunchKernelGGL(k_toy_sample<16>, g, b, lds, st, a);
}

void launch_toy_sample_stats(const float* part, int B, int tiles, int S, int x_d, float* mean, float* std,
                             hipStream_t st) {
    hipLaunchKernelGGL(k_toy_sample_stats, dim3((unsigned)(B * x_d)), dim3(64), 0, st, part, tiles, S, x_d, mean, std);
}

}  // namespace cnf
