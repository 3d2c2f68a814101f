// cnf_toy_train.hip — backward of the TOYcINN dense flow (TOYcINN_make_model.py:453-481 train_step,
// the GradientTape over log_loss :404-451), the counterpart of k_toy in direction -1.
//
//   k_toy_bwd       one workgroup owns TOY_TS consecutive samples and walks the coupling layers in the
//                   reverse of the order the forward executed them. Per layer both nets (b, then A)
//                   are recomputed from the layer input k_toy saved; a net's hidden activations
//                   ((L+1) x TS x H) stay in LDS while it is back-propagated. The H x H Dense layers
//                   run on v_mfma_f32_16x16x4_f32 (exact fp32 products; mma_tile, cnf_toy_device.h): the recompute
//                   [TS x H][H x H], the data gradient [TS x H][H x H]^T and the weight gradient
//                   [(H+1) x TS][TS x H], whose row H is a row of ones (the bias gradient, which
//                   follows the kernel in the canonical parameter order). The 1- and 2-wide first and
//                   last Dense layers run on the vector ALUs. Weights are read from global memory
//                   (they stay in L2). Edges (H not a multiple of 16 or 4, a last tile with fewer
//                   than TS samples) are zero operands. Every workgroup writes one full partial
//                   gradient row [num_params]; no atomics.
//   k_toy_grad_sum  dparams[i] = sum over tiles, in tile order, of part[tile][i] (fp64 sum):
//                   overwrites dparams; bitwise reproducible.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "cnf_kernels.h"
#include "cnf_toy_device.h"

namespace cnf {

namespace {

constexpr int TS = TOY_TS;
constexpr int BT = 256;          // threads per workgroup (4 waves)
constexpr int NW = BT / 64;
constexpr int SMALL_FLOATS = 3 * TS + 3 * TS + 2 * TS + 4 * TS;   // su, dv, dout, d1[2]

// LeakyReLU'(pre) from the stored post-activation value: h > 0 <=> pre > 0 (alpha > 0); 1 if pre > 0
// else alpha, as TF
__device__ __forceinline__ float lrelu_dh(float h) { return h > 0.f ? 1.f : LRELU_ALPHA; }

struct Net {
    const float* p;   // the net's parameters (global)
    float* gp;        // the net's slice of this tile's partial gradient row (global)
};

}  // namespace

__global__ __launch_bounds__(BT) void k_toy_bwd(ToyBwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int H = a.flow.H, L = a.flow.L, HP = a.HP;
    float* act = sm;                              // [L+1][TS][HP] post-activation hidden vectors
    float* gb = act + (size_t)(L + 1) * TS * HP;  // [2][TS][HP] d loss / d pre-activation, ping-pong
    float* su = gb + 2 * TS * HP;                 // [TS][3] the layer's input u
    float* dv = su + 3 * TS;                      // [TS][3] d loss / d (the layer's output), then input
    float* dout = dv + 3 * TS;                    // [TS][2] d loss / d (the net's output)
    float* d1 = dout + 2 * TS;                    // [2][TS][2] the two nets' input gradients
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int s0 = blockIdx.x * TS;
    const int HT = (H + 15) / 16;                 // 16-wide tiles across a hidden vector
    const int K4 = (H + 3) & ~3;
    float* part = a.part + (size_t)blockIdx.x * a.num_params;

    // seed (log_loss :404-451): d/dz = z, d/dy = lambda_y sign(y - y'), all times inv_batch; rows
    // past the batch are zero operands
    for (int e = tid; e < 3 * TS; e += BT) {
        const int s = e / 3, c = e - 3 * s;
        float g = 0.f;
        if (s0 + s < a.B) {
            const float z = a.zy[(size_t)(s0 + s) * 3 + c];
            if (c < a.flow.x_d) {
                g = z;
            } else {
                const float d = z - a.xy[(size_t)(s0 + s) * 3 + c];
                g = a.lambda_y * (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f));
            }
            g *= a.inv_batch;
        }
        dv[e] = g;
    }

    for (int step = a.flow.nl - 1; step >= 0; step--) {
        const int j = a.flow.order[a.flow.nl - 1 - step];
        const ToyMask m = toy_mask(j);   // u1 / u2 index sets (:149-163), as k_toy
        const int n1 = m.n1, n2 = m.n2;
        const int i1[2] = {m.i1[0], m.i1[1]}, i2[2] = {m.i2[0], m.i2[1]};
        const int net_floats = (a.flow.net_off[j + 1] - a.flow.net_off[j]) / 2;
        __syncthreads();   // dv of the previous layer complete; su free
        for (int e = tid; e < 3 * TS; e += BT) {
            const int s = e / 3;
            su[e] = s0 + s < a.B ? a.saved_u[((size_t)step * a.B + s0 + s) * 3 + (e - 3 * s)] : 0.f;
        }
        __syncthreads();

        for (int net = 0; net < 2; net++) {   // b, then A
            const float* p = a.params + a.flow.net_off[j] + net * net_floats;
            float* gp = part + a.flow.net_off[j] + net * net_floats;
            const int off_hid = n1 * H + H;                       // first hidden Dense
            const int off_last = off_hid + L * (H * H + H);       // last Dense: kernel [H][n2], bias [n2]

            // ---- recompute: first Dense on the vector ALUs (the fmaf order of k_toy)
            for (int e = tid; e < TS * H; e += BT) {
                const int s = e / H, o = e - s * H;
                float y = p[n1 * H + o];
                y = fmaf(su[3 * s + i1[0]], p[o], y);
                if (n1 > 1) y = fmaf(su[3 * s + i1[1]], p[H + o], y);
                act[s * HP + o] = toy_lrelu(y);
            }
            __syncthreads();
            // ---- recompute: hidden Dense layers, [TS x H][H x H] + bias
            for (int k = 1; k <= L; k++) {
                const float* W = p + off_hid + (k - 1) * (H * H + H);
                const float* bias = W + H * H;
                const float* in = act + (size_t)(k - 1) * TS * HP;
                float* out = act + (size_t)k * TS * HP;
                for (int tile = wave; tile < (TS / 16) * HT; tile += NW) {
                    const int rt = tile / HT, ct = tile - rt * HT;
                    const int col = ct * 16 + (lane & 15);
                    const float bz = col < H ? bias[col] : 0.f;
                    v4f acc = {bz, bz, bz, bz};
                    acc = mma_tile(
                        K4, [&](int r, int kk) { return kk < H ? in[(rt * 16 + r) * HP + kk] : 0.f; },
                        [&](int kk, int c) { return (kk < H && ct * 16 + c < H) ? W[kk * H + ct * 16 + c] : 0.f; }, acc);
                    if (col < H) {
#pragma unroll
                        for (int r = 0; r < 4; r++) out[(rt * 16 + (lane >> 4) * 4 + r) * HP + col] = toy_lrelu(acc[r]);
                    }
                }
                __syncthreads();
            }
            // ---- the net's output gradient; the coupling law v2 = exp(tanh a) u2 + b, logdet += tanh a
            const float* hl = act + (size_t)L * TS * HP;
            const float* Wl = p + off_last;
            for (int e = tid; e < TS * n2; e += BT) {
                const int s = e / n2, q = e - s * n2;
                const float dv2 = dv[3 * s + i2[q]];
                float d = dv2;   // db = dv2
                if (net == 1) {
                    float y = Wl[H * n2 + q];
                    for (int k = 0; k < H; k++) y = fmaf(hl[s * HP + k], Wl[k * n2 + q], y);
                    const float A = tanhf(y);
                    const float eA = expf(A);
                    const float dld = s0 + s < a.B ? -a.inv_batch : 0.f;
                    d = (dv2 * eA * su[3 * s + i2[q]] + dld) * (1.f - A * A);
                    dv[3 * s + i2[q]] = dv2 * eA;   // du2 (only this thread touches the element here)
                }
                dout[2 * s + q] = d;
            }
            __syncthreads();
            // ---- last Dense: weight + bias gradient (row H = ones), data gradient
            for (int e = tid; e < (H + 1) * n2; e += BT) {
                const int k = e / n2, q = e - k * n2;
                float acc = 0.f;
                for (int s = 0; s < TS; s++) acc = fmaf(k < H ? hl[s * HP + k] : 1.f, dout[2 * s + q], acc);
                gp[off_last + e] = acc;
            }
            for (int e = tid; e < TS * H; e += BT) {
                const int s = e / H, k = e - s * H;
                float acc = dout[2 * s] * Wl[k * n2];
                if (n2 > 1) acc = fmaf(dout[2 * s + 1], Wl[k * n2 + 1], acc);
                gb[s * HP + k] = acc * lrelu_dh(hl[s * HP + k]);
            }
            __syncthreads();
            // ---- hidden Dense layers, last to first
            int cur = 0;
            for (int k = L; k >= 1; k--) {
                const float* W = p + off_hid + (k - 1) * (H * H + H);
                float* gW = gp + off_hid + (k - 1) * (H * H + H);
                const float* in = act + (size_t)(k - 1) * TS * HP;
                const float* dy = gb + cur * TS * HP;
                float* dx = gb + (1 - cur) * TS * HP;
                const int RT = H / 16 + 1;   // row tiles of the [(H+1) x H] weight + bias gradient
                const int nwg = RT * HT, ndx = (TS / 16) * HT;
                for (int tile = wave; tile < nwg + ndx; tile += NW) {
                    v4f acc = {0.f, 0.f, 0.f, 0.f};
                    if (tile < nwg) {
                        // dW[i][o] = sum_s in[s][i] dy[s][o], i == H: the row of ones
                        const int rt = tile / HT, ct = tile - rt * HT;
                        acc = mma_tile(
                            TS,
                            [&](int r, int s) {
                                const int i = rt * 16 + r;
                                return i < H ? in[s * HP + i] : (i == H ? 1.f : 0.f);
                            },
                            [&](int s, int c) { return ct * 16 + c < H ? dy[s * HP + ct * 16 + c] : 0.f; }, acc);
                        const int col = ct * 16 + (lane & 15);
#pragma unroll
                        for (int r = 0; r < 4; r++) {
                            const int i = rt * 16 + (lane >> 4) * 4 + r;
                            if (i <= H && col < H) gW[i * H + col] = acc[r];
                        }
                    } else {
                        // dx[s][i] = (sum_o dy[s][o] W[i][o]) LeakyReLU'(in[s][i])
                        const int t2 = tile - nwg;
                        const int rt = t2 / HT, ct = t2 - rt * HT;
                        acc = mma_tile(
                            K4, [&](int r, int o) { return o < H ? dy[(rt * 16 + r) * HP + o] : 0.f; },
                            [&](int o, int c) { return (o < H && ct * 16 + c < H) ? W[(ct * 16 + c) * H + o] : 0.f; }, acc);
                        const int col = ct * 16 + (lane & 15);
                        if (col < H) {
#pragma unroll
                            for (int r = 0; r < 4; r++) {
                                const int s = rt * 16 + (lane >> 4) * 4 + r;
                                dx[s * HP + col] = acc[r] * lrelu_dh(in[s * HP + col]);
                            }
                        }
                    }
                }
                cur = 1 - cur;
                __syncthreads();
            }
            // ---- first Dense: weight + bias gradient (row n1 = ones), input gradient
            const float* dy0 = gb + cur * TS * HP;
            for (int e = tid; e < (n1 + 1) * H; e += BT) {
                const int k = e / H, o = e - k * H;
                float acc = 0.f;
                for (int s = 0; s < TS; s++) acc = fmaf(k < n1 ? su[3 * s + i1[k]] : 1.f, dy0[s * HP + o], acc);
                gp[e] = acc;
            }
            for (int e = tid; e < TS * n1; e += BT) {
                const int s = e / n1, k = e - s * n1;
                float acc = 0.f;
                for (int o = 0; o < H; o++) acc = fmaf(dy0[s * HP + o], p[k * H + o], acc);
                d1[(net * TS + s) * 2 + k] = acc;
            }
            __syncthreads();
        }
        // du1 = dv1 + the b net's input gradient + the A net's, in this order
        for (int e = tid; e < TS * n1; e += BT) {
            const int s = e / n1, k = e - s * n1;
            dv[3 * s + i1[k]] = (dv[3 * s + i1[k]] + d1[s * 2 + k]) + d1[(TS + s) * 2 + k];
        }
    }
}

int toy_bwd_hp(int H) { return (H + 31) / 32 * 32 + 4; }   // stride = 4 mod 32: the MFMA A reads spread over the banks

size_t toy_bwd_lds_bytes(int H, int L) {
    return ((size_t)(L + 3) * TS * toy_bwd_hp(H) + SMALL_FLOATS) * sizeof(float);
}

void launch_toy_bwd(const ToyBwdArgs& a, hipStream_t st) {
    const int tiles = (int)toy_tiles(a.B, TS);
    hipLaunchKernelGGL(k_toy_bwd, dim3(tiles), dim3(BT), toy_bwd_lds_bytes(a.flow.H, a.flow.L), st, a);
}

__global__ __launch_bounds__(256) void k_toy_grad_sum(const float* __restrict__ part, int tiles, int n,
                                                      float* __restrict__ dparams) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int t = 0; t < tiles; t++) s += (double)part[(size_t)t * n + i];
    dparams[i] = (float)s;
}

void launch_toy_grad_sum(const float* part, int tiles, int num_params, float* dparams, hipStream_t st) {
    hipLaunchKernelGGL(k_toy_grad_sum, dim3((num_params + 255) / 256), dim3(256), 0, st, part, tiles, num_params, dparams);
}

}  // namespace cnf
