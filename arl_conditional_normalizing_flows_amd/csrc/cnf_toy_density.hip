// cnf_toy_density.hip — the exact density of the TOYcINN dense flow on a grid or at given points
// (cnf_toy_density, include/cnf.h): log p(x | y) = log N(z; 0, I_xd) + log|det J| of the map xy -> zy
// (direction -1), from the point to its log-density in one launch.
//
//   k_toy_density       one workgroup owns one tile of TOY_SAMPLE_TS consecutive points of one condition. The
//                       tile's state [TS][3] lives in LDS from the prologue (a grid's bin centres, computed,
//                       or x, read; then y[b]) to the epilogue: no [B N, 3] input and no zy in global memory.
//                       Coupling layers run in direction -1 (reverse index order, u2 = exp(tanh A) u2 + b,
//                       ld += sum tanh A: k_toy's law). The structure is k_toy_sample's: per layer and net the
//                       hidden activations ping-pong between two [TS][HP] LDS images; the H x H Dense layers
//                       run on v_mfma_f32_16x16x4_f32 (mma_tile, cnf_toy_device.h; bias = the accumulator's
//                       start, zero operands pad H to 16 / 4) with the B fragments of a wave's 16-column tile
//                       in registers once per Dense layer; the 1- / 2-wide first and last Dense layers,
//                       tanhf / expf and the coupling law run on the vector ALUs in k_toy's fmaf order. The
//                       last Dense parks tanh A in LDS and thread s adds point s's log-det after the
//                       barrier: k = 0 then k = 1 within a layer, layers in execution order; no
//                       floating-point atomics. An MFMA row is a dot product in a fixed k order and every
//                       vector-ALU step is per point, so a point's bits depend on (params, y[b], its fp32
//                       coordinates) alone. Epilogue per point: log_prob, y_dev, z; per tile (grids, when
//                       log_mass is asked for) the partial (m, s): m the largest finite log_prob of the tile,
//                       s = sum expf(v - m) in point order.
//   k_toy_density_mass  one wave per condition: the tile partials merged in tile order in fp64, log, plus
//                       the cell volume's log, rounded once (the formula: include/cnf.h). No atomics.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "cnf_device.h"
#include "cnf_toy_device.h"

namespace cnf {

namespace {

constexpr int TS = TOY_SAMPLE_TS;
constexpr int BT = 256;   // threads per workgroup (4 waves)
constexpr int NW = BT / 64;
constexpr int RT = TS / 16;   // 16-row tiles of a point tile
static_assert(TS % 16 == 0 && TS <= BT, "one epilogue thread per point");

// centre of bin i: lo + (i + 0.5) step as one multiply and then one add, each rounded to fp32 (include/cnf.h), so
// that numpy fp32 reproduces it bit for bit. Contraction is switched off for these two operations: the
// __fmul_rn / __fadd_rn of the HIP headers are plain operators, which the compiler fuses into one fma like any other
__device__ __forceinline__ float bin_centre(float lo, int i, float step) {
#pragma clang fp contract(off)
    const float t = ((float)i + 0.5f) * step;
    return lo + t;
}

}  // namespace

// KS: k steps of the H x H MFMA layers (H <= 4 KS), the bound of the B-fragment register array
template <int KS>
__global__ __launch_bounds__(BT) void k_toy_density(ToyDensityArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int H = a.flow.H, L = a.flow.L, HP = a.HP;
    float* act = sm;                   // [2][TS][HP] post-activation hidden vectors, ping-pong
    float* su = act + 2 * TS * HP;     // [TS][3] the points' state: xy, then each layer's output, then zy
    float* bo = su + 3 * TS;           // [TS][2] the b net's output
    float* ta = bo + 2 * TS;           // [TS][2] tanh A of the current layer
    float* lp = ta + 2 * TS;           // [TS] the points' log_prob, for the tile's partial
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int b = blockIdx.x / a.tiles, tile = blockIdx.x - b * a.tiles;
    const int s0 = tile * TS;
    const int cnt = a.N - s0 < TS ? a.N - s0 : TS;   // points of this tile (>= 1); rows past them are zeros
    const int HT = (H + 15) / 16;
    const int x_d = a.flow.x_d, yd = 3 - x_d;
    const float* __restrict__ yb = a.y + (size_t)b * yd;
    const int fd_s = tid / H, fd_o = tid - fd_s * H;   // the first Dense's element walk: start and step of (s, o)
    const int fd_ds = BT / H, fd_do = BT - fd_ds * H;

    // the points: bin centre lo + (i + 0.5) step of a grid (one multiply, then one add, each rounded), or x; then y[b]
    for (int e = tid; e < 3 * TS; e += BT) {
        const int s = e / 3, c = e - 3 * s;
        float v = 0.f;
        if (s < cnt) {
            if (c >= x_d) {
                v = yb[c - x_d];
            } else if (a.x != nullptr) {
                v = a.x[((size_t)b * a.N + (size_t)(s0 + s)) * x_d + c];
            } else {
                const int p = s0 + s;   // p = i0 G + i1 (x_d 2: component 0 major), p = i0 (x_d 1)
                const int i0 = x_d == 2 ? p / a.G : p;
                const int ic = c == 0 ? i0 : p - i0 * a.G;
                v = bin_centre(a.lo[c], ic, a.step[c]);
            }
        }
        su[e] = v;
    }
    float ld = 0.f;   // thread s < TS: the log-det of point s

    for (int step = 0; step < a.flow.nl; step++) {
        const int j = a.flow.order[a.flow.nl - 1 - step];   // direction -1: reverse index order
        const ToyMask m = toy_mask(j);   // u1 / u2 index sets (:149-163), as k_toy
        const int n1 = m.n1, n2 = m.n2;
        const int i1[2] = {m.i1[0], m.i1[1]}, i2[2] = {m.i2[0], m.i2[1]};
        const int net_floats = (a.flow.net_off[j + 1] - a.flow.net_off[j]) / 2;
        __syncthreads();   // su of the previous layer (or the points) complete

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
                    ta[2 * s + q] = A;
                    su[3 * s + i2[q]] = expf(A) * su[3 * s + i2[q]] + bo[2 * s + q];   // :380
                }
            }
            __syncthreads();
        }
        // log det diag(exp A) (:386-387): one thread per point, k = 0 then k = 1 (ta is next written behind
        // the barriers of the next layer)
        if (tid < TS) {
            ld += ta[2 * tid];
            if (n2 == 2) ld += ta[2 * tid + 1];
        }
    }
    __syncthreads();   // (nl == 0 is refused by the host; keeps the points visible all the same)

    // epilogue: one thread per point
    if (tid < cnt) {
        const int s = tid;
        const size_t g = (size_t)b * a.N + (size_t)(s0 + s);
        // log N(z; 0, I_xd) in k_toy's order
        float llz = -0.5f * (float)x_d * (float)LOG_2PI_D;
        for (int c = 0; c < x_d; c++) llz -= 0.5f * su[3 * s + c] * su[3 * s + c];
        const float v = llz + ld;
        lp[s] = v;
        if (a.log_prob != nullptr) a.log_prob[g] = v;
        if (a.y_dev != nullptr) {
            float d = 0.f;
            for (int c = x_d; c < 3; c++) d += fabsf(su[3 * s + c] - yb[c - x_d]);
            a.y_dev[g] = d;
        }
        if (a.z != nullptr)
            for (int c = 0; c < x_d; c++) a.z[g * x_d + c] = su[3 * s + c];
    }
    // the tile's partial of log_mass, folded in point order: (NaN, NaN) once a log_prob is a NaN (or +inf,
    // which no finite flow produces), (-inf, 0) with no finite value
    if (a.part != nullptr) {
        __syncthreads();
        if (tid == 0) {
            float mx = -INFINITY;
            bool bad = false;
            for (int s = 0; s < cnt; s++) {
                const float v = lp[s];
                bad = bad || !(v <= 3.0e38f);
                if (v > mx) mx = v;
            }
            float sum = 0.f;
            if (!bad && mx > -INFINITY) {
#pragma unroll 8
                for (int s = 0; s < cnt; s++) sum += expf(lp[s] - mx);   // (-inf contributes expf(-inf) = 0)
            }
            float* dst = a.part + ((size_t)b * a.tiles + tile) * TOY_DENSITY_PART;
            dst[0] = bad ? NAN : mx;
            dst[1] = bad ? NAN : sum;
        }
    }
}

// One wave per condition b. The lanes read the partials (m_t, s_t) of 64 tiles at a time; lane 0 walks them in
// tile order in fp64:
//   M = max_t m_t over the tiles with a finite value,  S = sum_t s_t exp(m_t - M),
//   log_mass = fl32(M + log S + sum_c log step_c)
// -inf with no finite value in any tile, NaN once a tile's partial is a NaN.
__global__ __launch_bounds__(64) void k_toy_density_mass(const float* __restrict__ part, int tiles, double log_cell,
                                                         float* __restrict__ log_mass) {
    __shared__ double sm_[64], ss_[64];
    __shared__ double sh_M;
    const int lane = threadIdx.x;
    const int b = blockIdx.x;
    const float* __restrict__ p = part + (size_t)b * tiles * TOY_DENSITY_PART;
    double M = -INFINITY, S = 0.0;
    bool bad = false;
    for (int pass = 0; pass < 2; pass++) {
        for (int base = 0; base < tiles; base += 64) {
            const int t = base + lane;
            if (t < tiles) {
                sm_[lane] = (double)p[(size_t)t * TOY_DENSITY_PART];
                ss_[lane] = (double)p[(size_t)t * TOY_DENSITY_PART + 1];
            }
            __syncthreads();
            if (lane == 0) {
                const int n = tiles - base < 64 ? tiles - base : 64;
                if (pass == 0) {
                    for (int i = 0; i < n; i++) {
                        bad = bad || sm_[i] != sm_[i] || ss_[i] != ss_[i];
                        if (ss_[i] > 0.0 && sm_[i] > M) M = sm_[i];
                    }
                } else {
                    for (int i = 0; i < n; i++)
                        if (ss_[i] > 0.0) S += ss_[i] * exp(sm_[i] - M);
                }
            }
            __syncthreads();
        }
        if (pass == 0) {
            if (lane == 0) sh_M = M;
            __syncthreads();
            M = sh_M;
        }
    }
    if (lane == 0) {
        float r;
        if (bad)
            r = NAN;
        else if (!(S > 0.0))
            r = -INFINITY;
        else
            r = (float)(M + log(S) + log_cell);
        log_mass[b] = r;
    }
}

size_t toy_density_lds_bytes(int H) { return ((size_t)2 * TS * toy_bwd_hp(H) + 8 * TS) * sizeof(float); }

void launch_toy_density(const ToyDensityArgs& a, hipStream_t st) {
    const dim3 g((unsigned)a.B * (unsigned)a.tiles), b(BT);
    const size_t lds = toy_density_lds_bytes(a.flow.H);
    if (a.flow.H <= 16)
        hipLaunchKernelGGL(k_toy_density<4>, g, b, lds, st, a);
    else if (a.flow.H <= 32)
        hipLaunchKernelGGL(k_toy_density<8>, g, b, lds, st, a);
    else if (a.flow.H <= 48)
        hipLaunchKernelGGL(k_toy_density<12>, g, b, lds, st, a);
    else
        hipLaunchKernelGGL(k_toy_density<16>, g, b, lds, st, a);
}

void launch_toy_density_mass(const float* part, int B, int tiles, double log_cell, float* log_mass, hipStream_t st) {
    hipLaunchKernelGGL(k_toy_density_mass, dim3((unsigned)B), dim3(64), 0, st, part, tiles, log_cell, log_mass);
}

}  // namespace cnf
