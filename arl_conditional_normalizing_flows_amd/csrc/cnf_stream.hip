// cnf_stream.hip — image-looping streamed convolutions for coupling layers whose s,t-net
// activations do not fit one CU's LDS (k_net_lds covers the rest).
//
//   k_pw   1x1 convolution (conv_a / conv_b of dilated_residual_block,
//          conv_cINN_base_functions.py:561-565, 609-613) with LeakyReLU -> per-image LayerNorm
//          (per-element gamma/beta, :330-362) applied on load, bias + residual in the epilogue
//          and the per-wave LN partials of LeakyReLU(out) for the next LayerNorm.
//
// Work decomposition: a workgroup (PW_NW waves, 16 pixels each) owns one 64-pixel tile of one net
// and loops over `ipw` images. Every wave runs its own image loop without barriers: the next
// image's activations (and residual) are loaded into registers before the current image's MFMAs,
// so HBM traffic and compute overlap inside the wave. The tile's LN gamma/beta are loaded once and
// serve every image; weights and the per-image LN (mean, rstd) live in LDS.
//
// The contraction runs on the bf16 matrix cores as the exact three-term split of cnf_device.h
// (bf16x6, fp32-accurate): K in 32-deep steps, lane (i16, kq) of a wave holding channels
// 32c + 8kq .. +7 of its pixel at step c; the weights lie in LDS as their three bf16 planes (x6_at),
// copied once per workgroup from the plane image cnf_pack_params built (stage_copy16), or, under the
// debug option PRESPLIT=0, split from the fp32 image by the workgroup itself (stage_w_x6).
#include <cstdlib>
#include <cstring>
#include <stdexcept>

#include "cnf_device.h"

namespace cnf {

#include "cnf_pw_shapes.inc"   // shape-specialised k_pw instantiations (gen_netlds_shapes.py)

constexpr int PW_LDS_STAT = 256;    // byte offset of the per-image (mean, rstd) table
constexpr int PW_NW = 4;   // waves per k_pw workgroup (two workgroups per CU)

#ifndef CNF_PW_MINW
#define CNF_PW_MINW 2
#endif
// shape fields: compile-time constants of table entry SID in the shape-specialised instantiations
// (cin is read at run time in every instantiation: folded to a constant, the specialised builds gave
// run-to-run different outputs at cfg2 B = 64 and cfg5 (zy 2e-2 .. 6e-2 off the oracle), while
// builds with the same code and cin read at run time -- every other field still a constant -- were
// exact; found by bisecting the folded fields, profiles/sessions/r6_x6x.sh)
#define PP(f) (SID >= 0 ? kPwShapes[SID >= 0 ? SID : 0].f : P.f)
#define PA(f) (SID >= 0 ? kPwShapes[SID >= 0 ? SID : 0].f : a.f)
// diagnostic per-workgroup stamps (CNF_PW_STAMPS=SID builds only; never in timed runs): thread 0 of
// every workgroup of the instantiation SID records s_memrealtime at its start (0), before (1) and
// after (2) the prologue barrier and after each of its images (3 + i)
#if defined(CNF_PW_STAMPS) || defined(CNF_GC_WGSTAMPS)
constexpr int PW_ST_WG = 2048, PW_ST_N = 12;
#else
constexpr int PW_ST_WG = 1, PW_ST_N = 1;   // (no stamps in this build: a placeholder, never written)
#endif
__device__ long long g_pw_stamps[PW_ST_WG][PW_ST_N];
#ifdef CNF_PW_STAMPS
#define PWSTAMP(i)                                                                                       \
    do {                                                                                                 \
        if (SID == CNF_PW_STAMPS && threadIdx.x == 0 && (i) < PW_ST_N &&                                 \
            blockIdx.y * gridDim.x + blockIdx.x < PW_ST_WG)                                              \
            g_pw_stamps[blockIdx.y * gridDim.x + blockIdx.x][(i)] = (long long)__builtin_amdgcn_s_memrealtime(); \
    } while (0)
#else
#define PWSTAMP(i) do { } while (0)
#endif
int read_pw_stamps(long long* host) {
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_pw_stamps), sizeof(g_pw_stamps)) == hipSuccess ? 0 : -1;
}

// images of a wave in flight ahead of the one being computed: one. Deeper rings measured slower at
// cfg2 B=64 (two / four images: conv_a 19.1 -> 20.8 / 21.0 us, conv_out 11.9 -> 14.1 us; issued with
// the prologue's loads, slower still), and for the residual conv_b in round 2
//
// The PK_1X1 fp32 weight image (plan: [g][q][j][s], k = 16g + 4q + s, column j < 16 NR) -> the bf16x6
// fragment planes in LDS: plane p (h, m, l) of K step c and column block nb at byte
// ((c * 3 + p) * NR + nb) * 1024 + lane * 16, lane (kq, i16) holding W[k = 32c + 8kq + jj][16nb + i16]
// (jj < 8); zero past the image's G groups. Four float4 loads in flight per thread.
template <int NTH, int NR>
__device__ __forceinline__ void stage_w_x6(const float* __restrict__ src, unsigned char* dst, int G, int C) {
    constexpr int NSJ = 16 * NR;
    int n = __builtin_amdgcn_readfirstlane(C * NR * 128);   // float4 slots (c, nb, lane, half)
    asm volatile("" : "+s"(n));   // opaque count: a constant one unrolls the copy into the live image loads
    const f4* s4 = reinterpret_cast<const f4*>(src);
    for (int base = 0; base < n; base += NTH * 4) {
        f4 v[4];
        int o[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int t = base + u * NTH + (int)threadIdx.x;
            const int c = t / (NR * 128), r = t - c * (NR * 128), nb = r >> 7, ln = (r >> 1) & 63, half = r & 1;
            const int k0 = 32 * c + 8 * (ln >> 4) + 4 * half, col = 16 * nb + (ln & 15);
            const int g = k0 >> 4, q = (k0 >> 2) & 3;
            v[u] = t < n && g < G ? s4[(g * 4 + q) * NSJ + col] : f4{0.f, 0.f, 0.f, 0.f};
            o[u] = t < n ? x6_at(k0, col, 0, NR) : -1;   // plane 0; planes 1, 2 follow NR KiB apart
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (o[u] < 0) continue;
            bf16x4 h, m, l;
            split4(v[u], h, m, l);
            *reinterpret_cast<bf16x4*>(dst + o[u]) = h;
            *reinterpret_cast<bf16x4*>(dst + o[u] + NR * 1024) = m;
            *reinterpret_cast<bf16x4*>(dst + o[u] + 2 * NR * 1024) = l;
        }
    }
}

// Staging from the plan's bf16x6 plane image (cnf_kernels.h x6_at; built once per weight update by
// cnf_pack_params): the image is byte for byte what stage_w_x6 / stage_gcw_x6 leave in LDS, so the
// workgroup copies its n16 16-byte units, unit tid + u NTH by thread tid. MAXU > 0: a compile-time bound
// on the units per thread, every load in flight before the first LDS write (units past n16 read 0 through
// the buffer resource and are not written); MAXU == 0 (run-time shapes): sweeps of four units per thread
template <int NTH, int MAXU>
__device__ __forceinline__ void stage_copy16(const void* __restrict__ src, unsigned char* dst, int n16) {
    const auto r = buf_rsrc(src, (uint32_t)n16 * 16u);
    const int tid = (int)threadIdx.x;
    if constexpr (MAXU > 0) {
        f4 v[MAXU];
#pragma unroll
        for (int u = 0; u < MAXU; u++) v[u] = buf_load4(r, (uint32_t)(tid + u * NTH) * 16u);
#pragma unroll
        for (int u = 0; u < MAXU; u++)
            if (tid + u * NTH < n16) *reinterpret_cast<f4*>(dst + (tid + u * NTH) * 16) = v[u];
    } else {
        for (int base = 0; base < n16; base += NTH * 4) {
            f4 v[4];
#pragma unroll
            for (int u = 0; u < 4; u++) v[u] = buf_load4(r, (uint32_t)(base + tid + u * NTH) * 16u);
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (base + tid + u * NTH < n16) *reinterpret_cast<f4*>(dst + (base + tid + u * NTH) * 16) = v[u];
        }
    }
}

// DUAL (generic non-tap instantiations of the training forward only): every output element is also
// stored densely ([HW][cout]) to P.out2 -- conv_a's full t1 saved for the backward in the same launch
template <int NR, int GM, bool LN, bool RES, int SID, bool TAP = false, bool DUAL = false>
__global__ __launch_bounds__(64 * PW_NW, CNF_PW_MINW) void k_pw(ConvArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int NW = PW_NW;
    PWSTAMP(0);
    const ConvProb P = a.p[blockIdx.y];
    const int HW = PA(H) * PA(W);
    const int tile = blockIdx.x % PA(tiles_per_img);
    const int img0 = (blockIdx.x / PA(tiles_per_img)) * a.ipw;
    const int nimg = min(a.ipw, a.B - img0);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sub = wave;   // pixel subtile
    const int i16 = lane & 15, kq = lane >> 4;
    const int cin = P.cin, G = (cin + 15) >> 4, C = (cin + 31) >> 5, cout = PP(cout);
    // quad slots of the lane: slot g holds channels 32 (g / 2) + 8 kq + 4 (g % 2) .. +3 (K step g / 2)
    constexpr int CM = (GM + 1) / 2, GX = 2 * CM;
    unsigned char* lwb = smem + PP(lds_w_off);
    float* lstat = reinterpret_cast<float*>(smem + PW_LDS_STAT);
    // buffer resources: out-of-range offsets (BUF_OOB) load 0 / drop the store
    const uint32_t in_img = TAP ? (uint32_t)PA(uimg) * 4u : (uint32_t)HW * PP(in_cs) * 4u;
    const uint32_t out_img = (uint32_t)HW * PP(out_cs) * 4u;
    // one buffer resource per image (64-bit image base, 32-bit offsets inside the image): the batch
    // size never limits the addressing
    auto img_rsrc = [](const float* base, int img, uint32_t bytes) {
        return buf_rsrc(base + (size_t)img * (bytes >> 2), bytes);
    };

    // A operand: lane (i16, kq) feeds pixel pa, the channels of its quad slots. Masks are evaluated
    // per element from shape fields (folded to constants in the specialised instantiations, whose
    // offsets then become lane base + immediate)
    const bool full_px = HW % (16 * NW) == 0;
    const int pa = tile * (16 * NW) + sub * 16 + i16;
    const bool pav = full_px || pa < HW;
    auto chq = [&](int g) { return 32 * (g >> 1) + 8 * kq + 4 * (g & 1); };   // first channel of slot g
    const uint32_t aoff = ((uint32_t)pa * PP(in_cs) + PP(in_off)) * 4u;
    // mapped input (conv_b over a t2 split into its producers' sub-tensors): quad chq(g) / 4 of the
    // lane's pixel at in_map's (offset, pixel stride)
    uint32_t amap[GX];
#pragma unroll
    for (int g = 0; g < GX; g++)
        amap[g] = PP(in_mapped) && chq(g) < cin
                      ? (uint32_t)(P.in_map[2 * (chq(g) >> 2)] + pa * P.in_map[2 * (chq(g) >> 2) + 1]) * 4u
                      : 0u;
    auto aoffg = [&](int g) -> uint32_t { return PP(in_mapped) ? amap[g] : aoff + 4u * chq(g); };
    auto gok = [&](int g) { return pav && chq(g) < cin; };
    // output: acc[n][r] = out[pixel po0 + r][channel 16n + i16]
    const int po0 = tile * (16 * NW) + sub * 16 + kq * 4;
    const uint32_t obase = ((uint32_t)po0 * PP(out_cs) + PP(out_off) + i16) * 4u;
    const bool all_st = PP(st_mask_lo) == ~0u && PP(st_mask_hi) == ~0u;
    auto chv = [&](int n) { return cout % 16 == 0 || n * 16 + i16 < cout; };
    auto pv = [&](int r) { return full_px || po0 + r < HW; };
    // mapped stores (conv_a -> t1 of the streamed layers, Coupling::t1_map): the lane's channel of
    // group n goes to (offset of pixel 0, pixel stride) inside the image; offset < 0: not stored
    int cmo[NR], cms[NR];
#pragma unroll
    for (int n = 0; n < NR; n++) {
        cmo[n] = PP(st_compact) && n * 16 + i16 < 64 ? P.st_map[2 * (n * 16 + i16)] : -1;
        cms[n] = PP(st_compact) && n * 16 + i16 < 64 ? P.st_map[2 * (n * 16 + i16) + 1] : 0;
    }
    auto ooff = [&](int n, int r) -> uint32_t {   // byte offset inside one image, BUF_OOB when not stored
        const int ch = n * 16 + i16;
        if (PP(st_compact))
            return (pv(r) && chv(n) && cmo[n] >= 0) ? (uint32_t)(cmo[n] + (po0 + r) * cms[n]) * 4u : BUF_OOB;
        const bool st = all_st || ((ch < 32 ? (PP(st_mask_lo) >> ch) : (PP(st_mask_hi) >> (ch - 32))) & 1u) != 0u;
        return (pv(r) && chv(n) && st) ? obase + (uint32_t)(r * PP(out_cs) + 16 * n) * 4u : BUF_OOB;
    };
    // image activations (+ residual) in registers: the current image and the next
    f4 x[GX];
    float rv[NR][4];
    // tap mode: element k = chq(g) + j of the lane's im2col row -> offset inside one image of u
    auto toff = [&](int g, int j) -> uint32_t {
        const int k = chq(g) + j;
        if (!pav || k >= cin) return BUF_OOB;
        const int tap = k / PA(udc), c = k - tap * PA(udc);
        const int d = PA(udil);
        const int pr = pa / PA(W) + (tap / 3 - 1) * d, pc = pa % PA(W) + (tap % 3 - 1) * d;
        if ((unsigned)pr >= (unsigned)PA(H) || (unsigned)pc >= (unsigned)PA(W)) return BUF_OOB;
        if (PA(umask) < 0) return (uint32_t)((pr * PA(W) + pc) * PA(uD) + PA(uoff) + c) * 4u;
        return (uint32_t)mask_pos(PA(umask), pr * PA(W) + pc, c, PA(W), PA(uW), PA(uD)) * 4u;
    };
    // plain-NHWC tap sources with quad-aligned channels: one 16-byte load per (tap, quad) (the
    // row's channel quads never straddle two taps when cin % 4 == 0)
    const bool tquad = TAP && PA(umask) < 0 && PA(udc) % 4 == 0 && PA(uoff) % 4 == 0 && PA(uD) % 4 == 0;
    auto load_img = [&](int ii, f4 (&xd)[GX], float (&rd)[NR][4]) {
        const auto rin = img_rsrc(P.in, img0 + ii, in_img);
        constexpr uint32_t ib = 0;
        if constexpr (TAP) {
#pragma unroll
            for (int g = 0; g < GX; g++) {
                if (tquad) {   // the lane's 4 elements are one channel quad of one tap's pixel
                    const uint32_t o = toff(g, 0);
                    xd[g] = buf_load4(rin, o == BUF_OOB ? BUF_OOB : ib + o);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const uint32_t o = toff(g, j);
                        xd[g][j] = buf_load1(rin, o == BUF_OOB ? BUF_OOB : ib + o);
                    }
                }
            }
        } else {
#pragma unroll
            for (int g = 0; g < GX; g++) xd[g] = buf_load4(rin, gok(g) ? ib + aoffg(g) : BUF_OOB);
        }
        if (RES) {
            const auto rres = img_rsrc(RES ? P.res : P.out, img0 + ii, out_img);
            constexpr uint32_t ob = 0;
#pragma unroll
            for (int n = 0; n < NR; n++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const uint32_t o = ooff(n, r);
                    rd[n][r] = buf_load1(rres, o == BUF_OOB ? BUF_OOB : ob + o);
                }
        }
    };
    if (0 < nimg) load_img(0, x, rv);
    f4 gm[GX], bt[GX];
    if (LN) {
        const auto rg = buf_rsrc(P.gamma, in_img), rb = buf_rsrc(P.beta, in_img);
#pragma unroll
        for (int g = 0; g < GX; g++) {
            if constexpr (TAP) {   // the lane's im2col row: gamma / beta of every tap's pixel (0 outside: zero padding)
                if (tquad) {
                    const uint32_t o = toff(g, 0);
                    gm[g] = buf_load4(rg, o);
                    bt[g] = buf_load4(rb, o);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const uint32_t o = toff(g, j);
                        gm[g][j] = buf_load1(rg, o);
                        bt[g][j] = buf_load1(rb, o);
                    }
                }
            } else {
                const uint32_t o = gok(g) ? aoffg(g) : BUF_OOB;   // 0 where masked: the normalised value is then exactly 0
                gm[g] = buf_load4(rg, o);
                bt[g] = buf_load4(rb, o);
            }
        }
    }
    float bias[NR];
#pragma unroll
    for (int n = 0; n < NR; n++) bias[n] = n * 16 + i16 < cout ? P.bias[n * 16 + i16] : 0.f;

    // the first image of this wave's LN-statistics share: its partial slots fetched now, in the same
    // memory round trip as the loads above and the weights below (folded after the weight copy)
    const bool lnpre = LN && wave < nimg;   // (image wave: the LN table below is per workgroup)
    const LnSlots slot0 = lnpre ? in_ln_fetch(P, img0 + wave) : LnSlots{};
    // weights -> their bf16x6 planes in LDS; per-image input LN (mean, rstd) -> LDS
    if (P.wx6 != nullptr)   // (CM K steps at most: C <= CM)
        stage_copy16<64 * NW, (CM * 3 * NR * 64 + 64 * NW - 1) / (64 * NW)>(P.wx6, lwb, C * 3 * NR * 64);
    else
        stage_w_x6<64 * NW, NR>(P.wt, lwb, G, C);
    if (LN) {
        for (int i = wave; i < nimg; i += NW) {
            float mu, rs;
            if (i == wave && lnpre)
                in_ln_finish(P, img0 + i, slot0, mu, rs);
            else
                in_ln(P, img0 + i, mu, rs);
            if (lane == 0) {
                lstat[2 * i] = mu;
                lstat[2 * i + 1] = rs;
            }
        }
    }
    PWSTAMP(1);
    __syncthreads();
    PWSTAMP(2);

    const unsigned char* bl0 = lwb + lane * 16;
    // one image: A operand from xc / rc, which then receive image pf (when it exists)
    auto step = [&](int ii, f4 (&xc)[GX], float (&rc)[NR][4], int pf) {
        const int img = img0 + ii;
        const float rs = LN ? lstat[2 * ii + 1] : 1.f;
        const float mu = LN ? lstat[2 * ii] : 0.f;   // (t - mu) * rs, not fma(t, rs, -mu * rs): cnf_device.h
        f4 av[GX];
#pragma unroll
        for (int g = 0; g < GX; g++) {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const float v = !TAP || P.act ? lrelu(xc[g][j]) : xc[g][j];   // conv_in reads raw u
                av[g][j] = LN ? fmaf((v - mu) * rs, gm[g][j], bt[g][j]) : v;
            }
        }
        float res[NR][4];
        if (RES) {
#pragma unroll
            for (int n = 0; n < NR; n++)
#pragma unroll
                for (int r = 0; r < 4; r++) res[n][r] = rc[n][r];
        }
#ifdef CNF_DIAG
        if (!(a.diag & 2))
#endif
        if (pf < nimg) load_img(pf, xc, rc);   // in flight during this image's MFMAs and stores
        f4 acc[NR];
#pragma unroll
        for (int n = 0; n < NR; n++) acc[n] = f4{0.f, 0.f, 0.f, 0.f};
        // per K step: the lane's 8 activations split into their bf16 planes, then per column block the
        // weight planes from LDS and six MFMAs; the scheduling fence keeps the compiler from hoisting
        // every step's LDS reads into live registers
#pragma unroll
        for (int c = 0; c < CM; c++) {
            if (c < C) {
                const Split8 a8 = split8(av[2 * c], av[2 * c + 1]);
#pragma unroll
                for (int n = 0; n < NR; n++) {
                    const unsigned char* bp = bl0 + (c * 3 * NR + n) * 1024;
                    const bf16x8 bh = *reinterpret_cast<const bf16x8*>(bp);
                    const bf16x8 bm = *reinterpret_cast<const bf16x8*>(bp + NR * 1024);
                    const bf16x8 bl = *reinterpret_cast<const bf16x8*>(bp + 2 * NR * 1024);
                    acc[n] = mfma_x6(a8.h, a8.m, a8.l, bh, bm, bl, acc[n]);
                }
            }
        }
        // epilogue: bias, residual, masked store, per-wave LN partial of LeakyReLU(out)
        const auto rout = img_rsrc(P.out, img, out_img);
        const auto rout2 = img_rsrc(DUAL ? P.out2 : P.out, img, (uint32_t)HW * cout * 4u);
        constexpr uint32_t ob = 0;
        float vals[NR * 4];
        bool valid[NR * 4];
#pragma unroll
        for (int n = 0; n < NR; n++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                float v = acc[n][r] + bias[n];
                if (RES) v += res[n][r];
#ifndef CNF_ABL_PW_NOSTORE
                const uint32_t o = ooff(n, r);
                buf_store1(rout, o == BUF_OOB ? BUF_OOB : ob + o, v);
                if constexpr (DUAL)
                    buf_store1(rout2, pv(r) && chv(n) ? (uint32_t)((po0 + r) * cout + 16 * n + i16) * 4u : BUF_OOB, v);
#endif
                vals[n * 4 + r] = lrelu(v);
                valid[n * 4 + r] = pv(r) && chv(n);
            }
        if (P.out_part != nullptr)
            ln_partial(vals, valid,
                       P.out_part + ((size_t)img * PP(part_stride) + P.out_part_base + tile * NW + sub) * LNP);
    };
    // this wave's images: the buffers then receive image ii + 1
    for (int ii = 0; ii < nimg; ii++) {
#ifdef CNF_DIAG
        if ((a.diag & 2) && ii > 0) load_img(ii, x, rv);   // (experiment: no prefetch)
        if (a.diag & 4) __syncthreads();
#endif
        step(ii, x, rv, ii + 1);
        PWSTAMP(3 + ii);
    }
}

#undef PP
#undef PA

template <int S>
bool launch_pw_shape(int sid, const ConvArgs& a, dim3 g, dim3 b, int lds, hipStream_t st) {
    if constexpr (S < CNF_PW_NSHAPES) {
        if (sid == S) {
            constexpr PwShape k = kPwShapes[S];
            CNF_LAUNCH((k_pw<k.nr, k.gm, k.ln != 0, k.res != 0, S, k.tap != 0>), g, b, lds, st, a);
            return true;
        }
        return launch_pw_shape<S + 1>(sid, a, g, b, lds, st);
    }
    return false;
}

int pw_num_shapes() { return CNF_PW_NSHAPES; }

void launch_pw(int nr, int gm, bool ln, bool res, bool tap, const ConvArgs& a_in, int grid_x, int lds, hipStream_t st) {
#ifdef CNF_DIAG
    ConvArgs a = a_in;
    if (const char* e = std::getenv("CNF_PW_DIAG")) a.diag = std::atoi(e);
#else
    const ConvArgs& a = a_in;
#endif
    dim3 g(grid_x, a.nprob), b(64 * PW_NW);
    const bool generic = (opts().generic & 3) != 0;   // debug option GENERIC bit 1 (all) or 2 (k_pw)
    bool dual = false;
    for (int i = 0; i < a.nprob; i++) dual |= a.p[i].out2 != nullptr;
    if (dual) {   // training forward conv_a with the dense t1 copy: generic instantiations only
        if (tap || res || !ln) throw std::invalid_argument("k_pw dual store: LN, no residual, no tap mode");
        for (int i = 0; i < a.nprob; i++)
            if (a.p[i].out2 == nullptr) throw std::invalid_argument("k_pw dual store: every problem needs out2");
#define CNF_PW_DCASE(NR_, GM_)                                                         \
        if (nr == NR_ && gm == GM_) {                                                  \
            CNF_LAUNCH((k_pw<NR_, GM_, true, false, -1, false, true>), g, b, lds, st, a); \
            return;                                                                    \
        }
#define CNF_PW_DNR(GM_) CNF_PW_DCASE(1, GM_) CNF_PW_DCASE(2, GM_) CNF_PW_DCASE(3, GM_) CNF_PW_DCASE(4, GM_)
        CNF_PW_DNR(1) CNF_PW_DNR(2) CNF_PW_DNR(4) CNF_PW_DNR(8)
#undef CNF_PW_DNR
#undef CNF_PW_DCASE
        throw std::invalid_argument("k_pw dual store: no instantiation for this shape");
    }
    PwShape sh;
#ifdef CNF_DIAG
    const char* only = std::getenv("CNF_PW_ONLY_SID");   // diagnostic builds: one specialised instantiation
#endif
    if (!generic && pw_shape_of(nr, gm, ln, res, tap, a, sh))
        for (int sid = 0; sid < CNF_PW_NSHAPES; sid++) {
#ifdef CNF_DIAG
            if (only && std::atoi(only) != sid) continue;
#endif
            if (std::memcmp(&sh, &kPwShapes[sid], sizeof(sh)) == 0 && launch_pw_shape<0>(sid, a, g, b, lds, st)) return;
        }
    if (tap) {   // generic tap mode (streamed conv_in / grouped branches): no residual, K <= 128
        if (res || gm > 8) throw std::invalid_argument("k_pw tap mode: no residual, K <= 128");
#define CNF_PW_TCASE(NR_, GM_, LN_)                                                     \
        if (nr == NR_ && gm == GM_ && ln == LN_) {                                      \
            CNF_LAUNCH((k_pw<NR_, GM_, LN_, false, -1, true>), g, b, lds, st, a); \
            return;                                                                     \
        }
#define CNF_PW_TNR(GM_, LN_) CNF_PW_TCASE(1, GM_, LN_) CNF_PW_TCASE(2, GM_, LN_) CNF_PW_TCASE(3, GM_, LN_) CNF_PW_TCASE(4, GM_, LN_)
        CNF_PW_TNR(1, false) CNF_PW_TNR(2, false) CNF_PW_TNR(4, false) CNF_PW_TNR(8, false)
        CNF_PW_TNR(1, true) CNF_PW_TNR(2, true) CNF_PW_TNR(4, true) CNF_PW_TNR(8, true)
#undef CNF_PW_TNR
#undef CNF_PW_TCASE
        throw std::invalid_argument("k_pw tap mode: no instantiation for this shape");
    }
#define CNF_PW_CASE(NR_, GM_, LN_, RES_)                                              \
    if (nr == NR_ && gm == GM_ && ln == LN_ && res == RES_) {                          \
        CNF_LAUNCH((k_pw<NR_, GM_, LN_, RES_, -1>), g, b, lds, st, a);             \
        return;                                                                        \
    }
#define CNF_PW_NR(GM_, LN_, RES_) \
    CNF_PW_CASE(1, GM_, LN_, RES_) CNF_PW_CASE(2, GM_, LN_, RES_) CNF_PW_CASE(3, GM_, LN_, RES_) CNF_PW_CASE(4, GM_, LN_, RES_)
#define CNF_PW_GM(LN_, RES_) CNF_PW_NR(1, LN_, RES_) CNF_PW_NR(2, LN_, RES_) CNF_PW_NR(4, LN_, RES_) CNF_PW_NR(8, LN_, RES_)
    CNF_PW_GM(true, false) CNF_PW_GM(false, false) CNF_PW_GM(true, true) CNF_PW_GM(false, true)
#undef CNF_PW_GM
#undef CNF_PW_NR
#undef CNF_PW_CASE
    throw std::invalid_argument("k_pw: no instantiation for this shape");
}

}  // namespace cnf

namespace cnf {

#include "cnf_gc_shapes.inc"   // shape-specialised k_gc instantiations (gen_netlds_shapes.py)

// ---------------------------------------------------------------------------------------------
// k_gc: the grouped dilated stage of a residual block (conv_cINN_base_functions.py:364-413,
// 583-601) for the streamed layers — LN2(LeakyReLU(t1)) on the branch windows -> every branch's
// dense 3x3 dilated conv -> t2 slices, plus the per-wave LN3 partials of LeakyReLU(t2).
// ---------------------------------------------------------------------------------------------
// waves / threads of the instantiation for table entry SID (-1: generic)
#define GC_NWS (SID >= 0 ? kGcShapes[SID >= 0 ? SID : 0].nw : GC_NW_GEN)
#define GC_NTS (64 * GC_NWS)

// shape fields: compile-time constants of table entry SID in the shape-specialised instantiations
#define GS(f) (SID >= 0 ? kGcShapes[SID >= 0 ? SID : 0].f : a.s.f)

// BI >= 0 (specialised instantiations): branch BI of table entry SID, every field a constant
// tile pixel -> image pixel: full-width / 2-D tiles (ps == 1: px0 + row * W + column), or polyphase
// tiles (block blk of the tile = phase grid ph0 + blk, pixel (r0 + row, column) of that grid)
template <int SID>
__device__ __forceinline__ int gc_out_pixel(const GcArgs& a, int po, int px0, int r0, int ph0) {
    const int tpx = GS(TH) * GS(TW);
    const int blk = GS(nbk) > 1 ? po / tpx : 0;
    const int rem = po - blk * tpx;
    const int por = rem / GS(TW), poc = rem - por * GS(TW);
    if (GS(ps) > 1) {
        const int ph = ph0 + blk, pa = ph / GS(ps), pb = ph - pa * GS(ps);
        return (pa + (r0 + por) * GS(ps)) * GS(W) + pb + poc * GS(ps);
    }
    return px0 + por * GS(W) + poc;
}

// 16-byte units of a branch's planes and K-octet table (contiguous in LDS from w_off, and in the plan's
// plane image), and the most a thread of an nt-thread workgroup copies of any branch of s
__host__ __device__ constexpr int gc_w16(const GcBranch& br) { return br.G * 3 * ((br.cout + 15) >> 4) * 64 + 4 * br.G; }
constexpr int gc_copy_units(const GcShape& s, int nt) {
    int m = 1;
    for (int bi = 0; bi < s.nbr; bi++) m = (gc_w16(s.br[bi]) + nt - 1) / nt > m ? (gc_w16(s.br[bi]) + nt - 1) / nt : m;
    return m;
}

// The branch's PK_Q4 fp32 weight image (plan: quads qd = tap * cinp / 4 + ch / 4, [qd][16 nr][4]) ->
// its bf16x6 planes in LDS (as k_pw's stage_w_x6, rows = outputs): lane (kq, i16) of K step c, output
// block nb holds W[k = 32c + 8kq + jj][16nb + i16], k = tap * S + ch; zero past the taps / channels
template <int NTH>
__device__ __forceinline__ void stage_gcw_x6(const float* __restrict__ src, unsigned char* dst, const GcBranch& br,
                                             int nr) {
    const int n = br.G * nr * 128, ns = 16 * nr, cpq4 = br.cinp >> 2;   // float4 slots (c, nb, lane, half)
    for (int base = 0; base < n; base += NTH * 2) {
        f4 v[2];
        int o[2];
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const int t = base + u * NTH + (int)threadIdx.x;
            const int c = t / (nr * 128), r = t - c * (nr * 128), nb = r >> 7, ln = (r >> 1) & 63, half = r & 1;
            const int k0 = 32 * c + 8 * (ln >> 4) + 4 * half, col = 16 * nb + (ln & 15);
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int tap = (k0 + j) / br.S, ch = k0 + j - tap * br.S;
                v[u][j] = t < n && tap < 9 && ch < br.cin && col < br.cout
                              ? src[((tap * cpq4 + (ch >> 2)) * ns + col) * 4 + (ch & 3)]
                              : 0.f;
            }
            o[u] = t < n ? x6_at(k0, col, 0, nr) : -1;
        }
#pragma unroll
        for (int u = 0; u < 2; u++) {
            if (o[u] < 0) continue;
            bf16x4 h, m, l;
            split4(v[u], h, m, l);
            *reinterpret_cast<bf16x4*>(dst + o[u]) = h;
            *reinterpret_cast<bf16x4*>(dst + o[u] + nr * 1024) = m;
            *reinterpret_cast<bf16x4*>(dst + o[u] + 2 * nr * 1024) = l;
        }
    }
}

// one plane of a subtile lane's K octet (8 consecutive k = tap * S + ch of its im2col row) from the
// band: S >= 8 one 16-byte read, S = 4 two 8-byte reads (two taps), S = 2 four 4-byte reads
__device__ __forceinline__ bf16x8 gc_octet(const unsigned char* p, int S, const int4& o) {
    if (S >= 8) return *reinterpret_cast<const bf16x8*>(p + 2 * o.x);
    if (S == 4) {
        const bf16x4 u = *reinterpret_cast<const bf16x4*>(p + 2 * o.x), v = *reinterpret_cast<const bf16x4*>(p + 2 * o.y);
        return __builtin_shufflevector(u, v, 0, 1, 2, 3, 4, 5, 6, 7);
    }
    const bf16x2 u0 = *reinterpret_cast<const bf16x2*>(p + 2 * o.x), u1 = *reinterpret_cast<const bf16x2*>(p + 2 * o.y);
    const bf16x2 u2 = *reinterpret_cast<const bf16x2*>(p + 2 * o.z), u3 = *reinterpret_cast<const bf16x2*>(p + 2 * o.w);
    const bf16x4 lo = __builtin_shufflevector(u0, u1, 0, 1, 2, 3), hi = __builtin_shufflevector(u2, u3, 0, 1, 2, 3);
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

template <int NR, int SID, int BI>
__device__ __forceinline__ void gc_branch(const GcArgs& a, const GcBranch& brx, const unsigned char* smem,
                                          const float* bias, float* __restrict__ outp, int npx,
                                          int px0, int r0, int ph0, LnAcc& st, bool& first, bool stats, int boff,
                                          int wave) {
    const GcBranch& br = BI >= 0 ? kGcShapes[SID >= 0 ? SID : 0].br[BI >= 0 ? BI : 0] : brx;
    const int lane = threadIdx.x & 63;
    const int i16 = lane & 15, kq = lane >> 4;
    // bf16x6 contraction (cnf_device.h): the band's three planes (S bf16 channels per pixel), the weights'
    // three planes (1 KiB per K step, plane and 16 outputs), one int4 of band offsets per K octet
    const int S = br.S, PB = (br.BH * br.BW * S * 2 + 15) & ~15;
    const unsigned char* band = smem + br.band_off + boff;
    const unsigned char* wl = smem + br.w_off + lane * 16;
    const int4* ot = reinterpret_cast<const int4*>(smem + br.q_off);
    // operands swapped (A = weights, B = activations): lane (i16, kq) ends with pixel i16, channels
    // 16n + 4kq + r (r < 4) of the subtile, i.e. one 16-byte channel quad per n -> f4 stores
    f4 bz[NR];
    int nq[NR];   // valid channels of the lane's quad (0..4)
#pragma unroll
    for (int n = 0; n < NR; n++) {
        const int c0 = n * 16 + 4 * kq;
        nq[n] = max(0, min(4, br.cout - c0));
#pragma unroll
        for (int r = 0; r < 4; r++) bz[n][r] = r < nq[n] ? bias[c0 + r] : 0.f;
    }
    const bool vq = ((br.opcs | br.out_off) & 3) == 0;
    const int nsub = (npx + 15) >> 4;
    // two subtiles per wave and pass (s0, s0 + NW) share every weight read
    const int C = br.G;   // 32-deep K steps
    constexpr int NW = GC_NWS;   // (16 waves cover a 256-pixel tile in one pass: the pair's second half is dead code)
    for (int s0 = wave; s0 < nsub; s0 += 2 * NW) {
        const int s1 = s0 + NW;
        const bool v1 = s1 < nsub;
        const unsigned char* base[2];
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int pt = (h ? s1 : s0) * 16 + i16;
            const int ptc = pt < npx ? pt : 0;
            // block blk of a polyphase tile: band rows [blk (TH + 2 dil), ...)
            const int tpx = GS(TH) * GS(TW);
            const int blk = GS(nbk) > 1 ? ptc / tpx : 0;
            const int rem = ptc - blk * tpx;
            const int tr = rem / GS(TW), tc = rem - tr * GS(TW);
            base[h] = band + 2 * ((blk * (GS(TH) + 2 * br.dil) + tr) * br.BW + tc) * S;
        }
        f4 acc0[NR], acc1[NR];   // start at the bias
#pragma unroll
        for (int n = 0; n < NR; n++) {
            acc0[n] = bz[n];
            acc1[n] = bz[n];
        }
        for (int c = 0; c < C; c++) {
            const int4 o = ot[4 * c + kq];
#ifdef CNF_ABL_GC_BLDS   // ablation (diagnostic builds only, wrong results): one band plane read from LDS
            const bf16x8 xh0 = gc_octet(base[0], S, o), xm0 = xh0, xl0 = xh0;
#else
            const bf16x8 xh0 = gc_octet(base[0], S, o), xm0 = gc_octet(base[0] + PB, S, o),
                         xl0 = gc_octet(base[0] + 2 * PB, S, o);
#endif
            bf16x8 xh1 = xh0, xm1 = xm0, xl1 = xl0;
            if (v1) {
                xh1 = gc_octet(base[1], S, o);
                xm1 = gc_octet(base[1] + PB, S, o);
                xl1 = gc_octet(base[1] + 2 * PB, S, o);
            }
#pragma unroll
            for (int n = 0; n < NR; n++) {
                const unsigned char* wp = wl + (c * 3 * NR + n) * 1024;
                const bf16x8 wh = *reinterpret_cast<const bf16x8*>(wp);
#ifdef CNF_ABL_GC_WLDS   // ablation (diagnostic builds only, wrong results): one weight plane read from LDS
                const bf16x8 wm = wh, wlo = wh;
#else
                const bf16x8 wm = *reinterpret_cast<const bf16x8*>(wp + NR * 1024);
                const bf16x8 wlo = *reinterpret_cast<const bf16x8*>(wp + 2 * NR * 1024);
#endif
                acc0[n] = mfma_x6(wh, wm, wlo, xh0, xm0, xl0, acc0[n]);
                if (v1) acc1[n] = mfma_x6(wh, wm, wlo, xh1, xm1, xl1, acc1[n]);
            }
        }
        if (stats && first) {
            st.set_shift(lrelu(acc0[0][0]));
            first = false;
        }
#pragma unroll
        for (int h = 0; h < 2; h++) {
            if (h == 1 && !v1) break;
            const int po = (h ? s1 : s0) * 16 + i16;
            const bool pv = po < npx;
            float* orow = outp + (size_t)gc_out_pixel<SID>(a, pv ? po : 0, px0, r0, ph0) * br.opcs + br.out_off + 4 * kq;
#pragma unroll
            for (int n = 0; n < NR; n++) {
                const f4 v = h ? acc1[n] : acc0[n];
#ifdef CNF_ABL_GC_NOSTORE_POLY   // ablation (diagnostic builds only): no t2 stores from polyphase tiles
                if (GS(ps) > 1) {
                } else
#endif
                if (pv && nq[n] == 4 && vq) {
                    *reinterpret_cast<f4*>(orow + n * 16) = v;
                } else if (pv) {
#pragma unroll
                    for (int r = 0; r < 4; r++)
                        if (r < nq[n]) orow[n * 16 + r] = v[r];
                }
                if (stats) {
#pragma unroll
                    for (int r = 0; r < 4; r++) st.add(lrelu(v[r]), pv && r < nq[n]);
                }
            }
        }
    }
}

// staged band units per thread: 4 at 8 waves, 2 at 4 (the plan keeps a group's bands within
// gc_stage_units)
#define GC_GQS (gc_stage_units(GC_NWS) / GC_NTS)
#define GC_PDS (SID >= 0 ? kGcShapes[SID >= 0 ? SID : 0].pd : 1)   // band prefetch depth (images)

// the branches of table entry SID, unrolled at compile time
template <int SID, int BI>
__device__ __forceinline__ void gc_branches(const GcArgs& a, const unsigned char* smem, float* __restrict__ outp,
                                            int npx, int px0, int r0, int ph0, LnAcc& st, bool& first, bool stats,
                                            int boff, int vw) {
    if constexpr (BI < kGcShapes[SID].nbr) {
        constexpr GcBranch br = kGcShapes[SID].br[BI];
        const float* bias = reinterpret_cast<const float*>(smem + br.b_off);
        gc_branch<(br.cout + 15) / 16, SID, BI>(a, br, smem, bias, outp, npx, px0, r0, ph0, st, first, stats, boff, vw);
        gc_branches<SID, BI + 1>(a, smem, outp, npx, px0, r0, ph0, st, first, stats, boff, vw);
    }
}

// diagnostic phase stamps of workgroup (0, 0) (CNF_GC_STAMPS builds only; never in timed runs)
__device__ long long g_gc_stamps[64];
#ifdef CNF_GC_STAMPS
#define GSTAMP(i)                                                                             \
    do {                                                                                      \
        __syncthreads();                                                                      \
        if (threadIdx.x == 0 && blockIdx.x == 0 && blockIdx.y == 0)                           \
            g_gc_stamps[(i)] = (long long)__builtin_amdgcn_s_memrealtime();                  \
    } while (0)
#else
#define GSTAMP(i) do { } while (0)
#endif
// per-workgroup stamps (CNF_GC_WGSTAMPS builds only): thread 0 of every workgroup, at its start (0),
// after the prologue (1) and after each image (2 + i); read through cnf_debug_read_pw_stamps
#ifdef CNF_GC_WGSTAMPS
#define GWSTAMP(i)                                                                                       \
    do {                                                                                                 \
        if (threadIdx.x == 0 && (i) < PW_ST_N && blockIdx.y * gridDim.x + blockIdx.x < PW_ST_WG)         \
            g_pw_stamps[blockIdx.y * gridDim.x + blockIdx.x][(i)] = (long long)__builtin_amdgcn_s_memrealtime(); \
    } while (0)
#else
#define GWSTAMP(i) do { } while (0)
#endif

// One workgroup per CU: a tile of TH rows of one net, looping over `ipw` images. The bands are
// double-buffered: the next image's t1 quads are loaded into registers before the current image's
// MFMAs and written (LN2 + LeakyReLU applied) into the other buffer after them, so the staging
// latency hides behind the compute; the tile's LN2 gamma/beta stay in registers for all images.
template <int SID>
__global__ __launch_bounds__(GC_NTS, SID >= 0 ? 16 / GC_NWS : 1) void k_gc(GcArgs a) {
    constexpr int GC_NW = GC_NWS, GC_NT = GC_NTS, GC_GQ = GC_GQS, PD = GC_PDS;
    // image pairs: a specialised tile of at most GC_NW / 4 subtiles (the rows never cut by the image
    // edge) leaves three quarters of the waves without a subtile, so the two band buffers hold two
    // images computed at once by two wave sets (cfg5's 64-pixel dil-1 tile: 28.27 -> 27.13 ms per
    // cfg5 B=64 step; at GC_NW / 2 subtiles, cfg4's 128-pixel tile, it measured slower: 3.51 -> 3.61 ms,
    // the LDS reads of twice the waves against the staging no longer hidden) (waves w < NSUB: image i0, subtile w; NSUB <= w < 2 NSUB:
    // image i0 + 1, subtile w - NSUB), staged together before them instead of one behind the other.
    // Every subtile runs the same instructions as in one-image mode and writes the same LN slot
    // (subtile s -> slot s, zeros in the slots of waves without a subtile): bitwise the same results
    constexpr int NSUB = SID >= 0 ? (kGcShapes[SID >= 0 ? SID : 0].nbk * kGcShapes[SID >= 0 ? SID : 0].TH *
                                        kGcShapes[SID >= 0 ? SID : 0].TW + 15) / 16 : 0;
    // Off by default since the end of round 6: the cfg5 ragged-batch GPU test (B = 64 against batches of
    // 5, bit for bit) failed once (7.7e-3) in three full-suite runs of the final tree, and this is the
    // newest path of the cfg5 tiles; diagnostic builds with -DCNF_GC_PAIRS keep it for A/B
#ifndef CNF_GC_PAIRS
    constexpr bool PAIRS = false &&
#else
    constexpr bool PAIRS =
#endif
                           SID >= 0 && PD == 1 && NSUB > 0 && 4 * NSUB <= GC_NW &&
                           (kGcShapes[SID >= 0 ? SID : 0].ps > 1 ||
                            kGcShapes[SID >= 0 ? SID : 0].H % kGcShapes[SID >= 0 ? SID : 0].TH == 0);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int net = blockIdx.y;
    const int tile = blockIdx.x % GS(tiles_per_img);
    const int img0 = (blockIdx.x / GS(tiles_per_img)) * a.ipw;
    const int nimg = min(a.ipw, a.B - img0);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int H = GS(H), W = GS(W), HW = H * W;
    // 2-D tiles: TH rows x TW columns (TW == W for all but the widest images; W % TW == 0); polyphase
    // tiles (ps > 1): nbk phase grids from ph0, rows [r0, r0 + TH) of each (tpp row slices per grid)
    const bool poly = GS(ps) > 1;
    const int ty = GS(tiles_x) == 1 ? tile : tile / GS(tiles_x), tx = tile - ty * GS(tiles_x);
    const int ph0 = poly ? (tile / GS(tpp)) * GS(nbk) : 0;
    const int r0 = poly ? (tile - (tile / GS(tpp)) * GS(tpp)) * GS(TH) : ty * GS(TH), c0 = poly ? 0 : tx * GS(TW);
    const int rows = poly || GS(H) % GS(TH) == 0 ? GS(TH) : min(GS(TH), H - r0);
    const int npx = GS(nbk) * rows * GS(TW), px0 = r0 * W + c0;
    const bool ln = SID >= 0 ? (GS(lnst) & 1) != 0 : a.in_part[net] != nullptr;
    const bool stats = SID >= 0 ? (GS(lnst) & 2) != 0 : a.out_part[net] != nullptr;
    float* lstat = reinterpret_cast<float*>(smem + PW_LDS_STAT);
    int gs = 0;
    GSTAMP(gs++);
    GWSTAMP(0);

    // image-independent staging plan of this thread: unit e = tid + GC_NT*u of the concatenated branch
    // bands (a channel quad of a band pixel, up to the branch's S channels; S = 2: one pair) -> source
    // offset inside one image, LDS byte offset in plane 0 and plane stride, valid channels (0 = zeros;
    // bit 3: one 16-byte load, bit 4: a channel pair)
    int soff[GC_GQ], loff[GC_GQ], lpb[GC_GQ], nv[GC_GQ];
#pragma unroll
    for (int u = 0; u < GC_GQ; u++) {
        int e = tid + GC_NT * u;
        soff[u] = 0;
        loff[u] = -1;
        lpb[u] = 0;
        nv[u] = 0;
        for (int bi = 0; bi < GS(nbr); bi++) {
            const GcBranch& br = GS(br)[bi];
            const int cpq = br.S >= 4 ? br.S >> 2 : 1, nq = br.BH * br.BW * cpq;
            if (e < nq) {
                const int pix = cpq == 1 ? e : (int)__umulhi((unsigned)e, br.cpq_mag), cq = e - pix * cpq;
                const int brr = (int)__umulhi((unsigned)pix, br.bw_mag), bc = pix - brr * br.BW;
                int y = r0 - br.dil + brr, x = c0 + bc - br.dil;
                bool inb = y >= 0 && y < H && x >= 0 && x < W;
                if (poly) {   // band row brr of block blk -> row of phase grid ph0 + blk
                    const int bh = GS(TH) + 2, blk = brr / bh, sy = r0 - 1 + brr - blk * bh, sx = bc - 1;
                    const int ph = ph0 + blk, pa = ph / GS(ps), pb = ph - pa * GS(ps);
                    inb = sy >= 0 && sy < H / GS(ps) && sx >= 0 && sx < W / GS(ps);
                    y = pa + sy * GS(ps);
                    x = pb + sx * GS(ps);
                }
                loff[u] = br.band_off + 2 * (pix * br.S + 4 * cq);
                lpb[u] = (br.BH * br.BW * br.S * 2 + 15) & ~15;
                if (inb && 4 * cq < br.cin) {
                    soff[u] = (y * W + x) * br.pcs + br.cin_off + 4 * cq;
                    const int v = min(4, br.cin - 4 * cq);
                    const bool vec = v == 4 && ((br.cin_off | br.pcs) & 3) == 0;
                    nv[u] = v | (vec ? 8 : 0);
                }
                if (br.S == 2) nv[u] |= 16;
                break;
            }
            e -= nq;
        }
    }
    // one staged quad through a buffer resource (out-of-range offset BUF_OOB reads 0). The vector
    // / scalar choice is made per wave (ballot), never per lane: a lane-divergent choice makes both
    // paths write the same VGPRs, and the compiler then drains every load (vmcnt(0)) before the next
    // one — the gathers of a band would run one round trip at a time.
    auto load_q = [&](__amdgpu_buffer_rsrc_t r, int u) -> f4 {
        const int n = nv[u] & 7;
        const uint32_t o = (uint32_t)soff[u] * 4u;
        if (__all(n == 0 || (nv[u] & 8) != 0)) return buf_load4(r, n == 0 ? BUF_OOB : o);
        f4 v;
#pragma unroll
        for (int j = 0; j < 4; j++) v[j] = buf_load1(r, j < n ? o + 4u * j : BUF_OOB);
        return v;
    };
    const uint32_t img_bytes = (uint32_t)HW * GS(in_cs) * 4u;
    // tile LN2 gamma/beta (image-independent) and the first image's raw quads, all in flight together
    f4 gq[GC_GQ], bq[GC_GQ], xq[PD][GC_GQ];   // xq: a ring of PD images' raw quads
#pragma unroll
    for (int u = 0; u < GC_GQ; u++) {
        gq[u] = ln ? load_q(buf_rsrc(a.gamma[net], img_bytes), u) : f4{1.f, 1.f, 1.f, 1.f};
        bq[u] = ln ? load_q(buf_rsrc(a.beta[net], img_bytes), u) : f4{0.f, 0.f, 0.f, 0.f};
    }
    auto load_img = [&](int ii, f4 (&xd)[GC_GQ]) {
        const auto r = buf_rsrc(a.in[net] + (size_t)(img0 + ii) * HW * GS(in_cs), img_bytes);
#pragma unroll
        for (int u = 0; u < GC_GQ; u++) xd[u] = load_q(r, u);
    };
    // LN2(LeakyReLU(t1)) of the quads in xq -> the three bf16 planes of band buffer (ii & 1); zero
    // outside the image / window
    auto store_img = [&](int ii, const f4 (&xs)[GC_GQ]) {
        const float rs = ln ? lstat[2 * ii + 1] : 1.f;
        const float mu = ln ? lstat[2 * ii] : 0.f;   // (as k_pw)
        unsigned char* dst = smem + (ii & 1) * GS(band_bytes);
#pragma unroll
        for (int u = 0; u < GC_GQ; u++) {
            if (loff[u] < 0) continue;
            f4 v = f4{0.f, 0.f, 0.f, 0.f};
            if ((nv[u] & 7) != 0) {
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const float t = lrelu(xs[u][j]);
                    v[j] = ln ? fmaf((t - mu) * rs, gq[u][j], bq[u][j]) : t;
                }
            }
            bf16x4 h, m, l;
            split4(v, h, m, l);
            unsigned char* d = dst + loff[u];
            if (nv[u] & 16) {
                *reinterpret_cast<bf16x2*>(d) = __builtin_shufflevector(h, h, 0, 1);
                *reinterpret_cast<bf16x2*>(d + lpb[u]) = __builtin_shufflevector(m, m, 0, 1);
                *reinterpret_cast<bf16x2*>(d + 2 * lpb[u]) = __builtin_shufflevector(l, l, 0, 1);
            } else {
                *reinterpret_cast<bf16x4*>(d) = h;
                *reinterpret_cast<bf16x4*>(d + lpb[u]) = m;
                *reinterpret_cast<bf16x4*>(d + 2 * lpb[u]) = l;
            }
        }
    };
    load_img(0, xq[0]);
    f4 xq2[GC_GQ];   // (image pairs: the second image of the group)
    if (PAIRS && 1 < nimg) load_img(1, xq2);
    // this wave's first LN2 image: partial slots fetched in the same memory round trip as the band
    // and weight loads (folded below)
    ConvProb lnP;
    lnP.in_part = a.in_part[net];
    lnP.in_nparts = a.in_nparts;
    lnP.part_stride = a.part_stride;
    const bool lnpre = ln && wave < nimg;
    const LnSlots slot0 = lnpre ? in_ln_fetch(lnP, img0 + wave) : LnSlots{};
    // weight planes, biases and K-octet offset tables of every branch (once per workgroup). From the
    // plan's plane image (a.w6: planes, then the table, as they lie in LDS from w_off on), copied with every
    // branch's loads in flight before the first LDS write; or (debug option PRESPLIT=0, a.w6 null) split
    // from the fp32 image, the table computed
    if (a.w6[net][0] != nullptr) {
        if constexpr (SID >= 0) {
            constexpr int NBR = kGcShapes[SID >= 0 ? SID : 0].nbr, MU = gc_copy_units(kGcShapes[SID >= 0 ? SID : 0], GC_NT);
            f4 wv[NBR][MU];
#pragma unroll
            for (int bi = 0; bi < NBR; bi++) {
                const int n16 = gc_w16(GS(br)[bi]);
                const auto r = buf_rsrc(a.w6[net][bi], (uint32_t)n16 * 16u);
#pragma unroll
                for (int u = 0; u < MU; u++)
                    if (u * GC_NT < n16) wv[bi][u] = buf_load4(r, (uint32_t)(tid + u * GC_NT) * 16u);
            }
#pragma unroll
            for (int bi = 0; bi < NBR; bi++) {
                const int n16 = gc_w16(GS(br)[bi]);
#pragma unroll
                for (int u = 0; u < MU; u++)
                    if (u * GC_NT < n16 && tid + u * GC_NT < n16)
                        *reinterpret_cast<f4*>(smem + GS(br)[bi].w_off + (tid + u * GC_NT) * 16) = wv[bi][u];
            }
        } else {
            for (int bi = 0; bi < GS(nbr); bi++)
                stage_copy16<GC_NT, 0>(a.w6[net][bi], smem + GS(br)[bi].w_off, gc_w16(GS(br)[bi]));
        }
    } else {
        for (int bi = 0; bi < GS(nbr); bi++) {
            const GcBranch& br = GS(br)[bi];
            stage_gcw_x6<GC_NT>(a.w[net][bi], smem + br.w_off, br, (br.cout + 15) >> 4);
            int4* ot = reinterpret_cast<int4*>(smem + br.q_off);
            for (int e = tid; e < 4 * br.G; e += GC_NT)
                ot[e] = make_int4(gc_octet_word(br.S, br.dil, br.BW, e, 0), gc_octet_word(br.S, br.dil, br.BW, e, 1),
                                  gc_octet_word(br.S, br.dil, br.BW, e, 2), gc_octet_word(br.S, br.dil, br.BW, e, 3));
        }
    }
    for (int bi = 0; bi < GS(nbr); bi++) {
        const GcBranch& br = GS(br)[bi];
        for (int i = tid; i < br.cout; i += GC_NT) reinterpret_cast<float*>(smem + br.b_off)[i] = a.b[net][bi][i];
    }
    GSTAMP(gs++);   // (diagnostic builds: band / gamma / beta / weight loads landed)
    // per-image LN2 (mean, rstd) from the producer's partials
    if (ln) {
        for (int i = wave; i < nimg; i += GC_NW) {
            float mu, rs;
            if (i == wave && lnpre)
                in_ln_finish(lnP, img0 + i, slot0, mu, rs);
            else
                in_ln(lnP, img0 + i, mu, rs);
            if (lane == 0) {
                lstat[2 * i] = mu;
                lstat[2 * i + 1] = rs;
            }
        }
    }
    __syncthreads();
    store_img(0, xq[0]);
    if (PAIRS && 1 < nimg) store_img(1, xq2);
    __syncthreads();
    GSTAMP(gs++);
    GWSTAMP(1);

    if constexpr (PAIRS) {
        const int jw = wave / NSUB;                       // 0 / 1: image of the pair, >= 2: no subtile
        const int vw = jw < 2 ? wave - jw * NSUB : NSUB;  // the wave's subtile (NSUB: none)
        for (int i0 = 0; i0 < nimg; i0 += 2) {
            // the next pair lands while this one is computed
            if (i0 + 2 < nimg) load_img(i0 + 2, xq[0]);
            if (i0 + 3 < nimg) load_img(i0 + 3, xq2);
            const int ii = i0 + jw;
            if (jw < 2 && ii < nimg) {
                LnAcc st;
                st.reset();
                bool first = true;
                float* outp = a.out[net] + (size_t)(img0 + ii) * HW * GS(out_cs);
                gc_branches<SID, 0>(a, smem, outp, npx, px0, r0, ph0, st, first, stats, jw * GS(band_bytes), vw);
                if (stats) st.write(a.out_part[net] + ((size_t)(img0 + ii) * a.part_stride + tile * GC_NW + vw) * LNP);
            }
            if (stats && wave >= NSUB && lane == 0)   // the slots of the waves without a subtile: empty
                for (int j = 0; j < 2 && i0 + j < nimg; j++)
                    *reinterpret_cast<f4*>(a.out_part[net] + ((size_t)(img0 + i0 + j) * a.part_stride + tile * GC_NW + wave) * LNP) =
                        f4{0.f, 0.f, 0.f, 0.f};
            if (i0 + 2 < nimg) {
                __syncthreads();   // both buffers read
                store_img(i0 + 2, xq[0]);
                if (i0 + 3 < nimg) store_img(i0 + 3, xq2);
                __syncthreads();
            }
        }
        return;
    }

    // the ring's other images (PD > 1)
#pragma unroll
    for (int j = 1; j < PD; j++)
        if (j < nimg) load_img(j, xq[j]);
    for (int i0 = 0; i0 < nimg; i0 += PD)
#pragma unroll
    for (int jj = 0; jj < PD; jj++) {
        const int ii = i0 + jj;
        if (ii >= nimg) break;
        const int img = img0 + ii;
        // lands while this image's MFMAs run: the next image (PD == 1), or image ii + PD into the
        // ring slot image ii (already staged) leaves
        if (PD == 1 && ii + 1 < nimg) load_img(ii + 1, xq[0]);
        if (PD > 1 && ii + PD < nimg) load_img(ii + PD, xq[jj]);
        LnAcc st;
        st.reset();
        bool first = true;
        float* outp = a.out[net] + (size_t)img * HW * GS(out_cs);
        const int boff = (ii & 1) * GS(band_bytes);
        if constexpr (SID >= 0) {
            gc_branches<SID, 0>(a, smem, outp, npx, px0, r0, ph0, st, first, stats, boff, wave);
        } else {
            for (int bi = 0; bi < GS(nbr); bi++) {
                const GcBranch& br = GS(br)[bi];
                const float* bias = reinterpret_cast<const float*>(smem + br.b_off);
                switch ((br.cout + 15) >> 4) {
                    case 1: gc_branch<1, SID, -1>(a, br, smem, bias, outp, npx, px0, r0, ph0, st, first, stats, boff, wave); break;
                    case 2: gc_branch<2, SID, -1>(a, br, smem, bias, outp, npx, px0, r0, ph0, st, first, stats, boff, wave); break;
                    case 3: gc_branch<3, SID, -1>(a, br, smem, bias, outp, npx, px0, r0, ph0, st, first, stats, boff, wave); break;
                    default: gc_branch<4, SID, -1>(a, br, smem, bias, outp, npx, px0, r0, ph0, st, first, stats, boff, wave); break;
                }
                GSTAMP(gs++);
            }
        }
        if (stats) st.write(a.out_part[net] + ((size_t)img * a.part_stride + tile * GC_NW + wave) * LNP);
        // every wave's MFMAs of this image done before any wave stages the next one into the other
        // buffer. Without this barrier the shape-specialised instantiations whose waves do not all
        // compute (cfg5's 64-pixel dil-1 tile: 4 of 16 waves) gave run-to-run different t2 on the
        // second image of a workgroup (cfg5 B >= 2: zy 2e-2 off the oracle); the generic and the
        // runtime-shape builds of the same code, and this one with the barrier, are exact
        if (ii + 1 < nimg) {
            __syncthreads();
            store_img(ii + 1, xq[(jj + 1) % PD]);
        }
        __syncthreads();
        GSTAMP(gs++);
        GWSTAMP(2 + ii);
    }
#ifdef CNF_GC_STAMPS
    if (threadIdx.x == 0 && blockIdx.x == 0 && blockIdx.y == 0) g_gc_stamps[63] = gs;
#endif
}

int read_gc_stamps(long long* host, int n) {
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_gc_stamps), sizeof(long long) * (n > 64 ? 64 : n)) == hipSuccess ? 0 : -1;
}

template <int S>
bool launch_gc_shape(int sid, const GcArgs& a, dim3 grid, int lds, hipStream_t st) {
    if constexpr (S < CNF_GC_NSHAPES) {
        if (sid == S) {
            CNF_LAUNCH((k_gc<S>), grid, dim3(64 * kGcShapes[S].nw), lds, st, a);
            return true;
        }
        return launch_gc_shape<S + 1>(sid, a, grid, lds, st);
    }
    return false;
}

int gc_num_shapes() { return CNF_GC_NSHAPES; }

// table entry matching a's shape, -1 for the generic instantiation
static int gc_shape_id(const GcArgs& a) {
    const bool generic = (opts().generic & 5) != 0;   // debug option GENERIC bit 1 (all) or 4 (k_gc)
#ifdef CNF_DIAG
    const char* only = std::getenv("CNF_GC_ONLY_SID");   // diagnostic builds: one specialised instantiation
#endif
    if (!generic)
        for (int sid = 0; sid < CNF_GC_NSHAPES; sid++) {
#ifdef CNF_DIAG
            if (only && std::atoi(only) != sid) continue;
#endif
            if (std::memcmp(&a.s, &kGcShapes[sid], sizeof(GcShape)) == 0) return sid;
        }
    return -1;
}

int gc_waves(const GcArgs& a) {
    const int sid = gc_shape_id(a);
    return sid >= 0 ? kGcShapes[sid].nw : GC_NW_GEN;
}

void launch_gc(const GcArgs& a, int grid_x, int lds, hipStream_t st) {
    const dim3 grid(grid_x, 2);
    const int sid = gc_shape_id(a);
    if (sid >= 0 && launch_gc_shape<0>(sid, a, grid, lds, st)) return;
    CNF_LAUNCH((k_gc<-1>), grid, dim3(64 * GC_NW_GEN), lds, st, a);
}

}  // namespace cnf
