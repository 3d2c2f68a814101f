// cnf_kernels.h — kernel argument blocks and launch helpers (host <-> device contract).
#pragma once

#include <cstddef>

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <cstdint>
#include <cstdlib>

#include "../../include/cnf.h"   // cnf_optim_desc

namespace cnf {

constexpr float LRELU_ALPHA = 0.3f;      // keras.layers.LeakyReLU() default
constexpr float LN_EPS = 1e-3f;          // keras.layers.LayerNormalization() default
constexpr double LOG_2PI_D = 1.8378770664093453;
// LayerNorm statistics partial of one producing wave: (K, S1, S2, n) with S1 = sum(x - K),
// S2 = sum((x - K)^2) over its n values of LeakyReLU(out), K a sample of them (fp32, 16 bytes)
constexpr int LNP = 4;
// LN partial slots per image a consumer wave folds from its prologue loads, per lane (cnf_device.h
// in_ln_fetch); producers of more than 64 * LN_FETCH slots get a k_ln_merge launch (cnf_coupling.cpp)
constexpr int LN_FETCH = 8;

constexpr int MAXPROB = 12;

// Debug options of a plan: cnf_flow_desc.debug_options, "NAME=V[,NAME=V...]" (include/cnf.h). They
// select the alternative code paths the parity tests compare against the default ones; the library
// reads no environment variable, and the defaults are what bench.py measures.
struct Options {
    int netlds = 1;          // NETLDS: 0 = no LDS-resident (k_net_lds) layers, every layer streamed
    int gc = 1;              // GC: 0 = no fused k_gc stage (grouped branches as k_pw tap mode / k_conv<3>)
    int pw = 1;              // PW: 0 = the per-tile k_conv1 / k_conv<3> kernels and the one-kernel k_convtap conv_out
#ifndef CNF_DIAG_GENERIC
#define CNF_DIAG_GENERIC 0   // (diagnostic builds: a different default for A/B runs of the unmodified tests)
#endif
    int generic = CNF_DIAG_GENERIC;   // GENERIC bits: never the shape-specialised instantiations of 1 any kernel, 2 k_pw, 4 k_gc, 8 k_net_lds
    int layout = 7;          // LAYOUT bits: 1 compact t1 sub-tensors, 2 mapped t2 sub-tensors, 4 polyphase k_gc tiles
    int fuse_coupling = 1;   // FUSE_COUPLING: 0 = every coupling layer launches its own k_coupling
    int lds_bwd = 2;         // LDS_BWD: 0 multi-kernel backward of the k_net_lds layers, 1 fused (one launch), 2 fused split
    int presplit = 1;        // PRESPLIT: 0 = no bf16x6 plane image in aux, k_pw / k_gc split their fp32 weight images in every workgroup
    int train_alt = 0;       // TRAIN_ALT: a sum of the ALT_* bits below
    int train_sched = 0;     // TRAIN_SCHED: a sum of the SCHED_* bits below
    // SCHEDULE_CHECK: 1 = cnf_plan_create dry-runs the forward / inverse schedule and refuses a flow they
    // cannot run; 0 = the plan tables alone (such a plan fails in its first forward or inverse). Unset (-1):
    // 1 for CNF_GROUP_REFERENCE, 0 for CNF_GROUP_INTENDED, whose plans of flows with streamed layers
    // (dense grouped image over the LDS budget) serve host-side table checks; cFlow always asks for 1
    int schedule_check = -1;
};
// TRAIN_ALT bits: alternative training kernels, each the reference of a parity test or a fallback
enum : int {
    ALT_VALU = 1,            // every training convolution on the register-blocked VALU kernels (k_tconv, k_wgrad)
    ALT_WGRAD_BAND = 2,      // LDS-staged band weight gradients (k_wgrad_band) instead of k_wgrad_direct
    ALT_NO_TCONV_BAND = 4,   // no band-staged 3x3 transposed convolution (k_tconv_band)
    ALT_NO_THIN = 8,         // no thin-channel kernels (k_tconv_thin, k_wgrad_thin): the MFMA kernels take those convs
    ALT_LNB_REDUCE = 16,     // the LN backward's reduction as its own kernel (k_lnb_reduce), not in the producing data gradient
    ALT_ZERO_DT1 = 32,       // dt1's gradient buffer zeroed before the grouped branches instead of the LN2 channel mask
};
// TRAIN_SCHED bits: how the streamed layers' backward is scheduled
enum : int {
    SCHED_WGRAD_ON_CHAIN = 1,   // weight gradients on the chain streams (no weight-gradient streams)
    SCHED_RECOMPUTE = 2,        // recompute the streamed layers' activations in the backward (the forward saves none)
    SCHED_NET_OUTER = 4,        // enqueue net A's whole chain before net b's (no interleaving)
};
// parses a debug_options string (null / empty: defaults); throws std::invalid_argument on an unknown
// name or a malformed value (cnf_runtime.cpp)
Options parse_options(const char* s);
// the options of the plan the calling thread's current C-ABI call runs (defaults outside one)
const Options& opts();
struct OptScope {   // sets opts() for the duration of one C-ABI call
    const Options* prev;
    explicit OptScope(const Options* o);
    ~OptScope();
};

// Launch timing (bench.py via cnf_plan_set_launch_timing): while a pair is armed, the launch
// helpers dispatch through hipExtLaunchKernelGGL, which stores the kernel's own begin / end
// timestamps (the dispatch packet's profiling timestamps, as rocprofv3 reads them) into the
// events: no extra packets between the kernels, so the stream runs as it does untimed.
struct LaunchTiming {
    hipEvent_t start = nullptr, stop = nullptr;
    int used = 0;   // kernels that wrote the pair (the last one's times are kept)
};
LaunchTiming& launch_timing();   // per host thread (cnf_runtime.cpp)
#define CNF_LAUNCH(K, G, B, L, S, ...)                                                              \
    do {                                                                                            \
        ::cnf::LaunchTiming& lt_ = ::cnf::launch_timing();                                          \
        if (lt_.start != nullptr) {                                                                 \
            hipExtLaunchKernelGGL(K, G, B, L, S, lt_.start, lt_.stop, 0, __VA_ARGS__);              \
            lt_.used++;                                                                             \
        } else {                                                                                    \
            hipLaunchKernelGGL(K, G, B, L, S, __VA_ARGS__);                                         \
        }                                                                                           \
        CNF_DIAG_SYNC(S);                                                                           \
    } while (0)
#ifdef CNF_DIAG   // diagnostic builds: CNF_SYNC_ALL=1 synchronises the stream after every launch
#define CNF_DIAG_SYNC(S)                                                                            \
    do {                                                                                            \
        static const bool sync_ = std::getenv("CNF_SYNC_ALL") != nullptr;                          \
        if (sync_) (void)hipStreamSynchronize(S);                                                   \
    } while (0)
#else
#define CNF_DIAG_SYNC(S) do { } while (0)
#endif

// packed weight-image formats (see cnf_plan.h PackedConv)
enum { PK_1X1 = 0, PK_KN = 1, PK_TAP = 2, PK_Q4 = 3 };

// kernel roles: distinct symbols so per-kernel profiles separate the ResNeXt stages
enum { ROLE_CONV_IN = 0, ROLE_CONV_A = 1, ROLE_GC = 2, ROLE_CONV_B = 3, ROLE_CONV_OUT = 4 };

// One convolution problem of a k_conv launch (blockIdx.y selects the problem).
struct ConvProb {
    const float* in;          // NHWC, image 0
    const float* in_part;     // LN partials (K, S1, S2, n) of the input tensor [B][part_stride][LNP] (first
                              // in_nparts slots valid), or null (no LN)
    const float* gamma;       // LN gamma over the full in_cs-channel tensor (per h,w,c)
    const float* beta;
    const float* wt;          // pre-packed weight image (PK_1X1 / PK_KN / PK_TAP)
    const float* bias;        // [cout]
    const float* res;         // residual, same layout as out, or null
    float* out;
    float* out_part;          // per-wave LN partials of LeakyReLU(out) [B][part_stride][LNP], or null
    int in_cs, in_off, cin, in_nparts;
    int out_cs, out_off, cout, part_stride, out_part_base;
    int dil, act;
    int lds_in_off, lds_w_off, lds_k_off;  // byte offsets in dynamic LDS
    int S, Kpad, NS, nr;                   // LDS pixel stride, padded K, B row stride, N-subtiles
    uint32_t cin_mag, wp_mag;              // magic multipliers: x / cin == umulhi(x, cin_mag) (3x3 staging)
    uint32_t st_mask_lo, st_mask_hi;       // output channels actually stored (bit per channel < 64)
    int st_compact;                        // 1: stores through st_map (k_pw only)
    const int* st_map;                     // [64][2]: channel -> (offset of pixel 0 inside the image, pixel stride) in floats, offset < 0: not stored
    int in_mapped;                         // 1: A-operand quads through in_map (k_pw only; in_cs = floats per pixel of an image)
    const int* in_map;                     // [quad][2]: input channel quad -> (offset of pixel 0 inside the image, pixel stride)
    float* out2;                           // k_pw only: also every output channel, plain [B][HW][cout] (null: none) —
                                           // the training forward's full t1 next to conv_a's mapped stores
    const void* wx6;                       // k_pw only: the conv's bf16x6 plane image (x6_at; null: staged from wt)
};

struct ConvArgs {
    ConvProb p[MAXPROB];
    int H, W, TH, tiles_per_img, nprob, B;
    int P;     // 1x1 kernels: pixels per tile (tiles are runs of pixels inside one image)
    int ipw;   // k_pw: images per workgroup (looped, next image prefetched)
    // k_pw tap mode (streamed conv_in): the A operand is the im2col row of a 3x3 conv over the
    // mask-compressed half of the raw layer input u, gathered straight from u (no u1c tensor):
    // K index k = tap * udc + c, c < udc, pixel shifted by the tap, zero outside the image
    int umask, uW, uD, udc, uimg;   // mask, full-res width / depth, channels per tap, floats per image
    // umask < 0: the source is a plain NHWC tensor of the conv's own H x W (uD channels per pixel,
    // taps from channel uoff, dilation udil; LN / LeakyReLU on load as the problem says)
    int udil, uoff;
    int diag;   // -DCNF_DIAG builds only: k_pw experiment bits (CNF_PW_DIAG)
};

struct CoupArgs {
    const float* u;
    float* v;
    const float* s_pre;      // raw conv_out of net A (before tanh)
    const float* t;          // conv_out of net b
    const float* tanh_w;     // device scalar
    double* ld_part;         // [B][gridDim.x] or null
    int H, W, D, mask, mask_c, hc, wc, dc1, dc2, dir;
    // tap mode (tc[0] != null): s_pre / t are the 3x3 conv_out finished here from the tap GEMM
    // C[img][p][(tap, o)] (row stride 9*dc2) of each net, plus bias, and also written to
    // so_w[net] (the raw conv_out the training path reads)
    const float* tc[2];
    const float* tbias[2];
    float* so_w[2];
};

// Whole s,t network of one coupling layer in LDS (cnf_netlds.hip); grid (B, 2 nets).
constexpr int NETLDS_MAXBR = 8;
#ifndef CNF_NETLDS_OTAB
#define CNF_NETLDS_OTAB 192
#endif
constexpr int NETLDS_OTAB = CNF_NETLDS_OTAB;   // byte offset of the parameter-offset table (after the LN slots)
// one conv of k_net_lds: packed format (PK_*), image floats, K extent (PK_KN: padded K; PK_Q4:
// 16 * groups), B row stride (PK_KN)
struct LdsConv {
    int fmt, size, kpad, ns;
};

// A coupling law left pending by the previous layer (forward only): k_net_lds of layer k+1 applies
// layer k's affine law itself (conv_cINN_make_model.py:1215-1233, 1258-1328) — on the fly in its u1c
// gather, and for the whole v_k (split between its two workgroups) with layer k's log-det partials —
// so layer k needs no k_coupling launch. Same arithmetic as k_coupling, element for element.
struct CoupPend {
    const float* u = nullptr;       // u_k [B][H][W][D] (layer k's input; H, W, D as layer k+1's)
    const float* s_pre = nullptr;   // layer k's raw net-A conv_out (pre-tanh) [B][hc][wc][dc2]
    const float* t = nullptr;       // layer k's net-b conv_out
    const float* tanh_w = nullptr;  // layer k's tanh scale
    float* v = nullptr;             // v_k (== layer k+1's u)
    double* ld_part = nullptr;      // layer k's log-det partial slots [B][np]
    int mask_c = 0, hc = 0, wc = 0, dc2 = 0, np = 0, on = 0;
    // comp: layer k+1 conditions on exactly layer k's transformed half (mask_{k+1} == layer k's
    // complement mask, same compressed layout): its u1c gather then yields that half of v_k as is
    // (net A's workgroup stores it with the log-det sum), and net b's copies the other half (layer
    // k's conditioning half, mask / dc1) from u_k — no pass over v_k at the end of the kernel
    int comp = 0, mask = 0, dc1 = 0;
    int W = 0, D = 0;   // u_k's width and depth (k_map2 applies a pending coupling of the last layer of a block)
    // +1: the forward law v2 = exp(s) u2 + t (ld_part collects layer k's sum of s); -1: the inverse
    // law u2 = (1 / exp(s)) (v2 - t) of cnf_flow_inverse (ld_part null) / cnf_flow_inverse_logdet
    // (ld_part collects the same sum of s; the reduction negates it). In the inverse schedule
    // "layer k" is the layer just run and "k+1" the one before it in index order, run next.
    int dir = 1;
};

// fp32 constants of the reference's logit map (preprocess_dataset_class, conv_cINN_base_functions.py
// :174-231; TF evaluates the Python-float constants in fp32): c1 = (1-a) b, lo = logit(a),
// span = logit(1-a) - logit(a), inv_bc = 1 / (b (1 - a)) (cnf_transforms.hip logit_consts)
struct LogitK {
    float a, c1, lo, span, inv_bc;
};
// the flow's input as the reference pipeline builds it from the raw xy (conv_cINN.py:246-315): the
// logit map on the x channels (ch < x_d, logit != 0), then instance noise alpha v + (1 - alpha) N(0,1)
// on every channel (cnf_device.h input_prep_value)
struct InputPrepArgs {
    const float* src;   // the raw xy (null: no preparation)
    float alpha;
    unsigned long long seed, off;
    int logit, x_d, D;
    LogitK lk;
};

LogitK logit_consts(float a);   // cnf_transforms.hip
void launch_input_prep(float* out, long long n, const InputPrepArgs& q, hipStream_t st);   // k_prep

struct NetLdsArgs {
    const float* u;           // layer input [B][H][W][D]
    float* so[2];             // outputs: raw conv_out of net A (pre-tanh) / net b, [B][hc][wc][dc2]
    const float* params;      // canonical parameters
    const float* aux;         // dense grouped-conv image
    const int* offs;          // [2][offs_per_net] parameter offsets (see k_net_lds)
    int offs_per_net;
    int H, W, D, mask, hc, wc, dc1, dc2, nk, gc, R, nbr, ln;
    int br_cin_off[NETLDS_MAXBR], br_cin[NETLDS_MAXBR], br_cout[NETLDS_MAXBR], br_out_off[NETLDS_MAXBR],
        br_dil[NETLDS_MAXBR];
    int nwin, win_off[NETLDS_MAXBR], win_len[NETLDS_MAXBR];  // disjoint union of the branch input windows
    int sy, s1, s2, su;                          // LDS pixel strides (floats)
    LdsConv ci, ca, cb, co, gcv[NETLDS_MAXBR];   // packed images of conv_in, conv_a, conv_b, conv_out, branches
    const float* zero_bias;                      // >= 128 zeros (tap GEMM has no bias)
    int off_y, off_t1, off_t2, off_w, off_k;     // LDS byte offsets
    int off_ks;                                  // K-split partial buffers (0: the image has > 4 subtiles)
    int maxnr;                                   // widest conv's 16-column output blocks (picks the instantiation)
    int stamp_off;                               // diagnostic stamp builds: LDS byte offset of the stamp array
    CoupPend pend;                               // previous layer's deferred coupling (pend.on)
    int ci_off[2];                               // conv_in image offset in aux per net (offs[net][0]): its
                                                 // prefetch starts before the offset table is staged
    // training forward (cnf_flow_forward_train): the raw activations and LN statistics the fused
    // backward (k_lds_bwd) reads, one LdsSave block of save_img floats per (net, image), [net][B]
    // (null: inference)
    float* save;
    int save_img, save_t1, save_t2, save_st;
    // fused input preparation (cnf_flow_forward_noise, first coupling only): the u1c gather reads
    // nz.src and applies input_prep_value (logit on the x channels, instance noise of stream element
    // nz.off + flat batch index), and u (then the prepared xy, written here) receives every element
    // of the image: net A's workgroup the gathered half, net b's the transformed half. nz.src null:
    // u is read as is
    InputPrepArgs nz;
};

// Block of one (net, image) in a k_net_lds layer's training save area (all float offsets):
//   y_r  [HW][nk] at r * HW * nk                 (r = 0..R: conv_in's output, then each block's output)
//   t1_r [HW][nk] at t1 + r * HW * nk            (conv_a's raw output)
//   t2_r [HW][gc] at t2 + r * HW * gc            (the grouped stage's raw concat)
//   (mean, rstd) at st: LN1_r at 2r, LN2_r at 2(R + r), LN3_r at 2(2R + r), LN_out at 6R
struct LdsSave {
    int img = 0, t1 = 0, t2 = 0, st = 0;
    static LdsSave of(int HW, int nk, int gc, int R) {
        LdsSave s;
        s.t1 = (R + 1) * HW * nk;
        s.t2 = s.t1 + R * HW * nk;
        s.st = s.t2 + R * HW * gc;
        s.img = (s.st + 2 * (3 * R + 1) + 3) / 4 * 4;
        return s;
    }
};
// The launch-independent "shape" of a k_net_lds launch as int words: [offs_per_net, zero_bias) and
// [off_y, stamp_off) of NetLdsArgs (the mask word inside is not part of it). Shape-specialised
// instantiations take these words as compile-time constants (cnf_netlds_shapes.inc).
constexpr int NETSHAPE_W1 = (int)((offsetof(NetLdsArgs, zero_bias) - offsetof(NetLdsArgs, offs_per_net)) / 4);
constexpr int NETSHAPE_W2 = (int)((offsetof(NetLdsArgs, stamp_off) - offsetof(NetLdsArgs, off_y)) / 4);
constexpr int NETSHAPE_WORDS = NETSHAPE_W1 + NETSHAPE_W2;
static_assert(offsetof(NetLdsArgs, gcv) + sizeof(LdsConv) * NETLDS_MAXBR - offsetof(NetLdsArgs, offs_per_net) == 4 * 123,
              "gen_netlds_shapes.py assumes 123 int members in [offs_per_net, zero_bias)");
constexpr int NETSHAPE_MASK = (int)((offsetof(NetLdsArgs, mask) - offsetof(NetLdsArgs, offs_per_net)) / 4);
inline void netshape_words(const NetLdsArgs& a, int* w) {
    const int* p1 = &a.offs_per_net;
    const int* p2 = &a.off_y;
    for (int i = 0; i < NETSHAPE_W1; i++) w[i] = p1[i];
    for (int i = 0; i < NETSHAPE_W2; i++) w[NETSHAPE_W1 + i] = p2[i];
    w[NETSHAPE_MASK] = 0;
}
// The bf16x6 plane image of a conv's weights W[k][col] (cnf_stream.hip: what k_pw and k_gc keep in LDS, and
// what the plan appends to aux per streamed conv so that staging is a copy): K in 32-deep steps c, NR
// 16-column blocks nb, planes p = 0, 1, 2 (h, m, l of split3); 1 KiB per (c, p, nb), in which lane
// (kq, i16) owns the 16 bytes of W[32c + 8kq + jj][16nb + i16], jj < 8. The one statement of the layout:
// the plan's plane map and the kernels' fp32 staging both place an element with it.
__host__ __device__ constexpr int x6_at(int k, int col, int p, int NR) {
    return (((k >> 5) * 3 + p) * NR + (col >> 4)) * 1024 + ((((k >> 3) & 3) << 4) + (col & 15)) * 16 + (k & 7) * 2;
}
constexpr int64_t x6_bytes(int C, int NR) { return (int64_t)C * 3 * NR * 1024; }
// k_gc's K-octet table (4 G entries of four ints, right behind a branch's planes in LDS and in aux): word j
// of octet e (k = 8e .. 8e + 7, k = tap * S + ch) is the band offset, in bf16 elements from the pixel's
// tap-(0, 0) origin, of the octet's j-th tap: one tap (S >= 8), two (S = 4) or four (S = 2); 0 for unused
// words and past the 9 taps (their weights are zero: any in-band address is fine)
__host__ __device__ constexpr int gc_octet_word(int S, int dil, int BW, int e, int j) {
    const int per = S >= 8 ? 1 : 8 / S;
    if (j >= per) return 0;
    const int tap = S >= 8 ? 8 * e / S : per * e + j;
    if (tap >= 9) return 0;
    return ((tap / 3) * dil * BW + (tap % 3) * dil) * S + (S >= 8 ? 8 * e - tap * S : 0);
}
// k_gc (cnf_stream.hip): every grouped dilated branch of one residual block for a tile of TH
// image rows of one net, `ipw` images per workgroup. Branch input windows are staged into LDS
// bands with their own dilation halo (LN2 + LeakyReLU applied on the way in, zero padding), so
// the 3x3 taps need no bounds checks; weights are PK_Q4 over cin padded to a multiple of 4.
constexpr int GC_MAXBR = 8;
// waves per k_gc workgroup (one LN partial slot per wave): the shape-specialised instantiations run
// 16 (one 16-pixel subtile per wave and pass, 4 waves per SIMD within 128 VGPRs; 8 waves with two
// subtiles sharing every weight read measured slower with the bf16x6 contraction: 26.2 -> 29.7 us at
// cfg2), small polyphase groups 4-wave workgroups, four per CU; the generic one 8 (two subtiles per wave)
constexpr int GC_NW_GEN = 8, GC_NW_SPEC = 16, GC_NW_MAX = 16;
constexpr int GC_STAGE_QUADS = 2048;   // staged band units per workgroup (2 per thread at 16 waves)
// LDS budget and staged band units of a k_gc workgroup of nw waves (1 workgroup per CU at >= 8 waves,
// 4 at 4)
constexpr int gc_lds_budget(int nw) { return nw >= 8 ? 160 * 1024 : 40 * 1024; }
constexpr int gc_stage_units(int nw) { return nw >= 8 ? 2048 : 2 * 64 * nw; }
constexpr int gc_wg_per_cu(int nw) { return nw >= 8 ? 1 : 4; }
struct GcBranch {
    int cin_off, cin, cinp, cout, out_off, dil;   // input window (cin_off: floats from the image start to pixel 0's window), padded channels, outputs
    int G;                                        // quad groups of the PK_Q4 image
    int band_off, BW, BH, S;                      // LDS band: byte offset, width, height, pixel stride
    int w_off, q_off, b_off;                      // LDS byte offsets: packed weights, quad offsets, bias
    int pcs;                                      // pixel stride of the input window (floats)
    int opcs;                                     // pixel stride of the output slice (out_off: floats from the image start to pixel 0's slice)
    uint32_t cpq_mag, bw_mag;                     // x / (cinp/4) == umulhi(x, cpq_mag) (cinp > 4), x / BW likewise
};
struct GcShape {
    GcBranch br[GC_MAXBR];
    int nbr, H, W, in_cs, out_cs, TH, tiles_per_img;
    int TW, tiles_x;             // tile width (W, or a divisor of W for wide images) and column tiles
    int band_bytes;              // offset of the second band buffer (double-buffered staging)
    int lnst;                    // bit 0: LN2 on load (in_part set), bit 1: LN3 partials out (out_part set)
    // polyphase tiles (ps > 1, one branch of dilation ps): the image splits into ps*ps phase grids
    // (pixels a + i*ps, b + j*ps) of (H/ps) x (W/ps), on which the dilated conv is a dilation-1 conv;
    // a tile is nbk whole phase grids (TH x TW each, nbk > 1) or a TH-row slice of one (tpp slices per
    // grid), its band one (TH+2) x (TW+2) block per grid: the halo of the dilation no longer scales
    // with ps
    int ps, nbk, tpp;
    int nw;                      // waves per workgroup of the shape-specialised instantiation (16, or 4 for
                                 // small bands: four workgroups per CU hide each other's per-image latency)
    int pd;                      // images whose band quads are in flight (registers) ahead of the one computed
};
constexpr int GCSHAPE_WORDS = (int)(sizeof(GcShape) / 4);
struct GcArgs {
    const float* in[2];          // t1 per net [B][HW][in_cs]
    float* out[2];               // t2 per net [B][HW][out_cs]
    const float* in_part[2];     // LN2 partials of t1 (null: no LN)
    float* out_part[2];          // LN3 partials of LeakyReLU(t2)
    const float* gamma[2];       // LN2 gamma/beta [HW][in_cs]
    const float* beta[2];
    const float* w[2][GC_MAXBR];   // per k_gc branch (GcShape.br order)
    const float* b[2][GC_MAXBR];
    const void* w6[2][GC_MAXBR];   // per branch: bf16x6 plane image + K-octet table (x6_at, gc_octet_word), or null: built from w
    GcShape s;                   // launch-independent part (compile-time in the shape-specialised kernels)
    int B, ipw, in_nparts, part_stride;
};
void launch_gc(const GcArgs& a, int grid_x, int lds, hipStream_t st);
int gc_waves(const GcArgs& a);   // waves per workgroup of the instantiation launch_gc picks for a
int read_gc_stamps(long long* host, int n);
int gc_num_shapes();   // shape-specialised k_gc instantiations compiled in
// k_toy (cnf_toy.hip): TOYcINN dense flow, one thread per 3-dimensional sample
constexpr int TOY_MAXL = 128;
// the toy flow as its three kernels read it: nl coupling networks of hidden width H and L hidden Dense
// layers over (x_d, 3 - x_d) points, run in the order `order`
struct ToyNet {
    int nl, H, L, x_d;
    int order[TOY_MAXL];        // mask_indices
    int net_off[TOY_MAXL + 1];  // float offset of network j's parameters; [nl]: the parameter count
};
// inputs of the nets of coupling network j (its mask's u1; they write the other 3 - n1 components). The
// device side of the rule: toy_mask, cnf_toy_device.h
constexpr int toy_n1(int j) { return (j % 6) < 3 ? 1 : 2; }
// workgroups over n samples (draws) in tiles of ts
constexpr int64_t toy_tiles(int64_t n, int ts) { return (n + ts - 1) / ts; }
struct ToyArgs {
    const float* params;   // canonical flat parameters (per network j: b-block then A-block)
    const float* u;        // [B][3]
    float* v;              // [B][3]
    float* log_detJ;       // [B] (direction -1) or null
    float* per_sample;     // [B][3] (llz, lly, log_detJ) of log_loss (direction -1) or null
    int B, dir;
    float lambda_y;
    ToyNet flow;
    float* save_u;         // [nl][B][3] input of every executed coupling layer, by step (training) or null
};
void launch_toy(const ToyArgs& a, int lds_floats, hipStream_t st);
// k_toy_bwd / k_toy_grad_sum (cnf_toy_train.hip): backward of the whole toy flow, one workgroup per
// TOY_TS consecutive samples, one partial gradient row per workgroup, then the tile-order sum
#ifndef CNF_TOY_TS
#define CNF_TOY_TS 16   // a multiple of 16; -DCNF_TOY_TS=32 / 64 builds the variants DESIGN.md compares
#endif
constexpr int TOY_TS = CNF_TOY_TS;
struct ToyBwdArgs {
    const float* params;
    const float* xy;       // [B][3]
    const float* zy;       // [B][3]
    const float* saved_u;  // [nl][B][3], as ToyArgs::save_u wrote it
    float* part;           // [tiles][num_params]
    int B, HP, num_params;
    float lambda_y, inv_batch;
    ToyNet flow;
};
int toy_bwd_hp(int H);                   // LDS row stride of one sample's hidden vector
size_t toy_bwd_lds_bytes(int H, int L);  // dynamic LDS of k_toy_bwd
void launch_toy_bwd(const ToyBwdArgs& a, hipStream_t st);
void launch_toy_grad_sum(const float* part, int tiles, int num_params, float* dparams, hipStream_t st);
// k_toy_sample / k_toy_sample_stats (cnf_toy_sample.hip, cnf_toy_sample): one workgroup takes one tile of
// TOY_SAMPLE_TS consecutive draws of one condition from latent to result (tile = s / TOY_SAMPLE_TS; a
// condition's last tile is zero-padded) and leaves one shifted partial per component; the second kernel merges
// the partials in tile order
constexpr int TOY_SAMPLE_TS = 128;   // a multiple of 16
constexpr int TOY_SAMPLE_PART = 4;   // floats per partial: (n, K, S1, S2)
struct ToySampleArgs {
    const float* params;
    const float* y;        // [B][3 - x_d]
    float* samples;        // [B][S][x_d] or null
    float* y_dev;          // [B][S] or null
    unsigned* hist;        // [B][G] / [B][G][G] or null
    float* part;           // [B][tiles][x_d][TOY_SAMPLE_PART]
    int B, S, tiles, HP;
    float temperature;
    unsigned long long seed, offset;
    int G;                 // histogram bins per component
    float lo[2], scale[2];
    ToyNet flow;
};
size_t toy_sample_lds_bytes(int H);   // dynamic LDS of k_toy_sample
void launch_toy_sample(const ToySampleArgs& a, hipStream_t st);
void launch_toy_sample_stats(const float* part, int B, int tiles, int S, int x_d, float* mean, float* std,
                             hipStream_t st);
// k_toy_density / k_toy_density_mass (cnf_toy_density.hip, cnf_toy_density): one workgroup takes one tile of
// TOY_SAMPLE_TS consecutive points of one condition from xy to its log-density in direction -1 (tile =
// point / TOY_SAMPLE_TS; a condition's last tile is zero-padded) and leaves one log-sum-exp partial; the second
// kernel merges the partials in tile order
constexpr int TOY_DENSITY_PART = 2;   // floats per partial: (m, s)
struct ToyDensityArgs {
    const float* params;
    const float* y;        // [B][3 - x_d]
    const float* x;        // [B][N][x_d], or null: the centres of a grid of G bins per component
    float* log_prob;       // [B][N] or null
    float* y_dev;          // [B][N] or null
    float* z;              // [B][N][x_d] or null
    float* part;           // [B][tiles][TOY_DENSITY_PART], or null (log_mass not asked for)
    int B, N, tiles, HP;
    int G;                 // grid bins per component (0 with x)
    float lo[2], step[2];  // centre i of component c: lo[c] + (i + 0.5) step[c]
    ToyNet flow;
};
size_t toy_density_lds_bytes(int H);   // dynamic LDS of k_toy_density
void launch_toy_density(const ToyDensityArgs& a, hipStream_t st);
void launch_toy_density_mass(const float* part, int B, int tiles, double log_cell, float* log_mass, hipStream_t st);
void launch_nll_sums(const float* per_image, float* sums, int B, hipStream_t st);
void launch_net_lds(const NetLdsArgs& a, int B, int lds, hipStream_t st);
int netlds_num_shapes();   // shape-specialised k_net_lds instantiations compiled in
int read_stamps(long long* host, int n);
int read_cycles(long long* host, int n);

void launch_conv(int ks, int mr, int role, const ConvArgs& a, int grid_x, int lds, hipStream_t st);
void launch_conv1(int mr, bool vec, int role, const ConvArgs& a, int grid_x, int lds, hipStream_t st);
// k_pw launch shape: every launch-independent field a shape-specialised k_pw instantiation folds
// in (cnf_stream.hip; table generated by gen_netlds_shapes.py from a dry run of the forward)
struct PwShape {
    int nr, gm, ln, res, tap;            // template selection
    int H, W, tiles_per_img, nprob;
    int in_cs, in_off, cin, out_cs, out_off, cout, lds_w_off, part_stride;
    int umask, uW, uD, udc, uimg, udil, uoff;   // tap mode (0 otherwise)
    uint32_t st_mask_lo, st_mask_hi;
    int st_compact, in_mapped;
};
constexpr int PWSHAPE_WORDS = (int)(sizeof(PwShape) / 4);
// the shape of a k_pw launch; false when its problems differ in a shape field
inline bool pw_shape_of(int nr, int gm, bool ln, bool res, bool tap, const ConvArgs& a, PwShape& s) {
    const ConvProb& q = a.p[0];
    s = PwShape{nr, gm, ln ? 1 : 0, res ? 1 : 0, tap ? 1 : 0, a.H, a.W, a.tiles_per_img, a.nprob, q.in_cs, q.in_off,
                q.cin, q.out_cs, q.out_off, q.cout, q.lds_w_off, q.part_stride,
                tap ? a.umask : 0, tap ? a.uW : 0, tap ? a.uD : 0, tap ? a.udc : 0, tap ? a.uimg : 0,
                tap ? a.udil : 0, tap ? a.uoff : 0,
                q.st_mask_lo, q.st_mask_hi, q.st_compact, q.in_mapped};
    for (int i = 1; i < a.nprob; i++) {
        const ConvProb& r = a.p[i];
        if (r.in_cs != q.in_cs || r.in_off != q.in_off || r.cin != q.cin || r.out_cs != q.out_cs ||
            r.out_off != q.out_off || r.cout != q.cout || r.lds_w_off != q.lds_w_off || r.part_stride != q.part_stride ||
            r.st_mask_lo != q.st_mask_lo || r.st_mask_hi != q.st_mask_hi || r.st_compact != q.st_compact ||
            r.in_mapped != q.in_mapped)
            return false;
    }
    return true;
}
void launch_pw(int nr, int gm, bool ln, bool res, bool tap, const ConvArgs& a, int grid_x, int lds, hipStream_t st);
int pw_num_shapes();
int read_pw_stamps(long long* host);   // diagnostic builds (CNF_PW_STAMPS=SID): [2048 workgroups][12]
void launch_convtap(int mt, bool vec, const ConvArgs& a, int grid_x, int lds, hipStream_t st);
void launch_gather_u1c(const float* u, float* u1c, int B, int H, int W, int D, int mask, int hc, int wc, int dc1,
                       hipStream_t st);
void launch_coupling(const CoupArgs& a, int B, int nparts, hipStream_t st);
// out[img] (accumulate: +=) the sum of image img's slots part[nl][B][np]; negate: minus the sum
void launch_ld_reduce(const double* part, float* out, int B, int nl, int np, int accumulate, hipStream_t st,
                      int negate = 0);
// LN partial slots [B][part_stride][LNP] of one tensor (two nets: part0, part1 or null) merged into
// slot 0 of each image (k_ln_merge): consumers then read nparts = 1
void launch_ln_merge(float* part0, float* part1, int nparts, int part_stride, int B, hipStream_t st);
// (mean, rstd) [B][2] per net of up to LNF_MAX LN tensors from their producers' partial slots (as in_ln),
// one launch: tensor i's slots part[i][net] ([B][part_stride][LNP], nparts[i] used) -> st[i][net]
constexpr int LNF_MAX = 4;
struct LnFinalSet {
    const float* part[LNF_MAX][2];
    float* st[LNF_MAX][2];
    int nparts[LNF_MAX];
    int count, part_stride;
};
void launch_ln_final(const LnFinalSet& s, int B, hipStream_t st);
void launch_map_gather(const float* src, float* dst, const int* idx, int n, int ss, int ds, int B, hipStream_t st);
void launch_map_scatter(const float* src, float* dst, const int* sidx, const int* didx, int n, int ss, int ds,
                        int B, hipStream_t st);
// two independent index maps (+ optionally the per-image log-det reduction) in one launch:
// dst[b, didx ? didx[i] : i] = src[b, sidx ? sidx[i] : i] (a gather has didx == null, a scatter sidx
// == null or a source map). The forward's factor boundaries (keep gather + factored scatter) and its
// tail (final scatter + log-det reduction) each take one launch instead of two.
struct MapOp {
    const float* src = nullptr;
    float* dst = nullptr;
    const int* sidx = nullptr;
    const int* didx = nullptr;
    int n = 0, ss = 0, ds = 0;
    int pend = 0;   // k_map2: read the source through the launch's pending coupling (src is then unused)
};
struct LdReduce {
    const double* part = nullptr;   // null: no reduction
    float* out = nullptr;
    int nl = 0, np = 0, accumulate = 0;
};
// pend.on: the maps read v_k of a deferred coupling (computed from u_k, s, t on the fly; src is
// unused), and the extra block computes layer k's log-det sum — into its partial slots, or, with
// r.part, straight into the per-image total (r.nl then counts the layers before k)
void launch_map2(const MapOp& a, const MapOp& b, const LdReduce& r, const CoupPend& pend, int B, hipStream_t st);
void launch_squeeze(const float* in, float* out, int B, int H, int W, int C, int dir, hipStream_t st);
void launch_chcopy(const float* in, int in_cs, int in_off, float* out, int out_cs, int out_off, int C, long long npix,
                   hipStream_t st);
// per-image NLL terms and the batch sums in one launch; done: a zero-initialised device counter
// owned by the caller, left at 0 by every completed launch (concurrent launches need their own)
void launch_nll(const float* xy, const float* zy, const float* ld, float* per_image, float* sums, unsigned* done,
                int B, int HW, int D, int x_d, float lambda_y, hipStream_t st);
void launch_pack(const float* params, const int64_t* map, float* aux, long long n, hipStream_t st);
// the bf16x6 plane region of aux, one 16-bit unit per map entry (Plan::x6_map): 4 * parameter + plane (the
// plane's term of split3), -1: zero, <= -2: the literal -2 - entry (the K-octet tables' int halves)
void launch_pack_x6(const float* params, const int64_t* map, void* dst, long long n, hipStream_t st);

// ---- conditional sampling (cnf_sample.hip, cnf_flow_sample) -------------------------------------
// One chunk of the B*S images of a sampling call: images g0 .. g0 + n - 1 of the flat [B][S] order
// (condition g / S, draw g % S), whose zy / xy_hat live in the chunk buffers at image g - g0.
struct SampleChunk {
    long long g0;        // first image of the chunk in [B][S] order
    int n, S;            // images in the chunk, draws per condition
    int HW, D, x_d;      // io shape
};
// k_latent: zy[i] = concat(temperature * N(0,1), y[(g0 + i) / S]) for the chunk's images; the normal
// of image g, pixel p, channel c is stream element offset + (g * HW + p) * x_d + c (instance_noise_value)
void launch_latent(const SampleChunk& c, const float* y, float* zy, float temperature, unsigned long long seed,
                   unsigned long long offset, hipStream_t st);
// Where a chunk's draws live and where a draw's condition comes from: the one view every kernel after a
// chunk's inverse reads. The rule, stated here once: with y non-null the condition of image i of the chunk is
// y[b], b = (g0 + i) / S (cnf_flow_sample); with y null it is the y channels of the image's own zy[i], which
// the inverse leaves intact (cnf_flow_sample_cascade: at stage >= 2 a node's condition is `up` of its parent's
// value, not y[b]). The kernels that read a condition are templates on that source (NODE: the image's own zy;
// recorded with the suffix _node); same arithmetic, same bits. A draw's sample value is
// sample_post_value(x_hat, logit, lk, residual, condition) (cnf_device.h), the one arithmetic expression.
struct DrawView {
    const float* xy_hat;  // the chunk's inverse output [n][HW][D]: x_hat on the channels < x_d
    const float* zy;      // the chunk's latent [n][HW][D]: z on the channels < x_d, the condition on the rest
    const float* y;       // the per-condition table [B][HW][D - x_d], or null: the image's own zy
    int logit, residual;  // the post-transforms: de_logitify, + condition (needs D - x_d == x_d)
    LogitK lk;
    bool node() const { return y == nullptr; }
};
// k_sample_fold: one pass over the chunk's xy_hat. Per element (b, p, c < x_d) of the conditions the
// chunk touches, over the chunk's draws of b in draw order: v = the draw's sample value; stored to samples
// [B][S][HW][x_d] (non-null); folded into state [3][B][HW][x_d] = (K, S1, S2)
// (sample_fold; loaded unless the chunk holds b's first draw), and with b's last draw mean / std
// [B][HW][x_d] (each may be null) are written. state == null: no statistics.
struct SampleFoldArgs {
    DrawView v;
    float* samples;
    float* state;
    float* mean;
    float* std;
    int B;
};
void launch_sample_fold(const SampleChunk& c, const SampleFoldArgs& a, hipStream_t st);
// k_sample_ydev: y_dev[g0 + i] = sum_{p, c >= x_d} |xy_hat[i, p, c] - condition[p, c - x_d]|, one
// wave per image, fp64 lane sums in element order then a fixed-order wave sum
void launch_sample_ydev(const SampleChunk& c, const DrawView& v, float* y_dev, hipStream_t st);
// k_sample_logp: log_prob[g0 + i] = (float)(-0.5 q - 0.5 n log(2 pi) + L), n = HW * x_d, q the fp64 sum of
// z^2 over image i's latent (channels < x_d of the chunk's zy), L the fp64 sum of image i's log-det slots
// ld_part[nl][c.n][np] as the chunk's inverse wrote them (k_ld_reduce's order); one wave per image
void launch_sample_logp(const SampleChunk& c, const float* zy, const double* ld_part, int nl, int np, float* log_prob,
                        hipStream_t st);
// Scoring the draws against a truth (cnf_flow_sample_score). v below is k_sample_fold's sample value.
// The outputs are the state between chunks: a chunk that holds b's first
// draw initialises b's entries, every other chunk loads them, so nothing is read that this call did not write.
// k_sample_score: k_sample_fold's ownership (a workgroup owns a tile of elements of one condition b over the
// chunk's draws of b). rank[b,p,c] += #{v < truth} (null: none); abs_err[b,p,c]: the fp32 running sum of
// |v - truth| in draw order, divided by S with b's last draw (null: none); hist[b,p,c,k] += the draws with
// k == (int)floorf((v - lo) * scale), 0 <= k < bins (null: none; out of range and NaN dropped).
struct SampleScoreArgs {
    DrawView v;
    const float* truth;   // [B][HW][x_d]; needed by rank and abs_err
    int* rank;
    float* abs_err;
    int* hist;            // [B][HW][x_d][bins]
    int bins;
    float lo, scale;     // scale = (float)bins / (hi - lo)
};
constexpr int SCORE_MAX_BINS = 256, SCORE_MAX_QUANTILES = 8;
void launch_sample_score(const SampleChunk& c, const SampleScoreArgs& a, hipStream_t st);
// k_sample_sqerr: sq_err[g0 + i] = (float) sum_{p, c < x_d} ((double)v - (double)truth[(g0 + i) / S, p, c])^2,
// one wave per image, fp64 lane sums in element order then the fixed-order wave sum
struct SampleSqerrArgs {
    DrawView v;
    const float* truth;
    float* sq_err;        // [B][S]
};
void launch_sample_sqerr(const SampleChunk& c, const SampleSqerrArgs& a, hipStream_t st);
// k_sample_quantiles, once after the last chunk, one thread per element: quantiles[j][b][p][c] of level q[j] from
// hist by linear interpolation inside the bin where the cumulative count reaches q[j] * N; NaN where N == 0
struct SampleQuantileArgs {
    const int* hist;
    float* quantiles;     // [nq][n]
    long long n;          // B * HW * x_d
    int bins, nq;
    float lo, hi;
    float q[SCORE_MAX_QUANTILES];
};
void launch_sample_quantiles(const SampleQuantileArgs& a, hipStream_t st);

// ---- cascaded sampling (cnf_sample.hip, cnf_flow_sample_cascade) --------------------------------
// k_child_latent: one chunk c of a child stage's zy from the parent stage's chunk buffers. Child node g has
// parent g / Sc, image g / Sc - pg0 of the parent chunk. Per child pixel (h, w): the x channels get
// temperature * N(0,1) by k_latent's rule; y channel cy gets the parent's sample value (its view, its own
// condition) at pixel (h / 2, w / 2), channel cy -- the post-transform,
// cnf_up and k_latent in one pass, the parent's image never written at full size. D == 2 x_d.
struct ChildLatentArgs {
    DrawView parent;      // the parent chunk's buffers [pn][HW / 4][D]; y null
    float* zy;            // the child chunk's zy [n][HW][D]
    long long pg0;        // first node of the parent chunk
    int Sc, W;            // children per parent; the child's width
    float temperature;
    unsigned long long seed, offset;
};
void launch_child_latent(const SampleChunk& c, const ChildLatentArgs& a, hipStream_t st);
// k_block_dev: block_dev[g0 + i] = (float) sum over the 2x2 pixel blocks and channels c < x_d of
// |0.25 * sum over the block's 4 pixels in row-major order of ((double)v - (double)y)|, v the image's sample value,
// y its condition (the y channels of zy[i], whatever the view's source: k_latent copied y[b] there; D == 2 x_d,
// H and W even). One wave per image, fp64 lane sums over
// (block, c) in element order, then the fixed-order wave sum.
struct BlockDevArgs {
    DrawView v;
    float* block_dev;     // [B][S]
    int W;
};
void launch_block_dev(const SampleChunk& c, const BlockDevArgs& a, hipStream_t st);

// ---- density of given images (cnf_logprob.hip, cnf_flow_log_prob) ---------------------------------
// One chunk of the N pairs of a log_prob call: pairs g0 .. g0 + n - 1, pair g = (image, condition) =
// (g / K, g % K) pairwise (K >= 1), (g, g) paired (K == 0); its xy / zy live in the chunk buffers at g - g0.
struct LogpChunk {
    long long g0;        // first pair of the chunk
    int n, K;            // pairs in the chunk; conditions (0: paired)
    int HW, D, x_d;      // io shape
};
// The one reduction rule of these kernels: a thread folds its elements in fp64 in element order (which
// elements it owns depends on the image shape alone), the wave sums by the fixed xor butterfly (wave_sum),
// the waves of a workgroup are added in wave order and a pair's partial slots in slot order. A pair's value
// therefore does not depend on chunk, B, K or the pair's place in its chunk.
// k_logp_gather's tile: LOGP_QUADS quads of 4 consecutive pixels per workgroup, one per thread; an image of
// HW pixels has logp_parts(HW) tiles and as many log_jac partial slots
constexpr int LOGP_QUADS = 256;
inline int logp_parts(int HW) { return (HW + 4 * LOGP_QUADS - 1) / (4 * LOGP_QUADS); }
// the gather's grid for a chunk of n pairs: n * parts work items dealt over the 8 XCDs, per_xcd each (rounded up)
inline int logp_per_xcd(int n, int parts) { return (n * parts + 7) / 8; }
// Which gather runs (launch_logp_gather launches what this returns, cnf_debug_logp_choice reports it): the
// float4 template of the presets' (x_d, D - x_d) = (1, 1), (3, 1), (3, 3) when HW % 4 == 0 and x, y and xy are
// 16-byte aligned, k_logp_gather_any for every other depth or alignment
enum LogpGatherKernel { LOGP_GATHER_ANY = 0, LOGP_GATHER_1_1 = 1, LOGP_GATHER_3_1 = 2, LOGP_GATHER_3_3 = 3 };
inline LogpGatherKernel logp_gather_choice(int x_d, int yd, int HW, bool aligned) {
    if (HW % 4 != 0 || !aligned) return LOGP_GATHER_ANY;
    if (x_d == 1 && yd == 1) return LOGP_GATHER_1_1;
    if (x_d == 3 && yd == 1) return LOGP_GATHER_3_1;
    if (x_d == 3 && yd == 3) return LOGP_GATHER_3_3;
    return LOGP_GATHER_ANY;
}
// k_logp_finish's element loop: a workgroup takes LOGP_FINISH_STEP floats of the image's HW * D per trip (one
// float4 per thread); the threads of the last trip that still hold a float4 (256: the last trip is full)
constexpr int LOGP_FINISH_STEP = 4 * 256;
inline int logp_finish_trips(int HW, int D) { return (HW * D + LOGP_FINISH_STEP - 1) / LOGP_FINISH_STEP; }
inline int logp_finish_last_trip(int HW, int D) {
    return (HW * D - (logp_finish_trips(HW, D) - 1) * LOGP_FINISH_STEP + 3) / 4;
}
// k_logp_gather: xy[i] = concat(v, y[cond]) for the chunk's pairs, v = logit_value(x[img] - y[cond]) (the
// subtraction with residual, the map with logit: sample_post_value's inverse), and the pair's log_jac
// partials lj[i][part] = sum over the tile's x elements of -log(e (1 - e)), e = a + c1 x' in fp32 as the map
// sees it (0 without logit). An element with e outside (0, 1) (NaN included) adds -inf and enters xy as 0, so
// the flow runs on finite values.
struct LogpGatherArgs {
    const float* x;      // [B][HW][x_d]
    const float* y;      // [K or B][HW][D - x_d]
    float* xy;           // [n][HW][D]
    double* lj;          // [n][logp_parts(HW)]
    int logit, residual;
    LogitK lk;
};
void launch_logp_gather(const LogpChunk& c, const LogpGatherArgs& a, hipStream_t st);
// k_logp_finish: per pair of the chunk, one workgroup and one pass over zy[i]: q = sum z^2 over the x
// channels, dev = sum |y_hat - y[cond]| over the others; llz = -0.5 q - 0.5 HW x_d log(2 pi), J = the pair's
// lj slots in order + lj_const (HW x_d (log c1 - log span) with logit, else 0), log_prob =
// (float)(llz + ld[i] + J). J == -inf (an element outside the map's domain): log_prob = -inf, log_jac = -inf,
// llz, logdet and y_dev NaN. Outputs indexed by the pair g0 + i, each may be null. No counter, no atomics.
struct LogpFinishArgs {
    const float* zy;     // [n][HW][D]
    const float* y;
    const float* ld;     // [n] the forward's per-image log-det
    const double* lj;    // [n][parts]
    double lj_const;
    float *log_prob, *llz, *logdet, *log_jac, *y_dev;
};
void launch_logp_finish(const LogpChunk& c, const LogpFinishArgs& a, hipStream_t st);
// k_logp_posterior: per row b of log_prob [B][K], a_k = log_prob[b][k] + log_prior[k] (null: + 0) in fp64,
// m = max_k a_k, lse = m + log(sum_k exp(a_k - m)); posterior[b][k] = (float)exp(a_k - lse), log_evidence[b]
// = (float)lse (each may be null). A row of -inf only: posterior NaN, log_evidence -inf. One wave per row
// for K <= 64, else one workgroup.
void launch_logp_posterior(const float* log_prob, const float* log_prior, float* posterior, float* log_evidence,
                           int B, int K, hipStream_t st);

// ---- input gradients of the log-density (cnf_score.hip, cnf_flow_score / cnf_flow_ascend) -----------
// The kernels around the data-gradient-only backward, on one chunk of paired images (LogpChunk with K == 0).
// The reduction rule is the one stated above; none of them has an atomic or a counter.
// k_score_seed: one workgroup per image and one pass over zy[i] (k_logp_finish's ownership of the elements):
// dzy[i] = the seed of d(llz + logdet)/dzy, -z on the x channels and 0 on the others (null: not written), and
// llz[i] = -0.5 sum z^2 - 0.5 HW x_d log(2 pi) in fp64. trace (may be null): trace[g0 + i] = (float)(llz[i] +
// ld[i]), -inf for an image whose lj slots (null: none) sum to -inf: the flow-input-space log-density.
struct ScoreSeedArgs {
    const float* zy;     // [n][HW][D]
    float* dzy;          // [n][HW][D] or null
    double* llz;         // [n]
    const float* ld;     // [n] the forward's per-image log-det (read only with trace)
    const double* lj;    // [n][logp_parts(HW)] or null
    float* trace;        // [B] or null
};
void launch_score_seed(const LogpChunk& c, const ScoreSeedArgs& a, hipStream_t st);
// k_score_finish: the gradient g = d(llz + logdet)/dxy of the chunk ([n][HW][D], the backward's) through the
// gather's map, per element of image g0 + i: with v = x - y (residual) or x, e = a + c1 v and u = logit_value(v),
// t = g_x du/dv + d log_jac/dv = g_x c1 / (span e (1 - e)) - c1 (1 - 2 e) / (e (1 - e)) (without logit: t = g_x);
// grad_x = t, grad_y = g_y (- t on channel c with residual). log_prob[g0 + i] = (float)(llz + ld + J) with
// k_logp_finish's J. An image with J == -inf: log_prob -inf, its gradients NaN. Any output may be null. One
// float4 of g per thread, grid (trips, n).
struct ScoreFinishArgs {
    const float* g;      // [n][HW][D] or null (no gradient asked for)
    const float* x;      // [B][HW][x_d]
    const float* y;      // [B][HW][D - x_d]
    const double* llz;   // [n]
    const float* ld;     // [n]
    const double* lj;    // [n][parts]
    double lj_const;
    float *grad_x, *grad_y, *log_prob;
    int logit, residual;
    LogitK lk;
};
void launch_score_finish(const LogpChunk& c, const ScoreFinishArgs& a, hipStream_t st);
// k_ascend_step: Keras Adam (k_adam's arithmetic) on the x channels of the chunk's xy with the gradient -g, so the
// step climbs: gi = -g; m += (gi - m)(1 - b1); v += (gi^2 - v)(1 - b2); xy -= alpha m / (sqrt(v) + eps), in
// place. m, v: [n][HW][x_d] (the chunk's part of the state). The y channels are not read or written.
struct AscendStepArgs {
    float* xy;           // [n][HW][D]
    const float* g;      // [n][HW][D]
    float *m, *v;
    float alpha, b1, b2, eps;
};
void launch_ascend_step(const LogpChunk& c, const AscendStepArgs& a, hipStream_t st);
// k_ascend_out: x_out[g0 + i] = sample_post_value(xy[i] x channels, condition y[g0 + i]) (de_logitify, + y), or
// x0[g0 + i] for an image whose lj slots sum to -inf
struct AscendOutArgs {
    const float* xy;     // [n][HW][D]
    const float* x0;     // [B][HW][x_d]
    const float* y;      // [B][HW][D - x_d]
    const double* lj;    // [n][parts]
    float* x_out;        // [B][HW][x_d]
    int logit, residual;
    LogitK lk;
};
void launch_ascend_out(const LogpChunk& c, const AscendOutArgs& a, hipStream_t st);

// ---- training (cnf_train.hip) -------------------------------------------------------------------
// Generic fp32 convolution for the training path over the dense backward image (taps x k x n):
//   out[b,p,n] (=|+=) bias[n] + res[b,p,n] + sum_{tap,k} X[b, p + sgn*dil*off(tap), k] * W(tap,k,n)
// with W(tap,k,n) = w[tap*wt + k*wk + n*wn] and X = LN(LeakyReLU(in)) on load when stats != null
// (LeakyReLU only when act && !stats). sgn = +1 is the forward conv; sgn = -1 with transposed
// strides is the data gradient (dX = conv^T dY). Zero padding outside the image.
struct TConvArgs {
    const float* in;
    int in_cs, in_off, K;
    const float* stats;       // [B][2] (mean, rstd) of LeakyReLU(in) over the whole tensor, or null
    const float* gamma;       // per element [npx][in_cs] (channel in_off + k)
    const float* beta;
    int act;
    const float* w;
    long long wt;
    int wk, wn;
    const float* bias;        // [N] or null
    const float* res;         // [B][npx][out_cs] window or null
    float* out;
    int out_cs, out_off, N, accumulate;
    int H, W, taps, dil, sgn, B;
    const float* zero;        // >= 16 bytes of zeros, 16-byte aligned: what out-of-image loads read
    // LN-backward reduction of the output (lnr_part non-null): the output v is dL/d(LN output) of the
    // LayerNorm(LeakyReLU) whose raw input lnr_x has the output's layout; each workgroup adds sum v * gamma
    // and sum v * gamma * xhat over its elements and writes them to lnr_part[b][tile][2] (fixed order)
    const float* lnr_x;
    const float* lnr_gamma;
    const float* lnr_stats;
    double* lnr_part;
    int lnr_base, lnr_stride;   // the launch's partials at [b][lnr_base + tile] of a [B][lnr_stride] array
};
// returns the LN-reduction partials per image the launch wrote (0: none — the kernel has no fused
// reduction, the caller runs k_lnb_reduce)
int launch_tconv(const TConvArgs& a, hipStream_t st);
constexpr int LNR_MAXPARTS = 64;   // per image, k_tconv_* fused LN reductions
// the kernel launch_tconv runs for a convolution and its tiling (launch_tconv launches what this returns;
// cnf_debug_tconv_choice reports it). kernel TCONV_THIN: th = TR rows per workgroup; TCONV_BAND:
// k_tconv_band<nr, sub> on bands of th rows; TCONV_MFMA: k_tconv_mfma<nr, vec>; TCONV_VALU: k_tconv<tn>
enum TConvKernel { TCONV_VALU = 0, TCONV_THIN = 1, TCONV_BAND = 2, TCONV_MFMA = 3 };
struct TConvChoice {
    int kernel, nr, sub, th, all_taps, vec, tn;
    size_t lds;
};
TConvChoice tconv_choice(const TConvArgs& a);

// weight gradient: part[chunk][(tap*CI + ci)*CO + co] = sum over the chunk's pixels of
// X[b, p + dil*off(tap), ci] * dY[b, p, co] (X with LN-on-load as in TConvArgs); bpart[chunk][co]
// = sum dY (bias gradient) when non-null
struct WGradArgs {
    const float* x;
    int x_cs, x_off, CI;
    const float* stats;
    const float* gamma;
    const float* beta;
    int act;
    const float* dy;
    int dy_cs, dy_off, CO;
    float* part;
    float* bpart;
    int H, W, taps, dil, B, chunks, chunk_px;
    const float* zero;   // k_wgrad_direct: >= 1 float of zeros (what lanes outside the image read)
};
void launch_wgrad(const WGradArgs& a, hipStream_t st);
// k_wgrad_band (the MFMA weight gradient): partial rows per launch (<= WGRAD_MAX_CHUNKS), each
// [taps][CI][CO] weights then [CO] bias, and its LDS bytes
constexpr int WGRAD_MAX_CHUNKS = 256;
int wgrad_band_chunks(int B, int H, int W, int taps, int CI, int CO);
size_t wgrad_band_lds(int H, int W, int taps, int dil, int CI, int CO);
bool train_valu_kernels();   // CNF_TRAIN_VALU=1: the register-blocked VALU convolutions (A/B)
// k_wgrad_band handles this conv (taps 1 / 9, width >= 4, staged band within 160 KiB); otherwise the
// weight gradient runs on the VALU k_wgrad (WGradArgs::chunk_px > 0) with a separate bias scatter
bool wgrad_band_ok(int H, int W, int taps, int dil, int CI, int CO);
// k_wgrad_direct (register-operand MFMA weight gradient, WGradArgs::chunk_px == -1): width % 4 == 0,
// taps 1 / 9; its partial-row count (<= WGRAD_MAX_CHUNKS) for a batch of B images of H rows
bool wgrad_direct_ok(int H, int W, int taps);
int wgrad_direct_chunks(int B, int H);
// k_wgrad_thin (3x3, dilation 1, CO <= 4, CI <= 64, CI % 4 == 0: the streamed conv_out's weight
// gradient): one partial row [taps][CI][CO] + [CO] per workgroup, wgrad_thin_chunks of them
bool wgrad_thin_ok(int H, int W, int taps, int dil, int CI, int CO);
int wgrad_thin_chunks(int B, int H, int W);
void launch_wgrad_thin(const WGradArgs& a, hipStream_t st);
// How a weight-gradient launch partitions the batch, from the shape functions the launchers call (read
// by cnf_debug_wgrad_choice). chunks: partial rows written. k_wgrad_direct: units = row bands per image,
// per_chunk = RB rows per band, short_last = the image's last band has fewer than RB rows. k_wgrad_thin:
// units = row tiles per image, per_chunk = ipw images per workgroup, short_last = the last image group
// has fewer than ipw images. k_wgrad_band: units = (image, band of per_chunk = RB rows) work units, which
// the `chunks` grid columns loop over once units > chunks; short_last as for k_wgrad_direct.
struct WGradSplit {
    int chunks, units, per_chunk, short_last;
};
WGradSplit wgrad_direct_split(int B, int H);
WGradSplit wgrad_thin_split(int B, int H, int W);
WGradSplit wgrad_band_split(int B, int H, int W, int taps, int CI, int CO);
// dparams[map[i]] += sum_c part[c][i] for i < n (map[i] >= 0)
void launch_grad_scatter(const float* part, int chunks, long long n, const int64_t* map, float* dparams, hipStream_t st);
int grad_scatter_trips(int chunks);   // passes of k_grad_scatter's chunk loop (one up to 256 chunks)
void launch_ln_stats(const float* x, long long n, int B, int act, float* stats, hipStream_t st);
// LN + LeakyReLU backward: dx (=|+=) d/dx of LN(LeakyReLU(x)) given dxo = dL/d(LN output);
// dgamma/dbeta (+=) per element; stats == null: LeakyReLU backward only
// (the batch runs in LNB_SLICES slices: scratch holds their [2][LNB_SLICES][n] gamma / beta partials)
constexpr int LNB_SLICES = 8;
// k_lnb_reduce splits each image over up to LNB_RS workgroups (partial sums [B][rs][2], summed in slice
// order where they are read)
constexpr int LNB_RS = 8;
// presum > 0: sums already holds presum partials per image at [b][k] of a [B][pstride][2] array (k_tconv_*
// fused LN reductions), no k_lnb_reduce. cmod > 0: dxo holds only the channels whose bit is set in
// cmask (channel = element index % cmod, cmod <= 64); the others are read as 0 whatever dxo holds
void launch_ln_backward(const float* x, const float* dxo, const float* gamma, const float* stats, double* sums,
                        long long n, int B, int act, float* dx, int accumulate, float* dgamma, float* dbeta,
                        float* scratch, hipStream_t st, int presum = 0, int pstride = 0,
                        unsigned long long cmask = 0, int cmod = 0);
// launch_ln_backward's partition of a B-image batch of n-element images: rsl reduction partials per image
// at stride rstride, S batch slices (k_lnb_apply's grid.y) of bs images (the last ones short or empty),
// shared = a full slice's per-image sums go through LDS (bs <= 256) rather than per thread
struct LnbSlicing {
    int rsl, rstride, S, bs, shared;
};
LnbSlicing lnb_slicing(long long n, int B, int presum = 0, int pstride = 0);
// Fused training backward of a k_net_lds layer (cnf_ldsbwd.hip): grid (B, 2 nets), one workgroup per
// (image, net). Offsets table per net (int32, `offs_per_net` entries): canonical parameter offsets
// (LN gamma / beta, the net's first parameter, tanh scale or -1) and dense backward-image offsets
// (conv weights _DW, biases _DB), laid out as the LDSBWD_* indices below (per residual block r at
// LDSBWD_RB0 + r * (LDSBWD_PER_RB0 + 2 * nbr), branch bi's (dw, db) at LDSBWD_BR + 2 bi of it).
enum {
    LDSBWD_LO = 0, LDSBWD_CI_DW, LDSBWD_CI_DB, LDSBWD_LNO_G, LDSBWD_LNO_B, LDSBWD_CO_DW, LDSBWD_CO_DB, LDSBWD_TANH,
    LDSBWD_CI_K, LDSBWD_CI_B, LDSBWD_CO_K, LDSBWD_CO_B,   // canonical kernel / bias offsets of the plain convs
    LDSBWD_RB0
};
enum {
    LDSBWD_LN1G = 0, LDSBWD_LN1B, LDSBWD_CA_DW, LDSBWD_CA_DB, LDSBWD_LN2G, LDSBWD_LN2B, LDSBWD_LN3G, LDSBWD_LN3B,
    LDSBWD_CB_DW, LDSBWD_CB_DB, LDSBWD_CA_K, LDSBWD_CA_B, LDSBWD_CB_K, LDSBWD_CB_B, LDSBWD_BR
};
constexpr int LDSBWD_PER_RB0 = LDSBWD_BR;   // entries per residual block before its branches' (dw, db) pairs
struct LdsBwdArgs {
    const float* save;        // the training forward's save area of the layer [net][B][save_img] (LdsSave)
    int save_img, save_t1, save_t2, save_st;
    const float* dso[2];      // dL/d(raw conv_out) per net [B][hc][wc][dc2] (k_coup_bw)
    const float* u;           // the layer input [B][H][W][D] (conv_in reads its mask-compressed half)
    float* du1c[2];           // out: dL/du1c per net [B][hc][wc][dc1]
    const float* params;      // canonical parameters (LN gamma / beta)
    const float* bw;          // dense backward weight image (launch_pack)
    const int64_t* bw_map;    // dense -> canonical parameter index
    const int* offs;          // [2][offs_per_net]
    int offs_per_net;
    float* part;              // out: per (net, image) gradient rows [2][B][row], the net's canonical range
    int row;
    int H, W, D, mask, hc, wc, dc1, dc2, nk, gc, R, nbr, ln, taps;
    int br_cin_off[NETLDS_MAXBR], br_cin[NETLDS_MAXBR], br_cout[NETLDS_MAXBR], br_out_off[NETLDS_MAXBR],
        br_dil[NETLDS_MAXBR];
    int sy, st, sa, ac_chunk;                                   // LDS pixel strides (floats); conv_b staging chunk
    int wmax;                                                   // floats of the W region (weight-gradient scratch too)
    int stamps;                                                 // diagnostics: phase clock stamps (CNF_LDSBWD_STAMPS)
    int off_gt, off_ac, off_w, off_kt, off_red, off_ot, off_z, lds_bytes;   // LDS byte offsets (GY at 0)
    // split mode (CNF_LDS_SPLIT): 0 the whole backward; 1 the data-gradient chain only, storing the
    // gradients the weight gradients contract with to gsave; 2 the weight gradients only, from gsave
    int mode;
    float* gsave;                       // [2][B][gsave_img] per (net, image)
    int gsave_img, gs_rb, g_t3, g_t2, g_in;   // per residual block r: dL/dy_{r+1} at r * gs_rb, dL/dt2 at
                                             // + g_t3, dL/dt1 at + g_t2; dL/dy_0 (conv_in's) at g_in
};
void launch_lds_bwd(const LdsBwdArgs& a, int B, hipStream_t st);
int read_bwd_stamps(long long* host, int n);   // [0] = count, [1..] = s_memtime per phase boundary
// dparams[lo_n + i] += sum_b part[n][b][i] (i < len_n, n = 0, 1; row floats per (net, image) row)
void launch_grad_rows(const float* part, int B, int row, int64_t lo0, int64_t lo1, int len0, int len1, float* dparams,
                      hipStream_t st);
int grad_rows_trips(int B);   // passes of k_grad_rows' image loop (one up to B = 64)

// The weight-gradient kernel of a convolution on h x w images in a batch of B (cnf_train.cpp; wgrad_launch
// launches what this returns, cnf_debug_wgrad_choice reports it). x_cs: floats per pixel of the tensor the
// input window lies in; bias_follows: the dense image keeps the bias right after the weights.
// WGRAD_VALU: k_wgrad, `chunks` runs of chunk_px pixels of the flattened (image, pixel) axis.
enum WGradKernel { WGRAD_VALU = 0, WGRAD_THIN = 1, WGRAD_DIRECT = 2, WGRAD_BAND = 3 };
struct WGradChoice {
    int kernel, chunks, chunk_px;
};
WGradChoice wgrad_choice(int B, int h, int w, int taps, int dil, int cin, int cout, int x_cs, bool bias_follows);

struct CoupBwArgs {
    const float* u;           // layer input [B][H][W][D]
    const float* dv;          // dL/dv
    const float* s_pre;       // raw conv_out of net A
    const float* tanh_w;
    float* du;                // dL/du (u1 positions: dL/dv1 only; the nets' share is added later)
    float* ds_pre;            // dL/d s_pre  [B][hc][wc][dc2]
    float* dt;                // dL/dt
    double* dw_part;          // [B][gridDim.x]
    float g_ld;               // dL/d(per-image log-det)
    const float* count;       // non-null: g_ld = -1 / *count (the global image count, on device)
    int H, W, D, mask, mask_c, hc, wc, dc1, dc2;
};
void launch_coupling_backward(const CoupBwArgs& a, int B, int nparts, hipStream_t st);
void launch_scatter_add_u1c(const float* du1c, float* du, int B, int H, int W, int D, int mask, int hc, int wc, int dc1,
                            hipStream_t st);
void launch_dsum(const double* part, long long n, float* out, hipStream_t st);
// dL/dzy of the NLL (conv_cINN_make_model.py:1800-1848): z / Bg, lambda_y * sign(y - y') / Bg
// count (device, may be null): the global image count; when given, inv_batch = 1 / *count (computed in
// fp64 and rounded once, as the host does), so the scale needs no host read of the all-reduced count
void launch_nll_grad(const float* xy, const float* zy, float* dzy, int B, int HW, int D, int x_d, float lambda_y,
                     float inv_batch, const float* count, hipStream_t st);
void launch_adam(float* params, const float* grads, float* m, float* v, long long n, float alpha, float b1, float b2,
                 float eps, hipStream_t st);

// Clipped, guarded Adam (cnf_optim.hip; the rules: include/cnf.h at cnf_optim_step). One slab of the table:
// elements [start, start + count) of tensor `tensor`, count <= OPTIM_SLAB, never across a tensor boundary.
constexpr int OPTIM_SLAB = 4096;
struct OptimSlab {
    long long start;
    int count, tensor;
};
// The step's workspace: per-slab sums and counts, the tensors' scales, then the control record.
struct OptimCtrl {
    float alpha;   // the step size of this step
    int skip;      // non-zero: k_optim_step writes nothing
};
struct OptimWs {
    double* sum_g;       // [num_slabs] sum of g^2
    double* sum_h;       // [num_slabs] sum of h^2 (h = clamped g)
    unsigned* nonfinite; // [num_slabs] elements of g that are NaN or +-inf
    float* scale;        // [T] s_t after k_optim_finish's first pass, scale_t = fl32(s_t * S) after its second
    OptimCtrl* ctrl;
    size_t total;        // bytes
};
OptimWs optim_ws(void* base, int T, long long num_slabs);
struct OptimArgs {
    float* p;
    const float* g;
    float* m;
    float* v;
    float* ema;               // null without EMA
    const OptimSlab* slabs;   // [num_slabs], device
    const int* first;         // [T + 1], device: tensor t's slabs are first[t] .. first[t + 1] - 1
    long long num_slabs;
    int T;
    bool vec;                 // p, g, m, v, ema are all 16-byte aligned (else every access is scalar)
    cnf_optim_desc d;
    long long* state;         // [0] applied, [1] skipped
    float* stats;             // [CNF_OPTIM_STATS_FLOATS] or null
    float* scales_out;        // [T] or null
    OptimWs ws;
};
void launch_optim(const OptimArgs& a, hipStream_t st);   // k_optim_stats, k_optim_finish, k_optim_step
}  // namespace cnf
