// cnf_train.cpp — backward pass of the NLL training step (cFlow.train_step,
// conv_cINN_make_model.py:1850-1880: tf.GradientTape over log_loss :1800-1848).
//
// Gradient of loss = -(mean_b(llz_b + lly_b) + mean_b(logdet_b)) with respect to the canonical
// parameter vector. The training forward (cnf_flow_forward_train) saves every coupling layer's input
// and, by default, its activations; the backward walks the layer schedule in reverse:
//   - layout layers (squeeze / factor-out / final restoration) are permutations: their gradient is
//     the inverse map applied to dL/dv (the same index tables as cnf_flow_inverse);
//   - a k_net_lds layer runs the fused backward (k_lds_bwd, cnf_ldsbwd.hip) from its saved LdsSave
//     blocks: coupling_backward_lds;
//   - a streamed layer (and every layer under LDS_BWD=0) runs StreamedBwd: the coupling-law backward,
//     then each s,t network in reverse from the activations the forward saved (StreamActs) — recomputed
//     first when they were not (over the save budget, TRAIN_SCHED bit SCHED_RECOMPUTE, the lone-layer
//     API). Per conv: the weight gradient (launch_wgrad* + a scatter through the dense map onto the
//     canonical parameters, so the grouped-conv closure quirk and group boundaries come out exactly),
//     the data gradient (launch_tconv with transposed weights), and the LayerNorm backward with the
//     per-element gamma / beta gradients.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "cnf_api.h"
#include "cnf_kernels.h"
#include "cnf_plan.h"

namespace cnf {

namespace {

void hchk(hipError_t e, const char* what) {
    if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}

int wgrad_chunks(int B, int npx) {
    const long long total = (long long)B * npx;
    return (int)std::max<long long>(1, std::min<long long>(64, (total + 511) / 512));
}

}  // namespace

WGradChoice wgrad_choice(int B, int h, int w, int taps, int dil, int cin, int cout, int x_cs, bool bias_follows) {
    if (train_valu_kernels() || !wgrad_band_ok(h, w, taps, dil, cin, cout)) {
        const int chunks = wgrad_chunks(B, h * w);
        const long long total = (long long)B * h * w;
        return {WGRAD_VALU, chunks, (int)(((total + chunks - 1) / chunks + 15) / 16 * 16)};
    }
    if ((long long)h * w * x_cs * 4 < (1LL << 31) && wgrad_thin_ok(h, w, taps, dil, cin, cout) && bias_follows)
        return {WGRAD_THIN, wgrad_thin_chunks(B, h, w), 0};
    if ((opts().train_alt & ALT_WGRAD_BAND) == 0 && wgrad_direct_ok(h, w, taps))
        return {WGRAD_DIRECT, wgrad_direct_chunks(B, h), -1};
    return {WGRAD_BAND, wgrad_band_chunks(B, h, w, taps, cin, cout), 0};
}

void ldsbwd_geom(const Coupling& c, LdsBwdArgs& a) {
    const int HW = c.hc * c.wc;
    a.row = (int)std::max(c.net[0].hi - c.net[0].lo, c.net[1].hi - c.net[1].lo);
    a.gs_rb = HW * (2 * c.nk + c.gc);
    a.g_t3 = HW * c.nk;
    a.g_t2 = HW * (c.nk + c.gc);
    a.g_in = c.R * a.gs_rb;
    a.gsave_img = (a.g_in + HW * c.nk + 3) / 4 * 4;
}

// LDS pixel stride for C channels: a multiple of 4 floats (16-byte quads), odd in quads
static int bwd_stride(int C) {
    int s = (C + 3) / 4 * 4;
    if (s % 8 == 0) s += 4;
    return s;
}

size_t ldsbwd_setup(const Plan& p, const Coupling& c, LdsBwdArgs& a) {
    std::memset(&a, 0, sizeof(a));
    if (!c.use_lds || (int)c.br.size() > NETLDS_MAXBR || c.bwd_offs_per_net == 0) return 0;
    const int ks = p.desc.ksize, taps = ks * ks;
    if (taps != 1 && taps != 9) return 0;
    for (const Branch& b : c.br)
        if (b.dil > 32) return 0;
    a.H = c.H;
    a.W = c.W;
    a.D = c.D;
    a.mask = c.mask;
    a.hc = c.hc;
    a.wc = c.wc;
    a.dc1 = c.dc1;
    a.dc2 = c.dc2;
    a.nk = c.nk;
    a.gc = c.gc;
    a.R = c.R;
    a.nbr = (int)c.br.size();
    a.ln = p.desc.layer_norm;
    a.taps = taps;
    for (int i = 0; i < a.nbr; i++) {
        a.br_cin_off[i] = c.br[i].cin_off;
        a.br_cin[i] = c.br[i].cin;
        a.br_cout[i] = c.br[i].cout;
        a.br_out_off[i] = c.br[i].out_off;
        a.br_dil[i] = c.br[i].dil;
    }
    const int HW = c.hc * c.wc;
    const int ac = std::max(std::max(c.nk, c.dc1), 4);
    a.sy = bwd_stride(c.nk);
    a.st = bwd_stride(std::max(std::max(c.gc, c.nk), std::max(c.dc2, c.dc1)));
    a.sa = bwd_stride(ac);
    a.ac_chunk = std::min(c.gc, ac / 4 * 4);
    auto kp4 = [](int K) { return (K + 3) / 4 * 4; };
    auto np16 = [](int N) { return (N + 15) / 16 * 16; };
    // transposed-weight images of the data gradients (rows: taps x the output channels rounded up to 4,
    // stage_wt), the k-table lengths of the weight gradients, the zero row of gemm_tap (the widest A)
    size_t wmax = (size_t)taps * kp4(c.dc2) * np16(c.nk);
    wmax = std::max(wmax, (size_t)kp4(c.nk) * np16(c.gc));
    wmax = std::max(wmax, (size_t)kp4(c.nk) * np16(c.nk));
    wmax = std::max(wmax, (size_t)taps * kp4(c.nk) * np16(c.dc1));
    int ktmax = std::max(kp4(taps * c.nk), kp4(taps * c.dc1));
    ktmax = std::max(ktmax, std::max(kp4(c.nk), kp4(a.ac_chunk)));
    int zn = std::max(kp4(c.dc2), kp4(c.nk));
    for (const Branch& b : c.br) {
        wmax = std::max(wmax, (size_t)taps * kp4(b.cout) * np16(b.cin));
        ktmax = std::max(ktmax, kp4(taps * b.cin));
        zn = std::max(zn, kp4(b.cout));
    }
    auto al = [](size_t v) { return (v + 15) / 16 * 16; };
    size_t off = al((size_t)HW * a.sy * 4);
    a.off_gt = (int)off;
    off = al(off + (size_t)HW * a.st * 4);
    a.off_ac = (int)off;
    off = al(off + (size_t)HW * a.sa * 4);
    a.off_w = (int)off;
    a.wmax = (int)wmax;
    off = al(off + wmax * 4);
    a.off_kt = (int)off;
    off = al(off + (size_t)ktmax * 4);
    a.off_red = (int)off;
    off = al(off + 16 * 8);
    a.off_ot = (int)off;
    off = al(off + (size_t)c.bwd_offs_per_net * 4);
    a.off_z = (int)off;   // 4 zeros + 4 ones, then zn + 4 zeros (a lane reads up to kq + cpt4 - 1)
    off = al(off + 32 + (size_t)(zn + 4) * 4);
    if (off > 160 * 1024) return 0;
    a.lds_bytes = (int)off;
    a.offs_per_net = c.bwd_offs_per_net;
    const LdsSave s = LdsSave::of(HW, c.nk, c.gc, c.R);
    a.save_img = s.img;
    a.save_t1 = s.t1;
    a.save_t2 = s.t2;
    a.save_st = s.st;
    ldsbwd_geom(c, a);
    return off;
}

TrainLayout Plan::train_layout(int B) const {
    TrainLayout T;
    const WsLayout L = layout(B);
    size_t off = align_up(L.total, 256);
    auto take = [&](size_t bytes) {
        size_t o = off;
        off = align_up(off + std::max<size_t>(bytes, 4), 256);
        return o;
    };
    const size_t Bz = (size_t)B;
    // the recompute scratch set holds any one layer's activations: per-image maxima over the layers
    int64_t m_y = 0, m_t1 = 0, m_t2 = 0, m_so = 0, m_nk = 0, m_gc = 0, m_u1 = 0, m_dense = 0, m_co = 0;
    int m_st = 1;
    for (const Coupling& c : couplings) {
        const int64_t npx = (int64_t)c.hc * c.wc;
        const StreamActs a(1, c);
        m_y = std::max<int64_t>(m_y, (int64_t)(c.R + 1) * a.y_f);
        m_t1 = std::max<int64_t>(m_t1, (int64_t)c.R * a.y_f);
        m_t2 = std::max<int64_t>(m_t2, (int64_t)c.R * a.t2_f);
        m_so = std::max<int64_t>(m_so, a.so_f);
        m_nk = std::max<int64_t>(m_nk, npx * c.nk);
        m_gc = std::max<int64_t>(m_gc, npx * c.gc);
        m_u1 = std::max<int64_t>(m_u1, npx * c.dc1);
        m_st = std::max(m_st, a.ln.count());
        m_dense = std::max<int64_t>(m_dense, 9LL * c.dc1 * c.nk);
        m_dense = std::max<int64_t>(m_dense, (int64_t)c.nk * c.nk);
        m_dense = std::max<int64_t>(m_dense, (int64_t)c.gc * c.nk);
        m_dense = std::max<int64_t>(m_dense, 9LL * c.nk * c.dc2);
        for (const Branch& b : c.br) m_dense = std::max<int64_t>(m_dense, 9LL * b.cin * b.cout);
        m_co = std::max<int64_t>(m_co, std::max(std::max(c.nk, c.dc2), c.gc));
    }
    T.save_u.assign(couplings.size(), 0);
    for (const Coupling& c : couplings) T.save_u[c.index] = take(Bz * c.H * c.W * c.D * 4);
    T.bw = take((size_t)std::max<int64_t>(n_bw, 1) * 4);
    for (int n = 0; n < 2; n++) {
        T.ys[n] = take(Bz * m_y * 4);
        T.t1s[n] = take(Bz * m_t1 * 4);
        T.t2s[n] = take(Bz * m_t2 * 4);
        T.so[n] = take(Bz * m_so * 4);
        T.dso[n] = take(Bz * m_so * 4);
        T.stats[n] = take(Bz * m_st * 2 * 4);
    }
    for (int n = 0; n < 2; n++) {
        T.dy[n] = take(Bz * m_nk * 4);
        T.dln[n] = take(Bz * m_nk * 4);
        T.dbuf[n] = take(Bz * m_nk * 4);
        T.dt1[n] = take(Bz * m_nk * 4);
        T.dc[n] = take(Bz * m_gc * 4);
        T.dt2[n] = take(Bz * m_gc * 4);
        T.du1c[n] = take(Bz * m_u1 * 4);
    }
    T.u1c = take(Bz * m_u1 * 4);
    for (int k = 0; k < 2; k++) T.duv[k] = take(Bz * L.n_uv * 4);
    T.dzy = take(Bz * L.n_uv * 4);
    for (int n = 0; n < 2; n++) {
        T.lnsum[n] = take(Bz * std::max(LNB_RS, LNR_MAXPARTS) * 2 * 8);
        // LN backward: per batch slice partial gamma / beta gradients [2][LNB_SLICES][n]
        T.lnpart[n] = take((size_t)2 * LNB_SLICES * std::max(m_nk, m_gc) * 4);
    }
    int chunks = 1, mchunks = WGRAD_MAX_CHUNKS;
    for (const Coupling& c : couplings) {
        chunks = std::max(chunks, wgrad_chunks(B, c.hc * c.wc));
        mchunks = std::max(mchunks, wgrad_direct_chunks(B, c.hc));   // (B of them once B > WGRAD_MAX_CHUNKS)
    }
    // the MFMA weight gradients write up to mchunks rows of [weights | bias]
    for (int n = 0; n < 2; n++) {
        T.wpart[n] = take((size_t)std::max(chunks, mchunks) * (m_dense + m_co) * 4);
        T.bpart[n] = take((size_t)chunks * m_co * 4);
    }
    T.dwpart = take(Bz * std::max(1, L.ld_parts) * 8);
    T.zeros = take(64 * 4);
    T.act_save.assign(couplings.size(), 0);
    T.so_save.assign(couplings.size(), 0);
    for (const Coupling& c : couplings) {
        if (!c.lds_bwd) continue;
        const int HW = c.hc * c.wc;
        const LdsSave s = LdsSave::of(HW, c.nk, c.gc, c.R);
        T.act_save[c.index] = take(2 * Bz * s.img * 4);
        T.so_save[c.index] = take(2 * Bz * HW * c.dc2 * 4);
        LdsBwdArgs g{};
        ldsbwd_geom(c, g);
        T.row_max = std::max(T.row_max, g.row);
        T.gsave_max = std::max(T.gsave_max, g.gsave_img);
    }
    if (T.row_max > 0) {
        T.rows = take(2 * Bz * T.row_max * 4);
        T.rows2 = take(2 * Bz * T.row_max * 4);
        for (int par = 0; par < 2; par++) {
            T.gsave[par] = take(2 * Bz * T.gsave_max * 4);
            for (int n = 0; n < 2; n++) T.dso_l[par][n] = take(Bz * m_so * 4);
        }
    }
    // streamed layers' saved activations, when all of them fit 16 GiB (SCHED_RECOMPUTE: none)
    T.ssave.assign(couplings.size(), TrainLayout::StreamSave{});
    T.has_ssave.assign(couplings.size(), 0);
    auto saves = [](const Coupling& c) { return !c.use_lds && !c.t2_mapped; };
    size_t need = 0;
    for (const Coupling& c : couplings)
        if (saves(c)) need += StreamActs(B, c).save_bytes();
    if ((opts.train_sched & SCHED_RECOMPUTE) == 0 && need <= (16ull << 30))
        for (const Coupling& c : couplings) {
            if (!saves(c)) continue;
            const StreamActs a(B, c);
            TrainLayout::StreamSave& s = T.ssave[c.index];
            for (int n = 0; n < 2; n++) {
                s.y[n] = take(a.y_bytes());
                s.t1[n] = take(a.t1_bytes());
                s.t2[n] = take(a.t2_bytes());
                s.st[n] = take(a.st_bytes());
            }
            s.so = take(a.so_bytes());
            T.has_ssave[c.index] = 1;
        }
    T.total = off;
    return T;
}

namespace {

// One training call's view: Exec's plan, parameters, workspace and stream (no aux image: the training
// kernels read the dense backward image bw), plus what only the backward has. Copied per net chain, so
// it refers to the call's TrainLayout instead of holding one.
struct TExec : Exec {
    float* dparams;
    const TrainLayout& T;
    float inv_batch_ = 0.f;
    const float* count = nullptr;   // device global image count (overrides inv_batch_)
    bool saved = false;             // the training forward saved the streamed layers' activations (flow backward)
    int net = 0;                    // which per-net scratch set this executor's launches use
    hipStream_t wst = nullptr;      // weight-gradient stream (null: on st)
    // data-gradient-only backward (flow_backward_data): no launch whose only outputs are parameter gradients,
    // dparams null; bw_ / zeros_: the dense backward image and the zeros block the caller packed once per
    // native call (null: the layout's own, filled by begin_backward)
    bool data_only = false;
    const float* bw_ = nullptr;
    const float* zeros_ = nullptr;
    const float* bw() const { return bw_ != nullptr ? bw_ : at<const float>(T.bw); }
    const float* zeros() const { return zeros_ != nullptr ? zeros_ : at<const float>(T.zeros); }
    double* lnsum() const { return at<double>(T.lnsum[net]); }
};

// what both entry points do first: the executor, and on its stream the dense backward image, zeroed
// parameter gradients and the zeros block
TExec begin_backward(Plan& p, const TrainLayout& T, const float* params, float* dparams, void* workspace, int B,
                     hipStream_t st) {
    TExec E{{p, params, nullptr, (char*)workspace, p.layout(B), B, st}, dparams, T};
    // pooled events: each record of this call gets its own (a re-recorded event that a queued wait still
    // references serialised the two nets' chains on the GPU); the previous call's waits are all enqueued
    p.tev_next = 0;
    if (p.n_bw > 0) launch_pack(params, p.dev_bw_map, E.at<float>(T.bw), (long long)p.n_bw, st);
    hchk(hipMemsetAsync(dparams, 0, (size_t)p.n_params * 4, st), "hipMemsetAsync");
    hchk(hipMemsetAsync(E.at<float>(T.zeros), 0, 64 * 4, st), "hipMemsetAsync");
    return E;
}

// ---- one convolution's three launches ------------------------------------------------------------------
struct Geom {   // the (compressed) image every conv of a coupling layer runs on
    int h, w;
};

// channels [off, off + c) of an NHWC tensor with cs floats per pixel (as cnf_coupling.cpp's Window)
template <class T>
struct Window {
    T* ptr = nullptr;
    int cs = 0, off = 0, c = 0;
};
using Src = Window<const float>;
using Dst = Window<float>;
template <class T>
Window<T> whole(T* p, int c) {   // a dense tensor of c channels
    return {p, c, 0, c};
}
template <class T>
Window<T> branch_in(T* t1, int nk, const Branch& b) {   // what branch b reads of the nk-channel t1
    return {t1, nk, b.cin_off, b.cin};
}
template <class T>
Window<T> branch_out(T* t2, int gc, const Branch& b) {   // branch b's slice of the gc-channel concat t2
    return {t2, gc, b.out_off, b.cout};
}

// LN-on-load descriptor of a conv input
struct LnIn {
    const float* stats = nullptr;
    const float* gamma = nullptr;
    const float* beta = nullptr;
    int act = 0;
};

// the fields a convolution and its data gradient share: out = W * in over pc's dense image
TConvArgs tconv_args(const TExec& E, Geom g, Src in, const PackedConv& pc, int dil, Dst out) {
    TConvArgs a{};
    a.in = in.ptr;
    a.in_cs = in.cs;
    a.in_off = in.off;
    a.K = in.c;
    a.w = E.bw() + pc.dw;
    a.wt = (long long)in.c * out.c;
    a.out = out.ptr;
    a.out_cs = out.cs;
    a.out_off = out.off;
    a.N = out.c;
    a.H = g.h;
    a.W = g.w;
    a.taps = pc.taps;
    a.dil = dil;
    a.B = E.B;
    a.zero = E.zeros();
    return a;
}

// out = conv(LN(in)) (+ res) over the dense image of pc (forward, sgn = +1)
void conv_fwd(TExec& E, Geom g, Src in, const LnIn& ln, const PackedConv& pc, int dil, Dst out,
              const float* res = nullptr) {
    TConvArgs a = tconv_args(E, g, in, pc, dil, out);
    a.stats = ln.stats;
    a.gamma = ln.gamma;
    a.beta = ln.beta;
    a.act = ln.act;
    a.wk = out.c;
    a.wn = 1;
    a.bias = E.bw() + pc.db;
    a.res = res;
    a.sgn = 1;
    launch_tconv(a, E.st);
}

// an LN whose input has dx's layout and whose output gradient dx is: conv_dgrad's kernel also writes
// that LN backward's per-image reduction partials to the net's lnsum
struct LnRed {
    const float* x = nullptr;
    const float* gamma = nullptr;
    const float* stats = nullptr;
    int base = 0;   // this launch's first partial (several launches that write disjoint windows share one LN)
};
// dx (=|+=) conv^T(dy); returns the partials per image written for lr (0: not fused — ln_bwd runs
// k_lnb_reduce, as it always does under ALT_LNB_REDUCE)
int conv_dgrad(TExec& E, Geom g, Src dy, const PackedConv& pc, int dil, Dst dx, int accumulate,
               const LnRed* lr = nullptr) {
    TConvArgs a = tconv_args(E, g, dy, pc, dil, dx);
    if (lr != nullptr && lr->stats != nullptr && (opts().train_alt & ALT_LNB_REDUCE) == 0) {
        a.lnr_x = lr->x;
        a.lnr_gamma = lr->gamma;
        a.lnr_stats = lr->stats;
        a.lnr_part = E.lnsum();
        a.lnr_base = lr->base;
        a.lnr_stride = LNR_MAXPARTS;
    }
    a.wk = 1;
    a.wn = dy.c;
    a.accumulate = accumulate;
    a.sgn = -1;
    return launch_tconv(a, E.st);
}

hipEvent_t tevent(Plan& p) {
    constexpr int flags = (int)hipEventDisableTiming;
    if (p.tev_next == p.tev.size()) {
        hipEvent_t e;
        hchk(hipEventCreateWithFlags(&e, flags), "hipEventCreate");
        p.tev.push_back(e);
    }
    return p.tev[p.tev_next++];
}

WGradArgs wgrad_args(const TExec& E, Geom g, Src x, const LnIn& ln, Src dy, const PackedConv& pc, int dil) {
    WGradArgs a{};
    a.x = x.ptr;
    a.x_cs = x.cs;
    a.x_off = x.off;
    a.CI = x.c;
    a.stats = ln.stats;
    a.gamma = ln.gamma;
    a.beta = ln.beta;
    a.act = ln.act;
    a.dy = dy.ptr;
    a.dy_cs = dy.cs;
    a.dy_off = dy.off;
    a.CO = dy.c;
    a.part = E.at<float>(E.T.wpart[E.net]);
    a.bpart = E.at<float>(E.T.bpart[E.net]);
    a.H = g.h;
    a.W = g.w;
    a.taps = pc.taps;
    a.dil = dil;
    a.B = E.B;
    return a;
}

// dW, db of a conv on stream st: the kernel its shape allows, then the scatter of its partial rows
// through the dense map onto the canonical parameters
void wgrad_launch(const TExec& E, WGradArgs a, const PackedConv& pc, hipStream_t st) {
    const int cin = a.CI, cout = a.CO;
    const int64_t* map = E.p.dev_bw_map;
    const long long nw = (long long)pc.taps * cin * cout;
    const WGradChoice k = wgrad_choice(E.B, a.H, a.W, pc.taps, a.dil, cin, cout, a.x_cs, pc.db == pc.dw + nw);
    a.chunks = k.chunks;
    if (k.kernel == WGRAD_VALU) {
        a.chunk_px = k.chunk_px;
        launch_wgrad(a, st);
        launch_grad_scatter(a.part, a.chunks, nw, map + pc.dw, E.dparams, st);
        launch_grad_scatter(a.bpart, a.chunks, cout, map + pc.db, E.dparams, st);
        return;
    }
    // thin outputs (the streamed conv_out, CO = dc2): k_wgrad_thin, rows of [weights | bias] as below
    if (k.kernel == WGRAD_THIN) {
        launch_wgrad_thin(a, st);
        launch_grad_scatter(a.part, a.chunks, nw + cout, map + pc.dw, E.dparams, st);
        return;
    }
    // k_wgrad_direct (ALT_WGRAD_BAND: k_wgrad_band): rows of [weights | bias]; the dense image keeps the
    // bias right after the weights (pc.db == pc.dw + taps * cin * cout), so one scatter reduces both
    if (k.kernel == WGRAD_DIRECT) {
        a.chunk_px = k.chunk_px;
        a.zero = E.zeros();
    }
    launch_wgrad(a, st);
    if (pc.db != pc.dw + nw) throw std::logic_error("dense image: bias not after the weights");
    launch_grad_scatter(a.part, a.chunks, nw + cout, map + pc.dw, E.dparams, st);
}

// dW, db of a conv from X (LN-on-load) and dY, on E's weight-gradient stream when it has one: there it
// waits for the chain's launches so far (its X and dY are ready) and returns the event of its completion
// (null on the chain's own stream, where order alone protects dY)
hipEvent_t conv_wgrad(TExec& E, Geom g, Src x, const LnIn& ln, Src dy, const PackedConv& pc, int dil) {
    if (E.data_only) return nullptr;   // (no reader of dY on another stream either)
    const WGradArgs a = wgrad_args(E, g, x, ln, dy, pc, dil);
    if (E.wst == nullptr) {
        wgrad_launch(E, a, pc, E.st);
        return nullptr;
    }
    hipEvent_t in = tevent(E.p), done = tevent(E.p);
    hchk(hipEventRecord(in, E.st), "hipEventRecord");
    hchk(hipStreamWaitEvent(E.wst, in, 0), "hipStreamWaitEvent");
    wgrad_launch(E, a, pc, E.wst);
    hchk(hipEventRecord(done, E.wst), "hipEventRecord");
    return done;
}

void ln_bwd(TExec& E, const float* x, const float* dxo, const LnIn& ln, long long n, float* dx, int accumulate,
            int64_t g_off, int64_t b_off, int presum = 0, unsigned long long cmask = 0, int cmod = 0) {
    // (data-only: k_lnb_apply's gamma / beta partials stay in lnpart, no k_lnb_gsum)
    const bool pg = ln.stats != nullptr && !E.data_only;
    launch_ln_backward(x, dxo, ln.gamma, ln.stats, E.lnsum(), n, E.B, 1, dx, accumulate,
                       pg ? E.dparams + g_off : nullptr, pg ? E.dparams + b_off : nullptr,
                       E.at<float>(E.T.lnpart[E.net]), E.st, presum, LNR_MAXPARTS, cmask, cmod);
}

// the plan's side stream and fork / join events (created on first use on the current device)
void ensure_side(Plan& p) {
    int dev = 0;
    hchk(hipGetDevice(&dev), "hipGetDevice");
    if (p.side != nullptr && p.side_device == dev) return;
    if (p.side != nullptr) {
        (void)hipEventDestroy(p.ev_fork);
        (void)hipEventDestroy(p.ev_join);
        (void)hipStreamDestroy(p.side);
        for (hipStream_t& s : p.wside) (void)hipStreamDestroy(s);
        p.side = nullptr;
        // the pooled events belong to the old device too: recording them on the new device's streams fails
        for (hipEvent_t e : p.tev) (void)hipEventDestroy(e);
        p.tev.clear();
        p.tev_next = 0;
    }
    hchk(hipStreamCreateWithFlags(&p.side, hipStreamNonBlocking), "hipStreamCreate");
    hchk(hipEventCreateWithFlags(&p.ev_fork, hipEventDisableTiming), "hipEventCreate");
    hchk(hipEventCreateWithFlags(&p.ev_join, hipEventDisableTiming), "hipEventCreate");
    for (hipStream_t& s : p.wside) hchk(hipStreamCreateWithFlags(&s, hipStreamNonBlocking), "hipStreamCreate");
    p.side_device = dev;
}

// `to` waits for everything enqueued on `from` so far
void stream_wait(hipStream_t from, hipStream_t to, hipEvent_t ev) {
    hchk(hipEventRecord(ev, from), "hipEventRecord");
    hchk(hipStreamWaitEvent(to, ev, 0), "hipStreamWaitEvent");
}

// coupling law backward at u for upstream dv: du (u2 part, u1 copy), dL/d s_pre, dL/dt, and dL/d tanh_w
// (per-workgroup partials, then their sum)
void coupling_law_backward(TExec& E, const Coupling& c, const float* u, const float* dv, float* du,
                           const float* s_pre, float* ds_pre, float* dt) {
    CoupBwArgs a{};
    a.u = u;
    a.dv = dv;
    a.s_pre = s_pre;
    a.tanh_w = E.params + c.net[0].tanh_w;
    a.du = du;
    a.ds_pre = ds_pre;
    a.dt = dt;
    a.dw_part = E.at<double>(E.T.dwpart);
    a.g_ld = -E.inv_batch_;
    a.count = E.count;
    a.H = c.H;
    a.W = c.W;
    a.D = c.D;
    a.mask = c.mask;
    a.mask_c = c.mask_c;
    a.hc = c.hc;
    a.wc = c.wc;
    a.dc1 = c.dc1;
    a.dc2 = c.dc2;
    const int np = std::max(1, E.L.ld_parts);
    launch_coupling_backward(a, E.B, np, E.st);
    if (!E.data_only) launch_dsum(a.dw_part, (long long)E.B * np, E.dparams + c.net[0].tanh_w, E.st);
}

// du += the two nets' u1 gradients, net A's first (fixed order: bitwise reproducible)
void scatter_du1c(TExec& E, const Coupling& c, float* du, hipStream_t st) {
    for (int n = 0; n < 2; n++)
        launch_scatter_add_u1c(E.at<float>(E.T.du1c[n]), du, E.B, c.H, c.W, c.D, c.mask, c.hc, c.wc, c.dc1, st);
}

// The fused backward of a k_net_lds layer (cnf_ldsbwd.hip) from the activations the training forward
// saved: coupling law backward, k_lds_bwd for both nets, the batch sum of the gradient rows. Split
// (par >= 0): the data-gradient chain (k_lds_bwd mode 1, storing the gradients the weight gradients
// need) on the caller's stream, then the weight gradients (mode 2) and the row sum on the side stream
// wside[1] behind an event, so they run on the CUs the next layer's chain leaves idle (one workgroup per
// (image, net) fills half the GPU at B = 64); returns the event of the row sum (the layer's parameter
// gradients complete), null unsplit. par selects the alternating buffer set.
hipEvent_t coupling_backward_lds(TExec& E, const Coupling& c, const float* u, const float* dv, float* du, int par) {
    const int B = E.B;
    const bool split = par >= 0;
    float* dso0 = E.at<float>(split ? E.T.dso_l[par][0] : E.T.dso[0]);
    float* dso1 = E.at<float>(split ? E.T.dso_l[par][1] : E.T.dso[1]);
    coupling_law_backward(E, c, u, dv, du, E.at<float>(E.T.so_save[c.index]), dso0, dso1);
    LdsBwdArgs a;
    if (ldsbwd_setup(E.p, c, a) == 0) throw std::logic_error("fused LDS backward planned for a layer it does not fit");
    a.save = E.at<float>(E.T.act_save[c.index]);
    a.dso[0] = dso0;
    a.dso[1] = dso1;
    a.u = u;
    a.du1c[0] = E.at<float>(E.T.du1c[0]);
    a.du1c[1] = E.at<float>(E.T.du1c[1]);
    a.params = E.params;
    a.bw = E.bw();
    a.bw_map = E.p.dev_bw_map;
    a.offs = E.p.dev_table + c.dev_bwd_offs;
    a.part = E.at<float>(split && par == 1 ? E.T.rows2 : E.T.rows);
    a.row = E.T.row_max;
#ifdef CNF_DIAG
    static const bool stamps = [] {   // diagnostic builds: phase stamps (profiles/diag/diag_bwd_stamps.py)
        const char* e = std::getenv("CNF_LDSBWD_STAMPS");
        return e && std::atoi(e) != 0;
    }();
#else
    constexpr bool stamps = false;
#endif
    a.stamps = stamps ? 1 : 0;
    const NetParams& n0 = c.net[0];
    const NetParams& n1 = c.net[1];
    if (!split) {
        a.mode = 0;
        launch_lds_bwd(a, B, E.st);   // (data-only: as it is, its gradient rows stay in the workspace)
        if (!E.data_only)
            launch_grad_rows(a.part, B, a.row, n0.lo, n1.lo, (int)(n0.hi - n0.lo), (int)(n1.hi - n1.lo), E.dparams,
                             E.st);
        scatter_du1c(E, c, du, E.st);
        return nullptr;
    }
    if (!E.data_only) ensure_side(E.p);
    a.gsave = E.at<float>(E.T.gsave[par]);
    a.mode = 1;
    launch_lds_bwd(a, B, E.st);
    scatter_du1c(E, c, du, E.st);
    if (E.data_only) return nullptr;   // the chain alone: no weight-gradient launch, no side stream
    hipStream_t ws = E.p.wside[1];
    stream_wait(E.st, ws, tevent(E.p));   // the chain's stored gradients and LN rows
    a.mode = 2;
    a.stamps = 0;
    launch_lds_bwd(a, B, ws);
    launch_grad_rows(a.part, B, a.row, n0.lo, n1.lo, (int)(n0.hi - n0.lo), (int)(n1.hi - n1.lo), E.dparams, ws);
    hipEvent_t done = tevent(E.p);
    hchk(hipEventRecord(done, ws), "hipEventRecord");
    return done;
}

// How the grouped stage's data gradients and the LN2 backward share dbuf, from the branches' input
// windows alone. Pairwise disjoint windows (the reference group mode's closure windows [(card - 1) w,
// card w) of each branch width w): every element of dbuf is final after the one launch that writes it,
// so the LN2 reduction rides on those launches, each adding its window's partials after the previous
// ones'. Disjoint over <= 64 channels (and not ALT_ZERO_DT1): the branches store their windows without
// accumulating and the LN2 backward reads the channels outside `mask` as 0, so dbuf is not zeroed first.
struct BranchWindows {
    bool disjoint = true, masked = false;
    unsigned long long mask = 0;
};
BranchWindows branch_windows(const Coupling& c) {
    BranchWindows bw;
    const int nb = (int)c.br.size();
    for (int i = 0; i < nb; i++) {
        for (int j = i + 1; j < nb; j++)
            bw.disjoint = bw.disjoint && (c.br[i].cin_off + c.br[i].cin <= c.br[j].cin_off ||
                                          c.br[j].cin_off + c.br[j].cin <= c.br[i].cin_off);
        for (int ch = c.br[i].cin_off; ch < c.br[i].cin_off + c.br[i].cin && ch < 64; ch++) bw.mask |= 1ull << ch;
    }
    bw.masked = bw.disjoint && c.nk <= 64 && (opts().train_alt & ALT_ZERO_DT1) == 0;
    return bw;
}

// One streamed coupling layer's backward (conv_cINN_make_model.py:1850-1880 through the layer). The two
// s,t nets are independent until the coupling law joins them, so net b's chain (and recompute) runs on
// the plan's side stream with its own scratch set while net A's runs on the caller's: the many small,
// latency-bound launches of the two chains overlap. Each net's weight gradients run behind its chain on
// a stream of their own (SCHED_WGRAD_ON_CHAIN: on the chain's).
struct StreamedBwd {
    struct Step {   // one stage of a net's chain: (this->*stage)(net, r)
        void (StreamedBwd::*stage)(int, int);
        int r;
    };
    // Buffer reuse. A chain's dY buffers are written once per residual block, and the weight gradient
    // that reads one runs on another stream: wgrad() notes its completion event in the buffer, and the
    // stage that next overwrites the buffer takes it through fresh(), which makes the chain wait for that
    // reader first — dt2: conv_b's LN3 backward (read by the block after's branches), dt1: the LN2
    // backward (read by the block after's conv_a), dy: conv_a's LN1 backward (read by this block's conv_b).
    struct DyBuf {
        float* p = nullptr;
        hipEvent_t reader = nullptr;
    };
    struct Scratch {
        DyBuf dy, dt1, dt2;
        float *dln, *dbuf, *dcb, *du1c, *dso;
    };

    const Coupling& c;
    TExec X[2];   // per net: its chain stream, weight-gradient stream and scratch set
    const bool ln;
    const float* const P;
    const Geom g;
    const long long n_nk, n_gc;   // elements per image of an nk- / gc-channel tensor
    const bool saved;             // the forward saved this layer's activations (else: recompute)
    const StreamActs A;
    const BranchWindows bwin;
    float* const u1c;
    Scratch S[2];

    StreamedBwd(TExec& E, const Coupling& c_)
        : c(c_), X{E, E}, ln(E.p.desc.layer_norm != 0), P(E.params), g{c_.hc, c_.wc},
          n_nk((long long)c_.hc * c_.wc * c_.nk), n_gc((long long)c_.hc * c_.wc * c_.gc),
          saved(E.saved && E.T.has_ssave[c_.index]),
          A(saved ? StreamActs::saved(E.ws, E.T.ssave[c_.index], E.B, c_) : StreamActs::scratch(E.ws, E.T, E.B, c_)),
          bwin(branch_windows(c_)), u1c(E.at<float>(E.T.u1c)) {
        ensure_side(E.p);
        const bool wstreams = (opts().train_sched & SCHED_WGRAD_ON_CHAIN) == 0;
        X[1].net = 1;
        X[1].st = E.p.side;
        for (int n = 0; n < 2; n++) {
            X[n].wst = wstreams && !E.data_only ? E.p.wside[n] : nullptr;
            const TrainLayout& T = E.T;
            S[n] = Scratch{{E.at<float>(T.dy[n])}, {E.at<float>(T.dt1[n])}, {E.at<float>(T.dt2[n])},
                           E.at<float>(T.dln[n]), E.at<float>(T.dbuf[n]), E.at<float>(T.dc[n]),
                           E.at<float>(T.du1c[n]), E.at<float>(T.dso[n])};
        }
    }

    LnIn lnin(int n, int i, int64_t gamma, int64_t beta) const {
        LnIn l;
        l.act = 1;
        if (ln) {
            l.stats = A.stats(n, i);
            l.gamma = P + gamma;
            l.beta = P + beta;
        }
        return l;
    }
    void wgrad(int n, Src x, const LnIn& l, DyBuf& dy, Src dyw, const PackedConv& pc, int dil = 1) {
        dy.reader = conv_wgrad(X[n], g, x, l, dyw, pc, dil);
    }
    float* fresh(int n, const DyBuf& b) {
        if (b.reader != nullptr) hchk(hipStreamWaitEvent(X[n].st, b.reader, 0), "hipStreamWaitEvent");
        return b.p;
    }

    // net n's activations again, from the gathered u1c
    void recompute(int n) {
        TExec& E = X[n];
        const NetParams& np = c.net[n];
        const int nk = c.nk, gc = c.gc, B = E.B;
        auto stats = [&](const float* x, long long per_image, int i) {
            if (ln) launch_ln_stats(x, per_image, B, 1, A.stats(n, i), E.st);
        };
        conv_fwd(E, g, whole<const float>(u1c, c.dc1), LnIn{}, np.ci, 1, whole(A.y(n, 0), nk));
        stats(A.y(n, 0), n_nk, A.ln.ln1(0));
        for (int r = 0; r < c.R; r++) {
            const RBParams& rb = np.rb[r];
            conv_fwd(E, g, whole<const float>(A.y(n, r), nk), lnin(n, A.ln.ln1(r), rb.ln1g, rb.ln1b), rb.ca, 1,
                     whole(A.t1(n, r), nk));
            stats(A.t1(n, r), n_nk, A.ln.ln2(r));
            for (size_t bi = 0; bi < c.br.size(); bi++) {
                const Branch& b = c.br[bi];
                conv_fwd(E, g, branch_in<const float>(A.t1(n, r), nk, b), lnin(n, A.ln.ln2(r), rb.ln2g, rb.ln2b),
                         rb.gc[bi], b.dil, branch_out(A.t2(n, r), gc, b));
            }
            stats(A.t2(n, r), n_gc, A.ln.ln3(r));
            conv_fwd(E, g, whole<const float>(A.t2(n, r), gc), lnin(n, A.ln.ln3(r), rb.ln3g, rb.ln3b), rb.cb, 1,
                     whole(A.y(n, r + 1), nk), A.y(n, r));
            stats(A.y(n, r + 1), n_nk, A.ln.ln1(r + 1));
        }
        conv_fwd(E, g, whole<const float>(A.y(n, c.R), nk), lnin(n, A.ln.ln_out(), np.ln_out_g, np.ln_out_b), np.co, 1,
                 whole(A.so(n), c.dc2));
    }

    // coupling law backward -> du (u2 part, u1 copy), dL/d s_pre, dL/dt, dL/dw
    void law(const float* u, const float* dv, float* du) {
        coupling_law_backward(X[0], c, u, dv, du, A.so(0), S[0].dso, S[1].dso);
    }

    void conv_out(int n, int = 0) {
        Scratch& s = S[n];
        const NetParams& np = c.net[n];
        const float* y = A.y(n, c.R);
        const LnIn lo = lnin(n, A.ln.ln_out(), np.ln_out_g, np.ln_out_b);
        const Src dso = whole<const float>(s.dso, c.dc2);
        conv_wgrad(X[n], g, whole(y, c.nk), lo, dso, np.co, 1);
        const LnRed ro{y, lo.gamma, lo.stats};
        const int ps = conv_dgrad(X[n], g, dso, np.co, 1, whole(s.dln, c.nk), 0, &ro);
        ln_bwd(X[n], y, s.dln, lo, n_nk, fresh(n, s.dy), 0, np.ln_out_g, np.ln_out_b, ps);
    }

    // conv_b (y_{r+1} = y_r + conv_b(LN3(t2_r))) and the LN3 backward: dy -> dt2
    void conv_b(int n, int r) {
        Scratch& s = S[n];
        const RBParams& rb = c.net[n].rb[r];
        const float* t2 = A.t2(n, r);
        const LnIn l3 = lnin(n, A.ln.ln3(r), rb.ln3g, rb.ln3b);
        const Src dy = whole<const float>(s.dy.p, c.nk);
        wgrad(n, whole(t2, c.gc), l3, s.dy, dy, rb.cb);
        const LnRed r3{t2, l3.gamma, l3.stats};
        const int ps = conv_dgrad(X[n], g, dy, rb.cb, 1, whole(s.dcb, c.gc), 0, &r3);
        ln_bwd(X[n], t2, s.dcb, l3, n_gc, fresh(n, s.dt2), 0, rb.ln3g, rb.ln3b, ps);
    }

    // the grouped dilated branches and the LN2 backward: dt2 -> dt1 (through dbuf, see BranchWindows)
    void branches(int n, int r) {
        Scratch& s = S[n];
        TExec& E = X[n];
        const RBParams& rb = c.net[n].rb[r];
        const float* t1 = A.t1(n, r);
        const LnIn l2 = lnin(n, A.ln.ln2(r), rb.ln2g, rb.ln2b);
        if (!bwin.masked) hchk(hipMemsetAsync(s.dbuf, 0, (size_t)E.B * n_nk * 4, E.st), "hipMemsetAsync");
        int ps = 0;
        bool fused = bwin.disjoint;
        for (size_t bi = 0; bi < c.br.size(); bi++) {
            const Branch& b = c.br[bi];
            const Src dt2 = branch_out<const float>(s.dt2.p, c.gc, b);
            wgrad(n, branch_in(t1, c.nk, b), l2, s.dt2, dt2, rb.gc[bi], b.dil);
            LnRed r2{t1, l2.gamma, l2.stats};
            r2.base = ps;
            const int np = conv_dgrad(E, g, dt2, rb.gc[bi], b.dil, branch_in(s.dbuf, c.nk, b), bwin.masked ? 0 : 1,
                                      fused ? &r2 : nullptr);
            fused = fused && np > 0;
            ps += np;
        }
        if (!fused) ps = 0;   // (k_lnb_reduce, over whatever partials were written)
        ln_bwd(E, t1, s.dbuf, l2, n_nk, fresh(n, s.dt1), 0, rb.ln2g, rb.ln2b, ps, bwin.masked ? bwin.mask : 0ull,
               bwin.masked ? c.nk : 0);
    }

    // conv_a and the LN1 backward: dt1 -> dy (added to the residual path's gradient)
    void conv_a(int n, int r) {
        Scratch& s = S[n];
        const RBParams& rb = c.net[n].rb[r];
        const float* y = A.y(n, r);
        const LnIn l1 = lnin(n, A.ln.ln1(r), rb.ln1g, rb.ln1b);
        const Src dt1 = whole<const float>(s.dt1.p, c.nk);
        wgrad(n, whole(y, c.nk), l1, s.dt1, dt1, rb.ca);
        const LnRed r1{y, l1.gamma, l1.stats};
        const int ps = conv_dgrad(X[n], g, dt1, rb.ca, 1, whole(s.dln, c.nk), 0, &r1);
        ln_bwd(X[n], y, s.dln, l1, n_nk, fresh(n, s.dy), 1, rb.ln1g, rb.ln1b, ps);
    }

    void conv_in(int n, int = 0) {
        Scratch& s = S[n];
        const NetParams& np = c.net[n];
        const Src dy = whole<const float>(s.dy.p, c.nk);
        conv_wgrad(X[n], g, whole<const float>(u1c, c.dc1), LnIn{}, dy, np.ci, 1);
        conv_dgrad(X[n], g, dy, np.ci, 1, whole(s.du1c, c.dc1), 0);
    }

    void run(const float* u, const float* dv, float* du) {
        TExec& E = X[0];
        hipStream_t side = X[1].st;
        launch_gather_u1c(u, u1c, E.B, c.H, c.W, c.D, c.mask, c.hc, c.wc, c.dc1, E.st);
        stream_wait(E.st, side, tevent(E.p));   // u1c gathered
        for (int n = 0; n < 2 && !saved; n++) recompute(n);
        stream_wait(side, E.st, tevent(E.p));   // both nets' outputs
        law(u, dv, du);
        stream_wait(E.st, side, tevent(E.p));   // dL/d s_pre, dL/dt
        // a net's chain, last conv first
        using S = StreamedBwd;
        std::vector<Step> steps{{&S::conv_out, 0}};
        for (int r = c.R - 1; r >= 0; r--)
            for (auto stage : {&S::conv_b, &S::branches, &S::conv_a}) steps.push_back({stage, r});
        steps.push_back({&S::conv_in, 0});
        // The two chains are enqueued interleaved, step by step: the GPU starts a stream's kernels in about
        // the order the host submitted them across streams (measured: no kernel ran more than ~15
        // submissions ahead of the newest finished one), so a chain enqueued whole after the other only
        // overlapped it at the end. SCHED_NET_OUTER enqueues net A's chain, then net b's.
        if ((opts().train_sched & SCHED_NET_OUTER) == 0) {
            for (Step s : steps)
                for (int n = 0; n < 2; n++) (this->*s.stage)(n, s.r);
        } else {
            for (int n = 0; n < 2; n++)
                for (Step s : steps) (this->*s.stage)(n, s.r);
        }
        stream_wait(side, E.st, tevent(E.p));   // net b's chain done
        for (int n = 0; n < 2; n++)             // and both nets' weight gradients
            if (X[n].wst) stream_wait(X[n].wst, E.st, tevent(E.p));
        scatter_du1c(E, c, du, E.st);
    }
};

}  // namespace

void flow_backward(Plan& p, const float* params, const float* xy, const float* zy, void* workspace, int B,
                   float inv_batch, float* dparams, hipStream_t st, const float* count, LayerDoneFn done, void* user) {
    const TrainLayout TL = p.train_layout(B);
    TExec E = begin_backward(p, TL, params, dparams, workspace, B, st);
    E.inv_batch_ = inv_batch;
    E.count = count;
    E.saved = true;
    const WsLayout& L = E.L;
    const int* T = p.dev_table;
    const int nuv = (int)L.n_uv;
    const cnf_flow_desc& d = p.desc;
    float* dzy = E.at<float>(E.T.dzy);
    launch_nll_grad(xy, zy, dzy, B, d.io_h * d.io_w, d.io_d, d.x_d, d.lambda_y, inv_batch, count, st);
    float* buf[2] = {E.at<float>(E.T.duv[0]), E.at<float>(E.T.duv[1])};
    int which = 0;
    launch_map_gather(dzy, buf[which], T + p.dev_final_orig, p.last_n, nuv, p.last_n, B, st);
    float* cur = buf[which];
    which ^= 1;
    int bi = (int)p.boundaries.size() - 1;
    // split LDS layers: their weight gradients finish behind the next layers on a side stream; a layer's
    // buffer set (parity of its LDS-layer count) is reused two LDS layers later, when the caller's stream
    // first waits for them — that is also when the layer's gradients are complete for `done`
    const bool split = opts().lds_bwd == 2;   // (debug option LDS_BWD=1: one launch per layer)
    struct Pending {
        int ci = -1;
        hipEvent_t ev = nullptr;
    } pend[2];
    auto flush = [&](int par) {
        if (pend[par].ci < 0) return;
        hchk(hipStreamWaitEvent(st, pend[par].ev, 0), "hipStreamWaitEvent");
        if (done != nullptr) done(user, pend[par].ci);
        pend[par].ci = -1;
    };
    int lds_k = 0;
    for (int li = (int)p.layers.size() - 1; li >= 0; li--) {
        const Layer& ly = p.layers[li];
        if (ly.kind == CNF_LAYER_COUPLING) {
            const Coupling& c = p.couplings[ly.ci];
            float* nxt = buf[which];
            if (c.lds_bwd && split) {
                const int par = lds_k++ & 1;
                flush(par);
                pend[par].ev = coupling_backward_lds(E, c, E.at<float>(E.T.save_u[c.index]), cur, nxt, par);
                pend[par].ci = c.index;
            } else {
                if (c.lds_bwd)
                    coupling_backward_lds(E, c, E.at<float>(E.T.save_u[c.index]), cur, nxt, -1);
                else
                    StreamedBwd(E, c).run(E.at<float>(E.T.save_u[c.index]), cur, nxt);
                // every launch writing this layer's parameter gradients is ordered before anything enqueued
                // on st from here (its side streams joined st): the caller may reduce them now
                if (done != nullptr) done(user, c.index);
            }
            cur = nxt;
            which ^= 1;
        } else if (ly.kind == CNF_LAYER_FACTOR) {
            const Boundary& b = p.boundaries[bi--];
            float* prev = buf[which];
            launch_map_scatter(cur, prev, nullptr, T + b.dev_keep_src, b.n_next, b.n_next, b.n_cur, B, st);
            launch_map_scatter(dzy, prev, T + b.dev_fac_orig, T + b.dev_fac_src, b.n_fac, nuv, b.n_cur, B, st);
            cur = prev;
            which ^= 1;
        }
    }
    // the last split layers (the older first)
    const int last = lds_k & 1;
    flush(last);
    flush(last ^ 1);
    hchk(hipGetLastError(), "training kernel launch");
}

const float* flow_backward_data(Plan& p, const float* params, const float* bw, const float* zeros, const float* dzy,
                                void* workspace, int B, hipStream_t st) {
    const TrainLayout TL = p.train_layout(B);
    TExec E{{p, params, nullptr, (char*)workspace, p.layout(B), B, st}, nullptr, TL};
    p.tev_next = 0;   // (as begin_backward: the previous call's waits are all enqueued)
    E.data_only = true;
    E.bw_ = bw;
    E.zeros_ = zeros;
    E.inv_batch_ = -1.f;   // dL/d(per-image log-det) = +1
    E.saved = true;
    const WsLayout& L = E.L;
    const int* T = p.dev_table;
    const int nuv = (int)L.n_uv;
    float* buf[2] = {E.at<float>(E.T.duv[0]), E.at<float>(E.T.duv[1])};
    int which = 0;
    launch_map_gather(dzy, buf[which], T + p.dev_final_orig, p.last_n, nuv, p.last_n, B, st);
    float* cur = buf[which];
    which ^= 1;
    int bi = (int)p.boundaries.size() - 1;
    const bool split = opts().lds_bwd == 2;
    int lds_k = 0;
    for (int li = (int)p.layers.size() - 1; li >= 0; li--) {
        const Layer& ly = p.layers[li];
        if (ly.kind == CNF_LAYER_COUPLING) {
            const Coupling& c = p.couplings[ly.ci];
            float* nxt = buf[which];
            const float* u = E.at<float>(E.T.save_u[c.index]);
            if (c.lds_bwd)   // (split: the buffer sets alternate as in flow_backward; nothing runs behind the chain)
                coupling_backward_lds(E, c, u, cur, nxt, split ? lds_k++ & 1 : -1);
            else
                StreamedBwd(E, c).run(u, cur, nxt);
            cur = nxt;
            which ^= 1;
        } else if (ly.kind == CNF_LAYER_FACTOR) {
            const Boundary& b = p.boundaries[bi--];
            float* prev = buf[which];
            launch_map_scatter(cur, prev, nullptr, T + b.dev_keep_src, b.n_next, b.n_next, b.n_cur, B, st);
            launch_map_scatter(dzy, prev, T + b.dev_fac_orig, T + b.dev_fac_src, b.n_fac, nuv, b.n_cur, B, st);
            cur = prev;
            which ^= 1;
        }
    }
    hchk(hipGetLastError(), "training kernel launch");
    return cur;
}

void pack_backward_image(Plan& p, const float* params, float* bw, float* zeros, hipStream_t st) {
    if (p.n_bw > 0) launch_pack(params, p.dev_bw_map, bw, (long long)p.n_bw, st);
    hchk(hipMemsetAsync(zeros, 0, 64 * 4, st), "hipMemsetAsync");
}

void coupling_layer_backward(Plan& p, int ci, const float* params, const float* u, const float* dv, float* du,
                             float g_ld, void* workspace, int B, float* dparams, hipStream_t st) {
    const TrainLayout T = p.train_layout(B);
    TExec E = begin_backward(p, T, params, dparams, workspace, B, st);
    E.inv_batch_ = -g_ld;
    // (a lone layer has no saved activations: E.saved stays false and the layer recomputes them)
    StreamedBwd(E, p.couplings[ci]).run(u, dv, du);
    hchk(hipGetLastError(), "training kernel launch");
}

}  // namespace cnf
