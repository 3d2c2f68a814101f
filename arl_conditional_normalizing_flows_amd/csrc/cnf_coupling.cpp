// cnf_coupling.cpp — one planned coupling layer as launches on the caller's stream: the conv launch
// preparers (k_conv3, k_pw, k_conv1, k_convtap), k_net_lds, the streamed s,t net stage by stage
// (conv_cINN_make_model.py:1114-1213) and the affine coupling law. Host code only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>

#include "cnf_api.h"
#include "cnf_kernels.h"
#include "cnf_plan.h"

namespace cnf {

// ----------------------------------------------------------------------------------------------
// geometry
// ----------------------------------------------------------------------------------------------
Geo conv_geo(int h, int w) {
    Geo g;
    g.MR = (h * w >= 1024) ? 2 : 1;
    const int pt = 64 * g.MR;
    if (w > pt) throw std::invalid_argument("image width too large for the row-band tiling (w > 128)");
    g.TH = std::min(h, std::max(1, pt / w));
    g.tiles = (h + g.TH - 1) / g.TH;
    return g;
}

static int lds_stride(int cin) {  // pixel stride in floats, == 2 (mod 4): conflict-free A reads
    int s = std::max(cin, 2);
    while (s % 4 != 2) s++;
    return s;
}

// k_conv1: tiles of 64 * MR pixels
static int conv1_mr(int h, int w) { return h * w >= 1024 ? 2 : 1; }
static int conv1_tiles(int h, int w) { return (h * w + 64 * conv1_mr(h, w) - 1) / (64 * conv1_mr(h, w)); }

int ld_parts_for(int npx) { return std::max(1, std::min(16, (npx + 63) / 64)); }

// LN-partial slots per image: one per producing wave. Plan::layout sizes the slabs from these and the
// launch code below advances its slot cursor by them, so a tile shape is changed in one place.
constexpr int PW_WAVES = 4;                                                // k_pw: 4 waves x 16 pixels per tile
static int pw_tiles(int h, int w) { return (h * w + 16 * PW_WAVES - 1) / (16 * PW_WAVES); }
int ln_slots_conv3(int h, int w) { return 4 * conv_geo(h, w).tiles; }      // 4 waves per row-band workgroup
int ln_slots_pw(int h, int w) { return PW_WAVES * pw_tiles(h, w); }
int ln_slots_conv1(int h, int w) { return 4 * conv1_tiles(h, w); }
int ln_slots_gc(const Coupling::GcGroup& g, int waves) { return waves * g.tiles(); }
int ln_slots_grouped(const Coupling& c) {
    // a branch outside the k_gc groups runs as a k_pw tap-mode launch or as a k_conv<3> problem
    const int branch = std::max(ln_slots_conv3(c.hc, c.wc), ln_slots_pw(c.hc, c.wc));
    int fused = 0, ing = 0;
    for (const Coupling::GcGroup& g : c.gcg) {
        fused += ln_slots_gc(g);
        ing += (int)g.br.size();
    }
    fused += ((int)c.br.size() - ing) * branch;
    return std::max((int)c.br.size() * branch, fused);
}

// launch-independent part of a k_gc launch over group gg (lnst: GcShape::lnst)
GcShape gc_shape(const Coupling& c, const Coupling::GcGroup& gg, int lnst) {
    GcShape s;
    std::memset(&s, 0, sizeof(s));
    for (size_t k = 0; k < gg.br.size(); k++) s.br[k] = gg.gcb[k];
    s.nbr = (int)gg.br.size();
    s.H = c.hc;
    s.W = c.wc;
    s.in_cs = c.t1_cs;
    s.out_cs = c.t2_cs;
    s.TH = gg.TH;
    s.TW = gg.TW;
    s.tiles_x = gg.tiles_x;
    s.tiles_per_img = gg.tiles();
    s.ps = gg.ps;
    s.nbk = gg.nbk;
    s.tpp = gg.tpp;
    s.nw = gg.nw;
    s.pd = gg.pd;
    s.band_bytes = gg.band_bytes;
    s.lnst = lnst;
    return s;
}

// images per workgroup of the image-looping kernels (k_pw, k_gc): one round of `slots` workgroups
// over `units` (tile, problem, image) work items, at most 16 images each (the per-image LN table in LDS)
static int images_per_wg(int64_t units, int64_t slots, [[maybe_unused]] const char* diag_env) {
    int ipw = (int)std::min<int64_t>(16, std::max<int64_t>(1, (units + slots - 1) / slots));
#ifdef CNF_DIAG   // diagnostics: a fixed count, within what the kernels can run
    if (const char* e = std::getenv(diag_env)) ipw = std::min(16, std::max(1, std::atoi(e)));
#endif
    return ipw;
}

int pw_images_per_wg(int tiles, int nprob, int B, bool res) {
    return images_per_wg((int64_t)tiles * nprob * B, 512, res ? "CNF_PW_IPW_RES" : "CNF_PW_IPW");
}

// ----------------------------------------------------------------------------------------------
// launch recording
// ----------------------------------------------------------------------------------------------
void Exec::record(const std::string& name, double flops, double bytes, std::function<void(void*)> fn) {
    if (p.dry) {
        p.dry_launches.push_back(name);
        return;
    }
    const size_t k = p.recorded.size();
    const bool timed = p.timing && p.record && name.rfind("k_", 0) == 0;   // kernels only (not copies)
    if (timed) {
        while (p.ev.size() < 2 * (k + 1)) {
            hipEvent_t e;
            if (hipEventCreate(&e) != hipSuccess) throw std::runtime_error("hipEventCreate");
            p.ev.push_back(e);
        }
        launch_timing() = LaunchTiming{p.ev[2 * k], p.ev[2 * k + 1]};
    }
    try {
        fn(st);
    } catch (...) {
        launch_timing() = LaunchTiming{};
        throw;
    }
    // timed only when exactly one kernel wrote the pair (a launch helper may issue none)
    const bool wrote = timed && launch_timing().used == 1;
    launch_timing() = LaunchTiming{};
    if (p.record) p.recorded.push_back(Recorded{name, flops, bytes, std::move(fn), wrote});
}

// ----------------------------------------------------------------------------------------------
// conv problems
// ----------------------------------------------------------------------------------------------
// LN statistics slab of one tensor: per-wave partials [B][st_parts][LNP] of which the last producer
// wrote the first nparts (see ConvProb)
struct Slab {
    float* part = nullptr;
    int nparts = 0;
};

// channels [off, off + c) of an NHWC tensor with cs floats per pixel
template <class T>
struct Window {
    T* ptr = nullptr;
    int cs = 0, off = 0, c = 0;
};
using Src = Window<const float>;
using Dst = Window<float>;
// a whole dense tensor of c channels
static Src src(const float* p, int c) { return Src{p, c, 0, c}; }
static Dst dst(float* p, int c) { return Dst{p, c, 0, c}; }

struct LnLoad {   // LayerNorm on load from the input's partials (slab.part == null: none)
    Slab slab;
    const float* gamma = nullptr;
    const float* beta = nullptr;
};

struct Weights {   // packed image and bias in aux
    const float* w = nullptr;
    const float* b = nullptr;
    const void* x6 = nullptr;   // the conv's bf16x6 plane image for k_pw (PackedConv::x6): x6_C K steps of x6_nr
    int x6_C = 0, x6_nr = 0;    // column blocks; null: none
};

struct ProbSpec {
    ProbSpec(Src in_, LnLoad ln_, int act_, Weights wt_, Dst out_, Slab out_st_ = Slab{})
        : in(in_), ln(ln_), act(act_), wt(wt_), out(out_), out_st(out_st_) {}
    Src in;
    LnLoad ln;
    int act;                   // LeakyReLU on load
    Weights wt;
    Dst out;
    Slab out_st;               // .part == null: no output statistics
    const float* res = nullptr;
    int out_part_base = 0;     // first partial slot of this problem
    int dil = 1;
    uint64_t store_mask = ~0ull;   // output channels stored (the statistics cover all of them)
};

static const char* role_name(int r) {   // ROLE_* order
    static const char* const names[] = {"conv_in", "conv_a", "gc", "conv_b", "conv_out"};
    return names[r >= 0 && r < 4 ? r : 4];
}

// dry runs collect the distinct launch shapes of the shape-specialised kernels
template <class S>
static void note_shape(std::vector<S>& seen, const S& s) {
    for (const S& o : seen)
        if (std::memcmp(&o, &s, sizeof(S)) == 0) return;
    seen.push_back(s);
}

static uint32_t magic_for(int d, int64_t xmax) {
    // x / d == umulhi(x, ceil(2^32 / d)) exactly while x * d * d < 2^32 (error term x*e/2^32 < 1/d)
    if (d <= 1) return 0;
    if ((double)xmax * d * d >= 4294967296.0) throw std::invalid_argument("magic division out of range");
    return (uint32_t)((((uint64_t)1 << 32) + (uint64_t)d - 1) / (uint64_t)d);
}

// tap-mode source of a k_pw launch (streamed conv_in): the probs' `in` is the raw layer input u, the
// A operand the 3x3 im2col row over the mask-compressed half (K = 9 * dc), gathered in the kernel
struct TapSrc {
    int mask, W, D, dc, img;   // mask, full-res width / depth, channels per tap, floats per image of u
    int dil = 1, off = 0;      // mask < 0: plain NHWC source (D channels), taps from channel off, dilation
};

// what only k_pw can do: a 1x1 launch asking for any of it is refused when k_pw cannot run it
struct PwExtras {
    const TapSrc* tap = nullptr;
    const int* st_map = nullptr;            // stores through a channel map (device table)
    const int* in_map = nullptr;            // A-operand quads through a map
    float* out2[2] = {nullptr, nullptr};    // per problem: every output channel also to a plain [B][HW][cout] tensor
    bool any() const { return tap != nullptr || st_map != nullptr || in_map != nullptr; }
};

// the launch under preparation: argument block, accounting, dynamic LDS
struct ConvLaunch {
    ConvArgs a;
    double flops = 0, bytes = 0;
    size_t lds = 0;
};

static void conv_begin(ConvLaunch& cl, const Exec& E, int h, int w, const std::vector<ProbSpec>& probs) {
    if ((int)probs.size() > MAXPROB) throw std::invalid_argument("too many problems in one conv launch");
    ConvArgs& a = cl.a;
    std::memset(&a, 0, sizeof(a));
    a.H = h;
    a.W = w;
    a.nprob = (int)probs.size();
    a.B = E.B;
    for (size_t i = 0; i < probs.size(); i++) {
        const ProbSpec& s = probs[i];
        ConvProb& q = a.p[i];
        q.in = s.in.ptr;
        q.in_cs = s.in.cs;
        q.in_off = s.in.off;
        q.cin = s.in.c;
        q.in_part = s.ln.slab.part;
        q.in_nparts = s.ln.slab.nparts;
        q.gamma = s.ln.gamma;
        q.beta = s.ln.beta;
        q.act = s.act;
        q.wt = s.wt.w;
        q.bias = s.wt.b;
        q.out = s.out.ptr;
        q.out_cs = s.out.cs;
        q.out_off = s.out.off;
        q.cout = s.out.c;
        q.res = s.res;
        q.out_part = s.out_st.part;
        q.part_stride = E.L.st_parts;
        q.out_part_base = s.out_part_base;
        q.dil = s.dil;
        q.st_mask_lo = (uint32_t)(s.store_mask & 0xffffffffull);
        q.st_mask_hi = (uint32_t)(s.store_mask >> 32);
    }
}

// flops and algorithmic bytes of one ks x ks problem reading a_ch channels per pixel
static void conv_cost(ConvLaunch& cl, const ProbSpec& s, int ks, int a_ch) {
    const ConvArgs& a = cl.a;
    const double HWB = (double)a.H * a.W * a.B;
    const int K = ks * ks * s.in.c;
    cl.flops += 2.0 * HWB * K * s.out.c;
    // output bytes count only the stored channels (conv_a stores just the grouped branches' inputs)
    const uint64_t cmask = s.out.c >= 64 ? ~0ull : ((1ull << s.out.c) - 1);
    const double stored = (double)__builtin_popcountll(s.store_mask & cmask);
    cl.bytes += 4.0 * (HWB * a_ch + HWB * (stored + (s.res ? s.out.c : 0)) +
                       (s.ln.slab.part ? 2.0 * a.H * a.W * a_ch : 0.0) + (double)K * s.out.c + s.out.c);
}

// k_conv3: 3x3 (dilated) implicit GEMM over row bands; returns the LN-partial slots per image and problem
static int conv3_launch(Exec& E, int role, int h, int w, const std::vector<ProbSpec>& probs) {
    if (probs.empty()) return 0;
    ConvLaunch cl;
    conv_begin(cl, E, h, w, probs);
    ConvArgs& a = cl.a;
    const Geo g = conv_geo(h, w);
    a.TH = g.TH;
    a.tiles_per_img = g.tiles;
    for (size_t i = 0; i < probs.size(); i++) {
        const ProbSpec& s = probs[i];
        ConvProb& q = a.p[i];
        if (s.out.c > 64) throw std::invalid_argument("conv with more than 64 output channels");
        const int K = 9 * s.in.c;
        q.nr = (s.out.c + 15) / 16;
        q.S = lds_stride(s.in.c);
        q.Kpad = (K + 3) / 4 * 4;
        q.NS = 16 * q.nr;
        if (q.NS % 32 == 0) q.NS += 16;
        const int WP = w + 2 * s.dil;
        const int SR = g.TH + 2 * s.dil;
        const int64_t total = (int64_t)SR * WP * s.in.c;
        q.cin_mag = magic_for(s.in.c, total + 256 * 4);
        q.wp_mag = magic_for(WP, (int64_t)SR * WP + 256 * 4);
        if (WP == 1) throw std::invalid_argument("degenerate width");
        size_t off = 128;
        q.lds_in_off = (int)off;
        off = align_up(off + (size_t)SR * WP * q.S * 4, 16);
        q.lds_w_off = (int)off;
        off = align_up(off + (size_t)q.Kpad * q.NS * 4, 16);
        q.lds_k_off = (int)off;
        off = align_up(off + (size_t)q.Kpad * 4, 16);
        cl.lds = std::max(cl.lds, off);
        conv_cost(cl, s, 3, s.in.c);
    }
    if (cl.lds > 160 * 1024) throw std::invalid_argument("conv tile exceeds the 160 KiB LDS budget");
    const int grid_x = E.B * g.tiles, ilds = (int)cl.lds, mr = g.MR;
    const std::string name = std::string("k_conv3<") + std::to_string(mr) + "," + role_name(role) + ">";
    E.record(name, cl.flops, cl.bytes, [mr, role, a, grid_x, ilds](void* st) {
        launch_conv(3, mr, role, a, grid_x, ilds, (hipStream_t)st);
    });
    return ln_slots_conv3(h, w);
}

// k_pw: 64-pixel tiles (4 waves x 16 pixels), each workgroup looping over ipw images, sized so the
// launch is one round of two workgroups per CU (see cnf_stream.hip)
static int pw_launch(Exec& E, int role, ConvLaunch& cl, const std::vector<ProbSpec>& probs, int nr, int gm,
                     const PwExtras& x) {
    ConvArgs& a = cl.a;
    for (int i = 0; i < a.nprob; i++) {
        const ProbSpec& s = probs[i];
        ConvProb& q = a.p[i];
        if (x.in_map != nullptr && (x.tap != nullptr || s.in.off != 0 || s.in.c % 4 != 0))
            throw std::logic_error("mapped input: plain k_pw over whole quads only");
        if (x.st_map != nullptr && (s.res != nullptr || s.out.c > 64))
            throw std::logic_error("mapped stores: no residual, <= 64 outputs");
        q.st_compact = x.st_map != nullptr ? 1 : 0;
        q.st_map = x.st_map;
        q.in_mapped = x.in_map != nullptr ? 1 : 0;
        q.in_map = x.in_map;
        if (i < 2) q.out2 = x.out2[i];
        // staging: a copy of the plan's plane image, or (debug option PRESPLIT=0) the split of the fp32 image
        if (opts().presplit != 0) {
            if (s.wt.x6 == nullptr || s.wt.x6_C != (s.in.c + 31) / 32 || s.wt.x6_nr != nr)
                throw std::logic_error("k_pw launch: no plane image of this conv's K steps and column blocks in aux");
            q.wx6 = s.wt.x6;
        }
    }
    const bool lnf = probs[0].ln.slab.part != nullptr, resf = probs[0].res != nullptr, tapf = x.tap != nullptr;
    const int tiles = pw_tiles(a.H, a.W);
    a.tiles_per_img = tiles;
    a.ipw = pw_images_per_wg(tiles, a.nprob, E.B, resf);
    const int grid_x = tiles * ((E.B + a.ipw - 1) / a.ipw), ilds = (int)cl.lds;
    if (x.tap) {
        a.umask = x.tap->mask;
        a.uW = x.tap->W;
        a.uD = x.tap->D;
        a.udc = x.tap->dc;
        a.uimg = x.tap->img;
        a.udil = x.tap->dil;
        a.uoff = x.tap->off;
    }
    PwShape sh;
    if (E.p.dry && pw_shape_of(nr, gm, lnf, resf, tapf, a, sh)) note_shape(E.p.pw_shapes, sh);
    const std::string name =
        std::string("k_pw<") + std::to_string(nr) + "," + std::to_string(gm) + "," + role_name(role) + ">";
    E.record(name, cl.flops, cl.bytes, [nr, gm, lnf, resf, tapf, a, grid_x, ilds](void* st) {
        launch_pw(nr, gm, lnf, resf, tapf, a, grid_x, ilds, (hipStream_t)st);
    });
    return ln_slots_pw(a.H, a.W);
}

// k_conv1: the per-tile 1x1 kernel (runs of P pixels inside one image)
static int conv1_launch(Exec& E, int role, ConvLaunch& cl) {
    ConvArgs& a = cl.a;
    const int grid_x = E.B * a.tiles_per_img, ilds = (int)cl.lds, mr = conv1_mr(a.H, a.W);
    const std::string name = std::string("k_conv1<") + std::to_string(mr) + ",vec," + role_name(role) + ">";
    E.record(name, cl.flops, cl.bytes, [mr, role, a, grid_x, ilds](void* st) {
        launch_conv1(mr, true, role, a, grid_x, ilds, (hipStream_t)st);
    });
    return ln_slots_conv1(a.H, a.W);
}

struct Launched1x1 {
    int slots;   // LN-partial slots per image each problem wrote
    bool pw;     // ran as k_pw (out2 stored)
};

// a 1x1 conv launch: k_pw when it can run the problems, else k_conv1 (which knows none of PwExtras)
static Launched1x1 conv1x1_launch(Exec& E, int role, int h, int w, const std::vector<ProbSpec>& probs,
                                  const PwExtras& x = PwExtras{}) {
    if (probs.empty()) return {0, false};
    ConvLaunch cl;
    conv_begin(cl, E, h, w, probs);
    ConvArgs& a = cl.a;
    a.P = 64 * conv1_mr(h, w);   // (k_pw has its own tiles and ignores P)
    a.tiles_per_img = conv1_tiles(h, w);
    int pw_nr = 0, pw_gm = 0;
    for (size_t i = 0; i < probs.size(); i++) {
        const ProbSpec& s = probs[i];
        ConvProb& q = a.p[i];
        if (s.out.c > 64) throw std::invalid_argument("conv with more than 64 output channels");
        q.nr = (s.out.c + 15) / 16;
        const int G = (s.in.c + 15) / 16;
        size_t off = 512;   // k_pw keeps its per-image LN table at bytes [256, 384)
        q.lds_w_off = (int)off;
        // k_pw stages the weights as the three bf16 planes of 32-deep K steps (1 KiB per plane, step and
        // 16-column block); k_conv1 reads the fp32 image, G x 16 x 16 x nr floats, which fits in it
        const size_t wx6 = (size_t)((s.in.c + 31) / 32) * 3 * q.nr * 1024;
        off = align_up(off + std::max(wx6, (size_t)G * 16 * 16 * q.nr * 4), 16);
        // k_pw loads every channel quad the input window starts with 16 bytes at a time: a window
        // that is not quad-aligned (conv_b over the 62- / 30-channel concat of cfg5's grouped
        // stages) reads past its last channel into the next pixel (or 0 past the image), which
        // meets zero weight rows (the packed image pads K with zeros)
        pw_nr = std::max(pw_nr, q.nr);
        pw_gm = std::max(pw_gm, G);
        cl.lds = std::max(cl.lds, off);
        conv_cost(cl, s, 1, x.tap ? x.tap->dc : s.in.c);
    }
    if (cl.lds > 160 * 1024) throw std::invalid_argument("conv tile exceeds the 160 KiB LDS budget");
    // k_pw stages every problem's weights as pw_nr column blocks: the workgroup's LDS covers them
    for (int i = 0; i < a.nprob; i++)
        if ((size_t)a.p[i].lds_w_off + (size_t)((a.p[i].cin + 31) / 32) * 3 * pw_nr * 1024 > cl.lds || a.p[i].nr != pw_nr)
            throw std::logic_error("k_pw launch: problems of different widths or LDS short of the weight planes");
    pw_gm = pw_gm <= 1 ? 1 : pw_gm <= 2 ? 2 : pw_gm <= 4 ? 4 : pw_gm <= 8 ? 8 : 0;
    bool ln_uniform = true;
    bool fits32 = true;   // k_pw addresses one image per buffer resource with 32-bit byte offsets
    for (const ProbSpec& s : probs) {
        ln_uniform = ln_uniform && ((s.ln.slab.part != nullptr) == (probs[0].ln.slab.part != nullptr)) &&
                     ((s.res != nullptr) == (probs[0].res != nullptr));
        fits32 = fits32 && (double)h * w * std::max(s.in.cs, s.out.cs) * 4.0 < 2147483648.0 &&
                 (x.tap == nullptr || (double)x.tap->img * 4.0 < 2147483648.0);
    }
    const bool pw_ok = pw_gm > 0 && ln_uniform && fits32 && E.p.use_pw;
    if (x.any() && !pw_ok) throw std::logic_error("mapped loads / stores need the k_pw path");
    if (pw_ok) return {pw_launch(E, role, cl, probs, pw_nr, pw_gm, x), true};
    return {conv1_launch(E, role, cl), false};
}

// tap-decomposed 3x3 (dilation 1, cout <= 7): see k_convtap
static void convtap_launch(Exec& E, int h, int w, const std::vector<ProbSpec>& probs) {
    ConvLaunch cl;
    conv_begin(cl, E, h, w, probs);
    ConvArgs& a = cl.a;
    const Geo g = conv_geo(h, w);
    a.TH = g.TH;
    a.tiles_per_img = g.tiles;
    const int nband = (g.TH + 2) * w;
    int mt = (nband + 63) / 64;
    if (mt == 5) mt = 6;
    if (mt > 6) throw std::invalid_argument("tap conv band too large");
    const double HWB = (double)h * w * E.B;
    bool vec = true;
    for (size_t i = 0; i < probs.size(); i++) {
        const ProbSpec& s = probs[i];
        ConvProb& q = a.p[i];
        if (9 * s.out.c > 64) throw std::invalid_argument("tap conv needs 9*cout <= 64");
        q.nr = (9 * s.out.c + 15) / 16;
        const int NSJ = 16 * q.nr;
        const int G = (s.in.c + 15) / 16;
        size_t off = 128;
        q.lds_w_off = (int)off;
        off = align_up(off + (size_t)G * 16 * NSJ * 4, 16);
        q.lds_in_off = (int)off;
        off = align_up(off + (size_t)nband * (NSJ + 1) * 4, 16);
        q.lds_k_off = (int)off;
        off = align_up(off + (size_t)NSJ * 4, 16);
        cl.lds = std::max(cl.lds, off);
        if (s.in.c % 4 || s.in.cs % 4 || s.in.off % 4) vec = false;
        cl.flops += 2.0 * HWB * 9 * s.in.c * s.out.c;
        cl.bytes += 4.0 * (HWB * s.in.c + HWB * s.out.c + (s.ln.slab.part ? 2.0 * h * w * s.in.c : 0.0) +
                           9.0 * s.in.c * s.out.c);
    }
    if (cl.lds > 160 * 1024) throw std::invalid_argument("tap conv exceeds the LDS budget");
    const int ilds = (int)cl.lds, grid_x = E.B * g.tiles;
    const std::string name = std::string("k_convtap<") + std::to_string(mt) + (vec ? ",vec" : ",scalar") + ",conv_out>";
    E.record(name, cl.flops, cl.bytes, [mt, vec, a, grid_x, ilds](void* st) {
        launch_convtap(mt, vec, a, grid_x, ilds, (hipStream_t)st);
    });
}

// ----------------------------------------------------------------------------------------------
// k_net_lds
// ----------------------------------------------------------------------------------------------
// k_net_lds geometry for coupling c; returns the LDS bytes (0 if the layer cannot use it)
size_t netlds_setup(const Plan& p, const Coupling& c, NetLdsArgs& a) {
    std::memset(&a, 0, sizeof(a));
    if ((int)c.br.size() > NETLDS_MAXBR) return 0;
    for (const Branch& b : c.br)
        if (b.dil > 16) return 0;
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
    for (int i = 0; i < a.nbr; i++) {
        a.br_cin_off[i] = c.br[i].cin_off;
        a.br_cin[i] = c.br[i].cin;
        a.br_cout[i] = c.br[i].cout;
        a.br_out_off[i] = c.br[i].out_off;
        a.br_dil[i] = c.br[i].dil;
    }
    {   // disjoint union of the grouped branches' input channel windows (normalised once, in place)
        std::vector<std::pair<int, int>> iv;
        for (const Branch& b : c.br) iv.push_back({b.cin_off, b.cin_off + b.cin});
        std::sort(iv.begin(), iv.end());
        std::vector<std::pair<int, int>> mg;
        for (auto& x : iv) {
            if (!mg.empty() && x.first <= mg.back().second)
                mg.back().second = std::max(mg.back().second, x.second);
            else
                mg.push_back(x);
        }
        if ((int)mg.size() > NETLDS_MAXBR) return 0;
        a.nwin = (int)mg.size();
        for (int i = 0; i < a.nwin; i++) {
            a.win_off[i] = mg[i].first;
            a.win_len[i] = mg[i].second - mg[i].first;
        }
    }
    a.offs_per_net = c.lds_offs_per_net;
    const NetLdsGeom& g = c.lds;
    a.sy = g.sy;
    a.s1 = g.s1;
    a.s2 = g.s2;
    a.su = g.su;
    const NetParams& n0 = c.net[0];
    auto desc = [](const PackedConv& pc) { return LdsConv{pc.fmt, (int)pc.size, pc.kpad, pc.ns}; };
    a.ci = desc(n0.ci);
    a.co = desc(n0.co);
    if (!n0.rb.empty()) {
        a.ca = desc(n0.rb[0].ca);
        a.cb = desc(n0.rb[0].cb);
        for (int i = 0; i < a.nbr; i++) a.gcv[i] = desc(n0.rb[0].gc[i]);
    }
    a.off_y = g.off_y;
    a.off_t1 = g.off_t1;
    a.off_t2 = g.off_t2;
    a.off_w = g.off_w;
    a.off_k = g.off_k;
    a.off_ks = g.off_ks;
    auto nr = [](int cout) { return (cout + 15) / 16; };
    // the tap-decomposed conv_out runs in chunks of at most two 16-column blocks
    a.maxnr = std::max(nr(c.nk), c.co_fmt == PK_TAP ? std::min(2, nr(9 * c.dc2)) : nr(c.dc2));
    for (const Branch& b : c.br) a.maxnr = std::max(a.maxnr, nr(b.cout));
#ifdef CNF_DIAG
    if (const char* e = std::getenv("CNF_NETLDS_DUMP")) {   // diagnostics: every shape field, as C
        if (std::atoi(e)) {
            const int* w = reinterpret_cast<const int*>(&a.offs_per_net);
            const int n = (int)((reinterpret_cast<const char*>(&a.zero_bias) - reinterpret_cast<const char*>(w)) / 4);
            std::fprintf(stderr, "NETSHAPE hc=%d wc=%d mask=%d:", c.hc, c.wc, c.mask);
            for (int i = 0; i < n; i++) std::fprintf(stderr, " %d", w[i]);
            const int* w2 = reinterpret_cast<const int*>(&a.off_y);
            for (int i = 0; i < 7; i++) std::fprintf(stderr, " %d", w2[i]);
            std::fprintf(stderr, "\n");
        }
    }
    if (const char* e = std::getenv("CNF_NETLDS_VERBOSE"))
        if (std::atoi(e)) std::fprintf(stderr, "netlds layer hc=%d wc=%d nk=%d dc2=%d co_fmt=%d maxnr=%d\n", c.hc, c.wc,
                                       c.nk, c.dc2, c.co_fmt, a.maxnr);
#endif
    return (size_t)g.bytes;
}

static double net_flops(const Coupling& c) {
    const double HW = (double)c.hc * c.wc;
    double f = 9.0 * c.dc1 * c.nk + 9.0 * c.nk * c.dc2;
    double rb = (double)c.nk * c.nk + (double)c.gc * c.nk;
    for (const Branch& b : c.br) rb += 9.0 * b.cin * b.cout;
    return 2.0 * HW * (f + c.R * rb);
}

// The coupling law of layer c, whoever applies it: u -> v from the raw conv_out of net A (pre-tanh) /
// net b in so[0] / so[1]. k_coupling takes it as is (plus a tap-GEMM conv_out to finish), a deferred
// law is handed on as a CoupPend.
static CoupArgs law_of(const Exec& E, const Coupling& c, const float* u, float* v, float* const* so, double* ld_part,
                       int dir) {
    CoupArgs a;
    a.u = u;
    a.v = v;
    a.s_pre = so[0];
    a.t = so[1];
    a.tanh_w = E.params + c.net[0].tanh_w;
    a.ld_part = ld_part;
    a.H = c.H;
    a.W = c.W;
    a.D = c.D;
    a.mask = c.mask;
    a.mask_c = c.mask_c;
    a.hc = c.hc;
    a.wc = c.wc;
    a.dc1 = c.dc1;
    a.dc2 = c.dc2;
    a.dir = dir;
    for (int n = 0; n < 2; n++) {
        a.tc[n] = a.tbias[n] = nullptr;
        a.so_w[n] = so[n];
    }
    return a;
}

// the whole s,t net in one k_net_lds launch (which also applies the previous layer's deferred law)
static void netlds_layer(Exec& E, const Coupling& c, const CoupArgs& w, const CouplingOpts& o) {
    const int B = E.B;
    NetLdsArgs na;
    const size_t nlds = netlds_setup(E.p, c, na);
    if (nlds == 0) throw std::runtime_error("layer planned for k_net_lds does not fit its LDS budget");
    na.u = w.u;
    na.so[0] = w.so_w[0];
    na.so[1] = w.so_w[1];
    na.params = E.params;
    na.aux = E.aux;
    na.offs = E.p.dtab(c.dev_lds_offs);
    for (int n = 0; n < 2; n++) na.ci_off[n] = E.p.host_table[(size_t)c.dev_lds_offs + (size_t)n * na.offs_per_net];
    na.zero_bias = E.aux + E.p.aux_zero;
    if (o.save != nullptr) {
        const LdsSave s = LdsSave::of(c.hc * c.wc, c.nk, c.gc, c.R);
        na.save = o.save;
        na.save_img = s.img;
        na.save_t1 = s.t1;
        na.save_t2 = s.t2;
        na.save_st = s.st;
    }
    if (o.nz != nullptr) {
        if (o.pend != nullptr || o.save != nullptr) throw std::logic_error("fused input noise: first inference layer only");
        na.nz = *o.nz;
    }
    if (const CoupPend* pend = o.pend) {
        // buffer discipline of the deferred law (dry runs carry no real pointers): this layer's
        // input is the pending layer's output v_k, which must not be the u_k it is computed
        // from, and this layer's s/t outputs must not overwrite the pending s_pre / t it reads
        // (LDS layers alternate s/t sets by coupling index)
        if (!E.p.dry && (pend->v != w.u || pend->u == w.u || w.s_pre == pend->s_pre || w.s_pre == pend->t ||
                         w.t == pend->s_pre || w.t == pend->t))
            throw std::logic_error("deferred coupling: buffer aliasing (v_k / u_k / s,t sets)");
        na.pend = *pend;
        na.pend.comp = pend->mask_c == c.mask && pend->hc == c.hc && pend->wc == c.wc && pend->dc2 == c.dc1 ? 1 : 0;
    }
    const double fl = 2.0 * B * net_flops(c);
    // algorithmic bytes: u1c in and s/t out per image and net, plus the per-element LN
    // gamma/beta (only the branch input windows of LN2) and the conv weights once per launch
    const double HWc = (double)c.hc * c.wc;
    int win = 0;
    for (int i = 0; i < na.nwin; i++) win += na.win_len[i];
    const double ln_floats = E.p.desc.layer_norm != 0 ? 2.0 * HWc * (c.R * (c.nk + win + c.gc) + c.nk) : 0.0;
    const double w_floats = net_flops(c) / (2.0 * HWc);
    const double by = 4.0 * (B * HWc * (c.dc1 + c.dc2) * 2 + 2 * (ln_floats + w_floats));
    E.record("k_net_lds", fl, by, [na, B, ilds = (int)nlds](void* st) { launch_net_lds(na, B, ilds, (hipStream_t)st); });
}

// ----------------------------------------------------------------------------------------------
// the streamed layer
// ----------------------------------------------------------------------------------------------
// Training forward with saved activations (TrainLayout::StreamSave; ss == null: inference, every call
// a no-op): y_r and t2_r live in per-block slices of the save area (conv_b writes y_{r+1} next to its
// residual y_r instead of in place), conv_a also stores the full t1_r, and every LN tensor's statistics
// are folded once into [B][2] by one k_ln_final per residual block (flush before conv_b overwrites slab
// 0, and at the end): the three slabs hold y_r, t1_r and t2_r until then
struct TrainSave {
    Exec& E;
    const Coupling& c;
    const TrainLayout::StreamSave* ss;
    bool ln;
    LnFinalSet pend{};
    const LnIndex idx{c.R};
    const StreamActs acts = ss != nullptr ? StreamActs::saved(E.ws, *ss, E.B, c) : StreamActs{};

    bool on() const { return ss != nullptr; }

    void flush() {
        if (pend.count == 0) return;
        const LnFinalSet fs = pend;
        const int B = E.B;
        double bytes = 0.0;
        for (int q = 0; q < fs.count; q++) bytes += 16.0 * B * fs.nparts[q] * 2;
        E.record("k_ln_final", 0, bytes, [=](void* st) { launch_ln_final(fs, B, (hipStream_t)st); });
        pend.count = 0;
    }
    // the statistics of LN tensor i (an LnIndex number) from the slots of its slab
    void stats(const Slab (&sl)[2], int i) {
        if (!on() || !ln) return;
        if (pend.count == LNF_MAX) flush();
        const int q = pend.count++;
        for (int n = 0; n < 2; n++) {
            pend.part[q][n] = sl[n].part;
            pend.st[q][n] = acts.stats(n, i);
        }
        pend.nparts[q] = sl[0].nparts;
    }
};

// slabs of the three LN tensors
enum { SL_Y = 0, SL_T1 = 1, SL_T2 = 2 };

struct Streamed {
    Exec& E;
    const Coupling& c;
    const bool ln;
    const float* const P;   // canonical parameters
    const float* const X;   // aux image
    CoupArgs& law;   // so_w: where conv_out goes; tc / tbias: a tap-GEMM conv_out left to k_coupling
    float *y[2], *t1[2], *t2[2];
    Slab sl[3][2];   // [y, t1, t2][net]: a producing launch reports the slots it wrote per image (set_parts)
    TrainSave sv;
    int base = 0;    // grouped stage: first free LN3 slot (each launch's slots follow the previous ones')

    Streamed(Exec& E_, const Coupling& c_, CoupArgs& law_, const TrainLayout::StreamSave* ss)
        : E(E_), c(c_), ln(E_.p.desc.layer_norm != 0), P(E_.params), X(E_.aux), law(law_), sv{E_, c_, ss, ln} {
        const WsLayout& L = E.L;
        if (ss != nullptr && c.t2_mapped) throw std::logic_error("training save: mapped t2 layout");
        for (int n = 0; n < 2; n++) {
            y[n] = sv.on() ? sv.acts.y(n, 0) : E.at<float>(L.y[n]);
            t1[n] = E.at<float>(L.t1[n]);
            t2[n] = sv.on() ? sv.acts.t2(n, 0) : E.at<float>(L.t2[n]);
            for (int k = 0; k < 3; k++) sl[k][n].part = E.at<float>(L.st_part[n][k]);
        }
        sv.pend.part_stride = L.st_parts;
    }

    Slab slab(int k, int n) const { return ln ? sl[k][n] : Slab{}; }
    LnLoad ln_load(int k, int n, const float* gamma, const float* beta) const {
        return ln ? LnLoad{sl[k][n], gamma, beta} : LnLoad{};
    }
    Weights packed(const PackedConv& pc) const {
        const bool pw6 = pc.x6 >= 0 && pc.fmt != PK_Q4;   // (a PK_Q4 branch's planes are k_gc's)
        return Weights{X + pc.w, X + pc.b, pw6 ? X + pc.x6 : nullptr, pw6 ? pc.x6_C : 0, pw6 ? pc.nr : 0};
    }

    // more slots than a consumer wave fetches in its prologue (64 x LN_FETCH = 512: the 128x128 layers):
    // merged once per image by k_ln_merge instead of by every consumer workgroup for each of its images
    // (the 64x64 layers' slots are folded by the consumers: 70 fewer launches per cfg4 step)
    void set_parts(int k, int nparts) {
#ifdef CNF_DIAG_NO_LN_MERGE   // (diagnostic builds: the consumers fold every slot)
        constexpr int ln_merge_over = 1 << 30;
#else
        constexpr int ln_merge_over = 64 * LN_FETCH;
#endif
        if (ln && nparts > ln_merge_over) {
            float *p0 = sl[k][0].part, *p1 = sl[k][1].part;
            const int np = nparts, ps = E.L.st_parts, B = E.B;
            E.record("k_ln_merge", 0, 16.0 * B * np * 2 + 32.0 * B,
                     [=](void* st) { launch_ln_merge(p0, p1, np, ps, B, (hipStream_t)st); });
            nparts = 1;
        }
        for (int n = 0; n < 2; n++) sl[k][n].nparts = nparts;
    }

    // conv_in (:1114-1119 / :1159-1164): u1c -> y, both nets in one launch; straight from u (k_pw tap
    // mode: the mask gather inside the im2col loads) when packed for it
    void conv_in(const float* u) {
        const bool tap = E.p.use_pw && c.net[0].ci_pw.size > 0;
        float* u1c = E.at<float>(E.L.u1c);
        std::vector<ProbSpec> pr;
        for (int n = 0; n < 2; n++) {
            const NetParams& np = c.net[n];
            pr.push_back(ProbSpec(tap ? src(u, 9 * c.dc1) : src(u1c, c.dc1), LnLoad{}, 0,
                                  packed(tap ? np.ci_pw : np.ci), dst(y[n], c.nk), slab(SL_Y, n)));
        }
        if (tap) {
            const TapSrc ts{c.mask, c.W, c.D, c.dc1, c.H * c.W * c.D};
            PwExtras x;
            x.tap = &ts;
            set_parts(SL_Y, conv1x1_launch(E, ROLE_CONV_IN, c.hc, c.wc, pr, x).slots);
        } else {
            const int B = E.B, H = c.H, W = c.W, D = c.D, mask = c.mask, hc = c.hc, wc = c.wc, dc1 = c.dc1;
            E.record("k_gather_u1c", 0, 4.0 * B * hc * wc * dc1 * 2, [=](void* st) {
                launch_gather_u1c(u, u1c, B, H, W, D, mask, hc, wc, dc1, (hipStream_t)st);
            });
            set_parts(SL_Y, conv3_launch(E, ROLE_CONV_IN, c.hc, c.wc, pr));
        }
        sv.stats(sl[SL_Y], sv.idx.ln1(0));
    }

    // conv_a: LN1(LReLU(y)) -> 1x1 -> t1. Only the channels the branches read are stored (into their
    // consumers' sub-tensors when t1_compact); the LN2 statistics still cover all nk channels
    void conv_a(int r) {
        std::vector<ProbSpec> pr;
        PwExtras x;
        x.st_map = c.t1_compact ? E.p.dtab(c.dev_t1_map) : nullptr;
        for (int n = 0; n < 2; n++) {
            const RBParams& rb = c.net[n].rb[r];
            pr.push_back(ProbSpec(src(y[n], c.nk), ln_load(SL_Y, n, P + rb.ln1g, P + rb.ln1b), 1, packed(rb.ca),
                                  Dst{t1[n], c.t1_cs, 0, c.nk}, slab(SL_T1, n)));
            pr.back().store_mask = c.t1_used;
            // training: the full t1_r for the backward's LN2 from the same launch (k_pw's second
            // store; its dual-store instantiations exist for LN on only)
            if (sv.on() && ln) x.out2[n] = sv.acts.t1(n, r);
        }
        const Launched1x1 l = conv1x1_launch(E, ROLE_CONV_A, c.hc, c.wc, pr, x);
        set_parts(SL_T1, l.slots);
        if (!sv.on()) return;
        if (!(l.pw && ln)) {
            // no second store: the full t1_r by a launch of its own (the t1 above holds only the branch windows)
            for (int n = 0; n < 2; n++) {
                pr[n].out = dst(sv.acts.t1(n, r), c.nk);
                pr[n].out_st = Slab{};
                pr[n].store_mask = ~0ull;
            }
            conv1x1_launch(E, ROLE_CONV_A, c.hc, c.wc, pr);
        }
        sv.stats(sl[SL_T1], sv.idx.ln2(r));
    }

    // LN2 gamma/beta in t1's layout: the aux copies gathered to the compact layout, or the parameters
    LnLoad ln2(int n, const RBParams& rb) const {
        return c.t1_compact ? ln_load(SL_T1, n, X + rb.ln2c_g, X + rb.ln2c_b) : ln_load(SL_T1, n, P + rb.ln2g, P + rb.ln2b);
    }

    // one k_gc launch per planned group of branches
    void gc_groups(int r, std::vector<char>& done) {
        const int B = E.B;
        for (const Coupling::GcGroup& gg : c.gcg) {
            const int ng = (int)gg.br.size();
            GcArgs ga;
            std::memset(&ga, 0, sizeof(ga));
            for (int n = 0; n < 2; n++) {
                const RBParams& rb = c.net[n].rb[r];
                const LnLoad l2 = ln2(n, rb);
                ga.in[n] = t1[n];
                ga.out[n] = t2[n];
                ga.in_part[n] = l2.slab.part;
                ga.out_part[n] = ln ? sl[SL_T2][n].part + (size_t)base * LNP : nullptr;   // after earlier launches' slots
                ga.gamma[n] = l2.gamma;
                ga.beta[n] = l2.beta;
                for (int k = 0; k < ng; k++) {
                    ga.w[n][k] = X + rb.gc[gg.br[k]].w;
                    ga.b[n][k] = X + rb.gc[gg.br[k]].b;
                    if (opts().presplit != 0) {
                        if (rb.gc[gg.br[k]].x6 < 0) throw std::logic_error("k_gc launch: branch without a plane image in aux");
                        ga.w6[n][k] = X + rb.gc[gg.br[k]].x6;
                    }
                }
            }
            for (int bi : gg.br) done[bi] = 1;
            ga.s = gc_shape(c, gg, (ga.in_part[0] ? 1 : 0) | (ga.out_part[0] ? 2 : 0));
            ga.B = B;
            ga.in_nparts = sl[SL_T1][0].nparts;
            ga.part_stride = E.L.st_parts;
            // images per workgroup: one workgroup per CU (16 / nw of them), looping over its images
            // with the next image's band staged behind the current one's MFMAs
            ga.ipw = images_per_wg((int64_t)gg.tiles() * 2 * B, 256LL * gc_wg_per_cu(gg.nw), "CNF_GC_IPW");
            const int slots = ln_slots_gc(gg, gc_waves(ga));   // one slot per k_gc wave
            if (base + slots > E.L.st_parts) throw std::runtime_error("k_gc: LN partial slab too small");
            const int grid_x = gg.tiles() * ((B + ga.ipw - 1) / ga.ipw);
            double fl = 0, by = 0;
            int win = 0;
            for (int k = 0; k < ng; k++) {
                const Branch& b = c.br[gg.br[k]];
                fl += 2.0 * B * c.hc * c.wc * 9.0 * b.cin * b.cout * 2;
                win += b.cin;
                by += 4.0 * B * c.hc * c.wc * b.cout * 2;
            }
            by += 4.0 * B * c.hc * c.wc * win * 2 + (ln ? 4.0 * 2 * c.hc * c.wc * win * 2 : 0.0);
            if (E.p.dry) note_shape(E.p.gc_launch, ga.s);
            E.record("k_gc", fl, by, [ga, grid_x, ilds = gg.lds](void* st) { launch_gc(ga, grid_x, ilds, (hipStream_t)st); });
            base += slots;
        }
    }

    // every branch packed for it as a k_pw tap-mode launch over its im2col row (9 cin <= 128)
    void tap_branches(int r, std::vector<char>& done) {
        for (int bi = 0; bi < (int)c.br.size(); bi++) {
            const Branch& b = c.br[bi];
            if (done[bi] || !(E.p.use_pw && c.net[0].rb[r].gpw[bi].size > 0)) continue;
            std::vector<ProbSpec> pt;
            for (int n = 0; n < 2; n++) {
                const RBParams& rb = c.net[n].rb[r];
                pt.push_back(ProbSpec(src(t1[n], 9 * b.cin), ln2(n, rb), 1, packed(rb.gpw[bi]),
                                      Dst{t2[n], c.t2_cs, b.out_off, b.cout}, slab(SL_T2, n)));
                pt.back().out_part_base = base;
            }
            TapSrc ts{-1, c.wc, c.t1_pcs[bi], b.cin, c.hc * c.wc * c.t1_cs};
            ts.dil = b.dil;
            ts.off = c.t1_off[bi];
            PwExtras x;
            x.tap = &ts;
            x.st_map = c.t2_mapped ? E.p.dtab(c.dev_t2_bmap[bi]) : nullptr;
            base += conv1x1_launch(E, ROLE_GC, c.hc, c.wc, pt, x).slots;
            done[bi] = 1;
        }
    }

    // the rest as one k_conv<3> launch, a problem per (net, branch)
    void conv3_branches(int r, const std::vector<char>& done) {
        const int per = ln_slots_conv3(c.hc, c.wc);
        std::vector<ProbSpec> pr;
        int nrest = 0;
        for (int n = 0; n < 2; n++) {
            const RBParams& rb = c.net[n].rb[r];
            int k = 0;
            for (int bi = 0; bi < (int)c.br.size(); bi++) {
                const Branch& b = c.br[bi];
                if (done[bi]) continue;
                if (c.t1_compact || c.t2_mapped) throw std::logic_error("k_conv<3> branch on a mapped t1 / t2 layout");
                pr.push_back(ProbSpec(Src{t1[n], c.nk, b.cin_off, b.cin}, ln2(n, rb), 1, packed(rb.gc[bi]),
                                      Dst{t2[n], c.gc, b.out_off, b.cout}, slab(SL_T2, n)));
                pr.back().out_part_base = base + k * per;
                pr.back().dil = b.dil;
                k++;
            }
            nrest = k;
        }
        base += nrest * conv3_launch(E, ROLE_GC, c.hc, c.wc, pr);
    }

    // grouped dilated branches: LN2(LReLU(t1)) -> 3x3 dil d -> t2[:, out_off:out_off+cout]
    void grouped(int r) {
        base = 0;
        std::vector<char> done(c.br.size(), 0);
        gc_groups(r, done);
        tap_branches(r, done);
        conv3_branches(r, done);
        if (base > E.L.st_parts) throw std::runtime_error("grouped branches: LN partial slab too small");
        set_parts(SL_T2, base);
        sv.stats(sl[SL_T2], sv.idx.ln3(r));
    }

    // conv_b: LN3(LReLU(t2)) -> 1x1 -> + shortcut -> y (in place; training: the next save slice)
    void conv_b(int r) {
        sv.flush();   // (conv_b writes slab 0's slots: y_r's statistics first)
        std::vector<ProbSpec> pr;
        for (int n = 0; n < 2; n++) {
            const RBParams& rb = c.net[n].rb[r];
            const LnLoad l3 = c.t2_mapped ? ln_load(SL_T2, n, X + rb.ln3c_g, X + rb.ln3c_b)
                                          : ln_load(SL_T2, n, P + rb.ln3g, P + rb.ln3b);
            pr.push_back(ProbSpec(Src{t2[n], c.t2_cs, 0, c.gc}, l3, 1, packed(rb.cb),
                                  dst(sv.on() ? sv.acts.y(n, r + 1) : y[n], c.nk), slab(SL_Y, n)));
            pr.back().res = y[n];
        }
        PwExtras x;
        x.in_map = c.t2_mapped ? E.p.dtab(c.dev_t2_qmap) : nullptr;
        set_parts(SL_Y, conv1x1_launch(E, ROLE_CONV_B, c.hc, c.wc, pr, x).slots);
        for (int n = 0; n < 2; n++) y[n] = pr[n].out.ptr;
        sv.stats(sl[SL_Y], sv.idx.ln1(r + 1));   // (ln_out() after the last block)
    }

    // conv_out: LN_out(LReLU(y)) -> 3x3 -> so (raw A pre-tanh / b); > 64 outputs in 64-channel chunks
    void conv_out() {
        std::vector<ProbSpec> pr;
        for (int n = 0; n < 2; n++) {
            const NetParams& np = c.net[n];
            const ProbSpec full(src(y[n], c.nk), ln_load(SL_Y, n, P + np.ln_out_g, P + np.ln_out_b), 1, packed(np.co),
                                dst(law.so_w[n], c.dc2));   // (training: the save area)
            if (np.co_chunks.empty()) pr.push_back(full);
            for (size_t k = 0; k < np.co_chunks.size(); k++) {
                pr.push_back(full);
                pr.back().wt = packed(np.co_chunks[k]);
                pr.back().out.off = (int)(64 * k);
                pr.back().out.c = np.co_chunks[k].cout;
            }
        }
        if (c.net[0].co.fmt == PK_TAP && E.p.tap_pw && 9 * c.dc2 <= c.nk && pr.size() == 2) {
            // tap GEMM C = LN_out(LReLU(y)) . W_tap as a streamed 1x1 conv into the dead t1 buffer;
            // k_coupling finishes the 3x3 (tap sums + bias) where it reads s and t
            for (int n = 0; n < 2; n++) {
                pr[n].wt.b = X + E.p.aux_zero;
                pr[n].out = dst(t1[n], 9 * c.dc2);
                law.tc[n] = t1[n];
                law.tbias[n] = X + c.net[n].co.b;
            }
            conv1x1_launch(E, ROLE_CONV_OUT, c.hc, c.wc, pr);
        } else if (c.net[0].co.fmt == PK_TAP) {
            convtap_launch(E, c.hc, c.wc, pr);
        } else {
            conv3_launch(E, ROLE_CONV_OUT, c.hc, c.wc, pr);
        }
    }

    void run(const float* u) {
        conv_in(u);
        for (int r = 0; r < c.R; r++) {
            if (sv.on())
                for (int n = 0; n < 2; n++) t2[n] = sv.acts.t2(n, r);
            conv_a(r);
            grouped(r);
            conv_b(r);
        }
        sv.flush();
        conv_out();
    }
};

// ----------------------------------------------------------------------------------------------
// the coupling law
// ----------------------------------------------------------------------------------------------
// left to the next k_net_lds / k_map2 launch
static CoupPend pending_law(const CoupArgs& w, int ld_parts) {
    CoupPend q;
    q.u = w.u;
    q.s_pre = w.s_pre;
    q.t = w.t;
    q.tanh_w = w.tanh_w;
    q.v = w.v;
    q.ld_part = w.ld_part;
    q.mask_c = w.mask_c;
    q.hc = w.hc;
    q.wc = w.wc;
    q.dc2 = w.dc2;
    q.np = ld_parts;
    q.on = 1;
    q.mask = w.mask;
    q.dc1 = w.dc1;
    q.W = w.W;
    q.D = w.D;
    q.dir = w.dir;
    return q;
}

// k_coupling: affine law + decompress + log-det partials
static void coupling_launch(Exec& E, const CoupArgs& ca) {
    const int B = E.B, np = E.L.ld_parts;
    E.record("k_coupling", 0, 4.0 * B * ca.H * ca.W * ca.D * 2 + 8.0 * B * ca.hc * ca.wc * ca.dc2,
             [ca, B, np](void* st) { launch_coupling(ca, B, np, (hipStream_t)st); });
}

void run_coupling(Exec& E, const Coupling& c, const float* u, float* v, double* ld_part, int dir,
                  const CouplingOpts& o) {
    const WsLayout& L = E.L;
    // k_net_lds layers alternate between two s/t sets by coupling index, so a layer applying its
    // predecessor's deferred coupling never writes the set it reads
    const bool alt = c.use_lds && (c.index & 1) != 0;
    float* const ws_so[2] = {E.at<float>(alt ? L.so_alt[0] : L.so[0]), E.at<float>(alt ? L.so_alt[1] : L.so[1])};
    CoupArgs w = law_of(E, c, u, v, o.so_save ? o.so_save : ws_so, ld_part, dir);
    if (o.save != nullptr && (!c.use_lds || o.so_save == nullptr || o.defer))
        throw std::logic_error("training save: k_net_lds layers without a deferred law only");
    if ((o.pend != nullptr || o.defer) && !c.use_lds)
        throw std::logic_error("deferred couplings are only fused into k_net_lds layers");
    if (o.pend != nullptr && o.pend->dir != dir) throw std::logic_error("deferred coupling of the other direction");
    if (c.use_lds) {
        netlds_layer(E, c, w, o);
    } else {
        if (o.nz != nullptr) throw std::logic_error("fused input noise: k_net_lds layers only");
        Streamed(E, c, w, o.ss).run(u);
    }
    if (o.defer)
        *o.out_pend = pending_law(w, L.ld_parts);
    else
        coupling_launch(E, w);
}

}  // namespace cnf
