// cnf_plan.cpp — host-side restatement of cFlow.__init__ (conv_cINN_make_model.py:1431-1695) and
// of the coupling-layer geometry (:355-498, :1087-1104, conv_cINN_base_functions.py:364-413, 501-627).
// build_plan (at the end) is a sequence of passes, each a function below in the order it runs.
#include <cstring>
#include "cnf_plan.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <functional>
#include <memory>
#include <stdexcept>

namespace cnf {

namespace {

void require(bool ok, const std::string& msg) {
    if (!ok) throw std::invalid_argument(msg);
}

// conv_cINN_make_model.py:1553-1610 (dilation schedule; float arithmetic preserved)
void dilations_for_block(int h, int w, int ksize, std::vector<int>& cw, std::vector<int>& cb) {
    const double min_cw = std::min(h, w);
    const double min_cb = min_cw / 2.0;
    double d = 1.0, dk = ksize;
    if (dk > (min_cw + 1) / 2) {
        cw.push_back(1);
        cb.push_back(1);
        return;
    }
    int sanity = 0;
    while (dk < (min_cw + 1) / 2) {
        require(sanity < 10, "The dilation while loop ran unexpectedly many iterations.");
        cw.push_back((int)d);
        if (d < (min_cb + 1) / 2) cb.push_back((int)d);
        dk = (ksize - 1) * (dk - 1) + 1;
        d = ((dk - ksize) / (ksize - 1)) + 1;
        sanity++;
    }
}

// TF space_to_depth(2) on a per-image index image of shape (h,w,c):
// out[i, j, (di*2+dj)*c + ch] = in[2i+di, 2j+dj, ch]   (squeeze_layer :179)
std::vector<int> s2d(const std::vector<int>& in, int h, int w, int c) {
    std::vector<int> out((size_t)h * w * c);
    const int h2 = h / 2, w2 = w / 2, c4 = 4 * c;
    for (int i = 0; i < h2; i++)
        for (int j = 0; j < w2; j++)
            for (int di = 0; di < 2; di++)
                for (int dj = 0; dj < 2; dj++)
                    for (int ch = 0; ch < c; ch++)
                        out[((size_t)i * w2 + j) * c4 + (di * 2 + dj) * c + ch] =
                            in[((size_t)(2 * i + di) * w + (2 * j + dj)) * c + ch];
    return out;
}

// The dimensions of a packed conv image per format (see PackedConv): the one statement of them. pack
// fills a PackedConv from it and netlds_geometry sizes the LDS image from it. size = floats of the weight
// image, kpad = its K extent; PK_KN has no G.
struct PackedDims {
    int nr = 0, ns = 0, G = 0, kpad = 0;
    int64_t size = 0;
};
PackedDims packed_dims(int fmt, int ks, int cin, int cout) {
    PackedDims d;
    if (fmt == PK_Q4) {
        // K = 9*cin as a list of channel quads qd = tap*(cin/4) + cq (k = tap*cin + 4cq + s);
        // image [g][q][j][s] with qd = 4g + q: G groups of 4 channel quads
        d.nr = (cout + 15) / 16;
        d.ns = 16 * d.nr;
        d.G = (9 * (cin / 4) + 3) / 4;
        d.kpad = d.G * 16;
        d.size = (int64_t)d.G * 16 * d.ns;
    } else if (fmt == PK_KN) {
        d.nr = (cout + 15) / 16;
        d.ns = 16 * d.nr;
        if (d.ns % 32 == 0) d.ns += 16;
        d.kpad = (ks * ks * cin + 3) / 4 * 4;
        d.size = (int64_t)d.kpad * d.ns;
    } else {
        const int ncol = (fmt == PK_TAP) ? 9 * cout : cout;
        d.nr = (ncol + 15) / 16;
        d.ns = 16 * d.nr;
        d.G = (cin + 15) / 16;
        d.kpad = d.G * 16;
        d.size = (int64_t)d.G * 16 * d.ns;
    }
    return d;
}

int align16(int64_t v) { return (int)((v + 15) / 16 * 16); }
int stride8(int ch) {   // == 8 (mod 16) floats: conflict-free ds_read_b128 of channel quads
    int v = std::max(ch, 8);
    while (v % 16 != 8) v++;
    return v;
}
int stride2(int ch) {   // == 2 (mod 4) floats: conflict-free b32 reads of the tap-table path
    int v = std::max(ch, 2);
    while (v % 4 != 2) v++;
    return v;
}

// LDS image of k_net_lds for coupling c under the given conv formats; false if over 160 KiB.
bool netlds_geometry(const Coupling& c, int ci_fmt, int co_fmt, const std::vector<int>& gc_fmt, NetLdsGeom& g) {
    if (c.nk > 64 || c.dc2 > 64 || c.br.size() > 8) return false;
    for (const Branch& b : c.br)
        if (b.dil > 16) return false;
    const int64_t HW = (int64_t)c.hc * c.wc;
    g.sy = stride8(c.nk);
    g.s1 = stride8(c.nk);
    g.s2 = stride8(std::max(std::max(c.gc, c.nk), c.dc2));
    g.su = ci_fmt == PK_Q4 ? stride8(c.dc1) : stride2(c.dc1);
    g.s2r = std::max(g.s2, g.su);
    if (co_fmt == PK_TAP)   // tap-decomposed conv_out scratch (stride 16*nr+1) spans T1..T2
        g.s2r = std::max(g.s2r, 16 * ((9 * c.dc2 + 15) / 16) + (c.dc2 % 4 == 0 ? 4 : 1) - g.s1);
    int64_t wmax = 0;
    int kmax = 4;
    auto acc = [&](int fmt, int ks, int cin, int cout) {
        const PackedDims d = packed_dims(fmt, ks, cin, cout);
        wmax = std::max(wmax, d.size + (cout + 3) / 4 * 4);   // the bias follows the weights in LDS
        if (fmt == PK_KN || fmt == PK_Q4) kmax = std::max(kmax, fmt == PK_Q4 ? d.kpad / 4 : d.kpad);   // tap / quad table
    };
    acc(ci_fmt, 3, c.dc1, c.nk);
    acc(co_fmt, 3, c.nk, c.dc2);
    if (c.R > 0) {
        acc(PK_1X1, 1, c.nk, c.nk);
        acc(PK_1X1, 1, c.gc, c.nk);
        // the grouped branches are staged together: images back to back, tables back to back
        int64_t wsum = 0;
        int ksum = 0;
        for (size_t bi = 0; bi < c.br.size(); bi++) {
            const int cin_pk = gc_fmt[bi] == PK_Q4 ? (c.br[bi].cin + 3) / 4 * 4 : c.br[bi].cin;
            const PackedDims d = packed_dims(gc_fmt[bi], 3, cin_pk, c.br[bi].cout);
            wsum += d.size + (c.br[bi].cout + 3) / 4 * 4;
            ksum += gc_fmt[bi] == PK_Q4 ? d.kpad / 4 : d.kpad;
        }
        wmax = std::max(wmax, wsum);
        kmax = std::max(kmax, ksum);
    }
    // [0, 192): LN-statistics slots (8 waves x 3 doubles); [192, ...): this net's parameter-offset
    // table (2 + R*(10 + 2*nbr) + 4 ints), read from LDS so no phase waits on a global load of it
    const int64_t opn = 2 + (int64_t)c.R * (10 + 2 * (int64_t)c.br.size()) + 4;
    // ... then 16 zero bytes right below Y (k_net_lds: the 3x3 taps outside the image read them)
    int64_t off = std::max<int64_t>(512, align16(NETLDS_OTAB + 4 * opn) + 16);
    g.off_y = (int)off;
    off = align16(off + HW * g.sy * 4);
    g.off_t1 = (int)off;
    off = align16(off + HW * g.s1 * 4);   // T1 and T2 contiguous (tap scratch)
    g.off_t2 = (int)off;
    off = align16(off + HW * g.s2r * 4);
    g.off_w = (int)off;
    off = align16(off + wmax * 4);
    g.off_k = (int)off;
    off = align16(off + (int64_t)kmax * 4);
    // images of at most 4 16-pixel subtiles leave k_net_lds waves idle: their convs split K over the
    // waves and sum the slices through two alternating LDS buffers of (waves - 1) x 5 blocks x 1 KiB
    g.off_ks = 0;
    if ((HW + 15) / 16 <= 4) {
        g.off_ks = (int)off;
        off = align16(off + 2LL * 7 * 5 * 1024);
    }
    g.bytes = (int)std::min<int64_t>(off, 1 << 30);
    return off <= 160 * 1024;
}

// ---- tap mode and the units of a streamed layer's grouped stage ------------------------------------
// A grouped branch can run as k_pw's tap mode (a 1x1 over its 9*cin im2col row, k = tap * cin + c) when
// the row fits (K <= 128) and it has at most 64 outputs; dilations >= TAP_DIL_MIN only: below that the
// staged band's halo is cheap and k_conv<3>'s coalesced band loads beat the row's strided gathers. The
// grouping, both layout planners and the packer ask this one predicate.
constexpr int TAP_DIL_MIN = 4;
bool tap_able(const Branch& b, int ks) { return ks == 3 && 9 * b.cin <= 128 && b.cout <= 64 && b.dil >= TAP_DIL_MIN; }
// ... and a streamed layer's conv_in, the HWIO kernel read as its [9*dc1][nk] im2col matrix (dc1 <= 4: the
// im2col gathers are scalar mask-position loads, cheap only for narrow halves)
bool conv_in_tap_able(const Coupling& c, int ks) { return ks == 3 && c.dc1 <= 4 && c.nk <= 64; }
// branch bi of a streamed layer is launched on its own as k_pw tap mode, so the packer gives it a gpw image
bool lone_tap(const Coupling& c, int bi, int ks) { return !c.in_gc(bi) && tap_able(c.br[bi], ks); }

// The launches of a streamed layer's grouped stage, as lists of branch indices: the k_gc groups, then every
// other branch on its own. all_tap: every lone branch runs as k_pw tap mode (else one falls to k_conv<3>,
// which reads and writes the plain layouts only). They are t1's consumers and t2's producers.
struct StageUnits {
    std::vector<std::vector<int>> units;
    bool all_tap = true;
};
StageUnits stage_units(const Coupling& c, int ks) {
    StageUnits s;
    for (const auto& g : c.gcg) s.units.push_back(g.br);
    for (size_t bi = 0; bi < c.br.size(); bi++) {
        if (c.in_gc((int)bi)) continue;
        s.all_tap = s.all_tap && lone_tap(c, (int)bi, ks);
        s.units.push_back({(int)bi});
    }
    return s;
}

// ---- passes, in the order build_plan runs them ------------------------------------------------------

// Images of 64 x 64 and above (cfg4, cfg5): generic k_pw / k_gc instantiations unless GENERIC is
// given. Their shape-specialised bf16x6 instantiations gave intermittent differences on the
// ragged-batch tests (cfg5 B = 64: 3 of 6 runs, 1e-2 in zy; cfg4 B = 32 once, 3e-4), the generic
// ones none in 8 (profiles/sessions/r6_cfg5b.sh). The cause is open;
// the 32 x 32 and smaller images' instantiations (cfg2, cfg3, ref_default) passed every run.
#ifndef CNF_AUTO_GENERIC
#define CNF_AUTO_GENERIC 6   // (diagnostic builds: 2 / 4 to A/B the two kernels)
#endif
int auto_generic(const cnf_flow_desc& d) {
    const bool given = d.debug_options != nullptr && std::strstr(d.debug_options, "GENERIC=") != nullptr;
    return (int64_t)d.io_h * d.io_w >= 64 * 64 && !given ? CNF_AUTO_GENERIC : 0;
}

// Reads the descriptor; fills p.desc, p.opts (with the GENERIC default above) and the four per-block lists,
// and refuses what cFlow.__init__'s asserts refuse (:1443-1491), in their order and with their messages.
void check_desc(Plan& p, const cnf_flow_desc* d) {
    p.desc = *d;
    p.opts = parse_options(d->debug_options);
    p.opts.generic |= auto_generic(*d);
    p.desc.debug_options = nullptr;   // (the caller's string: not kept)
    const int nb = d->num_blocks;
    require(nb > 0 && d->squeeze_factor_block_list && d->resnext_block_list && d->num_kernels_list &&
                d->cardinality_list,
            "squeeze_factor_block_list, ResNeXt_block_list, num_kernels_list, and cardinality_list must all have the same length.");
    p.sfbl.assign(d->squeeze_factor_block_list, d->squeeze_factor_block_list + nb);
    p.rbl.assign(d->resnext_block_list, d->resnext_block_list + nb);
    p.nkl.assign(d->num_kernels_list, d->num_kernels_list + nb);
    p.cl.assign(d->cardinality_list, d->cardinality_list + nb);
    require(d->io_h > 0 && d->io_w > 0 && d->io_d > 0 && d->x_d > 0 && d->x_d < d->io_d, "invalid io_shape / x_d");
    require(!(d->io_h % 2) && !(d->io_w % 2), "The model input and output must have spatial dimensions divisible by 2.");
    for (int nk : p.nkl) require(!(nk % 2), "The number of kernels in each layer must be divisible by 2.");
    for (int c : p.cl) require(!(c % 2), "The cardinality in each layer must be divisible by 2.");
    for (int s : p.sfbl) require(s == 0 || s == 1, "The only allowed entries in squeeze_factor_block_list are 0 and 1.");
    require(d->ksize == 3, "only ksize=3 is implemented on the GPU path");
    require(d->group_mode == CNF_GROUP_REFERENCE || d->group_mode == CNF_GROUP_INTENDED, "unknown group_mode");
}

// Reads the checked lists and io shape; returns per block the number of factor layers before it, its io
// shape and the dilations of its checkerboard (cb) and channel-wise (cw) layers: the scale schedule
// (:1493-1518), the block shapes (:1521-1536) and the dilation schedule (:1553-1610).
struct BlockShapes {
    std::vector<int> npf, bh, bw, bd;
    std::vector<std::vector<int>> dil_cw, dil_cb;
};
BlockShapes block_shapes(const Plan& p) {
    const int nb = p.desc.num_blocks, H = p.desc.io_h, W = p.desc.io_w, D = p.desc.io_d;
    BlockShapes s;
    // scale schedule :1493-1518
    std::vector<int> scale;
    int scale_flag = 0, nprev = 0;
    for (int i = 0; i < nb; i++) {
        int sf = (i == 0) ? 0 : p.sfbl[i - 1];
        if (!scale_flag) {
            scale.push_back(1);
            scale_flag = 1;
        } else {
            scale.push_back((1 << sf) * scale.back());
        }
        nprev += sf;
        s.npf.push_back(nprev);
    }
    s.bh.resize(nb), s.bw.resize(nb), s.bd.resize(nb);
    for (int i = 0; i < nb; i++) {  // :1521-1536
        require(!(H % (scale[i] * 2)) && !(W % (scale[i] * 2)),
                "The cumulative scale (multiplied by 2 because the checkerboard-masked u/v are halved in spatial dimensions) must divide evenly into the original i/o spatial dimensions. This failed at block " +
                    std::to_string(i));
        s.bh[i] = H / scale[i];
        s.bw[i] = W / scale[i];
        s.bd[i] = D * scale[i];
    }
    s.dil_cw.resize(nb), s.dil_cb.resize(nb);
    for (int i = 0; i < nb; i++) {
        if (p.desc.dilations) {
            dilations_for_block(s.bh[i], s.bw[i], p.desc.ksize, s.dil_cw[i], s.dil_cb[i]);
            double nkc = (double)p.nkl[i] / p.cl[i];
            for (int dd : s.dil_cw[i])
                require(std::fmod(nkc, (double)dd) == 0.0,
                        "The ratio (number of kernels / cardinality) must be evenly divisible by each dilation factor used in that coupling block. This failed in coupling block " +
                            std::to_string(i) + ".");
        } else {
            s.dil_cw[i] = {1};
            s.dil_cb[i] = {1};
        }
    }
    return s;
}

// Reads c.nk, c.card and c.dils; fills c.br and c.gc: one branch per dilation of the grouped stage
// (base_functions.py:364-413, 556-613), as the dense 3x3 conv the kernels run. group_mode REFERENCE keeps
// the reference's closure quirk (every group reads the last group's input channels).
void make_branches(Coupling& c, int group_mode) {
    int off = 0;
    for (int dd : c.dils) {
        Branch b;
        b.dil = dd;
        double nb_ch = std::floor((double)c.nk / dd);  // nk // d (float floor-div)
        if (c.card == 1) {
            b.width = (int)nb_ch;
            b.in_offsets = {0};
            b.cin_off = 0;
            b.cin = b.width;
            b.cout = b.width;
        } else {
            require(std::fmod(nb_ch, (double)c.card) == 0.0, "assert not nb_channels % cardinality");
            b.width = (int)std::floor(nb_ch / c.card);
            require(b.width > 0, "zero-width group (nk / dilation < cardinality): the reference would build a 0-filter Conv2D");
            b.cout = c.card * b.width;
            if (group_mode == CNF_GROUP_REFERENCE) {
                for (int j = 0; j < c.card; j++) b.in_offsets.push_back((c.card - 1) * b.width);
                b.cin_off = (c.card - 1) * b.width;
                b.cin = b.width;
            } else {
                for (int j = 0; j < c.card; j++) b.in_offsets.push_back(j * b.width);
                b.cin_off = 0;
                b.cin = c.card * b.width;
            }
        }
        b.out_off = off;
        off += b.cout;
        c.br.push_back(b);
    }
    c.gc = off;
}

// The coupling layer with mask m (0, 1 checkerboard, 2, 3 channel-wise) of block i: its io shape, the
// compressed u1c shape and uv2 depth, the halved num_kernels of the checkerboard layers and its branches
// (:355-439, :474-498). Reads the block's shape and dilations and the per-block lists.
Coupling make_coupling(const Plan& p, const BlockShapes& s, int i, int m, int index) {
    Coupling c;
    c.index = index;
    c.block = i;
    c.H = s.bh[i];
    c.W = s.bw[i];
    c.D = s.bd[i];
    c.mask = m;
    c.mask_c = (m == 0) ? 1 : (m == 1) ? 0 : (m == 2) ? 3 : 2;
    require(!(c.H % 2) && !(c.W % 2), "u/v must have spatial dimensions divisible by 2.");
    c.nk = (m < 2) ? p.nkl[i] / 2 : p.nkl[i];
    c.card = p.cl[i];
    c.R = p.rbl[i];
    if (m < 2) {
        c.hc = c.H / 2;
        c.wc = c.W / 2;
        c.dc1 = 2 * c.D;
    } else {
        c.hc = c.H;
        c.wc = c.W;
        c.dc1 = (m == 2) ? (c.D + 1) / 2 : c.D / 2;
    }
    if (c.D % 2 && m == 2)
        c.dc2 = c.dc1 - 1;
    else if (c.D % 2 && m == 3)
        c.dc2 = c.dc1 + 1;
    else
        c.dc2 = c.dc1;
    require(c.dc1 > 0 && c.dc2 > 0, "coupling layer with an empty half (io depth too small)");
    c.dils = (m < 2) ? s.dil_cb[i] : s.dil_cw[i];
    make_branches(c, p.desc.group_mode);
    return c;
}

// Fills p.layers and p.couplings from the block shapes: four coupling layers per block, then a squeeze
// and a factor layer where squeeze_factor_block_list says so (layer list :1636-1689).
void layer_list(Plan& p, const BlockShapes& s) {
    for (int i = 0; i < p.desc.num_blocks; i++) {
        Layer L;
        L.h = s.bh[i];
        L.w = s.bw[i];
        L.d = s.bd[i];
        L.block = i;
        for (int m = 0; m < 4; m++) {
            L.kind = CNF_LAYER_COUPLING;
            L.ci = (int)p.couplings.size();
            p.couplings.push_back(make_coupling(p, s, i, m, L.ci));
            p.layers.push_back(L);
        }
        if (p.sfbl[i] == 1) {
            L.ci = -1;
            L.kind = CNF_LAYER_SQUEEZE;
            p.layers.push_back(L);
            L.kind = CNF_LAYER_FACTOR;
            L.npf = s.npf[i];
            p.layers.push_back(L);
        }
    }
}

int64_t add_param(Plan& p, const std::string& name, std::vector<int> shape) {
    ParamTensor t;
    t.name = name;
    t.offset = p.n_params;
    t.shape = shape;
    p.n_params += t.size();
    p.params.push_back(t);
    return t.offset;
}

// Appends coupling c's tensors to the canonical parameter table (Keras order; see oracle/cflow_np.py
// param_specs) and fills c.net[*]'s canonical offsets. Reads c's shapes and branches, ksize and LAYER_NORM.
void param_table(Plan& p, Coupling& c) {
    const int ks = p.desc.ksize;
    const bool ln = p.desc.layer_norm != 0;
    for (int net = 0; net < 2; net++) {
        NetParams& np = c.net[net];
        std::string pre = "c" + std::to_string(c.index) + (net == 0 ? ".A" : ".b");
        np.lo = p.n_params;
        np.conv_in_k = add_param(p, pre + ".conv_in.kernel", {ks, ks, c.dc1, c.nk});
        np.conv_in_b = add_param(p, pre + ".conv_in.bias", {c.nk});
        const int nhw = c.hc * c.wc;
        for (int r = 0; r < c.R; r++) {
            RBParams rb;
            std::string q = pre + ".rb" + std::to_string(r);
            if (ln) {
                rb.ln1g = add_param(p, q + ".ln1.gamma", {nhw * c.nk});
                rb.ln1b = add_param(p, q + ".ln1.beta", {nhw * c.nk});
            }
            rb.conv_a_k = add_param(p, q + ".conv_a.kernel", {1, 1, c.nk, c.nk});
            rb.conv_a_b = add_param(p, q + ".conv_a.bias", {c.nk});
            if (ln) {
                rb.ln2g = add_param(p, q + ".ln2.gamma", {nhw * c.nk});
                rb.ln2b = add_param(p, q + ".ln2.beta", {nhw * c.nk});
            }
            rb.gk.resize(c.br.size());
            rb.gb.resize(c.br.size());
            for (size_t bi = 0; bi < c.br.size(); bi++) {
                const Branch& b = c.br[bi];
                for (size_t j = 0; j < b.in_offsets.size(); j++) {
                    std::string g = q + ".gc.d" + std::to_string(bi) + ".g" + std::to_string(j);
                    rb.gk[bi].push_back(add_param(p, g + ".kernel", {ks, ks, b.width, b.width}));
                    rb.gb[bi].push_back(add_param(p, g + ".bias", {b.width}));
                }
            }
            if (ln) {
                rb.ln3g = add_param(p, q + ".ln3.gamma", {nhw * c.gc});
                rb.ln3b = add_param(p, q + ".ln3.beta", {nhw * c.gc});
            }
            rb.conv_b_k = add_param(p, q + ".conv_b.kernel", {1, 1, c.gc, c.nk});
            rb.conv_b_b = add_param(p, q + ".conv_b.bias", {c.nk});
            np.rb.push_back(rb);
        }
        if (ln) {
            np.ln_out_g = add_param(p, pre + ".ln_out.gamma", {nhw * c.nk});
            np.ln_out_b = add_param(p, pre + ".ln_out.beta", {nhw * c.nk});
        }
        np.conv_out_k = add_param(p, pre + ".conv_out.kernel", {ks, ks, c.nk, c.dc2});
        np.conv_out_b = add_param(p, pre + ".conv_out.bias", {c.dc2});
        if (net == 0) np.tanh_w = add_param(p, pre + ".tanh_scale.w", {});
        np.hi = p.n_params;
    }
}

// conv formats and which layers run the whole-net-in-LDS kernel (CNF_NETLDS=0 disables):
// prefer PK_Q4 for its 3x3 convs (channel-quad ds_read_b128 A reads), fall back to PK_KN
// when the Q4 images do not fit the 160 KiB LDS image, else stream the layer.
// Reads c's shapes and branches and option NETLDS; fills c.ci_fmt, c.co_fmt, c.gc_fmt, c.use_lds, c.lds.
void choose_lds_formats(Coupling& c, const Options& o) {
    const int tapco = 9 * c.dc2 <= 64 ? PK_TAP : PK_KN;
    c.ci_fmt = PK_KN;
    c.co_fmt = tapco;
    c.gc_fmt.assign(c.br.size(), PK_KN);
    c.use_lds = false;
    if (o.netlds == 0) return;
    const int ci9 = c.dc1 % 4 == 0 ? PK_Q4 : PK_KN;
    // conv_out: the tap-decomposed form (1x1 GEMM to 9*dc2 columns, computed in 32-column
    // chunks, + a 9-point shifted sum) when it needs fewer MFMAs than the quad-packed 3x3
    // (ceil(nk/16) * ceil(9 dc2/16) against ceil(9 nk/16) * ceil(dc2/16) 16x16 blocks)
    const int tap_cost = (c.nk + 15) / 16 * ((9 * c.dc2 + 15) / 16);
    const int q4_cost = (9 * c.nk + 15) / 16 * ((c.dc2 + 15) / 16);
    const bool tap = tap_cost < q4_cost;
    const int coq = c.nk % 4 == 0 ? PK_Q4 : PK_KN;
    std::vector<int> gc9;
    for (const Branch& b : c.br) gc9.push_back(b.cin % 4 == 0 && b.cin_off % 4 == 0 ? PK_Q4 : PK_KN);
    NetLdsGeom g;
    int co9 = tap ? PK_TAP : coq;
    bool fit = netlds_geometry(c, ci9, co9, gc9, g);
    if (!fit && co9 == PK_TAP) {   // the tap scratch did not fit: quad-packed conv_out
        co9 = coq;
        fit = netlds_geometry(c, ci9, co9, gc9, g);
    }
    if (fit) {
        c.ci_fmt = ci9;
        c.co_fmt = co9;
        c.gc_fmt = gc9;
        c.use_lds = true;
    } else if (netlds_geometry(c, PK_KN, tapco, c.gc_fmt, g)) {
        c.use_lds = true;
    }
    if (c.use_lds) c.lds = g;
}

// band geometry of a group (branches sel of c) at tile TH x TW: one band per branch, nblk blocks of
// (TH + 2 dil) x (TW + 2 dil) stacked by rows (nblk > 1 / dil_eff: polyphase tiles); false when the group
// does not fit the LDS and staging budgets of a workgroup of nw waves
bool gc_fit_geo(const Coupling& c, const std::vector<int>& sel, int TH, int TW, int dil_eff, int nblk,
                Coupling::GcGroup& out, int nw = GC_NW_SPEC) {
    int64_t off = 512;   // [256, 384): per-image LN table
    std::vector<GcBranch> gb;
    for (int bi : sel) {
        const Branch& b = c.br[bi];
        GcBranch g{};
        g.cin_off = b.cin_off;
        g.cin = b.cin;
        g.cinp = (b.cin + 3) / 4 * 4;
        g.cout = b.cout;
        g.out_off = b.out_off;
        g.opcs = c.gc;
        g.dil = dil_eff > 0 ? dil_eff : b.dil;
        // bf16x6 contraction (cnf_stream.hip k_gc): the band holds S bf16 channels per pixel
        // and plane (2, 4, or a multiple of 8: K = 9 S in 32-deep steps, G of them)
        g.S = b.cin <= 2 ? 2 : b.cin <= 4 ? 4 : (b.cin + 7) / 8 * 8;
        g.G = (9 * g.S + 31) / 32;
        g.BW = TW + 2 * g.dil;
        g.BH = nblk * (TH + 2 * g.dil);
        // staged band units per pixel: channel quads up to S (S = 2: one pair); the quads
        // past the window (to S) are staged as zeros. Exact umulhi division for x < 2^16
        const int cpq = std::max(1, g.S / 4);
        g.cpq_mag = cpq == 1 ? 0u : (uint32_t)((((uint64_t)1 << 32) + cpq - 1) / cpq);
        g.bw_mag = (uint32_t)((((uint64_t)1 << 32) + g.BW - 1) / g.BW);
        if ((int64_t)g.BH * g.BW * cpq >= (1 << 16)) return false;
        if (b.cout > 64) return false;
        g.w_off = (int)off;   // the weights' three bf16 planes: 1 KiB per (K step, plane, 16 outputs)
        off = align16(off + (int64_t)g.G * 3 * ((b.cout + 15) / 16) * 1024);
        g.q_off = (int)off;   // per K octet: up to 4 band offsets (int4)
        off = align16(off + 64LL * g.G);
        g.b_off = (int)off;   // biases (read from LDS in the epilogue: no global load there)
        off = align16(off + 4LL * g.cout);
        gb.push_back(g);
    }
    // the bands (three planes of BH x BW x S bf16 per branch), twice: the next image is
    // staged while the current one is computed
    const int64_t band0 = off;
    int64_t quads = 0;   // staged band units: at most 128 per wave (2 per thread)
    for (GcBranch& g : gb) {
        g.band_off = (int)off;
        off = align16(off + 3 * align16((int64_t)g.BH * g.BW * g.S * 2));
        quads += (int64_t)g.BH * g.BW * std::max(1, g.S / 4);
    }
    const int64_t band_bytes = off - band0;
    off += band_bytes;
    // nw < 16: 16 / nw workgroups share a CU, so its LDS
    if (off > gc_lds_budget(nw) || quads > gc_stage_units(nw)) return false;
    out.nw = nw;
    out.br = sel;
    out.gcb = gb;
    out.TH = TH;
    out.TW = TW;
    out.tiles_x = c.wc / TW;
    out.tiles_y = (c.hc + TH - 1) / TH;
    out.lds = (int)off;
    out.band_bytes = (int)band_bytes;
    out.TP = TH * TW;
    return true;
}
// ... at TP-pixel tiles of TW columns
bool gc_fit(const Coupling& c, const std::vector<int>& sel, int TW, int TP, Coupling::GcGroup& out) {
    const int TH = std::max(1, std::min(c.hc, TP / TW));
    if (!gc_fit_geo(c, sel, TH, TW, 0, 1, out)) return false;
    out.TP = TP;
    return true;
}
// ... at the first tile that fits: full-width row tiles of 256 pixels, then 2-D tiles
bool gc_fit_any(const Coupling& c, const std::vector<int>& sel, Coupling::GcGroup& out) {
    if (c.wc <= 128 && gc_fit(c, sel, c.wc, 256, out)) return true;
    for (int TP : {256, 128, 64})
        for (int TW : {64, 32, 16, 8})
            if (TW < c.wc && c.wc % TW == 0 && TW <= TP && gc_fit(c, sel, TW, TP, out)) return true;
    return false;
}

// streamed layers: the grouped stage as k_gc launches. Each group of branches gets the first
// tile that fits the LDS and staging budgets: full-width row tiles of 256 pixels, then 2-D
// tiles (TW = 64 .. 8 columns, W % TW == 0) of 256, 128, 64 pixels. The branches are taken
// in order of dilation and added to the current group while it still fits, else they open
// a new group; a branch that fits no tile on its own is left out (tap mode when tap_able,
// k_conv<3> otherwise).
// Reads c.use_lds, c's branches and option GC; fills c.gcg and c.gc_fused, and sets the grouped branches'
// c.gc_fmt to PK_Q4.
void plan_gc_groups(Coupling& c, const Options& o, int ks) {
    c.gcg.clear();
    c.gc_fused = false;
    if (c.use_lds || c.R == 0 || c.br.empty() || c.br.size() > (size_t)GC_MAXBR || o.gc == 0) return;
    // a large dilation that does not fit the current group opens a group of its own
    // (cfg5: 485 -> 437 ms/step against tap mode)
    std::vector<int> order;
    for (size_t bi = 0; bi < c.br.size(); bi++) order.push_back((int)bi);
    std::stable_sort(order.begin(), order.end(), [&c](int x, int y) { return c.br[x].dil < c.br[y].dil; });
    Coupling::GcGroup cur;
    bool have = false;
    for (int bi : order) {
        Coupling::GcGroup g;
        if (have) {
            std::vector<int> sel = cur.br;
            sel.push_back(bi);
            // a large dilation joins the current group only at the group's own tile (shrinking
            // the tile for its halo costs more than a launch of its own)
            if (tap_able(c.br[bi], ks) ? gc_fit(c, sel, cur.TW, cur.TP, g) : gc_fit_any(c, sel, g)) {
                cur = g;
                continue;
            }
        }
        if (gc_fit_any(c, {bi}, g)) {
            if (have) c.gcg.push_back(cur);
            cur = g;
            have = true;
        }
    }
    if (have) c.gcg.push_back(cur);
    c.gc_fused = !c.gcg.empty();
    for (const auto& g : c.gcg)
        for (int bi : g.br) c.gc_fmt[bi] = PK_Q4;
}

// a group of one large-dilation branch on polyphase tiles when its phase grids are whole
// (H, W divisible by the dilation): bands of (TH+2) x (TW+2) per grid instead of
// (TH + 2d) x (TW + 2d) (cfg5's dilation-16 branch: 400 staged pixels per 256 outputs
// instead of 1920 per 128); debug option LAYOUT without bit 4: none
// Reads c.gcg and option LAYOUT; replaces the geometry of the groups it retiles (their branches stay).
void retile_polyphase(Coupling& c, const Options& o) {
    if ((o.layout & 4) == 0) return;
    for (auto& gg : c.gcg) {
        if (gg.br.size() != 1) continue;
        const int d = c.br[gg.br[0]].dil;
        if (d < 4 || c.hc % d || c.wc % d) continue;
        const int hs = c.hc / d, wsb = c.wc / d;
        if (wsb > 256 || hs * wsb < 1) continue;
        // tiles of TP pixels: nbk whole grids, or TH-row slices of one grid
        auto tile_for = [hs, wsb, d](int TP, int& nbk, int& TH, int& tpp) {
            nbk = 1;
            TH = hs;
            tpp = 1;
            if (hs * wsb <= TP) {
                while (nbk * 2 * hs * wsb <= TP && (d * d) % (nbk * 2) == 0) nbk *= 2;
            } else {
                TH = std::max(1, TP / wsb);
                while (hs % TH) TH--;
                tpp = hs / TH;
            }
        };
        // four 4-wave workgroups per CU when the band is small (these branches have little
        // MFMA work per image: their time is per-image latency, which co-resident
        // workgroups hide; tiles down to 128 pixels for it), else one 16-wave workgroup
        Coupling::GcGroup g;
        int nbk = 1, TH = hs, tpp = 1;
        bool ok = false;
        for (int TP : {256, 128}) {
            tile_for(TP, nbk, TH, tpp);
            if ((ok = gc_fit_geo(c, gg.br, TH, wsb, 1, nbk, g, 4))) break;
        }
        if (!ok) {
            tile_for(256, nbk, TH, tpp);
            ok = gc_fit_geo(c, gg.br, TH, wsb, 1, nbk, g);
        }
        if (!ok) continue;
        g.ps = d;
        // little work per image: the next image's band load is a whole memory round trip
        // per image unless several are in flight (4 images: 32 VGPRs at 2 quads per thread)
        g.pd = g.nw == 4 ? 4 : 1;
        g.nbk = nbk;
        g.tpp = tpp;
        g.tiles_x = 1;
        g.tiles_y = (d * d / nbk) * tpp;
        gg = g;
    }
}

// streamed layers: t1 as one dense sub-tensor per consumer of it (Coupling::t1_map): each
// k_gc group (and each branch launched on its own) reads only its windows, 16-byte aligned,
// instead of a few channels out of every 256-byte pixel. conv_a runs as k_pw for it (CNF_PW=0
// selects k_conv1, which stores the plain layout), and no branch may be left to k_conv<3>
// (plain layout only); debug option LAYOUT without bit 1: the plain layout
// Reads c.gcg, c's branches and options PW, LAYOUT; fills the t1_* members and the groups' GcBranch
// cin_off / pcs.
void plan_t1_layout(Coupling& c, const Options& o, int ks) {
    c.t1_cs = c.nk;
    c.t1_compact = false;
    c.t1_used = 0;
    c.t1_off.clear();
    c.t1_pcs.clear();
    c.t1_map.clear();
    for (const Branch& b : c.br) {
        c.t1_off.push_back(b.cin_off);
        c.t1_pcs.push_back(c.nk);
        for (int ch = b.cin_off; ch < b.cin_off + b.cin && ch < 64; ch++) c.t1_used |= 1ull << ch;
    }
    for (auto& g : c.gcg)
        for (size_t k = 0; k < g.br.size(); k++) {
            g.gcb[k].cin_off = c.br[g.br[k]].cin_off;
            g.gcb[k].pcs = c.nk;
        }
    const bool allow = o.pw != 0 && (o.layout & 1) != 0;
    if (c.use_lds || c.R == 0 || c.br.empty() || c.nk > 64 || !allow) return;
    // consumers: the k_gc groups, then every other branch (k_pw tap mode) on its own
    const StageUnits su = stage_units(c, ks);
    const auto& units = su.units;
    bool ok = su.all_tap;
    if (!ok) return;
    // every window of a unit at the next 16-byte boundary (in channel order), so each
    // branch's quads stay aligned; windows of one unit must not overlap (one channel, one
    // place), nor may two units share a channel
    std::vector<std::vector<std::pair<int, int>>> uw;   // per unit: (cin_off, branch) sorted
    std::vector<int> ucs;
    uint64_t seen = 0;
    int total = 0;
    for (const auto& u : units) {
        std::vector<std::pair<int, int>> ws;
        for (int bi : u) ws.push_back({c.br[bi].cin_off, bi});
        std::sort(ws.begin(), ws.end());
        uint64_t m = 0;
        int cs = 0;
        for (const auto& wv : ws) {
            const Branch& b = c.br[wv.second];
            for (int ch = b.cin_off; ch < b.cin_off + b.cin; ch++) {
                ok = ok && ((m | seen) >> ch & 1ull) == 0;
                m |= 1ull << ch;
            }
            cs += (b.cin + 3) / 4 * 4;
        }
        seen |= m;
        uw.push_back(ws);
        ucs.push_back(cs);
        total += cs;
    }
    if (!ok || (units.size() == 1 && total >= c.nk)) return;
    const int hw = c.hc * c.wc;
    c.t1_compact = true;
    c.t1_cs = total;
    c.t1_map.assign(128, -1);
    int base = 0;   // floats from the image start to the sub-tensor
    for (size_t u = 0; u < units.size(); u++) {
        const int cs = ucs[u];
        int wo = 0;
        for (const auto& wv : uw[u]) {
            const Branch& b = c.br[wv.second];
            for (int ch = b.cin_off; ch < b.cin_off + b.cin; ch++) {
                c.t1_map[2 * ch] = base + wo + (ch - b.cin_off);
                c.t1_map[2 * ch + 1] = cs;
            }
            c.t1_off[wv.second] = base + wo;
            c.t1_pcs[wv.second] = cs;
            wo += (b.cin + 3) / 4 * 4;
        }
        base += hw * cs;
    }
    for (auto& g : c.gcg)
        for (size_t k = 0; k < g.br.size(); k++) {
            g.gcb[k].cin_off = c.t1_off[g.br[k]];
            g.gcb[k].pcs = c.t1_pcs[g.br[k]];
        }
}

// t2 split into its producers' sub-tensors when there are several (cfg4 / cfg5: k_gc groups of one
// branch each); debug option LAYOUT without bit 2: the plain layout
// Reads c.gcg, c's branches and options PW, LAYOUT; fills the t2_* members and the groups' GcBranch
// out_off / opcs.
void plan_t2_layout(Coupling& c, const Options& o, int ks) {
    c.t2_mapped = false;
    c.t2_cs = c.gc;
    c.t2_off.clear();
    c.t2_pcs.clear();
    c.t2_qmap.clear();
    c.t2_bmap.clear();
    for (const Branch& b : c.br) {
        c.t2_off.push_back(b.out_off);
        c.t2_pcs.push_back(c.gc);
    }
    const bool allow = o.pw != 0 && (o.layout & 2) != 0;
    if (c.use_lds || c.R == 0 || c.br.empty() || !allow || c.gc % 4 != 0 || c.gc > 128) return;
    // producers: the k_gc groups, then every other branch (k_pw tap mode) on its own
    const StageUnits su = stage_units(c, ks);
    const auto& units = su.units;
    bool ok = su.all_tap;
    for (const Branch& b : c.br) ok = ok && b.out_off % 4 == 0 && b.cout % 4 == 0;
    if (!ok || units.size() < 2) return;
    const int hw = c.hc * c.wc;
    std::vector<int> ust, ucs;
    int total = 0;
    for (const auto& u : units) {
        int lo = 1 << 30, hi = 0, sum = 0;
        for (int bi : u) {
            lo = std::min(lo, c.br[bi].out_off);
            hi = std::max(hi, c.br[bi].out_off + c.br[bi].cout);
            sum += c.br[bi].cout;
        }
        ok = ok && sum == hi - lo;   // the unit's slices are one channel range
        ust.push_back(lo);
        ucs.push_back(hi - lo);
        total += hi - lo;
    }
    if (!ok || total != c.gc) return;
    c.t2_mapped = true;
    c.t2_cs = total;
    c.t2_qmap.assign((size_t)2 * (c.gc / 4), -1);
    c.t2_bmap.assign(c.br.size(), std::vector<int>(128, -1));
    int base = 0;
    for (size_t u = 0; u < units.size(); u++) {
        for (int ch = ust[u]; ch < ust[u] + ucs[u]; ch += 4) {
            c.t2_qmap[2 * (ch / 4)] = base + (ch - ust[u]);
            c.t2_qmap[2 * (ch / 4) + 1] = ucs[u];
        }
        for (int bi : units[u]) {
            const Branch& b = c.br[bi];
            c.t2_off[bi] = base + (b.out_off - ust[u]);
            c.t2_pcs[bi] = ucs[u];
            for (int j = 0; j < b.cout; j++) {
                c.t2_bmap[bi][2 * j] = c.t2_off[bi] + j;
                c.t2_bmap[bi][2 * j + 1] = ucs[u];
            }
        }
        base += hw * ucs[u];
    }
    for (auto& g : c.gcg)
        for (size_t k = 0; k < g.br.size(); k++) {
            g.gcb[k].out_off = c.t2_off[g.br[k]];
            g.gcb[k].opcs = c.t2_pcs[g.br[k]];
        }
}

// ---- the kernel image and the dense backward image ---------------------------------------------------
// Where a conv's weights and bias come from: the canonical parameter offset of element (k, n) of its
// [taps*cin][cout] matrix (-1: a structural zero) and of bias n. Each conv states it once; pack and
// dense_img both read it.
struct ConvSrc {
    std::function<int64_t(int, int)> w;
    std::function<int64_t(int)> b;
};
// a Keras HWIO kernel at canonical offset k_off read as its [taps*cin][cout] matrix, bias at b_off
ConvSrc hwio_src(int64_t k_off, int64_t b_off, int cout) {
    return {[=](int k, int n) { return k_off + (int64_t)k * cout + n; }, [=](int n) { return b_off + n; }};
}
// dense [9*cin][cout] view of the card per-group Conv2D kernels of a branch (:401-411)
ConvSrc grouped_src(const Branch& b, const std::vector<int64_t>& gk, const std::vector<int64_t>& gb) {
    return {[=](int k, int n) -> int64_t {
                const int tap = k / b.cin, ci2 = k - tap * b.cin;
                const int j = n / b.width, o = n - j * b.width;
                const int in_rel = b.in_offsets[j] - b.cin_off;
                const int cj = ci2 - in_rel;
                if (cj < 0 || cj >= b.width) return -1;
                return gk[j] + ((int64_t)tap * b.width + cj) * b.width + o;
            },
            [=](int n) { return gb[n / b.width] + (n % b.width); }};
}
// views of a source: cin padded to cin_pk channels per tap (the padding channels carry zero weights) ...
ConvSrc padded_cin(const ConvSrc& s, int cin, int cin_pk) {
    return {[=](int k, int n) -> int64_t {
                const int tap = k / cin_pk, ci = k - tap * cin_pk;
                return ci < cin ? s.w(tap * cin + ci, n) : -1;
            },
            s.b};
}
// ... the tap GEMM's [cin][9*cout] matrix, columns j = tap*cout + o ...
ConvSrc tap_columns(const ConvSrc& s, int cin, int cout) {
    return {[=](int c, int j) { return s.w(j / cout * cin + c, j % cout); }, s.b};
}
// ... and the output columns from c0 on
ConvSrc columns_from(const ConvSrc& s, int c0) {
    return {[=](int k, int n) { return s.w(k, c0 + n); }, [=](int n) { return s.b(c0 + n); }};
}

// element s of quad qd (PK_Q4: channel quad tap * cin / 4 + cq; PK_1X1 / PK_TAP: input channels 4 qd .. + 3),
// column j of a quad image [g][q][j][s], qd = 4g + q, of ns columns: the one statement of that layout (pack
// writes with it, the plane image reads the fp32 image back with it)
int64_t quad_at(int ns, int qd, int j, int s) { return ((int64_t)qd * ns + j) * 4 + s; }

// kernel image (aux): a conv's weights + bias packed in its kernel's LDS layout (formats: PackedConv)
void pack(Plan& p, PackedConv& pc, int fmt, int cin, int cout, const ConvSrc& s) {
    const int ks = p.desc.ksize;
    const PackedDims d = packed_dims(fmt, ks, cin, cout);
    pc.fmt = fmt;
    pc.cin = cin;
    pc.cout = cout;
    pc.nr = d.nr;
    pc.ns = d.ns;
    pc.G = d.G;
    pc.kpad = d.kpad;
    pc.size = d.size;
    pc.w = p.n_aux;
    p.aux_map.resize(p.aux_map.size() + (size_t)pc.size, -1);
    int64_t* img = p.aux_map.data() + pc.w;
    if (fmt == PK_Q4) {
        const int cpq = cin / 4, nq = 9 * cpq;
        for (int qd = 0; qd < nq; qd++)
            for (int j = 0; j < cout; j++)
                for (int s4 = 0; s4 < 4; s4++) {
                    const int tap = qd / cpq, cq = qd - tap * cpq;
                    img[quad_at(pc.ns, qd, j, s4)] = s.w(tap * cin + 4 * cq + s4, j);
                }
    } else if (fmt == PK_KN) {
        const int K = ks * ks * cin;
        for (int k = 0; k < K; k++)
            for (int n = 0; n < cout; n++) img[(int64_t)k * pc.ns + n] = s.w(k, n);
    } else {
        const int ncol = (fmt == PK_TAP) ? 9 * cout : cout;
        for (int c = 0; c < cin; c++)
            for (int j = 0; j < ncol; j++) img[quad_at(pc.ns, c >> 2, j, c & 3)] = s.w(c, j);
    }
    p.n_aux += pc.size;
    pc.b = p.n_aux;
    const int bpad = (cout + 3) / 4 * 4;
    for (int n = 0; n < bpad; n++) p.aux_map.push_back(n < cout ? s.b(n) : -1);
    p.n_aux += bpad;
}
// ---- the bf16x6 plane image (debug option PRESPLIT) ---------------------------------------------------
// One conv's planes appended to aux: C K steps of NR column blocks (cnf_kernels.h x6_at), element (k, col)
// from the parameter that float at(k, col) of the fp32 kernel image holds (at < 0, or no parameter there:
// zero). One x6_map entry per 16-bit unit.
void plane_image(Plan& p, PackedConv& pc, int C, int NR, const std::function<int64_t(int, int)>& at) {
    require(p.n_aux % 4 == 0, "plane image not 16-byte aligned");
    pc.x6 = p.n_aux;
    pc.x6_C = C;
    const size_t base = p.x6_map.size();
    p.x6_map.resize(base + (size_t)(x6_bytes(C, NR) / 2), -1);
    for (int k = 0; k < 32 * C; k++)
        for (int col = 0; col < 16 * NR; col++) {
            const int64_t a = at(k, col);
            const int64_t src = a >= 0 ? p.aux_map[(size_t)a] : -1;
            if (src < 0) continue;
            for (int pl = 0; pl < 3; pl++) p.x6_map[base + (size_t)x6_at(k, col, pl, NR) / 2] = 4 * src + pl;
        }
    p.n_aux += x6_bytes(C, NR) / 4;
}
constexpr int X6_DIR_WORDS = 16;
// directory entry of the image just built: [kind (0 k_pw, 1 k_gc), coupling, net, role, residual block,
// branch, x6, C, NR, fp32 image, ns, k_pw: G of the fp32 image / k_gc: cinp, cout, K rows with weights
// (k_pw: cin; k_gc: S), dil, BW]
void plane_dir(Plan& p, const PackedConv& pc, int kind, int ci, int net, int role, int rb, int bi, int NR, int g_or_cinp,
               int krows, int dil, int BW) {
    for (int64_t v : {(int64_t)kind, (int64_t)ci, (int64_t)net, (int64_t)role, (int64_t)rb, (int64_t)bi, pc.x6,
                      (int64_t)pc.x6_C, (int64_t)NR, pc.w, (int64_t)pc.ns, (int64_t)g_or_cinp, (int64_t)pc.cout,
                      (int64_t)krows, (int64_t)dil, (int64_t)BW})
        p.x6_dir.push_back(v);
}
// a k_pw conv (PK_1X1 / PK_TAP image: rows k < 16 G, ns = 16 nr columns); k_pw runs K <= 128
void pw_planes(Plan& p, PackedConv& pc, int ci, int net, int role, int rb, int bi) {
    if (pc.size == 0 || pc.G > 8) return;
    const PackedConv q = pc;
    plane_image(p, pc, (pc.cin + 31) / 32, pc.nr,
                [q](int k, int col) { return k < 16 * q.G ? q.w + quad_at(q.ns, k >> 2, col, k & 3) : (int64_t)-1; });
    plane_dir(p, pc, 0, ci, net, role, rb, bi, pc.nr, pc.G, pc.cin, 0, 0);
}
// a k_gc branch (PK_Q4 image over cinp channels per tap): K index k = tap * S + ch (GcBranch), then its
// K-octet table (gc_octet_word), 16 G ints as two literal 16-bit units each
void gc_planes(Plan& p, PackedConv& pc, const GcBranch& g, int ci, int net, int rb, int bi) {
    require(pc.fmt == PK_Q4 && pc.cin == g.cinp, "k_gc branch without a PK_Q4 image");
    const PackedConv q = pc;
    const int cpq = g.cinp / 4, S = g.S, cinp = g.cinp;
    plane_image(p, pc, g.G, pc.nr, [q, cpq, S, cinp](int k, int col) {
        const int tap = k / S, ch = k - tap * S;
        return tap < 9 && ch < cinp ? q.w + quad_at(q.ns, tap * cpq + (ch >> 2), col, ch & 3) : (int64_t)-1;
    });
    for (int e = 0; e < 4 * g.G; e++)
        for (int j = 0; j < 4; j++) {
            const uint32_t w = (uint32_t)gc_octet_word(g.S, g.dil, g.BW, e, j);
            p.x6_map.push_back(-2 - (int64_t)(w & 0xffffu));
            p.x6_map.push_back(-2 - (int64_t)(w >> 16));
        }
    p.n_aux += 16 * g.G;
    plane_dir(p, pc, 1, ci, net, ROLE_GC, rb, bi, pc.nr, g.cinp, g.S, g.dil, g.BW);
}
// Appends the plane images of every conv a streamed coupling's k_pw / k_gc launches can run, after all
// fp32 images. Reads the PackedConvs' fp32 images (p.aux_map) and c.gcg; fills PackedConv::x6, p.x6_map,
// p.x6_dir.
void pack_planes(Plan& p, Coupling& c, int ci) {
    if (c.use_lds) return;
    for (int net = 0; net < 2; net++) {
        NetParams& np = c.net[net];
        pw_planes(p, np.ci_pw, ci, net, ROLE_CONV_IN, -1, -1);
        for (size_t r = 0; r < np.rb.size(); r++) {
            RBParams& rb = np.rb[r];
            pw_planes(p, rb.ca, ci, net, ROLE_CONV_A, (int)r, -1);
            for (const Coupling::GcGroup& gg : c.gcg)
                for (size_t k = 0; k < gg.br.size(); k++)
                    gc_planes(p, rb.gc[gg.br[k]], gg.gcb[k], ci, net, (int)r, gg.br[k]);
            for (size_t bi = 0; bi < rb.gpw.size(); bi++) pw_planes(p, rb.gpw[bi], ci, net, ROLE_GC, (int)r, (int)bi);
            pw_planes(p, rb.cb, ci, net, ROLE_CONV_B, (int)r, -1);
        }
        if (np.co.fmt == PK_TAP) pw_planes(p, np.co, ci, net, ROLE_CONV_OUT, -1, -1);
    }
}

// dense backward image: a conv as [taps][cin][cout] + [cout] bias (training kernels)
void dense_img(Plan& p, PackedConv& pc, int taps, int cin, int cout, const ConvSrc& s) {
    pc.taps = taps;
    pc.dw = p.n_bw;
    for (int k = 0; k < taps * cin; k++)
        for (int n = 0; n < cout; n++) p.bw_map.push_back(s.w(k, n));
    p.n_bw += (int64_t)taps * cin * cout;
    pc.db = p.n_bw;
    for (int n = 0; n < cout; n++) p.bw_map.push_back(s.b(n));
    p.n_bw += (cout + 3) / 4 * 4;
    for (int n = cout; n < (cout + 3) / 4 * 4; n++) p.bw_map.push_back(-1);
}
// LN gamma / beta gathered into a sub-tensor layout (0 on padding): appends to the kernel image, for each
// of the two, hw * cs floats of which channel ch of pixel px lies at at(ch).first + px * at(ch).second and
// comes from parameter px * nch + ch (at(ch).first < 0: the channel is not stored); g_out / b_out: where
void ln_gather(Plan& p, int64_t hw, int cs, int nch, const std::function<std::pair<int, int>(int)>& at,
               int64_t gamma, int64_t beta, int64_t& g_out, int64_t& b_out) {
    std::vector<int64_t> par((size_t)hw * cs, -1);   // image float -> its parameter, relative to gamma / beta
    for (int ch = 0; ch < nch; ch++) {
        const std::pair<int, int> a = at(ch);
        if (a.first < 0) continue;
        for (int64_t px = 0; px < hw; px++) par[a.first + px * a.second] = px * nch + ch;
    }
    for (int which = 0; which < 2; which++) {
        const int64_t src = which == 0 ? gamma : beta;
        (which == 0 ? g_out : b_out) = p.n_aux;
        for (int64_t v : par) p.aux_map.push_back(v >= 0 ? src + v : -1);
        p.n_aux += (int64_t)par.size();
    }
}

// One residual block's images, in kernel-image order: conv_a, the branches (+ their gpw images), the LN
// gathers, conv_b. Reads c's formats, groups and layouts and rb's canonical offsets; fills rb's PackedConvs
// and ln2c_* / ln3c_*.
void pack_res_block(Plan& p, const Coupling& c, RBParams& rb) {
    const int ks = p.desc.ksize, nk = c.nk;
    const ConvSrc a = hwio_src(rb.conv_a_k, rb.conv_a_b, nk);
    pack(p, rb.ca, PK_1X1, nk, nk, a);
    dense_img(p, rb.ca, 1, nk, nk, a);
    for (size_t bi = 0; bi < c.br.size(); bi++) {
        const Branch& b = c.br[bi];
        const ConvSrc dense = grouped_src(b, rb.gk[bi], rb.gb[bi]);
        PackedConv pc;
        // PK_Q4 over cin padded to a multiple of 4 (padding channels carry zero weights)
        const int cin_pk = c.gc_fmt[bi] == PK_Q4 ? (b.cin + 3) / 4 * 4 : b.cin;
        pack(p, pc, c.gc_fmt[bi], cin_pk, b.cout, padded_cin(dense, b.cin, cin_pk));
        dense_img(p, pc, ks * ks, b.cin, b.cout, dense);
        rb.gc.push_back(pc);
        // streamed layers without k_gc: the branch as k_pw's tap mode (see tap_able)
        PackedConv pw;
        if (!c.use_lds && lone_tap(c, (int)bi, ks)) pack(p, pw, PK_1X1, 9 * b.cin, b.cout, dense);
        rb.gpw.push_back(pw);
    }
    const int64_t hw = (int64_t)c.hc * c.wc;
    const bool ln = p.desc.layer_norm != 0;
    if (c.t1_compact && ln)   // LN2 gamma/beta in t1's layout (0 on padding)
        ln_gather(p, hw, c.t1_cs, nk, [&c](int ch) { return std::make_pair(c.t1_map[2 * ch], c.t1_map[2 * ch + 1]); },
                  rb.ln2g, rb.ln2b, rb.ln2c_g, rb.ln2c_b);
    if (c.t2_mapped && ln)   // LN3 gamma/beta in t2's layout
        ln_gather(p, hw, c.t2_cs, c.gc,
                  [&c](int ch) { return std::make_pair(c.t2_qmap[2 * (ch / 4)] + ch % 4, c.t2_qmap[2 * (ch / 4) + 1]); },
                  rb.ln3g, rb.ln3b, rb.ln3c_g, rb.ln3c_b);
    const ConvSrc cb = hwio_src(rb.conv_b_k, rb.conv_b_b, nk);
    pack(p, rb.cb, PK_1X1, c.gc, nk, cb);
    dense_img(p, rb.cb, 1, c.gc, nk, cb);
}

// Appends coupling c's convs to the kernel image (p.aux_map / n_aux: every conv's weights + bias packed in
// its kernel's LDS layout) and to the dense backward image (p.bw_map / n_bw). Reads the formats, groups and
// layouts the passes above chose and the canonical offsets; fills the PackedConvs of c.net[*].
void pack_images(Plan& p, Coupling& c) {
    const int ks = p.desc.ksize, nk = c.nk, dc2 = c.dc2;
    for (int net = 0; net < 2; net++) {
        NetParams& np = c.net[net];
        const ConvSrc in = hwio_src(np.conv_in_k, np.conv_in_b, nk);
        pack(p, np.ci, c.ci_fmt, c.dc1, nk, in);
        dense_img(p, np.ci, ks * ks, c.dc1, nk, in);
        // streamed layers: conv_in for k_pw's tap mode (see conv_in_tap_able)
        if (!c.use_lds && conv_in_tap_able(c, ks)) pack(p, np.ci_pw, PK_1X1, 9 * c.dc1, nk, in);
        for (auto& rb : np.rb) pack_res_block(p, c, rb);
        const ConvSrc out = hwio_src(np.conv_out_k, np.conv_out_b, dc2);
        pack(p, np.co, c.co_fmt, nk, dc2, c.co_fmt == PK_TAP ? tap_columns(out, nk, dc2) : out);
        dense_img(p, np.co, ks * ks, nk, dc2, out);
        // the streamed kernels produce at most 64 output channels per problem
        if (!c.use_lds && c.co_fmt != PK_TAP && dc2 > 64) {
            for (int c0 = 0; c0 < dc2; c0 += 64) {
                PackedConv pc;
                pack(p, pc, PK_KN, nk, std::min(64, dc2 - c0), columns_from(out, c0));
                np.co_chunks.push_back(pc);
            }
        }
    }
}

// Reads the PackedConvs and canonical offsets of c.net[*]; fills c.lds_offs, the k_net_lds offset table
// (params offsets for LN gamma/beta, kernel-image offsets for convs), and for an LDS layer c.bwd_offs, the
// fused LDS-layer backward offset table (LDSBWD_* layout: canonical LN / range offsets, dense
// backward-image conv offsets).
void offset_tables(Coupling& c) {
    for (int net = 0; net < 2; net++) {
        const NetParams& np = c.net[net];
        std::vector<int> o = {(int)np.ci.w, (int)np.ci.b};
        for (const auto& rb : np.rb) {
            for (int64_t v : {rb.ln1g, rb.ln1b, rb.ca.w, rb.ca.b, rb.ln2g, rb.ln2b, rb.ln3g, rb.ln3b, rb.cb.w, rb.cb.b})
                o.push_back((int)std::max<int64_t>(v, 0));
            for (const auto& g : rb.gc) {
                o.push_back((int)g.w);
                o.push_back((int)g.b);
            }
        }
        for (int64_t v : {np.ln_out_g, np.ln_out_b, np.co.w, np.co.b}) o.push_back((int)std::max<int64_t>(v, 0));
        c.lds_offs_per_net = (int)o.size();
        c.lds_offs.insert(c.lds_offs.end(), o.begin(), o.end());
    }
    if (!c.use_lds) return;
    for (int net = 0; net < 2; net++) {
        const NetParams& np = c.net[net];
        std::vector<int> o = {(int)np.lo, (int)np.ci.dw, (int)np.ci.db, (int)np.ln_out_g, (int)np.ln_out_b,
                              (int)np.co.dw, (int)np.co.db, (int)np.tanh_w, (int)np.conv_in_k, (int)np.conv_in_b,
                              (int)np.conv_out_k, (int)np.conv_out_b};
        for (const auto& rb : np.rb) {
            for (int64_t v : {rb.ln1g, rb.ln1b, rb.ca.dw, rb.ca.db, rb.ln2g, rb.ln2b, rb.ln3g, rb.ln3b, rb.cb.dw,
                              rb.cb.db, rb.conv_a_k, rb.conv_a_b, rb.conv_b_k, rb.conv_b_b})
                o.push_back((int)v);
            for (const auto& g : rb.gc) {
                o.push_back((int)g.dw);
                o.push_back((int)g.db);
            }
        }
        c.bwd_offs_per_net = (int)o.size();
        c.bwd_offs.insert(c.bwd_offs.end(), o.begin(), o.end());
    }
}

// squeeze/factor boundary maps. orig[i] = position in the xy layout of element i of
// the current block layout: the forward's final restoration (:1762-1770) is the exact
// inverse of the squeeze/factor chain, so every element returns to where it started.
// Reads the io shape and squeeze_factor_block_list; fills p.boundaries, p.final_orig and p.last_n.
void boundary_maps(Plan& p) {
    int ch = p.desc.io_h, cw = p.desc.io_w, cd = p.desc.io_d;
    std::vector<int> orig((size_t)ch * cw * cd);
    for (size_t i = 0; i < orig.size(); i++) orig[i] = (int)i;
    for (int i = 0; i < p.desc.num_blocks; i++) {
        if (p.sfbl[i] != 1) continue;
        Boundary bd;
        bd.after_block = i;
        const int n = ch * cw * cd;
        std::vector<int> ar(n);
        for (int k = 0; k < n; k++) ar[k] = k;
        std::vector<int> sq = s2d(ar, ch, cw, cd);
        const int h2 = ch / 2, w2 = cw / 2, c4 = 4 * cd, split = c4 / 2;
        std::vector<int> norig;
        for (int px = 0; px < h2 * w2; px++) {
            for (int c = 0; c < split; c++) {
                int src = sq[(size_t)px * c4 + c];
                bd.fac_src.push_back(src);
                bd.fac_orig.push_back(orig[src]);
            }
            for (int c = split; c < c4; c++) {
                int src = sq[(size_t)px * c4 + c];
                bd.keep_src.push_back(src);
                norig.push_back(orig[src]);
            }
        }
        bd.n_cur = n;
        bd.n_next = (int)bd.keep_src.size();
        bd.n_fac = (int)bd.fac_src.size();
        orig = norig;
        ch = h2;
        cw = w2;
        cd = split;
        p.boundaries.push_back(bd);
    }
    p.final_orig = orig;
    p.last_n = (int)orig.size();
}

// device table image: [boundaries..., per coupling its offset tables and layout maps, final_orig].
// Reads those vectors; fills p.host_table and every dev_* offset into it.
void device_table(Plan& p) {
    auto append = [&p](const std::vector<int>& v) {
        const int at = (int)p.host_table.size();
        p.host_table.insert(p.host_table.end(), v.begin(), v.end());
        return at;
    };
    for (auto& b : p.boundaries) {
        b.dev_keep_src = append(b.keep_src);
        b.dev_fac_src = append(b.fac_src);
        b.dev_fac_orig = append(b.fac_orig);
    }
    for (auto& c : p.couplings) {
        c.dev_lds_offs = append(c.lds_offs);
        if (!c.bwd_offs.empty()) c.dev_bwd_offs = append(c.bwd_offs);
        if (c.t1_compact) c.dev_t1_map = append(c.t1_map);
        c.dev_t2_bmap.assign(c.br.size(), -1);
        if (c.t2_mapped) {
            c.dev_t2_qmap = append(c.t2_qmap);
            for (size_t bi = 0; bi < c.br.size(); bi++) c.dev_t2_bmap[bi] = append(c.t2_bmap[bi]);
        }
    }
    p.dev_final_orig = append(p.final_orig);
}
}  // namespace

// The passes above, in order. use_pw, tap_pw and lds_bwd are not set here: cnf_plan_create sets them on
// the built plan (ldsbwd_setup lives in cnf_train.cpp).
Plan* build_plan(const cnf_flow_desc* d) {
    require(d != nullptr, "null descriptor");
    auto P = std::make_unique<Plan>();
    Plan& p = *P;
    check_desc(p, d);
    layer_list(p, block_shapes(p));
    for (auto& c : p.couplings) param_table(p, c);
    const int ks = p.desc.ksize;
    for (auto& c : p.couplings) {
        choose_lds_formats(c, p.opts);
        plan_gc_groups(c, p.opts, ks);
        retile_polyphase(c, p.opts);
        plan_t1_layout(c, p.opts, ks);
        plan_t2_layout(c, p.opts, ks);
    }
    for (auto& c : p.couplings) pack_images(p, c);
    p.aux_zero = p.n_aux;   // 128 zeros (bias of the bias-free tap GEMM, up to 80 columns)
    p.aux_map.resize(p.aux_map.size() + 128, -1);
    p.n_aux += 128;
    p.x6_base = p.n_aux;
    if (p.opts.presplit != 0) {
        while (p.n_aux % 4 != 0) {   // (the plane images are copied 16 bytes at a time)
            p.aux_map.push_back(-1);
            p.n_aux++;
        }
        p.x6_base = p.n_aux;
        for (size_t ci = 0; ci < p.couplings.size(); ci++) pack_planes(p, p.couplings[ci], (int)ci);
        p.aux_map.resize((size_t)p.n_aux, -1);   // (no fp32 entries there: k_pack stops at x6_base)
    }
    require((int64_t)p.x6_map.size() == 2 * (p.n_aux - p.x6_base), "plane map out of step with the plane region");
    require(p.n_params < (1ll << 31) && p.n_aux < (1ll << 31), "parameter image exceeds 2^31 floats");
    require(p.n_bw < (1ll << 31), "dense backward image exceeds 2^31 floats");
    for (auto& c : p.couplings) offset_tables(c);
    boundary_maps(p);
    device_table(p);
    return P.release();
}

}  // namespace cnf
