// cnf_debug.cpp — the introspection part of the C ABI (include/cnf.h): the cnf_debug_* shape, layout, schedule and
// stamp dumps the generators, tests and profiles read, and a plan's recorded launches and weight maps.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "cnf_api.h"
#include "cnf_plan.h"

using namespace cnf;

// coupling `coupling` of the plan (null: no plan, or out of range)
static const Coupling* coupling_of(const cnf_plan* plan, int coupling) {
    const bool ok = plan && coupling >= 0 && coupling < (int)plan->p->couplings.size();
    return ok ? &plan->p->couplings[coupling] : nullptr;
}

// head, then per branch (off, pcs, members a and b), then tail, into words; returns the count, -1 over cap
static int layout_words(std::vector<int> w, const Coupling& c, const std::vector<int>& off, const std::vector<int>& pcs,
                        int Branch::*a, int Branch::*b, const std::vector<int>& tail, int* words, int cap) {
    for (size_t bi = 0; bi < c.br.size(); bi++) {
        w.push_back(bi < off.size() ? off[bi] : -1);
        w.push_back(bi < pcs.size() ? pcs[bi] : -1);
        w.push_back(c.br[bi].*a);
        w.push_back(c.br[bi].*b);
    }
    w.insert(w.end(), tail.begin(), tail.end());
    if ((int)w.size() > cap) return -1;
    std::memcpy(words, w.data(), w.size() * sizeof(int));
    return (int)w.size();
}

extern "C" {

// shape words of coupling `coupling`'s k_net_lds launch (0 if the layer is streamed); host only, used
// by csrc/gen_netlds_shapes.py to generate the shape-specialised instantiations' table
int cnf_debug_netlds_shape(const cnf_plan* plan, int coupling, int* words, int cap) {
    OptScope os_(plan ? &plan->p->opts : nullptr);
    const Coupling* c = coupling_of(plan, coupling);
    if (!c || !words || cap < NETSHAPE_WORDS) return -1;
    NetLdsArgs a;
    if (!c->use_lds || netlds_setup(*plan->p, *c, a) == 0) return 0;
    netshape_words(a, words);
    return NETSHAPE_WORDS;
}
int cnf_debug_netlds_nshapes() { return netlds_num_shapes(); }

// launch names of a B-image forward (direction +1), inverse (-1) or inverse with log-det (-2) from a host-only
// dry run, one per line into out (cap bytes, NUL-terminated); returns the number of launches, -1 on error
int cnf_debug_schedule(cnf_plan* plan, int B, int direction, char* out, int cap) {
    OptScope os_(plan ? &plan->p->opts : nullptr);
    if (!plan || !out || cap <= 0 || B <= 0 || (direction != 1 && direction != -1 && direction != -2)) return -1;
    Plan& p = *plan->p;
    CNF_TRY
    dry_run(p, B, direction);
    std::string s;
    for (const std::string& n : p.dry_launches) s += n + "\n";
    if ((int)s.size() + 1 > cap) return -1;
    std::memcpy(out, s.c_str(), s.size() + 1);
    return (int)p.dry_launches.size();
    CNF_CATCH
}

// k_pw launch shapes of a B-image forward, from a host-only dry run (nothing is launched or
// dereferenced: the tensors are placeholder addresses); returns the number of words written
int cnf_debug_pw_shapes(cnf_plan* plan, int B, int* words, int cap) {
    OptScope os_(plan ? &plan->p->opts : nullptr);
    if (!plan || !words || B <= 0) return -1;
    Plan& p = *plan->p;
    CNF_TRY
    p.pw_shapes.clear();
    p.gc_launch.clear();
    dry_run(p, B, +1);
    const int n = (int)p.pw_shapes.size() * PWSHAPE_WORDS;
    if (n > cap) return -1;
    for (size_t i = 0; i < p.pw_shapes.size(); i++)
        std::memcpy(words + i * PWSHAPE_WORDS, &p.pw_shapes[i], sizeof(PwShape));
    return n;
    CNF_CATCH
}

int cnf_debug_pw_nshapes() { return pw_num_shapes(); }
int cnf_debug_pw_words() { return PWSHAPE_WORDS; }

// k_gc launch shapes of a B-image forward (host-only dry run, as cnf_debug_pw_shapes)
int cnf_debug_gc_launch_shapes(cnf_plan* plan, int B, int* words, int cap) {
    OptScope os_(plan ? &plan->p->opts : nullptr);
    if (!plan || !words || B <= 0) return -1;
    const int n = cnf_debug_pw_shapes(plan, B, words, cap);   // the dry run also records the k_gc shapes
    if (n < 0) return -1;
    const std::vector<GcShape>& g = plan->p->gc_launch;
    if ((int64_t)g.size() * GCSHAPE_WORDS > cap) return -1;
    for (size_t i = 0; i < g.size(); i++) std::memcpy(words + i * GCSHAPE_WORDS, &g[i], sizeof(GcShape));
    return (int)g.size() * GCSHAPE_WORDS;
}

// shape words of coupling `coupling`'s k_gc launches, one GcShape per group (0 if it has none)
int cnf_debug_gc_shape(const cnf_plan* plan, int coupling, int* words, int cap) {
    OptScope os_(plan ? &plan->p->opts : nullptr);
    const Coupling* c = coupling_of(plan, coupling);
    if (!c || !words) return -1;
    if (c->use_lds || !c->gc_fused) return 0;
    if (cap < GCSHAPE_WORDS * (int)c->gcg.size()) return -1;
    int n = 0;
    for (const Coupling::GcGroup& gg : c->gcg) {
        // the forward's k_gc: LN2 on load and LN3 partials iff LayerNorm
        const GcShape s = gc_shape(*c, gg, plan->p->desc.layer_norm ? 3 : 0);
        std::memcpy(words + n, &s, sizeof(s));
        n += GCSHAPE_WORDS;
    }
    return n;
}
int cnf_debug_gc_words() { return GCSHAPE_WORDS; }

// t2 layout of a coupling (Coupling::t2_*): [mapped, floats per pixel of the image, gc, then per branch
// (slice offset of pixel 0, pixel stride, out_off, cout), then conv_b's quad map (gc / 4 pairs, mapped only)]
int cnf_debug_t2_layout(const cnf_plan* plan, int coupling, int* words, int cap) {
    OptScope os_(plan ? &plan->p->opts : nullptr);
    const Coupling* c = coupling_of(plan, coupling);
    if (!c || !words) return -1;
    return layout_words({c->t2_mapped ? 1 : 0, c->t2_cs, c->gc}, *c, c->t2_off, c->t2_pcs, &Branch::out_off,
                        &Branch::cout, c->t2_qmap, words, cap);
}

// t1 layout of a coupling (Coupling::t1_map): [compact, floats per pixel of the image, then per branch
// (window offset of pixel 0, pixel stride, cin_off, cin), then 128 words of t1_map (compact only)]
int cnf_debug_t1_layout(const cnf_plan* plan, int coupling, int* words, int cap) {
    OptScope os_(plan ? &plan->p->opts : nullptr);
    const Coupling* c = coupling_of(plan, coupling);
    if (!c || !words) return -1;
    return layout_words({c->t1_compact ? 1 : 0, c->t1_cs}, *c, c->t1_off, c->t1_pcs, &Branch::cin_off, &Branch::cin,
                        c->t1_map, words, cap);
}

// ---- the training backward's batch partitions (tests/test_batch_partitions.py) ---------------------------------
// Each answer comes from the host function the launch code itself calls (wgrad_choice and the wgrad_*_split
// shape functions, tconv_choice, lnb_slicing, grad_rows_trips); nothing is launched. plan: its debug options
// (TRAIN_ALT) decide as they do in a call; null: the defaults.

// The convolutions of coupling `coupling`'s multi-kernel backward (StreamedBwd) as words: [lds_bwd (the layer runs
// the fused k_lds_bwd + k_grad_rows instead), hc, wc, dc1, dc2, nk, gc, R, n, then n x TRAINCONV_WORDS: role
// (0 conv_out, 1 conv_b, 2 a grouped branch, 3 conv_a, 4 conv_in; residual blocks share their shapes), taps, dil,
// cin, cout, then the input window's (floats per pixel, channel offset) and the output window's]. The weight
// gradient reads X in the input window and dY in the output window; the data gradient maps cout channels of the
// output window to cin channels of a tensor laid out as the input window.
enum { TRAINCONV_WORDS = 9 };
int cnf_debug_train_convs(const cnf_plan* plan, int coupling, int* words, int cap) {
    const Coupling* c = coupling_of(plan, coupling);
    if (!c || !words) return -1;
    const NetParams& np = c->net[0];
    std::vector<int> w{c->lds_bwd ? 1 : 0, c->hc, c->wc, c->dc1, c->dc2, c->nk, c->gc, c->R, 0};
    auto conv = [&](int role, int taps, int dil, int cin, int cout, int x_cs, int x_off, int y_cs, int y_off) {
        for (int v : {role, taps, dil, cin, cout, x_cs, x_off, y_cs, y_off}) w.push_back(v);
        w[8]++;
    };
    conv(0, np.co.taps, 1, c->nk, c->dc2, c->nk, 0, c->dc2, 0);
    if (c->R > 0) {
        const RBParams& rb = np.rb[0];
        conv(1, rb.cb.taps, 1, c->gc, c->nk, c->gc, 0, c->nk, 0);
        for (size_t bi = 0; bi < c->br.size(); bi++) {
            const Branch& b = c->br[bi];
            conv(2, rb.gc[bi].taps, b.dil, b.cin, b.cout, c->nk, b.cin_off, c->gc, b.out_off);
        }
        conv(3, rb.ca.taps, 1, c->nk, c->nk, c->nk, 0, c->nk, 0);
    }
    conv(4, np.ci.taps, 1, c->dc1, c->nk, c->dc1, 0, c->nk, 0);
    if ((int)w.size() > cap) return -1;
    std::memcpy(words, w.data(), w.size() * sizeof(int));
    return (int)w.size();
}

// The weight-gradient kernel of a taps-tap convolution cin -> cout (dilation dil, X in a tensor of x_cs floats per
// pixel) on h x w images at batch B: [kernel (WGradKernel: 0 k_wgrad, 1 k_wgrad_thin, 2 k_wgrad_direct,
// 3 k_wgrad_band), chunks (partial rows), units, per_chunk, short_last (WGradSplit; for k_wgrad: units = chunks,
// per_chunk = chunk_px pixels of the flattened (image, pixel) axis, short_last = some chunk edge lies inside an
// image), passes of k_grad_scatter's chunk loop]
int cnf_debug_wgrad_choice(const cnf_plan* plan, int h, int w, int taps, int dil, int cin, int cout, int x_cs, int B,
                           int* words, int cap) {
    OptScope os_(plan ? &plan->p->opts : nullptr);
    if (!words || cap < 6 || h < 1 || w < 1 || cin < 1 || cout < 1 || B < 1) return -1;
    const WGradChoice k = wgrad_choice(B, h, w, taps, dil, cin, cout, x_cs, true);
    WGradSplit s{k.chunks, k.chunks, k.chunk_px, 0};
    if (k.kernel == WGRAD_THIN) s = wgrad_thin_split(B, h, w);
    if (k.kernel == WGRAD_DIRECT) s = wgrad_direct_split(B, h);
    if (k.kernel == WGRAD_BAND) s = wgrad_band_split(B, h, w, taps, cin, cout);
    if (k.kernel == WGRAD_VALU)
        for (long long e = k.chunk_px; e < (long long)B * h * w; e += k.chunk_px)
            if (e % (h * w) != 0) s.short_last = 1;
    if (s.chunks != k.chunks) return -1;   // (the launchers throw on the same mismatch)
    const int out[6] = {k.kernel, s.chunks, s.units, s.per_chunk, s.short_last, grad_scatter_trips(s.chunks)};
    std::memcpy(words, out, sizeof(out));
    return 6;
}

// The kernel of a data gradient (cout channels of a tensor with in_cs floats per pixel at channel in_off -> cin
// channels at out_off of one with out_cs; 16-byte aligned buffers, as the train workspace's are) on h x w images at
// batch B: [kernel (TConvKernel: 0 k_tconv, 1 k_tconv_thin, 2 k_tconv_band, 3 k_tconv_mfma), NR, SUB, TH,
// all_taps, row bands per image]
int cnf_debug_tconv_choice(const cnf_plan* plan, int h, int w, int taps, int dil, int cin, int cout, int in_cs,
                           int in_off, int out_cs, int out_off, int B, int* words, int cap) {
    OptScope os_(plan ? &plan->p->opts : nullptr);
    if (!words || cap < 6 || h < 1 || w < 1 || cin < 1 || cout < 1 || B < 1) return -1;
    TConvArgs a{};
    a.in_cs = in_cs;
    a.in_off = in_off;
    a.K = cout;
    a.out = reinterpret_cast<float*>(uintptr_t{256});   // (never dereferenced: its alignment alone is read)
    a.out_cs = out_cs;
    a.out_off = out_off;
    a.N = cin;
    a.H = h;
    a.W = w;
    a.taps = taps;
    a.dil = dil;
    a.sgn = -1;
    a.B = B;
    const TConvChoice c = tconv_choice(a);
    const bool rows = c.kernel == TCONV_THIN || c.kernel == TCONV_BAND;
    const int out[6] = {c.kernel, c.nr, c.sub, c.th, c.all_taps, rows ? (h + c.th - 1) / c.th : 0};
    std::memcpy(words, out, sizeof(out));
    return 6;
}

// launch_ln_backward's slicing of a B-image batch of n-element images: [S, bs, shared (1) or per-thread (0) sums,
// reduction partials per image of its own k_lnb_reduce]
int cnf_debug_lnb_slicing(long long n, int B, int* words, int cap) {
    if (!words || cap < 4 || n < 1 || B < 1) return -1;
    const LnbSlicing s = lnb_slicing(n, B);
    const int out[4] = {s.S, s.bs, s.shared, s.rsl};
    std::memcpy(words, out, sizeof(out));
    return 4;
}

// images per workgroup of a k_pw launch with the tiles_per_img, nprob and res of one of cnf_debug_pw_shapes' shapes
int cnf_debug_pw_ipw(int tiles_per_img, int nprob, int res, int B) {
    if (tiles_per_img < 1 || nprob < 1 || B < 1) return -1;
    return pw_images_per_wg(tiles_per_img, nprob, B, res != 0);
}

// passes of k_grad_rows' image loop at batch B
int cnf_debug_grad_rows_trips(int B) { return B < 1 ? -1 : grad_rows_trips(B); }

// ---- the density of given images (tests/test_log_prob_sweep.py) ------------------------------------------------
// What cnf_flow_log_prob launches for a chunk of n pairs on the plan's io shape, from the host functions the
// launch code itself calls (logp_gather_choice, logp_parts, logp_per_xcd, logp_finish_trips); nothing is launched.
// aligned: x, y and the workspace's xy are 16-byte aligned. Words: [gather kernel (LogpGatherKernel: 0
// k_logp_gather_any, 1 <1,1>, 2 <3,1>, 3 <3,3>), parts (tiles and log_jac slots per image), per_xcd, the gather's
// grid, k_logp_finish's trips over an image, threads of its last trip that hold a float4]
int cnf_debug_logp_choice(const cnf_plan* plan, int n, int aligned, int* words, int cap) {
    if (!plan || !words || cap < 6 || n < 1) return -1;
    const cnf_flow_desc& d = plan->p->desc;
    const int HW = d.io_h * d.io_w, parts = logp_parts(HW), per_xcd = logp_per_xcd(n, parts);
    const int out[6] = {logp_gather_choice(d.x_d, d.io_d - d.x_d, HW, aligned != 0), parts, per_xcd, per_xcd * 8,
                        logp_finish_trips(HW, d.io_d), logp_finish_last_trip(HW, d.io_d)};
    std::memcpy(words, out, sizeof(out));
    return 6;
}

// diagnostic builds: the phase stamps the kernels of the last stamped launch left
int cnf_debug_read_stamps(long long* out, int n) { return read_stamps(out, n); }
int cnf_debug_read_bwd_stamps(long long* out, int n) { return read_bwd_stamps(out, n); }
int cnf_debug_read_cycles(long long* out, int n) { return read_cycles(out, n); }
int cnf_debug_read_gc_stamps(long long* out, int n) { return read_gc_stamps(out, n); }
int cnf_debug_read_pw_stamps(long long* out) { return read_pw_stamps(out); }

int cnf_plan_num_recorded_launches(const cnf_plan* plan) { return plan ? (int)plan->p->recorded.size() : -1; }

int cnf_plan_recorded_launch_info(const cnf_plan* plan, int i, char* name, int name_cap, double* flops,
                                  double* bytes) {
    OptScope os_(plan ? &plan->p->opts : nullptr);
    if (!plan) return fail(CNF_E_INVALID, "null plan");
    const Plan& p = *plan->p;
    if (i < 0 || i >= (int)p.recorded.size()) return fail(CNF_E_INVALID, "launch index out of range");
    if (name && name_cap > 0) std::snprintf(name, (size_t)name_cap, "%s", p.recorded[i].name.c_str());
    if (flops) *flops = p.recorded[i].flops;
    if (bytes) *bytes = p.recorded[i].bytes;
    return CNF_OK;
}

int cnf_plan_set_launch_timing(cnf_plan* plan, int on) {
    OptScope os_(plan ? &plan->p->opts : nullptr);
    if (!plan) return fail(CNF_E_INVALID, "null plan");
    plan->p->timing = on != 0;
    return CNF_OK;
}

int cnf_plan_launch_time_ms(const cnf_plan* plan, int i, float* ms) {
    OptScope os_(plan ? &plan->p->opts : nullptr);
    if (!plan || !ms) return fail(CNF_E_INVALID, "null argument");
    const Plan& p = *plan->p;
    if (i < 0 || i >= (int)p.recorded.size()) return fail(CNF_E_INVALID, "launch index out of range");
    if (!p.recorded[i].timed) {   // not a kernel (a copy), or the call ran without launch timing
        *ms = 0.f;
        return CNF_OK;
    }
    CNF_TRY
    hip_check(hipEventSynchronize(p.ev[2 * i + 1]), "hipEventSynchronize");
    hip_check(hipEventElapsedTime(ms, p.ev[2 * i], p.ev[2 * i + 1]), "hipEventElapsedTime");
    return CNF_OK;
    CNF_CATCH
}

int64_t cnf_plan_weight_map(const cnf_plan* plan, int which, int64_t* out, int64_t cap) {
    OptScope os_(plan ? &plan->p->opts : nullptr);
    if (!plan || which < 0 || which > 3) return fail(CNF_E_INVALID, "null plan or which not in {0, 1, 2, 3}");
    const Plan& pl = *plan->p;
    const std::vector<int64_t>& m = which == 0 ? pl.aux_map : which == 1 ? pl.bw_map : which == 2 ? pl.x6_map : pl.x6_dir;
    if (out)
        for (int64_t i = 0; i < std::min<int64_t>(cap, (int64_t)m.size()); i++) out[i] = m[i];
    return (int64_t)m.size();
}

int cnf_plan_relaunch(cnf_plan* plan, int i, void* stream) {
    OptScope os_(plan ? &plan->p->opts : nullptr);
    if (!plan) return fail(CNF_E_INVALID, "null plan");
    Plan& p = *plan->p;
    if (i < 0 || i >= (int)p.recorded.size()) return fail(CNF_E_INVALID, "launch index out of range");
    CNF_TRY
    p.recorded[i].relaunch(stream);
    check_launch();
    return CNF_OK;
    CNF_CATCH
}

}  // extern "C"
