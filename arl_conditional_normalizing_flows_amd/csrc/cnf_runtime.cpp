// cnf_runtime.cpp — plan execution and the C ABI of libcnf_hip.so (include/cnf.h).
//
// Executes the layer schedule of cFlow.call (conv_cINN_make_model.py:1723-1798) as a fixed
// sequence of coupling layers (cnf_coupling.cpp) and map launches on the caller's stream. All memory
// is the caller's (params, aux, workspace); the plan owns only its index tables.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>

#include "../../include/cnf.h"
#include "cnf_kernels.h"
#include "cnf_plan.h"

struct cnf_plan {
    cnf::Plan* p;
};

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

struct HipError : std::runtime_error {
    using std::runtime_error::runtime_error;
};

void hip_check(hipError_t e, const char* what) {
    if (e != hipSuccess) throw HipError(std::string(what) + ": " + hipGetErrorString(e));
}

#define CNF_TRY try {
#define CNF_CATCH                                                   \
    }                                                               \
    catch (const std::invalid_argument& e) {                        \
        return fail(CNF_E_INVALID, e.what());                       \
    }                                                               \
    catch (const HipError& e) {                                     \
        return fail(CNF_E_HIP, e.what());                           \
    }                                                               \
    catch (const std::exception& e) {                               \
        return fail(CNF_E_STATE, e.what());                         \
    }                                                               \
    catch (...) {                                                   \
        return fail(CNF_E_STATE, "unknown error");                  \
    }

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

}  // namespace

namespace cnf {

// error reporting for the entry points defined outside this file (cnf_transforms.hip)
int set_error(int code, const char* msg) { return fail(code, msg); }

// ----------------------------------------------------------------------------------------------
// debug options (cnf_flow_desc.debug_options)
// ----------------------------------------------------------------------------------------------
Options parse_options(const char* s) {
    Options o;
    if (s == nullptr) return o;
    struct Field {
        const char* name;
        int Options::*f;
    };
    static const Field fields[] = {{"NETLDS", &Options::netlds},           {"GC", &Options::gc},
                                   {"PW", &Options::pw},                   {"GENERIC", &Options::generic},
                                   {"LAYOUT", &Options::layout},           {"FUSE_COUPLING", &Options::fuse_coupling},
                                   {"LDS_BWD", &Options::lds_bwd},         {"TRAIN_ALT", &Options::train_alt},
                                   {"TRAIN_SCHED", &Options::train_sched}, {"SCHEDULE_CHECK", &Options::schedule_check},
                                   {"PRESPLIT", &Options::presplit}};
    std::string str(s);
    size_t pos = 0;
    while (pos < str.size()) {
        size_t end = str.find(',', pos);
        if (end == std::string::npos) end = str.size();
        const std::string item = str.substr(pos, end - pos);
        pos = end + 1;
        if (item.empty()) continue;
        const size_t eq = item.find('=');
        if (eq == std::string::npos) throw std::invalid_argument("debug_options: expected NAME=VALUE, got '" + item + "'");
        const std::string key = item.substr(0, eq), val = item.substr(eq + 1);
        char* endp = nullptr;
        const long v = std::strtol(val.c_str(), &endp, 10);
        if (val.empty() || *endp != '\0') throw std::invalid_argument("debug_options: bad value in '" + item + "'");
        bool found = false;
        for (const Field& f : fields)
            if (key == f.name) {
                o.*(f.f) = (int)v;
                found = true;
            }
        if (!found) throw std::invalid_argument("debug_options: unknown option '" + key + "'");
    }
    if (o.lds_bwd < 0 || o.lds_bwd > 2) throw std::invalid_argument("debug_options: LDS_BWD is 0, 1 or 2");
    if (o.presplit < 0 || o.presplit > 1) throw std::invalid_argument("debug_options: PRESPLIT is 0 or 1");
    return o;
}

namespace {
thread_local const Options* g_opts = nullptr;
const Options kDefaultOptions{};
}  // namespace
const Options& opts() { return g_opts != nullptr ? *g_opts : kDefaultOptions; }
OptScope::OptScope(const Options* o) : prev(g_opts) {
    if (o != nullptr) g_opts = o;
}
OptScope::~OptScope() { g_opts = prev; }

LaunchTiming& launch_timing() {
    thread_local LaunchTiming t;
    return t;
}

WsLayout Plan::layout(int B) const {
    WsLayout L;
    int64_t n_uv = (int64_t)desc.io_h * desc.io_w * desc.io_d;
    int64_t n_u1c = 0, n_y = 0, n_t2 = 0, n_so = 0;
    int parts = 1, ldp = 1;
    for (const auto& c : couplings) {
        int64_t npx = (int64_t)c.hc * c.wc;
        n_u1c = std::max<int64_t>(n_u1c, npx * c.dc1);
        n_y = std::max<int64_t>(n_y, npx * c.nk);
        n_t2 = std::max<int64_t>(n_t2, npx * c.gc);
        n_so = std::max<int64_t>(n_so, npx * c.dc2);
        // LN partial slots: the 1x1 launches as either kernel, and the grouped stage (whose bound also
        // covers a k_conv3 problem of conv_in)
        parts = std::max(parts, std::max(ln_slots_pw(c.hc, c.wc), ln_slots_conv1(c.hc, c.wc)));
        parts = std::max(parts, ln_slots_grouped(c));
        ldp = std::max(ldp, ld_parts_for((int)npx));
    }
    L.n_uv = n_uv;
    L.n_u1c = n_u1c;
    L.n_y = n_y;
    L.n_t2 = n_t2;
    L.n_so = n_so;
    L.st_parts = parts;
    L.ld_parts = ldp;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        size_t o = off;
        off = align_up(off + bytes, 256);
        return o;
    };
    const size_t Bz = (size_t)B;
    L.uv[0] = take(Bz * n_uv * 4);
    L.uv[1] = take(Bz * n_uv * 4);
    L.u1c = take(Bz * n_u1c * 4);
    for (int n = 0; n < 2; n++) {
        L.y[n] = take(Bz * n_y * 4);
        L.t1[n] = take(Bz * n_y * 4);
        L.t2[n] = take(Bz * n_t2 * 4);
        L.so[n] = take(Bz * n_so * 4);
        L.so_alt[n] = take(Bz * n_so * 4);
        for (int k = 0; k < 3; k++) {   // LN slabs y, t1, t2: per-wave partials
            L.st_part[n][k] = take(Bz * parts * LNP * 4);
        }
    }

    L.ld = take(std::max<size_t>(1, couplings.size()) * Bz * ldp * 8);
    L.total = off;
    return L;
}

static void ensure_tables(Plan& p) {
    int dev = 0;
    hip_check(hipGetDevice(&dev), "hipGetDevice");
    if (p.dev_table != nullptr && p.device == dev) return;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    // uploading is not capturable: the first call on a device must run eagerly
    if (hipStreamIsCapturing(nullptr, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
        throw std::runtime_error("plan tables not uploaded yet (call cnf_pack_params before graph capture)");
    // NLL_SLOTS ints past the table: cnf_nll's completion counters (zero between launches)
    size_t nb = (p.host_table.size() + Plan::NLL_SLOTS) * sizeof(int);
    hip_check(hipMalloc(&p.dev_table, nb), "hipMalloc(table)");
    hip_check(hipMemset(p.dev_table, 0, nb), "hipMemset(table)");
    if (!p.host_table.empty())
        hip_check(hipMemcpy(p.dev_table, p.host_table.data(), p.host_table.size() * sizeof(int), hipMemcpyHostToDevice),
                  "hipMemcpy(table)");
    // (the fp32 part of the kernel image: the plane region behind it has a map of its own)
    size_t na = std::max<size_t>(1, (size_t)p.x6_base) * sizeof(int64_t);
    hip_check(hipMalloc(&p.dev_aux_map, na), "hipMalloc(aux map)");
    if (p.x6_base > 0)
        hip_check(hipMemcpy(p.dev_aux_map, p.aux_map.data(), (size_t)p.x6_base * sizeof(int64_t), hipMemcpyHostToDevice),
                  "hipMemcpy(aux map)");
    size_t nx = std::max<size_t>(1, p.x6_map.size()) * sizeof(int64_t);
    hip_check(hipMalloc(&p.dev_x6_map, nx), "hipMalloc(plane map)");
    if (!p.x6_map.empty())
        hip_check(hipMemcpy(p.dev_x6_map, p.x6_map.data(), p.x6_map.size() * sizeof(int64_t), hipMemcpyHostToDevice),
                  "hipMemcpy(plane map)");
    size_t nbw = std::max<size_t>(1, p.bw_map.size()) * sizeof(int64_t);
    hip_check(hipMalloc(&p.dev_bw_map, nbw), "hipMalloc(bw map)");
    if (!p.bw_map.empty())
        hip_check(hipMemcpy(p.dev_bw_map, p.bw_map.data(), p.bw_map.size() * sizeof(int64_t), hipMemcpyHostToDevice),
                  "hipMemcpy(bw map)");
    p.device = dev;
}

static void check_launch() { hip_check(hipGetLastError(), "kernel launch"); }

}  // namespace cnf

using namespace cnf;

// host-only dry run of the B-image forward (direction +1), inverse (-1) or inverse-with-log-det (-2) schedule: nothing is launched or
// dereferenced, the launch names land in p.dry_launches; throws what the real call would throw before its
// first launch (defined after the schedules, below)
static void dry_run(Plan& p, int B, int direction);

// ================================================================================================
// C ABI
// ================================================================================================
extern "C" {

const char* cnf_last_error(void) { return g_err.c_str(); }
const char* cnf_version(void) { return "cnf-mi355x 0.1 (gfx950)"; }

int cnf_plan_create(const cnf_flow_desc* desc, cnf_plan** out) {
    if (!out) return fail(CNF_E_INVALID, "null out");
    *out = nullptr;
    CNF_TRY
    std::unique_ptr<Plan> owner(build_plan(desc));   // (the reference's asserts; parses desc->debug_options into p->opts)
    Plan* p = owner.get();
    OptScope os(&p->opts);
    p->use_pw = p->tap_pw = p->opts.pw != 0;
    // validate tiling / LDS budget for every layer up-front
    for (const auto& c : p->couplings) (void)conv_geo(c.hc, c.wc);
    // training: k_net_lds layers whose fused backward fits LDS use it (debug option LDS_BWD=0: none)
    const bool lds_bwd = p->opts.lds_bwd != 0;
    for (auto& c : p->couplings) {
        LdsBwdArgs a;
        c.lds_bwd = lds_bwd && c.use_lds && ldsbwd_setup(*p, c, a) > 0;
    }
    // a created plan can be scheduled: what the forward or the inverse schedule cannot run (a streamed conv
    // with more than 64 output channels, a tile over the LDS budget, ...) fails here, like the reference's
    // asserts, with the schedule's own message -- not on the first batch. One image, and a batch whose
    // image-looping launches are sized differently. (Debug option SCHEDULE_CHECK=0: plan tables only, the
    // default for group_mode 'intended' through the C ABI; cFlow asks for the check in either mode.)
    const int sc = p->opts.schedule_check;
    if (sc < 0 ? desc->group_mode == CNF_GROUP_REFERENCE : sc != 0)
        for (int B : {1, 3})
            for (int dir : {+1, -1}) dry_run(*p, B, dir);
    p->dry_launches.clear();
    p->pw_shapes.clear();
    p->gc_launch.clear();
    *out = new cnf_plan{owner.release()};
    return CNF_OK;
    CNF_CATCH
}

void cnf_plan_destroy(cnf_plan* plan) {
    if (!plan) return;
    if (plan->p) {
        if (plan->p->dev_table) (void)hipFree(plan->p->dev_table);
        if (plan->p->dev_aux_map) (void)hipFree(plan->p->dev_aux_map);
        if (plan->p->dev_x6_map) (void)hipFree(plan->p->dev_x6_map);
        if (plan->p->dev_bw_map) (void)hipFree(plan->p->dev_bw_map);
        for (hipEvent_t e : plan->p->ev) (void)hipEventDestroy(e);
        if (plan->p->ev_fork) (void)hipEventDestroy(plan->p->ev_fork);
        if (plan->p->ev_join) (void)hipEventDestroy(plan->p->ev_join);
        if (plan->p->side) (void)hipStreamDestroy(plan->p->side);
        for (hipStream_t s : plan->p->wside)
            if (s) (void)hipStreamDestroy(s);
        for (hipEvent_t e : plan->p->tev) (void)hipEventDestroy(e);
        for (hipEvent_t e : plan->p->nll_ev)
            if (e) (void)hipEventDestroy(e);
        delete plan->p;
    }
    delete plan;
}

int cnf_plan_num_layers(const cnf_plan* plan) { return plan ? (int)plan->p->layers.size() : -1; }

int cnf_plan_layer_info(const cnf_plan* plan, int layer, cnf_layer_info* out) {
    OptScope os_(plan ? &plan->p->opts : nullptr);
    if (!plan || !out) return fail(CNF_E_INVALID, "null argument");
    const Plan& p = *plan->p;
    if (layer < 0 || layer >= (int)p.layers.size()) return fail(CNF_E_INVALID, "layer index out of range");
    std::memset(out, 0, sizeof(*out));
    const Layer& L = p.layers[layer];
    out->kind = L.kind;
    out->coupling_index = L.ci;
    out->block = L.block;
    out->h = L.h;
    out->w = L.w;
    out->d = L.d;
    out->num_prev_factors = L.npf;
    if (L.kind == CNF_LAYER_COUPLING) {
        out->fused_net = p.couplings[L.ci].use_lds ? 1 : 0;
        const Coupling& c = p.couplings[L.ci];
        out->mask = c.mask;
        out->hc = c.hc;
        out->wc = c.wc;
        out->dc1 = c.dc1;
        out->dc2 = c.dc2;
        out->num_kernels = c.nk;
        out->cardinality = c.card;
        out->num_res_blocks = c.R;
        out->num_dilations = (int)c.dils.size();
        for (int i = 0; i < (int)c.dils.size() && i < 8; i++) out->dilations[i] = c.dils[i];
    }
    return CNF_OK;
}

int64_t cnf_plan_num_params(const cnf_plan* plan) { return plan ? plan->p->n_params : -1; }
int cnf_plan_num_param_tensors(const cnf_plan* plan) { return plan ? (int)plan->p->params.size() : -1; }

int cnf_plan_param_tensor(const cnf_plan* plan, int index, char* name, int name_cap, int64_t* offset, int* ndim,
                          int shape[4]) {
    OptScope os_(plan ? &plan->p->opts : nullptr);
    if (!plan) return fail(CNF_E_INVALID, "null plan");
    const Plan& p = *plan->p;
    if (index < 0 || index >= (int)p.params.size()) return fail(CNF_E_INVALID, "param index out of range");
    const ParamTensor& t = p.params[index];
    if (name && name_cap > 0) {
        std::snprintf(name, (size_t)name_cap, "%s", t.name.c_str());
    }
    if (offset) *offset = t.offset;
    if (ndim) *ndim = (int)t.shape.size();
    if (shape)
        for (int i = 0; i < 4; i++) shape[i] = i < (int)t.shape.size() ? t.shape[i] : 0;
    return CNF_OK;
}

int64_t cnf_plan_aux_floats(const cnf_plan* plan) { return plan ? std::max<int64_t>(1, plan->p->n_aux) : -1; }

int cnf_pack_params(cnf_plan* plan, const float* params, float* aux, void* stream) {
    OptScope os_(plan ? &plan->p->opts : nullptr);
    if (!plan || !params || !aux) return fail(CNF_E_INVALID, "null argument");
    CNF_TRY
    Plan& p = *plan->p;
    ensure_tables(p);
    if (p.x6_base > 0) launch_pack(params, p.dev_aux_map, aux, (long long)p.x6_base, (hipStream_t)stream);
    // the streamed convs' bf16x6 planes (and k_gc's K-octet tables): split here, once per weight update
    if (!p.x6_map.empty())
        launch_pack_x6(params, p.dev_x6_map, aux + p.x6_base, (long long)p.x6_map.size(), (hipStream_t)stream);
    check_launch();
    return CNF_OK;
    CNF_CATCH
}

size_t cnf_plan_workspace_bytes(const cnf_plan* plan, int B) {
    OptScope os_(plan ? &plan->p->opts : nullptr);
    if (!plan || B <= 0) return 0;
    return plan->p->layout(B).total;
}

}  // extern "C"

// the layer after li in schedule order (step +1: forward, -1: inverse) that launches anything: squeezes
// are folded into the factor maps
struct NextLaunch {
    const Coupling* coupling = nullptr;   // a coupling layer
    bool maps = false, end = false;       // a factor boundary (k_map2); nothing: the schedule's tail follows
};
static NextLaunch next_launch(const Plan& p, int li, int step) {
    const int n = (int)p.layers.size();
    int nx = li + step;
    while (nx >= 0 && nx < n && p.layers[nx].kind == CNF_LAYER_SQUEEZE) nx += step;
    NextLaunch r;
    if (nx < 0 || nx >= n)
        r.end = true;
    else if (p.layers[nx].kind == CNF_LAYER_COUPLING)
        r.coupling = &p.couplings[p.layers[nx].ci];
    else
        r.maps = p.layers[nx].kind == CNF_LAYER_FACTOR;
    return r;
}

// A k_net_lds layer leaves its coupling law (CoupPend) to the next launch when that is another
// k_net_lds or the boundary maps; the forward's tail (its final k_map2) applies one too, the inverse
// ends in the layer that writes xy. Debug option FUSE_COUPLING=0: a k_coupling per layer.
static bool defers(const Plan& p, const Coupling& c, int li, int step) {
    if (p.opts.fuse_coupling == 0 || !c.use_lds) return false;
    const NextLaunch nx = next_launch(p, li, step);
    return (nx.coupling != nullptr && nx.coupling->use_lds) || nx.maps || (nx.end && step > 0);
}

// the forward schedule; save_inputs: also copy every coupling layer's input into the training
// workspace (cnf_flow_forward_train)
// nz (cnf_flow_forward_noise): xy is the caller's buffer for the noisy input, which the first coupling's
// k_net_lds writes while gathering from nz->src with the noise applied (a k_noise pass into it first when
// that layer is streamed)
static void flow_forward(Plan& p, const float* params, const float* aux, const float* xy, float* zy,
                         float* logdet_per_image, void* workspace, int B, hipStream_t stream, bool save_inputs,
                         const InputPrepArgs* nz = nullptr) {
    if (!p.dry) ensure_tables(p);
    p.recorded.clear();
    Exec E{p, params, aux, (char*)workspace, p.layout(B), B, stream};
    TrainLayout TL;
    if (save_inputs) TL = p.train_layout(B);
    const WsLayout& L = E.L;
    double* ld = E.at<double>(L.ld);
    float* buf[2] = {E.at<float>(L.uv[0]), E.at<float>(L.uv[1])};
    const float* cur = xy;
    int which = 0;
    size_t bi = 0;
    const int nuv = (int)L.n_uv;
    const bool nz_fused = nz != nullptr && !save_inputs && !p.layers.empty() &&
                          p.layers[0].kind == CNF_LAYER_COUPLING && p.couplings[p.layers[0].ci].use_lds;
    if (nz != nullptr && !nz_fused) {
        const InputPrepArgs q = *nz;
        float* dst = const_cast<float*>(xy);
        const long long n = (long long)B * p.desc.io_h * p.desc.io_w * p.desc.io_d;
        E.record("k_prep", 0, 8.0 * n, [=](void* st) { launch_input_prep(dst, n, q, (hipStream_t)st); });
    }
    // a k_net_lds layer followed directly by another one leaves its coupling law to that layer's
    // kernel (CoupPend): no k_coupling launch for it. Not when saving layer inputs (training).
    CoupPend pend;
    bool have_pend = false;
    // training: a layer whose output is the next coupling's input writes it straight into that coupling's
    // save slot (no copy of every layer input; only the first coupling's, which reads xy)
    auto save_slot_after = [&](size_t li) -> float* {
        const NextLaunch nx = next_launch(p, (int)li, +1);
        if (!save_inputs || nx.coupling == nullptr) return nullptr;
        return E.at<float>(TL.save_u[nx.coupling->index]);
    };
    for (size_t li = 0; li < p.layers.size(); li++) {
        const Layer& ly = p.layers[li];
        if (ly.kind == CNF_LAYER_COUPLING) {
            const Coupling& c = p.couplings[ly.ci];
            const bool defer = !save_inputs && defers(p, c, (int)li, +1);
            float* nxt = buf[which];
            if (float* slot = save_slot_after(li)) nxt = slot;
            if (save_inputs && cur != E.at<float>(TL.save_u[c.index])) {
                float* dst = E.at<float>(TL.save_u[c.index]);
                const float* src = cur;
                const size_t bytes = (size_t)B * c.H * c.W * c.D * 4;
                E.record("copy", 0, 2.0 * bytes, [=](void* st) {
                    (void)hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, (hipStream_t)st);
                });
            }
            CoupPend next;
            CouplingOpts o;
            o.pend = have_pend ? &pend : nullptr;
            o.defer = defer;
            o.out_pend = &next;
            o.nz = nz_fused && li == 0 ? nz : nullptr;
            float* so_save[2] = {nullptr, nullptr};
            if (save_inputs && c.lds_bwd) {   // the fused LDS backward's activations
                o.save = E.at<float>(TL.act_save[c.index]);
                so_save[0] = E.at<float>(TL.so_save[c.index]);
            }
            if (save_inputs && !c.use_lds && TL.has_ssave[c.index]) {
                o.ss = &TL.ssave[c.index];
                so_save[0] = E.at<float>(o.ss->so);   // the raw conv_out (k_coupling's so_w in tap mode) into the save area
            }
            if (o.save != nullptr || o.ss != nullptr) {
                so_save[1] = so_save[0] + (size_t)B * c.hc * c.wc * c.dc2;
                o.so_save = so_save;
            }
            run_coupling(E, c, cur, nxt, ld + (size_t)c.index * B * L.ld_parts, +1, o);
            pend = next;
            have_pend = defer;
            cur = nxt;
            which ^= 1;
        } else if (ly.kind == CNF_LAYER_FACTOR) {
            // squeeze (:179) + factor (:276-286) at a block boundary: kept half -> next buffer,
            // factored half -> its final xy-layout position in zy (:1762-1770 restoration).
            const Boundary& b = p.boundaries[bi++];
            // with a pending coupling the maps read u_k (the other buffer) on the fly, and v_k's
            // own buffer (cur, never written) takes the kept half
            float* nxt = have_pend ? const_cast<float*>(cur) : buf[which];
            if (!have_pend)
                if (float* slot = save_slot_after(li)) nxt = slot;
            const bool flip = !have_pend;
            const int* T = p.dtab(0);
            const float* src = cur;
            const int ncur = b.n_cur, nnext = b.n_next, nfac = b.n_fac;
            const int* ks = T + b.dev_keep_src;
            const int* fs = T + b.dev_fac_src;
            const int* fo = T + b.dev_fac_orig;
            // keep gather -> next buffer and factored scatter -> zy: one launch (reading v of a
            // pending coupling on the fly, with that layer's log-det partials)
            MapOp mk, mf;
            mk.src = src, mk.dst = nxt, mk.sidx = ks, mk.n = nnext, mk.ss = ncur, mk.ds = nnext;
            mf.src = src, mf.dst = zy, mf.sidx = fs, mf.didx = fo, mf.n = nfac, mf.ss = ncur, mf.ds = nuv;
            const CoupPend q = have_pend ? pend : CoupPend{};
            mk.pend = mf.pend = q.on;
            if (!p.dry && q.on && (nxt == q.u || zy == q.u)) throw std::logic_error("k_map2 would overwrite the u_k it reads");
            have_pend = false;
            E.record("k_map2", 0, 8.0 * B * (nnext + nfac),
                     [=](void* st) { launch_map2(mk, mf, LdReduce{}, q, B, (hipStream_t)st); });
            cur = nxt;
            if (flip) which ^= 1;
        }
    }
    {
        // final scatter (restore to xy's layout) and the per-image log-det reduction: one launch
        MapOp mf;
        mf.src = cur, mf.dst = zy, mf.didx = p.dtab(p.dev_final_orig), mf.n = p.last_n, mf.ss = p.last_n;
        mf.ds = nuv;
        LdReduce r;
        r.part = ld, r.out = logdet_per_image, r.nl = (int)p.couplings.size(), r.np = L.ld_parts, r.accumulate = 0;
        const CoupPend q = have_pend ? pend : CoupPend{};
        mf.pend = q.on;
        if (have_pend) r.nl -= 1;   // the pending layer is the last one: its log-det sum goes straight into the total
        E.record("k_map2", 0, 8.0 * B * p.last_n, [=](void* st) { launch_map2(mf, MapOp{}, r, q, B, (hipStream_t)st); });
    }
    if (!p.dry) check_launch();
}

extern "C" {

int cnf_flow_forward(cnf_plan* plan, const float* params, const float* aux, const float* xy, float* zy,
                     float* logdet_per_image, void* workspace, int B, void* stream) {
    OptScope os_(plan ? &plan->p->opts : nullptr);
    if (!plan || !params || !aux || !xy || !zy || !logdet_per_image || !workspace || B <= 0)
        return fail(CNF_E_INVALID, "null argument or B <= 0");
    if (xy == zy) return fail(CNF_E_INVALID, "xy and zy must not alias (out-of-place only)");
    CNF_TRY
    flow_forward(*plan->p, params, aux, xy, zy, logdet_per_image, workspace, B, (hipStream_t)stream, false);
    return CNF_OK;
    CNF_CATCH
}

int cnf_flow_forward_noise(cnf_plan* plan, const float* params, const float* aux, const float* xy, float logit_a,
                           float alpha, uint64_t seed, uint64_t offset, float* xy_noisy, float* zy,
                           float* logdet_per_image, void* workspace, int B, void* stream) {
    OptScope os_(plan ? &plan->p->opts : nullptr);
    if (!plan || !params || !aux || !xy || !xy_noisy || !zy || !logdet_per_image || !workspace || B <= 0)
        return fail(CNF_E_INVALID, "null argument or B <= 0");
    if (xy == zy || xy_noisy == zy || xy_noisy == xy)
        return fail(CNF_E_INVALID, "xy, xy_noisy and zy must not alias (out-of-place only)");
    if (logit_a != 0.f && !(logit_a > 0.f && logit_a < 0.5f))
        return fail(CNF_E_INVALID, "logit_a must be 0 (no logit map) or in (0, 0.5)");
    CNF_TRY
    InputPrepArgs nz;
    std::memset(&nz, 0, sizeof(nz));
    nz.src = xy;
    nz.alpha = alpha;
    nz.seed = seed;
    nz.off = offset;
    nz.logit = logit_a != 0.f ? 1 : 0;
    nz.x_d = plan->p->desc.x_d;
    nz.D = plan->p->desc.io_d;
    if (nz.logit) nz.lk = logit_consts(logit_a);
    flow_forward(*plan->p, params, aux, xy_noisy, zy, logdet_per_image, workspace, B, (hipStream_t)stream, false, &nz);
    return CNF_OK;
    CNF_CATCH
}

size_t cnf_plan_train_workspace_bytes(const cnf_plan* plan, int B) {
    OptScope os_(plan ? &plan->p->opts : nullptr);
    if (!plan || B <= 0) return 0;
    try {
        return plan->p->train_layout(B).total;
    } catch (...) {
        return 0;
    }
}

int cnf_flow_forward_train(cnf_plan* plan, const float* params, const float* aux, const float* xy, float* zy,
                           float* logdet_per_image, void* train_workspace, int B, void* stream) {
    OptScope os_(plan ? &plan->p->opts : nullptr);
    if (!plan || !params || !aux || !xy || !zy || !logdet_per_image || !train_workspace || B <= 0)
        return fail(CNF_E_INVALID, "null argument or B <= 0");
    if (xy == zy) return fail(CNF_E_INVALID, "xy and zy must not alias (out-of-place only)");
    CNF_TRY
    flow_forward(*plan->p, params, aux, xy, zy, logdet_per_image, train_workspace, B, (hipStream_t)stream, true);
    return CNF_OK;
    CNF_CATCH
}

int cnf_flow_backward(cnf_plan* plan, const float* params, const float* xy, const float* zy, void* train_workspace,
                      int B, float inv_batch, float* dparams, void* stream) {
    OptScope os_(plan ? &plan->p->opts : nullptr);
    if (!plan || !params || !xy || !zy || !train_workspace || !dparams || B <= 0)
        return fail(CNF_E_INVALID, "null argument or B <= 0");
    CNF_TRY
    Plan& p = *plan->p;
    ensure_tables(p);
    flow_backward(p, params, xy, zy, train_workspace, B, inv_batch, dparams, (hipStream_t)stream);
    return CNF_OK;
    CNF_CATCH
}

int cnf_flow_backward_ex(cnf_plan* plan, const float* params, const float* xy, const float* zy, void* train_workspace,
                         int B, const float* global_count, float* dparams, cnf_layer_done_fn layer_done, void* user,
                         void* stream) {
    OptScope os_(plan ? &plan->p->opts : nullptr);
    if (!plan || !params || !xy || !zy || !train_workspace || !dparams || !global_count || B <= 0)
        return fail(CNF_E_INVALID, "null argument or B <= 0");
    CNF_TRY
    Plan& p = *plan->p;
    ensure_tables(p);
    flow_backward(p, params, xy, zy, train_workspace, B, 0.f, dparams, (hipStream_t)stream, global_count, layer_done,
                  user);
    return CNF_OK;
    CNF_CATCH
}

int cnf_coupling_backward(cnf_plan* plan, int layer, const float* params, const float* u, const float* dv, float* du,
                          float dlogdet, void* train_workspace, int B, float* dparams, void* stream) {
    OptScope os_(plan ? &plan->p->opts : nullptr);
    if (!plan || !params || !u || !dv || !du || !train_workspace || !dparams || B <= 0)
        return fail(CNF_E_INVALID, "null argument or B <= 0");
    CNF_TRY
    Plan& p = *plan->p;
    if (layer < 0 || layer >= (int)p.layers.size() || p.layers[layer].kind != CNF_LAYER_COUPLING)
        return fail(CNF_E_INVALID, "layer is not a coupling layer");
    if (du == dv || du == u) return fail(CNF_E_INVALID, "du must not alias u or dv");
    ensure_tables(p);
    coupling_layer_backward(p, p.layers[layer].ci, params, u, dv, du, dlogdet, train_workspace, B, dparams,
                            (hipStream_t)stream);
    return CNF_OK;
    CNF_CATCH
}

int cnf_adam_step(float* params, const float* grads, float* m, float* v, int64_t n, float lr, float beta_1,
                  float beta_2, float epsilon, int step, void* stream) {
    if (!params || !grads || !m || !v || n < 0 || step < 1) return fail(CNF_E_INVALID, "bad argument");
    CNF_TRY
    const double b1t = std::pow((double)beta_1, step), b2t = std::pow((double)beta_2, step);
    const float alpha = (float)((double)lr * std::sqrt(1.0 - b2t) / (1.0 - b1t));
    if (n > 0) launch_adam(params, grads, m, v, (long long)n, alpha, beta_1, beta_2, epsilon, (hipStream_t)stream);
    check_launch();
    return CNF_OK;
    CNF_CATCH
}

// append: keep the launches recorded so far (cnf_flow_sample records one inverse per chunk)
// logdet_per_image (may be null): every coupling's law also writes its log-det partial slots, reduced per
// image into -(sum of s); ld_slots: the slots are written and left to the caller (cnf_flow_sample_logp)
static void flow_inverse(Plan& p, const float* params, const float* aux, const float* zy, float* xy, void* workspace,
                         int B, hipStream_t stream, bool append = false, float* logdet_per_image = nullptr,
                         bool ld_slots = false);

int cnf_flow_inverse(cnf_plan* plan, const float* params, const float* aux, const float* zy, float* xy,
                     void* workspace, int B, void* stream) {
    OptScope os_(plan ? &plan->p->opts : nullptr);
    if (!plan || !params || !aux || !xy || !zy || !workspace || B <= 0)
        return fail(CNF_E_INVALID, "null argument or B <= 0");
    if (xy == zy) return fail(CNF_E_INVALID, "zy and xy must not alias (out-of-place only)");
    CNF_TRY
    flow_inverse(*plan->p, params, aux, zy, xy, workspace, B, (hipStream_t)stream);
    return CNF_OK;
    CNF_CATCH
}

int cnf_flow_inverse_logdet(cnf_plan* plan, const float* params, const float* aux, const float* zy, float* xy,
                            float* logdet_per_image, void* workspace, int B, void* stream) {
    OptScope os_(plan ? &plan->p->opts : nullptr);
    if (!plan || !params || !aux || !xy || !zy || !logdet_per_image || !workspace || B <= 0)
        return fail(CNF_E_INVALID, "null argument or B <= 0");
    if (xy == zy) return fail(CNF_E_INVALID, "zy and xy must not alias (out-of-place only)");
    CNF_TRY
    flow_inverse(*plan->p, params, aux, zy, xy, workspace, B, (hipStream_t)stream, false, logdet_per_image);
    return CNF_OK;
    CNF_CATCH
}

}  // extern "C"

// cFlow.call(zy, -1) (:1774-1798) as a launch schedule
static void flow_inverse(Plan& p, const float* params, const float* aux, const float* zy, float* xy, void* workspace,
                         int B, hipStream_t stream, bool append, float* logdet_per_image, bool ld_slots) {
    if (!p.dry) ensure_tables(p);
    if (!append) p.recorded.clear();
    Exec E{p, params, aux, (char*)workspace, p.layout(B), B, stream};
    const WsLayout& L = E.L;
    // log-det slots [couplings][B][ld_parts], as the forward's: each coupling's block is written once, by
    // the kernel that applies its law (k_coupling, the next k_net_lds, or the boundary k_map2)
    double* ld = logdet_per_image != nullptr || ld_slots ? E.at<double>(L.ld) : nullptr;
    float* buf[2] = {E.at<float>(L.uv[0]), E.at<float>(L.uv[1])};
    const int nuv = (int)L.n_uv;
    const int* T = p.dtab(0);
    // squeeze/factor forward on zy (:1784-1788) == gather of the last block layout from xy positions
    int which = 0;
    {
        float* dst = buf[which];
        const int off = p.dev_final_orig, n = p.last_n;
        E.record("k_map_gather", 0, 8.0 * B * n,
                 [=](void* st) { launch_map_gather(zy, dst, T + off, n, nuv, n, B, (hipStream_t)st); });
    }
    const float* cur = buf[which];
    which ^= 1;
    // the first layer that launches anything (squeezes are folded into the boundary maps): the layer
    // the inverse ends with writes xy itself
    int first = 0;
    while (first < (int)p.layers.size() && p.layers[first].kind == CNF_LAYER_SQUEEZE) first++;
    // deferred inverse law (as the forward's, CoupPend::dir = -1): an LDS layer whose successor in
    // the inverse order (the previous layer by index) launches k_net_lds or the boundary maps leaves
    // its law to that kernel — no k_coupling launch for it
    CoupPend pend;
    bool have_pend = false;
    int bi = (int)p.boundaries.size() - 1;
    for (int li = (int)p.layers.size() - 1; li >= 0; li--) {
        const Layer& ly = p.layers[li];
        if (ly.kind == CNF_LAYER_COUPLING) {
            const Coupling& c = p.couplings[ly.ci];
            float* nxt = li == first ? xy : buf[which];
            CoupPend next;
            CouplingOpts o;
            o.pend = have_pend ? &pend : nullptr;
            o.defer = defers(p, c, li, -1);
            o.out_pend = &next;
            run_coupling(E, c, cur, nxt, ld != nullptr ? ld + (size_t)c.index * B * L.ld_parts : nullptr, -1, o);
            pend = next;
            have_pend = o.defer;
            cur = nxt;
            which ^= 1;
        } else if (ly.kind == CNF_LAYER_FACTOR) {
            // factor.backward (:294-329) + squeeze.backward (:191-217): rebuild the previous block
            // layout from the kept part (cur) and the factored part (read from zy at xy positions), one
            // k_map2 launch. With a pending coupling the kept part is read through it from u_k (the
            // other buffer), and v_k's own buffer (cur, never written) takes the result.
            const Boundary& b = p.boundaries[bi--];
            const bool last = li == first;
            float* prev = last ? xy : have_pend ? const_cast<float*>(cur) : buf[which];
            const bool flip = !have_pend;
            const int ncur = b.n_cur, nnext = b.n_next, nfac = b.n_fac;
            MapOp mk, mf;
            mk.src = cur, mk.dst = prev, mk.didx = T + b.dev_keep_src, mk.n = nnext, mk.ss = nnext, mk.ds = ncur;
            mf.src = zy, mf.dst = prev, mf.sidx = T + b.dev_fac_orig, mf.didx = T + b.dev_fac_src, mf.n = nfac;
            mf.ss = nuv, mf.ds = ncur;
            const CoupPend q = have_pend ? pend : CoupPend{};
            mk.pend = q.on;
            if (!p.dry && q.on && prev == q.u) throw std::logic_error("k_map2 would overwrite the u_k it reads");
            have_pend = false;
            E.record("k_map2", 0, 8.0 * B * (nnext + nfac),
                     [=](void* st) { launch_map2(mk, mf, LdReduce{}, q, B, (hipStream_t)st); });
            cur = prev;
            if (flip) which ^= 1;
        }
    }
    if (have_pend) throw std::logic_error("inverse: a deferred coupling was left pending");
    if (cur != xy) {   // (a schedule ending in a layout layer the maps did not cover)
        const float* src = cur;
        const size_t bytes = (size_t)B * nuv * 4;
        E.record("copy", 0, 2.0 * bytes, [=](void* st) {
            (void)hipMemcpyAsync(xy, src, bytes, hipMemcpyDeviceToDevice, (hipStream_t)st);
        });
    }
    if (logdet_per_image != nullptr) {   // log|det d xy / d zy| = -(sum of s), the fixed-order fp64 reduction
        const int nl = (int)p.couplings.size(), np = L.ld_parts;
        E.record("k_ld_reduce", 0, 8.0 * B * nl * np,
                 [=](void* st) { launch_ld_reduce(ld, logdet_per_image, B, nl, np, 0, (hipStream_t)st, 1); });
    }
    if (!p.dry) check_launch();
}

// ---- conditional sampling (include/cnf.h cnf_flow_sample; kernels: cnf_sample.hip) -----------------
// the sample workspace: the inverse workspace of `chunk` images, one chunk of zy and of xy_hat, and the
// statistics state (K, S1, S2) [3][B][H][W][x_d]
struct SampleLayout {
    size_t zy = 0, xy = 0, state = 0, total = 0;
};
static SampleLayout sample_layout(const Plan& p, int B, int chunk) {
    const cnf_flow_desc& d = p.desc;
    const size_t n_uv = (size_t)d.io_h * d.io_w * d.io_d;
    SampleLayout L;
    size_t off = align_up(p.layout(chunk).total, 256);
    auto take = [&](size_t bytes) {
        const size_t o = off;
        off = align_up(off + bytes, 256);
        return o;
    };
    L.zy = take((size_t)chunk * n_uv * 4);
    L.xy = take((size_t)chunk * n_uv * 4);
    L.state = take((size_t)3 * B * d.io_h * d.io_w * d.x_d * 4);
    L.total = off;
    return L;
}

// the argument errors of cnf_flow_sample that need no pointer but the descriptor (null: fine)
static const char* sample_desc_error(const Plan& p, int B, const cnf_sample_desc* s) {
    if (s == nullptr) return "null sample descriptor";
    if (B < 1) return "B must be >= 1";
    if (s->num_samples < 1) return "num_samples must be >= 1";
    if (s->chunk < 1) return "chunk must be >= 1";
    if (!(s->temperature >= 0.f) || std::isinf(s->temperature)) return "temperature must be finite and >= 0";
    if (s->logit_a != 0.f && !(s->logit_a > 0.f && s->logit_a < 0.5f))
        return "logit_a must be 0 (no de_logitify) or in (0, 0.5)";
    if (s->residual != 0 && p.desc.io_d - p.desc.x_d != p.desc.x_d)
        return "residual needs y of x's depth (io_d - x_d == x_d)";
    return nullptr;
}

extern "C" {

size_t cnf_plan_sample_workspace_bytes(const cnf_plan* plan, int B, const cnf_sample_desc* desc) {
    OptScope os_(plan ? &plan->p->opts : nullptr);
    if (!plan) return 0;
    if (const char* e = sample_desc_error(*plan->p, B, desc)) {   // (the message for cnf_last_error)
        (void)fail(CNF_E_INVALID, std::string("cnf_plan_sample_workspace_bytes: ") + e);
        return 0;
    }
    return sample_layout(*plan->p, B, desc->chunk).total;
}

// the body of cnf_flow_sample (log_prob null: its launches, exactly) and cnf_flow_sample_logp
static int flow_sample(const char* who, cnf_plan* plan, const float* params, const float* aux, const float* y,
                       const cnf_sample_desc* desc, float* samples, float* mean, float* std, float* y_dev,
                       float* log_prob, void* workspace, int B, void* stream) {
    OptScope os_(plan ? &plan->p->opts : nullptr);
    const std::string w(who);
    if (!plan || !params || !aux || !workspace) return fail(CNF_E_INVALID, w + ": null argument");
    if (!y) return fail(CNF_E_INVALID, w + ": null y");
    if (const char* e = sample_desc_error(*plan->p, B, desc)) return fail(CNF_E_INVALID, w + ": " + e);
    if (!samples && !mean && !std && !y_dev && !log_prob)
        return fail(CNF_E_INVALID, w + ": no output requested (samples, mean, std, y_dev" +
                                       (w == "cnf_flow_sample" ? "" : ", log_prob") + " all null)");
    CNF_TRY
    Plan& p = *plan->p;
    const cnf_flow_desc& d = p.desc;
    ensure_tables(p);
    p.recorded.clear();
    const SampleLayout SL = sample_layout(p, B, desc->chunk);
    char* ws = (char*)workspace;
    float* zy = reinterpret_cast<float*>(ws + SL.zy);
    float* xy = reinterpret_cast<float*>(ws + SL.xy);
    const bool stats = mean != nullptr || std != nullptr;
    SampleFoldArgs fa;
    std::memset(&fa, 0, sizeof(fa));
    fa.xy_hat = xy;
    fa.y = y;
    fa.samples = samples;
    fa.state = stats ? reinterpret_cast<float*>(ws + SL.state) : nullptr;
    fa.mean = mean;
    fa.std = std;
    fa.B = B;
    fa.logit = desc->logit_a != 0.f ? 1 : 0;
    fa.residual = desc->residual != 0 ? 1 : 0;
    if (fa.logit) fa.lk = logit_consts(desc->logit_a);
    const float T = desc->temperature;
    const unsigned long long seed = desc->seed, off = desc->offset;
    const long long total = (long long)B * desc->num_samples;
    const double px = (double)d.io_h * d.io_w;
    for (long long g0 = 0; g0 < total; g0 += desc->chunk) {
        const int n = (int)std::min<long long>(desc->chunk, total - g0);
        const SampleChunk c{g0, n, desc->num_samples, d.io_h * d.io_w, d.io_d, d.x_d};
        Exec E{p, params, aux, ws, p.layout(n), n, (hipStream_t)stream};
        E.record("k_latent", 0, 4.0 * n * px * (2 * d.io_d - d.x_d),
                 [=](void* st) { launch_latent(c, y, zy, T, seed, off, (hipStream_t)st); });
        flow_inverse(p, params, aux, zy, xy, ws, n, (hipStream_t)stream, true, nullptr, log_prob != nullptr);
        if (samples != nullptr || stats)
            E.record("k_sample_fold", 0, 4.0 * n * px * d.x_d * (samples ? 2 : 1),
                     [=](void* st) { launch_sample_fold(c, fa, (hipStream_t)st); });
        if (y_dev != nullptr)
            E.record("k_sample_ydev", 0, 8.0 * n * px * (d.io_d - d.x_d),
                     [=](void* st) { launch_sample_ydev(c, xy, y, y_dev, (hipStream_t)st); });
        if (log_prob != nullptr) {
            // the slots the chunk's inverse just wrote, read here: no reduce launch per chunk
            const double* ld = E.at<double>(E.L.ld);
            const int nl = (int)p.couplings.size(), np = E.L.ld_parts;
            E.record("k_sample_logp", 0, 4.0 * n * px * d.x_d + 8.0 * n * nl * np,
                     [=](void* st) { launch_sample_logp(c, zy, ld, nl, np, log_prob, (hipStream_t)st); });
        }
    }
    check_launch();
    return CNF_OK;
    CNF_CATCH
}

int cnf_flow_sample(cnf_plan* plan, const float* params, const float* aux, const float* y,
                    const cnf_sample_desc* desc, float* samples, float* mean, float* std, float* y_dev,
                    void* workspace, int B, void* stream) {
    return flow_sample("cnf_flow_sample", plan, params, aux, y, desc, samples, mean, std, y_dev, nullptr, workspace, B,
                       stream);
}

int cnf_flow_sample_logp(cnf_plan* plan, const float* params, const float* aux, const float* y,
                         const cnf_sample_desc* desc, float* samples, float* mean, float* std, float* y_dev,
                         float* log_prob, void* workspace, int B, void* stream) {
    return flow_sample("cnf_flow_sample_logp", plan, params, aux, y, desc, samples, mean, std, y_dev, log_prob,
                       workspace, B, stream);
}

}  // extern "C"

static void dry_run(Plan& p, int B, int direction) {
    p.dry = true;
    p.dry_launches.clear();
    char* fake = reinterpret_cast<char*>(uintptr_t(1) << 40);   // never dereferenced
    const float* f = reinterpret_cast<const float*>(fake);
    float* g = reinterpret_cast<float*>(fake + (1 << 20));        // a distinct output address
    try {
        if (direction > 0)
            flow_forward(p, f, f, f, g, g, fake, B, nullptr, false);
        else   // (-2: with the log-det)
            flow_inverse(p, f, f, f, g, fake, B, nullptr, false, direction == -2 ? g + (1 << 18) : nullptr);
    } catch (...) {
        p.dry = false;
        throw;
    }
    p.dry = false;
    p.recorded.clear();
}

extern "C" {

int cnf_coupling_forward(cnf_plan* plan, int layer, const float* params, const float* aux, const float* u, float* v,
                         float* logdet_accum, void* workspace, int B, void* stream) {
    OptScope os_(plan ? &plan->p->opts : nullptr);
    if (!plan || !params || !aux || !u || !v || !workspace || B <= 0) return fail(CNF_E_INVALID, "null argument");
    CNF_TRY
    Plan& p = *plan->p;
    if (layer < 0 || layer >= (int)p.layers.size() || p.layers[layer].kind != CNF_LAYER_COUPLING)
        return fail(CNF_E_INVALID, "layer is not a coupling layer");
    if (u == v) return fail(CNF_E_INVALID, "u and v must not alias");
    ensure_tables(p);
    p.recorded.clear();
    Exec E{p, params, aux, (char*)workspace, p.layout(B), B, (hipStream_t)stream};
    double* ld = E.at<double>(E.L.ld);
    const Coupling& c = p.couplings[p.layers[layer].ci];
    run_coupling(E, c, u, v, logdet_accum ? ld : nullptr, +1);
    if (logdet_accum) {
        const int np = E.L.ld_parts;
        E.record("k_ld_reduce", 0, 0, [=](void* st) { launch_ld_reduce(ld, logdet_accum, B, 1, np, 1, (hipStream_t)st); });
    }
    check_launch();
    return CNF_OK;
    CNF_CATCH
}

int cnf_coupling_inverse(cnf_plan* plan, int layer, const float* params, const float* aux, const float* v, float* u,
                         void* workspace, int B, void* stream) {
    OptScope os_(plan ? &plan->p->opts : nullptr);
    if (!plan || !params || !aux || !u || !v || !workspace || B <= 0) return fail(CNF_E_INVALID, "null argument");
    CNF_TRY
    Plan& p = *plan->p;
    if (layer < 0 || layer >= (int)p.layers.size() || p.layers[layer].kind != CNF_LAYER_COUPLING)
        return fail(CNF_E_INVALID, "layer is not a coupling layer");
    if (u == v) return fail(CNF_E_INVALID, "u and v must not alias");
    ensure_tables(p);
    p.recorded.clear();
    Exec E{p, params, aux, (char*)workspace, p.layout(B), B, (hipStream_t)stream};
    run_coupling(E, p.couplings[p.layers[layer].ci], v, u, nullptr, -1);
    check_launch();
    return CNF_OK;
    CNF_CATCH
}

int cnf_coupling_inverse_logdet(cnf_plan* plan, int layer, const float* params, const float* aux, const float* v,
                                float* u, float* logdet_accum, void* workspace, int B, void* stream) {
    OptScope os_(plan ? &plan->p->opts : nullptr);
    if (!plan || !params || !aux || !u || !v || !workspace || B <= 0) return fail(CNF_E_INVALID, "null argument");
    CNF_TRY
    Plan& p = *plan->p;
    if (layer < 0 || layer >= (int)p.layers.size() || p.layers[layer].kind != CNF_LAYER_COUPLING)
        return fail(CNF_E_INVALID, "layer is not a coupling layer");
    if (u == v) return fail(CNF_E_INVALID, "u and v must not alias");
    ensure_tables(p);
    p.recorded.clear();
    Exec E{p, params, aux, (char*)workspace, p.layout(B), B, (hipStream_t)stream};
    double* ld = E.at<double>(E.L.ld);
    run_coupling(E, p.couplings[p.layers[layer].ci], v, u, logdet_accum ? ld : nullptr, -1);
    if (logdet_accum) {   // -= the per-image sum of s
        const int np = E.L.ld_parts;
        E.record("k_ld_reduce", 0, 0,
                 [=](void* st) { launch_ld_reduce(ld, logdet_accum, B, 1, np, 1, (hipStream_t)st, 1); });
    }
    check_launch();
    return CNF_OK;
    CNF_CATCH
}

int cnf_squeeze(const float* in, float* out, int B, int H, int W, int C, int dir, void* stream) {
    if (!in || !out || B <= 0 || H <= 0 || W <= 0 || C <= 0) return fail(CNF_E_INVALID, "bad argument");
    if (dir > 0 && ((H % 2) || (W % 2))) return fail(CNF_E_INVALID, "u must have spatial dimensions divisible by 2.");
    if (dir < 0 && (C % 4)) return fail(CNF_E_INVALID, "v must have channel dimensions divisible by 4.");
    CNF_TRY
    launch_squeeze(in, out, B, H, W, C, dir > 0 ? 1 : -1, (hipStream_t)stream);
    check_launch();
    return CNF_OK;
    CNF_CATCH
}

int cnf_channel_copy(const float* in, int in_cs, int in_off, float* out, int out_cs, int out_off, int C, int B, int HW,
                     void* stream) {
    if (!in || !out || C < 0 || B <= 0 || HW <= 0 || in_off + C > in_cs || out_off + C > out_cs)
        return fail(CNF_E_INVALID, "bad channel window");
    if (C == 0) return CNF_OK;
    CNF_TRY
    launch_chcopy(in, in_cs, in_off, out, out_cs, out_off, C, (long long)B * HW, (hipStream_t)stream);
    check_launch();
    return CNF_OK;
    CNF_CATCH
}

int cnf_nll(const cnf_plan* plan, const float* xy, const float* zy, const float* logdet_per_image, float* per_image,
            float* sums, int B, void* stream) {
    OptScope os_(plan ? &plan->p->opts : nullptr);
    if (!plan || !xy || !zy || !logdet_per_image || !per_image || !sums || B <= 0)
        return fail(CNF_E_INVALID, "null argument");
    CNF_TRY
    Plan& p = *plan->p;
    ensure_tables(p);
    const cnf_flow_desc& d = p.desc;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    hip_check(hipStreamIsCapturing((hipStream_t)stream, &cap), "hipStreamIsCapturing");
    const bool capturing = cap != hipStreamCaptureStatusNone;
    std::lock_guard<std::mutex> lk(*p.nll_mu);
    int slot = -1;
    for (size_t i = 0; i < p.nll_streams.size(); i++)
        if (p.nll_streams[i] == stream) slot = (int)i;
    if (slot < 0 && (int)p.nll_streams.size() < Plan::NLL_SLOTS) {
        p.nll_streams.push_back(stream);
        p.nll_ev.push_back(nullptr);
        p.nll_last.push_back(0);
        slot = (int)p.nll_streams.size() - 1;
    }
    if (slot < 0) {
        // every slot has its stream: take the least recently used one. Its counter is back at 0 once that
        // stream's last cnf_nll has completed, so this launch waits for it (stream-ordered, no host wait)
        slot = 0;
        for (int i = 1; i < Plan::NLL_SLOTS; i++)
            if (p.nll_last[i] < p.nll_last[slot]) slot = i;
        if (p.nll_ev[slot] != nullptr && hipEventQuery(p.nll_ev[slot]) != hipSuccess)
            hip_check(hipStreamWaitEvent((hipStream_t)stream, p.nll_ev[slot], 0), "hipStreamWaitEvent");
        else if (p.nll_ev[slot] == nullptr && capturing)
            throw std::runtime_error("cnf_nll: a 65th stream on one plan during graph capture (reuse needs an "
                                     "uncaptured call on the slot's stream first)");
        p.nll_streams[slot] = stream;
    }
    p.nll_last[slot] = ++p.nll_clock;
    unsigned* done = reinterpret_cast<unsigned*>(p.dev_table + p.host_table.size()) + slot;
    launch_nll(xy, zy, logdet_per_image, per_image, sums, done, B, d.io_h * d.io_w, d.io_d, d.x_d, d.lambda_y,
               (hipStream_t)stream);
    check_launch();
    if (!capturing) {   // (the slot's completion point, for a later reuse by another stream)
        if (p.nll_ev[slot] == nullptr)
            hip_check(hipEventCreateWithFlags(&p.nll_ev[slot], hipEventDisableTiming), "hipEventCreate");
        hip_check(hipEventRecord(p.nll_ev[slot], (hipStream_t)stream), "hipEventRecord");
    }
    return CNF_OK;
    CNF_CATCH
}

// diagnostic: phase stamps of the last CNF_STAMPS=1 k_net_lds launch (s_memrealtime, 100 MHz)
// ---- TOYcINN -------------------------------------------------------------------------------
static int64_t toy_net_floats(int n1, int n2, int H, int L) {
    return (int64_t)n1 * H + H + (int64_t)L * (H * H + H) + (int64_t)H * n2 + n2;
}

static void toy_check(const cnf_toy_desc* d) {
    if (!d) throw std::invalid_argument("null toy descriptor");
    if (d->io_shape != 3) throw std::invalid_argument("TOYcINN masks are defined for io_shape == 3 only");
    if (d->x_d < 1 || d->x_d > 2) throw std::invalid_argument("x_d must be 1 or 2");
    if (d->num_coupling_layers < 1 || d->num_coupling_layers > TOY_MAXL)
        throw std::invalid_argument("num_coupling_layers must be in [1, 128]");
    if (d->intermediate_dims < 1 || d->intermediate_dims > 64) throw std::invalid_argument("intermediate_dims must be in [1, 64]");
    if (d->num_layers < 0) throw std::invalid_argument("num_layers must be >= 0");
    if (!d->mask_indices) throw std::invalid_argument("mask_indices is required");
    std::vector<int> seen(d->num_coupling_layers, 0);
    for (int i = 0; i < d->num_coupling_layers; i++) {
        const int j = d->mask_indices[i];
        if (j < 0 || j >= d->num_coupling_layers || seen[j]++) throw std::invalid_argument("mask_indices must be a permutation");
    }
}

int64_t cnf_toy_num_params(const cnf_toy_desc* d) {
    CNF_TRY
    toy_check(d);
    int64_t n = 0;
    for (int j = 0; j < d->num_coupling_layers; j++) {
        const int n1 = (j % 6) < 3 ? 1 : 2;
        n += 2 * toy_net_floats(n1, 3 - n1, d->intermediate_dims, d->num_layers);
    }
    return n;
    CNF_CATCH
}

// k_toy's launch arguments for direction `direction`; returns the LDS staging floats (the largest coupling network)
static int64_t toy_args(const cnf_toy_desc* d, const float* params, const float* u, float* v, float* log_detJ,
                        float* per_sample, int B, int direction, ToyArgs& a) {
    std::memset(&a, 0, sizeof(a));
    a.params = params;
    a.u = u;
    a.v = v;
    a.log_detJ = direction < 0 ? log_detJ : nullptr;
    a.per_sample = direction < 0 ? per_sample : nullptr;
    a.B = B;
    a.nl = d->num_coupling_layers;
    a.H = d->intermediate_dims;
    a.L = d->num_layers;
    a.x_d = d->x_d;
    a.dir = direction;
    a.lambda_y = d->lambda_y;
    int64_t off = 0, maxn = 0;
    for (int j = 0; j < a.nl; j++) {
        a.order[j] = d->mask_indices[j];
        a.net_off[j] = (int)off;
        const int n1 = (j % 6) < 3 ? 1 : 2;
        const int64_t n = 2 * toy_net_floats(n1, 3 - n1, a.H, a.L);
        off += n;
        maxn = std::max(maxn, n);
    }
    a.net_off[a.nl] = (int)off;
    return maxn;
}

int cnf_toy_call(const cnf_toy_desc* d, const float* params, const float* u, float* v, float* log_detJ,
                 float* per_sample, int B, int direction, void* stream) {
    CNF_TRY
    toy_check(d);
    if (!params || !u || !v || B < 0) return fail(CNF_E_INVALID, "null pointer or negative batch");
    if (direction != 1 && direction != -1) return fail(CNF_E_INVALID, "direction must be +1 or -1");
    if (u == v) return fail(CNF_E_INVALID, "u and v must not alias");
    if (B == 0) return CNF_OK;
    ToyArgs a;
    const int64_t maxn = toy_args(d, params, u, v, log_detJ, per_sample, B, direction, a);
    if (maxn * 4 > 160 * 1024) return fail(CNF_E_INVALID, "toy coupling networks exceed the 160 KiB LDS staging budget");
    launch_toy(a, (int)maxn, (hipStream_t)stream);
    hip_check(hipGetLastError(), "k_toy");
    return CNF_OK;
    CNF_CATCH
}

// ---- TOYcINN training (TOYcINN_make_model.py:453-481) ------------------------------------------
// training workspace: the saved coupling-layer inputs [nl][B][3], then one partial gradient row per
// tile of TOY_TS samples [tiles][num_params]
static size_t toy_saved_bytes(const cnf_toy_desc* d, int B) {
    return ((size_t)d->num_coupling_layers * B * 3 * sizeof(float) + 255) & ~(size_t)255;
}

size_t cnf_toy_train_workspace_bytes(const cnf_toy_desc* d, int B) {
    try {
        toy_check(d);
        if (B < 1) throw std::invalid_argument("B must be >= 1");
        const int64_t n = cnf_toy_num_params(d);
        const size_t tiles = ((size_t)B + TOY_TS - 1) / TOY_TS;
        return toy_saved_bytes(d, B) + tiles * (size_t)n * sizeof(float);
    } catch (const std::exception& e) {
        fail(CNF_E_INVALID, e.what());
        return 0;
    }
}

int cnf_toy_forward_train(const cnf_toy_desc* d, const float* params, const float* xy, float* zy, float* per_sample,
                          void* train_workspace, int B, void* stream) {
    CNF_TRY
    toy_check(d);
    if (!params || !xy || !zy || !train_workspace) return fail(CNF_E_INVALID, "null pointer");
    if (B < 1) return fail(CNF_E_INVALID, "B must be >= 1");
    if (xy == zy) return fail(CNF_E_INVALID, "xy and zy must not alias");
    ToyArgs a;
    const int64_t maxn = toy_args(d, params, xy, zy, nullptr, per_sample, B, -1, a);
    if (maxn * 4 > 160 * 1024) return fail(CNF_E_INVALID, "toy coupling networks exceed the 160 KiB LDS staging budget");
    a.save_u = static_cast<float*>(train_workspace);
    launch_toy(a, (int)maxn, (hipStream_t)stream);
    hip_check(hipGetLastError(), "k_toy");
    return CNF_OK;
    CNF_CATCH
}

int cnf_toy_backward(const cnf_toy_desc* d, const float* params, const float* xy, const float* zy, void* train_workspace,
                     int B, float inv_batch, float* dparams, void* stream) {
    CNF_TRY
    toy_check(d);
    if (!params || !xy || !zy || !train_workspace || !dparams) return fail(CNF_E_INVALID, "null pointer");
    if (B < 1) return fail(CNF_E_INVALID, "B must be >= 1");
    if (!std::isfinite(inv_batch)) return fail(CNF_E_INVALID, "inv_batch must be finite");
    if (toy_bwd_lds_bytes(d->intermediate_dims, d->num_layers) > 160 * 1024)
        return fail(CNF_E_INVALID, "the toy backward's activations exceed the 160 KiB LDS budget");
    ToyArgs f;
    toy_args(d, params, xy, nullptr, nullptr, nullptr, B, -1, f);
    ToyBwdArgs a;
    std::memset(&a, 0, sizeof(a));
    a.params = params;
    a.xy = xy;
    a.zy = zy;
    a.saved_u = static_cast<const float*>(train_workspace);
    a.part = reinterpret_cast<float*>(static_cast<char*>(train_workspace) + toy_saved_bytes(d, B));
    a.B = B;
    a.nl = f.nl;
    a.H = f.H;
    a.L = f.L;
    a.x_d = f.x_d;
    a.HP = toy_bwd_hp(f.H);
    a.num_params = f.net_off[f.nl];
    a.lambda_y = d->lambda_y;
    a.inv_batch = inv_batch;
    std::memcpy(a.order, f.order, sizeof(a.order));
    std::memcpy(a.net_off, f.net_off, sizeof(a.net_off));
    launch_toy_bwd(a, (hipStream_t)stream);
    hip_check(hipGetLastError(), "k_toy_bwd");
    launch_toy_grad_sum(a.part, (B + TOY_TS - 1) / TOY_TS, a.num_params, dparams, (hipStream_t)stream);
    hip_check(hipGetLastError(), "k_toy_grad_sum");
    return CNF_OK;
    CNF_CATCH
}

// ---- TOYcINN sampling (TOYcINN.py:807-817; kernels: cnf_toy_sample.hip) -------------------------
// the argument errors of cnf_toy_sample that need no pointer but the descriptors (null: fine)
static const char* toy_sample_desc_error(const cnf_toy_desc* d, int B, const cnf_toy_sample_desc* s) {
    if (s == nullptr) return "null sample descriptor";
    if (B < 1) return "B must be >= 1";
    if (s->num_samples < 1) return "num_samples must be >= 1";
    if (!(s->temperature >= 0.f) || std::isinf(s->temperature)) return "temperature must be finite and >= 0";
    if (s->hist_bins < 0) return "hist_bins must be >= 0";
    const int64_t tiles = ((int64_t)s->num_samples + TOY_SAMPLE_TS - 1) / TOY_SAMPLE_TS;
    if ((int64_t)B * tiles > INT32_MAX || (double)B * s->num_samples * d->x_d > 4e18)
        return "B * num_samples * x_d exceeds the index range (B * tiles must stay below 2^31)";
    if (s->hist_bins >= 1) {
        for (int c = 0; c < d->x_d; c++) {
            if (!std::isfinite(s->hist_lo[c]) || !std::isfinite(s->hist_hi[c])) return "hist_lo / hist_hi must be finite";
            if (!(s->hist_lo[c] < s->hist_hi[c])) return "hist_lo must be below hist_hi";
            if (!std::isfinite((float)s->hist_bins / (s->hist_hi[c] - s->hist_lo[c]))) return "hist_lo / hist_hi: the bin scale is not finite";
        }
        if (std::pow((double)s->hist_bins, d->x_d) * B > 1e12) return "hist_bins: the grid exceeds 10^12 cells";
    }
    return nullptr;
}

static size_t toy_sample_part_bytes(const cnf_toy_desc* d, int B, const cnf_toy_sample_desc* s) {
    const size_t tiles = ((size_t)s->num_samples + TOY_SAMPLE_TS - 1) / TOY_SAMPLE_TS;
    return (size_t)B * tiles * d->x_d * TOY_SAMPLE_PART * sizeof(float);
}

size_t cnf_toy_sample_workspace_bytes(const cnf_toy_desc* d, int B, const cnf_toy_sample_desc* s) {
    try {
        toy_check(d);
        if (const char* e = toy_sample_desc_error(d, B, s)) throw std::invalid_argument(e);
        return toy_sample_part_bytes(d, B, s);
    } catch (const std::exception& e) {
        fail(CNF_E_INVALID, std::string("cnf_toy_sample_workspace_bytes: ") + e.what());
        return 0;
    }
}

int cnf_toy_sample(const cnf_toy_desc* d, const float* params, const float* y, const cnf_toy_sample_desc* s,
                   float* samples, float* mean, float* std, float* y_dev, uint32_t* hist, void* workspace, int B,
                   void* stream) {
    CNF_TRY
    toy_check(d);
    if (!params || !workspace) return fail(CNF_E_INVALID, "cnf_toy_sample: null params or workspace");
    if (!y) return fail(CNF_E_INVALID, "cnf_toy_sample: null y");
    if (const char* e = toy_sample_desc_error(d, B, s)) return fail(CNF_E_INVALID, std::string("cnf_toy_sample: ") + e);
    if (hist && s->hist_bins < 1) return fail(CNF_E_INVALID, "cnf_toy_sample: hist given with hist_bins < 1");
    if (!hist && s->hist_bins >= 1) return fail(CNF_E_INVALID, "cnf_toy_sample: hist_bins >= 1 with a null hist");
    if (!samples && !mean && !std && !y_dev && !hist)
        return fail(CNF_E_INVALID, "cnf_toy_sample: no output requested (samples, mean, std, y_dev, hist all null)");
    if (toy_sample_lds_bytes(d->intermediate_dims) > 160 * 1024)
        return fail(CNF_E_INVALID, "cnf_toy_sample: the hidden activations of a draw tile exceed the 160 KiB LDS budget");
    ToyArgs f;
    toy_args(d, params, nullptr, nullptr, nullptr, nullptr, B, 1, f);
    ToySampleArgs a;
    std::memset(&a, 0, sizeof(a));
    a.params = params;
    a.y = y;
    a.samples = samples;
    a.y_dev = y_dev;
    a.hist = hist;
    a.part = static_cast<float*>(workspace);
    a.B = B;
    a.S = s->num_samples;
    a.tiles = (s->num_samples + TOY_SAMPLE_TS - 1) / TOY_SAMPLE_TS;
    a.nl = f.nl;
    a.H = f.H;
    a.L = f.L;
    a.x_d = f.x_d;
    a.HP = toy_bwd_hp(f.H);
    a.temperature = s->temperature;
    a.seed = s->seed;
    a.offset = s->offset;
    a.G = hist ? s->hist_bins : 0;
    for (int c = 0; c < 2; c++) {
        a.lo[c] = hist && c < f.x_d ? s->hist_lo[c] : 0.f;
        a.scale[c] = hist && c < f.x_d ? (float)s->hist_bins / (s->hist_hi[c] - s->hist_lo[c]) : 0.f;
    }
    std::memcpy(a.order, f.order, sizeof(a.order));
    std::memcpy(a.net_off, f.net_off, sizeof(a.net_off));
    if (hist) {
        size_t cells = (size_t)B;
        for (int c = 0; c < f.x_d; c++) cells *= (size_t)s->hist_bins;
        hip_check(hipMemsetAsync(hist, 0, cells * sizeof(uint32_t), (hipStream_t)stream), "hipMemsetAsync(hist)");
    }
    launch_toy_sample(a, (hipStream_t)stream);
    hip_check(hipGetLastError(), "k_toy_sample");
    if (mean || std) {
        launch_toy_sample_stats(a.part, B, a.tiles, a.S, a.x_d, mean, std, (hipStream_t)stream);
        hip_check(hipGetLastError(), "k_toy_sample_stats");
    }
    return CNF_OK;
    CNF_CATCH
}

int cnf_toy_nll_sums(const float* per_sample, float* sums, int B, void* stream) {
    CNF_TRY
    if (!per_sample || !sums || B < 1) return fail(CNF_E_INVALID, "null pointer or empty batch");
    launch_nll_sums(per_sample, sums, B, (hipStream_t)stream);
    hip_check(hipGetLastError(), "k_nll_sums");
    return CNF_OK;
    CNF_CATCH
}

// shape words of coupling `coupling`'s k_net_lds launch (0 if the layer is streamed); host only, used
// by csrc/gen_netlds_shapes.py to generate the shape-specialised instantiations' table
int cnf_debug_netlds_shape(const cnf_plan* plan, int coupling, int* words, int cap) {
    OptScope os_(plan ? &plan->p->opts : nullptr);
    if (!plan || !words || cap < NETSHAPE_WORDS) return -1;
    const Plan& p = *plan->p;
    if (coupling < 0 || coupling >= (int)p.couplings.size()) return -1;
    const Coupling& c = p.couplings[coupling];
    if (!c.use_lds) return 0;
    NetLdsArgs a;
    if (netlds_setup(p, c, a) == 0) return 0;
    netshape_words(a, words);
    return NETSHAPE_WORDS;
}
int cnf_debug_netlds_nshapes() { return netlds_num_shapes(); }

// k_pw launch shapes of a B-image forward, from a host-only dry run (nothing is launched or
// dereferenced: the tensors are placeholder addresses); returns the number of words written
int cnf_debug_pw_shapes(cnf_plan* plan, int B, int* words, int cap);
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

// launch names of a B-image forward (direction +1), inverse (-1) or inverse with log-det (-2:
// cnf_flow_inverse_logdet) from a host-only dry run, one per
// line into out (cap bytes, NUL-terminated); returns the number of launches, -1 on error
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

// shape words of coupling `coupling`'s k_gc launches, one GcShape per group (0 if it has none)
int cnf_debug_gc_shape(const cnf_plan* plan, int coupling, int* words, int cap) {
    OptScope os_(plan ? &plan->p->opts : nullptr);
    if (!plan || !words) return -1;
    const Plan& p = *plan->p;
    if (coupling < 0 || coupling >= (int)p.couplings.size()) return -1;
    const Coupling& c = p.couplings[coupling];
    if (c.use_lds || !c.gc_fused) return 0;
    if (cap < GCSHAPE_WORDS * (int)c.gcg.size()) return -1;
    int n = 0;
    for (const Coupling::GcGroup& gg : c.gcg) {
        // the forward's k_gc: LN2 on load and LN3 partials iff LayerNorm
        const GcShape s = gc_shape(c, gg, p.desc.layer_norm ? 3 : 0);
        std::memcpy(words + n, &s, sizeof(s));
        n += GCSHAPE_WORDS;
    }
    return n;
}
int cnf_debug_gc_words() { return GCSHAPE_WORDS; }

// t1 layout of a coupling (Coupling::t1_map): [compact, floats per pixel of the image, then per branch
// (window offset of pixel 0, pixel stride, cin_off, cin), then 128 words of t1_map (compact only)]
// t2 layout of a coupling (Coupling::t2_*): [mapped, floats per pixel of the image, gc, then per branch
// (slice offset of pixel 0, pixel stride, out_off, cout), then conv_b's quad map (gc / 4 pairs, mapped only)]
int cnf_debug_t2_layout(const cnf_plan* plan, int coupling, int* words, int cap) {
    OptScope os_(plan ? &plan->p->opts : nullptr);
    if (!plan || !words) return -1;
    const Plan& p = *plan->p;
    if (coupling < 0 || coupling >= (int)p.couplings.size()) return -1;
    const Coupling& c = p.couplings[coupling];
    std::vector<int> w = {c.t2_mapped ? 1 : 0, c.t2_cs, c.gc};
    for (size_t bi = 0; bi < c.br.size(); bi++) {
        w.push_back(bi < c.t2_off.size() ? c.t2_off[bi] : -1);
        w.push_back(bi < c.t2_pcs.size() ? c.t2_pcs[bi] : -1);
        w.push_back(c.br[bi].out_off);
        w.push_back(c.br[bi].cout);
    }
    w.insert(w.end(), c.t2_qmap.begin(), c.t2_qmap.end());
    if ((int)w.size() > cap) return -1;
    std::memcpy(words, w.data(), w.size() * sizeof(int));
    return (int)w.size();
}

int cnf_debug_t1_layout(const cnf_plan* plan, int coupling, int* words, int cap) {
    OptScope os_(plan ? &plan->p->opts : nullptr);
    if (!plan || !words) return -1;
    const Plan& p = *plan->p;
    if (coupling < 0 || coupling >= (int)p.couplings.size()) return -1;
    const Coupling& c = p.couplings[coupling];
    std::vector<int> w = {c.t1_compact ? 1 : 0, c.t1_cs};
    for (size_t bi = 0; bi < c.br.size(); bi++) {
        w.push_back(bi < c.t1_off.size() ? c.t1_off[bi] : -1);
        w.push_back(bi < c.t1_pcs.size() ? c.t1_pcs[bi] : -1);
        w.push_back(c.br[bi].cin_off);
        w.push_back(c.br[bi].cin);
    }
    w.insert(w.end(), c.t1_map.begin(), c.t1_map.end());
    if ((int)w.size() > cap) return -1;
    std::memcpy(words, w.data(), w.size() * sizeof(int));
    return (int)w.size();
}

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
