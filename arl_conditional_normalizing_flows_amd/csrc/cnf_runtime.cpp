// cnf_runtime.cpp — the plan as an object of the C ABI of libcnf_hip.so (include/cnf.h): create / destroy /
// info, debug options, the workspace layout, the device tables, and the entry points that are one launch each
// (pack, NLL, Adam, squeeze, channel copy); the schedules that execute a plan: cnf_schedule.cpp. All memory is
// the caller's (params, aux, workspace); the plan owns only its index tables and the streams and events it made.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>

#include "cnf_api.h"
#include "cnf_plan.h"

namespace cnf {

static thread_local std::string g_err;   // cnf_last_error

int set_error(int code, const char* msg) {
    g_err = msg;
    return code;
}

// ---- debug options (cnf_flow_desc.debug_options)
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

static thread_local const Options* g_opts = nullptr;
static const Options kDefaultOptions{};
const Options& opts() { return g_opts != nullptr ? *g_opts : kDefaultOptions; }
OptScope::OptScope(const Options* o) : prev(g_opts) {
    if (o != nullptr) g_opts = o;
}
OptScope::~OptScope() { g_opts = prev; }

LaunchTiming& launch_timing() {
    thread_local LaunchTiming t;
    return t;
}

// ---- workspace layout
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
        for (int k = 0; k < 3; k++) L.st_part[n][k] = take(Bz * parts * LNP * 4);   // LN slabs y, t1, t2: per-wave partials
    }
    L.ld = take(std::max<size_t>(1, couplings.size()) * Bz * ldp * 8);
    L.total = off;
    return L;
}

// ---- device tables
// the n elements at src as a new device array with `zeroed` zero elements behind them (one element at
// least); label names the array in the error text
template <class T>
static T* upload(const T* src, size_t n, size_t zeroed, const char* label) {
    const std::string l = std::string("(") + label + ")";
    const size_t bytes = std::max<size_t>(1, n + zeroed) * sizeof(T);
    T* dev = nullptr;
    hip_check(hipMalloc(&dev, bytes), ("hipMalloc" + l).c_str());
    if (zeroed > 0) hip_check(hipMemset(dev, 0, bytes), ("hipMemset" + l).c_str());
    if (n > 0) hip_check(hipMemcpy(dev, src, n * sizeof(T), hipMemcpyHostToDevice), ("hipMemcpy" + l).c_str());
    return dev;
}

void ensure_tables(Plan& p) {
    int dev = 0;
    hip_check(hipGetDevice(&dev), "hipGetDevice");
    if (p.dev_table != nullptr && p.device == dev) return;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    // uploading is not capturable: the first call on a device must run eagerly
    if (hipStreamIsCapturing(nullptr, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
        throw std::runtime_error("plan tables not uploaded yet (call cnf_pack_params before graph capture)");
    // NLL_SLOTS ints past the table: cnf_nll's completion counters (zero between launches)
    p.dev_table = upload(p.host_table.data(), p.host_table.size(), Plan::NLL_SLOTS, "table");
    // (the fp32 part of the kernel image: the plane region behind it has a map of its own)
    p.dev_aux_map = upload(p.aux_map.data(), (size_t)std::max<int64_t>(0, p.x6_base), 0, "aux map");
    p.dev_x6_map = upload(p.x6_map.data(), p.x6_map.size(), 0, "plane map");
    p.dev_bw_map = upload(p.bw_map.data(), p.bw_map.size(), 0, "bw map");
    p.device = dev;
}

Plan::~Plan() {
    for (void* t : {(void*)dev_table, (void*)dev_aux_map, (void*)dev_x6_map, (void*)dev_bw_map})
        if (t) (void)hipFree(t);
    for (const std::vector<hipEvent_t>* set : {&ev, &tev, &nll_ev})
        for (hipEvent_t e : *set)
            if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : {ev_fork, ev_join})
        if (e) (void)hipEventDestroy(e);
    for (hipStream_t s : {side, wside[0], wside[1]})
        if (s) (void)hipStreamDestroy(s);
}

}  // namespace cnf

using namespace cnf;

extern "C" {

const char* cnf_last_error(void) { return g_err.c_str(); }
const char* cnf_version(void) { return "cnf-mi355x 0.2 (gfx950)"; }

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
    delete plan->p;   // (frees what it holds on a device: Plan::~Plan)
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
    if (name && name_cap > 0) std::snprintf(name, (size_t)name_cap, "%s", t.name.c_str());
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

size_t cnf_plan_train_workspace_bytes(const cnf_plan* plan, int B) {
    OptScope os_(plan ? &plan->p->opts : nullptr);
    if (!plan || B <= 0) return 0;
    try {
        return plan->p->train_layout(B).total;
    } catch (...) {
        return 0;
    }
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

}  // extern "C"
