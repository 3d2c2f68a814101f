// cnf_schedule.cpp — the layer schedule of cFlow.call (conv_cINN_make_model.py:1723-1798) as a fixed
// sequence of coupling layers (cnf_coupling.cpp) and map launches on the caller's stream, forward and
// inverse, and the C ABI that runs it: cnf_flow_*, cnf_coupling_* (include/cnf.h). The backward entry
// points only forward to cnf_train.cpp.
#include <cstring>
#include <stdexcept>

#include "cnf_api.h"
#include "cnf_plan.h"

namespace cnf {
namespace {

// the layer after li in schedule order (step +1: forward, -1: inverse) that launches anything: squeezes
// are folded into the factor maps
struct NextLaunch {
    const Coupling* coupling = nullptr;   // a coupling layer
    bool maps = false, end = false;       // a factor boundary (k_map2); nothing: the schedule's tail follows
};
NextLaunch next_launch(const Plan& p, int li, int step) {
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
bool defers(const Plan& p, const Coupling& c, int li, int step) {
    if (p.opts.fuse_coupling == 0 || !c.use_lds) return false;
    const NextLaunch nx = next_launch(p, li, step);
    return (nx.coupling != nullptr && nx.coupling->use_lds) || nx.maps || (nx.end && step > 0);
}

}  // namespace

void flow_forward(Plan& p, const float* params, const float* aux, const float* xy, float* zy,
                  float* logdet_per_image, void* workspace, int B, hipStream_t stream, bool save_inputs,
                  const InputPrepArgs* nz, bool append) {
    if (!p.dry) ensure_tables(p);
    if (!append) p.recorded.clear();
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

void flow_inverse(Plan& p, const float* params, const float* aux, const float* zy, float* xy, void* workspace, int B,
                  hipStream_t stream, const InverseOpts& io) {
    if (!p.dry) ensure_tables(p);
    if (!io.append) p.recorded.clear();
    float* const logdet_per_image = io.logdet_per_image;
    Exec E{p, params, aux, (char*)workspace, p.layout(B), B, stream};
    const WsLayout& L = E.L;
    // log-det slots [couplings][B][ld_parts], as the forward's: each coupling's block is written once, by
    // the kernel that applies its law (k_coupling, the next k_net_lds, or the boundary k_map2)
    double* ld = logdet_per_image != nullptr || io.ld_slots ? E.at<double>(L.ld) : nullptr;
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

void dry_run(Plan& p, int B, int direction) {
    p.dry = true;
    p.dry_launches.clear();
    char* fake = reinterpret_cast<char*>(uintptr_t(1) << 40);   // never dereferenced
    const float* f = reinterpret_cast<const float*>(fake);
    float* g = reinterpret_cast<float*>(fake + (1 << 20));        // a distinct output address
    try {
        InverseOpts io;
        if (direction == -2) io.logdet_per_image = g + (1 << 18);   // (with the log-det)
        if (direction > 0)
            flow_forward(p, f, f, f, g, g, fake, B, nullptr, false);
        else
            flow_inverse(p, f, f, f, g, fake, B, nullptr, io);
    } catch (...) {
        p.dry = false;
        throw;
    }
    p.dry = false;
    p.recorded.clear();
}

}  // namespace cnf

using namespace cnf;

namespace {

const char* const kNullOrB = "null argument or B <= 0";
const char* const kNotCoupling = "layer is not a coupling layer";

// what cnf_flow_forward, _forward_train, _inverse and _inverse_logdet refuse before anything runs: a null
// pointer (all_set false), an empty batch, or an output that is its input (dir: which way the text reads)
int flow_args_error(bool all_set, int B, const float* in, const float* out, int dir) {
    if (!all_set || B <= 0) return fail(CNF_E_INVALID, kNullOrB);
    if (in == out)
        return fail(CNF_E_INVALID, dir > 0 ? "xy and zy must not alias (out-of-place only)"
                                           : "zy and xy must not alias (out-of-place only)");
    return CNF_OK;
}

// one coupling layer on its own, in -> out in direction dir; logdet_accum (may be null) += the per-image sum
// of s (forward), -= it (inverse)
int single_coupling(cnf_plan* plan, int layer, const float* params, const float* aux, const float* in, float* out,
                    float* logdet_accum, void* workspace, int B, void* stream, int dir) {
    OptScope os_(plan ? &plan->p->opts : nullptr);
    if (!plan || !params || !aux || !in || !out || !workspace || B <= 0) return fail(CNF_E_INVALID, "null argument");
    CNF_TRY
    Plan& p = *plan->p;
    if (layer < 0 || layer >= (int)p.layers.size() || p.layers[layer].kind != CNF_LAYER_COUPLING)
        return fail(CNF_E_INVALID, kNotCoupling);
    if (in == out) return fail(CNF_E_INVALID, "u and v must not alias");
    ensure_tables(p);
    p.recorded.clear();
    Exec E{p, params, aux, (char*)workspace, p.layout(B), B, (hipStream_t)stream};
    double* ld = E.at<double>(E.L.ld);
    run_coupling(E, p.couplings[p.layers[layer].ci], in, out, logdet_accum ? ld : nullptr, dir);
    if (logdet_accum) {
        const int np = E.L.ld_parts, negate = dir < 0 ? 1 : 0;
        E.record("k_ld_reduce", 0, 0,
                 [=](void* st) { launch_ld_reduce(ld, logdet_accum, B, 1, np, 1, (hipStream_t)st, negate); });
    }
    check_launch();
    return CNF_OK;
    CNF_CATCH
}

// cnf_flow_backward (count null: the loss scaled by inv_batch) and cnf_flow_backward_ex
int flow_backward_entry(cnf_plan* plan, const float* params, const float* xy, const float* zy, void* train_workspace,
                        int B, float inv_batch, const float* count, float* dparams, cnf_layer_done_fn done, void* user,
                        void* stream) {
    OptScope os_(plan ? &plan->p->opts : nullptr);
    if (!plan || !params || !xy || !zy || !train_workspace || !dparams || B <= 0) return fail(CNF_E_INVALID, kNullOrB);
    CNF_TRY
    Plan& p = *plan->p;
    ensure_tables(p);
    flow_backward(p, params, xy, zy, train_workspace, B, inv_batch, dparams, (hipStream_t)stream, count, done, user);
    return CNF_OK;
    CNF_CATCH
}

}  // namespace

extern "C" {

int cnf_flow_forward(cnf_plan* plan, const float* params, const float* aux, const float* xy, float* zy,
                     float* logdet_per_image, void* workspace, int B, void* stream) {
    OptScope os_(plan ? &plan->p->opts : nullptr);
    if (int e = flow_args_error(plan && params && aux && xy && zy && logdet_per_image && workspace, B, xy, zy, +1))
        return e;
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
        return fail(CNF_E_INVALID, kNullOrB);
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

int cnf_flow_forward_train(cnf_plan* plan, const float* params, const float* aux, const float* xy, float* zy,
                           float* logdet_per_image, void* train_workspace, int B, void* stream) {
    OptScope os_(plan ? &plan->p->opts : nullptr);
    if (int e = flow_args_error(plan && params && aux && xy && zy && logdet_per_image && train_workspace, B, xy, zy, +1))
        return e;
    CNF_TRY
    flow_forward(*plan->p, params, aux, xy, zy, logdet_per_image, train_workspace, B, (hipStream_t)stream, true);
    return CNF_OK;
    CNF_CATCH
}

int cnf_flow_inverse(cnf_plan* plan, const float* params, const float* aux, const float* zy, float* xy,
                     void* workspace, int B, void* stream) {
    OptScope os_(plan ? &plan->p->opts : nullptr);
    if (int e = flow_args_error(plan && params && aux && xy && zy && workspace, B, zy, xy, -1)) return e;
    CNF_TRY
    flow_inverse(*plan->p, params, aux, zy, xy, workspace, B, (hipStream_t)stream);
    return CNF_OK;
    CNF_CATCH
}

int cnf_flow_inverse_logdet(cnf_plan* plan, const float* params, const float* aux, const float* zy, float* xy,
                            float* logdet_per_image, void* workspace, int B, void* stream) {
    OptScope os_(plan ? &plan->p->opts : nullptr);
    if (int e = flow_args_error(plan && params && aux && xy && zy && logdet_per_image && workspace, B, zy, xy, -1))
        return e;
    CNF_TRY
    InverseOpts io;
    io.logdet_per_image = logdet_per_image;
    flow_inverse(*plan->p, params, aux, zy, xy, workspace, B, (hipStream_t)stream, io);
    return CNF_OK;
    CNF_CATCH
}

int cnf_flow_backward_ex(cnf_plan* plan, const float* params, const float* xy, const float* zy, void* train_workspace,
                         int B, const float* global_count, float* dparams, cnf_layer_done_fn layer_done, void* user,
                         void* stream) {
    if (!global_count) return fail(CNF_E_INVALID, kNullOrB);
    return flow_backward_entry(plan, params, xy, zy, train_workspace, B, 0.f, global_count, dparams, layer_done, user,
                               stream);
}

int cnf_flow_backward(cnf_plan* plan, const float* params, const float* xy, const float* zy, void* train_workspace,
                      int B, float inv_batch, float* dparams, void* stream) {
    return flow_backward_entry(plan, params, xy, zy, train_workspace, B, inv_batch, nullptr, dparams, nullptr, nullptr,
                               stream);
}

int cnf_coupling_forward(cnf_plan* plan, int layer, const float* params, const float* aux, const float* u, float* v,
                         float* logdet_accum, void* workspace, int B, void* stream) {
    return single_coupling(plan, layer, params, aux, u, v, logdet_accum, workspace, B, stream, +1);
}

int cnf_coupling_inverse(cnf_plan* plan, int layer, const float* params, const float* aux, const float* v, float* u,
                         void* workspace, int B, void* stream) {
    return single_coupling(plan, layer, params, aux, v, u, nullptr, workspace, B, stream, -1);
}

int cnf_coupling_inverse_logdet(cnf_plan* plan, int layer, const float* params, const float* aux, const float* v,
                                float* u, float* logdet_accum, void* workspace, int B, void* stream) {
    return single_coupling(plan, layer, params, aux, v, u, logdet_accum, workspace, B, stream, -1);
}

int cnf_coupling_backward(cnf_plan* plan, int layer, const float* params, const float* u, const float* dv, float* du,
                          float dlogdet, void* train_workspace, int B, float* dparams, void* stream) {
    OptScope os_(plan ? &plan->p->opts : nullptr);
    if (!plan || !params || !u || !dv || !du || !train_workspace || !dparams || B <= 0)
        return fail(CNF_E_INVALID, kNullOrB);
    CNF_TRY
    Plan& p = *plan->p;
    if (layer < 0 || layer >= (int)p.layers.size() || p.layers[layer].kind != CNF_LAYER_COUPLING)
        return fail(CNF_E_INVALID, kNotCoupling);
    if (du == dv || du == u) return fail(CNF_E_INVALID, "du must not alias u or dv");
    ensure_tables(p);
    coupling_layer_backward(p, p.layers[layer].ci, params, u, dv, du, dlogdet, train_workspace, B, dparams,
                            (hipStream_t)stream);
    return CNF_OK;
    CNF_CATCH
}

}  // extern "C"
