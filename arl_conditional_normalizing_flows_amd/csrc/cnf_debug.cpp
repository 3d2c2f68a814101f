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
