// cnf_score.cpp — the input gradients of the log-density (include/cnf.h cnf_flow_score, cnf_flow_ascend;
// kernels: cnf_score.hip): per chunk of paired images cnf_flow_log_prob's gather, the training forward
// (cnf_schedule.cpp), the seed, the data-gradient-only backward (cnf_train.cpp flow_backward_data) and the pass
// that takes the gradient through the gather's map -- or, for the ascent, the Adam step on the chunk's xy.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <stdexcept>
#include <string>

#include "cnf_sampling.h"

using namespace cnf;

namespace {

// The workspace of both calls: the train workspace of `chunk` images; the dense backward image and the zeros
// block, packed once per call (the train layout of a ragged last chunk places its own elsewhere); one chunk each
// of xy, zy, the seed dzy, the forward's fp32 log-det [chunk], the log_jac partials [chunk][logp_parts] and llz
// [chunk] (fp64); for the ascent the chunk's Adam state m, v [chunk][HW][x_d] (used when the caller gives none).
// Nothing scales with B. The backward's scratch for the parameter outputs of the kernels that produce both kinds
// of gradient (k_lnb_apply's lnpart, k_lds_bwd's rows, k_coup_bw's dwpart) is the train layout's own.
struct ScoreLayout {
    size_t train = 0, bw = 0, zeros = 0, xy = 0, zy = 0, dzy = 0, ld = 0, lj = 0, llz = 0, m = 0, v = 0, total = 0;
};
ScoreLayout score_layout(const Plan& p, int chunk, bool ascend) {
    const cnf_flow_desc& d = p.desc;
    const size_t HW = (size_t)d.io_h * d.io_w, n_uv = HW * d.io_d;
    ScoreLayout L;
    L.train = p.train_layout(chunk).total;
    WsCarver ws(L.train);
    L.bw = ws.take((size_t)std::max<int64_t>(p.n_bw, 1) * 4);
    L.zeros = ws.take(64 * 4);
    L.xy = ws.take((size_t)chunk * n_uv * 4);
    L.zy = ws.take((size_t)chunk * n_uv * 4);
    L.dzy = ws.take((size_t)chunk * n_uv * 4);
    L.ld = ws.take((size_t)chunk * 4);
    L.lj = ws.take((size_t)chunk * logp_parts((int)HW) * 8);
    L.llz = ws.take((size_t)chunk * 8);
    if (ascend) {
        L.m = ws.take((size_t)chunk * HW * d.x_d * 4);
        L.v = ws.take((size_t)chunk * HW * d.x_d * 4);
    }
    L.total = ws.off;
    return L;
}

const char* score_desc_error(const Plan& p, int B, const cnf_score_desc* s) {
    if (s == nullptr) return "null score descriptor";
    if (B < 1) return "B must be >= 1";
    if (s->chunk < 1) return "chunk must be >= 1";
    return post_transform_error(p, s->logit_a, s->residual, LogitWord::logit_map);
}

const char* ascend_desc_error(const Plan& p, int B, const cnf_ascend_desc* s) {
    if (s == nullptr) return "null ascend descriptor";
    if (B < 1) return "B must be >= 1";
    if (s->chunk < 1) return "chunk must be >= 1";
    if (s->steps < 0) return "steps must be >= 0";
    if (s->first_step < 0) return "first_step must be >= 0";
    if (!std::isfinite(s->lr)) return "lr must be finite";
    if (!(s->beta_1 >= 0.f && s->beta_1 < 1.f) || !(s->beta_2 >= 0.f && s->beta_2 < 1.f))
        return "beta_1 and beta_2 must be in [0, 1)";
    if (!(s->epsilon >= 0.f) || !std::isfinite(s->epsilon)) return "epsilon must be finite and >= 0";
    return post_transform_error(p, s->logit_a, s->residual, LogitWord::logit_map);
}

// what the two calls share per chunk: the buffers, the gather and one forward + seed (+ backward) at the chunk's xy
struct ChunkRun {
    Plan& p;
    const float* params;
    const float* aux;
    char* ws;
    const ScoreLayout& L;
    hipStream_t st;
    int HW, parts;
    float *xy, *zy, *dzy, *ld;
    double *lj, *llz;

    ChunkRun(Plan& p_, const float* params_, const float* aux_, void* workspace, const ScoreLayout& L_, void* stream)
        : p(p_), params(params_), aux(aux_), ws((char*)workspace), L(L_), st((hipStream_t)stream),
          HW(p_.desc.io_h * p_.desc.io_w), parts(logp_parts(HW)), xy((float*)(ws + L_.xy)), zy((float*)(ws + L_.zy)),
          dzy((float*)(ws + L_.dzy)), ld((float*)(ws + L_.ld)), lj((double*)(ws + L_.lj)), llz((double*)(ws + L_.llz)) {}

    Exec exec(int n) const { return Exec{p, params, aux, ws, p.layout(n), n, st}; }

    // the dense backward image and the zeros block, once per native call
    void pack() const { pack_backward_image(p, params, (float*)(ws + L.bw), (float*)(ws + L.zeros), st); }

    LogpChunk chunk(long long g0, int n) const {
        const cnf_flow_desc& d = p.desc;
        if (p.train_layout(n).total > L.train) throw std::logic_error("train layout of a chunk exceeds the workspace's");
        return LogpChunk{g0, n, 0, HW, d.io_d, d.x_d};
    }

    void gather(const LogpChunk& c, LogpGatherArgs ga) const {
        const cnf_flow_desc& d = p.desc;
        ga.xy = xy;
        ga.lj = lj;
        Exec E = exec(c.n);
        E.record("k_logp_gather", 0, 4.0 * HW * c.n * 2.0 * d.io_d + 8.0 * c.n * parts,
                 [=](void* s) { launch_logp_gather(c, ga, (hipStream_t)s); });
    }

    // the training forward at xy, then the seed (with_dzy) and llz; trace (may be null): this iterate's row
    void forward_seed(const LogpChunk& c, bool with_dzy, float* trace, bool domain) const {
        const cnf_flow_desc& d = p.desc;
        flow_forward(p, params, aux, xy, zy, ld, ws, c.n, st, /*save_inputs=*/true, nullptr, /*append=*/true);
        ScoreSeedArgs sa;
        std::memset(&sa, 0, sizeof(sa));
        sa.zy = zy;
        sa.dzy = with_dzy ? dzy : nullptr;
        sa.llz = llz;
        sa.ld = ld;
        sa.lj = domain ? lj : nullptr;
        sa.trace = trace;
        Exec E = exec(c.n);
        E.record("k_score_seed", 0, 4.0 * c.n * HW * d.io_d * (with_dzy ? 2.0 : 1.0),
                 [=](void* s) { launch_score_seed(c, sa, (hipStream_t)s); });
    }

    // d(llz + logdet)/dxy of the chunk, in the train workspace
    const float* backward(const LogpChunk& c) const {
        return flow_backward_data(p, params, (const float*)(ws + L.bw), (const float*)(ws + L.zeros), dzy, ws, c.n, st);
    }
};

LogpGatherArgs gather_args(const float* x, const float* y, float logit_a, int residual) {
    LogpGatherArgs ga;
    std::memset(&ga, 0, sizeof(ga));
    ga.x = x;
    ga.y = y;
    ga.logit = logit_a != 0.f ? 1 : 0;
    ga.residual = residual != 0 ? 1 : 0;
    if (ga.logit) ga.lk = logit_consts(logit_a);
    return ga;
}

}  // namespace

extern "C" {

size_t cnf_plan_score_workspace_bytes(const cnf_plan* plan, int B, const cnf_score_desc* desc) {
    OptScope os_(plan ? &plan->p->opts : nullptr);
    const std::string w("cnf_plan_score_workspace_bytes: ");
    if (!plan) {
        (void)fail(CNF_E_INVALID, w + "null plan");
        return 0;
    }
    if (const char* e = score_desc_error(*plan->p, B, desc)) {
        (void)fail(CNF_E_INVALID, w + e);
        return 0;
    }
    try {
        return score_layout(*plan->p, desc->chunk, false).total;
    } catch (...) {
        (void)caught();
        return 0;
    }
}

int cnf_flow_score(cnf_plan* plan, const float* params, const float* aux, const float* x, const float* y,
                   const cnf_score_desc* desc, float* grad_x, float* grad_y, float* log_prob, void* workspace, int B,
                   void* stream) {
    OptScope os_(plan ? &plan->p->opts : nullptr);
    const std::string w("cnf_flow_score: ");
    if (!plan || !params || !aux || !workspace) return fail(CNF_E_INVALID, w + "null argument");
    if (!x) return fail(CNF_E_INVALID, w + "null x");
    if (!y) return fail(CNF_E_INVALID, w + "null y");
    if (!grad_x && !grad_y && !log_prob)
        return fail(CNF_E_INVALID, w + "no output requested (grad_x, grad_y, log_prob all null)");
    if (const char* e = score_desc_error(*plan->p, B, desc)) return fail(CNF_E_INVALID, w + e);
    CNF_TRY
    Plan& p = *plan->p;
    const cnf_flow_desc& d = p.desc;
    ensure_tables(p);
    p.recorded.clear();
    const ScoreLayout L = score_layout(p, desc->chunk, false);
    const ChunkRun R(p, params, aux, workspace, L, stream);
    const bool grads = grad_x != nullptr || grad_y != nullptr;
    const LogpGatherArgs ga = gather_args(x, y, desc->logit_a, desc->residual);
    ScoreFinishArgs fa;
    std::memset(&fa, 0, sizeof(fa));
    fa.x = x;
    fa.y = y;
    fa.llz = R.llz;
    fa.ld = R.ld;
    fa.lj = R.lj;
    fa.grad_x = grad_x;
    fa.grad_y = grad_y;
    fa.log_prob = log_prob;
    fa.logit = ga.logit;
    fa.residual = ga.residual;
    fa.lk = ga.lk;
    if (ga.logit)   // (cnf_flow_log_prob's constant part of log|dv/dx|)
        fa.lj_const = (double)R.HW * d.x_d * (std::log((double)ga.lk.c1) - std::log((double)ga.lk.span));
    if (grads) R.pack();
    for (long long g0 = 0; g0 < B; g0 += desc->chunk) {
        const int n = (int)std::min<long long>(desc->chunk, B - g0);
        const LogpChunk c = R.chunk(g0, n);
        R.gather(c, ga);
        R.forward_seed(c, grads, nullptr, false);
        fa.g = grads ? R.backward(c) : nullptr;
        const ScoreFinishArgs f = fa;
        Exec E = R.exec(n);
        E.record("k_score_finish", 0, 4.0 * n * R.HW * (grads ? 3.0 * d.io_d : 0.0) + n * (16.0 + 8.0 * R.parts),
                 [=](void* s) { launch_score_finish(c, f, (hipStream_t)s); });
    }
    check_launch();
    return CNF_OK;
    CNF_CATCH
}

size_t cnf_plan_ascend_workspace_bytes(const cnf_plan* plan, int B, const cnf_ascend_desc* desc) {
    OptScope os_(plan ? &plan->p->opts : nullptr);
    const std::string w("cnf_plan_ascend_workspace_bytes: ");
    if (!plan) {
        (void)fail(CNF_E_INVALID, w + "null plan");
        return 0;
    }
    if (const char* e = ascend_desc_error(*plan->p, B, desc)) {
        (void)fail(CNF_E_INVALID, w + e);
        return 0;
    }
    try {
        return score_layout(*plan->p, desc->chunk, true).total;
    } catch (...) {
        (void)caught();
        return 0;
    }
}

int cnf_flow_ascend(cnf_plan* plan, const float* params, const float* aux, const float* x0, const float* y,
                    const cnf_ascend_desc* desc, float* x_out, float* log_prob_trace, float* m, float* v,
                    void* workspace, int B, void* stream) {
    OptScope os_(plan ? &plan->p->opts : nullptr);
    const std::string w("cnf_flow_ascend: ");
    if (!plan || !params || !aux || !workspace) return fail(CNF_E_INVALID, w + "null argument");
    if (!x0) return fail(CNF_E_INVALID, w + "null x0");
    if (!y) return fail(CNF_E_INVALID, w + "null y");
    if (!x_out) return fail(CNF_E_INVALID, w + "null x_out");
    if (!log_prob_trace) return fail(CNF_E_INVALID, w + "null log_prob_trace");
    if ((m == nullptr) != (v == nullptr)) return fail(CNF_E_INVALID, w + "m and v must be given together");
    if (const char* e = ascend_desc_error(*plan->p, B, desc)) return fail(CNF_E_INVALID, w + e);
    CNF_TRY
    Plan& p = *plan->p;
    const cnf_flow_desc& d = p.desc;
    ensure_tables(p);
    p.recorded.clear();
    const ScoreLayout L = score_layout(p, desc->chunk, true);
    const ChunkRun R(p, params, aux, workspace, L, stream);
    const LogpGatherArgs ga = gather_args(x0, y, desc->logit_a, desc->residual);
    const size_t nx = (size_t)R.HW * d.x_d;   // x elements per image
    if (desc->steps > 0) R.pack();
    for (long long g0 = 0; g0 < B; g0 += desc->chunk) {
        const int n = (int)std::min<long long>(desc->chunk, B - g0);
        const LogpChunk c = R.chunk(g0, n);
        Exec E = R.exec(n);
        R.gather(c, ga);
        AscendStepArgs sa;
        std::memset(&sa, 0, sizeof(sa));
        sa.xy = R.xy;
        sa.b1 = desc->beta_1;
        sa.b2 = desc->beta_2;
        sa.eps = desc->epsilon;
        if (m != nullptr) {
            sa.m = m + (size_t)g0 * nx;
            sa.v = v + (size_t)g0 * nx;
        } else if (desc->steps > 0) {   // the chunk's state in the workspace, from zero
            sa.m = (float*)(R.ws + L.m);
            sa.v = (float*)(R.ws + L.v);
            hip_check(hipMemsetAsync(sa.m, 0, (size_t)n * nx * 4, R.st), "hipMemsetAsync");
            hip_check(hipMemsetAsync(sa.v, 0, (size_t)n * nx * 4, R.st), "hipMemsetAsync");
        }
        for (int t = 0; t < desc->steps; t++) {
            R.forward_seed(c, true, log_prob_trace + (size_t)t * B, true);
            sa.g = R.backward(c);
            // Keras Adam's step size at step first_step + t + 1 (cnf_adam_step's expression)
            const int step = desc->first_step + t + 1;
            const double b1t = std::pow((double)desc->beta_1, step), b2t = std::pow((double)desc->beta_2, step);
            sa.alpha = (float)((double)desc->lr * std::sqrt(1.0 - b2t) / (1.0 - b1t));
            const AscendStepArgs s1 = sa;
            E.record("k_ascend_step", 0, 4.0 * n * nx * 7.0,
                     [=](void* s) { launch_ascend_step(c, s1, (hipStream_t)s); });
        }
        R.forward_seed(c, false, log_prob_trace + (size_t)desc->steps * B, true);
        AscendOutArgs oa;
        std::memset(&oa, 0, sizeof(oa));
        oa.xy = R.xy;
        oa.x0 = x0;
        oa.y = y;
        oa.lj = R.lj;
        oa.x_out = x_out;
        oa.logit = ga.logit;
        oa.residual = ga.residual;
        oa.lk = ga.lk;
        E.record("k_ascend_out", 0, 4.0 * n * nx * 3.0, [=](void* s) { launch_ascend_out(c, oa, (hipStream_t)s); });
    }
    check_launch();
    return CNF_OK;
    CNF_CATCH
}

}  // extern "C"
