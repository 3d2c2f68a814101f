// cnf_logprob.cpp — the density of given images (include/cnf.h cnf_flow_log_prob; kernels: cnf_logprob.hip):
// per chunk of (image, condition) pairs the gather into the flow's input space, the forward schedule
// (cnf_schedule.cpp) and the pass that finishes the terms; then the posterior over the conditions.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "cnf_sampling.h"

using namespace cnf;

namespace {

// the log_prob workspace: the forward workspace of `chunk` images, then one chunk each of xy, zy, the
// forward's fp32 log-det [chunk] and the log_jac partials [chunk][logp_parts] (fp64). Nothing scales with B
// or K.
struct LogpLayout {
    size_t xy = 0, zy = 0, ld = 0, lj = 0, total = 0;
};
LogpLayout logp_layout(const Plan& p, int chunk) {
    const cnf_flow_desc& d = p.desc;
    const size_t n_uv = (size_t)d.io_h * d.io_w * d.io_d;
    LogpLayout L;
    WsCarver ws(p.layout(chunk).total);
    L.xy = ws.take((size_t)chunk * n_uv * 4);
    L.zy = ws.take((size_t)chunk * n_uv * 4);
    L.ld = ws.take((size_t)chunk * 4);
    L.lj = ws.take((size_t)chunk * logp_parts(d.io_h * d.io_w) * 8);
    L.total = ws.off;
    return L;
}

// the argument errors of cnf_flow_log_prob that need no pointer but the descriptor (null: fine)
const char* logp_desc_error(const Plan& p, int B, const cnf_logp_desc* s) {
    if (s == nullptr) return "null log_prob descriptor";
    if (B < 1) return "B must be >= 1";
    if (s->num_conditions < 0) return "num_conditions must be >= 1 (pairwise) or 0 (paired)";
    if (s->chunk < 1) return "chunk must be >= 1";
    return post_transform_error(p, s->logit_a, s->residual, LogitWord::logit_map);
}

}  // namespace

extern "C" {

size_t cnf_plan_logp_workspace_bytes(const cnf_plan* plan, int B, const cnf_logp_desc* desc) {
    OptScope os_(plan ? &plan->p->opts : nullptr);
    const std::string w("cnf_plan_logp_workspace_bytes: ");
    if (!plan) {
        (void)fail(CNF_E_INVALID, w + "null plan");
        return 0;
    }
    if (const char* e = logp_desc_error(*plan->p, B, desc)) {   // (the message for cnf_last_error)
        (void)fail(CNF_E_INVALID, w + e);
        return 0;
    }
    return logp_layout(*plan->p, desc->chunk).total;
}

int cnf_flow_log_prob(cnf_plan* plan, const float* params, const float* aux, const float* x, const float* y,
                      const cnf_logp_desc* desc, float* log_prob, float* llz, float* logdet, float* log_jac,
                      float* y_dev, const float* log_prior, float* posterior, float* log_evidence, void* workspace,
                      int B, void* stream) {
    OptScope os_(plan ? &plan->p->opts : nullptr);
    const std::string w("cnf_flow_log_prob: ");
    if (!plan || !params || !aux || !workspace) return fail(CNF_E_INVALID, w + "null argument");
    if (!x) return fail(CNF_E_INVALID, w + "null x");
    if (!y) return fail(CNF_E_INVALID, w + "null y");
    if (!log_prob && !llz && !logdet && !log_jac && !y_dev && !posterior && !log_evidence)
        return fail(CNF_E_INVALID, w + "no output requested (log_prob, llz, logdet, log_jac, y_dev, posterior, "
                                       "log_evidence all null)");
    if (const char* e = logp_desc_error(*plan->p, B, desc)) return fail(CNF_E_INVALID, w + e);
    const bool post = posterior != nullptr || log_evidence != nullptr;
    if (post && desc->num_conditions < 1)
        return fail(CNF_E_INVALID, w + "posterior and log_evidence need num_conditions >= 1 (pairwise)");
    if (post && !log_prob) return fail(CNF_E_INVALID, w + "posterior and log_evidence need log_prob");
    if (log_prior && !post) return fail(CNF_E_INVALID, w + "log_prior needs posterior or log_evidence");
    CNF_TRY
    Plan& p = *plan->p;
    const cnf_flow_desc& d = p.desc;
    ensure_tables(p);
    p.recorded.clear();
    const LogpLayout LL = logp_layout(p, desc->chunk);
    char* ws = (char*)workspace;
    float* xy = reinterpret_cast<float*>(ws + LL.xy);
    float* zy = reinterpret_cast<float*>(ws + LL.zy);
    float* ld = reinterpret_cast<float*>(ws + LL.ld);
    double* lj = reinterpret_cast<double*>(ws + LL.lj);
    const int K = desc->num_conditions, HW = d.io_h * d.io_w;
    LogpGatherArgs ga;
    std::memset(&ga, 0, sizeof(ga));
    ga.x = x;
    ga.y = y;
    ga.xy = xy;
    ga.lj = lj;
    ga.logit = desc->logit_a != 0.f ? 1 : 0;
    ga.residual = desc->residual != 0 ? 1 : 0;
    LogpFinishArgs fa;
    std::memset(&fa, 0, sizeof(fa));
    fa.zy = zy;
    fa.y = y;
    fa.ld = ld;
    fa.lj = lj;
    fa.log_prob = log_prob;
    fa.llz = llz;
    fa.logdet = logdet;
    fa.log_jac = log_jac;
    fa.y_dev = y_dev;
    if (ga.logit) {
        // the part of log|dv/dx| every element shares, from the constants the map runs on
        ga.lk = logit_consts(desc->logit_a);
        fa.lj_const = (double)HW * d.x_d * (std::log((double)ga.lk.c1) - std::log((double)ga.lk.span));
    }
    const long long total = K > 0 ? (long long)B * K : (long long)B;
    const double px = (double)HW;
    const int parts = logp_parts(HW);
    for (long long g0 = 0; g0 < total; g0 += desc->chunk) {
        const int n = (int)std::min<long long>(desc->chunk, total - g0);
        const LogpChunk c{g0, n, K, HW, d.io_d, d.x_d};
        Exec E{p, params, aux, ws, p.layout(n), n, (hipStream_t)stream};
        // x of an image once (its pairs share it through L2), y and xy per pair
        const double nimg = K > 0 ? (double)((g0 + n - 1) / K - g0 / K + 1) : (double)n;
        E.record("k_logp_gather", 0, 4.0 * px * (nimg * d.x_d + n * (2.0 * d.io_d - d.x_d)) + 8.0 * n * parts,
                 [=](void* st) { launch_logp_gather(c, ga, (hipStream_t)st); });
        flow_forward(p, params, aux, xy, zy, ld, ws, n, (hipStream_t)stream, false, nullptr, /*append=*/true);
        E.record("k_logp_finish", 0, 4.0 * n * px * (2.0 * d.io_d - d.x_d) + n * (4.0 + 8.0 * parts),
                 [=](void* st) { launch_logp_finish(c, fa, (hipStream_t)st); });
    }
    if (post) {
        Exec E{p, params, aux, ws, p.layout(1), 1, (hipStream_t)stream};
        E.record("k_logp_posterior", 0, 4.0 * B * K * (posterior ? 2.0 : 1.0),
                 [=](void* st) { launch_logp_posterior(log_prob, log_prior, posterior, log_evidence, B, K, (hipStream_t)st); });
    }
    check_launch();
    return CNF_OK;
    CNF_CATCH
}

}  // extern "C"
