// cnf_sampling.cpp — conditional sampling (include/cnf.h cnf_flow_sample; kernels: cnf_sample.hip): latents
// per chunk, the inverse schedule (cnf_schedule.cpp) and the folds of the draws into the outputs.
#include <algorithm>
#include <cmath>
#include <string>

#include "cnf_sampling.h"

using namespace cnf;

namespace cnf {

SampleLayout sample_layout(const Plan& p, int B, int chunk) {
    const cnf_flow_desc& d = p.desc;
    const size_t n_uv = (size_t)d.io_h * d.io_w * d.io_d;
    SampleLayout L;
    WsCarver ws(p.layout(chunk).total);
    L.zy = ws.take((size_t)chunk * n_uv * 4);
    L.xy = ws.take((size_t)chunk * n_uv * 4);
    L.state = ws.take((size_t)3 * B * d.io_h * d.io_w * d.x_d * 4);
    L.total = ws.off;
    return L;
}

const char* post_transform_error(const Plan& p, float logit_a, int residual, LogitWord zero_means) {
    if (logit_a != 0.f && !(logit_a > 0.f && logit_a < 0.5f))
        return zero_means == LogitWord::delogitify ? "logit_a must be 0 (no de_logitify) or in (0, 0.5)"
                                                   : "logit_a must be 0 (no logit map) or in (0, 0.5)";
    if (residual != 0 && p.desc.io_d - p.desc.x_d != p.desc.x_d)
        return "residual needs y of x's depth (io_d - x_d == x_d)";
    return nullptr;
}

// the argument errors of cnf_flow_sample that need no pointer but the descriptor (null: fine)
const char* sample_desc_error(const Plan& p, int B, const cnf_sample_desc* s) {
    if (s == nullptr) return "null sample descriptor";
    if (B < 1) return "B must be >= 1";
    if (s->num_samples < 1) return "num_samples must be >= 1";
    if (s->chunk < 1) return "chunk must be >= 1";
    if (!(s->temperature >= 0.f) || std::isinf(s->temperature)) return "temperature must be finite and >= 0";
    return post_transform_error(p, s->logit_a, s->residual, LogitWord::delogitify);
}

// the argument errors of the score part (no output given: none)
const char* score_error(const ScoreArgs& sc) {
    if (!sc.any()) return nullptr;
    const cnf_sample_score_desc* sd = sc.sd;
    if (sd == nullptr) return "null score descriptor";
    if ((sc.rank || sc.abs_err || sc.sq_err) && !sc.truth) return "rank, abs_err and sq_err need truth";
    if (sc.quantiles && !sc.hist) return "quantiles needs hist";
    if (sc.hist && sd->bins == 0) return "hist needs bins != 0";
    if (sd->bins != 0) {
        if (sd->bins < 2 || sd->bins > SCORE_MAX_BINS) return "bins must be in 2..256";
        if (!std::isfinite(sd->lo) || !std::isfinite(sd->hi)) return "lo and hi must be finite";
        if (!(sd->lo < sd->hi)) return "lo must be below hi";
        if (!std::isfinite((float)sd->bins / (sd->hi - sd->lo))) return "lo / hi: the bin scale is not finite";
    }
    if (sc.quantiles) {
        if (sd->num_quantiles < 1 || sd->num_quantiles > SCORE_MAX_QUANTILES) return "num_quantiles must be in 1..8";
        for (int j = 0; j < sd->num_quantiles; j++)
            if (!(sd->quantiles[j] >= 0.f && sd->quantiles[j] <= 1.f)) return "quantiles: every level must be in [0, 1]";
    }
    return nullptr;
}

void record_chunk_outputs(Exec& E, const SampleChunk& c, const DrawView& v, const ChunkOutputs& o) {
    const ScoreArgs& sc = o.sc;
    const int n = c.n, per = c.HW * c.x_d;   // elements per condition
    const bool node = v.node();
    const auto name = [&](const char* k) { return std::string(k) + (node ? "_node" : ""); };
    const double xs = 4.0 * n * (double)c.HW * c.x_d;   // the chunk's x_hat once
    const int cond = node && v.residual ? 1 : 0;        // ... and, in node form, its condition with every draw
    if (o.samples != nullptr || o.state != nullptr) {
        const SampleFoldArgs fa{v, o.samples, o.state, o.mean, o.std, o.B};
        E.record(name("k_sample_fold"), 0, xs * ((o.samples ? 2 : 1) + cond),
                 [=](void* st) { launch_sample_fold(c, fa, (hipStream_t)st); });
    }
    if (o.y_dev != nullptr) {
        float* y_dev = o.y_dev;
        E.record(name("k_sample_ydev"), 0, 8.0 * n * (double)c.HW * (c.D - c.x_d),
                 [=](void* st) { launch_sample_ydev(c, v, y_dev, (hipStream_t)st); });
    }
    if (o.block_dev != nullptr) {
        const BlockDevArgs ba{v, o.block_dev, E.p.desc.io_w};
        E.record("k_block_dev", 0, 2 * xs, [=](void* st) { launch_block_dev(c, ba, (hipStream_t)st); });
    }
    if (o.log_prob != nullptr) {
        // the slots the chunk's inverse just wrote
        const double* ld = E.at<double>(E.L.ld);
        const int nl = (int)E.p.couplings.size(), np = E.L.ld_parts;
        float* log_prob = o.log_prob;
        E.record("k_sample_logp", 0, xs + 8.0 * n * nl * np,
                 [=](void* st) { launch_sample_logp(c, v.zy, ld, nl, np, log_prob, (hipStream_t)st); });
    }
    if (sc.rank || sc.abs_err || sc.hist) {
        SampleScoreArgs sa{v, sc.truth, sc.rank, sc.abs_err, sc.hist, 0, 0.f, 0.f};
        if (sc.hist) {
            sa.bins = sc.sd->bins;
            sa.lo = sc.sd->lo;
            sa.scale = (float)sc.sd->bins / (sc.sd->hi - sc.sd->lo);
        }
        // per touched condition the truth and the read-modify-write of the outputs
        const double nb = (double)((c.g0 + n - 1) / c.S - c.g0 / c.S + 1);
        const double rmw = (sc.rank ? 8.0 : 0.0) + (sc.abs_err ? 8.0 : 0.0) + (sc.hist ? 8.0 * sa.bins : 0.0);
        E.record(name("k_sample_score"), 0, xs * (1 + cond) + nb * per * ((sc.truth ? 4.0 : 0.0) + rmw),
                 [=](void* st) { launch_sample_score(c, sa, (hipStream_t)st); });
    }
    if (sc.sq_err != nullptr) {
        const SampleSqerrArgs qa{v, sc.truth, sc.sq_err};
        E.record(name("k_sample_sqerr"), 0, xs * (2 + cond), [=](void* st) { launch_sample_sqerr(c, qa, (hipStream_t)st); });
    }
}

void record_quantiles(Exec& E, const ScoreArgs& sc, long long n) {
    SampleQuantileArgs ua{sc.hist, sc.quantiles, n, sc.sd->bins, sc.sd->num_quantiles, sc.sd->lo, sc.sd->hi, {}};
    for (int j = 0; j < ua.nq; j++) ua.q[j] = sc.sd->quantiles[j];
    E.record("k_sample_quantiles", 0, 4.0 * (double)ua.n * (ua.bins + ua.nq),   // (the second walk hits the cache)
             [=](void* st) { launch_sample_quantiles(ua, (hipStream_t)st); });
}

}  // namespace cnf

namespace {

// the body of cnf_flow_sample (log_prob null: its launches, exactly), cnf_flow_sample_logp and
// cnf_flow_sample_score (every score output null: cnf_flow_sample_logp's launches, exactly)
int flow_sample(const char* who, cnf_plan* plan, const float* params, const float* aux, const float* y,
                const cnf_sample_desc* desc, float* samples, float* mean, float* std, float* y_dev, float* log_prob,
                void* workspace, int B, void* stream, const ScoreArgs& sc = ScoreArgs()) {
    OptScope os_(plan ? &plan->p->opts : nullptr);
    const std::string w(who);
    if (!plan || !params || !aux || !workspace) return fail(CNF_E_INVALID, w + ": null argument");
    if (!y) return fail(CNF_E_INVALID, w + ": null y");
    if (const char* e = sample_desc_error(*plan->p, B, desc)) return fail(CNF_E_INVALID, w + ": " + e);
    if (const char* e = score_error(sc)) return fail(CNF_E_INVALID, w + ": " + e);
    if (!samples && !mean && !std && !y_dev && !log_prob && !sc.any())
        return fail(CNF_E_INVALID, w + ": no output requested (samples, mean, std, y_dev" +
                                       (w == "cnf_flow_sample" ? "" : ", log_prob") +
                                       (w == "cnf_flow_sample_score" ? ", rank, abs_err, sq_err, hist, quantiles" : "") +
                                       " all null)");
    CNF_TRY
    Plan& p = *plan->p;
    const cnf_flow_desc& d = p.desc;
    ensure_tables(p);
    p.recorded.clear();
    const SampleLayout SL = sample_layout(p, B, desc->chunk);
    char* ws = (char*)workspace;
    float* zy = reinterpret_cast<float*>(ws + SL.zy);
    float* xy = reinterpret_cast<float*>(ws + SL.xy);
    DrawView v{xy, zy, y, desc->logit_a != 0.f ? 1 : 0, desc->residual != 0 ? 1 : 0, LogitK{}};
    if (v.logit) v.lk = logit_consts(desc->logit_a);
    float* const state = mean != nullptr || std != nullptr ? reinterpret_cast<float*>(ws + SL.state) : nullptr;
    const ChunkOutputs out{samples, state, mean, std, y_dev, /*block_dev=*/nullptr, log_prob, sc, B};
    const float T = desc->temperature;
    const unsigned long long seed = desc->seed, off = desc->offset;
    const long long total = (long long)B * desc->num_samples;
    const double px = (double)d.io_h * d.io_w;
    InverseOpts io;
    io.append = true;                   // one recording for the whole call
    io.ld_slots = log_prob != nullptr;  // k_sample_logp reads the slots: no reduce launch per chunk
    for (long long g0 = 0; g0 < total; g0 += desc->chunk) {
        const int n = (int)std::min<long long>(desc->chunk, total - g0);
        const SampleChunk c{g0, n, desc->num_samples, d.io_h * d.io_w, d.io_d, d.x_d};
        Exec E{p, params, aux, ws, p.layout(n), n, (hipStream_t)stream};
        E.record("k_latent", 0, 4.0 * n * px * (2 * d.io_d - d.x_d),
                 [=](void* st) { launch_latent(c, y, zy, T, seed, off, (hipStream_t)st); });
        flow_inverse(p, params, aux, zy, xy, ws, n, (hipStream_t)stream, io);
        record_chunk_outputs(E, c, v, out);
    }
    if (sc.quantiles != nullptr) {
        Exec E{p, params, aux, ws, p.layout(1), 1, (hipStream_t)stream};
        record_quantiles(E, sc, (long long)B * d.io_h * d.io_w * d.x_d);
    }
    check_launch();
    return CNF_OK;
    CNF_CATCH
}

}  // namespace

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

int cnf_flow_sample_score(cnf_plan* plan, const float* params, const float* aux, const float* y,
                          const cnf_sample_desc* desc, const cnf_sample_score_desc* score, const float* truth,
                          float* samples, float* mean, float* std, float* y_dev, float* log_prob, int* rank,
                          float* abs_err, float* sq_err, int* hist, float* quantiles, void* workspace, int B,
                          void* stream) {
    ScoreArgs sc;
    sc.sd = score;
    sc.truth = truth;
    sc.rank = rank;
    sc.abs_err = abs_err;
    sc.sq_err = sq_err;
    sc.hist = hist;
    sc.quantiles = quantiles;
    return flow_sample("cnf_flow_sample_score", plan, params, aux, y, desc, samples, mean, std, y_dev, log_prob,
                       workspace, B, stream, sc);
}

}  // extern "C"
