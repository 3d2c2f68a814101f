// cnf_cascade.cpp — cascaded super-resolution sampling (include/cnf.h cnf_flow_sample_cascade; kernels:
// cnf_sample.hip): L flows chained, each stage's draws `up`-scaled into the next stage's conditions, the
// tree of nodes walked depth-first with one chunk buffer per stage. Per chunk of a stage: its zy (k_latent at
// stage 1, k_child_latent from the parent chunk's buffers below it), that plan's inverse schedule
// (cnf_schedule.cpp), cnf_sampling.cpp's record_chunk_outputs with the image's own condition, then the chunk's
// children.
#include <algorithm>
#include <climits>
#include <cstring>
#include <string>

#include "cnf_sampling.h"

using namespace cnf;

namespace {

constexpr int MAX_STAGES = 4;
const char* const WHO = "cnf_flow_sample_cascade";

std::string stage(int l) { return "stage " + std::to_string(l + 1) + ": "; }

// the argument errors that need the plans, B and the descriptor alone (empty: none)
// the descriptor itself and its stage count, which everything else reads (null: fine)
const char* stages_error(const cnf_cascade_desc* s) {
    if (s == nullptr) return "null cascade descriptor";
    if (s->num_stages < 1 || s->num_stages > MAX_STAGES) return "num_stages must be in 1..4";
    return nullptr;
}

std::string cascade_desc_error(const cnf_plan* const* plans, int B, const cnf_cascade_desc* s) {
    if (const char* e = stages_error(s)) return e;
    if (plans == nullptr) return "null plans array";
    for (int l = 0; l < s->num_stages; l++)
        if (plans[l] == nullptr) return stage(l) + "null plan";
    long long N = 1;
    for (int l = 0; l < s->num_stages; l++) {
        const cnf_flow_desc& d = plans[l]->p->desc;
        if (d.io_d != 2 * d.x_d)
            return stage(l) + "io_d must be 2 * x_d (y has x's depth), got io_d " + std::to_string(d.io_d) + ", x_d " +
                   std::to_string(d.x_d);
        if (l > 0) {
            const cnf_flow_desc& q = plans[l - 1]->p->desc;
            if (d.x_d != q.x_d)
                return stage(l) + "x_d " + std::to_string(d.x_d) + " differs from stage " + std::to_string(l) + "'s " +
                       std::to_string(q.x_d);
            if (d.io_h != 2 * q.io_h || d.io_w != 2 * q.io_w)
                return stage(l) + "io shape (" + std::to_string(d.io_h) + ", " + std::to_string(d.io_w) +
                       ") must be twice stage " + std::to_string(l) + "'s (" + std::to_string(q.io_h) + ", " +
                       std::to_string(q.io_w) + ")";
        }
        const cnf_sample_desc sd{s->num_samples[l], s->chunk, s->temperature[l], s->seed, s->offset[l], s->logit_a,
                                 s->residual};
        if (const char* e = sample_desc_error(*plans[l]->p, B, &sd)) return (l == 0 ? std::string() : stage(l)) + e;
        N *= s->num_samples[l];
        if (N > INT_MAX) return "num_samples: more than 2^31 - 1 nodes per condition at stage " + std::to_string(l + 1);
    }
    return std::string();
}

// one stage of a call
struct Stage {
    Plan* p;
    const float* params;
    const float* aux;
    char* ws;                 // this stage's part of the workspace
    float *zy, *xy, *state;   // its chunk buffers and statistics state
    int S;                    // children per parent node
    long long N;              // nodes per condition
    float T;
    unsigned long long off;
    float *mean, *std, *y_dev, *block_dev;
};

struct Cascade {
    Stage st[MAX_STAGES];
    int L, B, chunk, logit, residual;
    LogitK lk;
    unsigned long long seed;
    const float* y;
    float* samples;
    ScoreArgs sc;
    hipStream_t stream;

    // the nodes of stage l whose parents are nodes pg0 .. pg0 + pn - 1 of stage l - 1 (l == 0: every node),
    // `chunk` at a time, each chunk followed by its own children
    void run(int l, long long pg0, int pn) {
        Stage& s = st[l];
        Plan& p = *s.p;
        const cnf_flow_desc& d = p.desc;
        const bool leaf = l == L - 1;
        const long long first = l == 0 ? 0 : pg0 * s.S, last = l == 0 ? (long long)B * s.N : (pg0 + pn) * s.S;
        const double px = (double)d.io_h * d.io_w;
        float *zy = s.zy, *xy = s.xy;
        const DrawView v{xy, zy, nullptr, logit, residual, lk};   // a node's condition: its own zy
        float* const state = s.mean != nullptr || s.std != nullptr ? s.state : nullptr;
        // the leaves alone are returned and scored
        const ChunkOutputs out{leaf ? samples : nullptr, state, s.mean, s.std, s.y_dev, s.block_dev, /*log_prob=*/nullptr,
                               leaf ? sc : ScoreArgs(), B};
        InverseOpts io;
        io.append = true;   // one recording per plan for the whole call
        for (long long g0 = first; g0 < last; g0 += chunk) {
            const int n = (int)std::min<long long>(chunk, last - g0);
            {
                OptScope os_(&p.opts);
                const SampleChunk c{g0, n, (int)s.N, d.io_h * d.io_w, d.io_d, d.x_d};
                Exec E{p, s.params, s.aux, s.ws, p.layout(n), n, stream};
                if (l == 0) {
                    const float* y1 = y;
                    const float T = s.T;
                    const unsigned long long sd_ = seed, off = s.off;
                    E.record("k_latent", 0, 4.0 * n * px * (2 * d.io_d - d.x_d),
                             [=](void* q) { launch_latent(c, y1, zy, T, sd_, off, (hipStream_t)q); });
                } else {
                    const DrawView parent{st[l - 1].xy, st[l - 1].zy, nullptr, logit, residual, lk};
                    const ChildLatentArgs ca{parent, zy, pg0, s.S, d.io_w, s.T, seed, s.off};
                    // the parents' x_hat (and y with the residual) once, the chunk's zy written
                    E.record("k_child_latent", 0,
                             4.0 * n * px * d.io_d + 4.0 * ((double)n / s.S + 1) * (px / 4) * d.x_d * (residual ? 2 : 1),
                             [=](void* q) { launch_child_latent(c, ca, (hipStream_t)q); });
                }
                flow_inverse(p, s.params, s.aux, zy, xy, s.ws, n, stream, io);
                record_chunk_outputs(E, c, v, out);
            }
            if (!leaf) run(l + 1, g0, n);
        }
    }
};

}  // namespace

extern "C" {

size_t cnf_cascade_workspace_bytes(const cnf_plan* const* plans, int B, const cnf_cascade_desc* desc) {
    const std::string e = cascade_desc_error(plans, B, desc);
    if (!e.empty()) {   // (the message for cnf_last_error)
        (void)fail(CNF_E_INVALID, "cnf_cascade_workspace_bytes: " + e);
        return 0;
    }
    size_t total = 0;
    for (int l = 0; l < desc->num_stages; l++) {
        OptScope os_(&plans[l]->p->opts);
        total += sample_layout(*plans[l]->p, B, desc->chunk).total;
    }
    return total;
}

int cnf_flow_sample_cascade(cnf_plan* const* plans, const float* const* params, const float* const* aux,
                            const float* y, const cnf_cascade_desc* desc, const cnf_sample_score_desc* score,
                            const float* truth, float* samples, int* rank, float* abs_err, float* sq_err, int* hist,
                            float* quantiles, float* const* mean, float* const* std, float* const* y_dev,
                            float* const* block_dev, void* workspace, int B, void* stream) {
    const std::string w = std::string(WHO) + ": ";
    if (const char* e = stages_error(desc)) return fail(CNF_E_INVALID, w + e);
    const int L = desc->num_stages;
    // the pointer checks come before the descriptor's other errors, stage by stage: cascade_desc_error's own
    // null-plan tests cannot stand in for these without changing which message a caller with two errors sees
    if (!plans || !params || !aux) return fail(CNF_E_INVALID, w + "null plans, params or aux array");
    for (int l = 0; l < L; l++) {
        if (!plans[l]) return fail(CNF_E_INVALID, w + stage(l) + "null plan");
        if (!params[l]) return fail(CNF_E_INVALID, w + stage(l) + "null params");
        if (!aux[l]) return fail(CNF_E_INVALID, w + stage(l) + "null aux");
    }
    if (!workspace) return fail(CNF_E_INVALID, w + "null workspace");
    if (!y) return fail(CNF_E_INVALID, w + "null y");
    {
        const std::string e = cascade_desc_error(plans, B, desc);
        if (!e.empty()) return fail(CNF_E_INVALID, w + e);
    }
    Cascade cs;
    cs.sc.sd = score;
    cs.sc.truth = truth;
    cs.sc.rank = rank;
    cs.sc.abs_err = abs_err;
    cs.sc.sq_err = sq_err;
    cs.sc.hist = hist;
    cs.sc.quantiles = quantiles;
    if (const char* e = score_error(cs.sc)) return fail(CNF_E_INVALID, w + e);
    bool any = samples != nullptr || cs.sc.any();
    for (int l = 0; l < L; l++) {
        const cnf_flow_desc& d = plans[l]->p->desc;
        if (block_dev && block_dev[l] && (d.io_h % 2 != 0 || d.io_w % 2 != 0))
            return fail(CNF_E_INVALID, w + stage(l) + "block_dev needs an even io_h and io_w");
        any = any || (mean && mean[l]) || (std && std[l]) || (y_dev && y_dev[l]) || (block_dev && block_dev[l]);
    }
    if (!any)
        return fail(CNF_E_INVALID, w + "no output requested (samples, rank, abs_err, sq_err, hist, quantiles and every "
                                       "mean, std, y_dev, block_dev entry null)");
    CNF_TRY
    cs.L = L;
    cs.B = B;
    cs.chunk = desc->chunk;
    cs.logit = desc->logit_a != 0.f ? 1 : 0;
    cs.residual = desc->residual != 0 ? 1 : 0;
    std::memset(&cs.lk, 0, sizeof(cs.lk));
    if (cs.logit) cs.lk = logit_consts(desc->logit_a);
    cs.seed = desc->seed;
    cs.y = y;
    cs.samples = samples;
    cs.stream = (hipStream_t)stream;
    char* ws = (char*)workspace;
    long long N = 1;
    for (int l = 0; l < L; l++) {
        Plan& p = *plans[l]->p;
        OptScope os_(&p.opts);
        ensure_tables(p);
        p.recorded.clear();
        const SampleLayout SL = sample_layout(p, B, desc->chunk);
        N *= desc->num_samples[l];
        Stage& s = cs.st[l];
        s.p = &p;
        s.params = params[l];
        s.aux = aux[l];
        s.ws = ws;
        s.zy = reinterpret_cast<float*>(ws + SL.zy);
        s.xy = reinterpret_cast<float*>(ws + SL.xy);
        s.state = reinterpret_cast<float*>(ws + SL.state);
        s.S = desc->num_samples[l];
        s.N = N;
        s.T = desc->temperature[l];
        s.off = desc->offset[l];
        s.mean = mean ? mean[l] : nullptr;
        s.std = std ? std[l] : nullptr;
        s.y_dev = y_dev ? y_dev[l] : nullptr;
        s.block_dev = block_dev ? block_dev[l] : nullptr;
        ws += SL.total;
    }
    cs.run(0, 0, 0);
    if (quantiles != nullptr) {
        Stage& s = cs.st[L - 1];
        Plan& p = *s.p;
        OptScope os_(&p.opts);
        const cnf_flow_desc& d = p.desc;
        Exec E{p, s.params, s.aux, s.ws, p.layout(1), 1, cs.stream};
        record_quantiles(E, cs.sc, (long long)B * d.io_h * d.io_w * d.x_d);
    }
    check_launch();
    return CNF_OK;
    CNF_CATCH
}

}  // extern "C"
