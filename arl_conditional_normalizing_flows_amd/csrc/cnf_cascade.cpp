// cnf_cascade.cpp — cascaded super-resolution sampling (include/cnf.h cnf_flow_sample_cascade; kernels:
// cnf_sample.hip): L flows chained, each stage's draws `up`-scaled into the next stage's conditions, the
// tree of nodes walked depth-first with one chunk buffer per stage. Per chunk of a stage: its zy (k_latent at
// stage 1, k_child_latent from the parent chunk's buffers below it), that plan's inverse schedule
// (cnf_schedule.cpp), the folds of cnf_sampling.cpp with the image's own condition, then the chunk's children.
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
std::string cascade_desc_error(const cnf_plan* const* plans, int B, const cnf_cascade_desc* s) {
    if (s == nullptr) return "null cascade descriptor";
    if (s->num_stages < 1 || s->num_stages > MAX_STAGES) return "num_stages must be in 1..4";
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
        const int per = d.io_h * d.io_w * d.x_d;   // elements per condition
        const bool stats = s.mean != nullptr || s.std != nullptr;
        float* const out = leaf ? samples : nullptr;
        float *zy = s.zy, *xy = s.xy;
        SampleFoldArgs fa;
        std::memset(&fa, 0, sizeof(fa));
        fa.xy_hat = xy;
        fa.zy = zy;
        fa.samples = out;
        fa.state = stats ? s.state : nullptr;
        fa.mean = s.mean;
        fa.std = s.std;
        fa.B = B;
        fa.logit = logit;
        fa.residual = residual;
        fa.lk = lk;
        const bool scores = leaf && (sc.rank || sc.abs_err || sc.hist);
        SampleScoreArgs sa;
        std::memset(&sa, 0, sizeof(sa));
        SampleSqerrArgs qa;
        std::memset(&qa, 0, sizeof(qa));
        if (leaf && sc.any()) {
            sa.xy_hat = xy;
            sa.zy = zy;
            sa.truth = sc.truth;
            sa.rank = sc.rank;
            sa.abs_err = sc.abs_err;
            sa.hist = sc.hist;
            sa.logit = logit;
            sa.residual = residual;
            sa.lk = lk;
            if (sc.hist) {
                sa.bins = sc.sd->bins;
                sa.lo = sc.sd->lo;
                sa.scale = (float)sc.sd->bins / (sc.sd->hi - sc.sd->lo);
            }
            qa.xy_hat = xy;
            qa.zy = zy;
            qa.truth = sc.truth;
            qa.sq_err = sc.sq_err;
            qa.logit = logit;
            qa.residual = residual;
            qa.lk = lk;
        }
        const BlockDevArgs ba{xy, zy, s.block_dev, d.io_w, logit, residual, lk};
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
                    const ChildLatentArgs ca{st[l - 1].xy, st[l - 1].zy, zy, pg0, s.S, d.io_w, s.T, seed, s.off, logit,
                                             residual, lk};
                    // the parents' x_hat (and y with the residual) once, the chunk's zy written
                    E.record("k_child_latent", 0,
                             4.0 * n * px * d.io_d + 4.0 * ((double)n / s.S + 1) * (px / 4) * d.x_d * (residual ? 2 : 1),
                             [=](void* q) { launch_child_latent(c, ca, (hipStream_t)q); });
                }
                flow_inverse(p, s.params, s.aux, zy, xy, s.ws, n, stream, io);
                if (out != nullptr || stats)
                    E.record("k_sample_fold_node", 0, 4.0 * n * px * d.x_d * ((out ? 2 : 1) + (residual ? 1 : 0)),
                             [=](void* q) { launch_sample_fold(c, fa, (hipStream_t)q); });
                if (s.y_dev != nullptr) {
                    float* y_dev = s.y_dev;
                    E.record("k_sample_ydev_node", 0, 8.0 * n * px * (d.io_d - d.x_d),
                             [=](void* q) { launch_sample_ydev_node(c, xy, zy, y_dev, (hipStream_t)q); });
                }
                if (s.block_dev != nullptr)
                    E.record("k_block_dev", 0, 8.0 * n * px * d.x_d,
                             [=](void* q) { launch_block_dev(c, ba, (hipStream_t)q); });
                if (scores) {
                    const double nb = (double)((g0 + n - 1) / s.N - g0 / s.N + 1);
                    const double rmw = (sc.rank ? 8.0 : 0.0) + (sc.abs_err ? 8.0 : 0.0) + (sc.hist ? 8.0 * sa.bins : 0.0);
                    E.record("k_sample_score_node", 0,
                             4.0 * n * px * d.x_d * (residual ? 2 : 1) + nb * per * ((sc.truth ? 4.0 : 0.0) + rmw),
                             [=](void* q) { launch_sample_score(c, sa, (hipStream_t)q); });
                }
                if (leaf && sc.sq_err != nullptr)
                    E.record("k_sample_sqerr_node", 0, 4.0 * n * px * d.x_d * (residual ? 3 : 2),
                             [=](void* q) { launch_sample_sqerr(c, qa, (hipStream_t)q); });
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
    if (desc == nullptr) return fail(CNF_E_INVALID, w + "null cascade descriptor");
    if (desc->num_stages < 1 || desc->num_stages > MAX_STAGES) return fail(CNF_E_INVALID, w + "num_stages must be in 1..4");
    const int L = desc->num_stages;
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
        const SampleQuantileArgs ua = quantile_args(cs.sc, (long long)B * d.io_h * d.io_w * d.x_d);
        Exec E{p, s.params, s.aux, s.ws, p.layout(1), 1, cs.stream};
        E.record("k_sample_quantiles", 0, 4.0 * (double)ua.n * (ua.bins + ua.nq),
                 [=](void* q) { launch_sample_quantiles(ua, (hipStream_t)q); });
    }
    check_launch();
    return CNF_OK;
    CNF_CATCH
}

}  // extern "C"
