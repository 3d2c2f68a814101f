// cnf_sampling.h — what the sampling entry points share (cnf_sampling.cpp: cnf_flow_sample and its kin;
// cnf_cascade.cpp: cnf_flow_sample_cascade): the workspace layout, the argument checks and the launches that
// follow a chunk's inverse. Internal.
#pragma once

#include <cstddef>

#include "cnf_api.h"
#include "cnf_plan.h"

namespace cnf {

// carves a call's workspace behind the plan's own layout: regions in take() order, each 256-byte aligned
struct WsCarver {
    size_t off;
    explicit WsCarver(size_t start) : off(align_up(start, 256)) {}
    size_t take(size_t bytes) {
        const size_t o = off;
        off = align_up(off + bytes, 256);
        return o;
    }
};

// the logit_a / residual errors every descriptor with the post-transforms shares (null: fine); zero_means: what
// logit_a == 0 stands for in the caller's message, "de_logitify" (sampling) or "logit map" (cnf_flow_log_prob)
enum class LogitWord { delogitify, logit_map };
const char* post_transform_error(const Plan& p, float logit_a, int residual, LogitWord zero_means);

// the sample workspace: the inverse workspace of `chunk` images, one chunk of zy and of xy_hat, and the
// statistics state (K, S1, S2) [3][B][H][W][x_d]
struct SampleLayout {
    size_t zy = 0, xy = 0, state = 0, total = 0;
};
SampleLayout sample_layout(const Plan& p, int B, int chunk);

// the argument errors of cnf_flow_sample that need no pointer but the descriptor (null: fine)
const char* sample_desc_error(const Plan& p, int B, const cnf_sample_desc* s);

// the score arguments of cnf_flow_sample_score (every output null: cnf_flow_sample_logp)
struct ScoreArgs {
    const cnf_sample_score_desc* sd = nullptr;
    const float* truth = nullptr;
    int* rank = nullptr;
    float* abs_err = nullptr;
    float* sq_err = nullptr;
    int* hist = nullptr;
    float* quantiles = nullptr;
    bool any() const { return rank || abs_err || sq_err || hist || quantiles; }
};
// the argument errors of the score part (no output given: none)
const char* score_error(const ScoreArgs& sc);

// What a caller wants from a chunk's draws (null: not wanted); state: the (K, S1, S2) region, given with mean or
// std; sc: the score outputs (its quantiles: record_quantiles, once after the last chunk)
struct ChunkOutputs {
    float* samples = nullptr;
    float *state = nullptr, *mean = nullptr, *std = nullptr;
    float* y_dev = nullptr;
    float* block_dev = nullptr;
    float* log_prob = nullptr;   // from the log-det slots the chunk's inverse left in E's workspace (ld_slots)
    ScoreArgs sc;
    int B = 0;
};
// The launches that follow the inverse of chunk c, whose draws and conditions are v: k_sample_fold,
// k_sample_ydev, k_block_dev, k_sample_logp, k_sample_score, k_sample_sqerr, each if asked for, in that order; the
// kernels that read a condition are recorded with the suffix _node when it is the image's own zy (DrawView).
// The one set of names and byte counts of cnf_flow_sample and its kin and of cnf_flow_sample_cascade.
void record_chunk_outputs(Exec& E, const SampleChunk& c, const DrawView& v, const ChunkOutputs& o);
// k_sample_quantiles over the n elements of the finished histogram
void record_quantiles(Exec& E, const ScoreArgs& sc, long long n);

}  // namespace cnf
