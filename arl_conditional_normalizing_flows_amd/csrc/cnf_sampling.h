// cnf_sampling.h — what the sampling entry points share (cnf_sampling.cpp: cnf_flow_sample and its kin;
// cnf_cascade.cpp: cnf_flow_sample_cascade): the workspace layout and the argument checks. Internal.
#pragma once

#include <cstddef>

#include "cnf_api.h"
#include "cnf_plan.h"

namespace cnf {

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

// k_sample_quantiles' arguments for n elements, from the score descriptor
SampleQuantileArgs quantile_args(const ScoreArgs& sc, long long n);

}  // namespace cnf
