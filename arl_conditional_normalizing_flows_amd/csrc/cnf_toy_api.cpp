// cnf_toy_api.cpp — the C ABI of the TOYcINN dense flow (include/cnf.h cnf_toy_*): the descriptor checks, the
// one description of the flow its kernels read (ToyNet, cnf_kernels.h) and the launches of k_toy (cnf_toy.hip),
// k_toy_bwd (cnf_toy_train.hip), k_toy_sample (cnf_toy_sample.hip) and k_toy_density (cnf_toy_density.hip).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "cnf_api.h"
#include "cnf_kernels.h"

using namespace cnf;

namespace {

constexpr int64_t TOY_LDS_BUDGET = 160 * 1024;   // bytes of LDS a toy kernel's workgroup may ask for

void toy_check(const cnf_toy_desc* d) {
    if (!d) throw std::invalid_argument("null toy descriptor");
    if (d->io_shape != 3) throw std::invalid_argument("TOYcINN masks are defined for io_shape == 3 only");
    if (d->x_d < 1 || d->x_d > 2) throw std::invalid_argument("x_d must be 1 or 2");
    if (d->num_coupling_layers < 1 || d->num_coupling_layers > TOY_MAXL)
        throw std::invalid_argument("num_coupling_layers must be in [1, 128]");
    if (d->intermediate_dims < 1 || d->intermediate_dims > 64) throw std::invalid_argument("intermediate_dims must be in [1, 64]");
    if (d->num_layers < 0) throw std::invalid_argument("num_layers must be >= 0");
    if (!d->mask_indices) throw std::invalid_argument("mask_indices is required");
    std::vector<int> seen(d->num_coupling_layers, 0);
    for (int i = 0; i < d->num_coupling_layers; i++) {
        const int j = d->mask_indices[i];
        if (j < 0 || j >= d->num_coupling_layers || seen[j]++) throw std::invalid_argument("mask_indices must be a permutation");
    }
}

// parameters of coupling network j: its b net, then its A net, each Dense(H), L x Dense(H), Dense(3 - n1)
int64_t toy_coupling_floats(const cnf_toy_desc* d, int j) {
    const int64_t n1 = toy_n1(j), n2 = 3 - n1, H = d->intermediate_dims, L = d->num_layers;
    return 2 * (n1 * H + H + L * (H * H + H) + H * n2 + n2);
}

// the flow of a checked descriptor as the kernels read it; returns the floats of its largest coupling network
int64_t toy_flow(const cnf_toy_desc* d, ToyNet& f) {
    f.nl = d->num_coupling_layers;
    f.H = d->intermediate_dims;
    f.L = d->num_layers;
    f.x_d = d->x_d;
    int64_t off = 0, maxn = 0;
    for (int j = 0; j < f.nl; j++) {
        f.order[j] = d->mask_indices[j];
        f.net_off[j] = (int)off;
        const int64_t n = toy_coupling_floats(d, j);
        off += n;
        maxn = std::max(maxn, n);
    }
    f.net_off[f.nl] = (int)off;
    return maxn;
}

// k_toy over B samples in direction `direction`; save_u (may be null): the training forward's saved inputs
int run_toy(const cnf_toy_desc* d, const float* params, const float* u, float* v, float* log_detJ, float* per_sample,
            float* save_u, int B, int direction, void* stream) {
    ToyArgs a;
    std::memset(&a, 0, sizeof(a));
    const int64_t maxn = toy_flow(d, a.flow);
    if (maxn * 4 > TOY_LDS_BUDGET)
        return fail(CNF_E_INVALID, "toy coupling networks exceed the 160 KiB LDS staging budget");
    a.params = params;
    a.u = u;
    a.v = v;
    a.log_detJ = direction < 0 ? log_detJ : nullptr;
    a.per_sample = direction < 0 ? per_sample : nullptr;
    a.B = B;
    a.dir = direction;
    a.lambda_y = d->lambda_y;
    a.save_u = save_u;
    launch_toy(a, (int)maxn, (hipStream_t)stream);
    hip_check(hipGetLastError(), "k_toy");
    return CNF_OK;
}

// training workspace: the saved coupling-layer inputs [nl][B][3], then one partial gradient row per
// tile of TOY_TS samples [tiles][num_params]
size_t toy_saved_bytes(const cnf_toy_desc* d, int B) {
    return ((size_t)d->num_coupling_layers * B * 3 * sizeof(float) + 255) & ~(size_t)255;
}

// the argument errors of cnf_toy_sample that need no pointer but the descriptors (null: fine)
const char* toy_sample_desc_error(const cnf_toy_desc* d, int B, const cnf_toy_sample_desc* s) {
    if (s == nullptr) return "null sample descriptor";
    if (B < 1) return "B must be >= 1";
    if (s->num_samples < 1) return "num_samples must be >= 1";
    if (!(s->temperature >= 0.f) || std::isinf(s->temperature)) return "temperature must be finite and >= 0";
    if (s->hist_bins < 0) return "hist_bins must be >= 0";
    if ((int64_t)B * toy_tiles(s->num_samples, TOY_SAMPLE_TS) > INT32_MAX || (double)B * s->num_samples * d->x_d > 4e18)
        return "B * num_samples * x_d exceeds the index range (B * tiles must stay below 2^31)";
    if (s->hist_bins >= 1) {
        for (int c = 0; c < d->x_d; c++) {
            if (!std::isfinite(s->hist_lo[c]) || !std::isfinite(s->hist_hi[c])) return "hist_lo / hist_hi must be finite";
            if (!(s->hist_lo[c] < s->hist_hi[c])) return "hist_lo must be below hist_hi";
            if (!std::isfinite((float)s->hist_bins / (s->hist_hi[c] - s->hist_lo[c]))) return "hist_lo / hist_hi: the bin scale is not finite";
        }
        if (std::pow((double)s->hist_bins, d->x_d) * B > 1e12) return "hist_bins: the grid exceeds 10^12 cells";
    }
    return nullptr;
}

// points per condition of a density call (grid: G^x_d), or 0 with *err set: the argument errors of
// cnf_toy_density that need no pointer but the descriptors; grid: whether the points are a grid's centres
int64_t toy_density_points(const cnf_toy_desc* d, int B, const cnf_toy_density_desc* q, bool grid, const char** err) {
    *err = nullptr;
    if (q == nullptr) return *err = "null density descriptor", 0;
    if (B < 1) return *err = "B must be >= 1", 0;
    int64_t N = q->num_points;
    if (!grid) {
        if (q->grid_bins != 0) return *err = "grid_bins must be 0 when x is given", 0;
        if (q->num_points < 1) return *err = "num_points must be >= 1", 0;
    } else {
        if (q->grid_bins < 1) return *err = "grid_bins must be >= 1 when x is null", 0;
        for (int c = 0; c < d->x_d; c++) {
            if (!std::isfinite(q->lo[c]) || !std::isfinite(q->hi[c])) return *err = "lo / hi must be finite", 0;
            if (!(q->lo[c] < q->hi[c])) return *err = "lo must be below hi", 0;
            const float step = (q->hi[c] - q->lo[c]) / (float)q->grid_bins;
            if (!std::isfinite(step) || !(step > 0.f)) return *err = "lo / hi: the bin step is not a positive finite number", 0;
        }
        N = q->grid_bins;
        if (d->x_d == 2) N *= q->grid_bins;
    }
    if (N > INT32_MAX || (int64_t)B * toy_tiles(N, TOY_SAMPLE_TS) > INT32_MAX || (double)B * (double)N * 3.0 > 4e18)
        return *err = "B * N * 3 exceeds the index range (N and B * tiles must stay below 2^31)", 0;
    return N;
}

}  // namespace

extern "C" {

int64_t cnf_toy_num_params(const cnf_toy_desc* d) {
    CNF_TRY
    toy_check(d);
    int64_t n = 0;
    for (int j = 0; j < d->num_coupling_layers; j++) n += toy_coupling_floats(d, j);
    return n;
    CNF_CATCH
}

int cnf_toy_call(const cnf_toy_desc* d, const float* params, const float* u, float* v, float* log_detJ,
                 float* per_sample, int B, int direction, void* stream) {
    CNF_TRY
    toy_check(d);
    if (!params || !u || !v || B < 0) return fail(CNF_E_INVALID, "null pointer or negative batch");
    if (direction != 1 && direction != -1) return fail(CNF_E_INVALID, "direction must be +1 or -1");
    if (u == v) return fail(CNF_E_INVALID, "u and v must not alias");
    if (B == 0) return CNF_OK;
    return run_toy(d, params, u, v, log_detJ, per_sample, nullptr, B, direction, stream);
    CNF_CATCH
}

// ---- training (TOYcINN_make_model.py:453-481) --------------------------------------------------------
size_t cnf_toy_train_workspace_bytes(const cnf_toy_desc* d, int B) {
    try {
        toy_check(d);
        if (B < 1) throw std::invalid_argument("B must be >= 1");
        const int64_t n = cnf_toy_num_params(d);
        return toy_saved_bytes(d, B) + (size_t)toy_tiles(B, TOY_TS) * (size_t)n * sizeof(float);
    } catch (const std::exception& e) {
        fail(CNF_E_INVALID, e.what());
        return 0;
    }
}

int cnf_toy_forward_train(const cnf_toy_desc* d, const float* params, const float* xy, float* zy, float* per_sample,
                          void* train_workspace, int B, void* stream) {
    CNF_TRY
    toy_check(d);
    if (!params || !xy || !zy || !train_workspace) return fail(CNF_E_INVALID, "null pointer");
    if (B < 1) return fail(CNF_E_INVALID, "B must be >= 1");
    if (xy == zy) return fail(CNF_E_INVALID, "xy and zy must not alias");
    return run_toy(d, params, xy, zy, nullptr, per_sample, static_cast<float*>(train_workspace), B, -1, stream);
    CNF_CATCH
}

int cnf_toy_backward(const cnf_toy_desc* d, const float* params, const float* xy, const float* zy, void* train_workspace,
                     int B, float inv_batch, float* dparams, void* stream) {
    CNF_TRY
    toy_check(d);
    if (!params || !xy || !zy || !train_workspace || !dparams) return fail(CNF_E_INVALID, "null pointer");
    if (B < 1) return fail(CNF_E_INVALID, "B must be >= 1");
    if (!std::isfinite(inv_batch)) return fail(CNF_E_INVALID, "inv_batch must be finite");
    if ((int64_t)toy_bwd_lds_bytes(d->intermediate_dims, d->num_layers) > TOY_LDS_BUDGET)
        return fail(CNF_E_INVALID, "the toy backward's activations exceed the 160 KiB LDS budget");
    ToyBwdArgs a;
    std::memset(&a, 0, sizeof(a));
    toy_flow(d, a.flow);
    a.params = params;
    a.xy = xy;
    a.zy = zy;
    a.saved_u = static_cast<const float*>(train_workspace);
    a.part = reinterpret_cast<float*>(static_cast<char*>(train_workspace) + toy_saved_bytes(d, B));
    a.B = B;
    a.HP = toy_bwd_hp(a.flow.H);
    a.num_params = a.flow.net_off[a.flow.nl];
    a.lambda_y = d->lambda_y;
    a.inv_batch = inv_batch;
    launch_toy_bwd(a, (hipStream_t)stream);
    hip_check(hipGetLastError(), "k_toy_bwd");
    launch_toy_grad_sum(a.part, (int)toy_tiles(B, TOY_TS), a.num_params, dparams, (hipStream_t)stream);
    hip_check(hipGetLastError(), "k_toy_grad_sum");
    return CNF_OK;
    CNF_CATCH
}

// ---- sampling (TOYcINN.py:807-817; kernels: cnf_toy_sample.hip) -----------------------------------------
size_t cnf_toy_sample_workspace_bytes(const cnf_toy_desc* d, int B, const cnf_toy_sample_desc* s) {
    try {
        toy_check(d);
        if (const char* e = toy_sample_desc_error(d, B, s)) throw std::invalid_argument(e);
        // the tile partials [B][tiles][x_d][TOY_SAMPLE_PART]
        return (size_t)B * (size_t)toy_tiles(s->num_samples, TOY_SAMPLE_TS) * d->x_d * TOY_SAMPLE_PART * sizeof(float);
    } catch (const std::exception& e) {
        fail(CNF_E_INVALID, std::string("cnf_toy_sample_workspace_bytes: ") + e.what());
        return 0;
    }
}

int cnf_toy_sample(const cnf_toy_desc* d, const float* params, const float* y, const cnf_toy_sample_desc* s,
                   float* samples, float* mean, float* std, float* y_dev, uint32_t* hist, void* workspace, int B,
                   void* stream) {
    CNF_TRY
    toy_check(d);
    if (!params || !workspace) return fail(CNF_E_INVALID, "cnf_toy_sample: null params or workspace");
    if (!y) return fail(CNF_E_INVALID, "cnf_toy_sample: null y");
    if (const char* e = toy_sample_desc_error(d, B, s)) return fail(CNF_E_INVALID, std::string("cnf_toy_sample: ") + e);
    if (hist && s->hist_bins < 1) return fail(CNF_E_INVALID, "cnf_toy_sample: hist given with hist_bins < 1");
    if (!hist && s->hist_bins >= 1) return fail(CNF_E_INVALID, "cnf_toy_sample: hist_bins >= 1 with a null hist");
    if (!samples && !mean && !std && !y_dev && !hist)
        return fail(CNF_E_INVALID, "cnf_toy_sample: no output requested (samples, mean, std, y_dev, hist all null)");
    if ((int64_t)toy_sample_lds_bytes(d->intermediate_dims) > TOY_LDS_BUDGET)
        return fail(CNF_E_INVALID, "cnf_toy_sample: the hidden activations of a draw tile exceed the 160 KiB LDS budget");
    ToySampleArgs a;
    std::memset(&a, 0, sizeof(a));
    toy_flow(d, a.flow);
    const int x_d = a.flow.x_d;
    a.params = params;
    a.y = y;
    a.samples = samples;
    a.y_dev = y_dev;
    a.hist = hist;
    a.part = static_cast<float*>(workspace);
    a.B = B;
    a.S = s->num_samples;
    a.tiles = (int)toy_tiles(s->num_samples, TOY_SAMPLE_TS);
    a.HP = toy_bwd_hp(a.flow.H);
    a.temperature = s->temperature;
    a.seed = s->seed;
    a.offset = s->offset;
    a.G = hist ? s->hist_bins : 0;
    for (int c = 0; c < 2; c++) {
        a.lo[c] = hist && c < x_d ? s->hist_lo[c] : 0.f;
        a.scale[c] = hist && c < x_d ? (float)s->hist_bins / (s->hist_hi[c] - s->hist_lo[c]) : 0.f;
    }
    if (hist) {
        size_t cells = (size_t)B;
        for (int c = 0; c < x_d; c++) cells *= (size_t)s->hist_bins;
        hip_check(hipMemsetAsync(hist, 0, cells * sizeof(uint32_t), (hipStream_t)stream), "hipMemsetAsync(hist)");
    }
    launch_toy_sample(a, (hipStream_t)stream);
    hip_check(hipGetLastError(), "k_toy_sample");
    if (mean || std) {
        launch_toy_sample_stats(a.part, B, a.tiles, a.S, x_d, mean, std, (hipStream_t)stream);
        hip_check(hipGetLastError(), "k_toy_sample_stats");
    }
    return CNF_OK;
    CNF_CATCH
}

// ---- density (kernels: cnf_toy_density.hip) --------------------------------------------------------------
size_t cnf_toy_density_workspace_bytes(const cnf_toy_desc* d, int B, const cnf_toy_density_desc* q) {
    try {
        toy_check(d);
        const char* e = nullptr;
        const int64_t N = toy_density_points(d, B, q, q != nullptr && q->grid_bins != 0, &e);
        if (e) throw std::invalid_argument(e);
        // the tile partials [B][tiles][TOY_DENSITY_PART]
        return (size_t)B * (size_t)toy_tiles(N, TOY_SAMPLE_TS) * TOY_DENSITY_PART * sizeof(float);
    } catch (const std::exception& e) {
        fail(CNF_E_INVALID, std::string("cnf_toy_density_workspace_bytes: ") + e.what());
        return 0;
    }
}

int cnf_toy_density(const cnf_toy_desc* d, const float* params, const float* y, const float* x,
                    const cnf_toy_density_desc* q, float* log_prob, float* y_dev, float* z, float* log_mass,
                    void* workspace, int B, void* stream) {
    CNF_TRY
    toy_check(d);
    if (!params || !workspace) return fail(CNF_E_INVALID, "cnf_toy_density: null params or workspace");
    if (!y) return fail(CNF_E_INVALID, "cnf_toy_density: null y");
    const char* e = nullptr;
    const int64_t N = toy_density_points(d, B, q, x == nullptr, &e);
    if (e) return fail(CNF_E_INVALID, std::string("cnf_toy_density: ") + e);
    if (log_mass && x) return fail(CNF_E_INVALID, "cnf_toy_density: log_mass is defined for a grid only (x must be null)");
    if (!log_prob && !y_dev && !z && !log_mass)
        return fail(CNF_E_INVALID, "cnf_toy_density: no output requested (log_prob, y_dev, z, log_mass all null)");
    if ((int64_t)toy_density_lds_bytes(d->intermediate_dims) > TOY_LDS_BUDGET)
        return fail(CNF_E_INVALID, "cnf_toy_density: the hidden activations of a point tile exceed the 160 KiB LDS budget");
    ToyDensityArgs a;
    std::memset(&a, 0, sizeof(a));
    toy_flow(d, a.flow);
    const int x_d = a.flow.x_d;
    a.params = params;
    a.y = y;
    a.x = x;
    a.log_prob = log_prob;
    a.y_dev = y_dev;
    a.z = z;
    a.part = log_mass ? static_cast<float*>(workspace) : nullptr;
    a.B = B;
    a.N = (int)N;
    a.tiles = (int)toy_tiles(N, TOY_SAMPLE_TS);
    a.HP = toy_bwd_hp(a.flow.H);
    a.G = x ? 0 : q->grid_bins;
    double log_cell = 0.0;
    for (int c = 0; c < 2; c++) {
        const bool on = !x && c < x_d;
        a.lo[c] = on ? q->lo[c] : 0.f;
        a.step[c] = on ? (q->hi[c] - q->lo[c]) / (float)q->grid_bins : 0.f;
        if (on) log_cell += std::log((double)a.step[c]);
    }
    launch_toy_density(a, (hipStream_t)stream);
    hip_check(hipGetLastError(), "k_toy_density");
    if (log_mass) {
        launch_toy_density_mass(a.part, B, a.tiles, log_cell, log_mass, (hipStream_t)stream);
        hip_check(hipGetLastError(), "k_toy_density_mass");
    }
    return CNF_OK;
    CNF_CATCH
}

int cnf_toy_nll_sums(const float* per_sample, float* sums, int B, void* stream) {
    CNF_TRY
    if (!per_sample || !sums || B < 1) return fail(CNF_E_INVALID, "null pointer or empty batch");
    launch_nll_sums(per_sample, sums, B, (hipStream_t)stream);
    hip_check(hipGetLastError(), "k_nll_sums");
    return CNF_OK;
    CNF_CATCH
}

}  // extern "C"
