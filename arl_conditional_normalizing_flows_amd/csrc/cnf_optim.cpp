// cnf_optim.cpp — the C ABI of the clipped, guarded Adam step (include/cnf.h at cnf_optim_step): the slab table
// (pure host code), the workspace layout and the argument checks in front of cnf_optim.hip's three launches.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "cnf_api.h"
#include "cnf_kernels.h"

namespace cnf {

static_assert(sizeof(OptimSlab) == 16, "the table's entries are {int64 start, int32 count, int32 tensor}");
static_assert(OPTIM_SLAB % 4 == 0, "a slab inside a tensor starts on the tensor's float4 phase");

OptimWs optim_ws(void* base, int T, long long num_slabs) {
    OptimWs w;
    char* b = static_cast<char*>(base);
    size_t at = 0;
    auto take = [&](size_t bytes) {
        char* p = b ? b + at : nullptr;
        at += align_up(bytes, 16);
        return p;
    };
    w.sum_g = reinterpret_cast<double*>(take(sizeof(double) * (size_t)num_slabs));
    w.sum_h = reinterpret_cast<double*>(take(sizeof(double) * (size_t)num_slabs));
    w.nonfinite = reinterpret_cast<unsigned*>(take(sizeof(unsigned) * (size_t)num_slabs));
    w.scale = reinterpret_cast<float*>(take(sizeof(float) * (size_t)T));
    w.ctrl = reinterpret_cast<OptimCtrl*>(take(sizeof(OptimCtrl)));
    w.total = at;
    return w;
}

namespace {

// the number of slabs of a valid (n, offsets, T); the reason it is not valid otherwise
long long count_slabs(int64_t n, const int64_t* offsets, int T, std::string& why) {
    if (n < 1) return why = "n < 1", -1;
    if (T < 1) return why = "T < 1", -1;
    if (!offsets) return why = "offsets is NULL", -1;
    if (offsets[0] != 0 || offsets[T] != n) return why = "offsets must run from 0 to n", -1;
    long long slabs = 0;
    for (int t = 0; t < T; t++) {
        if (offsets[t + 1] < offsets[t]) return why = "offsets must be non-decreasing", -1;
        slabs += (offsets[t + 1] - offsets[t] + OPTIM_SLAB - 1) / OPTIM_SLAB;
    }
    if (slabs > 0x7fffffffLL) return why = "more than 2^31 - 1 slabs", -1;
    return slabs;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace
}  // namespace cnf

using namespace cnf;

int cnf_optim_slab_elems(void) { return OPTIM_SLAB; }

int64_t cnf_optim_num_slabs(int64_t n, const int64_t* offsets, int T) {
    std::string why;
    const long long s = count_slabs(n, offsets, T, why);
    if (s < 0) fail(CNF_E_INVALID, "cnf_optim_num_slabs: " + why);
    return s;
}

size_t cnf_optim_table_bytes(int64_t n, const int64_t* offsets, int T) {
    std::string why;
    const long long s = count_slabs(n, offsets, T, why);
    if (s < 0) return fail(CNF_E_INVALID, "cnf_optim_table_bytes: " + why), 0;
    return align_up(sizeof(OptimSlab) * (size_t)s + sizeof(int) * ((size_t)T + 1), 16);
}

int cnf_optim_table_build(int64_t n, const int64_t* offsets, int T, void* host_out) {
    std::string why;
    const long long slabs = count_slabs(n, offsets, T, why);
    if (slabs < 0) return fail(CNF_E_INVALID, "cnf_optim_table_build: " + why);
    if (!host_out) return fail(CNF_E_INVALID, "cnf_optim_table_build: host_out is NULL");
    CNF_TRY
    std::vector<OptimSlab> tab;
    std::vector<int> first((size_t)T + 1);
    tab.reserve((size_t)slabs);
    for (int t = 0; t < T; t++) {
        first[t] = (int)tab.size();
        for (int64_t at = offsets[t]; at < offsets[t + 1]; at += OPTIM_SLAB)
            tab.push_back(OptimSlab{(long long)at, (int)std::min<int64_t>(OPTIM_SLAB, offsets[t + 1] - at), t});
    }
    first[T] = (int)tab.size();
    char* out = static_cast<char*>(host_out);
    std::memset(out, 0, cnf_optim_table_bytes(n, offsets, T));
    std::memcpy(out, tab.data(), sizeof(OptimSlab) * tab.size());
    std::memcpy(out + sizeof(OptimSlab) * tab.size(), first.data(), sizeof(int) * first.size());
    return CNF_OK;
    CNF_CATCH
}

size_t cnf_optim_workspace_bytes(int64_t n, int T, int64_t num_slabs) {
    if (n < 1 || T < 1 || num_slabs < 1 || num_slabs > 0x7fffffffLL)
        return fail(CNF_E_INVALID, "cnf_optim_workspace_bytes: n, T and num_slabs must be >= 1"), 0;
    return optim_ws(nullptr, T, num_slabs).total;
}

int cnf_optim_step(float* params, const float* grads, float* m, float* v, float* ema, int64_t n,
                   const void* table_dev, int64_t num_slabs, int T, const cnf_optim_desc* desc, int64_t* state_dev,
                   float* stats_dev, float* scales_dev, void* workspace, void* stream) {
    auto bad = [](const std::string& why) { return fail(CNF_E_INVALID, "cnf_optim_step: " + why); };
    if (!params || !grads || !m || !v) return bad("params, grads, m and v are required");
    if (!table_dev || !desc || !state_dev || !workspace)
        return bad("table_dev, desc, state_dev and workspace are required");
    if (!aligned16(table_dev) || !aligned16(workspace) || (reinterpret_cast<uintptr_t>(state_dev) & 7u))
        return bad("table_dev and workspace must be 16-byte aligned, state_dev 8-byte aligned");
    if (n < 1) return bad("n < 1");
    if (T < 1) return bad("T < 1");
    if (num_slabs < 1 || num_slabs > 0x7fffffffLL) return bad("num_slabs out of range");
    const cnf_optim_desc& d = *desc;
    auto clip_ok = [](float c) { return std::isfinite(c) && c >= 0.f; };
    if (!clip_ok(d.clipvalue)) return bad("clipvalue must be finite and >= 0");
    if (!clip_ok(d.clipnorm)) return bad("clipnorm must be finite and >= 0");
    if (!clip_ok(d.global_clipnorm)) return bad("global_clipnorm must be finite and >= 0");
    if (d.clipnorm > 0.f && d.global_clipnorm > 0.f) return bad("clipnorm and global_clipnorm exclude each other");
    if (!(d.beta_1 >= 0.f && d.beta_1 < 1.f)) return bad("beta_1 must be in [0, 1)");
    if (!(d.beta_2 >= 0.f && d.beta_2 < 1.f)) return bad("beta_2 must be in [0, 1)");
    if (!(d.epsilon >= 0.f)) return bad("epsilon must be >= 0");
    if (!std::isfinite(d.lr)) return bad("lr must be finite");
    if (!(d.ema_momentum >= 0.f && d.ema_momentum < 1.f)) return bad("ema_momentum must be in [0, 1)");
    if (d.ema_momentum > 0.f && !ema) return bad("ema_momentum > 0 needs ema");
    CNF_TRY
    OptimArgs a;
    a.p = params;
    a.g = grads;
    a.m = m;
    a.v = v;
    a.ema = d.ema_momentum > 0.f ? ema : nullptr;
    a.slabs = static_cast<const OptimSlab*>(table_dev);
    a.first = reinterpret_cast<const int*>(a.slabs + num_slabs);
    a.num_slabs = (long long)num_slabs;
    a.T = T;
    a.vec = aligned16(params) && aligned16(grads) && aligned16(m) && aligned16(v) && aligned16(a.ema);
    a.d = d;
    a.state = reinterpret_cast<long long*>(state_dev);
    a.stats = stats_dev;
    a.scales_out = scales_dev;
    a.ws = optim_ws(workspace, T, (long long)num_slabs);
    launch_optim(a, (hipStream_t)stream);
    check_launch();
    return CNF_OK;
    CNF_CATCH
}
