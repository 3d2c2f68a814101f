// cnf_transforms.hip — the input transforms that feed the flow (conv_cINN_base_functions.py):
// logit preprocessing / de_logitify, super-resolution down / up / residual assembly, and
// instance / renewed Gaussian noise. All elementwise or 2x2-block HBM-bound kernels, one thread
// per output element (float4-free: every output is computed from a handful of inputs).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "cnf_api.h"
#include "cnf_device.h"

namespace cnf {

// LogitK (cnf_kernels.h) of the fudge factor a
LogitK logit_consts(float a) {
    const double ad = a;
    const double b = (1.0 - 2.0 * ad) / (1.0 - ad);
    LogitK k;
    k.a = a;
    k.c1 = (float)((1.0 - ad) * b);
    k.lo = logf((float)(ad / (1.0 - ad)));
    const float hi = logf((float)((1.0 - ad) / ad));
    k.span = hi - k.lo;
    k.inv_bc = (float)(1.0 / (b * (1.0 - ad)));
    return k;
}

namespace {

// preprocess_dataset_class._preprocess_for_logit / _logit / _scale_logit (:198-212)
__global__ __launch_bounds__(256) void k_logit(const float* __restrict__ x, float* __restrict__ out, long long n,
                                               LogitK k, int inverse) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const float v = x[i];
        out[i] = !inverse ? logit_value(v, k) : delogit_value(v, k);   // de_logitify (:306-318)
    }
}

// mean of the 2^L x 2^L block of `in` ([H][W][C] image) whose top-left corner is (r0, c0), as
// nested 2x2 means (down applied L times, :111-116: reduce_mean over each 2x2 block)
__device__ float nested_mean(const float* __restrict__ in, int W, int C, int r0, int c0, int c, int L) {
    if (L == 0) return in[((size_t)r0 * W + c0) * C + c];
    const int h = 1 << (L - 1);
    const float m00 = nested_mean(in, W, C, r0, c0, c, L - 1);
    const float m01 = nested_mean(in, W, C, r0, c0 + h, c, L - 1);
    const float m10 = nested_mean(in, W, C, r0 + h, c0, c, L - 1);
    const float m11 = nested_mean(in, W, C, r0 + h, c0 + h, c, L - 1);
    return ((m00 + m01) + (m10 + m11)) * 0.25f;
}

// preprocess_dataset_SR._preprocess_* (:252-273): one thread per (pixel, channel) of x
__global__ __launch_bounds__(256) void k_sr(const float* __restrict__ hi, float* __restrict__ xy, int B, int H, int W,
                                            int C, int xd, int yl, int residual) {
    const int Ho = H >> xd, Wo = W >> xd;
    const long long n = (long long)B * Ho * Wo * C;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
        const int c = (int)(e % C);
        const long long p = e / C;
        const int j = (int)(p % Wo);
        const long long q = p / Wo;
        const int i = (int)(q % Ho);
        const int b = (int)(q / Ho);
        const float* img = hi + (size_t)b * H * W * C;
        const int s = 1 << xd;
        const float x0 = nested_mean(img, W, C, i * s, j * s, c, xd);
        const int m = 1 << yl;
        const int bi = (i / m) * m, bj = (j / m) * m;   // y block of x0 containing (i, j)
        const float y = nested_mean(img, W, C, bi * s, bj * s, c, xd + yl);
        float* o = xy + (size_t)p * 2 * C;
        o[c] = residual ? x0 - y : x0;
        o[C + c] = y;
    }
}

__global__ __launch_bounds__(256) void k_down(const float* __restrict__ in, float* __restrict__ out, int B, int H,
                                              int W, int C) {
    const int Ho = H / 2, Wo = W / 2;
    const long long n = (long long)B * Ho * Wo * C;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
        const int c = (int)(e % C);
        const long long p = e / C;
        const int j = (int)(p % Wo);
        const long long q = p / Wo;
        const int i = (int)(q % Ho);
        const int b = (int)(q / Ho);
        out[e] = nested_mean(in + (size_t)b * H * W * C, W, C, 2 * i, 2 * j, c, 1);
    }
}

__global__ __launch_bounds__(256) void k_up(const float* __restrict__ in, float* __restrict__ out, int B, int H, int W,
                                            int C) {
    const int Ho = 2 * H, Wo = 2 * W;
    const long long n = (long long)B * Ho * Wo * C;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
        const int c = (int)(e % C);
        const long long p = e / C;
        const int j = (int)(p % Wo);
        const long long q = p / Wo;
        const int i = (int)(q % Ho);
        const int b = (int)(q / Ho);
        out[e] = in[(((size_t)b * H + i / 2) * W + j / 2) * C + c];
    }
}

// instance_noise (:635-654) / renew_noise (:660-676): element i of the stream offset + i
// (instance_noise_value, cnf_device.h)
__global__ __launch_bounds__(256) void k_noise(const float* __restrict__ x, float* __restrict__ out, long long n,
                                               float alpha, uint64_t seed, uint64_t offset) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
        out[i] = instance_noise_value(x != nullptr ? x[i] : 0.f, x != nullptr, alpha, seed, offset + (uint64_t)i);
}

// cnf_flow_forward_noise's input preparation as a pass of its own (the first coupling layer is
// streamed): out[i] = input_prep_value of element i
__global__ __launch_bounds__(256) void k_prep(float* __restrict__ out, long long n, InputPrepArgs q) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
        out[i] = input_prep_value(q.src[i], (int)(i % q.D), q, q.off + (uint64_t)i);
}

// cnf_batch_assemble: one training batch from the cached images in one pass. Element e of the output
// (batch-major NHWC) is k_logit / the label plane (CLASS) or k_sr (SR) of image index[b], then up to two
// k_noise stages of stream elements offset + e, in the same device functions as those kernels, so the
// result is theirs bit for bit. An index outside [0, N) is never dereferenced: its image is all NaN.
struct BatchArgs {
    const float* images;
    const int64_t* index;
    const float* label;
    long long N;
    int H, W, C, sr, logit, xd, yl, residual;
    LogitK lk;
    int on0, on1;   // a stage with alpha 1 is skipped, not computed: fmaf(1, x, 0 z) is x only for a finite z
    float alpha0, alpha1;
    uint64_t seed0, off0, seed1, off1;
};

__global__ __launch_bounds__(256) void k_batch(BatchArgs a, float* __restrict__ xy, long long n) {
    const int Ho = a.H >> a.xd, Wo = a.W >> a.xd;
    const int D = a.sr ? 2 * a.C : a.C + 1;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
        const int ch = (int)(e % D);
        const long long p = e / D;
        const int j = (int)(p % Wo);
        const long long q = p / Wo;
        const int i = (int)(q % Ho);
        const int b = (int)(q / Ho);
        const long long idx = a.index[b];
        if (idx < 0 || idx >= a.N) {
            xy[e] = __builtin_nanf("");
            continue;
        }
        const float* img = a.images + (size_t)idx * a.H * a.W * a.C;
        float v;
        if (!a.sr) {
            if (ch < a.C) {
                v = img[((size_t)i * a.W + j) * a.C + ch];
                if (a.logit) v = logit_value(v, a.lk);
            } else {
                v = a.label[b];
            }
        } else {   // k_sr's x and y of channel c
            const int c = ch < a.C ? ch : ch - a.C;
            const int s = 1 << a.xd;
            const int m = 1 << a.yl;
            const int bi = (i / m) * m, bj = (j / m) * m;
            const float y = nested_mean(img, a.W, a.C, bi * s, bj * s, c, a.xd + a.yl);
            if (ch < a.C) {
                const float x0 = nested_mean(img, a.W, a.C, i * s, j * s, c, a.xd);
                v = a.residual ? x0 - y : x0;
            } else {
                v = y;
            }
        }
        if (a.on0) v = instance_noise_value(v, true, a.alpha0, a.seed0, a.off0 + (uint64_t)e);
        if (a.on1) v = instance_noise_value(v, true, a.alpha1, a.seed1, a.off1 + (uint64_t)e);
        xy[e] = v;
    }
}

int grid_for(long long n) {
    long long g = (n + 255) / 256;
    return (int)(g < 1 ? 1 : (g > 65536 ? 65536 : g));
}

int finish(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(CNF_E_HIP, (std::string(what) + ": " + hipGetErrorString(e)).c_str());
    return CNF_OK;
}

}  // namespace

void launch_input_prep(float* out, long long n, const InputPrepArgs& q, hipStream_t st) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_prep, dim3(grid_for(n)), dim3(256), 0, st, out, n, q);
}

}  // namespace cnf

extern "C" {

int cnf_logit(const float* x, float* out, int64_t n, float a, int inverse, void* stream) {
    if (!x || !out || n < 0 || !(a > 0.f && a < 0.5f))
        return cnf::set_error(CNF_E_INVALID, "cnf_logit: null pointer, n < 0 or a outside (0, 0.5)");
    if (n == 0) return CNF_OK;
    hipLaunchKernelGGL(cnf::k_logit, dim3(cnf::grid_for(n)), dim3(256), 0, (hipStream_t)stream, x, out, (long long)n,
                       cnf::logit_consts(a), inverse);
    return cnf::finish("k_logit");
}

int cnf_sr_preprocess(const float* hires, float* xy, int B, int H, int W, int C, int x_down, int y_levels,
                      int residual, void* stream) {
    if (!hires || !xy || B <= 0 || H <= 0 || W <= 0 || C <= 0 || x_down < 0 || y_levels < 0 || x_down + y_levels > 8)
        return cnf::set_error(CNF_E_INVALID, "cnf_sr_preprocess: bad shape or levels");
    const int m = 1 << (x_down + y_levels);
    if (H % m || W % m) return cnf::set_error(CNF_E_INVALID, "cnf_sr_preprocess: H and W must be divisible by 2^(x_down + y_levels)");
    const long long n = (long long)B * (H >> x_down) * (W >> x_down) * C;
    hipLaunchKernelGGL(cnf::k_sr, dim3(cnf::grid_for(n)), dim3(256), 0, (hipStream_t)stream, hires, xy, B, H, W, C,
                       x_down, y_levels, residual);
    return cnf::finish("k_sr");
}

int cnf_down(const float* in, float* out, int B, int H, int W, int C, void* stream) {
    if (!in || !out || B <= 0 || H < 2 || W < 2 || C <= 0) return cnf::set_error(CNF_E_INVALID, "cnf_down: bad shape");
    const long long n = (long long)B * (H / 2) * (W / 2) * C;
    hipLaunchKernelGGL(cnf::k_down, dim3(cnf::grid_for(n)), dim3(256), 0, (hipStream_t)stream, in, out, B, H, W, C);
    return cnf::finish("k_down");
}

int cnf_up(const float* in, float* out, int B, int H, int W, int C, void* stream) {
    if (!in || !out || B <= 0 || H <= 0 || W <= 0 || C <= 0) return cnf::set_error(CNF_E_INVALID, "cnf_up: bad shape");
    const long long n = (long long)B * 4 * H * W * C;
    hipLaunchKernelGGL(cnf::k_up, dim3(cnf::grid_for(n)), dim3(256), 0, (hipStream_t)stream, in, out, B, H, W, C);
    return cnf::finish("k_up");
}

int cnf_instance_noise(const float* x, float* out, int64_t n, float alpha, uint64_t seed, uint64_t offset,
                       void* stream) {
    if (!out || n < 0) return cnf::set_error(CNF_E_INVALID, "cnf_instance_noise: null output or n < 0");
    if (n == 0) return CNF_OK;
    hipLaunchKernelGGL(cnf::k_noise, dim3(cnf::grid_for(n)), dim3(256), 0, (hipStream_t)stream, x, out, (long long)n,
                       alpha, seed, offset);
    return cnf::finish("k_noise");
}

int cnf_batch_assemble(const float* images, int64_t N, const int64_t* index_dev, const float* label_dev,
                       const cnf_batch_desc* desc, float* xy, int B, void* stream) {
    auto bad = [](const char* why) {
        return cnf::set_error(CNF_E_INVALID, (std::string("cnf_batch_assemble: ") + why).c_str());
    };
    if (!images || !index_dev || !desc || !xy) return bad("null images, index_dev, desc or xy");
    if (B < 1 || N < 1) return bad("B and N must be >= 1");
    const cnf_batch_desc& d = *desc;
    if (d.H <= 0 || d.W <= 0 || d.C <= 0) return bad("H, W and C must be positive");
    if (d.mode != CNF_BATCH_CLASS && d.mode != CNF_BATCH_SR) return bad("unknown mode");
    const bool sr = d.mode == CNF_BATCH_SR;
    if (!sr && !label_dev) return bad("CLASS mode needs label_dev");
    if (sr && label_dev) return bad("SR mode takes no label_dev");
    if (!(d.logit_a == 0.f || (d.logit_a > 0.f && d.logit_a < 0.5f))) return bad("logit_a must be 0 or in (0, 0.5)");
    if (sr && d.logit_a != 0.f) return bad("logit_a is for CLASS mode only");
    if (sr) {
        if (d.x_down < 0 || d.y_levels < 0 || d.x_down + d.y_levels > 8) return bad("bad SR levels");
        const int m = 1 << (d.x_down + d.y_levels);
        if (d.H % m || d.W % m) return bad("H and W must be divisible by 2^(x_down + y_levels)");
    }
    for (float al : {d.alpha0, d.alpha1})
        if (!std::isfinite(al) || al < 0.f || al > 1.f) return bad("alpha0 and alpha1 must be finite and in [0, 1]");
    cnf::BatchArgs a{};
    a.images = images;
    a.index = index_dev;
    a.label = label_dev;
    a.N = (long long)N;
    a.H = d.H;
    a.W = d.W;
    a.C = d.C;
    a.sr = sr;
    a.logit = d.logit_a != 0.f;
    if (a.logit) a.lk = cnf::logit_consts(d.logit_a);
    a.xd = sr ? d.x_down : 0;
    a.yl = sr ? d.y_levels : 0;
    a.residual = sr && d.residual;
    a.on0 = d.alpha0 != 1.f;
    a.on1 = d.alpha1 != 1.f;
    a.alpha0 = d.alpha0;
    a.alpha1 = d.alpha1;
    a.seed0 = d.seed0;
    a.off0 = d.offset0;
    a.seed1 = d.seed1;
    a.off1 = d.offset1;
    const long long n = sr ? (long long)B * (d.H >> d.x_down) * (d.W >> d.x_down) * 2 * d.C
                           : (long long)B * d.H * d.W * (d.C + 1);
    hipLaunchKernelGGL(cnf::k_batch, dim3(cnf::grid_for(n)), dim3(256), 0, (hipStream_t)stream, a, xy, n);
    return cnf::finish("k_batch");
}

}  // extern "C"
