/*
 * cnf.h — C ABI of libcnf_hip.so, the MI355X (gfx950) implementation of the
 * conditional-RealNVP forward / inverse + Jacobian log-det hot path of
 * USArmyResearchLab/ARL_Conditional_Normalizing_Flows.
 *
 * The reference is pure TensorFlow/Keras Python and has no FFI of its own; the
 * interfaces replaced are its Python layer/model protocol, and every entry point
 * below cites the reference function it stands in for
 * (file:line into conv_cINN_make_model.py unless stated).
 *
 * Conventions
 *   - All tensors are device pointers, NHWC, fp32, batch-first, contiguous.
 *   - The caller allocates ALL device memory (params, activations, workspace);
 *     the library never frees caller pointers. A plan owns only small constant
 *     tables (index maps) that it uploads once, lazily, on first use.
 *   - A call's outputs are a function of its inputs and the parameters only. The
 *     library ignores what `workspace` / `train_workspace` hold on entry: they
 *     need not be zeroed and may hold another call's leftovers or NaN patterns
 *     (every region is written in a call before that call reads it). Output
 *     buffers are fully overwritten (the one accumulating argument,
 *     cnf_coupling_forward's logdet_accum, is named as such). No byte outside the
 *     buffers given to a call is read for its result or written, and a graph
 *     replay computes what the eager call does
 *     (tests/test_state_independence.py).
 *   - Every compute call is asynchronous on the given stream (a hipStream_t passed
 *     as void*; NULL = default stream) and may be captured into a hipGraph.
 *   - Return value: 0 = OK, negative = error class (CNF_E_*); the message is
 *     available from cnf_last_error() (thread-local). No C++ exception crosses
 *     the ABI. A plan is not thread-safe: one host thread per plan, one process
 *     per GPU.
 *   - Reductions are deterministic (no float atomics): repeated runs are bitwise
 *     identical.
 */
#ifndef CNF_H_
#define CNF_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CNF_OK 0
#define CNF_E_INVALID (-1)   /* bad argument / shape: the reference's AssertionError */
#define CNF_E_HIP (-2)       /* HIP runtime error */
#define CNF_E_STATE (-3)     /* call out of order / unsupported configuration */

#define CNF_GROUP_REFERENCE 0 /* late-bound Lambda closure: every group reads the last slice
                                 (conv_cINN_base_functions.py:402) — the reference's behaviour */
#define CNF_GROUP_INTENDED 1  /* textbook grouped conv: group j reads slice j */

#define CNF_LAYER_COUPLING 0
#define CNF_LAYER_SQUEEZE 1
#define CNF_LAYER_FACTOR 2

typedef struct cnf_plan cnf_plan;

/* Constructor arguments of cFlow.__init__ (conv_cINN_make_model.py:1431-1442). */
typedef struct cnf_flow_desc {
    int io_h, io_w, io_d;                 /* io_shape */
    int x_d;                              /* depth of x inside xy */
    int num_blocks;                       /* len(squeeze_factor_block_list) */
    const int* squeeze_factor_block_list; /* [num_blocks], entries 0/1 */
    const int* resnext_block_list;        /* [num_blocks] */
    const int* num_kernels_list;          /* [num_blocks] */
    const int* cardinality_list;          /* [num_blocks] */
    float lambda_y;                       /* default 100 */
    int ksize;                            /* default 3 (only 3 is implemented on GPU) */
    /* Limits of the kernels beyond the reference's asserts, checked at cnf_plan_create (CNF_E_INVALID,
     * "conv with more than 64 output channels"): no convolution inside an s,t network has more than 64
     * output channels, i.e. every num_kernels_list entry is at most 64 (k_net_lds holds at most 64, and
     * the streamed kernels tile 64 output columns; only conv_out is split into 64-channel chunks, so
     * dc2 may exceed 64). Compressed images are at most 128 pixels wide. */
    int layer_norm;                       /* LAYER_NORM, default 1 */
    int dilations;                        /* DILATIONS, default 1 */
    int group_mode;                       /* CNF_GROUP_* (default REFERENCE) */
    /* Debug options, NULL or "" for the defaults (what is benchmarked): "NAME=V[,NAME=V...]" selecting
     * the alternative code paths the parity tests compare against — NETLDS, GC, PW, GENERIC, LAYOUT,
     * FUSE_COUPLING, LDS_BWD, TRAIN_ALT, TRAIN_SCHED, SCHEDULE_CHECK, PRESPLIT (meanings: csrc/cnf_kernels.h Options). Parsed at
     * cnf_plan_create (unknown name: CNF_E_INVALID); the string is not kept. Without a GENERIC entry, a
     * flow on images of 64 x 64 and above runs the generic k_pw / k_gc kernels (GENERIC=6; the
     * shape-specialised ones showed intermittent differences there). The library reads no
     * environment variable. No reference counterpart (the Keras model has no such switches). */
    const char* debug_options;
} cnf_flow_desc;

/* One entry of cFlow.layers_list (conv_cINN_make_model.py:1630-1689). */
typedef struct cnf_layer_info {
    int kind;              /* CNF_LAYER_* */
    int coupling_index;    /* ordinal among coupling layers, -1 otherwise */
    int block;             /* coupling block */
    int h, w, d;           /* io shape of the block (in_shape of the layer) */
    int mask;              /* which_mask 0..3 (coupling) */
    int hc, wc, dc1, dc2;  /* compressed u1c shape / uv2_d (coupling) */
    int num_kernels;       /* halved for checkerboard masks (:420-423) */
    int cardinality;
    int num_res_blocks;
    int num_dilations;
    int dilations[8];
    int num_prev_factors;  /* factor layers (:230-240) */
    int fused_net;         /* 1: both s,t nets run as one workgroup per image (k_net_lds) */
} cnf_layer_info;

/* Plan = cFlow.__init__ (:1431-1695): asserts, scale schedule, dilation
 * schedule, layer list, canonical parameter table. Host-only, no GPU work.
 * A created plan can be scheduled: after the reference's asserts, the forward and
 * the inverse schedule are dry-run on the host, and a configuration they cannot
 * run is refused here with the schedule's message, not on the first batch
 * (debug option SCHEDULE_CHECK=0: the plan tables alone, for host-side checks;
 * that is the default for CNF_GROUP_INTENDED, SCHEDULE_CHECK=1 asks for the
 * check there too, as cFlow does). */
int cnf_plan_create(const cnf_flow_desc* desc, cnf_plan** out);
void cnf_plan_destroy(cnf_plan* plan);

int cnf_plan_num_layers(const cnf_plan* plan);
int cnf_plan_layer_info(const cnf_plan* plan, int layer, cnf_layer_info* out);

/* Canonical parameters: one flat fp32 vector, tensors in Keras order (net A,
 * then net b, per coupling layer; Conv2D kernels HWIO, LayerNormalization
 * gamma/beta over the flattened H*W*C axis). */
int64_t cnf_plan_num_params(const cnf_plan* plan);
int cnf_plan_num_param_tensors(const cnf_plan* plan);
int cnf_plan_param_tensor(const cnf_plan* plan, int index, char* name, int name_cap,
                          int64_t* offset, int* ndim, int shape[4]);

/* Device-side auxiliary parameter image (every conv's weights in its kernel's
 * staging layout, the grouped convs as dense images built from the per-group
 * Conv2D kernels, and the streamed layers' LN2 / LN3 gamma/beta gathered into
 * their t1 / t2 sub-tensor layouts). Size in floats; filled by cnf_pack_params,
 * which must run again whenever the canonical params change. */
int64_t cnf_plan_aux_floats(const cnf_plan* plan);
int cnf_pack_params(cnf_plan* plan, const float* params, float* aux, void* stream);

/* Workspace bytes for a batch of B images (all activations, LN-stat partials,
 * log-det partials). */
size_t cnf_plan_workspace_bytes(const cnf_plan* plan, int B);

/* cFlow.call(xy, direction=+1) (:1743-1772): xy[B,H,W,D] -> zy[B,H,W,D] in xy
 * layout, logdet_per_image[B] = sum over coupling layers of sum_{h,w,c} A(u1)
 * (the reference returns its batch mean, :1323-1326). xy and zy must not alias
 * (CNF_E_INVALID): the reference returns new tensors, and the fused schedule
 * reads xy after zy's first writes. */
int cnf_flow_forward(cnf_plan* plan, const float* params, const float* aux,
                     const float* xy, float* zy, float* logdet_per_image,
                     void* workspace, int B, void* stream);

/* cnf_flow_forward of the input as the reference's training pipeline prepares it
 * (conv_cINN.py:246-315): with logit_a in (0, 0.5) the logit map of
 * preprocess_dataset_class(LOGITS=True, a=logit_a) on the x channels
 * (conv_cINN_base_functions.py:174-231; 0: none), then instance_noise(., alpha) on every
 * channel (:635-654, the pipeline's 2 % noise: alpha = 0.98). xy_noisy[B,H,W,D] receives the
 * prepared input -- bit for bit cnf_logit (x channels) followed by cnf_instance_noise(.,
 * xy_noisy, B*H*W*D, alpha, seed, offset) -- and zy / logdet_per_image are cnf_flow_forward
 * of it. The preparation runs inside the first coupling layer's gather (no pass over xy)
 * when that layer is LDS-resident, otherwise as one pass first. xy_noisy is the xy of the
 * matching cnf_nll call. No two of xy, xy_noisy, zy may alias. */
int cnf_flow_forward_noise(cnf_plan* plan, const float* params, const float* aux,
                           const float* xy, float logit_a, float alpha, uint64_t seed,
                           uint64_t offset, float* xy_noisy, float* zy, float* logdet_per_image,
                           void* workspace, int B, void* stream);

/* cFlow.call(zy, direction=-1) (:1774-1798): zy -> xy (must not alias). */
int cnf_flow_inverse(cnf_plan* plan, const float* params, const float* aux,
                     const float* zy, float* xy, void* workspace, int B, void* stream);

/* cnf_flow_inverse that also returns logdet_per_image[B] = log|det d xy / d zy|
 * = -(sum over coupling layers of sum_{h,w,c} s), s = tanh_w * tanh(s_pre) as the inverse itself
 * evaluates it (from the conditioning half it sees). xy is bit for bit cnf_flow_inverse's.
 * Every coupling's sum goes into its log-det partial slots of the workspace (the forward's slots:
 * cnf_plan_workspace_bytes is unchanged), written once by the kernel that applies its law, and one
 * fixed-order fp64 reduction per image follows (no atomics: the result does not depend on B, the
 * stream or the workspace's earlier contents). Aliasing rules and argument errors as
 * cnf_flow_inverse; a NULL logdet_per_image is CNF_E_INVALID before any HIP call. */
int cnf_flow_inverse_logdet(cnf_plan* plan, const float* params, const float* aux,
                            const float* zy, float* xy, float* logdet_per_image,
                            void* workspace, int B, void* stream);

/* Conditional sampling: S draws of x given y for each of B conditions, and their per-pixel
 * statistics. Replaces the recipe the reference's users write by hand (TOYcINN.py:807-817: draw z
 * from the prior, concatenate the condition y, call the model in the generative direction,
 * conv_cINN_make_model.py:1774-1798) together with the post-transforms and the reduction over
 * the draws that follow it.
 *
 * Latent: with H, W, D = io shape, the latent of condition b, draw s, pixel p, channel c < x_d is
 * temperature * element offset + ((b*S + s)*H*W + p)*x_d + c of the seed's stream, i.e. exactly
 * what cnf_instance_noise(NULL, out, B*S*H*W*x_d, 0, seed, offset) writes into a [B,S,H,W,x_d]
 * tensor, times temperature in one fp32 multiply; zy[b,s] = concat(latent, y[b]) in the xy layout.
 * Inverse and post-transforms: xy_hat = cnf_flow_inverse(zy); per drawn value take x_hat (the
 * first x_d channels), apply de_logitify (cnf_logit(., a, inverse)) if logit_a, then add the INPUT
 * y (not y_hat) if residual. `samples` holds these values; `mean` and `std` are over the S draws of
 * each condition in population form (divide by S, as np.std and tf.math.reduce_std do);
 * y_dev[b,s] = sum_{h,w,c} |y_hat - y| of that draw, the unweighted sum of log_loss's lly term
 * (:1815-1848): whether the draw honours its condition.
 * The B*S images run through the inverse `chunk` at a time; no result depends on chunk, bit for
 * bit (the per-element statistics are carried across chunks in draw order as a shifted sum
 * (K, S1, S2), K the first draw's value, S1 = sum (v - K), S2 = sum (v - K)^2, and
 * mean = K + S1/S, std = sqrt(max(0, (S2 - S1^2/S)/S))). */
typedef struct cnf_sample_desc {
    int   num_samples;   /* S >= 1 draws per condition */
    int   chunk;         /* images per inverse call, >= 1; results do not depend on it */
    float temperature;   /* z = temperature * N(0,1); >= 0 (0: the mode of the prior) */
    uint64_t seed, offset; /* Philox stream, as cnf_instance_noise */
    float logit_a;       /* 0: none; in (0,0.5): de_logitify(., a) on every drawn x value */
    int   residual;      /* 1: x + y per sample (preprocess_dataset_SR RESIDUAL=True);
                            needs io_d - x_d == x_d */
} cnf_sample_desc;

/* Workspace bytes of cnf_flow_sample for B conditions: cnf_plan_workspace_bytes(desc->chunk), the
 * zy and xy_hat buffers of one chunk and the statistics state (3*B*H*W*x_d floats); independent of
 * num_samples. 0 for a NULL or invalid argument. */
size_t cnf_plan_sample_workspace_bytes(const cnf_plan* plan, int B, const cnf_sample_desc* desc);

/* y: [B][H][W][D - x_d]. Outputs, each may be NULL but not all: samples [B][S][H][W][x_d], mean and
 * std [B][H][W][x_d], y_dev [B][S]. CNF_E_INVALID before any HIP call for: NULL y, S < 1, chunk < 1,
 * temperature < 0 or not finite, logit_a outside {0} u (0, 0.5), residual with D - x_d != x_d, no
 * output requested, B < 1. The launches are recorded as cnf_flow_inverse's (measurement hooks). */
int cnf_flow_sample(cnf_plan* plan, const float* params, const float* aux, const float* y,
                    const cnf_sample_desc* desc, float* samples, float* mean, float* std,
                    float* y_dev, void* workspace, int B, void* stream);

/* cnf_flow_sample plus log_prob[B][S] (may be NULL; counts as a requested output):
 * log_prob[b,s] = llz + sum_layers sum s, i.e. the llz + logdet that cnf_nll reports for the pair
 * (xy_hat, zy) of that draw: the model's log-density of the draw in the flow's input space (before
 * de_logitify / residual; the prior is N(0, I) whatever the temperature; y_dev carries the lly part).
 * Arithmetic, with z the fp32 latent as stored in the chunk's zy and n = H*W*x_d: q = the fp64 sum
 * of (double)z * (double)z over the image's latent (lane-strided partial sums in element order, then
 * a fixed-order wave sum), L = the fp64 sum of the image's log-det partial slots over all couplings
 * in cnf_flow_inverse_logdet's reduction order, log_prob = (float)(-0.5*q - 0.5*n*log(2*pi) + L).
 * One extra launch per chunk, which reads the slots directly. cnf_sample_desc, the workspace size
 * (cnf_plan_sample_workspace_bytes) and the bits of samples, mean, std and y_dev are
 * cnf_flow_sample's; no result depends on chunk, bit for bit. */
int cnf_flow_sample_logp(cnf_plan* plan, const float* params, const float* aux, const float* y,
                         const cnf_sample_desc* desc, float* samples, float* mean, float* std,
                         float* y_dev, float* log_prob, void* workspace, int B, void* stream);

/* Scoring the draws against a truth inside the sampling call: where the truth ranks among the draws of
 * its element, the per-element distribution of the draws, and how far each draw is from the truth,
 * without a [B][S][...] tensor. v below is the value `samples` holds for (b, s, p, c) (after de_logitify
 * and the residual), bit for bit; truth [B][H][W][x_d] lives in that space.
 *   rank[b,p,c]     int32: the number of draws with v < truth (strict, fp32). Uniform on 0..S for a
 *                   calibrated model (the rank / PIT histogram).
 *   abs_err[b,p,c]  the mean over the draws of |v - truth|: an fp32 sum in draw order, divided by S.
 *   sq_err[b,s]     (float) sum_{p,c} ((double)v - (double)truth)^2 of that draw: which draw is closest.
 *   hist[b,p,c,k]   int32, k < bins: the draws with k == (int)floorf((v - lo) * scale), scale =
 *                   (float)bins / (hi - lo) in fp32 (cnf_toy_sample's expression); draws outside
 *                   [lo, hi) and NaN are not counted, so sum_k hist <= S.
 *   quantiles[j,b,p,c]  for level q = quantiles[j] of the descriptor, from hist: N = sum_k hist[k],
 *                   target = q * N (fp32), k the first bin with cumulative count C_k >= target and
 *                   C_k > 0, value lo + (k + (target - C_{k-1}) / hist[k]) * (hi - lo) / bins, clamped to
 *                   [lo, hi]; within one bin width of the inverted-CDF quantile of the counted draws.
 *                   NaN where N == 0.
 * The outputs are the state between chunks (the chunk holding b's first draw initialises b's entries), so
 * the workspace is cnf_flow_sample's, nothing depends on what the buffers held, and no result depends on
 * chunk, bit for bit. */
typedef struct cnf_sample_score_desc {
    int bins;               /* 0: no histogram; else 2..256 */
    float lo, hi;           /* finite, lo < hi, when bins != 0 */
    int num_quantiles;      /* 0..8; needs bins != 0 */
    float quantiles[8];     /* each in [0, 1] */
} cnf_sample_score_desc;

/* cnf_flow_sample_logp plus the score outputs, each may be NULL; with all of them NULL (score may then
 * be NULL too) the launches are cnf_flow_sample_logp's. CNF_E_INVALID before any HIP call, besides
 * cnf_flow_sample's cases, for: a NULL score descriptor with a score output given; rank, abs_err or
 * sq_err without truth; hist with bins == 0; bins outside 2..256; lo or hi not finite or lo >= hi;
 * quantiles without hist, num_quantiles outside 1..8, or a level outside [0, 1] or NaN. */
int cnf_flow_sample_score(cnf_plan* plan, const float* params, const float* aux, const float* y,
                          const cnf_sample_desc* desc, const cnf_sample_score_desc* score,
                          const float* truth, float* samples, float* mean, float* std, float* y_dev,
                          float* log_prob, int* rank, float* abs_err, float* sq_err, int* hist,
                          float* quantiles, void* workspace, int B, void* stream);

/* Cascaded super-resolution sampling: L stages, 1 <= L <= 4, of flows trained independently per level
 * (conv_cINN.py:28-30, one model for 'SR4,2', one for 'SR2,1'), chained at inference. All stages have the
 * same x_d = C and io_d = 2C (y has x's depth); stage l+1's io shape is (2 H_l, 2 W_l, 2C). y [B][H_1][W_1][C]
 * conditions stage 1 (`up` of the low-resolution image, what preprocess_dataset_SR puts in the y channels).
 * Stage l has N_l = S_1 * ... * S_l nodes per condition; node g of the flat [B][N_l] order has parent
 * g / S_l at stage l - 1 and condition b = g / N_l. For a node:
 *   latent     temperature[l] * element offset[l] + (g*H_l*W_l + p)*x_d + c of the seed's stream:
 *              cnf_flow_sample's rule with S replaced by N_l
 *   condition  stage 1: y[b]; deeper: y_l = cnf_up (the 2x2 repeat) of the parent's value
 *   value      v_l = the value cnf_flow_sample returns for (latent, y_l): x_hat of the stage's inverse,
 *              de_logitify if logit_a, + y_l (the node's own input condition, not y_hat) if residual
 * The one rule: the next stage's condition is `up` of what cnf_flow_sample would have returned. The cascade
 * therefore equals, bit for bit, the composition of cnf_flow_sample calls on B*N_{l-1} conditions with
 * cnf_up between them, without materialising any [B][N_l][...] tensor but the leaves (if asked for).
 * Outputs: samples [B][N_L][H_L][W_L][C], the leaves; per stage mean_l, std_l [B][H_l][W_l][C] over the
 * N_l nodes of a condition in node order (cnf_flow_sample's (K, S1, S2) fold with S = N_l); y_dev_l
 * [B][N_l] as cnf_flow_sample's, against the node's own condition; block_dev_l [B][N_l], the reference's
 * stated sanity check (conv_cINN.py:44: the 2x2 pixel blocks of the residual sum to 0):
 *   block_dev = (float) sum over 2x2 blocks and c of | 0.25 * sum over the block's 4 pixels, row-major, of
 *               ((double)v_l - (double)y_l) |, one wave per node, fp64 lane sums over (block, c) in element
 *               order, then the fixed-order wave sum; 0 for a draw whose `down` reproduces its condition;
 * and on the leaves, with S = N_L, cnf_flow_sample_score's rank, abs_err, sq_err, hist, quantiles.
 * Traversal: depth-first in node order with one chunk buffer per stage: stage-1 nodes run `chunk` at a
 * time; the S_{l+1} children of each node of a finished chunk run through the next stage `chunk` at a
 * time (a child chunk may straddle parents and conditions). Every stage visits its nodes in increasing g,
 * the folds are cnf_flow_sample's serial folds, and no result depends on chunk, bit for bit. */
typedef struct cnf_cascade_desc {
    int   num_stages;       /* L in 1..4 */
    int   num_samples[4];   /* S_l >= 1 children per parent node (stage 1: draws per condition) */
    int   chunk;            /* images per inverse call of every stage, >= 1 */
    float temperature[4];   /* per stage, finite and >= 0 */
    uint64_t seed;
    uint64_t offset[4];     /* per stage; to put the stages' streams one after the other:
                               offset[l] = offset[l-1] + B*N_{l-1}*H_{l-1}*W_{l-1}*x_d */
    float logit_a;          /* as cnf_sample_desc, applied at every stage */
    int   residual;
} cnf_cascade_desc;

/* Workspace bytes: the sum over the stages of cnf_plan_sample_workspace_bytes(plans[l], B, chunk) (that
 * plan's inverse workspace for `chunk` images, one chunk each of zy and xy_hat, the 3*B*H_l*W_l*x_d
 * statistics state); independent of every S_l. 0 for a NULL or invalid argument (cnf_last_error). */
size_t cnf_cascade_workspace_bytes(const cnf_plan* const* plans, int B, const cnf_cascade_desc* desc);

/* plans, params, aux: arrays of L entries. mean, std, y_dev, block_dev: NULL or arrays of L per-stage
 * pointers, each entry may be NULL. score / truth / rank .. quantiles: cnf_flow_sample_score's, on the
 * leaves (truth [B][H_L][W_L][C]). At least one output must be requested. CNF_E_INVALID before any HIP
 * call, the message naming the argument (and the stage where one is at fault), for: every case
 * cnf_flow_sample / cnf_flow_sample_score reject, per stage where it applies; num_stages outside 1..4; a
 * NULL plans / params / aux array or entry; io_d != 2 x_d; an x_d or io-shape mismatch between consecutive
 * stages; N_L beyond 2^31 - 1; block_dev at a stage with odd H or W; no output. The launches are recorded on the plan of the stage they belong to (measurement
 * hooks): k_latent / k_child_latent, the inverse's, k_sample_fold_node, k_sample_ydev_node,
 * k_block_dev, k_sample_score_node, k_sample_sqerr_node, k_sample_quantiles. */
int cnf_flow_sample_cascade(cnf_plan* const* plans, const float* const* params, const float* const* aux,
                            const float* y, const cnf_cascade_desc* desc,
                            const cnf_sample_score_desc* score, const float* truth, float* samples,
                            int* rank, float* abs_err, float* sq_err, int* hist, float* quantiles,
                            float* const* mean, float* const* std, float* const* y_dev,
                            float* const* block_dev, void* workspace, int B, void* stream);

/* The density of given images: the counterpart of cnf_flow_sample. x[B][H][W][x_d] lives in the space
 * of the returned samples (after de_logitify and the residual); every image is scored against its own
 * condition (paired) or against each of K conditions (pairwise), N = B or B*K pairs, pair i =
 * (image, condition) = (i / K, i % K). For pair i, with v the flow-space image of x:
 *   v        = logit(x - y): the input y is subtracted if residual, then cnf_logit's forward map is
 *              applied if logit_a -- the exact inverse of cnf_flow_sample's post-transforms, in the
 *              kernels' own fp32 expressions; xy = concat(v, y), every y channel unchanged
 *   llz, logdet  as cnf_nll reports them for (xy, zy = cnf_flow_forward(xy))
 *   y_dev    = sum_{h,w,c} |y_hat - y|, unweighted, as cnf_flow_sample's
 *   log_jac  = sum over the image's x elements of log|dv/dx|: 0 without logit_a (the residual shift has
 *              unit Jacobian); with it each element adds log c1 - log e - log(1 - e) - log span,
 *              e = a + c1 x' (x' = x - y if residual), c1 = (1 - a) b = 1 - 2a, span = logit(1 - a) -
 *              logit(a), in fp64 from the fp32 e the map itself uses
 *   log_prob = llz + logdet + log_jac: cnf_flow_sample_logp's log_prob moved into the sample space
 * An image with an element outside the map's domain (e not in (0, 1), NaN included) has density 0 under
 * every such pair: log_prob = log_jac = -inf, and llz, logdet, y_dev are NaN (the flow ran on 0 in that
 * element's place, so nothing non-finite enters it or reaches another pair).
 * posterior[b][k] = softmax_k(log_prob[b][k] + log_prior[k]) (log_prior NULL: uniform, + 0) and
 * log_evidence[b] = that row's log-sum-exp, both in fp64 from the fp32 log_prob, max-shifted; a row whose
 * entries are all -inf gives a NaN posterior and -inf evidence.
 * The pairs run through the forward `chunk` at a time: per chunk a gather (xy and the log_jac partials),
 * cnf_flow_forward's launches, and one finishing pass over zy; then, if asked for, the posterior. Every
 * sum is taken in a fixed order that depends on the image shape alone, so no result depends on chunk, B,
 * K, the pair's place in its chunk, the stream or the workspace's earlier contents, bit for bit, and the
 * pairwise call equals the paired call on the B*K expanded pairs. */
typedef struct cnf_logp_desc {
    int   num_conditions; /* K >= 1: y is [K][H][W][D-x_d], every image against every condition,
                             outputs [B][K]; 0: paired, y is [B][H][W][D-x_d], outputs [B] */
    int   chunk;          /* pairs per forward, >= 1; results do not depend on it */
    float logit_a;        /* 0: none; in (0,0.5): x is in de_logitify(., a)'s output space */
    int   residual;       /* 1: x is x_flow + y; needs io_d - x_d == x_d */
} cnf_logp_desc;

/* Workspace bytes of cnf_flow_log_prob: cnf_plan_workspace_bytes(desc->chunk), one chunk each of xy, zy,
 * the per-image log-det and the log_jac partials; independent of B and of num_conditions. 0, with the
 * reason in cnf_last_error, for a NULL or invalid argument. */
size_t cnf_plan_logp_workspace_bytes(const cnf_plan* plan, int B, const cnf_logp_desc* desc);

/* Outputs log_prob, llz, logdet, log_jac, y_dev: [N] each, any may be NULL; posterior [B][K] and
 * log_evidence [B] (pairwise only; they read log_prob, which must then be given); log_prior [K] or NULL.
 * CNF_E_INVALID before any HIP call for: a NULL plan, params, aux, workspace, x or y; B < 1; no output
 * requested; num_conditions < 0; chunk < 1; logit_a outside {0} u (0, 0.5); residual with D - x_d != x_d;
 * posterior or log_evidence in paired mode or without log_prob; log_prior without posterior or
 * log_evidence. The launches are recorded under their own names (k_logp_gather, the forward's,
 * k_logp_finish per chunk, k_logp_posterior) for the measurement hooks below. */
int cnf_flow_log_prob(cnf_plan* plan, const float* params, const float* aux, const float* x,
                      const float* y, const cnf_logp_desc* desc, float* log_prob, float* llz,
                      float* logdet, float* log_jac, float* y_dev, const float* log_prior,
                      float* posterior, float* log_evidence, void* workspace, int B, void* stream);

/* The input gradients of the log-density: grad_x [B][H][W][x_d] = d log_prob[b] / d x[b] and grad_y
 * [B][H][W][D-x_d] = d log_prob[b] / d y[b] of cnf_flow_log_prob's paired log_prob = llz + logdet + log_jac
 * (image b under condition b), with x and y as that call takes them (x in the space of the samples; the
 * condition enters through the y channels of the flow's input and, with residual, through x - y).
 * Per chunk: cnf_flow_log_prob's gather, cnf_flow_forward_train's schedule, the seed d(llz + logdet)/dzy
 * (k_score_seed: -z on the x channels, 0 elsewhere, log-det weight +1), the training backward restricted to
 * the data gradients -- no launch whose only outputs are parameter gradients, no dparams -- and k_score_finish,
 * which takes the flow-input gradient g through the gather's map: with v = x - y (residual) or x and
 * e = a + c1 v, t = g_x c1 / (span e (1 - e)) - c1 (1 - 2e) / (e (1 - e)) (t = g_x without logit_a);
 * grad_x = t, grad_y = g_y (- t with residual). log_prob [B] is cnf_flow_log_prob's value up to the rounding
 * of the training forward's schedule. Any of the three outputs may be NULL, not all; with grad_x and grad_y
 * NULL no backward runs. An image with an element outside the logit map's domain gets log_prob = -inf and NaN
 * gradients; the other images are untouched. log_prob does not depend on chunk bit for bit; the gradients
 * agree across chunk up to fp32 rounding (k_tconv_band's tile height, and with it the number of partials of
 * the fused LayerNorm-backward reduction per image, follows the launch's workgroup count, which counts the
 * chunk's images). */
typedef struct cnf_score_desc {
    int   chunk;          /* images per forward / backward, >= 1 */
    float logit_a;        /* as cnf_logp_desc */
    int   residual;
} cnf_score_desc;

/* Workspace bytes of cnf_flow_score: cnf_plan_train_workspace_bytes(desc->chunk), the dense backward image
 * (packed once per call), one chunk each of xy, zy, the seed, the per-image log-det, the log_jac partials and
 * llz; independent of B. 0, with the reason in cnf_last_error, for a NULL or invalid argument. */
size_t cnf_plan_score_workspace_bytes(const cnf_plan* plan, int B, const cnf_score_desc* desc);

/* CNF_E_INVALID before any HIP call, with "cnf_flow_score: " and the reason in cnf_last_error, for: a NULL
 * plan, params, aux, workspace, x or y; all of grad_x, grad_y, log_prob NULL; a NULL desc; B < 1; chunk < 1;
 * logit_a outside {0} u (0, 0.5); residual with D - x_d != x_d. Not capturable into a graph when a streamed
 * layer's backward forks onto the plan's side stream. */
int cnf_flow_score(cnf_plan* plan, const float* params, const float* aux, const float* x, const float* y,
                   const cnf_score_desc* desc, float* grad_x, float* grad_y, float* log_prob,
                   void* workspace, int B, void* stream);

/* Gradient ascent on the flow-input-space log-density llz + logdet (what cnf_flow_sample_logp reports for a
 * draw) over the x channels of the flow's input, y fixed. Per chunk: x0 is gathered into flow space as above
 * (u0 = logit_value(x0 - y)); `steps` times the training forward, the seed, the data-gradient backward and
 * k_ascend_step -- Keras Adam (cnf_adam_step's arithmetic) with the gradient -g, written in place into the xy
 * the next forward reads; one last forward; x_out [B][H][W][x_d] = the iterate through the sampler's
 * post-transform (de_logitify, + y). log_prob_trace [steps+1][B]: row t = llz + logdet of iterate t, row 0 the
 * start, row `steps` what x_out holds. No host synchronisation between steps. m, v [B][H][W][x_d] (both or
 * neither): Adam's moments, read and written, so that a run continues with first_step = the steps taken so far
 * (the step counter starts at first_step + 1); NULL: the state lives in the workspace and starts at zero.
 * The mode of a density depends on the parametrisation: with logit_a this is the mode in flow-input space,
 * not in pixel space. An image with an element outside the logit map's domain gets -inf in every trace row
 * and x_out = x0. */
typedef struct cnf_ascend_desc {
    int   chunk, steps;   /* images per forward / backward, >= 1; ascent steps, >= 0 */
    float lr, beta_1, beta_2, epsilon;   /* Adam: lr finite, betas in [0, 1), epsilon >= 0 */
    float logit_a;        /* as cnf_logp_desc */
    int   residual;
    int   first_step;     /* Adam steps already taken on m, v; >= 0 */
} cnf_ascend_desc;

/* Workspace bytes of cnf_flow_ascend: cnf_flow_score's plus one chunk of m and v; independent of B. */
size_t cnf_plan_ascend_workspace_bytes(const cnf_plan* plan, int B, const cnf_ascend_desc* desc);

/* CNF_E_INVALID before any HIP call, with "cnf_flow_ascend: " and the reason in cnf_last_error, for: a NULL
 * plan, params, aux, workspace, x0, y, x_out or log_prob_trace; one of m, v without the other; a NULL desc;
 * B < 1; chunk < 1; steps < 0; first_step < 0; lr not finite; a beta outside [0, 1); epsilon negative or not
 * finite; logit_a outside {0} u (0, 0.5); residual with D - x_d != x_d. x_out may be x0. */
int cnf_flow_ascend(cnf_plan* plan, const float* params, const float* aux, const float* x0, const float* y,
                    const cnf_ascend_desc* desc, float* x_out, float* log_prob_trace, float* m, float* v,
                    void* workspace, int B, void* stream);

/* coupling_layer.forward_and_Jacobian (:1258-1328) for layer `layer` of
 * layers_list: u -> v (shape of the layer's in_shape); logdet_accum[B] +=
 * per-image sum of A(u1) (pass NULL to skip). u and v must not alias. */
int cnf_coupling_forward(cnf_plan* plan, int layer, const float* params, const float* aux,
                         const float* u, float* v, float* logdet_accum,
                         void* workspace, int B, void* stream);

/* coupling_layer.backward (:1333-1394): v -> u. */
int cnf_coupling_inverse(cnf_plan* plan, int layer, const float* params, const float* aux,
                         const float* v, float* u, void* workspace, int B, void* stream);

/* cnf_coupling_inverse with logdet_accum[B] -= per-image sum of s (NULL: skip), the mirror of
 * cnf_coupling_forward's logdet_accum. */
int cnf_coupling_inverse_logdet(cnf_plan* plan, int layer, const float* params, const float* aux,
                                const float* v, float* u, float* logdet_accum,
                                void* workspace, int B, void* stream);

/* squeeze_layer (:155-217): dir=+1 space_to_depth(2) in TF channel order,
 * dir=-1 depth_to_space(2). in: [B,H,W,C] (dir=+1) or [B,H,W,4C'] (dir=-1). */
int cnf_squeeze(const float* in, float* out, int B, int H, int W, int C, int dir, void* stream);

/* Channel-window copy used by factor_out_zy_layer (:256-329):
 * out[b,p,out_off + c] = in[b,p,in_off + c] for c < C, p < HW. */
int cnf_channel_copy(const float* in, int in_cs, int in_off, float* out, int out_cs, int out_off,
                     int C, int B, int HW, void* stream);

/* cFlow.log_loss terms (:1815-1848). per_image[B*3] = (llz, lly, logdet) with
 * llz = sum_{h,w} log N(z; 0, I_{x_d}), lly = -lambda_y * sum |y - y'|;
 * sums[4] = (sum_i loss_i, sum_i -llz_i, sum_i -lly_i, sum_i -logdet_i),
 * loss_i = -(llz_i + lly_i + logdet_i). Dividing sums by the (global) batch
 * gives the reference's (loss, z_loss, y_loss, detJ_loss). One kernel launch;
 * its last workgroup is found through a completion counter the plan keeps per
 * stream, so calls on different streams may run concurrently. 64 counters per
 * plan: a 65th stream reuses the least recently used one, its launch ordered
 * after that counter's last launch (a stream wait, no host wait; inside graph
 * capture that slot needs one earlier uncaptured call). The first call on a plan uploads its tables (not capturable:
 * cnf_pack_params does the same, call it before graph capture). */
int cnf_nll(const cnf_plan* plan, const float* xy, const float* zy, const float* logdet_per_image,
            float* per_image, float* sums, int B, void* stream);

/* ---------------------------------------------------------------------------
 * NLL training step (cFlow.train_step, :1850-1880: GradientTape over log_loss,
 * then Adam). Replaces the TF autodiff of the whole log_loss graph.
 * ------------------------------------------------------------------------- */

/* Training workspace bytes for B images (the inference workspace, the saved
 * coupling-layer inputs, one layer's recomputed activations, gradient buffers). */
size_t cnf_plan_train_workspace_bytes(const cnf_plan* plan, int B);

/* cnf_flow_forward that also saves every coupling layer's input into
 * train_workspace (for cnf_flow_backward on the same xy / zy). */
int cnf_flow_forward_train(cnf_plan* plan, const float* params, const float* aux,
                           const float* xy, float* zy, float* logdet_per_image,
                           void* train_workspace, int B, void* stream);

/* dparams[num_params] = d loss / d params for this shard, where
 * loss = -(sum_i (llz_i + lly_i + logdet_i)) * inv_batch (inv_batch = 1 / global
 * batch size: summing dparams over data-parallel shards gives the gradient of the
 * reference's batch-mean loss). d|y - y'| / dy = sign(y - y') (0 at 0), as TF. */
int cnf_flow_backward(cnf_plan* plan, const float* params, const float* xy, const float* zy,
                      void* train_workspace, int B, float inv_batch, float* dparams, void* stream);

/* cnf_flow_backward for data-parallel training with the gradient reduction
 * overlapped (conv_cINN_make_model.py:1863-1870):
 *  - global_count (device, 1 float) is the global image count, e.g. red5[4] of
 *    cnf_nll_allreduce: inv_batch = 1 / *global_count is taken on the device, so
 *    no host read of the all-reduced count sits between forward and backward;
 *  - layer_done (may be NULL) is called on the calling host thread as soon as the
 *    launches producing coupling layer `coupling_index`'s parameter gradients
 *    (names "c<index>.*", one contiguous range of dparams) are enqueued on
 *    `stream` (the backward's side streams have joined it). Work the callback
 *    enqueues behind that point on `stream` (or on a stream waiting for it), e.g.
 *    cnf_allreduce_sum_f32 of that range, overlaps the backward of the layers
 *    before it. Every coupling layer is reported exactly once, in an order that is
 *    the same on every rank: reverse index order, except that a layer whose
 *    weight gradients run on a side stream (the split LDS-layer backward) is
 *    reported when the stream first waits for them, two such layers later. */
typedef void (*cnf_layer_done_fn)(void* user, int coupling_index);
int cnf_flow_backward_ex(cnf_plan* plan, const float* params, const float* xy, const float* zy,
                         void* train_workspace, int B, const float* global_count, float* dparams,
                         cnf_layer_done_fn layer_done, void* user, void* stream);

/* Backward of one coupling layer (layer index into layers_list) at input u:
 * du = dL/du and dparams = dL/dparams (zeroed first; only this layer's entries
 * are non-zero) for upstream dv = dL/dv and dlogdet = dL/d(per-image log-det). */
int cnf_coupling_backward(cnf_plan* plan, int layer, const float* params, const float* u,
                          const float* dv, float* du, float dlogdet, void* train_workspace,
                          int B, float* dparams, void* stream);

/* Keras Adam (conv_cINN.py:567 Adam(3e-4); keras defaults beta_1 0.9, beta_2 0.999,
 * epsilon 1e-7): m += (g - m)(1 - b1); v += (g^2 - v)(1 - b2);
 * p -= lr sqrt(1 - b2^t) / (1 - b1^t) * m / (sqrt(v) + eps), t = step >= 1. */
int cnf_adam_step(float* params, const float* grads, float* m, float* v, int64_t n, float lr,
                  float beta_1, float beta_2, float epsilon, int step, void* stream);

/* ---- Clipped, guarded Adam (tf.keras.optimizers.Adam's clipvalue / clipnorm / global_clipnorm and
 * use_ema / ema_momentum, plus a skip of steps whose gradient holds a NaN or an infinity). The step
 * size's t is a counter on the device and nothing in the step reads the device from the host, so a
 * graph-captured cnf_optim_step advances on every replay. cnf_adam_step is not changed by any of this.
 *
 * A "tensor" is a range [offsets[t], offsets[t + 1]) of the flat parameter vector (offsets[T + 1]:
 * non-decreasing, offsets[0] = 0, offsets[T] = n; an empty tensor is allowed). With the gradient g:
 *   1. clipvalue c > 0: h = min(max(g, -c), c); otherwise h = g
 *   2. clipnorm c > 0, per tensor: n_t = sqrt(sum_t h^2) (fp64 sum of the fp32 values),
 *      s_t = (float)(c / max(n_t, c)) (1 for a zero or empty tensor); otherwise s_t = 1
 *   3. global_clipnorm c > 0: N = sqrt(sum_t (double)s_t^2 * sum_t h^2), S = (float)(c / max(N, c));
 *      otherwise S = 1 (N is computed and reported either way)
 *   4. g' = fl32(h * scale_t), scale_t = fl32(s_t * S): rounded to fp32 before Adam uses it
 *   5. cnf_adam_step's arithmetic on g' with t = applied + 1 and
 *      alpha = (float)(lr sqrt(1 - beta_2^t) / (1 - beta_1^t)) taken on the device in fp64
 *   6. ema_momentum > 0: ema += (p' - ema) * (1 - ema_momentum), in the same pass as the update
 *   7. skip_nonfinite and any element of g NaN or +-inf: params, m, v and ema are not written,
 *      applied stays and skipped increments (the next good step uses the t this one would have).
 *      Without skip_nonfinite such values propagate as IEEE arithmetic gives.
 * Every sum is taken in a fixed order without atomics (per slab in fp64, a tensor's slabs in slab
 * order, the tensors in table order): results are bitwise repeatable and do not depend on what the
 * workspace held before. */
typedef struct cnf_optim_desc {
    float lr, beta_1, beta_2, epsilon;   /* lr finite, betas in [0, 1), epsilon >= 0 */
    float clipvalue;                     /* 0 = off; else > 0 and finite */
    float clipnorm;                      /* 0 = off; not together with global_clipnorm */
    float global_clipnorm;               /* 0 = off */
    int   skip_nonfinite;                /* non-zero: rule 7 */
    float ema_momentum;                  /* 0 = no EMA; else in (0, 1), and ema must be given */
} cnf_optim_desc;

/* Elements per slab, the unit of work of the three kernels (a multiple of 4). */
int cnf_optim_slab_elems(void);

/* Number of slabs of the table of (n, offsets, T): the sum over tensors of
 * ceil(size_t / cnf_optim_slab_elems()), no slab crossing a tensor boundary. -1 for an invalid
 * argument (n < 1, T < 1, NULL, offsets not non-decreasing from 0 to n). */
int64_t cnf_optim_num_slabs(int64_t n, const int64_t* offsets, int T);

/* Bytes of that table (0 for an invalid argument): num_slabs entries
 * {int64 start, int32 count, int32 tensor} in order of start, then int32 first[T + 1], tensor t's
 * slabs being first[t] .. first[t + 1] - 1. */
size_t cnf_optim_table_bytes(int64_t n, const int64_t* offsets, int T);

/* Writes the table to host_out (cnf_optim_table_bytes bytes). Host code only: the caller copies
 * it to the device once and passes that copy as table_dev to every step. */
int cnf_optim_table_build(int64_t n, const int64_t* offsets, int T, void* host_out);

/* Bytes of cnf_optim_step's workspace (per-slab sums and counts, the tensors' scales, alpha and the
 * skip flag); 0 for an invalid argument. Every byte the step reads it has written in the same call. */
size_t cnf_optim_workspace_bytes(int64_t n, int T, int64_t num_slabs);

#define CNF_OPTIM_STATS_FLOATS 8
/* One step, three launches on `stream`: k_optim_stats (per slab: fp64 sums of g^2 and h^2, the count
 * of non-finite g), k_optim_finish (one workgroup: s_t, N, S, scale_t, skip, the counters, alpha,
 * stats), k_optim_step (clamp, scale, Adam, EMA over the slabs; returns at once on a skipped step).
 *   params, grads, m, v [n]; ema [n] or NULL (required when ema_momentum > 0; the caller sets it to
 *       the parameters before the first step)
 *   table_dev: the device copy of cnf_optim_table_build's table for this (n, offsets, T)
 *   state_dev int64[2]: [0] steps applied, [1] steps skipped; the caller zeroes it once
 *   stats_dev float[CNF_OPTIM_STATS_FLOATS] or NULL: [0] the global norm of g, [1] N of rule 3,
 *       [2] the number of non-finite elements of g, [3] 1 if this step was skipped else 0, [4] alpha,
 *       [5] S, [6..7] 0
 *   scales_dev float[T] or NULL: scale_t of rule 4
 * CNF_E_INVALID before anything is launched ("cnf_optim_step: ..." in cnf_last_error) for a NULL
 * required pointer, n < 1, T < 1, num_slabs < 1, a negative or non-finite clip value, clipnorm
 * together with global_clipnorm, a beta outside [0, 1), a negative epsilon, a non-finite lr, an
 * ema_momentum outside [0, 1), ema_momentum > 0 with ema NULL. (Bad offsets are refused where they
 * are given: cnf_optim_num_slabs / _table_bytes / _table_build.) */
int cnf_optim_step(float* params, const float* grads, float* m, float* v, float* ema, int64_t n,
                   const void* table_dev, int64_t num_slabs, int T, const cnf_optim_desc* desc,
                   int64_t* state_dev, float* stats_dev, float* scales_dev, void* workspace, void* stream);

/* ---------------------------------------------------------------------------
 * TOYcINN (BASELINE configs[0]): the dense conditional flow of
 * TOYcINN_make_model.py:29-506 on 3-dimensional points.
 * ------------------------------------------------------------------------- */
typedef struct cnf_toy_desc {
    int io_shape;              /* must be 3 (the reference masks, :149-163) */
    int x_d;                   /* 1 or 2 */
    int num_coupling_layers;   /* <= 128 */
    int intermediate_dims;     /* H <= 64 */
    int num_layers;            /* hidden Dense layers after the first */
    const int* mask_indices;   /* [num_coupling_layers], a permutation (cINN_affine.mask_indices) */
    float lambda_y;            /* 100 in the reference */
} cnf_toy_desc;

/* Number of fp32 parameters: per network j (j = 0..L-1, mask type j % 6), the b net then the A
 * net, each Dense as kernel [in][out] then bias [out] (:48-94). */
int64_t cnf_toy_num_params(const cnf_toy_desc* d);

/* cINN_affine.call(u, direction) (:237-417): direction -1 = xy' -> zy (reverse layer order,
 * log_detJ[B] = per-sample sum of A), +1 = zy -> xy'. u, v: [B][3], must not alias.
 * per_sample[B*3] (direction -1, optional) = (llz, lly, log_detJ) of log_loss (:419-451). */
int cnf_toy_call(const cnf_toy_desc* d, const float* params, const float* u, float* v, float* log_detJ,
                 float* per_sample, int B, int direction, void* stream);

/* Batch sums of the toy log_loss terms: sums[4] = (sum loss_i, sum -llz_i, sum -lly_i,
 * sum -log_detJ_i); divide by B for the reference's 4-tuple. */
int cnf_toy_nll_sums(const float* per_sample, float* sums, int B, void* stream);

/* ---- TOYcINN training (cINN_affine.train_step, TOYcINN_make_model.py:453-481: GradientTape
 * over log_loss :404-451, then the optimizer). Replaces the TF autodiff of the dense flow. ---- */

/* Training workspace bytes for B samples: the saved coupling-layer inputs [layers][B][3] and one
 * partial gradient row [num_params] per tile of 16 consecutive samples. 0 for an invalid
 * argument (cnf_last_error says which). */
size_t cnf_toy_train_workspace_bytes(const cnf_toy_desc* d, int B);

/* cnf_toy_call(..., direction -1) that also saves the input of every coupling layer it executes
 * into train_workspace (for cnf_toy_backward on the same xy / zy): zy and per_sample[B*3]
 * (optional, as cnf_toy_call) are bit-identical to cnf_toy_call's. */
int cnf_toy_forward_train(const cnf_toy_desc* d, const float* params, const float* xy, float* zy,
                          float* per_sample /* [B*3], as cnf_toy_call */, void* train_workspace,
                          int B, void* stream);

/* dparams[num_params] = d loss / d params for this shard (fully overwritten), where
 * loss = -(sum_i (llz_i + lly_i + log_detJ_i)) * inv_batch of log_loss (:404-451) and
 * inv_batch = 1 / global batch size, as in cnf_flow_backward: the dparams of data-parallel shards
 * add up to the gradient of the batch-mean loss. d|y - y'| / dy = sign(y - y') (0 at 0). The
 * gradient is taken at the saved activations of cnf_toy_forward_train, not at a re-inverted flow;
 * it is bitwise reproducible run to run, and a sample's contribution does not depend on B. */
int cnf_toy_backward(const cnf_toy_desc* d, const float* params, const float* xy, const float* zy,
                     void* train_workspace, int B, float inv_batch, float* dparams, void* stream);

/* ---- TOYcINN sampling: S draws of x given y for each of B conditions, their mean / std and an
 * optional histogram, in one fused launch. Replaces what the reference's toy driver does once
 * training ends (TOYcINN.py:807-817: z from the prior, concatenate y, model(zy, direction=1);
 * :823-... the cloud per condition), as cnf_flow_sample does for the image flow.
 *
 * Latent: the latent of condition b, draw s, component c < x_d is temperature * element
 * offset + (b*S + s)*x_d + c of the seed's stream, i.e. what
 * cnf_instance_noise(NULL, out, B*S*x_d, 0, seed, offset) writes into a [B,S,x_d] tensor, times
 * temperature in one fp32 multiply; the remaining 3 - x_d components are y[b]. The flow runs in
 * direction +1 (cnf_toy_call's law, u2 = (v2 - b) / exp(tanh A)); the H x H Dense layers run on
 * the fp32 matrix cores, so the draws are cnf_toy_call's up to rounding (the same 1e-5 bound
 * against the float64 model), not its bits. A draw's bits depend on (params, y[b], seed, its stream
 * index, temperature) only: not on B, S, or which draws share its tile of 128.
 *
 * Outputs, each may be NULL but not all: samples [B][S][x_d]; mean, std [B][x_d] over the S draws
 * (population form: divide by S, as np.std); y_dev [B][S] = sum over the 3 - x_d condition
 * components of |y_hat - y|; hist, the counts on a grid (below).
 *
 * Statistics: draw s belongs to tile t = s / 128. Per tile and component the kernel folds, in draw
 * order in fp32, the shifted partial (n_t, K_t, S1_t, S2_t): K_t the tile's first draw,
 * S1_t = sum (v - K_t), S2_t = sum (v - K_t)^2. The partials are merged in tile order in fp64:
 *   o_t = (K_t - K_0) + S1_t / n_t             the tile mean's offset from the first draw
 *   q_t = max(0, S2_t - S1_t * (S1_t / n_t))   its centred second moment, about its own K_t
 *   T = sum_t n_t o_t,  mean = K_0 + T / S
 *   M2 = sum_t (q_t + n_t (o_t - T / S)^2),  std = sqrt(max(0, M2 / S))
 * and rounded once to fp32. No atomics: the results are bitwise reproducible, and a tile's content
 * is fixed by s alone.
 *
 * Histogram (hist_bins = G >= 1): uint32 hist[B][G] (x_d 1) or hist[B][G][G] (x_d 2, component 0
 * major); bin_c = (int)floorf((v_c - hist_lo[c]) * scale_c) with scale_c = (float)G /
 * (hist_hi[c] - hist_lo[c]) computed once in fp32. A draw is counted only if every component is
 * finite and every bin_c lies in [0, G). The call zeroes hist itself on `stream`; counts are
 * integer atomic adds, so they are exact and reproducible. */
typedef struct cnf_toy_sample_desc {
    int      num_samples;          /* S >= 1 draws per condition */
    float    temperature;          /* >= 0, finite */
    uint64_t seed, offset;         /* Philox stream, as cnf_instance_noise */
    int      hist_bins;            /* 0: no histogram */
    float    hist_lo[2], hist_hi[2];
} cnf_toy_sample_desc;

/* Workspace bytes of cnf_toy_sample: the partial slab [B][ceil(S / 128)][x_d] of 16 bytes each,
 * whatever outputs are requested. 0 for an invalid argument (cnf_last_error says which). */
size_t cnf_toy_sample_workspace_bytes(const cnf_toy_desc* d, int B, const cnf_toy_sample_desc* s);

/* CNF_E_INVALID before any HIP call for: NULL y, params or workspace; B < 1 or S < 1; temperature
 * negative or not finite; hist given with hist_bins < 1; hist_lo >= hist_hi or a non-finite edge;
 * hist_bins >= 1 with hist NULL; no output requested; B * S * x_d beyond the index range (B *
 * tiles must stay below 2^31). */
int cnf_toy_sample(const cnf_toy_desc* d, const float* params, const float* y /* [B][3 - x_d] */,
                   const cnf_toy_sample_desc* s, float* samples, float* mean, float* std,
                   float* y_dev, uint32_t* hist, void* workspace, int B, void* stream);

/* ---- TOYcINN density: the flow's exact log-density at N points per condition, for each of B
 * conditions, in one fused launch: on the centres of a grid (the heat map of p(x | y), the curve
 * the counts of cnf_toy_sample's hist converge to) or at given points.
 *
 * Points: with x == NULL, the centres of a grid of grid_bins = G bins per component over
 * [lo[c], hi[c]), N = G^x_d: point p = i0 (x_d 1) or p = i0 * G + i1 (x_d 2, component 0 major, the
 * layout of cnf_toy_sample's hist); component c of it is lo[c] + ((float)i_c + 0.5f) * step_c with
 * step_c = (hi[c] - lo[c]) / (float)G, in fp32, one multiply and then one add, each rounded (no
 * fused multiply-add), so the centres can be recomputed bit for bit; centre i lies in bin i of
 * cnf_toy_sample's histogram over the same box. With x != NULL: x[B][N][x_d], N = num_points. The
 * remaining 3 - x_d components of every point of condition b are y[b].
 *
 * The flow runs in direction -1 (cnf_toy_call's law: reverse layer order, u2 = exp(tanh A) u2 + b,
 * log-det = the sum of tanh A, added layer by layer in execution order, within a layer output 0
 * then output 1); the H x H Dense layers run on the fp32 matrix cores, so the results are
 * cnf_toy_call(..., -1)'s up to rounding (the same bounds against the float64 model), not its bits.
 *
 * Per-point outputs, each may be NULL:
 *   log_prob [B][N] = llz + log-det, llz = -x_d/2 log(2 pi) - 1/2 sum_{c < x_d} z_c^2 (the llz and
 *                     log_detJ of cnf_toy_call's per_sample; what cnf_flow_sample calls log_prob).
 *                     Where the flow returns the condition (y_hat = y, a trained model) the
 *                     Jacobian is block-triangular and this is log p(x | y).
 *   y_dev    [B][N] = sum over the 3 - x_d condition components of |y_hat - y|, as cnf_toy_sample's
 *                     (lly = -lambda_y * y_dev)
 *   z        [B][N][x_d], the latent image of the point
 *
 * log_mass [B] (grid only, may be NULL) = log( sum_p exp(log_prob_p) * prod_c step_c ): the share
 * of the conditional density inside the box (about 0 for a trained model and a box that covers
 * it). Point p belongs to tile t = p / 128. Per tile the kernel folds, in point order in fp32,
 *   m_t = the largest finite log_prob of the tile,  s_t = sum_p expf(log_prob_p - m_t)
 * and the partials are merged in tile order in fp64:
 *   M = max_t m_t,  S = sum_t s_t exp(m_t - M),  log_mass = M + log S + sum_c log step_c
 * rounded once to fp32. A tile without a finite value contributes nothing; a condition without one
 * gives -inf; a NaN log_prob makes log_mass NaN. No atomics.
 *
 * Determinism: the bits of a point's log_prob, y_dev and z depend on (params, y[b], the point's
 * fp32 coordinates) only: not on B, N, which tile or tile row the point sits in, or whether it came
 * from the grid or from x. The bits of log_mass depend on (params, y[b], G, lo, hi) only. Nothing is
 * read that the call did not write: the contents of the workspace and the outputs do not matter. */
typedef struct cnf_toy_density_desc {
    int   num_points;        /* N per condition when x != NULL; ignored for a grid */
    int   grid_bins;         /* G >= 1 when x == NULL; must be 0 when x != NULL */
    float lo[2], hi[2];      /* the grid's box per component, as cnf_toy_sample_desc.hist_lo / hist_hi */
} cnf_toy_density_desc;

/* Workspace bytes of cnf_toy_density: the tile partials [B][ceil(N / 128)] of 8 bytes each, whatever
 * outputs are requested (grid_bins >= 1: N = G^x_d; grid_bins == 0: N = num_points). 0 for an
 * invalid argument (cnf_last_error says which). */
size_t cnf_toy_density_workspace_bytes(const cnf_toy_desc* d, int B, const cnf_toy_density_desc* q);

/* CNF_E_INVALID before any HIP call for: NULL y, params, descriptor or workspace; B < 1; x given
 * with num_points < 1 or grid_bins != 0; x NULL with grid_bins < 1, lo >= hi or a non-finite edge;
 * log_mass with x given; no output requested; B * tiles >= 2^31 or B * N * 3 beyond the index range.
 * No host read and no allocation: the call can be captured into a graph. */
int cnf_toy_density(const cnf_toy_desc* d, const float* params, const float* y /* [B][3 - x_d] */,
                    const float* x, const cnf_toy_density_desc* q, float* log_prob, float* y_dev, float* z,
                    float* log_mass, void* workspace, int B, void* stream);

/* ---- input transforms (the step before the path; conv_cINN_base_functions.py) ----------- */

/* Logit preprocessing of preprocess_dataset_class(LOGITS=True) (:174-231), elementwise over n
 * values in [0, 1]: x -> (logit(a + (1-a) b x) - logit(a)) / (logit(1-a) - logit(a)),
 * b = (1-2a)/(1-a). inverse != 0 applies de_logitify (:287-318) instead. out may alias x. */
int cnf_logit(const float* x, float* out, int64_t n, float a, int inverse, void* stream);

/* Super-resolution preprocessing (preprocess_dataset_SR :233-279 with down/up :74-164):
 * hires [B][H][W][C] -> xy [B][H>>x_down][W>>x_down][2C] with x0 = down^x_down(hires),
 * y = up^y_levels(down^y_levels(x0)) (nested 2x2 means, then 2x2 repeats) and x = x0 - y when
 * residual (RESIDUAL=True), else x0; xy = concat(x, y). 'SR2,1': x_down 0, y_levels 1;
 * 'SR4,2': x_down 1, y_levels 1; the 4x / 8x benchmark configs: y_levels 2 / 3. H and W must be
 * divisible by 2^(x_down + y_levels). */
int cnf_sr_preprocess(const float* hires, float* xy, int B, int H, int W, int C, int x_down, int y_levels,
                      int residual, void* stream);

/* 2x2 average-pool down (:74-125) / 2x2 repeat up (:127-160) of [B][H][W][C]. */
int cnf_down(const float* in, float* out, int B, int H, int W, int C, void* stream);
int cnf_up(const float* in, float* out, int B, int H, int W, int C, void* stream);

/* instance_noise (:635-654): out = alpha x + (1 - alpha) N(0, 1), and renew_noise (:660-676)
 * with x == NULL: out = N(0, 1). Normals from a counter-based generator (Philox4x32-10 +
 * Box-Muller): element i of a call depends only on (seed, offset + i), so results are
 * reproducible and independent of the launch shape. out may alias x. */
int cnf_instance_noise(const float* x, float* out, int64_t n, float alpha, uint64_t seed, uint64_t offset,
                       void* stream);

/* One training batch from a device-resident image cache in one launch (the per-batch half of the
 * reference's input pipeline, conv_cINN.py:209-508: gather, preprocess, label plane, the 2 %
 * baseline noise and the annealing noise). images [N][H][W][C] fp32 in [0, 1]; index_dev [B] picks
 * the batch's images. xy is [B][H][W][C+1] (CLASS) or [B][H>>x_down][W>>x_down][2C] (SR). For flat
 * element e of the whole xy tensor (batch-major NHWC), image b:
 *   v0  CLASS: channels < C: the pixel of images[index[b]], through cnf_logit's forward map if
 *              logit_a; channel C: label_dev[b]
 *       SR:    cnf_sr_preprocess's x and y of images[index[b]] (the same nested 2x2 means, x0 - y
 *              when residual)
 *   v1  = alpha0 v0 + (1 - alpha0) N(0,1) of stream element (seed0, offset0 + e); v0 if alpha0 == 1
 *   v2  = the same with (alpha1, seed1, offset1) on v1;                           v1 if alpha1 == 1
 *   xy[e] = v2
 * Contract: xy equals, bit for bit, this composition of calls on the gathered images:
 * cnf_logit (CLASS, if logit_a) or cnf_sr_preprocess (SR), the label plane concatenated (CLASS),
 * cnf_instance_noise(., n, alpha0, seed0, offset0), cnf_instance_noise(., n, alpha1, seed1,
 * offset1) -- the kernels share their device functions. A stage whose alpha is 1 is skipped, not
 * computed (alpha x + 0 z is x only for a finite z).
 * An index[b] outside [0, N) is never dereferenced: every element of that image is NaN. The guard
 * is in the kernel; the host never reads index_dev or label_dev.
 * CNF_E_INVALID ("cnf_batch_assemble: ..."), before any HIP call: a NULL images, index_dev, desc
 * or xy; B < 1 or N < 1; H, W or C <= 0; an unknown mode; CLASS without label_dev or SR with one;
 * logit_a outside {0} U (0, 0.5), or given in SR mode; SR levels cnf_sr_preprocess refuses; an
 * alpha that is not finite or outside [0, 1]. */
#define CNF_BATCH_CLASS 0
#define CNF_BATCH_SR    1
typedef struct cnf_batch_desc {
    int H, W, C;            /* the cached images [N][H][W][C], fp32 in [0,1] */
    int mode;               /* CNF_BATCH_CLASS | CNF_BATCH_SR */
    float logit_a;          /* CLASS: 0 = raw pixels, else in (0, 0.5): preprocess_dataset_class(LOGITS=True, a) on x */
    int x_down, y_levels, residual;   /* SR: cnf_sr_preprocess's arguments */
    float alpha0; uint64_t seed0, offset0;   /* noise stage 0 (the 2 % baseline); alpha0 == 1: stage off */
    float alpha1; uint64_t seed1, offset1;   /* noise stage 1 (annealing), applied to stage 0's result; 1: off */
} cnf_batch_desc;

int cnf_batch_assemble(const float* images, int64_t N, const int64_t* index_dev /* [B] */,
                       const float* label_dev /* [B]; CLASS only, else NULL */,
                       const cnf_batch_desc* desc, float* xy, int B, void* stream);

/* ---------------------------------------------------------------------------
 * Data-parallel exchange: one process per GPU, the batch
 * sharded over ranks, ONE all-reduce of the NLL sums. Replaces the batch means
 * of the log-det (:1323-1326) and of log_loss (:1840-1848) over a sharded batch.
 * RCCL over xGMI, loaded at run time (CNF_E_STATE when librccl is absent).
 * ------------------------------------------------------------------------- */
#define CNF_COMM_ID_BYTES 128
typedef struct cnf_comm cnf_comm;

/* Rank 0 creates the communicator id and hands it to every rank by any
 * out-of-band means (a file, a key-value store, MPI). */
int cnf_comm_unique_id(char uid[CNF_COMM_ID_BYTES]);
/* Collective over `world` processes; binds the communicator to the calling
 * thread's current HIP device. */
int cnf_comm_init(int rank, int world, const char uid[CNF_COMM_ID_BYTES], cnf_comm** out);
void cnf_comm_destroy(cnf_comm* comm);
/* In-place sum all-reduce of n fp32 device values, asynchronous on stream. */
int cnf_allreduce_sum_f32(cnf_comm* comm, float* buf, size_t n, void* stream);
/* The path's exchange step: red5 (device, 5 floats) = sum over ranks of
 * (sums[0..3] of this rank's cnf_nll, B); red5[k] / red5[4] for k < 4 is the
 * reference's (loss, z_loss, y_loss, detJ_loss) over the global batch. comm may
 * be NULL (one process: no collective, red5 = local sums and B). */
int cnf_nll_allreduce(cnf_comm* comm, const float* sums, int B, float* red5, void* stream);

/* Plan introspection (tests): the canonical parameter index behind every float
 * of the kernel image (which = 0; -1 = zero padding; cnf_pack_params computes
 * aux[i] = params[map[i]]) or of the dense training image (which = 1: every
 * conv as [taps][cin][cout] + bias padded to 4, in layer order). which = 2:
 * the bf16x6 plane region at the end of the kernel image (the streamed convs'
 * weights as k_pw / k_gc keep them in LDS, built unless PRESPLIT=0; which = 0
 * is -1 over it), one entry per 16-bit unit: 4 * parameter + plane (0, 1, 2 =
 * the h, m, l terms of the parameter's exact bf16 split), -1 = zero, <= -2 =
 * the literal value -2 - entry. which = 3: its directory, 16 words per conv
 * (DESIGN.md section 4). Returns the map length; copies min(length, cap)
 * entries when out != NULL. */
int64_t cnf_plan_weight_map(const cnf_plan* plan, int which, int64_t* out, int64_t cap);

/* Measurement hooks (bench.py): number of kernel launches recorded by the last
 * forward/inverse call on this plan, their kernel symbol names, and a re-launch
 * of one recorded launch with identical arguments (same buffers). */
int cnf_plan_num_recorded_launches(const cnf_plan* plan);
int cnf_plan_recorded_launch_info(const cnf_plan* plan, int i, char* name, int name_cap,
                                  double* flops, double* bytes);
int cnf_plan_relaunch(cnf_plan* plan, int i, void* stream);
/* In-stream launch timing: while on, every kernel of a forward/inverse call is
 * dispatched with hipExtLaunchKernelGGL start/stop events, which receive the
 * kernel's own begin/end timestamps (eager calls only, not inside graph
 * capture); cnf_plan_launch_time_ms then gives launch i's GPU duration in its
 * place in the sequence (waits for it; 0 for a launch that is not a kernel). */
int cnf_plan_set_launch_timing(cnf_plan* plan, int on);
int cnf_plan_launch_time_ms(const cnf_plan* plan, int i, float* ms);

const char* cnf_last_error(void);
const char* cnf_version(void);

#ifdef __cplusplus
}
#endif
#endif /* CNF_H_ */
