/*
 * nst_hip.h - C ABI of libnst_hip.so, the MI355X (gfx950) implementation of the pyramid
 * neural-style-transfer hot path.
 *
 * The reference (irenemizus/ArtStyleTransfer) has no FFI of its own: its hot path is Python on top
 * of torch ops.  Each entry point below names the reference interface it replaces
 * (file:line in the reference checkout; "torch:" = the torch package the reference calls into).
 *
 * Conventions
 *   - every function returns 0 on success, a negative NST_E_* code on failure, never throws;
 *     nst_last_error(ctx) returns a description of the last failure on that context
 *     (nst_last_error(NULL): the last failure of a call that had no context, thread-local).
 *   - the caller owns every image / gradient / optimiser buffer and passes raw DEVICE pointers
 *     plus the hipStream_t (as void*) the work must be ordered on; the context owns the VGG
 *     weights (pre-transformed), the per-level targets and the activation workspace.
 *   - images on the device are fp32 planar (3, H, W) in the reference's "prepared" domain
 *     (RGB * 255 - ImageNet mean: neural_style_transfer.py:375-383), exactly the storage of the
 *     (1,3,H,W) torch tensor the reference optimises.
 *   - every entry point binds the context's device itself (callers hop between thread-pool
 *     threads: neural_style_transfer.py:206) and is re-entrant across contexts.
 */
#ifndef NST_HIP_H
#define NST_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NST_OK 0
#define NST_E_ARG (-1)      /* bad argument (null pointer, bad size, unknown enum) */
#define NST_E_STATE (-2)    /* call order violated (e.g. closure before targets) */
#define NST_E_HIP (-3)      /* a HIP runtime call failed; see nst_last_error */
#define NST_E_NOMEM (-4)
#define NST_E_UNAVAILABLE (-5) /* this entry point does not run under the context's schedule; nothing was launched, use the
                                  entry point named in nst_last_error instead */

#define NST_VGG19_CONVS 13  /* conv1_1 ... conv5_1 (torchvision features[0:30]) */
#define NST_MAX_LEVELS 8    /* jobs of 4 .. 7 levels are held to the CPU oracle whole, the 8-level job in pieces: tests/test_hip_deep_pyramids.py */
#define NST_LOSS_ROW 4      /* per level: total, content, style, tv */
#define NST_MAX_STYLES 8    /* style images one level's targets may blend (nst_level_set_targets_blend) */
#define NST_MAX_REGIONS 4   /* regions of spatial control (nst_level_set_guidance) */
#define NST_MAX_LAPLACIAN 4 /* entries (pool size, weight) of the Laplacian loss (nst_job_set_laplacian) */
#define NST_MAX_FLOW_SCALES 12 /* pyramid scales of the flow estimator (nst_flow_estimate) */

typedef struct nst_ctx nst_ctx;
typedef struct nst_opt nst_opt;
typedef struct nst_comm nst_comm;

/* library / device ------------------------------------------------------------------------ */
int nst_version(void);
const char* nst_last_error(const nst_ctx* ctx);
/* number of visible HIP devices (does not initialise a context on any of them) */
int nst_device_count(int* count);

/* context: VGG19 feature network of math_utils.prepare_model (math_utils.py:9-23) and
 * neural_nets.Vgg19.__init__ (neural_nets.py:17-51).  weights[i]: HOST pointer, (Cout,Cin,3,3)
 * fp32 in torchvision order conv1_1..conv5_1; biases[i]: HOST pointer (Cout).  The context
 * keeps device copies re-laid-out for the forward and the input-gradient kernels. */
int nst_ctx_create(int device, const float* const* weights, const float* const* biases, nst_ctx** out);
void nst_ctx_destroy(nst_ctx* ctx);

/* The same with the execution options as ARGUMENTS (nst_ctx_create = nst_ctx_create_ex with opts == NULL).  A field
 * left at -1 takes the environment variable named beside it, read ONCE here, and otherwise the stated default; the
 * environment is never consulted again during the life of the context.  There is no counterpart in the reference
 * (torch picks its kernels by itself); the options exist for the parity tests, which hold the alternative
 * arithmetic / schedules against the default one. */
#define NST_CONV_F32 0      /* fp32 MFMA (v_mfma_f32_32x32x2_f32): the reference's arithmetic type, exactly */
#define NST_CONV_BF16X3 1   /* bf16 matrix pipe, three bf16 pieces that sum to the fp32 value exactly, 6 MFMAs */
#define NST_CONV_F16X2 2    /* fp16 matrix pipe, two scaled fp16 pieces per operand, 3 MFMAs per product block (default) */
typedef struct nst_options {
    int struct_size;      /* sizeof(nst_options), filled by nst_options_default */
    int conv_mode;        /* NST_CONV_*; -1: env NST_CONV (f32 | bf16x3 | f16x2), default f16x2 */
    int batched;          /* 1: one conv launch per layer covering every pyramid level; 0: per level; -1: env NST_BATCH, default 1 */
    int single_stream;    /* per-level schedule only - 1: all levels on the caller's stream; -1: env NST_SINGLE_STREAM, default 0 */
    int use_graph;        /* 1: replay the closure as a hipGraph; -1: env NST_GRAPH, default 0 */
    int h2_band_rows;     /* >= 16: run the f16x2 per-level launches in row bands of that many rows (the path tensors beyond
                             4 GiB take, forced onto small images); -1: env NST_H2_BAND_ROWS, default 0 = only when needed */
    int lbfgs_gram;       /* 1: L-BFGS direction from inner products (two passes over the history); 0: the sequential
                             recursion; -1: env NST_LBFGS_GRAM, default 1 */
    int h2_mfma16;        /* f16x2 convolutions with 32-channel chunks: v_mfma_f32_16x16x32_f16 instead of v_mfma_f32_32x32x16_f16
                             (same products, same accumulation chains per output; the chip clocks higher under it): 0 = never,
                             1 = on the 8-row x 128-channel shape (under-filled launches: +6 ... 11 % per launch),
                             2 = also on the 16-row shape where the launch does not un-pool (no gain measured), 3 = on every
                             32-channel-chunk shape (slower; both kept for experiments);
                             -1: env NST_H2_MFMA16, default 1 */
    int h2_wg256;         /* f16x2 convolutions, the 16x16-pixel x 128-channel tile: 1 = 256-thread workgroups, one wave per SIMD
                             with a 64 x 128 wave tile (accumulators in AGPRs), 0 = 512 threads with 64 x 64 wave tiles;
                             -1: env NST_H2_WG256, default 0 */
    int h2_tile_rows;     /* f16x2 direct convolutions (conv_h2.hip) with 128-channel tiles and 32-channel chunks - Cout a multiple
                             of 128 and Cin > 128, or the Gram source alone; batched and per-level launches alike: 4 / 8 / 16 =
                             pixel rows per workgroup tile, 0 = chosen per launch from the number of workgroups.  The short-K
                             launches (Cin <= 128), the 64-channel layers and the Winograd launches keep their own shape: with
                             h2_winograd = 1 the option reaches the launches that carry a Gram source only.
                             -1: env NST_H2_TILE_ROWS, default 0 */
    int gram_overlap;     /* f16x2 closure: 1 = the Gram matrices of relu1_1 ... relu3_1 (HBM-bound) run on a side stream of the
                             context under the MFMA-bound convolutions of conv3_2 ... conv5_1, joined before the backward pass;
                             0 = everything in order on the caller's stream; -1: env NST_GRAM_OVERLAP, default 0 (measured: no gain) */
    int h2_persist;       /* f16x2 batched launches: 1 = persistent workgroups (one grid that fills the chip once, each workgroup
                             walks its share of the tiles with the K pipeline chained from one tile into the next);
                             0 = one workgroup per tile; -1: env NST_H2_PERSIST, default 0 (measured: the chained form's extra scalar state
                             costs more than the hidden prologues gain) */
    int level_split;      /* f16x2 batched closure: 1 = the top pyramid level's chain on the caller's stream and the lower levels'
                             chain on a side stream of the context, joined before the gradients are merged; 0 = one launch per
                             layer over all levels; -1: env NST_LEVEL_SPLIT, default 0.  The context has ONE side
                             stream: level_split = 1 switches gram_overlap off, whatever that field or NST_GRAM_OVERLAP says */
    int h2_winograd;      /* f16x2 batched closure: 1 = the forward and input-gradient launches with Cin >= 256 and Cout a
                             multiple of 128 that have no second (Gram) source - 15 of the 24 of a closure - run as a 1-D Winograd
                             F(2,3) along x (conv_wino.hip: 1.5x fewer MFMAs there; the feature maps are no further from an fp64
                             evaluation than the direct path's); 0 = direct convolution everywhere;
                             -1: env NST_H2_WINOGRAD, default 1 */
} nst_options;
void nst_options_default(nst_options* opts);
int nst_ctx_create_ex(int device, const float* const* weights, const float* const* biases, const nst_options* opts,
                      nst_ctx** out);

/* pyramid geometry of one job: levels_num levels, level 0 = (H0, W0), level l = previous // 2
 * (neural_style_transfer.py:170-176).  Allocates the activation workspace of every level. */
int nst_job_configure(nst_ctx* ctx, int levels_num, int H0, int W0);

/* The feature maps the losses read: LossBuilder(content_feature_maps_index, style_feature_maps_indices, ...) and
 * Vgg19(use_relu=...) (neural_style_transfer.py:41-82, neural_nets.py:17-28) as a setting of the context.  Indices are
 * those of Vgg19.layer_names: 0..5 = relu1_1, relu2_1, relu3_1, relu4_1, conv4_2, relu5_1.
 *   content_index: 0..5;  style_mask: non-empty set of bits 0..5 (bit i = map i; order and repeats of the reference's
 *   list do not matter, the style term is the mean over the maps in the set);  use_relu: 1, or 0 = the reference's
 *   use_relu=False - map 5 is then conv5_1 BEFORE its ReLU (torchvision's in-place ReLUs leave maps 0..4 post-ReLU).
 * NST_E_ARG for anything else.  A new context has the reference's taps: (4, 0x2F, 1).  The forward of a closure stops at
 * the deepest map in use, its backward starts there.  Setting taps (even the same ones) waits for the context's work,
 * re-sizes the target buffers of every configured level and drops their targets (a closure returns NST_E_STATE until
 * nst_level_set_targets has run again) and any captured closure graph.  nst_vgg_features / nst_vgg_activations return
 * conv5_1 before its ReLU under use_relu = 0.  The stripe closure (nst_window_*) implements the default taps only and
 * returns NST_E_STATE under any other.  The full range is held to the CPU oracle: single maps and pairs in
 * tests/test_hip_taps.py, all six style maps (style_mask 0x3F, also with a content map below the top of the chain and with
 * unequal nst_job_set_style_weights) in tests/test_hip_deep_pyramids.py. */
int nst_job_set_taps(nst_ctx* ctx, int content_index, unsigned style_mask, int use_relu);

/* Colour preservation, luminance-only transfer (Gatys, Bethge, Hertzmann & Shechtman, "Preserving Color in Neural
 * Artistic Style Transfer", 2016): the channel count of the optimised image, a setting of the context like the taps.
 *   NST_COLOR_RGB (a new context's): images are prepared RGB (3,h,w).
 *   NST_COLOR_LUMINANCE: the optimised image is ONE plane u = 255 Y (1,H0,W0) that the network sees as the prepared
 *     image E(u)_c = u - mean_c (mean = IMAGENET_MEAN_255).  The loss is the RGB closure at E(u) (the bicubic 1/2 chain of
 *     u, then E, per level; TV taken on u, which equals TV(E(u))), the gradient is the sum over c of d loss / d x_c.
 *     nst_level_set_targets takes (1,h,w) / (1,hs,ws) prepared luminance images, nst_closure(_levels) a (1,H0,W0) x and
 *     grad, nst_level_image writes (1,h_l,w_l); nst_opt_create sizes its vectors by the channel count, and a step of an
 *     optimiser created under the other mode returns NST_E_STATE.  The stripe closure (nst_window_*) returns
 *     NST_E_STATE; nst_vgg_features* stay RGB.
 * Setting the mode (even the same one) waits for the context's work, re-sizes the level image buffers and drops every
 * level's targets and any captured closure graph.  It composes with any taps, every conv mode and schedule.
 * nst_job_color returns the current mode. */
#define NST_COLOR_RGB 0
#define NST_COLOR_LUMINANCE 1
int nst_job_set_color(nst_ctx* ctx, int mode);
int nst_job_color(const nst_ctx* ctx);

/* Pooling of the VGG19 feature network (Gatys, Ecker & Bethge, "Image Style Transfer Using Convolutional Neural
 * Networks", 2016, section 2: average pooling gives smoother gradients than max pooling), a setting of the context like
 * the taps and the colour mode.
 *   NST_POOL_MAX (a new context's): the four 2x2/2 max-pools of torchvision's vgg19.
 *   NST_POOL_AVG: each of them is a 2x2/2 average pool.  Definition, the same in every arithmetic mode and schedule:
 *     - sizes floor (h // 2, w // 2): a last odd row / column belongs to no window and receives no gradient, as with max;
 *     - pooled value = ((e00 + e01) + e10) + e11, then * 0.25f, in fp32, where e_yx is the post-ReLU activation at
 *       window row y, column x (the scan order of the window, added left to right).  EVERY kernel that pools uses
 *       this order, so the modes and schedules differ by the rounding of their convolutions only;
 *     - backward: each of the four positions gets 1/4 of the pooled map's gradient, then the ReLU mask of the pooled
 *       activation (a position whose unit is off gets none).  In the fused f16x2 path the code words of a window are
 *       multi-hot (bit of position q = e_q > 0) and the 1/4, a power of two, rides exactly on the scale the un-pooling
 *       input-gradient launch multiplies its accumulators by.
 * NST_E_ARG for any other value.  Setting the mode (even the same one) waits for the context's work and drops every
 * level's targets (a closure returns NST_E_STATE until nst_level_set_targets has run again: they were made with the
 * other network) and any captured closure graph.  It composes with any taps, NST_COLOR_LUMINANCE, every conv mode and
 * schedule, and level sharding.  nst_vgg_features / nst_vgg_activations / nst_vgg_features_backward follow it.  The
 * stripe closure (nst_window_*) implements max pooling only and returns NST_E_STATE under NST_POOL_AVG.
 * nst_job_pooling returns the current mode. */
#define NST_POOL_MAX 0
#define NST_POOL_AVG 1
int nst_job_set_pooling(nst_ctx* ctx, int mode);
int nst_job_pooling(const nst_ctx* ctx);

/* Per-layer style weights (the w_l of Gatys, Ecker & Bethge 2016, eq. 5), a setting of the context.  w[i]: the weight of
 * map i of Vgg19.layer_names (0..5), finite and >= 0; at least one map of the current style set (nst_job_set_taps) has
 * w > 0; NST_E_ARG for anything else (the weights then stay as they were).  With them
 *   style term of a level = (sum_i w_i MSE(G_i, Gt_i)) / nstyle, over the maps of the style set in ascending order,
 *   backward of map i: S_i = coef_i (G_i - Gt_i), coef_i = (float)((double)style_weight (double)w_i 4 / (nstyle C^2 C h w)).
 * A new context has w = 1 everywhere, which multiplies exactly: there is one code path, and under w = 1 every loss row and
 * gradient is bitwise what it is without the setting.  A map of the set with w_i = 0 is still evaluated and contributes
 * zero.  The weights belong to map indices, not to positions in the style set: they survive nst_job_set_taps, which
 * returns NST_E_ARG (and changes nothing) when no map of its style_mask has a positive weight.
 * Setting the weights (even the same ones, and when the call fails) waits for the context's work, drops any captured
 * closure graph and ends the validity of an optimiser's remembered closure (nst_opt_set_closure_reuse) and of a pending
 * nst_closure_backward.  It does NOT drop the targets: they do not depend on the weights.  It composes with any taps,
 * colour mode, pooling, conv mode and schedule, and with level sharding (targets are per level, weights per context).
 * The stripe closure (nst_window_*) implements w = 1 only and returns NST_E_STATE under any other weights.
 * nst_job_style_weights writes the current weights to w. */
int nst_job_set_style_weights(nst_ctx* ctx, const float w[6]);
int nst_job_style_weights(const nst_ctx* ctx, float w[6]);

/* Laplacian loss (Li, Xu, Nikolova & He, "Laplacian-Steered Neural Style Transfer", ACM MM 2017): a pixel-space term that
 * keeps the content's edges, a setting of the context.  The reference has no counterpart.
 *
 * Entries
 * - A job has up to NST_MAX_LAPLACIAN entries (p_k, gamma_k).
 * - The pool size p_k is an integer in 1..32; the entries have distinct pool sizes.
 * - The weight gamma_k is finite and >= 0, and at least one is > 0.
 * Term of a level image y, prepared, (3,h,w), and entry k
 * - s_k(y) = sum_c P_p(y_c), P_p a p x p mean pool with stride p.
 *   - Sizes floor: hk = h / p, wk = w / p.  Ragged last rows and columns belong to no cell and get no gradient.
 *   - The cell sum is accumulated in double (exactly: at most 3 x 32 x 32 fp32 values) and s_k stays in double: with prepared
 *     values near +-120 an fp32 s_k loses the digits that the stencil then needs.
 * - D is the valid (unpadded) 3x3 stencil [[0,-1,0],[-1,4,-1],[0,-1,0]]; its output is (hk-2, wk-2).  Unpadded, so the
 *   constant ImageNet means cancel.
 * - Residual r_k = (float)(D s_k(y) - D s_k(content_l)), both stencils in double, rounded once.
 * - lap_k = (float)(sum r_k^2 / n_k), n_k = (hk-2)(wk-2), the sum in double in a fixed two-stage order.
 * - lap = sum_k gamma_k lap_k, in float in ascending k, each product and each sum rounded.
 * Loss row
 * - With K > 0 the level total is ((cw content + sw style) + tvw tv) + lap.  With K = 0 it is the expression without the term.
 * - NST_LOSS_ROW stays 4 and entries 1..3 keep their meaning: the gamma_k carry the term's weight, and nst_closure* /
 *   nst_opt_step keep their signatures.  nst_job_laplacian_losses returns the lap_k.
 * Gradient
 * - d/dy_c(i,j) = coef_k (D^T r_k)(i / p, j / p) for i < hk p, j < wk p.
 * - coef_k = (float)((double)gamma_k 2 / (n_k p^2)).
 * - D^T is the full correlation of r_k with the symmetric stencil, zero outside r_k.
 * - It is accumulated into the level gradient after the total-variation gradient, in ascending k.
 * Luminance
 * - Under NST_COLOR_LUMINANCE the term is that of the RGB closure at E(u): s_k = 3 P_p(u), and the gradient with respect
 *   to u is the sum over the three channels.
 * No float atomics: a closure with the term is bitwise reproducible, as closure reuse and the lazy backward need.
 *
 * nst_job_set_laplacian: K = 0 switches the term off (pool and gamma are ignored).  Needs a configured job (NST_E_STATE
 * otherwise).  NST_E_ARG, with nothing changed, for a bad K, pool size or gamma, duplicate pool sizes, no positive gamma, or
 * when any level has h_l / p < 3 or w_l / p < 3.  Life cycle of nst_job_set_pooling: the call waits for the context's work,
 * drops every level's targets (the Laplacian targets D s_k(content) are made with them: nst_level_set_targets,
 * nst_level_set_targets_blend and nst_level_set_targets_guided make them from the `content` they are given) and any captured
 * closure graph, and ends the validity of an optimiser's remembered closure and of a pending nst_closure_backward.  Every
 * buffer of the term is allocated here, never in a closure.  nst_job_configure clears the setting.  It composes with any
 * taps, colour mode, pooling, style layer weights, blends, guidance, every conv mode and schedule (use_graph included), the
 * closure halves and level sharding (rows and gradients add up).  The stripe closure (nst_window_*) returns NST_E_STATE
 * while K > 0.
 * nst_job_laplacian: the current setting (any pointer may be NULL; unused entries are zeros).
 * nst_job_laplacian_losses: the unweighted lap_k of the last closure per level and entry, to out (DEVICE, levels x
 * NST_MAX_LAPLACIAN floats); levels outside the last level mask and unused entries are zeros.  Asynchronous on `stream`. */
int nst_job_set_laplacian(nst_ctx* ctx, int K, const int* pool, const float* gamma);
int nst_job_laplacian(const nst_ctx* ctx, int* K, int pool[NST_MAX_LAPLACIAN], float gamma[NST_MAX_LAPLACIAN]);
int nst_job_laplacian_losses(nst_ctx* ctx, float* out /* device, levels x NST_MAX_LAPLACIAN */, void* stream);

/* Matting term: the photorealism regulariser of Luan, Paris, Shechtman & Bala ("Deep Photo Style Transfer", CVPR 2017), the
 * quadratic form of Levin's matting Laplacian.  It penalises an output that is not, in every 3x3 window, an affine function
 * of the content's colours.  A pixel-space term, a setting of the context.  The reference has no counterpart.
 *
 * Setting
 * - A weight gamma, finite and >= 0 (0 = off), and epsilon, finite and > 0 (Luan's value is 1e-7).
 * Term of a level image y, prepared, (3,h,w), with the guide I = (content_l + IMAGENET_MEAN_255) / 255
 * - content_l is the level's content as given to nst_level_set_targets*; the context keeps a device copy per level, made
 *   where the Laplacian targets are made.  Only differences inside a window enter, so the means cancel.
 * - Windows: every 3x3 window k that lies fully inside the image, (h-2)(w-2) of them; n = 3 (h-2)(w-2).  Its nine pixels i:
 *   mu_k = mean_i I_i, Ic_i = I_i - mu_k, M_k = (1/9) sum_i Ic_i Ic_i^T + (epsilon/9) Id_3.
 * - Per output channel c, V = y_c / 255: Vc_i = V_i - mean_i V_i (the centred form: the ImageNet means cancel exactly),
 *   v = sum_i Vc_i Ic_i, a = M_k^{-1} v / 9, E_kc = sum_i Vc_i^2 - v^T a
 *   (= sum_i (Vc_i - a^T Ic_i)^2 + epsilon |a|^2 in exact arithmetic).
 * - mat = (float)((1/n) sum_k sum_c E_kc) = (1/n) sum_c V_c^T L V_c with Levin's matrix L.
 * - Per window the moments, v, the solve (an LDL^T factorisation of M_k; no inverse is stored) and E are formed in double
 *   from the fp32 images; the sum is in double in a fixed two-stage order (tiles of 32 x 8 windows, then the tile partials).
 *   M_k is singular up to epsilon/9 wherever the content's colours lie on a line or are constant.
 * Loss row
 * - With gamma > 0 the level total is (((cw content + sw style) + tvw tv) + lap) + gamma mat: added last, product and sum
 *   each rounded (the lap term only when it is set).  NST_LOSS_ROW stays 4.  nst_job_matting_losses returns the mat.
 * Gradient
 * - d/dy_c(i) = coef sum_{k containing i} (Vc_i^(k) - a_kc^T Ic_i^(k)), coef = (float)((double)gamma 2 / (255 n)); the sum
 *   over the (up to nine) windows in double in a fixed order, rounded once.  Border pixels lie in fewer windows.
 * - It is accumulated into the level gradient after the total-variation and the Laplacian gradients.
 * Luminance
 * - Under NST_COLOR_LUMINANCE the term is that of the RGB closure at E(u) with a guide whose three channels all equal
 *   content_u / 255, and the gradient with respect to u is the sum over the three channels.  That is the scalar form
 *   b = sum_i Vc_i gc_i / (sum_i gc_i^2 + epsilon/3), E_k = sum_i Vc_i^2 - b sum_i Vc_i gc_i, mat = sum_k E_k / ((h-2)(w-2)),
 *   which is what runs.
 * No float atomics: a closure with the term is bitwise reproducible, as closure reuse and the lazy backward need.
 *
 * nst_job_set_matting: needs a configured job (NST_E_STATE otherwise).  NST_E_ARG, with nothing changed, for a non-finite
 * or negative gamma or a non-finite or non-positive epsilon.  Life cycle of nst_job_set_laplacian: the call waits for the
 * context's work, drops every level's targets (the guide is made with them) and any captured closure graph, and ends the
 * validity of an optimiser's remembered closure and of a pending nst_closure_backward.  Every buffer of the term is
 * allocated here, never in a closure.  nst_job_configure clears the setting.  With gamma = 0 a closure launches what it
 * launches without the call and computes the same bits.  It composes with any taps, colour mode, pooling, style layer
 * weights, blends, guidance, the Laplacian loss, the Gram shift, every conv mode and schedule (use_graph included), the
 * closure halves and level sharding (rows and gradients add up).  The stripe closure (nst_window_*) returns NST_E_STATE
 * while gamma > 0.
 * nst_job_matting: the current setting (either pointer may be NULL).
 * nst_job_matting_losses: the unweighted mat of the last closure per level, to out (DEVICE, levels floats); levels outside
 * the last level mask are zeros.  Asynchronous on `stream`. */
int nst_job_set_matting(nst_ctx* ctx, float gamma, double epsilon);
int nst_job_matting(const nst_ctx* ctx, float* gamma, double* epsilon);
int nst_job_matting_losses(nst_ctx* ctx, float* out /* device, levels */, void* stream);

/* Gram shift: activation-shifted and mean-centred style statistics, a setting of the context.  The reference has no
 * counterpart: its statistic is the raw second moment G = F^T F / (C N) of the tapped maps.
 * - Activation shift (Novak & Nikulin, "Improving the Neural Algorithm of Artistic Style", 2016): G = (F + s)^T (F + s), s = -1
 *   in the paper.  Post-ReLU maps are sparse, and a raw Gram entry cannot tell "both channels off" from "one off".
 * - Mean-centred Gram, the covariance (Li, Wang, Liu & Hou, "Demystifying Neural Style Transfer", 2017; WCT-style methods).
 *
 * Setting
 * - Each of the six maps of Vgg19.layer_names has a setting, by map index as the style layer weights: a finite float s_i
 *   (0 = the plain Gram), or *centred* (bit i of center_mask; shift[i] must then be 0).
 * Statistic of a style map of C channels and N pixels
 * - o_c = s_i for a shifted map.
 * - o_c = -(1/N) sum_p F_pc for a centred map, the sum in double in a fixed two-stage order, rounded to fp32 once.  The style
 *   TARGET uses the style image's own means; the closure uses those of the image being optimised.
 * - G = sum_p (F_p + o)(F_p + o)^T / (C N), summed directly: on post-ReLU maps the covariance is a small difference of large
 *   second moments, so the correction form G - N mu mu^T would lose digits.  The pixels that pad a ragged last group of a
 *   split contribute 0, not o.
 * - The style term, layer weights, nstyle division and coefficients stay what they are for the plain Gram.
 * - Blended targets (nst_level_set_targets_blend) are the weighted mean of each style's G, each with its own means.
 * Gradient
 * - dF_p = (F_p + o) S = F_p S + r with S = coef (G - Gt) and r = o S, one C-vector per map: the launches that carry F S as
 *   their second K source add r in their epilogue, after the scale and before the addend and the ReLU mask.
 * - Under centring the dependence of the means on F drops out exactly, because sum_p (F_p + o) = 0.
 * - Pre-ReLU taps (use_relu = 0): the style gradient, r included, joins unmasked where the Gram term joins.
 * Operand bound
 * - The fp16-piece Gram kernels scale by a power of two from a bound of their operand.  F's own absmax does not bound F + o,
 *   so the offsets kernel records absmax(F) + max_c |o_c|, rounded up.
 * No float atomics: a closure with the option is bitwise reproducible.
 *
 * nst_job_set_gram_shift: all zeros with an empty mask switches the option off: the job then launches what it launches
 * without the call and computes the same bits.  NST_E_ARG, with nothing changed, for a non-finite shift, mask bits above
 * 5, or a non-zero shift of a centred map.  A non-trivial setting needs a configured job and the f16x2 arithmetic, and no
 * guided level (NST_E_STATE otherwise).  Life cycle of nst_job_set_pooling: the call waits for the context's work, drops
 * every level's targets (they are made with the statistic) and any captured closure graph, and ends the validity of an
 * optimiser's remembered closure and of a pending nst_closure_backward.  Every buffer of the option is allocated here,
 * never in a closure.  nst_job_configure clears the setting.  The work belongs to the forward half of the closure.  It
 * composes with any taps, colour mode, pooling, style layer weights, blends, the Laplacian loss, the closure halves, level
 * sharding and every f16x2 schedule - batched and per level (single_stream and h2_band_rows included), use_graph,
 * gram_overlap (its offset and row-bias launches ride with the Gram batch of their maps, on either stream), level_split,
 * h2_persist, keep_all_maps, forward_pack = 0, gram_pack = 0 - with the bits of the default schedule (level_split: of the two
 * masked closures its chains are); tests/test_hip_schedule_matrix.py holds each.  While it is non-trivial, nst_level_set_guidance (R > 0),
 * nst_level_set_targets_guided and nst_window_* return NST_E_STATE.
 * nst_job_gram_shift: the current setting (either pointer may be NULL).
 * nst_level_gram_offsets: the o that the level's last closure used for style slot `slot` (ascending map order of the
 * current taps), C floats to out (DEVICE); zeros before the first closure.  NST_E_STATE without a non-trivial setting.
 * nst_gram_shifted: the statistic alone, beside nst_gram: f device (C,h,w), C = 64 or a multiple of 128 up to 1024;
 * center != 0: centred (shift must be 0); gram device (C,C); offset_out (nullable): device, C floats, the o used.  shift = 0
 * without centring is nst_gram, bitwise.  f16x2 arithmetic only.  Synchronous on `stream`, as nst_gram. */
int nst_job_set_gram_shift(nst_ctx* ctx, const float shift[6], unsigned center_mask);
int nst_job_gram_shift(const nst_ctx* ctx, float shift[6], unsigned* center_mask);
int nst_level_gram_offsets(nst_ctx* ctx, int level, int slot, float* out, void* stream);
int nst_gram_shifted(nst_ctx* ctx, const float* f, int C, int h, int w, int normalize, int center, float shift, float* gram,
                     float* offset_out /* nullable, C floats */, void* stream);

/* nst_gram_batch: the closure's own Gram launch on the caller's maps - what a closure does with the style maps of its
 * pyramid levels, as a stand-alone call.  n items, 1 <= n <= NST_GRAM_BATCH_MAX; per item the planar map is made
 * pixel-major and its absmax recorded (as nst_gram does), then ONE batched launch under the context's gram_pack setting:
 * the partial products of every item - both tile shapes in one grid when packed, a smaller map of a channel count with
 * fewer splits than a lone map of its size gets - and one finish pass.  Per item:
 *   f        device (C,h,w); C = 64 or a multiple of 128
 *   guide    nullable, for ALL items or for none: device h w floats in [0,1], the guided Gram sum_p t(p)^2 F(p) F(p)^T
 *   target   nullable: device (C,C); with it the finish pass makes S = coef (G - target), one subtraction and one
 *            multiplication in fp32, the sum of (G - target)^2 in double and the absmax of S
 *   gram     device (C,C), required: G = (sum of the slabs) / (C h w), or the bare sum with normalize = 0
 *   S        nullable, device (C,C);  S_bf nullable, device 3 C C 16-bit words: S cut into three bf16 pieces (the truncated
 *            high 16 bits, then those of each remainder) at [row][col / 32][piece][col % 32]
 *   outputs on the HOST, written before the call returns: mse (the finish blocks' partial sums added in block order; 0
 *   without a target), S_absmax (the maximum of the record's words; 0 without a target), nsplit and pix_per_split (the
 *   geometry the launcher used: splits = slabs, pixels of one split).
 * NST_E_STATE outside the f16x2 arithmetic (the batch has no other form).  NST_E_ARG: n out of range, a null f or gram,
 * a C other than 64 or a multiple of 128, guided and unguided items mixed, S or S_bf without a target.  Reads no job
 * state; every buffer it needs is scratch of the call.  Synchronous on `stream`, as nst_gram. */
#ifndef NST_GRAM_BATCH_MAX
#define NST_GRAM_BATCH_MAX 16
#endif
typedef struct nst_gram_batch_item {
    const float* f;
    int C, h, w;
    const float* guide;
    const float* target;
    float coef;
    float* gram;
    float* S;
    unsigned short* S_bf;
    double mse;
    float S_absmax;
    int nsplit;
    long long pix_per_split;
} nst_gram_batch_item;
int nst_gram_batch(nst_ctx* ctx, nst_gram_batch_item* items, int n, int normalize, void* stream);

/* Moment loss: the channel means and standard deviations of the style maps matched to the style's, a setting of the
 * context.  The reference has no counterpart.  It is the "BN statistics matching" of Li, Wang, Liu & Hou, "Demystifying
 * Neural Style Transfer" (2017), and the style loss of Huang & Belongie, "Arbitrary Style Transfer in Real-time with
 * Adaptive Instance Normalization" (2017): sum_i |mu(F_i) - mu(F_i^style)|^2 + |sigma(F_i) - sigma(F_i^style)|^2.  Beside a
 * centred Gram (nst_job_set_gram_shift) it restores the first moment that centring removes from the statistic.
 *
 * Setting
 * - Each of the six maps of Vgg19.layer_names has two weights, by map index as the style layer weights: wm_i of its mean
 *   term and ws_i of its deviation term, finite and >= 0; and one epsilon > 0 (default 1e-5) for all maps.
 * Statistic of map i, C channels and N pixels, the sums in double in a fixed two-stage order
 * - mu_c = (1/N) sum_p F[p][c]
 * - var_c = (1/N) sum_p F[p][c]^2 - mu_c^2, clamped at 0 (one pass: in double the cancellation error is about 1e-13 E[F^2],
 *   against epsilon = 1e-5)
 * - sigma_c = sqrt(var_c + epsilon)
 * - mean_i = (1/C) sum_c (mu_c - mu^t_c)^2,  std_i = (1/C) sum_c (sigma_c - sigma^t_c)^2, in double, rounded to fp32 once
 * - The targets mu^t, sigma^t are the same statistics of the style level's map, rounded to fp32, taken when the targets are
 *   set.  Under nst_level_set_targets_blend they are the weighted mean of each style's moments with the b^ of the map's
 *   Gram target, accumulated in fp32 in ascending k as the Gram targets are.
 * Loss row
 * - The level total gains mom = sum_i (wm_i mean_i + ws_i std_i) over the style maps with a positive weight, in ascending
 *   map order, every product and sum rounded: ((((cw content + sw style) + tvw tv) + lap) + gamma mat) + mom, the lap and
 *   mat terms only when they are set.  The weights are the term's own: sw does not scale it.  NST_LOSS_ROW stays 4 and
 *   entries 1..3 keep their meaning.  nst_job_moment_losses returns the unweighted values.
 * Gradient
 * - dF[p][c] = b_c F[p][c] + (a_c - b_c mu_c) with a_c = wm_i 2 (mu_c - mu^t_c) / (C N) and
 *   b_c = ws_i 2 (sigma_c - sigma^t_c) / (C N sigma_c).  A channel with var_c = 0 has sigma_c = sqrt(epsilon) and a finite b_c.
 * - The launches that carry the Gram backward F S + r take it as S += diag(b), r += a - b o mu, after the Gram finish pass
 *   and after r = o S of a shifted Gram (which sees S without the diagonal).  b_c enters the bias as the rounded diagonal
 *   holds it (new entry minus old entry), so F S + r is a_c + b_c (F - mu_c) with one b_c.  The absmax record of S is raised
 *   to the diagonal.  A map whose style layer weight is 0 has S = diag(b).
 * No float atomics: a closure with the term is bitwise reproducible, as closure reuse and the lazy backward need.
 *
 * nst_job_set_moments: all-zero weights switch the term off: the job then launches what it launches without the call and
 * computes the same bits.  NST_E_ARG, with nothing changed, for a negative or non-finite weight, a non-finite or
 * non-positive epsilon, or a positive weight on a map that is not a style map of the job's taps.  A setting with a positive
 * weight needs a configured job, the f16x2 arithmetic and no guided level (NST_E_STATE otherwise).  Life cycle of
 * nst_job_set_gram_shift: the call waits for the context's work, drops every level's targets (mu^t and sigma^t are made with
 * them) and any captured closure graph, and ends the validity of an optimiser's remembered closure and of a pending
 * nst_closure_backward.  Every buffer of the term is allocated here, never in a closure.  nst_job_configure clears the
 * setting.  The work belongs to the forward half of the closure.  It composes with any taps (pre-ReLU included; a weight
 * on a map that later taps leave out is ignored), colour mode, pooling, style layer weights, blends, the Laplacian loss,
 * the matting term, the Gram shift, the closure halves, closure reuse, the lazy backward, level sharding and every f16x2
 * schedule - batched and per level (single_stream and h2_band_rows included), use_graph, gram_overlap (the statistics and
 * fold launches ride with the Gram batch of their maps, on either stream), level_split, h2_persist, keep_all_maps,
 * forward_pack = 0, gram_pack = 0 - with the bits of the default schedule (level_split: of the two masked closures its chains
 * are); tests/test_hip_schedule_matrix.py holds each.  While a weight is positive, nst_level_set_guidance (R > 0), nst_level_set_targets_guided and nst_window_*
 * return NST_E_STATE.
 * nst_job_moments: the current setting (any pointer may be NULL).
 * nst_job_moment_losses: the unweighted (mean_i, std_i) of the last closure, to out (DEVICE, levels x 6 x 2 floats, by map
 * index); zeros for maps without the term and for levels outside the last level mask.  Asynchronous on `stream`.
 * nst_moments: the statistic alone, beside nst_gram_shifted, by the closure's kernels: f device (C,h,w), C = 64 or a
 * multiple of 128 up to 1024; mean_out, std_out: device, C floats each.  Any arithmetic mode.  Synchronous on `stream`. */
int nst_job_set_moments(nst_ctx* ctx, const float mean_w[6], const float std_w[6], float epsilon);
int nst_job_moments(const nst_ctx* ctx, float mean_w[6], float std_w[6], float* epsilon);
int nst_job_moment_losses(nst_ctx* ctx, float* out /* device, levels x 6 x 2 */, void* stream);
int nst_moments(nst_ctx* ctx, const float* f, int C, int h, int w, float epsilon, float* mean_out, float* std_out, void* stream);

/* LossBuilder.__init__ (neural_style_transfer.py:68-82): target content representation
 * ReLU(conv4_2) of the content image and the 5 target Gram matrices of the style image of one
 * level (of the maps nst_job_set_taps chose, when it was called).  content: device (3,h,w) of that level's size; style: device (3,hs,ws), any size.
 * (1,h,w) / (1,hs,ws) prepared luminance images under NST_COLOR_LUMINANCE (nst_job_set_color). */
int nst_level_set_targets(nst_ctx* ctx, int level, const float* content, const float* style,
                          int hs, int ws, void* stream);

/* The same with the style targets blended from K style images (jcjohnson/neural-style's -style_blend_weights; per map, the
 * scale control of Gatys et al. 2017, "Controlling Perceptual Factors in Neural Style Transfer": fine structure from one
 * painting, coarse structure from another).  1 <= K <= NST_MAX_STYLES.  styles[k]: device (3,hs[k],ws[k]) ((1,hs[k],ws[k])
 * under NST_COLOR_LUMINANCE), every size its own and >= 16x16.  blend: HOST, K x 6 row-major, B[k][i] = weight of image k
 * on map i of Vgg19.layer_names; every entry finite and >= 0, every column of a map in the style set with a positive sum;
 * NST_E_ARG for anything else (the level then has the targets it had).  Columns of maps outside the style set are ignored.
 *   b^[k][i] = B[k][i] / sum_k B[k][i], computed in fp64 and cast to float;
 *   target of map i: Gt_i = sum_k b^[k][i] G_i(style_k), accumulated in fp32 in ascending k - the first contributing k is
 *   written as b^ G (not added to a zero fill), every later one as Gt + b^ G, product and sum each rounded; a k with
 *   B[k][i] = 0 is skipped, and a style image whose row is zero over the whole style set gets no forward pass.
 * The gradient of the style term is that of sum_k b^[k][i] MSE(G_i, G_i(style_k)); the LOSS differs from that sum by a
 * constant that does not depend on the image (sum_k b^_k |G_k|^2 - |sum_k b^_k G_k|^2, over C^2): the loss row reports
 * MSE(G_i, Gt_i).  The content target is that of nst_level_set_targets.  K = 1 gives the targets of nst_level_set_targets
 * bitwise, whatever the (positive) entries of its row: nst_level_set_targets is the K = 1 case of the same code.  Same
 * life cycle as nst_level_set_targets.  The stripe closure (nst_window_*) reads its Gram targets from the level's targets,
 * so blended targets are honoured there. */
int nst_level_set_targets_blend(nst_ctx* ctx, int level, const float* content, int K, const float* const* styles,
                                const int* hs, const int* ws, const float* blend /* K x 6, row-major */, void* stream);

/* Spatial control (Gatys et al. 2017, "Controlling Perceptual Factors in Neural Style Transfer", guided Gram matrices):
 * every region of the image takes its style from its own region of the style image.
 *
 * Regions and guidance maps
 * - Regions are r = 0..R-1, with 1 <= R <= 4.
 * - Each level has one guidance plane per region at the level's resolution: t_r(y,x) in [0,1], fp32, shape (R,h,w).
 * - Regions may overlap and need not cover the image.
 * - The guidance of a map at network scale s (0..4) is the level plane passed s times through a 2x2/2 mean pool.
 *   - Floor sizes.
 *   - Order ((e00+e01)+e10)+e11 times 1/4, the order of every pooling kernel here.
 *   - This holds regardless of nst_job_set_pooling.
 * Mass
 * - n_r = sum_p t_r(p)^2, formed in double in a fixed two-stage order and kept per (level, map, region).
 * Guided Gram of a map F (N pixels x C)
 * - G_r = sum_p t_r(p)^2 F(p)F(p)^T / (C n_r).
 * - With t = 1 this is today's F^T F/(C h w).
 * Style term of a level
 * - (sum_i w_i sum_r lambda_r MSE(G_ri, Gt_ri)) / nstyle.
 * - lambda_r >= 0 are the region weights.  The default is 1, and at least one must be positive.
 * - The loss rows keep their layout: the style entry holds this sum.
 * Backward
 * - dF(p) = sum_r t_r(p)^2 F(p) S_r.
 * - S_r = coef_r (G_r - Gt_r).
 * - coef_r = (float)((double)sw w_i lambda_r 4 / (nstyle C^2 C n_r)).
 * Targets
 * - Gt_ri is the guided Gram of the style image's map i under the style image's own guidance planes.
 * - Those planes use the same R, are sized to the style image of that level, and use the same pooling chain.
 * Refusals
 * - Refuse with NST_E_ARG, leaving the context unchanged and usable, when any of these holds:
 *   - a value lies outside [0,1] or is non-finite;
 *   - R is out of range;
 *   - any (map in use, region) has mass n_r < 1 on the image side or the style side.  Less than one pixel's worth gives a
 *     Gram of noise.
 *
 * nst_level_set_guidance: planes = device (R,h,w) of the level's size, copied (the caller's buffer is free on return: the
 * call synchronises `stream` to read the masses back); lambda = HOST, R floats, or NULL for ones.  R = 0 clears the level's
 * guidance (planes and lambda are ignored): the level is then evaluated by exactly the launches of a context that never had
 * any, with the targets nst_level_set_targets* gave it.  Guidance of another R than the level's guided targets were made
 * for invalidates those targets; new planes of the same R keep them (they depend on the style side only).  The workspace of
 * the R guided Grams (slabs, targets, S matrices, loss partials, the plane pyramid) is allocated here, never in a closure.
 * nst_level_set_targets_guided: the level's content target as nst_level_set_targets makes it, and the guided targets of the
 * R regions of the level's guidance (NST_E_STATE when the level has none) from `style` (device (3,hs,ws), (1,hs,ws) in
 * luminance mode) under style_planes = device (R,hs,ws).  The unguided Gram targets of the level are left as they are; the content target is
 * ONE buffer shared by the guided and the unguided path, so after a later nst_level_set_guidance(R = 0) the level is
 * evaluated with the content target given here and the style targets the last nst_level_set_targets* gave it.
 * A guided level is evaluated by nst_closure, nst_closure_levels and the closure halves under both schedules, with any
 * taps, pooling, colour mode and style layer weights; the levels of one closure call are all guided or all unguided
 * (NST_E_STATE otherwise), and under level sharding a level's guidance lives with the rank that owns it.  The guided Gram
 * partials run in the f16x2 arithmetic with the pixel row scaled by t_r(p) as it is staged; the guided backward is a launch
 * of its own on the exact fp32 matrix cores whose output reaches the input-gradient launch below the map as its addend, so
 * no convolution launch of a guided job carries a second K source.
 * NST_E_STATE (see nst_last_error): contexts in the bf16x3 / f32 arithmetic; the stripe closure (nst_window_*) while any
 * level is guided; nst_level_set_targets_blend with K > 1 on a guided level.
 * Both setters (also when they fail) drop any captured closure graph and end the validity of an optimiser's remembered
 * closure and of a pending nst_closure_backward.  nst_job_configure and nst_job_set_taps clear every level's guidance;
 * nst_job_set_color and nst_job_set_pooling keep the planes and drop the guided targets with the others.
 * nst_level_guidance: R (0: none), the R region weights, and the masses n_r of the five network scales (mass[s * 4 + r];
 * any pointer may be NULL).  nst_level_guidance_planes: the (R, h >> scale, w >> scale) planes of one scale, to device
 * memory. */
int nst_level_set_guidance(nst_ctx* ctx, int level, int R, const float* planes /* device (R,h,w) */,
                           const float* lambda /* host, R floats, or NULL */, void* stream);
int nst_level_set_targets_guided(nst_ctx* ctx, int level, const float* content, const float* style, int hs, int ws,
                                 const float* style_planes /* device (R,hs,ws) */, void* stream);
int nst_level_guidance(const nst_ctx* ctx, int level, int* R, float lambda[NST_MAX_REGIONS], double mass[5 * NST_MAX_REGIONS]);
int nst_level_guidance_planes(nst_ctx* ctx, int level, int scale, float* out, void* stream);

/* Temporal consistency: a pixel-space term that holds a level image to an anchor under a per-pixel weight plane, the warp
 * that makes the anchor and the weights that say where to trust it.  After Ruder, Dosovitskiy & Brox, "Artistic Style
 * Transfer for Videos" (GCPR 2016): frame i starts from the previous result warped along the optical flow (section 3,
 * "initialization"), a weighted squared distance to that warped result joins the loss (their eq. 7, the short-term temporal
 * loss), and the weight is 0 where the flow is unreliable (section 4, after Sundaram, Brox & Keutzer, ECCV 2010).  The
 * reference has no counterpart.  The anchor is DATA of one job, like the content levels - not a setting of the context.
 * Term of a level image y (C,h,w), C = 3, or 1 under NST_COLOR_LUMINANCE, an anchor a (C,h,w) and weights c (h,w) in [0,1]
 * - tmp = (float)((1/n) sum_{ch,p} c(p) (y(ch,p) - a(ch,p))^2), n = C h w.  c absent: ones.
 * - The differences and products are formed in double from the fp32 planes; the sum is in double in a fixed two-stage order
 *   (a fixed grid of blocks whose threads add their strided shares in index order, then the block partials).
 * Loss row
 * - A level with an anchor of weight gamma > 0 has the total (... + mom) + gamma tmp: added after the moment term, product
 *   and sum each rounded.  NST_LOSS_ROW stays 4.  nst_job_temporal_losses returns the tmp.
 * Gradient
 * - d/dy(ch,p) = coef (c(p) (y(ch,p) - a(ch,p))), coef = (float)((double)gamma 2 / n): the difference, the product with c
 *   (left out when c is absent) and the product with coef are fp32, each rounded.  It is accumulated into the level gradient
 *   after the total-variation, Laplacian and matting gradients; a term of exactly 0 leaves the gradient's bits as they are.
 * - Nothing is kept between the halves: the backward half forms the difference again.
 * Luminance
 * - The anchor is one plane in the units of the optimised plane u (nst_luminance of the warped frame), and C = 1 above.
 * Warp (nst_warp_bilinear): out(ch, x, y) = bilinear(src(ch), x + dx, y + dy), flow plane 0 = dx, plane 1 = dy, in pixels
 * - Per axis the sample position is the integer part and the fraction of the FLOW alone: x0 = x + (int)floor(dx),
 *   t = dx - floor(dx); x + dx is never formed in fp32, so the fraction does not depend on the image size.
 * - Taps x0, x0 + 1 (y0, y0 + 1) clamped to the image; out = (v00 (1-tx) + v01 tx)(1-ty) + (v10 (1-tx) + v11 tx) ty in fp32,
 *   every operation rounded once.
 * - valid = 1 where the four taps lie inside the image before clamping (x0 >= 0, x0 + 1 <= w - 1, likewise y), else 0: a
 *   sample exactly on the last column or row has its second tap outside and is not valid.
 * - Non-finite flow: valid = 0 and out = the source pixel itself.
 * Flow weights (nst_flow_weights): c (h,w) from the forward flow fwd (frame i-1 -> i) and the backward flow bwd (i -> i-1)
 * - w~(p) = fwd sampled bilinearly at p + bwd(p), by the position rule of the warp; (u^, v^) = bwd(p).
 * - c(p) = 0 where |w~ + bwd|^2 > 0.01 (|w~|^2 + |bwd|^2) + 0.5 (disocclusion: the flows do not undo one another),
 * - c(p) = 0 where |grad u^|^2 + |grad v^|^2 > 0.01 |bwd|^2 + 0.002 (motion boundary), grad = central differences with
 *   replicated borders, 0.5 (f(x+1) - f(x-1)) and likewise in y,
 * - c(p) = 0 where the sample of w~ is not valid or bwd(p) is not finite, c(p) = 1 everywhere else.
 * - The comparisons run in fp32, one rounding per operation, in this order: (su su + sv sv), s = w~ + bwd, against
 *   0.01 ((wu wu + wv wv) + (bu bu + bv bv)) + 0.5; ((ux ux + uy uy) + (vx vx + vy vy)) against 0.01 (bu bu + bv bv) + 0.002.
 * No float atomics: a closure with the term is bitwise reproducible, as closure reuse and the lazy backward need.
 *
 * nst_level_set_anchor: anchor = device (C,h,w) of the level's size, weights = device (h,w) or NULL for ones; both are
 * copied into buffers of the level that nst_ctx_bytes counts, and the caller's are free on return (the call synchronises
 * `stream`).  A NULL anchor or gamma = 0 clears the level's term and credits exactly what it was charged.  NST_E_STATE: no
 * configured job.  NST_E_ARG: level out of range, gamma negative or non-finite.  A refusal changes nothing about the level.
 * Life cycle of nst_level_set_guidance: the call waits for the context's work, never allocates in a closure, drops any
 * captured closure graph and ends the validity of an optimiser's remembered closure and of a pending nst_closure_backward.
 * The targets stay.  nst_job_configure drops every level's anchor with the levels; nst_job_set_color drops them when the
 * mode changes (the planes are the other mode's).  A level without an anchor is evaluated by exactly the launches of a
 * context that never had one and computes the same bits.  The term composes with every setting, conv mode and schedule
 * (use_graph included), the closure halves and level sharding (a level not owned contributes zeros).  The stripe closure
 * (nst_window_*) returns NST_E_STATE while its level carries an anchor.
 * nst_level_anchor: the level's gamma (0: none) and whether it has a weight plane (either pointer may be NULL).
 * nst_job_temporal_losses: the unweighted tmp of the last closure per level, to out (DEVICE, levels floats); zeros for
 * levels without an anchor or outside the last level mask.  Asynchronous on `stream`. */
int nst_level_set_anchor(nst_ctx* ctx, int level, const float* anchor /* device (C,h,w), or NULL: clear */,
                         const float* weights /* device (h,w), or NULL: ones */, float gamma, void* stream);
int nst_level_anchor(const nst_ctx* ctx, int level, float* gamma, int* weighted);
int nst_job_temporal_losses(nst_ctx* ctx, float* out /* device, levels */, void* stream);

/* Long-term consistency: several earlier frames in the one anchor a level holds.  Ruder, Dosovitskiy & Brox (GCPR 2016),
 * section 4.3, eq. 9-10: frame i is held to frame i-1 where that flow is reliable, elsewhere to i-2, then i-4, ... - so what
 * an object uncovers as it moves on comes back with the texture it had before it was covered.
 * Identity.  For anchors a_j under weights l_j, W = sum_j l_j and a~ = sum_j l_j a_j / W:
 *   sum_j l_j (y - a_j)^2 = W (y - a~)^2 + sum_j l_j (a_j - a~)^2, and the second sum does not depend on y.
 *   The single anchor a~ under the weight plane W has exactly the gradient of the J-term loss; tmp differs from the J-term
 *   value by the constant (1/n) sum_{ch,p} sum_j l_j (a_j - a~)^2 of the job, which is exactly 0 where at most one l_j is not 0
 *   (weights of 0 and 1, as nst_flow_weights makes them).  nst_level_set_anchor, the term and the closure are unchanged.
 * nst_anchor_fold: J sources (device (C,h,w) each: the warped results, ascending in frame offset) and J weight planes
 * (device (h,w) each: their reliability) -> anchor (C,h,w), weight (h,w) and, if parts is not NULL, parts (J,h,w).
 * Per pixel p, in fp32, no contraction, every operation rounded once, in this order:
 * - c_j = w_j(p) > 0 ? min(w_j(p), 1) : 0: a NaN or a negative weight counts as 0; values in [0,1] keep their bits.
 * - s_0 = 0, l_j = max(c_j - s_j, 0), s_{j+1} = s_j + c_j (eq. 10: a source counts only where no nearer one is reliable).
 * - Wsum = ((l_0 + l_1) + ...) in index order; weight(p) = min(Wsum, 1); parts(j, p) = l_j.
 * - j* = the first j with l_j > 0.  None: anchor(ch, p) = sources[0](ch, p) and weight(p) = 0.
 * - Otherwise anchor(ch, p) = ((a_j* + t_j') + t_j'') + ... over the j > j* with l_j > 0 in index order,
 *   t_j = (l_j / Wsum) (a_j - a_j*), the division correctly rounded.
 * - With one live source the sum is empty and the anchor has that source's bits.  A source with l_j = 0 never enters the
 *   result: its non-finite values do not leak.
 * One launch of a streaming kernel; the 2 J pointers travel by value as a kernel argument; the context allocates nothing and
 * nst_ctx_bytes does not move; reads no job state.  Asynchronous on `stream`.  16-byte accesses on every plane that starts
 * on a 16-byte boundary (per channel: plane ch of every source and of the anchor; the weight planes in and out together;
 * each plane of parts), pixel by pixel on the others and on the last h w % 4 pixels.
 * NST_E_ARG, with nothing launched: J outside 1 .. NST_MAX_ANCHOR_SOURCES, C not 1 or 3, h or w < 1, a null pointer other
 * than parts, an output that overlaps an input or another output. */
#define NST_MAX_ANCHOR_SOURCES 8
int nst_anchor_fold(nst_ctx* ctx, int J, const float* const* sources /* host array of J device (C,h,w) */,
                    const float* const* weights /* host array of J device (h,w) */, int C, int h, int w,
                    float* anchor /* device (C,h,w) */, float* weight /* device (h,w) */,
                    float* parts /* device (J,h,w), nullable */, void* stream);

/* optimizer_step_callback without its LR decay and prints (neural_style_transfer.py:152-199) =
 * sum over levels of LossBuilder.build (:84-112) on the bicubic 1/2 chain of x (:170-176),
 * then backward (:193).  x, grad: device (3,H0,W0) ((1,H0,W0) under NST_COLOR_LUMINANCE).  losses: device, NST_LOSS_ROW*levels+1
 * floats = per level (total, content, style, tv) unweighted components as the reference
 * prints them, then the grand total.  Asynchronous on `stream`. */
int nst_closure(nst_ctx* ctx, const float* x, float content_weight, float style_weight,
                float tv_weight, float* grad, float* losses, void* stream);

/* The same closure restricted to the pyramid levels whose bit is set in level_mask: the level-sharded
 * form of BASELINE config 4 (rank r owns some levels; loss = sum over levels, so the pixel gradients and
 * loss rows of the ranks add up: one all-reduce(sum) of `grad` (3*H0*W0 floats) and `losses`).  Rows of
 * levels not in the mask are zeros; the last element is the sum of the owned level totals. */
int nst_closure_levels(nst_ctx* ctx, const float* x, float content_weight, float style_weight,
                       float tv_weight, unsigned level_mask, float* grad, float* losses, void* stream);

/* nst_closure_levels in two halves, for a caller that needs the loss before it knows whether it needs the gradient (a
 * line search that takes or drops a trial point on its loss alone; the reference always runs both: loss.backward() at
 * neural_style_transfer.py:193).  Same arguments, same launches in the same order:
 *   nst_closure_forward: the bicubic pyramid, the forward convolutions, every Gram launch, the loss terms; writes
 *     `losses`, BITWISE the row nst_closure_levels writes for these arguments.  Nothing of the backward is launched.
 *   nst_closure_backward: the backward pass of that forward; writes `grad`, BITWISE the gradient nst_closure_levels
 *     writes.  x must still hold the image the forward half evaluated (the total-variation gradient reads it).
 * Validity: the backward half belongs to the LAST nst_closure_forward on the context and is valid only while that
 * forward is the last thing that used the context's workspaces - no nst_closure / nst_closure_levels, nst_window_*,
 * nst_level_activation, nst_level_set_* or nst_job_configure / nst_job_set_* call in between, not even a failed one - and only with the
 * same x pointer, weights and level_mask, once.  Otherwise it returns NST_E_STATE, launches nothing and leaves `grad`
 * untouched; the context stays usable (a refused backward half itself ends nothing: the forward half before it is still good).
 * What does NOT end the validity: calls that write no level's buffers - the standalone pieces below, which work on caller
 * buffers and scratch of their own (nst_vgg_*, nst_gram*, nst_moments, nst_guided_gram_backward, nst_total_variation, nst_laplacian_loss,
 * nst_matting_loss, nst_bicubic_*, nst_resize_bicubic, nst_color_*, nst_luminance*, nst_adam_step, nst_lbfgs_direction), the
 * getters (nst_job_color ... nst_job_moments, nst_level_guidance, nst_job_map_stats), the copies nst_level_image,
 * nst_job_laplacian_losses, nst_job_matting_losses, nst_job_moment_losses, nst_level_gram_offsets and
 * nst_level_guidance_planes, refused or not,
 * and nst_set_timing.  Both halves run on the batched schedule only (nst_options.batched, its default,
 * without use_graph): elsewhere nst_closure_forward returns NST_E_UNAVAILABLE before it launches anything, and the
 * caller evaluates nst_closure_levels.  Asynchronous on `stream`.  Timing (nst_set_timing): a forward half is one
 * closure record; its backward half adds its launches and time to the totals without counting a second closure. */
int nst_closure_forward(nst_ctx* ctx, const float* x, float content_weight, float style_weight, float tv_weight,
                        unsigned level_mask, float* losses, void* stream);
int nst_closure_backward(nst_ctx* ctx, const float* x, float content_weight, float style_weight, float tv_weight,
                         unsigned level_mask, float* grad, void* stream);

/* torch.optim.Adam / torch.optim.LBFGS as constructed at neural_style_transfer.py:134-136,
 * driving nst_closure, including the closure's `lr *= 0.999` (:155-158).  kind: 0 = adam
 * (torch:optim/adam.py:457-546, betas (0.9,0.999), eps 1e-8), 1 = lbfgs
 * (torch:optim/lbfgs.py:332-537: max_iter 1, strong_wolfe, history 100; lbfgs_max_eval is the
 * constructor's max_eval: 1 = torch 2.10 behaviour of the reference's arguments, 26 = legacy
 * line search). */
#define NST_OPT_ADAM 0
#define NST_OPT_LBFGS 1
int nst_opt_create(nst_ctx* ctx, int kind, float lr_start, int lbfgs_max_eval, nst_opt** out);
void nst_opt_destroy(nst_opt* opt);

typedef struct nst_step_info {
    int closures;        /* closures of this step as the reference's `step` counts them (Adam 1, L-BFGS >= 1), served
                            ones included (nst_opt_set_closure_reuse) */
    int total_closures;  /* the reference's `step` counter after this call */
    int accepted;        /* L-BFGS: 1 if x moved, 0 if the trial was rejected; Adam: 1 */
    float loss;          /* loss of the FIRST closure of this step (what optimizer.step returns) */
    float lr;            /* learning rate after this step's decays */
    float t;             /* L-BFGS step length taken (0 when rejected) */
    int history;         /* L-BFGS: curvature pairs held after this step (0..100) */
} nst_step_info;

/* one optimizer.step(closure) (neural_style_transfer.py:205-206).  x: device (3,H0,W0), updated
 * in place.  losses_host (nullable): HOST buffer of closures_capacity*(NST_LOSS_ROW*levels+1)
 * floats receiving the loss rows of every closure made.  Synchronous for L-BFGS (host control
 * flow needs the loss), asynchronous on `stream` for Adam when losses_host is NULL. */
int nst_opt_step(nst_opt* opt, float* x, float content_weight, float style_weight, float tv_weight,
                 float* losses_host, int closures_capacity, nst_step_info* info, void* stream);

/* Level sharding inside the optimiser drivers: every closure the driver evaluates covers only
 * `level_mask`, then calls hook(user) - which must all-reduce(sum) the `grad` and `losses` DEVICE buffers
 * given here over the ranks, ordered on the stream passed to nst_opt_step - before the driver reads
 * them.  The update itself is replicated (deterministic), so no broadcast is needed.  grad: 3*H0*W0
 * floats, losses: NST_LOSS_ROW*levels+1 floats, both owned by the caller and alive as long as `opt`. */
typedef void (*nst_reduce_hook)(void* user);
int nst_opt_shard_levels(nst_opt* opt, unsigned level_mask, float* grad, float* losses, nst_reduce_hook hook,
                         void* user);

/* The same with the collective behind the ABI: every closure the driver evaluates covers `level_mask`, then ONE
 * ncclAllReduce(sum, fp32) over `comm` of a single buffer holding the 3*H0*W0 gradient floats followed by the
 * NST_LOSS_ROW*levels+1 loss scalars, on the stream passed to nst_opt_step; the grand total is re-formed from the level rows
 * in level order, so L-BFGS' accept test takes the same branch as the unsharded run.  comm == NULL switches sharding off. */
int nst_opt_shard_levels_comm(nst_opt* opt, unsigned level_mask, nst_comm* comm);

/* curvature pairs currently held by L-BFGS and the optimiser's iteration count (Adam: its step count k).  The pair count
 * rises to 100 and stays there: the oldest pair leaves when a new one is kept (tests/test_hip_lbfgs_history.py holds a run
 * through a full history, 23 evictions and a dropped pair). */
int nst_opt_history(const nst_opt* opt, int* pairs, int* n_iter);

/* L-BFGS closure reuse (default on; env NST_CLOSURE_REUSE=0 at nst_opt_create turns it off).  The closure is bitwise
 * reproducible, so when a step starts at bitwise the image the previous step left (a rejected or skipped trial, or an
 * accepted trial whose closure was the last one made), with the same weights and no change to the job in between
 * (nst_job_configure, nst_job_set_taps, nst_job_set_color, nst_job_set_pooling, nst_job_set_style_weights,
 * nst_job_set_laplacian, nst_job_set_matting, nst_job_set_gram_shift, nst_job_set_moments, nst_level_set_targets, nst_level_set_targets_blend), its first closure is served from what
 * the optimiser remembers instead of evaluated: same loss row, step counter, lr decay, step info and image.  One
 * device compare of x decides, so the caller may write x between steps.  Never in the sharded modes; Adam never.
 * Changing the setting drops what is remembered. */
int nst_opt_set_closure_reuse(nst_opt* opt, int enabled);
/* closures this optimiser evaluated and served so far (their sum is nst_step_info.total_closures) */
int nst_opt_closure_stats(const nst_opt* opt, long* evaluated, long* served);

/* L-BFGS lazy backward (default on; env NST_LAZY_BACKWARD=0 at nst_opt_create turns it off).  The last evaluation a
 * line-search budget allows (with lbfgs_max_eval 1: every trial point) is used for its loss alone unless its point is
 * the one taken: strong_wolfe (torch:optim/lbfgs.py:40-209) never reads its gradient or its g.d again.  The driver
 * evaluates it with nst_closure_forward, decides as before, and runs nst_closure_backward only when that point is taken.
 * Loss rows, step info, lr decay, closure counts and the image are bitwise what they are with the setting off.  Never in
 * the sharded modes or under a partial level mask, and not where nst_closure_forward is unavailable; Adam never. */
int nst_opt_set_lazy_backward(nst_opt* opt, int enabled);
/* evaluated closures that ran as a forward half only so far, and those of them whose backward half never ran */
int nst_opt_backward_stats(const nst_opt* opt, long* forward_only, long* skipped);

/* ---- RCCL communicator (one rank per GPU; the reference has no collective: neural_style_transfer.py:236-245).
 * librccl is resolved at run time; without it these return NST_E_STATE.  Bootstrap: rank 0 calls nst_comm_unique_id and
 * hands the NST_COMM_ID_BYTES bytes to the other ranks by whatever channel the host program has (file, socket, MPI,
 * torch.distributed); then every rank calls nst_comm_create (collective). */
#define NST_COMM_ID_BYTES 128
int nst_comm_unique_id(void* id);
int nst_comm_create(int device, int rank, int world, const void* id, nst_comm** out);
void nst_comm_destroy(nst_comm* comm);
/* rank / world of the communicator and what it has carried so far (any pointer may be NULL) */
int nst_comm_info(const nst_comm* comm, int* rank, int* world, long* calls, double* bytes);
/* in-place all-reduce(sum) of n floats at the DEVICE pointer buf, ordered on `stream` */
int nst_comm_allreduce_sum(nst_comm* comm, float* buf, size_t n, void* stream);

/* ---- the optimisers' update arithmetic alone, exported for unit parity -------------------------------
 * One torch.optim.Adam update (torch:optim/adam.py:457-546, betas (0.9, 0.999), eps 1e-8) of the n floats at x from the
 * gradient g and the state (m = exp_avg, v = exp_avg_sq), all DEVICE pointers updated in place; k: the step count of
 * this update (1-based), lr: the group's learning rate at this update (neural_style_transfer.py:134, :155-158). */
int nst_adam_step(nst_ctx* ctx, float* x, const float* g, float* m, float* v, size_t n, int k, double lr, void* stream);
/* The L-BFGS direction d = -H g of torch:optim/lbfgs.py:396-442 from m curvature pairs: y[i] = old_dirs[i],
 * s[i] = old_stps[i] (HOST arrays of m DEVICE pointers, oldest first), ro[i] = 1 / (y_i . s_i) (HOST floats),
 * h_diag = H_diag; g, d: DEVICE, n floats.  form 0: from inner products (what the driver runs by default), form 1: the
 * sequential two-loop recursion in torch's arithmetic order.  Synchronous. */
int nst_lbfgs_direction(nst_ctx* ctx, const float* g, const float* const* y, const float* const* s, const float* ro, int m,
                        float h_diag, size_t n, int form, float* d, void* stream);

/* ---- standalone pieces of the path, exported for unit parity -------------------------------- */

/* Vgg19.forward (neural_nets.py:53-68): x device (3,h,w) -> the six maps, each written as
 * (C,h_i,w_i) planar fp32 (reference layout) into outs[i] (device; NULL to skip). */
int nst_vgg_features(nst_ctx* ctx, const float* x, int h, int w, float* const* outs, void* stream);
/* The same forward pass, all 13 post-ReLU conv outputs conv1_1 ... conv5_1 as (C,h_l,w_l) planar fp32 into outs[l]
 * (device; NULL to skip): the decisions (unit on / pooling arg-max) nst_vgg_features_backward of the same x takes. */
int nst_vgg_activations(nst_ctx* ctx, const float* x, int h, int w, float* const* outs, void* stream);
/* d(sum_i <outs_i, gouts_i>)/dx through the network: gouts[i] device (C,h_i,w_i) or NULL. */
int nst_vgg_features_backward(nst_ctx* ctx, const float* x, int h, int w, const float* const* gouts,
                              float* gx, void* stream);
/* The post-ReLU output of conv layer `layer` (0 = conv1_1 ... 12 = conv5_1) that the LAST closure / window pass left in the
 * workspace of pyramid level `level`, written as (C,h_l,w_l) planar fp32 to out (device).  The parity tests read the
 * ReLU and max-pool DECISIONS of the device pass from it (a unit is on where the value is > 0; a pooling window passes its
 * gradient to its first maximum) and hand them to the oracle, so that gradients are compared under equal decisions. */
int nst_level_activation(nst_ctx* ctx, int level, int layer, float* out, void* stream);
/* Which maps exist after a pass.  In the batched f16x2 schedule a forward launch that feeds a pooling layer (conv1_2,
 * conv2_2, conv3_4, conv4_4) writes the pooled map, the ReLU mask and the pool code, and its full-resolution map only where
 * something reads it: where it is a style or the content map of the job's taps, or the top of the chain.  With the default
 * taps none of the four is stored.  nst_level_activation stays exact: a request for a map that was left out repeats that
 * layer's launch over the levels of the level's last pass (same tiles, same summation order), now storing the map.  One
 * sequence cannot be served and returns NST_E_STATE with nothing written: the level's last pass covered other levels too
 * (nst_closure over levels {0, 1}) and a later call has evaluated some of those without this one (nst_closure_levels,
 * nst_closure_forward or nst_opt_shard_levels with a mask that leaves this level out) - evaluate the level again, or keep
 * all maps.  Every other schedule and arithmetic, and a context with use_graph = 1 (a replay runs no host code that could
 * keep the record of stored maps), stores all maps.
 *   nst_job_map_stats: bit l of *stored_mask = conv layer l's map was stored by the last forward pass of `level` (or by a
 *     request since); 0 before any pass and after a call that sets the job up anew.
 *   nst_ctx_set_keep_all_maps(ctx, 1): every launch stores its map, as before the elision - the A/B twin in one build;
 *     losses, gradients, pooled maps, masks and codes are bitwise the same under either setting.  A new context takes
 *     env NST_KEEP_ALL_MAPS (read once at creation), default 0.  nst_ctx_keep_all_maps: the setting, -1 for a null context. */
int nst_job_map_stats(nst_ctx* ctx, int level, unsigned* stored_mask);
int nst_ctx_set_keep_all_maps(nst_ctx* ctx, int enabled);
int nst_ctx_keep_all_maps(const nst_ctx* ctx);
/* The packed forward half (on by default).  In the batched f16x2 schedule a forward pass over more than one pyramid level
 * clears the absmax records, takes the TV partial sums and runs conv1_1 in ONE launch each for all levels of the pass
 * (conv1_1's persistent tile loop walks the tiles of every level), a forward half on its own (nst_closure_forward) takes its
 * content and TV loss terms in one launch each, and the Gram finish pass no longer writes S in bf16 pieces, which only the
 * bf16x3 arithmetic reads.  Every output element is computed by the same instructions in the same order under either
 * setting: losses, gradients, maps, masks and codes are bitwise the same (an absmax record may hold its maximum in another
 * slot).  Per-level walkers, target forwards, stripes and a context with use_graph = 1 keep the per-level launches.
 *   nst_ctx_set_forward_pack(ctx, 0): the per-level launches and the bf16 pieces of S - the A/B twin in one build.  A new
 *     context takes env NST_FORWARD_PACK (read once at creation), default 1.  nst_ctx_forward_pack: the setting, -1 for a
 *     null context. */
int nst_ctx_set_forward_pack(nst_ctx* ctx, int enabled);
int nst_ctx_forward_pack(const nst_ctx* ctx);
/* The packed Gram pass (on by default).  The finish pass of a Gram matrix reads only the elements with j >= i of every
 * partial slab and writes each result to (i,j) and (j,i).  Packed, the fp16-piece partial kernels - plain, guided and shifted,
 * single maps and batches - do not compute the 32x32 blocks strictly below the diagonal of a diagonal tile and leave that
 * part of a slab unwritten, and a plain batch (the style maps of all pyramid levels of a closure) takes its 64-channel and its
 * 128-channel-tile maps in ONE partial launch instead of two.  Every element that is read is the sum of the same products in
 * the same order under either setting: Gram matrices, losses and gradients are bitwise the same.
 *   nst_ctx_set_gram_pack(ctx, 0): every block computed and written, one partial launch per tile shape - the A/B twin in one
 *     build.  A new context takes env NST_GRAM_PACK (read once at creation), default 1.  nst_ctx_gram_pack: the setting, -1
 *     for a null context. */
int nst_ctx_set_gram_pack(nst_ctx* ctx, int enabled);
int nst_ctx_gram_pack(const nst_ctx* ctx);
/* Weight fragments from L2 in the short-K forward launches (on by default).  The forward launches of the f16x2 direct kernel
 * that run on 16-channel chunks - conv1_2, conv2_1, conv2_2, conv3_1 - read their weight fragments straight from a second
 * image of the layer's fp16 pieces, laid out in MFMA fragment order when the context is created (2.2 MB, counted in
 * nst_ctx_bytes), instead of staging a slice per tap through LDS: one workgroup barrier per 16-channel chunk instead of one
 * per tap.  Every accumulator sees the same products in the same order: all maps, losses and gradients are bitwise the same.
 * The input-gradient launches of those shapes are not affected.
 *   nst_ctx_set_h2_direct_weights(ctx, 0): the weight slices go through LDS - the A/B twin in one build.  Otherwise a mask of
 *     kernel shapes: 1 = the 64-channel shape (conv1_2), 2 = the 128-channel short-K shape (conv2_1, conv2_2, conv3_1), 3 =
 *     both; NST_E_ARG outside 0 .. 3.  A new context takes env NST_H2_DIRECT_WEIGHTS (read once at creation); the default, 3, is
 *     the set of shapes that measured faster (profiles/r21_h2_direct_weights.txt).  nst_ctx_h2_direct_weights: the setting, -1
 *     for a null context.  nst_ctx_h2_direct_launches: conv_h2 launches of this context that ran the new loop so far (-1 for a
 *     null context) - a launch that quietly stayed on the other loop is one this count misses. */
int nst_ctx_set_h2_direct_weights(nst_ctx* ctx, int enabled);
int nst_ctx_h2_direct_weights(const nst_ctx* ctx);
long long nst_ctx_h2_direct_launches(const nst_ctx* ctx);
/* The image of pyramid level `level` >= 1 that the last closure evaluated - the bicubic 1/2 chain of x
 * (neural_style_transfer.py:170-176) - as (3,h_l,w_l) planar fp32 to out (device).  The total-variation term takes
 * sign(y_i - y_j) of neighbouring pixels: on flat image regions those differences are rounding noise of the down-sampling,
 * so the parity tests read the signs the device pass took from this image. */
int nst_level_image(nst_ctx* ctx, int level, float* out, void* stream);
/* math_utils.gram_matrix (math_utils.py:26-34): f device (C,h,w) -> gram device (C,C). */
int nst_gram(nst_ctx* ctx, const float* f, int C, int h, int w, int normalize, float* gram, void* stream);
/* The guided Gram backward launch on its own, in the closure's own layout: out = addend + sum_r t_r^2 . F . S_r.
 * f, addend (nullable; may be `out` itself), out: device pixel-major (N,C); planes: device (R,N); S: device (R,C,C);
 * relu_bits (nullable): device (N, C/32) words, out is zero where the bit of (pixel, channel) is clear; amax_slots
 * (nullable): device, 64 words, zeroed by the call, whose maximum is the bit pattern of max |out|.  C a multiple of 64,
 * 1 <= R <= NST_MAX_REGIONS.  Reads no job state and needs no particular arithmetic mode. */
int nst_guided_gram_backward(nst_ctx* ctx, const float* f, size_t N, int C, int R, const float* planes, const float* S,
                             const float* addend, const unsigned* relu_bits, float* out, unsigned* amax_slots, void* stream);
/* math_utils.total_variation (math_utils.py:37-41): value (device scalar) and, if grad != NULL,
 * grad (C,h,w) = d tv / d y. */
int nst_total_variation(nst_ctx* ctx, const float* y, int C, int h, int w, float* value, float* grad,
                        void* stream);
/* One entry of the Laplacian loss on its own (nst_job_set_laplacian has the definition): y, content device (C,h,w), C = 3, or
 * 1 with the luminance rule; p the pool size.  value (device scalar) = lap_k; grad (nullable, overwritten) (C,h,w) =
 * d lap_k / dy, with gamma = 1.  Reads no job state.  Synchronous. */
int nst_laplacian_loss(nst_ctx* ctx, const float* y, const float* content, int C, int h, int w, int p, float* value,
                       float* grad /* nullable, overwritten */, void* stream);
/* The matting term on its own (nst_job_set_matting has the definition): y device (C,h,w), prepared; guide device (C,h,w), the
 * guide I itself (in [0,1] for ordinary input); C = 3, or 1 with the luminance rule (y and guide one plane each); h, w >= 3.
 * value (device scalar) = mat; grad (nullable, overwritten) (C,h,w) = d mat / dy, with gamma = 1.  The value is bitwise
 * the same with and without grad.  Reads no job state.  Synchronous. */
int nst_matting_loss(nst_ctx* ctx, const float* y, const float* guide, int C, int h, int w, double epsilon, float* value,
                     float* grad /* nullable, overwritten */, void* stream);
/* The temporal term on its own (nst_level_set_anchor has the definitions of these four): y, anchor device (C,h,w), C = 3 or 1;
 * weights device (h,w) or NULL for ones.  value (device scalar) = tmp; grad (nullable, overwritten) (C,h,w) = d tmp / dy, with
 * gamma = 1.  The value is bitwise the same with and without grad.  Reads no job state.  Synchronous.
 * nst_anchor_geometry: the blocks of the value pass and the elements one block covers per pass of its loop (what a test
 * sizes its block-boundary case by).
 * nst_warp_bilinear: src device (C,h,w), C >= 1; flow device (2,h,w); out device (C,h,w), not src; valid device (h,w) or NULL.
 * nst_flow_weights: fwd, bwd device (2,h,w); out device (h,w).  Both read no job state and are synchronous. */
int nst_anchor_loss(nst_ctx* ctx, const float* y, const float* anchor, const float* weights /* nullable */, int C, int h, int w,
                    float* value, float* grad /* nullable, overwritten */, void* stream);
int nst_anchor_geometry(int* blocks, int* block_elems);

/* ---- The MRF style term (Li & Wand, CVPR 2016: CNNMRF, neural-doodle) --------------------------------------------------
 * Every 3x3 patch of a tapped map is pulled towards its nearest neighbour among the 3x3 patches of the same map of the
 * style.  For one pyramid level and one tapped map of index i in Vgg19.layer_names:
 *   F  = the map of the level image, NHWC, h x w x C;  Fs = the same map of the level's style image, hs x ws x C, through
 *        the network the job uses (its tap flavour, its pooling, its colour mode).
 * Patches.  A patch is the 3x3xC block around a centre (y, x).  Image patches: 1 <= y <= h-2, 1 <= x <= w-2, n = (h-2)(w-2)
 *   of them in row-major order.
 * Dictionary.  Style centres (1 + a s, 1 + b s), a, b >= 0 integers, as long as they stay <= hs-2 and <= ws-2; s = the style
 *   stride, 1..8.  Entry j = a nb + b; m = na nb entries, na = (hs-3)/s + 1 in integer division, nb likewise.
 * Match.  score(i, j) = <P_i, Q_j> rq_j, rq_j = (float)(1 / sqrt(|Q_j|^2 + epsilon)), the norm summed in double, epsilon > 0
 *   (default 1e-5).  nn(i) = the LOWEST j among the maximal scores.  |P_i| does not change the arg-max and is not formed
 *   (Li & Wand's normalised cross-correlation).  The products run in the f16x2 arithmetic of the convolutions: each operand
 *   cut into two scaled fp16 pieces, three fp16 MFMAs per product block, fp32 accumulation.
 * Value.  mrf_i = (float)((1 / (9 C n)) sum_i |P_i - Q_nn(i)|^2), differences and squares formed in double from the fp32
 *   maps, summed in a fixed two-stage order (not |P|^2 - 2 <P,Q> + |Q|^2).
 * Loss row.  A level with the term has the total (... + gamma tmp) + sum_i w_i mrf_i: added after the temporal term, in
 *   ascending map order, every product and sum rounded.  NST_LOSS_ROW stays 4.  The weights w_i are the term's own:
 *   style_weight does not scale it (as with the moment term).
 * Gradient, nn held fixed.  dF(y,x,c) = coef_i sum over dy, dx in {-1,0,1} whose patch centre (y-dy, x-dx) exists of
 *   (F(y,x,c) - Fs(cy+dy, cx+dx, c)), (cy, cx) the centre of Q_nn of that patch, coef_i = (float)((double)w_i 2 / (9 C n)).
 *   Gather form, taps in the order dy outer, dx inner, ascending; fp32, one rounding per operation.  It reaches the network
 *   as the addend of the launch below the map: on top of the content gradient when the map is the content map too, beside
 *   the Gram second source and its row bias when the map carries those.
 * Between the closure halves the forward half keeps nn (int32 per patch) and the value; the backward half reads nn and the
 *   maps.  No float atomic takes part: across workgroups the search combines by an integer atomicMax on a 64-bit key (the
 *   order-preserving bit pattern of the score above ~j), so a closure with the term is bitwise reproducible.
 *
 * nst_level_set_patches: the term of one level, data of one job like the anchor (not a setting).  style = device (C,hs,ws)
 *   image in the job's colour mode (C = 3, or 1 under NST_COLOR_LUMINANCE), NULL: clear the level's term.  weights[6] by
 *   map index.  The call runs the style image through the network up to the deepest weighted map, keeps the weighted maps,
 *   prepares their dictionaries (rq, the absmax record, and the PACKED operand: both fp16 pieces of every entry in the
 *   search kernel's operand order, nine times the entries' share of the map, counted by nst_ctx_bytes) and allocates nn
 *   and the value partials: a closure allocates nothing.  Life cycle of nst_level_set_anchor: waits for the context's
 *   work; drops a captured graph, an L-BFGS memo and a pending backward half; a refusal changes nothing;
 *   nst_job_configure drops the term with the levels; nst_job_set_taps, nst_job_set_pooling and nst_job_set_color drop it
 *   (the maps are the other network's).
 *   NST_E_ARG: level out of range; negative or non-finite weights or epsilon (epsilon must be > 0); stride outside 1..8; a
 *   positive weight on a map that is not a style map of the job; a map or style map below 3x3.
 *   NST_E_STATE: no configured job; an arithmetic mode other than f16x2; a guided level (nst_level_set_guidance on a level
 *   with the term refuses likewise); a context with use_graph (the term's launches are not captured).
 *   The stripe closure returns NST_E_STATE while its level carries the term.
 * nst_level_patches: the level's setting (all-zero weights: no term).
 * nst_job_patch_losses: out = device, levels x 6: the unweighted mrf_i of the last closure by map index (zeros: maps
 *   without the term and levels outside the last level mask).
 * nst_level_patch_matches: idx_out = device int32, (h-2)(w-2) of the map: the nn of the last closure.  NST_E_STATE: the map
 *   carries no term on the level.  Both readers of a level return NST_E_ARG for a level out of range.
 * nst_patch_match: the match alone.  f = device NHWC (h,w,C), fs = device NHWC (hs,ws,C), C = 64, 128, 256 or 512, both
 *   maps at least 3x3; idx_out (int32, n) and score_out (float, n), either nullable.  Reads no job state.  Synchronous.
 * nst_patch_term: value and gradient alone at the given idx (entries outside [0, m) are clamped): value_out (device
 *   scalar, nullable) = mrf; grad_out (nullable, overwritten, NHWC like f) = the gradient with the given coef.  Synchronous. */
int nst_level_set_patches(nst_ctx* ctx, int level, const float* style /* device (C,hs,ws), or NULL: clear */, int hs, int ws,
                          const float* weights /* 6, by map index */, int stride, double epsilon, void* stream);
int nst_level_patches(const nst_ctx* ctx, int level, float* weights /* 6 */, int* stride, double* epsilon);
int nst_job_patch_losses(nst_ctx* ctx, float* out /* device, levels x 6 */, void* stream);
int nst_level_patch_matches(nst_ctx* ctx, int level, int map, int* idx_out /* device */, void* stream);
int nst_patch_match(nst_ctx* ctx, const float* f, int h, int w, int C, const float* fs, int hs, int ws, int stride, double epsilon,
                    int* idx_out /* nullable */, float* score_out /* nullable */, void* stream);
int nst_patch_term(nst_ctx* ctx, const float* f, int h, int w, int C, const float* fs, int hs, int ws, int stride, const int* idx,
                   float coef, float* value_out /* nullable */, float* grad_out /* nullable */, void* stream);
/* ---- The MRF term under semantic maps (Champandard 2016, "Semantic Style Transfer and Turning Two-Bit Doodles into Fine
 * Artworks": neural-doodle) ---------------------------------------------------------------------------------------------
 * A pair of semantic maps steers the patch search of a level that carries the MRF term: a patch prefers style patches of
 * its own region.  Only nn changes; value and gradient of the term are the ones above, at the new nn.
 * Inputs of a level.  Content planes c: (R,h,w) at the level image's size; style planes s: (R,hs,ws) at the size of the style
 *   image given to nst_level_set_patches; 1 <= R <= NST_MAX_REGIONS; all plane values in [0,1]; a weight gamma >= 0.
 * Descriptors.  For a weighted map i both stacks are brought to the map's resolution by the map's network scale (0, 1, 2, 3, 3,
 *   4 by map index) steps of the 2x2 mean pool of nst_level_set_guidance (floor sizes, ((e00 + e01) + e10) + e11 times 1/4,
 *   fp32).  The descriptor of a patch centred at (y,x): a[r] = the sum of the nine taps of pooled plane r, in double, taps in
 *   row-major order; d = (float)(a / sqrt(sum_r a[r]^2 + epsilon)), in double, with the term's own epsilon; stored as four
 *   floats, entries r >= R zero.  Image patches get d_i, i over all n patches; dictionary entries get e_j at the dictionary's
 *   centres (1 + a s, 1 + b s); the padding entries of the last dictionary tile are zero.  (An R-vector, not Champandard's
 *   9R-channel concatenation: 4 multiply-adds per score in the epilogue instead of 36, and for piecewise-constant labels the
 *   two agree wherever a patch lies inside one region.)
 * Score.  T(i,j) = cos(i,j) + gamma <d_i, e_j>, cos(i,j) = <P_i,Q_j> rq_j rp_i, rp_i = (float)(1 / sqrt(|P_i|^2 + epsilon)),
 *   summed in double over the image map and recomputed in every closure (the map changes).  rp_i is new: the unguided score
 *   omits it because it does not change an arg-max over j; next to an additive term it does.  On the device, without
 *   contraction:
 *     feat = (((main + cross * 2^-11) * inv) * rq_j) * rp_i
 *     sem  = ((d0*e0 + d1*e1) + d2*e2) + d3*e3
 *     sc   = feat + gamma * sem + 0.f
 *   The key, the atomicMax, the lowest-j tie rule and bitwise reproducibility are those of the unguided search; nn(i) is the
 *   arg-max of T.
 * Value and gradient do not change: mrf_i = sum |P - Q_nn|^2 / (9 C n) and its gather-form gradient at fixed nn - the
 *   semantic planes are constants, and the matches are held fixed.
 * Off.  gamma = 0, R = 0 and null planes all clear the guidance; a level without guidance launches the kernels of the
 *   unguided term and computes the same bits.
 *
 * nst_level_set_patch_guidance: the guidance of one level's term.  Both plane stacks are checked and pooled on scratch; the
 *   descriptors of every weighted map and the buffer of rp stay with the level (counted by nst_ctx_bytes, credited back when
 *   cleared): a closure allocates nothing.  Life cycle of nst_level_set_patches: waits for the context's work; ends a captured
 *   graph, an L-BFGS memo and a pending backward half; a refusal changes nothing.  Whatever drops the level's term drops its
 *   guidance: nst_level_set_patches (again or cleared), nst_job_configure, nst_job_set_taps, nst_job_set_pooling,
 *   nst_job_set_color.  So the order is patches first.
 *   NST_E_ARG: level or R out of range; a negative or non-finite gamma; a plane value outside [0,1] or not finite (a region
 *   may be empty on either side: the mass rule of the guided Gram does not apply).
 *   NST_E_STATE: no configured job; guidance for a level that carries no MRF term.
 * nst_level_patch_guidance: R and gamma of the level (zeros: unguided), and the size (hs, ws) the style planes of the level
 *   must have: that of the style image of nst_level_set_patches (zeros: the level carries no term).  All outputs nullable.
 * nst_patch_descriptors: the descriptors alone.  planes = device (R,hm,wm) at the MAP's resolution, hm, wm >= 3; out = device
 *   (count,4), count = ((hm-3)/stride + 1)((wm-3)/stride + 1): stride 1 for image patches, the style stride for a dictionary.
 * nst_patch_match_guided: nst_patch_match plus R, d (n,4), e (m,4) and gamma (the descriptors are used as given: entries
 *   r >= R are the caller's zeros); score_out is T.  Both read no job state and are synchronous. */
int nst_level_set_patch_guidance(nst_ctx* ctx, int level, int R, const float* content_planes /* device (R,h,w) */,
                                 const float* style_planes /* device (R,hs,ws) */, float gamma, void* stream);
int nst_level_patch_guidance(const nst_ctx* ctx, int level, int* R, float* gamma, int* hs, int* ws);
int nst_patch_descriptors(nst_ctx* ctx, const float* planes /* device (R,hm,wm) */, int R, int hm, int wm, int stride, double epsilon,
                          float* out /* device (count,4) */, void* stream);
int nst_patch_match_guided(nst_ctx* ctx, const float* f, int h, int w, int C, const float* fs, int hs, int ws, int stride,
                           double epsilon, int R, const float* d /* device (n,4) */, const float* e /* device (m,4) */, float gamma,
                           int* idx_out /* nullable */, float* score_out /* nullable */, void* stream);
/* ---- The histogram loss (Risser, Wilmot & Barnes 2017, "Stable and Controllable Neural Texture Synthesis and Style Transfer
 * Using Histogram Losses") ------------------------------------------------------------------------------------------------
 * Every channel of a tapped map is remapped so that its histogram becomes the style's, and the map is pulled towards its
 * remap.  For one pyramid level and one tapped map of index i in Vgg19.layer_names:
 *   F  = the map of the level image, NHWC, N = h w pixels by C channels, fp32;  Fs = the same map of the level's style image
 *        (Ns pixels), through the network the job uses (its tap flavour, its pooling, its colour mode);  B = the number of
 *        bins, 2..1024, default 256.
 * Range.  lo_c = min_p F[p,c], hi_c = max_p F[p,c], exact (-0 counts as +0).  A channel with hi_c == lo_c is FLAT and has no
 *   term: value 0, gradient 0, no counts.
 * Bin.  scale_c = (float)((double)B / ((double)hi_c - (double)lo_c));  x = (v - lo_c) scale_c in fp32, the subtraction and
 *   the product each rounded once;  b = min(B-1, (int)x);  f = min(1, x - (float)b);  counts[c][b] is uint32.
 * Style side.  slo, shi and scounts likewise from Fs with its own range, once, in the setter.  The style's maps are not
 *   kept: per map only C (B + 2) numbers are.
 * Table.  Every non-empty image bin gets two ends.  Per channel cum_b = sum_{b'<b} counts[b'] and scum_j likewise (uint64),
 *   width = ((double)shi - (double)slo) / B.
 *   start_b: the smallest j with scounts[j] > 0 and scum_{j+1} N > cum_b Ns;  t = (cum_b Ns - scum_j N) / (scounts[j] N), the
 *     products compared and subtracted as 64-bit integers, the quotient in double;  start_b = (float)(slo + (j + t) width).
 *   end_b: the same with cum_{b+1} and >= in place of >.
 *   A style channel with shi == slo has start = end = slo.  Empty image bins are never read (their ends are stored as zeros).
 *   Two ends, not one knot per bin edge: a non-empty bin that follows empty bins would otherwise start at the wrong end of the
 *   flat piece of the style's inverse CDF.  With two ends a map remapped onto its own histogram comes back, the remap is
 *   monotone per channel and stays inside [slo, shi].
 * Remap.  R(v) = start_b + f (end_b - start_b), fp32, three roundings.
 * Value.  hist_i = (float)((1 / (C N)) sum (F - R)^2), differences and squares formed in double from the fp32 numbers, summed
 *   in a fixed two-stage order.
 * Gradient, R held fixed.  dF = coef (F - R), coef = (float)(2 w_i / (C N)) formed in double; fp32, one rounding per
 *   operation.  It reaches the network as the addend of the launch below the map: after the content gradient and after the
 *   MRF term's addend where the map has those, beside the Gram second source and its row bias.  The launch's ReLU mask then
 *   applies as to any addend.
 * Loss row.  A level with the term has the total (... + sum_i w_i mrf_i) + sum_i w_i hist_i: added after the MRF term, in
 *   ascending map order, every product and sum rounded.  NST_LOSS_ROW stays 4.  The weights are the term's own:
 *   style_weight does not scale it.
 * Determinism.  No float atomic takes part: range and counts combine across workgroups by integer atomics only (the range on
 *   the order-preserving bit pattern the MRF keys use), the value by fixed-order double partials.  A closure with the term is
 *   bitwise reproducible.  Everything above is reproducible from the map's bits.
 * The term runs in all three arithmetic modes: the addend is the walkers' own.
 *
 * nst_level_set_histograms: the term of one level, data of one job like the MRF term.  style = device (C,hs,ws) image in the
 *   job's colour mode, NULL: clear the level's term.  weights[6] by map index.  The call runs the style image through the
 *   network up to the deepest weighted map, keeps range and counts of the weighted maps and allocates the image side (range,
 *   counts, tables, value partials): a closure allocates nothing.  Life cycle of nst_level_set_patches: waits for the
 *   context's work; drops a captured graph, an L-BFGS memo and a pending backward half; a refusal changes nothing;
 *   nst_job_configure drops the term with the levels; nst_job_set_taps, nst_job_set_pooling and nst_job_set_color drop it.
 *   NST_E_ARG: level out of range; bins outside 2..1024; negative or non-finite weights; a positive weight on a map that is
 *   not a style map of the job.
 *   NST_E_STATE: no configured job; a guided level (nst_level_set_guidance on a level with the term refuses likewise); a
 *   context with use_graph.  The stripe closure returns NST_E_STATE while its level carries the term.
 * nst_level_histograms: the level's setting (all-zero weights: no term).
 * nst_job_histogram_losses: out = device, levels x 6: the unweighted hist_i of the last closure by map index (zeros: maps
 *   without the term and levels outside the last level mask).
 * nst_level_histogram_tables: the image side of the last closure of one weighted map: lo_hi (C x 2 floats), counts (C x B
 *   uint32), ends (C x B x 2 floats), each nullable; zeros before any closure.  nst_level_histogram_style: the style's record.
 *   NST_E_STATE: the map carries no term on the level.  NST_E_ARG: a level or map out of range.
 * nst_histogram_counts, nst_histogram_tables, nst_histogram_term: the pieces alone, on NHWC device maps of C = 64, 128, 256 or
 *   512 channels (else NST_E_ARG) with N C < 2^31.  They read no job state.  Synchronous.  nst_histogram_term: value_out
 *   (device scalar, nullable) = hist; grad_out (nullable, overwritten, NHWC like f) = the gradient with the given coef. */
int nst_level_set_histograms(nst_ctx* ctx, int level, const float* style /* device (C,hs,ws), or NULL: clear */, int hs, int ws,
                             const float* weights /* 6, by map index */, int bins, void* stream);
int nst_level_histograms(const nst_ctx* ctx, int level, float* weights /* 6 */, int* bins);
int nst_job_histogram_losses(nst_ctx* ctx, float* out /* device, levels x 6 */, void* stream);
int nst_level_histogram_tables(nst_ctx* ctx, int level, int map, float* lo_hi /* C x 2 */, unsigned* counts /* C x B */,
                               float* ends /* C x B x 2 */, void* stream);
int nst_level_histogram_style(nst_ctx* ctx, int level, int map, float* lo_hi /* C x 2 */, unsigned* counts /* C x B */, void* stream);
int nst_histogram_counts(nst_ctx* ctx, const float* f, long long N, int C, int bins, float* lo_hi_out, unsigned* counts_out, void* stream);
int nst_histogram_tables(nst_ctx* ctx, const float* lo_hi, const unsigned* counts, long long N, const float* s_lo_hi,
                         const unsigned* s_counts, long long Ns, int C, int bins, float* ends_out, void* stream);
int nst_histogram_term(nst_ctx* ctx, const float* f, long long N, int C, int bins, const float* lo_hi, const float* ends, float coef,
                       float* value_out /* nullable */, float* grad_out /* nullable */, void* stream);
/* ---- The relaxed EMD style term (Kolkin, Salavon & Shakhnarovich 2019, "Style Transfer by Relaxed Optimal Transport and
 * Self-Similarity", STROTSS) ----------------------------------------------------------------------------------------------------
 * Two-way nearest-neighbour matching of feature vectors: every image vector must have a close style vector (side A), every
 * style vector a close image vector (side B), and the term is the larger of the two mean cosine distances.  For one pyramid
 * level and one tapped map of index i in Vgg19.layer_names:
 *   F  = the map of the level image, NHWC, h x w x C;  Fs = the same map of the level's style image, hs x ws x C, through the
 *        network the job uses (its tap flavour, its pooling, its colour mode);  C = 64, 128, 256 or 512.
 * Samples.  The image stride si and the style stride ss are integers in 1..256.  The image samples X_i, n of them, are the
 *   pixels (a si, b si), a = 0..(h-1)/si, b = 0..(w-1)/si (integer division), in row-major order; the style samples Y_j, m of
 *   them, likewise with ss.
 * Norms.  rp_i = (float)(1 / sqrt(|X_i|^2 + epsilon)), rq_j likewise for Y_j; epsilon > 0 (default 1e-5).  The squares are
 *   formed and summed in double: a wave per sample, lane l adds the squares of its 16-byte channel runs l, l + 64, ... in
 *   ascending order, the 64 lanes by the xor tree (offsets 32, 16, .., 1).
 * Matches.  c(i,j) = <X_i, Y_j> rp_i rq_j in the f16x2 arithmetic of the convolutions: each side's samples are scaled by the
 *   power of two of its map's absmax record and cut into a hi and a lo fp16 piece as in the MRF search; per 16 channels, in
 *   ascending order, the MFMA accumulates lo_d hi_c, hi_d hi_c, hi_d lo_c (d: the dictionary side, c: the column side) into a
 *   main (hi hi) and a cross accumulator; then c = (((main + cross 2^-11) inv) r_d) r_c + 0, every operation rounded in fp32,
 *   inv the product of the two inverse scales.  In direction A the style is the dictionary and the image the columns, in
 *   direction B the image is the dictionary: the same kernel twice, so r_d is rq in A and rp in B.
 *   nnA(i) = the lowest j among the maxima of c(i, .);  nnB(j) = the lowest i among the maxima of c(., j).  Scores of -0 count
 *   as +0.  An all-zero sample has every score +0 and so the match 0.
 * Value, formed in double from the fp32 maps at the matches, not from the search's scores.
 *   a_i = <X_i, Y_nnA(i)> / sqrt((|X_i|^2 + eps)(|Y_nnA(i)|^2 + eps));  b_j = the same expression at (nnB(j), j).  The three
 *   sums of one pair run over the channels in the order of the norms.  rA = 1 - (1/n) sum a_i, rB = 1 - (1/m) sum b_j, both sums
 *   in a fixed two-stage order (256 blocks of consecutive samples, four waves a block each taking every fourth sample, the waves
 *   in wave order; then the 256 partials by a tree).  remd_i = (float)max(rA, rB).  The active side is A when rA >= rB, else B.
 * Loss row.  A level with the term has the total (... + sum_i w_i hist_i) + sum_i w_i remd_i: added after the histogram term, in
 *   ascending map order, every product and sum rounded.  NST_LOSS_ROW stays 4.  The weights are the term's own: style_weight
 *   does not scale it.
 * Gradient of the active side, exact wherever the matches and the side are locally constant.  It reaches sampled pixels only.
 *   d(i,j) = rp_i ((cos rp_i) X_i - rq_j Y_j) with cos the stored (float)a_i (side A) or (float)b_j (side B), computed as
 *   t = cos rp_i; u = t X_i; v = rq_j Y_j; d = (u - v) rp_i.
 *   side A: dX_i = (float)(w/n) d(i, nnA(i));  side B: dX_i = (float)(w/m) sum over the j with nnB(j) = i, in ascending j, of
 *   d(i,j), the sum starting from +0.  fp32, contraction off, the coefficients formed in double.  It joins the addend of the
 *   launch below the map, after the content gradient, the MRF term's and the histogram term's where the map has those; at the
 *   top of the chain it is the addend of the 1x1 Gram launch, as for the MRF term.  The side flag is read on the device.
 * Determinism.  No float atomic takes part.  Across workgroups the searches combine by the integer atomicMax on the 64-bit key
 *   (score bits above ~index); side B's sum is formed in ascending j.  A closure with the term is bitwise reproducible.
 *
 * nst_level_set_remd: the term of one level, data of one job like the MRF term.  style = device (C,hs,ws) image in the job's
 *   colour mode, NULL: clear the level's term.  weights[6], image_stride[6], style_stride[6] by map index (all six stride pairs
 *   are checked).  The call runs the style image through the network up to the deepest weighted map, keeps the weighted maps
 *   with their absmax record, rq and packed operand, and allocates everything a closure needs.  Life cycle of
 *   nst_level_set_patches: waits for the context's work; drops a captured graph, an L-BFGS memo and a pending backward half; a
 *   refusal changes nothing; nst_job_configure drops the term with the levels; nst_job_set_taps, nst_job_set_pooling and
 *   nst_job_set_color drop it.
 *   NST_E_ARG: level out of range; negative or non-finite weights; epsilon <= 0 or not finite; a stride outside 1..256; a
 *   positive weight on a map that is not a style map of the job.
 *   NST_E_STATE: no configured job; an arithmetic mode other than f16x2; a guided level (nst_level_set_guidance on a level with
 *   the term refuses likewise); a context with use_graph.  The stripe closure returns NST_E_STATE while its level carries the
 *   term.
 * nst_level_remd: the level's setting (all-zero weights: no term; hs, ws: the size of the style image the setter was given);
 *   every output is nullable.
 * nst_job_remd_losses: out = device, levels x 6: the unweighted remd_i of the last closure by map index (zeros: maps without the
 *   term and levels outside the last level mask).
 * nst_level_remd_matches: nnA (n int32), nnB (m int32) and the side (one int32: 0 = A, 1 = B) of the last closure of one weighted
 *   map, device pointers, each nullable; zeros before any closure.  NST_E_STATE: the map carries no term on the level.
 * nst_remd_match, nst_remd_term: the pieces alone, on NHWC device maps.  They read no job state.  Synchronous.
 *   nst_remd_term: the value and the gradient at given matches.  side = 0 / 1 takes that side whatever the values (remd is then
 *   that side's r), -1 decides.  coef is the weight w of the definition.  value_out = device, 3 floats (remd, rA, rB); side_out =
 *   device int32; grad_out = NHWC like f, overwritten (zero off the sample grid); each nullable. */
int nst_level_set_remd(nst_ctx* ctx, int level, const float* style /* device (C,hs,ws), or NULL: clear */, int hs, int ws,
                       const float* weights /* 6, by map index */, const int* image_stride /* 6 */, const int* style_stride /* 6 */,
                       double epsilon, void* stream);
int nst_level_remd(const nst_ctx* ctx, int level, float* weights /* 6 */, int* image_stride /* 6 */, int* style_stride /* 6 */,
                   double* epsilon, int* hs, int* ws);
int nst_job_remd_losses(nst_ctx* ctx, float* out /* device, levels x 6 */, void* stream);
int nst_level_remd_matches(nst_ctx* ctx, int level, int map, int* nnA_out, int* nnB_out, int* side_out, void* stream);
int nst_remd_match(nst_ctx* ctx, const float* f, int h, int w, int C, const float* fs, int hs, int ws, int si, int ss, double epsilon,
                   int* nnA_out /* n */, int* nnB_out /* m */, void* stream);
int nst_remd_term(nst_ctx* ctx, const float* f, int h, int w, int C, const float* fs, int hs, int ws, int si, int ss, double epsilon,
                  const int* nnA, const int* nnB, int side, float coef, float* value_out /* 3, nullable */, int* side_out /* nullable */,
                  float* grad_out /* nullable */, void* stream);
/* ---- The self-similarity content term (the content half of Kolkin, Salavon & Shakhnarovich 2019, STROTSS) -------------------
 * The pattern of pairwise cosine distances between sampled positions of the image must be the content's; the feature vectors
 * themselves may become anything.  For one pyramid level and one tapped map of index k in Vgg19.layer_names - any map the job
 * uses, its content map or a style map:
 *   F  = the map of the level image, NHWC, h x w x C;  Fc = the same map of the level's content image, the same size, through
 *        the network the job uses (its tap flavour, its pooling, its colour mode);  C = 64, 128, 256 or 512.
 * Samples.  One stride s in 1..256 per map.  The image samples X_i, i = 0..n-1, are the pixels (a s, b s), a = 0..(h-1)/s,
 *   b = 0..(w-1)/s (integer division), in row-major order - the relaxed EMD term's rule; the content samples Z_i are the same
 *   pixels of Fc.  n <= 4096 (the term keeps n x n arrays): a stride that leaves more is refused.
 * Norms.  rp_i = (float)(1 / sqrt(|X_i|^2 + epsilon)), formed as the relaxed EMD term forms it (double, the same lane and tree
 *   order); epsilon > 0 (default 1e-5).
 * Distances.  c(i,j) = <X_i, X_j> rp_i rp_j in the f16x2 arithmetic, exactly the relaxed EMD search's product with the sample set
 *   on both sides under the one absmax record of the map: i in the dictionary role (the packed operand), j in the column role,
 *   per 16 channels in ascending order lo_i hi_j, hi_i hi_j, hi_i lo_j into the main and the cross accumulator, then
 *   c = (((main + cross 2^-11) inv) rp_i) rp_j + 0, every operation rounded in fp32, inv the square of the inverse scale.
 *   D_ii = 0;  D_ij = max(0, 1 - c(i,j)) otherwise (fp32).  D is used as computed: the two roles accumulate their cross pieces
 *   in different orders, so D_ij and D_ji need not share bits.
 * Column normalisation.  s_j = sum_i D_ij in double, in two ordered stages: 16 row blocks of ceil(n / 16) consecutive rows; in
 *   a block four partial sums, the v-th over the block's rows v, v + 4, ... in ascending order, joined ((p0 + p1) + p2) + p3;
 *   then the 16 blocks in ascending order, starting from +0.  q_j = 1 / (s_j + epsilon) (double);  N_ij = D_ij q_j (double).
 *   M is the same thing for the content samples: the setter makes it once by the same launches (it keeps the content's D and
 *   q), so an image whose maps equal the content's bit for bit has N = M bit for bit.
 * Value.  selfsim_k = (float)((1/n) sum_ij |N_ij - M_ij|): the mean over the columns of the L1 distance between two
 *   distributions, which lies in [0, 2] whatever n is - hence the factor 1/n and not the paper's printed 1/n^2, under which
 *   the term would shrink with the sample count.  The sum in double: per column and row block as for s_j, per column the 16
 *   blocks in ascending order, then thread u of 256 the columns u, u + 256, ... in ascending order and the 256 threads by a
 *   tree.  n = 1 gives 0.  A map equal to the content's bit for bit gives exactly 0, constant and all-zero maps included; two
 *   different constant maps need not (epsilon sits in the norms and in the column sums), only a finite value in [0, 2].
 * Decisions.  sg_ij = sign(N_ij - M_ij) in {-1, 0, +1}, evaluated on the doubles above and kept as int8; and the clamp: an
 *   off-diagonal entry with D_ij = 0 passes no gradient.
 * Gradient, exact wherever the decisions are locally constant.  It reaches sampled pixels only.
 *   t_j = sum_i sg_ij N_ij (double, in the order of s_j);  E_ij = (sg_ij - t_j) q_j (double), 0 on the diagonal and at clamped
 *   entries;  W_ij = (float)(E_ij + E_ji);  u_j = rp_j X_j (fp32, one rounding);  g_i = -sum_j W_ij u_j on
 *   v_mfma_f32_32x32x2_f32 with j ascending from a zero accumulator;  <g_i, u_i> in double (per 32 channels the xor tree with
 *   offsets 16 .. 1, the 32-channel blocks in ascending order);  dX_i = ((g_i - (float)<g_i, u_i> u_i) rp_i) (float)(w / n),
 *   fp32, contraction off, the coefficient formed in double.  It joins the addend of the launch below the map after the
 *   content gradient and the MRF, histogram and relaxed EMD terms' gradients; at the top of the chain it is the addend of the
 *   1x1 Gram launch, or, on a content map that is no style map, of the mask pass.
 * Loss row.  A level with the term has the total (... + sum_i w_i remd_i) + sum_k w_k selfsim_k: added after the relaxed EMD
 *   term, in ascending map order, every product and sum rounded.  NST_LOSS_ROW stays 4.  The weights are the term's own:
 *   content_weight does not scale it.
 * Determinism.  No atomic takes part; every reduction has one owner and a fixed order.  A closure with the term is bitwise
 *   reproducible.
 *
 * nst_level_set_selfsim: the term of one level, data of one job like the relaxed EMD term.  content = device (C,h,w) image in
 *   the job's colour mode, of the level's size, NULL: clear the level's term.  weights[6], stride[6] by map index (all six
 *   strides are checked).  The call runs the content image through the network up to the deepest weighted map, keeps per
 *   weighted map the content's D and q, and allocates everything a closure needs.  Life cycle of nst_level_set_remd.
 *   NST_E_ARG: level out of range; negative or non-finite weights; epsilon <= 0 or not finite; a stride outside 1..256; a
 *   size other than the level's; a positive weight on a map the job does not use (neither its content map nor a style map);
 *   more than 4096 samples on a weighted map.
 *   NST_E_STATE: no configured job; an arithmetic mode other than f16x2; a guided level (nst_level_set_guidance on a level with
 *   the term refuses likewise); a context with use_graph.  The stripe closure returns NST_E_STATE while its level carries the
 *   term.
 * nst_level_selfsim: the level's setting (all-zero weights: no term); every output is nullable.
 * nst_job_selfsim_losses: out = device, levels x 6: the unweighted selfsim_k of the last closure by map index (zeros: maps
 *   without the term and levels outside the last level mask).
 * nst_level_selfsim_decisions: the last closure's D (n x n float), s (n double) and sg (n x n int8) of one weighted map,
 *   device pointers, each nullable; zeros before any closure.  NST_E_STATE: the map carries no term on the level.
 * nst_selfsim_matrix, nst_selfsim_term: the pieces alone, on NHWC device maps.  They read no job state.  Synchronous.
 *   nst_selfsim_term: f against fc (both h x w x C).  coef is the weight w of the definition.  value_out = device float;
 *   sg_out = device, n x n int8; grad_out = NHWC like f, overwritten (zero off the sample grid); each nullable. */
int nst_level_set_selfsim(nst_ctx* ctx, int level, const float* content /* device (C,h,w), or NULL: clear */, int h, int w,
                          const float* weights /* 6, by map index */, const int* stride /* 6 */, double epsilon, void* stream);
int nst_level_selfsim(const nst_ctx* ctx, int level, float* weights /* 6 */, int* stride /* 6 */, double* epsilon);
int nst_job_selfsim_losses(nst_ctx* ctx, float* out /* device, levels x 6 */, void* stream);
int nst_level_selfsim_decisions(nst_ctx* ctx, int level, int map, float* D_out, double* s_out, signed char* sg_out, void* stream);
int nst_selfsim_matrix(nst_ctx* ctx, const float* f, int h, int w, int C, int stride, double epsilon, float* D_out /* n x n, nullable */,
                       double* s_out /* n, nullable */, void* stream);
int nst_selfsim_term(nst_ctx* ctx, const float* f, const float* fc, int h, int w, int C, int stride, double epsilon, float coef,
                     float* value_out /* nullable */, signed char* sg_out /* nullable */, float* grad_out /* nullable */, void* stream);
/* ---- The long-range style term, "xcorr": Gram matrices of spatially shifted maps (Berger & Memisevic, ICLR 2017) ---------------
 * Every summed style statistic is blind to arrangement; this one is not: the cross-correlation of a map with a shifted copy of
 * itself carries a texture's regular structure (a lattice, hatching at a fixed pitch).  ("Gram shift" is the activation shift of
 * nst_job_set_gram_shift; this term is called xcorr everywhere.)  For one pyramid level, one style map of index i in
 * Vgg19.layer_names and one shift d = (dx, dy), dx, dy >= 0, not both 0, dx < w, dy < h:
 *   F = the map of the level image, NHWC, h x w x C, the raw map whatever gram_shift is;  C = 64, 128, 256 or 512.
 *   G_d[c][e] = (1/Z_d) sum over y < h - dy, x < w - dx of F(y + dy, x + dx)[c] F(y, x)[e];   Z_d = C (h - dy)(w - dx): the Gram
 *     divisor with the pair count in place of the pixel count.  G_d is not symmetric.  A pixel at x >= w - dx is never paired
 *     with the next row's.
 *   Gt_d = the same statistic of the same map of the level's style image, which has its own size and hence its own Z_d.
 * Per map.  xcorr_i = (1/|D|) sum_d mean_{c,e} (G_d - Gt_d)^2 over the level's shift list D (1..16 distinct shifts, each
 *   component 0..64): the MEAN over the shifts, not the paper's sum, so that a weight means the same whatever the list is.
 * Arithmetic.  G_d in the f16x2 arithmetic of the Gram pass: both operands are windows of the same map under its one recorded
 *   absmax, two fp16 pieces each, per 16 pairs lo hi, hi hi, hi lo into a main and a cross accumulator (three
 *   v_mfma_f32_32x32x16_f16 per 32x32x16 block), joined as (main + cross 2^-11) inv^2.  The pairs are dealt to nsplit slabs of
 *   pix_per_split consecutive pixels p = y w + x < (h - dy) w - dx (whole chunks of 32; a function of the shape alone, which
 *   nst_xcorr reports); the slabs are added in slab order, then divided by (float)Z_d.  The value: (G_d - Gt_d)^2 in double,
 *   1024 consecutive elements a block joined by a fixed tree, the blocks of a shift likewise, the shifts in ascending order;
 *   xcorr_i = (float) of that.
 * Gradient.  S_d = (float)(2 w_i / (|D| C^2 Z_d)) (G_d - Gt_d), the coefficient formed in double;
 *   dF(q) = sum_d ( [x >= dx, y >= dy] F(q - d) S_d^T + [x < w - dx, y < h - dy] F(q + d) S_d )
 *   on v_mfma_f32_32x32x2_f32 with fp32 operands: per pixel and channel one chain over the shifts in list order, per shift the
 *   F(q - d) part before the F(q + d) part, channels ascending.  It joins the addend of the launch below the map after the
 *   self-similarity term's gradient: written unless an addend is held already, else added.
 * Loss row.  A level with the term has the total (... + sum_k w_k selfsim_k) + sum_i w_i xcorr_i: added after the
 *   self-similarity term, in ascending map order, every product and sum rounded.  NST_LOSS_ROW stays 4.  The weights are the
 *   term's own: style_weight and style_layer_weights do not scale it.
 * Determinism.  No float atomic takes part; every reduction has one owner and a fixed order.  A closure with the term is bitwise
 *   reproducible.
 *
 * nst_level_set_xcorr: the term of one level, data of one job like the relaxed EMD term.  style = device (C,hs,ws) image in the
 *   job's colour mode, NULL: clear the level's term.  weights[6] by map index; shifts = host, n x 2 ints (dx, dy), the same for
 *   every map of the level.  The call runs the style image through the network up to the deepest weighted map, keeps per
 *   weighted map the style's G_d stack, and allocates everything a closure needs.  Life cycle of nst_level_set_remd.
 *   NST_E_ARG: level out of range; negative or non-finite weights; n outside 1..16; a shift component outside 0..64, a (0,0)
 *   shift or a repeated one; a shift that is not smaller than a weighted map of the level or of the style image; a style image
 *   below 16x16; a positive weight on a map that is not a style map of the job.
 *   NST_E_STATE: no configured job; an arithmetic mode other than f16x2; a guided level (nst_level_set_guidance on a level with
 *   the term refuses likewise); a context with use_graph.  The stripe closure returns NST_E_STATE while its level carries the
 *   term.
 * nst_level_xcorr: the level's setting (all-zero weights: no term); shifts takes 16 x 2 ints; every output is nullable.
 * nst_job_xcorr_losses: out = device, levels x 6: the unweighted xcorr_i of the last closure by map index (zeros: maps without
 *   the term and levels outside the last level mask).
 * nst_level_xcorr_matrices: the last closure's G_d stack (|D| x C x C floats, device) of one weighted map; zeros before any
 *   closure.  NST_E_STATE: the map carries no term on the level.
 * nst_xcorr, nst_xcorr_term: the pieces alone, on an NHWC device map.  They read no job state.  Synchronous.
 *   nst_xcorr: out = device, n x C x C; geometry_out = host, n x 2 ints (nsplit, pix_per_split) per shift, nullable.
 *   nst_xcorr_term: f against the targets gt (device, n x C x C).  coef is the weight w of the definition.  value_out = device
 *   float (the unweighted xcorr); grad_out = NHWC like f, overwritten; each nullable. */
int nst_level_set_xcorr(nst_ctx* ctx, int level, const float* style /* device (C,hs,ws), or NULL: clear */, int hs, int ws,
                        const float* weights /* 6, by map index */, const int* shifts /* host, n x 2 */, int n, void* stream);
int nst_level_xcorr(const nst_ctx* ctx, int level, float* weights /* 6 */, int* shifts /* 16 x 2 */, int* n, int* hs, int* ws);
int nst_job_xcorr_losses(nst_ctx* ctx, float* out /* device, levels x 6 */, void* stream);
int nst_level_xcorr_matrices(nst_ctx* ctx, int level, int map, float* G_out /* device, |D| x C x C */, void* stream);
int nst_xcorr(nst_ctx* ctx, const float* f, int h, int w, int C, const int* shifts /* host, n x 2 */, int n, float* out /* n x C x C */,
              int* geometry_out /* host, n x 2, nullable */, void* stream);
int nst_xcorr_term(nst_ctx* ctx, const float* f, int h, int w, int C, const float* gt /* n x C x C */, const int* shifts /* host, n x 2 */,
                   int n, float coef, float* value_out /* nullable */, float* grad_out /* nullable */, void* stream);
int nst_warp_bilinear(nst_ctx* ctx, const float* src, const float* flow, int C, int h, int w, float* out,
                      float* valid /* nullable */, void* stream);
int nst_flow_weights(nst_ctx* ctx, const float* fwd, const float* bwd, int h, int w, float* out, void* stream);
/* Optical flow for a sequence whose caller has none: multi-scale Horn-Schunck with warping - Horn & Schunck, "Determining
 * Optical Flow" (1981) in the coarse-to-fine form of Meinhardt-Llopis, Sanchez & Kondermann, "Horn-Schunck Optical Flow with a
 * Multi-Scale Strategy" (IPOL 2013).  A baseline estimator: flows from a better one are handed to the warp as before.
 * Convention: estimate(from, to) gives w = (u, v) on the grid of `from` with from(p) ~ to(p + w(p)) - the convention of
 *   nst_warp_bilinear, out(p) = src(p + flow(p)).  The backward flow of frame i is estimate(frame i, frame i-1), the forward
 *   flow estimate(frame i-1, frame i).  Images are single planes (h,w), fp32, on the scale of nst_luminance (255 Y).  A flow
 *   is (2,h,w): plane 0 = u (x), plane 1 = v (y), in pixels.
 * Everything is fp32, every operation rounded once (no contraction), divisions correctly rounded; nothing is reduced and
 * nothing is added atomically: the same bits on every run.  The stages, with their order of operations:
 * reduce (nst_flow_reduce): (h,w) -> (hc,wc) = ((h+1)/2, (w+1)/2).  With k = (1, 4, 6, 4, 1)/16 (exact) and indices clamped to
 *   the image: r(y', x) = sum_i k_i in(y', clamp(2x+i-2)) (the pass along a row first), out(y, x) = sum_j k_j r(clamp(2y+j-2), x);
 *   each pass forms its five products and adds them in index order, ((((p0 + p1) + p2) + p3) + p4).
 * prolong (nst_flow_prolong): coarse (2,hc,wc) -> fine (2,h,w), hc = (h+1)/2, wc = (w+1)/2.  Per axis a = i >> 1,
 *   b = min(a + (i & 1), nc - 1); r(Y, x) = 0.5 (c(Y, a_x) + c(Y, b_x)) (along a row first), m = 0.5 (r(a_y, x) + r(b_y, x)),
 *   out = 2 m: a displacement doubles with the grid.
 * gradient: Bx = 0.5 (B(x+1) - B(x-1)), By likewise in y, B = `to` at the scale, replicated borders - the expression of the
 *   motion-boundary test of nst_flow_weights.
 * linearise (nst_flow_linearize) at the flow (u, v): the sample position of pixel p is p + (u, v)(p) by the position rule of
 *   the warp (integer part and fraction of the flow alone; four taps; "inside" = the warp's valid).  Bw, Ix, Iy = the bilinear
 *   samples of B, Bx, By in the warp's order of operations.  Inside: rho = ((Bw - Ix u) - Iy v) - A, A = `from`.  Elsewhere, and
 *   where the flow is not finite: Ix = Iy = rho = 0 - such a pixel has no data term and only diffuses.
 * sweep (nst_flow_sweeps): one Jacobi step, both new planes from the old ones.  With replicated borders
 *   u~ = (((N + S) + W) + E) / 6 + (((NW + NE) + SW) + SE) / 12, v~ likewise;
 *   t = ((rho + Ix u~) + Iy v~) / ((alpha^2 + Ix Ix) + Iy Iy), alpha^2 = the fp32 product alpha alpha;
 *   u' = u~ - Ix t, v' = v~ - Iy t.
 * driver (nst_flow_estimate): pyramids of both planes by reduce; scale s+1 exists while min(hc, wc) >= 8 for its size and
 *   s+1 < scales (scales = 0: as many as fit, at most NST_MAX_FLOW_SCALES); the flow is zero at the coarsest scale; per
 *   scale, `warps` times: linearise at the current flow, then `iterations` sweeps that start from it; then prolong to the
 *   next finer scale.  alpha is the same at every scale.  IPOL's defaults: alpha = 15 (images in 0 ... 255), warps = 5,
 *   iterations = 50 here, scales = 0.
 *
 * The CALLER supplies every buffer; the context allocates nothing and nst_ctx_bytes does not move.  All of these read no
 * job state and are synchronous.
 * nst_flow_workspace: pure (no context, no device).  floats = what nst_flow_estimate needs for (h, w, scales) (reduced
 *   planes of both images, Ix, Iy, rho, a second flow buffer); scales_used by the rule above.  Either pointer may be NULL.
 *   NST_E_ARG: h or w < 1, scales < 0 or > NST_MAX_FLOW_SCALES.
 * nst_flow_estimate: from, to device (h,w); flow device (2,h,w), out; workspace device, workspace_floats floats.  NST_E_ARG,
 *   with nothing launched and `flow` untouched: a workspace smaller than nst_flow_workspace says, a null pointer, h or w < 1,
 *   alpha non-finite or <= 0, or whose fp32 square overflows or is subnormal (the sweep divides by it alone where a pixel has
 *   no data term), warps < 1,
 *   iterations < 1, scales < 0 or > NST_MAX_FLOW_SCALES; an output that overlaps another argument.
 * nst_flow_reduce: in (h,w) -> out ((h+1)/2,(w+1)/2).  nst_flow_prolong: coarse (2,(h+1)/2,(w+1)/2) -> fine (2,h,w).
 * nst_flow_linearize: from, to (h,w), flow (2,h,w) -> ix, iy, rho (h,w).
 * nst_flow_sweeps: n >= 1 sweeps, one launch each, from flow_in (2,h,w, left as it is); the sweeps alternate between
 *   flow_out and scratch (2,h,w each; scratch may be NULL for n = 1) so that the result is always in flow_out.  alpha as
 *   for nst_flow_estimate.
 * No stage runs in place (every kernel reads neighbouring pixels): an output that overlaps an input or another output is
 *   NST_E_ARG for each of these entry points.
 * 16-byte accesses of the sweep: a group of four pixels takes them where u', v', u, v, Ix, Iy and rho all lie on a 16-byte
 *   boundary there.  The planes of a (2,h,w) flow are h w floats apart, so a flow whose h w is not a multiple of 4 (odd
 *   pyramid scales among them) is swept with single floats throughout; the result is the same either way. */
int nst_flow_workspace(int h, int w, int scales, size_t* floats, int* scales_used);
int nst_flow_estimate(nst_ctx* ctx, const float* from, const float* to, int h, int w, float alpha, int scales, int warps,
                      int iterations, float* flow /* out (2,h,w) */, float* workspace, size_t workspace_floats, void* stream);
int nst_flow_reduce(nst_ctx* ctx, const float* in, int h, int w, float* out, void* stream);
int nst_flow_prolong(nst_ctx* ctx, const float* coarse, int h, int w, float* fine, void* stream);
int nst_flow_linearize(nst_ctx* ctx, const float* from, const float* to, const float* flow, int h, int w, float* ix, float* iy,
                       float* rho, void* stream);
int nst_flow_sweeps(nst_ctx* ctx, const float* ix, const float* iy, const float* rho, const float* flow_in, int h, int w,
                    float alpha, int n, float* flow_out, float* scratch /* nullable for n = 1 */, void* stream);
/* TV-L1 optical flow in its dual form - Zach, Pock & Bischof, "A Duality Based Approach for Realtime TV-L1 Optical Flow"
 * (DAGM 2007) as Sanchez, Meinhardt-Llopis & Facciolo state it, "TV-L1 Optical Flow Estimation" (IPOL 2013) - for flows that
 * stay sharp at motion boundaries, where the quadratic smoothness term of nst_flow_estimate blurs them.  The convention, the
 * planes, the pyramid (reduce, prolong, the scale rule min(hc, wc) >= 8 and NST_MAX_FLOW_SCALES, the zero flow at the coarsest
 * scale) and the linearisation are nst_flow_estimate's, unchanged: Ix, Iy, rho of nst_flow_linearize - rho is TV-L1's constant
 * part rho_c - with the inside flag and the non-finite rule (no data term: Ix = Iy = rho_c = 0).  There is no stopping test
 * and no median filter: either makes the result discontinuous in its inputs or dependent on the run.
 * Parameters: lambda (data weight, default 0.15), theta (coupling, 0.3), tau (dual step, 0.25), scales (0), warps (5),
 *   iterations (50).  Constants, fp32: lt = lambda theta, taut = tau / theta.
 * Per scale: the duals p11, p12 (of u) and p21, p22 (of v) start at zero and are kept across the warps of the scale; then
 *   `warps` times: linearise at the current flow, then `iterations` iterations; then prolong the flow to the next finer scale.
 * One iteration (nst_flow_tvl1_iterations), fp32, every written operation rounded once (no contraction), division and square
 *   root correctly rounded; g2 = Ix Ix + Iy Iy:
 *     r = (rho_c + Ix u) + Iy v;  b = lt g2
 *     k = lt if r < -b;  k = -lt if r > b;  otherwise k = (-r) / g2 if g2 >= 1e-10f, else k = 0
 *     v1 = u + k Ix,  v2 = v + k Iy
 *     u' = v1 + theta (dx(p11) + dy(p12)),  v' = v2 + theta (dx(p21) + dy(p22)), with the backward differences
 *       dx(p)(x) = p(x) - p(x-1), dy likewise along y, where p(-1) = 0 and the last column of p11, p21 and the last row of
 *       p12, p22 are READ AS 0 (they stay exactly 0 from a zero start; the stage reads them as 0 whatever the caller passed)
 *     ux = u'(x+1) - u'(x) (0 in the last column), uy = u'(y+1) - u'(y) (0 in the last row); vx, vy likewise
 *     n1 = 1 + taut sqrt(ux ux + uy uy);  p11' = (p11 + taut ux) / n1,  p12' = (p12 + taut uy) / n1 (p11, p12 as read above)
 *     n2 = 1 + taut sqrt(vx vx + vy vy);  p21' = (p21 + taut vx) / n2,  p22' = (p22 + taut vy) / n2
 *   The flow of the next iteration is (u', v').  Nothing is reduced and nothing is added atomically: the same bits on every run.
 * The CALLER supplies every buffer; the context allocates nothing and nst_ctx_bytes does not move.  Synchronous, no job state.
 * nst_flow_tvl1_workspace: pure.  floats = what nst_flow_tvl1_estimate needs: what nst_flow_workspace counts plus two copies
 *   of the duals, 4 h w floats each (an iteration is one launch that writes a second copy of the flow and of the duals).
 *   Either pointer may be NULL.  NST_E_ARG: h or w < 1, scales < 0 or > NST_MAX_FLOW_SCALES.
 * nst_flow_tvl1_estimate: from, to device (h,w); flow device (2,h,w), out; workspace device, workspace_floats floats.
 * nst_flow_tvl1_iterations: n >= 1 iterations from flow_in (2,h,w) and dual_in (4,h,w: p11, p12, p21, p22), both left as they
 *   are, under the linearisation ix, iy, rho (h,w); the result in flow_out (2,h,w) and dual_out (4,h,w); scratch: 6 h w floats
 *   the iterations alternate with, not touched (and may be NULL) for n = 1.
 * NST_E_ARG for both, with nothing launched and the outputs untouched: a workspace smaller than nst_flow_tvl1_workspace says;
 *   a null pointer; h or w < 1; lambda, theta or tau non-finite or <= 0; lt or taut not a normal fp32 number; warps,
 *   iterations or n < 1; scales < 0 or > NST_MAX_FLOW_SCALES; an output that overlaps another argument.
 * 16-byte accesses: as the sweep's, over the fifteen planes of an iteration; the planes of the duals too are h w floats
 *   apart, so with h w % 4 != 0 an iteration takes single floats throughout; the result is the same either way. */
int nst_flow_tvl1_workspace(int h, int w, int scales, size_t* floats, int* scales_used);
int nst_flow_tvl1_estimate(nst_ctx* ctx, const float* from, const float* to, int h, int w, float lambda, float theta, float tau,
                           int scales, int warps, int iterations, float* flow /* out (2,h,w) */, float* workspace,
                           size_t workspace_floats, void* stream);
int nst_flow_tvl1_iterations(nst_ctx* ctx, const float* ix, const float* iy, const float* rho, const float* flow_in,
                             const float* dual_in, int h, int w, float lambda, float theta, float tau, int n, float* flow_out,
                             float* dual_out, float* scratch /* nullable for n = 1 */, void* stream);
/* F.interpolate(x, size=(h//2,w//2), mode='bicubic') (neural_style_transfer.py:173-176) and its
 * transpose (autograd backward); x (C,h,w) -> y (C,h/2,w/2); gy -> gx (overwritten). */
int nst_bicubic_half(nst_ctx* ctx, const float* x, int C, int h, int w, float* y, void* stream);
int nst_bicubic_half_backward(nst_ctx* ctx, const float* gy, int C, int h, int w, float* gx, void* stream);
/* prepare_img / unprepare_img (neural_style_transfer.py:375-393): HWC [0,1] RGB <-> planar
 * prepared, both on the device. */
int nst_prepare_img(nst_ctx* ctx, const float* hwc, int h, int w, float* chw, void* stream);
int nst_unprepare_img(nst_ctx* ctx, const float* chw, int h, int w, float* hwc, void* stream);

/* ---- job set-up on the device (the host-side OpenCV work of the reference's job driver) ----------- */

/* cv2.resize(img, (nw, nh), interpolation=cv2.INTER_CUBIC) for float32 HWC images (bicubic, A = -0.75, half-pixel
 * centres, replicate border, no antialias) - `resize` (neural_style_transfer.py:211-226) and the noise-map
 * up-sampling (:304-305); src (h,w,channels) -> dst (nh,nw,channels), both on the device. */
int nst_resize_bicubic(nst_ctx* ctx, const float* src, int h, int w, int channels, float* dst, int nh, int nw, void* stream);
/* dst[i][:] = src[perm[i]][:]: the row shuffle of make_style_noise (:422-432) with the permutation drawn on the
 * host by np.random.permutation (so the reference's RNG stream is reproduced); perm: device int64[rows]. */
int nst_gather_rows(nst_ctx* ctx, const float* src, const long long* perm, size_t rows, int channels, float* dst, void* stream);
/* acc += (src ? src : 1) * gaussian_mask((h,w), central, peripheral, dispersion) (gaussian_mask :396-418 and the
 * accumulation at :283-284, :311-313); acc, src: device float32 (h,w,channels); mask evaluated in double. */
int nst_gaussian_mask_accumulate(nst_ctx* ctx, float* acc, const float* src, int h, int w, int channels, double central,
                                 double peripheral, double dispersion, void* stream);
/* out = ((1 - nr) * content + nr * noise).astype(float32), nr = 5 nf / (5 + GaussianBlur_101,0.2(clip(|Sobel_5|, 0, 100)))
 * computed in double (:331-343, :355-358); all (h,w,channels) device float32.  Synchronous. */
int nst_noise_blend(nst_ctx* ctx, const float* content, const float* noise, int h, int w, int channels, double noise_factor,
                    float* out, void* stream);
/* dst = alpha * src (init_method 'random': 0.5 * noise, :351) */
int nst_scale(nst_ctx* ctx, const float* src, float alpha, size_t n, float* dst, void* stream);

/* ---- colour preservation set-up (Gatys et al. 2016; nst_job_set_color) ------------------------------------------
 * Images are HWC float32 RGB in [0,1].  YIQ (NTSC): Y = 0.299 R + 0.587 G + 0.114 B, I = 0.595716 R - 0.274453 G
 * - 0.321263 B, Q = 0.211456 R - 0.522591 G + 0.311135 B; its inverse is the fp64 inverse of that matrix.
 * nst_color_stats: per-channel mean (3) and population covariance (3x3, row-major) over all pixels, fp64, to HOST memory
 *   (a device reduction with fp64 partials in a fixed order).  Synchronous.
 * nst_color_transfer_matrix (host only): A = Sigma_c^{1/2} Sigma_s^{-1/2} (symmetric square roots by a Jacobi eigen-
 *   decomposition in fp64; style eigenvalues clamped below at 1e-10), b = mu_c - A mu_s.  Host pointers; A row-major.
 * nst_color_affine: dst = A p + b per pixel (fp64 arithmetic, stored fp32, not clipped); A, b HOST doubles; in place allowed.
 * nst_luminance: out (1,h,w) = 255 (alpha Y(p) + beta) - the luminance image u of an RGB image (alpha = 1, beta = 0) or of
 *   a style image matched to the content's luminance mean and deviation.
 * nst_luminance_recombine: out HWC = YIQ^-1 (u / 255, I(content), Q(content)), not clipped: the RGB image of a luminance
 *   job (in place of nst_unprepare_img). */
int nst_color_stats(nst_ctx* ctx, const float* hwc, int h, int w, double* mean, double* cov, void* stream);
int nst_color_transfer_matrix(const double* mean_c, const double* cov_c, const double* mean_s, const double* cov_s, double* A,
                              double* b);
int nst_color_affine(nst_ctx* ctx, const float* src, int h, int w, const double* A, const double* b, float* dst, void* stream);
int nst_luminance(nst_ctx* ctx, const float* hwc, int h, int w, double alpha, double beta, float* out, void* stream);
int nst_luminance_recombine(nst_ctx* ctx, const float* u, const float* content, int h, int w, float* out, void* stream);

/* ---- spatial sharding of one pyramid level: a context evaluates a horizontal STRIPE of a larger image ------------
 * (SURVEY 8(e) partition B with halo recompute.  There is no counterpart in the reference; the quantities are those of
 * neural_style_transfer.py:84-112 restricted to the rows a rank owns.)
 * The context is configured with nst_job_configure(ctx, 1, ext_rows, W0) and its targets set with
 * nst_level_set_targets(ctx, 0, <the same rows of the content image>, <the whole style image>, ...).  Its image `xs`
 * (3, ext_rows, W0) is rows [e0, e0 + ext_rows) of the (3, H0, W0) image: the rows the rank owns,
 * [row0, row0 + rows) in stripe coordinates, plus a halo on each interior side that covers the receptive field of
 * relu5_1 (78 rows; 96 keeps the boundaries multiples of 16).  row0 and the boundaries between stripes are multiples
 * of 16 (pooling alignment); only the bottom stripe may own a ragged last row group.
 *   nst_window_begin: forward pass; writes to `sums` (nst_window_sums_count floats, device) the un-normalised Gram
 *     sums of the five style maps, the content sum of squares and the two TV sums OVER THE OWNED ROWS.
 *   The caller adds the `sums` of all stripes (one all-reduce).
 *   nst_window_end: turns the summed `sums` into the style / content / TV terms of the FULL image (its normalisers),
 *     runs the backward pass for the loss terms of the owned rows and writes d loss / d xs to gxs (3, ext_rows, W0);
 *     the caller adds the stripes' gradients into the full image (overlap-add, one all-reduce).  losses[0..3] = (total,
 *     content, style, tv) of the level, losses[4] = total - identical on every rank.
 * Nothing else may run on the context between begin and end.  The stripe closure implements the default feature maps
 * only: after nst_job_set_taps with any other taps both calls return NST_E_STATE, as they do under NST_COLOR_LUMINANCE,
 * under NST_POOL_AVG (nst_job_set_pooling) and under style layer weights other than 1 (nst_job_set_style_weights).  The
 * Gram targets are the level's, so those of nst_level_set_targets_blend are honoured.  nst_window_* returns NST_E_STATE
 * while the Laplacian loss is set (nst_job_set_laplacian with K > 0), the matting term (nst_job_set_matting with gamma > 0),
 * a Gram shift (nst_job_set_gram_shift) or the moment loss (nst_job_set_moments with a positive weight), and while the
 * level carries an anchor (nst_level_set_anchor). */
int nst_window_sums_count(size_t* count);
int nst_window_begin(nst_ctx* ctx, const float* xs, int row0, int rows, int H0, float* sums, void* stream);
int nst_window_end(nst_ctx* ctx, const float* xs, int row0, int rows, int H0, float content_weight, float style_weight,
                   float tv_weight, float* sums, float* gxs, float* losses, void* stream);

/* arithmetic of the 3x3 convolutions of this context (nst_options.conv_mode): NST_CONV_F16X2 (default: both operands
 * cut into two scaled fp16 pieces, main and cross terms in separate fp32 accumulators; error measured against fp64 =
 * an fp32 MFMA's), NST_CONV_BF16X3 or NST_CONV_F32. */
int nst_conv_mode(const nst_ctx* ctx);

/* Device bytes the context holds right now: a function of its current state, whatever calls led there.  Counted, each at
 * the size actually allocated (a zero-size request takes 16 bytes): the weight images in the layouts of the context's
 * arithmetic, with the biases and the scratch of nst_color_stats (made by its first call and kept); the level workspaces
 * of the configured job (activations, gradient buffers, level images, targets and the buffers sized by the taps); the
 * blocks of the optional terms while they are on (guidance, Laplacian, matting, Gram shift, moments); and, while a
 * standalone call or a target-setting call runs, its scratch - gone again when the call returns.  Not counted: the
 * vectors of an optimiser (nst_opt_create: moments, L-BFGS history), which are allocated apart from the context. */
int nst_ctx_bytes(const nst_ctx* ctx, size_t* bytes);

/* wall time in ms of the kernels of the last nst_closure on `ctx`, measured with HIP events on
 * the streams the kernels ran on (0 if timing was not enabled with nst_set_timing). */
int nst_set_timing(nst_ctx* ctx, int enabled);   /* 0 off, 1 whole closure, 2 + every kernel launch, 3 + only the 3x3 conv
                                                    launches, 4 + those of every fourth closure only */
int nst_last_closure_ms(nst_ctx* ctx, float* ms);
/* last closure, per kernel class: summed launch durations (ms), launches, algorithmic flops.
 * cls: 0 = 3x3 MFMA convolutions (forward + input gradient), 1 = Gram forward + its 1x1 backward,
 * 2 = conv1_1 forward + input gradient, 3 = streaming kernels (pool, bicubic, TV, MSE, reductions). */
int nst_last_closure_class(nst_ctx* ctx, int cls, float* ms, int* launches, double* flops);
/* the same accumulated over every closure since the last reset (timing mode 2); cls = -1: whole
 * closures (ms = summed closure time on the caller's stream, launches = closures). */
int nst_timing_totals(nst_ctx* ctx, int cls, double* ms, long* launches, double* flops, int reset);
/* executed matrix-pipe FLOPs of the launches accumulated in nst_timing_totals(cls): algorithmic FLOPs x the MFMAs the
 * arithmetic spends per product (f16x2: 3, bf16x3: 6, f32: 1), x 2/3 for the launches that ran as Winograd F(2,3). */
int nst_timing_mfma_flops(nst_ctx* ctx, int cls, double* mfma_flops);
/* The timed launches of the last closure (timing mode 2), in launch order: up to `capacity` records into `out`, their
 * number into `count` (which may exceed capacity; 0 without a timed closure).  Read-only; waits for nothing.  h2_*: the kernel
 * shape the f16x2 direct-convolution launcher (conv_h2.hip) decided for the launch - conv_h2_batch_kernel<h2_rows, h2_bn,
 * h2_ntw, h2_chunk> - as the launcher itself reported it; h2_rows = 0: another kernel ran (Winograd, conv1_1, Gram, streaming, or
 * another arithmetic mode). */
typedef struct nst_launch_info {
    int cls;                      /* kernel class, as in nst_last_closure_class */
    int h, w, cin, cout;          /* 3x3 convolutions (cls 0): the launch's (first level's) map and channel counts; else 0 */
    int layer;                    /* 3x3 convolutions: conv layer 1..12 of a forward launch, minus that of an input-gradient launch */
    int h2_rows, h2_bn, h2_ntw, h2_chunk;   /* pixel rows (x 16 columns) and output channels of the workgroup tile, 32-channel
                                     tiles per wave, channels per K chunk */
    int h2_mfma16;                /* 1: the launch ran the 16x16x32 MFMA form */
    int h2_persist;               /* 1: persistent workgroups */
    int h2_second, h2_unpool;     /* 1: the launch carried a second (Gram) K source / un-pooled its input in the loader */
    int h2_bands;                 /* kernel launches it took (row bands of the per-level launcher; else 1) */
} nst_launch_info;
int nst_last_closure_launches(nst_ctx* ctx, nst_launch_info* out, int capacity, int* count);
/* What the last nst_closure, nst_closure_levels, nst_closure_forward or nst_closure_backward call on `ctx` did with streams
 * and graphs (any pointer may be NULL; zeros before the first such call; a call refused before it launched anything leaves
 * the record of the call before it).  Host integers of the context: the call reads state only - it launches nothing, waits
 * for nothing, needs no timing mode, and between nst_closure_forward and nst_closure_backward it leaves the backward half
 * valid.
 *   side_forks:    forks onto the context's side stream.  gram_overlap: 1 where the overlap ran, 0 where it fell back
 *                  (non-default taps, guided levels, use_graph, another arithmetic than f16x2).  level_split: 1 when the
 *                  level mask holds level 0 and a lower level, else 0.  level_split switches gram_overlap off (one side
 *                  stream), so both together report what level_split alone reports.
 *   level_streams: per-level streams the call forked to - the number of levels on the per-level schedule with more than
 *                  one level and single_stream = 0, else 0.
 *   graph_replay:  1 when the call was served by launching the captured hipGraph (use_graph: from the second consecutive
 *                  call with the same arguments on), 0 when its launches were enqueued one by one.  The fork counts of
 *                  such a call are 0: a captured closure stays on one stream. */
int nst_last_closure_schedule(const nst_ctx* ctx, int* side_forks, int* level_streams, int* graph_replay);
/* debugging aid: prints one line per timed launch of the last closure (timing mode 2) to stderr */
int nst_dump_last_closure(nst_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* NST_HIP_H */
