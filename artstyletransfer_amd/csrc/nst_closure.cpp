// nst_closure.cpp - network and closure of libnst_hip.so (include/nst_hip.h): the two walkers of the VGG19 feature network
// (per level: forward / backward; one launch per layer for all pyramid levels: batched_*), the Gram / style terms, the
// closure (forward + losses + backward of every pyramid level) with its optional hipGraph, the targets of a level, and the
// stripe closure of spatial sharding.  One vocabulary serves all of them: conv_setup, launch_conv_batch, launch_pool_*,
// style_term, content_coef, fill_loss_assembly.
//
// Host-side control only; every FLOP and byte of the path is in the .hip kernels.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "nst_ctx.h"

using namespace nst;

namespace {

double conv_flops(int h, int w, int cin, int cout, int taps) { return 2.0 * h * w * (double)cin * cout * taps; }

// the bf16-piece kernels address with 32-bit buffer offsets: tensors from 4 GiB up go to the fp32 kernel
bool uses_pieces(const nst_ctx* ctx, const ConvParams& p) {
    if (ctx->conv_mode == 2) return true;           // launch_conv_h2 runs larger tensors in row bands
    return ctx->conv_mode != 0 && (size_t)p.H * p.W * p.Cin * 4 < 0xFFFFFF00ull;
}
// 3x3 conv dispatch by mode, under the caller's timer (which keeps the shape a conv_h2 launch took); whatever kernel runs,
// the absmax record of the output is produced when asked for
hipError_t launch_conv3(nst_ctx* ctx, const ConvParams& p, Timer& t) {
    hipStream_t s = t.s;
    if (uses_pieces(ctx, p)) {
        if (ctx->conv_mode != 2) return launch_conv_bf3(p, s);
        H2Shape sh{};
        const hipError_t e = launch_conv_h2(p, s, &sh);
        t.shape(sh);
        ctx->h2_direct_launches += sh.direct ? sh.bands : 0;
        return e;
    }
    hipError_t e = launch_conv_mfma(p, 9, s);
    if (e == hipSuccess && ctx->conv_mode == 2 && p.amax_out)
        e = launch_absmax_slots(p.out, (size_t)p.H * p.W * p.Cout, p.amax_out, s);
    return e;
}
// true when the launch runs as ONE piece kernel, whose epilogue can write ReLU bit-masks / the pooled map and
// take a second K source (the fp16 kernel never splits K; the bf16 one may)
bool bf3_unsplit(const nst_ctx* ctx, const ConvParams& p) {
    if (!uses_pieces(ctx, p)) return false;
    if (ctx->conv_mode == 2) return true;
    const int S = conv_bf3_ksplit(p.H, p.W, p.Cin, p.Cout);
    return !(p.partial && S > 1 && (size_t)S * p.H * p.W * p.Cout <= p.partial_floats);
}

// nst_ctx_set_h2_direct_weights' bit of layer l's forward launch: 1 = the 64-channel shape, 2 = the 128-channel short-K shape
static int h2_direct_bit(int l) { return kCout[l] % 128 == 0 ? 2 : 1; }
// Layer l's weights (dgrad: those of its input-gradient launch), the split-K workspace and the context's f16x2 launch knobs
void conv_setup(const nst_ctx* ctx, ConvParams& p, const ActSet& a, int l, bool dgrad) {
    p.wt = dgrad ? ctx->wd[l] : ctx->wf[l]; p.wt_bf = dgrad ? ctx->wd_bf[l] : ctx->wf_bf[l];
    p.partial = a.splitk; p.partial_floats = a.splitk_floats;
    if (ctx->conv_mode != 2) return;
    p.wt_h2 = dgrad ? ctx->wd_h2[l] : ctx->wf_h2[l]; p.wt_h2_inv = dgrad ? ctx->wd_h2_inv[l] : ctx->wf_h2_inv[l];
    p.wt_h2_frag = (!dgrad && (ctx->h2_direct_weights & h2_direct_bit(l))) ? ctx->wf_h2_frag[l] : nullptr;
    p.band_rows = ctx->band_rows; p.mfma16 = ctx->mfma16; p.wg256 = ctx->wg256; p.tile_rows = ctx->tile_rows;
}
// The same for one launch per layer; l = 0: a launch without 3x3 weights (the Gram term alone)
void conv_setup(const nst_ctx* ctx, ConvBatch& b, int l, bool dgrad) {
    b.mfma16 = ctx->mfma16; b.wg256 = ctx->wg256; b.tile_rows = ctx->tile_rows; b.persist = ctx->persist;
    if (l < 1) { b.wt_h2_inv = 1.f; return; }
    b.wt_bf = dgrad ? ctx->wd_bf[l] : ctx->wf_bf[l];
    b.wt_h2 = dgrad ? ctx->wd_h2[l] : ctx->wf_h2[l]; b.wt_h2_inv = dgrad ? ctx->wd_h2_inv[l] : ctx->wf_h2_inv[l];
    b.wt_h2_frag = (!dgrad && (ctx->h2_direct_weights & h2_direct_bit(l))) ? ctx->wf_h2_frag[l] : nullptr;
    b.wt_wino = dgrad ? ctx->wd_wino[l] : ctx->wf_wino[l]; b.wt_wino_inv = dgrad ? ctx->wd_wino_inv[l] : ctx->wf_wino_inv[l];
}
// One conv launch for every level, under the caller's timer: the Winograd form where the layer has its weights and the
// launch qualifies (2/3 of the direct form's matrix-pipe work), else the direct kernel of the arithmetic mode
int launch_conv_batch(nst_ctx* ctx, const ConvBatch& b, hipStream_t s, Timer* t, bool allow_wino) {
    const bool h2 = ctx->conv_mode == 2;
    if (h2 && allow_wino && b.wt_wino && conv_wino_eligible(b)) { if (t) t->mfma_factor(2.0); HIPCHK(ctx, launch_conv_wino_batch(b, s)); }
    else if (h2) {
        H2Shape sh{};
        const hipError_t e = launch_conv_h2_batch(b, s, &sh);
        if (t) t->shape(sh);
        ctx->h2_direct_launches += sh.direct;
        HIPCHK(ctx, e);
    } else HIPCHK(ctx, launch_conv_bf3_batch(b, s));
    return NST_OK;
}
int launch_conv_batch(nst_ctx* ctx, const ConvBatch& b, Timer& t, bool allow_wino) { return launch_conv_batch(ctx, b, t.s, &t, allow_wino); }

// the 2x2/2 pool of the job (nst_job_set_pooling) as kernels of their own, and its backward fused with the ReLU mask of `a`
hipError_t launch_pool_fwd(const nst_ctx* ctx, const float* in, int H, int W, int C, float* out, hipStream_t s) {
    return (ctx->pool_avg ? launch_avgpool_fwd : launch_maxpool_fwd)(in, H, W, C, out, s);
}
hipError_t launch_pool_bwd_relu(const nst_ctx* ctx, const float* a, const float* gpool, int H, int W, int C, float* gin, hipStream_t s) {
    return (ctx->pool_avg ? launch_avgpool_bwd_relu : launch_maxpool_bwd_relu)(a, gpool, H, W, C, gin, s);
}

// The style term of slot q on a map of N = rows x w pixels and C channels: style = (sum_q w_q mse(G_q, Gt_q)) / nstyle,
// G = F^T F / divisor, so dL/dG = sw w_q/nstyle * 2 (G - Gt)/C^2 and dF = 2 * dL/dG * F / (C h w) = F * S with
// S = coef * (G - Gt).  w: the layer weight of the slot's map (nst_job_set_style_weights; 1 multiplies exactly).
// norm_rows > 0 (stripe closure): the normalisers of the full image, norm_rows level-0 rows, instead of the ActSet's own.
struct StyleTerm { int C; size_t N; double divisor; float coef; };
StyleTerm style_term(const Taps& tp, int q, const ActSet& a, float sw, float w, int norm_rows = 0) {
    const int l = tp.style[q], C = kCout[l];
    const size_t N = (size_t)(norm_rows > 0 ? norm_rows >> kScale[l] : a.h[l]) * a.w[l];
    const double chw = (double)C * (double)N;
    return {C, N, chw, (float)((double)sw * (double)w * 4.0 / ((double)tp.nstyle * (double)C * C * chw))};
}
// content = cw * mse(F, Ft) over n elements: dF = coef * (F - Ft)
float content_coef(float cw, double n) { return (float)((double)cw * 2.0 / n); }

// Which full-resolution maps a batched f16x2 forward pass stores.  A launch that feeds a pooling layer writes the pooled map
// beside the full one, and in that schedule the backward pass takes the ReLU and pool decisions from the bit-masks and the
// pool codes: the full map of such a layer has no reader there.  Every map a loss reads (Gram launches - guided ones too -,
// content MSE, second K source, the stripe closure's sums, the top of the chain) is one of the six of kTapLayer, and none of
// those lies in front of a pooling layer (asserted below: a tap that could land there would have to make the rule keep it).
// Under a captured graph every map is stored: a replay runs no host code, so what ActSet::stored[] says could go stale.
// Every other walker and arithmetic mode reads act[] as masks and pool inputs and stores all of it.
constexpr bool taps_avoid_pools() {
    for (int t : kTapLayer)
        for (int p : kPoolAfter) if (t == p) return false;
    return true;
}
static_assert(taps_avoid_pools(), "a map in front of a pooling layer became a tap: map_stored must keep it where a job reads it");
bool map_stored(const nst_ctx* ctx, int l) {
    if (ctx->conv_mode != 2 || ctx->keep_all_maps || ctx->use_graph) return true;
    return pool_index_after(l) < 0;
}

// partial-Gram workspace of one image: the style layers one after the other (the batched launch works on
// all of them at once); offset of style slot k = gram_part_offset(tp, h, w, k), total = gram_part_offset(tp, h, w, tp.nstyle)
size_t gram_part_offset(const Taps& tp, int h, int w, int k) {
    size_t off = 0;
    for (int q = 0; q < k; ++q) {
        const int l = tp.style[q];
        const size_t N = (size_t)(h >> kScale[l]) * (w >> kScale[l]);
        off += (size_t)gram_nsplit(kCout[l], N) * kCout[l] * kCout[l];
    }
    return off;
}

// ---- spatial control (include/nst_hip.h has the definitions) -----------------------------------------------------------
// the guided style term of region r of slot q: divisor C n_r and coef_r, from the mass of the map's scale
StyleTerm guided_term(const Taps& tp, int q, const ActSet& a, float sw, float w, const Guidance& g, int r) {
    const int l = tp.style[q], C = kCout[l];
    const size_t N = (size_t)a.h[l] * a.w[l];
    const double cn = (double)C * g.mass[kScale[l]][r];
    return {C, N, cn, (float)((double)sw * (double)w * (double)g.lambda[r] * 4.0 / ((double)tp.nstyle * (double)C * C * cn))};
}
// the levels of a closure call are all guided or all unguided (the caller has checked): what the first one is
bool guided_levels(const nst_ctx* ctx, const int* lv, int n) { return n > 0 && ctx->lv[lv[0]].guide.R > 0; }
// R, planes and S matrices of style slot q of a guided level: what the backward launch of that map starts from
GuidedBwd guided_bwd_of(const nst_ctx* ctx, const LevelWs& L, int q) {
    const int l = ctx->taps.style[q], C = kCout[l];
    GuidedBwd gb{};
    gb.R = L.guide.R; gb.C = C; gb.N = (size_t)L.acts.h[l] * L.acts.w[l]; gb.F = L.acts.act[l];
    for (int r = 0; r < gb.R; ++r) {
        gb.t[r] = L.guide.plane(kScale[l], r, L.h, L.w);
        gb.S[r] = L.guide.S[q] + (size_t)r * C * C;
    }
    return gb;
}
int launch_guided_backward(nst_ctx* ctx, const GuidedBwd& gb, hipStream_t s) {
    Timer t(ctx, s, K_GRAM, 2.0 * (double)gb.N * gb.C * gb.C * gb.R);
    HIPCHK(ctx, launch_guided_bwd(gb, s));
    return NST_OK;
}
// one region's sum of (G - Gt)^2 partials per finish block -> the map's, weighted by lambda_r: what the loss row reads
int guided_fold(nst_ctx* ctx, LevelWs& L, int q, hipStream_t s) {
    Timer t(ctx, s, K_OTHER, 0);
    HIPCHK(ctx, launch_guided_fold(L.guide.partial[q], L.guide.R, gram_finish_blocks(kCout[ctx->taps.style[q]]), L.guide.lambda,
                                   L.style_partial[q], s));
    return NST_OK;
}

// ---- the Laplacian loss (include/nst_hip.h has the definition; kernels: laplacian.hip) ---------------------------------
// forward part of level L on image y: per entry the pooled sum, then D s - target with the SSE partials the loss row reads.
// as_target: y is the level's content image and D s itself goes to the entry's target.
int lap_forward(nst_ctx* ctx, LevelWs& L, const float* y, bool as_target, hipStream_t s) {
    for (int k = 0; k < ctx->lap_k; ++k) {
        const int p = ctx->lap_pool[k];
        {
            Timer t(ctx, s, K_OTHER, 0);
            HIPCHK(ctx, launch_lap_pool(y, ctx->channels, L.h, L.w, p, L.lap.s[k], s));
        }
        Timer t(ctx, s, K_OTHER, 0);
        if (as_target) HIPCHK(ctx, launch_lap_stencil(L.lap.s[k], L.h / p, L.w / p, nullptr, L.lap.target[k], nullptr, nullptr, s));
        else HIPCHK(ctx, launch_lap_stencil(L.lap.s[k], L.h / p, L.w / p, L.lap.target[k], nullptr, L.lap.r[k], L.lap.partial[k], s));
    }
    return NST_OK;
}
// n_k = (hk-2)(wk-2) and coef_k = (float)(gamma_k 2 / (n_k p^2)); a luminance plane takes the sum over the three channels
double lap_n(const LevelWs& L, int p) { return (double)(L.h / p - 2) * (double)(L.w / p - 2); }
float lap_coef(float gamma, double n, int p, int channels) {
    return (float)((double)gamma * 2.0 * (channels == 1 ? 3.0 : 1.0) / (n * (double)p * (double)p));
}
// gradient part: one pass that adds every entry's coef_k D^T r_k into the level gradient (after the TV gradient)
int lap_backward(nst_ctx* ctx, LevelWs& L, float* grad, hipStream_t s) {
    if (ctx->lap_k < 1) return NST_OK;
    LapBackward lb{};
    lb.K = ctx->lap_k;
    for (int k = 0; k < lb.K; ++k) {
        lb.p[k] = ctx->lap_pool[k];
        lb.coef[k] = lap_coef(ctx->lap_gamma[k], lap_n(L, lb.p[k]), lb.p[k], ctx->channels);
        lb.r[k] = L.lap.r[k];
    }
    Timer t(ctx, s, K_OTHER, 0);
    HIPCHK(ctx, launch_lap_backward(lb, ctx->channels, L.h, L.w, grad, 1, s));
    return NST_OK;
}

// ---- the matting-Laplacian regulariser (include/nst_hip.h has the definition; kernels: matting.hip) --------------------
// n: 3 (h-2)(w-2); a luminance plane (h-2)(w-2), with which the one-plane value is the three-channel one
double mat_n(const nst_ctx* ctx, const LevelWs& L) { return (ctx->channels == 1 ? 1.0 : 3.0) * (double)(L.h - 2) * (double)(L.w - 2); }
// coef = (float)(gamma 2 / (255 n)); on a luminance plane that is the sum over the three channels of E(u)
float mat_coef(float gamma, double n) { return (float)((double)gamma * 2.0 / (255.0 * n)); }
// forward part of level L on image y: the value partials of the tiles, which the loss row reads
int mat_forward(nst_ctx* ctx, LevelWs& L, const float* y, hipStream_t s) {
    if (!(ctx->mat_gamma > 0.f)) return NST_OK;
    Timer t(ctx, s, K_OTHER, 0);
    HIPCHK(ctx, launch_mat_forward(y, L.mat.guide, ctx->channels, L.h, L.w, 1.0 / 255.0, ctx->mat_eps, L.mat.partial, s));
    return NST_OK;
}
// gradient part: one pass that adds coef * (the residuals of a pixel's windows) into the level gradient (after the TV and
// Laplacian gradients)
int mat_backward(nst_ctx* ctx, LevelWs& L, const float* y, float* grad, hipStream_t s) {
    if (!(ctx->mat_gamma > 0.f)) return NST_OK;
    Timer t(ctx, s, K_OTHER, 0);
    HIPCHK(ctx, launch_mat_backward(y, L.mat.guide, ctx->channels, L.h, L.w, 1.0 / 255.0, ctx->mat_eps,
                                    mat_coef(ctx->mat_gamma, mat_n(ctx, L)), grad, 1, s));
    return NST_OK;
}
// the guide of level L: a copy of its content, made where the Laplacian targets are made
int mat_set_guide(nst_ctx* ctx, LevelWs& L, const float* content, hipStream_t s) {
    if (!(ctx->mat_gamma > 0.f)) return NST_OK;
    HIPCHK(ctx, hipMemcpyAsync(L.mat.guide, content, (size_t)ctx->channels * L.h * L.w * sizeof(float), hipMemcpyDeviceToDevice, s));
    return NST_OK;
}

// ---- the temporal consistency term (include/nst_hip.h has the definition; kernels: temporal.hip) -----------------------
// n = channels h w; coef = (float)(gamma 2 / n), formed in double as content_coef is
double anchor_n(const nst_ctx* ctx, const LevelWs& L) { return (double)ctx->channels * (double)L.h * (double)L.w; }
float anchor_coef(float gamma, double n) { return (float)((double)gamma * 2.0 / n); }
// forward part of level L on image y: the value partials, which the loss row reads (a level without an anchor: no launch)
int anchor_forward(nst_ctx* ctx, LevelWs& L, const float* y, hipStream_t s) {
    if (!(L.anc.gamma > 0.f)) return NST_OK;
    Timer t(ctx, s, K_OTHER, 0);
    HIPCHK(ctx, launch_anchor_forward(y, L.anc.anchor, L.anc.weights, ctx->channels, L.h, L.w, L.anc.partial, s));
    return NST_OK;
}
// gradient part: one pass that adds coef c (y - a) into the level gradient (after the TV, Laplacian and matting gradients)
int anchor_backward(nst_ctx* ctx, LevelWs& L, const float* y, float* grad, hipStream_t s) {
    if (!(L.anc.gamma > 0.f)) return NST_OK;
    Timer t(ctx, s, K_OTHER, 0);
    HIPCHK(ctx, launch_anchor_backward(y, L.anc.anchor, L.anc.weights, ctx->channels, L.h, L.w,
                                       anchor_coef(L.anc.gamma, anchor_n(ctx, L)), grad, 1, s));
    return NST_OK;
}

// ---- the MRF term (include/nst_hip.h has the definition; kernels: patch_match.hip) ---------------------------------------
// map index i of level L: the term's operands on the level's own map, 9 C n, and coef = (float)(w 2 / (9 C n)) formed in double
PatchTerm patch_term_of(const LevelWs& L, int i) {
    const int l = kTapLayer[i];
    return PatchTerm{L.acts.act[l], L.acts.h[l], L.acts.w[l], L.pm.nn[i], L.pm.d[i]};
}
double patch_denom(const LevelWs& L, int i) {
    const int l = kTapLayer[i];
    return 9.0 * (double)kCout[l] * (double)(L.acts.h[l] - 2) * (double)(L.acts.w[l] - 2);
}
float patch_coef(float w, double denom) { return (float)((double)w * 2.0 / denom); }
// forward part of level L, once its maps exist: per map with a weight the search (nn), the value partials and mrf_i (a level
// without the term: no launch)
int patch_forward(nst_ctx* ctx, LevelWs& L, hipStream_t s) {
    for (int i = 0; i < 6 && L.pm.on(); ++i) {
        if (!(L.pm.w[i] > 0.f)) continue;
        const int l = kTapLayer[i];
        const PatchTerm t = patch_term_of(L, i);
        PatchSearch p{};
        p.f = t.f; p.h = t.h; p.w = t.w; p.C = kCout[l]; p.amax_f = amax_act(L.acts, l); p.d = t.d; p.keys = L.pm.keys[i];
        if (L.pm.sem.R > 0) {
            // a guided level (nst_level_set_patch_guidance): the norms of the map's own patches - a stride-1 geometry of the
            // map has them as its entries - then the guided search
            Timer tm(ctx, s, K_OTHER, 0, t.h, t.w, kCout[l], 0, 9, 200 + i);      // (layer tag 200 + map index: the rp pass)
            PatchDict own{};
            own.fs = t.f;
            if (!pm_dict_geometry(t.h, t.w, kCout[l], 1, &own)) return fail(ctx, NST_E_STATE, "a guided map has no patch geometry");
            HIPCHK(ctx, launch_pm_norms(own, L.pm.eps, L.pm.sem.rp[i], s));
            p.gd = L.pm.sem.gd[i]; p.ge = L.pm.sem.ge[i]; p.rp = L.pm.sem.rp[i]; p.gamma = L.pm.sem.gamma;
        }
        {
            Timer tm(ctx, s, K_OTHER, 2.0 * (double)(t.h - 2) * (t.w - 2) * (double)t.d.m * 9.0 * kCout[l], t.h, t.w, kCout[l], t.d.m, 9, 100 + i);
            HIPCHK(ctx, launch_pm_search(p, L.pm.nn[i], nullptr, s));
        }
        Timer tm(ctx, s, K_OTHER, 0);
        HIPCHK(ctx, launch_pm_value_partials(t, L.pm.partial[i], s));
        HIPCHK(ctx, launch_pm_value(L.pm.partial[i], patch_denom(L, i), L.pm.vals + i, s));
    }
    return NST_OK;
}

// ---- the histogram loss (include/nst_hip.h has the definition; kernels: histogram.hip) -----------------------------------
// map index i of level L: the term's operands on the level's own map, C N, and coef = (float)(2 w / (C N)) formed in double
HistTerm hist_term_of(const LevelWs& L, int i) {
    const int l = kTapLayer[i];
    return HistTerm{L.acts.act[l], (size_t)L.acts.h[l] * L.acts.w[l], kCout[l], L.hist.bins, L.hist.lo_hi[i], L.hist.ends[i]};
}
double hist_denom(const LevelWs& L, int i) {
    const int l = kTapLayer[i];
    return (double)kCout[l] * (double)L.acts.h[l] * (double)L.acts.w[l];
}
float hist_coef(float w, double denom) { return (float)(2.0 * (double)w / denom); }
// forward part of level L, once its maps exist: per map with a weight the range, the counts, the tables, the value partials
// and hist_i (a level without the term: no launch)
int hist_forward(nst_ctx* ctx, LevelWs& L, hipStream_t s) {
    for (int i = 0; i < 6 && L.hist.on(); ++i) {
        if (!(L.hist.w[i] > 0.f)) continue;
        const HistTerm t = hist_term_of(L, i);
        Timer tm(ctx, s, K_OTHER, 0);
        HIPCHK(ctx, launch_hist_counts(t.f, t.N, t.C, t.bins, L.hist.lo_hi[i], L.hist.counts[i], s));
        HIPCHK(ctx, launch_hist_tables(L.hist.counts[i], t.N, L.hist.s_lo_hi[i], L.hist.s_counts[i], L.hist.Ns[i], t.C, t.bins, L.hist.ends[i], s));
        HIPCHK(ctx, launch_hist_value_partials(t, L.hist.partial[i], s));
        HIPCHK(ctx, launch_hist_value(L.hist.partial[i], hist_denom(L, i), L.hist.vals + i, s));
    }
    return NST_OK;
}

// ---- the relaxed EMD term (include/nst_hip.h has the definition; kernels: remd.hip) ---------------------------------------
// map index i of level L: the term's operands on the level's own map (the image side: f, the sample grid, the absmax record of
// the map, rp and the packed operand of this closure), and the coefficients (float)(w / n) and (float)(w / m) formed in double
RemdSide remd_image_side(const LevelWs& L, int i) {
    const int l = kTapLayer[i];
    RemdSide x{};
    remd_side_geometry(L.acts.h[l], L.acts.w[l], kCout[l], L.remd.si[i], &x);
    x.f = L.acts.act[l]; x.amax = amax_act(L.acts, l); x.r = L.remd.rp[i]; x.packed = L.remd.xpacked[i];
    return x;
}
RemdTerm remd_term_of(const LevelWs& L, int i) {
    const RemdLevel& g = L.remd;
    return RemdTerm{remd_image_side(L, i), g.y[i], g.nnA[i], g.nnB[i], g.cosA[i], g.cosB[i], g.rec[i], g.side[i]};
}
float remd_coef(float w, int count) { return (float)((double)w / (double)count); }
// forward part of level L, once its maps exist: per map with a weight the image side's norms and packed operand, the two
// searches, the cosines, remd_i and the side (a level without the term: no launch)
int remd_forward(nst_ctx* ctx, LevelWs& L, hipStream_t s) {
    for (int i = 0; i < 6 && L.remd.on(); ++i) {
        if (!(L.remd.w[i] > 0.f)) continue;
        const RemdTerm t = remd_term_of(L, i);
        {
            Timer tm(ctx, s, K_OTHER, 0);
            HIPCHK(ctx, launch_remd_norms(t.x, L.remd.eps, L.remd.rp[i], s));
            HIPCHK(ctx, launch_remd_pack(t.x, L.remd.xpacked[i], s));
        }
        // two launches of n x m x C (three MFMAs per product block each), timed as "n x 1, cin C, cout m", layer tag 200 + map
        // for direction A (the style is the dictionary) and 210 + map for direction B (the image is)
        const double flops = 2.0 * (double)t.x.count * (double)t.y.count * (double)t.x.C;
        {
            Timer tm(ctx, s, K_OTHER, flops, t.x.count, 1, t.x.C, t.y.count, 1, 200 + i);
            HIPCHK(ctx, launch_remd_search(t.y, t.x, L.remd.keysA[i], L.remd.nnA[i], s));
        }
        {
            Timer tm(ctx, s, K_OTHER, flops, t.x.count, 1, t.x.C, t.y.count, 1, 210 + i);
            HIPCHK(ctx, launch_remd_search(t.x, t.y, L.remd.keysB[i], L.remd.nnB[i], s));
        }
        Timer tm(ctx, s, K_OTHER, 0);
        HIPCHK(ctx, launch_remd_value(t, L.remd.eps, -1, L.remd.partial[i], L.remd.vals + i, s));
    }
    return NST_OK;
}

// ---- the self-similarity term (include/nst_hip.h has the definition; kernels: selfsim.hip) ----------------------------------
// map index i of level L: the samples of the level's own map (f, the grid, the absmax record of the map, rp and the packed
// operand of this closure), the term's arrays, and the coefficient (float)(w / n) formed in double
RemdSide selfsim_side(const LevelWs& L, int i) {
    const int l = kTapLayer[i];
    RemdSide x{};
    remd_side_geometry(L.acts.h[l], L.acts.w[l], kCout[l], L.selfsim.stride[i], &x);
    x.f = L.acts.act[l]; x.amax = amax_act(L.acts, l); x.r = L.selfsim.rp[i]; x.packed = L.selfsim.xpacked[i];
    return x;
}
SelfSimTerm selfsim_term_of(const LevelWs& L, int i) {
    const SelfSimLevel& g = L.selfsim;
    return SelfSimTerm{g.D[i], g.q[i], g.Dc[i], g.qc[i], g.n[i], g.sg[i], g.partial[i], g.t[i], g.vals + i};
}
// forward part of level L, once its maps exist: per map with a weight the norms and the packed operand, the distance matrix
// (timed as "n x 1, cin C, cout n", layer tag 220 + map), the column sums, the signs and selfsim_k (a level without the term:
// no launch)
int selfsim_forward(nst_ctx* ctx, LevelWs& L, hipStream_t s) {
    for (int i = 0; i < 6 && L.selfsim.on(); ++i) {
        if (!(L.selfsim.w[i] > 0.f)) continue;
        const RemdSide x = selfsim_side(L, i);
        {
            Timer tm(ctx, s, K_OTHER, 0);
            HIPCHK(ctx, launch_remd_norms(x, L.selfsim.eps, L.selfsim.rp[i], s));
            HIPCHK(ctx, launch_remd_pack(x, L.selfsim.xpacked[i], s));
        }
        {
            Timer tm(ctx, s, K_OTHER, 2.0 * (double)x.count * (double)x.count * (double)x.C, x.count, 1, x.C, x.count, 1, 220 + i);
            HIPCHK(ctx, launch_selfsim_matrix(x, L.selfsim.D[i], s));
        }
        Timer tm(ctx, s, K_OTHER, 0, x.count, 1, x.count, x.count, 1, 240 + i);      // (the passes over the n x n arrays: tag 240 + map)
        HIPCHK(ctx, launch_selfsim_colsums(L.selfsim.D[i], x.count, L.selfsim.eps, L.selfsim.partial[i], L.selfsim.s[i], L.selfsim.q[i], s));
        HIPCHK(ctx, launch_selfsim_value(selfsim_term_of(L, i), s));
    }
    return NST_OK;
}

// ---- the long-range style term (include/nst_hip.h has the definition; kernels: xcorr.hip) -----------------------------------
// item (map index i, shift d) of level L: the level's own map with its absmax record, the shift's slabs, Z_d, the target and the
// coefficient 2 w_i / (|D| C^2 Z_d) formed in double, and the places of G_d, S_d, S_d^T and the partial sums of squares
double xcorr_divisor(int C, int h, int w, int dx, int dy) { return (double)C * (double)(h - dy) * (double)(w - dx); }
float xcorr_coef(float wgt, int nd, int C, double Z) { return (float)(2.0 * (double)wgt / ((double)nd * (double)C * (double)C * Z)); }
XcorrItem xcorr_item_of(const LevelWs& L, int i, int d) {
    const XcorrLevel& g = L.xcorr;
    const int l = kTapLayer[i], C = kCout[l], h = L.acts.h[l], w = L.acts.w[l];
    const size_t CC = (size_t)C * C;
    const double Z = xcorr_divisor(C, h, w, g.dx[d], g.dy[d]);
    XcorrItem it{};
    it.f = L.acts.act[l]; it.amax = amax_act(L.acts, l); it.part = g.part[i][d];
    it.C = C; it.h = h; it.w = w; it.dx = g.dx[d]; it.dy = g.dy[d];
    it.divisor = (float)Z;
    it.target = g.Gt[i] + d * CC; it.coef = xcorr_coef(g.w[i], g.nd, C, Z);
    it.G = g.G[i] + d * CC; it.S = g.S[i] + d * CC; it.St = g.St[i] + d * CC;
    it.sq = g.sq[i] + (size_t)d * xcorr_finish_blocks(C);
    return it;
}
// forward part of the levels lv[0..n), once their maps exist: every (level, weighted map, shift) in one value launch and one
// finish launch (XCORR_BATCH_MAX items a launch), then xcorr_i of every (level, weighted map) in one launch (levels without
// the term: no launch)
int xcorr_forward(nst_ctx* ctx, const int* lv, int n, hipStream_t s) {
    XcorrBatch b{};
    XcorrValueBatch vb{};
    double flops = 0.0;
    auto flush = [&]() -> int {
        if (b.n == 0) return NST_OK;
        Timer tm(ctx, s, K_OTHER, flops, b.n, 1, 0, 0, 1, 250);      // (timed as a whole, layer tag 250)
        HIPCHK(ctx, launch_xcorr_batch(b, s));
        b.n = 0; flops = 0.0;
        return NST_OK;
    };
    for (int k = 0; k < n; ++k) {
        const LevelWs& L = ctx->lv[lv[k]];
        for (int i = 0; i < 6 && L.xcorr.on(); ++i) {
            if (!(L.xcorr.w[i] > 0.f)) continue;
            const int C = kCout[kTapLayer[i]];
            for (int d = 0; d < L.xcorr.nd; ++d) {
                if (b.n == XCORR_BATCH_MAX) NSTCHK(flush());
                const XcorrItem it = xcorr_item_of(L, i, d);
                flops += 2.0 * (double)(it.h - it.dy) * (double)(it.w - it.dx) * (double)C * (double)C;
                b.it[b.n++] = it;
            }
            vb.it[vb.n++] = XcorrValueItem{L.xcorr.sq[i], L.xcorr.nd, xcorr_finish_blocks(C), (double)C * (double)C, L.xcorr.vals + i};
        }
    }
    NSTCHK(flush());
    if (vb.n > 0) {
        Timer tm(ctx, s, K_OTHER, 0);
        HIPCHK(ctx, launch_xcorr_values(vb, s));
    }
    return NST_OK;
}
// the term's share of the loss rows, behind the loss assembly (a closure none of whose levels in the mask carries the term: no
// launch, and the rows are what that assembly left)
int xcorr_loss_rows(nst_ctx* ctx, unsigned level_mask, float* losses, hipStream_t s) {
    XcorrRows r{};
    r.levels = ctx->levels; r.out = losses;
    bool any = false;
    for (int i = 0; i < ctx->levels; ++i) {
        const XcorrLevel& g = ctx->lv[i].xcorr;
        r.lv[i].owned = (int)((level_mask >> i) & 1u);
        if (!g.on()) continue;
        r.lv[i].vals = g.vals;
        for (int k = 0; k < 6; ++k) r.lv[i].w[k] = g.w[k];
        any = true;
    }
    if (any) HIPCHK(ctx, launch_xcorr_rows(r, s));
    return NST_OK;
}
// the gradient launch of map index i of level L into dst
XcorrGrad xcorr_grad_of(const LevelWs& L, int i, float* dst, bool held) {
    const XcorrLevel& g = L.xcorr;
    const int l = kTapLayer[i];
    XcorrGrad x{};
    x.f = L.acts.act[l]; x.h = L.acts.h[l]; x.w = L.acts.w[l]; x.C = kCout[l]; x.nd = g.nd;
    for (int d = 0; d < g.nd; ++d) { x.dx[d] = g.dx[d]; x.dy[d] = g.dy[d]; }
    x.S = g.S[i]; x.St = g.St[i]; x.out = dst; x.accumulate = held ? 1 : 0;
    return x;
}

// ---- the per-map terms together (MapTerm in nst_ctx.h): MRF, histogram loss, relaxed EMD, self-similarity, xcorr - always in this order
// forward parts of the levels lv[0..n), once their maps exist: every level of one term before the next term
int map_terms_forward(nst_ctx* ctx, const int* lv, int n, hipStream_t s) {
    for (int k = 0; k < n; ++k) NSTCHK(patch_forward(ctx, ctx->lv[lv[k]], s));
    for (int k = 0; k < n; ++k) NSTCHK(hist_forward(ctx, ctx->lv[lv[k]], s));
    for (int k = 0; k < n; ++k) NSTCHK(remd_forward(ctx, ctx->lv[lv[k]], s));
    for (int k = 0; k < n; ++k) NSTCHK(selfsim_forward(ctx, ctx->lv[lv[k]], s));
    NSTCHK(xcorr_forward(ctx, lv, n, s));
    return NST_OK;
}
// gradient parts of conv layer m of level L, of the terms the map carries, into dst (the map's shape).  `held`: dst holds an
// addend already (the content gradient) - the first launch writes unless it does, every later one adds - and on return:
// it holds one now.  The one place a walker's addend takes these gradients in, at the top of a chain or inside it.
int map_terms_backward(nst_ctx* ctx, const LevelWs& L, int m, float* dst, bool& held, hipStream_t s) {
    const int i = tap_index_of(m);
    if (L.pm.carries(m)) {
        Timer tm(ctx, s, K_OTHER, 0);
        HIPCHK(ctx, launch_pm_grad(patch_term_of(L, i), patch_coef(L.pm.w[i], patch_denom(L, i)), dst, held ? 1 : 0, s));
        held = true;
    }
    if (L.hist.carries(m)) {
        Timer tm(ctx, s, K_OTHER, 0);
        HIPCHK(ctx, launch_hist_grad(hist_term_of(L, i), hist_coef(L.hist.w[i], hist_denom(L, i)), dst, held ? 1 : 0, s));
        held = true;
    }
    if (L.remd.carries(m)) {
        Timer tm(ctx, s, K_OTHER, 0);
        const RemdTerm t = remd_term_of(L, i);
        HIPCHK(ctx, launch_remd_grad(t, remd_coef(L.remd.w[i], t.x.count), remd_coef(L.remd.w[i], t.y.count), dst, held ? 1 : 0, s));
        held = true;
    }
    if (L.selfsim.carries(m)) {
        // (W, U and the fp32 product g = -W U, n x n x C: timed as "n x 1, cin n, cout C", layer tag 230 + map; no f16 work)
        const RemdSide x = selfsim_side(L, i);
        Timer tm(ctx, s, K_OTHER, 0, x.count, 1, x.count, x.C, 1, 230 + i);
        HIPCHK(ctx, launch_selfsim_grad(x, selfsim_term_of(L, i), remd_coef(L.selfsim.w[i], x.count), L.selfsim.W[i], L.selfsim.U[i], dst,
                                        held ? 1 : 0, s));
        held = true;
    }
    if (L.xcorr.carries(m)) {
        // (the fp32 product over all shifts, N x 2 C |D| x C: timed as "N x 1, cin 2 C |D|, cout C", layer tag 260 + map)
        const XcorrGrad x = xcorr_grad_of(L, i, dst, held);
        Timer tm(ctx, s, K_OTHER, 0, x.h * x.w, 1, 2 * x.C * x.nd, x.C, 1, 260 + i);
        HIPCHK(ctx, launch_xcorr_grad(x, s));
        held = true;
    }
    return NST_OK;
}

// ---- the moment loss (include/nst_hip.h has the definition; kernels: moments.hip) ----------------------------------------
// style slot q of level L on its map f (N pixels, C channels): the statistics item, and the fold item that follows the Gram
// finish pass and the row bias of a shifted Gram (r0: that bias, or nullptr)
MomentItem moment_item(const nst_ctx* ctx, const LevelWs& L, int q, const float* f, size_t N, int C) {
    return MomentItem{f, N, C, (double)ctx->mom_eps, L.mom.part(q), L.mom.stat(q), nullptr, nullptr, 1.f, 0, 0, 0, 0};
}
MomentFoldItem moment_fold_item(const nst_ctx* ctx, const LevelWs& L, int q, size_t N, int C, unsigned short* S_bf, unsigned* S_amax) {
    return MomentFoldItem{L.mom.stat(q), L.mom.mean_t(q), L.mom.std_t(q), L.S[q], S_bf, S_amax,
                          ctx->gs_on() ? L.gs.row_bias(q) : nullptr, L.mom.row_bias(q), L.mom.loss(q), N, C,
                          ctx->mom_wm_of(q), ctx->mom_ws_of(q)};
}

}  // namespace

namespace nst {

// ---- network forward ----------------------------------------------------------------------------
int forward(nst_ctx* ctx, ActSet& a, const float* x, int h, int w, hipStream_t s, int last_layer, int channels) {
    a.begin_pass();
    const bool h2 = ctx->conv_mode == 2;
    if (h2) HIPCHK(ctx, launch_zero(a.amax, (size_t)(NL + kMaxStyle) * NST_AMAX_SLOTS, s));     // act + S records
    {
        Timer t(ctx, s, K_CONV1, conv_flops(h, w, 3, 64, 9));
        unsigned* bits = ctx->conv_mode ? a.bits[0] : nullptr;
        HIPCHK(ctx, launch_conv1_1_fwd(x, h, w, ctx->w11k, ctx->bias[0], a.act[0], bits, h2 ? amax_act(a, 0) : nullptr, s, channels));
        a.bits_valid[0] = bits != nullptr;
    }
    a.pass = 0;
    for (int l = 0; l <= last_layer; ++l) a.stored[l] = true;
    for (int l = 1; l <= last_layer; ++l) {
        const int pk = pool_index_after(l - 1);
        const float* in = (pk >= 0) ? a.pool[pk] : a.act[l - 1];
        ConvParams p{};
        p.in = in; p.bias = ctx->bias[l]; p.addend = nullptr; p.mask = nullptr; p.out = a.act[l];
        p.H = a.h[l]; p.W = a.w[l]; p.Cin = kCin[l]; p.Cout = kCout[l];
        p.relu = ctx->taps.relu_of(l);
        p.pool_avg = ctx->pool_avg;
        conv_setup(ctx, p, a, l, false);
        if (h2) {
            p.amax_in = amax_act(a, l - 1);       // the pooled map's maximum is its source's
            p.amax_out = amax_act(a, l);
        }
        const int pa = pool_index_after(l);
        const bool fuse = bf3_unsplit(ctx, p);        // the epilogue extras exist in the unsplit bf3 kernel only
        if (fuse) {
            p.bits_out = a.bits[l];                   // nullptr for layers whose mask nobody reads
            if (pa >= 0 && l < last_layer) p.pool_out = a.pool[pa];
        }
        {
            Timer t(ctx, s, K_CONV3, conv_flops(p.H, p.W, p.Cin, p.Cout, 9), p.H, p.W, p.Cin, p.Cout, 9, l);
            HIPCHK(ctx, launch_conv3(ctx, p, t));
        }
        a.bits_valid[l] = fuse && a.bits[l] != nullptr;
        if (pa >= 0 && l < last_layer) {
            if (p.pool_out) {
                a.pooled[pa] = true;
            } else {
                Timer t(ctx, s, K_OTHER, 0);
                HIPCHK(ctx, launch_pool_fwd(ctx, a.act[l], a.h[l], a.w[l], kCout[l], a.pool[pa], s));
            }
        }
    }
    return NST_OK;
}

// ---- network backward (nst_ctx.h has the contract) --------------------------------------------------
int backward(nst_ctx* ctx, ActSet& a, const Inject* inj, const ContentJob* cj, float* gbuf0, float* gbuf1, float* gx,
             int h, int w, hipStream_t s, int top, bool top_mask, int channels, const LevelWs* terms) {
    float* cur = gbuf0;     // holds the gradient w.r.t. the pre-ReLU output of the layer being processed
    float* oth = gbuf1;
    const bool h2 = ctx->conv_mode == 2;
    if (h2) HIPCHK(ctx, launch_zero(amax_grad(a, 0), (size_t)NL * NST_AMAX_SLOTS, s));
    // top of the chain
    {
        const int l = top;
        const size_t n = (size_t)a.h[l] * a.w[l] * kCout[l];
        const bool content = inj[l].content && cj;
        if (content) {
            Timer t(ctx, s, K_OTHER, 0);
            HIPCHK(ctx, launch_mse_grad(a.act[l], cj->target, cj->n, cj->coef, oth, cj->partial, s));
        }
        // the per-map terms of the top map: onto the content gradient when there is one, the addend of the 1x1 Gram launch - or,
        // on a content map that is no style map (the self-similarity term may sit there), of the mask pass below
        bool held = content;
        if (terms && (inj[l].S || content)) NSTCHK(map_terms_backward(ctx, *terms, l, oth, held, s));
        if (inj[l].guided) {
            GuidedBwd gb = *inj[l].guided;
            gb.addend = content ? oth : nullptr; gb.out = cur; gb.mask = top_mask ? a.act[l] : nullptr;
            NSTCHK(launch_guided_backward(ctx, gb, s));
        } else if (inj[l].S) {
            // (the content gradient, if any, as the addend of the 1x1 Gram launch)
            ConvParams p{};
            p.in = a.act[l]; p.wt = inj[l].S; p.out = cur; p.mask = top_mask ? a.act[l] : nullptr;
            p.addend = held ? oth : nullptr;
            p.bias = inj[l].bias;                  // (a shifted Gram: F S + r, then the addend and the mask)
            p.H = a.h[l]; p.W = a.w[l]; p.Cin = kCout[l]; p.Cout = kCout[l];
            Timer t(ctx, s, K_GRAM, conv_flops(p.H, p.W, p.Cin, p.Cout, 1));
            HIPCHK(ctx, launch_conv_mfma(p, 1, s));
        } else if (content || inj[l].direct) {
            const float* g = content ? oth : inj[l].direct;
            Timer t(ctx, s, K_OTHER, 0);
            if (top_mask) HIPCHK(ctx, launch_relu_mask(a.act[l], g, n, cur, s));
            else HIPCHK(ctx, launch_copy(g, cur, n, s));
        } else {
            HIPCHK(ctx, launch_zero(cur, n, s));
        }
        if (h2) HIPCHK(ctx, launch_absmax_slots(cur, n, amax_grad(a, l), s));
    }
    for (int l = top; l >= 1; --l) {
        // cur = g(pre-ReLU of layer l), dims of layer l, kCout[l] channels.  dgrad -> gradient w.r.t.
        // layer l's input: either pool[k] (then un-pool into act[l-1]'s shape) or act[l-1] directly.
        const int pk = pool_index_after(l - 1);
        ConvParams p{};
        p.in = cur; p.out = oth;
        p.H = a.h[l]; p.W = a.w[l]; p.Cin = kCout[l]; p.Cout = kCin[l];
        conv_setup(ctx, p, a, l, true);
        if (h2) {
            p.amax_in = amax_grad(a, l);
            p.amax_out = amax_grad(a, l - 1);     // when un-pooled next, this bounds the un-pooled gradient too
        }
        if (pk >= 0) {
            // (average pooling: the un-pooled gradient is a quarter of the pooled one, so the pooled gradient's absmax would
            // describe a tensor four times what the next launch reads - that launch's record is taken after the un-pooling)
            const bool avg = ctx->pool_avg != 0;
            if (avg) p.amax_out = nullptr;
            {
                Timer t(ctx, s, K_CONV3, conv_flops(p.H, p.W, p.Cin, p.Cout, 9), p.H, p.W, p.Cin, p.Cout, 9, -l);
                HIPCHK(ctx, launch_conv3(ctx, p, t));
            }
            // oth = g(pool[pk]); un-pool through act[l-1] with its ReLU mask -> cur
            Timer t(ctx, s, K_OTHER, 0);
            HIPCHK(ctx, launch_pool_bwd_relu(ctx, a.act[l - 1], oth, a.h[l - 1], a.w[l - 1], kCout[l - 1], cur, s));
            if (avg && h2)
                HIPCHK(ctx, launch_absmax_slots(cur, (size_t)a.h[l - 1] * a.w[l - 1] * kCout[l - 1], amax_grad(a, l - 1), s));
            // cur now holds g(pre-ReLU of layer l-1); no tap layer sits directly before a pool
        } else {
            const int m = l - 1;   // the layer whose activation this gradient flows into
            const Inject& in = inj[m];
            const bool fuse = bf3_unsplit(ctx, p);
            double extra_flops = 0;
            // the content gradient first: a Gram term of the same map then rides on the launch as well (second K source)
            // or accumulates into the addend (standalone 1x1 launch)
            if (in.content && cj) {
                Timer t(ctx, s, K_OTHER, 0);
                HIPCHK(ctx, launch_mse_grad(a.act[m], cj->target, cj->n, cj->coef, oth, cj->partial, s));
                p.addend = oth;
            } else if (in.direct) {
                p.addend = in.direct;
            }
            // the per-map terms of the map: written, or added to the content gradient
            bool held = p.addend == oth;
            if (terms) NSTCHK(map_terms_backward(ctx, *terms, m, oth, held, s));
            if (held) p.addend = oth;
            if (in.guided) {
                // the guided Gram backward by its own launch, onto the content gradient when there is one: the addend
                GuidedBwd gb = *in.guided;
                gb.addend = p.addend; gb.out = oth;
                NSTCHK(launch_guided_backward(ctx, gb, s));
                p.addend = oth;
            } else if (in.S && fuse && (h2 ? in.S_amax != nullptr : in.S_bf != nullptr)) {
                // Gram backward rides on this launch as a second K source: acc += act[m] * S
                p.in2 = a.act[m]; p.Cin2 = kCout[m]; p.wt2_bf = in.S_bf;
                p.wt2_f32 = in.S; p.amax_in2 = amax_act(a, m); p.amax_w2 = in.S_amax;
                p.bias = in.bias;                  // (a shifted Gram's row bias: after the scale, before the addend and the mask)
                extra_flops = conv_flops(a.h[m], a.w[m], kCout[m], kCout[m], 1);
            } else if (in.S) {
                ConvParams q{};
                q.in = a.act[m]; q.wt = in.S; q.out = oth; q.addend = p.addend; q.bias = in.bias;
                q.H = a.h[m]; q.W = a.w[m]; q.Cin = kCout[m]; q.Cout = kCout[m];
                Timer t(ctx, s, K_GRAM, conv_flops(q.H, q.W, q.Cin, q.Cout, 1));
                HIPCHK(ctx, launch_conv_mfma(q, 1, s));
                p.addend = oth;
            }
            if (fuse && a.bits_valid[m]) p.bits_in = a.bits[m];
            else p.mask = a.act[m];
            {
                Timer t(ctx, s, K_CONV3, conv_flops(p.H, p.W, p.Cin, p.Cout, 9) + extra_flops, p.H, p.W, p.Cin, p.Cout, 9, -l);
                HIPCHK(ctx, launch_conv3(ctx, p, t));
            }
            float* tmp = cur; cur = oth; oth = tmp;
        }
    }
    {
        Timer t(ctx, s, K_CONV1, conv_flops(h, w, 64, 3, 9));
        HIPCHK(ctx, launch_conv1_1_dgrad(cur, h, w, ctx->w11d, h2 ? amax_grad(a, 0) : nullptr, gx, s, channels));
    }
    return NST_OK;
}

int gram_of(nst_ctx* ctx, const GramOperand& op, const GramFinish& fin, hipStream_t s, bool timed) {
    const int ns = gram_nsplit(op.C, op.N);
    {
        std::optional<Timer> t;
        if (timed) t.emplace(ctx, s, K_GRAM, 2.0 * (double)op.N * op.C * op.C);
        HIPCHK(ctx, launch_gram_partial(op.f, op.N, op.C, ns, op.amax, op.part, s, op.guide, op.offset, ctx->gram_pack));
    }
    std::optional<Timer> t;
    if (timed) t.emplace(ctx, s, K_OTHER, 0);
    if (fin.alpha >= 0.f)
        HIPCHK(ctx, launch_gram_finish_blend(op.part, gram_nslabs(op.C, ns), op.C, op.divisor, fin.alpha, fin.accumulate, fin.gram_out, s));
    else
        HIPCHK(ctx, launch_gram_finish(op.part, gram_nslabs(op.C, ns), op.C, op.divisor, fin.target, fin.coef, fin.gram_out, fin.S, fin.S_bf,
                                       fin.S_amax, fin.mse_partial, s));
    return NST_OK;
}

int gram_shifted_of(nst_ctx* ctx, const GramOperand& op, const ShiftedGram& sg, const GramFinish& fin, hipStream_t s) {
    if (!op.amax) return fail(ctx, NST_E_STATE, "the shifted Gram runs in the f16x2 arithmetic only");
    {
        OffsetBatch ob{};
        ob.n = 1;
        ob.it[0] = OffsetItem{op.f, op.N, op.C, op.amax, sg.shift, sg.center, sg.offset, sg.rec, sg.sums, 0, 0, 0};
        Timer t(ctx, s, K_OTHER, 0);
        HIPCHK(ctx, launch_gram_offsets(ob, s));
    }
    GramOperand shifted = op;
    shifted.amax = sg.rec; shifted.guide = nullptr; shifted.offset = sg.offset;
    NSTCHK(gram_of(ctx, shifted, fin, s));
    if (sg.r && fin.S) {
        RowBiasBatch rb{};
        rb.n = 1;
        rb.it[0] = RowBiasItem{sg.offset, fin.S, sg.r, op.C, 0};
        Timer t(ctx, s, K_OTHER, 0);
        HIPCHK(ctx, launch_gram_row_bias(rb, s));
    }
    return NST_OK;
}

size_t gram_part_floats_for(const Taps& tp, int h, int w) { return gram_part_offset(tp, h, w, tp.nstyle); }

}  // namespace nst

namespace {

// ---- closure with every conv layer launched once for all pyramid levels ("batched") ----------------------
// Layer l has the same weights and channel counts at every level, and layer l of any level depends only on
// layer l-1 of that level, so the 12 forward and 12 input-gradient convolutions each become ONE launch whose
// grid lists the tiles of level 0, then level 1, ...: the small levels fill the tail of the big level's grid
// instead of running as under-filled launches.  Everything is ordered on the caller's stream.
// A job evaluated on a horizontal stripe of a larger image (spatial sharding): the level-0 image of this
// context is rows [.., ..) of an H0-row image; the loss terms of its rows [row0, row0 + rows) are this context's,
// with the normalisers of the full image.  Per-layer quantities scale by the layer's stride (row0, rows: multiples
// of 16).  Style / content / TV sums of the owned rows go to `sums` (begin); after the caller has added the other
// stripes' sums the backward uses them (end).
struct Window {
    int row0, rows, H0;
    float* sums;          // begin: out;  end: in (summed over the stripes)
};
// owned rows at a layer of stride 2^sc: [row0 >> sc, (row0 + rows) >> sc) (the bottom stripe may end on a ragged row)
inline int win_r0(const Window& w, int sc) { return w.row0 >> sc; }
inline int win_nr(const Window& w, int sc) { return ((w.row0 + w.rows) >> sc) - (w.row0 >> sc); }
constexpr size_t kWinGramOff[5] = {0, 64 * 64, 64 * 64 + 128 * 128, 64 * 64 + 128 * 128 + 256 * 256,
                                   64 * 64 + 128 * 128 + 256 * 256 + 512 * 512};
constexpr size_t kWinScalarOff = 64 * 64 + 128 * 128 + 256 * 256 + 2 * 512 * 512;    // content SSE, TV x, TV y
constexpr size_t kWinSums = kWinScalarOff + 4;

// Layer l's forward launch over the levels lv[0 .. n): what batched_forward enqueues and restore_map repeats.  full = false:
// the launch leaves out the full-resolution map (map_stored) and writes the pooled one, the mask and the code words only.
ConvBatch forward_batch(nst_ctx* ctx, const int* lv, int n, int l, bool full, double* flops) {
    const bool h2 = ctx->conv_mode == 2;
    const int pk = pool_index_after(l - 1), pa = pool_index_after(l);
    ConvBatch b{};
    b.n = n; b.bias = ctx->bias[l]; b.Cin = kCin[l]; b.Cout = kCout[l];
    // conv5_1 before its ReLU (use_relu = 0): the Winograd launch takes its general epilogue (MODE 0), which honours relu = 0
    b.relu = ctx->taps.relu_of(l);
    conv_setup(ctx, b, l, false);
    b.pool_avg = ctx->pool_avg;
    for (int k = 0; k < n; ++k) {
        ActSet& a = ctx->lv[lv[k]].acts;
        ConvImage& im = b.img[k];
        im.in = (pk >= 0) ? a.pool[pk] : a.act[l - 1];
        im.out = full ? a.act[l] : nullptr; im.H = a.h[l]; im.W = a.w[l];
        im.bits_out = a.bits[l];
        im.pool_out = (pa >= 0) ? a.pool[pa] : nullptr;
        im.pcode_out = (pa >= 0 && h2) ? a.pcode[pa] : nullptr;
        a.bits_valid[l] = a.bits[l] != nullptr;
        a.stored[l] = full;
        if (pa >= 0) a.pooled[pa] = true;
        im.amax_in = amax_act(a, l - 1); im.amax_out = amax_act(a, l);
        *flops += conv_flops(im.H, im.W, b.Cin, b.Cout, 9);
    }
    return b;
}

// `fork_sw` >= 0 (f16x2 closure, nst_options.gram_overlap): once relu3_1 is written, the Gram matrices of relu1_1, relu2_1 and
// relu3_1 - HBM-bound streams over 85 % of the style bytes - are launched on the context's side stream, where they run
// under the MFMA-bound convolutions of conv3_2 ... conv5_1 instead of after them; the caller joins before the backward.
int batched_gram(nst_ctx* ctx, const int* lv, int n, float sw, hipStream_t s, unsigned qmask);
int batched_forward(nst_ctx* ctx, const float* const* xi, const int* lv, int n, hipStream_t s, const Window* win, float fork_sw = -1.f) {
    const bool h2 = ctx->conv_mode == 2;
    const int top = ctx->taps.top;
    // nst_ctx_set_forward_pack: the front of the network - absmax clears, TV partials, conv1_1 - in one launch each for all
    // levels (levels 1 and 2 cannot fill the chip with conv1_1's two persistent workgroups per CU); stripes and a captured
    // graph keep the per-level launches below
    const bool pack = ctx->forward_pack && h2 && !win && !ctx->use_graph && n > 1;      // (one level: nothing to pack - target forwards)
    if (pack) {
        ZeroBatch zb{};
        TvBatch tb{};
        Conv1Batch cb{};
        double flops = 0;
        zb.n = tb.n = cb.n = n;
        tb.C = ctx->channels;
        cb.wk = ctx->w11k; cb.bias = ctx->bias[0]; cb.channels = ctx->channels;
        for (int k = 0; k < n; ++k) {
            LevelWs& L = ctx->lv[lv[k]];
            ActSet& a = L.acts;
            a.begin_pass();
            zb.out[k] = a.amax; zb.n_words[k] = (size_t)AMAX_IDS * NST_AMAX_SLOTS;
            tb.y[k] = xi[lv[k]]; tb.h[k] = L.h; tb.w[k] = L.w; tb.partial[k] = L.tv_partial;
            cb.img[k] = Conv1Image{xi[lv[k]], a.act[0], a.bits[0], amax_act(a, 0), L.h, L.w, 0, 0};
            flops += conv_flops(L.h, L.w, 3, 64, 9);
            a.bits_valid[0] = true;
            a.stored[0] = true;
        }
        HIPCHK(ctx, launch_zero_batch(zb, s));
        {
            Timer t(ctx, s, K_OTHER, 0);
            HIPCHK(ctx, launch_tv_partial_batch(tb, s));
        }
        Timer t(ctx, s, K_CONV1, flops);
        HIPCHK(ctx, launch_conv1_1_fwd_batch(cb, s));
    }
    for (int k = 0; k < n && !pack; ++k) {
        LevelWs& L = ctx->lv[lv[k]];
        ActSet& a = L.acts;
        a.begin_pass();
        if (h2) HIPCHK(ctx, launch_zero(a.amax, (size_t)AMAX_IDS * NST_AMAX_SLOTS, s));
        {
            Timer t(ctx, s, K_OTHER, 0);
            HIPCHK(ctx, launch_tv_partial(xi[lv[k]], ctx->channels, L.h, L.w, L.tv_partial, s, win ? win->row0 : 0, win ? win->rows : 0));
        }
        Timer t(ctx, s, K_CONV1, conv_flops(L.h, L.w, 3, 64, 9));
        HIPCHK(ctx, launch_conv1_1_fwd(xi[lv[k]], L.h, L.w, ctx->w11k, ctx->bias[0], a.act[0], a.bits[0],
                                       h2 ? amax_act(a, 0) : nullptr, s, ctx->channels));
        a.bits_valid[0] = true;
        a.stored[0] = true;
    }
    ++ctx->fwd_pass;
    for (int k = 0; k < n; ++k) {
        ActSet& a = ctx->lv[lv[k]].acts;
        a.pass = ctx->fwd_pass; a.pass_n = n;
        for (int j = 0; j < n; ++j) a.pass_lv[j] = lv[j];
    }
    for (int l = 1; l <= top; ++l) {
        double flops = 0;
        const ConvBatch b = forward_batch(ctx, lv, n, l, map_stored(ctx, l), &flops);
        {
            Timer t(ctx, s, K_CONV3, flops, b.img[0].H, b.img[0].W, b.Cin, b.Cout, 9, l);
            NSTCHK(launch_conv_batch(ctx, b, t, true));
        }
        if (l == 4 && fork_sw >= 0.f && ctx->side) {
            HIPCHK(ctx, hipEventRecord(ctx->side_fork, s));
            HIPCHK(ctx, hipStreamWaitEvent(ctx->side, ctx->side_fork, 0));
            ++ctx->sched.side_forks;
            NSTCHK(batched_gram(ctx, lv, n, fork_sw, ctx->side, 0x07u));
            HIPCHK(ctx, hipEventRecord(ctx->side_join, ctx->side));
        }
    }
    return NST_OK;
}

// ---- style losses: Gram matrices, S = d loss / d G folded for the backward
// guided levels: R items per (level, style map), as many batches as that takes, then the loss partials of every map
int batched_gram_guided(nst_ctx* ctx, const int* lv, int n, float sw, hipStream_t s) {
    GramBatch gb{};
    double flops = 0;
    auto flush = [&]() -> int {
        if (gb.n == 0) return NST_OK;
        Timer t(ctx, s, K_GRAM, flops);
        HIPCHK(ctx, launch_gram_batch(gb, s, ctx->gram_pack));
        gb = GramBatch{};
        flops = 0;
        return NST_OK;
    };
    for (int k = 0; k < n; ++k) {
        LevelWs& L = ctx->lv[lv[k]];
        const Guidance& g = L.guide;
        for (int q = 0; q < ctx->taps.nstyle; ++q) {
            const int l = ctx->taps.style[q];
            for (int r = 0; r < g.R; ++r) {
                if (gb.n == NST_GRAM_BATCH_MAX) NSTCHK(flush());
                const StyleTerm st = guided_term(ctx->taps, q, L.acts, sw, ctx->style_weight(q), g, r);
                GramItem& it = gb.it[gb.n++];
                it.f = L.acts.act[l]; it.N = st.N; it.C = st.C; it.amax = amax_act(L.acts, l);
                it.guide = g.plane(kScale[l], r, L.h, L.w);
                it.part = g.part + (size_t)r * g.part_floats_r + gram_part_offset(ctx->taps, L.h, L.w, q);
                it.divisor = (float)st.divisor; it.target = g.gram_t[q] + (size_t)r * st.C * st.C;
                it.coef = st.coef;
                it.gram_out = nullptr; it.S = g.S[q] + (size_t)r * st.C * st.C; it.S_bf = nullptr; it.S_amax = nullptr;
                it.mse_partial = g.partial[q] + (size_t)r * gram_finish_blocks(st.C);
                flops += 2.0 * (double)st.N * st.C * st.C;
            }
        }
    }
    NSTCHK(flush());
    for (int k = 0; k < n; ++k)
        for (int q = 0; q < ctx->taps.nstyle; ++q) NSTCHK(guided_fold(ctx, ctx->lv[lv[k]], q, s));
    return NST_OK;
}

int batched_gram(nst_ctx* ctx, const int* lv, int n, float sw, hipStream_t s, unsigned qmask) {
    const bool h2 = ctx->conv_mode == 2;
    if (guided_levels(ctx, lv, n)) return qmask ? batched_gram_guided(ctx, lv, n, sw, s) : NST_OK;
    if (h2) {
        // every (level, style layer) pair in one partial launch (two, one per tile shape, when shifted or with the Gram pack
        // switched off) and one finish launch
        const int per = std::max(1, NST_GRAM_BATCH_MAX / ctx->taps.nstyle);      // levels per launch (3 with five style maps)
        const bool shifted = ctx->gs_on();
        const bool moments = ctx->mom_on();
        for (int k0 = 0; k0 < n; k0 += per) {
            GramBatch gb{};
            OffsetBatch ob{};
            RowBiasBatch rb{};
            MomentBatch mb{};
            MomentFoldBatch mf{};
            double flops = 0;
            for (int k = k0; k < n && k < k0 + per; ++k) {
                LevelWs& L = ctx->lv[lv[k]];
                for (int q = 0; q < ctx->taps.nstyle; ++q) {
                    if (!((qmask >> q) & 1u)) continue;
                    const int l = ctx->taps.style[q];
                    const StyleTerm st = style_term(ctx->taps, q, L.acts, sw, ctx->style_weight(q));
                    GramItem& it = gb.it[gb.n++];
                    it.f = L.acts.act[l]; it.N = st.N; it.C = st.C; it.amax = amax_act(L.acts, l);
                    it.part = L.gram_part + gram_part_offset(ctx->taps, L.h, L.w, q);
                    it.divisor = (float)st.divisor; it.target = L.gram_t[q];
                    it.coef = st.coef;
                    // (S in bf16 pieces is conv_bf3's operand: the f16x2 launches that multiply by S cut the fp32 S themselves -
                    // conv_h2.hip takes wt2_f32 and never wt2_bf - so those 6 C^2 bytes per map are not written here;
                    // nst_ctx_set_forward_pack(0) writes them as before)
                    it.gram_out = nullptr; it.S = L.S[q]; it.S_bf = ctx->forward_pack ? nullptr : L.S_bf[q]; it.S_amax = amax_S(L.acts, q);
                    it.mse_partial = L.style_partial[q];
                    flops += 2.0 * (double)st.N * st.C * st.C;
                    if (shifted) {
                        // means -> SHIFT partial products -> finish -> row bias: the item reads o and the shifted operand's record
                        ob.it[ob.n++] = OffsetItem{it.f, it.N, it.C, it.amax, ctx->gs_shift_of(q), ctx->gs_center_of(q), L.gs.offset(q),
                                                   L.gs.amax(q), L.gs.part(q), 0, 0, 0};
                        rb.it[rb.n++] = RowBiasItem{L.gs.offset(q), L.S[q], L.gs.row_bias(q), it.C, 0};
                        it.offset = L.gs.offset(q); it.amax = L.gs.amax(q);
                    }
                    if (moments && ctx->mom_slot(q)) {
                        // channel sums of the map -> (after the Gram finish pass and r = o S) the fold into S and the row bias
                        mb.it[mb.n++] = moment_item(ctx, L, q, it.f, it.N, it.C);
                        mf.it[mf.n++] = moment_fold_item(ctx, L, q, it.N, it.C, it.S_bf, it.S_amax);
                    }
                }
            }
            if (gb.n == 0) continue;
            if (mb.n > 0) {
                Timer t(ctx, s, K_OTHER, 0);
                HIPCHK(ctx, launch_moment_stats(mb, s));
            }
            if (shifted) {
                Timer t(ctx, s, K_OTHER, 0);
                HIPCHK(ctx, launch_gram_offsets(ob, s));
            }
            {
                Timer t(ctx, s, K_GRAM, flops);
                HIPCHK(ctx, launch_gram_batch(gb, s, ctx->gram_pack));
            }
            if (shifted) {
                Timer t(ctx, s, K_OTHER, 0);
                HIPCHK(ctx, launch_gram_row_bias(rb, s));
            }
            if (mf.n > 0) {
                Timer t(ctx, s, K_OTHER, 0);
                HIPCHK(ctx, launch_moment_fold(mf, s));
            }
        }
    }
    for (int k = 0; k < n && !h2; ++k) {
        LevelWs& L = ctx->lv[lv[k]];
        for (int q = 0; q < ctx->taps.nstyle; ++q) {
            const StyleTerm st = style_term(ctx->taps, q, L.acts, sw, ctx->style_weight(q));
            NSTCHK(gram_of(ctx, GramOperand{L.acts.act[ctx->taps.style[q]], st.N, st.C, nullptr, nullptr, L.gram_part, (float)st.divisor},
                           GramFinish{L.gram_t[q], st.coef, L.S[q], L.S_bf[q], nullptr, L.style_partial[q]}, s));
        }
    }
    return NST_OK;
}

int batched_backward(nst_ctx* ctx, const float* const* xi, float* const* gi, const int* lv, int n, float cw, float tvw,
                     hipStream_t s, const Window* win, const float* win_means, double win_nx, double win_ny) {
    const bool h2 = ctx->conv_mode == 2;
    float* cur[NST_MAX_LEVELS]; float* oth[NST_MAX_LEVELS];
    for (int k = 0; k < n; ++k) { cur[k] = ctx->lv[lv[k]].gbuf[0]; oth[k] = ctx->lv[lv[k]].gbuf[1]; }
    const Taps& tp = ctx->taps;
    const int top = tp.top;
    const int top_q = tp.style_slot(top);
    const bool top_content = tp.content == top;
    // content gradient of level image k into dst (the content map's own shape), windowed or not
    auto content_grad = [&](int k, float* dst) -> int {
        LevelWs& L = ctx->lv[lv[k]];
        ActSet& a = L.acts;
        const int m = tp.content;
        Timer t(ctx, s, K_OTHER, 0);
        if (win) {
            // content gradient on the owned rows only (zero elsewhere), normalised by the full image's size
            const size_t off = (size_t)win_r0(*win, kScale[m]) * a.w[m] * kCout[m];
            const size_t cnt = (size_t)win_nr(*win, kScale[m]) * a.w[m] * kCout[m];
            const double n_all = (double)(win->H0 >> kScale[m]) * a.w[m] * kCout[m];
            HIPCHK(ctx, launch_zero(dst, L.content_n, s));
            HIPCHK(ctx, launch_mse_grad(a.act[m] + off, L.content_t + off, cnt, content_coef(cw, n_all), dst + off, L.content_partial, s));
        } else {
            HIPCHK(ctx, launch_mse_grad(a.act[m], L.content_t, L.content_n, content_coef(cw, (double)L.content_n), dst, L.content_partial, s));
        }
        return NST_OK;
    };
    if (top_content)
        for (int k = 0; k < n; ++k) NSTCHK(content_grad(k, oth[k]));
    // the per-map terms of the top map (a level's own), after the content gradient; top_add: the launch has an addend
    bool top_add[NST_MAX_LEVELS] = {};
    for (int k = 0; k < n; ++k) {
        top_add[k] = top_content;
        // (a content map alone at the top - no style slot - may carry the self-similarity term: onto its content gradient)
        if (top_q >= 0 || top_content) NSTCHK(map_terms_backward(ctx, ctx->lv[lv[k]], top, oth[k], top_add[k], s));
    }
    const bool guided = guided_levels(ctx, lv, n);
    if (guided && top_q >= 0) {
        // top of the chain of a guided job: the guided Gram backward of each level, which adds the content gradient (when
        // the top map is the content map too), applies the ReLU bit-mask (not for the pre-ReLU conv5_1) and records the absmax
        for (int k = 0; k < n; ++k) {
            LevelWs& L = ctx->lv[lv[k]];
            GuidedBwd gb = guided_bwd_of(ctx, L, top_q);
            gb.addend = top_content ? oth[k] : nullptr; gb.out = cur[k];
            gb.bits = tp.top_mask() ? L.acts.bits[top] : nullptr; gb.amax_out = amax_grad(L.acts, top);
            NSTCHK(launch_guided_backward(ctx, gb, s));
        }
    } else if (h2 && top_q >= 0) {
        // top of the chain: g(pre-ReLU of the top map) = mask(act * S (+ content gradient)) - the second K source of the
        // fp16 kernel on its own (no 3x3 part), one launch for all levels; its epilogue adds the content gradient (when the
        // top map is the content map too), applies the ReLU mask (not for the pre-ReLU conv5_1) and records the absmax
        const int l = top;
        ConvBatch b{};
        b.n = n; b.Cin = 0; b.Cout = kCout[l]; b.Cin2 = kCout[l]; b.relu = 0;
        conv_setup(ctx, b, 0, true);
        double flops = 0;
        for (int k = 0; k < n; ++k) {
            LevelWs& L = ctx->lv[lv[k]];
            ActSet& a = L.acts;
            ConvImage& im = b.img[k];
            im.out = cur[k]; im.H = a.h[l]; im.W = a.w[l];
            im.in2 = a.act[l]; im.wt2_f32 = L.S[top_q]; im.amax_in2 = amax_act(a, l); im.amax_w2 = amax_S(a, top_q);
            im.bits_in = tp.top_mask() ? a.bits[l] : nullptr; im.amax_out = amax_grad(a, l);
            im.addend = top_add[k] ? oth[k] : nullptr;
            im.bias = ctx->row_bias_of(L, top_q);      // (a shifted Gram, the moment term: F S + r, then the addend and the mask)
            if (win) { im.in2_row0 = win_r0(*win, kScale[l]); im.in2_rows = win_nr(*win, kScale[l]); }
            flops += conv_flops(im.H, im.W, b.Cin2, b.Cout, 1);
        }
        Timer t(ctx, s, K_GRAM, flops);
        NSTCHK(launch_conv_batch(ctx, b, t, false));
    }
    for (int k = 0; k < n && !((h2 || guided) && top_q >= 0); ++k) {
        LevelWs& L = ctx->lv[lv[k]];
        ActSet& a = L.acts;
        const int l = top;
        const size_t cnt = (size_t)a.h[l] * a.w[l] * kCout[l];
        if (top_q >= 0) {
            ConvParams p{};
            p.in = a.act[l]; p.wt = L.S[top_q]; p.out = cur[k]; p.mask = tp.top_mask() ? a.act[l] : nullptr;
            p.addend = top_add[k] ? oth[k] : nullptr;
            p.H = a.h[l]; p.W = a.w[l]; p.Cin = kCout[l]; p.Cout = kCout[l];
            Timer t(ctx, s, K_GRAM, conv_flops(p.H, p.W, p.Cin, p.Cout, 1));
            HIPCHK(ctx, launch_conv_mfma(p, 1, s));
        } else {
            // the content map alone at the top: its gradient through the ReLU mask
            Timer t(ctx, s, K_OTHER, 0);
            if (tp.top_mask()) HIPCHK(ctx, launch_relu_mask(a.act[l], oth[k], cnt, cur[k], s));
            else HIPCHK(ctx, launch_copy(oth[k], cur[k], cnt, s));
        }
        if (h2) HIPCHK(ctx, launch_absmax_slots(cur[k], cnt, amax_grad(a, l), s));
    }
    for (int l = top; l >= 1; --l) {
        const int pk = pool_index_after(l - 1);
        const int m = l - 1;
        const int style_q = tp.style_slot(m);
        ConvBatch b{};
        b.n = n; b.bias = nullptr; b.Cin = kCout[l]; b.Cout = kCin[l]; b.relu = 0;
        conv_setup(ctx, b, l, true);
        // f16x2: when a max-pool follows layer l, cur[] holds the gradient w.r.t. the POOLED map and this launch's
        // loader un-pools it through the arg-max code (no un-pool kernel, no full-size gradient round trip)
        const int pl = pool_index_after(l);
        b.unpool = (h2 && pl >= 0) ? 1 : 0;
        // average pooling: every position whose code bit is on gets a QUARTER of the pooled gradient.  The loader hands the
        // pooled gradient through as it is (same loads, same selects, a multi-hot code) and the 1/4 rides on the scale the
        // launch multiplies its accumulators by: exact (a power of two), and the second K source - re-expressed in the main
        // source's scale through the same factor - comes out unchanged.  The launch records the absmax of what it stores.
        if (b.unpool && ctx->pool_avg) { b.wt_h2_inv *= 0.25f; b.wt_wino_inv *= 0.25f; }
        b.Cin2 = (pk < 0 && style_q >= 0 && !guided) ? kCout[m] : 0;      // (a guided job: the addend carries the style gradient)
        double flops = 0;
        for (int k = 0; k < n; ++k) {
            LevelWs& L = ctx->lv[lv[k]];
            ActSet& a = L.acts;
            ConvImage& im = b.img[k];
            im.in = cur[k]; im.out = oth[k]; im.H = a.h[l]; im.W = a.w[l];
            im.pcode_in = b.unpool ? a.pcode[pl] : nullptr;
            im.amax_in = amax_grad(a, l); im.amax_out = amax_grad(a, l - 1);
            flops += conv_flops(im.H, im.W, b.Cin, b.Cout, 9);
            if (pk >= 0) continue;
            // a map that is both a style and the content map: the Gram term as the second K source AND the content
            // gradient as the addend of the same launch
            if (style_q >= 0 && guided) {
                // the guided Gram backward of the map into oth[k], onto the content gradient when the map is the content
                // map too; the launch below takes it as its addend and carries no second K source
                GuidedBwd gb = guided_bwd_of(ctx, L, style_q);
                if (m == tp.content) { NSTCHK(content_grad(k, oth[k])); gb.addend = oth[k]; }
                gb.out = oth[k];
                NSTCHK(launch_guided_backward(ctx, gb, s));
                im.addend = oth[k];
                im.bits_in = a.bits[m];
                continue;
            }
            if (style_q >= 0) {
                im.in2 = a.act[m]; im.wt2_bf = L.S_bf[style_q];
                im.wt2_f32 = L.S[style_q]; im.amax_in2 = amax_act(a, m); im.amax_w2 = amax_S(a, style_q);
                im.bias = ctx->row_bias_of(L, style_q);
                if (win) { im.in2_row0 = win_r0(*win, kScale[m]); im.in2_rows = win_nr(*win, kScale[m]); }
                flops += conv_flops(a.h[m], a.w[m], kCout[m], kCout[m], 1);
            }
            if (m == tp.content) {
                NSTCHK(content_grad(k, oth[k]));
                im.addend = oth[k];
            }
            // the per-map terms of the map, after the content gradient when the map is the content map too
            bool held = im.addend == oth[k];
            NSTCHK(map_terms_backward(ctx, L, m, oth[k], held, s));
            if (held) im.addend = oth[k];
            im.bits_in = a.bits[m];
        }
        {
            Timer t(ctx, s, K_CONV3, flops, b.img[0].H, b.img[0].W, b.Cin, b.Cout, 9, -l);
            NSTCHK(launch_conv_batch(ctx, b, t, !win));
        }
        for (int k = 0; k < n; ++k) {
            ActSet& a = ctx->lv[lv[k]].acts;
            if (pk >= 0 && !h2) {
                Timer t(ctx, s, K_OTHER, 0);
                HIPCHK(ctx, launch_pool_bwd_relu(ctx, a.act[l - 1], oth[k], a.h[l - 1], a.w[l - 1], kCout[l - 1], cur[k], s));
            } else {
                float* tmp = cur[k]; cur[k] = oth[k]; oth[k] = tmp;
            }
        }
    }
    for (int k = 0; k < n; ++k) {
        LevelWs& L = ctx->lv[lv[k]];
        {
            Timer t(ctx, s, K_CONV1, conv_flops(L.h, L.w, 64, 3, 9));
            HIPCHK(ctx, launch_conv1_1_dgrad(cur[k], L.h, L.w, ctx->w11d, h2 ? amax_grad(L.acts, 0) : nullptr, gi[lv[k]], s,
                                             ctx->channels));
        }
        Timer t(ctx, s, K_OTHER, 0);
        if (win)
            HIPCHK(ctx, launch_tv_finish(xi[lv[k]], ctx->channels, L.h, L.w, L.tv_partial, tvw, gi[lv[k]], 1, nullptr, s, win->row0, win->rows,
                                         win_means, win_nx, win_ny));
        else
            HIPCHK(ctx, launch_tv_finish(xi[lv[k]], ctx->channels, L.h, L.w, L.tv_partial, tvw, gi[lv[k]], 1, L.tv_means, s));
        if (!win) NSTCHK(lap_backward(ctx, L, gi[lv[k]], s));
        if (!win) NSTCHK(mat_backward(ctx, L, xi[lv[k]], gi[lv[k]], s));
        if (!win) NSTCHK(anchor_backward(ctx, L, xi[lv[k]], gi[lv[k]], s));
    }
    return NST_OK;
}

// The batched closure of the levels in `level_mask` in two halves that meet where the stripe closure splits too: the
// forward half leaves every activation, ReLU bit-mask, pool code, absmax record and S matrix in the level workspaces, the
// backward half reads them.  closure_batched runs one after the other; nst_closure_forward / nst_closure_backward run them
// apart.
int level_list(const nst_ctx* ctx, unsigned level_mask, int* lv) {
    int n = 0;
    for (int i = 0; i < ctx->levels; ++i)
        if ((level_mask >> i) & 1u) lv[n++] = i;
    return n;
}
// forward convolutions and every Gram launch, the side-stream overlap joined.  `loss_terms` (a forward half on its own):
// also the content SSE partials and the TV means of the loss row, by the launches the backward half produces them with
// (same kernels, same per-block reduction order, no gradient write), which that half then writes again.
int closure_batched_forward(nst_ctx* ctx, const float* const* xi, unsigned level_mask, float sw, float tvw, hipStream_t s,
                            bool loss_terms) {
    int lv[NST_MAX_LEVELS];
    const int n = level_list(ctx, level_mask, lv);
    if (n == 0) return NST_OK;
    // (not while a hipGraph is being captured or replayed: the closure then stays on one stream)
    // (the overlap's split of the style maps - relu1_1 .. relu3_1 on the side stream - is the default taps')
    const bool overlap = ctx->gram_overlap && ctx->conv_mode == 2 && !ctx->use_graph && ctx->side != nullptr && ctx->taps.is_default &&
                         !guided_levels(ctx, lv, n);
    // the Laplacian term's residuals and partials (nst_job_set_laplacian): pixel space, beside the TV partials
    for (int k = 0; k < n; ++k) NSTCHK(lap_forward(ctx, ctx->lv[lv[k]], xi[lv[k]], false, s));
    for (int k = 0; k < n; ++k) NSTCHK(mat_forward(ctx, ctx->lv[lv[k]], xi[lv[k]], s));       // (nst_job_set_matting: likewise)
    for (int k = 0; k < n; ++k) NSTCHK(anchor_forward(ctx, ctx->lv[lv[k]], xi[lv[k]], s));    // (nst_level_set_anchor: likewise)
    NSTCHK(batched_forward(ctx, xi, lv, n, s, nullptr, overlap ? sw : -1.f));
    NSTCHK(batched_gram(ctx, lv, n, sw, s, overlap ? 0x18u : (1u << ctx->taps.nstyle) - 1u));
    if (overlap) HIPCHK(ctx, hipStreamWaitEvent(s, ctx->side_join, 0));
    NSTCHK(map_terms_forward(ctx, lv, n, s));        // (the per-map terms: the maps exist)
    if (loss_terms && ctx->forward_pack && ctx->conv_mode == 2 && !ctx->use_graph && n > 1) {
        // one launch each for all levels; every level keeps its partial buffers and block decomposition
        MseBatch mb{};
        TvBatch tb{};
        mb.n = tb.n = n;
        tb.C = ctx->channels;
        for (int k = 0; k < n; ++k) {
            LevelWs& L = ctx->lv[lv[k]];
            mb.a[k] = L.acts.act[ctx->taps.content]; mb.t[k] = L.content_t; mb.cnt[k] = L.content_n; mb.partial[k] = L.content_partial;
            tb.y[k] = xi[lv[k]]; tb.h[k] = L.h; tb.w[k] = L.w; tb.partial[k] = L.tv_partial; tb.means[k] = L.tv_means;
        }
        Timer t(ctx, s, K_OTHER, 0);
        HIPCHK(ctx, launch_mse_partial_batch(mb, s));
        HIPCHK(ctx, launch_tv_means_batch(tb, s));
        return NST_OK;
    }
    for (int k = 0; k < n && loss_terms; ++k) {
        LevelWs& L = ctx->lv[lv[k]];
        Timer t(ctx, s, K_OTHER, 0);
        HIPCHK(ctx, launch_mse_grad(L.acts.act[ctx->taps.content], L.content_t, L.content_n, 0.f, nullptr, L.content_partial, s));
        HIPCHK(ctx, launch_tv_finish(xi[lv[k]], ctx->channels, L.h, L.w, L.tv_partial, tvw, nullptr, 1, L.tv_means, s));
    }
    return NST_OK;
}
// `zero_mask`: the levels whose gradient this call clears when they are not in `level_mask` (levels another rank owns)
int closure_batched_backward(nst_ctx* ctx, const float* const* xi, float* const* gi, unsigned level_mask, float cw, float tvw,
                             hipStream_t s, unsigned zero_mask) {
    for (int i = 0; i < ctx->levels; ++i)
        if (!((level_mask >> i) & 1u) && ((zero_mask >> i) & 1u))
            HIPCHK(ctx, launch_zero(gi[i], (size_t)ctx->channels * ctx->lv[i].h * ctx->lv[i].w, s));
    int lv[NST_MAX_LEVELS];
    const int n = level_list(ctx, level_mask, lv);
    if (n == 0) return NST_OK;
    return batched_backward(ctx, xi, gi, lv, n, cw, tvw, s, nullptr, nullptr, 0, 0);
}
int closure_batched(nst_ctx* ctx, const float* const* xi, float* const* gi, unsigned level_mask, float cw, float sw,
                    float tvw, hipStream_t s, unsigned zero_mask = ~0u) {
    NSTCHK(closure_batched_forward(ctx, xi, level_mask, sw, tvw, s, false));
    return closure_batched_backward(ctx, xi, gi, level_mask, cw, tvw, s, zero_mask);
}

bool batch_eligible(const nst_ctx* ctx) {
    // needs the bf16 conv kernels (32-bit buffer offsets) and enough tiles to be worth it
    return ctx->batched && ctx->conv_mode && (size_t)ctx->lv[0].h * ctx->lv[0].w * 64 * 4 < 0xFFFFFF00ull &&
           (ctx->levels > 1 || (size_t)ctx->lv[0].h * ctx->lv[0].w >= (size_t)256 * 256);
}

// ---- closure of ONE pyramid level by the per-level walker, on stream s (the counterpart of closure_batched) ------------
int closure_per_level(nst_ctx* ctx, const float* const* xi, float* const* gi, int level, float cw, float sw, float tvw,
                      hipStream_t s) {
    LevelWs& L = ctx->lv[level];
    const Taps& tp = ctx->taps;
    const bool h2 = ctx->conv_mode == 2;
    {
        Timer t(ctx, s, K_OTHER, 0);
        HIPCHK(ctx, launch_tv_partial(xi[level], ctx->channels, L.h, L.w, L.tv_partial, s));
    }
    NSTCHK(lap_forward(ctx, L, xi[level], false, s));
    NSTCHK(mat_forward(ctx, L, xi[level], s));
    NSTCHK(anchor_forward(ctx, L, xi[level], s));
    NSTCHK(forward(ctx, L.acts, xi[level], L.h, L.w, s, tp.top, ctx->channels));
    Inject inj[NL];
    GuidedBwd gbw[kMaxStyle];
    for (int k = 0; k < tp.nstyle && L.guide.R > 0; ++k) {
        // guided: R Gram matrices per map through the one slab workspace, then the map's loss partials
        const int l = tp.style[k];
        const Guidance& g = L.guide;
        for (int r = 0; r < g.R; ++r) {
            const StyleTerm st = guided_term(tp, k, L.acts, sw, ctx->style_weight(k), g, r);
            NSTCHK(gram_of(ctx, GramOperand{L.acts.act[l], st.N, st.C, amax_act(L.acts, l), g.plane(kScale[l], r, L.h, L.w), g.part, (float)st.divisor},
                           GramFinish{g.gram_t[k] + (size_t)r * st.C * st.C, st.coef, g.S[k] + (size_t)r * st.C * st.C, nullptr, nullptr,
                                      g.partial[k] + (size_t)r * gram_finish_blocks(st.C)}, s));
        }
        NSTCHK(guided_fold(ctx, L, k, s));
        gbw[k] = guided_bwd_of(ctx, L, k);
        inj[l].guided = &gbw[k];
    }
    for (int k = 0; k < tp.nstyle && L.guide.R == 0; ++k) {
        const int l = tp.style[k];
        const StyleTerm st = style_term(tp, k, L.acts, sw, ctx->style_weight(k));
        const GramOperand op{L.acts.act[l], st.N, st.C, h2 ? amax_act(L.acts, l) : nullptr, nullptr, L.gram_part, (float)st.divisor};
        const GramFinish fin{L.gram_t[k], st.coef, L.S[k], L.S_bf[k], h2 ? amax_S(L.acts, k) : nullptr, L.style_partial[k]};
        if (ctx->gs_on()) {
            const ShiftedGram sg{ctx->gs_shift_of(k), ctx->gs_center_of(k), L.gs.offset(k), L.gs.amax(k), L.gs.part(k), L.gs.row_bias(k)};
            NSTCHK(gram_shifted_of(ctx, op, sg, fin, s));
        } else {
            NSTCHK(gram_of(ctx, op, fin, s));
        }
        if (ctx->mom_on() && ctx->mom_slot(k)) {
            MomentBatch mb{};
            MomentFoldBatch mf{};
            mb.n = mf.n = 1;
            mb.it[0] = moment_item(ctx, L, k, L.acts.act[l], st.N, st.C);
            mf.it[0] = moment_fold_item(ctx, L, k, st.N, st.C, L.S_bf[k], h2 ? amax_S(L.acts, k) : nullptr);
            Timer t(ctx, s, K_OTHER, 0);
            HIPCHK(ctx, launch_moment_stats(mb, s));
            HIPCHK(ctx, launch_moment_fold(mf, s));
        }
        inj[l].bias = ctx->row_bias_of(L, k);
        inj[l].S = L.S[k];
        inj[l].S_bf = L.S_bf[k];
        inj[l].S_amax = h2 ? amax_S(L.acts, k) : nullptr;
    }
    inj[tp.content].content = true;
    // the per-map terms: matches, tables and values now, the gradients as addends of the walk
    NSTCHK(map_terms_forward(ctx, &level, 1, s));
    ContentJob cj{L.content_t, L.content_n, content_coef(cw, (double)L.content_n), L.content_partial};
    NSTCHK(backward(ctx, L.acts, inj, &cj, L.gbuf[0], L.gbuf[1], gi[level], L.h, L.w, s, tp.top, tp.top_mask(), ctx->channels, &L));
    {
        Timer t(ctx, s, K_OTHER, 0);
        HIPCHK(ctx, launch_tv_finish(xi[level], ctx->channels, L.h, L.w, L.tv_partial, tvw, gi[level], 1, L.tv_means, s));
    }
    NSTCHK(lap_backward(ctx, L, gi[level], s));
    NSTCHK(mat_backward(ctx, L, xi[level], gi[level], s));
    return anchor_backward(ctx, L, xi[level], gi[level], s);
}

// what the loss-assembly kernel reads: every level's partial sums and normalisers; the rows of levels not in level_mask are zeros
LossAssembly fill_loss_assembly(const nst_ctx* ctx, unsigned level_mask, float cw, float sw, float tvw, float* losses) {
    LossAssembly la{};
    la.levels = ctx->levels; la.nstyle = ctx->taps.nstyle; la.cw = cw; la.sw = sw; la.tvw = tvw; la.out = losses;
    for (int i = 0; i < ctx->levels; ++i) {
        const LevelWs& L = ctx->lv[i];
        la.lv[i].content_partial = L.content_partial;
        la.lv[i].content_n = L.content_n;
        for (int k = 0; k < ctx->taps.nstyle; ++k) { la.lv[i].style_partial[k] = L.style_partial[k]; la.lv[i].style_c[k] = kCout[ctx->taps.style[k]]; la.lv[i].style_w[k] = ctx->style_weight(k); }
        la.lv[i].tv_means = L.tv_means;
        la.lv[i].owned = (int)((level_mask >> i) & 1u);
        for (int k = 0; k < ctx->lap_k; ++k) { la.lv[i].lap_partial[k] = L.lap.partial[k]; la.lv[i].lap_n[k] = lap_n(L, ctx->lap_pool[k]); }
    }
    la.nlap = ctx->lap_k; la.lap_out = ctx->lv[0].lap.vals;
    la.mat_gamma = ctx->mat_gamma; la.mat_out = ctx->lv[0].mat.vals;
    for (int i = 0; i < ctx->levels && ctx->mat_gamma > 0.f; ++i) {
        const LevelWs& L = ctx->lv[i];
        la.lv[i].mat_partial = L.mat.partial; la.lv[i].mat_tiles = L.mat.tiles; la.lv[i].mat_n = mat_n(ctx, L);
    }
    for (int k = 0; k < ctx->lap_k; ++k) la.lap_gamma[k] = ctx->lap_gamma[k];
    la.mom_on = ctx->mom_on() ? 1 : 0; la.mom_out = ctx->lv[0].mom.vals; la.mom_stride = MOM_STAT_STRIDE;
    for (int k = 0; k < ctx->taps.nstyle && la.mom_on; ++k) {
        la.mom_wm[k] = ctx->mom_wm_of(k); la.mom_ws[k] = ctx->mom_ws_of(k); la.mom_index[k] = tap_index_of(ctx->taps.style[k]);
    }
    for (int i = 0; i < ctx->levels && la.mom_on; ++i) la.lv[i].mom_loss = ctx->lv[i].mom.stats ? ctx->lv[i].mom.loss(0) : nullptr;
    for (int i = 0; i < ctx->levels; ++i) {      // (a level's own: la{} left the levels without an anchor at gamma = 0)
        const LevelWs& L = ctx->lv[i];
        if (!(L.anc.gamma > 0.f)) continue;
        la.lv[i].tmp_partial = L.anc.partial; la.lv[i].tmp_gamma = L.anc.gamma; la.lv[i].tmp_n = anchor_n(ctx, L); la.lv[i].tmp_out = L.anc.val;
    }
    for (int i = 0; i < ctx->levels; ++i) {      // (a level's own: la{} left the levels without a per-map term at nullptr)
        for (int t = 0; t < NST_MAP_TERMS; ++t) {
            const MapTerm& g = ctx->lv[i].map_term(t);
            if (!g.on()) continue;
            la.lv[i].term[t].vals = g.vals;
            for (int k = 0; k < 6; ++k) la.lv[i].term[t].w[k] = g.w[k];
        }
    }
    return la;
}

// enqueues the closure on `main` (no host synchronisation; capturable unless it forks level streams): all of it, or - the
// batched schedule only - one of its halves.  FORWARD: pyramid, forward, Gram, loss row (`grad` unused); BACKWARD: the
// backward of the forward half the level workspaces still hold, and the bicubic-transpose chain (`losses` unused)
enum Half { WHOLE = 0, FORWARD = 1, BACKWARD = 2 };
int closure_record(nst_ctx* ctx, const float* x, float cw, float sw, float tvw, unsigned level_mask, float* grad,
                   float* losses, hipStream_t main, Half half = WHOLE) {
    const bool batch = batch_eligible(ctx);
    if (!batch && half != WHOLE) return fail(ctx, NST_E_STATE, "the closure halves run on the batched schedule only");
    // pyramid of the optimised image (neural_style_transfer.py:170-176)
    const float* xi[NST_MAX_LEVELS];
    float* gi[NST_MAX_LEVELS];
    xi[0] = x; gi[0] = grad;
    for (int i = 1; i < ctx->levels; ++i) {
        LevelWs& L = ctx->lv[i];
        xi[i] = L.img.xl; gi[i] = L.img.gxl;
        if (half == BACKWARD) continue;      // (the forward half left the level images in place)
        Timer t(ctx, main, K_OTHER, 0);
        HIPCHK(ctx, launch_bicubic_down(xi[i - 1], ctx->channels, ctx->lv[i - 1].h, ctx->lv[i - 1].w, L.h, L.w, L.img.xl, main));
    }
    // the levels in `mask` on stream s
    auto batched = [&](unsigned mask, hipStream_t s, unsigned zero_mask) -> int {
        if (half == WHOLE) return closure_batched(ctx, xi, gi, mask, cw, sw, tvw, s, zero_mask);
        if (half == FORWARD) return closure_batched_forward(ctx, xi, mask, sw, tvw, s, true);
        return closure_batched_backward(ctx, xi, gi, mask, cw, tvw, s, zero_mask);
    };
    if (batch) {
        const unsigned top = level_mask & 1u, rest = level_mask & ~1u;
        if (ctx->level_split && ctx->side && !ctx->use_graph && top && rest) {
            // nst_options.level_split: the top level's chain on the caller's stream, the lower levels' (batched among
            // themselves) on the side stream - two chains of unequal size whose launch ramps, tails and epilogue bursts can
            // fill one another, as two jobs on one GPU do.  Same kernels on the same tiles: bitwise the same.
            HIPCHK(ctx, hipEventRecord(ctx->side_fork, main));
            HIPCHK(ctx, hipStreamWaitEvent(ctx->side, ctx->side_fork, 0));
            ++ctx->sched.side_forks;
            NSTCHK(batched(top, main, 1u));
            NSTCHK(batched(rest, ctx->side, ~1u));
            HIPCHK(ctx, hipEventRecord(ctx->side_join, ctx->side));
            HIPCHK(ctx, hipStreamWaitEvent(main, ctx->side_join, 0));
        } else {
            NSTCHK(batched(level_mask, main, ~0u));
        }
    }
    const bool multi = !batch && !ctx->single_stream && ctx->levels > 1;
    if (multi) {
        // the per-level streams exist only for this schedule (a stream costs device memory that HIP does not hand back)
        for (int i = 0; i < ctx->levels; ++i) {
            LevelWs& L = ctx->lv[i];
            if (!L.stream) HIPCHK(ctx, hipStreamCreateWithFlags(&L.stream, hipStreamNonBlocking));
            if (!L.done) HIPCHK(ctx, hipEventCreateWithFlags(&L.done, hipEventDisableTiming));
        }
        HIPCHK(ctx, hipEventRecord(ctx->fork, main));
        ctx->sched.level_streams = ctx->levels;
    }
    for (int i = 0; i < ctx->levels && !batch; ++i) {
        LevelWs& L = ctx->lv[i];
        hipStream_t s = multi ? L.stream : main;
        if (multi) HIPCHK(ctx, hipStreamWaitEvent(s, ctx->fork, 0));
        // (a level another rank owns contributes nothing here: its gradient arrives by all-reduce)
        if ((level_mask >> i) & 1u) NSTCHK(closure_per_level(ctx, xi, gi, i, cw, sw, tvw, s));
        else HIPCHK(ctx, launch_zero(gi[i], (size_t)ctx->channels * L.h * L.w, s));
        if (multi) HIPCHK(ctx, hipEventRecord(L.done, s));
    }
    if (multi)
        for (int i = 0; i < ctx->levels; ++i) HIPCHK(ctx, hipStreamWaitEvent(main, ctx->lv[i].done, 0));

    // pull the coarse-level gradients back up the bicubic chain (autograd of :173-176)
    for (int i = ctx->levels - 1; i >= 1 && half != FORWARD; --i) {
        Timer t(ctx, main, K_OTHER, 0);
        HIPCHK(ctx, launch_bicubic_down_bwd(gi[i], ctx->channels, ctx->lv[i - 1].h, ctx->lv[i - 1].w, ctx->lv[i].h, ctx->lv[i].w,
                                            gi[i - 1], 1, main));
    }
    if (half != BACKWARD) HIPCHK(ctx, launch_loss_assemble(fill_loss_assembly(ctx, level_mask, cw, sw, tvw, losses), main));
    if (half != BACKWARD) NSTCHK(xcorr_loss_rows(ctx, level_mask, losses, main));
    return NST_OK;
}

// the levels of a closure call have their targets: the guided ones those of their R regions (nst_level_set_targets_guided),
// and they are all guided or all unguided
int closure_targets_check(nst_ctx* ctx, unsigned level_mask) {
    int guided = 0, plain = 0;
    for (int i = 0; i < ctx->levels; ++i) {
        if (!((level_mask >> i) & 1u)) continue;
        const LevelWs& L = ctx->lv[i];
        if (L.guide.R > 0) {
            ++guided;
            if (!L.guide.targets || L.guide.targets_R != L.guide.R)
                return fail(ctx, NST_E_STATE, "guided targets of level " + std::to_string(i) + " not set (nst_level_set_targets_guided)");
        } else {
            ++plain;
            if (!L.targets) return fail(ctx, NST_E_STATE, "targets of level " + std::to_string(i) + " not set");
        }
    }
    if (guided && plain) return fail(ctx, NST_E_STATE, "the levels of one closure are all guided or all unguided (nst_level_set_guidance)");
    return NST_OK;
}

// The content target of a level: the content map (default ReLU(conv4_2)) of the content image, through the level's own
// activation buffers - by the launches the closure of this job will use (one launch per layer, Winograd F(2,3) where it
// applies), so that target and current features carry the same rounding: an image that IS the content image then has a
// content loss of (all but) exactly zero, as in the reference, whose target and current features come from one and the
// same forward code
int set_content_target(nst_ctx* ctx, int level, const float* content, hipStream_t s) {
    LevelWs& L = ctx->lv[level];
    const Taps& tp = ctx->taps;
    if (batch_eligible(ctx)) {
        const float* xi[NST_MAX_LEVELS] = {};
        xi[level] = content;
        const int lv1 = level;
        NSTCHK(batched_forward(ctx, xi, &lv1, 1, s, nullptr));
    } else {
        NSTCHK(forward(ctx, L.acts, content, L.h, L.w, s, tp.content, ctx->channels));
    }
    HIPCHK(ctx, hipMemcpyAsync(L.content_t, L.acts.act[tp.content], L.content_n * 4, hipMemcpyDeviceToDevice, s));
    return NST_OK;
}

// The guidance pyramid of (R,h,w) planes (already at dst + off[0]) and its masses: the four pooling steps, the mass of every
// scale, then a wait for `s` and the read-back.  dscratch: (R GUIDE_MASS_BLOCKS + 5 R) * 2 device doubles.  bad: how many
// values of the level planes are outside [0,1] or not finite.
void guidance_offsets(int R, int h, int w, size_t off[6]) {
    off[0] = 0;
    for (int sc = 0; sc < 5; ++sc) off[sc + 1] = off[sc] + (size_t)R * (h >> sc) * (w >> sc);
}
int build_guidance(nst_ctx* ctx, float* dst, const size_t* off, int R, int h, int w, double* dscratch, double mass[5][NST_MAX_REGIONS],
                   double* bad, hipStream_t s) {
    double* out = dscratch + (size_t)R * GUIDE_MASS_BLOCKS * 2;
    for (int sc = 0; sc < 5; ++sc) {
        if (sc > 0) HIPCHK(ctx, launch_guide_pool(dst + off[sc - 1], R, h >> (sc - 1), w >> (sc - 1), dst + off[sc], s));
        HIPCHK(ctx, launch_guide_mass(dst + off[sc], R, (size_t)(h >> sc) * (w >> sc), dscratch, out + (size_t)sc * R * 2, s));
    }
    double host[5 * NST_MAX_REGIONS * 2];
    HIPCHK(ctx, hipMemcpyAsync(host, out, (size_t)5 * R * 2 * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    *bad = 0.0;
    for (int sc = 0; sc < 5; ++sc)
        for (int r = 0; r < R; ++r) {
            mass[sc][r] = host[((size_t)sc * R + r) * 2];
            if (sc == 0) *bad += host[((size_t)sc * R + r) * 2 + 1];
        }
    return NST_OK;
}
// every (map in use, region) carries at least one pixel's worth of guidance
bool guidance_mass_ok(const Taps& tp, const double mass[5][NST_MAX_REGIONS], int R) {
    for (int q = 0; q < tp.nstyle; ++q)
        for (int r = 0; r < R; ++r)
            if (!(mass[kScale[tp.style[q]]][r] >= 1.0)) return false;
    return true;
}

int window_check(nst_ctx* ctx, const float* xs, int row0, int rows, int H0) {
    if (ctx->levels != 1) return fail(ctx, NST_E_STATE, "a stripe context is configured with levels_num = 1");
    if (ctx->conv_mode != 2) return fail(ctx, NST_E_STATE, "the stripe closure runs on the f16x2 convolutions (NST_CONV unset)");
    if (!ctx->taps.is_default)
        return fail(ctx, NST_E_STATE, "the stripe closure implements the default feature maps only (nst_job_set_taps(ctx, 4, 0x2F, 1))");
    if (ctx->channels != 3)
        return fail(ctx, NST_E_STATE, "the stripe closure implements RGB only (nst_job_set_color(ctx, NST_COLOR_RGB))");
    if (ctx->pool_avg)
        return fail(ctx, NST_E_STATE, "the stripe closure implements max pooling only (nst_job_set_pooling(ctx, NST_POOL_MAX))");
    if (!ctx->unit_style_weights())
        return fail(ctx, NST_E_STATE, "the stripe closure implements unit style layer weights only (nst_job_set_style_weights)");
    if (ctx->lap_k > 0)
        return fail(ctx, NST_E_STATE, "the stripe closure implements no Laplacian loss (nst_job_set_laplacian(ctx, 0, NULL, NULL) switches it off)");
    if (ctx->mat_gamma > 0.f)
        return fail(ctx, NST_E_STATE, "the stripe closure implements no matting term (nst_job_set_matting(ctx, 0, epsilon) switches it off)");
    if (ctx->gs_on())
        return fail(ctx, NST_E_STATE, "the stripe closure implements the plain Gram statistic only (nst_job_set_gram_shift with zeros switches the shift off)");
    if (ctx->mom_on())
        return fail(ctx, NST_E_STATE, "the stripe closure implements no moment loss (nst_job_set_moments with zeros switches it off)");
    LevelWs& L = ctx->lv[0];
    if (L.anc.gamma > 0.f)
        return fail(ctx, NST_E_STATE, "the stripe closure implements no temporal term (nst_level_set_anchor(ctx, 0, NULL, NULL, 0, stream) clears it)");
    if (L.pm.on())
        return fail(ctx, NST_E_STATE, "the stripe closure implements no MRF term (nst_level_set_patches(ctx, 0, NULL, ...) clears it)");
    if (L.hist.on())
        return fail(ctx, NST_E_STATE, "the stripe closure implements no histogram loss (nst_level_set_histograms(ctx, 0, NULL, ...) clears it)");
    if (L.remd.on())
        return fail(ctx, NST_E_STATE, "the stripe closure implements no relaxed EMD term (nst_level_set_remd(ctx, 0, NULL, ...) clears it)");
    if (L.selfsim.on())
        return fail(ctx, NST_E_STATE, "the stripe closure implements no self-similarity term (nst_level_set_selfsim(ctx, 0, NULL, ...) clears it)");
    if (L.xcorr.on())
        return fail(ctx, NST_E_STATE, "the stripe closure implements no xcorr term (nst_level_set_xcorr(ctx, 0, NULL, ...) clears it)");
    if (L.guide.R > 0)
        return fail(ctx, NST_E_STATE, "the stripe closure implements no spatial control (nst_level_set_guidance(ctx, 0, 0, ...) clears it)");
    if (!L.targets) return fail(ctx, NST_E_STATE, "targets of the stripe not set");
    if (!xs) return fail(ctx, NST_E_ARG, "null buffer");
    // boundaries between stripes on multiples of 16 rows (pooling alignment); only a stripe that ends with the stripe
    // image - the bottom of the full image - may own a ragged last row group
    const bool to_bottom = (row0 + rows == L.h);
    if (row0 < 0 || rows < 16 || row0 % 16 || (!to_bottom && rows % 16) || row0 + rows > L.h || H0 < L.h)
        return fail(ctx, NST_E_ARG, "stripe rows: start and interior boundaries on multiples of 16 rows, inside the stripe image");
    if ((size_t)L.h * L.w * 64 * 4 >= 0xFFFFFF00ull) return fail(ctx, NST_E_ARG, "stripe image too large for the f16x2 kernels");
    return NST_OK;
}

}  // namespace

namespace nst {

int restore_map(nst_ctx* ctx, int level, int layer, hipStream_t s) {
    ActSet& a = ctx->lv[level].acts;
    // the map is there; or nothing to repeat: no pass since the job was set up, or one that stopped below this layer
    if (a.stored[layer] || a.pass == 0 || layer > ctx->taps.top) return NST_OK;
    // the launch covers every level of that pass: all of them must still hold it (its inputs, and what it rewrites)
    bool whole = a.pass_n >= 1;
    for (int k = 0; k < a.pass_n; ++k) whole = whole && ctx->lv[a.pass_lv[k]].acts.pass == a.pass;
    if (!whole)
        return fail(ctx, NST_E_STATE, "the level's last forward pass left this map out and a later pass has run over some of its levels: "
                                      "evaluate the level again, or set keep_all_maps");
    int lv[NST_MAX_LEVELS];
    for (int k = 0; k < a.pass_n; ++k) lv[k] = a.pass_lv[k];
    double flops = 0;
    const ConvBatch b = forward_batch(ctx, lv, a.pass_n, layer, true, &flops);
    return launch_conv_batch(ctx, b, s, nullptr, true);
}

}  // namespace nst

// ================================================================================================
extern "C" {

// The targets of one level from K style images blended per map (include/nst_hip.h has the definition).  nst_level_set_targets
// is its K = 1 case: one image, b^ = 1 on every map, whose alpha = 1 finish writes the bits the plain finish pass writes.
int nst_level_set_targets_blend(nst_ctx* ctx, int level, const float* content, int K, const float* const* styles, const int* hs,
                                const int* ws, const float* blend, void* stream) {
    if (ctx) { ++ctx->closure_epoch; ++ctx->ws_seq; }
    NSTCHK(bind(ctx));
    if (level < 0 || level >= ctx->levels) return fail(ctx, NST_E_STATE, "level not configured");
    if (K < 1 || K > NST_MAX_STYLES) return fail(ctx, NST_E_ARG, "the number of style images must be 1 .. NST_MAX_STYLES");
    if (!content || !styles || !hs || !ws || !blend) return fail(ctx, NST_E_ARG, "null argument");
    for (int k = 0; k < K; ++k) {
        if (!styles[k]) return fail(ctx, NST_E_ARG, "null image");
        if (hs[k] < 16 || ws[k] < 16) return fail(ctx, NST_E_ARG, "style image must be at least 16x16");
    }
    for (int i = 0; i < K * 6; ++i)
        if (!(blend[i] >= 0.f) || std::isinf(blend[i])) return fail(ctx, NST_E_ARG, "blend weights must be finite and >= 0");
    const Taps& tp = ctx->taps;
    // b^[k][q] = B[k][i] / sum_k B[k][i] (fp64, then fp32) for the map i of style slot q
    float bhat[NST_MAX_STYLES][kMaxStyle] = {};
    for (int q = 0; q < tp.nstyle; ++q) {
        const int i = tap_index_of(tp.style[q]);
        double sum = 0.0;
        for (int k = 0; k < K; ++k) sum += (double)blend[k * 6 + i];
        if (!(sum > 0.0)) return fail(ctx, NST_E_ARG, "every map of the style set needs a positive blend weight of some style image");
        for (int k = 0; k < K; ++k) bhat[k][q] = (float)((double)blend[k * 6 + i] / sum);
    }
    if (K > 1 && ctx->lv[level].guide.R > 0)
        return fail(ctx, NST_E_STATE, "a guided level takes one style image (nst_level_set_targets_guided): no blend of several");
    hipStream_t s = enter(ctx, stream);
    LevelWs& L = ctx->lv[level];
    NSTCHK(set_content_target(ctx, level, content, s));
    NSTCHK(lap_forward(ctx, L, content, true, s));      // D s_k(content): the Laplacian targets are made with the others
    NSTCHK(mat_set_guide(ctx, L, content, s));          // and the matting term's guide
    // style: Gt_q = sum_k b^[k][q] G_q(style_k), each image at its own size, in ascending k; the first contributing image
    // writes b^ G, the later ones add to it; an image with b^ = 0 on a map is skipped there, one with b^ = 0 on every map
    // of the set gets no forward pass, and no forward pass goes deeper than the deepest map its image contributes to
    bool written[kMaxStyle] = {};
    for (int k = 0; k < K; ++k) {
        int deepest = -1;
        for (int q = 0; q < tp.nstyle; ++q) if (bhat[k][q] > 0.f) deepest = q;
        if (deepest < 0) continue;
        Scratch sc(ctx, s);
        float* part = nullptr;
        NSTCHK(alloc_acts(ctx, sc.acts, hs[k], ws[k]));
        NSTCHK(sc.alloc(&part, gram_part_floats_for(tp, hs[k], ws[k])));
        // a shifted / centred statistic (nst_job_set_gram_shift): this image's own offsets, through the closure's kernels
        GramShiftLevel gsl;
        if (ctx->gs_on()) {
            NSTCHK(sc.alloc(&gsl.words, (size_t)GS_STRIDE));
            if (ctx->gs_center) NSTCHK(sc.alloc(&gsl.sums, (size_t)GS_PART_DOUBLES));
        }
        NSTCHK(forward(ctx, sc.acts, styles[k], hs[k], ws[k], s, tp.style[deepest], ctx->channels));
        for (int q = 0; q <= deepest; ++q) {
            if (!(bhat[k][q] > 0.f)) continue;
            const int l = tp.style[q];
            const StyleTerm st = style_term(tp, q, sc.acts, 0.f, 1.f);
            if (ctx->mom_on() && ctx->mom_slot(q)) {
                // the moment targets: this image's mu and sigma, b^-weighted into the slot's mu^t and sigma^t as G is into Gt
                // (the level's own scratch: no closure runs while its targets are made)
                MomentBatch mb{};
                mb.n = 1;
                mb.it[0] = moment_item(ctx, L, q, sc.acts.act[l], st.N, st.C);
                mb.it[0].mean_out = L.mom.mean_t(q); mb.it[0].std_out = L.mom.std_t(q);
                mb.it[0].alpha = bhat[k][q]; mb.it[0].accumulate = written[q] ? 1 : 0;
                Timer t(ctx, s, K_OTHER, 0);
                HIPCHK(ctx, launch_moment_stats(mb, s));
            }
            // G, b^-weighted into the slot's Gt
            const GramOperand op{sc.acts.act[l], st.N, st.C, ctx->conv_mode == 2 ? amax_act(sc.acts, l) : nullptr, nullptr, part, (float)st.divisor};
            GramFinish fin;
            fin.gram_out = L.gram_t[q]; fin.alpha = bhat[k][q]; fin.accumulate = written[q] ? 1 : 0;
            if (ctx->gs_on()) {
                const ShiftedGram sg{ctx->gs_shift_of(q), ctx->gs_center_of(q), gsl.offset(0), gsl.amax(0), gsl.part(0), nullptr};
                NSTCHK(gram_shifted_of(ctx, op, sg, fin, s));
            } else {
                NSTCHK(gram_of(ctx, op, fin, s));
            }
            written[q] = true;
        }
        NSTCHK(sc.finish());
    }
    L.targets = true;
    forget_forward_pass(ctx);           // (the content target's pass is no closure's)
    return NST_OK;
}

int nst_level_set_targets(nst_ctx* ctx, int level, const float* content, const float* style, int hs, int ws,
                          void* stream) {
    const float ones[6] = {1.f, 1.f, 1.f, 1.f, 1.f, 1.f};
    return nst_level_set_targets_blend(ctx, level, content, 1, &style, &hs, &ws, ones, stream);
}

// ---- spatial control (include/nst_hip.h has the definitions) -----------------------------------------------------------
int nst_level_set_guidance(nst_ctx* ctx, int level, int R, const float* planes, const float* lambda, void* stream) {
    if (ctx) { ++ctx->closure_epoch; ++ctx->ws_seq; }
    NSTCHK(bind(ctx));
    drop_closure_state(ctx, false);
    if (level < 0 || level >= ctx->levels) return fail(ctx, NST_E_STATE, "level not configured");
    if (R < 0 || R > NST_MAX_REGIONS) return fail(ctx, NST_E_ARG, "the number of regions must be 0 .. NST_MAX_REGIONS");
    LevelWs& L = ctx->lv[level];
    if (R == 0) {                       // (in every arithmetic mode: there is nothing to clear in the others)
        quiesce(ctx);
        L.guide = Guidance();
        return NST_OK;
    }
    if (ctx->conv_mode != 2) return fail(ctx, NST_E_STATE, "spatial control runs in the f16x2 arithmetic only (NST_CONV unset)");
    if (ctx->gs_on()) return fail(ctx, NST_E_STATE, "guided Gram matrices take the plain statistic only (nst_job_set_gram_shift with zeros switches the shift off)");
    if (ctx->mom_on()) return fail(ctx, NST_E_STATE, "guided levels take no moment loss (nst_job_set_moments with zeros switches it off)");
    if (L.pm.on()) return fail(ctx, NST_E_STATE, "a level with the MRF term takes no guidance (nst_level_set_patches(ctx, level, NULL, ...) clears the term)");
    if (L.hist.on()) return fail(ctx, NST_E_STATE, "a level with the histogram loss takes no guidance (nst_level_set_histograms(ctx, level, NULL, ...) clears the term)");
    if (L.remd.on()) return fail(ctx, NST_E_STATE, "a level with the relaxed EMD term takes no guidance (nst_level_set_remd(ctx, level, NULL, ...) clears the term)");
    if (L.selfsim.on()) return fail(ctx, NST_E_STATE, "a level with the self-similarity term takes no guidance (nst_level_set_selfsim(ctx, level, NULL, ...) clears the term)");
    if (L.xcorr.on()) return fail(ctx, NST_E_STATE, "a level with the xcorr term takes no guidance (nst_level_set_xcorr(ctx, level, NULL, ...) clears the term)");
    if (!planes) return fail(ctx, NST_E_ARG, "null argument");
    float lam[NST_MAX_REGIONS] = {1.f, 1.f, 1.f, 1.f};
    bool positive = lambda == nullptr;
    for (int r = 0; r < R && lambda; ++r) {
        if (!(lambda[r] >= 0.f) || std::isinf(lambda[r])) return fail(ctx, NST_E_ARG, "region weights must be finite and >= 0");
        lam[r] = lambda[r];
        positive = positive || lambda[r] > 0.f;
    }
    if (!positive) return fail(ctx, NST_E_ARG, "at least one region weight must be positive");
    hipStream_t s = enter(ctx, stream);
    const Taps& tp = ctx->taps;
    // the new pyramid and its masses beside what the level has: a refusal leaves the level as it was (g gives back what it
    // took on every path out)
    Guidance g;
    size_t off[6];
    guidance_offsets(R, L.h, L.w, off);
    g.R = R; g.plane_floats = off[5];
    for (int sc = 0; sc < 5; ++sc) g.plane_off[sc] = off[sc];
    for (int r = 0; r < NST_MAX_REGIONS; ++r) g.lambda[r] = lam[r];
    NSTCHK(g.mem.alloc(ctx, &g.planes, g.plane_floats));
    double bad = 0.0;
    {
        Scratch sc(ctx, s);
        double* dscratch = nullptr;
        NSTCHK(sc.alloc(&dscratch, ((size_t)R * GUIDE_MASS_BLOCKS + 5 * R) * 2));
        if (hipMemcpyAsync(g.planes, planes, (size_t)R * L.h * L.w * 4, hipMemcpyDeviceToDevice, s) != hipSuccess)
            return fail(ctx, NST_E_HIP, "hipMemcpyAsync of the guidance planes failed");
        NSTCHK(build_guidance(ctx, g.planes, off, R, L.h, L.w, dscratch, g.mass, &bad, s));
        NSTCHK(sc.finish());
    }
    if (bad > 0.0) return fail(ctx, NST_E_ARG, "guidance values must be finite and in [0,1]");
    if (!guidance_mass_ok(tp, g.mass, R))
        return fail(ctx, NST_E_ARG, "a region has a mass sum t^2 below 1 on a map in use: less than one pixel's worth of guidance");
    Guidance& old = L.guide;
    if (old.R == R) {
        // same R: the workspace and the guided targets (which depend on the style side only) stay, the planes change
        quiesce(ctx);
        old.mem.exchange(old.planes, g.mem, g.planes);
        std::swap(old.planes, g.planes);
        for (int sc = 0; sc < 5; ++sc)
            for (int r = 0; r < NST_MAX_REGIONS; ++r) old.mass[sc][r] = g.mass[sc][r];
        for (int r = 0; r < NST_MAX_REGIONS; ++r) old.lambda[r] = g.lambda[r];
        g = Guidance();
        mark(ctx, s);
        return NST_OK;
    }
    g.part_floats_r = gram_part_floats_for(tp, L.h, L.w);
    NSTCHK(g.mem.alloc(ctx, &g.part, (size_t)R * g.part_floats_r));
    for (int q = 0; q < tp.nstyle; ++q) {
        const size_t C = (size_t)kCout[tp.style[q]];
        NSTCHK(g.mem.alloc(ctx, &g.gram_t[q], (size_t)R * C * C));
        NSTCHK(g.mem.alloc(ctx, &g.S[q], (size_t)R * C * C));
        NSTCHK(g.mem.alloc(ctx, &g.partial[q], (size_t)R * gram_finish_blocks((int)C)));
    }
    quiesce(ctx);
    L.guide = std::move(g);
    mark(ctx, s);
    return NST_OK;
}

int nst_level_set_targets_guided(nst_ctx* ctx, int level, const float* content, const float* style, int hs, int ws,
                                 const float* style_planes, void* stream) {
    if (ctx) { ++ctx->closure_epoch; ++ctx->ws_seq; }
    NSTCHK(bind(ctx));
    drop_closure_state(ctx, false);
    if (level < 0 || level >= ctx->levels) return fail(ctx, NST_E_STATE, "level not configured");
    LevelWs& L = ctx->lv[level];
    Guidance& g = L.guide;
    if (ctx->gs_on()) return fail(ctx, NST_E_STATE, "guided Gram matrices take the plain statistic only (nst_job_set_gram_shift with zeros switches the shift off)");
    if (ctx->mom_on()) return fail(ctx, NST_E_STATE, "guided levels take no moment loss (nst_job_set_moments with zeros switches it off)");
    if (g.R < 1) return fail(ctx, NST_E_STATE, "the level has no guidance (nst_level_set_guidance first)");
    if (!content || !style || !style_planes) return fail(ctx, NST_E_ARG, "null argument");
    if (hs < 16 || ws < 16) return fail(ctx, NST_E_ARG, "style image must be at least 16x16");
    const Taps& tp = ctx->taps;
    const int R = g.R;
    hipStream_t s = enter(ctx, stream);
    Scratch sc(ctx, s);
    // the style side's pyramid and masses first: a refusal leaves the level's targets as they were
    size_t off[6];
    guidance_offsets(R, hs, ws, off);
    float* sp = nullptr;
    double* dscratch = nullptr;
    double smass[5][NST_MAX_REGIONS] = {};
    double bad = 0.0;
    NSTCHK(sc.alloc(&sp, off[5]));
    NSTCHK(sc.alloc(&dscratch, ((size_t)R * GUIDE_MASS_BLOCKS + 5 * R) * 2));
    HIPCHK(ctx, hipMemcpyAsync(sp, style_planes, (size_t)R * hs * ws * 4, hipMemcpyDeviceToDevice, s));
    NSTCHK(build_guidance(ctx, sp, off, R, hs, ws, dscratch, smass, &bad, s));
    if (bad > 0.0) return fail(ctx, NST_E_ARG, "guidance values must be finite and in [0,1]");
    if (!guidance_mass_ok(tp, smass, R))
        return fail(ctx, NST_E_ARG, "a style region has a mass sum t^2 below 1 on a map in use: less than one pixel's worth of guidance");
    g.targets = false;
    NSTCHK(set_content_target(ctx, level, content, s));
    NSTCHK(lap_forward(ctx, L, content, true, s));
    NSTCHK(mat_set_guide(ctx, L, content, s));
    float* part = nullptr;
    NSTCHK(alloc_acts(ctx, sc.acts, hs, ws));
    NSTCHK(sc.alloc(&part, gram_part_floats_for(tp, hs, ws)));
    NSTCHK(forward(ctx, sc.acts, style, hs, ws, s, tp.style[tp.nstyle - 1], ctx->channels));
    for (int q = 0; q < tp.nstyle; ++q) {
        const int l = tp.style[q], C = kCout[l], scl = kScale[l];
        const size_t N = (size_t)sc.acts.h[l] * sc.acts.w[l];
        for (int r = 0; r < R; ++r) {
            GramFinish fin;
            fin.gram_out = g.gram_t[q] + (size_t)r * C * C; fin.alpha = 1.f;
            NSTCHK(gram_of(ctx, GramOperand{sc.acts.act[l], N, C, amax_act(sc.acts, l), sp + off[scl] + (size_t)r * N, part,
                                            (float)((double)C * smass[scl][r])}, fin, s));
        }
    }
    NSTCHK(sc.finish());
    g.targets = true; g.targets_R = R;
    forget_forward_pass(ctx);
    mark(ctx, s);
    return NST_OK;
}

int nst_level_guidance(const nst_ctx* ctx, int level, int* R, float* lambda, double* mass) {
    if (!ctx) return fail(nullptr, NST_E_ARG, "null context");
    if (level < 0 || level >= ctx->levels) return NST_E_STATE;
    const Guidance& g = ctx->lv[level].guide;
    if (R) *R = g.R;
    for (int r = 0; r < NST_MAX_REGIONS && lambda; ++r) lambda[r] = g.lambda[r];
    for (int sc = 0; sc < 5 && mass; ++sc)
        for (int r = 0; r < NST_MAX_REGIONS; ++r) mass[sc * NST_MAX_REGIONS + r] = r < g.R ? g.mass[sc][r] : 0.0;
    return NST_OK;
}

int nst_level_guidance_planes(nst_ctx* ctx, int level, int scale, float* out, void* stream) {
    NSTCHK(bind(ctx));
    if (level < 0 || level >= ctx->levels) return fail(ctx, NST_E_STATE, "level not configured");
    const LevelWs& L = ctx->lv[level];
    if (L.guide.R < 1) return fail(ctx, NST_E_STATE, "the level has no guidance");
    if (scale < 0 || scale > 4 || !out) return fail(ctx, NST_E_ARG, "scale must be 0 .. 4 and out not null");
    hipStream_t s = enter(ctx, stream);
    HIPCHK(ctx, hipMemcpyAsync(out, L.guide.planes + L.guide.plane_off[scale],
                               (size_t)L.guide.R * (L.h >> scale) * (L.w >> scale) * 4, hipMemcpyDeviceToDevice, s));
    mark(ctx, s);
    return NST_OK;
}

int nst_closure(nst_ctx* ctx, const float* x, float cw, float sw, float tvw, float* grad, float* losses, void* stream) {
    return nst_closure_levels(ctx, x, cw, sw, tvw, 0xFFFFFFFFu, grad, losses, stream);
}

int nst_closure_levels(nst_ctx* ctx, const float* x, float cw, float sw, float tvw, unsigned level_mask, float* grad,
                       float* losses, void* stream) {
    NSTCHK(bind(ctx));
    ++ctx->ws_seq;
    if (ctx->levels < 1) return fail(ctx, NST_E_STATE, "nst_job_configure has not been called");
    if (!x || !grad || !losses) return fail(ctx, NST_E_ARG, "null buffer");
    NSTCHK(closure_targets_check(ctx, level_mask));
    hipStream_t main = enter(ctx, stream);
    ctx->sched = {};
    if (ctx->timing >= 2) NSTCHK(fold_timed(ctx));
    ctx->timed.clear();
    ctx->ev_used = 0;
    ctx->timed_valid = false;
    ctx->timed_backward = false;
    // mode 4: event pairs around the conv launches of every fourth closure only - a pair around each of the 24 conv
    // launches of EVERY closure (mode 3) costs 5 % of the closure rate at 9.5 ms per closure
    ctx->sample_now = (ctx->timing != 4) || ((ctx->closure_seq++ & 3) == 0);
    if (ctx->timing) HIPCHK(ctx, hipEventRecord(ctx->t0, main));

    // Optional (NST_GRAPH=1): replay the ~110 dependent launches as a hipGraph.  Captured the second consecutive time the
    // same buffers / weights / mask are passed (optimiser drivers always pass the same ones), never while per-launch
    // timing is on.  The closure holds kernel nodes only: hipMemsetAsync nodes were NOT ordered against the kernels
    // around them on replay (absmax records zeroed late -> garbage scales, run-to-run different losses), which is why
    // every zero fill in the closure is launch_zero.  Measured gain: none (the host runs ~16 ms ahead of the GPU).
    const nst_ctx::GraphKey key{x, grad, losses, cw, sw, tvw, level_mask};
    const bool same_as_last = std::memcmp(&key, &ctx->glast, sizeof(key)) == 0;
    ctx->glast = key;
    bool done = false;
    if (ctx->use_graph && ctx->timing < 2 && batch_eligible(ctx) && same_as_last) {
        if (!ctx->gexec || std::memcmp(&key, &ctx->gkey, sizeof(key)) != 0) {
            if (ctx->gexec) { (void)hipGraphExecDestroy(ctx->gexec); ctx->gexec = nullptr; }
            hipGraph_t graph = nullptr;
            HIPCHK(ctx, hipStreamBeginCapture(ctx->gstream, hipStreamCaptureModeThreadLocal));
            const int rc = closure_record(ctx, x, cw, sw, tvw, level_mask, grad, losses, ctx->gstream);
            const hipError_t ce = hipStreamEndCapture(ctx->gstream, &graph);
            if (rc != NST_OK) { if (graph) (void)hipGraphDestroy(graph); return rc; }
            HIPCHK(ctx, ce);
            const hipError_t ie = hipGraphInstantiate(&ctx->gexec, graph, nullptr, nullptr, 0);
            (void)hipGraphDestroy(graph);
            HIPCHK(ctx, ie);
            ctx->gkey = key;
        }
        HIPCHK(ctx, hipGraphLaunch(ctx->gexec, main));
        ctx->sched = {};                 // (what closure_record counted while capturing describes the capture, not this launch)
        ctx->sched.graph_replay = 1;
        done = true;
    }
    if (!done) NSTCHK(closure_record(ctx, x, cw, sw, tvw, level_mask, grad, losses, main));
    if (ctx->timing) { HIPCHK(ctx, hipEventRecord(ctx->t1, main)); ctx->timed_valid = true; }
    mark(ctx, main);
    return NST_OK;
}

// ---- the closure in two halves (include/nst_hip.h) -----------------------------------------------------------------
// A caller that needs the loss before it knows whether it needs the gradient - a line search whose trial point is taken
// or dropped on its loss alone - evaluates the forward half, reads the loss, and runs the backward half only for a point
// it takes.  Both halves are the launches of nst_closure_levels on the batched schedule, in its order.
int nst_closure_forward(nst_ctx* ctx, const float* x, float cw, float sw, float tvw, unsigned level_mask, float* losses,
                        void* stream) {
    NSTCHK(bind(ctx));
    ++ctx->ws_seq;
    ctx->fwd_token.valid = false;
    if (ctx->levels < 1) return fail(ctx, NST_E_STATE, "nst_job_configure has not been called");
    if (!x || !losses) return fail(ctx, NST_E_ARG, "null buffer");
    NSTCHK(closure_targets_check(ctx, level_mask));
    if (!batch_eligible(ctx) || ctx->use_graph)
        return fail(ctx, NST_E_UNAVAILABLE, "the closure halves run on the batched schedule without a hipGraph only: use nst_closure");
    hipStream_t main = enter(ctx, stream);
    ctx->sched = {};
    if (ctx->timing >= 2) NSTCHK(fold_timed(ctx));
    ctx->timed.clear();
    ctx->ev_used = 0;
    ctx->timed_valid = false;
    ctx->timed_backward = false;
    ctx->sample_now = (ctx->timing != 4) || ((ctx->closure_seq++ & 3) == 0);
    if (ctx->timing) HIPCHK(ctx, hipEventRecord(ctx->t0, main));
    const int rc = closure_record(ctx, x, cw, sw, tvw, level_mask, nullptr, losses, main, FORWARD);
    if (rc == NST_OK && ctx->timing && hipEventRecord(ctx->t1, main) == hipSuccess) ctx->timed_valid = true;
    mark(ctx, main);             // on every path out that may have launched work
    NSTCHK(rc);
    ctx->fwd_token = {true, x, cw, sw, tvw, level_mask, ctx->closure_epoch, ctx->ws_seq};
    return NST_OK;
}

int nst_closure_backward(nst_ctx* ctx, const float* x, float cw, float sw, float tvw, unsigned level_mask, float* grad,
                         void* stream) {
    NSTCHK(bind(ctx));
    if (!x || !grad) return fail(ctx, NST_E_ARG, "null buffer");
    const nst_ctx::ForwardToken tk = ctx->fwd_token;
    const float w[3] = {cw, sw, tvw}, tw[3] = {tk.cw, tk.sw, tk.tvw};
    if (!tk.valid || tk.seq != ctx->ws_seq || tk.epoch != ctx->closure_epoch || tk.x != x || tk.mask != level_mask ||
        std::memcmp(w, tw, sizeof(w)) != 0)
        return fail(ctx, NST_E_STATE, "nst_closure_backward: no forward half of these arguments is the last use of the context's workspaces");
    ++ctx->ws_seq;               // (one backward per forward: the gradient buffers of the levels are consumed)
    ctx->fwd_token.valid = false;
    hipStream_t main = enter(ctx, stream);
    ctx->sched = {};
    // timing: the forward half's record is folded as a closure, this half's launches and time then join the totals
    if (ctx->timing >= 2) NSTCHK(fold_timed(ctx));
    ctx->timed.clear();
    ctx->ev_used = 0;
    ctx->timed_valid = false;
    ctx->timed_backward = true;
    if (ctx->timing) HIPCHK(ctx, hipEventRecord(ctx->t0, main));
    const int rc = closure_record(ctx, x, cw, sw, tvw, level_mask, grad, nullptr, main, BACKWARD);
    if (rc == NST_OK && ctx->timing && hipEventRecord(ctx->t1, main) == hipSuccess) ctx->timed_valid = true;
    mark(ctx, main);
    return rc;
}

// ---- stripe (window) closure: spatial sharding of one pyramid level -------------------------------------
int nst_window_sums_count(size_t* count) {
    if (!count) return fail(nullptr, NST_E_ARG, "null argument");
    *count = kWinSums;
    return NST_OK;
}

int nst_window_begin(nst_ctx* ctx, const float* xs, int row0, int rows, int H0, float* sums, void* stream) {
    NSTCHK(bind(ctx));
    ++ctx->ws_seq;
    NSTCHK(window_check(ctx, xs, row0, rows, H0));
    if (!sums) return fail(ctx, NST_E_ARG, "null buffer");
    hipStream_t s = enter(ctx, stream);
    LevelWs& L = ctx->lv[0];
    ActSet& a = L.acts;
    Window win{row0, rows, H0, sums};
    const int lv[1] = {0};
    const float* xi[1] = {xs};
    NSTCHK(batched_forward(ctx, xi, lv, 1, s, &win));
    // un-normalised Gram sums of the owned rows
    for (int q = 0; q < ctx->taps.nstyle; ++q) {
        const int l = ctx->taps.style[q], C = kCout[l];
        const size_t off = (size_t)win_r0(win, kScale[l]) * a.w[l] * C;
        const size_t N = (size_t)win_nr(win, kScale[l]) * a.w[l];
        GramFinish fin;
        fin.gram_out = sums + kWinGramOff[q];
        NSTCHK(gram_of(ctx, GramOperand{a.act[l] + off, N, C, amax_act(a, l), nullptr, L.gram_part, 1.f}, fin, s, false));
    }
    // content: sum of squared differences over the owned rows
    {
        const int m = ctx->taps.content;
        const size_t off = (size_t)win_r0(win, kScale[m]) * a.w[m] * kCout[m];
        const size_t cnt = (size_t)win_nr(win, kScale[m]) * a.w[m] * kCout[m];
        HIPCHK(ctx, launch_mse_grad(a.act[m] + off, L.content_t + off, cnt, 0.f, nullptr, L.content_partial, s));
        HIPCHK(ctx, launch_sum_doubles(L.content_partial, MSE_BLOCKS, 1, 0, sums + kWinScalarOff, s));
    }
    // total variation: sums of |dx|, |dy| over the owned rows (batched_forward ran the windowed partial pass)
    HIPCHK(ctx, launch_sum_doubles(L.tv_partial, TV_BLOCKS, 2, 0, sums + kWinScalarOff + 1, s));
    HIPCHK(ctx, launch_sum_doubles(L.tv_partial, TV_BLOCKS, 2, 1, sums + kWinScalarOff + 2, s));
    mark(ctx, s);
    return NST_OK;
}

int nst_window_end(nst_ctx* ctx, const float* xs, int row0, int rows, int H0, float cw, float sw, float tvw, float* sums,
                   float* gxs, float* losses, void* stream) {
    NSTCHK(bind(ctx));
    ++ctx->ws_seq;
    NSTCHK(window_check(ctx, xs, row0, rows, H0));
    if (!sums || !gxs || !losses) return fail(ctx, NST_E_ARG, "null buffer");
    hipStream_t s = enter(ctx, stream);
    LevelWs& L = ctx->lv[0];
    ActSet& a = L.acts;
    Window win{row0, rows, H0, sums};
    // S = d loss / d G from the Gram sums of ALL stripes, normalised by the full image
    for (int q = 0; q < ctx->taps.nstyle; ++q) {
        const StyleTerm st = style_term(ctx->taps, q, a, sw, ctx->style_weight(q), H0);
        HIPCHK(ctx, launch_gram_finish(sums + kWinGramOff[q], 1, st.C, (float)st.divisor, L.gram_t[q], st.coef, nullptr, L.S[q], L.S_bf[q],
                                       amax_S(a, q), L.style_partial[q], s));
    }
    const double nx = 3.0 * H0 * (L.w - 1), ny = 3.0 * (H0 - 1) * L.w;
    HIPCHK(ctx, launch_window_scalars(sums + kWinScalarOff, nx, ny, L.tv_means, L.content_partial, 0, s));   // means only
    const int lv[1] = {0};
    const float* xi[1] = {xs};
    float* gi[1] = {gxs};
    NSTCHK(batched_backward(ctx, xi, gi, lv, 1, cw, tvw, s, &win, L.tv_means, nx, ny));
    // the level's loss row from the global sums (the backward's content pass left this stripe's partials behind)
    HIPCHK(ctx, launch_window_scalars(sums + kWinScalarOff, nx, ny, L.tv_means, L.content_partial, MSE_BLOCKS, s));
    LossAssembly la = fill_loss_assembly(ctx, 1u, cw, sw, tvw, losses);
    const int m = ctx->taps.content;
    la.lv[0].content_n = (size_t)(H0 >> kScale[m]) * a.w[m] * kCout[m];      // the full image's, not the stripe's
    HIPCHK(ctx, launch_loss_assemble(la, s));
    mark(ctx, s);
    return NST_OK;
}

}  // extern "C"
