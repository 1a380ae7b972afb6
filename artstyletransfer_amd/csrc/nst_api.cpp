// nst_api.cpp - standalone entry points of libnst_hip.so (include/nst_hip.h): the pieces of the pipeline one at a time
// (VGG19 features and their backward, Gram, total variation, bicubic, prepare / unprepare, read-backs of a job's workspace),
// the job set-up image operations, and the colour set-up functions with their 3x3 eigen-solver.  The context and the job
// state are nst_ctx.cpp's, the network walkers and the closure nst_closure.cpp's (nst_ctx.h).
//
// Host-side control only; every FLOP and byte of the path is in the .hip kernels.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "nst_ctx.h"

using namespace nst;

// ---- standalone pieces -----------------------------------------------------------------------------
// one forward pass of an h x w image; outs[i] (nullable) receives conv layer layer_of[i] (nullptr: layer i) as planar CHW
static int vgg_outputs(nst_ctx* ctx, const float* x, int h, int w, float* const* outs, int n, const int* layer_of, void* stream) {
    NSTCHK(bind(ctx));
    if (!x || !outs) return fail(ctx, NST_E_ARG, "null argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    Scratch sc(ctx, s);
    ActSet& a = sc.acts;
    NSTCHK(alloc_acts(ctx, a, h, w));
    NSTCHK(forward(ctx, a, x, h, w, s));
    for (int i = 0; i < n; ++i) {
        if (!outs[i]) continue;
        const int l = layer_of ? layer_of[i] : i;
        if (launch_hwc_to_chw(a.act[l], kCout[l], a.h[l], a.w[l], outs[i], s) != hipSuccess) return fail(ctx, NST_E_HIP, "hwc_to_chw launch failed");
    }
    return sc.finish();
}

extern "C" {

int nst_vgg_features(nst_ctx* ctx, const float* x, int h, int w, float* const* outs, void* stream) {
    return vgg_outputs(ctx, x, h, w, outs, 6, kTapLayer, stream);
}
int nst_vgg_activations(nst_ctx* ctx, const float* x, int h, int w, float* const* outs, void* stream) {
    return vgg_outputs(ctx, x, h, w, outs, NL, nullptr, stream);
}

int nst_vgg_features_backward(nst_ctx* ctx, const float* x, int h, int w, const float* const* gouts, float* gx,
                              void* stream) {
    NSTCHK(bind(ctx));
    if (!x || !gouts || !gx) return fail(ctx, NST_E_ARG, "null argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    Scratch sc(ctx, s);
    ActSet& a = sc.acts;
    float* g0 = nullptr; float* g1 = nullptr;
    NSTCHK(alloc_acts(ctx, a, h, w));
    NSTCHK(sc.alloc(&g0, (size_t)h * w * 64));
    NSTCHK(sc.alloc(&g1, (size_t)h * w * 64));
    NSTCHK(forward(ctx, a, x, h, w, s));
    Inject inj[NL];
    for (int i = 0; i < 6; ++i) {
        if (!gouts[i]) continue;
        const int l = kTapLayer[i];
        float* g = nullptr;
        NSTCHK(sc.alloc(&g, (size_t)a.h[l] * a.w[l] * kCout[l]));
        if (launch_chw_to_hwc(gouts[i], kCout[l], a.h[l], a.w[l], g, s) != hipSuccess) return fail(ctx, NST_E_HIP, "chw_to_hwc launch failed");
        inj[l].direct = g;
    }
    NSTCHK(backward(ctx, a, inj, nullptr, g0, g1, gx, h, w, s, NL - 1, ctx->taps.use_relu != 0));
    return sc.finish();
}

int nst_gram(nst_ctx* ctx, const float* f, int C, int h, int w, int normalize, float* gram, void* stream) {
    NSTCHK(bind(ctx));
    if (!f || !gram || C < 1 || h < 1 || w < 1) return fail(ctx, NST_E_ARG, "bad argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t N = (size_t)h * w;
    Scratch sc(ctx, s);
    float* nhwc = nullptr; float* part = nullptr; unsigned* amax = nullptr;
    NSTCHK(sc.alloc(&nhwc, N * C));
    NSTCHK(sc.alloc(&part, (size_t)gram_nsplit(C, N) * C * C));
    if (ctx->conv_mode == 2) NSTCHK(sc.alloc(&amax, (size_t)NST_AMAX_SLOTS));
    if (launch_chw_to_hwc(f, C, h, w, nhwc, s) != hipSuccess) return fail(ctx, NST_E_HIP, "chw_to_hwc launch failed");
    // the fp16-piece kernel needs the absmax of its operand (in the closure the producing conv records it)
    if (amax && (launch_zero(amax, NST_AMAX_SLOTS, s) != hipSuccess || launch_absmax_slots(nhwc, N * C, amax, s) != hipSuccess))
        return fail(ctx, NST_E_HIP, "absmax launch failed");
    GramFinish fin;
    fin.gram_out = gram;
    NSTCHK(gram_of(ctx, GramOperand{nhwc, N, C, amax, nullptr, part, normalize ? (float)((double)C * h * w) : 1.f}, fin, s));
    return sc.finish();
}

// the shifted / centred statistic alone (nst_job_set_gram_shift has the definition), beside nst_gram
int nst_gram_shifted(nst_ctx* ctx, const float* f, int C, int h, int w, int normalize, int center, float shift, float* gram,
                     float* offset_out, void* stream) {
    NSTCHK(bind(ctx));
    if (!f || !gram || C < 1 || h < 1 || w < 1) return fail(ctx, NST_E_ARG, "bad argument");
    if (!std::isfinite(shift) || (center && shift != 0.f)) return fail(ctx, NST_E_ARG, "shift must be finite, and 0 for a centred Gram");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!center && shift == 0.f) {
        // the plain statistic, by the plain kernels: bitwise nst_gram
        if (offset_out) HIPCHK(ctx, hipMemsetAsync(offset_out, 0, (size_t)C * sizeof(float), s));
        return nst_gram(ctx, f, C, h, w, normalize, gram, stream);
    }
    if (ctx->conv_mode != 2) return fail(ctx, NST_E_STATE, "the shifted Gram runs in the f16x2 arithmetic only (NST_CONV unset)");
    if (!(C == 64 || C % 128 == 0) || C > 1024) return fail(ctx, NST_E_ARG, "the shifted Gram takes C = 64 or a multiple of 128, at most 1024");
    const size_t N = (size_t)h * w;
    Scratch sc(ctx, s);
    float* nhwc = nullptr; float* part = nullptr; unsigned* amax = nullptr; float* words = nullptr; double* sums = nullptr;
    NSTCHK(sc.alloc(&nhwc, N * C));
    NSTCHK(sc.alloc(&part, (size_t)gram_nsplit(C, N) * C * C));
    NSTCHK(sc.alloc(&amax, (size_t)NST_AMAX_SLOTS));
    NSTCHK(sc.alloc(&words, (size_t)C + NST_AMAX_SLOTS));
    if (center) NSTCHK(sc.alloc(&sums, (size_t)GS_PART_DOUBLES));
    if (launch_chw_to_hwc(f, C, h, w, nhwc, s) != hipSuccess) return fail(ctx, NST_E_HIP, "chw_to_hwc launch failed");
    if (launch_zero(amax, NST_AMAX_SLOTS, s) != hipSuccess || launch_absmax_slots(nhwc, N * C, amax, s) != hipSuccess)
        return fail(ctx, NST_E_HIP, "absmax launch failed");
    const ShiftedGram sg{shift, center ? 1 : 0, words, reinterpret_cast<unsigned*>(words + C), sums, nullptr};
    GramFinish fin;
    fin.gram_out = gram;
    NSTCHK(gram_shifted_of(ctx, GramOperand{nhwc, N, C, amax, nullptr, part, normalize ? (float)((double)C * h * w) : 1.f}, sg, fin, s));
    if (offset_out) HIPCHK(ctx, hipMemcpyAsync(offset_out, words, (size_t)C * sizeof(float), hipMemcpyDeviceToDevice, s));
    return sc.finish();
}

// the closure's batched Gram launch on the caller's maps (one launch_gram_batch under the context's gram_pack), beside nst_gram_shifted
int nst_gram_batch(nst_ctx* ctx, nst_gram_batch_item* items, int n, int normalize, void* stream) {
    NSTCHK(bind(ctx));
    if (!items || n < 1 || n > NST_GRAM_BATCH_MAX) return fail(ctx, NST_E_ARG, "a Gram batch takes 1 .. NST_GRAM_BATCH_MAX items");
    if (ctx->conv_mode != 2) return fail(ctx, NST_E_STATE, "the Gram batch runs in the f16x2 arithmetic only (NST_CONV unset)");
    for (int i = 0; i < n; ++i) {
        const nst_gram_batch_item& a = items[i];
        if (!a.f || !a.gram || a.h < 1 || a.w < 1) return fail(ctx, NST_E_ARG, "bad argument");
        if (!(a.C == 64 || (a.C >= 128 && a.C % 128 == 0))) return fail(ctx, NST_E_ARG, "the Gram batch takes C = 64 or a multiple of 128");
        if ((a.guide != nullptr) != (items[0].guide != nullptr)) return fail(ctx, NST_E_ARG, "a Gram batch is guided as a whole or not at all");
        if (!a.target && (a.S || a.S_bf)) return fail(ctx, NST_E_ARG, "S and S_bf need a target");
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    Scratch sc(ctx, s);
    GramBatch gb{};
    gb.n = n;
    for (int i = 0; i < n; ++i) {
        const nst_gram_batch_item& a = items[i];
        const size_t N = (size_t)a.h * a.w;
        float* nhwc = nullptr; float* part = nullptr; unsigned* amax = nullptr; unsigned* s_amax = nullptr; double* partial = nullptr;
        NSTCHK(sc.alloc(&nhwc, N * a.C));
        NSTCHK(sc.alloc(&part, (size_t)gram_nsplit(a.C, N) * a.C * a.C));
        NSTCHK(sc.alloc(&amax, (size_t)NST_AMAX_SLOTS));
        if (a.target) {
            NSTCHK(sc.alloc(&s_amax, (size_t)NST_AMAX_SLOTS));
            NSTCHK(sc.alloc(&partial, (size_t)gram_finish_blocks(a.C)));
        }
        if (launch_chw_to_hwc(a.f, a.C, a.h, a.w, nhwc, s) != hipSuccess) return fail(ctx, NST_E_HIP, "chw_to_hwc launch failed");
        if (launch_zero(amax, NST_AMAX_SLOTS, s) != hipSuccess || launch_absmax_slots(nhwc, N * a.C, amax, s) != hipSuccess)
            return fail(ctx, NST_E_HIP, "absmax launch failed");
        if (s_amax && launch_zero(s_amax, NST_AMAX_SLOTS, s) != hipSuccess) return fail(ctx, NST_E_HIP, "zero launch failed");
        GramItem& it = gb.it[i];
        it.f = nhwc; it.N = N; it.C = a.C; it.amax = amax; it.part = part; it.guide = a.guide;
        it.divisor = normalize ? (float)((double)a.C * a.h * a.w) : 1.f;
        it.target = a.target; it.coef = a.coef; it.gram_out = a.gram; it.S = a.S; it.S_bf = a.S_bf; it.S_amax = s_amax;
        it.mse_partial = partial;
    }
    GramGeometry geo[NST_GRAM_BATCH_MAX] = {};
    HIPCHK(ctx, launch_gram_batch(gb, s, ctx->gram_pack, geo));
    HIPCHK(ctx, hipStreamSynchronize(s));
    std::vector<double> partial;
    for (int i = 0; i < n; ++i) {
        nst_gram_batch_item& a = items[i];
        a.nsplit = geo[i].nsplit;
        a.pix_per_split = (long long)geo[i].pix_per_split;
        a.mse = 0.0;
        a.S_absmax = 0.f;
        if (!a.target) continue;
        partial.resize((size_t)gram_finish_blocks(a.C));
        float words[NST_AMAX_SLOTS];
        HIPCHK(ctx, hipMemcpy(partial.data(), gb.it[i].mse_partial, partial.size() * sizeof(double), hipMemcpyDeviceToHost));
        HIPCHK(ctx, hipMemcpy(words, gb.it[i].S_amax, sizeof(words), hipMemcpyDeviceToHost));
        for (double v : partial) a.mse += v;
        for (float v : words) a.S_absmax = std::max(a.S_absmax, v);
    }
    return sc.finish();
}

// the moment statistic alone (nst_job_set_moments has the definition), beside nst_gram_shifted: the closure's kernels
int nst_moments(nst_ctx* ctx, const float* f, int C, int h, int w, float epsilon, float* mean_out, float* std_out, void* stream) {
    NSTCHK(bind(ctx));
    if (!f || !mean_out || !std_out || C < 1 || h < 1 || w < 1) return fail(ctx, NST_E_ARG, "bad argument");
    if (!(epsilon > 0.f) || std::isinf(epsilon)) return fail(ctx, NST_E_ARG, "the moment epsilon must be finite and > 0");
    if (!(C == 64 || C % 128 == 0) || C > 1024) return fail(ctx, NST_E_ARG, "the moment statistic takes C = 64 or a multiple of 128, at most 1024");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t N = (size_t)h * w;
    Scratch sc(ctx, s);
    float* nhwc = nullptr; double* part = nullptr; double* stat = nullptr;
    NSTCHK(sc.alloc(&nhwc, N * C));
    NSTCHK(sc.alloc(&part, (size_t)MOM_PART_DOUBLES));
    NSTCHK(sc.alloc(&stat, (size_t)2 * C));
    if (launch_chw_to_hwc(f, C, h, w, nhwc, s) != hipSuccess) return fail(ctx, NST_E_HIP, "chw_to_hwc launch failed");
    MomentBatch mb{};
    mb.n = 1;
    mb.it[0] = MomentItem{nhwc, N, C, (double)epsilon, part, stat, mean_out, std_out, 1.f, 0, 0, 0, 0};
    HIPCHK(ctx, launch_moment_stats(mb, s));
    return sc.finish();
}

int nst_guided_gram_backward(nst_ctx* ctx, const float* f, size_t N, int C, int R, const float* planes, const float* S,
                             const float* addend, const unsigned* relu_bits, float* out, unsigned* amax_slots, void* stream) {
    NSTCHK(bind(ctx));
    if (!f || !planes || !S || !out || N < 1 || C < 64 || C % 64 != 0 || R < 1 || R > NST_MAX_REGIONS)
        return fail(ctx, NST_E_ARG, "bad argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    GuidedBwd gb{};
    gb.F = f; gb.N = N; gb.C = C; gb.R = R;
    for (int r = 0; r < R; ++r) { gb.t[r] = planes + (size_t)r * N; gb.S[r] = S + (size_t)r * C * C; }
    gb.addend = addend; gb.out = out; gb.bits = relu_bits; gb.amax_out = amax_slots;
    if (amax_slots) HIPCHK(ctx, launch_zero(amax_slots, NST_AMAX_SLOTS, s));
    HIPCHK(ctx, launch_guided_bwd(gb, s));
    return NST_OK;
}

int nst_level_activation(nst_ctx* ctx, int level, int layer, float* out, void* stream) {
    NSTCHK(bind(ctx));
    ++ctx->ws_seq;
    if (level < 0 || level >= ctx->levels) return fail(ctx, NST_E_STATE, "level not configured");
    if (layer < 0 || layer >= NL || !out) return fail(ctx, NST_E_ARG, "bad argument");
    const ActSet& a = ctx->lv[level].acts;
    hipStream_t s = enter(ctx, stream);
    // a map the last forward pass left out (nothing of a closure reads it): that layer's launch once more, with the map
    const int rc = restore_map(ctx, level, layer, s);
    if (rc == NST_OK && launch_hwc_to_chw(a.act[layer], kCout[layer], a.h[layer], a.w[layer], out, s) != hipSuccess) {
        mark(ctx, s);
        return fail(ctx, NST_E_HIP, "hwc_to_chw launch failed");
    }
    mark(ctx, s);
    return rc;
}

int nst_level_image(nst_ctx* ctx, int level, float* out, void* stream) {
    NSTCHK(bind(ctx));
    if (level < 1 || level >= ctx->levels) return fail(ctx, NST_E_ARG, "level must be 1 .. levels_num - 1 (level 0 is the caller's x)");
    if (!out) return fail(ctx, NST_E_ARG, "null argument");
    const LevelWs& L = ctx->lv[level];
    hipStream_t s = enter(ctx, stream);
    HIPCHK(ctx, hipMemcpyAsync(out, L.img.xl, (size_t)ctx->channels * L.h * L.w * sizeof(float), hipMemcpyDeviceToDevice, s));
    mark(ctx, s);
    return NST_OK;
}

int nst_total_variation(nst_ctx* ctx, const float* y, int C, int h, int w, float* value, float* grad, void* stream) {
    NSTCHK(bind(ctx));
    if (!y || !value) return fail(ctx, NST_E_ARG, "null argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    Scratch sc(ctx, s);
    double* partial = nullptr; float* means = nullptr;
    NSTCHK(sc.alloc(&partial, 2 * TV_BLOCKS));
    NSTCHK(sc.alloc(&means, 2));
    hipError_t e = launch_tv_partial(y, C, h, w, partial, s);
    if (e == hipSuccess) e = launch_tv_finish(y, C, h, w, partial, 1.f, grad, 0, means, s);
    float m[2] = {0, 0};
    if (e == hipSuccess) e = hipMemcpyAsync(m, means, 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    const float tv = m[0] * m[0] + m[1] * m[1];
    if (e == hipSuccess) e = hipMemcpy(value, &tv, 4, hipMemcpyHostToDevice);
    HIPCHK(ctx, e);
    return sc.finish();
}

// The Laplacian term of one entry on its own (include/nst_hip.h): value = lap_k of y against content, grad (nullable,
// overwritten) = d lap_k / dy with gamma = 1.  The launches of the closure, on scratch buffers.  Synchronous.
int nst_laplacian_loss(nst_ctx* ctx, const float* y, const float* content, int C, int h, int w, int p, float* value, float* grad,
                       void* stream) {
    NSTCHK(bind(ctx));
    if (!y || !content || !value) return fail(ctx, NST_E_ARG, "null argument");
    if (C != 1 && C != 3) return fail(ctx, NST_E_ARG, "C must be 3, or 1 for a luminance plane");
    if (p < 1 || p > 32) return fail(ctx, NST_E_ARG, "a Laplacian pool size must be 1 .. 32");
    if (h < 1 || w < 1 || h / p < 3 || w / p < 3) return fail(ctx, NST_E_ARG, "the pooled image must be at least 3x3");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int hk = h / p, wk = w / p;
    const size_t n = (size_t)(hk - 2) * (wk - 2);
    Scratch sc(ctx, s);
    double* pooled = nullptr; double* target = nullptr; float* r = nullptr; double* partial = nullptr;
    NSTCHK(sc.alloc(&pooled, (size_t)hk * wk));
    NSTCHK(sc.alloc(&target, n));
    NSTCHK(sc.alloc(&r, n));
    NSTCHK(sc.alloc(&partial, LAP_BLOCKS));
    HIPCHK(ctx, launch_lap_pool(content, C, h, w, p, pooled, s));
    HIPCHK(ctx, launch_lap_stencil(pooled, hk, wk, nullptr, target, nullptr, nullptr, s));
    HIPCHK(ctx, launch_lap_pool(y, C, h, w, p, pooled, s));
    HIPCHK(ctx, launch_lap_stencil(pooled, hk, wk, target, nullptr, r, partial, s));
    HIPCHK(ctx, launch_lap_value(partial, (double)n, value, s));
    if (grad) {
        LapBackward lb{};
        lb.K = 1; lb.p[0] = p; lb.r[0] = r;
        lb.coef[0] = (float)(2.0 * (C == 1 ? 3.0 : 1.0) / ((double)n * (double)p * (double)p));
        HIPCHK(ctx, launch_lap_backward(lb, C, h, w, grad, 0, s));
    }
    return sc.finish();
}

// The matting term on its own (include/nst_hip.h): value = mat of y under the guide I, grad (nullable, overwritten) =
// d mat / dy with gamma = 1.  The launches of the closure, on scratch buffers.  Synchronous.
int nst_matting_loss(nst_ctx* ctx, const float* y, const float* guide, int C, int h, int w, double epsilon, float* value, float* grad,
                     void* stream) {
    NSTCHK(bind(ctx));
    if (!y || !guide || !value) return fail(ctx, NST_E_ARG, "null argument");
    if (C != 1 && C != 3) return fail(ctx, NST_E_ARG, "C must be 3, or 1 for a luminance plane");
    if (h < 3 || w < 3) return fail(ctx, NST_E_ARG, "the image must be at least 3x3");
    if (!(epsilon > 0.0) || std::isinf(epsilon)) return fail(ctx, NST_E_ARG, "the matting epsilon must be finite and > 0");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int tiles = mat_tiles(h, w);
    const double n = (C == 1 ? 1.0 : 3.0) * (double)(h - 2) * (double)(w - 2);
    Scratch sc(ctx, s);
    double* partial = nullptr;
    NSTCHK(sc.alloc(&partial, (size_t)tiles));
    HIPCHK(ctx, launch_mat_forward(y, guide, C, h, w, 1.0, epsilon, partial, s));
    HIPCHK(ctx, launch_mat_value(partial, tiles, n, value, s));
    if (grad) HIPCHK(ctx, launch_mat_backward(y, guide, C, h, w, 1.0, epsilon, (float)(2.0 / (255.0 * n)), grad, 0, s));
    return sc.finish();
}

// The temporal term on its own (include/nst_hip.h): value = tmp of y against the anchor under the weight plane (nullable:
// ones), grad (nullable, overwritten) = d tmp / dy with gamma = 1.  The launches of the closure, on scratch buffers.  Synchronous.
int nst_anchor_loss(nst_ctx* ctx, const float* y, const float* anchor, const float* weights, int C, int h, int w, float* value,
                    float* grad, void* stream) {
    NSTCHK(bind(ctx));
    if (!y || !anchor || !value) return fail(ctx, NST_E_ARG, "null argument");
    if (C != 1 && C != 3) return fail(ctx, NST_E_ARG, "C must be 3, or 1 for a luminance plane");
    if (h < 1 || w < 1) return fail(ctx, NST_E_ARG, "the image must be at least 1x1");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const double n = (double)C * (double)h * (double)w;
    Scratch sc(ctx, s);
    double* partial = nullptr;
    NSTCHK(sc.alloc(&partial, (size_t)ANCHOR_BLOCKS));
    HIPCHK(ctx, launch_anchor_forward(y, anchor, weights, C, h, w, partial, s));
    HIPCHK(ctx, launch_anchor_value(partial, ANCHOR_BLOCKS, n, value, s));
    if (grad) HIPCHK(ctx, launch_anchor_backward(y, anchor, weights, C, h, w, (float)(2.0 / n), grad, 0, s));
    return sc.finish();
}

int nst_anchor_geometry(int* blocks, int* block_elems) {
    if (blocks) *blocks = ANCHOR_BLOCKS;
    if (block_elems) *block_elems = anchor_block_elems();
    return NST_OK;
}

// The MRF term's pieces on their own (include/nst_hip.h has the definition): the kernels of patch_match.hip on scratch
// buffers.  Synchronous.
static int patch_args(nst_ctx* ctx, const float* f, int h, int w, int C, const float* fs, int hs, int ws, int stride, PatchDict* d) {
    if (!f || !fs) return fail(ctx, NST_E_ARG, "null argument");
    if (C != 64 && C != 128 && C != 256 && C != 512) return fail(ctx, NST_E_ARG, "the patch match takes maps of 64, 128, 256 or 512 channels");
    if (h < 3 || w < 3 || hs < 3 || ws < 3) return fail(ctx, NST_E_ARG, "the map and the style map must be at least 3x3");
    if (stride < 1 || stride > 8) return fail(ctx, NST_E_ARG, "the style stride must be 1..8");
    if ((double)h * w * C >= 2147483648.0 || (double)hs * ws * C >= 2147483648.0) return fail(ctx, NST_E_ARG, "the map is too large");
    *d = PatchDict{};
    d->fs = fs;
    if (!pm_dict_geometry(hs, ws, C, stride, d)) return fail(ctx, NST_E_ARG, "bad dictionary geometry");
    return NST_OK;
}

int nst_patch_match(nst_ctx* ctx, const float* f, int h, int w, int C, const float* fs, int hs, int ws, int stride, double epsilon,
                    int* idx_out, float* score_out, void* stream) {
    NSTCHK(bind(ctx));
    PatchDict d;
    NSTCHK(patch_args(ctx, f, h, w, C, fs, hs, ws, stride, &d));
    if (!idx_out && !score_out) return fail(ctx, NST_E_ARG, "null argument");
    if (!(epsilon > 0.0) || std::isinf(epsilon)) return fail(ctx, NST_E_ARG, "the patch epsilon must be finite and > 0");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t n = (size_t)(h - 2) * (w - 2);
    Scratch sc(ctx, s);
    unsigned* amax = nullptr; float* rq = nullptr; unsigned char* packed = nullptr; unsigned long long* keys = nullptr;
    NSTCHK(sc.alloc(&amax, (size_t)2 * NST_AMAX_SLOTS));
    NSTCHK(sc.alloc(&rq, (size_t)pm_dict_tiles(d.m) * 32));
    NSTCHK(sc.alloc(&packed, pm_packed_bytes(d.m, C)));
    NSTCHK(sc.alloc(&keys, n));
    HIPCHK(ctx, launch_pm_prepare(d, epsilon, amax, rq, packed, s));
    d.amax = amax; d.rq = rq; d.packed = packed;
    unsigned* amax_f = amax + NST_AMAX_SLOTS;
    HIPCHK(ctx, launch_zero(amax_f, NST_AMAX_SLOTS, s));
    HIPCHK(ctx, launch_absmax_slots(f, (size_t)h * w * C, amax_f, s));
    PatchSearch p{};
    p.f = f; p.h = h; p.w = w; p.C = C; p.amax_f = amax_f; p.d = d; p.keys = keys;
    HIPCHK(ctx, launch_pm_search(p, idx_out, score_out, s));
    return sc.finish();
}

// The descriptors of the guided search alone: planes at the MAP's resolution -> (count, 4), count the entries of the
// stride-`stride` geometry of an hm x wm map.
int nst_patch_descriptors(nst_ctx* ctx, const float* planes, int R, int hm, int wm, int stride, double epsilon, float* out, void* stream) {
    NSTCHK(bind(ctx));
    if (!planes || !out) return fail(ctx, NST_E_ARG, "null argument");
    if (R < 1 || R > NST_MAX_REGIONS) return fail(ctx, NST_E_ARG, "the number of regions must be 1 .. NST_MAX_REGIONS");
    if (hm < 3 || wm < 3) return fail(ctx, NST_E_ARG, "the map must be at least 3x3");
    if (stride < 1 || stride > 8) return fail(ctx, NST_E_ARG, "the style stride must be 1..8");
    if (!(epsilon > 0.0) || std::isinf(epsilon)) return fail(ctx, NST_E_ARG, "the patch epsilon must be finite and > 0");
    const long long count = (long long)((hm - 3) / stride + 1) * ((wm - 3) / stride + 1);
    if (count > (1ll << 30) || (double)R * hm * wm >= 2147483648.0) return fail(ctx, NST_E_ARG, "the map is too large");
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIPCHK(ctx, launch_pm_descriptors(planes, R, hm, wm, stride, epsilon, (int)count, out, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    return NST_OK;
}

// nst_patch_match under guidance: the norms of the image patches and a zero-padded copy of e on scratch, then the guided search
int nst_patch_match_guided(nst_ctx* ctx, const float* f, int h, int w, int C, const float* fs, int hs, int ws, int stride, double epsilon,
                           int R, const float* d_img, const float* e_dict, float gamma, int* idx_out, float* score_out, void* stream) {
    NSTCHK(bind(ctx));
    PatchDict d;
    NSTCHK(patch_args(ctx, f, h, w, C, fs, hs, ws, stride, &d));
    if ((!idx_out && !score_out) || !d_img || !e_dict) return fail(ctx, NST_E_ARG, "null argument");
    if (!(epsilon > 0.0) || std::isinf(epsilon)) return fail(ctx, NST_E_ARG, "the patch epsilon must be finite and > 0");
    if (R < 1 || R > NST_MAX_REGIONS) return fail(ctx, NST_E_ARG, "the number of regions must be 1 .. NST_MAX_REGIONS");
    if (!(gamma >= 0.f) || std::isinf(gamma)) return fail(ctx, NST_E_ARG, "the semantic weight must be finite and >= 0");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t n = (size_t)(h - 2) * (w - 2), padded = (size_t)pm_dict_tiles(d.m) * 32;
    PatchDict own{};
    own.fs = f;
    if (!pm_dict_geometry(h, w, C, 1, &own)) return fail(ctx, NST_E_ARG, "bad map geometry");
    Scratch sc(ctx, s);
    unsigned* amax = nullptr; float* rq = nullptr; unsigned char* packed = nullptr; unsigned long long* keys = nullptr;
    float* rp = nullptr; float* ge = nullptr;
    NSTCHK(sc.alloc(&amax, (size_t)2 * NST_AMAX_SLOTS));
    NSTCHK(sc.alloc(&rq, padded));
    NSTCHK(sc.alloc(&packed, pm_packed_bytes(d.m, C)));
    NSTCHK(sc.alloc(&keys, n));
    NSTCHK(sc.alloc(&rp, (size_t)pm_dict_tiles((int)n) * 32));
    NSTCHK(sc.alloc(&ge, padded * 4));
    HIPCHK(ctx, launch_pm_prepare(d, epsilon, amax, rq, packed, s));
    d.amax = amax; d.rq = rq; d.packed = packed;
    unsigned* amax_f = amax + NST_AMAX_SLOTS;
    HIPCHK(ctx, launch_zero(amax_f, NST_AMAX_SLOTS, s));
    HIPCHK(ctx, launch_absmax_slots(f, (size_t)h * w * C, amax_f, s));
    HIPCHK(ctx, launch_pm_norms(own, epsilon, rp, s));
    HIPCHK(ctx, hipMemsetAsync(ge, 0, padded * 4 * sizeof(float), s));
    HIPCHK(ctx, hipMemcpyAsync(ge, e_dict, (size_t)d.m * 4 * sizeof(float), hipMemcpyDeviceToDevice, s));
    PatchSearch p{};
    p.f = f; p.h = h; p.w = w; p.C = C; p.amax_f = amax_f; p.d = d; p.keys = keys;
    p.gd = d_img; p.ge = ge; p.rp = rp; p.gamma = gamma;
    HIPCHK(ctx, launch_pm_search(p, idx_out, score_out, s));
    return sc.finish();
}

int nst_patch_term(nst_ctx* ctx, const float* f, int h, int w, int C, const float* fs, int hs, int ws, int stride, const int* idx,
                   float coef, float* value_out, float* grad_out, void* stream) {
    NSTCHK(bind(ctx));
    PatchDict d;
    NSTCHK(patch_args(ctx, f, h, w, C, fs, hs, ws, stride, &d));
    if (!idx || (!value_out && !grad_out)) return fail(ctx, NST_E_ARG, "null argument");
    if (!std::isfinite(coef)) return fail(ctx, NST_E_ARG, "the coefficient must be finite");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const PatchTerm t{f, h, w, idx, d};
    Scratch sc(ctx, s);
    if (value_out) {
        double* partial = nullptr;
        NSTCHK(sc.alloc(&partial, (size_t)PM_VALUE_BLOCKS));
        HIPCHK(ctx, launch_pm_value_partials(t, partial, s));
        HIPCHK(ctx, launch_pm_value(partial, 9.0 * (double)C * (double)(h - 2) * (double)(w - 2), value_out, s));
    }
    if (grad_out) HIPCHK(ctx, launch_pm_grad(t, coef, grad_out, 0, s));
    return sc.finish();
}

// The histogram loss's pieces on their own (include/nst_hip.h has the definition): the kernels of histogram.hip.  Synchronous.
static int hist_args(nst_ctx* ctx, long long N, int C, int bins) {
    if (!hist_channels_ok(C)) return fail(ctx, NST_E_ARG, "the histogram loss takes maps of 64, 128, 256 or 512 channels");
    if (bins < 2 || bins > 1024) return fail(ctx, NST_E_ARG, "the number of bins must be 2..1024");
    if (N < 1 || (double)N * C >= 2147483648.0) return fail(ctx, NST_E_ARG, "the map must have 1 <= N and N C < 2^31");
    return NST_OK;
}

int nst_histogram_counts(nst_ctx* ctx, const float* f, long long N, int C, int bins, float* lo_hi_out, unsigned* counts_out, void* stream) {
    NSTCHK(bind(ctx));
    if (!f || !lo_hi_out || !counts_out) return fail(ctx, NST_E_ARG, "null argument");
    NSTCHK(hist_args(ctx, N, C, bins));
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIPCHK(ctx, launch_hist_counts(f, (size_t)N, C, bins, lo_hi_out, counts_out, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    return NST_OK;
}

int nst_histogram_tables(nst_ctx* ctx, const float* lo_hi, const unsigned* counts, long long N, const float* s_lo_hi, const unsigned* s_counts,
                         long long Ns, int C, int bins, float* ends_out, void* stream) {
    NSTCHK(bind(ctx));
    if (!lo_hi || !counts || !s_lo_hi || !s_counts || !ends_out) return fail(ctx, NST_E_ARG, "null argument");
    NSTCHK(hist_args(ctx, N, C, bins));
    NSTCHK(hist_args(ctx, Ns, C, bins));
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIPCHK(ctx, launch_hist_tables(counts, (size_t)N, s_lo_hi, s_counts, (size_t)Ns, C, bins, ends_out, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    return NST_OK;
}

int nst_histogram_term(nst_ctx* ctx, const float* f, long long N, int C, int bins, const float* lo_hi, const float* ends, float coef,
                       float* value_out, float* grad_out, void* stream) {
    NSTCHK(bind(ctx));
    if (!f || !lo_hi || !ends || (!value_out && !grad_out)) return fail(ctx, NST_E_ARG, "null argument");
    NSTCHK(hist_args(ctx, N, C, bins));
    if (!std::isfinite(coef)) return fail(ctx, NST_E_ARG, "the coefficient must be finite");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const HistTerm t{f, (size_t)N, C, bins, lo_hi, ends};
    Scratch sc(ctx, s);
    if (value_out) {
        double* partial = nullptr;
        NSTCHK(sc.alloc(&partial, (size_t)HIST_VALUE_BLOCKS));
        HIPCHK(ctx, launch_hist_value_partials(t, partial, s));
        HIPCHK(ctx, launch_hist_value(partial, (double)C * (double)N, value_out, s));
    }
    if (grad_out) HIPCHK(ctx, launch_hist_grad(t, coef, grad_out, 0, s));
    return sc.finish();
}

// The relaxed EMD term's pieces on their own (include/nst_hip.h has the definition): the kernels of remd.hip on scratch buffers.
// Synchronous.
static int remd_args(nst_ctx* ctx, const float* f, int h, int w, int C, const float* fs, int hs, int ws, int si, int ss, double epsilon,
                     RemdSide* x, RemdSide* y) {
    if (!f || !fs) return fail(ctx, NST_E_ARG, "null argument");
    if (C != 64 && C != 128 && C != 256 && C != 512) return fail(ctx, NST_E_ARG, "the relaxed EMD term takes maps of 64, 128, 256 or 512 channels");
    if (h < 1 || w < 1 || hs < 1 || ws < 1) return fail(ctx, NST_E_ARG, "the map and the style map must be at least 1x1");
    if (si < 1 || si > 256 || ss < 1 || ss > 256) return fail(ctx, NST_E_ARG, "the sample strides must be 1..256");
    if (!(epsilon > 0.0) || std::isinf(epsilon)) return fail(ctx, NST_E_ARG, "the relaxed EMD epsilon must be finite and > 0");
    *x = RemdSide{}; *y = RemdSide{};
    if (!remd_side_geometry(h, w, C, si, x) || !remd_side_geometry(hs, ws, C, ss, y)) return fail(ctx, NST_E_ARG, "the map is too large");
    x->f = f; y->f = fs;
    return NST_OK;
}

int nst_remd_match(nst_ctx* ctx, const float* f, int h, int w, int C, const float* fs, int hs, int ws, int si, int ss, double epsilon,
                   int* nnA_out, int* nnB_out, void* stream) {
    NSTCHK(bind(ctx));
    RemdSide x, y;
    NSTCHK(remd_args(ctx, f, h, w, C, fs, hs, ws, si, ss, epsilon, &x, &y));
    if (!nnA_out || !nnB_out) return fail(ctx, NST_E_ARG, "null argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    Scratch sc(ctx, s);
    RemdSide* sides[2] = {&x, &y};
    unsigned* amax = nullptr;
    NSTCHK(sc.alloc(&amax, (size_t)2 * NST_AMAX_SLOTS));
    HIPCHK(ctx, launch_zero(amax, (size_t)2 * NST_AMAX_SLOTS, s));
    for (int k = 0; k < 2; ++k) {
        RemdSide& d = *sides[k];
        float* r = nullptr; unsigned char* packed = nullptr;
        NSTCHK(sc.alloc(&r, (size_t)remd_tiles(d.count) * 32));
        NSTCHK(sc.alloc(&packed, remd_packed_bytes(d.count, C)));
        HIPCHK(ctx, launch_absmax_slots(d.f, (size_t)d.h * d.w * C, amax + k * NST_AMAX_SLOTS, s));
        d.amax = amax + k * NST_AMAX_SLOTS;
        HIPCHK(ctx, launch_remd_norms(d, epsilon, r, s));
        HIPCHK(ctx, launch_remd_pack(d, packed, s));
        d.r = r; d.packed = packed;
    }
    unsigned long long* keys = nullptr;
    NSTCHK(sc.alloc(&keys, (size_t)(x.count > y.count ? x.count : y.count)));
    HIPCHK(ctx, launch_remd_search(y, x, keys, nnA_out, s));
    HIPCHK(ctx, launch_remd_search(x, y, keys, nnB_out, s));
    return sc.finish();
}

int nst_remd_term(nst_ctx* ctx, const float* f, int h, int w, int C, const float* fs, int hs, int ws, int si, int ss, double epsilon,
                  const int* nnA, const int* nnB, int side, float coef, float* value_out, int* side_out, float* grad_out, void* stream) {
    NSTCHK(bind(ctx));
    RemdSide x, y;
    NSTCHK(remd_args(ctx, f, h, w, C, fs, hs, ws, si, ss, epsilon, &x, &y));
    if (!nnA || !nnB || (!value_out && !side_out && !grad_out)) return fail(ctx, NST_E_ARG, "null argument");
    if (side < -1 || side > 1) return fail(ctx, NST_E_ARG, "side must be 0 (A), 1 (B) or -1 (decide)");
    if (!std::isfinite(coef)) return fail(ctx, NST_E_ARG, "the coefficient must be finite");
    hipStream_t s = static_cast<hipStream_t>(stream);
    Scratch sc(ctx, s);
    float* rp = nullptr; float* rq = nullptr; float* cosA = nullptr; float* cosB = nullptr; float* rec = nullptr; int* sd = nullptr;
    double* partial = nullptr;
    NSTCHK(sc.alloc(&rp, (size_t)remd_tiles(x.count) * 32));
    NSTCHK(sc.alloc(&rq, (size_t)remd_tiles(y.count) * 32));
    NSTCHK(sc.alloc(&cosA, (size_t)x.count));
    NSTCHK(sc.alloc(&cosB, (size_t)y.count));
    NSTCHK(sc.alloc(&rec, 4));
    NSTCHK(sc.alloc(&sd, 4));
    NSTCHK(sc.alloc(&partial, (size_t)2 * REMD_VALUE_BLOCKS));
    HIPCHK(ctx, launch_remd_norms(x, epsilon, rp, s));
    HIPCHK(ctx, launch_remd_norms(y, epsilon, rq, s));
    x.r = rp; y.r = rq;
    const RemdTerm t{x, y, nnA, nnB, cosA, cosB, rec, sd};
    HIPCHK(ctx, launch_remd_value(t, epsilon, side, partial, nullptr, s));
    if (value_out) HIPCHK(ctx, hipMemcpyAsync(value_out, rec, 3 * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (side_out) HIPCHK(ctx, hipMemcpyAsync(side_out, sd, sizeof(int), hipMemcpyDeviceToDevice, s));
    if (grad_out)
        HIPCHK(ctx, launch_remd_grad(t, (float)((double)coef / (double)x.count), (float)((double)coef / (double)y.count), grad_out, 0, s));
    return sc.finish();
}

// The self-similarity term's pieces on their own (include/nst_hip.h has the definition): the kernels of selfsim.hip on scratch
// buffers.  Synchronous.
// one sample set on scratch: the absmax record, the norms, the packed operand, D, s and q
struct SelfSimSet { RemdSide x; float* D; double* s; double* q; };
static int selfsim_args(nst_ctx* ctx, const float* f, int h, int w, int C, int stride, double epsilon, RemdSide* x) {
    if (!f) return fail(ctx, NST_E_ARG, "null argument");
    if (C != 64 && C != 128 && C != 256 && C != 512) return fail(ctx, NST_E_ARG, "the self-similarity term takes maps of 64, 128, 256 or 512 channels");
    if (h < 1 || w < 1) return fail(ctx, NST_E_ARG, "the map must be at least 1x1");
    if (stride < 1 || stride > 256) return fail(ctx, NST_E_ARG, "the sample stride must be 1..256");
    if (!(epsilon > 0.0) || std::isinf(epsilon)) return fail(ctx, NST_E_ARG, "the self-similarity epsilon must be finite and > 0");
    *x = RemdSide{};
    if (!remd_side_geometry(h, w, C, stride, x)) return fail(ctx, NST_E_ARG, "the map is too large");
    if (x->count > SELFSIM_MAX_SAMPLES) return fail(ctx, NST_E_ARG, "the stride leaves more than 4096 samples");
    x->f = f;
    return NST_OK;
}
static int selfsim_set(nst_ctx* ctx, Scratch& sc, const RemdSide& geom, double epsilon, double* part, SelfSimSet* out, hipStream_t s) {
    RemdSide x = geom;
    const size_t n = (size_t)x.count;
    unsigned* amax = nullptr; float* r = nullptr; unsigned char* packed = nullptr;
    NSTCHK(sc.alloc(&amax, (size_t)NST_AMAX_SLOTS));
    NSTCHK(sc.alloc(&r, (size_t)remd_tiles(x.count) * 32));
    NSTCHK(sc.alloc(&packed, remd_packed_bytes(x.count, x.C)));
    NSTCHK(sc.alloc(&out->D, n * n));
    NSTCHK(sc.alloc(&out->s, n));
    NSTCHK(sc.alloc(&out->q, n));
    HIPCHK(ctx, launch_zero(amax, (size_t)NST_AMAX_SLOTS, s));
    HIPCHK(ctx, launch_absmax_slots(x.f, (size_t)x.h * x.w * x.C, amax, s));
    x.amax = amax;
    HIPCHK(ctx, launch_remd_norms(x, epsilon, r, s));
    x.r = r;
    HIPCHK(ctx, launch_remd_pack(x, packed, s));
    x.packed = packed;
    HIPCHK(ctx, launch_selfsim_matrix(x, out->D, s));
    HIPCHK(ctx, launch_selfsim_colsums(out->D, x.count, epsilon, part, out->s, out->q, s));
    out->x = x;
    return NST_OK;
}

int nst_selfsim_matrix(nst_ctx* ctx, const float* f, int h, int w, int C, int stride, double epsilon, float* D_out, double* s_out, void* stream) {
    NSTCHK(bind(ctx));
    RemdSide x;
    NSTCHK(selfsim_args(ctx, f, h, w, C, stride, epsilon, &x));
    if (!D_out && !s_out) return fail(ctx, NST_E_ARG, "null argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    Scratch sc(ctx, s);
    const size_t n = (size_t)x.count;
    double* part = nullptr;
    NSTCHK(sc.alloc(&part, (size_t)SELFSIM_ROW_BLOCKS * n));
    SelfSimSet a{};
    NSTCHK(selfsim_set(ctx, sc, x, epsilon, part, &a, s));
    if (D_out) HIPCHK(ctx, hipMemcpyAsync(D_out, a.D, n * n * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (s_out) HIPCHK(ctx, hipMemcpyAsync(s_out, a.s, n * sizeof(double), hipMemcpyDeviceToDevice, s));
    return sc.finish();
}

int nst_selfsim_term(nst_ctx* ctx, const float* f, const float* fc, int h, int w, int C, int stride, double epsilon, float coef, float* value_out,
                     signed char* sg_out, float* grad_out, void* stream) {
    NSTCHK(bind(ctx));
    RemdSide x, y;
    NSTCHK(selfsim_args(ctx, f, h, w, C, stride, epsilon, &x));
    NSTCHK(selfsim_args(ctx, fc, h, w, C, stride, epsilon, &y));
    if (!value_out && !sg_out && !grad_out) return fail(ctx, NST_E_ARG, "null argument");
    if (!std::isfinite(coef)) return fail(ctx, NST_E_ARG, "the coefficient must be finite");
    hipStream_t s = static_cast<hipStream_t>(stream);
    Scratch sc(ctx, s);
    const size_t n = (size_t)x.count;
    double* part = nullptr; double* t = nullptr; signed char* sg = nullptr; float* val = nullptr;
    NSTCHK(sc.alloc(&part, (size_t)2 * SELFSIM_ROW_BLOCKS * n));
    NSTCHK(sc.alloc(&t, n));
    NSTCHK(sc.alloc(&sg, n * n));
    NSTCHK(sc.alloc(&val, 4));
    SelfSimSet a{}, b{};
    NSTCHK(selfsim_set(ctx, sc, y, epsilon, part, &b, s));
    NSTCHK(selfsim_set(ctx, sc, x, epsilon, part, &a, s));
    const SelfSimTerm term{a.D, a.q, b.D, b.q, x.count, sg, part, t, val};
    HIPCHK(ctx, launch_selfsim_value(term, s));
    if (value_out) HIPCHK(ctx, hipMemcpyAsync(value_out, val, sizeof(float), hipMemcpyDeviceToDevice, s));
    if (sg_out) HIPCHK(ctx, hipMemcpyAsync(sg_out, sg, n * n, hipMemcpyDeviceToDevice, s));
    if (grad_out) {
        float* W = nullptr; float* U = nullptr;
        NSTCHK(sc.alloc(&W, n * n));
        NSTCHK(sc.alloc(&U, n * (size_t)C));
        HIPCHK(ctx, launch_selfsim_grad(a.x, term, (float)((double)coef / (double)x.count), W, U, grad_out, 0, s));
    }
    return sc.finish();
}

// The long-range style term's pieces on their own (include/nst_hip.h has the definition): the kernels of xcorr.hip on scratch
// buffers.  Synchronous.
// the n items of one map on scratch (the absmax record, per shift the slabs); G, and with a target S, St and sq, are the caller's
static int xcorr_items(nst_ctx* ctx, Scratch& sc, const float* f, int h, int w, int C, const int* shifts, int n, XcorrItem* items,
                       int* geometry_out, hipStream_t s) {
    if (!f || !shifts) return fail(ctx, NST_E_ARG, "null argument");
    if (ctx->conv_mode != 2) return fail(ctx, NST_E_STATE, "the xcorr term runs in the f16x2 arithmetic only (NST_CONV unset)");
    if (C != 64 && C != 128 && C != 256 && C != 512) return fail(ctx, NST_E_ARG, "the xcorr term takes maps of 64, 128, 256 or 512 channels");
    if (n < 1 || n > XCORR_MAX_SHIFTS) return fail(ctx, NST_E_ARG, "the xcorr term takes 1..16 shifts");
    unsigned* amax = nullptr;
    NSTCHK(sc.alloc(&amax, (size_t)NST_AMAX_SLOTS));
    HIPCHK(ctx, launch_zero(amax, (size_t)NST_AMAX_SLOTS, s));
    for (int d = 0; d < n; ++d) {
        XcorrGeometry geo;
        if (!xcorr_geometry(C, h, w, shifts[2 * d], shifts[2 * d + 1], &geo))
            return fail(ctx, NST_E_ARG, "a shift (dx, dy) has 0 <= dx < w, 0 <= dy < h, not both 0 (or the map is too large)");
        if (geometry_out) { geometry_out[2 * d] = geo.nsplit; geometry_out[2 * d + 1] = geo.pix_per_split; }
        XcorrItem& it = items[d];
        it = XcorrItem{};
        NSTCHK(sc.alloc(&it.part, (size_t)geo.nsplit * C * C));
        it.f = f; it.amax = amax; it.C = C; it.h = h; it.w = w; it.dx = shifts[2 * d]; it.dy = shifts[2 * d + 1];
        it.divisor = (float)((double)C * (double)(h - it.dy) * (double)(w - it.dx));
    }
    HIPCHK(ctx, launch_absmax_slots(f, (size_t)h * w * C, amax, s));
    return NST_OK;
}
static int xcorr_launch(nst_ctx* ctx, const XcorrItem* items, int n, hipStream_t s) {
    for (int d0 = 0; d0 < n; d0 += XCORR_BATCH_MAX) {
        XcorrBatch b{};
        b.n = std::min(n - d0, XCORR_BATCH_MAX);
        for (int d = 0; d < b.n; ++d) b.it[d] = items[d0 + d];
        HIPCHK(ctx, launch_xcorr_batch(b, s));
    }
    return NST_OK;
}

int nst_xcorr(nst_ctx* ctx, const float* f, int h, int w, int C, const int* shifts, int n, float* out, int* geometry_out, void* stream) {
    NSTCHK(bind(ctx));
    if (!out) return fail(ctx, NST_E_ARG, "null argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    Scratch sc(ctx, s);
    XcorrItem items[XCORR_MAX_SHIFTS];
    NSTCHK(xcorr_items(ctx, sc, f, h, w, C, shifts, n, items, geometry_out, s));
    for (int d = 0; d < n; ++d) items[d].G = out + (size_t)d * C * C;
    NSTCHK(xcorr_launch(ctx, items, n, s));
    return sc.finish();
}

int nst_xcorr_term(nst_ctx* ctx, const float* f, int h, int w, int C, const float* gt, const int* shifts, int n, float coef, float* value_out,
                   float* grad_out, void* stream) {
    NSTCHK(bind(ctx));
    if (!gt || (!value_out && !grad_out)) return fail(ctx, NST_E_ARG, "null argument");
    if (!std::isfinite(coef)) return fail(ctx, NST_E_ARG, "the coefficient must be finite");
    hipStream_t s = static_cast<hipStream_t>(stream);
    Scratch sc(ctx, s);
    XcorrItem items[XCORR_MAX_SHIFTS];
    NSTCHK(xcorr_items(ctx, sc, f, h, w, C, shifts, n, items, nullptr, s));
    const size_t CC = (size_t)C * C;
    float* S = nullptr; float* St = nullptr; double* sq = nullptr; float* val = nullptr;
    NSTCHK(sc.alloc(&S, (size_t)n * CC));
    NSTCHK(sc.alloc(&St, (size_t)n * CC));
    NSTCHK(sc.alloc(&sq, (size_t)n * xcorr_finish_blocks(C)));
    NSTCHK(sc.alloc(&val, 4));
    for (int d = 0; d < n; ++d) {
        XcorrItem& it = items[d];
        it.target = gt + d * CC; it.S = S + d * CC; it.St = St + d * CC; it.sq = sq + (size_t)d * xcorr_finish_blocks(C);
        it.coef = (float)(2.0 * (double)coef / ((double)n * (double)C * (double)C * (double)C * (double)(h - it.dy) * (double)(w - it.dx)));
    }
    NSTCHK(xcorr_launch(ctx, items, n, s));
    if (value_out) {
        XcorrValueBatch vb{};
        vb.n = 1;
        vb.it[0] = XcorrValueItem{sq, n, xcorr_finish_blocks(C), (double)C * (double)C, val};
        HIPCHK(ctx, launch_xcorr_values(vb, s));
        HIPCHK(ctx, hipMemcpyAsync(value_out, val, sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    if (grad_out) {
        XcorrGrad g{};
        g.f = f; g.h = h; g.w = w; g.C = C; g.nd = n;
        for (int d = 0; d < n; ++d) { g.dx[d] = items[d].dx; g.dy[d] = items[d].dy; }
        g.S = S; g.St = St; g.out = grad_out; g.accumulate = 0;
        HIPCHK(ctx, launch_xcorr_grad(g, s));
    }
    return sc.finish();
}

// The warp of a sequence (include/nst_hip.h): out = src sampled bilinearly at p + flow(p), valid (nullable) = the four taps
// lie inside the image.  Synchronous.
int nst_warp_bilinear(nst_ctx* ctx, const float* src, const float* flow, int C, int h, int w, float* out, float* valid, void* stream) {
    NSTCHK(bind(ctx));
    if (!src || !flow || !out) return fail(ctx, NST_E_ARG, "null argument");
    if (C < 1 || h < 1 || w < 1) return fail(ctx, NST_E_ARG, "the image must be at least 1x1 with one plane");
    if (out == src) return fail(ctx, NST_E_ARG, "the warp does not run in place");
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIPCHK(ctx, launch_warp_bilinear(src, flow, C, h, w, out, valid, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    return NST_OK;
}

// The reliability plane of a forward / backward flow pair (include/nst_hip.h).  Synchronous.
int nst_flow_weights(nst_ctx* ctx, const float* fwd, const float* bwd, int h, int w, float* out, void* stream) {
    NSTCHK(bind(ctx));
    if (!fwd || !bwd || !out) return fail(ctx, NST_E_ARG, "null argument");
    if (h < 1 || w < 1) return fail(ctx, NST_E_ARG, "the flow fields must be at least 1x1");
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIPCHK(ctx, launch_flow_weights(fwd, bwd, h, w, out, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    return NST_OK;
}

// `na` floats at a and `nb` floats at b share memory (either null: no)
static bool flow_overlap(const float* a, size_t na, const float* b, size_t nb) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a && b && a0 < b0 + nb * sizeof(float) && b0 < a0 + na * sizeof(float);
}

// The long-term anchor (include/nst_hip.h): J warped results under J reliability planes -> the one anchor and weight plane a
// level holds.  One launch; the pointers travel as a kernel argument; nothing is allocated.  Asynchronous on `stream`.
static_assert(NST_FOLD_MAX_SOURCES == NST_MAX_ANCHOR_SOURCES, "nst_kernels.h and include/nst_hip.h disagree about the source cap");
int nst_anchor_fold(nst_ctx* ctx, int J, const float* const* sources, const float* const* weights, int C, int h, int w, float* anchor,
                    float* weight, float* parts, void* stream) {
    NSTCHK(bind(ctx));
    if (J < 1 || J > NST_MAX_ANCHOR_SOURCES) return fail(ctx, NST_E_ARG, "J must lie in 1 .. NST_MAX_ANCHOR_SOURCES");
    if (C != 1 && C != 3) return fail(ctx, NST_E_ARG, "C must be 3, or 1 for a luminance plane");
    if (h < 1 || w < 1) return fail(ctx, NST_E_ARG, "the image must be at least 1x1");
    if (!sources || !weights || !anchor || !weight) return fail(ctx, NST_E_ARG, "null argument");
    const size_t hw = (size_t)h * w, chw = (size_t)C * hw;
    AnchorFoldArgs a{};
    for (int j = 0; j < J; ++j) {
        if (!sources[j] || !weights[j]) return fail(ctx, NST_E_ARG, "null source or weight plane");
        a.sources[j] = sources[j];
        a.weights[j] = weights[j];
    }
    const float* const outs[3] = {anchor, weight, parts};
    const size_t out_n[3] = {chw, hw, (size_t)J * hw};
    bool clash = flow_overlap(anchor, chw, weight, hw) || flow_overlap(anchor, chw, parts, out_n[2]) || flow_overlap(weight, hw, parts, out_n[2]);
    for (int o = 0; o < 3 && !clash; ++o)
        for (int j = 0; j < J && !clash; ++j)
            clash = flow_overlap(sources[j], chw, outs[o], out_n[o]) || flow_overlap(weights[j], hw, outs[o], out_n[o]);
    if (clash) return fail(ctx, NST_E_ARG, "an output overlaps an input or another output: the fold does not run in place");
    HIPCHK(ctx, launch_anchor_fold(a, J, C, h, w, anchor, weight, parts, static_cast<hipStream_t>(stream)));
    return NST_OK;
}

// ---- the flow estimator (include/nst_hip.h, nst_flow_estimate; flow.hip).  The caller owns every buffer: the context
// allocates nothing here, so nst_ctx_bytes does not move.  All synchronous.
static_assert(NST_FLOW_MAX_SCALES == NST_MAX_FLOW_SCALES, "nst_kernels.h and include/nst_hip.h disagree about the scale cap");

// alpha is finite and > 0 and its fp32 square, the smoothness weight the sweep divides by, a normal number (a square that
// underflows leaves a pixel without a data term with 0 / 0)
static bool flow_alpha_ok(float alpha) {
    const float a2 = alpha * alpha;
    return std::isfinite(alpha) && alpha > 0.f && std::isnormal(a2);
}
static const char* const kFlowAlpha = "alpha must be finite and > 0 and its fp32 square a normal number";
static const char* const kFlowOverlap = "an output overlaps another argument: no stage of the flow estimator runs in place";

int nst_flow_workspace(int h, int w, int scales, size_t* floats, int* scales_used) {
    FlowLayout l;
    if (flow_layout(h, w, scales, &l) != 0) return NST_E_ARG;
    if (floats) *floats = l.floats;
    if (scales_used) *scales_used = l.scales;
    return NST_OK;
}

int nst_flow_estimate(nst_ctx* ctx, const float* from, const float* to, int h, int w, float alpha, int scales, int warps,
                      int iterations, float* flow, float* workspace, size_t workspace_floats, void* stream) {
    NSTCHK(bind(ctx));
    if (!from || !to || !flow || !workspace) return fail(ctx, NST_E_ARG, "null argument");
    if (h < 1 || w < 1) return fail(ctx, NST_E_ARG, "the images must be at least 1x1");
    if (!flow_alpha_ok(alpha)) return fail(ctx, NST_E_ARG, kFlowAlpha);
    if (warps < 1 || iterations < 1) return fail(ctx, NST_E_ARG, "warps and iterations must be at least 1");
    FlowLayout l;
    if (flow_layout(h, w, scales, &l) != 0) return fail(ctx, NST_E_ARG, "scales must lie in 0 .. NST_MAX_FLOW_SCALES");
    if (workspace_floats < l.floats) return fail(ctx, NST_E_ARG, "the workspace is smaller than nst_flow_workspace says");
    const size_t hw = (size_t)h * w;
    if (flow_overlap(from, hw, flow, 2 * hw) || flow_overlap(to, hw, flow, 2 * hw) || flow_overlap(workspace, l.floats, flow, 2 * hw) ||
        flow_overlap(from, hw, workspace, l.floats) || flow_overlap(to, hw, workspace, l.floats))
        return fail(ctx, NST_E_ARG, kFlowOverlap);
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIPCHK(ctx, launch_flow_estimate(from, to, l, alpha * alpha, warps, iterations, flow, workspace, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    return NST_OK;
}

int nst_flow_reduce(nst_ctx* ctx, const float* in, int h, int w, float* out, void* stream) {
    NSTCHK(bind(ctx));
    if (!in || !out) return fail(ctx, NST_E_ARG, "null argument");
    if (h < 1 || w < 1) return fail(ctx, NST_E_ARG, "the image must be at least 1x1");
    if (flow_overlap(in, (size_t)h * w, out, (size_t)((h + 1) / 2) * ((w + 1) / 2))) return fail(ctx, NST_E_ARG, kFlowOverlap);
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIPCHK(ctx, launch_flow_reduce(in, h, w, out, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    return NST_OK;
}

int nst_flow_prolong(nst_ctx* ctx, const float* coarse, int h, int w, float* fine, void* stream) {
    NSTCHK(bind(ctx));
    if (!coarse || !fine) return fail(ctx, NST_E_ARG, "null argument");
    if (h < 1 || w < 1) return fail(ctx, NST_E_ARG, "the fine grid must be at least 1x1");
    if (flow_overlap(coarse, 2 * (size_t)((h + 1) / 2) * ((w + 1) / 2), fine, 2 * (size_t)h * w)) return fail(ctx, NST_E_ARG, kFlowOverlap);
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIPCHK(ctx, launch_flow_prolong(coarse, h, w, fine, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    return NST_OK;
}

int nst_flow_linearize(nst_ctx* ctx, const float* from, const float* to, const float* flow, int h, int w, float* ix, float* iy,
                       float* rho, void* stream) {
    NSTCHK(bind(ctx));
    if (!from || !to || !flow || !ix || !iy || !rho) return fail(ctx, NST_E_ARG, "null argument");
    if (h < 1 || w < 1) return fail(ctx, NST_E_ARG, "the images must be at least 1x1");
    const size_t hw = (size_t)h * w;
    float* const outs[3] = {ix, iy, rho};
    for (int i = 0; i < 3; ++i)
        if (flow_overlap(from, hw, outs[i], hw) || flow_overlap(to, hw, outs[i], hw) || flow_overlap(flow, 2 * hw, outs[i], hw) ||
            flow_overlap(outs[(i + 1) % 3], hw, outs[i], hw))
            return fail(ctx, NST_E_ARG, kFlowOverlap);
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIPCHK(ctx, launch_flow_linearize(from, to, flow, flow + hw, h, w, ix, iy, rho, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    return NST_OK;
}

int nst_flow_sweeps(nst_ctx* ctx, const float* ix, const float* iy, const float* rho, const float* flow_in, int h, int w, float alpha,
                    int n, float* flow_out, float* scratch, void* stream) {
    NSTCHK(bind(ctx));
    if (!ix || !iy || !rho || !flow_in || !flow_out || (n > 1 && !scratch)) return fail(ctx, NST_E_ARG, "null argument");
    if (h < 1 || w < 1 || n < 1) return fail(ctx, NST_E_ARG, "the planes must be at least 1x1 and n at least 1");
    if (!flow_alpha_ok(alpha)) return fail(ctx, NST_E_ARG, kFlowAlpha);
    const size_t hw = (size_t)h * w;
    float* const outs[2] = {flow_out, n > 1 ? scratch : nullptr};       // (scratch is not touched for n = 1)
    for (int i = 0; i < 2; ++i)
        if (flow_overlap(ix, hw, outs[i], 2 * hw) || flow_overlap(iy, hw, outs[i], 2 * hw) || flow_overlap(rho, hw, outs[i], 2 * hw) ||
            flow_overlap(flow_in, 2 * hw, outs[i], 2 * hw) || (i == 1 && flow_overlap(flow_out, 2 * hw, outs[i], 2 * hw)))
            return fail(ctx, NST_E_ARG, kFlowOverlap);
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIPCHK(ctx, launch_flow_sweeps(ix, iy, rho, flow_in, h, w, alpha * alpha, n, flow_out, scratch, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    return NST_OK;
}

// ---- TV-L1 (include/nst_hip.h, nst_flow_tvl1_estimate; flow_tvl1.hip) on the same terms: the caller's buffers, synchronous.
// lambda, theta, tau are finite and > 0 and the two constants of the iteration, lt = lambda theta and taut = tau / theta (the
// fp32 product and quotient), normal numbers
static bool flow_tvl1_ok(float lambda, float theta, float tau) {
    const float lt = lambda * theta, taut = tau / theta;
    return std::isfinite(lambda) && lambda > 0.f && std::isfinite(theta) && theta > 0.f && std::isfinite(tau) && tau > 0.f &&
           std::isnormal(lt) && std::isnormal(taut);
}
static const char* const kFlowTvl1 = "lambda, theta and tau must be finite and > 0, and lambda theta and tau / theta normal fp32 numbers";

int nst_flow_tvl1_workspace(int h, int w, int scales, size_t* floats, int* scales_used) {
    FlowTvl1Layout t;
    if (flow_tvl1_layout(h, w, scales, &t) != 0) return NST_E_ARG;
    if (floats) *floats = t.floats;
    if (scales_used) *scales_used = t.hs.scales;
    return NST_OK;
}

int nst_flow_tvl1_estimate(nst_ctx* ctx, const float* from, const float* to, int h, int w, float lambda, float theta, float tau,
                           int scales, int warps, int iterations, float* flow, float* workspace, size_t workspace_floats, void* stream) {
    NSTCHK(bind(ctx));
    if (!from || !to || !flow || !workspace) return fail(ctx, NST_E_ARG, "null argument");
    if (h < 1 || w < 1) return fail(ctx, NST_E_ARG, "the images must be at least 1x1");
    if (!flow_tvl1_ok(lambda, theta, tau)) return fail(ctx, NST_E_ARG, kFlowTvl1);
    if (warps < 1 || iterations < 1) return fail(ctx, NST_E_ARG, "warps and iterations must be at least 1");
    FlowTvl1Layout t;
    if (flow_tvl1_layout(h, w, scales, &t) != 0) return fail(ctx, NST_E_ARG, "scales must lie in 0 .. NST_MAX_FLOW_SCALES");
    if (workspace_floats < t.floats) return fail(ctx, NST_E_ARG, "the workspace is smaller than nst_flow_tvl1_workspace says");
    const size_t hw = (size_t)h * w;
    if (flow_overlap(from, hw, flow, 2 * hw) || flow_overlap(to, hw, flow, 2 * hw) || flow_overlap(workspace, t.floats, flow, 2 * hw) ||
        flow_overlap(from, hw, workspace, t.floats) || flow_overlap(to, hw, workspace, t.floats))
        return fail(ctx, NST_E_ARG, kFlowOverlap);
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIPCHK(ctx, launch_flow_tvl1_estimate(from, to, t, lambda * theta, theta, tau / theta, warps, iterations, flow, workspace, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    return NST_OK;
}

int nst_flow_tvl1_iterations(nst_ctx* ctx, const float* ix, const float* iy, const float* rho, const float* flow_in,
                             const float* dual_in, int h, int w, float lambda, float theta, float tau, int n, float* flow_out,
                             float* dual_out, float* scratch, void* stream) {
    NSTCHK(bind(ctx));
    if (!ix || !iy || !rho || !flow_in || !dual_in || !flow_out || !dual_out || (n > 1 && !scratch))
        return fail(ctx, NST_E_ARG, "null argument");
    if (h < 1 || w < 1 || n < 1) return fail(ctx, NST_E_ARG, "the planes must be at least 1x1 and n at least 1");
    if (!flow_tvl1_ok(lambda, theta, tau)) return fail(ctx, NST_E_ARG, kFlowTvl1);
    const size_t hw = (size_t)h * w;
    const float* const outs[3] = {flow_out, dual_out, n > 1 ? scratch : nullptr};       // (scratch is not touched for n = 1)
    const size_t sizes[3] = {2 * hw, 4 * hw, 6 * hw};
    for (int i = 0; i < 3; ++i) {
        if (flow_overlap(ix, hw, outs[i], sizes[i]) || flow_overlap(iy, hw, outs[i], sizes[i]) || flow_overlap(rho, hw, outs[i], sizes[i]) ||
            flow_overlap(flow_in, 2 * hw, outs[i], sizes[i]) || flow_overlap(dual_in, 4 * hw, outs[i], sizes[i]))
            return fail(ctx, NST_E_ARG, kFlowOverlap);
        for (int j = 0; j < i; ++j)
            if (flow_overlap(outs[j], sizes[j], outs[i], sizes[i])) return fail(ctx, NST_E_ARG, kFlowOverlap);
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIPCHK(ctx, launch_flow_tvl1_iterations(ix, iy, rho, flow_in, dual_in, h, w, lambda * theta, theta, tau / theta, n, flow_out, dual_out,
                                            n > 1 ? scratch : nullptr, n > 1 ? scratch + 2 * hw : nullptr, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    return NST_OK;
}

int nst_bicubic_half(nst_ctx* ctx, const float* x, int C, int h, int w, float* y, void* stream) {
    NSTCHK(bind(ctx));
    if (!x || !y || h < 2 || w < 2) return fail(ctx, NST_E_ARG, "bad argument");
    HIPCHK(ctx, launch_bicubic_down(x, C, h, w, h / 2, w / 2, y, static_cast<hipStream_t>(stream)));
    return NST_OK;
}
int nst_bicubic_half_backward(nst_ctx* ctx, const float* gy, int C, int h, int w, float* gx, void* stream) {
    NSTCHK(bind(ctx));
    if (!gy || !gx || h < 2 || w < 2) return fail(ctx, NST_E_ARG, "bad argument");
    HIPCHK(ctx, launch_bicubic_down_bwd(gy, C, h, w, h / 2, w / 2, gx, 0, static_cast<hipStream_t>(stream)));
    return NST_OK;
}
int nst_prepare_img(nst_ctx* ctx, const float* hwc, int h, int w, float* chw, void* stream) {
    NSTCHK(bind(ctx));
    if (!hwc || !chw) return fail(ctx, NST_E_ARG, "null argument");
    HIPCHK(ctx, launch_prepare_img(hwc, h, w, chw, static_cast<hipStream_t>(stream)));
    return NST_OK;
}
int nst_unprepare_img(nst_ctx* ctx, const float* chw, int h, int w, float* hwc, void* stream) {
    NSTCHK(bind(ctx));
    if (!hwc || !chw) return fail(ctx, NST_E_ARG, "null argument");
    HIPCHK(ctx, launch_unprepare_img(chw, h, w, hwc, static_cast<hipStream_t>(stream)));
    return NST_OK;
}

// ---- job set-up on the device -------------------------------------------------
int nst_resize_bicubic(nst_ctx* ctx, const float* src, int h, int w, int channels, float* dst, int nh, int nw, void* stream) {
    NSTCHK(bind(ctx));
    if (!src || !dst || h < 1 || w < 1 || nh < 1 || nw < 1 || channels < 1) return fail(ctx, NST_E_ARG, "bad argument");
    HIPCHK(ctx, launch_resize_hwc(src, h, w, channels, dst, nh, nw, static_cast<hipStream_t>(stream)));
    return NST_OK;
}
int nst_gather_rows(nst_ctx* ctx, const float* src, const long long* perm, size_t rows, int channels, float* dst, void* stream) {
    NSTCHK(bind(ctx));
    if (!src || !perm || !dst || channels < 1) return fail(ctx, NST_E_ARG, "bad argument");
    HIPCHK(ctx, launch_gather_rows(src, perm, rows, channels, dst, static_cast<hipStream_t>(stream)));
    return NST_OK;
}
int nst_gaussian_mask_accumulate(nst_ctx* ctx, float* acc, const float* src, int h, int w, int channels, double central,
                                 double peripheral, double dispersion, void* stream) {
    NSTCHK(bind(ctx));
    if (!acc || h < 1 || w < 1 || channels < 1) return fail(ctx, NST_E_ARG, "bad argument");
    HIPCHK(ctx, launch_gauss_mask_acc(acc, src, h, w, channels, central, peripheral, dispersion, static_cast<hipStream_t>(stream)));
    return NST_OK;
}
int nst_noise_blend(nst_ctx* ctx, const float* content, const float* noise, int h, int w, int channels, double noise_factor,
                    float* out, void* stream) {
    NSTCHK(bind(ctx));
    if (!content || !noise || !out || h < 1 || w < 1 || channels < 1) return fail(ctx, NST_E_ARG, "bad argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t n = (size_t)h * w * channels;
    Scratch sc(ctx, s);
    double* t0 = nullptr; double* t1 = nullptr; double* wt = nullptr;
    NSTCHK(sc.alloc(&t0, n));
    NSTCHK(sc.alloc(&t1, n));
    NSTCHK(sc.alloc(&wt, n));
    hipError_t e = launch_blend_weight(content, h, w, channels, noise_factor, t0, t1, wt, s);
    if (e == hipSuccess) e = launch_blend_init(content, noise, wt, n, out, s);
    HIPCHK(ctx, e);
    return sc.finish();
}
int nst_scale(nst_ctx* ctx, const float* src, float alpha, size_t n, float* dst, void* stream) {
    NSTCHK(bind(ctx));
    if (!src || !dst) return fail(ctx, NST_E_ARG, "null argument");
    HIPCHK(ctx, launch_scale(src, alpha, n, dst, static_cast<hipStream_t>(stream)));
    return NST_OK;
}

// ---- colour preservation: set-up entry points (Gatys et al. 2016) ------------------------------------------------------
int nst_color_stats(nst_ctx* ctx, const float* hwc, int h, int w, double* mean, double* cov, void* stream) {
    NSTCHK(bind(ctx));
    if (!hwc || !mean || !cov || h < 1 || w < 1) return fail(ctx, NST_E_ARG, "bad argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    // the context's own scratch (kept: no allocation or free, and so no device-wide synchronisation, per call)
    if (!ctx->color_scratch) NSTCHK(ctx->mem.alloc(ctx, &ctx->color_scratch, (size_t)COLOR_BLOCKS * 9 + 12));
    double* dev = ctx->color_scratch;
    double host[12];
    HIPCHK(ctx, launch_color_stats(hwc, (size_t)h * w, dev, dev + (size_t)COLOR_BLOCKS * 9, dev + (size_t)COLOR_BLOCKS * 9 + 3, s));
    HIPCHK(ctx, hipMemcpyAsync(host, dev + (size_t)COLOR_BLOCKS * 9, sizeof(host), hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));       // synchronous: the scratch is free again when this returns
    std::memcpy(mean, host, 3 * sizeof(double));
    std::memcpy(cov, host + 3, 9 * sizeof(double));
    return NST_OK;
}

namespace {
// eigen-decomposition of a symmetric 3x3 matrix by cyclic Jacobi rotations (fp64): a = V diag(e) V^T, columns of V
void jacobi3(const double* a_in, double* e, double* V) {
    double a[3][3];
    for (int i = 0; i < 9; ++i) { a[i / 3][i % 3] = 0.5 * (a_in[i] + a_in[(i % 3) * 3 + i / 3]); V[i] = (i % 4 == 0) ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < 64; ++sweep) {
        const double off = a[0][1] * a[0][1] + a[0][2] * a[0][2] + a[1][2] * a[1][2];
        const double diag = a[0][0] * a[0][0] + a[1][1] * a[1][1] + a[2][2] * a[2][2];
        if (off <= 1e-300 || off <= 1e-34 * diag) break;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                if (a[p][q] == 0.0) continue;
                const double theta = (a[q][q] - a[p][p]) / (2.0 * a[p][q]);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), sn = t * c;
                for (int k = 0; k < 3; ++k) {           // a <- a J (columns p, q)
                    const double akp = a[k][p], akq = a[k][q];
                    a[k][p] = c * akp - sn * akq;
                    a[k][q] = sn * akp + c * akq;
                }
                for (int k = 0; k < 3; ++k) {           // a <- J^T a (rows p, q)
                    const double apk = a[p][k], aqk = a[q][k];
                    a[p][k] = c * apk - sn * aqk;
                    a[q][k] = sn * apk + c * aqk;
                }
                for (int k = 0; k < 3; ++k) {           // V <- V J
                    const double vkp = V[k * 3 + p], vkq = V[k * 3 + q];
                    V[k * 3 + p] = c * vkp - sn * vkq;
                    V[k * 3 + q] = sn * vkp + c * vkq;
                }
            }
    }
    for (int i = 0; i < 3; ++i) e[i] = a[i][i];
}
// out = V diag(f(e)) V^T
void sym_apply(const double* V, const double* fe, double* out) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double acc = 0.0;
            for (int k = 0; k < 3; ++k) acc += V[i * 3 + k] * fe[k] * V[j * 3 + k];
            out[i * 3 + j] = acc;
        }
}
// the YIQ (NTSC) matrix of nst_luminance_recombine and its fp64 inverse (adjugate / determinant)
ColorAffine yiq_inverse() {
    const double m[3][3] = {{0.299, 0.587, 0.114}, {0.595716, -0.274453, -0.321263}, {0.211456, -0.522591, 0.311135}};
    ColorAffine r{};
    const double det = m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) +
                       m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const int a0 = (j + 1) % 3, a1 = (j + 2) % 3, b0 = (i + 1) % 3, b1 = (i + 2) % 3;
            r.m[i][j] = (m[a0][b0] * m[a1][b1] - m[a0][b1] * m[a1][b0]) / det;
        }
    return r;
}
}  // namespace

int nst_color_transfer_matrix(const double* mean_c, const double* cov_c, const double* mean_s, const double* cov_s, double* A,
                              double* b) {
    if (!mean_c || !cov_c || !mean_s || !cov_s || !A || !b) return fail(nullptr, NST_E_ARG, "null argument");
    double ec[3], Vc[9], es[3], Vs[9], fc[3], fs[3], Rc[9], Rs[9];
    jacobi3(cov_c, ec, Vc);
    jacobi3(cov_s, es, Vs);
    for (int k = 0; k < 3; ++k) {
        fc[k] = std::sqrt(std::max(ec[k], 0.0));                  // Sigma_c^{1/2}
        fs[k] = 1.0 / std::sqrt(std::max(es[k], 1e-10));          // Sigma_s^{-1/2}, eigenvalues clamped below at 1e-10
    }
    sym_apply(Vc, fc, Rc);
    sym_apply(Vs, fs, Rs);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double acc = 0.0;
            for (int k = 0; k < 3; ++k) acc += Rc[i * 3 + k] * Rs[k * 3 + j];
            A[i * 3 + j] = acc;
        }
    for (int i = 0; i < 3; ++i) b[i] = mean_c[i] - (A[i * 3] * mean_s[0] + A[i * 3 + 1] * mean_s[1] + A[i * 3 + 2] * mean_s[2]);
    return NST_OK;
}

int nst_color_affine(nst_ctx* ctx, const float* src, int h, int w, const double* A, const double* b, float* dst, void* stream) {
    NSTCHK(bind(ctx));
    if (!src || !dst || !A || !b || h < 1 || w < 1) return fail(ctx, NST_E_ARG, "bad argument");
    ColorAffine a{};
    for (int i = 0; i < 9; ++i) a.m[i / 3][i % 3] = A[i];
    for (int i = 0; i < 3; ++i) a.b[i] = b[i];
    HIPCHK(ctx, launch_color_affine(src, (size_t)h * w, a, dst, static_cast<hipStream_t>(stream)));
    return NST_OK;
}

int nst_luminance(nst_ctx* ctx, const float* hwc, int h, int w, double alpha, double beta, float* out, void* stream) {
    NSTCHK(bind(ctx));
    if (!hwc || !out || h < 1 || w < 1) return fail(ctx, NST_E_ARG, "bad argument");
    HIPCHK(ctx, launch_luminance(hwc, (size_t)h * w, alpha, beta, out, static_cast<hipStream_t>(stream)));
    return NST_OK;
}

int nst_luminance_recombine(nst_ctx* ctx, const float* u, const float* content, int h, int w, float* out, void* stream) {
    NSTCHK(bind(ctx));
    if (!u || !content || !out || h < 1 || w < 1) return fail(ctx, NST_E_ARG, "bad argument");
    static const ColorAffine inv = yiq_inverse();
    HIPCHK(ctx, launch_luminance_recombine(u, content, (size_t)h * w, inv, out, static_cast<hipStream_t>(stream)));
    return NST_OK;
}

}  // extern "C"
