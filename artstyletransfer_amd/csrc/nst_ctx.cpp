// nst_ctx.cpp - context and job state of libnst_hip.so (include/nst_hip.h): the VGG19 weights re-laid-out for the gfx950
// kernels (three arithmetic modes), context creation and destruction, the job settings (pyramid, taps, colour, pooling) with
// the per-level workspace they size, the ordering of caller streams against context-owned memory, and launch timing.
//
// Host-side control only; every FLOP and byte of the path is in the .hip kernels.
#include <algorithm>
#include <atomic>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "nst_ctx.h"

using namespace nst;

namespace {
thread_local std::string g_err;
}

int nst::fail(nst_ctx* ctx, int code, const std::string& msg) {
    if (ctx) ctx->err = msg; else g_err = msg;
    return code;
}

namespace nst {

// Debugging aid (tools/check_uninit_reads.py): NST_POISON_ALLOC=all | <first>-<last> fills the allocations with those
// sequence numbers with 0xFF bytes (NaN as floats, all-ones as masks), so that a kernel which reads memory nobody wrote -
// harmless on a fresh process, whose pages arrive zeroed, and wrong once the allocator recycles another context's blocks -
// shows in the results of a single job.
void poison_if_asked(void* p, size_t bytes) {
    static const char* spec = getenv("NST_POISON_ALLOC");
    static std::atomic<long> seq{0};
    if (!spec || !*spec) return;
    const long k = seq++;
    long lo = 0, hi = -1;
    if (strcmp(spec, "all") == 0) hi = LONG_MAX;
    else if (sscanf(spec, "%ld-%ld", &lo, &hi) != 2) return;
    if (k >= lo && k <= hi) { (void)hipMemset(p, 0xFF, bytes); (void)hipStreamSynchronize(nullptr); }
    if (getenv("NST_POISON_TRACE")) fprintf(stderr, "nst alloc #%ld: %zu bytes%s\n", k, bytes, (k >= lo && k <= hi) ? " (poisoned)" : "");
}
// hipMemset on device memory is enqueued on the NULL stream and returns before it has run: with another context's work
// queued there (two jobs per GPU is the scheduler's default) it lands AFTER the first kernels of this context, which run on
// the caller's non-blocking stream - and wipes what they wrote (absmax records -> a zero scale -> NaN targets; Adam
// moments; the packed loss rows).  Set-up-time zero fills therefore run on a stream of their own and are waited for:
// nothing of a context rides on the null stream.
int zero_now(void* p, size_t bytes) {
    hipStream_t zs = nullptr;
    hipError_t e = hipStreamCreateWithFlags(&zs, hipStreamNonBlocking);
    if (e != hipSuccess) return 1;
    e = hipMemsetAsync(p, 0, bytes, zs);
    if (e == hipSuccess) e = hipStreamSynchronize(zs);
    (void)hipStreamDestroy(zs);
    return e == hipSuccess ? 0 : 1;
}

int dev_alloc(nst_ctx* ctx, void** p, size_t bytes, size_t* charged) {
    if (bytes == 0) bytes = 16;
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) return fail(ctx, NST_E_NOMEM, std::string("hipMalloc(") + std::to_string(bytes) + "): " + hipGetErrorString(e));
    poison_if_asked(*p, bytes);
    ctx->bytes += bytes;
    if (charged) *charged = bytes;
    return NST_OK;
}
void dev_release(nst_ctx* ctx, void* p, size_t bytes) {
    (void)hipFree(p);
    ctx->bytes -= bytes;
}

int alloc_acts(nst_ctx* ctx, ActSet& a, int h, int w) {
    for (int l = 0; l < NL; ++l) {
        a.h[l] = h >> kScale[l];
        a.w[l] = w >> kScale[l];
        if (a.h[l] < 1 || a.w[l] < 1) return fail(ctx, NST_E_ARG, "image too small for VGG19 (needs >= 16 px per side)");
        const size_t n = (size_t)a.h[l] * a.w[l] * kCout[l];
        NSTCHK(a.mem.alloc(ctx, &a.act[l], n));
    }
    for (int k = 0; k < 4; ++k) {
        const int l = kPoolAfter[k];
        const size_t n = (size_t)(a.h[l] / 2) * (a.w[l] / 2) * kCout[l];
        NSTCHK(a.mem.alloc(ctx, &a.pool[k], n));
        NSTCHK(a.mem.alloc(ctx, &a.pcode[k], n / 8));          // n / 32 channel groups x 4 words
    }
    size_t need = 0;
    for (int l = 1; l < NL; ++l) {
        const size_t px = (size_t)a.h[l] * a.w[l];
        const int sf = std::max(conv_ksplit(a.h[l], a.w[l], kCin[l], kCout[l]), conv_bf3_ksplit(a.h[l], a.w[l], kCin[l], kCout[l]));
        const int sb = std::max(conv_ksplit(a.h[l], a.w[l], kCout[l], kCin[l]), conv_bf3_ksplit(a.h[l], a.w[l], kCout[l], kCin[l]));
        const size_t fwd = (size_t)sf * px * kCout[l];
        const size_t bwd = (size_t)sb * px * kCin[l];
        if (fwd > px * kCout[l] && fwd > need) need = fwd;
        if (bwd > px * kCin[l] && bwd > need) need = bwd;
    }
    // layers m whose ReLU mask a non-pooling input-gradient launch consumes
    const int mask_layers[9] = {0, 2, 4, 5, 6, 8, 9, 10, 12};     // (12: the Gram backward at relu5_1)
    for (int k = 0; k < 9; ++k) {
        const int m = mask_layers[k];
        const size_t nw = (size_t)a.h[m] * a.w[m] * (kCout[m] / 32);
        NSTCHK(a.mem.alloc(ctx, &a.bits[m], nw));
    }
    NSTCHK(a.mem.alloc(ctx, &a.amax, (size_t)AMAX_IDS * NST_AMAX_SLOTS));
    if (zero_now(a.amax, (size_t)AMAX_IDS * NST_AMAX_SLOTS * 4)) return fail(ctx, NST_E_HIP, "hipMemset failed");
    a.splitk_floats = need;
    if (need) NSTCHK(a.mem.alloc(ctx, &a.splitk, need));
    return NST_OK;
}

}  // namespace nst

namespace {

// fp32 -> three bf16 pieces that sum to it exactly (same cut as conv_bf3.hip::cut3)
void cut3_host(float a, uint16_t& h, uint16_t& m, uint16_t& l) {
    uint32_t u; std::memcpy(&u, &a, 4);
    const uint32_t uh = u & 0xFFFF0000u;
    float fh; std::memcpy(&fh, &uh, 4);
    const float r1 = a - fh;
    uint32_t u1; std::memcpy(&u1, &r1, 4);
    const uint32_t um = u1 & 0xFFFF0000u;
    float fm; std::memcpy(&fm, &um, 4);
    const float r2 = r1 - fm;
    uint32_t u2; std::memcpy(&u2, &r2, 4);
    h = (uint16_t)(uh >> 16); m = (uint16_t)(um >> 16); l = (uint16_t)(u2 >> 16);
}
// w: [taps][rows][K] fp32  ->  out: [taps][rows][K/32][3][32] bf16
void make_bf3(const float* w, int taps, int rows, int K, std::vector<uint16_t>& out) {
    const int nch = K / 32;
    out.assign((size_t)taps * rows * nch * 96, 0);
    for (int t = 0; t < taps; ++t)
        for (int r = 0; r < rows; ++r)
            for (int k = 0; k < K; ++k) {
                uint16_t h, m, l;
                cut3_host(w[((size_t)t * rows + r) * K + k], h, m, l);
                const size_t base = (((size_t)t * rows + r) * nch + k / 32) * 96 + (k % 32);
                out[base] = h; out[base + 32] = m; out[base + 64] = l;
            }
}

// fp32 <-> fp16 on the host with integer arithmetic (round to nearest even, subnormals, overflow to infinity: bit-identical to
// the compiler's _Float16 conversions over 4e7 random values) - without F16C code generation those go through a soft-float
// call each, and a context converts ~1e8 weights: 0.5 s of its 0.8 s creation.
static inline uint16_t f32_to_f16(float f) {
    uint32_t x; std::memcpy(&x, &f, 4);
    const uint32_t sign = (x >> 16) & 0x8000u;
    x &= 0x7FFFFFFFu;
    uint32_t o;
    if (x >= 0x47800000u) {                      // >= 65536 (rounds to infinity), infinity, NaN
        o = (x > 0x7F800000u) ? 0x7E00u : 0x7C00u;
    } else if (x < 0x38800000u) {                // < 2^-14: a half subnormal or zero: round(f * 2^24) through a float add
        float a; std::memcpy(&a, &x, 4);
        const uint32_t magic_bits = (uint32_t)((127 - 15) + (23 - 10) + 1) << 23;
        float magic; std::memcpy(&magic, &magic_bits, 4);
        a += magic;
        uint32_t ab; std::memcpy(&ab, &a, 4);
        o = ab - magic_bits;
    } else {                                     // normal: re-bias the exponent, round to nearest even on bit 13
        const uint32_t odd = (x >> 13) & 1u;
        x += 0xC8000FFFu + odd;
        o = x >> 13;
    }
    return (uint16_t)(sign | o);
}
static inline float f16_to_f32(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3FFu;
    uint32_t b;
    if (e == 0) { const float f = (float)m * 5.9604644775390625e-8f; std::memcpy(&b, &f, 4); b |= sign; }
    else if (e == 31) b = sign | 0x7F800000u | (m << 13);
    else b = sign | ((e + 112u) << 23) | (m << 13);
    float r; std::memcpy(&r, &b, 4);
    return r;
}

// w: [taps][rows][K] fp32  ->  out: [taps][rows][K/kc][2][kc] fp16 pieces of w * s, s = the power of two that
// brings the largest |w| into [2^14, 2^15); *inv = 1 / s (same cut as conv_h2.hip::cut2x4).  kc = channels per K
// chunk of the kernel shape that consumes these weights: 32 when `rows` (its output channels) is a multiple of
// 128 and K (its input channels) > NST_H2_SHORTK_CIN, else 16 (conv_h2.hip, shapes in use).
static int h2_chunk(int rows, int K) { return (rows % 128 == 0 && K > NST_H2_SHORTK_CIN) ? 32 : 16; }
void make_h2(const float* w, int taps, int rows, int K, std::vector<uint16_t>& out, float* inv) {
    const int kc = h2_chunk(rows, K);
    const size_t n = (size_t)taps * rows * K;
    float mx = 0.f;
    for (size_t i = 0; i < n; ++i) mx = std::max(mx, std::fabs(w[i]));
    int ex = 0;
    if (mx > 0.f) (void)std::frexp(mx, &ex);          // mx = f * 2^ex, f in [0.5, 1)
    const float s = std::ldexp(1.f, 15 - ex);          // mx * s in [2^14, 2^15)
    *inv = std::ldexp(1.f, ex - 15);
    const int nch = K / kc;
    out.assign((size_t)taps * rows * nch * 2 * kc, 0);
    for (int t = 0; t < taps; ++t)
        for (int r = 0; r < rows; ++r)
            for (int k = 0; k < K; ++k) {
                const float x = w[((size_t)t * rows + r) * K + k] * s;
                const uint16_t uh = f32_to_f16(x);
                const uint16_t ul = f32_to_f16((x - f16_to_f32(uh)) * 2048.f);
                const size_t base = (((size_t)t * rows + r) * nch + k / kc) * 2 * kc + (k % kc);
                out[base] = uh; out[base + kc] = ul;
            }
}

// h2: make_h2's image of a 16-channel-chunk layer, [9][rows][K/16][2][16] fp16  ->  the SAME pieces in the order a lane's
// v_mfma_f32_32x32x16_f16 B operand wants them (conv_h2.hip, DIRECT): 16-byte units [chunk][tap][rows/32][piece][lane], lane
// (r = lane & 31, h = lane >> 5) holding input channels chunk*16 + 8 h .. + 7 of output channel tile*32 + r - one 16-byte
// buffer load per (32-channel tile, piece) yields a fragment, and a wave walks the image front to back.
void make_h2_frag(const std::vector<uint16_t>& h2, int rows, int K, std::vector<uint16_t>& out) {
    const int nch = K / 16, nct = rows / 32;
    out.assign(h2.size(), 0);
    for (int ch = 0; ch < nch; ++ch)
        for (int t = 0; t < 9; ++t)
            for (int ct = 0; ct < nct; ++ct)
                for (int s = 0; s < 2; ++s)
                    for (int lane = 0; lane < 64; ++lane) {
                        const int r = lane & 31, h = lane >> 5;
                        const uint16_t* src = h2.data() + ((((size_t)t * rows + ct * 32 + r) * nch + ch) * 2 + s) * 16 + 8 * h;
                        uint16_t* dst = out.data() + ((((((size_t)ch * 9 + t) * nct + ct) * 2 + s) * 64) + lane) * 8;
                        for (int j = 0; j < 8; ++j) dst[j] = src[j];
                    }
}

// w: [9 taps = ky*3 + kx][rows = Cout][K = Cin] fp32  ->  the 1-D Winograd F(2,3) weights of conv_wino.hip: for every ky the
// four transformed taps u0 = g0, u1 = (g0 + g1 + g2)/2, u2 = (g0 - g1 + g2)/2, u3 = g2 (fp64), scaled by the power of two that
// brings the largest |u| into [2^14, 2^15), cut into two fp16 pieces, in MFMA FRAGMENT order - 16-byte units
// [Cout/128][K/32][ky][wave = xi + 4 wn][k-step][n tile][piece][lane]: lane (r = lane & 31, h = lane >> 5) holds the 8 input
// channels chunk*32 + kstep*16 + 8 h .. + 7 of output channel ct*128 + wn*64 + ntile*32 + r.
void make_wino(const float* w, int rows, int K, std::vector<uint16_t>& out, float* inv) {
    const int nct = rows / 128, nch = K / 32;
    // the transformed taps once, [ky][xi][Cout][Cin], and their largest magnitude
    std::vector<float> U((size_t)12 * rows * K);
    float mx = 0.f;
    for (int ky = 0; ky < 3; ++ky)
        for (int o = 0; o < rows; ++o) {
            const float* g0 = w + ((size_t)(ky * 3 + 0) * rows + o) * K;
            const float* g1 = w + ((size_t)(ky * 3 + 1) * rows + o) * K;
            const float* g2 = w + ((size_t)(ky * 3 + 2) * rows + o) * K;
            float* u0 = U.data() + ((size_t)(ky * 4 + 0) * rows + o) * K;
            float* u1 = U.data() + ((size_t)(ky * 4 + 1) * rows + o) * K;
            float* u2 = U.data() + ((size_t)(ky * 4 + 2) * rows + o) * K;
            float* u3 = U.data() + ((size_t)(ky * 4 + 3) * rows + o) * K;
            for (int c = 0; c < K; ++c) {
                const double a = g0[c], b = g1[c], d = g2[c];
                u0[c] = (float)a;
                u1[c] = (float)(0.5 * (a + b + d));
                u2[c] = (float)(0.5 * (a - b + d));
                u3[c] = (float)d;
                mx = std::max(std::max(mx, std::fabs(u0[c])), std::max(std::fabs(u1[c]), std::max(std::fabs(u2[c]), std::fabs(u3[c]))));
            }
        }
    int ex = 0;
    if (mx > 0.f) (void)std::frexp(mx, &ex);
    const float s = std::ldexp(1.f, 15 - ex);
    *inv = std::ldexp(1.f, ex - 15);
    out.assign((size_t)nct * nch * 3 * 8 * 2 * 2 * 2 * 64 * 8, 0);
    for (int ct = 0; ct < nct; ++ct)
        for (int ch = 0; ch < nch; ++ch)
            for (int ky = 0; ky < 3; ++ky)
                for (int wave = 0; wave < 8; ++wave)
                    for (int ks = 0; ks < 2; ++ks)
                        for (int nt = 0; nt < 2; ++nt) {
                            const int x = wave & 3, wn = wave >> 2;
                            const size_t unit0 = ((((((size_t)(ct * nch + ch) * 3 + ky) * 8 + wave) * 2 + ks) * 2 + nt) * 2) * 64;
                            for (int lane = 0; lane < 64; ++lane) {
                                const int r = lane & 31, h = lane >> 5;
                                const int o = ct * 128 + wn * 64 + nt * 32 + r;
                                const float* src = U.data() + ((size_t)(ky * 4 + x) * rows + o) * K + ch * 32 + ks * 16 + 8 * h;
                                uint16_t* hi_dst = out.data() + (unit0 + lane) * 8;             // piece 0
                                uint16_t* lo_dst = out.data() + (unit0 + 64 + lane) * 8;        // piece 1
                                for (int j = 0; j < 8; ++j) {
                                    const float v = src[j] * s;
                                    hi_dst[j] = f32_to_f16(v);
                                    lo_dst[j] = f32_to_f16((v - f16_to_f32(hi_dst[j])) * 2048.f);
                                }
                            }
                        }
}

// the tap-sized buffers of a level (LevelWs has the list), for the context's current taps
void free_tap_buffers(LevelWs& L) {
    L.tap_mem.release();
    L.content_t = nullptr; L.content_n = 0;
    for (int k = 0; k < kMaxStyle; ++k) { L.gram_t[k] = nullptr; L.S[k] = nullptr; L.S_bf[k] = nullptr; L.style_partial[k] = nullptr; }
    L.gram_part = nullptr; L.gram_part_floats = 0;
}
int alloc_tap_buffers(nst_ctx* ctx, LevelWs& L) {
    const Taps& tp = ctx->taps;
    const int m = tp.content;
    L.content_n = (size_t)L.acts.h[m] * L.acts.w[m] * kCout[m];
    NSTCHK(L.tap_mem.alloc(ctx, &L.content_t, L.content_n));
    for (int k = 0; k < tp.nstyle; ++k) {
        const int C = kCout[tp.style[k]];
        NSTCHK(L.tap_mem.alloc(ctx, &L.gram_t[k], (size_t)C * C));
        NSTCHK(L.tap_mem.alloc(ctx, &L.S[k], (size_t)C * C));
        NSTCHK(L.tap_mem.alloc(ctx, &L.S_bf[k], (size_t)C * C * 3));
        NSTCHK(L.tap_mem.alloc(ctx, &L.style_partial[k], gram_finish_blocks(C)));
    }
    L.gram_part_floats = gram_part_floats_for(tp, L.h, L.w);
    NSTCHK(L.tap_mem.alloc(ctx, &L.gram_part, L.gram_part_floats));
    return NST_OK;
}

// the level image and its gradient of an h x w level under `channels` (nst_job_set_color)
int alloc_level_image(nst_ctx* ctx, LevelImage& im, int channels, int h, int w) {
    const size_t n = (size_t)channels * h * w;
    NSTCHK(im.mem.alloc(ctx, &im.xl, n));
    NSTCHK(im.mem.alloc(ctx, &im.gxl, n));
    return NST_OK;
}

void free_level(LevelWs& L) {
    if (L.stream) (void)hipStreamDestroy(L.stream);
    if (L.done) (void)hipEventDestroy(L.done);
    L = LevelWs();      // (every member's DevMem gives back what it holds)
}

}  // namespace

namespace nst {

// What a closure remembered is void once the job changes: the captured graph and the keys it was captured under, and
// (drop_targets) every level's targets
void drop_closure_state(nst_ctx* ctx, bool drop_targets) {
    if (ctx->gexec) { (void)hipGraphExecDestroy(ctx->gexec); ctx->gexec = nullptr; }
    ctx->gkey = {}; ctx->glast = {};
    for (int i = 0; drop_targets && i < ctx->levels; ++i) { ctx->lv[i].targets = false; ctx->lv[i].guide.targets = false; }
    if (drop_targets) forget_forward_pass(ctx);
}
void forget_forward_pass(nst_ctx* ctx) {
    for (int i = 0; i < NST_MAX_LEVELS; ++i) {
        ctx->lv[i].acts.pass = 0; ctx->lv[i].acts.pass_n = 0;
        for (bool& st : ctx->lv[i].acts.stored) st = false;
    }
}

// folds the event pairs of the previous closure into the accumulators (waits for them to complete)
int fold_timed(nst_ctx* ctx) {
    if (!ctx->timed_valid) return NST_OK;
    HIPCHK(ctx, hipEventSynchronize(ctx->t1));
    float ms = 0.f;
    HIPCHK(ctx, hipEventElapsedTime(&ms, ctx->t0, ctx->t1));
    ctx->acc_closure_ms += ms;
    if (!ctx->timed_backward) {          // (a backward half belongs to the closure its forward half counted)
        ctx->acc_closures += 1;
        if (!ctx->timed.empty()) ctx->acc_sampled += 1;
    }
    ctx->timed_backward = false;
    for (const TimedLaunch& t : ctx->timed) {
        float d = 0.f;
        HIPCHK(ctx, hipEventSynchronize(t.b));
        HIPCHK(ctx, hipEventElapsedTime(&d, t.a, t.b));
        ctx->acc_ms[t.cls] += d;
        ctx->acc_flops[t.cls] += t.flops;
        {
            // f16x2: 3 MFMAs per product block, bf16x3: 6, fp32 MFMA: 1 (conv1_1 and the streaming kernels run no 16-bit MFMA)
            const double mode = (t.cls == K_CONV3 || t.cls == K_GRAM) ? (ctx->conv_mode == 2 ? 3.0 : ctx->conv_mode == 1 ? 6.0 : 1.0) : 1.0;
            ctx->acc_mfma[t.cls] += t.flops * (t.mfma_factor >= 0.0 ? t.mfma_factor : mode);
        }
        ctx->acc_launches[t.cls] += 1;
    }
    ctx->timed.clear();
    ctx->ev_used = 0;
    ctx->timed_valid = false;
    return NST_OK;
}

int bind(nst_ctx* ctx) {
    if (!ctx) return fail(nullptr, NST_E_ARG, "null context");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return NST_OK;
}

// Remember where the context's work ends: an event on the caller's stream after the last launch of an entry point that
// reads or writes context-owned memory.
void mark(nst_ctx* ctx, hipStream_t s) {
    if (ctx && ctx->tail && hipEventRecord(ctx->tail, s) == hipSuccess) { ctx->tail_stream = s; ctx->tail_set = true; }
}
// The entry points that read or write context-owned memory (targets, workspace, level images) are ordered as they are
// issued, whatever stream each is issued on: a call on ANOTHER stream than the previous one first makes its stream wait for
// the context's tail event.  One tail event then covers everything the context has in flight - what nst_job_configure and
// nst_ctx_destroy wait for before they free the workspace - without relying on hipFree's implicit synchronisation, and a
// read-back issued on a second stream (nst_level_image after nst_closure) sees the closure's results.
hipStream_t enter(nst_ctx* ctx, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (ctx->tail_set && s != ctx->tail_stream) (void)hipStreamWaitEvent(s, ctx->tail, 0);
    return s;
}
// Wait until nothing on the device uses the context's memory any more: its tail event and its own streams - NOT
// hipDeviceSynchronize, which would stall the other job sharing the GPU (two jobs per GPU is the scheduler's default).
void quiesce(nst_ctx* ctx) {
    if (ctx->tail) (void)hipEventSynchronize(ctx->tail);
    for (int i = 0; i < NST_MAX_LEVELS; ++i)
        if (ctx->lv[i].stream) (void)hipStreamSynchronize(ctx->lv[i].stream);
    if (ctx->gstream) (void)hipStreamSynchronize(ctx->gstream);
    if (ctx->side) (void)hipStreamSynchronize(ctx->side);
}

}  // namespace nst

namespace {

int env_flag(const char* name, int dflt) {
    const char* e = getenv(name);
    if (!e || !e[0]) return dflt;
    return std::atoi(e);
}

// bit i = map i has a positive style layer weight
unsigned positive_weight_mask(const float* w) {
    unsigned m = 0;
    for (int i = 0; i < 6; ++i) if (w[i] > 0.f) m |= 1u << i;
    return m;
}
unsigned style_mask_of(const Taps& tp) {
    unsigned m = 0;
    for (int q = 0; q < tp.nstyle; ++q) m |= 1u << tap_index_of(tp.style[q]);
    return m;
}

// An optional term's per-level block replaced by what fill builds (an untouched block: the term is off), every buffer
// allocated beside the old ones: a refusal changes nothing; else every level's targets and the captured closure go
template <typename Block, typename Fill>
int replace_term(nst_ctx* ctx, Block LevelWs::*member, Fill fill) {
    return replace_blocks(ctx->lv, ctx->levels, member, fill, [&] { quiesce(ctx); drop_closure_state(ctx, true); });
}

// ---- what the per-map terms (MapTerm: MRF, histogram loss, relaxed EMD, self-similarity, xcorr) share outside a closure -----------------------------
// how the refusals of a term's setter name it ("the <adj> weights", "no <name>"), and what the term asks of the job besides
// (any_used_map: a weight may sit on the job's content map as well as on a style map, and the image the setter is given is
// the level's content image, not a style image)
struct MapTermWords { const char* adj; const char* name; bool f16x2_only; bool min_3x3; bool any_used_map; };
const MapTermWords kMrfWords{"MRF", "MRF term", true, true, false};
const MapTermWords kHistWords{"histogram", "histogram loss", false, false, false};
const MapTermWords kRemdWords{"relaxed EMD", "relaxed EMD term", true, false, false};
const MapTermWords kSelfSimWords{"self-similarity", "self-similarity term", true, false, true};
const MapTermWords kXcorrWords{"xcorr", "xcorr term", true, false, false};

// every level's per-map terms go (they hold maps of the style image as the job's network saw it: the setters again)
void drop_map_terms(nst_ctx* ctx) {
    for (int i = 0; i < ctx->levels; ++i) {
        ctx->lv[i].pm = PatchLevel();
        ctx->lv[i].hist = HistLevel();
        ctx->lv[i].remd = RemdLevel();
        ctx->lv[i].selfsim = SelfSimLevel();
        ctx->lv[i].xcorr = XcorrLevel();
    }
}
// weight i of a setter's six into the new block
int take_weight(nst_ctx* ctx, const MapTermWords& t, const float* weights, int i, MapTerm& g) {
    if (!(weights[i] >= 0.f) || std::isinf(weights[i]))
        return fail(ctx, NST_E_ARG, std::string("the ") + t.adj + " weights must be finite and >= 0");
    g.w[i] = weights[i];
    return NST_OK;
}
// A setter after its own argument checks: orders the stream and, when the new block g has a positive weight, refuses what
// every term refuses, then runs the style image through the network on scratch up to the deepest weighted map (sc: left
// open, the setter copies from its maps) and makes the zeroed vals.  No positive weight: sc stays empty.
int begin_map_term(nst_ctx* ctx, const MapTermWords& t, const LevelWs& L, MapTerm& g, const float* style, int hs, int ws, void* stream,
                   std::optional<Scratch>& sc) {
    hipStream_t s = enter(ctx, stream);
    if (!g.on()) return NST_OK;
    const std::string name = t.name, adj = t.adj;
    if (t.f16x2_only && ctx->conv_mode != 2) return fail(ctx, NST_E_STATE, "the " + name + " runs in the f16x2 arithmetic only (NST_CONV unset)");
    if (ctx->use_graph) return fail(ctx, NST_E_STATE, "the " + name + "'s launches are not captured: a context with use_graph takes no term");
    if (L.guide.R > 0) return fail(ctx, NST_E_STATE, "a guided level takes no " + name + " (nst_level_set_guidance(ctx, level, 0, ...) clears the guidance)");
    if (t.any_used_map ? (hs != L.h || ws != L.w) : (hs < 16 || ws < 16))
        return fail(ctx, NST_E_ARG, t.any_used_map ? "the content image must have the level's size" : "style image must be at least 16x16");
    unsigned used_mask = style_mask_of(ctx->taps);
    if (t.any_used_map) used_mask |= 1u << tap_index_of(ctx->taps.content);
    int deepest = -1;
    for (int i = 0; i < 6; ++i) {
        if (!(g.w[i] > 0.f)) continue;
        if (!((used_mask >> i) & 1u))
            return fail(ctx, NST_E_ARG, "a positive " + adj + " weight on a map that is not " + (t.any_used_map ? "a map the job uses" : "a style map of the job"));
        const int l = kTapLayer[i];
        if (t.min_3x3 && (L.acts.h[l] < 3 || L.acts.w[l] < 3 || (hs >> kScale[l]) < 3 || (ws >> kScale[l]) < 3))
            return fail(ctx, NST_E_ARG, "a weighted map or its style map is below 3x3");
        deepest = l;
    }
    sc.emplace(ctx, s);
    NSTCHK(alloc_acts(ctx, sc->acts, hs, ws));
    NSTCHK(forward(ctx, sc->acts, style, hs, ws, s, deepest, ctx->channels));
    NSTCHK(g.mem.alloc(ctx, &g.vals, 6));
    HIPCHK(ctx, hipMemsetAsync(g.vals, 0, 6 * sizeof(float), s));
    return NST_OK;
}
// A setter's end: the scratch goes (or, no positive weight, g is a cleared block), the context's work is waited for, what a
// closure remembered goes, and g becomes the level's block
template <typename Block>
int commit_map_term(nst_ctx* ctx, std::optional<Scratch>& sc, Block& slot, Block& g) {
    if (sc) NSTCHK(sc->finish());       // (synchronises: the caller's image is free again when this returns)
    else g = Block();
    quiesce(ctx);
    drop_closure_state(ctx, false);
    slot = std::move(g);
    return NST_OK;
}
// the unweighted values of term t of the last closure, levels x 6 by map index (zeros: levels without the term or outside the
// last level mask, maps without a weight, no closure yet)
int map_term_losses(nst_ctx* ctx, int t, float* out, void* stream) {
    NSTCHK(bind(ctx));
    if (ctx->levels < 1) return fail(ctx, NST_E_STATE, "nst_job_configure has not been called");
    if (!out) return fail(ctx, NST_E_ARG, "null argument");
    hipStream_t s = enter(ctx, stream);
    for (int i = 0; i < ctx->levels; ++i) {
        const MapTerm& g = ctx->lv[i].map_term(t);
        if (g.on()) HIPCHK(ctx, hipMemcpyAsync(out + 6 * i, g.vals, 6 * sizeof(float), hipMemcpyDeviceToDevice, s));
        else HIPCHK(ctx, hipMemsetAsync(out + 6 * i, 0, 6 * sizeof(float), s));
    }
    mark(ctx, s);
    return NST_OK;
}

}  // namespace

// ================================================================================================
extern "C" {

int nst_version(void) { return 200; }

const char* nst_last_error(const nst_ctx* ctx) { return ctx ? ctx->err.c_str() : g_err.c_str(); }

int nst_device_count(int* count) {
    if (!count) return fail(nullptr, NST_E_ARG, "count is null");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *count = 0; return fail(nullptr, NST_E_HIP, hipGetErrorString(e)); }
    *count = n;
    return NST_OK;
}

void nst_options_default(nst_options* o) {
    if (!o) return;
    o->struct_size = (int)sizeof(nst_options);
    o->conv_mode = -1; o->batched = -1; o->single_stream = -1; o->use_graph = -1; o->h2_band_rows = -1; o->lbfgs_gram = -1;
    o->h2_mfma16 = -1; o->h2_wg256 = -1; o->h2_tile_rows = -1; o->gram_overlap = -1; o->h2_persist = -1; o->level_split = -1; o->h2_winograd = -1;
}

int nst_ctx_create(int device, const float* const* weights, const float* const* biases, nst_ctx** out) {
    return nst_ctx_create_ex(device, weights, biases, nullptr, out);
}

int nst_ctx_create_ex(int device, const float* const* weights, const float* const* biases, const nst_options* opts_in,
                      nst_ctx** out) {
    if (!weights || !biases || !out) return fail(nullptr, NST_E_ARG, "null argument");
    nst_options opts;
    nst_options_default(&opts);
    if (opts_in) {
        if (opts_in->struct_size != (int)sizeof(nst_options)) return fail(nullptr, NST_E_ARG, "nst_options.struct_size mismatch (use nst_options_default)");
        opts = *opts_in;
    }
    for (int l = 0; l < NL; ++l)
        if (!weights[l] || !biases[l]) return fail(nullptr, NST_E_ARG, "null weight/bias pointer");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(nullptr, NST_E_HIP, "no HIP device visible");
    if (device < 0 || device >= ndev) return fail(nullptr, NST_E_ARG, "device index out of range");
    nst_ctx* ctx = new (std::nothrow) nst_ctx();
    if (!ctx) return fail(nullptr, NST_E_NOMEM, "out of host memory");
    ctx->device = device;
    auto bail = [&](int code) { g_err = ctx->err; nst_ctx_destroy(ctx); return code; };
    if (hipSetDevice(device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return bail(NST_E_HIP); }
    hipError_t e = conv_mfma_init_device();
    if (e == hipSuccess) e = conv_bf3_init_device();
    if (e == hipSuccess) e = conv_h2_init_device();
    if (e == hipSuccess) e = conv_wino_init_device();
    if (e == hipSuccess) e = gram_init_device();
    if (e == hipSuccess) e = pm_init_device();
    if (e == hipSuccess) e = hist_init_device();
    if (e == hipSuccess) e = remd_init_device();
    if (e == hipSuccess) e = selfsim_init_device();
    if (e == hipSuccess) e = xcorr_init_device();
    // options: an explicit argument wins; -1 falls back to the environment (read here, once), then to the default
    if (opts.conv_mode >= 0) {
        if (opts.conv_mode > NST_CONV_F16X2) { ctx->err = "nst_options.conv_mode must be NST_CONV_F32, NST_CONV_BF16X3 or NST_CONV_F16X2"; return bail(NST_E_ARG); }
        ctx->conv_mode = opts.conv_mode;
    } else {
        const char* cm = getenv("NST_CONV");
        if (cm && std::strcmp(cm, "f32") == 0) ctx->conv_mode = 0;
        else if (cm && std::strcmp(cm, "bf16x3") == 0) ctx->conv_mode = 1;
        else if (cm && std::strcmp(cm, "f16x2") == 0) ctx->conv_mode = 2;
        else if (cm && cm[0]) { ctx->err = "NST_CONV must be f32, bf16x3 or f16x2"; return bail(NST_E_ARG); }
    }
    ctx->batched = (opts.batched >= 0 ? opts.batched : env_flag("NST_BATCH", 1)) ? 1 : 0;
    ctx->use_graph = (opts.use_graph >= 0 ? opts.use_graph : env_flag("NST_GRAPH", 0)) ? 1 : 0;
    ctx->single_stream = (opts.single_stream >= 0 ? opts.single_stream : env_flag("NST_SINGLE_STREAM", 0)) != 0;
    ctx->band_rows = opts.h2_band_rows >= 0 ? opts.h2_band_rows : env_flag("NST_H2_BAND_ROWS", 0);
    ctx->lbfgs_gram = (opts.lbfgs_gram >= 0 ? opts.lbfgs_gram : env_flag("NST_LBFGS_GRAM", 1)) ? 1 : 0;
    ctx->mfma16 = opts.h2_mfma16 >= 0 ? opts.h2_mfma16 : env_flag("NST_H2_MFMA16", 1);
    ctx->wg256 = (opts.h2_wg256 >= 0 ? opts.h2_wg256 : env_flag("NST_H2_WG256", 0)) ? 1 : 0;
    ctx->tile_rows = opts.h2_tile_rows >= 0 ? opts.h2_tile_rows : env_flag("NST_H2_TILE_ROWS", 0);
    ctx->persist = (opts.h2_persist >= 0 ? opts.h2_persist : env_flag("NST_H2_PERSIST", 0)) ? 1 : 0;
    ctx->winograd = (opts.h2_winograd >= 0 ? opts.h2_winograd : env_flag("NST_H2_WINOGRAD", 1)) ? 1 : 0;
    ctx->level_split = (opts.level_split >= 0 ? opts.level_split : env_flag("NST_LEVEL_SPLIT", 0)) ? 1 : 0;
    ctx->gram_overlap = (opts.gram_overlap >= 0 ? opts.gram_overlap : env_flag("NST_GRAM_OVERLAP", 0)) ? 1 : 0;
    ctx->keep_all_maps = env_flag("NST_KEEP_ALL_MAPS", 0) ? 1 : 0;      // (nst_ctx_set_keep_all_maps overrides)
    ctx->forward_pack = env_flag("NST_FORWARD_PACK", 1) ? 1 : 0;        // (nst_ctx_set_forward_pack overrides)
    ctx->gram_pack = env_flag("NST_GRAM_PACK", 1) ? 1 : 0;              // (nst_ctx_set_gram_pack overrides)
    ctx->h2_direct_weights = env_flag("NST_H2_DIRECT_WEIGHTS", NST_H2_DIRECT_DEFAULT) & 3;      // (nst_ctx_set_h2_direct_weights overrides)
    if (ctx->use_graph && hipStreamCreateWithFlags(&ctx->gstream, hipStreamNonBlocking) != hipSuccess) { ctx->err = "stream creation failed"; return bail(NST_E_HIP); }
    if (e != hipSuccess) { ctx->err = std::string("kernel attribute setup: ") + hipGetErrorString(e); return bail(NST_E_HIP); }

    std::vector<float> tmp;
    std::vector<uint16_t> tmp16;
    auto upload = [&](auto& dst, const void* src, size_t bytes, const char* what) -> int {      // a device copy of host data
        if (ctx->mem.alloc_bytes(ctx, reinterpret_cast<void**>(&dst), bytes) != NST_OK) return NST_E_NOMEM;
        if (hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice) != hipSuccess) { ctx->err = std::string(what) + " upload failed"; return NST_E_HIP; }
        return NST_OK;
    };
    // tmp = [9][rows][K] cut into the 16-bit pieces of the active arithmetic only (a context is created per job: 0.24 s -
    // tools/time_ctx_create.py - and ~200 MB of weight images)
    std::vector<uint16_t> frag16;
    auto pieces = [&](int rows, int K, void*& bf, void*& h2, float& h2_inv, void*& wino, float& wino_inv, void** frag) -> int {
        if (ctx->conv_mode == 1) {
            make_bf3(tmp.data(), 9, rows, K, tmp16);
            return upload(bf, tmp16.data(), tmp16.size() * 2, "weight");
        }
        if (ctx->conv_mode != 2) return NST_OK;
        make_h2(tmp.data(), 9, rows, K, tmp16, &h2_inv);
        NSTCHK(upload(h2, tmp16.data(), tmp16.size() * 2, "weight"));
        // (a forward layer on 16-channel chunks: the same pieces once more in fragment order, for its DIRECT launches)
        if (frag && h2_chunk(rows, K) == 16 && rows % 64 == 0 && K % 16 == 0) {
            make_h2_frag(tmp16, rows, K, frag16);
            NSTCHK(upload(*frag, frag16.data(), frag16.size() * 2, "weight"));
        }
        if (ctx->winograd && K >= 256 && K % 64 == 0 && rows % 128 == 0) {      // (K = 128: no gain measured)
            make_wino(tmp.data(), rows, K, tmp16, &wino_inv);
            NSTCHK(upload(wino, tmp16.data(), tmp16.size() * 2, "weight"));
        }
        return NST_OK;
    };
    for (int l = 0; l < NL; ++l) {
        const int ci = kCin[l], co = kCout[l];
        const float* W = weights[l];   // [co][ci][3][3]
        if (int r = upload(ctx->bias[l], biases[l], co * 4, "bias")) return bail(r);
        if (l == 0) {
            tmp.assign(28 * 64, 0.f);
            for (int o = 0; o < 64; ++o)
                for (int c = 0; c < 3; ++c)
                    for (int t = 0; t < 9; ++t) tmp[(c * 9 + t) * 64 + o] = W[(o * 3 + c) * 9 + t];
            if (int r = upload(ctx->w11k, tmp.data(), tmp.size() * 4, "weight")) return bail(r);
            tmp.assign(9 * 64 * 4, 0.f);
            for (int t = 0; t < 9; ++t) {
                const int ky = 2 - t / 3, kx = 2 - t % 3;
                for (int o = 0; o < 64; ++o)
                    for (int c = 0; c < 3; ++c) tmp[(t * 64 + o) * 4 + c] = W[(o * 3 + c) * 9 + ky * 3 + kx];
            }
            if (int r = upload(ctx->w11d, tmp.data(), tmp.size() * 4, "weight")) return bail(r);
            continue;
        }
        const size_t n = (size_t)9 * ci * co;
        tmp.resize(n);
        // forward: wf[tap][co][ci]
        for (int t = 0; t < 9; ++t)
            for (int o = 0; o < co; ++o)
                for (int c = 0; c < ci; ++c) tmp[((size_t)t * co + o) * ci + c] = W[((size_t)o * ci + c) * 9 + t];
        if (int r = upload(ctx->wf[l], tmp.data(), n * 4, "weight")) return bail(r);
        if (int r = pieces(co, ci, ctx->wf_bf[l], ctx->wf_h2[l], ctx->wf_h2_inv[l], ctx->wf_wino[l], ctx->wf_wino_inv[l], &ctx->wf_h2_frag[l])) return bail(r);
        // input gradient: a conv with "Cout" = ci and "Cin" = co: wd[tap'][ci][co] = W[co][ci][2-ky'][2-kx']
        for (int t = 0; t < 9; ++t) {
            const int ky = 2 - t / 3, kx = 2 - t % 3;
            for (int c = 0; c < ci; ++c)
                for (int o = 0; o < co; ++o) tmp[((size_t)t * ci + c) * co + o] = W[((size_t)o * ci + c) * 9 + ky * 3 + kx];
        }
        if (int r = upload(ctx->wd[l], tmp.data(), n * 4, "weight")) return bail(r);
        if (int r = pieces(ci, co, ctx->wd_bf[l], ctx->wd_h2[l], ctx->wd_h2_inv[l], ctx->wd_wino[l], ctx->wd_wino_inv[l], nullptr)) return bail(r);
    }
    if (ctx->level_split) ctx->gram_overlap = 0;      // (one side stream: the two experiments exclude each other)
    if ((ctx->gram_overlap || ctx->level_split) && ctx->conv_mode == 2 &&
        (hipStreamCreateWithFlags(&ctx->side, hipStreamNonBlocking) != hipSuccess ||
         hipEventCreateWithFlags(&ctx->side_fork, hipEventDisableTiming) != hipSuccess ||
         hipEventCreateWithFlags(&ctx->side_join, hipEventDisableTiming) != hipSuccess)) {
        ctx->err = "side stream creation failed";
        return bail(NST_E_HIP);
    }
    if (hipEventCreateWithFlags(&ctx->fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->tail, hipEventDisableTiming) != hipSuccess ||
        hipEventCreate(&ctx->t0) != hipSuccess || hipEventCreate(&ctx->t1) != hipSuccess) {
        ctx->err = "event creation failed";
        return bail(NST_E_HIP);
    }
    *out = ctx;
    return NST_OK;
}

void nst_ctx_destroy(nst_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    quiesce(ctx);
    for (int i = 0; i < NST_MAX_LEVELS; ++i) free_level(ctx->lv[i]);
    if (ctx->tail) (void)hipEventDestroy(ctx->tail);
    ctx->mem.release();
    drop_closure_state(ctx, false);
    if (ctx->gstream) (void)hipStreamDestroy(ctx->gstream);
    if (ctx->side) (void)hipStreamDestroy(ctx->side);
    if (ctx->side_fork) (void)hipEventDestroy(ctx->side_fork);
    if (ctx->side_join) (void)hipEventDestroy(ctx->side_join);
    if (ctx->fork) (void)hipEventDestroy(ctx->fork);
    if (ctx->t0) (void)hipEventDestroy(ctx->t0);
    if (ctx->t1) (void)hipEventDestroy(ctx->t1);
    for (hipEvent_t e : ctx->ev_pool) (void)hipEventDestroy(e);
    delete ctx;
}

int nst_conv_mode(const nst_ctx* ctx) { return ctx ? ctx->conv_mode : -1; }

int nst_ctx_bytes(const nst_ctx* ctx, size_t* bytes) {
    if (!ctx || !bytes) return fail(nullptr, NST_E_ARG, "null argument");
    *bytes = ctx->bytes;
    return NST_OK;
}

int nst_job_configure(nst_ctx* ctx, int levels_num, int H0, int W0) {
    if (ctx) { ++ctx->closure_epoch; ++ctx->ws_seq; }
    NSTCHK(bind(ctx));
    if (levels_num < 1 || levels_num > NST_MAX_LEVELS) return fail(ctx, NST_E_ARG, "levels_num out of range");
    if ((H0 >> (levels_num - 1)) < 16 || (W0 >> (levels_num - 1)) < 16)
        return fail(ctx, NST_E_ARG, "coarsest pyramid level must be at least 16x16");
    quiesce(ctx);
    for (int i = 0; i < NST_MAX_LEVELS; ++i) free_level(ctx->lv[i]);      // (the targets go with the levels)
    drop_closure_state(ctx, false);
    forget_forward_pass(ctx);
    ctx->levels = 0;
    ctx->lap_k = 0;                      // (the Laplacian setting belongs to the job's geometry: its buffers went with the levels)
    ctx->mat_gamma = 0.f; ctx->mat_eps = 1e-7;   // (the matting term likewise)
    for (float& v : ctx->gs_shift) v = 0.f;      // (the Gram shift likewise)
    ctx->gs_center = 0u;
    for (int i = 0; i < 6; ++i) { ctx->mom_wm[i] = 0.f; ctx->mom_ws[i] = 0.f; }      // (the moment term likewise)
    ctx->mom_eps = 1e-5f;
    int h = H0, w = W0;
    for (int i = 0; i < levels_num; ++i) {
        LevelWs& L = ctx->lv[i];
        L.h = h; L.w = w;
        NSTCHK(alloc_acts(ctx, L.acts, h, w));
        L.gbuf_floats = (size_t)h * w * 64;
        NSTCHK(L.mem.alloc(ctx, &L.gbuf[0], L.gbuf_floats));
        NSTCHK(L.mem.alloc(ctx, &L.gbuf[1], L.gbuf_floats));
        if (i > 0) NSTCHK(alloc_level_image(ctx, L.img, ctx->channels, h, w));
        NSTCHK(alloc_tap_buffers(ctx, L));       // sized for the context's current taps
        NSTCHK(L.mem.alloc(ctx, &L.content_partial, MSE_BLOCKS));
        NSTCHK(L.mem.alloc(ctx, &L.tv_partial, 2 * TV_BLOCKS));
        NSTCHK(L.mem.alloc(ctx, &L.tv_means, 2));
        h /= 2; w /= 2;
    }
    ctx->levels = levels_num;
    return NST_OK;
}

// LossBuilder(content_feature_maps_index, style_feature_maps_indices, ...) and Vgg19(use_relu=...) of the reference
// (neural_style_transfer.py:41-82, neural_nets.py:17-28) as a context setting
int nst_job_set_taps(nst_ctx* ctx, int content_index, unsigned style_mask, int use_relu) {
    if (ctx) { ++ctx->closure_epoch; ++ctx->ws_seq; }
    NSTCHK(bind(ctx));
    if (content_index < 0 || content_index > 5) return fail(ctx, NST_E_ARG, "content_index must be 0 .. 5");
    if (style_mask == 0u || (style_mask & ~0x3Fu) != 0u)
        return fail(ctx, NST_E_ARG, "style_mask must be a non-empty set of bits 0 .. 5");
    if (use_relu != 0 && use_relu != 1) return fail(ctx, NST_E_ARG, "use_relu must be 0 or 1");
    Taps tp;
    tp.content = kTapLayer[content_index];
    tp.nstyle = 0;
    for (int i = 0; i < 6; ++i)
        if ((style_mask >> i) & 1u) tp.style[tp.nstyle++] = kTapLayer[i];      // (ascending: kTapLayer increases)
    tp.top = std::max(tp.content, tp.style[tp.nstyle - 1]);
    tp.use_relu = use_relu;
    tp.is_default = content_index == 4 && style_mask == 0x2Fu && use_relu == 1;
    // the style layer weights stay as they are (they belong to map indices): the new set needs a map that counts
    if ((style_mask & positive_weight_mask(ctx->style_w)) == 0u)
        return fail(ctx, NST_E_ARG, "no map of style_mask has a positive style layer weight (nst_job_set_style_weights)");
    // every level's targets and the captured closure belong to the old taps; the tap-sized buffers are re-allocated
    quiesce(ctx);
    drop_closure_state(ctx, true);
    ctx->taps = tp;
    drop_map_terms(ctx);                    // (the style's maps of the old taps)
    for (int i = 0; i < ctx->levels; ++i) {
        LevelWs& L = ctx->lv[i];
        L.guide = Guidance();           // (sized for the old style set: nst_level_set_guidance again)
        free_tap_buffers(L);
        NSTCHK(alloc_tap_buffers(ctx, L));
    }
    return NST_OK;
}

// Gatys et al. 2016, luminance-only transfer: the optimised image becomes one plane u = 255 Y (channels = 1) that the
// network sees as x_c = u - mean_c.  Same life cycle as the taps: every level's targets and the captured closure go.
int nst_job_set_color(nst_ctx* ctx, int mode) {
    if (ctx) { ++ctx->closure_epoch; ++ctx->ws_seq; }
    NSTCHK(bind(ctx));
    if (mode != NST_COLOR_RGB && mode != NST_COLOR_LUMINANCE) return fail(ctx, NST_E_ARG, "mode must be NST_COLOR_RGB or NST_COLOR_LUMINANCE");
    const int channels = mode == NST_COLOR_LUMINANCE ? 1 : 3;
    quiesce(ctx);
    // the level images of the new channel count first: if one cannot be had, the context stays as it was (old mode, old
    // buffers, targets kept)
    LevelWs* lv = ctx->lv + 1;
    NSTCHK(replace_blocks(lv, ctx->levels - 1, &LevelWs::img,
                          [&](int i, LevelImage& im) { return alloc_level_image(ctx, im, channels, lv[i].h, lv[i].w); },
                          [&] { drop_closure_state(ctx, true); }));
    // an anchor has the planes of the mode it was set under (nst_level_set_anchor): another mode drops it
    for (int i = 0; i < ctx->levels && channels != ctx->channels; ++i) ctx->lv[i].anc = AnchorLevel();
    drop_map_terms(ctx);                    // (maps of the style image as the other mode's network saw it)
    ctx->channels = channels;
    return NST_OK;
}

int nst_job_color(const nst_ctx* ctx) { return ctx ? (ctx->channels == 1 ? NST_COLOR_LUMINANCE : NST_COLOR_RGB) : -1; }

// Gatys et al. 2016, section 2: average instead of max pooling in the feature network.  Same life cycle as the taps and the
// colour mode: every level's targets (made with the other network) and the captured closure go; no buffer changes size.
int nst_job_set_pooling(nst_ctx* ctx, int mode) {
    if (ctx) { ++ctx->closure_epoch; ++ctx->ws_seq; }
    NSTCHK(bind(ctx));
    if (mode != NST_POOL_MAX && mode != NST_POOL_AVG) return fail(ctx, NST_E_ARG, "mode must be NST_POOL_MAX or NST_POOL_AVG");
    quiesce(ctx);
    drop_closure_state(ctx, true);
    drop_map_terms(ctx);                    // (their style maps are the other network's)
    ctx->pool_avg = mode == NST_POOL_AVG ? 1 : 0;
    return NST_OK;
}

// The A/B twin of the unread-map elision in one build: 1 = every batched forward launch stores its full-resolution map.
// Results do not depend on it; a captured graph holds the launches of the setting it was captured under and goes.
int nst_ctx_set_keep_all_maps(nst_ctx* ctx, int enabled) {
    NSTCHK(bind(ctx));
    ++ctx->ws_seq;
    drop_closure_state(ctx, false);
    ctx->keep_all_maps = enabled ? 1 : 0;
    return NST_OK;
}
int nst_ctx_keep_all_maps(const nst_ctx* ctx) { return ctx ? ctx->keep_all_maps : -1; }

// The A/B twin of the packed forward half in one build: 0 = the per-level front and loss-term launches, and S also in bf16
// pieces.  Results do not depend on it; a captured graph never holds the packed launches.
int nst_ctx_set_forward_pack(nst_ctx* ctx, int enabled) {
    NSTCHK(bind(ctx));
    ++ctx->ws_seq;
    drop_closure_state(ctx, false);
    ctx->forward_pack = enabled ? 1 : 0;
    return NST_OK;
}
int nst_ctx_forward_pack(const nst_ctx* ctx) { return ctx ? ctx->forward_pack : -1; }

// The A/B twin of the packed Gram pass in one build: 0 = every block of a diagonal tile is computed and written, and a plain
// batch launches once per tile shape.  Results do not depend on it (gram.hip: a kept block sees the same MFMAs in the same
// order, and nothing reads the dropped ones).
int nst_ctx_set_gram_pack(nst_ctx* ctx, int enabled) {
    NSTCHK(bind(ctx));
    ++ctx->ws_seq;
    drop_closure_state(ctx, false);
    ctx->gram_pack = enabled ? 1 : 0;
    return NST_OK;
}
int nst_ctx_gram_pack(const nst_ctx* ctx) { return ctx ? ctx->gram_pack : -1; }

// The A/B twin of the DIRECT K loop in one build: 0 = the forward launches of the 16-channel-chunk conv_h2 shapes stage
// their weight slices through LDS as before.  Results do not depend on it (conv_h2.hip: every accumulator sees the same
// MFMAs on the same operands in the same order); a captured graph holds the kernels of the setting it was captured under.
int nst_ctx_set_h2_direct_weights(nst_ctx* ctx, int enabled) {
    NSTCHK(bind(ctx));
    ++ctx->ws_seq;
    drop_closure_state(ctx, false);
    if (enabled < 0 || enabled > 3) return fail(ctx, NST_E_ARG, "h2_direct_weights must be 0 .. 3");
    ctx->h2_direct_weights = enabled;
    return NST_OK;
}
int nst_ctx_h2_direct_weights(const nst_ctx* ctx) { return ctx ? ctx->h2_direct_weights : -1; }
long long nst_ctx_h2_direct_launches(const nst_ctx* ctx) { return ctx ? (long long)ctx->h2_direct_launches : -1; }

int nst_job_map_stats(nst_ctx* ctx, int level, unsigned* stored_mask) {
    NSTCHK(bind(ctx));
    if (level < 0 || level >= ctx->levels) return fail(ctx, NST_E_STATE, "level not configured");
    if (!stored_mask) return fail(ctx, NST_E_ARG, "null argument");
    unsigned m = 0;
    for (int l = 0; l < NL; ++l) m |= (ctx->lv[level].acts.stored[l] ? 1u : 0u) << l;
    *stored_mask = m;
    return NST_OK;
}

int nst_job_pooling(const nst_ctx* ctx) { return ctx ? (ctx->pool_avg ? NST_POOL_AVG : NST_POOL_MAX) : -1; }

// The Laplacian loss (Li et al. 2017; include/nst_hip.h has the definition): up to NST_MAX_LAPLACIAN entries (pool size,
// weight).  Same life cycle as the pooling: every level's targets go (the Laplacian targets D s_k(content) are made with
// them), and the captured closure.  Every buffer of the term is allocated here; a refusal changes nothing.
int nst_job_set_laplacian(nst_ctx* ctx, int K, const int* pool, const float* gamma) {
    if (ctx) { ++ctx->closure_epoch; ++ctx->ws_seq; }
    NSTCHK(bind(ctx));
    if (ctx->levels < 1) return fail(ctx, NST_E_STATE, "nst_job_configure has not been called");
    if (K < 0 || K > NST_MAX_LAPLACIAN) return fail(ctx, NST_E_ARG, "the number of Laplacian entries must be 0 .. NST_MAX_LAPLACIAN");
    if (K > 0 && (!pool || !gamma)) return fail(ctx, NST_E_ARG, "null argument");
    bool positive = false;
    for (int k = 0; k < K; ++k) {
        if (pool[k] < 1 || pool[k] > 32) return fail(ctx, NST_E_ARG, "a Laplacian pool size must be 1 .. 32");
        for (int j = 0; j < k; ++j)
            if (pool[j] == pool[k]) return fail(ctx, NST_E_ARG, "the Laplacian entries must have distinct pool sizes");
        if (!(gamma[k] >= 0.f) || std::isinf(gamma[k])) return fail(ctx, NST_E_ARG, "Laplacian weights must be finite and >= 0");
        positive = positive || gamma[k] > 0.f;
        for (int i = 0; i < ctx->levels; ++i)
            if (ctx->lv[i].h / pool[k] < 3 || ctx->lv[i].w / pool[k] < 3)
                return fail(ctx, NST_E_ARG, "level " + std::to_string(i) + " is too small for Laplacian pool size " + std::to_string(pool[k]) +
                                            ": the pooled image must be at least 3x3");
    }
    if (K > 0 && !positive) return fail(ctx, NST_E_ARG, "at least one Laplacian weight must be positive");
    NSTCHK(replace_term(ctx, &LevelWs::lap, [&](int i, LapLevel& q) {
        if (K > 0 && i == 0) NSTCHK(q.mem.alloc(ctx, &q.vals, (size_t)NST_MAX_LEVELS * NST_LAP_MAX));
        for (int k = 0; k < K; ++k) {
            const size_t hk = (size_t)(ctx->lv[i].h / pool[k]), wk = (size_t)(ctx->lv[i].w / pool[k]);
            NSTCHK(q.mem.alloc(ctx, &q.s[k], hk * wk));
            NSTCHK(q.mem.alloc(ctx, &q.r[k], (hk - 2) * (wk - 2)));
            NSTCHK(q.mem.alloc(ctx, &q.target[k], (hk - 2) * (wk - 2)));
            NSTCHK(q.mem.alloc(ctx, &q.partial[k], LAP_BLOCKS));
        }
        return NST_OK;
    }));
    ctx->lap_k = K;
    for (int k = 0; k < NST_LAP_MAX; ++k) {
        ctx->lap_pool[k] = k < K ? pool[k] : 0;
        ctx->lap_gamma[k] = k < K ? gamma[k] : 0.f;
    }
    if (K > 0) HIPCHK(ctx, hipMemset(ctx->lv[0].lap.vals, 0, (size_t)NST_MAX_LEVELS * NST_LAP_MAX * sizeof(float)));
    return NST_OK;
}

int nst_job_laplacian(const nst_ctx* ctx, int* K, int* pool, float* gamma) {
    if (!ctx) return fail(nullptr, NST_E_ARG, "null context");
    if (K) *K = ctx->lap_k;
    for (int k = 0; k < NST_LAP_MAX; ++k) {
        if (pool) pool[k] = ctx->lap_pool[k];
        if (gamma) gamma[k] = ctx->lap_gamma[k];
    }
    return NST_OK;
}

// the unweighted lap_k of the last closure, levels x NST_MAX_LAPLACIAN, as the loss rows left them (zeros: levels outside
// the last level mask, unused entries, no closure yet, term off)
int nst_job_laplacian_losses(nst_ctx* ctx, float* out, void* stream) {
    NSTCHK(bind(ctx));
    if (ctx->levels < 1) return fail(ctx, NST_E_STATE, "nst_job_configure has not been called");
    if (!out) return fail(ctx, NST_E_ARG, "null argument");
    hipStream_t s = enter(ctx, stream);
    const size_t bytes = (size_t)ctx->levels * NST_LAP_MAX * sizeof(float);
    if (ctx->lap_k > 0) HIPCHK(ctx, hipMemcpyAsync(out, ctx->lv[0].lap.vals, bytes, hipMemcpyDeviceToDevice, s));
    else HIPCHK(ctx, hipMemsetAsync(out, 0, bytes, s));
    mark(ctx, s);
    return NST_OK;
}

// The matting-Laplacian regulariser (Luan et al. 2017; include/nst_hip.h has the definition): a weight and epsilon.  The
// life cycle of nst_job_set_laplacian: every level's targets go (the guide, a copy of the level's content, is made with
// them), and the captured closure.  Every buffer of the term is allocated here; a refusal changes nothing.
int nst_job_set_matting(nst_ctx* ctx, float gamma, double epsilon) {
    if (ctx) { ++ctx->closure_epoch; ++ctx->ws_seq; }
    NSTCHK(bind(ctx));
    if (ctx->levels < 1) return fail(ctx, NST_E_STATE, "nst_job_configure has not been called");
    if (!(gamma >= 0.f) || std::isinf(gamma)) return fail(ctx, NST_E_ARG, "the matting weight must be finite and >= 0");
    if (!(epsilon > 0.0) || std::isinf(epsilon)) return fail(ctx, NST_E_ARG, "the matting epsilon must be finite and > 0");
    const bool on = gamma > 0.f;
    NSTCHK(replace_term(ctx, &LevelWs::mat, [&](int i, MatLevel& q) {
        if (!on) return NST_OK;
        if (i == 0) NSTCHK(q.mem.alloc(ctx, &q.vals, (size_t)NST_MAX_LEVELS));
        const size_t px = (size_t)ctx->lv[i].h * ctx->lv[i].w;
        q.tiles = mat_tiles(ctx->lv[i].h, ctx->lv[i].w);
        NSTCHK(q.mem.alloc(ctx, &q.guide, 3 * px));             // (three planes: a colour mode set later fits)
        NSTCHK(q.mem.alloc(ctx, &q.partial, (size_t)q.tiles));
        return NST_OK;
    }));
    ctx->mat_gamma = gamma;
    ctx->mat_eps = epsilon;
    if (on) HIPCHK(ctx, hipMemset(ctx->lv[0].mat.vals, 0, (size_t)NST_MAX_LEVELS * sizeof(float)));
    return NST_OK;
}

int nst_job_matting(const nst_ctx* ctx, float* gamma, double* epsilon) {
    if (!ctx) return fail(nullptr, NST_E_ARG, "null context");
    if (gamma) *gamma = ctx->mat_gamma;
    if (epsilon) *epsilon = ctx->mat_eps;
    return NST_OK;
}

// the unweighted mat of the last closure per level, as the loss rows left it (zeros: levels outside the last level mask, no
// closure yet, term off)
int nst_job_matting_losses(nst_ctx* ctx, float* out, void* stream) {
    NSTCHK(bind(ctx));
    if (ctx->levels < 1) return fail(ctx, NST_E_STATE, "nst_job_configure has not been called");
    if (!out) return fail(ctx, NST_E_ARG, "null argument");
    hipStream_t s = enter(ctx, stream);
    const size_t bytes = (size_t)ctx->levels * sizeof(float);
    if (ctx->mat_gamma > 0.f) HIPCHK(ctx, hipMemcpyAsync(out, ctx->lv[0].mat.vals, bytes, hipMemcpyDeviceToDevice, s));
    else HIPCHK(ctx, hipMemsetAsync(out, 0, bytes, s));
    mark(ctx, s);
    return NST_OK;
}

// Activation-shifted and mean-centred Gram matrices (Novak & Nikulin 2016; Li et al. 2017; include/nst_hip.h has the
// definition).  Same life cycle as the pooling: every level's targets go (they are made with the statistic), and the captured
// closure.  Every buffer of the option is allocated here; a refusal changes nothing.
int nst_job_set_gram_shift(nst_ctx* ctx, const float* shift, unsigned center_mask) {
    if (ctx) { ++ctx->closure_epoch; ++ctx->ws_seq; }
    NSTCHK(bind(ctx));
    if (!shift) return fail(ctx, NST_E_ARG, "null argument");
    if ((center_mask & ~0x3Fu) != 0u) return fail(ctx, NST_E_ARG, "center_mask must be a set of bits 0 .. 5");
    bool on = center_mask != 0u;
    for (int i = 0; i < 6; ++i) {
        if (!std::isfinite(shift[i])) return fail(ctx, NST_E_ARG, "Gram shifts must be finite");
        if (((center_mask >> i) & 1u) && shift[i] != 0.f) return fail(ctx, NST_E_ARG, "a centred map takes no constant shift: its entry must be 0");
        on = on || shift[i] != 0.f;
    }
    if (on) {
        if (ctx->levels < 1) return fail(ctx, NST_E_STATE, "nst_job_configure has not been called");
        if (ctx->conv_mode != 2) return fail(ctx, NST_E_STATE, "the shifted Gram runs in the f16x2 arithmetic only (NST_CONV unset)");
        for (int i = 0; i < ctx->levels; ++i)
            if (ctx->lv[i].guide.R > 0)
                return fail(ctx, NST_E_STATE, "guided Gram matrices take the plain statistic only (nst_level_set_guidance(ctx, level, 0, ...) clears the guidance)");
    }
    NSTCHK(replace_term(ctx, &LevelWs::gs, [&](int, GramShiftLevel& q) {
        if (!on) return NST_OK;
        NSTCHK(q.mem.alloc(ctx, &q.words, (size_t)kMaxStyle * GS_STRIDE));
        if (center_mask) NSTCHK(q.mem.alloc(ctx, &q.sums, (size_t)kMaxStyle * GS_PART_DOUBLES));
        // (o reads as zeros until a closure has run: nst_level_gram_offsets)
        if (hipMemset(q.words, 0, (size_t)kMaxStyle * GS_STRIDE * sizeof(float)) != hipSuccess)
            return fail(ctx, NST_E_HIP, "hipMemset of the Gram offsets failed");
        return NST_OK;
    }));
    for (int i = 0; i < 6; ++i) ctx->gs_shift[i] = shift[i];
    ctx->gs_center = center_mask;
    return NST_OK;
}

int nst_job_gram_shift(const nst_ctx* ctx, float* shift, unsigned* center_mask) {
    if (!ctx) return fail(nullptr, NST_E_ARG, "null context");
    for (int i = 0; i < 6 && shift; ++i) shift[i] = ctx->gs_shift[i];
    if (center_mask) *center_mask = ctx->gs_center;
    return NST_OK;
}

// the o of style slot `slot` as the level's last closure (or targets-free forward half) left it: C floats
int nst_level_gram_offsets(nst_ctx* ctx, int level, int slot, float* out, void* stream) {
    NSTCHK(bind(ctx));
    if (level < 0 || level >= ctx->levels) return fail(ctx, NST_E_STATE, "level not configured");
    if (!ctx->gs_on()) return fail(ctx, NST_E_STATE, "no Gram shift is set (nst_job_set_gram_shift)");
    if (slot < 0 || slot >= ctx->taps.nstyle || !out) return fail(ctx, NST_E_ARG, "slot must be a style slot of the current taps and out not null");
    hipStream_t s = enter(ctx, stream);
    HIPCHK(ctx, hipMemcpyAsync(out, ctx->lv[level].gs.offset(slot), (size_t)kCout[ctx->taps.style[slot]] * sizeof(float), hipMemcpyDeviceToDevice, s));
    mark(ctx, s);
    return NST_OK;
}

// The moment loss (Li et al. 2017; Huang & Belongie 2017; include/nst_hip.h has the definition): per map the weights of its
// mean and deviation terms, and epsilon.  The life cycle of nst_job_set_gram_shift: every level's targets go (mu^t and
// sigma^t are made with them), and the captured closure.  Every buffer of the term is allocated here; a refusal changes
// nothing.
int nst_job_set_moments(nst_ctx* ctx, const float* mean_w, const float* std_w, float epsilon) {
    if (ctx) { ++ctx->closure_epoch; ++ctx->ws_seq; }
    NSTCHK(bind(ctx));
    if (!mean_w || !std_w) return fail(ctx, NST_E_ARG, "null argument");
    if (!(epsilon > 0.f) || std::isinf(epsilon)) return fail(ctx, NST_E_ARG, "the moment epsilon must be finite and > 0");
    bool on = false;
    for (int i = 0; i < 6; ++i) {
        if (!(mean_w[i] >= 0.f) || std::isinf(mean_w[i]) || !(std_w[i] >= 0.f) || std::isinf(std_w[i]))
            return fail(ctx, NST_E_ARG, "moment weights must be finite and >= 0");
        on = on || mean_w[i] > 0.f || std_w[i] > 0.f;
    }
    if (on) {
        if (ctx->levels < 1) return fail(ctx, NST_E_STATE, "nst_job_configure has not been called");
        if (ctx->conv_mode != 2) return fail(ctx, NST_E_STATE, "the moment loss runs in the f16x2 arithmetic only (NST_CONV unset)");
        for (int i = 0; i < ctx->levels; ++i)
            if (ctx->lv[i].guide.R > 0)
                return fail(ctx, NST_E_STATE, "guided levels take no moment loss (nst_level_set_guidance(ctx, level, 0, ...) clears the guidance)");
        const unsigned taps_mask = style_mask_of(ctx->taps);
        for (int i = 0; i < 6; ++i)
            if ((mean_w[i] > 0.f || std_w[i] > 0.f) && !((taps_mask >> i) & 1u))
                return fail(ctx, NST_E_ARG, "a moment weight is positive on map " + std::to_string(i) + ", which is not a style map of the job (nst_job_set_taps)");
    }
    NSTCHK(replace_term(ctx, &LevelWs::mom, [&](int i, MomentLevel& q) {
        if (!on) return NST_OK;
        if (i == 0) NSTCHK(q.mem.alloc(ctx, &q.vals, (size_t)NST_MAX_LEVELS * 12));
        NSTCHK(q.mem.alloc(ctx, &q.words, (size_t)kMaxStyle * MOM_STRIDE));
        NSTCHK(q.mem.alloc(ctx, &q.stats, (size_t)kMaxStyle * MOM_STAT_STRIDE));
        NSTCHK(q.mem.alloc(ctx, &q.sums, (size_t)kMaxStyle * MOM_PART_DOUBLES));
        if (hipMemset(q.words, 0, (size_t)kMaxStyle * MOM_STRIDE * sizeof(float)) != hipSuccess ||
            hipMemset(q.stats, 0, (size_t)kMaxStyle * MOM_STAT_STRIDE * sizeof(double)) != hipSuccess)
            return fail(ctx, NST_E_HIP, "hipMemset of the moment buffers failed");
        return NST_OK;
    }));
    for (int i = 0; i < 6; ++i) { ctx->mom_wm[i] = mean_w[i]; ctx->mom_ws[i] = std_w[i]; }
    ctx->mom_eps = epsilon;
    if (on) HIPCHK(ctx, hipMemset(ctx->lv[0].mom.vals, 0, (size_t)NST_MAX_LEVELS * 12 * sizeof(float)));
    return NST_OK;
}

int nst_job_moments(const nst_ctx* ctx, float* mean_w, float* std_w, float* epsilon) {
    if (!ctx) return fail(nullptr, NST_E_ARG, "null context");
    for (int i = 0; i < 6; ++i) {
        if (mean_w) mean_w[i] = ctx->mom_wm[i];
        if (std_w) std_w[i] = ctx->mom_ws[i];
    }
    if (epsilon) *epsilon = ctx->mom_eps;
    return NST_OK;
}

// the unweighted (mean_i, std_i) of the last closure, levels x 6 x 2 by map index, as the loss rows left them (zeros: levels
// outside the last level mask, maps without the term, no closure yet, term off)
int nst_job_moment_losses(nst_ctx* ctx, float* out, void* stream) {
    NSTCHK(bind(ctx));
    if (ctx->levels < 1) return fail(ctx, NST_E_STATE, "nst_job_configure has not been called");
    if (!out) return fail(ctx, NST_E_ARG, "null argument");
    hipStream_t s = enter(ctx, stream);
    const size_t bytes = (size_t)ctx->levels * 12 * sizeof(float);
    if (ctx->mom_on()) HIPCHK(ctx, hipMemcpyAsync(out, ctx->lv[0].mom.vals, bytes, hipMemcpyDeviceToDevice, s));
    else HIPCHK(ctx, hipMemsetAsync(out, 0, bytes, s));
    mark(ctx, s);
    return NST_OK;
}

// The temporal consistency term of one level (Ruder et al. 2016; include/nst_hip.h has the definition): the anchor, its weight
// plane and the weight.  Data of one job with the life cycle of nst_level_set_guidance: the copies are made here, beside what
// the level has (a refusal changes nothing), the context's work is waited for before the level's block is replaced, and the
// captured closure, an optimiser's remembered closure and a pending backward half go.  The targets stay: they do not depend
// on it.  nst_job_configure drops it with the levels.
int nst_level_set_anchor(nst_ctx* ctx, int level, const float* anchor, const float* weights, float gamma, void* stream) {
    if (ctx) { ++ctx->closure_epoch; ++ctx->ws_seq; }
    NSTCHK(bind(ctx));
    if (ctx->levels < 1) return fail(ctx, NST_E_STATE, "nst_job_configure has not been called");
    if (level < 0 || level >= ctx->levels) return fail(ctx, NST_E_ARG, "level out of range");
    if (!(gamma >= 0.f) || std::isinf(gamma)) return fail(ctx, NST_E_ARG, "the temporal weight must be finite and >= 0");
    LevelWs& L = ctx->lv[level];
    AnchorLevel g;
    hipStream_t s = enter(ctx, stream);
    if (anchor && gamma > 0.f) {
        const size_t px = (size_t)L.h * L.w;
        g.gamma = gamma;
        NSTCHK(g.mem.alloc(ctx, &g.anchor, (size_t)ctx->channels * px));
        if (weights) NSTCHK(g.mem.alloc(ctx, &g.weights, px));
        NSTCHK(g.mem.alloc(ctx, &g.partial, (size_t)ANCHOR_BLOCKS));
        NSTCHK(g.mem.alloc(ctx, &g.val, 1));
        hipError_t e = hipMemcpyAsync(g.anchor, anchor, (size_t)ctx->channels * px * sizeof(float), hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess && weights) e = hipMemcpyAsync(g.weights, weights, px * sizeof(float), hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipMemsetAsync(g.val, 0, sizeof(float), s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);       // (the caller's buffers are free again when this returns)
        HIPCHK(ctx, e);
    }
    quiesce(ctx);
    drop_closure_state(ctx, false);
    L.anc = std::move(g);
    return NST_OK;
}

// the unweighted tmp of the last closure per level, as the loss rows left it (zeros: levels without an anchor or outside the
// last level mask, no closure yet)
int nst_job_temporal_losses(nst_ctx* ctx, float* out, void* stream) {
    NSTCHK(bind(ctx));
    if (ctx->levels < 1) return fail(ctx, NST_E_STATE, "nst_job_configure has not been called");
    if (!out) return fail(ctx, NST_E_ARG, "null argument");
    hipStream_t s = enter(ctx, stream);
    for (int i = 0; i < ctx->levels; ++i) {
        const AnchorLevel& a = ctx->lv[i].anc;
        if (a.gamma > 0.f) HIPCHK(ctx, hipMemcpyAsync(out + i, a.val, sizeof(float), hipMemcpyDeviceToDevice, s));
        else HIPCHK(ctx, hipMemsetAsync(out + i, 0, sizeof(float), s));
    }
    mark(ctx, s);
    return NST_OK;
}

int nst_level_anchor(const nst_ctx* ctx, int level, float* gamma, int* weighted) {
    if (!ctx) return fail(nullptr, NST_E_ARG, "null context");
    if (level < 0 || level >= ctx->levels) return NST_E_ARG;
    if (gamma) *gamma = ctx->lv[level].anc.gamma;
    if (weighted) *weighted = ctx->lv[level].anc.weights ? 1 : 0;
    return NST_OK;
}

// The MRF term of one level (Li & Wand 2016; include/nst_hip.h has the definition): the style's weighted maps, their
// dictionaries, nn and the value partials.  Data of one job with the life cycle of nst_level_set_anchor: everything is made
// here, beside what the level has (a refusal changes nothing), the context's work is waited for before the level's block is
// replaced, and the captured closure, an optimiser's remembered closure and a pending backward half go.  The targets stay.
int nst_level_set_patches(nst_ctx* ctx, int level, const float* style, int hs, int ws, const float* weights, int stride, double epsilon,
                          void* stream) {
    if (ctx) { ++ctx->closure_epoch; ++ctx->ws_seq; }
    NSTCHK(bind(ctx));
    if (ctx->levels < 1) return fail(ctx, NST_E_STATE, "nst_job_configure has not been called");
    if (level < 0 || level >= ctx->levels) return fail(ctx, NST_E_ARG, "level out of range");
    LevelWs& L = ctx->lv[level];
    PatchLevel g;
    if (style) {
        if (!weights) return fail(ctx, NST_E_ARG, "null argument");
        for (int i = 0; i < 6; ++i) NSTCHK(take_weight(ctx, kMrfWords, weights, i, g));
        if (!(epsilon > 0.0) || std::isinf(epsilon)) return fail(ctx, NST_E_ARG, "the MRF epsilon must be finite and > 0");
        if (stride < 1 || stride > 8) return fail(ctx, NST_E_ARG, "the style stride must be 1..8");
    }
    std::optional<Scratch> sc;
    NSTCHK(begin_map_term(ctx, kMrfWords, L, g, style, hs, ws, stream, sc));
    if (sc) {
        hipStream_t s = sc->s;
        g.stride = stride; g.eps = epsilon; g.hs = hs; g.ws = ws;
        for (int i = 0; i < 6; ++i) {
            if (!(g.w[i] > 0.f)) continue;
            const int l = kTapLayer[i], C = kCout[l], mh = sc->acts.h[l], mw = sc->acts.w[l];
            PatchDict& d = g.d[i];
            if (!pm_dict_geometry(mh, mw, C, stride, &d)) return fail(ctx, NST_E_ARG, "a weighted map or its style map is below 3x3");
            float* fs = nullptr; unsigned* amax = nullptr; float* rq = nullptr; unsigned char* packed = nullptr;
            const size_t fs_n = (size_t)mh * mw * C, n = (size_t)(L.acts.h[l] - 2) * (L.acts.w[l] - 2);
            NSTCHK(g.mem.alloc(ctx, &fs, fs_n));
            NSTCHK(g.mem.alloc(ctx, &amax, (size_t)NST_AMAX_SLOTS));
            NSTCHK(g.mem.alloc(ctx, &rq, (size_t)pm_dict_tiles(d.m) * 32));
            NSTCHK(g.mem.alloc(ctx, &packed, pm_packed_bytes(d.m, C)));
            NSTCHK(g.mem.alloc(ctx, &g.keys[i], n));
            NSTCHK(g.mem.alloc(ctx, &g.nn[i], n));
            NSTCHK(g.mem.alloc(ctx, &g.partial[i], (size_t)PM_VALUE_BLOCKS));
            HIPCHK(ctx, hipMemcpyAsync(fs, sc->acts.act[l], fs_n * sizeof(float), hipMemcpyDeviceToDevice, s));
            HIPCHK(ctx, hipMemsetAsync(g.nn[i], 0, n * sizeof(int), s));
            d.fs = fs;
            HIPCHK(ctx, launch_pm_prepare(d, epsilon, amax, rq, packed, s));
            d.amax = amax; d.rq = rq; d.packed = packed;
        }
    }
    return commit_map_term(ctx, sc, L.pm, g);
}

int nst_level_patches(const nst_ctx* ctx, int level, float* weights, int* stride, double* epsilon) {
    if (!ctx) return fail(nullptr, NST_E_ARG, "null context");
    if (level < 0 || level >= ctx->levels) return fail(nullptr, NST_E_ARG, "level out of range");
    const PatchLevel& g = ctx->lv[level].pm;
    for (int i = 0; i < 6 && weights; ++i) weights[i] = g.w[i];
    if (stride) *stride = g.stride;
    if (epsilon) *epsilon = g.eps;
    return NST_OK;
}

// the unweighted mrf_i of the last closure (map_term_losses)
int nst_job_patch_losses(nst_ctx* ctx, float* out, void* stream) { return map_term_losses(ctx, T_MRF, out, stream); }

// the nn of the last closure of one weighted map of a level ((h - 2)(w - 2) int32 of the map; zeros before any closure)
int nst_level_patch_matches(nst_ctx* ctx, int level, int map, int* idx_out, void* stream) {
    NSTCHK(bind(ctx));
    if (level < 0 || level >= ctx->levels) return fail(ctx, NST_E_ARG, "level out of range");
    if (map < 0 || map > 5 || !idx_out) return fail(ctx, NST_E_ARG, "bad argument");
    const LevelWs& L = ctx->lv[level];
    if (!(L.pm.w[map] > 0.f)) return fail(ctx, NST_E_STATE, "the map carries no MRF term on this level (nst_level_set_patches)");
    const int l = kTapLayer[map];
    const size_t n = (size_t)(L.acts.h[l] - 2) * (L.acts.w[l] - 2);
    hipStream_t s = enter(ctx, stream);
    HIPCHK(ctx, hipMemcpyAsync(idx_out, L.pm.nn[map], n * sizeof(int), hipMemcpyDeviceToDevice, s));
    mark(ctx, s);
    return NST_OK;
}

// The histogram loss of one level (Risser, Wilmot & Barnes 2017; include/nst_hip.h has the definition): the range and counts of
// the style's weighted maps, and the image side's buffers.  The style's maps live on scratch only.  Life cycle of
// nst_level_set_patches: everything is made here beside what the level has (a refusal changes nothing), the context's work is
// waited for before the level's block is replaced, and the captured closure, an optimiser's remembered closure and a pending
// backward half go.  The targets stay.
int nst_level_set_histograms(nst_ctx* ctx, int level, const float* style, int hs, int ws, const float* weights, int bins, void* stream) {
    if (ctx) { ++ctx->closure_epoch; ++ctx->ws_seq; }
    NSTCHK(bind(ctx));
    if (ctx->levels < 1) return fail(ctx, NST_E_STATE, "nst_job_configure has not been called");
    if (level < 0 || level >= ctx->levels) return fail(ctx, NST_E_ARG, "level out of range");
    LevelWs& L = ctx->lv[level];
    HistLevel g;
    if (style) {
        if (!weights) return fail(ctx, NST_E_ARG, "null argument");
        for (int i = 0; i < 6; ++i) NSTCHK(take_weight(ctx, kHistWords, weights, i, g));
        if (bins < 2 || bins > 1024) return fail(ctx, NST_E_ARG, "the number of bins must be 2..1024");
    }
    std::optional<Scratch> sc;
    NSTCHK(begin_map_term(ctx, kHistWords, L, g, style, hs, ws, stream, sc));
    if (sc) {
        hipStream_t s = sc->s;
        g.bins = bins;
        for (int i = 0; i < 6; ++i) {
            if (!(g.w[i] > 0.f)) continue;
            const int l = kTapLayer[i], C = kCout[l];
            const size_t cb = (size_t)C * bins;
            g.Ns[i] = (size_t)sc->acts.h[l] * sc->acts.w[l];
            NSTCHK(g.mem.alloc(ctx, &g.s_lo_hi[i], (size_t)2 * C));
            NSTCHK(g.mem.alloc(ctx, &g.s_counts[i], cb));
            NSTCHK(g.mem.alloc(ctx, &g.lo_hi[i], (size_t)2 * C));
            NSTCHK(g.mem.alloc(ctx, &g.counts[i], cb));
            NSTCHK(g.mem.alloc(ctx, &g.ends[i], 2 * cb));
            NSTCHK(g.mem.alloc(ctx, &g.partial[i], (size_t)HIST_VALUE_BLOCKS));
            HIPCHK(ctx, launch_hist_counts(sc->acts.act[l], g.Ns[i], C, bins, g.s_lo_hi[i], g.s_counts[i], s));
            HIPCHK(ctx, hipMemsetAsync(g.lo_hi[i], 0, (size_t)2 * C * sizeof(float), s));
            HIPCHK(ctx, hipMemsetAsync(g.counts[i], 0, cb * sizeof(unsigned), s));
            HIPCHK(ctx, hipMemsetAsync(g.ends[i], 0, 2 * cb * sizeof(float), s));
        }
    }
    return commit_map_term(ctx, sc, L.hist, g);
}

int nst_level_histograms(const nst_ctx* ctx, int level, float* weights, int* bins) {
    if (!ctx) return fail(nullptr, NST_E_ARG, "null context");
    if (level < 0 || level >= ctx->levels) return fail(nullptr, NST_E_ARG, "level out of range");
    const HistLevel& g = ctx->lv[level].hist;
    for (int i = 0; i < 6 && weights; ++i) weights[i] = g.w[i];
    if (bins) *bins = g.bins;
    return NST_OK;
}

// the unweighted hist_i of the last closure (map_term_losses)
int nst_job_histogram_losses(nst_ctx* ctx, float* out, void* stream) { return map_term_losses(ctx, T_HIST, out, stream); }

// one weighted map of a level: the image side of the last closure (zeros before any closure), or the style's record
static int hist_read(nst_ctx* ctx, int level, int map, bool style, float* lo_hi, unsigned* counts, float* ends, void* stream) {
    NSTCHK(bind(ctx));
    if (level < 0 || level >= ctx->levels) return fail(ctx, NST_E_ARG, "level out of range");
    if (map < 0 || map > 5) return fail(ctx, NST_E_ARG, "bad argument");
    const HistLevel& g = ctx->lv[level].hist;
    if (!(g.w[map] > 0.f)) return fail(ctx, NST_E_STATE, "the map carries no histogram loss on this level (nst_level_set_histograms)");
    const int C = kCout[kTapLayer[map]];
    const size_t cb = (size_t)C * g.bins;
    hipStream_t s = enter(ctx, stream);
    if (lo_hi) HIPCHK(ctx, hipMemcpyAsync(lo_hi, style ? g.s_lo_hi[map] : g.lo_hi[map], (size_t)2 * C * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (counts) HIPCHK(ctx, hipMemcpyAsync(counts, style ? g.s_counts[map] : g.counts[map], cb * sizeof(unsigned), hipMemcpyDeviceToDevice, s));
    if (ends) HIPCHK(ctx, hipMemcpyAsync(ends, g.ends[map], 2 * cb * sizeof(float), hipMemcpyDeviceToDevice, s));
    mark(ctx, s);
    return NST_OK;
}
int nst_level_histogram_tables(nst_ctx* ctx, int level, int map, float* lo_hi, unsigned* counts, float* ends, void* stream) {
    return hist_read(ctx, level, map, false, lo_hi, counts, ends, stream);
}
int nst_level_histogram_style(nst_ctx* ctx, int level, int map, float* lo_hi, unsigned* counts, void* stream) {
    return hist_read(ctx, level, map, true, lo_hi, counts, nullptr, stream);
}

// The relaxed EMD term of one level (Kolkin et al. 2019; include/nst_hip.h has the definition): the style's weighted maps with
// their norms and packed operands, and every buffer the image side needs in a closure.  Life cycle of nst_level_set_patches:
// everything is made here beside what the level has (a refusal changes nothing), the context's work is waited for before the
// level's block is replaced, and the captured closure, an optimiser's remembered closure and a pending backward half go.  The
// targets stay.
int nst_level_set_remd(nst_ctx* ctx, int level, const float* style, int hs, int ws, const float* weights, const int* image_stride,
                       const int* style_stride, double epsilon, void* stream) {
    if (ctx) { ++ctx->closure_epoch; ++ctx->ws_seq; }
    NSTCHK(bind(ctx));
    if (ctx->levels < 1) return fail(ctx, NST_E_STATE, "nst_job_configure has not been called");
    if (level < 0 || level >= ctx->levels) return fail(ctx, NST_E_ARG, "level out of range");
    LevelWs& L = ctx->lv[level];
    RemdLevel g;
    if (style) {
        if (!weights || !image_stride || !style_stride) return fail(ctx, NST_E_ARG, "null argument");
        for (int i = 0; i < 6; ++i) {
            NSTCHK(take_weight(ctx, kRemdWords, weights, i, g));
            if (image_stride[i] < 1 || image_stride[i] > 256 || style_stride[i] < 1 || style_stride[i] > 256)
                return fail(ctx, NST_E_ARG, "the sample strides must be 1..256");
            g.si[i] = image_stride[i]; g.ss[i] = style_stride[i];
        }
        if (!(epsilon > 0.0) || std::isinf(epsilon)) return fail(ctx, NST_E_ARG, "the relaxed EMD epsilon must be finite and > 0");
    }
    std::optional<Scratch> sc;
    NSTCHK(begin_map_term(ctx, kRemdWords, L, g, style, hs, ws, stream, sc));
    if (sc) {
        hipStream_t s = sc->s;
        g.eps = epsilon; g.hs = hs; g.ws = ws;
        for (int i = 0; i < 6; ++i) {
            if (!(g.w[i] > 0.f)) continue;
            const int l = kTapLayer[i], C = kCout[l], mh = sc->acts.h[l], mw = sc->acts.w[l];
            RemdSide& y = g.y[i];
            RemdSide x{};
            if (!remd_side_geometry(mh, mw, C, g.ss[i], &y) || !remd_side_geometry(L.acts.h[l], L.acts.w[l], C, g.si[i], &x))
                return fail(ctx, NST_E_ARG, "a weighted map or its style map is too large");
            const int n = x.count, m = y.count;
            g.n[i] = n;
            float* fs = nullptr; unsigned* amax = nullptr; float* rq = nullptr; unsigned char* packed = nullptr;
            const size_t fs_n = (size_t)mh * mw * C;
            NSTCHK(g.mem.alloc(ctx, &fs, fs_n));
            NSTCHK(g.mem.alloc(ctx, &amax, (size_t)NST_AMAX_SLOTS));
            NSTCHK(g.mem.alloc(ctx, &rq, (size_t)remd_tiles(m) * 32));
            NSTCHK(g.mem.alloc(ctx, &packed, remd_packed_bytes(m, C)));
            NSTCHK(g.mem.alloc(ctx, &g.rp[i], (size_t)remd_tiles(n) * 32));
            NSTCHK(g.mem.alloc(ctx, &g.xpacked[i], remd_packed_bytes(n, C)));
            NSTCHK(g.mem.alloc(ctx, &g.keysA[i], (size_t)n));
            NSTCHK(g.mem.alloc(ctx, &g.keysB[i], (size_t)m));
            NSTCHK(g.mem.alloc(ctx, &g.nnA[i], (size_t)n));
            NSTCHK(g.mem.alloc(ctx, &g.nnB[i], (size_t)m));
            NSTCHK(g.mem.alloc(ctx, &g.cosA[i], (size_t)n));
            NSTCHK(g.mem.alloc(ctx, &g.cosB[i], (size_t)m));
            NSTCHK(g.mem.alloc(ctx, &g.partial[i], (size_t)2 * REMD_VALUE_BLOCKS));
            NSTCHK(g.mem.alloc(ctx, &g.rec[i], 3));
            NSTCHK(g.mem.alloc(ctx, &g.side[i], 1));
            HIPCHK(ctx, hipMemcpyAsync(fs, sc->acts.act[l], fs_n * sizeof(float), hipMemcpyDeviceToDevice, s));
            HIPCHK(ctx, hipMemsetAsync(g.nnA[i], 0, (size_t)n * sizeof(int), s));
            HIPCHK(ctx, hipMemsetAsync(g.nnB[i], 0, (size_t)m * sizeof(int), s));
            HIPCHK(ctx, hipMemsetAsync(g.rec[i], 0, 3 * sizeof(float), s));
            HIPCHK(ctx, hipMemsetAsync(g.side[i], 0, sizeof(int), s));
            y.f = fs;
            HIPCHK(ctx, launch_zero(amax, NST_AMAX_SLOTS, s));
            HIPCHK(ctx, launch_absmax_slots(fs, fs_n, amax, s));
            y.amax = amax;
            HIPCHK(ctx, launch_remd_norms(y, epsilon, rq, s));
            HIPCHK(ctx, launch_remd_pack(y, packed, s));
            y.r = rq; y.packed = packed;
        }
    }
    return commit_map_term(ctx, sc, L.remd, g);
}

int nst_level_remd(const nst_ctx* ctx, int level, float* weights, int* image_stride, int* style_stride, double* epsilon, int* hs, int* ws) {
    if (!ctx) return fail(nullptr, NST_E_ARG, "null context");
    if (level < 0 || level >= ctx->levels) return fail(nullptr, NST_E_ARG, "level out of range");
    const RemdLevel& g = ctx->lv[level].remd;
    for (int i = 0; i < 6 && weights; ++i) weights[i] = g.w[i];
    for (int i = 0; i < 6 && image_stride; ++i) image_stride[i] = g.si[i];
    for (int i = 0; i < 6 && style_stride; ++i) style_stride[i] = g.ss[i];
    if (epsilon) *epsilon = g.eps;
    if (hs) *hs = g.hs;
    if (ws) *ws = g.ws;
    return NST_OK;
}

// the unweighted remd_i of the last closure (map_term_losses)
int nst_job_remd_losses(nst_ctx* ctx, float* out, void* stream) { return map_term_losses(ctx, T_REMD, out, stream); }

// the matches and the side of the last closure of one weighted map of a level (nnA: n int32, nnB: m int32, side: one int32;
// zeros before any closure; each nullable)
int nst_level_remd_matches(nst_ctx* ctx, int level, int map, int* nnA_out, int* nnB_out, int* side_out, void* stream) {
    NSTCHK(bind(ctx));
    if (level < 0 || level >= ctx->levels) return fail(ctx, NST_E_ARG, "level out of range");
    if (map < 0 || map > 5 || (!nnA_out && !nnB_out && !side_out)) return fail(ctx, NST_E_ARG, "bad argument");
    const RemdLevel& g = ctx->lv[level].remd;
    if (!(g.w[map] > 0.f)) return fail(ctx, NST_E_STATE, "the map carries no relaxed EMD term on this level (nst_level_set_remd)");
    hipStream_t s = enter(ctx, stream);
    if (nnA_out) HIPCHK(ctx, hipMemcpyAsync(nnA_out, g.nnA[map], (size_t)g.n[map] * sizeof(int), hipMemcpyDeviceToDevice, s));
    if (nnB_out) HIPCHK(ctx, hipMemcpyAsync(nnB_out, g.nnB[map], (size_t)g.y[map].count * sizeof(int), hipMemcpyDeviceToDevice, s));
    if (side_out) HIPCHK(ctx, hipMemcpyAsync(side_out, g.side[map], sizeof(int), hipMemcpyDeviceToDevice, s));
    mark(ctx, s);
    return NST_OK;
}

// The self-similarity term of one level (Kolkin et al. 2019; include/nst_hip.h has the definition): the content image goes
// through the network on scratch, and per weighted map the content's D and q are made by the launches a closure uses on the
// image's map - in the level's own D, s and partial buffers, which the first closure overwrites - beside every buffer a closure
// needs.  Life cycle of nst_level_set_remd.
int nst_level_set_selfsim(nst_ctx* ctx, int level, const float* content, int h, int w, const float* weights, const int* stride, double epsilon,
                          void* stream) {
    if (ctx) { ++ctx->closure_epoch; ++ctx->ws_seq; }
    NSTCHK(bind(ctx));
    if (ctx->levels < 1) return fail(ctx, NST_E_STATE, "nst_job_configure has not been called");
    if (level < 0 || level >= ctx->levels) return fail(ctx, NST_E_ARG, "level out of range");
    LevelWs& L = ctx->lv[level];
    SelfSimLevel g;
    if (content) {
        if (!weights || !stride) return fail(ctx, NST_E_ARG, "null argument");
        for (int i = 0; i < 6; ++i) {
            NSTCHK(take_weight(ctx, kSelfSimWords, weights, i, g));
            if (stride[i] < 1 || stride[i] > 256) return fail(ctx, NST_E_ARG, "the sample strides must be 1..256");
            g.stride[i] = stride[i];
        }
        if (!(epsilon > 0.0) || std::isinf(epsilon)) return fail(ctx, NST_E_ARG, "the self-similarity epsilon must be finite and > 0");
        for (int i = 0; i < 6; ++i) {
            RemdSide x{};
            const int l = kTapLayer[i];
            if (g.w[i] > 0.f && remd_side_geometry(L.acts.h[l], L.acts.w[l], kCout[l], g.stride[i], &x) && x.count > SELFSIM_MAX_SAMPLES)
                return fail(ctx, NST_E_ARG, "a weighted map has more than 4096 samples at its stride");
        }
    }
    std::optional<Scratch> sc;
    NSTCHK(begin_map_term(ctx, kSelfSimWords, L, g, content, h, w, stream, sc));
    if (sc) {
        hipStream_t s = sc->s;
        g.eps = epsilon;
        for (int i = 0; i < 6; ++i) {
            if (!(g.w[i] > 0.f)) continue;
            const int l = kTapLayer[i], C = kCout[l];
            RemdSide y{};
            if (!remd_side_geometry(sc->acts.h[l], sc->acts.w[l], C, g.stride[i], &y) || sc->acts.h[l] != L.acts.h[l] || sc->acts.w[l] != L.acts.w[l])
                return fail(ctx, NST_E_ARG, "a weighted map is too large");
            const size_t n = (size_t)y.count;
            g.n[i] = y.count;
            NSTCHK(g.mem.alloc(ctx, &g.Dc[i], n * n));
            NSTCHK(g.mem.alloc(ctx, &g.qc[i], n));
            NSTCHK(g.mem.alloc(ctx, &g.rp[i], (size_t)remd_tiles(y.count) * 32));
            NSTCHK(g.mem.alloc(ctx, &g.xpacked[i], remd_packed_bytes(y.count, C)));
            NSTCHK(g.mem.alloc(ctx, &g.D[i], n * n));
            NSTCHK(g.mem.alloc(ctx, &g.s[i], n));
            NSTCHK(g.mem.alloc(ctx, &g.q[i], n));
            NSTCHK(g.mem.alloc(ctx, &g.sg[i], n * n));
            NSTCHK(g.mem.alloc(ctx, &g.t[i], n));
            NSTCHK(g.mem.alloc(ctx, &g.partial[i], (size_t)2 * SELFSIM_ROW_BLOCKS * n));
            NSTCHK(g.mem.alloc(ctx, &g.W[i], n * n));
            NSTCHK(g.mem.alloc(ctx, &g.U[i], n * (size_t)C));
            // the content's side by the closure's launches: norms, pack, matrix, column sums
            y.f = sc->acts.act[l]; y.amax = amax_act(sc->acts, l);
            HIPCHK(ctx, launch_remd_norms(y, epsilon, g.rp[i], s));
            y.r = g.rp[i];
            HIPCHK(ctx, launch_remd_pack(y, g.xpacked[i], s));
            y.packed = g.xpacked[i];
            HIPCHK(ctx, launch_selfsim_matrix(y, g.Dc[i], s));
            HIPCHK(ctx, launch_selfsim_colsums(g.Dc[i], y.count, epsilon, g.partial[i], g.s[i], g.qc[i], s));
            // what nst_level_selfsim_decisions reads before any closure
            HIPCHK(ctx, hipMemsetAsync(g.D[i], 0, n * n * sizeof(float), s));
            HIPCHK(ctx, hipMemsetAsync(g.s[i], 0, n * sizeof(double), s));
            HIPCHK(ctx, hipMemsetAsync(g.sg[i], 0, n * n, s));
        }
    }
    return commit_map_term(ctx, sc, L.selfsim, g);
}

int nst_level_selfsim(const nst_ctx* ctx, int level, float* weights, int* stride, double* epsilon) {
    if (!ctx) return fail(nullptr, NST_E_ARG, "null context");
    if (level < 0 || level >= ctx->levels) return fail(nullptr, NST_E_ARG, "level out of range");
    const SelfSimLevel& g = ctx->lv[level].selfsim;
    for (int i = 0; i < 6 && weights; ++i) weights[i] = g.w[i];
    for (int i = 0; i < 6 && stride; ++i) stride[i] = g.stride[i];
    if (epsilon) *epsilon = g.eps;
    return NST_OK;
}

// the unweighted selfsim_k of the last closure (map_term_losses)
int nst_job_selfsim_losses(nst_ctx* ctx, float* out, void* stream) { return map_term_losses(ctx, T_SELFSIM, out, stream); }

// D (n x n float), s (n double) and sg (n x n int8) of the last closure of one weighted map of a level (zeros before any
// closure; each nullable)
int nst_level_selfsim_decisions(nst_ctx* ctx, int level, int map, float* D_out, double* s_out, signed char* sg_out, void* stream) {
    NSTCHK(bind(ctx));
    if (level < 0 || level >= ctx->levels) return fail(ctx, NST_E_ARG, "level out of range");
    if (map < 0 || map > 5 || (!D_out && !s_out && !sg_out)) return fail(ctx, NST_E_ARG, "bad argument");
    const SelfSimLevel& g = ctx->lv[level].selfsim;
    if (!(g.w[map] > 0.f)) return fail(ctx, NST_E_STATE, "the map carries no self-similarity term on this level (nst_level_set_selfsim)");
    const size_t n = (size_t)g.n[map];
    hipStream_t s = enter(ctx, stream);
    if (D_out) HIPCHK(ctx, hipMemcpyAsync(D_out, g.D[map], n * n * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (s_out) HIPCHK(ctx, hipMemcpyAsync(s_out, g.s[map], n * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (sg_out) HIPCHK(ctx, hipMemcpyAsync(sg_out, g.sg[map], n * n, hipMemcpyDeviceToDevice, s));
    mark(ctx, s);
    return NST_OK;
}

// The long-range style term of one level (Berger & Memisevic 2017; include/nst_hip.h has the definition): the style image goes
// through the network on scratch, and per weighted map the style's G_d stack is made by the launches a closure uses on the
// image's map, beside every buffer a closure needs.  Life cycle of nst_level_set_remd.
int nst_level_set_xcorr(nst_ctx* ctx, int level, const float* style, int hs, int ws, const float* weights, const int* shifts, int n,
                        void* stream) {
    if (ctx) { ++ctx->closure_epoch; ++ctx->ws_seq; }
    NSTCHK(bind(ctx));
    if (ctx->levels < 1) return fail(ctx, NST_E_STATE, "nst_job_configure has not been called");
    if (level < 0 || level >= ctx->levels) return fail(ctx, NST_E_ARG, "level out of range");
    LevelWs& L = ctx->lv[level];
    XcorrLevel g;
    if (style) {
        if (!weights || !shifts) return fail(ctx, NST_E_ARG, "null argument");
        for (int i = 0; i < 6; ++i) NSTCHK(take_weight(ctx, kXcorrWords, weights, i, g));
        if (n < 1 || n > XCORR_MAX_SHIFTS) return fail(ctx, NST_E_ARG, "the xcorr term takes 1..16 shifts");
        for (int d = 0; d < n; ++d) {
            const int dx = shifts[2 * d], dy = shifts[2 * d + 1];
            if (dx < 0 || dy < 0 || dx > 64 || dy > 64 || (dx == 0 && dy == 0))
                return fail(ctx, NST_E_ARG, "a shift (dx, dy) has 0 <= dx, dy <= 64, not both 0");
            for (int e = 0; e < d; ++e)
                if (g.dx[e] == dx && g.dy[e] == dy) return fail(ctx, NST_E_ARG, "the shifts must be distinct");
            g.dx[d] = dx; g.dy[d] = dy;
        }
        g.nd = n;
        // a shift must leave a pair on every weighted map, of the level's image and of the style image
        for (int i = 0; i < 6; ++i) {
            if (!(g.w[i] > 0.f)) continue;
            const int l = kTapLayer[i];
            for (int d = 0; d < n; ++d)
                if (g.dx[d] >= L.acts.w[l] || g.dy[d] >= L.acts.h[l] || g.dx[d] >= (ws >> kScale[l]) || g.dy[d] >= (hs >> kScale[l]))
                    return fail(ctx, NST_E_ARG, "a shift is not smaller than a weighted map or its style map");
        }
    }
    std::optional<Scratch> sc;
    NSTCHK(begin_map_term(ctx, kXcorrWords, L, g, style, hs, ws, stream, sc));
    if (sc) {
        hipStream_t s = sc->s;
        g.hs = hs; g.ws = ws;
        XcorrBatch b{};
        auto flush = [&]() -> int {
            if (b.n > 0) HIPCHK(ctx, launch_xcorr_batch(b, s));
            b.n = 0;
            return NST_OK;
        };
        for (int i = 0; i < 6; ++i) {
            if (!(g.w[i] > 0.f)) continue;
            const int l = kTapLayer[i], C = kCout[l], mh = sc->acts.h[l], mw = sc->acts.w[l];
            const size_t CC = (size_t)C * C, stack = (size_t)g.nd * CC;
            NSTCHK(g.mem.alloc(ctx, &g.Gt[i], stack));
            NSTCHK(g.mem.alloc(ctx, &g.G[i], stack));
            NSTCHK(g.mem.alloc(ctx, &g.S[i], stack));
            NSTCHK(g.mem.alloc(ctx, &g.St[i], stack));
            NSTCHK(g.mem.alloc(ctx, &g.sq[i], (size_t)g.nd * xcorr_finish_blocks(C)));
            // what nst_level_xcorr_matrices reads before any closure
            HIPCHK(ctx, hipMemsetAsync(g.G[i], 0, stack * sizeof(float), s));
            for (int d = 0; d < g.nd; ++d) {
                XcorrGeometry own, sty;
                if (!xcorr_geometry(C, L.acts.h[l], L.acts.w[l], g.dx[d], g.dy[d], &own) || !xcorr_geometry(C, mh, mw, g.dx[d], g.dy[d], &sty))
                    return fail(ctx, NST_E_ARG, "a weighted map or its style map is too large, or a shift is not smaller than it");
                NSTCHK(g.mem.alloc(ctx, &g.part[i][d], (size_t)own.nsplit * CC));
                // the style's G_d by the closure's launches, its slabs on scratch
                float* part = nullptr;
                NSTCHK(sc->alloc(&part, (size_t)sty.nsplit * CC));
                if (b.n == XCORR_BATCH_MAX) NSTCHK(flush());
                XcorrItem& it = b.it[b.n++];
                it = XcorrItem{};
                it.f = sc->acts.act[l]; it.amax = amax_act(sc->acts, l); it.part = part;
                it.C = C; it.h = mh; it.w = mw; it.dx = g.dx[d]; it.dy = g.dy[d];
                it.divisor = (float)((double)C * (double)(mh - g.dy[d]) * (double)(mw - g.dx[d]));
                it.G = g.Gt[i] + d * CC;
            }
        }
        NSTCHK(flush());
    }
    return commit_map_term(ctx, sc, L.xcorr, g);
}

int nst_level_xcorr(const nst_ctx* ctx, int level, float* weights, int* shifts, int* n, int* hs, int* ws) {
    if (!ctx) return fail(nullptr, NST_E_ARG, "null context");
    if (level < 0 || level >= ctx->levels) return fail(nullptr, NST_E_ARG, "level out of range");
    const XcorrLevel& g = ctx->lv[level].xcorr;
    for (int i = 0; i < 6 && weights; ++i) weights[i] = g.w[i];
    for (int d = 0; d < XCORR_MAX_SHIFTS && shifts; ++d) { shifts[2 * d] = d < g.nd ? g.dx[d] : 0; shifts[2 * d + 1] = d < g.nd ? g.dy[d] : 0; }
    if (n) *n = g.nd;
    if (hs) *hs = g.hs;
    if (ws) *ws = g.ws;
    return NST_OK;
}

// the unweighted xcorr_i of the last closure (map_term_losses)
int nst_job_xcorr_losses(nst_ctx* ctx, float* out, void* stream) { return map_term_losses(ctx, T_XCORR, out, stream); }

// the G_d stack (|D| x C x C floats) of the last closure of one weighted map of a level (zeros before any closure)
int nst_level_xcorr_matrices(nst_ctx* ctx, int level, int map, float* G_out, void* stream) {
    NSTCHK(bind(ctx));
    if (level < 0 || level >= ctx->levels) return fail(ctx, NST_E_ARG, "level out of range");
    if (map < 0 || map > 5 || !G_out) return fail(ctx, NST_E_ARG, "bad argument");
    const XcorrLevel& g = ctx->lv[level].xcorr;
    if (!(g.w[map] > 0.f)) return fail(ctx, NST_E_STATE, "the map carries no xcorr term on this level (nst_level_set_xcorr)");
    const size_t C = (size_t)kCout[kTapLayer[map]];
    hipStream_t s = enter(ctx, stream);
    HIPCHK(ctx, hipMemcpyAsync(G_out, g.G[map], (size_t)g.nd * C * C * sizeof(float), hipMemcpyDeviceToDevice, s));
    mark(ctx, s);
    return NST_OK;
}

// The semantic guidance of a level's MRF term (neural-doodle; include/nst_hip.h has the definition).  The planes of both sides
// are checked for their range and pooled on scratch; what stays with the level - in PatchGuide's own block, beside the old one
// until the call has succeeded - are the descriptors of every weighted map and the buffer of the image patches' norms.  The
// life cycle is that of nst_level_set_patches.  R = 0, gamma = 0 or null planes clear.
int nst_level_set_patch_guidance(nst_ctx* ctx, int level, int R, const float* content_planes, const float* style_planes, float gamma,
                                 void* stream) {
    if (ctx) { ++ctx->closure_epoch; ++ctx->ws_seq; }
    NSTCHK(bind(ctx));
    if (ctx->levels < 1) return fail(ctx, NST_E_STATE, "nst_job_configure has not been called");
    if (level < 0 || level >= ctx->levels) return fail(ctx, NST_E_ARG, "level out of range");
    if (R < 0 || R > NST_MAX_REGIONS) return fail(ctx, NST_E_ARG, "the number of regions must be 0 .. NST_MAX_REGIONS");
    if (!(gamma >= 0.f) || std::isinf(gamma)) return fail(ctx, NST_E_ARG, "the semantic weight must be finite and >= 0");
    LevelWs& L = ctx->lv[level];
    PatchGuide g;
    hipStream_t s = enter(ctx, stream);
    if (R > 0 && gamma > 0.f && content_planes && style_planes) {
        if (!L.pm.on()) return fail(ctx, NST_E_STATE, "the level carries no MRF term (nst_level_set_patches first)");
        g.R = R; g.gamma = gamma;
        int deepest = 0;                               // the deepest network scale among the weighted maps
        for (int i = 0; i < 6; ++i)
            if (L.pm.w[i] > 0.f && kScale[kTapLayer[i]] > deepest) deepest = kScale[kTapLayer[i]];
        Scratch sc(ctx, s);
        // both pyramids: side 0 the level image's planes, side 1 the style image's; off[k][scale] in floats
        const float* src[2] = {content_planes, style_planes};
        const int hh[2] = {L.h, L.pm.hs}, ww[2] = {L.w, L.pm.ws};
        float* pyr[2] = {};
        size_t off[2][6];
        double* dscratch = nullptr;
        NSTCHK(sc.alloc(&dscratch, ((size_t)R * GUIDE_MASS_BLOCKS + 2 * R) * 2));
        double* counts = dscratch + (size_t)R * GUIDE_MASS_BLOCKS * 2;
        for (int k = 0; k < 2; ++k) {
            off[k][0] = 0;
            for (int scl = 0; scl < 5; ++scl) off[k][scl + 1] = off[k][scl] + (size_t)R * (hh[k] >> scl) * (ww[k] >> scl);
            NSTCHK(sc.alloc(&pyr[k], off[k][deepest + 1]));
            HIPCHK(ctx, hipMemcpyAsync(pyr[k], src[k], (size_t)R * hh[k] * ww[k] * sizeof(float), hipMemcpyDeviceToDevice, s));
            // (mass, values outside [0,1] or not finite) of every plane: the count is what is asked here - a region may be empty
            HIPCHK(ctx, launch_guide_mass(pyr[k], R, (size_t)hh[k] * ww[k], dscratch, counts + (size_t)k * R * 2, s));
            for (int scl = 1; scl <= deepest; ++scl)
                HIPCHK(ctx, launch_guide_pool(pyr[k] + off[k][scl - 1], R, hh[k] >> (scl - 1), ww[k] >> (scl - 1), pyr[k] + off[k][scl], s));
        }
        double host[2 * NST_MAX_REGIONS * 2];
        HIPCHK(ctx, hipMemcpyAsync(host, counts, (size_t)2 * R * 2 * sizeof(double), hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipStreamSynchronize(s));
        for (int k = 0; k < 2 * R; ++k)
            if (host[2 * k + 1] > 0.0) return fail(ctx, NST_E_ARG, "semantic plane values must be finite and in [0,1]");
        for (int i = 0; i < 6; ++i) {
            if (!(L.pm.w[i] > 0.f)) continue;
            const int l = kTapLayer[i], scl = kScale[l];
            const PatchDict& d = L.pm.d[i];
            const int hm = L.acts.h[l], wm = L.acts.w[l];
            const int n = (hm - 2) * (wm - 2), padded = pm_dict_tiles(d.m) * 32;
            NSTCHK(g.mem.alloc(ctx, &g.gd[i], (size_t)n * 4));
            NSTCHK(g.mem.alloc(ctx, &g.ge[i], (size_t)padded * 4));
            NSTCHK(g.mem.alloc(ctx, &g.rp[i], (size_t)pm_dict_tiles(n) * 32));
            HIPCHK(ctx, launch_pm_descriptors(pyr[0] + off[0][scl], R, hm, wm, 1, L.pm.eps, n, g.gd[i], s));
            HIPCHK(ctx, launch_pm_descriptors(pyr[1] + off[1][scl], R, d.hs, d.ws, d.stride, L.pm.eps, padded, g.ge[i], s));
            HIPCHK(ctx, hipMemsetAsync(g.rp[i], 0, (size_t)pm_dict_tiles(n) * 32 * sizeof(float), s));
        }
        NSTCHK(sc.finish());       // (synchronises: the caller's planes are free again when this returns)
    }
    quiesce(ctx);
    drop_closure_state(ctx, false);
    L.pm.sem = std::move(g);
    return NST_OK;
}

int nst_level_patch_guidance(const nst_ctx* ctx, int level, int* R, float* gamma, int* hs, int* ws) {
    if (!ctx) return fail(nullptr, NST_E_ARG, "null context");
    if (level < 0 || level >= ctx->levels) return fail(nullptr, NST_E_ARG, "level out of range");
    const PatchGuide& g = ctx->lv[level].pm.sem;
    if (R) *R = g.R;
    if (gamma) *gamma = g.gamma;
    if (hs) *hs = ctx->lv[level].pm.hs;
    if (ws) *ws = ctx->lv[level].pm.ws;
    return NST_OK;
}

// Per-layer style weights (the w_l of Gatys, Ecker & Bethge 2016): a factor of each map's term in the loss row and in the
// coefficient of its Gram backward.  The targets do not depend on them and stay; what an optimiser remembers of a closure,
// a pending backward half and a captured graph (the coefficients are baked into it) do not.
int nst_job_set_style_weights(nst_ctx* ctx, const float* w) {
    if (ctx) { ++ctx->closure_epoch; ++ctx->ws_seq; }
    NSTCHK(bind(ctx));
    if (!w) return fail(ctx, NST_E_ARG, "null argument");
    for (int i = 0; i < 6; ++i)
        if (!(w[i] >= 0.f) || std::isinf(w[i])) return fail(ctx, NST_E_ARG, "style layer weights must be finite and >= 0");
    if ((style_mask_of(ctx->taps) & positive_weight_mask(w)) == 0u)
        return fail(ctx, NST_E_ARG, "at least one map of the current style set needs a positive style layer weight");
    quiesce(ctx);
    drop_closure_state(ctx, false);
    for (int i = 0; i < 6; ++i) ctx->style_w[i] = w[i];
    return NST_OK;
}

int nst_job_style_weights(const nst_ctx* ctx, float* w) {
    if (!ctx || !w) return fail(nullptr, NST_E_ARG, "null argument");
    for (int i = 0; i < 6; ++i) w[i] = ctx->style_w[i];
    return NST_OK;
}

int nst_set_timing(nst_ctx* ctx, int enabled) {
    NSTCHK(bind(ctx));
    ctx->timing = enabled;
    if (enabled >= 2 && ctx->ev_pool.empty()) {
        ctx->ev_pool.resize(2048);
        for (auto& e : ctx->ev_pool) HIPCHK(ctx, hipEventCreate(&e));
    }
    return NST_OK;
}

int nst_last_closure_ms(nst_ctx* ctx, float* ms) {
    NSTCHK(bind(ctx));
    if (!ms) return fail(ctx, NST_E_ARG, "null argument");
    *ms = 0.f;
    if (!ctx->timed_valid) return NST_OK;
    HIPCHK(ctx, hipEventSynchronize(ctx->t1));
    HIPCHK(ctx, hipEventElapsedTime(ms, ctx->t0, ctx->t1));
    return NST_OK;
}

// per kernel class of the last closure: summed launch durations (ms), launch count, algorithmic flops
int nst_last_closure_class(nst_ctx* ctx, int cls, float* ms, int* launches, double* flops) {
    NSTCHK(bind(ctx));
    if (!ms || !launches || !flops || cls < 0 || cls >= K_NCLASS) return fail(ctx, NST_E_ARG, "bad argument");
    *ms = 0.f; *launches = 0; *flops = 0.0;
    if (!ctx->timed_valid) return NST_OK;
    HIPCHK(ctx, hipEventSynchronize(ctx->t1));
    for (const TimedLaunch& t : ctx->timed) {
        if (t.cls != cls) continue;
        float d = 0.f;
        HIPCHK(ctx, hipEventSynchronize(t.b));
        HIPCHK(ctx, hipEventElapsedTime(&d, t.a, t.b));
        *ms += d; *launches += 1; *flops += t.flops;
    }
    return NST_OK;
}

// the timed launches of the last closure in launch order, with the kernel shape the conv_h2 launcher decided for each
int nst_last_closure_launches(nst_ctx* ctx, nst_launch_info* out, int capacity, int* count) {
    NSTCHK(bind(ctx));
    if (!count || capacity < 0 || (capacity > 0 && !out)) return fail(ctx, NST_E_ARG, "bad argument");
    *count = ctx->timed_valid ? (int)ctx->timed.size() : 0;
    for (int i = 0; i < *count && i < capacity; ++i) {
        const TimedLaunch& t = ctx->timed[i];
        const H2Shape& sh = t.shape;
        out[i] = nst_launch_info{t.cls, t.tag[0], t.tag[1], t.tag[2], t.tag[3], t.tag[5], sh.rows, sh.bn, sh.ntw, sh.chunk,
                                 sh.m16, sh.persist, sh.second, sh.unpool, sh.bands};
    }
    return NST_OK;
}

// what the last nst_closure* call did with streams and graphs: host counters of the context, nothing is launched or waited for
int nst_last_closure_schedule(const nst_ctx* ctx, int* side_forks, int* level_streams, int* graph_replay) {
    if (!ctx) return fail(nullptr, NST_E_ARG, "null context");
    if (side_forks) *side_forks = ctx->sched.side_forks;
    if (level_streams) *level_streams = ctx->sched.level_streams;
    if (graph_replay) *graph_replay = ctx->sched.graph_replay;
    return NST_OK;
}

// debugging aid: one line per timed launch of the last closure to stderr
int nst_dump_last_closure(nst_ctx* ctx) {
    NSTCHK(bind(ctx));
    if (!ctx->timed_valid) return NST_OK;
    HIPCHK(ctx, hipEventSynchronize(ctx->t1));
    for (const TimedLaunch& t : ctx->timed) {
        float d = 0.f;
        HIPCHK(ctx, hipEventSynchronize(t.b));
        HIPCHK(ctx, hipEventElapsedTime(&d, t.a, t.b));
        char shape[64] = "";
        if (t.shape.rows > 0)
            snprintf(shape, sizeof(shape), "  h2<%d,%d,%d,%d>%s%s x%d", t.shape.rows, t.shape.bn, t.shape.ntw, t.shape.chunk,
                     t.shape.m16 ? " m16" : "", t.shape.persist ? " persist" : "", t.shape.bands);
        fprintf(stderr, "cls %d  %4dx%-4d cin %3d cout %3d taps %d layer %3d  %8.3f ms  %7.2f TFLOP/s%s\n", t.cls, t.tag[0],
                t.tag[1], t.tag[2], t.tag[3], t.tag[4], t.tag[5], d, d > 0 ? t.flops / (d * 1e-3) / 1e12 : 0.0, shape);
    }
    return NST_OK;
}

// totals since the last reset (timing mode 2): per kernel class cls in 0..3 (0 = 3x3 MFMA conv fwd+dgrad,
// 1 = Gram forward + its 1x1 backward, 2 = conv1_1 fwd+dgrad, 3 = streaming kernels); cls = -1: whole closures
// (ms = summed closure wall on the caller's stream, launches = closures).  reset != 0 clears afterwards.
int nst_timing_totals(nst_ctx* ctx, int cls, double* ms, long* launches, double* flops, int reset) {
    NSTCHK(bind(ctx));
    if (!ms || !launches || !flops || cls < -2 || cls >= K_NCLASS) return fail(ctx, NST_E_ARG, "bad argument");
    NSTCHK(fold_timed(ctx));
    if (cls == -2) { *ms = 0; *launches = ctx->acc_sampled; *flops = 0; }       // closures with per-launch events
    else if (cls < 0) { *ms = ctx->acc_closure_ms; *launches = ctx->acc_closures; *flops = 0; }
    else { *ms = ctx->acc_ms[cls]; *launches = ctx->acc_launches[cls]; *flops = ctx->acc_flops[cls]; }
    if (reset) {
        for (int i = 0; i < 4; ++i) { ctx->acc_ms[i] = 0; ctx->acc_flops[i] = 0; ctx->acc_mfma[i] = 0; ctx->acc_launches[i] = 0; }
        ctx->acc_closure_ms = 0; ctx->acc_closures = 0; ctx->acc_sampled = 0;
    }
    return NST_OK;
}

int nst_timing_mfma_flops(nst_ctx* ctx, int cls, double* mfma_flops) {
    NSTCHK(bind(ctx));
    if (!mfma_flops || cls < 0 || cls >= K_NCLASS) return fail(ctx, NST_E_ARG, "bad argument");
    NSTCHK(fold_timed(ctx));
    *mfma_flops = ctx->acc_mfma[cls];
    return NST_OK;
}

// ---- not part of the public ABI ------------------------------------------------------------------
// test hooks (tests/test_hip_unread_maps.py): the raw NHWC buffer of one feature map filled with a byte / copied to `dst`
// (device memory), on a stream of their own and waited for - see zero_now
int nst_internal_map_fill(nst_ctx* ctx, int level, int layer, int byte) {
    if (!ctx || level < 0 || level >= ctx->levels || layer < 0 || layer >= NL) return 1;
    const ActSet& a = ctx->lv[level].acts;
    const size_t bytes = (size_t)a.h[layer] * a.w[layer] * kCout[layer] * 4;
    if (hipSetDevice(ctx->device) != hipSuccess) return 1;
    quiesce(ctx);
    hipStream_t zs = nullptr;
    if (hipStreamCreateWithFlags(&zs, hipStreamNonBlocking) != hipSuccess) return 1;
    hipError_t e = hipMemsetAsync(a.act[layer], byte, bytes, zs);
    if (e == hipSuccess) e = hipStreamSynchronize(zs);
    (void)hipStreamDestroy(zs);
    return e == hipSuccess ? 0 : 1;
}
int nst_internal_map_read(nst_ctx* ctx, int level, int layer, void* dst) {
    if (!ctx || !dst || level < 0 || level >= ctx->levels || layer < 0 || layer >= NL) return 1;
    const ActSet& a = ctx->lv[level].acts;
    const size_t bytes = (size_t)a.h[layer] * a.w[layer] * kCout[layer] * 4;
    if (hipSetDevice(ctx->device) != hipSuccess) return 1;
    quiesce(ctx);
    hipStream_t zs = nullptr;
    if (hipStreamCreateWithFlags(&zs, hipStreamNonBlocking) != hipSuccess) return 1;
    hipError_t e = hipMemcpyAsync(dst, a.act[layer], bytes, hipMemcpyDeviceToDevice, zs);
    if (e == hipSuccess) e = hipStreamSynchronize(zs);
    (void)hipStreamDestroy(zs);
    return e == hipSuccess ? 0 : 1;
}

}  // extern "C"
