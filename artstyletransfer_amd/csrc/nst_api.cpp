// nst_api.cpp - C ABI of libnst_hip.so (include/nst_hip.h): context (VGG19 weights re-laid-out for
// the gfx950 kernels), per-job pyramid workspace, the closure (forward + losses + backward of
// every pyramid level, one HIP stream per level), and the Adam / L-BFGS drivers.
//
// Host-side control only; every FLOP and byte of the path is in the .hip kernels.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/nst_hip.h"
#include "nst_kernels.h"

using namespace nst;

namespace {

constexpr int NL = NST_VGG19_CONVS;
const int kCin[NL] = {3, 64, 64, 128, 128, 256, 256, 256, 256, 512, 512, 512, 512};
const int kCout[NL] = {64, 64, 128, 128, 256, 256, 256, 256, 512, 512, 512, 512, 512};
const int kScale[NL] = {0, 0, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4};      // log2 of the spatial divisor
const int kPoolAfter[4] = {1, 3, 7, 11};
// reference output index (neural_nets.py:22) -> conv layer
const int kTapLayer[6] = {0, 2, 4, 8, 9, 12};
// the reference's default taps (neural_nets.py:25-28): content 4 = ReLU(conv4_2), style 0, 1, 2, 3, 5 =
// relu1_1, relu2_1, relu3_1, relu4_1, relu5_1; a context's own taps (nst_job_set_taps) live in nst_ctx::taps
constexpr int kMaxStyle = 6;

thread_local std::string g_err;

struct ActSet {                 // activations of one forward pass, NHWC
    int h[NL], w[NL];
    float* act[NL] = {};
    float* pool[4] = {};
    float* splitk = nullptr;     // split-K partial sums of the small-spatial conv layers
    size_t splitk_floats = 0;
    unsigned* bits[NL] = {};     // ReLU bit-masks ([h*w][C/32] words) of the layers whose mask the backward reads
    bool bits_valid[NL] = {};    // written by the last forward pass (false when that layer ran split-K / fp32)
    bool pooled[4] = {};         // pool[k] already produced by the conv epilogue of the last forward pass
    // absmax records for the fp16-piece convolutions (conv_h2.hip): AMAX_IDS x NST_AMAX_SLOTS words.
    // ids: act[l] -> l; the Gram factor S of style slot q -> NL + q (6 slots); the gradient w.r.t. the pre-ReLU output
    // of layer l (or a bound of it: the pooled gradient it was un-pooled from) -> NL + 6 + l
    unsigned* amax = nullptr;
    // arg-max codes of the four max-pools (average pooling: the multi-hot ReLU-on codes), written by the fused pooling of the
    // f16x2 forward launches and read by the un-pooling loader of the input-gradient launch below each pool: [H/2*W/2][C/32][4] words
    unsigned* pcode[4] = {};
    size_t bytes = 0;
};
constexpr int AMAX_IDS = 2 * NST_VGG19_CONVS + kMaxStyle;
inline unsigned* amax_act(const ActSet& a, int l) { return a.amax + (size_t)l * NST_AMAX_SLOTS; }
inline unsigned* amax_S(const ActSet& a, int q) { return a.amax + (size_t)(NST_VGG19_CONVS + q) * NST_AMAX_SLOTS; }
inline unsigned* amax_grad(const ActSet& a, int l) { return a.amax + (size_t)(NST_VGG19_CONVS + kMaxStyle + l) * NST_AMAX_SLOTS; }

// The feature maps a job's losses read (nst_job_set_taps), as conv layers.  The reference's LossBuilder keeps the indices
// of enumerate(features) that are `in` its lists (neural_style_transfer.py:48-64): order and repeats do not matter, the
// style term is the mean over the distinct maps kept (:104-106).
struct Taps {
    int content = 9;                           // conv layer of the content map
    int style[kMaxStyle] = {0, 2, 4, 8, 12};   // conv layers of the style maps, ascending (style slot q -> style[q])
    int nstyle = 5;
    int top = 12;                              // the deepest layer any loss reads: the forward stops, the backward starts there
    int use_relu = 1;                          // 0: tap 5 is conv5_1 BEFORE its ReLU (neural_nets.py:24-26 with use_relu=False)
    bool is_default = true;
    int style_slot(int l) const {
        for (int q = 0; q < nstyle; ++q) if (style[q] == l) return q;
        return -1;
    }
    // the top layer's gradient goes through its ReLU mask unless it is the pre-ReLU conv5_1
    bool top_mask() const { return use_relu || top != NST_VGG19_CONVS - 1; }
};

enum KClass { K_CONV3 = 0, K_GRAM = 1, K_CONV1 = 2, K_OTHER = 3, K_NCLASS = 4 };

struct TimedLaunch { hipEvent_t a, b; int cls; double flops; int tag[6]; double mfma_factor; };      // mfma_factor: executed matrix-pipe FLOPs per algorithmic FLOP (< 0: the arithmetic mode's)

struct LevelWs {
    int h = 0, w = 0;
    ActSet acts;
    float* gbuf[2] = {};
    size_t gbuf_floats = 0;
    float* xl = nullptr;        // level image (levels >= 1), planar
    float* gxl = nullptr;       // its gradient (levels >= 1), planar
    size_t xl_floats = 0;       // channels (nst_job_set_color) x h x w
    float* content_t = nullptr; // NHWC target ReLU(conv4_2)
    size_t content_n = 0;
    float* gram_t[kMaxStyle] = {};
    float* S[kMaxStyle] = {};
    unsigned short* S_bf[kMaxStyle] = {};
    float* gram_part = nullptr;
    size_t gram_part_floats = 0;
    double* style_partial[kMaxStyle] = {};
    int tap_c[kMaxStyle] = {};  // channels of the style map each Gram buffer was sized for
    double* content_partial = nullptr;
    double* tv_partial = nullptr;
    float* tv_means = nullptr;
    bool targets = false;
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;
};

}  // namespace

struct nst_ctx {
    int device = 0;
    std::string err;
    float* wf[NL] = {};
    float* wd[NL] = {};
    void* wf_bf[NL] = {};       // the same weights cut into 3 bf16 pieces (conv_bf3.hip layout)
    void* wd_bf[NL] = {};
    void* wd_wino[NL] = {};     // the same for the input-gradient launches
    float wd_wino_inv[NL] = {};
    void* wf_wino[NL] = {};     // conv_wino.hip's transformed forward weights (nst_options.h2_winograd), true = pieces * wf_wino_inv
    float wf_wino_inv[NL] = {};
    int winograd = 0;           // nst_options.h2_winograd
    void* wf_h2[NL] = {};       // ... cut into 2 scaled fp16 pieces (conv_h2.hip layout), true = pieces * w*_h2_inv
    void* wd_h2[NL] = {};
    float wf_h2_inv[NL] = {};
    float wd_h2_inv[NL] = {};
    // 3x3 convs: 2 = fp16 pipe, 2 scaled pieces per operand (3 MFMAs per product block; default),
    //            1 = bf16 pipe, 3 exact pieces (6 MFMAs), 0 = fp32 MFMA
    int conv_mode = 2;
    int band_rows = 0;          // nst_options.h2_band_rows (0 = bands only for tensors beyond 4 GiB)
    int lbfgs_gram = 1;         // nst_options.lbfgs_gram
    int mfma16 = 1;             // nst_options.h2_mfma16
    int wg256 = 0;              // nst_options.h2_wg256
    int tile_rows = 0;          // nst_options.h2_tile_rows
    int gram_overlap = 0;       // nst_options.gram_overlap
    int persist = 1;            // nst_options.h2_persist
    int level_split = 0;        // nst_options.level_split
    hipStream_t side = nullptr; // the Gram launches of the shallow style layers run here, under the deeper forward convolutions
    hipEvent_t side_fork = nullptr, side_join = nullptr;
    hipStream_t tail_stream = nullptr;   // the stream the tail event was last recorded on (see enter())
    bool tail_set = false;
    hipEvent_t tail = nullptr;  // recorded after the last launch that touches context-owned memory: what
                                // nst_job_configure / nst_ctx_destroy wait for instead of the whole device
    int batched = 1;            // 1: one conv launch per layer covering every pyramid level (one stream)
    // hipGraph of the closure: captured the second time the same (buffers, weights, mask) are seen
    int use_graph = 0;          // measured: no gain (the host already runs ~16 ms ahead of the GPU); NST_GRAPH=1 enables
    hipStream_t gstream = nullptr;          // capture stream (capture on the legacy stream is not allowed)
    hipGraphExec_t gexec = nullptr;
    struct GraphKey { const float* x; float* grad; float* losses; float cw, sw, tvw; unsigned mask; } gkey{}, glast{};
    float* bias[NL] = {};
    float* w11k = nullptr;      // [28][64]
    float* w11d = nullptr;      // [9][64][4]
    int levels = 0;
    Taps taps;                  // nst_job_set_taps
    int channels = 3;           // nst_job_set_color: 3 = RGB, 1 = luminance (the optimised image is u = 255 Y)
    int pool_avg = 0;           // nst_job_set_pooling: 1 = the four pools average their windows (include/nst_hip.h has the definition)
    // bumped on entry to every call that changes what a closure computes (configure, taps, colour, pooling, targets), failure paths
    // included: an optimiser's remembered closure result is valid only under the epoch it was made in (nst_opt.cpp)
    unsigned long long closure_epoch = 0;
    double* color_scratch = nullptr;   // nst_color_stats: COLOR_BLOCKS * 9 partials | mean (3) | cov (9), made on first use
    LevelWs lv[NST_MAX_LEVELS];
    hipEvent_t fork = nullptr;
    size_t bytes = 0;
    bool single_stream = false;
    // timing
    int timing = 0;
    hipEvent_t t0 = nullptr, t1 = nullptr;
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used = 0;
    std::vector<TimedLaunch> timed;
    bool timed_valid = false;
    // accumulated over closures since the last reset (timing mode 2)
    double acc_ms[4] = {0, 0, 0, 0};
    double acc_flops[4] = {0, 0, 0, 0};
    double acc_mfma[4] = {0, 0, 0, 0};          // executed matrix-pipe FLOPs of the timed launches
    long acc_launches[4] = {0, 0, 0, 0};
    double acc_closure_ms = 0;
    long acc_closures = 0;
    long acc_sampled = 0;       // closures whose launches carried event pairs (timing mode 4 samples one in four)
    long closure_seq = 0;
    bool sample_now = true;
};

namespace {

int fail(nst_ctx* ctx, int code, const std::string& msg) {
    if (ctx) ctx->err = msg; else g_err = msg;
    return code;
}

#define HIPCHK(ctx, expr)                                                                         \
    do {                                                                                          \
        hipError_t _e = (expr);                                                                   \
        if (_e != hipSuccess)                                                                     \
            return fail(ctx, NST_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));       \
    } while (0)

#define NSTCHK(expr)                 \
    do {                             \
        int _r = (expr);             \
        if (_r != NST_OK) return _r; \
    } while (0)

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

}  // namespace
// hipMemset on device memory is enqueued on the NULL stream and returns before it has run: with another context's work
// queued there (two jobs per GPU is the scheduler's default) it lands AFTER the first kernels of this context, which run on
// the caller's non-blocking stream - and wipes what they wrote (absmax records -> a zero scale -> NaN targets; Adam
// moments; the packed loss rows).  Set-up-time zero fills therefore run on a stream of their own and are waited for:
// nothing of a context rides on the null stream.
extern "C" int nst_internal_zero_now(void* p, size_t bytes) {
    hipStream_t zs = nullptr;
    hipError_t e = hipStreamCreateWithFlags(&zs, hipStreamNonBlocking);
    if (e != hipSuccess) return 1;
    e = hipMemsetAsync(p, 0, bytes, zs);
    if (e == hipSuccess) e = hipStreamSynchronize(zs);
    (void)hipStreamDestroy(zs);
    return e == hipSuccess ? 0 : 1;
}
namespace {
int dev_alloc(nst_ctx* ctx, void** p, size_t bytes) {
    if (bytes == 0) bytes = 16;
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) return fail(ctx, NST_E_NOMEM, std::string("hipMalloc(") + std::to_string(bytes) + "): " + hipGetErrorString(e));
    poison_if_asked(*p, bytes);
    ctx->bytes += bytes;
    return NST_OK;
}
template <typename T>
int dev_alloc_t(nst_ctx* ctx, T** p, size_t count) { return dev_alloc(ctx, reinterpret_cast<void**>(p), count * sizeof(T)); }

void dev_free(void* p) { if (p) (void)hipFree(p); }

int alloc_acts(nst_ctx* ctx, ActSet& a, int h, int w) {
    a.bytes = 0;
    for (int l = 0; l < NL; ++l) {
        a.h[l] = h >> kScale[l];
        a.w[l] = w >> kScale[l];
        if (a.h[l] < 1 || a.w[l] < 1) return fail(ctx, NST_E_ARG, "image too small for VGG19 (needs >= 16 px per side)");
        const size_t n = (size_t)a.h[l] * a.w[l] * kCout[l];
        NSTCHK(dev_alloc_t(ctx, &a.act[l], n));
        a.bytes += n * 4;
    }
    for (int k = 0; k < 4; ++k) {
        const int l = kPoolAfter[k];
        const size_t n = (size_t)(a.h[l] / 2) * (a.w[l] / 2) * kCout[l];
        NSTCHK(dev_alloc_t(ctx, &a.pool[k], n));
        a.bytes += n * 4;
        NSTCHK(dev_alloc_t(ctx, &a.pcode[k], n / 8));          // n / 32 channel groups x 4 words
        a.bytes += n / 8 * 4;
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
        NSTCHK(dev_alloc_t(ctx, &a.bits[m], nw));
        a.bytes += nw * 4;
    }
    NSTCHK(dev_alloc_t(ctx, &a.amax, (size_t)AMAX_IDS * NST_AMAX_SLOTS));
    a.bytes += (size_t)AMAX_IDS * NST_AMAX_SLOTS * 4;
    if (nst_internal_zero_now(a.amax, (size_t)AMAX_IDS * NST_AMAX_SLOTS * 4)) return fail(ctx, NST_E_HIP, "hipMemset failed");
    a.splitk_floats = need;
    if (need) {
        NSTCHK(dev_alloc_t(ctx, &a.splitk, need));
        a.bytes += need * 4;
    }
    return NST_OK;
}
void free_acts(nst_ctx* ctx, ActSet& a) {
    for (int l = 0; l < NL; ++l) { dev_free(a.act[l]); a.act[l] = nullptr; }
    for (int k = 0; k < 4; ++k) { dev_free(a.pool[k]); a.pool[k] = nullptr; dev_free(a.pcode[k]); a.pcode[k] = nullptr; }
    dev_free(a.splitk); a.splitk = nullptr; a.splitk_floats = 0;
    dev_free(a.amax); a.amax = nullptr;
    for (int l = 0; l < NL; ++l) { dev_free(a.bits[l]); a.bits[l] = nullptr; a.bits_valid[l] = false; }
    if (ctx->bytes >= a.bytes) ctx->bytes -= a.bytes;
    a.bytes = 0;
}

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
void make_h2(const float* w, int taps, int rows, int K, std::vector<uint16_t>& out, float* inv) {
    const int kc = (rows % 128 == 0 && K > NST_H2_SHORTK_CIN) ? 32 : 16;
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

int pool_index_after(int l) {
    for (int k = 0; k < 4; ++k) if (kPoolAfter[k] == l) return k;
    return -1;
}

// ---- timed launches ---------------------------------------------------------------------------
struct Timer {
    nst_ctx* ctx; hipStream_t s; bool on; size_t slot;
    Timer(nst_ctx* c, hipStream_t st, int cls, double flops, int t0 = 0, int t1 = 0, int t2 = 0, int t3 = 0, int t4 = 0,
          int t5 = 0)
        : ctx(c), s(st), on(false), slot(0) {
        if (c->timing >= 2 && (c->timing < 3 || cls == K_CONV3) && c->sample_now && c->ev_used + 2 <= c->ev_pool.size()) {
            on = true;
            TimedLaunch t{c->ev_pool[c->ev_used], c->ev_pool[c->ev_used + 1], cls, flops, {t0, t1, t2, t3, t4, t5}, -1.0};
            c->ev_used += 2;
            slot = c->timed.size();
            c->timed.push_back(t);
            (void)hipEventRecord(t.a, st);
        }
    }
    ~Timer() { if (on) (void)hipEventRecord(ctx->timed[slot].b, s); }
    // a launch whose matrix-pipe work per algorithmic FLOP differs from its arithmetic mode's (the Winograd form: 2/3 of it)
    void mfma_factor(double f) { if (on) ctx->timed[slot].mfma_factor = f; }
};

double conv_flops(int h, int w, int cin, int cout, int taps) { return 2.0 * h * w * (double)cin * cout * taps; }

// the bf16-piece kernels address with 32-bit buffer offsets: tensors from 4 GiB up go to the fp32 kernel
bool uses_pieces(const nst_ctx* ctx, const ConvParams& p) {
    if (ctx->conv_mode == 2) return true;           // launch_conv_h2 runs larger tensors in row bands
    return ctx->conv_mode != 0 && (size_t)p.H * p.W * p.Cin * 4 < 0xFFFFFF00ull;
}
// 3x3 conv dispatch by mode; whatever kernel runs, the absmax record of the output is produced when asked for
hipError_t launch_conv3(nst_ctx* ctx, const ConvParams& p, hipStream_t s) {
    if (uses_pieces(ctx, p)) return ctx->conv_mode == 2 ? launch_conv_h2(p, s) : launch_conv_bf3(p, s);
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

// ---- network forward ----------------------------------------------------------------------------
// channels = 1: x is a luminance plane u, conv1_1 sees x_c = u - mean_c (nst_job_set_color)
int forward(nst_ctx* ctx, ActSet& a, const float* x, int h, int w, hipStream_t s, int last_layer = NL - 1, int channels = 3) {
    for (int l = 0; l < NL; ++l) a.bits_valid[l] = false;
    for (int k = 0; k < 4; ++k) a.pooled[k] = false;
    const bool h2 = ctx->conv_mode == 2;
    if (h2) HIPCHK(ctx, launch_zero(a.amax, (size_t)(NL + kMaxStyle) * NST_AMAX_SLOTS, s));     // act + S records
    {
        Timer t(ctx, s, K_CONV1, conv_flops(h, w, 3, 64, 9));
        unsigned* bits = ctx->conv_mode ? a.bits[0] : nullptr;
        HIPCHK(ctx, launch_conv1_1_fwd(x, h, w, ctx->w11k, ctx->bias[0], a.act[0], bits, h2 ? amax_act(a, 0) : nullptr, s, channels));
        a.bits_valid[0] = bits != nullptr;
    }
    for (int l = 1; l <= last_layer; ++l) {
        const int pk = pool_index_after(l - 1);
        const float* in = (pk >= 0) ? a.pool[pk] : a.act[l - 1];
        ConvParams p{};
        p.in = in; p.wt = ctx->wf[l]; p.bias = ctx->bias[l]; p.addend = nullptr; p.mask = nullptr; p.out = a.act[l];
        p.H = a.h[l]; p.W = a.w[l]; p.Cin = kCin[l]; p.Cout = kCout[l];
        p.relu = (l == NL - 1 && !ctx->taps.use_relu) ? 0 : 1;      // conv5_1 before its ReLU (use_relu = 0)
        p.pool_avg = ctx->pool_avg;
        p.partial = a.splitk; p.partial_floats = a.splitk_floats; p.wt_bf = ctx->wf_bf[l];
        if (h2) {
            p.wt_h2 = ctx->wf_h2[l]; p.wt_h2_inv = ctx->wf_h2_inv[l];
            p.amax_in = amax_act(a, l - 1);       // the pooled map's maximum is its source's
            p.amax_out = amax_act(a, l);
            p.band_rows = ctx->band_rows; p.mfma16 = ctx->mfma16; p.wg256 = ctx->wg256; p.tile_rows = ctx->tile_rows;
        }
        const int pa = pool_index_after(l);
        const bool fuse = bf3_unsplit(ctx, p);        // the epilogue extras exist in the unsplit bf3 kernel only
        if (fuse) {
            p.bits_out = a.bits[l];                   // nullptr for layers whose mask nobody reads
            if (pa >= 0 && l < last_layer) p.pool_out = a.pool[pa];
        }
        {
            Timer t(ctx, s, K_CONV3, conv_flops(p.H, p.W, p.Cin, p.Cout, 9), p.H, p.W, p.Cin, p.Cout, 9, l);
            HIPCHK(ctx, launch_conv3(ctx, p, s));
        }
        a.bits_valid[l] = fuse && a.bits[l] != nullptr;
        if (pa >= 0 && l < last_layer) {
            if (p.pool_out) {
                a.pooled[pa] = true;
            } else {
                Timer t(ctx, s, K_OTHER, 0);
                HIPCHK(ctx, (ctx->pool_avg ? launch_avgpool_fwd : launch_maxpool_fwd)(a.act[l], a.h[l], a.w[l], kCout[l], a.pool[pa], s));
            }
        }
    }
    return NST_OK;
}

// gradient injected at a tap layer, w.r.t. its post-ReLU activation
struct Inject {
    const float* S = nullptr;        // Gram backward: dF = F * S (1x1 conv of the activation itself)
    const void* S_bf = nullptr;      // the same S cut into bf16 pieces (conv_bf3 weight layout), if available
    const unsigned* S_amax = nullptr; // absmax record of S (conv_h2), if available
    const float* direct = nullptr;   // or a ready NHWC gradient
    bool content = false;            // or the content MSE gradient (closure only)
};

struct ContentJob { const float* target; size_t n; float coef; double* partial; };

// Backward through the network down to the planar image gradient gx (overwritten).
// inj[l] describes what enters at conv layer l; gbuf: two NHWC scratch buffers of the largest size.  The chain starts at
// layer `top` (nothing above it is read); `top_mask` = false: the top map is pre-ReLU (its gradient passes unmasked).
// channels = 1: gx is the gradient of a luminance plane (the sum over the three channels)
int backward(nst_ctx* ctx, ActSet& a, const Inject* inj, const ContentJob* cj, float* gbuf0, float* gbuf1, float* gx,
             int h, int w, hipStream_t s, int top = NL - 1, bool top_mask = true, int channels = 3) {
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
        if (inj[l].S) {
            // (the content gradient, if any, as the addend of the 1x1 Gram launch)
            ConvParams p{};
            p.in = a.act[l]; p.wt = inj[l].S; p.out = cur; p.mask = top_mask ? a.act[l] : nullptr;
            p.addend = content ? oth : nullptr;
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
        p.in = cur; p.wt = ctx->wd[l]; p.out = oth;
        p.H = a.h[l]; p.W = a.w[l]; p.Cin = kCout[l]; p.Cout = kCin[l];
        p.partial = a.splitk; p.partial_floats = a.splitk_floats; p.wt_bf = ctx->wd_bf[l];
        if (h2) {
            p.wt_h2 = ctx->wd_h2[l]; p.wt_h2_inv = ctx->wd_h2_inv[l];
            p.amax_in = amax_grad(a, l);
            p.amax_out = amax_grad(a, l - 1);     // when un-pooled next, this bounds the un-pooled gradient too
            p.band_rows = ctx->band_rows; p.mfma16 = ctx->mfma16; p.wg256 = ctx->wg256; p.tile_rows = ctx->tile_rows;
        }
        if (pk >= 0) {
            // (average pooling: the un-pooled gradient is a quarter of the pooled one, so the pooled gradient's absmax would
            // describe a tensor four times what the next launch reads - that launch's record is taken after the un-pooling)
            const bool avg = ctx->pool_avg != 0;
            if (avg) p.amax_out = nullptr;
            {
                Timer t(ctx, s, K_CONV3, conv_flops(p.H, p.W, p.Cin, p.Cout, 9), p.H, p.W, p.Cin, p.Cout, 9, -l);
                HIPCHK(ctx, launch_conv3(ctx, p, s));
            }
            // oth = g(pool[pk]); un-pool through act[l-1] with its ReLU mask -> cur
            Timer t(ctx, s, K_OTHER, 0);
            HIPCHK(ctx, (avg ? launch_avgpool_bwd_relu : launch_maxpool_bwd_relu)(a.act[l - 1], oth, a.h[l - 1], a.w[l - 1], kCout[l - 1], cur, s));
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
            if (in.S && fuse && (h2 ? in.S_amax != nullptr : in.S_bf != nullptr)) {
                // Gram backward rides on this launch as a second K source: acc += act[m] * S
                p.in2 = a.act[m]; p.Cin2 = kCout[m]; p.wt2_bf = in.S_bf;
                p.wt2_f32 = in.S; p.amax_in2 = amax_act(a, m); p.amax_w2 = in.S_amax;
                extra_flops = conv_flops(a.h[m], a.w[m], kCout[m], kCout[m], 1);
            } else if (in.S) {
                ConvParams q{};
                q.in = a.act[m]; q.wt = in.S; q.out = oth; q.addend = p.addend;
                q.H = a.h[m]; q.W = a.w[m]; q.Cin = kCout[m]; q.Cout = kCout[m];
                Timer t(ctx, s, K_GRAM, conv_flops(q.H, q.W, q.Cin, q.Cout, 1));
                HIPCHK(ctx, launch_conv_mfma(q, 1, s));
                p.addend = oth;
            }
            if (fuse && a.bits_valid[m]) p.bits_in = a.bits[m];
            else p.mask = a.act[m];
            {
                Timer t(ctx, s, K_CONV3, conv_flops(p.H, p.W, p.Cin, p.Cout, 9) + extra_flops, p.H, p.W, p.Cin, p.Cout, 9, -l);
                HIPCHK(ctx, launch_conv3(ctx, p, s));
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

// f_amax (nullable): absmax record of f_nhwc; with it the partial products run on the fp16 pipe
int gram_of(nst_ctx* ctx, const float* f_nhwc, size_t N, int C, const unsigned* f_amax, float divisor, float* part, const float* target,
            float coef, float* gram_out, float* S, unsigned short* S_bf, unsigned* S_amax, double* mse_partial,
            hipStream_t s) {
    const int ns = gram_nsplit(C, N);
    {
        Timer t(ctx, s, K_GRAM, 2.0 * (double)N * C * C);
        HIPCHK(ctx, launch_gram_partial(f_nhwc, N, C, ns, f_amax, part, s));
    }
    Timer t(ctx, s, K_OTHER, 0);
    HIPCHK(ctx, launch_gram_finish(part, gram_nslabs(C, ns), C, divisor, target, coef, gram_out, S, S_bf, S_amax,
                                   mse_partial, s));
    return NST_OK;
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
size_t gram_part_floats_for(const Taps& tp, int h, int w) { return gram_part_offset(tp, h, w, tp.nstyle); }

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

// `fork_sw` >= 0 (f16x2 closure, nst_options.gram_overlap): once relu3_1 is written, the Gram matrices of relu1_1, relu2_1 and
// relu3_1 - HBM-bound streams over 85 % of the style bytes - are launched on the context's side stream, where they run
// under the MFMA-bound convolutions of conv3_2 ... conv5_1 instead of after them; the caller joins before the backward.
int batched_gram(nst_ctx* ctx, const int* lv, int n, float sw, hipStream_t s, unsigned qmask);
int batched_forward(nst_ctx* ctx, const float* const* xi, const int* lv, int n, hipStream_t s, const Window* win, float fork_sw = -1.f) {
    const bool h2 = ctx->conv_mode == 2;
    const int top = ctx->taps.top;
    for (int k = 0; k < n; ++k) {
        LevelWs& L = ctx->lv[lv[k]];
        ActSet& a = L.acts;
        for (int l = 0; l < NL; ++l) a.bits_valid[l] = false;
        for (int q = 0; q < 4; ++q) a.pooled[q] = false;
        if (h2) HIPCHK(ctx, launch_zero(a.amax, (size_t)AMAX_IDS * NST_AMAX_SLOTS, s));
        {
            Timer t(ctx, s, K_OTHER, 0);
            HIPCHK(ctx, launch_tv_partial(xi[lv[k]], ctx->channels, L.h, L.w, L.tv_partial, s, win ? win->row0 : 0, win ? win->rows : 0));
        }
        Timer t(ctx, s, K_CONV1, conv_flops(L.h, L.w, 3, 64, 9));
        HIPCHK(ctx, launch_conv1_1_fwd(xi[lv[k]], L.h, L.w, ctx->w11k, ctx->bias[0], a.act[0], a.bits[0],
                                       h2 ? amax_act(a, 0) : nullptr, s, ctx->channels));
        a.bits_valid[0] = true;
    }
    for (int l = 1; l <= top; ++l) {
        const int pk = pool_index_after(l - 1), pa = pool_index_after(l);
        ConvBatch b{};
        b.n = n; b.wt_bf = ctx->wf_bf[l]; b.bias = ctx->bias[l]; b.Cin = kCin[l]; b.Cout = kCout[l];
        // conv5_1 before its ReLU (use_relu = 0): the Winograd launch takes its general epilogue (MODE 0), which honours relu = 0
        b.relu = (l == NL - 1 && !ctx->taps.use_relu) ? 0 : 1;
        b.wt_h2 = ctx->wf_h2[l]; b.wt_h2_inv = ctx->wf_h2_inv[l]; b.mfma16 = ctx->mfma16; b.wg256 = ctx->wg256; b.tile_rows = ctx->tile_rows; b.persist = ctx->persist;
        b.wt_wino = ctx->wf_wino[l]; b.wt_wino_inv = ctx->wf_wino_inv[l];
        b.pool_avg = ctx->pool_avg;
        double flops = 0;
        for (int k = 0; k < n; ++k) {
            ActSet& a = ctx->lv[lv[k]].acts;
            ConvImage& im = b.img[k];
            im.in = (pk >= 0) ? a.pool[pk] : a.act[l - 1];
            im.out = a.act[l]; im.H = a.h[l]; im.W = a.w[l];
            im.bits_out = a.bits[l];
            im.pool_out = (pa >= 0) ? a.pool[pa] : nullptr;
            im.pcode_out = (pa >= 0 && h2) ? a.pcode[pa] : nullptr;
            a.bits_valid[l] = a.bits[l] != nullptr;
            if (pa >= 0) a.pooled[pa] = true;
            im.amax_in = amax_act(a, l - 1); im.amax_out = amax_act(a, l);
            flops += conv_flops(im.H, im.W, b.Cin, b.Cout, 9);
        }
        {
            Timer t(ctx, s, K_CONV3, flops, b.img[0].H, b.img[0].W, b.Cin, b.Cout, 9, l);
            if (h2 && b.wt_wino && conv_wino_eligible(b)) { t.mfma_factor(2.0); HIPCHK(ctx, launch_conv_wino_batch(b, s)); }
            else HIPCHK(ctx, h2 ? launch_conv_h2_batch(b, s) : launch_conv_bf3_batch(b, s));
        }
        if (l == 4 && fork_sw >= 0.f && ctx->side) {
            HIPCHK(ctx, hipEventRecord(ctx->side_fork, s));
            HIPCHK(ctx, hipStreamWaitEvent(ctx->side, ctx->side_fork, 0));
            NSTCHK(batched_gram(ctx, lv, n, fork_sw, ctx->side, 0x07u));
            HIPCHK(ctx, hipEventRecord(ctx->side_join, ctx->side));
        }
    }
    return NST_OK;
}

// ---- style losses: Gram matrices, S = d loss / d G folded for the backward
int batched_gram(nst_ctx* ctx, const int* lv, int n, float sw, hipStream_t s, unsigned qmask) {
    const bool h2 = ctx->conv_mode == 2;
    if (h2) {
        // every (level, style layer) pair in two partial launches (one per tile shape) and one finish launch
        const int per = std::max(1, NST_GRAM_BATCH_MAX / ctx->taps.nstyle);      // levels per launch (3 with five style maps)
        for (int k0 = 0; k0 < n; k0 += per) {
            GramBatch gb{};
            double flops = 0;
            for (int k = k0; k < n && k < k0 + per; ++k) {
                LevelWs& L = ctx->lv[lv[k]];
                for (int q = 0; q < ctx->taps.nstyle; ++q) {
                    if (!((qmask >> q) & 1u)) continue;
                    const int l = ctx->taps.style[q];
                    const int C = kCout[l];
                    const size_t N = (size_t)L.acts.h[l] * L.acts.w[l];
                    const double chw = (double)C * (double)N;
                    GramItem& it = gb.it[gb.n++];
                    it.f = L.acts.act[l]; it.N = N; it.C = C; it.amax = amax_act(L.acts, l);
                    it.part = L.gram_part + gram_part_offset(ctx->taps, L.h, L.w, q);
                    it.divisor = (float)chw; it.target = L.gram_t[q];
                    it.coef = (float)((double)sw * 4.0 / ((double)ctx->taps.nstyle * (double)C * C * chw));
                    it.gram_out = nullptr; it.S = L.S[q]; it.S_bf = L.S_bf[q]; it.S_amax = amax_S(L.acts, q);
                    it.mse_partial = L.style_partial[q];
                    flops += 2.0 * (double)N * C * C;
                }
            }
            if (gb.n == 0) continue;
            Timer t(ctx, s, K_GRAM, flops);
            HIPCHK(ctx, launch_gram_batch(gb, s));
        }
    }
    for (int k = 0; k < n && !h2; ++k) {
        LevelWs& L = ctx->lv[lv[k]];
        for (int q = 0; q < ctx->taps.nstyle; ++q) {
            const int l = ctx->taps.style[q];
            const int C = kCout[l];
            const size_t N = (size_t)L.acts.h[l] * L.acts.w[l];
            const double chw = (double)C * (double)N;
            const float coef = (float)((double)sw * 4.0 / ((double)ctx->taps.nstyle * (double)C * C * chw));
            NSTCHK(gram_of(ctx, L.acts.act[l], N, C, nullptr, (float)chw, L.gram_part, L.gram_t[q], coef, nullptr, L.S[q],
                           L.S_bf[q], nullptr, L.style_partial[q], s));
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
            HIPCHK(ctx, launch_mse_grad(a.act[m] + off, L.content_t + off, cnt, (float)((double)cw * 2.0 / n_all),
                                        dst + off, L.content_partial, s));
        } else {
            HIPCHK(ctx, launch_mse_grad(a.act[m], L.content_t, L.content_n,
                                        (float)((double)cw * 2.0 / (double)L.content_n), dst, L.content_partial, s));
        }
        return NST_OK;
    };
    if (top_content)
        for (int k = 0; k < n; ++k) NSTCHK(content_grad(k, oth[k]));
    if (h2 && top_q >= 0) {
        // top of the chain: g(pre-ReLU of the top map) = mask(act * S (+ content gradient)) - the second K source of the
        // fp16 kernel on its own (no 3x3 part), one launch for all levels; its epilogue adds the content gradient (when the
        // top map is the content map too), applies the ReLU mask (not for the pre-ReLU conv5_1) and records the absmax
        const int l = top;
        ConvBatch b{};
        b.n = n; b.Cin = 0; b.Cout = kCout[l]; b.Cin2 = kCout[l]; b.relu = 0; b.wt_h2_inv = 1.f; b.mfma16 = ctx->mfma16; b.wg256 = ctx->wg256; b.tile_rows = ctx->tile_rows; b.persist = ctx->persist;
        double flops = 0;
        for (int k = 0; k < n; ++k) {
            LevelWs& L = ctx->lv[lv[k]];
            ActSet& a = L.acts;
            ConvImage& im = b.img[k];
            im.out = cur[k]; im.H = a.h[l]; im.W = a.w[l];
            im.in2 = a.act[l]; im.wt2_f32 = L.S[top_q]; im.amax_in2 = amax_act(a, l); im.amax_w2 = amax_S(a, top_q);
            im.bits_in = tp.top_mask() ? a.bits[l] : nullptr; im.amax_out = amax_grad(a, l);
            im.addend = top_content ? oth[k] : nullptr;
            if (win) { im.in2_row0 = win_r0(*win, kScale[l]); im.in2_rows = win_nr(*win, kScale[l]); }
            flops += conv_flops(im.H, im.W, b.Cin2, b.Cout, 1);
        }
        Timer t(ctx, s, K_GRAM, flops);
        HIPCHK(ctx, launch_conv_h2_batch(b, s));
    }
    for (int k = 0; k < n && !(h2 && top_q >= 0); ++k) {
        LevelWs& L = ctx->lv[lv[k]];
        ActSet& a = L.acts;
        const int l = top;
        const size_t cnt = (size_t)a.h[l] * a.w[l] * kCout[l];
        if (top_q >= 0) {
            ConvParams p{};
            p.in = a.act[l]; p.wt = L.S[top_q]; p.out = cur[k]; p.mask = tp.top_mask() ? a.act[l] : nullptr;
            p.addend = top_content ? oth[k] : nullptr;
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
        b.n = n; b.wt_bf = ctx->wd_bf[l]; b.bias = nullptr; b.Cin = kCout[l]; b.Cout = kCin[l]; b.relu = 0;
        b.wt_h2 = ctx->wd_h2[l]; b.wt_h2_inv = ctx->wd_h2_inv[l]; b.mfma16 = ctx->mfma16; b.wg256 = ctx->wg256; b.tile_rows = ctx->tile_rows; b.persist = ctx->persist;
        b.wt_wino = ctx->wd_wino[l]; b.wt_wino_inv = ctx->wd_wino_inv[l];
        // f16x2: when a max-pool follows layer l, cur[] holds the gradient w.r.t. the POOLED map and this launch's
        // loader un-pools it through the arg-max code (no un-pool kernel, no full-size gradient round trip)
        const int pl = pool_index_after(l);
        b.unpool = (h2 && pl >= 0) ? 1 : 0;
        // average pooling: every position whose code bit is on gets a QUARTER of the pooled gradient.  The loader hands the
        // pooled gradient through as it is (same loads, same selects, a multi-hot code) and the 1/4 rides on the scale the
        // launch multiplies its accumulators by: exact (a power of two), and the second K source - re-expressed in the main
        // source's scale through the same factor - comes out unchanged.  The launch records the absmax of what it stores.
        if (b.unpool && ctx->pool_avg) { b.wt_h2_inv *= 0.25f; b.wt_wino_inv *= 0.25f; }
        b.Cin2 = (pk < 0 && style_q >= 0) ? kCout[m] : 0;
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
            if (style_q >= 0) {
                im.in2 = a.act[m]; im.wt2_bf = L.S_bf[style_q];
                im.wt2_f32 = L.S[style_q]; im.amax_in2 = amax_act(a, m); im.amax_w2 = amax_S(a, style_q);
                if (win) { im.in2_row0 = win_r0(*win, kScale[m]); im.in2_rows = win_nr(*win, kScale[m]); }
                flops += conv_flops(a.h[m], a.w[m], kCout[m], kCout[m], 1);
            }
            if (m == tp.content) {
                NSTCHK(content_grad(k, oth[k]));
                im.addend = oth[k];
            }
            im.bits_in = a.bits[m];
        }
        {
            Timer t(ctx, s, K_CONV3, flops, b.img[0].H, b.img[0].W, b.Cin, b.Cout, 9, -l);
            if (h2 && !win && b.wt_wino && conv_wino_eligible(b)) { t.mfma_factor(2.0); HIPCHK(ctx, launch_conv_wino_batch(b, s)); }
            else HIPCHK(ctx, h2 ? launch_conv_h2_batch(b, s) : launch_conv_bf3_batch(b, s));
        }
        for (int k = 0; k < n; ++k) {
            ActSet& a = ctx->lv[lv[k]].acts;
            if (pk >= 0 && !h2) {
                Timer t(ctx, s, K_OTHER, 0);
                HIPCHK(ctx, (ctx->pool_avg ? launch_avgpool_bwd_relu : launch_maxpool_bwd_relu)(a.act[l - 1], oth[k], a.h[l - 1], a.w[l - 1], kCout[l - 1], cur[k], s));
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
    }
    return NST_OK;
}

// `zero_mask`: the levels whose gradient this call clears when they are not in `level_mask` (levels another rank owns)
int closure_batched(nst_ctx* ctx, const float* const* xi, float* const* gi, unsigned level_mask, float cw, float sw,
                    float tvw, hipStream_t s, unsigned zero_mask = ~0u) {
    int lv[NST_MAX_LEVELS], n = 0;
    for (int i = 0; i < ctx->levels; ++i) {
        if ((level_mask >> i) & 1u) lv[n++] = i;
        else if ((zero_mask >> i) & 1u) HIPCHK(ctx, launch_zero(gi[i], (size_t)ctx->channels * ctx->lv[i].h * ctx->lv[i].w, s));
    }
    if (n == 0) return NST_OK;
    // (not while a hipGraph is being captured or replayed: the closure then stays on one stream)
    // (the overlap's split of the style maps - relu1_1 .. relu3_1 on the side stream - is the default taps')
    const bool overlap = ctx->gram_overlap && ctx->conv_mode == 2 && !ctx->use_graph && ctx->side != nullptr && ctx->taps.is_default;
    NSTCHK(batched_forward(ctx, xi, lv, n, s, nullptr, overlap ? sw : -1.f));
    NSTCHK(batched_gram(ctx, lv, n, sw, s, overlap ? 0x18u : (1u << ctx->taps.nstyle) - 1u));
    if (overlap) HIPCHK(ctx, hipStreamWaitEvent(s, ctx->side_join, 0));
    return batched_backward(ctx, xi, gi, lv, n, cw, tvw, s, nullptr, nullptr, 0, 0);
}

// the buffers whose size depends on the taps: content target, Gram targets / factors / partial sums, partial-Gram workspace
void free_tap_buffers(nst_ctx* ctx, LevelWs& L) {
    auto drop = [&](void* p, size_t bytes) { if (p) { dev_free(p); if (ctx->bytes >= bytes) ctx->bytes -= bytes; } };
    drop(L.content_t, L.content_n * 4); L.content_t = nullptr; L.content_n = 0;
    for (int k = 0; k < kMaxStyle; ++k) {
        const size_t C = (size_t)L.tap_c[k];
        drop(L.gram_t[k], C * C * 4); drop(L.S[k], C * C * 4); drop(L.S_bf[k], C * C * 6);
        drop(L.style_partial[k], (size_t)gram_finish_blocks((int)std::max<size_t>(C, 1)) * 8);
        L.gram_t[k] = nullptr; L.S[k] = nullptr; L.S_bf[k] = nullptr; L.style_partial[k] = nullptr; L.tap_c[k] = 0;
    }
    drop(L.gram_part, L.gram_part_floats * 4); L.gram_part = nullptr; L.gram_part_floats = 0;
}
int alloc_tap_buffers(nst_ctx* ctx, LevelWs& L) {
    const Taps& tp = ctx->taps;
    const int m = tp.content;
    L.content_n = (size_t)L.acts.h[m] * L.acts.w[m] * kCout[m];
    NSTCHK(dev_alloc_t(ctx, &L.content_t, L.content_n));
    for (int k = 0; k < tp.nstyle; ++k) {
        const int C = kCout[tp.style[k]];
        L.tap_c[k] = C;
        NSTCHK(dev_alloc_t(ctx, &L.gram_t[k], (size_t)C * C));
        NSTCHK(dev_alloc_t(ctx, &L.S[k], (size_t)C * C));
        NSTCHK(dev_alloc_t(ctx, &L.S_bf[k], (size_t)C * C * 3));
        NSTCHK(dev_alloc_t(ctx, &L.style_partial[k], gram_finish_blocks(C)));
    }
    L.gram_part_floats = gram_part_floats_for(tp, L.h, L.w);
    NSTCHK(dev_alloc_t(ctx, &L.gram_part, L.gram_part_floats));
    return NST_OK;
}

// the level image and its gradient (levels >= 1): their size follows the channel count (nst_job_set_color)
void free_level_image(nst_ctx* ctx, LevelWs& L) {
    for (float** p : {&L.xl, &L.gxl}) {
        if (*p) { dev_free(*p); if (ctx->bytes >= L.xl_floats * 4) ctx->bytes -= L.xl_floats * 4; }
        *p = nullptr;
    }
    L.xl_floats = 0;
}
int alloc_level_image(nst_ctx* ctx, LevelWs& L) {
    L.xl_floats = (size_t)ctx->channels * L.h * L.w;
    NSTCHK(dev_alloc_t(ctx, &L.xl, L.xl_floats));
    NSTCHK(dev_alloc_t(ctx, &L.gxl, L.xl_floats));
    return NST_OK;
}

void free_level(nst_ctx* ctx, LevelWs& L) {
    free_acts(ctx, L.acts);
    dev_free(L.gbuf[0]); dev_free(L.gbuf[1]); dev_free(L.xl); dev_free(L.gxl);
    free_tap_buffers(ctx, L);
    dev_free(L.content_partial); dev_free(L.tv_partial); dev_free(L.tv_means);
    if (L.stream) (void)hipStreamDestroy(L.stream);
    if (L.done) (void)hipEventDestroy(L.done);
    L = LevelWs();
}

// folds the event pairs of the previous closure into the accumulators (waits for them to complete)
int fold_timed(nst_ctx* ctx) {
    if (!ctx->timed_valid) return NST_OK;
    HIPCHK(ctx, hipEventSynchronize(ctx->t1));
    float ms = 0.f;
    HIPCHK(ctx, hipEventElapsedTime(&ms, ctx->t0, ctx->t1));
    ctx->acc_closure_ms += ms;
    ctx->acc_closures += 1;
    if (!ctx->timed.empty()) ctx->acc_sampled += 1;
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

int env_flag(const char* name, int dflt) {
    const char* e = getenv(name);
    if (!e || !e[0]) return dflt;
    return std::atoi(e);
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
    if (ctx->use_graph && hipStreamCreateWithFlags(&ctx->gstream, hipStreamNonBlocking) != hipSuccess) { ctx->err = "stream creation failed"; return bail(NST_E_HIP); }
    if (e != hipSuccess) { ctx->err = std::string("kernel attribute setup: ") + hipGetErrorString(e); return bail(NST_E_HIP); }

    std::vector<float> tmp;
    std::vector<uint16_t> tmp16;
    for (int l = 0; l < NL; ++l) {
        const int ci = kCin[l], co = kCout[l];
        const float* W = weights[l];   // [co][ci][3][3]
        if (dev_alloc_t(ctx, &ctx->bias[l], co) != NST_OK) return bail(NST_E_NOMEM);
        if (hipMemcpy(ctx->bias[l], biases[l], co * 4, hipMemcpyHostToDevice) != hipSuccess) { ctx->err = "bias upload failed"; return bail(NST_E_HIP); }
        if (l == 0) {
            tmp.assign(28 * 64, 0.f);
            for (int o = 0; o < 64; ++o)
                for (int c = 0; c < 3; ++c)
                    for (int t = 0; t < 9; ++t) tmp[(c * 9 + t) * 64 + o] = W[(o * 3 + c) * 9 + t];
            if (dev_alloc_t(ctx, &ctx->w11k, tmp.size()) != NST_OK) return bail(NST_E_NOMEM);
            if (hipMemcpy(ctx->w11k, tmp.data(), tmp.size() * 4, hipMemcpyHostToDevice) != hipSuccess) { ctx->err = "weight upload failed"; return bail(NST_E_HIP); }
            tmp.assign(9 * 64 * 4, 0.f);
            for (int t = 0; t < 9; ++t) {
                const int ky = 2 - t / 3, kx = 2 - t % 3;
                for (int o = 0; o < 64; ++o)
                    for (int c = 0; c < 3; ++c) tmp[(t * 64 + o) * 4 + c] = W[(o * 3 + c) * 9 + ky * 3 + kx];
            }
            if (dev_alloc_t(ctx, &ctx->w11d, tmp.size()) != NST_OK) return bail(NST_E_NOMEM);
            if (hipMemcpy(ctx->w11d, tmp.data(), tmp.size() * 4, hipMemcpyHostToDevice) != hipSuccess) { ctx->err = "weight upload failed"; return bail(NST_E_HIP); }
            continue;
        }
        const size_t n = (size_t)9 * ci * co;
        tmp.resize(n);
        // forward: wf[tap][co][ci]
        for (int t = 0; t < 9; ++t)
            for (int o = 0; o < co; ++o)
                for (int c = 0; c < ci; ++c) tmp[((size_t)t * co + o) * ci + c] = W[((size_t)o * ci + c) * 9 + t];
        if (dev_alloc_t(ctx, &ctx->wf[l], n) != NST_OK) return bail(NST_E_NOMEM);
        if (hipMemcpy(ctx->wf[l], tmp.data(), n * 4, hipMemcpyHostToDevice) != hipSuccess) { ctx->err = "weight upload failed"; return bail(NST_E_HIP); }
        // the 16-bit-piece copy of the active arithmetic only (a context is created per job: 0.24 s - tools/time_ctx_create.py - and ~200 MB of weight images)
        if (ctx->conv_mode == 1) {
            make_bf3(tmp.data(), 9, co, ci, tmp16);
            if (dev_alloc(ctx, &ctx->wf_bf[l], tmp16.size() * 2) != NST_OK) return bail(NST_E_NOMEM);
            if (hipMemcpy(ctx->wf_bf[l], tmp16.data(), tmp16.size() * 2, hipMemcpyHostToDevice) != hipSuccess) { ctx->err = "weight upload failed"; return bail(NST_E_HIP); }
        } else if (ctx->conv_mode == 2) {
            make_h2(tmp.data(), 9, co, ci, tmp16, &ctx->wf_h2_inv[l]);
            if (dev_alloc(ctx, &ctx->wf_h2[l], tmp16.size() * 2) != NST_OK) return bail(NST_E_NOMEM);
            if (hipMemcpy(ctx->wf_h2[l], tmp16.data(), tmp16.size() * 2, hipMemcpyHostToDevice) != hipSuccess) { ctx->err = "weight upload failed"; return bail(NST_E_HIP); }
            if (ctx->winograd && ci >= 256 && ci % 64 == 0 && co % 128 == 0) {      // (Cin = 128: no gain measured)
                make_wino(tmp.data(), co, ci, tmp16, &ctx->wf_wino_inv[l]);
                if (dev_alloc(ctx, &ctx->wf_wino[l], tmp16.size() * 2) != NST_OK) return bail(NST_E_NOMEM);
                if (hipMemcpy(ctx->wf_wino[l], tmp16.data(), tmp16.size() * 2, hipMemcpyHostToDevice) != hipSuccess) { ctx->err = "weight upload failed"; return bail(NST_E_HIP); }
            }
        }
        // input gradient: a conv with "Cout" = ci and "Cin" = co: wd[tap'][ci][co] = W[co][ci][2-ky'][2-kx']
        for (int t = 0; t < 9; ++t) {
            const int ky = 2 - t / 3, kx = 2 - t % 3;
            for (int c = 0; c < ci; ++c)
                for (int o = 0; o < co; ++o) tmp[((size_t)t * ci + c) * co + o] = W[((size_t)o * ci + c) * 9 + ky * 3 + kx];
        }
        if (dev_alloc_t(ctx, &ctx->wd[l], n) != NST_OK) return bail(NST_E_NOMEM);
        if (hipMemcpy(ctx->wd[l], tmp.data(), n * 4, hipMemcpyHostToDevice) != hipSuccess) { ctx->err = "weight upload failed"; return bail(NST_E_HIP); }
        if (ctx->conv_mode == 1) {
            make_bf3(tmp.data(), 9, ci, co, tmp16);
            if (dev_alloc(ctx, &ctx->wd_bf[l], tmp16.size() * 2) != NST_OK) return bail(NST_E_NOMEM);
            if (hipMemcpy(ctx->wd_bf[l], tmp16.data(), tmp16.size() * 2, hipMemcpyHostToDevice) != hipSuccess) { ctx->err = "weight upload failed"; return bail(NST_E_HIP); }
        } else if (ctx->conv_mode == 2) {
            make_h2(tmp.data(), 9, ci, co, tmp16, &ctx->wd_h2_inv[l]);
            if (dev_alloc(ctx, &ctx->wd_h2[l], tmp16.size() * 2) != NST_OK) return bail(NST_E_NOMEM);
            if (hipMemcpy(ctx->wd_h2[l], tmp16.data(), tmp16.size() * 2, hipMemcpyHostToDevice) != hipSuccess) { ctx->err = "weight upload failed"; return bail(NST_E_HIP); }
            if (ctx->winograd && co >= 256 && co % 64 == 0 && ci % 128 == 0) {
                make_wino(tmp.data(), ci, co, tmp16, &ctx->wd_wino_inv[l]);
                if (dev_alloc(ctx, &ctx->wd_wino[l], tmp16.size() * 2) != NST_OK) return bail(NST_E_NOMEM);
                if (hipMemcpy(ctx->wd_wino[l], tmp16.data(), tmp16.size() * 2, hipMemcpyHostToDevice) != hipSuccess) { ctx->err = "weight upload failed"; return bail(NST_E_HIP); }
            }
        }
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
    for (int i = 0; i < NST_MAX_LEVELS; ++i) free_level(ctx, ctx->lv[i]);
    if (ctx->tail) (void)hipEventDestroy(ctx->tail);
    for (int l = 0; l < NL; ++l) { dev_free(ctx->wf[l]); dev_free(ctx->wd[l]); dev_free(ctx->bias[l]); dev_free(ctx->wf_bf[l]); dev_free(ctx->wd_bf[l]); dev_free(ctx->wf_h2[l]); dev_free(ctx->wd_h2[l]); dev_free(ctx->wf_wino[l]); dev_free(ctx->wd_wino[l]); }
    dev_free(ctx->w11k); dev_free(ctx->w11d); dev_free(ctx->color_scratch);
    if (ctx->gexec) (void)hipGraphExecDestroy(ctx->gexec);
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
    if (ctx) ++ctx->closure_epoch;
    NSTCHK(bind(ctx));
    if (levels_num < 1 || levels_num > NST_MAX_LEVELS) return fail(ctx, NST_E_ARG, "levels_num out of range");
    if ((H0 >> (levels_num - 1)) < 16 || (W0 >> (levels_num - 1)) < 16)
        return fail(ctx, NST_E_ARG, "coarsest pyramid level must be at least 16x16");
    quiesce(ctx);
    for (int i = 0; i < NST_MAX_LEVELS; ++i) free_level(ctx, ctx->lv[i]);
    if (ctx->gexec) { (void)hipGraphExecDestroy(ctx->gexec); ctx->gexec = nullptr; }
    ctx->gkey = {}; ctx->glast = {};
    ctx->levels = 0;
    int h = H0, w = W0;
    for (int i = 0; i < levels_num; ++i) {
        LevelWs& L = ctx->lv[i];
        L.h = h; L.w = w;
        NSTCHK(alloc_acts(ctx, L.acts, h, w));
        L.gbuf_floats = (size_t)h * w * 64;
        NSTCHK(dev_alloc_t(ctx, &L.gbuf[0], L.gbuf_floats));
        NSTCHK(dev_alloc_t(ctx, &L.gbuf[1], L.gbuf_floats));
        if (i > 0) NSTCHK(alloc_level_image(ctx, L));      // sized for the context's current channel count
        NSTCHK(alloc_tap_buffers(ctx, L));       // sized for the context's current taps
        NSTCHK(dev_alloc_t(ctx, &L.content_partial, MSE_BLOCKS));
        NSTCHK(dev_alloc_t(ctx, &L.tv_partial, 2 * TV_BLOCKS));
        NSTCHK(dev_alloc_t(ctx, &L.tv_means, 2));
        h /= 2; w /= 2;
    }
    ctx->levels = levels_num;
    return NST_OK;
}

// LossBuilder(content_feature_maps_index, style_feature_maps_indices, ...) and Vgg19(use_relu=...) of the reference
// (neural_style_transfer.py:41-82, neural_nets.py:17-28) as a context setting
int nst_job_set_taps(nst_ctx* ctx, int content_index, unsigned style_mask, int use_relu) {
    if (ctx) ++ctx->closure_epoch;
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
    // every level's targets and the captured closure belong to the old taps; the tap-sized buffers are re-allocated
    quiesce(ctx);
    if (ctx->gexec) { (void)hipGraphExecDestroy(ctx->gexec); ctx->gexec = nullptr; }
    ctx->gkey = {}; ctx->glast = {};
    ctx->taps = tp;
    for (int i = 0; i < ctx->levels; ++i) {
        LevelWs& L = ctx->lv[i];
        L.targets = false;
        free_tap_buffers(ctx, L);
        NSTCHK(alloc_tap_buffers(ctx, L));
    }
    return NST_OK;
}

// Gatys et al. 2016, luminance-only transfer: the optimised image becomes one plane u = 255 Y (channels = 1) that the
// network sees as x_c = u - mean_c.  Same life cycle as the taps: every level's targets and the captured closure go.
int nst_job_set_color(nst_ctx* ctx, int mode) {
    if (ctx) ++ctx->closure_epoch;
    NSTCHK(bind(ctx));
    if (mode != NST_COLOR_RGB && mode != NST_COLOR_LUMINANCE) return fail(ctx, NST_E_ARG, "mode must be NST_COLOR_RGB or NST_COLOR_LUMINANCE");
    const int channels = mode == NST_COLOR_LUMINANCE ? 1 : 3;
    quiesce(ctx);
    // the level images of the new channel count first: if one cannot be had, the context stays as it was (old mode, old
    // buffers, targets kept)
    float* img[NST_MAX_LEVELS][2] = {};
    int r = NST_OK;
    for (int i = 1; i < ctx->levels && r == NST_OK; ++i) {
        const size_t n = (size_t)channels * ctx->lv[i].h * ctx->lv[i].w;
        r = dev_alloc_t(ctx, &img[i][0], n);
        if (r == NST_OK) r = dev_alloc_t(ctx, &img[i][1], n);
    }
    if (r != NST_OK) {
        for (int i = 1; i < ctx->levels; ++i) {
            const size_t bytes = (size_t)channels * ctx->lv[i].h * ctx->lv[i].w * 4;
            for (float* p : img[i])
                if (p) { dev_free(p); if (ctx->bytes >= bytes) ctx->bytes -= bytes; }
        }
        return r;
    }
    if (ctx->gexec) { (void)hipGraphExecDestroy(ctx->gexec); ctx->gexec = nullptr; }
    ctx->gkey = {}; ctx->glast = {};
    ctx->channels = channels;
    for (int i = 0; i < ctx->levels; ++i) {
        LevelWs& L = ctx->lv[i];
        L.targets = false;
        if (i > 0) {
            free_level_image(ctx, L);
            L.xl = img[i][0]; L.gxl = img[i][1];
            L.xl_floats = (size_t)channels * L.h * L.w;
        }
    }
    return NST_OK;
}

int nst_job_color(const nst_ctx* ctx) { return ctx ? (ctx->channels == 1 ? NST_COLOR_LUMINANCE : NST_COLOR_RGB) : -1; }

// Gatys et al. 2016, section 2: average instead of max pooling in the feature network.  Same life cycle as the taps and the
// colour mode: every level's targets (made with the other network) and the captured closure go; no buffer changes size.
int nst_job_set_pooling(nst_ctx* ctx, int mode) {
    if (ctx) ++ctx->closure_epoch;
    NSTCHK(bind(ctx));
    if (mode != NST_POOL_MAX && mode != NST_POOL_AVG) return fail(ctx, NST_E_ARG, "mode must be NST_POOL_MAX or NST_POOL_AVG");
    quiesce(ctx);
    if (ctx->gexec) { (void)hipGraphExecDestroy(ctx->gexec); ctx->gexec = nullptr; }
    ctx->gkey = {}; ctx->glast = {};
    ctx->pool_avg = mode == NST_POOL_AVG ? 1 : 0;
    for (int i = 0; i < ctx->levels; ++i) ctx->lv[i].targets = false;
    return NST_OK;
}

int nst_job_pooling(const nst_ctx* ctx) { return ctx ? (ctx->pool_avg ? NST_POOL_AVG : NST_POOL_MAX) : -1; }

static bool batch_eligible(const nst_ctx* ctx);
int nst_level_set_targets(nst_ctx* ctx, int level, const float* content, const float* style, int hs, int ws,
                          void* stream) {
    if (ctx) ++ctx->closure_epoch;
    NSTCHK(bind(ctx));
    if (level < 0 || level >= ctx->levels) return fail(ctx, NST_E_STATE, "level not configured");
    if (!content || !style) return fail(ctx, NST_E_ARG, "null image");
    if (hs < 16 || ws < 16) return fail(ctx, NST_E_ARG, "style image must be at least 16x16");
    hipStream_t s = enter(ctx, stream);
    LevelWs& L = ctx->lv[level];
    const Taps& tp = ctx->taps;
    // content: the content map (default ReLU(conv4_2)) of the content image, through the level's own activation buffers - by the launches the closure
    // of this job will use (one launch per layer, Winograd F(2,3) where it applies), so that target and current features
    // carry the same rounding: an image that IS the content image then has a content loss of (all but) exactly zero, as in
    // the reference, whose target and current features come from one and the same forward code
    if (batch_eligible(ctx)) {
        const float* xi[NST_MAX_LEVELS] = {};
        xi[level] = content;
        const int lv1 = level;
        NSTCHK(batched_forward(ctx, xi, &lv1, 1, s, nullptr));
    } else {
        NSTCHK(forward(ctx, L.acts, content, L.h, L.w, s, tp.content, ctx->channels));
    }
    HIPCHK(ctx, hipMemcpyAsync(L.content_t, L.acts.act[tp.content], L.content_n * 4, hipMemcpyDeviceToDevice, s));
    // style: the Gram matrices of the style image (its own size)
    ActSet sa;
    int r = alloc_acts(ctx, sa, hs, ws);
    float* part = nullptr;
    if (r == NST_OK) r = dev_alloc_t(ctx, &part, gram_part_floats_for(tp, hs, ws));
    if (r == NST_OK) r = forward(ctx, sa, style, hs, ws, s, tp.style[tp.nstyle - 1], ctx->channels);
    for (int k = 0; k < tp.nstyle && r == NST_OK; ++k) {
        const int l = tp.style[k];
        const int C = kCout[l];
        const size_t N = (size_t)sa.h[l] * sa.w[l];
        r = gram_of(ctx, sa.act[l], N, C, ctx->conv_mode == 2 ? amax_act(sa, l) : nullptr, (float)((double)C * sa.h[l] * sa.w[l]), part, nullptr, 0.f, L.gram_t[k],
                    nullptr, nullptr, nullptr, nullptr, s);
    }
    hipError_t e = hipStreamSynchronize(s);
    free_acts(ctx, sa);
    dev_free(part);
    if (r != NST_OK) return r;
    HIPCHK(ctx, e);
    L.targets = true;
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

int nst_closure(nst_ctx* ctx, const float* x, float cw, float sw, float tvw, float* grad, float* losses, void* stream) {
    return nst_closure_levels(ctx, x, cw, sw, tvw, 0xFFFFFFFFu, grad, losses, stream);
}

static bool batch_eligible(const nst_ctx* ctx) {
    // needs the bf16 conv kernels (32-bit buffer offsets) and enough tiles to be worth it
    return ctx->batched && ctx->conv_mode && (size_t)ctx->lv[0].h * ctx->lv[0].w * 64 * 4 < 0xFFFFFF00ull &&
           (ctx->levels > 1 || (size_t)ctx->lv[0].h * ctx->lv[0].w >= (size_t)256 * 256);
}

// enqueues the whole closure on `main` (no host synchronisation; capturable unless it forks level streams)
static int closure_record(nst_ctx* ctx, const float* x, float cw, float sw, float tvw, unsigned level_mask, float* grad,
                          float* losses, hipStream_t main);

int nst_closure_levels(nst_ctx* ctx, const float* x, float cw, float sw, float tvw, unsigned level_mask, float* grad,
                       float* losses, void* stream) {
    NSTCHK(bind(ctx));
    if (ctx->levels < 1) return fail(ctx, NST_E_STATE, "nst_job_configure has not been called");
    if (!x || !grad || !losses) return fail(ctx, NST_E_ARG, "null buffer");
    for (int i = 0; i < ctx->levels; ++i)
        if (((level_mask >> i) & 1u) && !ctx->lv[i].targets)
            return fail(ctx, NST_E_STATE, "targets of level " + std::to_string(i) + " not set");
    hipStream_t main = enter(ctx, stream);
    if (ctx->timing >= 2) NSTCHK(fold_timed(ctx));
    ctx->timed.clear();
    ctx->ev_used = 0;
    ctx->timed_valid = false;
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
        done = true;
    }
    if (!done) NSTCHK(closure_record(ctx, x, cw, sw, tvw, level_mask, grad, losses, main));
    if (ctx->timing) { HIPCHK(ctx, hipEventRecord(ctx->t1, main)); ctx->timed_valid = true; }
    mark(ctx, main);
    return NST_OK;
}

static int closure_record(nst_ctx* ctx, const float* x, float cw, float sw, float tvw, unsigned level_mask, float* grad,
                          float* losses, hipStream_t main) {

    // pyramid of the optimised image (neural_style_transfer.py:170-176)
    const float* xi[NST_MAX_LEVELS];
    float* gi[NST_MAX_LEVELS];
    xi[0] = x; gi[0] = grad;
    for (int i = 1; i < ctx->levels; ++i) {
        LevelWs& L = ctx->lv[i];
        Timer t(ctx, main, K_OTHER, 0);
        HIPCHK(ctx, launch_bicubic_down(xi[i - 1], ctx->channels, ctx->lv[i - 1].h, ctx->lv[i - 1].w, L.h, L.w, L.xl, main));
        xi[i] = L.xl; gi[i] = L.gxl;
    }
    const bool batch = batch_eligible(ctx);
    if (batch) {
        const unsigned top = level_mask & 1u, rest = level_mask & ~1u;
        if (ctx->level_split && ctx->side && !ctx->use_graph && top && rest) {
            // nst_options.level_split: the top level's chain on the caller's stream, the lower levels' (batched among
            // themselves) on the side stream - two chains of unequal size whose launch ramps, tails and epilogue bursts can
            // fill one another, as two jobs on one GPU do.  Same kernels on the same tiles: bitwise the same.
            HIPCHK(ctx, hipEventRecord(ctx->side_fork, main));
            HIPCHK(ctx, hipStreamWaitEvent(ctx->side, ctx->side_fork, 0));
            NSTCHK(closure_batched(ctx, xi, gi, top, cw, sw, tvw, main, 1u));
            NSTCHK(closure_batched(ctx, xi, gi, rest, cw, sw, tvw, ctx->side, ~1u));
            HIPCHK(ctx, hipEventRecord(ctx->side_join, ctx->side));
            HIPCHK(ctx, hipStreamWaitEvent(main, ctx->side_join, 0));
        } else {
            NSTCHK(closure_batched(ctx, xi, gi, level_mask, cw, sw, tvw, main));
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
    }

    for (int i = 0; i < ctx->levels && !batch; ++i) {
        LevelWs& L = ctx->lv[i];
        hipStream_t s = multi ? L.stream : main;
        if (multi) HIPCHK(ctx, hipStreamWaitEvent(s, ctx->fork, 0));
        if (!((level_mask >> i) & 1u)) {
            // a level another rank owns: it contributes nothing here (its gradient arrives by all-reduce)
            HIPCHK(ctx, launch_zero(gi[i], (size_t)ctx->channels * L.h * L.w, s));
            if (multi) HIPCHK(ctx, hipEventRecord(L.done, s));
            continue;
        }
        {
            Timer t(ctx, s, K_OTHER, 0);
            HIPCHK(ctx, launch_tv_partial(xi[i], ctx->channels, L.h, L.w, L.tv_partial, s));
        }
        const Taps& tp = ctx->taps;
        NSTCHK(forward(ctx, L.acts, xi[i], L.h, L.w, s, tp.top, ctx->channels));
        Inject inj[NL];
        for (int k = 0; k < tp.nstyle; ++k) {
            const int l = tp.style[k];
            const int C = kCout[l];
            const size_t N = (size_t)L.acts.h[l] * L.acts.w[l];
            const double chw = (double)C * (double)N;
            // style = mean_k mse(G_k, Gt_k); dL/dG = sw/nstyle * 2 (G-Gt)/C^2; dF = 2 * dL/dG * F / (C h w)
            const float coef = (float)((double)sw * 4.0 / ((double)tp.nstyle * (double)C * C * chw));
            NSTCHK(gram_of(ctx, L.acts.act[l], N, C, ctx->conv_mode == 2 ? amax_act(L.acts, l) : nullptr, (float)chw, L.gram_part, L.gram_t[k], coef, nullptr, L.S[k],
                           L.S_bf[k], ctx->conv_mode == 2 ? amax_S(L.acts, k) : nullptr, L.style_partial[k], s));
            inj[l].S = L.S[k];
            inj[l].S_bf = L.S_bf[k];
            inj[l].S_amax = ctx->conv_mode == 2 ? amax_S(L.acts, k) : nullptr;
        }
        inj[tp.content].content = true;
        ContentJob cj{L.content_t, L.content_n, (float)((double)cw * 2.0 / (double)L.content_n), L.content_partial};
        NSTCHK(backward(ctx, L.acts, inj, &cj, L.gbuf[0], L.gbuf[1], gi[i], L.h, L.w, s, tp.top, tp.top_mask(), ctx->channels));
        {
            Timer t(ctx, s, K_OTHER, 0);
            HIPCHK(ctx, launch_tv_finish(xi[i], ctx->channels, L.h, L.w, L.tv_partial, tvw, gi[i], 1, L.tv_means, s));
        }
        if (multi) HIPCHK(ctx, hipEventRecord(L.done, s));
    }
    if (multi)
        for (int i = 0; i < ctx->levels; ++i) HIPCHK(ctx, hipStreamWaitEvent(main, ctx->lv[i].done, 0));

    // pull the coarse-level gradients back up the bicubic chain (autograd of :173-176)
    for (int i = ctx->levels - 1; i >= 1; --i) {
        Timer t(ctx, main, K_OTHER, 0);
        HIPCHK(ctx, launch_bicubic_down_bwd(gi[i], ctx->channels, ctx->lv[i - 1].h, ctx->lv[i - 1].w, ctx->lv[i].h, ctx->lv[i].w,
                                            gi[i - 1], 1, main));
    }
    LossAssembly la{};
    la.levels = ctx->levels; la.nstyle = ctx->taps.nstyle; la.cw = cw; la.sw = sw; la.tvw = tvw; la.out = losses;
    for (int i = 0; i < ctx->levels; ++i) {
        LevelWs& L = ctx->lv[i];
        la.lv[i].content_partial = L.content_partial;
        la.lv[i].content_n = L.content_n;
        for (int k = 0; k < ctx->taps.nstyle; ++k) { la.lv[i].style_partial[k] = L.style_partial[k]; la.lv[i].style_c[k] = kCout[ctx->taps.style[k]]; }
        la.lv[i].tv_means = L.tv_means;
        la.lv[i].owned = (int)((level_mask >> i) & 1u);
    }
    HIPCHK(ctx, launch_loss_assemble(la, main));
    return NST_OK;
}

// ---- stripe (window) closure: spatial sharding of one pyramid level -------------------------------------
int nst_window_sums_count(size_t* count) {
    if (!count) return fail(nullptr, NST_E_ARG, "null argument");
    *count = kWinSums;
    return NST_OK;
}

static int window_check(nst_ctx* ctx, const float* xs, int row0, int rows, int H0) {
    if (ctx->levels != 1) return fail(ctx, NST_E_STATE, "a stripe context is configured with levels_num = 1");
    if (ctx->conv_mode != 2) return fail(ctx, NST_E_STATE, "the stripe closure runs on the f16x2 convolutions (NST_CONV unset)");
    if (!ctx->taps.is_default)
        return fail(ctx, NST_E_STATE, "the stripe closure implements the default feature maps only (nst_job_set_taps(ctx, 4, 0x2F, 1))");
    if (ctx->channels != 3)
        return fail(ctx, NST_E_STATE, "the stripe closure implements RGB only (nst_job_set_color(ctx, NST_COLOR_RGB))");
    if (ctx->pool_avg)
        return fail(ctx, NST_E_STATE, "the stripe closure implements max pooling only (nst_job_set_pooling(ctx, NST_POOL_MAX))");
    LevelWs& L = ctx->lv[0];
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

int nst_window_begin(nst_ctx* ctx, const float* xs, int row0, int rows, int H0, float* sums, void* stream) {
    NSTCHK(bind(ctx));
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
    for (int q = 0; q < 5; ++q) {
        const int l = ctx->taps.style[q], C = kCout[l];
        const size_t off = (size_t)win_r0(win, kScale[l]) * a.w[l] * C;
        const size_t N = (size_t)win_nr(win, kScale[l]) * a.w[l];
        const int ns = gram_nsplit(C, N);
        HIPCHK(ctx, launch_gram_partial(a.act[l] + off, N, C, ns, amax_act(a, l), L.gram_part, s));
        HIPCHK(ctx, launch_gram_finish(L.gram_part, gram_nslabs(C, ns), C, 1.f, nullptr, 0.f, sums + kWinGramOff[q], nullptr, nullptr,
                                       nullptr, nullptr, s));
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
    NSTCHK(window_check(ctx, xs, row0, rows, H0));
    if (!sums || !gxs || !losses) return fail(ctx, NST_E_ARG, "null buffer");
    hipStream_t s = enter(ctx, stream);
    LevelWs& L = ctx->lv[0];
    ActSet& a = L.acts;
    Window win{row0, rows, H0, sums};
    // S = d loss / d G from the Gram sums of ALL stripes, normalised by the full image
    for (int q = 0; q < 5; ++q) {
        const int l = ctx->taps.style[q], C = kCout[l];
        const double chw = (double)C * (double)(H0 >> kScale[l]) * a.w[l];
        const float coef = (float)((double)sw * 4.0 / (5.0 * (double)C * C * chw));
        HIPCHK(ctx, launch_gram_finish(sums + kWinGramOff[q], 1, C, (float)chw, L.gram_t[q], coef, nullptr, L.S[q], L.S_bf[q],
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
    LossAssembly la{};
    la.levels = 1; la.nstyle = 5; la.cw = cw; la.sw = sw; la.tvw = tvw; la.out = losses;
    la.lv[0].content_partial = L.content_partial;
    const int m = ctx->taps.content;
    la.lv[0].content_n = (size_t)(H0 >> kScale[m]) * a.w[m] * kCout[m];
    for (int k = 0; k < 5; ++k) { la.lv[0].style_partial[k] = L.style_partial[k]; la.lv[0].style_c[k] = kCout[ctx->taps.style[k]]; }
    la.lv[0].tv_means = L.tv_means;
    la.lv[0].owned = 1;
    HIPCHK(ctx, launch_loss_assemble(la, s));
    mark(ctx, s);
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

// debugging aid: one line per timed launch of the last closure to stderr
int nst_dump_last_closure(nst_ctx* ctx) {
    NSTCHK(bind(ctx));
    if (!ctx->timed_valid) return NST_OK;
    HIPCHK(ctx, hipEventSynchronize(ctx->t1));
    for (const TimedLaunch& t : ctx->timed) {
        float d = 0.f;
        HIPCHK(ctx, hipEventSynchronize(t.b));
        HIPCHK(ctx, hipEventElapsedTime(&d, t.a, t.b));
        fprintf(stderr, "cls %d  %4dx%-4d cin %3d cout %3d taps %d layer %3d  %8.3f ms  %7.2f TFLOP/s\n", t.cls, t.tag[0],
                t.tag[1], t.tag[2], t.tag[3], t.tag[4], t.tag[5], d, d > 0 ? t.flops / (d * 1e-3) / 1e12 : 0.0);
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

// ---- standalone pieces -----------------------------------------------------------------------------
int nst_vgg_features(nst_ctx* ctx, const float* x, int h, int w, float* const* outs, void* stream) {
    NSTCHK(bind(ctx));
    if (!x || !outs) return fail(ctx, NST_E_ARG, "null argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    ActSet a;
    int r = alloc_acts(ctx, a, h, w);
    if (r == NST_OK) r = forward(ctx, a, x, h, w, s);
    for (int i = 0; i < 6 && r == NST_OK; ++i) {
        if (!outs[i]) continue;
        const int l = kTapLayer[i];
        if (launch_hwc_to_chw(a.act[l], kCout[l], a.h[l], a.w[l], outs[i], s) != hipSuccess) r = fail(ctx, NST_E_HIP, "hwc_to_chw launch failed");
    }
    hipError_t e = hipStreamSynchronize(s);
    free_acts(ctx, a);
    if (r != NST_OK) return r;
    HIPCHK(ctx, e);
    return NST_OK;
}

int nst_vgg_activations(nst_ctx* ctx, const float* x, int h, int w, float* const* outs, void* stream) {
    NSTCHK(bind(ctx));
    if (!x || !outs) return fail(ctx, NST_E_ARG, "null argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    ActSet a;
    int r = alloc_acts(ctx, a, h, w);
    if (r == NST_OK) r = forward(ctx, a, x, h, w, s);
    for (int l = 0; l < NL && r == NST_OK; ++l) {
        if (!outs[l]) continue;
        if (launch_hwc_to_chw(a.act[l], kCout[l], a.h[l], a.w[l], outs[l], s) != hipSuccess) r = fail(ctx, NST_E_HIP, "hwc_to_chw launch failed");
    }
    hipError_t e = hipStreamSynchronize(s);
    free_acts(ctx, a);
    if (r != NST_OK) return r;
    HIPCHK(ctx, e);
    return NST_OK;
}

int nst_level_activation(nst_ctx* ctx, int level, int layer, float* out, void* stream) {
    NSTCHK(bind(ctx));
    if (level < 0 || level >= ctx->levels) return fail(ctx, NST_E_STATE, "level not configured");
    if (layer < 0 || layer >= NL || !out) return fail(ctx, NST_E_ARG, "bad argument");
    const ActSet& a = ctx->lv[level].acts;
    hipStream_t s = enter(ctx, stream);
    HIPCHK(ctx, launch_hwc_to_chw(a.act[layer], kCout[layer], a.h[layer], a.w[layer], out, s));
    mark(ctx, s);
    return NST_OK;
}

int nst_level_image(nst_ctx* ctx, int level, float* out, void* stream) {
    NSTCHK(bind(ctx));
    if (level < 1 || level >= ctx->levels) return fail(ctx, NST_E_ARG, "level must be 1 .. levels_num - 1 (level 0 is the caller's x)");
    if (!out) return fail(ctx, NST_E_ARG, "null argument");
    const LevelWs& L = ctx->lv[level];
    hipStream_t s = enter(ctx, stream);
    HIPCHK(ctx, hipMemcpyAsync(out, L.xl, (size_t)ctx->channels * L.h * L.w * sizeof(float), hipMemcpyDeviceToDevice, s));
    mark(ctx, s);
    return NST_OK;
}

int nst_vgg_features_backward(nst_ctx* ctx, const float* x, int h, int w, const float* const* gouts, float* gx,
                              void* stream) {
    NSTCHK(bind(ctx));
    if (!x || !gouts || !gx) return fail(ctx, NST_E_ARG, "null argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    ActSet a;
    float* g0 = nullptr; float* g1 = nullptr;
    float* inj_buf[6] = {};
    int r = alloc_acts(ctx, a, h, w);
    if (r == NST_OK) r = dev_alloc_t(ctx, &g0, (size_t)h * w * 64);
    if (r == NST_OK) r = dev_alloc_t(ctx, &g1, (size_t)h * w * 64);
    if (r == NST_OK) r = forward(ctx, a, x, h, w, s);
    Inject inj[NL];
    for (int i = 0; i < 6 && r == NST_OK; ++i) {
        if (!gouts[i]) continue;
        const int l = kTapLayer[i];
        r = dev_alloc_t(ctx, &inj_buf[i], (size_t)a.h[l] * a.w[l] * kCout[l]);
        if (r == NST_OK && launch_chw_to_hwc(gouts[i], kCout[l], a.h[l], a.w[l], inj_buf[i], s) != hipSuccess)
            r = fail(ctx, NST_E_HIP, "chw_to_hwc launch failed");
        inj[l].direct = inj_buf[i];
    }
    if (r == NST_OK) r = backward(ctx, a, inj, nullptr, g0, g1, gx, h, w, s, NL - 1, ctx->taps.use_relu != 0);
    hipError_t e = hipStreamSynchronize(s);
    free_acts(ctx, a);
    dev_free(g0); dev_free(g1);
    for (int i = 0; i < 6; ++i) dev_free(inj_buf[i]);
    if (r != NST_OK) return r;
    HIPCHK(ctx, e);
    return NST_OK;
}

int nst_gram(nst_ctx* ctx, const float* f, int C, int h, int w, int normalize, float* gram, void* stream) {
    NSTCHK(bind(ctx));
    if (!f || !gram || C < 1 || h < 1 || w < 1) return fail(ctx, NST_E_ARG, "bad argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t N = (size_t)h * w;
    float* nhwc = nullptr; float* part = nullptr; unsigned* amax = nullptr;
    int r = dev_alloc_t(ctx, &nhwc, N * C);
    if (r == NST_OK) r = dev_alloc_t(ctx, &part, (size_t)gram_nsplit(C, N) * C * C);
    if (r == NST_OK && ctx->conv_mode == 2) r = dev_alloc_t(ctx, &amax, (size_t)NST_AMAX_SLOTS);
    if (r == NST_OK && launch_chw_to_hwc(f, C, h, w, nhwc, s) != hipSuccess) r = fail(ctx, NST_E_HIP, "chw_to_hwc launch failed");
    if (r == NST_OK && amax) {
        // the fp16-piece kernel needs the absmax of its operand (in the closure the producing conv records it)
        if (launch_zero(amax, NST_AMAX_SLOTS, s) != hipSuccess || launch_absmax_slots(nhwc, N * C, amax, s) != hipSuccess)
            r = fail(ctx, NST_E_HIP, "absmax launch failed");
    }
    if (r == NST_OK)
        r = gram_of(ctx, nhwc, N, C, amax, normalize ? (float)((double)C * h * w) : 1.f, part, nullptr, 0.f, gram, nullptr, nullptr, nullptr, nullptr, s);
    hipError_t e = hipStreamSynchronize(s);
    dev_free(nhwc); dev_free(part); dev_free(amax);
    if (r != NST_OK) return r;
    HIPCHK(ctx, e);
    return NST_OK;
}

int nst_total_variation(nst_ctx* ctx, const float* y, int C, int h, int w, float* value, float* grad, void* stream) {
    NSTCHK(bind(ctx));
    if (!y || !value) return fail(ctx, NST_E_ARG, "null argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    double* partial = nullptr; float* means = nullptr;
    int r = dev_alloc_t(ctx, &partial, 2 * TV_BLOCKS);
    if (r == NST_OK) r = dev_alloc_t(ctx, &means, 2);
    hipError_t e = hipSuccess;
    if (r == NST_OK) {
        e = launch_tv_partial(y, C, h, w, partial, s);
        if (e == hipSuccess) e = launch_tv_finish(y, C, h, w, partial, 1.f, grad, 0, means, s);
        float m[2] = {0, 0};
        if (e == hipSuccess) e = hipMemcpyAsync(m, means, 8, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        const float tv = m[0] * m[0] + m[1] * m[1];
        if (e == hipSuccess) e = hipMemcpy(value, &tv, 4, hipMemcpyHostToDevice);
    }
    dev_free(partial); dev_free(means);
    if (r != NST_OK) return r;
    HIPCHK(ctx, e);
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
    double* t0 = nullptr; double* t1 = nullptr; double* wt = nullptr;
    int r = dev_alloc_t(ctx, &t0, n);
    if (r == NST_OK) r = dev_alloc_t(ctx, &t1, n);
    if (r == NST_OK) r = dev_alloc_t(ctx, &wt, n);
    hipError_t e = hipSuccess;
    if (r == NST_OK) {
        e = launch_blend_weight(content, h, w, channels, noise_factor, t0, t1, wt, s);
        if (e == hipSuccess) e = launch_blend_init(content, noise, wt, n, out, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
    }
    dev_free(t0); dev_free(t1); dev_free(wt);
    if (ctx->bytes >= 3 * n * 8) ctx->bytes -= 3 * n * 8;
    if (r != NST_OK) return r;
    HIPCHK(ctx, e);
    return NST_OK;
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
    if (!ctx->color_scratch) NSTCHK(dev_alloc_t(ctx, &ctx->color_scratch, (size_t)COLOR_BLOCKS * 9 + 12));
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

// ---- internal accessors for nst_opt.cpp (not part of the public ABI) --------------------------------
int nst_internal_device(const nst_ctx* ctx) { return ctx ? ctx->device : 0; }
int nst_internal_levels(const nst_ctx* ctx) { return ctx ? ctx->levels : 0; }
int nst_internal_channels(const nst_ctx* ctx) { return ctx ? ctx->channels : 3; }
size_t nst_internal_pixels(const nst_ctx* ctx) { return (ctx && ctx->levels > 0) ? (size_t)ctx->lv[0].h * ctx->lv[0].w : 0; }
int nst_internal_fail(nst_ctx* ctx, int code, const char* msg) { return fail(ctx, code, msg ? msg : ""); }
void nst_internal_poison(void* p, size_t bytes) { poison_if_asked(p, bytes); }
int nst_internal_lbfgs_gram(const nst_ctx* ctx) { return ctx ? ctx->lbfgs_gram : 1; }
unsigned long long nst_internal_closure_epoch(const nst_ctx* ctx) { return ctx ? ctx->closure_epoch : 0; }
void nst_internal_mark(nst_ctx* ctx, void* stream) { mark(ctx, static_cast<hipStream_t>(stream)); }

}  // extern "C"
