// nst_ctx.h - what the host sources of the C ABI share (not installed, not part of include/nst_hip.h): the VGG19 layer
// tables, the context and its per-level workspace, error reporting, the launch timer, and the helpers one source defines
// and another calls.  nst_ctx.cpp: context and job state; nst_closure.cpp: network and closure; nst_api.cpp: standalone
// entry points; nst_opt.cpp: the optimisers; nst_comm.cpp: the collective (error reporting only).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <optional>
#include <string>
#include <utility>
#include <vector>

#include "../../include/nst_hip.h"
#include "nst_kernels.h"

#pragma GCC visibility push(hidden)      // host-internal: none of this is a symbol of libnst_hip.so
#include "nst_devmem.h"                  // (in here: its two functions are host-internal too)
namespace nst {

constexpr int NL = NST_VGG19_CONVS;
constexpr int kCin[NL] = {3, 64, 64, 128, 128, 256, 256, 256, 256, 512, 512, 512, 512};
constexpr int kCout[NL] = {64, 64, 128, 128, 256, 256, 256, 256, 512, 512, 512, 512, 512};
constexpr int kScale[NL] = {0, 0, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4};      // log2 of the spatial divisor
constexpr int kPoolAfter[4] = {1, 3, 7, 11};
// reference output index (neural_nets.py:22) -> conv layer
constexpr int kTapLayer[6] = {0, 2, 4, 8, 9, 12};
// the reference's default taps (neural_nets.py:25-28): content 4 = ReLU(conv4_2), style 0, 1, 2, 3, 5 =
// relu1_1, relu2_1, relu3_1, relu4_1, relu5_1; a context's own taps (nst_job_set_taps) live in nst_ctx::taps
constexpr int kMaxStyle = 6;
// conv layer of a tap -> its index in Vgg19.layer_names (what the style layer weights are indexed by)
inline int tap_index_of(int layer) {
    for (int i = 0; i < 6; ++i) if (kTapLayer[i] == layer) return i;
    return -1;
}
inline int pool_index_after(int l) {
    for (int k = 0; k < 4; ++k) if (kPoolAfter[k] == l) return k;
    return -1;
}

struct ActSet {                 // activations of one forward pass, NHWC
    int h[NL], w[NL];
    float* act[NL] = {};
    float* pool[4] = {};
    float* splitk = nullptr;     // split-K partial sums of the small-spatial conv layers
    size_t splitk_floats = 0;
    unsigned* bits[NL] = {};     // ReLU bit-masks ([h*w][C/32] words) of the layers whose mask the backward reads
    bool bits_valid[NL] = {};    // written by the last forward pass (false when that layer ran split-K / fp32)
    bool pooled[4] = {};         // pool[k] already produced by the conv epilogue of the last forward pass
    // act[l] written by the last forward pass: the batched f16x2 walker leaves out a full-resolution map that nothing reads
    // (map_stored in nst_closure.cpp has the rule); nst_level_activation writes such a map on request (restore_map)
    bool stored[NL] = {};
    // the batched pass that last wrote this set: its number (nst_ctx::fwd_pass; 0: none since the job was set up) and the
    // levels its launches covered, in launch order - what restore_map repeats a layer's launch over
    unsigned long long pass = 0;
    int pass_lv[NST_MAX_LEVELS] = {};
    int pass_n = 0;
    // absmax records for the fp16-piece convolutions (conv_h2.hip): AMAX_IDS x NST_AMAX_SLOTS words.
    // ids: act[l] -> l; the Gram factor S of style slot q -> NL + q (6 slots); the gradient w.r.t. the pre-ReLU output
    // of layer l (or a bound of it: the pooled gradient it was un-pooled from) -> NL + 6 + l
    unsigned* amax = nullptr;
    // arg-max codes of the four max-pools (average pooling: the multi-hot ReLU-on codes), written by the fused pooling of the
    // f16x2 forward launches and read by the un-pooling loader of the input-gradient launch below each pool: [H/2*W/2][C/32][4] words
    unsigned* pcode[4] = {};
    DevMem mem;                  // owns every buffer above: `a = ActSet()` frees the set
    // a forward pass starts: nothing of the previous one's masks and fused pools is valid any more
    void begin_pass() {
        for (int l = 0; l < NL; ++l) bits_valid[l] = false;
        for (int k = 0; k < 4; ++k) pooled[k] = false;
        for (int l = 0; l < NL; ++l) stored[l] = false;
    }
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
    // every layer's output goes through its ReLU, but conv5_1's under use_relu = 0
    int relu_of(int l) const { return (l == NL - 1 && !use_relu) ? 0 : 1; }
    // the top layer's gradient goes through its ReLU mask unless it is the pre-ReLU conv5_1
    bool top_mask() const { return use_relu || top != NST_VGG19_CONVS - 1; }
};

enum KClass { K_CONV3 = 0, K_GRAM = 1, K_CONV1 = 2, K_OTHER = 3, K_NCLASS = 4 };

// mfma_factor: executed matrix-pipe FLOPs per algorithmic FLOP (< 0: the arithmetic mode's); shape: what the conv_h2 launcher
// decided for this launch (rows = 0: another kernel ran)
struct TimedLaunch { hipEvent_t a, b; int cls; double flops; int tag[6]; double mfma_factor; H2Shape shape; };

// Spatial control of one level (nst_level_set_guidance; include/nst_hip.h has the definitions).  Everything here is made
// when guidance is set and freed when it is cleared, the taps change or the job is configured again: a closure allocates
// nothing.  Region r of style slot q: gram_t[q] + r C^2, S[q] + r C^2, partial[q] + r gram_finish_blocks(C).
struct Guidance {
    int R = 0;                          // 0: the level is not guided
    float lambda[NST_MAX_REGIONS] = {1.f, 1.f, 1.f, 1.f};
    float* planes = nullptr;            // the guidance pyramid: scale s at plane_off[s], (R, h >> s, w >> s)
    size_t plane_off[5] = {};
    size_t plane_floats = 0;
    double mass[5][NST_MAX_REGIONS] = {};   // n_r of every scale (host copy: the divisors and coefficients are made from it)
    float* gram_t[kMaxStyle] = {};      // guided targets (nst_level_set_targets_guided)
    float* S[kMaxStyle] = {};
    double* partial[kMaxStyle] = {};
    float* part = nullptr;              // partial-Gram slabs: region r at r * part_floats_r
    size_t part_floats_r = 0;
    bool targets = false;               // gram_t holds the targets of targets_R regions
    int targets_R = 0;
    DevMem mem;
    const float* plane(int scale, int r, int h, int w) const { return planes + plane_off[scale] + (size_t)r * (h >> scale) * (w >> scale); }
};

// The Laplacian loss of one level (nst_job_set_laplacian; include/nst_hip.h has the definition): per entry k the pooled sum
// s (h / p, w / p, double), the residual r (float) and the target D s(content) (double; both (h / p - 2, w / p - 2)) and the SSE partials.  Made by
// the setter, freed when the setting is cleared or the job configured again: a closure allocates nothing.
struct LapLevel {
    double* s[NST_LAP_MAX] = {};
    float* r[NST_LAP_MAX] = {};
    double* target[NST_LAP_MAX] = {};
    double* partial[NST_LAP_MAX] = {};
    float* vals = nullptr;      // level 0 only: NST_MAX_LEVELS x NST_LAP_MAX, the unweighted lap_k of the last closure (the loss rows write it)
    DevMem mem;
};

// The matting term of one level (nst_job_set_matting; include/nst_hip.h has the definition): the guide, a copy of the level's
// content as nst_level_set_targets* got it (channels x h x w, made with the targets), and the value partials of the tiles.
// Made by the setter, freed when the setting is cleared or the job configured again: a closure allocates nothing.
struct MatLevel {
    float* guide = nullptr;
    double* partial = nullptr;
    int tiles = 0;
    float* vals = nullptr;      // level 0 only: NST_MAX_LEVELS, the unweighted mat of the last closure (the loss rows write it)
    DevMem mem;
};

// The shifted / centred Gram statistic of one level (nst_job_set_gram_shift; include/nst_hip.h has the definition): per style
// slot the offsets o the last closure used, the row bias r = o S of its backward, the absmax record of the shifted operand
// F + o, and (a centred map) the scratch of the channel sums.  Sized for the widest map, so the taps may change under it.
// Made by the setter, freed when the setting is cleared or the job configured again: a closure allocates nothing.
constexpr int GS_MAX_C = 512;
constexpr int GS_STRIDE = 2 * GS_MAX_C + NST_AMAX_SLOTS;      // words of one slot: o | r | record
constexpr bool maps_fit_gram_shift() {
    for (int c : kCout) if (c > GS_MAX_C) return false;
    return true;
}
static_assert(maps_fit_gram_shift(), "a map wider than GS_MAX_C: the per-slot buffers of GramShiftLevel are sized by it");
struct GramShiftLevel {
    float* words = nullptr;     // kMaxStyle x GS_STRIDE
    double* sums = nullptr;     // kMaxStyle x GS_PART_DOUBLES (only with a centred map)
    DevMem mem;
    float* offset(int q) const { return words + (size_t)q * GS_STRIDE; }
    float* row_bias(int q) const { return words + (size_t)q * GS_STRIDE + GS_MAX_C; }
    unsigned* amax(int q) const { return reinterpret_cast<unsigned*>(words + (size_t)q * GS_STRIDE + 2 * GS_MAX_C); }
    double* part(int q) const { return sums ? sums + (size_t)q * GS_PART_DOUBLES : nullptr; }
};

// The moment loss of one level (nst_job_set_moments; include/nst_hip.h has the definition): per style slot the targets mu^t
// and sigma^t (made with the level's targets), the row bias of the slot's backward launch (a - b o mu, on top of a shifted
// Gram's r = o S), mu and sigma of the last closure with its two values (doubles), and the scratch of the channel sums.
// Sized for the widest map, so the taps may change under it.  Made by the setter, freed when the setting is cleared or the
// job configured again: a closure allocates nothing.
constexpr int MOM_STRIDE = 3 * GS_MAX_C;                      // words of one slot: mu^t | sigma^t | row bias
constexpr int MOM_STAT_STRIDE = 2 * GS_MAX_C + 2;             // doubles of one slot: mu | sigma | mean_i, std_i
struct MomentLevel {
    float* words = nullptr;     // kMaxStyle x MOM_STRIDE
    double* stats = nullptr;    // kMaxStyle x MOM_STAT_STRIDE
    double* sums = nullptr;     // kMaxStyle x MOM_PART_DOUBLES
    float* vals = nullptr;      // level 0 only: NST_MAX_LEVELS x 6 x 2, the unweighted (mean_i, std_i) of the last closure by map index
    DevMem mem;
    float* mean_t(int q) const { return words + (size_t)q * MOM_STRIDE; }
    float* std_t(int q) const { return words + (size_t)q * MOM_STRIDE + GS_MAX_C; }
    float* row_bias(int q) const { return words + (size_t)q * MOM_STRIDE + 2 * GS_MAX_C; }
    double* stat(int q) const { return stats + (size_t)q * MOM_STAT_STRIDE; }
    double* loss(int q) const { return stats + (size_t)q * MOM_STAT_STRIDE + 2 * GS_MAX_C; }
    double* part(int q) const { return sums + (size_t)q * MOM_PART_DOUBLES; }
};

// The temporal term of one level (nst_level_set_anchor; include/nst_hip.h has the definition): copies of the anchor
// (channels x h x w) and of the weight plane (h x w; nullptr: ones), the value partials, and the unweighted tmp of the last
// closure (one float, which the loss rows write).  Data of one job, not a setting: made by the setter, freed when the level's
// anchor is cleared, the colour mode changes or the job is configured again: a closure allocates nothing.
struct AnchorLevel {
    float gamma = 0.f;          // 0: the level has no anchor
    float* anchor = nullptr;
    float* weights = nullptr;
    double* partial = nullptr;  // ANCHOR_BLOCKS
    float* val = nullptr;
    DevMem mem;
};

// What the per-map terms of one level share (PatchLevel, HistLevel, RemdLevel, SelfSimLevel, XcorrLevel below; always in that order; the
// loss assembly adds the rows of the first NST_MAP_TERMS of them, xcorr_loss_rows those of the last): the weights by map index (0: the map has no term), the six unweighted values of the last closure (which the forward
// half writes and the loss rows read), and the block's memory.
struct MapTerm {
    float w[6] = {};
    float* vals = nullptr;
    DevMem mem;
    bool on() const {
        for (float v : w) if (v > 0.f) return true;
        return false;
    }
    // conv layer m carries the term
    bool carries(int m) const {
        const int i = tap_index_of(m);
        return i >= 0 && w[i] > 0.f;
    }
};
enum MapTermId { T_MRF = 0, T_HIST = 1, T_REMD = 2, T_SELFSIM = 3, T_XCORR = 4 };

// The MRF term of one level (nst_level_set_patches; include/nst_hip.h has the definition), by map index: the weight (0: the
// map has no term), the style's map with its dictionary (d[i]: fs, the absmax record, rq and the packed operand), the search
// keys, nn and the value partials of the last closure, and the unweighted mrf_i (six floats, which the forward half writes
// and the loss rows read).  Data of one job, not a setting: made by the setter, freed when the level's term is cleared, the
// taps, the pooling or the colour mode are set or the job is configured again: a closure allocates nothing.
// The semantic guidance of a level's MRF term (nst_level_set_patch_guidance; include/nst_hip.h has the definition), by map
// index of the weighted maps: the descriptors of the image patches (n x 4) and of the dictionary entries (32 pm_dict_tiles(m)
// x 4, zeros behind entry m), both made by the setter from the pooled planes, and the image patches' norms rp (32
// pm_dict_tiles(n) floats), which the forward half writes before every guided search.  Part of PatchLevel: whatever drops the
// level's term drops its guidance.
struct PatchGuide {
    int R = 0;                  // 0: the level's search is unguided
    float gamma = 0.f;
    float* gd[6] = {};
    float* ge[6] = {};
    float* rp[6] = {};
    DevMem mem;
};

struct PatchLevel : MapTerm {
    int stride = 1;
    double eps = 1e-5;
    int hs = 0, ws = 0;         // the style image of nst_level_set_patches: the size of the guidance's style planes
    PatchGuide sem;
    PatchDict d[6] = {};
    unsigned long long* keys[6] = {};
    int* nn[6] = {};
    double* partial[6] = {};    // PM_VALUE_BLOCKS each
};

// The histogram loss of one level (nst_level_set_histograms; include/nst_hip.h has the definition), by map index: the weight
// (0: the map has no term), the style's record (s_lo_hi: C x 2, s_counts: C x bins, Ns pixels - the style's maps are not kept),
// the image side of the last closure (lo_hi, counts, the table ends: C x bins x 2), the value partials, and the unweighted
// hist_i (six floats, which the forward half writes and the loss rows read).  Data of one job with PatchLevel's life cycle:
// everything is made by the setter, a closure allocates nothing.
struct HistLevel : MapTerm {
    int bins = 256;
    size_t Ns[6] = {};
    float* s_lo_hi[6] = {};
    unsigned* s_counts[6] = {};
    float* lo_hi[6] = {};
    unsigned* counts[6] = {};
    float* ends[6] = {};
    double* partial[6] = {};    // HIST_VALUE_BLOCKS each
};

// The relaxed EMD term of one level (nst_level_set_remd; include/nst_hip.h has the definition), by map index: the weight (0: the
// map has no term) and the stride pair; the style side y[i] (the style's map, its absmax record, rq and the packed operand, all
// made by the setter); the image side's buffers, which the forward half fills every closure (rp and the packed operand; f, the
// size and the absmax record are the level's own map's); the keys of both directions, nnA, nnB, the stored cosines, the value
// partials, (remd, rA, rB) and the side flag; and the unweighted remd_i (six floats, which the forward half writes and the loss
// rows read).  Data of one job with PatchLevel's life cycle: everything is made by the setter, a closure allocates nothing.
struct RemdLevel : MapTerm {
    int si[6] = {1, 1, 1, 1, 1, 1}, ss[6] = {1, 1, 1, 1, 1, 1};
    double eps = 1e-5;
    int hs = 0, ws = 0;         // the style image of nst_level_set_remd
    RemdSide y[6] = {};
    int n[6] = {};              // image samples of the map
    float* rp[6] = {};
    unsigned char* xpacked[6] = {};
    unsigned long long* keysA[6] = {};
    unsigned long long* keysB[6] = {};
    int* nnA[6] = {};
    int* nnB[6] = {};
    float* cosA[6] = {};
    float* cosB[6] = {};
    double* partial[6] = {};    // 2 REMD_VALUE_BLOCKS each
    float* rec[6] = {};         // (remd, rA, rB)
    int* side[6] = {};
};

// The self-similarity term of one level (nst_level_set_selfsim; include/nst_hip.h has the definition), by map index: the weight
// (0: the map has no term; any map the job uses may carry one) and the stride; the content's side, made once by the setter (Dc:
// n x n, qc); the image side's buffers, which the forward half fills every closure (rp, the packed operand, D, s, q, the signs,
// t and the partials) and the backward half's workspace (W: n x n, U: n x C); and the unweighted selfsim_k (six floats, which
// the forward half writes and the loss rows read).  Data of one job with PatchLevel's life cycle: everything is made by the
// setter, a closure allocates nothing.
struct SelfSimLevel : MapTerm {
    int stride[6] = {1, 1, 1, 1, 1, 1};
    double eps = 1e-5;
    int n[6] = {};              // samples of the map
    float* Dc[6] = {};
    double* qc[6] = {};
    float* rp[6] = {};
    unsigned char* xpacked[6] = {};
    float* D[6] = {};
    double* s[6] = {};
    double* q[6] = {};
    signed char* sg[6] = {};
    double* t[6] = {};
    double* partial[6] = {};    // 2 SELFSIM_ROW_BLOCKS n each
    float* W[6] = {};
    float* U[6] = {};
};

// The long-range style term of one level (nst_level_set_xcorr; include/nst_hip.h has the definition): the shifts (nd of them, at
// most XCORR_MAX_SHIFTS, the same for every map of the level) and the style image's size; by map index the weight (0: the map
// has no term), the style's G_d stack (Gt: nd x C x C, made once by the setter), the image side's stacks, which the forward half
// fills every closure (G, S = coef (G - Gt) and its transpose St), per shift the slabs of the value pass, the finish pass's
// partial sums of squares (sq: nd x xcorr_finish_blocks(C)), and the unweighted xcorr_i (six floats, which the forward half
// writes and the loss rows read).  Data of one job with PatchLevel's life cycle: everything is made by the setter, a closure
// allocates nothing.
struct XcorrLevel : MapTerm {
    int nd = 0;
    int dx[XCORR_MAX_SHIFTS] = {}, dy[XCORR_MAX_SHIFTS] = {};
    int hs = 0, ws = 0;         // the style image of nst_level_set_xcorr
    float* Gt[6] = {};
    float* G[6] = {};
    float* S[6] = {};
    float* St[6] = {};
    float* part[6][XCORR_MAX_SHIFTS] = {};
    double* sq[6] = {};
};

// the level image and its gradient (levels >= 1), planar: channels (nst_job_set_color) x h x w floats each
struct LevelImage {
    float* xl = nullptr;
    float* gxl = nullptr;
    DevMem mem;
};

struct LevelWs {
    int h = 0, w = 0;
    Guidance guide;
    LapLevel lap;
    MatLevel mat;
    GramShiftLevel gs;
    MomentLevel mom;
    AnchorLevel anc;
    PatchLevel pm;
    HistLevel hist;
    RemdLevel remd;
    SelfSimLevel selfsim;
    XcorrLevel xcorr;
    const MapTerm& map_term(int t) const {
        return t == T_MRF ? (const MapTerm&)pm : t == T_HIST ? (const MapTerm&)hist : t == T_REMD ? (const MapTerm&)remd
             : t == T_SELFSIM ? (const MapTerm&)selfsim : xcorr;
    }
    ActSet acts;
    float* gbuf[2] = {};
    size_t gbuf_floats = 0;
    LevelImage img;
    // the buffers whose size depends on the taps (tap_mem owns them): content target, Gram targets / factors / partial sums,
    // partial-Gram workspace
    float* content_t = nullptr; // NHWC target ReLU(conv4_2)
    size_t content_n = 0;
    float* gram_t[kMaxStyle] = {};
    float* S[kMaxStyle] = {};
    unsigned short* S_bf[kMaxStyle] = {};
    float* gram_part = nullptr;
    size_t gram_part_floats = 0;
    double* style_partial[kMaxStyle] = {};
    DevMem tap_mem;
    double* content_partial = nullptr;
    double* tv_partial = nullptr;
    float* tv_means = nullptr;
    bool targets = false;
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;
    DevMem mem;                 // owns gbuf and the partials
};

}  // namespace nst

struct nst_ctx {
    int device = 0;
    std::string err;
    float* wf[nst::NL] = {};
    float* wd[nst::NL] = {};
    void* wf_bf[nst::NL] = {};       // the same weights cut into 3 bf16 pieces (conv_bf3.hip layout)
    void* wd_bf[nst::NL] = {};
    void* wd_wino[nst::NL] = {};     // the same for the input-gradient launches
    float wd_wino_inv[nst::NL] = {};
    void* wf_wino[nst::NL] = {};     // conv_wino.hip's transformed forward weights (nst_options.h2_winograd), true = pieces * wf_wino_inv
    float wf_wino_inv[nst::NL] = {};
    int winograd = 0;           // nst_options.h2_winograd
    void* wf_h2[nst::NL] = {};       // ... cut into 2 scaled fp16 pieces (conv_h2.hip layout), true = pieces * w*_h2_inv
    void* wd_h2[nst::NL] = {};
    float wf_h2_inv[nst::NL] = {};
    float wd_h2_inv[nst::NL] = {};
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
    int keep_all_maps = 0;      // nst_ctx_set_keep_all_maps: 1 = every batched forward launch stores its full-resolution map
    // nst_ctx_set_forward_pack: 1 = the batched f16x2 forward half launches its front (absmax clears, TV partials, conv1_1)
    // and its loss terms once for all levels and leaves S in bf16 pieces unwritten; 0 = per level, with the pieces
    int forward_pack = 1;
    // nst_ctx_set_gram_pack: 1 = the fp16-piece Gram kernels skip the blocks below the diagonal of a diagonal tile and a
    // plain batch takes both tile shapes in one launch; 0 = the kernels and the two launches from before
    int gram_pack = 1;
    // nst_ctx_set_h2_direct_weights: which forward launches of the 16-channel-chunk conv_h2 shapes take their B fragments
    // from wf_h2_frag (L2 -> registers, one barrier per chunk): bit 0 = <16,64,2,16> (conv1_2), bit 1 = <8,128,2,16>
    // (conv2_1, conv2_2, conv3_1); 0 = the weight slices go through LDS as before.  The default is decided per shape
    // (profiles/r21_h2_direct_weights.txt).  The images exist either way (2.2 MB), so the switch works in both directions.
    int h2_direct_weights = NST_H2_DIRECT_DEFAULT;
    unsigned long long h2_direct_launches = 0;      // conv_h2 launches that ran the DIRECT K loop (nst_ctx_h2_direct_launches)
    void* wf_h2_frag[nst::NL] = {};      // wf_h2's pieces in MFMA fragment order (make_h2_frag); nullptr: not a short-K layer
    unsigned long long fwd_pass = 0;     // batched forward passes so far (ActSet::pass)
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
    float* bias[nst::NL] = {};
    float* w11k = nullptr;      // [28][64]
    float* w11d = nullptr;      // [9][64][4]
    int levels = 0;
    nst::Taps taps;             // nst_job_set_taps
    int channels = 3;           // nst_job_set_color: 3 = RGB, 1 = luminance (the optimised image is u = 255 Y)
    int pool_avg = 0;           // nst_job_set_pooling: 1 = the four pools average their windows (include/nst_hip.h has the definition)
    // nst_job_set_style_weights: the weight of each of the six maps in the style term, by map index (not by style slot: they
    // survive nst_job_set_taps).  One code path: a new context's ones multiply exactly
    float style_w[6] = {1.f, 1.f, 1.f, 1.f, 1.f, 1.f};
    float style_weight(int q) const { return style_w[nst::tap_index_of(taps.style[q])]; }      // of style slot q
    bool unit_style_weights() const {
        for (float w : style_w) if (w != 1.f) return false;
        return true;
    }
    // nst_job_set_laplacian: lap_k entries (pool size, weight), 0 = the term is off
    int lap_k = 0;
    int lap_pool[nst::NST_LAP_MAX] = {};
    float lap_gamma[nst::NST_LAP_MAX] = {};
    // nst_job_set_matting: the weight (0 = the term is off) and epsilon
    float mat_gamma = 0.f;
    double mat_eps = 1e-7;
    // nst_job_set_gram_shift: per map index (as the style layer weights) a constant shift, or (bit of gs_center) centring
    float gs_shift[6] = {};
    unsigned gs_center = 0;
    bool gs_on() const {
        for (float v : gs_shift) if (v != 0.f) return true;
        return gs_center != 0u;
    }
    float gs_shift_of(int q) const { return gs_shift[nst::tap_index_of(taps.style[q])]; }                  // of style slot q
    int gs_center_of(int q) const { return (int)((gs_center >> nst::tap_index_of(taps.style[q])) & 1u); }
    // nst_job_set_moments: per map index (as the style layer weights) the weights of mean_i and std_i, and epsilon; all zero =
    // the term is off
    float mom_wm[6] = {};
    float mom_ws[6] = {};
    float mom_eps = 1e-5f;
    bool mom_on() const {
        for (int i = 0; i < 6; ++i) if (mom_wm[i] > 0.f || mom_ws[i] > 0.f) return true;
        return false;
    }
    float mom_wm_of(int q) const { return mom_wm[nst::tap_index_of(taps.style[q])]; }                      // of style slot q
    float mom_ws_of(int q) const { return mom_ws[nst::tap_index_of(taps.style[q])]; }
    bool mom_slot(int q) const { return mom_wm_of(q) > 0.f || mom_ws_of(q) > 0.f; }                        // slot q carries the term
    // the row bias of style slot q's backward launch at level L: the moment term's (which holds a shifted Gram's r too), else
    // a shifted Gram's, else none
    const float* row_bias_of(const nst::LevelWs& L, int q) const {
        if (mom_on() && mom_slot(q)) return L.mom.row_bias(q);
        return gs_on() ? L.gs.row_bias(q) : nullptr;
    }
    // bumped on entry to every call that changes what a closure computes (configure, taps, colour, pooling, style weights, Laplacian, matting, Gram shift, moments, targets, a level's anchor, a level's per-map terms - nst::MapTerm), failure paths
    // included: an optimiser's remembered closure result is valid only under the epoch it was made in (nst_opt.cpp)
    unsigned long long closure_epoch = 0;
    // advanced on entry to every call that reads or writes the level workspaces (nst_closure*, nst_window_*,
    // nst_level_activation, nst_level_set_targets, nst_job_*): what tells nst_closure_backward that the forward it
    // belongs to is still the last thing that used them
    unsigned long long ws_seq = 0;
    struct ForwardToken {                // the arguments and state of the last nst_closure_forward
        bool valid = false;
        const float* x = nullptr;
        float cw = 0.f, sw = 0.f, tvw = 0.f;
        unsigned mask = 0;
        unsigned long long epoch = 0, seq = 0;
    } fwd_token;
    double* color_scratch = nullptr;   // nst_color_stats: COLOR_BLOCKS * 9 partials | mean (3) | cov (9), made on first use
    nst::LevelWs lv[NST_MAX_LEVELS];
    hipEvent_t fork = nullptr;
    size_t bytes = 0;           // nst_ctx_bytes: what dev_alloc charged and dev_release has not yet credited
    nst::DevMem mem;            // owns the context's own buffers: weight images, biases, w11k / w11d, color_scratch
    bool single_stream = false;
    // nst_last_closure_schedule: what the last nst_closure* call did - host integers, counted where the forks are recorded
    // (closure_record, batched_forward) and where a captured graph is launched; no launch or stream depends on them
    struct ClosureSchedule { int side_forks = 0, level_streams = 0, graph_replay = 0; } sched;
    // timing
    int timing = 0;
    hipEvent_t t0 = nullptr, t1 = nullptr;
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used = 0;
    std::vector<nst::TimedLaunch> timed;
    bool timed_valid = false;
    bool timed_backward = false; // the pending record is a backward half (nst_closure_backward): its launches and time
                                 // join the totals, the closure was counted with its forward half
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

namespace nst {

// records msg as the context's (ctx = nullptr: the thread's) last error and returns code
int fail(nst_ctx* ctx, int code, const std::string& msg);

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

// ---- timed launches ---------------------------------------------------------------------------
struct Timer {
    nst_ctx* ctx; hipStream_t s; bool on; size_t slot;
    Timer(nst_ctx* c, hipStream_t st, int cls, double flops, int t0 = 0, int t1 = 0, int t2 = 0, int t3 = 0, int t4 = 0,
          int t5 = 0)
        : ctx(c), s(st), on(false), slot(0) {
        if (c->timing >= 2 && (c->timing < 3 || cls == K_CONV3) && c->sample_now && c->ev_used + 2 <= c->ev_pool.size()) {
            on = true;
            TimedLaunch t{c->ev_pool[c->ev_used], c->ev_pool[c->ev_used + 1], cls, flops, {t0, t1, t2, t3, t4, t5}, -1.0, H2Shape{}};
            c->ev_used += 2;
            slot = c->timed.size();
            c->timed.push_back(t);
            (void)hipEventRecord(t.a, st);
        }
    }
    ~Timer() { if (on) (void)hipEventRecord(ctx->timed[slot].b, s); }
    // a launch whose matrix-pipe work per algorithmic FLOP differs from its arithmetic mode's (the Winograd form: 2/3 of it)
    void mfma_factor(double f) { if (on) ctx->timed[slot].mfma_factor = f; }
    void shape(const H2Shape& sh) { if (on) ctx->timed[slot].shape = sh; }
};
// folds the event pairs of the previous closure into the accumulators (waits for them to complete)
int fold_timed(nst_ctx* ctx);

// ---- nst_ctx.cpp: device memory (nst_devmem.h), workspace, stream ordering ---------------------------------------------
void poison_if_asked(void* p, size_t bytes);       // a fresh device allocation under NST_POISON_ALLOC: 0xFF bytes if it is one asked for
int zero_now(void* p, size_t bytes);               // a set-up-time zero fill that has RUN when it returns (0: done)
int alloc_acts(nst_ctx* ctx, ActSet& a, int h, int w);
int bind(nst_ctx* ctx);                            // null check + hipSetDevice: first line of every entry point
// what a closure remembered is void once the job changes (captured graph; drop_targets: every level's targets)
void drop_closure_state(nst_ctx* ctx, bool drop_targets);
hipStream_t enter(nst_ctx* ctx, void* stream);     // orders the caller's stream after the context's tail event
void mark(nst_ctx* ctx, hipStream_t s);            // records the tail event
void quiesce(nst_ctx* ctx);                        // waits until nothing on the device uses the context's memory

// Scratch of a standalone call - an ActSet and device buffers that its launches on `s` use: freed on every path out of the
// scope, after the stream has been synchronised.  `return sc.finish();` ends the good path: synchronise, free, then report.
// (Counted in ctx->bytes while the call runs.)
struct Scratch {
    nst_ctx* ctx; hipStream_t s; ActSet acts; DevMem bufs; bool open = true;
    Scratch(nst_ctx* c, hipStream_t st) : ctx(c), s(st) {}
    ~Scratch() { (void)release(); }
    template <typename T>
    int alloc(T** p, size_t count) { return bufs.alloc(ctx, p, count); }
    hipError_t release() {
        if (!open) return hipSuccess;
        open = false;
        const hipError_t e = hipStreamSynchronize(s);
        acts = ActSet();
        bufs.release();
        return e;
    }
    int finish() { const hipError_t e = release(); HIPCHK(ctx, e); return NST_OK; }
};

// ---- nst_closure.cpp: the per-level network walker and Gram, as the standalone entry points use them --------------------
// gradient injected at a tap layer, w.r.t. its post-ReLU activation
struct Inject {
    const float* S = nullptr;        // Gram backward: dF = F * S (1x1 conv of the activation itself)
    const void* S_bf = nullptr;      // the same S cut into bf16 pieces (conv_bf3 weight layout), if available
    const unsigned* S_amax = nullptr; // absmax record of S (conv_h2), if available
    const float* direct = nullptr;   // or a ready NHWC gradient
    bool content = false;            // or the content MSE gradient (closure only)
    const float* bias = nullptr;     // with S, a shifted Gram (nst_job_set_gram_shift) and / or the moment term: the row bias, dF = F * S + r
    const GuidedBwd* guided = nullptr; // guided Gram backward (R, t, S filled in): dF = sum_r t_r^2 F S_r, by a launch of its own
    // (the per-map terms of a level - MapTerm - are not injected: backward() takes the level and asks it per map)
};
struct ContentJob { const float* target; size_t n; float coef; double* partial; };
// channels = 1: x is a luminance plane u, conv1_1 sees x_c = u - mean_c (nst_job_set_color)
int forward(nst_ctx* ctx, ActSet& a, const float* x, int h, int w, hipStream_t s, int last_layer = NL - 1, int channels = 3);
// Backward through the network down to the planar image gradient gx (overwritten).
// inj[l] describes what enters at conv layer l; gbuf: two NHWC scratch buffers of the largest size.  The chain starts at
// layer `top` (nothing above it is read); `top_mask` = false: the top map is pre-ReLU (its gradient passes unmasked).
// channels = 1: gx is the gradient of a luminance plane (the sum over the three channels)
// `terms`: the level (whose maps `a` holds) whose per-map terms join the walk - the gradient of every term a map carries joins
// the addend of that map's launch; nullptr: none (the stand-alone callers)
int backward(nst_ctx* ctx, ActSet& a, const Inject* inj, const ContentJob* cj, float* gbuf0, float* gbuf1, float* gx,
             int h, int w, hipStream_t s, int top = NL - 1, bool top_mask = true, int channels = 3, const LevelWs* terms = nullptr);
// The Gram of one map, the one recipe of every caller outside the batched closure: the partial products (launch_gram_partial,
// gram_nsplit(C, N) splits, timed as K_GRAM) and the finish pass over their slabs (timed as K_OTHER).
struct GramOperand {
    const float* f; size_t N; int C;     // NHWC map, N pixels x C
    const unsigned* amax;                // nullable: absmax record of f; with it the partial products run on the fp16 pipe
    const float* guide;                  // nullable: guidance plane t(p) of the N pixels (the guided Gram; amax required)
    float* part;                         // slab workspace, gram_nsplit(C, N) x C x C floats
    float divisor;
    const float* offset = nullptr;       // gram_shifted_of only: o[C], `amax` then the record of the shifted operand
};
// What the finish pass makes of G = (sum of the slabs) / divisor.  alpha < 0, launch_gram_finish: gram_out = G, and with a
// target S = coef (G - target) (S_bf / S_amax: its bf16 cut / absmax record) and the partial sums of (G - target)^2 - all
// nullable.  alpha >= 0, launch_gram_finish_blend: gram_out = alpha G, or gram_out + alpha G when `accumulate`.
struct GramFinish {
    const float* target = nullptr; float coef = 0.f;
    float* S = nullptr; unsigned short* S_bf = nullptr; unsigned* S_amax = nullptr; double* mse_partial = nullptr;
    float* gram_out = nullptr;
    float alpha = -1.f; int accumulate = 0;
};
// timed = false: the two launches without their timers (nst_window_begin)
int gram_of(nst_ctx* ctx, const GramOperand& op, const GramFinish& fin, hipStream_t s, bool timed = true);
// The shifted Gram of one map (nst_job_set_gram_shift): offsets and operand record (launch_gram_offsets) -> gram_of on the
// shifted operand -> the row bias r = o S (when r and fin.S are given).  offset: C floats, rec: NST_AMAX_SLOTS words, sums:
// GS_PART_DOUBLES doubles (a centred map).  The fp16-piece kernels only: op.amax is required (op.guide / op.offset unused).
struct ShiftedGram { float shift; int center; float* offset; unsigned* rec; double* sums; float* r; };
int gram_shifted_of(nst_ctx* ctx, const GramOperand& op, const ShiftedGram& sg, const GramFinish& fin, hipStream_t s);
// A full-resolution map of `level` that its last batched forward pass left out: that layer's launch again, over the levels
// of that pass (same ConvBatch, so the same tile shape and summation order), with `out` set.  The pooled map, mask and code
// words it rewrites are the values they hold; the absmax records stay (atomicMax of the same values).
int restore_map(nst_ctx* ctx, int level, int layer, hipStream_t s);
// the job changed: no forward pass is remembered (nst_level_activation copies what the buffers hold, as before any pass)
void forget_forward_pass(nst_ctx* ctx);
// floats of the partial-Gram workspace of one h x w image under these taps (the style layers one after the other)
size_t gram_part_floats_for(const Taps& tp, int h, int w);

}  // namespace nst
#pragma GCC visibility pop
