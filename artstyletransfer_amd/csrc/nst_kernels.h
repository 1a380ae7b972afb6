// nst_kernels.h - internal launch interface between the C-ABI layer (nst_api.cpp) and the
// gfx950 kernels.  Activations inside the network are NHWC fp32 ("pixel-major": [y][x][C]);
// the optimised image, its pyramid levels and their gradients are planar (3,h,w) fp32, the
// storage of the torch tensor the reference optimises.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace nst {

struct ConvParams {
    const float* in;      // [H][W][Cin]
    const float* wt;      // [TAPS][Cout][Cin]
    const void* wt_bf;    // conv_bf3 only: [9][Cout][Cin/32][3 pieces][32] bf16 (see conv_bf3.hip)
    const float* bias;    // [Cout] or nullptr
    const float* addend;  // [H][W][Cout] or nullptr (may alias out)
    const float* mask;    // [H][W][Cout] or nullptr: out = mask > 0 ? v : 0
    float* out;           // [H][W][Cout]
    int H, W, Cin, Cout;
    int relu;
    int tiles_x, tiles_y; // filled by the launcher
    float* partial;       // split-K workspace (nullable): [ksplit][H][W][Cout]
    size_t partial_floats;
    int ksplit;           // filled by the launcher
    // conv_bf3 only ------------------------------------------------------------------------------
    const float* in2;     // optional second K source [H][W][Cin2], accumulated as a 1x1 product with wt2_bf
    int Cin2;
    const void* wt2_bf;   // [1][Cout][Cin2/32][3][32] bf16
    unsigned* bits_out;   // optional: ReLU bit-mask of the output, [H*W][Cout/32] words (bit = channel & 31)
    const unsigned* bits_in;  // optional: replaces `mask` (same layout, of the tensor the gradient flows into)
    float* pool_out;      // optional: 2x2/2 max-pooled output [H/2][W/2][Cout]
    // conv_h2 only (bits_out / bits_in / pool_out / in2 / Cin2 above apply too) -------------------------
    const void* wt_h2;    // [9][Cout][Cin/32][2 pieces][32] fp16, the weights times 1/wt_h2_inv (see conv_h2.hip)
    float wt_h2_inv;      // power of two: true weight = (hi + lo 2^-11) * wt_h2_inv
    const float* wt2_f32; // weights of the second K source, fp32 [Cout][Cin2] (cut in the kernel)
    const unsigned* amax_in;   // NST_AMAX_SLOTS words: absmax of `in` (float bit patterns, max over the slots)
    const unsigned* amax_in2;  // ... of `in2`
    const unsigned* amax_w2;   // ... of `wt2_f32`
    unsigned* amax_out;        // optional: absmax of `out` is recorded here (atomic max; zero it beforehand)
    // un-pooling fused into the operand loader (input-gradient launches that follow a max-pool): `in` is then the
    // gradient w.r.t. the POOLED map, [H/2][W/2][Cin], and pcode_in the arg-max code of that pool
    // ([H/2*W/2][Cin/32][4 window positions] words, bit = channel & 31: set where that position held the window's
    // first maximum and it was positive); pcode_out: a forward launch with pool_out writes that code
    const unsigned* pcode_in;
    unsigned* pcode_out;
    int in2_row0, in2_rows;    // in2_rows > 0: the second source contributes on output rows [in2_row0, in2_row0 + in2_rows) only
    int ty0;                   // first tile row of this launch (filled by the launcher: tensors from 4 GiB up run in row bands)
    int band_rows;             // conv_h2: >= 16 forces row bands of that many rows (nst_options.h2_band_rows; 0 = only when needed)
    int mfma16;                // conv_h2: the 32-channel-chunk shapes run on v_mfma_f32_16x16x32_f16 (nst_options.h2_mfma16)
    int wg256;                 // conv_h2: the 16x16 x 128 tile as 4 waves of 64 x 128 (nst_options.h2_wg256)
    int tile_rows;             // conv_h2: 4 / 8 / 16 forces that tile height on the 128-channel shapes (nst_options.h2_tile_rows)
    // nst_job_set_pooling(NST_POOL_AVG): pool_out is the 2x2/2 AVERAGE, ((e00 + e01) + e10) + e11 times 1/4, and pcode_out the
    // multi-hot code bit q = (e_q > 0) (launch-uniform: a scalar branch in the epilogues).  The un-pooling loaders test every
    // position's bit on its own and are the same for both; the 1/4 of the average's backward rides on wt_h2_inv.
    int pool_avg;
    // conv_h2, forward launches of the 16-channel-chunk shapes (nst_ctx_set_h2_direct_weights): the pieces of wt_h2 in MFMA
    // FRAGMENT order (conv_h2.hip, DIRECT; make_h2_frag has the layout); nullptr: the weight slices go through LDS
    const void* wt_h2_frag;
};

// nst_ctx_set_h2_direct_weights' default: the shapes whose forward launches run the DIRECT K loop (bit 0: <16,64,2,16>, bit 1:
// <8,128,2,16>), decided per shape from the kernel traces of profiles/r21_h2_direct_weights.txt
#ifndef NST_H2_DIRECT_DEFAULT
#define NST_H2_DIRECT_DEFAULT 3
#endif
constexpr int NST_AMAX_SLOTS = 64;
// conv_h2: launches with at most this many input channels (K <= 1152) use the 16-channel-chunk shapes, and the
// host lays their pre-cut weights out in 16-channel chunks (make_h2)
#ifndef NST_H2_SHORTK_CIN_VALUE
#define NST_H2_SHORTK_CIN_VALUE 128
#endif
constexpr int NST_H2_SHORTK_CIN = NST_H2_SHORTK_CIN_VALUE;      // (-DNST_H2_SHORTK_CIN_VALUE=512: experiment builds)

// One image (pyramid level) of a batched conv_bf3 / conv_h2 launch; the layer's weights / channel counts are shared.  conv_h2
// has no other form: a lone image, and each row band of one, is a batch of one.
struct ConvImage {
    const float* in;
    const float* addend;
    const float* mask;
    float* out;
    const float* in2;
    const void* wt2_bf;
    unsigned* bits_out;
    const unsigned* bits_in;
    float* pool_out;
    int H, W;
    int tiles_x, tile_end;   // filled by the launcher
    // conv_h2 only
    int ty0;                 // first tile row of the image in this launch (filled by the launcher: 0, or a row band's first)
    const float* wt2_f32;
    const unsigned* amax_in;
    const unsigned* amax_in2;
    const unsigned* amax_w2;
    unsigned* amax_out;
    const unsigned* pcode_in;
    unsigned* pcode_out;
    int in2_row0, in2_rows;
    const float* bias;       // conv_h2 only: this image's bias [Cout] (the row bias of a shifted Gram backward); nullptr: ConvBatch::bias
};
struct ConvBatch {
    ConvImage img[8];
    int n;
    const void* wt_bf;
    const float* bias;
    int Cin, Cout, Cin2, relu;
    const void* wt_h2;       // conv_h2 only
    float wt_h2_inv;
    int unpool;              // every image's `in` is a pooled gradient to be un-pooled through pcode_in
    int mfma16, wg256, tile_rows;   // conv_h2: see ConvParams
    int persist;             // conv_h2: in: nst_options.h2_persist; the launcher clears it where the persistent form does not apply
    int total_tiles;         // conv_h2: filled by the launcher (tiles x output-channel tiles)
    const void* wt_wino;     // conv_wino: the layer's transformed weights in fragment order (nullptr: none)
    float wt_wino_inv;
    int pool_avg;            // see ConvParams
    const void* wt_h2_frag;  // conv_h2: see ConvParams (nullptr: none)
};

// conv_wino.hip: forward 3x3 convolution as 1-D Winograd F(2,3) in the f16x2 arithmetic (nst_options.h2_winograd)
hipError_t conv_wino_init_device();
bool conv_wino_eligible(const ConvBatch& b);
hipError_t launch_conv_wino_batch(const ConvBatch& b, hipStream_t stream);

// conv_mfma.hip
hipError_t conv_mfma_init_device();
hipError_t launch_conv_mfma(const ConvParams& p, int taps, hipStream_t stream);
// number of channel-chunk splits launch_conv_mfma uses for a 3x3 layer of this shape (1 = none)
int conv_ksplit(int H, int W, int Cin, int Cout);

hipError_t launch_conv_splitk_finish(const ConvParams& p, hipStream_t stream);

// conv_bf3.hip: the same 3x3 convolution on the bf16 matrix pipe with 3-piece operands (fp32-level accuracy)
hipError_t conv_bf3_init_device();
hipError_t launch_conv_bf3(const ConvParams& p, hipStream_t stream);
hipError_t launch_conv_bf3_batch(const ConvBatch& b, hipStream_t stream);
int conv_bf3_ksplit(int H, int W, int Cin, int Cout);

// conv_h2.hip: the same on the fp16 matrix pipe with 2-piece scaled operands (3 MFMAs per product block)
hipError_t conv_h2_init_device();
// The kernel shape a conv_h2 launch ran as - conv_h2_batch_kernel<rows, bn, ntw, chunk> (conv_h2.hip lists the shapes) - and the
// properties of the launch that entered the choice.  Decided in ONE place (h2_launch_shape) for both launchers, which hand it
// back through `shape` (nullable): what the timing record of a launch keeps (nst_last_closure_launches).  rows = 0: not a
// conv_h2 launch.
struct H2Shape {
    int rows, bn, ntw, chunk;   // pixel rows of the workgroup tile (x 16 columns), output channels per tile, 32-channel tiles per wave, channels per K chunk
    int m16;                    // the 16x16x32 MFMA form
    int persist;                // persistent workgroups (launch_conv_h2_batch only)
    int second, unpool;         // the launch has a second K source / un-pools its input in the loader
    int bands;                  // kernel launches it took (per-level launcher: one one-image batch per row band; else 1)
    int direct;                 // the DIRECT K loop: B fragments from the layer's fragment-order image (ConvParams::wt_h2_frag)
};
hipError_t launch_conv_h2(const ConvParams& p, hipStream_t stream, H2Shape* shape = nullptr);
hipError_t launch_conv_h2_batch(const ConvBatch& b, hipStream_t stream, H2Shape* shape = nullptr);
// absmax of n floats into NST_AMAX_SLOTS slots (atomic max; zero them beforehand)
hipError_t launch_absmax_slots(const float* x, size_t n, unsigned* slots, hipStream_t stream);

// conv_first.hip: conv1_1 (3 -> 64) forward from the planar image, and its input gradient
// wk: [28][64] (k = c*9 + ky*3 + kx, row 27 zero); bias [64]; out NHWC 64, ReLU applied.
// bits_out (nullable): ReLU bit-mask of the output, [H*W][2] words; amax_out (nullable): NST_AMAX_SLOTS words
// receiving the absmax of the output (atomic max).  channels = 1 (luminance mode): x is one plane u (1,H,W) and the
// convolution sees x_c = u - mean_c (bitwise the channels = 3 result at that planar image)
hipError_t launch_conv1_1_fwd(const float* x, int H, int W, const float* wk, const float* bias, float* out,
                              unsigned* bits_out, unsigned* amax_out, hipStream_t stream, int channels = 3);
// The same for every pyramid level of a pass in ONE launch: the persistent tile loop walks the tiles of image 0, then image
// 1, ... (tile_end: the prefix, as ConvBatch's), so the small levels - which cannot fill the chip with two workgroups per CU
// of their own - ride in the tail of the big one.  Every image keeps its outputs, mask words and absmax slots; each output
// element is computed as launch_conv1_1_fwd computes it (a record's maximum may land in another slot).
struct Conv1Image {
    const float* x; float* out; unsigned* bits_out; unsigned* amax_out;
    int H, W;
    int tiles_x, tile_end;   // filled by the launcher
};
struct Conv1Batch { Conv1Image img[8]; int n; const float* wk; const float* bias; int channels; };
hipError_t launch_conv1_1_fwd_batch(const Conv1Batch& b, hipStream_t stream);
// g: [H][W][64] gradient w.r.t. the pre-ReLU conv1_1 output; wd: [9][64][4] flipped taps
// (wd[t][co][c] = W[co][c][2-ky][2-kx], c = 3 unused 0); gx planar (3,H,W), overwritten.
// amax_g: the absmax slots of g (the matrix-pipe form), or null (fp32 on the VALU).  channels = 1 (luminance mode):
// gx is one plane, the sum over c of the three (added in fp32, (c0 + c1) + c2)
hipError_t launch_conv1_1_dgrad(const float* g, int H, int W, const float* wd, const unsigned* amax_g, float* gx,
                                hipStream_t stream, int channels = 3);

// pixel_ops.hip ---------------------------------------------------------------------------------
// 2x2/2 max pool (floor) over NHWC, C % 4 == 0
hipError_t launch_maxpool_fwd(const float* in, int H, int W, int C, float* out, hipStream_t stream);
// gin[y][x][c] = (a[y][x][c] is the first maximum of its window and a > 0) ? gpool[y/2][x/2][c] : 0
// (max_pool2d backward fused with the ReLU mask of the activation `a` that was pooled)
hipError_t launch_maxpool_bwd_relu(const float* a, const float* gpool, int H, int W, int C, float* gin,
                                   hipStream_t stream);
// 2x2/2 average pool (floor) over NHWC, C % 4 == 0: ((e00 + e01) + e10) + e11, times 1/4 (the order of every pooling kernel)
hipError_t launch_avgpool_fwd(const float* in, int H, int W, int C, float* out, hipStream_t stream);
// gin[y][x][c] = a[y][x][c] > 0 ? gpool[y/2][x/2][c] / 4 : 0 (avg_pool2d backward fused with the ReLU mask of the
// activation `a` that was pooled; the odd last row / column gets zeros)
hipError_t launch_avgpool_bwd_relu(const float* a, const float* gpool, int H, int W, int C, float* gin,
                                   hipStream_t stream);
// planar (C,h,w) <-> NHWC
hipError_t launch_chw_to_hwc(const float* src, int C, int H, int W, float* dst, hipStream_t stream);
hipError_t launch_hwc_to_chw(const float* src, int C, int H, int W, float* dst, hipStream_t stream);
// dst = (src > 0 ? g : 0) elementwise over n floats (n % 4 == 0)
hipError_t launch_relu_mask(const float* act, const float* g, size_t n, float* dst, hipStream_t stream);
// dst += src over n floats
hipError_t launch_add_inplace(float* dst, const float* src, size_t n, hipStream_t stream);

// general bicubic (A=-0.75, align_corners=False, clamped taps) down-sample of planar (C,h,w) to
// (C,oh,ow) and its transpose; the pyramid uses oh=h/2, ow=w/2.
hipError_t launch_bicubic_down(const float* x, int C, int h, int w, int oh, int ow, float* y, hipStream_t stream);
// gx (C,h,w): accumulate != 0 -> gx += transpose(gy), else gx = transpose(gy)
hipError_t launch_bicubic_down_bwd(const float* gy, int C, int h, int w, int oh, int ow, float* gx, int accumulate,
                                   hipStream_t stream);

// total variation: partial sums of |dx| and |dy| (NST_TV_BLOCKS x 2 doubles in `partial`)
constexpr int TV_BLOCKS = 1024;
// row window [row0, row0 + rows) of every channel (rows <= 0: all rows): the sums / the gradient of those rows only
hipError_t launch_tv_partial(const float* y, int C, int h, int w, double* partial, hipStream_t stream, int row0 = 0,
                             int rows = 0);
// Several images (the pyramid levels of a pass) in one launch each: launch_tv_partial of every image (all rows), and the
// means-only form of launch_tv_finish (grad = nullptr) - image i's TV_BLOCKS workgroups / one workgroup do what the launch of
// its own does, on its own partial buffer
struct TvBatch { const float* y[8]; int h[8], w[8]; double* partial[8]; float* means[8]; int n; int C; };
hipError_t launch_tv_partial_batch(const TvBatch& b, hipStream_t stream);
hipError_t launch_tv_means_batch(const TvBatch& b, hipStream_t stream);
// reduces the partials (fixed order), writes means to scal[0..1]; if grad: grad (+)= weight * d tv/dy
hipError_t launch_tv_finish(const float* y, int C, int h, int w, const double* partial, float weight, float* grad,
                            int accumulate, float* means, hipStream_t stream, int row0 = 0, int rows = 0,
                            const float* given_means = nullptr, double nx = 0, double ny = 0);

// content: sum((a - t)^2) partials and, if g != nullptr, g = coef * (a - t) (coef = cw*2/n)
constexpr int MSE_BLOCKS = 256;
hipError_t launch_mse_grad(const float* a, const float* t, size_t n, float coef, float* g, double* partial,
                           hipStream_t stream);

// the partial sums alone (g = nullptr) of several pairs in one launch: pair i's MSE_BLOCKS workgroups as launch_mse_grad's
struct MseBatch { const float* a[8]; const float* t[8]; size_t cnt[8]; double* partial[8]; int n; };
hipError_t launch_mse_partial_batch(const MseBatch& b, hipStream_t stream);

// scalar plumbing of the stripe closure (pixel_ops.hip)
hipError_t launch_sum_doubles(const double* p, int n, int stride, int offset, float* out, hipStream_t stream);
hipError_t launch_window_scalars(const float* sums, double nx, double ny, float* means, double* partial, int n,
                                 hipStream_t stream);

// prepare / unprepare
hipError_t launch_prepare_img(const float* hwc, int h, int w, float* chw, hipStream_t stream);
hipError_t launch_unprepare_img(const float* chw, int h, int w, float* hwc, hipStream_t stream);

// laplacian.hip: the Laplacian loss (include/nst_hip.h has the definition) ----------------------------------------
constexpr int NST_LAP_MAX = 4;       // = NST_MAX_LAPLACIAN
constexpr int LAP_BLOCKS = 256;      // SSE partials of one entry
// s (h / p, w / p) = sum over the channels of the p x p / p mean pool of planar y (C,h,w), C = 3, or 1 = a luminance plane
// whose three channels pool alike (s = 3 P_p(u)); cell sums in double, s kept in double
hipError_t launch_lap_pool(const float* y, int C, int h, int w, int p, double* s, hipStream_t stream);
// target nullptr: target_out (hk-2, wk-2) = D s.  Else r = (float)(D s - target) and partial: LAP_BLOCKS doubles, sums of r^2
hipError_t launch_lap_stencil(const double* s, int hk, int wk, const double* target, double* target_out, float* r, double* partial,
                              hipStream_t stream);
// out[0] = (float)(sum of the LAP_BLOCKS partials / n)
hipError_t launch_lap_value(const double* partial, double n, float* out, hipStream_t stream);
// grad (C,h,w) (+)= sum_k coef[k] (D^T r[k])(i / p[k], j / p[k]) over the cells' pixels, ascending k; the caller sets K, p,
// coef and r, the launcher fills the rest
struct LapBackward {
    int K;
    int p[NST_LAP_MAX];
    float coef[NST_LAP_MAX];
    const float* r[NST_LAP_MAX];         // residuals, (h / p - 2, w / p - 2)
    int hk[NST_LAP_MAX], wk[NST_LAP_MAX];
    unsigned magic[NST_LAP_MAX];         // ceil(2^32 / p): j / p as a multiply-high
};
hipError_t launch_lap_backward(const LapBackward& lb, int C, int h, int w, float* grad, int accumulate, hipStream_t stream);

// matting.hip: the matting-Laplacian regulariser (include/nst_hip.h has the definition) -------------------------------
// guide (C,h,w): gscale * guide is the guide I up to a constant per channel (1 / 255: the level's prepared content; 1: I
// itself).  C = 3, or 1 = a luminance plane under a one-plane guide (the scalar reduction, epsilon / 3).
int mat_tiles(int h, int w);         // tile partials of one image (0: smaller than 3x3)
// partial: mat_tiles(h, w) doubles, partial[t] = sum of E_kc over the windows of tile t (fixed order)
hipError_t launch_mat_forward(const float* y, const float* guide, int C, int h, int w, double gscale, double eps, double* partial,
                              hipStream_t stream);
// grad (C,h,w) (+)= coef * sum over the windows k of a pixel of (Vc_i - a_kc^T Ic_i); the windows are computed again
hipError_t launch_mat_backward(const float* y, const float* guide, int C, int h, int w, double gscale, double eps, float coef,
                               float* grad, int accumulate, hipStream_t stream);
// out[0] = (float)(sum of the tile partials / n), in the order of the loss rows
hipError_t launch_mat_value(const double* partial, int tiles, double n, float* out, hipStream_t stream);

// temporal.hip: the temporal consistency term, the warp and the flow weights (include/nst_hip.h has the definitions) ----
constexpr int ANCHOR_BLOCKS = 256;   // value partials of one image: the fixed grid of the forward half
int anchor_block_elems();            // elements one block covers per pass of its grid-stride loop (threads x lane width)
// partial: ANCHOR_BLOCKS doubles, partial[b] = block b's share of sum c d^2, d = y - a (fixed order); c nullptr: ones
hipError_t launch_anchor_forward(const float* y, const float* a, const float* c, int C, int h, int w, double* partial,
                                 hipStream_t stream);
// out[0] = (float)(sum of the block partials / n), in the order of the loss rows
hipError_t launch_anchor_value(const double* partial, int blocks, double n, float* out, hipStream_t stream);
// grad (C,h,w) (+)= coef * (c * (y - a)), the difference formed again; accumulating, a term of exactly 0 leaves grad's bits
hipError_t launch_anchor_backward(const float* y, const float* a, const float* c, int C, int h, int w, float coef, float* grad,
                                  int accumulate, hipStream_t stream);
// out (C,h,w) = src sampled bilinearly at p + flow(p) (flow (2,h,w): dx, dy in pixels); valid (h,w) nullable
hipError_t launch_warp_bilinear(const float* src, const float* flow, int C, int h, int w, float* out, float* valid,
                                hipStream_t stream);
// out (h,w) = the reliability plane c of a forward / backward flow pair
hipError_t launch_flow_weights(const float* fwd, const float* bwd, int h, int w, float* out, hipStream_t stream);
// the long-term anchor: J sources (C,h,w) under J weight planes (h,w), in ascending order of frame offset -> anchor (C,h,w),
// weight (h,w) and, if asked for, the parts l_j (J,h,w).  The 2 J pointers travel by value as one kernel argument.
constexpr int NST_FOLD_MAX_SOURCES = 8;   // = NST_MAX_ANCHOR_SOURCES
struct AnchorFoldArgs {
    const float* sources[NST_FOLD_MAX_SOURCES];
    const float* weights[NST_FOLD_MAX_SOURCES];
};
hipError_t launch_anchor_fold(const AnchorFoldArgs& a, int J, int C, int h, int w, float* anchor, float* weight,
                              float* parts /* nullable */, hipStream_t stream);
// which planes take 16-byte accesses: bits 0..2 plane ch of every source and of the anchor, bit 3 the weight planes in and
// out, bit 8 + j plane j of parts
unsigned anchor_fold_vec_mask(const AnchorFoldArgs& a, int J, int C, size_t hw, const float* anchor, const float* weight,
                              const float* parts);

// flow.hip: multi-scale Horn-Schunck optical flow with warping (include/nst_hip.h, nst_flow_estimate, has the definitions) ----
constexpr int NST_FLOW_MAX_SCALES = 12;   // = NST_MAX_FLOW_SCALES
// The scales of one estimate and where its planes lie in the caller's workspace (offsets in floats, multiples of 4).
struct FlowLayout {
    int scales;                                                 // scales in use, scale 0 = the images themselves
    int h[NST_FLOW_MAX_SCALES], w[NST_FLOW_MAX_SCALES];
    size_t from[NST_FLOW_MAX_SCALES], to[NST_FLOW_MAX_SCALES];  // the reduced planes of scale s >= 1
    size_t ix, iy, rho;                                         // the linearisation, h w floats each, shared by the scales
    size_t other;                                               // the second flow buffer, 2 h w floats
    size_t floats;                                              // the whole workspace
};
// 0, or -1 for h or w < 1, scales < 0 or above the cap.  scales = 0: as many as fit.  Pure.
int flow_layout(int h, int w, int scales, FlowLayout* out);
// out ((h+1)/2, (w+1)/2) = the 5-tap binomial of in (h,w) along x, then along y, every second pixel
hipError_t launch_flow_reduce(const float* in, int h, int w, float* out, hipStream_t stream);
// fine (2,h,w) = 2 x the two-tap mean per axis of coarse (2,(h+1)/2,(w+1)/2)
hipError_t launch_flow_prolong(const float* coarse, int h, int w, float* fine, hipStream_t stream);
// Ix, Iy, rho (h,w) of the pair at the flow (u, v); zeros where the four taps do not lie inside the image
hipError_t launch_flow_linearize(const float* from, const float* to, const float* u, const float* v, int h, int w, float* Ix,
                                 float* Iy, float* rho, hipStream_t stream);
// n Jacobi sweeps of the flow `in` (2,h,w), one launch each, alternating between `out` and `tmp` so that the last writes `out`;
// tmp may be null for n = 1; the first sweep's target must not be `in`
hipError_t launch_flow_sweeps(const float* Ix, const float* Iy, const float* rho, const float* in, int h, int w, float alpha2, int n,
                              float* out, float* tmp, hipStream_t stream);
// the driver: pyramids, then per scale `warps` x (linearise, `iterations` sweeps), prolong; the result ends in `flow`
hipError_t launch_flow_estimate(const float* from, const float* to, const FlowLayout& l, float alpha2, int warps, int iterations,
                                float* flow, float* ws, hipStream_t stream);

// flow_tvl1.hip: TV-L1 optical flow on the pyramid, warps and linearisation above (include/nst_hip.h, nst_flow_tvl1_estimate) ----
// The workspace of one estimate: flow.hip's, then the two copies of the duals (4 h w floats each) the iterations alternate between.
struct FlowTvl1Layout {
    FlowLayout hs;
    size_t dual[2];
    size_t floats;                                              // the whole workspace
};
// 0, or -1 where flow_layout gives -1.  Pure.
int flow_tvl1_layout(int h, int w, int scales, FlowTvl1Layout* out);
// n iterations of the flow `fin` (2,h,w) and the duals `pin` (4,h,w), one launch each, alternating between (fout, pout) and
// (ftmp, ptmp) so that the last writes (fout, pout); the tmp pair may be null for n = 1; the first iteration's target must not
// be the input.  lt = lambda theta, taut = tau / theta.
hipError_t launch_flow_tvl1_iterations(const float* Ix, const float* Iy, const float* rho, const float* fin, const float* pin, int h,
                                       int w, float lt, float theta, float taut, int n, float* fout, float* pout, float* ftmp,
                                       float* ptmp, hipStream_t stream);
// the driver: pyramids, then per scale zero duals and `warps` x (linearise, `iterations` iterations), prolong; ends in `flow`
hipError_t launch_flow_tvl1_estimate(const float* from, const float* to, const FlowTvl1Layout& t, float lt, float theta, float taut,
                                     int warps, int iterations, float* flow, float* ws, hipStream_t stream);

// loss assembly -----------------------------------------------------------------------------------
constexpr int NST_MAP_TERMS = 4;     // the per-map terms of a level: MRF, histogram loss, relaxed EMD, self-similarity - always in this order
struct LevelLossInputs {
    const double* content_partial;   // MSE_BLOCKS doubles
    size_t content_n;
    const double* style_partial[6];  // gram_finish_blocks(C) doubles each: partial sums of (G-Gt)^2
    int style_c[6];                  // C of each style layer (mse mean over C*C)
    float style_w[6];                // layer weight of each style layer (nst_job_set_style_weights; 1 = the plain mean)
    const float* tv_means;           // 2 floats (mean_x, mean_y)
    int owned;                       // 0: level computed by another rank, its row is written as zeros
    const double* lap_partial[NST_LAP_MAX];   // Laplacian entries: LAP_BLOCKS doubles each, partial sums of r_k^2
    double lap_n[NST_LAP_MAX];       // (hk-2)(wk-2) of each entry
    const double* mat_partial;       // matting term: mat_tiles doubles, partial sums of E_kc
    int mat_tiles;
    double mat_n;                    // channels (h-2)(w-2)
    const double* mom_loss;          // moment term: style slot k's (mean_i, std_i) as the fold left them, at k * mom_stride
    // temporal term (nst_level_set_anchor), a level's own: ANCHOR_BLOCKS doubles, partial sums of c d^2; the weight (0: the
    // level has no anchor and its row is what it is without the term); channels h w; where the unweighted tmp goes
    const double* tmp_partial;
    float tmp_gamma;
    double tmp_n;
    float* tmp_out;
    // the per-map terms, a level's own, in the order the row adds them: MRF (nst_level_set_patches), histogram loss
    // (nst_level_set_histograms), relaxed EMD (nst_level_set_remd), self-similarity (nst_level_set_selfsim).  Each: the six unweighted values by map index as the
    // forward half left them (nullptr: the level has no such term and its row is what it is without it), and the weights (0:
    // the map has no term)
    struct MapTerm { float* vals; float w[6]; } term[NST_MAP_TERMS];
};
struct LossAssembly {
    LevelLossInputs lv[8];
    int levels;
    int nstyle;                      // style layers in use (1..6): the style term is (sum_k w_k mse_k) / nstyle
    float cw, sw, tvw;
    float* out;                      // 4*levels + 1
    int nlap;                        // Laplacian entries (nst_job_set_laplacian); 0: the row is what it is without the term
    float lap_gamma[NST_LAP_MAX];
    float* lap_out;                  // levels x NST_LAP_MAX: the unweighted lap_k (zeros for levels not owned, unused entries)
    float mat_gamma;                 // matting term (nst_job_set_matting); 0: the row is what it is without the term
    float* mat_out;                  // levels: the unweighted mat (zeros for levels not owned)
    int mom_on;                      // moment term (nst_job_set_moments); 0: the row is what it is without the term
    float mom_wm[6], mom_ws[6];      // per style slot: the weights of mean_i and std_i (both 0: the slot has no term)
    int mom_stride;                  // doubles between two slots' values in LevelLossInputs::mom_loss
    int mom_index[6];                // per style slot: its map's index in Vgg19.layer_names
    float* mom_out;                  // levels x 6 x 2: the unweighted (mean_i, std_i) by map index (zeros: not owned, unused maps)
};
hipError_t launch_loss_assemble(const LossAssembly& la, hipStream_t stream);

// gram.hip -----------------------------------------------------------------------------------------
// partial Gram of NHWC f (N pixels x C): slabs part[s][C][C] (upper-triangle tiles only)
hipError_t gram_init_device();
int gram_nsplit(int C, size_t N);
// amax (nullable): NST_AMAX_SLOTS-word absmax record of f -> the fp16-piece kernel (3 MFMAs per product block)
// guide (nullable): the guided Gram sum_p t(p)^2 F(p) F(p)^T - every staged pixel row is scaled by t(p) in [0,1] (so the
// map's absmax still bounds the operand); the fp16-piece kernels only (amax required, C = 64 or a multiple of 128)
// offset (nullable; not with guide): the shifted Gram sum_p (F(p) + o)(F(p) + o)^T, o = offset[C]; `amax` is then the record
// of the shifted operand that launch_gram_offsets writes; the fp16-piece kernels only
hipError_t launch_gram_partial(const float* f, size_t N, int C, int nsplit, const unsigned* amax, float* part,
                               hipStream_t stream, const float* guide = nullptr, const float* offset = nullptr, int pack = 1);
// G = (sum_s part[s]) / divisor (fixed order).  If target: mse_out[0] = sum((G-Gt)^2) (double) and
// S = coef * (G - Gt) (C x C, for the backward 1x1 conv).  gram_out / target / S / mse_partial nullable;
// mse_partial: gram_finish_blocks(C) doubles.  `nslabs` = gram_nslabs(C, nsplit).
int gram_nslabs(int C, int nsplit);
// Several Gram matrices in two partial launches (one per tile shape; a plain batch under `pack`: one for both) + one finish
// launch.  pack (nst_ctx_set_gram_pack): the kernels that skip the below-diagonal blocks of a diagonal tile.  Per item the caller sets
// f, N, C, amax, part (its own gram_nsplit(C, N) x C x C floats) and the finish arguments; the rest is filled in.
#ifndef NST_GRAM_BATCH_MAX
#define NST_GRAM_BATCH_MAX 16      // (include/nst_hip.h states the same number for nst_gram_batch)
#endif
struct GramItem {
    const float* f; size_t N; int C; const unsigned* amax; float* part;
    float divisor; const float* target; float coef; float* gram_out; float* S; unsigned short* S_bf; unsigned* S_amax;
    double* mse_partial;
    int nsplit; size_t pix_per_split; int part_end, finish_end;     // filled by the launcher
    const float* guide;   // guided Gram (gram_guided.hip): t(p) of the N pixels, the staged pixel row is scaled by it; nullptr: plain
    const float* offset;  // shifted Gram (gram_shift.hip): o[C] added to every staged value, `amax` the shifted operand's record; nullptr: plain
};
struct GramBatch { GramItem it[NST_GRAM_BATCH_MAX]; int n; };
// what the launcher filled in for item i of the caller's batch: its splits (= slabs) and the pixels of one split
struct GramGeometry { int nsplit; size_t pix_per_split; };
// geo (nullable): b.n entries, the geometry of every item as launched
hipError_t launch_gram_batch(const GramBatch& b, hipStream_t stream, int pack = 1, GramGeometry* geo = nullptr);
#define NST_GRAM_FINISH_EPB 128      // elements of G a block of the finish pass owns (one partial sum of (G-Gt)^2 each)
int gram_finish_blocks(int C);
// S_amax (nullable): NST_AMAX_SLOTS words receiving the absmax of S (atomic max; zero them beforehand).
hipError_t launch_gram_finish(const float* part, int nslabs, int C, float divisor, const float* target, float coef,
                              float* gram_out, float* S, unsigned short* S_bf, unsigned* S_amax, double* mse_partial,
                              hipStream_t stream);
// The blend form of the finish pass (the targets of a level, nst_level_set_targets_blend): the same sum of the slabs in the
// same order, G = sum / divisor, then gram_out = alpha * G (accumulate = 0) or gram_out = gram_out + alpha * G (accumulate
// != 0), product and sum each rounded to fp32.  alpha = 1 without accumulation writes the bits launch_gram_finish writes.
hipError_t launch_gram_finish_blend(const float* part, int nslabs, int C, float divisor, float alpha, int accumulate,
                                    float* gram_out, hipStream_t stream);

// gram_shift.hip: activation-shifted and mean-centred Gram matrices (include/nst_hip.h has the definition) -----------
// Per item the offsets o[C] - center: o_c = -(1/N) sum_p F[p][c], the sums in double through two ordered stages (no atomics:
// bitwise reproducible); else o_c = shift for every c, without a pass over the map - and the NST_AMAX_SLOTS-word record of
// the shifted operand, absmax(F) + max_c |o_c| rounded up: a bound of |F + o| whatever the signs of F.  One launch pair
// covers all items.  C: 64 or a multiple of 128, at most 1024 - the launcher's own limit: `offset` is the caller's, C floats
// (a context's per-slot buffers hold GS_MAX_C; nst_ctx.h asserts that the network's maps fit).
constexpr int GS_PART_DOUBLES = 128 * 1024;     // stage-one partial sums of one item: gram_offset_blocks(C, N) x C doubles at most
struct OffsetItem {
    const float* f; size_t N; int C;
    const unsigned* amax;     // record of f
    float shift; int center;
    float* offset;            // out: C floats
    unsigned* amax_out;       // out: NST_AMAX_SLOTS words
    double* part;             // centred items: GS_PART_DOUBLES doubles of scratch
    int nblk; size_t pix_per_blk; int blk_end;     // filled by the launcher
};
struct OffsetBatch { OffsetItem it[NST_GRAM_BATCH_MAX]; int n; };
int gram_offset_blocks(int C, size_t N);
hipError_t launch_gram_offsets(const OffsetBatch& b, hipStream_t stream);
// r[c] = sum_k o[k] S[k][c] per item (double accumulation in a fixed order): the row bias of the shifted Gram backward,
// dF_p = (F_p + o) S = F_p S + r
struct RowBiasItem { const float* offset; const float* S; float* r; int C; int blk_end; };
struct RowBiasBatch { RowBiasItem it[NST_GRAM_BATCH_MAX]; int n; };
hipError_t launch_gram_row_bias(const RowBiasBatch& b, hipStream_t stream);

// moments.hip: the moment loss - channel means and deviations of the style maps (include/nst_hip.h has the definition) ---
// Per item mu_c = (1/N) sum_p F[p][c], var_c = (1/N) sum_p F[p][c]^2 - mu_c^2 clamped at 0, sigma_c = sqrt(var_c + epsilon):
// the sums in double through two ordered stages (no atomics: bitwise reproducible), one launch pair for all items.
// stat: 2 C doubles, mu then sigma.  mean_out / std_out (nullable, C floats): alpha * (float)mu and alpha * (float)sigma,
// written (accumulate = 0) or added to what is there (product and sum each rounded) - the targets of a blend of styles.
// C: 64 or a multiple of 128, at most 1024.
constexpr int MOM_PART_DOUBLES = 128 * 1024;    // stage-one partial sums of one item: moment_blocks(C, N) x 2 C doubles at most
struct MomentItem {
    const float* f; size_t N; int C;
    double epsilon;
    double* part;             // MOM_PART_DOUBLES doubles of scratch
    double* stat;             // out: 2 C doubles
    float* mean_out; float* std_out;
    float alpha; int accumulate;
    int nblk; size_t pix_per_blk; int blk_end;     // filled by the launcher
};
struct MomentBatch { MomentItem it[NST_GRAM_BATCH_MAX]; int n; };
int moment_blocks(int C, size_t N);
hipError_t launch_moment_stats(const MomentBatch& b, hipStream_t stream);
// The fold of the term into the Gram backward of its map, after the Gram finish pass and the row bias of a shifted Gram (which
// must see S without the diagonal).  Per item, from stat and the targets: loss[0] = mean_i = (1/C) sum_c (mu_c - mu^t_c)^2,
// loss[1] = std_i = (1/C) sum_c (sigma_c - sigma^t_c)^2; a_c = wm 2 (mu_c - mu^t_c) / (C N), b_c = ws 2 (sigma_c - sigma^t_c)
// / (C N sigma_c); S[c][c] += b_c (S_bf, nullable, likewise re-cut); S_amax (nullable): word 0 raised to the new diagonal's
// absmax; bias[c] = (bias0 ? bias0[c] : 0) + (a_c - b_c mu_c), with b_c as the rounded diagonal holds it.  bias0 may be bias.
struct MomentFoldItem {
    const double* stat; const float* mean_t; const float* std_t;
    float* S; unsigned short* S_bf; unsigned* S_amax;
    const float* bias0; float* bias;
    double* loss;             // out: 2 doubles
    size_t N; int C; float wm, ws;
};
struct MomentFoldBatch { MomentFoldItem it[NST_GRAM_BATCH_MAX]; int n; };
hipError_t launch_moment_fold(const MomentFoldBatch& b, hipStream_t stream);

// patch_match.hip: the MRF style term (include/nst_hip.h has the definition) --------------------------------------------
// The dictionary of one style map: the 3x3xC patches of fs (NHWC, hs x ws x C) centred at (1 + a stride, 1 + b stride), entry
// j = a nb + b, m = na nb of them.  pm_dict_geometry fills the integers (false: a map below 3x3, a stride outside 1..8, a C
// other than 64 / 128 / 256 / 512, or more than 2^30 entries); launch_pm_prepare writes the three buffers: the absmax record of
// fs (NST_AMAX_SLOTS words), rq (32 pm_dict_tiles(m) floats: rq_j, zeros behind entry m) and the packed operand
// (pm_packed_bytes(m, C) bytes: both fp16 pieces of every entry in the lane order of the search kernel's row operand - nine
// times the entries' share of the map).
struct PatchDict {
    const float* fs; int hs, ws, C, stride, na, nb, m;
    const unsigned* amax; const float* rq; const void* packed;
};
hipError_t pm_init_device();     // raises the dynamic-LDS limit of the search kernels: once per device, before the first launch there
__host__ __device__ inline int pm_dict_tiles(int m) { return (m + 31) / 32; }
size_t pm_packed_bytes(int m, int C);
bool pm_dict_geometry(int hs, int ws, int C, int stride, PatchDict* d);
hipError_t launch_pm_prepare(const PatchDict& d, double epsilon, unsigned* amax, float* rq, void* packed, hipStream_t stream);
// The norms alone: out[j] = (float)(1 / sqrt(|Q_j|^2 + epsilon)) of the 32 pm_dict_tiles(m) entries of the geometry (zeros behind
// entry m); d.fs and the integers of d are read.  launch_pm_prepare's rq, and - on a stride-1 geometry of the IMAGE map, whose
// entries are the n image patches - the rp_i of the guided search.
hipError_t launch_pm_norms(const PatchDict& d, double epsilon, float* out, hipStream_t stream);
// The semantic descriptors of the guided search (include/nst_hip.h has the definition): planes (R, hm, wm) at the map's
// resolution, R = 1..4; out = `padded` x 4 floats, the descriptors of the stride-`stride` geometry's entries and zeros behind
// them (padded >= the entry count: 32 pm_dict_tiles(m) for a dictionary, n for the image).
hipError_t launch_pm_descriptors(const float* planes, int R, int hm, int wm, int stride, double epsilon, int padded, float* out,
                                 hipStream_t stream);
// The search: nn and score of every 3x3 patch of f (NHWC, h x w x C; amax_f: its absmax record) against the dictionary.  keys:
// (h - 2)(w - 2) 64-bit words of scratch, which the launch clears and the kernel raises by atomicMax; idx / score (nullable):
// what the keys decode to.  (tiles_x, tiles_y, cshift: the launcher's.)  The guidance (all null: the unguided search and its
// kernels): gd = n x 4 descriptors of the image patches, ge = 32 pm_dict_tiles(m) x 4 of the entries, rp = the image patches'
// norms (launch_pm_norms), gamma >= 0; the score is then cos(i, j) + gamma <d_i, e_j>.
struct PatchSearchCore {       // (what the unguided kernels take: their argument block is what it was)
    const float* f; int h, w, C; const unsigned* amax_f;
    PatchDict d;
    unsigned long long* keys;
    int tiles_x, tiles_y, cshift;
};
struct PatchSearch : PatchSearchCore {
    const float* gd; const float* ge; const float* rp; float gamma;
};
hipError_t launch_pm_search(const PatchSearch& p, int* idx, float* score, hipStream_t stream);
// Value and gradient at fixed idx (d.fs and the integers of d are read; entries outside [0, m) are clamped).  The value in two
// ordered stages: PM_VALUE_BLOCKS double partials of sum_i |P_i - Q_idx(i)|^2, then out = (float)(their sum / denom).  The
// gradient in gather form: out (NHWC, the map's shape) = coef sum_taps (F - Fs), written or (accumulate) added.
constexpr int PM_VALUE_BLOCKS = 256;
struct PatchTerm { const float* f; int h, w; const int* idx; PatchDict d; };
hipError_t launch_pm_value_partials(const PatchTerm& t, double* partial, hipStream_t stream);
hipError_t launch_pm_value(const double* partial, double denom, float* out, hipStream_t stream);
hipError_t launch_pm_grad(const PatchTerm& t, float coef, float* out, int accumulate, hipStream_t stream);

// histogram.hip: the histogram loss (include/nst_hip.h has the definition) --------------------------------------------------
// Maps are NHWC, N pixels x C channels, C = 64 / 128 / 256 / 512, N C < 2^31; bins = 2..1024.  lo_hi: C x 2 floats (lo_c, hi_c);
// counts: C x bins uint32; ends: C x bins x 2 floats (start_b, end_b; zeros at empty image bins).
constexpr int HIST_SLAB = 32;               // channels of one workgroup of the counts pass: bins x 32 words of LDS
constexpr int HIST_VALUE_BLOCKS = 2048;     // double partials of the value's first stage
hipError_t hist_init_device();     // raises the dynamic-LDS limit of the counts kernel: once per device, before the first launch there
bool hist_channels_ok(int C);
// range, then counts, of f: both outputs are written whole (lo_hi holds the range keys in between)
hipError_t launch_hist_counts(const float* f, size_t N, int C, int bins, float* lo_hi, unsigned* counts, hipStream_t stream);
// the two ends of every non-empty image bin from the image's counts and the style's record
hipError_t launch_hist_tables(const unsigned* counts, size_t N, const float* s_lo_hi, const unsigned* s_counts, size_t Ns, int C, int bins,
                              float* ends, hipStream_t stream);
// Value and gradient at fixed tables.  The value in two ordered stages: HIST_VALUE_BLOCKS double partials of sum (F - R)^2, then
// out = (float)(their sum / denom).  The gradient: out (the map's shape) = coef (F - R), written or (accumulate) added.
struct HistTerm { const float* f; size_t N; int C, bins; const float* lo_hi; const float* ends; };
hipError_t launch_hist_value_partials(const HistTerm& t, double* partial, hipStream_t stream);
hipError_t launch_hist_value(const double* partial, double denom, float* out, hipStream_t stream);
hipError_t launch_hist_grad(const HistTerm& t, float coef, float* out, int accumulate, hipStream_t stream);

// remd.hip: the relaxed EMD term (include/nst_hip.h has the definition) ------------------------------------------------------
// One side of the term: the samples of f (NHWC, h x w x C) on the stride grid, sample k = pixel ((k / nb) stride, (k % nb) stride),
// count = na nb of them.  remd_side_geometry fills the integers (false: an empty map, a stride outside 1..256, a C other than
// 64 / 128 / 256 / 512, h w C >= 2^31).  amax: the absmax record of f; r: 32 remd_tiles(count) floats, the reciprocal norms
// (launch_remd_norms; zeros behind the last sample); packed: remd_packed_bytes(count, C) bytes, both fp16 pieces of every sample
// in the lane order of the search kernel's row operand (launch_remd_pack) - only a side that is searched as a dictionary needs it.
struct RemdSide {
    const float* f; int h, w, C, stride, na, nb, count;
    const unsigned* amax; const float* r; const void* packed;
};
hipError_t remd_init_device();   // raises the dynamic-LDS limit of the search kernels: once per device, before the first launch there
__host__ __device__ inline int remd_tiles(int count) { return (count + 31) / 32; }
size_t remd_packed_bytes(int count, int C);
bool remd_side_geometry(int h, int w, int C, int stride, RemdSide* s);
hipError_t launch_remd_norms(const RemdSide& s, double epsilon, float* r, hipStream_t stream);
hipError_t launch_remd_pack(const RemdSide& s, void* packed, hipStream_t stream);      // reads s.amax
// One direction of the search: for every sample of `cols` the lowest index among its best samples of `dict` (dict: amax, r and
// packed; cols: amax and r).  keys: cols.count 64-bit words, which the launch clears and the kernel raises by atomicMax; nn:
// cols.count int32, what the keys decode to.
hipError_t launch_remd_search(const RemdSide& dict, const RemdSide& cols, unsigned long long* keys, int* nn, hipStream_t stream);
// Value and gradient at fixed matches (x: the image side, y: the style side; f, the integers and r of both are read; matches
// outside their range are clamped).  The value in two ordered stages: 2 REMD_VALUE_BLOCKS double partials of sum_i a_i and
// sum_j b_j (the first stage also stores the cosines), then rec = (remd, rA, rB) and *side = 0 (A) or 1 (B); force = 0 / 1 takes
// that side whatever the values (remd is then its r), -1 decides; val (nullable) also receives remd.  The gradient in gather
// form, a wave per image sample, reading *side on the device: out (the image map's shape) gets coefA d(i, nnA(i)) or coefB
// sum_j d(i, j) at the sampled pixels - written, everything else zero, or (accumulate) added.
constexpr int REMD_VALUE_BLOCKS = 256;
struct RemdTerm {
    RemdSide x, y;
    const int* nnA; const int* nnB;      // x.count and y.count entries
    float* cosA; float* cosB;            // likewise: (float)a_i and (float)b_j
    float* rec; int* side;               // 3 floats and 1 int
};
hipError_t launch_remd_value(const RemdTerm& t, double epsilon, int force, double* partial, float* val, hipStream_t stream);
hipError_t launch_remd_grad(const RemdTerm& t, float coefA, float coefB, float* out, int accumulate, hipStream_t stream);

// selfsim.hip: the self-similarity content term (include/nst_hip.h has the definition) ----------------------------------------
// The samples are a RemdSide (f, the grid, the absmax record, r from launch_remd_norms, packed from launch_remd_pack) of at
// most SELFSIM_MAX_SAMPLES samples: the term keeps n x n arrays.
constexpr int SELFSIM_MAX_SAMPLES = 4096;
constexpr int SELFSIM_ROW_BLOCKS = 16;
hipError_t selfsim_init_device();   // raises the dynamic-LDS limit of the matrix kernels: once per device, before the first launch there
// D (n x n floats, row-major, row = the dictionary role i, column = the column role j): 0 on the diagonal, else max(0, 1 - c(i,j))
hipError_t launch_selfsim_matrix(const RemdSide& x, float* D, hipStream_t stream);
// s_j = sum_i D_ij (double, two ordered stages; part: SELFSIM_ROW_BLOCKS n doubles) and q_j = 1 / (s_j + epsilon)
hipError_t launch_selfsim_colsums(const float* D, int n, double epsilon, double* part, double* s, double* q, hipStream_t stream);
// Value and decisions: N = D q against M = Dc qc.  sg: n x n int8; part: 2 SELFSIM_ROW_BLOCKS n doubles; t: n doubles; val: one float
struct SelfSimTerm {
    const float* D; const double* q; const float* Dc; const double* qc; int n;
    signed char* sg; double* part; double* t; float* val;
};
hipError_t launch_selfsim_value(const SelfSimTerm& t, hipStream_t stream);
// The gradient at the decisions the value pass left (sg, t): W (n x n floats) and U (n x C floats) are workspace; out (the map's
// shape) gets coef rp_i (g_i - <g_i, u_i> u_i) at the sampled pixels - written, everything else zero, or (accumulate) added.
hipError_t launch_selfsim_grad(const RemdSide& x, const SelfSimTerm& t, float coef, float* W, float* U, float* out, int accumulate,
                               hipStream_t stream);

// xcorr.hip: the long-range style term, Gram matrices of spatially shifted maps (include/nst_hip.h has the definition) ---------
constexpr int XCORR_MAX_SHIFTS = 16;     // (include/nst_hip.h states the same number for nst_level_set_xcorr)
constexpr int XCORR_BATCH_MAX = 32;      // (level, map, shift) items of one launch
constexpr int XCORR_VALUE_MAX = 48;      // (level, map) items of one value launch: NST_MAX_LEVELS x 6
constexpr int XCORR_KP = 32;             // pairs per staged chunk
constexpr int XCORR_FINISH_EPB = 1024;   // elements of G_d per block of the finish pass
hipError_t xcorr_init_device();   // raises the dynamic-LDS limit of the value kernel: once per device, before the first launch there
// How the pairs of one shift are dealt to workgroups: nsplit slabs of pix_per_split consecutive pixels p (whole chunks), a
// function of the shape alone.  false: C other than 64 / 128 / 256 / 512, a shift outside 0 <= dx < w, 0 <= dy < h or (0,0),
// h w C >= 2^31.
struct XcorrGeometry { int nsplit; int pix_per_split; };
bool xcorr_geometry(int C, int h, int w, int dx, int dy, XcorrGeometry* g);
inline int xcorr_finish_blocks(int C) { return C * C / XCORR_FINISH_EPB; }
// One (map, shift): f NHWC with its absmax record; part: nsplit x C x C floats (the slabs); divisor Z_d; G (nullable) gets G_d;
// with a target also S = coef (G_d - target), St its transpose and sq (xcorr_finish_blocks(C) doubles) the partial sums of
// (G_d - target)^2.  launch_xcorr_batch fills the geometry and the block prefixes: one value launch and one finish launch.
struct XcorrItem {
    const float* f; const unsigned* amax; float* part;
    int C, h, w, dx, dy;
    int nsplit, pix_per_split, part_end;
    float divisor;
    const float* target; float coef; float* G; float* S; float* St; double* sq;
    int finish_end;
};
struct XcorrBatch { XcorrItem it[XCORR_BATCH_MAX]; int n; };
hipError_t launch_xcorr_batch(const XcorrBatch& b, hipStream_t stream);
// xcorr_i of a map from its shifts' partials (sq: nd x nblk doubles, cc = C^2): out = (float)((1/nd) sum_d (sum sq_d) / cc)
struct XcorrValueItem { const double* sq; int nd; int nblk; double cc; float* out; };
struct XcorrValueBatch { XcorrValueItem it[XCORR_VALUE_MAX]; int n; };
hipError_t launch_xcorr_values(const XcorrValueBatch& b, hipStream_t stream);
// the term's share of the loss rows, after launch_loss_assemble (NST_MAP_TERMS counts the four terms whose rows that launch adds):
// per level with the term out[4 l] = (out[4 l] + w_1 xcorr_1) + ... in ascending map order, every product and sum rounded, and
// the grand total out[4 levels] formed again from the owned levels' totals in level order, as launch_loss_assemble forms it
// (owned: the level is in the closure's mask; the six values of a level with the term outside it are zeroed)
struct XcorrRows { struct Level { float* vals; float w[6]; int owned; } lv[8]; int levels; float* out; };
hipError_t launch_xcorr_rows(const XcorrRows& r, hipStream_t stream);
// The gradient of one map over all its shifts: S and St are the nd x C x C stacks the finish pass left; out (the map's shape) is
// written, or (accumulate) added to.
struct XcorrGrad {
    const float* f; int h, w, C; int nd; int dx[XCORR_MAX_SHIFTS], dy[XCORR_MAX_SHIFTS];
    const float* S; const float* St; float* out; int accumulate;
};
hipError_t launch_xcorr_grad(const XcorrGrad& g, hipStream_t stream);

// gram_guided.hip: spatial control (guided Gram matrices; include/nst_hip.h has the definitions) ---------------------
constexpr int NST_MAX_REGIONS_K = 4;
constexpr int GUIDE_MASS_BLOCKS = 64;
// one step of the guidance pyramid: out (R,H/2,W/2) = the 2x2/2 mean of in (R,H,W), ((e00 + e01) + e10) + e11 times 1/4
hipError_t launch_guide_pool(const float* in, int R, int H, int W, float* out, hipStream_t stream);
// out[r * 2] = sum_p t_r(p)^2 over the n values of plane r (double, two ordered stages), out[r * 2 + 1] = how many of them
// are not in [0,1] (NaN included); scratch: R * GUIDE_MASS_BLOCKS * 2 doubles
hipError_t launch_guide_mass(const float* t, int R, size_t n, double* scratch, double* out, hipStream_t stream);
// out[b] = sum_r lambda[r] * part[r * blocks + b] (double): the (G - Gt)^2 partials of a guided map's R regions as one set
hipError_t launch_guided_fold(const double* part, int R, int blocks, const float* lambda, double* out, hipStream_t stream);
// Guided Gram backward: out[p][c] = addend[p][c] + sum_r t_r(p)^2 sum_k F[p][k] S_r[k][c] on the fp32 MFMA, then the
// optional ReLU mask (bits: [N][C/32] words, bit = channel & 31; else mask: out = mask > 0 ? v : 0) and absmax record
struct GuidedBwd {
    const float* F; size_t N; int C; int R;
    const float* t[NST_MAX_REGIONS_K];      // N floats each
    const float* S[NST_MAX_REGIONS_K];      // C x C each
    const float* addend;                    // nullable, may alias out
    float* out;
    const unsigned* bits;
    const float* mask;
    unsigned* amax_out;                     // nullable: NST_AMAX_SLOTS words (atomic max; zeroed beforehand)
};
hipError_t launch_guided_bwd(const GuidedBwd& g, hipStream_t stream);

// image_ops.hip: job set-up on the device (pyramid resize, structured-noise initial image) ---------------------
hipError_t launch_resize_hwc(const float* src, int h, int w, int C, float* dst, int oh, int ow, hipStream_t stream);
hipError_t launch_gather_rows(const float* src, const long long* perm, size_t n, int C, float* dst, hipStream_t stream);
hipError_t launch_gauss_mask_acc(float* acc, const float* src, int h, int w, int C, double central, double peripheral,
                                 double disp, hipStream_t stream);
// weight (double, h*w*C) = 5 nf / (5 + blur(clip(|sobel5(content)|, 0, 100))); tmp0/tmp1: h*w*C doubles each
hipError_t launch_blend_weight(const float* content, int h, int w, int C, double noise_factor, double* tmp0, double* tmp1,
                               double* weight, hipStream_t stream);
hipError_t launch_blend_init(const float* content, const float* noise, const double* weight, size_t n, float* out,
                             hipStream_t stream);
hipError_t launch_scale(const float* src, float alpha, size_t n, float* dst, hipStream_t stream);
// colour preservation (nst_job_set_color): fp64 statistics of an HWC RGB image - per-block partial sums, reduced in a
// fixed order; mean3 / cov9 are DEVICE doubles (population covariance, row-major); scratch: COLOR_BLOCKS * 9 doubles
constexpr int COLOR_BLOCKS = 256;
hipError_t launch_color_stats(const float* hwc, size_t pixels, double* scratch, double* mean3, double* cov9, hipStream_t stream);
struct ColorAffine { double m[3][3]; double b[3]; };
// out_c = (float)(sum_d m[c][d] p_d + b[c]) per pixel, fp64 arithmetic (HWC -> HWC, in place allowed)
hipError_t launch_color_affine(const float* src, size_t pixels, const ColorAffine& a, float* dst, hipStream_t stream);
// out (1,h,w) = (float)(255 (alpha Y(p) + beta)), Y = 0.299 R + 0.587 G + 0.114 B
hipError_t launch_luminance(const float* hwc, size_t pixels, double alpha, double beta, float* out, hipStream_t stream);
// out HWC = YIQ^-1 (u / 255, I(content), Q(content)); yiq_inv: the fp64 inverse of the YIQ matrix
hipError_t launch_luminance_recombine(const float* u, const float* content_hwc, size_t pixels, const ColorAffine& yiq_inv,
                                      float* out, hipStream_t stream);

// vector_ops.hip: optimiser arithmetic over the n pixel floats ---------------------------------------
constexpr int RED_BLOCKS = 256;
// out[0] = sum(a*b) as float (double accumulation inside), deterministic two-stage
hipError_t launch_dot(const float* a, const float* b, size_t n, double* scratch, float* out, hipStream_t stream);
// out[0] = max|a|, out[1] = sum|a|
hipError_t launch_absmax_abssum(const float* a, size_t n, double* scratch, float* out, hipStream_t stream);
// out[0] (32-bit word, read back as an unsigned) = how many of the n elements of a and b differ in their bit patterns.
// scratch: RED_BLOCKS doubles (stream order lets it share the scratch of launch_absmax_abssum in one launch sequence)
hipError_t launch_count_diff(const float* a, const float* b, size_t n, double* scratch, float* out, hipStream_t stream);
// y = alpha * x + beta * y'  variants
hipError_t launch_dot_partial(const float* a, const float* b, size_t n, double* scratch, hipStream_t stream);   // RED_BLOCKS partials
// one history pair of the L-BFGS two-loop recursion on the device (see vector_ops.hip)
hipError_t launch_lbfgs_pair(const double* sin, float ro, float* al, int second, const float* x, float* y, const float* nxt,
                             size_t n, double* sout, hipStream_t stream);
// L-BFGS direction from inner products (vector_ops.hip): out[j*3 + {0,1,2}] = vecs[j] . {a, b, c};  d = h q0 + sum coef[j] vecs[j]
int multi_dot_blocks(size_t n);                                       // scratch: multi_dot_blocks(n) * nvec * 3 doubles
hipError_t launch_multi_dot(const float* const* vecs_dev, int nvec, const float* a, const float* b, const float* c, size_t n,
                            double* scratch, float* out, hipStream_t stream);
hipError_t launch_multi_axpy(const float* const* vecs_dev, const float* coef_dev, int nvec, const float* q0, float h, float* d,
                             size_t n, hipStream_t stream);
hipError_t launch_axpy(float alpha, const float* x, float* y, size_t n, hipStream_t stream);               // y += alpha*x
hipError_t launch_axpy_dev(const float* alpha_dev, float sign, const float* x, float* y, size_t n, hipStream_t stream);
hipError_t launch_scale_copy(float alpha, const float* x, float* y, size_t n, hipStream_t stream);         // y = alpha*x
hipError_t launch_add_scaled(const float* a, float alpha, const float* b, float* out, size_t n, hipStream_t stream);  // out = a + alpha*b
struct ZeroBatch { void* out[8]; size_t n_words[8]; int n; };
hipError_t launch_zero_batch(const ZeroBatch& b, hipStream_t stream);                                       // launch_zero of each buffer, one launch
hipError_t launch_zero(void* out, size_t n_words, hipStream_t stream);                                      // out[0..n) = 0 (32-bit words, 16-byte aligned)
hipError_t launch_copy(const float* a, float* out, size_t n, hipStream_t stream);                          // out = a (16-byte aligned)
hipError_t launch_sub(const float* a, const float* b, float* out, size_t n, hipStream_t stream);           // out = a-b
hipError_t launch_adam(float* x, const float* g, float* m, float* v, size_t n, float beta2, float one_m_b1, float one_m_b2,
                       float eps, float step_size, float bc2_sqrt, hipStream_t stream);

}  // namespace nst
