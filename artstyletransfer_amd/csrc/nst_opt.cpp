// nst_opt.cpp - the two optimisers the reference constructs (neural_style_transfer.py:134-136)
// driving nst_closure on the device-resident pixel buffer:
//   Adam   torch:optim/adam.py:457-546  (single tensor, betas (0.9, 0.999), eps 1e-8)
//   L-BFGS torch:optim/lbfgs.py:332-537 (max_iter 1, strong_wolfe, history 100, tolerance_grad 1e-7,
//          tolerance_change 1e-9; max_eval is a parameter, see include/nst_hip.h)
// including the closure's own `lr *= 0.999` (neural_style_transfer.py:155-158).
// Vector arithmetic runs in vector_ops.hip; only scalars (loss, dots) come back to the host,
// because L-BFGS' control flow is host-side scalar logic in the reference too (those scalars: nst_lbfgs_host.h).
//
// Shares nst_ctx.h with the other host sources: the context is read directly, errors go through fail / HIPCHK / NSTCHK.
// An optimiser's memory is NOT the context's (nst_ctx_bytes does not count it, include/nst_hip.h): every device and
// pinned-host allocation of an nst_opt belongs to its OptMem below - the one hipMalloc / hipFree outside nst_ctx.cpp's
// dev_alloc / dev_release; the temporaries of the standalone nst_lbfgs_direction are a Scratch scope's, like any standalone call's.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "nst_ctx.h"
#include "nst_lbfgs_host.h"

using namespace nst;

namespace {
// Owner of one optimiser's allocations: take() / take_pinned() allocate (device memory poisoned under NST_POISON_ALLOC) and
// record, release() frees everything in allocation order.
struct OptMem {
    struct Rec { void* p; bool pinned; };
    std::vector<Rec> recs;
    template <typename T>
    int take(T** p, size_t count) {
        void* v = nullptr;
        if (hipMalloc(&v, count * sizeof(T)) != hipSuccess) return NST_E_NOMEM;
        poison_if_asked(v, count * sizeof(T));
        recs.push_back(Rec{v, false});
        *p = static_cast<T*>(v);
        return NST_OK;
    }
    template <typename T>
    int take_pinned(T** p, size_t count) {
        void* v = nullptr;
        if (hipHostMalloc(&v, count * sizeof(T), hipHostMallocDefault) != hipSuccess) return NST_E_NOMEM;
        recs.push_back(Rec{v, true});
        *p = static_cast<T*>(v);
        return NST_OK;
    }
    void release() {
        for (const Rec& r : recs) (void)(r.pinned ? hipHostFree(r.p) : hipFree(r.p));
        recs.clear();
    }
};
}  // namespace

// What L-BFGS knows about the point P its last step left in x (and, bitwise, in xinit).  The closure is bitwise
// reproducible, so while x still equals P and nothing the closure depends on has changed, the next step's first
// closure is the one already made at P: it is served from here instead of evaluated.
struct ClosureMemo {
    bool valid = false;
    bool have_abs = false;       // gmax, gsum known (else taken from g in the compare's launch sequence)
    bool have_dir = false;       // d, gtd, d_norm, d_sum were formed from g(P) under the current history; g(P) is then in
                                 // prev_g (the trial's gradient is in g), else in g
    float gmax = 0.f, gsum = 0.f;
    float gtd = 0.f, d_norm = 0.f, d_sum = 0.f;
    float w[3] = {0.f, 0.f, 0.f};          // cw, sw, tvw (compared bitwise)
    unsigned long long epoch = 0;          // nst_ctx::closure_epoch when P was evaluated
    std::vector<float> row;                // P's loss row
};

struct nst_opt {
    nst_ctx* ctx = nullptr;
    OptMem mem;                  // owns every device / pinned pointer below
    int kind = 0;
    size_t n = 0;                // channels * pixels of level 0
    int channels = 3;            // the context's channel count when the optimiser was created
    int levels = 0;
    double lr = 10.0;            // python float in the reference
    int total_closures = 0;
    // device
    float* g = nullptr;          // gradient of the latest closure
    float* losses = nullptr;     // 4*levels+1
    double* scratch = nullptr;   // 2*RED_BLOCKS
    float* scal = nullptr;       // 4 floats
    float* al_dev = nullptr;     // L-BFGS: the al_i of the two-loop recursion, one per history pair
    // direction from inner products (default; NST_LBFGS_GRAM=0 selects the sequential recursion): SY[i][j] = s_i . y_j and
    // YY[i][j] = y_i . y_j kept on the host, one multi-dot pass and one multi-axpy pass over the history per step
    // instead of 2 launches per pair (update at 100 pairs, L=2: 3.5 -> 1.5 ms per step)
    bool gram_mode = false;
    const float** vec_dev = nullptr;   // 2*history device pointers: y_0..y_{m-1}, s_0..s_{m-1}
    float* coef_dev = nullptr;         // 2*history coefficients of the direction
    double* md_scratch = nullptr;      // multi_dot_blocks(n) * 2*history * 3
    float* md_out = nullptr;           // 2*history * 3
    unsigned char* pin2 = nullptr;     // page-locked staging: pointers | coefficients | results
    PairTables tab;                    // SY, YY: history x history
    float* pinned = nullptr;     // page-locked host staging for the scalar read-backs (pageable targets make
                                 // hipMemcpyAsync stage through an internal buffer: ~50 us per read-back)
    // adam
    float* m = nullptr; float* v = nullptr; int k = 0;
    // lbfgs
    int max_eval = 1;
    int history = 100;
    int n_iter = 0;
    float* d = nullptr; float* prev_g = nullptr; float* xinit = nullptr; float* q = nullptr;
    std::vector<float*> old_dirs, old_stps;
    std::vector<float> ro;
    std::vector<float*> spare;   // free history vectors: slices of `pool`
    float* pool = nullptr;       // ONE allocation made by nst_opt_create holding every history vector (2*history + 2
                                 // of them): no hipMalloc - an implicit device synchronisation - inside a step
    hipEvent_t tail = nullptr;   // recorded after the last launch of every step: what nst_opt_destroy waits for
    hipStream_t tail_stream = nullptr;
    bool tail_set = false;
    bool want_rows = false;      // this step keeps the loss rows of its closures for the caller
    bool H_is_one = true; float H_diag = 1.f;
    bool t_is_float = true;      // t held as fp32 tensor value vs python double
    double t = 0.0;
    bool have_prev = false;
    // level sharding (BASELINE config 4)
    unsigned level_mask = 0xFFFFFFFFu;
    nst_reduce_hook hook = nullptr;
    void* hook_user = nullptr;
    float* own_g = nullptr; float* own_losses = nullptr;   // buffers this object allocated
    nst_comm* comm = nullptr;    // RCCL communicator (nst_opt_shard_levels_comm): all-reduce of `pack` per closure
    float* pack = nullptr;       // gradient (n floats, padded to 64) followed by the loss row: ONE collective buffer
    size_t pack_floats = 0;
    // per-step outputs
    std::vector<float> loss_rows;   // host copy of every closure's loss rows in this step
    // L-BFGS closure reuse (env NST_CLOSURE_REUSE, default on; nst_opt_set_closure_reuse)
    bool reuse = true;
    ClosureMemo memo;
    long served = 0;             // closures served from the memo (counted in total_closures like evaluated ones)
    // L-BFGS lazy backward (env NST_LAZY_BACKWARD, default on; nst_opt_set_lazy_backward)
    bool lazy = true;
    bool fwd_pending = false;    // the last closure ran as a forward half whose backward half can still be run
    bool no_halves = false;      // nst_closure_forward reported NST_E_UNAVAILABLE under closure epoch no_halves_epoch:
    unsigned long long no_halves_epoch = 0;   // not asked again until the job changes
    long forward_only = 0;       // evaluated closures that ran as a forward half
    long skipped = 0;            // ... whose backward half never ran
};

namespace {

// Scalars the host needs about the new gradient ride on the closure's own synchronisation (every separate read-back
// is a stream sync that leaves the GPU idle until the host has enqueued the next launches).
struct GradStats {
    bool want_abs = false;            // max|g| and sum|g|  (lbfgs.py: opt_cond / first-step t)
    const float* dot_with = nullptr;  // g . dot_with       (lbfgs.py: gtd_new of the line search)
    float gmax = 0.f, gsum = 0.f, gdot = 0.f;
};

// One closure evaluation at x, the part that enqueues: decays lr, fills o->g and o->losses (all-reduced under sharding),
// counts the closure.  Adam without loss rows stops here and stays asynchronous.
// `forward_only` (lazy_applies): the loss row alone by nst_closure_forward - o->g keeps what it held, and o->fwd_pending
// says that nst_closure_backward can still fill it; where the context has no forward half, the whole closure
int enqueue_closure(nst_opt* o, const float* x, float cw, float sw, float tvw, hipStream_t s, bool forward_only = false) {
    o->lr *= 0.999;                                                          // neural_style_transfer.py:155-158
    o->fwd_pending = false;
    if (forward_only && !(o->no_halves && o->no_halves_epoch == o->ctx->closure_epoch)) {
        const int rc = nst_closure_forward(o->ctx, x, cw, sw, tvw, o->level_mask, o->losses, s);
        if (rc == NST_OK) { o->fwd_pending = true; o->forward_only += 1; }
        else if (rc != NST_E_UNAVAILABLE) return rc;
        o->no_halves = rc == NST_E_UNAVAILABLE;
        o->no_halves_epoch = o->ctx->closure_epoch;
    }
    if (!o->fwd_pending) NSTCHK(nst_closure_levels(o->ctx, x, cw, sw, tvw, o->level_mask, o->g, o->losses, s));
    if (o->comm) NSTCHK(nst_comm_allreduce_sum(o->comm, o->pack, o->pack_floats, s));   // gradient + loss row, one call
    else if (o->hook) o->hook(o->hook_user);                                 // all-reduce(sum) over the ranks
    o->total_closures += 1;                                                  // :198
    return NST_OK;
}

// ... and the part that reads back: the loss row (appended to o->loss_rows) and the GradStats asked for (none after a
// forward half), one synchronisation; returns the total loss
int read_closure(nst_opt* o, hipStream_t s, float* loss_out, GradStats* gs = nullptr) {
    const size_t row = (size_t)NST_LOSS_ROW * o->levels + 1;
    const size_t off = o->loss_rows.size();
    o->loss_rows.resize(off + row);
    float* hrow = o->pinned + 8;                                             // [0..8): scalars, [8..): the loss row
    HIPCHK(o->ctx, hipMemcpyAsync(hrow, o->losses, row * sizeof(float), hipMemcpyDeviceToHost, s));
    float* r = o->pinned;
    if (gs && gs->want_abs) HIPCHK(o->ctx, launch_absmax_abssum(o->g, o->n, o->scratch, o->scal, s));
    if (gs && gs->dot_with) HIPCHK(o->ctx, launch_dot(o->g, gs->dot_with, o->n, o->scratch, o->scal + 2, s));
    if (gs) HIPCHK(o->ctx, hipMemcpyAsync(r, o->scal, 3 * sizeof(float), hipMemcpyDeviceToHost, s));
    HIPCHK(o->ctx, hipStreamSynchronize(s));
    if (o->comm) {
        // every level row has exactly one non-zero contributor, so the rows are exact; the grand total is re-formed from
        // them in level order - the association of the unsharded closure (neural_style_transfer.py:179-185) - so that
        // L-BFGS' `f_new < f` takes the same branch as the unsharded run
        float total = hrow[0];
        for (int l = 1; l < o->levels; ++l) total = total + hrow[(size_t)NST_LOSS_ROW * l];
        hrow[row - 1] = total;
    }
    std::memcpy(o->loss_rows.data() + off, hrow, row * sizeof(float));
    if (gs) { gs->gmax = r[0]; gs->gsum = r[1]; gs->gdot = r[2]; }
    *loss_out = o->loss_rows[off + row - 1];
    return NST_OK;
}

int eval_closure(nst_opt* o, const float* x, float cw, float sw, float tvw, hipStream_t s, float* loss_out,
                 GradStats* gs = nullptr, bool forward_only = false) {
    NSTCHK(enqueue_closure(o, x, cw, sw, tvw, s, forward_only));
    return read_closure(o, s, loss_out, gs);
}

// the first k scalars of `scal`, in `pinned` when this returns: one synchronisation for whatever the caller's launches
// before it left there
int read_scal(nst_opt* o, int k, hipStream_t s) {
    HIPCHK(o->ctx, hipMemcpyAsync(o->pinned, o->scal, (size_t)k * sizeof(float), hipMemcpyDeviceToHost, s));
    HIPCHK(o->ctx, hipStreamSynchronize(s));
    return NST_OK;
}

struct LsResult { double t; float f; int evals; double last_t; };   // last_t: the step length evaluated last

bool lazy_applies(const nst_opt* o);

// torch:optim/lbfgs.py:40-209.  Gradients of bracket points are never needed by the caller with
// max_iter == 1 (only f, g.d and t are consumed), so no gradient clones are kept.
int strong_wolfe(nst_opt* o, float* x, double t, float f, float gtd, float d_norm, int max_ls, float cw, float sw,
                 float tvw, hipStream_t s, LsResult* res) {
    const double c1 = 1e-4, c2 = 0.9, tol_change = 1e-9;
    double last_t = t;
    const bool lazy = lazy_applies(o);
    // `ls_after`: ls_iter once this evaluation is counted.  At ls_after == max_ls neither loop below runs again, so of this
    // evaluation only f_new can reach the result: gtd_new goes into br_gtd (read by cubic_interpolate alone, which is not
    // reached), into `done` (which only ends a loop that has ended) and into br[high] (not returned), and the gradient is
    // read by the caller only if this point is the one taken.  Such an evaluation runs as a forward half, without g.d
    // (gtd_new = 0); the caller runs the backward half if it takes the point.
    auto eval_at = [&](double tt, int ls_after, float* f_new, float* gtd_new) -> int {
        // x = x_init + t*d ; closure ; (x restored by the caller at the end)
        last_t = tt;
        HIPCHK(o->ctx, launch_add_scaled(o->xinit, (float)tt, o->d, x, o->n, s));
        if (lazy && ls_after == max_ls) {
            *gtd_new = 0.f;
            return eval_closure(o, x, cw, sw, tvw, s, f_new, nullptr, true);
        }
        GradStats gs;
        gs.dot_with = o->d;
        NSTCHK(eval_closure(o, x, cw, sw, tvw, s, f_new, &gs));
        *gtd_new = gs.gdot;
        return NST_OK;
    };
    float f_new, gtd_new;
    NSTCHK(eval_at(t, 0, &f_new, &gtd_new));
    int evals = 1;
    double t_prev = 0; float f_prev = f; float gtd_prev = gtd;
    bool done = false;
    int ls_iter = 0;
    double br[2] = {0, 0}; float br_f[2] = {0, 0}; float br_gtd[2] = {0, 0};
    int nbr = 0;
    while (ls_iter < max_ls) {
        if (f_new > (float)(f + (float)(c1 * t) * gtd) || (ls_iter > 1 && f_new >= f_prev)) {
            br[0] = t_prev; br[1] = t; br_f[0] = f_prev; br_f[1] = f_new; br_gtd[0] = gtd_prev; br_gtd[1] = gtd_new; nbr = 2;
            break;
        }
        if (std::fabs(gtd_new) <= -(float)c2 * gtd) {
            br[0] = t; br_f[0] = f_new; br_gtd[0] = gtd_new; nbr = 1; done = true;
            break;
        }
        if (gtd_new >= 0) {
            br[0] = t_prev; br[1] = t; br_f[0] = f_prev; br_f[1] = f_new; br_gtd[0] = gtd_prev; br_gtd[1] = gtd_new; nbr = 2;
            break;
        }
        const double min_step = t + 0.01 * (t - t_prev);
        const double max_step = t * 10;
        const double tmp = t;
        t = cubic_interpolate(t_prev, f_prev, gtd_prev, t, f_new, gtd_new, true, min_step, max_step);
        t_prev = tmp; f_prev = f_new; gtd_prev = gtd_new;
        NSTCHK(eval_at(t, ls_iter + 1, &f_new, &gtd_new));
        evals += 1;
        ls_iter += 1;
    }
    if (ls_iter == max_ls && nbr == 0) {
        br[0] = 0; br[1] = t; br_f[0] = f; br_f[1] = f_new; br_gtd[0] = gtd; br_gtd[1] = gtd_new; nbr = 2;
    }
    bool insuf = false;
    int low = (br_f[0] <= br_f[nbr - 1]) ? 0 : 1, high = 1 - low;
    if (nbr == 1) { low = 0; high = 0; }
    while (!done && ls_iter < max_ls) {
        if (std::fabs(br[1] - br[0]) * d_norm < tol_change) break;
        t = cubic_interpolate(br[0], br_f[0], br_gtd[0], br[1], br_f[1], br_gtd[1], false, 0, 0);
        const double bmax = std::max(br[0], br[1]), bmin = std::min(br[0], br[1]);
        const double eps = 0.1 * (bmax - bmin);
        if (std::min(bmax - t, t - bmin) < eps) {
            if (insuf || t >= bmax || t <= bmin) {
                t = (std::fabs(t - bmax) < std::fabs(t - bmin)) ? bmax - eps : bmin + eps;
                insuf = false;
            } else {
                insuf = true;
            }
        } else {
            insuf = false;
        }
        NSTCHK(eval_at(t, ls_iter + 1, &f_new, &gtd_new));
        evals += 1;
        ls_iter += 1;
        if (f_new > (float)(f + (float)(c1 * t) * gtd) || f_new >= br_f[low]) {
            br[high] = t; br_f[high] = f_new; br_gtd[high] = gtd_new;
            low = (br_f[0] <= br_f[1]) ? 0 : 1; high = 1 - low;
        } else {
            if (std::fabs(gtd_new) <= -(float)c2 * gtd) {
                done = true;
            } else if (gtd_new * (br[high] - br[low]) >= 0) {
                br[high] = br[low]; br_f[high] = br_f[low]; br_gtd[high] = br_gtd[low];
            }
            br[low] = t; br_f[low] = f_new; br_gtd[low] = gtd_new;
        }
    }
    res->t = br[low]; res->f = br_f[low]; res->evals = evals; res->last_t = last_t;
    return NST_OK;
}

// The two-loop recursion (lbfgs.py:444-460) in torch's arithmetic order, without a host round trip per pair: q = -g, then
// every launch finishes the previous launch's dot product, applies its pair's update and leaves the partials of the next
// pair's dot product (vector_ops.hip::lbfgs_pair_kernel).  The two halves of `scratch` (2 * RED_BLOCKS doubles) alternate as
// the partials buffer; al_dev: m floats; q: n floats of workspace; d: the direction.
int sequential_direction(nst_ctx* ctx, const float* g, const float* const* y, const float* const* sv, const float* ro, int m,
                         float Hd, float* al_dev, double* scratch, float* q, float* d, size_t n, hipStream_t s) {
    double* pp[2] = {scratch, scratch + RED_BLOCKS};
    int cur = 0;
    HIPCHK(ctx, launch_scale_copy(-1.f, g, q, n, s));            // q = -g
    if (m > 0) HIPCHK(ctx, launch_dot_partial(sv[m - 1], q, n, pp[cur], s));
    for (int i = m - 1; i >= 0; --i) {
        // al_i = (s_i . q) ro_i ;  q -= al_i y_i ;  partials of s_{i-1} . q
        HIPCHK(ctx, launch_lbfgs_pair(pp[cur], ro[i], al_dev + i, 0, y[i], q, i > 0 ? sv[i - 1] : nullptr, n, pp[cur ^ 1], s));
        cur ^= 1;
    }
    HIPCHK(ctx, launch_scale_copy(Hd, q, d, n, s));              // d = r = q * H_diag
    if (m > 0) HIPCHK(ctx, launch_dot_partial(y[0], d, n, pp[cur], s));
    for (int i = 0; i < m; ++i) {
        // be_i = (y_i . r) ro_i ;  r += (al_i - be_i) s_i ;  partials of y_{i+1} . r
        HIPCHK(ctx, launch_lbfgs_pair(pp[cur], ro[i], al_dev + i, 1, sv[i], d, i + 1 < m ? y[i + 1] : nullptr, n, pp[cur ^ 1], s));
        cur ^= 1;
    }
    return NST_OK;
}

// The device side of the inner-product form (nst_lbfgs_host.h has the arithmetic) over m >= 1 pairs: the table of the 2m
// vector pointers y_0..y_{m-1}, s_0..s_{m-1}, multi-dot passes over it, and the direction as one multi-axpy pass.  The host
// blocks are staging that outlives the copies enqueued from them: hp 2m pointers, hcoef 2m floats, hres 6m floats.
struct InnerProducts {
    nst_ctx* ctx; int m; size_t n; hipStream_t s;
    const float** vec_dev; double* md_scratch; float* md_out; float* coef_dev;
    const float** hp; float* hcoef; float* hres;
    int upload(const float* const* y, const float* const* sv) {
        for (int j = 0; j < m; ++j) { hp[j] = y[j]; hp[m + j] = sv[j]; }
        HIPCHK(ctx, hipMemcpyAsync(vec_dev, hp, 2 * (size_t)m * sizeof(float*), hipMemcpyHostToDevice, s));
        return NST_OK;
    }
    // hres = (a . v, b . v, q . v) of every vector v of the table, on the host when this returns
    int pass(const float* a, const float* b, const float* q) {
        HIPCHK(ctx, launch_multi_dot(vec_dev, 2 * m, a, b, q, n, md_scratch, md_out, s));
        HIPCHK(ctx, hipMemcpyAsync(hres, md_out, 2 * (size_t)m * 3 * sizeof(float), hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipStreamSynchronize(s));
        return NST_OK;
    }
    // d = Hd q + sum_j coef_j v_j with the coefficients of the tables and the q column of the last pass
    int direction(const PairTables& tab, const float* ro, float Hd, const float* q, float* d) {
        tab.coefficients(m, hres, ro, Hd, hcoef);
        HIPCHK(ctx, hipMemcpyAsync(coef_dev, hcoef, 2 * (size_t)m * sizeof(float), hipMemcpyHostToDevice, s));
        HIPCHK(ctx, launch_multi_axpy(vec_dev, coef_dev, 2 * m, q, Hd, d, n, s));
        return NST_OK;
    }
};

// The driver's direction in the inner-product form: ONE multi-dot pass gives s_i.q0, y_i.q0 and, for a new pair k, the new
// row / column of SY and YY.
int gram_direction(nst_opt* o, bool new_pair, hipStream_t s) {
    const int m = (int)o->old_dirs.size();
    const size_t H2 = 2 * (size_t)o->history;
    const float Hd = o->H_is_one ? 1.f : o->H_diag;
    HIPCHK(o->ctx, launch_scale_copy(-1.f, o->g, o->q, o->n, s));       // q0 = -g
    if (m == 0) {
        HIPCHK(o->ctx, launch_scale_copy(Hd, o->q, o->d, o->n, s));
        return NST_OK;
    }
    float* hcoef = reinterpret_cast<float*>(o->pin2 + H2 * sizeof(float*));
    InnerProducts ip{o->ctx, m, o->n, s, o->vec_dev, o->md_scratch, o->md_out, o->coef_dev,
                     reinterpret_cast<const float**>(o->pin2), hcoef, hcoef + H2};
    NSTCHK(ip.upload(o->old_dirs.data(), o->old_stps.data()));
    NSTCHK(ip.pass(new_pair ? o->old_stps[m - 1] : o->q, new_pair ? o->old_dirs[m - 1] : o->q, o->q));
    if (new_pair) o->tab.put_pair(m - 1, m, ip.hres);
    return ip.direction(o->tab, o->ro.data(), Hd, o->q, o->d);
}

// this optimiser evaluates whole closures on its own: no level sharding, no collective, no reduce hook (a rank-local
// decision to skip a closure or a backward pass would leave the other ranks in a collective alone)
bool evaluates_alone(const nst_opt* o) {
    const unsigned all = o->levels >= 32 ? 0xFFFFFFFFu : (1u << o->levels) - 1u;
    return !o->comm && !o->hook && (o->level_mask & all) == all;
}
// the closure memo applies: its switch, and whole closures of its own
bool memo_applies(const nst_opt* o) { return o->reuse && evaluates_alone(o); }
// a forward half in place of a whole closure: its switch, L-BFGS only, and whole closures of its own
bool lazy_applies(const nst_opt* o) { return o->lazy && o->kind == NST_OPT_LBFGS && evaluates_alone(o); }

// The first closure of an L-BFGS step, served from a valid memo if x is bitwise its P under the same weights and context
// epoch: one compare of x with xinit (plus max|g|, sum|g| when the memo lacks them) and one synchronisation.  A served
// closure decays lr, counts and appends its row exactly as eval_closure would.
int serve_closure(nst_opt* o, const float* x, float cw, float sw, float tvw, unsigned long long epoch, hipStream_t s,
                  bool* served) {
    *served = false;
    ClosureMemo& M = o->memo;
    const float w[3] = {cw, sw, tvw};
    if (std::memcmp(M.w, w, sizeof(w)) != 0 || M.epoch != epoch) return NST_OK;
    float* r = o->pinned;
    HIPCHK(o->ctx, launch_count_diff(x, o->xinit, o->n, o->scratch, o->scal + 3, s));
    if (!M.have_abs) HIPCHK(o->ctx, launch_absmax_abssum(o->g, o->n, o->scratch, o->scal, s));     // g(P) is in g
    NSTCHK(read_scal(o, 4, s));
    unsigned diff;
    std::memcpy(&diff, r + 3, sizeof(diff));
    if (diff != 0) return NST_OK;
    if (!M.have_abs) { M.gmax = r[0]; M.gsum = r[1]; M.have_abs = true; }
    o->lr *= 0.999;                                                          // neural_style_transfer.py:155-158
    o->loss_rows.insert(o->loss_rows.end(), M.row.begin(), M.row.end());
    o->total_closures += 1;                                                  // :198
    o->served += 1;
    *served = true;
    return NST_OK;
}

// the start of an L-BFGS step after its first closure (g in o->g, lbfgs.py:396-488): the curvature pair, the direction d,
// prev_g = g, the first step length t, and g.d, max|d|, sum|d|
int form_direction(nst_opt* o, double lr, float gsum, hipStream_t s, double* t, float* gtd, float* d_norm, float* d_sum) {
    if (o->n_iter == 1) {
        HIPCHK(o->ctx, launch_scale_copy(-1.f, o->g, o->d, o->n, s));   // d = -g
        for (float* p : o->old_dirs) o->spare.push_back(p);
        for (float* p : o->old_stps) o->spare.push_back(p);
        o->old_dirs.clear(); o->old_stps.clear(); o->ro.clear();
        o->H_is_one = true; o->H_diag = 1.f;
        if (o->gram_mode) o->tab.reset(o->history);
    } else {
        // y = g - prev_g ; s = d * t
        float* y; float* st;
        auto take = [&](float** p) -> int {
            if (o->spare.empty()) return fail(o->ctx, NST_E_STATE, "L-BFGS history pool exhausted");
            *p = o->spare.back(); o->spare.pop_back();
            return NST_OK;
        };
        NSTCHK(take(&y)); NSTCHK(take(&st));
        HIPCHK(o->ctx, launch_sub(o->g, o->prev_g, y, o->n, s));
        HIPCHK(o->ctx, launch_scale_copy((float)o->t, o->d, st, o->n, s));
        HIPCHK(o->ctx, launch_dot(y, st, o->n, o->scratch, o->scal, s));
        HIPCHK(o->ctx, launch_dot(y, y, o->n, o->scratch, o->scal + 1, s));
        NSTCHK(read_scal(o, 2, s));                              // two dot products, one synchronisation
        const float ys = o->pinned[0], yy = o->pinned[1];
        bool new_pair = false;
        if (ys > 1e-10f) {
            if ((int)o->old_dirs.size() == o->history) {
                o->spare.push_back(o->old_dirs.front()); o->spare.push_back(o->old_stps.front());
                o->old_dirs.erase(o->old_dirs.begin()); o->old_stps.erase(o->old_stps.begin()); o->ro.erase(o->ro.begin());
                if (o->gram_mode) o->tab.evict_oldest();
            }
            o->old_dirs.push_back(y); o->old_stps.push_back(st); o->ro.push_back(1.0f / ys);
            o->H_diag = ys / yy; o->H_is_one = false;
            new_pair = true;
        } else {
            o->spare.push_back(y); o->spare.push_back(st);
        }
        if (o->gram_mode) {
            NSTCHK(gram_direction(o, new_pair, s));
        } else {
            NSTCHK(sequential_direction(o->ctx, o->g, o->old_dirs.data(), o->old_stps.data(), o->ro.data(), (int)o->old_dirs.size(),
                                        o->H_is_one ? 1.f : o->H_diag, o->al_dev, o->scratch, o->q, o->d, o->n, s));
        }
    }
    HIPCHK(o->ctx, launch_copy(o->g, o->prev_g, o->n, s));
    o->have_prev = true;
    if (o->n_iter == 1) {
        const float inv = 1.0f / gsum;
        *t = (inv < 1.0f) ? (double)(inv * (float)lr) : lr;      // min(1., 1./|g|_1) * lr
    } else {
        *t = lr;
    }
    HIPCHK(o->ctx, launch_absmax_abssum(o->d, o->n, o->scratch, o->scal, s));
    HIPCHK(o->ctx, launch_dot(o->g, o->d, o->n, o->scratch, o->scal + 2, s));
    NSTCHK(read_scal(o, 3, s));                                  // max|d|, sum|d| and g . d, one synchronisation
    *d_norm = o->pinned[0]; *d_sum = o->pinned[1]; *gtd = o->pinned[2];
    return NST_OK;
}

int lbfgs_step(nst_opt* o, float* x, float cw, float sw, float tvw, hipStream_t s, nst_step_info* info) {
    const double lr = o->lr;                                     // read before the closure decays it (lbfgs.py:349)
    const bool memo_on = memo_applies(o);
    const unsigned long long epoch = o->ctx->closure_epoch;
    ClosureMemo& M = o->memo;
    const bool memo_valid = M.valid;
    M.valid = false;                                             // until this step has completed
    bool served = false;
    if (memo_on && memo_valid) NSTCHK(serve_closure(o, x, cw, sw, tvw, epoch, s, &served));
    // a step that left x where it began (no accepted trial) and had formed its direction: then g(P) = prev_g, the pair
    // y = g(P) - prev_g = 0 is dropped, and history, H_diag, d, g.d, max|d|, sum|d| are bitwise that step's
    const bool reuse_dir = served && M.have_dir;
    float loss, gmax, gsum;
    if (served) {
        loss = M.row.back(); gmax = M.gmax; gsum = M.gsum;
    } else {
        GradStats g0;
        g0.want_abs = true;
        NSTCHK(eval_closure(o, x, cw, sw, tvw, s, &loss, &g0));
        gmax = g0.gmax; gsum = g0.gsum;
    }
    info->loss = loss;
    const size_t row = (size_t)NST_LOSS_ROW * o->levels + 1;
    // memo of the point x holds when this step returns; xinit must hold it too (copied unless the compare showed it)
    auto remember = [&](bool have_dir, bool have_abs, const float* prow, bool copy_x) -> int {
        if (copy_x) HIPCHK(o->ctx, launch_copy(x, o->xinit, o->n, s));
        M.have_dir = have_dir; M.have_abs = have_abs;
        M.gmax = gmax; M.gsum = gsum;
        M.w[0] = cw; M.w[1] = sw; M.w[2] = tvw;
        M.epoch = epoch;
        M.row.assign(prow, prow + row);
        M.valid = true;
        return NST_OK;
    };
    if (gmax <= 1e-7f) {
        info->accepted = 0; info->t = 0.f;
        if (memo_on) NSTCHK(remember(false, true, o->loss_rows.data(), !served));      // g(P) is in g
        return NST_OK;
    }
    o->n_iter += 1;
    double t;
    float gtd, d_norm, d_sum;
    if (reuse_dir) {
        gtd = M.gtd; d_norm = M.d_norm; d_sum = M.d_sum;
        t = lr;                                                  // n_iter >= 2
    } else {
        NSTCHK(form_direction(o, lr, gsum, s, &t, &gtd, &d_norm, &d_sum));
    }
    info->accepted = 0; info->t = 0.f;
    const bool ran_ls = !(gtd > -1e-9f);
    bool moved = false, g_at_x = false;
    if (ran_ls) {
        if (!served) HIPCHK(o->ctx, launch_copy(x, o->xinit, o->n, s));     // (served: the compare found x == xinit)
        LsResult r;
        NSTCHK(strong_wolfe(o, x, t, loss, gtd, d_norm, o->max_eval - 1, cw, sw, tvw, s, &r));
        t = r.t;
        if (t != 0.0) HIPCHK(o->ctx, launch_add_scaled(o->xinit, (float)t, o->d, x, o->n, s));
        else HIPCHK(o->ctx, launch_copy(o->xinit, x, o->n, s));
        info->accepted = (t != 0.0) ? 1 : 0;
        info->t = (float)t;
        moved = t != 0.0;
        g_at_x = moved && r.last_t == t;                         // the last closure was at the point taken: its g is in g
        if (o->fwd_pending) {
            // the last closure was a forward half.  Taken: x holds xinit + t d, bitwise the image it evaluated (written again
            // above with the same operands), so its backward half puts g(x) into g now.  Not taken: nothing reads its gradient
            if (g_at_x) NSTCHK(nst_closure_backward(o->ctx, x, cw, sw, tvw, o->level_mask, o->g, s));
            else o->skipped += 1;
            o->fwd_pending = false;
        }
    }
    o->t = t;
    if (memo_on) {
        if (!moved) {
            // x is still P, and the direction formed here stays valid while the next step drops its pair.  A rejected trial
            // restored x from xinit; a step that skipped the line search left xinit as it was
            M.gtd = gtd; M.d_norm = d_norm; M.d_sum = d_sum;
            NSTCHK(remember(true, true, o->loss_rows.data(), !served && !ran_ls));
        } else if (g_at_x) {
            NSTCHK(remember(false, false, o->loss_rows.data() + o->loss_rows.size() - row, true));
        }
    }
    return NST_OK;
}

// everything an optimiser owns besides its tail event, in o->mem: what is taken when this fails goes with nst_opt_destroy
int allocate(nst_opt* o) {
    OptMem& mem = o->mem;
    const size_t row = (size_t)NST_LOSS_ROW * o->levels + 1;
    // gradient and loss row live in ONE allocation (gradient padded to 64 floats): the sharded closure all-reduces both
    // with a single collective (nst_opt_shard_levels_comm)
    const size_t n_pad = (o->n + 63) & ~(size_t)63;
    o->pack_floats = n_pad + row;
    NSTCHK(mem.take(&o->pack, o->pack_floats));
    if (zero_now(o->pack, o->pack_floats * sizeof(float))) return NST_E_HIP;
    o->g = o->own_g = o->pack;
    o->losses = o->own_losses = o->pack + n_pad;
    NSTCHK(mem.take(&o->scal, 4));
    if (o->kind == NST_OPT_LBFGS) NSTCHK(mem.take(&o->al_dev, (size_t)o->history));
    // nst_options.lbfgs_gram (env NST_LBFGS_GRAM as the default): 0 = the sequential recursion, one fused launch per pair and loop
    if (o->kind == NST_OPT_LBFGS && o->ctx->lbfgs_gram) {
        const size_t H2 = 2 * (size_t)o->history;
        o->gram_mode = true;
        o->tab.reset(o->history);
        NSTCHK(mem.take(&o->vec_dev, H2));
        NSTCHK(mem.take(&o->md_scratch, (size_t)multi_dot_blocks(o->n) * H2 * 3));
        NSTCHK(mem.take_pinned(&o->pin2, H2 * (sizeof(float*) + 4 * sizeof(float))));
        NSTCHK(mem.take(&o->coef_dev, H2));
        NSTCHK(mem.take(&o->md_out, H2 * 3));
    }
    NSTCHK(mem.take_pinned(&o->pinned, 8 + (size_t)NST_LOSS_ROW * NST_MAX_LEVELS + 1));
    NSTCHK(mem.take(&o->scratch, 2 * (size_t)RED_BLOCKS));
    if (o->kind == NST_OPT_ADAM) {
        NSTCHK(mem.take(&o->m, o->n));
        NSTCHK(mem.take(&o->v, o->n));
        if (zero_now(o->m, o->n * 4) || zero_now(o->v, o->n * 4)) return NST_E_HIP;
    }
    if (o->kind == NST_OPT_LBFGS) {
        NSTCHK(mem.take(&o->d, o->n));
        NSTCHK(mem.take(&o->prev_g, o->n));
        NSTCHK(mem.take(&o->xinit, o->n));
        NSTCHK(mem.take(&o->q, o->n));
        // the whole curvature history up front: history pairs (y, s) + the pair being formed.  3.8 GB at L=2, 15 GB at
        // L=3 of the 288 GB; a job that cannot have it fails here, not in the middle of its run
        const size_t nvec = 2 * (size_t)o->history + 2;
        NSTCHK(mem.take(&o->pool, nvec * n_pad));
        o->spare.reserve(nvec);
        for (size_t i = nvec; i-- > 0;) o->spare.push_back(o->pool + i * n_pad);
    }
    return NST_OK;
}

}  // namespace

extern "C" {

int nst_opt_create(nst_ctx* ctx, int kind, float lr_start, int lbfgs_max_eval, nst_opt** out) {
    if (!ctx || !out) return fail(ctx, NST_E_ARG, "null argument");
    if (kind != NST_OPT_ADAM && kind != NST_OPT_LBFGS) return fail(ctx, NST_E_ARG, "Unknown optimizer");
    if (ctx->levels < 1) return fail(ctx, NST_E_STATE, "nst_job_configure has not been called");
    if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, NST_E_HIP, "hipSetDevice failed");
    nst_opt* o = new (std::nothrow) nst_opt();
    if (!o) return fail(ctx, NST_E_NOMEM, "out of host memory");
    o->ctx = ctx; o->kind = kind; o->lr = (double)lr_start;
    o->levels = ctx->levels;
    o->channels = ctx->channels;
    o->n = (size_t)o->channels * ctx->lv[0].h * ctx->lv[0].w;
    o->max_eval = lbfgs_max_eval < 1 ? 1 : lbfgs_max_eval;
    const char* reuse_env = std::getenv("NST_CLOSURE_REUSE");
    o->reuse = !(reuse_env && reuse_env[0] && std::atoi(reuse_env) == 0);
    const char* lazy_env = std::getenv("NST_LAZY_BACKWARD");
    o->lazy = !(lazy_env && lazy_env[0] && std::atoi(lazy_env) == 0);
    int r = allocate(o);
    if (r == NST_OK && hipEventCreateWithFlags(&o->tail, hipEventDisableTiming) != hipSuccess) r = NST_E_HIP;
    if (r != NST_OK) { nst_opt_destroy(o); return fail(ctx, r, "optimiser allocation failed"); }
    *out = o;
    return NST_OK;
}

void nst_opt_destroy(nst_opt* o) {
    if (!o) return;
    (void)hipSetDevice(o->ctx->device);
    // wait for THIS optimiser's last launches only (a device-wide synchronisation would stall the other job that
    // shares the GPU in the two-jobs-per-GPU serving mode)
    if (o->tail) { (void)hipEventSynchronize(o->tail); (void)hipEventDestroy(o->tail); }
    o->mem.release();
    delete o;
}

int nst_opt_shard_levels(nst_opt* o, unsigned level_mask, float* grad, float* losses, nst_reduce_hook hook, void* user) {
    if (!o) return fail(nullptr, NST_E_ARG, "null optimiser");
    if ((hook != nullptr) != (grad != nullptr && losses != nullptr))
        return fail(o->ctx, NST_E_ARG, "a reduce hook needs caller-owned grad and losses buffers (and vice versa)");
    o->level_mask = level_mask;
    o->hook = hook; o->hook_user = user;
    o->comm = nullptr;
    o->memo.valid = false;
    o->g = grad ? grad : o->own_g;
    o->losses = losses ? losses : o->own_losses;
    return NST_OK;
}

int nst_opt_shard_levels_comm(nst_opt* o, unsigned level_mask, nst_comm* comm) {
    if (!o) return fail(nullptr, NST_E_ARG, "null optimiser");
    o->level_mask = comm ? level_mask : 0xFFFFFFFFu;
    o->hook = nullptr; o->hook_user = nullptr;
    o->comm = comm;
    o->g = o->own_g; o->losses = o->own_losses;
    o->memo.valid = false;
    return NST_OK;
}

int nst_opt_history(const nst_opt* o, int* pairs, int* n_iter) {
    if (!o) return fail(nullptr, NST_E_ARG, "null optimiser");
    if (pairs) *pairs = (int)o->old_dirs.size();
    if (n_iter) *n_iter = o->kind == NST_OPT_ADAM ? o->k : o->n_iter;
    return NST_OK;
}

int nst_opt_set_closure_reuse(nst_opt* o, int enabled) {
    if (!o) return fail(nullptr, NST_E_ARG, "null optimiser");
    o->reuse = enabled != 0;
    o->memo.valid = false;
    return NST_OK;
}

int nst_opt_closure_stats(const nst_opt* o, long* evaluated, long* served) {
    if (!o) return fail(nullptr, NST_E_ARG, "null optimiser");
    if (evaluated) *evaluated = (long)o->total_closures - o->served;
    if (served) *served = o->served;
    return NST_OK;
}

int nst_opt_set_lazy_backward(nst_opt* o, int enabled) {
    if (!o) return fail(nullptr, NST_E_ARG, "null optimiser");
    o->lazy = enabled != 0;
    return NST_OK;
}

int nst_opt_backward_stats(const nst_opt* o, long* forward_only, long* skipped) {
    if (!o) return fail(nullptr, NST_E_ARG, "null optimiser");
    if (forward_only) *forward_only = o->forward_only;
    if (skipped) *skipped = o->skipped;
    return NST_OK;
}

// torch:optim/adam.py:457-546 for one tensor, step count k (1-based), group lr `lr` (a python double in the reference)
static int adam_update(nst_ctx* ctx, float* x, const float* g, float* m, float* v, size_t n, int k, double lr, hipStream_t s,
                       float* step_size_out) {
    const double bc1 = 1.0 - std::pow(0.9, k);
    const double bc2 = 1.0 - std::pow(0.999, k);
    const double step_size = lr / bc1;
    // 1 - beta as torch forms them: double differences, rounded to fp32 when they meet the fp32 tensors
    const hipError_t e = launch_adam(x, g, m, v, n, 0.999f, (float)(1.0 - 0.9), (float)(1.0 - 0.999), 1e-8f, (float)step_size,
                                     (float)std::sqrt(bc2), s);
    if (e != hipSuccess) return fail(ctx, NST_E_HIP, hipGetErrorString(e));
    if (step_size_out) *step_size_out = (float)step_size;
    return NST_OK;
}

int nst_adam_step(nst_ctx* ctx, float* x, const float* g, float* m, float* v, size_t n, int k, double lr, void* stream) {
    if (!ctx || !x || !g || !m || !v || k < 1) return fail(ctx, NST_E_ARG, "bad argument");
    if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, NST_E_HIP, "hipSetDevice failed");
    return adam_update(ctx, x, g, m, v, n, k, lr, static_cast<hipStream_t>(stream), nullptr);
}

int nst_lbfgs_direction(nst_ctx* ctx, const float* g, const float* const* y, const float* const* sv, const float* ro, int m,
                        float h_diag, size_t n, int form, float* d, void* stream) {
    if (!ctx || !g || !d || m < 0 || (m > 0 && (!y || !sv || !ro)) || (form != 0 && form != 1))
        return fail(ctx, NST_E_ARG, "bad argument");
    if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, NST_E_HIP, "hipSetDevice failed");
    hipStream_t s = static_cast<hipStream_t>(stream);
    // (host staging of the inner-product form: declared before the scratch scope, whose end waits for the copies from it)
    const size_t M2 = 2 * (size_t)m;
    std::vector<const float*> hp;
    std::vector<float> hcoef, hres;
    Scratch sc(ctx, s);
    float* q = nullptr;
    NSTCHK(sc.alloc(&q, n));
    if (form == 1 || m == 0) {
        // sequential form: the arithmetic order of torch's two loops, one fused launch per pair and loop (no pair: H q0 either way)
        float* al_dev = nullptr; double* scratch = nullptr;
        NSTCHK(sc.alloc(&al_dev, (size_t)m));
        NSTCHK(sc.alloc(&scratch, 2 * (size_t)RED_BLOCKS));
        NSTCHK(sequential_direction(ctx, g, y, sv, ro, m, h_diag, al_dev, scratch, q, d, n, s));
        return sc.finish();
    }
    // inner-product form: S^T Y and Y^T Y by m multi-dot passes (the optimiser driver keeps them incrementally, one
    // pass per step), then the same recurrences and the same multi-axpy pass as the driver
    HIPCHK(ctx, launch_scale_copy(-1.f, g, q, n, s));                               // q0 = -g
    hp.resize(M2); hcoef.resize(M2); hres.resize(M2 * 3);
    InnerProducts ip{ctx, m, n, s, nullptr, nullptr, nullptr, nullptr, hp.data(), hcoef.data(), hres.data()};
    NSTCHK(sc.alloc(&ip.vec_dev, M2));
    NSTCHK(sc.alloc(&ip.md_scratch, (size_t)multi_dot_blocks(n) * M2 * 3));
    NSTCHK(sc.alloc(&ip.md_out, M2 * 3));
    NSTCHK(sc.alloc(&ip.coef_dev, M2));
    NSTCHK(ip.upload(y, sv));
    PairTables tab;
    tab.reset(m);
    for (int k = 0; k < m; ++k) {
        NSTCHK(ip.pass(sv[k], y[k], q));
        tab.put_pair(k, m, hres.data());
    }
    NSTCHK(ip.direction(tab, ro, h_diag, q, d));
    return sc.finish();
}

static int opt_step_body(nst_opt* o, float* x, float cw, float sw, float tvw, nst_step_info* info, hipStream_t s) {
    if (o->kind == NST_OPT_ADAM) {
        float loss = NAN;
        NSTCHK(enqueue_closure(o, x, cw, sw, tvw, s));
        if (o->want_rows) NSTCHK(read_closure(o, s, &loss));     // (else the step stays asynchronous)
        o->k += 1;
        float step_size = 0.f;
        NSTCHK(adam_update(o->ctx, x, o->g, o->m, o->v, o->n, o->k, o->lr, s, &step_size));   // lr already decayed by the closure
        info->loss = loss; info->accepted = 1; info->t = step_size;
    } else {
        NSTCHK(lbfgs_step(o, x, cw, sw, tvw, s, info));
    }
    return NST_OK;
}

int nst_opt_step(nst_opt* o, float* x, float cw, float sw, float tvw, float* losses_host, int closures_capacity,
                 nst_step_info* info, void* stream) {
    if (!o || !x || !info) return fail(o ? o->ctx : nullptr, NST_E_ARG, "null argument");
    if (hipSetDevice(o->ctx->device) != hipSuccess) return fail(o->ctx, NST_E_HIP, "hipSetDevice failed");
    if (o->channels != o->ctx->channels)
        return fail(o->ctx, NST_E_STATE, "the optimiser was created under the other colour mode (nst_job_set_color)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    // a step issued on another stream than the previous one is ordered behind it (one tail event then covers the optimiser)
    if (o->tail_set && s != o->tail_stream) HIPCHK(o->ctx, hipStreamWaitEvent(s, o->tail, 0));
    std::memset(info, 0, sizeof(*info));
    o->loss_rows.clear();
    const int before = o->total_closures;
    o->want_rows = losses_host != nullptr;
    const int rc = opt_step_body(o, x, cw, sw, tvw, info, s);
    // recorded on EVERY path out of the step - a step that failed half way has launches in flight too - so that
    // nst_opt_destroy never frees the optimiser's buffers under them
    if (hipEventRecord(o->tail, s) == hipSuccess) { o->tail_stream = s; o->tail_set = true; }
    if (rc != NST_OK) return rc;
    info->closures = o->total_closures - before;
    info->total_closures = o->total_closures;
    info->lr = (float)o->lr;
    info->history = (int)o->old_dirs.size();
    if (losses_host) {
        const size_t row = (size_t)NST_LOSS_ROW * o->levels + 1;
        const size_t have = o->loss_rows.size() / row;
        const size_t cp = std::min(have, (size_t)std::max(closures_capacity, 0));
        std::memcpy(losses_host, o->loss_rows.data(), cp * row * sizeof(float));
    }
    return NST_OK;
}

}  // extern "C"
