// nst_devmem.h - who owns device memory (nothing of HIP is needed here: tests/devmem_host.cpp drives this header alone over
// malloc).  Every allocation of nst_ctx.cpp, nst_closure.cpp and nst_api.cpp, and the scratch of nst_opt.cpp's standalone
// nst_lbfgs_direction, belongs to a DevMem, which remembers per allocation the pointer and the bytes the context was
// charged, and gives back exactly that.  The typed pointers of ActSet, Guidance, LapLevel ... are views into their struct's
// DevMem.  The one other owner is nst_opt.cpp's OptMem: an optimiser's vectors are deliberately NOT charged to the context
// (nst_ctx_bytes, include/nst_hip.h), so they do not go through dev_alloc.
#pragma once
#include <cstddef>
#include <utility>
#include <vector>

struct nst_ctx;

namespace nst {

// nst_ctx.cpp: the only hipMalloc (a zero-size request gets 16 bytes; *charged = what ctx->bytes grew by) and the only
// hipFree (ctx->bytes shrinks by `bytes`) of context-charged memory
int dev_alloc(nst_ctx* ctx, void** p, size_t bytes, size_t* charged = nullptr);
void dev_release(nst_ctx* ctx, void* p, size_t bytes);

class DevMem {
    struct Rec { void* p; size_t bytes; };      // bytes: what the context was charged
    nst_ctx* ctx_ = nullptr;
    std::vector<Rec> recs_;

public:
    DevMem() = default;
    DevMem(DevMem&& o) noexcept : ctx_(o.ctx_), recs_(std::move(o.recs_)) { o.recs_.clear(); }
    DevMem& operator=(DevMem&& o) noexcept {
        if (this != &o) { release(); ctx_ = o.ctx_; recs_ = std::move(o.recs_); o.recs_.clear(); }
        return *this;
    }
    ~DevMem() { release(); }

    int alloc_bytes(nst_ctx* ctx, void** p, size_t bytes) {
        size_t charged = 0;
        const int rc = dev_alloc(ctx, p, bytes, &charged);
        if (rc != 0) return rc;
        ctx_ = ctx;
        recs_.push_back(Rec{*p, charged});
        return 0;
    }
    template <typename T>
    int alloc(nst_ctx* ctx, T** p, size_t count) { return alloc_bytes(ctx, reinterpret_cast<void**>(p), count * sizeof(T)); }

    // frees everything, in allocation order; the views into it dangle (the owning struct is reset or dies with it)
    void release() {
        for (const Rec& b : recs_) dev_release(ctx_, b.p, b.bytes);
        recs_.clear();
    }
    // `mine` becomes `other`'s and `theirs` this one's, each with its charge (both of one context)
    void exchange(void* mine, DevMem& other, void* theirs) {
        for (Rec& a : recs_)
            for (Rec& b : other.recs_)
                if (a.p == mine && b.p == theirs) { std::swap(a, b); return; }
    }
};

// The transactional replace of one per-level member (a struct with its DevMem): fill(i, fresh) builds level i's new block
// beside the old one.  A failure returns fill's code with everything taken so far released and the levels untouched;
// otherwise commit() runs (the caller's quiesce and drop of the closure state: the old blocks may still be in use until
// then), and each level's old block is released as the new one moves in.
template <typename Level, typename Block, typename Fill, typename Commit>
int replace_blocks(Level* lv, int n, Block Level::*member, Fill fill, Commit commit) {
    std::vector<Block> fresh(n > 0 ? n : 0);
    for (int i = 0; i < n; ++i)
        if (const int rc = fill(i, fresh[i])) return rc;
    commit();
    for (int i = 0; i < n; ++i) lv[i].*member = std::move(fresh[i]);
    return 0;
}

}  // namespace nst
