// devmem_host.cpp - artstyletransfer_amd/csrc/nst_devmem.h alone, on the host: the owner of device allocations and the
// transactional replace helper over malloc / free, with an allocator that can be told to fail its k-th request.  Built with
// -fsanitize=address,undefined and run by tests/test_devmem_host.py: a leak, a double free or a use after release ends the
// program with a non-zero status, as does a failed CHECK.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "nst_devmem.h"

struct nst_ctx {
    size_t bytes = 0;
    int fail_in = 0;                 // > 0: the fail_in-th allocation from now fails
    int allocs = 0, releases = 0;
};

namespace nst {
int dev_alloc(nst_ctx* ctx, void** p, size_t bytes, size_t* charged) {
    if (ctx->fail_in > 0 && --ctx->fail_in == 0) return -3;
    if (bytes == 0) bytes = 16;
    *p = malloc(bytes);
    ctx->bytes += bytes;
    ctx->allocs += 1;
    if (charged) *charged = bytes;
    return 0;
}
void dev_release(nst_ctx* ctx, void* p, size_t bytes) {
    free(p);
    ctx->bytes -= bytes;
    ctx->releases += 1;
}
}  // namespace nst

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

namespace {

// a term's per-level block: three buffers, the last of size zero
struct Term {
    float* a = nullptr;
    double* b = nullptr;
    char* z = nullptr;
    size_t n = 0;
    nst::DevMem mem;
};
struct Level { Term term; };
constexpr int kLevels = 2, kAllocs = 3 * kLevels;

int fill(nst_ctx* ctx, Term& t, size_t n) {
    t.n = n;
    if (int rc = t.mem.alloc(ctx, &t.a, n)) return rc;
    if (int rc = t.mem.alloc(ctx, &t.b, n + 3)) return rc;
    if (int rc = t.mem.alloc(ctx, &t.z, 0)) return rc;
    return 0;
}
size_t charge(size_t n) { return n * sizeof(float) + (n + 3) * sizeof(double) + 16; }
void write_through(Term& t) {
    memset(t.a, 0x5a, t.n * sizeof(float));
    memset(t.b, 0x5a, (t.n + 3) * sizeof(double));
    memset(t.z, 0x5a, 16);
}

void replace_with_kth_failure(int k) {
    nst_ctx ctx;
    Level lv[kLevels];
    int commits = 0;
    auto commit = [&] { ++commits; };
    const size_t old_n[kLevels] = {5, 9}, new_n[kLevels] = {7, 2};
    CHECK(nst::replace_blocks(lv, kLevels, &Level::term, [&](int i, Term& t) { return fill(&ctx, t, old_n[i]); }, commit) == 0);
    CHECK(commits == 1 && ctx.allocs == kAllocs && ctx.releases == 0);
    const size_t before = ctx.bytes;
    CHECK(before == charge(old_n[0]) + charge(old_n[1]));
    const float* a_before[kLevels] = {lv[0].term.a, lv[1].term.a};
    const double* b_before[kLevels] = {lv[0].term.b, lv[1].term.b};

    ctx.fail_in = k;
    const int rc = nst::replace_blocks(lv, kLevels, &Level::term, [&](int i, Term& t) { return fill(&ctx, t, new_n[i]); }, commit);
    if (k <= kAllocs) {
        // refused: what was taken is back, nothing moved, nothing of the old blocks was released
        CHECK(rc == -3 && commits == 1);
        CHECK(ctx.bytes == before);
        CHECK(ctx.releases == k - 1 && ctx.allocs == kAllocs + k - 1);
        for (int i = 0; i < kLevels; ++i) {
            CHECK(lv[i].term.a == a_before[i] && lv[i].term.b == b_before[i] && lv[i].term.n == old_n[i]);
            write_through(lv[i].term);
        }
    } else {
        CHECK(rc == 0 && commits == 2);
        CHECK(ctx.bytes == charge(new_n[0]) + charge(new_n[1]));
        CHECK(ctx.releases == kAllocs && ctx.allocs == 2 * kAllocs);      // each old buffer once (twice: the sanitizer speaks)
        for (int i = 0; i < kLevels; ++i) {
            CHECK(lv[i].term.n == new_n[i]);
            write_through(lv[i].term);
        }
    }
    for (Level& L : lv) L.term = Term();
    CHECK(ctx.bytes == 0 && ctx.allocs == ctx.releases);
}

void owner_basics() {
    nst_ctx ctx;
    {
        nst::DevMem a;
        char* z = nullptr;
        int* v = nullptr;
        CHECK(a.alloc(&ctx, &z, 0) == 0 && ctx.bytes == 16);       // a zero-size request is charged the floor
        CHECK(a.alloc(&ctx, &v, 10) == 0 && ctx.bytes == 16 + 40);
        nst::DevMem b = std::move(a);
        a.release();                                                // moved from: nothing to give back
        CHECK(ctx.bytes == 56 && ctx.releases == 0);
        v[9] = 1;
        nst::DevMem c;
        c = std::move(b);
        b.release();
        CHECK(ctx.bytes == 56 && ctx.releases == 0);
        // exchange: each buffer changes owner with its charge
        nst::DevMem d;
        long* w = nullptr;
        CHECK(d.alloc(&ctx, &w, 100) == 0 && ctx.bytes == 56 + 800);
        c.exchange(v, d, w);
        d.release();                                                // frees v (40), keeps w
        CHECK(ctx.bytes == 16 + 800 && ctx.releases == 1);
        w[99] = 1;
        ctx.fail_in = 1;
        CHECK(c.alloc(&ctx, &v, 4) == -3 && ctx.bytes == 16 + 800);
    }                                                               // leaving the scope releases the rest
    CHECK(ctx.bytes == 0 && ctx.allocs == 3 && ctx.releases == 3);
}

}  // namespace

int main() {
    owner_basics();
    for (int k = 1; k <= kAllocs + 1; ++k) replace_with_kth_failure(k);
    printf("devmem ok: %d replace runs\n", kAllocs + 1);
    return 0;
}
