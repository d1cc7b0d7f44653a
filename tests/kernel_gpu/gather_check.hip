// TEST-ONLY: the product's table-driven movers on their own -- gather_kernel<SCATTER> (the mover of
// ftar_allreduce_multi), gather_cvt_kernel<T, SCATTER> (the converting mover of
// ftar_allreduce_multi_acc32) and gather_mix_kernel<SCATTER> (the mover of
// ftar_allreduce_multi_mixed) -- launched through ftar::launch_gather / launch_gather_cvt /
// launch_gather_mix with a table built here and a grid chosen here, so that the capped grid's stride loop, every alignment
// of the user buffers against the packed vector, the kWavePiece threshold with its deal of small
// pieces over the four waves, the exact ends of the unrolled loops and the tile-edge exits all
// run on the GPU.  Whole Allreduce jobs reach none of these.
//
//   gather_check        the plain mover: the tables of gen_movers.h's plain_tables() -- element sizes
//       1, 2, 4, 8, 16; user buffers at every multiple of the type's alignment past a 16-byte boundary,
//       congruent to their packed address or not; 2-byte elements against an odd packed address
//       (units of one byte); entries of one element, around one vector, around 1024 bytes, around
//       4 * 64 and 4 * 256 vectors, one tile -1 / 0 / +1 element, an entry ending on a tile edge with
//       another behind it, one entry over five tiles, 320 one-element entries in one tile, 1024
//       entries; user buffers in device memory or in pinned host memory -- each gathered and
//       scattered at grids of ntiles, min(7, ntiles) and 1.  Expectation: concatenation, byte for
//       byte; every other byte of the arena (guards, gaps, the packed bytes past the total, the
//       whole source side) keeps what it held.
//   gather_check cvt    the converting mover on cvt_tables(): user buffers of 2-byte floats at every
//       even offset, packed starts that give classes 8, 4, 2, 1 with heads and tails; float16 and
//       bfloat16.  Gather: every 16-bit pattern, expected (float)decode16, bit for bit.  Scatter at
//       scales 1, 0.5, 1/3, -1, 2^-12, 0, 3.0000002: expected
//       encode16((double)(float)((double)scale * (double)a)) -- one float32 multiplication, one
//       conversion -- on every widened pattern, every tie of two neighbours -1 / 0 / +1 ulp of
//       float32, ties in the subnormal range, the overflow edge, -0 and products underflowing to
//       -0, float32-subnormal products, infinities and NaNs whose upper half reads as an infinity.
//       Bit for bit; a NaN of any payload where the expectation is a NaN.
//   gather_check mix    the mixed mover on mix_tables(): every entry float16, bfloat16 or float32 by
//       the type words behind the table (ftar::mix_types, uploaded as the product lays them out) --
//       the same sizes with the types cycling from each of the three, user offsets of every class and
//       congruence, packed starts 0, 4, 8, 12, 20 (float32 heads of 0, 3, 2, 1 words), whole float32
//       tiles of 1024 and 1023 vectors, 320 one-element entries with type periods of 3 and 4, tables
//       of 1024, 1023 and 7 entries, a tile edge exactly between and 3 elements in front of every
//       ordered pair of types, pieces of 1020 / 1024 / 1028 packed bytes of every type, pinned tables,
//       and the converting tables' value blocks with float32 entries between them.  A 2-byte entry
//       is expected as in `cvt`.  A float32 entry: gathered, the same bits (arbitrary words,
//       signalling NaNs among them; the launch's scale is 0.5 and must not be applied); scattered at
//       the seven scales, (float)((double)scale * (double)a) -- ONE float32 multiplication -- bit
//       for bit on +-0, subnormal products, products underflowing to -0, the overflow at 3.0000002,
//       infinities, NaNs and the largest value; any NaN where a NaN is expected.
// One line per failing case, then "gather_check: N cases, F failed" / "gather_check cvt: ..." /
// "gather_check mix: ...".  A
// case is one launch.  Any HIP error ends the program with status 2 before anything else is launched.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ftar_kernels.h"
#include "gen_movers.h"

#define CHK(x)                                                                                              \
    do {                                                                                                    \
        hipError_t e_ = (x);                                                                                \
        if (e_ != hipSuccess) {                                                                             \
            fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_));               \
            exit(2);                                                                                        \
        }                                                                                                   \
    } while (0)

static_assert(kmov::kTile == ftar::kTileBytes && kref::kFloat16 == ftar::kFloat16 && kref::kBFloat16 == ftar::kBFloat16,
              "gen_movers.h's numbers are the product's");
static_assert(kref::kFloat32 == ftar::kFloat32, "a mixed table's type words are the product's");

namespace {
using namespace kmov;

// the table, in front of the arena's image; in mode `mix` with its type words behind it
size_t kTabBytes = (size_t)ftar::kMaxGather * sizeof(ftar::GEntry);
constexpr int kMix = -1; // Run::launch's `dt` for a mixed table: every entry by its own type

struct Arena {
    unsigned char *dev = nullptr, *host = nullptr, *host_dev = nullptr; // host_dev: the pinned arena as the GPU addresses it
    size_t dev_bytes = 0, host_bytes = 0;
};

// both memories of a table as one image: [0, dev_bytes) the device arena, then the pinned one
struct Image {
    Bytes b;
    size_t dev_bytes = 0;
    unsigned char *packed(const Layout &L) { return &b[L.packed_at]; }
    unsigned char *user(const Table &T, const Layout &L, size_t e) { return &b[(T.pinned ? dev_bytes : 0) + L.user_at[e]]; }
};

bool inside(const Table &T, const Layout &L, const Arena &A)
{
    if (L.dev_bytes > A.dev_bytes || L.host_bytes > A.host_bytes || T.cnt.size() > (size_t)ftar::kMaxGather) return false;
    if (L.packed_at + L.total + kPackedGuard > L.dev_bytes) return false;
    const size_t lim = T.pinned ? L.host_bytes : L.dev_bytes, floor = T.pinned ? 0 : L.packed_at + L.total + kPackedGuard;
    size_t prev = floor;
    for (size_t e = 0; e < T.cnt.size(); e++) {
        const size_t bytes = T.cnt[e] * T.ues(e);
        if (T.cnt[e] == 0 || L.user_at[e] < prev + kGuard || L.user_at[e] + bytes + kGuard > lim) return false;
        prev = L.user_at[e] + bytes;
    }
    return true;
}

struct Run {
    const Arena &A;
    int cases = 0, failed = 0;
    Bytes back;
    explicit Run(const Arena &a) : A(a), back(a.dev_bytes + a.host_bytes) {}

    // uploads `img`, launches, downloads; `dt` 0: the plain mover, kMix: the mixed one.  want: the
    // expected image; its destination elements that hold a NaN (converting runs, and the scatter
    // of a mixed table's float32 entry: a gathered float32 is a copy and compared by its bits) are
    // met by any NaN.
    void launch(const Table &T, const Layout &L, Image &img, const Image &want, int dt, float scale, int scatter, unsigned grid)
    {
        cases++;
        ftar::GatherArgs G;
        memset(&G, 0, sizeof(G));
        G.packed = (char *)A.dev + kTabBytes + L.packed_at;
        G.tab = (const ftar::GEntry *)A.dev;
        G.n = (int)T.cnt.size();
        G.es = T.es;
        G.total = L.total;
        G.ntiles = (unsigned)((L.total + kTile - 1) / kTile);
        CHK(hipMemcpy(A.dev + kTabBytes, img.b.data(), L.dev_bytes, hipMemcpyHostToDevice));
        if (L.host_bytes) memcpy(A.host, &img.b[img.dev_bytes], L.host_bytes);
        CHK(dt == kMix ? ftar::launch_gather_mix(G, ftar::mix_types(G.tab, G.n), scale, scatter, grid, 0)
            : dt       ? ftar::launch_gather_cvt(G, dt, scale, scatter, grid, 0)
                       : ftar::launch_gather(G, scatter, grid, 0));
        CHK(hipDeviceSynchronize());
        CHK(hipMemcpy(back.data(), A.dev + kTabBytes, L.dev_bytes, hipMemcpyDeviceToHost));
        if (L.host_bytes) memcpy(&back[img.dev_bytes], A.host, L.host_bytes);
        const size_t nb = img.dev_bytes + L.host_bytes;
        if (!memcmp(back.data(), want.b.data(), L.dev_bytes) && !memcmp(&back[img.dev_bytes], &want.b[img.dev_bytes], L.host_bytes)) return;
        Bytes tol(want.b.begin(), want.b.begin() + nb);
        if (dt) { // a NaN expectation accepts any NaN
            for (size_t e = 0; e < T.cnt.size(); e++)
                for (size_t i = 0; i < T.cnt[e]; i++) {
                    const int edt = dt == kMix ? T.ty[e] : dt;
                    if (edt == kFloat32) {
                        if (!scatter) continue;
                        const size_t at = (T.pinned ? img.dev_bytes : 0) + L.user_at[e] + 4 * i;
                        float w, g;
                        memcpy(&w, &tol[at], 4);
                        memcpy(&g, &back[at], 4);
                        if (w != w && g != g) memcpy(&tol[at], &g, 4);
                    } else if (scatter) {
                        const size_t at = (T.pinned ? img.dev_bytes : 0) + L.user_at[e] + 2 * i;
                        uint16_t w, g;
                        memcpy(&w, &tol[at], 2);
                        memcpy(&g, &back[at], 2);
                        if (is_nan16(w, edt) && is_nan16(g, edt)) memcpy(&tol[at], &g, 2);
                    } else {
                        const size_t at = L.packed_at + L.off[e] + 4 * i;
                        float w, g;
                        memcpy(&w, &tol[at], 4);
                        memcpy(&g, &back[at], 4);
                        if (w != w && g != g) memcpy(&tol[at], &g, 4);
                    }
                }
        }
        size_t at = 0;
        while (at < nb && (at >= L.dev_bytes && at < img.dev_bytes ? true : back[at] == tol[at])) at++;
        if (at == nb) return;
        failed++;
        // where: inside the packed vector, inside an entry's user buffer, or outside every destination
        char where[160];
        snprintf(where, sizeof(where), "byte %zu of the %s arena", at < img.dev_bytes ? at : at - img.dev_bytes,
                 at < img.dev_bytes ? "device" : "pinned");
        if (at >= L.packed_at && at < L.packed_at + L.total) {
            size_t e = 0;
            while (e + 1 < T.cnt.size() && L.off[e + 1] <= at - L.packed_at) e++;
            snprintf(where, sizeof(where), "packed byte %zu (entry %zu%s%s, its byte %zu)", at - L.packed_at, e, T.mixed() ? ", " : "",
                     T.mixed() ? type_name(T.ty[e]) : "", at - L.packed_at - L.off[e]);
        } else {
            const size_t u = at < img.dev_bytes ? at : at - img.dev_bytes;
            if ((at >= img.dev_bytes) == T.pinned)
                for (size_t e = 0; e < T.cnt.size(); e++)
                    if (u >= L.user_at[e] - kGuard && u < L.user_at[e] + T.cnt[e] * T.ues(e) + kGuard)
                        snprintf(where, sizeof(where), "entry %zu (%zu %selements, user offset %d, packed offset %zu): user byte %td", e,
                                 T.cnt[e], T.mixed() ? (std::string(type_name(T.ty[e])) + " ").c_str() : "", T.uoff[e], L.off[e],
                                 (ptrdiff_t)u - (ptrdiff_t)L.user_at[e]);
        }
        printf("FAIL %s, %s%s, grid %u of %u tiles", T.name.c_str(), scatter ? "scatter" : "gather",
               dt == kFloat16 ? " float16" : dt == kBFloat16 ? " bfloat16" : "", grid, G.ntiles);
        if (dt && (scatter || dt == kMix)) printf(", scale %.9g", scale);
        printf(": %s holds 0x%02x, expected 0x%02x\n", where, back[at], tol[at]);
    }
};

void upload_table(const Arena &A, const Table &T, const Layout &L)
{
    std::vector<ftar::GEntry> tab(T.cnt.size());
    for (size_t e = 0; e < tab.size(); e++) {
        tab[e].ptr = (T.pinned ? A.host_dev : A.dev + kTabBytes) + L.user_at[e];
        tab[e].off = L.off[e];
        tab[e].bytes = T.cnt[e] * T.es;
    }
    CHK(hipMemcpy(A.dev, tab.data(), tab.size() * sizeof(ftar::GEntry), hipMemcpyHostToDevice));
    if (!T.mixed()) return;
    // the type words, where the product puts them: behind the n entries, in the same allocation
    std::vector<unsigned> ty(T.ty.begin(), T.ty.end());
    const ftar::GEntry *dev_tab = (const ftar::GEntry *)A.dev;
    CHK(hipMemcpy((void *)ftar::mix_types(dev_tab, (int)tab.size()), ty.data(), ty.size() * sizeof(unsigned), hipMemcpyHostToDevice));
}

Image blank(const Arena &A)
{
    Image I;
    I.b.assign(A.dev_bytes - kTabBytes + A.host_bytes, kSentinel);
    I.dev_bytes = A.dev_bytes - kTabBytes;
    return I;
}

void plain_table(Run &R, const Table &T)
{
    const Layout L = layout(T);
    if (!inside(T, L, Arena{nullptr, nullptr, nullptr, R.A.dev_bytes - kTabBytes, R.A.host_bytes})) {
        printf("FAIL %s: the table does not fit its arena\n", T.name.c_str());
        R.cases++;
        R.failed++;
        return;
    }
    upload_table(R.A, T, L);
    const unsigned ntiles = (unsigned)((L.total + kTile - 1) / kTile);
    for (int scatter = 0; scatter < 2; scatter++) {
        Image img = blank(R.A);
        if (scatter) {
            for (size_t b = 0; b < L.total; b++) img.packed(L)[b] = plain_byte(T.seed, ~(uint64_t)0, b);
        } else {
            for (size_t e = 0; e < T.cnt.size(); e++)
                for (size_t b = 0; b < T.cnt[e] * T.es; b++) img.user(T, L, e)[b] = plain_byte(T.seed, e, b);
        }
        Image want = img;
        for (size_t e = 0; e < T.cnt.size(); e++) {
            if (scatter) memcpy(want.user(T, L, e), img.packed(L) + L.off[e], T.cnt[e] * T.es);
            else memcpy(want.packed(L) + L.off[e], img.user(T, L, e), T.cnt[e] * T.es);
        }
        for (unsigned grid : grids(ntiles)) R.launch(T, L, img, want, 0, 1.0f, scatter, grid);
    }
}

void cvt_table(Run &R, const Table &T)
{
    const Layout L = layout(T);
    if (!inside(T, L, Arena{nullptr, nullptr, nullptr, R.A.dev_bytes - kTabBytes, R.A.host_bytes})) {
        printf("FAIL %s: the table does not fit its arena\n", T.name.c_str());
        R.cases++;
        R.failed++;
        return;
    }
    upload_table(R.A, T, L);
    const unsigned ntiles = (unsigned)((L.total + kTile - 1) / kTile);
    for (int dt : {(int)kFloat16, (int)kBFloat16}) {
        { // gather: widen
            Image img = blank(R.A);
            Image want = img;
            for (size_t e = 0; e < T.cnt.size(); e++)
                for (size_t i = 0; i < T.cnt[e]; i++) {
                    const uint16_t u = cvt_user(T, L.first[e] + i);
                    const float f = (float)decode16(u, dt);
                    memcpy(img.user(T, L, e) + 2 * i, &u, 2);
                    memcpy(want.user(T, L, e) + 2 * i, &u, 2);
                    memcpy(want.packed(L) + L.off[e] + 4 * i, &f, 4);
                }
            for (unsigned grid : grids(ntiles)) R.launch(T, L, img, want, dt, 1.0f, 0, grid);
        }
        for (float scale : kScales) { // scatter: scale and narrow
            Image img = blank(R.A);
            Image want = img;
            for (size_t e = 0; e < T.cnt.size(); e++)
                for (size_t i = 0; i < T.cnt[e]; i++) {
                    const float a = cvt_packed(T, dt, scale, L.first[e] + i);
                    const uint16_t u = narrow_ref(a, scale, dt);
                    memcpy(img.packed(L) + L.off[e] + 4 * i, &a, 4);
                    memcpy(want.packed(L) + L.off[e] + 4 * i, &a, 4);
                    memcpy(want.user(T, L, e) + 2 * i, &u, 2);
                }
            for (unsigned grid : grids(ntiles)) R.launch(T, L, img, want, dt, scale, 1, grid);
        }
    }
}

// every entry by its own type, from the generators of gen_movers.h alone
void mix_table(Run &R, const Table &T)
{
    const Layout L = layout(T);
    if (!inside(T, L, Arena{nullptr, nullptr, nullptr, R.A.dev_bytes - kTabBytes, R.A.host_bytes}) || T.ty.size() != T.cnt.size() ||
        T.cnt.size() * ftar::kMixEntryBytes > kTabBytes) {
        printf("FAIL %s: the table does not fit its arena\n", T.name.c_str());
        R.cases++;
        R.failed++;
        return;
    }
    upload_table(R.A, T, L);
    const unsigned ntiles = (unsigned)((L.total + kTile - 1) / kTile);
    { // gather: widen a 2-byte entry, copy a float32 one
        Image img = blank(R.A);
        Image want = img;
        for (size_t e = 0; e < T.cnt.size(); e++)
            for (size_t i = 0; i < T.cnt[e]; i++) {
                if (T.ty[e] == kFloat32) {
                    const uint32_t w = f32_user(T, e, i);
                    memcpy(img.user(T, L, e) + 4 * i, &w, 4);
                    memcpy(want.user(T, L, e) + 4 * i, &w, 4);
                    memcpy(want.packed(L) + L.off[e] + 4 * i, &w, 4);
                } else {
                    const uint16_t u = cvt_user(T, L.sub[e] + i);
                    const float f = (float)decode16(u, T.ty[e]);
                    memcpy(img.user(T, L, e) + 2 * i, &u, 2);
                    memcpy(want.user(T, L, e) + 2 * i, &u, 2);
                    memcpy(want.packed(L) + L.off[e] + 4 * i, &f, 4);
                }
            }
        for (unsigned grid : grids(ntiles)) R.launch(T, L, img, want, kMix, 0.5f, 0, grid); // (the scale is the scatter's alone)
    }
    for (float scale : kScales) { // scatter: scale, and narrow into a 2-byte entry
        Image img = blank(R.A);
        Image want = img;
        for (size_t e = 0; e < T.cnt.size(); e++)
            for (size_t i = 0; i < T.cnt[e]; i++) {
                const bool f32 = T.ty[e] == kFloat32;
                const float a = f32 ? f32_packed(T, scale, L.sub[e] + i) : cvt_packed(T, T.ty[e], scale, L.sub[e] + i);
                memcpy(img.packed(L) + L.off[e] + 4 * i, &a, 4);
                memcpy(want.packed(L) + L.off[e] + 4 * i, &a, 4);
                if (f32) {
                    const uint32_t w = scale_ref(a, scale);
                    memcpy(want.user(T, L, e) + 4 * i, &w, 4);
                } else {
                    const uint16_t u = narrow_ref(a, scale, T.ty[e]);
                    memcpy(want.user(T, L, e) + 2 * i, &u, 2);
                }
            }
        for (unsigned grid : grids(ntiles)) R.launch(T, L, img, want, kMix, scale, 1, grid);
    }
}

} // namespace

int main(int argc, char **argv)
{
    const bool cvt = argc > 1 && !strcmp(argv[1], "cvt"), mixed = argc > 1 && !strcmp(argv[1], "mix");
    if (argc > 1 && !cvt && !mixed) {
        fprintf(stderr, "usage: gather_check [cvt | mix]\n");
        return 2;
    }
    if (mixed) kTabBytes = round256((size_t)ftar::kMaxGather * ftar::kMixEntryBytes);
    const std::vector<Table> tables = cvt ? cvt_tables() : mixed ? mix_tables() : plain_tables();
    Arena A;
    for (const Table &T : tables) {
        const Layout L = layout(T);
        A.dev_bytes = std::max(A.dev_bytes, L.dev_bytes);
        A.host_bytes = std::max(A.host_bytes, L.host_bytes);
    }
    A.dev_bytes += kTabBytes;
    // mix: room behind both arenas (not part of the compared image) for a kernel that takes an entry
    // for one of another type and moves twice its user bytes: a failing case, not a fault
    size_t slack = 0;
    if (mixed)
        for (const Table &T : tables)
            for (size_t c : T.cnt) slack = std::max(slack, round256(4 * c));
    CHK(hipMalloc((void **)&A.dev, A.dev_bytes + slack));
    CHK(hipHostMalloc((void **)&A.host, A.host_bytes + slack, hipHostMallocMapped));
    CHK(hipHostGetDevicePointer((void **)&A.host_dev, A.host, 0));
    if (((uintptr_t)A.dev | (uintptr_t)A.host_dev) & 255) {
        fprintf(stderr, "gather_check: an arena is not 256-byte aligned\n");
        return 2;
    }
    Run R(A);
    R.back.resize(A.dev_bytes - kTabBytes + A.host_bytes);
    for (const Table &T : tables) {
        if (cvt) cvt_table(R, T);
        else if (mixed) mix_table(R, T);
        else plain_table(R, T);
    }
    CHK(hipFree(A.dev));
    CHK(hipHostFree(A.host));
    printf("gather_check%s: %d cases, %d failed\n", cvt ? " cvt" : mixed ? " mix" : "", R.cases, R.failed);
    return R.failed ? 1 : 0;
}
