// TEST-ONLY: the product's segment kernel (every pull, copy, relay phase and guard store of
// the schedules) on its own, against the CPU oracle, bit for bit.
//
// Random segment lists as the schedules build them -- up to 16 pieces of copies and
// reduces, ragged lengths, element offsets that are co-aligned or not (vector body with
// scalar head / tail, or the scalar path), a second destination receiving the result again --
// planned by plan_segments at several grid caps (one tile per workgroup, and capped grids
// whose workgroups loop, as the mid-size gated launches run) and launched by
// launch_segments.  Expected values: copies as they are, reduces by the oracle's
// reduce_local (out = x op y, OpenMPI's operand roles), MAX / MIN over NaN, signed zeros and
// infinities.  Every byte around each destination is checked untouched.
//   seg_check [lists [swapped]]   prints one line per failing list, then "seg_check: N lists, F failed";
//   `swapped` expects y op x -- the checker's own test: float MAX / MIN lists must then fail
//
//   seg_check types [swapped]   the same on the element types the oracle does not know (element
//   sizes 2, 8 and 16): 210 lists, float16 / bfloat16 x SUM, PROD, MAX, MIN and the three pair
//   types x MAXLOC, MINLOC in rotation, against the plain reference of ref_types.h on the inputs
//   of gen_types.h; windows at every offset past a 16-byte boundary the type's alignment allows
//   (heads of 7, 5 and 1 two-byte elements; 8-byte pairs at 4 and 12: co-aligned, yet the scalar
//   path), co-aligned or independent; one piece in eight 256 KiB .. 2 MiB, and three lists
//   per combination built to reach the interleaved prefix (counted per element size, each must
//   occur); the four grid caps.  One device
//   arena serves every list.  Destinations bit for bit (NaN-ness where a SUM / PROD expectation
//   is a NaN), every other byte of the arena -- guards and sources -- untouched.  Prints
//   "seg_check types: N lists, F failed"; `swapped` succeeds when exactly the order-sensitive
//   lists with a reduce piece of n >= 257 fail and every SUM / PROD and FTAR_2INT list passes.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "ftar_kernels.h"
#include "gen_types.h"

extern "C" int ftar_oracle_reduce_local(int dtype, int op, const void *in, void *inout, size_t n);

#define CHK(x)                                                                                              \
    do {                                                                                                    \
        hipError_t e_ = (x);                                                                                \
        if (e_ != hipSuccess) {                                                                             \
            fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_));               \
            exit(2);                                                                                        \
        }                                                                                                   \
    } while (0)

static size_t esize(int dt) { return (dt == ftar::kInt64 || dt == ftar::kFloat64) ? 8 : 4; }

static void fill(unsigned char *buf, int dt, int op, size_t n, std::mt19937_64 &g)
{
    const bool sel = op == ftar::kMax || op == ftar::kMin;
    for (size_t i = 0; i < n; i++) {
        const unsigned r = (unsigned)(g() % 16);
        if (dt == ftar::kFloat32 || dt == ftar::kFloat64) {
            double v = std::ldexp((double)(int64_t)(g() % 2000001) - 1000000.0, -(int)(g() % 20));
            if (r == 0) v = 0.0;
            else if (r == 1) v = -0.0;
            else if (sel && r == 2) v = std::nan("");
            else if (sel && r == 3) v = -std::nan("");
            else if (sel && r == 4) v = INFINITY;
            else if (sel && r == 5) v = -INFINITY;
            if (dt == ftar::kFloat32) {
                float f = (float)v;
                memcpy(buf + i * 4, &f, 4);
            } else {
                memcpy(buf + i * 8, &v, 8);
            }
        } else {
            const uint64_t v = r < 3 ? r : g();
            memcpy(buf + i * esize(dt), &v, esize(dt));
        }
    }
}

// one device allocation with a guard band around the operand
struct Buf {
    unsigned char *base = nullptr;
    size_t off = 0, bytes = 0;
    static constexpr size_t kPad = 64;
    void *ptr() const { return base + kPad + off; }
};

static Buf alloc(size_t bytes, size_t off, unsigned char fillbyte)
{
    Buf b;
    b.off = off;
    b.bytes = bytes;
    CHK(hipMalloc((void **)&b.base, bytes + 2 * Buf::kPad + 16));
    CHK(hipMemset(b.base, fillbyte, bytes + 2 * Buf::kPad + 16));
    return b;
}

int types_main(bool swapped);

int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "types")) return types_main(argc > 2 && !strcmp(argv[2], "swapped"));
    const int lists = argc > 1 ? atoi(argv[1]) : 400;
    const bool swapped = argc > 2 && !strcmp(argv[2], "swapped");
    std::mt19937_64 g(4242);
    const int ops[][2] = {{ftar::kFloat32, ftar::kSum}, {ftar::kFloat32, ftar::kMax}, {ftar::kFloat32, ftar::kMin},
                          {ftar::kFloat64, ftar::kSum}, {ftar::kFloat64, ftar::kMin}, {ftar::kInt32, ftar::kSum},
                          {ftar::kInt32, ftar::kBor},   {ftar::kInt64, ftar::kProd}, {ftar::kInt64, ftar::kMax}};
    const unsigned caps[] = {1u << 20, 1024, 128, 7};
    int failed = 0;
    for (int li = 0; li < lists; li++) {
        const int *o = ops[li % (sizeof(ops) / sizeof(ops[0]))];
        const int dt = o[0], op = o[1];
        const size_t es = esize(dt);
        const unsigned cap = caps[(li / 9) % 4];
        const int nseg = 1 + (int)(g() % 16);
        const bool coalign = g() % 4 != 0;
        const size_t common = (size_t)(g() % 4) * es % 16;
        std::vector<ftar::SegIn> in(nseg);
        std::vector<Buf> outs, out2s, xs, ys;
        std::vector<std::vector<unsigned char>> hx(nseg), hy(nseg), want(nseg), want2(nseg);
        for (int s = 0; s < nseg; s++) {
            // mostly short pieces, some long ones (the interleaved prefix deals 128 KiB chunks)
            const size_t n = g() % 8 == 0 ? (size_t)(g() % (1u << 20)) + 1 : (size_t)(g() % 9000) + 1;
            auto off = [&]() { return coalign ? common : (size_t)(g() % 4) * es % 16; };
            const int kind = g() % 3 == 0 ? ftar::kCopy : ftar::kReduce;
            const bool with2 = g() % 3 != 0; // a second destination: the result again
            hx[s].resize(n * es);
            hy[s].resize(n * es);
            fill(hx[s].data(), dt, op, n, g);
            fill(hy[s].data(), dt, op, n, g);
            xs.push_back(alloc(n * es, off(), 0));
            ys.push_back(alloc(n * es, off(), 0));
            outs.push_back(alloc(n * es, off(), 0xA5));
            out2s.push_back(with2 ? alloc(n * es, off(), 0x5A) : Buf{});
            CHK(hipMemcpy(xs.back().ptr(), hx[s].data(), n * es, hipMemcpyHostToDevice));
            CHK(hipMemcpy(ys.back().ptr(), hy[s].data(), n * es, hipMemcpyHostToDevice));
            in[s].kind = kind;
            in[s].out = outs.back().ptr();
            in[s].x = xs.back().ptr();
            in[s].y = kind == ftar::kCopy ? nullptr : ys.back().ptr();
            in[s].n = n;
            in[s].out2 = with2 ? out2s.back().ptr() : nullptr;
            want[s] = swapped && kind == ftar::kReduce ? hy[s] : hx[s];
            if (kind == ftar::kReduce &&
                ftar_oracle_reduce_local(dt, op, (swapped ? hx[s] : hy[s]).data(), want[s].data(), n) != 0) {
                fprintf(stderr, "oracle refused dtype %d op %d\n", dt, op);
                return 2;
            }
            want2[s] = want[s];
        }
        ftar::KSegList L;
        const unsigned grid = ftar::plan_segments(in.data(), nseg, es, cap, &L);
        L.nt_store = (unsigned)(li & 1);
        memset(&L.sig, 0, sizeof(L.sig));
        bool ok = grid != 0;
        if (!ok) printf("FAIL list %d: plan_segments refused (%d pieces, cap %u)\n", li, nseg, cap);
        else CHK(ftar::launch_segments(dt, op, L, grid, 0));
        CHK(hipDeviceSynchronize());
        for (int s = 0; s < nseg && ok; s++) {
            const size_t n = in[s].n, bytes = n * es;
            for (int which = 0; which < 2 && ok; which++) {
                const Buf &b = which ? out2s[s] : outs[s];
                if (!b.base) continue;
                std::vector<unsigned char> whole(b.bytes + 2 * Buf::kPad + 16);
                CHK(hipMemcpy(whole.data(), b.base, whole.size(), hipMemcpyDeviceToHost));
                const std::vector<unsigned char> &w = which ? want2[s] : want[s];
                if (memcmp(whole.data() + Buf::kPad + b.off, w.data(), bytes)) {
                    size_t e = 0;
                    while (e < n && !memcmp(whole.data() + Buf::kPad + b.off + e * es, w.data() + e * es, es)) e++;
                    printf("FAIL list %d piece %d/%d (%s, n %zu, dtype %d op %d, cap %u, %s%s): element %zu\n", li, s,
                           nseg, in[s].kind == ftar::kCopy ? "copy" : "reduce", n, dt, op, cap,
                           which ? "second destination" : "out",
                           coalign ? ", co-aligned" : "", e);
                    ok = false;
                }
                const unsigned char fb = which ? 0x5A : 0xA5;
                for (size_t i = 0; i < whole.size() && ok; i++)
                    if ((i < Buf::kPad + b.off || i >= Buf::kPad + b.off + bytes) && whole[i] != fb) {
                        printf("FAIL list %d piece %d: byte %zu outside the destination written\n", li, s, i);
                        ok = false;
                    }
            }
            // the sources are never written
            std::vector<unsigned char> chk(bytes);
            CHK(hipMemcpy(chk.data(), xs[s].ptr(), bytes, hipMemcpyDeviceToHost));
            if (ok && chk != hx[s]) {
                printf("FAIL list %d piece %d: source x modified\n", li, s);
                ok = false;
            }
        }
        if (!ok) failed++;
        for (auto *v : {&outs, &out2s, &xs, &ys})
            for (auto &b : *v)
                if (b.base) CHK(hipFree(b.base));
    }
    printf("seg_check: %d lists, %d failed\n", lists, failed);
    return failed ? 1 : 0;
}

// ---------------------------------------------------------------------------------
// `types`: float16, bfloat16 and the pair types (gen_types.h's lists, ref_types.h's reference)
// ---------------------------------------------------------------------------------
static_assert(kref::kFloat16 == ftar::kFloat16 && kref::kBFloat16 == ftar::kBFloat16 && kref::kFloatInt == ftar::kFloatInt &&
                  kref::k2Int == ftar::k2Int && kref::kDoubleInt == ftar::kDoubleInt && kref::kSum == ftar::kSum &&
                  kref::kProd == ftar::kProd && kref::kMax == ftar::kMax && kref::kMin == ftar::kMin &&
                  kref::kMaxloc == ftar::kMaxloc && kref::kMinloc == ftar::kMinloc,
              "ref_types.h's numbers are the product's");

namespace {

constexpr size_t kGuard = 64;
inline size_t slot_size(size_t bytes) { return (bytes + 16 + 2 * kGuard + 255) & ~(size_t)255; }

// a piece's four slots in the arena: x, y, out, out2, each 256-byte aligned, the operand kGuard
// bytes and its window offset past the slot's start
struct Placed {
    size_t at[4], bytes;
    size_t pos(int which, int off) const { return at[which] + kGuard + (size_t)off; }
};

size_t place(const kgen::SegList &L, std::vector<Placed> *out)
{
    size_t next = 0;
    for (const kgen::SegPiece &P : L.pc) {
        Placed pl;
        pl.bytes = P.n * kref::esize(L.dt);
        for (int w = 0; w < 4; w++) {
            pl.at[w] = next;
            next += slot_size(pl.bytes);
        }
        if (out) out->push_back(pl);
    }
    return next;
}

} // namespace

int types_main(bool swapped)
{
    size_t arena = 0;
    for (int li = 0; li < kgen::kSegLists; li++) arena = std::max(arena, place(kgen::seg_list(li), nullptr));
    unsigned char *dev;
    CHK(hipMalloc((void **)&dev, arena));
    std::vector<unsigned char> img(arena), back(arena);
    int failed = 0, must = 0, must_failed = 0, free_failed = 0, interleaved[3] = {0, 0, 0}; // by element size 2, 8, 16
    for (int li = 0; li < kgen::kSegLists; li++) {
        const kgen::SegList G = kgen::seg_list(li);
        const kgen::Combo combo{G.dt, G.op};
        const size_t es = kref::esize(G.dt);
        const int nseg = (int)G.pc.size();
        std::vector<Placed> pl;
        const size_t used = place(G, &pl);
        if (used > arena) return 2;
        std::vector<ftar::SegIn> in(nseg);
        std::vector<kgen::Bytes> want(nseg);
        bool judged = false; // a reduce piece long enough for the inputs to show the operand order
        for (int s = 0; s < nseg; s++) {
            const kgen::SegPiece &P = G.pc[s];
            const Placed &p = pl[s];
            const int offs[4] = {P.ox, P.oy, P.oo, P.oo2};
            const unsigned char fillbyte[4] = {0x33, 0x33, 0xA5, 0x5A};
            for (int w = 0; w < 4; w++) memset(&img[p.at[w]], fillbyte[w], slot_size(p.bytes));
            kgen::Bytes x(p.bytes), y(p.bytes);
            kgen::fill(x.data(), G.dt, G.op, P.n, 0, 2, P.seed);
            kgen::fill(y.data(), G.dt, G.op, P.n, 1, 2, P.seed);
            memcpy(&img[p.pos(0, offs[0])], x.data(), p.bytes);
            memcpy(&img[p.pos(1, offs[1])], y.data(), p.bytes);
            in[s].kind = P.kind ? ftar::kReduce : ftar::kCopy;
            in[s].x = dev + p.pos(0, offs[0]);
            in[s].y = P.kind ? dev + p.pos(1, offs[1]) : nullptr;
            in[s].out = dev + p.pos(2, offs[2]);
            in[s].out2 = P.with2 ? dev + p.pos(3, offs[3]) : nullptr;
            in[s].n = P.n;
            if (!P.kind) {
                want[s] = x;
                continue;
            }
            judged |= P.n >= 257;
            want[s] = swapped ? y : x; // out = x op y: the reference's inout is x, its in is y
            if (kref::reduce_local(G.dt, G.op, (swapped ? x : y).data(), want[s].data(), P.n) != 0) {
                fprintf(stderr, "reference refused dtype %d op %d\n", G.dt, G.op);
                return 2;
            }
        }
        ftar::KSegList L;
        const unsigned grid = ftar::plan_segments(in.data(), nseg, es, G.cap, &L);
        L.nt_store = (unsigned)(kgen::mix((uint64_t)li) >> 7) & 1;
        memset(&L.sig, 0, sizeof(L.sig));
        bool ok = grid != 0;
        if (!ok) printf("FAIL list %d: plan_segments refused (%d pieces, cap %u)\n", li, nseg, G.cap);
        if (ok) {
            interleaved[es == 2 ? 0 : es == 8 ? 1 : 2] += L.il_blocks > 0;
            CHK(hipMemcpy(dev, img.data(), used, hipMemcpyHostToDevice));
            CHK(ftar::launch_segments(G.dt, G.op, L, grid, 0));
            CHK(hipDeviceSynchronize());
            CHK(hipMemcpy(back.data(), dev, used, hipMemcpyDeviceToHost));
        }
        for (int s = 0; s < nseg && ok; s++) {
            const kgen::SegPiece &P = G.pc[s];
            const Placed &p = pl[s];
            const int offs[4] = {P.ox, P.oy, P.oo, P.oo2};
            for (int w = 0; w < 4 && ok; w++) {
                const bool dest = w == 2 || (w == 3 && P.with2);
                const size_t a = p.at[w], b = dest ? p.pos(w, offs[w]) : a + slot_size(p.bytes), e = a + slot_size(p.bytes);
                // sources, unused slots and the bytes around a destination: as uploaded
                if (memcmp(&back[a], &img[a], b - a) || (dest && memcmp(&back[b + p.bytes], &img[b + p.bytes], e - b - p.bytes))) {
                    printf("FAIL list %d piece %d/%d: %s written\n", li, s, nseg,
                           dest ? "bytes outside a destination" : "a source or an unused destination");
                    ok = false;
                }
                size_t first = 0;
                if (ok && dest && kgen::count_diff(&back[b], want[s].data(), G.dt, G.op, P.n, &first)) {
                    printf("FAIL list %d piece %d/%d (%s, n %zu, dtype %d op %d, cap %u, offsets %d %d %d %d, %s): element %zu\n", li,
                           s, nseg, P.kind ? "reduce" : "copy", P.n, G.dt, G.op, G.cap, P.ox, P.oy, P.oo, P.oo2,
                           w == 3 ? "second destination" : "out", first);
                    ok = false;
                }
            }
        }
        failed += !ok;
        if (kgen::order_sensitive(combo) && judged) {
            must++;
            must_failed += !ok;
        } else if (!kgen::order_sensitive(combo)) {
            free_failed += !ok;
        }
    }
    CHK(hipFree(dev));
    if (!swapped) {
        printf("seg_check types: lists with an interleaved prefix: %d / %d / %d at element size 2 / 8 / 16\n", interleaved[0],
               interleaved[1], interleaved[2]);
        if (!interleaved[0] || !interleaved[1] || !interleaved[2]) {
            printf("FAIL an element size never reached the interleaved prefix\n");
            failed++;
        }
        printf("seg_check types: %d lists, %d failed\n", kgen::kSegLists, failed);
        return failed ? 1 : 0;
    }
    printf("seg_check types swapped: %d lists, %d failed; order-sensitive with a reduce piece of n >= 257: %d of %d failed; "
           "order-free: %d failed\n", kgen::kSegLists, failed, must_failed, must, free_failed);
    return (must_failed == must && free_failed == 0) ? 0 : 1;
}
