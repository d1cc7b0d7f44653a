// TEST-ONLY: the product's kernels (fault-tolerant_amd/build/ftar_kernels.o, as linked into
// libftar.so) on the 8-, 16-bit and unsigned integer types, each kernel on its own through the
// planners and launchers of ftar_kernels.h, against the plain reference of int_ref.h byte for byte.
//
//   int_check [wide]
//
//   pairs     default: every (type, op) whose kernel is the type's own (ftar::canon_dtype(type, op)
//             == type: the 8 shared ops of uint8 / uint16, MAX / MIN of all six) and, through the
//             dispatch alone, SUM and BXOR of the four types that borrow a sibling's kernel;
//             `wide`: all 6 x 10
//   lengths   5 (scalar only), 31 (head + tail, no body), one full 16 KiB tile + a partial one +
//             a tail of 3 (iref::case_lengths)
//   windows   every byte offset 0..15 the element's alignment allows, at every length, all operands
//             co-aligned; at offset 0 also one operand one element further (not co-aligned: the
//             scalar path)
//   segment   plan_segments + launch_segments: reduce into a second buffer with a second output,
//             reduce in place, copy with two outputs; plain and non-temporal stores in turn, both at
//             offset 0
//   tree      plan_tree + launch_tree at P = 2, 4, 8, 16, U = 1 and at P = 4, 8 also U = 2, 4, with
//             P - 1 further destinations at P <= 8, U = 1
//   batch     plan_tree_batch + launch_tree_batch at P = 2, 4, 8: P trees over consecutive blocks
//             of one vector (blocks begin on odd addresses)
//   lds       launch_reduce_lds: 1 vector, one tile + 17 vectors, grids of 1 and of all tiles
//   mover     launch_gather, both directions, at 1- and 2-byte elements: 7 entries of 1, 3, 16, 17,
//             4099, 33 and 16384 + 5 elements at odd addresses
// Every output buffer is compared whole: the window and the guard bytes around it.  One line per
// failing case, then "int_check: N cases, F failed".  Any HIP error ends the program with status 2
// before anything else is launched.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ftar_kernels.h"
#include "int_ref.h"

#define CHK(x)                                                                                              \
    do {                                                                                                    \
        hipError_t e_ = (x);                                                                                \
        if (e_ != hipSuccess) {                                                                             \
            fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_));               \
            exit(2);                                                                                        \
        }                                                                                                   \
    } while (0)

static_assert(iref::kInt8 == ftar::kInt8 && iref::kUInt8 == ftar::kUInt8 && iref::kInt16 == ftar::kInt16 &&
                  iref::kUInt16 == ftar::kUInt16 && iref::kUInt32 == ftar::kUInt32 && iref::kUInt64 == ftar::kUInt64 &&
                  iref::kSum == ftar::kSum && iref::kBxor == ftar::kBxor,
              "the reference's numbers are the product's");

using iref::Bytes;

constexpr size_t kCap = 24576, kLead = 64; // bytes per device buffer; the window begins at kLead + offset
constexpr unsigned char kSentinel = 0xC3;
constexpr int kMaxSrc = 16, kMaxOut = 8;
constexpr unsigned kMaxBlocks = 262144;

static unsigned char *g_src[kMaxSrc], *g_out[kMaxOut];
static int g_cases = 0, g_failed = 0;

static void failed(const char *kernel, int dt, int op, size_t n, unsigned off, const char *what, const char *why)
{
    g_failed++;
    printf("FAIL %s dtype %d op %d, %zu elements at byte %u, %s: %s\n", kernel, dt, op, n, off, what, why);
}

// device buffer b holds `bytes` of data at kLead + off, sentinels elsewhere
static void put_window(unsigned char *dev, unsigned off, const unsigned char *data, size_t bytes)
{
    CHK(hipMemset(dev, kSentinel, kCap));
    if (bytes) CHK(hipMemcpy(dev + kLead + off, data, bytes, hipMemcpyHostToDevice));
}

// the whole buffer against sentinels around `want` at kLead + off
static const char *check_window(unsigned char *dev, unsigned off, const Bytes &want)
{
    static Bytes back(kCap);
    CHK(hipMemcpy(back.data(), dev, kCap, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < kLead + off; i++)
        if (back[i] != kSentinel) return "bytes in front of the window written";
    for (size_t i = kLead + off + want.size(); i < kCap; i++)
        if (back[i] != kSentinel) return "bytes behind the window written";
    if (want.size() && memcmp(&back[kLead + off], want.data(), want.size())) return "wrong element";
    return nullptr;
}

struct Pair { int dt, op; };
static std::vector<Pair> pairs(bool wide)
{
    std::vector<Pair> v;
    for (int dt : iref::kTypes)
        for (int op = 0; op < iref::kNumOps; op++)
            if (wide || ftar::canon_dtype(dt, op) == dt || op == iref::kSum || op == iref::kBxor) v.push_back({dt, op});
    return v;
}

struct Window { unsigned off; unsigned skew; }; // skew: bytes the last operand sits further (0 = co-aligned)
static std::vector<Window> windows(size_t es)
{
    std::vector<Window> w;
    for (unsigned o = 0; o < 16; o += (unsigned)es) {
        w.push_back({o, 0});
    }
    w.push_back({0, (unsigned)es});
    return w;
}

static void run_segments(const Pair &c, size_t n, const Window &w)
{
    const size_t es = iref::esize(c.dt), bytes = n * es;
    Bytes x(bytes), y(bytes);
    const uint64_t seed = iref::case_seed(c.dt, c.op, n);
    iref::fill(c.dt, c.op, n, 0, seed, x.data());
    iref::fill(c.dt, c.op, n, 1, seed, y.data());
    Bytes want = x;
    iref::reduce_local(c.dt, c.op, y.data(), want.data(), n);
    // form 0: out = x op y, out2 too; 1: x op= y in place; 2: out = out2 = y (copy)
    for (int form = 0; form < 3; form++)
        for (unsigned nts = 0; nts < 2; nts++) {
            if (w.off && nts != ((w.off / es + form) & 1)) continue;
            g_cases++;
            put_window(g_src[0], w.off, x.data(), bytes);
            put_window(g_src[1], w.off + w.skew, y.data(), bytes);
            put_window(g_out[0], w.off, nullptr, 0);
            put_window(g_out[1], w.off, nullptr, 0);
            unsigned char *X = g_src[0] + kLead + w.off, *Y = g_src[1] + kLead + w.off + w.skew;
            unsigned char *O = g_out[0] + kLead + w.off, *O2 = g_out[1] + kLead + w.off;
            ftar::SegIn in;
            if (form == 0) in = ftar::SegIn{ftar::kReduce, O, X, Y, n, O2};
            else if (form == 1) in = ftar::SegIn{ftar::kReduce, X, X, Y, n, nullptr};
            else in = ftar::SegIn{ftar::kCopy, O, Y, nullptr, n, O2};
            ftar::KSegList L;
            const unsigned grid = ftar::plan_segments(&in, 1, es, kMaxBlocks, &L);
            if (grid == 0) {
                failed("segment", c.dt, c.op, n, w.off, "plan", "no grid");
                continue;
            }
            L.nt_store = nts;
            CHK(ftar::launch_segments(c.dt, c.op, L, grid, 0));
            CHK(hipDeviceSynchronize());
            const char *why = nullptr;
            static const char *const names[] = {"reduce, two outputs", "reduce in place", "copy, two outputs"};
            if (form == 1) why = check_window(g_src[0], w.off, want);
            else if (!(why = check_window(g_out[0], w.off, form == 0 ? want : y))) why = check_window(g_out[1], w.off, form == 0 ? want : y);
            if (!why && form != 1) why = check_window(g_src[0], w.off, x) ? "x written" : nullptr;
            if (!why) why = check_window(g_src[1], w.off + w.skew, y) ? "y written" : nullptr;
            if (why) failed("segment", c.dt, c.op, n, w.off, names[form], why);
        }
}

static void run_tree(const Pair &c, size_t n, const Window &w, int p, unsigned unroll, int nmore)
{
    const size_t es = iref::esize(c.dt), bytes = n * es;
    const uint64_t seed = iref::case_seed(c.dt, c.op, n);
    std::vector<Bytes> s(p, Bytes(bytes));
    const unsigned char *sp[kMaxSrc];
    ftar::TreeArgs A{};
    for (int j = 0; j < p; j++) {
        iref::fill(c.dt, c.op, n, j, seed, s[j].data());
        sp[j] = s[j].data();
        const unsigned off = w.off + (j == p - 1 ? w.skew : 0);
        put_window(g_src[j], off, s[j].data(), bytes);
        A.src[j] = g_src[j] + kLead + off;
    }
    Bytes want(bytes);
    iref::tree(c.dt, c.op, p, sp, want.data(), n);
    for (int o = 0; o <= nmore; o++) put_window(g_out[o], w.off, nullptr, 0);
    A.out = g_out[0] + kLead + w.off;
    A.nmore = nmore;
    for (int o = 0; o < nmore; o++) A.more[o] = g_out[o + 1] + kLead + w.off;
    A.n = n;
    A.unroll = unroll;
    A.nt_store = (n + w.off) & 1; // both kinds of store over the cases
    g_cases++;
    char what[64];
    snprintf(what, sizeof(what), "P %d U %u, %d more", p, unroll, nmore);
    const unsigned grid = ftar::plan_tree(&A, p, es, kMaxBlocks);
    if (grid == 0) return failed("tree", c.dt, c.op, n, w.off, what, "no grid");
    CHK(ftar::launch_tree(c.dt, c.op, p, A, grid, 0));
    CHK(hipDeviceSynchronize());
    const char *why = nullptr;
    for (int o = 0; o <= nmore && !why; o++) why = check_window(g_out[o], w.off, want);
    for (int j = 0; j < p && !why; j++)
        if (check_window(g_src[j], w.off + (j == p - 1 ? w.skew : 0), s[j])) why = "a source written";
    if (why) failed("tree", c.dt, c.op, n, w.off, what, why);
}

static void run_batch(const Pair &c, size_t n, const Window &w, int p)
{
    const size_t es = iref::esize(c.dt), bytes = n * es;
    const uint64_t seed = iref::case_seed(c.dt, c.op, n);
    std::vector<Bytes> s(p, Bytes(bytes));
    const unsigned char *sp[kMaxSrc];
    for (int j = 0; j < p; j++) {
        iref::fill(c.dt, c.op, n, j, seed, s[j].data());
        sp[j] = s[j].data();
        put_window(g_src[j], w.off + (j == p - 1 ? w.skew : 0), s[j].data(), bytes);
    }
    Bytes want(bytes);
    iref::tree(c.dt, c.op, p, sp, want.data(), n);
    put_window(g_out[0], w.off, nullptr, 0);
    ftar::TreeBatch B{};
    size_t at = 0;
    for (int k = 0; k < p; k++) { // near-equal blocks; an empty one gets no tree
        const size_t m = n / p + ((size_t)k < n % p);
        if (m == 0) continue;
        ftar::TreeArgs &A = B.t[B.nt++];
        for (int j = 0; j < p; j++) A.src[j] = g_src[j] + kLead + w.off + (j == p - 1 ? w.skew : 0) + at * es;
        A.out = g_out[0] + kLead + w.off + at * es;
        A.n = m;
        A.unroll = 1;
        A.nt_store = k & 1;
        at += m;
    }
    g_cases++;
    char what[32];
    snprintf(what, sizeof(what), "P %d", p);
    const unsigned grid = ftar::plan_tree_batch(&B, p, es, kMaxBlocks);
    if (grid == 0) return failed("batch", c.dt, c.op, n, w.off, what, "no grid");
    CHK(ftar::launch_tree_batch(c.dt, c.op, p, B, grid, 0));
    CHK(hipDeviceSynchronize());
    const char *why = check_window(g_out[0], w.off, want);
    if (why) failed("batch", c.dt, c.op, n, w.off, what, why);
}

static void run_lds(const Pair &c)
{
    const size_t es = iref::esize(c.dt);
    for (size_t nv : {(size_t)1, (size_t)ftar::kTileVecs + 17})
        for (unsigned grid : {1u, (unsigned)((nv + ftar::kTileVecs - 1) / ftar::kTileVecs)})
            for (unsigned nts = 0; nts < 2; nts++) {
                const size_t bytes = nv * 16, n = bytes / es;
                Bytes x(bytes), y(bytes);
                const uint64_t seed = iref::case_seed(c.dt, c.op, n);
                iref::fill(c.dt, c.op, n, 0, seed, x.data());
                iref::fill(c.dt, c.op, n, 1, seed, y.data());
                Bytes want = x;
                iref::reduce_local(c.dt, c.op, y.data(), want.data(), n);
                put_window(g_src[0], 0, x.data(), bytes);
                put_window(g_src[1], 0, y.data(), bytes);
                g_cases++;
                CHK(ftar::launch_reduce_lds(c.dt, c.op, g_src[0] + kLead, g_src[1] + kLead, nv, grid, 0, nts));
                CHK(hipDeviceSynchronize());
                const char *why = check_window(g_src[0], 0, want);
                if (!why && check_window(g_src[1], 0, y)) why = "`in` written";
                if (why) failed("lds", c.dt, c.op, n, 0, nts ? "nt stores" : "plain stores", why);
            }
}

// the gather / scatter mover at element size es: entries at odd addresses inside one user buffer
static void run_mover(size_t es)
{
    const size_t counts[] = {1, 3, 16, 17, 4099, 33, 16384 + 5};
    constexpr int kN = 7;
    size_t total = 0, ubytes = 0, uoff[kN];
    for (int i = 0; i < kN; i++) {
        ubytes += es; // one element of slack in front of every entry: odd addresses at es = 1
        if (i == 2) ubytes += 16 - ubytes % 16; // ... and one entry 16-byte aligned
        uoff[i] = ubytes;
        ubytes += counts[i] * es;
        total += counts[i] * es;
    }
    ubytes += 32;
    unsigned char *user, *packed, *back;
    ftar::GEntry *tab;
    CHK(hipMalloc((void **)&user, ubytes));
    CHK(hipMalloc((void **)&back, ubytes));
    CHK(hipMalloc((void **)&packed, total + 64));
    CHK(hipMalloc((void **)&tab, 2 * kN * sizeof(ftar::GEntry)));
    Bytes hu(ubytes), hp(total), got(ubytes), gp(total + 64);
    for (size_t i = 0; i < ubytes; i++) hu[i] = (unsigned char)(iref::mix(i ^ (es << 20)) | 1);
    ftar::GEntry g[kN], sc[kN];
    size_t at = 0;
    for (int i = 0; i < kN; i++) {
        g[i] = ftar::GEntry{user + uoff[i], at, counts[i] * es};
        sc[i] = ftar::GEntry{back + uoff[i], at, counts[i] * es};
        memcpy(&hp[at], &hu[uoff[i]], counts[i] * es);
        at += counts[i] * es;
    }
    CHK(hipMemcpy(user, hu.data(), ubytes, hipMemcpyHostToDevice));
    CHK(hipMemcpy(tab, g, sizeof(g), hipMemcpyHostToDevice));
    CHK(hipMemcpy(tab + kN, sc, sizeof(sc), hipMemcpyHostToDevice));
    CHK(hipMemset(packed, kSentinel, total + 64));
    CHK(hipMemset(back, 0, ubytes));
    ftar::GatherArgs A{};
    A.packed = (char *)packed;
    A.tab = tab;
    A.n = kN;
    A.es = (unsigned)es;
    A.total = total;
    A.ntiles = (unsigned)((total + ftar::kTileBytes - 1) / ftar::kTileBytes);
    g_cases++;
    CHK(ftar::launch_gather(A, 0, A.ntiles, 0));
    CHK(hipDeviceSynchronize());
    CHK(hipMemcpy(gp.data(), packed, total + 64, hipMemcpyDeviceToHost));
    bool ok = !memcmp(gp.data(), hp.data(), total);
    for (size_t i = total; i < total + 64; i++) ok = ok && gp[i] == kSentinel;
    if (!ok) failed("mover", 0, 0, total / es, (unsigned)es, "gather", "packed vector differs or was overrun");
    g_cases++;
    A.tab = tab + kN;
    CHK(ftar::launch_gather(A, 1, 1, 0)); // one workgroup: the stride loop over the tiles
    CHK(hipDeviceSynchronize());
    CHK(hipMemcpy(got.data(), back, ubytes, hipMemcpyDeviceToHost));
    Bytes wantu(ubytes, 0);
    for (int i = 0; i < kN; i++) memcpy(&wantu[uoff[i]], &hu[uoff[i]], counts[i] * es);
    if (got != wantu) failed("mover", 0, 0, total / es, (unsigned)es, "scatter", "entries differ or bytes between them written");
    CHK(hipFree(user));
    CHK(hipFree(back));
    CHK(hipFree(packed));
    CHK(hipFree(tab));
}

int main(int argc, char **argv)
{
    const bool wide = argc > 1 && !strcmp(argv[1], "wide");
    for (int j = 0; j < kMaxSrc; j++) CHK(hipMalloc((void **)&g_src[j], kCap));
    for (int o = 0; o < kMaxOut; o++) CHK(hipMalloc((void **)&g_out[o], kCap));
    for (const Pair &c : pairs(wide)) {
        const size_t es = iref::esize(c.dt);
        for (size_t n : iref::case_lengths(es)) {
            if (kLead + 16 + es + n * es + 64 > kCap) {
                fprintf(stderr, "case does not fit its buffer\n");
                return 2;
            }
            for (const Window &w : windows(es)) {
                run_segments(c, n, w);
                for (int p : {2, 4, 8, 16})
                    for (unsigned u : {1u, 2u, 4u}) {
                        if (u > 1 && !(p == 4 || p == 8)) continue;
                        run_tree(c, n, w, p, u, (p <= 8 && u == 1) ? p - 1 : 0);
                    }
                for (int p : {2, 4, 8}) run_batch(c, n, w, p);
            }
        }
        run_lds(c);
    }
    run_mover(1);
    run_mover(2);
    for (int j = 0; j < kMaxSrc; j++) CHK(hipFree(g_src[j]));
    for (int o = 0; o < kMaxOut; o++) CHK(hipFree(g_out[o]));
    printf("int_check: %d cases, %d failed\n", g_cases, g_failed);
    return g_failed ? 1 : 0;
}
