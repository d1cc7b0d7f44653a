// TEST-ONLY: the product's LDS-staged local reduce (reduce_lds_kernel, the default variant of the
// local reduce) on its own, through ftar::launch_reduce_lds with a grid chosen here -- so that its
// outer loop takes several full tiles per workgroup and ends in the ragged path on every element
// type and op, which the library's own grid (one tile per workgroup up to thousands of tiles)
// never does.
//
//   lds_check   all nine element types with every op the type has (int32 / int64: ten, the float
//   types: SUM, PROD, MAX, MIN, the pair types: MAXLOC, MINLOC) x both kinds of store x 1, 63, 64,
//   255, 256, 257, 1023, 1024, 1025 and 4 * 1024 + 65 vectors of 16 bytes x grids of ntiles,
//   min(3, ntiles) and 1.  Inputs: gen_movers.h's fill for the oracle's four types, gen_types.h's for
//   the others -- NaNs, +-0, infinities, pair padding.  Expectation: inout = inout op in by the
//   oracle's reduce_local (the four old types) or kref::reduce_local, bit for bit, by NaN-ness where
//   a SUM / PROD expectation is a NaN.  The full-tile path and the ragged path name their operands
//   separately: ref_check's selftest shows that swapped operands would be seen in either.  `in` and
//   the guards around `inout` keep what they held.
// One line per failing case, then "lds_check: N cases, F failed".  Any HIP error ends the program
// with status 2 before anything else is launched.
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

static_assert(kref::kInt32 == ftar::kInt32 && kref::kFloat32 == ftar::kFloat32 && kref::kInt64 == ftar::kInt64 &&
                  kref::kFloat64 == ftar::kFloat64 && kref::kFloat16 == ftar::kFloat16 && kref::kBFloat16 == ftar::kBFloat16 &&
                  kref::kFloatInt == ftar::kFloatInt && kref::k2Int == ftar::k2Int && kref::kDoubleInt == ftar::kDoubleInt &&
                  kref::kSum == ftar::kSum && kref::kProd == ftar::kProd && kref::kMax == ftar::kMax && kref::kMin == ftar::kMin &&
                  kref::kMaxloc == ftar::kMaxloc && kref::kMinloc == ftar::kMinloc && kmov::kLdsTileVecs == ftar::kTileVecs,
              "the references' numbers are the product's");

int main()
{
    using namespace kmov;
    constexpr size_t kPad = 256;
    const size_t maxb = kLdsVecs[9] * 16, arena = 3 * kPad + 2 * maxb;
    unsigned char *dev;
    CHK(hipMalloc((void **)&dev, arena));
    Bytes img(arena), back(arena);
    int cases = 0, failed = 0;
    for (const LdsCombo &c : lds_combos())
        for (size_t nv : kLdsVecs) {
            // [guard][inout][guard][in][guard], both operands 16-byte aligned
            const size_t bytes = nv * 16, n = bytes / esize(c.dt), io = kPad, in = 2 * kPad + bytes, used = 3 * kPad + 2 * bytes;
            const uint64_t seed = lds_seed(c.dt, c.op, nv);
            memset(img.data(), kSentinel, used);
            lds_fill(&img[io], c.dt, c.op, n, 0, seed);
            lds_fill(&img[in], c.dt, c.op, n, 1, seed);
            Bytes want(img.begin() + io, img.begin() + io + bytes);
            if (reduce_local(c.dt, c.op, &img[in], want.data(), n) != 0) {
                fprintf(stderr, "reference refused dtype %d op %d\n", c.dt, c.op);
                return 2;
            }
            for (unsigned nts = 0; nts < 2; nts++)
                for (unsigned grid : lds_grids(nv)) {
                    cases++;
                    CHK(hipMemcpy(dev, img.data(), used, hipMemcpyHostToDevice));
                    CHK(ftar::launch_reduce_lds(c.dt, c.op, dev + io, dev + in, nv, grid, 0, nts));
                    CHK(hipDeviceSynchronize());
                    CHK(hipMemcpy(back.data(), dev, used, hipMemcpyDeviceToHost));
                    size_t first = 0;
                    const char *why = nullptr;
                    if (memcmp(&back[0], &img[0], io) || memcmp(&back[io + bytes], &img[io + bytes], kPad)) why = "a guard of inout written";
                    else if (memcmp(&back[in], &img[in], bytes + kPad)) why = "`in` or the guard behind it written";
                    else if (lds_diff(&back[io], want.data(), c.dt, c.op, n, &first)) why = "wrong element";
                    if (why) {
                        failed++;
                        printf("FAIL dtype %d op %d, %zu vectors, grid %u, nt stores %u: %s (element %zu of %zu)\n", c.dt, c.op, nv, grid,
                               nts, why, first, n);
                    }
                }
        }
    CHK(hipFree(dev));
    printf("lds_check: %d cases, %d failed\n", cases, failed);
    return failed ? 1 : 0;
}
