/*
 * measure.c -- the mover measurement of profiles/acc32/README.md, one rank on one GPU.
 *
 *   ftrun -np 1 --devmap 0 measure <K> <packed MiB> <iterations> [uneven]
 *
 * K entries whose float32 (packed) total is <packed MiB>; with `uneven` the entries alternate
 * between per + 3 and per - 3 elements, so that packed offsets and user addresses lose their
 * common alignment after the first entry (the converting kernel's narrower classes, the copying
 * kernel's element-by-element path).  Two lists of each kind used in turn, so that with the staging
 * vectors more than 1 GiB passes through the 256 MiB Infinity Cache between two uses of a byte.
 * With ftar_set_profiling on, per round the device time of all kernels of
 *   a) one ftar_allreduce_multi_acc32 over K bfloat16 buffers (widening gather + the one-rank
 *      schedule's copy of the packed float32 vector + narrowing scatter),
 *   b) the same over K float16 buffers,
 *   c) one ftar_allreduce_multi over K float32 buffers of the same element counts (the existing
 *      mover: gather + the same copy + scatter),
 *   d) one plain float32 call on the packed total (that copy alone).
 * a - d, b - d and c - d are the movers' two launches.  Prints every round and the summary.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <hip/hip_runtime_api.h>

#include "ftar.h"

#define CHECK_HIP(x)                                                                               \
    do {                                                                                           \
        hipError_t e_ = (x);                                                                       \
        if (e_ != hipSuccess) {                                                                    \
            fprintf(stderr, "measure: %s: %s\n", #x, hipGetErrorString(e_));                       \
            return 1;                                                                              \
        }                                                                                          \
    } while (0)

static int by_val(const void *a, const void *b) { return *(const double *)a < *(const double *)b ? -1 : *(const double *)a > *(const double *)b; }
static double pct(double *v, int n, double q)
{
    qsort(v, (size_t)n, sizeof(double), by_val);
    return v[(int)(q * (n - 1) + 0.5)];
}

int main(int argc, char **argv)
{
    if (argc < 4) return 2;
    const int K = atoi(argv[1]), iters = atoi(argv[3]), uneven = argc > 4 && !strcmp(argv[4], "uneven");
    if (K < 2 || K > FTAR_MULTI_MAX || K % 2 || iters < 5 || iters > 1000) return 2;
    const size_t per = (size_t)atoll(argv[2]) * (1 << 20) / 4 / (size_t)K;
    ftar_comm *comm;
    if (ftar_init(&comm) != FTAR_SUCCESS) return 3;
    int dev;
    ftar_comm_device(comm, &dev);
    CHECK_HIP(hipSetDevice(dev));
    static const void *s16[2][FTAR_MULTI_MAX], *s32[2][FTAR_MULTI_MAX];
    static void *r16[2][FTAR_MULTI_MAX], *r32[2][FTAR_MULTI_MAX];
    static size_t counts[FTAR_MULTI_MAX];
    size_t total = 0;
    for (int k = 0; k < K; k++) {
        counts[k] = uneven ? (k % 2 ? per - 3 : per + 3) : per;
        total += counts[k];
    }
    for (int s = 0; s < 2; s++)
        for (int k = 0; k < K; k++) {
            void *a = NULL, *b = NULL;
            CHECK_HIP(hipMalloc(&a, counts[k] * 2));
            CHECK_HIP(hipMalloc(&r16[s][k], counts[k] * 2));
            CHECK_HIP(hipMemset(a, 0x3c, counts[k] * 2)); /* 0x3c3c: 1.0586 (float16), 0.0115 (bfloat16) */
            CHECK_HIP(hipMalloc(&b, counts[k] * 4));
            CHECK_HIP(hipMalloc(&r32[s][k], counts[k] * 4));
            CHECK_HIP(hipMemset(b, 0, counts[k] * 4));
            s16[s][k] = a;
            s32[s][k] = b;
        }
    float *ps[2], *pr[2];
    for (int s = 0; s < 2; s++) {
        CHECK_HIP(hipMalloc((void **)&ps[s], total * 4));
        CHECK_HIP(hipMalloc((void **)&pr[s], total * 4));
        CHECK_HIP(hipMemset(ps[s], 0, total * 4));
    }
    CHECK_HIP(hipDeviceSynchronize());
    ftar_set_profiling(comm, 1);
    ftar_stats st;
    double *t[4];
    for (int j = 0; j < 4; j++) t[j] = malloc(sizeof(double) * (size_t)iters);
    int bad = 0;
    for (int it = -3; it < iters; it++) {
        const int s = it & 1;
        double v[4];
        bad |= ftar_allreduce_multi_acc32(FTAR_ALGO_RABENSEIFNER, s16[s], r16[s], counts, K, FTAR_BFLOAT16, FTAR_SUM, 1.0f, comm);
        ftar_last_stats(comm, &st);
        v[0] = st.kernel_ms;
        bad |= ftar_allreduce_multi_acc32(FTAR_ALGO_RABENSEIFNER, s16[s], r16[s], counts, K, FTAR_FLOAT16, FTAR_SUM, 1.0f, comm);
        ftar_last_stats(comm, &st);
        v[1] = st.kernel_ms;
        bad |= ftar_allreduce_multi(FTAR_ALGO_RABENSEIFNER, s32[s], r32[s], counts, K, FTAR_FLOAT32, FTAR_SUM, comm);
        ftar_last_stats(comm, &st);
        v[2] = st.kernel_ms;
        bad |= ftar_allreduce_rabenseifner(ps[s], pr[s], total, FTAR_FLOAT32, FTAR_SUM, comm);
        ftar_last_stats(comm, &st);
        v[3] = st.kernel_ms;
        if (it < 0) continue;
        printf("{\"round\": %d, \"acc32_bf16_ms\": %.4f, \"acc32_f16_ms\": %.4f, \"multi_f32_ms\": %.4f, \"plain_copy_ms\": %.4f}\n", it,
               v[0], v[1], v[2], v[3]);
        for (int j = 0; j < 3; j++) t[j][it] = v[j] - v[3]; /* the mover's two launches */
        t[3][it] = v[3];
    }
    unsigned short h = 0;
    CHECK_HIP(hipMemcpy(&h, r16[0][K - 1], 2, hipMemcpyDeviceToHost));
    const double el = (double)total;
    const char *name[3] = {"acc32_bf16", "acc32_f16", "multi_f32"};
    const double bytes[3] = {12, 12, 16}; /* per element, gather + scatter */
    printf("{\"entries\": %d, \"uneven\": %d, \"elements\": %zu, \"packed_mib\": %.1f, \"iterations\": %d, \"rc\": %d, \"checked\": %s",
           K, uneven, total, el * 4 / (1 << 20), iters, bad, h == 0x3c3c ? "true" : "false");
    for (int j = 0; j < 3; j++) {
        const double med = pct(t[j], iters, 0.5), lo = pct(t[j], iters, 0.0), hi = pct(t[j], iters, 1.0);
        printf(", \"%s_mover_ms\": {\"median\": %.4f, \"min\": %.4f, \"max\": %.4f, \"tb_per_s\": %.3f}", name[j], med, lo, hi,
               bytes[j] * el / (med * 1e-3) / 1e12);
    }
    printf("}\n");
    fflush(stdout);
    ftar_finalize(comm);
    return bad != 0;
}
