/*
 * measure.c -- the two measurements of profiles/multi/README.md, one rank of an ftrun job.
 *
 *   ftrun -np N --devmap 0,0 measure small <K> <elements per buffer> <iterations>
 *       K float32 buffers, each a hipMalloc of its own.  After 20 warm-up rounds, `iterations`
 *       rounds of: one ftar_allreduce_multi over the list (timed), then the same K buffers as K
 *       plain ftar_allreduce_rabenseifner calls (timed as one span).  Host wall clock around the
 *       blocking calls; prints the medians, the 10th / 90th percentiles and the ratio.
 *
 *   ftrun -np 1 --devmap 0 measure large <K> <total MiB> <iterations>
 *       K equal 16-byte-aligned float32 buffers of <total MiB> in all, two such lists used in turn
 *       (and two pairs of plain buffers), so that with the staging vectors more than 1 GiB passes
 *       through the 256 MiB Infinity Cache between two uses of a byte.  With ftar_set_profiling
 *       on, per round: the device time of all kernels of one multi call (gather + the one-rank
 *       schedule's segment-kernel copy of the packed vector + scatter) and of one plain call on
 *       <total MiB> (that same segment-kernel copy alone).  Prints the medians and the rates.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

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

static double now_us(void)
{
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return t.tv_sec * 1e6 + t.tv_nsec * 1e-3;
}

static int by_val(const void *a, const void *b) { return *(const double *)a < *(const double *)b ? -1 : *(const double *)a > *(const double *)b; }
static double pct(double *v, int n, double q)
{
    qsort(v, (size_t)n, sizeof(double), by_val);
    return v[(int)(q * (n - 1) + 0.5)];
}

int main(int argc, char **argv)
{
    if (argc < 5) return 2;
    const int large = !strcmp(argv[1], "large");
    const int K = atoi(argv[2]), iters = atoi(argv[4]);
    if (K < 1 || K > FTAR_MULTI_MAX || iters < 1 || iters > 100000) return 2;
    const size_t per = large ? (size_t)atoll(argv[3]) * (1 << 20) / 4 / (size_t)K : (size_t)atoll(argv[3]);
    ftar_comm *comm;
    if (ftar_init(&comm) != FTAR_SUCCESS) return 3;
    int rank, size, dev;
    ftar_world_rank(comm, &rank);
    ftar_world_size(comm, &size);
    ftar_comm_device(comm, &dev);
    CHECK_HIP(hipSetDevice(dev));
    const int sets = large ? 2 : 1;
    static const void *sb[2][FTAR_MULTI_MAX];
    static void *rb[2][FTAR_MULTI_MAX];
    static size_t counts[FTAR_MULTI_MAX];
    float *h = malloc(per * sizeof(float));
    for (size_t i = 0; i < per; i++) h[i] = (float)(rank + 1);
    for (int s = 0; s < sets; s++)
        for (int k = 0; k < K; k++) {
            void *a = NULL;
            CHECK_HIP(hipMalloc(&a, per * sizeof(float)));
            CHECK_HIP(hipMalloc(&rb[s][k], per * sizeof(float)));
            CHECK_HIP(hipMemcpy(a, h, per * sizeof(float), hipMemcpyHostToDevice));
            sb[s][k] = a;
            counts[k] = per;
        }
    double *tm = malloc(sizeof(double) * (size_t)iters), *tp = malloc(sizeof(double) * (size_t)iters);
    int bad = 0;
    if (!large) {
        for (int it = -20; it < iters; it++) {
            double t0 = now_us();
            bad |= ftar_allreduce_multi(FTAR_ALGO_RABENSEIFNER, sb[0], rb[0], counts, K, FTAR_FLOAT32, FTAR_SUM, comm);
            double t1 = now_us();
            for (int k = 0; k < K; k++)
                bad |= ftar_allreduce_rabenseifner(sb[0][k], rb[0][k], per, FTAR_FLOAT32, FTAR_SUM, comm);
            double t2 = now_us();
            if (it >= 0) tm[it] = t1 - t0, tp[it] = t2 - t1;
        }
        CHECK_HIP(hipMemcpy(h, rb[0][K - 1], per * sizeof(float), hipMemcpyDeviceToHost));
        const float want = (float)(size * (size + 1) / 2);
        const double mm = pct(tm, iters, 0.5), mp = pct(tp, iters, 0.5);
        printf("{\"mode\": \"small\", \"rank\": %d, \"ranks\": %d, \"buffers\": %d, \"elements_each\": %zu, \"iterations\": %d, "
               "\"multi_us\": %.2f, \"multi_p10_p90\": [%.2f, %.2f], \"plain_calls_us\": %.2f, \"plain_p10_p90\": [%.2f, %.2f], "
               "\"ratio\": %.2f, \"rc\": %d, \"checked\": %s}\n",
               rank, size, K, per, iters, mm, pct(tm, iters, 0.1), pct(tm, iters, 0.9), mp, pct(tp, iters, 0.1),
               pct(tp, iters, 0.9), mp / mm, bad, h[0] == want && h[per - 1] == want ? "true" : "false");
    } else {
        const size_t total = per * (size_t)K;
        float *ps[2], *pr[2];
        for (int s = 0; s < 2; s++) {
            CHECK_HIP(hipMalloc((void **)&ps[s], total * sizeof(float)));
            CHECK_HIP(hipMalloc((void **)&pr[s], total * sizeof(float)));
            CHECK_HIP(hipMemset(ps[s], 0, total * sizeof(float)));
        }
        ftar_set_profiling(comm, 1);
        ftar_stats st;
        int nk = 0;
        for (int it = -3; it < iters; it++) {
            const int s = it & 1;
            bad |= ftar_allreduce_multi(FTAR_ALGO_RABENSEIFNER, sb[s], rb[s], counts, K, FTAR_FLOAT32, FTAR_SUM, comm);
            ftar_last_stats(comm, &st);
            if (it >= 0) tm[it] = st.kernel_ms, nk = st.kernels;
            bad |= ftar_allreduce_rabenseifner(ps[s], pr[s], total, FTAR_FLOAT32, FTAR_SUM, comm);
            ftar_last_stats(comm, &st);
            if (it >= 0) tp[it] = st.kernel_ms;
        }
        CHECK_HIP(hipMemcpy(h, rb[0][K - 1], per * sizeof(float), hipMemcpyDeviceToHost));
        const double mm = pct(tm, iters, 0.5), mp = pct(tp, iters, 0.5), gib = (double)total * 4 / (1 << 30);
        printf("{\"mode\": \"large\", \"buffers\": %d, \"total_mib\": %.0f, \"iterations\": %d, \"multi_kernels\": %d, "
               "\"multi_kernel_ms\": %.4f, \"multi_min_max\": [%.4f, %.4f], \"segment_copy_ms\": %.4f, \"segment_min_max\": [%.4f, %.4f], "
               "\"gather_plus_scatter_ms\": %.4f, \"segment_copy_gb_s\": %.1f, \"gather_scatter_mean_gb_s\": %.1f, \"rc\": %d, "
               "\"checked\": %s}\n",
               K, gib * 1024, iters, nk, mm, pct(tm, iters, 0.0), pct(tm, iters, 1.0), mp, pct(tp, iters, 0.0),
               pct(tp, iters, 1.0), mm - mp, 2 * gib * 1.073741824 / (mp * 1e-3), 4 * gib * 1.073741824 / ((mm - mp) * 1e-3), bad,
               h[0] == (float)(rank + 1) ? "true" : "false");
    }
    fflush(stdout);
    ftar_finalize(comm);
    return bad != 0;
}
