/*
 * ftbench -- one rank of a timed, device-resident Allreduce job under ftrun: the C5 leg
 * of bench.py (BASELINE configs[4]: Rabenseifner, 256 MiB float32 SUM, 9 ranks = 8 GPUs +
 * one idle spare, a single kill mid-exchange, ULFM-style shrink + recovery).
 *
 *   ftrun -np N --devmap d0,d1,... ftbench <raben|rd> <count> <calls> [f32|f16|bf16|float_int|2int|double_int]
 *
 * The element type is float32 unless the 4th argument or FTBENCH_DTYPE names another (the
 * argument wins): float16 and bfloat16 time the same job on 2-byte elements.  Their inputs are
 * small integers whose sums stay exact in 8 significand bits -- the rank modulo 4, or with
 * FTBENCH_PATTERN (7 i + 13 r) mod 4 -- so that at up to 64 ranks every partial sum is an
 * integer below 256: finite, and the same in any reduction tree.
 * float_int, 2int and double_int time MAXLOC on MPI's pair types: every rank contributes the
 * value f(rank, i) -- its rank, or with FTBENCH_PATTERN (7 i + 13 r) mod 3, which ties between
 * ranks from 4 ranks on -- and its rank as the index; the check recomputes each element's winner
 * (the largest value, the lowest rank among equals) on the host.
 *
 * FTBENCH_MULTI=K (float32, float16, bfloat16; 1 <= K <= min(count, FTAR_MULTI_MAX)): the job's `count` is
 * split into K buffers as equal as possible, each send and receive buffer a hipMalloc of its own, and
 * every call is one ftar_allreduce_multi over the list; the check and the output line are unchanged.
 * FTBENCH_ACC32=1 (with FTBENCH_MULTI and a 16-bit type): the call is ftar_allreduce_multi_acc32 with
 * scale 1 instead -- float32 accumulation; the sums are exact either way, so the check is the same.
 * FTBENCH_MIXED=1 (with FTBENCH_MULTI; no element type, or f32): buffer k is bfloat16, float32, float16 for
 * k mod 3 = 0, 1, 2 and the call is ftar_allreduce_multi_mixed with scale 1; the inputs are the 16-bit job's
 * small integers, exact in all three types, so the check and the output line are the same again.
 *
 * Every rank hipMallocs float32 send / receive vectors of `count` elements on its device,
 * fills the send vector with its original rank (the reference drivers' input,
 * rd/recursive_doubling.c:112-115 / raben/rabenseifner.c:408-411, as float32: every
 * partial sum is an exact integer, so the result is independent of the reduction tree)
 * and runs `calls` Allreduces through the C ABI.  FTAR_KILL (with a call index, e.g.
 * "6:1:1:3:1") injects the fault.  Per call it records the library's wall time
 * (ftar_last_stats), the recoveries, the comm size after the call, and the result read
 * back after the timed region: its first element and whether every element equals it.
 * One JSON line per surviving rank on stdout.  The reference's own numbers for this case
 * are data/data_fault/log_single_Raben.csv (N = 9, clock() seconds per run).
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <hip/hip_runtime_api.h>

#include "ftar.h"

#define MAX_CALLS 16

#define CHECK_HIP(x)                                                                               \
    do {                                                                                           \
        hipError_t e_ = (x);                                                                       \
        if (e_ != hipSuccess) {                                                                    \
            fprintf(stderr, "ftbench: %s: %s\n", #x, hipGetErrorString(e_));                       \
            return 1;                                                                              \
        }                                                                                          \
    } while (0)

/* float32 -> the 16-bit formats and back, for integers of at most 8 significand bits (exact:
 * nothing to round, no subnormals) */
static uint16_t to_bf16(float v)
{
    uint32_t u;
    memcpy(&u, &v, 4);
    return (uint16_t)(u >> 16);
}
static float from_bf16(uint16_t h)
{
    uint32_t u = (uint32_t)h << 16;
    float v;
    memcpy(&v, &u, 4);
    return v;
}
static uint16_t to_f16(float v)
{
    uint32_t u;
    memcpy(&u, &v, 4);
    if ((u & 0x7fffffffu) == 0) return (uint16_t)(u >> 16);
    return (uint16_t)(((u >> 16) & 0x8000u) | ((((u >> 23) & 0xffu) - 127 + 15) << 10) | ((u >> 13) & 0x3ffu));
}
static float from_f16(uint16_t h)
{
    uint32_t u = (uint32_t)(h & 0x8000u) << 16;
    if (h & 0x7fffu) u |= ((((uint32_t)h >> 10) & 0x1fu) - 15 + 127) << 23 | ((uint32_t)h & 0x3ffu) << 13;
    float v;
    memcpy(&v, &u, 4);
    return v;
}

/* the 16-bit job: same schedule calls, same JSON line */
static int run16(int rd, size_t count, int calls, ftar_dtype dt, ftar_comm *comm, int wrank, int wsize, int dev,
                 int multi, int acc32);
/* the mixed-list job: ftar_allreduce_multi_mixed over bfloat16, float32 and float16 buffers in turn */
static int runmixed(int rd, size_t count, int calls, ftar_comm *comm, int wrank, int wsize, int dev, int multi);
/* the pair-type job (MAXLOC) */
static int runpair(int rd, size_t count, int calls, ftar_dtype dt, ftar_comm *comm, int wrank, int wsize, int dev);
/* the job on the 8-, 16-bit and unsigned integers (SUM, checked modulo 2^w) */
static int runint(int rd, size_t count, int calls, ftar_dtype dt, ftar_comm *comm, int wrank, int wsize, int dev);

int main(int argc, char **argv)
{
    if (argc < 4) {
        fprintf(stderr, "usage: ftbench <raben|rd> <count> <calls> [f32|f16|bf16|float_int|2int|double_int|i8|u8|i16|u16|u32|u64]\n");
        return 2;
    }
    int rd = !strcmp(argv[1], "rd");
    size_t count = strtoull(argv[2], NULL, 10);
    int calls = atoi(argv[3]);
    if (count == 0 || calls < 1 || calls > MAX_CALLS) return 2;
    const char *tn = argc > 4 ? argv[4] : getenv("FTBENCH_DTYPE");
    int dt16 = 0, dtpair = 0, dtint = -1;
    if (tn && *tn && strcmp(tn, "f32")) {
        if (!strcmp(tn, "f16")) dt16 = FTAR_FLOAT16;
        else if (!strcmp(tn, "bf16")) dt16 = FTAR_BFLOAT16;
        else if (!strcmp(tn, "float_int")) dtpair = FTAR_FLOAT_INT;
        else if (!strcmp(tn, "2int")) dtpair = FTAR_2INT;
        else if (!strcmp(tn, "double_int")) dtpair = FTAR_DOUBLE_INT;
        else if (!strcmp(tn, "i8")) dtint = FTAR_INT8;
        else if (!strcmp(tn, "u8")) dtint = FTAR_UINT8;
        else if (!strcmp(tn, "i16")) dtint = FTAR_INT16;
        else if (!strcmp(tn, "u16")) dtint = FTAR_UINT16;
        else if (!strcmp(tn, "u32")) dtint = FTAR_UINT32;
        else if (!strcmp(tn, "u64")) dtint = FTAR_UINT64;
        else {
            fprintf(stderr, "ftbench: element type %s is not f32, f16, bf16, float_int, 2int, double_int, i8, u8, i16, "
                            "u16, u32 or u64\n", tn);
            return 2;
        }
    }

    ftar_comm *comm;
    if (ftar_init(&comm) != FTAR_SUCCESS) return 3;
    int wrank, wsize, dev;
    ftar_world_rank(comm, &wrank);
    ftar_world_size(comm, &wsize);
    ftar_comm_device(comm, &dev);
    CHECK_HIP(hipSetDevice(dev));
    const char *me = getenv("FTBENCH_MULTI");
    const int multi = me && *me ? atoi(me) : 0;
    if (me && *me && (multi < 1 || multi > FTAR_MULTI_MAX || (size_t)multi > count || dtpair || dtint >= 0)) {
        fprintf(stderr, "ftbench: FTBENCH_MULTI=%s: 1 .. min(count, %d) buffers of f32, f16 or bf16\n", me,
                FTAR_MULTI_MAX);
        return 2;
    }
    const char *ae = getenv("FTBENCH_ACC32");
    const int acc32 = ae && atoi(ae) != 0;
    if (acc32 && !(multi && dt16)) {
        fprintf(stderr, "ftbench: FTBENCH_ACC32 needs FTBENCH_MULTI and f16 or bf16\n");
        return 2;
    }
    const char *xe = getenv("FTBENCH_MIXED");
    if (xe && atoi(xe) != 0) {
        if (!multi || dt16 || acc32) {
            fprintf(stderr, "ftbench: FTBENCH_MIXED needs FTBENCH_MULTI, no element type (or f32) and no FTBENCH_ACC32\n");
            return 2;
        }
        return runmixed(rd, count, calls, comm, wrank, wsize, dev, multi);
    }
    if (dt16) return run16(rd, count, calls, (ftar_dtype)dt16, comm, wrank, wsize, dev, multi, acc32);
    if (dtpair) return runpair(rd, count, calls, (ftar_dtype)dtpair, comm, wrank, wsize, dev);
    if (dtint >= 0) return runint(rd, count, calls, (ftar_dtype)dtint, comm, wrank, wsize, dev);

    /* FTBENCH_PATTERN=1: x_r[i] = (7 i + 13 r) mod 4096 instead of r, so every element
     * has its own exact sum (all partial sums are integers < 2^24) and a misplaced
     * window or a 32-bit index wrap shows as a wrong element (the size tests beyond
     * 2^31 elements); "uniform" then means "every element equals its exact sum". */
    const char *pe = getenv("FTBENCH_PATTERN");
    const int pattern = pe && atoi(pe) != 0;
    float *h = malloc(count * sizeof(float));
    if (!h) return 4;
    for (size_t i = 0; i < count; i++) h[i] = pattern ? (float)((7 * i + 13 * (size_t)wrank) % 4096) : (float)wrank;
    float *s = NULL, *r = NULL;
    static const void *ms_[FTAR_MULTI_MAX];
    static void *mr_[FTAR_MULTI_MAX];
    static size_t mc_[FTAR_MULTI_MAX];
    if (multi) {
        size_t off = 0;
        for (int k = 0; k < multi; k++) {
            mc_[k] = count / (size_t)multi + ((size_t)k < count % (size_t)multi);
            void *a = NULL;
            CHECK_HIP(hipMalloc(&a, mc_[k] * sizeof(float)));
            CHECK_HIP(hipMalloc(&mr_[k], mc_[k] * sizeof(float)));
            CHECK_HIP(hipMemcpy(a, h + off, mc_[k] * sizeof(float), hipMemcpyHostToDevice));
            ms_[k] = a;
            off += mc_[k];
        }
    } else {
        CHECK_HIP(hipMalloc((void **)&s, count * sizeof(float)));
        CHECK_HIP(hipMalloc((void **)&r, count * sizeof(float)));
        CHECK_HIP(hipMemcpy(s, h, count * sizeof(float), hipMemcpyHostToDevice));
    }
    CHECK_HIP(hipDeviceSynchronize());

    double ms[MAX_CALLS], value[MAX_CALLS], hbm[MAX_CALLS];
    int rc[MAX_CALLS], rec[MAX_CALLS], size_after[MAX_CALLS], uniform[MAX_CALLS], step0_copy = 0;
    for (int c = 0; c < calls; c++) {
        if (multi)
            rc[c] = ftar_allreduce_multi(rd ? FTAR_ALGO_RD : FTAR_ALGO_RABENSEIFNER, ms_, mr_, mc_, multi, FTAR_FLOAT32,
                                         FTAR_SUM, comm);
        else
            rc[c] = rd ? ftar_recursive_doubling(s, r, count, FTAR_FLOAT32, FTAR_SUM, comm)
                       : ftar_allreduce_rabenseifner(s, r, count, FTAR_FLOAT32, FTAR_SUM, comm);
        ftar_stats st;
        ftar_last_stats(comm, &st);
        ms[c] = st.wall_s * 1e3;
        hbm[c] = st.hbm_bytes; /* algorithmic local HBM bytes of this rank's kernels */
        rec[c] = st.recoveries;
        size_after[c] = st.comm_size_after;
        step0_copy |= st.step0_copy;
        /* outside the call's timed region: read the result back and check it is uniform */
        if (multi) {
            size_t off = 0;
            for (int k = 0; k < multi; off += mc_[k], k++)
                CHECK_HIP(hipMemcpy(h + off, mr_[k], mc_[k] * sizeof(float), hipMemcpyDeviceToHost));
        } else {
            CHECK_HIP(hipMemcpy(h, r, count * sizeof(float), hipMemcpyDeviceToHost));
        }
        value[c] = h[0];
        uniform[c] = 1;
        const int members = size_after[c]; /* the original ranks 0 .. members-1 (no fault) */
        for (size_t i = 0; i < count; i++) {
            float want = h[0];
            if (pattern) {
                size_t sum = 0;
                for (int q = 0; q < members; q++) sum += (7 * i + 13 * (size_t)q) % 4096;
                want = (float)sum;
            }
            if (h[i] != want) {
                uniform[c] = 0;
                break;
            }
        }
    }
    printf("{\"rank\": %d, \"size\": %d, \"device\": %d, \"step0_copy\": %d, \"calls\": [", wrank, wsize, dev,
           step0_copy);
    for (int c = 0; c < calls; c++)
        printf("%s{\"rc\": %d, \"ms\": %.4f, \"recoveries\": %d, \"comm_size\": %d, \"value\": %.1f, \"uniform\": %s, "
               "\"hbm_bytes\": %.0f}",
               c ? ", " : "", rc[c], ms[c], rec[c], size_after[c], value[c], uniform[c] ? "true" : "false", hbm[c]);
    printf("]}\n");
    fflush(stdout);
    ftar_finalize(comm);
    for (int k = 0; k < multi; k++) {
        (void)hipFree((void *)(uintptr_t)ms_[k]);
        (void)hipFree(mr_[k]);
    }
    (void)hipFree(s);
    (void)hipFree(r);
    free(h);
    return 0;
}

static int run16(int rd, size_t count, int calls, ftar_dtype dt, ftar_comm *comm, int wrank, int wsize, int dev,
                 int multi, int acc32)
{
    const char *pe = getenv("FTBENCH_PATTERN");
    const int pattern = pe && atoi(pe) != 0;
    const int bf = dt == FTAR_BFLOAT16;
    uint16_t *h = malloc(count * sizeof(uint16_t));
    if (!h) return 4;
    for (size_t i = 0; i < count; i++) {
        const float v = pattern ? (float)((7 * i + 13 * (size_t)wrank) % 4) : (float)(wrank % 4);
        h[i] = bf ? to_bf16(v) : to_f16(v);
    }
    uint16_t *s = NULL, *r = NULL;
    static const void *ms_[FTAR_MULTI_MAX];
    static void *mr_[FTAR_MULTI_MAX];
    static size_t mc_[FTAR_MULTI_MAX];
    if (multi) {
        size_t off = 0;
        for (int k = 0; k < multi; k++) {
            mc_[k] = count / (size_t)multi + ((size_t)k < count % (size_t)multi);
            void *a = NULL;
            CHECK_HIP(hipMalloc(&a, mc_[k] * sizeof(uint16_t)));
            CHECK_HIP(hipMalloc(&mr_[k], mc_[k] * sizeof(uint16_t)));
            CHECK_HIP(hipMemcpy(a, h + off, mc_[k] * sizeof(uint16_t), hipMemcpyHostToDevice));
            ms_[k] = a;
            off += mc_[k];
        }
    } else {
        CHECK_HIP(hipMalloc((void **)&s, count * sizeof(uint16_t)));
        CHECK_HIP(hipMalloc((void **)&r, count * sizeof(uint16_t)));
        CHECK_HIP(hipMemcpy(s, h, count * sizeof(uint16_t), hipMemcpyHostToDevice));
    }
    CHECK_HIP(hipDeviceSynchronize());

    double ms[MAX_CALLS], value[MAX_CALLS], hbm[MAX_CALLS];
    int rc[MAX_CALLS], rec[MAX_CALLS], size_after[MAX_CALLS], uniform[MAX_CALLS], step0_copy = 0;
    for (int c = 0; c < calls; c++) {
        const ftar_algo al = rd ? FTAR_ALGO_RD : FTAR_ALGO_RABENSEIFNER;
        if (acc32) rc[c] = ftar_allreduce_multi_acc32(al, ms_, mr_, mc_, multi, dt, FTAR_SUM, 1.0f, comm);
        else if (multi) rc[c] = ftar_allreduce_multi(al, ms_, mr_, mc_, multi, dt, FTAR_SUM, comm);
        else
            rc[c] = rd ? ftar_recursive_doubling(s, r, count, dt, FTAR_SUM, comm)
                       : ftar_allreduce_rabenseifner(s, r, count, dt, FTAR_SUM, comm);
        ftar_stats st;
        ftar_last_stats(comm, &st);
        ms[c] = st.wall_s * 1e3;
        hbm[c] = st.hbm_bytes;
        rec[c] = st.recoveries;
        size_after[c] = st.comm_size_after;
        step0_copy |= st.step0_copy;
        if (multi) {
            size_t off = 0;
            for (int k = 0; k < multi; off += mc_[k], k++)
                CHECK_HIP(hipMemcpy(h + off, mr_[k], mc_[k] * sizeof(uint16_t), hipMemcpyDeviceToHost));
        } else {
            CHECK_HIP(hipMemcpy(h, r, count * sizeof(uint16_t), hipMemcpyDeviceToHost));
        }
        value[c] = bf ? from_bf16(h[0]) : from_f16(h[0]);
        uniform[c] = 1;
        const int members = size_after[c];
        for (size_t i = 0; i < count; i++) {
            uint16_t want = h[0];
            if (pattern) {
                size_t sum = 0;
                for (int q = 0; q < members; q++) sum += (7 * i + 13 * (size_t)q) % 4;
                want = bf ? to_bf16((float)sum) : to_f16((float)sum);
            }
            if (h[i] != want) {
                uniform[c] = 0;
                break;
            }
        }
    }
    printf("{\"rank\": %d, \"size\": %d, \"device\": %d, \"step0_copy\": %d, \"calls\": [", wrank, wsize, dev,
           step0_copy);
    for (int c = 0; c < calls; c++)
        printf("%s{\"rc\": %d, \"ms\": %.4f, \"recoveries\": %d, \"comm_size\": %d, \"value\": %.1f, \"uniform\": %s, "
               "\"hbm_bytes\": %.0f}",
               c ? ", " : "", rc[c], ms[c], rec[c], size_after[c], value[c], uniform[c] ? "true" : "false", hbm[c]);
    printf("]}\n");
    fflush(stdout);
    ftar_finalize(comm);
    for (int k = 0; k < multi; k++) {
        (void)hipFree((void *)(uintptr_t)ms_[k]);
        (void)hipFree(mr_[k]);
    }
    (void)hipFree(s);
    (void)hipFree(r);
    free(h);
    return 0;
}

static const ftar_dtype mixed_cycle[3] = {FTAR_BFLOAT16, FTAR_FLOAT32, FTAR_FLOAT16};

/* element i of a buffer of type dt */
static void mixed_put(void *buf, ftar_dtype dt, size_t i, float v)
{
    if (dt == FTAR_FLOAT32) ((float *)buf)[i] = v;
    else ((uint16_t *)buf)[i] = dt == FTAR_BFLOAT16 ? to_bf16(v) : to_f16(v);
}
static float mixed_get(const void *buf, ftar_dtype dt, size_t i)
{
    if (dt == FTAR_FLOAT32) return ((const float *)buf)[i];
    return dt == FTAR_BFLOAT16 ? from_bf16(((const uint16_t *)buf)[i]) : from_f16(((const uint16_t *)buf)[i]);
}

static int runmixed(int rd, size_t count, int calls, ftar_comm *comm, int wrank, int wsize, int dev, int multi)
{
    const char *pe = getenv("FTBENCH_PATTERN");
    const int pattern = pe && atoi(pe) != 0;
    float *h = malloc(count * sizeof(float)); /* the dense vector's values */
    void *stage = malloc((count / (size_t)multi + 1) * sizeof(float));
    if (!h || !stage) return 4;
    for (size_t i = 0; i < count; i++) h[i] = pattern ? (float)((7 * i + 13 * (size_t)wrank) % 4) : (float)(wrank % 4);
    static const void *ms_[FTAR_MULTI_MAX];
    static void *mr_[FTAR_MULTI_MAX];
    static size_t mc_[FTAR_MULTI_MAX];
    static ftar_dtype mt_[FTAR_MULTI_MAX];
    size_t off = 0;
    for (int k = 0; k < multi; k++) {
        mc_[k] = count / (size_t)multi + ((size_t)k < count % (size_t)multi);
        mt_[k] = mixed_cycle[k % 3];
        const size_t b = mc_[k] * (mt_[k] == FTAR_FLOAT32 ? 4 : 2);
        for (size_t i = 0; i < mc_[k]; i++) mixed_put(stage, mt_[k], i, h[off + i]);
        void *a = NULL;
        CHECK_HIP(hipMalloc(&a, b));
        CHECK_HIP(hipMalloc(&mr_[k], b));
        CHECK_HIP(hipMemcpy(a, stage, b, hipMemcpyHostToDevice));
        ms_[k] = a;
        off += mc_[k];
    }
    CHECK_HIP(hipDeviceSynchronize());

    double ms[MAX_CALLS], value[MAX_CALLS], hbm[MAX_CALLS];
    int rc[MAX_CALLS], rec[MAX_CALLS], size_after[MAX_CALLS], uniform[MAX_CALLS], step0_copy = 0;
    for (int c = 0; c < calls; c++) {
        rc[c] = ftar_allreduce_multi_mixed(rd ? FTAR_ALGO_RD : FTAR_ALGO_RABENSEIFNER, ms_, mr_, mc_, mt_, multi, FTAR_SUM,
                                           1.0f, comm);
        ftar_stats st;
        ftar_last_stats(comm, &st);
        ms[c] = st.wall_s * 1e3;
        hbm[c] = st.hbm_bytes;
        rec[c] = st.recoveries;
        size_after[c] = st.comm_size_after;
        step0_copy |= st.step0_copy;
        off = 0;
        for (int k = 0; k < multi; off += mc_[k], k++) {
            CHECK_HIP(hipMemcpy(stage, mr_[k], mc_[k] * (mt_[k] == FTAR_FLOAT32 ? 4 : 2), hipMemcpyDeviceToHost));
            for (size_t i = 0; i < mc_[k]; i++) h[off + i] = mixed_get(stage, mt_[k], i);
        }
        value[c] = h[0];
        uniform[c] = 1;
        const int members = size_after[c];
        for (size_t i = 0; i < count; i++) {
            float want = h[0];
            if (pattern) {
                size_t sum = 0;
                for (int q = 0; q < members; q++) sum += (7 * i + 13 * (size_t)q) % 4;
                want = (float)sum;
            }
            if (h[i] != want) {
                uniform[c] = 0;
                break;
            }
        }
    }
    printf("{\"rank\": %d, \"size\": %d, \"device\": %d, \"step0_copy\": %d, \"calls\": [", wrank, wsize, dev,
           step0_copy);
    for (int c = 0; c < calls; c++)
        printf("%s{\"rc\": %d, \"ms\": %.4f, \"recoveries\": %d, \"comm_size\": %d, \"value\": %.1f, \"uniform\": %s, "
               "\"hbm_bytes\": %.0f}",
               c ? ", " : "", rc[c], ms[c], rec[c], size_after[c], value[c], uniform[c] ? "true" : "false", hbm[c]);
    printf("]}\n");
    fflush(stdout);
    ftar_finalize(comm);
    for (int k = 0; k < multi; k++) {
        (void)hipFree((void *)(uintptr_t)ms_[k]);
        (void)hipFree(mr_[k]);
    }
    free(stage);
    free(h);
    return 0;
}

/* rank q's contribution to element i: the value (a small integer, exact in every value type) */
static int pair_value(int pattern, size_t i, int q) { return pattern ? (int)((7 * i + 13 * (size_t)q) % 3) : q; }

static void pair_put(void *buf, ftar_dtype dt, size_t i, int v, int idx)
{
    if (dt == FTAR_FLOAT_INT) ((ftar_float_int *)buf)[i] = (ftar_float_int){(float)v, idx};
    else if (dt == FTAR_2INT) ((ftar_2int *)buf)[i] = (ftar_2int){v, idx};
    else ((ftar_double_int *)buf)[i] = (ftar_double_int){(double)v, idx};
}

static void pair_get(const void *buf, ftar_dtype dt, size_t i, double *v, int *idx)
{
    if (dt == FTAR_FLOAT_INT) *v = ((const ftar_float_int *)buf)[i].v, *idx = ((const ftar_float_int *)buf)[i].i;
    else if (dt == FTAR_2INT) *v = ((const ftar_2int *)buf)[i].v, *idx = ((const ftar_2int *)buf)[i].i;
    else *v = ((const ftar_double_int *)buf)[i].v, *idx = ((const ftar_double_int *)buf)[i].i;
}

static int runpair(int rd, size_t count, int calls, ftar_dtype dt, ftar_comm *comm, int wrank, int wsize, int dev)
{
    const char *pe = getenv("FTBENCH_PATTERN");
    const int pattern = pe && atoi(pe) != 0;
    const size_t es = dt == FTAR_DOUBLE_INT ? sizeof(ftar_double_int) : sizeof(ftar_2int);
    void *h = calloc(count, es); /* (zeroed: the padding of ftar_double_int too) */
    if (!h) return 4;
    for (size_t i = 0; i < count; i++) pair_put(h, dt, i, pair_value(pattern, i, wrank), wrank);
    void *s = NULL, *r = NULL;
    CHECK_HIP(hipMalloc(&s, count * es));
    CHECK_HIP(hipMalloc(&r, count * es));
    CHECK_HIP(hipMemcpy(s, h, count * es, hipMemcpyHostToDevice));
    CHECK_HIP(hipDeviceSynchronize());

    double ms[MAX_CALLS], value[MAX_CALLS], hbm[MAX_CALLS];
    int rc[MAX_CALLS], rec[MAX_CALLS], size_after[MAX_CALLS], uniform[MAX_CALLS], index[MAX_CALLS], step0_copy = 0;
    for (int c = 0; c < calls; c++) {
        rc[c] = rd ? ftar_recursive_doubling(s, r, count, dt, FTAR_MAXLOC, comm)
                   : ftar_allreduce_rabenseifner(s, r, count, dt, FTAR_MAXLOC, comm);
        ftar_stats st;
        ftar_last_stats(comm, &st);
        ms[c] = st.wall_s * 1e3;
        hbm[c] = st.hbm_bytes;
        rec[c] = st.recoveries;
        size_after[c] = st.comm_size_after;
        step0_copy |= st.step0_copy;
        CHECK_HIP(hipMemcpy(h, r, count * es, hipMemcpyDeviceToHost));
        pair_get(h, dt, 0, &value[c], &index[c]);
        uniform[c] = 1;
        const int members = size_after[c]; /* the original ranks 0 .. members-1 (no fault) */
        for (size_t i = 0; i < count; i++) {
            /* the winner over the members: the largest value, the lowest rank among equals */
            int wv = pair_value(pattern, i, 0), wi = 0;
            for (int q = 1; q < members; q++)
                if (pair_value(pattern, i, q) > wv) wv = pair_value(pattern, i, q), wi = q;
            double v;
            int idx;
            pair_get(h, dt, i, &v, &idx);
            if (v != (double)wv || idx != wi) {
                uniform[c] = 0;
                break;
            }
        }
    }
    printf("{\"rank\": %d, \"size\": %d, \"device\": %d, \"step0_copy\": %d, \"calls\": [", wrank, wsize, dev,
           step0_copy);
    for (int c = 0; c < calls; c++)
        printf("%s{\"rc\": %d, \"ms\": %.4f, \"recoveries\": %d, \"comm_size\": %d, \"value\": %.1f, \"index\": %d, "
               "\"uniform\": %s, \"hbm_bytes\": %.0f}",
               c ? ", " : "", rc[c], ms[c], rec[c], size_after[c], value[c], index[c], uniform[c] ? "true" : "false",
               hbm[c]);
    printf("]}\n");
    fflush(stdout);
    ftar_finalize(comm);
    (void)hipFree(s);
    (void)hipFree(r);
    free(h);
    return 0;
}

/* rank q's contribution to element i: a small value, so the exact sum is known; it is compared
 * modulo 2^w (at 64 ranks the 8-bit sum of the plain job, 2016, wraps) */
static uint64_t int_value(int pattern, size_t i, int q) { return pattern ? (7 * i + 13 * (size_t)q) % 4 : (uint64_t)q; }

static int runint(int rd, size_t count, int calls, ftar_dtype dt, ftar_comm *comm, int wrank, int wsize, int dev)
{
    const char *pe = getenv("FTBENCH_PATTERN");
    const int pattern = pe && atoi(pe) != 0;
    const size_t es = dt == FTAR_INT8 || dt == FTAR_UINT8 ? 1 : dt == FTAR_INT16 || dt == FTAR_UINT16 ? 2 : dt == FTAR_UINT32 ? 4 : 8;
    const uint64_t mask = es == 8 ? ~0ull : (1ull << (8 * es)) - 1;
    unsigned char *h = malloc(count * es);
    if (!h) return 4;
    for (size_t i = 0; i < count; i++) {
        const uint64_t v = int_value(pattern, i, wrank); /* little-endian: the low es bytes */
        memcpy(h + i * es, &v, es);
    }
    void *s = NULL, *r = NULL;
    CHECK_HIP(hipMalloc(&s, count * es));
    CHECK_HIP(hipMalloc(&r, count * es));
    CHECK_HIP(hipMemcpy(s, h, count * es, hipMemcpyHostToDevice));
    CHECK_HIP(hipDeviceSynchronize());

    double ms[MAX_CALLS], value[MAX_CALLS], hbm[MAX_CALLS];
    int rc[MAX_CALLS], rec[MAX_CALLS], size_after[MAX_CALLS], uniform[MAX_CALLS], step0_copy = 0;
    for (int c = 0; c < calls; c++) {
        rc[c] = rd ? ftar_recursive_doubling(s, r, count, dt, FTAR_SUM, comm)
                   : ftar_allreduce_rabenseifner(s, r, count, dt, FTAR_SUM, comm);
        ftar_stats st;
        ftar_last_stats(comm, &st);
        ms[c] = st.wall_s * 1e3;
        hbm[c] = st.hbm_bytes;
        rec[c] = st.recoveries;
        size_after[c] = st.comm_size_after;
        step0_copy |= st.step0_copy;
        CHECK_HIP(hipMemcpy(h, r, count * es, hipMemcpyDeviceToHost));
        uint64_t first = 0;
        memcpy(&first, h, es);
        value[c] = (double)first;
        uniform[c] = 1;
        const int members = size_after[c]; /* the original ranks 0 .. members-1 (no fault) */
        for (size_t i = 0; i < count; i++) {
            uint64_t sum = 0, got = 0;
            for (int q = 0; q < members; q++) sum += int_value(pattern, i, q);
            memcpy(&got, h + i * es, es);
            if (got != (sum & mask)) {
                uniform[c] = 0;
                break;
            }
        }
    }
    printf("{\"rank\": %d, \"size\": %d, \"device\": %d, \"step0_copy\": %d, \"calls\": [", wrank, wsize, dev,
           step0_copy);
    for (int c = 0; c < calls; c++)
        printf("%s{\"rc\": %d, \"ms\": %.4f, \"recoveries\": %d, \"comm_size\": %d, \"value\": %.1f, \"uniform\": %s, "
               "\"hbm_bytes\": %.0f}",
               c ? ", " : "", rc[c], ms[c], rec[c], size_after[c], value[c], uniform[c] ? "true" : "false", hbm[c]);
    printf("]}\n");
    fflush(stdout);
    ftar_finalize(comm);
    (void)hipFree(s);
    (void)hipFree(r);
    free(h);
    return 0;
}
