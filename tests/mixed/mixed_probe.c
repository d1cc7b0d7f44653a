/*
 * mixed_probe.c -- TEST driver: one rank of an ftar_allreduce_multi_mixed run on the GPU.
 *
 * Launched by ftrun.  Call k reads the bytes of its list, entry after entry, each in its own
 * type, from $FTAR_PROBE_DIR/in_<rank>_<k>.bin, cuts them into one separately hipMalloc'd buffer
 * per entry, runs the call on the list and writes the results, concatenated again, to
 * out_<rank>_<k>.bin plus a status line.  Linked against libftar.so; the HIP runtime is the one
 * the library brings (looked up with dlsym).
 *
 * Entry i's buffer starts (i + FTAR_PROBE_OFFSET) % 8 elements past a 16-byte boundary, with a
 * guard on both sides; outputs start as 0xEE.  `intact` in the status line is 1 when every guard
 * of every input and output buffer is unchanged after the call and, out of place, every input as
 * well.  Empty entries pass wild pointers and a type that does not exist: they must not be looked at.
 *
 * env: FTAR_PROBE_DIR, FTAR_PROBE_ALGO=rd|raben, FTAR_MULTI_COUNTS="1,3,0,5;7,7" (one list per
 *      call), FTAR_MIXED_TYPES="17,1,16,1;16,16" (the entries' ftar_dtype, as the counts),
 *      FTAR_PROBE_INPLACE=1 (rbufs[i] == sbufs[i]), FTAR_PROBE_OFFSET=k, and one value or one per
 *      call with ';' between them: FTAR_PROBE_OP, FTAR_MIXED_SCALE (a float), FTAR_MIXED_MODE
 *      (0: the new entry point; 1: ftar_allreduce_multi and 2: ftar_allreduce_multi_acc32 on the
 *      same list, which is then of one type -- the three movers share the staging and the table
 *      mirror),
 *      FTAR_MIXED_PLAIN=1 (after each call, the plain FLOAT32 entry point on the float32 vector
 *      of in32_<rank>_<k>.bin: out_plain_<rank>_<k>.bin, its return code in the status line)
 * status: rc crank csize recoveries coalesced intact kernels plain_rc comm_size_after hbm_bytes
 */
#include <dlfcn.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ftar.h"

#define GUARD 64
#define MAXB 2048

static int (*hip_malloc)(void **, size_t);
static int (*hip_free)(void *);
static int (*hip_memcpy)(void *, const void *, size_t, int);

/* a buffer: host shadow h (guard, pad, data, guard) and its device twin d */
typedef struct {
    unsigned char *h, *d;
    size_t size, data; /* bytes in all, offset of the data */
} buf_t;

static int buf_make(buf_t *b, size_t bytes, size_t pad)
{
    b->size = (GUARD + pad + bytes + GUARD + 63) / 64 * 64;
    b->data = GUARD + pad;
    b->h = aligned_alloc(64, b->size);
    if (!b->h) return 1;
    memset(b->h, 0xA5, b->size);
    return hip_malloc((void **)&b->d, b->size) != 0;
}
static int up(buf_t *b) { return hip_memcpy(b->d, b->h, b->size, 1); }
static int down(buf_t *b, unsigned char *to) { return hip_memcpy(to, b->d, b->size, 2); }
static void buf_drop(buf_t *b)
{
    hip_free(b->d);
    free(b->h);
}

/* value k of a ';'-separated list (its last one when the list is shorter) */
static const char *nth(const char *list, int k)
{
    if (!list) return "0";
    for (; k > 0 && strchr(list, ';'); k--) list = strchr(list, ';') + 1;
    return list;
}

static int guards_ok(const unsigned char *img, const buf_t *b, size_t bytes)
{
    for (size_t i = 0; i < b->data; i++)
        if (img[i] != 0xA5) return 0;
    for (size_t i = b->data + bytes; i < b->size; i++)
        if (img[i] != 0xA5) return 0;
    return 1;
}

int main(void)
{
    const char *dir = getenv("FTAR_PROBE_DIR"), *algo = getenv("FTAR_PROBE_ALGO"), *lists = getenv("FTAR_MULTI_COUNTS");
    const char *tq = getenv("FTAR_MIXED_TYPES");
    if (!dir || !algo || !lists || !tq) return 2;
    int inplace = getenv("FTAR_PROBE_INPLACE") ? atoi(getenv("FTAR_PROBE_INPLACE")) : 0;
    size_t offset = getenv("FTAR_PROBE_OFFSET") ? strtoull(getenv("FTAR_PROBE_OFFSET"), NULL, 10) : 0;
    int plain = getenv("FTAR_MIXED_PLAIN") ? atoi(getenv("FTAR_MIXED_PLAIN")) : 0;
    ftar_algo al = !strcmp(algo, "rd") ? FTAR_ALGO_RD : FTAR_ALGO_RABENSEIFNER;

    ftar_comm *comm;
    if (ftar_init(&comm) != FTAR_SUCCESS) return 3;
    hip_malloc = (int (*)(void **, size_t))dlsym(RTLD_DEFAULT, "hipMalloc");
    hip_free = (int (*)(void *))dlsym(RTLD_DEFAULT, "hipFree");
    hip_memcpy = (int (*)(void *, const void *, size_t, int))dlsym(RTLD_DEFAULT, "hipMemcpy");
    if (!hip_malloc || !hip_free || !hip_memcpy) return 3;
    int rank;
    ftar_world_rank(comm, &rank);

    int k = 0;
    for (const char *q = lists; *q; k++) {
        static size_t counts[MAXB], es[MAXB];
        static ftar_dtype types[MAXB];
        static buf_t in[MAXB], out[MAXB];
        static const void *sb[MAXB];
        static void *rb[MAXB];
        int n = 0;
        size_t total = 0, bytes = 0;
        const int op = atoi(nth(getenv("FTAR_PROBE_OP"), k));
        const int mode = atoi(nth(getenv("FTAR_MIXED_MODE"), k));
        const float scale = getenv("FTAR_MIXED_SCALE") ? strtof(nth(getenv("FTAR_MIXED_SCALE"), k), NULL) : 1.0f;
        int dt = -1; /* modes 1 and 2: the list's one type */
        while (*q && *q != ';') {
            if (n >= MAXB) return 6;
            counts[n] = strtoull(q, (char **)&q, 10);
            types[n] = (ftar_dtype)strtol(tq, (char **)&tq, 10);
            es[n] = types[n] == FTAR_FLOAT32 ? 4 : 2;
            if (counts[n]) dt = (int)types[n];
            else types[n] = (ftar_dtype)99; /* never looked at */
            total += counts[n];
            bytes += counts[n] * es[n];
            n++;
            if (*q == ',') q++;
            if (*tq == ',') tq++;
        }
        if (*q == ';') q++;
        if (*tq == ';') tq++;
        char path[512];
        unsigned char *vec = malloc(bytes + 1), *res = malloc(bytes + 1);
        snprintf(path, sizeof(path), "%s/in_%d_%d.bin", dir, rank, k);
        FILE *f = fopen(path, "rb");
        if (!f || fread(vec, 1, bytes, f) != bytes) return 4;
        fclose(f);
        size_t off = 0;
        for (int i = 0; i < n; i++) {
            const size_t b = counts[i] * es[i], pad = ((size_t)i + offset) % 8 * es[i];
            if (!b) { /* never looked at */
                sb[i] = (const void *)(uintptr_t)(8 * (i + 1) + 1);
                rb[i] = (void *)(uintptr_t)(8 * (i + 1) + 1);
                continue;
            }
            if (buf_make(&in[i], b, pad)) return 5;
            memcpy(in[i].h + in[i].data, vec + off, b);
            if (up(&in[i])) return 5;
            sb[i] = in[i].d + in[i].data;
            if (inplace) {
                rb[i] = in[i].d + in[i].data;
            } else {
                if (buf_make(&out[i], b, pad)) return 5;
                memset(out[i].h + out[i].data, 0xEE, b);
                if (up(&out[i])) return 5;
                rb[i] = out[i].d + out[i].data;
            }
            off += b;
        }
        int rc = mode == 1   ? ftar_allreduce_multi(al, sb, rb, counts, n, (ftar_dtype)dt, (ftar_op)op, comm)
                 : mode == 2 ? ftar_allreduce_multi_acc32(al, sb, rb, counts, n, (ftar_dtype)dt, (ftar_op)op, scale, comm)
                             : ftar_allreduce_multi_mixed(al, sb, rb, counts, types, n, (ftar_op)op, scale, comm);
        ftar_stats st;
        ftar_last_stats(comm, &st);
        int crank = -1, csize = -1, intact = 1;
        ftar_comm_rank(comm, &crank);
        ftar_comm_size(comm, &csize);
        off = 0;
        for (int i = 0; i < n; i++) {
            const size_t b = counts[i] * es[i];
            if (!b) continue;
            buf_t *o = inplace ? &in[i] : &out[i];
            unsigned char *img = malloc(o->size);
            if (down(o, img)) return 5;
            intact &= guards_ok(img, o, b);
            memcpy(res + off, img + o->data, b);
            if (!inplace) { /* the input and its guards */
                unsigned char *im2 = malloc(in[i].size);
                if (down(&in[i], im2)) return 5;
                intact &= guards_ok(im2, &in[i], b) && memcmp(im2 + in[i].data, vec + off, b) == 0;
                free(im2);
            }
            free(img);
            off += b;
        }
        snprintf(path, sizeof(path), "%s/out_%d_%d.bin", dir, rank, k);
        f = fopen(path, "wb");
        fwrite(res, 1, bytes, f);
        fclose(f);
        int prc = -1;
        if (plain && total) { /* the widened vector through the plain FLOAT32 entry point */
            buf_t pi, po;
            if (buf_make(&pi, total * 4, 0) || buf_make(&po, total * 4, 0)) return 5;
            snprintf(path, sizeof(path), "%s/in32_%d_%d.bin", dir, rank, k);
            f = fopen(path, "rb");
            if (!f || fread(pi.h + pi.data, 1, total * 4, f) != total * 4) return 4;
            fclose(f);
            if (up(&pi) || up(&po)) return 5;
            prc = al == FTAR_ALGO_RD
                      ? ftar_recursive_doubling(pi.d + pi.data, po.d + po.data, total, FTAR_FLOAT32, (ftar_op)op, comm)
                      : ftar_allreduce_rabenseifner(pi.d + pi.data, po.d + po.data, total, FTAR_FLOAT32, (ftar_op)op, comm);
            unsigned char *img = malloc(po.size);
            if (down(&po, img)) return 5;
            snprintf(path, sizeof(path), "%s/out_plain_%d_%d.bin", dir, rank, k);
            f = fopen(path, "wb");
            fwrite(img + po.data, 1, total * 4, f);
            fclose(f);
            free(img);
            buf_drop(&pi);
            buf_drop(&po);
        }
        snprintf(path, sizeof(path), "%s/status_%d_%d.txt", dir, rank, k);
        f = fopen(path, "w");
        fprintf(f, "%d %d %d %d %d %d %d %d %d %.0f\n", rc, crank, csize, st.recoveries, st.coalesced, intact, st.kernels,
                prc, st.comm_size_after, st.hbm_bytes);
        fclose(f);
        for (int i = 0; i < n; i++) {
            if (!counts[i]) continue;
            buf_drop(&in[i]);
            if (!inplace) buf_drop(&out[i]);
        }
        free(vec);
        free(res);
    }
    ftar_finalize(comm);
    return 0;
}
