/*
 * ftar_raben.h -- what ftar_raben.c and ftar_raben_mesh.c share (private): the call's context,
 * the window rule and the mesh forms' phase helpers.
 */
#ifndef FTAR_RABEN_H
#define FTAR_RABEN_H

#include "ftar_internal.h"

#define MAXSTEPS 32

typedef struct {
    ftar_comm *c;
    int dtype, op;
    size_t es, count;
    int steps, adjsize, rem;
    int rank, vrank, corr, has_recov;
    int keep_recov; /* step 0 also pulls the partner's other half into T (recovery data) */
    int alt;        /* RS accumulators alternate W / T (an idle spare at the call's start; rb_acc) */
    int bg_pending; /* step-0 redundancy copy still running on the background stream */
    int fast_io;    /* power of two, no recovery data: sbuf/rbuf used in place (see below) */
    int out_done;   /* the last allgather step already stored this rank's result in rbuf */
    int mesh;       /* fast_io on the full mesh: one-hop reduce-scatter and allgather */
    int push;       /* the mesh's reduce-scatter by remote stores into the owners' R (FTAR_OPT_PUSH) */
    int64_t slot;   /* push: elements per source slot in an owner's R */
    int oneshot;    /* mesh of a small vector: every block in its owner's tree, one launch */
    int own_in_rbuf; /* the mesh's tree stored this rank's final block in rbuf too: the allgather skips it */
    int io_safe;     /* sbuf == rbuf or the two do not overlap: rbuf may be written while peers read sbuf */
    int devwait;     /* the mesh's allgather ordered behind the peers' trees on the device (rb_mesh_devwait) */
    /* the one-shot launch queued ahead of the barrier (rb_oneshot_prelaunch): its plan, to
     * be checked against the one the inputs' resolution gives */
    int gated;
    struct rb_batch {
        const void *src[FDEV_MAX_BATCH * FDEV_MAX_BATCH];
        void *out[FDEV_MAX_BATCH];
        size_t n[FDEV_MAX_BATCH];
        unsigned remote[FDEV_MAX_BATCH];
    } gplan;
    int in0_w[FTAR_MAX_RANKS]; /* world rank whose IN held vrank v's input at RS step 0 */
    int64_t rindex[MAXSTEPS], sindex[MAXSTEPS], rcount[MAXSTEPS], scount[MAXSTEPS];
} rb_ctx;

static inline int rb_real(const rb_ctx *x, int v) { return (v < x->rem) ? v * 2 : v + x->rem; }

static inline void *at(const rb_ctx *x, void *base, int64_t idx) { return (char *)base + (size_t)idx * x->es; }

/* Windows of virtual rank v at every step (raben/rabenseifner.c:170-249).  The
 * reference compares real ranks (rank < dest); the vrank->rank map is monotone, so
 * that is bit s of v being 0. */
static inline void rb_windows(int v, size_t count, int steps, int64_t *rindex, int64_t *sindex, int64_t *rcount,
                              int64_t *scount)
{
    int64_t wsize = (int64_t)count;
    rindex[0] = sindex[0] = 0;
    for (int s = 0; s < steps; s++) {
        int lower = !((v >> s) & 1);
        if (lower) {
            rcount[s] = wsize / 2;
            scount[s] = wsize - rcount[s];
            sindex[s] = rindex[s] + rcount[s];
        } else {
            scount[s] = wsize / 2;
            rcount[s] = wsize - scount[s];
            rindex[s] = sindex[s] + scount[s];
        }
        if (s + 1 < steps) {
            rindex[s + 1] = rindex[s];
            sindex[s + 1] = rindex[s];
            wsize = rcount[s];
        }
    }
}

/* Vrank u's final block, rb_windows(u)'s rindex / rcount [steps - 1], by the same halving:
 * the lower rank of a step keeps the window's first wsize / 2 elements, the upper one the
 * rest (empty blocks where count < p). */
static inline void rb_block(const rb_ctx *x, int u, int64_t *off, int64_t *n)
{
    int64_t lo = 0, wsize = (int64_t)x->count;
    for (int s = 0; s < x->steps; s++) {
        if ((u >> s) & 1) lo += wsize / 2, wsize -= wsize / 2;
        else wsize /= 2;
    }
    *off = lo;
    *n = wsize;
}

/* Phase helpers: a form that runs a whole phase as one launch still passes every step's kill
 * points, in the phase's own order: FTAR_PH_LOOP steps 0 .. L-1, FTAR_PH_AG steps L-1 .. 0,
 * FTAR_PH_POST step 0 only.  rb_pass: every step of `phase` passes `point` (from its
 * `first`-th step on). */
static inline void rb_pass_from(const rb_ctx *x, int phase, int point, int first)
{
    const int n = phase == FTAR_PH_POST ? 1 : x->steps;
    for (int i = first; i < n; i++) ftar_maybe_die(x->c, phase, phase == FTAR_PH_AG ? n - 1 - i : i, point);
}
static inline void rb_pass(const rb_ctx *x, int phase, int point) { rb_pass_from(x, phase, point, 0); }

/* the phase's one launch is in flight: every step's DURING point */
static inline void rb_launched(const rb_ctx *x, int phase)
{
    ftar_launched(x->c, phase, phase == FTAR_PH_AG ? x->steps - 1 : 0);
    rb_pass_from(x, phase, FTAR_PT_DURING, 1);
}

/* The phase's launch has drained: one mesh exchange, standing for `steps` steps of the
 * reference, is complete; then the AFTER and BARRIER points.  The agree is the caller's. */
static inline void rb_close(const rb_ctx *x, int phase, int steps)
{
    ftar_exchange_done(x->c);
    x->c->stats.steps += steps;
    x->c->stats.mesh_steps++;
    rb_pass(x, phase, FTAR_PT_AFTER);
    rb_pass(x, phase, FTAR_PT_BARRIER);
}

#endif
