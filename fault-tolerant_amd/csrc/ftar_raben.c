/*
 * ftar_raben.c -- fault-tolerant Rabenseifner Allreduce on MI355X (per rank, host C).
 *
 * Restates src/raben/rabenseifner.c:3-395 and src/raben/errhandler.c:3-468 for ranks
 * that own one GPU each.  Every MPI_Sendrecv + MPI_Reduce_local pair becomes ONE
 * receiver-driven kernel that reads the partner's window straight out of its HBM
 * over xGMI (IPC peer mapping) and reduces it into the local window:
 *
 *   RS step 0 (:206-211 full exchange + :231-237 reduce):
 *       A0[rw0] = IN[rw0] + peer.IN[rw0]       (reduce half)
 *       T[sw0] = peer.IN[sw0]                  (redundancy copy, where a spare can use it:
 *                                               a replay otherwise reads peer.IN itself)
 *   RS step k>=1 (:219-237):  Ak[rwk] = A(k-1)[rwk] + peer.A(k-1)[rwk]
 *   AG step k (:299-315):     W[swk] = peer.W[swk]
 * The accumulators Ak are W, except with an idle spare, where the steps alternate W and T's
 * free half (rb_acc) so that no step overwrites its own input: a partner that dies
 * mid-exchange costs no pre-image (see the reduce-scatter loop).
 *
 * Buffers (exported workspace, ftar_internal.h): IN = this rank's vector after the
 * pre-step (the reference's sbuf after :128), W = rbuf, T = tmp_buf.  The reference's
 * tmp also stages the step>=1 windows; here those are fused into the reduce, which
 * leaves T holding the partner's vector where recovery reads it (:191-197).
 * No rank ever writes a window a peer reads in the same step, and each step ends at
 * the agree+barrier of the reference (:258-260, :330-332), so pulls need no locks.
 *
 * Deviations: sbuf is never written (IN is a private shadow); the
 * impersonator accumulates the dead rank's replay in W's half it does not own yet,
 * not in sbuf/tmp, so a second impersonation by the same rank stays correct; a
 * recovery that needs redundancy a replacement rank never received aborts instead of
 * replaying garbage; new_entry pulls only the dead rank's live window.
 *
 * This file: the entry points, the step-by-step schedule and the two error handlers.  The
 * one-hop mesh forms (power-of-two p without a spare) are in ftar_raben_mesh.c, included
 * below the handlers; the context and helpers both use are in ftar_raben.h.
 */
#include "ftar_raben.h"

#include <stdio.h>
#include <string.h>

/* host-buffer pipeline: vectors of at least HOST_PIPE_MIN bytes go through in chunks of
 * HOST_PIPE_CHUNK bytes (at most HOST_PIPE_MAX chunks, FDEV_MAX_CHUNKS) */
#define HOST_PIPE_MIN ((size_t)16 << 20)
#define HOST_PIPE_CHUNK ((size_t)8 << 20)
#define HOST_PIPE_MAX 16

static void rb_vrank(rb_ctx *x)
{
    x->rank = ftar_my_comm_rank(x->c);
    if (x->rank < 2 * x->rem) x->vrank = (x->rank % 2 == 0) ? x->rank / 2 : -1;
    else x->vrank = x->rank - x->rem;
}

/* The buffer holding every rank's reduce-scatter window after step s (uniform: the same on
 * every rank and for the whole call).  Without a spare, W: every failure aborts, and the
 * steps reduce in place.  With a spare a partner's death mid-exchange is recoverable and the
 * received window must then be discarded (corr, :238-241): the steps reduce OUT OF PLACE,
 * alternating W and T -- whose half rw0 is free, T holding the partner's other half sw0 -- so
 * the step's input window stays intact and nothing has to be restored (round 4 stored the
 * pre-image, rcount x es bytes per step: 96 MiB per 256 MiB call at p = 9).  The parity ends
 * in W at the last step, where the allgather reads the final blocks.  Every later window lies
 * in the earlier ones, and a rank only writes its own receive windows, so a partner's send
 * window at step s stays what it held after step s - 1 (the replay of rb_handler_rs reads it
 * there). */
static int rb_acc(const rb_ctx *x, int s) { return (!x->alt || (x->steps - 1 - s) % 2 == 0) ? WS_W : WS_T; }

static int rb_vrank_of(const rb_ctx *x, int cr)
{
    if (cr < 2 * x->rem) return (cr % 2 == 0) ? cr / 2 : -1;
    return cr - x->rem;
}

/* Every receiver's pull(s) at a reduce-scatter (ag = 0) or allgather (ag = 1) step:
 * what ftar_xfer needs to stripe the exchange over relays (raben/rabenseifner.c:170-249,
 * :299-315). */
static void rb_plan(const rb_ctx *x, int step, int mask, int ag, ftar_plan *P)
{
    ftar_comm *c = x->c;
    ftar_plan_clear(P);
    int64_t ri[MAXSTEPS], si[MAXSTEPS], rc[MAXSTEPS], sc[MAXSTEPS];
    for (int cr = 0; cr < c->size; cr++) {
        int v = rb_vrank_of(x, cr);
        if (v == -1) continue;
        rb_windows(v, x->count, x->steps, ri, si, rc, sc);
        int src = c->order[rb_real(x, v ^ mask)];
        ftar_pull *pl = P->pull[cr];
        memset(pl, 0, sizeof(ftar_pull) * FTAR_MAX_PULLS);
        if (ag) { /* the last allgather step lands in rbuf: only there (fast_io) or also in W */
            int last = step == 0;
            pl[0] = (ftar_pull){FDEV_COPY, 0, src, WS_W, (x->fast_io && last) ? WS_UOUT : WS_W, WS_W, si[step],
                                sc[step], !x->fast_io && last};
            P->npull[cr] = 1;
        } else if (step == 0) { /* fast_io: the local operand is sbuf itself */
            pl[0] = (ftar_pull){FDEV_REDUCE, 0, src, WS_IN, rb_acc(x, 0), x->fast_io ? WS_UIN : WS_IN, ri[0], rc[0], 0};
            pl[1] = (ftar_pull){FDEV_COPY, 0, src, WS_IN, WS_T, WS_T, si[0], sc[0], 0};
            P->npull[cr] = x->keep_recov ? 2 : 1;
        } else { /* the partner's window of the previous step, reduced into this step's accumulator */
            pl[0] = (ftar_pull){FDEV_REDUCE, 0, src, rb_acc(x, step - 1), rb_acc(x, step), rb_acc(x, step - 1), ri[step],
                                rc[step], 0};
            P->npull[cr] = 1;
        }
    }
}

static void run_reduce(rb_ctx *x, void *out, const void *xin, const void *yin, int64_t n, int remote, int tag)
{
    fdev_seg s = {FDEV_REDUCE, remote, out, xin, yin, (size_t)n, NULL};
    ftar_run(x->c, x->dtype, x->op, &s, 1, tag);
}

static void run_copy(rb_ctx *x, void *out, const void *src, int64_t n, int remote, int tag)
{
    fdev_seg s = {FDEV_COPY, remote, out, src, NULL, (size_t)n, NULL};
    ftar_run(x->c, x->dtype, x->op, &s, 1, tag);
}

/* errhandler_reduce_scatter (raben/errhandler.c:3-282) in pull form */
static void rb_handler_rs(rb_ctx *x, uint64_t newf, int fs)
{
    ftar_comm *c = x->c;
    int nf = __builtin_popcountll(newf);
    c->acked |= newf; /* MPIX_Comm_failure_ack (:20-21) */
    if (nf > 1 || fs == 0) ftar_abort(c, 1); /* :37-38 */
    int dead_w = __builtin_ctzll(newf);
    int dead = ftar_comm_rank_of(c, dead_w);
    int idle_die = (dead < x->rem * 2 && dead % 2 == 1);
    if (idle_die) { /* :50-76 */
        ftar_regroup(c, dead, x->rem * 2 - 1);
    } else {
        int vdead = (dead < x->rem * 2) ? dead / 2 : dead - x->rem; /* :80-88 */
        int org = rb_real(x, vdead ^ 1);                           /* :89-90 */
        int new_entry = x->rem * 2 - 1;                            /* :207 */
        if (new_entry == -1) ftar_abort(c, 1);                     /* :210-211 */
        int org_w = c->order[org];
        int64_t dri[MAXSTEPS], dsi[MAXSTEPS], drc[MAXSTEPS], dsc[MAXSTEPS];
        rb_windows(vdead, x->count, x->steps, dri, dsi, drc, dsc);
        if (x->rank == org) {
            if (!x->has_recov) ftar_abort(c, 1); /* deviation: a replacement holds no step-0 half */
            if (x->bg_pending) { /* the dead rank's half of its vector must be in T */
                ftar_drain_bg(c);
                x->bg_pending = 0;
            }
            /* replay the dead rank's steps 0..fs (:106-200) into W's half this rank sent at
             * step 0 (= the dead rank's reduce window, unused here until the allgather).
             * The dead rank's step-0 half: the reference's tmp copy (:191-197) where it was
             * made (FTAR_REDUNDANCY=1: T), else read where it lies -- the IN of the rank that
             * held vrank vdead at step 0 stays mapped and unwritten after its death (the
             * peers' mappings hold its memory), so the copy need not cross a link in every
             * call to make a recovery possible. */
            void *W = c->ws[WS_W], *IN = ftar_local(c, WS_IN);
            /* Failure model of the elided copy (deviation 6): the dead process's
             * memory outlives it through the peers' mappings (process death), but not a lost
             * or reset device.  The read happens only if the dead rank published that input
             * for this call and our mapping belongs to its current workspace generation;
             * otherwise there is no redundancy to replay from and the job aborts, the
             * reference's rule for an unrecoverable failure (errhandler.c:207-211). */
            const void *D0 = x->keep_recov ? (const void *)c->ws[WS_T]
                                           : ftar_dead_input(c, x->in0_w[vdead], x->count * x->es);
            if (!D0) {
                fprintf(stderr, "ftar: rank %d: the dead rank's step-0 input is not readable: no redundancy\n",
                        c->wrank);
                ftar_abort(c, 1);
            }
            run_reduce(x, at(x, W, dri[0]), at(x, IN, dri[0]), at(x, (void *)D0, dri[0]), drc[0],
                       x->keep_recov ? 0 : FDEV_REMOTE_Y, FDEV_TAG_RECOV);
            for (int s = 1; s <= fs; s++) { /* the step-s partner's send window, as it left step s - 1 */
                int pw = c->order[rb_real(x, vdead ^ (1 << s))];
                void *PW = ftar_buf(c, pw, rb_acc(x, s - 1));
                run_reduce(x, at(x, W, dri[s]), at(x, W, dri[s]), at(x, PW, dri[s]), drc[s], FDEV_REMOTE_Y,
                           FDEV_TAG_RECOV);
            }
            ftar_drain(c);
        }
        ftar_sync_fatal(c); /* the dead rank's state is ready in org's W */
        int cp = rb_real(x, vdead ^ (1 << fs));
        void *OW = ftar_buf(c, org_w, WS_W);
        if (x->rank == cp && x->corr) { /* :170-180: reduce the window the dead rank owed us */
            /* this rank's step-fs window from its (intact) step fs - 1 input: a pull that was
             * skipped, cut short or made from a dying rank's memory is simply not used */
            run_reduce(x, at(x, ftar_local(c, rb_acc(x, fs)), x->rindex[fs]),
                       at(x, ftar_local(c, rb_acc(x, fs - 1)), x->rindex[fs]), at(x, OW, x->rindex[fs]),
                       x->rcount[fs], FDEV_REMOTE_Y, FDEV_TAG_RECOV);
        }
        if (x->rank == new_entry) { /* :213-241: take over the dead rank's role */
            memcpy(x->rindex, dri, sizeof(dri));
            memcpy(x->sindex, dsi, sizeof(dsi));
            memcpy(x->rcount, drc, sizeof(drc));
            memcpy(x->scount, dsc, sizeof(dsc));
            /* the dead rank's whole reduce-scatter state, not only its current window: a
             * later replay (a second failure) pulls this rank's sindex[s] windows of the
             * steps s <= fs, which all lie in the step-0 window (the reference ships the
             * whole buffer, :213-241).  Each part goes where the dead rank held it: the part
             * of window s it sent at step s + 1 in step s's accumulator, the live window
             * fs in step fs's (one launch) */
            fdev_seg seg[MAXSTEPS + 1];
            int nseg = 0;
            for (int s = 0; s <= fs; s++) {
                int64_t off = s < fs ? dsi[s + 1] : dri[fs], n = s < fs ? dsc[s + 1] : drc[fs];
                if (n <= 0) continue;
                seg[nseg++] = (fdev_seg){FDEV_COPY, FDEV_REMOTE_X, at(x, ftar_local(c, rb_acc(x, s)), off),
                                         at(x, OW, off), NULL, (size_t)n, NULL};
            }
            if (nseg) ftar_run(c, x->dtype, x->op, seg, nseg, FDEV_TAG_RECOV);
            x->has_recov = 0;
        }
        ftar_drain(c);
        ftar_sync_fatal(c);
        ftar_regroup(c, dead, new_entry); /* :243-281 */
    }
    x->rem--; /* rabenseifner.c:268-283 */
    rb_vrank(x);
    x->corr = 0;
    c->stats.recoveries++;
}

/* errhandler_allgather (raben/errhandler.c:284-468) in pull form */
static void rb_handler_ag(rb_ctx *x, uint64_t newf, int fs)
{
    ftar_comm *c = x->c;
    int nf = __builtin_popcountll(newf);
    c->acked |= newf; /* MPIX_Comm_failure_ack (:300-301) */
    if (nf > 1 || fs == x->steps - 1) ftar_abort(c, 1); /* :320-323 */
    int dead_w = __builtin_ctzll(newf);
    int dead = ftar_comm_rank_of(c, dead_w);
    int idle_die = (dead < x->rem * 2 && dead % 2 == 1);
    if (idle_die) {
        ftar_regroup(c, dead, x->rem * 2 - 1);
    } else {
        int vdead = (dead < x->rem * 2) ? dead / 2 : dead - x->rem;
        int org = rb_real(x, vdead ^ (x->adjsize >> 1)); /* :372-373 */
        int new_entry = x->rem * 2 - 1;
        if (new_entry == -1) ftar_abort(c, 1); /* :377-378 */
        if (x->rank == new_entry) {
            /* :381-398: the original partner's buffer and index arrays (equal to the dead
             * rank's for every remaining step).  Only the part held after the allgather
             * step fs is live: the reduce-scatter window of step fs-1, or all of it. */
            rb_windows(vdead, x->count, x->steps, x->rindex, x->sindex, x->rcount, x->scount);
            int64_t off = 0, n = (int64_t)x->count;
            if (fs >= 1) {
                off = x->rindex[fs - 1];
                n = x->rcount[fs - 1];
            }
            void *OW = ftar_buf(c, c->order[org], WS_W);
            run_copy(x, at(x, c->ws[WS_W], off), at(x, OW, off), n, FDEV_REMOTE_X, FDEV_TAG_RECOV);
            x->has_recov = 0;
            ftar_drain(c);
        }
        ftar_sync_fatal(c);
        int lp = rb_real(x, vdead ^ (1 << fs)); /* :400-414 */
        if (x->rank == lp) {
            void *NW = ftar_buf(c, c->order[new_entry], WS_W);
            run_copy(x, at(x, c->ws[WS_W], x->sindex[fs]), at(x, NW, x->sindex[fs]), x->scount[fs], FDEV_REMOTE_X,
                     FDEV_TAG_RECOV);
            ftar_drain(c);
        }
        ftar_sync_fatal(c);
        ftar_regroup(c, dead, new_entry);
    }
    x->rem--;
    rb_vrank(x);
    c->stats.recoveries++;
}

/* the mesh forms: rb_push_slot, rb_oneshot_prelaunch, rb_oneshot, rb_mesh */
#include "ftar_raben_mesh.c"

/* The call's context: its arguments checked (the reference's errors) and the form it takes,
 * decided from the comm's options, p and the size alone, so the same on every rank.  Decides
 * only -- nothing is launched, staged or published here. */
static int rb_select_form(rb_ctx *x, const void *sbuf, void *rbuf, size_t count, ftar_dtype dtype, ftar_op op,
                          ftar_comm *c)
{
    memset(x, 0, sizeof(*x));
    x->c = c;
    x->dtype = (int)dtype;
    x->op = (int)op;
    x->es = ftar_esize(dtype);
    x->count = count;
    int orc = ftar_check_op((int)dtype, (int)op);
    if (orc) return orc;
    x->steps = ftar_hibit(c->size, (int)(sizeof(int) * 8) - 1); /* :16-21 */
    if (x->steps == -1) return FTAR_ERR_ARG;
    if (count == 0) return FTAR_ERR_UNKNOWN; /* copy_buffer(count <= 0), util.c:40-43 */
    if (count > (size_t)INT64_MAX / 16 || !sbuf || !rbuf) return FTAR_ERR_ARG;
    /* device pointers: pageable host memory or a short allocation is refused, not faulted on */
    if (fdev_check_ptr(c->dev, sbuf, count * x->es) || fdev_check_ptr(c->dev, rbuf, count * x->es))
        return FTAR_ERR_ARG;
    x->adjsize = 1 << x->steps;
    x->rem = c->size - x->adjsize;
    x->alt = x->rem > 0; /* uniform; fixed for the call (rem only decreases) */
    /* The step-0 copy of the partner's other half (tmp, :191-197) is only ever read by
     * an RS error handler's replay, and every handler aborts before replaying when
     * there is no idle spare (new_entry = 2 rem - 1 = -1, errhandler.c:207-211,377-378).
     * rem only decreases during a call, so with rem = 0 at the start the copy can never
     * be consumed: skip it (FTAR_REDUNDANCY=1 keeps it, the reference's shape).
     * With a spare, the copy is what lets the replay survive the loss of the dead rank's
     * memory (the reference copies at step 0 precisely because that memory is gone,
     * :206-211).  A peer's mapping keeps a killed process's memory readable on one device
     * (tested), but across GPUs that premise is unverified, so by default (auto, 2) the
     * copy moves whenever the comm spans more than one GPU; FTAR_REDUNDANCY=0 elides it on
     * any layout (the replay then reads the dead rank's input in place, deviation 6).
     * Uniform: the members' devices are the same on every rank. */
    x->keep_recov = c->redundancy == 1 || (c->redundancy == 2 && x->rem > 0 && ftar_spans_devices(c));
    /* The reference's recovery data: every rank holds its step-0 partner's other half (in
     * tmp) while a spare can use it, except a replacement rank (errhandler.c:213-241 ships
     * it the dead rank's state, not its redundancy: a replay by it aborts, as the oracle's
     * restatement does).  Without the physical copy (keep_recov = 0) the replay reads that
     * half where it lies: the IN of the rank that held the vrank at step 0. */
    x->has_recov = x->keep_recov || x->rem > 0;
    /* Without an idle rank every failure aborts (new_entry = -1, errhandler.c:207-211,
     * 377-378), so nothing outside the schedule has to stay recoverable: step 0 reads
     * this rank's reduce half straight from sbuf (only the half peers pull is staged in
     * IN), the last allgather step writes rbuf directly and copies this rank's own final
     * half out of W in the same launch, and the prologue's three barriers (no pre-step
     * exchange at rem = 0) collapse into one.  Same operands, same bits. */
    x->fast_io = !x->keep_recov && x->rem == 0 && x->steps >= 1;
    x->mesh = x->fast_io && c->mesh && c->size <= FDEV_MAX_TREE;
    /* Uniform: count, p and the options are the same on every rank.  At p = 2 the
     * one-shot form moves the same link bytes as the two-launch mesh (S per direction)
     * in one launch, so it runs at every size; at p > 2 it reads (p - 2) S / p more per
     * link and pays off only below oneshot_max. */
    x->oneshot = x->mesh && c->size <= FDEV_MAX_BATCH && c->oneshot_max > 0 &&
                 (c->size == 2 || count * (size_t)x->es <= c->oneshot_max);
    /* push 2 (both phases) needs every peer as an extra destination of one tree: p <= 8 */
    x->push = (x->mesh && !x->oneshot && c->push) ? (c->push == 2 && c->size <= 8 ? 2 : 1) : 0;
    /* uniform too; every block non-empty (count >= p: the allgather launch always exists); not
     * with FTAR_OPT_FLAG_SYNC off, the conservative mode of fenced-marker drains only (whose
     * pinned flag words the wait also uses) */
    x->devwait = x->mesh && !x->oneshot && !x->push && c->mesh_wait && count >= (size_t)c->size &&
                 c->size - 1 <= FDEV_MAX_PEERS && fdev_get_knob(c->dev, FDEV_KNOB_FLAG_SYNC) == 1 && ftar_flag(c, c->wrank);
    return FTAR_SUCCESS;
}

/* Input staging, up to the drain before the call's first barrier: what the peers read of this
 * rank's input is its sbuf in place or a copy in IN.  Returns this rank's IN. */
static void *rb_stage(rb_ctx *x, const void *sbuf, void *rbuf)
{
    ftar_comm *c = x->c;
    const size_t count = x->count, bytes = count * x->es;
    void *IN = c->ws[WS_IN];
    /* Where nothing writes this rank's IN -- every rank but the pre-step pairs; the
     * handlers only read it -- the peers read sbuf in place; otherwise, or when its
     * memory cannot be shared, it is staged in IN.  With a spare, the partner's step-0
     * redundancy copy may still be reading sbuf while the last allgather step writes
     * rbuf, so there sbuf and rbuf must not overlap. */
    const char *s0 = (const char *)sbuf, *d0 = (const char *)rbuf;
    int disjoint = s0 + bytes <= d0 || d0 + bytes <= s0;
    /* partly overlapping sbuf / rbuf (neither the same buffer nor disjoint): rbuf is written
     * only after every peer is done reading sbuf */
    x->io_safe = disjoint || s0 == d0;
    /* The one-shot launch writes rbuf while peers still read this rank's input: in place,
     * that input must be staged (whole: peers read every block of it). */
    /* push: no peer ever reads this rank's input (it stores its parts into the owners) */
    int aliased = x->push ? 0 :
                  ftar_stage_input(c, sbuf, bytes,
                                   x->oneshot ? disjoint : (x->fast_io || (x->rank >= 2 * x->rem && disjoint)));
    if (x->push) {
        ftar_inputs_done(c);
    } else if (aliased) {
        IN = (void *)sbuf;
    } else if (x->oneshot) {
        /* small inputs are staged by every rank (ftar_stage_input): the launch's operands
         * are known before the barrier, and the staging copy can ride in it */
        if (bytes <= c->stage_max) {
            rb_oneshot_prelaunch(x, sbuf, rbuf, IN);
            if (x->gated) ftar_note_launch(c, NULL, 0); /* the staging phase is in flight */
        }
        if (!x->gated) {
            run_copy(x, IN, sbuf, (int64_t)count, 0, FDEV_TAG_LOCAL);
            if (bytes <= c->stage_max) rb_oneshot_prelaunch(x, sbuf, rbuf, NULL);
        }
    } else if (x->mesh) { /* peers pull every block of sbuf but this rank's own final one */
        int64_t b0 = x->rindex[x->steps - 1], b1 = b0 + x->rcount[x->steps - 1];
        fdev_seg cp[2] = {{FDEV_COPY, 0, IN, sbuf, NULL, (size_t)b0, NULL},
                          {FDEV_COPY, 0, at(x, IN, b1), at(x, (void *)sbuf, b1), NULL, (size_t)((int64_t)count - b1),
                           NULL}};
        ftar_run(c, x->dtype, x->op, cp, 2, FDEV_TAG_LOCAL);
    } else if (x->fast_io) { /* the half of sbuf peers pull at step 0 */
        run_copy(x, at(x, IN, x->sindex[0]), at(x, (void *)sbuf, x->sindex[0]), x->scount[0], 0, FDEV_TAG_LOCAL);
    } else {
        run_copy(x, IN, sbuf, (int64_t)count, 0, FDEV_TAG_LOCAL); /* rbuf = sbuf, :35-42 */
    }
    ftar_drain(c);
    return IN;
}

/* ---- pre-step (:61-139): failures are fatal here ---- */
static void rb_pre_step(rb_ctx *x, void *IN)
{
    ftar_comm *c = x->c;
    const size_t count = x->count;
    ftar_maybe_die(c, FTAR_PH_PRE, 0, FTAR_PT_BEFORE);
    if (x->fast_io) {
        ftar_enter(c);
        ftar_launched(c, FTAR_PH_PRE, 0);
        ftar_exchange_done(c);
        ftar_maybe_die(c, FTAR_PH_PRE, 0, FTAR_PT_AFTER);
        ftar_maybe_die(c, FTAR_PH_PRE, 0, FTAR_PT_BARRIER);
        ftar_sync_fatal(c); /* every IN is ready; the barrier before the tolerant region (:166) */
        ftar_resolve_inputs(c);
    } else {
        ftar_sync_fatal(c); /* every IN is ready */
        ftar_resolve_inputs(c);
        ftar_enter(c);
        int64_t lh = (int64_t)count / 2, rh = (int64_t)count - lh;
        int pair = x->rank < 2 * x->rem;
        if (pair) {
            if (x->rank % 2 != 0) { /* odd: reduce the right half with the even's right half */
                void *P = ftar_buf(c, c->order[x->rank - 1], WS_IN);
                run_reduce(x, at(x, IN, lh), at(x, IN, lh), at(x, P, lh), rh, FDEV_REMOTE_Y, FDEV_TAG_STEP);
            } else { /* even: reduce the left half with the odd's left half */
                void *P = ftar_buf(c, c->order[x->rank + 1], WS_IN);
                run_reduce(x, IN, IN, P, lh, FDEV_REMOTE_Y, FDEV_TAG_STEP);
            }
        }
        ftar_launched(c, FTAR_PH_PRE, 0);
        if (pair) {
            ftar_drain(c);
            c->stats.steps++;
        }
        ftar_exchange_done(c);
        ftar_maybe_die(c, FTAR_PH_PRE, 0, FTAR_PT_AFTER);
        ftar_maybe_die(c, FTAR_PH_PRE, 0, FTAR_PT_BARRIER);
        ftar_sync_fatal(c);
        if (x->rank < 2 * x->rem && x->rank % 2 == 0) { /* even: receive the reduced right half (:120) */
            void *P = ftar_buf(c, c->order[x->rank + 1], WS_IN);
            run_copy(x, at(x, IN, lh), at(x, P, lh), rh, FDEV_REMOTE_X, FDEV_TAG_STEP);
            ftar_drain(c);
        }
        ftar_sync_fatal(c); /* MPI_Barrier before the tolerant region (:166) */
    }
}

/* ---- reduce-scatter (:170-284) ---- */
static void rb_reduce_scatter(rb_ctx *x)
{
    ftar_comm *c = x->c;
    void *T = c->ws[WS_T];
    for (int v = 0; v < x->adjsize; v++) x->in0_w[v] = c->order[rb_real(x, v)];
    int step = 0;
    for (int mask = 1; mask < x->adjsize; mask <<= 1, step++) {
        ftar_plan P;
        ftar_xstate xs;
        memset(&xs, 0, sizeof(xs));
        rb_plan(x, step, mask, 0, &P);
        ftar_maybe_die(c, FTAR_PH_LOOP, step, FTAR_PT_BEFORE);
        ftar_enter(c);
        int skip = 0, pw = -1;
        if (x->vrank != -1) {
            pw = c->order[rb_real(x, x->vrank ^ mask)];
            if (!ftar_peer_entered(c, pw)) skip = x->corr = 1; /* the exchange failed (:238-241) */
            c->stats.steps++;
        }
        /* A partner that dies mid-exchange (after entering, before its side completed) fails
         * the Sendrecv too: the reference then discards the received window (corr, :238-241)
         * and the RS handler rebuilds it from the impersonator's replay.  With a spare the
         * step reduced out of place (rb_acc): its input window is intact, so discarding is
         * just not using the result -- the handler's corr reduce recomputes the window from
         * the step's input and the replayed state.  (At step 0 the handler aborts.)  If a
         * relay died the window may be partly unreduced, but then a second rank died with
         * the partner and the handler aborts (nf > 1, errhandler.c:37-38). */
        int guard = x->rem > 0 && step >= 1 && pw >= 0 && !skip;
        double lb0 = ftar_link_bytes(c);
        int tag = step == 0 ? FDEV_TAG_STEP0 : FDEV_TAG_STEP;
        if (step == 0 && c->overlap && !ftar_xfer_would_relay(c, &P, x->es)) {
            /* :206-211 full exchange + :231-237 reduce, direct.  The reduce half is on the
             * critical path; the redundancy half (kept in T for recovery, :191-197) is only
             * needed by a later error handler, so it runs on the background stream and
             * overlaps steps 1.. (joined before any replay and before the final barrier).
             * (With relays both halves are striped in the step itself.) */
            if (x->vrank != -1 && !skip) {
                const ftar_pull *pl = P.pull[x->rank];
                void *PIN = ftar_buf(c, pl[0].src, WS_IN);
                fdev_seg red = {FDEV_REDUCE, FDEV_REMOTE_Y, at(x, ftar_local(c, pl[0].dst_buf), pl[0].off),
                                at(x, ftar_local(c, pl[0].x_buf), pl[0].off), at(x, PIN, pl[0].off), (size_t)pl[0].n,
                                NULL};
                fdev_seg cpy = {FDEV_COPY, FDEV_REMOTE_X, at(x, T, pl[1].off), at(x, PIN, pl[1].off), NULL,
                                (size_t)pl[1].n, NULL};
                ftar_run_pulls(c, x->dtype, x->op, &red, 1, FDEV_TAG_STEP0, 0);
                if (x->keep_recov) {
                    ftar_run_pulls(c, x->dtype, x->op, &cpy, 1, FDEV_TAG_BG, 1);
                    x->bg_pending = 1;
                }
            }
            ftar_launched(c, FTAR_PH_LOOP, step);
            if (x->vrank != -1 && !skip) ftar_drain(c);
            ftar_exchange_done(c);
            ftar_maybe_die(c, FTAR_PH_LOOP, step, FTAR_PT_AFTER);
        } else {
            ftar_xfer_step(c, &P, x->dtype, x->op, tag, skip, FTAR_PH_LOOP, step, NULL, 0, &xs);
        }
        if (guard && !ftar_peer_done(c, pw)) { /* partner died mid-exchange: corr */
            x->corr = 1;
            xs.skipped = 1; /* nothing of this window is re-pulled after the agree */
            if (c->verbose)
                fprintf(stderr, "ftar: rank %d: partner %d died mid-exchange at RS step %d: window discarded\n",
                        c->wrank, pw, step);
        }
        if (step == 0) c->stats.step0_link_bytes += ftar_link_bytes(c) - lb0;
        ftar_maybe_die(c, FTAR_PH_LOOP, step, FTAR_PT_BARRIER);
        uint64_t newf = ftar_step_sync(c, 2 * x->steps); /* agree + barrier (:258-265) */
        if (newf) {
            ftar_xfer_repair(c, &P, x->dtype, x->op, &xs, newf);
            rb_handler_rs(x, newf, step);
        }
    }
}

/* ---- allgather (:299-355) ---- */
static void rb_allgather(rb_ctx *x, void *rbuf)
{
    ftar_comm *c = x->c;
    void *W = c->ws[WS_W];
    int step = x->steps - 1;
    for (int mask = x->adjsize >> 1; mask > 0; mask >>= 1, step--) {
        ftar_plan P;
        ftar_xstate xs;
        rb_plan(x, step, mask, 1, &P);
        ftar_maybe_die(c, FTAR_PH_AG, step, FTAR_PT_BEFORE);
        ftar_enter(c);
        int skip = 0;
        if (x->vrank != -1) {
            skip = !ftar_peer_entered(c, c->order[rb_real(x, x->vrank ^ mask)]);
            c->stats.steps++;
        }
        /* last step: this rank's own final half W -> rbuf rides in the same launch */
        fdev_seg own = {FDEV_COPY, 0, NULL, NULL, NULL, 0, NULL};
        int nown = 0;
        if (step == 0 && x->vrank != -1) {
            own.out = at(x, rbuf, x->rindex[0]);
            own.x = at(x, W, x->rindex[0]);
            own.n = (size_t)x->rcount[0];
            nown = 1;
        }
        ftar_xfer_step(c, &P, x->dtype, x->op, FDEV_TAG_STEP, skip, FTAR_PH_AG, step, &own, nown, &xs);
        ftar_maybe_die(c, FTAR_PH_AG, step, FTAR_PT_BARRIER);
        uint64_t newf = ftar_step_sync(c, 2 * x->steps); /* (:330-335) */
        x->out_done = nown && !skip && !newf; /* a recovery here re-homes windows: copy W at the end */
        if (newf) {
            ftar_xfer_repair(c, &P, x->dtype, x->op, &xs, newf);
            rb_handler_ag(x, newf, step);
        }
    }
}

/* ---- ERRORS_ARE_FATAL barrier + post-step (:357-381) ---- */
static int rb_epilogue(rb_ctx *x, void *IN, void *rbuf)
{
    ftar_comm *c = x->c;
    const size_t count = x->count;
    void *W = c->ws[WS_W];
    if (x->bg_pending) { /* peers read our IN until their copies are done: join before the barrier */
        ftar_drain_bg(c);
        x->bg_pending = 0;
    }
    ftar_pass_post(c);
    ftar_sync_fatal(c);
    if (x->fast_io) { /* rbuf is complete; no idle rank reads W, every peer is done with it */
        ftar_stats_end(c);
        return FTAR_SUCCESS;
    }
    if (x->rank < 2 * x->rem && x->rank % 2 != 0) {
        void *P = ftar_buf(c, c->order[x->rank - 1], WS_W); /* odd: result from rank-1 */
        run_copy(x, rbuf, P, (int64_t)count, FDEV_REMOTE_X, FDEV_TAG_STEP);
        c->stats.steps++;
    } else if (!x->out_done) { /* with one rank there is no exchange and rbuf = sbuf (:35-42) */
        run_copy(x, rbuf, x->steps == 0 ? IN : W, (int64_t)count, 0, FDEV_TAG_LOCAL);
    }
    ftar_drain(c);
    ftar_sync_fatal(c); /* peers are done reading our W before it is reused */
    ftar_stats_end(c);
    return FTAR_SUCCESS;
}

int ftar_allreduce_rabenseifner(const void *sbuf, void *rbuf, size_t count, ftar_dtype dtype, ftar_op op,
                                ftar_comm *c)
{
    if (!c) return FTAR_ERR_ARG;
    rb_ctx X;
    rb_ctx *x = &X;
    int rc = rb_select_form(x, sbuf, rbuf, count, dtype, op, c);
    if (rc) return rc;
    c->uin = sbuf;
    c->uout = rbuf;
    ftar_stats_begin(c);
    c->stats.step0_copy = x->keep_recov && c->size > 1;
    if (c->size == 1) return ftar_single_rank(c, sbuf, rbuf, count * x->es);

    ftar_ensure_workspace(c, count * x->es);
    if (x->push) { /* uniform: the same geometry on every rank */
        x->slot = rb_push_slot(x);
        x->push = x->slot > 0;
    }
    fdev_order_after(c->dev, c->user_stream); /* sbuf may still be in flight on the caller's stream */
    rb_vrank(x);
    /* this rank's windows of every step: a function of vrank, count and steps alone (an idle
     * odd rank of a pre-step pair, vrank -1, has none until a handler gives it a role) */
    if (x->vrank != -1) rb_windows(x->vrank, count, x->steps, x->rindex, x->sindex, x->rcount, x->scount);
    void *IN = rb_stage(x, sbuf, rbuf);
    rb_pre_step(x, IN);
    if (x->oneshot) return rb_oneshot(x, sbuf, rbuf);
    if (x->mesh) return rb_mesh(x, sbuf, rbuf);
    rb_reduce_scatter(x);
    rb_allgather(x, rbuf);
    return rb_epilogue(x, IN, rbuf);
}

int ftar_allreduce_rabenseifner_host(const void *sbuf, void *rbuf, size_t count, ftar_dtype dtype, ftar_op op,
                                     ftar_comm *c)
{
    if (!c) return FTAR_ERR_ARG;
    int orc = ftar_check_op((int)dtype, (int)op); /* before anything is copied */
    if (orc) return orc;
    size_t es = ftar_esize(dtype);
    size_t bytes = count * es;
    /* Power of two without a spare (every failure aborts, so nothing is recovered across
     * calls): the vector goes through as a pipeline of chunk Allreduces -- chunk k's
     * H2D, chunk k-1's Allreduce and chunk k-2's D2H in flight at once (copy engines both
     * ways, xGMI) -- instead of H2D, Allreduce, D2H in turn.  Each chunk is a complete
     * fault-tolerant call (barriers, agree, abort).
     * Chunks move the block boundaries, and an element's tree takes its operands in its
     * owner's order (src[j] = x_(owner ^ j)): the unordered tree is the same for every
     * owner, so the bits are too wherever the op commutes exactly -- integers, float
     * SUM/PROD -- but not float MAX/MIN (NaN, signed zeros), which stay one call. */
    int p = c->size;
    int nchunk = 1;
    int commutes = dtype == FTAR_INT32 || dtype == FTAR_INT64 || (dtype >= FTAR_INT8 && dtype <= FTAR_UINT64) ||
                   op == FTAR_SUM || op == FTAR_PROD; /* every integer type, every op it has */
    if (c->host_pipe && commutes && c->redundancy != 1 && c->loop_seconds <= 0 && p >= 2 && (p & (p - 1)) == 0 &&
        bytes >= HOST_PIPE_MIN) {
        nchunk = (int)(bytes / HOST_PIPE_CHUNK);
        if (nchunk > HOST_PIPE_MAX) nchunk = HOST_PIPE_MAX;
    }
    /* Not pipelined and the caller's buffers pinned: the device entry point reads sbuf and
     * writes rbuf in place over PCIe, no staging copies */
    if (nchunk <= 1 && fdev_host_pinned(sbuf) && fdev_host_pinned(rbuf))
        return ftar_allreduce_rabenseifner(sbuf, rbuf, count, dtype, op, c);
    ftar_ensure_staging(c, bytes);
    if (nchunk <= 1) {
        if (bytes && fdev_h2d(c->dev, c->hsend, sbuf, bytes)) ftar_host_copy_failed(c, "H2D copy");
        int rc = ftar_allreduce_rabenseifner(c->hsend, c->hrecv, count, dtype, op, c);
        if (rc) return rc;
        if (bytes && fdev_d2h(c->dev, rbuf, c->hrecv, bytes)) ftar_host_copy_failed(c, "D2H copy");
        return FTAR_SUCCESS;
    }
    size_t per = (count + (size_t)nchunk - 1) / (size_t)nchunk;
    per = (per + 63) / 64 * 64; /* chunk boundaries on multiples of 64 elements: 256 bytes at 4, 64 at 1 (16-byte multiples at every size) */
    int n = 0;
    for (size_t off = 0; off < count; off += per, n++) {
        size_t m = count - off < per ? count - off : per;
        if (fdev_h2d_async(c->dev, (char *)c->hsend + off * es, (const char *)sbuf + off * es, m * es, n))
            ftar_host_copy_failed(c, "H2D copy");
    }
    n = 0;
    for (size_t off = 0; off < count; off += per, n++) {
        size_t m = count - off < per ? count - off : per;
        if (fdev_wait_h2d(c->dev, n, ftar_ctrl_poll, &c->job)) ftar_host_copy_failed(c, "H2D copy");
        c->chunk_cont = n > 0;
        int rc = ftar_allreduce_rabenseifner((char *)c->hsend + off * es, (char *)c->hrecv + off * es, m, dtype, op,
                                             c);
        c->chunk_cont = 0;
        if (rc) return rc;
        if (fdev_d2h_async(c->dev, (char *)rbuf + off * es, (char *)c->hrecv + off * es, m * es))
            ftar_host_copy_failed(c, "D2H copy");
    }
    if (fdev_sync_d2h(c->dev, ftar_ctrl_poll, &c->job)) ftar_host_copy_failed(c, "D2H copy");
    return FTAR_SUCCESS;
}
