/*
 * ftar_raben_mesh.c -- the one-hop "mesh" forms of the Rabenseifner Allreduce (power-of-two p
 * without an idle rank): rb_mesh lists them, rb_oneshot is the one-launch form.  Each is a short
 * list of launches, drains and agree rounds between the phases' kill-point walks (ftar_raben.h).
 *
 * Part of ftar_raben.c's translation unit (included there): the forms, the handlers and the
 * schedule stay static to each other, and a build lists ftar_raben.c alone.  What this file
 * takes from it is declared here; what it gives is rb_push_slot, rb_oneshot_prelaunch,
 * rb_oneshot and rb_mesh.
 */
#include "ftar_raben.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

/* errhandler_reduce_scatter / errhandler_allgather after step fs's agree reported newf (ftar_raben.c) */
static void rb_handler_rs(rb_ctx *x, uint64_t newf, int fs);
static void rb_handler_ag(rb_ctx *x, uint64_t newf, int fs);

/* Push form of the mesh (FTAR_OPT_PUSH): where the pull form's tree kernel reads the p - 1
 * peers' parts of this rank's block over xGMI, here every rank stores its part of each
 * peer's block INTO that peer (the owner's R, one slot per source) and each owner reduces
 * its block from local memory.  Link bytes are the same (S/p per link and direction); the
 * fabric moves remote stores instead of remote loads, which bench.py compares on the node.
 * Slot j of owner u holds x_(u^j) over u's final block -- the tree's src[j] -- starting at
 * the same element offset modulo 16 bytes as the block itself, so the copies and the tree
 * keep their 16-byte vector bodies.  Returns the slot stride in elements, or 0 if the p - 1
 * slots do not fit the workspace (the caller then pulls). */
static int64_t rb_push_slot(const rb_ctx *x)
{
    int64_t e16 = (int64_t)(16 / x->es), bmax = 0;
    for (int u = 0; u < x->adjsize; u++) {
        int64_t off, n;
        rb_block(x, u, &off, &n);
        if (n > bmax) bmax = n;
    }
    int64_t stride = (bmax + e16 + 63) / 64 * 64; /* 256-byte multiples (x 4 or 8 B) */
    if ((size_t)((x->adjsize - 1) * stride) * x->es > x->c->ws_bytes) return 0;
    return stride;
}

static void *rb_push_at(const rb_ctx *x, void *R, int j, int64_t block_off)
{
    int64_t e16 = (int64_t)(16 / x->es);
    return at(x, R, (int64_t)(j - 1) * x->slot + block_off % e16);
}

/* The reduce-scatter of rb_mesh in push form (see rb_push_slot): one launch of p - 1 remote
 * copies, the phase's agree (every slot has landed), the owner's tree over local memory,
 * and one more agree before the allgather reads the owners' blocks.  Kill points and
 * outcomes are rb_mesh's (no idle rank: every failure aborts). */
static void rb_mesh_push_rs(rb_ctx *x, const void *sbuf, void *rbuf)
{
    ftar_comm *c = x->c;
    const int L = x->steps, p = x->adjsize, v = x->vrank;
    void *W = c->ws[WS_W];
    int64_t own0 = x->rindex[L - 1], own_n = x->rcount[L - 1];
    rb_pass(x, FTAR_PH_LOOP, FTAR_PT_BEFORE);
    ftar_enter(c);
    fdev_seg segs[FDEV_MAX_SEGS];
    int ns = 0;
    for (int j = 1; j < p; j++) { /* owner u = v ^ j: its tree takes x_v as src[j] */
        int u = v ^ j;
        int64_t off, n;
        rb_block(x, u, &off, &n);
        void *R = ftar_buf(c, c->order[rb_real(x, u)], WS_R);
        segs[ns++] = (fdev_seg){FDEV_COPY, FDEV_REMOTE_OUT, rb_push_at(x, R, j, off), at(x, (void *)sbuf, off), NULL,
                                (size_t)n, NULL};
    }
    double lb0 = ftar_link_bytes(c);
    ftar_run(c, x->dtype, x->op, segs, ns, FDEV_TAG_STEP0);
    rb_launched(x, FTAR_PH_LOOP); /* every step's DURING point: the pushes are in flight */
    ftar_drain(c);
    c->stats.step0_link_bytes += ftar_link_bytes(c) - lb0;
    rb_close(x, FTAR_PH_LOOP, L);
    uint64_t newf = ftar_step_sync(c, 3); /* every slot landed (:258-265) */
    if (newf) rb_handler_rs(x, newf, L - 1); /* no idle rank: aborts */
    const void *src[FDEV_MAX_TREE];
    src[0] = at(x, (void *)sbuf, own0);
    for (int j = 1; j < p; j++) src[j] = rb_push_at(x, c->ws[WS_R], j, own0);
    /* push == 2: the allgather rides on the tree -- its result goes to this rank's rbuf
     * and straight into every peer's W (the owner's block, remote stores) */
    void *more[FDEV_MAX_TREE];
    int nmore = 0;
    if (x->push == 2) {
        rb_pass(x, FTAR_PH_AG, FTAR_PT_BEFORE);
        ftar_enter(c);
        for (int j = 1; j < p; j++) more[nmore++] = at(x, ftar_buf(c, c->order[rb_real(x, v ^ j)], WS_W), own0);
    }
    void *out = x->push == 2 ? at(x, rbuf, own0) : at(x, W, own0);
    if (x->push == 1) { /* as the pull form: the block into rbuf too, where co-aligned (rb_mesh_tree) */
        more[0] = at(x, rbuf, own0);
        x->own_in_rbuf = x->io_safe && (((uintptr_t)more[0] ^ (uintptr_t)out) & 15) == 0;
        nmore = x->own_in_rbuf;
    }
    ftar_launch_check(c, fdev_tree_out(c->dev, x->dtype, x->op, src, p, 0, out, more, nmore, x->push == 2,
                                       (size_t)own_n, FDEV_TAG_STEP));
    ftar_note_launch(c, x->push == 2 ? more[0] : NULL, 0);
    if (x->push == 2) rb_launched(x, FTAR_PH_AG);
    ftar_drain(c);
    if (x->push == 2) rb_close(x, FTAR_PH_AG, L);
    /* every owner's block is final (push == 1: before the allgather pulls it; push == 2:
     * every peer's pushed block has landed in this rank's W) */
    newf = ftar_step_sync(c, 3);
    if (newf) rb_handler_rs(x, newf, L - 1);
}

/* push == 2, after rb_mesh_push_rs: the peers' blocks, pushed into this rank's W, to rbuf
 * (one local copy launch), then the ERRORS_ARE_FATAL barrier (:357-360).  The copy comes
 * before this rank arrives at the barrier: no peer's next call can push into W while it
 * is being read. */
static int rb_mesh_push_finish(rb_ctx *x, void *rbuf)
{
    ftar_comm *c = x->c;
    const int p = x->adjsize, v = x->vrank;
    fdev_seg segs[FDEV_MAX_SEGS];
    int ns = 0;
    for (int j = 1; j < p; j++) {
        int64_t off, n;
        rb_block(x, v ^ j, &off, &n);
        segs[ns++] = (fdev_seg){FDEV_COPY, 0, at(x, rbuf, off), at(x, c->ws[WS_W], off), NULL, (size_t)n, NULL};
    }
    ftar_run(c, x->dtype, x->op, segs, ns, FDEV_TAG_LOCAL);
    ftar_drain(c);
    ftar_pass_post(c);
    uint64_t newf = ftar_step_sync(c, 3);
    if (newf) rb_handler_ag(x, newf, 0); /* no idle rank: aborts */
    ftar_stats_end(c);
    return FTAR_SUCCESS;
}

/* The pull forms' reduce-scatter up to its one launch: T(v, L) over this rank's final block,
 * one tree kernel over the p - 1 peers' inputs (see rb_mesh).  Returns the link-byte counter
 * before the launch, for the caller's step0_link_bytes. */
static double rb_mesh_tree(rb_ctx *x, const void *sbuf, void *rbuf)
{
    ftar_comm *c = x->c;
    const int L = x->steps, p = x->adjsize, v = x->vrank;
    void *W = c->ws[WS_W];
    int64_t own0 = x->rindex[L - 1], own_n = x->rcount[L - 1];
    rb_pass(x, FTAR_PH_LOOP, FTAR_PT_BEFORE);
    ftar_enter(c);
    const void *src[FDEV_MAX_TREE];
    unsigned remote = 0;
    for (int j = 0; j < p; j++) {
        int u = v ^ j;
        /* a peer's input: its sbuf in place, or its staged IN */
        src[j] = j == 0 ? at(x, (void *)sbuf, own0) : at(x, ftar_buf(c, c->order[rb_real(x, u)], WS_IN), own0);
        if (j) remote |= 1u << j;
    }
    double lb0 = ftar_link_bytes(c);
    ftar_note_launch(c, src[1], (size_t)own_n * x->es);
    /* the block goes to W, where the peers' allgather pulls it, and in the same pass to its
     * place in rbuf (a second destination of the tree: one more local store of S/p), so the
     * allgather only pulls the peers' blocks -- no local copy of this rank's own block, S/p
     * fewer HBM reads per call (in place, rbuf's block is sbuf's, read by this lane only) */
    void *own_out = at(x, rbuf, own0);
    /* only where rbuf is co-aligned with W (a 16-byte vector body needs every operand at the
     * same offset mod 16; otherwise the tree would fall back to scalar accesses): else the
     * allgather copies the block out of W as before */
    x->own_in_rbuf = x->io_safe && (((uintptr_t)own_out ^ (uintptr_t)at(x, W, own0)) & 15) == 0;
    ftar_launch_check(c, fdev_tree_out(c->dev, x->dtype, x->op, src, p, remote, at(x, W, own0), &own_out,
                                       x->own_in_rbuf, 0, (size_t)own_n, FDEV_TAG_STEP0));
    return lb0;
}

/* The mesh allgather's one launch: this rank's final block W -> rbuf and every peer's final
 * block, pulled out of its W, into rbuf (the operands are known before the reduce-scatter's
 * barrier: the launch can be queued ahead of it, behind a gate). */
static int rb_mesh_ag_segs(rb_ctx *x, void *rbuf, fdev_seg *segs)
{
    ftar_comm *c = x->c;
    const int L = x->steps, p = x->adjsize, v = x->vrank;
    int ns = 0;
    if (!x->own_in_rbuf)
        segs[ns++] = (fdev_seg){FDEV_COPY, 0, at(x, rbuf, x->rindex[L - 1]), at(x, c->ws[WS_W], x->rindex[L - 1]),
                                NULL, (size_t)x->rcount[L - 1], NULL};
    for (int j = 1; j < p; j++) {
        int u = v ^ j;
        int64_t off, n;
        rb_block(x, u, &off, &n);
        void *PW = ftar_buf(c, c->order[rb_real(x, u)], WS_W);
        segs[ns++] = (fdev_seg){FDEV_COPY, FDEV_REMOTE_X, at(x, rbuf, off), at(x, PW, off), NULL, (size_t)n, NULL};
    }
    return ns;
}

/* The mesh with its allgather ordered on the device (FTAR_OPT_MESH_WAIT): the tree launch of
 * the pull form, then this.  The reduce-scatter's agree only ever served to say "every
 * owner's block is final" -- with no idle rank every failure aborts the job at whichever
 * agree sees it (new_entry = -1, raben/errhandler.c:207-211, 377-378) -- so that fact moves
 * to the device: each rank releases its tree (a fenced marker) and publishes the call's token
 * in its line of the control block's flag page (host memory every GPU maps); the allgather,
 * queued right behind, runs once every peer's flag holds the token.  Per call this saves one
 * host agree round, one drain and the allgather's launch latency; the call keeps its first
 * and last agree.  A peer that dies before publishing: the drain's failure detector gives
 * the wait up (the allgather returns untouched), and the last agree sees the death -- the
 * handler aborts, as at the agree this form leaves out.  A wait the device gave up with
 * every member alive (its timeout): each rank publishes its verdict in the last agree round,
 * so all of them learn it alike; by then every tree is released (each rank drained its own
 * before arriving), the ranks whose allgather returned untouched launch it again (it never
 * writes what it reads), and one more round keeps the peers' next call off their W until it
 * is done.  Every step's kill points are passed, in the order both launches are queued: RS
 * BEFORE, DURING; AG BEFORE, DURING; then, once drained, RS AFTER / BARRIER and AG AFTER /
 * BARRIER. */
static int rb_mesh_devwait(rb_ctx *x, const void *sbuf, void *rbuf)
{
    ftar_comm *c = x->c;
    const int L = x->steps, p = x->adjsize, v = x->vrank;
    fdev_seg segs[FDEV_MAX_SEGS];
    double lb0 = rb_mesh_tree(x, sbuf, rbuf);
    rb_launched(x, FTAR_PH_LOOP);
    rb_pass(x, FTAR_PH_AG, FTAR_PT_BEFORE);
    /* the call's token: the agree sequence number, uniform over the members and only growing */
    const uint64_t token = c->job.seq;
#ifdef FTAR_TEST_HOOKS
    /* TEST-ONLY: this rank's flag published late (its peers' waits time out) */
    if (getenv("FTAR_PEER_WAIT_DELAY_US")) {
        ftar_drain(c); /* the tree done first: the delay is in the host, not on the device */
        usleep((useconds_t)atoll(getenv("FTAR_PEER_WAIT_DELAY_US")));
    }
#endif
    void *pf[FDEV_MAX_PEERS];
    int np = 0;
    for (int j = 1; j < p; j++) pf[np++] = ftar_flag(c, c->order[rb_real(x, v ^ j)]);
    for (int i = 0; i < c->size; i++) /* FTAR_TRACE: each flag line is its owner's */
        fdev_trace_region(c->dev, ftar_flag(c, c->order[i]), sizeof(c->job.shm->pwflag[0]), c->order[i], "PF");
    if (fdev_peer_wait(c->dev, ftar_flag(c, c->wrank), pf, np, token, ftar_watch_peers, c)) {
        fprintf(stderr, "ftar: rank %d: peer wait failed: %s\n", c->wrank, fdev_last_error());
        ftar_ctrl_abort(&c->job, FTAR_ERR_DEVICE);
    }
    int ns = rb_mesh_ag_segs(x, rbuf, segs);
    ftar_run(c, x->dtype, x->op, segs, ns, FDEV_TAG_STEP);
    rb_launched(x, FTAR_PH_AG);
    ftar_drain_watch(c);
    const int ran = fdev_peer_wait_verdict(c->dev);
    if (!ran) c->stats.peer_wait_skips++;
    /* both phases close at once: one exchange mark, two mesh exchanges */
    ftar_exchange_done(c);
    c->stats.step0_link_bytes += ftar_link_bytes(c) - lb0;
    c->stats.steps += 2 * L;
    c->stats.mesh_steps += 2;
    c->stats.peer_waits++;
    rb_pass(x, FTAR_PH_LOOP, FTAR_PT_AFTER);
    rb_pass(x, FTAR_PH_LOOP, FTAR_PT_BARRIER);
    rb_pass(x, FTAR_PH_AG, FTAR_PT_AFTER);
    rb_pass(x, FTAR_PH_AG, FTAR_PT_BARRIER);
    ftar_pass_post(c);
    /* the reduce-scatter's and the allgather's agree and the ERRORS_ARE_FATAL barrier: one
     * round, which also carries every rank's verdict */
    c->pubval = ran ? 0 : 1;
    uint64_t newf = ftar_step_sync(c, 1);
    c->pubval = 0;
    if (newf) rb_handler_ag(x, newf, 0); /* no idle rank: aborts */
    int any_skipped = 0;
    for (int i = 0; i < c->size; i++) any_skipped |= ftar_peer_pub(c, c->order[i]) != 0;
    if (any_skipped) {
        if (!ran) {
            ftar_run(c, x->dtype, x->op, segs, ns, FDEV_TAG_STEP);
            ftar_drain(c);
        }
        newf = ftar_step_sync(c, 1);
        if (newf) rb_handler_ag(x, newf, 0);
    }
    ftar_stats_end(c);
    return FTAR_SUCCESS;
}

/* The pull form's reduce-scatter ordered on the host (FTAR_OPT_MESH_WAIT=0): the tree, its
 * drain and the phase's agree, after which the allgather is launched.
 * (Round 4's form with the allgather queued behind the tree behind a host-opened gate,
 * FTAR_GATE_MAX >= S, was slower in every rehearsal and is superseded by the device wait:
 * removed in round 6.) */
static void rb_mesh_pull_rs(rb_ctx *x, const void *sbuf, void *rbuf)
{
    ftar_comm *c = x->c;
    double lb0 = rb_mesh_tree(x, sbuf, rbuf);
    rb_launched(x, FTAR_PH_LOOP); /* every step's DURING point: the one launch is in flight */
    ftar_drain(c);
    c->stats.step0_link_bytes += ftar_link_bytes(c) - lb0;
    rb_close(x, FTAR_PH_LOOP, x->steps);
    uint64_t newf = ftar_step_sync(c, 2); /* agree + barrier (:258-265) */
    if (newf) rb_handler_rs(x, newf, x->steps - 1); /* no idle rank: aborts */
}

/* The allgather ordered on the host, after the reduce-scatter's agree (pull or push 1):
 * every peer's final block into rbuf, this rank's own out of W. */
static int rb_mesh_allgather(rb_ctx *x, void *rbuf)
{
    ftar_comm *c = x->c;
    fdev_seg segs[FDEV_MAX_SEGS];
    rb_pass(x, FTAR_PH_AG, FTAR_PT_BEFORE);
    ftar_enter(c);
    int ns = rb_mesh_ag_segs(x, rbuf, segs);
    ftar_run(c, x->dtype, x->op, segs, ns, FDEV_TAG_STEP);
    rb_launched(x, FTAR_PH_AG);
    ftar_drain(c);
    rb_close(x, FTAR_PH_AG, x->steps);
    /* The allgather's agree (:330-335) and the ERRORS_ARE_FATAL barrier (:357-360; no
     * post-step at rem = 0) are one round: a failure seen at either ends the job the same
     * way (no idle rank: errhandler_allgather aborts, new_entry = -1, :377-378), so the
     * outcome of every kill point is unchanged. */
    ftar_pass_post(c);
    uint64_t newf = ftar_step_sync(c, 2);
    if (newf) rb_handler_ag(x, newf, 0); /* no idle rank: aborts */
    ftar_stats_end(c);
    return FTAR_SUCCESS;
}

/* The tolerant region at power-of-two p without an idle rank, on the full xGMI mesh.
 *
 * Recursive halving leaves in vrank v's final block the value
 *     T(v, L),  T(v, 0) = x_v,  T(v, s+1) = T(v, s) op T(v ^ 2^s, s)
 * (raben/rabenseifner.c:231-237: own window first, the partner's second; the partner's
 * window was reduced by the same rule).  With the sources listed owner-relative
 * (src[j] = x_{v^j}) that is the left-to-right balanced tree over j, which one tree
 * kernel computes from p - 1 one-hop pulls -- every link of the GPU busy with 1/p of the
 * vector instead of one link per step.  The allgather (:299-355) likewise pulls every
 * peer's final block straight into rbuf.  Per rank and direction each link carries
 * S/p for the reduce-scatter and S/p for the allgather: the mesh lower bound for an
 * allreduce, half of what a 2-hop relay moves.
 *
 * The reference's per-step states are unobservable here: with no idle rank every
 * handler aborts (new_entry = -1, raben/errhandler.c:207-211, 377-378), so a failure
 * anywhere in a phase ends the job exactly as it would at that step's agree.  Every
 * step's kill points are still passed (the injected death lands in the same phase), and
 * each phase ends in the reference's agree + barrier. */
static int rb_mesh(rb_ctx *x, const void *sbuf, void *rbuf)
{
    if (x->push == 2) {
        rb_mesh_push_rs(x, sbuf, rbuf);
        return rb_mesh_push_finish(x, rbuf);
    }
    if (x->devwait) return rb_mesh_devwait(x, sbuf, rbuf); /* never with push */
    if (x->push) rb_mesh_push_rs(x, sbuf, rbuf);
    else rb_mesh_pull_rs(x, sbuf, rbuf);
    return rb_mesh_allgather(x, rbuf);
}

/* The one-shot launch's operands as the peers' inputs stand now (ftar_buf: a peer's
 * exported sbuf once ftar_resolve_inputs mapped it, else its staged IN). */
static void rb_oneshot_plan(rb_ctx *x, const void *sbuf, void *rbuf, struct rb_batch *B)
{
    ftar_comm *c = x->c;
    const int p = x->adjsize, v = x->vrank;
    memset(B, 0, sizeof(*B));
    for (int u = 0; u < p; u++) { /* block owned by vrank u */
        int64_t off, n;
        rb_block(x, u, &off, &n);
        B->out[u] = at(x, rbuf, off);
        B->n[u] = (size_t)n;
        for (int j = 0; j < p; j++) {
            const int w = u ^ j;
            if (w == v) {
                B->src[u * p + j] = at(x, (void *)sbuf, off);
            } else {
                B->src[u * p + j] = at(x, ftar_buf(c, c->order[rb_real(x, w)], WS_IN), off);
                B->remote[u] |= 1u << j;
            }
        }
    }
}

/* Queue the one-shot launch right behind this rank's staging copy, before the barrier
 * after which the peers' staged inputs may be read: its workgroups wait on a gate that
 * rb_oneshot opens at the point where it would otherwise launch, so the launch latency
 * overlaps the staging drain and the barrier.  The plan assumes every peer stages its
 * input (this rank did, so the size is the same everywhere); rb_oneshot re-plans after
 * the inputs are resolved and skips the gated launch if anything differs. */
static void rb_oneshot_prelaunch(rb_ctx *x, const void *sbuf, void *rbuf, void *stage_dst)
{
    ftar_comm *c = x->c;
    x->gated = 0;
    if (!c->gate) return;
    rb_oneshot_plan(x, sbuf, rbuf, &x->gplan);
    /* stage_dst: this rank's staging copy (sbuf -> IN) rides in the same launch, ahead of
     * the gate -- one launch per call instead of two */
    ftar_launch_check(c, fdev_tree_batch_staged_gated(c->dev, x->dtype, x->op, x->gplan.src, x->adjsize,
                                                      x->gplan.remote, x->gplan.out, x->gplan.n, x->adjsize,
                                                      FDEV_TAG_STEP0, stage_dst, sbuf, stage_dst ? x->count : 0,
                                                      &x->gated));
    if (x->gated) c->stats.gated_launches++;
}

/* One-shot mesh for small vectors: the allgather's data movement folded into the
 * reduce-scatter launch.  Each rank evaluates EVERY block in its owner's tree,
 * T(u, L) = tree over x_(u^j) (the same operands and order as rb_mesh's reduce-scatter,
 * so the same bits), straight into rbuf: one launch instead of two, (p-1) S link bytes
 * per rank instead of 2 (p-1) S / p -- cheaper below the size where a launch + drain
 * (~11 us) outweighs the extra link time.  Kill points and the two agree rounds are
 * rb_mesh's; with no idle rank a failure anywhere aborts. */
static int rb_oneshot(rb_ctx *x, const void *sbuf, void *rbuf)
{
    ftar_comm *c = x->c;
    const int L = x->steps, p = x->adjsize;
    rb_pass(x, FTAR_PH_LOOP, FTAR_PT_BEFORE);
    ftar_enter(c);
    struct rb_batch B;
    rb_oneshot_plan(x, sbuf, rbuf, &B);
    const void *const *src = B.src;
    double lb0 = ftar_link_bytes(c);
    for (int k = 0; k < p * p; k++) /* the first peer operand: the padding's re-pull source */
        if (B.remote[k / p] & (1u << (k % p))) {
            ftar_note_launch(c, src[k], B.n[k / p] * x->es);
            break;
        }
    /* the queued launch runs now, or returns untouched and is replaced (also when another
     * launch has given it up meanwhile) */
    int pending = x->gated && fdev_gate_pending(c->dev);
    int go = pending && memcmp(&B, &x->gplan, sizeof(B)) == 0;
    if (x->gated && !go) c->stats.gated_skips++;
    if (pending) fdev_gate_open(c->dev, !go);
    x->gated = 0;
    if (!go)
        ftar_launch_check(c, fdev_tree_batch(c->dev, x->dtype, x->op, src, p, B.remote, B.out, B.n, p, FDEV_TAG_STEP0));
    rb_launched(x, FTAR_PH_LOOP);
    ftar_drain(c);
    c->stats.step0_link_bytes += ftar_link_bytes(c) - lb0;
    rb_close(x, FTAR_PH_LOOP, 2 * L); /* the one exchange stands for both phases' steps */
    /* The reduce-scatter's agree (:258-265), the allgather's (:330-335) and the
     * ERRORS_ARE_FATAL barrier (:357-360) are one round here: the allgather's data moved in
     * the same launch, and with no idle rank a failure seen at any of them ends the job the
     * same way (both handlers abort, new_entry = -1, errhandler.c:207-211, 377-378) -- the
     * kill points of every phase are passed before it, so each one's outcome is unchanged. */
    rb_pass(x, FTAR_PH_AG, FTAR_PT_BEFORE);
    ftar_enter(c); /* the allgather's data already moved in the one launch */
    rb_launched(x, FTAR_PH_AG);
    ftar_exchange_done(c); /* no second exchange to count: the phase closes without rb_close */
    rb_pass(x, FTAR_PH_AG, FTAR_PT_AFTER);
    rb_pass(x, FTAR_PH_AG, FTAR_PT_BARRIER);
    ftar_pass_post(c);
    uint64_t newf = ftar_step_sync(c, 1);
    if (newf) rb_handler_rs(x, newf, L - 1); /* no idle rank: aborts */
    ftar_stats_end(c);
    return FTAR_SUCCESS;
}
