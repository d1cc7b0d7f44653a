// ftar_kernels.h -- internal interface between the HIP runtime glue and the kernels.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>

namespace ftar {

enum {
    kInt32 = 0, kFloat32 = 1, kInt64 = 2, kFloat64 = 3, kFloat16 = 16, kBFloat16 = 17,
    kFloatInt = 32, k2Int = 33, kDoubleInt = 34, // MPI's pair types: 8, 8 and 16 bytes, kMaxloc / kMinloc only
    kInt8 = 48, kUInt8 = 49, kInt16 = 50, kUInt16 = 51, kUInt32 = 52, kUInt64 = 53 // ops 0..9 (canon_dtype)
};
enum {
    kSum = 0, kProd = 1, kMax = 2, kMin = 3, kLand = 4, kBand = 5, kLor = 6, kBor = 7, kLxor = 8, kBxor = 9,
    kMaxloc = 16, kMinloc = 17
};
constexpr int kNumOps = 10; // logical / bitwise ops (>= kLand) exist for the integer types only
// an op some element type has (which types: with_op in ftar_kernels.hip)
inline bool op_known(int op) { return (op >= 0 && op < kNumOps) || op == kMaxloc || op == kMinloc; }
// The canonical dispatch: the element type whose instantiation computes `op` on `dtype`.  Within
// one width, signed and unsigned integers give identical bits for SUM and PROD (modulo 2^w) and
// for the logical and bitwise ops; only MAX / MIN compare.  So each width has ONE type with all
// ten ops (uint8_t, uint16_t, int32_t, int64_t) and its sibling is instantiated for MAX / MIN
// alone.  The one dtype dispatcher of ftar_kernels.hip (with_type) switches on this.  Never across
// widths: the planners (ftar_plan.cpp) derive heads, tails and vector counts from the element size.
inline int canon_dtype(int dtype, int op)
{
    const bool order = op == kMax || op == kMin;
    switch (dtype) {
    case kInt8: return order ? kInt8 : kUInt8;
    case kInt16: return order ? kInt16 : kUInt16;
    case kUInt32: return order ? kUInt32 : kInt32;
    case kUInt64: return order ? kUInt64 : kInt64;
    default: return dtype;
    }
}
enum { kCopy = 0, kReduce = 1 };

constexpr int kMaxKSegs = 48; // 16 user segments x (head, body, tail); 2.3 KB of kernarg
constexpr int kTileVecs = 1024; // 16-byte vectors per workgroup tile (256 threads x 4)
constexpr int kBlock = 256; // threads per workgroup: the kernels (ftar_kernels.hip) and the planners (ftar_plan.cpp)
// 4 x 16 B per lane and operand (16 KiB per operand per workgroup): 6.49-6.50 TB/s on
// rotating buffers with nt stores against 6.14-6.20 for 2 and 6.05-6.09 for 8
// (tools/hbm_sweep.hip, profiles/r02/hbm_sweep_focused.txt)
constexpr int kUnroll = 4;
static_assert(kBlock * kUnroll == kTileVecs, "tile size");
constexpr int kChunkTiles = 8; // tiles per chunk of the interleaved block mapping (128 KiB)
constexpr int kMaxIleave = 16; // vector pieces that can share the interleaved prefix

// Completion signal of a short launch (the small-message path): instead of a
// marker packet the host spins on, the kernel itself tells the host it is done.  Every
// workgroup, once its stores have completed, releases them at system scope (write-back of
// its XCD's L2: the data is in HBM for peer GPUs and the host) and adds one to `cnt`; the
// workgroup whose add completes the grid resets `cnt` and stores `tag` into `flag`, a word of
// pinned host memory the host polls.  `acquire`: every workgroup first invalidates its
// cached copies of remote memory (system-scope acquire) -- the host sets it when the last
// drain was such a signal, i.e. no marker packet has invalidated the caches since the
// barrier after which this launch reads the peers' new data.
//
// `gate` (optional): the launch was queued before the host barrier that makes its
// operands ready.  Thread 0 of every workgroup polls the pinned host word (system scope)
// until it reaches gate_val (= 2 x sequence, bit 0 set = skip), the workgroup then runs or
// returns without touching memory; either way it signals.  A gate still closed after
// gate_ticks of the wall clock (tens of seconds: the host never got past its barrier) is
// taken as skip and reported through `err`, which the host checks after the drain.
constexpr unsigned kGateSlots = 8; // gate words, used in turn (sig_flag[16 + seq % 8])
struct KSignal {
    unsigned *cnt;  // device counter, agent-scope atomics; nullptr = no signal
    unsigned *flag; // pinned host word
    unsigned tag;
    unsigned acquire;
    const unsigned *gate; // pinned host word (slot gate_val / 2 % kGateSlots); nullptr = not gated
    unsigned gate_val;
    unsigned *err;        // pinned host word of this gate's slot: set to gate_val on a gate timeout
    unsigned long long gate_ticks;
    // Relayed gate (every gated launch of FTAR_GATE_RELAY_MIN = 2 workgroups or more: the short
    // signalling ones and the mid-size ones queued behind a fenced marker): only the first
    // workgroup to start -- elected by an atomic max of gate_val into *gate_poll -- polls the
    // host word over PCIe; it relays the verdict through the device word *gate_dev, which the
    // other workgroups poll.  nullptr = the workgroup polls the host word itself.
    unsigned *gate_poll;
    unsigned *gate_dev;
    // Optional staging phase BEFORE the gate (a gated launch that also stages this rank's
    // input for its peers, saving the separate staging launch): every workgroup copies its
    // share of stage_n elements of stage_es bytes from stage_src to stage_dst, releases its
    // stores at system scope and counts itself in stage_cnt; the last one stores stage_tag
    // into `flag` -- the host's signal that the input is staged, before it opens the gate.
    const void *stage_src;
    void *stage_dst;
    size_t stage_n;
    unsigned stage_es;
    unsigned stage_tag;
    unsigned *stage_cnt;  // device counter (agent scope)
    // Behind a peer wait (PeerWait, queued just before on the same stream): every workgroup
    // runs only if the wait kernel wrote `vval` into the device word *vword (go); any other
    // value (vval | 1: given up) and it returns untouched.  nullptr = no wait in front.
    const unsigned *vword;
    unsigned vval;
};

// The wait of the mesh allgather for the peers' reduce-scatter (fdev_peer_wait): ONE
// wavefront.  Lane 0 first publishes this rank's flag (`token` into *own, system scope: the
// flags are lines of one host page every rank's GPU maps, read coherently by every GPU of the
// node; the tree's data was released to HBM device-wide by the fenced marker in front of this
// kernel); then lane i polls peer i's flag over PCIe (system-scope loads of host memory)
// until every one holds at least `token`, the host's abort word holds vval (a peer died: give
// up), or `ticks` of the wall clock pass (give up, so the grid always drains).  The verdict
// (vval = go, vval | 1 = given up) goes to *verdict_dev for the launch behind it and to the
// pinned host word *verdict_host for the host after its drain.
constexpr int kMaxPeers = 15;
struct PeerWait {
    unsigned long long *own;
    const unsigned long long *peer[kMaxPeers];
    int npeers;
    unsigned long long token;
    const unsigned *abort_word;
    unsigned *verdict_dev;
    unsigned *verdict_host;
    unsigned vval;
    unsigned long long ticks;
};
hipError_t launch_peer_wait(const PeerWait &W, hipStream_t s);

struct KSeg {
    void *out;
    void *out2;          // optional second destination (same values), nullptr = none
    const void *x;
    const void *y;
    size_t n;
    unsigned kind;
    unsigned vec;
    unsigned blk_begin;  // sequential region: blocks [blk_begin, blk_end) ...
    unsigned blk_end;
    unsigned tile_base;  // ... take tiles tile_base, tile_base + 1, ... of this piece
    unsigned ntiles;     // tiles of the whole piece (the stride of a capped grid)
};

// Blocks [0, il_blocks) are dealt round-robin, one kChunkTiles chunk at a time, over the
// vector pieces il[0..nil): pieces that pull from different peers then stream over
// their xGMI links at the same time instead of one after the other.  The remaining
// blocks map sequentially (blk_begin/blk_end) onto what is left of every piece.
struct KSegList {
    KSeg s[kMaxKSegs];
    int nseg;
    int nil;
    unsigned il_blocks;
    unsigned char il[kMaxIleave];
    unsigned nt_store; // 16-byte stores non-temporal (set by the caller after plan_segments)
    KSignal sig;       // optional completion signal (sig.cnt == nullptr: none)
};

// What one workgroup of segment_kernel processes: piece `seg`, starting at tile (vector
// pieces) or block slot (scalar pieces) `first`, then every `stride`-th one.  Shared by
// the kernel and the host-side coverage test (tests/kernel_plan).
struct BlockWork {
    int seg;
    size_t first;
    size_t stride;
};

__host__ __device__ inline BlockWork map_block(const KSegList &L, unsigned b)
{
    BlockWork w;
    if (b < L.il_blocks) { // interleaved prefix: chunk q of piece il[q % nil]
        const unsigned q = b / kChunkTiles;
        w.seg = L.il[q % (unsigned)L.nil];
        w.first = (size_t)(q / (unsigned)L.nil) * kChunkTiles + b % kChunkTiles;
        w.stride = L.s[w.seg].ntiles;
        return w;
    }
    int si = 0;
    while (si + 1 < L.nseg && b >= L.s[si].blk_end) si++;
    const KSeg &S = L.s[si];
    const size_t j = b - S.blk_begin, nblk = S.blk_end - S.blk_begin;
    w.seg = si;
    w.first = (S.vec ? S.tile_base : 0) + j;
    w.stride = (S.vec && S.tile_base) ? S.ntiles : nblk;
    return w;
}

struct SegIn {
    int kind;
    void *out;
    const void *x;
    const void *y;
    size_t n;
    void *out2;
};

// Tree reduce: out[i] = balanced left-to-right tree of src[0..p-1][i] (p = 2, 4, 8, 16):
// ((s0 op s1) op (s2 op s3)) op ...  With the sources in owner-relative order
// (src[j] = vrank owner ^ j) this is exactly the value recursive halving leaves in the
// owner's final block (every level: the owner's subtree first).
constexpr int kMaxTree = 16;
constexpr int kMaxMore = 7; // extra destinations of one tree (the push mesh's allgather: every peer)
struct TreeArgs {
    const void *src[kMaxTree];
    void *out;
    void *more[kMaxMore]; // further destinations receiving the same values (nmore of them)
    int nmore;
    size_t n;      // elements
    size_t head;   // scalar elements before the 16-byte vector body (co-aligned sources)
    size_t nv;     // 16-byte vectors in the body (0 when the pointers are not co-aligned)
    unsigned nvb;  // workgroups of the vector body; the rest do the scalar elements
    unsigned nt_store; // 16-byte stores non-temporal
    unsigned unroll;   // 16-byte vectors per lane and source (1, 2, 4; > 1 only for tree_kernel at p = 4, 8)
};
constexpr int kMaxUnroll = 4;
// fills the alignment fields of A (src/out/n/unroll set) and returns the grid size
unsigned plan_tree(TreeArgs *A, int p, size_t esize, unsigned max_blocks);
hipError_t launch_tree(int dtype, int op, int p, const TreeArgs &A, unsigned grid, hipStream_t s);
// up to kMaxBatch trees of p <= kMaxBatchP sources in one launch; tree k owns
// workgroups [first[k], first[k + 1])
constexpr int kMaxBatch = 8, kMaxBatchP = 8;
struct TreeBatch {
    TreeArgs t[kMaxBatch];
    unsigned first[kMaxBatch + 1];
    int nt;
    KSignal sig; // optional completion signal
};
unsigned plan_tree_batch(TreeBatch *B, int p, size_t esize, unsigned max_blocks);
// shrinks a planned batch to at most max_total workgroups by giving each vector workgroup
// several chunks (its scalar workgroups stay); the new grid, or 0 if it cannot fit
unsigned cap_tree_batch(TreeBatch *B, unsigned max_total);
hipError_t launch_tree_batch(int dtype, int op, int p, const TreeBatch &B, unsigned grid, hipStream_t s);

// Table-driven gather / scatter (fdev_gather: the mover of ftar_allreduce_multi).  The table --
// {user pointer, packed byte offset, bytes} per entry, non-empty, ascending and dense -- lives in
// device memory (1024 entries do not fit the kernel arguments).  The grid is laid out in PACKED
// space, one workgroup per 16 KiB tile (capped, with a stride loop), so the load is balanced
// whatever the entries' sizes: a workgroup finds the first entry overlapping its tile by binary
// search (gather_first) and walks the entries that follow while they overlap it (gather_piece).
constexpr int kMaxGather = 1024;
constexpr size_t kTileBytes = (size_t)kTileVecs * 16;
struct GEntry {
    void *ptr;
    size_t off;
    size_t bytes;
};
struct GatherArgs {
    char *packed;
    const GEntry *tab; // device memory
    int n;
    unsigned es;       // element size of the call: 1, 2, 4, 8, 16
    size_t total;      // bytes of the packed vector
    unsigned ntiles;
    KSignal sig;       // optional completion signal
};

// The entry holding packed byte `lo` (< total): the last one whose offset is <= lo.  (A template
// over the pointer type: the kernel reads the table through the constant address space.)
template <typename Tab> __host__ __device__ inline int gather_first(Tab tab, int n, size_t lo)
{
    int a = 0, b = n - 1;
    while (a < b) {
        const int m = (a + b + 1) >> 1;
        if (tab[m].off <= lo) a = m;
        else b = m - 1;
    }
    return a;
}

// What a workgroup moves for one entry inside its tile [lo, hi): `bytes` from `user` to packed
// offset `poff` (or back).  Where the user address and the packed address are congruent mod 16
// (vec): a head of `head` bytes up to the packed 16-byte boundary, nvec 16-byte vectors, a tail;
// otherwise everything element by element (head = bytes, nvec = 0).  Heads, tails and unaligned
// pieces move in units of `unit` bytes: the element size, 8 for the 16-byte type (two halves,
// its alignment is 8), lowered to what the two addresses allow (a pair of 4-byte fields needs
// 4-byte alignment only).  Offsets and sizes are multiples of the element size, so no element
// straddles a piece.
struct GPiece {
    char *user;
    size_t poff;
    size_t bytes;
    size_t head;
    size_t nvec;
    unsigned unit;
    unsigned vec;
};

__host__ __device__ inline bool gather_piece(const GEntry &E, size_t lo, size_t hi, const char *packed, unsigned es,
                                             GPiece *P)
{
    const size_t b = E.off > lo ? E.off : lo;
    const size_t e = E.off + E.bytes < hi ? E.off + E.bytes : hi;
    if (b >= e) return false;
    P->user = (char *)E.ptr + (b - E.off);
    P->poff = b;
    P->bytes = e - b;
    const uintptr_t ua = (uintptr_t)P->user, pa = (uintptr_t)packed + b;
    unsigned unit = es < 8 ? es : 8;
    while (unit > 1 && ((ua | pa) & (unit - 1))) unit >>= 1;
    P->unit = unit;
    P->vec = ((ua ^ pa) & 15) == 0;
    if (P->vec) {
        const size_t h = (16 - (pa & 15)) & 15;
        P->head = h < P->bytes ? h : P->bytes;
        P->nvec = (P->bytes - P->head) / 16;
    } else {
        P->head = P->bytes;
        P->nvec = 0;
    }
    return true;
}

hipError_t launch_gather(const GatherArgs &A, int scatter, unsigned grid, hipStream_t s);

// The converting sibling (fdev_gather_cvt: the mover of ftar_allreduce_multi_acc32).  The user
// buffers hold 2-byte floats, the packed vector float32: the same table, grid and walk, with
// `off` and `bytes` of an entry counted in PACKED bytes (4 per element), so a tile is 4096
// elements = 8 KiB of user memory, and GatherArgs::es = 4.  Element j of a piece sits at
// user + 2 j and packed + 4 j: the two sides advance at different rates, so "co-aligned" is a
// property of an element, not of the two addresses.  Class k (8, 4, 2 elements per access: 16 /
// 32, 8 / 16, 4 / 8 bytes of user / packed memory) fits a piece when the first element whose
// user address is a multiple of 2 k has a packed address that is a multiple of 4 k; the widest
// class that fits is taken -- the widest one, one 16-byte user access against two 16-byte packed
// ones, exactly where the element at which the user address reaches a 16-byte boundary has its
// packed address on a 32-byte boundary.  `head` elements in front of that element and the
// tail behind the last whole group go element by element (2 / 4 bytes, always aligned: user
// pointers are 2-byte aligned, packed offsets multiples of 4); k = 1: the whole piece does
// (head = n, nvec = 0).  Pieces begin and end on elements: nothing straddles.
struct CPiece {
    char *user;   // first element's user address
    size_t poff;  // its packed byte offset
    size_t n;     // elements
    size_t head;  // elements before the first group
    size_t nvec;  // groups of k elements
    unsigned k;   // 8, 4, 2 or 1
};

__host__ __device__ inline bool cvt_piece(const GEntry &E, size_t lo, size_t hi, const char *packed, CPiece *P)
{
    const size_t b = E.off > lo ? E.off : lo;
    const size_t e = E.off + E.bytes < hi ? E.off + E.bytes : hi;
    if (b >= e) return false;
    P->user = (char *)E.ptr + (b - E.off) / 2;
    P->poff = b;
    P->n = (e - b) / 4;
    const uintptr_t ua = (uintptr_t)P->user, pa = (uintptr_t)packed + b;
    unsigned k = 8;
    size_t h = 0;
    for (; k > 1; k >>= 1) {
        h = (size_t)(((uintptr_t)0 - ua) & (2 * k - 1)) / 2; // elements up to the user boundary of 2 k bytes
        if (((pa + 4 * h) & (4 * k - 1)) == 0) break;
    }
    P->k = k;
    if (k == 1) {
        P->head = P->n;
        P->nvec = 0;
    } else {
        P->head = h < P->n ? h : P->n;
        P->nvec = (P->n - P->head) / k;
    }
    return true;
}

// dtype: kFloat16 or kBFloat16.  scale: applied on scatter only (packed float32 -> scale * a,
// rounded once to nearest even into the 2-byte type); the gather widens exactly.
hipError_t launch_gather_cvt(const GatherArgs &A, int dtype, float scale, int scatter, unsigned grid, hipStream_t s);

// The mixed sibling (fdev_gather_mix: the mover of ftar_allreduce_multi_mixed).  The packed vector
// is float32 and the table counts packed bytes, as the converting mover's; every entry has a type
// of its own, kFloat16, kBFloat16 or kFloat32.  The types are a parallel array of n 32-bit words
// that follows the n GEntry of the table in the same device buffer (and in the pinned mirror, so
// one copy uploads both): GEntry, the other two kernels and their launches stay as they are, and
// an entry still is three 8-byte scalar loads, its type one 4-byte load more.  A 2-byte entry
// moves by cvt_piece / the converting mover's groups; a float32 entry by gather_piece with es = 4
// (a copy on gather; on scatter scale * a, the same 16-byte accesses where user and packed
// addresses are congruent mod 16).
inline const unsigned *mix_types(const GEntry *tab, int n) { return (const unsigned *)(tab + n); }
constexpr size_t kMixEntryBytes = sizeof(GEntry) + sizeof(unsigned);
// types: device memory, mix_types(A.tab, A.n).  scale: applied on scatter only.
hipError_t launch_gather_mix(const GatherArgs &A, const unsigned *types, float scale, int scatter, unsigned grid,
                             hipStream_t s);

unsigned plan_segments(const SegIn *in, int nin, size_t esize, unsigned max_blocks, KSegList *L);
hipError_t launch_segments(int dtype, int op, const KSegList &L, unsigned grid, hipStream_t s);
hipError_t launch_reduce_lds(int dtype, int op, void *inout, const void *in, size_t nvec, unsigned grid,
                             hipStream_t s, unsigned nt_store);

} // namespace ftar
