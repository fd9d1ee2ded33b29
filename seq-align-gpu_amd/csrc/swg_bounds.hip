// swg_bounds.hip -- the coordinates of reported hits without a traceback (swg_align_bounds).
//
// swg_trace.hip stores one predecessor byte per cell and walks them back; most of a pipeline wants only where an
// alignment begins and ends and how long it is.  Those follow from a forward pass alone: every state of the recurrence
// (H, A, B of src/alignment.c:124-161, kept whole as in swg_trace_kernel) carries a tag -- the origin of its path and
// the path's steps so far -- and takes the tag of the predecessor the walk would have chosen (none if the maximum is 0,
// else the first of H, A, B that reaches it).  The best cell's tag is then what the walk would have found.
//
// One lane group of G lanes takes a pair: lane g holds K consecutive query columns in registers and works database row
// t - g at step t, the anti-diagonal wavefront of the fill kernels.  What crosses a lane boundary -- the left
// neighbour's left and diagonal reductions, three registers each -- moves by DPP (row_shr:1 in a 16-lane group,
// wave_shr:1 in wider ones); there is no barrier in the row loop.  Pairs are dealt statically: group g of a launch's n
// takes pairs g, g + n, g + 2n, ... of the launch's order, longest first.  (Every branch around a DPP move or a shuffle
// is decided by the group as a whole -- a ticket fetched by one lane and handed round by a shuffle is not, and the
// compiler is free to send the other lanes round the loop without it.)  Residues are read from the resident
// database's bytes where they lie.
//
// swg_align_stats is the same pass with two counts more in every tag -- the path's identical columns and its
// gap openings -- on a sibling kernel, swg_stats_kernel, that shares the records, the classes and the host path below.
#include "swg_host_internal.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <stdexcept>

struct SwgBoundsJob {
    uint64_t q_off;   // into the batch's queries: first index byte, or first PSSM row
    uint64_t res_off; // the sequence's first byte among the resident residue bytes (index << 3 each)
    uint32_t lq;      // query length
    uint32_t len;     // database sequence length
    uint32_t pad[2];
};

struct SwgBoundsOut {
    int32_t score;
    uint32_t q_begin, q_end, d_begin, d_end, n_ops, pad[2];
};

struct SwgBoundsParams {
    const int8_t *query;  // table indices of the batch's queries, back to back (PSSM kernel: unread)
    const int8_t *sub;    // [32][32], row = query residue (PSSM kernel: unread)
    const int8_t *pssm;   // PSSM kernel: the batch's rows [positions][32], SWG_BOUNDS_COLS rows of slack behind them
    const uint8_t *codes; // the resident database's residue bytes
    const SwgBoundsJob *jobs;
    SwgBoundsOut *out;
    uint32_t n_jobs, n_groups;
    int go, ge;
};

#define SWG_BOUNDS_THREADS 256
#define SWG_BOUNDS_Q_BITS 12 /* tag origin: query position in the low 12 bits (columns <= 1024), sequence position above */
#define BDEVINL __device__ __forceinline__

// lanes without a source lane (and lane 0 of a group inside a wider wavefront, which reads another group) keep `keep`
template <int G> BDEVINL int bounds_from_left(int keep, int src)
{
    return __builtin_amdgcn_update_dpp(keep, src, G == 16 ? 0x111 /* row_shr:1 */ : 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
}

// One state with its tag.
struct BState {
    int v;
    uint32_t org, st;
};

// The value and tag a neighbour cell starts from: max-with-pick over one cell's states as the neighbour sees them
// (x, y, z = H, A, B plus the gap scores of the direction).  A maximum of 0 starts the alignment at this cell (`here`);
// otherwise the first of H, A, B that reaches it is continued.  Either way the step into the neighbour is counted.
BDEVINL BState bounds_reduce(int x, int y, int z, const BState &h, const BState &a, const BState &b, uint32_t here)
{
    const int m3 = max(max(x, y), z);
    BState r;
    r.v = max(m3, 0);
    uint32_t o = b.org, s = b.st;
    if (y == m3) o = a.org, s = a.st;
    if (x == m3) o = h.org, s = h.st;
    s += 1;
    if (m3 <= 0) o = here, s = 1;
    r.org = o, r.st = s;
    return r;
}

template <int G, int K, bool PSSM>
__global__ __launch_bounds__(SWG_BOUNDS_THREADS) void swg_bounds_kernel(SwgBoundsParams p)
{
    __shared__ int8_t s_sub[1024];
    if (!PSSM)
        for (uint32_t k = threadIdx.x; k < 1024; k += SWG_BOUNDS_THREADS) s_sub[k] = p.sub[k];
    __syncthreads(); // (the only one: before any group takes a job)
    const uint32_t lane = threadIdx.x & (G - 1);
    const uint32_t group = (blockIdx.x * SWG_BOUNDS_THREADS + threadIdx.x) / G;
    if (group >= p.n_groups) return;
    const int go = p.go, ge = p.ge;
    const int edge = max(max(go, ge), 0); // what a border cell hands down and to the right
    const uint32_t i0 = lane * K;         // columns i0 + 1 .. i0 + K (from 1, as the rows)

    for (uint32_t jn = group; jn < p.n_jobs; jn += p.n_groups) {
        const SwgBoundsJob job = p.jobs[jn];
        const uint32_t lq = job.lq, len = job.len;
        const uint8_t *d = p.codes + job.res_off;
        const uint32_t steps = len + (lq + K - 1) / K - 1; // lanes past the query's last column are not waited for

        // this lane's columns: their score rows, and the two reductions kept per column -- D: the diagonal one of
        // the row above (what column c + 1 continues), V: the vertical one (this column's own A).  Row 0 is the border.
        uint32_t qrow[K];
        const int8_t *prow = nullptr;
        if (PSSM) prow = p.pssm + (job.q_off + i0) * 32;
        BState D[K], V[K];
#pragma unroll
        for (int c = 0; c < K; ++c) {
            if (!PSSM) qrow[c] = i0 + c < lq ? (uint32_t)p.query[job.q_off + i0 + c] * 32u : 0u;
            D[c].v = 0, D[c].org = i0 + c + 1, D[c].st = 1;
            V[c].v = edge, V[c].org = i0 + c + 1, V[c].st = 1;
        }
        BState inD = {0, i0, 1};   // D of (row above, column i0): from the left lane, a step late
        BState Lout = {edge, i0 + K, 1}; // the left reduction of this lane's last column: the right lane's B
        int best = 0;
        uint32_t bpos = ~0u, borg = 0, bst = 0; // bpos = row << 12 | column: the smaller the better

        // residue of the row this lane works at step 0, then one step ahead
        uint32_t dcur = lane == 0 ? (uint32_t)d[0] >> 3 : 0u;
        for (uint32_t t = 0; t < steps; ++t) {
            const uint32_t j = t - lane + 1; // (wraps below row 1: then it is above len)
            const bool active = j - 1 < len;
            const uint32_t jnext = j + 1;
            uint32_t dnext = 0;
            if (jnext - 1 < len) dnext = (uint32_t)d[jnext - 1] >> 3;
            // hand-over: the left lane's values of the step before
            BState inL, newD;
            inL.v = bounds_from_left<G>(0, Lout.v);
            inL.org = (uint32_t)bounds_from_left<G>(0, (int)Lout.org);
            inL.st = (uint32_t)bounds_from_left<G>(0, (int)Lout.st);
            newD.v = bounds_from_left<G>(0, D[K - 1].v);
            newD.org = (uint32_t)bounds_from_left<G>(0, (int)D[K - 1].org);
            newD.st = (uint32_t)bounds_from_left<G>(0, (int)D[K - 1].st);
            const uint32_t rowbits = j << SWG_BOUNDS_Q_BITS;
            if (lane == 0) { // column 0 is the border
                inL.v = edge, inL.org = rowbits, inL.st = 1;
                newD.v = 0, newD.org = rowbits, newD.st = 1;
            }
            if (active) {
                BState diag = inD, left = inL;
                const int8_t *srow = PSSM ? prow + dcur : nullptr;
#pragma unroll
                for (int c = 0; c < K; ++c) {
                    const int s = PSSM ? (int)srow[c * 32] : (int)s_sub[qrow[c] + dcur];
                    const uint32_t here = rowbits | (i0 + c + 1);
                    BState H = {diag.v + s, diag.org, diag.st};
                    const BState A = V[c], B = left;
                    diag = D[c];
                    D[c] = bounds_reduce(H.v, A.v, B.v, H, A, B, here);
                    V[c] = bounds_reduce(H.v + go, A.v + ge, B.v + go, H, A, B, here);
                    left = bounds_reduce(H.v + go, A.v + go, B.v + ge, H, A, B, here);
                    // rows, then columns, ascending: only a higher score replaces the best cell
                    if (H.v > best && i0 + c < lq) best = H.v, bpos = here, borg = H.org, bst = H.st;
                }
                Lout = left;
            }
            inD = newD;
            dcur = dnext;
        }

        // the group's best cell: highest score, then smallest database position, then smallest query position
#pragma unroll
        for (int off = G / 2; off > 0; off >>= 1) {
            const int ob = __shfl_xor(best, off, G);
            const uint32_t op = (uint32_t)__shfl_xor((int)bpos, off, G);
            const uint32_t oo = (uint32_t)__shfl_xor((int)borg, off, G);
            const uint32_t os = (uint32_t)__shfl_xor((int)bst, off, G);
            if (ob > best || (ob == best && op < bpos)) best = ob, bpos = op, borg = oo, bst = os;
        }
        if (lane == 0) {
            SwgBoundsOut o = {};
            if (best > 0) {
                o.score = best;
                o.q_end = bpos & ((1u << SWG_BOUNDS_Q_BITS) - 1), o.d_end = bpos >> SWG_BOUNDS_Q_BITS;
                o.q_begin = borg & ((1u << SWG_BOUNDS_Q_BITS) - 1), o.d_begin = borg >> SWG_BOUNDS_Q_BITS;
                o.n_ops = bst;
            }
            p.out[jn] = o;
        }
    }
}

// ---- swg_align_stats: the same forward pass with two counts more in every tag ---------------------------
// A sibling of swg_bounds_kernel, not a flag of it: the bounds instantiations keep their code objects to the instruction.
// The loop structure and the hand-over are swg_bounds_kernel's; what differs is the tag's third register `cnt` -- the
// path's identical columns so far in the low SWG_STATS_IDENT_BITS bits, its gap openings above them.
#define SWG_STATS_IDENT_BITS 12
#define SWG_STATS_OPEN (1u << SWG_STATS_IDENT_BITS) /* one gap opening */
#define SWG_STATS_NO_RESIDUE 0xffu                  /* a consensus byte no database residue (1..31) equals */
struct SState {
    int v;
    uint32_t org, st, cnt;
};

// bounds_reduce with the counts.  DIR is the direction of the step: 0 diagonal, 1 down (the neighbour's A), 2 right (its
// B).  A step down or right opens a gap run unless it continues the direction's own state (A downwards, B to the right);
// one that starts the alignment is the path's first run.
template <int DIR>
BDEVINL SState stats_reduce(int x, int y, int z, const SState &h, const SState &a, const SState &b, uint32_t here)
{
    const int m3 = max(max(x, y), z);
    SState r;
    r.v = max(m3, 0);
    uint32_t o = b.org, s = b.st;
    if (y == m3) o = a.org, s = a.st;
    if (x == m3) o = h.org, s = h.st;
    s += 1;
    if (m3 <= 0) o = here, s = 1;
    r.org = o, r.st = s;
    uint32_t n = b.cnt + (DIR == 1 ? SWG_STATS_OPEN : 0u);
    if (y == m3) n = a.cnt + (DIR == 2 ? SWG_STATS_OPEN : 0u);
    if (x == m3) n = h.cnt + (DIR != 0 ? SWG_STATS_OPEN : 0u);
    if (m3 <= 0) n = DIR != 0 ? SWG_STATS_OPEN : 0u;
    r.cnt = n;
    return r;
}

// Two more DPP moves per step, one more shuffle per round of the best-cell reduction, and the result's two pad words
// take the best cell's counts.  A border cell's vertical and left hand-overs (V[c], Lout, lane 0's inL) begin with one
// opening: a path that runs in from the border begins with a gap whichever of the border's states the maximum picks.
// A PSSM's identity is counted against its consensus residues, which the host puts where the index kernel has its
// queries (p.query).
template <int G, int K, bool PSSM>
__global__ __launch_bounds__(SWG_BOUNDS_THREADS) void swg_stats_kernel(SwgBoundsParams p)
{
    __shared__ int8_t s_sub[1024];
    if (!PSSM)
        for (uint32_t k = threadIdx.x; k < 1024; k += SWG_BOUNDS_THREADS) s_sub[k] = p.sub[k];
    __syncthreads(); // (the only one: before any group takes a job)
    const uint32_t lane = threadIdx.x & (G - 1);
    uint32_t group = (blockIdx.x * SWG_BOUNDS_THREADS + threadIdx.x) / G;
    if (G == 64) group = (uint32_t)__builtin_amdgcn_readfirstlane((int)group); // a whole wavefront: job fields in SGPRs
    if (group >= p.n_groups) return;
    const int go = p.go, ge = p.ge;
    const int edge = max(max(go, ge), 0); // what a border cell hands down and to the right
    const uint32_t i0 = lane * K;         // columns i0 + 1 .. i0 + K (from 1, as the rows)

    for (uint32_t jn = group; jn < p.n_jobs; jn += p.n_groups) {
        const SwgBoundsJob job = p.jobs[jn];
        const uint32_t lq = job.lq, len = job.len;
        const uint8_t *d = p.codes + job.res_off;
        const uint32_t steps = len + (lq + K - 1) / K - 1; // lanes past the query's last column are not waited for

        // this lane's columns: their score rows, and the two reductions kept per column -- D: the diagonal one of
        // the row above (what column c + 1 continues), V: the vertical one (this column's own A).  Row 0 is the border.
        uint32_t qrow[K];
        uint32_t cons[K / 4]; // PSSM: the columns' consensus residues, four to a register
        const int8_t *prow = nullptr;
        if (PSSM) prow = p.pssm + (job.q_off + i0) * 32;
        SState D[K], V[K];
#pragma unroll
        for (int c = 0; c < K; ++c) {
            if (!PSSM) qrow[c] = i0 + c < lq ? (uint32_t)p.query[job.q_off + i0 + c] * 32u : 0u;
            if (PSSM) {
                const uint32_t r = i0 + c < lq ? (uint32_t)(uint8_t)p.query[job.q_off + i0 + c] : SWG_STATS_NO_RESIDUE;
                cons[c / 4] = c % 4 == 0 ? r : cons[c / 4] | r << (c % 4 * 8);
            }
            D[c].v = 0, D[c].org = i0 + c + 1, D[c].st = 1, D[c].cnt = 0;
            V[c].v = edge, V[c].org = i0 + c + 1, V[c].st = 1, V[c].cnt = SWG_STATS_OPEN;
        }
        SState inD = {0, i0, 1, 0};   // D of (row above, column i0): from the left lane, a step late
        SState Lout = {edge, i0 + K, 1, SWG_STATS_OPEN}; // the left reduction of this lane's last column: the right lane's B
        int best = 0;
        uint32_t bpos = ~0u, borg = 0, bst = 0, bcnt = 0; // bpos = row << 12 | column: the smaller the better

        // residue of the row this lane works at step 0, then one step ahead
        uint32_t dcur = lane == 0 ? (uint32_t)d[0] >> 3 : 0u;
        for (uint32_t t = 0; t < steps; ++t) {
            const uint32_t j = t - lane + 1; // (wraps below row 1: then it is above len)
            const bool active = j - 1 < len;
            const uint32_t jnext = j + 1;
            uint32_t dnext = 0;
            if (jnext - 1 < len) dnext = (uint32_t)d[jnext - 1] >> 3;
            // hand-over: the left lane's values of the step before
            SState inL, newD;
            inL.v = bounds_from_left<G>(0, Lout.v);
            inL.org = (uint32_t)bounds_from_left<G>(0, (int)Lout.org);
            inL.st = (uint32_t)bounds_from_left<G>(0, (int)Lout.st);
            newD.v = bounds_from_left<G>(0, D[K - 1].v);
            newD.org = (uint32_t)bounds_from_left<G>(0, (int)D[K - 1].org);
            newD.st = (uint32_t)bounds_from_left<G>(0, (int)D[K - 1].st);
            inL.cnt = (uint32_t)bounds_from_left<G>(0, (int)Lout.cnt);
            newD.cnt = (uint32_t)bounds_from_left<G>(0, (int)D[K - 1].cnt);
            const uint32_t rowbits = j << SWG_BOUNDS_Q_BITS;
            if (lane == 0) { // column 0 is the border
                inL.v = edge, inL.org = rowbits, inL.st = 1, inL.cnt = SWG_STATS_OPEN;
                newD.v = 0, newD.org = rowbits, newD.st = 1, newD.cnt = 0;
            }
            if (active) {
                SState diag = inD, left = inL;
                const int8_t *srow = PSSM ? prow + dcur : nullptr;
#pragma unroll
                for (int c = 0; c < K; ++c) {
                    const int s = PSSM ? (int)srow[c * 32] : (int)s_sub[qrow[c] + dcur];
                    const uint32_t here = rowbits | (i0 + c + 1);
                    SState H = {diag.v + s, diag.org, diag.st, diag.cnt};
                    // (a padding column has qrow 0 or no residue: it never matches)
                    H.cnt += PSSM ? ((cons[c / 4] >> (c % 4 * 8)) & 0xffu) == dcur : qrow[c] == dcur * 32u;
                    const SState A = V[c], B = left;
                    diag = D[c];
                    D[c] = stats_reduce<0>(H.v, A.v, B.v, H, A, B, here);
                    V[c] = stats_reduce<1>(H.v + go, A.v + ge, B.v + go, H, A, B, here);
                    left = stats_reduce<2>(H.v + go, A.v + go, B.v + ge, H, A, B, here);
                    // rows, then columns, ascending: only a higher score replaces the best cell
                    if (H.v > best && i0 + c < lq) best = H.v, bpos = here, borg = H.org, bst = H.st, bcnt = H.cnt;
                }
                Lout = left;
            }
            inD = newD;
            dcur = dnext;
        }

        // the group's best cell: highest score, then smallest database position, then smallest query position
#pragma unroll
        for (int off = G / 2; off > 0; off >>= 1) {
            const int ob = __shfl_xor(best, off, G);
            const uint32_t op = (uint32_t)__shfl_xor((int)bpos, off, G);
            const uint32_t oo = (uint32_t)__shfl_xor((int)borg, off, G);
            const uint32_t os = (uint32_t)__shfl_xor((int)bst, off, G);
            const uint32_t oc = (uint32_t)__shfl_xor((int)bcnt, off, G);
            if (ob > best || (ob == best && op < bpos)) best = ob, bpos = op, borg = oo, bst = os, bcnt = oc;
        }
        if (lane == 0) {
            SwgBoundsOut o = {};
            if (best > 0) {
                o.score = best;
                o.q_end = bpos & ((1u << SWG_BOUNDS_Q_BITS) - 1), o.d_end = bpos >> SWG_BOUNDS_Q_BITS;
                o.q_begin = borg & ((1u << SWG_BOUNDS_Q_BITS) - 1), o.d_begin = borg >> SWG_BOUNDS_Q_BITS;
                o.n_ops = bst;
                o.pad[0] = bcnt & (SWG_STATS_OPEN - 1), o.pad[1] = bcnt >> SWG_STATS_IDENT_BITS;
            }
            p.out[jn] = o;
        }
    }
}

// The instantiations, narrowest first: a query goes to the first whose G * K columns hold it.
struct BoundsClass {
    int G, K;
};
static const BoundsClass kBoundsClasses[] = {{16, 4}, {16, 8}, {32, 8}, {64, 8}, {64, 16}};
#define SWG_BOUNDS_CLASSES 5
static_assert(64 * 16 == SWG_BOUNDS_COLS, "the widest instantiation is the column limit");
static_assert(SWG_BOUNDS_COLS < (1u << SWG_BOUNDS_Q_BITS) && SWG_BOUNDS_LEN <= (1u << (32 - SWG_BOUNDS_Q_BITS)),
              "a tag's origins share one register");
// identical columns <= the query's columns; openings <= 2 * columns + 1 (every D run takes a column, and two I runs are
// separated by an M or a D)
static_assert(SWG_BOUNDS_COLS < (1u << SWG_STATS_IDENT_BITS) && 2 * SWG_BOUNDS_COLS + 1 < (1u << (32 - SWG_STATS_IDENT_BITS)),
              "a tag's two counts share one register");

static int bounds_class(uint32_t lq)
{
    for (int c = 0; c < SWG_BOUNDS_CLASSES; ++c)
        if (lq <= (uint32_t)(kBoundsClasses[c].G * kBoundsClasses[c].K)) return c;
    return -1;
}

template <int G, int K>
static void bounds_launch_gk(bool pssm, bool stats, unsigned blocks, hipStream_t s, const SwgBoundsParams &p)
{
    if (stats && pssm) hipLaunchKernelGGL((swg_stats_kernel<G, K, true>), dim3(blocks), dim3(SWG_BOUNDS_THREADS), 0, s, p);
    else if (stats) hipLaunchKernelGGL((swg_stats_kernel<G, K, false>), dim3(blocks), dim3(SWG_BOUNDS_THREADS), 0, s, p);
    else if (pssm) hipLaunchKernelGGL((swg_bounds_kernel<G, K, true>), dim3(blocks), dim3(SWG_BOUNDS_THREADS), 0, s, p);
    else hipLaunchKernelGGL((swg_bounds_kernel<G, K, false>), dim3(blocks), dim3(SWG_BOUNDS_THREADS), 0, s, p);
}

static void bounds_launch(int cls, bool pssm, bool stats, unsigned blocks, hipStream_t s, const SwgBoundsParams &p)
{
    switch (cls) {
    case 0: bounds_launch_gk<16, 4>(pssm, stats, blocks, s, p); break;
    case 1: bounds_launch_gk<16, 8>(pssm, stats, blocks, s, p); break;
    case 2: bounds_launch_gk<32, 8>(pssm, stats, blocks, s, p); break;
    case 3: bounds_launch_gk<64, 8>(pssm, stats, blocks, s, p); break;
    default: bounds_launch_gk<64, 16>(pssm, stats, blocks, s, p); break;
    }
}

#define BOUNDS_TRY(ctx, expr)                                                                           \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess) {                                                                         \
            rc = swg_set_ctx_error(ctx, e_ == hipErrorOutOfMemory ? SWG_ERR_NOMEM : SWG_ERR_HIP,        \
                                   "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            goto done;                                                                                  \
        }                                                                                               \
    } while (0)

// A PSSM's consensus (swg.h, swg_align_stats): per position the lowest residue index in 1..31 whose score is the row's
// maximum over 1..31.
static void stats_consensus(const int8_t *rows, size_t positions, uint8_t *out)
{
    for (size_t r = 0; r < positions; ++r) {
        int at = 1;
        for (int b = 2; b < 32; ++b)
            if (rows[r * 32 + b] > rows[r * 32 + at]) at = b;
        out[r] = (uint8_t)at;
    }
}

// The four counts of one result: the two the forward pass (or the walk) carried, the other two from the coordinates --
// every M takes a query column and a residue, every I or D one of the two.
static swg_align_counts stats_counts(const swg_alignment &a, uint32_t ident, uint32_t opens)
{
    swg_align_counts c;
    c.n_ident = ident, c.n_gap_open = opens;
    c.n_match = (a.q_end - a.q_begin) + (a.d_end - a.d_begin) - a.n_ops;
    c.n_gap = a.n_ops - c.n_match;
    return c;
}

// The counts of a path the traceback spelled (the stats calls' fallback pairs): q = the query's residues from the
// path's first column (a PSSM's consensus), d = the sequence's residue bytes (index << 3) from its first row.
static swg_align_counts stats_from_ops(const swg_alignment &a, const char *ops, const uint8_t *q, const uint8_t *d)
{
    uint32_t ident = 0, opens = 0;
    size_t qi = 0, di = 0;
    for (uint32_t n = 0; n < a.n_ops; ++n) {
        if (ops[n] == 'M') ident += q[qi++] == (uint8_t)(d[di++] >> 3);
        else {
            opens += n == 0 || ops[n - 1] != ops[n];
            ops[n] == 'I' ? ++di : ++qi;
        }
    }
    return stats_counts(a, ident, opens);
}

// Every hit of a checked batch (total > 0 hits).  The pairs the kernel holds are ordered by instantiation and, within
// one, longest first; one device buffer holds the job records, the queries and the results; one launch per
// instantiation that has pairs, then one copy back and one stream synchronisation for the call.  The rest of the pairs
// goes through the traceback's kernel without paths.  counts != NULL (the stats calls): the stats kernel, a PSSM
// batch's consensus uploaded behind its rows, and the rest of the pairs through the traceback's kernel with their
// paths, which are counted here.
static int bounds_batch(swg_ctx *ctx, const swg_db *db, const SwgTraceBatch &tb, size_t total, swg_alignment *out,
                        swg_align_counts *counts)
{
    const char *fn = tb.fn;
    // original index -> slot of the sorted order
    std::vector<uint32_t> slot_of(db->n_total, ~0u);
    for (size_t s = 0; s < db->order.size(); ++s)
        if (db->order[s] < db->n_total) slot_of[db->order[s]] = (uint32_t)s;
    struct Pair {
        SwgBoundsJob job;
        size_t dest;
        int cls;
    };
    std::vector<Pair> pairs;
    pairs.reserve(total);
    std::vector<swg_hit> fb_hits;   // the fallback's rows: the batch's layout, its pairs moved to the front of each row
    std::vector<size_t> fb_n, fb_dest;
    size_t fb_total = 0;
    for (size_t i = 0; i < tb.n_queries; ++i) {
        const size_t lq = (size_t)(tb.q_offsets[i + 1] - tb.q_offsets[i]);
        const int cls = bounds_class((uint32_t)std::min<size_t>(lq, SWG_BOUNDS_COLS + 1));
        for (size_t j = 0; j < tb.n_hits[i]; ++j) {
            const uint32_t index = tb.hits[i * tb.k + j].index;
            const uint32_t s = index < db->n_total ? slot_of[index] : ~0u;
            if (s == ~0u)
                return swg_set_ctx_error(ctx, SWG_ERR_ARG, "%s: sequence %u is not in this database shard", fn, index);
            const size_t len = db->lens[s];
            const uint64_t cells = (uint64_t)(lq + len) * lq;
            if (len == 0 || cells > (16ull << 30))
                return swg_set_ctx_error(ctx, SWG_ERR_ARG, "%s: pair %u (%zu x %zu) is outside what a traceback holds", fn,
                                         index, lq, len);
            if (cls < 0 || len >= SWG_BOUNDS_LEN) {
                if (fb_hits.empty()) fb_hits.resize(tb.n_queries * tb.k), fb_n.assign(tb.n_queries, 0), fb_dest.resize(tb.n_queries * tb.k);
                fb_hits[i * tb.k + fb_n[i]] = tb.hits[i * tb.k + j];
                fb_dest[i * tb.k + fb_n[i]] = i * tb.k + j;
                ++fb_n[i], ++fb_total;
                continue;
            }
            Pair pr = {};
            pr.job.q_off = tb.q_offsets[i] - tb.q_offsets[0];
            pr.job.res_off = db->code_off[s];
            pr.job.lq = (uint32_t)lq, pr.job.len = (uint32_t)len;
            pr.dest = i * tb.k + j, pr.cls = cls;
            pairs.push_back(pr);
        }
    }
    const size_t n = pairs.size();
    std::stable_sort(pairs.begin(), pairs.end(), [](const Pair &a, const Pair &b) {
        if (a.cls != b.cls) return a.cls < b.cls;
        return (uint64_t)a.job.len + a.job.lq > (uint64_t)b.job.len + b.job.lq;
    });

    int rc = SWG_OK;
    uint32_t launches = 0;
    uint8_t *d_buf = nullptr;
    const size_t row_bytes = tb.pssm ? 32 : 1;
    const size_t positions = (size_t)(tb.q_offsets[tb.n_queries] - tb.q_offsets[0]);
    std::vector<uint8_t> h_cons; // a PSSM batch's consensus residues, position by position
    if (counts && tb.pssm) {
        h_cons.resize(positions);
        stats_consensus(tb.src + tb.q_offsets[0] * 32, positions, h_cons.data());
    }
    if (n > 0) {
        const size_t q_bytes = positions * row_bytes;
        // the lanes past a PSSM's last column read rows behind it: slack for the widest group
        const size_t q_room = (q_bytes + (tb.pssm ? (size_t)SWG_BOUNDS_COLS * 32 : 0) + 255) / 256 * 256;
        const size_t jobs_bytes = (n * sizeof(SwgBoundsJob) + 255) / 256 * 256;
        const size_t cons_off = jobs_bytes + q_room, cons_room = (h_cons.size() + 255) / 256 * 256;
        const size_t up_bytes = jobs_bytes + q_bytes, out_off = cons_off + cons_room;
        std::vector<uint8_t> h_up(up_bytes, 0);
        for (size_t h = 0; h < n; ++h) memcpy(h_up.data() + h * sizeof(SwgBoundsJob), &pairs[h].job, sizeof(SwgBoundsJob));
        memcpy(h_up.data() + jobs_bytes, tb.src + tb.q_offsets[0] * row_bytes, q_bytes);
        std::vector<SwgBoundsOut> h_out(n);
        BOUNDS_TRY(ctx, hipSetDevice(ctx->device));
        BOUNDS_TRY(ctx, hipMalloc(&d_buf, out_off + n * sizeof(SwgBoundsOut)));
        BOUNDS_TRY(ctx, hipMemcpyAsync(d_buf, h_up.data(), up_bytes, hipMemcpyHostToDevice, ctx->stream));
        if (!h_cons.empty())
            BOUNDS_TRY(ctx, hipMemcpyAsync(d_buf + cons_off, h_cons.data(), h_cons.size(), hipMemcpyHostToDevice, ctx->stream));
        for (size_t b = 0; b < n;) {
            size_t e = b;
            while (e < n && pairs[e].cls == pairs[b].cls) ++e;
            const BoundsClass &bc = kBoundsClasses[pairs[b].cls];
            const size_t per_block = SWG_BOUNDS_THREADS / bc.G;
            size_t groups = std::min<size_t>(e - b, (size_t)std::max(ctx->n_cu, 1) * 8 * per_block);
            if (ctx->opt_bounds_groups > 0) groups = std::min<size_t>(groups, (size_t)ctx->opt_bounds_groups);
            SwgBoundsParams p;
            p.query = reinterpret_cast<const int8_t *>(d_buf + jobs_bytes), p.pssm = p.query;
            if (!h_cons.empty()) p.query = reinterpret_cast<const int8_t *>(d_buf + cons_off);
            p.sub = ctx->d_sub; // (uploaded by swg_set_scoring on this stream)
            p.codes = reinterpret_cast<const uint8_t *>(db->d_codes);
            p.jobs = reinterpret_cast<const SwgBoundsJob *>(d_buf) + b;
            p.out = reinterpret_cast<SwgBoundsOut *>(d_buf + out_off) + b;
            p.n_jobs = (uint32_t)(e - b), p.n_groups = (uint32_t)groups;
            p.go = ctx->gap_open + ctx->gap_extend, p.ge = ctx->gap_extend; // src/alignment.c:58-59
            bounds_launch(pairs[b].cls, tb.pssm, counts != nullptr, (unsigned)((groups + per_block - 1) / per_block), ctx->stream, p);
            BOUNDS_TRY(ctx, hipGetLastError());
            ++launches;
            b = e;
        }
        BOUNDS_TRY(ctx, hipMemcpyAsync(h_out.data(), d_buf + out_off, n * sizeof(SwgBoundsOut), hipMemcpyDeviceToHost, ctx->stream));
        BOUNDS_TRY(ctx, hipStreamSynchronize(ctx->stream));
        for (size_t h = 0; h < n; ++h) {
            const SwgBoundsOut &o = h_out[h];
            swg_alignment &a = out[pairs[h].dest];
            a.score = o.score, a.index = tb.hits[pairs[h].dest].index;
            a.q_begin = o.q_begin, a.q_end = o.q_end, a.d_begin = o.d_begin, a.d_end = o.d_end;
            a.n_ops = o.n_ops, a.reserved = 0;
            if (counts) counts[pairs[h].dest] = stats_counts(a, o.pad[0], o.pad[1]);
        }
    }
done:
    (void)hipFree(d_buf);
    if (rc != SWG_OK) return rc;
    if (fb_total > 0 && !counts) {
        std::vector<swg_alignment> fb_out(tb.n_queries * tb.k);
        SwgTraceBatch fb = tb;
        fb.hits = fb_hits.data(), fb.n_hits = fb_n.data();
        rc = swg_trace_align_batch(ctx, db, fb, fb_total, fb_out.data(), nullptr, 0);
        if (rc != SWG_OK) return rc;
        for (size_t i = 0; i < tb.n_queries; ++i)
            for (size_t j = 0; j < fb_n[i]; ++j) out[fb_dest[i * tb.k + j]] = fb_out[i * tb.k + j];
    }
    // The stats calls' fallback pairs come back with their paths: runs of consecutive queries, each run's rows as wide as
    // its fullest and its paths kept to about 256 MB (a query whose own paths are more goes alone).
    for (size_t qa = 0; fb_total > 0 && counts && qa < tb.n_queries;) {
        if (fb_n[qa] == 0) {
            ++qa;
            continue;
        }
        size_t qb = qa, kf = 0, stride = 0, run_total = 0;
        for (; qb < tb.n_queries; ++qb) {
            size_t k2 = std::max(kf, fb_n[qb]), s2 = stride;
            const size_t lq = (size_t)(tb.q_offsets[qb + 1] - tb.q_offsets[qb]);
            for (size_t j = 0; j < fb_n[qb]; ++j)
                s2 = std::max(s2, lq + db->lens[slot_of[fb_hits[qb * tb.k + j].index]] + 1);
            if (qb > qa && (qb - qa + 1) * k2 * s2 > ((size_t)256 << 20)) break;
            kf = k2, stride = s2, run_total += fb_n[qb];
        }
        const size_t nq = qb - qa;
        std::vector<swg_hit> r_hits(nq * kf);
        std::vector<swg_alignment> r_out(nq * kf);
        std::vector<char> r_ops(nq * kf * stride);
        for (size_t i = 0; i < nq; ++i)
            for (size_t j = 0; j < fb_n[qa + i]; ++j) r_hits[i * kf + j] = fb_hits[(qa + i) * tb.k + j];
        SwgTraceBatch fb = tb;
        fb.q_offsets = tb.q_offsets + qa, fb.n_queries = nq, fb.hits = r_hits.data(), fb.k = kf, fb.n_hits = fb_n.data() + qa;
        rc = swg_trace_align_batch(ctx, db, fb, run_total, r_out.data(), r_ops.data(), stride);
        if (rc != SWG_OK) return rc;
        for (size_t i = 0; i < nq; ++i)
            for (size_t j = 0; j < fb_n[qa + i]; ++j) {
                const swg_alignment &a = r_out[i * kf + j];
                const size_t dest = fb_dest[(qa + i) * tb.k + j];
                const size_t q_at = (size_t)(tb.q_offsets[qa + i] - tb.q_offsets[0]) + a.q_begin;
                const uint8_t *q = tb.pssm ? h_cons.data() + q_at
                                           : reinterpret_cast<const uint8_t *>(tb.src) + tb.q_offsets[0] + q_at;
                const uint8_t *d = swg_db_codes(db) + db->code_off[slot_of[a.index]] + a.d_begin;
                out[dest] = a;
                counts[dest] = stats_from_ops(a, r_ops.data() + (i * kf + j) * stride, q, d);
            }
        qa = qb;
    }
    ctx->bounds_last[0] = (uint32_t)n, ctx->bounds_last[1] = (uint32_t)fb_total, ctx->bounds_last[2] = launches;
    ctx->bounds_last[3] = SWG_BOUNDS_COLS;
    return SWG_OK;
}

// try/catch: no C++ exception crosses the ABI (the host vectors are sized by the batch and by the database)
static int bounds_checked(swg_ctx *ctx, const swg_db *db, const SwgTraceBatch &tb, swg_alignment *out,
                          swg_align_counts *counts = nullptr, bool stats = false)
{
    size_t total = 0;
    const int rc = swg_trace_check_batch(ctx, db, tb, out, false, &total);
    if (rc != SWG_OK) return rc;
    if (stats && total > 0 && !counts) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "%s: NULL argument", tb.fn);
    ctx->bounds_last[0] = ctx->bounds_last[1] = ctx->bounds_last[2] = 0, ctx->bounds_last[3] = SWG_BOUNDS_COLS;
    if (total == 0) return SWG_OK;
    try {
        return bounds_batch(ctx, db, tb, total, out, counts);
    } catch (const std::bad_alloc &) {
        return swg_set_ctx_error(ctx, SWG_ERR_NOMEM, "%s: out of host memory", tb.fn);
    } catch (const std::exception &e) {
        return swg_set_ctx_error(ctx, SWG_ERR_NOMEM, "%s: %s", tb.fn, e.what());
    }
}

extern "C" int swg_align_bounds(swg_ctx *ctx, const swg_db *db, const swg_hit *hits, size_t n_hits, swg_alignment *out)
{
    if (!ctx) return swg_set_global_error(SWG_ERR_ARG, "swg_align_bounds: NULL context");
    if (!db || (n_hits && (!hits || !out)))
        return swg_set_ctx_error(ctx, SWG_ERR_ARG, "swg_align_bounds: NULL argument");
    if (!ctx->have_scoring || ctx->query_len() == 0)
        return swg_set_ctx_error(ctx, SWG_ERR_STATE, "swg_align_bounds: scoring and query must be set first");
    const uint64_t q_offsets[2] = {0, ctx->query_len()};
    const SwgTraceBatch tb = {"swg_align_bounds", ctx->query_pssm ? ctx->pssm.data() : ctx->query.data(), ctx->query_pssm,
                              q_offsets, 1, hits, n_hits, &n_hits};
    return bounds_checked(ctx, db, tb, out);
}

extern "C" int swg_align_bounds_multi(swg_ctx *ctx, const swg_db *db, const int8_t *queries, const uint64_t *q_offsets,
                                      size_t n_queries, const swg_hit *hits, size_t k, const size_t *n_hits,
                                      swg_alignment *out)
{
    const SwgTraceBatch tb = {"swg_align_bounds_multi", queries, false, q_offsets, n_queries, hits, k, n_hits};
    return bounds_checked(ctx, db, tb, out);
}

extern "C" int swg_align_bounds_multi_pssm(swg_ctx *ctx, const swg_db *db, const int8_t *pssms, const uint64_t *q_offsets,
                                           size_t n_queries, const swg_hit *hits, size_t k, const size_t *n_hits,
                                           swg_alignment *out)
{
    const SwgTraceBatch tb = {"swg_align_bounds_multi_pssm", pssms, true, q_offsets, n_queries, hits, k, n_hits};
    return bounds_checked(ctx, db, tb, out);
}

// The stats calls: the bounds calls' arguments plus the counts (swg.h).
extern "C" int swg_align_stats(swg_ctx *ctx, const swg_db *db, const swg_hit *hits, size_t n_hits, swg_alignment *out,
                               swg_align_counts *counts)
{
    if (!ctx) return swg_set_global_error(SWG_ERR_ARG, "swg_align_stats: NULL context");
    if (!db || (n_hits && (!hits || !out || !counts)))
        return swg_set_ctx_error(ctx, SWG_ERR_ARG, "swg_align_stats: NULL argument");
    if (!ctx->have_scoring || ctx->query_len() == 0)
        return swg_set_ctx_error(ctx, SWG_ERR_STATE, "swg_align_stats: scoring and query must be set first");
    const uint64_t q_offsets[2] = {0, ctx->query_len()};
    const SwgTraceBatch tb = {"swg_align_stats", ctx->query_pssm ? ctx->pssm.data() : ctx->query.data(), ctx->query_pssm,
                              q_offsets, 1, hits, n_hits, &n_hits};
    return bounds_checked(ctx, db, tb, out, counts, true);
}

extern "C" int swg_align_stats_multi(swg_ctx *ctx, const swg_db *db, const int8_t *queries, const uint64_t *q_offsets,
                                     size_t n_queries, const swg_hit *hits, size_t k, const size_t *n_hits,
                                     swg_alignment *out, swg_align_counts *counts)
{
    const SwgTraceBatch tb = {"swg_align_stats_multi", queries, false, q_offsets, n_queries, hits, k, n_hits};
    return bounds_checked(ctx, db, tb, out, counts, true);
}

extern "C" int swg_align_stats_multi_pssm(swg_ctx *ctx, const swg_db *db, const int8_t *pssms, const uint64_t *q_offsets,
                                          size_t n_queries, const swg_hit *hits, size_t k, const size_t *n_hits,
                                          swg_alignment *out, swg_align_counts *counts)
{
    const SwgTraceBatch tb = {"swg_align_stats_multi_pssm", pssms, true, q_offsets, n_queries, hits, k, n_hits};
    return bounds_checked(ctx, db, tb, out, counts, true);
}

extern "C" int swg_debug_bounds_last(const swg_ctx *ctx, uint32_t out[4])
{
    if (!ctx || !out) return swg_set_global_error(SWG_ERR_ARG, "swg_debug_bounds_last: NULL argument");
    for (int i = 0; i < 4; ++i) out[i] = ctx->bounds_last[i];
    return SWG_OK;
}
