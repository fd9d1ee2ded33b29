// swg_comp.hip -- composition-based score adjustment of reported hits (swg_comp_adjust*, include/swg.h).
//
// Three kernels on the context's stream, then one copy back:
//   swg_comp_counts_kernel  one workgroup per query: the count table C[a][s] (how many positions score residue a with s),
//                           32 x 256 words, built in LDS by integer atomics -- the counts do not depend on their order.
//   swg_comp_stat_kernel    one workgroup per pair: the 32-bin composition of the hit's residues, read from the resident
//                           bytes where they lie; h[s] in 64-bit integers, one s per thread; lambda_hit by the iteration of
//                           swg_comp_rule.h, every thread carrying the same lambda through the same steps, the two sums of
//                           a step reduced in a fixed order; ratio16, status and the pair's 256-entry table T.
//   swg_comp_fill_kernel    a score-only sibling of swg_bounds_kernel (swg_bounds.hip): one lane group of G lanes per pair,
//                           K consecutive columns per lane in registers, DPP hand-over between lanes, no barrier in the row
//                           loop, pairs dealt longest first.  Without tags a state is one register where the bounds kernel's
//                           is three, which is what lets the widest instantiation hold 32 columns per lane.
// Every score of a pair goes through the PAIR's table.  Index queries: T is applied once per pair, into a per-group
// int16 copy of the substitution table in LDS (TS[r][a] = T[sub[r][a]], 2 KB: 1024 / G look-ups per lane and pair), so a
// cell costs the one LDS read it costs the bounds kernel.  A PSSM has no table to compose with -- its per-group int16
// profile would be 64 bytes a column, 128 KB for the widest group -- so there T itself lies in LDS per group (512 bytes)
// and is applied per cell, behind the row's byte from global memory.
// A group's table is written and read by lanes of one wavefront only (G <= 64), whose LDS operations complete in
// program order: a wavefront-scope fence on either side of the build is all that orders them.
#include "swg_host_internal.h"
#include "swg_comp_rule.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <stdexcept>

int swg_pssm_background(const char *fn, const double *freq, double P[32], uint32_t *mask); // swg_pssm_host.cpp

struct SwgCompJob {
    uint64_t q_off;   // into the batch's queries: first index byte, or first PSSM row
    uint64_t res_off; // the sequence's first byte among the resident residue bytes (index << 3 each)
    uint32_t lq;      // query length
    uint32_t len;     // database sequence length
    uint32_t cq;      // the query's place among the call's queries that have hits: its count table, lambda_std and status
    uint32_t pad;
};

struct SwgCompQuery {
    uint64_t q_off; // as a job's
    uint32_t lq, std_status;
    double lambda_std;
};

static_assert(sizeof(swg_comp_result) == 24, "the kernels write the public record");

struct SwgCompParams {
    const int8_t *query;  // table indices of the batch's queries, back to back (PSSM kernels: unread)
    const int8_t *sub;    // [32][32], row = query residue (PSSM kernels: unread)
    const int8_t *pssm;   // PSSM kernels: the batch's rows [positions][32], SWG_COMP_COLS rows of slack behind them
    const uint8_t *codes; // the resident database's residue bytes
    const SwgCompQuery *queries;
    const SwgCompJob *jobs;
    uint32_t *counts;     // [queries][32][256]
    int16_t *T;           // [jobs][256]
    swg_comp_result *out; // [jobs]
    uint32_t n_jobs, n_groups, mask;
    int go, ge, F;        // the gap scores already times F
};

#define SWG_COMP_THREADS 256
#define CDEVINL __device__ __forceinline__

// ---- 1. the count tables ----------------------------------------------------------------------------------------------
template <bool PSSM> __global__ __launch_bounds__(SWG_COMP_THREADS) void swg_comp_counts_kernel(SwgCompParams p)
{
    __shared__ uint32_t C[32 * 256];
    __shared__ uint32_t cnt[32];
    const uint32_t t = threadIdx.x;
    const SwgCompQuery q = p.queries[blockIdx.x];
    for (uint32_t k = t; k < 32u * 256u; k += SWG_COMP_THREADS) C[k] = 0u;
    if (t < 32u) cnt[t] = 0u;
    __syncthreads();
    if (PSSM) {
        const int8_t *rows = p.pssm + q.q_off * 32;
        for (uint64_t k = t; k < (uint64_t)q.lq * 32u; k += SWG_COMP_THREADS)
            atomicAdd(&C[(uint32_t)(k & 31u) * 256u + (uint32_t)((int)rows[k] + 128)], 1u);
    } else {
        // the query's residues first: position p scores residue a with sub[q_p][a], so a residue seen n times adds n
        for (uint32_t k = t; k < q.lq; k += SWG_COMP_THREADS) atomicAdd(&cnt[(uint32_t)p.query[q.q_off + k] & 31u], 1u);
        __syncthreads();
        for (uint32_t k = t; k < 1024u; k += SWG_COMP_THREADS)
            if (cnt[k >> 5] != 0u) atomicAdd(&C[(k & 31u) * 256u + (uint32_t)((int)p.sub[k] + 128)], cnt[k >> 5]);
    }
    __syncthreads();
    uint32_t *dst = p.counts + (size_t)blockIdx.x * (32u * 256u);
    for (uint32_t k = t; k < 32u * 256u; k += SWG_COMP_THREADS) dst[k] = C[k];
}

// ---- 2. the statistic of a pair ---------------------------------------------------------------------------------------
// Two sums over the workgroup's 256 threads at once, each in a fixed order -- its wavefront's butterfly, then the four
// wavefronts' sums left to right --, the same in every thread (calib_block_sum3 of swg_calib.hip, for two).
template <class T> __device__ static void comp_block_sum2(T v[2], T (*part)[4])
{
#pragma unroll
    for (int k = 0; k < 2; ++k) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v[k] += __shfl_xor(v[k], d, 64);
    }
    __syncthreads();
    if ((threadIdx.x & 63u) == 0u)
        for (int k = 0; k < 2; ++k) part[k][threadIdx.x >> 6] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 2; ++k) v[k] = ((part[k][0] + part[k][1]) + part[k][2]) + part[k][3];
}

__global__ __launch_bounds__(SWG_COMP_THREADS) void swg_comp_stat_kernel(SwgCompParams p)
{
#pragma clang fp contract(off)
    __shared__ uint32_t hist[32];
    __shared__ double part[2][4];
    __shared__ long long part_i[2][4];
    __shared__ int s_smax;
    const uint32_t t = threadIdx.x;
    const SwgCompJob job = p.jobs[blockIdx.x];
    const SwgCompQuery q = p.queries[job.cq];
    const uint8_t *d = p.codes + job.res_off;
    if (t < 32u) hist[t] = 0u;
    if (t == 0u) s_smax = -129;
    __syncthreads();
    for (uint32_t j = t; j < job.len; j += SWG_COMP_THREADS) atomicAdd(&hist[(uint32_t)d[j] >> 3], 1u);
    __syncthreads();
    // thread t owns the score t - 128: h = sum_{a in A} c_a C[a][s], exact
    const uint32_t *C = p.counts + (size_t)job.cq * (32u * 256u);
    unsigned long long n = 0ull, h = 0ull;
    for (uint32_t a = 1; a < 32u; ++a) {
        if (!(p.mask >> a & 1u)) continue;
        n += hist[a];
        h += (unsigned long long)hist[a] * C[a * 256u + t];
    }
    const int sv = (int)t - 128;
    long long m[2] = {(long long)sv * (long long)h, 0ll}; // sum_s s h[s] (below 2^63: swg_comp_pair_fits bounds n lq)
    if (h != 0ull) atomicMax(&s_smax, sv);
    comp_block_sum2(m, part_i); // (its barriers also publish s_smax)
    const int smax = s_smax;
    swg_comp_result r;
    r.adj_score = 0, r.scaled_score = 0, r.ratio16 = 65536u, r.status = 1, r.lambda_hit = 0.0;
    if (n != 0ull && q.std_status != 0u) r.status = (int32_t)q.std_status;
    if (n != 0ull && q.std_status == 0u && m[0] < 0ll && smax > 0) { // (the same in every thread)
        const double w = (double)h, W = (double)n * (double)q.lq;
        double lam = 0.0;
        int iters;
        r.status = swg_comp_solve(
            [&](double l, double *f, double *df) {
                double v[2] = {0.0, 0.0};
                if (h != 0ull) {
                    v[0] = w * exp(l * (double)sv);
                    v[1] = (double)sv * v[0];
                }
                comp_block_sum2(v, part);
                *f = v[0], *df = v[1];
            },
            W, smax, &lam, &iters);
        if (r.status == 0) r.lambda_hit = lam, r.ratio16 = swg_comp_ratio16(lam, q.lambda_std);
    }
    p.T[(size_t)blockIdx.x * 256u + t] = swg_comp_rescale(sv, p.F, r.ratio16);
    if (t == 0u) p.out[blockIdx.x] = r;
}

// ---- 3. the fill ------------------------------------------------------------------------------------------------------
// lanes without a source lane (and lane 0 of a group inside a wider wavefront, which reads another group) keep `keep`
template <int G> CDEVINL int comp_from_left(int keep, int src)
{
    return __builtin_amdgcn_update_dpp(keep, src, G == 16 ? 0x111 /* row_shr:1 */ : 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
}

// what orders a group's table build against its reads: the lanes are one wavefront's (see the head of the file)
CDEVINL void comp_group_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int G, int K, bool PSSM>
__global__ __launch_bounds__(SWG_COMP_THREADS) void swg_comp_fill_kernel(SwgCompParams p)
{
    constexpr uint32_t TAB = PSSM ? 256u : 1024u; // entries of a group's table
    __shared__ int16_t s_tab[(SWG_COMP_THREADS / G) * TAB];
    __shared__ int8_t s_sub[PSSM ? 1 : 1024]; // (a PSSM has no table to stage)
    if (!PSSM)
        for (uint32_t k = threadIdx.x; k < 1024; k += SWG_COMP_THREADS) s_sub[k] = p.sub[k];
    __syncthreads(); // (the only one: before any group takes a job)
    const uint32_t lane = threadIdx.x & (G - 1);
    const uint32_t group = (blockIdx.x * SWG_COMP_THREADS + threadIdx.x) / G;
    if (group >= p.n_groups) return;
    int16_t *tab = s_tab + (threadIdx.x / G) * TAB;
    const int go = p.go, ge = p.ge;
    const int edge = max(max(go, ge), 0); // what a border cell hands down and to the right
    const uint32_t i0 = lane * K;         // columns i0 + 1 .. i0 + K (from 1, as the rows)

    for (uint32_t jn = group; jn < p.n_jobs; jn += p.n_groups) {
        const SwgCompJob job = p.jobs[jn];
        const uint32_t lq = job.lq, len = job.len;
        const uint8_t *d = p.codes + job.res_off;
        const uint32_t steps = len + (lq + K - 1) / K - 1; // lanes past the query's last column are not waited for

        // the pair's table: T itself, or T composed with the substitution table
        const int16_t *T = p.T + (size_t)jn * 256u;
        comp_group_fence(); // (the reads of the pair before)
        for (uint32_t k = lane; k < TAB; k += G) tab[k] = PSSM ? T[k] : T[(int)s_sub[PSSM ? 0 : k] + 128];
        comp_group_fence();

        uint32_t qrow[K];
        const int8_t *prow = nullptr;
        if (PSSM) prow = p.pssm + (job.q_off + i0) * 32;
        int D[K], V[K]; // per column: the diagonal reduction of the row above, the vertical one.  Row 0 is the border.
#pragma unroll
        for (int c = 0; c < K; ++c) {
            if (!PSSM) qrow[c] = i0 + c < lq ? (uint32_t)p.query[job.q_off + i0 + c] * 32u : 0u;
            D[c] = 0, V[c] = edge;
        }
        int inD = 0;     // D of (row above, column i0): from the left lane, a step late
        int Lout = edge; // the left reduction of this lane's last column: the right lane's B
        int best = 0;

        // residue of the row this lane works at step 0, then one step ahead
        uint32_t dcur = lane == 0 ? (uint32_t)d[0] >> 3 : 0u;
        for (uint32_t t = 0; t < steps; ++t) {
            const uint32_t j = t - lane + 1; // (wraps below row 1: then it is above len)
            const bool active = j - 1 < len;
            const uint32_t jnext = j + 1;
            uint32_t dnext = 0;
            if (jnext - 1 < len) dnext = (uint32_t)d[jnext - 1] >> 3;
            // hand-over: the left lane's values of the step before
            int inL = comp_from_left<G>(0, Lout);
            int newD = comp_from_left<G>(0, D[K - 1]);
            if (lane == 0) inL = edge, newD = 0; // column 0 is the border
            if (active) {
                int diag = inD, left = inL;
                const int8_t *srow = PSSM ? prow + dcur : nullptr;
#pragma unroll
                for (int c = 0; c < K; ++c) {
                    const int s = PSSM ? (int)tab[(int)srow[c * 32] + 128] : (int)tab[qrow[c] + dcur];
                    const int H = diag + s, A = V[c], B = left;
                    diag = D[c];
                    D[c] = max(max(max(H, A), B), 0);
                    V[c] = max(max(max(H + go, A + ge), B + go), 0);
                    left = max(max(max(H + go, A + go), B + ge), 0);
                    if (i0 + c < lq) best = max(best, H);
                }
                Lout = left;
            }
            inD = newD;
            dcur = dnext;
        }
#pragma unroll
        for (int off = G / 2; off > 0; off >>= 1) best = max(best, __shfl_xor(best, off, G));
        if (lane == 0) {
            p.out[jn].scaled_score = best;
            p.out[jn].adj_score = swg_comp_unscale(best, p.F);
        }
    }
}

// The instantiations, narrowest first: a query goes to the first whose G * K columns hold it.
struct CompClass {
    int G, K;
};
static const CompClass kCompClasses[] = {{16, 4}, {16, 8}, {32, 8}, {64, 8}, {64, 16}, {64, 32}};
#define SWG_COMP_CLASSES 6
static_assert(64 * 32 == SWG_COMP_COLS, "the widest instantiation is the column limit");

static int comp_class(size_t lq)
{
    for (int c = 0; c < SWG_COMP_CLASSES; ++c)
        if (lq <= (size_t)(kCompClasses[c].G * kCompClasses[c].K)) return c;
    return -1;
}

template <int G, int K> static void comp_launch_gk(bool pssm, unsigned blocks, hipStream_t s, const SwgCompParams &p)
{
    if (pssm) hipLaunchKernelGGL((swg_comp_fill_kernel<G, K, true>), dim3(blocks), dim3(SWG_COMP_THREADS), 0, s, p);
    else hipLaunchKernelGGL((swg_comp_fill_kernel<G, K, false>), dim3(blocks), dim3(SWG_COMP_THREADS), 0, s, p);
}

static void comp_launch(int cls, bool pssm, unsigned blocks, hipStream_t s, const SwgCompParams &p)
{
    switch (cls) {
    case 0: comp_launch_gk<16, 4>(pssm, blocks, s, p); break;
    case 1: comp_launch_gk<16, 8>(pssm, blocks, s, p); break;
    case 2: comp_launch_gk<32, 8>(pssm, blocks, s, p); break;
    case 3: comp_launch_gk<64, 8>(pssm, blocks, s, p); break;
    case 4: comp_launch_gk<64, 16>(pssm, blocks, s, p); break;
    default: comp_launch_gk<64, 32>(pssm, blocks, s, p); break;
    }
}

#define COMP_TRY(ctx, expr)                                                                             \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess) {                                                                         \
            rc = swg_set_ctx_error(ctx, e_ == hipErrorOutOfMemory ? SWG_ERR_NOMEM : SWG_ERR_HIP,        \
                                   "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            goto done;                                                                                  \
        }                                                                                               \
    } while (0)

static size_t comp_round(size_t bytes) { return (bytes + 255) / 256 * 256; }

// Every hit of a checked batch (total > 0 hits).  Everything that refuses the call comes first.  The pairs the fill kernel
// holds are ordered by instantiation and, within one, longest first; one device buffer holds the job records, the
// queries, the count tables, the pairs' tables and the results; the count kernel, the statistic kernel, one fill launch
// per instantiation that has pairs, then one copy back and one stream synchronisation for the call.  The pairs of a query
// beyond the column limit go through the host twin, threaded over pairs.
static int comp_batch(swg_ctx *ctx, const swg_db *db, const SwgTraceBatch &tb, const double P[32], uint32_t mask, swg_comp_result *out,
                      double *lambda_std)
{
    const char *fn = tb.fn;
    const int F = (int)ctx->opt_comp_scale, go = ctx->gap_open + ctx->gap_extend, ge = ctx->gap_extend; // src/alignment.c:58-59
    // original index -> slot of the sorted order
    std::vector<uint32_t> slot_of(db->n_total, ~0u);
    for (size_t s = 0; s < db->order.size(); ++s)
        if (db->order[s] < db->n_total) slot_of[db->order[s]] = (uint32_t)s;
    struct Pair {
        SwgCompJob job;
        size_t dest;
        int cls;
    };
    std::vector<Pair> pairs;
    std::vector<SwgCompHostPair> host_pairs;
    std::vector<size_t> empty_dest; // sequences without a residue: nothing to count, nothing to score
    std::vector<SwgCompQuery> qs;   // the queries that have hits, in the batch's order
    std::vector<size_t> q_of;       // ... and which of the batch's they are
    for (size_t i = 0; i < tb.n_queries; ++i) {
        const size_t lq = (size_t)(tb.q_offsets[i + 1] - tb.q_offsets[i]);
        const int cls = comp_class(lq);
        bool listed = false;
        for (size_t j = 0; j < tb.n_hits[i]; ++j) {
            const uint32_t index = tb.hits[i * tb.k + j].index;
            if (index >= db->n_total)
                return swg_set_ctx_error(ctx, SWG_ERR_ARG, "%s: sequence %u is outside the database of %zu sequences", fn, index, db->n_total);
            const uint32_t s = slot_of[index];
            if (s == ~0u) continue; // another shard's, or outside the view: not written
            const size_t len = db->lens[s];
            if (!swg_comp_pair_fits(lq, len, go, ge, F))
                return swg_set_ctx_error(ctx, SWG_ERR_ARG, "%s: pair %u (%zu x %zu) at scale %d could leave int32 cells", fn, index, lq, len, F);
            if (!listed) {
                SwgCompQuery q = {};
                q.q_off = tb.q_offsets[i] - tb.q_offsets[0], q.lq = (uint32_t)lq;
                qs.push_back(q), q_of.push_back(i), listed = true;
            }
            if (len == 0) {
                empty_dest.push_back(i * tb.k + j);
            } else if (cls < 0) {
                const SwgCompHostPair hp = {i, qs.size() - 1, i * tb.k + j, index, len};
                host_pairs.push_back(hp);
            } else {
                Pair pr = {};
                pr.job.q_off = tb.q_offsets[i] - tb.q_offsets[0];
                pr.job.res_off = db->code_off[s];
                pr.job.lq = (uint32_t)lq, pr.job.len = (uint32_t)len, pr.job.cq = (uint32_t)(qs.size() - 1);
                pr.dest = i * tb.k + j, pr.cls = cls;
                pairs.push_back(pr);
            }
        }
    }
    const size_t n = pairs.size(), nq = qs.size();
    std::stable_sort(pairs.begin(), pairs.end(), [](const Pair &a, const Pair &b) {
        if (a.cls != b.cls) return a.cls < b.cls;
        return (uint64_t)a.job.len + a.job.lq > (uint64_t)b.job.len + b.job.lq;
    });

    // lambda_std of every query of the batch, once, on the host; the count tables of those with hits are kept for the
    // host route
    const size_t row_bytes = tb.pssm ? 32 : 1;
    std::vector<uint32_t> C(std::max<size_t>(nq, 1) * 32 * 256);
    std::vector<double> lam_of(nq);
    std::vector<int> st_of(nq);
    {
        std::vector<uint32_t> C1(32 * 256);
        size_t at = 0;
        for (size_t i = 0; i < tb.n_queries; ++i) {
            const bool held = at < nq && q_of[at] == i;
            if (!held && !lambda_std) continue;
            uint32_t *Ci = held ? C.data() + at * 32 * 256 : C1.data();
            const int8_t *q = tb.src + tb.q_offsets[i] * row_bytes;
            swg_comp_counts(ctx->sub, tb.pssm ? nullptr : q, tb.pssm ? q : nullptr, (size_t)(tb.q_offsets[i + 1] - tb.q_offsets[i]), Ci);
            double lam;
            const int st = swg_comp_lambda_std(Ci, P, mask, &lam);
            if (lambda_std) lambda_std[i] = lam;
            if (held) lam_of[at] = lam, st_of[at] = st, qs[at].lambda_std = lam, qs[at].std_status = (uint32_t)st, ++at;
        }
    }

    int rc = SWG_OK;
    uint32_t launches = 0, per_class[SWG_COMP_CLASSES] = {};
    uint8_t *d_buf = nullptr;
    if (n > 0) {
        const size_t positions = (size_t)(tb.q_offsets[tb.n_queries] - tb.q_offsets[0]);
        const size_t q_bytes = positions * row_bytes;
        // the lanes past a PSSM's last column read rows behind it: slack for the widest group
        const size_t jobs_bytes = comp_round(n * sizeof(SwgCompJob)), qs_bytes = comp_round(nq * sizeof(SwgCompQuery));
        const size_t q_at = jobs_bytes + qs_bytes, up_bytes = q_at + q_bytes;
        const size_t c_off = q_at + comp_round(q_bytes + (tb.pssm ? (size_t)SWG_COMP_COLS * 32 : 0));
        const size_t t_off = c_off + nq * 32 * 256 * sizeof(uint32_t), out_off = t_off + comp_round(n * 256 * sizeof(int16_t));
        std::vector<uint8_t> h_up(up_bytes, 0);
        for (size_t h = 0; h < n; ++h) memcpy(h_up.data() + h * sizeof(SwgCompJob), &pairs[h].job, sizeof(SwgCompJob));
        memcpy(h_up.data() + jobs_bytes, qs.data(), nq * sizeof(SwgCompQuery));
        memcpy(h_up.data() + q_at, tb.src + tb.q_offsets[0] * row_bytes, q_bytes);
        std::vector<swg_comp_result> h_out(n);
        COMP_TRY(ctx, hipSetDevice(ctx->device));
        COMP_TRY(ctx, hipMalloc(&d_buf, out_off + n * sizeof(swg_comp_result)));
        if (tb.pssm) COMP_TRY(ctx, hipMemsetAsync(d_buf + q_at + q_bytes, 0, c_off - q_at - q_bytes, ctx->stream));
        COMP_TRY(ctx, hipMemcpyAsync(d_buf, h_up.data(), up_bytes, hipMemcpyHostToDevice, ctx->stream));
        SwgCompParams p;
        p.query = reinterpret_cast<const int8_t *>(d_buf + q_at), p.pssm = p.query;
        p.sub = ctx->d_sub; // (uploaded by swg_set_scoring on this stream)
        p.codes = reinterpret_cast<const uint8_t *>(db->d_codes);
        p.queries = reinterpret_cast<const SwgCompQuery *>(d_buf + jobs_bytes);
        p.jobs = reinterpret_cast<const SwgCompJob *>(d_buf);
        p.counts = reinterpret_cast<uint32_t *>(d_buf + c_off);
        p.T = reinterpret_cast<int16_t *>(d_buf + t_off);
        p.out = reinterpret_cast<swg_comp_result *>(d_buf + out_off);
        p.n_jobs = (uint32_t)n, p.n_groups = 0, p.mask = mask;
        p.go = F * go, p.ge = F * ge, p.F = F;
        if (tb.pssm) hipLaunchKernelGGL(swg_comp_counts_kernel<true>, dim3((unsigned)nq), dim3(SWG_COMP_THREADS), 0, ctx->stream, p);
        else hipLaunchKernelGGL(swg_comp_counts_kernel<false>, dim3((unsigned)nq), dim3(SWG_COMP_THREADS), 0, ctx->stream, p);
        COMP_TRY(ctx, hipGetLastError());
        hipLaunchKernelGGL(swg_comp_stat_kernel, dim3((unsigned)n), dim3(SWG_COMP_THREADS), 0, ctx->stream, p);
        COMP_TRY(ctx, hipGetLastError());
        for (size_t b = 0; b < n;) {
            size_t e = b;
            while (e < n && pairs[e].cls == pairs[b].cls) ++e;
            const CompClass &cc = kCompClasses[pairs[b].cls];
            const size_t per_block = SWG_COMP_THREADS / cc.G;
            size_t groups = std::min<size_t>(e - b, (size_t)std::max(ctx->n_cu, 1) * 8 * per_block);
            if (ctx->opt_bounds_groups > 0) groups = std::min<size_t>(groups, (size_t)ctx->opt_bounds_groups); // (tests, as the bounds launches)
            SwgCompParams pf = p;
            pf.jobs = p.jobs + b, pf.T = p.T + b * 256, pf.out = p.out + b;
            pf.n_jobs = (uint32_t)(e - b), pf.n_groups = (uint32_t)groups;
            comp_launch(pairs[b].cls, tb.pssm, (unsigned)((groups + per_block - 1) / per_block), ctx->stream, pf);
            COMP_TRY(ctx, hipGetLastError());
            ++launches, per_class[pairs[b].cls] = (uint32_t)(e - b);
            b = e;
        }
        COMP_TRY(ctx, hipMemcpyAsync(h_out.data(), d_buf + out_off, n * sizeof(swg_comp_result), hipMemcpyDeviceToHost, ctx->stream));
        COMP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        for (size_t h = 0; h < n; ++h) out[pairs[h].dest] = h_out[h];
    }
done:
    (void)hipFree(d_buf);
    if (rc != SWG_OK) return rc;
    for (size_t dest : empty_dest) {
        const swg_comp_result r = {0, 0, 65536u, 1, 0.0};
        out[dest] = r;
    }
    if (!host_pairs.empty()) {
        const int bad = swg_comp_pairs_host(db, ctx->sub, go, ge, tb.src, tb.pssm, tb.q_offsets, C.data(), mask, lam_of.data(), st_of.data(), F,
                                            host_pairs.data(), host_pairs.size(), out);
        if (bad) return swg_set_ctx_error(ctx, bad & 2 ? SWG_ERR_NOMEM : SWG_ERR_STATE, "%s: the host route could not read a sequence back", fn);
    }
    ctx->comp_last[0] = (uint32_t)n, ctx->comp_last[1] = (uint32_t)host_pairs.size(), ctx->comp_last[2] = launches;
    for (int c = 0; c < SWG_COMP_CLASSES; ++c) ctx->comp_last[5 + c] = per_class[c];
    return SWG_OK;
}

// try/catch: no C++ exception crosses the ABI (the host vectors are sized by the batch and by the database)
static int comp_checked(swg_ctx *ctx, const swg_db *db, const SwgTraceBatch &tb, const double *freq, swg_comp_result *out, double *lambda_std)
{
    size_t total = 0;
    for (size_t i = 0; ctx && lambda_std && tb.q_offsets && i < tb.n_queries; ++i) lambda_std[i] = 0.0;
    const int rc = swg_trace_check_batch(ctx, db, tb, reinterpret_cast<const swg_alignment *>(out), false, &total);
    if (rc != SWG_OK) return rc;
    if (db->tokens_only)
        return swg_set_ctx_error(ctx, SWG_ERR_STATE, "%s: a database built from 16-lane batches has no residue bytes", tb.fn);
    for (SwgSlot &sl : ctx->slots)
        if (sl.busy) return swg_set_ctx_error(ctx, SWG_ERR_STATE, "%s: searches are in flight on this context", tb.fn);
    double P[32];
    uint32_t mask;
    if (swg_pssm_background(tb.fn, freq, P, &mask) != SWG_OK) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "%s", swg_global_error());
    for (uint32_t &v : ctx->comp_last) v = 0;
    ctx->comp_last[3] = SWG_COMP_COLS, ctx->comp_last[4] = (uint32_t)ctx->opt_comp_scale;
    if (total == 0 && !lambda_std) return SWG_OK;
    try {
        return comp_batch(ctx, db, tb, P, mask, out, lambda_std);
    } catch (const std::bad_alloc &) {
        return swg_set_ctx_error(ctx, SWG_ERR_NOMEM, "%s: out of host memory", tb.fn);
    } catch (const std::exception &e) {
        return swg_set_ctx_error(ctx, SWG_ERR_NOMEM, "%s: %s", tb.fn, e.what());
    }
}

extern "C" int swg_comp_adjust(swg_ctx *ctx, const swg_db *db, const swg_hit *hits, size_t n_hits, const double *freq,
                               swg_comp_result *out, double *lambda_std)
{
    if (!ctx) return swg_set_global_error(SWG_ERR_ARG, "swg_comp_adjust: NULL context");
    if (!db || (n_hits && (!hits || !out))) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "swg_comp_adjust: NULL argument");
    if (!ctx->have_scoring || ctx->query_len() == 0)
        return swg_set_ctx_error(ctx, SWG_ERR_STATE, "swg_comp_adjust: scoring and query must be set first");
    const uint64_t q_offsets[2] = {0, ctx->query_len()};
    const SwgTraceBatch tb = {"swg_comp_adjust", ctx->query_pssm ? ctx->pssm.data() : ctx->query.data(), ctx->query_pssm,
                              q_offsets, 1, hits, n_hits, &n_hits};
    return comp_checked(ctx, db, tb, freq, out, lambda_std);
}

extern "C" int swg_comp_adjust_multi(swg_ctx *ctx, const swg_db *db, const int8_t *queries, const uint64_t *q_offsets, size_t n_queries,
                                     const swg_hit *hits, size_t k, const size_t *n_hits, const double *freq, swg_comp_result *out,
                                     double *lambda_std)
{
    const SwgTraceBatch tb = {"swg_comp_adjust_multi", queries, false, q_offsets, n_queries, hits, k, n_hits};
    return comp_checked(ctx, db, tb, freq, out, lambda_std);
}

extern "C" int swg_comp_adjust_multi_pssm(swg_ctx *ctx, const swg_db *db, const int8_t *pssms, const uint64_t *q_offsets, size_t n_queries,
                                          const swg_hit *hits, size_t k, const size_t *n_hits, const double *freq, swg_comp_result *out,
                                          double *lambda_std)
{
    const SwgTraceBatch tb = {"swg_comp_adjust_multi_pssm", pssms, true, q_offsets, n_queries, hits, k, n_hits};
    return comp_checked(ctx, db, tb, freq, out, lambda_std);
}

int swg_comp_set_option(swg_ctx *ctx, const char *key, long value, bool *known)
{
    *known = strcmp(key, "comp_scale") == 0;
    if (!*known) return SWG_OK;
    if (value < 1 || value > SWG_COMP_SCALE_MAX)
        return swg_set_ctx_error(ctx, SWG_ERR_ARG, "comp_scale must be 1..64 (swg_comp_adjust*: the scale F of the rescaled scores; default 32)");
    ctx->opt_comp_scale = value;
    return SWG_OK;
}

extern "C" int swg_debug_comp_last(const swg_ctx *ctx, uint32_t out[12])
{
    if (!ctx || !out) return swg_set_global_error(SWG_ERR_ARG, "swg_debug_comp_last: NULL argument");
    for (int i = 0; i < 12; ++i) out[i] = ctx->comp_last[i];
    return SWG_OK;
}
