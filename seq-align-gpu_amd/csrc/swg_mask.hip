// swg_mask.hip -- swg_db_mask (include/swg.h): a masked copy of a resident database, made on the device.
//
// The rule is the integer rule of include/swg.h (SEG's trigger and extension stages, no trimming).  Three kernels over the
// parent's resident bytes, none with a floating-point operation:
//   swg_mask_flags_kernel   a wavefront per slot; a tile of 1024 window starts is read with coalesced dword loads into
//                           LDS, every lane slides the weight S over 16 consecutive starts (its 32 residue counts in a
//                           lane-private LDS row) and the two flags per start -- low at K2, low at K1 -- go into two
//                           bitmaps, 64 starts per word, every sequence on words of its own;
//   swg_mask_runs_kernel    a thread per slot: the kept runs by a carry-propagating fill of the K1 bits inside the K2 runs,
//                           upwards and then downwards with the carry handed from word to word (so a trigger at either
//                           end of a run of any length keeps all of it), the widening by W on the same words, and the
//                           three counts, summed per wavefront before one atomic each;
//   swg_mask_apply_kernel   a wavefront per slot, lanes over the dwords: masked bytes take replace << 3.
// A sequence's words: word (byte offset >> 6) + slot onwards -- sequences are whole dwords, not whole 64-byte lines, so the
// slot number keeps two sequences that share a line on different words; nothing but the offsets the database has is needed.
#include "swg_host_internal.h"

#include <chrono>
#include <exception>

#define SWG_MASK_LANE_STARTS 16u                          // window starts a lane slides over
#define SWG_MASK_TILE_STARTS (64u * SWG_MASK_LANE_STARTS) // ... and a wavefront per tile: 16 words of each bitmap
#define SWG_MASK_TILE_DWORDS ((SWG_MASK_TILE_STARTS + 64u) / 4u) // residues of a tile: its starts and W - 1 <= 63 more
// a tile's byte p lies at p + 4 (p >> 7): a lane's 16-byte stride is 4 dwords, and one dword more per 32 puts the 32 lanes
// of an LDS lane group on 32 banks; the count rows are 9 dwords apart for the same reason
#define SWG_MASK_TILE_LDS_DWORDS (SWG_MASK_TILE_DWORDS + SWG_MASK_TILE_DWORDS / 32u + 1u)
#define SWG_MASK_COUNT_ROW 36u

__device__ static inline uint64_t mask_word_base(const uint64_t *code_off, uint64_t slot) { return (code_off[slot] >> 4) + slot; }

__global__ __launch_bounds__(256) void swg_mask_flags_kernel(const uint32_t *codes, const uint64_t *code_off, const uint32_t *lens, uint32_t n_slots,
                                                             uint32_t W, int32_t thr_trigger, int32_t thr_extend, const int32_t *step,
                                                             unsigned long long *low_extend, unsigned long long *low_trigger)
{
    __shared__ uint32_t tile[4][SWG_MASK_TILE_LDS_DWORDS];
    __shared__ __attribute__((aligned(16))) uint8_t counts[4][64][SWG_MASK_COUNT_ROW];
    __shared__ int32_t s_step[64]; // step[c] = T[c + 1] - T[c]: what S gains when a count goes from c to c + 1
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    if (threadIdx.x < 64u) s_step[threadIdx.x] = step[threadIdx.x];
    __syncthreads();
    const uint8_t *tb = reinterpret_cast<const uint8_t *>(tile[wave]);
    uint8_t *cnt = counts[wave][lane];
    for (uint64_t slot = (uint64_t)blockIdx.x * 4u + wave; slot < n_slots; slot += (uint64_t)gridDim.x * 4u) {
        const uint64_t len = lens[slot];
        if (len < W) continue;
        const uint64_t nd = (len + 3u) / 4u, nw = len - W + 1u;
        const uint32_t *c = codes + code_off[slot];
        const uint64_t wbase = mask_word_base(code_off, slot);
        for (uint64_t t0 = 0; t0 < nw; t0 += SWG_MASK_TILE_STARTS) {
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); // (the last tile's reads are behind us)
            __builtin_amdgcn_wave_barrier();
            for (uint32_t k = lane; k < SWG_MASK_TILE_DWORDS; k += 64u) {
                const uint64_t g = t0 / 4u + k;
                tile[wave][k + (k >> 5)] = g < nd ? c[g] : 0u;
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            __builtin_amdgcn_wave_barrier();
            const uint64_t a = t0 + (uint64_t)lane * SWG_MASK_LANE_STARTS; // this lane's first start
            uint32_t f = 0u; // low at K2 in bits 0..15, low at K1 in bits 16..31
            if (a < nw) {
                const uint32_t p0 = lane * SWG_MASK_LANE_STARTS;
                auto residue = [&](uint32_t p) -> uint32_t { return (tb[p + 4u * (p >> 7)] >> 3) & 31u; };
#pragma unroll
                for (uint32_t j = 0; j < 8u; ++j) reinterpret_cast<uint32_t *>(cnt)[j] = 0u;
                int32_t S = 0;
                for (uint32_t j = 0; j < W; ++j) {
                    const uint32_t r = residue(p0 + j), n = cnt[r];
                    S += s_step[n];
                    cnt[r] = (uint8_t)(n + 1u);
                }
                const uint32_t mine = nw - a < SWG_MASK_LANE_STARTS ? (uint32_t)(nw - a) : SWG_MASK_LANE_STARTS;
                for (uint32_t t = 0; t < mine; ++t) {
                    f |= (S >= thr_extend ? 1u : 0u) << t;
                    f |= (S >= thr_trigger ? 0x10000u : 0u) << t;
                    if (t + 1u < mine) { // the slide into this lane's next start
                        const uint32_t ro = residue(p0 + t), no = cnt[ro] - 1u;
                        cnt[ro] = (uint8_t)no;
                        S -= s_step[no];
                        const uint32_t ri = residue(p0 + t + W), ni = cnt[ri];
                        S += s_step[ni];
                        cnt[ri] = (uint8_t)(ni + 1u);
                    }
                }
            }
            const uint32_t g1 = __shfl_down(f, 1, 64), g2 = __shfl_down(f, 2, 64), g3 = __shfl_down(f, 3, 64);
            if ((lane & 3u) == 0u && a < nw) {
                const unsigned long long e = (unsigned long long)(f & 0xFFFFu) | (unsigned long long)(g1 & 0xFFFFu) << 16 |
                                             (unsigned long long)(g2 & 0xFFFFu) << 32 | (unsigned long long)(g3 & 0xFFFFu) << 48;
                const unsigned long long t = (unsigned long long)(f >> 16) | (unsigned long long)(g1 >> 16) << 16 |
                                             (unsigned long long)(g2 >> 16) << 32 | (unsigned long long)(g3 >> 16) << 48;
                const uint64_t w = wbase + t0 / 64u + lane / 4u;
                low_extend[w] = e;
                low_trigger[w] = t;
            }
        }
    }
}

// seeds spread upwards through the runs of m that hold them (seeds within m): the carry of m + seeds runs from the
// lowest seed of a run to the run's end and flips exactly the run's bits above it that are not seeds themselves
__device__ static inline unsigned long long mask_fill_up(unsigned long long m, unsigned long long seeds)
{
    return (((m + seeds) ^ m) & m) | seeds;
}

// (hi : lo) |= itself shifted up by s, 0 <= s <= 32
__device__ static inline void mask_or_shl(unsigned long long &hi, unsigned long long &lo, uint32_t s)
{
    if (s == 0u) return;
    hi |= (hi << s) | (lo >> (64u - s));
    lo |= lo << s;
}

__global__ __launch_bounds__(256) void swg_mask_runs_kernel(const uint64_t *code_off, const uint32_t *lens, uint32_t n_slots, uint32_t W,
                                                            unsigned long long *low_extend, unsigned long long *low_trigger,
                                                            unsigned long long *totals)
{
    unsigned long long n_masked = 0ull, n_segments = 0ull, n_sequences = 0ull;
    for (uint64_t slot = (uint64_t)blockIdx.x * 256u + threadIdx.x; slot < n_slots; slot += (uint64_t)gridDim.x * 256u) {
        const uint64_t len = lens[slot];
        if (len < W) continue;
        const uint64_t nww = (len - W + 1u + 63u) / 64u, nwords = (len + 63u) / 64u;
        unsigned long long *m = low_extend + mask_word_base(code_off, slot), *k = low_trigger + mask_word_base(code_off, slot);
        unsigned long long carry = 0ull;
        for (uint64_t w = 0; w < nww; ++w) { // upwards: a run that the word below filled to its top goes on at bit 0
            const unsigned long long mw = m[w], f = mask_fill_up(mw, (k[w] & mw) | (carry & mw));
            k[w] = f;
            carry = f >> 63;
        }
        carry = 0ull;
        for (uint64_t w = nww; w-- > 0;) { // downwards: the same on the reversed words
            const unsigned long long mw = __brevll(m[w]), f = mask_fill_up(mw, __brevll(k[w]) | (carry & mw));
            k[w] = __brevll(f);
            carry = f >> 63;
        }
        unsigned long long prev = 0ull, mine = 0ull; // the kept starts of the word below; this sequence's masked positions
        for (uint64_t w = 0; w < nwords; ++w) {
            const unsigned long long kw = w < nww ? k[w] : 0ull;
            n_segments += (unsigned long long)__popcll(kw & ~((kw << 1) | (prev >> 63)));
            unsigned long long hi = kw, lo = prev; // a start covers itself and the W - 1 positions above it
            uint32_t span = 1u;
            while (2u * span <= W) mask_or_shl(hi, lo, span), span *= 2u;
            mask_or_shl(hi, lo, W - span);
            m[w] = hi; // the K2 flags of this word are read: the word now holds the masked positions
            mine += (unsigned long long)__popcll(hi);
            prev = kw;
        }
        n_masked += mine;
        n_sequences += mine != 0ull ? 1ull : 0ull;
    }
    unsigned long long v[3] = {n_masked, n_sequences, n_segments};
#pragma unroll
    for (int q = 0; q < 3; ++q) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v[q] += __shfl_xor(v[q], d, 64);
    }
    if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
        for (int q = 0; q < 3; ++q)
            if (v[q] != 0ull) atomicAdd(&totals[q], v[q]);
    }
}

__global__ __launch_bounds__(256) void swg_mask_apply_kernel(const uint64_t *code_off, const uint32_t *lens, uint32_t n_slots, uint32_t W,
                                                             uint32_t replace_code, const unsigned long long *masked, uint32_t *codes)
{
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    for (uint64_t slot = (uint64_t)blockIdx.x * 4u + wave; slot < n_slots; slot += (uint64_t)gridDim.x * 4u) {
        const uint64_t len = lens[slot];
        if (len < W) continue;
        const uint64_t nd = (len + 3u) / 4u;
        uint32_t *c = codes + code_off[slot];
        const unsigned long long *m = masked + mask_word_base(code_off, slot);
        for (uint64_t k = lane; k < nd; k += 64u) {
            const uint32_t bits = (uint32_t)(m[k >> 4] >> ((k & 15u) * 4u)) & 15u;
            if (bits == 0u) continue;
            uint32_t v = c[k];
#pragma unroll
            for (uint32_t j = 0; j < 4u; ++j)
                if ((bits >> j) & 1u) v = (v & ~(0xFFu << (8u * j))) | (replace_code << (8u * j));
            c[k] = v;
        }
    }
}

// ---------------------------------------------------------------------------
// the call
// ---------------------------------------------------------------------------
#define MASK_TRY(expr)                                                                                                       \
    do {                                                                                                                     \
        hipError_t e_ = (expr);                                                                                              \
        if (e_ != hipSuccess)                                                                                                \
            return swg_set_ctx_error(ctx, e_ == hipErrorOutOfMemory ? SWG_ERR_NOMEM : SWG_ERR_HIP, "swg_db_mask: %s failed: %s", #expr, \
                                     hipGetErrorString(e_));                                                                 \
    } while (0)

// Test hook (not part of the public ABI): the n-th device allocation of the next swg_db_mask finds no memory, as a full
// device would have it; 0 disarms.  The call disarms it when it returns.
static int g_mask_fail_alloc = 0;
extern "C" void swg_debug_mask_fail_alloc(int n) { g_mask_fail_alloc = n; }
template <class T> static hipError_t mask_malloc(T **p, size_t bytes)
{
    if (g_mask_fail_alloc > 0 && --g_mask_fail_alloc == 0) return hipErrorOutOfMemory;
    return hipMalloc(p, bytes);
}

static int mask_device(swg_ctx *ctx, const swg_db *parent, const swg_mask_params &p, const int32_t *T, int32_t thr1, int32_t thr2, swg_db *db,
                       void **tmp, hipEvent_t *ev)
{
    const size_t ns = (size_t)parent->n_bins * SWG_BIN, code_bytes = parent->codes.size();
    const size_t words = (code_bytes >> 6) + ns + 1; // of each bitmap (mask_word_base)
    MASK_TRY(hipSetDevice(ctx->device));
    db->device = ctx->device;
    MASK_TRY(mask_malloc(&db->d_codes, std::max<size_t>(4, code_bytes)));
    MASK_TRY(mask_malloc(&db->d_code_off, (ns + 1) * 8));
    MASK_TRY(mask_malloc(&db->d_lens, std::max<size_t>(4, ns * 4)));
    MASK_TRY(mask_malloc(&db->d_order, std::max<size_t>(4, ns * 4)));
    MASK_TRY(mask_malloc(&tmp[0], words * 8));
    MASK_TRY(mask_malloc(&tmp[1], words * 8));
    MASK_TRY(mask_malloc(&tmp[2], 64 * 4 + 3 * 8));
    unsigned long long *d_extend = static_cast<unsigned long long *>(tmp[0]), *d_trigger = static_cast<unsigned long long *>(tmp[1]);
    unsigned long long *d_totals = static_cast<unsigned long long *>(tmp[2]);
    int32_t *d_step = reinterpret_cast<int32_t *>(d_totals + 3);
    MASK_TRY(hipEventCreate(&ev[0]));
    MASK_TRY(hipEventCreate(&ev[1]));
    int32_t step[64];
    for (int c = 0; c < 64; ++c) step[c] = T[c + 1] - T[c]; // (entries from W on are never read: a count stays below W + 1)
    unsigned long long totals[3] = {0, 0, 0};
    hipStream_t s = ctx->stream;
    if (code_bytes) MASK_TRY(hipMemcpyAsync(db->d_codes, parent->d_codes, code_bytes, hipMemcpyDeviceToDevice, s));
    MASK_TRY(hipMemcpyAsync(db->d_code_off, parent->d_code_off, (ns + 1) * 8, hipMemcpyDeviceToDevice, s));
    if (ns) {
        MASK_TRY(hipMemcpyAsync(db->d_lens, parent->d_lens, ns * 4, hipMemcpyDeviceToDevice, s));
        MASK_TRY(hipMemcpyAsync(db->d_order, parent->d_order, ns * 4, hipMemcpyDeviceToDevice, s));
    }
    MASK_TRY(hipMemsetAsync(d_extend, 0, words * 8, s));
    MASK_TRY(hipMemsetAsync(d_trigger, 0, words * 8, s));
    MASK_TRY(hipMemsetAsync(d_totals, 0, 3 * 8, s));
    MASK_TRY(hipMemcpyAsync(d_step, step, sizeof step, hipMemcpyHostToDevice, s));
    MASK_TRY(hipEventRecord(ev[0], s));
    if (ns) {
        const uint32_t per_wave = (uint32_t)std::min<size_t>((ns + 3) / 4, 4096), per_thread = (uint32_t)((ns + 255) / 256);
        hipLaunchKernelGGL(swg_mask_flags_kernel, dim3(per_wave), dim3(256), 0, s, parent->d_codes, parent->d_code_off, parent->d_lens, (uint32_t)ns,
                           (uint32_t)p.window, thr1, thr2, d_step, d_extend, d_trigger);
        MASK_TRY(hipGetLastError());
        hipLaunchKernelGGL(swg_mask_runs_kernel, dim3(per_thread), dim3(256), 0, s, parent->d_code_off, parent->d_lens, (uint32_t)ns, (uint32_t)p.window,
                           d_extend, d_trigger, d_totals);
        MASK_TRY(hipGetLastError());
        hipLaunchKernelGGL(swg_mask_apply_kernel, dim3(per_wave), dim3(256), 0, s, parent->d_code_off, parent->d_lens, (uint32_t)ns, (uint32_t)p.window,
                           (uint32_t)p.replace << 3, d_extend, db->d_codes);
        MASK_TRY(hipGetLastError());
    }
    MASK_TRY(hipEventRecord(ev[1], s));
    MASK_TRY(hipMemcpyAsync(totals, d_totals, sizeof totals, hipMemcpyDeviceToHost, s));
    MASK_TRY(hipStreamSynchronize(s));
    float ms = 0.f;
    MASK_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
    // the host image: the device's bytes, in one copy
    const auto t0 = std::chrono::steady_clock::now();
    if (code_bytes) MASK_TRY(hipMemcpy(db->codes.data(), db->d_codes, code_bytes, hipMemcpyDeviceToHost));
    const auto t1 = std::chrono::steady_clock::now();
    db->masked = true;
    db->mask_info.params = p;
    db->mask_info.residues_masked = totals[0];
    db->mask_info.sequences_masked = totals[1];
    db->mask_info.segments = totals[2];
    db->mask_info.kernel_ms = ms;
    db->mask_info.host_image_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
    db->upload_bytes = 0; // nothing crossed PCIe towards the device
    return SWG_OK;
}

extern "C" int swg_db_mask(swg_ctx *ctx, const swg_db *parent, const swg_mask_params *params, swg_db **out)
{
    if (out) *out = nullptr;
    if (!ctx || !parent || !out) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "swg_db_mask: NULL argument");
    if (parent->root)
        return swg_set_ctx_error(ctx, SWG_ERR_ARG, "swg_db_mask: the parent is a view: mask the root and take the view of the result");
    swg_mask_params p;
    swg_mask_params_default(&p);
    if (params) p = *params;
    int32_t T[65];
    int64_t thr1 = 0, thr2 = 0;
    const int rt = swg_mask_tables(&p, T, &thr1, &thr2);
    if (rt != SWG_OK) return swg_set_ctx_error(ctx, rt, "swg_db_mask: %s", swg_global_error());
    if (parent->tokens_only)
        return swg_set_ctx_error(ctx, SWG_ERR_STATE, "swg_db_mask: a database built from 16-lane batches has no residue bytes to mask");
    if (parent->device != ctx->device || !parent->d_codes)
        return swg_set_ctx_error(ctx, SWG_ERR_STATE, "swg_db_mask: the parent is not resident on device %d", ctx->device);
    // S lies in 0 .. W log2(W) 65536 <= 2^25: thresholds outside int32 cannot be (K >= 0), but the kernels compare in int32
    const int32_t t1 = (int32_t)std::max<int64_t>(INT32_MIN, std::min<int64_t>(INT32_MAX, thr1));
    const int32_t t2 = (int32_t)std::max<int64_t>(INT32_MIN, std::min<int64_t>(INT32_MAX, thr2));
    swg_db *db = nullptr;
    try {
        db = new swg_db();
        db->n_total = parent->n_total;
        db->n_local = parent->n_local;
        db->n_bins = parent->n_bins;
        db->max_nblk = parent->max_nblk;
        db->residues = parent->residues;
        db->rows_padded = parent->rows_padded;
        db->bin_off = parent->bin_off;
        db->bin_nblk = parent->bin_nblk;
        db->order = parent->order;
        db->lens = parent->lens;
        db->code_off = parent->code_off;
        db->pair_rows_prefix = parent->pair_rows_prefix;
        db->codes.resize(parent->codes.size()); // written whole by the copy from the device
    } catch (const std::exception &) {
        delete db;
        return swg_set_ctx_error(ctx, SWG_ERR_NOMEM, "swg_db_mask: out of host memory");
    }
    void *tmp[3] = {nullptr, nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    const int rc = mask_device(ctx, parent, p, T, t1, t2, db, tmp, ev);
    g_mask_fail_alloc = 0;
    if (rc != SWG_OK) (void)hipStreamSynchronize(ctx->stream); // nothing queued may still read what is freed below
    for (void *t : tmp) (void)hipFree(t);
    for (hipEvent_t e : ev)
        if (e) (void)hipEventDestroy(e);
    if (rc != SWG_OK) {
        swg_db_release_device(db);
        delete db;
        return rc;
    }
    *out = db;
    return SWG_OK;
}

extern "C" int swg_db_mask_info(const swg_db *db, swg_mask_info *out)
{
    if (!db || !out) return swg_set_global_error(SWG_ERR_ARG, "swg_db_mask_info: NULL argument");
    if (!db->masked) return swg_set_global_error(SWG_ERR_STATE, "swg_db_mask_info: not a database that swg_db_mask made");
    *out = db->mask_info;
    return SWG_OK;
}
