// swg_api.cpp -- the C-ABI of include/swg.h over the gfx950 kernels.
//
// Replaces, for one query against a whole database, the reference's timed
// region `#pragma omp parallel for ... alignment_fill_matrices(aligners[i])`
// (src/alignment_cmdline.c:503-509) and the aligner_create/aligner_update
// bookkeeping in front of it (src/alignment.c:190-233).  There is no CPU
// fallback in this file: without a GPU swg_create fails with SWG_ERR_NODEVICE.
#include "swg_host_internal.h"
#include "../../include/swg_host.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

// ---------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------
static thread_local std::string g_err;
// (query, scoring) epochs are unique in the process, not per context: a database keeps hints keyed by the epoch
// (f16_veto_epoch), and two contexts that both counted from 1 would hand each other's hints on
static std::atomic<uint64_t> g_epoch{1};

int swg_set_global_error(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

int swg_set_ctx_error(swg_ctx *ctx, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf;
    g_err = buf;
    return code;
}

#define HIP_TRY(ctx, expr)                                                                      \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess)                                                                   \
            return swg_set_ctx_error(ctx, e_ == hipErrorOutOfMemory ? SWG_ERR_NOMEM : SWG_ERR_HIP, \
                                     "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),      \
                                     __FILE__, __LINE__);                                       \
    } while (0)

// A device buffer that grows: room for `need` entries (and `extra` more that the capacity does not count), what it held
// is gone when it had to be allocated anew.
template <class T> static int device_grow(swg_ctx *ctx, T **d, size_t *cap, size_t need, size_t extra = 0)
{
    if (*d && *cap >= need) return SWG_OK;
    (void)hipFree(*d);
    *d = nullptr;
    *cap = 0;
    HIP_TRY(ctx, hipMalloc(d, std::max<size_t>(16, (need + extra) * sizeof(T))));
    *cap = need;
    return SWG_OK;
}

// Wait for everything queued on the stream by polling an event from user space.  A blocking
// hipStreamSynchronize may put the thread to sleep; on a busy host the wake-up alone can cost
// milliseconds per search, several times the fill itself.
static hipError_t spin_sync(swg_ctx *ctx, hipStream_t s)
{
    hipError_t e = hipEventRecord(ctx->cur->ev_done, s);
    if (e != hipSuccess) return e;
    for (;;) {
        e = hipEventQuery(ctx->cur->ev_done);
        if (e != hipErrorNotReady) return e;
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
    }
}

// No C++ exception crosses the ABI (include/swg.h:9-12): the bodies below touch std containers -- the plan cache of a
// database (std::map), the fall-back key vector of swg_search_end (up to n_local keys) -- so every hot entry point
// runs its body inside this guard; an allocation failure or any other std::exception becomes SWG_ERR_NOMEM with
// the text in swg_last_error.  (The reference asserts / exits instead: src/alignment.c:63-66.)
template <class F> static int ctx_guarded(swg_ctx *ctx, const char *what, F &&f)
{
    try {
        return f();
    } catch (const std::bad_alloc &) {
        return swg_set_ctx_error(ctx, SWG_ERR_NOMEM, "%s: out of host memory", what);
    } catch (const std::exception &e) {
        return swg_set_ctx_error(ctx, SWG_ERR_NOMEM, "%s: %s", what, e.what());
    }
}

// Test hook (csrc/swg_host_internal.h, not part of the public ABI): the next time the named site is reached it
// throws std::bad_alloc as a failed allocation there would.  Sites: 1 = body of swg_search_begin, 2 = body of
// swg_search_end, 3 = the fall-back key vector of swg_search_end (reached only when the device top-K could not be
// used).  One shot: the hook clears itself when it fires.  Site 4 is not an exception: the next growth of
// swg_search_above_multi's key pool is refused as if the device had no room (above_multi_pool).  Nor are sites 5 and 6:
// the next reservation of the fourth level's table (5) or of the fifth's (6) of a pruned search is refused in the same
// way (reserve_refine_table).
static int g_fail_alloc_site = 0;
extern "C" void swg_debug_fail_alloc(int site) { g_fail_alloc_site = site; }
static inline void fail_alloc_here(int site)
{
    if (g_fail_alloc_site == site) {
        g_fail_alloc_site = 0;
        throw std::bad_alloc();
    }
}

extern "C" const char *swg_last_error(const swg_ctx *ctx) { return ctx ? ctx->err.c_str() : g_err.c_str(); }
extern "C" const char *swg_global_error(void) { return g_err.c_str(); }
extern "C" int swg_abi_version(void) { return SWG_ABI_VERSION; }

// ---------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------
// The long-pair kernel must run BESIDE the bulk kernel: a stream of its own priority level gets its own hardware
// queue even when other runtimes in the process (RCCL, torch) have used up the default queues, and its workgroups are
// dispatched first.  Created by the first search whose plan has two classes.
static int ensure_stream2(swg_ctx *ctx)
{
    if (ctx->stream2) return SWG_OK;
    int least = 0, greatest = 0;
    HIP_TRY(ctx, hipDeviceGetStreamPriorityRange(&least, &greatest));
    HIP_TRY(ctx, hipStreamCreateWithPriority(&ctx->stream2, hipStreamNonBlocking, greatest));
    return SWG_OK;
}

// A plan of two classes forks before its launches and joins after them: stream2 waits for what the main stream has
// queued so far (ev[6]), the long class is launched on stream2 and the bulk on the main stream, and the main stream
// then waits for the end of stream2's work (ev[7]); bulk_end: ev[5] marks the end of the bulk's launches first, for a
// search that times the two classes (diag_fill_ms).  A plan of one class does neither.
static int fork_long_class(swg_ctx *ctx, const SwgDiagWork &wk)
{
    if (wk.n_classes != 2) return SWG_OK;
    const int r2 = ensure_stream2(ctx);
    if (r2 != SWG_OK) return r2;
    HIP_TRY(ctx, hipEventRecord(ctx->cur->ev[6], ctx->stream));
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream2, ctx->cur->ev[6], 0));
    return SWG_OK;
}
static int join_long_class(swg_ctx *ctx, const SwgDiagWork &wk, bool bulk_end)
{
    if (wk.n_classes != 2) return SWG_OK;
    if (bulk_end) HIP_TRY(ctx, hipEventRecord(ctx->cur->ev[5], ctx->stream));
    HIP_TRY(ctx, hipEventRecord(ctx->cur->ev[7], ctx->stream2));
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->cur->ev[7], 0));
    return SWG_OK;
}

// Top-K and read-out of a finished fill run on a stream of their own, beside the NEXT search's fill: there is no next
// search before the context's second one, which is when the stream is made (the first search's read-out follows its
// fill on the fill stream).
static int ensure_stream3(swg_ctx *ctx)
{
    if (ctx->stream3) return SWG_OK;
    HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->stream3, hipStreamNonBlocking));
    return SWG_OK;
}

// Events and pinned landing buffers of one in-flight search, made when the slot is first used.
static int ensure_slot(swg_ctx *ctx, SwgSlot *sl)
{
    if (sl->ev_done) return SWG_OK;
    for (auto &ev : sl->ev)
        if (!ev) HIP_TRY(ctx, hipEventCreate(&ev));
    if (!sl->h_cand) HIP_TRY(ctx, hipHostMalloc(reinterpret_cast<void **>(&sl->h_cand), SWG_TOPK_CAND_CAP * 8, hipHostMallocDefault));
    if (!sl->h_counters) HIP_TRY(ctx, hipHostMalloc(reinterpret_cast<void **>(&sl->h_counters), 128, hipHostMallocDefault));
    HIP_TRY(ctx, hipEventCreateWithFlags(&sl->ev_done, hipEventDisableTiming)); // (last: marks the slot complete)
    return SWG_OK;
}

extern "C" int swg_create(const swg_config *cfg, swg_ctx **out)
{
    if (!out) return swg_set_global_error(SWG_ERR_ARG, "swg_create: out is NULL");
    *out = nullptr;
    const int dev = cfg ? cfg->device : 0;
    int n = 0;
    const std::chrono::steady_clock::time_point t_enter = std::chrono::steady_clock::now();
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return swg_set_global_error(SWG_ERR_NODEVICE,
                                    "swg_create: no HIP device (%s); libswg has no CPU backend",
                                    e != hipSuccess ? hipGetErrorString(e) : "device count 0");
    if (dev < 0 || dev >= n)
        return swg_set_global_error(SWG_ERR_ARG, "swg_create: device %d out of range (have %d)", dev, n);
    swg_ctx *ctx = new (std::nothrow) swg_ctx();
    if (!ctx) return swg_set_global_error(SWG_ERR_NOMEM, "swg_create: out of memory");
    ctx->device = dev;
    ctx->epoch = g_epoch.fetch_add(1) + 1;
    memset(ctx->sub, 0, sizeof ctx->sub);
    // SWG_TIMING=1: where the wall time of this call goes (most of a one-shot tool run is here: the HIP runtime's
    // own start-up, which the first HIP call of the process pays -- hipGetDeviceCount above)
    typedef std::chrono::steady_clock clk;
    const bool timing = getenv("SWG_TIMING") != nullptr;
    clk::time_point tp = clk::now();
    auto lap = [&](const char *what) {
        if (!timing) return;
        const clk::time_point t = clk::now();
        fprintf(stderr, "[swg_create] %-44s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(t - tp).count());
        tp = t;
    };
    if (timing) fprintf(stderr, "[swg_create] %-44s %8.2f ms\n", "hipGetDeviceCount (HIP runtime start-up)", std::chrono::duration<double, std::milli>(tp - t_enter).count());
    int rc = [&]() -> int {
        HIP_TRY(ctx, hipSetDevice(dev));
        hipDeviceProp_t prop;
        HIP_TRY(ctx, hipGetDeviceProperties(&prop, dev));
        ctx->n_cu = prop.multiProcessorCount;
        lap("hipSetDevice + device properties");
        HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
        lap("the fill stream");
        // (the long class's stream and the read-out stream: ensure_stream2 / ensure_stream3, when a search first needs
        // them -- a stream is ~18 ms of runtime work, and a one-shot tool run is start-up bound)
        // slot 0 (what swg_search uses); the other in-flight slots get their events and pinned buffers when
        // swg_search_begin first hands them out (a tool that searches once never pays for them)
        const int rs = ensure_slot(ctx, &ctx->slots[0]);
        if (rs != SWG_OK) return rs;
        lap("events + pinned buffers of one search slot");
        ctx->cur = &ctx->slots[0];
        HIP_TRY(ctx, hipMalloc(&ctx->d_sub, 32 * 32));
        lap("first device allocation");
        if (timing) {
            // the library's code object (~350 kernel instantiations) is loaded by the first launch of any of its kernels
            HIP_TRY(ctx, swg_launch_zero2(ctx->d_sub, 16, reinterpret_cast<uint8_t *>(ctx->d_sub) + 16, 16, ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            lap("first kernel launch (code object load)");
        }
        return SWG_OK;
    }();
    if (rc != SWG_OK) {
        g_err = ctx->err;
        swg_destroy(ctx);
        return rc;
    }
    *out = ctx;
    return SWG_OK;
}

extern "C" void swg_destroy(swg_ctx *ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    (void)hipFree(ctx->d_sub);
    (void)hipFree(ctx->d_query);
    (void)hipFree(ctx->d_pssm);
    (void)hipFree(ctx->d_kmer_cprof);
    (void)hipFree(ctx->kmer_first[0].d);
    (void)hipFree(ctx->kmer_first[1].d);
    for (SwgKmerTable &t : ctx->kmer_refine) (void)hipFree(t.d);
    (void)hipFree(ctx->d_profile[0]);
    (void)hipFree(ctx->d_profile[1]);
    (void)hipFree(ctx->d_profile[2]);
    (void)hipFree(ctx->d_profile[3]);
    (void)hipFree(ctx->d_profile[4]);
    (void)hipFree(ctx->d_profile[5]);
    (void)hipFree(ctx->d_profile[6]);
    (void)hipFree(ctx->d_profile[7]);
    (void)hipFree(ctx->d_scratch);
    for (SwgSlot &sl : ctx->slots) {
        for (auto &ev : sl.ev)
            if (ev) (void)hipEventDestroy(ev);
        if (sl.ev_done) (void)hipEventDestroy(sl.ev_done);
        (void)hipHostFree(sl.h_cand);
        (void)hipHostFree(sl.h_counters);
        (void)hipHostFree(sl.h_scores);
    }
    if (ctx->b16.db) swg_db_free(ctx->b16.db);
    if (ctx->calib.db) swg_db_free(ctx->calib.db);
    (void)hipHostFree(ctx->b16.h_stage);
    (void)hipHostFree(ctx->b16.h_meta);
    (void)hipFree(ctx->b16.d_stage);
    (void)hipFree(ctx->b16.d_pair_src);
    (void)hipFree(ctx->b16.d_pair_len);
    for (int i = 0; i < 4; ++i) {
        (void)hipHostFree(ctx->h_query_stage[i]);
        if (ctx->ev_query_stage[i]) (void)hipEventDestroy(ctx->ev_query_stage[i]);
    }
    if (ctx->stream2) (void)hipStreamDestroy(ctx->stream2);
    if (ctx->stream3) (void)hipStreamDestroy(ctx->stream3);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

// the row of SWG_REFINE_LEVEL whose option `key` names, or -1
static int refine_option_row(const char *key)
{
    for (int i = 0; i < SWG_REFINE_LEVELS; ++i)
        if (!strcmp(key, SWG_REFINE_LEVEL[i].option)) return i;
    return -1;
}

extern "C" int swg_set_option(swg_ctx *ctx, const char *key, long value)
{
    if (!ctx || !key) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "swg_set_option: NULL argument");
    if (!strcmp(key, "force_bits")) {
        if (value != 0 && value != 16 && value != 32)
            return swg_set_ctx_error(ctx, SWG_ERR_ARG, "force_bits must be 0, 16 or 32");
        ctx->opt_force_bits = value;
    } else if (!strcmp(key, "cols_per_wave")) {
        ctx->opt_cols = value;
    } else if (!strcmp(key, "max_waves")) {
        if (value < 0 || value > 16) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "max_waves must be 0..16");
        ctx->opt_max_waves = value;
    } else if (!strcmp(key, "engine")) {
        if (value < 0 || value > 2) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "engine must be 0 (auto), 1 (systolic) or 2 (diagonal)");
        ctx->opt_engine = value;
    } else if (!strcmp(key, "group_lanes")) {
        if (value != 0 && value != 16 && value != 32 && value != 64)
            return swg_set_ctx_error(ctx, SWG_ERR_ARG, "group_lanes must be 0, 16, 32 or 64");
        ctx->opt_group = value;
    } else if (!strcmp(key, "long_cols")) {
        extern long g_swg_long_cols;
        g_swg_long_cols = value;
    } else if (!strcmp(key, "long_group")) {
        extern long g_swg_long_group;
        g_swg_long_group = value;
    } else if (!strcmp(key, "autotune")) {
        ctx->opt_autotune = value != 0;
    } else if (!strcmp(key, "side_readout")) {
        ctx->opt_side_readout = value != 0;
    } else if (!strcmp(key, "wide16")) {
        ctx->opt_wide = value != 0;
    } else if (!strcmp(key, "f16")) {
        if (value < 0 || value > 2) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "f16 must be 0 (off), 1 (auto) or 2 (whenever the gap scores allow)");
        ctx->opt_f16 = value;
    } else if (!strcmp(key, "f16_pair")) {
        if (value < 0 || value > 2)
            return swg_set_ctx_error(ctx, SWG_ERR_ARG, "f16_pair must be 0 (auto), 1 (v_perm_b32) or 2 (v_pk_fma_f16 wherever it fits)");
        ctx->opt_f16_pair = value;
    } else if (!strcmp(key, "bounds_groups")) {
        if (value < 0) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "bounds_groups must be 0 (auto) or the most lane groups of a bounds launch");
        ctx->opt_bounds_groups = value;
    } else if (!strcmp(key, "last_pass")) {
        ctx->opt_last_pass = value != 0;
    } else if (!strcmp(key, "qq")) {
        ctx->opt_qq = value != 0;
    } else if (!strcmp(key, "batch_geometry")) {
        if (value != 0 && value != 1)
            return swg_set_ctx_error(ctx, SWG_ERR_ARG, "batch_geometry must be 0 (a forced geometry sends a batch one by one) or 1 (the batch takes it)");
        ctx->opt_batch_geometry = value;
    } else if (!strcmp(key, "long_helps")) {
        ctx->opt_long_helps = value != 0;
    } else if (!strcmp(key, "segment_blocks")) {
        // (tests: the multi-pass fill cuts its launches into segments of at most this many token blocks)
        if (value < 0 || value > (long)SWG_DYN_SEG_BLOCKS)
            return swg_set_ctx_error(ctx, SWG_ERR_ARG, "segment_blocks must be 0 (default) .. 2^26-64");
        ctx->opt_seg_blocks = value ? (uint32_t)value : SWG_DYN_SEG_BLOCKS;
    } else if (!strcmp(key, "prune")) {
        if (value < 0 || value > 2)
            return swg_set_ctx_error(ctx, SWG_ERR_ARG, "prune must be 0 (off), 1 (auto) or 2 (wherever it is structurally possible: diagnostic)");
        ctx->opt_prune = value;
    } else if (!strcmp(key, "prune_head")) {
        if (value < 0 || value > 4096) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "prune_head must be 0..4096 (pairs per lane group)");
        ctx->opt_prune_head = value;
    } else if (!strcmp(key, "prune_kmer")) {
        if (value != 0 && value != 1 && value != 4 && value != 5)
            return swg_set_ctx_error(ctx, SWG_ERR_ARG, "prune_kmer must be 0 (auto), 1 (the colmax bound), 4 or 5 (the k-mer bound of that k)");
        ctx->opt_prune_kmer = value;
    } else if (!strcmp(key, "prune_segments")) {
        if (value < 0 || value > (long)SWG_KMER_MAX_SEGMENTS)
            return swg_set_ctx_error(ctx, SWG_ERR_ARG, "prune_segments must be 0 (auto) or 1..32 (the segments of the k-mer bound's table; 1: unsegmented)");
        ctx->opt_prune_segments = value;
    } else if (const int row = refine_option_row(key); row >= 0) { // "prune_refine" .. "prune_refine5"
        if (!swg_refine_value_ok(row, value)) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "%s", SWG_REFINE_LEVEL[row].option_error);
        ctx->opt_prune_refine[row] = value;
    } else if (!strcmp(key, "prune_gate")) {
        if (!swg_prune_gate_value_ok(value))
            return swg_set_ctx_error(ctx, SWG_ERR_ARG, "prune_gate must be 0 (auto), 1 (off) or 2 (wherever the first-level bound is a segmented k-mer bound)");
        ctx->opt_prune_gate = value;
    } else if (!strcmp(key, "prune_table_bits")) {
        if (value != 0 && value != 16)
            return swg_set_ctx_error(ctx, SWG_ERR_ARG, "prune_table_bits must be 0 (auto: bytes where they hold every entry) or 16");
        ctx->opt_prune_table_bits = value;
    } else if (!strcmp(key, "prune_cut")) {
        if (value != 0 && value != 1)
            return swg_set_ctx_error(ctx, SWG_ERR_ARG, "prune_cut must be 0 (a stage's pairs are cut one by one) or 1 (the prefix of the length order)");
        ctx->opt_prune_cut = value;
    } else if (!strcmp(key, "above_batch")) {
        if (value < 0 || value > 2)
            return swg_set_ctx_error(ctx, SWG_ERR_ARG, "above_batch must be 0 (auto), 1 (one launch wherever the batch is admitted) or 2 (one query after another)");
        ctx->opt_above_batch = value;
    } else if (!strcmp(key, "calib_seqs")) {
        if (value < 2 || value > (1l << 20)) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "calib_seqs must be 2..1048576 (random sequences a calibration scores)");
        ctx->opt_calib_seqs = value;
    } else if (!strcmp(key, "pssm_msa_mb")) {
        if (value < 0 || value > 65536) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "pssm_msa_mb must be 0..65536 (MiB of device rows one group of queries of swg_pssm_build* may take; 0: every query alone)");
        ctx->opt_pssm_msa_mb = value;
    } else if (!strcmp(key, "pssm_blocks")) {
        if (value != 0 && value != 1)
            return swg_set_ctx_error(ctx, SWG_ERR_ARG, "pssm_blocks must be 0 (swg_pssm_build*: the whole query is every column's block) or 1 (per-column blocks)");
        ctx->opt_pssm_blocks = value;
    } else if (!strcmp(key, "pssm_purge")) {
        if (value != 0 && (value < 50 || value > 100))
            return swg_set_ctx_error(ctx, SWG_ERR_ARG, "pssm_purge must be 0 (off) or 50..100 (swg_pssm_build*: percent identity at which a hit is dropped)");
        ctx->opt_pssm_purge = value;
    } else if (!strcmp(key, "calib_len")) {
        if (value < 8 || value > (1l << 14)) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "calib_len must be 8..16384 (residues of a calibration's random sequences)");
        ctx->opt_calib_len = value;
    } else if (!strcmp(key, "calib_seed")) {
        if (value < 0) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "calib_seed must be >= 0");
        ctx->opt_calib_seed = value;
    } else if (!strcmp(key, "q32_waves")) {
        ctx->opt_q32_waves = value;
    } else if (!strcmp(key, "wave_budget")) {
        ctx->opt_wave_budget = value;
    } else if (!strcmp(key, "batch")) {
        if (value < 0 || value > 8) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "batch must be 0..8 (pairs one queue request claims; 0 and 1: one)");
        ctx->opt_batch = value;
    } else if (!strcmp(key, "batch_blocks")) {
        if (value < 0) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "batch_blocks must be >= 0 (token blocks; 0: from the geometry)");
        ctx->opt_batch_blocks = value;
    } else if (!strcmp(key, "work_queue")) {
        ctx->opt_dynamic = value != 0;
    } else if (!strcmp(key, "prio_share")) {
        if (value < 0) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "prio_share must be >= 0 (percent)");
        ctx->opt_prio_share = value;
    } else if (!strcmp(key, "long_split")) {
        if (value < -1) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "long_split must be -1 (off), 0 (auto) or a row count");
        ctx->opt_long_split = value;
    } else if (!strcmp(key, "workgroups")) {
        if (value < 0) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "workgroups must be >= 0");
        ctx->opt_workgroups = value;
    } else {
        bool known = false; // (the options of swg_comp_adjust* are checked beside the calls that read them)
        const int rc = swg_comp_set_option(ctx, key, value, &known);
        if (known) return rc;
        return swg_set_ctx_error(ctx, SWG_ERR_ARG, "swg_set_option: unknown key '%s'", key);
    }
    return SWG_OK;
}

extern "C" int swg_set_scoring(swg_ctx *ctx, const int8_t sub[32][32], int gap_open, int gap_extend)
{
    if (!ctx || !sub) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "swg_set_scoring: NULL argument");
    if (gap_open < -32768 || gap_open > 32767 || gap_extend < -32768 || gap_extend > 32767)
        return swg_set_ctx_error(ctx, SWG_ERR_ARG,
                                 "swg_set_scoring: gap scores must fit the reference's int16 score_t");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    memcpy(ctx->sub, sub, 32 * 32);
    ctx->gap_open = gap_open;
    ctx->gap_extend = gap_extend;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_sub, ctx->sub, 32 * 32, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->have_scoring = true;
    ctx->epoch = g_epoch.fetch_add(1) + 1;
    return SWG_OK;
}

// Queues a copy of the query (index bytes or a PSSM) to dst on the context's stream.  No wait here: the copy and the
// profile build that consumes it are ordered on the context's stream behind any search still in flight, so a caller
// can stream queries against a resident database (set_query, search_begin, set_query, search_begin, search_end, ...).
// The copy reads a pinned staging buffer of its own (four in rotation, each guarded by an event): the host copy
// ctx->query / ctx->pssm is rewritten by the next call while this one's transfer may still be queued.
static int stage_query(swg_ctx *ctx, int8_t *dst, const int8_t *src, size_t bytes)
{
    const int b = ctx->query_stage_next;
    ctx->query_stage_next = (b + 1) % 4;
    if (!ctx->ev_query_stage[b]) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_query_stage[b], hipEventDisableTiming));
    else HIP_TRY(ctx, hipEventSynchronize(ctx->ev_query_stage[b])); // (four transfers ago: long done)
    if (bytes > ctx->h_query_stage_cap[b]) {
        (void)hipHostFree(ctx->h_query_stage[b]);
        ctx->h_query_stage[b] = nullptr;
        ctx->h_query_stage_cap[b] = 0;
        HIP_TRY(ctx, hipHostMalloc(reinterpret_cast<void **>(&ctx->h_query_stage[b]), bytes, hipHostMallocDefault));
        ctx->h_query_stage_cap[b] = bytes;
    }
    memcpy(ctx->h_query_stage[b], src, bytes);
    HIP_TRY(ctx, hipMemcpyAsync(dst, ctx->h_query_stage[b], bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(ctx->ev_query_stage[b], ctx->stream));
    return SWG_OK;
}

extern "C" int swg_set_query(swg_ctx *ctx, const int8_t *idx, size_t lq)
{
    if (!ctx || !idx || lq == 0)
        return swg_set_ctx_error(ctx, SWG_ERR_ARG, "swg_set_query: NULL or empty query");
    if (lq > (1u << 24)) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "swg_set_query: query too long");
    for (size_t i = 0; i < lq; ++i)
        if (idx[i] < 1 || idx[i] > 31)
            return swg_set_ctx_error(ctx, SWG_ERR_RESIDUE,
                                     "swg_set_query: residue index %d at %zu outside 1..31", idx[i], i);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (lq > ctx->d_query_cap) {
        (void)hipFree(ctx->d_query);
        ctx->d_query = nullptr;
        ctx->d_query_cap = 0;
        HIP_TRY(ctx, hipMalloc(&ctx->d_query, lq));
        ctx->d_query_cap = lq;
    }
    ctx->query.assign(idx, idx + lq);
    ctx->pssm.clear();
    ctx->query_pssm = false;
    const int rc = stage_query(ctx, ctx->d_query, idx, lq);
    if (rc != SWG_OK) return rc;
    ctx->epoch = g_epoch.fetch_add(1) + 1;
    return SWG_OK;
}

extern "C" int swg_set_query_pssm(swg_ctx *ctx, const int8_t *pssm, size_t lq)
{
    if (!ctx || !pssm || lq == 0)
        return swg_set_ctx_error(ctx, SWG_ERR_ARG, "swg_set_query_pssm: NULL or empty PSSM");
    if (lq > (1u << 24)) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "swg_set_query_pssm: query too long");
    const size_t bytes = lq * 32;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (bytes > ctx->d_pssm_cap) {
        (void)hipFree(ctx->d_pssm);
        ctx->d_pssm = nullptr;
        ctx->d_pssm_cap = 0;
        HIP_TRY(ctx, hipMalloc(&ctx->d_pssm, bytes));
        ctx->d_pssm_cap = bytes;
    }
    ctx->pssm.assign(pssm, pssm + bytes);
    ctx->query.clear();
    ctx->query_pssm = true;
    const int rc = stage_query(ctx, ctx->d_pssm, pssm, bytes);
    if (rc != SWG_OK) return rc;
    ctx->epoch = g_epoch.fetch_add(1) + 1;
    return SWG_OK;
}

// ---------------------------------------------------------------------------
// database residency
// ---------------------------------------------------------------------------
void swg_db_release_search_state(swg_db *db)
{
    if (!db || db->device < 0) return;
    (void)hipSetDevice(db->device);
    (void)hipFree(db->d_packed);
    (void)hipFree(db->d_bin_off);
    (void)hipFree(db->d_bin_nblk);
    for (swg_db::Bufs &b : db->bufs) {
        (void)hipFree(b.d_scores);
        (void)hipFree(b.d_list);
        (void)hipFree(b.d_counters);
        (void)hipFree(b.d_keys);
        (void)hipFree(b.d_hist);
        (void)hipFree(b.d_pair_bound);
        (void)hipFree(b.d_above);
        b = swg_db::Bufs();
    }
    (void)hipFree(db->ptok.d_tok);
    (void)hipFree(db->ptok.d_pair_off);
    (void)hipFree(db->ptok.d_edge[0]);
    (void)hipFree(db->ptok.d_edge[1]);
    (void)hipFree(db->ptok.d_edge32[0]);
    (void)hipFree(db->ptok.d_edge32[1]);
    (void)hipFree(db->ptok.d_edge32d[0]);
    (void)hipFree(db->ptok.d_edge32d[1]);
    db->ptok = SwgPairTokens();
    for (SwgDiagLayout &L : db->diag) {
        (void)hipFree(L.d_tok);
        (void)hipFree(L.d_stream_off);
        (void)hipFree(L.d_stream_pairs);
        (void)hipFree(L.d_stream_pair_off);
        (void)hipFree(L.d_scratch);
        L = SwgDiagLayout();
    }
    db->d_packed = nullptr;
    db->d_bin_off = nullptr;
    db->d_bin_nblk = nullptr;
    db->d_scores = nullptr;
    db->d_list = nullptr;
    db->d_counters = nullptr;
    db->d_keys = nullptr;
    db->d_hist = nullptr;
    db->d_pair_bound = nullptr;
}

void swg_db_release_device(swg_db *db)
{
    if (!db || db->device < 0) return;
    swg_db_release_search_state(db);
    if (!db->root) (void)hipFree(db->d_codes); // (a view's residue bytes are its root's)
    (void)hipFree(db->d_code_off);
    (void)hipFree(db->d_lens);
    (void)hipFree(db->d_order);
    db->d_codes = nullptr;
    db->d_code_off = nullptr;
    db->d_lens = nullptr;
    db->d_order = nullptr;
    db->device = -1;
}

// Output buffers of in-flight slot `slot` (allocated on first use) become the current ones.
static int select_bufs(swg_ctx *ctx, swg_db *db, int slot)
{
    swg_db::Bufs &b = db->bufs[slot];
    const size_t ns = (size_t)db->n_bins * SWG_BIN;
    if (!b.d_scores) {
        HIP_TRY(ctx, hipMalloc(&b.d_scores, std::max<size_t>(4, ns * 4)));
        HIP_TRY(ctx, hipMalloc(&b.d_list, std::max<size_t>(4, ns * 8)));
        HIP_TRY(ctx, hipMalloc(&b.d_counters, SWG_COUNTER_BYTES));
        HIP_TRY(ctx, hipMalloc(&b.d_keys, SWG_TOPK_CAND_CAP * 8));
        HIP_TRY(ctx, hipMalloc(&b.d_hist, 4096 * 4));
    }
    db->d_scores = b.d_scores;
    db->d_list = b.d_list;
    db->d_counters = b.d_counters;
    db->d_keys = b.d_keys;
    db->d_hist = b.d_hist;
    db->d_pair_bound = b.d_pair_bound;
    return SWG_OK;
}

// What crosses PCIe: one byte per residue (whole dwords per sequence) and 16 bytes per slot.  The
// kernels' own layouts are built from that on the device: the pair tokens on the first search that
// uses the diagonal engine's work queue (ensure_pair_tokens), the bin image only if an engine that
// reads bins is ever used (ensure_bins).
extern "C" int swg_db_upload(swg_ctx *ctx, swg_db *db)
{
    if (!ctx || !db) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "swg_db_upload: NULL argument");
    if (db->root) return swg_set_ctx_error(ctx, SWG_ERR_STATE, "swg_db_upload: a view is resident from its creation, where its parent is");
    if (swg_db_views_alive(db) > 0)
        return swg_set_ctx_error(ctx, SWG_ERR_STATE, "swg_db_upload: %zu views read this database's resident bytes: free them first",
                                 swg_db_views_alive(db));
    swg_db_release_device(db);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    db->device = ctx->device;
    const size_t nb = db->n_bins, ns = nb * SWG_BIN;
    int rc = [&]() -> int {
        std::vector<uint64_t> off_dw;
        try {
            off_dw.resize(ns + 1);
        } catch (const std::exception &) {
            return swg_set_ctx_error(ctx, SWG_ERR_NOMEM, "swg_db_upload: out of host memory");
        }
        for (size_t i = 0; i <= ns; ++i) off_dw[i] = db->code_off[i] / 4;
        HIP_TRY(ctx, hipMalloc(&db->d_codes, std::max<size_t>(4, db->codes.size())));
        HIP_TRY(ctx, hipMalloc(&db->d_code_off, (ns + 1) * 8));
        HIP_TRY(ctx, hipMalloc(&db->d_lens, std::max<size_t>(4, ns * 4)));
        HIP_TRY(ctx, hipMalloc(&db->d_order, std::max<size_t>(4, ns * 4)));
        int rb = select_bufs(ctx, db, 0);
        if (rb != SWG_OK) return rb;
        if (!db->codes.empty())
            HIP_TRY(ctx, hipMemcpyAsync(db->d_codes, swg_db_codes(db), db->codes.size(), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(db->d_code_off, off_dw.data(), (ns + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
        if (ns) {
            HIP_TRY(ctx, hipMemcpyAsync(db->d_lens, db->lens.data(), ns * 4, hipMemcpyHostToDevice, ctx->stream));
            HIP_TRY(ctx, hipMemcpyAsync(db->d_order, db->order.data(), ns * 4, hipMemcpyHostToDevice, ctx->stream));
        }
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); // off_dw goes out of scope
        db->upload_bytes = db->codes.size() + (ns + 1) * 8 + ns * 8;
        return SWG_OK;
    }();
    if (rc != SWG_OK) swg_db_release_device(db);
    return rc;
}

// A view: the listed sequences of a resident database as a database of its own.  The host image (swg_view_host) is made
// from the parent's without touching a residue byte; what crosses PCIe is the selected slots, 4 bytes each, from which
// swg_gather_view_kernel writes the view's three words per slot out of the root's resident ones.  d_codes is the root's
// pointer; pair tokens, bins and output buffers come from the same lazy paths as any database's.
extern "C" int swg_db_view(swg_ctx *ctx, swg_db *parent, const uint32_t *indices, size_t n, swg_db **out)
{
    if (out) *out = nullptr;
    if (!ctx || !parent || !out || (n > 0 && !indices)) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "swg_db_view: NULL argument");
    return ctx_guarded(ctx, "swg_db_view", [&]() -> int {
        if (parent->device != ctx->device || !parent->d_codes)
            return swg_set_ctx_error(ctx, SWG_ERR_STATE, "swg_db_view: the parent is not resident on device %d", ctx->device);
        if (parent->tokens_only)
            return swg_set_ctx_error(ctx, SWG_ERR_STATE, "swg_db_view: a database built from 16-lane batches has no residue bytes to view");
        std::vector<uint32_t> slots;
        const int rs = swg_view_select(parent, indices, n, &slots);
        if (rs != SWG_OK) return swg_set_ctx_error(ctx, rs, "%s", swg_global_error());
        swg_db *root = parent->root ? parent->root : parent;
        swg_db *v = swg_view_host(parent, slots);
        const size_t ns = (size_t)v->n_bins * SWG_BIN;
        slots.resize(ns, 0xFFFFFFFFu); // the empty slots of the last bin
        uint32_t *d_slots = nullptr;
        const int rc = [&]() -> int {
            HIP_TRY(ctx, hipSetDevice(ctx->device));
            v->device = ctx->device;
            v->d_codes = root->d_codes;
            HIP_TRY(ctx, hipMalloc(&v->d_code_off, (ns + 1) * 8));
            HIP_TRY(ctx, hipMalloc(&v->d_lens, std::max<size_t>(4, ns * 4)));
            HIP_TRY(ctx, hipMalloc(&v->d_order, std::max<size_t>(4, ns * 4)));
            HIP_TRY(ctx, hipMalloc(&d_slots, std::max<size_t>(4, ns * 4)));
            const int rb = select_bufs(ctx, v, 0);
            if (rb != SWG_OK) return rb;
            if (ns) HIP_TRY(ctx, hipMemcpyAsync(d_slots, slots.data(), ns * 4, hipMemcpyHostToDevice, ctx->stream));
            HIP_TRY(ctx, swg_launch_gather_view(d_slots, (uint32_t)ns, (uint32_t)root->order.size(), root->d_code_off, root->d_lens,
                                                root->d_order, v->d_code_off, v->d_lens, v->d_order, ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); // `slots` goes out of scope; the view may be used from any context of the device
            v->upload_bytes = ns * 4;
            return SWG_OK;
        }();
        (void)hipFree(d_slots);
        if (rc != SWG_OK) {
            swg_db_free(v);
            return rc;
        }
        *out = v;
        return SWG_OK;
    });
}

// The bin image: built on the device from the residue dwords the first time an engine that reads
// bins is used on this database (the default engine never does).
static int ensure_bins(swg_ctx *ctx, swg_db *db)
{
    if (db->d_packed || db->n_bins == 0) return SWG_OK;
    if (db->tokens_only)
        return swg_set_ctx_error(ctx, SWG_TAKE_HOST_ROUTE, "this search needs the bin image, which a database built from 16-lane batches does not have");
    const size_t nb = db->n_bins;
    const uint64_t dwords = db->bin_off[nb - 1] + (uint64_t)db->bin_nblk[nb - 1] * SWG_BIN;
    HIP_TRY(ctx, hipMalloc(&db->d_bin_off, nb * 8));
    HIP_TRY(ctx, hipMalloc(&db->d_bin_nblk, nb * 4));
    HIP_TRY(ctx, hipMemcpyAsync(db->d_bin_off, db->bin_off.data(), nb * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(db->d_bin_nblk, db->bin_nblk.data(), nb * 4, hipMemcpyHostToDevice, ctx->stream));
    uint32_t *packed = nullptr;
    HIP_TRY(ctx, hipMalloc(&packed, std::max<uint64_t>(4, dwords * 4)));
    hipError_t e = swg_launch_build_bins(db->d_codes, db->d_code_off, db->d_lens, db->d_bin_off, db->d_bin_nblk,
                                         (uint32_t)nb, packed, ctx->stream);
    if (e != hipSuccess) {
        (void)hipFree(packed);
        HIP_TRY(ctx, e);
    }
    db->d_packed = packed;
    return SWG_OK;
}

// ---------------------------------------------------------------------------
// planning
// ---------------------------------------------------------------------------
// The systolic plan from plain values (make_plan for a search, swg_debug_plan_systolic for the tests): cols > 0 asks for the
// instantiation with that many columns per wavefront, max_waves > 0 caps the wavefronts of a workgroup (more passes),
// workgroups > 0 fixes the grid.  false: no instantiation of `cols` columns is built for these cells.
static bool systolic_plan(int bits, uint32_t n_items, long cols, long max_waves, long workgroups, size_t lq, int n_cu, SwgSystolicPlan *pl)
{
    const int nv = swg_num_variants(bits);
    int variant = 0;
    if (cols > 0) {
        variant = -1;
        for (int v = 0; v < nv; ++v)
            if (swg_variant_info(bits, v).K == (int)cols) variant = v;
        if (variant < 0) return false;
    }
    const SwgKernelInfo info = swg_variant_info(bits, variant);
    int maxw = info.max_waves;
    if (max_waves > 0) maxw = std::min<int>(maxw, (int)max_waves);
    const size_t cols_per_pass_max = (size_t)maxw * info.K;
    const int npass = (int)((lq + cols_per_pass_max - 1) / cols_per_pass_max);
    const int W = (int)((lq + (size_t)npass * info.K - 1) / ((size_t)npass * info.K));
    // residency: info.max_waves is also the wave budget of one CU for this
    // instantiation's register allocation; LDS is the other limit
    const size_t lds = info.lds_per_wave * (size_t)W + info.lds_fixed;
    long wgs = (long)n_cu * swg_workgroups_per_cu(info.max_waves, W, lds);
    if (workgroups > 0) wgs = workgroups;
    wgs = std::max<long>(1, std::min<long>(wgs, (long)n_items));
    pl->bits = bits;
    pl->variant = variant;
    pl->K = info.K;
    pl->W = W;
    pl->npass = npass;
    pl->workgroups = (int)wgs;
    pl->info = info;
    return true;
}

// cols > 0: the instantiation with that many columns per wavefront (option cols_per_wave, or a measured / modelled choice)
static int make_plan(swg_ctx *ctx, int bits, uint32_t n_items, long cols, SwgSystolicPlan *pl)
{
    if (!systolic_plan(bits, n_items, cols, ctx->opt_max_waves, ctx->opt_workgroups, ctx->query_len(), ctx->n_cu, pl))
        return swg_set_ctx_error(ctx, SWG_ERR_ARG, "cols_per_wave=%ld not built for the %d-bit path",
                                 cols, bits);
    return SWG_OK;
}

// tail_cols > 0: the last tail_cols layout columns (one pass) have a slice geometry of their own, tail_k_real query
// columns in tail_k_padded layout columns per lane, and begin at query column tail_qcol0.
static int ensure_profile_cols(swg_ctx *ctx, int which, uint32_t ncols, int elem_size, uint64_t geom, int k_real = 1,
                               int k_padded = 1, int chunk_cols = 4, int swizzle_lanes = 0, int f16 = 0, uint32_t tail_cols = 0,
                               int tail_k_real = 0, int tail_k_padded = 0, uint32_t tail_qcol0 = 0)
{
    const size_t bytes = (size_t)ncols * 32 * elem_size;
    // (query, scoring) epoch and geometry: the epoch is spread over all 64 bits so that no geometry field can alias it
    const uint64_t tag = (ctx->epoch * 0x9E3779B97F4A7C15ull) ^ geom ^ ((uint64_t)swizzle_lanes << 56) ^ ((uint64_t)chunk_cols << 60) ^
                         ((uint64_t)(f16 != 0) << 53) ^ (((uint64_t)tail_cols * 0xD6E8FEB86659FD93ull) ^ ((uint64_t)tail_k_real << 24));
    if (ctx->profile_tag[which] == tag && ctx->d_profile[which]) return SWG_OK;
    if (bytes > ctx->d_profile_cap[which]) {
        (void)hipFree(ctx->d_profile[which]);
        ctx->d_profile[which] = nullptr;
        ctx->d_profile_cap[which] = 0;
        HIP_TRY(ctx, hipMalloc(&ctx->d_profile[which], bytes));
        ctx->d_profile_cap[which] = bytes;
    }
    // (a PSSM query: the scores come from the PSSM's rows instead of the table's, every layout the same)
    const int8_t *d_pssm = ctx->query_pssm ? ctx->d_pssm : nullptr;
    HIP_TRY(ctx, swg_launch_build_profile(ctx->d_sub, ctx->d_query, (uint32_t)ctx->query_len(), ncols - tail_cols,
                                          elem_size, chunk_cols, k_real, k_padded, ctx->d_profile[which], ctx->stream,
                                          swizzle_lanes, f16, 0, d_pssm));
    if (tail_cols > 0)
        HIP_TRY(ctx, swg_launch_build_profile(ctx->d_sub, ctx->d_query, (uint32_t)ctx->query_len(), tail_cols, elem_size, chunk_cols,
                                              tail_k_real, tail_k_padded, ctx->d_profile[which] + (size_t)(ncols - tail_cols) * 32 * elem_size,
                                              ctx->stream, swizzle_lanes, f16, tail_qcol0, d_pssm));
    ctx->profile_tag[which] = tag;
    return SWG_OK;
}

static int ensure_profile(swg_ctx *ctx, const SwgSystolicPlan &pl)
{
    return ensure_profile_cols(ctx, pl.bits == 16 ? 0 : 1, (uint32_t)(pl.npass * pl.W * pl.K), pl.info.elem_size,
                               ((uint64_t)pl.K << 20) ^ ((uint64_t)pl.W << 12) ^ (uint64_t)pl.npass, 1, 1, 4, 0, pl.bits == 16 && pl.f16);
}

// Stream layout of the diagonal engine for this database at this stream count,
// built on the host and kept resident until the geometry changes.
static int ensure_diag_layout(swg_ctx *ctx, swg_db *db, int cls, const SwgDiagPlan &pl, uint64_t pair_begin,
                              uint64_t pair_end)
{
    SwgDiagLayout &L = db->diag[cls];
    const uint32_t spw = (uint32_t)(pl.W * (64 / pl.G));
    if (L.n_streams != pl.n_streams || L.streams_per_wg != spw || L.pair_begin != pair_begin ||
        L.pair_end != pair_end || !L.d_tok) {
        (void)hipFree(L.d_tok);
        (void)hipFree(L.d_stream_off);
        (void)hipFree(L.d_stream_pairs);
        (void)hipFree(L.d_stream_pair_off);
        (void)hipFree(L.d_scratch);
        L = SwgDiagLayout();
        try {
            swg_build_diag_layout(db, pair_begin, pair_end, pl.n_streams, spw, &L);
            L.streams_per_wg = spw;
        } catch (const std::bad_alloc &) {
            L = SwgDiagLayout();
            return swg_set_ctx_error(ctx, SWG_ERR_NOMEM, "diagonal layout: out of host memory");
        }
        const size_t S = L.n_streams;
        HIP_TRY(ctx, hipMalloc(&L.d_tok, std::max<size_t>(16, L.tok.size() * 4)));
        HIP_TRY(ctx, hipMalloc(&L.d_stream_off, (S + 1) * 8));
        HIP_TRY(ctx, hipMalloc(&L.d_stream_pairs, std::max<size_t>(4, L.stream_pairs.size() * 4)));
        HIP_TRY(ctx, hipMalloc(&L.d_stream_pair_off, (S + 1) * 4));
        if (!L.tok.empty())
            HIP_TRY(ctx, hipMemcpyAsync(L.d_tok, L.tok.data(), L.tok.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(L.d_stream_off, L.stream_off.data(), (S + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
        if (!L.stream_pairs.empty())
            HIP_TRY(ctx, hipMemcpyAsync(L.d_stream_pairs, L.stream_pairs.data(), L.stream_pairs.size() * 4,
                                        hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(L.d_stream_pair_off, L.stream_pair_off.data(), (S + 1) * 4,
                                    hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        std::vector<uint32_t>().swap(L.tok); // the device copy is the one that is used
    }
    if (pl.npass > 1 && L.d_scratch_rows < L.total_blocks * 4) {
        (void)hipFree(L.d_scratch);
        L.d_scratch = nullptr;
        L.d_scratch_rows = 0;
        HIP_TRY(ctx, hipMalloc(&L.d_scratch, std::max<size_t>(8, L.total_blocks * 4 * sizeof(uint2))));
        L.d_scratch_rows = L.total_blocks * 4;
    }
    return SWG_OK;
}

// Pair-major tokens, built once per database on first use by the diagonal engine: the block
// offsets of the pairs on the host (they follow from the lengths alone, and the planner wants them
// too), the tokens themselves on the device from the resident residue dwords.
static int ensure_pair_tokens(swg_ctx *ctx, swg_db *db)
{
    SwgPairTokens &T = db->ptok;
    if (T.tried) return SWG_OK;
    T.tried = true;
    try {
        if (swg_build_pair_tokens(db, nullptr, nullptr, &T.pair_blocks_prefix) != 0) return SWG_OK; // too large: static streams
    } catch (const std::exception &) {
        return swg_set_ctx_error(ctx, SWG_ERR_NOMEM, "pair tokens: out of host memory");
    }
    T.total_blocks = T.pair_blocks_prefix.back();
    const uint32_t n_pairs = (uint32_t)(T.pair_blocks_prefix.size() - 1);
    // (one more block, all zeros, behind the last pair: what lanes that feed no pair read)
    HIP_TRY(ctx, hipMalloc(&T.d_tok, ((size_t)T.total_blocks + 1) * 16));
    HIP_TRY(ctx, hipMemsetAsync(T.d_tok + T.total_blocks, 0, 16, ctx->stream));
    HIP_TRY(ctx, hipMalloc(&T.d_pair_off, T.pair_blocks_prefix.size() * 4));
    // (the host vector lives as long as the database: no wait needed for the copy)
    HIP_TRY(ctx, hipMemcpyAsync(T.d_pair_off, T.pair_blocks_prefix.data(), T.pair_blocks_prefix.size() * 4,
                                hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, swg_launch_build_tokens(db->d_codes, db->d_code_off, db->d_lens, T.d_pair_off, n_pairs, T.total_blocks,
                                         T.d_tok, ctx->stream));
    T.ok = true;
    return SWG_OK;
}

// Test hook (not part of the public ABI, declared in swg_host_internal.h): the pair-token image of
// a resident database as the device built it (from_host = 0) or as the host restatement of the
// same layout builds it (from_host = 1).  *n_dwords = size of the image; copied when it fits cap.
extern "C" int swg_debug_pair_tokens(swg_ctx *ctx, swg_db *db, int from_host, uint32_t *out, size_t cap_dwords,
                                     size_t *n_dwords)
{
    if (!ctx || !db || !n_dwords) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "swg_debug_pair_tokens: NULL argument");
    *n_dwords = 0;
    if (from_host) {
        std::unique_ptr<uint32_t[]> tok;
        std::vector<uint32_t> off;
        size_t n = 0;
        try {
            if (swg_build_pair_tokens(db, &tok, &n, &off) != 0)
                return swg_set_ctx_error(ctx, SWG_ERR_ARG, "swg_debug_pair_tokens: database too large for pair tokens");
        } catch (const std::exception &) {
            return swg_set_ctx_error(ctx, SWG_ERR_NOMEM, "swg_debug_pair_tokens: out of host memory");
        }
        *n_dwords = n;
        if (out && n <= cap_dwords) memcpy(out, tok.get(), n * 4);
        return SWG_OK;
    }
    if (db->device != ctx->device || !db->d_codes)
        return swg_set_ctx_error(ctx, SWG_ERR_STATE, "swg_debug_pair_tokens: database is not resident");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int rc = ensure_pair_tokens(ctx, db);
    if (rc != SWG_OK) return rc;
    if (!db->ptok.ok) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "swg_debug_pair_tokens: database too large for pair tokens");
    const size_t n = (size_t)db->ptok.total_blocks * 4;
    *n_dwords = n;
    if (out && n <= cap_dwords && n) {
        HIP_TRY(ctx, hipMemcpyAsync(out, db->ptok.d_tok, n * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    return SWG_OK;
}

// Classes take their pairs off a work queue (several passes: one launch per pass, the rows' edges
// go from launch to launch through memory); fixed streams only on request or when the database is
// too large for the queue's 32-bit row indices.
static bool diag_class_is_dynamic(const swg_ctx *ctx, const swg_db *db, const SwgDiagPlan &pl)
{
    if (ctx->opt_dynamic == 0 || !db->ptok.ok) return false;
    return pl.npass == 1 || db->ptok.total_blocks < (1ull << 30);
}

// The cells a class runs on (CellsDiag FORM): packed f16 and the wide form exist in the work-queue kernels
// (the wide form also in the fixed-stream one).
static int diag_class_form(const swg_ctx *ctx, const swg_db *db, const SwgDiagPlan &pl)
{
    if (pl.f16 && diag_class_is_dynamic(ctx, db, pl)) return pl.gapless ? 3 : 2;
    return pl.wide ? 1 : 0;
}

// The f16 cells of a class pair the two sequences' scores with v_pk_fma_f16 (the planner's choice, SwgDiagPlan::fma);
// its profile layout: (score, 1.0) dwords, 2 columns per chunk.
static bool diag_class_fma(const swg_ctx *ctx, const swg_db *db, const SwgDiagPlan &pl)
{
    return pl.fma && diag_class_form(ctx, db, pl) == 2;
}

// An integer 0..2048 as an f16 bit pattern (exact), in both halves of a dword.
static uint32_t f16x2_of(int v)
{
    uint32_t b = 0;
    if (v > 0) {
        int e = 0;
        while ((v >> (e + 1)) != 0) ++e; // floor(log2 v), <= 11
        const uint32_t mant = (e <= 10 ? (uint32_t)v << (10 - e) : (uint32_t)v >> (e - 10)) & 0x3FFu;
        b = ((uint32_t)(e + 15) << 10) | mant;
    }
    return b | (b << 16);
}

// Workgroups to launch for class c.  Work-queue kernels are persistent: a workgroup that is not
// resident from the start only gets in when another one has run out of pairs, so when the long
// class runs beside the bulk the bulk leaves it its wave slots (one per SIMD per long workgroup).
static int diag_class_workgroups(const swg_ctx *ctx, const swg_db *db, const SwgDiagWork &wk, int c)
{
    const SwgDiagPlan &pl = wk.plan[c];
    if (c != 0 || !diag_class_is_dynamic(ctx, db, pl)) return pl.workgroups;
    const SwgKernelInfo info = swg_diag_variant_info(pl.variant);
    const size_t lds = swg_diag_dyn_lds_bytes(pl.K, pl.G, pl.W, diag_class_fma(ctx, db, pl));
    const int per_cu = swg_workgroups_per_cu(info.max_waves, pl.W, lds);
    if (ctx->opt_wave_budget > 0 && wk.n_classes == 1) // experiment: more resident wavefronts than the planner's 16 per CU
        return std::max(1, ctx->n_cu * swg_workgroups_per_cu((int)ctx->opt_wave_budget, pl.W, lds));
    const int capacity = ctx->n_cu * per_cu;
    int displaced = 0;
    if (wk.n_classes == 2 && diag_class_is_dynamic(ctx, db, wk.plan[1]))
        displaced = (wk.plan[1].workgroups * wk.plan[1].W + pl.W - 1) / pl.W;
    int wgs = std::min(pl.workgroups, capacity - displaced);
    // three wavefronts per SIMD issue as fast as four and leave the scheduler more room: measured
    // (round 2 kernels, uniform database, tools/sweeps/r2_occ.sh) +1.3 % at K=16, level at K=20 and 23, +1.1 % at K=24
    if (wk.n_classes == 1 && pl.K >= 16 && pl.W == 4 && per_cu == 4) wgs = std::min(wgs, ctx->n_cu * 3);
    return std::max(1, wgs);
}

// 4-row token blocks and lane groups of class c, for the statistics
static uint64_t diag_class_blocks(const swg_ctx *ctx, const swg_db *db, const SwgDiagWork &wk, int c)
{
    if (!diag_class_is_dynamic(ctx, db, wk.plan[c])) return db->diag[c].total_blocks;
    return (uint64_t)db->ptok.pair_blocks_prefix[wk.pair_end[c]] - db->ptok.pair_blocks_prefix[wk.pair_begin[c]];
}
static uint32_t diag_class_streams(const swg_ctx *ctx, const swg_db *db, const SwgDiagWork &wk, int c)
{
    if (!diag_class_is_dynamic(ctx, db, wk.plan[c])) return db->diag[c].n_streams;
    return (uint32_t)(diag_class_workgroups(ctx, db, wk, c) * wk.plan[c].W * (64 / wk.plan[c].G));
}

static int ensure_scratch(swg_ctx *ctx, size_t dwords)
{
    if (dwords <= ctx->d_scratch_cap) return SWG_OK;
    (void)hipFree(ctx->d_scratch);
    ctx->d_scratch = nullptr;
    ctx->d_scratch_cap = 0;
    HIP_TRY(ctx, hipMalloc(&ctx->d_scratch, dwords * 4));
    ctx->d_scratch_cap = dwords;
    return SWG_OK;
}


// ---------------------------------------------------------------------------
// diagonal engine: make a work plan resident, launch it
// ---------------------------------------------------------------------------
// Which profile buffer a class reads: every class has its own ([3] the bulk, [2] the long class) -- a
// lane's slice is its K columns padded to whole chunks, its rows swizzled by the lane's position in a
// group of G: the layout depends on (K, G).  ([0] and [1] are the systolic engine's, in plain order.)
static int diag_profile_slot(const SwgDiagPlan &, int cls) { return cls == 0 ? 3 : 2; }

// The edges of the rows between consecutive passes of a work-queue fill, ping-pong: one of the three buffer pairs of
// SwgPairTokens, `block_bytes` per 4-row token block, allocated for the token blocks of the database (*cap_blocks), and
// again when a re-filled database has grown.
template <class E> static int ensure_edge_pair(swg_ctx *ctx, const SwgPairTokens &T, E *(&d_edge)[2], uint64_t *cap_blocks, size_t block_bytes)
{
    if (d_edge[0] && *cap_blocks >= T.total_blocks) return SWG_OK;
    (void)hipFree(d_edge[0]);
    (void)hipFree(d_edge[1]);
    d_edge[0] = d_edge[1] = nullptr;
    const size_t bytes = std::max<size_t>(8, (size_t)T.total_blocks * block_bytes);
    HIP_TRY(ctx, hipMalloc(&d_edge[0], bytes));
    HIP_TRY(ctx, hipMalloc(&d_edge[1], bytes));
    *cap_blocks = T.total_blocks;
    return SWG_OK;
}
// the 16-bit kernels' (M,B) per row (prepare_diag and the list re-run)
static int ensure_edges(swg_ctx *ctx, SwgPairTokens *T) { return ensure_edge_pair(ctx, *T, T->d_edge, &T->edge_blocks, 4 * sizeof(uint2)); }

// A gap magnitude as the cells of `form` take it, in both halves of a dword: an f16 integer (form 2) or 16 bits.
static uint32_t gap_word(int form, int gap)
{
    const uint32_t m = (uint32_t)(-gap) & 0xFFFFu;
    return form == 2 ? f16x2_of(-gap) : m | (m << 16);
}

// What every work-queue kernel (P: SwgDiagDynParams, SwgDiagQ32Params, SwgDiagQQParams) is told the same way, the rest
// zero: the pair tokens and their offsets, the lane-group width, the turn levels (three beside a second class, else
// four) and the per-SIMD rank words.
template <class P> static P token_params(const SwgPairTokens &T, int G, int n_classes, uint32_t *simd_ranks)
{
    P q;
    memset(&q, 0, sizeof q);
    q.tok = T.d_tok;
    q.zero_block = (uint32_t)T.total_blocks;
    q.pair_off = T.d_pair_off;
    q.G = (uint32_t)G;
    q.turn_levels = n_classes == 2 ? 3u : 4u;
    q.simd_ranks = simd_ranks;
    return q;
}

// ... and every launch of swg_diag_dyn_kernel besides: the score array of n_slots entries and its pair limit, the gap
// words of the cells `form`.
static SwgDiagDynParams dyn_params_base(const SwgPairTokens &T, int32_t *scores, size_t n_slots, int G, int form, int go, int ge,
                                        int n_classes, uint32_t *simd_ranks)
{
    SwgDiagDynParams q = token_params<SwgDiagDynParams>(T, G, n_classes, simd_ranks);
    q.scores = scores;
    q.pair_limit = (uint32_t)(n_slots / 2);
    q.go = gap_word(form, go);
    q.ge = gap_word(form, ge);
    return q;
}

// The bulk's priority threshold: an item (pair, or sequence) of at least this many token blocks runs at raised
// priority -- one that alone is well above an average lane group's whole share of the class's `blocks`: prio_share
// percent of it, times `factor`; never fewer than 8 blocks.
static uint32_t bulk_prio_blocks(const swg_ctx *ctx, uint64_t blocks, uint64_t groups, double factor = 1.0)
{
    return (uint32_t)std::max<uint64_t>(8, (uint64_t)(ctx->opt_prio_share * 0.01 * factor * (double)blocks / (double)std::max<uint64_t>(1, groups)));
}

// The launches of one pass over the pairs [begin, end).  The form with edges addresses a launch's tokens and edges by
// 32-bit offsets: where the token buffer spans more than seg_blocks, the pairs go in several launches per pass, each
// over a run of consecutive pairs (a segment) and addressing the buffer from its segment's origin (*cut) -- also where
// this range fits one segment and only the whole buffer does not: the bulk behind a long class begins far from block 0.
// Normally there is one run, the whole range.  False: one pair alone is beyond a segment.
static bool token_segments(const SwgPairTokens &T, uint32_t begin, uint32_t end, uint32_t seg_blocks, bool edges,
                           std::vector<std::pair<uint32_t, uint32_t>> *segs, bool *cut)
{
    segs->clear();
    *cut = edges && T.total_blocks > seg_blocks;
    if (!*cut) {
        segs->push_back(std::make_pair(begin, end));
        return true;
    }
    const std::vector<uint32_t> &pre = T.pair_blocks_prefix;
    for (uint32_t b = begin; b < end;) {
        const uint64_t limit = (uint64_t)pre[b] + seg_blocks;
        const uint32_t e = (uint32_t)(std::upper_bound(pre.begin() + b, pre.begin() + end + 1, limit,
                                                       [](uint64_t v, uint32_t x) { return v < (uint64_t)x; }) - pre.begin()) - 1u;
        if (e <= b) return false;
        segs->push_back(std::make_pair(b, e));
        b = e;
    }
    return true;
}

static int prepare_diag(swg_ctx *ctx, swg_db *db, const SwgDiagWork &wk)
{
    if (ctx->opt_dynamic) {
        int rc = ensure_pair_tokens(ctx, db);
        if (rc != SWG_OK) return rc;
    }
    for (int c = 0; c < wk.n_classes; ++c) {
        const SwgDiagPlan &pl = wk.plan[c];
        if (!diag_class_is_dynamic(ctx, db, pl)) {
            if (db->tokens_only)
                return swg_set_ctx_error(ctx, SWG_TAKE_HOST_ROUTE, "this search needs fixed streams, which a database built from 16-lane batches does not have");
            int rc = ensure_diag_layout(ctx, db, c, pl, wk.pair_begin[c], wk.pair_end[c]);
            if (rc != SWG_OK) return rc;
        } else if (pl.npass > 1) {
            int rc = ensure_edges(ctx, &db->ptok);
            if (rc != SWG_OK) return rc;
        }
        // (the f16 cells with the fma pairing: (score, 1.0) dwords in 2-column chunks, K padded to 2 columns)
        const bool fma = diag_class_fma(ctx, db, pl);
        const int kp = swg_diag_padded_cols(pl.K, fma);
        // (a last pass with a geometry of its own: its slice follows the other passes' in the same buffer)
        const bool own_last = pl.npass > 1 && pl.last_variant >= 0 && diag_class_is_dynamic(ctx, db, pl);
        const int kp_last = own_last ? swg_diag_padded_cols(pl.last_K, fma) : kp;
        const uint32_t tail = own_last ? (uint32_t)(pl.G * kp_last) : 0u;
        const uint32_t ncols = (uint32_t)((pl.npass - (own_last ? 1 : 0)) * pl.G * kp) + tail;
        const uint32_t qcol0 = (uint32_t)((pl.npass - 1) * pl.G * pl.K);
        int rc = ensure_profile_cols(ctx, diag_profile_slot(pl, c), ncols, fma ? 4 : 2,
                                     (1ull << 55) | ((uint64_t)fma << 51) | ((uint64_t)pl.K << 40) | ((uint64_t)pl.G << 32) | (uint64_t)ncols,
                                     pl.K, kp, fma ? 2 : 4, SWG_LDS_SWIZZLE ? pl.G : 0, diag_class_form(ctx, db, pl) >= 2, tail, pl.last_K,
                                     kp_last, qcol0);
        if (rc != SWG_OK) return rc;
        if (pl.f16_from > 0) { // both forms in this class: the f16 cells' profile of the same geometry (v_perm_b32 pairing)
            rc = ensure_profile_cols(ctx, 7, ncols, 2, (1ull << 55) | ((uint64_t)pl.K << 40) | ((uint64_t)pl.G << 32) | (uint64_t)ncols,
                                     pl.K, kp, 4, SWG_LDS_SWIZZLE ? pl.G : 0, 1, tail, pl.last_K, kp_last, qcol0);
            if (rc != SWG_OK) return rc;
        }
    }
    return SWG_OK;
}

// The queue's zones for one launch over pairs [q->q_begin, q->q_end) (see the kernel's event code): the pairs of at most
// N token blocks (see below) -- lengths do not increase along the range -- are claimed opt_batch at a time, except
// the last two per lane group, which go out one by one again so that the lane groups still end together (a claim of
// B pairs is B times the granularity of the hand-out).  Whole batches only; shard c's first U1 requests are single.
static void dyn_batch_zones(const swg_ctx *ctx, const SwgPairTokens &T, SwgDiagDynParams *q, uint64_t groups, int K, int G, int form)
{
    q->batch_u1 = q->batch_u2 = q->batch_B = 0u;
    const uint32_t B = (uint32_t)ctx->opt_batch;
    if (B <= 1u || q->list || q->q_end <= q->q_begin) return;
    const std::vector<uint32_t> &pre = T.pair_blocks_prefix;
    // "Short" is a time, not a length: a request costs ~2.2 us, so batches pay where a whole pair takes a few tens of
    // microseconds -- and a claim of B pairs is B pair-times taken out of the balance at the end of the launch.  A 4-row
    // block costs 4 x (instructions per row) x 4.06 cycles of its SIMD, shared with the other wavefronts on it: 1.3 us
    // at K = 2, 3 us at K = 8, 7 us at K = 32 (three wavefronts).  Pairs of at most 40 us count as short: 30 blocks at
    // K = 2, 13 at K = 8, 5 at K = 32.  (Measured, round 4: a fixed 32 blocks cost config 3 -- K = 32 -- 6 %: 2 300
    // claims of eight 30-block pairs, 1.5 ms of work each, ended after everybody else.)  Option batch_blocks > 0 overrides.
    uint32_t N = (uint32_t)std::min<long>(ctx->opt_batch_blocks, 1l << 30);
    if (ctx->opt_batch_blocks <= 0) {
        const double waves_per_simd = std::min(4.0, std::max(1.0, (double)groups * G / 64.0 / (4.0 * ctx->n_cu)));
        const double block_us = 4.0 * ((form == 3 ? 3.5 : form == 2 ? 8.5 : 10.0) * K + 30.0) * 4.06 * waves_per_simd / 2.4e3;
        N = (uint32_t)std::max(2.0, 40.0 / block_us);
    }
    uint32_t lo = q->q_begin, hi = q->q_end; // first pair with at most N blocks
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (pre[mid + 1] - pre[mid] <= N) hi = mid; else lo = mid + 1u;
    }
    const uint64_t tail = std::min<uint64_t>(q->q_end - lo, 2ull * groups);
    const uint64_t to = (uint64_t)q->q_end - tail;
    const uint64_t u1 = ((uint64_t)(lo - q->q_begin) + SWG_DYN_SHARDS - 1u) / SWG_DYN_SHARDS;
    const uint64_t p1 = (uint64_t)q->q_begin + SWG_DYN_SHARDS * u1;
    if (to <= p1) return;
    const uint64_t u2 = (to - p1) / ((uint64_t)SWG_DYN_SHARDS * B);
    if (u2 == 0u) return;
    q->batch_u1 = (uint32_t)u1;
    q->batch_u2 = (uint32_t)u2;
    q->batch_B = B;
}

// One class's fill off the work queue, launch by launch: what every launch of the class shares (dyn_fill_begin sets it
// up), and the launch itself.  The pruned and the unpruned loop both go through launch().
struct DynFill {
    swg_ctx *ctx;
    const swg_db *db;
    const SwgDiagWork &wk;
    int c;
    SwgDiagDynParams q;
    hipStream_t qs = nullptr;
    int form = 0;
    bool edges = false, fma = false, cut = false;
    size_t slice = 0;
    std::vector<std::pair<uint32_t, uint32_t>> segs; // pair ranges (token_segments)
    bool first_launch = true;
    int launches = 0, f16_launches = 0;

    // one launch: pass `pass` over the pairs [b, en) of segment sg on the cells pform
    int launch(int pass, const std::pair<uint32_t, uint32_t> &sg, uint32_t b, uint32_t en, int pform, const uint8_t *prof, bool f16_part)
    {
        const SwgDiagPlan &pl = wk.plan[c];
        const SwgPairTokens &T = db->ptok;
        // one launch per pass: the kernel boundary is what lets any lane group take any pair
        q.profile = prof + (size_t)pass * slice;
        q.edge_in = pass > 0 ? T.d_edge[(pass - 1) & 1] : nullptr;
        q.edge_out = pass + 1 < pl.npass ? T.d_edge[pass & 1] : nullptr;
        if (!first_launch)
            HIP_TRY(ctx, hipMemsetAsync(q.queue, 0, (size_t)SWG_DYN_SHARDS * SWG_DYN_SHARD_STRIDE * 4, qs));
        first_launch = false;
        q.q_begin = b;
        q.q_end = en;
        if (cut) {
            q.seg_origin = T.pair_blocks_prefix[sg.first];
            q.seg_blocks = T.pair_blocks_prefix[sg.second] - q.seg_origin;
        }
        const int variant = pass + 1 == pl.npass && pl.npass > 1 && pl.last_variant >= 0 ? pl.last_variant : pl.variant;
        const int wgs_c = diag_class_workgroups(ctx, db, wk, c);
        // (with long_helps the long class's kernel reads the bulk's counters too, as single pairs: no zones then)
        if (!(ctx->opt_long_helps && wk.n_classes == 2)) dyn_batch_zones(ctx, T, &q, (uint64_t)wgs_c * pl.W * (64 / pl.G), swg_diag_variant_info(variant).K, pl.G, pform);
        HIP_TRY(ctx, swg_launch_diag_dyn(variant, edges, pform, pl.W, wgs_c, q, qs, 1, fma));
        ++launches;
        if (f16_part) ++f16_launches;
        return SWG_OK;
    }
};

static int dyn_fill_begin(DynFill *F, int go, int ge, uint64_t *d_trace)
{
    swg_ctx *ctx = F->ctx;
    const swg_db *db = F->db;
    const SwgDiagWork &wk = F->wk;
    const int c = F->c;
    const SwgDiagPlan &pl = wk.plan[c];
    const SwgPairTokens &T = db->ptok;
    SwgDiagDynParams &q = F->q;
    F->form = diag_class_form(ctx, db, pl);
    q = dyn_params_base(T, db->d_scores, (size_t)db->n_bins * SWG_BIN, pl.G, F->form, go, ge, wk.n_classes, db->d_counters + SWG_RANK_WORD(c));
    q.q_begin = (uint32_t)wk.pair_begin[c];
    q.q_end = (uint32_t)wk.pair_end[c];
    q.queue = db->d_counters + SWG_QUEUE_WORD(c); // zeroed with the other counters before the fill
    q.profile = ctx->d_profile[diag_profile_slot(pl, c)];
    // the long class always runs at raised priority; in the bulk, a pair that alone is well
    // above an average lane group's whole share
    auto bulk_prio = [&]() -> uint32_t {
        const uint64_t blocks = T.pair_blocks_prefix[wk.pair_end[0]] - T.pair_blocks_prefix[wk.pair_begin[0]];
        return bulk_prio_blocks(ctx, blocks, (uint64_t)diag_class_workgroups(ctx, db, wk, 0) * wk.plan[0].W * (64 / wk.plan[0].G));
    };
    q.prio_blocks = c == 1 ? 0u : bulk_prio();
    if (c == 1 && ctx->opt_long_helps && diag_class_is_dynamic(ctx, db, wk.plan[0])) {
        // when the long pairs are done their lane groups go on with the bulk's queue
        q.q2_begin = (uint32_t)wk.pair_begin[0];
        q.q2_end = (uint32_t)wk.pair_end[0];
        q.queue2 = db->d_counters + SWG_QUEUE_WORD(0);
        q.prio_blocks2 = bulk_prio();
    }
    // (f16 sums round to nearest: a computed 32768 needs a true score within a few units of it)
    q.f16_wipe = ctx->cur->plan.score_bound >= 32000ull ? 1u : 0u;
    q.trace = d_trace;
    q.stamps = pl.npass == 1 ? reinterpret_cast<unsigned long long *>(db->d_counters + SWG_WORD_STAMPS(c)) : nullptr; // (single-pass launches only)
    F->edges = pl.npass > 1 || F->form == 1;
    F->fma = diag_class_fma(ctx, db, pl); // (never with a split: its f16 part takes the v_perm_b32 profile)
    F->slice = swg_diag_slice_bytes(pl.K, pl.G, F->fma);
    F->qs = c == 1 ? ctx->stream2 : ctx->stream;
    if (!token_segments(T, q.q_begin, q.q_end, ctx->opt_seg_blocks, F->edges, &F->segs, &F->cut))
        return swg_set_ctx_error(ctx, SWG_ERR_ARG, "a pair of sequences too long for the multi-pass fill");
    q.seg_origin = 0;
    q.seg_blocks = (uint32_t)std::min<uint64_t>(T.total_blocks, ctx->opt_seg_blocks);
    if (F->cut) {
        q.q2_begin = q.q2_end = 0; // (the other class's pairs lie outside a segment)
        q.queue2 = nullptr;
    }
    return SWG_OK;
}

// The walk of the level of row i of SWG_REFINE_LEVEL over the pairs of [begin, end) whose bound reaches *d_thr, in S
// segments of the level's table: blocks of the table's k over the pairs every earlier level has left at or above that
// word.  The fifth level's walk is a kernel of its own: the same blocks over both k = 5 tables, the columns between two
// blocks charged.
static hipError_t launch_refine_level(swg_ctx *ctx, const SwgPairTokens &T, int i, uint32_t begin, uint32_t end, int S, const uint32_t *d_thr,
                                      uint32_t *d_bound, hipStream_t qs)
{
    const SwgRefineLevel &L = SWG_REFINE_LEVEL[i];
    const SwgKmerTable &t = ctx->kmer_refine[i];
    if (L.reads >= 0)
        return swg_launch_pair_bound_refine5(T.d_tok, T.d_pair_off, begin, end, ctx->prune_colmax, ctx->kmer_refine[L.reads].d, t.d, (uint32_t)ctx->query_len(),
                                             (uint32_t)-(long)ctx->gap_extend, d_thr, d_bound, qs);
    return swg_launch_pair_bound_refine(T.d_tok, T.d_pair_off, begin, end, (uint32_t)S, ctx->prune_colmax, t.d, t.bits, d_thr, d_bound, qs, L.k);
}

// The fill of a pruned search, stage by stage -- all passes of a stage, then the threshold so far and the
// next stage's cut, all on the fill's stream with no host wait.  The bound of every pair first -- unless the list queues
// the first level with a stage (the gate: behind that stage's threshold, for the pairs from it on) --; then the stages of
// swg_prune_stages, each behind what that list queues in front of it and nothing else: the K-th best score so far (every
// entry of d_scores is at most its sequence's true score at a kernel boundary) or, once, a caller's threshold; then the
// stage's cut, held for all its passes.
// A cut stage's launches are LIST launches: the kernel reads the list's device-side length once at entry, leaves before
// it loads the profile when it is 0, and hands out exactly those pairs in every pass (no batch claims in list mode).  So
// the fill kernels are the unpruned search's, instruction for instruction.  The prefix cut's list is the pair ids in
// order, from the stage's first pair, and its length is the cut.  Pair by pair (the default): the second-level bound of
// the stage's pairs that still reach the threshold (and the third level's of those that reach it after that), then the stage's own list -- the ids of its pairs whose bound reaches
// T, in order.  Under a caller's threshold the first of SEVERAL stages -- the longest pairs, whose bounds stand furthest
// above any T -- is walked a second time only where the first level cut an eighth of it: the gate's word is its T.
// (The tables are this epoch's: prepare_prune queued their builds on this stream.)
static int enqueue_pruned_fill(swg_ctx *ctx, swg_db *db, const SwgPrunePlan &pr, size_t k, DynFill *F)
{
    const SwgPairTokens &T = db->ptok;
    const SwgDiagPlan &pl = F->wk.plan[F->c];
    hipStream_t qs = F->qs;
    uint32_t *thr = db->d_counters + SWG_PRUNE_WORD_T, *cut_word = db->d_counters + SWG_PRUNE_WORD_CUT, *gate = db->d_counters + SWG_PRUNE_WORD_GATE;
    const uint32_t n_pairs = (uint32_t)swg_db_pair_count(db);
    const SwgPruneLayout L = swg_prune_layout(db->d_pair_bound, n_pairs);
    // (a caller's threshold stands in its word before anything reads it)
    if (pr.fixed) HIP_TRY(ctx, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(thr), (int)pr.fixed_T, 1, qs));
    const std::vector<SwgPruneStage> stages = swg_prune_stages(pr, F->segs);
    // the first level of the pairs [b, en): gated by the threshold word, or (gated_by null) of every pair from the first
    // (only a segmented k-mer bound is ever gated: swg_prune_gate_choice; the other forms would bound [0, en) ungated)
    auto first_level = [&](uint32_t b, uint32_t en, const uint32_t *gated_by) -> int {
        if (pr.kmer > 1 && pr.segments > 1)
            HIP_TRY(ctx, swg_launch_pair_bound_kmer_seg(T.d_tok, T.d_pair_off, b, en, pr.kmer, (uint32_t)pr.segments, ctx->prune_colmax, ctx->kmer_first[pr.kmer - 4].d,
                                                        ctx->kmer_first[pr.kmer - 4].bits, gated_by, L.bounds, L.ids, qs));
        else if (pr.kmer > 1)
            HIP_TRY(ctx, swg_launch_pair_bound_kmer(T.d_tok, T.d_pair_off, en, pr.kmer, ctx->prune_colmax, ctx->kmer_first[pr.kmer - 4].d,
                                                    ctx->kmer_first[pr.kmer - 4].bits, L.bounds, L.ids, qs));
        else
            HIP_TRY(ctx, swg_launch_pair_bound(T.d_tok, T.d_pair_off, en, ctx->prune_colmax, L.bounds, L.ids, qs));
        return SWG_OK;
    };
    // Where no stage queues the first level, every pair is bounded here; where one does, the pairs in front of that
    // stage are launched unpruned and their words say "not bounded" (swg_prune_bound_range).
    const SwgPruneBoundRange br = swg_prune_bound_range(stages, n_pairs);
    if (br.stage == stages.size()) {
        const int rc = first_level(br.begin, br.end, nullptr);
        if (rc != SWG_OK) return rc;
    } else if (br.skip_end > br.skip_begin)
        HIP_TRY(ctx, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(L.bounds + br.skip_begin), (int)SWG_PRUNE_NOT_BOUNDED, br.skip_end - br.skip_begin, qs));
    db->prune_stages.clear(); // (the stages cut pair by pair, for the tests)
    for (const SwgPruneStage &st : stages) {
        if (st.queued & SWG_STAGE_THRESHOLD)
            HIP_TRY(ctx, swg_launch_prune_threshold(db->d_scores, db->d_order, (uint32_t)((size_t)db->n_bins * SWG_BIN), (uint32_t)k, db->d_hist, thr, qs));
        if (st.queued & SWG_STAGE_BOUND) {
            const int rc = first_level(br.begin, br.end, thr);
            if (rc != SWG_OK) return rc;
        }
        if (st.queued & SWG_STAGE_PREFIX_CUT) HIP_TRY(ctx, swg_launch_prune_cut(L.bounds, T.d_pair_off, st.begin, st.end, thr, cut_word, qs));
        if (st.queued & SWG_STAGE_GATE) HIP_TRY(ctx, swg_launch_prune_refine_gate(L.bounds, st.begin, st.end, thr, gate, qs));
        // (the levels behind the first, in their order and under one word: a gated stage skips all the walks together)
        for (int i = 0; i < SWG_REFINE_LEVELS; ++i)
            if (st.queued & SWG_REFINE_LEVEL[i].stage_bit)
                HIP_TRY(ctx, launch_refine_level(ctx, T, i, st.begin, st.end, pr.refine[i], st.queued & SWG_STAGE_GATE ? gate : thr, L.bounds, qs));
        if (st.queued & SWG_STAGE_LIST) {
            const size_t rec = db->prune_stages.size() / 2;
            HIP_TRY(ctx, swg_launch_prune_list(L.bounds, T.d_pair_off, st.begin, st.end, thr, L.tiles, L.lists + st.begin, cut_word,
                                               rec < SWG_PRUNE_STAGE_RECS ? L.recs + 2 * rec : nullptr, qs));
            db->prune_stages.push_back(st.begin), db->prune_stages.push_back(st.end);
        }
        F->q.list = st.queued & SWG_STAGE_PREFIX_CUT ? L.ids + st.begin : st.queued & SWG_STAGE_LIST ? L.lists + st.begin : nullptr;
        F->q.list_count = F->q.list ? cut_word : nullptr;
        for (int pass = 0; pass < pl.npass; ++pass) {
            const int rc = F->launch(pass, F->segs[st.segment], st.begin, st.end, F->form, ctx->d_profile[diag_profile_slot(pl, F->c)], false);
            if (rc != SWG_OK) return rc;
        }
    }
    F->q.list = nullptr, F->q.list_count = nullptr;
    return SWG_OK;
}

// Launches the fill of one work plan.  Events: ev[1] before, ev[2] after on the main stream;
// with a long class also ev[5] (bulk end) and ev[7] (long end).
// prune (or null: the whole range, pass by pass): a pruned search runs stage by stage (enqueue_pruned_fill).
static int launch_diag(swg_ctx *ctx, swg_db *db, const SwgDiagWork &wk, int go, int ge, bool *two_ends,
                       const SwgPrunePlan *prune = nullptr, size_t prune_k = 0)
{
    hipStream_t s = ctx->stream;
    *two_ends = false;
    // diagnostics: SWG_TRACE=<file> dumps one line per wavefront (class, workgroup, wave, start and
    // end in 10 ns ticks, blocks of its longest stream) for every diagonal fill
    static const char *trace_path = getenv("SWG_TRACE");
    uint64_t *d_trace[2] = {nullptr, nullptr};
    if (trace_path)
        for (int c = 0; c < wk.n_classes; ++c) {
            const size_t bytes = (size_t)wk.plan[c].workgroups * wk.plan[c].W * 4 * 8;
            HIP_TRY(ctx, hipMalloc(&d_trace[c], bytes));
            HIP_TRY(ctx, hipMemsetAsync(d_trace[c], 0, bytes, s));
        }
    HIP_TRY(ctx, hipEventRecord(ctx->cur->ev[1], s));
    // the long pairs start first, on their own stream, beside the bulk
    int rf = fork_long_class(ctx, wk);
    if (rf != SWG_OK) return rf;
    for (int c = wk.n_classes - 1; c >= 0; --c) {
        const SwgDiagLayout &L = db->diag[c];
        const SwgDiagPlan &pl = wk.plan[c];
        if (diag_class_is_dynamic(ctx, db, pl)) {
            DynFill F{ctx, db, wk, c};
            int rc = dyn_fill_begin(&F, go, ge, d_trace[c]);
            if (rc != SWG_OK) return rc;
            // Both 16-bit forms in one class (pl.f16_from, see plan_search): the pairs before it -- the longest --
            // take all their passes on the wide form, then the rest theirs on the f16 cells, the same geometry
            // throughout; ev[5] between the two parts tells their times apart.
            const uint32_t class_begin = F.q.q_begin, class_end = F.q.q_end;
            const bool split = c == 0 && wk.n_classes == 1 && F.form != 2 && pl.f16_from > class_begin && pl.f16_from < class_end;
            // (plan_prune decided; what swg_prune_last reports is what was launched)
            const bool pruned = prune && prune->on && c == 0 && wk.n_classes == 1 && !split && db->d_pair_bound;
            if (c == 0) ctx->cur->pruned = pruned;
            if (pruned) {
                if ((rc = enqueue_pruned_fill(ctx, db, *prune, prune_k, &F)) != SWG_OK) return rc;
            } else
            for (int part = 0; part < (split ? 2 : 1); ++part) {
                const int pform = split && part == 1 ? 2 : F.form;
                const uint32_t part_begin = split && part == 1 ? pl.f16_from : class_begin;
                const uint32_t part_end = split && part == 0 ? pl.f16_from : class_end;
                const uint8_t *prof = ctx->d_profile[split && part == 1 ? 7 : diag_profile_slot(pl, c)];
                F.q.go = gap_word(pform, go);
                F.q.ge = gap_word(pform, ge);
                if (split && part == 1) HIP_TRY(ctx, hipEventRecord(ctx->cur->ev[5], F.qs));
                for (int pass = 0; pass < pl.npass; ++pass) {
                    for (const std::pair<uint32_t, uint32_t> &sg : F.segs) {
                        const uint32_t b = std::max(sg.first, part_begin), en = std::min(sg.second, part_end);
                        if (b >= en) continue;
                        if ((rc = F.launch(pass, sg, b, en, pform, prof, split && part == 1)) != SWG_OK) return rc;
                    }
                }
            }
            if (c == 0) ctx->cur->fill_launches = F.launches, ctx->cur->fill_f16_launches = F.f16_launches;
            continue;
        }
        SwgDiagParams d;
        memset(&d, 0, sizeof d);
        d.tok = L.d_tok;
        d.stream_off = L.d_stream_off;
        d.stream_pairs = L.d_stream_pairs;
        d.stream_pair_off = L.d_stream_pair_off;
        d.n_streams = L.n_streams;
        d.profile = ctx->d_profile[diag_profile_slot(pl, c)];
        d.scores = db->d_scores;
        d.scratch = L.d_scratch;
        d.npass = (uint32_t)pl.npass;
        d.G = (uint32_t)pl.G;
        d.go = gap_word(0, go);
        d.ge = gap_word(0, ge);
        // wavefronts on the critical path get issue priority over the ones they share a SIMD
        // with: all of the long class; in the bulk, streams that hold little more than one very
        // long pair
        const double mean_blocks = (double)L.total_blocks / std::max<uint32_t>(1, L.n_streams);
        d.prio_blocks = c == 1 ? 0u
                        : (double)L.max_stream_blocks > 1.1 * mean_blocks ? (uint32_t)(0.75 * (double)L.max_stream_blocks)
                                                                          : 0xFFFFFFFFu;
        d.trace = d_trace[c];
        HIP_TRY(ctx, swg_launch_diag(pl.variant, pl.npass > 1, pl.wide != 0, pl.W, pl.workgroups, pl.lds_bytes, d,
                                     c == 1 ? ctx->stream2 : s));
    }
    // the end of the fill is the later of the two kernels' ends
    rf = join_long_class(ctx, wk, true);
    if (rf != SWG_OK) return rf;
    *two_ends = wk.n_classes == 2;
    HIP_TRY(ctx, hipEventRecord(ctx->cur->ev[2], s));
    if (trace_path) {
        HIP_TRY(ctx, hipStreamSynchronize(s));
        FILE *f = fopen(trace_path, "a");
        if (f) fprintf(f, "# fill K=%d G=%d W=%d wgs=%d classes=%d\n", wk.plan[0].K, wk.plan[0].G, wk.plan[0].W,
                       wk.plan[0].workgroups, wk.n_classes);
        for (int c = 0; c < wk.n_classes; ++c) {
            const size_t n = (size_t)wk.plan[c].workgroups * wk.plan[c].W;
            std::vector<uint64_t> h(n * 4);
            HIP_TRY(ctx, hipMemcpy(h.data(), d_trace[c], n * 32, hipMemcpyDeviceToHost));
            (void)hipFree(d_trace[c]);
            for (size_t i = 0; f && i < n; ++i)
                fprintf(f, "%d %zu %zu %llu %llu %llu %llu\n", c, i / wk.plan[c].W, i % wk.plan[c].W,
                        (unsigned long long)h[4 * i], (unsigned long long)h[4 * i + 1], (unsigned long long)h[4 * i + 2],
                        (unsigned long long)h[4 * i + 3]);
        }
        if (f) fclose(f);
    }
    return SWG_OK;
}

static int diag_fill_ms(swg_ctx *ctx, bool two_ends, double *out)
{
    float ms = 0.f;
    HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->cur->ev[1], ctx->cur->ev[2]));
    *out = ms;
    if (two_ends) {
        float a = 0.f, b = 0.f;
        HIP_TRY(ctx, hipEventElapsedTime(&a, ctx->cur->ev[1], ctx->cur->ev[5]));
        HIP_TRY(ctx, hipEventElapsedTime(&b, ctx->cur->ev[1], ctx->cur->ev[7]));
        *out = std::max(*out, (double)std::max(a, b));
    }
    return SWG_OK;
}

// What every bin-based launch (systolic fill, int32 kernels) is told the same way: the bin image, the scores, the scratch.
static SwgFillParams fill_params_base(const swg_ctx *ctx, const swg_db *db)
{
    SwgFillParams p;
    memset(&p, 0, sizeof p);
    p.residues = db->d_packed;
    p.bin_off = db->d_bin_off;
    p.bin_nblk = db->d_bin_nblk;
    p.n_bins = db->n_bins;
    p.scores = db->d_scores;
    p.scratch = ctx->d_scratch;
    return p;
}

// Launches the systolic int16/int32 fill of one plan over the whole database (events ev[1], ev[2]).
static int launch_systolic(swg_ctx *ctx, const swg_db *db, const SwgSystolicPlan &pl, int go, int ge)
{
    hipStream_t s = ctx->stream;
    SwgFillParams p = fill_params_base(ctx, db);
    p.profile = ctx->d_profile[pl.bits == 16 ? 0 : 1];
    p.queue = db->d_counters + SWG_WORD_WORK_QUEUE;
    p.n_items = pl.bits == 16 ? db->n_bins : db->n_bins * 2;
    p.npass = (uint32_t)pl.npass;
    if (pl.bits == 16 && pl.f16) {
        p.go = (int32_t)f16x2_of(-go);
        p.ge = (int32_t)f16x2_of(-ge);
    } else if (pl.bits == 16) {
        const uint32_t g = (uint32_t)(-go) & 0xFFFFu, e = (uint32_t)(-ge) & 0xFFFFu;
        p.go = (int32_t)(g | (g << 16));
        p.ge = (int32_t)(e | (e << 16));
    } else {
        p.go = go;
        p.ge = ge;
    }
    p.scratch_wg_dwords = (uint64_t)db->max_nblk * SWG_ROWS_PER_BLK * 64 * pl.info.nb;
    HIP_TRY(ctx, hipEventRecord(ctx->cur->ev[1], s));
    HIP_TRY(ctx, swg_launch_fill(pl.bits, pl.variant, pl.W, pl.workgroups, p, s, pl.bits == 16 && pl.f16));
    HIP_TRY(ctx, hipEventRecord(ctx->cur->ev[2], s));
    return SWG_OK;
}

static int prepare_systolic(swg_ctx *ctx, swg_db *db, const SwgSystolicPlan &pl)
{
    int rc = ensure_bins(ctx, db);
    if (rc != SWG_OK) return rc;
    if ((rc = ensure_profile(ctx, pl)) != SWG_OK) return rc;
    const size_t need = pl.npass > 1 ? (size_t)pl.workgroups * db->max_nblk * SWG_ROWS_PER_BLK * 64 * pl.info.nb : 0;
    return ensure_scratch(ctx, need);
}

// ---------------------------------------------------------------------------
// int32 with a work queue (swg_diag32q_kernel): non-positive gap scores, one pass
// ---------------------------------------------------------------------------
// The bulk's workgroup size where the profile is twice the int16 one (the int32 kernel's, the query pairs'), so that
// LDS, not registers, decides how many workgroups a CU holds: the long class keeps one workgroup of four wavefronts per
// CU, and the bulk takes the smallest workgroup size W (4, 8, 12 or 16 wavefronts sharing one profile) that leaves the
// most wavefronts resident in the LDS that is left, `wave_cap` per CU at most.  forced_W > 0: that size where it fits
// (one class only).  False: not even one workgroup of four fits; *bulk_W and *bulk_per_cu are then 4 and 1.
static bool lds_bound_workgroup(const SwgDiagWork &wk, int wave_cap, long forced_W, int *bulk_W, int *bulk_per_cu)
{
    const SwgDiagPlan &pl = wk.plan[0];
    const SwgKernelInfo info = swg_diag_variant_info(pl.variant);
    size_t room = SWG_LDS_PER_CU;
    int cap_waves = std::min(wave_cap, info.max_waves);
    if (wk.n_classes == 2) {
        room -= std::min(room, swg_diag32q_lds_bytes(wk.plan[1].K, wk.plan[1].G, 4));
        cap_waves = std::min(cap_waves, info.max_waves - 4);
    }
    int best_W = 4, best_n = 1, best_waves = 0;
    for (int W = 4; W <= info.max_waves; W += 4) {
        const size_t lds = swg_diag32q_lds_bytes(pl.K, pl.G, W);
        const int n = std::min<int>((int)(room / lds), cap_waves / W);
        if (n >= 1 && n * W > best_waves) {
            best_waves = n * W;
            best_W = W;
            best_n = n;
        }
    }
    if (forced_W > 0 && forced_W <= info.max_waves && wk.n_classes == 1 && swg_diag32q_lds_bytes(pl.K, pl.G, (int)forced_W) <= room) {
        best_W = (int)forced_W;
        best_n = std::max(1, std::min<int>((int)(room / swg_diag32q_lds_bytes(pl.K, pl.G, best_W)), cap_waves / best_W));
    }
    *bulk_W = best_W;
    *bulk_per_cu = best_n;
    return best_waves > 0;
}

// Occupancy of an int32 work plan: three wavefronts per SIMD, or as many as LDS holds; a plan nothing fits runs one
// workgroup of four per CU.  (Option q32_waves, an experiment: the workgroup size of an int32 launch.)
static void q32_occupancy(const swg_ctx *ctx, const SwgDiagWork &wk, int *bulk_W, int *bulk_per_cu)
{
    (void)lds_bound_workgroup(wk, 12, ctx->opt_q32_waves, bulk_W, bulk_per_cu);
}

// Workgroups of class c over `items` sequences, and (*waves) their size
static int q32_class_workgroups(const swg_ctx *ctx, const SwgDiagWork &wk, int c, uint64_t items, int *waves)
{
    int per_cu = 1;
    *waves = 4;
    if (c == 0) q32_occupancy(ctx, wk, waves, &per_cu);
    const uint64_t per_wg = (uint64_t)*waves * (64 / wk.plan[c].G);
    return (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)ctx->n_cu * per_cu, (items + per_wg - 1) / per_wg));
}

static bool q32_plan_fits(const SwgDiagWork &wk, size_t lq)
{
    if (wk.n_classes < 1) return false;
    for (int c = 0; c < wk.n_classes; ++c) {
        const SwgDiagPlan &pl = wk.plan[c];
        if (pl.npass != 1 || (size_t)pl.G * pl.K < lq || swg_diag32q_lds_bytes(pl.K, pl.G, 4) > SWG_LDS_PER_CU) return false;
    }
    // both classes run side by side on every CU
    if (wk.n_classes == 2 && swg_diag32q_lds_bytes(wk.plan[0].K, wk.plan[0].G, 4) + swg_diag32q_lds_bytes(wk.plan[1].K, wk.plan[1].G, 4) >
                                 SWG_LDS_PER_CU)
        return false;
    return true;
}

// One class of one geometry for the int32 work-queue kernel (workgroups of four wavefronts) over the pairs [0, n_pairs);
// a list's plan has no pair range.
static SwgDiagWork q32_one_class(int variant, int K, int G, size_t npass, uint64_t n_pairs = 0)
{
    SwgDiagWork wk;
    wk.n_classes = 1;
    wk.plan[0].variant = variant;
    wk.plan[0].K = K;
    wk.plan[0].G = G;
    wk.plan[0].W = 4;
    wk.plan[0].npass = (int)npass;
    wk.pair_end[0] = n_pairs;
    return wk;
}

// Columns per lane for lane groups of G lanes whose profile `fits` LDS.  one_pass: the fewest that cover the query in
// one pass.  Otherwise the most that fit give the number of passes, and then the fewest that still need no more passes
// are taken (less padding in the last one).  Returns the variant (-1: none) with its K and the passes.
template <class Fits> static int cols_per_lane(int G, size_t lq, bool one_pass, Fits fits, int *K_out, size_t *npass)
{
    int best = -1, bestK = one_pass ? 1 << 30 : 0;
    for (int v = 0; v < swg_num_diag_variants(); ++v) {
        const int K = swg_diag_variant_info(v).K;
        if (fits(K, G) && (one_pass ? (size_t)G * K >= lq && K < bestK : K > bestK)) best = v, bestK = K;
    }
    if (best < 0) return -1;
    *npass = one_pass ? 1 : (lq + (size_t)G * bestK - 1) / ((size_t)G * bestK);
    for (int v = 0; v < swg_num_diag_variants() && !one_pass; ++v) {
        const int K = swg_diag_variant_info(v).K;
        if (K < bestK && (size_t)G * K * *npass >= lq) best = v, bestK = K;
    }
    *K_out = bestK;
    return best;
}

// Geometry for a list of `n_items` flagged sequences (or, with a plan the int16 planner's choice does not
// fit, the whole database): few items get 64 lanes each (the shortest chain per row), many the narrowest
// lane group that covers the query in one pass.  A query no single pass holds (LDS: G*K int32 columns of
// 128 bytes in 160 KB, about 1150) takes several passes of the widest geometry for the item count.
static bool q32_list_plan(const swg_ctx *ctx, size_t lq, uint32_t n_items, SwgDiagWork *wk)
{
    const bool few = n_items <= 8u * (uint32_t)ctx->n_cu;
    auto fits = [](int K, int G) { return swg_diag32q_lds_bytes(K, G, 4) <= SWG_LDS_PER_CU; };
    const int order[4] = {few ? 64 : 16, 32, few ? 16 : 64, few ? 64 : 32}; // (the last: several passes, few items 64 lanes, many 32)
    for (int gi = 0; gi < 4; ++gi) {
        int K = 0;
        size_t npass = 0;
        const int v = cols_per_lane(order[gi], lq, gi < 3, fits, &K, &npass);
        if (v < 0) continue;
        if (npass > 64) return false;
        *wk = q32_one_class(v, K, order[gi], npass);
        return true;
    }
    return false;
}

// Geometry of the exact int32 cells (gap scores of any sign) for a whole database: one class; the narrowest lane
// group that covers the query in one pass with at most SWG_X32_MAX_K columns per lane (forced cols_per_wave /
// group_lanes are honoured where they fit), else several passes of 64 lanes.
static bool x32_plan(const swg_ctx *ctx, const swg_db *db, size_t lq, SwgDiagWork *wk)
{
    auto set = [&](int v, int K, int G, size_t npass) { *wk = q32_one_class(v, K, G, npass, swg_db_pair_count(db)); };
    auto fits = [&](int K, int G) { return K <= SWG_X32_MAX_K && swg_diag32q_lds_bytes(K, G, 4) <= SWG_LDS_PER_CU; };
    if (ctx->opt_cols > 0 && ctx->opt_group > 0) {
        for (int v = 0; v < swg_num_diag_variants(); ++v) {
            const int K = swg_diag_variant_info(v).K, G = (int)ctx->opt_group;
            if (K != (int)ctx->opt_cols || !fits(K, G)) continue;
            const size_t np = (lq + (size_t)G * K - 1) / ((size_t)G * K);
            if (np > 64) continue;
            set(v, K, G, np);
            return true;
        }
    }
    const int groups[4] = {16, 32, 64, 64}; // (the last: several passes)
    for (int gi = 0; gi < 4; ++gi) {
        int K = 0;
        size_t npass = 0;
        const int v = cols_per_lane(groups[gi], lq, gi < 3, fits, &K, &npass);
        if (v < 0) continue;
        if (npass > 64) return false;
        set(v, K, groups[gi], npass);
        return true;
    }
    return false;
}

// Launches the int32 work-queue fill: every sequence of the plan's classes (list == NULL), or the
// device-side list of ranks with one class.  A plan of several passes (one class) is one launch per
// pass, the rows' edges going from launch to launch through memory.  Events as launch_diag.
static int launch_q32(swg_ctx *ctx, swg_db *db, const SwgDiagWork &wk, int go, int ge, const uint32_t *d_list,
                      const uint32_t *d_list_count, uint32_t list_items, uint32_t *queue_words, bool *two_ends,
                      bool timing_events = true, bool exact = false)
{
    hipStream_t s = ctx->stream;
    SwgPairTokens &T = db->ptok;
    const size_t n_slots = (size_t)db->n_bins * SWG_BIN;
    *two_ends = false;
    const int npass = wk.plan[0].npass;
    if (npass > 1) {
        if (wk.n_classes != 1 || T.total_blocks >= (1ull << 28))
            return swg_set_ctx_error(ctx, SWG_ERR_ARG, "int32 multi-pass fill: plan not supported");
        // per row and per sequence of the pair; the exact cells' third edge value beside it
        int rc = ensure_edge_pair(ctx, T, T.d_edge32, &T.edge32_blocks, 4 * 2 * sizeof(int2));
        if (rc == SWG_OK && exact) rc = ensure_edge_pair(ctx, T, T.d_edge32d, &T.edge32d_blocks, 4 * 2 * sizeof(int32_t));
        if (rc != SWG_OK) return rc;
    }
    for (int c = 0; c < wk.n_classes; ++c) {
        const SwgDiagPlan &pl = wk.plan[c];
        const int kp = swg_q32_padded_cols(pl.K);
        const uint32_t ncols = (uint32_t)(pl.npass * pl.G * kp);
        int rc = ensure_profile_cols(ctx, 4 + c, ncols, 4, (1ull << 54) | ((uint64_t)pl.K << 40) | ((uint64_t)pl.G << 32) | (uint64_t)ncols,
                                     pl.K, kp, 2, SWG_LDS_SWIZZLE ? pl.G : 0);
        if (rc != SWG_OK) return rc;
    }
    if (timing_events) HIP_TRY(ctx, hipEventRecord(ctx->cur->ev[1], s));
    int rf = fork_long_class(ctx, wk);
    if (rf != SWG_OK) return rf;
    for (int c = wk.n_classes - 1; c >= 0; --c) {
        const SwgDiagPlan &pl = wk.plan[c];
        SwgDiagQ32Params q = token_params<SwgDiagQ32Params>(T, pl.G, wk.n_classes, db->d_counters + SWG_RANK_WORD(c));
        uint64_t items;
        if (d_list) {
            q.list = d_list;
            q.list_count = d_list_count;
            items = list_items;
        } else {
            q.q_begin = (uint32_t)std::min<uint64_t>(2 * wk.pair_begin[c], n_slots);
            q.q_end = (uint32_t)std::min<uint64_t>(2 * wk.pair_end[c], n_slots);
            items = q.q_end - q.q_begin;
        }
        q.queue = queue_words + (size_t)c * SWG_DYN_SHARDS * SWG_DYN_SHARD_STRIDE;
        q.scores = db->d_scores;
        q.seq_limit = (uint32_t)n_slots;
        q.go = exact ? go : -go; // (the exact cells add the signed scores, the reduced ones subtract magnitudes)
        q.ge = exact ? ge : -ge;
        int W = 4;
        const int wgs = q32_class_workgroups(ctx, wk, c, items, &W);
        if (c == 0 && !d_list) {
            const uint64_t blocks = T.pair_blocks_prefix[wk.pair_end[0]] - T.pair_blocks_prefix[wk.pair_begin[0]];
            q.prio_blocks = bulk_prio_blocks(ctx, blocks, (uint64_t)wgs * W * (64 / pl.G), 2.0); // (the int32 kernel's rule has a factor 2)
        } else {
            q.prio_blocks = c == 1 ? 0u : 0xFFFFFFFFu;
        }
        const size_t slice = (size_t)pl.G * swg_q32_padded_cols(pl.K) * 128;
        hipStream_t qs = c == 1 ? ctx->stream2 : s;
        for (int pass = 0; pass < pl.npass; ++pass) {
            if (pass > 0) HIP_TRY(ctx, hipMemsetAsync(q.queue, 0, (size_t)SWG_DYN_SHARDS * SWG_DYN_SHARD_STRIDE * 4, qs));
            q.profile = ctx->d_profile[4 + c] + (size_t)pass * slice;
            q.edge_in = pass > 0 ? T.d_edge32[(pass - 1) & 1] : nullptr;
            q.edge_out = pass + 1 < pl.npass ? T.d_edge32[pass & 1] : nullptr;
            q.edge_d_in = exact && pass > 0 ? T.d_edge32d[(pass - 1) & 1] : nullptr;
            q.edge_d_out = exact && pass + 1 < pl.npass ? T.d_edge32d[pass & 1] : nullptr;
            HIP_TRY(ctx, swg_launch_diag32q(pl.variant, pl.npass > 1, exact, W, wgs, q, qs));
        }
    }
    rf = join_long_class(ctx, wk, true);
    if (rf != SWG_OK) return rf;
    *two_ends = wk.n_classes == 2;
    if (timing_events) HIP_TRY(ctx, hipEventRecord(ctx->cur->ev[2], s));
    return SWG_OK;
}

// ---------------------------------------------------------------------------
// the pairs the f16 cells flagged, again on int16 cells
// ---------------------------------------------------------------------------
// A pair whose f16 score reached 4096 is run again by the same work-queue kernel on the packed int16 cells (or
// the wide form when the query can score beyond 32767), which are exact where the f16 cells are not: 10
// instead of 8.5 instructions per column pair, against 16 for the int32 kernel, and -- unlike the int32
// kernel's 32-bit edge indices -- on databases of any size.  The launch reads the list's length on the device
// and leaves at once when it is empty.  Geometry: few pairs get 64 lanes each (the shortest chain per row),
// many the main fill's own.
static bool i16_list_plan(int n_cu, size_t lq, uint32_t n_pairs_guess, const SwgDiagPlan &main_plan, SwgDiagPlan *out)
{
    // 64 lanes per pair: one pair per wavefront, so a list shorter than the launch has lane groups still fills every
    // wavefront it occupies (with 16-lane groups a list of 3 100 pairs -- config 4's share with 0.5 % relatives --
    // lands one pair in every fourth group and every wavefront issues its rows for one group in four: 26 ms against
    // 15), and at 512 columns or more its rows cost the same instructions per pair as the main fill's narrower groups
    // in more passes (lq 3000: 2 x 269 per pair-row against 6 x 349 / 4).  Only a short query's long list -- where a
    // 64-lane group would hold two or three columns per lane -- keeps the main fill's geometry.
    if (n_pairs_guess > 4u * (uint32_t)n_cu && lq < 512) {
        *out = main_plan;
        out->f16 = 0;
        out->f16_from = 0;
        out->last_variant = -1;
        out->last_K = 0;
        return true;
    }
    const int G = 64;
    int bestK = 0;
    size_t npass = 0;
    const int best = cols_per_lane(G, lq, false, [](int K, int g) { return swg_diag_dyn_lds_bytes(K, g, 4) <= SWG_LDS_PER_CU; }, &bestK, &npass);
    if (best < 0) return false;
    *out = SwgDiagPlan();
    out->variant = best;
    out->K = bestK;
    out->G = G;
    // One workgroup per CU is all that fits beside a 64-lane profile of 512 columns or more (98 KB at K = 24), so the
    // workgroup is as large as the kernel was compiled for, and the kernel sends home the wavefronts a shorter list
    // does not need (it knows the list's length; the host does not).  Until round 4's last day the workgroup had 4
    // wavefronts -- ONE per SIMD, 5.2 cycles per instruction instead of 4.07 -- whatever the list, and config 4's
    // 3 100 pairs took three rounds and 28 left-overs on 1 024 wavefronts (7.7 ms per pass, now 5.3; the text of
    // DESIGN 9 counted 3 072).
    int W = swg_diag_variant_info(best).max_waves / 4 * 4;
    while (W > 4 && swg_diag_dyn_lds_bytes(bestK, G, W) > SWG_LDS_PER_CU) W -= 4;
    out->W = std::max(4, W);
    out->npass = (int)npass;
    return true;
}

// test hook (not in the public headers): the list re-run's geometry for a query of lq columns, on the host.
// main_kgw: the main fill's (K, G, W), which a short query's long list keeps; out: {K, G, W, passes}
extern "C" int swg_debug_list_plan(size_t lq, uint32_t n_pairs_guess, int n_cu, const int32_t *main_kgw, int32_t *out)
{
    if (!main_kgw || !out || n_cu < 1) return SWG_ERR_ARG;
    SwgDiagPlan mp = SwgDiagPlan(), lp = SwgDiagPlan();
    mp.K = main_kgw[0];
    mp.G = main_kgw[1];
    mp.W = main_kgw[2];
    mp.npass = 1;
    if (!i16_list_plan(n_cu, lq, n_pairs_guess, mp, &lp)) return SWG_ERR_ARG;
    out[0] = lp.K;
    out[1] = lp.G;
    out[2] = lp.W;
    out[3] = lp.npass;
    return SWG_OK;
}

static int launch_dyn_list(swg_ctx *ctx, swg_db *db, const SwgDiagPlan &pl, bool wide, int go, int ge, const uint32_t *d_list,
                           const uint32_t *d_count, hipStream_t s)
{
    SwgPairTokens &T = db->ptok;
    const int form = wide ? 1 : 0;
    const bool edges = pl.npass > 1 || form == 1;
    int rc = pl.npass > 1 ? ensure_edges(ctx, &T) : SWG_OK;
    if (rc != SWG_OK) return rc;
    const int kp = swg_diag_padded_cols(pl.K);
    const uint32_t ncols = (uint32_t)(pl.npass * pl.G * kp);
    rc = ensure_profile_cols(ctx, 6, ncols, 2, (1ull << 52) | ((uint64_t)pl.K << 40) | ((uint64_t)pl.G << 32) | (uint64_t)ncols, pl.K, kp,
                             4, SWG_LDS_SWIZZLE ? pl.G : 0, 0);
    if (rc != SWG_OK) return rc;
    SwgDiagDynParams q = dyn_params_base(T, db->d_scores, (size_t)db->n_bins * SWG_BIN, pl.G, form, go, ge, 1, db->d_counters + SWG_RANK_WORD(0));
    q.list = d_list;
    q.list_count = d_count;
    q.queue = db->d_counters + SWG_QUEUE_WORD(0);
    q.prio_blocks = 0xFFFFFFFFu;
    q.prio_blocks2 = 0xFFFFFFFFu;
    const int per_cu = swg_workgroups_per_cu(swg_diag_variant_info(pl.variant).max_waves, pl.W, swg_diag_dyn_lds_bytes(pl.K, pl.G, pl.W));
    const int wgs = ctx->n_cu * std::min(per_cu, 3);
    const uint32_t n_pairs = (uint32_t)swg_db_pair_count(db);
    std::vector<std::pair<uint32_t, uint32_t>> segs; // (the list spans the whole token buffer)
    bool cut = false;
    if (!token_segments(T, 0u, n_pairs, ctx->opt_seg_blocks, edges, &segs, &cut))
        return swg_set_ctx_error(ctx, SWG_ERR_ARG, "a pair of sequences too long for the multi-pass fill");
    q.seg_origin = 0;
    q.seg_blocks = (uint32_t)std::min<uint64_t>(T.total_blocks, ctx->opt_seg_blocks);
    const size_t slice = (size_t)pl.G * kp * 64;
    bool first_launch = true;
    for (int pass = 0; pass < pl.npass; ++pass) {
        q.profile = ctx->d_profile[6] + (size_t)pass * slice;
        q.edge_in = pass > 0 ? T.d_edge[(pass - 1) & 1] : nullptr;
        q.edge_out = pass + 1 < pl.npass ? T.d_edge[pass & 1] : nullptr;
        for (const std::pair<uint32_t, uint32_t> &sg : segs) {
            if (!first_launch) HIP_TRY(ctx, hipMemsetAsync(q.queue, 0, (size_t)SWG_DYN_SHARDS * SWG_DYN_SHARD_STRIDE * 4, s));
            first_launch = false;
            q.q_begin = sg.first;
            q.q_end = sg.second;
            if (cut) {
                q.seg_origin = T.pair_blocks_prefix[sg.first];
                q.seg_blocks = T.pair_blocks_prefix[sg.second] - q.seg_origin;
            }
            HIP_TRY(ctx, swg_launch_diag_dyn(pl.variant, edges, form, pl.W, wgs, q, s));
        }
    }
    return SWG_OK;
}

// First search of a query length on a database: the cost model ranks the geometries, the few
// best are timed once on this device (each is a complete, valid fill) and the fastest is kept.
static int autotune_diag(swg_ctx *ctx, swg_db *db, size_t lq, int go, int ge, SwgTuned *tuned, int form)
{
    SwgDiagWork *best = &tuned->wk;
    std::vector<SwgDiagWork> cands;
    const bool work_queue = ctx->opt_dynamic != 0 && db->ptok.ok;
    if (swg_plan_diag_candidates(db, lq, ctx->n_cu, 0, 0, 0, 0, true, work_queue, &cands, 1.0, form, form == 3 ? 1 : ctx->opt_f16_pair) <= 0) return SWG_ERR_ARG;
    for (SwgDiagWork &c : cands) // (the trials run on the cells the search will use)
        for (int k = 0; k < c.n_classes; ++k) c.plan[k].f16 = form >= 2, c.plan[k].gapless = form == 3;
    // distinct (K, G, W, split) among the best-ranked
    std::vector<SwgDiagWork> pick;
    for (const SwgDiagWork &c : cands) {
        bool dup = false;
        for (const SwgDiagWork &p : pick)
            dup |= p.plan[0].K == c.plan[0].K && p.plan[0].G == c.plan[0].G && p.plan[0].W == c.plan[0].W &&
                   p.n_classes == c.n_classes &&
                   (c.n_classes < 2 || (p.plan[1].K == c.plan[1].K && p.plan[1].G == c.plan[1].G &&
                                        p.pair_end[1] == c.pair_end[1]));
        if (!dup) pick.push_back(c);
        // long fills: fewer trials (a trial is a warm-up and a few complete fills)
        if (pick.size() >= (cands[0].plan[0].est_ms > 50.0 ? 4u : 8u)) break;
    }
    const size_t n_slots = (size_t)db->n_bins * SWG_BIN;
    double best_ms = 1e300;
    // One trial = a warm-up fill, then four fills queued back to back the way consecutive searches
    // are, timed as a whole: what happens where one fill ends and the next begins (workgroups of
    // two classes competing for the freed slots) is part of what is being chosen.
    auto time_one = [&](const SwgDiagWork &c, double *ms_out) -> int {
        int rc = prepare_diag(ctx, db, c);
        if (rc != SWG_OK) return rc;
        // (enough repetitions for about 20 ms of fills: four 2 ms fills differ by more from trial to trial than the
        // geometries being compared do -- round 3: the tuner picked K=24 over the model's K=23 on config 2 and lost 3 %)
        const int reps = c.plan[0].est_ms > 20.0 ? 2 : std::max(4, std::min(16, (int)(20.0 / std::max(0.5, c.plan[0].est_ms))));
        for (int rep = -1; rep < reps; ++rep) {
            bool two = false;
            if (rep == 0) HIP_TRY(ctx, hipEventRecord(ctx->cur->ev[0], ctx->stream));
            HIP_TRY(ctx, hipMemsetAsync(db->d_scores, 0, n_slots * 4, ctx->stream));
            HIP_TRY(ctx, hipMemsetAsync(db->d_counters, 0, SWG_COUNTER_BYTES, ctx->stream));
            rc = launch_diag(ctx, db, c, go, ge, &two);
            if (rc != SWG_OK) return rc;
        }
        HIP_TRY(ctx, hipEventRecord(ctx->cur->ev[4], ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        float ms = 0.f;
        HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->cur->ev[0], ctx->cur->ev[4]));
        *ms_out = (double)ms / reps;
        return SWG_OK;
    };
    if (!pick.empty()) {
        // (one untimed trial first: the first candidate -- the model's choice -- otherwise pays for the clocks ramping
        // up and the code objects' first touch, and loses to candidates that are in fact slower)
        double warm = 0;
        int rc = time_one(pick[0], &warm);
        if (rc != SWG_OK) return rc;
    }
    for (const SwgDiagWork &c : pick) {
        double ms = 0;
        int rc = time_one(c, &ms);
        if (rc != SWG_OK) return rc;
        // the model's first choice stays unless another geometry is clearly (2 %) faster: two
        // timings of the same fill differ by about a percent
        if (ms < best_ms * (best_ms < 1e299 ? 0.98 : 1.0)) {
            best_ms = ms;
            *best = c;
            best->plan[0].est_ms = ms;
        }
    }
    // second stage: with the winning geometry, where to cut the long class off.  Fixed streams only:
    // with the work queue the model's cut (the longest pair a fair-share wavefront still finishes
    // within the search) is within a percent of the best measured one, less than two trials differ.
    if (best->n_classes == 2 && !diag_class_is_dynamic(ctx, db, best->plan[0])) {
        const SwgDiagWork base = *best;
        const uint64_t n_pairs = swg_db_pair_count(db);
        const bool dyn = diag_class_is_dynamic(ctx, db, base.plan[0]);
        // static streams: multiples of a stream's mean share; work queue: around the model's cut
        const double unit = dyn ? (double)(2ull + db->lens[2 * base.pair_end[1]])
                                : (double)swg_db_pair_rows(db, 0, n_pairs, nullptr) / (double)base.plan[0].n_streams;
        const double fr_static[] = {0.25, 0.45, 0.8, 1.0, 1.3, 1.7};
        const double fr_dyn[] = {0.6, 0.75, 0.88, 1.15, 1.35, 1.7};
        for (int i = 0; i < 6; ++i) {
            const long thr = (long)std::max(64.0, (dyn ? fr_dyn[i] : fr_static[i]) * unit);
            std::vector<SwgDiagWork> alt;
            if (swg_plan_diag_candidates(db, lq, ctx->n_cu, base.plan[0].K, base.plan[0].G, base.plan[0].W, thr, true,
                                         work_queue, &alt, 1.0, form, ctx->opt_f16_pair) <= 0)
                continue;
            for (SwgDiagWork &c : alt)
                for (int k = 0; k < c.n_classes; ++k) c.plan[k].f16 = form >= 2, c.plan[k].gapless = form == 3;
            const SwgDiagWork *same = nullptr;
            for (const SwgDiagWork &c : alt)
                if (c.n_classes == 2 && c.plan[1].K == base.plan[1].K && c.plan[1].G == base.plan[1].G) {
                    same = &c;
                    break;
                }
            if (!same || same->pair_end[1] == base.pair_end[1]) continue;
            double ms = 0;
            int rc = time_one(*same, &ms);
            if (rc != SWG_OK) return rc;
            if (ms < best_ms * 0.985) {
                best_ms = ms;
                *best = *same;
                best->plan[0].est_ms = ms;
            }
        }
    }
    tuned->engine = 2;
    tuned->ms = best_ms;
    // third stage: the systolic engine (less bookkeeping per row, coarse work units); it has not won
    // a measured case since the diagonal engine got its work queue and is only tried where a trial
    // is cheap
    for (int v = 0; v < swg_num_variants(16) && tuned->ms < 100.0 && form != 3; ++v) { // (the gapless cells exist on lane groups only)
        SwgSystolicPlan pl;
        int rc = make_plan(ctx, 16, db->n_bins, swg_variant_info(16, v).K, &pl);
        if (rc != SWG_OK) continue;
        if ((rc = prepare_systolic(ctx, db, pl)) != SWG_OK) return rc;
        double ms_min = 1e300;
        for (int rep = 0; rep < 2; ++rep) {
            HIP_TRY(ctx, hipMemsetAsync(db->d_scores, 0, n_slots * 4, ctx->stream));
            HIP_TRY(ctx, hipMemsetAsync(db->d_counters, 0, SWG_COUNTER_BYTES, ctx->stream));
            if ((rc = launch_systolic(ctx, db, pl, go, ge)) != SWG_OK) return rc;
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            double ms = 0;
            if ((rc = diag_fill_ms(ctx, false, &ms)) != SWG_OK) return rc;
            ms_min = std::min(ms_min, ms);
        }
        if (ms_min < tuned->ms) {
            tuned->ms = ms_min;
            tuned->engine = 1;
            tuned->systolic_K = pl.K;
        }
    }
    return SWG_OK;
}

// ---------------------------------------------------------------------------
// the hot path
// ---------------------------------------------------------------------------
extern "C" uint64_t swg_hit_key(int32_t score, uint32_t index)
{
    return ((uint64_t)(uint32_t)(score < 0 ? 0 : score) << 32) | (uint64_t)(0xFFFFFFFFu - index);
}
extern "C" void swg_key_hit(uint64_t key, swg_hit *out)
{
    if (!out) return;
    out->score = (int32_t)(key >> 32);
    out->index = 0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFu);
}
extern "C" size_t swg_topk_merge_keys(const uint64_t *keys, size_t n, size_t k, swg_hit *out)
{
    if (!keys || !out || k == 0) return 0;
    std::vector<uint64_t> v;
    v.reserve(n);
    for (size_t i = 0; i < n; ++i)
        if (keys[i] != 0) v.push_back(keys[i]);
    const size_t m = std::min(k, v.size());
    std::partial_sort(v.begin(), v.begin() + m, v.end(), std::greater<uint64_t>());
    for (size_t i = 0; i < m; ++i) swg_key_hit(v[i], &out[i]);
    return m;
}

// Pinned landing buffer of a slot's score read-out (a pageable destination would make the "async"
// copy block the host behind everything queued before it).
static int slot_scores(swg_ctx *ctx, SwgSlot *S, size_t n)
{
    if (n <= S->h_scores_cap) return SWG_OK;
    (void)hipHostFree(S->h_scores);
    S->h_scores = nullptr;
    S->h_scores_cap = 0;
    HIP_TRY(ctx, hipHostMalloc(reinterpret_cast<void **>(&S->h_scores), std::max<size_t>(n, 64) * sizeof(int32_t), hipHostMallocDefault));
    S->h_scores_cap = std::max<size_t>(n, 64);
    return SWG_OK;
}

// ---------------------------------------------------------------------------
// one search: what it decides (plan_search), then what it queues (the other stages of search_begin)
// ---------------------------------------------------------------------------
// The cost model's word on the ENGINE (round 4; until then only the autotuner could pick the systolic one, and it
// is off for databases beyond 4 M sequences and wherever the caller turned it off): a database of short sequences
// of near-equal length -- peptides -- is what the systolic engine is good at (no reset rows, no flags, nothing per
// pair: 2 M peptides of 20-40 residues, lq 128: 6 570 GCUPS against the lane groups' 4 840, lq 30: 4 820 against
// 1 930), and the two estimates tell: the lane groups' from the planner (plan0, on the cells `form`), the systolic one
// from the bin table, for n_queries queries one after another (no batch form of that engine exists).  It has to win by
// 15 % (both models are good to about 10 %).  bound: the largest score of the search(es), which decides the systolic
// engine's cells; *sys_K: the columns per wavefront of its best instantiation.
static bool systolic_beats_lane_groups(const swg_ctx *ctx, const swg_db *db, size_t lq, const SwgDiagPlan &plan0, int form,
                                       uint64_t bound, size_t n_queries, int *sys_K)
{
    *sys_K = 0;
    if (ctx->opt_engine != 0 || ctx->opt_f16 == 2 || db->tokens_only || !(plan0.est_ms > 0.0)) return false;
    const bool sys_f16 = ctx->opt_f16 != 0 && swg_f16_gaps_ok(ctx->gap_open + ctx->gap_extend, ctx->gap_extend) && bound < SWG_F16_CEILING;
    const double sys_ms = swg_systolic_estimate_ms(db, lq, ctx->n_cu, sys_K, sys_f16) * (double)n_queries;
    return *sys_K > 0 && sys_ms < SWG_SYSTOLIC_MARGIN * plan0.est_ms * swg_diag_short_pair_factor(db, plan0, form);
}

// One class of exactly (K = cols, G = group) over the whole database for the int32 work-queue kernel, a launch per pass,
// if its int32 profile fits LDS (a forced geometry that needs several passes, or whose long class did not fit).
static bool q32_forced_plan(const swg_db *db, size_t lq, long cols, long group, SwgDiagWork *wk)
{
    for (int v = 0; v < swg_num_diag_variants(); ++v) {
        const int K = swg_diag_variant_info(v).K, G = (int)group;
        if (K != (int)cols || swg_diag32q_lds_bytes(K, G, 4) > SWG_LDS_PER_CU) continue;
        const size_t np = (lq + (size_t)G * K - 1) / ((size_t)G * K);
        if (np > 64 || (np > 1 && db->ptok.total_blocks >= (1ull << 28))) continue;
        *wk = q32_one_class(v, K, G, np, swg_db_pair_count(db));
        return true;
    }
    return false;
}

// Three of plan_search's rules, spelled once for the search and for the test hooks behind it (swg_debug_plan_streams,
// swg_debug_plan_systolic).  The wide form first: int16 arithmetic, a score that can pass 32767, lane groups.
static bool wide_form_first(int bits, uint64_t score_bound, long engine, bool wide_ok)
{
    return bits == 16 && score_bound >= SWG_I16_CEILING && engine != 1 && wide_ok;
}
// The systolic engine on packed-f16 cells: one pass, gap magnitudes f16 holds, and no score that can reach their ceiling.
static bool systolic_takes_f16(int bits, bool use_diag, int npass, bool f16_gaps, uint64_t score_bound)
{
    return bits == 16 && !use_diag && npass == 1 && f16_gaps && score_bound < SWG_F16_CEILING;
}
// Option workgroups on lane groups: at most that many, and the streams that go with them.
static void cap_workgroups(SwgDiagPlan *d0, long workgroups)
{
    const uint64_t per_wg = (uint64_t)d0->W * (64 / d0->G);
    d0->workgroups = (int)std::min<long>(workgroups, d0->workgroups);
    d0->n_streams = (uint32_t)((uint64_t)d0->workgroups * per_wg);
}

// Every decision of one search: arithmetic, cell forms and their hand-overs, engines and geometries.  It allocates no
// profile, scratch or bin image and puts no launch on the search's own timeline; the only device work it may do is what
// the decisions themselves read: the pair tokens of the database (ensure_pair_tokens, built once per database) and the
// timed trials of the first search of a query length (autotune_diag, which end in a stream synchronisation).  *plan is
// the slot's own plan: launch_diag reads its score_bound inside the tuner's trials, so the bound is written first.
static int plan_search(swg_ctx *ctx, swg_db *db, bool allow_autotune, SwgSearchPlan *plan)
{
    *plan = SwgSearchPlan();
    SwgSearchPlan &P = *plan;
    SwgDiagWork &wk = P.wk, &wk32 = P.wk32;
    const size_t lq = ctx->query_len();
    const uint32_t n_bins = db->n_bins;
    const size_t n_slots = (size_t)n_bins * SWG_BIN;
    P.epoch = ctx->epoch;

    // How high can a score get (swg_score_bound)?  Below the int16 ceiling nothing can saturate; below the wide form's
    // (values biased by -32768, same instruction count) that form is exact and nothing needs the int32 re-score.
    const uint64_t longest = (uint64_t)db->max_nblk * SWG_ROWS_PER_BLK;
    const SwgScoreBound sb = ctx->query_pssm ? swg_score_bound(ctx->pssm.data(), nullptr, lq, longest)
                                             : swg_score_bound(&ctx->sub[0][0], ctx->query.data(), lq, longest);
    const uint64_t score_bound = P.score_bound = sb.bound, qbound = P.qbound = sb.qbound;
    // A gapless search (swg_search_gapless) never reads the context's gap scores: every level that has gap operands runs
    // with the gaps priced out.  A path with a gap can beat the best ungapped segment only if the segments on both sides
    // of the gap each score more than the gap costs.  The packed int16 cells stick at 32767, so with a magnitude of 32767
    // -- their saturating ceiling -- no such segment exists below the flag level: they are exact whatever the query.
    // The wide form and the int32 cells hold larger values: 32767 serves them while no score can pass 2 x 32767 (the
    // two segments use different query columns and different rows, so their sum is within score_bound); beyond that the
    // wide form is not used and the int32 levels take a magnitude above the score bound itself.
    const bool gapless = ctx->gapless;
    const bool gl_small = score_bound <= 2ull * SWG_I16_CEILING;
    const int gl_gap32 = gl_small ? -SWG_I16_CEILING : -(int)std::min<uint64_t>(score_bound + 1, 1u << 30);
    // which arithmetic: the packed int16 form needs non-positive gap scores
    const bool gl_bits32 = gapless && ctx->opt_force_bits == 32;
    const int go = P.go = gapless ? (gl_bits32 ? gl_gap32 : -SWG_I16_CEILING) : ctx->gap_open + ctx->gap_extend;
    const int ge = P.ge = gapless ? go : ctx->gap_extend;
    P.go32 = gapless ? gl_gap32 : go;
    P.ge32 = gapless ? gl_gap32 : ge;
    const bool fast_ok = P.fast_ok = gapless || (ctx->gap_open <= 0 && ctx->gap_extend <= 0 && -go <= SWG_I16_CEILING);
    const int bits = P.bits = fast_ok && ctx->opt_force_bits != 32 ? 16 : 32;
    if (ctx->opt_force_bits == 16 && !fast_ok)
        return swg_set_ctx_error(ctx, SWG_ERR_ARG,
                                 "force_bits=16 needs gap_open <= 0 and gap_extend <= 0");

    const bool f16_gaps = ctx->opt_f16 != 0 && swg_f16_gaps_ok(go, ge); // the f16 cells are allowed and hold the gap magnitudes
    const bool wide_ok = ctx->opt_wide != 0 && (!gapless || gl_small);
    P.wide = wide_form_first(bits, score_bound, ctx->opt_engine, wide_ok);
    // Gapless, route 1: the gapless cells (CellsGapless, form 3) where the query fits one pass of a geometry the table
    // offers (a forced cols_per_wave / group_lanes included), on the work queue, unless the options rule the f16 cells or
    // the lane groups out or the database came from 16-lane batches.  Everything else is route 0: the machinery below
    // as it stands, with the gap magnitudes above.
    bool gl_route1 = gapless && bits == 16 && ctx->opt_engine != 1 && ctx->opt_dynamic != 0 && ctx->opt_f16 != 0 && !db->tokens_only &&
                     lq <= 64u * 32u;
    if (gl_route1) {
        int rc1 = ensure_pair_tokens(ctx, db);
        if (rc1 != SWG_OK) return rc1;
        SwgDiagWork probe1;
        gl_route1 = db->ptok.ok && swg_plan_diag_work(db, lq, ctx->n_cu, ctx->opt_cols, ctx->opt_group, ctx->opt_max_waves, ctx->opt_long_split,
                                                      ctx->opt_workgroups == 0, true, &probe1, 1.0, 3, 1) > 0;
    }
    // The packed-f16 cells (three-operand maxima, 8.5 instead of 10 instructions per column pair) are exact
    // while scores stay below 4096; a sequence that reaches it is flagged and re-scored in int32.  They are the
    // first step whenever the gap magnitudes are f16 integers and the query is not so long that scores are
    // expected far beyond (where the wide form is exact on its own) -- unless this database has shown, for this
    // query, that a good part of its rows gets flagged ("f16" option: 0 never, 2 regardless of both).
    const bool want_f16 = gl_route1 || (bits == 16 && ctx->opt_engine != 1 && ctx->opt_dynamic != 0 && f16_gaps &&
                                        (ctx->opt_f16 == 2 || (score_bound < SWG_I16_CEILING && db->f16_veto_epoch != ctx->epoch)));
    if (want_f16) P.wide = false; // (only with f16 = 2: the f16 cells first, whatever the score bound)
    const int plan_form = gl_route1 ? 3 : want_f16 ? 2 : 0;

    // (the systolic plan: only the systolic engine needs it to exist -- a cols_per_wave meant for the
    // diagonal engine has no systolic instantiation, and with engine != 1 both widths run on lane groups)
    int rc = make_plan(ctx, bits, bits == 16 ? n_bins : n_bins * 2, ctx->opt_cols, &P.main_pl);
    if (rc != SWG_OK && ctx->opt_engine == 1) return rc;
    // int16: the diagonal engine unless the systolic one is asked for
    bool tuned_systolic = false;
    if (bits == 16 && ctx->opt_engine != 1) {
        // pair tokens, first condition: the lane groups' planner and the tuner's trials want the work queue
        if (ctx->opt_dynamic && (rc = ensure_pair_tokens(ctx, db)) != SWG_OK) return rc;
        const bool free_geometry = ctx->opt_cols == 0 && ctx->opt_group == 0 && ctx->opt_max_waves == 0 &&
                                   ctx->opt_long_split == 0 && ctx->opt_workgroups == 0;
        // (a geometry is tuned for the cells it ran on, and the pairings it was allowed)
        // (and a gapless search keeps its picks apart from the gapped searches')
        const uint64_t tuned_key = (uint64_t)lq | ((uint64_t)plan_form << 40) | ((uint64_t)ctx->opt_f16_pair << 44) | ((uint64_t)gapless << 48);
        auto it = free_geometry ? db->tuned.find(tuned_key) : db->tuned.end();
        if (it == db->tuned.end() && free_geometry && allow_autotune && ctx->opt_engine == 0 &&
            db->n_local >= 4096 && db->n_local <= (4u << 20)) {
            SwgTuned tn;
            if (autotune_diag(ctx, db, lq, go, ge, &tn, plan_form) == SWG_OK && tn.wk.n_classes > 0)
                it = db->tuned.insert(std::make_pair(tuned_key, tn)).first;
        }
        if (it != db->tuned.end() && !(P.wide && it->second.engine == 1)) {
            if (it->second.engine == 1 && ctx->opt_engine == 0) {
                // the systolic engine measured faster for this database and query length
                if ((rc = make_plan(ctx, 16, n_bins, it->second.systolic_K, &P.main_pl)) != SWG_OK) return rc;
                tuned_systolic = true;
            } else {
                wk = it->second.wk;
                P.use_diag = true;
            }
        }
        if (!P.use_diag && !tuned_systolic)
            P.use_diag = swg_plan_diag_work(db, lq, ctx->n_cu, ctx->opt_cols, ctx->opt_group, ctx->opt_max_waves,
                                            ctx->opt_long_split, ctx->opt_workgroups == 0,
                                            ctx->opt_dynamic != 0 && db->ptok.ok, &wk, 1.0, plan_form, gl_route1 ? 1 : ctx->opt_f16_pair) > 0;
        // the cost model's own comparison of the engines, where nothing was measured and nothing forced
        int sys_K = 0;
        if (P.use_diag && !tuned_systolic && free_geometry && !P.wide && it == db->tuned.end() && !gl_route1 &&
            systolic_beats_lane_groups(ctx, db, lq, wk.plan[0], plan_form, score_bound, 1, &sys_K)) {
            if (make_plan(ctx, 16, n_bins, sys_K, &P.main_pl) == SWG_OK) { // (a failed make_plan leaves the plan as it was)
                P.use_diag = false;
                tuned_systolic = true;
            }
        }
        if (!P.use_diag && !tuned_systolic && ctx->opt_engine == 2)
            return swg_set_ctx_error(ctx, SWG_ERR_ARG, "no diagonal-engine geometry for these options");
        if (P.use_diag && ctx->opt_workgroups > 0) cap_workgroups(&wk.plan[0], ctx->opt_workgroups);
        if (!P.use_diag && !tuned_systolic && rc != SWG_OK) return rc;
        // the wide form exists in the diagonal engine only
        if (P.wide && P.use_diag)
            for (int c = 0; c < wk.n_classes; ++c) wk.plan[c].wide = 1;
        else
            P.wide = false;
    }
    // The systolic engine on packed-f16 cells (round 4: 8.5 instead of 10 instructions per column pair) where NO score of
    // this search can reach their ceiling -- the engine has no flag-and-re-run route, and the databases the cost model
    // gives it are the ones whose longest sequence is short (372 residues x BLOSUM62's 11 < 4096).
    if (systolic_takes_f16(bits, P.use_diag, P.main_pl.npass, f16_gaps, score_bound)) P.main_pl.f16 = 1;
    // int32 work (forced / unusual gap scores / re-score of saturated sequences) also runs on
    // the diagonal engine unless the systolic one is asked for
    P.use_diag32 = ctx->opt_engine != 1;
    // Non-positive gap scores: the int32 work-queue kernel (8 instructions per cell, any lane-group
    // geometry, sequences off the queue) instead of the bin-based one (12 per cell, 64 lanes x 16 columns
    // whatever the query length).  Probed twice: before the token build for the query alone (one pass up to about
    // 1150 columns, else several: a query no geometry holds never builds tokens for this), and after it for what the
    // tokens add (they exist, and several passes fit the kernel's 32-bit edge indices).
    SwgDiagWork probe;
    P.q32_ok = fast_ok && P.use_diag32 && ctx->opt_dynamic != 0 && q32_list_plan(ctx, lq, 1, &probe);
    // the f16 cells: every class on the work queue, and a re-score path for what they flag
    P.use_f16 = want_f16 && P.use_diag;
    for (int c = 0; P.use_f16 && c < wk.n_classes; ++c) P.use_f16 = diag_class_is_dynamic(ctx, db, wk.plan[c]);
    if (P.q32_ok && (bits == 32 || score_bound >= (uint64_t)(P.wide ? SWG_WIDE_CEILING : SWG_I16_CEILING))) {
        // pair tokens, second condition: an int32 level on the work queue may follow (work_queue = 1 with the
        // systolic 16-bit fill, or a forced 32-bit search, has not built them above)
        if ((rc = ensure_pair_tokens(ctx, db)) != SWG_OK) return rc;
        P.q32_ok = db->ptok.ok && q32_list_plan(ctx, lq, 1, &probe) &&
                   (probe.plan[0].npass == 1 || db->ptok.total_blocks < (1ull << 28)); // (32-bit edge indices)
    }
    // A query long enough to score beyond 32767 gets the wide form (wide16 = 0: plain int16 cells and the int32
    // re-score from 32767) -- but only a sequence that is long itself can get
    // anywhere near: an exact copy of a stretch of the query scores qbound / lq per row on average, so one of fewer
    // than 4096 * lq / qbound rows stays below the f16 cells' ceiling even then.  Those (most of a protein database:
    // 730 rows with BLOSUM62) take the f16 cells, 8.5 instructions per column pair instead of 10, in launches of
    // their own after the long ones' (launch_diag).  The threshold is an expectation, not a bound: whatever the f16
    // cells flag all the same is run again on the wide form like any other flagged pair, so results do not depend on it.
    if (!gapless && !P.use_f16 && bits == 16 && score_bound >= SWG_I16_CEILING && P.use_diag && ctx->opt_f16 == 1 && db->f16_veto_epoch != ctx->epoch &&
        swg_f16_gaps_ok(go, ge) && wk.n_classes == 1 && diag_class_is_dynamic(ctx, db, wk.plan[0]) && !db->tokens_only && qbound > 0) {
        const uint32_t rows = swg_split_rows(lq, qbound);
        swg_db_split_at(db, rows); // (per database and length: a binary search and one pass over the lengths)
        const uint32_t cut = std::max<uint32_t>(db->split_pair, (uint32_t)wk.pair_begin[0]);
        if (cut <= wk.pair_begin[0] && (score_bound < SWG_WIDE_CEILING || P.q32_ok)) {
            // nothing long in this database: the f16 cells for all of it (what they flag: the wide form, as below)
            P.use_f16 = true;
            P.wide = false;
            wk.plan[0].wide = 0;
        } else if (cut > wk.pair_begin[0] && cut < wk.pair_end[0]) {
            P.split_at = cut;
            P.split_rows = rows;
            P.split_residues = db->split_residues;
        }
    }
    wk.plan[0].f16_from = P.split_at; // (0 without a split, and never read without the diagonal engine)
    // Several passes of G*K columns each leave the last one partly empty (3000 columns in 6 passes of 512: 72 of them,
    // 2.3 % of the work): it runs the instantiation with the fewest columns per lane that cover what is left.
    for (int c = 0; c < wk.n_classes; ++c) {
        SwgDiagPlan &pl = wk.plan[c];
        pl.last_variant = -1;
        pl.last_K = 0;
        if (!P.use_diag || wk.n_classes != 1 || pl.npass < 2 || !diag_class_is_dynamic(ctx, db, pl) || ctx->opt_last_pass == 0) continue;
        if (!swg_plan_last_pass(pl, lq, &pl.last_variant, &pl.last_K)) pl.last_variant = -1, pl.last_K = 0;
    }
    // what the f16 cells flag is run again on int16 cells (the wide form if scores may pass 32767); only what
    // saturates those too needs the int32 kernel
    P.rerun_wide = (P.use_f16 && score_bound >= SWG_I16_CEILING && wide_ok) || (P.split_at != 0u && P.wide);
    const int32_t rerun_ceiling = P.rerun_wide ? SWG_WIDE_CEILING : SWG_I16_CEILING;
    if (P.use_f16 && score_bound >= (uint64_t)rerun_ceiling && !P.q32_ok) P.use_f16 = false;
    for (int c = 0; c < wk.n_classes; ++c) wk.plan[c].f16 = P.use_f16 ? 1 : 0;
    P.gapless = gapless;
    P.gapless_cells = gl_route1 && P.use_f16; // (route 1 stands: the gapless cells fill, their flags take the list re-run)
    for (int c = 0; c < wk.n_classes; ++c) wk.plan[c].gapless = P.gapless_cells ? 1 : 0;
    P.ceiling = P.use_f16 ? SWG_F16_CEILING : P.wide ? SWG_WIDE_CEILING : SWG_I16_CEILING;
    P.may_saturate = bits == 16 && (score_bound >= (uint64_t)P.ceiling || P.split_at != 0u);
    // (the int32 level follows the last 16-bit one: the fill's own cells, or the re-run's when f16 cells came first)
    P.level_ceiling = P.some_f16() ? rerun_ceiling : P.ceiling;
    P.int32_level = bits == 16 && score_bound >= (uint64_t)P.level_ceiling;
    // (the systolic int32 re-score uses its default geometry, whatever cols_per_wave asks of the fill)
    if (P.may_saturate && (rc = make_plan(ctx, 32, (uint32_t)std::min<size_t>(n_slots / 64, 1u << 30), 0, &P.re_pl)) != SWG_OK) return rc;
    P.npass32 = (int)((lq + 64 * SWG_DIAG32_K - 1) / (64 * SWG_DIAG32_K));
    if (bits == 32 && !fast_ok && P.use_diag32 && ctx->opt_dynamic != 0) {
        // gap scores the reduced algebra cannot express (a positive one): the same work-queue kernel on the
        // exact cells, unless the token array is beyond its 32-bit edge indices.  Pair tokens, third condition: q32_ok
        // is false here (it needs fast_ok), so neither of the two above has built them.
        if ((rc = ensure_pair_tokens(ctx, db)) != SWG_OK) return rc;
        if (db->ptok.ok) {
            // the planner's split into a bulk and a long class where it fits the int32 profile and the exact cells'
            // register budget (config 2's shape: 2 580 GCUPS as one class, the longest pairs' chains last), else one class
            bool two = swg_plan_diag_work(db, lq, ctx->n_cu, ctx->opt_cols, ctx->opt_group, ctx->opt_max_waves, ctx->opt_long_split,
                                          ctx->opt_workgroups == 0, true, &wk32) > 0 && q32_plan_fits(wk32, lq);
            for (int c = 0; two && c < wk32.n_classes; ++c) two = wk32.plan[c].K <= SWG_X32_MAX_K;
            if (two || (x32_plan(ctx, db, lq, &wk32) && (wk32.plan[0].npass == 1 || db->ptok.total_blocks < (1ull << 28))))
                P.use_q32 = P.exact32 = true;
        }
    }
    if (bits == 32 && P.q32_ok) {
        P.use_q32 = swg_plan_diag_work(db, lq, ctx->n_cu, ctx->opt_cols, ctx->opt_group, ctx->opt_max_waves, ctx->opt_long_split,
                                       ctx->opt_workgroups == 0, true, &wk32) > 0 && q32_plan_fits(wk32, lq);
        // a forced geometry as it is where it can run; otherwise the library's own pick below, which swg_stats reports
        if (!P.use_q32 && ctx->opt_cols > 0 && ctx->opt_group > 0) P.use_q32 = q32_forced_plan(db, lq, ctx->opt_cols, ctx->opt_group, &wk32);
        if (!P.use_q32) {
            // the int16 planner's choice does not fit (LDS holds half as many int32 columns): fewest lanes that do
            P.use_q32 = q32_list_plan(ctx, lq, (uint32_t)std::min<size_t>(n_slots, 1u << 30), &wk32);
            if (P.use_q32) wk32.pair_end[0] = swg_db_pair_count(db);
        }
    }
    P.bin32 = P.use_diag32 && ((bits == 32 && !P.use_q32) || (P.int32_level && !P.q32_ok)); // the bin-based int32 kernel is needed
    return SWG_OK;
}

// Test hooks (swg_host_internal.h): what plan_search decides for the two engines the work queue does not serve, without a
// device, from the rules above and the planners the search itself calls.
// swg_debug_plan_streams: the fixed-stream fill of options engine = 2, work_queue = 0, f16 = 0, long_split = -1 with
// cols_per_wave, group_lanes, max_waves and workgroups (0 = free) for a query idx[0 .. lq) under the table `rows`.
extern "C" int swg_debug_plan_streams(const swg_db *db, const int8_t *rows, const int8_t *idx, size_t lq, int n_cu, long cols, long group,
                                      long waves, long workgroups, int32_t *out)
{
    if (!db || !rows || !idx || !out || lq == 0 || n_cu <= 0 || cols < 0 || group < 0 || waves < 0 || workgroups < 0) return SWG_ERR_ARG;
    memset(out, 0, 8 * sizeof(int32_t));
    try {
        const SwgScoreBound sb = swg_score_bound(rows, idx, lq, (uint64_t)db->max_nblk * SWG_ROWS_PER_BLK);
        SwgDiagWork wk;
        if (swg_plan_diag_work(db, lq, n_cu, cols, group, waves, -1, workgroups == 0, false, &wk, 1.0, 0, 0) <= 0) return SWG_OK;
        if (workgroups > 0) cap_workgroups(&wk.plan[0], workgroups);
        const SwgDiagPlan &b = wk.plan[0];
        const int32_t v[8] = {wk.n_classes, b.K, b.G, b.W, b.npass, b.workgroups, (int32_t)b.n_streams, wide_form_first(16, sb.bound, 2, true) ? 1 : 0};
        memcpy(out, v, sizeof v);
    } catch (const std::exception &) {
        return SWG_ERR_NOMEM;
    }
    return SWG_OK;
}
// swg_debug_plan_systolic: the systolic fill of option engine = 1 with force_bits (0 or 32), cols_per_wave, max_waves,
// workgroups and f16 (0 = never the f16 cells) under the gap scores given, and the int32 re-score behind it.
extern "C" int swg_debug_plan_systolic(const swg_db *db, const int8_t *rows, const int8_t *idx, size_t lq, int gap_open, int gap_extend, int n_cu,
                                       long force_bits, long cols, long max_waves, long workgroups, long f16, int32_t *out)
{
    if (!db || !rows || !idx || !out || lq == 0 || n_cu <= 0 || cols < 0 || max_waves < 0 || workgroups < 0 || (force_bits != 0 && force_bits != 32))
        return SWG_ERR_ARG;
    memset(out, 0, 12 * sizeof(int32_t));
    const SwgScoreBound sb = swg_score_bound(rows, idx, lq, (uint64_t)db->max_nblk * SWG_ROWS_PER_BLK);
    const int go = gap_open + gap_extend, ge = gap_extend;
    const bool fast_ok = gap_open <= 0 && gap_extend <= 0 && -go <= SWG_I16_CEILING;
    const int bits = fast_ok && force_bits != 32 ? 16 : 32;
    SwgSystolicPlan pl, re;
    if (!systolic_plan(bits, bits == 16 ? db->n_bins : db->n_bins * 2, cols, max_waves, workgroups, lq, n_cu, &pl)) return SWG_OK;
    const bool takes_f16 = systolic_takes_f16(bits, false, pl.npass, f16 != 0 && swg_f16_gaps_ok(go, ge), sb.bound);
    const bool rescore = bits == 16 && sb.bound >= (uint64_t)SWG_I16_CEILING;
    const size_t n_slots = (size_t)db->n_bins * SWG_BIN;
    if (rescore && !systolic_plan(32, (uint32_t)std::min<size_t>(n_slots / 64, 1u << 30), 0, max_waves, workgroups, lq, n_cu, &re)) return SWG_OK;
    const int32_t v[12] = {1, pl.K, pl.W, pl.npass, pl.workgroups, takes_f16 ? 1 : 0, pl.info.max_waves, bits, rescore ? 1 : 0, re.K, re.W, re.npass};
    memcpy(out, v, sizeof v);
    return SWG_OK;
}
// swg_debug_systolic_variants: the systolic instantiations of the 16- or 32-bit cells as (K, max_waves), up to cap pairs;
// returns how many there are.
extern "C" int swg_debug_systolic_variants(int bits, int32_t *out, size_t cap)
{
    if (bits != 16 && bits != 32) return 0;
    const int n = swg_num_variants(bits);
    for (int v = 0; out && v < n && (size_t)v < cap; ++v) {
        const SwgKernelInfo info = swg_variant_info(bits, v);
        out[2 * v] = info.K, out[2 * v + 1] = info.max_waves;
    }
    return n;
}

// The colmax table of the current (query, scoring) epoch, built on the host when either has changed ...
static void ensure_prune_colmax(swg_ctx *ctx)
{
    if (ctx->prune_colmax_epoch == ctx->epoch) return;
    ctx->prune_colmax = ctx->query_pssm ? swg_prune_colmax(ctx->pssm.data(), nullptr, ctx->query_len())
                                        : swg_prune_colmax(&ctx->sub[0][0], ctx->query.data(), ctx->query_len());
    ctx->prune_colmax_epoch = ctx->epoch;
}
// ... and from it the width of this epoch's tables of k: bytes where they hold every entry, unless "prune_table_bits" says 16
static int kmer_table_bits(swg_ctx *ctx, int k)
{
    ensure_prune_colmax(ctx);
    return ctx->opt_prune_table_bits == 16 ? 16 : swg_kmer_table_bits(ctx->prune_colmax, k);
}

// Whether this search is pruned (swg_prune_plan has the rules) and by which bound, decided once the plan stands.  It only
// decides: P->prune and the context's record of the choice; prepare_prune builds what the choice needs.
static int plan_prune(swg_ctx *ctx, swg_db *db, bool want_scores, size_t k, SwgSearchPlan *P)
{
    P->prune = SwgPrunePlan();
    if (!P->use_diag || P->bits != 16) return SWG_OK;
    const SwgDiagWork &wk = P->wk;
    const SwgDiagPlan &pl = wk.plan[0];
    SwgPruneAsk a;
    a.mode = (int)ctx->opt_prune;
    a.k = k;
    a.want_scores = want_scores;
    a.gap_open = ctx->gap_open;
    a.gap_extend = ctx->gap_extend;
    a.bits = P->bits;
    a.use_diag = P->use_diag;
    a.n_classes = wk.n_classes;
    a.work_queue = diag_class_is_dynamic(ctx, db, pl) && db->ptok.ok;
    a.both_forms = P->split_at != 0u;
    a.gapless = P->gapless;
    a.batch = ctx->in_batch;
    a.prune_head = ctx->opt_prune_head;
    a.fixed = ctx->above_min > 0; // (swg_search_above: the caller's threshold, exact against the uint32 bounds)
    if (a.mode == 0 || !a.work_queue || wk.n_classes != 1) return SWG_OK;
    a.range_pairs = wk.pair_end[0] - wk.pair_begin[0];
    a.groups = diag_class_streams(ctx, db, wk, 0);
    const int form = diag_class_form(ctx, db, pl);
    std::vector<std::pair<uint32_t, uint32_t>> segs;
    bool cut = false;
    if (!token_segments(db->ptok, (uint32_t)wk.pair_begin[0], (uint32_t)wk.pair_end[0], ctx->opt_seg_blocks, pl.npass > 1 || form == 1, &segs, &cut))
        return SWG_OK; // (launch_diag reports it)
    a.n_segments = segs.size();
    P->prune = swg_prune_plan(a);
    ctx->prune_choice = SwgPruneChoice();
    if (!P->prune.on) return SWG_OK;
    P->prune.fixed_T = P->prune.fixed ? (uint32_t)ctx->above_min : 0u;
    // which bound: the colmax table, or the k-mer table of the k that pays for its build on this range (a forced k as it is)
    SwgKmerAsk ka;
    ka.forced = ctx->opt_prune_kmer;
    ka.forced_segments = ctx->opt_prune_segments;
    std::copy(ctx->opt_prune_refine, ctx->opt_prune_refine + SWG_REFINE_LEVELS, ka.forced_refine);
    ensure_prune_colmax(ctx);
    ka.table_bits = kmer_table_bits(ctx, 4);
    ka.table_bits5 = kmer_table_bits(ctx, 5);
    ka.pruned = true;
    ka.lq = ctx->query_len();
    ka.pair_rows = 4ull * (db->ptok.pair_blocks_prefix[wk.pair_end[0]] - db->ptok.pair_blocks_prefix[wk.pair_begin[0]]);
    ka.fill_rate = swg_kmer_fill_rate(ka.lq);
    P->prune.kmer = swg_prune_kmer_choice(ka, &P->prune.segments);
    // how a stage is cut: pair by pair, behind the second-level bound where that pays, or the prefix of the length order
    P->prune.prefix_cut = ctx->opt_prune_cut == 1 && !P->prune.fixed; // (a caller's threshold takes the list)
    // (the fifth level: e > 0 and second entries that are bytes)
    ka.fixed = P->prune.fixed;
    ka.refine5_ok = ctx->gap_extend <= 0 && swg_kmer_refine5_admitted(ctx->prune_colmax, (int)std::min<long>(-(long)ctx->gap_extend, 65536), ka.lq);
    swg_prune_refine_choices(ka, P->prune.kmer, P->prune.segments, P->prune.refine);
    // (not under the prefix cut; and a context that could not allocate a table a level reads searches without the level:
    // reserve_refine_table)
    for (int i = 0; i < SWG_REFINE_LEVELS; ++i) {
        const int reads = SWG_REFINE_LEVEL[i].reads;
        if (P->prune.prefix_cut || ctx->kmer_refine_refused[i] || (reads >= 0 && ctx->kmer_refine_refused[reads])) P->prune.refine[i] = 0;
    }
    // whether the first level's launch waits for a threshold (the pairs whose colmax bound is below it are not walked)
    ka.forced_gate = ctx->opt_prune_gate;
    // (not under the prefix cut, which like the levels behind the first keeps to what it was measured with)
    P->prune.gate = !P->prune.prefix_cut && swg_prune_gate_choice(ka, P->prune.kmer, P->prune.segments);
    ctx->prune_choice.kmer = P->prune.kmer, ctx->prune_choice.segments = P->prune.segments, ctx->prune_choice.gate = P->prune.gate ? 1 : 0;
    std::copy(P->prune.refine, P->prune.refine + SWG_REFINE_LEVELS, ctx->prune_choice.refine);
    return SWG_OK;
}

// A k-mer table of (k, S) for the current (query, scoring) epoch: the class profile from the device copies
// of table and query, then every class block's best cell per segment, both queued on the context's stream -- behind the
// copy of the query a set_query queued there and behind any search still in flight, in front of the bound kernel that
// reads it: the rule the profiles follow (ensure_profile_cols).  A table that holds (epoch, k, S) already is left alone; it
// grows when S x entries does.  Which (k, S) a table may hold is the caller's to say.
// spans: the fifth level's second entries instead (swg_kmer_table5_kernel<E, true>), of k = 5 as bytes.  *builds: the
// counter of the level the table belongs to.
static int ensure_kmer_table(swg_ctx *ctx, SwgKmerTable *t, uint64_t *builds, int k, int S, bool spans = false)
{
    const int bits = kmer_table_bits(ctx, k);
    if (t->holds(ctx->epoch, k, S, bits)) return SWG_OK;
    const size_t lq = ctx->query_len();
    int rc;
    if ((rc = device_grow(ctx, &ctx->d_kmer_cprof, &ctx->d_kmer_cprof_cap, lq * 32)) != SWG_OK) return rc;
    const size_t bytes = (size_t)swg_kmer_entries(k) * (size_t)S * (size_t)(bits / 8);
    if (t->cap < bytes) t->epoch = 0; // (allocated anew below: what it held is gone)
    if ((rc = device_grow(ctx, &t->d, &t->cap, bytes)) != SWG_OK) return rc;
    // (gap scores: a gap's first residue costs open + extend, every further one extend -- SwgSearchPlan's go / ge)
    const long go = (long)ctx->gap_open + ctx->gap_extend, ge = ctx->gap_extend;
    HIP_TRY(ctx, swg_launch_kmer_table(ctx->d_sub, ctx->d_query, ctx->query_pssm ? ctx->d_pssm : nullptr, (uint32_t)lq, (uint32_t)-go, (uint32_t)-ge, k,
                                       (uint32_t)S, ctx->d_kmer_cprof, t->d, bits, ctx->stream, spans));
    t->epoch = ctx->epoch, t->k = k, t->segments = S, t->bits = bits;
    ++*builds;
    return SWG_OK;
}

// A reserved table (SwgRefineLevel::reserved: the fourth level's and the fifth's, 1.32 GB each): the buffer of row i's
// table is allocated in front of the search that first wants it, and an allocation that fails is no error -- the search,
// and every later one of this context, runs without the levels that read the table (the capacity is written only once
// the buffer stands; a table refused once is not asked for again).  -> whether the buffer stands.
static bool reserve_refine_table(swg_ctx *ctx, int i)
{
    SwgKmerTable *t = &ctx->kmer_refine[i];
    const size_t bytes = (size_t)swg_kmer_entries(SWG_REFINE_LEVEL[i].k) * SWG_KMER_REFINE4_SEGMENTS;
    if (ctx->kmer_refine_refused[i]) return false;
    if (t->d && t->cap >= bytes) return true;
    (void)hipFree(t->d);
    t->d = nullptr, t->cap = 0, t->epoch = 0;
    uint8_t *d = nullptr;
    const bool refuse = g_fail_alloc_site == 3 + i; // (swg_debug_fail_alloc sites 5 and 6, 1 + the level: this allocation fails, once)
    if (refuse) g_fail_alloc_site = 0;
    if (refuse || hipSetDevice(ctx->device) != hipSuccess || hipMalloc(&d, bytes) != hipSuccess) {
        (void)hipGetLastError(); // (taken: the search goes on)
        ctx->kmer_refine_refused[i] = true;
        return false;
    }
    t->d = d, t->cap = bytes;
    return true;
}
// The reserved tables of the levels a plan has; a level that reads a table which cannot be had goes, from the plan and
// from what the context reports (the fifth level reads the fourth's table and its own: without either buffer the search
// runs without it -- and where it was chosen behind an automatic fourth level that is now off, without both).
static void reserve_refine_tables(swg_ctx *ctx, SwgPrunePlan *pr)
{
    for (int i = 0; i < SWG_REFINE_LEVELS; ++i) {
        const SwgRefineLevel &L = SWG_REFINE_LEVEL[i];
        if (!pr->refine[i] || !L.reserved) continue;
        if ((L.reads >= 0 && !reserve_refine_table(ctx, L.reads)) || !reserve_refine_table(ctx, i)) pr->refine[i] = 0, ctx->prune_choice.refine[i] = 0;
    }
}

// What a pruned search reads besides the fill's own: the colmax table for the current query and scoring (built on the
// host when either has changed; it travels to the bound kernels as a launch argument), the k-mer tables of the plan's
// choice -- the first level's within SWG_KMER_TABLE_BUDGET, the second and third levels' queued behind it and counted apart -- and
// the slot's buffer of pair bounds (swg_prune_layout).
static int prepare_prune(swg_ctx *ctx, swg_db *db, const SwgPrunePlan &pr)
{
    int rc;
    ensure_prune_colmax(ctx);
    if (pr.kmer > 1) {
        const int k = pr.kmer, S = pr.segments;
        if (S < 1 || S > (int)SWG_KMER_MAX_SEGMENTS) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "the k-mer bound's table: %d segments (1..32)", S);
        if (!swg_kmer_table_admitted(k, S))
            return swg_set_ctx_error(ctx, SWG_ERR_ARG, "the k-mer bound's table of k = %d in %d segments is %zu MB: above its budget of %zu MB (prune_kmer, prune_segments)", k,
                                     S, (size_t)swg_kmer_entries(k) * (size_t)S * sizeof(uint16_t) >> 20, (size_t)(SWG_KMER_TABLE_BUDGET >> 20));
        if ((rc = ensure_kmer_table(ctx, &ctx->kmer_first[k - 4], &ctx->kmer_builds, k, S)) != SWG_OK) return rc;
    }
    // the levels behind the first: segments the level's option can name, a table of 5-residue blocks as bytes only; then
    // the table it reads besides its own (the fifth level the fourth's -- with or without a fourth level's walk) and its own
    for (int i = 0; i < SWG_REFINE_LEVELS; ++i) {
        const SwgRefineLevel &L = SWG_REFINE_LEVEL[i];
        const int S = pr.refine[i];
        if (!S) continue;
        if ((S != L.forced[0].segments && S != L.forced[1].segments) || (L.k == 5 && !swg_kmer_refine4_admitted(kmer_table_bits(ctx, 5))))
            return swg_set_ctx_error(ctx, SWG_ERR_ARG, L.table_error, S);
        if (L.reads >= 0 && (rc = ensure_kmer_table(ctx, &ctx->kmer_refine[L.reads], &ctx->kmer_refine_builds[L.reads], SWG_REFINE_LEVEL[L.reads].k, S)) != SWG_OK)
            return rc;
        if ((rc = ensure_kmer_table(ctx, &ctx->kmer_refine[i], &ctx->kmer_refine_builds[i], L.k, S, L.spans)) != SWG_OK) return rc;
    }
    swg_db::Bufs &b = db->bufs[ctx->cur - ctx->slots];
    const size_t n_pairs = (size_t)swg_db_pair_count(db);
    if ((rc = device_grow(ctx, &b.d_pair_bound, &b.pair_bound_cap, n_pairs, swg_prune_layout(b.d_pair_bound, n_pairs).words - n_pairs)) != SWG_OK) return rc;
    db->d_pair_bound = b.d_pair_bound;
    return SWG_OK;
}

// Profiles, scratch and the bin image of a planned search, and what its pruning reads.
static int prepare_search(swg_ctx *ctx, swg_db *db, const SwgSearchPlan &P)
{
    int rc = SWG_OK;
    const bool systolic_fill = !P.use_diag && !P.use_q32 && !(P.bits == 32 && P.use_diag32);
    const bool systolic_rescore = P.may_saturate && !P.use_diag32;
    const size_t bin32_scratch = P.bin32 && P.npass32 > 1 ? ((size_t)db->max_nblk * 4 + 4) * 4 * 16 * (size_t)ctx->n_cu : 0; // dwords: one uint4 per stream row
    if (P.bin32) {
        rc = ensure_profile_cols(ctx, 1, (uint32_t)(P.npass32 * 64 * SWG_DIAG32_K), 4, (1ull << 30) ^ (uint64_t)P.npass32);
        if (rc != SWG_OK) return rc;
        if ((rc = ensure_scratch(ctx, bin32_scratch)) != SWG_OK) return rc;
    }
    if (P.use_diag) {
        if ((rc = prepare_diag(ctx, db, P.wk)) == SWG_OK && P.prune.on) rc = prepare_prune(ctx, db, P.prune);
    } else if (systolic_fill) rc = ensure_profile(ctx, P.main_pl);
    // (the int32 work-queue fill builds its profiles at the launch)
    if (rc != SWG_OK) return rc;
    if (systolic_rescore && (rc = ensure_profile(ctx, P.re_pl)) != SWG_OK) return rc;
    size_t need = bin32_scratch;
    if (systolic_fill && P.main_pl.npass > 1)
        need = std::max(need, (size_t)P.main_pl.workgroups * db->max_nblk * SWG_ROWS_PER_BLK * 64 * P.main_pl.info.nb);
    if (systolic_rescore && P.re_pl.npass > 1)
        need = std::max(need, (size_t)P.re_pl.workgroups * db->max_nblk * SWG_ROWS_PER_BLK * 64 * P.re_pl.info.nb);
    if ((rc = ensure_scratch(ctx, need)) != SWG_OK) return rc;
    // the systolic engine and the bin-based int32 kernel read the bin image (built on the device on first use)
    if ((!P.use_diag && !P.use_q32) || (P.int32_level && !P.q32_ok)) return ensure_bins(ctx, db);
    return SWG_OK;
}

// The first level on the main stream: the diagonal engine, the int32 work queue, the bin-based int32 kernel or the
// systolic engine (events ev[0] before the buffers are cleared, ev[1] .. ev[2] around the fill).
static int enqueue_fill(swg_ctx *ctx, swg_db *db, const SwgSearchPlan &P, SwgSlot *S)
{
    hipStream_t s = ctx->stream;
    const size_t n_slots = (size_t)db->n_bins * SWG_BIN;
    HIP_TRY(ctx, hipEventRecord(S->ev[0], s));
    HIP_TRY(ctx, swg_launch_zero2(db->d_scores, n_slots * 4, db->d_counters, SWG_COUNTER_BYTES, s)); // (one launch, not two memsets)
    S->two_ends = false;
    S->fill_launches = 0;
    S->pruned = false;
    if (P.use_diag) return launch_diag(ctx, db, P.wk, P.go, P.ge, &S->two_ends, &P.prune, S->k);
    if (P.use_q32)
        return launch_q32(ctx, db, P.wk32, P.go, P.ge, nullptr, nullptr, 0, db->d_counters + SWG_QUEUE_WORD(0), &S->two_ends, true, P.exact32);
    if (!(P.bits == 32 && P.use_diag32)) return launch_systolic(ctx, db, P.main_pl, P.go, P.ge);
    SwgFillParams p = fill_params_base(ctx, db);
    p.profile = ctx->d_profile[1];
    p.queue = db->d_counters + SWG_WORD_WORK_QUEUE;
    p.n_items = (uint32_t)n_slots;
    p.npass = (uint32_t)P.npass32;
    p.go = P.go;
    p.ge = P.ge;
    p.scratch_wg_dwords = ((uint64_t)db->max_nblk * 4 + 4) * 4;
    HIP_TRY(ctx, hipEventRecord(S->ev[1], s));
    HIP_TRY(ctx, swg_launch_diag32(16, (int)std::min<size_t>((size_t)ctx->n_cu, (n_slots + 15) / 16), p, s));
    HIP_TRY(ctx, hipEventRecord(S->ev[2], s));
    return SWG_OK;
}

// The levels behind the first: the pairs the f16 cells flagged are collected and run again on int16 cells, then what
// saturated the last 16-bit level is collected and re-scored in int32 (event ev[3] at the end).
static int enqueue_rescore(swg_ctx *ctx, swg_db *db, const SwgSearchPlan &P, SwgSlot *S)
{
    hipStream_t s = ctx->stream;
    const size_t lq = ctx->query_len();
    const size_t n_slots = (size_t)db->n_bins * SWG_BIN;
    const bool some_f16 = P.some_f16();
    int rc = SWG_OK;
    uint32_t *seq_list = db->d_list;
    if (P.may_saturate && some_f16) {
        // (the flagged pairs are the list's length; their rows / 16 the veto's input)
        HIP_TRY(ctx, swg_launch_collect_flagged_pairs(db->d_scores, P.split_at, (uint32_t)(n_slots / 2), SWG_F16_CEILING, db->d_list, db->d_counters + SWG_WORD_FLAGGED_PAIRS,
                                                      db->d_counters + SWG_WORD_FLAGGED_SEQS, db->d_lens, db->d_counters + SWG_WORD_FLAGGED_ROWS, s));
        SwgDiagPlan lp;
        const uint32_t guess = db->sat_hint > 0 ? (uint32_t)std::min<long long>(db->sat_hint, 1ll << 30) : 1u;
        if (!i16_list_plan(ctx->n_cu, lq, guess, P.wk.plan[0], &lp)) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "no geometry for the int16 re-run");
        HIP_TRY(ctx, hipMemsetAsync(db->d_counters + SWG_QUEUE_WORD(0), 0, (size_t)(SWG_COUNTER_BYTES - SWG_QUEUE_WORD(0) * 4u), s));
        if ((rc = launch_dyn_list(ctx, db, lp, P.rerun_wide, P.go, P.ge, db->d_list, db->d_counters + SWG_WORD_FLAGGED_PAIRS, s)) != SWG_OK) return rc;
        seq_list = db->d_list + n_slots; // (the pair list keeps the first half)
    }
    if (P.int32_level) {
        // (the saturated sequences are the list's length)
        HIP_TRY(ctx, swg_launch_collect_saturated(db->d_scores, (uint32_t)n_slots, P.level_ceiling, seq_list, db->d_counters + SWG_WORD_SATURATED,
                                                  some_f16 ? nullptr : db->d_lens, db->d_counters + SWG_WORD_FLAGGED_ROWS, s));
        SwgFillParams p = fill_params_base(ctx, db);
        p.profile = ctx->d_profile[1];
        p.queue = db->d_counters + SWG_WORD_RESCORE_QUEUE;
        p.list = seq_list;
        p.list_count = db->d_counters + SWG_WORD_SATURATED;
        p.go = P.go32; // (the first level's gap scores, except in a gapless search: see plan_search)
        p.ge = P.ge32;
        SwgDiagWork wkl;
        // The work-queue re-score reads the count on the device and leaves at once when it is zero, so it is queued
        // behind every fill that may flag something and the host never waits for the count in the middle of a
        // search (it did until round 3: a round trip per search, and the end of the two-deep pipeline of
        // swg_search_begin).  Only its lane-group width is a guess -- few flagged sequences get 64 lanes each,
        // many the narrowest group that covers the query -- made from what the last search of this database saw.
        const uint32_t guess = !some_f16 && db->sat_hint > 0 ? (uint32_t)std::min<long long>(db->sat_hint, 1ll << 30) : 1u;
        if (P.use_diag32 && P.q32_ok && q32_list_plan(ctx, lq, guess, &wkl)) {
            // (fresh queue counters and rank table: the fill's are spent; no events of its own: the
            // re-score is timed as ev[2] .. ev[3] like the other re-score forms)
            HIP_TRY(ctx, hipMemsetAsync(db->d_counters + SWG_QUEUE_WORD(0), 0,
                                        (size_t)(SWG_COUNTER_BYTES - SWG_QUEUE_WORD(0) * 4u), s));
            bool two = false;
            rc = launch_q32(ctx, db, wkl, P.go32, P.ge32, seq_list, db->d_counters + SWG_WORD_SATURATED, std::max<uint32_t>(2u * guess, 4096u),
                            db->d_counters + SWG_QUEUE_WORD(0), &two, false);
            if (rc != SWG_OK) return rc;
        } else if (P.use_diag32) {
            // the bin-based kernel (positive gap scores never get here; a database beyond the queue's
            // indices, work_queue = 0): its shape comes from the count, read back over PCIe
            uint32_t n_sat = 0;
            HIP_TRY(ctx, hipMemcpyAsync(&n_sat, db->d_counters + SWG_WORD_SATURATED, 4, hipMemcpyDeviceToHost, s));
            HIP_TRY(ctx, spin_sync(ctx, s));
            if (n_sat > 0) {
                int W = (int)((n_sat + (uint32_t)ctx->n_cu - 1) / (uint32_t)ctx->n_cu);
                W = std::min(16, std::max(4, (W + 3) / 4 * 4));
                const int wgs = (int)std::min<uint32_t>((uint32_t)ctx->n_cu, (n_sat + W - 1) / W);
                p.npass = (uint32_t)P.npass32;
                p.scratch_wg_dwords = ((uint64_t)db->max_nblk * 4 + 4) * 4;
                HIP_TRY(ctx, swg_launch_diag32(W, wgs, p, s));
            }
        } else {
            p.npass = (uint32_t)P.re_pl.npass;
            p.scratch_wg_dwords = (uint64_t)db->max_nblk * SWG_ROWS_PER_BLK * 64 * P.re_pl.info.nb;
            HIP_TRY(ctx, swg_launch_fill(32, P.re_pl.variant, P.re_pl.W, P.re_pl.workgroups, p, s));
        }
    }
    HIP_TRY(ctx, hipEventRecord(S->ev[3], s));
    return SWG_OK;
}

// Top-K and read-out go to their own stream: the next search's fill is queued right behind this
// one's on the main stream and these small kernels run beside its start instead of holding it
// up (the output buffers belong to this in-flight slot until swg_search_end).  swg_search_end waits for ev_done.
static int enqueue_readout(swg_ctx *ctx, swg_db *db, SwgSlot *S)
{
    hipStream_t s = ctx->stream;
    const size_t n_slots = (size_t)db->n_bins * SWG_BIN;
    const size_t k = S->k;
    // (the read-out stream exists from the context's second search on: ensure_stream3)
    S->side = false;
    if (ctx->opt_side_readout && ctx->n_begun > 0) {
        const int r3 = ensure_stream3(ctx);
        if (r3 != SWG_OK) return r3;
        HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream3, S->ev[3], 0));
        s = ctx->stream3;
        S->side = true;
    }
    ++ctx->n_begun;
    // top-K on the device unless every score goes to the host anyway
    S->dev_topk = k > 0 && !S->want_scores && k <= SWG_TOPK_CAND_CAP / 2;
    // swg_search_above: every slot at or above the caller's threshold, behind the last re-score; the counter word came
    // zeroed with the block and counts them all, the keys that fit stay on the device until swg_search_end knows how many
    S->above_min = ctx->above_min;
    if (S->above_min > 0) {
        const swg_db::Bufs &b = db->bufs[S - ctx->slots];
        S->above_cap = b.d_above ? b.above_cap : SWG_ABOVE_KEYS_FLOOR;
        HIP_TRY(ctx, swg_launch_above_compact(db->d_scores, db->d_order, (uint32_t)n_slots, S->above_min, b.d_above ? b.d_above : db->d_keys,
                                              (uint32_t)S->above_cap, db->d_counters + SWG_ABOVE_WORD_COUNT, s));
    }
    if (S->dev_topk)
        HIP_TRY(ctx, swg_launch_topk(db->d_scores, db->d_order, (uint32_t)n_slots, (uint32_t)k, db->d_hist,
                                     db->d_counters + SWG_WORD_TOPK_THR, db->d_keys, SWG_TOPK_CAND_CAP, db->d_counters + SWG_WORD_TOPK_COUNT, s));
    HIP_TRY(ctx, hipEventRecord(S->ev[4], s));
    // read-out, queued behind the kernels
    S->need_scores = S->want_scores || (k > 0 && !S->dev_topk);
    S->first_chunk = SWG_TOPK_CAND_CAP;
    if (S->dev_topk)
        HIP_TRY(ctx, hipMemcpyAsync(S->h_cand, db->d_keys, S->first_chunk * 8, hipMemcpyDeviceToHost, s));
    if (S->need_scores) {
        const int rc = slot_scores(ctx, S, n_slots);
        if (rc != SWG_OK) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(S->h_scores, db->d_scores, n_slots * 4, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(ctx, hipMemcpyAsync(S->h_counters, db->d_counters, 128, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipEventRecord(S->ev_done, s));
    return SWG_OK;
}

// Queues one whole search on the context's stream and returns without waiting (except on the
// first search of a query length, which tunes the geometry when allow_autotune says so, and when int16 scores may
// saturate without the work queue, where the number of flagged sequences is read back to size the re-score).
static int search_begin(swg_ctx *ctx, swg_db *db, bool want_scores, size_t k, bool allow_autotune, SwgSlot *S)
{
    if (!ctx || !db) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "swg_search: NULL argument");
    if (!ctx->have_scoring) return swg_set_ctx_error(ctx, SWG_ERR_STATE, "swg_search: no scoring set");
    if (ctx->query_len() == 0) return swg_set_ctx_error(ctx, SWG_ERR_STATE, "swg_search: no query set");
    if (db->device != ctx->device || !db->d_codes)
        return swg_set_ctx_error(ctx, SWG_ERR_STATE, "swg_search: database is not resident on device %d",
                                 ctx->device);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = ensure_slot(ctx, S);
    if (rc != SWG_OK) return rc;
    ctx->cur = S;
    if ((rc = select_bufs(ctx, db, (int)(S - ctx->slots))) != SWG_OK) return rc;
    S->bufs = db->bufs[S - ctx->slots];
    S->db = db;
    S->k = k;
    S->want_scores = want_scores;
    memset(&S->st, 0, sizeof S->st);
    S->st.cells = (uint64_t)ctx->query_len() * db->residues;
    S->st.bytes_alg = db->residues + 8ull * db->n_local + 32ull * ctx->query_len() + 1024ull;
    S->plan = SwgSearchPlan(); // (bits = 0 marks "nothing queued" for an empty database)
    if (db->n_bins == 0) return SWG_OK;
    if ((rc = plan_search(ctx, db, allow_autotune, &S->plan)) != SWG_OK) return rc;
    if ((rc = plan_prune(ctx, db, want_scores, k, &S->plan)) != SWG_OK) return rc;
    reserve_refine_tables(ctx, &S->plan.prune);
    if ((rc = prepare_search(ctx, db, S->plan)) != SWG_OK) return rc;
    if ((rc = enqueue_fill(ctx, db, S->plan, S)) != SWG_OK) return rc;
    if ((rc = enqueue_rescore(ctx, db, S->plan, S)) != SWG_OK) return rc;
    return enqueue_readout(ctx, db, S);
}

// Scores by sorted rank to the caller's order, and the k best of them selected on the host.
static void deliver_scores(const swg_db *db, const int32_t *h_scores, size_t n_slots, int32_t *scores_out, swg_hit *topk_out,
                           size_t k, size_t *n_hits)
{
    if (scores_out)
        for (size_t i = 0; i < n_slots; ++i) {
            const uint32_t oi = db->order[i];
            if (oi != 0xFFFFFFFFu) scores_out[oi] = h_scores[i];
        }
    if (k > 0 && topk_out) {
        std::vector<uint64_t> keys;
        keys.reserve(db->n_local);
        for (size_t i = 0; i < n_slots; ++i) {
            const uint32_t oi = db->order[i];
            if (oi != 0xFFFFFFFFu) keys.push_back(swg_hit_key(h_scores[i], oi));
        }
        const size_t m = std::min(k, keys.size());
        std::partial_sort(keys.begin(), keys.begin() + m, keys.end(), std::greater<uint64_t>());
        for (size_t i = 0; i < m; ++i) swg_key_hit(keys[i], &topk_out[i]);
        if (n_hits) *n_hits = m;
    } else if (n_hits) {
        *n_hits = 0;
    }
}

// What swg_search_above hands to search_end: where its hits go, how many fit, and the count of all of them.
struct SwgAboveOut {
    swg_hit *hits_out = nullptr;
    size_t cap = 0;
    uint64_t n_total = 0;
};

// The read-out of swg_search_above, once the search's counter words are back: the count of every slot at or above the
// threshold is the answer's n_total; the keys that fitted the device buffer are copied back and sorted as 64-bit keys
// (the library's total order).  A count beyond the buffer grows it for the next search -- the new capacity is committed
// only once the allocation stands -- and, where the caller takes any hits, this search selects from the score array on
// the host, as the top-K does at its capacity edge: the keys dropped are whichever came last, not the worst.
static int deliver_above(swg_ctx *ctx, SwgSlot *S, hipStream_t s, SwgAboveOut *out, size_t *n_hits)
{
    swg_db *db = S->db;
    const size_t n_slots = (size_t)db->n_bins * SWG_BIN;
    const size_t count = S->h_counters[SWG_ABOVE_WORD_COUNT], kept = std::min(count, S->above_cap);
    out->n_total = count;
    const size_t m = std::min(out->cap, count);
    if (count > S->above_cap) {
        swg_db::Bufs &b = db->bufs[S - ctx->slots];
        const size_t want = std::min<size_t>(db->n_local, std::max<size_t>(count + count / 4, 2 * (size_t)SWG_ABOVE_KEYS_FLOOR));
        uint64_t *grown = nullptr;
        if (hipMalloc(&grown, want * 8) == hipSuccess) { // (no room: the next search falls back as this one does)
            (void)hipFree(b.d_above);
            b.d_above = grown;
            b.above_cap = want;
        } else
            (void)hipGetLastError();
    }
    std::vector<uint64_t> keys;
    if (count > S->above_cap && m > 0) { // (the device dropped keys, any of them: what it kept need not hold the best)
        int rc = slot_scores(ctx, S, n_slots);
        if (rc != SWG_OK) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(S->h_scores, S->bufs.d_scores, n_slots * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(ctx, spin_sync(ctx, s));
        keys.reserve(count);
        for (size_t i = 0; i < n_slots; ++i) {
            const uint32_t oi = db->order[i];
            if (oi != 0xFFFFFFFFu && S->h_scores[i] >= S->above_min) keys.push_back(swg_hit_key(S->h_scores[i], oi));
        }
    } else if (m > 0) {
        keys.resize(kept);
        const uint64_t *d_keys = S->above_cap > SWG_ABOVE_KEYS_FLOOR ? S->bufs.d_above : S->bufs.d_keys;
        HIP_TRY(ctx, hipMemcpyAsync(keys.data(), d_keys, kept * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(ctx, spin_sync(ctx, s));
    }
    const size_t w = std::min(m, keys.size());
    std::partial_sort(keys.begin(), keys.begin() + w, keys.end(), std::greater<uint64_t>());
    for (size_t i = 0; i < w; ++i) swg_key_hit(keys[i], &out->hits_out[i]);
    if (n_hits) *n_hits = w;
    return SWG_OK;
}

static int search_end(swg_ctx *ctx, SwgSlot *S, int32_t *scores_out, swg_hit *topk_out, size_t *n_hits,
                      swg_stats *stats, SwgAboveOut *above = nullptr)
{
    swg_db *db = S->db;
    const size_t k = S->k;
    if (n_hits) *n_hits = 0;
    if (k > 0 && !topk_out) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "swg_search: k > 0 but topk_out NULL");
    if (scores_out && !S->want_scores)
        return swg_set_ctx_error(ctx, SWG_ERR_ARG, "swg_search_end: scores were not requested at swg_search_begin");
    swg_stats &st = S->st;
    const SwgSearchPlan &P = S->plan;
    if (P.bits == 0) { // empty database
        if (above) above->n_total = 0;
        if (stats) *stats = st;
        return SWG_OK;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ctx->cur = S;
    hipStream_t s = S->side ? ctx->stream3 : ctx->stream; // (the stream this search's read-out was queued on: not behind queued fills)
    for (;;) { // poll: a blocking wait can cost milliseconds of wake-up latency on a busy host
        const hipError_t q = hipEventQuery(S->ev_done);
        if (q == hipSuccess) break;
        if (q != hipErrorNotReady) HIP_TRY(ctx, q);
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
    }
    const size_t n_slots = (size_t)db->n_bins * SWG_BIN;
    const bool some_f16 = P.some_f16();
    const SwgDiagWork &wk = P.wk;
    const SwgDiagPlan &dpl = wk.plan[0];
    const uint32_t *h_counters = S->h_counters;
    int rc = SWG_OK;
    const bool cand_ok = S->dev_topk && h_counters[SWG_WORD_TOPK_OVERFLOW] == 0 && h_counters[SWG_WORD_TOPK_COUNT] <= SWG_TOPK_CAND_CAP;
    if (S->dev_topk && !cand_ok) { // threshold beyond the histogram or too many ties: select on the host
        if ((rc = slot_scores(ctx, S, n_slots)) != SWG_OK) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(S->h_scores, S->bufs.d_scores, n_slots * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(ctx, spin_sync(ctx, s));
    }

    float ms = 0.f;
    if ((rc = diag_fill_ms(ctx, S->two_ends, &st.fill_ms)) != SWG_OK) return rc;
    HIP_TRY(ctx, hipEventElapsedTime(&ms, S->ev[2], S->ev[3]));
    st.rescore_ms = P.may_saturate ? ms : 0.0;
    HIP_TRY(ctx, hipEventElapsedTime(&ms, S->ev[0], S->ev[4]));
    st.total_ms = ms;
    HIP_TRY(ctx, hipEventElapsedTime(&ms, S->ev[3], S->ev[4]));
    const double topk_dev_ms = ms;
    st.n_rescored = h_counters[some_f16 ? SWG_WORD_FLAGGED_SEQS : SWG_WORD_SATURATED];
    st.path_bits = P.bits;
    st.cell_form = P.use_diag ? diag_class_form(ctx, db, dpl) : P.main_pl.f16 ? 2 : 0;
    if (st.cell_form == 3) st.cell_form = 6; // (the gapless cells: kernel form 3, reported as 6 -- 3 .. 5 are taken, see swg.h)
    if (P.use_diag && dpl.f16_from != 0u) {
        st.cell_form = dpl.wide ? 4 : 5;
        st.n_rescored = (uint64_t)h_counters[SWG_WORD_FLAGGED_SEQS] + h_counters[SWG_WORD_SATURATED]; // flagged by the f16 cells + saturated on the wide form
        st.split_rows = (int32_t)P.split_rows;
        st.fill_f16_launches = S->fill_f16_launches;
        st.cells_f16 = st.cells / std::max<uint64_t>(1, db->residues) * P.split_residues; // (cells = lq * residues)
        HIP_TRY(ctx, hipEventElapsedTime(&ms, S->ev[5], S->ev[2]));
        st.fill_f16_ms = ms;
    }
    if (P.may_saturate) {
        // what the next search's plan may assume (never its results)
        db->sat_hint = (long long)h_counters[some_f16 ? SWG_WORD_FLAGGED_PAIRS : SWG_WORD_SATURATED]; // (f16: pairs; else sequences)
        // f16 cells whose flagged pairs hold more than 1/16 of the pair rows (SWG_WORD_FLAGGED_ROWS: rows of the flagged pairs / 16;
        // a pair row is two residues) cost more in re-runs than they save: the cells save 15 % of the fill, the list
        // re-run of a share f of the rows costs f x 10 / 8.5 at about half the fill's efficiency.  Measured on config
        // 4's share with 4 % of the pair rows flagged: f16 + re-run 191 ms, int16 cells alone 200.
        if (some_f16 && !P.gapless && (uint64_t)h_counters[SWG_WORD_FLAGGED_ROWS] * 16ull * 2ull * 16ull > db->residues + 2ull * db->n_local) db->f16_veto_epoch = P.epoch;
    }
    // what a pruned search left out (swg_prune_last): from the counter words that came back with the search
    swg_prune_info &pi = ctx->prune_last;
    pi = swg_prune_info();
    pi.pruned = S->pruned ? 1 : 0;
    if (S->pruned) {
        pi.pairs_skipped = h_counters[SWG_PRUNE_WORD_CUT + 1u];
        pi.pair_rows_skipped = 4ull * ((uint64_t)h_counters[SWG_PRUNE_WORD_CUT + 2u] | ((uint64_t)h_counters[SWG_PRUNE_WORD_CUT + 3u] << 32));
        pi.threshold = h_counters[SWG_PRUNE_WORD_T];
    }
    if (P.use_diag && db->ptok.ok && !db->ptok.pair_blocks_prefix.empty())
        pi.pair_rows = 4ull * (db->ptok.pair_blocks_prefix[wk.pair_end[0]] - db->ptok.pair_blocks_prefix[wk.pair_begin[0]]);
    st.classes_overlapped = -1;
    if (P.use_diag && wk.n_classes == 2 && wk.plan[0].npass == 1 && wk.plan[1].npass == 1) {
        // did the two classes run side by side?  (stamps: complement of the earliest start, latest end)
        unsigned long long t[4];
        memcpy(t, h_counters + SWG_WORD_STAMPS(0), sizeof t);
        if (t[0] && t[1] && t[2] && t[3]) {
            const unsigned long long bulk_start = ~t[0], bulk_end = t[1], long_start = ~t[2];
            st.classes_overlapped = (bulk_end > bulk_start && long_start < bulk_start + (bulk_end - bulk_start) / 10) ? 1 : 0;
        }
    }
    if (P.use_diag) {
        st.engine = 2;
        st.cols_per_wave = dpl.K;
        st.group_lanes = dpl.G;
        st.waves = dpl.W;
        st.passes = dpl.npass;
        st.fill_launches = S->fill_launches > 0 ? S->fill_launches : dpl.npass;
        st.workgroups = diag_class_workgroups(ctx, db, wk, 0);
        st.work_queue = diag_class_is_dynamic(ctx, db, dpl) ? 1 : 0;
        st.streams = (int32_t)diag_class_streams(ctx, db, wk, 0);
        st.cells_padded = 2ull * ((uint64_t)(dpl.npass - (dpl.last_variant >= 0 ? 1 : 0)) * dpl.K + (dpl.last_variant >= 0 ? dpl.last_K : 0)) *
                          dpl.G * diag_class_blocks(ctx, db, wk, 0) * 4ull;
        st.last_pass_cols = dpl.last_variant >= 0 ? dpl.last_K : 0;
        if (wk.n_classes == 2) {
            const SwgDiagPlan &lp = wk.plan[1];
            st.long_pairs = (int32_t)(wk.pair_end[1] - wk.pair_begin[1]);
            st.long_cols_per_lane = lp.K;
            st.long_streams = (int32_t)diag_class_streams(ctx, db, wk, 1);
            st.cells_padded += 2ull * lp.npass * lp.G * lp.K * diag_class_blocks(ctx, db, wk, 1) * 4ull;
        }
    } else if (P.use_q32) {
        const SwgDiagWork &w32 = P.wk32;
        st.engine = 2;
        st.work_queue = 1;
        st.cols_per_wave = w32.plan[0].K;
        st.group_lanes = w32.plan[0].G;
        st.passes = w32.plan[0].npass;
        const uint64_t items0 = 2 * (w32.pair_end[0] - w32.pair_begin[0]);
        st.workgroups = q32_class_workgroups(ctx, w32, 0, items0, &st.waves);
        st.streams = st.workgroups * st.waves * (64 / w32.plan[0].G);
        for (int c = 0; c < w32.n_classes; ++c)
            st.cells_padded += 2ull * w32.plan[c].npass * w32.plan[c].G * w32.plan[c].K *
                               (uint64_t)(db->ptok.pair_blocks_prefix[w32.pair_end[c]] - db->ptok.pair_blocks_prefix[w32.pair_begin[c]]) * 4ull;
        if (w32.n_classes == 2) {
            st.long_pairs = (int32_t)(w32.pair_end[1] - w32.pair_begin[1]);
            st.long_cols_per_lane = w32.plan[1].K;
        }
    } else if (P.bits == 32 && P.use_diag32) {
        st.engine = 2;
        st.cols_per_wave = SWG_DIAG32_K;
        st.group_lanes = 64;
        st.waves = 16;
        st.passes = P.npass32;
        st.workgroups = (int)std::min<size_t>((size_t)ctx->n_cu, (n_slots + 15) / 16);
        st.cells_padded = (uint64_t)P.npass32 * 64 * SWG_DIAG32_K * ((uint64_t)db->rows_padded);
    } else {
        const SwgSystolicPlan &mp = P.main_pl;
        st.engine = 1;
        st.cols_per_wave = mp.K;
        st.waves = mp.W;
        st.passes = mp.npass;
        st.workgroups = mp.workgroups;
        st.cells_padded = (uint64_t)mp.npass * mp.W * mp.K * db->rows_padded;
    }
    if (st.fill_launches <= 0) st.fill_launches = std::max(1, st.passes);

    const auto t0 = std::chrono::steady_clock::now();
    if (above) {
        if ((rc = deliver_above(ctx, S, s, above, n_hits)) != SWG_OK) return rc;
    } else if (k > 0 && cand_ok) { // (the device's candidates: every hit with a score >= the k-th best one; no score array was asked for)
        uint64_t *keys = S->h_cand;
        const size_t nc = h_counters[SWG_WORD_TOPK_COUNT], m = std::min(k, nc);
        std::partial_sort(keys, keys + m, keys + nc, std::greater<uint64_t>());
        for (size_t i = 0; i < m; ++i) swg_key_hit(keys[i], &topk_out[i]);
        if (n_hits) *n_hits = m;
    } else {
        if (k > 0) fail_alloc_here(3);
        deliver_scores(db, S->h_scores, n_slots, scores_out, topk_out, k, n_hits);
    }
    st.topk_ms = topk_dev_ms + std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (stats) *stats = st;
    return SWG_OK;
}

// test hooks: what a pruned search left on the device, read once everything queued has run.  `table`, with table_out (or
// NULL): the context's table of (k, S), an error unless it holds exactly that for the current query and scoring.
// bound_out / list_out (or NULL; pair_cap entries each): the pair bounds of the search last begun on db as it left them,
// and the list words (one per pair: a stage's list starts at its first pair's word); stages_out (or NULL): four words per
// stage cut pair by pair, {begin, end, T, kept pairs}.  info[0..6] = the k that search cut by (0: not pruned), first-level
// builds queued so far, the database's pairs, S, S2 (0: no second level), second-level builds, stages written.
static int debug_prune_read(swg_ctx *ctx, const swg_db *db, const char *fn, const SwgKmerTable *table, int k, int S, uint16_t *table_out, uint32_t *bound_out,
                            uint32_t *list_out, size_t pair_cap, uint32_t *stages_out, size_t stages_cap, int n_info, uint64_t *info)
{
    if (!ctx || !info) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "%s: NULL argument", fn);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipDeviceSynchronize());
    const size_t n_pairs = db ? (size_t)swg_db_pair_count(db) : 0;
    const uint64_t all[7] = {(uint64_t)ctx->prune_choice.kmer, ctx->kmer_builds, n_pairs, (uint64_t)ctx->prune_choice.segments, (uint64_t)ctx->prune_choice.refine[0],
                             ctx->kmer_refine_builds[0], 0};
    std::copy(all, all + n_info, info);
    if (table_out) {
        if (!table || !table->holds(ctx->epoch, k, S, table->bits))
            return swg_set_ctx_error(ctx, SWG_ERR_STATE, "%s: no table of k = %d in %d segments for the current query and scoring", fn, k, S);
        const size_t entries = (size_t)swg_kmer_entries(k) * (size_t)S;
        if (table->bits == 8) { // (widened: the hooks hand out uint16_t whatever the device keeps)
            std::vector<uint8_t> narrow(entries);
            HIP_TRY(ctx, hipMemcpy(narrow.data(), table->d, entries, hipMemcpyDeviceToHost));
            std::copy(narrow.begin(), narrow.end(), table_out);
        } else
            HIP_TRY(ctx, hipMemcpy(table_out, table->d, entries * sizeof(uint16_t), hipMemcpyDeviceToHost));
    }
    if (bound_out || list_out || stages_out) {
        if (!db || !db->d_pair_bound || pair_cap < n_pairs) return swg_set_ctx_error(ctx, SWG_ERR_STATE, "%s: no pair bounds on this database, or too little room", fn);
        const SwgPruneLayout L = swg_prune_layout(db->d_pair_bound, n_pairs);
        if (bound_out) HIP_TRY(ctx, hipMemcpy(bound_out, L.bounds, n_pairs * sizeof(uint32_t), hipMemcpyDeviceToHost));
        if (list_out) HIP_TRY(ctx, hipMemcpy(list_out, L.lists, n_pairs * sizeof(uint32_t), hipMemcpyDeviceToHost));
        if (stages_out) {
            const size_t n = std::min<size_t>(std::min<size_t>(db->prune_stages.size() / 2, SWG_PRUNE_STAGE_RECS), stages_cap);
            std::vector<uint32_t> recs(2 * n);
            if (n) HIP_TRY(ctx, hipMemcpy(recs.data(), L.recs, 2 * n * sizeof(uint32_t), hipMemcpyDeviceToHost));
            for (size_t i = 0; i < n; ++i)
                stages_out[4 * i] = db->prune_stages[2 * i], stages_out[4 * i + 1] = db->prune_stages[2 * i + 1], stages_out[4 * i + 2] = recs[2 * i],
                               stages_out[4 * i + 3] = recs[2 * i + 1];
            info[6] = n;
        }
    }
    return SWG_OK;
}
// the unsegmented table of k (a table built with more segments is refused) and the bounds: info[0..2]
extern "C" int swg_debug_prune_kmer_read(swg_ctx *ctx, const swg_db *db, int k, uint16_t *table_out, uint32_t *bound_out, size_t bound_cap,
                                         uint64_t *info)
{
    return debug_prune_read(ctx, db, "swg_debug_prune_kmer_read", ctx && (k == 4 || k == 5) ? &ctx->kmer_first[k - 4] : nullptr, k, 1, table_out, bound_out, nullptr,
                            bound_cap, nullptr, 0, 3, info);
}
// ... the table of k in S segments: info[0..3]
extern "C" int swg_debug_prune_kmer_seg_read(swg_ctx *ctx, const swg_db *db, int k, int S, uint16_t *table_out, uint32_t *bound_out, size_t bound_cap,
                                             uint64_t *info)
{
    return debug_prune_read(ctx, db, "swg_debug_prune_kmer_seg_read", ctx && (k == 4 || k == 5) ? &ctx->kmer_first[k - 4] : nullptr, k, S, table_out, bound_out, nullptr,
                            bound_cap, nullptr, 0, 4, info);
}
// ... and the second level's table of S2 segments, the lists and the stages: info[0..6]
extern "C" int swg_debug_prune_refine_read(swg_ctx *ctx, const swg_db *db, int S2, uint16_t *table_out, uint32_t *bound_out, uint32_t *list_out, size_t pair_cap,
                                           uint32_t *stages_out, size_t stages_cap, uint64_t *info)
{
    return debug_prune_read(ctx, db, "swg_debug_prune_refine_read", ctx ? &ctx->kmer_refine[S2 == 256 ? 1 : 0] : nullptr, 4, S2, table_out, bound_out,
                            list_out, pair_cap, stages_out, stages_cap, 7, info);
}
// ... the third level and the widths: out[0..6] = S3 of the search last begun (0: no third level), third-level builds so
// far, then the entry bits of the tables that hold the current query and scoring (0: none): first level k = 4, k = 5,
// second level, third level; out[6] = what "prune_table_bits" left automatic gives at k = 4 (8 or 16)
extern "C" int swg_debug_prune_tables(swg_ctx *ctx, int64_t *out)
{
    if (!ctx || !out) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "swg_debug_prune_tables: NULL argument");
    const SwgKmerTable *t[4] = {&ctx->kmer_first[0], &ctx->kmer_first[1], &ctx->kmer_refine[0], &ctx->kmer_refine[1]};
    out[0] = ctx->prune_choice.refine[1];
    out[1] = (int64_t)ctx->kmer_refine_builds[1];
    for (int i = 0; i < 4; ++i) out[2 + i] = t[i]->d && t[i]->epoch == ctx->epoch ? t[i]->bits : 0;
    out[6] = 0;
    if (ctx->query_len() > 0) {
        ensure_prune_colmax(ctx);
        out[6] = swg_kmer_table_bits(ctx->prune_colmax, 4);
    }
    return SWG_OK;
}

// ... a level with a reserved table, the fourth or the fifth (its own table: the second entries): out[0..3] = the
// level's segments in the search last begun (0: without the level), builds of its table so far, the entry bits of the
// table if it holds the current query and scoring (0: not), whether its allocation was refused
static int debug_prune_level_tables(swg_ctx *ctx, int level, int64_t *out)
{
    if (!ctx || !out) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "swg_debug_prune_tables%d: NULL argument", level);
    const int i = level - 2;
    const SwgKmerTable &t = ctx->kmer_refine[i];
    out[0] = ctx->prune_choice.refine[i];
    out[1] = (int64_t)ctx->kmer_refine_builds[i];
    out[2] = t.d && t.epoch == ctx->epoch ? t.bits : 0;
    out[3] = ctx->kmer_refine_refused[i] ? 1 : 0;
    return SWG_OK;
}
extern "C" int swg_debug_prune_tables4(swg_ctx *ctx, int64_t *out) { return debug_prune_level_tables(ctx, 4, out); }
extern "C" int swg_debug_prune_tables5(swg_ctx *ctx, int64_t *out) { return debug_prune_level_tables(ctx, 5, out); }
// ... the gate in front of the first level: out[0] = whether the search last begun took it (swg_prune_gate_choice)
extern "C" int swg_debug_prune_gate(swg_ctx *ctx, int64_t *out)
{
    if (!ctx || !out) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "swg_debug_prune_gate: NULL argument");
    out[0] = ctx->prune_choice.gate;
    return SWG_OK;
}
// ... and n rows of the table of the fourth level, or of the fifth's second entries: out[i][0..256) = the entries of class
// block blocks[i] (< 22^5), an error unless the table holds the current query and scoring
static int debug_prune_level_rows(swg_ctx *ctx, int level, const uint32_t *blocks, size_t n, uint16_t *out)
{
    if (!ctx || (n > 0 && (!blocks || !out))) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "swg_debug_prune_refine%d_read: NULL argument", level);
    const SwgKmerTable &t = ctx->kmer_refine[level - 2];
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipDeviceSynchronize());
    if (!t.holds(ctx->epoch, 5, (int)SWG_KMER_REFINE4_SEGMENTS, 8))
        return swg_set_ctx_error(ctx, SWG_ERR_STATE, "no table of 5-residue blocks in 256 segments of this kind for the current query and scoring");
    uint8_t row[SWG_KMER_REFINE4_SEGMENTS];
    for (size_t i = 0; i < n; ++i) {
        if (blocks[i] >= swg_kmer_entries(5)) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "a table of 5-residue blocks: block %u", blocks[i]);
        HIP_TRY(ctx, hipMemcpy(row, t.d + (size_t)blocks[i] * SWG_KMER_REFINE4_SEGMENTS, sizeof row, hipMemcpyDeviceToHost));
        std::copy(row, row + SWG_KMER_REFINE4_SEGMENTS, out + i * SWG_KMER_REFINE4_SEGMENTS);
    }
    return SWG_OK;
}
extern "C" int swg_debug_prune_refine4_read(swg_ctx *ctx, const uint32_t *blocks, size_t n, uint16_t *out) { return debug_prune_level_rows(ctx, 4, blocks, n, out); }
extern "C" int swg_debug_prune_refine5_read(swg_ctx *ctx, const uint32_t *blocks, size_t n, uint16_t *out) { return debug_prune_level_rows(ctx, 5, blocks, n, out); }

extern "C" int swg_prune_last(const swg_ctx *ctx, swg_prune_info *out)
{
    if (!ctx || !out) return SWG_ERR_ARG;
    *out = ctx->prune_last;
    return SWG_OK;
}

// The body of swg_search_begin; allow_autotune: the first search of a query length may time geometries on the device.
static int search_begin_ticket(swg_ctx *ctx, swg_db *db, bool want_scores, size_t k, bool allow_autotune, int *ticket)
{
    return ctx_guarded(ctx, "swg_search_begin", [&]() -> int {
        fail_alloc_here(1);
        if (!ctx || !db || !ticket) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "swg_search_begin: NULL argument");
        int slot = -1;
        for (int i = 0; i < SWG_MAX_INFLIGHT; ++i) {
            const int c = (ctx->next_slot + i) % SWG_MAX_INFLIGHT;
            if (!ctx->slots[c].busy) {
                slot = c;
                break;
            }
        }
        if (slot < 0)
            return swg_set_ctx_error(ctx, SWG_ERR_STATE, "swg_search_begin: %d searches already in flight", SWG_MAX_INFLIGHT);
        const int rc = search_begin(ctx, db, want_scores, k, allow_autotune, &ctx->slots[slot]);
        if (rc != SWG_OK) return rc;
        ctx->slots[slot].busy = true;
        ctx->next_slot = (slot + 1) % SWG_MAX_INFLIGHT;
        *ticket = slot;
        return SWG_OK;
    });
}

// (the database handle is const in the ABI; a search keeps plans, hints and lazily built device images in it: the entry
// points cast once, everything below them takes swg_db *)
extern "C" int swg_search_begin(swg_ctx *ctx, const swg_db *db, int want_scores, size_t k, int *ticket)
{
    return search_begin_ticket(ctx, const_cast<swg_db *>(db), want_scores != 0, k, ctx && ctx->opt_autotune != 0, ticket);
}

extern "C" int swg_search_end(swg_ctx *ctx, int ticket, int32_t *scores_out, swg_hit *topk_out, size_t *n_hits,
                              swg_stats *stats)
{
    bool valid = false; // the ticket named a search in flight: it is spent whatever happens next (a failed read-out is not retried)
    const int rc = ctx_guarded(ctx, "swg_search_end", [&]() -> int {
        fail_alloc_here(2);
        if (!ctx || ticket < 0 || ticket >= SWG_MAX_INFLIGHT || !ctx->slots[ticket].busy)
            return swg_set_ctx_error(ctx, SWG_ERR_ARG, "swg_search_end: no search in flight under that ticket");
        valid = true;
        return search_end(ctx, &ctx->slots[ticket], scores_out, topk_out, n_hits, stats);
    });
    if (valid) ctx->slots[ticket].busy = false;
    return rc;
}

// The body of swg_search: one search from begin to end.
static int search_now(swg_ctx *ctx, swg_db *db, bool allow_autotune, int32_t *scores_out, swg_hit *topk_out, size_t k,
                      size_t *n_hits, swg_stats *stats)
{
    if (k > 0 && !topk_out) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "swg_search: k > 0 but topk_out NULL");
    int ticket = -1;
    const int rc = search_begin_ticket(ctx, db, scores_out != nullptr, k, allow_autotune, &ticket);
    if (rc != SWG_OK) return rc;
    return swg_search_end(ctx, ticket, scores_out, topk_out, n_hits, stats);
}

extern "C" int swg_search(swg_ctx *ctx, const swg_db *db, int32_t *scores_out, swg_hit *topk_out, size_t k,
                          size_t *n_hits, swg_stats *stats)
{
    return search_now(ctx, const_cast<swg_db *>(db), ctx && ctx->opt_autotune != 0, scores_out, topk_out, k, n_hits, stats);
}

// ---------------------------------------------------------------------------
// many queries against one resident database in one pass
// ---------------------------------------------------------------------------
// The reference runs one query per process (src/alignment_cmdline.c:381-396 reads a single query
// record); its report says the design "extends naturally" to many-to-many (Final Report p.7).  Here
// that is one launch per class for a whole batch of queries: row y of the grid works for query y (its
// own profile, its own pair queue, its own score array), so a database too small to fill the chip
// with one query -- where a search lasts as long as its longest pair's chain of rows -- fills it with
// many.  Queries that cannot take this path (several passes, scores that may saturate int16, gap
// scores outside the packed form, options that ask for another engine) are searched one after
// another with swg_search: same results, no batching.
namespace {
// The device buffers of one batch call, and the host vectors a chunk is staged from and read back into.
struct MultiBufs {
    int8_t *d_q = nullptr;
    uint32_t *d_qoff = nullptr;
    uint32_t *d_order = nullptr;
    uint8_t *d_prof[2] = {nullptr, nullptr};
    int32_t *d_scores = nullptr;
    uint32_t *d_cnt = nullptr;
    uint32_t *d_hist = nullptr, *d_meta = nullptr; // device top-K of the batch (no score array asked for)
    uint64_t *d_cand = nullptr;
    // How many rows each per-query buffer holds, written where the buffer is allocated and checked against what a
    // launch will index before every launch (multi_rows_ok): with two queries per lane the grid's row y stands for
    // queries 2y and 2y+1, so a batch of odd size indexes ONE ROW MORE than it has queries.  Round 3 sized these
    // buffers by the queries and a wavefront of the last pair ran off the end ("the fault of round 3").
    size_t rows_scores = 0, rows_order = 0, rows_prof[2] = {0, 0}, rows_cnt = 0, rows_topk = 0;
    std::vector<int32_t> h_scores;
    std::vector<uint32_t> qoff32, order, h_meta; // order: row r of the score buffer belongs to query order[r] of the chunk
    std::vector<uint64_t> h_cand;
    // swg_search_above_multi: per score row of a chunk its threshold, count and cursor (d_above_words: three arrays of
    // above_rows words) and its offset into the key pool (d_above_off), and the pool of the chunk's keys, which grows
    // with the answers (above_keys_cap keys: committed only once the allocation stands)
    uint32_t *d_above_words = nullptr;
    uint64_t *d_above_off = nullptr, *d_above_keys = nullptr;
    size_t above_rows = 0, above_keys_cap = 0;
    ~MultiBufs()
    {
        for (void *p : {(void *)d_hist, (void *)d_meta, (void *)d_cand, (void *)d_q, (void *)d_qoff, (void *)d_order, (void *)d_prof[0],
                        (void *)d_prof[1], (void *)d_scores, (void *)d_cnt, (void *)d_above_words, (void *)d_above_off, (void *)d_above_keys})
            (void)hipFree(p);
    }
};

// The queries of a batch: index bytes (one per position), or PSSM rows (32 bytes per position); the n + 1 offsets count
// positions either way.
struct MultiQueries {
    const int8_t *src;
    const uint64_t *off;
    size_t n;
    bool pssm;
    const char *fn; // the entry point, for messages
    size_t row_bytes() const { return pssm ? 32 : 1; } // bytes per query position
    size_t len(size_t i) const { return (size_t)(off[i + 1] - off[i]); }
    const int8_t *at(size_t i) const { return src + off[i] * row_bytes(); }
};
} // namespace

// Every per-query buffer of a batch launch against the rows the launch indexes: Qb queries on Qrows grid rows (query
// pairs when two queries share a lane: the kernels then address score rows 2y and 2y+1 for y < Qrows, i.e. Qb + 1
// rows for an odd batch).  What the buffers hold was written down where they were allocated; what the launch indexes
// comes from the plan, as the launch's own arguments do.  A mismatch is a bug of this file; it is reported, not launched.
static int multi_rows_ok(swg_ctx *ctx, const MultiBufs &B, const SwgBatchPlan &P, size_t Qb, size_t Qrows)
{
    const bool qq = P.qq;
    const size_t order_rows = qq ? P.score_rows(Qb) : 0; // entries of d_order the profile builder may read
    struct { const char *name; size_t have, need; } chk[] = {
        {"d_scores", B.rows_scores, P.score_rows(Qb)}, {"d_order", B.rows_order, order_rows},
        {"d_prof[0]", B.rows_prof[0], Qrows},          {"d_prof[1]", P.wk.n_classes == 2 ? B.rows_prof[1] : Qrows, Qrows},
        {"d_cnt", B.rows_cnt, Qrows},                  {"d_hist/d_meta/d_cand", P.dev_topk ? B.rows_topk : Qb, Qb},
    };
    if (Qrows != P.grid_rows(Qb))
        return swg_set_ctx_error(ctx, SWG_ERR_STATE, "swg_search_multi: %zu grid rows for %zu queries (qq %d)", Qrows, Qb, (int)qq);
    for (const auto &c : chk)
        if (c.have < c.need)
            return swg_set_ctx_error(ctx, SWG_ERR_STATE, "swg_search_multi: %s holds %zu rows, the launch indexes %zu (batch of %zu, qq %d)",
                                     c.name, c.have, c.need, Qb, (int)qq);
    return SWG_OK;
}

// The geometry of a batch launch: what plan_batch and plan_lists decide once the cells are known, and what the test
// hooks swg_debug_plan_batch / swg_debug_plan_lists answer without a device -- one spelling for the three of them.
// cols / group: options cols_per_wave and group_lanes.  A set one sends the batch one by one (false) unless option
// batch_geometry is 1: then the planner is asked for exactly that geometry with long split -1 (one class), as a forced
// single search asks it.  Whatever the planner answers, every class must take the longest query in one pass.
struct SwgBatchAsk {
    size_t lq_max;
    int n_cu;
    double copies;     // queries that share the launch (the planner's throughput terms grow with it)
    int form;          // 0 packed int16, 2 packed f16
    long cols, group, batch_geometry;
    long long_split;   // option long_split, for a geometry left free
    bool allow_split;  // a long class may run beside the bulk (not for candidate lists)
};
static bool batch_plan_work(const swg_db *db, const SwgBatchAsk &a, SwgDiagWork *wk)
{
    const bool forced = a.cols != 0 || a.group != 0;
    if (forced && a.batch_geometry == 0) return false;
    if (swg_plan_diag_work(db, a.lq_max, a.n_cu, a.cols, a.group, 0, forced ? -1 : a.long_split, a.allow_split, true, wk, a.copies, a.form, 1) <= 0)
        return false; // (batches: v_perm_b32 pairing)
    for (int c = 0; c < wk->n_classes; ++c)
        if (wk->plan[c].npass != 1 || (size_t)wk->plan[c].G * wk->plan[c].K < a.lq_max) return false;
    return true;
}
// Two queries per lane (swg_diag_qq_kernel) where the batch runs on the f16 cells, option "qq" allows it and the pairs'
// 4-byte profile fits LDS beside the other class's: then each class gets the W it is launched with, and *per_cu the bulk's
// workgroups per CU (LDS decides).
static bool batch_pairs_queries(SwgDiagWork *wk, int form, bool qq_on, int *per_cu)
{
    int qq_W = 0;
    if (form != 2 || !qq_on || !lds_bound_workgroup(*wk, INT_MAX, 0, &qq_W, per_cu)) return false;
    wk->plan[0].W = qq_W;
    if (wk->n_classes == 2) wk->plan[1].W = 4;
    return true;
}
// Profile bytes of one grid row of a class: (qq) 128 bytes per column per query PAIR, else 64 per query.
static size_t batch_prof_row_bytes(const SwgDiagPlan &pl, bool qq)
{
    return (size_t)pl.G * (qq ? (size_t)swg_q32_padded_cols(pl.K) * 128 : (size_t)swg_diag_padded_cols(pl.K) * 64);
}
// LDS bytes of one workgroup of a class, and the workgroups of it that a CU holds.
static size_t batch_class_lds_bytes(const SwgDiagPlan &pl, bool qq)
{
    return qq ? swg_diag32q_lds_bytes(pl.K, pl.G, pl.W) : swg_diag_dyn_lds_bytes(pl.K, pl.G, pl.W);
}
static int batch_class_per_cu(const SwgDiagPlan &pl, bool qq, int qq_per_cu, int c)
{
    return qq ? (c == 0 ? qq_per_cu : 1) : swg_workgroups_per_cu(swg_diag_variant_info(pl.variant).max_waves, pl.W, batch_class_lds_bytes(pl, false));
}
// The planner's model of a lists call's job table: its pairs' lengths (first, second sequence), longest first -- the
// planner reads lengths and nothing else.
static void lists_model_db(std::vector<std::pair<uint32_t, uint32_t>> *pairs, swg_db *M)
{
    const size_t np = pairs->size();
    std::sort(pairs->begin(), pairs->end(), std::greater<std::pair<uint32_t, uint32_t>>());
    M->n_local = 2 * np;
    M->n_bins = (uint32_t)((2 * np + SWG_BIN - 1) / SWG_BIN);
    M->lens.assign((size_t)M->n_bins * SWG_BIN, 0u);
    for (size_t p = 0; p < np; ++p) M->lens[2 * p] = (*pairs)[p].first, M->lens[2 * p + 1] = (*pairs)[p].second;
}
static void debug_plan_answer(const SwgDiagWork &wk, bool qq, int qq_per_cu, int32_t *out)
{
    const SwgDiagPlan &b = wk.plan[0];
    const int32_t v[8] = {1, b.K, b.G, b.W, batch_class_per_cu(b, qq, qq_per_cu, 0), qq ? 1 : 0, (int32_t)batch_class_lds_bytes(b, qq), wk.n_classes};
    memcpy(out, v, sizeof v);
}
// Test hooks (swg_host_internal.h): what plan_batch / plan_lists launch for a batch whose cells are `form`, no device.
extern "C" int swg_debug_plan_batch(const swg_db *db, size_t lq_max, size_t n_queries, int n_cu, int form, int qq_on, long cols, long group,
                                    long batch_geometry, int32_t *out)
{
    if (!db || !out || lq_max == 0 || n_cu <= 0 || (form != 0 && form != 2) || cols < 0 || group < 0) return SWG_ERR_ARG;
    memset(out, 0, 8 * sizeof(int32_t));
    if (n_queries < 2 || db->n_bins == 0) return SWG_OK; // (plan_batch: a batch of one is a single search)
    try {
        SwgDiagWork wk;
        const SwgBatchAsk ask = {lq_max, n_cu, (double)std::min<size_t>(256, n_queries), form, cols, group, batch_geometry, 0, true};
        if (!batch_plan_work(db, ask, &wk)) return SWG_OK;
        int per_cu = 1;
        const bool qq = batch_pairs_queries(&wk, form, qq_on != 0, &per_cu);
        debug_plan_answer(wk, qq, per_cu, out);
    } catch (const std::exception &) {
        return SWG_ERR_NOMEM;
    }
    return SWG_OK;
}
extern "C" int swg_debug_plan_lists(const uint32_t *pair_lens, size_t n_pairs, size_t lq_max, int n_cu, int form, long cols, long group,
                                    long batch_geometry, int32_t *out)
{
    if (!out || (n_pairs && !pair_lens) || lq_max == 0 || n_cu <= 0 || (form != 0 && form != 2) || cols < 0 || group < 0) return SWG_ERR_ARG;
    memset(out, 0, 8 * sizeof(int32_t));
    if (n_pairs == 0) return SWG_OK; // (nothing to launch)
    try {
        std::vector<std::pair<uint32_t, uint32_t>> pairs(n_pairs);
        for (size_t p = 0; p < n_pairs; ++p) pairs[p] = std::make_pair(pair_lens[2 * p], pair_lens[2 * p + 1]);
        swg_db M;
        lists_model_db(&pairs, &M);
        SwgDiagWork wk;
        const SwgBatchAsk ask = {lq_max, n_cu, 1.0, form, cols, group, batch_geometry, -1, false};
        if (!batch_plan_work(&M, ask, &wk) || wk.n_classes != 1) return SWG_OK;
        debug_plan_answer(wk, false, 1, out);
    } catch (const std::exception &) {
        return SWG_ERR_NOMEM;
    }
    return SWG_OK;
}

// What the call's arguments and the context's state rule out, and what the batch is worth whichever way it is searched:
// the real cells and the algorithmic bytes of all its queries.
static int validate_batch(swg_ctx *ctx, const swg_db *db, const MultiQueries &mq, const swg_hit *topk_out, size_t k, swg_stats *st)
{
    const char *fn = mq.fn;
    if (!ctx || !db || (mq.n && (!mq.src || !mq.off)))
        return swg_set_ctx_error(ctx, SWG_ERR_ARG, "%s: NULL argument", fn);
    if (k > 0 && !topk_out) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "%s: k > 0 but topk_out NULL", fn);
    if (!ctx->have_scoring) return swg_set_ctx_error(ctx, SWG_ERR_STATE, "%s: no scoring set", fn);
    if (db->device != ctx->device || !db->d_codes)
        return swg_set_ctx_error(ctx, SWG_ERR_STATE, "%s: database is not resident on device %d", fn, ctx->device);
    for (const SwgSlot &sl : ctx->slots)
        if (sl.busy) return swg_set_ctx_error(ctx, SWG_ERR_STATE, "%s: searches are in flight on this context", fn);
    for (size_t i = 0; i < mq.n; ++i) {
        if (mq.off[i + 1] <= mq.off[i])
            return swg_set_ctx_error(ctx, SWG_ERR_ARG, "%s: query %zu is empty or the offsets are not increasing", fn, i);
        const size_t lq = mq.len(i);
        if (lq > (1u << 24)) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "%s: query %zu too long", fn, i);
        for (size_t j = 0; j < lq && !mq.pssm; ++j) // (a PSSM takes any int8)
            if (mq.at(i)[j] < 1 || mq.at(i)[j] > 31)
                return swg_set_ctx_error(ctx, SWG_ERR_RESIDUE, "%s: residue index %d in query %zu outside 1..31", fn, mq.at(i)[j], i);
        st->cells += (uint64_t)lq * db->residues;
        st->bytes_alg += db->residues + 8ull * db->n_local + 32ull * lq + 1024ull;
    }
    return SWG_OK;
}

// Decides how the batch is searched.  One launch per class for a chunk of queries where every query takes one pass of a
// work-queue class, no score can reach the ceiling of the cells (the batch path has no re-score and no re-run), the gap
// scores fit the packed form and no option asks for another engine; otherwise one query after another.
static int plan_batch(swg_ctx *ctx, swg_db *db, const MultiQueries &mq, bool want_scores, size_t k, SwgBatchPlan *plan)
{
    *plan = SwgBatchPlan(); // (one after another, unless everything below allows the launch)
    SwgBatchPlan P;
    P.chunk_queries = 256;
    P.first_chunk = std::min(P.chunk_queries, mq.n);
    P.n_slots = (size_t)db->n_bins * SWG_BIN;
    P.go = ctx->gap_open + ctx->gap_extend;
    P.ge = ctx->gap_extend;
    for (size_t i = 0; i < mq.n; ++i) P.lq_max = std::max(P.lq_max, mq.len(i));
    // (options max_waves and workgroups: one by one; cols_per_wave and group_lanes: batch_plan_work decides)
    bool fast = ctx->gap_open <= 0 && ctx->gap_extend <= 0 && -P.go <= SWG_I16_CEILING && ctx->opt_force_bits != 32 &&
                ctx->opt_engine != 1 && ctx->opt_dynamic != 0 && db->n_bins > 0 && mq.n > 1 && ctx->opt_max_waves == 0 &&
                ctx->opt_workgroups == 0;
    // no score of any query may reach the int16 ceiling: each query's swg_score_bound, as a single search bounds it
    const uint64_t longest = (uint64_t)db->max_nblk * SWG_ROWS_PER_BLK;
    for (size_t i = 0; i < mq.n && fast; ++i) {
        const SwgScoreBound sb = mq.pssm ? swg_score_bound(mq.at(i), nullptr, mq.len(i), longest)
                                         : swg_score_bound(&ctx->sub[0][0], mq.at(i), mq.len(i), longest);
        P.bound_max = std::max(P.bound_max, sb.bound);
        if (sb.bound >= SWG_I16_CEILING) fast = false;
    }
    if (!fast) return SWG_OK;
    // the packed-f16 cells (8.5 instead of 10 instructions per column pair) where no query of the batch can reach
    // their ceiling
    P.form = ctx->opt_f16 != 0 && P.bound_max < SWG_F16_CEILING && swg_f16_gaps_ok(P.go, P.ge) ? 2 : 0;
    int rc = ensure_pair_tokens(ctx, db);
    if (rc != SWG_OK) return rc;
    SwgDiagWork &wk = P.wk;
    const SwgBatchAsk ask = {P.lq_max, ctx->n_cu, (double)P.first_chunk, P.form, ctx->opt_cols, ctx->opt_group, ctx->opt_batch_geometry,
                             ctx->opt_long_split, true};
    fast = db->ptok.ok && batch_plan_work(db, ask, &wk);
    for (int c = 0; fast && c < wk.n_classes; ++c) fast = diag_class_is_dynamic(ctx, db, wk.plan[c]);
    // A database of short sequences is faster on the systolic engine, one query after another, than as a batch on
    // the lane groups: 16 queries against 500 000 peptides 3 720 GCUPS as a batch, ~7 000 one by one.  Same
    // comparison as a single search makes, per query.
    int sys_K = 0;
    if (!fast || systolic_beats_lane_groups(ctx, db, P.lq_max, wk.plan[0], P.form, P.bound_max, P.first_chunk, &sys_K)) return SWG_OK;
    // Two queries per lane (swg_diag_qq_kernel, 7.5 instead of 8.5 instructions per column pair: the two halves of a
    // register hold two QUERIES against one sequence, so no v_perm pairs two sequences' profile words) where the batch
    // runs on the f16 cells and the pairs' 4-byte profile fits LDS beside the other class's; option "qq" = 0 turns it off.
    // The pairs' profile is twice the size, so LDS decides the occupancy (as for the int32 kernel, but up to every
    // wavefront the instantiation allows): four 57 KB workgroups of four do not fit a CU, two of eight do -- the first
    // version of this path ran at two wavefronts per SIMD and lost to the perm.  No room beside the long class: two
    // sequences per lane, as without the option.
    P.qq = batch_pairs_queries(&wk, P.form, ctx->opt_qq != 0, &P.qq_per_cu);
    // Top-K only (no score array asked for): selected on the device for the whole batch in three launches, and a few
    // hundred keys per query come back instead of every score (round 3: with 32 queries against 100 000 sequences the
    // copy and the host's selection took longer than the fill: 82 ms of wall time for 49 ms of device time).
    P.dev_topk = !want_scores && k > 0 && k <= SWG_TOPK_MULTI_CAP / 2;
    // The buffers: rows are counted in QUERIES for scores / order / top-K, in grid rows (query pairs with qq) for the
    // profiles and the queues.
    P.score_rows_cap = P.score_rows(P.first_chunk);
    P.grid_rows_cap = P.grid_rows(P.first_chunk);
    P.order_entries = P.chunk_queries + 1;
    P.class_queue_dwords = SWG_DYN_SHARDS * SWG_DYN_SHARD_STRIDE;
    P.rank_word_base = P.chunk_queries * 2 * P.class_queue_dwords; // (the queues serve a full chunk's grid rows)
    P.queue_dwords = P.rank_word_base + 2 * SWG_DYN_SIMD_SLOTS;
    for (int c = 0; c < wk.n_classes; ++c) // (qq: an odd batch's last pair is a whole pair)
        P.prof_row_bytes[c] = batch_prof_row_bytes(wk.plan[c], P.qq);
    P.one_launch = true;
    *plan = P;
    return SWG_OK;
}

// One query after another with swg_search's own body; the context's own query is put back afterwards (a PSSM as a
// PSSM), whether or not a query failed.  Statistics: the times, the re-scored sequences and the padded cells add up,
// the geometry is the last search's; what a single search reports beyond that (lane groups, the long class, launches)
// stays zero, as this route has always reported it.
namespace {
struct KeptQuery { // the context's own query across a batch searched one by one
    bool pssm;
    std::vector<int8_t> bytes;
    swg_ctx *owner; // (a batch's searches are never pruned: in_batch for as long as this object lives -- unless each of them is
                    // a search of its own right, batch_member false: swg_search_above_multi's queries, cut at their own scores)
    explicit KeptQuery(swg_ctx *ctx, bool batch_member = true) : pssm(ctx->query_pssm), bytes(ctx->query_pssm ? ctx->pssm : ctx->query), owner(ctx)
    {
        ctx->in_batch = batch_member;
    }
    ~KeptQuery() { owner->in_batch = false; }
    KeptQuery(const KeptQuery &) = delete;
    KeptQuery &operator=(const KeptQuery &) = delete;
    int restore(swg_ctx *ctx, int rc) const
    {
        if (!bytes.empty()) {
            const int rq = pssm ? swg_set_query_pssm(ctx, bytes.data(), bytes.size() / 32) : swg_set_query(ctx, bytes.data(), bytes.size());
            if (rc == SWG_OK) rc = rq;
        } else {
            ctx->query.clear();
        }
        return rc;
    }
};
} // namespace
static void add_one_search(swg_stats *st, const swg_stats &one)
{
    st->fill_ms += one.fill_ms;
    st->rescore_ms += one.rescore_ms;
    st->topk_ms += one.topk_ms;
    st->total_ms += one.total_ms;
    st->n_rescored += one.n_rescored;
    st->cells_padded += one.cells_padded;
    st->path_bits = one.path_bits;
    st->cell_form = one.cell_form;
    st->engine = one.engine;
    st->cols_per_wave = one.cols_per_wave;
    st->group_lanes = one.group_lanes;
    st->waves = one.waves;
    st->passes = one.passes;
    st->workgroups = one.workgroups;
    st->work_queue = one.work_queue;
}

static int search_batch_one_by_one(swg_ctx *ctx, swg_db *db, const MultiQueries &mq, int32_t *scores_out, swg_hit *topk_out, size_t k,
                                   size_t *n_hits, swg_stats *st)
{
    const KeptQuery keep(ctx);
    int rc = SWG_OK;
    for (size_t i = 0; i < mq.n && rc == SWG_OK; ++i) {
        swg_stats one;
        rc = mq.pssm ? swg_set_query_pssm(ctx, mq.at(i), mq.len(i)) : swg_set_query(ctx, mq.at(i), mq.len(i));
        if (rc == SWG_OK)
            rc = search_now(ctx, db, ctx->opt_autotune != 0, scores_out ? scores_out + i * db->n_total : nullptr,
                            topk_out ? topk_out + i * k : nullptr, k, n_hits ? n_hits + i : nullptr, &one);
        if (rc != SWG_OK) break;
        add_one_search(st, one);
    }
    return keep.restore(ctx, rc);
}

// ---- one launch per class for up to chunk_queries queries: the stages -----------------------------
// Every device buffer of the call, by the plan's sizes, each with the rows it holds written beside it (multi_rows_ok).
static int batch_allocate(swg_ctx *ctx, const SwgBatchPlan &P, MultiBufs *B)
{
    HIP_TRY(ctx, hipMalloc(&B->d_cnt, P.queue_dwords * 4));
    B->rows_cnt = P.chunk_queries;
    HIP_TRY(ctx, hipMalloc(&B->d_scores, P.score_rows_cap * P.n_slots * 4));
    B->rows_scores = P.score_rows_cap;
    HIP_TRY(ctx, hipMalloc(&B->d_qoff, P.order_entries * 4));
    HIP_TRY(ctx, hipMalloc(&B->d_order, P.order_entries * 4));
    B->rows_order = P.order_entries;
    if (P.dev_topk) {
        HIP_TRY(ctx, hipMalloc(&B->d_hist, P.first_chunk * 4096 * 4));
        HIP_TRY(ctx, hipMalloc(&B->d_meta, P.first_chunk * 16));
        HIP_TRY(ctx, hipMalloc(&B->d_cand, P.first_chunk * (size_t)SWG_TOPK_MULTI_CAP * 8));
        B->rows_topk = P.first_chunk;
    }
    for (int c = 0; c < P.wk.n_classes; ++c) {
        HIP_TRY(ctx, hipMalloc(&B->d_prof[c], P.grid_rows_cap * P.prof_row_bytes[c]));
        B->rows_prof[c] = P.grid_rows_cap;
    }
    return SWG_OK;
}

// The queries [q0, q0 + Qb) to the device -- their bytes, their offsets, (qq) the order that pairs them --, scores and
// queues zeroed, and every class's profiles built.
static int batch_stage_chunk(swg_ctx *ctx, const SwgBatchPlan &P, const MultiQueries &mq, size_t q0, size_t Qb, MultiBufs *B)
{
    hipStream_t s = ctx->stream;
    std::vector<uint32_t> &qoff32 = B->qoff32, &order = B->order;
    qoff32.resize(Qb + 1); // (a failed host allocation is reported by the entry point's guard)
    if (P.dev_topk) {
        B->h_meta.resize(Qb * 4);
        B->h_cand.resize(Qb * (size_t)SWG_TOPK_MULTI_CAP);
    } else {
        B->h_scores.resize(Qb * P.n_slots);
    }
    for (size_t i = 0; i <= Qb; ++i) qoff32[i] = (uint32_t)(mq.off[q0 + i] - mq.off[q0]);
    // qq: queries of similar length share a lane
    order.resize(Qb);
    for (size_t i = 0; i < Qb; ++i) order[i] = (uint32_t)i;
    if (P.qq)
        std::stable_sort(order.begin(), order.end(),
                         [&](uint32_t a, uint32_t b) { return qoff32[a + 1] - qoff32[a] > qoff32[b + 1] - qoff32[b]; });
    const uint64_t qbytes = (mq.off[q0 + Qb] - mq.off[q0]) * mq.row_bytes();
    (void)hipFree(B->d_q);
    B->d_q = nullptr;
    HIP_TRY(ctx, hipMalloc(&B->d_q, std::max<uint64_t>(4, qbytes)));
    HIP_TRY(ctx, hipMemcpyAsync(B->d_q, mq.at(q0), qbytes, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(B->d_qoff, qoff32.data(), (Qb + 1) * 4, hipMemcpyHostToDevice, s));
    order.push_back(order.back()); // (qq, odd batch: the last pair's absent partner is its query once more)
    HIP_TRY(ctx, hipMemcpyAsync(B->d_order, order.data(), (Qb + 1) * 4, hipMemcpyHostToDevice, s));
    order.pop_back();
    HIP_TRY(ctx, hipMemsetAsync(B->d_scores, 0, P.score_rows(Qb) * P.n_slots * 4, s));
    HIP_TRY(ctx, hipMemsetAsync(B->d_cnt, 0, P.queue_dwords * 4, s));
    const int8_t *d_idx = mq.pssm ? nullptr : B->d_q, *d_pssms = mq.pssm ? B->d_q : nullptr; // (the builders' two sources)
    for (int c = 0; c < P.wk.n_classes; ++c) {
        const SwgDiagPlan &pl = P.wk.plan[c];
        if (P.qq)
            HIP_TRY(ctx, swg_launch_build_profiles_qq(ctx->d_sub, d_idx, B->d_qoff, B->d_order, (uint32_t)Qb,
                                                      (uint32_t)(pl.G * swg_q32_padded_cols(pl.K)), pl.K, swg_q32_padded_cols(pl.K),
                                                      B->d_prof[c], s, SWG_LDS_SWIZZLE ? pl.G : 0, d_pssms));
        else
            HIP_TRY(ctx, swg_launch_build_profiles_multi(ctx->d_sub, d_idx, B->d_qoff, (uint32_t)Qb,
                                                         (uint32_t)(pl.G * swg_diag_padded_cols(pl.K)), pl.K,
                                                         swg_diag_padded_cols(pl.K), B->d_prof[c], s, SWG_LDS_SWIZZLE ? pl.G : 0, P.form == 2,
                                                         d_pssms));
    }
    return SWG_OK;
}

// Workgroups per grid row of each class for a chunk of Qrows grid rows -- the chip's resident workgroups shared out
// over the chunk -- and the bulk's lane groups over the whole grid.
static void batch_chunk_workgroups(const SwgBatchPlan &P, size_t Qrows, int n_cu, int wgs[2], uint64_t *groups0)
{
    const SwgDiagWork &wk = P.wk;
    wgs[0] = wgs[1] = 1;
    *groups0 = 1;
    for (int c = 0; c < wk.n_classes; ++c) {
        const SwgDiagPlan &pl = wk.plan[c];
        const int per_cu = batch_class_per_cu(pl, P.qq, P.qq_per_cu, c);
        int total = n_cu * per_cu;
        if (wk.n_classes == 2 && !P.qq) total = c == 1 ? n_cu : std::max(n_cu, total - n_cu); // one wavefront per SIMD for the long class
        const uint64_t items = (wk.pair_end[c] - wk.pair_begin[c]) * (P.qq ? 2u : 1u); // pairs, or (qq) single sequences
        const uint64_t per_wg = (uint64_t)pl.W * (64 / pl.G);
        wgs[c] = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)total / Qrows, (items + per_wg - 1) / per_wg));
        if (c == 0) *groups0 = (uint64_t)wgs[0] * Qrows * per_wg;
    }
}

// The fill of one chunk: a launch per class, the grid's row y working for query (qq: query pair) y.  Events: ev[1]
// before, ev[2] after on the main stream.
static int batch_launch_chunk(swg_ctx *ctx, const swg_db *db, const SwgBatchPlan &P, const MultiBufs &B, size_t Qb, size_t Qrows)
{
    hipStream_t s = ctx->stream;
    const SwgDiagWork &wk = P.wk;
    const SwgPairTokens &T = db->ptok;
    const size_t n_slots = P.n_slots;
    int wgs[2];
    uint64_t groups0;
    batch_chunk_workgroups(P, Qrows, ctx->n_cu, wgs, &groups0);
    const uint64_t bulk_blocks = (uint64_t)(T.pair_blocks_prefix[wk.pair_end[0]] - T.pair_blocks_prefix[wk.pair_begin[0]]);
    HIP_TRY(ctx, hipEventRecord(ctx->cur->ev[1], s));
    int rf = fork_long_class(ctx, wk);
    if (rf != SWG_OK) return rf;
    for (int c = wk.n_classes - 1; c >= 0; --c) {
        const SwgDiagPlan &pl = wk.plan[c];
        uint32_t *simd_ranks = B.d_cnt + P.rank_word_base + (size_t)c * SWG_DYN_SIMD_SLOTS;
        hipStream_t qs = c == 1 ? ctx->stream2 : s;
        auto per_row = [&](auto *q) { // grid row y: its own queue, profile and score rows
            q->queue = B.d_cnt + (size_t)c * P.class_queue_dwords;
            q->queue_stride = 2 * P.class_queue_dwords;
            q->profile = B.d_prof[c];
            q->profile_stride = P.prof_row_bytes[c];
            q->score_stride = n_slots;
        };
        if (P.qq) {
            SwgDiagQQParams q = token_params<SwgDiagQQParams>(T, pl.G, wk.n_classes, simd_ranks);
            per_row(&q);
            q.q_begin = (uint32_t)std::min<uint64_t>(2 * wk.pair_begin[c], n_slots);
            q.q_end = (uint32_t)std::min<uint64_t>(2 * wk.pair_end[c], n_slots);
            q.scores = B.d_scores;
            q.n_queries = (uint32_t)Qb;
            q.seq_limit = (uint32_t)n_slots;
            q.go = f16x2_of(-P.go);
            q.ge = f16x2_of(-P.ge);
            q.prio_blocks = c == 0 ? bulk_prio_blocks(ctx, 2ull * bulk_blocks * Qrows, groups0) : 0u;
            HIP_TRY(ctx, swg_launch_diag_qq(pl.variant, pl.W, wgs[c], (int)Qrows, q, qs));
            continue;
        }
        SwgDiagDynParams q = dyn_params_base(T, B.d_scores, n_slots, pl.G, P.form, P.go, P.ge, wk.n_classes, simd_ranks);
        per_row(&q);
        q.q_begin = (uint32_t)wk.pair_begin[c];
        q.q_end = (uint32_t)wk.pair_end[c];
        if (c == 0) q.prio_blocks = bulk_prio_blocks(ctx, bulk_blocks * Qb, groups0);
        dyn_batch_zones(ctx, T, &q, (uint64_t)wgs[c] * pl.W * (64 / pl.G), pl.K, pl.G, P.form);
        HIP_TRY(ctx, swg_launch_diag_dyn(pl.variant, false, P.form, pl.W, wgs[c], q, qs, (int)Qb));
    }
    rf = join_long_class(ctx, wk, false); // (a batch does not time its classes)
    if (rf != SWG_OK) return rf;
    HIP_TRY(ctx, hipEventRecord(ctx->cur->ev[2], s));
    return SWG_OK;
}

// What a chunk's fill left, to the caller: (device top-K) the few keys per query, or every score, after which the host
// selects.  Adds the chunk's times to *st.
static int batch_deliver_chunk(swg_ctx *ctx, const swg_db *db, const SwgBatchPlan &P, MultiBufs *B, size_t q0, size_t Qb, size_t k,
                               int32_t *scores_out, swg_hit *topk_out, size_t *n_hits, swg_stats *st)
{
    hipStream_t s = ctx->stream;
    const size_t n_slots = P.n_slots, n_total = db->n_total;
    std::vector<int32_t> &h_scores = B->h_scores;
    const std::vector<uint32_t> &h_meta = B->h_meta;
    if (P.dev_topk) {
        HIP_TRY(ctx, swg_launch_topk_multi(B->d_scores, n_slots, db->d_order, (uint32_t)n_slots, (uint32_t)Qb, (uint32_t)k, B->d_hist,
                                           B->d_meta, B->d_cand, SWG_TOPK_MULTI_CAP, s));
        HIP_TRY(ctx, hipMemcpyAsync(B->h_meta.data(), B->d_meta, Qb * 16, hipMemcpyDeviceToHost, s));
        HIP_TRY(ctx, hipMemcpyAsync(B->h_cand.data(), B->d_cand, Qb * (size_t)SWG_TOPK_MULTI_CAP * 8, hipMemcpyDeviceToHost, s));
    } else {
        HIP_TRY(ctx, hipMemcpyAsync(h_scores.data(), B->d_scores, Qb * n_slots * 4, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(ctx, spin_sync(ctx, s));
    float ms = 0.f;
    HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->cur->ev[1], ctx->cur->ev[2]));
    st->fill_ms += ms;
    st->total_ms += ms;
    const auto t0 = std::chrono::steady_clock::now();
    for (size_t r = 0; r < Qb; ++r) { // (row r of the score buffer = query order[r] of this chunk)
        const size_t i = q0 + B->order[r];
        if (P.dev_topk && h_meta[4 * r + 1] == 0 && h_meta[4 * r + 2] <= SWG_TOPK_MULTI_CAP) {
            // every hit with a score >= the k-th best one: sort those few keys
            uint64_t *c = B->h_cand.data() + r * (size_t)SWG_TOPK_MULTI_CAP;
            const size_t nc = h_meta[4 * r + 2], m = std::min(k, nc);
            std::partial_sort(c, c + m, c + nc, std::greater<uint64_t>());
            for (size_t j = 0; j < m; ++j) swg_key_hit(c[j], &topk_out[i * k + j]);
            if (n_hits) n_hits[i] = m;
            continue;
        }
        if (P.dev_topk) { // threshold beyond the histogram, or too many ties: this query's scores to the host after all
            if (h_scores.size() < n_slots) h_scores.resize(n_slots);
            HIP_TRY(ctx, hipMemcpyAsync(h_scores.data(), B->d_scores + r * n_slots, n_slots * 4, hipMemcpyDeviceToHost, s));
            HIP_TRY(ctx, spin_sync(ctx, s));
            deliver_scores(db, h_scores.data(), n_slots, nullptr, topk_out + i * k, k, n_hits ? n_hits + i : nullptr);
            continue;
        }
        deliver_scores(db, h_scores.data() + r * n_slots, n_slots, scores_out ? scores_out + i * n_total : nullptr,
                       topk_out ? topk_out + i * k : nullptr, k, n_hits ? n_hits + i : nullptr);
    }
    st->topk_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return SWG_OK;
}

// The statistics of a batch that went through the launches, from its plan (workgroups and lane groups: the last chunk's).
static void batch_report(const swg_ctx *ctx, const swg_db *db, const SwgBatchPlan &P, size_t n_queries, swg_stats *st)
{
    const SwgDiagWork &wk = P.wk;
    const size_t last_rows = P.grid_rows(n_queries - (n_queries - 1) / P.chunk_queries * P.chunk_queries);
    int wgs[2];
    uint64_t groups0;
    batch_chunk_workgroups(P, last_rows, ctx->n_cu, wgs, &groups0);
    st->workgroups = wgs[0] * (int)last_rows;
    st->streams = (int32_t)groups0;
    st->path_bits = 16;
    st->engine = 2;
    st->work_queue = 1;
    st->classes_overlapped = -1; // (not measured for a batch)
    st->cell_form = P.qq ? 3 : P.form;
    st->cols_per_wave = wk.plan[0].K;
    st->group_lanes = wk.plan[0].G;
    st->waves = wk.plan[0].W;
    st->passes = 1;
    st->fill_launches = 1;
    if (wk.n_classes == 2) {
        st->long_pairs = (int32_t)(wk.pair_end[1] - wk.pair_begin[1]);
        st->long_cols_per_lane = wk.plan[1].K;
    }
    for (int c = 0; c < wk.n_classes; ++c)
        st->cells_padded += 2ull * wk.plan[c].G * wk.plan[c].K * diag_class_blocks(ctx, db, wk, c) * 4ull * n_queries;
}

static int search_multi_impl(swg_ctx *ctx, swg_db *db, const MultiQueries &mq, int32_t *scores_out, swg_hit *topk_out, size_t k,
                             size_t *n_hits, swg_stats *stats)
{
    swg_stats st;
    memset(&st, 0, sizeof st);
    int rc = validate_batch(ctx, db, mq, topk_out, k, &st);
    if (rc != SWG_OK) return rc;
    ctx->prune_last = swg_prune_info(); // (swg_prune_last: a batch call ends with nothing pruned)
    if (stats) *stats = st;
    if (mq.n == 0) return SWG_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    SwgBatchPlan P;
    rc = plan_batch(ctx, db, mq, scores_out != nullptr, k, &P);
    if (rc != SWG_OK) return rc;
    if (!P.one_launch) {
        rc = search_batch_one_by_one(ctx, db, mq, scores_out, topk_out, k, n_hits, &st);
        if (stats) *stats = st;
        return rc;
    }
    MultiBufs B;
    ctx->cur = &ctx->slots[0];
    rc = batch_allocate(ctx, P, &B);
    for (size_t q0 = 0; q0 < mq.n && rc == SWG_OK; q0 += P.chunk_queries) {
        const size_t Qb = std::min(P.chunk_queries, mq.n - q0);
        const size_t Qrows = P.grid_rows(Qb); // rows of the grid: query pairs, or queries
        // the fence: what this chunk's launches will index, against what the buffers hold
        rc = multi_rows_ok(ctx, B, P, Qb, Qrows);
        if (rc == SWG_OK) rc = batch_stage_chunk(ctx, P, mq, q0, Qb, &B);
        if (rc == SWG_OK) rc = batch_launch_chunk(ctx, db, P, B, Qb, Qrows);
        if (rc == SWG_OK) rc = batch_deliver_chunk(ctx, db, P, &B, q0, Qb, k, scores_out, topk_out, n_hits, &st);
    }
    if (rc != SWG_OK) return rc;
    batch_report(ctx, db, P, mq.n, &st);
    if (stats) *stats = st;
    return SWG_OK;
}

extern "C" int swg_search_multi(swg_ctx *ctx, const swg_db *db, const int8_t *queries, const uint64_t *q_offsets,
                                size_t n_queries, int32_t *scores_out, swg_hit *topk_out, size_t k, size_t *n_hits,
                                swg_stats *stats)
{
    return ctx_guarded(ctx, "swg_search_multi", [&]() -> int { // (the body sizes host vectors by the batch)
        return search_multi_impl(ctx, const_cast<swg_db *>(db), MultiQueries{queries, q_offsets, n_queries, false, "swg_search_multi"},
                                 scores_out, topk_out, k, n_hits, stats);
    });
}

extern "C" int swg_search_multi_pssm(swg_ctx *ctx, const swg_db *db, const int8_t *pssms, const uint64_t *q_offsets,
                                     size_t n_queries, int32_t *scores_out, swg_hit *topk_out, size_t k, size_t *n_hits,
                                     swg_stats *stats)
{
    return ctx_guarded(ctx, "swg_search_multi_pssm", [&]() -> int {
        return search_multi_impl(ctx, const_cast<swg_db *>(db), MultiQueries{pssms, q_offsets, n_queries, true, "swg_search_multi_pssm"},
                                 scores_out, topk_out, k, n_hits, stats);
    });
}

// ---------------------------------------------------------------------------
// the gapless prefilter score
// ---------------------------------------------------------------------------
// swg_search_gapless is swg_search with another recurrence, H[i][j] = max(0, H[i-1][j-1] + S(q_i, d_j)): the context's
// query, the database, the outputs and the whole stream of one search (fill, re-run of what the f16 cells flagged, int32
// level, top-K, read-out) are the gapped search's.  What differs is decided in plan_search under ctx->gapless: the cells of
// the fill (route 1: CellsGapless on the work queue) and the gap magnitudes of every level that has gap operands (priced
// out; the context's own are not read).  The batch calls are the loop "set query i, search" over that path.
namespace {
struct GaplessMode { // ctx->gapless for the duration of a call
    swg_ctx *ctx;
    explicit GaplessMode(swg_ctx *c) : ctx(c) { ctx->gapless = true; }
    ~GaplessMode() { ctx->gapless = false; }
};
} // namespace

extern "C" int swg_search_gapless(swg_ctx *ctx, const swg_db *db, int32_t *scores_out, swg_hit *topk_out, size_t k, size_t *n_hits,
                                  swg_stats *stats)
{
    if (!ctx || !db) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "swg_search_gapless: NULL argument");
    for (const SwgSlot &sl : ctx->slots)
        if (sl.busy) return swg_set_ctx_error(ctx, SWG_ERR_STATE, "swg_search_gapless: searches are in flight on this context");
    const GaplessMode mode(ctx);
    return search_now(ctx, const_cast<swg_db *>(db), ctx->opt_autotune != 0, scores_out, topk_out, k, n_hits, stats);
}

// swg_search_above / swg_search_gapless_above: one search whose read-out is every sequence at or above the caller's
// score (enqueue_readout, deliver_above), and whose 16-bit fill, where swg_prune_plan admits it, is cut at that score
// from its first launch on (plan_prune, launch_diag).  ctx->above_min says so for the duration of the call.
namespace {
struct AboveMode {
    swg_ctx *ctx;
    AboveMode(swg_ctx *c, int32_t min_score) : ctx(c) { ctx->above_min = min_score; }
    ~AboveMode() { ctx->above_min = 0; }
};
} // namespace

static int search_above_impl(swg_ctx *ctx, const swg_db *db, bool gapless, const char *what, int32_t min_score, swg_hit *hits_out, size_t cap,
                             size_t *n_hits, uint64_t *n_total, swg_stats *stats)
{
    if (n_hits) *n_hits = 0;
    if (n_total) *n_total = 0;
    if (!ctx || !db) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "%s: NULL argument", what);
    if (min_score < 1) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "%s: min_score must be at least 1 (every sequence scores at least 0)", what);
    if (cap > 0 && !hits_out) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "%s: cap > 0 but hits_out NULL", what);
    for (const SwgSlot &sl : ctx->slots)
        if (sl.busy) return swg_set_ctx_error(ctx, SWG_ERR_STATE, "%s: searches are in flight on this context", what);
    const AboveMode mode(ctx, min_score);
    ctx->gapless = gapless;
    struct Restore {
        swg_ctx *c;
        ~Restore() { c->gapless = false; }
    } restore{ctx};
    int ticket = -1;
    int rc = search_begin_ticket(ctx, const_cast<swg_db *>(db), false, 0, ctx->opt_autotune != 0, &ticket);
    if (rc != SWG_OK) return rc;
    SwgAboveOut out;
    out.hits_out = hits_out, out.cap = cap;
    rc = ctx_guarded(ctx, what, [&]() -> int { return search_end(ctx, &ctx->slots[ticket], nullptr, nullptr, n_hits, stats, &out); });
    ctx->slots[ticket].busy = false;
    if (rc == SWG_OK && n_total) *n_total = out.n_total;
    return rc;
}

extern "C" int swg_search_above(swg_ctx *ctx, const swg_db *db, int32_t min_score, swg_hit *hits_out, size_t cap, size_t *n_hits, uint64_t *n_total,
                                swg_stats *stats)
{
    return search_above_impl(ctx, db, false, "swg_search_above", min_score, hits_out, cap, n_hits, n_total, stats);
}

extern "C" int swg_search_gapless_above(swg_ctx *ctx, const swg_db *db, int32_t min_score, swg_hit *hits_out, size_t cap, size_t *n_hits,
                                        uint64_t *n_total, swg_stats *stats)
{
    return search_above_impl(ctx, db, true, "swg_search_gapless_above", min_score, hits_out, cap, n_hits, n_total, stats);
}

static int search_gapless_multi_impl(swg_ctx *ctx, swg_db *db, const MultiQueries &mq, int32_t *scores_out, swg_hit *topk_out, size_t k,
                                     size_t *n_hits, swg_stats *stats)
{
    swg_stats st;
    memset(&st, 0, sizeof st);
    int rc = validate_batch(ctx, db, mq, topk_out, k, &st);
    if (rc != SWG_OK) return rc;
    if (stats) *stats = st;
    if (mq.n == 0) return SWG_OK;
    const GaplessMode mode(ctx);
    rc = search_batch_one_by_one(ctx, db, mq, scores_out, topk_out, k, n_hits, &st);
    if (stats) *stats = st;
    return rc;
}

extern "C" int swg_search_gapless_multi(swg_ctx *ctx, const swg_db *db, const int8_t *queries, const uint64_t *q_offsets, size_t n_queries,
                                        int32_t *scores_out, swg_hit *topk_out, size_t k, size_t *n_hits, swg_stats *stats)
{
    return ctx_guarded(ctx, "swg_search_gapless_multi", [&]() -> int {
        return search_gapless_multi_impl(ctx, const_cast<swg_db *>(db), MultiQueries{queries, q_offsets, n_queries, false, "swg_search_gapless_multi"},
                                         scores_out, topk_out, k, n_hits, stats);
    });
}

extern "C" int swg_search_gapless_multi_pssm(swg_ctx *ctx, const swg_db *db, const int8_t *pssms, const uint64_t *q_offsets, size_t n_queries,
                                             int32_t *scores_out, swg_hit *topk_out, size_t k, size_t *n_hits, swg_stats *stats)
{
    return ctx_guarded(ctx, "swg_search_gapless_multi_pssm", [&]() -> int {
        return search_gapless_multi_impl(ctx, const_cast<swg_db *>(db), MultiQueries{pssms, q_offsets, n_queries, true, "swg_search_gapless_multi_pssm"},
                                         scores_out, topk_out, k, n_hits, stats);
    });
}

// ---------------------------------------------------------------------------
// every hit at or above a score, per query of a batch
// ---------------------------------------------------------------------------
// swg_search_above_multi*: row i is what swg_set_query(query i) + swg_search_above(min_scores[i]) gives.  Two routes
// (swg_above_multi_route decides; DESIGN 4.2.1, "A caller's threshold, per query of a batch"):
//   1  the batch launch of swg_search_multi as it stands (plan_batch admits it, batch_stage_chunk and batch_launch_chunk
//      fill it, unpruned), and a read-out of its own: every score row of a chunk is compacted on the device against its
//      own threshold, and only counts and keys come back;
//   2  one query after another, each a plain swg_search_above -- NOT a batch member (ctx->in_batch stays false), so its
//      fill is cut at its own min_scores[i] wherever swg_prune_plan admits a caller's threshold.
// The gapless forms always take route 2 (the batch kernels have no gapless cells).
extern "C" int swg_debug_above_multi_route(long option, int admitted, int single_pruned)
{
    if (option < 0 || option > 2) return SWG_ERR_ARG;
    return swg_above_multi_route(option, admitted != 0, single_pruned != 0);
}

namespace {
struct AboveMultiOut { // the caller's arrays: rows of cap hits, and per query what was written and what there is
    const int32_t *min_scores;
    swg_hit *hits_out;
    size_t cap;
    size_t *n_hits;
    uint64_t *n_total;
};
} // namespace

// Whether swg_search_above of the batch's longest query would be pruned on this database under the context's options:
// plan_search and plan_prune asked with that query as the context's host copy (no device copy, no tuner's trials, nothing
// queued), and everything put back.
static bool above_multi_single_pruned(swg_ctx *ctx, swg_db *db, const MultiQueries &mq, const int32_t *min_scores)
{
    if (ctx->opt_prune == 0 || db->n_bins == 0) return false;
    size_t L = 0;
    for (size_t i = 1; i < mq.n; ++i)
        if (mq.len(i) > mq.len(L)) L = i;
    std::vector<int8_t> kept_query, kept_pssm;
    kept_query.swap(ctx->query);
    kept_pssm.swap(ctx->pssm);
    const bool kept_is_pssm = ctx->query_pssm;
    const SwgPruneChoice kept_choice = ctx->prune_choice;
    const std::string kept_err = ctx->err;
    (mq.pssm ? ctx->pssm : ctx->query).assign(mq.at(L), mq.at(L) + mq.len(L) * mq.row_bytes());
    ctx->query_pssm = mq.pssm;
    bool pruned = false;
    {
        const AboveMode mode(ctx, min_scores[L]);
        SwgSearchPlan plan;
        pruned = plan_search(ctx, db, false, &plan) == SWG_OK && plan_prune(ctx, db, false, 0, &plan) == SWG_OK && plan.prune.on;
    }
    ctx->query.swap(kept_query);
    ctx->pssm.swap(kept_pssm);
    ctx->query_pssm = kept_is_pssm;
    ctx->prune_choice = kept_choice;
    ctx->err = kept_err;
    return pruned;
}

// Route 2.  swg_prune_last afterwards: the sums over the batch's searches, pruned if any was.
static int above_multi_one_by_one(swg_ctx *ctx, swg_db *db, const MultiQueries &mq, bool gapless, const AboveMultiOut &o, swg_stats *st)
{
    const KeptQuery keep(ctx, false);
    swg_prune_info sum = swg_prune_info();
    int rc = SWG_OK;
    for (size_t i = 0; i < mq.n && rc == SWG_OK; ++i) {
        swg_stats one;
        memset(&one, 0, sizeof one);
        rc = mq.pssm ? swg_set_query_pssm(ctx, mq.at(i), mq.len(i)) : swg_set_query(ctx, mq.at(i), mq.len(i));
        if (rc == SWG_OK)
            rc = search_above_impl(ctx, db, gapless, mq.fn, o.min_scores[i], o.hits_out ? o.hits_out + i * o.cap : nullptr, o.cap,
                                   o.n_hits ? o.n_hits + i : nullptr, o.n_total ? o.n_total + i : nullptr, &one);
        if (rc != SWG_OK) break;
        add_one_search(st, one);
        sum.pruned |= ctx->prune_last.pruned;
        sum.pairs_skipped += ctx->prune_last.pairs_skipped;
        sum.pair_rows_skipped += ctx->prune_last.pair_rows_skipped;
        sum.pair_rows += ctx->prune_last.pair_rows;
    }
    sum.threshold = (uint32_t)o.min_scores[mq.n - 1];
    ctx->prune_last = sum;
    return keep.restore(ctx, rc);
}

// The per-row words of the read-out, for the first chunk (the largest), and a key pool to start with.
static int above_multi_allocate(swg_ctx *ctx, const SwgBatchPlan &P, MultiBufs *B)
{
    HIP_TRY(ctx, hipMalloc(&B->d_above_words, 3 * P.first_chunk * sizeof(uint32_t)));
    HIP_TRY(ctx, hipMalloc(&B->d_above_off, P.first_chunk * sizeof(uint64_t)));
    B->above_rows = P.first_chunk;
    return SWG_OK;
}

// Room for `need` keys in the chunk's pool: false where the device has none (the caller then selects on the host).
static bool above_multi_pool(MultiBufs *B, size_t need)
{
    if (need <= B->above_keys_cap) return true;
    const bool refuse = g_fail_alloc_site == 4; // (swg_debug_fail_alloc site 4: this allocation fails, once)
    if (refuse) g_fail_alloc_site = 0;
    const size_t want = std::max<size_t>(need + need / 4, SWG_ABOVE_KEYS_FLOOR);
    uint64_t *grown = nullptr;
    if (refuse || hipMalloc(&grown, want * sizeof(uint64_t)) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    (void)hipFree(B->d_above_keys);
    B->d_above_keys = grown;
    B->above_keys_cap = want;
    return true;
}

// What a chunk's fill left, to the caller: each score row r < Qb (query order[r] of the chunk; the row of an odd pair's
// absent partner is never read) against its own threshold.  The count kernel's answers are the n_total; where the caller
// takes hits the rows' keys are laid end to end in the pool, copied back and sorted per row as 64-bit keys (the appended
// order is not deterministic, the sorted one is).  Adds the chunk's times to *st.
static int above_multi_deliver_chunk(swg_ctx *ctx, const swg_db *db, const SwgBatchPlan &P, MultiBufs *B, size_t q0, size_t Qb, const AboveMultiOut &o,
                                     swg_stats *st)
{
    hipStream_t s = ctx->stream;
    const size_t n_slots = P.n_slots;
    if (Qb > B->above_rows || Qb > B->rows_scores)
        return swg_set_ctx_error(ctx, SWG_ERR_STATE, "swg_search_above_multi: the read-out indexes %zu rows, its buffers hold %zu", Qb,
                                 std::min(B->above_rows, B->rows_scores));
    uint32_t *d_thr = B->d_above_words, *d_counts = d_thr + B->above_rows, *d_cursors = d_counts + B->above_rows;
    std::vector<int32_t> thr(Qb); // (row order, not query order)
    for (size_t r = 0; r < Qb; ++r) thr[r] = o.min_scores[q0 + B->order[r]];
    std::vector<uint32_t> counts(Qb);
    HIP_TRY(ctx, hipMemcpyAsync(d_thr, thr.data(), Qb * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, swg_launch_above_rows_count(B->d_scores, n_slots, db->d_order, (uint32_t)n_slots, (uint32_t)Qb, (const int32_t *)d_thr, d_counts, s));
    HIP_TRY(ctx, hipEventRecord(ctx->cur->ev[3], s));
    HIP_TRY(ctx, hipMemcpyAsync(counts.data(), d_counts, Qb * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, spin_sync(ctx, s));
    float ms = 0.f, ms_read = 0.f;
    HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->cur->ev[1], ctx->cur->ev[2]));
    st->fill_ms += ms;
    st->total_ms += ms;
    HIP_TRY(ctx, hipEventElapsedTime(&ms_read, ctx->cur->ev[2], ctx->cur->ev[3]));
    std::vector<uint64_t> offsets(Qb), keys;
    uint64_t total = 0;
    for (size_t r = 0; r < Qb; ++r) {
        const size_t i = q0 + B->order[r];
        if (o.n_total) o.n_total[i] = counts[r];
        offsets[r] = total;
        total += counts[r];
    }
    double host_ms = 0.0;
    if (o.cap > 0 && total > 0) {
        const bool on_device = above_multi_pool(B, total);
        if (on_device) {
            HIP_TRY(ctx, hipMemcpyAsync(B->d_above_off, offsets.data(), Qb * 8, hipMemcpyHostToDevice, s));
            HIP_TRY(ctx, hipEventRecord(ctx->cur->ev[4], s));
            HIP_TRY(ctx, swg_launch_above_rows_scatter(B->d_scores, n_slots, db->d_order, (uint32_t)n_slots, (uint32_t)Qb, (const int32_t *)d_thr,
                                                       d_counts, B->d_above_off, d_cursors, B->d_above_keys, B->above_keys_cap, s));
            HIP_TRY(ctx, hipEventRecord(ctx->cur->ev[5], s));
            keys.resize(total);
            HIP_TRY(ctx, hipMemcpyAsync(keys.data(), B->d_above_keys, total * 8, hipMemcpyDeviceToHost, s));
            HIP_TRY(ctx, spin_sync(ctx, s));
            HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->cur->ev[4], ctx->cur->ev[5]));
            ms_read += ms;
        } else { // no room for the keys on the device: this chunk's score rows to the host, selected there
            B->h_scores.resize(Qb * n_slots);
            HIP_TRY(ctx, hipMemcpyAsync(B->h_scores.data(), B->d_scores, Qb * n_slots * 4, hipMemcpyDeviceToHost, s));
            HIP_TRY(ctx, spin_sync(ctx, s));
        }
        const auto t0 = std::chrono::steady_clock::now();
        for (size_t r = 0; r < Qb; ++r) {
            const size_t i = q0 + B->order[r], m = std::min<size_t>(o.cap, counts[r]);
            if (!on_device) {
                keys.clear();
                const int32_t *row = B->h_scores.data() + r * n_slots;
                for (size_t j = 0; j < n_slots; ++j)
                    if (db->order[j] != 0xFFFFFFFFu && row[j] >= thr[r]) keys.push_back(swg_hit_key(row[j], db->order[j]));
            }
            uint64_t *c = on_device ? keys.data() + offsets[r] : keys.data();
            const size_t nc = on_device ? counts[r] : keys.size(), w = std::min(m, nc);
            std::partial_sort(c, c + w, c + nc, std::greater<uint64_t>());
            for (size_t j = 0; j < w; ++j) swg_key_hit(c[j], &o.hits_out[i * o.cap + j]);
            if (o.n_hits) o.n_hits[i] = w;
        }
        host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    st->topk_ms += ms_read + host_ms;
    st->total_ms += ms_read;
    return SWG_OK;
}

static int search_above_multi_impl(swg_ctx *ctx, swg_db *db, const MultiQueries &mq, bool gapless, const AboveMultiOut &o, swg_stats *stats)
{
    const char *fn = mq.fn;
    for (size_t i = 0; i < mq.n; ++i) { // (zeroed before anything can fail)
        if (o.n_hits) o.n_hits[i] = 0;
        if (o.n_total) o.n_total[i] = 0;
    }
    swg_stats st;
    memset(&st, 0, sizeof st);
    if (!ctx || !db || !o.min_scores) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "%s: NULL argument", fn);
    if (o.cap > 0 && !o.hits_out) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "%s: cap > 0 but hits_out NULL", fn);
    int rc = validate_batch(ctx, db, mq, o.hits_out, o.cap, &st);
    if (rc != SWG_OK) return rc;
    for (size_t i = 0; i < mq.n; ++i)
        if (o.min_scores[i] < 1)
            return swg_set_ctx_error(ctx, SWG_ERR_ARG, "%s: min_score %d of query %zu must be at least 1 (every sequence scores at least 0)", fn,
                                     o.min_scores[i], i);
    if (stats) *stats = st;
    if (mq.n == 0) return SWG_OK;
    ctx->prune_last = swg_prune_info();
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    SwgBatchPlan P;
    if (!gapless && ctx->opt_above_batch != 2 && (rc = plan_batch(ctx, db, mq, false, 0, &P)) != SWG_OK) return rc;
    const bool single_pruned = P.one_launch && ctx->opt_above_batch == 0 && above_multi_single_pruned(ctx, db, mq, o.min_scores);
    if (swg_above_multi_route(ctx->opt_above_batch, P.one_launch, single_pruned) == 2) {
        rc = above_multi_one_by_one(ctx, db, mq, gapless, o, &st);
        if (stats) *stats = st;
        return rc;
    }
    MultiBufs B;
    ctx->cur = &ctx->slots[0];
    rc = batch_allocate(ctx, P, &B);
    if (rc == SWG_OK) rc = above_multi_allocate(ctx, P, &B);
    int chunks = 0;
    for (size_t q0 = 0; q0 < mq.n && rc == SWG_OK; q0 += P.chunk_queries, ++chunks) {
        const size_t Qb = std::min(P.chunk_queries, mq.n - q0);
        const size_t Qrows = P.grid_rows(Qb);
        rc = multi_rows_ok(ctx, B, P, Qb, Qrows);
        if (rc == SWG_OK) rc = batch_stage_chunk(ctx, P, mq, q0, Qb, &B);
        if (rc == SWG_OK) rc = batch_launch_chunk(ctx, db, P, B, Qb, Qrows);
        if (rc == SWG_OK) rc = above_multi_deliver_chunk(ctx, db, P, &B, q0, Qb, o, &st);
    }
    if (rc != SWG_OK) return rc;
    batch_report(ctx, db, P, mq.n, &st);
    st.fill_launches = chunks; // (launches of the bulk class's fill kernel: one per chunk)
    ctx->prune_last.threshold = (uint32_t)o.min_scores[mq.n - 1]; // (nothing pruned; pair_rows is not counted on this route)
    if (stats) *stats = st;
    return SWG_OK;
}

extern "C" int swg_search_above_multi(swg_ctx *ctx, const swg_db *db, const int8_t *queries, const uint64_t *q_offsets, size_t n_queries,
                                      const int32_t *min_scores, swg_hit *hits_out, size_t cap, size_t *n_hits, uint64_t *n_total, swg_stats *stats)
{
    return ctx_guarded(ctx, "swg_search_above_multi", [&]() -> int {
        return search_above_multi_impl(ctx, const_cast<swg_db *>(db), MultiQueries{queries, q_offsets, n_queries, false, "swg_search_above_multi"}, false,
                                       AboveMultiOut{min_scores, hits_out, cap, n_hits, n_total}, stats);
    });
}

extern "C" int swg_search_above_multi_pssm(swg_ctx *ctx, const swg_db *db, const int8_t *pssms, const uint64_t *q_offsets, size_t n_queries,
                                           const int32_t *min_scores, swg_hit *hits_out, size_t cap, size_t *n_hits, uint64_t *n_total,
                                           swg_stats *stats)
{
    return ctx_guarded(ctx, "swg_search_above_multi_pssm", [&]() -> int {
        return search_above_multi_impl(ctx, const_cast<swg_db *>(db), MultiQueries{pssms, q_offsets, n_queries, true, "swg_search_above_multi_pssm"},
                                       false, AboveMultiOut{min_scores, hits_out, cap, n_hits, n_total}, stats);
    });
}

extern "C" int swg_search_gapless_above_multi(swg_ctx *ctx, const swg_db *db, const int8_t *queries, const uint64_t *q_offsets, size_t n_queries,
                                              const int32_t *min_scores, swg_hit *hits_out, size_t cap, size_t *n_hits, uint64_t *n_total,
                                              swg_stats *stats)
{
    return ctx_guarded(ctx, "swg_search_gapless_above_multi", [&]() -> int {
        return search_above_multi_impl(ctx, const_cast<swg_db *>(db),
                                       MultiQueries{queries, q_offsets, n_queries, false, "swg_search_gapless_above_multi"}, true,
                                       AboveMultiOut{min_scores, hits_out, cap, n_hits, n_total}, stats);
    });
}

extern "C" int swg_search_gapless_above_multi_pssm(swg_ctx *ctx, const swg_db *db, const int8_t *pssms, const uint64_t *q_offsets, size_t n_queries,
                                                   const int32_t *min_scores, swg_hit *hits_out, size_t cap, size_t *n_hits, uint64_t *n_total,
                                                   swg_stats *stats)
{
    return ctx_guarded(ctx, "swg_search_gapless_above_multi_pssm", [&]() -> int {
        return search_above_multi_impl(ctx, const_cast<swg_db *>(db),
                                       MultiQueries{pssms, q_offsets, n_queries, true, "swg_search_gapless_above_multi_pssm"}, true,
                                       AboveMultiOut{min_scores, hits_out, cap, n_hits, n_total}, stats);
    });
}

// ---------------------------------------------------------------------------
// E-values: the residue counts of a database, and queries calibrated on the device
// ---------------------------------------------------------------------------
extern "C" int swg_db_composition(swg_ctx *ctx, const swg_db *db, uint64_t counts[32])
{
    if (!ctx || !db || !counts) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "swg_db_composition: NULL argument");
    memset(counts, 0, 32 * sizeof(uint64_t));
    if (db->tokens_only)
        return swg_set_ctx_error(ctx, SWG_ERR_STATE, "swg_db_composition: a database built from 16-lane batches has no residue bytes");
    if (db->device != ctx->device || !db->d_codes)
        return swg_set_ctx_error(ctx, SWG_ERR_STATE, "swg_db_composition: database is not resident on device %d", ctx->device);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    unsigned long long *d_counts = nullptr;
    HIP_TRY(ctx, hipMalloc(&d_counts, 32 * sizeof(unsigned long long)));
    hipError_t e = swg_launch_db_composition(db->d_codes, db->d_code_off, db->d_lens, (uint32_t)((size_t)db->n_bins * SWG_BIN), d_counts, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(counts, d_counts, 32 * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = spin_sync(ctx, ctx->stream);
    (void)hipFree(d_counts);
    HIP_TRY(ctx, e);
    return SWG_OK;
}

// swg_calibrate*: the queries are scored against the context's random database by the routes a search takes -- the one
// launch per chunk of swg_search_multi where plan_batch admits the batch, one search after another otherwise --, with
// the score rows left where the fill wrote them; swg_calib_fit_kernel histograms and fits each row, and one record per
// query comes back.
extern "C" int swg_debug_calib_iters(const swg_ctx *ctx, int32_t *out, size_t cap, size_t *n)
{
    if (!ctx || !n || (cap && !out)) return SWG_ERR_ARG;
    *n = ctx->calib_iters.size();
    if (*n <= cap && *n) memcpy(out, ctx->calib_iters.data(), *n * sizeof(int32_t));
    return SWG_OK;
}

// The random database of (freq, options calib_seqs / calib_len / calib_seed): the context's, or made now in its place.
static int calib_database(swg_ctx *ctx, const char *fn, const double *freq, swg_db **out)
{
    double key[32] = {};
    if (freq) {
        double tot = 0.0;
        for (int r = 0; r < 32; ++r) {
            if (!(freq[r] >= 0.0) || freq[r] > 1.7e308) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "%s: freq[%d] is not a finite, non-negative weight", fn, r);
            tot += freq[r];
        }
        if (freq[0] != 0.0) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "%s: freq[0], the padding residue's weight, must be 0", fn);
        if (!(tot > 0.0) || tot > 1.7e308) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "%s: the weights of freq must add up to a positive, finite sum", fn);
        for (int r = 0; r < 32; ++r) key[r] = freq[r] / tot;
    } else {
        key[0] = -1.0; // (the built-in table: no caller's freq normalises to this)
    }
    auto &c = ctx->calib;
    if (c.db && c.seqs == ctx->opt_calib_seqs && c.len == ctx->opt_calib_len && c.seed == ctx->opt_calib_seed && !memcmp(c.freq, key, sizeof key)) {
        *out = c.db;
        return SWG_OK;
    }
    int8_t *flat = nullptr;
    uint64_t *off = nullptr;
    int rc = swg_synth_db_iid((uint64_t)ctx->opt_calib_seed, (size_t)ctx->opt_calib_seqs, (uint32_t)ctx->opt_calib_len, freq, &flat, &off);
    if (rc != SWG_OK) return swg_set_ctx_error(ctx, rc, "%s: the random database could not be generated", fn);
    swg_db *db = nullptr;
    rc = swg_db_pack(flat, off, (size_t)ctx->opt_calib_seqs, 0, 1, &db);
    swg_synth_free(flat);
    swg_synth_free(off);
    if (rc != SWG_OK) return swg_set_ctx_error(ctx, rc, "%s: the random database could not be packed: %s", fn, swg_global_error());
    if ((rc = swg_db_upload(ctx, db)) != SWG_OK) {
        swg_db_free(db);
        return rc;
    }
    if (c.db) swg_db_free(c.db);
    c.db = db;
    memcpy(c.freq, key, sizeof key);
    c.seqs = ctx->opt_calib_seqs, c.len = ctx->opt_calib_len, c.seed = ctx->opt_calib_seed;
    *out = db;
    return SWG_OK;
}

static void calib_record(const swg_ctx *ctx, const SwgCalibFit &f, size_t lq, swg_evalue_params *p)
{
    p->lambda = f.lambda;
    p->mu = f.mu;
    p->K = f.status == 1 ? 0.0 : exp(f.lambda * f.mu) / ((double)lq * (double)ctx->calib.len);
    p->lq = (uint32_t)lq;
    p->n_seqs = (uint32_t)ctx->calib.seqs;
    p->seq_len = (uint32_t)ctx->calib.len;
    p->status = f.status;
}

// One search of the context's query against the random database, begun and ended with nothing read out; its exact
// scores -- the re-runs of flagged sequences included -- then lie in the slot's score buffer by sorted rank, and the fit
// kernel takes them as a single row.  Never tuned (a calibration is one search) and never pruned (ctx->in_batch).
static int calib_search_fit(swg_ctx *ctx, swg_db *cdb, bool gapless, const char *fn, SwgCalibFit *d_fit, SwgCalibFit *h_fit)
{
    struct Mode {
        swg_ctx *c;
        bool was_batch;
        Mode(swg_ctx *c_, bool g) : c(c_), was_batch(c_->in_batch) { c->gapless = g, c->in_batch = true; }
        ~Mode() { c->gapless = false, c->in_batch = was_batch; }
    } mode(ctx, gapless);
    int ticket = -1;
    int rc = search_begin_ticket(ctx, cdb, false, 0, false, &ticket);
    if (rc != SWG_OK) return rc;
    SwgSlot *S = &ctx->slots[ticket];
    // (search_begin has queued the fill and every re-run on the context's stream, or on streams joined to it: the fit
    // goes in behind them now, and the search's own end costs no idle gap in front of it)
    hipError_t e = swg_launch_calib_fit(S->bufs.d_scores, 0, cdb->d_order, (uint32_t)((size_t)cdb->n_bins * SWG_BIN), 1, d_fit, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(h_fit, d_fit, sizeof *h_fit, hipMemcpyDeviceToHost, ctx->stream);
    rc = ctx_guarded(ctx, fn, [&]() -> int { return search_end(ctx, S, nullptr, nullptr, nullptr, nullptr); });
    S->busy = false;
    if (rc != SWG_OK) return rc;
    HIP_TRY(ctx, e);
    HIP_TRY(ctx, spin_sync(ctx, ctx->stream));
    return SWG_OK;
}

namespace {
struct CalibFits { // the fit records of a chunk on the device
    SwgCalibFit *d = nullptr;
    ~CalibFits() { (void)hipFree(d); }
};
} // namespace

static int calib_state_ok(swg_ctx *ctx, const char *fn)
{
    if (!ctx->have_scoring) return swg_set_ctx_error(ctx, SWG_ERR_STATE, "%s: no scoring set", fn);
    for (const SwgSlot &sl : ctx->slots)
        if (sl.busy) return swg_set_ctx_error(ctx, SWG_ERR_STATE, "%s: searches are in flight on this context", fn);
    return SWG_OK;
}

static int calibrate_multi_impl(swg_ctx *ctx, const MultiQueries &mq, const double *freq, bool gapless, swg_evalue_params *out)
{
    const char *fn = mq.fn;
    if (!ctx || (mq.n && (!mq.src || !mq.off || !out))) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "%s: NULL argument", fn);
    int rc = calib_state_ok(ctx, fn);
    if (rc != SWG_OK) return rc;
    ctx->calib_iters.clear();
    if (mq.n == 0) return SWG_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    swg_db *cdb = nullptr;
    if ((rc = calib_database(ctx, fn, freq, &cdb)) != SWG_OK) return rc;
    swg_stats st;
    memset(&st, 0, sizeof st);
    if ((rc = validate_batch(ctx, cdb, mq, nullptr, 0, &st)) != SWG_OK) return rc;
    ctx->prune_last = swg_prune_info();
    ctx->calib_iters.assign(mq.n, 0);
    SwgBatchPlan P;
    if (!gapless && (rc = plan_batch(ctx, cdb, mq, false, 0, &P)) != SWG_OK) return rc;
    CalibFits fits;
    const size_t rows = P.one_launch ? P.first_chunk : 1;
    HIP_TRY(ctx, hipMalloc(&fits.d, rows * sizeof(SwgCalibFit)));
    std::vector<SwgCalibFit> h(rows);
    if (!P.one_launch) {
        const KeptQuery keep(ctx);
        for (size_t i = 0; i < mq.n && rc == SWG_OK; ++i) {
            rc = mq.pssm ? swg_set_query_pssm(ctx, mq.at(i), mq.len(i)) : swg_set_query(ctx, mq.at(i), mq.len(i));
            if (rc == SWG_OK) rc = calib_search_fit(ctx, cdb, gapless, fn, fits.d, h.data());
            if (rc != SWG_OK) break;
            calib_record(ctx, h[0], mq.len(i), &out[i]);
            ctx->calib_iters[i] = h[0].n_iter;
        }
        return keep.restore(ctx, rc);
    }
    MultiBufs B;
    ctx->cur = &ctx->slots[0];
    rc = batch_allocate(ctx, P, &B);
    for (size_t q0 = 0; q0 < mq.n && rc == SWG_OK; q0 += P.chunk_queries) {
        const size_t Qb = std::min(P.chunk_queries, mq.n - q0);
        const size_t Qrows = P.grid_rows(Qb);
        rc = multi_rows_ok(ctx, B, P, Qb, Qrows);
        if (rc == SWG_OK) rc = batch_stage_chunk(ctx, P, mq, q0, Qb, &B);
        if (rc == SWG_OK) rc = batch_launch_chunk(ctx, cdb, P, B, Qb, Qrows);
        if (rc != SWG_OK) break;
        if (Qb > rows || Qb > B.rows_scores)
            return swg_set_ctx_error(ctx, SWG_ERR_STATE, "%s: the fit indexes %zu rows, its buffers hold %zu", fn, Qb, std::min(rows, B.rows_scores));
        // score row r of the chunk belongs to its query order[r] (the row of an odd pair's absent partner is not read)
        HIP_TRY(ctx, swg_launch_calib_fit(B.d_scores, P.n_slots, cdb->d_order, (uint32_t)P.n_slots, (uint32_t)Qb, fits.d, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(h.data(), fits.d, Qb * sizeof(SwgCalibFit), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, spin_sync(ctx, ctx->stream));
        for (size_t r = 0; r < Qb; ++r) {
            const size_t i = q0 + B.order[r];
            calib_record(ctx, h[r], mq.len(i), &out[i]);
            ctx->calib_iters[i] = h[r].n_iter;
        }
    }
    return rc;
}

extern "C" int swg_calibrate(swg_ctx *ctx, const double *freq, int gapless, swg_evalue_params *out)
{
    const char *fn = "swg_calibrate";
    if (!ctx || !out) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "%s: NULL argument", fn);
    return ctx_guarded(ctx, fn, [&]() -> int {
        int rc = calib_state_ok(ctx, fn);
        if (rc != SWG_OK) return rc;
        if (ctx->query_len() == 0) return swg_set_ctx_error(ctx, SWG_ERR_STATE, "%s: no query set", fn);
        ctx->calib_iters.clear();
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        swg_db *cdb = nullptr;
        if ((rc = calib_database(ctx, fn, freq, &cdb)) != SWG_OK) return rc;
        CalibFits fits;
        HIP_TRY(ctx, hipMalloc(&fits.d, sizeof(SwgCalibFit)));
        SwgCalibFit h;
        if ((rc = calib_search_fit(ctx, cdb, gapless != 0, fn, fits.d, &h)) != SWG_OK) return rc;
        calib_record(ctx, h, ctx->query_len(), out);
        ctx->calib_iters.assign(1, h.n_iter);
        return SWG_OK;
    });
}

extern "C" int swg_calibrate_multi(swg_ctx *ctx, const int8_t *queries, const uint64_t *q_offsets, size_t n_queries, const double *freq,
                                   int gapless, swg_evalue_params *out)
{
    return ctx_guarded(ctx, "swg_calibrate_multi", [&]() -> int {
        return calibrate_multi_impl(ctx, MultiQueries{queries, q_offsets, n_queries, false, "swg_calibrate_multi"}, freq, gapless != 0, out);
    });
}

extern "C" int swg_calibrate_multi_pssm(swg_ctx *ctx, const int8_t *pssms, const uint64_t *q_offsets, size_t n_queries, const double *freq,
                                        int gapless, swg_evalue_params *out)
{
    return ctx_guarded(ctx, "swg_calibrate_multi_pssm", [&]() -> int {
        return calibrate_multi_impl(ctx, MultiQueries{pssms, q_offsets, n_queries, true, "swg_calibrate_multi_pssm"}, freq, gapless != 0, out);
    });
}

// ---------------------------------------------------------------------------
// every query of a batch against its own candidate list in one pass
// ---------------------------------------------------------------------------
// swg_search_multi searches the same sequences for every query and keeps n_queries x n_slots scores on the device; a
// prefilter hands over a list per query, 0.01 % of the database each.  Here the lists become one job database J
// (swg_list_jobs: a view-like selection per query, laid end to end, aliasing the resident residue bytes), J gets slot words,
// pair offsets and pair tokens by the kernels every database gets them from, and ONE launch of the work-queue fill's
// LISTS instantiation runs it: workgroup b works for the row its table entry names, with that row's profile and queue, on
// that row's pairs of J only, and every pair writes its two scores into the one score array of J.  What comes back is 4
// bytes per job; the host scatters them to the caller's entries and selects each row's top-K.
namespace {
// One chunk of queries [q0, q0 + Qb): its job database on the host and how the launch's workgroups are dealt.
struct ListChunk {
    size_t q0 = 0, Qb = 0;
    SwgListJobs J;
    std::vector<uint32_t> pair_off;  // [pairs + 1] token blocks before each pair of J
    std::vector<uint32_t> row_pairs; // [Qb + 1] J.row_pairs in the kernel's 32 bits
    std::vector<uint2> wg_rows;      // the grid: (row, index within the row), rows with the most work first
    size_t n_slots() const { return J.slots.size(); }
    size_t n_pairs() const { return J.slots.size() / 2; }
    uint64_t blocks() const { return pair_off.empty() ? 0 : pair_off.back(); }
};
// What a lists call decides before it queues anything: written once by plan_lists, read by the stages.
struct SwgListsPlan {
    bool one_launch = false; // else one list after another through a view, and nothing below is set
    int go = 0, ge = 0, form = 0;
    SwgDiagPlan pl;          // the one class
    uint64_t bound_max = 0;
    size_t lq_max = 0;
    size_t chunk_queries = 256;
    int resident_wgs = 0;    // workgroups of this geometry the chip holds
    bool equal_shares = false; // experiment (SWG_LISTS_EQUAL_SHARES): workgroups dealt one share per row instead of by work
    uint32_t class_queue_dwords = 0;
    size_t rank_word_base = 0, queue_dwords = 0, prof_row_bytes = 0;
};
// Device buffers of a lists call, grown to the largest chunk; beside each what it holds (lists_fence).
struct ListBufs {
    uint32_t *d_slots = nullptr, *d_lens = nullptr, *d_order = nullptr, *d_pair_off = nullptr, *d_row_pairs = nullptr, *d_cnt = nullptr,
             *d_qoff = nullptr;
    uint64_t *d_code_off = nullptr;
    uint4 *d_tok = nullptr;
    uint2 *d_wg_rows = nullptr;
    int32_t *d_scores = nullptr;
    uint8_t *d_prof = nullptr;
    int8_t *d_q = nullptr;
    size_t cap_slots = 0, cap_pairs = 0, cap_rows = 0, cap_wgs = 0, cap_prof_rows = 0, cap_q = 0, cnt_rows = 0;
    uint64_t cap_blocks = 0;
    std::vector<int32_t> h_scores;
    std::vector<uint32_t> qoff32;
    std::vector<uint64_t> keys;
    ~ListBufs()
    {
        for (void *p : {(void *)d_slots, (void *)d_lens, (void *)d_order, (void *)d_pair_off, (void *)d_row_pairs, (void *)d_cnt, (void *)d_qoff,
                        (void *)d_code_off, (void *)d_tok, (void *)d_wg_rows, (void *)d_scores, (void *)d_prof, (void *)d_q})
            (void)hipFree(p);
    }
};
const uint64_t kListChunkBlocks = 1ull << 28; // token blocks of one chunk's J (4 GB of tokens); well inside pair_off's 32 bits
} // namespace

// The host image of every chunk: the job tables, their pair offsets, and the cells the batch is worth.  A chunk is at
// most chunk_queries queries and is cut further where its J would pass the 32-bit limits of the slot count or the pair
// offsets; a single list beyond them has no chunk (*too_large: the call then goes one list after another).
static int lists_build_chunks(swg_ctx *ctx, const swg_db *db, const MultiQueries &mq, const uint32_t *cand, const uint64_t *c_off,
                              size_t chunk_queries, std::vector<ListChunk> *chunks, bool *too_large, swg_stats *st)
{
    chunks->clear();
    *too_large = false;
    st->cells = st->bytes_alg = 0;
    for (size_t q0 = 0; q0 < mq.n;) {
        size_t Qb = std::min(chunk_queries, mq.n - q0);
        ListChunk C;
        for (;;) {
            C = ListChunk();
            C.q0 = q0;
            C.Qb = Qb;
            const int rc = swg_list_jobs(db, cand, c_off, q0, Qb, &C.J);
            if (rc != SWG_OK) return swg_set_ctx_error(ctx, rc, "%s", swg_global_error());
            const size_t np = C.n_pairs();
            const uint64_t total = C.J.pair_blocks.back();
            C.pair_off.assign(np + 1, 0u);
            for (size_t p = 0; p <= np; ++p) C.pair_off[p] = (uint32_t)std::min<uint64_t>(C.J.pair_blocks[p], 0xFFFFFFFFull);
            if (total <= kListChunkBlocks && C.n_slots() < (1ull << 31)) break;
            if (Qb == 1) {
                *too_large = true;
                break;
            }
            Qb = (Qb + 1) / 2;
        }
        C.row_pairs.resize(Qb + 1);
        for (size_t i = 0; i <= Qb; ++i) C.row_pairs[i] = (uint32_t)C.J.row_pairs[i];
        for (size_t i = 0; i < Qb; ++i) {
            st->cells += (uint64_t)mq.len(q0 + i) * C.J.row_residues[i];
            st->bytes_alg += C.J.row_residues[i] + 8ull * (C.J.row_pairs[i + 1] - C.J.row_pairs[i]) * 2 + 32ull * mq.len(q0 + i) + 1024ull;
        }
        chunks->push_back(std::move(C));
        q0 += Qb;
    }
    return SWG_OK;
}

// plan_batch's rules applied to the job database: the gap scores fit the packed form, no option asks for an engine or a
// geometry, every query takes one pass of the class and no score can reach the int16 ceiling -- each query bounded by the
// longest sequence of ITS OWN list --; the f16 cells where no query's bound reaches theirs.  One class takes all pairs
// (the many rows amortise the chains: DESIGN 4.2), one pair per request, no two queries per lane (they would need the same
// sequence).  The geometry is the planner's for the chunk with the most work, its pairs longest first.
static int plan_lists(swg_ctx *ctx, const swg_db *db, const MultiQueries &mq, const std::vector<ListChunk> &chunks, bool too_large,
                      SwgListsPlan *plan)
{
    *plan = SwgListsPlan();
    SwgListsPlan P;
    const swg_db *root = db->root ? db->root : db;
    P.go = ctx->gap_open + ctx->gap_extend;
    P.ge = ctx->gap_extend;
    for (size_t i = 0; i < mq.n; ++i) P.lq_max = std::max(P.lq_max, mq.len(i));
    bool fast = ctx->gap_open <= 0 && ctx->gap_extend <= 0 && -P.go <= SWG_I16_CEILING && ctx->opt_force_bits != 32 &&
                ctx->opt_engine != 1 && ctx->opt_dynamic != 0 && !too_large && ctx->opt_max_waves == 0 && ctx->opt_workgroups == 0;
    const ListChunk *big = nullptr;
    for (const ListChunk &C : chunks) {
        if (!big || C.blocks() > big->blocks()) big = &C;
        for (size_t i = 0; i < C.Qb && fast; ++i) {
            if (C.J.row_pairs[i + 1] == C.J.row_pairs[i]) continue; // (an empty list scores nothing)
            const size_t q = C.q0 + i;
            const uint64_t longest = ((uint64_t)C.J.row_longest[i] + SWG_ROWS_PER_BLK - 1) / SWG_ROWS_PER_BLK * SWG_ROWS_PER_BLK;
            const SwgScoreBound sb = mq.pssm ? swg_score_bound(mq.at(q), nullptr, mq.len(q), longest)
                                             : swg_score_bound(&ctx->sub[0][0], mq.at(q), mq.len(q), longest);
            P.bound_max = std::max(P.bound_max, sb.bound);
            if (sb.bound >= SWG_I16_CEILING) fast = false;
        }
    }
    if (!fast || !big || big->n_pairs() == 0) { // (nothing to launch anywhere: the route that launches nothing)
        plan->lq_max = P.lq_max;
        return SWG_OK;
    }
    P.form = ctx->opt_f16 != 0 && P.bound_max < SWG_F16_CEILING && swg_f16_gaps_ok(P.go, P.ge) ? 2 : 0;
    // the planner's model of J: its pairs, longest first (the planner reads lengths and nothing else)
    swg_db M;
    {
        const size_t np = big->n_pairs();
        std::vector<std::pair<uint32_t, uint32_t>> pairs(np);
        for (size_t p = 0; p < np; ++p) {
            const uint32_t sy = big->J.slots[2 * p + 1];
            pairs[p] = std::make_pair(root->lens[big->J.slots[2 * p]], sy == 0xFFFFFFFFu ? 0u : root->lens[sy]);
        }
        lists_model_db(&pairs, &M);
    }
    SwgDiagWork wk;
    const SwgBatchAsk ask = {P.lq_max, ctx->n_cu, 1.0, P.form, ctx->opt_cols, ctx->opt_group, ctx->opt_batch_geometry, -1, false};
    fast = batch_plan_work(&M, ask, &wk) && wk.n_classes == 1;
    if (!fast) {
        plan->lq_max = P.lq_max;
        return SWG_OK;
    }
    P.pl = wk.plan[0];
    P.resident_wgs = ctx->n_cu * batch_class_per_cu(P.pl, false, 1, 0);
    static const bool equal_shares = getenv("SWG_LISTS_EQUAL_SHARES") != nullptr;
    P.equal_shares = equal_shares;
    P.class_queue_dwords = SWG_DYN_SHARDS * SWG_DYN_SHARD_STRIDE;
    P.rank_word_base = P.chunk_queries * P.class_queue_dwords; // (the queues serve a full chunk's rows)
    P.queue_dwords = P.rank_word_base + SWG_DYN_SIMD_SLOTS;
    P.prof_row_bytes = batch_prof_row_bytes(P.pl, false);
    P.one_launch = true;
    *plan = P;
    return SWG_OK;
}

// The workgroups of one chunk's launch, dealt by work: every row with pairs gets one, and the rest of the chip's
// resident workgroups go to the rows in proportion to their token blocks -- never more than a row's pairs can keep busy
// (one pair per lane group).  Rows with the most work come first in the grid; empty rows get none.  With 256 rows per
// chunk and a workgroup per CU the grid stays within what the chip holds at once.
static void lists_deal_workgroups(const SwgListsPlan &P, ListChunk *C)
{
    swg_lists_deal(C->J, (uint64_t)P.pl.W * (64 / P.pl.G), (uint64_t)std::max(0, P.resident_wgs), P.equal_shares, &C->wg_rows);
}

// The device buffers for one chunk, each with what it holds written beside it.
static int lists_allocate(swg_ctx *ctx, const SwgListsPlan &P, const ListChunk &C, const MultiQueries &mq, ListBufs *B)
{
    int rc;
    size_t cap = B->cap_slots;
    if ((rc = device_grow(ctx, &B->d_slots, &cap, C.n_slots())) != SWG_OK) return rc;
    cap = B->cap_slots;
    if ((rc = device_grow(ctx, &B->d_lens, &cap, C.n_slots())) != SWG_OK) return rc;
    cap = B->cap_slots;
    if ((rc = device_grow(ctx, &B->d_order, &cap, C.n_slots())) != SWG_OK) return rc;
    cap = B->cap_slots;
    if ((rc = device_grow(ctx, &B->d_code_off, &cap, C.n_slots(), 1)) != SWG_OK) return rc;
    if ((rc = device_grow(ctx, &B->d_scores, &B->cap_slots, C.n_slots())) != SWG_OK) return rc;
    if ((rc = device_grow(ctx, &B->d_pair_off, &B->cap_pairs, C.n_pairs(), 1)) != SWG_OK) return rc;
    size_t cb = (size_t)B->cap_blocks;
    if ((rc = device_grow(ctx, &B->d_tok, &cb, (size_t)C.blocks(), 1)) != SWG_OK) return rc; // (+ the block of zeros behind the last pair)
    B->cap_blocks = cb;
    if ((rc = device_grow(ctx, &B->d_row_pairs, &B->cap_rows, C.Qb, 1)) != SWG_OK) return rc;
    cap = B->cap_prof_rows;
    if ((rc = device_grow(ctx, &B->d_qoff, &cap, C.Qb, 1)) != SWG_OK) return rc;
    if (!B->d_prof || B->cap_prof_rows < C.Qb) {
        (void)hipFree(B->d_prof);
        B->d_prof = nullptr;
        B->cap_prof_rows = 0;
        HIP_TRY(ctx, hipMalloc(&B->d_prof, C.Qb * P.prof_row_bytes));
        B->cap_prof_rows = C.Qb;
    }
    if ((rc = device_grow(ctx, &B->d_wg_rows, &B->cap_wgs, C.wg_rows.size())) != SWG_OK) return rc;
    if (!B->d_cnt) {
        HIP_TRY(ctx, hipMalloc(&B->d_cnt, P.queue_dwords * 4));
        B->cnt_rows = P.chunk_queries;
    }
    const size_t qbytes = (size_t)(mq.off[C.q0 + C.Qb] - mq.off[C.q0]) * mq.row_bytes();
    return device_grow(ctx, &B->d_q, &B->cap_q, qbytes);
}

// The fence before every launch, in the manner of multi_rows_ok: what the launch will index -- from the chunk's tables,
// as the launch's own arguments are -- against what the buffers hold.  A violation is a bug of this file; it is reported
// as SWG_ERR_STATE, not launched (the fault of round 3 was a row count that disagreed with a buffer: DESIGN 4.2).
static int lists_fence(swg_ctx *ctx, const SwgListsPlan &P, const ListChunk &C, const ListBufs &B, size_t grid)
{
    const char *fn = "swg_search_lists";
    const size_t np = C.n_pairs();
    if (C.wg_rows.size() != grid || grid == 0 || B.cap_wgs < grid)
        return swg_set_ctx_error(ctx, SWG_ERR_STATE, "%s: the workgroup table has %zu entries (room for %zu), the grid %zu", fn, C.wg_rows.size(), B.cap_wgs, grid);
    for (size_t b = 0; b < grid; ++b)
        if (C.wg_rows[b].x >= C.Qb)
            return swg_set_ctx_error(ctx, SWG_ERR_STATE, "%s: workgroup %zu is dealt to row %u of a chunk of %zu rows", fn, b, C.wg_rows[b].x, C.Qb);
    if (C.row_pairs.size() != C.Qb + 1 || C.row_pairs[0] != 0u || C.pair_off.size() != np + 1)
        return swg_set_ctx_error(ctx, SWG_ERR_STATE, "%s: %zu range entries and %zu pair offsets for %zu rows and %zu pairs", fn, C.row_pairs.size(),
                                 C.pair_off.size(), C.Qb, np);
    for (size_t i = 0; i < C.Qb; ++i) // disjoint and ascending by construction of a prefix: each range within J, none reversed
        if (C.row_pairs[i + 1] < C.row_pairs[i] || C.row_pairs[i + 1] > np)
            return swg_set_ctx_error(ctx, SWG_ERR_STATE, "%s: row %zu takes pairs [%u, %u) of a job table of %zu pairs", fn, i, C.row_pairs[i],
                                     C.row_pairs[i + 1], np);
    struct { const char *name; size_t have, need; } chk[] = {
        {"d_scores / slot words", B.cap_slots, C.n_slots()}, {"d_pair_off", B.cap_pairs, np},
        {"d_tok", (size_t)B.cap_blocks, (size_t)C.blocks()},  {"d_row_pairs", B.cap_rows, C.Qb},
        {"d_prof", B.cap_prof_rows, C.Qb},                    {"d_cnt", B.cnt_rows, C.Qb},
        {"queue words", P.queue_dwords, C.Qb * (size_t)P.class_queue_dwords + SWG_DYN_SIMD_SLOTS},
    };
    for (const auto &c : chk)
        if (c.have < c.need)
            return swg_set_ctx_error(ctx, SWG_ERR_STATE, "%s: %s holds %zu, the launch indexes %zu (chunk of %zu rows, %zu jobs)", fn, c.name, c.have,
                                     c.need, C.Qb, C.n_slots());
    if (2 * np != C.n_slots()) return swg_set_ctx_error(ctx, SWG_ERR_STATE, "%s: %zu slots are not %zu whole pairs", fn, C.n_slots(), np);
    return SWG_OK;
}

// One chunk to the device: J's slots (4 bytes per job) and pair offsets, from which the gather and token kernels write
// its slot words and tokens out of the root's resident ones; the queries, their profiles; scores and queues zeroed.
static int lists_stage_chunk(swg_ctx *ctx, const swg_db *db, const SwgListsPlan &P, const MultiQueries &mq, const ListChunk &C, ListBufs *B)
{
    hipStream_t s = ctx->stream;
    const swg_db *root = db->root ? db->root : db;
    const size_t ns = C.n_slots(), np = C.n_pairs(), Qb = C.Qb;
    HIP_TRY(ctx, hipMemcpyAsync(B->d_slots, C.J.slots.data(), ns * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(B->d_pair_off, C.pair_off.data(), (np + 1) * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(B->d_row_pairs, C.row_pairs.data(), (Qb + 1) * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(B->d_wg_rows, C.wg_rows.data(), C.wg_rows.size() * sizeof(uint2), hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, swg_launch_gather_view(B->d_slots, (uint32_t)ns, (uint32_t)root->order.size(), root->d_code_off, root->d_lens, root->d_order,
                                        B->d_code_off, B->d_lens, B->d_order, s));
    HIP_TRY(ctx, hipMemsetAsync(B->d_tok + C.blocks(), 0, 16, s));
    HIP_TRY(ctx, swg_launch_build_tokens(root->d_codes, B->d_code_off, B->d_lens, B->d_pair_off, (uint32_t)np, C.blocks(), B->d_tok, s));
    std::vector<uint32_t> &qoff32 = B->qoff32;
    qoff32.resize(Qb + 1);
    for (size_t i = 0; i <= Qb; ++i) qoff32[i] = (uint32_t)(mq.off[C.q0 + i] - mq.off[C.q0]);
    const size_t qbytes = (size_t)(mq.off[C.q0 + Qb] - mq.off[C.q0]) * mq.row_bytes();
    HIP_TRY(ctx, hipMemcpyAsync(B->d_q, mq.at(C.q0), qbytes, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(B->d_qoff, qoff32.data(), (Qb + 1) * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemsetAsync(B->d_scores, 0, ns * 4, s));
    HIP_TRY(ctx, hipMemsetAsync(B->d_cnt, 0, P.queue_dwords * 4, s));
    const int kp = swg_diag_padded_cols(P.pl.K);
    HIP_TRY(ctx, swg_launch_build_profiles_multi(ctx->d_sub, mq.pssm ? nullptr : B->d_q, B->d_qoff, (uint32_t)Qb, (uint32_t)(P.pl.G * kp), P.pl.K, kp,
                                                 B->d_prof, s, SWG_LDS_SWIZZLE ? P.pl.G : 0, P.form == 2, mq.pssm ? B->d_q : nullptr));
    return SWG_OK;
}

// The fill of one chunk: one launch, a 1-D grid of the dealt workgroups.  Events: ev[1] before, ev[2] after.
static int lists_launch_chunk(swg_ctx *ctx, const SwgListsPlan &P, const ListChunk &C, const ListBufs &B)
{
    hipStream_t s = ctx->stream;
    SwgPairTokens T; // (what the launch's token parameters are read from: this chunk's J)
    T.d_tok = B.d_tok;
    T.d_pair_off = B.d_pair_off;
    T.total_blocks = C.blocks();
    SwgDiagDynParams q = dyn_params_base(T, B.d_scores, C.n_slots(), P.pl.G, P.form, P.go, P.ge, 1, B.d_cnt + P.rank_word_base);
    q.queue = B.d_cnt;
    q.queue_stride = P.class_queue_dwords;
    q.profile = B.d_prof;
    q.profile_stride = P.prof_row_bytes;
    q.score_stride = 0;
    q.q_begin = 0;
    q.q_end = (uint32_t)C.n_pairs();
    q.row_pairs = B.d_row_pairs;
    q.wg_rows = B.d_wg_rows;
    q.prio_blocks = bulk_prio_blocks(ctx, C.blocks(), (uint64_t)C.wg_rows.size() * P.pl.W * (64 / P.pl.G));
    HIP_TRY(ctx, hipEventRecord(ctx->cur->ev[1], s));
    HIP_TRY(ctx, swg_launch_diag_lists(P.pl.variant, P.form, P.pl.W, (int)C.wg_rows.size(), q, s));
    HIP_TRY(ctx, hipEventRecord(ctx->cur->ev[2], s));
    return SWG_OK;
}

// A row's results from J's scores (host): the caller's entries through the entry-to-job map -- duplicates get the same
// score, ignored entries none -- and the row's k best by swg_hit_key's order over its non-empty slots.
static void lists_deliver_rows(const swg_db *db, const ListChunk &C, const int32_t *h_scores, const uint64_t *c_off, size_t k,
                               int32_t *scores_out, swg_hit *topk_out, size_t *n_hits, std::vector<uint64_t> *keys)
{
    const swg_db *root = db->root ? db->root : db;
    if (scores_out)
        for (size_t e = 0; e < C.J.entry_job.size(); ++e)
            if (C.J.entry_job[e] != 0xFFFFFFFFu) scores_out[C.J.entry0 + e] = h_scores[C.J.entry_job[e]];
    (void)c_off;
    for (size_t i = 0; i < C.Qb; ++i) {
        size_t m = 0;
        if (k > 0 && topk_out) {
            keys->clear();
            for (size_t j = 2 * C.J.row_pairs[i]; j < 2 * C.J.row_pairs[i + 1]; ++j)
                if (C.J.slots[j] != 0xFFFFFFFFu) keys->push_back(swg_hit_key(h_scores[j], root->order[C.J.slots[j]]));
            m = std::min(k, keys->size());
            std::partial_sort(keys->begin(), keys->begin() + m, keys->end(), std::greater<uint64_t>());
            for (size_t j = 0; j < m; ++j) swg_key_hit((*keys)[j], &topk_out[(C.q0 + i) * k + j]);
        }
        if (n_hits) n_hits[C.q0 + i] = m;
    }
}

// One device-to-host copy of J's scores (4 bytes per job) behind the chunk's fill, then the rows on the host.
static int lists_deliver_chunk(swg_ctx *ctx, const swg_db *db, const ListChunk &C, ListBufs *B, const uint64_t *c_off, size_t k,
                               int32_t *scores_out, swg_hit *topk_out, size_t *n_hits, swg_stats *st)
{
    hipStream_t s = ctx->stream;
    B->h_scores.resize(C.n_slots());
    HIP_TRY(ctx, hipMemcpyAsync(B->h_scores.data(), B->d_scores, C.n_slots() * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, spin_sync(ctx, s));
    float ms = 0.f;
    HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->cur->ev[1], ctx->cur->ev[2]));
    st->fill_ms += ms;
    st->total_ms += ms;
    const auto t0 = std::chrono::steady_clock::now();
    lists_deliver_rows(db, C, B->h_scores.data(), c_off, k, scores_out, topk_out, n_hits, &B->keys);
    st->topk_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return SWG_OK;
}

// One list after another: a view per list, then swg_search's own body; the context's query is put back afterwards.
// Statistics as search_batch_one_by_one reports them (fill_launches stays 0).
static int lists_one_by_one(swg_ctx *ctx, swg_db *db, const MultiQueries &mq, const std::vector<ListChunk> &chunks, const uint32_t *cand,
                            const uint64_t *c_off, int32_t *scores_out, swg_hit *topk_out, size_t k, size_t *n_hits, swg_stats *st)
{
    const KeptQuery keep(ctx);
    std::vector<int32_t> by_index(scores_out ? db->n_total : 0);
    int rc = SWG_OK;
    for (const ListChunk &C : chunks)
        for (size_t i = 0; i < C.Qb && rc == SWG_OK; ++i) {
            const size_t q = C.q0 + i;
            const uint64_t e0 = c_off[q], e1 = c_off[q + 1];
            if (n_hits) n_hits[q] = 0;
            if (C.J.row_pairs[i + 1] == C.J.row_pairs[i]) continue; // nothing of the list is held here
            swg_db *view = nullptr;
            swg_stats one;
            rc = swg_db_view(ctx, db, cand + e0, (size_t)(e1 - e0), &view);
            if (rc == SWG_OK) rc = mq.pssm ? swg_set_query_pssm(ctx, mq.at(q), mq.len(q)) : swg_set_query(ctx, mq.at(q), mq.len(q));
            if (rc == SWG_OK)
                rc = search_now(ctx, view, ctx->opt_autotune != 0, scores_out ? by_index.data() : nullptr, topk_out ? topk_out + q * k : nullptr, k,
                                n_hits ? n_hits + q : nullptr, &one);
            swg_db_free(view);
            if (rc != SWG_OK) break;
            for (uint64_t e = e0; e < e1 && scores_out; ++e)
                if (C.J.entry_job[(size_t)(e - C.J.entry0)] != 0xFFFFFFFFu) scores_out[e] = by_index[cand[e]];
            add_one_search(st, one);
        }
    return keep.restore(ctx, rc);
}

// The statistics of a lists call that went through the launches, from its plan and its chunks.
static void lists_report(const SwgListsPlan &P, const std::vector<ListChunk> &chunks, int launches, swg_stats *st)
{
    st->path_bits = 16;
    st->engine = 2;
    st->work_queue = 1;
    st->classes_overlapped = -1;
    st->cell_form = P.form;
    st->cols_per_wave = P.pl.K;
    st->group_lanes = P.pl.G;
    st->waves = P.pl.W;
    st->passes = 1;
    st->fill_launches = launches;
    for (const ListChunk &C : chunks) {
        if (C.wg_rows.empty()) continue;
        st->workgroups = (int32_t)C.wg_rows.size(); // (the last launch's)
        st->streams = (int32_t)(C.wg_rows.size() * P.pl.W * (64 / P.pl.G));
        st->cells_padded += 2ull * P.pl.G * P.pl.K * C.blocks() * 4ull;
    }
}

static int search_lists_impl(swg_ctx *ctx, swg_db *db, const MultiQueries &mq, const uint32_t *cand, const uint64_t *c_off,
                             int32_t *scores_out, swg_hit *topk_out, size_t k, size_t *n_hits, swg_stats *stats)
{
    swg_stats st;
    memset(&st, 0, sizeof st);
    int rc = validate_batch(ctx, db, mq, topk_out, k, &st);
    if (rc != SWG_OK) return rc;
    ctx->prune_last = swg_prune_info(); // (swg_prune_last: a batch call ends with nothing pruned)
    if (mq.n && (!c_off || (c_off[mq.n] > c_off[0] && !cand))) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "%s: NULL argument", mq.fn);
    if (db->tokens_only)
        return swg_set_ctx_error(ctx, SWG_ERR_STATE, "%s: a database built from 16-lane batches has no residue bytes to list candidates of", mq.fn);
    st.cells = st.bytes_alg = 0;
    if (stats) *stats = st;
    if (mq.n == 0) return SWG_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::vector<ListChunk> chunks;
    bool too_large = false;
    rc = lists_build_chunks(ctx, db, mq, cand, c_off, 256, &chunks, &too_large, &st);
    if (rc != SWG_OK) return rc;
    SwgListsPlan P;
    rc = plan_lists(ctx, db, mq, chunks, too_large, &P);
    if (rc != SWG_OK) return rc;
    if (!P.one_launch) {
        rc = lists_one_by_one(ctx, db, mq, chunks, cand, c_off, scores_out, topk_out, k, n_hits, &st);
        if (stats) *stats = st;
        return rc;
    }
    ListBufs B;
    ctx->cur = &ctx->slots[0];
    int launches = 0;
    for (ListChunk &C : chunks) {
        lists_deal_workgroups(P, &C);
        if (C.wg_rows.empty()) { // every list of the chunk is empty here: nothing to launch, nothing to write
            for (size_t i = 0; i < C.Qb && n_hits; ++i) n_hits[C.q0 + i] = 0;
            continue;
        }
        rc = lists_allocate(ctx, P, C, mq, &B);
        if (rc == SWG_OK) rc = lists_fence(ctx, P, C, B, C.wg_rows.size()); // what this chunk's launch will index, against the buffers
        if (rc == SWG_OK) rc = lists_stage_chunk(ctx, db, P, mq, C, &B);
        if (rc == SWG_OK) rc = lists_launch_chunk(ctx, P, C, B);
        if (rc == SWG_OK) rc = lists_deliver_chunk(ctx, db, C, &B, c_off, k, scores_out, topk_out, n_hits, &st);
        if (rc != SWG_OK) return rc;
        ++launches;
    }
    lists_report(P, chunks, launches, &st);
    if (stats) *stats = st;
    return SWG_OK;
}

extern "C" int swg_search_lists(swg_ctx *ctx, const swg_db *db, const int8_t *queries, const uint64_t *q_offsets, size_t n_queries,
                                const uint32_t *cand, const uint64_t *c_offsets, int32_t *scores_out, swg_hit *topk_out, size_t k,
                                size_t *n_hits, swg_stats *stats)
{
    return ctx_guarded(ctx, "swg_search_lists", [&]() -> int {
        return search_lists_impl(ctx, const_cast<swg_db *>(db), MultiQueries{queries, q_offsets, n_queries, false, "swg_search_lists"}, cand,
                                 c_offsets, scores_out, topk_out, k, n_hits, stats);
    });
}

extern "C" int swg_search_lists_pssm(swg_ctx *ctx, const swg_db *db, const int8_t *pssms, const uint64_t *q_offsets, size_t n_queries,
                                     const uint32_t *cand, const uint64_t *c_offsets, int32_t *scores_out, swg_hit *topk_out, size_t k,
                                     size_t *n_hits, swg_stats *stats)
{
    return ctx_guarded(ctx, "swg_search_lists_pssm", [&]() -> int {
        return search_lists_impl(ctx, const_cast<swg_db *>(db), MultiQueries{pssms, q_offsets, n_queries, true, "swg_search_lists_pssm"}, cand,
                                 c_offsets, scores_out, topk_out, k, n_hits, stats);
    });
}

// ---------------------------------------------------------------------------
// reference-shaped replay (16-lane batches as alignment_fill_matrices gets them)
// ---------------------------------------------------------------------------
// The device route.  The batches go to the GPU as they are -- [max_len][16] table indices, copied end to end into
// pinned staging by all cores and from there in one transfer -- and the pair tokens are built from that image on the
// device: the two sequences of a pair are two adjacent lanes of one batch, so a row's two residues are two adjacent
// bytes (swg_build_tokens16_kernel).  Nothing is un-transposed or re-coded on the host, and nothing is allocated or
// freed per call once the buffers have grown to the size of the caller's macro-batches (round 2 rebuilt a whole
// database per call: 26-34 ms of host work and hipFree around 2.5 ms of device time).  Returns SWG_TAKE_HOST_ROUTE when
// the search cannot take this route (options that ask for an engine that reads the bin image, a query the work-queue kernels
// cannot hold): the caller falls back to the host route.
static int fill_batches16_device(swg_ctx *ctx, const swg_batch16 *batches, size_t n_batches, size_t n_records,
                                 const size_t *first_rec, double *fill_seconds, double *t_ms)
{
    typedef std::chrono::steady_clock clk;
    const clk::time_point t0 = clk::now();
    if (ctx->opt_engine == 1 || ctx->opt_dynamic == 0 || !ctx->have_scoring || ctx->query_len() == 0) return SWG_TAKE_HOST_ROUTE;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    SwgBatch16Cache &C = ctx->b16;
    // batches longest first (the reference's caller passes them sorted: then this is the identity)
    std::vector<uint32_t> bo(n_batches);
    for (size_t b = 0; b < n_batches; ++b) bo[b] = (uint32_t)b;
    bool sorted = true;
    for (size_t b = 1; b < n_batches && sorted; ++b) sorted = batches[b].max_len <= batches[b - 1].max_len;
    if (!sorted)
        std::stable_sort(bo.begin(), bo.end(), [&](uint32_t x, uint32_t y) { return batches[x].max_len > batches[y].max_len; });
    // sizes
    size_t n_pairs = 0;
    uint64_t stage_bytes = 0, total_blocks = 0, residues = 0, longest = 0;
    for (size_t b = 0; b < n_batches; ++b) {
        const swg_batch16 &bt = batches[b];
        if (bt.max_len > 0x3FFFFFFFull) return swg_set_ctx_error(ctx, SWG_ERR_ARG, "swg_fill_batches16: batch %zu too long", b);
        const size_t np = (bt.vector_size + 1) / 2;
        n_pairs += np;
        stage_bytes += (uint64_t)bt.max_len * 16u;
        total_blocks += (uint64_t)np * ((2ull + bt.max_len + 3) / 4);
        residues += (uint64_t)bt.vector_size * bt.max_len;
        longest = std::max<uint64_t>(longest, bt.max_len);
    }
    if (n_pairs >= (1ull << 31) || total_blocks + 1 >= (1ull << 32)) return SWG_TAKE_HOST_ROUTE;
    const size_t n_slots = (2 * n_pairs + SWG_BIN - 1) / SWG_BIN * SWG_BIN;
    // ---- buffers: grown, never shrunk ---------------------------------------------------------
    if (!C.db || n_slots > C.slots_cap || n_pairs > C.pairs_cap || total_blocks > C.blocks_cap || stage_bytes > C.stage_cap) {
        // The new capacities live in locals until EVERY allocation has succeeded: a failure half way leaves the cache
        // empty (capacities 0, no database), so the next call grows again instead of writing through NULL buffers.
        auto release = [&C]() {
            if (C.db) swg_db_free(C.db);
            C.db = nullptr;
            (void)hipHostFree(C.h_stage);
            (void)hipHostFree(C.h_meta);
            (void)hipFree(C.d_stage);
            (void)hipFree(C.d_pair_src);
            (void)hipFree(C.d_pair_len);
            C.h_stage = C.h_meta = nullptr;
            C.d_stage = nullptr;
            C.d_pair_src = nullptr;
            C.d_pair_len = nullptr;
        };
        auto grow = [](uint64_t need, uint64_t have) { return std::max<uint64_t>(need + need / 4 + 64, have); };
        const size_t slots_cap = (size_t)((grow(n_slots, C.slots_cap) + SWG_BIN - 1) / SWG_BIN * SWG_BIN);
        const size_t pairs_cap = (size_t)grow(n_pairs, C.pairs_cap);
        const uint64_t blocks_cap = grow(total_blocks, C.blocks_cap);
        const size_t stage_cap = (size_t)grow(stage_bytes, C.stage_cap);
        release();
        C.slots_cap = C.pairs_cap = C.stage_cap = 0;
        C.blocks_cap = 0;
        const int ra = [&]() -> int {
            swg_db *db = new (std::nothrow) swg_db();
            if (!db) return swg_set_ctx_error(ctx, SWG_ERR_NOMEM, "swg_fill_batches16: out of memory");
            C.db = db;
            db->tokens_only = true;
            db->device = ctx->device;
            db->n_bins = (uint32_t)(slots_cap / SWG_BIN); // (sizes the per-search output buffers)
            HIP_TRY(ctx, hipHostMalloc(reinterpret_cast<void **>(&C.h_stage), stage_cap, hipHostMallocDefault));
            HIP_TRY(ctx, hipHostMalloc(reinterpret_cast<void **>(&C.h_meta), pairs_cap * 16 + 8 + slots_cap * 8, hipHostMallocDefault));
            HIP_TRY(ctx, hipMalloc(&C.d_stage, stage_cap));
            HIP_TRY(ctx, hipMalloc(&C.d_pair_src, pairs_cap * 8));
            HIP_TRY(ctx, hipMalloc(&C.d_pair_len, pairs_cap * 4));
            HIP_TRY(ctx, hipMalloc(&db->d_codes, 16)); // (marks the database resident; there are no residue bytes by rank)
            HIP_TRY(ctx, hipMalloc(&db->d_lens, slots_cap * 4));
            HIP_TRY(ctx, hipMalloc(&db->d_order, slots_cap * 4));
            HIP_TRY(ctx, hipMalloc(&db->ptok.d_tok, (size_t)(blocks_cap + 1) * 16));
            HIP_TRY(ctx, hipMalloc(&db->ptok.d_pair_off, (pairs_cap + 1) * 4));
            return select_bufs(ctx, db, 0);
        }();
        if (ra != SWG_OK) {
            release();
            return ra;
        }
        C.slots_cap = slots_cap;
        C.pairs_cap = pairs_cap;
        C.blocks_cap = blocks_cap;
        C.stage_cap = stage_cap;
    }
    swg_db *db = C.db;
    // ---- this call's database: ranks 2p, 2p+1 = lanes 2i, 2i+1 of a batch --------------------------------
    uint64_t *pair_src = reinterpret_cast<uint64_t *>(C.h_meta);
    uint32_t *pair_len = reinterpret_cast<uint32_t *>(C.h_meta + C.pairs_cap * 8);
    uint32_t *h_lens = reinterpret_cast<uint32_t *>(C.h_meta + C.pairs_cap * 12);
    uint32_t *h_order = h_lens + C.slots_cap;
    try {
        db->lens.assign(n_slots, 0u);
        db->order.assign(n_slots, 0xFFFFFFFFu);
        db->ptok.pair_blocks_prefix.assign(n_pairs + 1, 0u);
    } catch (const std::exception &) {
        return swg_set_ctx_error(ctx, SWG_ERR_NOMEM, "swg_fill_batches16: out of host memory");
    }
    std::vector<uint64_t> stage_off(n_batches);
    {
        uint64_t so = 0;
        size_t p = 0;
        uint32_t blocks = 0;
        for (size_t k = 0; k < n_batches; ++k) {
            const size_t b = bo[k];
            const swg_batch16 &bt = batches[b];
            stage_off[b] = so;
            for (size_t i = 0; 2 * i < bt.vector_size; ++i, ++p) {
                const bool has_y = 2 * i + 1 < bt.vector_size;
                pair_src[p] = (so + 2 * i) | (has_y ? 0ull : 1ull << 63);
                pair_len[p] = (uint32_t)bt.max_len;
                db->lens[2 * p] = (uint32_t)bt.max_len;
                db->order[2 * p] = (uint32_t)(first_rec[b] + 2 * i);
                if (has_y) {
                    db->lens[2 * p + 1] = (uint32_t)bt.max_len;
                    db->order[2 * p + 1] = (uint32_t)(first_rec[b] + 2 * i + 1);
                }
                blocks += (uint32_t)((2ull + bt.max_len + 3) / 4);
                db->ptok.pair_blocks_prefix[p + 1] = blocks;
            }
            so += (uint64_t)bt.max_len * 16u;
        }
    }
    db->n_total = n_records;
    db->n_local = 2 * n_pairs; // (an odd batch's missing lane is an empty slot in the middle: pairs stay batch-aligned)
    db->n_bins = (uint32_t)(n_slots / SWG_BIN);
    db->residues = residues;
    db->max_nblk = (uint32_t)((longest + 3) / 4);
    db->rows_padded = 0;
    // one macro-batch has nothing to tell the next: plans and hints start afresh with the cache's database
    db->tuned.clear();
    db->pair_rows_prefix.clear(); // (the lengths changed under the same pair count)
    db->sat_hint = -1;
    db->f16_veto_epoch = 0;
    SwgPairTokens &T = db->ptok;
    T.tried = T.ok = true;
    T.total_blocks = total_blocks;
    memcpy(h_lens, db->lens.data(), n_slots * 4);
    memcpy(h_order, db->order.data(), n_slots * 4);
    t_ms[0] = std::chrono::duration<double, std::milli>(clk::now() - t0).count();
    const clk::time_point t1 = clk::now();
    hipStream_t s = ctx->stream;
    {
        // the batches into pinned staging by all cores, in runs of about 4 MB (in staging order): a run's transfer is
        // queued as soon as it is copied, so the upload of one run overlaps the copy of the next
        size_t k0 = 0;
        while (k0 < n_batches) {
            size_t k1 = k0;
            uint64_t bytes = 0;
            while (k1 < n_batches && bytes < (4u << 20)) bytes += (uint64_t)batches[bo[k1++]].max_len * 16u;
            const long long lo = (long long)k0, hi = (long long)k1;
            swg_stage_batches16(batches, bo.data(), stage_off.data(), (size_t)lo, (size_t)hi, C.h_stage); // all cores (swg_pack.cpp)
            const uint64_t from = stage_off[bo[k0]];
            HIP_TRY(ctx, hipMemcpyAsync(C.d_stage + from, C.h_stage + from, bytes, hipMemcpyHostToDevice, s));
            k0 = k1;
        }
    }
    t_ms[1] = std::chrono::duration<double, std::milli>(clk::now() - t1).count();
    const clk::time_point t2 = clk::now();
    HIP_TRY(ctx, hipMemcpyAsync(C.d_pair_src, pair_src, n_pairs * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(C.d_pair_len, pair_len, n_pairs * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(T.d_pair_off, T.pair_blocks_prefix.data(), (n_pairs + 1) * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(db->d_lens, h_lens, n_slots * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(db->d_order, h_order, n_slots * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemsetAsync(T.d_tok + total_blocks, 0, 16, s)); // the block of zeros behind the last pair
    uint32_t *d_bad = reinterpret_cast<uint32_t *>(db->d_codes);
    HIP_TRY(ctx, hipMemsetAsync(d_bad, 0, 4, s));
    HIP_TRY(ctx, swg_launch_build_tokens16(C.d_stage, C.d_pair_src, C.d_pair_len, T.d_pair_off, (uint32_t)n_pairs, total_blocks,
                                           T.d_tok, d_bad, s));
    // ---- the search itself (the cost model's geometry: this database is searched once) ----------------------
    swg_stats st;
    int rc = search_begin(ctx, db, true, 0, false, &ctx->slots[0]);
    if (rc == SWG_OK) {
        ctx->slots[0].busy = true;
        // (scores by record index: straight from the slot's pinned landing buffer, no int32 array in between)
        rc = search_end(ctx, &ctx->slots[0], nullptr, nullptr, nullptr, &st);
        ctx->slots[0].busy = false;
    }
    if (rc != SWG_OK) return rc; // (SWG_TAKE_HOST_ROUTE from the search itself: it needs what this database does not have)
    uint32_t bad = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, spin_sync(ctx, s));
    if (bad) return swg_set_ctx_error(ctx, SWG_ERR_RESIDUE, "swg_fill_batches16: residue index outside 1..31 in a batch");
    t_ms[2] = std::chrono::duration<double, std::milli>(clk::now() - t2).count();
    const clk::time_point t3 = clk::now();
    const int32_t *hs = ctx->slots[0].h_scores;
    {
        size_t p = 0;
        for (size_t k = 0; k < n_batches; ++k) {
            const swg_batch16 &bt = batches[bo[k]];
            for (size_t i = 0; 2 * i < bt.vector_size; ++i, ++p) {
                bt.max_scores[2 * i] = (int16_t)std::min<int32_t>(hs[2 * p], INT16_MAX);
                if (2 * i + 1 < bt.vector_size) bt.max_scores[2 * i + 1] = (int16_t)std::min<int32_t>(hs[2 * p + 1], INT16_MAX);
            }
        }
    }
    t_ms[3] = std::chrono::duration<double, std::milli>(clk::now() - t3).count();
    t_ms[4] = st.total_ms;
    if (fill_seconds) *fill_seconds = st.total_ms * 1e-3;
    return SWG_OK;
}

static int fill_batches16_impl(swg_ctx *ctx, const swg_batch16 *batches, size_t n_batches, double *fill_seconds);

extern "C" int swg_fill_batches16(swg_ctx *ctx, const swg_batch16 *batches, size_t n_batches,
                                  double *fill_seconds)
{
    try { // no C++ exception crosses the ABI
        return fill_batches16_impl(ctx, batches, n_batches, fill_seconds);
    } catch (const std::bad_alloc &) {
        return swg_set_ctx_error(ctx, SWG_ERR_NOMEM, "swg_fill_batches16: out of host memory");
    } catch (const std::exception &e) {
        return swg_set_ctx_error(ctx, SWG_ERR_NOMEM, "swg_fill_batches16: %s", e.what());
    }
}

static int fill_batches16_impl(swg_ctx *ctx, const swg_batch16 *batches, size_t n_batches, double *fill_seconds)
{
    if (!ctx || (!batches && n_batches))
        return swg_set_ctx_error(ctx, SWG_ERR_ARG, "swg_fill_batches16: NULL argument");
    if (fill_seconds) *fill_seconds = 0.0;
    // diagnostics: SWG_TIMING=1 prints where the wall time of this call went
    static const bool timing = getenv("SWG_TIMING") != nullptr;
    typedef std::chrono::steady_clock clk;
    clk::time_point tp[8];
    tp[0] = clk::now();
    std::vector<uint64_t> offsets(1, 0);
    std::vector<size_t> first_rec(n_batches);
    try {
        for (size_t b = 0; b < n_batches; ++b) {
            if (!batches[b].db_idx_t || !batches[b].max_scores || batches[b].vector_size > 16 ||
                batches[b].max_len == 0)
                return swg_set_ctx_error(ctx, SWG_ERR_ARG, "swg_fill_batches16: bad batch %zu", b);
            first_rec[b] = offsets.size() - 1;
            // lane l, padded rows included: the reference computes them as real
            // rows (src/alignment_cmdline.c:448-450)
            for (size_t l = 0; l < batches[b].vector_size; ++l) offsets.push_back(offsets.back() + batches[b].max_len);
        }
    } catch (const std::exception &) {
        return swg_set_ctx_error(ctx, SWG_ERR_NOMEM, "swg_fill_batches16: out of host memory");
    }
    const size_t n_all = offsets.size() - 1;
    if (n_all == 0) return SWG_OK;
    // one rule for both routes (the device route searches on slot 0 with the cache's one database; the host route used to
    // slip past a ticket on another slot)
    for (const SwgSlot &sl : ctx->slots)
        if (sl.busy) return swg_set_ctx_error(ctx, SWG_ERR_STATE, "swg_fill_batches16: searches are in flight on this context");
    {
        double t_ms[5] = {0, 0, 0, 0, 0};
        int rd = SWG_OK;
        try {
            rd = fill_batches16_device(ctx, batches, n_batches, n_all, first_rec.data(), fill_seconds, t_ms);
        } catch (const std::exception &) {
            return swg_set_ctx_error(ctx, SWG_ERR_NOMEM, "swg_fill_batches16: out of host memory");
        }
        if (rd != SWG_TAKE_HOST_ROUTE) {
            if (rd == SWG_OK && timing)
                fprintf(stderr, "[swg_fill_batches16] %zu records, device route: tables %.2f ms, staging copy %.2f, upload + tokens + search + "
                                "read-out %.2f (device, first kernel to last: %.2f), scores to the batches %.2f; wall %.2f\n",
                        n_all, t_ms[0], t_ms[1], t_ms[2], t_ms[4], t_ms[3],
                        std::chrono::duration<double, std::milli>(clk::now() - tp[0]).count());
            return rd;
        }
    }
    // the host route (searches the device route cannot take: engine = 1, work_queue = 0, what needs the bin image)
    std::unique_ptr<int8_t[]> flat(new (std::nothrow) int8_t[std::max<uint64_t>(1, offsets.back())]);
    if (!flat) return swg_set_ctx_error(ctx, SWG_ERR_NOMEM, "swg_fill_batches16: out of host memory");
    swg_untranspose_batches16(batches, n_batches, first_rec.data(), offsets.data(), flat.get());
    tp[1] = clk::now();
    const size_t n = offsets.size() - 1;
    if (n == 0) return SWG_OK;
    swg_db *db = nullptr;
    int rc = swg_db_pack(flat.get(), offsets.data(), n, 0, 1, &db);
    if (rc != SWG_OK) {
        // (the packer speaks of a database: the caller handed over batches, and the device route says so)
        if (rc == SWG_ERR_RESIDUE) return swg_set_ctx_error(ctx, SWG_ERR_RESIDUE, "swg_fill_batches16: residue index outside 1..31 in a batch");
        ctx->err = swg_global_error();
        return rc;
    }
    tp[2] = clk::now();
    rc = swg_db_upload(ctx, db);
    tp[3] = clk::now();
    std::vector<int32_t> scores;
    try {
        scores.assign(n, 0);
    } catch (const std::exception &) {
        swg_db_free(db);
        return swg_set_ctx_error(ctx, SWG_ERR_NOMEM, "swg_fill_batches16: out of host memory");
    }
    swg_stats st;
    // (this database is searched exactly once: the cost model's geometry, no timed trials)
    if (rc == SWG_OK) rc = search_now(ctx, db, false, scores.data(), nullptr, 0, nullptr, &st);
    tp[4] = clk::now();
    swg_db_free(db);
    tp[5] = clk::now();
    if (rc != SWG_OK) return rc;
    size_t i = 0;
    for (size_t b = 0; b < n_batches; ++b)
        for (size_t l = 0; l < batches[b].vector_size; ++l, ++i)
            batches[b].max_scores[l] = (int16_t)std::min<int32_t>(scores[i], INT16_MAX);
    if (fill_seconds) *fill_seconds = st.total_ms * 1e-3;
    if (timing) {
        auto ms = [&](int i) { return std::chrono::duration<double, std::milli>(tp[i + 1] - tp[i]).count(); };
        fprintf(stderr, "[swg_fill_batches16] %zu records: un-transpose %.2f ms, pack %.2f, upload %.2f, search %.2f (device %.2f), free %.2f\n",
                n, ms(0), ms(1), ms(2), ms(3), st.total_ms, ms(4));
    }
    return SWG_OK;
}
