// C-ABI implementation (include/joxsz_hip.h) for gfx950, the one translation unit of the library: the C entry points, uploads, the
// table building of jx_finalize (finalize_impl and its steps), the per-chunk dispatcher (run_chunk) with the per-walker kernel launch and
// the operator route, the sampler, RCCL and the bandwidth / timing utilities.  The context and the host side of each back end are
// headers included here: jx_ctx.hpp, jx_host_exact.hpp (plan_exact, exact_setup, run_exact), jx_host_mix.hpp (plan_mix, mix_setup, run_mix,
// the truncation guard), jx_host_fft.hpp (fft_setup, run_fft).
// The SZ side of the log-posterior (joxsz_funcs.py:457-472) behind the Compton-y profile:
//   * the exact form (jx_exact.hpp; default since round 5): the spline, the map, the beam convolution, the transfer function and the row
//     extraction as ONE constant operator on the spline ordinates, built on the host at jx_finalize (jx_tables.hpp: every pixel, every
//     radius, nothing truncated) -- per step: jx_walker2_kernel -> jx_ordrow_kernel -> jx_rowsum_tail_kernel;
//   * the contracted forms of rounds 3-4 (jx_mix.hpp; option JOXSZ_MIX_FORM=legacy|lowrank|full, kept for one round): low-rank (stage 1 on
//     the vector units + stage 2 on the matrix cores) or full (one matrix-core product fed by the sample evaluation), with their
//     truncation guard;
//   * the literal sequence, "rocFFT sequence" below (forward transforms -> beam multiply -> inverse -> window -> forward transforms, on the
//     hand-written LDS transforms of jx_fft.hpp or on rocFFT's plans): the reference's lines executed pass by pass -- the
//     independent cross-check, the fallback for inputs without the mirror structure, and, as a small reference facility inside every other
//     context, the source of the beam-convolved-map tap and of jx_audit.
// Every switch is an option of the context (jx_set_option; the process environment is the default of each name), read once, in
// jx_finalize; nothing on the launch path calls getenv.
#include <dlfcn.h>
#include <unistd.h>

#include <cctype>

#include "jx_ctx.hpp"

static int g_rocfft_refs = 0;

static size_t tensor_bytes(const jx_config& c, int id) {
    const size_t f = sizeof(double);
    switch (id) {
        case JX_T_R_PP: return f * c.N;
        case JX_T_D_MAT: return f * (size_t)c.S * c.S;
        case JX_T_BEAM_2D: return f * (size_t)c.B * c.B;
        case JX_T_FILTERING: return f * (size_t)c.S * c.S;
        case JX_T_RADIUS: return f * c.S;
        case JX_T_FLUX_DATA: return f * 3 * c.nflux;
        case JX_T_CONV_T: case JX_T_CONV_V: return f * c.nconv;
        case JX_T_PAR_VALS: case JX_T_PAR_MIN: case JX_T_PAR_MAX: case JX_T_PAR_MU: case JX_T_PAR_SIGMA:
            return f * c.npar;
        case JX_T_PAR_KIND: return sizeof(int32_t) * c.npar;
        case JX_T_THAWED_IDX: return sizeof(int32_t) * c.ndim;
        case JX_T_X_R_NE: case JX_T_X_R_T: case JX_T_GEOMAREA: return f * c.nann;
        case JX_T_PROJVOLS: return f * (size_t)c.nann * c.nann;
        case JX_T_CTS: case JX_T_AREASCALES: case JX_T_EXPOSURES: case JX_T_BACKRATES:
            return f * (size_t)c.nband * c.nann;
        case JX_T_LNT: return f * c.ntab;
        case JX_T_LNRATE: return f * (size_t)c.nband * 2 * c.ntab;
        case JX_T_INTEG_W: return f * ((size_t)c.N + 1);
    }
    return 0;
}

static bool tensor_is_xray(int id) { return id >= JX_T_X_R_NE && id <= JX_T_LNRATE; }

// librccl, loaded on first use (dlopen): the functions of the all-gather path only
namespace {
struct RcclApi {
    void* h = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*CommCount)(const ncclComm_t, int*) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    std::string err;
};
RcclApi g_rccl;
std::string g_last_global_error;       // failures of calls that have no context (jx_comm_unique_id)

bool rccl_load() {
    if (g_rccl.h) return true;
    void* h = nullptr;
    std::string why;
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
        h = dlopen(name, RTLD_NOW | RTLD_LOCAL);
        if (h) break;
        const char* e = dlerror();                              // (one call: it clears the error it returns)
        why = std::string(name) + ": " + (e ? e : "unknown error");
    }
    if (!h) { g_rccl.err = "dlopen(librccl): " + why; return false; }
    RcclApi api;
    bool ok = true;
#define JX_SYM(field, sym) if (ok) { *(void**)(&api.field) = dlsym(h, sym); if (!api.field) { g_rccl.err = std::string("librccl lacks ") + sym; ok = false; } }
    JX_SYM(GetUniqueId, "ncclGetUniqueId") JX_SYM(CommInitRank, "ncclCommInitRank") JX_SYM(AllGather, "ncclAllGather")
    JX_SYM(AllReduce, "ncclAllReduce") JX_SYM(CommCount, "ncclCommCount") JX_SYM(CommDestroy, "ncclCommDestroy") JX_SYM(GetErrorString, "ncclGetErrorString")
#undef JX_SYM
    if (!ok) { dlclose(h); return false; }
    api.h = h;
    g_rccl = api;
    return true;
}
}  // namespace

#define NCCLCHK(ctx, call)                                                                         \
    do {                                                                                           \
        ncclResult_t r_ = (call);                                                                  \
        if (r_ != ncclSuccess) {                                                                   \
            (ctx)->err = std::string(#call) + ": " + g_rccl.GetErrorString(r_);                    \
            return JX_ERR_COMM;                                                                    \
        }                                                                                          \
    } while (0)

// ---------------------------------------------------------------------------------------------------------------------
// Abel + map kernel launches (jx_abel_map_sym_kernel / jx_abel_map_kernel): full map, quadrant, or phases 1-3 only
// ---------------------------------------------------------------------------------------------------------------------
static size_t map_lds_need(const JxDev& d, int threads) {
    const int N = d.N, S = d.S;
    size_t scratch = (d.pairw == 2) ? JX_MAP_SCRATCH2_DOUBLES(N) : JX_MAP_SCRATCH_DOUBLES(N);
    if (d.fast_map) scratch = std::max(scratch, (size_t)(threads / 64) * ((S + 3) & ~1));
    const size_t dbl = JX_MAP_FIXED_DOUBLES(N) + scratch + (d.pairw == 2 ? 4 * JX_MAP_NE(N) + 8 : 0);
    return dbl * sizeof(double);
}

// picks pairw and the block size for `d` so that the kernel's LDS fits; returns false when the radial grid is too long
static bool map_geometry(JxDev& d, int want_threads, int* threads_out, size_t* lds_out, bool pair_full) {
    const size_t LDS_MAX = 160 * 1024;
    int threads = want_threads;
    d.pairw = 1;
    if (d.quad) {
        d.pairw = 2;                                           // two walkers per block share every table entry, while two such blocks fit a CU
        if (map_lds_need(d, threads) > (LDS_MAX - 2048) / 2) d.pairw = 1;
    } else if (pair_full && d.fast_map) {
        // full rows: two walkers per block take the Abel weights out of the L2 once (2 MB per walker otherwise: the stream
        // that competes with the map's stores); one such block per CU
        d.pairw = 2;
        if (map_lds_need(d, threads) > LDS_MAX - 1024) d.pairw = 1;
    }
    while (threads > 64 && map_lds_need(d, threads) > LDS_MAX - 1024) threads /= 2;
    const size_t lds = map_lds_need(d, threads);
    if (lds > LDS_MAX - 1024) return false;
    *threads_out = threads; *lds_out = lds;
    return true;
}

static void launch_map(hipStream_t st, const JxDev& dm_in, int threads, size_t lds, const double* theta_dev, int w0, int n, double* img,
                       double* tpp, double* tab, double* ty, bool coef_only) {
    JxDev dm = dm_in;
    dm.nlaunch = n;
    const bool vec2 = (dm.S % 2 == 0) && (dm.img_ld % 2 == 0);
    const int npw = (dm.pairw == 2) ? 2 : 1;
    if (coef_only) dm.map_split = 1;
    const dim3 grid(((n + npw - 1) / npw) * dm.map_split), block(threads);
    if (dm.fast_map) {
        const int nait = (dm.q_na + 63) / 64;
#define JX_SYM_LAUNCH(V, NA) hipLaunchKernelGGL((jx_abel_map_sym_kernel<V, NA>), grid, block, lds, st, dm, theta_dev, w0, img, tpp, tab, ty)
        if (vec2) { if (nait <= 3) JX_SYM_LAUNCH(true, 3); else if (nait <= 5) JX_SYM_LAUNCH(true, 5); else JX_SYM_LAUNCH(true, 9); }
        else      { if (nait <= 3) JX_SYM_LAUNCH(false, 3); else if (nait <= 5) JX_SYM_LAUNCH(false, 5); else JX_SYM_LAUNCH(false, 9); }
#undef JX_SYM_LAUNCH
    } else {
        if (vec2) hipLaunchKernelGGL(jx_abel_map_kernel<true>, grid, block, lds, st, dm, theta_dev, w0, img, tpp, tab, ty);
        else hipLaunchKernelGGL(jx_abel_map_kernel<false>, grid, block, lds, st, dm, theta_dev, w0, img, tpp, tab, ty);
    }
}

// the Compton-y map tap of the exact and contracted forms: the quadrant of distinct pixels
static int launch_y2d(jx_ctx* ctx, const Chunk& c) {
    int rc;
    if (!ctx->d_img && (rc = dev_new(ctx, (size_t)ctx->chunk * c.d.img_ws, &ctx->d_img, true))) return rc;
    launch_map(c.st, ctx->d, ctx->map_threads, ctx->map_lds, c.theta, c.w0, c.n, ctx->d_img, nullptr, nullptr, nullptr, false);
    return JX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Per-walker kernel (jx_walker2_kernel / jx_prep_kernel): priors, vetoes, pressure profile, X-ray side, conversion factors
// ---------------------------------------------------------------------------------------------------------------------
// two blocks per walker (the X-ray side beside the rest): the timed sequence of the exact and contracted forms only
// (up to ~640 radii: beyond, the grid pass on half the threads is the longer of the two chains by more than the split saves --
//  measured at N = 1000: 32.5 -> 34.7 us; at N = 500: 27.6 -> 23.4, at N = 313: 26.8 -> 22.3)
static bool prep_splits(const jx_ctx* ctx, const Chunk& c) {
    const JxDev& d = c.d;
    return ctx->prep_split && !c.t.any() && !d.sz_only && !d.prep_pow && !d.calc_integ /* (its sums are grouped by the block's size) */ && 3 * d.nann <= 128 && d.nband * d.nann <= 4096 && d.N <= 640;
}

#ifdef JOXSZ_ABLATIONS
// diagnostic build only (JOXSZ_P_STAMPS): wall-clock stamps of the per-walker kernel's phases, printed once, at the 40th launch
static void prep_stamps(hipStream_t ps, int n, bool xr_split, JxDev& dp) {
    static long long* stamps = nullptr;
    if (!stamps) { (void)hipMalloc((void**)&stamps, sizeof(long long) * 8 * 65536); (void)hipMemset(stamps, 0, sizeof(long long) * 8 * 65536); }
    dp.stamps = stamps;
    static int calls = 0;
    if (++calls != 40) return;
    (void)hipStreamSynchronize(ps);
    const int nb = xr_split ? 2 * n : n;
    std::vector<long long> h((size_t)nb * 8);
    (void)hipMemcpy(h.data(), stamps, sizeof(long long) * h.size(), hipMemcpyDeviceToHost);
    long long t0 = h[0];
    for (int b = 0; b < nb; ++b) t0 = std::min(t0, h[(size_t)b * 8]);
    for (int half = 0; half < (xr_split ? 2 : 1); ++half) {
        const int b0 = half * n, b1 = b0 + n;
        double mx[7] = {0}, sm[7] = {0};
        for (int b = b0; b < b1; ++b)
            for (int k = 0; k < 7; ++k) { const double v = h[(size_t)b * 8 + k] ? (h[(size_t)b * 8 + k] - t0) * 0.01 : 0.0; mx[k] = std::max(mx[k], v); sm[k] += v / n; }
        fprintf(stderr, "prep stamps, %s blocks (us after the first start; mean/max): start %.2f/%.2f params %.2f/%.2f priors %.2f/%.2f grid pass %.2f/%.2f veto+integ %.2f/%.2f factors %.2f/%.2f end %.2f/%.2f\n",
                half ? "X-ray" : (xr_split ? "SZ-side" : "all"), sm[0], mx[0], sm[1], mx[1], sm[2], mx[2], sm[3], mx[3], sm[4], mx[4], sm[5], mx[5], sm[6], mx[6]);
    }
}
#endif

// ps: the stream (the chunk's, or the side stream of the contracted forms); pp_buf: where the pressure profiles go (null: nowhere), in rows
// of pp_ld doubles (0: N); ncf: conversion factors up to the outputs this launch's consumers read (the lean form; every other all of them)
static void launch_prep(jx_ctx* ctx, const Chunk& c, hipStream_t ps, double* pp_buf, int pp_ld, int ncf) {
    const JxDev& d = c.d;
    const Taps& t = c.t;
    const int n = c.n;
    JxDev dp = d;
    dp.inject_pp = ctx->d.inject_pp;
    dp.xr_split = c.xr_split ? 1 : 0;
    dp.xr_out = ctx->d_xr;
    dp.pp_ld = pp_ld;
#ifdef JOXSZ_ABLATIONS
    if (opt_str(ctx, "JOXSZ_P_STAMPS")) prep_stamps(ps, n, c.xr_split, dp);
#endif
    const unsigned pgrid = c.xr_split ? 2u * (unsigned)n : (unsigned)n, pthr = c.xr_split ? 128u : (unsigned)JX_PREP_THREADS;
    if (c.xr_split && ctx->prep_lean && ctx->prep_fastmath && pp_buf && sizeof(double) * JX_W2_LDS_DOUBLES(d) <= (size_t)19 * 1024 + 512 &&
        d.N <= JX_W2_RPL * JX_W2_THREADS && 3 * d.nann <= JX_W2_THREADS) {
        // the two-block form as two lean roles (same arithmetic, same bits; every table of a role in one batched copy into LDS, a lane's radii in registers)
        hipLaunchKernelGGL(jx_walker2_kernel, dim3(pgrid), dim3(JX_W2_THREADS), sizeof(double) * JX_W2_LDS_DOUBLES(d), ps, dp, c.theta, c.w0, c.base, c.cfac, pp_buf, ncf, c.sm);
        return;
    }
    const size_t sh = sizeof(double) * (JX_LDS_HDR + (size_t)2 * d.N + 2 * d.nann + 2 * (size_t)d.nband * d.nann + 2 * (size_t)d.nconv + 8 + JX_FM_TABLE_DOUBLES);
    if (d.prep_pow) hipLaunchKernelGGL((jx_prep_kernel<true, false>), dim3(pgrid), dim3(pthr), sh, ps, dp, c.theta, c.w0,
                                       c.base, c.cfac, pp_buf, c.sz0, t.tprof, t.xprofs, t.parts, t.integ, c.sm);
    else if (ctx->prep_fastmath) hipLaunchKernelGGL((jx_prep_kernel<false, true>), dim3(pgrid), dim3(pthr), sh, ps, dp, c.theta, c.w0,
                                                    c.base, c.cfac, pp_buf, c.sz0, t.tprof, t.xprofs, t.parts, t.integ, c.sm);
    else hipLaunchKernelGGL((jx_prep_kernel<false, false>), dim3(pgrid), dim3(pthr), sh, ps, dp, c.theta, c.w0,
                            c.base, c.cfac, pp_buf, c.sz0, t.tprof, t.xprofs, t.parts, t.integ, c.sm);
}

#include "jx_host_fft.hpp"
#include "jx_host_mix.hpp"
#include "jx_host_exact.hpp"

extern "C" {

int jx_comm_unique_id(void* id_out) {
    if (!id_out) return JX_ERR_INVALID;
    if (!rccl_load()) { g_last_global_error = g_rccl.err; return JX_ERR_COMM; }
    ncclUniqueId id;
    const ncclResult_t r = g_rccl.GetUniqueId(&id);
    if (r != ncclSuccess) { g_last_global_error = std::string("ncclGetUniqueId: ") + g_rccl.GetErrorString(r); return JX_ERR_COMM; }
    static_assert(sizeof(id) == JX_COMM_ID_BYTES, "id size");
    memcpy(id_out, &id, sizeof(id));
    return JX_OK;
}

int jx_comm_init_rank(jx_ctx* ctx, const void* idp, int nranks, int rank) {
    if (!ctx || !idp || nranks < 1 || rank < 0 || rank >= nranks) return JX_ERR_INVALID;
    if (ctx->comm) { ctx->err = "jx_comm_init_rank: this context already has a communicator"; return JX_ERR_STATE; }
    if (!rccl_load()) { ctx->err = g_rccl.err; return JX_ERR_COMM; }
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    ncclUniqueId id;
    memcpy(&id, idp, sizeof(id));
    // RCCL prints a version banner on stdout when its first communicator comes up; a caller whose stdout is a protocol
    // (bench.py: one JSON line) must not see it, so file descriptor 1 points at stderr for the duration of the call
    fflush(stdout);
    const int saved = dup(1);
    if (saved >= 0) dup2(2, 1);
    const ncclResult_t r0 = g_rccl.CommInitRank(&ctx->comm, nranks, id, rank);
    fflush(stdout);
    if (saved >= 0) { dup2(saved, 1); close(saved); }
    NCCLCHK(ctx, r0);
    ctx->comm_rank = rank; ctx->comm_size = nranks;
    return JX_OK;
}

int jx_comm_count(jx_ctx* ctx) {
    if (!ctx) return JX_ERR_INVALID;
    if (!ctx->comm) { ctx->err = "jx_comm_count before jx_comm_init_rank"; return JX_ERR_STATE; }
    int n = 0;
    NCCLCHK(ctx, g_rccl.CommCount(ctx->comm, &n));
    return n;
}

static int gather_drain(jx_ctx* ctx) {
    for (auto& pr : ctx->gt_inflight) {
        HIPCHK(ctx, hipEventSynchronize(pr.second));
        float ms = 0.f;
        HIPCHK(ctx, hipEventElapsedTime(&ms, pr.first, pr.second));
        ctx->gather_ms += ms; ctx->gather_calls += 1;
        ctx->gt_free.push_back(pr);
    }
    ctx->gt_inflight.clear();
    return JX_OK;
}

// the stream the communicator's collectives run on; in overlap mode it first waits for everything enqueued on the compute stream so far
static int comm_fork(jx_ctx* ctx, hipStream_t* out) {
    if (!ctx->comm_overlap) { *out = ctx->stream; return JX_OK; }
    HIPCHK(ctx, hipEventRecord(ctx->ev_fork, ctx->stream));
    HIPCHK(ctx, hipStreamWaitEvent(ctx->comm_stream, ctx->ev_fork, 0));
    *out = ctx->comm_stream;
    return JX_OK;
}

int jx_comm_set_overlap(jx_ctx* ctx, int on) {
    if (!ctx) return JX_ERR_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->comm_stream) HIPCHK(ctx, hipStreamSynchronize(ctx->comm_stream));
    if (on && !ctx->comm_stream) {
        HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->comm_stream, hipStreamNonBlocking));
        HIPCHK(ctx, hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming));
        for (auto& g : ctx->gslot) HIPCHK(ctx, hipEventCreateWithFlags(&g.done, hipEventDisableTiming));
    }
    for (auto& g : ctx->gslot) g.busy = false;
    ctx->comm_overlap = on != 0;
    return JX_OK;
}

int jx_allgather_logp(jx_ctx* ctx, const double* send_dev, double* recv_dev, int count) {
    if (!ctx || !send_dev || !recv_dev || count < 0) return JX_ERR_INVALID;
    if (!ctx->comm) { ctx->err = "jx_allgather_logp before jx_comm_init_rank"; return JX_ERR_STATE; }
    if (count == 0) return JX_OK;
    int rc;
    hipStream_t cs;
    if ((rc = comm_fork(ctx, &cs))) return rc;
    std::pair<hipEvent_t, hipEvent_t> pr{nullptr, nullptr};
    const bool timed = ctx->timing_on && ctx->timing_mode == 1;    // (the stage pass; the timed region of bench.py carries no events of the gather)
    if (timed) {
        if (ctx->gt_inflight.size() > 4096 && (rc = gather_drain(ctx))) return rc;
        if (!ctx->gt_free.empty()) { pr = ctx->gt_free.back(); ctx->gt_free.pop_back(); }
        else { HIPCHK(ctx, hipEventCreate(&pr.first)); HIPCHK(ctx, hipEventCreate(&pr.second)); }
        HIPCHK(ctx, hipEventRecord(pr.first, cs));
    }
    NCCLCHK(ctx, g_rccl.AllGather(send_dev, recv_dev, (size_t)count, ncclDouble, ctx->comm, cs));
    if (timed) { HIPCHK(ctx, hipEventRecord(pr.second, cs)); ctx->gt_inflight.push_back(pr); }
    if (ctx->comm_overlap) {
        // remember the send buffer: the next evaluation that writes it waits for this gather (run_chunk), nothing else does
        jx_ctx::GatherSlot* slot = nullptr;
        for (auto& g : ctx->gslot) if (g.busy && g.send == (const char*)send_dev) slot = &g;
        if (!slot) for (auto& g : ctx->gslot) if (!g.busy) { slot = &g; break; }
        if (!slot) {                                                 // every slot taken: retire the oldest by waiting for it on the compute stream
            slot = &ctx->gslot[0];
            HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, slot->done, 0));
        }
        slot->send = (const char*)send_dev; slot->bytes = sizeof(double) * (size_t)count; slot->busy = true;
        HIPCHK(ctx, hipEventRecord(slot->done, cs));
    }
    return JX_OK;
}

int jx_comm_allreduce_max(jx_ctx* ctx, double* inout_dev, int count) {
    if (!ctx || !inout_dev || count < 1) return JX_ERR_INVALID;
    if (!ctx->comm) { ctx->err = "jx_comm_allreduce_max before jx_comm_init_rank"; return JX_ERR_STATE; }
    int rc;
    hipStream_t cs;
    if ((rc = comm_fork(ctx, &cs))) return rc;
    NCCLCHK(ctx, g_rccl.AllReduce(inout_dev, inout_dev, (size_t)count, ncclDouble, ncclMax, ctx->comm, cs));
    if (ctx->comm_overlap) {                                         // the result is awaited on the compute stream, as in strict mode
        HIPCHK(ctx, hipEventRecord(ctx->ev_fork, cs));
        HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_fork, 0));
    }
    return JX_OK;
}

int jx_comm_gather_time(jx_ctx* ctx, double* ms_total, int64_t* calls) {
    if (!ctx || !ms_total || !calls) return JX_ERR_INVALID;
    int rc = gather_drain(ctx);
    if (rc) return rc;
    *ms_total = ctx->gather_ms; *calls = ctx->gather_calls;
    ctx->gather_ms = 0.0; ctx->gather_calls = 0;
    return JX_OK;
}

int jx_comm_destroy(jx_ctx* ctx) {
    if (!ctx) return JX_ERR_INVALID;
    if (!ctx->comm) return JX_OK;
    (void)hipStreamSynchronize(ctx->stream);
    if (ctx->comm_stream) (void)hipStreamSynchronize(ctx->comm_stream);
    NCCLCHK(ctx, g_rccl.CommDestroy(ctx->comm));
    ctx->comm = nullptr; ctx->comm_rank = 0; ctx->comm_size = 1;
    return JX_OK;
}

const char* jx_strerror(int s) {
    switch (s) {
        case JX_OK: return "ok";
        case JX_ERR_INVALID: return "invalid argument";
        case JX_ERR_STATE: return "call out of order";
        case JX_ERR_MISSING: return "required tensor not uploaded";
        case JX_ERR_HIP: return "HIP runtime error";
        case JX_ERR_ROCFFT: return "rocFFT error";
        case JX_ERR_NOMEM: return "out of memory";
        case JX_ERR_NODEVICE: return "no usable HIP device";
        case JX_ERR_UNSUPPORTED: return "unsupported size";
        case JX_ERR_COMM: return "RCCL error";
    }
    return "unknown status";
}

const char* jx_last_error(jx_ctx* ctx) { return ctx ? ctx->err.c_str() : g_last_global_error.c_str(); }

int jx_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char* jx_device_name(jx_ctx* ctx) { return ctx ? ctx->devname.c_str() : ""; }

int jx_create(const jx_config* cfg, jx_ctx** out) {
    if (!cfg || !out) return JX_ERR_INVALID;
    *out = nullptr;
    if (cfg->abi_version != JX_ABI_VERSION) return JX_ERR_INVALID;
    const jx_config& c = *cfg;
    if (c.S < 7 || c.N < 4 || c.B < 1 || (c.B % 2) == 0 || c.nflux < 1 || c.nconv < 2) return JX_ERR_INVALID;
    if (c.npar != 16 && c.npar != 19) return JX_ERR_INVALID;
    if ((c.ne_mode == 1) != (c.npar == 19)) return JX_ERR_INVALID;
    if (c.ndim < 1 || c.ndim > c.npar) return JX_ERR_INVALID;
    if (!c.sz_only && (c.nann < 1 || c.nband < 1 || c.ntab < 2)) return JX_ERR_INVALID;
    if (c.N < c.S - c.S / 2) return JX_ERR_INVALID;       // r_pp[:nrow-1] must exist (joxsz_funcs.py:469)
    if (!(c.step > 0) || !(c.kpc_as > 0) || !(c.m_e > 0) || !(c.sigma_T > 0) || !(c.kpc_cm > 0)) return JX_ERR_INVALID;
    if (c.nann > 64 || c.nband > 64 || c.N > 4096 || c.S > 4096) return JX_ERR_UNSUPPORTED;
    if (c.dtype < 0 || c.dtype > 3) return JX_ERR_INVALID;
    if (c.calc_integ && !(c.integ_sig > 0)) return JX_ERR_INVALID;

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return JX_ERR_NODEVICE;
    if (c.device < 0 || c.device >= ndev) return JX_ERR_NODEVICE;

    jx_ctx* ctx = new (std::nothrow) jx_ctx();
    if (!ctx) return JX_ERR_NOMEM;
    ctx->cfg = c;
    ctx->host.resize(JX_T_COUNT);
    ctx->have.assign(JX_T_COUNT, false);
    if (hipSetDevice(c.device) != hipSuccess) { delete ctx; return JX_ERR_NODEVICE; }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, c.device) != hipSuccess) { delete ctx; return JX_ERR_NODEVICE; }
    ctx->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    ctx->devname = std::string(prop.name[0] ? prop.name : "AMD GPU") + " (" + prop.gcnArchName + ", " + std::to_string(prop.multiProcessorCount) + " CUs)";
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) { delete ctx; return JX_ERR_HIP; }
    ctx->own_stream = ctx->stream;
    if (g_rocfft_refs++ == 0) rocfft_setup();
    *out = ctx;
    return JX_OK;
}

int jx_upload(jx_ctx* ctx, int id, const void* host, size_t nbytes) {
    if (!ctx || !host) return JX_ERR_INVALID;
    if (ctx->finalized) { ctx->err = "jx_upload after jx_finalize"; return JX_ERR_STATE; }
    if (id < 0 || id >= JX_T_COUNT) return JX_ERR_INVALID;
    const size_t want = tensor_bytes(ctx->cfg, id);
    if (nbytes != want) {
        ctx->err = "tensor " + std::to_string(id) + ": got " + std::to_string(nbytes) + " bytes, expected " + std::to_string(want);
        return JX_ERR_INVALID;
    }
    ctx->host[id].assign((const unsigned char*)host, (const unsigned char*)host + nbytes);
    ctx->have[id] = true;
    return JX_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------
// jx_finalize: the steps of finalize_impl, in the order it calls them
// ---------------------------------------------------------------------------------------------------------------------
#define JX_LR_TOL_DEFAULT 1e-8
#define JX_PRUNE_TOL 1e-22            // weights of the data-radii spline below this fraction of the largest are not read (an fp64 sum cannot see them)

// does d_mat have the mirror structure d_mat[iy][ix] = Q[|iy-c|][|ix-c|] (what centdistmat builds)?  Q: the quadrant table
static void mirror_quadrant(jx_ctx* ctx) {
    const int S = ctx->cfg.S;
    std::vector<double> dm_h = host_vec<double>(ctx, JX_T_D_MAT);
    const int cc0 = S / 2, qn = std::max(cc0, S - 1 - cc0) + 1;
    std::vector<double>& Qtab = ctx->h_Qtab;
    Qtab.assign((size_t)qn * qn, 0.0);
    ctx->qn = qn;
    bool dmat_mirror = true;
    for (int b = 0; b < qn; ++b)
        for (int a = 0; a < qn; ++a) {
            const int iy = (cc0 + b < S) ? cc0 + b : cc0 - b, ix = (cc0 + a < S) ? cc0 + a : cc0 - a;
            Qtab[(size_t)b * qn + a] = dm_h[(size_t)iy * S + ix];
        }
    for (int iy = 0; iy < S && dmat_mirror; ++iy)
        for (int ix = 0; ix < S; ++ix) {
            const double q = Qtab[(size_t)std::abs(iy - cc0) * qn + std::abs(ix - cc0)];
            if (memcmp(&q, &dm_h[(size_t)iy * S + ix], sizeof(double)) != 0) { dmat_mirror = false; break; }
        }
    ctx->dmat_mirror = dmat_mirror;
}

// the options, read here and nowhere else (but JOXSZ_MIX_FORM: choose_form; the transforms' two: fft_setup; the exact form's fold: plan_exact)
static int parse_options(jx_ctx* ctx, int* want_out, int* chunk_out) {
    const jx_config& c = ctx->cfg;
    int want = c.conv_mode;
    if (const char* e = opt_str(ctx, "JOXSZ_CONV")) {
        if (!strcmp(e, "rocfft")) want = 1; else if (!strcmp(e, "custom") || !strcmp(e, "mix")) want = 2; else if (!strcmp(e, "auto")) want = 0;
    }
    if (want < 0 || want > 2) { ctx->err = "conv_mode must be 0, 1 or 2"; return JX_ERR_INVALID; }
    *want_out = want;
    ctx->lr_tol0 = (c.S < 400) ? 1e-13 : JX_LR_TOL_DEFAULT;
    // (singular-value cut of the transfer-function weights: small maps -- a beam image comparable with the map, the
    //  log-posterior a small difference of large terms -- keep every term above rounding, where it costs next to nothing)
    if (const char* e = opt_str(ctx, "JOXSZ_LOWRANK_TOL")) { const double v2 = atof(e); if (v2 > 0.0 && v2 < 1e-6) { ctx->lr_tol0 = v2; ctx->tol_pinned = true; } }
    if (const char* e = opt_str(ctx, "JOXSZ_TRUNC_BOUND")) { const double v = atof(e); if (v > 0.0) { ctx->trunc_bound = v; ctx->trunc_bound_ll = std::min(ctx->trunc_bound_ll, 10.0 * v); } }
    if (const char* e = opt_str(ctx, "JOXSZ_MAP_PAIR")) ctx->map_pair = atoi(e) != 0;
    if (const char* e = opt_str(ctx, "JOXSZ_MIX_USPLIT")) { const int v = atoi(e); if (v >= 1 && v <= 4) { ctx->usplit = v; ctx->usplit_forced = true; } }
    if (const char* e = opt_str(ctx, "JOXSZ_MIX_SUBSAMPLE")) {
        // 0: every distinct sample; "u0,u1,npts": full resolution below u0 pixels from the axis, every second row up to u1, every fourth up to 2 u1, every eighth beyond
        int a0 = 0, a1 = 0, a2 = 0;
        const int got = sscanf(e, "%d,%d,%d", &a0, &a1, &a2);
        if (got == 1 && a0 == 0) ctx->subsample = false;
        else if (got == 3 && a0 >= 8 && a1 >= a0 && a2 >= 4 && a2 <= 16) { ctx->sub_u0 = a0; ctx->sub_u1 = a1; ctx->sub_npts = a2; }
    }
    if (const char* e = opt_str(ctx, "JOXSZ_EVAL_DIRECT")) { const int v = atoi(e); if (v >= 0 && v <= 3) ctx->eval_direct = v; }
    if (const char* e = opt_str(ctx, "JOXSZ_MIX_RANKCAP")) { const int v = atoi(e); if (v >= 0 && v <= 16) ctx->rank_cap = v; }
    if (const char* e = opt_str(ctx, "JOXSZ_MIX_MFMA")) ctx->mix_mfma = atoi(e) != 0;
    if (const char* e = opt_str(ctx, "JOXSZ_MIX_WPB")) { const int v = atoi(e); if (v >= 1 && v <= 16) { ctx->mix.wpb_force = v; ctx->mix.wpb = std::min(v, 4); } }
    if (const char* e = opt_str(ctx, "JOXSZ_MIX_KSPLIT")) { const int v = atoi(e); if (v >= 1) ctx->mix.ksplit_force = v; }
    if (const char* e = opt_str(ctx, "JOXSZ_MIX_KSPLIT_USE")) { const int v = atoi(e); if (v >= 1) ctx->mix.ksplit_u_force = v; }
    if (const char* e = opt_str(ctx, "JOXSZ_ABEL_GEMM")) ctx->abel_gemm = atoi(e) != 0;
    if (const char* e = opt_str(ctx, "JOXSZ_AG_NARROW")) ctx->ag_narrow = atoi(e) != 0;
    if (const char* e = opt_str(ctx, "JOXSZ_AG_SINGLE")) ctx->ag_single = atoi(e) != 0;
    if (const char* e = opt_str(ctx, "JOXSZ_X_PAIRWISE")) ctx->exact.pairwise = atoi(e) != 0;
    if (const char* e = opt_str(ctx, "JOXSZ_X_CONTRACT")) ctx->exact.contract = atoi(e) != 0;
    if (const char* e = opt_str(ctx, "JOXSZ_PREP_SPLIT")) ctx->prep_split = atoi(e) != 0;
    if (const char* e = opt_str(ctx, "JOXSZ_PREP_LEAN")) ctx->prep_lean = atoi(e) != 0;
    if (const char* e = opt_str(ctx, "JOXSZ_AG_SUBSAMPLE")) {
        int a0 = 0, a1 = 0, a2 = 0;
        const int got = sscanf(e, "%d,%d,%d", &a0, &a1, &a2);
        if (got == 1 && a0 == 0) ctx->ag_sub = false;
        else if (got == 3 && a0 >= 8 && a1 >= a0 && a2 >= 4 && a2 <= 24) { ctx->ag_u0 = a0; ctx->ag_u1 = a1; ctx->ag_npts = a2; }
    }
    if (const char* e = opt_str(ctx, "JOXSZ_PREP_FASTMATH")) ctx->prep_fastmath = atoi(e) != 0;
    ctx->op_narrow = opt_str(ctx, "JOXSZ_OP_NARROW") != nullptr;
    if (const char* e = opt_str(ctx, "JOXSZ_SIDE_STREAM")) ctx->side_on = atoi(e) != 0;
    if (const char* e = opt_str(ctx, "JOXSZ_SIDE_FORK")) ctx->side_fork = atoi(e) != 0;
    ctx->f32 = c.dtype == 1 || c.dtype == 2;
    ctx->f32c = c.dtype == 2;
    ctx->f32x = c.dtype == 3;
    if (ctx->f32x && want == 1) { ctx->err = "dtype 3 (f32x) is the exact form with fp32 products: the rocFFT sequence (conv = rocfft) is f64 only"; return JX_ERR_UNSUPPORTED; }
    if (ctx->f32x && !ctx->exact.pairwise) { ctx->err = "dtype 3 (f32x): JOXSZ_X_PAIRWISE=0 selects the reference kernels of the exact form, which are f64 only"; return JX_ERR_UNSUPPORTED; }
    if (ctx->f32 && !ctx->abel_gemm) { ctx->err = "dtype f32 takes its spline arrays from the matrix product only (JOXSZ_ABEL_GEMM=0 is an f64 setting)"; return JX_ERR_UNSUPPORTED; }

    int chunk = c.max_batch > 0 ? c.max_batch : 1024;
    if (const char* e = opt_str(ctx, "JOXSZ_CHUNK")) { int v = atoi(e); if (v > 0) chunk = v; }
    *chunk_out = chunk;
    if (const char* e = opt_str(ctx, "JOXSZ_PRUNE_OUTPUTS")) ctx->prune = atoi(e) != 0;
    return JX_OK;
}

// sizes and scalars of the kernels' constant block (JxDev)
static int scalar_constants(jx_ctx* ctx, const std::vector<double>& r) {
    const jx_config& c = ctx->cfg;
    const int N = c.N;
    JxDev& d = ctx->d;
    memset(&d, 0, sizeof(d));
    d.S = c.S; d.N = N; d.B = c.B; d.Sh = ctx->Sh; d.nrow = ctx->nrow; d.nt = ctx->nt;
    d.nflux = c.nflux; d.nconv = c.nconv; d.nann = c.nann; d.nband = c.nband; d.ntab = c.ntab;
    d.npar = c.npar; d.ndim = c.ndim; d.ne_mode = c.ne_mode; d.exclude_unphy_mass = c.exclude_unphy_mass;
    d.sz_only = c.sz_only;
#ifdef JOXSZ_ABLATIONS
    if (const char* e = opt_str(ctx, "JOXSZ_DBG")) d.dbg = atoi(e);      // diagnostic build only: timing experiments, results are wrong
    if (const char* e = opt_str(ctx, "JOXSZ_MIX_DBG")) ctx->mix.dbg = atoi(e);
#endif
    d.y_scale = c.kpc_cm * c.sigma_T / c.m_e;
    d.inv_h_mean = (double)(N - 1) / (r[N - 1] - r[0]);
    d.prep_pow = opt_str(ctx, "JOXSZ_PREP_POW") && atoi(opt_str(ctx, "JOXSZ_PREP_POW")) ? 1 : 0;
    if (!c.sz_only) {
        const std::vector<double> lt = host_vec<double>(ctx, JX_T_LNT);
        for (int i = 1; i < c.ntab; ++i)
            if (!(lt[i] > lt[i - 1])) { ctx->err = "lnT must be increasing"; return JX_ERR_INVALID; }
        d.inv_dlnT = (double)(c.ntab - 1) / (lt[c.ntab - 1] - lt[0]);
    }
    return JX_OK;
}

// evaluation matrix of g at the data radii (joxsz_funcs.py:476), and which outputs of the extracted row it reads at all:
// the cardinal functions of a cubic spline decay by 2 - sqrt(3) per knot, so data radii inside r_max give the row beyond
// r_max + ~35 pixels weights below 1e-22 of the largest -- nothing an fp64 sum can see.  The matrix-core product computes the
// outputs in use (whole tiles of 16); the row and brightness taps still get every output.
static int data_radii_matrix(jx_ctx* ctx, std::vector<double>& h_E, std::vector<double>& h_flux) {
    const jx_config& c = ctx->cfg;
    std::vector<double> radius = host_vec<double>(ctx, JX_T_RADIUS);
    std::vector<double> xk(radius.begin() + c.S / 2, radius.end());
    for (size_t i = 1; i < xk.size(); ++i)
        if (!(xk[i] > xk[i - 1])) { ctx->err = "radius[S//2:] must be increasing"; return JX_ERR_INVALID; }
    h_flux = host_vec<double>(ctx, JX_T_FLUX_DATA);
    std::vector<double> q(h_flux.begin(), h_flux.begin() + c.nflux);
    if (!jxt::nak_eval_matrix(xk, q, h_E)) { ctx->err = "profile spline: singular system"; return JX_ERR_INVALID; }
    double emax = 0.0;
    for (double v : h_E) if (std::isfinite(v)) emax = std::max(emax, std::fabs(v));
    int kuse = 0;
    bool finite = true;
    for (int k = 0; k < ctx->nrow; ++k)
        for (int dd = 0; dd < c.nflux; ++dd) {
            const double v = h_E[(size_t)dd * ctx->nrow + k];
            if (!std::isfinite(v)) finite = false;
            else if (std::fabs(v) > JX_PRUNE_TOL * emax) kuse = k + 1;
        }
    ctx->nrow_use = (finite && emax > 0.0) ? std::max(1, kuse) : ctx->nrow;
    return JX_OK;
}

// the plan of the exact form or of a contracted form (choose_form), on the checks and tables both share; false: `why`
static bool plan_back_end(jx_ctx* ctx, const std::vector<double>& r, long long tW, PlanShared& sh, MixBuild& mixb, ExactBuild& xb, std::string& why) {
    if (!plan_shared(ctx, host_vec<double>(ctx, JX_T_FILTERING), sh, why)) return false;
    const std::vector<double> beam = host_vec<double>(ctx, JX_T_BEAM_2D);
    const int form = choose_form(ctx);
    if (form == JX_FORM_EXACT) plan_exact(ctx, sh, beam, r, xb);
    else { plan_mix(ctx, sh, beam, r, ctx->lr_tol0, form, tW, mixb); why = mixb.why; }
    return xb.ok || mixb.ok;
}

// which back end: the exact form, a contracted form, or the rocFFT sequence (conv_mode; *P_out: its padded side)
static int choose_back_end(jx_ctx* ctx, int want, const std::vector<double>& r, long long tW, PlanShared& sh, MixBuild& mixb, ExactBuild& xb, int* P_out) {
    const jx_config& c = ctx->cfg;
    const int S = c.S, o = (c.B - 1) / 2;
    JxDev& d = ctx->d;
    // ---- does the Abel + map kernel (taps, rocFFT route, the guard's reference facility) fit this radial grid in LDS?  Without it
    //      the contracted route still runs -- its timed kernels never needed it -- but nothing can measure a truncation, so there
    //      is none: every singular term above rounding is kept and no cap applies.
    {
        JxDev dt = d;
        dt.quad = 1; dt.fast_map = (ctx->dmat_mirror && ctx->qn <= 9 * 64) ? 1 : 0; dt.q_na = dt.q_nb = ctx->qn;
        int th; size_t ld;
        ctx->map_ok = map_geometry(dt, 512, &th, &ld);
        if (!ctx->map_ok) { ctx->lr_tol0 = std::min(ctx->lr_tol0, 1e-13); ctx->rank_cap = 0; ctx->tol_pinned = true; ctx->subsample = false; }   // (nothing could measure a truncation or a sub-grid: neither is taken)
    }
    // ---- spline moment operator of the mirrored grid (joxsz_funcs.py:460) and the half-width of its band
    if (!jxt::mirrored_spline_op(r, ctx->h_G)) { ctx->err = "spline operator: singular system"; return JX_ERR_INVALID; }
    ctx->K = d.K = jxt::band_halfwidth(ctx->h_G, c.N, 1e-20);
    std::string why;
    bool planned = false;
    if (want != 1) {
        planned = plan_back_end(ctx, r, tW, sh, mixb, xb, why);
        if (want == 2 && !planned) { ctx->err = "contracted route: " + why; return JX_ERR_UNSUPPORTED; }
    }
    ctx->conv_mode = planned ? 2 : 1;
    if (ctx->f32 && ctx->conv_mode != 2) {                       // never silently fall back to the fp64 arithmetic
        ctx->err = "dtype f32 is available on the contracted route only" + (why.empty() ? std::string() : " (" + why + ")");
        return JX_ERR_UNSUPPORTED;
    }
    if (ctx->f32x && !xb.ok) {                                    // dtype 3 is the exact form or nothing
        const char* e = opt_str(ctx, "JOXSZ_MIX_FORM");
        if (planned && e && strcmp(e, "exact")) ctx->err = std::string("dtype 3 (f32x) is the exact form with fp32 products: JOXSZ_MIX_FORM=") + e + " selects a contracted form (dtypes 1 and 2 run there)";
        else if (planned) ctx->err = "dtype 3 (f32x): the exact form is not taken on this problem (the outputs the data-radii spline reads do not fit the tail's LDS)";
        else ctx->err = "dtype 3 (f32x): the exact form does not exist on this problem" + (why.empty() ? std::string() : " (" + why + ")");
        return JX_ERR_UNSUPPORTED;
    }
    if (ctx->f32c && mixb.form != 0) {
        ctx->err = "dtype 2 (fp32 arithmetic) exists on the low-rank form of the contracted route only; this problem takes the full form (dtype 1 keeps the arithmetic in fp64)";
        return JX_ERR_UNSUPPORTED;
    }
    int P = c.fft_pad > 0 ? c.fft_pad : jxt::next_smooth_even(S + o);
    if (const char* e = opt_str(ctx, "JOXSZ_FFT_PAD")) { int v = atoi(e); if (v > 0 && ctx->conv_mode == 1) P = v; }
    if (P < S + o) { ctx->err = "fft_pad smaller than S + (B-1)/2"; return JX_ERR_INVALID; }
    d.P = P; d.Ph = P / 2 + 1;
    *P_out = P;
    return JX_OK;
}

// device tables every route reads: Abel weights, the spline moment operator as a band, the integrated-Compton weights, h(0) weights,
// the data-radii matrix, the data, the twiddles of the rocFFT sequence's tail
static int shared_tables(jx_ctx* ctx, const std::vector<double>& r, const std::vector<double>& h_E, const std::vector<double>& h_flux, std::vector<double>& h_hw) {
    const jx_config& c = ctx->cfg;
    const int S = c.S, N = c.N;
    JxDev& d = ctx->d;
    int rc;
    // ---- Abel weights in on-the-fly form (per-source factor, diagonal, first off-diagonal)
    {
        std::vector<double> cj, dg, sp;
        jxt::abel_onfly_tables(r, cj, dg, sp);
        std::vector<double> tab((size_t)N * 4);
        for (int j = 0; j < N; ++j) { tab[4 * j] = r[j]; tab[4 * j + 1] = cj[j]; tab[4 * j + 2] = dg[j]; tab[4 * j + 3] = sp[j]; }
        double* p;
        if ((rc = dev_put(ctx, tab.data(), tab.size(), &p))) return rc; d.abel_tab = p;
    }
    // ---- spline moment operator of the mirrored grid, stored as a band
    {
        const std::vector<double>& G = ctx->h_G;
        const int K = ctx->K;
        std::vector<double> band((size_t)(2 * K + 1) * N, 0.0);
        for (int i = 0; i < N; ++i)
            for (int k = -K; k <= K; ++k) {
                const int j = i + k;
                if (j >= 0 && j < N) band[(size_t)(k + K) * N + i] = G[(size_t)i * N + j];
            }
        double* p; if ((rc = dev_put(ctx, band.data(), band.size(), &p))) return rc; d.gband = p;
        if (c.calc_integ) {
            // cint = w . [f(0), y],  f(0) = y_0 - r_0^2/2 * (G y)_0 (value at 0 of the mirrored spline),  y = y_scale * A pp:
            // one weight per radius of the pressure profile
            std::vector<double> w = host_vec<double>(ctx, JX_T_INTEG_W), wy(N), A, wp(N, 0.0);
            for (int j = 0; j < N; ++j) wy[j] = w[j + 1] - w[0] * 0.5 * r[0] * r[0] * G[j];
            wy[0] += w[0];
            jxt::abel_matrix(r, A);
            for (int i = 0; i < N; ++i) {
                const double f = d.y_scale * wy[i];
                for (int j = i; j < N; ++j) wp[j] += f * A[(size_t)i * N + j];
            }
            if ((rc = dev_put(ctx, wp.data(), wp.size(), &p))) return rc;
            d.integ_wp = p; d.calc_integ = 1; d.integ_mu = c.integ_mu; d.integ_sig = c.integ_sig;
        }
    }
    // ---- h(0) weights: spline through (+-r_pp[:nt], t) evaluated at 0 (joxsz_funcs.py:470-473)
    {
        std::vector<double> rt(r.begin(), r.begin() + ctx->nt), G;
        if (!jxt::mirrored_spline_op(rt, G)) { ctx->err = "h(0) operator: singular system"; return JX_ERR_INVALID; }
        std::vector<double>& hw = h_hw;
        hw.assign(ctx->nt, 0.0);
        for (int j = 0; j < ctx->nt; ++j) hw[j] = -0.5 * rt[0] * rt[0] * G[j];
        hw[0] += 1.0;
        double* p; if ((rc = dev_put(ctx, hw.data(), hw.size(), &p))) return rc; d.hw = p;
    }
    {
        double* p; if ((rc = dev_put(ctx, h_E.data(), h_E.size(), &p))) return rc; d.emat = p;
        if ((rc = dev_put(ctx, h_flux.data(), h_flux.size(), &p))) return rc; d.flux = p;
    }
    // ---- twiddles of the final inverse transform of the extracted row (rocFFT sequence's tail)
    {
        double* p;
        std::vector<double> tw((size_t)S * 2);
        for (int m = 0; m < S; ++m) { tw[2 * m] = std::cos(2.0 * jxt::kPi * m / S); tw[2 * m + 1] = std::sin(2.0 * jxt::kPi * m / S); }
        if ((rc = dev_put(ctx, tw.data(), tw.size(), &p))) return rc; d.twid = p;
    }
    return JX_OK;
}

// plain copies of the uploaded tensors, and the table packs an SZ-side / X-ray block of jx_walker2_kernel copies into LDS in one run
static int walker_tables(jx_ctx* ctx, const std::vector<double>& r, const std::vector<double>& h_hw) {
    const jx_config& c = ctx->cfg;
    JxDev& d = ctx->d;
    int rc;
    {
        double* p; int* q;
#define PUTD(field, id) { std::vector<double> v = host_vec<double>(ctx, id); if ((rc = dev_put(ctx, v.data(), v.size(), &p))) return rc; d.field = p; }
#define PUTI(field, id) { std::vector<int32_t> v = host_vec<int32_t>(ctx, id); if ((rc = dev_put(ctx, v.data(), v.size(), &q))) return rc; d.field = q; }
        {
            std::vector<double> lr = r;
            for (double& v : lr) v = std::log(v);
            if ((rc = dev_put(ctx, lr.data(), lr.size(), &p))) return rc;
            d.lr_pp = p;
        }
        {
            std::vector<double> fm;
            jxt::fastmath_tables(fm);                             // exp / log tables of the per-walker kernel (jx_fastmath.hpp)
            if ((rc = dev_put(ctx, fm.data(), fm.size(), &p))) return rc;
            d.fm_tab = p;
        }
        PUTD(r_pp, JX_T_R_PP) PUTD(d_mat, JX_T_D_MAT) PUTD(conv_T, JX_T_CONV_T) PUTD(conv_v, JX_T_CONV_V)
        PUTD(par_vals, JX_T_PAR_VALS) PUTD(par_min, JX_T_PAR_MIN) PUTD(par_max, JX_T_PAR_MAX)
        PUTD(par_mu, JX_T_PAR_MU) PUTD(par_sigma, JX_T_PAR_SIGMA)
        {   // -log(sqrt(2 pi)) - log(sigma) of the Gaussian priors, once
            std::vector<double> sg = host_vec<double>(ctx, JX_T_PAR_SIGMA);
            for (double& v : sg) v = (v > 0.0) ? -0.5 * std::log(2.0 * 3.14159265358979323846) - std::log(v) : 0.0;
            if ((rc = dev_put(ctx, sg.data(), sg.size(), &p))) return rc;
            d.par_lnorm = p;
        }
        PUTI(par_kind, JX_T_PAR_KIND) PUTI(thawed_idx, JX_T_THAWED_IDX)
        ctx->d_par_vals = const_cast<double*>(d.par_vals);
        {   // exp / log tables, radii and their logarithms, h(0) weights, conversion table in one run: what an SZ-side block of jx_walker2_kernel copies into LDS
            std::vector<double> pack;
            jxt::fastmath_tables(pack);
            pack.insert(pack.end(), r.begin(), r.end());
            for (double v : r) pack.push_back(std::log(v));
            pack.insert(pack.end(), h_hw.begin(), h_hw.end());
            for (int id : {JX_T_CONV_T, JX_T_CONV_V}) { const std::vector<double> v = host_vec<double>(ctx, id); pack.insert(pack.end(), v.begin(), v.end()); }
            if (pack.size() != JX_SZ_PACK_DOUBLES(d)) { ctx->err = "per-walker table pack: size"; return JX_ERR_INVALID; }
            if ((rc = dev_put(ctx, pack.data(), pack.size(), &p))) return rc;
            d.sz_pack = p;
        }
        if (!c.sz_only) {
            PUTD(x_r_ne, JX_T_X_R_NE) PUTD(x_r_T, JX_T_X_R_T) PUTD(projvols, JX_T_PROJVOLS) PUTD(cts, JX_T_CTS)
            PUTD(areascales, JX_T_AREASCALES) PUTD(exposures, JX_T_EXPOSURES) PUTD(backrates, JX_T_BACKRATES)
            PUTD(geomarea, JX_T_GEOMAREA) PUTD(lnT, JX_T_LNT) PUTD(lnrate, JX_T_LNRATE)
            // exp / log tables and the small tables of the X-ray side in one run: what an X-ray block of jx_walker2_kernel copies into LDS
            std::vector<double> pack;
            jxt::fastmath_tables(pack);
            for (int id : {JX_T_X_R_NE, JX_T_X_R_T, JX_T_GEOMAREA, JX_T_LNT, JX_T_PROJVOLS, JX_T_AREASCALES, JX_T_EXPOSURES, JX_T_BACKRATES, JX_T_CTS}) {
                const std::vector<double> v = host_vec<double>(ctx, id);
                pack.insert(pack.end(), v.begin(), v.end());
            }
            pack.insert(pack.end(), 2 * (size_t)d.nann, 0.0);    // log x_r_ne | log x_r_T: filled on the device below
            if (pack.size() != JX_XR_PACK_DOUBLES(d)) { ctx->err = "X-ray table pack: size"; return JX_ERR_INVALID; }
            if ((rc = dev_put(ctx, pack.data(), pack.size(), &p))) return rc;
            d.xr_pack = p;
            // the logarithms of the X-ray radii by the device's own table-driven function, once (the host's differ in the last bits)
            hipLaunchKernelGGL(jx_xr_logr_kernel, dim3(1), dim3(64), 0, 0, d.fm_tab, p + JX_FM_TABLE_DOUBLES, p + pack.size() - 2 * (size_t)d.nann, 2 * d.nann);
            HIPCHK(ctx, hipGetLastError());
            HIPCHK(ctx, hipDeviceSynchronize());
        }
#undef PUTD
#undef PUTI
    }
    return JX_OK;
}

// symmetric-map tables of the Abel + map kernel: coefficient slot and local abscissa of every quadrant radius; row slabs per walker
static int map_tables(jx_ctx* ctx, const std::vector<double>& r) {
    const jx_config& c = ctx->cfg;
    const int S = c.S, N = c.N;
    const std::vector<double>& Qtab = ctx->h_Qtab;
    JxDev& d = ctx->d;
    int rc;
    {
        const int na = ctx->qn;
        const bool sym = ctx->dmat_mirror && na <= 9 * 64;       // register-resident half row: |ix-c| < 576
        d.fast_map = sym ? 1 : 0;
        d.q_na = d.q_nb = na;
        if (sym) {
            std::vector<int32_t> qk((size_t)na * na);
            std::vector<double> qt((size_t)na * na);
            for (size_t e = 0; e < Qtab.size(); ++e) {
                const double dd = Qtab[e];
                if (!(dd <= r[N - 1])) { qk[e] = N; qt[e] = (dd != dd) ? dd : 0.0; }       // fill value 0 / NaN
                else if (dd < r[0]) { qk[e] = N - 1; qt[e] = dd; }                           // centre interval
                else {
                    int k = (int)(std::upper_bound(r.begin(), r.end(), dd) - r.begin()) - 1;
                    k = std::max(0, std::min(N - 2, k));
                    qk[e] = k; qt[e] = dd - r[k];
                }
            }
            int* qi; double* qd;
            if ((rc = dev_put(ctx, qk.data(), qk.size(), &qi))) return rc; d.q_k = qi;
            if ((rc = dev_put(ctx, qt.data(), qt.size(), &qd))) return rc; d.q_t = qd;
        }
    }
    int split = c.map_split > 0 ? c.map_split : 1;
    if (const char* e = opt_str(ctx, "JOXSZ_MAP_SPLIT")) { int v = atoi(e); if (v > 0) split = v; }
    d.map_split = std::min(split, S);
    return JX_OK;
}

// chunk capacity: the work buffers of a launch stay under 24 GB (mix_doubles: per walker, of the exact / contracted forms); the
// per-walker scalars of a chunk
static int chunk_capacity(jx_ctx* ctx, int chunk, int P, size_t mix_doubles, bool contracted_planned) {
    const jx_config& c = ctx->cfg;
    const int S = c.S;
    JxDev& d = ctx->d;
    int rc;
    const size_t budget = (size_t)24 << 30;
    if (ctx->conv_mode == 2) {
        // quadrant image of the Compton-y map (y_2d tap; only the profile taps and the full-map measurement use the kernel)
        d.quad = 1;
        d.img_ld = (d.q_na + 16) & ~15; d.img_ws = (long long)d.q_nb * d.img_ld;          // rows start on cache lines, >= 1 spare column
        const size_t per_walker = sizeof(double) * mix_doubles;
        if (c.max_batch <= 0 && !opt_str(ctx, "JOXSZ_CHUNK")) while (chunk > 128 && per_walker * chunk > budget) chunk /= 2;
    } else {
        d.quad = 0; d.img_ld = P; d.img_ws = (long long)P * P;
        const size_t per_walker = sizeof(double) * ((size_t)P * P * 2 + (size_t)P * d.Ph * 2 + (size_t)S * ctx->Sh * 2);
        while (chunk > 1 && per_walker * chunk > budget) chunk /= 2;
    }
    ctx->chunk = chunk;
    if (!map_geometry(d, 512, &ctx->map_threads, &ctx->map_lds)) {
        if (ctx->conv_mode != 2) { ctx->err = "radial grid too long for the LDS-resident spline of the Abel + map kernel (the rocFFT sequence needs it)"; return JX_ERR_UNSUPPORTED; }
        // the contracted forms decided their truncation and sub-grids on the earlier check of the same geometry: had that one passed and this one not,
        // those approximations would run with nothing to measure them -- refuse rather than run unguarded; the exact form takes none
        if (ctx->map_ok && contracted_planned) { ctx->err = "radial grid too long for the Abel + map kernel after the contracted tables were planned with it: use the exact form (JOXSZ_MIX_FORM=exact)"; return JX_ERR_UNSUPPORTED; }
        ctx->map_ok = false;
    }
    {
        const int lds = 160 * 1024 - 1024;
#define JX_ATTR(V, NA) HIPCHK(ctx, hipFuncSetAttribute((const void*)jx_abel_map_sym_kernel<V, NA>, hipFuncAttributeMaxDynamicSharedMemorySize, lds))
        JX_ATTR(true, 3); JX_ATTR(true, 5); JX_ATTR(true, 9); JX_ATTR(false, 3); JX_ATTR(false, 5); JX_ATTR(false, 9);
#undef JX_ATTR
        HIPCHK(ctx, hipFuncSetAttribute((const void*)jx_abel_map_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        HIPCHK(ctx, hipFuncSetAttribute((const void*)jx_abel_map_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    }
    if ((rc = dev_new(ctx, (size_t)chunk, &ctx->d_base))) return rc;
    if ((rc = dev_new(ctx, (size_t)chunk * 2, &ctx->d_xr))) return rc;
    if ((rc = dev_new(ctx, (size_t)chunk * ctx->nrow, &ctx->d_cfac))) return rc;
    if (c.calc_integ && (rc = dev_new(ctx, (size_t)chunk, &ctx->d_sz0, true))) return rc;
    return JX_OK;
}

static int finalize_impl(jx_ctx* ctx) {
    if (!ctx) return JX_ERR_INVALID;
    if (ctx->finalized) { ctx->err = "jx_finalize called twice"; return JX_ERR_STATE; }
    const jx_config& c = ctx->cfg;
    for (int id = 0; id < JX_T_COUNT; ++id) {
        if (c.sz_only && tensor_is_xray(id)) continue;
        if (id == JX_T_INTEG_W && !c.calc_integ) continue;
        if (!ctx->have[id]) { ctx->err = "tensor " + std::to_string(id) + " missing"; return JX_ERR_MISSING; }
    }
    HIPCHK(ctx, hipSetDevice(c.device));

    const int S = c.S, N = c.N;
    ctx->nrow = S - S / 2;
    ctx->nt = ctx->nrow - 1;
    ctx->Sh = S / 2 + 1;
    std::vector<double> r = host_vec<double>(ctx, JX_T_R_PP);
    for (int i = 0; i < N; ++i) {
        if (!(r[i] > 0) || (i && !(r[i] > r[i - 1]))) { ctx->err = "r_pp must be positive and increasing"; return JX_ERR_INVALID; }
    }
    std::vector<int32_t> thawed = host_vec<int32_t>(ctx, JX_T_THAWED_IDX);
    for (int k = 0; k < c.ndim; ++k)
        if (thawed[k] < 0 || thawed[k] >= c.npar) { ctx->err = "thawed_idx out of range"; return JX_ERR_INVALID; }

    int rc, want = 0, chunk = 0, P = 0;
    std::vector<double> h_E, h_flux, h_hw;
    PlanShared sh;
    MixBuild mixb;
    ExactBuild xb;
    mirror_quadrant(ctx);
    if ((rc = parse_options(ctx, &want, &chunk))) return rc;
    if ((rc = scalar_constants(ctx, r))) return rc;
    if ((rc = data_radii_matrix(ctx, h_E, h_flux))) return rc;
    const long long tW = ((long long)chunk + 127) & ~127LL;
    if ((rc = choose_back_end(ctx, want, r, tW, sh, mixb, xb, &P))) return rc;
    if ((rc = shared_tables(ctx, r, h_E, h_flux, h_hw))) return rc;
    if ((rc = walker_tables(ctx, r, h_hw))) return rc;
    if ((rc = map_tables(ctx, r))) return rc;
    if ((rc = chunk_capacity(ctx, chunk, P, (xb.ok ? 0 : mixb.krows) + (size_t)(JX_MIX_KSPLIT_MAX + 1) * 16 * sh.ntile + 8 * (size_t)N + 64, mixb.ok))) return rc;
    chunk = ctx->chunk;

    // ---- back-end set-up
    if (ctx->conv_mode == 2) {
        const long long tW2 = ((long long)chunk + 127) & ~127LL;
        if (tW2 != tW && mixb.ok && mixb.form == 1) {            // (the chunk shrank: the full form's sample offsets carry the walker stride)
            std::string why;
            mixb = MixBuild();
            if (!plan_back_end(ctx, r, tW2, sh, mixb, xb, why)) { ctx->err = "contracted route: " + why; return JX_ERR_UNSUPPORTED; }
        }
        if ((rc = dev_new(ctx, (size_t)chunk * ctx->d.q_nb, &ctx->d.xcol))) return rc;
        if (xb.ok) rc = exact_setup(ctx, xb, tW2);
        else if (!(rc = mix_setup(ctx, mixb, tW2))) rc = mix_context_tables(ctx, r, chunk);
        if (rc) return rc;
    } else {
        if ((rc = fft_setup(ctx, ctx->fft, chunk, P))) return rc;
    }
    HIPCHK(ctx, hipDeviceSynchronize());                          // (the zero fills ran on the null stream)
    ctx->finalized = true;
    return JX_OK;
}

static int ensure_batch(jx_ctx* ctx, int n) {
    if (n <= ctx->batch_cap) return JX_OK;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->d_theta) { (void)hipFree(ctx->d_theta); (void)hipFree(ctx->d_logp); ctx->d_theta = ctx->d_logp = nullptr; ctx->batch_cap = 0; }
    if (ctx->h_theta) { (void)hipHostFree(ctx->h_theta); (void)hipHostFree(ctx->h_logp); ctx->h_theta = ctx->h_logp = nullptr; }
    HIPCHK(ctx, hipMalloc((void**)&ctx->d_theta, sizeof(double) * (size_t)n * ctx->cfg.ndim));
    HIPCHK(ctx, hipMalloc((void**)&ctx->d_logp, sizeof(double) * (size_t)n));
    HIPCHK(ctx, hipHostMalloc((void**)&ctx->h_theta, sizeof(double) * (size_t)n * ctx->cfg.ndim, hipHostMallocMapped | hipHostMallocCoherent));
    HIPCHK(ctx, hipHostMalloc((void**)&ctx->h_logp, sizeof(double) * (size_t)n, hipHostMallocMapped | hipHostMallocCoherent));
    HIPCHK(ctx, hipHostGetDevicePointer((void**)&ctx->hd_theta, ctx->h_theta, 0));
    HIPCHK(ctx, hipHostGetDevicePointer((void**)&ctx->hd_logp, ctx->h_logp, 0));
    ctx->batch_cap = n;
    return JX_OK;
}

static int get_evset(jx_ctx* ctx, EvSet* out) {
    if (!ctx->ev_free.empty()) { *out = ctx->ev_free.back(); ctx->ev_free.pop_back(); return JX_OK; }
    for (int k = 0; k < 6; ++k) HIPCHK(ctx, hipEventCreate(&out->e[k]));
    return JX_OK;
}

static int drain_events(jx_ctx* ctx) {
    if (ctx->ev_inflight.empty()) return JX_OK;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (auto& es : ctx->ev_inflight) {
        float ms[5] = {0, 0, 0, 0, 0}, tot;
        if (es.p1only) {                               // two events per launch sequence: one kernel of the step alone
            HIPCHK(ctx, hipEventElapsedTime(&ms[2], es.e[2], es.e[3]));
            if (es.p1stage == 3) ctx->acc.prep_ms += ms[2];
            else if (es.p1stage == 4) ctx->acc.tail_ms += ms[2];
            else if (es.exact) ctx->acc.abel_map_ms += ms[2];
            else ctx->acc.beam_fft_ms += ms[2];
            ctx->acc.launches += 1; ctx->acc.walkers += es.walkers;
            ctx->ev_free.push_back(es);
            continue;
        }
        if (es.op) {                                   // collapsed route: prep, then one kernel
            HIPCHK(ctx, hipEventElapsedTime(&ms[0], es.e[0], es.e[1]));
            HIPCHK(ctx, hipEventElapsedTime(&ms[4], es.e[1], es.e[5]));
        } else if (es.exact) {                         // exact form: per-walker kernel, ordinate product, row product + tail
            HIPCHK(ctx, hipEventElapsedTime(&ms[0], es.e[0], es.e[1]));
            HIPCHK(ctx, hipEventElapsedTime(&ms[1], es.e[1], es.e[2]));
            HIPCHK(ctx, hipEventElapsedTime(&ms[4], es.e[2], es.e[5]));
        } else {
            for (int k = 0; k < 5; ++k) HIPCHK(ctx, hipEventElapsedTime(&ms[k], es.e[k], es.e[k + 1]));
        }
        HIPCHK(ctx, hipEventElapsedTime(&tot, es.e[0], es.e[5]));
        ctx->acc.prep_ms += ms[0]; ctx->acc.abel_map_ms += ms[1]; ctx->acc.beam_fft_ms += ms[2];
        ctx->acc.tf_fft_ms += ms[3]; ctx->acc.tail_ms += ms[4]; ctx->acc.total_ms += tot;
        ctx->acc.launches += 1; ctx->acc.walkers += es.walkers;
        ctx->ev_free.push_back(es);
    }
    ctx->ev_inflight.clear();
    return JX_OK;
}

// the reference facility of a contracted-route context: the rocFFT sequence for up to 16 walkers at a time
static int ensure_ref(jx_ctx* ctx) {
    if (ctx->fft.ready) return JX_OK;
    if (!ctx->map_ok) { ctx->err = "radial grid too long for the Abel + map kernel: the rocFFT reference facility (beam-convolved map tap, truncation probe) does not exist on this problem"; return JX_ERR_UNSUPPORTED; }
    return fft_setup(ctx, ctx->fft, std::min(16, ctx->chunk), ctx->d.P);
}

static int ensure_taps(jx_ctx* ctx) {
    if (ctx->t_pp) return JX_OK;
    const jx_config& c = ctx->cfg;
    const size_t C = ctx->chunk;
    int rc;
    if ((rc = dev_new(ctx, C * c.N, &ctx->t_pp))) return rc;
    if ((rc = dev_new(ctx, C * c.N, &ctx->t_ab))) return rc;
    if ((rc = dev_new(ctx, C * c.N, &ctx->t_y))) return rc;
    if ((rc = dev_new(ctx, C * ctx->nrow, &ctx->t_row))) return rc;
    if ((rc = dev_new(ctx, C * ctx->nrow, &ctx->t_bright))) return rc;
    if ((rc = dev_new(ctx, C * ctx->nrow, &ctx->t_tprof))) return rc;
    if ((rc = dev_new(ctx, C, &ctx->t_chisq))) return rc;
    if ((rc = dev_new(ctx, C * std::max(1, c.nband * c.nann), &ctx->t_xprofs, true))) return rc;
    if ((rc = dev_new(ctx, C * 4, &ctx->t_parts, true))) return rc;
    if ((rc = dev_new(ctx, C, &ctx->t_integ, true))) return rc;
    return JX_OK;
}

static Taps all_taps(jx_ctx* ctx, bool profiles) {
    Taps t;
    if (profiles) { t.pp = ctx->t_pp; t.ab = ctx->t_ab; t.y = ctx->t_y; }
    t.row = ctx->t_row; t.bright = ctx->t_bright; t.chisq = ctx->t_chisq; t.tprof = ctx->t_tprof;
    t.xprofs = ctx->cfg.sz_only ? nullptr : ctx->t_xprofs; t.parts = ctx->t_parts; t.integ = ctx->t_integ;
    return t;
}

// collapsed route (jx_set_route): per-walker kernel, then the SZ side as one kernel (no map, no transforms)
static int run_operator(jx_ctx* ctx, Chunk& c) {
    const JxDev& d = c.d;
    const Taps& t = c.t;
    hipStream_t st = c.st;
    const int n = c.n;
    launch_prep(ctx, c, st, ctx->d_pp, 0, d.nrow);
    if (c.tm) HIPCHK(ctx, hipEventRecord(c.es->e[1], st));
    const int nrow = d.nrow, Re = (nrow + 1) & ~1;
    // large launches: G pp on the fp64 matrix cores (G fetched once per 32 walkers), the rest in the kernel behind it
    const int mt = (nrow + 63) / 64;                                     // row tiles per wave
    const bool wide = n >= 4096 && (mt == 1 || mt == 2 || mt == 4 || mt == 8) && !ctx->op_narrow;
    if (wide) {
        const size_t shw = sizeof(double) * JX_OPM_JC * 33;
#define JX_OPM_GO(MTv) hipLaunchKernelGGL((jx_operator_mfma_kernel<MTv>), dim3((n + 31) / 32), dim3(256), shw, st, ctx->d_pp, n, d.N, nrow, \
                       ctx->d_G, ctx->g_ld, ctx->d_rows)
        if (mt == 1) JX_OPM_GO(1); else if (mt == 2) JX_OPM_GO(2); else if (mt == 4) JX_OPM_GO(4); else JX_OPM_GO(8);
#undef JX_OPM_GO
    }
    const double* rows_t = wide ? ctx->d_rows : nullptr;
    // walkers per block (x radii per LDS chunk = 2048): more of them spare G traffic; behind the matrix-core product there is none to spare
    int wpb = wide ? 4 : ((n >= 4096) ? 16 : (n >= 2048 ? 8 : 4));
    while (wpb > 4 && sizeof(double) * (2048 + (size_t)wpb * Re + 8) > 64 * 1024) wpb >>= 1;
    const size_t sh = sizeof(double) * (2048 + (size_t)wpb * Re + 8);
#define JX_OP_GO(WPBv) hipLaunchKernelGGL((jx_operator_kernel<WPBv, 2048 / WPBv>), dim3((n + WPBv - 1) / WPBv), dim3(256), sh, st, d, ctx->d_pp, c.w0, n, \
                       ctx->d_G, ctx->g_ld, rows_t, c.cfac, c.sz0, c.base, c.logp, t.row, t.bright, t.chisq, t.parts)
    if (wpb == 16) JX_OP_GO(16); else if (wpb == 8) JX_OP_GO(8); else JX_OP_GO(4);
#undef JX_OP_GO
    return JX_OK;
}

// One chunk: walkers [w0, w0+n) of the batch whose thetas live at theta_dev, through the context's route.  use_ref: through the reference
// facility (rocFFT sequence) of an exact / contracted context instead of its own back end.  smp: the stretch move inside the per-walker
// kernel and the tail (exact and contracted forms).
static int run_chunk(jx_ctx* ctx, const double* theta_dev, double* logp_dev, int w0, int n, const Taps& t, bool use_ref, const JxSm* smp) {
    int rc;
    hipStream_t st = ctx->stream;
    if (ctx->comm_overlap)                                         // a gather still reading this output buffer: the evaluation waits for it, and only for it
        for (auto& g : ctx->gslot)
            if (g.busy && g.send < (const char*)(logp_dev + w0 + n) && (const char*)(logp_dev + w0) < g.send + g.bytes) {     // (byte ranges overlap)
                // (a gather that has already finished costs a query on the host, not a barrier in the queue)
                if (hipEventQuery(g.done) != hipSuccess) HIPCHK(ctx, hipStreamWaitEvent(st, g.done, 0));
                g.busy = false;
            }
    const bool fftb = ctx->conv_mode == 1 || use_ref;
    const bool op_route = ctx->route == JX_ROUTE_OPERATOR && !t.pp && !ctx->d.inject_pp && !use_ref;   // stage taps and the operator build: map route
    const bool exact = !fftb && !op_route && ctx->exact.ready;
    EvSet es;
    // the operator route has no per-walker work buffers beyond these three, so its launches can be much larger than a chunk
    Chunk c{st, fftb ? ctx->fft.d : ctx->d, theta_dev, logp_dev, w0, n, t, JxSm{},
            op_route ? ctx->d_base_op : ctx->d_base, op_route ? ctx->d_cfac_op : ctx->d_cfac, op_route ? ctx->d_sz0_op : ctx->d_sz0, &es};
    memset(&c.sm, 0, sizeof(c.sm));
    if (smp) c.sm = *smp;
    // timing modes 2..4 record the two events around one kernel of the step only (exact and contracted forms)
    c.tm = ctx->timing_on && ctx->timing_mode == 1 && !use_ref;
    c.tm2 = ctx->timing_on && ctx->timing_mode >= 2 && !fftb && !op_route;
    if (c.tm || c.tm2) {
        if (ctx->ev_inflight.size() > 2048 && (rc = drain_events(ctx))) return rc;
        if ((rc = get_evset(ctx, &es))) return rc;
        es.walkers = n;
        es.op = op_route;
        es.p1only = c.tm2;
        es.exact = exact;
        es.p1stage = (exact && ctx->timing_mode >= 3) ? ctx->timing_mode : 2;
        if (c.tm) HIPCHK(ctx, hipEventRecord(es.e[0], st));
    }
    if ((rc = op_route ? run_operator(ctx, c) : exact ? run_exact(ctx, c) : !fftb ? run_mix(ctx, c) : run_fft(ctx, c))) return rc;
    if (c.tm) HIPCHK(ctx, hipEventRecord(es.e[5], st));
    if (c.tm || c.tm2) ctx->ev_inflight.push_back(es);
    HIPCHK(ctx, hipGetLastError());
    return JX_OK;
}

extern "C" {

int jx_finalize(jx_ctx* ctx) {
    int rc = finalize_impl(ctx);
    if (rc) return rc;
    if (const char* e = opt_str(ctx, "JOXSZ_TRUNC_PROBE")) { if (atoi(e) == 0) return JX_OK; }
    return mix_guard(ctx);
}

int jx_eval_device(jx_ctx* ctx, const double* theta_dev, int nwalkers, double* logp_dev) {
    if (!ctx || !theta_dev || !logp_dev || nwalkers < 0) return JX_ERR_INVALID;
    if (!ctx->finalized) { ctx->err = "jx_eval before jx_finalize"; return JX_ERR_STATE; }
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    Taps none;
    const int step = (ctx->route == JX_ROUTE_OPERATOR) ? ctx->op_cap : ctx->chunk;
    for (int w0 = 0; w0 < nwalkers; w0 += step) {
        const int n = std::min(step, nwalkers - w0);
        int rc = run_chunk(ctx, theta_dev, logp_dev, w0, n, none);
        if (rc) return rc;
    }
    return JX_OK;
}

int jx_sample(jx_ctx* ctx, const double* theta0, int nwalkers, int nsteps, double a, uint64_t seed,
              double* chain_out, double* logp_out, int64_t* naccept_out) {
    if (!ctx || !theta0 || nwalkers < 2 || (nwalkers & 1) || nsteps < 0 || !(a > 1.0)) return JX_ERR_INVALID;
    if (!ctx->finalized) { ctx->err = "jx_sample before jx_finalize"; return JX_ERR_STATE; }
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    const int ndim = ctx->cfg.ndim, W = nwalkers, half = W / 2;
    hipStream_t st = ctx->stream;
    double *x = nullptr, *lp = nullptr, *q = nullptr, *lq = nullptr, *zz = nullptr, *chain = nullptr, *lps = nullptr;
    long long* nacc = nullptr;
#define SCHK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { ctx->err = std::string(#expr) + ": " + hipGetErrorString(e_); return JX_ERR_HIP; } } while (0)
    // a run re-uses the buffers of the last one when they are large enough: repeated runs (burn-in, then sampling) do not
    // pay for device allocations of tens of megabytes each time (the buffers stay with the context, freed by jx_destroy)
    auto grab = [&](int slot, size_t bytes, void** out) -> hipError_t {
        if (ctx->samp_cap[slot] < bytes) {
            if (ctx->samp_buf[slot]) { (void)hipStreamSynchronize(st); (void)hipFree(ctx->samp_buf[slot]); ctx->samp_buf[slot] = nullptr; ctx->samp_cap[slot] = 0; }
            const hipError_t e = hipMalloc(&ctx->samp_buf[slot], bytes);
            if (e != hipSuccess) return e;
            ctx->samp_cap[slot] = bytes;
        }
        *out = ctx->samp_buf[slot];
        return hipSuccess;
    };
    SCHK(grab(0, sizeof(double) * (size_t)W * ndim, (void**)&x));
    SCHK(grab(1, sizeof(double) * (size_t)W, (void**)&lp));
    SCHK(grab(2, sizeof(double) * (size_t)half * ndim, (void**)&q));
    SCHK(grab(3, sizeof(double) * (size_t)half, (void**)&lq));
    SCHK(grab(4, sizeof(double) * (size_t)half, (void**)&zz));
    SCHK(grab(5, sizeof(long long) * (size_t)W, (void**)&nacc));
    SCHK(hipMemsetAsync(nacc, 0, sizeof(long long) * (size_t)W, st));
    if (chain_out && nsteps) SCHK(grab(6, sizeof(double) * (size_t)nsteps * W * ndim, (void**)&chain));
    if (logp_out && nsteps) SCHK(grab(7, sizeof(double) * (size_t)nsteps * W, (void**)&lps));
    SCHK(hipMemcpyAsync(x, theta0, sizeof(double) * (size_t)W * ndim, hipMemcpyHostToDevice, st));
    int rc = jx_eval_device(ctx, x, W, lp);
    if (rc) return rc;
    {
        std::vector<double> l0(W);
        SCHK(hipMemcpyAsync(l0.data(), lp, sizeof(double) * W, hipMemcpyDeviceToHost, st));
        SCHK(hipStreamSynchronize(st));
        for (double v : l0) if (!std::isfinite(v)) { ctx->err = "initial positions must have finite log-posterior"; return JX_ERR_INVALID; }
    }
    const dim3 grid((half + 255) / 256), block(256);
    const bool fused = ctx->conv_mode == 2 && ctx->route != JX_ROUTE_OPERATOR && !ctx->side_stream && !(opt_str(ctx, "JOXSZ_SAMPLE_FUSED") && atoi(opt_str(ctx, "JOXSZ_SAMPLE_FUSED")) == 0);
    // shares of a half step: one per rank of the communicator, or JOXSZ_SAMPLE_VIRTUAL_RANKS of them run in turn by this process
    const bool dist = ctx->comm != nullptr;                                  // (a communicator of one rank runs the same collectives: in place, on its own share = everything)
    int nshare = dist ? ctx->comm_size : 1;
    if (!dist) if (const char* e = opt_str(ctx, "JOXSZ_SAMPLE_VIRTUAL_RANKS")) nshare = std::max(1, atoi(e));
    if (nshare > 1 && (!fused || half % nshare)) { ctx->err = "jx_sample over " + std::to_string(nshare) + " ranks: the contracted route and a half ensemble divisible by the ranks"; return JX_ERR_INVALID; }
    const int r_first = dist ? ctx->comm_rank : 0, r_last = dist ? ctx->comm_rank + 1 : nshare;
    for (int it = 0; it < nsteps; ++it) {
        for (int hs = 0; hs < 2; ++hs) {
            const int s1 = hs * half, s2 = (1 - hs) * half;
            if (fused) {
                // contracted route: the proposal is drawn by the per-walker kernel, the tail accepts or rejects -- five launches per half step, not seven
                JxSm sm;
                memset(&sm, 0, sizeof(sm));
                sm.on = 1; sm.ndim = ndim; sm.half = half; sm.s1 = s1; sm.s2 = s2; sm.iter2 = 2 * it + hs; sm.a = a; sm.seed = seed;
                sm.x = x; sm.q = q; sm.zz = zz; sm.lp = lp; sm.nacc = reinterpret_cast<long long*>(nacc);
                Taps none;
                // Walkers shard over the ranks of the context's communicator (jx_comm_init_rank): the proposals of a half step read the OTHER half
                // and the walker's own position only, so a rank moves its contiguous share of the half alone, and one in-place all-gather of the
                // share's positions and log-posteriors brings every rank's copy of the ensemble up to date before the next half step -- the RCCL
                // exchange of a real sampling run.  (JOXSZ_SAMPLE_VIRTUAL_RANKS=R, no communicator: the R shares one after the other in this
                // process -- the same chain by construction; the test of the share arithmetic where there is one GPU.)
                for (int r = r_first; r < r_last; ++r) {
                    const int lo = (int)((long long)r * half / nshare), hi = (int)((long long)(r + 1) * half / nshare);
                    for (int w0 = lo; w0 < hi; w0 += ctx->chunk)
                        if ((rc = run_chunk(ctx, q, lq, w0, std::min(ctx->chunk, hi - w0), none, false, &sm))) return rc;
                }
                if (dist) {
                    const size_t share = (size_t)half / nshare;
                    NCCLCHK(ctx, g_rccl.AllGather(x + ((size_t)s1 + ctx->comm_rank * share) * ndim, x + (size_t)s1 * ndim, share * ndim, ncclDouble, ctx->comm, st));
                    NCCLCHK(ctx, g_rccl.AllGather(lp + (size_t)s1 + ctx->comm_rank * share, lp + (size_t)s1, share, ncclDouble, ctx->comm, st));
                }
                continue;
            }
            hipLaunchKernelGGL(jx_sm_propose_kernel, grid, block, 0, st, x, q, zz, ndim, half, s1, s2, 2 * it + hs, a, seed);
            if ((rc = jx_eval_device(ctx, q, half, lq))) return rc;
            hipLaunchKernelGGL(jx_sm_accept_kernel, grid, block, 0, st, x, lp, q, lq, zz, nacc, ndim, half, s1, 2 * it + hs, seed);
        }
        if (chain) SCHK(hipMemcpyAsync(chain + (size_t)it * W * ndim, x, sizeof(double) * (size_t)W * ndim, hipMemcpyDeviceToDevice, st));
        if (lps) SCHK(hipMemcpyAsync(lps + (size_t)it * W, lp, sizeof(double) * (size_t)W, hipMemcpyDeviceToDevice, st));
    }
    if (chain) SCHK(hipMemcpyAsync(chain_out, chain, sizeof(double) * (size_t)nsteps * W * ndim, hipMemcpyDeviceToHost, st));
    if (lps) SCHK(hipMemcpyAsync(logp_out, lps, sizeof(double) * (size_t)nsteps * W, hipMemcpyDeviceToHost, st));
    if (dist) NCCLCHK(ctx, g_rccl.AllReduce(nacc, nacc, (size_t)W, ncclInt64, ncclSum, ctx->comm, st));      // (a rank counted its own shares only)
    if (naccept_out) SCHK(hipMemcpyAsync(naccept_out, nacc, sizeof(long long) * (size_t)W, hipMemcpyDeviceToHost, st));
    SCHK(hipStreamSynchronize(st));
    SCHK(hipGetLastError());
#undef SCHK
    return JX_OK;
}

}  // extern "C"

// G by the MAP route's own kernels: the unit profiles e_j go in as injected pressure profiles, their map rows come out
// of the row tap.  (theta only feeds the prep kernel here; the current parameter values keep it on ordinary numbers.)
static int build_operator(jx_ctx* ctx) {
    const jx_config& c = ctx->cfg;
    const int N = c.N, nrow = ctx->nrow, ld = (nrow + 15) & ~15;
    int rc;
    if ((rc = ensure_taps(ctx))) return rc;
    if ((rc = ensure_batch(ctx, ctx->chunk))) return rc;
    double* G = nullptr;
    double* inj = nullptr;
    if ((rc = dev_new(ctx, (size_t)(N + JX_OPM_GPAD) * ld, &G, true))) return rc;   // zero rows behind the last: the kernels read j in pairs / groups of 16, three k-steps ahead
    HIPCHK(ctx, hipMalloc((void**)&inj, sizeof(double) * (size_t)ctx->chunk * N));
    std::vector<double> th((size_t)ctx->chunk * c.ndim);
    {
        const std::vector<double> pv = host_vec<double>(ctx, JX_T_PAR_VALS);
        const std::vector<int32_t> ti = host_vec<int32_t>(ctx, JX_T_THAWED_IDX);
        for (int w = 0; w < ctx->chunk; ++w) for (int k = 0; k < c.ndim; ++k) th[(size_t)w * c.ndim + k] = pv[ti[k]];
    }
    hipStream_t st = ctx->stream;
    const bool tm = ctx->timing_on;
    auto fail = [&](int code) { (void)hipStreamSynchronize(st); ctx->d.inject_pp = nullptr; ctx->timing_on = tm; (void)hipFree(inj); return code; };
    if (hipMemcpyAsync(ctx->d_theta, th.data(), sizeof(double) * th.size(), hipMemcpyHostToDevice, st) != hipSuccess) return fail(JX_ERR_HIP);
    // (fp32 contexts take their spline arrays from the matrix product of the injected profiles: no profile taps there)
    Taps t = all_taps(ctx, !ctx->f32 && ctx->map_ok);
    std::vector<double> eye;
    ctx->timing_on = false;
    for (int j0 = 0; j0 < N; j0 += ctx->chunk) {
        const int n = std::min(ctx->chunk, N - j0);
        eye.assign((size_t)n * N, 0.0);
        for (int w = 0; w < n; ++w) eye[(size_t)w * N + j0 + w] = 1.0;
        if (hipMemcpyAsync(inj, eye.data(), sizeof(double) * eye.size(), hipMemcpyHostToDevice, st) != hipSuccess) return fail(JX_ERR_HIP);
        ctx->d.inject_pp = inj;
        rc = run_chunk(ctx, ctx->d_theta, ctx->d_logp, 0, n, t);
        ctx->d.inject_pp = nullptr;
        if (rc) return fail(rc);
        if (hipMemcpy2DAsync(G + (size_t)j0 * ld, sizeof(double) * ld, ctx->t_row, sizeof(double) * nrow, sizeof(double) * nrow, n,
                             hipMemcpyDeviceToDevice, st) != hipSuccess) return fail(JX_ERR_HIP);
        if (hipStreamSynchronize(st) != hipSuccess) return fail(JX_ERR_HIP);
    }
    ctx->timing_on = tm;
    (void)hipFree(inj);
    ctx->op_cap = std::max(ctx->chunk, ctx->cfg.max_batch > 0 ? ctx->chunk : 16384);      // (an explicit max_batch bounds this route too)
    if ((rc = dev_new(ctx, (size_t)ctx->op_cap * N, &ctx->d_pp))) return rc;
    if ((rc = dev_new(ctx, (size_t)ctx->op_cap, &ctx->d_base_op))) return rc;
    if ((rc = dev_new(ctx, (size_t)ctx->op_cap * nrow, &ctx->d_cfac_op))) return rc;
    if (c.calc_integ && (rc = dev_new(ctx, (size_t)ctx->op_cap, &ctx->d_sz0_op, true))) return rc;
    if ((rc = dev_new(ctx, ((size_t)ctx->op_cap + 32) * nrow, &ctx->d_rows))) return rc;
    ctx->d_G = G;
    ctx->g_ld = ld;
    return JX_OK;
}

extern "C" {

int jx_set_route(jx_ctx* ctx, int route) {
    if (!ctx || (route != JX_ROUTE_MAP && route != JX_ROUTE_OPERATOR)) return JX_ERR_INVALID;
    if (!ctx->finalized) { ctx->err = "jx_set_route before jx_finalize"; return JX_ERR_STATE; }
    if (route == JX_ROUTE_OPERATOR && ctx->f32x) { ctx->err = "dtype 3 (f32x): the operator route is built from and run in f64; use an f64 context for it"; return JX_ERR_UNSUPPORTED; }
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    if (route == JX_ROUTE_OPERATOR && !ctx->d_G) {
        const int rc = build_operator(ctx);
        if (rc) return rc;
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->route = route;
    return JX_OK;
}

int jx_get_route(jx_ctx* ctx) { return ctx ? ctx->route : JX_ERR_INVALID; }

int jx_get_operator(jx_ctx* ctx, double* out, size_t nbytes) {
    if (!ctx || !out) return JX_ERR_INVALID;
    if (!ctx->d_G) { ctx->err = "jx_get_operator: the operator route was never selected"; return JX_ERR_STATE; }
    if (nbytes != sizeof(double) * (size_t)ctx->cfg.N * ctx->nrow) { ctx->err = "jx_get_operator: wrong output size"; return JX_ERR_INVALID; }
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    HIPCHK(ctx, hipMemcpy2DAsync(out, sizeof(double) * ctx->nrow, ctx->d_G, sizeof(double) * ctx->g_ld, sizeof(double) * ctx->nrow,
                                 ctx->cfg.N, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return JX_OK;
}

int jx_set_stream(jx_ctx* ctx, void* hip_stream) {
    if (!ctx) return JX_ERR_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->stream = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream;
    if (ctx->fft.info) FFTCHK(ctx, rocfft_execution_info_set_stream(ctx->fft.info, ctx->stream));
    return JX_OK;
}

int jx_sync(jx_ctx* ctx) {
    if (!ctx) return JX_ERR_INVALID;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->comm_stream) HIPCHK(ctx, hipStreamSynchronize(ctx->comm_stream));
    return JX_OK;
}

int jx_eval(jx_ctx* ctx, const double* theta, int nwalkers, double* logp) {
    if (!ctx || nwalkers < 0 || (nwalkers && (!theta || !logp))) return JX_ERR_INVALID;
    if (!ctx->finalized) { ctx->err = "jx_eval before jx_finalize"; return JX_ERR_STATE; }
    if (nwalkers == 0) return JX_OK;
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    int rc = ensure_batch(ctx, nwalkers);
    if (rc) return rc;
    // through pinned staging: the copies are then plain DMA enqueued on the stream, and the call waits once, at its end
    // The staging buffers are mapped into the device's address space: the per-walker kernel reads its 13 parameters straight
    // from the host buffer and the tail stores the log-probability there (posted writes over PCIe, visible at the
    // synchronisation) -- no copy command on either side of the five kernels.  JOXSZ_EVAL_DIRECT=0: both as DMA copies.
    memcpy(ctx->h_theta, theta, sizeof(double) * (size_t)nwalkers * ctx->cfg.ndim);
    const bool th_direct = (ctx->eval_direct & 2) != 0, lp_direct = (ctx->eval_direct & 1) != 0;
    if (!th_direct) HIPCHK(ctx, hipMemcpyAsync(ctx->d_theta, ctx->h_theta, sizeof(double) * (size_t)nwalkers * ctx->cfg.ndim, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = jx_eval_device(ctx, th_direct ? ctx->hd_theta : ctx->d_theta, nwalkers, lp_direct ? ctx->hd_logp : ctx->d_logp))) return rc;
    if (!lp_direct) HIPCHK(ctx, hipMemcpyAsync(ctx->h_logp, ctx->d_logp, sizeof(double) * (size_t)nwalkers, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(logp, ctx->h_logp, sizeof(double) * (size_t)nwalkers);
    return JX_OK;
}

int jx_eval_stage(jx_ctx* ctx, const double* theta, int nwalkers, int stage, double* out, size_t nbytes) {
    if (!ctx || !theta || !out || nwalkers <= 0) return JX_ERR_INVALID;
    if (!ctx->finalized) { ctx->err = "jx_eval_stage before jx_finalize"; return JX_ERR_STATE; }
    if (stage < 0 || stage >= JX_STAGE_COUNT) return JX_ERR_INVALID;
    const jx_config& c = ctx->cfg;
    const size_t S = c.S;
    size_t per = 0;
    switch (stage) {
        case JX_STAGE_PP: case JX_STAGE_AB: case JX_STAGE_Y: per = c.N; break;
        case JX_STAGE_Y2D: case JX_STAGE_CONV2D: per = S * S; break;
        case JX_STAGE_MAPROW: case JX_STAGE_BRIGHT: case JX_STAGE_TPROF: per = ctx->nrow; break;
        case JX_STAGE_CHISQ: per = 1; break;
        case JX_STAGE_XPROFS: per = (size_t)c.nband * c.nann; break;
        case JX_STAGE_PARTS: per = 4; break;
        case JX_STAGE_INTEG: per = 1; break;
    }
    if (stage == JX_STAGE_INTEG && !c.calc_integ) { ctx->err = "the 'integ' output needs calc_integ"; return JX_ERR_INVALID; }
    if (stage == JX_STAGE_XPROFS && c.sz_only) { ctx->err = "no X-ray profiles in sz_only mode"; return JX_ERR_INVALID; }
    if (nbytes != per * sizeof(double) * (size_t)nwalkers) { ctx->err = "jx_eval_stage: wrong output size"; return JX_ERR_INVALID; }
    HIPCHK(ctx, hipSetDevice(c.device));
    int rc;
    if ((rc = ensure_taps(ctx))) return rc;
    // the beam-convolved map exists in the rocFFT sequence only: contracted-route contexts send this tap through their
    // reference facility (16 walkers at a time)
    const bool via_ref = stage == JX_STAGE_CONV2D && ctx->conv_mode == 2;
    if (via_ref && (rc = ensure_ref(ctx))) return rc;
    const bool y2d_quad = (stage == JX_STAGE_Y2D && ctx->conv_mode == 2);
    if (y2d_quad && !ctx->t_y2d && (rc = dev_new(ctx, (size_t)ctx->chunk * S * S, &ctx->t_y2d))) return rc;
    if ((rc = ensure_batch(ctx, nwalkers))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_theta, theta, sizeof(double) * (size_t)nwalkers * c.ndim, hipMemcpyHostToDevice, ctx->stream));
    const bool profiles = !ctx->f32 || stage == JX_STAGE_PP || stage == JX_STAGE_AB || stage == JX_STAGE_Y;
    Taps t = all_taps(ctx, profiles);
    t.need_img = (stage == JX_STAGE_Y2D);
    t.need_conv = (stage == JX_STAGE_CONV2D);
    // exact form with contracted partials: chi^2 and the parts come from the launches jx_eval runs (no row, no brightness: those two taps
    // would bring the partial rows back); every other stage, and every other form, keeps all its taps
    if ((stage == JX_STAGE_CHISQ || stage == JX_STAGE_PARTS) && !via_ref && ctx->exact.ready && ctx->exact.contracted()) { t.row = nullptr; t.bright = nullptr; }
    const int step = via_ref ? ctx->fft.cap : ctx->chunk;
    for (int w0 = 0; w0 < nwalkers; w0 += step) {
        const int n = std::min(step, nwalkers - w0);
        if ((rc = run_chunk(ctx, ctx->d_theta, ctx->d_logp, w0, n, t, via_ref))) return rc;
        double* dst = out + per * (size_t)w0;
        const double* src = nullptr;
        switch (stage) {
            case JX_STAGE_PP: src = ctx->t_pp; break;
            case JX_STAGE_AB: src = ctx->t_ab; break;
            case JX_STAGE_Y: src = ctx->t_y; break;
            case JX_STAGE_MAPROW: src = ctx->t_row; break;
            case JX_STAGE_BRIGHT: src = ctx->t_bright; break;
            case JX_STAGE_TPROF: src = ctx->t_tprof; break;
            case JX_STAGE_CHISQ: src = ctx->t_chisq; break;
            case JX_STAGE_XPROFS: src = ctx->t_xprofs; break;
            case JX_STAGE_PARTS: src = ctx->t_parts; break;
            case JX_STAGE_INTEG: src = ctx->t_integ; break;
            default: break;
        }
        if (src) {
            HIPCHK(ctx, hipMemcpyAsync(dst, src, per * sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream));
        } else {
            const size_t P = ctx->fft.P;
            if (y2d_quad)
                hipLaunchKernelGGL(jx_expand_quad_kernel, dim3((unsigned)S, n), dim3(256), 0, ctx->stream, ctx->d_img, (size_t)ctx->d.img_ld,
                                   (size_t)ctx->d.img_ws, (int)S, ctx->t_y2d);
            const double* base = (stage == JX_STAGE_Y2D) ? (y2d_quad ? ctx->t_y2d : ctx->fft.img) : ctx->fft.conv;
            const size_t ld = (stage == JX_STAGE_Y2D && y2d_quad) ? S : P;
            const size_t ws = (stage == JX_STAGE_Y2D && y2d_quad) ? S * S : P * (size_t)ctx->fft.rows;
            for (int w = 0; w < n; ++w)
                HIPCHK(ctx, hipMemcpy2DAsync(dst + (size_t)w * S * S, S * sizeof(double), base + (size_t)w * ws,
                                             ld * sizeof(double), S * sizeof(double), S, hipMemcpyDeviceToHost, ctx->stream));
        }
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    return JX_OK;
}

int jx_set_option(jx_ctx* ctx, const char* name, const char* value) {
    if (!ctx || !name) return JX_ERR_INVALID;
    std::string key = name;
    for (char& ch : key) ch = (char)toupper((unsigned char)ch);
    if (key.rfind("JOXSZ_", 0) != 0) key = "JOXSZ_" + key;
    bool known = false;
    for (const char* k : kOptions) if (key == k) known = true;
    if (!known) { ctx->err = "jx_set_option: unknown option " + key; return JX_ERR_INVALID; }
    const bool at_call = key == "JOXSZ_SAMPLE_FUSED" || key == "JOXSZ_SAMPLE_VIRTUAL_RANKS";
    if (ctx->finalized && !at_call) { ctx->err = "jx_set_option(" + key + ") after jx_finalize: read there and nowhere else"; return JX_ERR_STATE; }
    ctx->opts[key] = value ? value : "";                         // (an empty value: the option unset, whatever the environment says)
    return JX_OK;
}

// Run-time assurance: the given walkers through the context's own route (as jx_eval runs it) AND through the rocFFT sequence held inside
// the same context (joxsz_funcs.py:460-467 executed literally, 16 walkers at a time: an independent implementation, not the same tables).
int jx_audit(jx_ctx* ctx, const double* theta, int n, double out[4]) {
    if (!ctx || !theta || n < 1 || !out) return JX_ERR_INVALID;
    if (!ctx->finalized) { ctx->err = "jx_audit before jx_finalize"; return JX_ERR_STATE; }
    out[0] = out[1] = 0.0; out[2] = -1.0; out[3] = 0.0;
    if (ctx->conv_mode != 2) return JX_OK;                       // (the rocFFT sequence IS this context's route: nothing to compare)
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    int rc;
    if ((rc = ensure_taps(ctx))) return rc;
    if ((rc = ensure_ref(ctx))) return rc;
    const int cap = ctx->fft.cap, nrow = ctx->nrow, ndim = ctx->cfg.ndim;
    if ((rc = ensure_batch(ctx, cap))) return rc;
    std::vector<double> ra((size_t)cap * nrow), rb((size_t)cap * nrow), la((size_t)cap * 4), lb((size_t)cap * 4);
    const bool tm = ctx->timing_on;
    const int route = ctx->route;
    ctx->timing_on = false;
    ctx->route = JX_ROUTE_MAP;                                   // (the taps exist on this route; the collapsed route is built from it)
    Taps t = all_taps(ctx, false);
    auto fetch = [&](std::vector<double>& rows, std::vector<double>& parts, int m) {
        if (hipMemcpyAsync(rows.data(), ctx->t_row, sizeof(double) * (size_t)m * nrow, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) return (int)JX_ERR_HIP;
        if (hipMemcpyAsync(parts.data(), ctx->t_parts, sizeof(double) * (size_t)m * 4, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) return (int)JX_ERR_HIP;
        return (hipStreamSynchronize(ctx->stream) == hipSuccess) ? (int)JX_OK : (int)JX_ERR_HIP;
    };
    rc = JX_OK;
    for (int w0 = 0; w0 < n && !rc; w0 += cap) {
        const int m = std::min(cap, n - w0);
        if (hipMemcpyAsync(ctx->d_theta, theta + (size_t)w0 * ndim, sizeof(double) * (size_t)m * ndim, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) { rc = JX_ERR_HIP; break; }
        rc = run_chunk(ctx, ctx->d_theta, ctx->d_logp, 0, m, t);
        if (!rc) rc = fetch(ra, la, m);
        if (!rc) rc = run_chunk(ctx, ctx->d_theta, ctx->d_logp, 0, m, t, true);
        if (!rc) rc = fetch(rb, lb, m);
        if (rc) break;
        for (int p = 0; p < m; ++p) {
            double mx = 0.0, df = 0.0;
            bool fin = true;
            for (int k = 0; k < nrow; ++k) {
                const double a = ra[(size_t)p * nrow + k], b = rb[(size_t)p * nrow + k];
                if (!std::isfinite(a) || !std::isfinite(b)) { fin = false; break; }
                mx = std::max(mx, std::fabs(b)); df = std::max(df, std::fabs(a - b));
            }
            const double sa = la[(size_t)p * 4 + 1], sb = lb[(size_t)p * 4 + 1];     // SZ log-likelihood (-chi^2/2 [+ integrated-Compton term])
            if (!fin || !(mx > 0.0) || !std::isfinite(sa) || !std::isfinite(sb)) continue;
            if (la[(size_t)p * 4 + 3] != 0.0) continue;               // (a rejected walker -- outside the prior box, vetoed -- is no place a chain lives)
            out[3] += 1.0;
            out[1] = std::max(out[1], df / mx);
            if (std::fabs(sa - sb) >= out[0]) { out[0] = std::fabs(sa - sb); out[2] = (double)(w0 + p); }
        }
    }
    ctx->timing_on = tm;
    ctx->route = route;
    return rc;
}

int jx_set_par_vals(jx_ctx* ctx, const double* v, int npar) {
    if (!ctx || !v || npar != ctx->cfg.npar) return JX_ERR_INVALID;
    if (!ctx->finalized) return jx_upload(ctx, JX_T_PAR_VALS, v, sizeof(double) * npar);
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_par_vals, v, sizeof(double) * npar, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->host[JX_T_PAR_VALS].assign((const unsigned char*)v, (const unsigned char*)v + sizeof(double) * npar);
    return JX_OK;
}

int jx_dev_alloc(jx_ctx* ctx, size_t nbytes, void** out) {
    if (!ctx || !out) return JX_ERR_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    HIPCHK(ctx, hipMalloc(out, std::max<size_t>(nbytes, 8)));
    return JX_OK;
}

int jx_dev_free(jx_ctx* ctx, void* p) {
    if (!ctx) return JX_ERR_INVALID;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipFree(p));
    return JX_OK;
}

int jx_memcpy_h2d(jx_ctx* ctx, void* dev, const void* host, size_t n) {
    if (!ctx || !dev || !host) return JX_ERR_INVALID;
    HIPCHK(ctx, hipMemcpyAsync(dev, host, n, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return JX_OK;
}

int jx_memcpy_d2h(jx_ctx* ctx, void* host, const void* dev, size_t n) {
    if (!ctx || !dev || !host) return JX_ERR_INVALID;
    HIPCHK(ctx, hipMemcpyAsync(host, dev, n, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return JX_OK;
}

int jx_timing_enable(jx_ctx* ctx, int on) {
    if (!ctx) return JX_ERR_INVALID;
    ctx->timing_on = on != 0;
    ctx->timing_mode = (on >= 2 && on <= 4) ? on : (on ? 1 : 0);
    return JX_OK;
}

int jx_timing_reset(jx_ctx* ctx) {
    if (!ctx) return JX_ERR_INVALID;
    int rc = drain_events(ctx);
    if (rc) return rc;
    memset(&ctx->acc, 0, sizeof(ctx->acc));
    return JX_OK;
}

int jx_timing_get(jx_ctx* ctx, jx_timing* out) {
    if (!ctx || !out) return JX_ERR_INVALID;
    int rc = drain_events(ctx);
    if (rc) return rc;
    *out = ctx->acc;
    return JX_OK;
}

int jx_get_info(jx_ctx* ctx, int32_t* fft_pad, int32_t* chunk, int32_t* band, int32_t* nrow, int64_t* bytes) {
    if (!ctx || !ctx->finalized) return JX_ERR_STATE;
    if (fft_pad) *fft_pad = ctx->d.P;
    if (chunk) *chunk = ctx->chunk;
    if (band) *band = ctx->K;
    if (nrow) *nrow = ctx->nrow;
    if (bytes) *bytes = ctx->device_bytes;
    return JX_OK;
}

int jx_get_fft_info(jx_ctx* ctx, int32_t out[34]) {
    if (!ctx || !ctx->finalized || !out) return JX_ERR_STATE;
    const FftBack& fb = ctx->fft;
    for (int i = 0; i < 34; ++i) out[i] = 0;
    if (!fb.ready) return JX_OK;
    out[0] = 1; out[1] = fb.cols ? 1 : 0; out[2] = fb.rows_custom ? 1 : 0; out[3] = fb.P;
    if (!fb.cols) return JX_OK;
    out[4] = fb.ldc; out[5] = fb.ldt; out[6] = fft_cb(fb.P);
    out[7] = fb.fP.npass;
    for (int p = 0; p < fb.fP.npass && p < JX_FFT_MAXPASS; ++p) out[8 + p] = fb.fP.radix[p];
    out[20] = fb.fS.npass;
    for (int p = 0; p < fb.fS.npass && p < JX_FFT_MAXPASS; ++p) out[21 + p] = fb.fS.radix[p];
    return JX_OK;
}

int jx_get_conv_mode(jx_ctx* ctx) {
    if (!ctx || !ctx->finalized) return JX_ERR_STATE;
    return ctx->conv_mode;
}

int jx_get_conv_layout(jx_ctx* ctx, int32_t out[12]) {
    if (!ctx || !ctx->finalized || !out) return JX_ERR_STATE;
    if (ctx->conv_mode != 2) { ctx->err = "layout of the contracted route only"; return JX_ERR_UNSUPPORTED; }
    if (ctx->exact.ready) {
        const ExactBack& x = ctx->exact;
        out[0] = 2; out[1] = ctx->qn; out[2] = x.Nk; out[3] = x.Nkp; out[4] = 0; out[5] = 0; out[6] = x.nxt; out[7] = x.nxt * x.ng;
        out[8] = x.Nkp / 4; out[9] = (int32_t)x.tW; out[10] = 16 * x.nxt * x.ng_use; out[11] = JX_ROP_NW;
        return JX_OK;
    }
    const MixBack& m = ctx->mix;
    out[0] = m.form; out[1] = ctx->qn; out[2] = m.r; out[3] = m.ns; out[4] = m.form == 0 ? m.mx.R : 0; out[5] = m.RT;
    out[6] = m.nxt; out[7] = m.og.ntile; out[8] = m.ksteps; out[9] = (int32_t)m.tW; out[10] = m.og.ldx; out[11] = m.last_ksplit;
    return JX_OK;
}

int jx_get_exact_info(jx_ctx* ctx, int32_t out[8]) {
    if (!ctx || !ctx->finalized || !out) return JX_ERR_STATE;
    const ExactBack& m = ctx->exact;
    if (!m.ready) { ctx->err = "the exact form is not in use"; return JX_ERR_UNSUPPORTED; }
    const bool ct = m.contracted();
    out[0] = ct ? 1 : 0; out[1] = m.ldm; out[2] = 16 * m.nxt * m.ng_use; out[3] = m.last_ct;
    out[4] = 0; out[5] = (int32_t)(sizeof(double) * (ct ? (size_t)JX_ORD_CT_LDS_DOUBLES(m.ndt) : (size_t)JX_ORD_LDS_DOUBLES));
    out[6] = m.f32x ? 1 : 0; out[7] = m.f32x ? m.t_log2 : 0;
    return JX_OK;
}

int jx_debug_workspace(jx_ctx* ctx, int which, void** dev, int32_t geom[4]) {
    if (!ctx || !ctx->finalized || !dev || !geom) return JX_ERR_STATE;
    if (ctx->conv_mode != 2) { ctx->err = "work buffers of the contracted route only"; return JX_ERR_UNSUPPORTED; }
    const MixBack& m = ctx->mix;
    geom[0] = geom[1] = geom[2] = geom[3] = 0;
    if (ctx->exact.ready) {
        const ExactBack& x = ctx->exact;
        if (which == 6) { *dev = x.y; geom[0] = 1; geom[1] = (int)x.tW; geom[2] = x.Nkp; geom[3] = 8; return JX_OK; }
        if (which == 7 && x.pairwise) { *dev = x.f32x ? (void*)x.Opk32 : (void*)x.Opk; geom[0] = x.ng * (x.Nkp / 16) * x.nxt; geom[1] = 64; geom[2] = 4; geom[3] = x.f32x ? 4 : 8; return JX_OK; }
        if (which == 0 && ctx->d_img) { *dev = ctx->d_img; geom[0] = ctx->chunk; geom[1] = ctx->d.q_nb; geom[2] = (int)ctx->d.img_ld; geom[3] = 8; return JX_OK; }
        ctx->err = "exact form: work buffers 6 (ordinates [1][tW][Nkp]) and 7 (row operator of the pair-wise kernels, tile-major [ng nS nxt][64][4]; not with JOXSZ_X_PAIRWISE=0) -- and 0 after a y_2d tap -- exist; the others belong to the contracted forms";
        return JX_ERR_UNSUPPORTED;
    }
    if (which >= 6) { ctx->err = "work buffers 6 and 7 belong to the exact form"; return JX_ERR_UNSUPPORTED; }
    switch (which) {
        case 0: if (!ctx->d_img) { ctx->err = "the map quadrant exists after the first y_2d tap"; return JX_ERR_STATE; }
                *dev = ctx->d_img; geom[0] = ctx->chunk; geom[1] = ctx->d.q_nb; geom[2] = (int)ctx->d.img_ld; geom[3] = 8; break;
        case 1: *dev = m.cft; geom[0] = ctx->cfg.N; geom[1] = (int)m.tW; geom[2] = 2; geom[3] = ctx->f32 ? 4 : 8; break;
        case 2: if (m.form != 0) { ctx->err = "no stage-1 rows in the full form"; return JX_ERR_UNSUPPORTED; }
                *dev = m.Dt; geom[0] = m.mx.NU; geom[1] = m.mx.R; geom[2] = (int)m.tW; geom[3] = ctx->f32c ? 4 : 8; break;
        case 3: *dev = m.Pt; geom[0] = m.last_was_u ? m.ksplit_u : m.last_ksplit; geom[1] = (int)m.tW; geom[2] = m.last_was_u ? m.og_u.ldx : m.og.ldx; geom[3] = ctx->f32c ? 4 : 8; break;
        case 4: if (m.form != 0) { ctx->err = "no stage-1 operator in the full form"; return JX_ERR_UNSUPPORTED; }
                *dev = const_cast<double*>(m.mx.Cm); geom[0] = 1; geom[1] = m.mx.wld; geom[2] = m.mx.cld; geom[3] = 8; break;
        case 5: *dev = const_cast<double*>(m.og.Op); geom[0] = 4 * m.ksteps; geom[1] = 16; geom[2] = m.og.ntile; geom[3] = 8; break;
        default: ctx->err = "unknown work buffer"; return JX_ERR_INVALID;
    }
    return JX_OK;
}

int jx_get_sampling(jx_ctx* ctx, int32_t out[8], int32_t* rows, int nrows_cap) {
    if (!ctx || !ctx->finalized || !out) return JX_ERR_STATE;
    const MixBack& m = ctx->mix;
    const bool on = ctx->conv_mode == 2 && !m.sub.empty();
    out[0] = on ? m.NU_full : (ctx->conv_mode == 2 ? ctx->qn : 0); out[1] = on ? (int)m.sub.size() : out[0];
    out[2] = ctx->sub_u0; out[3] = ctx->sub_u1; out[4] = ctx->sub_npts; out[5] = on ? 1 : 0; out[6] = ctx->trunc_unsub; out[7] = 0;
    if (rows) for (int i = 0; i < nrows_cap && i < out[1]; ++i) rows[i] = on ? m.sub[i] : i;
    return JX_OK;
}

int jx_get_radial_sampling(jx_ctx* ctx, int32_t out[6], int32_t* rows, int nrows_cap) {
    if (!ctx || !ctx->finalized || !out) return JX_ERR_STATE;
    const bool on = ctx->ag_sub_on;
    out[0] = ctx->cfg.N; out[1] = on ? ctx->ag_ns : ctx->cfg.N; out[2] = ctx->ag_u0; out[3] = ctx->ag_u1; out[4] = ctx->ag_npts;
    out[5] = on ? 1 : 0;
    if (rows) for (int i = 0; i < nrows_cap && i < out[1]; ++i) rows[i] = on ? ctx->h_rsub[i] : i;
    return ctx->ag_removed;
}

int jx_get_output_pruning(jx_ctx* ctx, int32_t out[6]) {
    if (!ctx || !ctx->finalized || !out) return JX_ERR_STATE;
    if (ctx->exact.ready) {
        const ExactBack& x = ctx->exact;
        out[0] = ctx->nrow; out[1] = ctx->prune ? ctx->nrow_use : ctx->nrow; out[2] = std::min(16 * x.nxt * x.ng_use, 16 * x.nxt * x.ng);
        out[3] = x.nxt; out[4] = JX_ROP_NW; out[5] = x.ng_use < x.ng ? 1 : 0;
        return JX_OK;
    }
    const MixBack& m = ctx->mix;
    const bool u = ctx->conv_mode == 2 && m.has_u;
    out[0] = ctx->nrow; out[1] = ctx->nrow_use; out[2] = u ? 16 * m.og_u.ntile : ctx->nrow; out[3] = u ? m.nxt_u : 0; out[4] = u ? m.ksplit_u : 0;
    out[5] = u ? 1 : 0;
    return JX_OK;
}

int jx_get_truncation(jx_ctx* ctx, double out[12]) {
    if (!ctx || !ctx->finalized || !out) return JX_ERR_STATE;
    const bool lr = ctx->mix.ready && ctx->mix.form == 0;
    out[0] = lr ? ctx->mix.tol : 0.0; out[1] = ctx->trunc_est[0]; out[2] = lr ? (double)ctx->mix.r : 0.0; out[3] = (double)ctx->trunc_retried;
    out[4] = (double)ctx->trunc_points; out[5] = ctx->trunc_bound; out[6] = ctx->trunc_est[1]; out[7] = ctx->trunc_est[2];
    out[8] = lr ? (double)ctx->mix.r_tol : 0.0; out[9] = ctx->trunc_bound_ll; out[10] = (lr && ctx->mix.mfma) ? 1.0 : 0.0;
    out[11] = (double)ctx->trunc_uncapped;
    return JX_OK;
}

// Duration of the Abel + map kernel writing the full S x S Compton-y map of `nwalkers` walkers (the kernel BASELINE's metric
// is worded around: profile -> Abel integral -> spline -> map, S^2 * 8 B per walker), averaged over `repeats` launches
// between two HIP events on the context's stream.  Scratch image allocated for the call.
namespace {
// scratch of the measurement calls below: device buffers and events released on every path out of the call
struct Scratch {
    std::vector<void*> mem;
    std::vector<hipEvent_t> ev;
    ~Scratch() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); for (void* p : mem) (void)hipFree(p); }
    hipError_t alloc(void** p, size_t n) { const hipError_t e = hipMalloc(p, n); if (e == hipSuccess) mem.push_back(*p); return e; }
    hipError_t event(hipEvent_t* e) { const hipError_t r = hipEventCreate(e); if (r == hipSuccess) ev.push_back(*e); return r; }
};
}  // namespace

int jx_map_kernel_time(jx_ctx* ctx, const double* theta_dev, int nwalkers, int repeats, double* ms_out) {
    if (!ctx || !theta_dev || nwalkers < 1 || repeats < 1 || !ms_out) return JX_ERR_INVALID;
    if (!ctx->finalized) { ctx->err = "jx_map_kernel_time before jx_finalize"; return JX_ERR_STATE; }
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    const size_t S = ctx->cfg.S;
    JxDev dm = ctx->d;
    dm.quad = 0; dm.img_ld = (long long)S; dm.img_ws = (long long)(S * S); dm.cf_out = nullptr; dm.xcol = nullptr;
    dm.map_split = std::max(dm.map_split, 2);                  // (two row slabs per walker: launches desynchronise, stores overlap compute)
    int threads; size_t lds;
    if (!map_geometry(dm, 512, &threads, &lds, ctx->map_pair != 0)) { ctx->err = "radial grid too long for the LDS-resident spline"; return JX_ERR_UNSUPPORTED; }
    Scratch sc;
    double* img = nullptr;
    HIPCHK(ctx, sc.alloc((void**)&img, sizeof(double) * (size_t)nwalkers * S * S));
    hipEvent_t e0, e1;
    HIPCHK(ctx, sc.event(&e0)); HIPCHK(ctx, sc.event(&e1));
    hipStream_t st = ctx->stream;
    launch_map(st, dm, threads, lds, theta_dev, 0, nwalkers, img, nullptr, nullptr, nullptr, false);       // warm-up
    HIPCHK(ctx, hipEventRecord(e0, st));
    for (int i = 0; i < repeats; ++i) launch_map(st, dm, threads, lds, theta_dev, 0, nwalkers, img, nullptr, nullptr, nullptr, false);
    HIPCHK(ctx, hipEventRecord(e1, st));
    HIPCHK(ctx, hipEventSynchronize(e1));
    float ms = 0.f;
    HIPCHK(ctx, hipEventElapsedTime(&ms, e0, e1));
    HIPCHK(ctx, hipGetLastError());
    *ms_out = (double)ms / repeats;
    return JX_OK;
}

// Test hook: the table-driven exp and log of the per-walker kernel (jx_fastmath.hpp) on n host values, through the same tables the
// context uploaded -- what tests/test_gpu_fastmath.py holds to 2 ulp against long double.
__global__ void __launch_bounds__(256) jx_fastmath_kernel(const double* __restrict__ tab, const double* __restrict__ x, double* __restrict__ oe, double* __restrict__ ol, int n) {
    __shared__ double st[JX_FM_TABLE_DOUBLES];
    for (int i = threadIdx.x; i < JX_FM_TABLE_DOUBLES; i += blockDim.x) st[i] = tab[i];
    __syncthreads();
    const JxFm t{st, st + JX_FM_EXP_N};
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { oe[i] = jx_fm_exp(t, x[i]); ol[i] = jx_fm_log(t, x[i]); }
}

int jx_fastmath_eval(jx_ctx* ctx, const double* x, int n, double* exp_out, double* log_out) {
    if (!ctx || !x || n < 1 || !exp_out || !log_out) return JX_ERR_INVALID;
    if (!ctx->finalized) { ctx->err = "jx_fastmath_eval before jx_finalize"; return JX_ERR_STATE; }
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    Scratch sc;
    double *dx = nullptr, *de = nullptr, *dl = nullptr;
    HIPCHK(ctx, sc.alloc((void**)&dx, sizeof(double) * (size_t)n)); HIPCHK(ctx, sc.alloc((void**)&de, sizeof(double) * (size_t)n)); HIPCHK(ctx, sc.alloc((void**)&dl, sizeof(double) * (size_t)n));
    HIPCHK(ctx, hipMemcpyAsync(dx, x, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(jx_fastmath_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, ctx->d.fm_tab, dx, de, dl, n);
    HIPCHK(ctx, hipMemcpyAsync(exp_out, de, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(log_out, dl, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipGetLastError());
    return JX_OK;
}

// What a pair of HIP events around ONE kernel of a dependent chain reads when that kernel does nothing: a one-wave kernel that
// returns at once, between two events, with another such kernel in front and behind (the situation of the stage events of
// jx_timing_enable).  The figure (a few microseconds: the command processor's hand-over between dependent dispatches, which
// rocprofv3's kernel trace does not count into a kernel's duration) is what the HIP-event duration of a short kernel carries on
// top of the kernel itself; bench.py reports it beside `roofline.launch_ms`.
__global__ void jx_null_kernel(int* p) { if (p && threadIdx.x == 1024) *p = 0; }

int jx_event_bracket_time(jx_ctx* ctx, int repeats, double* ms_out) {
    if (!ctx || repeats < 1 || repeats > 256 || !ms_out) return JX_ERR_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    Scratch sc;
    std::vector<hipEvent_t> ev(2 * (size_t)repeats);
    for (auto& e : ev) HIPCHK(ctx, sc.event(&e));
    hipStream_t st = ctx->stream;
    for (int i = 0; i < repeats; ++i) {
        hipLaunchKernelGGL(jx_null_kernel, dim3(1), dim3(64), 0, st, (int*)nullptr);
        HIPCHK(ctx, hipEventRecord(ev[2 * i], st));
        hipLaunchKernelGGL(jx_null_kernel, dim3(1), dim3(64), 0, st, (int*)nullptr);
        HIPCHK(ctx, hipEventRecord(ev[2 * i + 1], st));
        hipLaunchKernelGGL(jx_null_kernel, dim3(1), dim3(64), 0, st, (int*)nullptr);
    }
    HIPCHK(ctx, hipStreamSynchronize(st));
    HIPCHK(ctx, hipGetLastError());
    double sum = 0.0;
    for (int i = 0; i < repeats; ++i) { float ms = 0.f; HIPCHK(ctx, hipEventElapsedTime(&ms, ev[2 * i], ev[2 * i + 1])); sum += ms; }
    *ms_out = sum / repeats;
    return JX_OK;
}

// Device-to-device copy bandwidth of this GPU (read + write bytes per second, in GB/s): `nbytes` copied `repeats` times
// between two scratch buffers by a plain grid-stride kernel (16 B per lane), timed with HIP events on the context's
// stream.  The practical HBM roofline to quote beside the nominal one.
__global__ void __launch_bounds__(256) jx_copy_kernel(const double2* __restrict__ src, double2* __restrict__ dst, size_t n) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) dst[i] = src[i];
}

__global__ void __launch_bounds__(256) jx_fill_kernel(double2* __restrict__ dst, size_t n, double v) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) dst[i] = double2{v, v};
}
__global__ void __launch_bounds__(256) jx_readsum_kernel(const double2* __restrict__ src, double* __restrict__ out, size_t n) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    double s = 0.0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) { const double2 v = src[i]; s += v.x + v.y; }
    if (s == 1.2345e300) out[0] = s;                       // (never: keeps the loads)
}

// mode 0: copy (bytes read + written counted), 1: read stream, 2: write stream.  Launch shapes: the best of
// scripts/ubench/hbm_rates.hip on this chip (a write stream wants FEW blocks: one per CU sweeps memory as one compact window).
int jx_stream_bandwidth(jx_ctx* ctx, int mode, size_t nbytes, int repeats, double* gbps_out) {
    if (!ctx || mode < 0 || mode > 2 || nbytes < 4096 || repeats < 1 || !gbps_out) return JX_ERR_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    Scratch sc;
    void *a = nullptr, *b = nullptr;
    HIPCHK(ctx, sc.alloc(&a, nbytes));
    HIPCHK(ctx, sc.alloc(&b, nbytes));
    hipStream_t st = ctx->stream;
    hipEvent_t e0, e1;
    HIPCHK(ctx, sc.event(&e0)); HIPCHK(ctx, sc.event(&e1));
    HIPCHK(ctx, hipMemsetAsync(a, 0, nbytes, st));
    HIPCHK(ctx, hipMemsetAsync(b, 0, nbytes, st));
    const size_t n = nbytes / sizeof(double2);
    const int per_cu = mode == 2 ? 1 : 4;
    const dim3 grid((unsigned)(ctx->num_cu * per_cu));
    auto go = [&]() {
        if (mode == 0) hipLaunchKernelGGL(jx_copy_kernel, grid, dim3(256), 0, st, (const double2*)a, (double2*)b, n);
        else if (mode == 1) hipLaunchKernelGGL(jx_readsum_kernel, grid, dim3(256), 0, st, (const double2*)a, (double*)b, n);
        else hipLaunchKernelGGL(jx_fill_kernel, grid, dim3(256), 0, st, (double2*)b, n, 1.0);
    };
    go();
    HIPCHK(ctx, hipEventRecord(e0, st));
    for (int i = 0; i < repeats; ++i) go();
    HIPCHK(ctx, hipEventRecord(e1, st));
    HIPCHK(ctx, hipEventSynchronize(e1));
    float ms = 0.f;
    HIPCHK(ctx, hipEventElapsedTime(&ms, e0, e1));
    HIPCHK(ctx, hipGetLastError());
    *gbps_out = (mode == 0 ? 2.0 : 1.0) * (double)(n * sizeof(double2)) * repeats / ((double)ms * 1e-3) / 1e9;
    return JX_OK;
}

int jx_copy_bandwidth(jx_ctx* ctx, size_t nbytes, int repeats, double* gbps_out) {
    if (!ctx || nbytes < 4096 || repeats < 1 || !gbps_out) return JX_ERR_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    Scratch sc;
    void *a = nullptr, *b = nullptr;
    HIPCHK(ctx, sc.alloc(&a, nbytes));
    HIPCHK(ctx, sc.alloc(&b, nbytes));
    hipStream_t st = ctx->stream;
    hipEvent_t e0, e1;
    HIPCHK(ctx, sc.event(&e0)); HIPCHK(ctx, sc.event(&e1));
    HIPCHK(ctx, hipMemsetAsync(a, 0, nbytes, st));
    const size_t n = nbytes / sizeof(double2);
    const dim3 grid((unsigned)(ctx->num_cu * 16));
    hipLaunchKernelGGL(jx_copy_kernel, grid, dim3(256), 0, st, (const double2*)a, (double2*)b, n);
    HIPCHK(ctx, hipEventRecord(e0, st));
    for (int i = 0; i < repeats; ++i) hipLaunchKernelGGL(jx_copy_kernel, grid, dim3(256), 0, st, (const double2*)a, (double2*)b, n);
    HIPCHK(ctx, hipEventRecord(e1, st));
    HIPCHK(ctx, hipEventSynchronize(e1));
    float ms = 0.f;
    HIPCHK(ctx, hipEventElapsedTime(&ms, e0, e1));
    HIPCHK(ctx, hipGetLastError());
    *gbps_out = 2.0 * (double)(n * sizeof(double2)) * repeats / ((double)ms * 1e-3) / 1e9;
    return JX_OK;
}

void jx_destroy(jx_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->cfg.device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (ctx->comm) (void)jx_comm_destroy(ctx);
    fft_teardown(ctx->fft);
    mix_teardown(ctx, ctx->mix);
    exact_teardown(ctx, ctx->exact);
    for (auto& es : ctx->ev_inflight) for (int k = 0; k < 6; ++k) (void)hipEventDestroy(es.e[k]);
    for (auto& es : ctx->ev_free) for (int k = 0; k < 6; ++k) (void)hipEventDestroy(es.e[k]);
    for (auto& pr : ctx->gt_inflight) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
    for (auto& pr : ctx->gt_free) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
    if (ctx->side_stream) { (void)hipStreamSynchronize(ctx->side_stream); (void)hipStreamDestroy(ctx->side_stream); }
    if (ctx->ev_side) (void)hipEventDestroy(ctx->ev_side);
    if (ctx->ev_tail) (void)hipEventDestroy(ctx->ev_tail);
    for (auto& g : ctx->gslot) if (g.done) (void)hipEventDestroy(g.done);
    if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
    if (ctx->comm_stream) (void)hipStreamDestroy(ctx->comm_stream);
    for (void* p : ctx->dev_allocs) (void)hipFree(p);
    for (void* p : ctx->samp_buf) if (p) (void)hipFree(p);
    if (ctx->d_theta) (void)hipFree(ctx->d_theta);
    if (ctx->d_logp) (void)hipFree(ctx->d_logp);
    if (ctx->h_theta) (void)hipHostFree(ctx->h_theta);
    if (ctx->h_logp) (void)hipHostFree(ctx->h_logp);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    if (--g_rocfft_refs == 0) rocfft_cleanup();
    delete ctx;
}

}  // extern "C"
