// Host side of the library, shared by every route: the context (jx_ctx) with its three back ends, error macros, device allocations, options,
// and the per-chunk arguments the routes hand to the per-walker kernel.  Included by joxsz_hip.hip only (one translation unit).
#pragma once
#include <hip/hip_runtime.h>
#include <rocfft/rocfft.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/joxsz_hip.h"
#include "jx_kernels.hpp"
#include "jx_mix.hpp"
#include "jx_exact.hpp"
#include "jx_fft.hpp"
#include "jx_tables.hpp"

namespace {

struct Plan3 {
    rocfft_plan beam_fwd = nullptr, beam_inv = nullptr, tf_fwd = nullptr;         // 2-D plans (JOXSZ_FFT_COLUMNS=rocfft, or a side that is not 2^a 3^b 5^c)
    rocfft_plan row_fwd = nullptr, row_inv = nullptr, row_tf = nullptr;           // batched 1-D row plans beside the column kernels of jx_fft.hpp
};

struct EvSet {
    hipEvent_t e[6];
    int walkers;
    bool op;                           // operator route: only e[0], e[1], e[5] were recorded
    bool p1only = false;               // timing modes 2..4: only e[2], e[3] (around one kernel of the step) were recorded
    int p1stage = 2;                   //   which one: 2 stage 1 (contracted forms) / the ordinate product (exact form), 3 the per-walker kernel, 4 the row product + tail (exact form)
    bool exact = false;                // exact form: e[0], e[1], e[2], e[5] were recorded (per-walker kernel, ordinate product, row product + tail)
};

// rocFFT sequence (jx_host_fft.hpp): constants in the padded full-image layout, work buffers for `cap` walkers, plans per batch size
struct FftBack {
    bool ready = false;
    int cap = 0, P = 0, Ph = 0;
    JxDev d;
    int map_threads = 512;
    size_t map_lds = 0;
    double *img = nullptr, *conv = nullptr;
    double2 *spec = nullptr, *tfspec = nullptr;
    // hand-written column passes (jx_fft.hpp): rows of the padded image kept (S: the zero rows are never stored), leading dimensions of the
    // row spectra (multiples of 8 complex), columns per block, the two transforms, the tables in those leading dimensions, Z of the tail
    bool cols = false, rows_custom = false;
    int rows = 0, ldc = 0, ldt = 0;
    JxFft fP{}, fS{};
    double2 *bhat_p = nullptr, *htab_p = nullptr;
    double* zbuf = nullptr;
    std::map<int, Plan3> plans;
    rocfft_execution_info info = nullptr;
    void* work = nullptr;
    size_t work_cap = 0;
    std::vector<void*> allocs;
};

// contracted forms of rounds 3-4 (jx_host_mix.hpp): tables and work buffers (freed and rebuilt when the truncation probe asks for a tighter cut)
struct MixBack {
    bool ready = false;
    int form = 0;                      // 0 low-rank (stage 1 + stage 2), 1 full operator on the samples (JOXSZ_MIX_FORM=legacy|lowrank|full)
    JxMix mx{};
    JxOpg og{};
    JxOpg og_u{};                      // the product restricted to the outputs the tail reads (nxt_u tiles per block, ksplit_u slices); og: every output (taps)
    int nxt_u = 0, ksplit_u = 0, ksplit_u_force = 0;
    bool has_u = false, last_was_u = false;
    int NU_full = 0;                   // distinct rows of the quadrant (mx.NU: the ones stage 1 evaluates)
    std::vector<int> sub;              // indices of the rows (= columns) stage 1 evaluates; empty: all
    int RT = 0, nxt = 0, r = 0, ns = 0, ksteps = 0, wpb = 4, wpb_force = 0, ksplit_force = 0, last_ksplit = 1, dbg = 0;
    bool mfma = false;                 // stage 1 on the fp64 matrix cores (R <= 16: jx_rowmix_mfma_kernel)
    int r_tol = 0;                     // terms above the singular-value cut (r < r_tol: capped to one 16-row tile)
    long long tW = 0;
    int ncol = 0;
    double tol = 0.0;
    double *cft = nullptr, *Dt = nullptr, *Pt = nullptr;
    std::vector<void*> allocs;
    int64_t bytes = 0;
};

// exact form (jx_host_exact.hpp; kernels: jx_exact.hpp): the ordinate product's operator Typ, the row operator Opk, the ordinates y and the
// partial rows of a chunk
struct ExactBack {
    bool ready = false;                // the exact form is this context's route
    int Nk = 0, Nkp = 0, nxt = 0, ng = 0, ng_use = 0, npair = 0, nSj = 0, ldpp = 0, nfold = 0;
    bool lean = true;                  // JOXSZ_X_FOLD=0 clears it: the timed path then stores the ordinates and forms every tile, like a call with taps
    double *Wfk = nullptr;             // odd number of ordinate tiles: the last one's share of the row as an operator on the profile (timed path; jxt::exact_fold_layout, tile-major)
                                       // Opk: tile-major (jxt::row_tile_major) for the pair-wise kernels; with JOXSZ_X_PAIRWISE=0 in exact_row_layout's own order, for jx_rowop_tail_kernel
    double *Typ = nullptr, *Opk = nullptr, *y = nullptr, *cf = nullptr, *P = nullptr, *ppi = nullptr;
    bool pairwise = true;              // JOXSZ_X_PAIRWISE=0: the ordinates read back by one block per 16 walkers (jx_rowop_tail_kernel)
    bool contract = true;              // JOXSZ_X_CONTRACT=0: the pair-wise kernels exchange partial rows in every call (with it: only in calls with row / brightness taps)
    bool ct_ok = false;                // the contracted epilogue fits this problem (at most JX_CT_NDT tiles of data radii, fewer data radii than outputs)
    int ldm = 0, ndt = 0, last_ct = -1;   // its geometry (JxRowOp); form of the last launch (-1: none yet)
    double *Pm = nullptr, *Eop = nullptr;   // contracted partials [tW / 16][npair][16][ldm]; data-radii matrix as an operand [ng_use][nxt][ndt][64][4]
    // fp32 products (jx_config.dtype 3): the three operators rounded once to fp32 IN PLACE of the fp64 ones (Wfk, Typ, Opk stay null), Eop in the
    // fp32 instruction's output order, and the range guard T = 2^t_log2 on the profile (plan_exact)
    bool f32x = false;
    float *Wfk32 = nullptr, *Typ32 = nullptr, *Opk32 = nullptr;
    int t_log2 = 0;
    long long tW = 0;
    JxRowOp ro{};                      // what every launch's kernel argument shares (exact_setup); run_exact adds the launch's own fields to a copy
    std::vector<void*> allocs;
    int64_t bytes = 0;
    bool contracted() const { return pairwise && contract && ct_ok; }   // calls without row / brightness taps take the contracted epilogue
};

}  // namespace

struct jx_ctx {
    jx_config cfg;
    bool finalized = false;
    std::string err;
    std::string devname;
    hipStream_t stream = nullptr;
    hipStream_t own_stream = nullptr;  // created by jx_create; `stream` may point at a caller's stream instead (jx_set_stream)

    std::map<std::string, std::string> opts;   // jx_set_option (the process environment is the default of every name)

    // host copies of the uploaded tensors
    std::vector<std::vector<unsigned char>> host;
    std::vector<bool> have;

    // derived sizes
    int nrow = 0, nt = 0, Sh = 0, K = 0, chunk = 0, num_cu = 256;
    int nrow_use = 0;                  // outputs of the extracted row the data-radii spline reads with a weight above JX_PRUNE_TOL of its largest (<= nrow)
    bool subsample = true;             // JOXSZ_MIX_SUBSAMPLE=0: stage 1 evaluates every distinct map sample (default: a tensor sub-grid, the rest by interpolation folded into the operators)
    int sub_u0 = 40, sub_u1 = 160, sub_npts = 14;   // full resolution below u0 pixels from the axis, every second row up to u1, every fourth up to 2 u1, every eighth beyond; interpolation points
    bool prune = true;                 // JOXSZ_PRUNE_OUTPUTS=0: the matrix-core product computes every output of the row, read or not
    int64_t device_bytes = 0;
    int conv_mode = 1;                 // 1 rocFFT sequence, 2 exact form (exact.ready) or contracted forms (mix.ready)

    // device constants
    std::vector<void*> dev_allocs;
    JxDev d;
    double* d_par_vals = nullptr;
    int map_threads = 512;
    size_t map_lds = 0;
    bool dmat_mirror = false;
    bool map_ok = true;                // the Abel + map kernel fits its spline in LDS (radial grids up to ~1690 points); without it: no map taps, no rocFFT
                                       // reference facility (guard), profile taps from the matrix product's own arrays
    std::vector<double> h_Qtab;        // [qn][qn] pixel radii of the quadrant (host; table builds)
    int qn = 0;
    std::vector<double> h_G;           // [N][N] moment operator of the mirrored spline (host; table builds)

    // per-walker scalars (chunk capacity)
    double *d_base = nullptr, *d_cfac = nullptr, *d_sz0 = nullptr;
    double* d_xr = nullptr;            // [chunk][2] Cash log-likelihood and reject flag of the two-block form of the per-walker kernel
    bool prep_split = true;            // JOXSZ_PREP_SPLIT=0: one block per walker in the per-walker kernel (as in every call with taps)
    bool prep_lean = true;             // JOXSZ_PREP_LEAN=0: the two-block form runs in jx_prep_kernel itself instead of jx_walker2_kernel (same bits)
    double* d_img = nullptr;           // exact and contracted forms: quadrant of the Compton-y map (y_2d tap only; allocated on first use)
    // spline arrays as one matrix product (jx_abel_gemm_kernel; contracted forms)
    double* d_Tm = nullptr; int tm_ld = 0, tm_ntile = 0, tm_npair = 0;
    double* d_ppc = nullptr;           // [chunk][N] (exact form: [chunk][16 nSj]) prep kernel -> jx_abel_gemm_kernel / jx_ordrow_kernel
    // radial sub-grid of the spline-array product (DESIGN of round 4, 6.3): Tm through the interpolation from the kept radii, their indices, the first k-step of every column tile
    bool ag_sub = true;                // JOXSZ_AG_SUBSAMPLE=0: every radius of the profile; "u0,u1,npts": another sub-grid
    int ag_u0 = 64, ag_u1 = 256, ag_npts = 18;
    bool ag_sub_on = false;            // in use (set by mix_context_tables; the guard of jx_finalize may take it away)
    int ag_ns = 0, ag_removed = 0;
    double* d_Tm_s = nullptr; int* d_rsub = nullptr; int* d_tks = nullptr;
    std::vector<int> h_rsub;
    bool abel_gemm = true;
    bool prep_fastmath = true;         // JOXSZ_PREP_FASTMATH=0: the per-walker kernel's exp / log from the device library instead of jx_fastmath.hpp's tables
    bool ag_single = false;            // JOXSZ_AG_SINGLE=1: one column tile per wave (twice the blocks) in the spline-array product
    int ag_narrow = -1;                // JOXSZ_AG_NARROW: 16-walker blocks of the spline-array product for every launch (1) / never (0)
    bool f32 = false;                  // jx_config.dtype >= 1: fp32 spline arrays, fp32 evaluation of the map samples
    bool f32c = false;                 // jx_config.dtype == 2: fp32 arithmetic in stage 1 and stage 2 as well (packed fp32 FMAs, fp32 matrix cores)
    bool f32x = false;                 // jx_config.dtype == 3: the exact form with its two big products on the fp32 matrix cores (neither f32 nor f32c is set)

    ExactBack exact;                   // conv_mode 2, default
    MixBack mix;                       // conv_mode 2, JOXSZ_MIX_FORM=legacy|lowrank|full (and every f32 context)
    FftBack fft;                       // conv_mode 1: the back end (cap = chunk); conv_mode 2: reference facility (built on first use)

    // truncation guard (contracted forms)
    double trunc_est[3] = {-1.0, -1.0, -1.0};   // measure_truncation: row at the current values, row over the probe points, SZ log-likelihood
    double trunc_bound = 1e-9, trunc_bound_ll = 1e-8;
    int trunc_retried = 0, trunc_points = 0, trunc_uncapped = 0, trunc_unsub = 0;   // rebuilds in all; of which: the cap on the rank taken away
    bool tol_pinned = false;           // JOXSZ_LOWRANK_TOL given: the guard measures but never overrides
    double lr_tol0 = 0.0;              // singular-value cut the low-rank form starts from (parse_options)
    int map_pair = 1;                  // full-map kernel: two walkers per block (JOXSZ_MAP_PAIR=0: one)
    int usplit = 2;                    // pieces a map column is walked in by stage 1 (JOXSZ_MIX_USPLIT: 1..4; a setting, never a function of the launch)
    bool usplit_forced = false;        // (otherwise plan_mix picks it from the columns stage 1 walks and the chunk)
    int rank_cap = 16;                 // low-rank form: a rank within JX_MIX_CAP_REACH terms above this is cut to it, so that stage 1 fits one 16-row matrix-core
                                       // tile (the guard measures the result and takes the cap away when it costs accuracy; JOXSZ_MIX_RANKCAP=0: never)
    bool mix_mfma = false;             // JOXSZ_MIX_MFMA=1: stage 1 on the fp64 matrix cores when R <= 16 (measured slower than the vector-unit kernel: DESIGN of round 4, 6.1)

    // batch staging for the host-pointer API
    double *d_theta = nullptr, *d_logp = nullptr;
    double *h_theta = nullptr, *h_logp = nullptr;   // pinned host staging of jx_eval (a pageable hipMemcpyAsync stages and synchronises by itself)
    double *hd_theta = nullptr, *hd_logp = nullptr; // the same two buffers as the device sees them (mapped, coherent)
    int eval_direct = 3;                            // JOXSZ_EVAL_DIRECT bit 0: the tail writes the log-probabilities into the host buffer itself; bit 1: the per-walker kernel reads theta from it
    int batch_cap = 0;
    // taps (chunk capacity, allocated on first use)
    double *t_pp = nullptr, *t_ab = nullptr, *t_y = nullptr, *t_row = nullptr, *t_bright = nullptr,
           *t_chisq = nullptr, *t_tprof = nullptr, *t_xprofs = nullptr, *t_parts = nullptr, *t_integ = nullptr, *t_y2d = nullptr;
    void* samp_buf[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // jx_sample work buffers (grow-only)
    size_t samp_cap[8] = {0, 0, 0, 0, 0, 0, 0, 0};

    // collapsed route (jx_set_route): Gt [N][g_ld], row j = map row of the unit pressure profile e_j
    int route = JX_ROUTE_MAP;
    double* d_G = nullptr;
    double* d_pp = nullptr;            // [op_cap][N] pressure profiles, prep kernel -> operator kernel
    double *d_base_op = nullptr, *d_cfac_op = nullptr, *d_sz0_op = nullptr;
    double* d_rows = nullptr;          // [op_cap / 32][nrow][32] G pp of large launches (jx_operator_mfma_kernel)
    int op_cap = 0, g_ld = 0;
    bool op_narrow = false;            // JOXSZ_OP_NARROW: the small-launch operator kernel for every launch size

    ncclComm_t comm = nullptr;         // RCCL communicator of this rank (jx_comm_init_rank)
    int comm_rank = 0, comm_size = 1;
    // the per-walker kernel beside the SZ chain (contracted forms): second stream, joined in front of the tail
    bool side_on = false;              // JOXSZ_SIDE_STREAM=1: the per-walker kernel on a second stream beside the SZ chain (measured: no gain, profiles/r04_side_stream_timeline.log)
    int side_fork = 0;                 // where the side stream forks: 0 behind the profile kernel, 1 behind stage 1 (JOXSZ_SIDE_FORK)
    hipStream_t side_stream = nullptr;
    hipEvent_t ev_side = nullptr, ev_tail = nullptr;
    // overlapped gather (jx_comm_set_overlap): the collectives of the communicator run on a stream of their own, ordered
    // behind the evaluation by an event; a send buffer still being gathered holds back the next evaluation that writes it
    bool comm_overlap = false;
    hipStream_t comm_stream = nullptr;
    struct GatherSlot { const char* send = nullptr; size_t bytes = 0; hipEvent_t done = nullptr; bool busy = false; };
    GatherSlot gslot[4];
    hipEvent_t ev_fork = nullptr;      // compute stream -> collective stream
    std::vector<std::pair<hipEvent_t, hipEvent_t>> gt_inflight, gt_free;   // events around every all-gather (its own duration)
    double gather_ms = 0.0; long long gather_calls = 0;

    // timing
    bool timing_on = false;
    int timing_mode = 0;               // jx_timing_enable: 1 = every stage, 2 = only the events around the time-dominant kernel
    std::vector<EvSet> ev_inflight, ev_free;
    jx_timing acc{};
};

static const char* opt_str(const jx_ctx* ctx, const char* name) {
    if (ctx) { const auto it = ctx->opts.find(name); if (it != ctx->opts.end()) return it->second.empty() ? nullptr : it->second.c_str(); }
    const char* e = getenv(name);
    return (e && e[0]) ? e : nullptr;
}

#define HIPCHK(ctx, call)                                                                          \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess) {                                                                    \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);                        \
            return (e_ == hipErrorOutOfMemory) ? JX_ERR_NOMEM : JX_ERR_HIP;                        \
        }                                                                                          \
    } while (0)

#define FFTCHK(ctx, call)                                                                          \
    do {                                                                                           \
        rocfft_status s_ = (call);                                                                 \
        if (s_ != rocfft_status_success) {                                                         \
            (ctx)->err = std::string(#call) + ": rocfft status " + std::to_string((int)s_);        \
            return JX_ERR_ROCFFT;                                                                  \
        }                                                                                          \
    } while (0)

// allocations: `list` = the owner's list (context, or a back end that can be torn down on its own)
template <typename T>
static int dev_put_l(jx_ctx* ctx, std::vector<void*>& list, const T* src, size_t count, T** out) {
    void* p = nullptr;
    HIPCHK(ctx, hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(T)));
    list.push_back(p);
    ctx->device_bytes += (int64_t)(count * sizeof(T));
    if (count) HIPCHK(ctx, hipMemcpy(p, src, count * sizeof(T), hipMemcpyHostToDevice));
    *out = (T*)p;
    return JX_OK;
}
template <typename T>
static int dev_new_l(jx_ctx* ctx, std::vector<void*>& list, size_t count, T** out, bool zero = false) {
    void* p = nullptr;
    HIPCHK(ctx, hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(T)));
    list.push_back(p);
    ctx->device_bytes += (int64_t)(count * sizeof(T));
    if (zero) {
        // hipMemset of device memory returns before the fill has run, on the null stream; the context's streams are non-blocking
        // and do not wait for it.  Finish it here: the first writer of the buffer may be the very next call on one of them.
        HIPCHK(ctx, hipMemset(p, 0, count * sizeof(T)));
        HIPCHK(ctx, hipStreamSynchronize(nullptr));
    }
    *out = (T*)p;
    return JX_OK;
}
template <typename T> static int dev_put(jx_ctx* ctx, const T* src, size_t count, T** out) { return dev_put_l(ctx, ctx->dev_allocs, src, count, out); }
template <typename T> static int dev_new(jx_ctx* ctx, size_t count, T** out, bool zero = false) { return dev_new_l(ctx, ctx->dev_allocs, count, out, zero); }

template <typename T>
static std::vector<T> host_vec(jx_ctx* ctx, int id) {
    const auto& b = ctx->host[id];
    std::vector<T> v(b.size() / sizeof(T));
    if (!v.empty()) memcpy(v.data(), b.data(), b.size());
    return v;
}

// Every switch of the library: set per context with jx_set_option (before jx_finalize for those it reads, which is all but the two
// SAMPLE_ ones), with the process environment as the default of each.  The list is the one include/joxsz_hip.h documents
// (tests/test_abi.py holds the two and the uses in csrc/ together).
static const char* const kOptions[] = {
    "JOXSZ_CONV", "JOXSZ_MIX_FORM", "JOXSZ_X_PAIRWISE", "JOXSZ_X_CONTRACT", "JOXSZ_X_FOLD", "JOXSZ_PRUNE_OUTPUTS", "JOXSZ_CHUNK", "JOXSZ_FFT_PAD", "JOXSZ_FFT_COLUMNS", "JOXSZ_FFT_ROWS", "JOXSZ_MAP_SPLIT", "JOXSZ_MAP_PAIR",
    "JOXSZ_EVAL_DIRECT", "JOXSZ_PREP_SPLIT", "JOXSZ_PREP_LEAN", "JOXSZ_PREP_POW", "JOXSZ_PREP_FASTMATH", "JOXSZ_OP_NARROW", "JOXSZ_SAMPLE_FUSED", "JOXSZ_SAMPLE_VIRTUAL_RANKS",
    // the contracted forms of rounds 3-4 (JOXSZ_MIX_FORM=legacy|lowrank|full)
    "JOXSZ_LOWRANK_TOL", "JOXSZ_TRUNC_PROBE", "JOXSZ_TRUNC_BOUND", "JOXSZ_MIX_SUBSAMPLE", "JOXSZ_MIX_RANKCAP", "JOXSZ_MIX_MFMA", "JOXSZ_MIX_USPLIT", "JOXSZ_MIX_WPB",
    "JOXSZ_MIX_KSPLIT", "JOXSZ_MIX_KSPLIT_USE", "JOXSZ_ABEL_GEMM", "JOXSZ_AG_NARROW", "JOXSZ_AG_SINGLE", "JOXSZ_AG_SUBSAMPLE", "JOXSZ_SIDE_STREAM", "JOXSZ_SIDE_FORK",
    // diagnostic build only (make ABLATIONS=1): timing experiments, results are wrong
    "JOXSZ_DBG", "JOXSZ_MIX_DBG", "JOXSZ_X_STAMPS", "JOXSZ_P_STAMPS",
};

struct Taps {
    double *pp = nullptr, *ab = nullptr, *y = nullptr, *row = nullptr, *bright = nullptr, *chisq = nullptr,
           *tprof = nullptr, *xprofs = nullptr, *parts = nullptr, *integ = nullptr;
    bool need_img = false;            // the Compton-y map itself is wanted (y_2d tap)
    bool need_conv = false;           // the beam-convolved map is wanted (conv_2d tap): the hand-written row kernels write it only then
    bool profiles() const { return pp || ab || y; }
    bool any() const { return profiles() || row || bright || chisq || tprof || xprofs || parts || integ || need_img; }
};

// One chunk as run_chunk hands it to its route: walkers [w0, w0+n) of the batch at theta, the route's JxDev, where the per-walker kernel writes,
// the stretch move (zero outside jx_sample), the launch's event set (recorded into where tm / tm2 say so).  The route sets xr_split before it
// launches that kernel.
struct Chunk {
    hipStream_t st;
    const JxDev& d;
    const double* theta;
    double* logp;
    int w0, n;
    const Taps& t;
    JxSm sm;
    double *base, *cfac, *sz0;         // (sz0: null unless calc_integ)
    EvSet* es;
    bool tm, tm2;                      // every stage between events / only the kernel es->p1stage names
    bool xr_split = false;             // two blocks per walker in the per-walker kernel (the X-ray side beside the rest)
};

// shared by the routes, defined in joxsz_hip.hip
static int run_chunk(jx_ctx* ctx, const double* theta_dev, double* logp_dev, int w0, int n, const Taps& t, bool use_ref = false, const JxSm* smp = nullptr);
static void launch_map(hipStream_t st, const JxDev& dm_in, int threads, size_t lds, const double* theta_dev, int w0, int n, double* img,
                       double* tpp, double* tab, double* ty, bool coef_only);
static bool map_geometry(JxDev& d, int want_threads, int* threads_out, size_t* lds_out, bool pair_full = false);
static bool prep_splits(const jx_ctx* ctx, const Chunk& c);
static void launch_prep(jx_ctx* ctx, const Chunk& c, hipStream_t ps, double* pp_buf, int pp_ld, int ncf);
static int launch_y2d(jx_ctx* ctx, const Chunk& c);
static int ensure_batch(jx_ctx* ctx, int n);
static int ensure_taps(jx_ctx* ctx);
static int ensure_ref(jx_ctx* ctx);
static Taps all_taps(jx_ctx* ctx, bool profiles);

// ---------------------------------------------------------------------------------------------------------------------
// What the exact form and the contracted forms share of their plans: the checks (mirror structure, no padding parameter, quadrant size,
// the symmetric map kernel's range), the real transfer-function weights A of the extracted row, the tiling of the outputs (all / in use)
// ---------------------------------------------------------------------------------------------------------------------
#define JX_MIX_NXTS(X) X(1) X(2) X(3) X(4) X(5) X(6)
struct PlanShared {
    int NU = 0;
    int nxt = 0, nog = 0, ntile = 0;
    int nxt_u = 0, nog_u = 0, ntile_u = 0;     // tiling of the outputs in use (0: all of them)
    std::vector<double> A;                     // [S][Sh]
};

static void mix_output_tiling(int nrow, int* nxt, int* nog, int* ntile) {
    const int tiles = (nrow + 15) / 16;
    double best = 1e300;
#define JX_PICK(Xv) { const int og = (tiles + Xv - 1) / Xv; const double cost = (double)og * Xv * (1.0 + 0.5 / Xv); if (cost < best) { best = cost; *nxt = Xv; *nog = og; } }
    JX_MIX_NXTS(JX_PICK)
#undef JX_PICK
    *ntile = *nog * *nxt;
}

// Which form a context of conv_mode 2 takes: 2 exact (default); the contracted forms of rounds 3-4: -1 legacy (the cheaper of the two),
// 0 lowrank, 1 full -- as JOXSZ_MIX_FORM says, and instead of the exact form where that one does not exist
enum { JX_FORM_LEGACY = -1, JX_FORM_LOWRANK = 0, JX_FORM_FULL = 1, JX_FORM_EXACT = 2 };
static int choose_form(const jx_ctx* ctx) {
    int form = JX_FORM_EXACT;
    if (const char* e = opt_str(ctx, "JOXSZ_MIX_FORM")) {
        if (!strcmp(e, "lowrank")) form = JX_FORM_LOWRANK; else if (!strcmp(e, "full")) form = JX_FORM_FULL;
        else if (!strcmp(e, "legacy")) form = JX_FORM_LEGACY; else if (!strcmp(e, "exact")) form = JX_FORM_EXACT;
    }
    if (form != JX_FORM_EXACT) return form;
    if (ctx->f32) return JX_FORM_LEGACY;                         // (the fp32 variants 1 and 2 exist on the forms of rounds 3-4; dtype 3 is the exact form's own)
    // (the row of 16 walkers and the eight waves' partial tiles have to fit the LDS of the row product: data radii reaching
    //  across a very large map go to the contracted forms)
    const int nrow = ctx->nrow, nuse0 = std::min(ctx->prune ? std::max(1, ctx->nrow_use) : nrow, nrow);
    if (sizeof(double) * JX_RST_LDS_DOUBLES((nuse0 + 1) | 1, ctx->cfg.nflux, 0) > (size_t)158 * 1024) return JX_FORM_LEGACY;
    return JX_FORM_EXACT;
}

// false: `why` says what the input lacks (both forms then leave the problem to the rocFFT sequence)
static bool plan_shared(const jx_ctx* ctx, const std::vector<double>& filt, PlanShared& sh, std::string& why) {
    const jx_config& c = ctx->cfg;
    const int S = c.S, Sh = S / 2 + 1, nrow = S - S / 2;
    if (!ctx->dmat_mirror) { why = "d_mat lacks the mirror structure of centdistmat"; return false; }
    if (c.fft_pad != 0) { why = "fft_pad is a parameter of the rocFFT sequence"; return false; }
    const int NU = std::max(S / 2, S - 1 - S / 2) + 1;
    if (ctx->qn != NU) { why = "quadrant table size"; return false; }
    if (NU > 9 * 64) { why = "map side beyond the symmetric map kernel's range"; return false; }
    sh.NU = NU;
    mix_output_tiling(nrow, &sh.nxt, &sh.nog, &sh.ntile);
    if (ctx->prune && ctx->nrow_use > 0 && (ctx->nrow_use + 15) / 16 < (nrow + 15) / 16) mix_output_tiling(ctx->nrow_use, &sh.nxt_u, &sh.nog_u, &sh.ntile_u);
    // transfer-function weights of the extracted row, real for a real filter that is symmetric in each wavenumber
    std::vector<double> hy;
    jxt::tf_hy_table(filt, S, hy);
    sh.A.resize((size_t)S * Sh);
    double maxre = 0.0, maxim = 0.0;
    for (size_t e = 0; e < sh.A.size(); ++e) { sh.A[e] = hy[2 * e]; maxre = std::max(maxre, std::fabs(hy[2 * e])); maxim = std::max(maxim, std::fabs(hy[2 * e + 1])); }
    if (!(maxim <= 1e-15 * maxre)) { why = "transfer-function weights are not real"; return false; }
    return true;
}
