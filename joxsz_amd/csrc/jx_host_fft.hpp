// Host side of the rocFFT sequence (kernels: jx_fft.hpp, jx_kernels.hpp): tables, work buffers, plans per batch size, and the launch
// sequence of one chunk (run_fft) -- a context's own route (conv_mode 1) or the reference facility inside an exact / contracted context.
#pragma once
#include "jx_ctx.hpp"

static void fft_teardown(FftBack& fb) {
    for (auto& kv : fb.plans) {
        if (kv.second.beam_fwd) rocfft_plan_destroy(kv.second.beam_fwd);
        if (kv.second.beam_inv) rocfft_plan_destroy(kv.second.beam_inv);
        if (kv.second.tf_fwd) rocfft_plan_destroy(kv.second.tf_fwd);
        if (kv.second.row_fwd) rocfft_plan_destroy(kv.second.row_fwd);
        if (kv.second.row_inv) rocfft_plan_destroy(kv.second.row_inv);
        if (kv.second.row_tf) rocfft_plan_destroy(kv.second.row_tf);
    }
    fb.plans.clear();
    if (fb.info) { rocfft_execution_info_destroy(fb.info); fb.info = nullptr; }
    for (void* p : fb.allocs) (void)hipFree(p);
    fb.allocs.clear();
    if (fb.work) { (void)hipFree(fb.work); fb.work = nullptr; fb.work_cap = 0; }
    fb.ready = false;
}

static int fft_factor(int n, int* radix) { return jxt::fft_radices(n, radix, JX_FFT_MAXPASS); }

static int fft_transform(jx_ctx* ctx, FftBack& fb, int n, JxFft& f) {
    f.n = n;
    f.npass = fft_factor(n, f.radix);
    for (int p = 0, ns = 1; p < f.npass; ns *= f.radix[p++]) {
        f.ns[p] = ns;
        f.tstep[p] = p ? n / (ns * f.radix[p]) : 0;
        f.magic[p] = ns > 1 ? (unsigned)((((unsigned long long)1 << 32) + ns - 1) / ns) : 0u;
    }
    std::vector<double> root((size_t)2 * n);
    for (int m = 0; m < n; ++m) {
        const long double a = -2.0L * 3.14159265358979323846264338327950288L * (long double)m / (long double)n;
        root[2 * m] = (double)cosl(a); root[2 * m + 1] = (double)sinl(a);
    }
    double* p;
    int rc;
    if ((rc = dev_put_l(ctx, fb.allocs, root.data(), root.size(), &p))) return rc;
    f.root = reinterpret_cast<const double2*>(p);
    return JX_OK;
}

// the column kernels come per rows-per-lane bound NU = ceil(length / 64): 8 columns per block up to 640, 4 beyond
#define JX_FFT_NU_OF(n) (((n) + 63) / 64)
#define JX_FFT_DISPATCH(nu, X) do {                                                                                     \
        const int nu_ = (nu);                                                                                           \
        if (nu_ <= 4) { X(8, 4); } else if (nu_ <= 8) { X(8, 8); } else if (nu_ <= 9) { X(8, 9); } else if (nu_ <= 10) { X(8, 10); }   \
        else if (nu_ <= 16) { X(4, 16); } else if (nu_ <= 17) { X(4, 17); } else { X(4, 20); }                         \
    } while (0)
static inline int fft_cb(int n) { return JX_FFT_NU_OF(n) <= 10 ? 8 : 4; }
// the roots of unity go to LDS when two blocks still fit a compute unit with them
static inline int fft_roots_in_lds(int n) { return JX_FFT_SMALL(JX_FFT_NU_OF(n)) ? 1 : 0; }

static void fft_launch_beam(FftBack& fb, int walkers, hipStream_t st, int S) {
    const int P = fb.P, r = fft_roots_in_lds(P);
#define X(CB, NU) hipLaunchKernelGGL((jx_fft_beam_cols_kernel<CB, NU>), dim3(walkers, fb.ldc / CB), dim3(64 * CB), JX_FFT_LDS_BYTES(P, CB, r), st, fb.fP, fb.spec, fb.bhat_p, S, fb.ldc)
    JX_FFT_DISPATCH(JX_FFT_NU_OF(P), X);
#undef X
}

static void fft_launch_tf(FftBack& fb, int walkers, hipStream_t st, int Sh) {
    const int S = fb.fS.n, r = fft_roots_in_lds(S);
#define X(CB, NU) hipLaunchKernelGGL((jx_fft_tf_cols_kernel<CB, NU>), dim3(walkers, fb.ldt / CB), dim3(64 * CB), JX_FFT_LDS_BYTES(S, CB, r), st, fb.fS, fb.tfspec, fb.htab_p, fb.ldt, Sh, fb.zbuf, r)
    JX_FFT_DISPATCH(JX_FFT_NU_OF(S), X);
#undef X
}

// row kernels: 8 waves (pairs of rows) per block for the forward pass, 7 for the fused inverse + window + forward one (its second table of
// roots takes the room of the eighth); 4 where the roots stay in global memory
#define JX_FFT_ROWS_DISPATCH(nu, WS, X) do {                                                                            \
        const int nu_ = (nu);                                                                                           \
        if (nu_ <= 4) { X(WS, 4); } else if (nu_ <= 8) { X(WS, 8); } else if (nu_ <= 9) { X(WS, 9); } else if (nu_ <= 10) { X(WS, 10); }   \
        else if (nu_ <= 16) { X(4, 16); } else if (nu_ <= 17) { X(4, 17); } else { X(4, 20); }                         \
    } while (0)

static void fft_launch_rows_fwd(FftBack& fb, int walkers, hipStream_t st, int S) {
    const int P = fb.P, R = walkers * S, small = fft_roots_in_lds(P);
#define X(WPB, NU) hipLaunchKernelGGL((jx_fft_rows_fwd_kernel<WPB, NU>), dim3(((R + 1) / 2 + WPB - 1) / WPB), dim3(64 * WPB), JX_FFT_ROWS_LDS_BYTES(P, WPB, small ? P : 0), st, \
                                      fb.fP, fb.img, fb.spec, S, fb.ldc, R)
    JX_FFT_ROWS_DISPATCH(JX_FFT_NU_OF(P), 8, X);
#undef X
}

static void fft_launch_rows_inv_tf(FftBack& fb, int walkers, hipStream_t st, int S, bool want_conv) {
    const int P = fb.P, R = walkers * S, small = fft_roots_in_lds(P);
#define X(WPB, NU) hipLaunchKernelGGL((jx_fft_rows_inv_tf_kernel<WPB, NU>), dim3(((R + 1) / 2 + WPB - 1) / WPB), dim3(64 * WPB), JX_FFT_ROWS_LDS_BYTES(P, WPB, small ? P + S : 0), st, \
                                      fb.fP, fb.fS, fb.spec, want_conv ? fb.conv : (double*)nullptr, fb.tfspec, fb.ldc, fb.ldt, R)
    JX_FFT_ROWS_DISPATCH(JX_FFT_NU_OF(P), 7, X);
#undef X
}

static int fft_kernels(jx_ctx* ctx, FftBack& fb) {
    // the attribute belongs to the kernel instance, not to the context: another context of the process may launch the same instance with a
    // longer transform, so every instance is allowed the whole LDS of a compute unit (as the Abel + map kernel is)
    const int S = ctx->cfg.S, lds = 160 * 1024 - 1024;
#define X(CB, NU) HIPCHK(ctx, hipFuncSetAttribute((const void*)jx_fft_beam_cols_kernel<CB, NU>, hipFuncAttributeMaxDynamicSharedMemorySize, lds))
    JX_FFT_DISPATCH(JX_FFT_NU_OF(fb.P), X);
#undef X
#define X(CB, NU) HIPCHK(ctx, hipFuncSetAttribute((const void*)jx_fft_tf_cols_kernel<CB, NU>, hipFuncAttributeMaxDynamicSharedMemorySize, lds))
    JX_FFT_DISPATCH(JX_FFT_NU_OF(S), X);
#undef X
#define X(WPB, NU) HIPCHK(ctx, hipFuncSetAttribute((const void*)jx_fft_rows_fwd_kernel<WPB, NU>, hipFuncAttributeMaxDynamicSharedMemorySize, lds))
    JX_FFT_ROWS_DISPATCH(JX_FFT_NU_OF(fb.P), 8, X);
#undef X
#define X(WPB, NU) HIPCHK(ctx, hipFuncSetAttribute((const void*)jx_fft_rows_inv_tf_kernel<WPB, NU>, hipFuncAttributeMaxDynamicSharedMemorySize, lds))
    JX_FFT_ROWS_DISPATCH(JX_FFT_NU_OF(fb.P), 7, X);
#undef X
    return JX_OK;
}

// tables (beam spectrum, transfer-function row table) and work buffers for `cap` walkers; P = padded side
static int fft_setup(jx_ctx* ctx, FftBack& fb, int cap, int P) {
    const jx_config& c = ctx->cfg;
    const int S = c.S, B = c.B;
    int rc;
    fb.cap = cap; fb.P = P; fb.Ph = P / 2 + 1;
    fb.d = ctx->d;
    JxDev& d = fb.d;
    d.P = P; d.Ph = fb.Ph;
    // column passes: hand-written (jx_fft.hpp) when both sides are 2^a 3^b 5^c and short enough for one column per 32 / 64 threads
    {
        int rx[JX_FFT_MAXPASS];
        const char* e = opt_str(ctx, "JOXSZ_FFT_COLUMNS");
        const bool want = !(e && !strcmp(e, "rocfft"));
        fb.cols = want && fft_factor(P, rx) > 1 && fft_factor(S, rx) > 1 && std::max(P, S) <= JX_FFT_MAX_PER_THREAD * 64 && P % 2 == 0;
        const char* er = opt_str(ctx, "JOXSZ_FFT_ROWS");
        fb.rows_custom = fb.cols && !(er && !strcmp(er, "rocfft"));
        fb.rows = fb.cols ? S : P;
        fb.ldc = (fb.Ph + 7) & ~7; fb.ldt = (ctx->Sh + 7) & ~7;
    }
    d.quad = 0; d.img_ld = P; d.img_ws = (long long)fb.rows * P; d.cf_out = nullptr; d.xcol = nullptr;
    if (!map_geometry(d, 512, &fb.map_threads, &fb.map_lds, ctx->map_pair != 0)) { ctx->err = "radial grid too long for the LDS-resident spline"; return JX_ERR_UNSUPPORTED; }
    {
        std::vector<double> beam = host_vec<double>(ctx, JX_T_BEAM_2D), bh, H;
        jxt::beam_spectrum(beam, B, P, c.step * c.step / ((double)P * (double)P), bh);
        double* p;
        if ((rc = dev_put_l(ctx, fb.allocs, bh.data(), bh.size(), &p))) return rc; d.bhat = p;
        jxt::tf_row_table(host_vec<double>(ctx, JX_T_FILTERING), S, H);
        if ((rc = dev_put_l(ctx, fb.allocs, H.data(), H.size(), &p))) return rc; d.htab = p;
        if (fb.cols) {
            // the two tables one column after the other (the lanes of a column's wave read consecutive entries), zero in the padding columns
            std::vector<double> bp((size_t)2 * P * fb.ldc, 0.0), hp((size_t)2 * S * fb.ldt, 0.0);
            for (int y = 0; y < P; ++y)
                for (int x = 0; x < fb.Ph; ++x) { bp[2 * ((size_t)x * P + y)] = bh[2 * ((size_t)y * fb.Ph + x)]; bp[2 * ((size_t)x * P + y) + 1] = bh[2 * ((size_t)y * fb.Ph + x) + 1]; }
            for (int y = 0; y < S; ++y)
                for (int x = 0; x < ctx->Sh; ++x) { hp[2 * ((size_t)x * S + y)] = H[2 * ((size_t)y * ctx->Sh + x)]; hp[2 * ((size_t)x * S + y) + 1] = H[2 * ((size_t)y * ctx->Sh + x) + 1]; }
            if ((rc = dev_put_l(ctx, fb.allocs, bp.data(), bp.size(), &p))) return rc; fb.bhat_p = reinterpret_cast<double2*>(p);
            if ((rc = dev_put_l(ctx, fb.allocs, hp.data(), hp.size(), &p))) return rc; fb.htab_p = reinterpret_cast<double2*>(p);
            if ((rc = fft_transform(ctx, fb, P, fb.fP))) return rc;
            if ((rc = fft_transform(ctx, fb, S, fb.fS))) return rc;
            if ((rc = dev_new_l(ctx, fb.allocs, (size_t)cap * 2 * ctx->Sh, &fb.zbuf))) return rc;
            if ((rc = fft_kernels(ctx, fb))) return rc;
        }
    }
    const size_t R = fb.rows;
    if ((rc = dev_new_l(ctx, fb.allocs, (size_t)cap * R * P, &fb.img, true))) return rc;       // padding stays zero for ever
    if ((rc = dev_new_l(ctx, fb.allocs, (size_t)cap * R * P, &fb.conv))) return rc;
    if ((rc = dev_new_l(ctx, fb.allocs, fb.cols ? (size_t)cap * S * fb.ldc : (size_t)cap * P * fb.Ph, &fb.spec, fb.cols))) return rc;
    if ((rc = dev_new_l(ctx, fb.allocs, fb.cols ? (size_t)cap * S * fb.ldt : (size_t)cap * S * ctx->Sh, &fb.tfspec, fb.cols))) return rc;
    FFTCHK(ctx, rocfft_execution_info_create(&fb.info));
    FFTCHK(ctx, rocfft_execution_info_set_stream(fb.info, ctx->stream));
    HIPCHK(ctx, hipDeviceSynchronize());                        // (the zero fills ran on the null stream)
    fb.ready = true;
    return JX_OK;
}

static int fft_plans(jx_ctx* ctx, FftBack& fb, int batch, Plan3** out) {
    auto it = fb.plans.find(batch);
    if (it != fb.plans.end()) { *out = &it->second; return JX_OK; }
    Plan3 pl;
    const size_t P = fb.P, S = ctx->cfg.S, Sh = ctx->Sh;
    rocfft_plan p1, p2, p3;
    if (fb.cols) {
        // rows only: img [batch * S][P] -> spec [batch * S][ldc]; spec -> conv [batch * S][P]; conv's first S columns -> tfspec [batch * S][ldt]
        auto row_plan = [&](rocfft_plan* out, bool inverse, size_t len, size_t rdist, size_t cdist) -> int {
            rocfft_plan_description desc = nullptr;
            FFTCHK(ctx, rocfft_plan_description_create(&desc));
            size_t one[1] = {1};
            if (!inverse) FFTCHK(ctx, rocfft_plan_description_set_data_layout(desc, rocfft_array_type_real, rocfft_array_type_hermitian_interleaved,
                                                                              nullptr, nullptr, 1, one, rdist, 1, one, cdist));
            else FFTCHK(ctx, rocfft_plan_description_set_data_layout(desc, rocfft_array_type_hermitian_interleaved, rocfft_array_type_real,
                                                                     nullptr, nullptr, 1, one, cdist, 1, one, rdist));
            size_t l[1] = {len};
            FFTCHK(ctx, rocfft_plan_create(out, rocfft_placement_notinplace, inverse ? rocfft_transform_type_real_inverse : rocfft_transform_type_real_forward,
                                           rocfft_precision_double, 1, l, (size_t)batch * S, desc));
            rocfft_plan_description_destroy(desc);
            return JX_OK;
        };
        int rc;
        if ((rc = row_plan(&pl.row_fwd, false, P, P, fb.ldc))) return rc;
        if ((rc = row_plan(&pl.row_inv, true, P, P, fb.ldc))) return rc;
        if ((rc = row_plan(&pl.row_tf, false, S, P, fb.ldt))) return rc;
        p1 = pl.row_fwd; p2 = pl.row_inv; p3 = pl.row_tf;
    } else {
    {   // beam convolution forward: real [P][P] -> hermitian [P][Ph]
        size_t len[2] = {P, P};
        FFTCHK(ctx, rocfft_plan_create(&pl.beam_fwd, rocfft_placement_notinplace, rocfft_transform_type_real_forward,
                                       rocfft_precision_double, 2, len, (size_t)batch, nullptr));
        FFTCHK(ctx, rocfft_plan_create(&pl.beam_inv, rocfft_placement_notinplace, rocfft_transform_type_real_inverse,
                                       rocfft_precision_double, 2, len, (size_t)batch, nullptr));
    }
    {   // transfer function forward: real S x S window of the padded image (row stride P)
        rocfft_plan_description desc = nullptr;
        FFTCHK(ctx, rocfft_plan_description_create(&desc));
        size_t istr[2] = {1, P}, ostr[2] = {1, Sh};
        FFTCHK(ctx, rocfft_plan_description_set_data_layout(desc, rocfft_array_type_real, rocfft_array_type_hermitian_interleaved,
                                                            nullptr, nullptr, 2, istr, P * P, 2, ostr, S * Sh));
        size_t len[2] = {S, S};
        FFTCHK(ctx, rocfft_plan_create(&pl.tf_fwd, rocfft_placement_notinplace, rocfft_transform_type_real_forward,
                                       rocfft_precision_double, 2, len, (size_t)batch, desc));
        rocfft_plan_description_destroy(desc);
    }
        p1 = pl.beam_fwd; p2 = pl.beam_inv; p3 = pl.tf_fwd;
    }
    size_t w1 = 0, w2 = 0, w3 = 0;
    FFTCHK(ctx, rocfft_plan_get_work_buffer_size(p1, &w1));
    FFTCHK(ctx, rocfft_plan_get_work_buffer_size(p2, &w2));
    FFTCHK(ctx, rocfft_plan_get_work_buffer_size(p3, &w3));
    const size_t need = std::max(w1, std::max(w2, w3));
    if (need > fb.work_cap) {
        if (fb.work) { HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); HIPCHK(ctx, hipFree(fb.work)); fb.work = nullptr; }
        HIPCHK(ctx, hipMalloc(&fb.work, need));
        ctx->device_bytes += (int64_t)need - (int64_t)fb.work_cap;
        fb.work_cap = need;
    }
    if (fb.work_cap) FFTCHK(ctx, rocfft_execution_info_set_work_buffer(fb.info, fb.work, fb.work_cap));
    fb.plans[batch] = pl;
    *out = &fb.plans[batch];
    return JX_OK;
}

// one chunk: per-walker kernel, Abel + map kernel into the padded image, the transforms, the tail
static int run_fft(jx_ctx* ctx, Chunk& c) {
    FftBack& fb = ctx->fft;
    const JxDev& d = c.d;
    const Taps& t = c.t;
    hipStream_t st = c.st;
    const int n = c.n;
    const bool tm = c.tm;
    EvSet& es = *c.es;
    int rc;
    launch_prep(ctx, c, st, nullptr, 0, d.nrow);
    if (tm) HIPCHK(ctx, hipEventRecord(es.e[1], st));
    if (n > fb.cap) { ctx->err = "rocFFT sequence: launch beyond its work buffers"; return JX_ERR_INVALID; }
    Plan3* pl = nullptr;
    if (!fb.rows_custom && (rc = fft_plans(ctx, fb, n, &pl))) return rc;          // (no rocFFT plan where rows and columns are hand-written)
    {
        JxDev dm = fb.d;
        dm.inject_pp = ctx->d.inject_pp;
        launch_map(st, dm, fb.map_threads, fb.map_lds, c.theta, c.w0, n, fb.img, t.pp, t.ab, t.y, false);
    }
    if (tm) HIPCHK(ctx, hipEventRecord(es.e[2], st));
    const double* zin = nullptr;
    if (fb.cols) {
        // rows by rocFFT, columns by jx_fft.hpp: forward, times the beam spectrum, inverse in one pass over the row spectra; then the
        // window's row spectra and its column pass, which leaves the spectrum of the extracted row
        const int S = d.S;
        if (fb.rows_custom) {
            fft_launch_rows_fwd(fb, n, st, S);
            fft_launch_beam(fb, n, st, S);
            if (tm) HIPCHK(ctx, hipEventRecord(es.e[3], st));       // (the inverse row pass of the convolution is inside the next kernel)
            fft_launch_rows_inv_tf(fb, n, st, S, t.need_conv);
        } else {
            void* a[1] = {fb.img};   void* b[1] = {fb.spec};
            FFTCHK(ctx, rocfft_execute(pl->row_fwd, a, b, fb.info));
            fft_launch_beam(fb, n, st, S);
            void* c2[1] = {fb.conv};
            FFTCHK(ctx, rocfft_execute(pl->row_inv, b, c2, fb.info));
            if (tm) HIPCHK(ctx, hipEventRecord(es.e[3], st));
            void* t2[1] = {fb.tfspec};
            FFTCHK(ctx, rocfft_execute(pl->row_tf, c2, t2, fb.info));
        }
        fft_launch_tf(fb, n, st, d.Sh);
        if (tm) HIPCHK(ctx, hipEventRecord(es.e[4], st));
        zin = fb.zbuf;
    } else {
        {
            void* in[1] = {fb.img};
            void* out[1] = {fb.spec};
            FFTCHK(ctx, rocfft_execute(pl->beam_fwd, in, out, fb.info));
            const size_t per = (size_t)fb.P * fb.Ph, total = per * n;
            const int blocks = (int)std::min<size_t>((total + 255) / 256, 8192);
            hipLaunchKernelGGL(jx_beam_mul_kernel, dim3(blocks), dim3(256), 0, st, fb.spec, (const double2*)fb.d.bhat, per, total);
            void* in2[1] = {fb.spec};
            void* out2[1] = {fb.conv};
            FFTCHK(ctx, rocfft_execute(pl->beam_inv, in2, out2, fb.info));
        }
        if (tm) HIPCHK(ctx, hipEventRecord(es.e[3], st));
        {
            void* in[1] = {fb.conv};
            void* out[1] = {fb.tfspec};
            FFTCHK(ctx, rocfft_execute(pl->tf_fwd, in, out, fb.info));
        }
        if (tm) HIPCHK(ctx, hipEventRecord(es.e[4], st));
    }
    const size_t sh = sizeof(double) * (JX_LDS_HDR + (size_t)2 * d.Sh + d.nrow + 8 + (size_t)2 * d.S);      // (+ the roots of unity of the row)
    hipLaunchKernelGGL(jx_tail_kernel, dim3(n), dim3(JX_TAIL_THREADS), sh, st, fb.d, fb.tfspec, zin, ctx->d_cfac, ctx->d_sz0,
                       ctx->d_base, c.logp, c.w0, t.row, t.bright, t.chisq, t.parts);
    return JX_OK;
}
