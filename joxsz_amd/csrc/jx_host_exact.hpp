// Host side of the exact form (kernels: jx_exact.hpp; default route): the row as one constant operator on the spline ordinates, planned on
// the host (plan_exact), uploaded with the work buffers of a chunk (exact_setup), and run per chunk as
//   jx_walker2_kernel -> jx_ordrow_kernel -> [taps] -> jx_rowsum_tail_kernel   (run_exact).
// jx_config.dtype 3 ('f32x'): the same plan with the three operators rounded once to fp32, a range guard on the profile derived from them, and
// jx_ordrow32_kernel in the place of jx_ordrow_kernel (same grid, LDS and JxRowOp; its tables, the guard and the priors come
// in JxRowOp32); the per-walker kernel, the taps and the tails are the f64 ones.
#pragma once
#include "jx_ctx.hpp"

struct ExactBuild {
    bool ok = false;
    int Nk = 0, Nkp = 0, nxt = 0, ng = 0, ng_use = 0, npair = 0, nSj = 0, nfold = 0;
    bool lean = true;
    std::vector<double> Wfk, Typ, Opk;                           // Wfk, Opk (and their fp32 roundings): tile-major, as the pair-wise kernels read them (jxt::row_tile_major)
    std::vector<double> OpkLane;                                 // JOXSZ_X_PAIRWISE=0 only: the row operator in exact_row_layout's own order, a lane's tiles contiguous (jx_rowop_tail_kernel)
    // fp32 products (jx_config.dtype 3): the same three tables rounded once to fp32, and the range guard T = 2^t_log2 on the profile
    bool f32x = false;
    std::vector<float> Wfk32, Typ32, Opk32;
    int t_log2 = 0;
};

// every pixel, every radius, nothing truncated: nothing here can fail once plan_shared has passed
static void plan_exact(jx_ctx* ctx, const PlanShared& sh, const std::vector<double>& beam, const std::vector<double>& r, ExactBuild& xb) {
    const jx_config& c = ctx->cfg;
    const int S = c.S, B = c.B, nrow = S - S / 2;
    std::vector<double> Wy;
    xb.Nk = jxt::exact_row_operator(beam, B, c.step * c.step, sh.A, S, sh.NU, ctx->h_Qtab, ctx->qn, r, ctx->h_G, ctx->K, Wy);
    if (!ctx->map_ok) xb.Nk = c.N;                          // (the profile taps are then read off the product's own array: every ordinate)
    xb.Nkp = (xb.Nk + 15) & ~15;
    const int tiles_use = (std::max(1, ctx->prune ? ctx->nrow_use : nrow) + 15) / 16, tiles = (nrow + 15) / 16;
    xb.nxt = std::min(6, tiles_use);
    xb.ng_use = (tiles_use + xb.nxt - 1) / xb.nxt;
    xb.ng = (tiles + xb.nxt - 1) / xb.nxt;
    jxt::exact_row_layout(Wy, nrow, c.N, xb.Nkp / 16, xb.nxt, xb.ng, xb.Opk);
    xb.npair = (xb.Nkp / 16 + 1) / 2;
    xb.nSj = (c.N + 15) / 16;
    jxt::abel_ordinate_layout(r, c.kpc_cm * c.sigma_T / c.m_e, xb.Nkp / 16, xb.nSj, xb.Typ);
    {   // an odd number of ordinate tiles: the last one folded into the row product (timed path), the others pair up exactly
        const int nS = xb.Nkp / 16;
        const char* e = opt_str(ctx, "JOXSZ_X_FOLD");
        xb.lean = !(e && atoi(e) == 0);
        if ((nS & 1) && nS >= 3 && xb.lean) {
            xb.nfold = xb.nSj - (nS - 1);
            jxt::exact_fold_layout(Wy, nrow, r, c.kpc_cm * c.sigma_T / c.m_e, nS, xb.nSj, xb.nxt, xb.ng, xb.Wfk);
        }
    }
    if (ctx->f32x) {
        // the tables as built above, in long double then double, rounded once more in the same operand orders; the guard from their absolute row sums
        xb.f32x = true;
        jxt::round_to_f32(xb.Typ, xb.Typ32);
        jxt::round_to_f32(xb.Opk, xb.Opk32);
        jxt::round_to_f32(xb.Wfk, xb.Wfk32);
        const int nS = xb.Nkp / 16;
        xb.t_log2 = jxt::f32_range_guard_log2(jxt::ordinate_layout_abs_rowsum(xb.Typ32, nS, xb.nSj), jxt::row_layout_abs_rowsum(xb.Opk32, nS, xb.nxt, xb.ng),
                                              xb.nfold ? jxt::row_layout_abs_rowsum(xb.Wfk32, xb.nfold, xb.nxt, xb.ng) : 0.0);
    }
    {   // the pair-wise kernels multiply one output tile at a time: their row and fold operators go tile-major, [g][s][NXT][64][4], one vector
        // load per lane, ordinate tile and output tile (a pure permutation, behind the rounding and the guard, which read exact_row_layout's order)
        const int nS = xb.Nkp / 16;
        if (!ctx->exact.pairwise) xb.OpkLane = xb.Opk;
        std::vector<double> td;
        std::vector<float> tf;
        jxt::row_tile_major(xb.Opk, nS, xb.nxt, xb.ng, td); xb.Opk.swap(td);
        if (xb.nfold) { jxt::row_tile_major(xb.Wfk, xb.nfold, xb.nxt, xb.ng, td); xb.Wfk.swap(td); }
        if (xb.f32x) {
            jxt::row_tile_major(xb.Opk32, nS, xb.nxt, xb.ng, tf); xb.Opk32.swap(tf);
            if (xb.nfold) { jxt::row_tile_major(xb.Wfk32, xb.nfold, xb.nxt, xb.ng, tf); xb.Wfk32.swap(tf); }
        }
    }
    xb.ok = true;
}

static void exact_teardown(jx_ctx* ctx, ExactBack& m) {
    for (void* p : m.allocs) (void)hipFree(p);
    m.allocs.clear();
    ctx->device_bytes -= m.bytes;
    m.bytes = 0;
    m.ready = false;
}

// two constant operators, the ordinates and partial rows of a chunk, and the part of the kernel argument that no launch changes
static int exact_setup(jx_ctx* ctx, const ExactBuild& xb, long long tW) {
    ExactBack& m = ctx->exact;
    const int64_t before = ctx->device_bytes;
    int rc;
    m.tW = tW;
    m.Nk = xb.Nk; m.Nkp = xb.Nkp; m.nxt = xb.nxt; m.ng = xb.ng; m.ng_use = xb.ng_use;
    m.npair = xb.npair; m.nSj = xb.nSj; m.ldpp = 16 * xb.nSj; m.nfold = xb.nfold; m.lean = xb.lean;
    m.cf = nullptr; m.ppi = nullptr;
    m.f32x = xb.f32x; m.t_log2 = xb.t_log2;
    if (m.f32x) {                                                // (only the fp32 copies are uploaded)
        if (m.t_log2 < 32) {
            ctx->err = "dtype 3 (f32x): the fp32 operators of this problem leave the pressure profile a range of 2^" + std::to_string(m.t_log2) + " before an fp32 partial sum could overflow (2^32 required); use dtype 0";
            return JX_ERR_UNSUPPORTED;
        }
        if (xb.nfold && (rc = dev_put_l(ctx, m.allocs, xb.Wfk32.data(), xb.Wfk32.size(), &m.Wfk32))) return rc;
        if ((rc = dev_put_l(ctx, m.allocs, xb.Typ32.data(), xb.Typ32.size(), &m.Typ32))) return rc;
        if ((rc = dev_put_l(ctx, m.allocs, xb.Opk32.data(), xb.Opk32.size(), &m.Opk32))) return rc;
    } else {
        if (xb.nfold && (rc = dev_put_l(ctx, m.allocs, xb.Wfk.data(), xb.Wfk.size(), &m.Wfk))) return rc;
        if ((rc = dev_put_l(ctx, m.allocs, xb.Typ.data(), xb.Typ.size(), &m.Typ))) return rc;
        // (the reference kernel's launches form no row product in jx_ordrow_kernel, ng = 0: the one table they read is the lane-major one)
        const std::vector<double>& opk = m.pairwise ? xb.Opk : xb.OpkLane;
        if ((rc = dev_put_l(ctx, m.allocs, opk.data(), opk.size(), &m.Opk))) return rc;
    }
    if ((rc = dev_new_l(ctx, m.allocs, (size_t)tW * m.Nkp, &m.y, true))) return rc;
    if ((rc = dev_new_l(ctx, m.allocs, (size_t)(tW / 16) * m.npair * m.ng * 256 * m.nxt, &m.P, true))) return rc;
    // contracted form of the pair-wise kernels: as many data-radii tiles as the epilogue is instantiated for, and fewer data radii than
    // outputs (or the partial rows are the smaller ones); the data-radii matrix in the order its product reads it
    const int nflux = ctx->d.nflux, nrow = ctx->nrow, nuse = std::min(ctx->prune ? ctx->nrow_use : nrow, nrow);
    m.ldm = nflux; m.ndt = (nflux + 15) / 16;
    m.ct_ok = m.ndt <= JX_CT_NDT && nflux < 16 * m.nxt * m.ng_use;
    m.Pm = nullptr; m.Eop = nullptr; m.last_ct = -1;
    if (m.ct_ok) {
        if ((rc = dev_new_l(ctx, m.allocs, (size_t)(tW / 16) * m.npair * 16 * m.ldm, &m.Pm, true))) return rc;
        std::vector<double> hE((size_t)nflux * nrow), eop;
        HIPCHK(ctx, hipMemcpy(hE.data(), ctx->d.emat, sizeof(double) * hE.size(), hipMemcpyDeviceToHost));
        jxt::contract_operand_layout(hE.data(), nflux, nrow, nuse, m.nxt, m.ng_use, eop, m.f32x ? 1 : 0);
        if ((rc = dev_put_l(ctx, m.allocs, eop.data(), eop.size(), &m.Eop))) return rc;
    }
    JxRowOp& ro = m.ro;
    memset(&ro, 0, sizeof(ro));
    ro.nS = m.Nkp / 16; ro.ldy = m.Nkp;
    ro.nuse = nuse;
    ro.ldr = (ro.nuse + 1) | 1;
    ro.lde = ro.nuse;
    ro.ldpp = m.ldpp; ro.nSj = m.nSj; ro.npair = m.npair;
    ro.Opk = m.Opk; ro.Typ = m.Typ; ro.P = m.P;
#ifdef JOXSZ_ABLATIONS
    ro.dbg = ctx->mix.dbg;                                       // (JOXSZ_MIX_DBG: one setting for both families of kernels)
#endif
#define JX_ROP_ATTR(Xv) HIPCHK(ctx, hipFuncSetAttribute((const void*)jx_rowop_tail_kernel<Xv>, hipFuncAttributeMaxDynamicSharedMemorySize, 158 * 1024)); \
    HIPCHK(ctx, hipFuncSetAttribute((const void*)jx_rowsum_tail_kernel<Xv>, hipFuncAttributeMaxDynamicSharedMemorySize, 158 * 1024));
    JX_MIX_NXTS(JX_ROP_ATTR)
#undef JX_ROP_ATTR
    m.bytes = ctx->device_bytes - before;
    if ((rc = dev_new(ctx, (size_t)ctx->chunk * m.ldpp, &ctx->d_ppc, true))) return rc;   // (the profiles in rows padded with zeros to whole 16-radius steps)
    m.ready = true;
    return JX_OK;
}

#ifdef JOXSZ_ABLATIONS
// diagnostic build only (JOXSZ_X_STAMPS; the option is read on the launch path here): wall-clock stamps of jx_ordrow_kernel's phases,
// printed once, at the 40th launch
static int ordrow_stamps(jx_ctx* ctx, hipStream_t st, int n, JxRowOp& ro) {
    static long long* stamps = nullptr;
    if (!stamps) { HIPCHK(ctx, hipMalloc((void**)&stamps, sizeof(long long) * JX_STAMP_LD * 65536)); }
    ro.stamps = stamps;
    static int calls = 0;
    if (++calls != 40) return JX_OK;
    HIPCHK(ctx, hipStreamSynchronize(st));
    const int nb = 8 * ((((n + 15) / 16) + 7) / 8) * ro.npair;
    std::vector<long long> h((size_t)nb * JX_STAMP_LD);
    HIPCHK(ctx, hipMemcpy(h.data(), stamps, sizeof(long long) * h.size(), hipMemcpyDeviceToHost));
    long long t0 = h[0];
    for (int b = 0; b < nb; ++b) t0 = std::min(t0, h[(size_t)b * JX_STAMP_LD]);
    double mx[5] = {0, 0, 0, 0, 0}, sm[5] = {0, 0, 0, 0, 0};
    for (int b = 0; b < nb; ++b)
        for (int k = 0; k < 5; ++k) { const double v = (h[(size_t)b * JX_STAMP_LD + k] - t0) * 0.01; mx[k] = std::max(mx[k], v); sm[k] += v / nb; }
    fprintf(stderr, "ordrow stamps (us after the first block's start; mean / max over %d blocks): start %.2f/%.2f  first loads %.2f/%.2f  k loop %.2f/%.2f  ordinates %.2f/%.2f  end %.2f/%.2f\n",
            nb, sm[0], mx[0], sm[1], mx[1], sm[2], mx[2], sm[3], mx[3], sm[4], mx[4]);
    {                                                            // where the late first operands are: by XCD, by eighth of the grid, and the ten latest blocks
        double bx[8] = {0}, bo[8] = {0}; int cx[8] = {0}, co[8] = {0}, late = 0;
        std::vector<std::pair<double, int>> fl;
        for (int b = 0; b < nb; ++b) {
            const double v = (h[(size_t)b * JX_STAMP_LD + 1] - h[(size_t)b * JX_STAMP_LD]) * 0.01;
            bx[b & 7] += v; ++cx[b & 7]; bo[b * 8 / nb] += v; ++co[b * 8 / nb]; if (v > 3.0) ++late;
            fl.push_back({v, b});
        }
        std::sort(fl.rbegin(), fl.rend());
        fprintf(stderr, "  first operands after the block's own start, mean by XCD:");
        for (int k = 0; k < 8; ++k) fprintf(stderr, " %.2f", bx[k] / std::max(1, cx[k]));
        fprintf(stderr, " | by eighth of the grid:");
        for (int k = 0; k < 8; ++k) fprintf(stderr, " %.2f", bo[k] / std::max(1, co[k]));
        fprintf(stderr, " | %d blocks beyond 3 us; latest:", late);
        for (int k = 0; k < 10 && k < (int)fl.size(); ++k) fprintf(stderr, " %d(%.1f, start %.1f)", fl[k].second, fl[k].first, (h[(size_t)fl[k].second * JX_STAMP_LD] - t0) * 0.01);
        fprintf(stderr, "\n");
    }
    for (int pp_ = 0; pp_ < ro.npair; ++pp_) {                  // per pair: mean first loads | k loop | end
        double a[3] = {0, 0, 0}, e_max = 0; int cnt = 0;
        for (int b = 0; b < nb; ++b) if ((b >> 3) % ro.npair == pp_) {
            a[0] += (h[(size_t)b * JX_STAMP_LD + 1] - t0) * 0.01; a[1] += (h[(size_t)b * JX_STAMP_LD + 2] - t0) * 0.01; a[2] += (h[(size_t)b * JX_STAMP_LD + 4] - t0) * 0.01;
            e_max = std::max(e_max, (h[(size_t)b * JX_STAMP_LD + 4] - t0) * 0.01); ++cnt;
        }
        fprintf(stderr, "  pair %2d: first loads %.2f  k loop %.2f  end %.2f (max %.2f)\n", pp_, a[0] / cnt, a[1] / cnt, a[2] / cnt, e_max);
    }
    {   // per wave: the end of the epilogue (in front of the block's last barrier) after the block's ordinates stamp
        double aw[4] = {0, 0, 0, 0}, mw[4] = {0, 0, 0, 0};
        for (int b = 0; b < nb; ++b)
            for (int w = 0; w < 4; ++w) {
                const double v = (h[(size_t)b * JX_STAMP_LD + 8 + w] - h[(size_t)b * JX_STAMP_LD + 3]) * 0.01;
                aw[w] += v / nb; mw[w] = std::max(mw[w], v);
            }
        fprintf(stderr, "  epilogue end after the block's ordinates, mean (max) by wave: %.2f (%.2f) %.2f (%.2f) %.2f (%.2f) %.2f (%.2f)\n",
                aw[0], mw[0], aw[1], mw[1], aw[2], mw[2], aw[3], mw[3]);
        // where the waves ran: hardware id bits 5:4 SIMD, 15:8 compute unit with shader array and engine, XCD number above bit 32
        std::map<long long, std::vector<int>> cu;                // compute unit -> its blocks
        std::map<long long, int> simd_tiles;                     // (compute unit, SIMD) -> output tiles owned by the roles that ran there
        int off[4] = {0, 0, 0, 0}, split = 0;
        for (int b = 0; b < nb; ++b) {
            const long long* hb = &h[(size_t)b * JX_STAMP_LD + 12];
            const long long key0 = (hb[0] >> 32 << 8) | ((hb[0] >> 8) & 255);
            cu[key0].push_back(b);
            ++off[(int)((hb[0] >> 4) & 3)];
            for (int w = 0; w < 4; ++w) {
                const long long key = (hb[w] >> 32 << 8) | ((hb[w] >> 8) & 255);
                if (key != key0 || (int)((hb[w] >> 4) & 3) != (int)(((hb[0] >> 4) & 3) + w) % 4) ++split;
                simd_tiles[key * 4 + ((hb[w] >> 4) & 3)] += (w + 4 < 6) ? 2 : 1;   // (six output tiles, wave w owns w and w + 4: the flagship instance)
            }
        }
        int hist[8] = {0}, tmax_sum = 0; std::map<long long, int> cumax;
        for (auto& kv : cu) ++hist[std::min<size_t>(7, kv.second.size())];
        for (auto& kv : simd_tiles) cumax[kv.first >> 2] = std::max(cumax[kv.first >> 2], kv.second);
        int worst = 0; for (auto& kv : cumax) { tmax_sum += kv.second; worst = std::max(worst, kv.second); }
        fprintf(stderr, "  placement: %d compute units; blocks per unit 1..7+: %d %d %d %d %d %d %d; SIMD of wave 0: %d %d %d %d; waves off (SIMD of wave 0 + w) or off the unit: %d\n",
                (int)cu.size(), hist[1], hist[2], hist[3], hist[4], hist[5], hist[6], hist[7], off[0], off[1], off[2], off[3], split);
        fprintf(stderr, "  output tiles on the busiest SIMD of a unit (six-tile instance): mean %.2f, worst %d\n", tmax_sum / std::max(1.0, (double)cumax.size()), worst);
        int shown = 0;
        for (auto& kv : cu) {
            if (shown++ >= 12) break;
            fprintf(stderr, "    unit %llx:", kv.first);
            for (int b : kv.second) fprintf(stderr, " id %d (jj %d, start %.2f, wave0 SIMD %d)", b, b >> 3, (h[(size_t)b * JX_STAMP_LD] - t0) * 0.01, (int)((h[(size_t)b * JX_STAMP_LD + 12] >> 4) & 3));
            fprintf(stderr, "\n");
        }
    }
    return JX_OK;
}
#endif

// One chunk: y = y_scale A pp on the matrix cores and each column-tile pair's share of out = Wy y (jx_ordrow_kernel), then the partial
// rows -- or, contracted, their shares of the model at the data radii -- added in pair order with the tail behind them
static int run_exact(jx_ctx* ctx, Chunk& c) {
    ExactBack& m = ctx->exact;
    const JxDev& d = c.d;
    const Taps& t = c.t;
    hipStream_t st = c.st;
    const int n = c.n, N = d.N;
    const bool tm = c.tm, tm2 = c.tm2;
    EvSet& es = *c.es;
    int rc;
    const bool all = t.row || t.bright;                      // the row and brightness taps get every output; the data-radii matrix reads the same ones either way
    const bool lean = m.lean && m.pairwise && !all && !t.profiles();     // the timed path: nothing reads the ordinates
    // contracted form: every call of the pair-wise kernels without row / brightness taps, whatever the fold and the ordinates do (a
    // walker's bits must not depend on them); where it does not fit, or is switched off, the partial rows as before
    const bool contract = m.contracted() && !all;

    // ---- per-walker kernel: conversion factors up to the outputs of the groups in use, the profile into the padded rows of the product
    c.xr_split = prep_splits(ctx, c);
    if (tm2 && es.p1stage == 3) HIPCHK(ctx, hipEventRecord(es.e[2], st));
    launch_prep(ctx, c, st, ctx->d.inject_pp ? (double*)nullptr : ctx->d_ppc, ctx->d.inject_pp ? 0 : m.ldpp, std::min(d.nrow, 16 * m.nxt * m.ng_use));
    if (tm2 && es.p1stage == 3) HIPCHK(ctx, hipEventRecord(es.e[3], st));
    if (tm) HIPCHK(ctx, hipEventRecord(es.e[1], st));
    if (!ctx->map_ok && t.need_img) { ctx->err = "radial grid too long for the Abel + map kernel: no Compton-y map tap on this problem (and JOXSZ_ABEL_GEMM=0 is not available)"; return JX_ERR_UNSUPPORTED; }

    // ---- ordinate product + row product
    const double* pp_src = ctx->d_ppc;
    if (ctx->d.inject_pp) {                                  // (operator build: the unit profiles into the padded rows of the product)
        if (!m.ppi && (rc = dev_new_l(ctx, m.allocs, (size_t)ctx->chunk * m.ldpp, &m.ppi, true))) return rc;
        HIPCHK(ctx, hipMemcpy2DAsync(m.ppi, sizeof(double) * m.ldpp, ctx->d.inject_pp, sizeof(double) * N, sizeof(double) * N, n, hipMemcpyDeviceToDevice, st));
        pp_src = m.ppi;
    }
    JxRowOp ro = m.ro;
    ro.n = n; ro.ng = all ? m.ng : m.ng_use;
    if (m.nfold && lean) {                                   // folded form: the last ordinate tile is not computed, one pair fewer
        ro.nfold = m.nfold; ro.s0f = ro.nS - 1; ro.Wfk = m.Wfk; ro.npair = (ro.nS - 1) / 2;
    }
#ifdef JOXSZ_ABLATIONS
    if (opt_str(ctx, "JOXSZ_X_STAMPS") && (rc = ordrow_stamps(ctx, st, n, ro))) return rc;
#endif
    ro.pp = pp_src; ro.y = lean ? (double*)nullptr : m.y;    // (lean: the ordinates stay in LDS)
    if (contract) {
        ro.nflux = d.nflux; ro.nrow = d.nrow; ro.ldm = m.ldm; ro.ndt = m.ndt;
        ro.cfac = ctx->d_cfac; ro.Eop = m.Eop; ro.Pm = m.Pm;
    }
    m.last_ct = contract ? 1 : 0;
    {
        JxRowOp r1 = ro;
        if (!m.pairwise) r1.ng = 0;                          // (the ordinates alone: the row product reads them back)
        const int ntw = (n + 15) / 16;
        const dim3 grid((unsigned)(8 * ((ntw + 7) / 8) * r1.npair));
        const size_t sh1 = sizeof(double) * (contract ? (size_t)JX_ORD_CT_LDS_DOUBLES(ro.ndt) : (size_t)JX_ORD_LDS_DOUBLES);
        if (tm2 && es.p1stage == 2) HIPCHK(ctx, hipEventRecord(es.e[2], st));
        bool done = false;
        JxRowOp32 r32{};
        if (m.f32x) r32 = JxRowOp32{m.Wfk32, m.Opk32, m.Typ32, std::ldexp(1.0, m.t_log2), ctx->d_base};
#define JX_ORD_GO(Xv) if (!done && m.nxt == Xv) { \
            if (m.f32x && contract) hipLaunchKernelGGL((jx_ordrow32_kernel<Xv, true>), grid, dim3(256), sh1, st, r1, r32); \
            else if (m.f32x) hipLaunchKernelGGL((jx_ordrow32_kernel<Xv>), grid, dim3(256), sh1, st, r1, r32); \
            else if (contract) hipLaunchKernelGGL((jx_ordrow_kernel<Xv, true>), grid, dim3(256), sh1, st, r1); \
            else hipLaunchKernelGGL((jx_ordrow_kernel<Xv>), grid, dim3(256), sh1, st, r1); \
            done = true; }
        JX_MIX_NXTS(JX_ORD_GO)
#undef JX_ORD_GO
        if (!done) { ctx->err = "no ordinate-product kernel for this output tiling"; return JX_ERR_UNSUPPORTED; }
        if (tm2 && es.p1stage == 2) HIPCHK(ctx, hipEventRecord(es.e[3], st));
    }

    // ---- taps
    if (t.profiles()) {
        if (ctx->map_ok) {
            // the profile taps come from the Abel kernel's own phases 1-3 (an independent evaluation of the same three lines)
            if (!m.cf && (rc = dev_new_l(ctx, m.allocs, (size_t)ctx->chunk * 2 * N, &m.cf, true))) return rc;
            JxDev dm = ctx->d;
            dm.cf_out = m.cf; dm.cf_ws = 2LL * N; dm.cf_tr = 0;
            launch_map(st, dm, ctx->map_threads, ctx->map_lds, c.theta, c.w0, n, nullptr, t.pp, t.ab, t.y, true);
        } else {
            if (t.pp) HIPCHK(ctx, hipMemcpy2DAsync(t.pp, sizeof(double) * N, pp_src, sizeof(double) * m.ldpp, sizeof(double) * N, n, hipMemcpyDeviceToDevice, st));
            if (t.y || t.ab) hipLaunchKernelGGL(jx_unpack_ordinates_kernel, dim3((unsigned)((N + 255) / 256), (unsigned)n), dim3(256), 0, st,
                                                m.y, m.Nkp, N, d.y_scale, t.y, t.ab);
        }
    }
    if (t.need_img && (rc = launch_y2d(ctx, c))) return rc;
    if (tm) HIPCHK(ctx, hipEventRecord(es.e[2], st));

    // ---- tail
    JxDev dtl = d;
    dtl.xr_split = c.xr_split ? 1 : 0;
    dtl.xr_out = ctx->d_xr;
    const dim3 gridt((unsigned)((n + 15) / 16));
    if (contract) {
        // the contracted partials added in pair order, chi^2, total, acceptance: 16 walkers x nflux values per block
        const unsigned tth = (unsigned)std::min(JX_RST_THREADS, 64 * ((16 * d.nflux + 63) / 64));
        if (tm2 && es.p1stage == 4) HIPCHK(ctx, hipEventRecord(es.e[2], st));
        hipLaunchKernelGGL((jx_rowsum_tail_kernel<0, true>), gridt, dim3(tth), sizeof(double) * 16 * (size_t)(d.nflux + 1), st,
                           dtl, ro, ctx->d_cfac, ctx->d_sz0, ctx->d_base, c.logp, c.w0, (double*)nullptr, (double*)nullptr, t.chisq, t.parts, c.sm);
    } else {
        const size_t lds_max = (size_t)158 * 1024;
        const size_t extra = m.pairwise ? 0 : sizeof(double) * (size_t)JX_ROP_NW * 16 * JX_ROP_LDP(m.nxt);
        if (extra + sizeof(double) * JX_RST_LDS_DOUBLES(ro.ldr, d.nflux, ro.lde) > lds_max) ro.lde = 0;   // (the data-radii matrix from memory then)
        const size_t shr = extra + sizeof(double) * JX_RST_LDS_DOUBLES(ro.ldr, d.nflux, ro.lde);
        if (shr > lds_max) { ctx->err = "exact form: the outputs the data-radii spline reads do not fit the tail's LDS (JOXSZ_MIX_FORM=legacy runs them)"; return JX_ERR_UNSUPPORTED; }
        if (tm2 && es.p1stage == 4) HIPCHK(ctx, hipEventRecord(es.e[2], st));
        bool done = false;
#define JX_ROP_GO(Xv) if (!done && m.nxt == Xv) { \
            if (m.pairwise) hipLaunchKernelGGL((jx_rowsum_tail_kernel<Xv>), gridt, dim3(JX_RST_THREADS), shr, st, dtl, ro, ctx->d_cfac, ctx->d_sz0, ctx->d_base, c.logp, c.w0, t.row, t.bright, t.chisq, t.parts, c.sm); \
            else hipLaunchKernelGGL((jx_rowop_tail_kernel<Xv>), gridt, dim3(64 * JX_ROP_NW), shr, st, dtl, ro, ctx->d_cfac, ctx->d_sz0, ctx->d_base, c.logp, c.w0, t.row, t.bright, t.chisq, t.parts, c.sm); \
            done = true; }
        JX_MIX_NXTS(JX_ROP_GO)
#undef JX_ROP_GO
        if (!done) { ctx->err = "no row-product kernel for this output tiling"; return JX_ERR_UNSUPPORTED; }
    }
    if (tm2 && es.p1stage == 4) HIPCHK(ctx, hipEventRecord(es.e[3], st));
    return JX_OK;
}
