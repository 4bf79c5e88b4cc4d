// Host side of the contracted forms of rounds 3-4 (kernels: jx_mix.hpp; JOXSZ_MIX_FORM=legacy|lowrank|full and every f32 context), frozen:
// planner (plan_mix), tables and work buffers (mix_setup, mix_context_tables), the launches of one chunk (launch_mix, run_mix), and the
// truncation guard (measure_truncation, mix_guard) that jx_finalize runs behind them.
#pragma once
#include "jx_ctx.hpp"

#define JX_MIX_NS 8
#define JX_MIX_RTS(X) X(2) X(4) X(6) X(8) X(10) X(12) X(14) X(16) X(18) X(20) X(22) X(24) X(26) X(28) X(30) X(32) X(36) X(40) X(44) X(48) X(56) X(64)
#define JX_MIX_KSPLIT_MAX 64
#define JX_MIX_CAP_REACH 4             // ranks up to rank_cap + this many terms are cut to rank_cap (then measured by the guard)
struct MixBuild {
    bool ok = false;
    std::string why;
    int form = 0, NU = 0, r = 0, ns = 0, R = 0, RT = 0, nxt = 0, ntile = 0, nog = 0, ksteps = 0;
    int r_tol = 0;                     // terms above the cut before the cap
    bool mfma = false;
    int nxt_u = 0, ntile_u = 0, nog_u = 0;     // tiling of the outputs in use (0: all of them)
    std::vector<double> Op_u;
    int NU_full = 0;                   // distinct rows of the quadrant; NU below = the rows stage 1 evaluates (sub)
    std::vector<int> sub;              // their indices (empty: all)
    size_t krows = 0;
    jxt::MixColumns cols;
    std::vector<double> Cm, Op;
    std::vector<JxSamp> ent;
    int cld = 0;
    double tol = 0.0, beam_tol = 0.0;
    double cost_lowrank = 0.0, cost_full = 0.0;
};

// form_force: -1 the cheaper form, 0 low-rank, 1 full.  tW: walker stride of the spline arrays (the full form's sample entries
// carry element offsets into them).
static void plan_mix(jx_ctx* ctx, const PlanShared& sh, const std::vector<double>& beam, const std::vector<double>& r,
                     double tol, int form_force, long long tW, MixBuild& mb) {
    const jx_config& c = ctx->cfg;
    const int S = c.S, B = c.B, Sh = S / 2 + 1, nrow = S - S / 2;
    const int NU = sh.NU;
    const std::vector<double>& A = sh.A;
    mb.NU = NU; mb.tol = tol; mb.beam_tol = 1e-14;          // (NU: replaced by the size of the sub-grid below when stage 1 evaluates one)
    mb.nxt = sh.nxt; mb.nog = sh.nog; mb.ntile = sh.ntile;
    mb.nxt_u = sh.nxt_u; mb.nog_u = sh.nog_u; mb.ntile_u = sh.ntile_u;
    // ---- low-rank form: separable terms of the beam x singular terms of the weights
    std::vector<double> U, V, by, bx;
    // Which rows (= columns) of the quadrant stage 1 evaluates: all of them, or -- when the quadrant lies inside the radial grid
    // (no fill values, no NaN radius: the map is then smooth away from the core) -- the sub-grid of jxt::mix_row_subset, the
    // others entering through the interpolation folded into both operators below.  mix_guard measures the result with the
    // truncation and takes the sub-grid away first when a bound is exceeded.
    mb.NU_full = NU;
    std::vector<double> Lint;                                    // [NU][ns]
    std::vector<double> Qsub;
    int NUs = NU;
    if (ctx->subsample) {
        bool inside = true;
        for (double v : ctx->h_Qtab) if (!(v <= r.back())) { inside = false; break; }
        jxt::mix_row_subset(NU, ctx->sub_u0, ctx->sub_u1, mb.sub);
        if (!inside || (int)mb.sub.size() > (3 * NU) / 4 || (int)mb.sub.size() < 2 * ctx->sub_npts) mb.sub.clear();
        else {
            NUs = (int)mb.sub.size();
            jxt::mix_interp_matrix(NU, mb.sub, ctx->sub_npts, Lint);
            Qsub.resize((size_t)NUs * NUs);
            for (int a = 0; a < NUs; ++a)
                for (int b2 = 0; b2 < NUs; ++b2) Qsub[(size_t)a * NUs + b2] = ctx->h_Qtab[(size_t)mb.sub[a] * ctx->qn + mb.sub[b2]];
        }
    }
    bool lowrank_ok = mb.sub.empty() ? jxt::mix_column_tables(ctx->h_Qtab, ctx->qn, NU, r, mb.cols, ctx->usplit)
                                     : jxt::mix_column_tables(Qsub, NUs, NUs, r, mb.cols, ctx->usplit);
    std::string why_lr = lowrank_ok ? "" : "pixel radii do not grow along the columns of d_mat";
    if (lowrank_ok && form_force != 1) {
        mb.r = jxt::lowrank_factor_qr(A.data(), S, Sh, tol, U, V);
        mb.ns = jxt::beam_separable_terms(beam, B, c.step * c.step, mb.beam_tol, by, bx);
        mb.r_tol = mb.r;
        // A rank a few terms above 16 is cut to 16 (terms are sorted by singular value: the first rows of U and V): the stage-1
        // kernel instance with 16 rows per column, stage 2 shorter by as much (and one 16-row tile of the matrix cores carries
        // stage 1 where that kernel is asked for).  mix_guard measures what the cut costs on the caller's data and rebuilds
        // without the cap when it is beyond the bounds.
        if (!ctx->tol_pinned && ctx->rank_cap > 0 && mb.ns > 0 && mb.r * mb.ns > ctx->rank_cap && ctx->rank_cap / mb.ns >= 1 &&
            mb.r <= ctx->rank_cap / mb.ns + JX_MIX_CAP_REACH) {
            mb.r = ctx->rank_cap / mb.ns;
            U.resize((size_t)mb.r * S); V.resize((size_t)mb.r * Sh);
        }
        mb.R = mb.r * mb.ns;
        mb.mfma = ctx->mix_mfma && mb.R <= 16;
        if (mb.r <= 0 || mb.ns <= 0) { lowrank_ok = false; why_lr = "transfer-function weights or beam image vanish"; }
        else if (mb.mfma) mb.RT = 16;
        else {
#define JX_PICK(Rv) if (!mb.RT && mb.R <= Rv) mb.RT = Rv;
            JX_MIX_RTS(JX_PICK)
#undef JX_PICK
            if (!mb.RT) { lowrank_ok = false; why_lr = "rank of the separable form beyond the stage-1 kernel (" + std::to_string(mb.r) + " x " + std::to_string(mb.ns) + " terms)"; }
        }
    }
    if (!ctx->usplit_forced && lowrank_ok && mb.RT) {
        // pieces per column: a chunk of 1024 walkers should fill the chip in as few rounds of waves as possible (24 resident waves per CU:
        // scripts/ubench/occ_rowmix.hip), each piece paying its ring fill once more -- rounds x (1 / pieces + 0.08), measured
        // against JOXSZ_MIX_USPLIT = 1..4 at 512^2 with and without the sub-grid (profiles/r04_subsample_scan.log); the hand-over of
        // the later pieces (RT sums per lane each) has to fit the 64 KB of dynamic LDS of one walker group
        const double cap = 24.0 * std::max(1, ctx->num_cu), ngrp = 16.0;      // (a nominal chunk of 1024 walkers, not this context's: the grouping of a walker's sums must not depend on max_batch)
        double best = 1e300;
        int pick = 1;
        for (int usp = 1; usp <= 4; ++usp) {
            if ((size_t)(usp - 1) * mb.RT * 64 * sizeof(double) > (size_t)64 * 1024) break;
            const double c = std::ceil(NUs * usp * ngrp / cap) * (1.0 / usp + 0.08);
            if (c < best * (1.0 - 1e-9)) { best = c; pick = usp; }
        }
        if (pick != ctx->usplit) {
            ctx->usplit = pick;
            lowrank_ok = mb.sub.empty() ? jxt::mix_column_tables(ctx->h_Qtab, ctx->qn, NU, r, mb.cols, ctx->usplit)
                                        : jxt::mix_column_tables(Qsub, NUs, NUs, r, mb.cols, ctx->usplit);
        }
    }
    // cost of each form in fused multiply-adds per walker; stage 1 runs on the vector units at about 0.6 of the rate the
    // matrix cores reach in the product kernels (measured: 256^2 with 32 terms 0.141 ms low-rank against 0.126 ms full; 257^2 0.155 against 0.132)
    const double nsamp_lr = (double)NUs * NUs;                                   // (samples evaluated: the sub-grid when there is one)
    // (stage 1 on the matrix cores: 16 multiply-adds per sample there, the 4 of the evaluation beside them on the vector units)
    const double nout = mb.ntile_u > 0 ? 16.0 * mb.ntile_u : (double)nrow;      // outputs the timed product computes
    const int nog_t = mb.ntile_u > 0 ? mb.nog_u : mb.nog;
    mb.cost_lowrank = (lowrank_ok && mb.RT) ? (mb.mfma ? nsamp_lr * 18.0 : 1.6 * nsamp_lr * (4.0 + mb.RT)) + nout * NUs * mb.R : 1e300;
    mb.cost_full = nout * nsamp_lr * 0.5 + nsamp_lr * 6.0 * nog_t;                // (the full form evaluates the same sub-grid)
    int form = (mb.cost_lowrank <= mb.cost_full) ? 0 : 1;
    if (form_force == 0) { if (!lowrank_ok || !mb.RT) { mb.why = "low-rank form: " + why_lr; return; } form = 0; }
    if (form_force == 1) form = 1;
    mb.form = form;
    if (form != 0) mb.mfma = false;
    if (form == 0) {
        mb.cld = mb.RT;
        if (mb.sub.empty()) {
            jxt::mix_stage1_operator(U, mb.r, by, mb.ns, S, B, NU, (mb.cols.wld + 4 + 1) & ~1, mb.cld, mb.Cm);   // (zero rows behind the last: the matrix-core kernel reads whole groups of four)
            const size_t K = (size_t)NU * mb.R;
            mb.ksteps = (int)((K + 3) / 4);
            mb.krows = 4 * ((size_t)mb.ksteps + (size_t)JX_MIX_KSPLIT_MAX * JX_OPG_RD + JX_OPG_RD);
            jxt::mix_stage2_operator(V, mb.r, bx, mb.ns, S, B, NU, mb.krows, mb.ntile, mb.Op);
        } else {
            // both operators on every row / column of the quadrant first, then through the interpolation: C_sub = L^T C,
            // Op_sub[(x'_s R + j)] = sum_x' L[x'][x'_s] Op[(x' R + j)]
            std::vector<double> Cf, Of;
            const int rows_f = (NU + 3) & ~3;
            jxt::mix_stage1_operator(U, mb.r, by, mb.ns, S, B, NU, rows_f, mb.cld, Cf);
            const int rows_s = (mb.cols.wld + 4 + 1) & ~1;
            mb.Cm.assign((size_t)rows_s * mb.cld, 0.0);
            for (int u = 0; u < NU; ++u)
                for (int a = 0; a < NUs; ++a) {
                    const double l = Lint[(size_t)u * NUs + a];
                    if (l == 0.0) continue;
                    for (int j = 0; j < mb.cld; ++j) mb.Cm[(size_t)a * mb.cld + j] += l * Cf[(size_t)u * mb.cld + j];
                }
            const size_t Kf = (size_t)NU * mb.R;
            const size_t krows_f = 4 * ((Kf + 3) / 4);
            jxt::mix_stage2_operator(V, mb.r, bx, mb.ns, S, B, NU, krows_f, mb.ntile, Of);
            const size_t K = (size_t)NUs * mb.R;
            mb.ksteps = (int)((K + 3) / 4);
            mb.krows = 4 * ((size_t)mb.ksteps + (size_t)JX_MIX_KSPLIT_MAX * JX_OPG_RD + JX_OPG_RD);
            const size_t rowlen = (size_t)16 * mb.ntile;
            mb.Op.assign(mb.krows * rowlen, 0.0);
            for (int x = 0; x < NU; ++x)
                for (int a = 0; a < NUs; ++a) {
                    const double l = Lint[(size_t)x * NUs + a];
                    if (l == 0.0) continue;
                    for (int j = 0; j < mb.R; ++j) {
                        const double* src = &Of[((size_t)x * mb.R + j) * rowlen];
                        double* dst = &mb.Op[((size_t)a * mb.R + j) * rowlen];
                        for (size_t e = 0; e < rowlen; ++e) dst[e] += l * src[e];
                    }
                }
        }
    } else {
        // ---- full form: every distinct sample (u <= x' when the quadrant is symmetric) is a row of the operator
        mb.r = 0; mb.ns = 0; mb.R = 0; mb.RT = 0;
        std::vector<double> Om;                                  // [nrow][NU][NU]
        jxt::mix_full_operator(beam, B, c.step * c.step, A, S, NU, Om);
        int NQ = NU;                                             // rows = columns of the samples evaluated
        if (!mb.sub.empty()) {
            // the sub-grid: Om_sub[x][a][b] = sum_{u, x'} L[u][a] L[x'][b] Om[x][u][x'] (L: at most sub_npts entries per row)
            std::vector<std::vector<std::pair<int, double>>> Ls(NU);
            for (int u = 0; u < NU; ++u)
                for (int a = 0; a < NUs; ++a) { const double l = Lint[(size_t)u * NUs + a]; if (l != 0.0) Ls[u].emplace_back(a, l); }
            std::vector<double> Os((size_t)nrow * NUs * NUs, 0.0), T((size_t)NU * NUs);
            for (int x = 0; x < nrow; ++x) {
                std::fill(T.begin(), T.end(), 0.0);
                const double* ox = &Om[(size_t)x * NU * NU];
                for (int u = 0; u < NU; ++u)
                    for (int xq = 0; xq < NU; ++xq) {
                        const double v = ox[(size_t)u * NU + xq];
                        if (v == 0.0) continue;
                        for (const auto& e : Ls[xq]) T[(size_t)u * NUs + e.first] += e.second * v;
                    }
                double* os = &Os[(size_t)x * NUs * NUs];
                for (int u = 0; u < NU; ++u)
                    for (const auto& e : Ls[u]) {
                        const double* tu = &T[(size_t)u * NUs];
                        double* oa = &os[(size_t)e.first * NUs];
                        for (int b2 = 0; b2 < NUs; ++b2) oa[b2] += e.second * tu[b2];
                    }
            }
            Om.swap(Os);
            NQ = NUs;
        }
        const std::vector<double>& Qt = mb.sub.empty() ? ctx->h_Qtab : Qsub;
        const int qld = mb.sub.empty() ? ctx->qn : NUs;
        const bool tri = jxt::quadrant_is_symmetric(Qt, qld, NQ);
        std::vector<int> ku, kx;
        for (int u = 0; u < NQ; ++u)
            for (int x = tri ? u : 0; x < NQ; ++x) { ku.push_back(u); kx.push_back(x); }
        const size_t K = ku.size();
        mb.ksteps = (int)((K + 3) / 4);
        mb.krows = 4 * ((size_t)mb.ksteps + (size_t)JX_MIX_KSPLIT_MAX * JX_OPG_RD + JX_OPG_RD + JX_OPG_ECH);
        mb.Op.assign(mb.krows * 16 * (size_t)mb.ntile, 0.0);
        JxSamp zero{};
        mb.ent.assign(mb.krows, zero);
        for (size_t k = 0; k < K; ++k) {
            const int u = ku[k], xq = kx[k];
            int k16; double w[4];
            jxt::spline_sample_weights(r, Qt[(size_t)u * qld + xq], &k16, w);
            JxSamp& e = mb.ent[k];
            e.off = (long long)(k16 / 16) * tW;
            e.a = w[0]; e.b = w[1]; e.c = w[2]; e.d = w[3];
            for (int x = 0; x < nrow; ++x) {
                double v = Om[((size_t)x * NQ + u) * NQ + xq];
                if (tri && xq != u) v += Om[((size_t)x * NQ + xq) * NQ + u];
                mb.Op[(k * 16 + (x & 15)) * mb.ntile + (x >> 4)] = v;
            }
        }
    }
    if (form == 0 && !mb.sub.empty()) mb.NU = NUs;               // (stage 1 walks the sub-grid's columns; the full form keeps NU and lists its samples)
    if (mb.ntile_u > 0 && mb.ntile_u < mb.ntile) {
        // the same operator for the outputs in use alone: tiles [0, ntile_u) of every row, compact
        const size_t rows = mb.Op.size() / ((size_t)16 * mb.ntile);
        mb.Op_u.assign(rows * 16 * (size_t)mb.ntile_u, 0.0);
        for (size_t kx = 0; kx < rows * 16; ++kx)
            for (int t = 0; t < mb.ntile_u; ++t) mb.Op_u[kx * mb.ntile_u + t] = mb.Op[kx * mb.ntile + t];
    } else { mb.ntile_u = 0; mb.nxt_u = 0; mb.nog_u = 0; }
    mb.ok = true;
}

static void mix_teardown(jx_ctx* ctx, MixBack& m) {
    for (void* p : m.allocs) (void)hipFree(p);
    m.allocs.clear();
    ctx->device_bytes -= m.bytes;
    m.bytes = 0;
    m.ready = false;
}

// K slices of the matrix-core product: a function of the problem alone (about 64 k-steps each, whole multiples of 8 slices so
// that a full chunk fills whole rounds of blocks), never of the launch -- a walker's sums are grouped the same way wherever it
// sits in whatever batch, so its result is bitwise independent of both
static void mix_kslices(const MixBack& m, bool used, int* ksplit_out, int* kper_out) {
    int ksplit = m.ksplit_force > 0 ? m.ksplit_force : (m.ksteps + 32) / 64;
    if (ksplit >= 8 && m.ksplit_force <= 0) ksplit = (ksplit + 4) / 8 * 8;
    // few output groups per walker block (the outputs in use alone; small sides): more K slices, of about 16 k-steps each, so
    // that the launch still fills the chip (measured: profiles/r04_subsample_scan.log)
    if (used && m.ksplit_u_force > 0) ksplit = m.ksplit_u_force;
    else if (used || m.ksplit_force <= 0) ksplit = std::max(ksplit, std::min((m.ksteps + 15) / 16, std::max(1, 32 / std::max(1, used ? m.og_u.nog : m.og.nog))));
    ksplit = std::max(1, std::min(ksplit, JX_MIX_KSPLIT_MAX));
    int kper = (m.ksteps + ksplit - 1) / ksplit;
    kper = (kper + JX_OPG_RD - 1) / JX_OPG_RD * JX_OPG_RD;
    ksplit = (m.ksteps + kper - 1) / kper;
    *ksplit_out = ksplit; *kper_out = kper;
}

static int mix_setup(jx_ctx* ctx, const MixBuild& mb, long long tW) {
    MixBack& m = ctx->mix;
    const int N = ctx->cfg.N;
    const int64_t before = ctx->device_bytes;
    int rc;
    m.form = mb.form; m.RT = mb.RT; m.nxt = mb.nxt; m.r = mb.r; m.ns = mb.ns; m.ksteps = mb.ksteps; m.tW = tW; m.tol = mb.tol;
    m.mfma = mb.mfma; m.r_tol = mb.r_tol;
    m.NU_full = mb.NU_full; m.sub = mb.sub;
    int* qi; double* qd;
    const size_t esz = ctx->f32 ? sizeof(float) : sizeof(double);
    const size_t cft_rows = (size_t)N + 2 * JX_MIX_NS + 2;
    if (2 * esz * cft_rows * tW >= ((size_t)1 << 32)) { ctx->err = "contracted route: launch too large for 32-bit knot offsets (lower max_batch)"; return JX_ERR_UNSUPPORTED; }
    JxMix& mx = m.mx;
    memset(&mx, 0, sizeof(mx));
    mx.dbg = m.dbg;
    if (mb.form == 0) {
        mx.NU = mb.NU; mx.R = mb.R; mx.tW = tW; mx.segld = mb.cols.segld; mx.wld = mb.cols.wld; mx.cld = mb.cld;
        mx.cft_bytes = (unsigned)(2 * esz * cft_rows * tW);
        mx.usplit = mb.cols.usplit;
        if ((rc = dev_put_l(ctx, m.allocs, mb.cols.urange.data(), mb.cols.urange.size(), &qi))) return rc; mx.urange = qi;
        if ((rc = dev_put_l(ctx, m.allocs, mb.cols.seg0.data(), mb.cols.seg0.size(), &qi))) return rc; mx.seg0 = qi;
        if ((rc = dev_put_l(ctx, m.allocs, mb.cols.nseg.data(), mb.cols.nseg.size(), &qi))) return rc; mx.nseg = qi;
        if ((rc = dev_put_l(ctx, m.allocs, mb.cols.seg.data(), mb.cols.seg.size(), &qi))) return rc; mx.seg = qi;
        if ((rc = dev_put_l(ctx, m.allocs, mb.cols.w4.data(), mb.cols.w4.size(), &qd))) return rc; mx.w4 = qd;
        if ((rc = dev_put_l(ctx, m.allocs, mb.Cm.data(), mb.Cm.size(), &qd))) return rc; mx.Cm = qd;
    }
    if (ctx->f32c && mb.form == 0) {                              // fp32 arithmetic: the stage-1 tables once more, rounded to fp32
        std::vector<float> wf(mb.cols.w4.begin(), mb.cols.w4.end()), cf(mb.Cm.begin(), mb.Cm.end());
        float* qf;
        if ((rc = dev_put_l(ctx, m.allocs, wf.data(), wf.size(), &qf))) return rc; mx.w4f = qf;
        if ((rc = dev_put_l(ctx, m.allocs, cf.data(), cf.size(), &qf))) return rc; mx.Cmf = qf;
    }
    JxOpg& og = m.og;
    memset(&og, 0, sizeof(og));
    og.tW = tW; og.ntile = mb.ntile; og.nog = mb.nog; og.ldx = 16 * mb.ntile;
    if ((rc = dev_put_l(ctx, m.allocs, mb.Op.data(), mb.Op.size(), &qd))) return rc; og.Op = qd;
    if (ctx->f32c && mb.form == 0) {
        std::vector<float> of(mb.Op.begin(), mb.Op.end());
        float* qf;
        if ((rc = dev_put_l(ctx, m.allocs, of.data(), of.size(), &qf))) return rc; og.Opf = qf;
    }
    m.has_u = mb.ntile_u > 0;
    m.og_u = og;
    if (m.has_u) {
        JxOpg& ou = m.og_u;
        m.nxt_u = mb.nxt_u;
        ou.ntile = mb.ntile_u; ou.nog = mb.nog_u; ou.ldx = 16 * mb.ntile_u;
        if ((rc = dev_put_l(ctx, m.allocs, mb.Op_u.data(), mb.Op_u.size(), &qd))) return rc; ou.Op = qd;
        if (ctx->f32c && mb.form == 0) {
            std::vector<float> of(mb.Op_u.begin(), mb.Op_u.end());
            float* qf;
            if ((rc = dev_put_l(ctx, m.allocs, of.data(), of.size(), &qf))) return rc; ou.Opf = qf;
        }
    }
    m.ncol = 2 * N;
    if ((rc = dev_new_l(ctx, m.allocs, 2 * esz * cft_rows * tW / sizeof(double) + 1, &m.cft, true))) return rc;
    if (mb.form == 0) {
        if ((rc = dev_new_l(ctx, m.allocs, mb.krows * (size_t)tW, &m.Dt, true))) return rc;    // (fp32 arithmetic: the same buffer holds floats)
        og.Dt = m.Dt; og.Dtf = reinterpret_cast<const float*>(m.Dt);
        m.og_u.Dt = og.Dt; m.og_u.Dtf = og.Dtf;
    } else {
        JxSamp* qe;
        if ((rc = dev_put_l(ctx, m.allocs, mb.ent.data(), mb.ent.size(), &qe))) return rc; og.ent = qe; m.og_u.ent = qe;
    }
    og.pstride = (long long)tW * og.ldx + 272;                // (not a power of two: the tail reads all slices of a walker at once)
    m.og_u.pstride = (long long)tW * m.og_u.ldx + 272;
    if ((rc = dev_new_l(ctx, m.allocs, (size_t)JX_MIX_KSPLIT_MAX * og.pstride, &m.Pt))) return rc;
    { int kp; mix_kslices(m, false, &m.last_ksplit, &kp); if (m.has_u) mix_kslices(m, true, &m.ksplit_u, &kp); }   // (reported before the first launch too)
    m.bytes = ctx->device_bytes - before;
    m.ready = true;
    return JX_OK;
}

// What the context holds for the contracted forms alone, behind mix_setup: the side stream, the operator Tm of the spline-array product
// (jx_abel_gemm_kernel) with its input, the radial sub-grid of that product, and the LDS limits of the kernels these forms launch
static int mix_context_tables(jx_ctx* ctx, const std::vector<double>& r, int chunk) {
    const int N = ctx->cfg.N;
    int rc;
    if (ctx->side_on) {
        HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->side_stream, hipStreamNonBlocking));
        HIPCHK(ctx, hipEventCreateWithFlags(&ctx->ev_side, hipEventDisableTiming));
        HIPCHK(ctx, hipEventCreateWithFlags(&ctx->ev_tail, hipEventDisableTiming));
    }
    std::vector<double> h_Tm;
    ctx->tm_ntile = (2 * N + 15) / 16;
    ctx->tm_npair = (ctx->tm_ntile + 1) / 2;
    ctx->tm_ld = 32 * ctx->tm_npair;
    jxt::abel_spline_operator(r, ctx->h_G, ctx->K, ctx->d.y_scale, JX_AG_ROWS(N), ctx->tm_ld, h_Tm);
    if ((rc = dev_put(ctx, h_Tm.data(), h_Tm.size(), &ctx->d_Tm))) return rc;
    if ((rc = dev_new(ctx, (size_t)chunk * (size_t)N, &ctx->d_ppc, true))) return rc;
    // The pressure profile is smooth away from the core: its values on a sub-grid of the radial grid carry the others by high-order
    // interpolation, pp ~ L pp_sub, and the product needs only L^T Tm -- K shrinks from N to the kept radii (222 of 500, 285 of 1000)
    // and with it the k loop that bounds the kernel.  Measured by mix_guard like the sub-grid of map samples.
    if (ctx->ag_sub && ctx->map_ok) {
        std::vector<int> rs;
        jxt::mix_row_subset(N, ctx->ag_u0, ctx->ag_u1, rs);
        const int ns = (int)rs.size();
        if (ns <= (3 * N) / 4 && ns >= 2 * ctx->ag_npts && ctx->ag_u0 >= ctx->ag_npts) {
            std::vector<double> L;
            jxt::mix_interp_matrix(N, rs, ctx->ag_npts, L);
            const int ld = ctx->tm_ld, rows = JX_AG_ROWS(ns);
            std::vector<double> Ts((size_t)rows * ld, 0.0);
            for (int j = 0; j < N; ++j)
                for (int a = 0; a < ns; ++a) {
                    const double l = L[(size_t)j * ns + a];
                    if (l == 0.0) continue;
                    const double* src = &h_Tm[(size_t)j * ld];
                    double* dst = &Ts[(size_t)a * ld];
                    for (int e = 0; e < ld; ++e) dst[e] += l * src[e];
                }
            // first k-step (four rows) of every column tile with an entry; made non-decreasing in the tile (the kernel's blocks start at their lowest tile's)
            std::vector<int> tks(ctx->tm_ntile, 0);
            for (int t = 0; t < ctx->tm_ntile; ++t) {
                int first = ns;
                for (int a = 0; a < ns && first == ns; ++a)
                    for (int e = 16 * t; e < std::min(16 * t + 16, ld); ++e) if (Ts[(size_t)a * ld + e] != 0.0) { first = a; break; }
                tks[t] = std::min(first, ns - 1) / 4;
            }
            for (int t = ctx->tm_ntile - 2; t >= 0; --t) tks[t] = std::min(tks[t], tks[t + 1]);
            if ((rc = dev_put(ctx, Ts.data(), Ts.size(), &ctx->d_Tm_s))) return rc;
            if ((rc = dev_put(ctx, rs.data(), rs.size(), &ctx->d_rsub))) return rc;
            if ((rc = dev_put(ctx, tks.data(), tks.size(), &ctx->d_tks))) return rc;
            ctx->h_rsub = rs; ctx->ag_ns = ns; ctx->ag_sub_on = true;
        }
    }
    HIPCHK(ctx, hipFuncSetAttribute((const void*)jx_rowmix_mfma_kernel<JX_MIX_NS, double2>, hipFuncAttributeMaxDynamicSharedMemorySize, 158 * 1024));
    HIPCHK(ctx, hipFuncSetAttribute((const void*)jx_rowmix_mfma_kernel<JX_MIX_NS, float2>, hipFuncAttributeMaxDynamicSharedMemorySize, 158 * 1024));
#define JX_OPG_ATTR(Xv) HIPCHK(ctx, hipFuncSetAttribute((const void*)jx_opgemm_kernel<1, Xv, double2>, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024)); \
    HIPCHK(ctx, hipFuncSetAttribute((const void*)jx_opgemm_kernel<1, Xv, float2>, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
    JX_MIX_NXTS(JX_OPG_ATTR)
#undef JX_OPG_ATTR
    return JX_OK;
}

// stage 1 + stage 2 (low-rank form) or the one product of the full form; es: the launch's event set or null
template <typename F>
static int launch_mix(jx_ctx* ctx, int n, EvSet* es, bool used /* the product for the outputs the tail reads alone */, F&& between /* called between stage 1 and the matrix-core product */) {
    MixBack& m = ctx->mix;
    hipStream_t st = ctx->stream;
    if (m.form == 0) {
        JxMix mx = m.mx;
        mx.n = n;
        // block = gpb walker groups x usplit pieces of one column (usplit: a setting of the context, never of the launch)
        const int usp = mx.usplit, ngrp = (n + 63) / 64;
        int wcap = m.wpb;
        size_t lds_c = 0;
        const int crows = (mx.wld + 4 + 1) & ~1;
        if (m.mfma) {
            // the matrix-core kernel keeps the operator in LDS: blocks of 8 waves, two per CU -- or of 16, one per CU, when the
            // operator is too large for two copies (sides beyond ~600)
            lds_c = sizeof(double) * 16 * (size_t)crows;
            wcap = (2 * (lds_c + sizeof(double) * JX_MXM_REGION(usp) * (8 / usp)) <= 158 * 1024) ? 8 : 16;
            if (m.wpb_force > 0) wcap = m.wpb_force;
        }
        if (!m.mfma && usp > 1) {                                   // walker groups per block: their hand-over (RT sums per lane and later piece) within 64 KB
            const int fit = (int)((size_t)64 * 1024 / (sizeof(double) * (usp - 1) * m.RT * 64));
            wcap = std::min(wcap, std::max(fit, 0) * usp);
            if (wcap < usp) { ctx->err = "stage 1: JOXSZ_MIX_USPLIT = " + std::to_string(usp) + " pieces of " + std::to_string(m.RT) + " rows per column do not fit the LDS hand-over (lower it)"; return JX_ERR_UNSUPPORTED; }
        }
        const int gpb = std::max(1, std::min(wcap / usp, ngrp)), wpb = gpb * usp;
        const int nq = (ngrp + gpb - 1) / gpb;
        mx.cper = (nq <= 8 && 8 % nq == 0) ? 8 / nq : 0;
        const dim3 g1((unsigned)(mx.cper ? 8 * ((mx.NU + mx.cper - 1) / mx.cper) : nq * mx.NU));
        const size_t lds1 = m.mfma ? lds_c + sizeof(double) * JX_MXM_REGION(usp) * gpb : sizeof(double) * (size_t)gpb * (usp - 1) * m.RT * 64;
        // (the vector-unit kernel keeps the default 64 KB limit of dynamic LDS: plan_mix clamps usplit so that a block's hand-over fits)
        if (lds1 > (m.mfma ? (size_t)158 * 1024 : (size_t)64 * 1024)) { ctx->err = "stage 1: the hand-over of the column pieces does not fit the LDS (lower JOXSZ_MIX_USPLIT or JOXSZ_MIX_WPB)"; return JX_ERR_UNSUPPORTED; }
        bool done = false;
        if (ctx->f32c) {
            const size_t ldsf = sizeof(float) * (size_t)gpb * (usp - 1) * m.RT * 64;
#define JX_MIXF_GO(Rv) if (!done && m.RT == Rv) { \
            hipLaunchKernelGGL((jx_rowmix_f32_kernel<Rv, JX_MIX_NS>), g1, dim3(64 * wpb), ldsf, st, mx, reinterpret_cast<const float2*>(m.cft), reinterpret_cast<float*>(m.Dt)); \
            done = true; }
            JX_MIX_RTS(JX_MIXF_GO)
#undef JX_MIXF_GO
        }
        if (!done && m.mfma) {
            if (ctx->f32) hipLaunchKernelGGL((jx_rowmix_mfma_kernel<JX_MIX_NS, float2>), g1, dim3(64 * wpb), lds1, st, mx, crows, reinterpret_cast<const float2*>(m.cft), m.Dt);
            else hipLaunchKernelGGL((jx_rowmix_mfma_kernel<JX_MIX_NS, double2>), g1, dim3(64 * wpb), lds1, st, mx, crows, reinterpret_cast<const double2*>(m.cft), m.Dt);
            done = true;
        }
#define JX_MIX_GO(Rv) if (!done && m.RT == Rv) { \
            if (ctx->f32) hipLaunchKernelGGL((jx_rowmix_kernel<Rv, JX_MIX_NS, float2>), g1, dim3(64 * wpb), lds1, st, mx, reinterpret_cast<const float2*>(m.cft), m.Dt); \
            else hipLaunchKernelGGL((jx_rowmix_kernel<Rv, JX_MIX_NS, double2>), g1, dim3(64 * wpb), lds1, st, mx, reinterpret_cast<const double2*>(m.cft), m.Dt); \
            done = true; }
        JX_MIX_RTS(JX_MIX_GO)
#undef JX_MIX_GO
        if (!done) { ctx->err = "no stage-1 kernel for this rank"; return JX_ERR_UNSUPPORTED; }
    }
    if (es) HIPCHK(ctx, hipEventRecord(es->e[3], st));
    { const int rcb = between(); if (rcb) return rcb; }
    {
        used = used && m.has_u;
        JxOpg og = used ? m.og_u : m.og;
        const int nxt = used ? m.nxt_u : m.nxt;
        og.n = n;
        const int nwb = (n + 127) / 128;
        int ksplit, kper;
        mix_kslices(m, used, &ksplit, &kper);
        og.ksplit = ksplit; og.kper = kper;
        if (used) m.ksplit_u = ksplit; else m.last_ksplit = ksplit;   // (the tail sums this many partials)
        m.last_was_u = used;
        const int nunit = ksplit * og.nog;
        og.kmajor = ksplit >= 8 ? 1 : 0;
        const dim3 g2((unsigned)(og.kmajor ? 8 * nwb * og.nog * ((ksplit + 7) / 8) : 8 * nwb * ((nunit + 7) / 8)));
        const size_t lds = m.form == 1 ? (size_t)JX_OPG_ECH * 4 * sizeof(JxSamp) : 0;
        bool done = false;
#define JX_OPGF_GO(Xv) if (!done && ctx->f32c && nxt == Xv) { \
            hipLaunchKernelGGL((jx_opgemm_f32_kernel<Xv>), g2, dim3(256), 0, st, og, reinterpret_cast<float*>(m.Pt)); done = true; }
        JX_MIX_NXTS(JX_OPGF_GO)
#undef JX_OPGF_GO
#define JX_OPG_GO(Xv) if (!done && nxt == Xv) { \
            if (m.form == 1 && ctx->f32) hipLaunchKernelGGL((jx_opgemm_kernel<1, Xv, float2>), g2, dim3(256), lds, st, og, reinterpret_cast<const float2*>(m.cft), m.Pt); \
            else if (m.form == 1) hipLaunchKernelGGL((jx_opgemm_kernel<1, Xv, double2>), g2, dim3(256), lds, st, og, reinterpret_cast<const double2*>(m.cft), m.Pt); \
            else hipLaunchKernelGGL((jx_opgemm_kernel<0, Xv, double2>), g2, dim3(256), lds, st, og, reinterpret_cast<const double2*>(m.cft), m.Pt); \
            done = true; }
        JX_MIX_NXTS(JX_OPG_GO)
#undef JX_OPG_GO
        if (!done) { ctx->err = "no stage-2 kernel for this output tiling"; return JX_ERR_UNSUPPORTED; }
    }
    if (es && !es->p1only) HIPCHK(ctx, hipEventRecord(es->e[4], st));
    return JX_OK;
}

// One chunk: per-walker kernel (in line, or beside the SZ chain on the side stream), spline arrays, stage 1 + stage 2, tail.
// Only the pressure profile is in the way of the SZ chain (spline arrays -> stage 1 -> stage 2); priors, vetoes, X-ray side and
// conversion factors feed the tail alone.  With JOXSZ_SIDE_STREAM a small kernel evaluates the profile in line, and the per-walker
// kernel runs on a second stream BESIDE THE MATRIX-CORE PRODUCT: forked by an event behind stage 1 (stage 1 fills every wave slot of
// the chip, the product leaves more than half of the registers free), joined by one in front of the tail.  Everything the fork event
// follows on the compute stream -- the previous tail, which reads the buffers this kernel writes, and whatever produced theta -- is
// therefore complete when it starts.  Calls with taps stay in line.
static int run_mix(jx_ctx* ctx, Chunk& c) {
    MixBack& m = ctx->mix;
    const JxDev& d = c.d;
    const Taps& t = c.t;
    hipStream_t st = c.st;
    const int n = c.n;
    const bool tm = c.tm, tm2 = c.tm2;
    EvSet& es = *c.es;
    int rc;
    // the spline arrays come from one matrix product, unless the profile taps are asked for (they live in the Abel kernel, which then
    // writes the arrays itself) or the matrix product is switched off
    // (a grid too long for the Abel kernel: always the matrix product; the profile taps are then read off its own arrays)
    const bool want_abel_taps = t.profiles();
    const bool ag = ctx->abel_gemm && (ctx->f32 || !ctx->map_ok || (!want_abel_taps && !ctx->d.inject_pp));
    const bool side = ag && ctx->side_stream && !ctx->d.inject_pp && !t.any();
    c.xr_split = !side && prep_splits(ctx, c);
    double* pp_buf = (ag && !ctx->d.inject_pp) ? ctx->d_ppc : (double*)nullptr;
    auto fork_prep = [&]() -> int {                                 // the per-walker kernel on the side stream, behind what the compute stream holds so far
        HIPCHK(ctx, hipEventRecord(ctx->ev_tail, st));
        HIPCHK(ctx, hipStreamWaitEvent(ctx->side_stream, ctx->ev_tail, 0));
        launch_prep(ctx, c, ctx->side_stream, nullptr, 0, d.nrow);
        HIPCHK(ctx, hipEventRecord(ctx->ev_side, ctx->side_stream));
        return JX_OK;
    };
    if (side) {
        JxDev dp = d;
        const size_t shp = sizeof(double) * (JX_LDS_HDR + 8);
        if (d.prep_pow) hipLaunchKernelGGL(jx_pp_kernel<true>, dim3(n), dim3(128), shp, st, dp, c.theta, c.w0, pp_buf);
        else hipLaunchKernelGGL(jx_pp_kernel<false>, dim3(n), dim3(128), shp, st, dp, c.theta, c.w0, pp_buf);
        if (ctx->side_fork == 0 && (rc = fork_prep())) return rc;   // fork behind the profile kernel: beside the spline-array product
    } else {
        if (tm2 && es.p1stage == 3) HIPCHK(ctx, hipEventRecord(es.e[2], st));
        launch_prep(ctx, c, st, pp_buf, 0, d.nrow);
        if (tm2 && es.p1stage == 3) HIPCHK(ctx, hipEventRecord(es.e[3], st));
    }
    if (tm) HIPCHK(ctx, hipEventRecord(es.e[1], st));
    if (ctx->f32 && (want_abel_taps || t.need_img)) { ctx->err = "dtype f32: the profile and map taps exist in the f64 build of the context only"; return JX_ERR_UNSUPPORTED; }
    if (ctx->f32 && !ag) { ctx->err = "dtype f32 takes its spline arrays from the matrix product only (JOXSZ_ABEL_GEMM=0 is an f64 setting)"; return JX_ERR_UNSUPPORTED; }
    if (!ctx->map_ok && (!ag || t.need_img)) { ctx->err = "radial grid too long for the Abel + map kernel: no Compton-y map tap on this problem (and JOXSZ_ABEL_GEMM=0 is not available)"; return JX_ERR_UNSUPPORTED; }
    if (ag) {
        // 32 walkers per block, or 16 when that would leave SIMDs without a wave (a walker's sums do not depend on it)
        const int gy = (ctx->tm_npair + 3) / 4;
        const bool narrow = ctx->ag_narrow >= 0 ? ctx->ag_narrow != 0 : (size_t)((n + 31) / 32) * gy * 4 < 1024;
        const dim3 grid(narrow ? (n + 15) / 16 : (n + 31) / 32, gy);
        const double* pp_src = ctx->d.inject_pp ? ctx->d.inject_pp : ctx->d_ppc;
        const size_t shg = sizeof(double) * JX_OPM_JC * 33;
        const bool rsg = ctx->ag_sub_on;                        // the radial sub-grid: K = the kept radii, gathered from the profiles
        const int agN = rsg ? ctx->ag_ns : d.N;
        const double* agT = rsg ? ctx->d_Tm_s : ctx->d_Tm;
        const int* agR = rsg ? ctx->d_rsub : nullptr;
        const int* agK = rsg ? ctx->d_tks : nullptr;
#define JX_AG_GO(TOv, NWTv) do { if (rsg) hipLaunchKernelGGL((jx_abel_gemm_kernel<1, TOv, 1, NWTv, 0, true>), grid, dim3(256), shg, st, pp_src, n, agN, agT, ctx->tm_ld, \
                                           d.K, ctx->tm_ntile, ctx->tm_npair, reinterpret_cast<TOv*>(m.cft), m.tW, (long long)m.ncol, agR, d.N, agK); \
                              else hipLaunchKernelGGL((jx_abel_gemm_kernel<1, TOv, 1, NWTv, 0, false>), grid, dim3(256), shg, st, pp_src, n, agN, agT, ctx->tm_ld, \
                                           d.K, ctx->tm_ntile, ctx->tm_npair, reinterpret_cast<TOv*>(m.cft), m.tW, (long long)m.ncol, agR, d.N, agK); } while (0)
#define JX_AG_GO1(TOv) hipLaunchKernelGGL((jx_abel_gemm_kernel<1, TOv, 1, 2, 1>), dim3(grid.x, (unsigned)((ctx->tm_ntile + 3) / 4)), dim3(256), shg, st, pp_src, n, agN, agT, ctx->tm_ld, \
                                           d.K, ctx->tm_ntile, ctx->tm_npair, reinterpret_cast<TOv*>(m.cft), m.tW, (long long)m.ncol, agR, d.N, agK)
        if (ctx->ag_single && !narrow && !rsg) { if (ctx->f32) JX_AG_GO1(float); else JX_AG_GO1(double); }
        else if (ctx->f32) { if (narrow) JX_AG_GO(float, 1); else JX_AG_GO(float, 2); }
        else { if (narrow) JX_AG_GO(double, 1); else JX_AG_GO(double, 2); }
#undef JX_AG_GO
#undef JX_AG_GO1
        if (!ctx->map_ok && want_abel_taps && !ctx->f32) {
            // the profile taps without the Abel kernel: the pressure profile as the per-walker kernel wrote it, the spline
            // ordinates y_k of the matrix product, the Abel integral as y / y_scale
            if (t.pp) HIPCHK(ctx, hipMemcpyAsync(t.pp, pp_src, sizeof(double) * (size_t)n * d.N, hipMemcpyDeviceToDevice, st));
            if (t.y || t.ab) hipLaunchKernelGGL(jx_unpack_splines_kernel, dim3((unsigned)((d.N + 255) / 256), (unsigned)n), dim3(256), 0, st,
                                                reinterpret_cast<const double2*>(m.cft), m.tW, d.N, d.y_scale, t.y, t.ab);
        }
    } else {
        // phases 1-3 of the Abel kernel (profile, Abel integral, Compton y, spline moments): taps out, arrays walker-minor
        JxDev dm = ctx->d;
        dm.cf_out = m.cft; dm.cf_ws = m.tW; dm.cf_tr = 1;
        launch_map(st, dm, ctx->map_threads, ctx->map_lds, c.theta, c.w0, n, nullptr, t.pp, t.ab, t.y, true);
    }
    if (t.need_img && (rc = launch_y2d(ctx, c))) return rc;
    if (tm || tm2) HIPCHK(ctx, hipEventRecord(es.e[2], st));
    auto between = [&]() -> int { return (side && ctx->side_fork == 1) ? fork_prep() : (int)JX_OK; };   // ("fork": behind stage 1)
    // the matrix-core product computes the outputs the data-radii spline of the tail reads (nrow_use of nrow); the whole row when
    // the row or the brightness profile is tapped
    const bool used = m.has_u && !t.row && !t.bright;
    if ((rc = launch_mix(ctx, n, (tm || tm2) ? &es : nullptr, used, between))) return rc;
    const int nks = used ? m.ksplit_u : m.last_ksplit, nuse = used ? std::min(ctx->nrow_use, d.nrow) : d.nrow;
    const JxOpg& ogt = used ? m.og_u : m.og;
    const size_t sh = sizeof(double) * (JX_LDS_HDR + (size_t)d.nrow + 8);
    if (side) HIPCHK(ctx, hipStreamWaitEvent(st, ctx->ev_side, 0));
    JxDev dtl = d;
    dtl.xr_split = c.xr_split ? 1 : 0;
    dtl.xr_out = ctx->d_xr;
    if (ctx->f32c) hipLaunchKernelGGL(jx_tail_row_kernel<float>, dim3(n), dim3(JX_TAIL_THREADS), sh, st, dtl, reinterpret_cast<const float*>(m.Pt), nks,
                                      ogt.pstride, ogt.ldx, nuse, ctx->d_cfac, ctx->d_sz0, ctx->d_base, c.logp, c.w0, t.row, t.bright, t.chisq, t.parts, c.sm);
    else hipLaunchKernelGGL(jx_tail_row_kernel<double>, dim3(n), dim3(JX_TAIL_THREADS), sh, st, dtl, m.Pt, nks, ogt.pstride, ogt.ldx, nuse,
                            ctx->d_cfac, ctx->d_sz0, ctx->d_base, c.logp, c.w0, t.row, t.bright, t.chisq, t.parts, c.sm);
    return JX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Truncation guard of the low-rank form.  The extracted row (joxsz_funcs.py:472) through the contracted route against the
// rocFFT sequence (exact, independent) on parameter vectors spread over the prior box: the current values and the corners
// of the box in the pressure-profile shape parameters (a, b, r_p) that are thawed.  est = largest difference relative to
// the row's largest entry.
// ---------------------------------------------------------------------------------------------------------------------
static void probe_vectors(jx_ctx* ctx, std::vector<double>& th, int* npts) {
    const jx_config& c = ctx->cfg;
    const std::vector<double> pv = host_vec<double>(ctx, JX_T_PAR_VALS), pmin = host_vec<double>(ctx, JX_T_PAR_MIN), pmax = host_vec<double>(ctx, JX_T_PAR_MAX);
    const std::vector<int32_t> ti = host_vec<int32_t>(ctx, JX_T_THAWED_IDX);
    std::vector<double> base(c.ndim);
    for (int k = 0; k < c.ndim; ++k) base[k] = pv[ti[k]];
    const int shape[3] = {P_A, P_B, P_RP};
    int slot[3] = {-1, -1, -1}, nv = 0;
    for (int s = 0; s < 3; ++s)
        for (int k = 0; k < c.ndim; ++k)
            if (ti[k] == shape[s] && std::isfinite(pmin[shape[s]]) && std::isfinite(pmax[shape[s]]) && pmax[shape[s]] > pmin[shape[s]]) slot[nv++] = k;
    th.assign(base.begin(), base.end());
    int n = 1;
    for (int corner = 0; nv > 0 && corner < (1 << nv); ++corner) {
        std::vector<double> v = base;
        for (int s = 0; s < nv; ++s) {
            const int par = ti[slot[s]];
            // (just inside the box: on the bound itself a profile can degenerate, and the sampler never sits there)
            const double lo = pmin[par] + 0.02 * (pmax[par] - pmin[par]), hi = pmax[par] - 0.02 * (pmax[par] - pmin[par]);
            v[slot[s]] = ((corner >> s) & 1) ? hi : lo;
        }
        th.insert(th.end(), v.begin(), v.end());
        ++n;
    }
    *npts = n;
}

// nothing truncated, every distinct sample and radius evaluated: the exact form, the rocFFT sequence, the full form without sub-grids
static bool mix_truncates(const jx_ctx* ctx) { return ctx->mix.ready && (ctx->mix.form == 0 || !ctx->mix.sub.empty() || ctx->ag_sub_on); }

// est[0] = largest row difference relative to the row's largest entry at the current parameter values, est[1] = the same
// over all probe points, est[2] = largest |difference of the SZ log-likelihood| relative to max(1, |SZ log-likelihood|) over
// all probe points (-1 each where nothing finite came back)
static int measure_truncation(jx_ctx* ctx, double est[3], int* used) {
    est[0] = est[1] = est[2] = -1.0; *used = 0;
    if (!mix_truncates(ctx)) return JX_OK;
    if (!ctx->map_ok) return JX_OK;                                         // nothing to measure against (and every term above rounding is kept)
    const jx_config& c = ctx->cfg;
    int rc, npts = 0;
    std::vector<double> th;
    probe_vectors(ctx, th, &npts);
    if ((rc = ensure_taps(ctx))) return rc;
    if ((rc = ensure_ref(ctx))) return rc;
    npts = std::min(npts, ctx->fft.cap);
    if ((rc = ensure_batch(ctx, npts))) return rc;
    const int nrow = ctx->nrow;
    std::vector<double> ra((size_t)npts * nrow), rb((size_t)npts * nrow), la((size_t)npts * 4), lb((size_t)npts * 4);
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_theta, th.data(), sizeof(double) * (size_t)npts * c.ndim, hipMemcpyHostToDevice, ctx->stream));
    const bool tm = ctx->timing_on;
    ctx->timing_on = false;
    Taps t = all_taps(ctx, false);
    auto fetch = [&](std::vector<double>& rows, std::vector<double>& parts) {
        if (hipMemcpyAsync(rows.data(), ctx->t_row, sizeof(double) * rows.size(), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) return (int)JX_ERR_HIP;
        if (hipMemcpyAsync(parts.data(), ctx->t_parts, sizeof(double) * parts.size(), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) return (int)JX_ERR_HIP;
        return (hipStreamSynchronize(ctx->stream) == hipSuccess) ? (int)JX_OK : (int)JX_ERR_HIP;
    };
    rc = run_chunk(ctx, ctx->d_theta, ctx->d_logp, 0, npts, t);
    if (!rc) rc = fetch(ra, la);
    if (!rc) rc = run_chunk(ctx, ctx->d_theta, ctx->d_logp, 0, npts, t, true);
    if (!rc) rc = fetch(rb, lb);
    ctx->timing_on = tm;
    if (rc) return rc;
    for (int p = 0; p < npts; ++p) {
        double mx = 0.0, df = 0.0;
        bool fin = true;
        for (int k = 0; k < nrow; ++k) {
            const double a = ra[(size_t)p * nrow + k], b = rb[(size_t)p * nrow + k];
            if (!std::isfinite(a) || !std::isfinite(b)) { fin = false; break; }
            mx = std::max(mx, std::fabs(b)); df = std::max(df, std::fabs(a - b));
        }
        const double sa = la[(size_t)p * 4 + 1], sb = lb[(size_t)p * 4 + 1];   // SZ log-likelihood (-chi^2/2 [+ integrated-Compton term])
        if (!fin || !(mx > 0.0) || !std::isfinite(sa) || !std::isfinite(sb)) continue;
        if (p == 0) est[0] = df / mx;
        est[1] = std::max(est[1], df / mx);
        est[2] = std::max(est[2], std::fabs(sa - sb) / std::max(1.0, std::fabs(sb)));
        *used += 1;
    }
    return JX_OK;
}

// The low-rank form drops the small singular values of the transfer-function weights.  What that costs is measured on the
// caller's own beam / transfer function / prior box (measure_truncation); beyond the bounds the tables are rebuilt with
// a cut ten times tighter -- in place: stream, communicator and every other piece of the context stay -- until the
// bounds hold or every term above rounding is kept.
static int mix_guard(jx_ctx* ctx) {
    int rc;
    if (!mix_truncates(ctx)) return JX_OK;
    if ((rc = measure_truncation(ctx, ctx->trunc_est, &ctx->trunc_points))) return rc;
    auto too_large = [&]() {
        // the row at the current parameter values (where the chain lives) within 1e-9 of its largest entry; the SZ
        // log-likelihood at every probe point -- corners of the prior box included -- within 1e-8 relative, a hundred times
        // inside the 1e-6 the log-posterior is held to.  (An estimate that could not be taken counts as too large.)
        return !(ctx->trunc_est[0] >= 0.0 && ctx->trunc_est[0] <= ctx->trunc_bound && ctx->trunc_est[2] >= 0.0 && ctx->trunc_est[2] <= ctx->trunc_bound_ll);
    };
    auto rebuild = [&](double tol) -> int {
        PlanShared sh;
        MixBuild mb;
        if (plan_shared(ctx, host_vec<double>(ctx, JX_T_FILTERING), sh, mb.why))
            plan_mix(ctx, sh, host_vec<double>(ctx, JX_T_BEAM_2D), host_vec<double>(ctx, JX_T_R_PP), tol, choose_form(ctx), ctx->mix.tW, mb);
        if (!mb.ok) { ctx->err = "contracted route, tables rebuilt by the guard: " + mb.why; return JX_ERR_UNSUPPORTED; }
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        const long long tW = ctx->mix.tW;
        mix_teardown(ctx, ctx->mix);
        int rc2 = mix_setup(ctx, mb, tW);
        if (rc2) return rc2;
        HIPCHK(ctx, hipDeviceSynchronize());
        return measure_truncation(ctx, ctx->trunc_est, &ctx->trunc_points);
    };
    // (an f32 context is measured and reported but never rebuilt: the rounding of its spline arrays is of the bounds' size)
    const bool sub_at_start = !ctx->mix.sub.empty(), rad_at_start = ctx->ag_sub_on;
    double tol_now = ctx->mix.tol;
    if (!ctx->f32 && ctx->ag_sub_on && too_large()) {
        // the radial sub-grid of the spline-array product goes first: nothing to rebuild, the full operator is resident
        ctx->ag_sub_on = false; ctx->ag_removed += 1;
        if ((rc = measure_truncation(ctx, ctx->trunc_est, &ctx->trunc_points))) return rc;
    }
    while (!ctx->f32 && (!ctx->mix.sub.empty() || (!ctx->tol_pinned && ctx->mix.form == 0 && (ctx->mix.tol > 2e-13 || ctx->mix.r < ctx->mix.r_tol))) && too_large()) {
        // first the sub-grid of stage 1 goes (every distinct sample evaluated), then the cap on the rank (the same cut, every
        // term above it kept), then the cut tightens
        const bool subbed = !ctx->mix.sub.empty();
        const bool capped = !subbed && ctx->mix.r < ctx->mix.r_tol;
        if (subbed) { ctx->subsample = false; ctx->trunc_unsub += 1; }
        else ctx->trunc_retried += 1;
        if (capped) { ctx->rank_cap = 0; ctx->trunc_uncapped += 1; }
        tol_now = (subbed || capped) ? ctx->mix.tol : std::max(1e-13, ctx->mix.tol * 1e-1);
        if ((rc = rebuild(tol_now))) return rc;
    }
    if (sub_at_start && ctx->trunc_unsub > 0 && ctx->trunc_retried == 0 && too_large()) {
        // every distinct sample evaluated and still outside (a cut set by hand, which is measured but never tightened): the
        // sub-grid was not what the bounds object to
        ctx->subsample = true;
        if ((rc = rebuild(tol_now))) return rc;
        ctx->trunc_unsub = 0;
    } else if (sub_at_start && ctx->trunc_unsub > 0 && ctx->trunc_retried > 0) {
        // the truncation was (also) at fault: the sub-grid once more on the tables the loop ended at, kept when the bounds hold
        ctx->subsample = true;
        if ((rc = rebuild(tol_now))) return rc;
        if (!ctx->mix.sub.empty() && !too_large()) ctx->trunc_unsub = 0;             // (either form: the full form's figures are those of the sub-grid alone)
        else { ctx->subsample = false; if ((rc = rebuild(tol_now))) return rc; }
    }
    if (rad_at_start && !ctx->ag_sub_on && (ctx->trunc_unsub > 0 || ctx->trunc_retried > 0 || too_large())) {
        // something else was (also) at fault: the radial sub-grid once more on what the guard ended at, kept when it changes nothing for the worse
        const double e0 = ctx->trunc_est[0], e2 = ctx->trunc_est[2];
        const bool was_ok = !too_large();
        ctx->ag_sub_on = true;
        if ((rc = measure_truncation(ctx, ctx->trunc_est, &ctx->trunc_points))) return rc;
        const bool keep = was_ok ? !too_large() : (ctx->trunc_est[0] <= 1.5 * e0 + 1e-13 && ctx->trunc_est[2] <= 1.5 * e2 + 1e-13);
        if (keep) ctx->ag_removed = 0;
        else { ctx->ag_sub_on = false; if ((rc = measure_truncation(ctx, ctx->trunc_est, &ctx->trunc_points))) return rc; }
    }
    return JX_OK;
}
