"""The exact form with fp32 products (dtype='f32x': jx_ordrow32_kernel<NXT, CT> of csrc/jx_exact.hpp, NXT = 1 ... 6, contracted and partial rows)
at the cases of sz_chain_reference.CASES -- the smallest shapes that reach each instance -- against the long-double reference of the chain with
the DERIVED bound of tests/sz_chain_f32.py (fp32 roundings counted from the code as built, fp64 roundings as before, an absolute underflow
term) in the place of hand-picked tolerances; test_sz_chain_f32.py shows on the CPU that the bound catches a dropped profile point, macro
step, output or data radius at every case.

Per case three contexts are built once and shared by the tests: f64 with JOXSZ_X_CONTRACT=0 (the source of the walkers' pressure profiles and
conversion factors, as in test_gpu_exact_instances.py), 'f32x' default (contracted) and 'f32x' with JOXSZ_X_CONTRACT=0 (partial rows).  Taps run
the plain pairing of the ordinate tiles, so the folded tile is held through the log-posterior of a JOXSZ_X_FOLD=0 'f32x' context.  Beyond the
bound: launch independence bit for bit, the sampler replayed on the host, the range guard on the pressure profile (the one semantic difference
to f64: -inf where f64 returns about -1e30 or below), the refusals (nothing falls back silently), the audit, and one sweep at 512^2 / 500."""
import numpy as np
import pytest

import sz_chain_reference as szr
import sz_chain_f32 as szf

pytestmark = pytest.mark.gpu

BY_ID = {c['id']: c for c in szr.CASES}
IDS = list(BY_ID)
WIDE = [i for i in IDS if BY_ID[i]['layout']['nxt'] == 5 or BY_ID[i]['layout']['ng_use'] == 2]
FOLDED = [i for i in IDS if BY_ID[i]['layout']['nfold'] > 0]
ONE_RADIUS = ['129-150-19radii', '129-150-32radii', '144-170-19radii', '200-240-19radii']
GUARD = '129-150-19radii'
F32X = ('default', 'partial rows')
_RUNS = {}


def _post(pb, **kw):
    from joxsz_amd.posterior import JoxszPosterior
    return JoxszPosterior(pb, device=0, **kw)


def _describe(case):
    lay = case['layout']
    return '%s NXT %d groups %d/%d Nk %d nS %d pairs %d fold %d ndt %d' % (case['id'], lay['nxt'], lay['ng_use'], lay['ng'], lay['Nk'], lay['nS'],
                                                                             lay['npair'], lay['nfold'], lay['ndt'])


def _assert_layout(post, case, contracted, arithmetic):
    """The live context against the case's table (as test_gpu_exact_instances.py holds the f64 contexts to it), and the arithmetic it reports."""
    lay, c, info = case['layout'], post.ctx.conv_layout, post.ctx.exact_info()
    assert post.ctx.conv == 'custom' and c['form'] == 'exact', c
    assert c['nxt'] == lay['nxt'] and c['ldx'] == 16 * lay['nxt'] * lay['ng_use'] and c['ntile'] == lay['nxt'] * lay['ng'], (c, lay)
    assert c['rank'] == lay['Nk'] and c['beam_terms'] == 16 * lay['nS'], (c, lay)
    assert info['contracted'] == contracted and info['doubles_per_partial_row'] == c['ldx'], info
    if contracted:
        assert info['doubles_per_contracted_partial'] == case['nflux'] and (case['nflux'] + 15) // 16 == lay['ndt']
    assert info['arithmetic'] == arithmetic, info
    assert (info['pp_limit_log2'] >= 32) if arithmetic == 'f32 products' else (info['pp_limit_log2'] == 0), info


def _taps(post, th, pp=False):
    o = dict(logp=post.log_prob(th))
    o['launch_logp'] = post.ctx.exact_info()['last_launch']
    o['chisq'] = post.stage(th, 'chisq')
    o['launch_chisq'] = post.ctx.exact_info()['last_launch']
    o['parts'] = post.stage(th, 'parts')
    o['row'], o['bright'] = post.stage(th, 'map_row'), post.stage(th, 'bright')
    if pp:
        o['pp'] = post.stage(th, 'pp')
    return o


def _run(cid):
    """The three contexts of a case, evaluated once; the chain's reference with the bounds of the fp32 products."""
    if cid in _RUNS:
        return _RUNS[cid]
    case = BY_ID[cid]
    pb, th = szr.build_case(case)
    ch = szf.SzChainF32(chain=szr.oriented_chain(pb, th))
    assert {k: ch.layout[k] for k in case['layout']} == case['layout'], ch.layout
    r = dict(case=case, pb=pb, th=th, chain=ch)
    for name, kw in (('f64', dict(options={'X_CONTRACT': '0'})), ('default', dict(dtype='f32x')), ('partial rows', dict(dtype='f32x', options={'X_CONTRACT': '0'}))):
        post = _post(pb, **kw)
        try:
            _assert_layout(post, case, contracted=(name == 'default' and case['layout']['contracted']), arithmetic='f64' if name == 'f64' else 'f32 products')
            r[name] = _taps(post, th, pp=(name == 'f64'))
            r[name]['info'] = post.ctx.exact_info()
        finally:
            post.close()
    b = r['f64']
    fin = np.isfinite(b['logp'])
    assert np.isfinite(b['row'][fin]).all() and np.all(b['row'][fin] != 0.0) and np.isfinite(b['bright'][fin]).all() and np.isfinite(b['pp'][fin]).all()
    r['fin'] = fin
    r['pp'], r['cf'] = b['pp'][fin], b['bright'][fin] / b['row'][fin]
    r['ref'] = ch.reference(r['pp'], r['cf'])
    _RUNS[cid] = r
    return r


@pytest.mark.parametrize('cid', IDS)
def test_layout_arithmetic_and_accepted_walkers(cid):
    """dtype='f32x' builds (it raises without the feature), takes the exact form with the layout of the case's table, reports 'f32 products' and a
    range guard of at least 2^32; the same walkers are finite as in f64: at least 15 of 21, never walker 2 (outside the box) or 4 (NaN)."""
    r = _run(cid)
    fin, th = r['fin'], r['th']
    assert fin.sum() >= 15 and not fin[2] and not fin[4], fin
    for name in F32X:
        assert np.array_equal(np.isfinite(r[name]['logp']), fin), (name, r[name]['logp'])
        assert not np.isnan(r[name]['logp']).any()
    print('%s | %d of %d walkers accepted | T = 2^%d' % (_describe(r['case']), fin.sum(), th.shape[0], r['default']['info']['pp_limit_log2']))


@pytest.mark.parametrize('cid', IDS)
def test_rows_against_the_reference(cid):
    """Row and brightness taps of both 'f32x' contexts, element by element, within the fp32 row bound of the long-double row (the brightness
    within row_bound |cf| of cf row_ref) at every output and every accepted walker."""
    r = _run(cid)
    ref, fin, cf = r['ref'], r['fin'], r['cf']
    worst = {}
    for name in F32X:
        o = r[name]
        assert o['row'].shape == (szr.NWALKERS, r['chain'].nrow)
        worst[name] = (szr.ratio(o['row'][fin], ref['row'], ref['row_bound']), szr.ratio(o['bright'][fin], cf * ref['row'], ref['row_bound'] * np.abs(cf)))
    print('%s | n32 = %d, n = %d | row, brightness of the bound: %s' % (_describe(r['case']), r['chain'].n32, r['chain'].n_terms,
                                                                        '  '.join('%s %.3f %.3f' % (k, *v) for k, v in worst.items())))
    for name, v in worst.items():
        assert max(v) <= 1.0, (name, v)


@pytest.mark.parametrize('cid', IDS)
def test_chisq_and_log_posterior(cid):
    """chi^2 of both forms within the fp32 chi_bound of the long-double chi^2; contracted against partial rows: SZ log-likelihood and log-posterior
    differ by at most chi_bound; the log-posterior against the f64 context's within chi_bound / 2 + u (|logp| + |logp'|); the last_launch
    reports match the form."""
    r = _run(cid)
    ref, fin = r['ref'], r['fin']
    form = 'contracted' if r['case']['layout']['contracted'] else 'partial rows'
    a, b, d = r['default'], r['partial rows'], r['f64']
    assert a['launch_logp'] == form and a['launch_chisq'] == form, a
    assert b['launch_logp'] == 'partial rows' and b['launch_chisq'] == 'partial rows', b
    worst = {name: szr.ratio(r[name]['chisq'][fin], ref['chi2'], ref['chi_bound']) for name in F32X}
    d_ll = szr.ratio(a['parts'][fin, 1], b['parts'][fin, 1].astype(szr.LD), ref['chi_bound'])
    d_lp = szr.ratio(a['logp'][fin], b['logp'][fin].astype(szr.LD), ref['chi_bound'])
    d_64 = {name: szr.ratio(r[name]['logp'][fin], d['logp'][fin].astype(szr.LD), ref['chi_bound'] / 2 + szr.U * (np.abs(r[name]['logp'][fin]) + np.abs(d['logp'][fin])))
            for name in F32X}
    print('%s | chi^2 %.3g ... %.3g, chi_bound / chi^2 <= %.1e | chi^2 of the bound: %s | contracted - partial rows: ll %.3f  logp %.3f | logp - f64 logp of its bound: %s | '
          'max |logp - f64 logp| %.2e' % (_describe(r['case']), ref['chi2'].min(), ref['chi2'].max(), np.max(ref['chi_bound'] / ref['chi2'].astype(np.float64)),
                                          '  '.join('%s %.3f' % kv for kv in worst.items()), d_ll, d_lp, '  '.join('%s %.3f' % kv for kv in d_64.items()),
                                          np.max(np.abs(a['logp'][fin] - d['logp'][fin]))))
    for name in F32X:
        assert np.isfinite(r[name]['chisq'][fin]).all(), name
    assert max(worst.values()) <= 1.0, worst
    assert d_ll <= 1.0 and d_lp <= 1.0, (d_ll, d_lp)
    assert max(d_64.values()) <= 1.0, d_64


@pytest.mark.parametrize('cid', FOLDED)
def test_folded_tile_through_the_log_posterior(cid):
    """The folded last ordinate tile -- an fp32 operator on the fp32 profile, continuing the upper tile's chain -- is reached by the log-posterior
    alone: held against a JOXSZ_X_FOLD=0 'f32x' context with the f64 test's formula and the fp32 bound, contracted and partial rows."""
    r = _run(cid)
    pb, th, fin, bound = r['pb'], r['th'], r['fin'], r['ref']['chi_bound']
    worst = {}
    for name, opt in (('default', {}), ('partial rows', {'X_CONTRACT': '0'})):
        plain = _post(pb, dtype='f32x', options=dict(opt, X_FOLD='0'))
        try:
            _assert_layout(plain, r['case'], contracted=(name == 'default'), arithmetic='f32 products')
            lp = plain.log_prob(th)
        finally:
            plain.close()
        folded = r[name]['logp']
        assert np.array_equal(np.isfinite(lp), fin)
        worst[name] = szr.ratio(folded[fin], lp[fin].astype(szr.LD), bound + szr.U * (np.abs(folded[fin]) + np.abs(lp[fin])))
    print('%s | folded - plain pairing, logp of chi_bound + u (|logp| + |logp\'|): %s' % (_describe(r['case']), '  '.join('%s %.3f' % kv for kv in worst.items())))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize('cid', ONE_RADIUS)
def test_one_data_radius_at_a_time(cid):
    """The permuted data-radii operand at the tile edges: the flux errors times 1e30 everywhere but at data radius j = 0, 15, 16 and the last, so
    that chi^2 is that radius's term; contracted and partial rows against the chi_bound formula with those errors."""
    r = _run(cid)
    pb, th, fin, ch = r['pb'], r['th'], r['fin'], r['chain']
    nflux = r['case']['nflux']
    fd0 = pb.flux_data.copy()
    worst = {}
    try:
        for j in sorted({min(j, nflux - 1) for j in (0, 15, 16, nflux - 1)}):
            err = fd0[2] * 1e30
            err[j] = fd0[2, j]
            pb.flux_data = np.ascontiguousarray(np.vstack((fd0[0], fd0[1], err)))
            ref = ch.reference(r['pp'], r['cf'], errors=err)
            term = ((fd0[1, j] - ref['m'][:, j]) / fd0[2, j]) ** 2
            assert np.all(np.abs(ref['chi2'] - term) <= 1e-50 * nflux)
            for name, opt in (('default', None), ('partial rows', {'X_CONTRACT': '0'})):
                post = _post(pb, dtype='f32x', options=opt)
                try:
                    chi = post.stage(th, 'chisq')
                    assert post.ctx.exact_info()['last_launch'] == ('contracted' if name == 'default' else 'partial rows')
                finally:
                    post.close()
                assert np.isfinite(chi[fin]).all()
                worst[(j, name)] = szr.ratio(chi[fin], ref['chi2'], ref['chi_bound'])
    finally:
        pb.flux_data = fd0
    print('%s | chi^2 of one data radius, of the bound: %s' % (_describe(r['case']), '  '.join('j=%d %s %.3f' % (*k, v) for k, v in worst.items())))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize('cid', WIDE)
def test_launch_independence(cid):
    """The first 1, 15, 16 and 17 walkers evaluated alone get the bits they get in the launch of 21, a permuted launch the permuted bits, and so
    does a context that evaluates 16 walkers at a time."""
    r = _run(cid)
    pb, th, lp = r['pb'], r['th'], r['default']['logp']
    perm = np.random.default_rng(r['case']['S']).permutation(th.shape[0])
    post = _post(pb, dtype='f32x')
    try:
        for n in (1, 15, 16, 17):
            np.testing.assert_array_equal(post.log_prob(th[:n]), lp[:n], err_msg='first %d' % n)
        np.testing.assert_array_equal(post.log_prob(th[perm]), lp[perm], err_msg='permuted')
        assert post.ctx.exact_info()['last_launch'] == 'contracted'
    finally:
        post.close()
    small = _post(pb, dtype='f32x', max_batch=16)
    try:
        np.testing.assert_array_equal(small.log_prob(th), lp, err_msg='max_batch=16')
    finally:
        small.close()


def test_sampler_replays_on_the_host():
    """A 6-walker sample() of 4 steps on an 'f32x' context (acceptance inside the tail) replays on the host, bit for bit, with that context's
    log_prob."""
    from joxsz_amd.sampler import DeviceStretchMove
    r = _run(GUARD)
    p0 = r['th'][r['fin']][:6]
    post = _post(r['pb'], dtype='f32x')
    try:
        s = DeviceStretchMove(post, seed=5)
        chain, lp, nacc = s.run(p0, 4)
        rc, rl, rn = s.replay(p0, 4)
    finally:
        post.close()
    print('sampler on f32x: accepted %s | max |chain - replay| %.3g  max |logp - replay| %.3g' % (nacc.tolist(), np.max(np.abs(chain - rc)), np.max(np.abs(lp - rl))))
    np.testing.assert_array_equal(nacc, rn)
    np.testing.assert_array_equal(chain, rc)
    np.testing.assert_array_equal(lp, rl)


def test_range_guard():
    """129 / 150, 19 radii, par_max of the pressure normalisation widened in the test's own problem: one walker inside the box with
    max |pp| = 8 T gets -inf from log_prob, with JOXSZ_X_CONTRACT=0, and from the launches of the chi^2 tap -- whose log-posterior is what
    log_prob of a JOXSZ_X_FOLD=0 context returns (plain pairing, ordinates stored) -- where f64 returns a finite value; the other 20 walkers
    keep, bit for bit, the values of a launch without it (their chi^2 taps too, and the rejected walker's own chi^2 stays finite: its column
    was kept finite).  jx_finalize succeeded, so T >= 2^32 held."""
    import copy
    r = _run(GUARD)
    pb, th = copy.deepcopy(r['pb']), r['th'].copy()
    k, i = pb.par_names.index('P_0'), pb.thawed.index('P_0')
    pb.par_max = np.array(pb.par_max, dtype=np.float64)
    pb.par_max[k] = 1e300
    w = int(np.flatnonzero(r['fin'])[5])
    f64 = _post(pb)
    try:
        pp_max = np.abs(f64.stage(th[w:w + 1], 'pp')).max()
        res = {}
        for name, opt in (('default', None), ('partial rows', {'X_CONTRACT': '0'}), ('chi^2-tap launches', {'X_FOLD': '0'})):
            post = _post(pb, dtype='f32x', options=opt)
            try:
                info = post.ctx.exact_info()
                t_log2 = info['pp_limit_log2']
                assert t_log2 >= 32 and info['arithmetic'] == 'f32 products', info
                big = th.copy()
                big[w, i] = th[w, i] * (8.0 * 2.0 ** t_log2 / pp_max)         # the profile is linear in its normalisation: max |pp| = 8 T
                res[name] = dict(clean=post.log_prob(th), lp=post.log_prob(big), chi_clean=post.stage(th, 'chisq'), chi=post.stage(big, 'chisq'), t_log2=t_log2)
            finally:
                post.close()
        lp64 = f64.log_prob(big)
        assert np.abs(f64.stage(big[w:w + 1], 'pp')).max() > 2.0 ** t_log2
    finally:
        f64.close()
    others = np.arange(th.shape[0]) != w
    print('range guard: T = 2^%d, walker %d at max |pp| = 8 T: f64 logp %.3e | f32x %s' % (t_log2, w, lp64[w], '  '.join('%s %s' % (n_, o['lp'][w]) for n_, o in res.items())))
    assert np.isfinite(lp64[w])
    for name, o in res.items():
        assert np.isfinite(o['clean'][w]) and o['lp'][w] == -np.inf, (name, o['lp'][w])
        assert not np.isnan(o['lp']).any()
        np.testing.assert_array_equal(o['lp'][others], o['clean'][others], err_msg=name)
        np.testing.assert_array_equal(o['chi'][others], o['chi_clean'][others], err_msg=name)
        assert np.isfinite(o['chi'][w]), (name, o['chi'][w])


@pytest.mark.parametrize('kw, word', [(dict(conv='rocfft'), 'rocFFT'), (dict(options={'MIX_FORM': 'legacy'}), 'MIX_FORM'), (dict(options={'X_PAIRWISE': '0'}), 'X_PAIRWISE')],
                         ids=['rocfft', 'mix_form', 'pairwise'])
def test_refusals_at_finalize(kw, word):
    """dtype='f32x' never falls back: the rocFFT sequence, a contracted form and the f64-only reference kernels are refused at jx_finalize with a reason."""
    from joxsz_amd.hip_backend import JoxszHipError
    r = _run('32-40-5radii')
    with pytest.raises(JoxszHipError) as ei:
        _post(r['pb'], dtype='f32x', **kw).close()
    msg = str(ei.value)
    print(msg)
    assert 'jx_finalize' in msg and 'f32x' in msg and word in msg and ' -- ' in msg, msg


def test_operator_route_is_refused():
    from joxsz_amd.hip_backend import JoxszHipError
    r = _run('32-40-5radii')
    post = _post(r['pb'], dtype='f32x')
    try:
        with pytest.raises(JoxszHipError) as ei:
            post.ctx.set_route('operator')
        assert 'f32x' in str(ei.value) and 'operator' in str(ei.value), str(ei.value)
        assert post.ctx.route == 'map'
        np.testing.assert_array_equal(post.log_prob(r['th']), r['default']['logp'])
    finally:
        post.close()
    with pytest.raises(JoxszHipError):
        _post(r['pb'], dtype='f32x', route='operator').close()


def test_audit():
    """audit() on an 'f32x' context (129 / 150): its route against the rocFFT sequence held inside it, in f64.  The largest SZ log-likelihood
    difference is at most the largest chi_bound / 2 of the audited walkers plus 1e-8, the exact-versus-literal bar of test_gpu_exact.py."""
    r = _run(GUARD)
    post = _post(r['pb'], dtype='f32x')
    try:
        res = post.ctx.audit(r['th'])
    finally:
        post.close()
    bar = float(np.max(r['ref']['chi_bound'])) / 2 + 1e-8
    print('audit on f32x: %s | bar %.3e' % (res, bar))
    assert res['walkers_compared'] == int(r['fin'].sum())
    assert res['max_abs_sz_loglike_diff'] <= bar, (res, bar)


def test_sweep_at_the_headline_shape():
    """512^2 / 500 points, 32 walkers of walker_ball: 'f32x' against f64.  Printed: the largest and median relative log-posterior difference and the
    largest |delta chi^2 / 2|; asserted: the derived bound alone."""
    from joxsz_amd import datasets
    from oracle import joxsz_oracle as orc
    pb = datasets.synthetic_problem(S=512, N=500, seed=12)
    p0 = orc.pars_dict(pb, datasets.fiducial_theta(pb))
    datasets.fill_data(pb, orc.sz_stages(pb, p0)['bright'], orc.calc_profiles(pb, p0), seed=12)
    th = datasets.walker_ball(pb, 32, spread=0.03, seed=12)
    ch = szf.SzChainF32(chain=szr.oriented_chain(pb, th))
    f64 = _post(pb, options={'X_CONTRACT': '0'})
    try:
        lp64, chi64 = f64.log_prob(th), f64.stage(th, 'chisq')
        row, bright, pp = f64.stage(th, 'map_row'), f64.stage(th, 'bright'), f64.stage(th, 'pp')
    finally:
        f64.close()
    x = _post(pb, dtype='f32x')
    try:
        info = x.ctx.exact_info()
        lpx, chix = x.log_prob(th), x.stage(th, 'chisq')
        assert x.ctx.exact_info()['arithmetic'] == 'f32 products'
    finally:
        x.close()
    fin = np.isfinite(lp64)
    assert fin.sum() >= 24 and np.array_equal(np.isfinite(lpx), fin)
    ref = ch.reference(pp[fin], bright[fin] / row[fin])
    rel = np.abs(lpx[fin] - lp64[fin]) / np.abs(lp64[fin])
    dchi = np.abs(chix[fin] - chi64[fin]) / 2
    r_chi = szr.ratio(chix[fin], ref['chi2'], ref['chi_bound'])
    r_lp = szr.ratio(lpx[fin], lp64[fin].astype(szr.LD), ref['chi_bound'] / 2 + szr.U * (np.abs(lpx[fin]) + np.abs(lp64[fin])))
    print('sweep 512^2 / 500, %d of 32 walkers, n32 = %d, T = 2^%d: f32x against f64: relative log-posterior difference max %.3e median %.3e | max |delta chi^2 / 2| %.3e | '
          'chi_bound / 2 %.2e ... %.2e | chi^2 %.3f, logp %.3f of the bound' % (fin.sum(), ch.n32, info['pp_limit_log2'], rel.max(), np.median(rel), dchi.max(),
                                                                               ref['chi_bound'].min() / 2, ref['chi_bound'].max() / 2, r_chi, r_lp))
    assert r_chi <= 1.0 and r_lp <= 1.0, (r_chi, r_lp)
