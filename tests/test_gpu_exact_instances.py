"""Every instance of the exact-form kernels (csrc/jx_exact.hpp: jx_ordrow_kernel<NXT, CT>, jx_rowsum_tail_kernel<NXT, CT>, jx_rowop_tail_kernel<NXT>,
NXT = 1 ... 6 output tiles per block, contracted and partial rows) at the smallest shapes that reach it, against a long-double reference of
the same linear chain with a DERIVED forward error bound (tests/sz_chain_reference.py: n = N + Nkp + 16 NXT ng_use + 32 rounded terms, gamma_n
times the sums of absolute terms) in place of hand-picked tolerances.  Which instance runs is fixed by the problem alone, so each case first
holds the live context to the layout it was chosen for (sz_chain_reference.CASES; the same table is held to the host tables on the CPU in
test_sz_chain_reference.py, where the bound is also shown to catch one dropped output, profile point, macro step or data radius).

The inputs of the reference are the walkers' pressure profiles (the pp tap) and conversion factors (brightness tap / row tap) of the
JOXSZ_X_CONTRACT=0 context; per case the default context (contracted), JOXSZ_X_CONTRACT=0 (partial rows) and -- for NXT = 1, 3, 5 --
JOXSZ_X_PAIRWISE=0 (the reference kernels) are evaluated once and shared by the tests below.  Every tap runs the plain pairing of the
ordinate tiles, so the folded last tile is held through the log-posterior of a JOXSZ_X_FOLD=0 context
(test_folded_tile_through_the_log_posterior; what that can and cannot see is written down in DESIGN 6.2).  The oracle and the rocFFT sequence stay the
independent checks at the bars of test_gpu_exact.py."""
import numpy as np
import pytest

from oracle import joxsz_oracle as orc

import sz_chain_reference as szr

pytestmark = pytest.mark.gpu

BY_ID = {c['id']: c for c in szr.CASES}
IDS = list(BY_ID)
# the NXT = 5 cases and the two-group cases: rocFFT row and launch independence (the other instances have both in test_gpu_exact.py / test_gpu_contract.py)
WIDE = [i for i in IDS if BY_ID[i]['layout']['nxt'] == 5 or BY_ID[i]['layout']['ng_use'] == 2]
FOLDED = [i for i in IDS if BY_ID[i]['layout']['nfold'] > 0]
ONE_RADIUS = ['129-150-19radii', '129-150-32radii', '144-170-19radii', '200-240-19radii']
_RUNS = {}


def _post(pb, **kw):
    from joxsz_amd.posterior import JoxszPosterior
    return JoxszPosterior(pb, device=0, **kw)


def _describe(case, lay):
    return '%s NXT %d groups %d/%d Nk %d nS %d pairs %d fold %d ndt %d' % (case['id'], lay['nxt'], lay['ng_use'], lay['ng'], lay['Nk'], lay['nS'],
                                                                             lay['npair'], lay['nfold'], lay['ndt'])


def _assert_layout(post, case, contracted):
    """The live context against the case's table: form, NXT, outputs computed, output tiles, ordinates in use, ordinate tiles, data radii."""
    lay, c, info = case['layout'], post.ctx.conv_layout, post.ctx.exact_info()
    assert post.ctx.conv == 'custom' and c['form'] == 'exact', c
    assert c['nxt'] == lay['nxt'] and c['ldx'] == 16 * lay['nxt'] * lay['ng_use'] and c['ntile'] == lay['nxt'] * lay['ng'], (c, lay)
    assert c['rank'] == lay['Nk'] and c['beam_terms'] == 16 * lay['nS'], (c, lay)
    assert info['contracted'] == contracted and info['doubles_per_partial_row'] == c['ldx'], info
    if contracted:
        assert info['doubles_per_contracted_partial'] == case['nflux'] and (case['nflux'] + 15) // 16 == lay['ndt']


def _run(cid):
    """The three contexts of a case, evaluated once: taps, chi^2, parts and log-posterior of each, the chain's reference and its bounds."""
    if cid in _RUNS:
        return _RUNS[cid]
    case = BY_ID[cid]
    pb, th = szr.build_case(case)
    ch = szr.oriented_chain(pb, th)
    assert {k: ch.layout[k] for k in case['layout']} == case['layout'], ch.layout
    r = dict(case=case, pb=pb, th=th, chain=ch)
    options = {'default': None, 'partial rows': {'X_CONTRACT': '0'}}
    if case['layout']['nxt'] in (1, 3, 5):
        options['reference kernels'] = {'X_PAIRWISE': '0'}
    for name, opt in options.items():
        post = _post(pb, options=opt)
        try:
            _assert_layout(post, case, contracted=(name == 'default' and case['layout']['contracted']))
            o = dict(logp=post.log_prob(th))
            o['launch_logp'] = post.ctx.exact_info()['last_launch']
            o['chisq'] = post.stage(th, 'chisq')
            o['launch_chisq'] = post.ctx.exact_info()['last_launch']
            o['parts'] = post.stage(th, 'parts')
            o['row'], o['bright'] = post.stage(th, 'map_row'), post.stage(th, 'bright')
            if name == 'partial rows':
                o['pp'] = post.stage(th, 'pp')
        finally:
            post.close()
        r[name] = o
    b = r['partial rows']
    fin = np.isfinite(b['logp'])
    # the cap on rejections, the two named ones, and the same set in every form
    assert fin.sum() >= th.shape[0] - 6 and not fin[2] and not fin[4], fin
    for name in options:
        assert np.array_equal(np.isfinite(r[name]['logp']), fin), name
    assert np.isfinite(b['row'][fin]).all() and np.all(b['row'][fin] != 0.0) and np.isfinite(b['bright'][fin]).all() and np.isfinite(b['pp'][fin]).all()
    r['fin'] = fin
    r['pp'], r['cf'] = b['pp'][fin], b['bright'][fin] / b['row'][fin]
    r['ref'] = ch.reference(r['pp'], r['cf'])
    r['forms'] = list(options)
    _RUNS[cid] = r
    return r


@pytest.mark.parametrize('cid', IDS)
def test_rows_against_the_reference(cid):
    """(a) Partial rows and reference kernels, element by element: the row tap within row_bound of the long-double row at every output and
    every accepted walker, the brightness tap within row_bound |cf| of cf row_ref; the default context's taps (partial rows with every output
    group) and the JOXSZ_X_PAIRWISE=0 context's meet the same bars."""
    r = _run(cid)
    ref, fin, cf = r['ref'], r['fin'], r['cf']
    worst = {}
    for name in r['forms']:
        o = r[name]
        assert o['row'].shape == (szr.NWALKERS, r['chain'].nrow)
        worst[name] = (szr.ratio(o['row'][fin], ref['row'], ref['row_bound']), szr.ratio(o['bright'][fin], cf * ref['row'], ref['row_bound'] * np.abs(cf)))
    print('%s | n = %d | row, brightness of the bound: %s' % (_describe(r['case'], r['case']['layout']), r['chain'].n_terms,
                                                              '  '.join('%s %.3f %.3f' % (k, *v) for k, v in worst.items())))
    for name, v in worst.items():
        assert max(v) <= 1.0, (name, v)


@pytest.mark.parametrize('cid', IDS)
def test_chisq_against_the_reference(cid):
    """(b) The contracted form: after the chi^2 tap (and after the log-posterior) the default context reports a contracted launch, the others
    partial rows; chi^2 of every form within chi_bound of the long-double chi^2 for every accepted walker; the SZ log-likelihood and the
    log-posterior of the default and the JOXSZ_X_CONTRACT=0 contexts differ by at most chi_bound."""
    r = _run(cid)
    ref, fin = r['ref'], r['fin']
    form = 'contracted' if r['case']['layout']['contracted'] else 'partial rows'
    a, b = r['default'], r['partial rows']
    assert a['launch_logp'] == form and a['launch_chisq'] == form, a
    assert b['launch_logp'] == 'partial rows' and b['launch_chisq'] == 'partial rows', b
    worst = {name: szr.ratio(r[name]['chisq'][fin], ref['chi2'], ref['chi_bound']) for name in r['forms']}
    d_ll = szr.ratio(a['parts'][fin, 1], b['parts'][fin, 1].astype(szr.LD), ref['chi_bound'])
    d_lp = szr.ratio(a['logp'][fin], b['logp'][fin].astype(szr.LD), ref['chi_bound'])
    print('%s | chi^2 %.3g ... %.3g, chi_bound / chi^2 <= %.1e | chi^2 of the bound: %s | contracted - partial rows: ll %.3f  logp %.3f' % (
        _describe(r['case'], r['case']['layout']), ref['chi2'].min(), ref['chi2'].max(), np.max(ref['chi_bound'] / ref['chi2'].astype(np.float64)),
        '  '.join('%s %.3f' % kv for kv in worst.items()), d_ll, d_lp))
    for name in r['forms']:
        assert np.isfinite(r[name]['chisq'][fin]).all(), name
    assert max(worst.values()) <= 1.0, worst
    assert d_ll <= 1.0 and d_lp <= 1.0, (d_ll, d_lp)


@pytest.mark.parametrize('cid', FOLDED)
def test_folded_tile_through_the_log_posterior(cid):
    """Every tap -- chi^2 included -- runs the plain pairing: the folded last ordinate tile (and with it the a2 loop of fold steps beyond the
    pairs) is reached by the log-posterior alone.  Its chi^2 is pinned through the JOXSZ_X_FOLD=0 context, whose log-posterior runs the launches
    of the chi^2 tap held to the reference above: both chi^2 lie within chi_bound of the reference, so the two SZ log-likelihoods differ by
    at most chi_bound, and the two totals -- the same priors and X-ray term, one rounding each -- by at most chi_bound + u (|logp| + |logp'|).
    Contracted and partial rows (the latter against its own JOXSZ_X_FOLD=0 context)."""
    r = _run(cid)
    pb, th, fin, bound = r['pb'], r['th'], r['fin'], r['ref']['chi_bound']
    worst = {}
    for name, opt in (('default', {}), ('partial rows', {'X_CONTRACT': '0'})):
        plain = _post(pb, options=dict(opt, X_FOLD='0'))
        try:
            _assert_layout(plain, r['case'], contracted=(name == 'default'))
            lp = plain.log_prob(th)
        finally:
            plain.close()
        folded = r[name]['logp']
        assert np.array_equal(np.isfinite(lp), fin)
        worst[name] = szr.ratio(folded[fin], lp[fin].astype(szr.LD), bound + szr.U * (np.abs(folded[fin]) + np.abs(lp[fin])))
    print('%s | folded - plain pairing, logp of chi_bound + u (|logp| + |logp\'|): %s | |logp| <= %.3g' % (
        _describe(r['case'], r['case']['layout']), '  '.join('%s %.3f' % kv for kv in worst.items()), np.max(np.abs(r['default']['logp'][fin]))))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize('cid', ONE_RADIUS)
def test_one_data_radius_at_a_time(cid):
    """(c) The edges of the data-radii tiles: the flux errors times 1e30 everywhere but at data radius j = 0, 15, 16 and the last, so that
    chi^2 is that radius's term (a dropped radius whose residual happens to be near 0 would vanish in the sum); contracted and partial rows
    against the same chi_bound formula with those errors."""
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
                post = _post(pb, options=opt)
                try:
                    chi = post.stage(th, 'chisq')
                    assert post.ctx.exact_info()['last_launch'] == ('contracted' if name == 'default' else 'partial rows')
                finally:
                    post.close()
                assert np.isfinite(chi[fin]).all()
                worst[(j, name)] = szr.ratio(chi[fin], ref['chi2'], ref['chi_bound'])
    finally:
        pb.flux_data = fd0
    print('%s | chi^2 of one data radius, of the bound: %s' % (_describe(r['case'], r['case']['layout']), '  '.join('j=%d %s %.3f' % (*k, v) for k, v in worst.items())))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize('cid', IDS)
def test_against_the_oracle_and_the_rocfft_sequence(cid):
    """(d) The independent checks at the bars of test_gpu_exact.py: the log-posterior of the first three walkers against the oracle (rtol
    1e-11 from side 128 up, 1e-9 below); for the NXT = 5 and two-group cases the row tap within 1e-12 of its maximum of the rocFFT sequence's."""
    r = _run(cid)
    pb, th, S = r['pb'], r['th'], r['case']['S']
    want = orc.log_posterior_batch(pb, th[:3])
    got = r['default']['logp'][:3]
    ok = np.isfinite(want)
    rel = np.max(np.abs(got[ok] - want[ok]) / np.abs(want[ok]))
    rrow = -1.0
    if cid in WIDE:
        ref = _post(pb, conv='rocfft')
        try:
            row_b, lp_b = ref.stage(th, 'map_row'), ref.log_prob(th)
        finally:
            ref.close()
        assert np.array_equal(np.isfinite(lp_b), r['fin'])
        rrow = np.max(np.abs(r['default']['row'] - row_b)[r['fin']] / np.max(np.abs(row_b[r['fin']]), axis=1, keepdims=True))
    print('%s | logp against the oracle rel %.1e | row against the rocFFT sequence %.1e of its maximum' % (_describe(r['case'], r['case']['layout']), rel, rrow))
    np.testing.assert_allclose(got, want, rtol=1e-11 if S >= 128 else 1e-9)
    assert rrow <= 1e-12


@pytest.mark.parametrize('cid', WIDE)
def test_launch_independence(cid):
    """(e) NXT = 5 and the two-group cases: the first 1, 15, 16 and 17 walkers evaluated alone get the bits they get in the launch of 21, a
    permuted launch gives the permuted bits, and so does a context that evaluates 16 walkers at a time."""
    r = _run(cid)
    pb, th, lp = r['pb'], r['th'], r['default']['logp']
    perm = np.random.default_rng(r['case']['S']).permutation(th.shape[0])
    post = _post(pb)
    try:
        for n in (1, 15, 16, 17):
            np.testing.assert_array_equal(post.log_prob(th[:n]), lp[:n], err_msg='first %d' % n)
        np.testing.assert_array_equal(post.log_prob(th[perm]), lp[perm], err_msg='permuted')
        assert post.ctx.exact_info()['last_launch'] == 'contracted'
    finally:
        post.close()
    small = _post(pb, max_batch=16)
    try:
        np.testing.assert_array_equal(small.log_prob(th), lp, err_msg='max_batch=16')
    finally:
        small.close()
    print('%s | launches of 1, 15, 16, 17, a permutation and max_batch=16: the bits of the launch of %d' % (_describe(r['case'], r['case']['layout']), th.shape[0]))
