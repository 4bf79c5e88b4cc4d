"""The pair-wise kernels of the exact form read the row and fold operators tile-major (jxt::row_tile_major; jx_ordrow_kernel and
jx_ordrow32_kernel of csrc/jx_exact.hpp: the row operator's load, the fold operator's load and the a2 loop of fold steps beyond the pairs),
the reference kernel (JOXSZ_X_PAIRWISE=0, jx_rowop_tail_kernel) still reads exact_row_layout's own order.  At the smallest shapes that
reach one tile, a fold with one tile, three, four (two groups allocated, one in use), five tiles with a fold, the a2 loop, two groups of six
and two groups with a fold: the row tap and the log-posterior of the default context (contracted) and of JOXSZ_X_CONTRACT=0 (partial rows)
against the reference kernel's, at the derived bars of tests/sz_chain_reference.py -- no tolerance of this file's own:

    row         both within row_bound of the long-double row, so within 2 row_bound of one another (each is also held to row_bound itself)
    log_prob    both chi^2 within chi_bound of the long-double chi^2, so the SZ log-likelihoods within chi_bound of one another and the
                totals -- the same priors and X-ray term, one rounding each -- within chi_bound + u (|logp| + |logp'|)

and the 'f32x' context to the bound of tests/sz_chain_f32.py (row_bound of the fp32 products; its log-posterior against the f64 reference
kernel's within half the sum of the fp32 and the f64 chi_bound, plus u (|logp| + |logp'|)).  The rejected
walkers 2 and 4 are -inf everywhere, and launches of 16, 17 and 21 walkers give the same bits.  Needs an MI355X: run with -m gpu."""
import numpy as np
import pytest

import sz_chain_f32 as szf
import sz_chain_reference as szr

pytestmark = pytest.mark.gpu

BY_ID = {c['id']: c for c in szr.CASES}
IDS = ['15-16-5radii', '32-40-5radii', '65-80-19radii', '129-150-5radii', '144-170-19radii', '130-300-19radii', '200-240-19radii', '224-260-19radii']
CONTEXTS = (('reference kernels', dict(options={'X_PAIRWISE': '0'})), ('default', {}), ('partial rows', dict(options={'X_CONTRACT': '0'})),
            ('f32x', dict(dtype='f32x')))
_RUNS = {}


def _post(pb, **kw):
    from joxsz_amd.posterior import JoxszPosterior
    return JoxszPosterior(pb, device=0, **kw)


def _run(cid):
    """The four contexts of a case, evaluated once: log-posterior at launches of 21, 17 and 16 walkers, the row tap; the pressure profiles
    and conversion factors of the reference kernels' context feed the long-double reference and its f64 and fp32 bounds."""
    if cid in _RUNS:
        return _RUNS[cid]
    case = BY_ID[cid]
    pb, th = szr.build_case(case)
    assert th.shape[0] == 21
    ch = szr.oriented_chain(pb, th)
    assert {k: ch.layout[k] for k in case['layout']} == case['layout'], ch.layout
    r = dict(case=case, chain=ch)
    for name, kw in CONTEXTS:
        post = _post(pb, **kw)
        try:
            c = post.ctx.conv_layout
            assert c['form'] == 'exact' and c['nxt'] == case['layout']['nxt'] and c['ntile'] == case['layout']['nxt'] * case['layout']['ng'], c
            o = dict(logp=post.log_prob(th))
            o['launch'] = post.ctx.exact_info()['last_launch']
            o['logp17'], o['logp16'] = post.log_prob(th[:17]), post.log_prob(th[:16])
            o['row'] = post.stage(th, 'map_row')
            if name == 'reference kernels':
                o['bright'], o['pp'] = post.stage(th, 'bright'), post.stage(th, 'pp')
        finally:
            post.close()
        r[name] = o
    b = r['reference kernels']
    fin = np.isfinite(b['logp'])
    assert fin.sum() >= 15 and not fin[2] and not fin[4], fin
    assert np.isfinite(b['row'][fin]).all() and np.all(b['row'][fin] != 0.0) and np.isfinite(b['bright'][fin]).all() and np.isfinite(b['pp'][fin]).all()
    r['fin'] = fin
    pp, cf = b['pp'][fin], b['bright'][fin] / b['row'][fin]
    r['ref'] = ch.reference(pp, cf)
    r['ref32'] = szf.SzChainF32(chain=ch).reference(pp, cf)
    _RUNS[cid] = r
    return r


def _describe(case):
    lay = case['layout']
    return '%s NXT %d groups %d/%d nS %d pairs %d fold %d' % (case['id'], lay['nxt'], lay['ng_use'], lay['ng'], lay['nS'], lay['npair'], lay['nfold'])


@pytest.mark.parametrize('cid', IDS)
def test_f64_against_the_reference_kernels(cid):
    r = _run(cid)
    ref, fin, old = r['ref'], r['fin'], r['reference kernels']
    assert r['default']['launch'] == 'contracted' and r['partial rows']['launch'] == 'partial rows' and old['launch'] == 'partial rows', r['default']['launch']
    out = {}
    for name in ('default', 'partial rows'):
        o = r[name]
        assert np.array_equal(np.isfinite(o['logp']), fin) and o['logp'][2] == -np.inf and o['logp'][4] == -np.inf, o['logp']
        assert old['logp'][2] == -np.inf and old['logp'][4] == -np.inf
        assert o['row'].shape == old['row'].shape == (21, r['chain'].nrow)
        q_ref = szr.ratio(o['row'][fin], ref['row'], ref['row_bound'])
        q_old = szr.ratio(o['row'][fin], old['row'][fin].astype(szr.LD), 2.0 * ref['row_bound'])
        q_lp = szr.ratio(o['logp'][fin], old['logp'][fin].astype(szr.LD), ref['chi_bound'] + szr.U * (np.abs(o['logp'][fin]) + np.abs(old['logp'][fin])))
        out[name] = (q_ref, q_old, q_lp)
    q0 = szr.ratio(old['row'][fin], ref['row'], ref['row_bound'])
    print('%s | reference kernels: row %.3f of row_bound | row of row_bound, row - reference kernels\' of 2 row_bound, logp - theirs of chi_bound + u (|logp| + |logp\'|): %s'
          % (_describe(r['case']), q0, '  '.join('%s %.3f %.3f %.3f' % (k, *v) for k, v in out.items())))
    assert q0 <= 1.0, q0
    for name, v in out.items():
        assert max(v) <= 1.0, (name, v)


@pytest.mark.parametrize('cid', IDS)
def test_f32x_against_its_bound(cid):
    r = _run(cid)
    ref, fin, old, o = r['ref32'], r['fin'], r['reference kernels'], r['f32x']
    assert o['launch'] == 'contracted', o['launch']
    assert np.array_equal(np.isfinite(o['logp']), fin) and o['logp'][2] == -np.inf and o['logp'][4] == -np.inf, o['logp']
    q_row = szr.ratio(o['row'][fin], ref['row'], ref['row_bound'])
    # (its chi^2 within the fp32 chi_bound of the long-double chi^2, the reference kernels' within the f64 one: the log-likelihoods within half their sum)
    bar = (ref['chi_bound'] + r['ref']['chi_bound']) / 2 + szr.U * (np.abs(o['logp'][fin]) + np.abs(old['logp'][fin]))
    q_lp = szr.ratio(o['logp'][fin], old['logp'][fin].astype(szr.LD), bar)
    print('%s | f32x: row %.3f of the fp32 row_bound, logp - f64 reference kernels\' %.3f of (chi_bound32 + chi_bound) / 2 + u (|logp| + |logp\'|)' % (_describe(r['case']), q_row, q_lp))
    assert q_row <= 1.0 and q_lp <= 1.0, (q_row, q_lp)


@pytest.mark.parametrize('cid', IDS)
def test_launches_of_16_17_and_21_walkers(cid):
    r = _run(cid)
    for name, _ in CONTEXTS[1:]:
        o = r[name]
        np.testing.assert_array_equal(o['logp17'], o['logp'][:17], err_msg='%s: launch of 17' % name)
        np.testing.assert_array_equal(o['logp16'], o['logp'][:16], err_msg='%s: launch of 16' % name)
