"""The long-double reference of the SZ linear chain and its derived bound (tests/sz_chain_reference.py) on the CPU: numpy's fp64 evaluation
of the same chain sits well inside the bound, one dropped term lies far outside it -- so the GPU tests that hold the exact-form kernels
to the bound (test_gpu_exact_instances.py) have teeth -- and every case of those tests reaches the instance of the kernels it is meant for."""
import numpy as np
import pytest

from oracle import joxsz_oracle as orc

import sz_chain_reference as szr


@pytest.fixture(scope='module')
def lib():
    return szr.load_host_tables()


def _oracle_inputs(pb, th, count=4):
    """pp, cf = bright / map_row and chi^2 of the first `count` walkers the oracle accepts."""
    fin = np.isfinite(orc.log_posterior_batch(pb, th))
    st = [orc.sz_stages(pb, orc.pars_dict(pb, t)) for t in th[fin][:count]]
    return fin, np.array([s['pp'] for s in st]), np.array([s['bright'] / s['map_row'] for s in st]), np.array([s['chisq'] for s in st])


@pytest.mark.parametrize('case', [c for c in szr.CASES if c['id'] in ('129-150-19radii', '32-40-5radii')], ids=lambda c: c['id'])
def test_fp64_is_inside_the_bound_and_a_dropped_term_is_outside(lib, case):
    """129^2 / 150 and 32^2 / 40 with 5 data radii, pp and cf of four oracle walkers: the fp64 evaluation of the chain differs from the
    long-double reference by less than a tenth of row_bound, m_bound and chi_bound; without the last output in use, the last profile point,
    the last macro step of 16 radii or the last data radius the model at the data radii and chi^2 leave their bounds."""
    pb, th = szr.build_case(case)
    ch = szr.oriented_chain(pb, th, lib)
    _, pp, cf, chi_orc = _oracle_inputs(pb, th)
    ref = ch.reference(pp, cf)
    row, m, chi = ch.fp64(pp, cf)
    got = (szr.ratio(row, ref['row'], ref['row_bound']), szr.ratio(m, ref['m'], ref['m_bound']), szr.ratio(chi, ref['chi2'], ref['chi_bound']))
    line = '%s: n = %d, m_bound / |m| <= %.1e; fp64 row %.3f  m %.3f  chi^2 %.3f of the bound' % (
        case['id'], ch.n_terms, np.max(ref['m_bound'] / np.abs(ref['m'].astype(np.float64))), *got)
    faults = {}
    for drop in ('output', 'profile point', 'macro step', 'data radius'):
        _, md, cd = ch.fp64(pp, cf, drop=drop)
        faults[drop] = (szr.ratio(md, ref['m'], ref['m_bound']), szr.ratio(cd, ref['chi2'], ref['chi_bound']))
        line += ' | without the last %s: m %.1e  chi^2 %.1e' % (drop, *faults[drop])
    print(line)
    assert max(got) < 0.1, got
    for drop, (rm, rc) in faults.items():
        assert rm > 1.0 and rc > 1.0, (drop, rm, rc)
    # the oracle's chi^2 (FFT chain, scipy's splines) is the same quantity: far inside the 1e-9 bar it is held to elsewhere
    np.testing.assert_allclose(ref['chi2'].astype(np.float64), chi_orc, rtol=1e-9)


@pytest.mark.parametrize('case', szr.CASES, ids=lambda c: c['id'])
def test_every_case_reaches_its_instance(lib, case):
    """The layout the library's set-up picks for each case of test_gpu_exact_instances.py, restated from the host tables (outputs in use
    under JX_PRUNE_TOL, NXT, groups, ordinates, tiles, pairs, fold steps, data-radii tiles), equals the table; the oracle accepts 19 of the
    21 walkers and rejects the two that were placed outside the box and at NaN."""
    pb, th = szr.build_case(case)
    ch = szr.SzChain(pb, lib)
    assert {k: ch.layout[k] for k in case['layout']} == case['layout'], ch.layout
    assert pb.flux_data.shape[1] == case['nflux'] and 0 < ch.layout['nuse'] <= min(ch.nrow, 16 * ch.layout['nxt'] * ch.layout['ng_use'])
    fin = np.isfinite(orc.log_posterior_batch(pb, th))
    assert fin.sum() == szr.NWALKERS - 2 and not fin[2] and not fin[4]
