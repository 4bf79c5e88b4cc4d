"""The bound of the exact form with fp32 products (tests/sz_chain_f32.py) on the CPU, at every case of sz_chain_reference.CASES: the numpy
float32 evaluation of the chain under the contract of dtype='f32x' -- rounded operands, fp32 accumulation chain by chain as jx_ordrow32_kernel
groups it, fp64 from a pair's share of the row on -- stays below the bound on the row, the model and chi^2, in the plain pairing and (where
the case folds its last ordinate tile) in the folded one; and each of five faults -- the last profile point, the last and the first macro
step of 16 radii, the first output, the last data radius -- leaves the bound on the row or on the model, so that the GPU test that holds the
kernels to it (test_gpu_exact_f32.py) has teeth.  (Not the last output in use: its weight is 1e-22 by construction, no bound can see it.)

At every case every one of the five faults is visible: there is no excused pair."""
import numpy as np
import pytest

from oracle import joxsz_oracle as orc

import sz_chain_reference as szr
import sz_chain_f32 as f32

FAULTS = ('profile point', 'macro step', 'first macro step', 'first output', 'data radius')


@pytest.fixture(scope='module')
def lib():
    return szr.load_host_tables()


def _oracle_inputs(pb, th, count=4):
    """pp, cf = bright / map_row of the first `count` walkers the oracle accepts."""
    fin = np.isfinite(orc.log_posterior_batch(pb, th))
    st = [orc.sz_stages(pb, orc.pars_dict(pb, t)) for t in th[fin][:count]]
    return np.array([s['pp'] for s in st]), np.array([s['bright'] / s['map_row'] for s in st])


@pytest.mark.parametrize('case', szr.CASES, ids=lambda c: c['id'])
def test_f32_is_inside_the_bound_and_a_dropped_term_is_outside(lib, case):
    pb, th = szr.build_case(case)
    ch = f32.SzChainF32(chain=szr.oriented_chain(pb, th, lib))
    assert {k: ch.layout[k] for k in case['layout']} == case['layout'], ch.layout
    pp, cf = _oracle_inputs(pb, th)
    ref = ch.reference(pp, cf)
    line = '%s: n32 = %d (cap %d), n = %d' % (case['id'], ch.n32, ch.N + ch.layout['Nkp'] + 16 * ch.layout['nfold'] + 32, ch.n_terms)
    clean = {}
    for folded in ((False, True) if ch.layout['nfold'] else (False,)):
        row, m, chi, _ = ch.f32(pp, cf, folded=folded)
        clean[folded] = (szr.ratio(row, ref['row'], ref['row_bound']), szr.ratio(m, ref['m'], ref['m_bound']), szr.ratio(chi, ref['chi2'], ref['chi_bound']))
        line += ' | %s row %.3f  m %.3f  chi^2 %.3f of the bound' % ('folded' if folded else 'plain', *clean[folded])
    faults = {}
    for drop in FAULTS:
        row, m, _, _ = ch.f32(pp, cf, folded=bool(ch.layout['nfold']), drop=drop)
        faults[drop] = (szr.ratio(row, ref['row'], ref['row_bound']), szr.ratio(m, ref['m'], ref['m_bound']))
        line += ' | without the %s: row %.1e  m %.1e' % (drop, *faults[drop])
    print(line)
    for folded, got in clean.items():
        assert max(got) <= 1.0, (folded, got)
    for drop, (rr, rm) in faults.items():
        assert max(rr, rm) > 1.0, (case['id'], drop, rr, rm)
