"""The contracted epilogue of jx_ordrow_kernel on the matrix cores (csrc/jx_exact.hpp): the row product formed transposed, its accumulator
registers -- times the conversion factors -- the B operand of the product with the data-radii matrix in operand order
(jxt::contract_operand_layout), the waves' sums added in wave order.  Held to the partial rows of JOXSZ_X_CONTRACT=0 with the bars of
test_gpu_contract.py (log-posterior rtol 1e-13 from side 128 up, 1e-10 below; chi^2 within 1e-10 max(1, chi^2)) at the edges of the
data-radii tiles, and to the rule that a walker lives in one column of every operand: a NaN or rejected walker changes no other bit."""
import numpy as np
import pytest

from oracle import joxsz_oracle as orc

pytestmark = pytest.mark.gpu


def _post(pb, **kw):
    from joxsz_amd.posterior import JoxszPosterior
    return JoxszPosterior(pb, device=0, **kw)


def _filled(pb, seed):
    from joxsz_amd import datasets
    p0 = orc.pars_dict(pb, datasets.fiducial_theta(pb))
    datasets.fill_data(pb, orc.sz_stages(pb, p0)['bright'], None if pb.sz_only else orc.calc_profiles(pb, p0), seed=seed)
    return pb


def _walkers(pb, W, seed):
    """A ball of walkers with one outside the prior box and one NaN parameter."""
    from joxsz_amd import datasets
    th = datasets.walker_ball(pb, W, spread=0.03, seed=seed)
    th[2, 1] = 9.0
    th[4, 0] = np.nan
    return th


def _with_data_radii(pb, nflux):
    """The flux table cut to its first nflux data radii, or refined to nflux radii over the same range."""
    fd = pb.flux_data
    r = fd[0, :nflux] if nflux <= fd.shape[1] else np.linspace(fd[0, 0], fd[0, -1], nflux)
    pb.flux_data = np.ascontiguousarray(np.vstack((r, np.interp(r, fd[0], fd[1]), np.interp(r, fd[0], fd[2]))))
    return pb.validate()


def _against_partial_rows(pb, th, S, contracted=True):
    """Default context against JOXSZ_X_CONTRACT=0: the form that ran, the same rejection set, and test_gpu_contract.py's bars."""
    a, b = _post(pb), _post(pb, options={'X_CONTRACT': '0'})
    ia = a.ctx.exact_info()
    assert ia['contracted'] == contracted and not b.ctx.exact_info()['contracted']
    assert not ia['data_radii_matrix_in_lds']
    la, lb = a.log_prob(th), b.log_prob(th)
    form = 'contracted' if contracted else 'partial rows'
    assert a.ctx.exact_info()['last_launch'] == form and b.ctx.exact_info()['last_launch'] == 'partial rows'
    ca, cb = a.stage(th, 'chisq'), b.stage(th, 'chisq')
    assert a.ctx.exact_info()['last_launch'] == form
    a.close(); b.close()
    fin = np.isfinite(lb)
    assert fin.sum() >= th.shape[0] - 6 and not fin[2] and not fin[4] and np.array_equal(np.isfinite(la), fin)
    bar = 1e-10 * np.maximum(1.0, np.abs(cb[fin]))
    print('S %d, %d data radii for %d outputs (%s): logp rel %.1e  chi^2 %.1e of max(1, chi^2)' %
          (S, ia['doubles_per_contracted_partial'], ia['doubles_per_partial_row'], form,
           np.max(np.abs(la[fin] - lb[fin]) / np.abs(lb[fin])), np.max(np.abs(ca[fin] - cb[fin]) / bar) * 1e-10))
    if contracted:
        np.testing.assert_allclose(la[fin], lb[fin], rtol=1e-13 if S >= 128 else 1e-10)
        assert np.all(np.isfinite(ca[fin])) and np.all(np.abs(ca[fin] - cb[fin]) <= bar)
    else:
        assert np.array_equal(la, lb) and np.array_equal(ca, cb, equal_nan=True)
    return ia


def test_fold_with_more_macro_steps_than_pairs():
    """56^2 / 70, 21 walkers: five ordinate tiles, the folded tile's macro steps outnumber the pairs (the a2 loop of the transposed product)."""
    from joxsz_amd import datasets
    pb = _filled(datasets.synthetic_problem(S=56, N=70, seed=57), 56)
    _against_partial_rows(pb, _walkers(pb, 21, 56), 56)


@pytest.mark.parametrize('nflux', [5, 16, 17, 32])
def test_data_radii_tile_edges(nflux):
    """128^2 / 150, 21 walkers, the flux table cut to 5 data radii or refined to 16, 17 and 32: one partly filled tile, one full tile, one
    full and one with a single row, two full tiles.  128^2 extracts 64 outputs, more than the 32 data radii of the last case (asserted)."""
    from joxsz_amd import datasets
    pb = _filled(_with_data_radii(datasets.synthetic_problem(S=128, N=150, seed=7), nflux), 7)
    info = _against_partial_rows(pb, _walkers(pb, 21, 7), 128)
    assert info['doubles_per_contracted_partial'] == nflux < info['doubles_per_partial_row']


def test_more_data_radii_than_the_tiles_hold():
    """33 data radii at 128^2 / 150: more than the two instantiated tiles of 16 hold.  jx_get_exact_info says partial rows, the launch takes
    them, and the results equal the JOXSZ_X_CONTRACT=0 context's."""
    from joxsz_amd import datasets
    pb = _filled(_with_data_radii(datasets.synthetic_problem(S=128, N=150, seed=7), 33), 7)
    info = _against_partial_rows(pb, _walkers(pb, 21, 7), 128, contracted=False)
    assert info['doubles_per_partial_row'] > 33


@pytest.fixture(scope='module')
def side128():
    from joxsz_amd import datasets
    return _filled(datasets.synthetic_problem(S=128, N=150, seed=7), 7)


def test_no_value_crosses_between_walkers(side128):
    """A ragged tile: 17 walkers of which one has a NaN parameter, one lies outside the box and one fails the mass veto (found in a wide
    ball by its rejection flags).  The other 14 get the same bits as when they are evaluated without the three."""
    from joxsz_amd import datasets
    pb = side128
    post = _post(pb)
    assert post.ctx.exact_info()['contracted']
    wide = datasets.walker_ball(pb, 300, spread=0.08, seed=11)
    flags = post.stage(wide, 'parts')[:, 3].astype(int)
    veto = np.flatnonzero(flags == 2)
    assert veto.size, np.bincount(flags)
    th = datasets.walker_ball(pb, 17, spread=0.03, seed=19)
    bad = [3, 9, 16]
    th[3, 0] = np.nan
    th[9, 1] = 9.0
    th[16] = wide[veto[0]]
    good = np.setdiff1d(np.arange(17), bad)
    lp = post.log_prob(th)
    assert post.ctx.exact_info()['last_launch'] == 'contracted'
    alone = post.log_prob(th[good])
    post.close()
    assert np.all(lp[bad] == -np.inf) and np.isfinite(lp[good]).all()
    np.testing.assert_array_equal(lp[good], alone)


def test_conversion_factors_up_to_the_outputs_in_use(side128):
    """The timed per-walker kernel writes the conversion factors of the outputs its launch reads and no more.  The brightness tap still
    returns every output -- before and after a contracted launch on the same context -- and a contracted launch followed by a
    JOXSZ_X_CONTRACT=0 launch on another context agrees to the bars."""
    pb = side128
    th = _walkers(pb, 21, 23)
    a, b = _post(pb), _post(pb, options={'X_CONTRACT': '0'})
    nrow = pb.S - pb.S // 2
    b0 = a.stage(th, 'bright')
    la = a.log_prob(th)
    assert a.ctx.exact_info()['last_launch'] == 'contracted'
    b1 = a.stage(th, 'bright')
    lb = b.log_prob(th)
    bb = b.stage(th, 'bright')
    a.close(); b.close()
    fin = np.isfinite(lb)
    assert fin.sum() >= 15 and np.array_equal(np.isfinite(la), fin)
    assert b0.shape == (21, nrow) and np.isfinite(b0[fin]).all() and np.all(b0[fin] != 0.0)
    assert np.array_equal(b0[fin], b1[fin]) and np.array_equal(b0[fin], bb[fin])
    np.testing.assert_allclose(la[fin], lb[fin], rtol=1e-13)
