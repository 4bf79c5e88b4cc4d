"""The contracted form of the exact form's pair-wise kernels (csrc/jx_exact.hpp; JOXSZ_X_CONTRACT, default on): between a pair's share of
the extracted row and the model at the data radii every step is linear with constant or per-walker coefficients,
    m[w][d] = sum_x E[d][x] cfac[w][x] sum_pair P_pair[w][x] = sum_pair (sum_x E[d][x] cfac[w][x] P_pair[w][x]),
so a block of jx_ordrow_kernel applies the conversion factors and the data-radii matrix to its own share and hands nflux values per walker
to the tail instead of the share.  Held here to the partial rows of JOXSZ_X_CONTRACT=0 -- the form every call with a row or brightness tap
still takes -- with the bars test_folded_last_tile_against_the_plain_pairing uses for a regrouped sum, and to the library's invariant: a
walker's bits do not depend on the launch it travels in."""
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


def _against_partial_rows(pb, th, S, contracted=True, options=None):
    """Default context against JOXSZ_X_CONTRACT=0 on the same problem and walkers: which form ran (jx_get_exact_info, against the form the
    caller expects for this shape, so a silent fall-back cannot hide a broken kernel), the same rejection set, log-posterior within rtol
    1e-13 from side 128 up and 1e-10 below, and the chi^2 tap -- which, like the parts tap, asks for no row and no brightness and so runs
    the contracted launches in the default context -- within 1e-10 max(1, chi^2); the SZ log-likelihood of the parts tap (-chi^2 / 2 + a
    term both contexts share) within half of that."""
    opt = dict(options or {})
    a, b = _post(pb, options=opt), _post(pb, options=dict(opt, X_CONTRACT='0'))
    assert a.ctx.conv_layout['form'] == 'exact' and b.ctx.conv_layout['form'] == 'exact'
    ia, ib = a.ctx.exact_info(), b.ctx.exact_info()
    form = 'contracted' if contracted else 'partial rows'
    assert ia['contracted'] == contracted and not ib['contracted'] and ia['last_launch'] is None
    la, lb = a.log_prob(th), b.log_prob(th)
    assert a.ctx.exact_info()['last_launch'] == form and b.ctx.exact_info()['last_launch'] == 'partial rows'
    ca, cb = a.stage(th, 'chisq'), b.stage(th, 'chisq')
    assert a.ctx.exact_info()['last_launch'] == form and b.ctx.exact_info()['last_launch'] == 'partial rows'
    pa, pb_ = a.stage(th, 'parts'), b.stage(th, 'parts')
    assert a.ctx.exact_info()['last_launch'] == form
    ra = a.stage(th, 'map_row')                                        # (a call with the row tap: partial rows in either context)
    assert a.ctx.exact_info()['last_launch'] == 'partial rows' and np.array_equal(ra, b.stage(th, 'map_row'), equal_nan=True)
    assert np.array_equal(a.log_prob(th), la)                         # ... and the contracted form again behind it, the same bits
    a.close(); b.close()
    fin = np.isfinite(lb)
    assert fin.sum() >= th.shape[0] - 6 and not fin[2] and not fin[4] and np.array_equal(np.isfinite(la), fin)
    bar = 1e-10 * np.maximum(1.0, np.abs(cb[fin]))
    rel = np.max(np.abs(la[fin] - lb[fin]) / np.abs(lb[fin]))
    dchi = np.max(np.abs(ca[fin] - cb[fin]) / bar) * 1e-10
    print('S %d: logp rel %.1e  chi^2 tap %.1e of max(1, chi^2)  (chi^2 up to %.3g)  contracted %s, %d for %d doubles' %
          (S, rel, dchi, np.max(cb[fin]), ia['contracted'], ia['doubles_per_contracted_partial'], ia['doubles_per_partial_row']))
    np.testing.assert_allclose(la[fin], lb[fin], rtol=1e-13 if S >= 128 else 1e-10)
    assert np.all(np.isfinite(ca[fin])) and np.all(np.abs(ca[fin] - cb[fin]) <= bar)
    assert np.all(np.abs(pa[fin, 1] - pb_[fin, 1]) <= 0.5 * bar)
    return ia


@pytest.mark.parametrize('S,N,W,measured', [(31, 40, 21, False), (56, 70, 21, False), (64, 80, 21, False), (256, 300, 40, False),
                                            (171, 313, 33, True), (512, 500, 37, False)])
def test_contracted_form_against_partial_rows(S, N, W, measured):
    """3, 5 and 25 ordinate tiles with a fold (56^2: more macro steps than pairs), an even tile count (256^2), the measured beam and
    transfer function, the headline shape; ragged walker counts, a walker outside the box and a NaN parameter in each."""
    from joxsz_amd import datasets
    if measured:
        from test_gpu_parity import _measured_problem
        pb = _measured_problem(S, N)
    else:
        pb = datasets.synthetic_problem(S=S, N=N, seed=S + 1)
    pb = _filled(pb, S)
    info = _against_partial_rows(pb, _walkers(pb, W, S), S, contracted=(S != 31))
    assert info['contracted'] == (S != 31)                           # (16 outputs at 31^2, 19 data radii: the partial rows are the smaller ones)


@pytest.fixture(scope='module')
def headline():
    """512^2 / 500 with data at the fiducial vector, 333 walkers, and their log-posterior from one default context (left unchanged)."""
    from joxsz_amd import datasets
    pb = _filled(datasets.synthetic_problem(S=512, N=500, seed=3), 3)
    th = _walkers(pb, 333, 3)
    post = _post(pb)
    assert post.ctx.exact_info()['contracted']
    full = post.log_prob(th)
    info = post.ctx.exact_info()
    post.close()
    assert info['last_launch'] == 'contracted' and info['doubles_per_contracted_partial'] == 19 and info['doubles_per_partial_row'] == 96
    full.setflags(write=False)
    return pb, th, full


def test_bits_do_not_depend_on_the_launch(headline):
    """Walker counts 1, 15, 17 and 333; contexts with max_batch 16 and 100; evaluated twice; permuted: the same bits walker by walker."""
    pb, th, full = headline
    assert np.isfinite(full).sum() >= 320
    perm = np.random.default_rng(5).permutation(th.shape[0])
    for mb in (0, 16, 100):
        post = _post(pb, **({'max_batch': mb} if mb else {}))
        for n in (1, 15, 17, 333):
            np.testing.assert_array_equal(post.log_prob(th[:n]), full[:n], err_msg='max_batch=%d n=%d' % (mb, n))
        np.testing.assert_array_equal(post.log_prob(th), full, err_msg='max_batch=%d, second evaluation' % mb)
        np.testing.assert_array_equal(post.log_prob(th[perm]), full[perm], err_msg='max_batch=%d, permuted' % mb)
        assert post.ctx.exact_info()['last_launch'] == 'contracted'
        post.close()


def test_host_pointers_against_device_resident(headline):
    """jx_eval (host pointers) and jx_eval_device take the same form: the difference is exactly 0."""
    pb, th, full = headline
    post = _post(pb)
    c = post.ctx
    W = th.shape[0]
    dth, dlp = c.dev_alloc(th.nbytes), c.dev_alloc(8 * W)
    c.h2d(dth, th)
    c.eval_device(dth, W, dlp)
    c.sync()
    got = np.empty(W)
    c.d2h(got, dlp)
    c.dev_free(dth); c.dev_free(dlp)
    assert c.exact_info()['last_launch'] == 'contracted'
    post.close()
    np.testing.assert_array_equal(got, full)


def test_device_sampler_against_host_replay(headline):
    """A 20-step jx_sample run (acceptance inside the contracted tail) against the stretch move replayed on the host with the same Philox
    counters and the device's own log-posterior.  The acceptances are compared exactly: that pins the tail's acceptance arithmetic.  The chain
    and the log-posteriors are held to the bars test_gpu_parity.py holds its replay to; whether the replay is bitwise has not been measured."""
    from joxsz_amd import datasets
    from joxsz_amd.sampler import DeviceStretchMove, initial_ball
    pb, _, _ = headline
    post = _post(pb)
    p0 = initial_ball(post.log_prob, datasets.fiducial_theta(pb), 28, spread=0.01, rng=np.random.default_rng(3))
    sm = DeviceStretchMove(post, a=2.0, seed=1234)
    chain, lps, nacc = sm.run(p0, 20)
    assert post.ctx.exact_info()['last_launch'] == 'contracted'
    rchain, rlps, rnacc = sm.replay(p0, 20)
    post.close()
    assert chain.shape == (20, 28, pb.ndim) and np.isfinite(lps).all() and 0 < nacc.sum() < 20 * 28
    np.testing.assert_array_equal(nacc, rnacc)
    np.testing.assert_allclose(chain, rchain, rtol=1e-13, atol=0)
    np.testing.assert_allclose(lps, rlps, rtol=1e-12)


def test_three_output_groups(headline):
    """JOXSZ_PRUNE_OUTPUTS=0 at 512^2 / 500: every output of the row in three groups of 96, a converted share that reaches beyond the
    reduction area in LDS, the data-radii matrix through the caches."""
    pb, th, _ = headline
    info = _against_partial_rows(pb, th[:37], 512, options={'PRUNE_OUTPUTS': '0'})
    assert info['doubles_per_partial_row'] == 288 and not info['data_radii_matrix_in_lds']


@pytest.mark.parametrize('nflux', [5, 23])
def test_other_numbers_of_data_radii(nflux):
    """The flux table cut to 5 data radii, and refined to 23 (more than 20: more than five data radii per lane of the product)."""
    from joxsz_amd import datasets
    pb = datasets.synthetic_problem(S=128, N=150, seed=7)
    fd = pb.flux_data
    r = fd[0, :5] if nflux == 5 else np.linspace(fd[0, 0], fd[0, -1], nflux)
    pb.flux_data = np.ascontiguousarray(np.vstack((r, np.interp(r, fd[0], fd[1]), np.interp(r, fd[0], fd[2]))))
    pb = _filled(pb.validate(), 7)
    info = _against_partial_rows(pb, _walkers(pb, 21, 7), 128)
    assert info['doubles_per_contracted_partial'] == nflux


def test_large_map_reports_the_form_that_ran():
    """1024^2 / 1000 with 20 walkers: jx_get_conv_layout and jx_get_exact_info say what the launch exchanges, and the launch agrees."""
    from joxsz_amd import datasets
    pb = _filled(datasets.synthetic_problem(S=1024, N=1000, seed=11), 11)
    th = _walkers(pb, 20, 11)
    post = _post(pb)
    lay, info = post.ctx.conv_layout, post.ctx.exact_info()
    post.close()
    assert lay['form'] == 'exact' and info['doubles_per_partial_row'] == lay['ldx']
    print('1024^2 / 1000: %s  %s' % (lay, info))
    assert info['contracted'], (lay, info)
    _against_partial_rows(pb, th, 1024)
