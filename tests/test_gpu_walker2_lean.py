"""The two lean roles of jx_walker2_kernel against the one-block form of jx_prep_kernel, bit for bit.

The X-ray role runs a function of its own (one code path per wave in the shell phase, log T_X and its interval of the temperature grid once per
annulus, the logarithms of the X-ray radii from the context's pack) and the SZ-side role holds its radii in registers and makes one reduction
round of the prior sum, the h(0) sum and the rejection bits.  None of this may move a bit: every case compares the default context with a
context under JOXSZ_PREP_LEAN=0 (the two-block form inside jx_prep_kernel) and one under JOXSZ_PREP_SPLIT=0 (the one-block form, the
reference), each form on a context of its own.  Needs an MI355X: run with -m gpu."""
import numpy as np
import pytest

from oracle import joxsz_oracle as orc

pytestmark = pytest.mark.gpu

MODES = (('one block', {'JOXSZ_PREP_SPLIT': '0'}), ('two blocks in jx_prep_kernel', {'JOXSZ_PREP_LEAN': '0'}), ('two lean roles', {}))
I_LOGTR = 5          # log(T_X/T_SZ) in the thawed vector (slot 7 of the parameter table)

# the smallest shapes that reach each branch of the lean roles (S, N, nann, nband, density model)
SMALL = {
    # grid pass with no second radius per lane; 150 (band, annulus) entries: two trips of the rate and projection phases
    '64/100': dict(S=64, N=100, nann=15, nband=10),
    # N equal to the thread count; 120 entries, one trip
    '64/128': dict(S=64, N=128, nann=15, nband=8),
    # the clamped second index with one radius over; nann at the edge of the one-path-per-wave mapping; exactly 128 entries
    '96/129': dict(S=96, N=129, nann=32, nband=4),
    # second trip of the grid pass with one radius; 320 entries, three trips
    '128/257': dict(S=128, N=257, nann=32, nband=10),
    # nann beyond the one-path-per-wave mapping
    '128/150 nann 40': dict(S=128, N=150, nann=40, nband=3),
    # the second density model
    '128/150 double': dict(S=128, N=150, nann=15, nband=10, ne_mode='double'),
    # The X-ray role's LDS grows with nann^2 and the three shapes above with nann >= 32 exceed what jx_walker2_kernel is launched with: they
    # run the two-block form of jx_prep_kernel in the default context.  These two are the same edges at sizes the lean kernel does run:
    # nann = 32, the last with one path per wave, and nann = 33, the first with jx_xray_side's lane groups inside the lean function.
    '96/129 nann 32 x 3': dict(S=96, N=129, nann=32, nband=3),
    '96/129 nann 33 x 3': dict(S=96, N=129, nann=33, nband=3),
}


def _run(monkeypatch, pb, th, **kw):
    from joxsz_amd.posterior import JoxszPosterior
    res = {}
    for name, env in MODES:
        for k in ('JOXSZ_PREP_SPLIT', 'JOXSZ_PREP_LEAN'):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        post = JoxszPosterior(pb, device=0, **kw)
        res[name] = post.log_prob(th)
        post.close()
    return res


def _check(res, pb, th):
    ref = res['one block']
    fin = np.isfinite(ref)
    print('finite %d of %d' % (fin.sum(), ref.size))
    # the inputs have teeth: at least a quarter of the walkers finite, at least one rejected (on the reference form's output)
    assert 4 * fin.sum() >= ref.size and fin.sum() < ref.size
    assert np.all(ref[~fin] == -np.inf)
    for name, got in res.items():
        np.testing.assert_array_equal(got, ref, err_msg=name)
    want = orc.log_posterior_batch(pb, th[:12])
    ok = np.isfinite(want)
    assert np.array_equal(np.isfinite(ref[:12]), ok)
    np.testing.assert_allclose(ref[:12][ok], want[ok], rtol=1e-9)


def _problem(seed=13, move_T_radii=False, **shape):
    from joxsz_amd import datasets
    pb = datasets.synthetic_problem(seed=seed, **shape)
    if move_T_radii:
        pb.x_r_T_kpc[1::2] *= 1.07        # lanes with equal and with unequal radii side by side: the second density job runs on some of them
    p0 = orc.pars_dict(pb, datasets.fiducial_theta(pb))
    datasets.fill_data(pb, orc.sz_stages(pb, p0)['bright'], orc.calc_profiles(pb, p0), seed=seed)
    return pb


@pytest.mark.parametrize('move_T_radii', [False, True], ids=['radii equal', 'T radii moved'])
@pytest.mark.parametrize('case', list(SMALL))
def test_lean_roles_same_bits_as_one_block(case, move_T_radii, monkeypatch):
    """300 walkers (one with a NaN parameter) in three chunks, the last ragged: the same bits from all three forms, rejected walkers included."""
    from joxsz_amd import datasets
    pb = _problem(move_T_radii=move_T_radii, **SMALL[case])
    th = datasets.walker_ball(pb, 300, spread=0.08, seed=13)
    th[7, 2] = np.nan
    _check(_run(monkeypatch, pb, th, max_batch=128), pb, th)


@pytest.mark.parametrize('logtr', [1.6, -3.0], ids=['above the grid', 'below the grid'])
def test_lean_roles_at_the_clamps_of_the_temperature_grid(logtr, monkeypatch):
    """log(T_X/T_SZ) at +1.6 puts every annulus beyond the upper end of the count-rate tables' temperature grid, at -3.0 below its lower end
    (the box of that parameter widened from +-1 to +-4): the end values of the tables, by the case codes of the lean X-ray role."""
    from joxsz_amd import datasets
    pb = _problem(**SMALL['64/100'])
    pb.par_min[7], pb.par_max[7] = -4.0, 4.0
    th0 = datasets.fiducial_theta(pb)
    th0[I_LOGTR] = logtr
    th = datasets.walker_ball(pb, 64, spread=0.05, seed=13, theta0=th0)
    th[7, 2] = np.nan
    _check(_run(monkeypatch, pb, th, max_batch=128), pb, th)


def test_lean_roles_headline_shape(monkeypatch):
    """512^2 / 500 radii: two trips of the grid pass per lane from registers, 150 (band, annulus) entries."""
    from joxsz_amd import datasets
    pb = datasets.synthetic_problem(S=512, N=500, seed=12)
    th = datasets.walker_ball(pb, 200, spread=0.05, seed=12)
    th[7, 2] = np.nan
    _check(_run(monkeypatch, pb, th), pb, th)
