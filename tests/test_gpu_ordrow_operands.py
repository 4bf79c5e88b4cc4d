"""jx_ordrow_kernel requests the upper tile's ordinate operator only for the steps that multiply it, and no conversion factors for an
output tile a wave does not own (csrc/jx_exact.hpp).  Which requests a wave makes depends on its pair and on the problem's tiling, never
on the launch: the same walkers give the same bits in one launch of 130 (nine walker tiles), in launches of 16, 17 and 40, at the end of a
launch where they sat in other blocks, and in chunks of 16 (max_batch = 16) -- contracted form and partial rows, at the smallest shapes
with one ordinate tile (no upper tile at all), a fold, outputs ending inside a tile, and two groups of six tiles.  Needs an MI355X: run
with -m gpu."""
import numpy as np
import pytest

import sz_chain_reference as szr

pytestmark = pytest.mark.gpu

BY_ID = {c['id']: c for c in szr.CASES}
# 15^2 / 16 (one ordinate tile), 32^2 / 40 (a fold), 65^2 / 80 (33 outputs in use of 33), 129^2 / 150 (65 outputs), 144^2 / 170 (72 in use, a fold),
# 200^2 / 240 (two groups of six tiles)
SHAPES = ['15-16-5radii', '32-40-5radii', '65-80-19radii', '129-150-19radii', '144-170-19radii', '200-240-19radii']


def _post(pb, **kw):
    from joxsz_amd.posterior import JoxszPosterior
    return JoxszPosterior(pb, device=0, **kw)


@pytest.mark.parametrize('form', ['contracted', 'partial rows'])
@pytest.mark.parametrize('cid', SHAPES)
def test_same_bits_in_every_launch(cid, form):
    from joxsz_amd import datasets
    case = BY_ID[cid]
    pb, _ = szr.build_case(case)
    th = datasets.walker_ball(pb, 130, spread=0.03, seed=case['S'])
    th[2, 1] = 9.0                       # outside the prior box
    th[4, 0] = np.nan
    opt = {'X_CONTRACT': '0'} if form == 'partial rows' else None
    a, c16 = _post(pb, max_batch=256, options=opt), _post(pb, max_batch=16, options=opt)
    try:
        whole = a.log_prob(th)
        fin = np.isfinite(whole)
        print('%s %s: %d of %d finite, launch form %s' % (cid, form, fin.sum(), th.shape[0], a.ctx.exact_info()['last_launch']))
        assert fin.sum() >= th.shape[0] - 8 and not fin[2] and not fin[4] and np.all(whole[~fin] == -np.inf)
        for n in (16, 17, 21, 40):
            np.testing.assert_array_equal(a.log_prob(th[:n]), whole[:n], err_msg='launch of %d' % n)
        np.testing.assert_array_equal(a.log_prob(th[113:]), whole[113:], err_msg='the last 17 walkers alone')
        np.testing.assert_array_equal(c16.log_prob(th), whole, err_msg='chunks of 16')
    finally:
        a.close()
        c16.close()
