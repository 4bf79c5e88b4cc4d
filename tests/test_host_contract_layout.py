"""The data-radii matrix as an operand of the contracted epilogue (jxt::contract_operand_layout, csrc/jx_tables.hpp) and the two chained
matrix-core products of jx_ordrow_kernel<NXT, true> (csrc/jx_exact.hpp), emulated in numpy with the instruction's index maps
    A lane l = A[l & 15][k = l >> 4],   B lane l = B[k = l >> 4][l & 15],   D register g of lane l = D[(l >> 4) + 4 g][l & 15].
The row product is formed transposed, mfma(Op, y): register r of lane (lk, li) is the share of walker li at output 16 tile + lk + 4 r, and
-- times its conversion factor, selected to 0 beyond the outputs in use -- the B operand of sub-step r of the product with the table.
CPU only: the host-only build libjx_tables_host.so."""
import ctypes
import os

import numpy as np
import pytest

LIB = os.path.join(os.path.dirname(__file__), '..', 'joxsz_amd', 'csrc', 'libjx_tables_host.so')
DP = ctypes.POINTER(ctypes.c_double)
LI, LK = np.arange(64) & 15, np.arange(64) >> 4


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build_host_tables()
    return ctypes.CDLL(LIB)


def _p(a):
    return a.ctypes.data_as(DP)


def _eop(lib, E, nuse, NXT, ng):
    nflux, ld = E.shape
    ndt = (nflux + 15) // 16
    out = np.full((ng, NXT, ndt, 64, 4), np.nan)
    assert lib.jxt_contract_operand_layout(_p(E), nflux, ld, nuse, NXT, ng, _p(out)) == 0
    return out


def _mfma(a, b, c):
    """One v_mfma_f64_16x16x4: a, b [64] lane values, c [64][4] accumulator registers; products added in the order of k."""
    A, B, D = np.zeros((16, 4)), np.zeros((4, 16)), np.zeros((16, 16))
    A[LI, LK] = a
    B[LK, LI] = b
    for g in range(4):
        D[LK + 4 * g, LI] = c[:, g]
    for k in range(4):
        D = D + np.outer(A[:, k], B[k, :])
    return np.stack([D[LK + 4 * g, LI] for g in range(4)], axis=1)


CASES = [(nflux, NXT, ng, nuse) for nflux in (5, 16, 17, 19, 32) for (NXT, ng, nuse) in ((6, 1, 91), (3, 3, 131), (6, 3, 275))]


@pytest.mark.parametrize('nflux,NXT,ng,nuse', CASES)
def test_operand_layout_unpacks_to_the_matrix(lib, nflux, NXT, ng, nuse):
    """Unpacked by the lane / register map, the table is E on [nflux x nuse] and exactly zero elsewhere."""
    assert nuse % 16 and 16 * NXT * (ng - 1) < nuse <= 16 * NXT * ng
    rng = np.random.default_rng(nflux * 1000 + nuse)
    nrow = nuse + 7
    E = np.ascontiguousarray(rng.normal(size=(nflux, nrow)))
    E[E == 0.0] = 1.0
    eop = _eop(lib, E, nuse, NXT, ng)
    ndt = (nflux + 15) // 16
    full = np.full((16 * ndt, 16 * NXT * ng), np.nan)
    for g in range(ng):
        for t in range(NXT):
            for dt in range(ndt):
                for r in range(4):
                    full[16 * dt + LI, 16 * (g * NXT + t) + LK + 4 * r] = eop[g, t, dt, :, r]
    assert not np.isnan(full).any()
    assert np.array_equal(full[:nflux, :nuse], E[:, :nuse])
    assert np.all(full[nflux:, :] == 0.0) and np.all(full[:, nuse:] == 0.0)


@pytest.mark.parametrize('nflux,NXT,ng,nuse', CASES)
def test_chained_products_reproduce_the_contraction(lib, nflux, NXT, ng, nuse):
    """share^T = Wy y^T on the matrix cores (transposed form), then E (cfac . share) straight from its accumulator registers, the wave's
    tiles and the groups in ascending order, the four waves in wave order: E (cfac . share) within 1e-15 of its largest value (reference in
    long double on the emulated share), with NaN conversion factors beyond the outputs in use, which must not reach any sum.  "1e-15
    relative" is read in the max norm, error over the largest value of the result: an element of a sum of up to 275 signed terms can cancel to
    far below its terms, and no fp64 sum keeps 1e-15 of such an element.  Element by element the test holds every value to the rounding
    bound of its own sum instead, n eps sum |E| |cfac . share|."""
    rng = np.random.default_rng(nflux * 77 + nuse)
    nrow = nuse + 7
    NX = 16 * NXT * ng
    E = np.ascontiguousarray(rng.normal(size=(nflux, nrow)))
    eop = _eop(lib, E, nuse, NXT, ng)
    ndt = (nflux + 15) // 16
    y = rng.normal(size=(16, 16))                                   # [walker][ordinate]: one macro step of 16 ordinates
    Wy = np.zeros((NX, 16))
    Wy[:min(NX, nrow)] = rng.normal(size=(min(NX, nrow), 16))       # [output][ordinate]
    cfac = np.full((16, max(NX, nrow)), np.nan)
    cfac[:, :nuse] = rng.uniform(0.5, 1.5, size=(16, nuse))
    share = np.zeros((16, NX))
    waves = np.zeros((4, ndt, 64, 4))
    for g in range(ng):
        for t in range(NXT):
            wv, X0 = t % 4, 16 * (g * NXT + t)
            cs = np.zeros((64, 4))
            for e in range(4):                                      # mfma(Op, y, c): A = Wy[x = li][k], B = y[w = li][k], k = 4 lk + e
                cs = _mfma(Wy[X0 + LI, 4 * LK + e], y[LI, 4 * LK + e], cs)
            for r in range(4):
                share[LI, X0 + LK + 4 * r] = cs[:, r]
            bv = np.zeros((64, 4))
            for r in range(4):
                X = X0 + LK + 4 * r
                with np.errstate(invalid='ignore'):
                    bv[:, r] = np.where(X < nuse, cs[:, r] * cfac[LI, X], 0.0)
            for dt in range(ndt):
                for r in range(4):
                    waves[wv, dt] = _mfma(eop[g, t, dt, :, r], bv[:, r], waves[wv, dt])
    np.testing.assert_allclose(share, y @ Wy.T, rtol=0, atol=1e-15 * np.abs(y @ Wy.T).max() * 4)
    m = np.zeros((16 * ndt, 16))                                    # m^T[d][w]
    for dt in range(ndt):
        for r in range(4):
            s = np.zeros(64)
            for wv in range(4):
                s = s + waves[wv, dt, :, r]
            m[16 * dt + LK + 4 * r, LI] = s
    assert np.isfinite(m).all()
    want = (E[:, :nuse].astype(np.longdouble) @ (cfac[:, :nuse] * share[:, :nuse]).astype(np.longdouble).T)
    err = np.abs(m[:nflux] - want).max() / np.abs(want).max()
    # element by element: a sum of n products in fp64 is within n eps of the sum of their magnitudes (n <= nuse terms, each product and each
    # addition rounded once; the emulation adds a wave's terms in order and then the four waves)
    mag = np.abs(E[:, :nuse]).astype(np.longdouble) @ np.abs(cfac[:, :nuse] * share[:, :nuse]).astype(np.longdouble).T
    per = (np.abs(m[:nflux] - want) / (np.finfo(np.float64).eps * mag)).max()
    print('nflux %d nuse %d groups %d: %.1e of the largest value, %.2f eps sum|terms| at the worst element' % (nflux, nuse, ng, err, per))
    assert err <= 1e-15
    assert per <= nuse + 4
    assert np.all(m[nflux:] == 0.0)
