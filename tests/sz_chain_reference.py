"""A long-double reference of the SZ linear chain with a derived forward error bound (no GPU; used by test_sz_chain_reference.py and
test_gpu_exact_instances.py).

The chain.  Between the pressure profile pp [N] of a walker and its chi^2 the exact form (csrc/jx_exact.hpp) evaluates

    y    = ys A pp                 ordinates, ys = kpc_cm sigma_T / m_e, A the forward Abel matrix (jxt::abel_matrix)
    row  = Wy y                    the extracted map row, Wy [nrow][N] (jxt::exact_row_operator)
    m    = E (cf . row)            the model at the data radii, cf the walker's conversion factors, E [nflux][nrow] (jxt::nak_eval_matrix)
    chi2 = sum_d ((f_d - m_d) / e_d)^2

with constant A, Wy, E from the host table library and per-walker pp, cf.  ``SzChain.reference`` evaluates the four lines in np.longdouble
(64-bit significand: its own error is 2^-11 of the bound below and is not accounted for).

The bound.  A sum of K products formed in fp64 in any order and grouping, fused or not, differs from the exact sum by at most
gamma_K sum |terms|, gamma_K = K u / (1 - K u), u = 2^-53 (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1; a fused
multiply-add, what the matrix cores issue, rounds once per term; a reduction tree rounds no more often per term than a chain).  Along
the chain every elementary term E[d][x] cf[x] Wy[x][k] ys A[k][j] pp[j] collects the factors (1 + delta), |delta| <= u, of

    N                    the ordinate's sum over the profile (any split over steps, chains and waves),
    Nkp                  the row's sum over the ordinates in use, padded to whole tiles of 16 (Nkp = 16 nS); a folded last tile is a sum
                         over the profile instead, of a host-built operator: no more terms than N,
    16 NXT ng_use        the sum over the outputs the launch computes (the data-radii matrix reads nuse <= 16 NXT ng_use of them),
    32                   everything else: the host's rounding of ys A and of the folded operator (2 + 1), the additions of the two chains of a
                         tile, the four or eight waves and the pairs where they are not already part of the sums above (2 + 7 + 7), the
                         conversion multiply (1), the division that recovers cf from the brightness and row taps (1), with room to spare,

so with n = N + Nkp + 16 NXT ng_use + 32 and gamma = n u / (1 - n u)

    |row - row_ref| <= row_bound = gamma row_abs,   row_abs = |Wy| |ys| |A| |pp|
    |m   - m_ref|   <= m_bound   = gamma m_abs,     m_abs   = |E| (|cf| . row_abs)

(the absolute-term sums in fp64: their own rounding is a relative 1e-13 of a bound).  With z_d = (f_d - m_d) / e_d and a model off by at
most m_bound_d, z_d^2 moves by at most 2 |z_d| m_bound_d / e_d + (m_bound_d / e_d)^2; the subtraction, the division, the square and the
sum of the terms add 8 u chi^2:

    |chi2 - chi2_ref| <= chi_bound = sum_d (2 |z_d| m_bound_d / e_d + (m_bound_d / e_d)^2) + 8 u chi2

This is a derivation, not a measurement: an evaluation that exceeds it has dropped or misplaced a term.  test_sz_chain_reference.py shows
both sides on the CPU -- numpy's fp64 evaluation of the same chain stays below a tenth of it, and one dropped output, profile point,
macro step of 16 radii or data radius exceeds it by orders of magnitude.

The layout.  ``SzChain.layout`` restates, from the same tables, which instance of the kernels the library picks for the problem
(plan_exact of csrc/jx_host_exact.hpp and data_radii_matrix of csrc/joxsz_hip.hip): the outputs in use under JX_PRUNE_TOL, NXT, the output groups, the ordinate tiles,
pairs and fold steps.  The GPU tests hold the live context to it."""
import ctypes
import os

import numpy as np

LIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'joxsz_amd', 'csrc', 'libjx_tables_host.so')
DP = ctypes.POINTER(ctypes.c_double)
LD = np.longdouble
U = 2.0 ** -53
PRUNE_TOL = 1e-22                      # JX_PRUNE_TOL of csrc/joxsz_hip.hip

assert np.finfo(LD).eps <= 2.0 ** -63, 'np.longdouble has no 64-bit significand on this platform: no precision reference'


def load_host_tables():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build_host_tables()
    return ctypes.CDLL(LIB)


def _p(a):
    return a.ctypes.data_as(DP)


def gamma(n):
    return n * U / (1.0 - n * U)


class SzChain:
    """The constant tables of the chain for one problem, its layout in the exact form, and the reference with its bounds."""

    def __init__(self, pb, lib=None):
        lib = lib or load_host_tables()
        S, N = pb.S, pb.N
        self.S, self.N, self.nrow = S, N, S - S // 2
        nrow = self.nrow
        self.ys = pb.kpc_cm * pb.sigma_T / pb.m_e
        r = np.ascontiguousarray(pb.r_pp, dtype=np.float64)
        A = np.zeros((N, N))
        assert lib.jxt_abel_matrix(_p(r), N, _p(A)) == 0
        self.A = A                     # y = ys A pp (upper triangular; see orient())
        Wy = np.zeros((nrow, N))
        nk = lib.jxt_exact_row_operator(_p(np.ascontiguousarray(pb.d_mat)), _p(np.ascontiguousarray(pb.beam_2d)), int(pb.beam_2d.shape[0]),
                                        ctypes.c_double(pb.step ** 2), _p(np.ascontiguousarray(pb.filtering)), S, _p(r), N, _p(Wy))
        assert nk > 0, nk
        self.Wy, self.Nk = Wy, int(nk)
        xk = np.ascontiguousarray(pb.radius[S // 2:], dtype=np.float64)
        self.set_data(pb.flux_data, lib, xk)
        # ---- the instance the library picks (plan_exact / data_radii_matrix)
        emax = np.abs(self.E).max()
        used = np.flatnonzero(np.abs(self.E).max(axis=0) > PRUNE_TOL * emax)
        nuse = max(1, int(used[-1]) + 1) if used.size else nrow
        tiles_use, tiles = (nuse + 15) // 16, (nrow + 15) // 16
        nxt = min(6, tiles_use)
        Nkp = (self.Nk + 15) & ~15
        nS, nSj = Nkp // 16, (N + 15) // 16
        nflux = self.E.shape[0]
        ng_use = (tiles_use + nxt - 1) // nxt
        self.layout = dict(nuse=nuse, nxt=nxt, ng_use=ng_use, ng=(tiles + nxt - 1) // nxt, Nk=self.Nk, Nkp=Nkp, nS=nS, nSj=nSj,
                           npair=(nS + 1) // 2, nfold=(nSj - (nS - 1)) if (nS & 1) and nS >= 3 else 0, ndt=(nflux + 15) // 16,
                           contracted=(nflux + 15) // 16 <= 2 and nflux < 16 * nxt * ng_use)
        self.n_terms = N + Nkp + 16 * nxt * ng_use + 32
        self.gamma = gamma(self.n_terms)

    def set_data(self, flux_data, lib=None, xk=None):
        """The data radii, values and errors (E depends on the radii alone)."""
        fd = np.ascontiguousarray(flux_data, dtype=np.float64)
        if lib is not None:
            q = np.ascontiguousarray(fd[0])
            E = np.zeros((q.size, self.nrow))
            assert lib.jxt_nak_eval_matrix(_p(xk), self.nrow, _p(q), q.size, _p(E)) == 0
            self.E = E
        assert fd.shape[1] == self.E.shape[0]
        self.f, self.e = fd[1].copy(), fd[2].copy()

    def orient(self, pp, y_want):
        """A or A.T, whichever reproduces a given evaluation of y = ys A pp (the oracle's); returns the relative distance."""
        d = [np.max(np.abs(self.ys * (M @ pp) - y_want)) / np.max(np.abs(y_want)) for M in (self.A, self.A.T)]
        if d[1] < d[0]:
            self.A = np.ascontiguousarray(self.A.T)
        return min(d)

    def reference(self, pp, cf, errors=None):
        """pp [W][N], cf [W][nrow] -> dict of row, row_bound [W][nrow]; m, m_bound [W][nflux]; chi2, chi_bound [W].
        errors: data errors in place of the problem's (same data radii and values)."""
        pp, cf = np.atleast_2d(np.asarray(pp, np.float64)), np.atleast_2d(np.asarray(cf, np.float64))
        e = self.e if errors is None else np.asarray(errors, np.float64)
        A, Wy, E = self.A.astype(LD), self.Wy.astype(LD), self.E.astype(LD)
        y = LD(self.ys) * (pp.astype(LD) @ A.T)
        row = y @ Wy.T
        m = (cf.astype(LD) * row) @ E.T
        z = (self.f.astype(LD) - m) / e.astype(LD)
        chi2 = np.sum(z * z, axis=1)
        row_abs = (abs(self.ys) * (np.abs(pp) @ np.abs(self.A).T)) @ np.abs(self.Wy).T
        m_abs = (np.abs(cf) * row_abs) @ np.abs(self.E).T
        row_bound, m_bound = self.gamma * row_abs, self.gamma * m_abs
        zb = m_bound / e
        chi_bound = np.sum(2.0 * np.abs(z.astype(np.float64)) * zb + zb * zb, axis=1) + 8.0 * U * chi2.astype(np.float64)
        return dict(row=row, row_bound=row_bound, m=m, m_bound=m_bound, chi2=chi2, chi_bound=chi_bound)

    def fp64(self, pp, cf, drop=None):
        """numpy's fp64 evaluation of the same chain -> (row, m, chi2).  drop: one of the faults the bound has to catch --
        'output' (the last output in use), 'profile point' (the last radius), 'macro step' (the last 16 radii), 'data radius' (the last)."""
        pp, cf = np.atleast_2d(np.asarray(pp, np.float64)).copy(), np.atleast_2d(np.asarray(cf, np.float64))
        if drop == 'profile point':
            pp[:, -1] = 0.0
        if drop == 'macro step':
            pp[:, 16 * (self.layout['nSj'] - 1):] = 0.0
        row = (self.ys * (pp @ self.A.T)) @ self.Wy.T
        b = cf * row
        if drop == 'output':
            b[:, self.layout['nuse'] - 1] = 0.0
        m = b @ self.E.T
        if drop == 'data radius':
            m[:, -1] = 0.0
        z = (self.f - m) / self.e
        return row, m, np.sum(z * z, axis=1)


def ratio(got, ref, bound):
    """max |got - ref| / bound in long double; entries with a zero bound must agree exactly."""
    d = np.abs(np.asarray(got).astype(LD) - ref).astype(np.float64)
    bound = np.asarray(bound, np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        q = np.where(bound > 0, d / bound, np.where(d == 0, 0.0, np.inf))
    return float(np.max(q)) if q.size else 0.0


# ---------------------------------------------------------------------------------------------------------------------
# One case per instance of the exact-form kernels at the smallest shapes that reach it: side, radial grid, data radii, builder
# arguments, and the layout the library has to pick (NXT, groups in use / all, ordinates in use, ordinate tiles, pairs, fold steps,
# data-radii tiles) -- tabulated from the host tables, asserted on the CPU (test_sz_chain_reference.py) and against the live context
# (test_gpu_exact_instances.py), so that no case drifts to another instance unnoticed.
# ---------------------------------------------------------------------------------------------------------------------
def _case(S, N, nflux, kw, nxt, ng_use, ng, Nk, nS, npair, nfold, ndt, what):
    return dict(S=S, N=N, nflux=nflux, kw=kw, what=what, id='%d-%d-%dradii' % (S, N, nflux),
                layout=dict(nxt=nxt, ng_use=ng_use, ng=ng, Nk=Nk, nS=nS, npair=npair, nfold=nfold, ndt=ndt, contracted=True))


CASES = [
    _case(15, 16, 5, {}, 1, 1, 1, 16, 1, 1, 0, 1, 'one ordinate tile: the only pair has no upper tile'),
    _case(24, 32, 5, {}, 1, 1, 1, 32, 2, 1, 0, 1, 'one full pair, no fold'),
    _case(32, 40, 5, {}, 1, 1, 1, 40, 3, 2, 1, 1, '<1, true> with a fold'),
    _case(65, 80, 19, {}, 3, 1, 1, 80, 5, 3, 1, 2, 'one output in the last tile'),
    _case(96, 120, 19, {}, 3, 1, 1, 105, 7, 4, 2, 2, 'full tiles'),
    _case(129, 150, 19, {}, 5, 1, 1, 128, 8, 4, 0, 2, 'one output in the fifth tile, no fold'),
    _case(129, 150, 32, {}, 5, 1, 1, 128, 8, 4, 0, 2, 'two full data-radii tiles'),
    _case(129, 150, 5, {}, 4, 1, 2, 128, 8, 4, 0, 1, 'pruning at a small side: 52 outputs in use of 65'),
    _case(144, 170, 19, {}, 5, 1, 1, 139, 9, 5, 3, 2, '72 outputs in use end inside a tile, with a fold'),
    _case(144, 170, 16, {}, 5, 1, 1, 139, 9, 5, 3, 1, 'one data-radii tile'),
    _case(160, 180, 19, {}, 5, 1, 1, 151, 10, 5, 0, 2, 'five full tiles'),
    _case(130, 300, 19, {}, 5, 1, 1, 129, 9, 5, 11, 2, 'more fold macro steps than pairs (the a2 loop; a tile folded over several steps lies beyond the map corner, its weights '
          'below rounding: the loop is run, an arithmetic error in it cannot show, DESIGN 6.2)'),
    _case(200, 240, 19, dict(step=1.0), 6, 2, 2, 179, 12, 6, 0, 2, 'two groups, 100 outputs in use end in group 1'),
    _case(224, 260, 19, dict(step=1.0), 6, 2, 2, 196, 13, 7, 5, 2, 'two groups and a fold'),
]
NWALKERS = 21


def build_case(case):
    """(problem, walkers) of a case: synthetic_problem(S, N, seed = S + 1), the flux table cut or refined to the case's data radii, data =
    the oracle's model at the fiducial vector plus noise, and a ball of 21 walkers with walker 2 outside the prior box and walker 4 NaN."""
    from joxsz_amd import datasets
    from oracle import joxsz_oracle as orc
    S = case['S']
    pb = datasets.synthetic_problem(S=S, N=case['N'], seed=S + 1, **case['kw'])
    fd, nflux = pb.flux_data, case['nflux']
    if nflux != fd.shape[1]:
        r = fd[0, :nflux] if nflux <= fd.shape[1] else np.linspace(fd[0, 0], fd[0, -1], nflux)
        pb.flux_data = np.ascontiguousarray(np.vstack((r, np.interp(r, fd[0], fd[1]), np.interp(r, fd[0], fd[2]))))
        pb.validate()
    p0 = orc.pars_dict(pb, datasets.fiducial_theta(pb))
    datasets.fill_data(pb, orc.sz_stages(pb, p0)['bright'], None if pb.sz_only else orc.calc_profiles(pb, p0), seed=S)
    th = datasets.walker_ball(pb, NWALKERS, spread=0.03, seed=S)
    th[2, 1] = 9.0
    th[4, 0] = np.nan
    return pb, th


def oriented_chain(pb, th, lib=None):
    """SzChain of a problem with its Abel matrix oriented on the oracle's ordinates of walker 0 (asserted: to rounding)."""
    from oracle import joxsz_oracle as orc
    ch = SzChain(pb, lib)
    st = orc.sz_stages(pb, orc.pars_dict(pb, th[0]))
    d = ch.orient(st['pp'], st['y'])
    assert d <= 4e-15, d
    return ch
