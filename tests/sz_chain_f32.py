"""The derived bound of tests/sz_chain_reference.py extended to the exact form with fp32 products (dtype='f32x': jx_ordrow32_kernel of
csrc/jx_exact.hpp), and a numpy float32 evaluation of the chain under that contract (no GPU; used by test_sz_chain_f32.py and
test_gpu_exact_f32.py).

The contract.  Of the four lines of the chain

    y = ys A pp,    row = Wy y,    m = E (cf . row),    chi2 = sum_d ((f_d - m_d) / e_d)^2

the first two run on v_mfma_f32_16x16x4_f32 -- exact fp32, bit for bit a chain of fmaf in k order -- with operands rounded once: the host's
tables ys A, Wy and the folded operator Wf = Wy[:, last tile] ys A[last tile, :] (built in long double, then double, as for f64) to fp32
with entries below FLT_MIN stored as 0; pp as it is loaded; the pair's 32 ordinates once.  Accumulation is fp32 inside a wave's chains; what
leaves a chain is converted to fp64 and every further sum (two chains of a tile, four waves, the two chains of the row product, the pairs)
and everything from the conversion factor on is today's fp64 code.

The bound.  Every elementary term E[d][x] cf[x] Wy[x][k] ys A[k][j] pp[j] collects, beside the fp64 factors (1 + delta), |delta| <= u = 2^-53,
that sz_chain_reference counts (n = N + Nkp + 16 NXT ng_use + 32: all of them kept, although the two big sums now collect most of theirs in
fp32), factors (1 + delta32), |delta32| <= u32 = 2^-24, counted from the code as built:

    2                    the roundings of pp[j] and of (ys A)[k][j] to fp32,
    8 ceil(nSj / 4)      the ordinate's chain: a wave takes every fourth of the nSj macro steps of 16 radii, a macro step is four instructions
                         of four terms each, alternating between the two chains of the tile: 8 fmaf per chain and step,
    2                    the roundings of the ordinate y[k] and of Wy[x][k] to fp32,
    16 (1 + fsteps)      the row product's chain: 16 fmaf for a tile's 16 ordinates (four instructions of four terms); the upper tile's chain
                         continues into the folded tile's share, 16 fmaf per fold step, fsteps = ceil(nfold / pairs) of them per block (a
                         term of the folded share has rounded pp[j] and Wf[x][j] and the same chain: fewer factors),

    n32 = 8 ceil(nSj / 4) + 16 (1 + fsteps) + 4  <=  N + Nkp + 16 nfold + 32   (asserted),
    gamma32 = n32 u32 / (1 - n32 u32),           gamma_x = (1 + gamma32) (1 + gamma) - 1     in the place of gamma.

Underflow.  An fp32 rounding of a value below FLT_MIN = 2^-126 in magnitude loses at most eta = 2^-126 ABSOLUTE -- whether the result is a
subnormal, flushed to zero by the instruction, or stored as 0 by the host -- so nothing has to be known about the denormal mode.  One eta
at each rounding, carried to the row through the absolute values of what multiplies it:

    eta in pp[j]            -> |Wy| |ys A| 1                  =: WA1[x]
    eta in (ys A)[k][j]     -> |Wy| 1 * sum_j |pp_j|          =: W1[x] |pp|_1
    eta in an ordinate's fmaf (at most 8 ceil(nSj / 4) + 1 per ordinate, its rounding to fp32 included)  -> n32 W1[x]
    eta in Wy[x][k]         -> sum_k |y|_k <= |ys A| |pp| 1   =: |y|_1
    eta in Wf[x][j]         -> |pp|_1
    eta in the row's fmaf   -> n32

    row_under = eta (1 + gamma_x) (WA1 + W1 (|pp|_1 + n32) + |y|_1 + |pp|_1 + n32),        m_under = |E| (|cf| . row_under)
    |row - row_ref| <= row_bound = gamma_x row_abs + row_under,      |m - m_ref| <= m_bound = gamma_x m_abs + m_under

and chi_bound is sz_chain_reference's formula on this m_bound, unchanged.  Accepted walkers only: a walker the range guard rejects (a
profile value that is not finite or beyond T) has no row to bound.

A derivation again, not a measurement.  test_sz_chain_f32.py shows on the CPU, at every case, that the float32 evaluation below -- the
kernel's grouping, chain by chain -- stays inside it and that a dropped profile point, macro step, output or data radius leaves it."""
import numpy as np

import sz_chain_reference as szr
from sz_chain_reference import LD, U

U32 = 2.0 ** -24
ETA = 2.0 ** -126                      # FLT_MIN
F32 = np.float32


def gamma32(n):
    return n * U32 / (1.0 - n * U32)


def round_table(a):
    """A host table rounded once to fp32; a nonzero entry below FLT_MIN in magnitude is stored as 0 (jxt::round_to_f32)."""
    with np.errstate(under='ignore', over='ignore'):
        f = np.asarray(a, np.float64).astype(F32)
    f[np.abs(f) < F32(ETA)] = F32(0.0)
    return f


def _fma32(acc, a, b):
    """fmaf on float32 arrays: the product of two fp32 values is exact in fp64; the sum is rounded to fp64, then to fp32 (a double rounding that
    can differ from fmaf's single one by 2^-29 of an fp32 ulp: far below anything the bound resolves)."""
    with np.errstate(under='ignore'):
        return (acc.astype(np.float64) + a.astype(np.float64) * b.astype(np.float64)).astype(F32)


class SzChainF32(szr.SzChain):
    """SzChain with the bound of the fp32 products and their float32 evaluation.  Built from a problem, or from an SzChain (tables shared)."""

    def __init__(self, pb=None, lib=None, chain=None):
        if chain is not None:
            self.__dict__.update(chain.__dict__)
        else:
            super().__init__(pb, lib)
        lay, N = self.layout, self.N
        self.npair_folded = (lay['nS'] - 1) // 2 if lay['nfold'] else 0
        self.fsteps = -(-lay['nfold'] // self.npair_folded) if lay['nfold'] else 0
        self.n32 = 8 * (-(-lay['nSj'] // 4)) + 16 * (1 + self.fsteps) + 4
        assert self.n32 <= N + lay['Nkp'] + 16 * lay['nfold'] + 32, (self.n32, lay)
        self.gamma32 = gamma32(self.n32)
        self.gamma_x = (1.0 + self.gamma32) * (1.0 + self.gamma) - 1.0

    # ---- the bound
    def reference(self, pp, cf, errors=None):
        """As SzChain.reference, with row_bound, m_bound and chi_bound of the fp32 products (accepted walkers only)."""
        pp, cf = np.atleast_2d(np.asarray(pp, np.float64)), np.atleast_2d(np.asarray(cf, np.float64))
        e = self.e if errors is None else np.asarray(errors, np.float64)
        r = super().reference(pp, cf, errors)
        aA, aW, aE = abs(self.ys) * np.abs(self.A), np.abs(self.Wy), np.abs(self.E)
        y_abs = np.abs(pp) @ aA.T
        row_abs = y_abs @ aW.T
        m_abs = (np.abs(cf) * row_abs) @ aE.T
        W1 = aW.sum(axis=1)
        WA1 = aW @ aA.sum(axis=1)
        pp1, y1 = np.abs(pp).sum(axis=1, keepdims=True), y_abs.sum(axis=1, keepdims=True)
        row_under = ETA * (1.0 + self.gamma_x) * (WA1[None, :] + W1[None, :] * (pp1 + self.n32) + y1 + pp1 + self.n32)
        m_under = (np.abs(cf) * row_under) @ aE.T
        row_bound, m_bound = self.gamma_x * row_abs + row_under, self.gamma_x * m_abs + m_under
        zb = m_bound / e
        z = ((self.f.astype(LD) - r['m']) / e.astype(LD)).astype(np.float64)
        chi_bound = np.sum(2.0 * np.abs(z) * zb + zb * zb, axis=1) + 8.0 * U * r['chi2'].astype(np.float64)
        r.update(row_bound=row_bound, m_bound=m_bound, chi_bound=chi_bound)
        return r

    # ---- the float32 evaluation under the contract
    def _tables32(self):
        if not hasattr(self, '_t32'):
            lay, N = self.layout, self.N
            Ty = round_table(self.ys * self.A)                            # (y_scale A in fp64, as jxt::abel_ordinate_layout forms it)
            Wy32 = round_table(self.Wy)
            Wf32 = None
            if lay['nfold']:
                i0 = 16 * (lay['nS'] - 1)
                Wf = (self.Wy[:, i0:min(N, i0 + 16)].astype(LD) @ (LD(self.ys) * self.A[i0:min(N, i0 + 16), :].astype(LD))).astype(np.float64)
                Wf[:, :i0] = 0.0                                          # (A is upper triangular: the folded tile reads the profile from its own first radius on)
                Wf32 = round_table(Wf)
            self._t32 = (Ty, Wy32, Wf32)
        return self._t32

    def f32(self, pp, cf, folded=False, drop=None):
        """(row, m, chi2, y) as jx_ordrow32_kernel and the fp64 tail form them.  folded: the timed path's pairing (odd number of ordinate tiles: the
        last one as an operator on the profile); otherwise the plain pairing of every call with taps.
        drop: 'profile point' (the last radius), 'macro step' (the last 16 radii), 'first macro step' (the first 16), 'first output', 'data radius'
        (the last)."""
        lay, N, nrow = self.layout, self.N, self.nrow
        pp, cf = np.atleast_2d(np.asarray(pp, np.float64)).copy(), np.atleast_2d(np.asarray(cf, np.float64))
        if drop == 'profile point':
            pp[:, -1] = 0.0
        if drop == 'macro step':
            pp[:, 16 * (lay['nSj'] - 1):] = 0.0
        if drop == 'first macro step':
            pp[:, :16] = 0.0
        W = pp.shape[0]
        nS, nSj = lay['nS'], lay['nSj']
        Ty, Wy32, Wf32 = self._tables32()
        folded = bool(folded and lay['nfold'])
        npair = (nS - 1) // 2 if folded else (nS + 1) // 2
        ntile = nS - 1 if folded else nS
        ppp = np.zeros((W, 16 * nSj), F32)
        with np.errstate(under='ignore'):
            ppp[:, :N] = pp.astype(F32)                                   # rounded to nearest as it is loaded
        Typ = np.zeros((16 * nS, 16 * nSj), F32)
        kr = min(N, 16 * nS)
        Typ[:kr, :N] = Ty[:kr, :]
        # ordinates: tile t of pair p (p = t or 2 npair - 1 - t); wave v takes the steps p + v, p + v + 4, ...; chain c the sub-steps c, c + 2;
        # a sub-step is one instruction: k = lk = 0..3 in order, radius 16 s + 4 lk + e
        y = np.zeros((W, 16 * nS))
        for t in range(ntile):
            p = t if t < npair else 2 * npair - 1 - t
            tile = slice(16 * t, 16 * t + 16)
            tot = None
            for v in range(4):
                chains = [np.zeros((W, 16), F32), np.zeros((W, 16), F32)]
                for s in range(p + v, nSj, 4):
                    if s < t:
                        continue                                          # (the upper tile's products start at its own first step; below it the operator is zero)
                    for e in range(4):
                        for lk in range(4):
                            j = 16 * s + 4 * lk + e
                            chains[e & 1] = _fma32(chains[e & 1], ppp[:, j:j + 1], Typ[tile, j][None, :])
                wave = chains[0].astype(np.float64) + chains[1].astype(np.float64)
                tot = wave if tot is None else tot + wave                 # ((w0 + w1) + w2) + w3
            y[:, tile] = tot
        # row product: per pair two chains (lower tile | upper tile, then the fold steps p, p + npair, ...), added in fp64, the pairs in pair order
        Wp = np.zeros((nrow, 16 * nS), F32)
        Wp[:, :min(N, 16 * nS)] = Wy32[:, :min(N, 16 * nS)]
        with np.errstate(under='ignore', over='ignore'):
            y32 = y.astype(F32)                                           # the pair's 32 ordinates rounded once
        row = np.zeros((W, nrow))
        for p in range(npair):
            q = 2 * npair - 1 - p
            c0, c1 = np.zeros((W, nrow), F32), np.zeros((W, nrow), F32)
            for e in range(4):
                for lk in range(4):
                    k = 16 * p + 4 * lk + e
                    c0 = _fma32(c0, y32[:, k:k + 1], Wp[:, k][None, :])
            if q < ntile:
                for e in range(4):
                    for lk in range(4):
                        k = 16 * q + 4 * lk + e
                        c1 = _fma32(c1, y32[:, k:k + 1], Wp[:, k][None, :])
            if folded:
                for sf in range(p, lay['nfold'], npair):
                    for e in range(4):
                        for lk in range(4):
                            j = 16 * (nS - 1 + sf) + 4 * lk + e
                            if j < N:
                                c1 = _fma32(c1, ppp[:, j:j + 1], Wf32[:, j][None, :])
            row = row + (c0.astype(np.float64) + c1.astype(np.float64))
        if drop == 'first output':
            row[:, 0] = 0.0
        b = cf * row
        m = b @ self.E.T
        if drop == 'data radius':
            m[:, -1] = 0.0
        z = (self.f - m) / self.e
        return row, m, np.sum(z * z, axis=1), y[:, :N] if 16 * nS >= N else y
