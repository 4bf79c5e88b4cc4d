"""The row and fold operators as the pair-wise kernels read them (jxt::row_tile_major, csrc/jx_tables.hpp): a pure permutation of
jxt::exact_row_layout's and jxt::exact_fold_layout's tables, [g][s][4 e][64 lanes][NXT] -> [g][s][NXT][64 lanes][4 e],

    out[((((g nS + s) NXT + t) 64 + lane) 4 + e] = in[((((g nS + s) 4 + e) 64 + lane) NXT + t],

so that a wave's operand of one output tile is one contiguous run and a lane's four sub-steps one vector load (jx_ordrow_kernel,
jx_ordrow32_kernel of csrc/jx_exact.hpp).  Entry by entry and bitwise against the formula, a bijection that writes every output index
once, the same for the fp32 tables, and the input -- from which the f32x range guard is derived -- left as it was.
CPU only: the host-only build libjx_tables_host.so."""
import ctypes
import os

import numpy as np
import pytest

LIB = os.path.join(os.path.dirname(__file__), '..', 'joxsz_amd', 'csrc', 'libjx_tables_host.so')
DP = ctypes.POINTER(ctypes.c_double)

# nrow, N, NXT, ng: two tiles in two groups with outputs ending inside a tile; six full tiles; five tiles, one output in the last; two groups of six
SHAPES = [(37, 100, 2, 2), (96, 80, 6, 1), (65, 150, 5, 1), (100, 240, 6, 2)]


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build_host_tables()
    lib = ctypes.CDLL(LIB)
    lib.jxt_row_layout_abs_rowsum.restype = ctypes.c_double
    return lib


def _p(a):
    return a.ctypes.data_as(DP)


def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _tables(lib, nrow, N, NXT, ng):
    """(Opk [ng][nS][4][64][NXT], Wfk [ng][nfold][4][64][NXT]) of a random operator with an odd number of ordinate tiles (so that it folds)."""
    rng = np.random.default_rng(nrow * 1000 + N)
    nSj = (N + 15) // 16
    nS = nSj if nSj & 1 else nSj - 1
    Wy = np.ascontiguousarray(rng.normal(size=(nrow, N)) * 10.0 ** rng.uniform(-30, 0, size=(nrow, N)))
    r = np.ascontiguousarray(np.geomspace(1.0, 900.0, N))
    Opk = np.full((ng, nS, 4, 64, NXT), np.nan)
    assert lib.jxt_exact_row_layout(_p(Wy), nrow, N, nS, NXT, ng, _p(Opk)) == 0
    nfold = nSj - (nS - 1)
    Wfk = np.full((ng, nfold, 4, 64, NXT), np.nan)
    assert lib.jxt_exact_fold_layout(_p(Wy), nrow, _p(r), N, ctypes.c_double(1.7e-3), nS, nSj, NXT, ng, _p(Wfk)) == 0
    assert not np.isnan(Opk).any() and not np.isnan(Wfk).any()
    assert np.count_nonzero(Opk) > Opk.size // 4 and np.count_nonzero(Wfk) > 0
    return Opk, Wfk


def _permute(lib, tab, f32=False):
    ng, nS, _, _, NXT = tab.shape
    src = tab.copy()
    out = np.full((ng, nS, NXT, 64, 4), np.nan, tab.dtype)          # a sentinel in every entry: each must be written
    assert lib.jxt_row_tile_major(_vp(src), nS, NXT, ng, 1 if f32 else 0, _vp(out)) == 0
    assert src.tobytes() == tab.tobytes()                           # the input is read, never written
    return out


@pytest.mark.parametrize('nrow,N,NXT,ng', SHAPES)
def test_permutation_matches_the_formula(lib, nrow, N, NXT, ng):
    """Entry by entry, bitwise, through the flat index formulas of the two layouts -- row and fold operator."""
    for tab in _tables(lib, nrow, N, NXT, ng):
        nS = tab.shape[1]
        out = _permute(lib, tab)
        assert not np.isnan(out).any()
        g, s, t, lane, e = np.meshgrid(np.arange(ng), np.arange(nS), np.arange(NXT), np.arange(64), np.arange(4), indexing='ij')
        dst = ((((g * nS + s) * NXT + t) * 64 + lane) * 4 + e).ravel()
        src = ((((g * nS + s) * 4 + e) * 64 + lane) * NXT + t).ravel()
        assert np.array_equal(np.sort(dst), np.arange(tab.size)) and np.array_equal(np.sort(src), np.arange(tab.size))
        assert out.ravel()[dst].tobytes() == tab.ravel()[src].tobytes()
        # ... which is the transposition of the axes, and what a lane of the kernel's 32-byte load of (g, s, t) holds: the four sub-steps of
        # Wy[16 (g NXT + t) + (lane & 15)][16 s + 4 (lane >> 4) + e]
        assert out.tobytes() == np.ascontiguousarray(tab.transpose(0, 1, 4, 3, 2)).tobytes()


@pytest.mark.parametrize('nrow,N,NXT,ng', SHAPES)
def test_permutation_is_a_bijection(lib, nrow, N, NXT, ng):
    """The sorted values are those of the input, and a table of distinct values (its own flat indices) comes back with every output index
    written exactly once: no sentinel left, no value twice."""
    for tab in _tables(lib, nrow, N, NXT, ng):
        out = _permute(lib, tab)
        assert np.array_equal(np.sort(out, axis=None), np.sort(tab, axis=None))
        idx = np.arange(tab.size, dtype=np.float64).reshape(tab.shape)
        back = _permute(lib, idx)
        assert not np.isnan(back).any()
        assert np.array_equal(np.sort(back, axis=None), idx.ravel())


@pytest.mark.parametrize('nrow,N,NXT,ng', SHAPES)
def test_float_instantiation(lib, nrow, N, NXT, ng):
    """The fp32 tables go through the same permutation: np.float32 of the same values at the same places."""
    for tab in _tables(lib, nrow, N, NXT, ng):
        with np.errstate(under='ignore'):
            t32 = np.ascontiguousarray(tab.astype(np.float32))
        out32 = _permute(lib, t32, f32=True)
        assert out32.dtype == np.float32 and not np.isnan(out32).any()
        with np.errstate(under='ignore'):
            want = _permute(lib, tab).astype(np.float32)
        assert out32.tobytes() == want.tobytes()


def test_range_guard_input_is_unchanged(lib):
    """The f32x range guard is derived from the fp32 table in exact_row_layout's order, ahead of the permutation: its largest absolute row
    sum (jxt::row_layout_abs_rowsum) is the operator's own, before and after the table went through the permutation."""
    nrow, N, NXT, ng = SHAPES[3]
    Opk, _ = _tables(lib, nrow, N, NXT, ng)
    nS = Opk.shape[1]
    t32 = np.zeros(Opk.shape, np.float32)
    assert lib.jxt_round_to_f32(_p(Opk), ctypes.c_longlong(Opk.size), t32.ctypes.data_as(ctypes.POINTER(ctypes.c_float))) == 0
    fp = ctypes.POINTER(ctypes.c_float)
    before = lib.jxt_row_layout_abs_rowsum(t32.ctypes.data_as(fp), nS, NXT, ng)
    out32 = _permute(lib, t32, f32=True)
    after = lib.jxt_row_layout_abs_rowsum(t32.ctypes.data_as(fp), nS, NXT, ng)
    # row x = 16 (g NXT + t) + li of the operator, summed over s, e and lk in the table's order
    rs = np.zeros(16 * NXT * ng)
    a = np.abs(t32.astype(np.float64))
    for g in range(ng):
        for s in range(nS):
            for e in range(4):
                for lane in range(64):
                    rs[16 * (g * NXT + np.arange(NXT)) + (lane & 15)] += a[g, s, e, lane, :]
    assert before == after == rs.max() and before > 0.0
    assert out32.tobytes() == np.ascontiguousarray(t32.transpose(0, 1, 4, 3, 2)).tobytes()
