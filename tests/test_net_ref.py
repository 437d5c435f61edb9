"""tests/_net_ref.py, the longdouble reference of the network-inference kernels, against the oracle's _node_select (which golden G14
pins to the reference's networks.py:885-896) on tie-free random rows, both rules.  CPU only."""
import numpy as np
import pytest
from scipy.special import logsumexp

import frankenz_oracle as fo
import _net_ref as nr


def rows(Nn, seed):
    rs = np.random.RandomState(seed)
    lp = rs.normal(0, 3, size=(12, Nn)) - rs.uniform(0, 50, size=(12, 1))
    assert all(len(np.unique(r)) == Nn for r in lp)                            # tie-free: np.argsort's order is defined
    return lp


@pytest.mark.parametrize('Nn', [1, 2, 64, 65, 257, 1000])
def test_select_and_stats_equal_the_oracle(Nn):
    lp = rows(Nn, 500 + Nn)
    for wt in (1e-3, 0.5, 1.0, 0.0):
        for r in lp:
            with np.errstate(divide='ignore'):
                want = fo._node_select(r, wt, None)
            sel, gap = nr.select(r, True, wt, 0.5)
            np.testing.assert_array_equal(sel, want)
            assert gap == np.inf
            if len(want):
                lmap, levid = nr.stats(r, sel)
                assert lmap == np.max(r[want])
                np.testing.assert_allclose(float(levid), logsumexp(r[want]), rtol=1e-14, atol=1e-14)
    for cdf in (0.5, 0.05, 2e-4):
        for r in lp:
            want = fo._node_select(r, None, cdf)
            sel, gap = nr.select(r, False, 0.0, cdf)
            assert gap > 1e-9                           # float64 and longdouble running sums cannot disagree about the prefix
            np.testing.assert_array_equal(sel, want)
            lmap, levid = nr.stats(r, sel)
            if len(want):
                assert lmap == np.max(r[want])
                np.testing.assert_allclose(float(levid), logsumexp(r[want]), rtol=1e-14, atol=1e-14)
            else:
                assert lmap == -np.inf and levid == -np.inf


def test_special_rows_follow_numpy():
    """what NumPy itself gives for a nan, a +inf and an all -inf row (the oracle's two lines, run as they stand), and the two
    conventions that are the project's own: ties by index, every column for a negative wt_thresh"""
    Nn = 70
    base = rows(Nn, 9)[0]
    nan = base.copy(); nan[9] = np.nan
    top = base.copy(); top[[4, 60]] = np.inf
    low = np.full(Nn, -np.inf)
    with np.errstate(all='ignore'):
        for r in (nan, top, low):
            for wt in (1e-3, 0.0):
                np.testing.assert_array_equal(nr.select(r, True, wt, 0.5)[0], fo._node_select(r, wt, None))
        for r in (top, low):                            # (np.argsort puts nan last and the oracle's cdf <= limit is False from there on)
            np.testing.assert_array_equal(nr.select(r, False, 0.0, 0.05)[0], fo._node_select(r, None, 0.05))
    assert len(nr.select(nan, False, 0.0, 0.05)[0]) == 0 and len(nr.select(nan, True, -np.inf, 0.5)[0]) == 0
    assert len(nr.select(top, False, 0.0, 0.05)[0]) == Nn - 2 and len(nr.select(low, False, 0.0, 0.05)[0]) == 0
    assert len(nr.select(low, True, 0.0, 0.5)[0]) == 0 and len(nr.select(top, True, 0.0, 0.5)[0]) == 0
    np.testing.assert_array_equal(nr.select(low, True, -np.inf, 0.5)[0], np.arange(Nn))
    tie = base.copy(); tie[::7] = tie[0]
    sel = nr.select(tie, False, 0.0, 2e-4)[0]
    pos = [int(np.nonzero(sel == c)[0][0]) for c in range(0, Nn, 7) if c in sel]
    assert pos == sorted(pos) and len(pos) > 1          # equal values in index order
    assert nr.stats(base, np.zeros(0, dtype=int)) == (-np.inf, -np.inf)


def test_table_gather_stack_on_a_case_worked_by_hand():
    match = np.array([2, 0, 1]); off = np.array([0, 2, 2, 5]); items = np.array([10, 11, 20, 21, 22])
    sels = [np.array([1, 0]), np.array([2]), np.zeros(0, dtype=int)]         # nodes (0, 2), (1), ()
    np.testing.assert_array_equal(nr.table(sels, match, off, items, 6),
                                  [[10, 11, 20, 21, 22, 10], [0] * 6, [0] * 6])
    np.testing.assert_array_equal(nr.table(sels, match, off, items, 3)[0], [10, 11, 20])
    assert [nr.rawlen(s, match, off) for s in sels] == [5, 0, 0]
    plane = np.arange(9.).reshape(3, 3)
    np.testing.assert_array_equal(nr.gather(plane, sels, 2, -99.), [[1, 0], [5, -99], [-99, -99]])
    lp = np.log(np.array([[1., 3., 5.], [1., 1., 1.], [1., 1., 1.]]))
    node_pdfs = np.array([[1., 0.], [0., 1.], [1., 1.]])
    p, lmap, levid = nr.stack(lp, sels, match, node_pdfs)
    # object 0: weights 3/4 on node 0 and 1/4 on node 2 -> (1, 1/4) / (5/4)
    np.testing.assert_allclose(p[0].astype(float), [0.8, 0.2], rtol=1e-15)
    np.testing.assert_allclose(p[1].astype(float), [0., 1.], rtol=1e-15)
    assert np.all(np.isnan(p[2].astype(float))) and lmap[2] == -np.inf and levid[2] == -np.inf
    assert lmap[0] == np.log(3.) and abs(float(levid[0]) - np.log(4.)) < 1e-15
