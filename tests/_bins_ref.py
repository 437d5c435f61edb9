"""The law of the posterior bin masses and mixture CDFs (include/frankenz_hip.h, docs/bins.md section 1) restated with NumPy: the
kernel CDF by SciPy's float64 `erfc` of the argument formed as the law's DIVISION `(x - y) / (s sqrt 2)` (the kernels multiply by a
reciprocal rounded once: an independent route to the same number), the sums in `np.longdouble` -- or, for the precondition of the
GPU bars, in float64 in a given order.  Also the inputs that tests/test_bins_host.py and tests/test_hip_bins.py share."""
import functools

import numpy as np
from scipy.special import erfc

LD = np.longdouble
U = 2.0 ** -53

WIDTHS = (1, 2, 63, 64, 65, 256, 257, 500, 4096)
NBINS = (1, 2, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256)      # both sides of every pass of 16 bins (and the issue's 31 .. 65)
DENSE = (1, 255, 4096, 4097, 70001)


def tol(W):
    """the bar of docs/predictive.md section 2 (a fixed-order sum of W terms, safety factor 4), ABSOLUTE here: the sums are of
    Z-normalised terms w_t / Z times a CDF value or a difference of two, each at most 1 in magnitude"""
    return 4. * (W / 64. + 16.) * U


def _kernel_cdf(x, y, s, edge):
    """F (n, P) float64 of n entries at P points; s == 0 is a step: the CDF is right-continuous (x >= y), a bin EDGE at y belongs to
    the bin above (x > y)"""
    x = np.asarray(x, dtype=np.float64)[None, :]
    y, s = y[:, None], s[:, None]
    with np.errstate(divide='ignore', invalid='ignore'):
        z = ((x.astype(LD) - y.astype(LD)) / (s.astype(LD) * np.sqrt(LD(2)))).astype(np.float64)
        F = 0.5 * erfc(-z)
    step = (x > y) if edge else (x >= y)
    return np.where(s == 0, step.astype(np.float64), F)


def _upper(e, y, s):
    with np.errstate(divide='ignore', invalid='ignore'):
        z = ((LD(e) - y.astype(LD)) / (s.astype(LD) * np.sqrt(LD(2)))).astype(np.float64)
        Uu = 0.5 * erfc(z)
    return np.where(s == 0, (y >= e).astype(np.float64), Uu)


def _row(rows, i, neighbors, nnbr, wt_thresh):
    """the included entries of row i -> (w float64-decided weights as longdouble, model indices, positions) or None (no posterior)"""
    W = rows.shape[1]
    n = W if nnbr is None else int(nnbr[i])
    r = np.asarray(rows[i, :n], dtype=np.float64)
    if n == 0 or np.isnan(r).any() or not np.isfinite(r.max()):
        return None
    j = np.arange(n) if neighbors is None else np.asarray(neighbors[i, :n])
    d = r - r.max()
    with np.errstate(divide='ignore'):
        keep = (np.exp(d) > 0) if not wt_thresh else (d > np.log(wt_thresh)) & (np.exp(d) > 0)
    return np.exp(d[keep].astype(LD)), j[keep]


def bins_ref(rows, y, s, edges, neighbors=None, nnbr=None, wt_thresh=1e-3, dtype=LD, perm=None):
    """-> p (N, Nbins), below (N), above (N) -- never normalised over the bins --, nskip.  `dtype` float64: every sum in float64 in
    index order, or with `perm` (a RandomState) in a shuffled order"""
    rows = np.asarray(rows, dtype=np.float64)
    y, s, edges = (np.asarray(a, dtype=np.float64) for a in (y, s, edges))
    N, NB = rows.shape[0], len(edges) - 1
    p, below, above = np.full((N, NB), np.nan), np.full(N, np.nan), np.full(N, np.nan)
    nskip = 0
    for i in range(N):
        got = _row(rows, i, neighbors, nnbr, wt_thresh)
        if got is None:
            nskip += 1
            continue
        w, j = got
        assert ((j >= 0) & (j < len(y))).all()
        if perm is not None:
            o = perm.permutation(len(w)); w, j = w[o], j[o]
        w = w.astype(dtype)
        F = _kernel_cdf(edges, y[j], s[j], True)
        Z = w.sum()
        p[i] = ((w[:, None] * (F[:, 1:] - F[:, :-1]).astype(dtype)).sum(axis=0) / Z).astype(np.float64)
        below[i] = float((w * F[:, 0].astype(dtype)).sum() / Z)
        above[i] = float((w * _upper(edges[-1], y[j], s[j]).astype(dtype)).sum() / Z)
    return p, below, above, nskip


def cdf_ref(rows, y, s, points, neighbors=None, nnbr=None, wt_thresh=1e-3, dtype=LD, perm=None):
    """points (P,) shared or (N, P) -> C (N, P), nskip"""
    rows = np.asarray(rows, dtype=np.float64)
    y, s, points = (np.asarray(a, dtype=np.float64) for a in (y, s, points))
    N = rows.shape[0]
    P = points.shape[-1]
    C = np.full((N, P), np.nan)
    nskip = 0
    for i in range(N):
        got = _row(rows, i, neighbors, nnbr, wt_thresh)
        if got is None:
            nskip += 1
            continue
        w, j = got
        if perm is not None:
            o = perm.permutation(len(w)); w, j = w[o], j[o]
        w = w.astype(dtype)
        F = _kernel_cdf(points if points.ndim == 1 else points[i], y[j], s[j], False)
        C[i] = ((w[:, None] * F.astype(dtype)).sum(axis=0) / w.sum()).astype(np.float64)
    return C, nskip


def assert_close(got, want, W, what, factor=1.):
    """|got - want| <= factor tol(W), nan in the same places"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: shape %s, expected %s" % (what, got.shape, want.shape)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=what)
    ok = ~np.isnan(want)
    err = np.abs(got[ok] - want[ok])
    bar = factor * tol(W)
    print("%s: worst %.3g of the bar %.3g" % (what, err.max() / bar if err.size else 0., bar))
    assert (err <= bar).all(), "%s: worst %.3g of its bar %.3g" % (what, err.max() / bar, bar)


def assert_bins(got_p, ref, W, got_below=None, got_above=None, normalize=False, got_nskip=None):
    """The device's masses against `bins_ref`'s at the bar `tol(W)`, absolute, for p, below and above alike.
    `normalize`: got_p was divided by its sum over the bins S' = S + D.  With |p'_k - p_k| <= tol each, |D| <= Nbins tol (+ the
    rounding of the sum over the bins itself, (Nbins / 64 + 6) u S), so that
        |p'_k / S' - p_k / S| <= (tol + (p_k / S) (Nbins tol + (Nbins / 64 + 8) u S)) / S'
    -- a bar that grows as 1 / S when little mass lies inside the range, as the error does.  S == 0 must give nan."""
    p, below, above, nskip = ref
    if got_nskip is not None:
        assert got_nskip == nskip
    if not normalize:
        assert_close(got_p, p, W, "p")
    else:
        NB = p.shape[1]
        S = p.astype(LD).sum(axis=1)
        with np.errstate(invalid='ignore', divide='ignore'):
            pn = (p / S[:, None]).astype(np.float64)
        np.testing.assert_array_equal(np.isnan(got_p), np.isnan(pn))
        ok = ~np.isnan(pn)
        t = tol(W)
        Sd = np.maximum(S.astype(np.float64) - NB * t, 1e-300)[:, None]
        bar = (t + pn * (NB * t + (NB / 64. + 8.) * U * S.astype(np.float64)[:, None])) / Sd
        err = np.abs(got_p - pn)
        assert (err[ok] <= bar[ok]).all(), "normalised p: worst %.3g of its bar" % np.max(err[ok] / bar[ok])
    if got_below is not None:
        assert_close(got_below, below, W, "below")
    if got_above is not None:
        assert_close(got_above, above, W, "above")


# ---- the inputs of the GPU tests (tests/test_hip_bins.py); tests/test_bins_host.py checks their precondition ------------------------
def edges_case(NB, seed=0, lo=0., hi=6.):
    """NB unequal bins on [lo, hi]"""
    rs = np.random.RandomState(7100 + 3 * NB + seed)
    cuts = np.sort(rs.uniform(lo, hi, NB - 1)) if NB > 1 else np.zeros(0)
    e = np.concatenate(([lo], cuts, [hi]))
    assert (np.diff(e) > 0).all()
    return e


def labels_case(M, edges, seed=0):
    """labels below e_0, above e_last and exactly on edges; errors from 1e-3 of a bin to ten times the range"""
    rs = np.random.RandomState(7200 + M % 1000 + seed)
    span = edges[-1] - edges[0]
    y = rs.uniform(edges[0] - 0.2 * span, edges[-1] + 0.2 * span, M)
    on = rs.rand(M) < 0.15
    y[on] = edges[rs.randint(0, len(edges), on.sum())]
    bin_w = span / (len(edges) - 1)
    s = np.exp(rs.uniform(np.log(1e-3 * bin_w), np.log(10. * span), M))
    return y, s


def sparse_case(N, W, M, seed, counts=None):
    """rows whose weights span e^-12, repeated indices when M < W, counts that include W, W - 1, 1 and 0 (as tests/test_hip_moments.py
    builds them)"""
    rs = np.random.RandomState(7300 + 17 * W + N + M + seed)
    rows = -rs.uniform(0., 12., size=(N, W))
    nbr = rs.randint(0, M, size=(N, W)).astype(np.int64)
    nnbr = rs.randint(0, W + 1, N).astype(np.int64)
    edge = [W, max(W - 1, 0), 1, 0] if counts is None else counts
    for i in range(N):
        if i < len(edge):
            nnbr[i] = min(edge[i], W)
    for i in range(N):
        rows[i, nnbr[i]:] = -np.inf; nbr[i, nnbr[i]:] = -99
    return rows, nbr, nnbr


@functools.lru_cache(maxsize=None)
def width_case(W, k):
    """the sparse rows of width W over M = 7 (k = 0) or 1000 (k = 1) models, the 8 unequal bins and the labels"""
    M = (7, 1000)[k]
    e = edges_case(8, W)
    y, s = labels_case(M, e, W + k)
    return sparse_case(5, W, M, k) + (y, s, e)


@functools.lru_cache(maxsize=None)
def nbins_case(NB):
    e = edges_case(NB, 1)
    y, s = labels_case(1000, e, NB)
    return sparse_case(5, 65, 1000, 100 + NB) + (y, s, e)


@functools.lru_cache(maxsize=None)
def dense_case(M):
    rs = np.random.RandomState(7900 + min(M, 4096))                  # 4096 and 4097 share their leading content
    m = max(M, 4097) if M in (4096, 4097) else M
    e = edges_case(9, 2)
    y, s = labels_case(m, e, 5)
    rows = -rs.uniform(0., 12., size=(3, m))
    rows, y, s = rows[:, :M].copy(), y[:M].copy(), s[:M].copy()
    if M == 4097:
        rows[:, -1] = -np.inf                                        # the entry the longer row adds holds no weight
    return rows, y, s, e


def cdf_points(P, N, seed=0):
    """unsorted points, shared (P,) and per object (N, P), some beyond the labels' range"""
    rs = np.random.RandomState(7500 + P + seed)
    return rs.uniform(-2., 8., P), rs.uniform(-2., 8., size=(N, P))
