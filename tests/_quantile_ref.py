"""The law of the posterior quantiles (include/frankenz_hip.h, docs/quantiles.md section 1) restated with NumPy: the mixture CDF `C` and
its left limit `C-` in `np.longdouble` from the pieces of tests/_bins_ref.py, the hull, `delta` and `tau` per row, and the contract
    x in the hull,    C-(x - 2 delta) - 2 tau <= p <= C(x + 2 delta) + 2 tau.
Also the inputs that tests/test_quantile_host.py and tests/test_hip_quantiles.py share."""
import functools

import numpy as np

import _bins_ref as br
from _bins_ref import _kernel_cdf, _row, tol

LD = np.longdouble
U = 2.0 ** -53
PROBS = np.array([1e-6, 1e-3, 0.025, 0.16, 0.5, 0.84, 0.975, 0.999, 1 - 1e-6])
QCOUNTS = (1, 7, 8, 9, 15, 16, 17, 33, 256)                          # both sides of a pass of 8 (FZ_QUANT_BB) and of 16


def mixture(rows, i, y, s, nbr, nnbr, wt_thresh):
    """the included entries of row i -> (w longdouble, y, s) or None (no posterior)"""
    got = _row(np.asarray(rows, dtype=np.float64), i, nbr, nnbr, wt_thresh)
    if got is None:
        return None
    w, j = got
    assert ((j >= 0) & (j < len(y))).all()
    return w, np.asarray(y, dtype=np.float64)[j], np.asarray(s, dtype=np.float64)[j]


def C(w, y, s, x, left=False):
    """C (left: its left limit C-) at the points x (P,), longdouble"""
    F = _kernel_cdf(np.atleast_1d(x), y, s, left)                    # `edge` form x > y: the left limit at a point mass
    return (w[:, None] * F.astype(LD)).sum(axis=0) / w.sum()


def hull(y, s):
    """a0, b0, delta of the included entries (the device forms the same float64 bits)"""
    a0, b0 = float((y - 40. * s).min()), float((y + 40. * s).max())
    return a0, b0, 4. * U * max(abs(a0), abs(b0))


def cantelli(w, y, s, p):
    """the bracket the kernel starts from, formed as the kernel forms it (float64, index order): mixture mean and deviation, Cantelli's
    inequality, rounded outward"""
    w = w.astype(np.float64)
    Z = w.sum()
    mu = (w * y).sum() / Z
    sig = np.sqrt((w * ((y - mu) * (y - mu) + s * s)).sum() / Z)
    rl, rh = sig * np.sqrt((1. - p) / p), sig * np.sqrt(p / (1. - p))
    return mu - rl - 1e-9 * (rl + abs(mu)), mu + rh + 1e-9 * (rh + abs(mu))


def bisect(w, y, s, p):
    """longdouble bisection over float64 points from the hull: (a, b) (P,) adjacent to within delta with C(a) < p <= C(b)"""
    p = np.atleast_1d(np.asarray(p, dtype=np.float64))
    a0, b0, delta = hull(y, s)
    a, b = np.full(len(p), a0), np.full(len(p), b0)
    for _ in range(200):
        m = 0.5 * a + 0.5 * b
        inside = (m > a) & (m < b) & (b - a > 0.25 * delta)
        if not inside.any():
            break
        up = C(w, y, s, m) >= p
        b = np.where(inside & up, m, b); a = np.where(inside & ~up, m, a)
    return a, b


def assert_quantiles(got, rows, y, s, p, nbr=None, nnbr=None, wt_thresh=1e-3, got_nskip=None, what="quantiles"):
    """the contract of docs/quantiles.md section 1 for every (row, p), nan exactly on the rows without a posterior, nskip the law's.
    Prints the worst case as a share of the margin 2 tau; returns it."""
    rows = np.asarray(rows, dtype=np.float64)
    p = np.atleast_1d(np.asarray(p, dtype=np.float64))
    got = np.asarray(got)
    N, W = rows.shape
    assert got.shape == (N, len(p)), "%s: shape %s, expected %s" % (what, got.shape, (N, len(p)))
    tau = tol(W)
    nskip, worst = 0, 0.
    for i in range(N):
        mix = mixture(rows, i, y, s, nbr, nnbr, wt_thresh)
        if mix is None:
            nskip += 1
            assert np.isnan(got[i]).all(), "%s: row %d has no posterior and must be nan" % (what, i)
            continue
        w, yy, ss = mix
        x = got[i]
        assert np.isfinite(x).all(), "%s: row %d: %r" % (what, i, x)
        a0, b0, delta = hull(yy, ss)
        assert ((x >= a0) & (x <= b0)).all(), "%s: row %d leaves its hull [%r, %r]: %r" % (what, i, a0, b0, x)
        # the shifted points rounded TOWARDS x: never a looser check than the exact x -+ 2 delta
        hi = np.nextafter(x + 2. * delta, -np.inf) if delta > 0 else x
        lo = np.nextafter(x - 2. * delta, np.inf) if delta > 0 else x
        short = np.maximum(p - C(w, yy, ss, hi), C(w, yy, ss, lo, left=True) - p).astype(np.float64)
        share = short / (2. * tau)
        worst = max(worst, float(share.max()))
        assert (share <= 1.).all(), "%s: row %d misses the contract: worst %.3g of the margin 2 tau = %.3g at p = %r" % (
            what, i, share.max(), 2. * tau, p[int(np.argmax(share))])
    print("%s: worst %.3g of the margin 2 tau = %.3g" % (what, worst, 2. * tau))
    if got_nskip is not None:
        assert got_nskip == nskip, "%s: nskip %r, the law's %d" % (what, got_nskip, nskip)
    return worst


# ---- the inputs of the GPU tests; tests/test_quantile_host.py checks their preconditions --------------------------------------------
@functools.lru_cache(maxsize=None)
def width_case(W, k, zeros):
    """_bins_ref.width_case with the labels' errors as given, or with every second error 0"""
    rows, nbr, nnbr, y, s, e = br.width_case(W, k)
    if zeros:
        s = s.copy(); s[::2] = 0.
    return rows, nbr, nnbr, y, s


def probs_case(Q):
    """Q unsorted probabilities with duplicates, the extremes among them"""
    rs = np.random.RandomState(7600 + Q)
    p = rs.uniform(1e-4, 1. - 1e-4, Q)
    p[0] = 0.5
    if Q > 2:
        p[1], p[2] = 1e-6, p[0]
    if Q > 16:
        p[16] = 1. - 1e-6
    return p
