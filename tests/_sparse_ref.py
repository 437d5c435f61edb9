"""The law of the sparse fits (docs/sparse_fits.md) in NumPy, and the rows tests/test_sparse_host.py and tests/test_hip_sparse.py share.

For one row r[0..L) of ln-weights, a cap W >= 1 and a cut lncut < 0 (-inf allowed):
    a nan among the L entries, or a max that is not finite: nothing is kept (Nneighbors = 0)
    else m = max r;  entry j is eligible iff r_j - m > lncut  (one IEEE subtraction, a strict comparison)
    kept: the first min(W, E) eligible entries in the order (value descending, index ascending), stored in that order
    neighbors padded with -99, vals with -inf;  lmap = max r, levid = logsumexp r of the FULL row;  lnkept = logsumexp of the kept

A device row comes from the device's own likelihood and may differ from the oracle's by FIT_TOL: an object whose kept SET or ORDER
hangs on a difference that small is `fragile` -- the only objects the GPU tests may leave out of an index comparison with the
oracle.  Comparisons on given rows are exact."""
import numpy as np

import _draw_ref as dr

FIT_TOL = dr.FIT_TOL
FRAGILE_CAP = 0.01
PLANE_TOL = dict(rtol=1e-8, atol=1e-8)       # what the parity tests hold the fit_* planes to
PADS = dict(lnprior=-np.inf, lnlike=-np.inf, lnprob=-np.inf, chi2=np.inf, Ndim=0, scale=1., scale_err=0.)


def has_posterior(r):
    return len(r) > 0 and not np.isnan(r).any() and np.isfinite(r.max())


def lncut_of(wt_thresh):
    return np.log(wt_thresh) if wt_thresh else -np.inf


def logsumexp(v):
    m = v.max()
    return m + np.log(np.exp(v - m).sum())


def kept_order(r, W, lncut):
    """indices of the kept entries of one row, in the law's order"""
    if not has_posterior(r):
        return np.zeros(0, dtype=np.int64)
    with np.errstate(invalid='ignore'):
        elig = (r - r.max()) > lncut
    order = np.lexsort((np.arange(len(r)), -r))           # value descending, then index ascending
    return order[elig[order]][:W].astype(np.int64)


def kept_order_restated(r, W, lncut):
    """the same rule restated: a STABLE sort of -r keeps equal values in index order; the eligible ones are taken in turn"""
    if not has_posterior(r):
        return np.zeros(0, dtype=np.int64)
    m = r.max()
    out = []
    for j in np.argsort(-r, kind='stable'):
        if r[j] - m > lncut:
            out.append(j)
            if len(out) == W:
                break
    return np.array(out, dtype=np.int64)


def sparse_ref(rows, W, lncut, order=kept_order):
    """-> dict(neighbors (N, W) int64, Nneighbors (N) int64, vals (N, W), lmap, levid, lnkept (N))"""
    rows = np.asarray(rows, dtype=np.float64)
    N = len(rows)
    nbr = np.full((N, W), -99, dtype=np.int64)
    vals = np.full((N, W), -np.inf)
    nn = np.zeros(N, dtype=np.int64)
    lmap, levid, lnkept = np.full(N, np.nan), np.full(N, np.nan), np.full(N, -np.inf)
    for i, r in enumerate(rows):
        if not np.isnan(r).any():
            lmap[i] = levid[i] = r.max()
        if not has_posterior(r):
            continue
        k = order(r, W, lncut)
        nn[i] = len(k); nbr[i, :len(k)] = k; vals[i, :len(k)] = r[k]
        levid[i] = logsumexp(r)
        lnkept[i] = logsumexp(r[k])
    return dict(neighbors=nbr, Nneighbors=nn, vals=vals, lmap=lmap, levid=levid, lnkept=lnkept)


def fragile(rows, W, lncut, tol=FIT_TOL):
    """(N) bool: among the object's first W + 1 eligible entries two adjacent values lie within tol of each other, or an entry lies
    within tol of the cut"""
    rows = np.asarray(rows, dtype=np.float64)
    out = np.zeros(len(rows), dtype=bool)
    for i, r in enumerate(rows):
        if not has_posterior(r):
            continue
        v = r[kept_order(r, W + 1, lncut)]
        if len(v) > 1 and (np.abs(np.diff(v)) <= tol).any():
            out[i] = True
        if np.isfinite(lncut):
            fin = r[np.isfinite(r)]
            if (np.abs(fin - r.max() - lncut) <= tol).any():
                out[i] = True
    return out


def gather_ref(plane, nbr, nn, pad):
    """plane (N, M) at the kept entries, padded"""
    out = np.full(nbr.shape, pad, dtype=plane.dtype)
    for i in range(len(nbr)):
        out[i, :nn[i]] = plane[i, nbr[i, :nn[i]]]
    return out


# ---- hand-made rows ---------------------------------------------------------------------------------------------------------------
def special_rows(L, seed=0):
    """rows of length L whose difficulty is in the ORDER: a constant row, values quantised to 1/4 (tie groups straddle any W-th
    place), equal values at the segment and geometry seams (255, 256, 257 and 4095, 4096, 4097) above everything else, the maximum
    repeated, ascending and descending rows"""
    rs = np.random.RandomState(4200 + L + seed)
    base = -rs.uniform(0., 12., size=L)
    rows = [np.full(L, -3.25), np.round(base * 4.) / 4., np.sort(base), np.sort(base)[::-1].copy()]
    seam = base.copy()
    for j in (255, 256, 257, 4095, 4096, 4097):
        if j < L:
            seam[j] = 1.5
    rows.append(seam)
    rep = base.copy()
    rep[rs.choice(L, min(L, 7), replace=False)] = 0.75
    rows.append(rep)
    return np.array(rows)


def cut_rows(L, lncut, seed=0):
    """a row with an entry exactly at m + lncut (excluded) and its nextafter towards m (kept), in a row whose other entries are far
    from the cut"""
    rs = np.random.RandomState(4300 + L + seed)
    r = rs.uniform(-0.5, 0., size=L) * (-lncut) * 0.5      # inside the cut
    r[rs.rand(L) < 0.4] -= 3. * (-lncut)                    # far outside
    m = 0.0                                                  # (at - m is then the cut itself, exactly)
    r[L // 2] = m
    at = m + lncut
    assert at - m == lncut and np.nextafter(at, m) - m > lncut
    r[0] = at
    r[L - 1] = np.nextafter(at, m)
    return r[None, :].copy(), (0, L - 1)
