"""The law of the posterior scoring rules (include/frankenz_hip.h, docs/scores.md section 1) restated with NumPy: SciPy's float64 `erf`
of the argument formed as the law's DIVISION `d / sqrt(2 v)` (the kernels multiply by a reciprocal rounded once: an independent route
to the same number), everything else and the sums in `np.longdouble` -- or, for the precondition of the GPU bars, the sums in float64
in index order or in a shuffled order.  The pair sums are formed over tiles of rows so that rows of 4 096 included entries stay in
memory.  Also the inputs that tests/test_scores_host.py and tests/test_hip_scores.py share, built from those of tests/_bins_ref.py."""
import functools

import numpy as np
from scipy.special import erf

import _bins_ref as br
from _bins_ref import LD, U, _row

WIDTHS = (1, 2, 63, 64, 65, 127, 128, 129, 256, 257, 500, 4096)      # both sides of every 64-entry tile of the pair loop
CASES = ((0, False), (0, True), (1, True))                          # (k, zeros) of width_case: M = 7 (k = 0) or 1000, s == 0 among the errors
WIDTH_CASES = tuple((W, k, z) for W in WIDTHS for k, z in CASES)
DENSE = (1, 255, 4096)
DENSE4 = (4097, 70001)                                               # the four-wave form
PCOUNTS = (1, 15, 16, 17, 256)
NMAX = 16384                                                         # FZ_SCORES_NMAX
PI = LD(np.pi)
TILE = 256


def bar_sum(K):
    """the bar of docs/predictive.md section 2, relative to the sum of the absolute terms of a fixed-order sum of K terms"""
    return 4. * (np.asarray(K, dtype=np.float64) / 64. + 16.) * U


def A_G(d, v):
    """A(d, v), G(d, v) of the law, longdouble, elementwise; erf in float64 of the float64 quotient"""
    d, v = np.asarray(d, dtype=LD), np.asarray(v, dtype=LD)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore', under='ignore'):
        z = d / np.sqrt(2 * v)
        e = np.exp(-(z * z))
        A = d * erf(z.astype(np.float64)).astype(LD) + np.sqrt(2 * v / PI) * e
        G = e / np.sqrt(2 * PI * v)
    zero = v == 0
    A = np.where(zero, np.abs(d), A)
    G = np.where(zero, np.where(d == 0, LD(np.inf), LD(0)), G)
    return A, G


def _total(a, dtype, perm):
    """the sum of a 1-D array: longdouble, or float64 in index order (a running sum) or in a shuffled order"""
    a = np.asarray(a).ravel()
    if dtype is LD:
        return a.astype(LD).sum()
    a = a.astype(np.float64)
    if perm is not None:
        a = a[perm.permutation(len(a))]
    return np.cumsum(a)[-1] if len(a) else 0.


def pair_sums(w, y, v, dtype=LD, perm=None):
    """sum_{t<u} w_t w_u (A, G) + 1/2 sum_t w_t^2 (A, G)(0, 2 v_t) -> (SA, SG): each unordered pair once, tile by tile"""
    n = len(w)
    SA, SG = [], []
    for a in range(0, n, TILE):
        b = min(a + TILE, n)
        A, G = A_G(y[a:b, None] - y[None, a:], v[a:b, None] + v[None, a:])
        f = np.triu(np.ones((b - a, n - a), dtype=LD), 1) + 0.5 * np.eye(b - a, n - a, dtype=LD)
        c = (w[a:b, None] * w[None, a:]).astype(dtype).astype(LD) * f
        keep = f > 0
        with np.errstate(invalid='ignore'):
            SA.append((c[keep] * A[keep]).astype(dtype))
            SG.append((c[keep] * G[keep]).astype(dtype))
    return _total(np.concatenate(SA), dtype, perm), _total(np.concatenate(SG), dtype, perm)


def scores_ref(rows, y, s, points, neighbors=None, nnbr=None, wt_thresh=1e-3, dtype=LD, perm=None, pairs=True):
    """points (P,) shared or (N, P) -> dict of float64 arrays: lnpdf, term (the first CRPS term), crps (N, P); spread, sqnorm (N); ninc;
    nskip; and for the bars E (N, P)-free (N,) -- the largest z^2 + |ln s| + |r - m| among the included entries with s > 0, over the
    row's points -- and K1 (N), the counted length.  A >= 0 and G >= 0: the sums of absolute terms ARE term, spread and sqnorm."""
    rows = np.asarray(rows, dtype=np.float64)
    y, s, points = (np.asarray(a, dtype=np.float64) for a in (y, s, points))
    with np.errstate(under='ignore'):
        s = np.where(s * s == 0, 0., s)                              # the law: an error whose square is 0 in float64 is a point mass
    N, W = rows.shape
    P = points.shape[-1]
    out = dict(lnpdf=np.full((N, P), np.nan), term=np.full((N, P), np.nan), crps=np.full((N, P), np.nan), spread=np.full(N, np.nan),
               sqnorm=np.full(N, np.nan), ninc=np.zeros(N, dtype=np.int64), E=np.zeros(N), nskip=0,
               K1=np.full(N, W, dtype=np.int64) if nnbr is None else np.asarray(nnbr, dtype=np.int64).copy())
    for i in range(N):
        got = _row(rows, i, neighbors, nnbr, wt_thresh)
        if got is None:
            out['nskip'] += 1
            continue
        w, j = got
        x = (points if points.ndim == 1 else points[i]).astype(LD)
        yy, ss = y[j].astype(LD), s[j].astype(LD)
        n = len(w)
        out['ninc'][i] = n
        Z = w.sum()
        # ---- the density, in ln space ----
        with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
            z = (x[None, :] - yy[:, None]) / (ss[:, None] * np.sqrt(LD(2)))
            a = np.log(w)[:, None] - z * z - np.log(ss)[:, None]
            a = np.where(ss[:, None] == 0, np.where(x[None, :] == yy[:, None], LD(np.inf), -LD(np.inf)), a)
            am = a.max(axis=0)
            ex = np.where(a == am[None, :], LD(1), np.exp(a - am[None, :]))
            out['lnpdf'][i] = (am + np.log(ex.sum(axis=0)) - np.log(Z) - 0.5 * np.log(2 * PI)).astype(np.float64)
            pos = ss > 0
            if pos.any():
                out['E'][i] = float((z[pos] ** 2 + np.abs(np.log(ss[pos]))[:, None] + np.abs(np.log(w[pos]))[:, None]).max())
        # ---- the first CRPS term ----
        A, _ = A_G(x[None, :] - yy[:, None], (ss * ss)[:, None] + 0 * x[None, :])
        t1 = np.array([_total((w.astype(dtype).astype(LD) * A[:, p]).astype(dtype), dtype, perm) for p in range(P)], dtype=LD) / Z
        out['term'][i] = t1.astype(np.float64)
        if not pairs:
            continue
        SA, SG = pair_sums(w, yy, ss * ss, dtype, perm)
        sp, sq = LD(SA) / Z / Z, 2 * LD(SG) / Z / Z
        if (ss == 0).any():
            sq = LD(np.inf)
        out['spread'][i], out['sqnorm'][i] = float(sp), float(sq)
        out['crps'][i] = (t1 - sp).astype(np.float64)
    return out


def bars(ref, W):
    """the absolute bars of lnpdf (N, 1), term (N, P), spread (N), sqnorm (N) and crps (N, P) of a reference"""
    n = ref['ninc'].astype(np.float64)
    K2 = n * (n + 1.) / 2.
    b = dict(lnpdf=(4. * (W / 64. + 16.) * U + 16. * U * ref['E'])[:, None] * np.ones_like(ref['lnpdf']),
             term=bar_sum(ref['K1'])[:, None] * ref['term'], spread=bar_sum(K2) * ref['spread'], sqnorm=bar_sum(K2) * ref['sqnorm'])
    b['crps'] = b['term'] + b['spread'][:, None]
    return b


def assert_scores(got, ref, W, what, keys=('lnpdf', 'crps', 'spread', 'sqnorm')):
    """every result of `got` against the reference at its bar: nan and +-inf in the same places.  Prints and returns the worst share."""
    b = bars(ref, W)
    worst = 0.
    for k in keys:
        g, r = np.asarray(got[k], dtype=np.float64), ref[k]
        g = g.reshape(r.shape)
        np.testing.assert_array_equal(np.isnan(g), np.isnan(r), err_msg="%s: %s" % (what, k))
        inf = np.isinf(r)
        np.testing.assert_array_equal(g[inf], r[inf], err_msg="%s: %s" % (what, k))
        ok = np.isfinite(r)
        if not ok.any():
            continue
        err, bar = np.abs(g[ok] - r[ok]), b[k][ok]
        share = float(np.max(err / np.maximum(bar, 1e-300)))
        print("%s: %s worst %.3g of its bar" % (what, k, share))
        assert (err <= bar).all(), "%s: %s worst %.3g of its bar" % (what, k, share)
        worst = max(worst, share)
    if 'ninc' in got:
        np.testing.assert_array_equal(got['ninc'], ref['ninc'], err_msg=what)
    return worst


# ---- the inputs of the GPU tests (tests/test_hip_scores.py); tests/test_scores_host.py checks their precondition ---------------------
def with_zeros(y, s, seed):
    """every fifth error 0, and the labels of models 0 and 5 equal where there are that many: equal labels with s == 0"""
    y, s = y.copy(), s.copy()
    s[::5] = 0.
    if len(y) > 5:
        y[5] = y[0]
    return y, s


def points_case(rows, y, nbr, P, seed=0):
    """(N, P) points per object: uniform beyond the labels' range, the first exactly on the label of the object's first entry and the
    second on that of model 0; and the (P,) of object 0 to share"""
    N = rows.shape[0]
    rs = np.random.RandomState(7800 + P + seed)
    x = rs.uniform(-2., 8., size=(N, P))
    first = y[np.clip(nbr[:, 0], 0, len(y) - 1)] if nbr is not None else np.full(N, y[0])
    x[:, 0] = first
    if P > 1:
        x[:, 1] = y[0]
    return x, x[0].copy()


@functools.lru_cache(maxsize=None)
def width_case(W, k, zeros):
    """_bins_ref.width_case (5 rows, counts W, W - 1, 1, 0 and a random one) over M = 7 or 1000, the errors as given or with zeros
    among them, and 3 points per object -> rows, nbr, nnbr, y, s, x"""
    rows, nbr, nnbr, y, s, e = br.width_case(W, k)
    if zeros:
        y, s = with_zeros(y, s, W)
    x, _ = points_case(rows, y, nbr, 3, W + k)
    return rows, nbr, nnbr, y, s, x


@functools.lru_cache(maxsize=None)
def dense_case(M):
    """_bins_ref.dense_case (3 rows) with one truth per object -> rows, y, s, x"""
    rows, y, s, e = br.dense_case(M)
    rs = np.random.RandomState(7850 + M % 977)
    return rows, y, s, rs.uniform(-1., 7., 3)


@functools.lru_cache(maxsize=None)
def dense4_case(M):
    """2 dense rows for the four-wave form: about 600 entries pass the cut, on both sides of every 256-entry stride of the first 2 048
    entries and in the last positions; every other entry lies below it -> rows, y, s, x"""
    rs = np.random.RandomState(7900 + M % 991)
    e = br.edges_case(9, 2)
    y, s = br.labels_case(M, e, 6)
    s[::7] = 0.
    rows = -rs.uniform(8., 30., size=(2, M))                         # below ln(1e-3) = -6.9
    at = np.unique(np.concatenate([np.arange(c - 2, c + 2) for c in range(256, 2049, 256)] + [np.arange(M - 40, M)] +
                                  [rs.randint(0, M, 530)]))
    rows[:, at] = -rs.uniform(0., 6.5, size=(2, len(at)))
    rows[0, M - 1] = 0.
    return rows, y, s, rs.uniform(-1., 7., 2)


@functools.lru_cache(maxsize=None)
def pcount_case(P):
    """5 rows of 65 entries over 1000 models (zeros among the errors) and P points per object -> rows, nbr, nnbr, y, s, x"""
    rows, nbr, nnbr, y, s, e = br.nbins_case(P)
    y, s = with_zeros(y, s, P)
    x, _ = points_case(rows, y, nbr, P, 1)
    return rows, nbr, nnbr, y, s, x


BLOCK_REF, BITS_REF = 6, 12                                        # rows of the two cases below that are held to the reference


@functools.lru_cache(maxsize=None)
def block_case():
    """257 rows of 65 entries over 1000 models and one truth each, for the object counts around a block of four
    -> rows, nbr, nnbr, y, s, x"""
    rows, nbr, nnbr = br.sparse_case(257, 65, 1000, 9, counts=[])
    _, _, _, y, s, _ = width_case(65, 1, True)
    return rows, nbr, nnbr, y, s, np.random.RandomState(9).uniform(-1., 7., 257)


@functools.lru_cache(maxsize=None)
def bits_case():
    """700 rows of 257 entries over 1000 models (zeros among the errors) and 3 points per object, for the bit-for-bit properties
    -> rows, nbr, nnbr, y, s, x"""
    e = br.edges_case(33, 5)
    y, s = br.labels_case(1000, e, 6)
    y, s = with_zeros(y, s, 0)
    rows, nbr, nnbr = br.sparse_case(700, 257, 1000, 4, counts=[])
    return rows, nbr, nnbr, y, s, np.random.RandomState(2).uniform(-1., 7., size=(700, 3))


@functools.lru_cache(maxsize=None)
def ref_cached(kind, *key):
    """scores_ref of a named case, computed once: ('width', W, k, zeros, wt_thresh), ('dense', M), ('dense4', M), ('pcount', P),
    ('block',) and ('bits',): their first BLOCK_REF and BITS_REF rows"""
    if kind in ('block', 'bits'):
        rows, nbr, nnbr, y, s, x = block_case() if kind == 'block' else bits_case()
        n = BLOCK_REF if kind == 'block' else BITS_REF
        return scores_ref(rows[:n], y, s, x[:n].reshape(n, -1), nbr[:n], nnbr[:n])
    if kind == 'width':
        rows, nbr, nnbr, y, s, x = width_case(*key[:3])
        return scores_ref(rows, y, s, x, nbr, nnbr, wt_thresh=key[3])
    if kind == 'pcount':
        rows, nbr, nnbr, y, s, x = pcount_case(*key)
        return scores_ref(rows, y, s, x, nbr, nnbr)
    rows, y, s, x = (dense_case if kind == 'dense' else dense4_case)(*key)
    return scores_ref(rows, y, s, x[:, None])
