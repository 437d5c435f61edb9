"""The definition of a posterior draw over the model set (docs/draws.md) in NumPy, and the problems tests/test_draw_host.py and
tests/test_hip_draw.py share.

For one row r[0..L) of ln-weights (L = Nmodel, or Nneighbors[i] on the k-NN route):
    w_j = exp(r_j - max r),  cdf = cumsum(w) (sequential),  tot = cdf[-1]
    a draw with uniform u is  j = #{k : cdf_k <= u tot},  clipped to the last entry with w_j > 0
    a nan among the L entries, or a max that is not finite: -1 for every draw
    on the k-NN route the value is neighbors[i][j];  lmap = max r,  levid = lmap + log(tot)

The device sums the same weights in a fixed segmented order, and its rows come from its own likelihood: a draw whose u tot lies
within `rel` tot of a cdf value may legitimately land on the neighbouring entry.  `near` marks those draws; the host tests assert
that they are at most 1 % of every problem (none, for the problems here), and they are the only draws the GPU tests may leave out
of the index-for-index comparison (`assert_draws`), each still having to land on an entry adjacent in the CDF."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))

TOP = 1.0 - 2.0 ** -53          # the largest uniform below 1
FIT_TOL = 1e-8                  # what the project holds fit_lnprob to: a device row may differ from the oracle's by this much
SUM_TOL = 1e-12                 # rows given bit for bit: only the summation order differs (2^20 entries x 2^-53 is 1.2e-10 at the very worst)
NEAR_CAP = 0.01


def _row(rows, nnbr, i):
    return rows[i] if nnbr is None else rows[i, :nnbr[i]]


def draw_ref(rows, u, neighbors=None, nnbr=None):
    """-> idx (N, S) int64, lmap (N), levid (N)"""
    rows, u = np.asarray(rows, dtype=np.float64), np.asarray(u, dtype=np.float64)
    N, S = u.shape
    idx = np.full((N, S), -1, dtype=np.int64)
    lmap, levid = np.full(N, np.nan), np.full(N, np.nan)
    for i in range(N):
        r = _row(rows, nnbr, i)
        if len(r) == 0:
            lmap[i] = levid[i] = -np.inf
            continue
        if np.isnan(r).any():
            continue
        m = r.max()
        lmap[i] = levid[i] = m
        if not np.isfinite(m):
            continue
        w = np.exp(r - m)
        cdf = np.cumsum(w)
        tot = cdf[-1]
        j = (cdf[None, :] <= (u[i] * tot)[:, None]).sum(axis=1)
        j = np.minimum(j, np.nonzero(w > 0)[0][-1])
        idx[i] = j if neighbors is None else neighbors[i][j]
        levid[i] = m + np.log(tot)
    return idx, lmap, levid


def draw_ref_searchsorted(rows, u, neighbors=None, nnbr=None):
    """the same rule restated: the draw is where u tot would be inserted to the right of equal cdf values, over the entries that hold
    mass only (an entry without mass repeats its predecessor's cdf and can never be the answer)"""
    rows, u = np.asarray(rows, dtype=np.float64), np.asarray(u, dtype=np.float64)
    idx = np.full(u.shape, -1, dtype=np.int64)
    for i in range(len(u)):
        r = _row(rows, nnbr, i)
        if len(r) == 0 or np.isnan(r).any() or not np.isfinite(r.max()):
            continue
        w = np.exp(r - r.max())
        cdf = np.add.accumulate(w)
        mass = np.nonzero(w > 0)[0]
        pos = np.searchsorted(cdf[mass], u[i] * cdf[-1], side='right')
        j = mass[np.minimum(pos, len(mass) - 1)]
        idx[i] = j if neighbors is None else neighbors[i][j]
    return idx


def draw_segmented(rows, u, neighbors=None, nnbr=None):
    """The device's arithmetic (csrc/fz_draw.h) restated: 256-entry segments, per segment its own max m_k, e = exp(r - m_k), four
    entries per lane summed in order, the lanes' sums scanned Hillis-Steele, S_k the last running sum; f_k = exp(m_k - m),
    P_k = P_{k-1} + S_k f_k in order; a draw takes the first segment with P_k > u tot and in it the first entry with
    P_{k-1} + (scan + running sum) f_k > u tot that holds mass, else the last entry with mass."""
    rows, u = np.asarray(rows, dtype=np.float64), np.asarray(u, dtype=np.float64)
    idx = np.full(u.shape, -1, dtype=np.int64)
    for i in range(len(u)):
        r = _row(rows, nnbr, i)
        if len(r) == 0 or np.isnan(r).any() or not np.isfinite(r.max()):
            continue
        nseg = (len(r) + 255) // 256
        pad = np.full(nseg * 256, -np.inf); pad[:len(r)] = r
        seg = pad.reshape(nseg, 64, 4)
        mk = seg.max(axis=(1, 2))
        with np.errstate(invalid='ignore'):
            e = np.where(np.isfinite(mk)[:, None, None], np.exp(seg - mk[:, None, None]), 0.)
        p = np.zeros_like(e); p[:, :, 0] = e[:, :, 0]
        for t in range(1, 4):
            p[:, :, t] = p[:, :, t - 1] + e[:, :, t]
        incl = p[:, :, 3].copy()
        d = 1
        while d < 64:
            nxt = incl.copy(); nxt[:, d:] = incl[:, d:] + incl[:, :-d]; incl = nxt; d *= 2
        x = np.zeros_like(incl); x[:, 1:] = incl[:, :-1]
        f = np.exp(mk - r.max())
        mass = (x[:, 63] + p[:, 63, 3]) * f
        P = np.zeros(nseg); acc = 0.
        for k in range(nseg):
            acc += mass[k]; P[k] = acc
        tot = P[-1]
        for s in range(u.shape[1]):
            t = u[i, s] * tot
            k = int(np.searchsorted(P, t, side='right'))
            top = k == nseg
            if top:
                k = int(np.nonzero(f > 0)[0][-1])
            cum = ((P[k - 1] if k else 0.) + (x[k][:, None] + p[k]) * f[k]).ravel()
            pos = (e[k] * f[k] > 0).ravel()
            hit = np.nonzero(pos & (cum > t))[0]
            j = k * 256 + (hit[0] if len(hit) and not top else np.nonzero(pos)[0][-1])
            idx[i, s] = j if neighbors is None else neighbors[i][j]
    return idx


def near(rows, u, rel, nnbr=None):
    """(N, S) bool: u tot within rel tot of the cdf of an entry that holds mass.  The two ends of the unit interval are exact by
    construction and are not marked: u = 0 gives the first entry with mass whatever the sums are, and u = TOP gives the last one as
    long as that entry outweighs the rounding of tot by far (asserted here)."""
    rows, u = np.asarray(rows, dtype=np.float64), np.asarray(u, dtype=np.float64)
    out = np.zeros(u.shape, dtype=bool)
    for i in range(len(u)):
        r = _row(rows, nnbr, i)
        if len(r) == 0 or np.isnan(r).any() or not np.isfinite(r.max()):
            continue
        w = np.exp(r - r.max())
        cdf = np.cumsum(w)
        tot = cdf[-1]
        mass = np.nonzero(w > 0)[0]
        if (u[i] >= TOP).any():
            assert w[mass[-1]] > 1e-10 * tot
        c = cdf[mass]
        t = u[i] * tot
        pos = np.clip(np.searchsorted(c, t), 1, len(c) - 1) if len(c) > 1 else np.zeros(len(t), dtype=int)
        d = np.minimum(np.abs(c[pos] - t), np.abs(c[pos - 1] - t)) if len(c) > 1 else np.abs(c[0] - t)
        out[i] = (d <= rel * tot) & (u[i] > 0.0) & (u[i] < TOP)
    return out


def assert_draws(got, ref, rows, close, neighbors=None, nnbr=None):
    """index for index outside `close`; a close draw lands on an entry with mass next to the reference's in the CDF"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == np.int64
    np.testing.assert_array_equal(got[~close], ref[~close])
    for i, s in zip(*np.nonzero(close & (got != ref))):
        r = _row(rows, nnbr, i)
        mass = list(np.nonzero(np.exp(r - r.max()) > 0)[0])
        val = (lambda j: j) if neighbors is None else (lambda j: neighbors[i][j])
        where = [k for k, j in enumerate(mass) if val(j) == ref[i, s]]
        assert any(val(mass[k2]) == got[i, s] for k in where for k2 in (k - 1, k + 1) if 0 <= k2 < len(mass)), (i, s)


# ---- hand-made rows: (L, S, N) ------------------------------------------------------------------------------------------------
HAND_CASES = [(1, 1, 1), (63, 63, 3), (64, 64, 37), (65, 65, 3), (255, 257, 1), (256, 64, 37), (257, 63, 3), (513, 257, 37),
              (70001, 65, 3), (257, 1, 37)]


def hand_rows(L, S, N, seed=0):
    """rows whose weights span e^-12 (every entry with mass outweighs SUM_TOL tot by far), with by row index: -inf at both ends, -inf
    in whole 256-entry segments, the last entry as the only mass, weights that underflow to 0 (800 below the max); and uniforms with
    u = 0 in the first column of even rows and u = TOP in the last column of odd rows (of every row when S > 1)"""
    rs = np.random.RandomState(9000 + 7 * L + 3 * S + N + seed)
    rows = -rs.uniform(0., 12., size=(N, L))
    for i in range(N):
        kind = i % 6
        if kind == 1 and L > 10:
            rows[i, :3] = -np.inf; rows[i, -5:] = -np.inf
        elif kind == 2 and L > 300:
            rows[i, :256] = -np.inf; rows[i, 512:min(L - 1, 5000)] = -np.inf
        elif kind == 3 and L > 1:
            rows[i, :-1] = -np.inf
        elif kind == 4 and L > 4:
            rows[i, rs.rand(L) < 0.5] -= 800.
            rows[i, L // 2] = 0.
        elif kind == 5 and L > 300:
            rows[i, 256:] -= 800.                   # whole segments that underflow
    u = rs.rand(N, S)
    u[0::2, 0] = 0.
    if S > 1:
        u[:, -1] = TOP
    else:
        u[1::2, -1] = TOP
    return rows, u


def no_posterior_rows(L=257):
    """an all -inf row, a row with one nan, a row with a +inf, and a sound one"""
    rs = np.random.RandomState(77)
    rows = -rs.uniform(0., 12., size=(4, L))
    rows[0] = -np.inf
    rows[1, L // 3] = np.nan
    rows[2, L - 2] = np.inf
    return rows, rs.rand(4, 5)


# ---- fitted problems: (N, M, S, B, lprob_kwargs as sorted items) ---------------------------------------------------------------
FIT_CASES = [(37, 257, 64, 5, ()),
             (37, 257, 64, 5, (('free_scale', True), ('ignore_model_err', True))),
             (37, 257, 64, 5, (('dim_prior', False),)),
             (5, 65, 257, 5, ()),
             (2, 70001, 65, 5, ()),
             (37, 513, 64, 12, (('free_scale', True),))]


def fit_id(case):
    return '%d-%d-%d-%d-%s' % (case[:4] + ('+'.join(k for k, _ in case[4]) or 'A',))


def photometry(rs, N, M, B):
    """the generator of test_oracle_parity_band_counts without masks, model errors 4 %"""
    sig = rs.uniform(0.3, 3.0, B)
    Y = rs.lognormal(1., 1., size=(M, B)); Ye = 0.04 * Y; Ym = np.ones((M, B))
    X = Y[rs.choice(M, N)] * rs.lognormal(0, .3, N)[:, None] + sig * rs.randn(N, B)
    return X, np.tile(sig, (N, 1)), np.ones((N, B)), Y, Ye, Ym


@functools.lru_cache(maxsize=None)
def fit_problem(case):
    """objects, models, the oracle's ln-posterior rows, the uniforms (drawn after the oracle fit) and the reference draws"""
    import frankenz_oracle as fo
    N, M, S, B, kw = case
    rs = np.random.RandomState(7100 + M + S)
    X, Xe, Xm, Y, Ye, Ym = photometry(rs, N, M, B)
    rows = fo.bruteforce_fit(X.copy(), Xe.copy(), Xm.copy(), Y, Ye, Ym, **dict(kw))['lnprob']
    u = rs.rand(N, S)
    idx, lmap, levid = draw_ref(rows, u)
    for a in (X, Xe, Xm, Y, Ye, Ym, rows, u, idx, lmap, levid):
        a.setflags(write=False)
    return dict(X=X, Xe=Xe, Xm=Xm, Y=Y, Ye=Ye, Ym=Ym, kw=dict(kw), rows=rows, u=u, idx=idx, lmap=lmap, levid=levid)


# ---- problems this module adds (masks, priors, k-NN); each passes the same host check -------------------------------------------
def masked_problem(B, seed=0):
    """masked bands on objects and models (at most one per row), per-model errors"""
    rs = np.random.RandomState(7300 + B + seed)
    N, M, S = 37, 257, 64
    X, Xe, Xm, Y, Ye, Ym = photometry(rs, N, M, B)
    hit = rs.rand(M) < 0.15; Ym[hit, rs.randint(0, B, hit.sum())] = 0
    hit = rs.rand(N) < 0.3; Xm[hit, rs.randint(0, B, hit.sum())] = 0
    return X, Xe, Xm, Y, Ye, Ym, rs.rand(N, S)


def prior_problem(seed=0):
    """the first fitted problem with a ln-prior table of P = 7 rows and a row index, and an interpolated prior on 6 nodes"""
    rs = np.random.RandomState(7400 + seed)
    N, M, S, B = 37, 257, 64, 5
    X, Xe, Xm, Y, Ye, Ym = photometry(rs, N, M, B)
    tab = rs.normal(0., 2., size=(7, M)); prow = rs.randint(0, 7, N)
    vals = rs.uniform(0.05, 1., size=(6, M)); grid = np.linspace(18., 23., 6); coord = rs.uniform(17.5, 23.5, N)
    return X, Xe, Xm, Y, Ye, Ym, tab, prow, vals, grid, coord, rs.rand(N, S)


def knn_problem(K, k, seed=0):
    rs = np.random.RandomState(7500 + K * k + seed)
    N, M, S, B = 37, 700, 64, 5
    X, Xe, Xm, Y, Ye, Ym = photometry(rs, N, M, B)
    return X, Xe, Xm, Y, Ye, Ym, S
