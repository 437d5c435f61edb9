"""The law of EM over the model weights (docs/model_weights.md, "EM") in NumPy with `longdouble` sums, and the problems
tests/test_mw_em_host.py and tests/test_hip_mw_em.py share.

One iteration from lnw (= ln w - ln sum w, -inf for an exact zero):
    t_ik  = r_ik + lnw[nbr_ik]                      one fp64 add, the row of tests/_mw_ref.py: added_rows
    ell_i = logsumexp_k t_ik over the counted entries; a row without a posterior (a nan, a max that is not finite, Nneighbors[i] == 0,
            the rule of _mw_ref / _draw_ref) is skipped: it adds to nothing and is counted in nskip
    lnpost = sum_i ell_i + sum_{j: alpha_j != 1} (alpha_j - 1) lnw_j
    c_j   = sum of exp(t_ik - ell_i) over the counted entries with nbr_ik = j
    a_j   = c_j + (alpha_j - 1);  pos = a / sum(a);  lnw' = ln a - ln sum(a)
`dtype=np.float64, order=RandomState` is the fp64 restatement with the entries added in a random order: what any fp64 realisation
of the law may differ by."""
import numpy as np

import _mw_ref as mw

U = 2.0 ** -53
EPS_EXP = 2.0 ** -52            # the device library's fp64 exp: 1 ulp
FLOOR = 1e-290


def entries(rows, M, neighbors=None, nnbr=None):
    """the counted entries in (i, k) order -> obj (E), k (E), model (E)"""
    N, W = rows.shape
    if neighbors is None:
        valid = np.ones((N, W), dtype=bool)
        nb = np.broadcast_to(np.arange(W)[None, :], (N, W))
    else:
        valid = np.arange(W)[None, :] < np.asarray(nnbr)[:, None]
        nb = neighbors
    i, k = np.nonzero(valid)
    return i, k, np.asarray(nb)[i, k].astype(np.int64)


def lnw_of(w):
    """ln w - ln sum(w) with the library's fixed-order sum"""
    from frankenz_amd.samplers import _mw_em_lnw
    return _mw_em_lnw(w, len(w))


def row_pass(rows, lnw, neighbors=None, nnbr=None, dtype=np.longdouble):
    """-> t (N, W) fp64 (padding -inf), ell (N) `dtype` (nan: skipped), counted (N) bool"""
    rows = np.asarray(rows, dtype=np.float64)
    N, W = rows.shape
    t = mw.added_rows(rows, lnw, neighbors, nnbr)
    if nnbr is not None:
        t = np.where(np.arange(W)[None, :] < np.asarray(nnbr)[:, None], t, -np.inf)
    with np.errstate(invalid='ignore', over='ignore'):
        m = np.where(np.isnan(t).any(axis=1), np.nan, t.max(axis=1, initial=-np.inf))
        ok = np.isfinite(m)
        ms = np.where(ok, m, 0.)
        s = np.exp((t - ms[:, None]).astype(dtype)).sum(axis=1, dtype=dtype)
        ell = np.where(ok, ms.astype(dtype) + np.log(np.where(ok, s, 1)), np.nan)
    return t, ell, ok


def step(rows, lnw, M, alpha=None, neighbors=None, nnbr=None, dtype=np.longdouble, order=None):
    """one iteration -> dict(ell, counted, nskip, lnlike, lnpost, c, a, pos, lnw, t, obj, model)"""
    alpha = np.ones(M) if alpha is None else np.asarray(alpha, dtype=np.float64)
    lnw = np.asarray(lnw, dtype=np.float64)
    t, ell, ok = row_pass(rows, lnw, neighbors, nnbr, dtype)
    i, k, j = entries(np.asarray(rows), M, neighbors, nnbr)
    keep = ok[i]
    i, k, j = i[keep], k[keep], j[keep]
    te = t[i, k]
    with np.errstate(under='ignore'):
        rho = np.exp(te.astype(dtype) - ell[i])
    if order is not None:
        perm = order.permutation(len(rho))
        i, k, j, te, rho = i[perm], k[perm], j[perm], te[perm], rho[perm]
    c = np.zeros(M, dtype=dtype)
    np.add.at(c, j, rho)
    ells = ell[ok]
    if order is not None:
        ells = ells[order.permutation(len(ells))]
    lnlike = ells.sum(dtype=dtype) if order is None else np.add.reduce(ells, dtype=dtype)
    pr = alpha != 1.
    with np.errstate(invalid='ignore'):
        lnpost = lnlike + ((alpha[pr] - 1.).astype(dtype) * lnw[pr].astype(dtype)).sum(dtype=dtype)
    a = c + (alpha - 1.).astype(dtype)
    tot = a.sum(dtype=dtype)
    if not tot > 0:
        raise RuntimeError("no object has a posterior under these weights")
    with np.errstate(divide='ignore'):
        out_lnw = np.log(a) - np.log(tot)
    return dict(ell=ell, counted=ok, nskip=int((~ok).sum()), lnlike=lnlike, lnpost=lnpost, c=c, a=a, pos=a / tot, lnw=out_lnw, t=te, obj=i,
                model=j)


def iterate(rows, lnw, M, niter, alpha=None, neighbors=None, nnbr=None, dtype=np.longdouble, order=None):
    """niter iterations; the weights go from one to the next as fp64 ln-weights (what the device hands on) -> (pos, trace (niter))"""
    trace = []
    for _ in range(niter):
        s = step(rows, lnw, M, alpha, neighbors, nnbr, dtype, order)
        trace.append(float(s['lnpost']))
        lnw = np.asarray(s['lnw'], dtype=np.float64)
    return np.asarray(s['pos'], dtype=np.float64), np.array(trace), s


def lnpost_bar(N, ell):
    """what rounding may take from a sum of N terms ell_i in any order, with room for the terms' own rounding"""
    e = np.asarray(ell, dtype=np.float64)
    return 4. * (np.log2(max(N, 2)) + 8.) * U * np.abs(e[np.isfinite(e)]).sum()


def count_bars(s, M):
    """per model the relative bar of the one-step comparison: 4 (len_j u + max_e(|t_e| + |ell_i| + |t_e - ell_i|) u + eps_exp)"""
    ell = np.asarray(s['ell'], dtype=np.float64)[s['obj']]
    arg = np.abs(s['t']) + np.abs(ell) + np.abs(s['t'] - ell)
    arg = np.where(np.isfinite(arg), arg, 0.)                        # an entry at -inf is an exact zero on both sides
    worst = np.zeros(M)
    np.maximum.at(worst, s['model'], arg)
    length = np.bincount(s['model'], minlength=M)
    return 4. * (length * U + worst * U + EPS_EXP)


# ---- problems ---------------------------------------------------------------------------------------------------------------------
def em_problem(N, W, M, seed=0):
    """_mw_ref.sparse_problem with weights that hold exact zeros and values down to 1e-200"""
    rows, nbr, nnbr, _, _ = mw.sparse_problem(N, W, M, seed=seed)
    rs = np.random.RandomState(4100 + N + 3 * W + M + seed)
    w = rs.uniform(0.1, 1., M)
    w[rs.rand(M) < 0.1] = 0.
    small = rs.rand(M) < 0.1
    w[small] *= 10. ** -rs.uniform(20., 200., small.sum())
    if not w.sum() > 0.:
        w[0] = 1.
    return rows, nbr, nnbr, w


def column_problem(lengths, N, seed=0):
    """sparse rows in which model j is listed by exactly lengths[j] objects (at most once per object): columns of given lengths"""
    rs = np.random.RandomState(4200 + len(lengths) + N + seed)
    M = len(lengths)
    lists = [[] for _ in range(N)]
    for j, n in enumerate(lengths):
        assert n <= N
        for i in (rs.permutation(N)[:n] if n < N else range(N)):
            lists[i].append(j)
    W = max(1, max(len(l) for l in lists))
    nbr = np.full((N, W), -99, dtype=np.int64); rows = np.full((N, W), -np.inf); nnbr = np.zeros(N, dtype=np.int64)
    for i, l in enumerate(lists):
        l = list(rs.permutation(l))
        nnbr[i] = len(l); nbr[i, :len(l)] = l; rows[i, :len(l)] = -rs.uniform(0., 12., len(l))
    return rows, nbr, nnbr, M
