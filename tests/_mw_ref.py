"""The law of the model-weight sampler (docs/model_weights.md) in NumPy, and the problems tests/test_mw_host.py and
tests/test_hip_mw.py share.

One sweep: the row of object i is t_ij = r_ij + lnw[nbr_ij] (dense rows: nbr_ij = j); its assignment is the posterior draw of
docs/draws.md on t_i with one uniform (tests/_draw_ref.py: draw_ref, and draw_segmented for the device's order); a row without a
posterior (a nan, a max that is not finite, Nneighbors[i] == 0) reports -1 and is left out of the counts; then
pos ~ Dirichlet(alpha + counts), lnw = log(pos).  `chain_host` is the draws='host' chain with NumPy's own generator."""
import numpy as np

import _draw_ref as dr

NEAR_REL = 1e-12                # a device row is the same fp64 add: only the summation order differs (dr.SUM_TOL)


def added_rows(rows, lnw, neighbors=None, nnbr=None):
    """t = r + lnw[nbr]; entries past nnbr[i] (the k-NN padding, -99) are never looked up and keep the row's own value"""
    rows, lnw = np.asarray(rows, dtype=np.float64), np.asarray(lnw, dtype=np.float64)
    with np.errstate(invalid='ignore'):
        if neighbors is None:
            return rows + lnw[None, :]
        valid = np.arange(rows.shape[1])[None, :] < np.asarray(nnbr)[:, None]
        return np.where(valid, rows + lnw[np.where(valid, neighbors, 0)], rows)


def sweep_ref(rows, lnw, u, M, neighbors=None, nnbr=None, draw=dr.draw_ref):
    """-> assign (N) int64 (model indices, -1: no posterior), counts (M) int64"""
    t = added_rows(rows, lnw, neighbors, nnbr)
    out = draw(t, np.asarray(u, dtype=np.float64)[:, None], neighbors, nnbr)
    assign = (out[0] if isinstance(out, tuple) else out)[:, 0]
    return assign, np.bincount(assign[assign >= 0], minlength=M).astype(np.int64)


def sweep_dense(rows, lnw, u):
    """sweep_ref on dense rows in one piece (the same sums: np.cumsum along a row is sequential): the long statistical chains"""
    t = added_rows(rows, lnw)
    M = t.shape[1]
    m = t.max(axis=1)
    ok = np.isfinite(m) & ~np.isnan(t).any(axis=1)
    with np.errstate(invalid='ignore'):
        w = np.where(ok[:, None], np.exp(t - m[:, None]), 1.)
    cdf = np.cumsum(w, axis=1)
    j = (cdf <= (np.asarray(u) * cdf[:, -1])[:, None]).sum(axis=1)
    last = M - 1 - np.argmax(w[:, ::-1] > 0, axis=1)
    assign = np.where(ok, np.minimum(j, last), -1).astype(np.int64)
    return assign, np.bincount(assign[assign >= 0], minlength=M).astype(np.int64)


def near_share(rows, lnw, u, neighbors=None, nnbr=None, rel=NEAR_REL):
    """share of the objects whose u tot lies within `rel` tot of a cdf value of the added row"""
    t = added_rows(rows, lnw, neighbors, nnbr)
    return dr.near(t, np.asarray(u)[:, None], rel, nnbr).mean()


def chain_host(rows, M, alpha, pos0, rstate, nsweeps, neighbors=None, nnbr=None, check_near=True):
    """the draws='host' chain: per sweep u = rstate.rand(N), the assignments, pos = rstate.dirichlet(alpha + counts).
    -> counts (nsweeps, M), pos (nsweeps, M), the largest near_share over the sweeps (check_near=False: not looked at, and dense rows
    take sweep_dense)"""
    N = len(rows)
    with np.errstate(divide='ignore'):
        lnw = np.log(np.asarray(pos0, dtype=np.float64))
    cs, ps, worst = [], [], 0.
    for _ in range(nsweeps):
        u = rstate.rand(N)
        if check_near:
            worst = max(worst, near_share(rows, lnw, u, neighbors, nnbr))
        _, c = sweep_ref(rows, lnw, u, M, neighbors, nnbr) if check_near or neighbors is not None else sweep_dense(rows, lnw, u)
        pos = rstate.dirichlet(alpha + c)
        with np.errstate(divide='ignore'):
            lnw = np.log(pos)
        cs.append(c); ps.append(pos)
    return np.array(cs), np.array(ps), worst


def stack_start(rows, M, neighbors=None, nnbr=None):
    """pos_j proportional to sum_i exp(r_ij - logsumexp_j' r_ij'): the sampler's default start"""
    pos = np.zeros(M)
    for i in range(len(rows)):
        r = rows[i] if nnbr is None else rows[i, :nnbr[i]]
        if len(r) == 0 or np.isnan(r).any() or not np.isfinite(r.max()):
            continue
        p = np.exp(r - r.max()); p /= p.sum()
        np.add.at(pos, np.arange(M) if neighbors is None else neighbors[i, :nnbr[i]], p)
    return pos / pos.sum()


# ---- problems ---------------------------------------------------------------------------------------------------------------------
def sparse_problem(N, W, M, seed=0, ragged=True):
    """rows of W ln-likelihoods spanning e^-12 over random distinct neighbours out of M models, Nneighbors ragged (0 included when
    N > 3), padding -99 / -inf as NearestNeighbors.fit leaves it; lnw spanning e^-6 with one model at weight 0"""
    rs = np.random.RandomState(2300 + 7 * N + 3 * W + M + seed)
    rows = -rs.uniform(0., 12., size=(N, W))
    nbr = np.stack([rs.permutation(M)[:W] if W <= M else rs.randint(0, M, W) for _ in range(N)]).astype(np.int64)
    nnbr = np.full(N, W, dtype=np.int64)
    if ragged:
        nnbr = rs.randint(max(1, W // 2), W + 1, N).astype(np.int64)
        if N > 3:
            nnbr[3] = 0
    for i in range(N):
        rows[i, nnbr[i]:] = -np.inf; nbr[i, nnbr[i]:] = -99
    lnw = -rs.uniform(0., 6., M)
    lnw[M // 2] = -np.inf
    return rows, nbr, nnbr, lnw, rs.rand(N)


def chain_problem(tag):
    """host-made chain problems of the draws='host' tests: (rows, neighbors, nnbr, M, alpha, seed)"""
    if tag == 'sparse20':
        rows, nbr, nnbr, _, _ = sparse_problem(53, 20, 300, seed=1)
        return rows, nbr, nnbr, 300, np.full(300, 0.5), 2311
    if tag == 'sparse600':
        rows, nbr, nnbr, _, _ = sparse_problem(41, 600, 900, seed=2)
        return rows, nbr, nnbr, 900, np.ones(900), 2312
    raise KeyError(tag)


CHAIN_TAGS = ('sparse20', 'sparse600')
CHAIN_SWEEPS = 40


def golden_chain_check(smp, ref, N):
    """per-model means within 5 batch-means sigma of the reference's chain (the bar of G16); models the reference gives fewer than 10
    objects are pooled"""
    from test_nz_samplers_host import batch_means
    mean, se = batch_means(smp)
    rmean, rse = batch_means(ref)
    rare = rmean * N < 10
    dev = np.abs(mean - rmean) / np.sqrt(se**2 + rse**2)
    print('largest per-model deviation %.2f sigma, %d models pooled' % (dev[~rare].max(), rare.sum()))
    assert (dev[~rare] <= 5.).all()
    if rare.any():
        pm, pse = batch_means(smp[:, rare].sum(axis=1))
        rm, rs_ = batch_means(ref[:, rare].sum(axis=1))
        assert abs(pm - rm) <= 5 * np.sqrt(pse**2 + rs_**2) + 10. / N
