"""EM over the model weights on the GPU (csrc/fz_mw_em.h, docs/model_weights.md "EM"): the row pass against fz_draw_logwt on host-formed
rows, the inverted index against NumPy's stable argsort, one step and 60 iterations against the `longdouble` law of
tests/_mw_em_ref.py, the bit-for-bit properties and the Python surface.  tests/test_mw_em_host.py shows what an fp64 realisation of the
law may differ from the `longdouble` one by (1e-13 relative, measured 2.5e-14): the bars here rest on that."""
import functools

import numpy as np
import pytest

import _draw_ref as dr
import _mw_em_ref as em
import _mw_ref as mw
from conftest import DevArray, load_golden

pytestmark = pytest.mark.gpu

CSEG = 1024                     # FZ_MW_EM_CSEG: entries of a column segment


def engine():
    from frankenz_amd.engine import get_engine
    return get_engine()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def gpu_loglike(rows, lnw, M, nbr=None, nnbr=None):
    ell = np.full(len(rows), -7.)
    lnlike, nskip = engine().mw_loglike(rows, rows.shape[0], rows.shape[1], M, lnw, neighbors=nbr, nnbr=nnbr, ell=ell)
    return ell, lnlike, nskip


def gpu_levid(t, nbr=None, nnbr=None):
    idx, levid = np.empty((len(t), 1), dtype=np.int64), np.empty(len(t))
    engine().draw_logwt(t, 1, idx, u=np.zeros((len(t), 1)), neighbors=nbr, nnbr=nnbr, levid=levid)
    return levid


class Problem(object):
    """device-resident rows and (sparse rows) their index"""

    def __init__(self, rows, M, nbr=None, nnbr=None):
        from frankenz_amd.engine import DeviceArray
        eng = engine()
        self.N, self.W = rows.shape
        self.M = M
        self.rows, self.nbr, self.nnbr = eng.device_array(rows), None, None
        self.E, self.index = 0, None
        if nbr is not None:
            self.nbr, self.nnbr = eng.device_array(nbr), eng.device_array(nnbr)
            self.E, self.nbytes = eng.mw_em_index_bytes(self.N, self.W, M, nnbr)
            assert self.E == int(nnbr.sum()) and self.nbytes == 8 * (M + 1) + 12 * self.E
            assert eng.mw_em_index_bytes(self.N, self.W, M, self.nnbr) == (self.E, self.nbytes)
            self.build()

    def build(self):
        from frankenz_amd.engine import DeviceArray
        eng, E = engine(), self.E
        self.index = (DeviceArray(eng, (self.M + 1,), np.int64), DeviceArray(eng, (max(E, 1),), np.int32), DeviceArray(eng, (max(E, 1),), np.float64))
        eng.mw_em_index(self.rows, self.N, self.W, self.M, self.nbr, self.nnbr, E, *self.index)
        return self.host_index()

    def host_index(self):
        co, cj, cv = self.index
        return co.numpy(), cj.numpy()[:self.E], cv.numpy()[:self.E]

    def em(self, lnw, alpha=None, niter=1):
        M = self.M
        alpha = np.ones(M) if alpha is None else alpha
        lnw = np.array(lnw, dtype=np.float64)
        pos, c, trace, nskip = np.empty(M), np.empty(M), np.empty(niter), np.empty(niter, dtype=np.int64)
        engine().mw_em(self.rows, self.N, self.W, M, alpha, lnw, niter, pos, c, trace, nskip, neighbors=self.nbr, nnbr=self.nnbr, index=self.index,
                       entries=self.E)
        return pos, c, trace, nskip, lnw


# ---- the row pass -------------------------------------------------------------------------------------------------------------------
def edge_problem(N, W, seed=0):
    """_mw_ref.sparse_problem (ragged Nneighbors, 0 on object 3, one model at weight 0) with, by object index: -inf in whole segments
    (1), a nan (2), every neighbour at weight 0 (4), a +inf entry (5)"""
    M = W + 57
    rows, nbr, nnbr, lnw, _ = mw.sparse_problem(N, W, M, seed=seed)
    lnw = lnw.copy()
    if N > 1 and W > 300:
        rows[1, :256] = -np.inf
        rows[1, 512:min(nnbr[1] - 1, 4000)] = -np.inf
    if N > 2 and nnbr[2] > 1:
        rows[2, nnbr[2] // 2] = np.nan
    if N > 4:
        lnw[nbr[4, :nnbr[4]]] = -np.inf
    if N > 5:
        rows[5, 0] = np.inf
    return rows, nbr, nnbr, lnw, M


def check_row_pass(rows, lnw, M, nbr=None, nnbr=None):
    t = mw.added_rows(rows, lnw, nbr, nnbr)
    ell, lnlike, nskip = gpu_loglike(rows, lnw, M, nbr, nnbr)
    levid = gpu_levid(t, nbr, nnbr)
    _, _, counted = em.row_pass(rows, lnw, nbr, nnbr)
    np.testing.assert_array_equal(np.isnan(ell), ~counted)                                      # nan marks a skipped row, and only that
    np.testing.assert_array_equal(bits(ell[counted]), bits(levid[counted]))                    # bit for bit
    assert not np.isfinite(levid[~counted]).any()
    assert nskip == (~counted).sum()
    ref = float(ell[counted].astype(np.longdouble).sum())
    assert abs(lnlike - ref) <= em.lnpost_bar(len(rows), ell)
    return ell, lnlike, nskip


@pytest.mark.parametrize('W', [1, 3, 255, 256, 257, 1024, 1025, 4096, 4097])
def test_row_pass_is_the_levid_of_the_pre_added_rows(W):
    for N in (1, 4, 5, 1027):
        rows, nbr, nnbr, lnw, M = edge_problem(N, W)
        ell, _, nskip = check_row_pass(rows, lnw, M, nbr, nnbr)
        if N > 5:
            assert np.isnan(ell[[3, 4, 5]]).all() and (W == 1 or np.isnan(ell[2])) and nskip >= 3


def test_row_pass_on_dense_rows_of_70001_models():
    rs = np.random.RandomState(4301)
    N, M = 3, 70001
    rows = -rs.uniform(0., 12., size=(N, M)); lnw = -rs.uniform(0., 6., M)
    rows[1, 256:5000] = -np.inf
    lnw[rs.rand(M) < 0.3] = -np.inf
    check_row_pass(rows, lnw, M)


@pytest.mark.parametrize('W', [3, 513, 1024, 4097])
def test_forced_geometries_and_the_re_reading_form_give_the_same_bits(W, monkeypatch):
    rows, nbr, nnbr, lnw, M = edge_problem(37, W, seed=3)
    ref = gpu_loglike(rows, lnw, M, nbr, nnbr)
    for name, val in (('FZ_DRAW_WPO', '1'), ('FZ_DRAW_WPO', '4'), ('FZ_MW_REG', '0')):
        monkeypatch.setenv(name, val)
        got = gpu_loglike(rows, lnw, M, nbr, nnbr)
        monkeypatch.delenv(name)
        np.testing.assert_array_equal(bits(got[0]), bits(ref[0]))
        assert bits(got[1]) == bits(ref[1]) and got[2] == ref[2]


# ---- the index ----------------------------------------------------------------------------------------------------------------------
def twice_problem():
    """model 2 listed twice by object 1, three times by object 4; models 0 and 6 listed by nobody"""
    nbr = np.array([[1, 2, 3, -99], [2, 5, 2, -99], [4, -99, -99, -99], [-99] * 4, [2, 2, 2, 7]], dtype=np.int64)
    nnbr = np.array([3, 3, 1, 0, 4], dtype=np.int64)
    rows = -np.random.RandomState(9).uniform(0., 5., size=nbr.shape)
    rows[np.arange(4)[None, :] >= nnbr[:, None]] = -np.inf
    return rows, nbr, nnbr, 8


@functools.lru_cache(maxsize=None)
def index_case(tag):
    """-> rows, nbr, nnbr, M (read-only)"""
    if tag.startswith('M'):
        M = int(tag[1:])
        rows, nbr, nnbr, _, _ = mw.sparse_problem(41, min(M, 9) if M > 1 else 1, M, seed=5)
    elif tag == 'lengths':
        rows, nbr, nnbr, M = em.column_problem([0, 1, 63, 64, 65, CSEG - 1, CSEG, CSEG + 1, 0, 7], CSEG + 3)
    elif tag == 'everyrow':
        rows, nbr, nnbr, M = em.column_problem([4099, 5, 0, 70], 4099)
    elif tag == 'twice':
        rows, nbr, nnbr, M = twice_problem()
    elif tag == 'repeats':                                          # W > M: neighbours drawn with repetition
        rows, nbr, nnbr, _, _ = mw.sparse_problem(53, 20, 7, seed=6)
        M = 7
    elif tag == 'empty':
        rows, nbr, nnbr, _, _ = mw.sparse_problem(9, 5, 30, seed=7)
        nnbr = np.zeros_like(nnbr)
        M = 30
    else:
        raise KeyError(tag)
    for a in (rows, nbr, nnbr):
        a.setflags(write=False)
    return rows, nbr, nnbr, M


INDEX_TAGS = ['M1', 'M63', 'M64', 'M65', 'M70001', 'lengths', 'everyrow', 'twice', 'repeats', 'empty']


@pytest.mark.parametrize('tag', INDEX_TAGS)
def test_index_is_the_stable_sort_by_model(tag):
    rows, nbr, nnbr, M = index_case(tag)
    p = Problem(rows, M, nbr, nnbr)
    col_off, col_obj, col_val = p.host_index()
    i, k, j = em.entries(rows, M, nbr, nnbr)
    order = np.argsort(j, kind='stable')
    np.testing.assert_array_equal(col_off, np.concatenate(([0], np.cumsum(np.bincount(j, minlength=M)))))
    np.testing.assert_array_equal(col_obj, i[order])
    np.testing.assert_array_equal(bits(col_val), bits(rows[i, k][order]))
    if tag == 'lengths':
        np.testing.assert_array_equal(np.diff(col_off), [0, 1, 63, 64, 65, CSEG - 1, CSEG, CSEG + 1, 0, 7])
    again = p.build()                                                                          # built twice: identical
    for a, b in zip(again, (col_off, col_obj, col_val)):
        np.testing.assert_array_equal(a.view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


# ---- one step -----------------------------------------------------------------------------------------------------------------------
def case_weights(M, seed):
    """weights with exact zeros and values down to 1e-200"""
    rs = np.random.RandomState(4400 + M + seed)
    w = rs.uniform(0.1, 1., M)
    if M > 2:
        w[rs.rand(M) < 0.1] = 0.
        small = rs.rand(M) < 0.1
        w[small] *= 10. ** -rs.uniform(20., 200., small.sum())
    if not w.max() > 0.1:
        w[0] = 1.
    return w


def assert_step(got, ref, N, M):
    """the one-step bar: per model 4 (len_j u + max_e(|t_e| + |ell_i| + |t_e - ell_i|) u + eps_exp) relative on c, + 8 u on pos, floor
    1e-290; lnpost within the bar of a sum of N terms; counts.sum() within N u (relative: the bound of a sum of N terms) of N - nskip"""
    pos, c, trace, nskip = got[:4]
    bars = em.count_bars(ref, M)
    cr, pr = np.asarray(ref['c'], dtype=np.float64), np.asarray(ref['pos'], dtype=np.float64)
    dc, dp = np.abs(c - cr) - em.FLOOR, np.abs(pos - pr) - em.FLOOR
    print('worst c: %.2f of its bar; worst pos: %.2f of its bar' % (np.max(dc / np.maximum(bars * cr, 1e-300)), np.max(dp / np.maximum((bars + 8 * em.U) * pr, 1e-300))))
    assert (dc <= bars * cr).all()
    assert (dp <= (bars + 8 * em.U) * pr).all()
    assert nskip[0] == ref['nskip']
    lp = float(ref['lnpost'])
    if np.isfinite(lp):
        assert abs(trace[0] - lp) <= em.lnpost_bar(N, ref['ell']) + 4 * em.U * abs(lp - float(ref['lnlike'])) * (np.log2(M) + 8)
    else:
        assert trace[0] == lp
    kept = N - ref['nskip']
    assert abs(c.sum() - kept) <= N * em.U * kept


@pytest.mark.parametrize('alpha', [1.0, 1.5])
@pytest.mark.parametrize('tag', [t for t in INDEX_TAGS if t != 'empty'])
def test_one_step_against_the_longdouble_law(tag, alpha):
    rows, nbr, nnbr, M = index_case(tag)
    lnw = em.lnw_of(case_weights(M, 1))
    al = np.full(M, alpha)
    ref = em.step(rows, lnw, M, al, nbr, nnbr)
    got = Problem(rows, M, nbr, nnbr).em(lnw, al)
    assert_step(got, ref, len(rows), M)
    zero = np.isneginf(lnw)
    if alpha == 1.0:
        assert (got[0][zero] == 0.).all() and np.isneginf(got[4][zero]).all()                  # a weight of 0 stays 0


def test_one_step_on_dense_rows_and_on_permuted_objects():
    rows = np.ascontiguousarray(load_golden('g22_model_weights')['lnlike'], dtype=np.float64)
    N, M = rows.shape
    lnw = em.lnw_of(case_weights(M, 2))
    ref = em.step(rows, lnw, M)
    assert_step(Problem(rows, M).em(lnw), ref, N, M)
    rs = np.random.RandomState(3)
    big = -rs.uniform(0., 12., size=(2051, 130)); big[7, 5] = np.nan                           # more than one strip of rows and of columns
    lnw = em.lnw_of(case_weights(130, 3))
    assert_step(Problem(big, 130).em(lnw, np.full(130, 1.5)), em.step(big, lnw, 130, np.full(130, 1.5)), 2051, 130)
    # a permutation of the objects changes the order of every column: not bitwise, held to the one-step bar
    rows, nbr, nnbr, M = index_case('lengths')
    perm = rs.permutation(len(rows))
    lnw = em.lnw_of(case_weights(M, 1))
    assert_step(Problem(rows[perm], M, nbr[perm], nnbr[perm]).em(lnw), em.step(rows, lnw, M, None, nbr, nnbr), len(rows), M)


# ---- iterations ---------------------------------------------------------------------------------------------------------------------
def knn_rows(K, k):
    from frankenz_amd import NearestNeighbors
    X, Xe, Xm, Y, Ye, Ym, _ = dr.knn_problem(K, k)
    nn = NearestNeighbors(Y, Ye, Ym, K=K, rstate=np.random.RandomState(1), verbose=False)
    nn.fit(X.copy(), Xe.copy(), Xm.copy(), rstate=np.random.RandomState(44), k=k, verbose=False)
    return nn


def sparse_fits():
    from frankenz_amd import BruteForce
    rs = np.random.RandomState(31)
    X, Xe, Xm, Y, Ye, Ym = dr.photometry(rs, 37, 1500, 5)
    return BruteForce(Y, Ye, Ym).fit_sparse(X.copy(), Xe.copy(), Xm.copy(), Nkeep=65, verbose=False)


@functools.lru_cache(maxsize=None)
def fitted(tag):
    """-> (fitter or None, rows, nbr, nnbr, M)"""
    if tag == 'g22':
        rows = np.ascontiguousarray(load_golden('g22_model_weights')['lnlike'], dtype=np.float64)
        return None, rows, None, None, rows.shape[1]
    f = knn_rows(5, 4) if tag == 'knn20' else knn_rows(25, 24) if tag == 'knn600' else sparse_fits()
    return f, np.array(f.fit_lnlike), np.array(f.neighbors), np.array(f.Nneighbors), f.NMODEL


ITER_TAGS = ['knn20', 'knn600', 'sparse', 'g22']
ITER_BAR = 1e-11                # 225 x the 4.4e-14 the fp64 NumPy restatement itself moves in 60 iterations (tests/test_mw_em_host.py)


@pytest.mark.parametrize('alpha', [1.0, 1.5])
@pytest.mark.parametrize('tag', ITER_TAGS)
def test_sixty_iterations_stay_with_the_longdouble_law(tag, alpha):
    f, rows, nbr, nnbr, M = fitted(tag)
    if tag == 'knn600':
        assert rows.shape[1] == 600
    al, lnw0 = np.full(M, alpha), np.full(M, -np.log(float(M)))
    rpos, rtrace, last = em.iterate(rows, lnw0, M, 60, al, nbr, nnbr)
    pos, c, trace, nskip, lnw = Problem(rows, M, nbr, nnbr).em(lnw0, al, niter=60)
    rel = np.abs(pos - rpos) / np.maximum(rpos, em.FLOOR)
    rel[np.abs(pos - rpos) <= em.FLOOR] = 0.
    bar = em.lnpost_bar(len(rows), last['ell'])
    print('%s alpha %.1f: worst weight %.2e relative (bar %.0e); smallest increase %+.2e nats (bar %.2e)' % (tag, alpha, rel.max(), ITER_BAR,
                                                                                                         np.diff(trace).min(), bar))
    assert rel.max() <= ITER_BAR
    assert np.diff(trace).min() >= -bar
    assert np.abs(trace - rtrace).max() <= bar
    assert abs(pos.sum() - 1.) <= 4 * M * em.U


# ---- one function of its inputs, bit for bit -----------------------------------------------------------------------------------------
def test_n_iterations_are_n_calls_and_host_rows_equal_device_rows():
    from frankenz_amd import model_weight_em
    rows, nbr, nnbr, _, M = edge_problem(1027, 257, seed=4)                                    # 2 MiB of rows (the smallest limit is 1 MiB)
    alpha = np.full(M, 1.25)
    p = Problem(rows, M, nbr, nnbr)
    lnw0 = np.full(M, -np.log(float(M)))
    pos, c, trace, nskip, lnw = p.em(lnw0, alpha, niter=7)
    cur, tr = lnw0, []
    for _ in range(7):
        pos1, c1, t1, n1, cur = p.em(cur, alpha, niter=1)
        tr.append(t1[0])
    for a, b in ((pos, pos1), (c, c1), (lnw, cur), (trace, np.array(tr))):
        np.testing.assert_array_equal(bits(a), bits(b))
    # the Python surface on uploaded NumPy rows, on device arrays, and under a workspace limit that still holds rows and index
    eng = engine()
    a = model_weight_em(rows, neighbors=nbr, Nneighbors=nnbr, Nmodels=M)
    b = model_weight_em(DevArray(rows), neighbors=DevArray(nbr), Nneighbors=DevArray(nnbr), Nmodels=M)
    d = model_weight_em(rows, neighbors=nbr, Nneighbors=nnbr, Nmodels=M)
    a.run(maxiter=7, alpha=alpha, tol=-1., check_every=3, verbose=False)
    b.run(maxiter=7, alpha=alpha, tol=-1., check_every=7, verbose=False)
    old = eng.workspace_limit()
    eng.set_workspace_limit(2 * rows.nbytes + nnbr.nbytes + 4096)
    try:
        d.run(maxiter=7, alpha=alpha, tol=-1., check_every=2, verbose=False)
    finally:
        eng.set_workspace_limit(old)
    for s in (a, b, d):
        assert s.niter == 7 and not s.converged
        np.testing.assert_array_equal(bits(s.pos), bits(pos)); np.testing.assert_array_equal(bits(s.lnw), bits(lnw))
        np.testing.assert_array_equal(bits(s.counts), bits(c)); np.testing.assert_array_equal(bits(s.lnpost_trace), bits(trace))
    assert b._dev[0] is b.lnlike


def test_loglike_on_host_rows_in_chunks_equals_the_resident_call():
    eng = engine()
    rows, nbr, nnbr, lnw, M = edge_problem(1027, 257, seed=4)                                  # 2 MiB of rows
    ref = gpu_loglike(rows, lnw, M, nbr, nnbr)
    dev = gpu_loglike(DevArray(rows), lnw, M, DevArray(nbr), DevArray(nnbr))
    old = eng.workspace_limit()
    eng.set_workspace_limit(1 << 20)
    try:
        got = gpu_loglike(rows, lnw, M, nbr, nnbr)
    finally:
        eng.set_workspace_limit(old)
    for g in (got, dev):
        np.testing.assert_array_equal(bits(g[0]), bits(ref[0]))
        assert bits(g[1]) == bits(ref[1]) and g[2] == ref[2]
    # and the trace of an iteration is that ln-likelihood at alpha = 1
    assert bits(Problem(rows, M, nbr, nnbr).em(lnw)[2][0]) == bits(ref[1])


# ---- the Python surface ---------------------------------------------------------------------------------------------------------------
def test_weight_em_from_the_three_fitters_and_the_stopping_rule():
    from frankenz_amd import BruteForce
    for tag in ('knn20', 'sparse'):
        f, rows, nbr, nnbr, M = fitted(tag)
        e = f.weight_em()
        e.run(maxiter=40, tol=-1., verbose=False)
        assert e.niter == 40 and not e.converged and e.lnpost_trace.shape == (40,)
        e2 = f.weight_em()
        e2.run(maxiter=2000, tol=1e-3, check_every=10, verbose=False)
        inc = np.diff(e2.lnpost_trace)
        assert e2.converged and e2.niter < 2000 and e2.niter % 10 == 0 and (inc[-10:] <= 1e-3).any() and not (inc[:-10] <= 1e-3).any()
        ref = em.iterate(rows, np.full(M, -np.log(float(M))), M, 40, None, nbr, nnbr)[0]
        np.testing.assert_allclose(e.pos, ref, rtol=ITER_BAR, atol=em.FLOOR)
        lnl, ns = e.loglike()
        assert ns == e.nskip_trace[-1] and lnl >= e.lnpost_trace[-1] - 1e-9                  # (alpha = 1: lnpost is the ln-likelihood)
    rs = np.random.RandomState(32)
    X, Xe, Xm, Y, Ye, Ym = dr.photometry(rs, 37, 257, 5)
    bf = BruteForce(Y, Ye, Ym)
    with pytest.raises(ValueError):
        bf.weight_em()
    bf.fit(X.copy(), Xe.copy(), Xm.copy(), verbose=False)
    e = bf.weight_em()
    w, lnpost, counts = e.step(np.ones(257))
    ref = em.step(np.array(bf.fit_lnlike), np.full(257, -np.log(257.)), 257)
    np.testing.assert_allclose(w, np.asarray(ref['pos'], dtype=np.float64), rtol=1e-12, atol=em.FLOOR)
    assert abs(lnpost - float(ref['lnpost'])) <= em.lnpost_bar(37, ref['ell'])


def test_the_em_weights_start_a_chain_and_the_sampler_scores_weights():
    f, rows, nbr, nnbr, M = fitted('knn20')
    e = f.weight_em()
    e.run(maxiter=30, verbose=False)
    s = f.weight_sampler()
    alpha, seed = np.ones(M), 4501
    s.run_mcmc(2, alpha=alpha, pos_init=e.pos, thin=1, rstate=np.random.RandomState(seed), verbose=False, draws='host')
    counts, _, worst = mw.chain_host(rows, M, alpha, e.pos, np.random.RandomState(seed), 1, nbr, nnbr)
    assert worst <= dr.NEAR_CAP
    np.testing.assert_array_equal(s.sweep_counts[0], counts[0])
    assert s.marginal_lnlike() == e.loglike(np.mean(s.samples, axis=0))
    assert s.marginal_lnlike(e.pos) == e.loglike()
    assert e.loglike()[0] >= s.marginal_lnlike()[0]                                             # the maximum explains the catalogue best


def test_logwt_through_predict_and_population_pdfs():
    import frankenz_oracle as fo
    from frankenz_amd import PDFDict
    nn, rows, nbr, nnbr, M = fitted('knn20')
    e = nn.weight_em()
    e.run(maxiter=30, verbose=False)
    lw = e.logwt()
    with np.errstate(divide='ignore'):
        np.testing.assert_array_equal(lw, mw.added_rows(rows, np.log(e.pos), nbr, nnbr))
    rs = np.random.RandomState(2802)
    z, ze = rs.uniform(0.1, 5.9, M), rs.uniform(0.01, 0.2, M)
    grid, sgrid = np.arange(0, 7 + 1e-5, .01), np.linspace(.005, 2, 500)
    pd, od = PDFDict(grid, sgrid), fo.KernelDict(grid, sgrid)
    pdfs = nn.predict(z, ze, label_dict=pd, logwt=lw, verbose=False)
    assert pdfs.shape == (len(rows), len(grid))
    live = nnbr > 0
    np.testing.assert_allclose(pdfs[live].sum(axis=1), 1., rtol=1e-9)
    pop = e.population_pdfs(z, ze, label_dict=pd, kde_kwargs={'wt_thresh': 0})
    ref = fo.gauss_kde_dict(od, y=z, y_std=ze, y_wt=e.pos, wt_thresh=0.)
    assert pop.shape == (1, len(grid))
    np.testing.assert_allclose(pop[0], ref / ref.sum(), rtol=1e-8, atol=1e-14)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from frankenz_amd import model_weight_em
    eng = engine()
    rows, nbr, nnbr, M, _, _ = mw.chain_problem('sparse20')
    w = np.ones(M)
    for bad in (M, -1):
        nb = nbr.copy(); nb[7, 2] = bad
        assert nnbr[7] > 2
        with pytest.raises(IndexError):
            model_weight_em(rows, neighbors=nb, Nneighbors=nnbr, Nmodels=M).step(w)
        with pytest.raises(IndexError):
            model_weight_em(rows, neighbors=nb, Nneighbors=nnbr, Nmodels=M).loglike(w)
    nn2 = nnbr.copy(); nn2[5] = rows.shape[1] + 1
    with pytest.raises(IndexError):
        model_weight_em(rows, neighbors=nbr, Nneighbors=nn2, Nmodels=M).step(w)
    with pytest.raises(ValueError):
        model_weight_em(rows, neighbors=nbr, Nneighbors=nnbr, Nmodels=M).step(w, alpha=np.full(M, 0.5))
    # every object skipped at alpha = 1: nothing to normalise
    with pytest.raises(RuntimeError):
        model_weight_em(np.full_like(rows, -np.inf), neighbors=nbr, Nneighbors=nnbr, Nmodels=M).step(w)
    with pytest.raises(RuntimeError):
        model_weight_em(rows, neighbors=nbr, Nneighbors=np.zeros_like(nnbr), Nmodels=M).step(w)
    # ... while alpha > 1 gives the prior's own maximum
    pos, lnpost, counts = model_weight_em(rows, neighbors=nbr, Nneighbors=np.zeros_like(nnbr), Nmodels=M).step(w, alpha=np.full(M, 2.))
    np.testing.assert_allclose(pos, 1. / M, rtol=1e-15)
    assert (counts == 0).all() and abs(lnpost + M * np.log(float(M))) <= 4 * M * em.U * M * np.log(float(M))
    with pytest.raises(NotImplementedError, match='FZ_MW_EM_NMAX'):                            # col_obj is int32
        eng.mw_em_index_bytes(2**31, 5, M, None)
    # the index must fit the workspace limit: the rows (device arrays need no room) do, the index does not
    rows, nbr, nnbr, _, M = edge_problem(1027, 257, seed=4)                                    # an index above the smallest limit, 1 MiB
    w = np.ones(M)
    e = model_weight_em(DevArray(rows), neighbors=DevArray(nbr), Nneighbors=DevArray(nnbr), Nmodels=M)
    need = 8 * (M + 1) + 12 * int(nnbr.sum())
    assert need > (1 << 20)
    old = eng.workspace_limit()
    eng.set_workspace_limit(need - 1)
    try:
        with pytest.raises(MemoryError, match=str(need)):
            e.step(w)
        eng.set_workspace_limit(need)
        e.step(w)
    finally:
        eng.set_workspace_limit(old)
