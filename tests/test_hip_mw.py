"""Gibbs over model weights on the GPU (csrc/fz_mw.h, docs/model_weights.md): the sweep against fz_draw_logwt on host-formed rows and
against the NumPy law of tests/_mw_ref.py, the Dirichlet step against its NumPy twin, the chains against NumPy chains and against
the reference's chains (golden g22).  tests/test_mw_host.py shows that no draw of the host-made chain problems lies close enough
to a cdf value for a count to differ legitimately; the k-NN chain problems assert the same here on the rows the GPU fitted."""
import numpy as np
import pytest

import _draw_ref as dr
import _mw_ref as mw
from conftest import DevArray, load_golden

pytestmark = pytest.mark.gpu

KEY = np.array([0x9E3779B9, 0x7F4A7C15], dtype=np.uint32)


def engine():
    from frankenz_amd.engine import get_engine
    return get_engine()


def to_host(a, dtype):
    """a DevArray's contents"""
    from frankenz_amd._lib import check, ptr
    eng = engine()
    out = np.empty(a.shape, dtype=dtype)
    check(eng.lib.fz_dev_copy(eng.h, ptr(out), a.data_ptr(), out.nbytes))
    return out


def gpu_sweep(rows, lnw, M, u=None, key=None, sweep=0, first=0, nbr=None, nnbr=None, want_assign=True):
    N, W = rows.shape
    counts = np.full(M, -7, dtype=np.int64)                       # the call zeroes them
    assign = np.full(N, -7, dtype=np.int64) if want_assign else None
    engine().mw_sweep(rows, N, W, M, lnw, counts, u=u, key=key, sweep=sweep, first=first, neighbors=nbr, nnbr=nnbr, assign=assign)
    return assign, counts


def gpu_draw(t, u, nbr=None, nnbr=None):
    idx = np.empty((len(t), 1), dtype=np.int64)
    engine().draw_logwt(t, 1, idx, u=np.ascontiguousarray(u[:, None]), neighbors=nbr, nnbr=nnbr)
    return idx[:, 0]


def edge_problem(N, W, seed=0):
    """sparse rows with, by object index: -inf in whole 256-entry segments, a nan, every neighbour at weight 0, Nneighbors == 0;
    u = 0 on object 0 (and 4), u = 1 - 2^-53 on the last object"""
    M = W + 57
    rows, nbr, nnbr, lnw, u = mw.sparse_problem(N, W, M, seed=seed)
    lnw = lnw.copy()
    if N > 1 and W > 300:
        rows[1, :256] = -np.inf
        rows[1, 512:min(nnbr[1] - 1, 4000)] = -np.inf
    if N > 2 and nnbr[2] > 1:
        rows[2, nnbr[2] // 2] = np.nan
    if N > 4:
        lnw[nbr[4, :nnbr[4]]] = -np.inf                            # object 4: all of its neighbours have w = 0
    u[0] = 0.
    u[-1] = dr.TOP
    return rows, nbr, nnbr, lnw, u, M


# ---- the sweep --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('W', [1, 3, 255, 256, 257, 513, 1024, 1025, 4096, 4097])
def test_sweep_is_the_draw_on_pre_added_rows(W):
    for N in (1, 4, 5, 1027):
        rows, nbr, nnbr, lnw, u, M = edge_problem(N, W)
        t = mw.added_rows(rows, lnw, nbr, nnbr)
        assign, counts = gpu_sweep(rows, lnw, M, u=u, nbr=nbr, nnbr=nnbr)
        np.testing.assert_array_equal(assign, gpu_draw(t, u, nbr, nnbr))                       # index for index
        np.testing.assert_array_equal(counts, np.bincount(assign[assign >= 0], minlength=M))
        assert counts.sum() == (assign >= 0).sum()
        if N > 4:
            assert assign[4] == -1 and assign[3] == -1 and (W == 1 or assign[2] == -1)
        if N <= 5:                                                                             # and the NumPy law itself
            close = dr.near(t, u[:, None], mw.NEAR_REL, nnbr)
            assert not close.any()
            np.testing.assert_array_equal(assign, mw.sweep_ref(rows, lnw, u, M, nbr, nnbr)[0])
        _, c2 = gpu_sweep(rows, lnw, M, u=u, nbr=nbr, nnbr=nnbr, want_assign=False)           # assign is optional
        np.testing.assert_array_equal(c2, counts)


def test_sweep_on_dense_rows_of_70001_models():
    rs = np.random.RandomState(2401)
    N, M = 3, 70001
    rows = -rs.uniform(0., 12., size=(N, M)); lnw = -rs.uniform(0., 6., M)
    rows[1, 256:5000] = -np.inf
    lnw[rs.rand(M) < 0.3] = -np.inf
    u = np.array([0., rs.rand(), dr.TOP])
    assign, counts = gpu_sweep(rows, lnw, M, u=u)
    np.testing.assert_array_equal(assign, gpu_draw(rows + lnw[None, :], u))
    np.testing.assert_array_equal(assign, mw.sweep_ref(rows, lnw, u, M)[0])
    np.testing.assert_array_equal(counts, np.bincount(assign, minlength=M))
    assert np.isfinite(lnw[assign]).all()


def test_all_objects_on_one_model():
    rs = np.random.RandomState(2402)
    N, M = 4096, 9
    rows = -rs.uniform(0., 12., size=(N, M))
    lnw = np.full(M, -np.inf); lnw[7] = -1.5
    assign, counts = gpu_sweep(rows, lnw, M, u=rs.rand(N))
    assert counts[7] == 4096 and counts.sum() == 4096 and (assign == 7).all()


def test_both_geometries_give_the_same_assignments(monkeypatch):
    rows, nbr, nnbr, lnw, u, M = edge_problem(37, 513, seed=3)
    ref = gpu_sweep(rows, lnw, M, u=u, nbr=nbr, nnbr=nnbr)
    for wpo in ('1', '4'):
        monkeypatch.setenv('FZ_DRAW_WPO', wpo)
        got = gpu_sweep(rows, lnw, M, u=u, nbr=nbr, nnbr=nnbr)
        np.testing.assert_array_equal(got[0], ref[0]); np.testing.assert_array_equal(got[1], ref[1])
    monkeypatch.delenv('FZ_DRAW_WPO')
    np.testing.assert_array_equal(ref[0], mw.sweep_ref(rows, lnw, u, M, nbr, nnbr)[0])


@pytest.mark.parametrize('W', [3, 513, 1024])
def test_register_and_re_reading_forms_give_the_same_assignments(W, monkeypatch):
    """rows of up to 1 024 entries stay in the wave's registers; FZ_MW_REG=0 forces the form that re-reads the hit segment"""
    rows, nbr, nnbr, lnw, u, M = edge_problem(37, W, seed=9)
    ref = gpu_sweep(rows, lnw, M, u=u, nbr=nbr, nnbr=nnbr)
    monkeypatch.setenv('FZ_MW_REG', '0')
    got = gpu_sweep(rows, lnw, M, u=u, nbr=nbr, nnbr=nnbr)
    np.testing.assert_array_equal(got[0], ref[0]); np.testing.assert_array_equal(got[1], ref[1])
    np.testing.assert_array_equal(got[0], gpu_draw(mw.added_rows(rows, lnw, nbr, nnbr), u, nbr, nnbr))
    dense = -np.random.RandomState(W).uniform(0., 12., size=(5, W))
    a = gpu_sweep(dense, lnw[:W], W, u=u[:5])
    monkeypatch.delenv('FZ_MW_REG')
    b = gpu_sweep(dense, lnw[:W], W, u=u[:5])
    np.testing.assert_array_equal(a[0], b[0]); np.testing.assert_array_equal(a[0], gpu_draw(dense + lnw[None, :W], u[:5]))


def test_host_pointers_under_a_small_workspace_equal_device_pointers():
    eng = engine()
    rows, nbr, nnbr, lnw, u, M = edge_problem(1027, 257, seed=4)
    N, W = rows.shape
    ref = gpu_sweep(rows, lnw, M, u=u, nbr=nbr, nnbr=nnbr)
    old = eng.workspace_limit()
    eng.set_workspace_limit(1 << 20)                                # rows alone are 2 MiB: several chunks
    try:
        small = gpu_sweep(rows, lnw, M, u=u, nbr=nbr, nnbr=nnbr)
    finally:
        eng.set_workspace_limit(old)
    d_counts, d_assign = DevArray(np.zeros(M, dtype=np.int64)), DevArray(np.zeros(N, dtype=np.int64))
    eng.mw_sweep(DevArray(rows), N, W, M, DevArray(lnw), d_counts, u=DevArray(u), neighbors=DevArray(nbr), nnbr=DevArray(nnbr), assign=d_assign)
    for got in (small, (to_host(d_assign, np.int64), to_host(d_counts, np.int64))):
        np.testing.assert_array_equal(got[0], ref[0]); np.testing.assert_array_equal(got[1], ref[1])


def test_a_permutation_of_the_objects_permutes_the_assignments():
    rows, nbr, nnbr, lnw, u, M = edge_problem(1027, 20, seed=5)
    ref = gpu_sweep(rows, lnw, M, u=u, nbr=nbr, nnbr=nnbr)
    p = np.random.RandomState(6).permutation(len(rows))
    got = gpu_sweep(np.ascontiguousarray(rows[p]), lnw, M, u=np.ascontiguousarray(u[p]), nbr=np.ascontiguousarray(nbr[p]),
                    nnbr=np.ascontiguousarray(nnbr[p]))
    np.testing.assert_array_equal(got[0], ref[0][p]); np.testing.assert_array_equal(got[1], ref[1])


def test_philox_uniforms_of_the_sweep():
    from frankenz_amd.samplers import _philox_uniform
    rows, nbr, nnbr, lnw, _, M = edge_problem(1027, 20, seed=7)
    N = len(rows)
    for sweep in (0, 3, 2**33 + 1):
        ref = gpu_sweep(rows, lnw, M, u=_philox_uniform(KEY, sweep, N), nbr=nbr, nnbr=nnbr)
        got = gpu_sweep(rows, lnw, M, key=KEY, sweep=sweep, nbr=nbr, nnbr=nnbr)
        np.testing.assert_array_equal(got[0], ref[0]); np.testing.assert_array_equal(got[1], ref[1])
    # `first`: the object's index in the caller's whole array
    tail = gpu_sweep(np.ascontiguousarray(rows[5:]), lnw, M, key=KEY, sweep=3, first=5, nbr=np.ascontiguousarray(nbr[5:]),
                     nnbr=np.ascontiguousarray(nnbr[5:]))
    np.testing.assert_array_equal(tail[0], gpu_sweep(rows, lnw, M, key=KEY, sweep=3, nbr=nbr, nnbr=nnbr)[0][5:])


def test_refusals():
    eng = engine()
    rows, nbr, nnbr, lnw, u, M = edge_problem(9, 20, seed=8)
    for bad in (M, -1):                                              # inside Nneighbors: refused, never used as an index
        nb = nbr.copy(); nb[6, 1] = bad
        assert nnbr[6] > 1
        with pytest.raises(IndexError, match='neighbour index'):
            gpu_sweep(rows, lnw, M, u=u, nbr=nb, nnbr=nnbr)
    nb = nbr.copy(); nb[6, nnbr[6]:] = 10**12                        # past Nneighbors: never read
    np.testing.assert_array_equal(gpu_sweep(rows, lnw, M, u=u, nbr=nb, nnbr=nnbr)[0], gpu_sweep(rows, lnw, M, u=u, nbr=nbr, nnbr=nnbr)[0])
    nn = nnbr.copy(); nn[2] = 21
    with pytest.raises(IndexError, match='Nneighbors'):
        gpu_sweep(rows, lnw, M, u=u, nbr=nbr, nnbr=nn)
    uu = u.copy(); uu[1] = 1.5
    with pytest.raises(ValueError, match='uniform'):
        gpu_sweep(rows, lnw, M, u=uu, nbr=nbr, nnbr=nnbr)
    counts = np.zeros(M, dtype=np.int64)
    with pytest.raises(NotImplementedError, match='FZ_DRAW_LMAX'):   # refused before anything is read
        eng.mw_sweep(rows, 9, (1 << 20) + 1, M, lnw, counts, u=u, neighbors=nbr, nnbr=nnbr)
    with pytest.raises(NotImplementedError, match='2\\^31'):
        eng.mw_sweep(rows, 9, 20, 1 << 31, lnw, counts, u=u, neighbors=nbr, nnbr=nnbr)
    with pytest.raises(ValueError, match='dense'):
        eng.mw_sweep(rows, 9, 20, M, lnw, counts, u=u)
    pos, lw = np.empty(M), np.empty(M)
    for a in (0., -1., np.nan, np.inf):
        alpha = np.ones(M); alpha[3] = a
        with pytest.raises(ValueError, match='alpha'):
            eng.mw_dirichlet(alpha, counts, M, KEY, 0, pos, lw)
    with pytest.raises(ValueError, match='device arrays'):
        eng.mw_chain(rows, 9, 20, M, np.ones(M), lnw.copy(), KEY, 0, 2, counts, pos, neighbors=nbr, nnbr=nnbr)


# ---- the Dirichlet step -------------------------------------------------------------------------------------------------------------
def dirichlet_case(M, seed=0):
    rs = np.random.RandomState(2500 + M + seed)
    alpha = np.exp(rs.uniform(np.log(0.05), np.log(2.), M))
    counts = np.where(rs.rand(M) < 0.5, 0, np.floor(np.exp(rs.uniform(0., np.log(1e4), M)))).astype(np.int64)
    return alpha, counts


@pytest.mark.parametrize('M', [1, 63, 64, 65, 70001])
def test_dirichlet_step_against_the_numpy_twin(M):
    from frankenz_amd.samplers import _philox_gamma
    eng = engine()
    alpha, counts = dirichlet_case(M)
    shape = alpha + counts
    assert M < 1000 or (shape.min() < 0.06 and shape.max() > 5e3)
    pos, lnw, pos2, lnw2 = np.empty(M), np.empty(M), np.empty(M), np.empty(M)
    eng.mw_dirichlet(alpha, counts, M, KEY, 11, pos, lnw)
    eng.mw_dirichlet(DevArray(alpha), DevArray(counts), M, KEY, 11, pos2, lnw2)
    assert pos.tobytes() == pos2.tobytes() and lnw.tobytes() == lnw2.tobytes()                # the same key: the same bits
    assert abs(pos.sum() - 1.) <= 1e-12
    nz = pos > 0
    np.testing.assert_allclose(lnw[nz], np.log(pos[nz]), rtol=1e-12, atol=1e-12)
    assert np.all(np.isneginf(lnw[~nz]))
    eng.mw_dirichlet(alpha, counts, M, KEY, 12, pos2, lnw2)
    assert M == 1 or not np.array_equal(pos, pos2)
    g = _philox_gamma(KEY, 11, shape)
    # a draw that took another number of attempts is another draw altogether; one that took the same number agrees to 1e-12
    ratio = pos[g > 0] * g.sum() / g[g > 0]
    other = np.abs(ratio / np.median(ratio) - 1.) > 1e-12
    print('M = %d: %d of %d draws differ from the twin' % (M, other.sum(), M))
    assert other.sum() <= M // 10000
    if not other.any():
        np.testing.assert_allclose(pos, g / g.sum(), rtol=1e-12, atol=0)


# ---- chains -------------------------------------------------------------------------------------------------------------------------
def knn_rows(K, k):
    from frankenz_amd import NearestNeighbors
    X, Xe, Xm, Y, Ye, Ym, _ = dr.knn_problem(K, k)
    nn = NearestNeighbors(Y, Ye, Ym, K=K, rstate=np.random.RandomState(1), verbose=False)
    nn.fit(X.copy(), Xe.copy(), Xm.copy(), rstate=np.random.RandomState(44), k=k, verbose=False)
    return nn


def host_chain_equals_numpy(s, rows, nbr, nnbr, M, alpha, seed):
    pos0 = mw.stack_start(rows, M, nbr, nnbr)
    counts, pos, worst = mw.chain_host(rows, M, alpha, pos0, np.random.RandomState(seed), mw.CHAIN_SWEEPS, nbr, nnbr)
    assert worst <= dr.NEAR_CAP
    thin = 3
    s.run_mcmc((mw.CHAIN_SWEEPS - 1) // thin, alpha=alpha, pos_init=pos0, thin=thin, rstate=np.random.RandomState(seed), verbose=False, draws='host')
    got = np.array(s.sweep_counts)
    assert got.shape == (mw.CHAIN_SWEEPS, M)
    np.testing.assert_array_equal(got, counts)
    smp, lnp = s.results
    np.testing.assert_array_equal(smp, pos[thin::thin])
    assert np.isfinite(lnp).all() and s.philox_key is None


@pytest.mark.parametrize('K,k', [(5, 4), (25, 24)])
def test_host_chain_on_knn_rows(K, k):
    nn = knn_rows(K, k)
    rows, nbr, nnbr = nn.fit_lnlike.copy(), nn.neighbors.copy(), nn.Nneighbors.copy()
    assert rows.shape[1] == K * k
    host_chain_equals_numpy(nn.weight_sampler(), rows, nbr, nnbr, nn.NMODEL, np.full(nn.NMODEL, 0.7), 2600 + K)


@pytest.mark.parametrize('tag', mw.CHAIN_TAGS)
def test_host_chain_on_host_made_rows(tag):
    from frankenz_amd import model_weight_sampler
    rows, nbr, nnbr, M, alpha, seed = mw.chain_problem(tag)
    host_chain_equals_numpy(model_weight_sampler(rows, neighbors=nbr, Nneighbors=nnbr, Nmodels=M), rows, nbr, nnbr, M, alpha, seed)


def test_device_chain_is_single_calls_back_to_back():
    eng = engine()
    rows, nbr, nnbr, M, alpha, _ = mw.chain_problem('sparse600')
    N, W = rows.shape
    lnw0 = np.log(mw.stack_start(rows, M, nbr, nnbr) + 1e-300)
    d_rows, d_nbr, d_nn = DevArray(rows), DevArray(nbr), DevArray(nnbr)
    thin, s0 = 5, 4
    lnw = lnw0.copy()
    counts, pos, call = np.zeros(M, dtype=np.int64), np.empty(M), np.zeros((thin, M), dtype=np.int64)
    eng.mw_chain(d_rows, N, W, M, alpha, lnw, KEY, s0, thin, counts, pos, neighbors=d_nbr, nnbr=d_nn, counts_all=call)
    l1, c1, p1 = lnw0.copy(), np.zeros(M, dtype=np.int64), np.empty(M)
    for t in range(thin):
        eng.mw_sweep(rows, N, W, M, l1, c1, key=KEY, sweep=s0 + t, neighbors=nbr, nnbr=nnbr)
        np.testing.assert_array_equal(call[t], c1)
        eng.mw_dirichlet(alpha, c1, M, KEY, s0 + t, p1, l1)
    assert pos.tobytes() == p1.tobytes() and lnw.tobytes() == l1.tobytes()
    np.testing.assert_array_equal(counts, c1)
    assert c1.sum() == (nnbr > 0).sum()
    # without the per-sweep buffer, and with every argument on the device
    d_lnw, d_counts, d_pos = DevArray(lnw0), DevArray(np.zeros(M, dtype=np.int64)), DevArray(np.zeros(M))
    eng.mw_chain(d_rows, N, W, M, DevArray(alpha), d_lnw, KEY, s0, thin, d_counts, d_pos, neighbors=d_nbr, nnbr=d_nn)
    assert to_host(d_pos, np.float64).tobytes() == p1.tobytes() and to_host(d_lnw, np.float64).tobytes() == l1.tobytes()
    np.testing.assert_array_equal(to_host(d_counts, np.int64), c1)


def test_device_mode_of_the_sampler_is_the_twins_chain():
    """draws='device' from the Python surface: the key comes from rstate once, sweep s draws _philox_uniform(key, s, N) and
    _philox_gamma(key, s, alpha + counts); a saved sample is the thin-th sweep"""
    from frankenz_amd import model_weight_sampler
    from frankenz_amd.samplers import _philox_gamma, _philox_uniform
    rows, nbr, nnbr, M, alpha, seed = mw.chain_problem('sparse20')
    N = len(rows)
    s = model_weight_sampler(DevArray(rows), neighbors=DevArray(nbr), Nneighbors=DevArray(nnbr), Nmodels=M)
    pos0 = mw.stack_start(rows, M, nbr, nnbr)
    s.run_mcmc(3, alpha=alpha, pos_init=pos0, thin=2, rstate=np.random.RandomState(seed), verbose=False)
    key = np.random.RandomState(seed).randint(0, 2**32, size=2, dtype=np.uint32)
    np.testing.assert_array_equal(s.philox_key, key)
    assert len(s.sweep_counts) == 7
    with np.errstate(divide='ignore'):
        lnw = np.log(pos0)
    saved = []
    for sweep in range(7):
        u = _philox_uniform(key, sweep, N)
        assert mw.near_share(rows, lnw, u, nbr, nnbr) == 0.
        _, c = mw.sweep_ref(rows, lnw, u, M, nbr, nnbr)
        np.testing.assert_array_equal(s.sweep_counts[sweep], c)
        g = _philox_gamma(key, sweep, alpha + c)
        lnw = np.log(g) - np.log(g.sum())
        saved.append(g / g.sum())
    np.testing.assert_allclose(s.results[0], np.array(saved)[2::2], rtol=1e-11, atol=0)


@pytest.mark.parametrize('draws', ['host', 'device'])
@pytest.mark.parametrize('tag', ['a1', 'a03'])
def test_chains_against_the_reference_chains(tag, draws):
    from frankenz_amd import model_weight_sampler
    g = load_golden('g22_model_weights')
    lnlike, alpha, ref = g['lnlike'], g[tag + '_alpha'], g[tag + '_samples']
    N, M = lnlike.shape
    s = model_weight_sampler(lnlike)
    s.run_mcmc(len(ref), alpha=alpha, thin=5, rstate=np.random.RandomState(2700 + len(tag)), verbose=False, draws=draws)
    smp, lnp = s.results
    assert smp.shape == ref.shape and np.isfinite(lnp).all() and np.max(np.abs(smp.sum(axis=1) - 1.)) < 1e-9
    mw.golden_chain_check(smp, ref, N)
    from test_nz_samplers_host import batch_means
    lm, lse = batch_means(lnp)
    rm, rse = batch_means(g[tag + '_samples_lnp'])
    print('%s %s: lnpost %.3f +- %.3f, reference %.3f +- %.3f' % (tag, draws, lm, lse, rm, rse))
    assert abs(lm - rm) <= 5 * np.sqrt(lse**2 + rse**2)


# ---- what the weights are for ---------------------------------------------------------------------------------------------------------
def test_logwt_through_predict_and_population_pdfs():
    import frankenz_oracle as fo
    from frankenz_amd import PDFDict
    nn = knn_rows(5, 4)
    M, N = nn.NMODEL, nn.NDATA
    s = nn.weight_sampler()
    s.run_mcmc(4, thin=2, rstate=np.random.RandomState(2801), verbose=False)
    w = np.mean(s.samples, axis=0)
    lw = s.logwt()
    np.testing.assert_array_equal(lw, mw.added_rows(nn.fit_lnlike, np.log(w), nn.neighbors, nn.Nneighbors))
    rs = np.random.RandomState(2802)
    z, ze = rs.uniform(0.1, 5.9, M), rs.uniform(0.01, 0.2, M)
    grid, sgrid = np.arange(0, 7 + 1e-5, .01), np.linspace(.005, 2, 500)
    pd, od = PDFDict(grid, sgrid), fo.KernelDict(grid, sgrid)
    pdfs = nn.predict(z, ze, label_dict=pd, logwt=lw, verbose=False)
    assert pdfs.shape == (N, len(grid)) and np.isfinite(pdfs).all()
    np.testing.assert_allclose(pdfs.sum(axis=1), 1., rtol=1e-9)
    assert not np.allclose(pdfs, nn.predict(z, ze, label_dict=pd, verbose=False))             # the population weights matter
    for i in (0, 7, 19, N - 1):                                                                # the route itself: the KDE under exp(lw - max)
        n = nn.Nneighbors[i]
        idx, t = nn.neighbors[i, :n], lw[i, :n]
        ref = fo.gauss_kde_dict(od, y=z[idx], y_std=ze[idx], y_wt=np.exp(t - t.max()))
        np.testing.assert_allclose(pdfs[i], ref / ref.sum(), rtol=1e-8, atol=1e-14)
    # n(z) samples: the KDE of the labels weighted by each weight sample
    pop = s.population_pdfs(z, ze, label_dict=pd, kde_kwargs={'wt_thresh': 0})
    assert pop.shape == (4, len(grid))
    for k in range(4):
        ref = fo.gauss_kde_dict(od, y=z, y_std=ze, y_wt=s.samples[k], wt_thresh=0.)
        np.testing.assert_allclose(pop[k], ref / ref.sum(), rtol=1e-8, atol=1e-14)
    ref = fo.gauss_kde_dict(od, y=z, y_std=ze, y_wt=w)                                        # the default threshold clips
    np.testing.assert_allclose(s.population_pdfs(z, ze, label_dict=pd, w=w)[0], ref / ref.sum(), rtol=1e-8, atol=1e-14)


def test_device_resident_rows_stay_on_the_device():
    """by construction: with device rows and a given start the sampler holds no host copy of the rows, so nothing of size N x W can
    cross the bus inside a chain (the library has no copy counters); the chain equals the one on uploaded host rows"""
    from frankenz_amd import model_weight_sampler
    rows, nbr, nnbr, M, alpha, seed = mw.chain_problem('sparse20')
    pos0 = mw.stack_start(rows, M, nbr, nnbr)
    a = model_weight_sampler(rows, neighbors=nbr, Nneighbors=nnbr, Nmodels=M)
    b = model_weight_sampler(DevArray(rows), neighbors=DevArray(nbr), Nneighbors=DevArray(nnbr), Nmodels=M)
    for s in (a, b):
        s.run_mcmc(3, alpha=alpha, pos_init=pos0, thin=2, rstate=np.random.RandomState(seed), verbose=False)
    assert b._dev[0] is b.lnlike and not isinstance(b.lnlike, np.ndarray)
    assert np.array(a.samples).tobytes() == np.array(b.samples).tobytes()
    np.testing.assert_array_equal(a.sweep_counts, b.sweep_counts)


def test_default_start_and_logwt_read_device_rows_back():
    """pos_init=None and logwt() are the two places that copy device rows to the host (DeviceArray.numpy()): the chain and the rows
    equal the ones from host arrays"""
    from frankenz_amd import model_weight_sampler
    eng = engine()
    rows, nbr, nnbr, M, alpha, seed = mw.chain_problem('sparse20')
    a = model_weight_sampler(rows, neighbors=nbr, Nneighbors=nnbr, Nmodels=M)
    b = model_weight_sampler(eng.device_array(rows), neighbors=eng.device_array(nbr), Nneighbors=eng.device_array(nnbr), Nmodels=M)
    np.testing.assert_array_equal(b._stack_start(), a._stack_start())
    np.testing.assert_allclose(a._stack_start(), mw.stack_start(rows, M, nbr, nnbr), rtol=1e-13, atol=1e-16)
    for s in (a, b):
        s.run_mcmc(2, alpha=alpha, thin=2, rstate=np.random.RandomState(seed), verbose=False)
    assert np.array(a.samples).tobytes() == np.array(b.samples).tobytes()
    np.testing.assert_array_equal(b.logwt(), a.logwt())
    np.testing.assert_array_equal(b.logwt(), mw.added_rows(rows, np.log(np.mean(a.samples, axis=0)), nbr, nnbr))
    d = model_weight_sampler(eng.device_array(rows[:, :7].copy()))                             # dense
    np.testing.assert_array_equal(d.logwt(np.full(7, 0.25)), rows[:, :7] + np.log(0.25))


def test_device_arrays_need_no_workspace_and_uploads_do():
    from frankenz_amd import model_weight_sampler
    eng = engine()
    rows, nbr, nnbr, lnw, u, M = edge_problem(1027, 257, seed=4)                               # 2 MiB of rows
    pos0 = np.full(M, 1. / M)
    old = eng.workspace_limit()
    eng.set_workspace_limit(1 << 20)
    try:
        with pytest.raises(MemoryError, match='bytes'):
            next(model_weight_sampler(rows, neighbors=nbr, Nneighbors=nnbr, Nmodels=M).sample(1, pos_init=pos0))
        s = model_weight_sampler(DevArray(rows), neighbors=DevArray(nbr), Nneighbors=DevArray(nnbr), Nmodels=M)
        pos, lnp = next(s.sample(1, pos_init=pos0, thin=1, rstate=np.random.RandomState(1)))
    finally:
        eng.set_workspace_limit(old)
    assert abs(pos.sum() - 1.) < 1e-12 and np.isfinite(lnp)


def test_a_sum_of_zero_fails_loudly():
    """shapes so small that every gamma draw underflows: no weights to normalise, the call says so instead of returning nan"""
    eng = engine()
    M = 300
    pos, lnw = np.empty(M), np.empty(M)
    with pytest.raises(RuntimeError, match='underflowed'):
        eng.mw_dirichlet(np.full(M, 1e-300), np.zeros(M, dtype=np.int64), M, KEY, 0, pos, lnw)
    alpha = np.full(M, 1e-300); alpha[17] = 1.                                                 # one draw with mass is enough
    eng.mw_dirichlet(alpha, np.zeros(M, dtype=np.int64), M, KEY, 0, pos, lnw)
    assert pos[17] == 1. and lnw[17] == 0. and (np.delete(pos, 17) == 0.).all() and np.isneginf(np.delete(lnw, 17)).all()
