"""The Monte-Carlo draws of the k-NN fitter on the GPU (docs/knn.md, "Monte-Carlo draws on the device"): fz_knn_draw_features and
fz_knn_draw_trees against the NumPy twin ``knn._philox_normal`` and this package's NumPy feature maps, the refusals, the feature
sets installed as an upload of the same floats would install them, and ``query_draws='device'`` end to end (NumPy arrays and
library device arrays here; torch tensors and the two-rank sharded call in fresh processes)."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from frankenz_amd import knn, pdf
from frankenz_amd.knn import NearestNeighbors

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
KEY = (0x5EED0001, 0x0BADF00D)          # the key tests/test_knn_mc_host.py holds the twin's law at
U = 2. ** -53


def eng():
    from frankenz_amd.engine import get_engine
    return get_engine(None)


def draw(x, xe, kind='identity', fk=None, key=KEY, first=0):
    x, xe = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(xe, dtype=np.float64)
    q = np.full(x.shape, -777.)
    eng().knn_draw_features(x, xe, x.shape[0], x.shape[1], knn._fmap_struct(kind, [], fk or {}, x.shape[1]), key, first, q)
    return q


@pytest.mark.parametrize('F', [1, 2, 5, 6, 7, 32])
def test_standard_normals_against_the_twin(F):
    """identity map, x = 0, xe = 1: |dz| <= 2e-14 (r <= 8.57; the rounding of the angle 2 pi u2 and one to two ulps each in log,
    sqrt, cos / sin bound it near 1e-14)"""
    worst = 0.
    for N in (1, 63, 64, 65, 257, 1000):
        z = draw(np.zeros((N, F)), np.ones((N, F)))
        d = np.abs(z - knn._philox_normal(KEY, 0, N, F, 0)).max()
        worst = max(worst, d)
        assert d <= 2e-14, (N, F, d)
    print("F=%d: max |z_device - z_twin| = %.3g" % (F, worst))


@pytest.mark.parametrize('base', [0, 2**32 - 3])
def test_a_call_equals_its_two_halves_bit_for_bit(base):
    """a draw is a function of (key, row, band, set): 300 rows from `base` in one call, and in two calls split at row 130"""
    rs = np.random.RandomState(11)
    x, xe = rs.normal(size=(300, 5)), rs.uniform(0.1, 2., size=(300, 5))
    whole = draw(x, xe, first=base)
    np.testing.assert_array_equal(whole[:130], draw(x[:130], xe[:130], first=base))
    np.testing.assert_array_equal(whole[130:], draw(x[130:], xe[130:], first=base + 130))
    z = knn._philox_normal(KEY, base, 300, 5, 0)
    assert np.all(np.abs(whole - (x + xe * z)) <= 2e-14 * np.abs(xe) + 4.5e-16 * (np.abs(x) + 9. * np.abs(xe)))


def test_draws_against_the_twin_and_zero_errors():
    """|d - (x + xe z_twin)| <= 2e-14 |xe| + 4.5e-16 (|x| + 9 |xe|); xe == 0 returns x bit for bit"""
    rs = np.random.RandomState(12)
    N, F = 1000, 5
    x = rs.normal(size=(N, F)) * 10. ** rs.uniform(-3, 6, size=(N, F))
    xe = 10. ** rs.uniform(-4, 4, size=(N, F))
    zero = rs.rand(N, F) < 0.2
    xe[zero] = 0.
    d = draw(x, xe)
    z = knn._philox_normal(KEY, 0, N, F, 0)
    err = np.abs(d - (x + xe * z))
    bound = 2e-14 * np.abs(xe) + 4.5e-16 * (np.abs(x) + 9. * np.abs(xe))
    print("draws: max err / bound = %.3g" % (err / np.maximum(bound, 1e-300)).max())
    assert np.all(err <= bound)
    np.testing.assert_array_equal(d[zero], x[zero])


def test_maps_against_the_numpy_functions_on_the_devices_own_draws():
    """magnitude (vector zeropoints) and luptitude (vector skynoise and zeropoints) of the identity call's draws: within
    16 u (2.5 |log10(d / zp)| + 1), resp. 16 u (|asinh t| + |ln(skynoise / zeropoint)| + 1); nan where NumPy has nan"""
    rs = np.random.RandomState(13)
    N, F = 1000, 5
    sky = np.array([0.873, 0.348, 0.418, 0.873, 3.476])
    zp = 10 ** (0.4 * np.array([23.9, 22.5, 24.1, 23.0, 21.7]))
    x = rs.lognormal(1., 1., size=(N, F)) * 3.
    x[::7] *= 0.01                                                     # faint objects: draws on both sides of zero
    xe = np.tile(sky, (N, 1))
    d = draw(x, xe)
    assert (d < 0).sum() > 20
    with np.errstate(all='ignore'):
        mag = draw(x, xe, 'magnitude', dict(zeropoints=zp))
        want = pdf.magnitude(d, xe, zeropoints=zp)[0]
        np.testing.assert_array_equal(np.isnan(mag), np.isnan(want))
        assert np.isnan(want).sum() == (d < 0).sum()
        ok = ~np.isnan(want)
        tol = 16. * U * (2.5 * np.abs(np.log10(d / zp)) + 1.)
        print("magnitude: max err / tol = %.3g" % (np.abs(mag - want)[ok] / tol[ok]).max())
        assert np.all(np.abs(mag - want)[ok] <= tol[ok])
    lup = draw(x, xe, 'luptitude', dict(skynoise=sky, zeropoints=zp))
    want = pdf.luptitude(d, xe, skynoise=sky, zeropoints=zp)[0]
    tol = 16. * U * (np.abs(np.arcsinh(d / (2. * sky))) + np.abs(np.log(sky / zp)) + 1.)
    print("luptitude: max err / tol = %.3g" % (np.abs(lup - want) / tol).max())
    assert np.all(np.isfinite(lup)) and np.all(np.abs(lup - want) <= tol)


def test_refusals_and_propagation():
    rs = np.random.RandomState(14)
    N, F = 300, 5
    x, xe = rs.normal(size=(N, F)), rs.uniform(0.1, 2., size=(N, F))
    for bad in (-0.5, np.nan):
        e = xe.copy(); e[137, 3] = bad
        with pytest.raises(ValueError, match=r'object 137\b'):
            draw(x, e)
        e[41, 0] = np.nan; e[250, 4] = -1.
        with pytest.raises(ValueError, match=r'object 41\b'):
            draw(x, e, 'luptitude')
    # non-finite fluxes: NumPy's arithmetic
    xb = x.copy(); xb[5, 1] = np.inf; xb[6, 2] = -np.inf; xb[7, 0] = np.nan
    z = knn._philox_normal(KEY, 0, N, F, 0)
    d = draw(xb, xe)
    with np.errstate(all='ignore'):
        want = xb + xe * z
        np.testing.assert_array_equal(np.isnan(d), np.isnan(want))
        np.testing.assert_array_equal(d[np.isinf(want)], want[np.isinf(want)])
        assert np.isnan(d).sum() == 1 and np.isinf(d).sum() == 2
        for kind, f in (('magnitude', lambda v: pdf.magnitude(v, xe)[0]), ('luptitude', lambda v: pdf.luptitude(v, xe)[0])):
            got, ref = draw(xb, xe, kind), f(d)
            np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
            np.testing.assert_array_equal(got[np.isinf(ref)], ref[np.isinf(ref)])
    # an infinite error is a scale NumPy accepts: inf or nan draws, no refusal
    e = xe.copy(); e[9, 2] = np.inf
    assert not np.isfinite(draw(x, e)[9, 2])
    # no objects: no launch, an empty result
    assert draw(np.zeros((0, F)), np.zeros((0, F))).shape == (0, F)
    nn = NearestNeighbors(np.ones((8, F)), np.ones((8, F)), np.ones((8, F)), K=1, rstate=np.random.RandomState(0), verbose=False)
    q0 = nn.query_features(np.zeros((0, F)), np.zeros((0, F)), draws='device', key=KEY)
    assert q0.shape == (0, F) and q0.dtype == np.float64
    # the feature sets refuse a bad model error the same way, and install nothing
    Y = rs.lognormal(1., 1., size=(70, F)); Ye = 0.05 * Y; Ye[33, 1] = -1e-3
    with pytest.raises(ValueError, match=r'model 33\b'):
        NearestNeighbors(Y, Ye, np.ones_like(Y), K=2, rstate=np.random.RandomState(0), verbose=False, feature_draws='device')


def sets_problem(M, F, seed):
    rs = np.random.RandomState(seed)
    sky = rs.uniform(0.3, 1.5, F)
    zp = 10 ** (0.4 * rs.uniform(22., 24., F))
    Y = rs.lognormal(1., 1., size=(M, F)) * 3.; Ye = 0.05 * Y + 0.2 * sky; Ym = np.ones((M, F))
    N = 96
    X = Y[rs.choice(M, N)] + sky * rs.randn(N, F); Xe = np.tile(sky, (N, 1)); Xm = np.ones((N, F))
    return Y, Ye, Ym, X, Xe, Xm, dict(skynoise=sky, zeropoints=zp)


@pytest.mark.parametrize('F', [5, 7])
@pytest.mark.parametrize('K', [1, 3])
@pytest.mark.parametrize('M', [64, 65, 3073])
def test_feature_sets_drawn_on_the_device(M, K, F):
    """3073 is one past FZ_MP_ALIGN; F = 5 takes the k-d-ordered matrix-pipe search, F = 7 the vector one"""
    Y, Ye, Ym, X, Xe, Xm, fk = sets_problem(M, F, 100 + F)
    R = np.random.RandomState(7)
    nn = NearestNeighbors(Y, Ye, Ym, K=K, feature_map='luptitude', fmap_kwargs=fk, rstate=R, verbose=False, feature_draws='device')
    # rstate: exactly one randint, kept as the key
    R2 = np.random.RandomState(7)
    key = R2.randint(0, 2**32, size=2, dtype=np.uint32)
    np.testing.assert_array_equal(nn.feature_key, key)
    assert R.rand() == R2.rand()
    assert len(nn.KDTrees) == K
    # the sets: float32(map(float32(y + ye z))) with the map in fp64, within one float32 ulp of the twin
    ndiff = 0
    for t in range(K):
        got = nn.KDTrees[t].data
        assert got.dtype == np.float32 and got.shape == (M, F)
        z = knn._philox_normal(key, 0, M, F, 1 + t)
        d32 = (Y + Ye * z).astype(np.float32)
        want = pdf.luptitude(d32.astype(np.float64), Ye, **fk)[0].astype(np.float32)
        assert np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64))
        ndiff += int((got != want).sum())
    print("M=%d K=%d F=%d: %d of %d entries differ from the twin (by one float32 ulp at the most)" % (M, K, F, ndiff, K * M * F))
    # searching the sets as drawn == searching the copied-out floats sent through fz_knn_upload_trees
    e = eng()
    assert e._trees_key == nn._feats_key
    nn.fit(X.copy(), Xe.copy(), Xm.copy(), rstate=np.random.RandomState(3), k=5, verbose=False)
    assert e._trees_key == nn._feats_key
    nn2 = NearestNeighbors(Y, Ye, Ym, K=K, feature_map='luptitude', fmap_kwargs=fk, rstate=np.random.RandomState(8), verbose=False)
    nn2.KDTrees = [knn._FeatureSet(nn.KDTrees[t].data.copy(), nn.leafsize) for t in range(K)]
    nn2._feats = None
    e._trees_key = None                                              # (the content key would otherwise spare the upload)
    nn2.fit(X.copy(), Xe.copy(), Xm.copy(), rstate=np.random.RandomState(3), k=5, verbose=False)
    np.testing.assert_array_equal(nn.neighbors, nn2.neighbors)
    np.testing.assert_array_equal(nn.Nneighbors, nn2.Nneighbors)
    np.testing.assert_array_equal(nn.fit_lnlike, nn2.fit_lnlike)
    assert (nn.Nneighbors >= 5).all()


@pytest.fixture(scope='module')
def e2e():
    rs = np.random.RandomState(21)
    sky = np.array([0.873, 0.348, 0.418, 0.873, 3.476])
    fk = dict(skynoise=sky, zeropoints=10 ** (0.4 * 23.9))
    M, N = 500, 200
    Y = rs.lognormal(1., 1., size=(M, 5)) * 3.; Ye = 0.05 * Y; Ym = np.ones((M, 5))
    X = Y[rs.choice(M, N)] + sky * rs.randn(N, 5); Xe = np.tile(sky, (N, 1)); Xm = np.ones((N, 5))
    z = rs.uniform(0, 6, M); ze = np.full(M, 0.05)
    nn = NearestNeighbors(Y, Ye, Ym, K=3, feature_map='luptitude', fmap_kwargs=fk, rstate=np.random.RandomState(1), verbose=False)
    return nn, X, Xe, Xm, z, ze, dict(label_grid=np.linspace(0., 6., 101), k=5, verbose=False, return_gof=True)


def test_query_draws_on_the_device_end_to_end(e2e):
    nn, X, Xe, Xm, z, ze, kw = e2e
    R = np.random.RandomState(31)
    p, (lm, le) = nn.fit_predict(X.copy(), Xe.copy(), Xm.copy(), z, ze, rstate=R, query_draws='device', **kw)
    R2 = np.random.RandomState(31)
    key = R2.randint(0, 2**32, size=2, dtype=np.uint32)
    np.testing.assert_array_equal(nn.query_key, key)
    assert R.rand() == R2.rand()                                     # exactly one randint was taken
    nb, nnb = nn.neighbors.copy(), nn.Nneighbors.copy()
    q = nn.query_features(X, Xe, draws='device', key=nn.query_key)
    assert isinstance(q, np.ndarray) and q.shape == X.shape and q.dtype == np.float64
    # the features are the map of the twin's draws, and the call is the call with them handed in
    want = pdf.luptitude(X + Xe * knn._philox_normal(key, 0, len(X), 5, 0), Xe, *nn.fmap_args, **nn.fmap_kwargs)[0]
    np.testing.assert_allclose(q, want, rtol=0, atol=1e-12)
    p2, (lm2, le2) = nn.fit_predict(X.copy(), Xe.copy(), Xm.copy(), z, ze, query_features=q, **kw)
    for a, b in ((p, p2), (lm, lm2), (le, le2)):
        np.testing.assert_array_equal(a, b)
    for save in (False, True):                                       # the save_fits=False route draws the same features
        p3 = nn.fit_predict(X.copy(), Xe.copy(), Xm.copy(), z, ze, rstate=np.random.RandomState(31), query_draws='device',
                            save_fits=save, **kw)[0]
        np.testing.assert_array_equal(p3, p)
    # fit() stores the same neighbours
    nn.fit(X.copy(), Xe.copy(), Xm.copy(), rstate=np.random.RandomState(31), query_draws='device', k=5, verbose=False)
    np.testing.assert_array_equal(nn.neighbors, nb); np.testing.assert_array_equal(nn.Nneighbors, nnb)
    # objects in device memory: the same features, left in device memory
    e = eng()
    dq = nn.query_features(e.device_array(X), e.device_array(Xe), draws='device', key=key)
    assert hasattr(dq, 'data_ptr')
    np.testing.assert_array_equal(dq.numpy(), q)
    # a sliced call with `first` is the slice of the whole call
    np.testing.assert_array_equal(nn.query_features(X[77:], Xe[77:], draws='device', key=key, first=77), q[77:])
    # key=None takes one randint from rstate
    np.testing.assert_array_equal(nn.query_features(X, Xe, rstate=np.random.RandomState(31), draws='device'), q)


def test_a_foreign_lprob_func_searches_with_the_same_features(e2e):
    nn, X, Xe, Xm, z, ze, kw = e2e
    nn.fit(X.copy(), Xe.copy(), Xm.copy(), rstate=np.random.RandomState(32), query_draws='device', k=5, verbose=False)
    nb, nnb, key = nn.neighbors.copy(), nn.Nneighbors.copy(), nn.query_key.copy()

    def hook(x, xe, xm, ys, yes, yms):
        lnl = -0.5 * np.square((ys - x) / xe).sum(axis=1)
        return np.zeros(len(ys)), lnl, lnl, np.full(len(ys), 5), -2. * lnl
    nn.fit(X.copy(), Xe.copy(), Xm.copy(), lprob_func=hook, rstate=np.random.RandomState(32), query_draws='device', k=5, verbose=False)
    np.testing.assert_array_equal(nn.query_key, key)
    np.testing.assert_array_equal(nn.Nneighbors, nnb)
    np.testing.assert_array_equal(nn.neighbors, nb)


def test_defaults_are_the_host_draws(e2e):
    nn, X, Xe, Xm, z, ze, kw = e2e
    a = nn.fit_predict(X.copy(), Xe.copy(), Xm.copy(), z, ze, rstate=np.random.RandomState(33), **kw)
    b = nn.fit_predict(X.copy(), Xe.copy(), Xm.copy(), z, ze, rstate=np.random.RandomState(33), query_draws='host', **kw)
    np.testing.assert_array_equal(a[0], b[0]); np.testing.assert_array_equal(a[1][1], b[1][1])
    q = nn._query_features(X, Xe, np.random.RandomState(33))
    c = nn.fit_predict(X.copy(), Xe.copy(), Xm.copy(), z, ze, query_features=q, **kw)
    np.testing.assert_array_equal(a[0], c[0])


def test_torch_tensors_in_a_fresh_process():
    """device tensors with ``out=``, ``prepare_fit_predict().run`` and ``fit_sample`` on device tensors (tests/_gpu_knn_mc_torch.py)"""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0')
    r = subprocess.run([sys.executable, os.path.join(HERE, '_gpu_knn_mc_torch.py')], capture_output=True, text=True, timeout=600, env=env)
    for marker in ('KNN_MC_DEVICE_TENSORS_OK', 'KNN_MC_PREPARED_OK', 'KNN_MC_FIT_SAMPLE_OK'):
        assert marker in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_two_ranks_draw_what_one_process_draws(tmp_path):
    """``sharded_fit_predict(query_draws='device')`` in two gloo ranks on GPU 0 (the overlapped path and the block path): each rank
    draws the rows it computes at their global row numbers, and the result is the single-process call's, bit for bit"""
    s = socket.socket(); s.bind(('127.0.0.1', 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0')
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, '_gpu_knn_mc_shard_worker.py'), str(r), '2', str(port), str(tmp_path)], env=env)
             for r in range(2)]
    for p in procs:
        assert p.wait(timeout=600) == 0
    sys.path.insert(0, HERE)
    import _gpu_knn_mc_shard_worker as w
    mk, X, Xe, Xm, z, ze, kw = w.scenario()
    nn = mk()
    Xc = X.copy()
    p, (lm, le) = nn.fit_predict(Xc, Xe.copy(), Xm.copy(), z, ze, rstate=np.random.RandomState(2), query_draws='device', return_gof=True,
                                 verbose=False, **kw)
    for r in range(2):
        out = np.load(os.path.join(str(tmp_path), 'rank%d.npz' % r))
        np.testing.assert_array_equal(out['key'], nn.query_key)
        for tag in ('ov', 'blk'):
            np.testing.assert_array_equal(out[tag + '_pdfs'], p)
            np.testing.assert_array_equal(out[tag + '_lmap'], lm)
            np.testing.assert_array_equal(out[tag + '_levid'], le)
