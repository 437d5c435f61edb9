"""The torch side of tests/test_hip_knn_mc.py, run in ONE fresh process (the suite's own process never brings up a second GPU runtime
stack): ``query_draws='device'`` with device tensors and ``out=``, through ``prepare_fit_predict().run``, and ``fit_sample`` on
device tensors without ``query_features``.  Prints one ``<NAME>_OK`` marker per check.
    python tests/_gpu_knn_mc_torch.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIG = np.array([0.873, 0.348, 0.418, 0.873, 3.476])


def main():
    import torch
    from frankenz_amd import NearestNeighbors
    dev = torch.device('cuda', 0)
    rs = np.random.RandomState(21)
    M, N = 500, 200
    Y = rs.lognormal(1., 1., size=(M, 5)) * 3.; Ye = 0.05 * Y; Ym = np.ones((M, 5))
    X = Y[rs.choice(M, N)] + SIG * rs.randn(N, 5); Xe = np.tile(SIG, (N, 1)); Xm = np.ones((N, 5))
    z = rs.uniform(0, 6, M); ze = np.full(M, 0.05)
    grid = np.linspace(0., 6., 101)
    nn = NearestNeighbors(Y, Ye, Ym, K=3, feature_map='luptitude', fmap_kwargs=dict(skynoise=SIG, zeropoints=10 ** (0.4 * 23.9)),
                          rstate=np.random.RandomState(1), verbose=False, device=0, feature_draws='device')
    kw = dict(label_grid=grid, k=5, verbose=False, return_gof=True, save_fits=False)
    tens = lambda: tuple(torch.from_numpy(a.copy()).to(dev) for a in (X, Xe, Xm))
    new_out = lambda: (torch.empty((N, len(grid)), dtype=torch.float64, device=dev), torch.empty(N, dtype=torch.float64, device=dev),
                       torch.empty(N, dtype=torch.float64, device=dev))

    # NumPy call, device tensors with out=, and the call with the features handed in: one result, bit for bit
    p, (lm, le) = nn.fit_predict(X.copy(), Xe.copy(), Xm.copy(), z, ze, rstate=np.random.RandomState(2), query_draws='device', **kw)
    key = nn.query_key.copy()
    dX, dXe, dXm = tens()
    out = new_out()
    r = nn.fit_predict(dX, dXe, dXm, z, ze, rstate=np.random.RandomState(2), query_draws='device', out=out, **kw)
    torch.cuda.synchronize()
    assert r[0] is out[0] and np.array_equal(nn.query_key, key)
    for a, b in zip(out, (p, lm, le)):
        np.testing.assert_array_equal(a.cpu().numpy(), b)
    dX, dXe, dXm = tens()
    dq = nn.query_features(dX, dXe, draws='device', key=key)
    assert dq.is_cuda and dq.dtype == torch.float64 and tuple(dq.shape) == (N, 5)
    np.testing.assert_array_equal(dq.cpu().numpy(), nn.query_features(X, Xe, draws='device', key=key))
    out2 = new_out()
    nn.fit_predict(dX, dXe, dXm, z, ze, query_features=dq, out=out2, **kw)
    torch.cuda.synchronize()
    for a, b in zip(out2, out):
        assert torch.equal(a, b)
    # the host form of the public draw on tensors: the stream of rstate.normal, returned on the tensors' device
    hq = nn.query_features(dX, dXe, rstate=np.random.RandomState(4))
    assert hq.is_cuda
    np.testing.assert_array_equal(hq.cpu().numpy(), nn._query_features(X, Xe, np.random.RandomState(4)))
    print("KNN_MC_DEVICE_TENSORS_OK")

    prep = nn.prepare_fit_predict(z, ze, label_grid=grid, k=5)
    dX, dXe, dXm = tens()
    a = prep.run(dX, dXe, dXm, rstate=np.random.RandomState(2), query_draws='device')
    torch.cuda.synchronize()
    for u, v in zip(a, (p, lm, le)):
        np.testing.assert_array_equal(u.cpu().numpy(), v)
    b = prep.run(X.copy(), Xe.copy(), Xm.copy(), rstate=np.random.RandomState(2), query_draws='device')
    for u, v in zip(b, (p, lm, le)):
        np.testing.assert_array_equal(np.asarray(u), v)
    try:
        prep.run(dX, dXe, dXm, query_features=dq, query_draws='device')
        raise AssertionError("query_features with query_draws='device' was accepted")
    except ValueError:
        pass
    print("KNN_MC_PREPARED_OK")

    # fit_sample on device tensors needs no query_features any more; rstate gives the query key first, then the Philox key
    R = np.random.RandomState(9)
    dX, dXe, dXm = tens()
    idx = nn.fit_sample(dX, dXe, dXm, 4, rstate=R, k=5, query_draws='device', verbose=False)
    torch.cuda.synchronize()
    R2 = np.random.RandomState(9)
    k_query = R2.randint(0, 2**32, size=2, dtype=np.uint32)
    k_post = R2.randint(0, 2**32, size=2, dtype=np.uint32)
    np.testing.assert_array_equal(nn.query_key, k_query)
    np.testing.assert_array_equal(nn.philox_key, k_post)
    assert R.rand() == R2.rand()
    R3 = np.random.RandomState(9)
    R3.randint(0, 2**32, size=2, dtype=np.uint32)
    want = nn.fit_sample(X.copy(), Xe.copy(), Xm.copy(), 4, rstate=R3, k=5, verbose=False,
                         query_features=nn.query_features(X, Xe, draws='device', key=k_query))
    np.testing.assert_array_equal(idx.cpu().numpy(), want)
    assert idx.min() >= 0 and idx.max() < M
    try:
        nn.fit_sample(dX, dXe, dXm, 4, k=5, verbose=False)
        raise AssertionError("device objects without features and with the host draw were accepted")
    except NotImplementedError:
        pass
    print("KNN_MC_FIT_SAMPLE_OK")


if __name__ == '__main__':
    main()
