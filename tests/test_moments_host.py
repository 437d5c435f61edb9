"""The law of the posterior moments and of the zero-point iteration (tests/_moments_ref.py, docs/predictive.md) on the CPU: the
`longdouble` loops against dense float64 formulas, the edge rules, the reason the variance is the central form, and the one
statistical assertion of the feature -- the iteration recovers known offsets -- on the reference law over the oracle's planes."""
import os
import sys

import numpy as np

import _moments_ref as mr

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, "oracle"))


def softmax(rows):
    w = np.exp(rows - rows.max(axis=1, keepdims=True))
    return w / w.sum(axis=1, keepdims=True)


def test_law_against_dense_float64():
    rs = np.random.RandomState(1)
    for N, M, L in ((1, 1, 1), (5, 7, 3), (9, 40, 5)):
        rows = -rs.uniform(0., 12., size=(N, M))
        V, Ve = rs.normal(3., 2., size=(M, L)), rs.uniform(0.1, 1., size=(M, L))
        p = softmax(rows)
        mean, var, share, nskip, A = mr.moments_ref(rows, V, Ve)
        mu = p @ V
        np.testing.assert_allclose(mean, mu, rtol=1e-13, atol=1e-13)
        np.testing.assert_allclose(var, np.einsum('ij,ijl->il', p, (V[None] - mu[:, None]) ** 2) + p @ Ve ** 2, rtol=1e-12, atol=1e-13)
        np.testing.assert_array_equal(share, 1.)
        np.testing.assert_allclose(A, p @ np.abs(V), rtol=1e-13)
        assert nskip == 0
        # sparse rows with a scale: the same formula on the gathered tables
        W = min(M, 4)
        nbr = np.array([rs.choice(M, W, replace=False) for _ in range(N)])
        nnbr = rs.randint(1, W + 1, N)
        sc = rs.uniform(0.5, 2., size=(N, W))
        mean, var, share, nskip, _ = mr.moments_ref(rows[:, :W], V, Ve, None, sc, nbr, nnbr)
        for i in range(N):
            n = nnbr[i]
            q = softmax(rows[i:i + 1, :n])[0]
            c = sc[i, :n, None] * V[nbr[i, :n]]
            np.testing.assert_allclose(mean[i], q @ c, rtol=1e-13, atol=1e-13)
            np.testing.assert_allclose(var[i], q @ (c - q @ c) ** 2 + q @ (sc[i, :n, None] * Ve[nbr[i, :n]]) ** 2, rtol=1e-12, atol=1e-13)


def test_edge_rules():
    V = np.array([[1., 10.], [2., 20.], [3., np.inf], [4., 40.]])
    Vm = np.array([[1., 0.], [1., 0.], [1., 0.], [0., 0.]])
    rows = np.array([[0., -1., -2000., -1.],                        # the entry holding inf underflows: w == 0, ignored
                     [0., np.nan, 0., 0.],                         # a nan: no posterior
                     [-np.inf, -np.inf, -np.inf, -np.inf],         # no finite max
                     [0., 0., 0., 0.]])
    mean, var, share, nskip, _ = mr.moments_ref(rows, V)
    assert nskip == 2 and np.isnan(mean[1:3]).all() and np.isnan(var[1:3]).all() and (share[1:3] == 0).all()
    assert np.isfinite(mean[0]).all() and np.isfinite(var[0]).all()
    assert np.isinf(mean[3, 1]) and np.isnan(var[3, 1])            # inf under a positive weight: NumPy's arithmetic
    mean, var, share, nskip, _ = mr.moments_ref(rows[[0, 3]], V, None, Vm)
    assert np.isnan(mean[:, 1]).all() and np.isnan(var[:, 1]).all() and (share[:, 1] == 0).all()      # a column masked everywhere
    w = np.exp(rows[0, [0, 1, 3]])
    np.testing.assert_allclose(share[0, 0], w[:2].sum() / w.sum(), rtol=1e-15)
    np.testing.assert_allclose(mean[0, 0], (w[:2] * [1., 2.]).sum() / w[:2].sum(), rtol=1e-15)
    # n = 0
    nbr = np.zeros((1, 4), dtype=np.int64)
    mean, var, share, nskip, _ = mr.moments_ref(rows[3:], V, neighbors=nbr, nnbr=np.array([0]))
    assert nskip == 1 and np.isnan(mean).all() and (share == 0).all()


def test_raw_moment_form_misses_the_variance_bar():
    rows, V = mr.spread_row()
    mean, var, _, _, A = mr.moments_ref(rows, V)
    p = softmax(rows)[0]
    raw = (p * V[:, 0] ** 2).sum() - (p * V[:, 0]).sum() ** 2
    central = (p * (V[:, 0] - (p * V[:, 0]).sum()) ** 2).sum()
    bar = mr.sum_tol(500) * var[0, 0] + 4. * mr.U * A[0, 0] * np.sqrt(var[0, 0]) + (mr.sum_tol(500) * A[0, 0]) ** 2
    assert abs(central - var[0, 0]) <= bar
    assert abs(raw - var[0, 0]) > 100. * bar


def test_zeropoint_iteration_recovers_known_offsets():
    import frankenz_oracle as fo
    X, Xe, Xm, Y, Ye, Ym = mr.zp_problem()

    def moments(xs, xes, xm):
        rows = fo.bruteforce_fit(xs, xes, xm, Y, Ye, Ym)['lnprob']
        mean, var, _, _, _ = mr.moments_ref(rows, Y, Ye, Ym)
        return mean, var

    keep = X.copy(), Xe.copy(), Xm.copy()
    a, trace, sums, converged = mr.zeropoints_ref(moments, X, Xe, Xm, Niter=10, tol=1e-4, ref_band=0)
    for got, was in zip((X, Xe, Xm), keep):
        np.testing.assert_array_equal(got, was)
    assert converged and len(trace) < 10
    Bb = sums[1].astype(np.float64)
    bar = 5. * a * np.sqrt(1. / Bb + 1. / Bb[0])
    print("iterations", len(trace), "offsets", a, "errors in units of the bar", np.abs(a - mr.ZP_OFFSETS / mr.ZP_OFFSETS[0]) / np.maximum(bar, 1e-300))
    assert a[0] == 1.
    assert (np.abs(a - mr.ZP_OFFSETS / mr.ZP_OFFSETS[0])[1:] <= bar[1:]).all()
