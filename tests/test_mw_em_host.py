"""EM over the model weights (docs/model_weights.md, "EM") without a GPU: the NumPy restatement of the law (tests/_mw_em_ref.py)
against itself and against what exists, the refusals the Python layer raises before it touches a device, and the precondition of
the GPU bars of tests/test_hip_mw_em.py -- how far ANY fp64 realisation of the law may sit from the `longdouble` one."""
import numpy as np
import pytest

import _mw_em_ref as em
import _mw_ref as mw
from conftest import load_golden


def g22_rows():
    return np.ascontiguousarray(load_golden('g22_model_weights')['lnlike'], dtype=np.float64)


def uniform_lnw(M):
    return np.full(M, -np.log(float(M)))


@pytest.mark.parametrize('tag', ['g22', 'sparse20', 'sparse600'])
def test_first_step_from_uniform_weights_is_the_stacked_start(tag):
    from frankenz_amd.samplers import model_weight_sampler
    if tag == 'g22':
        rows, nbr, nnbr = g22_rows(), None, None
        M = rows.shape[1]
    else:
        rows, nbr, nnbr, M, _, _ = mw.chain_problem(tag)
    start = model_weight_sampler(rows, neighbors=nbr, Nneighbors=nnbr, Nmodels=M)._stack_start()
    s = em.step(rows, uniform_lnw(M), M, None, nbr, nnbr)
    got = np.asarray(s['pos'], dtype=np.float64)
    rel = np.abs(got - start).max() / start.max()
    print('largest difference %.2e of the largest weight' % rel)
    np.testing.assert_allclose(got, start, rtol=1e-13, atol=1e-13 * start.max())
    np.testing.assert_allclose(got, mw.stack_start(rows, M, nbr, nnbr), rtol=1e-13, atol=1e-13 * start.max())


def test_rows_that_list_one_model_give_the_bincount():
    rs = np.random.RandomState(31)
    N, M = 1027, 37
    nbr = rs.randint(0, M, size=(N, 1)).astype(np.int64)
    rows, nnbr = np.zeros((N, 1)), np.ones(N, dtype=np.int64)
    s = em.step(rows, uniform_lnw(M), M, None, nbr, nnbr, dtype=np.float64)
    np.testing.assert_array_equal(s['pos'], np.bincount(nbr[:, 0], minlength=M) / float(N))
    assert s['nskip'] == 0


@pytest.mark.parametrize('alpha', [1.0, 1.5])
def test_g22_trace_is_monotone_and_the_fixed_point_is_one(alpha):
    rows = g22_rows()
    N, M = rows.shape
    pos, trace, last = em.iterate(rows, uniform_lnw(M), M, 400, np.full(M, alpha))
    bar = em.lnpost_bar(N, last['ell'])
    inc = np.diff(trace)
    print('alpha %.1f: smallest increase %+.2e nats, bar %.2e' % (alpha, inc.min(), bar))
    assert inc.min() >= -bar
    if alpha == 1.0:
        ell = np.asarray(last['ell'], dtype=np.float64)
        grad = np.exp(rows - ell[:, None]).sum(axis=0) / N
        big = pos > 1e-8
        print('fixed point: |grad - 1| <= %.2e over %d models' % (np.abs(grad[big] - 1.).max(), big.sum()))
        assert np.abs(grad[big] - 1.).max() < 1e-9


def test_a_zero_weight_stays_zero_at_alpha_one():
    rows = g22_rows()
    M = rows.shape[1]
    w = np.ones(M); w[[3, 11]] = 0.
    s = em.step(rows, em.lnw_of(w), M)
    assert s['pos'][3] == 0 and s['pos'][11] == 0 and s['lnw'][3] == -np.inf
    s = em.step(rows, em.lnw_of(w), M, np.full(M, 1.5))
    assert s['pos'][3] > 0 and s['lnpost'] == -np.inf               # the prior pulls it back; ln-posterior of a zero weight


def test_refusals_raised_by_the_python_layer():
    from frankenz_amd.samplers import model_weight_em
    rows = g22_rows()
    M = rows.shape[1]
    e = model_weight_em(rows)
    w = np.ones(M)
    for bad in (np.full(M, 0.5), np.where(np.arange(M) == 2, np.nan, 1.), np.where(np.arange(M) == 2, np.inf, 1.), np.ones(M - 1)):
        with pytest.raises(ValueError):
            e.step(w, alpha=bad)
        with pytest.raises(ValueError):
            e.run(alpha=bad, verbose=False)
    for bad in (np.where(np.arange(M) == 2, -1e-3, 1.), np.zeros(M), np.where(np.arange(M) == 2, np.nan, 1.), np.ones(M + 1)):
        with pytest.raises(ValueError):
            e.step(bad)
        with pytest.raises(ValueError):
            e.loglike(bad)
        with pytest.raises(ValueError):
            e.run(pos_init=bad, verbose=False)
    with pytest.raises(ValueError):
        e.loglike()                                                  # no weights yet
    nbr = np.zeros((len(rows), M), dtype=np.int64)
    with pytest.raises(ValueError):
        model_weight_em(rows, neighbors=nbr)
    with pytest.raises(ValueError):
        model_weight_em(rows, neighbors=nbr, Nneighbors=np.ones(len(rows), dtype=np.int64))       # Nmodels missing


def test_the_fixed_order_sum_is_a_sum():
    from frankenz_amd.samplers import _mw_fixed_sum
    rs = np.random.RandomState(5)
    for n in (1, 255, 256, 257, 70001):
        a = rs.uniform(0., 1., n)
        assert abs(_mw_fixed_sum(a) - float(a.astype(np.longdouble).sum())) <= 4 * n * em.U * a.sum()
    assert _mw_fixed_sum(np.arange(1., 9.)) == 36.


@pytest.mark.parametrize('tag', ['g22', 'sparse65'])
def test_fp64_in_any_order_stays_within_1e13_of_longdouble(tag):
    """the precondition of the GPU bars: per step, and after 60 iterations run side by side"""
    if tag == 'g22':
        rows, nbr, nnbr = g22_rows(), None, None
        M = rows.shape[1]
    else:
        rows, nbr, nnbr, _ = em.em_problem(1027, 65, 300, seed=1)
        M = 300
    rs = np.random.RandomState(17)
    lnw = uniform_lnw(M)
    worst_step = 0.
    lnw64 = lnw.copy()
    for it in range(60):
        ref = em.step(rows, lnw, M, None, nbr, nnbr)
        same = em.step(rows, lnw, M, None, nbr, nnbr, dtype=np.float64, order=rs)
        p = np.asarray(ref['pos'], dtype=np.float64)
        big = p > em.FLOOR
        worst_step = max(worst_step, (np.abs(same['pos'][big] - p[big]) / p[big]).max())
        own = em.step(rows, lnw64, M, None, nbr, nnbr, dtype=np.float64, order=rs)
        lnw, lnw64 = np.asarray(ref['lnw'], dtype=np.float64), own['lnw']
    run = (np.abs(own['pos'][big] - p[big]) / p[big]).max()
    print('%s: %.2e per step, %.2e after 60 iterations' % (tag, worst_step, run))
    assert worst_step <= 1e-13 and run <= 1e-13
