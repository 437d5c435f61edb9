"""The model-weight sampler without a GPU (docs/model_weights.md): the NumPy law of tests/_mw_ref.py against the draw definition, the
Philox gamma twin against scipy's gamma law, the precondition of the GPU chain tests, the NumPy draws='host' chain against the
reference's chains (golden g22), and the refusals the Python layer makes before any library call."""
import numpy as np
import pytest

import _draw_ref as dr
import _mw_ref as mw
from conftest import load_golden

GAMMA_KEY = (0x243F6A88, 0x85A308D3)       # the first 64 fractional bits of pi: fixed here, not picked by trying


def test_law_agrees_with_the_draw_definition_on_pre_added_rows():
    for N, W, M in ((5, 3, 40), (37, 257, 700), (9, 600, 900)):
        rows, nbr, nnbr, lnw, u = mw.sparse_problem(N, W, M)
        t = mw.added_rows(rows, lnw, nbr, nnbr)
        ref = dr.draw_ref(t, u[:, None], nbr, nnbr)[0][:, 0]
        assign, counts = mw.sweep_ref(rows, lnw, u, M, nbr, nnbr)
        np.testing.assert_array_equal(assign, ref)
        np.testing.assert_array_equal(counts, np.bincount(ref[ref >= 0], minlength=M))
        assert counts.sum() == (ref >= 0).sum() and (N <= 3 or assign[3] == -1)                 # Nneighbors == 0
        assert counts[M // 2] == 0                                                            # the model at weight 0 is never drawn
        # the device's segmented order lands every draw on the definition's entry
        np.testing.assert_array_equal(mw.sweep_ref(rows, lnw, u, M, nbr, nnbr, draw=dr.draw_segmented)[0], ref)
        assert mw.near_share(rows, lnw, u, nbr, nnbr) <= dr.NEAR_CAP
    # dense rows, a nan row, a row whose models all have weight 0
    rs = np.random.RandomState(3)
    rows = -rs.uniform(0, 12, (6, 50)); lnw = -rs.uniform(0, 3, 50)
    rows[1, 7] = np.nan
    rows[2, :] = -np.inf; rows[2, 4] = 0.; lnw[4] = -np.inf
    u = rs.rand(6)
    assign, counts = mw.sweep_ref(rows, lnw, u, 50)
    assert assign[1] == -1 and assign[2] == -1 and (assign[[0, 3, 4, 5]] >= 0).all() and counts.sum() == 4
    np.testing.assert_array_equal(assign, dr.draw_ref(rows + lnw[None, :], u[:, None])[0][:, 0])
    for a, b in zip(mw.sweep_dense(rows, lnw, u), (assign, counts)):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize('shape', [0.05, 0.5, 1., 3.7, 1000.])
def test_philox_gamma_twin_follows_the_gamma_law(shape):
    """KS distance to scipy.stats.gamma below 2.23 / sqrt(n) at n = 1e5: the 1e-4 level per shape"""
    from scipy import stats
    from frankenz_amd.samplers import _philox_gamma
    n = 100000
    g, att = _philox_gamma(GAMMA_KEY, 0, np.full(n, shape), return_attempts=True)
    d = stats.kstest(g, 'gamma', args=(shape,)).statistic
    print('shape %g: KS distance %.3g (bar %.3g), most attempts %d' % (shape, d, 2.23 / np.sqrt(n), att.max()))
    assert d < 2.23 / np.sqrt(n)
    assert (g > 0).all() and att.max() < 20


def test_philox_gamma_twin_counters():
    from frankenz_amd.samplers import _philox_gamma, _philox_uniform
    a = np.array([0.3, 1., 2.5, 40.])
    g = _philox_gamma(GAMMA_KEY, 5, a)
    np.testing.assert_array_equal(g, _philox_gamma(GAMMA_KEY, 5, a))
    np.testing.assert_array_equal(g[:2], _philox_gamma(GAMMA_KEY, 5, a[:2]))                   # a draw depends on (key, model, sweep, shape) alone
    assert not np.array_equal(g, _philox_gamma(GAMMA_KEY, 6, a))
    assert not np.array_equal(g, _philox_gamma((GAMMA_KEY[0], GAMMA_KEY[1] ^ 1), 5, a))
    # the key domain is not the sweep's: the gamma key differs from the chain's in its second word
    from frankenz_amd import samplers
    assert samplers._MW_KEY_XOR == 0x6D775F67 and _philox_uniform(GAMMA_KEY, 5, 4).shape == (4,)
    with pytest.raises(ValueError):
        _philox_gamma(GAMMA_KEY, 0, np.array([1., 0.]))
    with pytest.raises(ValueError):
        _philox_gamma(GAMMA_KEY, 0, np.array([np.inf]))


@pytest.mark.parametrize('tag', mw.CHAIN_TAGS)
def test_precondition_of_the_gpu_chain_tests(tag):
    """over every sweep of the draws='host' test chains no u tot lies within 1e-12 (relative) of a cdf value: the GPU may be compared
    count for count.  Allowed share 1 %; expected, and found, 0."""
    rows, nbr, nnbr, M, alpha, seed = mw.chain_problem(tag)
    counts, pos, worst = mw.chain_host(rows, M, alpha, mw.stack_start(rows, M, nbr, nnbr), np.random.RandomState(seed), mw.CHAIN_SWEEPS, nbr, nnbr)
    print('%s: largest share of close draws over %d sweeps: %g' % (tag, mw.CHAIN_SWEEPS, worst))
    assert worst <= dr.NEAR_CAP
    assert counts.shape == (mw.CHAIN_SWEEPS, M) and (counts.sum(axis=1) == (nnbr > 0).sum()).all()


@pytest.mark.parametrize('tag', ['a1', 'a03'])
def test_numpy_host_chain_against_the_reference_chains(tag):
    g = load_golden('g22_model_weights')
    lnlike, alpha, ref = g['lnlike'], g[tag + '_alpha'], g[tag + '_samples']
    N, M = lnlike.shape
    niter, thin = ref.shape[0], 5
    counts, pos, worst = mw.chain_host(lnlike, M, alpha, mw.stack_start(lnlike, M), np.random.RandomState(2220 + len(tag)), 1 + niter * thin,
                                       check_near=False)
    mw.golden_chain_check(pos[thin::thin], ref, N)


def test_refusals_without_a_library_call():
    from frankenz_amd import model_weight_sampler
    r = np.zeros((4, 6))
    with pytest.raises(ValueError):
        model_weight_sampler(r, neighbors=np.zeros((4, 6), dtype=np.int64))                 # neighbors without Nneighbors
    with pytest.raises(ValueError):
        model_weight_sampler(r, neighbors=np.zeros((4, 6), dtype=np.int64), Nneighbors=np.zeros(4, dtype=np.int64))    # no Nmodels
    with pytest.raises(ValueError):
        model_weight_sampler(r, neighbors=np.zeros((4, 5), dtype=np.int64), Nneighbors=np.zeros(4, dtype=np.int64), Nmodels=9)
    with pytest.raises(ValueError):
        model_weight_sampler(r, Nmodels=7)
    with pytest.raises(ValueError):
        model_weight_sampler(np.zeros(6))
    s = model_weight_sampler(r)
    assert (s.NOBJ, s.W, s.NMODEL) == (4, 6, 6) and s.results[0].shape == (0,)
    for kw in (dict(draws='neither'), dict(thin=0), dict(alpha=np.zeros(6)), dict(alpha=np.full(6, np.nan)), dict(alpha=np.ones(5)),
               dict(pos_init=np.array([1., -1., 0, 0, 0, 0])), dict(pos_init=np.array([np.nan, 1., 0, 0, 0, 0])), dict(pos_init=np.ones(5))):
        with pytest.raises(ValueError):
            next(s.sample(1, **kw))
    with pytest.raises(ValueError):
        s.logwt()                                                                             # no samples, no w
    np.testing.assert_array_equal(s.logwt(np.full(6, 0.5)), r + np.log(0.5))
    # the default start is the stacked normalised rows
    rows, nbr, nnbr, _, _ = mw.sparse_problem(9, 5, 30)
    s = model_weight_sampler(rows, neighbors=nbr, Nneighbors=nnbr, Nmodels=30)
    np.testing.assert_allclose(s._stack_start(), mw.stack_start(rows, 30, nbr, nnbr), rtol=1e-13, atol=1e-16)
    lw = s.logwt(np.linspace(0.1, 1., 30))
    np.testing.assert_array_equal(lw, mw.added_rows(rows, np.log(np.linspace(0.1, 1., 30)), nbr, nnbr))
    import torch                                                                              # tensors in, a tensor out, the same values
    st = model_weight_sampler(torch.from_numpy(rows), neighbors=torch.from_numpy(nbr), Nneighbors=torch.from_numpy(nnbr), Nmodels=30)
    lt = st.logwt(np.linspace(0.1, 1., 30))
    assert isinstance(lt, torch.Tensor)
    np.testing.assert_array_equal(lt.numpy(), lw)
    # device arrays are read as raw C-contiguous 8-byte items: a strided view or the wrong dtype is refused before any library call,
    # and an array that is already resident is not held against the workspace limit
    class NoRoom(object):
        def workspace_limit(self):
            return 8
    t = torch.zeros((4, 12), dtype=torch.float64)
    with pytest.raises(ValueError, match='contiguous'):
        model_weight_sampler(t[:, ::2])._resident(NoRoom())
    with pytest.raises(TypeError):
        model_weight_sampler(torch.zeros((4, 6), dtype=torch.int64))._resident(NoRoom())
    with pytest.raises(TypeError):
        model_weight_sampler(torch.zeros((4, 6), dtype=torch.float32))._resident(NoRoom())
    assert model_weight_sampler(t)._resident(NoRoom())[0] is t
    with pytest.raises(MemoryError, match='%d bytes' % (4 * 6 * 8)):
        model_weight_sampler(np.zeros((4, 6)))._resident(NoRoom())
    from frankenz_amd.samplers import _mw_lnpost
    from scipy import stats
    c, p, a = np.array([3, 0, 5, 2]), np.array([0.3, 0.1, 0.4, 0.2]), np.array([0.5, 1., 2., 1.5])
    np.testing.assert_allclose(_mw_lnpost(c, p, a), stats.multinomial.logpmf(c, 10, p) + stats.dirichlet.logpdf(p, a), rtol=1e-13)
