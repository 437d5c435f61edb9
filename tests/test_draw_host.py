"""Posterior draws over the model set, the part that needs no GPU: the NumPy definition (tests/_draw_ref.py) against an independent
restatement, ``pdf.sample_labels``, the Philox twin at (object, draw) counters, the refusals made before any device call -- and
the precondition of tests/test_hip_draw.py, from the oracle alone: on every problem the GPU tests draw from, the draws whose
u tot lies within the rows' tolerance of a cdf value (the only ones an index may legitimately flip on) are at most 1 %."""
import numpy as np
import pytest

import _draw_ref as dr


def test_definition_against_searchsorted():
    for L, S, N in dr.HAND_CASES:
        rows, u = dr.hand_rows(L, S, N)
        idx, lmap, levid = dr.draw_ref(rows, u)
        np.testing.assert_array_equal(idx, dr.draw_ref_searchsorted(rows, u))
        assert idx.min() >= 0 and idx.max() < L
        w = np.exp(rows - rows.max(axis=1, keepdims=True))
        assert (w[np.arange(N)[:, None], idx] > 0).all()                       # zero-weight stretches are skipped
        first = np.array([np.nonzero(r > 0)[0][0] for r in w]); last = np.array([np.nonzero(r > 0)[0][-1] for r in w])
        np.testing.assert_array_equal(idx[0::2, 0], first[0::2])               # u = 0: the first entry with mass
        top = u[:, -1] == dr.TOP
        np.testing.assert_array_equal(idx[top, -1], last[top])
        np.testing.assert_allclose(levid, np.log(np.exp(rows - lmap[:, None]).sum(axis=1)) + lmap, rtol=1e-12)
    rows, u = dr.no_posterior_rows()
    idx, lmap, levid = dr.draw_ref(rows, u)
    assert (idx[:3] == -1).all() and (idx[3] >= 0).all()
    assert lmap[0] == -np.inf and np.isnan(lmap[1]) and lmap[2] == np.inf
    np.testing.assert_array_equal(idx, dr.draw_ref_searchsorted(rows, u))


def test_definition_maps_neighbours_and_stops_at_the_count():
    rs = np.random.RandomState(3)
    N, W, S = 9, 20, 33
    rows = -rs.uniform(0, 12, (N, W)); nnbr = rs.randint(0, W + 1, N); nnbr[0] = 0; nnbr[1] = W
    nbr = np.array([rs.permutation(1000)[:W] for _ in range(N)])
    for i in range(N):
        rows[i, nnbr[i]:] = 5.                     # padding that would win if it were read
    u = rs.rand(N, S)
    idx, lmap, levid = dr.draw_ref(rows, u, nbr, nnbr)
    assert (idx[0] == -1).all()
    for i in range(1, N):
        assert set(idx[i]) <= set(nbr[i, :nnbr[i]])
    np.testing.assert_array_equal(idx, dr.draw_ref_searchsorted(rows, u, nbr, nnbr))
    np.testing.assert_array_equal(lmap[1:], [rows[i, :nnbr[i]].max() for i in range(1, N)])


def test_hand_made_rows_meet_the_precondition():
    for L, S, N in dr.HAND_CASES:
        rows, u = dr.hand_rows(L, S, N)
        share = dr.near(rows, u, dr.SUM_TOL).mean()
        print('L %d S %d N %d: %.4f of the draws within %g tot of a cdf value' % (L, S, N, share, dr.SUM_TOL))
        assert share <= dr.NEAR_CAP


@pytest.mark.parametrize('case', dr.FIT_CASES, ids=dr.fit_id)
def test_fitted_problems_meet_the_precondition(case):
    p = dr.fit_problem(case)
    assert np.isfinite(p['lmap']).all() and (p['idx'] >= 0).all()
    for rel in (dr.FIT_TOL, dr.SUM_TOL):
        share = dr.near(p['rows'], p['u'], rel).mean()
        print('%s: %.4f of the draws within %g tot of a cdf value' % (dr.fit_id(case), share, rel))
        assert share <= dr.NEAR_CAP
    assert len(np.unique(p['idx'])) > 1


def test_added_problems_meet_the_precondition():
    import frankenz_oracle as fo
    for B in (5, 12, 32):
        X, Xe, Xm, Y, Ye, Ym, u = dr.masked_problem(B)
        rows = fo.bruteforce_fit(X.copy(), Xe.copy(), Xm.copy(), Y, Ye, Ym)['lnprob']
        assert dr.near(rows, u, dr.FIT_TOL).mean() <= dr.NEAR_CAP
    X, Xe, Xm, Y, Ye, Ym, tab, prow, vals, grid, coord, u = dr.prior_problem()
    rows = fo.bruteforce_fit(X.copy(), Xe.copy(), Xm.copy(), Y, Ye, Ym, lnprior=tab[prow])['lnprob']
    assert dr.near(rows, u, dr.FIT_TOL).mean() <= dr.NEAR_CAP
    from frankenz_amd.pdf import lerp_cells
    r, f = lerp_cells(grid, coord)
    lp = np.log((1 - f)[:, None] * vals[r] + f[:, None] * vals[r + 1])
    rows = fo.bruteforce_fit(X.copy(), Xe.copy(), Xm.copy(), Y, Ye, Ym, lnprior=lp)['lnprob']
    assert dr.near(rows, u, dr.FIT_TOL).mean() <= dr.NEAR_CAP


def test_the_segmented_order_draws_what_the_definition_draws():
    """the summation order of the kernel (restated in NumPy) lands every draw of every problem on the definition's entry"""
    for L, S, N in dr.HAND_CASES:
        rows, u = dr.hand_rows(L, S, N)
        dr.assert_draws(dr.draw_segmented(rows, u), dr.draw_ref(rows, u)[0], rows, dr.near(rows, u, dr.SUM_TOL))
    rows, u = dr.no_posterior_rows()
    np.testing.assert_array_equal(dr.draw_segmented(rows, u), dr.draw_ref(rows, u)[0])
    for case in dr.FIT_CASES:
        p = dr.fit_problem(case)
        dr.assert_draws(dr.draw_segmented(p['rows'], p['u']), p['idx'], p['rows'], dr.near(p['rows'], p['u'], dr.SUM_TOL))


def test_sample_labels():
    from frankenz_amd import pdf
    labels = np.array([0.5, 1.5, 2.5, 3.5]); errs = np.array([0., 0.1, 0.2, 0.3])
    idx = np.array([[0, 3, 3], [-1, -1, -1], [2, 1, 0]])
    out = pdf.sample_labels(idx, labels)
    np.testing.assert_array_equal(out[[0, 2]], labels[idx[[0, 2]]])
    assert np.isnan(out[1]).all() and out.shape == idx.shape
    np.testing.assert_array_equal(pdf.sample_labels(idx, labels, errs), out)          # errors without a generator: no jitter
    j = pdf.sample_labels(idx, labels, errs, np.random.RandomState(4))
    ref = np.random.RandomState(4).normal(labels[np.where(idx < 0, 0, idx)], errs[np.where(idx < 0, 0, idx)])
    np.testing.assert_array_equal(j[[0, 2]], ref[[0, 2]])
    assert np.isnan(j[1]).all() and j[0, 0] == 0.5 and j[0, 1] != 3.5
    with pytest.raises(IndexError):
        pdf.sample_labels(np.array([4]), labels)
    with pytest.raises(ValueError):
        pdf.sample_labels(np.array([0.5]), labels)
    z = pdf.sample_labels(idx, np.stack([labels, -labels], axis=1))                    # any label, vector labels included
    assert z.shape == (3, 3, 2) and np.isnan(z[1]).all()


def test_philox_twin_at_object_draw_counters():
    """draw s of object i reads Philox at the counter (i, s): ``samplers._philox_uniform(key, s, n)[i]``, whatever n is, and a
    different number for every (i, s)"""
    from frankenz_amd.samplers import _philox4x32, _philox_uniform
    key = np.array([0xA4093822, 0x299F31D0], dtype=np.uint32)
    u = np.stack([_philox_uniform(key, s, 50) for s in range(7)], axis=1)
    assert ((u >= 0) & (u < 1)).all() and len(np.unique(u)) == u.size
    np.testing.assert_array_equal(_philox_uniform(key, 5, 9), u[:9, 5])
    big = (1 << 33) + 5                                                                # an object index beyond 32 bits: the high word counts
    lo = _philox4x32(key, np.array([[5, 0, 3, 0]], dtype=np.uint64))[0]
    hi = _philox4x32(key, np.array([[big & 0xFFFFFFFF, big >> 32, 3, 0]], dtype=np.uint64))[0]
    assert (lo != hi).any()
    np.testing.assert_array_equal(_philox_uniform(key, 3, 6)[5], ((lo[0] >> np.uint32(5)) * 67108864.0 + (lo[1] >> np.uint32(6))) / 2.0 ** 53)


def test_refusals_before_any_device_call():
    from frankenz_amd import BruteForce, NearestNeighbors
    from frankenz_amd.bruteforce import _draw_uniforms
    ones = np.ones((4, 5))
    bf = BruteForce(ones, ones, ones)
    for bad in (0, -3, 2.5):
        with pytest.raises(ValueError, match='Nsamples'):
            bf.fit_sample(ones[:2], ones[:2], ones[:2], bad, verbose=False)
        with pytest.raises(ValueError, match='Nsamples'):
            bf.sample(bad, logwt=np.zeros((2, 4)))
    with pytest.raises(ValueError, match='Fits have not been computed'):
        bf.sample(3)
    with pytest.raises(ValueError, match='draws'):
        bf.sample(3, logwt=np.zeros((2, 4)), draws='gpu')
    with pytest.raises(ValueError, match='logwt'):
        bf.sample(3, logwt=np.zeros(4))
    with pytest.raises(ValueError):
        bf.fit_sample(ones[:2], ones[:2], ones[:2], 3, lprob_func='not callable', verbose=False)
    with pytest.raises(NotImplementedError):
        bf.fit_sample(ones[:2], ones[:2], ones[:2], 3, lprob_func=lambda *a: None, out=(np.zeros((2, 3), dtype=np.int64),), verbose=False)
    nn = NearestNeighbors.__new__(NearestNeighbors)
    nn.fit_lnprob = nn.neighbors = None
    with pytest.raises(ValueError, match='Fits have not been computed'):
        nn.sample(3)
    # the two sources consume the generator as documented
    rs = np.random.RandomState(11)
    u, key = _draw_uniforms(rs, 'host', 3, 4)
    assert key is None
    np.testing.assert_array_equal(u, np.random.RandomState(11).rand(3, 4))
    u, key = _draw_uniforms(np.random.RandomState(11), 'device', 3, 4)
    assert u is None
    np.testing.assert_array_equal(key, np.random.RandomState(11).randint(0, 2**32, size=2, dtype=np.uint32))
