"""Posterior scoring rules on the GPU (csrc/fz_scores.h, docs/scores.md): k_scores_stage and k_scores_pairs against the law as
tests/_scores_ref.py restates it in longdouble, at the bars of docs/scores.md section 2 (tests/test_scores_host.py checks their
precondition on the same inputs); the hand rows of the point-mass rules, the identities, the bit-for-bit properties, the three fitters,
the cap on the pair sums and every refusal.  assert_scores prints the worst case of each result as a share of its bar."""
import functools
import time

import numpy as np
import pytest

import _bins_ref as br
import _draw_ref as dr
import _scores_ref as sr
from conftest import DevArray

pytestmark = pytest.mark.gpu

ALL = ('lnpdf', 'crps', 'spread', 'sqnorm', 'ninc')
SQPI = np.sqrt(np.pi)


def engine():
    from frankenz_amd.engine import get_engine
    return get_engine()


def scores(rows, y, s, x, nbr=None, nnbr=None, wt_thresh=1e-3, want=ALL):
    """pdf.posterior_scores -> the dict with nskip in it"""
    from frankenz_amd import pdf
    out, info = pdf.posterior_scores(rows, y, s, x, neighbors=nbr, Nneighbors=nnbr, wt_thresh=wt_thresh, want=want, return_info=True)
    out['nskip'] = info['nskip']
    return out


def same_bits(a, b, keys=ALL):
    for k in keys:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def dev_numpy(d, shape, dtype=np.float64):
    """a DevArray's contents"""
    import ctypes as C
    out = np.empty(shape, dtype=dtype)
    assert DevArray._hip.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(d.data_ptr()), C.c_size_t(out.nbytes), 2) == 0
    return out


# ---- given rows ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,k,zeros", sr.WIDTH_CASES)
def test_sparse_rows_every_width(W, k, zeros):
    rows, nbr, nnbr, y, s, x = sr.width_case(W, k, zeros)
    for wt in (1e-3, None) if W <= 257 else (1e-3,):
        ref = sr.ref_cached('width', W, k, zeros, wt)
        got = scores(rows, y, s, x, nbr, nnbr, wt_thresh=wt)
        sr.assert_scores(got, ref, W, "W = %d, M = %d, wt_thresh = %r" % (W, len(y), wt))
        assert got['nskip'] == ref['nskip'] >= 1                     # the row with no entry
        assert got['lnpdf'].shape == got['crps'].shape == (5, 3) and got['spread'].shape == got['sqnorm'].shape == (5,)
        if zeros and W >= 63:
            assert np.isinf(got['sqnorm']).any()


@pytest.mark.parametrize("M", sr.DENSE + sr.DENSE4)
def test_dense_rows_through_both_geometries(M):
    rows, y, s, x = (sr.dense_case if M in sr.DENSE else sr.dense4_case)(M)
    ref = sr.ref_cached('dense' if M in sr.DENSE else 'dense4', M)
    got = scores(rows, y, s, x)                                      # one truth per object
    assert got['lnpdf'].shape == got['crps'].shape == (len(rows),) and got['nskip'] == 0
    sr.assert_scores(got, ref, M, "dense M = %d" % M)
    if M in sr.DENSE4:
        assert (got['ninc'] > 500).all() and (got['ninc'] < 700).all()


@pytest.mark.parametrize("wpo,W", [(4, 65), (4, 257), (1, 4097)])
def test_the_geometry_the_rule_would_not_choose(wpo, W, monkeypatch):
    """FZ_DRAW_WPO forces four waves per object on short rows (at 65 the last two waves own no entry and no tile) and one wave on the
    first row too long for it by default"""
    monkeypatch.setenv('FZ_DRAW_WPO', str(wpo))
    if wpo == 4:
        for k, zeros in sr.CASES:
            rows, nbr, nnbr, y, s, x = sr.width_case(W, k, zeros)
            sr.assert_scores(scores(rows, y, s, x, nbr, nnbr), sr.ref_cached('width', W, k, zeros, 1e-3), W, "WPO = 4, W = %d" % W)
    else:
        rows, y, s, x = sr.dense4_case(4097)
        sr.assert_scores(scores(rows, y, s, x), sr.ref_cached('dense4', 4097), W, "WPO = 1, W = 4097")
    monkeypatch.delenv('FZ_DRAW_WPO')


@pytest.mark.parametrize("P", sr.PCOUNTS)
def test_point_counts_on_both_sides_of_a_pass_shared_and_per_object(P):
    rows, nbr, nnbr, y, s, x = sr.pcount_case(P)
    got = scores(rows, y, s, x, nbr, nnbr)
    assert got['lnpdf'].shape == (5, P)
    sr.assert_scores(got, sr.ref_cached('pcount', P), 65, "P = %d" % P)
    shared = scores(rows, y, s, x[:1].copy(), nbr, nnbr)              # (1, P): shared by all objects
    same_bits(shared, scores(rows, y, s, np.tile(x[0], (5, 1)), nbr, nnbr))
    same_bits(shared, got, ('spread', 'sqnorm', 'ninc'))
    np.testing.assert_array_equal(shared['crps'][0], got['crps'][0])


@functools.lru_cache(maxsize=None)
def block_full():
    """the scores of sr.block_case's 257 rows in one call"""
    rows, nbr, nnbr, y, s, x = sr.block_case()
    return scores(rows, y, s, x, nbr, nnbr)


@pytest.mark.parametrize("N", (1, 3, 4, 5, 257))
def test_object_counts_around_a_block_of_four(N):
    rows, nbr, nnbr, y, s, x = sr.block_case()
    full = block_full()
    got = scores(rows[:N], y, s, x[:N], nbr[:N], nnbr[:N]) if N < 257 else full
    same_bits(got, {k: full[k][:N] for k in ALL})
    n = min(N, sr.BLOCK_REF)
    ref = sr.ref_cached('block')
    sr.assert_scores({k: got[k][:n] for k in ALL}, {k: (v[:n] if isinstance(v, np.ndarray) else v) for k, v in ref.items()}, 65, "N = %d" % N)


# ---- hand rows -------------------------------------------------------------------------------------------------------------------
def test_the_cut_is_strict_and_in_ln_space():
    y, s = np.array([0., 100.]), np.array([0.1, 0.1])
    cut = np.log(1e-3)
    rows = np.array([[0., cut], [0., np.nextafter(cut, 0.)]])
    x = np.array([0.05, 100.])
    xs = x[None, :]                                                  # (1, 2): shared by the two objects, and the one object's own
    got = scores(rows, y, s, xs)
    np.testing.assert_array_equal(got['ninc'], [1, 2])               # exactly at the cut: excluded
    same_bits({k: got[k][:1] for k in ALL}, scores(np.array([[0., -np.inf]]), y, s, xs))
    sr.assert_scores(got, sr.scores_ref(rows, y, s, x), 2, "the cut")
    got = scores(rows, y, s, xs, wt_thresh=None)
    np.testing.assert_array_equal(got['ninc'], [2, 2])
    sr.assert_scores(got, sr.scores_ref(rows, y, s, x, wt_thresh=None), 2, "no cut")


def test_point_masses_equal_labels_and_rows_without_a_posterior():
    y, s = np.array([1., 4., 2., 1.]), np.array([0., 0., 0.5, 0.])
    rows = np.array([[np.log(0.25), 0., -np.inf, -np.inf], [0., 0., 0., -np.inf], [0., -np.inf, -np.inf, 0.], [-np.inf] * 4,
                     [0., np.nan, 0., 0.]])
    x = np.array([1., 2., 4., 5.])
    got = scores(rows, y, s, x, wt_thresh=None)
    ref = sr.scores_ref(rows, y, s, x, wt_thresh=None)
    sr.assert_scores(got, ref, 4, "point masses")
    assert got['nskip'] == 2 and all(np.isnan(got[k][3:]).all() for k in ALL[:4]) and (got['ninc'][3:] == 0).all()
    np.testing.assert_array_equal(got['lnpdf'][0], [np.inf, -np.inf, np.inf, -np.inf])     # all s == 0
    assert (got['sqnorm'][:3] == np.inf).all()
    assert got['lnpdf'][1, 0] == np.inf and got['lnpdf'][1, 2] == np.inf and np.isfinite(got['lnpdf'][1, [1, 3]]).all()
    np.testing.assert_allclose(got['crps'][2], np.abs(x - 1.), rtol=0, atol=1e-15)          # two equal point masses are one
    assert got['spread'][2] == 0.
    # an error whose square is 0 in float64 is a point mass in both kernels: the same bits as s == 0; the next larger one is a Gaussian
    t = s.copy(); t[s == 0] = 2. ** -538
    same_bits(scores(rows, y, t, x, wt_thresh=None), got)
    t[s == 0] = 2. ** -536
    narrow = scores(rows[:3], y, t, x, wt_thresh=None)
    assert np.isfinite(narrow['sqnorm']).all() and (narrow['sqnorm'] > 1e150).all()
    sr.assert_scores(narrow, sr.scores_ref(rows[:3], y, t, x, wt_thresh=None), 4, "errors just above the point-mass rule")
    # weights whose products underflow leave no nan behind a point mass
    tiny = scores(np.array([[0., -400., -400., -400.]]), y, s, x, wt_thresh=None)
    assert tiny['sqnorm'][0] == np.inf and np.isfinite(tiny['crps']).all() and tiny['ninc'][0] == 4
    rows4, _ = dr.no_posterior_rows(257)
    e = br.edges_case(8, 4)
    y4, s4 = br.labels_case(257, e, 4)
    got = scores(rows4, y4, s4, np.full(4, 3.))
    assert got['nskip'] == 3 and np.isnan(got['crps'][:3]).all() and np.isfinite(got['crps'][3])
    sr.assert_scores(got, sr.scores_ref(rows4, y4, s4, np.full((4, 1), 3.)), 257, "no posterior")


def test_single_components_against_their_closed_forms():
    y, s = np.array([3., -2., 1e3]), np.array([0.25, 1e-6, 40.])
    rows = np.full((3, 3), -np.inf)
    rows[np.arange(3), np.arange(3)] = 0.
    x = np.array([[3.1, 2.], [-2., -2. + 3e-6], [900., 1e3]])
    got = scores(rows, y, s, x)
    sr.assert_scores(got, sr.scores_ref(rows, y, s, x), 3, "one entry")
    for i in range(3):
        A, _ = sr.A_G(x[i] - y[i], s[i] ** 2)
        np.testing.assert_allclose(got['crps'][i], (A - sr.LD(s[i]) / np.sqrt(sr.PI)).astype(np.float64), rtol=0, atol=2 * sr.bar_sum(1) * float(A.max()))
        assert got['spread'][i] == pytest.approx(s[i] / SQPI, rel=sr.bar_sum(1))
        assert got['sqnorm'][i] == pytest.approx(1. / (2. * s[i] * SQPI), rel=sr.bar_sum(1))


# ---- identities ------------------------------------------------------------------------------------------------------------------
def test_crps_is_not_negative_and_the_spread_does_not_depend_on_the_entry_order():
    rows, nbr, nnbr, y, s, x = sr.width_case(500, 1, True)
    ref = sr.ref_cached('width', 500, 1, True, 1e-3)
    b = sr.bars(ref, 500)
    got = scores(rows, y, s, x, nbr, nnbr)
    ok = np.isfinite(ref['crps'])
    assert (got['crps'][ok] >= -b['crps'][ok]).all()
    rs = np.random.RandomState(3)
    rp, np_ = rows.copy(), nbr.copy()
    for i in range(len(rows)):
        o = rs.permutation(int(nnbr[i]))
        rp[i, :len(o)], np_[i, :len(o)] = rows[i, o], nbr[i, o]
    perm = scores(rp, y, s, x, np_, nnbr)
    np.testing.assert_array_equal(perm['ninc'], got['ninc'])
    for k in ('spread', 'crps'):
        okk = np.isfinite(ref[k])
        share = np.max(np.abs(perm[k][okk] - got[k][okk]) / np.maximum(b[k][okk], 1e-300))
        print("permuted entries: %s differs by %.3g of its bar" % (k, share))
        assert share <= 1., k


def test_density_against_a_central_difference_of_posterior_cdf():
    """C(x + h) - C(x - h) = 2 h p(x) + h^3 p'''(xi) / 3: with every s >= smin the third derivative of the mixture density is at most
    max |(3 z - z^3) phi(z)| / smin^4 = 0.5506 / smin^4, so that |dC / 2h - p| <= h^2 0.5506 / (6 smin^4) + tol(W) / h, the second term
    the bar of the two CDF values.  smin = 0.1, h = 1e-3: 9.2e-4 + 1e-11."""
    from frankenz_amd import pdf
    rs = np.random.RandomState(11)
    N, W, M, smin, h = 6, 300, 1000, 0.1, 1e-3
    rows, nbr, nnbr = br.sparse_case(N, W, M, 21, counts=[])
    y, s = rs.uniform(0., 6., M), rs.uniform(smin, 0.5, M)
    x = rs.uniform(0.5, 5.5, N)
    got = scores(rows, y, s, x, nbr, nnbr, want=('lnpdf',))
    C = pdf.posterior_cdf(rows, y, s, np.stack((x - h, x + h), axis=1), neighbors=nbr, Nneighbors=nnbr)
    dens = (C[:, 1] - C[:, 0]) / (2. * h)
    tolr = h * h * 0.5506 / (6. * smin ** 4) + br.tol(W) / h
    err = np.abs(np.exp(got['lnpdf']) - dens)
    print("central difference: worst %.3g of the tolerance %.3g" % (err.max() / tolr, tolr))
    assert (err <= tolr).all() and np.median(dens) > 0.1             # (densities the tolerance is small against)


def test_want_subsets_give_the_same_bits():
    rows, nbr, nnbr, y, s, x = sr.width_case(257, 1, True)
    full = scores(rows, y, s, x, nbr, nnbr)
    for want in (('lnpdf',), ('crps',), ('spread',), ('sqnorm',), ('ninc',), ('lnpdf', 'crps', 'sqnorm'), ('sqnorm', 'ninc'), 'crps'):
        got = scores(rows, y, s, x, nbr, nnbr, want=want)
        keys = (want,) if isinstance(want, str) else want
        assert set(got) == set(keys) | {'nskip'}
        same_bits(got, full, keys)
        assert got['nskip'] == full['nskip']


# ---- reproducibility -------------------------------------------------------------------------------------------------------------
def test_same_bits_chunked_device_resident_and_in_reversed_order():
    from frankenz_amd import pdf
    N, W, M, P = 700, 257, 1000, 3
    rows, nbr, nnbr, y, s, x = sr.bits_case()
    base = scores(rows, y, s, x, nbr, nnbr)
    sr.assert_scores({k: base[k][:sr.BITS_REF] for k in ALL}, sr.ref_cached('bits'), W, "700 rows (the first 12)")
    eng = engine()
    old = eng.workspace_limit()
    eng.set_workspace_limit(1 << 21)                                 # 10 392 bytes per object, 6 168 of them the compacted records: four chunks
    try:
        small = scores(rows, y, s, x, nbr, nnbr)
    finally:
        eng.set_workspace_limit(old)
    same_bits(small, base)
    assert small['nskip'] == base['nskip']
    # device-resident arguments and results
    d_rows, d_nbr, d_nn, d_y, d_s, d_x = (DevArray(a) for a in (rows, nbr, nnbr, y, s, x))
    outs = dict(lnpdf=DevArray(np.zeros((N, P))), crps=DevArray(np.zeros((N, P))), spread=DevArray(np.zeros(N)), sqnorm=DevArray(np.zeros(N)),
                ninc=DevArray(np.zeros(N, dtype=np.int64)))
    ns = eng.row_scores(d_rows, N, W, M, d_y, d_s, d_x, P, per_object=True, lncut=np.log(1e-3), neighbors=d_nbr, nnbr=d_nn, **outs)
    assert ns == base['nskip']
    for k in ALL:
        np.testing.assert_array_equal(dev_numpy(outs[k], base[k].shape, base[k].dtype), base[k], err_msg=k)
    same_bits(scores(d_rows, d_y, d_s, d_x, d_nbr, d_nn), base)      # the public call on device arrays, host results
    # reversed and permuted object order, one object alone
    same_bits(scores(rows[::-1].copy(), y, s, x[::-1].copy(), nbr[::-1].copy(), nnbr[::-1].copy()), {k: base[k][::-1] for k in ALL})
    perm = np.random.RandomState(1).permutation(N)
    same_bits(scores(rows[perm], y, s, x[perm], nbr[perm], nnbr[perm]), {k: base[k][perm] for k in ALL})
    same_bits(scores(rows[100:101], y, s, x[100:101], nbr[100:101], nnbr[100:101]), {k: base[k][100:101] for k in ALL})


# ---- fitted problems -------------------------------------------------------------------------------------------------------------
def test_the_three_fitters():
    from frankenz_amd import BruteForce, NearestNeighbors, pdf
    X, Xe, Xm, Y, Ye, Ym = dr.photometry(np.random.RandomState(7700), 40, 300, 5)
    M, N = len(Y), len(X)
    rs = np.random.RandomState(3)
    z, ze = rs.uniform(0., 6., M), rs.uniform(0.01, 0.3, M)
    truth = rs.uniform(0., 6., N)
    bf = BruteForce(Y, Ye, Ym)
    bf.fit(X.copy(), Xe.copy(), Xm.copy(), verbose=False)
    nn = NearestNeighbors(Y, Ye, Ym, K=4, rstate=np.random.RandomState(1), verbose=False)
    nn.fit(X.copy(), Xe.copy(), Xm.copy(), rstate=np.random.RandomState(2), k=5, verbose=False)
    sp = bf.fit_sparse(X.copy(), Xe.copy(), Xm.copy(), Nkeep=64, verbose=False)
    for f, nbr, nnbr in ((bf, None, None), (nn, nn.neighbors, nn.Nneighbors), (sp, sp.neighbors, sp.Nneighbors)):
        got = f.predict_scores(z, ze, truth)
        assert set(got) == {'lnpdf', 'crps', 'sqnorm'} and all(v.shape == (N,) for v in got.values())
        want = pdf.posterior_scores(f.fit_lnprob, z, ze, truth, neighbors=nbr, Nneighbors=nnbr)
        same_bits(got, want, ('lnpdf', 'crps', 'sqnorm'))
        lw = np.asarray(f.fit_lnprob)
        ref = sr.scores_ref(lw[:8], z, ze, truth[:8, None], None if nbr is None else np.asarray(nbr)[:8], None if nnbr is None else np.asarray(nnbr)[:8])
        sr.assert_scores({k: v[:8] for k, v in got.items()}, ref, lw.shape[1], type(f).__name__, keys=('lnpdf', 'crps', 'sqnorm'))
        everything = f.predict_scores(z, ze, truth, want=ALL)
        same_bits(everything, got, ('lnpdf', 'crps', 'sqnorm'))
        assert (everything['ninc'] >= 1).all()


# ---- the cap ---------------------------------------------------------------------------------------------------------------------
def test_the_cap_on_the_pair_sums():
    M = sr.NMAX + 1
    y, s = np.full(M, 2.5), np.full(M, 0.3)
    rows = np.zeros((2, M))
    rows[0, 7:] = -20.                                               # object 0: 7 entries; object 1: one more than the cap
    x = np.array([2.4, 3.])
    with pytest.raises(NotImplementedError, match=r"object 1 has 16385 included entries.*16384 \(FZ_SCORES_NMAX\)"):
        scores(rows, y, s, x)
    only = scores(rows, y, s, x, want=('lnpdf', 'ninc'))             # no pair sum asked for: no cap
    np.testing.assert_array_equal(only['ninc'], [7, M])
    want = -0.5 * ((x - 2.5) / 0.3) ** 2 - np.log(0.3) - 0.5 * np.log(2. * np.pi)
    np.testing.assert_allclose(only['lnpdf'], want, rtol=0, atol=4. * (M / 64. + 16.) * sr.U + 16. * sr.U * 4.)


def test_a_full_cap_row_of_identical_components():
    """FZ_SCORES_NMAX identical components are one Gaussian: the single-component closed forms, within the bars of n (n + 1) / 2 pair
    terms.  Its time is the number the cap rests on (docs/scores.md section 4)."""
    n, yv, sv = sr.NMAX, 2.5, 0.3
    y, s = np.full(n, yv), np.full(n, sv)
    rows = np.zeros((1, n))
    x = np.array([2.9])
    scores(rows[:, :64].copy(), y[:64], s[:64], x)                   # (the first call of a process allocates)
    t0 = time.perf_counter()
    got = scores(rows, y, s, x)
    dt = time.perf_counter() - t0
    print("a full-cap row, %d pairs: %.3f s wall" % (n * (n + 1) // 2, dt))
    assert got['ninc'][0] == n
    K2 = n * (n + 1.) / 2.
    A = float(sr.A_G(x[0] - yv, sv * sv)[0])
    assert got['spread'][0] == pytest.approx(sv / SQPI, rel=sr.bar_sum(K2))
    assert got['sqnorm'][0] == pytest.approx(1. / (2. * sv * SQPI), rel=sr.bar_sum(K2))
    assert abs(got['crps'][0] - (A - sv / SQPI)) <= sr.bar_sum(n) * A + sr.bar_sum(K2) * sv / SQPI
    assert abs(got['lnpdf'][0] - (-0.5 * ((x[0] - yv) / sv) ** 2 - np.log(sv) - 0.5 * np.log(2. * np.pi))) <= 4. * (n / 64. + 16.) * sr.U + 16. * sr.U * 3.


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals():
    rows, nbr, nnbr = br.sparse_case(5, 65, 1000, 5, counts=[65] * 5)
    _, _, _, y, s, _ = sr.width_case(65, 1, False)
    N, W, M = 5, 65, 1000
    eng = engine()
    x = np.random.RandomState(4).uniform(0., 6., size=(N, 2))

    def raw(x_=x, y_=y, s_=s, nbr_=nbr, nnbr_=nnbr, M_=M, lncut=np.log(1e-3), P=2, per_object=True, pairs=True):
        return eng.row_scores(rows, N, W, M_, y_, s_, x_, P, per_object=per_object, lncut=lncut, neighbors=nbr_, nnbr=nnbr_,
                              lnpdf=np.empty((N, max(P, 1))), crps=np.empty((N, max(P, 1))) if pairs else None)

    assert raw() == 0
    for bad in (np.nan, np.inf, -np.inf):
        xb = x.copy(); xb[3, 1] = bad
        with pytest.raises(ValueError, match="object 3"):
            raw(x_=xb)
        with pytest.raises(ValueError, match="point"):
            raw(x_=DevArray(xb))
        for arr in (xb[3].copy(), DevArray(xb[3].copy())):
            with pytest.raises(ValueError, match="point 1 "):
                raw(x_=arr, per_object=False)
    with pytest.raises(ValueError):
        raw(P=0)
    for lncut in (0., np.nan, 1.):
        with pytest.raises(ValueError):
            raw(lncut=lncut)
    # labels and errors, s = inf among them (posterior_bins takes it): the smallest refused model is named
    for k, v in ((0, np.nan), (0, np.inf), (1, -1e-300), (1, np.nan), (1, np.inf)):
        t = [y.copy(), s.copy()]
        t[k][[17, 400]] = v
        for conv in (lambda a: a, DevArray):
            with pytest.raises(ValueError, match="model 17 "):
                raw(y_=conv(t[0]), s_=conv(t[1]))
    # indices and counts, with and without the pair stage
    for pairs in (True, False):
        for badv in (1000, -1):
            b = nbr.copy(); b[3, 64] = badv
            with pytest.raises(IndexError):
                raw(nbr_=b, pairs=pairs)
        for badc in (66, -1):
            c = nnbr.copy(); c[2] = badc
            with pytest.raises(IndexError):
                raw(nnbr_=c, pairs=pairs)
    b = nbr.copy(); b[3, 64] = 1000; c = nnbr.copy(); c[3] = 64      # a bad index past the count is never read
    raw(nbr_=b, nnbr_=c)
    # limits, by name; 256 points run
    with pytest.raises(NotImplementedError, match="FZ_BINS_MAX"):
        raw(x_=np.zeros(257), P=257, per_object=False)
    assert raw(x_=np.linspace(0., 6., 256), P=256, per_object=False) == 0
    with pytest.raises(NotImplementedError, match="FZ_DRAW_LMAX"):
        eng.row_scores(rows, 1, (1 << 20) + 1, M, y, s, x, 2, lnpdf=np.empty((1, 2)), neighbors=nbr, nnbr=nnbr)
    with pytest.raises(NotImplementedError, match="FZ_MW_MMAX"):
        raw(M_=1 << 31)
    with pytest.raises(ValueError):                                  # dense rows of 65 entries over 1000 models
        raw(nbr_=None, nnbr_=None)
    from frankenz_amd import pdf
    for wt in (1., -0.1, np.nan):
        with pytest.raises(ValueError):
            pdf.posterior_scores(DevArray(rows), DevArray(y), DevArray(s), DevArray(x), neighbors=DevArray(nbr), Nneighbors=DevArray(nnbr), wt_thresh=wt)
