"""Posterior quantiles on the GPU (csrc/fz_quantile.h, docs/quantiles.md): k_row_quantiles against the contract of the law as
tests/_quantile_ref.py restates it in longdouble (tests/test_quantile_host.py checks the bar's precondition on the same inputs), the
hand rows of the law's three shapes, the round trip through posterior_cdf, the bit-for-bit properties, the three fitters and every
refusal.  Every case asserts nfail == 0, and assert_quantiles prints the worst case as a share of the margin."""
import warnings

import numpy as np
import pytest

import _bins_ref as br
import _draw_ref as dr
import _quantile_ref as qr
from conftest import DevArray

pytestmark = pytest.mark.gpu

SQPI = np.sqrt(np.pi)


def engine():
    from frankenz_amd.engine import get_engine
    return get_engine()


def quant(rows, y, s, p, nbr=None, nnbr=None, wt_thresh=1e-3, **kw):
    """pdf.posterior_quantiles -> x, info; nfail == 0"""
    from frankenz_amd import pdf
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        x, info = pdf.posterior_quantiles(rows, y, s, p, neighbors=nbr, Nneighbors=nnbr, wt_thresh=wt_thresh, return_info=True, **kw)
    assert info['nfail'] == 0
    return x, info


def dev_numpy(d, shape):
    """a DevArray's contents"""
    import ctypes as C
    out = np.empty(shape)
    assert DevArray._hip.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(d.data_ptr()), C.c_size_t(out.nbytes), 2) == 0
    return out


# ---- given rows ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("zeros", [False, True])
@pytest.mark.parametrize("W", br.WIDTHS)
def test_sparse_rows_every_width(W, zeros):
    for k in (0, 1):
        rows, nbr, nnbr, y, s = qr.width_case(W, k, zeros)
        x, info = quant(rows, y, s, qr.PROBS, nbr, nnbr)
        qr.assert_quantiles(x, rows, y, s, qr.PROBS, nbr, nnbr, got_nskip=info['nskip'], what="W = %d, M = %d" % (W, len(y)))
        assert info['nskip'] >= 1                                    # the row with no entry
        live = (~np.isnan(x[:, 0])).sum()
        assert info['niter'] <= 128 * live * len(qr.PROBS)           # (a hull no wider than delta takes no evaluation)
        print("evaluations per (row, p): %.2f" % (info['niter'] / max(1, live * len(qr.PROBS))))


@pytest.mark.parametrize("Q", qr.QCOUNTS)
def test_probability_counts_on_both_sides_of_a_pass(Q):
    rows, nbr, nnbr, y, s, e = br.nbins_case(Q)
    p = qr.probs_case(Q)
    x, info = quant(rows, y, s, p, nbr, nnbr)
    assert x.shape == (5, Q)
    qr.assert_quantiles(x, rows, y, s, p, nbr, nnbr, got_nskip=info['nskip'], what="Q = %d" % Q)


@pytest.mark.parametrize("M", br.DENSE)
def test_dense_rows_through_both_geometries(M):
    rows, y, s, e = br.dense_case(M)
    x, info = quant(rows, y, s, qr.PROBS)
    assert info['nskip'] == 0
    qr.assert_quantiles(x, rows, y, s, qr.PROBS, got_nskip=0, what="dense M = %d" % M)
    if M == 4097:                                                    # the four-wave form against the one-wave form's row
        r6, y6, s6, _ = br.dense_case(4096)
        qr.assert_quantiles(x, r6, y6, s6, qr.PROBS, what="dense 4097 against 4096's law")


@pytest.mark.parametrize("wpo,W", [(4, 65), (4, 257), (1, 4097)])
def test_the_geometry_the_rule_would_not_choose(wpo, W, monkeypatch):
    """FZ_DRAW_WPO forces four waves per object on short rows (at 65 the last two waves own no entry, and the row with no entry is a
    block that makes no evaluation) and one wave on the first row too long for it by default"""
    if wpo == 4:
        cases = [qr.width_case(W, k, z) for k in (0, 1) for z in (False, True)]
    else:
        rows, y, s, e = br.dense_case(4097)
        cases = [(rows, None, None, y, s)]
    monkeypatch.setenv('FZ_DRAW_WPO', str(wpo))
    for rows, nbr, nnbr, y, s in cases:
        x, info = quant(rows, y, s, qr.PROBS, nbr, nnbr)
        qr.assert_quantiles(x, rows, y, s, qr.PROBS, nbr, nnbr, got_nskip=info['nskip'], what="WPO = %d, W = %d" % (wpo, W))
    monkeypatch.delenv('FZ_DRAW_WPO')


# ---- hand rows -------------------------------------------------------------------------------------------------------------------
def test_one_entry_against_the_normal_quantile():
    from scipy.special import ndtri
    y, s = np.array([3., -2., 1e3]), np.array([0.25, 1e-6, 40.])
    rows = np.full((3, 3), -np.inf)
    rows[np.arange(3), np.arange(3)] = 0.
    x, info = quant(rows, y, s, qr.PROBS)
    qr.assert_quantiles(x, rows, y, s, qr.PROBS, got_nskip=0, what="one entry")
    tau = qr.tol(3)
    for j in range(3):
        z = ndtri(qr.PROBS)
        dens = np.exp(-0.5 * z * z) / (np.sqrt(2. * np.pi) * s[j])
        delta = 4. * qr.U * (abs(y[j]) + 40. * s[j])
        # (ndtri itself: a few ulp of z, s u |z| 8 in x)
        assert (np.abs(x[j] - (y[j] + s[j] * z)) <= 2. * tau / dens + 2. * delta + 8. * qr.U * s[j] * np.abs(z)).all(), j


def test_two_equal_point_masses():
    y, s = np.array([1.25, 3.5]), np.zeros(2)
    rows = np.zeros((1, 2))
    p = np.array([0.5, np.nextafter(0.5, 1.), 0.25, 0.75])
    x, _ = quant(rows, y, s, p)
    delta = 4. * qr.U * 3.5
    assert abs(x[0, 0] - 1.25) <= 2. * delta and abs(x[0, 1] - 3.5) <= 2. * delta
    assert abs(x[0, 2] - 1.25) <= 2. * delta and abs(x[0, 3] - 3.5) <= 2. * delta
    qr.assert_quantiles(x, rows, y, s, p, what="two point masses")


def test_a_gap_row_and_all_mass_on_one_model():
    y, s = np.array([0., 5., 2.]), np.array([1e-3, 1e-3, 0.3])
    rows = np.array([[0., 0., -np.inf], [np.log(0.25), 0., -np.inf], [-np.inf, -np.inf, 0.], [-800., -800., 0.]])
    p = np.array([0.5, 0.2, 0.2 + 1e-13, 0.9])                     # 0.5 and 0.2 are exactly the first component's mass in rows 0 and 1
    x, info = quant(rows, y, s, p)
    qr.assert_quantiles(x, rows, y, s, p, got_nskip=0, what="gap")
    assert (x[:2] >= -0.04).all() and (x[:2] <= 5.04).all()
    # all mass on one model: its own normal quantile, whatever the others are (entries at e^-800 hold no weight)
    np.testing.assert_array_equal(x[3], x[2])
    qr.assert_quantiles(x[3:], rows[3:], y, s, p, wt_thresh=None, what="one model")
    x0, _ = quant(rows[3:], y, s, p, wt_thresh=None)
    np.testing.assert_array_equal(x0[0], x[2])


def test_the_cut_is_strict_and_in_ln_space():
    y, s = np.array([0., 100.]), np.array([0.1, 0.1])
    cut = np.log(1e-3)
    rows = np.array([[0., cut], [0., np.nextafter(cut, 0.)]])
    p = np.array([0.5, 1. - 5e-4])
    x, _ = quant(rows, y, s, p)
    qr.assert_quantiles(x, rows, y, s, p, what="the cut")
    # exactly at the cut: excluded, the row is the first model alone; its nextafter: included, and 5e-4 of upper tail lies at 100
    one, _ = quant(np.array([[0., -np.inf]]), y, s, p)
    np.testing.assert_array_equal(x[0], one[0])
    assert x[0, 1] < 1. and x[1, 1] > 99.
    x, _ = quant(rows, y, s, p, wt_thresh=None)
    assert (x[:, 1] > 99.).all()
    qr.assert_quantiles(x, rows, y, s, p, wt_thresh=None, what="no cut")


def test_rows_without_a_posterior_and_rows_with_holes():
    e = br.edges_case(8, 4)
    y, s = br.labels_case(257, e, 4)
    rows, _ = dr.no_posterior_rows(257)
    x, info = quant(rows, y, s, qr.PROBS)
    assert info['nskip'] == 3 and np.isnan(x[:3]).all()
    qr.assert_quantiles(x, rows, y, s, qr.PROBS, got_nskip=info['nskip'], what="no posterior")
    rs = np.random.RandomState(8)
    W = 70
    rows = -rs.uniform(0., 5., size=(6, W)); nbr = rs.randint(0, 257, size=(6, W)).astype(np.int64); nnbr = np.full(6, 60, dtype=np.int64)
    rows[0] = -np.inf
    rows[1, 59] = np.nan                                             # inside the count: no posterior
    rows[2, 60] = np.nan                                             # outside: never read
    rows[3, ::3] = -np.inf
    nnbr[5] = 0                                                      # count 0
    nbr[:, 60:] = -99                                                # padding never read
    x, info = quant(rows, y, s, qr.PROBS, nbr, nnbr)
    assert info['nskip'] == 3 and np.isnan(x[[0, 1, 5]]).all() and np.isfinite(x[[2, 3, 4]]).all()
    qr.assert_quantiles(x, rows, y, s, qr.PROBS, nbr, nnbr, got_nskip=3, what="holes")


# ---- identities ------------------------------------------------------------------------------------------------------------------
def test_round_trip_through_posterior_cdf_and_monotone_outputs():
    from frankenz_amd import pdf
    rows, nbr, nnbr, y, s = qr.width_case(500, 1, False)
    assert (s > 0).all()
    p = np.sort(np.concatenate((qr.PROBS, np.linspace(0.01, 0.99, 55))))
    x, info = quant(rows, y, s, p, nbr, nnbr)
    ok = ~np.isnan(x[:, 0])
    assert ok.sum() >= 3 and (np.diff(x[ok], axis=1) >= 0.).all()    # sorted probabilities: non-decreasing outputs
    C = pdf.posterior_cdf(rows, y, s, np.where(np.isnan(x), 0., x), neighbors=nbr, Nneighbors=nnbr)
    tau = qr.tol(500)
    for i in np.flatnonzero(ok):
        w, yy, ss = qr.mixture(rows, i, y, s, nbr, nnbr, 1e-3)
        delta = qr.hull(yy, ss)[2]
        bar = 2. * tau + 2. * delta * (1. / (ss * np.sqrt(2.))).max() / SQPI
        err = np.abs(C[i] - p)
        print("round trip row %d: worst %.3g of the bar %.3g" % (i, err.max() / bar, bar))
        assert (err <= bar).all()


# ---- reproducibility -------------------------------------------------------------------------------------------------------------
def test_same_bits_alone_among_16_and_17_chunked_device_permuted():
    from frankenz_amd import pdf
    N, W, M = 700, 257, 1000
    e = br.edges_case(33, 5)
    y, s = br.labels_case(M, e, 6)
    s[::5] = 0.
    rows, nbr, nnbr = br.sparse_case(N, W, M, 4, counts=[])
    p17 = qr.probs_case(17)
    base, info = quant(rows, y, s, p17, nbr, nnbr)
    qr.assert_quantiles(base[:40], rows[:40], y, s, p17, nbr[:40], nnbr[:40], what="700 rows (the first 40)")
    # a probability alone, among 16, among 17 (where it falls in the second pass), and in another place of the pass
    for k in (0, 5, 16):
        np.testing.assert_array_equal(quant(rows, y, s, p17[k], nbr, nnbr)[0], base[:, k])
    np.testing.assert_array_equal(quant(rows, y, s, p17[:16], nbr, nnbr)[0], base[:, :16])
    np.testing.assert_array_equal(quant(rows, y, s, p17[::-1].copy(), nbr, nnbr)[0], base[:, ::-1])
    eng = engine()
    old = eng.workspace_limit()
    eng.set_workspace_limit(1 << 20)                                 # 2 x 2056 + 8 + 136 bytes per object: three chunks
    try:
        small, info_small = quant(rows, y, s, p17, nbr, nnbr)
    finally:
        eng.set_workspace_limit(old)
    np.testing.assert_array_equal(small, base)
    assert info_small == info
    d_rows, d_nbr, d_nn, d_y, d_s, d_p = (DevArray(a) for a in (rows, nbr, nnbr, y, s, p17))
    d_x = DevArray(np.zeros((N, 17)))
    cnt = eng.row_quantiles(d_rows, N, W, M, d_y, d_s, d_p, 17, d_x, lncut=np.log(1e-3), neighbors=d_nbr, nnbr=d_nn)
    assert cnt == (info['nskip'], 0, info['niter'])
    np.testing.assert_array_equal(dev_numpy(d_x, (N, 17)), base)
    out = DevArray(np.zeros((N, 17)))                                # the public call, filled in place
    assert pdf.posterior_quantiles(d_rows, d_y, d_s, d_p, neighbors=d_nbr, Nneighbors=d_nn, out=out) is out
    np.testing.assert_array_equal(dev_numpy(out, (N, 17)), base)
    host = np.zeros((N, 17))
    assert pdf.posterior_quantiles(rows, y, s, p17, neighbors=nbr, Nneighbors=nnbr, out=host) is host
    np.testing.assert_array_equal(host, base)
    perm = np.random.RandomState(1).permutation(N)
    np.testing.assert_array_equal(quant(rows[perm], y, s, p17, nbr[perm], nnbr[perm])[0], base[perm])
    np.testing.assert_array_equal(quant(rows[100:101], y, s, p17, nbr[100:101], nnbr[100:101])[0], base[100:101])
    assert quant(rows, y, s, 0.5, nbr, nnbr)[0].shape == (N,)


# ---- fitted problems -------------------------------------------------------------------------------------------------------------
def test_the_three_fitters():
    from frankenz_amd import BruteForce, NearestNeighbors
    X, Xe, Xm, Y, Ye, Ym = dr.photometry(np.random.RandomState(7700), 300, 1000, 5)
    M, N = len(Y), len(X)
    rs = np.random.RandomState(3)
    z, ze = rs.uniform(0., 6., M), rs.uniform(0.01, 0.3, M)
    bf = BruteForce(Y, Ye, Ym)
    bf.fit(X.copy(), Xe.copy(), Xm.copy(), verbose=False)
    nn = NearestNeighbors(Y, Ye, Ym, K=4, rstate=np.random.RandomState(1), verbose=False)
    nn.fit(X.copy(), Xe.copy(), Xm.copy(), rstate=np.random.RandomState(2), k=5, verbose=False)
    sp = bf.fit_sparse(X.copy(), Xe.copy(), Xm.copy(), Nkeep=64, verbose=False)
    default = np.array([0.025, 0.16, 0.5, 0.84, 0.975])
    for f, nbr, nnbr in ((bf, None, None), (nn, nn.neighbors, nn.Nneighbors), (sp, sp.neighbors, sp.Nneighbors)):
        with warnings.catch_warnings():
            warnings.simplefilter("error")                           # nfail > 0 warns
            x = f.predict_quantiles(z, ze)
        assert x.shape == (N, 5)
        sub = slice(0, 60)
        qr.assert_quantiles(x[sub], np.asarray(f.fit_lnprob)[sub], z, ze, default, None if nbr is None else nbr[sub],
                            None if nnbr is None else nnbr[sub], what=type(f).__name__)
        np.testing.assert_array_equal(f.predict_quantiles(z, ze, q=0.5), x[:, 2])
        out = DevArray(np.zeros((N, 5)))
        assert f.predict_quantiles(z, ze, out=out) is out
        np.testing.assert_array_equal(dev_numpy(out, (N, 5)), x)


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals():
    rows, nbr, nnbr = br.sparse_case(5, 65, 1000, 5, counts=[65] * 5)
    _, _, _, y, s = qr.width_case(65, 1, False)
    N, W, M = 5, 65, 1000
    eng = engine()
    q = np.array([0.16, 0.5, 0.84])

    def raw(p_=q, y_=y, s_=s, nbr_=nbr, nnbr_=nnbr, M_=M, lncut=np.log(1e-3), Q=None):
        Q = len(p_) if Q is None else Q
        return eng.row_quantiles(rows, N, W, M_, y_, s_, p_, Q, np.empty((N, max(Q, 1))), lncut=lncut, neighbors=nbr_, nnbr=nnbr_)

    assert raw()[:2] == (0, 0)
    for bad in (0., 1., -0.5, 2., np.nan, np.inf):
        pb = np.array([0.5, bad, 0.3])
        for arr in (pb, DevArray(pb)):
            with pytest.raises(ValueError, match="probability 1 "):
                raw(p_=arr, Q=3)
    with pytest.raises(ValueError):
        raw(Q=0)
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
    from frankenz_amd import pdf
    t = s.copy(); t[17] = np.inf
    assert np.isfinite(pdf.posterior_bins(rows, y, t, np.array([0., 3., 6.]), neighbors=nbr, Nneighbors=nnbr)).all()
    t = [y.copy(), s.copy()]
    t[0][[23, 400]] = -1.7e308; t[1][[23, 400]] = 1e307              # finite each, |y| + 40 s is not
    for conv in (lambda a: a, DevArray):
        with pytest.raises(ValueError, match="model 23 "):
            raw(y_=conv(t[0]), s_=conv(t[1]))
    # indices and counts
    for badv in (1000, -1):
        b = nbr.copy(); b[3, 64] = badv
        with pytest.raises(IndexError):
            raw(nbr_=b)
    for badc in (66, -1):
        c = nnbr.copy(); c[2] = badc
        with pytest.raises(IndexError):
            raw(nnbr_=c)
    b = nbr.copy(); b[3, 64] = 1000; c = nnbr.copy(); c[3] = 64      # a bad index past the count is never read
    raw(nbr_=b, nnbr_=c)
    # limits, by name; 256 probabilities run
    with pytest.raises(NotImplementedError, match="FZ_BINS_MAX"):
        raw(p_=np.linspace(0.1, 0.9, 257))
    assert raw(p_=np.linspace(0.1, 0.9, 256))[1] == 0
    with pytest.raises(NotImplementedError, match="FZ_DRAW_LMAX"):
        eng.row_quantiles(rows, 1, (1 << 20) + 1, M, y, s, q, 3, np.empty((1, 3)), neighbors=nbr, nnbr=nnbr)
    with pytest.raises(NotImplementedError, match="FZ_MW_MMAX"):
        raw(M_=1 << 31)
    with pytest.raises(ValueError):                                  # dense rows of 65 entries over 1000 models
        raw(nbr_=None, nnbr_=None)
    for wt in (1., -0.1, np.nan):
        with pytest.raises(ValueError):
            pdf.posterior_quantiles(DevArray(rows), DevArray(y), DevArray(s), q, neighbors=DevArray(nbr), Nneighbors=DevArray(nnbr), wt_thresh=wt)
