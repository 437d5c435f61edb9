"""Posterior bin masses and mixture CDFs on the GPU (csrc/fz_bins.h, docs/bins.md): k_row_bins against the NumPy law of
tests/_bins_ref.py at the absolute bar 4 (W / 64 + 16) u (tests/test_bins_host.py checks its precondition on the same inputs), the
hand rows of the law's edge rules, the identities, the bit-for-bit properties, the three fitters, the hand-off to the hierarchical
sampler and every refusal."""
import numpy as np
import pytest

import _bins_ref as br
import _draw_ref as dr
from conftest import DevArray

pytestmark = pytest.mark.gpu


def engine():
    from frankenz_amd.engine import get_engine
    return get_engine()


def bins(rows, y, s, e, nbr=None, nnbr=None, wt_thresh=1e-3, normalize=False):
    """pdf.posterior_bins -> p, below, above"""
    from frankenz_amd import pdf
    p, (below, above) = pdf.posterior_bins(rows, y, s, e, neighbors=nbr, Nneighbors=nnbr, wt_thresh=wt_thresh, normalize=normalize,
                                           return_outside=True)
    return p, below, above


def cdf(rows, y, s, x, nbr=None, nnbr=None, wt_thresh=1e-3):
    from frankenz_amd import pdf
    return pdf.posterior_cdf(rows, y, s, x, neighbors=nbr, Nneighbors=nnbr, wt_thresh=wt_thresh)


def dev_numpy(d, shape):
    """a DevArray's contents"""
    import ctypes as C
    out = np.empty(shape)
    assert DevArray._hip.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(d.data_ptr()), C.c_size_t(out.nbytes), 2) == 0
    return out


# ---- given rows ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", br.WIDTHS)
def test_sparse_rows_every_width(W):
    for k in (0, 1):
        rows, nbr, nnbr, y, s, e = br.width_case(W, k)
        ref = br.bins_ref(rows, y, s, e, nbr, nnbr)
        assert ref[3] >= 1                                           # the row with no entry
        p, below, above = bins(rows, y, s, e, nbr, nnbr)
        br.assert_bins(p, ref, W, below, above)
        assert engine().row_bins(rows, len(rows), W, len(y), y, s, e, len(e), np.empty_like(p), lncut=np.log(1e-3), neighbors=nbr, nnbr=nnbr) == ref[3]
        pn, b2, a2 = bins(rows, y, s, e, nbr, nnbr, normalize=True)
        br.assert_bins(pn, ref, W, normalize=True)
        np.testing.assert_array_equal(b2, below); np.testing.assert_array_equal(a2, above)
        ok = ~np.isnan(p[:, 0])
        br.assert_close(p[ok].sum(axis=1) + below[ok] + above[ok], np.ones(ok.sum()), W, "total")
        # the CDF at the edges, differenced
        C = cdf(rows, y, s, e, nbr, nnbr)
        br.assert_close(C, br.cdf_ref(rows, y, s, e, nbr, nnbr)[0], W, "C")
        br.assert_close(np.diff(C, axis=1), p, W, "cdf differences", factor=2.)
        br.assert_close(C[:, 0], below, W, "C(e_0)", factor=2.)


@pytest.mark.parametrize("NB", br.NBINS)
def test_every_bin_count(NB):
    rows, nbr, nnbr, y, s, e = br.nbins_case(NB)
    ref = br.bins_ref(rows, y, s, e, nbr, nnbr)
    p, below, above = bins(rows, y, s, e, nbr, nnbr)
    assert p.shape == (5, NB)
    br.assert_bins(p, ref, 65, below, above)
    pn, _, _ = bins(rows, y, s, e, nbr, nnbr, normalize=True)
    br.assert_bins(pn, ref, 65, normalize=True)
    # without below and above: the same masses, bit for bit
    from frankenz_amd import pdf
    np.testing.assert_array_equal(pdf.posterior_bins(rows, y, s, e, neighbors=nbr, Nneighbors=nnbr, normalize=False), p)


@pytest.mark.parametrize("N", [1, 3, 4, 5, 257])
def test_block_of_four_edge(N):
    e = br.edges_case(8, 3)
    y, s = br.labels_case(1000, e, 3)
    rows, nbr, nnbr = br.sparse_case(N, 64, 1000, 2)
    ref = br.bins_ref(rows, y, s, e, nbr, nnbr)
    p, below, above = bins(rows, y, s, e, nbr, nnbr)
    br.assert_bins(p, ref, 64, below, above)


@pytest.mark.parametrize("M", br.DENSE)
def test_dense_rows(M):
    rows, y, s, e = br.dense_case(M)
    ref = br.bins_ref(rows, y, s, e)
    p, below, above = bins(rows, y, s, e)
    assert ref[3] == 0
    br.assert_bins(p, ref, M, below, above)
    br.assert_close(cdf(rows, y, s, e), br.cdf_ref(rows, y, s, e)[0], M, "C")
    if M == 4097:                                                    # the four-wave form against the one-wave form's reference
        r6, y6, s6, _ = br.dense_case(4096)
        br.assert_bins(p, br.bins_ref(r6, y6, s6, e), M, below, above)


@pytest.mark.parametrize("wpo,W", [(4, 65), (4, 257), (1, 4097)])
def test_both_geometries_at_the_widths_the_rule_keeps_from_them(wpo, W, monkeypatch):
    """FZ_DRAW_WPO forces the form the row length would not choose: four waves per object at W = 65 (the object's last two waves own no
    entry) and 257 (a ragged last pass), with the row that has no entry; one wave per object on the first row too long for it by
    default.  Masses, below / above and the CDF of each form at the bar that covers both, and per form the same bits for host and
    device arrays."""
    if wpo == 4:
        cases = [br.width_case(W, k) for k in (0, 1)]
    else:
        rows, y, s, e = br.dense_case(4097)
        cases = [(rows, None, None, y, s, e)]
    eng = engine()
    dev = lambda a: None if a is None else DevArray(a)
    monkeypatch.setenv('FZ_DRAW_WPO', str(wpo))
    for rows, nbr, nnbr, y, s, e in cases:
        ref = br.bins_ref(rows, y, s, e, nbr, nnbr)
        assert ref[3] >= (1 if wpo == 4 else 0)
        p, below, above = bins(rows, y, s, e, nbr, nnbr)
        br.assert_bins(p, ref, W, below, above)
        C = cdf(rows, y, s, e, nbr, nnbr)
        br.assert_close(C, br.cdf_ref(rows, y, s, e, nbr, nnbr)[0], W, "C")
        N, M, NB = len(rows), len(y), len(e) - 1
        d_p, d_lo, d_hi, d_c = DevArray(np.zeros((N, NB))), DevArray(np.zeros(N)), DevArray(np.zeros(N)), DevArray(np.zeros((N, NB + 1)))
        d_rows, d_nbr, d_nn, d_y, d_s = DevArray(rows), dev(nbr), dev(nnbr), DevArray(y), DevArray(s)
        ns = eng.row_bins(d_rows, N, W, M, d_y, d_s, DevArray(e), NB + 1, d_p, lncut=np.log(1e-3), normalize=False, below=d_lo, above=d_hi,
                          neighbors=d_nbr, nnbr=d_nn)
        eng.row_cdf(d_rows, N, W, M, d_y, d_s, DevArray(e), NB + 1, d_c, per_object=False, lncut=np.log(1e-3), neighbors=d_nbr, nnbr=d_nn)
        assert ns == ref[3]
        for d, h in ((d_p, p), (d_lo, below), (d_hi, above), (d_c, C)):
            np.testing.assert_array_equal(dev_numpy(d, h.shape), h)
    monkeypatch.delenv('FZ_DRAW_WPO')


# ---- hand rows -------------------------------------------------------------------------------------------------------------------
def test_point_masses_on_edges_inside_and_at_the_last_edge():
    e = np.array([0., 1., 2., 4.])
    y = np.array([1., 1.5, 4., -1., 0.])
    s = np.zeros(5)
    rows = np.full((5, 5), -np.inf)
    rows[np.arange(5), np.arange(5)] = 0.
    p, below, above = bins(rows, y, s, e)
    np.testing.assert_array_equal(p, [[0, 1, 0], [0, 1, 0], [0, 0, 0], [0, 0, 0], [1, 0, 0]])
    np.testing.assert_array_equal(below, [0, 0, 0, 1, 0])
    np.testing.assert_array_equal(above, [0, 0, 1, 0, 0])
    np.testing.assert_array_equal(cdf(rows, y, s, e), [[float(x >= yy) for x in e] for yy in y])
    ref = br.bins_ref(rows, y, s, e)
    br.assert_bins(p, ref, 5, below, above)
    # a point mass beside a Gaussian in one row
    rows = np.array([[0., -1., -np.inf, -np.inf, -np.inf]]); s2 = s.copy(); s2[1] = 0.3
    p, below, above = bins(rows, y, s2, e)
    br.assert_bins(p, br.bins_ref(rows, y, s2, e), 5, below, above)


def test_all_mass_outside_the_range():
    e = np.array([0., 1., 2.])
    y, s = np.array([-50., 102., 150.]), np.array([1., 1., 0.])
    rows = np.array([[0., -1., -2.], [-3., 0., -0.5]])
    p, below, above = bins(rows, y, s, e)
    np.testing.assert_array_equal(p, np.zeros((2, 2)))
    br.assert_close(below + above, np.ones(2), 3, "outside")
    assert np.isnan(bins(rows, y, s, e, normalize=True)[0]).all()


def test_rows_without_a_posterior_and_rows_with_holes():
    e = br.edges_case(8, 4)
    y, s = br.labels_case(257, e, 4)
    rows, _ = dr.no_posterior_rows(257)
    ref = br.bins_ref(rows, y, s, e)
    p, below, above = bins(rows, y, s, e)
    assert ref[3] == 3 and np.isnan(p[:3]).all() and np.isnan(below[:3]).all() and np.isnan(above[:3]).all()
    br.assert_bins(p, ref, 257, below, above)
    assert np.isnan(cdf(rows, y, s, e)[:3]).all()
    # a row of all -inf; a nan inside and outside the count; -inf entries; padding of -99 never read
    rs = np.random.RandomState(8)
    W = 70
    rows = -rs.uniform(0., 5., size=(5, W)); nbr = rs.randint(0, 257, size=(5, W)).astype(np.int64); nnbr = np.full(5, 60, dtype=np.int64)
    rows[0] = -np.inf
    rows[1, 59] = np.nan                                             # inside the count: no posterior
    rows[2, 60] = np.nan                                             # outside: never read
    rows[3, ::3] = -np.inf
    nbr[:, 60:] = -99
    ref = br.bins_ref(rows, y, s, e, nbr, nnbr)
    assert ref[3] == 2
    p, below, above = bins(rows, y, s, e, nbr, nnbr)
    br.assert_bins(p, ref, W, below, above)
    assert np.isnan(p[:2]).all() and np.isfinite(p[2:]).all()


def test_the_cut_is_strict_and_in_ln_space():
    e = np.array([0., 1., 2., 4.])
    y, s = np.array([0.5, 1.5]), np.array([0., 0.])
    cut = np.log(1e-3)
    rows = np.array([[0., cut], [0., np.nextafter(cut, 0.)], [0., -30.]])
    p, _, _ = bins(rows, y, s, e)
    np.testing.assert_array_equal(p[0], [1., 0., 0.])                # exactly at the cut: excluded
    assert 0. < p[1, 1] < 1.1e-3 and p[1, 0] < 1.                    # its nextafter towards the max: kept
    br.assert_bins(p, br.bins_ref(rows, y, s, e), 2)
    for wt in (None, 0.):                                            # no cut: every positive weight counts
        p, below, above = bins(rows, y, s, e, wt_thresh=wt)
        assert p[2, 1] > 0.
        br.assert_bins(p, br.bins_ref(rows, y, s, e, wt_thresh=wt), 2, below, above)
    rows, nbr, nnbr, y, s, e = br.width_case(257, 1)
    for wt in (None, 0.3):
        p, below, above = bins(rows, y, s, e, nbr, nnbr, wt_thresh=wt)
        br.assert_bins(p, br.bins_ref(rows, y, s, e, nbr, nnbr, wt_thresh=wt), 257, below, above)


# ---- CDF mode --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 8, 9, 16, 17, 64, 65, 256])
def test_cdf_shared_and_per_object_points(P):
    rows, nbr, nnbr, y, s, e = br.width_case(65, 1)
    N = len(rows)
    shared, per = br.cdf_points(P, N)
    assert P < 3 or (np.diff(shared) < 0).any()                      # unsorted
    C = cdf(rows, y, s, shared, nbr, nnbr)
    assert C.shape == (N, P)
    br.assert_close(C, br.cdf_ref(rows, y, s, shared, nbr, nnbr)[0], 65, "shared")
    np.testing.assert_array_equal(cdf(rows, y, s, shared[None, :], nbr, nnbr), C)
    Cp = cdf(rows, y, s, per, nbr, nnbr)
    br.assert_close(Cp, br.cdf_ref(rows, y, s, per, nbr, nnbr)[0], 65, "per object")
    # a point's value does not depend on the points beside it
    np.testing.assert_array_equal(cdf(rows, y, s, per[:, :1].copy(), nbr, nnbr), Cp[:, :1])
    np.testing.assert_array_equal(cdf(rows, y, s, DevArray(per), DevArray(nbr), DevArray(nnbr)), Cp)


def test_the_pit_form():
    rows, nbr, nnbr, y, s, e = br.width_case(500, 1)
    N = len(rows)
    truth = np.random.RandomState(3).uniform(0., 6., N)
    pit = cdf(rows, y, s, truth, nbr, nnbr)
    assert pit.shape == (N,)
    br.assert_close(pit, br.cdf_ref(rows, y, s, truth[:, None], nbr, nnbr)[0][:, 0], 500, "PIT")
    ok = ~np.isnan(pit)
    assert ((pit[ok] >= 0.) & (pit[ok] <= 1.)).all()


# ---- reproducibility -------------------------------------------------------------------------------------------------------------
def test_same_bits_chunked_device_permuted_and_alone():
    from frankenz_amd import pdf
    N, W, M = 700, 257, 1000
    e = br.edges_case(33, 5)
    y, s = br.labels_case(M, e, 6)
    rows, nbr, nnbr = br.sparse_case(N, W, M, 4, counts=[])
    pts = br.cdf_points(20, N)[1]
    base = bins(rows, y, s, e, nbr, nnbr, normalize=True) + (cdf(rows, y, s, pts, nbr, nnbr),)
    eng = engine()
    old = eng.workspace_limit()
    eng.set_workspace_limit(1 << 20)                                 # 2 x 2056 + 8 + 264 + 16 bytes per object: three chunks
    try:
        small = bins(rows, y, s, e, nbr, nnbr, normalize=True) + (cdf(rows, y, s, pts, nbr, nnbr),)
    finally:
        eng.set_workspace_limit(old)
    d_p, d_lo, d_hi, d_c = DevArray(np.zeros((N, 33))), DevArray(np.zeros(N)), DevArray(np.zeros(N)), DevArray(np.zeros((N, 20)))
    d_rows, d_nbr, d_nn, d_y, d_s = (DevArray(a) for a in (rows, nbr, nnbr, y, s))
    ns = eng.row_bins(d_rows, N, W, M, d_y, d_s, DevArray(e), 34, d_p, lncut=np.log(1e-3), normalize=True, below=d_lo, above=d_hi,
                      neighbors=d_nbr, nnbr=d_nn)
    eng.row_cdf(d_rows, N, W, M, d_y, d_s, DevArray(pts), 20, d_c, per_object=True, lncut=np.log(1e-3), neighbors=d_nbr, nnbr=d_nn)
    dev = (dev_numpy(d_p, (N, 33)), dev_numpy(d_lo, (N,)), dev_numpy(d_hi, (N,)), dev_numpy(d_c, (N, 20)))
    assert ns == br.bins_ref(rows, y, s, e, nbr, nnbr)[3]
    out = DevArray(np.zeros((N, 33)))                                # the public call on device arrays, filled in place
    assert pdf.posterior_bins(d_rows, d_y, d_s, DevArray(e), neighbors=d_nbr, Nneighbors=d_nn, out=out) is out
    np.testing.assert_array_equal(dev_numpy(out, (N, 33)), base[0])
    perm = np.random.RandomState(1).permutation(N)
    pm = bins(rows[perm], y, s, e, nbr[perm], nnbr[perm], normalize=True) + (cdf(rows[perm], y, s, pts[perm], nbr[perm], nnbr[perm]),)
    sub = bins(rows[100:103], y, s, e, nbr[100:103], nnbr[100:103], normalize=True) + (cdf(rows[100:103], y, s, pts[100:103], nbr[100:103], nnbr[100:103]),)
    for k in range(4):
        np.testing.assert_array_equal(small[k], base[k])
        np.testing.assert_array_equal(dev[k], base[k])
        np.testing.assert_array_equal(pm[k], base[k][perm])
        np.testing.assert_array_equal(sub[k], base[k][100:103])


# ---- fitted problems -------------------------------------------------------------------------------------------------------------
def test_the_three_fitters_and_the_hand_off_to_the_sampler():
    from frankenz_amd import BruteForce, NearestNeighbors, samplers
    X, Xe, Xm, Y, Ye, Ym = dr.photometry(np.random.RandomState(7700), 300, 1000, 5)
    M, N = len(Y), len(X)
    rs = np.random.RandomState(3)
    z, ze = rs.uniform(0., 6., M), rs.uniform(0.01, 0.3, M)
    e = np.array([0., 0.4, 0.9, 1.3, 2., 2.6, 3.5, 4.7, 6.])
    truth = rs.uniform(0., 6., N)
    bf = BruteForce(Y, Ye, Ym)
    bf.fit(X.copy(), Xe.copy(), Xm.copy(), verbose=False)
    nn = NearestNeighbors(Y, Ye, Ym, K=4, rstate=np.random.RandomState(1), verbose=False)
    nn.fit(X.copy(), Xe.copy(), Xm.copy(), rstate=np.random.RandomState(2), k=5, verbose=False)
    sp = bf.fit_sparse(X.copy(), Xe.copy(), Xm.copy(), Nkeep=64, verbose=False)
    for f, W, nbr, nnbr in ((bf, M, None, None), (nn, nn.neighbors.shape[1], nn.neighbors, nn.Nneighbors), (sp, 64, sp.neighbors, sp.Nneighbors)):
        ref = br.bins_ref(f.fit_lnprob, z, ze, e, nbr, nnbr)
        p, (below, above) = f.predict_bins(z, ze, e, normalize=False, return_outside=True)
        br.assert_bins(p, ref, W, below, above)
        br.assert_bins(f.predict_bins(z, ze, e), ref, W, normalize=True)
        br.assert_close(f.predict_cdf(z, ze, e), br.cdf_ref(f.fit_lnprob, z, ze, e, nbr, nnbr)[0], W, "C")
        pit = f.predict_cdf(z, ze, truth)
        assert pit.shape == (N,)
        br.assert_close(pit, br.cdf_ref(f.fit_lnprob, z, ze, truth[:, None], nbr, nnbr)[0][:, 0], W, "PIT")
    # sparse rows that keep every model, no cut: the dense result
    full = bf.fit_sparse(X.copy(), Xe.copy(), Xm.copy(), Nkeep=M, wt_thresh=0, verbose=False)
    dense = bf.predict_bins(z, ze, e, wt_thresh=0, normalize=False)
    br.assert_close(full.predict_bins(z, ze, e, wt_thresh=0, normalize=False), dense, M, "full sparse rows", factor=2.)
    # hand-off: the device stack given to the hierarchical sampler, against the sampler on its NumPy copy
    out = DevArray(np.zeros((N, 8)))
    assert nn.predict_bins(z, ze, e, out=out) is out
    host = dev_numpy(out, (N, 8))
    np.testing.assert_array_equal(host, nn.predict_bins(z, ze, e))
    assert np.isfinite(host).all()
    chains = []
    for stack in (out, host):
        smp = samplers.hierarchical_sampler(stack)
        smp.run_mcmc(4, thin=2, rstate=np.random.RandomState(5), verbose=False)
        chains.append(smp.results)
    np.testing.assert_array_equal(chains[0][0], chains[1][0])
    np.testing.assert_array_equal(chains[0][1], chains[1][1])


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals():
    rows, nbr, nnbr, y, s, e = br.width_case(65, 1)
    rows, nbr, nnbr = br.sparse_case(5, 65, 1000, 5, counts=[65] * 5)
    N, W, M = 5, 65, 1000
    eng = engine()

    def raw(e_=e, y_=y, s_=s, nbr_=nbr, nnbr_=nnbr, M_=M, lncut=np.log(1e-3)):
        return eng.row_bins(rows, N, W, M_, y_, s_, e_, len(e_), np.empty((N, max(len(e_) - 1, 1))), lncut=lncut, neighbors=nbr_, nnbr=nnbr_)

    def raw_cdf(x, per_object=False, P=None):
        P = x.shape[-1] if P is None else P
        return eng.row_cdf(rows, N, W, M, y, s, x, P, np.empty((N, max(P, 1))), per_object=per_object, lncut=np.log(1e-3), neighbors=nbr, nnbr=nnbr)

    raw(); raw_cdf(e)
    # edges and points
    for bad in (e[:1], np.array([0., 1., 1.]), np.array([0., 2., 1.]), np.array([0., np.nan, 2.]), np.array([0., 1., np.inf])):
        for arr in (bad, DevArray(bad)):
            with pytest.raises(ValueError):
                eng.row_bins(rows, N, W, M, y, s, arr, len(bad), np.empty((N, 2)), lncut=np.log(1e-3), neighbors=nbr, nnbr=nnbr)
    with pytest.raises(ValueError):
        raw_cdf(e, P=0)
    x = np.tile(e, (N, 1)); x[3, 2] = np.nan
    for arr in (x, DevArray(x)):
        with pytest.raises(ValueError, match="not finite"):
            raw_cdf(arr, per_object=True, P=len(e))
    with pytest.raises(ValueError, match="not finite"):
        raw_cdf(np.array([0., -np.inf]))
    with pytest.raises(ValueError):
        raw(lncut=0.)
    with pytest.raises(ValueError):
        raw(lncut=np.nan)
    # labels and errors: the smallest refused model is named
    for k, v in ((0, np.nan), (0, np.inf), (1, -1e-300), (1, np.nan)):
        t = [y.copy(), s.copy()]
        t[k][[17, 400]] = v
        for conv in (lambda a: a, DevArray):
            with pytest.raises(ValueError, match="model 17 "):
                raw(y_=conv(t[0]), s_=conv(t[1]))
    # indices and counts
    for badv in (1000, -1):
        b = nbr.copy(); b[3, 64] = badv
        with pytest.raises(IndexError):
            raw(nbr_=b)
    c = nnbr.copy(); c[2] = 66
    with pytest.raises(IndexError):
        raw(nnbr_=c)
    c[2] = -1
    with pytest.raises(IndexError):
        raw(nnbr_=c)
    b = nbr.copy(); b[3, 64] = 1000; c = nnbr.copy(); c[3] = 64      # a bad index past the count is never read
    raw(nbr_=b, nnbr_=c)
    # limits, by name; 256 bins and points run
    big = np.arange(258.)
    with pytest.raises(NotImplementedError, match="FZ_BINS_MAX"):
        raw(e_=big)
    with pytest.raises(NotImplementedError, match="FZ_BINS_MAX"):
        raw_cdf(big[:257])
    assert raw(e_=big[:257]) == 0 and raw_cdf(big[:256]) == 0
    with pytest.raises(NotImplementedError, match="FZ_DRAW_LMAX"):
        eng.row_bins(rows, 1, (1 << 20) + 1, M, y, s, e, len(e), np.empty((1, 8)), neighbors=nbr, nnbr=nnbr)
    with pytest.raises(NotImplementedError, match="FZ_MW_MMAX"):
        raw(M_=1 << 31)
    with pytest.raises(ValueError):                                  # dense rows of 65 entries over 1000 models
        raw(nbr_=None, nnbr_=None)
