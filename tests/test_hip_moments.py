"""Posterior moments and zero-point sums on the GPU (csrc/fz_moments.h, docs/predictive.md): k_row_moments against the `longdouble` law of
tests/_moments_ref.py at the bars derived there (a sum of W terms: 4 (W / 64 + 16) u of its absolute terms), its bit-for-bit properties,
refusals, the fitters' `predict_phot` / `moments` on the device's own rows, `phot_sums` and `zeropoint_offsets`."""
import functools
import os
import sys

import numpy as np
import pytest

import _draw_ref as dr
import _moments_ref as mr
from conftest import DevArray

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, "oracle"))

LS = (1, 2, 4, 5, 8, 9, 16, 17, 32)             # both sides of each column bucket


def engine():
    from frankenz_amd.engine import get_engine
    return get_engine()


def raw(rows, V, Ve=None, Vm=None, scale=None, nbr=None, nnbr=None, var=True, share=True, M=None, L=None):
    """Engine.row_moments on arrays as they are -> mean, var, share, nskip"""
    N, W = rows.shape
    M, L = (V.shape[0] if M is None else M), (V.shape[1] if L is None else L)
    mean = np.full((N, L), -7.)
    v = np.full((N, L), -7.) if var else None
    s = np.full((N, L), -7.) if share else None
    ns = engine().row_moments(rows, N, W, M, L, V, mean, var=v, share=s, value_errs=Ve, value_mask=Vm, scale=scale, neighbors=nbr, nnbr=nnbr)
    return mean, v, s, ns


def sparse_case(N, W, M, L, seed, counts=None):
    """rows whose weights span e^-12, repeated indices when M < W, counts that include 0, 1, W - 1 and W"""
    rs = np.random.RandomState(3000 + 17 * W + 5 * L + N + M + seed)
    rows = -rs.uniform(0., 12., size=(N, W))
    nbr = rs.randint(0, M, size=(N, W)).astype(np.int64)
    nnbr = rs.randint(0, W + 1, N).astype(np.int64)
    edge = [W, max(W - 1, 0), 1, 0] if counts is None else counts
    for i in range(N):
        if i < len(edge):
            nnbr[i] = min(edge[i], W)
    for i in range(N):
        rows[i, nnbr[i]:] = -np.inf; nbr[i, nnbr[i]:] = -99
    scale = rs.uniform(0.5, 2., size=(N, W))
    V = rs.lognormal(1., 1., size=(M, L)); Ve = rs.uniform(0.01, 0.2, size=(M, L)) * V
    Vm = (rs.rand(M, L) > 0.2).astype(np.float64)
    return rows, nbr, nnbr, scale, V, Ve, Vm


# ---- given rows ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [1, 2, 63, 64, 65, 256, 257, 500, 4096])
def test_sparse_rows_every_width(W):
    for k, M in enumerate((7, 1000)):
        L = LS[(W + 4 * k) % len(LS)]
        rows, nbr, nnbr, sc, V, Ve, Vm = sparse_case(5, W, M, L, k)
        ref = mr.moments_ref(rows, V, Ve, Vm, sc, nbr, nnbr)
        mean, var, share, ns = raw(rows, V, Ve, Vm, sc, nbr, nnbr)
        assert ns == ref[3] and ns >= 1                              # the row with no entry
        mr.assert_moments(mean, var, ref, W, share)


@pytest.mark.parametrize("L", LS)
def test_every_column_count(L):
    rows, nbr, nnbr, sc, V, Ve, Vm = sparse_case(5, 65, 1000, L, 1)
    ref = mr.moments_ref(rows, V, Ve, Vm, sc, nbr, nnbr)
    mean, var, share, ns = raw(rows, V, Ve, Vm, sc, nbr, nnbr)
    mr.assert_moments(mean, var, ref, 65, share)
    # without var and share: the same mean, bit for bit
    m2, v2, s2, _ = raw(rows, V, Ve, Vm, sc, nbr, nnbr, var=False, share=False)
    np.testing.assert_array_equal(m2, mean)
    m3, v3, s3, _ = raw(rows, V, Ve, Vm, sc, nbr, nnbr, share=False)
    np.testing.assert_array_equal(v3, var)


@pytest.mark.parametrize("N", [1, 3, 4, 5, 257])
def test_block_of_four_edge(N):
    rows, nbr, nnbr, sc, V, Ve, Vm = sparse_case(N, 64, 1000, 5, 2)
    ref = mr.moments_ref(rows, V, Ve, Vm, sc, nbr, nnbr)
    mean, var, share, ns = raw(rows, V, Ve, Vm, sc, nbr, nnbr)
    assert ns == ref[3]
    mr.assert_moments(mean, var, ref, 64, share)


@pytest.mark.parametrize("flags", range(8))
def test_optional_tables(flags):
    rows, nbr, nnbr, sc, V, Ve, Vm = sparse_case(5, 257, 1000, 5, 3)
    sc, Ve, Vm = (sc if flags & 1 else None), (Ve if flags & 2 else None), (Vm if flags & 4 else None)
    ref = mr.moments_ref(rows, V, Ve, Vm, sc, nbr, nnbr)
    mean, var, share, _ = raw(rows, V, Ve, Vm, sc, nbr, nnbr)
    mr.assert_moments(mean, var, ref, 257, share)
    if Vm is None:
        np.testing.assert_array_equal(share[nnbr > 0], 1.)


@functools.lru_cache(maxsize=None)
def dense_case(M):
    rs = np.random.RandomState(3900 + min(M, 4096))                  # 4096 and 4097 share their leading content
    m = max(M, 4097) if M in (4096, 4097) else M
    rows = -rs.uniform(0., 12., size=(3, m)); V = rs.lognormal(1., 1., size=(m, 5)); Ve = 0.1 * V
    Vm = (rs.rand(m, 5) > 0.2).astype(np.float64)
    rows, V, Ve, Vm = rows[:, :M].copy(), V[:M].copy(), Ve[:M].copy(), Vm[:M].copy()
    if M == 4097:
        rows[:, -1] = -np.inf                                        # the entry the longer row adds holds no weight
    return rows, V, Ve, Vm


@pytest.mark.parametrize("M", [1, 255, 4096, 4097, 70001])
def test_dense_rows(M):
    rows, V, Ve, Vm = dense_case(M)
    ref = mr.moments_ref(rows, V, Ve, Vm)
    mean, var, share, ns = raw(rows, V, Ve, Vm)
    assert ns == 0
    mr.assert_moments(mean, var, ref, M, share)
    if M == 4097:                                                    # the four-wave form against the one-wave form's reference
        mr.assert_moments(mean, var, mr.moments_ref(*dense_case(4096)), M, share)


@pytest.mark.parametrize("wpo,W", [(4, 65), (4, 257), (1, 4097)])
def test_both_geometries_at_the_widths_the_rule_keeps_from_them(wpo, W, monkeypatch):
    """FZ_DRAW_WPO forces the form the row length would not choose: four waves per object at W = 65 (the object's last two waves own no
    entry) and 257 (a ragged last pass), with the row that has no entry; one wave per object on the first row too long for it by
    default.  Each form at the bar that covers both, and per form the same bits for host and device arrays."""
    if wpo == 4:
        cases = []
        for k, M in enumerate((7, 1000)):
            rows, nbr, nnbr, sc, V, Ve, Vm = sparse_case(5, W, M, 5, k)
            cases.append((rows, V, Ve, Vm, sc, nbr, nnbr))
    else:
        cases = [dense_case(4097) + (None, None, None)]
    eng = engine()
    monkeypatch.setenv('FZ_DRAW_WPO', str(wpo))
    for rows, V, Ve, Vm, sc, nbr, nnbr in cases:
        ref = mr.moments_ref(rows, V, Ve, Vm, sc, nbr, nnbr)
        mean, var, share, ns = raw(rows, V, Ve, Vm, sc, nbr, nnbr)
        assert ns == ref[3] and ns >= (1 if wpo == 4 else 0)
        mr.assert_moments(mean, var, ref, W, share)
        N, M, L = len(rows), len(V), V.shape[1]
        d_out = [DevArray(np.zeros((N, L))) for _ in range(3)]
        dev = lambda a: None if a is None else DevArray(a)
        dns = eng.row_moments(DevArray(rows), N, W, M, L, DevArray(V), d_out[0], var=d_out[1], share=d_out[2], value_errs=DevArray(Ve),
                              value_mask=DevArray(Vm), scale=dev(sc), neighbors=dev(nbr), nnbr=dev(nnbr))
        assert dns == ns
        for d, h in zip(d_out, (mean, var, share)):
            np.testing.assert_array_equal(dr_numpy(d, (N, L)), h)
    monkeypatch.delenv('FZ_DRAW_WPO')


# ---- row kinds -------------------------------------------------------------------------------------------------------------------
def test_hand_rows_and_rows_without_a_posterior():
    rows, _ = dr.hand_rows(513, 1, 37)
    rs = np.random.RandomState(5)
    V = rs.normal(0., 3., size=(513, 5)); Ve = rs.uniform(0.1, 1., size=(513, 5))       # negative values that cancel in the mean
    ref = mr.moments_ref(rows, V, Ve)
    mean, var, share, ns = raw(rows, V, Ve)
    assert ns == 0
    mr.assert_moments(mean, var, ref, 513, share)
    rows, _ = dr.no_posterior_rows(257)
    ref = mr.moments_ref(rows, V[:257], Ve[:257])
    mean, var, share, ns = raw(rows, V[:257], Ve[:257])
    assert ns == 3 and np.isnan(mean[:3]).all() and np.isnan(var[:3]).all() and (share[:3] == 0).all()
    mr.assert_moments(mean, var, ref, 257, share)


def test_infinite_values_masked_columns_and_underflow():
    rs = np.random.RandomState(6)
    W = 300
    rows = -rs.uniform(0., 12., size=(4, W))
    rows[0, 1:] -= 2000.; rows[0, 0] = 0.                            # one entry at weight 1, the rest underflow
    rows[1, 7] = -2000.                                              # ... holds an inf value under a zero weight
    rows[2, 9] = -np.inf
    V = rs.lognormal(1., 1., size=(W, 3))
    V[7, 0] = np.inf
    Vm = np.ones((W, 3)); Vm[:, 2] = 0.                              # a column masked for every model
    ref = mr.moments_ref(rows, V, None, Vm)
    mean, var, share, ns = raw(rows, V, None, Vm)
    assert ns == 0 and np.isnan(mean[:, 2]).all() and np.isnan(var[:, 2]).all() and (share[:, 2] == 0).all()
    assert mean[0, 0] == V[0, 0] and var[0, 0] == 0. and np.isfinite(mean[1, 0])
    assert np.isinf(mean[2, 0]) and np.isnan(var[2, 0])              # inf under a positive weight: NumPy's arithmetic
    mr.assert_moments(mean, var, ref, W, share)


def test_the_variance_is_the_central_form():
    rows, V = mr.spread_row()
    ref = mr.moments_ref(rows, V)
    mean, var, share, _ = raw(rows, V)
    mr.assert_moments(mean, var, ref, rows.shape[1], share)


# ---- reproducibility -------------------------------------------------------------------------------------------------------------
def test_same_bits_chunked_device_permuted_and_alone():
    N, W, M, L = 700, 257, 1000, 5
    rows, nbr, nnbr, sc, V, Ve, Vm = sparse_case(N, W, M, L, 4, counts=[])
    base = raw(rows, V, Ve, Vm, sc, nbr, nnbr)
    eng = engine()
    old = eng.workspace_limit()
    eng.set_workspace_limit(1 << 20)                                 # 3 x 2056 + 8 + 120 bytes per object: five chunks
    try:
        small = raw(rows, V, Ve, Vm, sc, nbr, nnbr)
    finally:
        eng.set_workspace_limit(old)
    d_mean, d_var, d_share = (DevArray(np.zeros((N, L))) for _ in range(3))
    ns = eng.row_moments(DevArray(rows), N, W, M, L, DevArray(V), d_mean, var=d_var, share=d_share, value_errs=DevArray(Ve), value_mask=DevArray(Vm),
                         scale=DevArray(sc), neighbors=DevArray(nbr), nnbr=DevArray(nnbr))
    dev = tuple(dr_numpy(a, (N, L)) for a in (d_mean, d_var, d_share)) + (ns,)
    perm = np.random.RandomState(1).permutation(N)
    pm = raw(rows[perm], V, Ve, Vm, sc[perm], nbr[perm], nnbr[perm])
    sub = raw(rows[100:103], V, Ve, Vm, sc[100:103], nbr[100:103], nnbr[100:103])
    for k in range(3):
        np.testing.assert_array_equal(small[k], base[k])
        np.testing.assert_array_equal(dev[k], base[k])
        np.testing.assert_array_equal(pm[k], base[k][perm])
        np.testing.assert_array_equal(sub[k], base[k][100:103])
    assert small[3] == base[3] == dev[3] == pm[3]


def dr_numpy(d, shape):
    """a DevArray's contents"""
    import ctypes as C
    out = np.empty(shape)
    assert DevArray._hip.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(d.data_ptr()), C.c_size_t(out.nbytes), 2) == 0
    return out


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from frankenz_amd import pdf
    rows, nbr, nnbr, sc, V, Ve, Vm = sparse_case(5, 65, 1000, 5, 5, counts=[65] * 5)
    for badv in (1000, -1):
        b = nbr.copy(); b[3, 64] = badv
        with pytest.raises(IndexError):
            raw(rows, V, Ve, Vm, sc, b, nnbr)
    c = nnbr.copy(); c[2] = 66
    with pytest.raises(IndexError):
        raw(rows, V, Ve, Vm, sc, nbr, c)
    b = nbr.copy(); b[3, 64] = 1000; c = nnbr.copy(); c[3] = 64      # a bad index past the count is never read
    raw(rows, V, Ve, Vm, sc, b, c)
    with pytest.raises(NotImplementedError):
        raw(rows, np.ones((1000, 33)), None, None, None, nbr, nnbr)
    with pytest.raises(ValueError):
        raw(rows, V, None, None, None, nbr, nnbr, L=0)
    for kw in (dict(value_errs=Ve[:, :4]), dict(value_mask=Vm[:-1]), dict(scale=sc[:, :-1]), dict(neighbors=nbr[:4], Nneighbors=nnbr),
               dict(neighbors=nbr), dict()):
        with pytest.raises(ValueError):                              # (the last: dense rows of 65 entries over 1000 models)
            pdf.posterior_moments(rows, V, **kw)


# ---- fitted problems -------------------------------------------------------------------------------------------------------------
def plane_bar(rows, rtol, atol):
    """what the planes' tolerance lets an entry that carries weight differ by, per object: entries more than 40 below the row's max
    weigh less than 4e-18 of it"""
    return (rtol * (np.abs(rows.max(axis=1)) + 40.) + atol)[:, None]


@pytest.mark.parametrize("B,free", [(5, False), (5, True), (12, True)])
def test_predict_phot_of_the_three_fitters(B, free):
    import frankenz_oracle as fo
    from frankenz_amd import BruteForce, NearestNeighbors
    X, Xe, Xm, Y, Ye, Ym, _ = dr.masked_problem(B)
    kw = dict(free_scale=True) if free else {}
    M = len(Y)
    # dense
    bf = BruteForce(Y, Ye, Ym)
    bf.fit(X.copy(), Xe.copy(), Xm.copy(), lprob_kwargs=kw, track_scale=True, verbose=False)
    got = bf.predict_phot()
    ref = mr.moments_ref(bf.fit_lnprob, Y, Ye, Ym, bf.fit_scale)
    mr.assert_moments(got[0], got[1], ref, M, got[2])
    # ... and against the oracle's planes, at the planes' own tolerance (tests/test_hip_parity.py: ln-posterior rtol 1e-7 / atol 1e-9
    # with a free scale, 1e-9 / 1e-10 without; the scale 1e-8): rows off by d change every normalised weight by <= 2 d relative, which
    # moves the mean by <= 4 d A and the variance by <= 4 d var + the square of the mean's move
    o = fo.bruteforce_fit(X.copy(), Xe.copy(), Xm.copy(), Y, Ye, Ym, track_scale=free, **(dict(kw, return_scale=True) if free else kw))
    oref = mr.moments_ref(o['lnprob'], Y, Ye, Ym, o['scale'])
    d = plane_bar(o['lnprob'], *((1e-7, 1e-9) if free else (1e-9, 1e-10))) + (1e-8 if free else 0.)
    ok = np.isfinite(oref[0])
    d = np.broadcast_to(d, oref[0].shape)[ok]
    mean_bar = (4. * d + mr.sum_tol(M)) * oref[4][ok]
    var_bar = (4. * d + mr.sum_tol(M)) * oref[1][ok] + mean_bar ** 2 + 4. * mr.U * oref[4][ok] * np.sqrt(oref[1][ok])
    assert (np.abs(got[0] - oref[0])[ok] <= mean_bar).all()
    assert (np.abs(got[1] - oref[1])[ok] <= var_bar).all()
    # without model errors, and a label's moments
    z, ze = np.random.RandomState(3).uniform(0., 6., M), np.full(M, 0.05)
    for v, ve in ((Y, None), (z[:, None], ze[:, None])):
        got = bf.moments(v, ve, use_scale=ve is None)
        ref = mr.moments_ref(bf.fit_lnprob, v, ve, None, bf.fit_scale if ve is None else None)
        mr.assert_moments(got[0], got[1], ref, M)
    assert bf.moments(z, ze)[0].shape == (len(X),)
    # sparse rows of the exhaustive fit
    sp = bf.fit_sparse(X.copy(), Xe.copy(), Xm.copy(), Nkeep=64, lprob_kwargs=kw, track_scale=True, verbose=False)
    got = sp.predict_phot(Y, Ye, Ym)
    ref = mr.moments_ref(sp.fit_lnprob, Y, Ye, Ym, sp.fit_scale, sp.neighbors, sp.Nneighbors)
    mr.assert_moments(got[0], got[1], ref, 64, got[2])
    got = sp.moments(z, ze)
    mr.assert_moments(got[0][:, None], got[1][:, None], mr.moments_ref(sp.fit_lnprob, z[:, None], ze[:, None], None, None, sp.neighbors, sp.Nneighbors), 64)
    # k-NN
    nn = NearestNeighbors(Y, Ye, Ym, K=4, rstate=np.random.RandomState(1), verbose=False)
    nn.fit(X.copy(), Xe.copy(), Xm.copy(), rstate=np.random.RandomState(2), k=5, lprob_kwargs=kw, track_scale=True, verbose=False)
    got = nn.predict_phot()
    W = nn.neighbors.shape[1]
    ref = mr.moments_ref(nn.fit_lnprob, Y, Ye, Ym, nn.fit_scale, nn.neighbors, nn.Nneighbors)
    mr.assert_moments(got[0], got[1], ref, W, got[2])
    got = nn.moments(z, ze)
    mr.assert_moments(got[0][:, None], got[1][:, None], mr.moments_ref(nn.fit_lnprob, z[:, None], ze[:, None], None, None, nn.neighbors, nn.Nneighbors), W)


# ---- phot_sums -------------------------------------------------------------------------------------------------------------------
def phot_case(N=12000, B=5):
    rs = np.random.RandomState(61)
    p = rs.lognormal(1., 1., size=(N, B)); v = (0.05 * p) ** 2
    xe = 0.1 * p
    x = np.abs(p * 1.03 + xe * rs.randn(N, B)) + 0.01
    xm = (rs.rand(N, B) > 0.1).astype(np.float64)
    xm[:, 3] = 0.                                                    # a band with no usable object
    p[5, 0] = np.nan; v[6, 1] = np.nan; x[7, 2] = np.inf; xe[8, 0] = np.nan      # skipped
    # an object-band exactly at the clip (xe^2 + v = 1, d = 3, clip = 3): included; one just beyond: clipped
    x[10, 0], p[10, 0], xe[10, 0], v[10, 0], xm[10, 0] = 5., 2., 0.5, 0.75, 1.
    x[11, 0], p[11, 0], xe[11, 0], v[11, 0], xm[11, 0] = 5.5, 2., 0.5, 0.75, 1.
    return x, xe, xm, p, v


@pytest.mark.parametrize("clip", [None, 3.])
def test_phot_sums(clip):
    from frankenz_amd import calibrate
    x, xe, xm, p, v = phot_case()
    N = len(x)
    A, B, C, n, nclip = mr.phot_sums_ref(x, xe, xm, p, v, clip)
    got = calibrate.phot_sums(x, xe, xm, p, v, clip=clip)
    np.testing.assert_array_equal(got.n, n)
    np.testing.assert_array_equal(got.nclip, nclip)
    assert n[3] == 0 and got.A[3] == 0. and np.isnan(got.factor[3])
    rtol = (N / mr.STRIP + 16) * 4 * mr.U
    for g, r in ((got.A, A), (got.B, B), (got.C, C)):
        np.testing.assert_allclose(g, r.astype(np.float64), rtol=rtol, atol=0.)
    if clip:
        assert nclip[0] >= 1 and nclip.sum() > 1
        keep = calibrate.phot_sums(x[10:11], xe[10:11], xm[10:11], p[10:11], v[10:11], clip=clip)
        assert keep.n[0] == 1 and keep.nclip[0] == 0 and keep.C[0] == 9.
        out = calibrate.phot_sums(x[11:12], xe[11:12], xm[11:12], p[11:12], v[11:12], clip=clip)
        assert out.n[0] == 0 and out.nclip[0] == 1
    # chunked host arrays against device arrays, bit for bit
    eng = engine()
    old = eng.workspace_limit()
    eng.set_workspace_limit(1 << 20)                                 # 200 bytes per object: chunks of five strips, three of them
    try:
        small = calibrate.phot_sums(x, xe, xm, p, v, clip=clip)
    finally:
        eng.set_workspace_limit(old)
    dev = calibrate.phot_sums(*(DevArray(a) for a in (x, xe, xm, p, v)), clip=clip)
    for o in (small, dev):
        for k in ('A', 'B', 'C', 'n', 'nclip'):
            np.testing.assert_array_equal(getattr(o, k), getattr(got, k))
    with pytest.raises(ValueError):
        calibrate.phot_sums(x, xe, xm, p[:-1], v)


# ---- zeropoint_offsets -----------------------------------------------------------------------------------------------------------
def test_zeropoint_offsets_follow_the_reference_iteration():
    from frankenz_amd import BruteForce, NearestNeighbors, calibrate
    X, Xe, Xm, Y, Ye, Ym = mr.zp_problem()
    keep = X.copy(), Xe.copy(), Xm.copy()
    bf = BruteForce(Y, Ye, Ym)
    res = calibrate.zeropoint_offsets(bf, X, Xe, Xm, Niter=10, tol=1e-4, ref_band=0, Nkeep=64, verbose=False)

    def moments(xs, xes, xm):                                        # the reference law on the device's own rows
        sp = bf.fit_sparse(xs, xes, xm, Nkeep=64, track_scale=True, verbose=False)
        mean, var, _, _, _ = mr.moments_ref(sp.fit_lnprob, Y, Ye, Ym, sp.fit_scale, sp.neighbors, sp.Nneighbors)
        return mean, var

    a, trace, sums, converged = mr.zeropoints_ref(moments, X, Xe, Xm, Niter=10, tol=1e-4, ref_band=0)
    for got, was in zip((X, Xe, Xm), keep):
        np.testing.assert_array_equal(got, was)
    assert res.converged and converged and res.trace.shape == trace.shape
    np.testing.assert_allclose(res.trace, trace, rtol=1e-10, atol=0.)
    np.testing.assert_allclose(res.offsets, a, rtol=1e-10, atol=0.)
    np.testing.assert_array_equal(res.sums.n, sums[3])
    with pytest.raises(ValueError):
        calibrate.zeropoint_offsets(bf, X, Xe, Xm, lprob_kwargs=dict(free_scale=True), verbose=False)
    nn = NearestNeighbors(Y, Ye, Ym, K=4, rstate=np.random.RandomState(1), verbose=False)
    res = calibrate.zeropoint_offsets(nn, X, Xe, Xm, Niter=10, tol=1e-3, ref_band=0, rstate=np.random.RandomState(2), fit_kwargs=dict(k=5),
                                      verbose=False)
    assert res.converged and np.isfinite(res.offsets).all() and res.offsets[0] == 1.
