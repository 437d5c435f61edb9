"""The law of the posterior moments, the zero-point sums and the zero-point iteration (include/frankenz_hip.h, docs/predictive.md),
restated in `np.longdouble` as plain loops: what tests/test_moments_host.py checks against float64 formulas and
tests/test_hip_moments.py holds the kernels to."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
STRIP = 1024                    # objects of a strip of fz_phot_sums (NZ_CHUNK)


def sum_tol(W):
    """relative error of one fixed-order sum of W terms against its sum of absolute terms, times the safety factor 4: a thread adds
    ceil(W / 64) terms at most, the butterfly has six levels, and 16 covers exp, the product, the division and (rows of more than
    4096 entries, where a thread adds W / 256 terms) the three additions of the four wave sums"""
    return 4. * (W / 64. + 16.) * U


def moments_ref(rows, V, Ve=None, Vm=None, scale=None, neighbors=None, nnbr=None):
    """-> mean, var, share (N, L) float64, nskip, and A (N, L) = sum w |c| / Z_l, the scale of the rounding bound of the mean"""
    rows = np.asarray(rows, dtype=np.float64)
    V = np.asarray(V, dtype=np.float64)
    N, W = rows.shape
    M, L = V.shape
    mean, var, share, A = (np.full((N, L), np.nan) for _ in range(4))
    share[:] = 0.
    nskip = 0
    for i in range(N):
        n = W if nnbr is None else int(nnbr[i])
        r = rows[i, :n]
        if n == 0 or np.isnan(r).any() or not np.isfinite(r.max()):
            nskip += 1
            continue
        j = np.arange(n) if neighbors is None else np.asarray(neighbors[i, :n])
        assert ((j >= 0) & (j < M)).all()
        w = np.exp((r - r.max()).astype(LD))
        keep = np.exp(r - r.max()) > 0                                # the float64 weight decides what counts (no 0 * inf)
        w, j = w[keep], j[keep]
        s = np.ones(len(j)) if scale is None else np.asarray(scale[i, :n], dtype=np.float64)[keep]
        Z = w.sum()
        with np.errstate(invalid='ignore', over='ignore'):
            for l in range(L):
                inc = np.ones(len(j), dtype=bool) if Vm is None else (np.asarray(Vm)[j, l] != 0)
                if not inc.any():
                    continue
                wl = w[inc]
                c = (s[inc] * V[j[inc], l]).astype(LD)                # one float64 rounding, as the law says
                Zl = wl.sum()
                mu = (wl * c).sum() / Zl
                v = (wl * (c - mu) ** 2).sum() / Zl
                if Ve is not None:
                    se = (s[inc] * np.asarray(Ve, dtype=np.float64)[j[inc], l]).astype(LD)
                    v = v + (wl * se ** 2).sum() / Zl
                mean[i, l], var[i, l], share[i, l] = float(mu), float(v), float(Zl / Z)
                A[i, l] = float((wl * np.abs(c)).sum() / Zl)
    return mean, var, share, nskip, A


def assert_moments(got_mean, got_var, ref, W, got_share=None):
    """the derived bars: |mean - ref| <= tol A; |var - ref| <= tol var_ref + 4 u A sqrt(var_ref) (+ the mean's own error squared, which
    the central form carries exactly: (c - mean)^2 about a mean off by e adds e^2); nan and inf must match in place"""
    mean, var, share, _, A = ref
    tol = sum_tol(W)
    for got, want in ((got_mean, mean), (got_var, var)):
        if got is not None:
            np.testing.assert_array_equal(np.isfinite(got), np.isfinite(want))
            np.testing.assert_array_equal(got[~np.isfinite(want)], want[~np.isfinite(want)])
    ok = np.isfinite(mean)
    err = np.abs(got_mean[ok] - mean[ok])
    assert (err <= tol * A[ok]).all(), "mean: worst %.3g of its bar" % np.max(err / (tol * A[ok] + 1e-300))
    if got_var is not None:
        ok = np.isfinite(var)
        bar = tol * var[ok] + 4. * U * A[ok] * np.sqrt(var[ok]) + (tol * A[ok]) ** 2
        err = np.abs(got_var[ok] - var[ok])
        assert (err <= bar).all(), "var: worst %.3g of its bar" % np.max(err / (bar + 1e-300))
    if got_share is not None:
        np.testing.assert_allclose(got_share, share, rtol=2. * tol, atol=0.)


def phot_sums_ref(x, xe, xm, p, v, clip=None):
    """-> A, B, C (longdouble, per band), n, nclip"""
    x, xe, xm, p, v = (np.asarray(a, dtype=np.float64) for a in (x, xe, xm, p, v))
    Bn = x.shape[1]
    A, B, C = np.zeros(Bn, dtype=LD), np.zeros(Bn, dtype=LD), np.zeros(Bn, dtype=LD)
    n, nclip = np.zeros(Bn, dtype=np.int64), np.zeros(Bn, dtype=np.int64)
    for b in range(Bn):
        ok = (xm[:, b] != 0) & np.isfinite(x[:, b]) & np.isfinite(xe[:, b]) & np.isfinite(p[:, b]) & np.isfinite(v[:, b])
        xb, eb, pb, vb = (a[ok, b].astype(LD) for a in (x, xe, p, v))
        w = 1 / (eb * eb + vb)
        d = xb - pb
        if clip is not None:
            # the decision is the float64 one of the kernel: w d d against clip clip, each product rounded
            w64 = 1. / (xe[ok, b] * xe[ok, b] + v[ok, b]); d64 = x[ok, b] - p[ok, b]
            out = w64 * d64 * d64 > clip * clip
            nclip[b] = out.sum()
            xb, pb, w, d = xb[~out], pb[~out], w[~out], d[~out]
        A[b], B[b], C[b], n[b] = (w * xb * pb).sum(), (w * pb * pb).sum(), (w * d * d).sum(), len(xb)
    return A, B, C, n, nclip


def zeropoints_ref(moments, x, xe, xm, Niter=10, tol=1e-4, ref_band=None, clip=None):
    """the iteration of calibrate.zeropoint_offsets with `moments(xs, xes, xm) -> (phot_mean, phot_var)` passed in
    -> offsets, trace (iterations, B), the last (A, B, C, n, nclip), converged"""
    x, xe, xm = (np.asarray(a, dtype=np.float64) for a in (x, xe, xm))
    a = np.ones(x.shape[1])
    trace, sums, converged = [], None, False
    for _ in range(Niter):
        xs, xes = x / a, xe / a
        pm, pv = moments(xs.copy(), xes.copy(), xm.copy())
        sums = phot_sums_ref(xs, xes, xm, pm, pv, clip)
        with np.errstate(divide='ignore', invalid='ignore'):
            f = np.where(sums[3] > 0, (sums[0] / sums[1]).astype(np.float64), 1.)
        if ref_band is not None:
            f = np.where(sums[3] > 0, f / f[ref_band], 1.)
        a = a * f
        trace.append(a.copy())
        if np.max(np.abs(f - 1.)) < tol:
            converged = True
            break
    return a, np.array(trace), sums, converged


def spread_row(W=500, rel=1e-6, seed=4):
    """values that spread by `rel` relative about 1: the variance is ~ rel^2, far below the rounding of sum w c^2"""
    rs = np.random.RandomState(seed)
    rows = -rs.uniform(0., 3., size=(1, W))
    V = (1. + rel * rs.randn(W))[:, None]
    return rows, V


# ---- the zero-point problem both test files use ------------------------------------------------------------------------------------
ZP_OFFSETS = np.array([1., 1.05, 0.93, 1., 1.10])


def zp_problem(N=300, M=200, seed=0):
    """objects drawn uniformly FROM the model set, 3 % photometric errors, the catalogue multiplied by ZP_OFFSETS per band, 5 % of the
    object-bands masked; model errors 1 %, no model masks"""
    rs = np.random.RandomState(8800 + seed)
    B = len(ZP_OFFSETS)
    Y = rs.lognormal(1., 1., size=(M, B)); Ye = 0.01 * Y; Ym = np.ones((M, B))
    truth = Y[rs.choice(M, N)]
    Xe = 0.03 * truth
    X = (truth + Xe * rs.randn(N, B)) * ZP_OFFSETS
    Xe = Xe * ZP_OFFSETS
    Xm = (rs.rand(N, B) >= 0.05).astype(np.float64)
    Xm[Xm.sum(axis=1) == 0, 0] = 1.
    return X, Xe, Xm, Y, Ye, Ym
