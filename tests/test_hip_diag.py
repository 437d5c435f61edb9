"""GPU parity of frankenz_amd.plotting (fz_stack2d, fz_recentre_rows, fz_cdf_draws): against the reference's recorded results (G19)
and, at shapes the fixture does not hold, against the NumPy restatement tests/_diag_ref.py.

Tolerances, with u = 2^-53 (derived, not tuned):
* a stack cell is a sum of at most n non-negative terms (n selected objects), each carrying the error of two normalising sums of at
  most Gx and Gy non-negative terms and a handful of roundings: rtol = 4 (n + Gx + Gy) u, atol = 0, and a cell the reference leaves
  at 0 is exactly 0;
* a CDF draw lies in [0, 1] and comes from a running sum of G non-negative terms: atol = 4 (G + 8) u, no rtol; a clamped draw of
  exactly 1 is exactly 1;
* histogram counts against np.histogram of the SAME draws: rtol = 4 N Nmc u (sums of at most N Nmc non-negative terms); the
  density-normalised histogram against G19's, a ratio of two such sums: rtol = 8 N Nmc u;
* a recentred row is np.interp's four operations on the same operands in the same order: rtol = 8 u should a last bit differ."""
import numpy as np
import pytest

import _diag_ref as ref
from conftest import DevArray, load_golden

pytestmark = pytest.mark.gpu
U = 2.0 ** -53


def stack_close(got, want, n, where=''):
    gx, gy = want.shape
    assert got.shape == want.shape
    assert np.isfinite(got).all(), where
    assert np.array_equal(got == 0, want == 0), where          # exactly zero where the reference is
    np.testing.assert_allclose(got, want, rtol=4 * (n + gx + gy) * U, atol=0, err_msg=where)


@pytest.fixture(scope='module')
def g19():
    g = load_golden('g19_diagnostics')
    return g, ref.StoredDict(g)


@pytest.fixture(scope='module')
def demo_dict():
    from frankenz_amd import PDFDict
    return PDFDict(np.arange(0, 7 + 1e-5, .01), np.linspace(.005, 2, 500))


def make_case(seed, n, vdict, gy, emax, vlo=None, vhi=None):
    """n objects for ``vdict``: truths from beyond both ends of its grid (windows clipped at both ends; an object off the grid gets
    an error wide enough to reach it), PDFs of one Gaussian on a floor on a gy-point grid over the same range; from 16 objects on,
    one row of all zeros and two weights below the default cut"""
    rs = np.random.RandomState(seed)
    lo, hi = vdict.grid[0], vdict.grid[-1]
    span = hi - lo
    vlo, vhi = (lo - 0.05 * span if vlo is None else vlo), (hi + 0.05 * span if vhi is None else vhi)
    pgrid = np.linspace(lo, hi, gy)
    vals = rs.uniform(vlo, vhi, n)
    errs = rs.uniform(vdict.sigma_grid[0], emax, n)
    off = np.maximum(np.maximum(lo - vals, vals - hi), 0.)
    errs = np.maximum(errs, off / 5. + 2 * vdict.dsigma + vdict.delta)
    mu, sd = rs.uniform(lo, hi, n), rs.uniform(0.01, 0.12, n) * span
    pdfs = np.exp(-0.5 * np.square((pgrid[None, :] - mu[:, None]) / sd[:, None])) + 1e-5 * rs.rand(n, gy)
    pdfs /= pdfs.sum(axis=1)[:, None]
    weights = rs.uniform(0.05, 1., n)
    if n >= 16:
        pdfs[3] = 0.
        weights[[1, 9]] = 1e-5
    return vals, errs, pdfs, pgrid, weights


# ---- 1. G19: every recorded stack and both PIT outputs -----------------------------------------------------------------------
G19_STACKS = {
    'stack_default': lambda g: {},
    'stack_harsh': lambda g: dict(pdf_wt_thresh=g['harsh'][0], wt_thresh=g['harsh'][1]),
    'stack_obj_cdf': lambda g: dict(wt_thresh=None, cdf_thresh=float(g['obj_cdf_thresh'])),
    'stack_pdf_cdf': lambda g: dict(pdf_wt_thresh=None, pdf_cdf_thresh=float(g['pdf_cdf_thresh'])),
}


@pytest.mark.parametrize('name', sorted(G19_STACKS))
def test_g19_input_vs_pdf(g19, name):
    from frankenz_amd import plotting
    g, d = g19
    got = plotting.input_vs_pdf(g['vals'], g['errs'], d, g['pdfs'], g['pgrid'], weights=g['weights'], plot=False,
                                **G19_STACKS[name](g))
    stack_close(got, g[name], len(g['vals']), name)


@pytest.mark.parametrize('name', ['dstack_default', 'dstack_scaled'])
def test_g19_input_vs_dpdf(g19, name):
    from frankenz_amd import plotting
    g, d = g19
    disp = plotting.disp_scaled if name == 'dstack_scaled' else None
    got = plotting.input_vs_dpdf(g['vals'], g['errs'], d, g['pdfs'], g['pgrid'], g['pdf_cent'], g['dgrid'], weights=g['weights'],
                                 disp_func=disp, plot=False)
    stack_close(got, g[name], len(g['vals']), name)


def test_g19_input_vs_dpdf_callable_dispersion_takes_the_host_path(g19):
    from frankenz_amd import plotting
    g, d = g19
    got = plotting.input_vs_dpdf(g['vals'], g['errs'], d, g['pdfs'], g['pgrid'], g['pdf_cent'], g['dgrid'], weights=g['weights'],
                                 disp_func=lambda p, c, s: (p - c) / (s + c), disp_args=[1.], plot=False)
    stack_close(got, g['dstack_scaled'], len(g['vals']))


def test_g19_pit(g19):
    from frankenz_amd import plotting
    g, _ = g19
    nmc, nbins, seed = int(g['nmc']), int(g['nbins']), int(g['seed'])
    n_obj, G = g['pdfs'].shape
    a = (g['vals'], g['errs'], g['pdfs'], g['pgrid'])
    n = plotting.cdf_vs_epdf(*a, Nmc=nmc, weights=g['weights'], Nbins=nbins, rstate=np.random.RandomState(seed), plot=False)
    print('epdf max rel', np.abs(n / g['epdf_n'] - 1).max())
    np.testing.assert_allclose(n, g['epdf_n'], rtol=8 * n_obj * nmc * U, atol=0)
    x, y = plotting.cdf_vs_ecdf(*a, Nmc=nmc, rstate=np.random.RandomState(seed), plot=False)
    # x: running sum of unit weights, exact.  y: running sum of the sorted draws' spacings = the sorted draws themselves up to the
    # draws' own bound, divided by the last one (a draw of exactly 1 here)
    assert np.array_equal(x, g['ecdf_x'])
    np.testing.assert_allclose(y, g['ecdf_y'], rtol=0, atol=2 * 4 * (G + 8) * U + 4 * n_obj * nmc * U)


# ---- 2. shapes at which the tiling can go wrong ----------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 5, 16, 17, 3000])
def test_stack_150_by_77(g19, n):
    """neither side a multiple of 16, x crosses a 128 tile edge; 1 and 5 objects are below one k-step, 3000 give several splits with
    a ragged last one; from 16 objects on the case holds a zero row and objects the weight rule drops"""
    from frankenz_amd import plotting
    _, d = g19
    vals, errs, pdfs, pgrid, w = make_case(100 + n, n, d, 77, 0.28)
    got = plotting.input_vs_pdf(vals, errs, d, pdfs, pgrid, weights=w, plot=False)
    want = ref.input_vs_pdf(vals, errs, d, pdfs, pgrid, weights=w)
    stack_close(got, want, n)
    assert (got != 0).any()


@pytest.mark.parametrize('n', [17, 3000])
def test_stack_701_by_701_demo_dictionary(demo_dict, n):
    from frankenz_amd import plotting
    vals, errs, pdfs, pgrid, w = make_case(200 + n, n, demo_dict, 701, 0.3)
    got = plotting.input_vs_pdf(vals, errs, demo_dict, pdfs, pgrid, weights=w, plot=False)
    want = ref.input_vs_pdf(vals, errs, demo_dict, pdfs, pgrid, weights=w)
    stack_close(got, want, n)


# ---- 3. empty tile ranges ---------------------------------------------------------------------------------------------------------
def test_objects_in_the_left_tenth_leave_the_other_tiles_zero(demo_dict):
    from frankenz_amd import plotting
    vals, errs, pdfs, pgrid, w = make_case(31, 400, demo_dict, 701, 0.04, vlo=0., vhi=0.7)
    assert (demo_dict.sigma_width[demo_dict.fit(vals, errs)[1]] <= 30).all()
    got = plotting.input_vs_pdf(vals, errs, demo_dict, pdfs, pgrid, weights=w, plot=False)
    assert (got[128:] == 0).all() and np.isfinite(got).all()
    stack_close(got, ref.input_vs_pdf(vals, errs, demo_dict, pdfs, pgrid, weights=w), 400)


# ---- 4. clipped windows, a row of zeros, dropped objects ---------------------------------------------------------------------------
def test_clipped_windows_zero_row_and_dropped_objects(g19):
    from frankenz_amd import plotting
    _, d = g19
    vals, errs, pdfs, pgrid, w = make_case(41, 40, d, 77, 0.28)
    vals[:4] = [-0.2, 3.2, 0.01, 2.99]                     # centres off both ends and just inside them
    errs[:4] = [0.2, 0.2, 0.28, 0.28]
    ci, ei = d.fit(vals, errs)
    hw = d.sigma_width[ei]
    assert ci[0] < 0 and ci[1] > d.Ngrid - 1 and ci[2] - hw[2] < 0 and ci[3] + hw[3] > d.Ngrid - 1
    assert not pdfs[3].any() and (w[[1, 9]] < 1e-3 * w.max()).all()
    got = plotting.input_vs_pdf(vals, errs, d, pdfs, pgrid, weights=w, plot=False)
    stack_close(got, ref.input_vs_pdf(vals, errs, d, pdfs, pgrid, weights=w), 40)
    # the zero row and the dropped objects add nothing: the same stack without them
    keep = np.ones(40, dtype=bool)
    keep[[1, 3, 9]] = False
    wk = w[keep]
    sub = plotting.input_vs_pdf(vals[keep], errs[keep], d, pdfs[keep], pgrid, weights=wk, plot=False)
    stack_close(sub, got, 40)
    # every object's cells sum to its weight (np.sum's pairwise order adds a few u)
    np.testing.assert_allclose(got.sum(), wk.sum(), rtol=(4 * (40 + 150 + 77) + 32) * U)
    # no per-PDF cut at all (both thresholds None): 0 * -inf must not leak a nan from the zero row
    got = plotting.input_vs_pdf(vals, errs, d, pdfs, pgrid, weights=w, pdf_wt_thresh=None, pdf_cdf_thresh=None, plot=False)
    stack_close(got, ref.input_vs_pdf(vals, errs, d, pdfs, pgrid, weights=w, pdf_wt_thresh=None, pdf_cdf_thresh=None), 40)


# ---- 5 / 6. the same bits twice, and from host and resident PDFs -------------------------------------------------------------------
def test_run_to_run_bits_and_resident_input(g19):
    from frankenz_amd import plotting
    _, d = g19
    vals, errs, pdfs, pgrid, w = make_case(51, 3000, d, 77, 0.28)
    a = plotting.input_vs_pdf(vals, errs, d, pdfs, pgrid, weights=w, plot=False)
    b = plotting.input_vs_pdf(vals, errs, d, pdfs, pgrid, weights=w, plot=False)
    assert np.array_equal(a, b)
    dev = DevArray(pdfs)
    c = plotting.input_vs_pdf(vals, errs, d, dev, pgrid, weights=w, plot=False)
    assert np.array_equal(a, c)
    cent = (pdfs * pgrid).sum(axis=1)
    dgrid = np.linspace(-1., 1., 45)
    e = plotting.input_vs_dpdf(vals, errs, d, pdfs, pgrid, cent, dgrid, weights=w, plot=False)
    f = plotting.input_vs_dpdf(vals, errs, d, dev, pgrid, cent, dgrid, weights=w, plot=False)
    assert np.array_equal(e, f)
    stack_close(e, ref.input_vs_dpdf(vals, errs, d, pdfs, pgrid, cent, dgrid, weights=w), 3000)


def test_chunked_host_rows_give_the_stack_of_one_chunk(g19):
    """a workspace limit that forces the host rows through several chunks: the chunk stacks add up in chunk order"""
    from frankenz_amd import plotting
    from frankenz_amd.engine import get_engine
    _, d = g19
    vals, errs, pdfs, pgrid, w = make_case(52, 3000, d, 77, 0.28)
    want = ref.input_vs_pdf(vals, errs, d, pdfs, pgrid, weights=w)
    eng = get_engine()
    try:
        eng.set_workspace_limit(1 << 20)                       # the smallest limit: half of it stages 851 rows of 77 doubles
        got = plotting.input_vs_pdf(vals, errs, d, pdfs, pgrid, weights=w, plot=False)
    finally:
        eng.set_workspace_limit(32 << 30)
    stack_close(got, want, 3000)


def test_resident_rows_that_are_not_finite_are_refused(g19):
    from frankenz_amd import plotting
    _, d = g19
    vals, errs, pdfs, pgrid, w = make_case(53, 64, d, 77, 0.28)
    pdfs[1, 5] = np.nan                                     # a dropped object: not looked at
    plotting.input_vs_pdf(vals, errs, d, DevArray(pdfs), pgrid, weights=w, plot=False)
    pdfs[20, 76] = np.inf
    with pytest.raises(ValueError, match='row 20 '):
        plotting.input_vs_pdf(vals, errs, d, DevArray(pdfs), pgrid, weights=w, plot=False)


# ---- 7. k_recentre ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('disp', [0, 1])
def test_recentre_rows_against_np_interp(disp):
    from frankenz_amd.engine import get_engine
    rs = np.random.RandomState(7)
    n, G, Gd = 37, 333, 101
    pgrid = np.linspace(0., 4., G)
    pdfs = rs.rand(n, G)
    cent = rs.uniform(0.2, 3.8, n)
    cent[:2] = [0.1, 3.9]                                   # dgrid hangs off the low end, then off the high end
    dgrid = np.linspace(-1.5, 1.5, Gd)
    f = (lambda p, c: (p - c) / (1. + c)) if disp else (lambda p, c: p - c)
    want = np.array([np.interp(dgrid, f(pgrid, c), p) for p, c in zip(pdfs, cent)])
    assert (dgrid[0] < f(pgrid, cent[0])[0]) and (dgrid[-1] > f(pgrid, cent[1])[-1])
    for src in (pdfs, DevArray(pdfs)):
        got = np.empty((n, Gd))
        get_engine().recentre_rows(src, n, pgrid, cent, disp, dgrid, got)
        np.testing.assert_allclose(got, want, rtol=8 * U, atol=0)
    assert np.array_equal(got[0, dgrid < f(pgrid, cent[0])[0]], np.full((dgrid < f(pgrid, cent[0])[0]).sum(), pdfs[0, 0]))


# ---- 8. PIT ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('G,n', [(701, 300), (5000, 50)])
@pytest.mark.parametrize('nmc', [1, 100])
def test_cdf_draws_and_histogram(G, n, nmc):
    """grids of 701 (four waves per block) and 5000 points (two); truths outside the grid on both sides clamp; a zero error"""
    from frankenz_amd.engine import get_engine
    from frankenz_amd import plotting
    rs = np.random.RandomState(G + nmc)
    grid = np.linspace(0., 7., G)
    mu, sd = rs.uniform(0.2, 6.8, n), rs.uniform(0.05, 0.8, n)
    pdfs = np.exp(-0.5 * np.square((grid[None, :] - mu[:, None]) / sd[:, None]))
    pdfs[rs.rand(n, G) < 0.1] = 0.                         # plateaus in the CDFs
    # weights in eighths: every partial sum of np.histogram's cumulative-sum-and-difference is exact, so that the comparison of the
    # counts tests the bin rule and the device's sum, not NumPy's rounding (which is relative to the total, not to a bin)
    vals, errs, w = mu + 0.3 * rs.randn(n), rs.uniform(0.01, 0.5, n), rs.randint(1, 17, n) / 8.
    vals[:2], errs[:2] = [-1., 8.5], [0.05, 0.05]          # off the low end, off the high end
    errs[2] = 0.
    mc = plotting._mc_truths(vals, errs, nmc, np.random.RandomState(5))
    assert (mc[0] < 0).all() and (mc[1] > 7).all() and (mc[2] == vals[2]).all()
    want = ref.cdf_draws(vals, errs, pdfs, grid, nmc, np.random.RandomState(5))
    nbins = 50
    edges = np.linspace(0., 1., nbins + 1)
    for src in (pdfs, DevArray(pdfs)):
        draws, hist = np.empty((n, nmc)), np.empty(nbins)
        get_engine().cdf_draws(src, n, grid, mc, weights=w, edges=edges, draws=draws, hist=hist)
        print('draws max abs', np.abs(draws - want).max())
        np.testing.assert_allclose(draws, want, rtol=0, atol=4 * (G + 8) * U)
        assert (draws[1] == 1.).all()                          # clamped at the high end: exactly 1
        counts, _ = np.histogram(draws.ravel(), bins=edges, weights=np.repeat(w, nmc))
        np.testing.assert_allclose(hist, counts, rtol=4 * n * nmc * U, atol=0)
        only = np.empty(nbins)
        get_engine().cdf_draws(src, n, grid, mc, weights=w, edges=edges, hist=only)   # the histogram alone: the same bits
        assert np.array_equal(only, hist)
    n_pub = plotting.cdf_vs_epdf(vals, errs, pdfs, grid, Nmc=nmc, weights=w, Nbins=nbins, rstate=np.random.RandomState(5), plot=False)
    assert np.array_equal(n_pub, hist / hist.sum() / np.diff(edges))


def test_histogram_bin_rule_on_the_edges():
    """draws that ARE bin edges: a single-bin PDF at the grid's second point makes the CDF a step, so truths on grid points read
    exactly 0 or 1 and a truth between the first two points reads a multiple of 1/8 -- bin j holds edges[j] <= u < edges[j + 1],
    the last bin closed"""
    from frankenz_amd.engine import get_engine
    grid = np.arange(8.)
    pdfs = np.zeros((3, 8))
    pdfs[:, 1] = 1.
    mc = np.array([[0., 0.125, 0.25, 0.5], [0.75, 1., 5., 9.], [-3., 0.375, 0.625, 0.875]])
    edges = np.linspace(0., 1., 9)
    w = np.array([1., 10., 100.])
    draws, hist = np.empty((3, 4)), np.empty(8)
    get_engine().cdf_draws(pdfs, 3, grid, mc, weights=w, edges=edges, draws=draws, hist=hist)
    assert np.array_equal(draws, np.clip(mc, 0., 1.))
    counts, _ = np.histogram(draws.ravel(), bins=edges, weights=np.repeat(w, 4))
    assert np.array_equal(hist, counts)
    assert hist[7] == 30. + 100. and hist[0] == 1. + 100.  # u = 1 thrice (weight 10) and 0.875 land in the last bin


def test_cdf_draws_refuses_a_grid_beyond_the_lds_row():
    from frankenz_amd import plotting
    G = 19201
    with pytest.raises(NotImplementedError, match='19200'):
        plotting.cdf_vs_ecdf(np.ones(2), np.ones(2), np.ones((2, G)), np.arange(float(G)), Nmc=3, rstate=np.random.RandomState(0),
                             plot=False)
