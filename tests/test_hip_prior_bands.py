"""The prior-carrying likelihood kernels (``PhotSrc<BT, MODE, VAR, PRI>``, csrc/fz_kernels.h) at every compiled band count, in every
mode, arithmetic variant and prior kind, through ``k_fused`` at each of its launch geometries and through ``k_stats + k_kde``,
against the oracle fed a dense ln-prior formed in NumPy (docs/bpz_prior.md, "Coverage", has the matrix).

Problems, tables and oracle runs come from tests/_prior_case.py; tests/test_prior_bands_host.py checks there, without a GPU, that
every one of these problems would show a prior taken from the wrong row or the neighbouring model.  Model counts sit one past a tile
of the geometry that runs (and once at exactly two tiles), so the prior row is read across a tile boundary and in a short last tile.
In every case

* object 0 reads the last table row and object N - 1 row 0;
* one object (K_EX) alone has prior 0 (-inf) on the last two models and on the last model of the first tile, which between them
  hold its best fit: run again on the table without those entries, that object's row changes and no other;
* the interpolated form has an object on an interior node (f == 0), one on the top node (r = P - 2, f = 1) and one in a cell of
  two all-zero rows (all -inf: nan PDF);
* with masks, one object and one model lack their LAST real band (bit 31 / 23 of the mask word at 32 / 24 bands) beside a row
  index that is not zero.

Tolerances are the project's: PDFs rtol 1e-7 / atol 1e-13, ln-max and ln-evidence rtol 1e-9 / atol 1e-11 (``close`` of the two
older prior modules), fit_lnlike and fit_lnprob rtol 1e-9 / atol 1e-9 (test_oracle_parity_band_counts), fit_lnprior of a ln table
bit for bit, of the interpolated form within ``close_ln`` of test_hip_bpz_prior.py.  nan and infinities must sit where the oracle
has them.  The only rows left out are those with a pair of one usable band under the free scale with the dimensionality prior
(3 bands, mode B), undefined in the reference itself."""
import numpy as np
import pytest

import _prior_case as pc
import frankenz_oracle as fo

pytestmark = pytest.mark.gpu
WORST = {}                       # what was compared -> largest relative deviation seen (printed when the module's engine fixture ends)


def ident(c):
    return '%d-%s-M%d-%s-%s' % c


@pytest.fixture(scope='module')
def eng():
    """the engine; the cases' object and model counts are worked out for the compute-unit count the library itself reports.  When the
    module is done, the largest deviations seen go to stdout in one place (docs/bpz_prior.md quotes them)."""
    from frankenz_amd.engine import get_engine
    e = get_engine()
    assert e.cu_count() == pc.CU_COUNT
    yield e
    for tag in sorted(WORST):
        print('WORST %-28s %.3e' % (tag, WORST[tag]))


@pytest.fixture(scope='module')
def pdict():
    from frankenz_amd import PDFDict
    return PDFDict(*pc.grids())


def held(tag, got, want, rows, tol):
    """assert_allclose over ``rows`` after printing the worst relative deviation and where it is (entries smaller than atol / rtol
    are measured against that floor, as the tolerance does)"""
    got, want = np.asarray(got)[rows], np.asarray(want)[rows]
    with np.errstate(invalid='ignore'):
        dev = np.abs(got - want) / np.maximum(np.abs(want), tol['atol'] / tol['rtol'])
    dev = np.where(np.isfinite(dev), dev, 0.)                  # equal infinities, nan beside nan: assert_allclose looks at those
    w = float(dev.max()) if dev.size else 0.
    print('%s: worst relative deviation %.3e at %s' % (tag, w, np.unravel_index(dev.argmax(), dev.shape) if dev.size else ()))
    WORST[tag] = max(WORST.get(tag, 0.), w)
    np.testing.assert_allclose(got, want, equal_nan=True, **tol)


def held_ln(got, want):
    """``close_ln`` of test_hip_bpz_prior.py: -inf and nan where NumPy has them, else |difference| <= 6.3e-16 + 3.2e-16 |ln x|"""
    np.testing.assert_array_equal(np.isneginf(got), np.isneginf(want))
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    ok = np.isfinite(want)
    d = np.abs(got[ok] - want[ok])
    print('fit_lnprior: worst |difference| %.3e' % (d.max() if d.size else 0.))
    WORST['fit_lnprior (abs)'] = max(WORST.get('fit_lnprior (abs)', 0.), float(d.max()) if d.size else 0.)
    assert not d.size or (d - (6.3e-16 + 3.2e-16 * np.abs(want[ok]))).max() <= 0.


def run(pr, pri, mode, pdict, idx=None, plain=False):
    """fit_predict of the objects ``idx`` (in that order; None: all) through the public hook: (pdfs, lmap, levid)"""
    from frankenz_amd import BruteForce
    sel = slice(None) if idx is None else np.asarray(idx)
    with np.errstate(all='ignore'):
        p, (lm, le) = BruteForce(pr['Y'], pr['Ye'], pr['Ym']).fit_predict(
            pr['X'][sel].copy(), pr['Xe'][sel].copy(), pr['Xm'][sel].copy(), pr['z'], pr['ze'], lprob_func=pri.hook(idx, plain),
            lprob_kwargs=pc.MODES[mode], label_dict=pdict, return_gof=True, verbose=False, save_fits=False)
    return p, lm, le


def against_oracle(tag, got, ref, at):
    """rows ``at`` of the reference against the run's rows, in the run's order"""
    keep = ~ref['undef'][at].any(axis=1)
    fin = np.isfinite(ref['pdfs'][at][keep]).all(axis=1)
    assert fin.mean() >= 0.75, 'only %.2f of the compared rows are finite in the oracle' % fin.mean()
    held(tag + ' PDFs', got[0], ref['pdfs'][at], keep, pc.PDF_TOL)
    held(tag + ' lmap', got[1], ref['lmap'][at], keep, pc.GOF_TOL)
    held(tag + ' levid', got[2], ref['levid'][at], keep, pc.GOF_TOL)


def only_k_ex_changes(got, plain, k):
    """the run on the table without the excluding entries: the same bits everywhere but in row ``k``"""
    others = np.arange(len(got[0])) != k
    for a, b in zip(got, plain):
        np.testing.assert_array_equal(a[others], b[others])
    assert not np.array_equal(got[0][k], plain[0][k], equal_nan=True) and got[1][k] != plain[1][k]


# ---- 1: every unit at the (1, 4) geometry and through the two-pass kernels -------------------------------------------------------
@pytest.mark.parametrize('case', pc.small_cases(), ids=ident)
def test_every_unit_small_chunks(eng, pdict, case):
    from frankenz_amd import BruteForce
    B, variant, M, mode, kind = case
    # M: one model past a tile of the (1, 4) geometry every chunk of n < cu_count * 64 objects takes --
    #   static constexpr int TILE = (NVAL > 32) ? 64 : (NVAL > 16 ? 128 : 256);        (csrc/fz_kernels.h; NVAL = BT, 2 BT in mode A)
    T = pc.tile(pc.unit(B), mode)
    assert M in (1, T + 1)
    N2 = pc.twopass_objects(M)
    pr, pri = pc.problem(B, variant, N2, M, T), pc.prior(kind, B, variant, N2, M, T)
    ref = pc.reference(kind, B, variant, N2, M, T, mode, None)
    idx = np.array(pc.small_idx(M))
    assert len(idx) == pc.SMALL_N and idx[-1] == N2 - 1 and N2 < eng.cu_count() * 64
    # the single-pass kernel: 37 objects, the problem's first 36 and its last
    got = run(pr, pri, mode, pdict, idx)
    assert eng.last_form() == 'k_fused'
    against_oracle('k_fused (1, 4)', got, ref, idx)
    only_k_ex_changes(got, run(pr, pri, mode, pdict, idx, plain=True), pc.K_EX)
    # no room for the candidate lists at 1 MiB: all N2 objects through the two-pass kernels (pc.twopass_objects has the arithmetic)
    before = eng.workspace_limit()
    eng.set_workspace_limit(pc.TWOPASS_LIMIT)
    try:
        got2 = run(pr, pri, mode, pdict)
        form = eng.last_form()
    finally:
        eng.set_workspace_limit(before)
    assert eng.workspace_limit() == before
    assert form == ('k_stats + k_kde' if M > 1 else 'k_fused')          # (a single model's lists always fit)
    against_oracle('k_stats + k_kde', got2, ref, np.arange(N2))
    # the three planes of fit()
    bf = BruteForce(pr['Y'], pr['Ye'], pr['Ym'])
    with np.errstate(all='ignore'):
        bf.fit(pr['X'][idx].copy(), pr['Xe'][idx].copy(), pr['Xm'][idx].copy(), lprob_func=pri.hook(idx), lprob_kwargs=pc.MODES[mode],
               verbose=False)
        lp, lnl, undef = ref['lp'][idx], ref['lnl'][idx], ref['undef'][idx]
        lnprob = lnl + lp
    if kind == 'rows':
        np.testing.assert_array_equal(bf.fit_lnprior, lp)
    else:
        held_ln(bf.fit_lnprior, lp)
    assert not np.isfinite(bf.fit_lnlike[undef]).any() and not np.isfinite(lnl[undef]).any()
    held('fit_lnlike', bf.fit_lnlike, lnl, ~undef, pc.LNL_TOL)
    held('fit_lnprob', bf.fit_lnprob, lnprob, ~undef, pc.LNL_TOL)


# ---- 2: the large-chunk geometries ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', pc.large_cases(), ids=ident)
def test_large_chunk_geometries(eng, pdict, case):
    B, variant, M, mode, kind = case
    # n >= cu_count * 64 (256 compute units): (2, 16) where PhotSrc::PREF_2x16, else (4, 8) (fz_launch_fitpredict), with tiles of
    #   tile_len() { return (NWAVES >= 12 && RW <= 6) ? 1024 : ((NWAVES >= 8 && RW <= 10) ? 512 : TILE); }     (csrc/fz_kernels.h)
    tw, nw, TL = pc.large_geometry(pc.unit(B), mode, variant)
    N = pc.LARGE_N
    assert N >= eng.cu_count() * 64 and N % tw != 0 and M in (TL + 1, 2 * TL)
    pr, pri = pc.problem(B, variant, N, M, TL), pc.prior(kind, B, variant, N, M, TL)
    idx = pc.large_idx(B, variant, M, mode)
    ref = pc.reference(kind, B, variant, N, M, TL, mode, idx)
    got = run(pr, pri, mode, pdict)
    assert eng.last_form() == 'k_fused'
    against_oracle('k_fused (%d, %d)' % (tw, nw), [a[ref['idx']] for a in got], ref, np.arange(len(idx)))
    # every other row: the same call with the objects in another order gives the same bits
    perm = np.random.RandomState(6).permutation(N)
    for a, b in zip(run(pr, pri, mode, pdict, perm), got):
        np.testing.assert_array_equal(a, b[perm])
    only_k_ex_changes(got, run(pr, pri, mode, pdict, plain=True), pc.K_EX)


# ---- 4: the routes that add the prior to materialised rows (k_prior_add) ------------------------------------------------------------
@pytest.mark.parametrize('case', pc.modec_cases(), ids=ident)
def test_mode_c_rows_route(pdict, case):
    B, variant, M, mode, kind = case
    N = pc.SMALL_N
    pr, pri = pc.problem(B, variant, N, M, 64), pc.prior(kind, B, variant, N, M, 64)
    ref = pc.reference(kind, B, variant, N, M, 64, mode, None)
    got = run(pr, pri, mode, pdict)
    against_oracle('mode C', got, ref, np.arange(N))
    only_k_ex_changes(got, run(pr, pri, mode, pdict, plain=True), pc.K_EX)


def test_knn_rows_route_at_twelve_bands(pdict):
    from frankenz_amd import NearestNeighbors
    B, N, M = 12, pc.SMALL_N, 300
    pr, pri = pc.problem(B, 'fast', N, M, 256), pc.prior('rows', B, 'fast', N, M, 256)
    lp = pri.dense(np.arange(N))
    nn = NearestNeighbors(pr['Y'], pr['Ye'], pr['Ym'], K=4, feature_map='identity', rstate=np.random.RandomState(5), verbose=False)
    p, (lm, le) = nn.fit_predict(pr['X'].copy(), pr['Xe'].copy(), pr['Xm'].copy(), pr['z'], pr['ze'], lprob_func=pri.hook(),
                                 rstate=np.random.RandomState(6), k=8, label_dict=pdict, return_gof=True, verbose=False)
    feats = fo.knn_train(pr['Y'], pr['Ye'], 4, 'identity', np.random.RandomState(5))
    q = fo.knn_query_features(pr['X'], pr['Xe'], 'identity', np.random.RandomState(6))
    nt = fo.knn_neighbors_exact(feats, q, 8)
    rp, rlm, rle, rn, rnn, rlnp = fo.knn_fit_predict(pr['X'].copy(), pr['Xe'].copy(), pr['Xm'].copy(), pr['Y'], pr['Ye'], pr['Ym'], nt,
                                                     pr['z'], pr['ze'], label_dict=pc.oracle_dict(), lnprior=lp)
    np.testing.assert_array_equal(nn.neighbors, rn)
    every = np.ones(N, dtype=bool)
    assert np.isfinite(rp).all(axis=1).mean() >= 0.75
    held('k-NN fit_lnprob', nn.fit_lnprob, rlnp, every, dict(rtol=1e-8, atol=1e-8))          # test_knn_prior_other_routes_vs_oracle
    held('k-NN PDFs', p, rp, every, pc.PDF_TOL); held('k-NN lmap', lm, rlm, every, pc.GOF_TOL); held('k-NN levid', le, rle, every, pc.GOF_TOL)
