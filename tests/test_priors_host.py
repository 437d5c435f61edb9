"""Host side of the magnitude-dependent priors (no GPU): ``frankenz_amd.priors`` against the reference's priors.py (golden g18,
tests/golden/make_golden_bpz.py) and the cell / fraction arithmetic of ``pdf.logprob_prior_lerp``."""
import numpy as np
import pytest

from conftest import load_golden

RTOL = 1e-13          # the reference's own corner sum and this one differ by a few roundings (measured: 4.4e-16)


def same(a, b):
    """rtol = 1e-13 and exact zeros where the reference has zeros"""
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    assert a.shape == b.shape
    np.testing.assert_array_equal(a == 0, b == 0)
    err = np.max(np.abs(a - b) / np.where(b == 0, 1., np.abs(b)))
    print('max relative difference %.3g' % err)
    np.testing.assert_allclose(a, b, rtol=RTOL, atol=0)


def test_pmag_and_raw_prior_match_reference():
    from frankenz_amd import priors
    g = load_golden('g18_bpz_prior')
    same(priors.pmag(g['pmag_mag'], float(g['pmag_maglim'])), g['pmag'])
    same(priors.pmag(g['pmag_mag'], 26.5, mbounds=(12., 29.), alpha=10., beta=1.5, gamma=0.5, Npoints=300), g['pmag_b'])
    for k, m in enumerate(g['raw_m']):                   # scalar magnitude: the reference's shapes
        p, f = priors._bpz_prior(float(m), g['raw_zgrid'])
        assert p.shape == (len(g['raw_zgrid']), 3) and f.shape == (3,)
        same(p, g['raw_p'][k]); same(f, g['raw_f'][k])
    p, f = priors._bpz_prior(g['raw_m'], g['raw_zgrid'])  # ... and all of them at once
    same(p, g['raw_p']); same(f, g['raw_f'])


def test_bpz_functions_and_base_table_match_reference():
    from frankenz_amd import priors
    g = load_golden('g18_bpz_prior')
    z, t, m = g['fn_z'], g['fn_t'], g['fn_m']
    assert (m < 20).any() and (m > 32).any() and (z == 0).any() and (z > 15).any()
    same(priors.bpz_pt_m(t, m), g['bpz_pt_m'])
    same(priors.bpz_pz_tm(z, t, m), g['bpz_pz_tm'])
    for k in (0, 3, 7, 100):                             # one point at a time, the reference's call
        same(priors.bpz_pz_tm(z[k], int(t[k]), m[k]), g['bpz_pz_tm'][k])
        same(priors.bpz_pt_m(int(t[k]), m[k]), g['bpz_pt_m'][k])
    i = g['base_idx']
    same(priors._base_table('pztm')[i[:, 0], i[:, 1], i[:, 2]], g['base_val'])
    i = g['ptm_idx']
    same(priors._base_table('ptm')[i[:, 0], i[:, 1]], g['ptm_val'])
    assert priors._base_table('pztm') is priors._base_table('pztm')            # built once
    # clipping as the reference clips
    zz = np.array([0.3, 1.7, 4.])
    np.testing.assert_array_equal(priors.bpz_pz_tm(zz, 1, 15.), priors.bpz_pz_tm(zz, 1, 20.))
    np.testing.assert_array_equal(priors.bpz_pz_tm(zz, 1, 40.), priors.bpz_pz_tm(zz, 1, 32.))
    np.testing.assert_array_equal(priors.bpz_pz_tm(20., 2, 25.), priors.bpz_pz_tm(15., 2, 25.))
    np.testing.assert_array_equal(priors.bpz_pt_m(0, 15.), priors.bpz_pt_m(0, 20.))


def test_bpz_functions_refuse_what_the_reference_refuses():
    from frankenz_amd import priors
    for bad_t in (-1, 3, np.array([0, 1, 2.5])):
        with pytest.raises(ValueError):
            priors.bpz_pz_tm(1., bad_t, 22.)
        with pytest.raises(ValueError):
            priors.bpz_pt_m(bad_t, 22.)
    with pytest.raises(ValueError):
        priors.bpz_pz_tm(1., 1, np.nan)
    with pytest.raises(ValueError):
        priors.bpz_pz_tm(np.array([0.5, np.nan]), 1, 22.)
    with pytest.raises(ValueError):
        priors.bpz_pt_m(1, np.nan)
    with pytest.raises(ValueError):                       # bounds wider than the table: the interpolator is out of bounds
        priors.bpz_pz_tm(1., 1, 15., mbounds=(10, 32))
    with pytest.raises(ValueError):
        priors.model_cells(np.array([0.5, 1.]), np.array([0, 3]))
    with pytest.raises(ValueError):
        priors.model_cells(np.array([0.5, np.nan]), np.array([0, 1]))


def test_lerp_cells_edges():
    from frankenz_amd.pdf import lerp_cells, logprob_prior_lerp
    grid = np.array([-1., 0., 0.5, 2., 2.25, 7., 11.])
    P = len(grid)
    coord = np.array([-1., 11., -5., 40., 0.5, 2.25, 1.25, np.nextafter(11., 0.), np.inf, -np.inf])
    r, f = lerp_cells(grid, coord)
    assert r.dtype == np.int64 and f.dtype == np.float64
    np.testing.assert_array_equal(r, [0, P - 2, 0, P - 2, 2, 4, 2, P - 2, P - 2, 0])
    np.testing.assert_array_equal(f[:6], [0., 1., 0., 1., 0., 0.])
    assert f[6] == 0.5 and 0. < f[7] < 1. and f[8] == 1. and f[9] == 0.
    assert r.min() >= 0 and r.max() <= P - 2 and f.min() >= 0. and f.max() <= 1.   # row P is never read
    np.testing.assert_allclose(grid[r] + f * (grid[r + 1] - grid[r]), np.clip(coord, grid[0], grid[-1]), rtol=1e-15)
    with pytest.raises(ValueError):
        lerp_cells(grid, np.array([0.5, np.nan]))
    with pytest.raises(ValueError):                       # P = 1
        lerp_cells(np.array([3.]), np.array([3.]))
    with pytest.raises(ValueError):
        lerp_cells(np.array([0., 1., 1., 2.]), np.array([0.5]))
    with pytest.raises(ValueError):
        logprob_prior_lerp(np.ones((1, 4)), np.array([3.]), np.array([3.]))
    with pytest.raises(ValueError):
        logprob_prior_lerp(np.ones((3, 4)), np.array([0., 1., 2.]), np.array([0.5, np.nan]))
    with pytest.raises(ValueError):                       # grid and table disagree
        logprob_prior_lerp(np.ones((3, 4)), np.array([0., 1.]), np.array([0.5]))
    hook = logprob_prior_lerp(np.ones((P, 4)), grid, coord)
    tab, p, rr, ff = hook.chunk(2, 5, len(coord))
    assert p == P and tab.shape == (P, 4)
    np.testing.assert_array_equal(rr, r[2:5]); np.testing.assert_array_equal(ff, f[2:5])
    with pytest.raises(ValueError):
        hook.chunk(0, 3, len(coord) + 1)
