"""What k_hist's finish does in front of the PDF row (docs/k_hist.md, "In front of the PDF row"): the ambiguous band -- the pairs whose
weight lies within a thousandth of the stacking threshold times the best weight, which wait in a per-object list in global memory
until the exact maximum and evidence are known.  The acquire in front of the list's loads has workgroup scope (FZ_HIST_BAND_ACQ); the
band with several entries per lane and trip (FZ_HIST_BAND) and the three wave reductions advancing together (FZ_HIST_RED3) are in
the source and compiled out.  None changes an operation, an operand or an order, so the expectation is what the kernel gave BEFORE, bit for
bit: tests/golden/hist_band_*.npz were recorded from a release build of the commit in front of it (tools/record_hist_band.py writes
them from `problem` below).

The point is a list whose LENGTH is known by construction.  With band-constant errors and the dimensionality prior a pair's weight
relative to the mode is w(c) = (c / k)^(k/2) exp(-(c - k) / 2) of its chi2 c, k = bands - 2.  At 5 bands w = 1e-3 at c0 = 22.915056 and
the band (0.999e-3, 1.001e-3] is chi2 in [22.9128, 22.9174).  A model at chi2 = d^2 from the object: the object's flux displaced in ONE
band by d sqrt(xe^2 + ye^2).
  models 0..383  the whole first tile at chi2 = k: weight 1, all stacked, and the bar at its final place before anything else is seen
  n models       chi2 spread over [22.9135, 22.9168]: they straddle c0, none within 1e-4 of it (some stacked by the strict rule, some
                 not), weights pairwise distinct, labels on only THREE grid points -- many adds meet in one bin, and a changed order
                 of the adds shows in the last bit
  fillers        chi2 50.2-80: they pass the screen, their weight is at most 4e-9, far under the bar
  n = 0, 1, 63, 64, 65, 64 T - 1, 64 T, 64 T + 1, 3 x 64 T + 37 for T = 4 entries per lane and trip; the n models right behind the first
  tile (`front`), at the very end of the set (`end`: they reach the list through the finish's own last drains) and interleaved with
  the fillers (`mixed`); one case not normalised and one at 4 bands (k = 2: c0 solved from the same formula).  `rounds` has more objects
  than one round of the launch holds (2 R + 37, R = 16 waves x CUs; replicas of the 32): a wave then reads its list's memory again
  one round later with another object's entries in it, which is what the fences in front of the band's loads are there for.
32 objects: 16 copies of the constructed one on the even slots (every second wave of two blocks) and 16 ordinary ones of
tests/test_hip_hist_lean.py's kind (0.05 / 1 / 10 x the SDSS noise around models of the set).  Asserted: the kernel form; ln-max,
ln-evidence and the kept PDF rows equal to the fixture bit for bit; the 16 copies identical; every object against the oracle at the
tolerances of tests/test_hip_hist_ahead.py; and, on the CPU from the oracle's ln-likes of the constructed object, that exactly n
models have a weight relative to the best in (0.999e-3, 1.001e-3] and no other model one in (1e-6, 2e-3) -- a fixture could not
otherwise pass with a different list than intended."""
import os

import numpy as np
import pytest

import frankenz_oracle as fo
from conftest import EVID64, SDSS_SIGMA
from test_hip_hist_lean import engine, same_bits

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
T = 4                                                              # entries per lane and trip (FZ_HIST_BAND_T)
TILE, NFILL, N = 384, 600, 32
COPIES, ORDINARY = np.arange(0, N, 2), np.arange(1, N, 2)
KEEP = np.r_[0, 30, ORDINARY[:6]]                                  # the PDF rows a fixture holds: two copies, six ordinary objects
SPREAD5 = (22.9135, 22.9168)
# name: (n, placement, bands, normalize, seed)
CASES = {}
for _k, _n in enumerate([0, 1, 63, 64, 65, 64 * T - 1, 64 * T, 64 * T + 1, 3 * 64 * T + 37]):
    CASES['n%d_front' % _n] = (_n, 'front', 5, True, 400 + _k)
for _k, _n in enumerate([1, 65, 64 * T + 1, 3 * 64 * T + 37]):
    CASES['n%d_end' % _n] = (_n, 'end', 5, True, 420 + _k)
    CASES['n%d_mixed' % _n] = (_n, 'mixed', 5, True, 440 + _k)
CASES['n%d_mixed_raw' % (64 * T + 1)] = (64 * T + 1, 'mixed', 5, False, 460)
CASES['n%d_mixed_b4' % (64 * T + 1)] = (64 * T + 1, 'mixed', 4, True, 461)
CASES['rounds'] = (64 * T + 1, 'mixed', 5, True, 462)
_cache = {}


def fixture_path(name):
    return os.path.join(GOLDEN, 'hist_band_%s.npz' % name)


def dicts():
    """a short grid (101 points) so that a fixture's rows are a few KB; one kernel width in force (every label error is 0.05)"""
    if 'dicts' not in _cache:
        from frankenz_amd import PDFDict
        grid, sg = np.arange(0, 2 + 1e-5, .02), np.linspace(.005, 2, 500)
        _cache['dicts'] = (PDFDict(grid, sg), fo.KernelDict(grid, sg))
    return _cache['dicts']


def rel_weight(c, k):
    """w(c) = (c / k)^(k/2) exp(-(c - k) / 2): a pair's weight relative to the mode's"""
    return (c / k) ** (0.5 * k) * np.exp(-0.5 * (c - k))


def band_chi2(k):
    """(c0, lo, hi): w(c0) = 1e-3 on the far side of the mode, by Newton on ln w; and the interval the n models are spread over --
    the stated one at 5 bands, at 4 bands the same shares of the band's width (w between 1.00068e-3 and 0.99924e-3)"""
    c = 20.
    for _ in range(60):
        c -= (0.5 * k * np.log(c / k) - 0.5 * (c - k) - np.log(1e-3)) / (0.5 * k / c - 0.5)
    if k == 3:
        assert abs(c - 22.915056) < 1e-6
        return c, SPREAD5[0], SPREAD5[1]
    s = 0.5 * k / c - 0.5                                          # d ln w / d chi2 < 0
    return c, c + 0.68e-3 / s, c - 0.76e-3 / s


def spread(n, k):
    """n distinct chi2 over [lo, hi] in two runs, one on either side of c0 and none within 2e-4 of it"""
    c0, lo, hi = band_chi2(k)
    nlo = (n + 1) // 2
    return np.r_[np.linspace(lo, c0 - 2e-4, nlo), np.linspace(c0 + 2e-4, hi, n - nlo)]


def problem(name, nobj=None):
    n, place, B, normalize, seed = CASES[name]
    rs = np.random.RandomState(seed)
    k = B - 2
    sig = np.resize(SDSS_SIGMA, B)
    x0 = np.array([3., 5., 7., 9., 11.])[:B]
    # chi2 of every model from the constructed object, in the order of the set
    cband, cfill = spread(n, k), rs.uniform(50.2, 80., NFILL)
    if place == 'front':
        rest, isband = np.r_[cband, cfill], np.r_[np.ones(n, bool), np.zeros(NFILL, bool)]
    elif place == 'end':
        rest, isband = np.r_[cfill, cband], np.r_[np.zeros(NFILL, bool), np.ones(n, bool)]
    else:
        isband = np.zeros(n + NFILL, bool)
        isband[np.sort(rs.choice(n + NFILL, n, replace=False))] = True
        rest = np.empty(n + NFILL)
        rest[isband], rest[~isband] = cband, cfill
    chi2 = np.r_[np.full(TILE, float(k)), rest]
    isband = np.r_[np.zeros(TILE, bool), isband]
    M = len(chi2)
    Ye = np.tile(sig, (M, 1))
    Ym = np.ones((M, B))
    Y = np.tile(x0, (M, 1))
    b = np.arange(M) % B                                           # the displaced band
    Y[np.arange(M), b] += np.sqrt(chi2) * np.sqrt(2.) * sig[b]     # xe = ye = sig: sqrt(xe^2 + ye^2) = sqrt(2) sig
    pd, _ = dicts()
    z = rs.uniform(0.2, 1.8, M)
    z[isband] = pd.grid[np.array([30, 31, 60])[np.arange(n) % 3]]  # the n models' labels: three grid points
    ze = np.full(M, 0.05)
    # the objects: copies of the constructed one on the even slots, ordinary ones on the odd slots
    scale = np.array([0.05, 1., 10.])[np.arange(N) % 3][:, None]
    X = Y[rs.randint(0, M, N)] + scale * sig * rs.standard_normal((N, B))
    Xe = scale * np.tile(sig, (N, 1))
    X[COPIES], Xe[COPIES] = x0, sig
    Xm = np.ones((N, B))
    if name == 'rounds':
        # more objects than one round of the launch holds: object i is a replica of object i mod 32, so a wave reads its list's
        # memory again in the next round, with another object's entries in it
        if nobj is None:
            nobj = int(np.load(fixture_path(name))['N'])
        rep = np.arange(nobj) % N
        X, Xe, Xm = X[rep], Xe[rep], Xm[rep]
    return dict(Y=Y, Ye=Ye, Ym=Ym, X=X, Xe=Xe, Xm=Xm, z=z, ze=ze, n=n, k=k, isband=isband, normalize=normalize)


def run(pr):
    """one fit_predict into NaN-filled device buffers: every PDF row, ln-max, ln-evidence, the kernel form"""
    from frankenz_amd.engine import DeviceArray, kde_opts, like_opts
    eng = engine()
    pd, _ = dicts()
    eng.upload_models(pr['Y'], pr['Ye'], pr['Ym'])
    G = eng.set_labels(pr['z'], pr['ze'], label_dict=pd)
    N = len(pr['X'])
    out = [DeviceArray(eng, (N, G)), DeviceArray(eng, (N, 1)), DeviceArray(eng, (N, 1))]
    for a in out:
        a.set_rows(0, np.full(a.shape, np.nan))
    eng.fit_predict_prior(pr['X'].copy(), pr['Xe'].copy(), pr['Xm'].copy(), like_opts({}), kde_opts({}, normalize=pr['normalize']), None,
                          out[0], out[1], out[2], n=N)
    eng.sync()
    return dict(pdfs=out[0].numpy(), lmap=out[1].numpy()[:, 0], levid=out[2].numpy()[:, 0], form=eng.last_form())


def check_list_length(pr):
    """the list is the intended one: from the oracle's ln-likes of the constructed object"""
    lnl, _, _ = fo.lnlike_fixed(pr['X'][0], pr['Xe'][0], pr['Xm'][0], pr['Y'], pr['Ye'], pr['Ym'])
    w = np.exp(lnl - lnl.max())
    inband = (w > 0.999e-3) & (w <= 1.001e-3)
    assert inband.sum() == pr['n'] and np.array_equal(inband, pr['isband'])
    assert not ((w > 1e-6) & (w < 2e-3) & ~inband).any()
    assert len(np.unique(w[inband])) == pr['n']                    # pairwise distinct
    if pr['n'] > 1:
        assert (w[inband] > 1e-3).any() and (w[inband] <= 1e-3).any()      # some stacked by the strict rule, some not
    c0 = band_chi2(pr['k'])[0]
    assert abs(rel_weight(c0, pr['k']) - 1e-3) < 1e-12


@pytest.mark.parametrize('name', list(CASES))
def test_bits_of_the_parent(name):
    want = np.load(fixture_path(name))
    pr = problem(name)
    check_list_length(pr)
    got = run(pr)
    print(name, 'M', len(pr['Y']), 'form', got['form'])
    assert got['form'] == str(want['form']) == 'k_hist<screen>'
    if name == 'rounds':
        assert len(pr['X']) > 16 * engine().cu_count()             # more than one round
        # every replica has the bits of its original, whichever wave and round it fell to
        for key in ('lmap', 'levid', 'pdfs'):
            assert np.array_equal(got[key], got[key][np.arange(len(pr['X'])) % N], equal_nan=True), key
        pr = {k: (v[:N] if k in ('X', 'Xe', 'Xm') else v) for k, v in pr.items()}
        got = {k: (v if k == 'form' else v[:N]) for k, v in got.items()}
    for key, g in (('lmap', got['lmap']), ('levid', got['levid']), ('pdfs', got['pdfs'][KEEP])):
        assert np.array_equal(g, want[key], equal_nan=True), key
        same_bits(g, want[key])
    assert not np.isnan(got['lmap']).any() and not np.isnan(got['levid']).any() and not np.isnan(got['pdfs']).any()
    # the 16 copies: identical, whichever wave they fell to
    for key in ('lmap', 'levid', 'pdfs'):
        assert (got[key][COPIES] == got[key][0]).all(), key
    # every object against the oracle
    with np.errstate(all='ignore'):
        rp, rlm, rle = fo.bruteforce_fit_predict(pr['X'].copy(), pr['Xe'].copy(), pr['Xm'].copy(), pr['Y'], pr['Ye'], pr['Ym'],
                                                 pr['z'], pr['ze'], label_dict=dicts()[1])
    p = got['pdfs']
    if not pr['normalize']:
        tot = p.sum(axis=1, keepdims=True)
        assert (tot <= 1. + 1e-12).all() and (tot > 0.5).all()     # the stacked share of the evidence
        p = p / tot
    np.testing.assert_allclose(p, rp, rtol=1e-7, atol=1e-13)
    np.testing.assert_allclose(got['lmap'], rlm, rtol=1e-9)
    np.testing.assert_allclose(got['levid'], rle, **EVID64)
