"""k_hist<screen> deals the objects of a launch to its waves in the order of their expected settle cost (csrc/fz_hist_order.h).
The order is a scheduling matter only: an object's pass over the models is the same instruction stream on whichever wave it runs,
so every output must equal the FZ_HIST_ORDER=0 run BIT FOR BIT -- and a wrong permutation (a slot dealt twice, a slot never dealt)
shows as a row that was not written.  Sizes follow the launch geometry: R = 16 waves x CUs objects make one round, and the order is
built only for launches of more than one round."""
import numpy as np
import pytest

import frankenz_oracle as fo
from conftest import EVID64, SDSS_SIGMA

pytestmark = pytest.mark.gpu
MODES = {'A': {}, 'Ai': {'ignore_model_err': True}}
_cache = {}


def engine():
    from frankenz_amd.engine import get_engine
    return get_engine()


def dicts():
    if 'dicts' not in _cache:
        from frankenz_amd import PDFDict
        grid, sg = np.arange(0, 7 + 1e-5, .01), np.linspace(.005, 2, 500)
        _cache['dicts'] = (PDFDict(grid, sg), fo.KernelDict(grid, sg))
    return _cache['dicts']


def problem(N, M, seed, model_err='const', obj_mask=0.0, special=True):
    """heterogeneous objects: a third at 0.05 x the SDSS noise, a third at 1 x, a third at 10 x, interleaved; with `special` a few
    training-set self matches, one object nothing fits and a run of 64 identical objects"""
    rs = np.random.RandomState(seed)
    B = 5
    Y = rs.lognormal(1., 1., size=(M, B))
    Ye = np.tile(SDSS_SIGMA, (M, 1)) if model_err == 'const' else SDSS_SIGMA * rs.uniform(0.5, 1.5, size=(M, B))
    Ym = np.ones((M, B))
    scale = np.array([0.05, 1., 10.])[np.arange(N) % 3][:, None]
    X = Y[rs.randint(0, M, N)] + scale * SDSS_SIGMA * rs.standard_normal((N, B))
    Xe = scale * np.tile(SDSS_SIGMA, (N, 1))
    Xm = np.ones((N, B))
    sp = {}
    if special and N >= 200:
        sp['self'] = np.array([3, 4, 5, N // 2, N - 1])
        X[sp['self']] = Y[[0, 1, M // 2, M - 1, 7 % M]]
        sp['misfit'] = np.array([11])
        X[11] = 1e6 + Y[0]
        sp['same'] = np.arange(100, 164)
        X[100:164] = X[100]; Xe[100:164] = Xe[100]
    if obj_mask > 0:
        Xm = (rs.uniform(size=(N, B)) >= obj_mask).astype(float)
        Xm[Xm.sum(axis=1) < 3] = 1.0
        X[Xm == 0] = -7e5                                         # garbage in the unobserved bands must not matter
    z = rs.uniform(0, 6, M); ze = np.full(M, 0.05)
    return dict(Y=Y, Ye=Ye, Ym=Ym, X=X, Xe=Xe, Xm=Xm, z=z, ze=ze, sp=sp)


def run(pr, kw, monkeypatch, env=()):
    """one fit_predict into NaN-filled device buffers: (pdfs, ln-max, ln-evidence, kernel form, fused launches)"""
    from frankenz_amd.engine import DeviceArray, kde_opts, like_opts
    eng = engine()
    pd, _ = dicts()
    for k, v in env:
        monkeypatch.setenv(k, v)
    try:
        eng.upload_models(pr['Y'], pr['Ye'], pr['Ym'])
        G = eng.set_labels(pr['z'], pr['ze'], label_dict=pd)
        N = len(pr['X'])
        out = [DeviceArray(eng, (N, G)), DeviceArray(eng, (N, 1)), DeviceArray(eng, (N, 1))]
        for a in out:
            a.set_rows(0, np.full(a.shape, np.nan))
        eng.timing_reset()
        eng.fit_predict_prior(pr['X'].copy(), pr['Xe'].copy(), pr['Xm'].copy(), like_opts(kw), kde_opts({}), None, out[0], out[1], out[2], n=N)
        eng.sync()
        return out[0].numpy(), out[1].numpy()[:, 0], out[2].numpy()[:, 0], eng.last_form(), eng.timing()['n_fused']
    finally:
        for k, _ in env:
            monkeypatch.delenv(k)


def same_bits(a, b):
    """equal as bit patterns up to the payload of a nan: the same nans and nowhere else, every other entry array_equal"""
    assert a.shape == b.shape
    na, nb = np.isnan(a), np.isnan(b)
    assert np.array_equal(na, nb)
    assert np.array_equal(a[~na].view(np.int64), b[~nb].view(np.int64))


def on_off(pr, kw, monkeypatch, env=(), form='k_hist<screen>', launches=1, rows=None):
    """the default against FZ_HIST_ORDER=0: bit equality, every row written, same form, same number of fused launches"""
    off = run(pr, kw, monkeypatch, tuple(env) + (('FZ_HIST_ORDER', '0'),))
    on = run(pr, kw, monkeypatch, tuple(env))
    assert on[3] == off[3] and on[4] == off[4] == launches
    if form is not None:
        assert on[3] == form
    sl = slice(None) if rows is None else rows
    for a, b in zip(on[:3], off[:3]):
        same_bits(a[sl], b[sl])
    # written: ln-evidence and ln-max of every object are numbers (-inf allowed), and a PDF row is all numbers or all nan
    assert not np.isnan(on[2][sl]).any() and not np.isnan(on[1][sl]).any()
    nanrow = np.isnan(on[0][sl])
    assert (nanrow.all(axis=1) | ~nanrow.any(axis=1)).all() and nanrow.all(axis=1).mean() < 0.01
    return on, off


def R():
    return 16 * engine().cu_count()


@pytest.mark.parametrize('mode', ['A', 'Ai'])
def test_bit_equality_on_off(mode, monkeypatch):
    """n = 2 R + 37 objects (three rounds, the last one partial) against 1000 models (three 384-model tiles, the last one partial)"""
    pr = problem(2 * R() + 37, 1000, 41)
    on, off = on_off(pr, MODES[mode], monkeypatch)
    _cache[('first', mode)] = (pr, on)
    assert np.isfinite(on[0]).all()
    # the run of identical objects: identical rows
    s = pr['sp']['same']
    for a in on[:3]:
        assert (a[s] == a[s[0]]).all()


def test_oracle(monkeypatch):
    """40 objects of the first case (the special ones among them) against the oracle: both runs wrong together would pass the comparison"""
    if ('first', 'A') not in _cache:
        pr = problem(2 * R() + 37, 1000, 41)
        _cache[('first', 'A')] = (pr, run(pr, {}, monkeypatch))
    pr, on = _cache[('first', 'A')]
    sp = pr['sp']
    N = len(pr['X'])
    first = list(sp['self']) + list(sp['misfit']) + list(sp['same'][:4]) + list(range(0, N, N // 50))
    idx = np.sort(np.array(list(dict.fromkeys(int(i) for i in first))[:40]))
    assert len(idx) == 40
    _, od = dicts()
    with np.errstate(all='ignore'):
        rp, rlm, rle = fo.bruteforce_fit_predict(pr['X'][idx].copy(), pr['Xe'][idx].copy(), pr['Xm'][idx].copy(), pr['Y'], pr['Ye'], pr['Ym'],
                                                 pr['z'], pr['ze'], label_dict=od)
    np.testing.assert_allclose(on[0][idx], rp, rtol=1e-7, atol=1e-13)
    np.testing.assert_allclose(on[1][idx], rlm, rtol=1e-9)
    np.testing.assert_allclose(on[2][idx], rle, **EVID64)


def test_per_object_band_counts(monkeypatch):
    """the OBJK form: 10 % of the object bands unobserved against unmasked models"""
    pr = problem(2 * R() + 37, 1000, 42, obj_mask=0.10)
    on_off(pr, MODES['Ai'], monkeypatch, form='k_hist<screen> (per-object band counts)')


def test_split_launch_object_map_under_the_order(monkeypatch):
    """an object map UNDER the order: objects with unobserved bands against per-model errors with FZ_HIST_SEG=0 -- the segmented form
    declines, the form with per-object band counts is not compiled for per-model errors, so the chunk is split and its fully observed
    objects (~80 % here: more than two rounds) run k_hist<screen> through a map, the others the masked kernel (two fused launches; the
    form reported is the second one's).  The mapped rows are compared bit for bit, the others to rounding."""
    pr = problem(3 * R() + 37, 1000, 43, model_err='varying', obj_mask=0.04)
    full = pr['Xm'].all(axis=1)
    assert full.sum() > 2 * R() and (~full).sum() > 0
    env = (('FZ_HIST_SEG', '0'),)
    on, off = on_off(pr, {}, monkeypatch, env=env, form=None, launches=2, rows=full)
    assert 'segmented' not in on[3]
    with np.errstate(all='ignore'):
        for a, b in zip(on[:3], off[:3]):
            np.testing.assert_allclose(a[~full], b[~full], rtol=1e-12, atol=1e-300, equal_nan=True)
    assert not np.isnan(on[2][~full]).any()


@pytest.mark.parametrize('case', ['n=1', 'n=R', 'n=R+1', 'n=3R, stride > M', 'M=65'])
def test_boundaries(case, monkeypatch):
    r = R()
    n, M, env = {'n=1': (1, 1000, ()), 'n=R': (r, 1000, ()), 'n=R+1': (r + 1, 1000, ()),
                 'n=3R, stride > M': (3 * r, 1000, (('FZ_HIST_ORDER_STRIDE', '5000'),)),
                 'M=65': (2 * r + 37, 65, ())}[case]
    pr = problem(n, M, 44 + n % 7 + M % 5)
    on_off(pr, {}, monkeypatch, env=env)


def test_launch_accounting(monkeypatch):
    """the cost pass and the sort sit inside the main launch's timer: one fused launch per call with the switch on or off, and the
    form reported does not change"""
    pr = problem(R() + 1, 1000, 45)
    on = run(pr, {}, monkeypatch)
    off = run(pr, {}, monkeypatch, (('FZ_HIST_ORDER', '0'),))
    assert on[3] == off[3] == 'k_hist<screen>'
    assert on[4] == off[4] == 1
