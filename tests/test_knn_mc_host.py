"""The Monte-Carlo draws of the k-NN fitter on the device, host half (no GPU): the NumPy twin ``knn._philox_normal`` of
csrc/fz_philox.h: philox_normal2 -- counter layout, independence of how a call is sliced, distinct streams per set and per key
domain, the law at the key the GPU tests use --, the per-band resolution of ``fmap_args`` / ``fmap_kwargs``, the layout of
``fz_knn_map``, the argument checks of the new keywords and what the compiler made of the two kernels."""
import ctypes

import numpy as np
import pytest

from frankenz_amd import knn
from frankenz_amd.samplers import _philox4x32

KEY = (0x5EED0001, 0x0BADF00D)          # the key of the law tests here and of tests/test_hip_knn_mc.py


def _u53(a, b):
    return ((int(a) >> 5) * 67108864.0 + (int(b) >> 6)) / 9007199254740992.0


@pytest.mark.parametrize('first,i,band,set_', [(0, 0, 0, 0), (2**32 - 1, 0, 3, 2), (2**32 - 1, 2, 4, 1)])
def test_twin_is_box_muller_of_the_philox_words(first, i, band, set_):
    """counter (row lo, row hi, band >> 1, set), key (k0, k1 ^ 0x6B6E6D63); an even band takes r cos, an odd one r sin"""
    import math
    row = first + i
    ctr = np.array([[row & 0xFFFFFFFF, row >> 32, band >> 1, set_]], dtype=np.uint64)
    w = _philox4x32((KEY[0], KEY[1] ^ 0x6B6E6D63), ctr)[0]
    u1, u2 = 1. - _u53(w[0], w[1]), _u53(w[2], w[3])
    assert 0. < u1 <= 1. and 0. <= u2 < 1.
    r, a = math.sqrt(-2. * math.log(u1)), 6.283185307179586 * u2
    want = r * (math.sin(a) if band & 1 else math.cos(a))
    z = knn._philox_normal(KEY, first, 3, 6, set_)
    assert z.shape == (3, 6) and z.dtype == np.float64
    assert abs(z[i, band] - want) <= 4e-16 * max(1., abs(want))


def test_a_draw_does_not_depend_on_how_the_rows_are_sliced():
    whole = knn._philox_normal(KEY, 0, 300, 5, 0)
    np.testing.assert_array_equal(whole[:130], knn._philox_normal(KEY, 0, 130, 5, 0))
    np.testing.assert_array_equal(whole[130:], knn._philox_normal(KEY, 130, 170, 5, 0))
    # an odd band count drops the last pair's second variate: the first five bands of a six-band draw
    np.testing.assert_array_equal(whole, knn._philox_normal(KEY, 0, 300, 6, 0)[:, :5])
    hi = knn._philox_normal(KEY, 2**32 - 3, 6, 5, 0)
    np.testing.assert_array_equal(hi[3:], knn._philox_normal(KEY, 2**32, 3, 5, 0))


def test_sets_and_the_key_domain_are_distinct_streams():
    z = [knn._philox_normal(KEY, 0, 50, 5, s) for s in (0, 1, 2)]
    for a in range(3):
        for b in range(a + 1, 3):
            assert not np.any(z[a] == z[b])
    # the key xor: the words of the plain key at the same counters give other variates
    ctr = np.array([[i, 0, 0, 0] for i in range(50)], dtype=np.uint64)
    plain, mine = _philox4x32(KEY, ctr), _philox4x32((KEY[0], KEY[1] ^ knn._KNN_KEY_XOR), ctr)
    assert not np.any(plain == mine)
    assert knn._KNN_KEY_XOR == 0x6B6E6D63 and knn._KNN_KEY_XOR != 0x6D775F67


def test_the_law_at_the_test_key():
    """1e5 variates: chi-square over 40 equiprobable bins below its 1 - 1e-6 quantile, mean and variance within 5 standard errors,
    the z0 / z1 bands and set 0 / set 1 uncorrelated within 5 / sqrt(n)"""
    from scipy import stats
    n, F = 20000, 5
    z = knn._philox_normal(KEY, 0, n, F, 0)
    v = z.ravel()
    assert np.all(np.isfinite(v))
    edges = stats.norm.ppf(np.arange(1, 40) / 40.)
    cnt = np.bincount(np.searchsorted(edges, v), minlength=40)
    chi2 = np.sum(np.square(cnt - v.size / 40.) / (v.size / 40.))
    assert chi2 < stats.chi2.ppf(1. - 1e-6, 39), chi2
    assert abs(v.mean()) <= 5. / np.sqrt(v.size)
    assert abs(v.var() - 1.) <= 5. * np.sqrt(2. / v.size)
    for a, b in ((0, 1), (2, 3)):                                   # the two variates of one Philox call
        assert abs(np.corrcoef(z[:, a], z[:, b])[0, 1]) <= 5. / np.sqrt(n)
    z1 = knn._philox_normal(KEY, 0, n, F, 1)
    assert abs(np.corrcoef(v, z1.ravel())[0, 1]) <= 5. / np.sqrt(v.size)


def test_per_band_resolution_of_the_map_arguments():
    sig = np.array([0.9, 0.3, 0.4, 0.8, 3.5])
    zp = 10 ** (0.4 * 23.9)
    one = np.ones(5)
    # luptitude(phot, err, skynoise=1., zeropoints=1., *args, **kwargs)
    s, z = knn._fmap_bands('luptitude', [], dict(skynoise=sig, zeropoints=zp), 5)
    np.testing.assert_array_equal(s, sig); np.testing.assert_array_equal(z, np.full(5, zp))
    s, z = knn._fmap_bands('luptitude', [sig], {}, 5)
    np.testing.assert_array_equal(s, sig); np.testing.assert_array_equal(z, one)
    s, z = knn._fmap_bands('luptitude', [2., sig, 'ignored'], {}, 5)
    np.testing.assert_array_equal(s, 2. * one); np.testing.assert_array_equal(z, sig)
    s, z = knn._fmap_bands('luptitude', [sig], dict(zeropoints=3.), 5)
    np.testing.assert_array_equal(s, sig); np.testing.assert_array_equal(z, 3. * one)
    with pytest.raises(TypeError, match='multiple values'):
        knn._fmap_bands('luptitude', [sig], dict(skynoise=1.), 5)
    # magnitude(phot, err, zeropoints=1., *args, **kwargs): the first positional argument is the zeropoint
    s, z = knn._fmap_bands('magnitude', [sig], dict(skynoise=7.), 5)
    np.testing.assert_array_equal(s, one); np.testing.assert_array_equal(z, sig)
    s, z = knn._fmap_bands('identity', [sig], dict(zeropoints=2.), 5)
    np.testing.assert_array_equal(s, one); np.testing.assert_array_equal(z, one)
    with pytest.raises(ValueError, match='per band'):
        knn._fmap_bands('luptitude', [], dict(skynoise=np.ones(4)), 5)
    with pytest.raises(ValueError, match='per band'):
        knn._fmap_bands('luptitude', [], dict(skynoise=np.ones((3, 5))), 5)
    m = knn._fmap_struct('luptitude', [], dict(skynoise=sig, zeropoints=zp), 5)
    assert m.kind == 2 and list(m.skynoise[:5]) == list(sig) and list(m.zeropoints[:5]) == [zp] * 5
    assert list(m.skynoise[5:]) == [1.] * 27 and list(m.zeropoints[5:]) == [1.] * 27
    assert knn._fmap_struct('identity', [], {}, 3).kind == 0 and knn._fmap_struct('magnitude', [], {}, 32).kind == 1
    with pytest.raises(NotImplementedError):
        knn._fmap_struct('magnitude', [], {}, 33)


def test_layout_of_the_map_struct():
    """fz_knn_map of include/frankenz_hip.h: int32 kind, int32 reserved, double skynoise[32], double zeropoints[32]"""
    from frankenz_amd._lib import ABI, KnnMap
    assert ctypes.sizeof(KnnMap) == 8 + 2 * 32 * 8
    assert (KnnMap.kind.offset, KnnMap.reserved_.offset, KnnMap.skynoise.offset, KnnMap.zeropoints.offset) == (0, 4, 8, 264)
    assert len(ABI['fz_knn_draw_features'][1]) == 10 and len(ABI['fz_knn_draw_trees'][1]) == 10


def test_argument_checks_of_the_new_keywords():
    Y = np.ones((4, 5))
    with pytest.raises(ValueError, match="`feature_draws` must be 'host' or 'device'"):
        knn.NearestNeighbors(Y, Y, Y, K=1, feature_draws='gpu', verbose=False)
    nn = knn.NearestNeighbors(Y, Y, Y, K=1, rstate=np.random.RandomState(0), verbose=False)         # (the default: drawn on the host)
    assert nn.feature_key is None and nn.query_key is None
    X = np.ones((2, 5))
    z, ze, grid = np.zeros(4), np.ones(4), np.linspace(0, 1, 11)
    q = np.zeros((2, 5))
    with pytest.raises(ValueError, match="`query_draws` must be 'host' or 'device'"):
        nn.fit(X, X, X, query_draws='gpu', verbose=False)
    with pytest.raises(ValueError, match="`query_draws` must be 'host' or 'device'"):
        nn.fit_predict(X, X, X, z, ze, label_grid=grid, query_draws=None, verbose=False)
    with pytest.raises(ValueError, match="`query_draws` must be 'host' or 'device'"):
        nn.fit_sample(X, X, X, 3, query_draws='numpy', verbose=False)
    with pytest.raises(ValueError, match="`query_draws` must be 'host' or 'device'"):
        next(nn._fit(X, X, X, query_draws='gpu'))
    with pytest.raises(ValueError, match="`query_draws` must be 'host' or 'device'"):
        next(nn._fit_predict(X, X, X, z, ze, label_grid=grid, query_draws='gpu'))
    with pytest.raises(ValueError, match="exclude each other"):
        nn.fit_predict(X, X, X, z, ze, label_grid=grid, query_features=q, query_draws='device', verbose=False)
    with pytest.raises(ValueError, match="exclude each other"):
        nn.fit_sample(X, X, X, 3, query_features=q, query_draws='device', verbose=False)
    with pytest.raises(ValueError, match="`draws` must be 'host' or 'device'"):
        nn.query_features(X, X, draws='gpu')
    # the host form of the public draw is today's: the stream of rstate.normal
    got = nn.query_features(X, 0.5 * X, rstate=np.random.RandomState(3))
    want = nn._query_features(X, 0.5 * X, np.random.RandomState(3))
    np.testing.assert_array_equal(got, want)
    assert got.shape == (2, 5) and got.dtype == np.float64
    from frankenz_amd import sharded
    with pytest.raises(ValueError, match="`query_draws` must be 'host' or 'device'"):
        sharded.sharded_fit_predict(nn, X, X, X, z, ze, gather=None, label_grid=grid, query_draws='gpu')
    with pytest.raises(ValueError, match="exclude each other"):
        sharded.sharded_fit_predict(nn, X, X, X, z, ze, gather=None, label_grid=grid, query_draws='device', query_features=q)


def test_the_draw_kernels_use_no_scratch():
    """the build's resource report (kept beside the library): the six instantiations of k_knn_mc_features / k_knn_mc_sets are
    streaming kernels without scratch or LDS"""
    import os
    import re
    import __graft_entry__ as ge
    ge.build()
    if not os.path.exists(ge.RESOURCES):
        ge.build(force=True)
    blocks = [b for b in re.split(r'remark: Function Name: ', open(ge.RESOURCES).read())[1:] if 'k_knn_mc_' in b.split(' ', 1)[0]]
    names = sorted(b.split(' ', 1)[0] for b in blocks)
    assert len(names) == 6 and sum('k_knn_mc_features' in n for n in names) == 3 and sum('k_knn_mc_sets' in n for n in names) == 3
    for b in blocks:
        get = lambda key: int(re.search(key + r': (\d+)', b).group(1))
        assert get(r'ScratchSize \[bytes/lane\]') == 0 and get('VGPRs Spill') == 0 and get(r'LDS Size \[bytes/block\]') == 0
        assert get(r'Occupancy \[waves/SIMD\]') >= 4
