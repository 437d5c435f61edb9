"""The four network-inference kernels of fz_net.h (k_net_select, k_net_table, k_net_gather, k_net_stack) called directly through the
engine and held to tests/_net_ref.py (plain NumPy, longdouble sums): rows longer than one 64-column chunk, ties across chunk edges,
-inf runs, the 2 560 / 2 561 node switch of the block size and the 4 096 node limit, special rows, host and device arguments."""
import functools

import numpy as np
import pytest

import _net_ref as nr
from conftest import DevArray

pytestmark = pytest.mark.gpu

N = 9                                                    # three blocks of four waves (the last with one live wave), five of two
NN = [1, 2, 63, 64, 65, 127, 128, 129, 257, 1000, 2560, 2561, 4096]
WT = [1e-3, 0.5, 1.0, 0.0, -np.inf]                      # 1.0: strict > against the max, nothing; 0: ln 0; -inf: Network's "no threshold"
CDF = [0.5, 0.05, 2e-4]
GAP = 1e-9                                               # the CDF rule is compared only where no cdf lies this close to the limit
worst = {'select levid': 0.0, 'stack levid': 0.0, 'stack pdf': 0.0}


def eng():
    from frankenz_amd.engine import get_engine
    return get_engine(None)


def levid_bound(ref):
    """fz_fastmath.h: exp_neg 4e-16 + 3.4e-17 |x| relative, weighted by e^x; a lane-strided sum and a 6-level tree of at most 4 096
    non-negative terms, at most 70 ulp = 8e-15; log_pos 4e-16 + 2e-16 |log|; one rounding of the final add"""
    return 2e-14 + 4e-16 * np.abs(ref)


def check_levid(got, ref, key):
    ref64 = np.asarray(ref, dtype=np.float64)
    fin = np.isfinite(ref64)
    np.testing.assert_array_equal(got[~fin], ref64[~fin])
    dev = np.abs(got[fin].astype(nr.LD) - np.asarray(ref)[fin]).astype(np.float64)
    if dev.size:
        worst[key] = max(worst[key], float(np.max(dev / levid_bound(ref64[fin]))))
        print('%s: worst |dev| %.3g, %.3g of the bound (worst so far %.3g)' % (key, dev.max(), np.max(dev / levid_bound(ref64[fin])),
                                                                              worst[key]))
        assert np.all(dev <= levid_bound(ref64[fin]))


@functools.lru_cache(maxsize=None)
def case(Nn):
    """the rows of one shape, their node map and lists"""
    rs = np.random.RandomState(1000 + Nn)
    lp = rs.normal(0, 3, size=(N, Nn)) - rs.uniform(0, 50, size=(N, 1))
    if Nn > 70:
        lp[3, 50:50 + min(40, Nn // 3)] = -np.inf        # a run of -inf across a chunk edge
        lp[5, ::7] = lp[5, 0]                            # one value at a stride of 7: ties in every chunk
    Nnodes = Nn + 5
    match = rs.permutation(Nnodes)[:Nn].astype(np.int32)
    lens = rs.randint(0, 4, size=Nnodes)
    lens[rs.rand(Nnodes) < 0.3] = 0
    off = np.zeros(Nnodes + 1, dtype=np.int64); np.cumsum(lens, out=off[1:])
    for a in (lp, match, off):
        a.setflags(write=False)
    return lp, match, off


def reference(lp, match, off, use_wt, wt, cdf):
    sels, gaps = zip(*[nr.select(r, use_wt, wt, cdf) for r in lp])
    st = [nr.stats(r, s) for r, s in zip(lp, sels)]
    return dict(sel=sels, gap=np.array(gaps), nsel=np.array([len(s) for s in sels]), lmap=np.array([s[0] for s in st]),
                levid=np.array([s[1] for s in st], dtype=nr.LD), rawlen=np.array([nr.rawlen(s, match, off) for s in sels]))


def run_select(lp, match, off, use_wt, wt, cdf, device=False):
    e = eng()
    n, nn = lp.shape
    if device:
        nsel, sel = e.device_empty(n, np.int32), e.device_array(np.zeros((n, nn), dtype=np.int32))
        rawlen, lmap, levid = e.device_empty(n, np.int64), e.device_empty(n), e.device_empty(n)
        e.net_select(DevArray(lp), use_wt, wt, cdf, e.device_array(match), DevArray(off), nsel, sel, rawlen, lmap, levid)
        return [a.numpy() for a in (nsel, sel, rawlen, lmap, levid)]
    nsel = np.full(n, -1, dtype=np.int32); sel = np.zeros((n, nn), dtype=np.int32)
    rawlen = np.full(n, -1, dtype=np.int64); lmap = np.full(n, 7.); levid = np.full(n, 7.)
    e.net_select(np.ascontiguousarray(lp), use_wt, wt, cdf, match, off, nsel, sel, rawlen, lmap, levid)
    return nsel, sel, rawlen, lmap, levid


def check_select(lp, match, off, use_wt, wt, cdf, device=False):
    ref = reference(lp, match, off, use_wt, wt, cdf)
    if not use_wt:
        assert np.all(ref['gap'] > GAP), 'a cdf within %g of the limit: %r' % (GAP, ref['gap'])      # every row, none left out
    got = run_select(lp, match, off, use_wt, wt, cdf, device)
    nsel, sel, rawlen, lmap, levid = got
    np.testing.assert_array_equal(nsel, ref['nsel'])
    for i, s in enumerate(ref['sel']):
        np.testing.assert_array_equal(sel[i, :len(s)], s)
    np.testing.assert_array_equal(rawlen, ref['rawlen'])
    np.testing.assert_array_equal(lmap, ref['lmap'])                                                  # a max: bit for bit
    check_levid(levid, ref['levid'], 'select levid')
    return ref, got


@pytest.mark.parametrize('Nn', NN)
@pytest.mark.parametrize('rule', ['wt', 'cdf'])
def test_select_against_the_longdouble_reference(rule, Nn):
    lp, match, off = case(Nn)
    for thr in (WT if rule == 'wt' else CDF):
        use_wt = rule == 'wt'
        ref, _ = check_select(lp, match, off, use_wt, thr if use_wt else 0.0, 0.5 if use_wt else thr)
        if use_wt and thr == 1.0:
            assert not ref['nsel'].any()
        if use_wt and thr == -np.inf:
            assert np.all(ref['nsel'] == Nn)            # the deviation of docs/deviations.md: numpy's ln(-inf) = nan selects nothing
        if use_wt and thr == 0.0 and Nn > 70:
            assert ref['nsel'][3] == Nn - min(40, Nn // 3)                                             # ln 0 = -inf, strict >: -inf entries go
        if not use_wt and Nn == 1:
            assert not ref['nsel'].any() and np.all(ref['levid'] == -np.inf)                          # one node holds all the probability


@pytest.mark.parametrize('Nn', [129, 2561])
@pytest.mark.parametrize('rule', ['wt', 'cdf'])
def test_select_with_device_resident_arguments_gives_equal_bits(rule, Nn):
    lp, match, off = case(Nn)
    args = (lp, match, off, rule == 'wt', 1e-3, 0.05)
    _, host = check_select(*args)
    _, dev = check_select(*args, device=True)
    for h, d, ns in zip(host, dev, [None, host[0], None, None, None]):
        if ns is None:
            np.testing.assert_array_equal(h.view(np.int64) if h.dtype == np.float64 else h, d.view(np.int64) if d.dtype == np.float64 else d)
        else:
            for i, k in enumerate(ns):
                np.testing.assert_array_equal(h[i, :k], d[i, :k])


def special_rows(Nn):
    rs = np.random.RandomState(77)
    lp = rs.normal(0, 3, size=(N, Nn)) - rs.uniform(0, 50, size=(N, 1))
    lp[0, Nn // 2] = np.nan
    lp[1, [3, Nn - 2]] = np.inf                          # +inf, twice
    lp[2] = -np.inf
    lp[3] = -1000.; lp[3, 70 % Nn] = 0.                  # one dominant node: the CDF rule keeps all the others
    lp[4, 5:] = -np.inf                                  # five live entries
    lp[6, -1] = np.nan
    lp[7, 0] = np.inf; lp[7, 1:] = -np.inf
    Nnodes = Nn + 5
    match = rs.permutation(Nnodes)[:Nn].astype(np.int32)
    off = np.zeros(Nnodes + 1, dtype=np.int64); np.cumsum(rs.randint(0, 3, size=Nnodes), out=off[1:])
    return lp, match, off


@pytest.mark.parametrize('Nn', [130, 2600])
@pytest.mark.parametrize('rule', [('wt', 1e-3), ('wt', 0.0), ('wt', -np.inf), ('cdf', 0.05), ('cdf', 0.5)])
def test_select_special_rows_follow_numpy(rule, Nn):
    lp, match, off = special_rows(Nn)
    use_wt = rule[0] == 'wt'
    ref, _ = check_select(lp, match, off, use_wt, rule[1] if use_wt else 0.0, 0.5 if use_wt else rule[1])
    assert ref['nsel'][0] == 0 and ref['nsel'][6] == 0                                                # a nan: nothing, under every rule
    if not use_wt:
        assert ref['nsel'][1] == Nn - 2 and ref['nsel'][2] == 0 and ref['nsel'][3] == Nn - 1 and ref['nsel'][7] == Nn - 1
        assert ref['lmap'][2] == -np.inf and ref['levid'][2] == -np.inf
    elif rule[1] >= 0:
        assert ref['nsel'][1] == 0 and ref['nsel'][2] == 0 and ref['nsel'][7] == 0 and ref['nsel'][3] == (1 if rule[1] > 0 else Nn)
    else:
        assert ref['nsel'][1] == Nn and ref['nsel'][2] == Nn and ref['levid'][1] == np.inf and ref['levid'][2] == -np.inf


def test_select_refuses_more_than_4096_nodes_with_the_limit_in_the_message():
    e = eng()
    lp = np.zeros((2, 4097))
    with pytest.raises(NotImplementedError, match=r'4097 nodes.*limit.*4096'):
        e.net_select(lp, True, 1e-3, 0.5, None, None, np.zeros(2, dtype=np.int32), np.zeros((2, 4097), dtype=np.int32))


# ---- k_net_table -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def table_case():
    """9 objects on 40 columns of a 50-node network; lists of up to 200 models (the lane stride wraps), a third of them empty;
    selections from the reference's CDF rule (not in index order); objects 1 and 4 start with an empty list; object 7 selects nothing"""
    rs = np.random.RandomState(31)
    Nn, Nnodes = 40, 50
    lp = rs.normal(0, 3, size=(N, Nn))
    lp[7, 11] = np.nan
    sels = [nr.select(r, False, 0.0, 0.3)[0] for r in lp]
    match = rs.permutation(Nnodes)[:Nn].astype(np.int32)
    lens = rs.randint(1, 201, size=Nnodes)
    lens[rs.rand(Nnodes) < 0.33] = 0
    lens[match[sels[1][0]]] = 0; lens[match[sels[4][0]]] = 0
    lens[match[sels[1][1]]] = 130; lens[match[sels[2][0]]] = 67
    off = np.zeros(Nnodes + 1, dtype=np.int64); np.cumsum(lens, out=off[1:])
    items = rs.randint(0, 10**6, size=off[-1]).astype(np.int64)
    nsel = np.array([len(s) for s in sels], dtype=np.int32)
    sel = np.zeros((N, Nn), dtype=np.int32)
    for i, s in enumerate(sels):
        sel[i, :len(s)] = s
    raw = np.array([nr.rawlen(s, match, off) for s in sels])
    assert all(lens[match[sels[k][0]]] == 0 and 0 < raw[k] < raw.max() for k in (1, 4))         # padded from a later list's first entry
    assert nsel[7] == 0 and raw[7] == 0 and raw.max() > 1000 and all(len(s) > 2 for k, s in enumerate(sels) if k != 7)
    return sels, nsel, sel, match, off, items, raw


@pytest.mark.parametrize('cut', ['full', 'truncated', 'one'])
@pytest.mark.parametrize('device', [False, True])
def test_table_against_the_reference(device, cut):
    sels, nsel, sel, match, off, items, raw = table_case()
    W = {'full': int(raw.max()), 'truncated': int(np.sort(raw)[N // 2]) - 3, 'one': 1}[cut]
    assert cut == 'full' or (raw > W).sum() >= 4
    ref = nr.table(sels, match, off, items, W)
    e = eng()
    band = 512
    out = e.device_array(np.full(N * W + band, -7, dtype=np.int64))            # the table, and a guard band behind it
    if device:
        e.net_table(e.device_array(nsel), e.device_array(sel), e.device_array(match), DevArray(off), DevArray(items), W, out)
    else:
        e.net_table(nsel, sel, match, off, items, W, out)
    got = out.numpy()
    np.testing.assert_array_equal(got[:N * W].reshape(N, W), ref)
    np.testing.assert_array_equal(got[N * W:], -7)                               # nothing is written past a row cut at W
    if cut == 'full':
        host = np.full((N, W), -7, dtype=np.int64)
        e.net_table(nsel, sel, match, off, items, W, host)
        np.testing.assert_array_equal(host, ref)
        assert np.all(ref[7] == 0) and ref[1, 0] == items[off[match[sels[1][1]]]]


# ---- k_net_gather ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.float64, np.int64])
@pytest.mark.parametrize('pad', [0, -99])
@pytest.mark.parametrize('device', [False, True])
def test_gather_is_bit_exact(device, pad, dtype):
    rs = np.random.RandomState(5)
    Nn = 100
    lp = rs.normal(0, 3, size=(N, Nn))
    lp[6, 3] = np.nan                                                            # an object that selects nothing: a row of pads
    sels = [nr.select(r, False, 0.0, 0.05 if i % 2 else 0.6)[0] for i, r in enumerate(lp)]
    nsel = np.array([len(s) for s in sels], dtype=np.int32)
    sel = np.zeros((N, Nn), dtype=np.int32)
    for i, s in enumerate(sels):
        sel[i, :len(s)] = s
    plane = lp.copy() if dtype == np.float64 else rs.randint(-2**62, 2**62, size=(N, Nn)).astype(np.int64)
    plane[6, 3] = 0
    e = eng()
    for W in (1, int(nsel.max())):
        assert (N * W) % 256 and (W == 1 or N * W > 256) and nsel.min() == 0 and nsel.max() > 64
        ref = nr.gather(plane, sels, W, pad)
        if device:
            out = e.device_empty((N, W), dtype)
            e.net_gather(e.device_array(plane), e.device_array(nsel), e.device_array(sel), W, pad, out)
            got = out.numpy()
        else:
            got = np.full((N, W), 5, dtype=dtype)
            e.net_gather(plane, nsel, sel, W, pad, got)
        np.testing.assert_array_equal(got.view(np.int64), ref.view(np.int64))


# ---- k_net_stack -------------------------------------------------------------------------------------------------------------------
ULP = 2.0**-52


@pytest.mark.parametrize('G', [1, 64, 65, 701])
@pytest.mark.parametrize('n', [1, 64, 65, 300])
def test_stack_against_the_longdouble_reference(n, G):
    rs = np.random.RandomState(100 * n + G)
    Nn, Nnodes = n + 7, n + 12
    lp = -rs.uniform(0, 600, size=(N, Nn)) - rs.uniform(0, 50, size=(N, 1))     # selected entries within 600 of their row's max
    sels = [rs.permutation(Nn)[:n] for _ in range(N)]
    sels[8] = np.zeros(0, dtype=np.int64)                                       # no node: a nan row, as numpy's 0 / 0
    sels[2] = np.sort(sels[2])[:max(1, n // 2)]                                 # a shorter selection, in index order
    nsel = np.array([len(s) for s in sels], dtype=np.int32)
    sel = np.zeros((N, Nn), dtype=np.int32)
    for i, s in enumerate(sels):
        sel[i, :len(s)] = s
    match = rs.permutation(Nnodes)[:Nn].astype(np.int32)
    node_pdfs = rs.rand(Nnodes, G) * (rs.rand(Nnodes, G) > 0.2) * np.exp(rs.uniform(-20, 0, size=(Nnodes, 1)))
    node_pdfs[:, 0] += 1e-30                                                     # (no all-zero stack)
    rp, rlm, rle = nr.stack(lp, sels, match, node_pdfs)
    e = eng()
    pdfs = np.full((N, G), 5.); lmap = np.full(N, 5.); levid = np.full(N, 5.)
    e.net_stack(lp, nsel, sel, match, node_pdfs, pdfs, lmap, levid)
    live = nsel > 0
    assert np.all(np.isnan(pdfs[~live])) and np.all(np.isnan(rp[~live].astype(np.float64)))
    got, ref = pdfs[live].astype(nr.LD), rp[live]
    # all terms are non-negative: (n + G / 64 + 10) ulp from the sums and the division, 6e-16 from the weights -- 5e-14 here
    rel = float(np.max(np.abs(got - ref) / np.maximum(ref, nr.LD(1e-290))))
    worst['stack pdf'] = max(worst['stack pdf'], rel)
    print('stack pdf: worst relative deviation %.3g (worst so far %.3g)' % (rel, worst['stack pdf']))
    assert np.all(np.abs(got - ref) <= 1e-12 * np.abs(ref) + 1e-290)
    assert np.all(np.abs(got.sum(axis=1) - 1) <= G * ULP)
    np.testing.assert_array_equal(lmap, rlm)
    check_levid(levid, rle, 'stack levid')
    # the same call with every argument in device memory: equal bits
    d_pdfs, d_lmap, d_levid = e.device_empty((N, G)), e.device_empty(N), e.device_empty(N)
    e.net_stack(DevArray(lp), e.device_array(nsel), e.device_array(sel), e.device_array(match), DevArray(node_pdfs), d_pdfs, d_lmap, d_levid)
    for h, d in zip((pdfs, lmap, levid), (d_pdfs, d_lmap, d_levid)):
        np.testing.assert_array_equal(h.view(np.int64), d.numpy().view(np.int64))
