"""Host-or-device arguments of the chunked entry points (csrc/fz_stage.h): the same seeded input run four ways -- every array in
host memory or in device memory, the workspace limit at its default or at 1 MiB, the smallest the library takes -- gives the same
bits.  At 1 MiB every case below runs in two or more chunks with a short last one in at least one of the two placements: the
smallest shapes at which the offset arithmetic of a chunk (``i0 * stride``, ``stats + r * N + i0``) can go wrong.  The chunk length
of each case is worked out from the rule in the source in the comment above it, as ``host / device`` objects per chunk at 1 MiB
(``N``: one chunk, the rule does not cut that placement).

What is compared:
* per-row results (statistics, resampled and recentred rows, bins, draws, PDFs, ln-max / ln-evidence, neighbour tables, fits) and
  integer call-wide results (counts): ``array_equal`` across all four ways;
* floating call-wide sums (``lnlike`` of overlap_nz, ``hist`` of cdf_draws) are summed chunk by chunk, so their last bits follow
  the chunking: ``array_equal`` between any two ways that cut the objects alike, and across different cuts the tolerance the
  entry point's own test holds against its reference (test_hip_summary: rtol 1e-13; test_hip_diag: rtol 4 N Nmc u).  Device PDFs
  are never cut by these two entry points (nc = N in the source), so at 1 MiB the device way runs ONE chunk where the host way
  runs two: there the two ways differ in the cut although the limit is the same, and it is the cut that decides which of the two
  comparisons applies.

The plane entry points that predict use the CDF rule or the neighbour kernels: the weight-threshold route of fz_predict_logwt
chooses between kernels by the workspace limit itself (candidate lists or two passes), which is not what is under test here."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
DEFAULT, SMALL = 32 << 30, 1 << 20
N, G, G2, NMC = 2500, 64, 48, 8
M, B, K = 600, 5, 8                 # the plane entry points: models, bands, neighbours


@pytest.fixture(scope='module')
def eng():
    from frankenz_amd.engine import get_engine
    return get_engine()


class Way(object):
    """where a case's arrays live: ``put`` an input, ``new`` an output, ``get`` a result back as NumPy"""

    def __init__(self, eng, dev):
        self.eng, self.dev = eng, dev

    def put(self, a):
        a = np.ascontiguousarray(a)
        return self.eng.device_array(a) if self.dev else a.copy()

    def new(self, shape, dtype=np.float64, fill=-7):
        return self.put(np.full(shape, fill, dtype=dtype))

    @staticmethod
    def get(a):
        return a if isinstance(a, np.ndarray) else a.numpy()


def stack(seed, n=N, g=G):
    """n positive rows on g points, not normalised, and the grid"""
    rs = np.random.RandomState(seed)
    grid = np.linspace(0., 4., g)
    mu, sd = rs.uniform(0.2, 3.8, n)[:, None], rs.uniform(0.05, 0.6, n)[:, None]
    pdfs = np.exp(-0.5 * np.square((grid[None, :] - mu) / sd)) + 1e-4 * rs.rand(n, g)
    return rs, grid, pdfs * rs.uniform(0.5, 2., n)[:, None]


# ---- the cases: f(way) -> {name: result} ------------------------------------------------------------------------------------------
# summarize: per object G * 8 (+ G * 8 for a staged row) + 26 * 8 bytes -> 1 MiB / 1232 = 851 / 1 MiB / 720 = 1456
def case_summarize(w):
    rs, grid, pdfs = stack(1)
    loss = 1. - 1. / (1. + np.square((grid[:, None] - grid[None, :]) / 0.1))
    d_pdfs, stats = w.put(pdfs), w.new((21, N))
    w.eng.pdfs_summarize(d_pdfs, grid, True, w.put(rs.rand(N)), w.put(loss), w.put(rs.uniform(0.02, 0.2, (N, 4))), 0.03, stats)
    return {'stats': w.get(stats), 'pdfs renormalised in place': w.get(d_pdfs)}


# resample: (G + G2) * 8 = 896 bytes per object -> 1170 / 1170
def case_resample(w):
    _, grid, pdfs = stack(2)
    out = w.new((N, G2))
    w.eng.pdfs_resample(w.put(pdfs), grid, np.linspace(-0.3, 4.2, G2), 0., -1., True, out)
    return {'rows': w.get(out)}


# recentre: (G + G2) * 8 + 8 = 904 bytes per object -> 1159 / 1159
def case_recentre(w):
    rs, grid, pdfs = stack(3)
    out = w.new((N, G2))
    w.eng.recentre_rows(w.put(pdfs), N, grid, w.put(rs.uniform(0.1, 3.9, N)), 1, np.linspace(-1.5, 1.5, G2), out)
    return {'rows': w.get(out)}


# overlap_nz: G * 8 + 16 = 528 bytes per host object -> 1985 / N
def case_overlap(w):
    rs, _, pdfs = stack(4)
    ov = w.new(N)
    ll = w.eng.overlap_nz(w.put(pdfs), rs.dirichlet(np.full(G, 0.8)), (5, 40), 1e-3, ov)
    return {'overlap': w.get(ov), 'sum:lnlike': np.array([ll])}


# nz_assign: G * 8 + 32 = 544 bytes per host object -> 1927 / N; with the bins and without them (scratch behind a NULL output)
def case_assign(w):
    rs, _, pdfs = stack(5)
    nz, u = rs.dirichlet(np.full(G, 0.8)), rs.rand(N)
    bins, counts, only = w.new(N, np.int64), w.new(G, np.int64), w.new(G, np.int64)
    w.eng.nz_assign(w.put(pdfs), nz, w.put(u), bins, counts)
    w.eng.nz_assign(w.put(pdfs), nz, w.put(u), None, only)
    return {'bins': w.get(bins), 'counts': w.get(counts), 'counts without bins': w.get(only)}


# nz_sweep: as nz_assign -> 1927 / N; the caller's uniforms, and the generator (its counter is the object's index in the whole stack)
def case_sweep(w):
    rs, _, pdfs = stack(6)
    nz, u = rs.dirichlet(np.full(G, 0.8)), rs.rand(N)
    cu, cp = w.new(G, np.int64), w.new(G, np.int64)
    d_pdfs = w.put(pdfs)
    w.eng.nz_sweep(d_pdfs, N, nz, cu, u=w.put(u))
    w.eng.nz_sweep(d_pdfs, N, nz, cp, key=(12345, 678), sweep=3)
    return {'counts, uniforms': w.get(cu), 'counts, philox': w.get(cp)}


# colsum: whole blocks of rows within 1 MiB / (G * 8) = 2048 -> 2048 / N; one summation order whatever the cut: equal bits
def case_colsum(w):
    _, _, pdfs = stack(7)
    out = w.new(G)
    w.eng.pdfs_colsum(w.put(pdfs), G, out)
    return {'colsum': w.get(out)}


# cdf_draws: G * 8 + 2 * NMC * 8 + 8 = 648 bytes per host object -> 1618 / N (8 bytes per resident object); the histogram alone too
def case_cdf_draws(w):
    rs, grid, pdfs = stack(8)
    mc, wt, edges = rs.uniform(-0.2, 4.2, (N, NMC)), rs.uniform(0.05, 1., N), np.linspace(0., 1., 11)
    draws, hist, only = w.new((N, NMC)), w.new(10), w.new(10)
    d_pdfs, d_mc, d_wt = w.put(pdfs), w.put(mc), w.put(wt)
    w.eng.cdf_draws(d_pdfs, N, grid, d_mc, weights=d_wt, edges=edges, draws=draws, hist=hist)
    w.eng.cdf_draws(d_pdfs, N, grid, d_mc, weights=d_wt, edges=edges, hist=only)
    return {'draws': w.get(draws), 'sum:hist': w.get(hist), 'sum:hist alone': w.get(only)}


def plane_problem(seed, n):
    """M models of B bands with dictionary labels on a G-point grid, uploaded; n objects"""
    from frankenz_amd import PDFDict
    from frankenz_amd.engine import get_engine
    rs = np.random.RandomState(seed)
    sig = np.array([0.873, 0.348, 0.418, 0.873, 3.476])
    Y = rs.lognormal(1., 1., size=(M, B)); Ye = 0.05 * Y; Ym = np.ones((M, B))
    X = Y[rs.choice(M, n)] + sig * rs.randn(n, B); Xe = np.tile(sig, (n, 1)); Xm = np.ones((n, B))
    eng = get_engine()
    eng.upload_models(Y, Ye, Ym)
    assert eng.set_labels(rs.uniform(0.3, 6., M), rs.uniform(0.05, 0.4, M), label_dict=PDFDict(np.linspace(0., 6.3, G), np.linspace(0.05, 0.6, 12))) == G
    eng.knn_upload_trees(Y[None].astype(np.float32))
    return rs, X, Xe, Xm


# predict_logwt (CDF rule): M * 8 = 4800 bytes per host row -> 218 / N; with the goodness-of-fit outputs and without them
def case_predict_logwt(w):
    from frankenz_amd.engine import kde_opts
    n = 700
    rs, _, _, _ = plane_problem(9, n)
    logwt = w.put(-rs.exponential(3., (n, M)))
    ko = kde_opts({'wt_thresh': None, 'cdf_thresh': 0.01})
    pdfs, lmap, levid, only = w.new((n, G)), w.new(n), w.new(n), w.new((n, G))
    w.eng.predict_logwt(logwt, ko, pdfs, lmap, levid)
    w.eng.predict_logwt(logwt, ko, only)
    return {'pdfs': w.get(pdfs), 'lmap': w.get(lmap), 'levid': w.get(levid), 'pdfs without lmap / levid': w.get(only)}


# fit_prior: M * 8 = 4800 bytes per object and staged plane, three planes, + 4800 for a dense host table -> 72 and 54 / N
def case_fit_prior(w):
    from frankenz_amd.engine import like_opts
    n, P = 700, 7
    rs, X, Xe, Xm = plane_problem(10, n)
    out = {}
    for tag, prior in (('rows', (w.put(rs.dirichlet(np.full(M, 0.5), size=P)), P, w.put(rs.randint(0, P - 1, n).astype(np.int64)), w.put(rs.rand(n)))),
                       ('dense', (w.put(np.log(rs.dirichlet(np.full(M, 0.5), size=n))), n, None))):
        lnprior, lnlike, lnprob = w.new((n, M)), w.new((n, M)), w.new((n, M))
        w.eng.fit_prior(w.put(X), w.put(Xe), w.put(Xm), like_opts({}), prior, lnprior=lnprior, lnlike=lnlike, lnprob=lnprob)
        out.update({tag + ' lnprior': w.get(lnprior), tag + ' lnlike': w.get(lnlike), tag + ' lnprob': w.get(lnprob)})
    return out


# knn_query: 2^18 objects per chunk whatever the limit -> N / N: host against device only (the limits repeat it)
def knn_table(w, X):
    idx = w.new((len(X), K), np.int64)
    w.eng.knn_query(w.put(X), K, np.inf, idx)
    return idx


def case_knn_query(w):
    _, X, _, _ = plane_problem(11, N)
    return {'idx': w.get(knn_table(w, X))}


# knn_fit_predict: 3 * K * 8 = 192 bytes per object + 920 of staged outputs -> 942 / 5461, hence 6000 objects; then without
# lmap / levid.  knn_predict_logwt on its results: K * 16 + G * 8 = 640 bytes per object -> 1638 / 1638
def case_knn_fit_predict(w):
    from frankenz_amd.engine import kde_opts, like_opts
    n = 6000
    _, X, Xe, Xm = plane_problem(12, n)
    idx = knn_table(w, X)
    o = dict(neighbors=w.new((n, K), np.int64), nnbr=w.new(n, np.int64), lnlike=w.new((n, K)), chi2=w.new((n, K)), ndim=w.new((n, K), np.int64),
             scale=w.new((n, K)), scale_err=w.new((n, K)), pdfs=w.new((n, G)), lmap=w.new(n), levid=w.new(n))
    w.eng.knn_fit_predict(w.put(X), w.put(Xe), w.put(Xm), idx, K, like_opts({}), kde_opts({}), **o)
    only = w.new((n, G))
    w.eng.knn_fit_predict(w.put(X), w.put(Xe), w.put(Xm), idx, K, like_opts({}), kde_opts({}), pdfs=only)
    out = {k: w.get(v) for k, v in o.items()}
    out['pdfs without the rest'] = w.get(only)
    p2, lm2, p3 = w.new((n, G)), w.new(n), w.new((n, G))
    w.eng.knn_predict_logwt(o['lnlike'], o['neighbors'], o['nnbr'], K, kde_opts({}), p2, lm2, None)
    w.eng.knn_predict_logwt(o['lnlike'], o['neighbors'], o['nnbr'], K, kde_opts({'wt_thresh': None, 'cdf_thresh': 0.01}), p3)
    out.update({'predict_logwt pdfs': w.get(p2), 'predict_logwt lmap': w.get(lm2), 'predict_logwt pdfs, CDF rule': w.get(p3)})
    return out


CASES = {f.__name__[5:]: f for f in (case_summarize, case_resample, case_recentre, case_overlap, case_assign, case_sweep, case_colsum,
                                     case_cdf_draws, case_predict_logwt, case_fit_prior, case_knn_query, case_knn_fit_predict)}
# objects per chunk (host, device) at 1 MiB of the cases with a chunk-dependent sum, and the tolerance across different cuts
SUMS = {'overlap': ((1985, N), dict(rtol=1e-13, atol=0)), 'cdf_draws': ((1618, N), dict(rtol=4 * N * NMC * U, atol=0))}


def four_ways(eng, name):
    """{(device?, limit): results}"""
    res = {}
    for lim in (DEFAULT, SMALL):
        eng.set_workspace_limit(lim)
        try:
            for dev in (False, True):
                res[dev, lim] = CASES[name](Way(eng, dev))
        finally:
            eng.set_workspace_limit(DEFAULT)
    return res


@pytest.mark.parametrize('name', sorted(CASES))
def test_four_ways_give_the_same_bits(eng, name):
    res = four_ways(eng, name)
    first = res[False, DEFAULT]
    cut = lambda way: N if way[1] == DEFAULT else SUMS[name][0][int(way[0])]
    for way, got in res.items():
        assert sorted(got) == sorted(first)
        for key in got:
            where = '%s, %s: %s at %d bytes' % (name, key, 'device' if way[0] else 'host', way[1])
            assert got[key].shape == first[key].shape and not (got[key] == -7).all(), where
            if not key.startswith('sum:') or cut(way) == N:
                assert np.array_equal(got[key], first[key], equal_nan=True), where
            else:
                print(where, 'max rel', np.abs(got[key] / first[key] - 1).max())
                np.testing.assert_allclose(got[key], first[key], err_msg=where, **SUMS[name][1])


# ---- in / out arrays: fz_nz_pairs with host state and a segment that starts past the first sample -----------------------------------
def nz_pairs_segment(eng, dev, nsamp=3, thin=4, mh=2, s0=1):
    """samples [s0, nsamp) of a chain over 400 resident PDFs, its in / out state in host or device arrays filled with -7"""
    from frankenz_amd.samplers import _predraw_population, stack_nz
    rs, _, pdfs = stack(13, n=400)
    pdfs /= pdfs.sum(axis=1)[:, None]
    pairs, normals, expo = _predraw_population(rs, G, nsamp, thin, mh)
    d_pdfs = eng.device_array(pdfs)
    pos0 = stack_nz(d_pdfs)
    w = Way(eng, dev)
    overlap, dcol = eng.device_empty(400), eng.device_array(np.zeros(400))
    lnpost = np.array([eng.overlap_nz(d_pdfs, pos0, None, 0., overlap, n=400)])
    st = dict(pos=w.put(pos0), lnpost=w.put(lnpost), samples=w.new((nsamp, G)), samples_lnp=w.new(nsamp),
              accept=w.new((nsamp * thin, mh), np.int32), gscale=w.new(nsamp * thin))
    eng.nz_pairs(d_pdfs, 400, G, st['pos'], overlap, dcol, st['lnpost'], w.put(pairs), w.put(normals), w.put(expo), nsamp, thin, mh, s0,
                 nsamp, st['samples'], st['samples_lnp'], st['accept'], st['gscale'])
    out = {k: w.get(v) for k, v in st.items()}
    out['overlap'] = overlap.numpy()
    return out


def test_nz_pairs_host_state_keeps_what_the_segment_does_not_write(eng):
    """samples [1, 3) of 3: sample 0 and the pairs before the segment keep the caller's values in the host arrays, as they do in
    device arrays; what the segment writes is the same bits either way"""
    h, d = nz_pairs_segment(eng, False), nz_pairs_segment(eng, True)
    for k in h:
        assert np.array_equal(h[k], d[k]), k
    assert (h['samples'][:1] == -7).all() and (h['samples_lnp'][:1] == -7).all()
    assert (h['accept'][:4] == -7).all() and (h['gscale'][:4] == -7).all()
    assert not (h['samples'][1:] == -7).any() and not (h['gscale'][4:] == -7).any()
    assert np.array_equal(h['samples'][-1], h['pos']) and h['samples_lnp'][-1] == h['lnpost'][0]


# ---- the placement the 1 MiB tests of fz_stack2d and fz_synphot leave out: device memory ----------------------------------------------
def test_stack2d_resident_rows_at_the_smallest_limit(eng):
    """test_hip_diag holds host rows at both limits and resident rows at the default one"""
    import _diag_ref as ref
    from conftest import load_golden
    from frankenz_amd import plotting
    from test_hip_diag import make_case, stack_close
    d = ref.StoredDict(load_golden('g19_diagnostics'))
    vals, errs, pdfs, pgrid, wt = make_case(54, 3000, d, 77, 0.28)
    want = ref.input_vs_pdf(vals, errs, d, pdfs, pgrid, weights=wt)
    eng.set_workspace_limit(SMALL)
    try:
        got = plotting.input_vs_pdf(vals, errs, d, eng.device_array(pdfs), pgrid, weights=wt, plot=False)
    finally:
        eng.set_workspace_limit(DEFAULT)
    stack_close(got, want, 3000)


def test_synphot_device_output_at_the_smallest_limit(eng):
    """test_hip_synphot holds a host output at both limits and a device output at the default one.  1 MiB / (5 filters * 8 + 40)
    = 13 107 pairs per chunk: 14 000 pairs are two chunks, the second written at an offset into the device array"""
    import _synphot_case as case
    from frankenz_amd import simulate
    ms = case.synthetic_survey([2, 63, 64, 65, 129], [2, 300], seed=3)
    tb = simulate._Tables(ms.filters, ms.templates)
    rs = np.random.RandomState(14)
    tmpl, z = rs.randint(0, 2, 14000).astype(np.int64), rs.uniform(0., 4., 14000)
    eng.synphot_upload(tb)
    want = np.full((14000, tb.Nf), -7.)
    eng.synphot(tmpl, z, np.log(1 + z), 1, want)
    got = eng.device_array(np.full((14000, tb.Nf), -7.))
    eng.set_workspace_limit(SMALL)
    try:
        eng.synphot(tmpl, z, np.log(1 + z), 1, got)
    finally:
        eng.set_workspace_limit(DEFAULT)
    assert np.array_equal(got.numpy(), want) and not (want == -7).any()
