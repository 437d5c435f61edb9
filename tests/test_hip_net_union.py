"""``fz_net_union`` / ``k_net_union`` alone against the NumPy law (tests/_net_union_ref.py), exact: the union of the selected nodes' lists
with repeats removed, ascending, cut at W and padded with the smallest element -- at every model count where the geometry changes
(word, wave step and waves-per-block seams), on lists of every shape, for host and device arguments."""
import numpy as np
import pytest

import _net_union_ref as ur

pytestmark = pytest.mark.gpu

LDS = 160 * 1024
SEAM4 = LDS // 4 // 4 * 32          # the largest M whose bitmap fits four times: 327 680
SEAM2 = LDS // 2 // 4 * 32          # ... twice: 655 360
MMAX = 1 << 20
FILL = -7


def engine():
    from frankenz_amd.engine import get_engine
    return get_engine(None)


def make_case(M, N, seed):
    """30 nodes, 24 of them behind the columns through a non-identity ``match``.  Lists: empty ones in front and in between, one
    holding 0 and M - 1, one longer than 64, one longer than 4 096, the rest random (repeats inside a list allowed).  Object 0 selects
    nothing, object 1 only empty lists, the others a random number of columns in random order."""
    rs = np.random.RandomState(seed)
    Nnodes, Nn = 30, 24
    lists = [rs.randint(0, M, size=rs.randint(1, 90)).tolist() for _ in range(Nnodes)]
    lists[0] = []; lists[11] = []; lists[12] = []
    lists[3] = [M - 1, 0, M - 1]
    lists[5] = rs.randint(0, M, size=200).tolist()
    lists[9] = rs.randint(0, M, size=5000).tolist()
    match = np.array([0, 11] + [k for k in range(Nnodes) if k not in (0, 11, 20, 21, 22, 23, 24, 25)][::-1], dtype=np.int32)[:Nn]
    assert len(match) == Nn and not (match == np.arange(Nn)).all()
    nsel = rs.randint(1, Nn + 1, size=N).astype(np.int32)
    sel = np.stack([rs.permutation(Nn) for _ in range(N)]).astype(np.int32)
    if N > 1:
        nsel[0] = 0
    if N > 2:
        nsel[1] = 2; sel[1, :2] = [1, 0]                     # columns 0 and 1: nodes 0 and 11, both empty
    if N == 1:
        sel[0] = np.roll(np.arange(Nn), -2); nsel[0] = Nn    # everything, the long lists included
    off, items = ur.csr(lists)
    return nsel, sel, match, off, items


def run(eng, nsel, sel, match, off, items, M, W=None, dev=False, idx=None):
    """-> nuniq [, idx] of the device"""
    N = len(nsel)
    nuniq = np.full(N, FILL, dtype=np.int64)
    if W is not None and idx is None:
        idx = np.full((N, W), FILL, dtype=np.int64)
    if not dev:
        eng.net_union(nsel, sel, match, off, items, M, nuniq, W or 0, idx)
        return (nuniq, idx) if W is not None else nuniq
    d = [eng.device_array(a) if a is not None else None for a in (nsel, sel, match, off, items, nuniq, idx)]
    eng.net_union(d[0], d[1], d[2], d[3], d[4], M, d[5], W or 0, d[6], n=N, nn=sel.shape[1])
    return (d[5].numpy(), d[6].numpy()) if W is not None else d[5].numpy()


M_CASES = [1, 31, 32, 33, 2047, 2048, 2049, 4096, 4097, SEAM4 - 1, SEAM4, SEAM4 + 1, SEAM2 - 1, SEAM2, SEAM2 + 1, 100000]


@pytest.mark.parametrize('M', M_CASES)
def test_union_against_numpy_at_every_seam(M):
    """N = 7: no multiple of four, two or (trivially) one wave per block"""
    eng = engine()
    nsel, sel, match, off, items = make_case(M, 7, M % 1000)
    ref = ur.union(nsel, sel, match, off, items)
    assert ref[0] == 0 and ref[1] == 0 and ref.max() > 0
    cnt = run(eng, nsel, sel, match, off, items, M)
    np.testing.assert_array_equal(cnt, ref)
    for W in sorted({int(ref.max()), max(1, int(ref.max()) // 2)}):
        rnu, ridx = ur.union(nsel, sel, match, off, items, W)
        nu, idx = run(eng, nsel, sel, match, off, items, M, W)
        np.testing.assert_array_equal(nu, ref)                  # the full count in either call, cut or not
        np.testing.assert_array_equal(idx, ridx)
        dnu, didx = run(eng, nsel, sel, match, off, items, M, W, dev=True)
        np.testing.assert_array_equal(dnu, nu); np.testing.assert_array_equal(didx, idx)      # host and device arguments: equal bits


def test_union_of_the_largest_model_set_one_object():
    eng = engine()
    nsel, sel, match, off, items = make_case(MMAX, 1, 3)
    ref = ur.union(nsel, sel, match, off, items)
    W = int(ref[0])
    assert W > 4096
    rnu, ridx = ur.union(nsel, sel, match, off, items, W)
    nu, idx = run(eng, nsel, sel, match, off, items, MMAX, W)
    np.testing.assert_array_equal(nu, rnu); np.testing.assert_array_equal(idx, ridx)
    assert idx[0, 0] == 0 and idx[0, -1] == MMAX - 1
    np.testing.assert_array_equal(run(eng, nsel, sel, match, off, items, MMAX), rnu)
    with pytest.raises(NotImplementedError, match='FZ_NET_UNION_MMAX'):
        run(eng, nsel, sel, match, off, items, MMAX + 1)
    with pytest.raises(NotImplementedError, match='FZ_NET_UNION_MMAX'):
        run(eng, nsel, sel, match, off, items, MMAX + 1, W)


@pytest.mark.parametrize('M', [700, 70000])
def test_every_node_lists_the_same_models_and_disjoint_lists(M):
    eng = engine()
    rs = np.random.RandomState(M)
    base = rs.choice(M, 120, replace=False)
    same = [rs.permutation(base).tolist() for _ in range(50)]                  # rawlen = 50 x unique
    off, items = ur.csr(same)
    nsel = np.array([50, 1, 17], dtype=np.int32)
    sel = np.stack([rs.permutation(50) for _ in range(3)]).astype(np.int32)
    nu, idx = run(eng, nsel, sel, None, off, items, M, 120)                    # identity match
    np.testing.assert_array_equal(nu, [120, 120, 120])
    np.testing.assert_array_equal(idx, np.tile(np.sort(base), (3, 1)))
    perm = rs.permutation(M)[:600]
    disjoint = [perm[k * 12:(k + 1) * 12].tolist() for k in range(50)]
    off, items = ur.csr(disjoint)
    rnu, ridx = ur.union(nsel, sel, None, off, items, 600)
    np.testing.assert_array_equal(rnu, [600, 12, 204])
    nu, idx = run(eng, nsel, sel, None, off, items, M, 600)
    np.testing.assert_array_equal(nu, rnu); np.testing.assert_array_equal(idx, ridx)


@pytest.mark.parametrize('N', [1, 5])
def test_width_equal_to_the_union_and_one_short_with_a_guard_band(N):
    """nuniq == W fills the row exactly; nuniq == W + 1 drops the largest element; nothing is written behind idx"""
    eng = engine()
    M = 5000
    rs = np.random.RandomState(N)
    lists = [rs.choice(M, 77, replace=False).tolist()]
    off, items = ur.csr(lists)
    nsel = np.ones(N, dtype=np.int32); sel = np.zeros((N, 1), dtype=np.int32)
    want = np.sort(lists[0])
    for W in (77, 76):
        guard = 256
        buf = eng.device_array(np.full(N * W + guard, FILL, dtype=np.int64))
        nu = np.zeros(N, dtype=np.int64)
        eng.net_union(nsel, sel, None, off, items, M, nu, W, buf.data_ptr(), n=N, nn=1)
        got = buf.numpy()
        np.testing.assert_array_equal(nu, np.full(N, 77))
        np.testing.assert_array_equal(got[:N * W].reshape(N, W), np.tile(want[:W], (N, 1)))
        assert (got[N * W:] == FILL).all()


def test_an_index_outside_the_models_is_refused_before_any_row_is_written():
    eng = engine()
    M = 3000
    for bad in (M, -1):
        nsel, sel, match, off, items = make_case(M, 7, 11)
        k = int(off[5]) + 130                                # inside list 5 (200 entries), which column 21 reaches
        assert off[5] <= k < off[6]
        ok = ur.union(nsel, sel, match, off, items)
        W = int(ok.max())
        broken = items.copy(); broken[k] = bad
        for dev in (False, True):
            idx = np.full((7, W), FILL, dtype=np.int64)
            didx = eng.device_array(idx) if dev else idx
            args = [eng.device_array(a) for a in (nsel, sel, match, off, broken)] if dev else [nsel, sel, match, off, broken]
            nu = eng.device_array(np.zeros(7, dtype=np.int64)) if dev else np.zeros(7, dtype=np.int64)
            with pytest.raises(IndexError, match=r'outside \[0, %d\)' % M):
                eng.net_union(args[0], args[1], args[2], args[3], args[4], M, nu, W, didx, n=7, nn=sel.shape[1])
            assert ((didx.numpy() if dev else didx) == FILL).all()
            with pytest.raises(IndexError):
                eng.net_union(args[0], args[1], args[2], args[3], args[4], M, nu, n=7, nn=sel.shape[1])       # the counting call too
        # the same bad index in a list that no object selects: nodes 20 .. 25 are behind no column
        lone = items.copy(); lone[int(off[22])] = bad
        nu, idx = run(eng, nsel, sel, match, off, lone, M, W)
        rnu, ridx = ur.union(nsel, sel, match, off, items, W)
        np.testing.assert_array_equal(nu, rnu); np.testing.assert_array_equal(idx, ridx)
