"""The law of ``fz_net_union`` as NumPy states it (tests/_net_union_ref.py), and the refusals of ``Network.fit_sparse`` that are raised
before any device call.  No GPU."""
import numpy as np
import pytest

import _net_union_ref as ur


def random_case(seed, N=40, Nn=12, Nnodes=20, M=500):
    rs = np.random.RandomState(seed)
    lists = [rs.randint(0, M, size=rs.randint(0, 60)).tolist() for _ in range(Nnodes)]
    lists[0] = []; lists[7] = []
    match = rs.choice(Nnodes, Nn, replace=False).astype(np.int32)
    nsel = rs.randint(0, Nn + 1, size=N).astype(np.int32)
    sel = np.stack([rs.permutation(Nn) for _ in range(N)]).astype(np.int32)
    off, items = ur.csr(lists)
    return nsel, sel, match, off, items


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_union_is_the_sorted_first_appearance_list(seed):
    nsel, sel, match, off, items = random_case(seed)
    nuniq = ur.union(nsel, sel, match, off, items)
    for i in range(len(nsel)):
        fa = ur.first_appearance(ur.concat(nsel, sel, match, off, items, i))
        assert nuniq[i] == len(fa)
    W = int(nuniq.max())
    nu2, idx = ur.union(nsel, sel, match, off, items, W)
    np.testing.assert_array_equal(nu2, nuniq)
    for i in range(len(nsel)):
        fa = np.sort(ur.first_appearance(ur.concat(nsel, sel, match, off, items, i)))
        np.testing.assert_array_equal(idx[i, :nuniq[i]], fa)
        if nuniq[i]:
            assert (idx[i, nuniq[i]:] == fa[0]).all()
            # what the subset fit does to the padded row leaves the ascending union
            np.testing.assert_array_equal(ur.first_appearance(idx[i]), fa)
        else:
            assert (idx[i] == 0).all()


def test_union_cut_at_w_and_identity_match():
    lists = [[5, 3, 9], [], [3, 3, 0], [11]]
    off, items = ur.csr(lists)
    nsel = np.array([3, 0, 1, 2], dtype=np.int32)
    sel = np.array([[0, 1, 2, 3], [0, 0, 0, 0], [1, 0, 0, 0], [3, 2, 0, 0]], dtype=np.int32)
    nuniq, idx = ur.union(nsel, sel, None, off, items, 3)
    np.testing.assert_array_equal(nuniq, [4, 0, 0, 3])
    np.testing.assert_array_equal(idx, [[0, 3, 5], [0, 0, 0], [0, 0, 0], [0, 3, 11]])
    _, wide = ur.union(nsel, sel, None, off, items, 6)
    np.testing.assert_array_equal(wide[0], [0, 3, 5, 9, 0, 0])
    np.testing.assert_array_equal(wide[3], [0, 3, 11, 0, 0, 0])
    # a row whose smallest element is not 0 is padded with that element
    nsel[:] = [1, 1, 1, 1]; sel[:, 0] = [0, 3, 0, 3]
    _, pad = ur.union(nsel, sel, None, off, items, 5)
    np.testing.assert_array_equal(pad[0], [3, 5, 9, 3, 3])
    np.testing.assert_array_equal(pad[1], [11, 11, 11, 11, 11])


def bare_network(M=6, B=3):
    from frankenz_amd.networks import Network
    return Network(np.ones((M, B)), np.ones((M, B)), np.ones((M, B)))


def test_fit_sparse_refusals_that_need_no_device():
    from frankenz_amd import pdf as fpdf
    from frankenz_amd import networks
    X = np.ones((2, 3))
    net = bare_network()
    with pytest.raises(ValueError, match='has not been trained'):
        net.fit_sparse(X, X, X, verbose=False)
    # a populated network, as data (the lists are plain attributes)
    net.set_nodes(np.ones((2, 3)))
    net.nodes_idxs, net.nodes_bmus, net.nodes_Nmatch = [[0, 1], [2]], [[0, 1], [2]], np.array([2, 1])
    net.lpnet_func, net.lpnet_args, net.lpnet_kwargs = fpdf.logprob, [], {'free_scale': True, 'ignore_model_err': True, 'return_scale': True}
    mine = lambda *a, **k: fpdf.logprob(*a, **k)
    with pytest.raises(NotImplementedError, match='built-in likelihood'):
        net.fit_sparse(X, X, X, lprob_func=mine, verbose=False)
    with pytest.raises(NotImplementedError, match='built-in likelihood'):
        net.fit_sparse(X, X, X, lprob_args=[1.0], verbose=False)
    with pytest.raises(TypeError):
        net.fit_sparse(X, X, X, nodes_only=True, verbose=False)           # rows over nodes are not rows over models
    net.lpnet_func = mine
    with pytest.raises(NotImplementedError, match='built-in node likelihood'):
        net.fit_sparse(X, X, X, verbose=False)
    net.lpnet_func = fpdf.logprob
    assert networks._UNION_MMAX == 1 << 20 and networks._UNION_MAX == 4096
    net.NMODEL = (1 << 20) + 1
    with pytest.raises(NotImplementedError, match='FZ_NET_UNION_MMAX'):
        net.fit_sparse(X, X, X, verbose=False)
    net.NMODEL = 6
    with pytest.raises(NotImplementedError, match='not understood'):
        net.fit_sparse(X, X, X, lprob_kwargs={'bogus': 1}, verbose=False)
