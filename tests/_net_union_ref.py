"""The law of ``fz_net_union`` in NumPy (include/frankenz_hip.h; docs/network.md, "Sparse rows"): per object the set of model indices
in the lists of its selected nodes -- ``np.unique`` of the concatenated lists --, its size, and the table row: ascending, cut at
``W``, padded with the row's own smallest element (an empty union: ``W`` times index 0)."""
import numpy as np


def csr(lists):
    """ragged per-node lists -> (offsets int64 [Nnodes + 1], items int64, at least one entry long)"""
    off = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([len(v) for v in lists], out=off[1:])
    items = np.concatenate([np.asarray(v, dtype=np.int64) for v in lists]) if off[-1] else np.zeros(1, dtype=np.int64)
    return off, np.ascontiguousarray(items)


def concat(nsel, sel, match, off, items, i):
    """the lists of object i's selected nodes, concatenated in the order of the selection"""
    parts = []
    for s in range(int(nsel[i])):
        c = int(sel[i, s])
        nd = int(match[c]) if match is not None else c
        parts.append(items[off[nd]:off[nd + 1]])
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)


def union(nsel, sel, match, off, items, W=None):
    """-> nuniq (N) int64 [, idx (N, W) int64]"""
    N = len(nsel)
    nuniq = np.zeros(N, dtype=np.int64)
    idx = np.zeros((N, W), dtype=np.int64) if W is not None else None
    for i in range(N):
        u = np.unique(concat(nsel, sel, match, off, items, i))
        nuniq[i] = len(u)
        if idx is not None and len(u):
            k = min(len(u), W)
            idx[i, :k] = u[:k]
            idx[i, k:] = u[0]
    return (nuniq, idx) if W is not None else nuniq


def first_appearance(a):
    """``pandas.unique``: the distinct entries of ``a`` in the order they first appear (what fz_knn_fit_predict does to a table row)"""
    seen, out = set(), []
    for v in np.asarray(a).tolist():
        if v not in seen:
            seen.add(v)
            out.append(v)
    return np.array(out, dtype=np.int64)
