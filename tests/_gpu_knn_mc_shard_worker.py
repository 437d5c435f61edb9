"""One rank of the two-rank test of tests/test_hip_knn_mc.py: a fresh process per rank, gloo rendezvous on 127.0.0.1, every rank on
GPU 0.  Runs ``sharded_fit_predict(query_draws='device')`` on the overlapped path (gather='pdfs', save_fits=False) and on the block
path (fits kept) and saves what it got.
    python tests/_gpu_knn_mc_shard_worker.py <rank> <world> <port> <outdir>"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))


def scenario():
    """-> (fitter factory, data, err, mask, labels, label_errs, fit_predict kwargs): 1001 objects (no rank count divides them)"""
    from frankenz_amd import NearestNeighbors
    rs = np.random.RandomState(2027)
    sig = np.array([0.873, 0.348, 0.418, 0.873, 3.476])
    N, M = 1001, 1500
    Y = rs.lognormal(1., 1., size=(M, 5)) * 3; Ye = 0.05 * Y; Ym = np.ones((M, 5))
    X = Y[rs.choice(M, N)] + sig * rs.randn(N, 5); Xe = np.tile(sig, (N, 1)); Xm = np.ones((N, 5))
    # an error of 0: the clean (pdf.py:310-311) rewrites the entry to (0, 1, 0), so the draw must come first -- and is x itself.  One
    # such entry in each of the 6 blocks of 167 objects that 2 ranks x 3 rounds deal out: a block with a masked entry takes the
    # library's masked arithmetic variant, one without the fast one (they differ in the last bits), and the single call is one block
    Xe[17 + 167 * np.arange(6), 3] = 0.
    z = rs.uniform(0, 6, M); ze = np.full(M, 0.05)
    mk = lambda: NearestNeighbors(Y, Ye, Ym, K=3, feature_map='luptitude', fmap_kwargs=dict(skynoise=sig, zeropoints=10 ** (0.4 * 23.9)),
                                  rstate=np.random.RandomState(1), verbose=False)
    return mk, X, Xe, Xm, z, ze, dict(label_grid=np.linspace(0., 6., 101), k=5, save_fits=False)


def main():
    rank, world, port, outdir = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    import torch.distributed as dist
    from frankenz_amd import sharded
    os.environ['MASTER_ADDR'] = '127.0.0.1'; os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    mk, X, Xe, Xm, z, ze, kw = scenario()
    nn = mk()
    ov, (ovm, ove) = sharded.sharded_fit_predict(nn, X.copy(), Xe.copy(), Xm.copy(), z, ze, gather='pdfs', chunks=3,
                                                 rstate=np.random.RandomState(2), query_draws='device', **kw)
    key = np.array(nn.query_key)
    nn2 = mk()
    blk, (blm, ble) = sharded.sharded_fit_predict(nn2, X.copy(), Xe.copy(), Xm.copy(), z, ze, gather='pdfs', rstate=np.random.RandomState(2),
                                                  query_draws='device', **dict(kw, save_fits=True))
    assert np.array_equal(nn2.query_key, key)
    np.savez(os.path.join(outdir, 'rank%d.npz' % rank), key=key, ov_pdfs=ov, ov_lmap=ovm, ov_levid=ove, blk_pdfs=blk, blk_lmap=blm, blk_levid=ble)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == '__main__':
    main()
