"""Golden fixture of the bin masses (docs/bins.md): what the reference's ``frankenz.pdf.gaussian_bin`` gives on fixed inputs.

    python tests/golden/make_golden_bins.py <path to a checkout of the reference, joshspeagle/frankenz v0.3.5>

Writes tests/golden/g23_bins.npz -- data only, no reference source:
  edges_u (71), edges_t (9)          70 uniform bins of 0.1 on [0, 7]; 8 unequal tomographic bins
  mu, std (200)                      centres inside and outside the range and exactly on edges; widths from 1/10 of a uniform bin to
                                     the whole range
  bin_u (200, 70), bin_t (200, 8)    gaussian_bin(mu_i, std_i, edges)
  mix_w, mix_y, mix_s (500)          one mixture: weights (max 1, down to e^-6), labels, errors
  mix_u (70), mix_t (8)              sum_t w_t gaussian_bin(y_t, s_t, edges), added in index order in float64
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    sys.path.insert(0, sys.argv[1])
    from frankenz.pdf import gaussian_bin
    rs = np.random.RandomState(2300)
    edges_u = np.arange(71) * 0.1
    edges_t = np.array([0., 0.3, 0.5, 0.7, 0.9, 1.2, 1.6, 2.5, 7.])
    n = 200
    mu = rs.uniform(-1., 8., n)
    mu[:40] = edges_u[rs.randint(0, 71, 40)]                         # exactly on an edge
    mu[40:50] = edges_t[rs.randint(0, 9, 10)]
    mu[50:60] = rs.uniform(-3., -0.5, 10); mu[60:70] = rs.uniform(7.5, 10., 10)
    std = np.exp(rs.uniform(np.log(0.01), np.log(7.), n))
    bin_u = np.array([gaussian_bin(m, s, edges_u) for m, s in zip(mu, std)])
    bin_t = np.array([gaussian_bin(m, s, edges_t) for m, s in zip(mu, std)])
    W = 500
    mix_w = np.exp(-rs.uniform(0., 6., W)); mix_w[rs.randint(W)] = 1.
    mix_y = rs.uniform(-0.5, 7.5, W)
    mix_s = np.exp(rs.uniform(np.log(0.01), np.log(2.), W))
    mix_u, mix_t = np.zeros(70), np.zeros(8)
    for w, y, s in zip(mix_w, mix_y, mix_s):
        mix_u += w * gaussian_bin(y, s, edges_u)
        mix_t += w * gaussian_bin(y, s, edges_t)
    np.savez_compressed(os.path.join(HERE, 'g23_bins.npz'), edges_u=edges_u, edges_t=edges_t, mu=mu, std=std, bin_u=bin_u, bin_t=bin_t,
                        mix_w=mix_w, mix_y=mix_y, mix_s=mix_s, mix_u=mix_u, mix_t=mix_t)


if __name__ == '__main__':
    main()
