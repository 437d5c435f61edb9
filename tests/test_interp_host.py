"""interp1 (frankenz_amd/csrc/fz_interp.h), the interpolation rule shared by k_summarize, k_resample, k_recentre, k_cdf_draws and
k_synphot, on the host (no GPU): tests/host/interp_check.cpp is compiled with the system C++ compiler and
``-fsanitize=address,undefined`` (the runtimes linked in statically, nothing preloaded), run over heap arrays of exactly n doubles,
and what it prints is compared with ``numpy.interp``.

What is compared.  ``numpy.interp`` looks for the cell from a guess (the previous cell) before it bisects, and a NaN node answers
"not less" to the probes around the guess but "not greater or equal" to the bisection: with NaN nodes its result can depend on the
order of the points.  So numpy is asked three times (one point at a time, all points ascending, all points descending), and wherever
the three agree bit for bit the program's result must be those bits.  The rest is pinned by rule:
  * finite nodes, then NaNs (the cumsum of a row with a NaN): the NaNs order as +inf, so a point ON the last finite node takes its
    value (numpy does so from a guess below the node);
  * NaN at node 0 with finite nodes after it: numpy's (settled) result from the first finite node on, NaN below it;
  * one node: its value for every point, NaN included (numpy's one-node rule).
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NS = (1, 2, 5, 50)
CASES = ('finite', 'plateau', 'tail', 'allnan', 'nan0')


def _compiler():
    for c in (os.environ.get('CXX'), 'c++', 'g++', 'clang++'):
        if c and shutil.which(c):
            return shutil.which(c)
    return None


def _nodes(case, n):
    """xp, fp of tests/host/interp_check.cpp"""
    k = np.arange(n)
    xp = 0.25 + 0.5 * ((k - (k + 1) // 3) if case == 'plateau' else k)
    fp = 1.0 + 0.125 * k * k
    if case == 'tail':
        xp[max(n // 2, 1):] = np.nan
    if case == 'allnan':
        xp[:] = np.nan
    if case == 'nan0':
        xp[0] = np.nan
    return xp, fp


@pytest.fixture(scope='module')
def printed(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip('no C++ compiler')
    exe = str(tmp_path_factory.mktemp('interp') / 'interp_check')
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-fno-omit-frame-pointer', '-ffp-contract=off', '-fsanitize=address,undefined',
           '-fno-sanitize-recover=all', '-I', os.path.join(ROOT, 'frankenz_amd', 'csrc'),
           os.path.join(ROOT, 'tests', 'host', 'interp_check.cpp'), '-o', exe]
    if 'clang' not in os.path.basename(cxx):
        cmd[1:1] = ['-static-libasan', '-static-libubsan']             # (clang links its runtimes statically by default)
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS='detect_leaks=0'))
    assert run.returncode == 0 and not run.stderr, run.stderr[-3000:]    # a sanitizer report ends the program with a message
    out = {}
    for line in run.stdout.strip().split('\n'):
        case, n, xb, rb = line.split()
        out.setdefault((case, int(n)), []).append((int(xb, 16), int(rb, 16)))
    return {k: (np.array([a for a, _ in v], dtype=np.uint64).view(np.float64), np.array([b for _, b in v], dtype=np.uint64).view(np.float64))
            for k, v in out.items()}


def test_every_case_ran(printed):
    assert sorted(printed) == sorted((c, n) for c in CASES for n in NS)
    for (case, n), (x, _) in printed.items():
        xp, _ = _nodes(case, n)
        fin = xp[np.isfinite(xp)]
        assert np.isnan(x).any() and (x < 0.25).any() and (x > 24.75).any()                    # NaN, below and above every node
        assert np.isin(fin, x).all() and np.isin(np.nextafter(fin, 1e9), x).all()              # on every node, and just off it


@pytest.mark.parametrize('n', NS)
@pytest.mark.parametrize('case', CASES)
def test_interp1_against_numpy(printed, case, n):
    x, got = printed[(case, n)]
    xp, fp = _nodes(case, n)
    one = np.array([np.interp(v, xp, fp) for v in x])
    up = np.argsort(x, kind='stable')
    asc = np.empty_like(x); asc[up] = np.interp(x[up], xp, fp)
    dsc = np.empty_like(x); dsc[up[::-1]] = np.interp(x[up[::-1]], xp, fp)
    bits = lambda a: a.view(np.uint64)
    nan3 = np.isnan(one) & np.isnan(asc) & np.isnan(dsc)
    settled = nan3 | ((bits(one) == bits(asc)) & (bits(one) == bits(dsc)))
    last = xp[np.isfinite(xp)][-1] if np.isfinite(xp).any() else None
    if case == 'tail' and n > 1:
        # NaN nodes order as +inf: below the last finite node numpy's result from a fresh guess, which is its result on the finite
        # nodes alone; ON that node its value; NaN beyond it (a NaN slope between two different values)
        m = int(np.isfinite(xp).sum())
        below = x < last
        assert below.sum() >= 3
        assert np.array_equal(bits(got[below]), bits(one[below]))
        assert np.array_equal(bits(got[below]), bits(np.interp(x[below], xp[:m], fp[:m])))
        assert (x == last).any() and np.array_equal(got[x == last], np.full((x == last).sum(), fp[m - 1]))
        assert (x > last).any() and np.isnan(got[~below & (x != last)]).all()
        return
    # where numpy's answer does not depend on its search path: the same bits, NaN where NaN
    assert np.array_equal(np.isnan(got[settled]), np.isnan(one[settled]))
    ok = settled & ~np.isnan(one)
    assert np.array_equal(bits(got[ok]), bits(one[ok]))
    assert np.isnan(got[~settled]).all()                  # ... and NaN where it does
    if case in ('finite', 'plateau', 'allnan') or n == 1:
        assert settled.all()
    if case in ('finite', 'plateau') and n > 1:
        assert np.array_equal(np.isnan(got), np.isnan(x))
    if n == 1:
        assert np.array_equal(got, np.full(len(x), fp[0]))            # numpy's one-node rule: the value, for a NaN point as well
    elif case == 'allnan':
        assert np.isnan(got).all()
    elif case == 'nan0':
        at = (x >= xp[1]) & (x <= last)
        assert settled[at].all() and at.sum() >= 1 and not np.isnan(got[at]).any()
        assert (x < xp[1]).sum() >= 3 and np.isnan(got[x < xp[1]]).all()
        assert np.array_equal(got[x > last], np.full((x > last).sum(), fp[-1]))
