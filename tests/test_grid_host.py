"""The launch arithmetic of frankenz_amd/csrc/fz_grid.h on the host (no GPU): tests/host/grid_check.cpp is compiled with the system C++
compiler and ``-fsanitize=address,undefined`` (the runtimes linked in statically, nothing preloaded), and every line it prints is
compared with the rule as the launch functions spelled it out before the header existed (fz_launch_fused_wm / fz_launch_hist_g,
fz_launch_kde, fz_launch_plane_rows), restated here in Python."""
import os
import subprocess

import pytest

from conftest import ROOT
from test_interp_host import _compiler

LDS = 160 * 1024


def resident(need, bpc, fit, cus):
    """blocks of a resident kernel with candidate lists, or None (+1, not applicable)"""
    blocks = min(need, max(1, bpc) * cus)             # what the occupancy helper answers
    if need > cus:
        k = min(bpc, fit // cus)
        if k >= 1:
            blocks = min(need, k * cus)
        elif fit >= cus // 2:
            blocks = fit
        else:
            return None
    elif fit < need:
        return None
    return blocks


def amb_cap(M, forced, value):
    acap = M if M <= 131072 else max(131072, M // 8)
    if forced:
        acap = max(1, value)
    return acap


def kde_geometry(acc_stride):
    per_obj = acc_stride * 8
    if per_obj * 8 <= 53 * 1024:
        return 2, 4
    if per_obj * 4 <= LDS:
        return 1, 4
    if per_obj * 2 <= LDS:
        return 1, 2
    return 1, 1


def rows_shape(M, G, w2, acc_stride):
    if w2 >= 128 or G + w2 > 65535 or G + w2 > acc_stride or G > 8 * 128:
        return 0, 0
    if M <= 5120:
        nw, e2 = 8, 5
    elif M <= 10240:
        nw, e2 = 8, 10
    else:
        nw, e2 = 16, 10
    capn = nw * 64 * 2 * e2
    if M > capn or M * 5 < capn * 4:
        return 0, 0
    return nw, e2


@pytest.fixture(scope='module')
def printed(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip('no C++ compiler')
    exe = str(tmp_path_factory.mktemp('grid') / 'grid_check')
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-fno-omit-frame-pointer', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
           '-I', os.path.join(ROOT, 'frankenz_amd', 'csrc'), os.path.join(ROOT, 'tests', 'host', 'grid_check.cpp'), '-o', exe]
    if 'clang' not in os.path.basename(cxx):
        cmd[1:1] = ['-static-libasan', '-static-libubsan']             # (clang links its runtimes statically by default)
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS='detect_leaks=0'))
    assert run.returncode == 0 and not run.stderr, run.stderr[-3000:]    # a sanitizer report ends the program with a message
    out = {}
    for line in run.stdout.strip().split('\n'):
        kind, *nums = line.split()
        out.setdefault(kind, []).append(tuple(int(v) for v in nums))
    return out


def test_resident_grid_rule(printed):
    rows = printed['grid']
    seen = set()
    for cus, need, bpc, fit, rc, blocks in rows:
        want = resident(need, bpc, fit, cus)
        assert (rc, blocks) == ((1, -1) if want is None else (0, want)), (cus, need, bpc, fit)
        seen.add((cus, need, bpc, fit))
    for cus in (256, 8):
        for need in (cus - 1, cus, cus + 1):
            for fit in (0, cus // 2 - 1, cus // 2, cus - 1, cus, 2 * cus + 1):
                for bpc in (1, 2):
                    assert (cus, need, bpc, fit) in seen
    # every branch of the rule is among the inputs
    got = {(cus, need > cus, rc, blocks == need, blocks == fit) for cus, need, _, fit, rc, blocks in rows}
    for cus in (256, 8):
        assert {(cus, False, 0, True, False), (cus, False, 1, False, False), (cus, True, 1, False, False), (cus, True, 0, False, True),
                (cus, True, 0, True, False), (cus, True, 0, False, False)} <= got


def test_ambiguous_list_cap(printed):
    rows = printed['cap']
    assert {(M, f, v) for M, f, v, _ in rows} >= {(M, f, v) for M in (1, 131072, 131073, 1048576, 2000000) for f, v in ((0, 0), (1, 1), (1, 3))}
    for M, forced, value, cap in rows:
        assert cap == amb_cap(M, bool(forced), value), (M, forced, value)
    assert dict(((M, f, v), c) for M, f, v, c in rows)[(2000000, 0, 0)] == 250000


def test_kde_geometry_ladder(printed):
    rows = printed['kde']
    assert {st for st, _, _ in rows} >= {848, 849, 5120, 5121, 10240, 10241, 20480}
    for st, tw, wpb in rows:
        assert (tw, wpb) == kde_geometry(st), st
        assert tw * wpb * st * 8 <= LDS                                # what fz_launch_kde_tw asks of the LDS
    assert len({(tw, wpb) for _, tw, wpb in rows}) == 4


def test_plane_rows_shapes(printed):
    rows = printed['rows']
    assert {r[0] for r in rows} >= {4095, 4096, 5120, 5121, 8191, 8192, 10240, 10241, 16383, 16384, 20480, 20481}
    for M, G, w2, stride, nw, e2 in rows:
        assert (nw, e2) == rows_shape(M, G, w2, stride), (M, G, w2, stride)
    assert {(nw, e2) for *_, nw, e2 in rows} == {(0, 0), (8, 5), (8, 10), (16, 10)}
