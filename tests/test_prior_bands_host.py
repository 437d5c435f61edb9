"""What tests/test_hip_prior_bands.py relies on, checked without a GPU: on every problem of that module a prior read from the wrong
object's row, or from the neighbouring model's entry, moves the oracle's ln-evidence by more than ten times the tolerance the GPU
result is held to on at least 90 % of the finite rows; at least three quarters of the rows are finite in the oracle; the object whose
best fit the prior excludes is what its name says; and the source rules the model counts are derived from give what
docs/bpz_prior.md lists."""
import numpy as np
import pytest

import _prior_case as pc


def ident(c):
    return '%d-%s-M%d-%s-%s' % c


def check(kind, B, variant, N, M, T, mode, idx):
    sa, sb, fin, right, excl, weighs = pc.sensitivity(kind, B, variant, N, M, T, mode, idx)
    print('moved by the object shift %.3f, by the model shift %.3f of the finite rows (%.3f of all)' % (sa, sb, fin))
    assert fin >= 0.75
    assert sa >= 0.9
    assert M == 1 or sb >= 0.9                    # (one model: there is no neighbouring entry)
    assert excl and weighs
    return right


@pytest.mark.parametrize('case', pc.small_cases(), ids=ident)
def test_small_problems_tell_a_wrong_prior_row(case):
    B, variant, M, mode, kind = case
    T = pc.tile(pc.unit(B), mode)
    N2 = pc.twopass_objects(M)
    idx = tuple(range(202)) + (N2 - 1,)           # (per-object results are independent: the first 202 objects and the last)
    right = check(kind, B, variant, N2, M, T, mode, idx)
    if pc.small_cases().index(case) % 16 == 0:    # the shortcut is the oracle's own ln-evidence, bit for bit
        np.testing.assert_array_equal(right, pc.reference(kind, B, variant, N2, M, T, mode, idx)['levid'])


@pytest.mark.parametrize('case', pc.large_cases(), ids=ident)
def test_large_problems_tell_a_wrong_prior_row(case):
    B, variant, M, mode, kind = case
    T = pc.large_geometry(pc.unit(B), mode, variant)[2]
    idx = pc.large_idx(B, variant, M, mode)
    N = pc.LARGE_N
    assert {0, N - 4, N - 3, N - 2, N - 1, pc.K_EX, pc.K_NODE, pc.K_LAST} <= set(idx) and len(set(idx)) == 64
    right = check(kind, B, variant, N, M, T, mode, idx)
    if pc.large_cases().index(case) % 16 == 0:
        np.testing.assert_array_equal(right, pc.reference(kind, B, variant, N, M, T, mode, idx)['levid'])


@pytest.mark.parametrize('case', pc.modec_cases(), ids=ident)
def test_modec_problems_tell_a_wrong_prior_row(case):
    B, variant, M, mode, kind = case
    check(kind, B, variant, pc.SMALL_N, M, 64, mode, None)


def test_model_counts_follow_the_source_rules():
    """the table of docs/bpz_prior.md ("Coverage"): tile of the (1, 4) geometry and (objects per wave, waves, tile) of a large chunk"""
    small = {(B, mode): pc.tile(pc.unit(B), mode) for B in pc.BANDS_SMALL for mode in ('A', 'Ai', 'B')}
    assert [small[B, 'A'] for B in pc.BANDS_SMALL] == [256, 256, 256, 256, 256, 256, 128, 128, 128, 64, 64, 64]
    assert [small[B, 'Ai'] for B in pc.BANDS_SMALL] == [256] * 9 + [128] * 3
    assert all(small[B, 'B'] == small[B, 'Ai'] for B in pc.BANDS_SMALL)
    geo = {(B, mode, v): pc.large_geometry(B, mode, v) for B in pc.BANDS_LARGE for mode in ('A', 'Ai', 'B') for v in ('fast', 'masked')}
    assert [geo[B, 'A', 'masked'] for B in pc.BANDS_LARGE] == [(2, 16, 512), (2, 16, 512), (2, 16, 256), (4, 8, 256), (4, 8, 256),
                                                               (4, 8, 128), (4, 8, 128)]
    assert [geo[B, 'A', 'fast'] for B in (4, 5, 6, 7, 8)] == [(4, 8, 512), (4, 8, 512), (4, 8, 256), (4, 8, 256), (4, 8, 256)]
    for v in ('fast', 'masked'):
        assert [geo[B, 'Ai', v] for B in pc.BANDS_LARGE] == [(2, 16, 1024)] * 3 + [(4, 8, 512)] * 2 + [(4, 8, 256)] * 2
        assert all(geo[B, 'B', v] == geo[B, 'Ai', v] for B in pc.BANDS_LARGE)
    # every geometry runs once at exactly two tiles
    twice = [c for c in pc.large_cases() if c[2] % 2 == 0]
    assert sorted({pc.large_geometry(pc.unit(c[0]), c[3], c[1]) for c in twice}) == sorted(set(geo.values()))
    assert len(twice) == len(set(geo.values()))
    # 203 objects keep their candidate lists at 1 MiB at these model counts; the object counts of the fallback runs do not
    for M in (65, 129, 257):
        fit = pc.TWOPASS_LIMIT // (4 * M * 16)
        assert fit >= (203 + 3) // 4 and fit < (pc.twopass_objects(M) + 3) // 4 <= pc.CU_COUNT
    assert [pc.twopass_objects(M) for M in (1, 65, 129, 257)] == [203, 1011, 511, 255]
