"""Seeded problems, prior tables and oracle runs of tests/test_hip_prior_bands.py (GPU) and tests/test_prior_bands_host.py (the
same problems' sensitivity, checked without a GPU).  Nothing here touches the library: NumPy and the oracle only.

The problems follow ``test_hip_parity.test_oracle_parity_band_counts``: per-band noise ``uniform(0.3, 3.0, B)``, lognormal models
with varying errors, at most ONE masked band per model (15 % of models) and per object (30 % of objects), so ``Ndim >= B - 2``.

Arithmetic variant of a chunk (``pick_var``, csrc/fz_ctx.h) and why each generator variant gets it:

* ``fast``   -- no mask anywhere, tame values, ``B`` itself a compiled band count (4..8).  ``models_wild`` and the objects' flag 4
  are clear (first line), ``models_real_masked`` and the objects' flag 1 are clear (second line), ``BT == B`` (third line): the rule
  falls through to ``VAR_FAST``.
* ``masked`` -- a model has an unobserved band, so ``k_prep_models`` raises flag 1, ``models_real_masked`` is set and the second
  line answers ``VAR_MASKED`` whatever the objects hold.  (Padded counts 3, 10, 20 would get it from the third line or ``VAR_PAD``,
  which every kernel but k_hist runs as its masked variant, even without a mask.)
* ``safe``   -- one model band has ``Ye = 1e20``: its variance 1e40 lies beyond the 1e30 bound of ``k_prep_models``, which raises
  flag 4, ``models_wild`` is set and the FIRST line answers ``VAR_SAFE`` before masks are looked at.  One object band holds a flux
  of 1e40 (flag 4 of ``k_prep_objects``), which alone would do the same.
"""
import functools
import zlib

import numpy as np
from scipy.special import logsumexp

import frankenz_oracle as fo

BT_LIST = (4, 5, 6, 7, 8, 12, 16, 24, 32)                    # FZ_BT_LIST, csrc/fz_ctx.h
MODES = {'A': {}, 'Ai': {'ignore_model_err': True}, 'B': {'free_scale': True, 'ignore_model_err': True},
         'A_nodim': {'dim_prior': False}, 'C': {'free_scale': True}}
KINDS = ('rows', 'lerp')
P = 7                                                        # rows of every prior table
GRID7 = np.array([-1., 0., 0.5, 2., 2.25, 7., 11.])          # uneven nodes of the interpolated form
ALPHA = 0.5                                                  # Dirichlet concentration of the table rows (see sensitivity())
CU_COUNT = 256                                               # compute units of an MI355X: n >= CU_COUNT * 64 takes the large-chunk geometries
PDF_TOL = dict(rtol=1e-7, atol=1e-13)
GOF_TOL = dict(rtol=1e-9, atol=1e-11)                        # ln-max, ln-evidence: close() of test_hip_prior.py / test_hip_bpz_prior.py
LNL_TOL = dict(rtol=1e-9, atol=1e-9)                         # fit_lnlike: test_oracle_parity_band_counts

# objects and models with a part to play (every problem has N >= 37 objects)
K_WILD, K_EX, K_NODE, K_LAST = 3, 5, 7, 6                    # wild flux | best fit excluded by the prior | on an interior node | last band unobserved
J_LAST, J_WILD = 11, 13                                      # model with its last band masked | model with Ye = 1e20 in one band
ROW_EX = 3                                                   # rows form: the table row only K_EX reads; lerp form: K_EX sits in cell ROW_EX + 1


def unit(B):
    """the compiled band count a set of B bands is padded to (pick_bt, csrc/frankenz_hip.hip)"""
    return min(bt for bt in BT_LIST if bt >= B)


# ---- tile lengths, from the rules in csrc/fz_kernels.h ---------------------------------------------------------------------------
def _mode_id(mode):
    return {'A': 0, 'A_nodim': 0, 'Ai': 1, 'B': 2}[mode]


def nval(BT, mode):
    """``static constexpr int NVAL = BT + (MODE == 0 ? BT : 0);``"""
    return BT + (BT if _mode_id(mode) == 0 else 0)


def tile(BT, mode):
    """``static constexpr int TILE = (NVAL > 32) ? 64 : (NVAL > 16 ? 128 : 256);`` -- the tile of the (1, 4) geometry, which runs
    4 waves: ``tile_len<4>()`` below answers TILE"""
    n = nval(BT, mode)
    return 64 if n > 32 else (128 if n > 16 else 256)


def rec_width(BT, mode):
    """``static constexpr int RW = NVAL + ((6 - NVAL % 4) % 4);``"""
    n = nval(BT, mode)
    return n + (6 - n % 4) % 4


def tile_len(BT, mode, nwaves):
    """``tile_len() { return (NWAVES >= 12 && RW <= 6) ? 1024 : ((NWAVES >= 8 && RW <= 10) ? 512 : TILE); }``"""
    rw = rec_width(BT, mode)
    return 1024 if (nwaves >= 12 and rw <= 6) else (512 if (nwaves >= 8 and rw <= 10) else tile(BT, mode))


def large_geometry(BT, mode, variant):
    """(objects per wave, waves per block, tile length) of a chunk of ``n >= cu_count * 64`` objects with a prior
    (fz_launch_fitpredict, csrc/fz_launch.h: ``else if constexpr (SRC::PREF_2x16) ... <SRC, 2, 16> ... else ... <SRC, 4, 8>``) with
    ``PREF_2x16 = (BT <= 6) && ((MODE == 1) || (MODE == 2) || (MODE == 0 && VAR != VAR_FAST))``; above 16 bands every launch takes
    (1, 4)"""
    assert BT <= 16
    m = _mode_id(mode)
    tw, nw = (2, 16) if (BT <= 6 and (m in (1, 2) or variant != 'fast')) else (4, 8)
    return tw, nw, tile_len(BT, mode, nw)


TWOPASS_LIMIT = 1 << 20                                      # the smallest workspace limit fz_set_workspace_limit takes


def twopass_objects(M):
    """How many objects it takes at TWOPASS_LIMIT for a chunk of n < cu_count * 64 objects to lose its candidate lists and run the
    two-pass kernels.  fz_launch_fused_wm at (TW, NW) = (1, 4): ``per_wave = TW * M * sizeof(Cand)`` (16 bytes each), ``need =
    (groups + NW - 1) / NW``, ``fit = ws_limit / (per_wave * NW)`` and, while ``need <= cu_count``, +1 when ``fit < need``
    (fz_grid_resident, csrc/fz_grid.h).  At 1 MiB fit = 16384 / M: 252, 127, 63 at M = 65, 129, 257.  203 objects need 51 blocks, which fit at every one of
    these model counts, so the fallback runs take 4 fit + 3 objects instead (need = fit + 1 <= 253 blocks; three objects in the
    last one): 1011, 511, 255.  A single model's lists always fit (fit = 16384 blocks): that case stays at 203 objects and k_fused."""
    if M == 1:
        return 203
    fit = TWOPASS_LIMIT // (4 * M * 16)
    assert fit + 1 <= CU_COUNT and P * M * 8 <= TWOPASS_LIMIT
    return 4 * fit + 3


# ---- problems --------------------------------------------------------------------------------------------------------------------------
def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7fffffff


def excluded(M, T):
    """models the prior excludes for K_EX: the last two and the last of the first tile of T models"""
    return sorted({j for j in (T - 1, M - 2, M - 1) if 0 <= j < M})


@functools.lru_cache(maxsize=4)
def problem(B, variant, N, M, T):
    """variant: 'fast' (no masks, tame), 'masked', 'safe' (module docstring).  The models of ``excluded(M, T)`` are copies of
    one bright model and K_EX is drawn from it: they share the likelihood of that object, and the prior takes all of them away."""
    assert variant in ('fast', 'masked', 'safe') and N >= 37
    rs = np.random.RandomState(_seed(B, variant, N, M, T))
    sig = rs.uniform(0.3, 3.0, B)
    Y = rs.lognormal(1., 1., size=(M, B))
    jex = excluded(M, T)
    base = 1e4 * Y[M - 1]                       # (bright: no other model comes near K_EX, even with a band less and a free scale)
    Y[jex] = base
    Ye = 0.05 * Y * rs.uniform(0.5, 2, size=(M, B))
    Ye[jex] = Ye[M - 1]
    X = Y[rs.choice(M, N)] * rs.lognormal(0, .3, N)[:, None] + sig * rs.randn(N, B)
    X[K_EX] = base + sig * rs.randn(B)
    Xe = np.tile(sig, (N, 1))
    Ym, Xm = np.ones((M, B)), np.ones((N, B))
    if variant != 'fast':
        hit = rs.rand(M) < 0.15; Ym[hit, rs.randint(0, B, hit.sum())] = 0
        hit = rs.rand(N) < 0.30; Xm[hit, rs.randint(0, B, hit.sum())] = 0
        Ym[jex] = 1; Xm[K_EX] = 1
        # an object and a model without their LAST real band: at 32 (24) bands bit 31 (23) of the mask word then shares its slot
        # with a row index that is not zero (K_LAST never reads row 0)
        Xm[K_LAST] = 1; Xm[K_LAST, B - 1] = 0
        jl = min(J_LAST, M - 1); Ym[jl] = 1; Ym[jl, B - 1] = 0
    if variant == 'safe':
        Ye[min(J_WILD, M - 1), 1] = 1e20       # variance 1e40: beyond the 1e30 bound
        X[K_WILD, 1] = 1e40                     # as test_wild_values_take_the_ieee_variant: X[3, 4] = 1e40
    z, ze = rs.uniform(0.3, 6., M), rs.uniform(0.05, 0.4, M)
    for a in (Y, Ye, Ym, X, Xe, Xm, z, ze):
        a.setflags(write=False)
    return dict(B=B, N=N, M=M, T=T, Y=Y, Ye=Ye, Ym=Ym, X=X, Xe=Xe, Xm=Xm, z=z, ze=ze, jex=jex)


def grids():
    return np.linspace(0., 6.3, 64), np.linspace(0.05, 0.6, 12)


@functools.lru_cache(maxsize=None)
def oracle_dict():
    return fo.KernelDict(*grids())


# ---- prior tables ------------------------------------------------------------------------------------------------------------------------
class Prior(object):
    """kind 'rows': ``table`` (P, M) of ln-prior rows and ``rows`` (N,); kind 'lerp': ``table`` (P, M) of prior VALUES on GRID7 and
    ``coord`` (N,).  ``plain`` is the same table without the entries that exclude ``jex`` for K_EX.  In both forms

    * object 0 reads the last table row (lerp: the top node, r = P - 2, f = 1), object N - 1 reads row 0 (lerp: the cell of rows 0
      and 1, which are all zero: every ln-prior of that object is -inf);
    * K_EX alone reads the entries that are -inf (value 0) at ``jex``;
    * lerp: K_NODE sits on an interior node (f == 0); the other objects lie in cells 1 and 2.  Cells 3 and 5, which share a row
      with K_EX's cell 4, hold nobody, so ``plain`` and ``table`` differ for K_EX only (the top node multiplies row 5 by 0.0);
    * rows: the other objects draw from the remaining rows so that no object reads its predecessor's row."""

    def __init__(self, kind, N, M, jex, seed):
        rs = np.random.RandomState(seed)
        self.kind, self.N, self.M = kind, N, M
        val = rs.dirichlet(np.full(max(M, 2), ALPHA), size=P)[:, :M].copy()
        if kind == 'rows':
            with np.errstate(divide='ignore'):
                self.plain = np.log(val)
            self.table = self.plain.copy(); self.table[ROW_EX, jex] = -np.inf
            fixed = {0: P - 1, N - 1: 0, K_EX: ROW_EX}
            draw = rs.randint(0, 1 << 30, N)
            rows = np.empty(N, dtype=np.int64)
            for i in range(N):
                if i in fixed:
                    rows[i] = fixed[i]; continue
                bad = {ROW_EX, rows[i - 1] if i else -1, fixed.get(i + 1, -1), 0 if i == K_LAST else -1}
                free = [r for r in range(P) if r not in bad]
                rows[i] = free[draw[i] % len(free)]
            assert (rows != np.roll(rows, 1)).all()
            self.rows = rows.astype(np.int64)
            assert (self.rows == ROW_EX).sum() == 1 and self.rows[K_LAST] != 0
        else:
            val[0] = 0.; val[1] = 0.
            self.plain = val
            self.table = val.copy(); self.table[ROW_EX + 1, jex] = 0.; self.table[ROW_EX + 2, jex] = 0.
            coord = rs.uniform(GRID7[1], GRID7[3], N)
            coord[0], coord[N - 1], coord[K_NODE] = GRID7[-1] + 1., -0.4, GRID7[2]
            coord[K_EX] = 0.5 * (GRID7[ROW_EX + 1] + GRID7[ROW_EX + 2])
            self.coord = coord

    def dense(self, idx, plain=False):
        """(len(idx), M) ln-prior of the objects ``idx``, formed in NumPy"""
        from frankenz_amd.pdf import lerp_cells
        tab = self.plain if plain else self.table
        idx = np.asarray(idx)
        if self.kind == 'rows':
            return tab[self.rows[idx]]
        r, f = lerp_cells(GRID7, self.coord[idx])
        with np.errstate(divide='ignore'):
            return np.log((1. - f)[:, None] * tab[r] + f[:, None] * tab[r + 1])

    def hook(self, idx=None, plain=False):
        """the public ``lprob_func`` for the objects ``idx`` (all of them: None), in that order"""
        from frankenz_amd.pdf import logprob_prior, logprob_prior_lerp
        tab = self.plain if plain else self.table
        sel = slice(None) if idx is None else np.asarray(idx)
        if self.kind == 'rows':
            return logprob_prior(tab, self.rows[sel])
        return logprob_prior_lerp(tab, GRID7, self.coord[sel])


@functools.lru_cache(maxsize=8)
def prior(kind, B, variant, N, M, T):
    return Prior(kind, N, M, tuple(excluded(M, T)), _seed('prior', kind, B, variant, N, M, T))


# ---- oracle runs ---------------------------------------------------------------------------------------------------------------------------
def oracle_rows(pr, idx, mode, lp):
    """fo.bruteforce_fit_predict of the objects ``idx`` with the dense ln-prior ``lp``: (pdfs, lmap, levid)"""
    with np.errstate(all='ignore'):
        return fo.bruteforce_fit_predict(pr['X'][idx].copy(), pr['Xe'][idx].copy(), pr['Xm'][idx].copy(), pr['Y'], pr['Ye'], pr['Ym'],
                                         pr['z'], pr['ze'], label_dict=oracle_dict(), lnprior=lp, **MODES[mode])


def oracle_planes(pr, idx, mode):
    """per-object fo.logprob: (lnlike, Ndim) planes of the objects ``idx``"""
    lnl, ndim = np.empty((len(idx), pr['M'])), np.empty((len(idx), pr['M']), dtype=np.int64)
    with np.errstate(all='ignore'):
        for k, i in enumerate(idx):
            r = fo.logprob(pr['X'][i].copy(), pr['Xe'][i].copy(), pr['Xm'][i].copy(), pr['Y'], pr['Ye'], pr['Ym'], **MODES[mode])
            lnl[k], ndim[k] = r[1], r[3]
    return lnl, ndim


def undefined_pairs(ndim, mode):
    """one usable band + free scale + dimensionality prior: nan or -inf by rounding luck in the reference itself (the rule of
    test_oracle_parity_band_counts); reachable at B = 3 only (Ndim >= B - 2)"""
    kw = MODES[mode]
    if kw.get('free_scale') and kw.get('dim_prior', True):
        return ndim == 1
    return np.zeros_like(ndim, dtype=bool)


@functools.lru_cache(maxsize=8)
def planes(B, variant, N, M, T, mode, idx):
    """(indices, lnlike, Ndim) of the objects ``idx`` (a tuple; None: all): the prior does not enter"""
    ix = np.arange(N) if idx is None else np.array(idx)
    return (ix,) + oracle_planes(problem(B, variant, N, M, T), ix, mode)


@functools.lru_cache(maxsize=8)
def reference(kind, B, variant, N, M, T, mode, idx):
    """everything the GPU tests compare against, for the objects ``idx`` (a tuple; None: all)"""
    pr, pri = problem(B, variant, N, M, T), prior(kind, B, variant, N, M, T)
    ix, lnl, ndim = planes(B, variant, N, M, T, mode, idx)
    lp = pri.dense(ix)
    p, lm, le = oracle_rows(pr, ix, mode, lp)
    return dict(idx=ix, lp=lp, lnl=lnl, ndim=ndim, undef=undefined_pairs(ndim, mode), pdfs=p, lmap=lm, levid=le)


def differs(a, b, tol):
    """|a - b| beyond ten times ``tol`` (a value that stopped being finite differs)"""
    with np.errstate(invalid='ignore'):
        return ~(np.abs(a - b) <= 10. * (tol['atol'] + tol['rtol'] * np.abs(b)))


def oracle_levid(lnl, lp):
    """the ln-evidence of fo.bruteforce_fit_predict without its PDFs: ``logsumexp(lnlike + lnprior)`` per object with the oracle's
    own logsumexp (tests/test_prior_bands_host.py holds the two equal, bit for bit, on a sample of the cases)"""
    with np.errstate(all='ignore'):
        return np.array([logsumexp(a + b) for a, b in zip(lnl, lp)])


def sensitivity(kind, B, variant, N, M, T, mode, idx):
    """What makes a wrong prior row and an off-by-one model index visible: the oracle's ln-evidence with (a) every object given
    its predecessor's prior and (b) every model its predecessor's entry, against the right one.  Returns the share of the finite
    rows that move by more than ten times the comparison tolerance under (a) and under (b), the finite share of the compared rows
    (those without an undefined pair), the right
    ln-evidence, and for K_EX whether its best-fit model is one the prior excludes and whether every excluded model weighs at
    least 1e-2 of that best in its likelihood.  Dirichlet rows of concentration ALPHA = 0.5 spread a row's entries over orders of
    magnitude (a share ~ sqrt(x) of them lies below x times the mean), so neither shift leaves a sum of M weighted terms in
    place; a concentration of 50 or more would (entries within 15 % of each other)."""
    pr, pri = problem(B, variant, N, M, T), prior(kind, B, variant, N, M, T)
    ix, lnl, ndim = planes(B, variant, N, M, T, mode, idx)
    lp = pri.dense(ix)
    right = oracle_levid(lnl, lp)
    keep = ~undefined_pairs(ndim, mode).any(axis=1)               # the rows the GPU tests compare
    fin = np.isfinite(right) & keep
    sa = differs(oracle_levid(lnl, pri.dense((ix - 1) % N)), right, GOF_TOL)[fin].mean()
    sb = differs(oracle_levid(lnl, np.roll(lp, 1, axis=1)), right, GOF_TOL)[fin].mean()
    row = lnl[int(np.nonzero(ix == K_EX)[0][0])]
    best = int(np.nanargmax(row))
    with np.errstate(all='ignore'):
        weighs = bool((row[pr['jex']] - row[best] > np.log(1e-2)).all())
    return sa, sb, fin.sum() / keep.sum(), right, best in pr['jex'], weighs


# ---- the case lists ----------------------------------------------------------------------------------------------------------------------
SMALL_N = 37
BANDS_SMALL = (3, 4, 5, 6, 7, 8, 10, 12, 16, 20, 24, 32)
BANDS_LARGE = (4, 5, 6, 7, 8, 12, 16)
LARGE_N = 16391                                              # 4 * 4097 + 3 = 2 * 8195 + 1: a short last wave group in both geometries


def variants(B):
    return ('fast', 'masked', 'safe') if 4 <= B <= 8 else ('masked', 'safe')


def small_cases():
    """(B, variant, M, mode, kind): M = TILE + 1 of the (1, 4) geometry, plus M = 1 at 32 bands"""
    out = []
    for B in BANDS_SMALL:
        for variant in variants(B):
            for mode in ('A', 'Ai', 'B', 'A_nodim'):
                for kind in KINDS:
                    out.append((B, variant, tile(unit(B), mode) + 1, mode, kind))
    out += [(32, 'masked', 1, 'A', 'rows'), (5, 'fast', 1, 'B', 'lerp')]
    return out


def small_idx(M):
    """the objects of the SMALL_N-object run out of the twopass_objects(M)-object problem: the first 36 and the last"""
    return tuple(range(SMALL_N - 1)) + (twopass_objects(M) - 1,)


def large_cases():
    """(B, variant, M, mode, kind): M = tile length + 1 of the chunk's geometry, plus one case per geometry at twice the tile"""
    out, seen = [], {}
    for B in BANDS_LARGE:
        for variant in [v for v in variants(B) if v != 'safe']:
            for mode in ('A', 'Ai', 'B'):
                geo = large_geometry(unit(B), mode, variant)
                for kind in KINDS:
                    out.append((B, variant, geo[2] + 1, mode, kind))
                if variant == 'masked':
                    seen.setdefault(geo, (B, variant, 2 * geo[2], mode, KINDS[len(seen) % 2]))
    return out + list(seen.values())


def large_idx(B, variant, M, mode):
    """the objects the oracle runs: the first 8, the last 8 (they hold the last object of the last full 4-object and 2-object
    wave groups, N - 4 and N - 2, and the short last groups, N - 3 .. N - 1 and N - 1) and 48 seeded others"""
    N = LARGE_N
    assert N % 4 == 3 and N % 2 == 1
    rs = np.random.RandomState(_seed('sample', B, variant, M, mode))
    return tuple(range(8)) + tuple(sorted(8 + rs.choice(N - 16, 48, replace=False))) + tuple(range(N - 8, N))


def modec_cases():
    """(B, variant, M, mode, kind): the materialised-rows route (k_prior_add) of mode C, SMALL_N objects"""
    return [(B, 'masked', 65, 'C', kind) for B in (4, 8, 12, 32) for kind in KINDS]
