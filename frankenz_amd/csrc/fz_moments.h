// Posterior moments of per-model values under rows of ln-weights, and the per-band sums of the zero-point fit (docs/predictive.md;
// extension, no reference counterpart; the law is stated in include/frankenz_hip.h).
//
//   k_row_moments<LB, WPO>  one object per group of WPO waves: the row consumers' geometry (RowGeom, fz_rows.h), a function of the row
//                      length alone.  Thread q of the object's 64 WPO owns the entries q, q + 64 WPO, ... and keeps the sums of up to
//                      LB columns in registers.  Three walks over the row: (0) row_walk0 (fz_rows.h): max, nan, and EVERY counted
//                      index against [0, M) -- nothing is gathered for a row that fails; (1) w = exp(r - m), Z, Z_l, sum w c; (2) the central sums sum w (c - mean_l)^2 and sum w (s Ve)^2, with w
//                      recomputed (the same bits) and the records re-gathered from cache.
//   k_mom_pack         the value, error and mask tables of a call -> one record per model (below)
//   k_phot_sums        block (strip, band): the sums A, B, C and the counts n, nclip of one band over a strip of NZ_CHUNK objects
//   k_phot_fin         the strip sums in index order (nz_sum_partials), one block per (quantity, band)
//
// Every sum has one fixed order, a function of the row (or of N) alone: a thread adds its entries in order, the 64 lane sums go
// through one xor butterfly (em_wave_sum: every lane ends with the same bits), and with WPO == 4 the four wave sums are added in wave
// order.  No float atomic, and the build passes -ffp-contract=off: w c is rounded before it is added.
#pragma once
#include "fz_draw.h"
#include "fz_nzmc.h"
#include "fz_mw_em.h"

#define FZ_MOM_LMAX 32                     // columns of a value table: the package's band limit
#define FZ_PHOT_NQ 5                       // A, B, C, n, nclip

namespace fz {

// `v` of every wave of the object added in wave order (WPO == 1: v itself); slot: a column of sh no other value of this round uses
template <int WPO>
__device__ __forceinline__ double mom_obj_sum(double v, double (*sh)[2 * FZ_MOM_LMAX + 2], int obj, int slot) {
    if constexpr (WPO == 1) return v;
    double s = sh[obj * WPO][slot];
#pragma unroll
    for (int w = 1; w < WPO; ++w) s += sh[obj * WPO + w][slot];
    return s;
}

// One record per model, RS doubles apart: V[j][0..L), Ve[j][0..L) (zeros without Ve), then one word whose bit l says that column l is
// usable (every bit set without Vm).  RS is a power of two up to 16 doubles, so that a record of up to 7 columns lies in ONE 128-byte
// line, and a multiple of 16 beyond: a gather touches one line where the three tables as given would touch three to six.
__host__ __device__ inline int mom_record_stride(int L) {
    const int n = 2 * L + 1;
    if (n > 16) return (n + 15) / 16 * 16;
    int rs = 1;
    while (rs < n) rs <<= 1;
    return rs;
}
static __global__ __launch_bounds__(256) void k_mom_pack(const double* __restrict__ V, const double* __restrict__ Ve, const double* __restrict__ Vm,
                                                         int64_t M, int L, int RS, double* __restrict__ rec) {
    const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (x >= M * RS) return;
    const int64_t j = x / RS;
    const int k = (int)(x - j * RS);
    double out = 0.0;
    if (k < L) out = V[j * L + k];
    else if (k < 2 * L) out = Ve ? Ve[j * L + (k - L)] : 0.0;
    else if (k == 2 * L) {
        unsigned long long bits = 0ull;
        for (int l = 0; l < L; ++l) if (!Vm || Vm[j * L + l] != 0.0) bits |= 1ull << l;
        out = __longlong_as_double((long long)bits);
    }
    rec[x] = out;
}

// rows (N, W); nbr (N, W) / nnb (N) or both nullptr (dense: W == M, entry t is model t); scale (N, W) or nullptr; rec (M, RS): the
// records of k_mom_pack; mean (N, L); var, share (N, L) or nullptr; *nskip += rows without a posterior.  L <= LB.
template <int LB, int WPO>
static __global__ __launch_bounds__(256) void k_row_moments(const double* __restrict__ rows, int64_t N, int64_t W, const int64_t* __restrict__ nbr,
                                                            const int64_t* __restrict__ nnb, const double* __restrict__ scale, int64_t M, int L,
                                                            const double* __restrict__ rec, int RS, bool has_ve,
                                                            double* __restrict__ mean, double* __restrict__ var,
                                                            double* __restrict__ share, unsigned long long* __restrict__ nskip,
                                                            int* __restrict__ errflag) {
    static_assert(LB <= FZ_MOM_LMAX, "column bucket");
    __shared__ double sh[4][2 * FZ_MOM_LMAX + 2];
    RowGeom<WPO> g(N);
    constexpr int NT = RowGeom<WPO>::NT;
    const int lane = g.lane, wave = g.wave, obj = g.obj, sub = g.sub;
    const int64_t i = g.i, t0 = g.t0();
    const bool live = g.live;
    const int64_t n = g.counted(nnb, W, errflag, FZ_MW_ERR_NNB);
    const double* r = g.row(rows, W);
    const int64_t* nb = g.opt(nbr, W);
    const double* sc = g.opt(scale, W);

    // ---- walk 0: the max, a nan, and every counted index (before anything is gathered) ----
    double m;
    const bool ok = row_walk0<WPO>(g, r, nb, n, M, sh, errflag, m);
    const int64_t ne = ok ? n : 0;                                   // a row without a posterior walks nothing below

    // ---- walk 1: Z, Z_l, sum w c ----
    double Z = 0.0, Zl[LB], S[LB];
#pragma unroll
    for (int l = 0; l < LB; ++l) { Zl[l] = 0.0; S[l] = 0.0; }
    for (int64_t t = t0; t < ne; t += NT) {
        const double w = exp(r[t] - m);
        if (!(w > 0.0)) continue;                                    // contributes nothing at all (not 0 * inf)
        const int64_t j = nb ? nb[t] : t;
        const double s = sc ? sc[t] : 1.0;
        const double* v = rec + j * RS;
        const unsigned long long usable = (unsigned long long)__double_as_longlong(v[2 * L]);
        Z += w;
#pragma unroll
        for (int l = 0; l < LB; ++l) {
            if (l < L && ((usable >> l) & 1ull)) {
                const double c = s * v[l];
                Zl[l] += w;
                S[l] += w * c;
            }
        }
    }
    Z = em_wave_sum(Z);
#pragma unroll
    for (int l = 0; l < LB; ++l) { if (l < L) { Zl[l] = em_wave_sum(Zl[l]); S[l] = em_wave_sum(S[l]); } }
    if constexpr (WPO > 1) {
        if (lane == 0) {
            sh[wave][2 * FZ_MOM_LMAX] = Z;
#pragma unroll
            for (int l = 0; l < LB; ++l) { if (l < L) { sh[wave][l] = Zl[l]; sh[wave][FZ_MOM_LMAX + l] = S[l]; } }
        }
        __syncthreads();
        Z = mom_obj_sum<WPO>(Z, sh, obj, 2 * FZ_MOM_LMAX);
#pragma unroll
        for (int l = 0; l < LB; ++l) {
            if (l < L) { Zl[l] = mom_obj_sum<WPO>(Zl[l], sh, obj, l); S[l] = mom_obj_sum<WPO>(S[l], sh, obj, FZ_MOM_LMAX + l); }
        }
        __syncthreads();
    }
    double mu[LB];
    double my_mu = (double)NAN, my_zl = 0.0;                         // lane l keeps column l's results
#pragma unroll
    for (int l = 0; l < LB; ++l) {
        mu[l] = Zl[l] > 0.0 ? S[l] / Zl[l] : (double)NAN;
        if (lane == l) { my_mu = mu[l]; my_zl = Zl[l]; }
    }
    const bool writer = live && sub == 0 && lane < L;
    if (writer) {
        mean[i * L + lane] = ok ? my_mu : (double)NAN;
        if (share) share[i * L + lane] = (ok && my_zl > 0.0) ? my_zl / Z : 0.0;
    }
    if (live && !ok && sub == 0 && lane == 0) atomicAdd(nskip, 1ull);
    if (!var) return;                                                // (uniform over the grid)

    // ---- walk 2: the central sums ----
    double Q[LB], E[LB];
#pragma unroll
    for (int l = 0; l < LB; ++l) { Q[l] = 0.0; E[l] = 0.0; }
    for (int64_t t = t0; t < ne; t += NT) {
        const double w = exp(r[t] - m);
        if (!(w > 0.0)) continue;
        const int64_t j = nb ? nb[t] : t;
        const double s = sc ? sc[t] : 1.0;
        const double* v = rec + j * RS;
        const unsigned long long usable = (unsigned long long)__double_as_longlong(v[2 * L]);
#pragma unroll
        for (int l = 0; l < LB; ++l) {
            if (l < L && ((usable >> l) & 1ull)) {
                const double c = s * v[l];
                const double d = c - mu[l];
                Q[l] += w * (d * d);
                if (has_ve) { const double se = s * v[L + l]; E[l] += w * (se * se); }
            }
        }
    }
#pragma unroll
    for (int l = 0; l < LB; ++l) { if (l < L) { Q[l] = em_wave_sum(Q[l]); E[l] = em_wave_sum(E[l]); } }
    if constexpr (WPO > 1) {
        if (lane == 0) {
#pragma unroll
            for (int l = 0; l < LB; ++l) { if (l < L) { sh[wave][l] = Q[l]; sh[wave][FZ_MOM_LMAX + l] = E[l]; } }
        }
        __syncthreads();
#pragma unroll
        for (int l = 0; l < LB; ++l) {
            if (l < L) { Q[l] = mom_obj_sum<WPO>(Q[l], sh, obj, l); E[l] = mom_obj_sum<WPO>(E[l], sh, obj, FZ_MOM_LMAX + l); }
        }
    }
    double my_q = 0.0, my_e = 0.0;
#pragma unroll
    for (int l = 0; l < LB; ++l) { if (lane == l) { my_q = Q[l]; my_e = E[l]; } }
    if (writer) {
        double vv = (double)NAN;
        if (ok && my_zl > 0.0) vv = has_ve ? my_q / my_zl + my_e / my_zl : my_q / my_zl;
        var[i * L + lane] = vv;
    }
}

// x, xe, xm, p, v: (n, B) rows of the launch's objects, whose first is object strip0 NZ_CHUNK of the call; grid (strips of the launch,
// B).  partial[(q B + b) nstrips + strip], q = 0 A, 1 B, 2 C, 3 n, 4 nclip (counts as doubles: at most NZ_CHUNK, exact).
static __global__ __launch_bounds__(NZ_NT) void k_phot_sums(const double* __restrict__ x, const double* __restrict__ xe, const double* __restrict__ xm,
                                                            const double* __restrict__ p, const double* __restrict__ v, int64_t n, int B,
                                                            double clip, int64_t strip0, int64_t nstrips, double* __restrict__ partial) {
    __shared__ double sh[NZ_NT];
    const int b = blockIdx.y;
    const int64_t base = (int64_t)blockIdx.x * NZ_CHUNK;
    const double clip2 = clip * clip;
    double sA = 0.0, sB = 0.0, sC = 0.0, cn = 0.0, cc = 0.0;
#pragma unroll
    for (int k = 0; k < NZ_CHUNK / NZ_NT; ++k) {
        const int64_t i = base + k * NZ_NT + threadIdx.x;
        if (i < n) {
            const int64_t e = i * B + b;
            const double xi = x[e], ei = xe[e], mi = xm[e], pi = p[e], vi = v[e];
            const bool fin = (xi - xi == 0.0) && (ei - ei == 0.0) && (pi - pi == 0.0) && (vi - vi == 0.0);
            if (mi != 0.0 && fin) {
                const double w = 1.0 / (ei * ei + vi), d = xi - pi;
                const double c = w * d * d;
                if (clip > 0.0 && c > clip2) cc += 1.0;
                else { sA += w * xi * pi; sB += w * pi * pi; sC += c; cn += 1.0; }
            }
        }
    }
    const double vals[FZ_PHOT_NQ] = {sA, sB, sC, cn, cc};
    const int64_t strip = strip0 + blockIdx.x;
#pragma unroll
    for (int q = 0; q < FZ_PHOT_NQ; ++q) {
        const double s = nz_block_sum(vals[q], sh);
        if (threadIdx.x == 0) partial[((int64_t)q * B + b) * nstrips + strip] = s;
    }
}
// block q B + b: sums (3, B) = A, B, C; counts (2, B) = n, nclip
static __global__ __launch_bounds__(NZ_NT) void k_phot_fin(const double* __restrict__ partial, int64_t nstrips, int B, double* __restrict__ sums,
                                                           long long* __restrict__ counts) {
    __shared__ double sh[NZ_NT];
    const double s = nz_sum_partials(partial + (int64_t)blockIdx.x * nstrips, nstrips, sh);
    if (threadIdx.x == 0) {
        if ((int)blockIdx.x < 3 * B) sums[blockIdx.x] = s;
        else counts[blockIdx.x - 3 * B] = (long long)s;
    }
}

}  // namespace fz
