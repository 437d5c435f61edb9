// Posterior bin masses and mixture CDFs of a Gaussian label kernel under rows of ln-weights (docs/bins.md; extension, no reference
// counterpart; the law is stated in include/frankenz_hip.h).
//
//   k_bins_pack             the label and error tables of a call -> one 16-byte record (y, q = 1 / (s sqrt 2)) per model; s == 0 gives
//                           q = +inf, which the row kernel reads as "step function".  A label that is not finite, or an error that is
//                           negative or nan, leaves the smallest such model in *badmodel (atomicMin on integers).
//   k_bins_check_points     a device array of CDF points: any that is not finite sets FZ_BINS_ERR_POINT
//   k_row_bins<WPO, CDF>   one object per group of WPO waves -- the row consumers' geometry (RowGeom, fz_rows.h).  Thread q
//                           of the object's 64 WPO owns the entries q, q + 64 WPO, ... and keeps the sums of up to FZ_BINS_BB bins (CDF:
//                           points) in registers; more bins take ceil(NB / FZ_BINS_BB) passes over the row, each with the weights recomputed
//                           (the same bits) and the records gathered again from cache.  Walk 0 is row_walk0 (fz_rows.h): the max, a nan, and
//                           EVERY counted index against [0, M) -- nothing is gathered for a row that fails.  An excluded entry leaves the
//                           loop before any erfc.  Within a pass the kernel CDF is carried from one edge to the next: one erfc per edge.
//
// Every sum has one fixed order, a function of the row length (and of the bin count) alone: a thread adds its entries in order, the 64
// lane sums go through one xor butterfly (em_wave_sum: every lane ends with the same bits), with WPO == 4 the four wave sums are added
// in wave order, and the normalising sum over the bins is formed by lane l over the bins l, l + 64, l + 128, l + 192 in order and one
// butterfly.  No float atomic, and the build passes -ffp-contract=off: w (F' - F) is rounded before it is added.
#pragma once
#include "fz_moments.h"

#define FZ_BINS_MAX 256                    // bins of a call, and points of a CDF call
#define FZ_BINS_BB 16                      // bins (points) of a pass: their sums live in registers.  An 8-bin instantiation ran the 8-bin
                                           // workload of docs/bins.md 2 % faster (15.2 against 15.6 ms): not kept
#define FZ_BINS_ERR_POINT 64               // a CDF point that is not finite (beside the FZ_MW_ERR_* bits of the same word)

namespace fz {

// rec[j] = (y_j, 1 / (s_j sqrt 2)); *badmodel = min(*badmodel, j) over the models the law refuses
static __global__ __launch_bounds__(256) void k_bins_pack(const double* __restrict__ y, const double* __restrict__ s, int64_t M,
                                                          double2* __restrict__ rec, unsigned long long* __restrict__ badmodel) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= M) return;
    const double yj = y[j], sj = s[j];
    if (!(yj - yj == 0.0) || !(sj >= 0.0)) atomicMin(badmodel, (unsigned long long)j);
    rec[j] = make_double2(yj, 1.0 / (sj * 1.4142135623730951));      // s == 0: +inf; s == inf: 0 (F = 1/2 everywhere, the law's limit)
}

static __global__ __launch_bounds__(256) void k_bins_check_points(const double* __restrict__ x, int64_t n, int* __restrict__ errflag) {
    bool bad = false;
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (int64_t)gridDim.x * 256) { const double v = x[k]; bad |= !(v - v == 0.0); }
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(errflag, FZ_BINS_ERR_POINT);
}

// The kernel CDF of one entry at x.  q == +inf is s == 0, a step at y: the CDF itself is right-continuous (x >= y), while a bin EDGE
// at y belongs to the bin above it (e_k <= y < e_k+1), so that the edge function is x > y.
template <bool CDF>
__device__ __forceinline__ double bins_cdf_at(double x, double y, double q) {
    const double F = 0.5 * erfc(-((x - y) * q));
    if (q == INFINITY) return (CDF ? x >= y : x > y) ? 1.0 : 0.0;
    return F;
}

// rows (N, W); nbr (N, W) / nnb (N) or both nullptr (dense: W == M, entry t is model t); rec (M): the records of k_bins_pack.
// x: the P points of object i at x + i xstride (xstride 0: shared by all objects); CDF: out (N, P) = C; else the points are the
// E = P edges, out (N, P - 1) = the bin masses, below / above (N) or nullptr.  *nskip += rows without a posterior.
template <int WPO, bool CDF>
static __global__ __launch_bounds__(256) void k_row_bins(const double* __restrict__ rows, int64_t N, int64_t W, const int64_t* __restrict__ nbr,
                                                         const int64_t* __restrict__ nnb, int64_t M, const double2* __restrict__ rec,
                                                         const double* __restrict__ x, int64_t xstride, int P, double lncut, bool normalize,
                                                         double* __restrict__ out, double* __restrict__ below, double* __restrict__ above,
                                                         unsigned long long* __restrict__ nskip, int* __restrict__ errflag) {
    constexpr int BB = FZ_BINS_BB;
    __shared__ double shw[4][BB + 3];                                // the wave sums of a pass (WPO == 4), then Z, below, above
    __shared__ double shp[4 / WPO][FZ_BINS_MAX];                     // the object's sums, bin by bin
    RowGeom<WPO> g(N);
    constexpr int NT = RowGeom<WPO>::NT;
    const int lane = g.lane, wave = g.wave, obj = g.obj, sub = g.sub;
    const int64_t i = g.i, t0 = g.t0();
    const bool live = g.live;
    const int NB = CDF ? P : P - 1;
    const int64_t n = g.counted(nnb, W, errflag, FZ_MW_ERR_NNB);
    const double* r = g.row(rows, W);
    const int64_t* nb = g.opt(nbr, W);
    const double* xp = g.row(x, xstride);

    // ---- walk 0: the max, a nan, and every counted index (before anything is gathered) ----
    double m;
    const bool ok = row_walk0<WPO>(g, r, nb, n, M, shw, errflag, m);
    const int64_t ne = ok ? n : 0;                                   // a row without a posterior walks nothing below

    // ---- the passes: BB bins (points) each ----
    double Z = 0.0, lo = 0.0, hi = 0.0;
    for (int b0 = 0; b0 < NB; b0 += BB) {
        const int nbp = NB - b0 < BB ? NB - b0 : BB;
        const bool first = b0 == 0, last = b0 + nbp == NB;
        double acc[BB];
#pragma unroll
        for (int k = 0; k < BB; ++k) acc[k] = 0.0;
        for (int64_t t = t0; t < ne; t += NT) {
            const double d = r[t] - m;
            const double w = exp(d);
            if (!(d > lncut) || !(w > 0.0)) continue;                // excluded: before any erfc
            const double2 yq = rec[nb ? nb[t] : t];
            if (first) Z += w;
            if constexpr (CDF) {
#pragma unroll
                for (int k = 0; k < BB; ++k) { if (k < nbp) acc[k] += w * bins_cdf_at<true>(xp[b0 + k], yq.x, yq.y); }
            } else {
                double F = bins_cdf_at<false>(xp[b0], yq.x, yq.y);
                if (first && below) lo += w * F;
#pragma unroll
                for (int k = 0; k < BB; ++k) {
                    if (k < nbp) {
                        const double Fn = bins_cdf_at<false>(xp[b0 + k + 1], yq.x, yq.y);
                        acc[k] += w * (Fn - F);
                        F = Fn;
                    }
                }
                if (last && above) {                                 // the upper tail by its own erfc, not 1 - F
                    const double e = xp[NB];
                    double U = 0.5 * erfc((e - yq.x) * yq.y);
                    if (yq.y == INFINITY) U = yq.x >= e ? 1.0 : 0.0;
                    hi += w * U;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < BB; ++k) { if (k < nbp) acc[k] = em_wave_sum(acc[k]); }
        if constexpr (WPO > 1) {
            if (lane == 0) {
#pragma unroll
                for (int k = 0; k < BB; ++k) { if (k < nbp) shw[wave][k] = acc[k]; }
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < BB; ++k) {
                if (k < nbp) {
                    double s = shw[obj * WPO][k];
#pragma unroll
                    for (int w = 1; w < WPO; ++w) s += shw[obj * WPO + w][k];
                    acc[k] = s;
                }
            }
        }
        double mine = 0.0;                                           // lane k keeps bin b0 + k
#pragma unroll
        for (int k = 0; k < BB; ++k) { if (lane == k) mine = acc[k]; }
        if (sub == 0 && lane < nbp) shp[obj][b0 + lane] = mine;
        __syncthreads();                                             // (also: shw is free for the next pass)
    }
    Z = em_wave_sum(Z); lo = em_wave_sum(lo); hi = em_wave_sum(hi);
    if constexpr (WPO > 1) {
        if (lane == 0) { shw[wave][BB] = Z; shw[wave][BB + 1] = lo; shw[wave][BB + 2] = hi; }
        __syncthreads();
        Z = shw[obj * WPO][BB]; lo = shw[obj * WPO][BB + 1]; hi = shw[obj * WPO][BB + 2];
#pragma unroll
        for (int w = 1; w < WPO; ++w) { Z += shw[obj * WPO + w][BB]; lo += shw[obj * WPO + w][BB + 1]; hi += shw[obj * WPO + w][BB + 2]; }
    }
    if (!live || sub != 0) return;

    // ---- the object's first wave: divide by Z, normalise over the bins, write ----
    double v[FZ_BINS_MAX / 64], tot = 0.0;
#pragma unroll
    for (int c = 0; c < FZ_BINS_MAX / 64; ++c) {
        const int k = lane + 64 * c;
        v[c] = k < NB ? shp[obj][k] / Z : 0.0;
        tot += v[c];
    }
    if (!CDF && normalize) tot = em_wave_sum(tot);
#pragma unroll
    for (int c = 0; c < FZ_BINS_MAX / 64; ++c) {
        const int k = lane + 64 * c;
        if (k < NB) out[i * NB + k] = !ok ? (double)NAN : (!CDF && normalize) ? v[c] / tot : v[c];
    }
    if (lane == 0) {
        if (below) below[i] = ok ? lo / Z : (double)NAN;
        if (above) above[i] = ok ? hi / Z : (double)NAN;
        if (!ok) atomicAdd(nskip, 1ull);
    }
}

}  // namespace fz
