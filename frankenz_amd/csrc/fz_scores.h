// Posterior scoring rules of a Gaussian label kernel under rows of ln-weights: the ln-density at a point, the CRPS and the squared
// norm of the mixture (docs/scores.md; extension, no reference counterpart; the law is stated in include/frankenz_hip.h).
//
//   k_scores_pack         the label and error tables of a call -> one 32-byte record (y, q = 1 / (s sqrt 2), s, ln s) per model.  An error
//                         whose square is 0 in fp64 (s < 2^-537, 0 included) is stored as s = 0, q = +inf, ln s = -inf: BOTH kernels
//                         decide "point mass" on this one stored s (the stage kernel by s == 0, the pair kernel by s^2 == 0 of the
//                         same s).  A label that is not finite, or an error that is negative, nan or inf, leaves the smallest such
//                         model in *badmodel (atomicMin on integers).
//   k_scores_stage<WPO>   one object per group of WPO waves (RowGeom, fz_rows.h).  Walk 0 is row_walk0.  The next walk forms Z and the
//                         included count and compacts the included entries, in entry order, into the chunk's scratch of 24-byte
//                         records (y, s^2, w); in the same walk the points of the first pass find the max of their exponents a_t.  A
//                         third walk forms sum exp(a_t - a_max) and the first CRPS term.  More than FZ_SCORES_BB points take further
//                         passes of two walks each, the weights recomputed (the same bits).
//   k_scores_pairs<WPO>   the sums over all pairs of an object's compacted entries: tile I of 64 entries one per lane, the tiles
//                         J >= I through 1.5 KB of LDS per wave, read by broadcast; on the diagonal tile lane l takes u > l and half
//                         of its own term.  A(d, v) and G(d, v) share their exp.  v == 0 is settled by selects after the arithmetic.
//
// Every sum has one fixed order, a function of the row alone: in the stage kernel a thread adds its entries in order, the 64 lane sums go
// through one xor butterfly (em_wave_sum), with WPO == 4 the four wave sums are added in wave order.  In the pair kernel a lane adds
// its terms in (I, J, u) order, then one butterfly; with WPO == 4 the tiles I are dealt to the four waves round-robin and the wave sums
// are added in wave order.  No float atomic, and the build passes -ffp-contract=off.
#pragma once
#include "fz_quantile.h"

#define FZ_SCORES_NMAX 16384               // included entries of a row whose pair sums are asked for: 1.3e8 pairs (docs/scores.md)
#define FZ_SCORES_BB 8                     // points of a pass: a_max, sum exp and the CRPS term of each live in registers
#define FZ_SCORES_REC 3                    // doubles of a compacted record: y, s^2, w

namespace fz {

// rec[j] = (y_j, 1 / (s_j sqrt 2), s_j, ln s_j); *badmodel = min(*badmodel, j) over the models the law refuses
static __global__ __launch_bounds__(256) void k_scores_pack(const double* __restrict__ y, const double* __restrict__ s, int64_t M,
                                                            double4* __restrict__ rec, unsigned long long* __restrict__ badmodel) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= M) return;
    const double yj = y[j], sg = s[j];
    if (!(yj - yj == 0.0) || !(sg >= 0.0) || !(sg - sg == 0.0)) atomicMin(badmodel, (unsigned long long)j);
    const double sj = sg * sg == 0.0 ? 0.0 : sg;                     // the law's point-mass rule: s^2 == 0 in fp64
    rec[j] = make_double4(yj, 1.0 / (sj * 1.4142135623730951), sj, log(sj));
}

// the exponent of entry t at x: a = (r_t - m) - z^2 - ln s, z = (x - y) q.  A point mass: +inf at its label, -inf elsewhere
__device__ __forceinline__ double scores_expo(double d, double x, const double4& v) {
    const double z = (x - v.x) * v.y;
    const double a = (d - z * z) - v.w;
    if (v.z == 0.0) return x == v.x ? (double)INFINITY : -(double)INFINITY;
    return a;
}

// rows (N, W); nbr (N, W) / nnb (N) or both nullptr (dense: W == M, entry t is model t); rec (M): the records of k_scores_pack.
// x: the P points of object i at x + i xstride (xstride 0: shared by all objects).  lnpdf (N, P) or nullptr; term (N, P) or nullptr:
// the first CRPS term sum w_t A(x - y_t, s_t^2) / Z.  comp or nullptr: the compacted records of object i at comp + 3 i W.  zsum (N): Z
// (nan: no posterior); ninc (N): the included count.  nmax > 0: an object with more included entries leaves min(first + i) in *over.
// *nskip += rows without a posterior.
template <int WPO>
static __global__ __launch_bounds__(256) void k_scores_stage(const double* __restrict__ rows, int64_t N, int64_t W, const int64_t* __restrict__ nbr,
                                                             const int64_t* __restrict__ nnb, int64_t M, const double4* __restrict__ rec,
                                                             const double* __restrict__ x, int64_t xstride, int P, double lncut,
                                                             double* __restrict__ lnpdf, double* __restrict__ term, double* __restrict__ comp,
                                                             double* __restrict__ zsum, int64_t* __restrict__ ninc, int64_t nmax, int64_t first,
                                                             unsigned long long* __restrict__ over, unsigned long long* __restrict__ nskip,
                                                             int* __restrict__ errflag) {
    constexpr int BB = FZ_SCORES_BB;
    __shared__ double shw[4][2 * BB + 2];                            // walk 0; the wave maxima and sums of a pass (WPO == 4)
    __shared__ int shc[2][4];                                        // the waves' included counts of a round, two buffers in turn
    RowGeom<WPO> g(N);
    constexpr int NT = RowGeom<WPO>::NT;
    const int lane = g.lane, wave = g.wave, obj = g.obj, sub = g.sub;
    const int64_t i = g.i, t0 = g.t0();
    const bool live = g.live;
    const int64_t n = g.counted(nnb, W, errflag, FZ_MW_ERR_NNB);
    const double* r = g.row(rows, W);
    const int64_t* nb = g.opt(nbr, W);
    const double* xp = g.row(x, xstride);
    double* cp = comp ? comp + (live ? i : 0) * (FZ_SCORES_REC * W) : nullptr;
    const int NP = (lnpdf || term) ? P : 0;

    // ---- walk 0: the max, a nan, and every counted index (before anything is gathered) ----
    double m;
    const bool ok = row_walk0<WPO>(g, r, nb, n, M, shw, errflag, m);
    const int64_t ne = ok ? n : 0;                                   // a row without a posterior walks nothing below
    const int64_t rounds = (ne + NT - 1) / NT;                       // the same for every thread of the object

    double Z = 0.0;
    int64_t cnt = 0;
    int b0 = 0;
    do {
        const int nbp = NP - b0 < BB ? NP - b0 : BB;
        const bool head = b0 == 0;
        double xs[BB], amax[BB];
#pragma unroll
        for (int k = 0; k < BB; ++k) { xs[k] = k < nbp ? xp[b0 + k] : 0.0; amax[k] = -INFINITY; }

        // ---- the max of the exponents; in the first pass also Z, the count and the compaction, round by round ----
        for (int64_t k = 0; k < rounds; ++k) {
            const int64_t t = t0 + k * NT;
            double d = 0.0, w = 0.0;
            bool inc = false;
            if (t < ne) { d = r[t] - m; w = exp(d); inc = d > lncut && w > 0.0; }
            double4 v = make_double4(0.0, 0.0, 0.0, 0.0);
            if (inc) v = rec[nb ? nb[t] : t];
            if (head) {
                const unsigned long long bal = __ballot(inc);
                int before = 0, total = __popcll(bal);
                if constexpr (WPO > 1) {
                    const int par = (int)(k & 1);
                    if (lane == 0) shc[par][sub] = total;
                    __syncthreads();
                    total = 0;
#pragma unroll
                    for (int q = 0; q < WPO; ++q) { const int cq = shc[par][q]; if (q < sub) before += cq; total += cq; }
                }
                if (inc) {
                    Z += w;
                    if (cp) {
                        double* o = cp + (cnt + before + __popcll(bal & ((1ull << lane) - 1ull))) * FZ_SCORES_REC;
                        o[0] = v.x; o[1] = v.z * v.z; o[2] = w;
                    }
                }
                cnt += total;
            }
            if (inc) {
#pragma unroll
                for (int q = 0; q < BB; ++q) { if (q < nbp) amax[q] = fmax(amax[q], scores_expo(d, xs[q], v)); }
            }
        }
#pragma unroll
        for (int q = 0; q < BB; ++q) { if (q < nbp) amax[q] = wave_max(amax[q]); }
        if (head) Z = em_wave_sum(Z);
        if constexpr (WPO > 1) {
            if (lane == 0) {
#pragma unroll
                for (int q = 0; q < BB; ++q) { if (q < nbp) shw[wave][q] = amax[q]; }
                if (head) shw[wave][2 * BB] = Z;
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < BB; ++q) {
                if (q < nbp) {
                    double a = shw[0][q];
#pragma unroll
                    for (int w = 1; w < WPO; ++w) a = fmax(a, shw[w][q]);
                    amax[q] = a;
                }
            }
            if (head) { Z = shw[0][2 * BB]; for (int w = 1; w < WPO; ++w) Z += shw[w][2 * BB]; }
            __syncthreads();
        }

        // ---- sum exp(a - a_max) and the first CRPS term ----
        if (nbp > 0) {
            double accE[BB], accA[BB];
#pragma unroll
            for (int q = 0; q < BB; ++q) { accE[q] = 0.0; accA[q] = 0.0; }
            for (int64_t t = t0; t < ne; t += NT) {
                const double d = r[t] - m;
                const double w = exp(d);
                if (!(d > lncut) || !(w > 0.0)) continue;            // excluded: before any erf
                const double4 v = rec[nb ? nb[t] : t];
                const double c = v.z * 0.7978845608028654;           // sqrt(2 v / pi) = s sqrt(2 / pi)
#pragma unroll
                for (int q = 0; q < BB; ++q) {
                    if (q < nbp) {
                        const double dx = xs[q] - v.x;
                        const double z = dx * v.y;
                        const double a = scores_expo(d, xs[q], v);
                        double E = exp(a - amax[q]);
                        if (a == amax[q]) E = 1.0;                   // (also +inf - +inf and -inf - -inf)
                        double A = dx * erf(z) + c * exp(-(z * z));
                        if (v.z == 0.0) A = fabs(dx);
                        accE[q] += E;
                        accA[q] += w * A;
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < BB; ++q) { if (q < nbp) { accE[q] = em_wave_sum(accE[q]); accA[q] = em_wave_sum(accA[q]); } }
            if constexpr (WPO > 1) {
                if (lane == 0) {
#pragma unroll
                    for (int q = 0; q < BB; ++q) { if (q < nbp) { shw[wave][q] = accE[q]; shw[wave][BB + q] = accA[q]; } }
                }
                __syncthreads();
#pragma unroll
                for (int q = 0; q < BB; ++q) {
                    if (q < nbp) {
                        double e = shw[0][q], a = shw[0][BB + q];
#pragma unroll
                        for (int w = 1; w < WPO; ++w) { e += shw[w][q]; a += shw[w][BB + q]; }
                        accE[q] = e; accA[q] = a;
                    }
                }
                __syncthreads();
            }
            double am = 0.0, e = 1.0, a = 0.0;                       // lane q keeps point b0 + q
#pragma unroll
            for (int q = 0; q < BB; ++q) { if (lane == q) { am = amax[q]; e = accE[q]; a = accA[q]; } }
            if (live && sub == 0 && lane < nbp) {
                const int64_t o = i * P + b0 + lane;
                if (lnpdf) lnpdf[o] = ok ? ((am + log(e)) - log(Z)) - 0.9189385332046727 : (double)NAN;    // ln sqrt(2 pi)
                if (term) term[o] = ok ? a / Z : (double)NAN;
            }
        }
        b0 += BB;
    } while (b0 < NP);

    if (!live || sub != 0 || lane != 0) return;
    zsum[i] = ok ? Z : (double)NAN;
    ninc[i] = cnt;
    if (nmax > 0 && cnt > nmax) atomicMin(over, (unsigned long long)(first + i));
    if (!ok) atomicAdd(nskip, 1ull);
}

// comp, zsum, ninc: what k_scores_stage left for the chunk's N objects (rows of W records).  spread (N), sqnorm (N) or nullptr;
// crps (N, P) or nullptr: holds the first term and leaves with the spread subtracted.
template <int WPO>
static __global__ __launch_bounds__(256) void k_scores_pairs(const double* __restrict__ comp, const double* __restrict__ zsum,
                                                             const int64_t* __restrict__ ninc, int64_t N, int64_t W, int P,
                                                             double* __restrict__ crps, double* __restrict__ spread, double* __restrict__ sqnorm) {
    __shared__ double shy[4][64], shv[4][64], shq[4][64];            // tile J of the wave: y, s^2, w
    __shared__ double shs[4][3];
    RowGeom<WPO> g(N);
    const int lane = g.lane, wave = g.wave, sub = g.sub;
    const int64_t i = g.i;
    const double Z = g.live ? zsum[i] : (double)NAN;
    int64_t n = (g.live && Z == Z) ? ninc[i] : 0;                    // a row without a posterior pairs nothing
    if (n > W) n = W;                                                // (the stage kernel counts within the row)
    const double* cp = comp + (g.live ? i : 0) * (FZ_SCORES_REC * W);
    const int64_t T = (n + 63) >> 6;

    double sA = 0.0, sG = 0.0;
    bool zero = false;
    for (int64_t I = sub; I < T; I += WPO) {
        const int64_t ti = I * 64 + lane;
        const bool mine = ti < n;
        const double yl = mine ? cp[ti * FZ_SCORES_REC] : 0.0, vl = mine ? cp[ti * FZ_SCORES_REC + 1] : 1.0,
                     wl = mine ? cp[ti * FZ_SCORES_REC + 2] : 0.0;
        zero |= mine && vl == 0.0;
        for (int64_t J = I; J < T; ++J) {
            const int64_t tj = J * 64 + lane;
            const bool has = tj < n;
            __builtin_amdgcn_wave_barrier();                         // the wave's reads of the last tile come before these writes
            shy[wave][lane] = has ? cp[tj * FZ_SCORES_REC] : 0.0;
            shv[wave][lane] = has ? cp[tj * FZ_SCORES_REC + 1] : 1.0;
            shq[wave][lane] = has ? cp[tj * FZ_SCORES_REC + 2] : 0.0;
            __builtin_amdgcn_wave_barrier();
            const int nu = n - J * 64 < 64 ? (int)(n - J * 64) : 64;
            const bool diag = J == I;
            for (int u = 0; u < nu; ++u) {
                const double yu = shy[wave][u], vu = shv[wave][u], wu = shq[wave][u];
                double c = wl * wu;
                if (diag) c = u > lane ? c : u == lane ? 0.5 * c : 0.0;
                const double d = yl - yu, v = vl + vu;
                const double rt = sqrt(v + v);                       // sqrt(2 v)
                const double ir = 1.0 / rt;
                const double z = d * ir;
                const double e = exp(-(z * z));
                double A = d * erf(z) + (rt * 0.5641895835477563) * e;       // sqrt(2 v / pi) = sqrt(2 v) / sqrt(pi)
                double G = (e * ir) * 0.5641895835477563;                     // 1 / sqrt(2 pi v)
                if (v == 0.0) { A = fabs(d); G = 0.0; }              // point masses: |d|; their +inf goes through `zero`
                sA += c * A;
                sG += c * G;
            }
        }
    }
    sA = em_wave_sum(sA); sG = em_wave_sum(sG);
    zero = __any(zero);
    if constexpr (WPO > 1) {
        if (lane == 0) { shs[wave][0] = sA; shs[wave][1] = sG; shs[wave][2] = zero ? 1.0 : 0.0; }
        __syncthreads();
        sA = shs[0][0]; sG = shs[0][1]; zero = shs[0][2] != 0.0;
#pragma unroll
        for (int w = 1; w < WPO; ++w) { sA += shs[w][0]; sG += shs[w][1]; zero |= shs[w][2] != 0.0; }
    }
    if (!g.live || sub != 0) return;
    const double sp = (sA / Z) / Z;                                  // Z nan: nan
    if (crps) for (int k = lane; k < P; k += 64) crps[i * P + k] = crps[i * P + k] - sp;
    if (lane == 0) {
        if (spread) spread[i] = sp;
        if (sqnorm) sqnorm[i] = Z != Z ? (double)NAN : zero ? (double)INFINITY : ((sG + sG) / Z) / Z;
    }
}

}  // namespace fz
