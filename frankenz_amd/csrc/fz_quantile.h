// Posterior quantiles of a Gaussian label kernel under rows of ln-weights: the inverse of k_row_bins<WPO, true>'s mixture CDF
// (docs/quantiles.md; extension, no reference counterpart; the law is stated in include/frankenz_hip.h).
//
//   k_quant_pack            the label and error tables of a call -> one 32-byte record (y, q = 1 / (s sqrt 2), s, 0) per model: the
//                           (y, q) of k_bins_pack in front, s behind it for the hull and the variance.  A label that is not finite, an
//                           error that is negative, nan or inf, or an overflowing |y| + 40 s leaves the smallest such model in
//                           *badmodel (atomicMin on integers).
//   k_row_quantiles<WPO>    one object per group of WPO waves (RowGeom, fz_rows.h).  Walk 0 is row_walk0.  Two walks without erfc
//                           form Z, the hull and the mixture mean, then the mixture variance.  Then, FZ_QUANT_BB probabilities to a
//                           pass, a safeguarded Newton whose every evaluation is one walk of the row: w recomputed (the same bits),
//                           excluded entries out before any erfc, the record gathered from cache, and per probability still active
//                           F = bins_cdf_at<true> and the density term.  Lane k of every wave of the object keeps the state of the
//                           pass's probability k in its own registers and takes its step from the object's combined sums, so that
//                           the states of a pass cost the registers of one and the four waves of a long row decide alike.
//
// Barriers.  The trip count of the solve depends on the row.  With WPO == 1 four independent objects share a block and the kernel has
// no block barrier at all.  With WPO == 4 a block is one object: its four waves combine their sums through LDS once per evaluation
// (two buffers in turn, one barrier), read the same bits, take the same decisions and leave the loop together; a block without a
// posterior makes no evaluation in any wave.  FZ_QUANT_MAXIT bounds every loop.
//
// Every sum has k_row_bins' order: a thread adds its entries in order, one xor butterfly (em_wave_sum), the wave sums in wave order.
// No float atomic; -ffp-contract=off: w F is rounded before it is added.
#pragma once
#include "fz_bins.h"

#define FZ_QUANT_BB 8                      // probabilities of a pass: their sums live in registers, their states one per lane.  16 to a
                                           // pass took 247 VGPRs and 92 spilled SGPRs (1 wave per SIMD); the usual call asks for 3 or 5
#define FZ_QUANT_MAXIT 128                 // evaluations of one (row, p) at most
#define FZ_QUANT_HULL 40.0                 // the hull is y -+ 40 s: erfc(40 / sqrt 2) is 0 in fp64
#define FZ_QUANT_SLOTS 64                  // the call's counters (nskip, nfail, niter) are spread over this many 128-byte lines

namespace fz {

// rec[j] = (y_j, 1 / (s_j sqrt 2), s_j, 0); *badmodel = min(*badmodel, j) over the models the law refuses
static __global__ __launch_bounds__(256) void k_quant_pack(const double* __restrict__ y, const double* __restrict__ s, int64_t M,
                                                           double4* __restrict__ rec, unsigned long long* __restrict__ badmodel) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= M) return;
    const double yj = y[j], sj = s[j];
    const double reach = fabs(yj) + FZ_QUANT_HULL * sj;
    if (!(yj - yj == 0.0) || !(sj >= 0.0) || !(reach - reach == 0.0)) atomicMin(badmodel, (unsigned long long)j);
    rec[j] = make_double4(yj, 1.0 / (sj * 1.4142135623730951), sj, 0.0);
}

// lane k's value in every lane (k uniform): two scalar reads
__device__ __forceinline__ double quant_lane(double v, int k) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), k), __builtin_amdgcn_readlane(__double2loint(v), k));
}
__device__ __forceinline__ unsigned long long quant_wave_count(unsigned long long v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// rows (N, W); nbr (N, W) / nnb (N) or both nullptr (dense: W == M, entry t is model t); rec (M): the records of k_quant_pack;
// probs (Q), each inside (0, 1); out (N, Q).  cnt: FZ_QUANT_SLOTS lines of 16 words, word 0 += rows without a posterior, word 1 +=
// solves that ended on the cap, word 2 += evaluations.
template <int WPO>
static __global__ __launch_bounds__(256) void k_row_quantiles(const double* __restrict__ rows, int64_t N, int64_t W, const int64_t* __restrict__ nbr,
                                                              const int64_t* __restrict__ nnb, int64_t M, const double4* __restrict__ rec,
                                                              const double* __restrict__ probs, int Q, double lncut, double* __restrict__ out,
                                                              unsigned long long* __restrict__ cnt, int* __restrict__ errflag) {
    constexpr int BB = FZ_QUANT_BB;
    __shared__ double shw[4][4];                                     // walk 0 and the two walks without erfc
    __shared__ double shs[WPO > 1 ? 2 : 1][WPO > 1 ? 4 : 1][2 * BB]; // the wave sums of an evaluation, two buffers in turn (WPO == 4)
    RowGeom<WPO> g(N);
    constexpr int NT = RowGeom<WPO>::NT;
    const int lane = g.lane, wave = g.wave, obj = g.obj, sub = g.sub;
    const int64_t i = g.i, t0 = g.t0();
    const bool live = g.live;
    const int64_t n = g.counted(nnb, W, errflag, FZ_MW_ERR_NNB);
    const double* r = g.row(rows, W);
    const int64_t* nb = g.opt(nbr, W);
    const double2* yq2 = (const double2*)rec;                        // (y, q) of model j at 2 j

    // ---- walk 0: the max, a nan, and every counted index (before anything is gathered) ----
    double m;
    const bool ok = row_walk0<WPO>(g, r, nb, n, M, shw, errflag, m);
    const int64_t ne = ok ? n : 0;                                   // a row without a posterior walks nothing below

    // ---- no erfc: Z, the hull, the mean; then the variance ----
    double Z = 0.0, S1 = 0.0, a0 = INFINITY, b0 = -INFINITY;
    for (int64_t t = t0; t < ne; t += NT) {
        const double d = r[t] - m;
        const double w = exp(d);
        if (!(d > lncut) || !(w > 0.0)) continue;
        const double4 v = rec[nb ? nb[t] : t];
        Z += w;
        S1 += w * v.x;
        const double reach = FZ_QUANT_HULL * v.z;
        a0 = fmin(a0, v.x - reach);
        b0 = fmax(b0, v.x + reach);
    }
    Z = em_wave_sum(Z); S1 = em_wave_sum(S1);
    a0 = -wave_max(-a0); b0 = wave_max(b0);
    if constexpr (WPO > 1) {
        if (lane == 0) { shw[wave][0] = Z; shw[wave][1] = S1; shw[wave][2] = a0; shw[wave][3] = b0; }
        __syncthreads();
        Z = shw[obj * WPO][0]; S1 = shw[obj * WPO][1]; a0 = shw[obj * WPO][2]; b0 = shw[obj * WPO][3];
#pragma unroll
        for (int w = 1; w < WPO; ++w) {
            Z += shw[obj * WPO + w][0]; S1 += shw[obj * WPO + w][1];
            a0 = fmin(a0, shw[obj * WPO + w][2]); b0 = fmax(b0, shw[obj * WPO + w][3]);
        }
        __syncthreads();
    }
    const double mu = S1 / Z;
    double V = 0.0;
    for (int64_t t = t0; t < ne; t += NT) {
        const double d = r[t] - m;
        const double w = exp(d);
        if (!(d > lncut) || !(w > 0.0)) continue;
        const double4 v = rec[nb ? nb[t] : t];
        const double dy = v.x - mu;
        V += w * (dy * dy + v.z * v.z);
    }
    V = em_wave_sum(V);
    if constexpr (WPO > 1) {
        if (lane == 0) shw[wave][0] = V;
        __syncthreads();
        V = shw[obj * WPO][0];
#pragma unroll
        for (int w = 1; w < WPO; ++w) V += shw[obj * WPO + w][0];
    }
    const double sigma = sqrt(V / Z);
    const double u = 1.1102230246251565e-16;                         // 2^-53
    const double delta = 4.0 * u * fmax(fabs(a0), fabs(b0));
    const double tau = 4.0 * ((double)W / 64.0 + 16.0) * u;

    // ---- the solve: BB probabilities to a pass, lane k keeps probability p0 + k ----
    unsigned long long tot_it = 0ull, tot_fail = 0ull;
    int par = 0;
    for (int p0 = 0; p0 < Q; p0 += BB) {
        const int nbp = Q - p0 < BB ? Q - p0 : BB;
        const bool mine = lane < nbp;
        const double p = mine ? probs[p0 + lane] : 0.5;
        double a = a0, b = b0, fa = -p, fb = 1.0 - p, da = 0.0, db = 0.0;    // C_dev(a) < p <= C_dev(b); the hull's ends by the law
        double wprev = b0 - a0, fprev = 1.0, res = b0;
        int it = 0;
        bool done = !mine || !ok;
        // Cantelli's bracket, rounded outward; an end is trusted only once the device's C has been formed there
        const double rl = sigma * sqrt((1.0 - p) / p), rh = sigma * sqrt(p / (1.0 - p));
        const double sa = mu - rl - 1e-9 * (rl + fabs(mu)), sb = mu + rh + 1e-9 * (rh + fabs(mu));
        double x = mu + sigma * (0.6267 * log(p / (1.0 - p)));       // the logistic stand-in for the normal quantile
        if (x < sa) x = sa;
        if (x > sb) x = sb;
        if (!(x > a && x < b)) x = 0.5 * a + 0.5 * b;
        if (!done && (!(b - a > delta) || !(x > a && x < b))) done = true;   // a hull no wider than the resolution: its upper end

        unsigned long long active = __ballot(!done);
        while (active) {
            double xs[BB], aC[BB], aD[BB];
#pragma unroll
            for (int k = 0; k < BB; ++k) { xs[k] = quant_lane(x, k); aC[k] = 0.0; aD[k] = 0.0; }
            for (int64_t t = t0; t < ne; t += NT) {
                const double d = r[t] - m;
                const double w = exp(d);
                if (!(d > lncut) || !(w > 0.0)) continue;            // excluded: before any erfc
                const double2 yq = yq2[2 * (nb ? nb[t] : t)];
#pragma unroll
                for (int k = 0; k < BB; ++k) {
                    if ((active >> k) & 1ull) {                      // a probability that has stopped takes no erfc
                        const double z = (xs[k] - yq.x) * yq.y;
                        const double F = bins_cdf_at<true>(xs[k], yq.x, yq.y);
                        double e = (yq.y * exp(-(z * z))) * 0.5641895835477563;
                        if (yq.y == INFINITY) e = 0.0;               // a point mass has no density
                        aC[k] += w * F;
                        aD[k] += w * e;
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < BB; ++k) { if ((active >> k) & 1ull) { aC[k] = em_wave_sum(aC[k]); aD[k] = em_wave_sum(aD[k]); } }
            if constexpr (WPO > 1) {
                if (lane == 0) {
#pragma unroll
                    for (int k = 0; k < BB; ++k) { if ((active >> k) & 1ull) { shs[par][wave][k] = aC[k]; shs[par][wave][BB + k] = aD[k]; } }
                }
                __syncthreads();                                     // every wave of the block has this object's `active`
#pragma unroll
                for (int k = 0; k < BB; ++k) {
                    if ((active >> k) & 1ull) {
                        double sc = shs[par][0][k], sd = shs[par][0][BB + k];
#pragma unroll
                        for (int w = 1; w < WPO; ++w) { sc += shs[par][w][k]; sd += shs[par][w][BB + k]; }
                        aC[k] = sc; aD[k] = sd;
                    }
                }
                par ^= 1;
            }
            double S = 0.0, D = 0.0;                                 // lane k takes probability k's sums
#pragma unroll
            for (int k = 0; k < BB; ++k) { if (lane == k) { S = aC[k]; D = aD[k]; } }
            if (!done) {
                ++it;
                const double dn = D / Z, f = S / Z - p;
                if (f < 0.0) { a = x; fa = f; da = dn; } else { b = x; fb = f; db = dn; }
                const double wd = b - a;
                if (fabs(f) <= tau && dn > 0.0) { res = x; done = true; }    // (on a flat stretch the solve goes on to its lower end)
                else if (wd <= delta) { res = b; done = true; }
                else if (it >= FZ_QUANT_MAXIT) { res = 0.5 * a + 0.5 * b; tot_fail += 1ull; done = true; }
                else {
                    // Newton from the end of the bracket with the smaller residual (its density must be positive)
                    const bool usea = (fabs(fa) <= fabs(fb) && da > 0.0) || !(db > 0.0);
                    const double bx = usea ? a : b, bf = usea ? fa : fb, bd = usea ? da : db;
                    double xn = bx - bf / bd;
                    const bool newton = bd > 0.0 && xn > a && xn < b && (wd <= 0.5 * wprev || fabs(bf) <= 0.5 * fprev);
                    if (!newton) {                                   // bisect; a Cantelli end not yet tried stands in for the midpoint
                        const double lo = (sa > a && sa < b) ? sa : a, hi = (sb < b && sb > a) ? sb : b;
                        if (lo > a && hi < b) xn = (lo - a >= b - hi) ? lo : hi;
                        else if (lo > a) xn = lo;
                        else if (hi < b) xn = hi;
                        else xn = 0.5 * a + 0.5 * b;
                        if (!(xn > a && xn < b)) { res = b; done = true; }
                    }
                    fprev = fabs(bf); wprev = wd; x = xn;
                }
            }
            active = __ballot(!done);
        }
        if (mine && live && sub == 0) out[i * Q + p0 + lane] = ok ? res : (double)NAN;
        tot_it += (unsigned long long)it;
    }
    if (!live || sub != 0) return;
    tot_it = quant_wave_count(tot_it); tot_fail = quant_wave_count(tot_fail);
    if (lane == 0) {
        unsigned long long* c = cnt + (size_t)(blockIdx.x % FZ_QUANT_SLOTS) * 16;
        if (!ok) atomicAdd(c, 1ull);
        if (tot_fail) atomicAdd(c + 1, tot_fail);
        if (tot_it) atomicAdd(c + 2, tot_it);
    }
}

}  // namespace fz
