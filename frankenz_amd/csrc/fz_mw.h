// Hierarchical re-weighting of the training set (docs/model_weights.md; the law of the reference's hierarchical_sampler,
// samplers.py:311-535, over the MODEL set instead of a label grid): one Gibbs sweep is
//
//   k_mw_sweep<WPO, REG>   per object the row t_ij = r_ij + lnw[nbr_ij] (one fp64 add) and ONE draw from it, which is k_draw's draw on that
//                     row (fz_draw.h: the same segments, the same draw_segment, the same stage A / stage B, the same geometry by the
//                     row length); counts[j] += 1 by one lane per object, optionally assign[i] = j (-1: no posterior, not counted)
//   k_mw_gamma        g_j ~ Gamma(alpha_j + counts_j, 1), one thread per model, and the block partials of sum(g) in index order
//   k_mw_gsum         the partials in index order by one block (nz_sum_partials); a sum of 0 (every draw underflowed) fails the call
//   k_mw_norm         pos = g / sum(g), lnw = log(g) - log(sum(g))   (g = 0: pos = 0, lnw = -inf)
//
// Every neighbour index is checked against [0, M) BEFORE the gather: one outside sets MW_ERR_NBR, reads nothing (its entry counts as
// -inf) and the call fails; the object is not counted.
//
// Random numbers are Philox4x32-10 (fz_philox.h), a pure function of (key, counter):
//   the sweep's uniform of object i    key (k0, k1),                  counter (i lo, i hi, sweep lo, sweep hi)    [philox_uniform]
//   the gamma draw of model j          key (k0, k1 ^ FZ_MW_KEY_XOR),  counter (j, slot, sweep lo, sweep hi)
//        slot 2 a      attempt a's normal: u1 = 1 - U(words 0, 1) in (0, 1], u2 = U(words 2, 3); x = sqrt(-2 ln u1) cos(2 pi u2)
//        slot 2 a + 1  attempt a's acceptance uniform 1 - U(words 0, 1)
//        slot 128      the uniform of the shape + 1 boost (shape < 1)
// U(a, b) = ((a >> 5) 2^26 + (b >> 6)) / 2^53 as everywhere.  samplers._philox_gamma is the NumPy twin.
#pragma once
#include "fz_draw.h"
#include "fz_nzmc.h"

#define FZ_MW_REG_SEGS 4                   // segments of a row the register form holds
#define FZ_MW_REG_LMAX (FZ_MW_REG_SEGS * FZ_DRAW_SEG)
#define FZ_MW_TRIES 64                     // attempts of the gamma rejection loop before the call fails
#define FZ_MW_KEY_XOR 0x6D775F67u          // second key word of the gamma draws: k1 ^ this ("mw_g")
#define FZ_MW_BOOST_SLOT 128u
                                           // error bits 1 and 2: FZ_MW_ERR_NNB, FZ_MW_ERR_NBR of every row kernel (fz_rows.h)
#define FZ_MW_ERR_TRIES 4                 // the rejection loop ran out
#define FZ_MW_ERR_ALPHA 8                  // alpha_j <= 0 or not finite
#define FZ_MW_ERR_ZERO 16                  // every gamma draw underflowed: sum(g) == 0, no weights to normalise

namespace fz {

// draw_load with the gathered add: the four entries of lane `lane` in segment k of the row r + lnw[nb] (nb == nullptr: entry j is
// model j), -inf past the end
__device__ __forceinline__ void mw_load(const double* __restrict__ in, const int64_t* __restrict__ nb, const double* __restrict__ lnw, int64_t M,
                                        int64_t n, int k, int lane, double (&r)[4], bool& bad) {
    const int64_t j0 = (int64_t)k * FZ_DRAW_SEG + 4 * lane;
    int64_t m[4];
    double v[4];
    if (j0 + 4 <= n) {
#pragma unroll
        for (int t = 0; t < 4; ++t) { m[t] = nb ? nb[j0 + t] : j0 + t; v[t] = in[j0 + t]; }
    } else {
#pragma unroll
        for (int t = 0; t < 4; ++t) { const bool on = j0 + t < n; m[t] = on ? (nb ? nb[j0 + t] : j0 + t) : 0; v[t] = on ? in[j0 + t] : -INFINITY; }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const bool in_row = j0 + t < n, in_set = m[t] >= 0 && m[t] < M;
        bad |= in_row && !in_set;
        r[t] = (in_row && in_set) ? v[t] + lnw[m[t]] : -INFINITY;
    }
}

// Stage A of k_mw_sweep and k_mw_em_rows: k_draw's, on the gathered row in / nb of n counted entries (nseg segments), from the loads
// to the f_k scaling and its barrier.  On return fk[k] = f_k and Pk[k] = S_k f_k for the object's segments; m: the row's max; R: the
// register form's copy of the gathered row (REG), which the sweep's stage B draws from.  sm: the block's dynamic LDS (its header takes
// the waves' flags).  Returns ok: the object is live, no nan, no index that was refused, and the max is finite.
// REG (WPO == 1, L <= FZ_MW_REG_LMAX: every default k-NN row): the wave keeps the whole gathered row, at most four segments, in
// registers.  All of its loads are issued at once -- the indices, then the gathers -- instead of segment by segment.
template <int WPO, bool REG>
__device__ __forceinline__ bool mw_stage_a(const RowGeom<WPO>& g, const double* __restrict__ in, const int64_t* __restrict__ nb,
                                           const double* __restrict__ lnw, int64_t M, int64_t n, int nseg, double* sm, double* fk, double* Pk,
                                           int* __restrict__ errflag, double (&R)[REG ? FZ_MW_REG_SEGS : 1][4], double& m) {
    const int lane = g.lane, wave = g.wave, obj = g.obj, sub = g.sub;
    bool isnan = false, bad = false;
    if constexpr (REG) {
        static_assert(!REG || WPO == 1, "the register form is one wave per object");
        int64_t mm[FZ_MW_REG_SEGS][4];
#pragma unroll
        for (int s = 0; s < FZ_MW_REG_SEGS; ++s) {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int64_t j = (int64_t)s * FZ_DRAW_SEG + 4 * lane + t;
                const bool on = j < n;
                mm[s][t] = on ? (nb ? nb[j] : j) : 0;
                R[s][t] = on ? in[j] : -INFINITY;
            }
        }
#pragma unroll
        for (int s = 0; s < FZ_MW_REG_SEGS; ++s) {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const bool on = (int64_t)s * FZ_DRAW_SEG + 4 * lane + t < n, in_set = mm[s][t] >= 0 && mm[s][t] < M;
                bad |= on && !in_set;
                R[s][t] = (on && in_set) ? R[s][t] + lnw[mm[s][t]] : -INFINITY;
            }
        }
#pragma unroll
        for (int s = 0; s < FZ_MW_REG_SEGS; ++s) {
            if (s < nseg) {                                          // (uniform over the wave)
                double e[4], p[4], x, mk;
                isnan |= (R[s][0] != R[s][0]) | (R[s][1] != R[s][1]) | (R[s][2] != R[s][2]) | (R[s][3] != R[s][3]);
                draw_segment(R[s], lane, e, p, x, mk);
                if (lane == 63) { fk[s] = mk; Pk[s] = x + p[3]; }
            }
        }
    } else {
        double r[4], rn[4], e[4], p[4], x, mk;
        if (sub < nseg) mw_load(in, nb, lnw, M, n, sub, lane, r, bad);
        for (int k = sub; k < nseg; k += WPO) {
            const bool more = k + WPO < nseg;
            if (more) mw_load(in, nb, lnw, M, n, k + WPO, lane, rn, bad);
            isnan |= (r[0] != r[0]) | (r[1] != r[1]) | (r[2] != r[2]) | (r[3] != r[3]);
            draw_segment(r, lane, e, p, x, mk);
            if (lane == 63) { fk[k] = mk; Pk[k] = x + p[3]; }
            if (more) {
#pragma unroll
                for (int t = 0; t < 4; ++t) r[t] = rn[t];
            }
        }
    }
    const bool wnan = __any(isnan), wbad = __any(bad);
    if (lane == 0) {
        sm[wave] = (wnan ? 1.0 : 0.0) + (wbad ? 2.0 : 0.0);
        if (wbad) atomicOr(errflag, FZ_MW_ERR_NBR);
    }
    __syncthreads();
    m = -INFINITY;
    for (int k = lane; k < nseg; k += 64) m = fmax(m, fk[k]);
    m = wave_max(m);
    bool unfit = false;                                              // a nan, or an index that was refused
#pragma unroll
    for (int w = 0; w < WPO; ++w) unfit |= sm[obj * WPO + w] != 0.0;
    __syncthreads();
    for (int k = sub * 64 + lane; k < nseg; k += WPO * 64) {
        const double f = exp(fk[k] - m);
        fk[k] = f; Pk[k] = Pk[k] * f;
    }
    __syncthreads();
    return g.live && !unfit && (m - m == 0.0);
}

// rows (N, L); nbr (N, L) / nnb (N) or both nullptr (dense rows: L == M, checked by the host); lnw (M); u (N) or nullptr: Philox under
// (k0, k1) at the counter (first + i, sweep); counts (M), zeroed by the caller; assign (N) or nullptr.
// Dynamic LDS as k_draw: FZ_DRAW_HDR + (4 / WPO) * 2 * nsegL doubles.
// REG: stage B re-reads nothing: it calls draw_segment on the register copy of the hit segment, the values stage A saw, so the draw is
// the same function of (row, u) as without REG (FZ_MW_REG=0 forces that form: the tests compare them).
template <int WPO, bool REG>
static __global__ __launch_bounds__(256) void k_mw_sweep(const double* __restrict__ rows, int64_t N, int64_t L, const int64_t* __restrict__ nbr,
                                                         const int64_t* __restrict__ nnb, int64_t M, const double* __restrict__ lnw,
                                                         const double* __restrict__ u, uint32_t k0, uint32_t k1, int64_t first, uint64_t sweep,
                                                         unsigned long long* __restrict__ counts, int64_t* __restrict__ assign,
                                                         int* __restrict__ errflag) {
    extern __shared__ double sm[];
    RowGeom<WPO> g(N);
    const int lane = g.lane, obj = g.obj, sub = g.sub;
    const int64_t i = g.i;
    const bool live = g.live;
    const int nsegL = (int)((L + FZ_DRAW_SEG - 1) / FZ_DRAW_SEG);
    double* fk = sm + FZ_DRAW_HDR + (size_t)obj * 2 * nsegL;       // m_k, then f_k
    double* Pk = fk + nsegL;                                        // S_k, then the mass, then P_k
    const int64_t n = g.counted(nnb, L, errflag, FZ_MW_ERR_NNB);
    const double* in = g.row(rows, L);
    const int64_t* nb = g.opt(nbr, L);
    const int nseg = (int)((n + FZ_DRAW_SEG - 1) / FZ_DRAW_SEG);

    // ---- stage A: k_draw's, on the gathered row ----
    double R[REG ? FZ_MW_REG_SEGS : 1][4], m;
    const bool ok = mw_stage_a<WPO, REG>(g, in, nb, lnw, M, n, nseg, sm, fk, Pk, errflag, R, m);
    if (sub == 0 && lane == 0) {
        double P = 0.0; int klast = 0;
        for (int k = 0; k < nseg; ++k) { P += Pk[k]; Pk[k] = P; if (fk[k] > 0.0) klast = k; }
        sm[4 + obj] = (double)klast;
    }
    __syncthreads();
    if (!live || sub != 0) return;
    const double tot = nseg ? Pk[nseg - 1] : 0.0;
    const int klast = (int)sm[4 + obj];

    // ---- stage B: k_draw's, one draw ----
    int64_t out = -1;
    if (ok) {
        const double uu = u ? u[i] : philox_uniform(k0, k1, (uint64_t)(first + i), sweep);
        const double tgt = uu * tot;
        int lo = 0, hi = nseg;                                       // first k with P_k > tgt (nseg: none)
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (Pk[mid] > tgt) hi = mid; else lo = mid + 1; }
        const bool top = lo == nseg;
        const int k = __builtin_amdgcn_readfirstlane(top ? klast : lo);
        double r[4], e[4], p[4], x, mk;
        if constexpr (REG) {
#pragma unroll
            for (int s = 0; s < FZ_MW_REG_SEGS; ++s) {
                if (s == k) {
#pragma unroll
                    for (int t = 0; t < 4; ++t) r[t] = R[s][t];
                }
            }
        } else {
            bool again = false;
            mw_load(in, nb, lnw, M, n, k, lane, r, again);
        }
        draw_segment(r, lane, e, p, x, mk);
        const double f = fk[k], base = k ? Pk[k - 1] : 0.0;
        int hit = -1, lastpos = -1;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const double cum = base + (x + p[t]) * f;
            if (e[t] * f > 0.0) { lastpos = t; if (hit < 0 && !top && cum > tgt) hit = t; }
        }
        const unsigned long long bh = __ballot(hit >= 0), bp = __ballot(lastpos >= 0);
        int src, slot;
        if (bh) { src = __builtin_ctzll(bh); slot = __shfl(hit, src, 64); }
        else { src = bp ? 63 - __builtin_clzll(bp) : 0; slot = __shfl(lastpos, src, 64); if (slot < 0) slot = 0; }
        const int64_t j = (int64_t)k * FZ_DRAW_SEG + 4 * src + slot;
        out = (j < n) ? (nb ? nb[j] : j) : -1;
        if (out < 0 || out >= M) out = -1;                           // (cannot happen for an entry that holds mass: it passed mw_load)
    }
    if (lane == 0) {
        if (out >= 0) atomicAdd(&counts[out], 1ull);
        if (assign) assign[i] = out;
    }
}

// ---- the Dirichlet step ----------------------------------------------------------------------------------------------------------
__device__ inline double mw_u53(uint32_t a, uint32_t b) {
    return (double)(((uint64_t)(a >> 5) << 26) | (uint64_t)(b >> 6)) * (1.0 / 9007199254740992.0);
}

// Gamma(shape, 1) of model j in sweep `sweep` (Marsaglia & Tsang 2000, without the squeeze: ONE acceptance expression, so that the
// twin takes the same decisions).  shape < 1: Gamma(shape + 1) U^(1 / shape), formed as exp(ln g + ln U / shape): U^(1 / shape) alone
// underflows for shapes of a few hundredths where the product does not.  Returns a negative value when the loop runs out.
__device__ inline double mw_gamma(double shape, uint32_t k0, uint32_t k1, uint32_t j, uint64_t sweep) {
    const uint32_t s0 = (uint32_t)sweep, s1 = (uint32_t)(sweep >> 32);
    const bool boost = shape < 1.0;
    const double a = boost ? shape + 1.0 : shape;
    const double d = a - 1.0 / 3.0, c = 1.0 / sqrt(9.0 * d);
    double g = -1.0;
    for (uint32_t att = 0; att < FZ_MW_TRIES; ++att) {
        const Philox4 o = philox4x32_10(j, 2 * att, s0, s1, k0, k1);
        const double u1 = 1.0 - mw_u53(o.v[0], o.v[1]), u2 = mw_u53(o.v[2], o.v[3]);
        const double x = sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
        const double v1 = 1.0 + c * x;
        if (v1 <= 0.0) continue;
        const double v = v1 * v1 * v1;
        const Philox4 q = philox4x32_10(j, 2 * att + 1, s0, s1, k0, k1);
        const double ua = 1.0 - mw_u53(q.v[0], q.v[1]);
        if (log(ua) < 0.5 * x * x + d - d * v + d * log(v)) { g = d * v; break; }
    }
    if (g < 0.0 || !boost) return g;
    const Philox4 o = philox4x32_10(j, FZ_MW_BOOST_SLOT, s0, s1, k0, k1);
    const double ub = 1.0 - mw_u53(o.v[0], o.v[1]);
    return exp(log(g) + log(ub) / shape);
}

// g (M); partial[b] = sum of block b's 256 draws (nz_block_sum's order)
static __global__ __launch_bounds__(NZ_NT) void k_mw_gamma(const double* __restrict__ alpha, const unsigned long long* __restrict__ counts, int64_t M,
                                                           uint32_t k0, uint32_t k1, uint64_t sweep, double* __restrict__ g,
                                                           double* __restrict__ partial, int* __restrict__ errflag) {
    __shared__ double sh[NZ_NT];
    const int64_t j = (int64_t)blockIdx.x * NZ_NT + threadIdx.x;
    double v = 0.0;
    if (j < M) {
        const double al = alpha[j];
        if (!(al > 0.0) || !(al - al == 0.0)) atomicOr(errflag, FZ_MW_ERR_ALPHA);
        else {
            v = mw_gamma(al + (double)counts[j], k0, k1 ^ FZ_MW_KEY_XOR, (uint32_t)j, sweep);
            if (v < 0.0) { v = 0.0; atomicOr(errflag, FZ_MW_ERR_TRIES); }
        }
        g[j] = v;
    }
    const double b = nz_block_sum(v, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = b;
}
// partial[nblk] = the partials in index order
static __global__ __launch_bounds__(NZ_NT) void k_mw_gsum(double* __restrict__ partial, int64_t nblk, int* __restrict__ errflag) {
    __shared__ double sh[NZ_NT];
    const double s = nz_sum_partials(partial, nblk, sh);
    if (threadIdx.x == 0) {
        partial[nblk] = s;
        if (!(s > 0.0)) atomicOr(errflag, FZ_MW_ERR_ZERO);            // pos would be 0 / 0: the call fails loudly
    }
}
// pos may be g itself
static __global__ __launch_bounds__(NZ_NT) void k_mw_norm(const double* g, int64_t M, const double* __restrict__ total, double* pos,
                                                          double* __restrict__ lnw) {
    const int64_t j = (int64_t)blockIdx.x * NZ_NT + threadIdx.x;
    if (j >= M) return;
    const double s = total[0], v = g[j];
    pos[j] = v / s;
    lnw[j] = log(v) - log(s);
}

}  // namespace fz
