// Posterior draws over the model set (docs/draws.md; no reference counterpart): S draws j ~ P(j | i) = exp(r_ij - levid_i) per object
// from rows of ln-weights in device memory.
//
//   k_draw_check_u   a caller's uniforms lie in [0, 1] (nan fails)
//   k_draw<WPO>      one object per group of WPO waves (1: rows of <= FZ_DRAW_WAVE_LMAX entries, four objects per block; 4: a block
//                    per object); the row is read ONCE, every draw re-reads one 2-KB segment
//
// A draw is a fixed function of (row, u): nothing below depends on the launch geometry, the chunk or the object's place in it.
// The row is cut into SEGMENTS of 256 entries; a segment is always evaluated by one whole wave, lane l holding the four entries
// 256 k + 4 l + {0, 1, 2, 3}, by ONE function (draw_segment) that both stages call:
//     m_k  = max of the segment (nan skipped),          e_j = exp(r_j - m_k)             (the math library's fp64 exp; 0 past the row's end)
//     p_t  = e_0 + ... + e_t within the lane (in order), x_l  = the inclusive Hillis-Steele scan of p_3 over the lanes, shifted by one lane
//     cumulative weight of the segment at (l, t): x_l + p_t;  S_k = x_63 + p_3 is its last term
// Stage A keeps (m_k, S_k) per segment in LDS.  With m = max_k m_k the segment's factor is f_k = exp(m_k - m), its mass S_k f_k, and
// P_k = P_{k-1} + S_k f_k (summed in order by one lane), tot = P_last; lmap = m, levid = m + log(tot).
// Stage B, per draw: t = u tot; the segment is the first k with P_k > t (binary search: P never decreases); in it the entry is the
// first (l, t) with  P_{k-1} + (x_l + p_t) f_k > t  and  e f_k > 0.  The last of those running sums IS P_k, term for term, so a draw
// the prefix places in segment k is found there except by the rounding of the lane scan, and then (as for t >= tot) it is clamped
// to the last entry that holds mass.  The build passes -ffp-contract=off and nothing here asks for an fma: (x + p) f is rounded
// before it is added.
#pragma once
#include "fz_device.h"
#include "fz_philox.h"
#include "fz_rows.h"

#define FZ_DRAW_SEG 256                    // entries per segment: 64 lanes x 4
#define FZ_DRAW_LMAX (1 << 20)             // longest row (4096 segments: 64 KB of LDS)
#define FZ_DRAW_SMAX (1 << 16)             // most draws per object
#define FZ_DRAW_HDR 8                      // doubles in front of the segment tables: per wave {nan seen}, per object slot {last segment with mass}

namespace fz {

static __global__ void k_draw_check_u(const double* __restrict__ u, int64_t n, int* __restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && !(u[i] >= 0.0 && u[i] <= 1.0)) atomicExch(flag, 1);
}

// the four entries of lane `lane` in segment k of a row of n entries (-inf past the end)
__device__ __forceinline__ void draw_load(const double* __restrict__ in, int64_t n, int k, int lane, double (&r)[4]) {
    const int64_t j0 = (int64_t)k * FZ_DRAW_SEG + 4 * lane;
    if (j0 + 4 <= n) {
#pragma unroll
        for (int t = 0; t < 4; ++t) r[t] = in[j0 + t];
    } else {
#pragma unroll
        for (int t = 0; t < 4; ++t) r[t] = (j0 + t < n) ? in[j0 + t] : -INFINITY;
    }
}
// one segment (see above): e[t], the lane's running sums p[t], the scan of the lanes before this one, the segment's max
__device__ __forceinline__ void draw_segment(const double (&r)[4], int lane, double (&e)[4], double (&p)[4], double& x, double& mk) {
    mk = wave_max(fmax(fmax(r[0], r[1]), fmax(r[2], r[3])));
#pragma unroll
    for (int t = 0; t < 4; ++t) e[t] = (mk > -INFINITY) ? exp(r[t] - mk) : 0.0;
    p[0] = e[0]; p[1] = p[0] + e[1]; p[2] = p[1] + e[2]; p[3] = p[2] + e[3];
    double incl = p[3];
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const double v = __shfl_up(incl, d, 64); if (lane >= d) incl += v; }
    x = __shfl_up(incl, 1, 64);
    if (lane == 0) x = 0.0;
}

// rows (N, L) of ln-weights; nnb (optional): entries of row i that count, nbr (optional, (N, L)): the value returned for entry j;
// u (N, S) or nullptr: Philox under (k0, k1) at the counter (first + i, draw); idx (N, S); lmap / levid (N) or nullptr.
// Dynamic LDS: FZ_DRAW_HDR + (4 / WPO) * 2 * nsegL doubles, nsegL = segments of a row of L entries.
template <int WPO>
static __global__ __launch_bounds__(256) void k_draw(const double* __restrict__ rows, int64_t N, int64_t L, const int64_t* __restrict__ nbr,
                                                     const int64_t* __restrict__ nnb, const double* __restrict__ u, uint32_t k0, uint32_t k1,
                                                     int64_t first, int S, int64_t* __restrict__ idx, double* __restrict__ lmap,
                                                     double* __restrict__ levid, int* __restrict__ errflag) {
    extern __shared__ double sm[];
    RowGeom<WPO> g(N);
    const int lane = g.lane, wave = g.wave, obj = g.obj, sub = g.sub;
    const int64_t i = g.i;
    const bool live = g.live;
    const int nsegL = (int)((L + FZ_DRAW_SEG - 1) / FZ_DRAW_SEG);
    double* fk = sm + FZ_DRAW_HDR + (size_t)obj * 2 * nsegL;       // m_k, then f_k
    double* Pk = fk + nsegL;                                        // S_k, then the mass, then P_k
    const int64_t n = g.template counted<true>(nnb, L, errflag, 1);
    const double* in = g.row(rows, L);
    const int nseg = (int)((n + FZ_DRAW_SEG - 1) / FZ_DRAW_SEG);

    // ---- stage A: the row, once; the next segment's loads are in flight under this one's arithmetic ----
    bool isnan = false;
    {
        double r[4], rn[4], e[4], p[4], x, mk;
        if (sub < nseg) draw_load(in, n, sub, lane, r);
        for (int k = sub; k < nseg; k += WPO) {
            const bool more = k + WPO < nseg;
            if (more) draw_load(in, n, k + WPO, lane, rn);
            isnan |= (r[0] != r[0]) | (r[1] != r[1]) | (r[2] != r[2]) | (r[3] != r[3]);
            draw_segment(r, lane, e, p, x, mk);
            if (lane == 63) { fk[k] = mk; Pk[k] = x + p[3]; }
            if (more) {
#pragma unroll
                for (int t = 0; t < 4; ++t) r[t] = rn[t];
            }
        }
    }
    const bool wnan = __any(isnan);
    if (lane == 0) sm[wave] = wnan ? 1.0 : 0.0;
    __syncthreads();
    // the row's max and nan flag, formed by every wave of the object for itself
    double m = -INFINITY;
    for (int k = lane; k < nseg; k += 64) m = fmax(m, fk[k]);
    m = wave_max(m);
    bool anynan = false;
#pragma unroll
    for (int w = 0; w < WPO; ++w) anynan |= sm[obj * WPO + w] != 0.0;
    const bool ok = live && !anynan && (m - m == 0.0);
    __syncthreads();
    for (int k = sub * 64 + lane; k < nseg; k += WPO * 64) {
        const double f = exp(fk[k] - m);
        fk[k] = f; Pk[k] = Pk[k] * f;
    }
    __syncthreads();
    if (sub == 0 && lane == 0) {
        double P = 0.0; int klast = 0;
        for (int k = 0; k < nseg; ++k) { P += Pk[k]; Pk[k] = P; if (fk[k] > 0.0) klast = k; }
        sm[4 + obj] = (double)klast;
    }
    __syncthreads();
    if (!live) return;
    const double tot = nseg ? Pk[nseg - 1] : 0.0;
    const int klast = (int)sm[4 + obj];
    if (sub == 0 && lane == 0) {
        const double lm = anynan ? (double)NAN : m;
        if (lmap) lmap[i] = lm;
        if (levid) levid[i] = ok ? m + log(tot) : lm;
    }

    // ---- stage B: one wave per draw ----
    for (int s = sub; s < S; s += WPO) {
        int64_t out = -1;
        if (ok) {
            const double uu = u ? u[i * S + s] : philox_uniform(k0, k1, (uint64_t)(first + i), (uint64_t)s);
            const double tgt = uu * tot;
            int lo = 0, hi = nseg;                                   // first k with P_k > tgt (nseg: none)
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (Pk[mid] > tgt) hi = mid; else lo = mid + 1; }
            const bool top = lo == nseg;
            const int k = __builtin_amdgcn_readfirstlane(top ? klast : lo);
            double r[4], e[4], p[4], x, mk;
            draw_load(in, n, k, lane, r);
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
            out = nbr ? nbr[i * L + j] : j;
        }
        if (lane == 0) idx[i * (int64_t)S + s] = out;
    }
}

}  // namespace fz
