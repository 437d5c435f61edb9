// EM over the model weights (docs/model_weights.md, "EM"; the expectation form of fz_mw.h's Gibbs sweep, the law of the reference's
// hierarchical_sampler, samplers.py:311-535, with every entry's responsibility added where the sweep draws one and counts).  One
// iteration from weights w:
//
//   k_mw_em_rows<WPO, REG>  per object ell_i = logsumexp_k (r_ik + lnw[nbr_ik]): k_mw_sweep's stage A (mw_stage_a, fz_mw.h: the same
//                      mw_load, the same index check before the gather, the same register form and geometry) without stage B and
//                      without the uniform; nan marks a row without a posterior.  The stage is SHARED with k_mw_sweep, as one
//                      __forceinline__ function.  Against the copy it replaced, the six instantiations keep their registers (78 / 72 /
//                      74 VGPRs, no scratch, the same occupancy), their instruction counts move by -12 to +2 of 1 271 to 3 296, and
//                      their times on 1e6 rows of 500 entries stay within the copy's own spread: sweeps of k_mw_sweep<1, REG> / <1> /
//                      <4> 11.61 -> 11.63 / 15.40 -> 15.38 / 6.38 -> 6.36 ms per four, k_mw_em_rows 2.860 -> 2.857 / 3.056 -> 3.055 /
//                      1.550 -> 1.553 ms (docs/model_weights.md); the results are the same bits.
//   k_mw_em_lsum       block partials of sum(ell) over NZ_CHUNK objects each, in index order, and the count of the skipped rows.  It is
//                      a pass of its own over ell (N) so that the sum does not depend on the row pass's geometry or on the chunks a
//                      host caller's rows arrive in.
//   k_mw_em_cols       per fixed-length SEGMENT of a column of the inverted index (one wave each): sum of exp((val_e + lnw_j) - ell[obj_e])
//   k_mw_em_cols_dense dense rows: a wave takes 64 columns and walks FZ_MW_EM_RSEG rows in order
//   k_mw_em_fin        c_j = the column's segment sums in order; a_j = c_j + (alpha_j - 1); block partials of sum(a) and of the prior term
//   k_mw_em_sums       the partials in index order (nz_sum_partials): lnpost of the weights going in, sum(a); sum(a) == 0 fails the call
//   k_mw_norm          fz_mw.h's: pos = a / sum(a), lnw = log(a) - log(sum(a))
//
// No float atomic anywhere: every sum has one fixed order, a function of the inputs and of the constants below alone.  Within a
// segment lane l adds entries l, l + 64, ... in order and the 64 lane sums are added by a fixed butterfly.  exp is the device
// library's fp64 exp (1 ulp).
//
// The inverted index (col_off (M + 1) int64, col_obj (E) int32, col_val (E) float64; column j lists its counted entries in ascending
// (i, k) order with a copy of the row value) is built by a stable LSD counting sort of the counted entries by model index, 8 bits per
// pass: k_mw_em_count (validation + column lengths by integer atomics, whose result has no order), em scans, k_mw_em_gather (the
// counted entries in (i, k) order), then per pass k_mw_em_rhist (digit histogram per tile), a scan over (digit, tile) and
// k_mw_em_rscatter (one wave per tile walks it in order; the rank among equal digits within 64 entries by ballots).
#pragma once
#include "fz_mw.h"

#define FZ_MW_EM_CSEG 1024                 // entries of a column segment (a wave's job in k_mw_em_cols)
#define FZ_MW_EM_RSEG 1024                 // rows of a dense strip segment
#define FZ_MW_EM_TILE 4096                 // entries of a radix tile
#define FZ_MW_EM_SCAN 2048                 // entries of a scan block: 256 threads x 8
#define FZ_MW_ERR_ALPHA1 32                // alpha_j < 1 or not finite: no MAP

namespace fz {

// ---- the row pass --------------------------------------------------------------------------------------------------------------
// rows (N, L); nbr (N, L) / nnb (N) or both nullptr (dense: L == M); lnw (M); ell (N).  Dynamic LDS as k_mw_sweep.
template <int WPO, bool REG>
static __global__ __launch_bounds__(256) void k_mw_em_rows(const double* __restrict__ rows, int64_t N, int64_t L, const int64_t* __restrict__ nbr,
                                                           const int64_t* __restrict__ nnb, int64_t M, const double* __restrict__ lnw,
                                                           double* __restrict__ ell, int* __restrict__ errflag) {
    extern __shared__ double sm[];
    RowGeom<WPO> g(N);
    const int nsegL = (int)((L + FZ_DRAW_SEG - 1) / FZ_DRAW_SEG);
    double* fk = sm + FZ_DRAW_HDR + (size_t)g.obj * 2 * nsegL;
    double* Pk = fk + nsegL;
    const int64_t n = g.counted(nnb, L, errflag, FZ_MW_ERR_NNB);
    const int nseg = (int)((n + FZ_DRAW_SEG - 1) / FZ_DRAW_SEG);
    double R[REG ? FZ_MW_REG_SEGS : 1][4], m;
    const bool ok = mw_stage_a<WPO, REG>(g, g.row(rows, L), g.opt(nbr, L), lnw, M, n, nseg, sm, fk, Pk, errflag, R, m);
    if (g.live && g.sub == 0 && g.lane == 0) {
        double P = 0.0;
        for (int k = 0; k < nseg; ++k) P += Pk[k];
        ell[g.i] = ok ? m + log(P) : (double)NAN;
    }
}

// partial[b] = sum of ell over the counted objects of [b NZ_CHUNK, (b + 1) NZ_CHUNK); *nskip += the skipped ones (an integer atomic)
static __global__ __launch_bounds__(NZ_NT) void k_mw_em_lsum(const double* __restrict__ ell, int64_t N, double* __restrict__ partial,
                                                             unsigned long long* __restrict__ nskip) {
    __shared__ double sh[NZ_NT];
    const int64_t base = (int64_t)blockIdx.x * NZ_CHUNK;
    double s = 0.0;
    int skipped = 0;
#pragma unroll
    for (int k = 0; k < NZ_CHUNK / NZ_NT; ++k) {
        const int64_t i = base + k * NZ_NT + threadIdx.x;
        if (i < N) {
            const double l = ell[i];
            if (l == l) s += l; else ++skipped;
        }
    }
    const double b = nz_block_sum(s, sh);
    const double ns = nz_block_sum((double)skipped, sh);             // (at most 1 024: exact)
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = b;
        if (ns > 0.0) atomicAdd(nskip, (unsigned long long)ns);
    }
}

// ---- the column pass -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int64_t em_min(int64_t a, int64_t b) { return a < b ? a : b; }
__device__ __forceinline__ double em_wave_sum(double v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// seg_off (M + 1): column j owns the segments [seg_off[j], seg_off[j + 1]); at most `smax` waves are launched and those past
// seg_off[M] leave at once.  segsum (smax).
static __global__ __launch_bounds__(256) void k_mw_em_cols(const int64_t* __restrict__ col_off, const int64_t* __restrict__ seg_off, int64_t M,
                                                           int64_t E, const int32_t* __restrict__ col_obj, const double* __restrict__ col_val,
                                                           const double* __restrict__ lnw, const double* __restrict__ ell, int64_t N,
                                                           double* __restrict__ segsum, int64_t smax) {
    const int lane = threadIdx.x & 63;
    const int64_t s = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (s >= smax || s >= seg_off[M]) return;
    int64_t lo = 0, hi = M;                                          // the last j with seg_off[j] <= s
    while (hi - lo > 1) { const int64_t mid = (lo + hi) >> 1; if (seg_off[mid] <= s) lo = mid; else hi = mid; }
    const int64_t j = lo;
    const int64_t e0 = col_off[j] + (s - seg_off[j]) * FZ_MW_EM_CSEG;
    const int64_t e1 = em_min(em_min(e0 + FZ_MW_EM_CSEG, col_off[j + 1]), E);
    const double lw = lnw[j];
    double acc = 0.0;
    for (int64_t e = e0 + lane; e < e1; e += 64) {
        const int32_t o = col_obj[e];
        if (o < 0 || o >= N) continue;                               // (cannot happen for an index this library built)
        const double l = ell[o];
        if (l == l) acc += exp((col_val[e] + lw) - l);
    }
    acc = em_wave_sum(acc);
    if (lane == 0) segsum[s] = acc;
}

// dense rows (N, M): block (bx, by) is one wave; lane -> column 64 bx + lane, rows [by RSEG, (by + 1) RSEG) in order;
// segsum[j nrs + by], nrs = gridDim.y
static __global__ __launch_bounds__(64) void k_mw_em_cols_dense(const double* __restrict__ rows, int64_t N, int64_t M, const double* __restrict__ lnw,
                                                                const double* __restrict__ ell, double* __restrict__ segsum) {
    const int64_t j = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (j >= M) return;
    const int64_t i0 = (int64_t)blockIdx.y * FZ_MW_EM_RSEG, i1 = em_min(i0 + FZ_MW_EM_RSEG, N);
    const double lw = lnw[j];
    double acc = 0.0;
    for (int64_t i = i0; i < i1; ++i) {
        const double l = ell[i];
        if (l == l) acc += exp((rows[i * M + j] + lw) - l);
    }
    segsum[j * (int64_t)gridDim.y + blockIdx.y] = acc;
}

// seg_off == nullptr: dense, column j owns [j nrs, (j + 1) nrs).  cnt (M): c; a (M); partA / partP (blocks of NZ_NT models)
static __global__ __launch_bounds__(NZ_NT) void k_mw_em_fin(const int64_t* __restrict__ seg_off, int64_t nrs, const double* __restrict__ segsum,
                                                            const double* __restrict__ alpha, const double* __restrict__ lnw, int64_t M,
                                                            double* __restrict__ cnt, double* __restrict__ a, double* __restrict__ partA,
                                                            double* __restrict__ partP, int* __restrict__ errflag) {
    __shared__ double sh[NZ_NT];
    const int64_t j = (int64_t)blockIdx.x * NZ_NT + threadIdx.x;
    double v = 0.0, pr = 0.0;
    if (j < M) {
        const int64_t s0 = seg_off ? seg_off[j] : j * nrs, s1 = seg_off ? seg_off[j + 1] : (j + 1) * nrs;
        double c = 0.0;
        for (int64_t s = s0; s < s1; ++s) c += segsum[s];
        cnt[j] = c;
        const double al = alpha[j];
        if (!(al >= 1.0) || !(al - al == 0.0)) atomicOr(errflag, FZ_MW_ERR_ALPHA1);
        else {
            v = c + (al - 1.0);
            if (al != 1.0) pr = (al - 1.0) * lnw[j];
        }
        a[j] = v;
    }
    const double bA = nz_block_sum(v, sh), bP = nz_block_sum(pr, sh);
    if (threadIdx.x == 0) { partA[blockIdx.x] = bA; partP[blockIdx.x] = bP; }
}

// lnpost[0] = sum(partL) [+ sum(partP)]; partA given: total[0] = sum(partA), which must be positive
static __global__ __launch_bounds__(NZ_NT) void k_mw_em_sums(const double* __restrict__ partL, int64_t nblkL, const double* __restrict__ partA,
                                                             const double* __restrict__ partP, int64_t nblkM, double* __restrict__ lnpost,
                                                             double* __restrict__ total, int* __restrict__ errflag) {
    __shared__ double sh[NZ_NT];
    const double sL = nz_sum_partials(partL, nblkL, sh);
    if (!partA) { if (threadIdx.x == 0) lnpost[0] = sL; return; }
    const double sA = nz_sum_partials(partA, nblkM, sh), sP = nz_sum_partials(partP, nblkM, sh);
    if (threadIdx.x == 0) {
        lnpost[0] = sL + sP;
        total[0] = sA;
        if (!(sA > 0.0)) atomicOr(errflag, FZ_MW_ERR_ZERO);
    }
}

// ---- the inverted index --------------------------------------------------------------------------------------------------------
// exclusive scan of int64: out[k] = in[0] + ... + in[k - 1], out[n] = the total (out may be in)
static __global__ __launch_bounds__(256) void k_mw_em_scan_part(const int64_t* __restrict__ in, int64_t n, int64_t* __restrict__ part) {
    __shared__ long long sh[256];
    const int64_t b0 = (int64_t)blockIdx.x * FZ_MW_EM_SCAN + 8 * threadIdx.x;
    long long s = 0;
#pragma unroll
    for (int t = 0; t < 8; ++t) if (b0 + t < n) s += in[b0 + t];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) { if ((int)threadIdx.x < d) sh[threadIdx.x] += sh[threadIdx.x + d]; __syncthreads(); }
    if (threadIdx.x == 0) part[blockIdx.x] = sh[0];
}
// part (nb) -> its exclusive scan, in place, by one block: thread t owns a run of ceil(nb / 256) partials
static __global__ __launch_bounds__(256) void k_mw_em_scan_top(int64_t* __restrict__ part, int64_t nb) {
    __shared__ long long sh[256];
    const int64_t run = (nb + 255) / 256, k0 = run * threadIdx.x, k1 = em_min(k0 + run, nb);
    long long s = 0;
    for (int64_t k = k0; k < k1; ++k) s += part[k];
    sh[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) { long long acc = 0; for (int t = 0; t < 256; ++t) { const long long v = sh[t]; sh[t] = acc; acc += v; } }
    __syncthreads();
    long long acc = sh[threadIdx.x];
    for (int64_t k = k0; k < k1; ++k) { const long long v = part[k]; part[k] = acc; acc += v; }
}
static __global__ __launch_bounds__(256) void k_mw_em_scan_apply(const int64_t* in, int64_t n, const int64_t* __restrict__ part, int64_t* out) {
    __shared__ long long sh[256];
    const int64_t b0 = (int64_t)blockIdx.x * FZ_MW_EM_SCAN + 8 * threadIdx.x;
    long long v[8], s = 0;
#pragma unroll
    for (int t = 0; t < 8; ++t) { v[t] = b0 + t < n ? in[b0 + t] : 0; s += v[t]; }
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const long long u = (int)threadIdx.x >= d ? sh[threadIdx.x - d] : 0;
        __syncthreads();
        sh[threadIdx.x] += u;
        __syncthreads();
    }
    long long acc = part[blockIdx.x] + sh[threadIdx.x] - s;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        if (b0 + t < n) out[b0 + t] = acc;
        acc += v[t];
        if (b0 + t == n - 1) out[n] = acc;
    }
}

// one thread per entry of the (N, W) tables: Nneighbors and the counted neighbour indices are checked (nothing is read through one
// that fails); cnt[j] += 1 per counted entry of model j
static __global__ __launch_bounds__(256) void k_mw_em_count(const int64_t* __restrict__ nbr, const int64_t* __restrict__ nnb, int64_t N, int64_t W,
                                                            int64_t M, unsigned long long* __restrict__ cnt, int* __restrict__ errflag) {
    const int64_t tot = N * W;
    for (int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x; x < tot; x += (int64_t)gridDim.x * 256) {
        const int64_t i = x / W, k = x - i * W, n = nnb[i];
        if (n < 0 || n > W) { if (k == 0) atomicOr(errflag, FZ_MW_ERR_NNB); continue; }
        if (k >= n) continue;
        const int64_t m = nbr[x];
        if (m < 0 || m >= M) { atomicOr(errflag, FZ_MW_ERR_NBR); continue; }
        atomicAdd(&cnt[m], 1ull);
    }
}
// ns[j] = segments of column j
static __global__ __launch_bounds__(256) void k_mw_em_nseg(const int64_t* __restrict__ col_off, int64_t M, int64_t* __restrict__ ns) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j < M) ns[j] = (col_off[j + 1] - col_off[j] + FZ_MW_EM_CSEG - 1) / FZ_MW_EM_CSEG;
}
// the counted entries in (i, k) order: entry (i, k) goes to rowstart[i] + k  (the tables have passed k_mw_em_count)
static __global__ __launch_bounds__(256) void k_mw_em_gather(const double* __restrict__ rows, const int64_t* __restrict__ nbr,
                                                             const int64_t* __restrict__ nnb, const int64_t* __restrict__ rowstart, int64_t N,
                                                             int64_t W, int64_t E, int32_t* __restrict__ key, int32_t* __restrict__ obj,
                                                             double* __restrict__ val) {
    const int64_t tot = N * W;
    for (int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x; x < tot; x += (int64_t)gridDim.x * 256) {
        const int64_t i = x / W, k = x - i * W;
        if (k >= nnb[i]) continue;
        const int64_t p = rowstart[i] + k;
        if (p < 0 || p >= E) continue;
        key[p] = (int32_t)nbr[x]; obj[p] = (int32_t)i; val[p] = rows[x];
    }
}
// hist[d nT + tile] = entries of the tile whose digit is d
static __global__ __launch_bounds__(256) void k_mw_em_rhist(const int32_t* __restrict__ key, int64_t E, int shift, int64_t nT,
                                                            int64_t* __restrict__ hist) {
    __shared__ int h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const int64_t e0 = (int64_t)blockIdx.x * FZ_MW_EM_TILE, e1 = em_min(e0 + FZ_MW_EM_TILE, E);
    for (int64_t e = e0 + threadIdx.x; e < e1; e += 256) atomicAdd(&h[(key[e] >> shift) & 255], 1);
    __syncthreads();
    hist[(int64_t)threadIdx.x * nT + blockIdx.x] = h[threadIdx.x];
}
// one wave per tile, in order: an entry goes to (scanned hist of its digit and tile) + (entries of that digit before it in the tile)
static __global__ __launch_bounds__(64) void k_mw_em_rscatter(const int32_t* __restrict__ ksrc, const int32_t* __restrict__ osrc,
                                                              const double* __restrict__ vsrc, int64_t E, int shift, const int64_t* __restrict__ hist,
                                                              int64_t nT, int32_t* __restrict__ kdst, int32_t* __restrict__ odst,
                                                              double* __restrict__ vdst) {
    __shared__ long long cur[256];
    const int lane = threadIdx.x;
    for (int d = lane; d < 256; d += 64) cur[d] = hist[(int64_t)d * nT + blockIdx.x];
    __syncthreads();
    const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
    for (int it = 0; it < FZ_MW_EM_TILE / 64; ++it) {
        const int64_t e = (int64_t)blockIdx.x * FZ_MW_EM_TILE + it * 64 + lane;
        const bool on = e < E;
        const int32_t kk = on ? ksrc[e] : 0;
        const int d = (kk >> shift) & 255;
        unsigned long long same = __ballot(on);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1;
            const unsigned long long bal = __ballot(bit);
            same &= bit ? bal : ~bal;
        }
        const int rank = __builtin_popcountll(same & below), cnt = __builtin_popcountll(same);
        const long long base = cur[d];
        __syncthreads();
        if (on) {
            const long long p = base + rank;
            if (p >= 0 && p < E) { if (kdst) kdst[p] = kk; odst[p] = osrc[e]; vdst[p] = vsrc[e]; }
            if (rank == cnt - 1) cur[d] = base + cnt;
        }
        __syncthreads();
    }
}

}  // namespace fz
