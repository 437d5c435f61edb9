// Sparse rows out of a brute-force fit (docs/sparse_fits.md; no reference counterpart): per object the exact W entries of largest
// ln-weight among those within `lncut` of the row's maximum, in the k-NN layout (neighbors, Nneighbors, padded rows).
//
//   k_sparse_select<NW>   one object per block of NW waves (1: rows of <= FZ_DRAW_WAVE_LMAX entries; 4: longer rows); the row is read twice
//   k_sparse_gather       a plane's values at the kept entries, padded
//
// The law, for a row r[0..L):  a nan, or a maximum that is not finite: nothing is kept.  Else m = max r, entry j is eligible iff
// r_j - m > lncut (one IEEE subtraction, a strict comparison), and kept are the first min(W, E) eligible entries in the order
// (value descending, index ascending), stored in that order.  The result is a function of (row, W, lncut) alone.
//
// Pass 1 is k_draw's stage A, by the same function (draw_segment) on the same 256-entry segments with the same in-order sum of the
// segments' masses: lmap / levid are bit for bit what fz_draw_logwt reports.  Its LDS table is dead once `tot` is known, and pass 2
// reuses the space for a CANDIDATE BUFFER of `cap` entries (a 64-bit order-preserving image of the value, and the index): every
// eligible entry that beats the bar is appended; before a step that could overflow the buffer it is CUT to its best W in the order
// (image descending, index ascending), which has no ties, and the W-th becomes the new bar.  A cut is a radix select, not a sort:
// eight passes of 256-bin counts over the images give the W-th largest image T, three more over the indices of the entries at T
// give the last index that still belongs, and the survivors are compacted in place -- some 80 bytes of LDS traffic per candidate
// where a bitonic sort of the buffer moves a thousand (LDS bandwidth is what a block per object spends here).  Appending and
// compacting are in no fixed order, which is immaterial: what survives a cut is a SET that the pair order defines, and one bitonic
// sort of the at most W survivors at the end puts it in the law's order.  cap >= min(W, L) + one step, so a cut always makes room.
#pragma once
#include "fz_draw.h"

#define FZ_SPARSE_WMAX 4096                // most entries kept per object (what the k-NN consumers take)

namespace fz {

// doubles -> unsigned integers in the same order (no nan here; -0 counts as +0: the entries are compared as doubles)
__device__ __forceinline__ unsigned long long sparse_key(double v) {
    if (v == 0.0) v = 0.0;
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double sparse_val(unsigned long long k) {
    const unsigned long long b = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
    return __longlong_as_double((long long)b);
}
// (ka, ia) comes before (kb, ib): the larger value, then the smaller index
__device__ __forceinline__ bool sparse_before(unsigned long long ka, unsigned ia, unsigned long long kb, unsigned ib) {
    return ka > kb || (ka == kb && ia < ib);
}

// sorts keys[0..n) / idx[0..n) into the law's order, using the buffer up to the next power of two; every thread of the block calls it
__device__ __forceinline__ void sparse_sort(unsigned long long* keys, unsigned* idx, int n, int nthreads) {
    int P = 1;
    while (P < n) P <<= 1;
    for (int t = n + (int)threadIdx.x; t < P; t += nthreads) { keys[t] = 0ull; idx[t] = 0xFFFFFFFFu; }     // behind every real entry
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int p = threadIdx.x; p < (P >> 1); p += nthreads) {
                const int a = ((p & ~(j - 1)) << 1) | (p & (j - 1)), b = a | j;
                const unsigned long long ka = keys[a], kb = keys[b];
                const unsigned ia = idx[a], ib = idx[b];
                const bool fwd = (a & k) == 0;                       // this run is sorted best first
                if (fwd ? sparse_before(kb, ib, ka, ia) : sparse_before(ka, ia, kb, ib)) { keys[a] = kb; keys[b] = ka; idx[a] = ib; idx[b] = ia; }
            }
            __syncthreads();
        }
    }
}

// The kth (1-based) largest (`largest`) or smallest of the `nbytes`-byte keys get(t) hands out for t in [0, n) with in == true;
// kth must not exceed their number.  On return kth is the answer's place among the keys EQUAL to it (kth less the keys beyond it).
// Every thread of the block calls it and gets the same answer; hist: 256 ints, sel: 2 ints of LDS.
template <int NT, class F>
__device__ __forceinline__ unsigned long long sparse_radix_select(int n, int& kth, int nbytes, bool largest, F get, int* hist, int* sel) {
    const int lane = threadIdx.x & 63;
    unsigned long long prefix = 0ull;
    for (int pass = nbytes - 1; pass >= 0; --pass) {
        const int shift = 8 * pass;
        const unsigned long long himask = pass == 7 ? 0ull : (~0ull << (shift + 8));       // the bytes already decided
        for (int b = threadIdx.x; b < 256; b += NT) hist[b] = 0;
        __syncthreads();
        for (int t = threadIdx.x; t < n; t += NT) {
            bool in; unsigned long long k;
            get(t, in, k);
            if (in && ((k ^ prefix) & himask) == 0ull) atomicAdd(&hist[(int)((k >> shift) & 255ull)], 1);
        }
        __syncthreads();
        if (threadIdx.x < 64) {                                     // the first wave: lane l takes the 4 bins at places 4 l .. 4 l + 3 of the scan
            int c[4], tot = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) { const int place = 4 * lane + q; c[q] = hist[largest ? 255 - place : place]; tot += c[q]; }
            int incl = tot;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) { const int v = __shfl_up(incl, d, 64); if (lane >= d) incl += v; }
            int run = incl - tot;
            if (run < kth && kth <= incl) {                         // exactly one lane
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (kth > run && kth <= run + c[q]) { const int place = 4 * lane + q; sel[0] = largest ? 255 - place : place; sel[1] = kth - run; }
                    run += c[q];
                }
            }
        }
        __syncthreads();
        prefix |= (unsigned long long)sel[0] << shift;
        kth = sel[1];
    }
    return prefix;
}

// cuts the n > W candidates to the best W (in no order): -> the bar, the W-th in the law's order.  hist: 256 ints, sel: 8 ints of LDS
template <int NW>
__device__ __forceinline__ void sparse_cut(unsigned long long* keys, unsigned* idx, int n, int W, int* hist, int* sel, unsigned long long& bkey,
                                           unsigned& bidx) {
    constexpr int NT = NW * 64;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int ties = W;                                                   // -> how many of the entries AT the W-th largest image still belong (>= 1)
    const unsigned long long T = sparse_radix_select<NT>(n, ties, 8, true, [&](int t, bool& in, unsigned long long& k) { in = true; k = keys[t]; }, hist, sel);
    int last = ties;
    const unsigned Ti = (unsigned)sparse_radix_select<NT>(n, last, 3, false,
                                                          [&](int t, bool& in, unsigned long long& k) { in = keys[t] == T; k = idx[t]; }, hist, sel);
    // in place, chunk by chunk: a chunk is read by every thread before any of its survivors is written, and a survivor only moves left
    int wbase = 0;
    for (int c0 = 0; c0 < n; c0 += NT) {
        const int t = c0 + threadIdx.x;
        unsigned long long k = 0ull; unsigned id = 0u; bool keep = false;
        if (t < n) { k = keys[t]; id = idx[t]; keep = !sparse_before(T, Ti, k, id); }
        const unsigned long long mask = __ballot(keep);
        if (lane == 0) sel[4 + wave] = __popcll(mask);
        __syncthreads();
        int off = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) { const int cw = sel[4 + w]; if (w < wave) off += cw; tot += cw; }
        if (keep) { const int slot = wbase + off + __popcll(mask & ((1ull << lane) - 1ull)); keys[slot] = k; idx[slot] = id; }
        wbase += tot;
        __syncthreads();
    }
    bkey = T; bidx = Ti;
}

// rows (N, L) of ln-weights -> nbr (N, W) int64 (-99 behind the kept), nn (N) int64, vals (N, W) (-inf behind the kept), lmap, levid,
// lnkept (N); every output but nbr and nn may be nullptr.  cap: entries of the candidate buffer, >= min(W, L rounded up to a
// step) + NW * 256 and >= the power of two that min(W, L) rounds up to.  Dynamic LDS: max(16 x segments, 12 x cap) bytes.
template <int NW>
static __global__ __launch_bounds__(NW * 64) void k_sparse_select(const double* __restrict__ rows, int64_t N, int64_t L, int W, double lncut, int cap,
                                                                  int64_t* __restrict__ nbr, int64_t* __restrict__ nn, double* __restrict__ vals,
                                                                  double* __restrict__ lmap, double* __restrict__ levid,
                                                                  double* __restrict__ lnkept) {
    extern __shared__ double sm[];
    __shared__ double s_w[4];                                       // per wave: nan seen
    __shared__ double s_tot;
    __shared__ int s_cnt;
    __shared__ int s_hist[256], s_sel[8];
    constexpr int NT = NW * 64;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t i = blockIdx.x;
    if (i >= N) return;
    const int nseg = (int)((L + FZ_DRAW_SEG - 1) / FZ_DRAW_SEG);
    double* fk = sm;                                                // m_k, then f_k
    double* Pk = sm + nseg;                                         // S_k, then the mass
    const double* in = rows + i * L;

    // ---- pass 1: k_draw's stage A ----
    bool isnan = false;
    {
        double r[4], rn[4], e[4], p[4], x, mk;
        if (wave < nseg) draw_load(in, L, wave, lane, r);
        for (int k = wave; k < nseg; k += NW) {
            const bool more = k + NW < nseg;
            if (more) draw_load(in, L, k + NW, lane, rn);
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
    if (lane == 0) s_w[wave] = wnan ? 1.0 : 0.0;
    __syncthreads();
    double m = -INFINITY;
    for (int k = lane; k < nseg; k += 64) m = fmax(m, fk[k]);
    m = wave_max(m);
    bool anynan = false;
#pragma unroll
    for (int w = 0; w < NW; ++w) anynan |= s_w[w] != 0.0;
    const bool ok = !anynan && (m - m == 0.0);
    __syncthreads();
    for (int k = threadIdx.x; k < nseg; k += NT) {
        const double f = exp(fk[k] - m);
        fk[k] = f; Pk[k] = Pk[k] * f;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double P = 0.0;
        for (int k = 0; k < nseg; ++k) P += Pk[k];
        s_tot = P;
        s_cnt = 0;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double lm = anynan ? (double)NAN : m;
        if (lmap) lmap[i] = lm;
        if (levid) levid[i] = ok ? m + log(s_tot) : lm;
    }
    __syncthreads();                                                // the table is dead from here on

    // ---- pass 2: candidates ----
    unsigned long long* keys = (unsigned long long*)sm;
    unsigned* idx = (unsigned*)(keys + cap);
    int kept = 0;
    if (ok) {                                                       // (block-uniform)
        constexpr int STEP = NW * FZ_DRAW_SEG;
        bool bar = false; unsigned long long bkey = 0ull; unsigned bidx = 0u;
        double r[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY}, rn[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        if (wave < nseg) draw_load(in, L, wave, lane, r);
        int have = 0;                                               // the count, as every thread read it between two barriers
        for (int k0 = 0; k0 < nseg; k0 += NW) {
            const int k = k0 + wave;
            if (k + NW < nseg) draw_load(in, L, k + NW, lane, rn);
            if (have + STEP > cap) {                                // cut to the best W (have > W here, because cap >= W + STEP)
                sparse_cut<NW>(keys, idx, have, W, s_hist, s_sel, bkey, bidx);
                bar = true;
                if (threadIdx.x == 0) s_cnt = W;
                __syncthreads();
                have = W;
            }
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const unsigned j = (unsigned)k * FZ_DRAW_SEG + 4u * lane + t;
                bool take = k < nseg && (r[t] - m > lncut);         // past the row's end the load gave -inf
                const unsigned long long key = sparse_key(r[t]);
                if (take && bar) take = sparse_before(key, j, bkey, bidx);
                const unsigned long long mask = __ballot(take);
                if (mask) {
                    int base = 0;
                    if (lane == 0) base = atomicAdd(&s_cnt, __popcll(mask));
                    base = __shfl(base, 0, 64);
                    if (take) {
                        const int slot = base + __popcll(mask & ((1ull << lane) - 1ull));
                        keys[slot] = key; idx[slot] = j;
                    }
                }
            }
            __syncthreads();
            have = s_cnt;
            __syncthreads();                                        // (the next step's appends come after every thread's read)
#pragma unroll
            for (int t = 0; t < 4; ++t) r[t] = rn[t];
        }
        if (have > W) { sparse_cut<NW>(keys, idx, have, W, s_hist, s_sel, bkey, bidx); have = W; }
        sparse_sort(keys, idx, have, NT);
        kept = have;
    }

    // ---- outputs ----
    for (int t = threadIdx.x; t < W; t += NT) {
        const bool in_row = t < kept;
        nbr[i * W + t] = in_row ? (int64_t)idx[t] : (int64_t)-99;
        if (vals) vals[i * W + t] = in_row ? sparse_val(keys[t]) : -INFINITY;
    }
    // lnkept by the first wave alone, lane l summing the entries l, l + 64, ... in turn: one order whatever the geometry
    if (wave == 0) {
        double part = 0.0;
        for (int t = lane; t < kept; t += 64) part += exp(sparse_val(keys[t]) - m);
        part = wave_sum(part);
        if (lane == 0) {
            nn[i] = kept;
            if (lnkept) lnkept[i] = kept ? m + log(part) : -INFINITY;
        }
    }
}

// out (n, W) = plane (n, M) at the kept entries, `pad` behind them; 8-byte items of any kind.  plane == nullptr: `fill` at the kept
// entries (the ln-prior of a fit without one)
static __global__ void k_sparse_gather(const unsigned long long* __restrict__ plane, int64_t n, int64_t M, const int64_t* __restrict__ nbr,
                                       const int64_t* __restrict__ nn, int W, unsigned long long fill, unsigned long long pad,
                                       unsigned long long* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * W) return;
    const int64_t i = e / W; const int t = (int)(e - i * W);
    unsigned long long v = pad;
    if (t < nn[i]) {
        const int64_t j = nbr[e];
        v = !plane ? fill : (j >= 0 && j < M) ? plane[i * M + j] : pad;
    }
    out[e] = v;
}

}  // namespace fz
