// What the consumers of rows of ln-weights share on the device ("Adding a row consumer"): k_draw, k_mw_sweep, k_mw_em_rows,
// k_row_moments, k_row_bins.
//
//   RowGeom<WPO>     one object per group of WPO waves of a 256-thread block: WPO == 1, four objects per block, for rows of up to
//                    FZ_DRAW_WAVE_LMAX entries; WPO == 4, a block per object, beyond.  The geometry is a function of the row length
//                    alone (the host's row_geometry, fz_rows_host.inc), never of the chunk or of the object's place in it.
//   row_walk0<WPO>   the first walk of the consumers that keep their sums in registers (k_row_moments, k_row_bins): thread q of the
//                    object's 64 WPO owns the entries q, q + 64 WPO, ...; the max, a nan, and EVERY counted index against [0, M)
//                    before anything is gathered.
//
// The segment-table consumers (k_draw, k_mw_sweep, k_mw_em_rows) share the geometry and walk the row by segments (fz_draw.h).
#pragma once
#include "fz_device.h"

#define FZ_DRAW_WAVE_LMAX 4096             // rows up to here: one wave per object
#define FZ_MW_ERR_NNB 1                    // Nneighbors outside [0, W]                  (the two row bits of the error word; the
#define FZ_MW_ERR_NBR 2                    // a neighbour index outside [0, M)            other FZ_*_ERR_* bits belong to their kernels)

namespace fz {

template <int WPO>
struct RowGeom {
    static constexpr int OPB = 4 / WPO, NT = 64 * WPO;               // objects per block, threads per object
    const int lane, wave, obj, sub;                                  // wave: of the block; obj: of the block; sub: wave of the object
    const int64_t i;
    const bool live;
    bool badn = false;
    __device__ __forceinline__ explicit RowGeom(int64_t N)
        : lane(threadIdx.x & 63), wave(__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)), obj(wave / WPO), sub(wave % WPO),
          i((int64_t)blockIdx.x * OPB + obj), live(i < N) {}
    // the entries of the row that count: nnb[i], or W without nnb.  Outside [0, W]: 0, badn, and one lane raises `bit` of errflag
    // (EXCH: by atomicExch, k_draw's flag is that one value)
    template <bool EXCH = false>
    __device__ __forceinline__ int64_t counted(const int64_t* __restrict__ nnb, int64_t W, int* __restrict__ errflag, int bit) {
        int64_t n = 0;
        if (live) {
            n = nnb ? nnb[i] : W;
            if (n < 0 || n > W) {
                n = 0; badn = true;
                if (lane == 0 && sub == 0) { if constexpr (EXCH) atomicExch(errflag, bit); else atomicOr(errflag, bit); }
            }
        }
        return n;
    }
    // row i of a table `stride` apart (row 0 for a wave past the last object: it reads nothing through it); opt: nullptr stays nullptr
    template <class T> __device__ __forceinline__ const T* row(const T* p, int64_t stride) const { return p + (live ? i : 0) * stride; }
    template <class T> __device__ __forceinline__ const T* opt(const T* p, int64_t stride) const { return p ? row(p, stride) : nullptr; }
    __device__ __forceinline__ int64_t t0() const { return sub * 64 + lane; }    // the thread's first entry (row_walk0's ownership)
};

// r: the object's row, nb: its indices or nullptr, n: g.counted().  sh: columns 0 and 1 of an LDS array of one line per wave of the
// block carry the cross-wave combine (WPO > 1: two barriers; the columns are free again on return).  m: the row's max.
// Returns ok: the object is live, its count and every counted index are in range, no nan, and the max is finite.
template <int WPO, int C>
__device__ __forceinline__ bool row_walk0(const RowGeom<WPO>& g, const double* __restrict__ r, const int64_t* __restrict__ nb, int64_t n,
                                          int64_t M, double (*sh)[C], int* __restrict__ errflag, double& m) {
    m = -INFINITY;
    bool isnan = false, bad = false;
    for (int64_t t = g.t0(); t < n; t += g.NT) {
        const double v = r[t];
        isnan |= v != v;
        m = fmax(m, v);
        if (nb) { const int64_t j = nb[t]; bad |= j < 0 || j >= M; }
    }
    m = wave_max(m);
    const bool wbad = __any(bad);
    bool unfit = __any(isnan) || wbad;
    if (wbad && g.lane == 0) atomicOr(errflag, FZ_MW_ERR_NBR);
    if constexpr (WPO > 1) {
        if (g.lane == 0) { sh[g.wave][0] = m; sh[g.wave][1] = unfit ? 1.0 : 0.0; }
        __syncthreads();
        m = -INFINITY; unfit = false;
#pragma unroll
        for (int w = 0; w < WPO; ++w) { m = fmax(m, sh[g.obj * WPO + w][0]); unfit |= sh[g.obj * WPO + w][1] != 0.0; }
        __syncthreads();
    }
    return g.live && !g.badn && !unfit && (m - m == 0.0);
}

}  // namespace fz
