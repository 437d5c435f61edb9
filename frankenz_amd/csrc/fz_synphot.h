// Synthetic photometry: the per-(template, redshift) loop of the reference's simulate.py (MockSurvey.sample_phot, simulate.py:811-840;
// make_model_grid, simulate.py:986-1014) with the Madau IGM transmission of reddening.py:23-95 (docs/simulate.md).
//
//   k_synphot   out[pair][f] = sum_k w_k sinh(np.interp(lw_k - ln(1 + z), t_lw, t_asinh)) exp(-tau(wave_k, z)): one wave per
//               (pair, filter), lanes striding the filter's points; a block serves a run of pairs of ONE template, whose ln-wavelength
//               table it stages in LDS (templates beyond the LDS budget are searched in global memory)
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "fz_summary.h"

namespace fz {

#define FZ_SYN_THREADS 512         // 8 waves; the kernel holds ~120 VGPRs (4 waves per SIMD), so two blocks share a CU and their two
                                   // staged tables (at most 64 KB each) fit its 160 KB of LDS
#define FZ_SYN_LDS_MAX 8192        // template points staged in LDS (64 KB)
#define FZ_SYN_NLINE 11            // Lyman lines of reddening.py:47-50
#define FZ_SYN_TABW 18             // per filter point: 12 running sums of the line terms, 6 powers of wave / 912

// One (template, redshift) pair, in template order; `slot` is its row of `out`.
struct SynPair { double z, ln1pz; int32_t tmpl, slot; };
// One block: pairs [p0, p1) of the sorted list, all of template `tmpl`
struct SynItem { int32_t tmpl, p0, p1, pad_; };
// What fz_synphot_upload left on the device.  ftab row k: P[0..11], P[j] = the first j line terms coeff_i (wave_k / l_i)^3.46 added in
// the reference's order (P[0] = 0), then (wave_k / 912)^{3, 0.46, 1.5, 0.18, -1.32, 1.68}: everything of tau that does not depend on z.
struct SynView {
    int Nf;
    const int64_t* foff; const double *fwave, *flw, *fwt, *ftab;
    const int64_t* toff; const double *tlw, *tas;
};

template <bool LDSX>
static __global__ __launch_bounds__(FZ_SYN_THREADS) void k_synphot(SynView v, const SynPair* __restrict__ pairs,
                                                                   const SynItem* __restrict__ items, int igm, double* __restrict__ out) {
    extern __shared__ double s_tlw[];
    constexpr double SYN_LINES[FZ_SYN_NLINE] = {1216.0, 1026.0, 973.0, 950.0, 938.1, 931.0, 926.5, 923.4, 921.2, 919.6, 918.4};
    const SynItem it = items[blockIdx.x];
    const int64_t t0 = v.toff[it.tmpl];
    const int n = (int)(v.toff[it.tmpl + 1] - t0);
    const double* gx = v.tlw + t0;
    const double* gy = v.tas + t0;
    if (LDSX) {
        for (int i = threadIdx.x; i < n; i += blockDim.x) s_tlw[i] = gx[i];
        __syncthreads();
    }
    const int lane = threadIdx.x & 63, nw = blockDim.x >> 6;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    auto XP = [&](int j) { return LDSX ? s_tlw[j] : gx[j]; };
    auto FP = [&](int j) { return gy[j]; };
    const int ntask = (it.p1 - it.p0) * v.Nf;
    for (int task = wave; task < ntask; task += nw) {
        const int p = it.p0 + task / v.Nf, f = task % v.Nf;
        const double z = pairs[p].z, l1z = pairs[p].ln1pz;
        const int64_t row = (int64_t)pairs[p].slot * v.Nf;
        // the powers of 1 + z: all of tau that belongs to the pair (reddening.py:31, 66, 71-75)
        const double xem = 1. + z;
        double e046 = 0., e018 = 0., em132 = 0., e168 = 0.;
        if (igm) { e046 = pow(xem, 0.46); e018 = pow(xem, 0.18); em132 = pow(xem, -1.32); e168 = pow(xem, 1.68); }
        const double zl0 = SYN_LINES[0] * xem, z912 = 912.0 * xem;
        const int64_t k1 = v.foff[f + 1];
        double acc = 0.0;
        for (int64_t k = v.foff[f] + lane; k < k1; k += 64) {
            const double y = sinh(interp1(v.flw[k] - l1z, XP, FP, n));
            double term = v.fwt[k] * y;
            if (igm) {
                const double wv = v.fwave[k];
                if (wv < zl0) {                                            // strict, as reddening.py:33
                    const double* tab = v.ftab + k * FZ_SYN_TABW;
                    int na = 1;
#pragma unroll
                    for (int i = 1; i < FZ_SYN_NLINE; ++i) na += (wv < SYN_LINES[i] * xem) ? 1 : 0;
                    double tau = tab[na];
                    if (wv < z912) {                                       // reddening.py:68-76
                        const double c3 = tab[12], c046 = tab[13], c15 = tab[14], c018 = tab[15], cm132 = tab[16], c168 = tab[17];
                        double tau2 = (((0.25 * c3) * (e046 - c046)) + ((9.4 * c15) * (e018 - c018)) - ((0.7 * c3) * (cm132 - em132))) -
                                      (0.023 * (e168 - c168));
                        if (tau2 < 0.) tau2 = 0.;
                        tau = tau + tau2;
                    }
                    term = term * exp(-tau);
                }
            }
            acc += term;
        }
        acc = wsum(acc);
        if (lane == 0) out[row + f] = acc;
    }
}

}  // namespace fz
