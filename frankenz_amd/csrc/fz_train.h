// What the persistent-workgroup trainers share (k_som_train in fz_som.h, k_gng_train in fz_gng.h): the per-row terms of the
// ln-likelihood, the staging of a chunk of drawn rows into LDS, the ln-likelihood of a row against one node (noiseless, unmasked
// model), the np.argmax order with its wave butterfly, and the workgroup rank of a predicate.  `Args` below is SomArgs or GngArgs:
// both carry x, xe, xm, rowk, draws, B and the option flags free_scale, dim_prior, modec, track_scale.  docs/som.md, docs/gng.md.
#pragma once
#include "fz_device.h"

namespace fz {

#define TRAIN_CHUNK 32      // steps whose rows are staged into LDS at once
#define TRAIN_NT 1024       // threads of a trainer's workgroup (at most)

// The terms of a row's ln-likelihood that are the same for every node (pdf.py:90-98, 226-235): ym = 1, so Ndim = sum(xm), and
// tot_var = xe^2 (+ 0^2) in every mode.  One thread per model row, once per launch of a trainer (lgamma kept out of its loop).
// rowk (M, 4): am1, gammaln(a), ln2 a, -0.5 (Ndim ln 2pi + sum log tot_var)
__global__ __launch_bounds__(256) void k_train_rowk(const double* __restrict__ xe, const double* __restrict__ xm, int64_t M, int B,
                                                    int free_scale, double* __restrict__ rowk) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= M) return;
    double nd = 0.0, slv = 0.0;
    for (int b = 0; b < B; ++b) {
        const double e = xe[j * B + b];
        nd += xm[j * B + b];
        slv += log(e * e);
    }
    const double av = free_scale ? 0.5 * (nd - 1.0) : 0.5 * nd;
    rowk[j * 4 + 0] = av - 1.0; rowk[j * 4 + 1] = lgamma(av); rowk[j * 4 + 2] = FZ_LN2 * av;
    rowk[j * 4 + 3] = -0.5 * (nd * FZ_LN2PI + slv);
}

// per-step record staged in LDS: the head x[B] tv[B] m[B] am1 G1 G2 K, then the trainer's own tail
__host__ __device__ constexpr int train_rec_head(int B) { return 3 * B + 4; }

// Stages the records of the nc steps from c0 on (records RW doubles apart), between the two barriers of a chunk: the head here,
// the tail by tail(step, drawn row, the record's tail), called by one thread per record.
template <class Args, class Tail>
__device__ __forceinline__ void train_stage(const Args& a, int64_t c0, int nc, double* rec, int RW, int t, int NT, Tail tail) {
    const int B = a.B;
    __syncthreads();                                             // the previous chunk's records are no longer read
    for (int e = t; e < nc * B; e += NT) {
        const int r = e / B, b = e - r * B;
        const int64_t j = a.draws[c0 + r];
        const double xe = a.xe[j * B + b];
        double* R = rec + r * RW;
        R[b] = a.x[j * B + b]; R[B + b] = xe * xe; R[2 * B + b] = a.xm[j * B + b];
    }
    if (t < nc) {
        const int64_t j = a.draws[c0 + t];
        const double* q = a.rowk + j * 4;
        double* R = rec + t * RW + 3 * B;
        R[0] = q[0]; R[1] = q[1]; R[2] = q[2]; R[3] = q[3];
        tail(c0 + t, j, R + 4);
    }
    __syncthreads();
}

// a staged record's head, read once per step
struct TrainRow { const double *x, *tv, *m; double am1, G1, G2, K; };
__device__ __forceinline__ TrainRow train_row(const double* R, int B) {
    return TrainRow{R, R + B, R + 2 * B, R[3 * B], R[3 * B + 1], R[3 * B + 2], R[3 * B + 3]};
}

// ln-likelihood of the row against the node y (pdf.py:90-98, 199-235, in the reference's operation order); chi2 comes back too, and
// under track_scale y leaves rescaled by the fitted scale (networks.py:1838-1840, 2171-2173)
template <class Args>
__device__ __forceinline__ double train_lnl(const Args& a, const TrainRow& r, double* y, double& chi2) {
    const int B = a.B;
    const double *x = r.x, *tv = r.tv, *m = r.m;
    double s = 1.0;
    chi2 = 0.0;
    if (a.free_scale) {
        double inter = 0.0, shape = 0.0;
        for (int b = 0; b < B; ++b) { const double yb = y[b]; inter += (m[b] * yb) * x[b] / tv[b]; shape += m[b] * (yb * yb) / tv[b]; }
        s = inter / shape;
        for (int b = 0; b < B; ++b) { const double d = x[b] - s * y[b]; chi2 += m[b] * (d * d) / tv[b]; }
    } else {
        for (int b = 0; b < B; ++b) { const double d = x[b] - y[b]; chi2 += m[b] * (d * d) / tv[b]; }
    }
    double lnl;
    if (a.dim_prior) {
        const double xl = (r.am1 == 0.0) ? ((chi2 == chi2) ? 0.0 : chi2) : r.am1 * log(chi2);     // xlogy
        lnl = ((xl - chi2 / 2.0) - r.G1) - r.G2;
    } else {
        lnl = -0.5 * chi2 + r.K;
    }
    // mode C with noiseless nodes: the second pass of pdf.py:199-222 repeats the first exactly, except that a non-finite scale makes
    // tot_var = xe^2 + (s * 0)^2 nan
    if (a.modec && !(s - s == 0.0)) lnl = NAN;
    if (a.track_scale) {
        for (int b = 0; b < B; ++b) y[b] = y[b] * s;
    }
    return lnl;
}

// np.argmax order: the first nan wins, else the larger value, ties to the lower index
__device__ __forceinline__ bool train_better(double va, int ia, double vb, int ib) {
    const bool na = va != va, nb = vb != vb;
    if (na || nb) return na && (!nb || ia < ib);
    return va > vb || (va == vb && ia < ib);
}

// np.argmax over the wave: every lane leaves with the winner
__device__ __forceinline__ void train_argmax_butterfly(double& v, int& i) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(v, o, 64); const int oi = __shfl_xor(i, o, 64);
        if (train_better(ov, oi, v, i)) { v = ov; i = oi; }
    }
}

// The number of lower threads of the workgroup whose pred is set; total: the number of all of them.  Every thread of the workgroup
// calls it; sc holds one int per wave and is free again on return (two barriers inside).
__device__ __forceinline__ int train_rank(bool pred, int* sc, int lane, int wave, int NW, int& total) {
    const unsigned long long bal = __ballot(pred);
    const int pre = __builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0));
    if (lane == 0) sc[wave] = __builtin_popcountll(bal);
    __syncthreads();
    int off = 0, tot = 0;
    for (int w = 0; w < NW; ++w) { const int v = sc[w]; if (w < wave) off += v; tot += v; }
    __syncthreads();
    total = tot;
    return off + pre;
}

}  // namespace fz
