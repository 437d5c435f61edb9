// The n(z) samplers' device side (samplers.py:83-535 of the reference; docs/samplers.md).
//
// population_sampler -- Metropolis-Hastings-in-Gibbs over random pairs of bins.  The state (pos, overlap = pdfs @ pos, lnpost) lives
// on the device; the random stream is the reference's, drawn ahead by the host into tables (pairs, normals, exponentials).  A pair
// costs one k_pair_open (gather d = pdfs[:, i] - pdfs[:, j], both gradient sums) and mh_steps k_pair_try (one proposal sum each),
// every one followed by a ONE-BLOCK decision kernel that adds the block partials in index order and takes the reference's decision
// in one thread.  Nothing waits on another workgroup: the order is the stream's.  An accepted step is not applied to `overlap` by a
// pass of its own: it stays PENDING and the next pass over the objects applies it first (overlap + z * d, rounded as NumPy rounds
// it: the build passes -ffp-contract=off and nothing here asks for an fma).
//
// hierarchical_sampler -- k_nz_sweep is k_nz_assign's draw without the per-object bins, with the uniform either read (the caller's
// stream) or made in the kernel by Philox4x32-10 from (key, object, sweep).
#pragma once
#include "fz_device.h"
#include "fz_philox.h"

namespace fz {

#define NZ_NT 256           // threads of a block of the object passes
#define NZ_CHUNK 1024       // objects per block: partial b is the sum over objects [b * NZ_CHUNK, (b + 1) * NZ_CHUNK)

// What the object passes read and the decision kernels write (the host writes it in the per-evaluation form).
struct NzState {
    int32_t pi, pj;         // the pair whose difference column sits in `d`
    int32_t has_pend;       // the last accepted step has not been applied to `overlap` yet
    int32_t valid;          // the proposal leaves pos[pi], pos[pj] finite and non-negative (else: no evaluation, samplers.py:63-64)
    double pend;            // the pending step
    double h;               // scale / 2 of the numerical gradient
    double z;               // the proposal
    double scale, gscale;
    double pni, pnj;        // pos[pi] + z, pos[pj] - z
    double sum[2];          // the last sums (per-evaluation form: read back by the host)
};

// fixed-order block sum: thread t adds its four objects, then one tree over the 256 threads
__device__ inline double nz_block_sum(double v, double* sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int s = NZ_NT / 2; s > 0; s >>= 1) { if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s]; __syncthreads(); }
    const double r = sh[0];
    __syncthreads();
    return r;
}

// ---- a new pair: apply the pending step (with the OLD difference column), gather the new column, both gradient sums ----
static __global__ __launch_bounds__(NZ_NT) void k_pair_open(const double* __restrict__ pdfs, int64_t N, int G, const NzState* __restrict__ st,
                                                            double* __restrict__ overlap, double* __restrict__ d,
                                                            double* __restrict__ partial, int64_t nblk) {
    __shared__ double sh[NZ_NT];
    const int pi = st->pi, pj = st->pj, has_pend = st->has_pend;
    const double pend = st->pend, h = st->h;
    const int64_t base = (int64_t)blockIdx.x * NZ_CHUNK;
    double sp = 0.0, sm = 0.0;
#pragma unroll
    for (int k = 0; k < NZ_CHUNK / NZ_NT; ++k) {
        const int64_t i = base + k * NZ_NT + threadIdx.x;
        if (i < N) {
            double ov = overlap[i];
            if (has_pend) { ov = ov + pend * d[i]; overlap[i] = ov; }
            const double* p = pdfs + i * G;
            const double dn = p[pi] - p[pj];
            d[i] = dn;
            const double t = h * dn;
            sp += log(ov + t);
            sm += log(ov - t);
        }
    }
    const double bp = nz_block_sum(sp, sh), bm = nz_block_sum(sm, sh);
    if (threadIdx.x == 0) { partial[blockIdx.x] = bp; partial[nblk + blockIdx.x] = bm; }
}

// ---- one proposal: apply the pending step, sum(log(overlap + z * d)) ----
static __global__ __launch_bounds__(NZ_NT) void k_pair_try(int64_t N, const NzState* __restrict__ st, double* __restrict__ overlap,
                                                           const double* __restrict__ d, double* __restrict__ partial) {
    __shared__ double sh[NZ_NT];
    const int has_pend = st->has_pend, valid = st->valid;
    if (!has_pend && !valid) return;                 // uniform over the grid: nothing to apply, nothing to evaluate
    const double pend = st->pend, z = st->z;
    const int64_t base = (int64_t)blockIdx.x * NZ_CHUNK;
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < NZ_CHUNK / NZ_NT; ++k) {
        const int64_t i = base + k * NZ_NT + threadIdx.x;
        if (i < N) {
            double ov = overlap[i];
            const double di = d[i];
            if (has_pend) { ov = ov + pend * di; overlap[i] = ov; }
            if (valid) s += log(ov + z * di);
        }
    }
    if (!valid) return;
    const double b = nz_block_sum(s, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = b;
}

// the step a segment (or a per-evaluation chain) leaves pending, applied
static __global__ __launch_bounds__(NZ_NT) void k_pair_flush(int64_t N, const NzState* __restrict__ st, double* __restrict__ overlap,
                                                             const double* __restrict__ d) {
    if (!st->has_pend) return;
    const double pend = st->pend;
    const int64_t i = (int64_t)blockIdx.x * NZ_NT + threadIdx.x;
    if (i < N) overlap[i] = overlap[i] + pend * d[i];
}
static __global__ void k_pair_flushed(NzState* st) { st->has_pend = 0; st->pend = 0.0; }

// sum of `n` block partials in index order: thread t adds partials t, t + 256, ..., then one tree
__device__ inline double nz_sum_partials(const double* partial, int64_t n, double* sh) {
    double s = 0.0;
    for (int64_t k = threadIdx.x; k < n; k += NZ_NT) s += partial[k];
    return nz_block_sum(s, sh);
}

// per-evaluation form: the sums only (the decision is the host's)
static __global__ __launch_bounds__(NZ_NT) void k_pair_sums(const double* __restrict__ partial, int64_t nblk, int nsum, NzState* __restrict__ st) {
    __shared__ double sh[NZ_NT];
    for (int q = 0; q < nsum; ++q) {
        const double s = nz_sum_partials(partial + q * nblk, nblk, sh);
        if (threadIdx.x == 0) st->sum[q] = s;
    }
}

struct NzChain {
    const int64_t* pairs;   // (nsamp * thin, 2)
    const double* normals;  // (nsamp * thin, mh_steps)
    const double* expo;     // (nsamp * thin, mh_steps)
    double* pos;            // (G) in/out
    double* lnpost;         // (1) in/out
    double* samples;        // (nsamp, G)
    double* samples_lnp;    // (nsamp)
    int32_t* accept;        // (nsamp * thin, mh_steps)
    double* gscale;         // (nsamp * thin)
    int G, thin, mh;
};

// the reference's pair set-up (samplers.py:268-272): scale = 1e-4 * min(pos[i], pos[j], 1 - pos[i], 1 - pos[j])
__device__ inline void nz_begin_pair(const NzChain& c, int64_t p, NzState* st) {
    const int pi = (int)c.pairs[2 * p], pj = (int)c.pairs[2 * p + 1];
    const double a = c.pos[pi], b = c.pos[pj];
    double m = a;
    m = (b < m || b != b) ? b : m;
    const double a1 = 1. - a, b1 = 1. - b;
    m = (a1 < m || a1 != a1) ? a1 : m;
    m = (b1 < m || b1 != b1) ? b1 : m;
    st->pi = pi; st->pj = pj;
    st->scale = 1e-4 * m;
    st->h = st->scale / 2.;
}
// proposal k of pair p (samplers.py:291-294): z = randn * gscale, pos_new = pos + t * z
__device__ inline void nz_propose(const NzChain& c, int64_t p, int k, NzState* st) {
    const double z = c.normals[p * c.mh + k] * st->gscale;
    const double ni = c.pos[st->pi] + z, nj = c.pos[st->pj] + (-1. * z);
    st->z = z; st->pni = ni; st->pnj = nj;
    st->valid = (ni - ni == 0.0) && (nj - nj == 0.0) && !(ni < 0.) && !(nj < 0.);
}

// first pair of a segment
static __global__ void k_pair_begin(NzChain c, int64_t p, NzState* st) { nz_begin_pair(c, p, st); st->has_pend = 0; st->pend = 0.0; st->valid = 0; }

// after k_pair_open of pair p: the gradient, its scale and the first proposal (samplers.py:273-294)
static __global__ __launch_bounds__(NZ_NT) void k_pair_grad(NzChain c, int64_t p, const double* __restrict__ partial, int64_t nblk,
                                                            NzState* __restrict__ st) {
    __shared__ double sh[NZ_NT];
    const double lnp1 = nz_sum_partials(partial, nblk, sh);
    const double lnp2 = nz_sum_partials(partial + nblk, nblk, sh);
    if (threadIdx.x != 0) return;
    const double scale = st->scale;
    const double grad = (lnp1 - lnp2) / scale;
    double gs;
    if (grad != 0.) {
        const double g1 = fabs(1. / grad), g2 = fabs(scale * 1e4);
        gs = (g2 < g1) ? g2 : g1;                    // Python's min(g1, g2): g1 unless g2 is smaller (a nan g1 stays)
    } else gs = fabs(scale);
    st->gscale = gs; c.gscale[p] = gs;
    st->sum[0] = lnp1; st->sum[1] = lnp2;
    st->has_pend = 0; st->pend = 0.0;                // k_pair_open applied it
    nz_propose(c, p, 0, st);
}

// after k_pair_try of proposal k of pair p: the Metropolis decision (samplers.py:303-305), then the next proposal, or the next pair, or
// the saved sample
static __global__ __launch_bounds__(NZ_NT) void k_pair_decide(NzChain c, int64_t p, int k, int64_t p_end, const double* __restrict__ partial,
                                                              int64_t nblk, NzState* __restrict__ st) {
    __shared__ double sh[NZ_NT];
    __shared__ int save_row;
    const int valid = st->valid;
    double lnew = 0.0;
    if (valid) lnew = nz_sum_partials(partial, nblk, sh);
    if (threadIdx.x == 0) {
        const double lnpost = c.lnpost[0];
        const bool acc = valid && (-c.expo[p * c.mh + k] < lnew - lnpost);
        c.accept[p * c.mh + k] = acc ? 1 : 0;
        if (acc) {
            c.pos[st->pi] = st->pni; c.pos[st->pj] = st->pnj; c.lnpost[0] = lnew;
            st->has_pend = 1; st->pend = st->z;
        } else { st->has_pend = 0; st->pend = 0.0; }  // k_pair_try applied what was pending
        st->sum[0] = lnew;
        save_row = 0;
        if (k + 1 < c.mh) nz_propose(c, p, k + 1, st);
        else {
            st->valid = 0;
            save_row = (p + 1) % c.thin == 0;
            if (save_row) c.samples_lnp[p / c.thin] = c.lnpost[0];
            // the next pair's columns are gathered by k_pair_open, which applies the pending step with THIS pair's column first:
            // only the pair and its scale change here
            if (p + 1 < p_end) nz_begin_pair(c, p + 1, st);
        }
    }
    __syncthreads();
    if (save_row) {
        const int64_t s = p / c.thin;
        for (int g = threadIdx.x; g < c.G; g += NZ_NT) c.samples[s * c.G + g] = c.pos[g];
    }
}

// ---- column sums of the stack (pos_init = pdfs.sum(axis=0) / pdfs.sum(); the "stacked n(z)") in a fixed order ----
#define NZ_COLROWS 512
static __global__ __launch_bounds__(NZ_NT) void k_colsum_part(const double* __restrict__ pdfs, int64_t N, int G, double* __restrict__ part) {
    const int64_t r0 = (int64_t)blockIdx.x * NZ_COLROWS, r1 = (r0 + NZ_COLROWS < N) ? r0 + NZ_COLROWS : N;
    for (int g = threadIdx.x; g < G; g += NZ_NT) {
        double s = 0.0;
        for (int64_t r = r0; r < r1; ++r) s += pdfs[r * G + g];
        part[(int64_t)blockIdx.x * G + g] = s;
    }
}
static __global__ __launch_bounds__(NZ_NT) void k_colsum_fin(const double* __restrict__ part, int64_t nblk, int G, double* __restrict__ out) {
    const int g = blockIdx.x * NZ_NT + threadIdx.x;
    if (g >= G) return;
    double s = 0.0;
    for (int64_t b = 0; b < nblk; ++b) s += part[b * G + g];
    out[g] = s;
}

// ---- one Gibbs sweep's categorical draws, counts only (k_nz_assign's draw, fz_summary.h: the same arithmetic) ----
template <bool PHILOX>
static __global__ __launch_bounds__(256) void k_nz_sweep(const double* __restrict__ pdfs, int64_t N, int G, const double* __restrict__ nz,
                                                         const double* __restrict__ u, uint32_t k0, uint32_t k1, uint64_t sweep, int64_t i_off,
                                                         unsigned long long* __restrict__ counts, int staged) {
    extern __shared__ double s_w[];                               // [4][G]: the wave's row of p[g] * nz[g]
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= N) return;
    double* pl = s_w + (size_t)(threadIdx.x >> 6) * G;
    const double* pg = pdfs + i * G;
    if (staged) for (int g = lane; g < G; g += 64) pl[g] = pg[g] * nz[g];
    auto W = [&](int g) { return staged ? pl[g] : pg[g] * nz[g]; };
    const int per = (G + 63) / 64;
    const int g0 = lane * per, g1 = min(G, g0 + per);
    double s = 0.0;
    for (int g = g0; g < g1; ++g) s += W(g);
    double incl = s;
#pragma unroll
    for (int dd = 1; dd < 64; dd <<= 1) { const double t = __shfl_up(incl, dd, 64); if (lane >= dd) incl += t; }
    const double total = __shfl(incl, 63, 64);
    if (total > 0.0 && total - total == 0.0) {                    // (a row without mass under nz is left out of the counts)
        const double ui = PHILOX ? philox_uniform(k0, k1, (uint64_t)(i_off + i), sweep) : u[i];
        const double target = ui * total;
        const double excl = incl - s;
        const unsigned long long mass = __ballot(s > 0.0), at = __ballot(incl > target) & mass;
        const int owner = at ? __builtin_ctzll(at) : 63 - __builtin_clzll(mass);
        if (lane == owner) {
            double c = excl; int g = g0, last = g0;
            for (; g < g1; ++g) { const double w = W(g); if (w > 0.0) last = g; c += w; if (at && c > target) break; }
            const int bin = (g < g1) ? g : last;
            atomicAdd(&counts[bin], 1ull);
        }
    }
}

}  // namespace fz
