// Counter-based random numbers on the device: Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as
// 1, 2, 3", SC'11).  A draw is a pure function of (key, counter): no state, no ordering between threads, reproducible on the host
// (frankenz_amd/samplers.py:_philox4x32 is the NumPy twin; tests/test_nz_samplers_host.py holds the paper's known answers).
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

namespace fz {

struct Philox4 { uint32_t v[4]; };

__host__ __device__ inline Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)M0 * c0, p1 = (uint64_t)M1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += W0; k1 += W1;
    }
    Philox4 o; o.v[0] = c0; o.v[1] = c1; o.v[2] = c2; o.v[3] = c3;
    return o;
}

// one uniform double in [0, 1) per (index, sweep) under a 64-bit key: the counter is (index lo, index hi, sweep lo, sweep hi); the
// double is made of the first two output words the way NumPy's RandomState makes one of two 32-bit draws (53 random bits)
__host__ __device__ inline double philox_uniform(uint32_t k0, uint32_t k1, uint64_t index, uint64_t sweep) {
    const Philox4 o = philox4x32_10((uint32_t)index, (uint32_t)(index >> 32), (uint32_t)sweep, (uint32_t)(sweep >> 32), k0, k1);
    const uint64_t a = o.v[0] >> 5, b = o.v[1] >> 6;
    return (double)((a << 26) | b) * (1.0 / 9007199254740992.0);
}

// U(a, b) = ((a >> 5) 2^26 + (b >> 6)) / 2^53 of two output words
__host__ __device__ inline double philox_u53(uint32_t a, uint32_t b) {
    return (double)(((uint64_t)(a >> 5) << 26) | (uint64_t)(b >> 6)) * (1.0 / 9007199254740992.0);
}

// Two standard normals per Philox call (the Monte-Carlo draws of the k-NN fitter, fz_knn_mc.h; knn._philox_normal is the NumPy twin):
// the counter is (index lo, index hi, pair, set) -- index: the 64-bit row (object first + i, or model j); pair = band >> 1, band b takes
// z0 when even and z1 when odd (an odd band count drops its last z1); set = 0 for a query draw, 1 + t for feature set t -- and the key
// (k0, k1 ^ FZ_KNN_KEY_XOR), so that a user key shared with the posterior draws of fit_sample (which use the key itself) gives an
// independent stream.  Box-Muller in the form of fz_mw.h's slot 2a: u1 = 1 - U(words 0, 1) in (0, 1], u2 = U(words 2, 3) in [0, 1),
// r = sqrt(-2 ln u1), z0 = r cos(2 pi u2), z1 = r sin(2 pi u2).
#define FZ_KNN_KEY_XOR 0x6B6E6D63u         // second key word of the k-NN Monte-Carlo draws: k1 ^ this ("knmc")
__host__ __device__ inline void philox_normal2(uint32_t k0, uint32_t k1, uint64_t index, uint32_t pair, uint32_t set, double& z0, double& z1) {
    const Philox4 o = philox4x32_10((uint32_t)index, (uint32_t)(index >> 32), pair, set, k0, k1 ^ FZ_KNN_KEY_XOR);
    const double u1 = 1.0 - philox_u53(o.v[0], o.v[1]), u2 = philox_u53(o.v[2], o.v[3]);
    const double r = sqrt(-2.0 * log(u1)), a = 6.283185307179586 * u2;
    z0 = r * cos(a);
    z1 = r * sin(a);
}

}  // namespace fz
