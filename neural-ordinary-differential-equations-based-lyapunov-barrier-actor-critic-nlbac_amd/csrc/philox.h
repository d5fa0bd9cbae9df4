// Philox4x32-10 and the device-side minibatch draw built on it (device_rng mode), shared by the
// launches that draw a minibatch: nlbac_sample_rows (length by value) and nlbac_sample_rows_head (length read from a
// replay head in device memory) run the SAME body, so equal length, seed and draw give equal rows and noise.
#pragma once
#include "common.h"

__device__ __forceinline__ uint4 philox4x32_10(uint4 ctr, uint2 key) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * ctr.x;
        const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * ctr.z;
        ctr = make_uint4((unsigned)(p1 >> 32) ^ ctr.y ^ key.x, (unsigned)p1, (unsigned)(p0 >> 32) ^ ctr.w ^ key.y,
                         (unsigned)p0);
        key.x += 0x9E3779B9u;
        key.y += 0xBB67AE85u;
    }
    return ctr;
}

// The last counter word tags what a draw is for: 0 and 1 are sample_rows_body's (row indices, policy noise), 2 is the
// SimulatedCars reset's initial-velocity offset (env_reset_kernels.hip: cars_reset_offset, defined there because it
// must be compiled with contraction off).  THE definition of that draw, which the tests restate in numpy:
//   (x, y, z, w) = philox4x32_10(counter (lane, reset_count[lane] before the increment, 0, 2),
//                                key (seed & 0xffffffff, seed >> 32))
//   m1 = (x << 20) | (y >> 12),  u1 = (m1 + 0.5) * 2^-52;   m2, u2 likewise from z, w     (52-bit, exact, in (0, 1))
//   off = 0.5 * (sqrt(-2 * log(u1)) * cos(6.283185307179586 * u2)),   all in float64
// A lane's k-th offset depends on (seed, lane, k) alone: not on the lane count, nor on when the k-th reset happened.
#define PHILOX_TAG_CARS_RESET 2u
// 3 is the Quadrotor-like reset's start-position offsets (env_reset_kernels.hip: quadrotor_reset_offsets), the same
// counter and the same two 52-bit uniforms under a tag of their own:
//   (x, y, z, w) = philox4x32_10(counter (lane, reset_count[lane] before the increment, 0, 3), the same key)
//   u0 from (x, y), u1 from (z, w) as u1, u2 above;   dx = sx * (2 * u0 - 1),  dz = sz * (2 * u1 - 1),   all in float64
#define PHILOX_TAG_QUADROTOR_RESET 3u
// 4 is the start-position offsets of the Unicycle and Pvtol resets and their barrier copies' (env_reset_kernels.hip:
// start_reset_offsets), one tag for both tasks, again the same counter and the same two 52-bit uniforms:
//   (x, y, z, w) = philox4x32_10(counter (lane, reset_count[lane] before the increment, 0, 4), the same key)
//   u0 from (x, y), u1 from (z, w) as u1, u2 above;   dx = sx * (2 * u0 - 1),  dy = sy * (2 * u1 - 1),   all in float64
// (tests/test_start_spread_host.py restates it in numpy).
#define PHILOX_TAG_START_RESET 4u

__device__ __forceinline__ float u01(unsigned x) { return (float)(x >> 8) * 0x1p-24f + 0x1p-25f; }   // (0, 1]

// Thread t of the launch: row indices uniform on [0, src_rows) with replacement, the gather into minibatch layout and
// the N(0,1) policy noise of the update.  Counter = (draw number, row | lane); Box-Muller.  src_rows == 0: no row is
// copied and src is not read.
__device__ __forceinline__ void sample_rows_body(long t, const float4* __restrict__ src, int ld4, long n_rows,
                                                 long src_rows, float4* __restrict__ dst, float* __restrict__ eps,
                                                 long n_eps, unsigned long long seed, unsigned long long draw) {
    const uint2 key = make_uint2((unsigned)seed, (unsigned)(seed >> 32));
    if (t < n_rows * ld4 && src_rows > 0) {
        const long r = t / ld4;
        const int c = (int)(t - r * ld4);
        const uint4 x = philox4x32_10(make_uint4((unsigned)draw, (unsigned)(draw >> 32), (unsigned)r, 0u), key);
        const long j = (long)(((unsigned long long)x.x * (unsigned long long)src_rows) >> 32);
        dst[r * ld4 + c] = src[j * ld4 + c];
    }
    const long q = (n_eps + 3) >> 2;
    if (eps && t < q) {
        const uint4 x = philox4x32_10(make_uint4((unsigned)draw, (unsigned)(draw >> 32), (unsigned)t, 1u), key);
        const float r0 = sqrtf(-2.f * logf(u01(x.x))), r1 = sqrtf(-2.f * logf(u01(x.z)));
        float s0, c0, s1, c1;
        sincosf(6.283185307179586f * u01(x.y), &s0, &c0);
        sincosf(6.283185307179586f * u01(x.w), &s1, &c1);
        const float v[4] = {r0 * c0, r0 * s0, r1 * c1, r1 * s1};
        for (int k = 0; k < 4; ++k)
            if (4 * t + k < n_eps) eps[4 * t + k] = v[k];
    }
}
