// Resets of the batched device simulators on the device (envs/device.py, device_resets=True): ONE launch per vector
// step restarts the lanes whose flag is set — state, step counter, clock / last distance, observation, reset counter,
// for SimulatedCars the initial-velocity offset and for the Quadrotor-like task, Unicycle and Pvtol with a start spread
// the start-position offsets, counter-based draws (philox.h: cars_reset_offset, quadrotor_reset_offsets,
// start_reset_offsets) — and leaves the float32 observation of EVERY lane, which is what the policy reads next.  A lane whose flag is not set keeps every
// float64 value the step kernel wrote; nothing of it is written but its obs32 row.  One lane per thread, no LDS, no
// atomics; include/nlbac_hip.h has the contract of every array.
//
// The step kernels stay in env_kernels.hip under their own contraction mode, which the reference traces pin.  Here a
// reset lane must hold what the host-mode reset (torch, numpy: every product and sum rounded on its own) holds, bit for
// bit, so the pragma below covers every function DEFINED after it and the arithmetic is written with plain * + -
// (handover_kernels.hip has the reason why the __dmul_rn family does not do).
#include <cstdint>
#include "common.h"
#include "philox.h"
#pragma clang fp contract(off)

// The N(0, 0.5) initial-velocity offset of lane `lane`'s reset number `count` (0 = the constructor's) under `seed`:
// philox.h has the definition, tests/test_env_reset_host.py restates it in numpy.
__device__ __forceinline__ double cars_reset_offset(unsigned long long seed, unsigned lane, unsigned count) {
    const uint2 key = make_uint2((unsigned)seed, (unsigned)(seed >> 32));
    const uint4 r = philox4x32_10(make_uint4(lane, count, 0u, PHILOX_TAG_CARS_RESET), key);
    const unsigned long long m1 = ((unsigned long long)r.x << 20) | (unsigned long long)(r.y >> 12);
    const unsigned long long m2 = ((unsigned long long)r.z << 20) | (unsigned long long)(r.w >> 12);
    const double u1 = ((double)m1 + 0.5) * 0x1p-52, u2 = ((double)m2 + 0.5) * 0x1p-52;      // exact, in (0, 1)
    const double rad = sqrt(-2.0 * log(u1));
    const double ang = 6.283185307179586 * u2;
    return 0.5 * (rad * cos(ang));
}

__global__ __launch_bounds__(256) void env_reset_rows_kernel(int n, const int* __restrict__ done, int state_dim,
                                                             int obs_dim, const double* __restrict__ start_state,
                                                             const double* __restrict__ start_obs,
                                                             double start_last_dist, double* __restrict__ state,
                                                             int* __restrict__ ep_step, double* __restrict__ last_dist,
                                                             double* __restrict__ obs, float* __restrict__ obs32,
                                                             int* __restrict__ reset_count) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double* o = obs + (long)i * obs_dim;
    float* o32 = obs32 + (long)i * obs_dim;
    if (!done || done[i] > 0) {
        double* st = state + (long)i * state_dim;
        for (int c = 0; c < state_dim; ++c) st[c] = start_state[c];
        ep_step[i] = 0;
        if (last_dist) last_dist[i] = start_last_dist;
        for (int c = 0; c < obs_dim; ++c) {
            const double v = start_obs[c];
            o[c] = v;
            o32[c] = (float)v;
        }
        reset_count[i] += 1;
    } else {
        for (int c = 0; c < obs_dim; ++c) o32[c] = (float)o[c];
    }
}

__global__ __launch_bounds__(256) void cars_env_reset_kernel(int n, const int* __restrict__ done,
                                                             unsigned long long seed, const double* __restrict__ noise,
                                                             double* __restrict__ state, double* __restrict__ t,
                                                             int* __restrict__ ep_step, double* __restrict__ obs,
                                                             float* __restrict__ obs32, int* __restrict__ reset_count,
                                                             double* __restrict__ reset_noise) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double* o = obs + (long)i * 10;
    float* o32 = obs32 + (long)i * 10;
    if (!done || done[i] > 0) {
        const int count = reset_count[i];
        const double off = noise ? noise[i] : cars_reset_offset(seed, (unsigned)i, (unsigned)count);
        double* st = state + (long)i * 10;
        // The host-mode reset scales the observation with torch's `tensor /= python scalar`, which the device evaluates
        // as a product with the scalar's reciprocal (rounded once, on the host): the same two roundings here, so that a
        // reset lane's observation is the host mode's bit for bit.
        const double per100 = 1.0 / 100.0, per30 = 1.0 / 30.0;
        for (int c = 0; c < 5; ++c) {
            const double pos = 42.0 - 8.0 * (double)c;           // 42, 34, 26, 18, 10
            const double vel = c == 3 ? 3.0 : 3.0 + off;         // (car 4 keeps 3.0: simulated_cars_env.py:139)
            const double op = pos * per100, ov = vel * per30;
            st[2 * c] = pos;
            st[2 * c + 1] = vel;
            o[2 * c] = op;
            o[2 * c + 1] = ov;
            o32[2 * c] = (float)op;
            o32[2 * c + 1] = (float)ov;
        }
        t[i] = 0.0;
        ep_step[i] = 0;
        reset_noise[i] = off;
        reset_count[i] = count + 1;
    } else {
        for (int c = 0; c < 10; ++c) o32[c] = (float)o[c];
    }
}

// The start-position offsets (dx, dz) of lane `lane`'s reset number `count` of the Quadrotor-like task under `seed`,
// uniform on [-sx, sx] x [-sz, sz]: philox.h has the definition, tests/test_quadrotor_env_gpu.py restates it in numpy.
__device__ __forceinline__ void uniform_reset_offsets(unsigned long long seed, unsigned lane, unsigned count,
                                                      unsigned tag, double s0, double s1, double* d0, double* d1) {
    const uint2 key = make_uint2((unsigned)seed, (unsigned)(seed >> 32));
    const uint4 r = philox4x32_10(make_uint4(lane, count, 0u, tag), key);
    const unsigned long long m0 = ((unsigned long long)r.x << 20) | (unsigned long long)(r.y >> 12);
    const unsigned long long m1 = ((unsigned long long)r.z << 20) | (unsigned long long)(r.w >> 12);
    const double u0 = ((double)m0 + 0.5) * 0x1p-52, u1 = ((double)m1 + 0.5) * 0x1p-52;      // exact, in (0, 1)
    *d0 = s0 * (2.0 * u0 - 1.0);
    *d1 = s1 * (2.0 * u1 - 1.0);
}

__device__ __forceinline__ void quadrotor_reset_offsets(unsigned long long seed, unsigned lane, unsigned count,
                                                        double sx, double sz, double* dx, double* dz) {
    uniform_reset_offsets(seed, lane, count, PHILOX_TAG_QUADROTOR_RESET, sx, sz, dx, dz);
}

struct QuadReset { double start[6], sx, sz; };

__global__ __launch_bounds__(256) void quadrotor_env_reset_kernel(int n, const int* __restrict__ done,
                                                                  unsigned long long seed, const QuadReset R,
                                                                  const double* __restrict__ noise,
                                                                  double* __restrict__ state, int* __restrict__ ep_step,
                                                                  double* __restrict__ obs, float* __restrict__ obs32,
                                                                  int* __restrict__ reset_count,
                                                                  double* __restrict__ reset_noise) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double* o = obs + (long)i * 6;
    float* o32 = obs32 + (long)i * 6;
    if (!done || done[i] > 0) {
        const int count = reset_count[i];
        double dx, dz;
        if (noise) { dx = noise[2 * (long)i]; dz = noise[2 * (long)i + 1]; }
        else quadrotor_reset_offsets(seed, (unsigned)i, (unsigned)count, R.sx, R.sz, &dx, &dz);
        double* st = state + (long)i * 6;
        for (int c = 0; c < 6; ++c) {
            double v = R.start[c];
            if (c == 0) v = v + dx;                              // (the host simulator's reset(offset): start + offset)
            if (c == 2) v = v + dz;
            st[c] = v;
            o[c] = v;
            o32[c] = (float)v;
        }
        ep_step[i] = 0;
        reset_noise[2 * (long)i] = dx;
        reset_noise[2 * (long)i + 1] = dz;
        reset_count[i] = count + 1;
    } else {
        for (int c = 0; c < 6; ++c) o32[c] = (float)o[c];
    }
}

// The start-position offsets (dx, dy) of lane `lane`'s reset number `count` of Unicycle / Pvtol (and their barrier
// copies) under `seed`, uniform on [-sx, sx] x [-sy, sy]: philox.h has the definition, tests/test_start_spread_host.py
// restates it in numpy.
__device__ __forceinline__ void start_reset_offsets(unsigned long long seed, unsigned lane, unsigned count, double sx,
                                                    double sy, double* dx, double* dy) {
    uniform_reset_offsets(seed, lane, count, PHILOX_TAG_START_RESET, sx, sy, dx, dy);
}

// What the Unicycle and Pvtol observations hold of the goal (unicycle_env.py:257-273, pvtol_env.py:361-406; the step
// kernels' unicycle_obs / pvtol_obs in env_kernels.hip): heading cosine and sine, the compass — the vector to the goal in
// the body frame, normalised with + 0.001 — and exp(-distance).
struct GoalObs { double c, s, v0, v1, e; };
__device__ __forceinline__ GoalObs goal_obs(double x, double y, double th, double gx, double gy) {
    const double rx = gx - x, ry = gy - y;
    const double dist = sqrt(rx * rx + ry * ry);
    const double c = cos(th), s = sin(th);
    const double v0 = rx * c + ry * s, v1 = -rx * s + ry * c;
    const double n = sqrt(v0 * v0 + v1 * v1) + 0.001;
    return GoalObs{c, s, v0 / n, v1 / n, exp(-dist)};
}

// envs.UnicycleEnv.reset(offset): the position moves, the centre l_p ahead of it moves with it, and last_dist is the
// moved centre's distance to the goal; the heading stays.
struct UniReset { double start[3], cx, cy, gx, gy, sx, sy; };

__global__ __launch_bounds__(256) void unicycle_env_reset_kernel(int n, const int* __restrict__ done,
                                                                 unsigned long long seed, const UniReset R,
                                                                 const double* __restrict__ noise,
                                                                 double* __restrict__ state, int* __restrict__ ep_step,
                                                                 double* __restrict__ last_dist,
                                                                 double* __restrict__ obs, float* __restrict__ obs32,
                                                                 int* __restrict__ reset_count,
                                                                 double* __restrict__ reset_noise) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double* o = obs + (long)i * 7;
    float* o32 = obs32 + (long)i * 7;
    if (!done || done[i] > 0) {
        const int count = reset_count[i];
        double dx, dy;
        if (noise) { dx = noise[2 * (long)i]; dy = noise[2 * (long)i + 1]; }
        else start_reset_offsets(seed, (unsigned)i, (unsigned)count, R.sx, R.sy, &dx, &dy);
        const double x = R.start[0] + dx, y = R.start[1] + dy, th = R.start[2];
        double* st = state + (long)i * 3;
        st[0] = x; st[1] = y; st[2] = th;
        const double ex = R.gx - (R.cx + dx), ey = R.gy - (R.cy + dy);
        last_dist[i] = sqrt(ex * ex + ey * ey);
        const GoalObs g = goal_obs(x, y, th, R.gx, R.gy);
        const double v[7] = {x, y, g.c, g.s, g.v0, g.v1, g.e};
        for (int c = 0; c < 7; ++c) { o[c] = v[c]; o32[c] = (float)v[c]; }
        ep_step[i] = 0;
        reset_noise[2 * (long)i] = dx;
        reset_noise[2 * (long)i + 1] = dy;
        reset_count[i] = count + 1;
    } else {
        for (int c = 0; c < 7; ++c) o32[c] = (float)o[c];
    }
}

// envs.PvtolEnv.reset(offset): x and y move, and the safety operator's x (state 6), which a reset places at the
// vehicle's x, moves by dx; tilt, velocities and thrust stay.
struct PvReset { double start[7], gx, gy, sx, sy; };

__global__ __launch_bounds__(256) void pvtol_env_reset_kernel(int n, const int* __restrict__ done,
                                                              unsigned long long seed, const PvReset R,
                                                              const double* __restrict__ noise,
                                                              double* __restrict__ state, int* __restrict__ ep_step,
                                                              double* __restrict__ obs, float* __restrict__ obs32,
                                                              int* __restrict__ reset_count,
                                                              double* __restrict__ reset_noise) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double* o = obs + (long)i * 11;
    float* o32 = obs32 + (long)i * 11;
    if (!done || done[i] > 0) {
        const int count = reset_count[i];
        double dx, dy;
        if (noise) { dx = noise[2 * (long)i]; dy = noise[2 * (long)i + 1]; }
        else start_reset_offsets(seed, (unsigned)i, (unsigned)count, R.sx, R.sy, &dx, &dy);
        double v[7];
        for (int c = 0; c < 7; ++c) v[c] = R.start[c];
        v[0] = v[0] + dx;
        v[1] = v[1] + dy;
        v[6] = v[6] + dx;
        double* st = state + (long)i * 7;
        for (int c = 0; c < 7; ++c) st[c] = v[c];
        const GoalObs g = goal_obs(v[0], v[1], v[2], R.gx, R.gy);
        const double w[11] = {v[0], v[1], g.c, g.s, v[3], v[4], v[5], v[6], g.v0, g.v1, g.e};
        for (int c = 0; c < 11; ++c) { o[c] = w[c]; o32[c] = (float)w[c]; }
        ep_step[i] = 0;
        reset_noise[2 * (long)i] = dx;
        reset_noise[2 * (long)i + 1] = dy;
        reset_count[i] = count + 1;
    } else {
        for (int c = 0; c < 11; ++c) o32[c] = (float)o[c];
    }
}

#define RESET_GRID(n) dim3(nlbac_ceil_div((n), 256)), dim3(256), 0, (hipStream_t)s

extern "C" int nlbac_env_reset_rows(int n, const int* done, int state_dim, int obs_dim, const double* start_state,
                                    const double* start_obs, double start_last_dist, double* state, int* ep_step,
                                    double* last_dist, double* obs, float* obs32, int* reset_count, nlbac_stream_t s) {
    NLBAC_REQUIRE(n >= 1, "nlbac_env_reset_rows: n >= 1 lanes (got %d)", n);
    NLBAC_REQUIRE(state_dim >= 1 && state_dim <= 64 && obs_dim >= 1 && obs_dim <= 64,
                  "nlbac_env_reset_rows: 1 <= state_dim, obs_dim <= 64 (got %d, %d)", state_dim, obs_dim);
    NLBAC_REQUIRE(start_state && start_obs && state && ep_step && obs && obs32 && reset_count,
                  "nlbac_env_reset_rows: null pointer");
    hipLaunchKernelGGL(env_reset_rows_kernel, RESET_GRID(n), n, done, state_dim, obs_dim, start_state, start_obs,
                       start_last_dist, state, ep_step, last_dist, obs, obs32, reset_count);
    NLBAC_CHECK_LAUNCH("nlbac_env_reset_rows");
    return 0;
}

extern "C" int nlbac_cars_env_reset(int n, const int* done, unsigned long long seed, const double* noise, double* state,
                                    double* t, int* ep_step, double* obs, float* obs32, int* reset_count,
                                    double* reset_noise, nlbac_stream_t s) {
    NLBAC_REQUIRE(n >= 1, "nlbac_cars_env_reset: n >= 1 lanes (got %d)", n);
    NLBAC_REQUIRE(state && t && ep_step && obs && obs32 && reset_count && reset_noise,
                  "nlbac_cars_env_reset: null pointer");
    hipLaunchKernelGGL(cars_env_reset_kernel, RESET_GRID(n), n, done, seed, noise, state, t, ep_step, obs, obs32,
                       reset_count, reset_noise);
    NLBAC_CHECK_LAUNCH("nlbac_cars_env_reset");
    return 0;
}

extern "C" int nlbac_quadrotor_env_reset(int n, const int* done, unsigned long long seed,
                                         const double* params /* host: start state (6), spread in x, in z */,
                                         const double* noise, double* state, int* ep_step, double* obs, float* obs32,
                                         int* reset_count, double* reset_noise, nlbac_stream_t s) {
    NLBAC_REQUIRE(n >= 1, "nlbac_quadrotor_env_reset: n >= 1 lanes (got %d)", n);
    NLBAC_REQUIRE(params && state && ep_step && obs && obs32 && reset_count && reset_noise,
                  "nlbac_quadrotor_env_reset: null pointer");
    NLBAC_REQUIRE(params[6] >= 0.0 && params[7] >= 0.0,
                  "nlbac_quadrotor_env_reset: the spread is not negative (got %g, %g)", params[6], params[7]);
    QuadReset R = {{params[0], params[1], params[2], params[3], params[4], params[5]}, params[6], params[7]};
    hipLaunchKernelGGL(quadrotor_env_reset_kernel, RESET_GRID(n), n, done, seed, R, noise, state, ep_step, obs, obs32,
                       reset_count, reset_noise);
    NLBAC_CHECK_LAUNCH("nlbac_quadrotor_env_reset");
    return 0;
}

extern "C" int nlbac_unicycle_env_reset(int n, const int* done, unsigned long long seed,
                                        const double* params /* host: start state (3), start centre (2), goal (2),
                                        spread in x, in y */, const double* noise, double* state, int* ep_step,
                                        double* last_dist, double* obs, float* obs32, int* reset_count,
                                        double* reset_noise, nlbac_stream_t s) {
    NLBAC_REQUIRE(n >= 1, "nlbac_unicycle_env_reset: n >= 1 lanes (got %d)", n);
    NLBAC_REQUIRE(params && state && ep_step && last_dist && obs && obs32 && reset_count && reset_noise,
                  "nlbac_unicycle_env_reset: null pointer");
    NLBAC_REQUIRE(params[7] >= 0.0 && params[8] >= 0.0,
                  "nlbac_unicycle_env_reset: the spread is not negative (got %g, %g)", params[7], params[8]);
    UniReset R = {{params[0], params[1], params[2]}, params[3], params[4], params[5], params[6], params[7], params[8]};
    hipLaunchKernelGGL(unicycle_env_reset_kernel, RESET_GRID(n), n, done, seed, R, noise, state, ep_step, last_dist, obs,
                       obs32, reset_count, reset_noise);
    NLBAC_CHECK_LAUNCH("nlbac_unicycle_env_reset");
    return 0;
}

extern "C" int nlbac_pvtol_env_reset(int n, const int* done, unsigned long long seed,
                                     const double* params /* host: start state (7), goal (2), spread in x, in y */,
                                     const double* noise, double* state, int* ep_step, double* obs, float* obs32,
                                     int* reset_count, double* reset_noise, nlbac_stream_t s) {
    NLBAC_REQUIRE(n >= 1, "nlbac_pvtol_env_reset: n >= 1 lanes (got %d)", n);
    NLBAC_REQUIRE(params && state && ep_step && obs && obs32 && reset_count && reset_noise,
                  "nlbac_pvtol_env_reset: null pointer");
    NLBAC_REQUIRE(params[9] >= 0.0 && params[10] >= 0.0,
                  "nlbac_pvtol_env_reset: the spread is not negative (got %g, %g)", params[9], params[10]);
    PvReset R = {{params[0], params[1], params[2], params[3], params[4], params[5], params[6]}, params[7], params[8],
                 params[9], params[10]};
    hipLaunchKernelGGL(pvtol_env_reset_kernel, RESET_GRID(n), n, done, seed, R, noise, state, ep_step, obs, obs32,
                       reset_count, reset_noise);
    NLBAC_CHECK_LAUNCH("nlbac_pvtol_env_reset");
    return 0;
}
