// Backup-controller hand-over of the vectorised driver on the device (train.train_vectorized(handover=...)): the
// per-lane state machines of train._UnicycleHandover / _CarsHandover / _PvtolHandover (U/main.py:39-142,
// C/main.py:41-112, P/main.py:40-200), the fused assembly of a vector step's transition rows, the order-preserving
// compaction of the rows the primary controller produced into the controller replay, and the minibatch draw that
// reads that replay's length from device memory.  include/nlbac_hip.h has the contract of every array.
//
// The decisions are float64 on the simulators' float64 outputs, the host classes' operations in their order, every
// product and sum rounded on its own: a fused multiply-add would round `moved` differently from numpy and could flip a
// comparison against its threshold.  What keeps them apart is the pragma below, which covers every function DEFINED
// after it — so the arithmetic is written out here with plain * + -.  (HIP's __dmul_rn / __dadd_rn are plain operators
// in a header compiled before the pragma, under the default contraction mode: wrapped in them, the products and sums
// were fused again.  tests/test_vector_handover_gpu.py has a case that a contracted build fails.)
#include <cstdint>
#include "common.h"
#include "philox.h"
#pragma clang fp contract(off)

enum { HS_B0 = 0, HS_B1, HS_T0, HS_T1, HS_V0, HS_V1, HS_EPISODES, HS_ALLOWED, HS_BACKUP_STEPS, HS_N };
static_assert(HS_N == NLBAC_HANDOVER_ISTATE, "istate rows");

struct LaneState {
    int b0, b1, t0, t1, v0, v1, episodes, allowed, backup_steps;
    double x0, y0;
};

__device__ __forceinline__ double sq2(double dx, double dy) { return dx * dx + dy * dy; }   // (three roundings)

__device__ __forceinline__ bool use_backup(const nlbac_handover_params& P, const LaneState& S) {
    return (S.b0 && S.allowed) || (P.kind == 2 && S.b1 && S.allowed);
}

__device__ __forceinline__ void begin_episode(const nlbac_handover_params& P, LaneState& S) {
    if (S.episodes >= P.first_backup_episode) S.allowed = 1;
    S.b0 = S.b1 = S.t0 = S.t1 = S.v0 = S.v1 = 0;
    S.x0 = S.y0 = 0.0;
}

__device__ __forceinline__ void on_backup_action(const nlbac_handover_params& P, LaneState& S) {
    S.backup_steps += 1;
    if (P.kind != 2) {
        S.t0 += 1;
    } else if (S.b0 && S.b1) {
        S.t0 += 1;
        S.t1 += 1;
    } else if (S.b0 && !S.b1) {
        S.t0 += 1;
    } else {
        S.t1 += 1;
    }
}

// moved^2 of the look-ahead point / the vehicle over the look-back, after this step's position went into the ring
__device__ __forceinline__ double ring_moved(const nlbac_handover_params& P, double* ring, int n, int i, int k, double x,
                                             double y) {
    const int D = NLBAC_HANDOVER_RING;
    const int cur = ((k - 1) % D + D) % D;
    ring[(long)(2 * cur) * n + i] = x;
    ring[(long)(2 * cur + 1) * n + i] = y;
    if (k < P.min_check_step) return 0.0;
    const int old = ((k - P.lookback) % D + D) % D;
    const double ox = old == cur ? x : ring[(long)(2 * old) * n + i];
    const double oy = old == cur ? y : ring[(long)(2 * old + 1) * n + i];
    return sq2(x - ox, y - oy);
}

// The stuck (Unicycle) / trapped (Pvtol) hand-over, the same lines in both host classes: `checks` checks in a row that
// find moved^2 <= stuck2 hand over; max_backup steps or away2 from the hand-over point hand back.  False before the
// first check of an episode (the host's early return).
__device__ __forceinline__ bool stuck_check(const nlbac_handover_params& P, LaneState& S, double* ring, int n, int i, int k,
                                            const double* nx) {
    const double moved = ring_moved(P, ring, n, i, k, nx[0], nx[1]);
    if (k < P.min_check_step) return false;
    if (S.allowed && !S.b0) {
        if (moved <= P.stuck2) {
            S.v0 += 1;
            if (S.v0 >= P.checks) {
                S.b0 = 1, S.v0 = 0;
                S.x0 = nx[0], S.y0 = nx[1];
            }
        }
        if (moved > P.stuck2 && S.v0 > 0) S.v0 = 0;
    }
    if (S.b0 && S.allowed) {
        if (S.t0 >= P.max_backup) S.b0 = 0, S.t0 = 0;
        if (sq2(nx[0] - S.x0, nx[1] - S.y0) >= P.away2) S.b0 = 0, S.t0 = 0;
    }
    return true;
}

__device__ __forceinline__ void after_step(const nlbac_handover_params& P, LaneState& S, double* ring, int n, int i, int k,
                                           const double* pv, const double* nx, const double* nobs, double info0) {
    if (P.kind == 0) {                                   // train._UnicycleHandover.after_step
        if (!stuck_check(P, S, ring, n, i, k, nx)) return;
    } else if (P.kind == 1) {                            // train._CarsHandover.after_step
        const double d34 = nobs[4] * 100.0 - nobs[6] * 100.0;
        const double d45 = nobs[6] * 100.0 - nobs[8] * 100.0;
        if (S.allowed && !S.b0) {
            if (d45 < P.gap && info0 != 0.0) S.b0 = 1;
        }
        if (S.b0 && S.allowed) {
            if (S.t0 >= P.max_backup) S.b0 = 0, S.t0 = 0;
            if (S.t0 >= P.min_backup && d34 > P.gap && d45 > P.gap) S.b0 = 0, S.t0 = 0;
        }
    } else {                                             // train._PvtolHandover.after_step
        if (!stuck_check(P, S, ring, n, i, k, nx)) return;
        const double vx = nx[0] - pv[0], ahead = nx[0] - nx[7], behind = nx[7] - nx[0];
        const bool running = (nx[0] <= P.x_mid && vx > 0.0 && ahead > P.operator_dist) ||
                             (nx[0] > P.x_mid && vx < 0.0 && behind > P.operator_dist);
        if (S.allowed && !S.b1) {
            if (running) {
                S.v1 += 1;
                if (S.v1 >= P.run_checks) S.b1 = 1, S.v1 = 0;
            }
            if (!running && S.v1 > 0) S.v1 = 0;
        }
        if (S.b1 && S.allowed) {
            if (S.t1 >= P.run_max_backup) S.b1 = 0, S.t1 = 0;
            const double back = P.back_frac * P.operator_dist;
            if ((nx[0] <= P.x_mid && ahead <= back) || (nx[0] > P.x_mid && behind <= back)) S.b1 = 0, S.t1 = 0;
        }
    }
}

struct StepArgs {
    int n;
    nlbac_handover_params P;
    nlbac_row_layout L;
    const double *lya_pre, *lya_next, *obs_next, *reward, *constraint, *info0;
    int info_ld;
    const int *done, *ep_step;
    const float *obs_prev, *action;
    float dt;
    int max_steps;
    float* node_ring;
    long node_first, node_cap;
    double* pos_ring;
    int* istate;
    double* dstate;
    unsigned char *flags, *kept;
    int* counts;
};

__global__ __launch_bounds__(256) void vector_step_rows_kernel(const StepArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x, n = a.n;
    const nlbac_handover_params& P = a.P;
    const nlbac_row_layout& L = a.L;
    bool keep = false;
    if (i < n) {
        LaneState S;
        int* st = a.istate + i;
        S.b0 = st[(long)HS_B0 * n], S.b1 = st[(long)HS_B1 * n], S.t0 = st[(long)HS_T0 * n], S.t1 = st[(long)HS_T1 * n];
        S.v0 = st[(long)HS_V0 * n], S.v1 = st[(long)HS_V1 * n], S.episodes = st[(long)HS_EPISODES * n];
        S.allowed = st[(long)HS_ALLOWED * n], S.backup_steps = st[(long)HS_BACKUP_STEPS * n];
        S.x0 = a.dstate[i], S.y0 = a.dstate[(long)n + i];
        const bool flag = a.flags[i] != 0;               // (what the last call left: use_backup of the state)
        keep = !flag;
        const int k = a.ep_step[i];
        const bool dn = a.done[i] != 0;
        const double* pv = a.lya_pre + (long)i * L.lya_dim;
        const double* nx = a.lya_next + (long)i * L.lya_dim;
        const double* nobs = a.obs_next + (long)i * L.obs_dim;
        if (a.node_ring) {                               // (a) the row, in train_vectorized's float32 roundings
            float* row = a.node_ring + ((a.node_first + i) % a.node_cap) * L.ld;
            for (int c = 0; c < L.ld; ++c) row[c] = 0.f;
            for (int c = 0; c < L.obs_dim; ++c) row[L.obs + c] = a.obs_prev[(long)i * L.obs_dim + c];
            for (int c = 0; c < L.act_dim; ++c) row[L.act + c] = a.action[(long)i * L.act_dim + c];
            row[L.rew] = (float)a.reward[i];
            row[L.con] = (float)a.constraint[i];
            for (int c = 0; c < L.lya_dim; ++c) row[L.lya + c] = (float)pv[c];
            for (int c = 0; c < L.lya_dim; ++c) row[L.nlya + c] = (float)nx[c];
            for (int c = 0; c < L.obs_dim; ++c) row[L.nobs + c] = (float)nobs[c];
            row[L.mask] = k >= a.max_steps ? 1.f : (dn ? 0.f : 1.f);
            const float tf = (float)k;
            row[L.t] = tf * a.dt;
            row[L.nt] = (tf + 1.f) * a.dt;
        }
        if (a.kept) a.kept[i] = keep ? 1 : 0;            // (b)
        if (flag) on_backup_action(P, S);                // (c)
        after_step(P, S, a.pos_ring, n, i, k, pv, nx, nobs, a.info0[(long)i * a.info_ld]);
        if (dn) {
            S.episodes += 1;
            begin_episode(P, S);
        }
        st[(long)HS_B0 * n] = S.b0, st[(long)HS_B1 * n] = S.b1, st[(long)HS_T0 * n] = S.t0, st[(long)HS_T1 * n] = S.t1;
        st[(long)HS_V0 * n] = S.v0, st[(long)HS_V1 * n] = S.v1, st[(long)HS_EPISODES * n] = S.episodes;
        st[(long)HS_ALLOWED * n] = S.allowed, st[(long)HS_BACKUP_STEPS * n] = S.backup_steps;
        a.dstate[i] = S.x0, a.dstate[(long)n + i] = S.y0;
        a.flags[i] = use_backup(P, S) ? 1 : 0;           // (d)
    }
    __shared__ int s_cnt[4];
    const unsigned long long m = __ballot(keep);
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0 && a.counts) a.counts[blockIdx.x] = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
}

extern "C" int nlbac_vector_step_rows(int n, const nlbac_handover_params* p, const nlbac_row_layout* lay,
                                      const double* lya_pre, const double* lya_next, const double* obs_next,
                                      const double* reward, const double* constraint, const double* info0, int info_ld,
                                      const int* done, const int* ep_step, const float* obs_prev, const float* action,
                                      double dt, int max_steps, float* node_ring, long node_first, long node_cap,
                                      double* pos_ring, int* istate, double* dstate, unsigned char* flags,
                                      unsigned char* kept, int* counts, nlbac_stream_t s) {
    NLBAC_REQUIRE(p && lay && lya_pre && lya_next && obs_next && info0 && done && ep_step && istate && dstate && flags,
                  "nlbac_vector_step_rows: null pointer");
    NLBAC_REQUIRE(n >= 1 && n <= 65536 && info_ld >= 1, "nlbac_vector_step_rows: 1 <= n <= 65536 lanes (got %d)", n);
    NLBAC_REQUIRE(p->kind >= 0 && p->kind <= 2, "nlbac_vector_step_rows: kind %d", p->kind);
    NLBAC_REQUIRE(p->lookback >= 1 && p->lookback <= NLBAC_HANDOVER_RING && p->min_check_step >= p->lookback,
                  "nlbac_vector_step_rows: 1 <= lookback <= %d <= ... and min_check_step >= lookback (got %d, %d)",
                  NLBAC_HANDOVER_RING, p->lookback, p->min_check_step);
    NLBAC_REQUIRE(lay->obs_dim >= 1 && lay->lya_dim >= 1 && lay->act_dim >= 1, "nlbac_vector_step_rows: bad dimensions");
    NLBAC_REQUIRE(p->kind != 0 || lay->lya_dim >= 2, "nlbac_vector_step_rows: Unicycle reads 2 Lyapunov inputs");
    NLBAC_REQUIRE(p->kind != 1 || lay->obs_dim >= 9, "nlbac_vector_step_rows: SimulatedCars reads observation 8");
    NLBAC_REQUIRE(p->kind != 2 || lay->lya_dim >= 8, "nlbac_vector_step_rows: Pvtol reads Lyapunov input 7");
    NLBAC_REQUIRE(p->kind == 1 || pos_ring, "nlbac_vector_step_rows: this kind needs the position ring");
    if (node_ring) {
        NLBAC_REQUIRE(reward && constraint && obs_prev && action, "nlbac_vector_step_rows: null pointer (row inputs)");
        NLBAC_REQUIRE(node_cap >= n && node_first >= 0 && node_first < node_cap,
                      "nlbac_vector_step_rows: n <= node_cap and 0 <= node_first < node_cap");
        const int cols[10] = {lay->obs, lay->act, lay->rew, lay->con, lay->lya, lay->nlya, lay->nobs, lay->mask, lay->t, lay->nt};
        const int wid[10] = {lay->obs_dim, lay->act_dim, 1, 1, lay->lya_dim, lay->lya_dim, lay->obs_dim, 1, 1, 1};
        for (int c = 0; c < 10; ++c)
            NLBAC_REQUIRE(cols[c] >= 0 && cols[c] + wid[c] <= lay->ld, "nlbac_vector_step_rows: column %d leaves the row", c);
    }
    StepArgs a;
    a.n = n, a.P = *p, a.L = *lay;
    a.lya_pre = lya_pre, a.lya_next = lya_next, a.obs_next = obs_next, a.reward = reward, a.constraint = constraint;
    a.info0 = info0, a.info_ld = info_ld, a.done = done, a.ep_step = ep_step, a.obs_prev = obs_prev, a.action = action;
    a.dt = (float)dt, a.max_steps = max_steps, a.node_ring = node_ring, a.node_first = node_first, a.node_cap = node_cap;
    a.pos_ring = pos_ring, a.istate = istate, a.dstate = dstate, a.flags = flags, a.kept = kept, a.counts = counts;
    hipLaunchKernelGGL(vector_step_rows_kernel, dim3((unsigned)nlbac_ceil_div(n, 256)), dim3(256), 0, (hipStream_t)s, a);
    NLBAC_CHECK_LAUNCH("nlbac_vector_step_rows");
    return 0;
}

// ---------------------------------------------------------------------------
// Compaction of the kept rows into the controller ring, in lane order.  Rank of a kept lane = kept lanes of the
// workgroups before it (a sum over counts[], <= 256 reads) + of the waves before it + of the lower lanes of its wave
// (ballot popcounts): integers, no atomics, the same in any execution order.
// ---------------------------------------------------------------------------
__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

__global__ __launch_bounds__(256) void ring_append_kept_kernel(int n, const unsigned char* __restrict__ kept,
                                                               const int* __restrict__ counts, int n_wg,
                                                               const float4* __restrict__ node, long node_first,
                                                               long node_cap, float4* __restrict__ ring, long cap, int ld4,
                                                               long* head, int half, const int* __restrict__ ep_step,
                                                               int shift, float dt, int t_col, int nt_col) {
    __shared__ int s_wave[4], s_pre[4], s_tot[4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int i = blockIdx.x * 256 + t;
    const int c = t < n_wg ? counts[t] : 0;
    const int pre = wave_sum_int(t < (int)blockIdx.x ? c : 0), tot = wave_sum_int(c);
    const bool keep = i < n && kept[i] != 0;
    const unsigned long long m = __ballot(keep);
    if (lane == 0) s_wave[wave] = __popcll(m), s_pre[wave] = pre, s_tot[wave] = tot;
    __syncthreads();
    long pos = head[2 * half], len = head[2 * half + 1];
    if (pos < 0 || pos >= cap) pos = 0;                  // (never form a row outside the ring from a head nobody set)
    if (len < 0) len = 0;
    const long total = (s_tot[0] + s_tot[1]) + (s_tot[2] + s_tot[3]);
    if (keep) {
        int rank = __popcll(m & ((1ull << lane) - 1ull));
        for (int w = 0; w < wave; ++w) rank += s_wave[w];
        const long off = (s_pre[0] + s_pre[1]) + (s_pre[2] + s_pre[3]);
        const float4* src = node + ((node_first + i) % node_cap) * ld4;
        float4* dst = ring + ((pos + off + rank) % cap) * ld4;
        for (int q = 0; q < ld4; ++q) dst[q] = src[q];
        if (shift != 0) {
            const float tf = (float)(ep_step[i] + shift);
            ((float*)dst)[t_col] = tf * dt;
            ((float*)dst)[nt_col] = (tf + 1.f) * dt;
        }
    }
    if (blockIdx.x == 0 && t == 0) {
        head[2 * (1 - half)] = (pos + total) % cap;
        head[2 * (1 - half) + 1] = len + total < cap ? len + total : cap;
    }
}

extern "C" int nlbac_ring_append_kept(int n, const unsigned char* kept, const int* counts, const float* node_ring,
                                      long node_first, long node_cap, float* ring, long cap, int ld, long* head, int half,
                                      const int* ep_step, int shift, double dt, int t_col, int nt_col, nlbac_stream_t s) {
    NLBAC_REQUIRE(kept && counts && node_ring && ring && head && ep_step, "nlbac_ring_append_kept: null pointer");
    NLBAC_REQUIRE(n >= 1 && n <= 65536, "nlbac_ring_append_kept: 1 <= n <= 65536 lanes (got %d)", n);
    NLBAC_REQUIRE(cap >= n && node_cap >= n, "nlbac_ring_append_kept: n (%d) exceeds a ring's capacity", n);
    NLBAC_REQUIRE(node_first >= 0 && node_first < node_cap, "nlbac_ring_append_kept: 0 <= node_first < node_cap");
    NLBAC_REQUIRE(half == 0 || half == 1, "nlbac_ring_append_kept: half is 0 or 1");
    NLBAC_REQUIRE(ld >= 4 && ld % 4 == 0 && ((uintptr_t)node_ring % 16) == 0 && ((uintptr_t)ring % 16) == 0,
                  "nlbac_ring_append_kept: rows must be whole float4s (ld %d)", ld);
    NLBAC_REQUIRE(t_col >= 0 && t_col < ld && nt_col >= 0 && nt_col < ld, "nlbac_ring_append_kept: stamp columns");
    const int n_wg = nlbac_ceil_div(n, 256);
    hipLaunchKernelGGL(ring_append_kept_kernel, dim3((unsigned)n_wg), dim3(256), 0, (hipStream_t)s, n, kept, counts, n_wg,
                       (const float4*)node_ring, node_first, node_cap, (float4*)ring, cap, ld / 4, head, half, ep_step,
                       shift, (float)dt, t_col, nt_col);
    NLBAC_CHECK_LAUNCH("nlbac_ring_append_kept");
    return 0;
}

// nlbac_sample_rows with the ring's length read from the head in device memory
__global__ __launch_bounds__(256) void sample_rows_head_kernel(const float4* __restrict__ src, const long* __restrict__ head,
                                                               int half, long cap, int ld4, long n_rows,
                                                               float4* __restrict__ dst, float* __restrict__ eps,
                                                               long n_eps, unsigned long long seed,
                                                               unsigned long long draw) {
    long len = head[2 * half + 1];
    len = len < 0 ? 0 : (len > cap ? cap : len);
    sample_rows_body((long)blockIdx.x * 256 + threadIdx.x, src, ld4, n_rows, len, dst, eps, n_eps, seed, draw);
}

extern "C" int nlbac_sample_rows_head(const float* src, const long* head, int half, long cap, int ld, long n_rows,
                                      float* dst, float* eps, long n_eps, unsigned long long seed,
                                      unsigned long long draw, nlbac_stream_t s) {
    NLBAC_REQUIRE(src && head && dst && cap >= 1 && cap < (1L << 32) && n_rows >= 1 && n_eps >= 0 && (half == 0 || half == 1),
                  "nlbac_sample_rows_head: bad arguments");
    NLBAC_REQUIRE(ld >= 4 && ld % 4 == 0 && ((uintptr_t)src % 16) == 0 && ((uintptr_t)dst % 16) == 0,
                  "nlbac_sample_rows_head: rows must be whole float4s (ld %d)", ld);
    NLBAC_REQUIRE(eps || n_eps == 0, "nlbac_sample_rows_head: n_eps without a buffer");
    const long total = n_rows * (ld / 4), q = (n_eps + 3) / 4;
    const long threads = total > q ? total : q;
    hipLaunchKernelGGL(sample_rows_head_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)s,
                       (const float4*)src, head, half, cap, ld / 4, n_rows, (float4*)dst, eps, n_eps, seed, draw);
    NLBAC_CHECK_LAUNCH("nlbac_sample_rows_head");
    return 0;
}
