// Per-episode ledger of the vectorised driver on the device (vector_episodes.EpisodeLedger; train.train_vectorized(
// episodes=...) and train.evaluate_vectorized): what the reference's main.py logs per episode — return, length, number
// of safety violations, safety cost — accumulated per lane from the simulators' own outputs, and one fixed-width record
// per finished episode appended to a ring in lane order.  include/nlbac_hip.h has the contract of every array.
//
// The float64 sums are plain sequential adds in step order (acc = acc + x; there is no product to contract), so they
// are the bits a host loop over the same numbers gets.  The order of the log is integer arithmetic: ballot popcounts
// and a sum over the workgroups' counts, as handover_kernels.hip ranks the kept rows — no atomics, no election.
#include <cstdint>
#include "common.h"

enum { ED_RET = 0, ED_COST, ED_VIOL, ED_LIFE_RET, ED_LIFE_COST, ED_LIFE_VIOL, ED_INFO0, ED_N };
enum { EI_LEN = 0, EI_BACKUP, EI_LIFE_STEPS, EI_LIFE_BACKUP, EI_EPISODES, EI_N };
static_assert(ED_N == NLBAC_EPISODE_DSTATE && EI_N == NLBAC_EPISODE_ISTATE, "state rows");
static_assert(sizeof(nlbac_episode_record) == 64 && alignof(nlbac_episode_record) == 16, "a record is four 16-byte units");

__global__ __launch_bounds__(256) void episode_step_kernel(int n, const double* __restrict__ reward,
                                                           const double* __restrict__ info0, int info_ld,
                                                           const int* __restrict__ done, const int* __restrict__ ep_step,
                                                           int max_steps, const unsigned char* __restrict__ flags,
                                                           double* __restrict__ dstate, int* __restrict__ istate,
                                                           unsigned char* __restrict__ fin, int* __restrict__ counts) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    bool dn = false;
    if (i < n) {
        const double* inf = info0 + (long)i * info_ld;
        double* d = dstate + i;
        int* s = istate + i;
        d[(long)ED_RET * n] = d[(long)ED_RET * n] + reward[i];
        d[(long)ED_VIOL * n] = d[(long)ED_VIOL * n] + inf[1];
        d[(long)ED_COST * n] = d[(long)ED_COST * n] + inf[2];
        d[(long)ED_INFO0 * n] = inf[0];
        s[(long)EI_LEN * n] += 1;
        if (flags && flags[i] != 0) s[(long)EI_BACKUP * n] += 1;
        dn = done[i] != 0;
        fin[i] = dn ? (unsigned char)(1 | (ep_step[i] >= max_steps ? 2 : 0)) : (unsigned char)0;
    }
    __shared__ int s_cnt[4];
    const unsigned long long m = __ballot(dn);
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
}

extern "C" int nlbac_episode_step(int n, const double* reward, const double* info0, int info_ld, const int* done,
                                  const int* ep_step, int max_steps, const unsigned char* flags, double* dstate,
                                  int* istate, unsigned char* fin, int* counts, nlbac_stream_t s) {
    NLBAC_REQUIRE(reward && info0 && done && ep_step && dstate && istate && fin && counts,
                  "nlbac_episode_step: null pointer");
    NLBAC_REQUIRE(n >= 1 && n <= 65536, "nlbac_episode_step: 1 <= n <= 65536 lanes (got %d)", n);
    NLBAC_REQUIRE(info_ld >= 3, "nlbac_episode_step: info rows hold 3 doubles, info_ld >= 3 (got %d)", info_ld);
    NLBAC_REQUIRE(max_steps >= 1, "nlbac_episode_step: max_steps >= 1 (got %d)", max_steps);
    hipLaunchKernelGGL(episode_step_kernel, dim3((unsigned)nlbac_ceil_div(n, 256)), dim3(256), 0, (hipStream_t)s, n, reward,
                       info0, info_ld, done, ep_step, max_steps, flags, dstate, istate, fin, counts);
    NLBAC_CHECK_LAUNCH("nlbac_episode_step");
    return 0;
}

__device__ __forceinline__ int episode_wave_sum(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

__global__ __launch_bounds__(256) void episode_append_kernel(int n, const unsigned char* __restrict__ fin,
                                                             const int* __restrict__ counts, int n_wg,
                                                             double* __restrict__ dstate, int* __restrict__ istate,
                                                             nlbac_episode_record* __restrict__ ring, long cap, long* head,
                                                             int half, int vstep, int updates) {
    __shared__ int s_wave[4], s_pre[4], s_tot[4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int i = blockIdx.x * 256 + t;
    const int c = t < n_wg ? counts[t] : 0;
    const int pre = episode_wave_sum(t < (int)blockIdx.x ? c : 0), tot = episode_wave_sum(c);
    const unsigned char f = i < n ? fin[i] : (unsigned char)0;
    const bool dn = f != 0;
    const unsigned long long m = __ballot(dn);
    if (lane == 0) s_wave[wave] = __popcll(m), s_pre[wave] = pre, s_tot[wave] = tot;
    __syncthreads();
    long pos = head[2 * half], written = head[2 * half + 1];
    if (pos < 0 || pos >= cap) pos = 0;                  // (never form a record outside the ring from a head nobody set)
    if (written < 0) written = 0;
    const long total = (s_tot[0] + s_tot[1]) + (s_tot[2] + s_tot[3]);
    if (dn) {
        int rank = __popcll(m & ((1ull << lane) - 1ull));
        for (int w = 0; w < wave; ++w) rank += s_wave[w];
        const long off = (s_pre[0] + s_pre[1]) + (s_pre[2] + s_pre[3]);
        double* d = dstate + i;
        int* s = istate + i;
        nlbac_episode_record r;
        r.ret = d[(long)ED_RET * n], r.safety_cost = d[(long)ED_COST * n], r.violations = d[(long)ED_VIOL * n];
        r.info0 = d[(long)ED_INFO0 * n];
        r.length = s[(long)EI_LEN * n], r.lane = i, r.lane_episode = s[(long)EI_EPISODES * n];
        r.vstep = vstep, r.updates = updates, r.timeout = (f & 2) ? 1 : 0, r.backup_steps = s[(long)EI_BACKUP * n];
        r.reserved = 0;
        ring[(pos + off + rank) % cap] = r;
        d[(long)ED_LIFE_RET * n] = d[(long)ED_LIFE_RET * n] + r.ret;
        d[(long)ED_LIFE_COST * n] = d[(long)ED_LIFE_COST * n] + r.safety_cost;
        d[(long)ED_LIFE_VIOL * n] = d[(long)ED_LIFE_VIOL * n] + r.violations;
        d[(long)ED_RET * n] = 0.0, d[(long)ED_COST * n] = 0.0, d[(long)ED_VIOL * n] = 0.0;
        s[(long)EI_LIFE_STEPS * n] += r.length;
        s[(long)EI_LIFE_BACKUP * n] += r.backup_steps;
        s[(long)EI_EPISODES * n] = r.lane_episode + 1;
        s[(long)EI_LEN * n] = 0, s[(long)EI_BACKUP * n] = 0;
    }
    if (blockIdx.x == 0 && t == 0) {
        head[2 * (1 - half)] = (pos + total) % cap;
        head[2 * (1 - half) + 1] = written + total;
    }
}

extern "C" int nlbac_episode_append(int n, const unsigned char* fin, const int* counts, double* dstate, int* istate,
                                    nlbac_episode_record* ring, long capacity, long* head, int half, int vstep, int updates,
                                    nlbac_stream_t s) {
    NLBAC_REQUIRE(fin && counts && dstate && istate && ring && head, "nlbac_episode_append: null pointer");
    NLBAC_REQUIRE(n >= 1 && n <= 65536, "nlbac_episode_append: 1 <= n <= 65536 lanes (got %d)", n);
    NLBAC_REQUIRE(capacity >= n, "nlbac_episode_append: n (%d) exceeds the ring's capacity (%ld)", n, capacity);
    NLBAC_REQUIRE(half == 0 || half == 1, "nlbac_episode_append: half is 0 or 1");
    NLBAC_REQUIRE(((uintptr_t)ring % 16) == 0 && ((uintptr_t)head % 8) == 0,
                  "nlbac_episode_append: the ring must be aligned to 16 bytes (records are whole 16-byte units)");
    NLBAC_REQUIRE(vstep >= 0 && updates >= 0, "nlbac_episode_append: vstep and updates count up from 0");
    const int n_wg = nlbac_ceil_div(n, 256);
    hipLaunchKernelGGL(episode_append_kernel, dim3((unsigned)n_wg), dim3(256), 0, (hipStream_t)s, n, fin, counts, n_wg, dstate,
                       istate, ring, capacity, head, half, vstep, updates);
    NLBAC_CHECK_LAUNCH("nlbac_episode_append");
    return 0;
}
