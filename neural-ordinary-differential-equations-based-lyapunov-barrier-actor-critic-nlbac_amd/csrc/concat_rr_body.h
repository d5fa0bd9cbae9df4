// Bodies of the register-resident fused RK kernels of the single-net NODE  dx/dt = net([x | c]): the one-step kernels of
// concat_rr_kernels.hip (TRAJ = false) and the one-launch fixed-grid rollout of concat_traj_kernels.hip (TRAJ = true),
// which carries a wave's 16 rows through H intervals of the same step.  What the two launchers share sits here too.
#pragma once
#include "concat_rk_shared.h"
#include "rr_device.h"
#include <type_traits>

#define CRR_MAX_IN 15       /* in_dim + the bias column <= 16: four k-steps of layer 0 */

// this lane's state component in register r: c = 4 r + q (the layout of layer 0's B operand and of the output block)
#ifdef RR_TIMING
#define CSTAMP(slot_) if (L.err && blockIdx.x == 0 && lane == 0) reinterpret_cast<long long*>(L.err)[half * 256 + (slot_)] = (long long)__builtin_readcyclecounter();
#define BSTAMP(slot_) if (L.dyn && !L.norm && blockIdx.x == 0 && lane == 0) reinterpret_cast<long long*>(L.dyn)[half * 256 + (slot_)] = (long long)__builtin_readcyclecounter();
#else
#define CSTAMP(slot_)
#define BSTAMP(slot_)
#endif
// the step's result for (row mm of the tile, component r):  y0 + sum_j K_j (c_out[j] h)  in rk_combine_kernel's op order
template <int TILE>
__device__ __forceinline__ float crr_step_output(const ConcatRkLaunch& L, const float* sY0, const float* sK, int mm, int r, float h) {
    float a = sY0[mm * CK_LD + r];
    for (int j = 0; j < L.n_out; ++j)
        if (L.c_out[j] != 0.f) a = a + sK[(j * TILE + mm) * CK_LD + r] * (L.c_out[j] * h);
    return a;
}

// NW: waves per workgroup (2 or 4: 32- or 64-row tiles).  Four where the problems' row counts allow it (a tile must not
// straddle two problems of a device-driven chain): of two 2-wave workgroups on one CU the hardware puts two waves on the
// same SIMD and leaves one SIMD empty (tools/micro/wave_place.hip: 512 workgroups x 128 threads use 768 of the 1024 SIMDs,
// 256 of them twice) — the doubled-up waves ran a stage in 11-13k cycles against 8.2k, and the launch waits for them.
// TRAJ: a whole fixed-grid rollout (concat_traj_kernels.hip), intervals k = 0 .. H-1 in one launch.  Interval k is the
// one-step launch's step through the same code: carried columns L.c + k n n_c, stage index k S + st of H S stages in
// the [k][stage][row] layout of the mask words / activation rows / stage-input rows (L.Xn, here written for an
// un-normalised net too; K and Y rows are not written), its result to L.out + k n n_s and, as interval k+1's y0, to
// sY0 — by the wave that owns the rows, so that no barrier enters the interval loop.  The dopri5 machinery (control
// block, slots, FSAL, interpolant, norms, tickets) is compiled out.  TRAJ = false (H = 1): the one-step kernel.
// GRID (with TRAJ; nlbac_concat_rk_grid_fwd: the solution on a time grid): interval k's step size is hs[k] (device
// array), written to sH by the wave that owns the rows at the top of the interval, and the carried columns L.c [n][n_c]
// are the same for every interval (sC is filled once).
// SUB (with GRID; nlbac_concat_rk_subgrid_fwd: a time grid under step_size): the intervals are the N fine intervals, and
// L.out takes the T - 1 output points read off them (NlbacSubGrid, common.h): out[j-1] for the outputs j of interval k,
// written by the lane that holds the old state and the new one, before sY0 is overwritten.
// HOLD (with GRID, not SUB; nlbac_concat_rk_hold_fwd: a rollout under step_size): H = N fine intervals, hm of them per
// control interval, i = k hm + r: the step size is hs[r], the carried columns L.c + k n n_c are held in sC through the
// control interval and replaced behind r = hm-1 (TRAJ's hand-over, every hm-th fine interval), and L.out + k n n_s is
// written there only.
template <int NB, int R, int BITS, int NW, bool TRAJ = false, bool GRID = false, bool SUB = false, bool HOLD = false>
__device__ __forceinline__ void concat_rr_fwd_body(const ConcatRkLaunch& L, const int H = 1, const float* hs = nullptr,
                                                   const NlbacSubGrid* sub = nullptr, const int hm = 1) {
    static_assert(TRAJ || !GRID, "a time grid is a trajectory");
    static_assert(GRID || !SUB, "sub-steps are a time grid's");
    static_assert((GRID && !SUB) || !HOLD, "a held control's fine steps are a time grid's, its outputs their end points");
    constexpr int TILE = 16 * NW, NTHR = 64 * NW;
    (void)NTHR;
    using S = RRShape<NB, R>;
    constexpr int KS = S::KS, HID = S::HID, TB = NB - 2, NT = KS - 4 * TB, G0 = rr_group_first(NB);
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int half = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = L.n, ns = L.n_s, nc = L.n_c;
    const int row0 = blockIdx.x * TILE;
    const int p_tile = row0 / L.rpp;
    long soff = 0;
    bool fsal = false, ip = false;
    float ip_x = 0.f;
    if (!TRAJ && L.ctl) {
        const double* c = L.ctl + (long)p_tile * NLBAC_DOPRI_CTL;
        if (c[C_DONE] > 0.0) return;              // (uniform) this problem's solve has finished
        const int slot = (int)c[C_NACC];
        soff = (long)slot * L.slot_floats;
        fsal = slot > 0;
        if (L.ip_out) {          // this attempt reaches t_end: it also evaluates the solve's result (node_rk_shared.h::rk_fwd_where)
            const double t = c[C_T], hd = c[C_H];
            ip = t + hd >= L.t_end;
            ip_x = (float)((L.t_end - t) / hd);
        }
    }
    float* const gK = TRAJ ? nullptr : L.K + soff;
    float* const gY = TRAJ ? nullptr : L.Y + soff;
    float* const gErr = (!TRAJ && L.err) ? L.err + soff : nullptr;
    float* const gXn = L.Xn ? L.Xn + soff : nullptr;
    const float* const gy0 = fsal ? (gY - L.slot_floats) + (long)(L.S_total - 1) * n * ns : L.y0;
    const nlbac_mlp& net = L.net;
    const int idim = net.in_dim;
    const int n_rows = min(TILE, n - row0);
    const int q = lane >> 4, r16 = lane & 15, m = 16 * half + r16, grow = row0 + m;
    const bool row_ok = grow < n;
    const int KS0 = (ns + 3) >> 2;      // registers per row of state (layer 0 always runs four k-steps over [x | c | 1 | 0..])
    const float* const params = net.params;
    float* const acts = L.acts ? L.acts + soff : nullptr;
    const long acts_ls = L.acts_ls;
    const float* const nrm = L.norm;
    const int stage_end = L.stage_end;

    float* sK = smem;                                               // [stage][32][CK_NS]
    float* sY0 = sK + CK_MAX_STAGES * TILE * CK_LD;       // [32][CK_NS]
    float* sC = sY0 + TILE * CK_LD;                       // [32][CK_NC]
    float* sH = sC + TILE * CK_NC;                        // [32]
    float* sW0 = sH + TILE;                               // [k-step < 4][block < 8][lane]: layer 0's A fragments

    // ---- the wave's weight stream: hid x hid layers 1, 2, then 1 again (next stage)
    const __amdgpu_buffer_rsrc_t rs = rr_rsrc(net.packed, net.packed_floats);
    const int voff = lane * 16, wbase = net.rr_fwd_off * 4;
    RRGemm<S> gemm;
    CSTAMP(0)
    gemm.prime(rs, voff, wbase);

    // ---- constants: layer 0's A fragments over [x | c | 1] (bias in the column behind the inputs) -> LDS, the output
    //      layer's into registers (A row 4 q' + r' computes state component 4 r' + q')
    {       // (the workgroup's waves share the job: k-step k0 by wave k0 mod NW)
        const float* W0 = params + net.w_off[0];
        const float* b0 = params + net.b_off[0];
#pragma unroll
        for (int kk = 0; kk < 4 / NW; ++kk)
#pragma unroll
            for (int jo = 0; jo < NB; ++jo) {
                const int k0 = half + NW * kk;
                const int uo = rr_unit_out(NB, R, jo, r16), col = 4 * k0 + q, uc = max(uo, 0);
                const float vw = W0[uc * idim + min(col, idim - 1)], vb0 = b0[uc];
                sW0[(k0 * 8 + jo) * 64 + lane] = (uo < 0 || col > idim) ? 0.f : (col < idim ? vw : vb0);
            }
    }
    float wo[KS];
    {
        const int cq = 4 * (r16 & 3) + (r16 >> 2);
        const bool ok = (r16 & 3) < KS0 && cq < ns;
        const float* wrow = params + net.w_off[3] + (long)(ok ? cq : 0) * HID;
#pragma unroll
        for (int jo = 0; jo < NB; ++jo) {
            const f32x4 v = rr_row_load<S>(wrow, jo, q);
#pragma unroll
            for (int r = 0; r < ((jo < NB - 1) ? 4 : R); ++r) wo[4 * jo + r] = ok ? v[r] : 0.f;
        }
    }
    // (every load of the prologue is unconditional — clamped index, select afterwards — so that they are all in flight
    // together: as guarded loads each was a branch and an L2 round trip of its own, 8k cycles before the first stage)
    float o_bias[4], o_mu[4], o_sig[4];
    const float* const nrm_v = nrm ? nrm : params;        // (a readable address either way)
    const int nrm_n = nrm ? 2 * idim + 2 * ns : 1;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int c = 4 * r + q, cc = min(c, ns - 1);
        const bool ok = r < KS0 && c < ns;
        const float vb = params[net.b_off[3] + cc];
        const float vm = nrm_v[min(2 * idim + cc, nrm_n - 1)], vs = nrm_v[min(2 * idim + ns + cc, nrm_n - 1)];
        o_bias[r] = ok ? vb : 0.f;
        o_mu[r] = (ok && nrm) ? vm : 0.f;
        o_sig[r] = (ok && nrm) ? vs : 1.f;
    }
    // this lane's input columns 4 k0 + q: where they come from, their normalisation
    float i_mu[4], i_isig[4];
#pragma unroll
    for (int k0 = 0; k0 < 4; ++k0) {
        const int col = 4 * k0 + q, cc = min(col, idim - 1);
        const float vm = nrm_v[min(cc, nrm_n - 1)], vs = nrm_v[min(idim + cc, nrm_n - 1)];
        i_mu[k0] = (nrm && col < idim) ? vm : 0.f;
        i_isig[k0] = (nrm && col < idim) ? vs : 1.f;
    }
    // ---- this wave's rows of the tile constants
    for (int idx = lane; idx < 16 * CK_NS; idx += 64) {
        const int mm = 16 * half + idx / CK_NS, c = idx % CK_NS, row = row0 + mm;
        const float v = gy0[(long)min(row, n - 1) * ns + min(c, ns - 1)];
        sY0[mm * CK_LD + c] = (row < n && c < ns) ? v : 0.f;
    }
    {
        const int mm = 16 * half + (lane >> 2), c = lane & 3, row = row0 + mm;
        const float v = L.c[(long)min(row, n - 1) * nc + min(c, max(nc - 1, 0))];
        sC[mm * CK_NC + c] = (row < n && c < nc) ? v : 0.f;
    }
    if (lane < 16) {
        const int p = min(row0 + 16 * half + lane, n - 1) / L.rpp;
        sH[16 * half + lane] = L.h_dev ? (float)L.h_dev[(long)p * L.h_stride] : L.h_val[p];
    }
    if (!TRAJ && L.stage_begin > 0) {      // stages of an earlier launch: all loads first, then the LDS (and FSAL) stores
        constexpr int NIT = CK_MAX_STAGES * 16 * CK_NS / 64;
        float vals[NIT];
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int idx = lane + 64 * it;
            const int j = idx / (16 * CK_NS), rem = idx - j * 16 * CK_NS;           // (j is uniform per iteration)
            const int mm = 16 * half + rem / CK_NS, c = rem % CK_NS, row = row0 + mm;
            const long rc = (long)min(row, n - 1) * ns + min(c, ns - 1);
            float v = 0.f;
            if (j < L.stage_begin) {
                if (fsal && j == 0) v = (gK - L.slot_floats)[(long)(L.S_total - 1) * n * ns + rc];   // first stage = the previous slot's last
                else v = gK[(long)j * n * ns + rc];
            }
            vals[it] = (row < n && c < ns) ? v : 0.f;
        }
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int idx = lane + 64 * it;
            const int j = idx / (16 * CK_NS), rem = idx - j * 16 * CK_NS;
            const int mm = 16 * half + rem / CK_NS, c = rem % CK_NS, row = row0 + mm;
            if (j < L.stage_begin) {
                sK[(j * TILE + mm) * CK_LD + c] = vals[it];
                if (fsal && j == 0 && row < n && c < ns) gK[(long)row * ns + c] = vals[it];   // kept in this slot for the interpolant
            }
        }
    }
    // narrow nets keep both hid x hid layers' biases in registers for the whole launch: a bias load inside the stage loop
    // queues behind the previous stage's stores (vmcnt is in order) and the layer's first MFMAs need it as their C operand
    constexpr bool BRES = NB <= 4;
    f32x4 bres[BRES ? 2 : 1][NB];
    if (BRES) {
#pragma unroll
        for (int l = 0; l < 2; ++l)
#pragma unroll
            for (int jo = 0; jo < NB; ++jo) bres[BRES ? l : 0][jo] = rr_bias<S>(params + net.b_off[1 + l], jo, q);
    }
    __syncthreads();           // (sW0 is shared by the two waves; everything else above is the wave's own rows)
    CSTAMP(1)

    // (a stage's tableau row is a scalar load from the kernel arguments: requested one stage ahead, its latency — a
    // scalar-cache miss per stage — is off the stage's critical path)
    float bnext[CK_MAX_STAGES];
#pragma unroll
    for (int j = 0; j < CK_MAX_STAGES; ++j) bnext[j] = L.beta[L.stage_begin][j];
    for (int k = 0; k < H; ++k) {
    // (TRAJ) the next interval's carried columns are requested HERE, ahead of the interval's weight-fragment loads and
    // behind the previous interval's store burst — not between two fragment loads of a layer (vmcnt is in order); they
    // reach sC behind the interval's last stage
    float cnext = 0.f;
    const int kc = HOLD ? k / hm : k;                    // (HOLD) the control interval; `last`: behind its last fine step
    const bool last = !HOLD || k - kc * hm == hm - 1;
    if constexpr (TRAJ && !GRID) {
        const int mm = 16 * half + (lane >> 2), c = lane & 3, row = row0 + mm;
        cnext = L.c[(long)min(k + 1, H - 1) * n * nc + (long)min(row, n - 1) * nc + min(c, max(nc - 1, 0))];
    }
    if constexpr (HOLD) {
        if (last) {      // (uniform)
            const int mm = 16 * half + (lane >> 2), c = lane & 3, row = row0 + mm;
            cnext = L.c[(long)(min(k + 1, H - 1) / hm) * n * nc + (long)min(row, n - 1) * nc + min(c, max(nc - 1, 0))];
        }
    }
    if constexpr (GRID) { if (lane < 16) sH[16 * half + lane] = hs[HOLD ? k - kc * hm : k]; }      // (the wave's own rows: no barrier)
    const long kS = TRAJ ? (long)k * L.S_total : 0;      // interval k's first stage in the [k][stage][row] layout
    for (int st = L.stage_begin; st < stage_end; ++st) {
        const int sb = 2 + 8 * (st - L.stage_begin);
        (void)sb;
        CSTAMP(sb + 0)
        float bn[CK_MAX_STAGES];
#pragma unroll
        for (int j = 0; j < CK_MAX_STAGES; ++j) bn[j] = bnext[j];
        const long srow = (kS + st) * n + grow;
        // ---- stage input [Y_st | c | 1] in registers,  Y_st = y0 + h sum_j beta[st][j] K_j  (rk_combine_kernel's op order)
        // What a stage leaves in global memory — Y_st, K_st, the layers' mask words — is stored in ONE burst at its end:
        // vmcnt counts stores and loads in order, so a store issued between two weight-fragment loads makes the MFMAs
        // behind the second one wait for the store's trip to HBM (a 64-wide layer is 2k cycles of MFMAs: one such wait
        // per layer doubled it).  Behind the burst come the next stage's input and layer 0, which need no load.
        float yv[4], ykeep[4] = {0.f, 0.f, 0.f, 0.f};
        unsigned wsave0 = 0u, wsave1 = 0u, wsave2 = 0u;
        {
            // (no data-dependent branch: every lane requests its operands with clamped indices, all reads in flight
            // together, selects at the end — the per-column if / else ladder was four serialised LDS round trips)
            const float h = sH[m];
            float y0v[4], cv[4], kv[4][CK_MAX_STAGES - 1];
#pragma unroll
            for (int k0 = 0; k0 < 4; ++k0) {
                const int col = 4 * k0 + q, cs = min(col, ns - 1), cc = min(max(col - ns, 0), max(nc - 1, 0));
                y0v[k0] = sY0[m * CK_LD + cs];
                cv[k0] = sC[m * CK_NC + cc];
#pragma unroll
                for (int j = 0; j < CK_MAX_STAGES - 1; ++j) kv[k0][j] = sK[(j * TILE + m) * CK_LD + cs];
            }
#pragma unroll
            for (int k0 = 0; k0 < 4; ++k0) {
                const int col = 4 * k0 + q;
                float a = y0v[k0];
#pragma unroll
                for (int j = 0; j < CK_MAX_STAGES - 1; ++j) {
                    const float t = a + kv[k0][j] * (bn[j] * h);
                    a = (j < st && bn[j] != 0.f) ? t : a;
                }
                ykeep[k0] = a;
                a = (col < ns) ? a : ((col < idim) ? cv[k0] : 0.f);
                if (nrm) {
                    a = (col < idim) ? (a - i_mu[k0]) * i_isig[k0] : a;
                    if (!TRAJ && gXn && row_ok && col < idim) gXn[srow * idim + col] = a;
                }
                if constexpr (TRAJ && BITS == 0) ykeep[k0] = a;      // (the stage-input row, stored with the stage's burst)
                yv[k0] = (col == idim) ? 1.f : a;
            }
        }
        float Ha[KS], Hb[KS];
        f32x4 acc0[NB], acc[NB], bv[NB], bpre[3];
        auto prefetch_bias = [&](int l) __attribute__((always_inline)) {
            if (BRES) return;
#pragma unroll
            for (int jo = 0; jo < G0; ++jo) bpre[jo] = rr_bias<S>(params + net.b_off[l], jo, q);
        };
        prefetch_bias(1);
        unsigned wd = 0u;                 // (mask mode) the layer's mask word, values shifted in in ascending register order
        auto save_block = [&](int l, int jo, const float (&H)[KS]) __attribute__((always_inline)) {
            if (BITS || !acts || !row_ok) return;
            f32x4 hv{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int rr = 0; rr < ((jo < NB - 1) ? 4 : R); ++rr) hv[rr] = H[4 * jo + rr];
            rr_row_store<S>(acts + (long)l * acts_ls + srow * HID, jo, q, hv);
        };
        auto save_word = [&](int l) __attribute__((always_inline)) {       // (kept; stored with the stage's burst)
            if (l == 0) wsave0 = wd; else if (l == 1) wsave1 = wd; else wsave2 = wd;
        };
        auto pre_l0 = [&](int ks) __attribute__((always_inline)) {
            const int jo = (ks < 4 * (NB - 1)) ? (ks >> 2) : NB - 1, r = ks - 4 * jo;
            const float h = rr_relu(acc0[jo][r]);
            Ha[ks] = h;
            if (BITS) rr_mask_push(wd, h);
            if (r == ((jo < NB - 1) ? 3 : R - 1)) save_block(0, jo, Ha);
            if (ks == KS - 1) save_word(0);
        };
        auto pre_tail = [&](int lp, float (&H)[KS], int t) __attribute__((always_inline)) {
            if (t >= NT) return;
            const int jo = TB + (t >> 2), r = t & 3;
            const float h = rr_relu(acc[jo][r]);
            H[4 * TB + t] = h;
            if (BITS) rr_mask_push(wd, h);
            if (t == 3 || t == NT - 1) save_block(lp, jo, H);
            if (t == NT - 1) save_word(lp);
        };
        CSTAMP(sb + 1)
        // ---- layer 0 (bias folded into the product): always four k-steps — fragments and inputs past the width are zero —
        //      with the k-step outside, so that the MFMAs of one block are NB issue slots apart and nothing branches
        {
            float a0[4][NB];
#pragma unroll
            for (int k0 = 0; k0 < 4; ++k0)
#pragma unroll
                for (int jo = 0; jo < NB; ++jo) a0[k0][jo] = sW0[(k0 * 8 + jo) * 64 + lane];
#pragma unroll
            for (int jo = 0; jo < NB; ++jo)
                acc0[jo] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[0][jo], yv[0], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
            for (int k0 = 1; k0 < 4; ++k0)
#pragma unroll
                for (int jo = 0; jo < NB; ++jo)
                    acc0[jo] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[k0][jo], yv[k0], acc0[jo], 0, 0, 0);
        }
        // ---- the two hid x hid layers, then the output layer (statically unrolled, as node_rr_kernels.hip)
        auto wide = [&](auto lc, float (&Hin)[KS], float (&Hout)[KS]) __attribute__((always_inline)) {
            constexpr int l = decltype(lc)::value;
#pragma unroll
            for (int jo = 0; jo < NB; ++jo)
                bv[jo] = BRES ? bres[BRES ? l - 1 : 0][jo] : ((jo < G0) ? bpre[jo] : rr_bias<S>(params + net.b_off[l], jo, q));
            __builtin_amdgcn_sched_barrier(0);
            if (l == 1) {
                // the next stage's tableau row: a scalar load, requested HERE — behind the stage's last LDS wait (scalar
                // and LDS loads share lgkmcnt and scalar loads return out of order, so a wait for LDS data is a wait
                // for every scalar load in flight) and ahead of two layers of MFMAs that need neither
                int sn = TRAJ ? ((st + 1 < L.S_total) ? st + 1 : 0) : min(st + 1, L.S_total - 1);
                asm volatile("" : "+s"(sn));
#pragma unroll
                for (int j = 0; j < CK_MAX_STAGES; ++j) bnext[j] = L.beta[sn][j];
                __builtin_amdgcn_sched_barrier(0);
            }
            const int cur = wbase + (l - 1) * S::LAYER_BYTES;
            const int nxt = (l == 1) ? cur + S::LAYER_BYTES : wbase;
            gemm.run(acc, bv, Hin, rs, voff, cur, nxt,
                     [&](int ks) __attribute__((always_inline)) {
                         if (l == 1) pre_l0(ks);
                         else pre_tail(l - 1, Hin, ks);
                     },
                     [&](int jo, int r) __attribute__((always_inline)) {
                         const float h = rr_relu(acc[jo][r]);
                         Hout[4 * jo + r] = h;
                         if (BITS) rr_mask_push(wd, h);
                         if (r == 3) save_block(l, jo, Hout);
                     },
                     [&]() __attribute__((always_inline)) { if (l == 1) prefetch_bias(2); });
        };
        CSTAMP(sb + 2)
        wide(std::integral_constant<int, 1>{}, Ha, Hb);
        CSTAMP(sb + 3)
        wide(std::integral_constant<int, 2>{}, Hb, Ha);
        CSTAMP(sb + 4)
        {
            const f32x4 o = RRGemm<S>::block(wo, Ha, [&](int ks) __attribute__((always_inline)) { pre_tail(2, Ha, ks); });
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int c = 4 * r + q;
                if (r < KS0 && c < ns) {
                    const float val = (o[r] + o_bias[r]) * o_sig[r] + o_mu[r];
                    sK[(st * TILE + m) * CK_LD + c] = val;
                    if (!TRAJ && row_ok) gK[srow * ns + c] = val;
                }
            }
#pragma unroll
            for (int k0 = 0; k0 < 4; ++k0) {
                if constexpr (TRAJ) {       // (rows go with rows: mask words alone keep no stage inputs)
                    if (BITS == 0 && gXn && row_ok && 4 * k0 + q < idim) gXn[srow * idim + 4 * k0 + q] = ykeep[k0];
                } else {
                    if (row_ok && 4 * k0 + q < ns) gY[srow * ns + 4 * k0 + q] = ykeep[k0];
                }
            }
            if (BITS && acts && row_ok) {
                unsigned* wp = reinterpret_cast<unsigned*>(acts) + srow * 4 + q;
                wp[0] = wsave0; wp[acts_ls] = wsave1; wp[2 * acts_ls] = wsave2;
            }
        }
        CSTAMP(sb + 5)
    }
    if constexpr (TRAJ) {      // ---- the interval's result, this wave's 16 rows: out[k+1], and the next interval's y0 / c
        for (int idx = lane; idx < 16 * ns; idx += 64) {
            const int mm = 16 * half + idx / ns, r = idx % ns, row = row0 + mm;
            if (row >= n) continue;
            const float a = crr_step_output<TILE>(L, sY0, sK, mm, r, sH[mm]);
            if constexpr (SUB) {
                const float y_old = sY0[mm * CK_LD + r];
                const int j1 = sub->ofs[k + 1];
                for (int j = sub->ofs[k]; j < j1; ++j)
                    L.out[(long)(j - 1) * n * ns + (long)row * ns + r] = nlbac_sub_point(y_old, a, sub->theta[j - 1]);
            } else {
                if (last) L.out[(long)kc * n * ns + (long)row * ns + r] = a;
            }
            sY0[mm * CK_LD + r] = a;
        }
        if constexpr (!GRID) {
            const int mm = 16 * half + (lane >> 2), c = lane & 3;
            sC[mm * CK_NC + c] = (row0 + mm < n && c < nc) ? cnext : 0.f;
        }
        if constexpr (HOLD) {
            if (last) {
                const int mm = 16 * half + (lane >> 2), c = lane & 3;
                sC[mm * CK_NC + c] = (row0 + mm < n && c < nc) ? cnext : 0.f;
            }
        }
    }
    }
    if constexpr (TRAJ) return;
    __syncthreads();
    CSTAMP(2 + 8 * (stage_end - L.stage_begin))
#ifdef RR_TIMING
    if (L.err) return;
#endif

    // ---- step outputs
    for (int idx = tid; idx < TILE * ns; idx += NTHR) {
        const int mm = idx / ns, r = idx - mm * ns, row = row0 + mm;
        if (row >= n) continue;
        const float h = sH[mm];
        if (L.out) L.out[(long)row * ns + r] = crr_step_output<TILE>(L, sY0, sK, mm, r, h);
        if (gErr) {
            float a = 0.f;
            for (int j = 0; j < L.n_err; ++j)
                if (L.c_err[j] != 0.f) a = a + sK[(j * TILE + mm) * CK_LD + r] * (L.c_err[j] * h);
            gErr[(long)row * ns + r] = a;
        }
    }
    if (ip && tid < n_rows) {      // the interpolant at t_end, should this attempt be accepted: one thread per row
        const int mm = tid, row = row0 + mm, sl = L.S_total - 1;
        const float h = sH[mm];
        for (int r = 0; r < ns; ++r) {
            const float a0 = sY0[mm * CK_LD + r];
            float a1 = a0, k[7];
            for (int j = 0; j < sl; ++j)
                if (L.beta[sl][j] != 0.f) a1 = a1 + sK[(j * TILE + mm) * CK_LD + r] * (L.beta[sl][j] * h);
#pragma unroll
            for (int j = 0; j < 7; ++j) k[j] = sK[(j * TILE + mm) * CK_LD + r];
            L.ip_out[(long)row * ns + r] = dopri_interp_value(a0, a1, k, h, ip_x);
        }
    }
    // ---- fused step control (as concat_rk_fwd_kernel): tile partial sums, one ticket per problem, last workgroup = controller
    if (L.norm_mode < 0) return;
    __shared__ unsigned s_last;
    if (tid < 64) {
        const int mm = tid;
        float v0 = 0.f, v1 = 0.f;
        if (mm < n_rows) {
            const float h = sH[mm];
            for (int r = 0; r < ns; ++r) {
                const float y = sY0[mm * CK_LD + r];
                if (L.norm_mode == 2) {
                    float e = 0.f, y1 = y;
                    for (int j = 0; j < L.n_err; ++j)
                        if (L.c_err[j] != 0.f) e = e + sK[(j * TILE + mm) * CK_LD + r] * (L.c_err[j] * h);
                    const int sl = L.S_total - 1;
                    for (int j = 0; j < sl; ++j)
                        if (L.beta[sl][j] != 0.f) y1 = y1 + sK[(j * TILE + mm) * CK_LD + r] * (L.beta[sl][j] * h);
                    const float qq = e / (L.atol + L.rtol * fmaxf(fabsf(y), fabsf(y1)));
                    v0 += qq * qq;
                } else {
                    const float sc = L.atol + fabsf(y) * L.rtol;
                    if (L.norm_mode == 0) {
                        const float q0 = y / sc, q1 = sK[mm * CK_LD + r] / sc;
                        v0 += q0 * q0; v1 += q1 * q1;
                    } else {
                        const float qq = (sK[(TILE + mm) * CK_LD + r] - sK[mm * CK_LD + r]) / sc;
                        v0 += qq * qq;
                    }
                }
            }
            if (L.norm_mode == 0)
                for (int c = 0; c < nc; ++c) {
                    const float y = sC[mm * CK_NC + c];
                    const float qq = y / (L.atol + fabsf(y) * L.rtol);
                    v0 += qq * qq;
                }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { v0 += __shfl_down(v0, off, 64); v1 += __shfl_down(v1, off, 64); }
        if (tid == 0) {
            const int nblk = (L.rpp + TILE - 1) / TILE;
            const int blk = (row0 - p_tile * L.rpp) / TILE;
            float* pq = L.partials + ((long)p_tile * nblk + blk) * 2;
            const float o0 = __hip_atomic_exchange(pq + 0, v0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const float o1 = __hip_atomic_exchange(pq + 1, v1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("" ::"v"(o0), "v"(o1) : "memory");
            const unsigned ticket = __hip_atomic_fetch_add(L.tickets + p_tile, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            s_last = (ticket == (unsigned)nblk - 1u) ? 1u : 0u;
            if (s_last) __hip_atomic_store(L.tickets + p_tile, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    __syncthreads();
    if (!s_last || tid >= 64) return;
    {
        const int nblk = (L.rpp + TILE - 1) / TILE;
        double d0 = 0.0, d1 = 0.0;
        for (int b = tid; b < nblk; b += 64) {
            const float* pq = L.partials + ((long)p_tile * nblk + b) * 2;
            d0 += (double)__hip_atomic_load(pq + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            d1 += (double)__hip_atomic_load(pq + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { d0 += __shfl_down(d0, off, 64); d1 += __shfl_down(d1, off, 64); }
        if (tid == 0) {
            const double cnt = (double)L.rpp * (double)(ns + nc);
            double* c = L.ctl_w + (long)p_tile * NLBAC_DOPRI_CTL;
            const int slot_before = (int)c[C_NACC];
            const double h_try = c[C_H];
            dopri_control_vals(sqrt(d0 / cnt), sqrt(d1 / cnt), p_tile, L.norm_mode, L.t_end, L.ctl_w, L.n_slots);
            if (L.norm_mode == 2 && L.hslots && c[C_ACCEPT] > 0.0) L.hslots[(long)p_tile * L.n_slots + slot_before] = h_try;
            if (L.norm_mode == 2 && L.alog) {
                const int k = (int)c[C_NSTEPS] - 1;
                if (k >= 0 && k < L.alog_cap) {
                    double* a = L.alog + ((long)p_tile * L.alog_cap + k) * 3;
                    a[0] = h_try; a[1] = c[C_RATIO]; a[2] = c[C_ACCEPT];
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Backward of the same step, same wave roles: per stage (descending) the output layer's gradient enters one transposed
// block product, dz runs down the chain in registers (backward RR pack), dX = W_0^T dz_0 is one more block product whose
// state columns feed the stage algebra and whose carried columns accumulate dc — all on the wave's own 16 rows.
// ---------------------------------------------------------------------------------------------------------------------
// What the rollout's backward adds to the one-step descriptor.
struct ConcatRkTrajBwd {
    int H;
    const float* dout;                // [H+1][n][n_s] dL/d(rollout output)
    float* dx0;                       // [n][n_s]
    float c_out[CK_MAX_STAGES]; int n_out;
};

// TRAJ: the backward of a whole fixed-grid rollout, intervals k = H-1 .. 0 in one launch.  Interval k's step is the
// one-step launch's with dL/dout_k = X.dout[k+1] + the dy0 of interval k+1 (carried in sDY0: the fp32 add the chained
// path does between two launches), dy0 = 0 + d and dK_j = 0 + (c_out[j] h) d formed from it as nlbac_rk_stage_bwd forms
// them from the step's output combination; mask words / rows / dz at stage index k S + st of H S stages; the carried
// columns' gradient of interval k to L.dc + k n n_c.  With weight gradients wanted (L.dz) every stage's gradient w.r.t.
// the net's own output (dK, times out_sig for a normalised net) goes to L.dyn as rows [k S + st][row][n_s].
// X.dx0 = X.dout[0] + the dy0 of interval 0.  All of it on the wave's own 16 rows: no barrier in the interval loop.
// The device-driven chain and the interpolant's backward are compiled out.  TRAJ = false (X null): the one-step kernel.
// GRID (with TRAJ; nlbac_concat_rk_grid_bwd): step size hs[k] per interval, and L.dc [n][n_c] is the sum of the
// intervals' gradients w.r.t. the (one set of) carried columns, formed by the wave that owns the rows in the order
// k = H-1 .. 0 — total = dc_{H-1}; total = total + dc_k, the fp32 adds the chained path does between its launches —
// in sDYup, which only the interpolant's backward uses otherwise.
// SUB (with GRID; nlbac_concat_rk_subgrid_bwd): X->dout [T][n][n_s] belongs to the output points: interval k's d is
// sum_j theta_j dout[j] over its outputs (j ascending; + the dy0 of interval k+1), and sum_j (1 - theta_j) dout[j] joins
// the interval's dy0 before it is handed to interval k-1 resp. enters dx0 — by the lane that holds the entry.  With every
// weight 1: the GRID kernel's fp32 operations on the fine grid with zero dout at the unused points.
// HOLD (with GRID, not SUB; nlbac_concat_rk_hold_bwd): X->H = N fine intervals, hm per control interval, i = k hm + r;
// X->dout [N/hm + 1][n][n_s] and L.dc [N/hm][n][n_c] belong to the control intervals: d takes dout[k+1] at r = hm-1 and 0
// elsewhere (SUB's fine interval without an output), dc is summed inside a control interval in GRID's order
// (total = dc_{hm-1}; total = total + dc_r, afresh in every control interval) and written at r = 0.
template <int NB, int R, int BITS, int NW, bool TRAJ = false, bool GRID = false, bool SUB = false, bool HOLD = false>
__device__ __forceinline__ void concat_rr_bwd_body(const ConcatRkBwdLaunch& L, const ConcatRkTrajBwd* X = nullptr,
                                                   const float* hs = nullptr, const NlbacSubGrid* sub = nullptr,
                                                   const int hm = 1) {
    static_assert(TRAJ || !GRID, "a time grid is a trajectory");
    static_assert(GRID || !SUB, "sub-steps are a time grid's");
    static_assert((GRID && !SUB) || !HOLD, "a held control's fine steps are a time grid's, its outputs their end points");
    constexpr int TILE = 16 * NW;
    using S = RRShape<NB, R>;
    constexpr int KS = S::KS, HID = S::HID, TB = NB - 2, NT = KS - 4 * TB;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int half = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = L.n, ns = L.n_s, nc = L.n_c;
    const int row0 = blockIdx.x * TILE;
    long soff = 0;
    int slot = 0;
    const bool chained = !TRAJ && L.ctl != nullptr;
    if (chained) {
        slot = (int)L.ctl[(long)(row0 / L.rpp) * NLBAC_DOPRI_CTL + C_NACC] - L.back_idx;
        if (slot < 0) return;                       // (uniform) this problem took fewer steps
        soff = (long)slot * L.slot_floats;
    }
    const bool carry = chained && L.back_idx > 0;
    const bool ip = L.ip_on && chained && !carry;      // dK / dy0 / dy1 of the last step from d loss / d y(t_end): no interp launch
    float* const gdK = TRAJ ? nullptr : L.dK + soff;
    float* const gdy0 = L.dy0 ? L.dy0 + soff : nullptr;
    float* const gdyn = L.dyn ? L.dyn + soff : nullptr;
    const float* const gdYup = TRAJ ? nullptr : (carry ? gdy0 + L.slot_floats : (L.dYup ? L.dYup + soff : nullptr));
    const int H = TRAJ ? X->H : 1;
    const nlbac_mlp& net = L.net;
    const int idim = net.in_dim;
    const bool keep_dz = L.dz != nullptr;
    const int q = lane >> 4, r16 = lane & 15, m = 16 * half + r16, grow = row0 + m;
    const bool row_ok = grow < n;
    const int growc = min(grow, n - 1);
    const int KS0 = (ns + 3) >> 2;
    const float* const params = net.params;
    const float* const acts = L.acts + soff;
    float* const dz = keep_dz ? L.dz + soff : nullptr;
    const long acts_ls = L.acts_ls;
    const float* const nrm = L.norm;
    const int dx_stage0 = L.dx_stage0;

    float* sDK = smem;                                              // [stage][32][CK_NS]
    float* sH = sDK + CK_MAX_STAGES * TILE * CK_LD;       // [32]
    float* sDY0 = sH + TILE;                              // [32][CK_NS] running dy0
    float* sDC = sDY0 + TILE * CK_LD;                     // [32][CK_NC] running d carried
    float* sDX = sDC + TILE * CK_NC;                      // [32][16] dX of the current stage (input columns)
    float* sWt = sDX + TILE * 16;                         // [k-step < 4][block < 8][lane]: W_out^T's A fragments
    float* sDYup = sWt + 4 * 8 * 64;                                // [32][CK_NS] dL/dy1 when the launch forms it itself (ip)

    const int st_lo = chained ? (slot == 0 ? 0 : 1) : L.st_lo;
    const bool stage0_data = dx_stage0 || keep_dz;
#define crr_has_data(st_) ((st_) >= st_lo && ((st_) > 0 || stage0_data))

    const __amdgpu_buffer_rsrc_t rs = rr_rsrc(net.packed, net.packed_floats);
    const int voff = lane * 16, wbase = net.rr_bwd_off * 4;
    RRGemm<S> gemm;
    BSTAMP(0)
    gemm.prime(rs, voff, wbase + S::LAYER_BYTES);           // (layer 2's fragments first, then layer 1's)

    {       // (k-step e by wave e mod NW)
        const float* Wl = params + net.w_off[3];
#pragma unroll
        for (int ee = 0; ee < 4 / NW; ++ee) {
            const int e = half + NW * ee;
            const int c = 4 * e + q;
            const bool ok = e < KS0 && c < ns;
#pragma unroll
            for (int jo = 0; jo < NB; ++jo) {
                const int uo = rr_unit_out(NB, R, jo, r16);
                const float v = Wl[(long)min(c, ns - 1) * HID + max(uo, 0)];      // (unconditional: see the forward's prologue)
                sWt[(e * 8 + jo) * 64 + lane] = (ok && uo >= 0) ? v : 0.f;
            }
        }
    }
    float w0t[KS];        // A of dX: row i (< in_dim) of W_0^T
    {
        const float* W0 = params + net.w_off[0];
        const bool ok = r16 < idim;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const float v = W0[(long)rr_unit_in(NB, R, ks, q) * idim + min(r16, idim - 1)];
            w0t[ks] = ok ? v : 0.f;
        }
    }
    float o_sig[4], x_isig[4];
    const float* const nrm_v = nrm ? nrm : params;
    const int nrm_n = nrm ? 2 * idim + 2 * ns : 1;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int c = 4 * r + q;
        const float vs = nrm_v[min(2 * idim + ns + min(c, ns - 1), nrm_n - 1)];
        o_sig[r] = (nrm && r < KS0 && c < ns) ? vs : 1.f;
        const int i = 4 * q + r;                     // dX leaves lane (q, row) with input column 4 q + r in register r
        const float vi = nrm_v[min(idim + min(i, idim - 1), nrm_n - 1)];
        x_isig[r] = (nrm && i < idim) ? vi : 1.f;
    }
    // ---- this wave's rows of the tile constants
    {       // (uniform conditions branch; per-lane ones clamp the address and select: every load in flight at once)
        const int mm = 16 * half + (lane >> 2), c = lane & 3, row = row0 + mm;
        float v = 0.f;
        if (!TRAJ && L.dc && L.dc_acc) v = L.dc[(long)min(row, n - 1) * nc + min(c, max(nc - 1, 0))];
        sDC[mm * CK_NC + c] = (row < n && c < nc) ? v : 0.f;
    }
    if (ip) {       // (uniform) the interpolant's backward for this wave's rows (ode_kernels.hip::dopri_interp_bwd_kernel's arithmetic)
#pragma unroll
        for (int it = 0; it < (16 * CK_LD + 63) / 64; ++it) {
            const int idx = lane + 64 * it;
            const int mm = 16 * half + idx / CK_NS, c = idx % CK_NS, row = row0 + mm, rowc = min(row, n - 1), p = rowc / L.rpp;
            const float hh = (float)L.ctl[(long)p * NLBAC_DOPRI_CTL + C_HUSED], xx = (float)L.ctl[(long)p * NLBAC_DOPRI_CTL + C_X];
            const float g = L.ip_dout[(long)rowc * ns + min(c, ns - 1)];
            float d0v, d1v, dk[7];
            dopri_interp_grad(g, hh, xx, d0v, d1v, dk);
            const bool ok = row < n && c < ns;
            if (idx < 16 * CK_NS) {
                sDY0[mm * CK_LD + c] = ok ? d0v : 0.f;
                sDYup[mm * CK_LD + c] = ok ? d1v : 0.f;
#pragma unroll
                for (int j = 0; j < 7; ++j) sDK[(j * TILE + mm) * CK_LD + c] = ok ? dk[j] : 0.f;
            }
        }
    } else if constexpr (!TRAJ) {
        const bool have = gdy0 && L.dy0_in && !carry;
#pragma unroll
        for (int it = 0; it < (16 * CK_LD + 63) / 64; ++it) {
            const int idx = lane + 64 * it;
            const int mm = 16 * half + idx / CK_NS, c = idx % CK_NS, row = row0 + mm;
            float v = 0.f;
            if (have) v = gdy0[(long)min(row, n - 1) * ns + min(c, ns - 1)];
            if (idx < 16 * CK_NS) sDY0[mm * CK_LD + c] = (row < n && c < ns) ? v : 0.f;
        }
    }
    if (lane < 16) {
        const int p = min(row0 + 16 * half + lane, n - 1) / L.rpp;
        sH[16 * half + lane] = chained ? (float)L.hslots[(long)p * L.n_slots + slot]
                                       : (L.h_dev ? (float)L.h_dev[(long)p * L.h_stride] : L.h_val[p]);
    }
    if (!TRAJ && !ip) {   // dK of every stage into LDS: all loads first (a loop with a run-time bound and the LDS store behind each load
        // was one global round trip per iteration: 16 in a row for rk4, most of the launch's prologue)
        constexpr int NIT = CK_MAX_STAGES * 16 * CK_NS / 64;
        float vals[NIT];
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int idx = lane + 64 * it;
            const int j = idx / (16 * CK_NS), rem = idx - j * 16 * CK_NS;           // (j is uniform: 16 * CK_NS is a multiple of 64)
            const int mm = 16 * half + rem / CK_NS, c = rem % CK_NS, row = row0 + mm;
            const long rc = (long)min(row, n - 1) * ns + min(c, ns - 1);
            float v = 0.f;
            if (j < L.st_hi) {
                if (!carry) v = gdK[(long)j * n * ns + rc];
                else if (j == L.S_total - 1) v = (gdK + L.slot_floats)[rc];     // FSAL: next slot's dK[0]
            }
            vals[it] = (row < n && c < ns) ? v : 0.f;
        }
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int idx = lane + 64 * it;
            const int j = idx / (16 * CK_NS), rem = idx - j * 16 * CK_NS;
            const int mm = 16 * half + rem / CK_NS, c = rem % CK_NS;
            if (j < L.st_hi) sDK[(j * TILE + mm) * CK_LD + c] = vals[it];
        }
    }
    __syncthreads();           // (sWt is shared by the two waves)

    f32x4 zero[NB];
#pragma unroll
    for (int jo = 0; jo < NB; ++jo) zero[jo] = f32x4{0.f, 0.f, 0.f, 0.f};
    // (mask mode) a stage's three mask words are requested while the stage before it runs: a load from HBM issued at the
    // start of a product would hold back every fragment load behind it (vmcnt is in order) for longer than the product's
    // own MFMAs take
    unsigned mnext0 = 0u, mnext1 = 0u, mnext2 = 0u;
    auto request_masks = [&](int stn) __attribute__((always_inline)) {
        if (!BITS || stn < st_lo) return;       // (TRAJ: stn counts over all H S stages)
        const unsigned* wp = reinterpret_cast<const unsigned*>(acts) + ((long)stn * n + growc) * 4 + q;
        mnext0 = wp[0]; mnext1 = wp[acts_ls]; mnext2 = wp[2 * acts_ls];
    };
    request_masks((H - 1) * L.S_total + L.st_hi - 1);
    float bnext[CK_MAX_STAGES];
#pragma unroll
    for (int j = 0; j < CK_MAX_STAGES; ++j) bnext[j] = L.beta[max(L.st_hi - 1, 0)][j];
    // (TRAJ) an interval's dL/dout rows are loaded where they are needed, between two intervals: held in registers
    // through an interval they would cost the mask-word instances their third wave per SIMD
    constexpr int NITD = 16 * CK_NS / 64;
    float dnext[NITD];
    auto request_dout = [&](int kn) __attribute__((always_inline)) {
        if constexpr (TRAJ) {
#pragma unroll
            for (int it = 0; it < NITD; ++it) {
                const int idx = lane + 64 * it, mm = 16 * half + idx / CK_NS, c = idx % CK_NS;
                dnext[it] = X->dout[(long)kn * n * ns + (long)min(row0 + mm, n - 1) * ns + min(c, ns - 1)];
            }
        }
    };
    // (SUB) this lane's (row, column) offset into an output point's gradient rows, formed anew wherever it is needed: kept
    // in registers through an interval, four of them would cost what dnext would (see above)
    auto sub_rc = [&](int it) __attribute__((always_inline)) {
        int idx = lane + 64 * it;
        asm volatile("" : "+v"(idx));
        return (long)min(row0 + 16 * half + idx / CK_NS, n - 1) * ns + min(idx % CK_NS, ns - 1);
    };
    (void)sub_rc;
    for (int kk = 0; kk < H; ++kk) {
    const int k = H - 1 - kk, kS = TRAJ ? k * L.S_total : 0;      // interval k's first stage in the [k][stage][row] layout
    if constexpr (TRAJ) {       // d = dout[k+1] (+ interval k+1's dy0): dy0 = 0 + d, dK_j = 0 + (c_out[j] h) d; dc = 0
        const int kc = HOLD ? k / hm : k, kr = k - kc * hm;      // (HOLD) control interval and fine step inside it
        (void)kr;
        if constexpr (HOLD) {
            if (kr == hm - 1) request_dout(kc + 1);      // (uniform)
            else {
#pragma unroll
                for (int it = 0; it < NITD; ++it) dnext[it] = 0.f;
            }
        } else if constexpr (!SUB) request_dout(k + 1);
        if constexpr (GRID) { if (lane < 16) sH[16 * half + lane] = hs[HOLD ? kr : k]; }
#pragma unroll
        for (int it = 0; it < NITD; ++it) {
            const int idx = lane + 64 * it, mm = 16 * half + idx / CK_NS, c = idx % CK_NS;
            const bool ok = row0 + mm < n && c < ns;
            const float vh = sH[mm];
            float d = SUB ? 0.f : dnext[it];
            if constexpr (SUB) {      // the outputs' gradients come in here, entry by entry, by the lane that holds the entry
                const long rc = sub_rc(it);
                d = nlbac_sub_gather<true>(*sub, X->dout, (long)n * ns, rc, k, d);
                if (kk > 0) d = d + nlbac_sub_gather<false>(*sub, X->dout, (long)n * ns, rc, k + 1, sDY0[mm * CK_LD + c]);
            } else {
                if (kk > 0) d = d + sDY0[mm * CK_LD + c];
            }
            sDY0[mm * CK_LD + c] = ok ? 0.f + d : 0.f;
#pragma unroll 1
            for (int j = 0; j < L.S_total; ++j) {       // (a rolled loop: the tableau's weights stay out of the SGPRs)
                float v = 0.f;
                if (j < X->n_out && X->c_out[j] != 0.f) v = 0.f + (X->c_out[j] * vh) * d;
                sDK[(j * TILE + mm) * CK_LD + c] = ok ? v : 0.f;
            }
        }
        sDC[(16 * half + (lane >> 2)) * CK_NC + (lane & 3)] = 0.f;
    }
    for (int st = L.st_hi - 1; st >= st_lo; --st) {
        const unsigned mcur0 = mnext0, mcur1 = mnext1, mcur2 = mnext2;
        request_masks(kS + st - 1);
        float bn[CK_MAX_STAGES];
#pragma unroll
        for (int j = 0; j < CK_MAX_STAGES; ++j) bn[j] = bnext[j];
        {
            const int sn = (TRAJ && st == 0) ? L.st_hi - 1 : max(st - 1, 0);          // (requested one stage ahead: see the forward)
#pragma unroll
            for (int j = 0; j < CK_MAX_STAGES; ++j) bnext[j] = L.beta[sn][j];
        }
        if (!crr_has_data(st)) continue;      // (uniform; the dyn of such a stage is not wanted either)
        const int sbb = 2 + 8 * st;
        (void)sbb;
        BSTAMP(sbb + 0)
        const long srow = (long)(kS + st) * n + growc;
        // ---- the output layer's gradient: dK (times out_sig), also kept for the weight gradients of a normalised field
        float dy[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = 4 * e + q;
            const float raw = sDK[(st * TILE + m) * CK_LD + min(c, ns - 1)];
            const float v = (e < KS0 && c < ns) ? raw * o_sig[e] : 0.f;
            if (gdyn && (TRAJ || nrm) && row_ok && e < KS0 && c < ns) gdyn[((long)(kS + st) * n + grow) * ns + c] = v;
            dy[e] = v;
        }
        float Za[KS], Zb[KS];
        f32x4 acct[NB], acc[NB], av[NB], avt[2];
        unsigned mw = 0u, mwt = 0u;
        auto fetch_masks = [&](int l) __attribute__((always_inline)) {
            if (BITS) {
                mw = (l == 0) ? mcur0 : (l == 1 ? mcur1 : mcur2);
                mw = row_ok ? mw : 0u;
            } else {
                const float* arow = acts + (long)l * acts_ls + srow * HID;
#pragma unroll
                for (int jo = 0; jo < NB; ++jo) av[jo] = rr_row_load<S>(arow, jo, q);
            }
        };
        auto save_block = [&](int l, int jo, const float (&Z)[KS]) __attribute__((always_inline)) {
            if (BITS || !dz || !row_ok) return;
            f32x4 zv{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int rr = 0; rr < ((jo < NB - 1) ? 4 : R); ++rr) zv[rr] = Z[4 * jo + rr];
            rr_row_store<S>(dz + (long)l * acts_ls + ((long)(kS + st) * n + grow) * HID, jo, q, zv);
        };
        auto pre_tail = [&](int lp, float (&Z)[KS], int t) __attribute__((always_inline)) {
            if (t >= NT) return;
            const int jo = TB + (t >> 2), r = t & 3;
            if (BITS) Z[4 * TB + t] = rr_mask_gate<KS>(mwt, 4 * TB + t, acc[jo][r]);
            else Z[4 * TB + t] = (row_ok && avt[jo - TB][r] > 0.f) ? acc[jo][r] : 0.f;
            if (t == 3 || t == NT - 1) save_block(lp, jo, Z);
        };
        // ---- top product: dz_2 = mask_2 * (W_out^T dy), finished at once
        fetch_masks(2);
        {       // (always four k-steps: fragments and dy past the width are zero; k-step outside, nothing branches)
            float at[4][NB];
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int jo = 0; jo < NB; ++jo) at[e][jo] = sWt[(e * 8 + jo) * 64 + lane];
#pragma unroll
            for (int jo = 0; jo < NB; ++jo)
                acct[jo] = __builtin_amdgcn_mfma_f32_16x16x4f32(at[0][jo], dy[0], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
            for (int e = 1; e < 4; ++e)
#pragma unroll
                for (int jo = 0; jo < NB; ++jo)
                    acct[jo] = __builtin_amdgcn_mfma_f32_16x16x4f32(at[e][jo], dy[e], acct[jo], 0, 0, 0);
        }
#pragma unroll
        for (int jo = 0; jo < NB; ++jo) {
#pragma unroll
            for (int r = 0; r < ((jo < NB - 1) ? 4 : R); ++r) {
                if (BITS) Za[4 * jo + r] = rr_mask_gate<KS>(mw, 4 * jo + r, acct[jo][r]);
                else Za[4 * jo + r] = (row_ok && av[jo][r] > 0.f) ? acct[jo][r] : 0.f;
            }
            save_block(2, jo, Za);
        }
        // ---- dz_1 = mask_1 * (W_2^T dz_2), dz_0 = mask_0 * (W_1^T dz_1)
        auto prod = [&](auto pc, float (&Zin)[KS], float (&Zout)[KS]) __attribute__((always_inline)) {
            constexpr int p = decltype(pc)::value;
            constexpr int lo = 2 - p;                             // the layer whose dz this product yields
            avt[0] = av[TB]; avt[1] = av[TB + 1]; mwt = mw;
            fetch_masks(lo);
            __builtin_amdgcn_sched_barrier(0);
            const int cur = wbase + lo * S::LAYER_BYTES;              // fragments of layer lo + 1 sit at index lo
            const int nxt = (lo >= 1) ? cur - S::LAYER_BYTES : wbase + S::LAYER_BYTES;
            gemm.run(acc, zero, Zin, rs, voff, cur, nxt,
                     [&](int ks) __attribute__((always_inline)) { if (p > 1) pre_tail(lo + 1, Zin, ks); },
                     [&](int jo, int r) __attribute__((always_inline)) {
                         if (BITS) Zout[4 * jo + r] = rr_mask_gate<KS>(mw, 4 * jo + r, acc[jo][r]);
                         else Zout[4 * jo + r] = (row_ok && av[jo][r] > 0.f) ? acc[jo][r] : 0.f;
                         if (r == 3) save_block(lo, jo, Zout);
                     },
                     [&]() __attribute__((always_inline)) {});
        };
        BSTAMP(sbb + 1)
        prod(std::integral_constant<int, 1>{}, Za, Zb);
        BSTAMP(sbb + 2)
        prod(std::integral_constant<int, 2>{}, Zb, Za);
        BSTAMP(sbb + 3)
        avt[0] = av[TB]; avt[1] = av[TB + 1]; mwt = mw;
        const f32x4 o = RRGemm<S>::block(w0t, Za, [&](int ks) __attribute__((always_inline)) { pre_tail(0, Za, ks); });
        BSTAMP(sbb + 4)
        if (st == 0 && !dx_stage0) continue;       // only the dz of stage 0 were wanted (uniform)
        // ---- dX (times in_isig): lane (q, row) holds input columns 4q + r of ITS row in register r — state columns go
        //      into the stage algebra (dy0 += d, dK_j += beta[st][j] h d for the earlier stages j), carried columns into
        //      dc — each (row, column) by the lane that holds it: every LDS operand requested up front with a clamped
        //      address, updated values written back under the lane's own predicate (no loop over the tile, no branch
        //      between the reads)
        {
            const float h = sH[m];
            const bool up = (gdYup || ip) && st == L.S_total - 1;       // (uniform)
            float yv0[4], dcv[4], kvv[4][CK_MAX_STAGES - 1], gup[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = 4 * q + r, cs = min(i, ns - 1), cc = min(max(i - ns, 0), max(nc - 1, 0));
                yv0[r] = sDY0[m * CK_LD + cs];
                dcv[r] = sDC[m * CK_NC + cc];
#pragma unroll
                for (int j = 0; j < CK_MAX_STAGES - 1; ++j) kvv[r][j] = sDK[(j * TILE + m) * CK_LD + cs];
                gup[r] = up ? (ip ? sDYup[m * CK_LD + cs] : gdYup[(long)growc * ns + cs]) : 0.f;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = 4 * q + r;
                const float dxv = o[r] * x_isig[r];
                if (i < ns) {
                    float d = (up && row_ok) ? gup[r] : 0.f;
                    d += dxv;
                    sDY0[m * CK_LD + i] = yv0[r] + d;
#pragma unroll
                    for (int j = 0; j < CK_MAX_STAGES - 1; ++j) {
                        const float t = kvv[r][j] + (bn[j] * h) * d;
                        sDK[(j * TILE + m) * CK_LD + i] = (j < st && bn[j] != 0.f) ? t : kvv[r][j];
                    }
                } else if (i < ns + nc) {
                    sDC[m * CK_NC + (i - ns)] = dcv[r] + dxv;
                }
            }
        }
        BSTAMP(sbb + 5)
    }
    if constexpr (TRAJ) {      // ---- interval k's gradient w.r.t. its carried columns, this wave's rows
        for (int idx = lane; idx < 16 * nc; idx += 64) {
            const int mm = 16 * half + idx / nc, c = idx % nc, row = row0 + mm;
            if constexpr (HOLD) {       // (GRID's sum below, afresh in every control interval)
                const int kc = k / hm, kr = k - kc * hm;
                float a = sDC[mm * CK_NC + c];
                if (kr != hm - 1) a = sDYup[mm * CK_NC + c] + a;
                sDYup[mm * CK_NC + c] = a;
                if (kr == 0 && row < n) L.dc[(long)kc * n * nc + (long)row * nc + c] = a;
            } else if constexpr (GRID) {
                float a = sDC[mm * CK_NC + c];
                if (kk > 0) a = sDYup[mm * CK_NC + c] + a;
                sDYup[mm * CK_NC + c] = a;
                if (k == 0 && row < n) L.dc[(long)row * nc + c] = a;
            } else {
                if (row < n) L.dc[(long)k * n * nc + (long)row * nc + c] = sDC[mm * CK_NC + c];
            }
        }
    }
    }
    if constexpr (TRAJ) {      // ---- dx0 = dout[0] + the dy0 of interval 0
        request_dout(0);
#pragma unroll
        for (int it = 0; it < NITD; ++it) {
            const int idx = lane + 64 * it, mm = 16 * half + idx / CK_NS, c = idx % CK_NS, row = row0 + mm;
            if constexpr (SUB) {
                if (row < n && c < ns)
                    X->dx0[(long)row * ns + c] = dnext[it] + nlbac_sub_gather<false>(*sub, X->dout, (long)n * ns, sub_rc(it), 0, sDY0[mm * CK_LD + c]);
            } else {
                if (row < n && c < ns) X->dx0[(long)row * ns + c] = dnext[it] + sDY0[mm * CK_LD + c];
            }
        }
        return;
    }
    BSTAMP(1)
    // ---- this wave's rows of the results
    for (int idx = lane; idx < L.st_hi * 16 * ns; idx += 64) {
        const int j = idx / (16 * ns), rem = idx - j * 16 * ns;
        const int mm = 16 * half + rem / ns, c = rem % ns, row = row0 + mm;
        if (row < n) gdK[((long)j * n + row) * ns + c] = sDK[(j * TILE + mm) * CK_LD + c];
    }
    if (gdy0)
        for (int idx = lane; idx < 16 * ns; idx += 64) {
            const int mm = 16 * half + idx / ns, c = idx % ns, row = row0 + mm;
            if (row < n) gdy0[(long)row * ns + c] = sDY0[mm * CK_LD + c];
        }
    if (L.dc)
        for (int idx = lane; idx < 16 * nc; idx += 64) {
            const int mm = 16 * half + idx / nc, c = idx % nc, row = row0 + mm;
            if (row < n) L.dc[(long)row * nc + c] = sDC[mm * CK_NC + c];
        }
#undef crr_has_data
}

// ---- what the one-step launchers and the rollout's share: the instance per width, waves per workgroup, LDS sizes
static inline int crr_shape_index(int hid) { return hid == 64 ? 0 : (hid == 100 ? 1 : (hid == 128 ? 2 : -1)); }

// waves per workgroup: four (64-row tiles) unless a tile would then straddle two problems
static inline int crr_waves(int n, int rpp) { return (rpp >= n || rpp % 64 == 0) ? 4 : 2; }
static inline size_t crr_fwd_lds(int tile) {
    return (size_t)(CK_MAX_STAGES * tile * CK_LD + tile * (CK_LD + CK_NC + 1) + 4 * 8 * 64) * sizeof(float);
}
static inline size_t crr_bwd_lds(int tile) {
    return (size_t)(CK_MAX_STAGES * tile * CK_LD + tile * (1 + CK_LD + CK_NC + 16 + CK_LD) + 4 * 8 * 64) * sizeof(float);
}

// the instances of one kernel template KERN<NB, R, BITS, NW> for one NW, [shape][BITS]
template <typename Launch>
struct ConcatRrTable {
    void (*k[3][2])(const Launch);
};

#define CONCAT_RR_TABLE(KERN, NW)                                                                                       \
    {{{KERN<4, 4, 0, NW>, KERN<4, 4, 1, NW>}, {KERN<7, 1, 0, NW>, KERN<7, 1, 1, NW>}, {KERN<8, 4, 0, NW>, KERN<8, 4, 1, NW>}}}

// launch the instance of `t` (the table of nw waves per workgroup) for a net `hid` wide and this acts_bits over n rows;
// `lds` is crr_fwd_lds or crr_bwd_lds
template <typename Launch>
static void crr_start(const ConcatRrTable<Launch>& t, int nw, const Launch& A, int hid, int n, int acts_bits,
                      size_t (*lds)(int), hipStream_t s) {
    const int tile = 16 * nw;
    hipLaunchKernelGGL(t.k[crr_shape_index(hid)][acts_bits ? 1 : 0], dim3(nlbac_ceil_div(n, tile)), dim3(64 * nw),
                       lds(tile), s, A);
}
