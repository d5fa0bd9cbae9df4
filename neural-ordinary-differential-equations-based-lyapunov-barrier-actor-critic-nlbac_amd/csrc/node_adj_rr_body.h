// The register-resident adjoint step of the control-affine NODE as a body two kernels share: node_adj_rr_kernels.hip (one
// RK step of z = [y | a_x | a_u] per launch: nlbac_node_adj_step; the scheme is described there) and
// node_adj_traj_kernels.hip (TRAJ: the same stages in a loop over a run of fine intervals, last to first, z in LDS from
// the run's top to its end: nlbac_node_adj_traj; adj_traj_shared.h says what happens between the intervals).  Every TRAJ
// addition sits behind `if constexpr (TRAJ)`: the one-step instances are the code they were.
#pragma once
#include "node_adj_shared.h"
#include "adj_traj_shared.h"
#include "rr_device.h"
#include <type_traits>

bool nlbac_node_rr_eligible(const nlbac_mlp* f, const nlbac_mlp* g);      // (node_rr_kernels.hip)

#define ARR_MAX_W 4        /* layer 0 + up to three hid x hid layers */

// KEEP (the NODE fit's parameter quadrature): every evaluated stage's inputs, the output-layer gradient of g_net, the
// activations and the pre-activation gradients additionally go out as rows, for nlbac_mlp_bwd_weights.  TRAJ + KEEP: the
// rows of stage st of fine interval fi are rows (fi S + st) n .. of the run's batch, and the cotangent rows (dz, dG, dK)
// are stored times that stage's h c_sol[st], so that the plain row sum of the one weight-gradient launch is the quadrature.
struct NodeAdjTrajLaunch : NodeAdjLaunch {
    AdjTrajArgs T;
};

template <int NB, int R, int KEEP, int TRAJ = 0>
__global__ __launch_bounds__(256) void node_adj_rr_kernel(const std::conditional_t<TRAJ != 0, NodeAdjTrajLaunch, NodeAdjLaunch> L) {
    using S = RRShape<NB, R>;
    constexpr int KS = S::KS, HID = S::HID, TB = NB - 2, NT = KS - 4 * TB, G0 = rr_group_first(NB);
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = wave >> 1, half = wave & 1;
    const int n = L.n, ns = L.n_s, nu = L.n_u, W = L.W;
    const int WP = L.ld;          // LDS row stride of a row of z: W | 1 (odd: the lanes of a column walk distinct banks)
    const int row0 = blockIdx.x * NLBAC_MLP_TILE;
    const nlbac_mlp& net = L.net[grp];
    const int nw = net.n_layers - 1;
    const int q = lane >> 4, r16 = lane & 15;
    const int m = 16 * half + r16, grow = row0 + m;
    const bool row_ok = grow < n;
    const int KS0 = (ns + 3) >> 2, KL0 = (ns + 4) >> 2;
    const int KSO = (grp == 0) ? KS0 : KS0 * nu;          // k-steps of the output layer's transposed product (<= 4)

    // ---- LDS
    float* const sKZ = smem;                                              // [stage][32][WP]
    float* const sZ0 = sKZ + L.S_total * NLBAC_MLP_TILE * WP;    // [32][WP]
    float* const sZS = sZ0 + NLBAC_MLP_TILE * WP;                     // [32][WP] stage input
    float* const sU = sZS + NLBAC_MLP_TILE * WP;                      // [32][4]
    float* const sH = sU + NLBAC_MLP_TILE * ADJ_MAX_NU;                   // [32]
    float* const sLive = sH + NLBAC_MLP_TILE;                             // [32]
    float* const sF = sLive + NLBAC_MLP_TILE;                             // [32][8]
    float* const sG = sF + NLBAC_MLP_TILE * ADJ_MAX_NS;                   // [32][32]
    float* const sDX = sG + NLBAC_MLP_TILE * ADJ_MAX_GOUT;                // [2][32][8]
    float* const sW0 = sDX + 2 * NLBAC_MLP_TILE * ADJ_MAX_NS;             // [net][k-step < 3][block < 8][lane] layer 0's A fragments
    float* const sWt = sW0 + 2 * 3 * 8 * 64;                              // [net][k-step < 4][block < 8][lane] W_out^T's A fragments
    // (TRAJ) what the intervals need between the stages lives in LDS, not in registers held over the stage body: c_sol
    //  [stage < 8], the run's arguments, the output interval being solved and whether the summed du still has to start
    float* const sCo = sWt + 2 * 4 * 8 * 64;
    AdjTrajArgs* const sT = reinterpret_cast<AdjTrajArgs*>(sCo + ADJ_MAX_STAGES);
    int* const sI = reinterpret_cast<int*>(sT + 1);                       // [0] kcur, [1] du_first
    (void)sCo; (void)sI;
    __shared__ int s_any;
    if (tid == 0) s_any = 0;

    const float* const params = net.params;
    int boff[ARR_MAX_W];
#pragma unroll
    for (int l = 0; l < ARR_MAX_W; ++l) boff[l] = net.b_off[l];

    // ---- the wave's weight stream: forward fragments of layers 1 .. nw-1, then the backward fragments nw-1 .. 1, round and
    //      round over the stages
    const __amdgpu_buffer_rsrc_t rs = rr_rsrc(net.packed, net.packed_floats);
    const int voff = lane * 16;
    const int fbase = net.rr_fwd_off * 4, bbase = net.rr_bwd_off * 4;
    RRGemm<S> gemm;
    gemm.prime(rs, voff, fbase);

    // ---- constants of the launch: layer 0's and W_out^T's A fragments to LDS, the output layer's and W_0^T's into registers
    if (half == 0) {
        const float* W0 = params + net.w_off[0];
        const float* b0 = params + boff[0];
        const float* Wl = params + net.w_off[nw];
#pragma unroll
        for (int k0 = 0; k0 < 3; ++k0)
#pragma unroll
            for (int jo = 0; jo < NB; ++jo) {
                const int uo = rr_unit_out(NB, R, jo, r16), col = 4 * k0 + q, uc = max(uo, 0);
                const float vw = W0[uc * ns + min(col, ns - 1)], vb = b0[uc];
                sW0[((grp * 3 + k0) * 8 + jo) * 64 + lane] = (uo < 0 || col > ns) ? 0.f : (col < ns ? vw : vb);
            }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            int o = -1;
            if (grp == 0) { const int c = 4 * e + q; if (e < KS0 && c < ns) o = c; }
            else { const int k0 = e / nu, u = e - k0 * nu, c = 4 * k0 + q; if (e < KS0 * nu && c < ns) o = c * nu + u; }
#pragma unroll
            for (int jo = 0; jo < NB; ++jo) {
                const int uo = rr_unit_out(NB, R, jo, r16);
                const float vw = Wl[(long)max(o, 0) * HID + max(uo, 0)];
                sWt[((grp * 4 + e) * 8 + jo) * 64 + lane] = (o >= 0 && uo >= 0) ? vw : 0.f;
            }
        }
    }
    float wo[KS], w0t[KS];
    {
        // forward: which output the A row r16 of the output block computes (node_rr_kernels.hip::rr_out_row)
        int orow;
        {
            const int qp = r16 >> 2, rp = r16 & 3;
            if (grp == 0) { const int c = 4 * rp + qp; orow = (rp < KS0 && c < ns) ? c : -1; }
            else { const int k0 = rp / nu, u = rp - k0 * nu, c = 4 * k0 + qp; orow = (rp < KS0 * nu && c < ns) ? c * nu + u : -1; }
        }
        const float* wrow = params + net.w_off[nw] + (long)max(orow, 0) * HID;
#pragma unroll
        for (int jo = 0; jo < NB; ++jo) {
            const f32x4 v = rr_row_load<S>(wrow, jo, q);
#pragma unroll
            for (int r = 0; r < ((jo < NB - 1) ? 4 : R); ++r) wo[4 * jo + r] = (orow >= 0) ? v[r] : 0.f;
        }
        const float* W0 = params + net.w_off[0];
        const int c = 4 * (r16 & 3) + (r16 >> 2);          // A row 4 q' + r' computes dX component 4 r' + q'
        const bool ok = (r16 & 3) < KS0 && c < ns;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const float vw = W0[(long)rr_unit_in(NB, R, ks, q) * ns + min(c, ns - 1)];
            w0t[ks] = ok ? vw : 0.f;
        }
    }
    int o_idx[4]; float o_bias[4];
    {
        const float* bo = params + net.b_off[nw];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            int o = -1;
            if (grp == 0) { const int c = 4 * r + q; if (r < KS0 && c < ns) o = c; }
            else { const int k0 = r / nu, u = r - k0 * nu, c = 4 * k0 + q; if (r < KS0 * nu && c < ns) o = c * nu + u; }
            o_idx[r] = o;
            const float vb = bo[max(o, 0)];
            o_bias[r] = (o >= 0) ? vb : 0.f;
        }
    }

    // ---- the tile's rows of the step: z0, u, h, liveness, the stage derivatives an earlier launch left
    if constexpr (TRAJ) {
        // the run's top: what the run above left (nothing at the horizon's end); every row of the batch is live, the
        // controls and the step come with the intervals
        for (int idx = tid; idx < NLBAC_MLP_TILE * WP; idx += 256) {
            const int mm = idx / WP, c = idx - mm * WP, row = row0 + mm;
            sZ0[idx] = (!L.T.top && row < n && c < W) ? L.T.carry[(long)row * W + c] : 0.f;
        }
        if (tid < NLBAC_MLP_TILE * ADJ_MAX_NU) sU[tid] = 0.f;
        if (tid == 0) {
#pragma unroll
            for (int j = 0; j < ADJ_MAX_STAGES; ++j) sCo[j] = L.c_out[j];
            *sT = L.T;
            sI[0] = 0; sI[1] = L.T.top;
        }
        if (tid < NLBAC_MLP_TILE) { sH[tid] = 0.f; sLive[tid] = (row0 + tid < n) ? 1.f : 0.f; }
        __syncthreads();
    } else {
    for (int idx = tid; idx < NLBAC_MLP_TILE * WP; idx += 256) {
        const int mm = idx / WP, c = idx - mm * WP, row = row0 + mm;
        sZ0[idx] = (row < n && c < W) ? L.Z0[(long)row * W + c] : 0.f;
    }
    if (tid < NLBAC_MLP_TILE * ADJ_MAX_NU) {
        const int mm = tid >> 2, c = tid & 3, row = row0 + mm;
        sU[tid] = (row < n && c < nu) ? L.u[(long)row * nu + c] : 0.f;
    }
    __syncthreads();            // (s_any = 0 is there)
    if (tid < NLBAC_MLP_TILE) {
        const int row = row0 + tid, p = min(row, n - 1) / L.rpp;
        sH[tid] = L.h_dev ? (float)L.h_dev[(long)p * L.h_stride] : L.h_val[p];
        const bool live = row < n && !(L.ctl && L.ctl[(long)p * NLBAC_DOPRI_CTL + C_DONE] > 0.0);
        sLive[tid] = live ? 1.f : 0.f;
        if (live) s_any = 1;
    }
    for (int idx = tid; idx < L.st_lo * NLBAC_MLP_TILE * WP; idx += 256) {
        const int j = idx / (NLBAC_MLP_TILE * WP), rem = idx - j * NLBAC_MLP_TILE * WP;
        const int mm = rem / WP, c = rem - mm * WP, row = row0 + mm;
        sKZ[idx] = (row < n && c < W) ? L.KZ[((long)j * n + row) * W + c] : 0.f;
    }
    __syncthreads();
    if (!s_any) return;                      // (uniform) every problem of this tile has finished its solve
    }

    int fi = 0;                  // (TRAJ) the fine interval, N-1 .. 0: uniform, the one interval index kept in a register
    if constexpr (TRAJ) fi = __builtin_amdgcn_readfirstlane(sT->N) - 1;
    do {         // (one pass, and no loop at all, in the one-step instances)
    if constexpr (TRAJ) {
        const int kb = __builtin_amdgcn_readfirstlane(sT->begin[fi]);
        if (kb >= 0) {           // an output interval's upper end: y <- out[kb+1], a_x <- dout[kb+1] (+ a_x), a_c <- 0, its controls
            const bool add = !(sT->top && fi == sT->N - 1);
            const float* const po = sT->out + (long)(kb + 1) * n * sT->out_ld;
            const float* const pd = sT->dout + (long)(kb + 1) * n * ns;
            const int old = sT->out_ld;
            for (int idx = tid; idx < NLBAC_MLP_TILE * WP; idx += 256) {
                const int mm = idx / WP, c = idx - mm * WP, row = row0 + mm;
                float v = 0.f;
                if (row < n && c < ns) v = po[(long)row * old + c];
                else if (row < n && c < 2 * ns) {
                    const float d = pd[(long)row * ns + (c - ns)];
                    v = add ? d + sZ0[idx] : d;
                }
                sZ0[idx] = v;
            }
            if (tid < NLBAC_MLP_TILE * ADJ_MAX_NU) {
                const int mm = tid >> 2, c = tid & 3, row = row0 + mm;
                sU[tid] = (row < n && c < nu) ? sT->ctl[(long)kb * sT->ctl_stride + (long)row * nu + c] : 0.f;
            }
            if (tid == 0) sI[0] = kb;
        }
        if (tid < NLBAC_MLP_TILE) sH[tid] = sT->hs[fi];
        __syncthreads();
    }
    for (int st = L.st_lo; st < L.st_hi; ++st) {
        // ---- stage input  Z_st = Z0 + h sum_j beta[st][j] K_j  (all of z: y feeds the nets, a_x is the cotangent)
        const long fioff = TRAJ ? (long)fi * L.S_total * n : 0;       // (TRAJ) the fine interval's block of kept rows
        (void)fioff;
        for (int idx = tid; idx < NLBAC_MLP_TILE * WP; idx += 256) {
            const int mm = idx / WP, c = idx - mm * WP;
            float a = sZ0[idx];
            const float h = sH[mm];
            for (int j = 0; j < st; ++j)
                if (L.beta[st][j] != 0.f) a = a + sKZ[(j * NLBAC_MLP_TILE + mm) * WP + c] * (L.beta[st][j] * h);
            sZS[idx] = a;
            if (KEEP && c < W && sLive[mm] != 0.f) L.ZS[((long)st * n + row0 + mm + fioff) * W + c] = a;
            if constexpr (TRAJ && KEEP)
                if (c >= ns && c < 2 * ns && sLive[mm] != 0.f) sT->dK[((long)st * n + row0 + mm + fioff) * ns + (c - ns)] = a * (sCo[st] * h);
        }
        __syncthreads();
        const long srow = (long)st * n + grow + fioff;
        const bool keep_row = KEEP && row_ok && sLive[m] != 0.f;
        (void)srow; (void)keep_row;

        // =========================== forward chain ===========================
        float Ha[KS], Hb[KS];
        f32x4 acc0[NB], acc[NB], bv[NB], bpre[3];
        unsigned wd = 0u;                 // the mask word being assembled
        unsigned mreg[ARR_MAX_W];         // the finished words, one per layer: what the backward half gates with
#pragma unroll
        for (int l = 0; l < ARR_MAX_W; ++l) mreg[l] = 0u;
        auto prefetch_bias = [&](int l) __attribute__((always_inline)) {
#pragma unroll
            for (int jo = 0; jo < G0; ++jo) bpre[jo] = rr_bias<S>(params + boff[l], jo, q);
        };
        prefetch_bias(1);
        auto keep_word = [&](int l, unsigned word) __attribute__((always_inline)) {
            // (static layer index after inlining; rows past the end gate everything off)
#pragma unroll
            for (int ll = 0; ll < ARR_MAX_W; ++ll)
                if (ll == l) mreg[ll] = row_ok ? word : 0u;
        };
        auto save_rows = [&](float* base, int l, int jo, const float (&H)[KS]) __attribute__((always_inline)) {
            if (!keep_row) return;
            f32x4 hv{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int rr = 0; rr < ((jo < NB - 1) ? 4 : R); ++rr) hv[rr] = H[4 * jo + rr];
            rr_row_store<S>(base + (long)l * L.acts_ls[grp] + srow * HID, jo, q, hv);
        };
        auto pre_l0 = [&](int ks) __attribute__((always_inline)) {
            const int jo = (ks < 4 * (NB - 1)) ? (ks >> 2) : NB - 1, r = ks - 4 * jo;
            const float h = rr_relu(acc0[jo][r]);
            Ha[ks] = h;
            rr_mask_push(wd, h);
            if (KEEP && r == ((jo < NB - 1) ? 3 : R - 1)) save_rows(L.acts[grp], 0, jo, Ha);
            if (ks == KS - 1) keep_word(0, wd);
        };
        auto pre_tail_f = [&](int lp, float (&H)[KS], int t) __attribute__((always_inline)) {
            if (t >= NT) return;
            const int jo = TB + (t >> 2), r = t & 3;
            const float h = rr_relu(acc[jo][r]);
            H[4 * TB + t] = h;
            rr_mask_push(wd, h);
            if (KEEP && (t == 3 || t == NT - 1)) save_rows(L.acts[grp], lp, jo, H);
            if (t == NT - 1) keep_word(lp, wd);
        };
        {   // layer 0: K = ns + 1 (one to three k-steps), straight from the stage input's y part
            float yv[3], a0[3][NB];
#pragma unroll
            for (int k0 = 0; k0 < 3; ++k0) {
                const int col = 4 * k0 + q;
                yv[k0] = (col < ns) ? sZS[m * WP + min(col, ns - 1)] : (col == ns ? 1.f : 0.f);
            }
#pragma unroll
            for (int k0 = 0; k0 < 3; ++k0)
#pragma unroll
                for (int jo = 0; jo < NB; ++jo) a0[k0][jo] = (k0 < KL0) ? sW0[((grp * 3 + k0) * 8 + jo) * 64 + lane] : 0.f;
#pragma unroll
            for (int jo = 0; jo < NB; ++jo) {
                acc0[jo] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[0][jo], yv[0], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                if (KL0 > 1) acc0[jo] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[1][jo], yv[1], acc0[jo], 0, 0, 0);
                if (KL0 > 2) acc0[jo] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[2][jo], yv[2], acc0[jo], 0, 0, 0);
            }
        }
        auto wide = [&](auto lc, float (&Hin)[KS], float (&Hout)[KS]) __attribute__((always_inline)) {
            constexpr int l = decltype(lc)::value;
#pragma unroll
            for (int jo = 0; jo < NB; ++jo) bv[jo] = (jo < G0) ? bpre[jo] : rr_bias<S>(params + boff[l], jo, q);
            __builtin_amdgcn_sched_barrier(0);
            const int cur = fbase + (l - 1) * S::LAYER_BYTES;
            // behind the last forward layer the stream turns round: the first backward product's fragments (layer nw-1)
            const int nxt = (l + 1 < nw) ? cur + S::LAYER_BYTES : bbase + (nw - 2) * S::LAYER_BYTES;
            gemm.run(acc, bv, Hin, rs, voff, cur, nxt,
                     [&](int ks) __attribute__((always_inline)) {
                         if (l == 1) pre_l0(ks);
                         else pre_tail_f(l - 1, Hin, ks);
                     },
                     [&](int jo, int r) __attribute__((always_inline)) {
                         const float h = rr_relu(acc[jo][r]);
                         Hout[4 * jo + r] = h;
                         rr_mask_push(wd, h);
                         if (KEEP && r == 3) save_rows(L.acts[grp], l, jo, Hout);
                     },
                     [&]() __attribute__((always_inline)) {
                         if (l + 1 < nw) prefetch_bias(l + 1);
                     });
        };
        auto outl = [&](auto lc, float (&Hin)[KS]) __attribute__((always_inline)) {
            constexpr int l = decltype(lc)::value;
            const f32x4 o = RRGemm<S>::block(wo, Hin, [&](int ks) __attribute__((always_inline)) { pre_tail_f(l - 1, Hin, ks); });
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (o_idx[r] < 0) continue;
                const float val = o[r] + o_bias[r];
                if (grp == 0) sF[m * ADJ_MAX_NS + o_idx[r]] = val;
                else sG[m * ADJ_MAX_GOUT + o_idx[r]] = val;
            }
        };
        using I1 = std::integral_constant<int, 1>; using I2 = std::integral_constant<int, 2>;
        using I3 = std::integral_constant<int, 3>; using I4 = std::integral_constant<int, 4>;
        wide(I1{}, Ha, Hb);
        wide(I2{}, Hb, Ha);
        if (grp == 0) { wide(I3{}, Ha, Hb); outl(I4{}, Hb); }
        else outl(I3{}, Ha);
        __syncthreads();

        // ---- k_y = -(f + g u) ; k_au = g^T a_x
        for (int idx = tid; idx < NLBAC_MLP_TILE * ns; idx += 256) {
            const int mm = idx / ns, r = idx - mm * ns;
            float a = sF[mm * ADJ_MAX_NS + r];
            for (int c = 0; c < nu; ++c) a += sG[mm * ADJ_MAX_GOUT + r * nu + c] * sU[mm * ADJ_MAX_NU + c];
            sKZ[(st * NLBAC_MLP_TILE + mm) * WP + r] = -a;
        }
        for (int idx = tid; idx < NLBAC_MLP_TILE * nu; idx += 256) {
            const int mm = idx / nu, c = idx - mm * nu;
            float a = 0.f;
            for (int r = 0; r < ns; ++r) a += sG[mm * ADJ_MAX_GOUT + r * nu + c] * sZS[mm * WP + ns + r];
            sKZ[(st * NLBAC_MLP_TILE + mm) * WP + 2 * ns + c] = a;
        }

        // =========================== backward chain ===========================
        // cotangents of the two output layers: f: a_x itself, g: a_x u^T — this lane's B operands of the top product
        float dy[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int k0 = (grp == 0) ? e : e / nu, u = (grp == 0) ? 0 : e - k0 * nu, c = 4 * k0 + q;
            const bool ok = (grp == 0) ? (e < KS0 && c < ns) : (e < KS0 * nu && c < ns);
            const float ax = sZS[m * WP + ns + min(c, ns - 1)];
            const float uu = (grp == 0) ? 1.f : sU[m * ADJ_MAX_NU + min(u, nu - 1)];
            dy[e] = ok ? ((grp == 0) ? ax : ax * uu) : 0.f;
            if (KEEP && grp == 1 && ok && keep_row) L.dG[srow * (ns * nu) + c * nu + u] = TRAJ ? dy[e] * (sCo[st] * sH[m]) : dy[e];
        }
        auto save_dz = [&](int l, int jo, const float (&Z)[KS]) __attribute__((always_inline)) {
            if constexpr (TRAJ) {      // (the quadrature weight h c_sol[st] goes on at the store, outside the MFMA chain; it
                if (!keep_row) return; //  is formed here from the step slot in LDS, not held in a register over the stage)
                const float sc = sCo[st] * sH[m];
                f32x4 zv{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int rr = 0; rr < ((jo < NB - 1) ? 4 : R); ++rr) zv[rr] = Z[4 * jo + rr] * sc;
                rr_row_store<S>(L.dz[grp] + (long)l * L.acts_ls[grp] + srow * HID, jo, q, zv);
            }
        };
        float Za[KS], Zb[KS];
        f32x4 acct[NB], zero[NB];
#pragma unroll
        for (int jo = 0; jo < NB; ++jo) zero[jo] = f32x4{0.f, 0.f, 0.f, 0.f};
        unsigned mw = 0u, mwt = 0u;
        auto word_of = [&](int l) __attribute__((always_inline)) {
            unsigned v = 0u;
#pragma unroll
            for (int ll = 0; ll < ARR_MAX_W; ++ll)
                if (ll == l) v = mreg[ll];
            return v;
        };
        auto pre_top = [&](int ks) __attribute__((always_inline)) {
            const int jo = (ks < 4 * (NB - 1)) ? (ks >> 2) : NB - 1, r = ks - 4 * jo;
            Za[ks] = rr_mask_gate<KS>(mwt, ks, acct[jo][r]);
            if (KEEP && r == ((jo < NB - 1) ? 3 : R - 1)) { if constexpr (TRAJ) save_dz(nw - 1, jo, Za); else save_rows(L.dz[grp], nw - 1, jo, Za); }
        };
        int tail_layer = 0;          // (the layer whose dz the pending tail belongs to)
        auto pre_tail_b = [&](float (&Z)[KS], int t) __attribute__((always_inline)) {
            if (t >= NT) return;
            const int jo = TB + (t >> 2), r = t & 3;
            Z[4 * TB + t] = rr_mask_gate<KS>(mwt, 4 * TB + t, acc[jo][r]);
            if (KEEP && (t == 3 || t == NT - 1)) { if constexpr (TRAJ) save_dz(tail_layer, jo, Z); else save_rows(L.dz[grp], tail_layer, jo, Z); }
        };
        mw = word_of(nw - 1);
        {   // top product: dz_top = mask_top * (W_out^T dy)
            float at[4][NB];
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int jo = 0; jo < NB; ++jo) at[e][jo] = (e < 2 || KSO > 2) ? sWt[((grp * 4 + e) * 8 + jo) * 64 + lane] : 0.f;
#pragma unroll
            for (int jo = 0; jo < NB; ++jo) {
                acct[jo] = __builtin_amdgcn_mfma_f32_16x16x4f32(at[0][jo], dy[0], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                acct[jo] = __builtin_amdgcn_mfma_f32_16x16x4f32(at[1][jo], dy[1], acct[jo], 0, 0, 0);
                if (KSO > 2) {
                    acct[jo] = __builtin_amdgcn_mfma_f32_16x16x4f32(at[2][jo], dy[2], acct[jo], 0, 0, 0);
                    acct[jo] = __builtin_amdgcn_mfma_f32_16x16x4f32(at[3][jo], dy[3], acct[jo], 0, 0, 0);
                }
            }
        }
        auto prod = [&](auto pc, float (&Zin)[KS], float (&Zout)[KS]) __attribute__((always_inline)) {
            constexpr int p = decltype(pc)::value;
            const int lo = nw - 1 - p;                            // the layer whose dz this product yields
            mwt = mw;
            mw = word_of(lo);
            __builtin_amdgcn_sched_barrier(0);
            const int cur = bbase + lo * S::LAYER_BYTES;              // fragments of layer lo + 1 sit at index lo
            // behind the last backward product the stream goes on with the next stage's first forward layer
            const int nxt = (lo >= 1) ? cur - S::LAYER_BYTES : fbase;
            gemm.run(acc, zero, Zin, rs, voff, cur, nxt,
                     [&](int ks) __attribute__((always_inline)) {
                         if (p == 1) pre_top(ks);
                         else pre_tail_b(Zin, ks);
                     },
                     [&](int jo, int r) __attribute__((always_inline)) {
                         Zout[4 * jo + r] = rr_mask_gate<KS>(mw, 4 * jo + r, acc[jo][r]);
                         if (KEEP && r == 3) { if constexpr (TRAJ) save_dz(lo, jo, Zout); else save_rows(L.dz[grp], lo, jo, Zout); }
                     },
                     [&]() __attribute__((always_inline)) {});
            tail_layer = lo;          // (this product's own tail is finished inside the next one)
        };
        auto dxl = [&](float (&Zin)[KS]) __attribute__((always_inline)) {
            mwt = mw;
            const f32x4 o = RRGemm<S>::block(w0t, Zin, [&](int ks) __attribute__((always_inline)) { pre_tail_b(Zin, ks); });
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int c = 4 * r + q;
                if (r < KS0 && c < ns) sDX[(grp * NLBAC_MLP_TILE + m) * ADJ_MAX_NS + c] = o[r];
            }
        };
        prod(I1{}, Za, Zb);
        prod(I2{}, Zb, Za);
        if (grp == 0) { prod(I3{}, Za, Zb); dxl(Zb); }
        else dxl(Za);
        __syncthreads();

        // ---- k_ax = dX_f + dX_g; the stage's derivative row goes out
        for (int idx = tid; idx < NLBAC_MLP_TILE * ns; idx += 256) {
            const int mm = idx / ns, c = idx - mm * ns;
            sKZ[(st * NLBAC_MLP_TILE + mm) * WP + ns + c] =
                sDX[mm * ADJ_MAX_NS + c] + sDX[(NLBAC_MLP_TILE + mm) * ADJ_MAX_NS + c];
        }
        __syncthreads();
        if constexpr (!TRAJ)
        for (int idx = tid; idx < NLBAC_MLP_TILE * W; idx += 256) {
            const int mm = idx / W, c = idx - mm * W;
            if (sLive[mm] != 0.f) L.KZ[((long)st * n + row0 + mm) * W + c] = sKZ[(st * NLBAC_MLP_TILE + mm) * WP + c];
        }
    }
    if constexpr (TRAJ) {
        // ---- Z0 <- Z1 in LDS: the step result as the one-step launch forms it (every element by the thread that owns it)
        for (int idx = tid; idx < NLBAC_MLP_TILE * W; idx += 256) {
            const int mm = idx / W, c = idx - mm * W;
            const float h = sH[mm];
            float a = sZ0[mm * WP + c];
            for (int j = 0; j < L.n_out; ++j)
                if (L.c_out[j] != 0.f) a = a + sKZ[(j * NLBAC_MLP_TILE + mm) * WP + c] * (L.c_out[j] * h);
            sZ0[mm * WP + c] = a;
        }
        __syncthreads();
        if (fi == 0 || __builtin_amdgcn_readfirstlane(sT->begin[max(fi - 1, 0)]) >= 0) {
            // (uniform) the output interval's lower end: a_c is its controls' gradient
            const bool assign = sT->du_stride != 0 || sI[1] != 0;
            float* const pu = sT->du + (long)sI[0] * sT->du_stride;
            for (int idx = tid; idx < NLBAC_MLP_TILE * nu; idx += 256) {
                const int mm = idx / nu, c = idx - mm * nu, row = row0 + mm;
                if (row >= n) continue;
                const float a = sZ0[mm * WP + 2 * ns + c];
                float* const p = pu + (long)row * nu + c;
                *p = assign ? a : *p + a;
            }
            __syncthreads();                         // (the next interval's top rewrites these rows, and sI)
            if (tid == 0) sI[1] = 0;
        }
    }
    } while (TRAJ && --fi >= 0);
    if constexpr (TRAJ) {
        for (int idx = tid; idx < NLBAC_MLP_TILE * W; idx += 256) {
            const int mm = idx / W, c = idx - mm * W, row = row0 + mm;
            if (row < n) sT->carry[(long)row * W + c] = sZ0[mm * WP + c];
        }
        return;
    }

    // ---- step outputs
    for (int idx = tid; idx < NLBAC_MLP_TILE * W; idx += 256) {
        const int mm = idx / W, c = idx - mm * W, row = row0 + mm;
        if (sLive[mm] == 0.f) continue;
        const float h = sH[mm];
        if (L.Z1) {
            float a = sZ0[mm * WP + c];
            for (int j = 0; j < L.n_out; ++j)
                if (L.c_out[j] != 0.f) a = a + sKZ[(j * NLBAC_MLP_TILE + mm) * WP + c] * (L.c_out[j] * h);
            L.Z1[(long)row * W + c] = a;
        }
        if (L.ERR) {
            float a = 0.f;
            for (int j = 0; j < L.n_err; ++j)
                if (L.c_err[j] != 0.f) a = a + sKZ[(j * NLBAC_MLP_TILE + mm) * WP + c] * (L.c_err[j] * h);
            L.ERR[(long)row * W + c] = a;
        }
        if (L.ip_out) {
            // the interpolant of z at t_end, should this attempt be accepted and finish the problem's solve (the
            // controller's own test and abscissa: ode_control.h; dopri_interp_fwd_kernel's arithmetic on z1 = the value
            // written to Z1 above)
            const int p = row / L.rpp;
            const double t = L.ctl[(long)p * NLBAC_DOPRI_CTL + C_T], hd = L.ctl[(long)p * NLBAC_DOPRI_CTL + C_H];
            if (t + hd >= L.t_end) {
                const float x = (float)((L.t_end - t) / hd);
                const float a0 = sZ0[mm * WP + c];
                float a1 = a0, k[7];
                for (int j = 0; j < L.n_out; ++j)
                    if (L.c_out[j] != 0.f) a1 = a1 + sKZ[(j * NLBAC_MLP_TILE + mm) * WP + c] * (L.c_out[j] * h);
#pragma unroll
                for (int j = 0; j < 7; ++j) k[j] = sKZ[(j * NLBAC_MLP_TILE + mm) * WP + c];
                L.ip_out[(long)row * W + c] = dopri_interp_value(a0, a1, k, h, x);
            }
        }
    }
}
