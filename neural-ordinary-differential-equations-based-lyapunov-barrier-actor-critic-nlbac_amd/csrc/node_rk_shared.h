// What the two families of fused Runge-Kutta step kernels of the control-affine NODE  dx/dt = f(x) + g(x) u  share:
// the launch descriptors and the per-tile bookkeeping around the layer chains (tile constants, stage algebra, step
// outputs, the in-launch step control).  The families differ in how a 32-row tile's layer chains run:
//   node_kernels.hip     LDS-tiled: 8 waves, activations in LDS ping-pong tiles, any width up to 256
//   node_rr_kernels.hip  register-resident: 4 waves, one (net, 16 rows) chain per wave, widths <= 128
// Reference: torchdiffeq.odeint at U/sac_cbf_clf/sac_cbf_clf.py:453,577 and U/sac_cbf_clf/model.py:252 over
// NeuralODEModel.forward (model.py:208-217).
#pragma once
#include "mlp_device.h"
#include "ode_control.h"

#define NODE_LDS_MAX (160 * 1024 - 64)   /* dynamic LDS per workgroup; the rest holds the static group-barrier counters */
#define RK_MAX_STAGES 8
#define RK_MAX_NS 8
#define RK_MAX_NU 4
#define RK_MAX_GOUT (RK_MAX_NS * RK_MAX_NU)

struct NodeRkLaunch {
    nlbac_mlp net[2];                 // f, g
    const float* y0; const float* u;
    int n, rpp, n_s, n_u;
    int stage_begin, stage_end, S_total;
    float beta[RK_MAX_STAGES][RK_MAX_STAGES];
    float c_out[RK_MAX_STAGES]; int n_out;
    float c_err[RK_MAX_STAGES]; int n_err;
    const double* h_dev; int h_stride; float h_val[8];
    float* K; float* Y; float* G;
    float* acts[2]; long acts_ls[2];
    int acts_bits;                    // acts hold bit-packed ReLU masks [layer][stage*n + row][words per row] (uint32)
    float* out; float* err;
    int ld;
    int sw_off1;                      // float offset of g_net's output-layer block behind f_net's in LDS
    // device-driven dopri5 chain (nlbac_rk_chain): problems whose solve is done are skipped; the step's buffers (K, Y,
    // G, acts, err) are those of step slot C_NACC, `slot_floats` floats apart; a slot > 0 starts from its predecessor's
    // last stage (y1 = Y[6], FSAL K[6]).  norm_mode >= 0: the scaled norms of nlbac_dopri_norm_control and the step
    // controller run in this launch's epilogue (last workgroup of each problem).
    const double* ctl; long slot_floats;
    int norm_mode, n_slots; float rtol, atol; double t_end;
    float* partials; unsigned* tickets; double* ctl_w; double* hslots;
    double* alog; int alog_cap;       // attempt log [P][alog_cap][3] = (h tried, error ratio, accepted) or null
    // nlbac_in_map: the solve's initial state is formed by this launch (stage 0 of a fresh step) from observation rows
    // and written to y0 for the launches that follow; kind 1 = the Unicycle tasks' state (+ its look-ahead point)
    int in_kind; const float* in_obs; int in_obs_ld; float in_l; float* in_ps; float* y0_w;
    // nlbac_rk_chain::interp_*: an attempt whose step reaches t_end also evaluates the solve's result — the interpolant
    // at t_end, and the owner's out-map of it — for its rows (register-resident kernels; what nlbac_dopri_interp_fwd
    // does as a launch of its own after the accept decision; a rejected attempt's values are overwritten by the next)
    float* ip_out; int ip_kind; float ip_l; float* ip_p;
    // nlbac_rk_chain::norm_defer / norm_pre: the fused norm WITHOUT its election.  norm_defer: the epilogue only leaves
    // this tile's partial sums (plain stores); norm_pre = 1 + mode: every workgroup of THIS launch sums the partials the
    // previous launch left (partials_pre, the same fixed order) and runs that mode's controller itself before its first
    // stage — the step size it yields is this launch's; the problem's first tile writes the control block.
    int norm_defer, norm_pre; const float* partials_pre;
};

struct NodeRkBwdLaunch {
    nlbac_mlp net[2];
    const float* u; const float* G;
    const float* acts[2]; long acts_ls[2];
    int acts_bits;                    // acts hold bit-packed ReLU masks (see NodeRkLaunch)
    float* dz[2]; float* dG;
    float* dK; const float* dYup;
    float* dy0; int dy0_in;
    float* du; int du_acc;
    int n, rpp, n_s, n_u, S_total, st_lo, st_hi, dx_stage0;
    float beta[RK_MAX_STAGES][RK_MAX_STAGES];
    const double* h_dev; int h_stride; float h_val[8];
    int ld, sw_off1;
    // device-driven chain: launch `back_idx` differentiates step slot C_NACC - back_idx of each problem (problems with
    // fewer accepted steps are skipped); back_idx 0 is every problem's LAST step (dK / dy0 / dYup come from the
    // interpolant's backward), the others start from the slot behind them: dK[6] = its dK[0] (FSAL), dYup = its dy0.
    // Step sizes come from hslots[p][slot].
    const double* ctl; long slot_floats; int back_idx, n_slots; const double* hslots;
    // nlbac_rk_chain::interp_*: launch back_idx 0 forms dK / dy0 / dy1 of each problem's last step itself, from
    // d loss / d y(t_end) (ip_dout) or, with the out-map, from d loss / d p (ip_dp [+ ip_dp2]) and the solve's output
    // ip_x — what nlbac_dopri_interp_bwd does as a launch of its own (register-resident kernels)
    int ip_on, ip_kind; float ip_l; const float *ip_dout, *ip_dp, *ip_dp2, *ip_x;
};

// The register-resident kernels (node_rr_kernels.hip): 0 = launched, 1 = these nets / this launch are not theirs (the
// LDS-tiled kernels take it), < 0 = error.
int nlbac_node_rr_fwd_launch(NodeRkLaunch& L, hipStream_t s);
int nlbac_node_rr_bwd_launch(NodeRkBwdLaunch& L, hipStream_t s);
bool nlbac_node_rr_eligible(const nlbac_mlp* f, const nlbac_mlp* g);
// what the trajectory kernels (node_traj_kernels.hip) select by, as the one-step launchers do: the width's template
// shape (0, 1, 2 for 64, 100, 128; -1 none)
int nlbac_node_rr_shape(int hid);

// ---------------------------------------------------------------------------------------------------------------
// forward: the small per-tile arrays in LDS
// ---------------------------------------------------------------------------------------------------------------
struct RkFwdTile {
    float* sK;     // [stage][32][8]   stage derivatives
    float* sY0;    // [32][8]          the step's initial state
    float* sU;     // [32][4]          actions
    float* sH;     // [32]             step size per row
    float* sF;     // [32][8]          f(x) of the current stage
    float* sG;     // [32][32]         g(x) of the current stage
    __host__ __device__ __forceinline__ static constexpr int floats() {
        return RK_MAX_STAGES * NLBAC_MLP_TILE * RK_MAX_NS + NLBAC_MLP_TILE * (RK_MAX_NS + RK_MAX_NU + 1 + RK_MAX_NS + RK_MAX_GOUT);
    }
    __device__ __forceinline__ void carve(float* p) {
        sK = p;
        sY0 = sK + RK_MAX_STAGES * NLBAC_MLP_TILE * RK_MAX_NS;
        sU = sY0 + NLBAC_MLP_TILE * RK_MAX_NS;
        sH = sU + NLBAC_MLP_TILE * RK_MAX_NU;
        sF = sH + NLBAC_MLP_TILE;
        sG = sF + NLBAC_MLP_TILE * RK_MAX_NS;
    }
};

// where a tile's step lives: its problem, step slot and FSAL source (device-driven chain) — false: the problem is done
struct RkFwdWhere {
    int p_tile; long soff; bool fsal;
    float *gK, *gY, *gG, *gErr; const float* gy0;
    bool ip; float ip_x;         // this attempt reaches t_end: evaluate the interpolant at abscissa ip_x (nlbac_rk_chain::interp_out)
    double h_pre;                // norm_pre: the step size this launch's own controller produced (rk_fwd_norm_pre)
};
__device__ __forceinline__ bool rk_fwd_where(const NodeRkLaunch& L, int row0, RkFwdWhere& w) {
    w.p_tile = row0 / L.rpp;
    w.soff = 0;
    w.fsal = false;
    w.ip = false;
    w.ip_x = 0.f;
    w.h_pre = 0.0;
    if (L.ctl) {
        const double* c = L.ctl + (long)w.p_tile * NLBAC_DOPRI_CTL;
        if (c[C_DONE] > 0.0) return false;              // (uniform) this problem's solve has finished
        const int slot = (int)c[C_NACC];
        w.soff = (long)slot * L.slot_floats;
        w.fsal = slot > 0;
        if (L.ip_out && !L.norm_pre) {      // the controller's own test and abscissa (ode_control.h: accept && t + h >= t_end -> C_X)
            const double t = c[C_T], h = c[C_H];
            w.ip = t + h >= L.t_end;
            w.ip_x = (float)((L.t_end - t) / h);
        }
    }
    w.gK = L.K + w.soff;
    w.gY = L.Y + w.soff;
    w.gG = L.G + w.soff;
    w.gErr = L.err ? L.err + w.soff : nullptr;
    w.gy0 = w.fsal ? (w.gY - L.slot_floats) + (long)(L.S_total - 1) * L.n * L.n_s : L.y0;
    return true;
}

// nlbac_rk_chain::norm_pre: the controller of the norm whose tile partials the previous launch left, run by every
// workgroup for its own problem: the sums in the order the elected workgroup of the fused form takes them (same bits),
// dopri_control_vals on a private copy of the block; the problem's first tile runs it on the block itself, for the
// launches that follow.  What a launch saves this way is the previous launch's election: two device-scope atomic round
// trips per workgroup behind its stores, the last workgroup's sums and controller with the whole chip idle, ~10 us per
// one-stage launch; what it pays is this reduction (L2-resident loads, one fp64 pow) under its own prologue's loads.
// Contains a barrier.
template <int NTHR>
__device__ __forceinline__ void rk_fwd_norm_pre(const NodeRkLaunch& L, RkFwdWhere& w, int row0, int tid) {
    __shared__ double s_hpre_[2];
    const int mode = L.norm_pre - 1, p = w.p_tile;
    if (tid < 64) {
        const int nblk = (L.rpp + NLBAC_MLP_TILE - 1) / NLBAC_MLP_TILE;
        double d0 = 0.0, d1 = 0.0;
        for (int b = tid; b < nblk; b += 64) {
            const float* q = L.partials_pre + ((long)p * nblk + b) * 2;
            d0 += (double)q[0];
            d1 += (double)q[1];
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { d0 += __shfl_down(d0, off, 64); d1 += __shfl_down(d1, off, 64); }
        if (tid == 0) {
            const double cnt = (double)L.rpp * (double)(L.n_s + L.n_u);
            const double n0 = sqrt(d0 / cnt), n1 = sqrt(d1 / cnt);
            double* c = L.ctl_w + (long)p * NLBAC_DOPRI_CTL;
            double loc[NLBAC_DOPRI_CTL];
#pragma unroll
            for (int k = 0; k < NLBAC_DOPRI_CTL; ++k) loc[k] = 0.0;
            if (mode == 1) { loc[C_H0] = c[C_H0]; loc[C_D1] = c[C_D1]; }     // (what mode 1 reads: the previous launch's first tile wrote them)
            dopri_control_vals(n0, n1, 0, mode, L.t_end, loc, L.n_slots);
            if (row0 == p * L.rpp) dopri_control_vals(n0, n1, p, mode, L.t_end, L.ctl_w, L.n_slots);
            s_hpre_[0] = mode == 0 ? loc[C_H0] : loc[C_H];
            s_hpre_[1] = mode == 0 ? 0.0 : c[C_T];
        }
    }
    __syncthreads();
    w.h_pre = s_hpre_[0];
    if (L.ip_out) {
        const double t = s_hpre_[1], h = w.h_pre;
        w.ip = t + h >= L.t_end;
        w.ip_x = (float)((L.t_end - t) / h);
    }
}

// tile constants: y0 (or the in-map's state), u, h, already-known stages (FSAL / f0 from an earlier launch).
// Contains barriers; ends with one.
template <int NTHR>
__device__ __forceinline__ void rk_fwd_tile_constants(const NodeRkLaunch& L, RkFwdWhere& w, const RkFwdTile& T,
                                                      int row0, int tid) {
    const int n = L.n, ns = L.n_s, nu = L.n_u;
    if (L.in_kind == 1 && !w.fsal) {
        // same arithmetic as unicycle_state_kernel (the reference takes arctan2 on the host in float64 and casts back)
        for (int idx = tid; idx < NLBAC_MLP_TILE * RK_MAX_NS; idx += NTHR) T.sY0[idx] = 0.f;
        __syncthreads();
        if (tid < NLBAC_MLP_TILE && row0 + tid < n) {
            const int row = row0 + tid, i = row % L.rpp;
            const float* o = L.in_obs + (long)i * L.in_obs_ld;
            const float th = (float)atan2((double)o[3], (double)o[2]);
            T.sY0[tid * RK_MAX_NS + 0] = o[0]; T.sY0[tid * RK_MAX_NS + 1] = o[1]; T.sY0[tid * RK_MAX_NS + 2] = th;
            L.y0_w[(long)row * 3 + 0] = o[0]; L.y0_w[(long)row * 3 + 1] = o[1]; L.y0_w[(long)row * 3 + 2] = th;
            if (L.in_ps && row < L.rpp) {
                L.in_ps[i * 2 + 0] = o[0] + L.in_l * cosf(th);
                L.in_ps[i * 2 + 1] = o[1] + L.in_l * sinf(th);
            }
        }
    }
    // Every global load below is issued before the first LDS store that consumes one (clamped addresses, selects
    // afterwards): written as "sX[idx] = cond ? load : 0" statement by statement — and as a loop with a run-time bound for
    // the earlier stages — each was a global round trip of its own, several microseconds of a launch's prologue in a row.
    {
        constexpr int NY = (NLBAC_MLP_TILE * RK_MAX_NS + NTHR - 1) / NTHR, NU = (NLBAC_MLP_TILE * RK_MAX_NU + NTHR - 1) / NTHR;
        constexpr int NK = (RK_MAX_STAGES * NLBAC_MLP_TILE * RK_MAX_NS + NTHR - 1) / NTHR;
        const bool plain_y0 = !(L.in_kind == 1 && !w.fsal);
        float vy[NY], vu[NU], vk[NK], vh = 0.f;
#pragma unroll
        for (int it = 0; it < NY; ++it) {
            const int idx = tid + NTHR * it, m = (idx >> 3) & (NLBAC_MLP_TILE - 1), c = idx & 7;
            vy[it] = plain_y0 ? w.gy0[(long)min(row0 + m, n - 1) * ns + min(c, ns - 1)] : 0.f;
        }
#pragma unroll
        for (int it = 0; it < NU; ++it) {
            const int idx = tid + NTHR * it, m = (idx >> 2) & (NLBAC_MLP_TILE - 1), c = idx & 3;
            vu[it] = L.u[(long)min(row0 + m, n - 1) * nu + min(c, nu - 1)];
        }
        if (tid < NLBAC_MLP_TILE) {
            const int p = min(row0 + tid, n - 1) / L.rpp;
            vh = L.h_dev ? (float)L.h_dev[(long)p * L.h_stride] : L.h_val[p];
        }
#pragma unroll
        for (int it = 0; it < NK; ++it) {
            const int idx = tid + NTHR * it;
            const int j = idx / (NLBAC_MLP_TILE * RK_MAX_NS), rem = idx - j * NLBAC_MLP_TILE * RK_MAX_NS;
            const int m = rem >> 3, c = rem & 7;
            const long rc = (long)min(row0 + m, n - 1) * ns + min(c, ns - 1);
            float v = 0.f;
            if (j < L.stage_begin) {          // (uniform per wave: a stage's block is a multiple of 64 entries)
                if (w.fsal && j == 0) v = (w.gK - L.slot_floats)[(long)(L.S_total - 1) * n * ns + rc];   // first stage = the previous slot's last
                else v = w.gK[(long)j * n * ns + rc];
            }
            vk[it] = v;
        }
        // nlbac_rk_chain::norm_pre: the step size of this launch comes from the previous launch's tile partials — summed
        // HERE, behind the row loads above (their trips to memory overlap; in front of them the two latencies added up)
        if (L.norm_pre) {
            rk_fwd_norm_pre<NTHR>(L, w, row0, tid);
            vh = (float)w.h_pre;
        }
#pragma unroll
        for (int it = 0; it < NY; ++it) {
            const int idx = tid + NTHR * it, m = idx >> 3, c = idx & 7;
            if (plain_y0 && idx < NLBAC_MLP_TILE * RK_MAX_NS) T.sY0[idx] = (row0 + m < n && c < ns) ? vy[it] : 0.f;
        }
#pragma unroll
        for (int it = 0; it < NU; ++it) {
            const int idx = tid + NTHR * it, m = idx >> 2, c = idx & 3;
            if (idx < NLBAC_MLP_TILE * RK_MAX_NU) T.sU[idx] = (row0 + m < n && c < nu) ? vu[it] : 0.f;
        }
        if (tid < NLBAC_MLP_TILE) T.sH[tid] = vh;
#pragma unroll
        for (int it = 0; it < NK; ++it) {
            const int idx = tid + NTHR * it;
            const int j = idx / (NLBAC_MLP_TILE * RK_MAX_NS), rem = idx - j * NLBAC_MLP_TILE * RK_MAX_NS;
            const int m = rem >> 3, c = rem & 7, row = row0 + m;
            if (j < L.stage_begin) {
                const float v = (row < n && c < ns) ? vk[it] : 0.f;
                T.sK[idx] = v;
                if (w.fsal && j == 0 && row < n && c < ns) w.gK[(long)row * ns + c] = v;      // kept in this slot for the interpolant
            }
        }
    }
    __syncthreads();
}

// stage input  Y_st = y0 + h sum_j beta[st][j] K_j  of the launch's FIRST stage (same op order as rk_combine_kernel),
// for the threads [t, t + nthr, ...) of one consumer: written to `in` (row stride LD, columns ns..inp-1 zero) and, by
// the consumer that `owns` the global copy, to Y
__device__ __forceinline__ void rk_fwd_first_input(const NodeRkLaunch& L, const RkFwdWhere& w, const RkFwdTile& T,
                                                   int row0, int st, int inp, float* in, int LD, bool owns, int t,
                                                   int nthr) {
    const int n = L.n, ns = L.n_s;
    for (int idx = t; idx < NLBAC_MLP_TILE * inp; idx += nthr) {
        const int m = idx / inp, c = idx - m * inp;
        float a = 0.f;
        if (c < ns) {
            a = T.sY0[m * RK_MAX_NS + c];
            const float h = T.sH[m];
            for (int j = 0; j < st; ++j)
                if (L.beta[st][j] != 0.f) a = a + T.sK[(j * NLBAC_MLP_TILE + m) * RK_MAX_NS + c] * (L.beta[st][j] * h);
            if (owns && row0 + m < n) w.gY[((long)st * n + row0 + m) * ns + c] = a;
        }
        in[m * LD + c] = a;
    }
}

// k = f + g u   (same op order as affine_fwd_kernel), and — same thread, same (row, component) — the next stage's input
// Y_{st+1} = y0 + h sum_j beta[st+1][j] K_j into in_f (and in_g when given; row stride LD, columns ns..inp-1 zeroed
// again).  Call between two workgroup barriers: reads sF / sG of the stage, nothing else touches the input tiles.
template <int NTHR>
__device__ __forceinline__ void rk_fwd_combine(const NodeRkLaunch& L, const RkFwdWhere& w, const RkFwdTile& T, int row0,
                                               int st, int inp, float* in_f, float* in_g, int LD, int tid) {
    const int n = L.n, ns = L.n_s, nu = L.n_u;
    const bool more = st + 1 < L.stage_end;
    for (int idx = tid; idx < NLBAC_MLP_TILE * inp; idx += NTHR) {
        const int m = idx / inp, c = idx - m * inp;
        float y = 0.f;
        if (c < ns) {
            float a = T.sF[m * RK_MAX_NS + c];
            for (int q = 0; q < nu; ++q) a += T.sG[m * RK_MAX_GOUT + c * nu + q] * T.sU[m * RK_MAX_NU + q];
            T.sK[(st * NLBAC_MLP_TILE + m) * RK_MAX_NS + c] = a;
            if (row0 + m < n) w.gK[((long)st * n + row0 + m) * ns + c] = a;
            if (more) {
                y = T.sY0[m * RK_MAX_NS + c];
                const float h = T.sH[m];
                for (int j = 0; j < st; ++j)
                    if (L.beta[st + 1][j] != 0.f) y = y + T.sK[(j * NLBAC_MLP_TILE + m) * RK_MAX_NS + c] * (L.beta[st + 1][j] * h);
                if (L.beta[st + 1][st] != 0.f) y = y + a * (L.beta[st + 1][st] * h);
                if (row0 + m < n) w.gY[((long)(st + 1) * n + row0 + m) * ns + c] = y;
            }
        }
        if (more) { in_f[m * LD + c] = y; if (in_g) in_g[m * LD + c] = y; }
    }
}

// step outputs (solution / error combination) and, with norm_mode >= 0, the fused step control: this tile's partial
// sums of the scaled norms (same per-entry arithmetic as dopri_norm_block), one ticket per problem; the last workgroup
// of a problem sums the tile partials in a fixed order and runs the controller.  Contains a barrier when norm_mode >= 0
// (every thread of the workgroup must call it).
template <int NTHR>
__device__ __forceinline__ void rk_fwd_outputs_and_control(const NodeRkLaunch& L, const RkFwdWhere& w, const RkFwdTile& T,
                                                           int row0, int n_rows, int tid) {
    const int n = L.n, ns = L.n_s, nu = L.n_u, p_tile = w.p_tile;
    const float *sK = T.sK, *sY0 = T.sY0, *sU = T.sU, *sH = T.sH;
    for (int idx = tid; idx < NLBAC_MLP_TILE * ns; idx += NTHR) {
        const int m = idx / ns, r = idx - m * ns, row = row0 + m;
        if (row >= n) continue;
        const float h = sH[m];
        if (L.out) {
            float a = sY0[m * RK_MAX_NS + r];
            for (int j = 0; j < L.n_out; ++j)
                if (L.c_out[j] != 0.f) a = a + sK[(j * NLBAC_MLP_TILE + m) * RK_MAX_NS + r] * (L.c_out[j] * h);
            L.out[(long)row * ns + r] = a;
        }
        if (w.gErr) {
            float a = 0.f;
            for (int j = 0; j < L.n_err; ++j)
                if (L.c_err[j] != 0.f) a = a + sK[(j * NLBAC_MLP_TILE + m) * RK_MAX_NS + r] * (L.c_err[j] * h);
            w.gErr[(long)row * ns + r] = a;
            if (L.norm_mode == 2) {
                // the error norm's term of this (row, component) — one per thread here; the row sums follow below (one
                // thread per row doing all of its components' 13-term chains in a row cost the attempt launch 4 us)
                const float y = sY0[m * RK_MAX_NS + r];
                float y1 = y;
                const int sl = L.S_total - 1;         // y1 = the last stage's input
                for (int j = 0; j < sl; ++j)
                    if (L.beta[sl][j] != 0.f) y1 = y1 + sK[(j * NLBAC_MLP_TILE + m) * RK_MAX_NS + r] * (L.beta[sl][j] * h);
                const float tol = L.atol + L.rtol * fmaxf(fabsf(y), fabsf(y1));
                const float q = a / tol;
                T.sG[m * RK_MAX_NS + r] = q * q;      // (g(x) of the last stage is no longer needed)
            }
        }
    }
    if (w.ip) {      // (uniform per tile) the solve's result, should this attempt be accepted: one (row, component) per thread
        static_assert(NTHR >= NLBAC_MLP_TILE * RK_MAX_NS, "one (row, component) per thread");
        const int m = tid >> 3, r = tid & 7, row = row0 + m, sl = L.S_total - 1;
        if (tid < NLBAC_MLP_TILE * RK_MAX_NS && r < ns) {
            const float h = sH[m];
            const float a0 = sY0[m * RK_MAX_NS + r];
            float k[7], bl[RK_MAX_STAGES];
#pragma unroll
            for (int j = 0; j < 7; ++j) k[j] = sK[(j * NLBAC_MLP_TILE + m) * RK_MAX_NS + r];
#pragma unroll
            for (int j = 0; j < RK_MAX_STAGES; ++j) bl[j] = L.beta[sl][j];
            float a1 = a0;                            // y1 = the last stage's input (the expression that wrote Y[6])
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                const float t = a1 + k[j] * (bl[j] * h);
                a1 = (j < sl && bl[j] != 0.f) ? t : a1;
            }
            const float o = dopri_interp_value(a0, a1, k, h, w.ip_x);
            if (row < n) L.ip_out[(long)row * ns + r] = o;
            T.sF[m * RK_MAX_NS + r] = o;              // (f(x) of the last stage is no longer needed)
        }
        if (L.ip_kind == 1) {
            __syncthreads();
            if (tid < 2 * NLBAC_MLP_TILE) {          // the look-ahead point: component `which` of row mm
                const int mm = tid >> 1, which = tid & 1, rw = row0 + mm;
                const float th = T.sF[mm * RK_MAX_NS + 2];
                const float v = T.sF[mm * RK_MAX_NS + which] + L.ip_l * (which ? sinf(th) : cosf(th));
                if (rw < n) L.ip_p[(long)rw * 2 + which] = v;
            }
        }
    }
    if (L.norm_mode < 0) return;
    __shared__ unsigned s_last;
    if (L.norm_mode == 2) __syncthreads();         // (uniform) the terms in sG
    if (tid < 64) {
        const int m = tid;
        float v0 = 0.f, v1 = 0.f;
        if (m < n_rows) {
            for (int r = 0; r < ns; ++r) {
                const float y = sY0[m * RK_MAX_NS + r];
                if (L.norm_mode == 2) {
                    v0 += T.sG[m * RK_MAX_NS + r];
                } else {
                    const float sc = L.atol + fabsf(y) * L.rtol;
                    if (L.norm_mode == 0) {
                        const float q0 = y / sc, q1 = sK[m * RK_MAX_NS + r] / sc;
                        v0 += q0 * q0; v1 += q1 * q1;
                    } else {
                        const float q = (sK[(NLBAC_MLP_TILE + m) * RK_MAX_NS + r] - sK[m * RK_MAX_NS + r]) / sc;
                        v0 += q * q;
                    }
                }
            }
            if (L.norm_mode == 0)
                for (int c = 0; c < nu; ++c) {
                    const float y = sU[m * RK_MAX_NU + c];
                    const float q = y / (L.atol + fabsf(y) * L.rtol);
                    v0 += q * q;
                }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { v0 += __shfl_down(v0, off, 64); v1 += __shfl_down(v1, off, 64); }
        if (tid == 0) {
            const int nblk = (L.rpp + NLBAC_MLP_TILE - 1) / NLBAC_MLP_TILE;
            const int blk = (row0 - p_tile * L.rpp) / NLBAC_MLP_TILE;
            float* q = L.partials + ((long)p_tile * nblk + blk) * 2;
            if (L.norm_defer) { q[0] = v0; q[1] = v1; }        // (the next launch sums them: rk_fwd_norm_pre)
            else {
            // No agent-scope fence here: on gfx950 a release at agent scope writes the XCD's whole L2 back, and this
            // workgroup has just written the step's K / Y / masks (measured: +15 us on a one-stage launch, +30 us on an
            // attempt).  The two partial sums go out as device-scope atomic exchanges — performed at the level all
            // XCDs see — and the ticket is only taken once both have RETURNED; the last workgroup reads them with
            // device-scope atomic loads.  Everything else this kernel wrote is for later launches (kernel boundary).
            const float o0 = __hip_atomic_exchange(q + 0, v0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const float o1 = __hip_atomic_exchange(q + 1, v1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("" ::"v"(o0), "v"(o1) : "memory");
            const unsigned ticket = __hip_atomic_fetch_add(L.tickets + p_tile, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            s_last = (ticket == (unsigned)nblk - 1u) ? 1u : 0u;
            if (s_last) __hip_atomic_store(L.tickets + p_tile, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    if (L.norm_defer) return;                  // (uniform)
    __syncthreads();
    if (!s_last || tid >= 64) return;
    {
        const int nblk = (L.rpp + NLBAC_MLP_TILE - 1) / NLBAC_MLP_TILE;
        double d0 = 0.0, d1 = 0.0;
        for (int b = tid; b < nblk; b += 64) {
            const float* q = L.partials + ((long)p_tile * nblk + b) * 2;
            d0 += (double)__hip_atomic_load(q + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            d1 += (double)__hip_atomic_load(q + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { d0 += __shfl_down(d0, off, 64); d1 += __shfl_down(d1, off, 64); }
        if (tid == 0) {
            const double cnt = (double)L.rpp * (double)(ns + nu);
            double* c = L.ctl_w + (long)p_tile * NLBAC_DOPRI_CTL;
            const int slot_before = (int)c[C_NACC];
            const double h_try = c[C_H];
            dopri_control_vals(sqrt(d0 / cnt), sqrt(d1 / cnt), p_tile, L.norm_mode, L.t_end, L.ctl_w, L.n_slots);
            if (L.norm_mode == 2 && L.hslots && c[C_ACCEPT] > 0.0)
                L.hslots[(long)p_tile * L.n_slots + slot_before] = h_try;      // step size of the accepted step in its slot
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

// ---------------------------------------------------------------------------------------------------------------
// backward: the small per-tile arrays in LDS
// ---------------------------------------------------------------------------------------------------------------
struct RkBwdTile {
    float* sDK;    // [stage][32][8]   dL/dK_j
    float* sU;     // [32][4]
    float* sH;     // [32]
    float* sDY0;   // [32][8]          running dy0
    float* sDU;    // [32][4]          running du
    float* sDX;    // [2][32][8]       dX of f_net / g_net for the current stage
    float* sDYup;  // [32][8]          dL/dy1 of the step when the launch forms it itself (nlbac_rk_chain::interp_*)
    __host__ __device__ __forceinline__ static constexpr int floats() {
        return RK_MAX_STAGES * NLBAC_MLP_TILE * RK_MAX_NS + NLBAC_MLP_TILE * (RK_MAX_NU + 1 + RK_MAX_NS + RK_MAX_NU + 2 * RK_MAX_NS + RK_MAX_NS);
    }
    __device__ __forceinline__ void carve(float* p) {
        sDK = p;
        sU = sDK + RK_MAX_STAGES * NLBAC_MLP_TILE * RK_MAX_NS;
        sH = sU + NLBAC_MLP_TILE * RK_MAX_NU;
        sDY0 = sH + NLBAC_MLP_TILE;
        sDU = sDY0 + NLBAC_MLP_TILE * RK_MAX_NS;
        sDX = sDU + NLBAC_MLP_TILE * RK_MAX_NU;
        sDYup = sDX + 2 * NLBAC_MLP_TILE * RK_MAX_NS;
    }
};

struct RkBwdWhere {
    long soff; int slot; bool chained, carry;
    bool ip;       // this launch forms the step's dK / dy0 / dy1 from the gradient of the solve's result (interpolant backward)
    const float* gG; float* gdG; float* gdK; float* gdy0; const float* gdYup;
    int st_lo; bool stage0_data;
    __device__ __forceinline__ bool has_data(int st) const { return st >= st_lo && (st > 0 || stage0_data); }
};
__device__ __forceinline__ bool rk_bwd_where(const NodeRkBwdLaunch& L, int row0, RkBwdWhere& w) {
    w.soff = 0;
    w.slot = 0;
    w.chained = L.ctl != nullptr;
    if (w.chained) {
        const int p_tile = row0 / L.rpp;
        w.slot = (int)L.ctl[(long)p_tile * NLBAC_DOPRI_CTL + C_NACC] - L.back_idx;
        if (w.slot < 0) return false;                       // (uniform) this problem took fewer steps
        w.soff = (long)w.slot * L.slot_floats;
    }
    w.carry = w.chained && L.back_idx > 0;    // not the problem's last step: gradients arrive from the slot behind
    w.ip = L.ip_on && w.chained && !w.carry;
    w.gG = L.G + w.soff;
    w.gdG = L.dG ? L.dG + w.soff : nullptr;
    w.gdK = L.dK + w.soff;
    w.gdy0 = L.dy0 ? L.dy0 + w.soff : nullptr;
    w.gdYup = w.carry ? w.gdy0 + L.slot_floats : (L.dYup ? L.dYup + w.soff : nullptr);
    w.st_lo = w.chained ? (w.slot == 0 ? 0 : 1) : L.st_lo;    // (a later step's stage 0 is its predecessor's last stage)
    w.stage0_data = L.dx_stage0 || L.dz[0] != nullptr;
    return true;
}

// u, running du / dy0, h, dK of the tile -> LDS.  No barrier inside.
template <int NTHR>
__device__ __forceinline__ void rk_bwd_tile_constants(const NodeRkBwdLaunch& L, const RkBwdWhere& w, const RkBwdTile& T,
                                                      int row0, int tid) {
    const int n = L.n, ns = L.n_s, nu = L.n_u;
    // (all global loads first, then the LDS stores: see rk_fwd_tile_constants)
    constexpr int NY = (NLBAC_MLP_TILE * RK_MAX_NS + NTHR - 1) / NTHR, NU = (NLBAC_MLP_TILE * RK_MAX_NU + NTHR - 1) / NTHR;
    constexpr int NK = (RK_MAX_STAGES * NLBAC_MLP_TILE * RK_MAX_NS + NTHR - 1) / NTHR;
    const bool du_in = L.du && L.du_acc, dy_in = w.gdy0 && L.dy0_in && !w.carry && !w.ip;
    float vu[NU], vdu[NU], vy[NY], vk[NK], vh = 0.f;
    float ip_g = 0.f, ip_h = 0.f, ip_xx = 0.f;
    if (w.ip) {      // (uniform) this thread's (row, component) of d loss / d y(t_end): every load up front with the others
        static_assert(NTHR == NLBAC_MLP_TILE * RK_MAX_NS, "one (row, component) per thread");
        const int m = tid >> 3, c = tid & 7, row = min(row0 + m, n - 1), p = row / L.rpp;
        ip_h = (float)L.ctl[(long)p * NLBAC_DOPRI_CTL + C_HUSED];
        ip_xx = (float)L.ctl[(long)p * NLBAC_DOPRI_CTL + C_X];
        if (L.ip_kind == 1) {        // out-map 1 (ode_kernels.hip::dopri_interp_bwd_kernel's arithmetic)
            float d0 = L.ip_dp[(long)row * 2 + 0], d1 = L.ip_dp[(long)row * 2 + 1];
            if (L.ip_dp2) { d0 += L.ip_dp2[(long)row * 2 + 0]; d1 += L.ip_dp2[(long)row * 2 + 1]; }
            const float th = L.ip_x[(long)row * ns + 2];
            const float g2 = L.ip_l * (-sinf(th) * d0 + cosf(th) * d1);
            ip_g = c == 0 ? d0 : (c == 1 ? d1 : (c == 2 ? g2 : 0.f));
        } else {
            ip_g = L.ip_dout[(long)row * ns + min(c, ns - 1)];
        }
    }
#pragma unroll
    for (int it = 0; it < NU; ++it) {
        const int idx = tid + NTHR * it, m = (idx >> 2) & (NLBAC_MLP_TILE - 1), c = idx & 3;
        const long rc = (long)min(row0 + m, n - 1) * nu + min(c, nu - 1);
        vu[it] = L.u[rc];
        vdu[it] = du_in ? L.du[rc] : 0.f;
    }
#pragma unroll
    for (int it = 0; it < NY; ++it) {
        const int idx = tid + NTHR * it, m = (idx >> 3) & (NLBAC_MLP_TILE - 1), c = idx & 7;
        vy[it] = dy_in ? w.gdy0[(long)min(row0 + m, n - 1) * ns + min(c, ns - 1)] : 0.f;
    }
    if (tid < NLBAC_MLP_TILE) {
        const int p = min(row0 + tid, n - 1) / L.rpp;
        vh = w.chained ? (float)L.hslots[(long)p * L.n_slots + w.slot]
                       : (L.h_dev ? (float)L.h_dev[(long)p * L.h_stride] : L.h_val[p]);
    }
#pragma unroll
    for (int it = 0; it < NK; ++it) {
        const int idx = tid + NTHR * it;
        const int j = idx / (NLBAC_MLP_TILE * RK_MAX_NS), rem = idx - j * NLBAC_MLP_TILE * RK_MAX_NS;
        const int m = rem >> 3, c = rem & 7;
        const long rc = (long)min(row0 + m, n - 1) * ns + min(c, ns - 1);
        float v = 0.f;
        if (j < L.st_hi && !w.ip) {           // (uniform per wave)
            if (!w.carry) v = w.gdK[(long)j * n * ns + rc];
            else if (j == L.S_total - 1) v = (w.gdK + L.slot_floats)[rc];     // FSAL: next slot's dK[0]
        }
        vk[it] = v;
    }
    if (w.ip) {
        float d0v, d1v, dk[7];
        dopri_interp_grad(ip_g, ip_h, ip_xx, d0v, d1v, dk);
        const bool ok = row0 + (tid >> 3) < n && (tid & 7) < ns;
        vy[0] = d0v;
        T.sDYup[tid] = ok ? d1v : 0.f;
#pragma unroll
        for (int it = 0; it < NK; ++it)
            if (it < 7) vk[it] = dk[it];
    }
#pragma unroll
    for (int it = 0; it < NU; ++it) {
        const int idx = tid + NTHR * it, m = idx >> 2, c = idx & 3;
        if (idx < NLBAC_MLP_TILE * RK_MAX_NU) {
            const bool ok = row0 + m < n && c < nu;
            T.sU[idx] = ok ? vu[it] : 0.f;
            T.sDU[idx] = ok ? vdu[it] : 0.f;
        }
    }
#pragma unroll
    for (int it = 0; it < NY; ++it) {
        const int idx = tid + NTHR * it, m = idx >> 3, c = idx & 7;
        if (idx < NLBAC_MLP_TILE * RK_MAX_NS) T.sDY0[idx] = (row0 + m < n && c < ns) ? vy[it] : 0.f;
    }
    if (tid < NLBAC_MLP_TILE) T.sH[tid] = vh;
#pragma unroll
    for (int it = 0; it < NK; ++it) {
        const int idx = tid + NTHR * it;
        const int j = idx / (NLBAC_MLP_TILE * RK_MAX_NS), rem = idx - j * NLBAC_MLP_TILE * RK_MAX_NS;
        const int m = rem >> 3, c = rem & 7;
        if (j < L.st_hi) T.sDK[idx] = (row0 + m < n && c < ns) ? vk[it] : 0.f;
    }
}

// du += g(Y_st)^T dK_st for the tile's rows
template <int NTHR>
__device__ __forceinline__ void rk_bwd_du(const NodeRkBwdLaunch& L, const RkBwdWhere& w, const RkBwdTile& T, int row0,
                                          int st, int tid) {
    if (!L.du) return;
    const int n = L.n, ns = L.n_s, nu = L.n_u, gout = ns * nu;
    for (int idx = tid; idx < NLBAC_MLP_TILE * nu; idx += NTHR) {
        const int m = idx / nu, c = idx - m * nu, row = min(row0 + m, n - 1);
        float a = 0.f;
        for (int r = 0; r < ns; ++r)
            a += w.gG[((long)st * n + row) * gout + r * nu + c] * T.sDK[(st * NLBAC_MLP_TILE + m) * RK_MAX_NS + r];
        T.sDU[m * RK_MAX_NU + c] = T.sDU[m * RK_MAX_NU + c] + 1.0f * a;
    }
}

// the stage algebra once both nets' dX sit in sDX: dY = [dYup at the last stage] + dX_f + dX_g; dy0 += dY;
// dK[j] += beta[st][j] h dY (j < st)
template <int NTHR>
__device__ __forceinline__ void rk_bwd_stage_algebra(const NodeRkBwdLaunch& L, const RkBwdWhere& w, const RkBwdTile& T,
                                                     int row0, int st, int tid) {
    const int n = L.n, ns = L.n_s;
    for (int idx = tid; idx < NLBAC_MLP_TILE * ns; idx += NTHR) {
        const int m = idx / ns, c = idx - m * ns, row = row0 + m;
        float d = (w.gdYup && !w.ip && st == L.S_total - 1 && row < n) ? w.gdYup[(long)row * ns + c] : 0.f;
        if (w.ip && st == L.S_total - 1) d = T.sDYup[m * RK_MAX_NS + c];
        d += T.sDX[m * RK_MAX_NS + c];
        d += T.sDX[(NLBAC_MLP_TILE + m) * RK_MAX_NS + c];
        T.sDY0[m * RK_MAX_NS + c] = T.sDY0[m * RK_MAX_NS + c] + d;
        const float h = T.sH[m];
        for (int j = 0; j < st; ++j)
            if (L.beta[st][j] != 0.f) T.sDK[(j * NLBAC_MLP_TILE + m) * RK_MAX_NS + c] += (L.beta[st][j] * h) * d;
    }
}

// dK, dy0, du of the tile -> global
template <int NTHR>
__device__ __forceinline__ void rk_bwd_outputs(const NodeRkBwdLaunch& L, const RkBwdWhere& w, const RkBwdTile& T,
                                               int row0, int tid) {
    const int n = L.n, ns = L.n_s, nu = L.n_u;
    for (int idx = tid; idx < L.st_hi * NLBAC_MLP_TILE * ns; idx += NTHR) {
        const int j = idx / (NLBAC_MLP_TILE * ns), rem = idx - j * NLBAC_MLP_TILE * ns;
        const int m = rem / ns, c = rem - m * ns, row = row0 + m;
        if (row < n) w.gdK[((long)j * n + row) * ns + c] = T.sDK[(j * NLBAC_MLP_TILE + m) * RK_MAX_NS + c];
    }
    if (w.gdy0)
        for (int idx = tid; idx < NLBAC_MLP_TILE * ns; idx += NTHR) {
            const int m = idx / ns, c = idx - m * ns, row = row0 + m;
            if (row < n) w.gdy0[(long)row * ns + c] = T.sDY0[m * RK_MAX_NS + c];
        }
    if (L.du)
        for (int idx = tid; idx < NLBAC_MLP_TILE * nu; idx += NTHR) {
            const int m = idx / nu, c = idx - m * nu, row = row0 + m;
            if (row < n) L.du[(long)row * nu + c] = T.sDU[m * RK_MAX_NU + c];
        }
}

// ---------------------------------------------------------------------------------------------------------------
// one-launch fixed-grid trajectories (node_traj_kernels.hip): H intervals of euler / rk4 with a new action per interval,
// every row on its own — a tile walks the intervals one after the other, no workgroup waits for another
// GRID (nlbac_node_rk_grid_*: the solution on a time grid): the intervals have a step size each (hs[k], written to sH
// by the body at the top of interval k) and ONE set of actions u [n][n_u] for all of them; the backward sums the
// intervals' du in the tile's LDS (sDYup, which only the interpolant's backward uses otherwise), k = H-1 .. 0:
//     total = du_{H-1};  total = total + du_k  —  the fp32 adds the chained path does between its launches
// SUB (with GRID; nlbac_node_rk_subgrid_*: a time grid under step_size): the intervals are the N fine intervals and the
// outputs are the T - 1 points read off them (NlbacSubGrid, common.h): the forward writes out[j-1] for the outputs j of
// interval k in place of the interval's state; the backward forms interval k's d from sum_j theta_j dout[j] and adds
// sum_j (1 - theta_j) dout[j] to the dy0 it hands to interval k-1 (resp. to dx0).  With every weight 1 these are the
// GRID kernels' fp32 operations on the fine grid with zero dout at the unused points.
// HOLD (with GRID, not SUB; nlbac_node_rk_hold_*: a rollout under step_size): the intervals are N = H m fine intervals,
// i = k m + r: control interval k's actions u[k] held over its m fine steps hs[r] (the same schedule in every control
// interval).  The forward replaces the actions in sU behind r = m-1 and writes out[k] there only; the backward takes
// dout[k+1] at r = m-1 (d = 0 + the carried dy0 elsewhere, SUB's fine interval without an output), sums du inside a
// control interval as GRID sums it over its grid (total = du_{m-1}; total = total + du_r) and writes du[k] at r = 0.
// ---------------------------------------------------------------------------------------------------------------
struct NodeRkTrajBwd {
    int H;
    const float* dout;                // [H+1][n][n_s] dL/d(rollout output)
    float* dx0;                       // [n][n_s]
    float c_out[RK_MAX_STAGES]; int n_out;
};

// forward, behind interval k's last stage: out[k] = y0 + h sum_j c_j K_j (rk_fwd_outputs_and_control's arithmetic) to
// global and, as interval k+1's y0, to sY0; interval k+1's actions to sU.  One (row, component) per thread; ends with a
// barrier (every thread must call it).
template <int NTHR, bool GRID = false, bool SUB = false, bool HOLD = false>
__device__ __forceinline__ void rk_traj_advance(const NodeRkLaunch& L, const RkFwdTile& T, int row0, int k, int H, int tid,
                                                const NlbacSubGrid* sub = nullptr, int hm = 1) {
    static_assert(NTHR >= NLBAC_MLP_TILE * RK_MAX_NS, "one (row, component) per thread");
    const int n = L.n, ns = L.n_s, nu = L.n_u;
    const int kc = HOLD ? k / hm : k;          // (HOLD) the control interval, whose last fine step this is or is not
    const bool last = !HOLD || k - kc * hm == hm - 1;
    // (GRID: the actions in sU are every interval's; HOLD: the control interval's, replaced behind its last fine step)
    const bool more = (HOLD ? last : !GRID) && k + 1 < H;
    float vu = 0.f;
    if (more && tid < NLBAC_MLP_TILE * RK_MAX_NU) {
        const int m = tid >> 2, c = tid & 3;
        vu = L.u[(long)(kc + 1) * n * nu + (long)min(row0 + m, n - 1) * nu + min(c, nu - 1)];
    }
    if (tid < NLBAC_MLP_TILE * RK_MAX_NS) {
        const int m = tid >> 3, r = tid & 7, row = row0 + m;
        if (r < ns && row < n) {
            const float h = T.sH[m];
            float a = T.sY0[m * RK_MAX_NS + r];
            for (int j = 0; j < L.n_out; ++j)
                if (L.c_out[j] != 0.f) a = a + T.sK[(j * NLBAC_MLP_TILE + m) * RK_MAX_NS + r] * (L.c_out[j] * h);
            if constexpr (SUB) {      // (before sY0 is overwritten: the thread holds the old state and the new one)
                const float y_old = T.sY0[m * RK_MAX_NS + r];
                const int j1 = sub->ofs[k + 1];
                for (int j = sub->ofs[k]; j < j1; ++j)
                    L.out[(long)(j - 1) * n * ns + (long)row * ns + r] = nlbac_sub_point(y_old, a, sub->theta[j - 1]);
            } else {
                if (last) L.out[(long)kc * n * ns + (long)row * ns + r] = a;
            }
            T.sY0[m * RK_MAX_NS + r] = a;
        }
    }
    if (more && tid < NLBAC_MLP_TILE * RK_MAX_NU) {
        const int m = tid >> 2, c = tid & 3;
        T.sU[tid] = (row0 + m < n && c < nu) ? vu : 0.f;
    }
    __syncthreads();
}

// backward, before interval k's stages (kk = H-1-k intervals done): u_k -> sU, du = 0, and from
// d = dout[k+1] (+ the dy0 of interval k+1, in sDY0 when kk > 0): dy0 = 0 + d, dK_j = 0 + (c_j h) d — what
// nlbac_rk_stage_bwd leaves for the one-step backward (same arithmetic).  No barrier inside.
template <int NTHR, bool GRID = false, bool SUB = false, bool HOLD = false>
__device__ __forceinline__ void rk_traj_bwd_begin(const NodeRkBwdLaunch& L, const NodeRkTrajBwd& X, const RkBwdTile& T,
                                                  int row0, int k, int kk, int tid, const float* hs = nullptr,
                                                  const NlbacSubGrid* sub = nullptr, int hm = 1) {
    static_assert(NTHR >= NLBAC_MLP_TILE * RK_MAX_NS, "one (row, component) per thread");
    const int n = L.n, ns = L.n_s, nu = L.n_u;
    float vu = 0.f, vd = 0.f;
    const int kc = HOLD ? k / hm : k, kr = k - kc * hm;  // (HOLD) control interval and fine step inside it
    const float vh = GRID ? hs[HOLD ? kr : k] : L.h_val[0];          // (one problem: one step size for every row)
    if (tid < NLBAC_MLP_TILE * RK_MAX_NU) {
        const int m = tid >> 2, c = tid & 3;
        vu = L.u[(long)(HOLD ? kc : (GRID ? 0 : k)) * n * nu + (long)min(row0 + m, n - 1) * nu + min(c, nu - 1)];
    }
    if (tid < NLBAC_MLP_TILE * RK_MAX_NS) {
        const int m = tid >> 3, c = tid & 7;
        if constexpr (SUB) vd = nlbac_sub_gather<true>(*sub, X.dout, (long)n * ns, (long)min(row0 + m, n - 1) * ns + min(c, ns - 1), k, 0.f);
        else if (HOLD && kr != hm - 1) vd = 0.f;          // (no output behind this fine step)
        else vd = X.dout[(long)(kc + 1) * n * ns + (long)min(row0 + m, n - 1) * ns + min(c, ns - 1)];
    }
    if (tid < NLBAC_MLP_TILE * RK_MAX_NU) {
        const int m = tid >> 2, c = tid & 3;
        const bool ok = row0 + m < n && c < nu;
        T.sU[tid] = ok ? vu : 0.f;
        T.sDU[tid] = 0.f;
    }
    if (tid < NLBAC_MLP_TILE) T.sH[tid] = vh;
    if (tid < NLBAC_MLP_TILE * RK_MAX_NS) {
        const int m = tid >> 3, c = tid & 7;
        const bool ok = row0 + m < n && c < ns;
        float d = vd;
        if constexpr (SUB) {      // interval k+1's outputs' share of its initial state joins its dy0 here, by the thread that holds it
            if (kk > 0) d = d + nlbac_sub_gather<false>(*sub, X.dout, (long)n * ns, (long)min(row0 + m, n - 1) * ns + min(c, ns - 1), k + 1, T.sDY0[tid]);
        } else {
            if (kk > 0) d = d + T.sDY0[tid];
        }
        T.sDY0[tid] = ok ? 0.f + d : 0.f;
        for (int j = 0; j < RK_MAX_STAGES; ++j) {
            float v = 0.f;
            if (j < X.n_out && X.c_out[j] != 0.f) v = 0.f + (X.c_out[j] * vh) * d;
            if (j < L.S_total) T.sDK[j * NLBAC_MLP_TILE * RK_MAX_NS + tid] = ok ? v : 0.f;
        }
    }
}

// backward, behind interval k's stages: du_k (and dK when the weight gradients want it) to global; the dy0 stays in sDY0
// for interval k-1, after interval 0 dx0 = dout[0] + dy0.  No barrier inside.
template <int NTHR, bool GRID = false, bool SUB = false, bool HOLD = false>
__device__ __forceinline__ void rk_traj_bwd_end(const NodeRkBwdLaunch& L, const NodeRkTrajBwd& X, const RkBwdWhere& w,
                                                const RkBwdTile& T, int row0, int k, int tid,
                                                const NlbacSubGrid* sub = nullptr, int hm = 1) {
    const int n = L.n, ns = L.n_s, nu = L.n_u;
    if (w.gdK)
        for (int idx = tid; idx < L.st_hi * NLBAC_MLP_TILE * ns; idx += NTHR) {
            const int j = idx / (NLBAC_MLP_TILE * ns), rem = idx - j * NLBAC_MLP_TILE * ns;
            const int m = rem / ns, c = rem - m * ns, row = row0 + m;
            if (row < n) w.gdK[((long)j * n + row) * ns + c] = T.sDK[(j * NLBAC_MLP_TILE + m) * RK_MAX_NS + c];
        }
    for (int idx = tid; idx < NLBAC_MLP_TILE * nu; idx += NTHR) {
        const int m = idx / nu, c = idx - m * nu, row = row0 + m;
        if constexpr (HOLD) {       // (GRID's sum below, afresh in every control interval)
            const int kc = k / hm, kr = k - kc * hm;
            float a = T.sDU[m * RK_MAX_NU + c];
            if (kr != hm - 1) a = T.sDYup[m * RK_MAX_NU + c] + a;
            T.sDYup[m * RK_MAX_NU + c] = a;
            if (kr == 0 && row < n) L.du[(long)kc * n * nu + (long)row * nu + c] = a;
        } else if constexpr (GRID) {       // (the same thread holds (m, c) in every interval: no barrier between them)
            float a = T.sDU[m * RK_MAX_NU + c];
            if (k != X.H - 1) a = T.sDYup[m * RK_MAX_NU + c] + a;
            T.sDYup[m * RK_MAX_NU + c] = a;
            if (k == 0 && row < n) L.du[(long)row * nu + c] = a;
        } else {
            if (row < n) L.du[(long)k * n * nu + (long)row * nu + c] = T.sDU[m * RK_MAX_NU + c];
        }
    }
    if (k == 0)
        for (int idx = tid; idx < NLBAC_MLP_TILE * ns; idx += NTHR) {
            const int m = idx / ns, c = idx - m * ns, row = row0 + m;
            if constexpr (SUB) {      // interval 0's outputs' share of the initial state joins its dy0 first
                if (row < n)
                    X.dx0[(long)row * ns + c] = X.dout[(long)row * ns + c] +
                        nlbac_sub_gather<false>(*sub, X.dout, (long)n * ns, (long)row * ns + c, 0, T.sDY0[m * RK_MAX_NS + c]);
            } else {
                if (row < n) X.dx0[(long)row * ns + c] = X.dout[(long)row * ns + c] + T.sDY0[m * RK_MAX_NS + c];
            }
        }
}

// ---------------------------------------------------------------------------------------------------------------
// dopri5 under tile-local step control (node_tile_kernels.hip): every 32-row tile is an adaptive solve of its own — its
// own error norm, step sizes and accept decisions — so a tile never waits for another workgroup and a whole horizon of
// H control intervals is ONE launch.  Per interval the tile does what the chained solve's launches do for a batch of
// its rows, in their order: stage 0, the norm of mode 0 and its controller; the probe stage f(y0 + h0 f0), mode 1;
// attempts of stages 1-6 (stage 0 = the accepted step before: FSAL) with the error norm and the controller behind each,
// until an accepted step reaches dt; the interpolant there.  The control block lives in LDS; one lane runs the
// controller (fp64, one pow) in a function of its own, outside the stage loop's live ranges.
// What a backward needs is kept per (slot, stage, row), a slot per ACCEPTED step, counted per tile over the whole
// horizon (a rejected attempt overwrites its slot): G, mask words / activation rows, stage inputs Y — the [k][stage][row]
// layout of the fixed-grid kernels with the slot in place of k — and per tile the slots' step sizes, per interval its
// first slot, its accepted count and the interpolation abscissa.
// Every loop has a bound from the launch's arguments: H intervals, NODE_TILE_MAX_ATTEMPTS attempts per interval,
// max_slots slots.  A tile that hits one stops: status, NaN into its rows of the outputs from that interval on.
// PAGED (page0 non-null; the *_paged_* entry points): the slots are counted per tile.  Everything kept per (slot, stage,
// row) lies in pages of S stages x 32 rows, tile j owning the pages page0[j] .. page0[j+1] - 1 (page0 [tiles + 1]: the
// exclusive prefix sum of the tiles' slot counts, `pages` their total): slot s of the tile is page page0[j] + s, and
// stage st, tile row m of it sits at stage-row index (page S + st) 32 + m — the index above with 32 in place of n, 0 in
// place of the tile's first row and the page in place of the slot (NodeTilePlace: the three substitutes, once per
// workgroup).  hslots is indexed by page; iv_first / ov_slot and the slot arithmetic stay relative to the tile.  What is
// read of page0 is clamped to the pages, so that no content of it takes an index outside the buffers.
// ---------------------------------------------------------------------------------------------------------------
#define NODE_TILE_MAX_ATTEMPTS 1000      /* per interval: the chained solve's own cap (ode_dopri.py) */
enum { TILE_OK = 0, TILE_NO_SLOT = 1, TILE_MAX_ATTEMPTS = 2 };

struct NodeTileFwd {
    int H;
    int keep;                         // a backward follows: accepted steps are kept in slots
    int max_slots;                    // (keep) slots a tile has for the whole horizon; PAGED: the pages of all tiles
    const int* page0;                 // (keep, PAGED) [tiles + 1] a tile's first page; null: max_slots slots for every tile
    double* hslots;                   // (keep) [tile][max_slots] the kept steps' sizes; PAGED: [page]
    int* iv_first;                    // (keep) [tile][H] interval k's first slot
    float* iv_x;                      // (keep) [tile][H] the abscissa of out[k+1] in interval k's last step
    int* accepted;                    // [tile][H] accepted steps of interval k
    int* attempts;                    // [tile][H] attempted steps of interval k
    int* status;                      // [tile] TILE_*
};

struct NodeTileBwd {
    int H, max_slots;                 // (max_slots, page0, hslots: as in NodeTileFwd)
    const int* page0;
    const double* hslots; const int* iv_first; const int* iv_nacc; const float* iv_x;
    const float* dout;                // [H+1][n][n_s]
    float* dx0;                       // [n][n_s]
};

// DENSE (node_tile_dense_kernels.hip: odeint_dense under tile-local step control): the tile runs ONE interval of length
// tau[n_out - 1] and reads it at the n_out output times tau (device doubles, increasing) — behind every ACCEPTED attempt
// it emits the pending outputs the step reaches, out[j] = the step's interpolant at x = (float)((tau_j - t) / h) with
// t the controller's C_T before it moved (dopri_dense_fwd_kernel's walk, ode_kernels.hip).  When a backward follows,
// ov_slot / ov_x [tile][n_out] record the slot that emitted output j and its abscissa.
struct NodeTileDenseFwd {
    const double* tau;                // [n_out]
    int n_out;
    int* ov_slot;                     // (keep) [tile][n_out]
    float* ov_x;                      // (keep) [tile][n_out]
};

struct NodeTileDenseBwd {
    int n_out;
    const int* ov_slot; const float* ov_x;
};

// Where workgroup `tile` keeps its steps: the rows of a kept stage (kn) and the tile's first row there (krow0), its first
// page (page; 0 when every tile has max_slots slots: the slot is the page), its slots, the stage sets the buffers hold
// (total: what the layer stride of the BITS-2 words counts) and the index of its slot 0 in hslots.
struct NodeTilePlace {
    int kn, krow0, page, slots, total;
    long hbase;
};
__device__ __forceinline__ NodeTilePlace rk_tile_place(const int* page0, int max_slots, int n, int row0, int tile) {
    NodeTilePlace p;
    if (page0) {      // (uniform)
        const int pages = max(max_slots, 1);
        const int p0 = min(max(page0[tile], 0), pages), p1 = min(max(page0[tile + 1], 0), pages);
        p.slots = max(p1 - p0, 1);
        p.page = min(p0, pages - p.slots);
        p.kn = NLBAC_MLP_TILE; p.krow0 = 0; p.total = pages; p.hbase = p.page;
    } else {
        p.kn = n; p.krow0 = row0; p.page = 0; p.slots = max_slots; p.total = max_slots;
        p.hbase = (long)tile * max_slots;
    }
    return p;
}

// the tile's ints in LDS (TI_OUT: DENSE, the outputs emitted so far)
enum { TI_SLOT = 0, TI_OUT = 1, TI_COUNT = 4 };

// the controller on the tile's finished squared-norm sums (a batch of `cnt` entries), on the block in LDS
static __device__ __attribute__((noinline)) void rk_tile_controller(double s0, double s1, double cnt, int mode,
                                                                    double t_end, double* ctl) {
    dopri_control_vals(sqrt(s0 / cnt), sqrt(s1 / cnt), 0, mode, t_end, ctl);
}

// the first stage's input of a phase (rk_fwd_first_input's arithmetic; probe: the table row is (1, 0, ...)), to sYin
// and, when the slot keeps its stage inputs, to gY
__device__ __forceinline__ void rk_tile_first_input(const NodeRkLaunch& L, const RkFwdTile& T, int row0, int st, bool probe,
                                                    float* gY, int kn, int krow0, float* in, int t, int nthr) {
    const int n = L.n, ns = L.n_s;
    for (int idx = t; idx < NLBAC_MLP_TILE * 8; idx += nthr) {
        const int m = idx >> 3, c = idx & 7;
        float a = 0.f;
        if (c < ns) {
            a = T.sY0[m * RK_MAX_NS + c];
            const float h = T.sH[m];
            for (int j = 0; j < st; ++j) {
                const float b = probe ? (j == 0 ? 1.f : 0.f) : L.beta[st][j];
                if (b != 0.f) a = a + T.sK[(j * NLBAC_MLP_TILE + m) * RK_MAX_NS + c] * (b * h);
            }
            if (gY && row0 + m < n) gY[((long)st * kn + krow0 + m) * ns + c] = a;
        }
        in[m * 8 + c] = a;
    }
}

// the tile stops in interval k: NaN into its rows of out[k ..], its status.  No barrier inside.
template <int NTHR>
__device__ __forceinline__ void rk_tile_stop(const NodeRkLaunch& L, const NodeTileFwd& X, int row0, int k, int status, int tid) {
    const int n = L.n, ns = L.n_s;
    const float nanv = __int_as_float(0x7fc00000);
    for (int kk = k; kk < X.H; ++kk)
        for (int idx = tid; idx < NLBAC_MLP_TILE * ns; idx += NTHR) {
            const int m = idx / ns, r = idx - m * ns;
            if (row0 + m < n) L.out[(long)kk * n * ns + (long)(row0 + m) * ns + r] = nanv;
        }
    if (tid == 0) X.status[row0 / NLBAC_MLP_TILE] = status;
}

// (DENSE) the tile stops: NaN into its rows of every output it has not emitted (j0 = sInt[TI_OUT], read behind the
// barrier that ends rk_tile_after_phase), its status and the counts so far.  No barrier inside.
template <int NTHR>
__device__ __forceinline__ void rk_tile_dense_stop(const NodeRkLaunch& L, const NodeTileFwd& X, const NodeTileDenseFwd& D,
                                                   const double* sCtl, int row0, int j0, int status, int tid) {
    const int n = L.n, ns = L.n_s;
    const float nanv = __int_as_float(0x7fc00000);
    for (int j = max(j0, 0); j < D.n_out; ++j)
        for (int idx = tid; idx < NLBAC_MLP_TILE * ns; idx += NTHR) {
            const int m = idx / ns, r = idx - m * ns;
            if (row0 + m < n) L.out[(long)j * n * ns + (long)(row0 + m) * ns + r] = nanv;
        }
    if (tid == 0) {
        const int tile = row0 / NLBAC_MLP_TILE;
        X.status[tile] = status;
        X.accepted[tile] = (int)sCtl[C_NACC];
        X.attempts[tile] = (int)sCtl[C_NSTEPS];
    }
}

// behind a phase's stages (ph 0: stage 0; 1: the probe; >= 2: an attempt): the tile's norm of that mode (the per-entry
// arithmetic of rk_fwd_outputs_and_control, summed as rk_fwd_norm_pre sums one tile), the controller, and what its
// decision asks for — the next phase's step size in sH; an accepted step's size into its slot; behind an accepted
// step that stops short of dt the next step's y0 = y1 (the last stage's input, sYin) and K_0 = K_6 (FSAL); behind one
// that reaches dt out[k] = the interpolant there, the next interval's state and actions.  Returns 0: go on, 1: the
// interval is done, 2 / 3: no slot is left for the next step of this interval / for interval k + 1 (the tile stops).
// DENSE (H = 1, D the output times): nothing is interpolated at dt; behind an ACCEPTED attempt, before the hand-over,
// every (row, component) thread writes the pending outputs the step reaches (the walk over tau is uniform), and the
// interval is done when an accepted step reaches dt = tau[n_out - 1] — by then every output is out.
// P: where the tile keeps its steps — its own slot count is the limit, its hslots start at P.hbase.
// Every thread calls it; contains barriers, ends with one.
template <int NTHR, bool DENSE = false>
__device__ __forceinline__ int rk_tile_after_phase(const NodeRkLaunch& L, const NodeTileFwd& X, const NodeTilePlace& P,
                                                   const RkFwdTile& T, const float* sYin, double* sCtl, int* sInt,
                                                   int row0, int n_rows, int k, int ph, int slot, int tid,
                                                   const NodeTileDenseFwd* D = nullptr) {
    static_assert(NTHR == NLBAC_MLP_TILE * RK_MAX_NS, "one (row, component) per thread");
    const int n = L.n, ns = L.n_s, nu = L.n_u, tile = row0 / NLBAC_MLP_TILE;
    const int mode = ph < 2 ? ph : 2;
    const float *sK = T.sK, *sY0 = T.sY0, *sU = T.sU, *sH = T.sH;
    const int m8 = tid >> 3, r8 = tid & 7, row8 = row0 + m8;
    float o = 0.f;
    // (DENSE) the step's start and size before the controller moves them, the outputs emitted so far
    [[maybe_unused]] double d_t = 0.0, d_hd = 0.0;
    [[maybe_unused]] int d_j = 0;
    if (mode == 2) {      // the error estimate's term of this (row, component) and, if the step reaches dt, the interpolant there
        const double t = sCtl[C_T], hd = sCtl[C_H];
        const bool ip = !DENSE && t + hd >= L.t_end;
        const float ipx = (float)((L.t_end - t) / hd);
        if constexpr (DENSE) { d_t = t; d_hd = hd; d_j = sInt[TI_OUT]; }
        if (r8 < ns) {
            const int sl = L.S_total - 1;
            const float h = sH[m8];
            float a = 0.f;
            for (int j = 0; j < L.n_err; ++j)
                if (L.c_err[j] != 0.f) a = a + sK[(j * NLBAC_MLP_TILE + m8) * RK_MAX_NS + r8] * (L.c_err[j] * h);
            const float y = sY0[m8 * RK_MAX_NS + r8];
            float y1 = y;
            for (int j = 0; j < sl; ++j)
                if (L.beta[sl][j] != 0.f) y1 = y1 + sK[(j * NLBAC_MLP_TILE + m8) * RK_MAX_NS + r8] * (L.beta[sl][j] * h);
            const float tol = L.atol + L.rtol * fmaxf(fabsf(y), fabsf(y1));
            const float q = a / tol;
            T.sG[m8 * RK_MAX_NS + r8] = q * q;
            if (ip) {      // (uniform)
                float kk[7], bl[RK_MAX_STAGES];
#pragma unroll
                for (int j = 0; j < 7; ++j) kk[j] = sK[(j * NLBAC_MLP_TILE + m8) * RK_MAX_NS + r8];
#pragma unroll
                for (int j = 0; j < RK_MAX_STAGES; ++j) bl[j] = L.beta[sl][j];
                float a1 = y;
#pragma unroll
                for (int j = 0; j < 6; ++j) {
                    const float tt = a1 + kk[j] * (bl[j] * h);
                    a1 = (j < sl && bl[j] != 0.f) ? tt : a1;
                }
                o = dopri_interp_value(y, a1, kk, h, ipx);
            }
        }
        __syncthreads();
    }
    if (tid < 64) {
        const int m = tid;
        float v0 = 0.f, v1 = 0.f;
        if (m < n_rows) {
            for (int r = 0; r < ns; ++r) {
                const float y = sY0[m * RK_MAX_NS + r];
                if (mode == 2) {
                    v0 += T.sG[m * RK_MAX_NS + r];
                } else {
                    const float sc = L.atol + fabsf(y) * L.rtol;
                    if (mode == 0) {
                        const float q0 = y / sc, q1 = sK[m * RK_MAX_NS + r] / sc;
                        v0 += q0 * q0; v1 += q1 * q1;
                    } else {
                        const float q = (sK[(NLBAC_MLP_TILE + m) * RK_MAX_NS + r] - sK[m * RK_MAX_NS + r]) / sc;
                        v0 += q * q;
                    }
                }
            }
            if (mode == 0)
                for (int c = 0; c < nu; ++c) {
                    const float y = sU[m * RK_MAX_NU + c];
                    const float q = y / (L.atol + fabsf(y) * L.rtol);
                    v0 += q * q;
                }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { v0 += __shfl_down(v0, off, 64); v1 += __shfl_down(v1, off, 64); }
        if (tid == 0) {
            rk_tile_controller((double)v0, (double)v1, (double)n_rows * (double)(ns + nu), mode, L.t_end, sCtl);
            if (!DENSE && mode == 0 && X.keep) X.iv_first[(long)tile * X.H + k] = slot;
        }
    }
    __syncthreads();
    if (mode < 2) {
        if (tid < NLBAC_MLP_TILE) T.sH[tid] = (float)sCtl[mode == 0 ? C_H0 : C_H];
        __syncthreads();
        return 0;
    }
    const bool accept = sCtl[C_ACCEPT] > 0.0, done = sCtl[C_DONE] > 0.0;      // (uniform)
    int ret = done ? 1 : 0;
    if (accept && tid == 0 && X.keep) X.hslots[P.hbase + slot] = sCtl[C_HUSED];
    if constexpr (DENSE) {
        if (accept) {      // (uniform) the outputs this step reaches: a0 = y0, a1 = the last stage's input, K_0..6 as the slots hold them
            const double tn = d_t + d_hd;
            int j = min(max(d_j, 0), D->n_out);
            if (j < D->n_out && tn >= D->tau[j]) {
                const float h = (float)d_hd, a0 = sY0[m8 * RK_MAX_NS + r8], a1 = sYin[m8 * 8 + r8];
                float kk[7];
#pragma unroll
                for (int s = 0; s < 7; ++s) kk[s] = sK[(s * NLBAC_MLP_TILE + m8) * RK_MAX_NS + r8];
                do {
                    const float x = (float)((D->tau[j] - d_t) / d_hd);
                    const float v = dopri_interp_value(a0, a1, kk, h, x);
                    if (r8 < ns && row8 < n) L.out[(long)j * n * ns + (long)row8 * ns + r8] = v;
                    if (tid == 0 && X.keep) {
                        D->ov_slot[(long)tile * D->n_out + j] = slot;
                        D->ov_x[(long)tile * D->n_out + j] = x;
                    }
                    ++j;
                } while (j < D->n_out && tn >= D->tau[j]);
            }
            if (tid == 0) sInt[TI_OUT] = j;
        }
        if (done && tid == 0) {
            X.accepted[tile] = (int)sCtl[C_NACC] + 1;
            X.attempts[tile] = (int)sCtl[C_NSTEPS];
        }
    }
    if (!DENSE && done) {
        // out[k] and the next interval's state; its actions
        const bool more = k + 1 < X.H;
        float vu = 0.f;
        if (more && tid < NLBAC_MLP_TILE * RK_MAX_NU) {
            const int m = tid >> 2, c = tid & 3;
            vu = L.u[(long)(k + 1) * n * nu + (long)min(row0 + m, n - 1) * nu + min(c, nu - 1)];
        }
        if (r8 < ns && row8 < n) {
            L.out[(long)k * n * ns + (long)row8 * ns + r8] = o;
            T.sY0[m8 * RK_MAX_NS + r8] = o;
        }
        if (more && tid < NLBAC_MLP_TILE * RK_MAX_NU) {
            const int m = tid >> 2, c = tid & 3;
            T.sU[tid] = (row0 + m < n && c < nu) ? vu : 0.f;
        }
        if (tid == 0) {
            X.accepted[(long)tile * X.H + k] = (int)sCtl[C_NACC] + 1;
            X.attempts[(long)tile * X.H + k] = (int)sCtl[C_NSTEPS];
            if (X.keep) X.iv_x[(long)tile * X.H + k] = (float)sCtl[C_X];
        }
    } else {
        if (accept && r8 < ns && row8 < n) {      // the next step starts where this one ended; its stage 0 is this one's last (FSAL)
            T.sY0[m8 * RK_MAX_NS + r8] = sYin[m8 * 8 + r8];
            T.sK[m8 * RK_MAX_NS + r8] = sK[((L.S_total - 1) * NLBAC_MLP_TILE + m8) * RK_MAX_NS + r8];
        }
        if (tid < NLBAC_MLP_TILE) T.sH[tid] = (float)sCtl[C_H];
    }
    if (accept && X.keep) {      // the slot is taken; the next step — of this interval or of the next — needs one more
        const bool need = !done || k + 1 < X.H;
        if (need && slot + 1 >= P.slots) ret = done ? 3 : 2;
        if (tid == 0) sInt[TI_SLOT] = slot + 1;
    }
    __syncthreads();
    return ret;
}

// backward of a tile's kept steps (node_rr_bwd_body with TILE), before the stages of interval k's step sj (slot =
// first + sj; of nacc): the step size; at the interval's LAST step (the first one walked) the actions, du = 0 and, from
// d = dout[k+1] (+ the dy0 of interval k+1 in sDY0 when kk > 0), the interpolant's backward: dy0, dy1 (sDYup), dK_0..6
// (rk_bwd_tile_constants' ip branch); at an earlier step the hand-over of the chained launches (back_idx > 0): dYup =
// the later step's dy0, dK_6 = its dK_0 (FSAL), every other dK and dy0 zero; du goes on accumulating.  No barrier inside.
template <int NTHR>
__device__ __forceinline__ void rk_tile_bwd_begin(const NodeRkBwdLaunch& L, const NodeTileBwd& X, const RkBwdTile& T,
                                                  int row0, int k, int kk, bool last, float h, float x, int tid) {
    static_assert(NTHR == NLBAC_MLP_TILE * RK_MAX_NS, "one (row, component) per thread");
    const int n = L.n, ns = L.n_s, nu = L.n_u;
    const int m = tid >> 3, c = tid & 7;
    const bool ok = row0 + m < n && c < ns;
    if (tid < NLBAC_MLP_TILE) T.sH[tid] = h;
    if (last) {
        float vu = 0.f;
        if (tid < NLBAC_MLP_TILE * RK_MAX_NU) {
            const int mu = tid >> 2, cu = tid & 3;
            vu = L.u[(long)k * n * nu + (long)min(row0 + mu, n - 1) * nu + min(cu, nu - 1)];
        }
        float d = X.dout[(long)(k + 1) * n * ns + (long)min(row0 + m, n - 1) * ns + min(c, ns - 1)];
        if (kk > 0) d = d + T.sDY0[tid];
        float d0v, d1v, dk[7];
        dopri_interp_grad(d, h, x, d0v, d1v, dk);
        if (tid < NLBAC_MLP_TILE * RK_MAX_NU) {
            const int mu = tid >> 2, cu = tid & 3;
            T.sU[tid] = (row0 + mu < n && cu < nu) ? vu : 0.f;
            T.sDU[tid] = 0.f;
        }
        T.sDY0[tid] = ok ? d0v : 0.f;
        T.sDYup[tid] = ok ? d1v : 0.f;
#pragma unroll
        for (int j = 0; j < 7; ++j) T.sDK[j * NLBAC_MLP_TILE * RK_MAX_NS + tid] = ok ? dk[j] : 0.f;
    } else {
        const float dy = T.sDY0[tid], dk0 = T.sDK[tid];
        T.sDYup[tid] = ok ? dy : 0.f;
        T.sDY0[tid] = 0.f;
#pragma unroll
        for (int j = 0; j < 7; ++j) T.sDK[j * NLBAC_MLP_TILE * RK_MAX_NS + tid] = (j == 6 && ok) ? dk0 : 0.f;
    }
}

// (DENSE) before the stages of the step in `slot` (the tile's steps last to first): what the outputs that fell in the
// step send to its y0 / y1 / K — the sum of dopri_interp_grad over them in increasing j, from 0.f
// (dopri_dense_bwd_kernel's order; [jb, je) are the outputs ov_slot names this slot, je the ones not yet taken, both
// inside [0, n_out] whatever the arrays hold) — and the hand-over of the chained launches as ADDS onto it
// (nlbac_dopri_dense_carry): dy1 = g1 + the later step's dy0, dK_6 = gk_6 + its dK_0; the step's own backward adds
// onto dy0 = g0 and dK = gk.  dout [n_out][n][n_s]: the gradients of the outputs 1 .. n_out.  No barrier inside.
template <int NTHR>
__device__ __forceinline__ void rk_tile_dense_bwd_begin(const NodeRkBwdLaunch& L, const NodeTileBwd& X,
                                                        const NodeTileDenseBwd& D, const RkBwdTile& T, int row0, int slot,
                                                        bool last, float h, int& je, int tid) {
    static_assert(NTHR == NLBAC_MLP_TILE * RK_MAX_NS, "one (row, component) per thread");
    const int n = L.n, ns = L.n_s, nu = L.n_u;
    const int m = tid >> 3, c = tid & 7;
    const bool ok = row0 + m < n && c < ns;
    const long tb = (long)(row0 / NLBAC_MLP_TILE) * D.n_out;
    if (tid < NLBAC_MLP_TILE) T.sH[tid] = h;
    int jb = je;
    while (jb > 0 && D.ov_slot[tb + jb - 1] >= slot) --jb;      // (uniform; at most n_out looks over the whole walk)
    float g0 = 0.f, g1 = 0.f, gk[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int j = jb; j < je; ++j) {
        const float x = D.ov_x[tb + j];
        const float d = X.dout[(long)j * n * ns + (long)min(row0 + m, n - 1) * ns + min(c, ns - 1)];
        float d0v, d1v, dk[7];
        dopri_interp_grad(d, h, x, d0v, d1v, dk);
        g0 += d0v; g1 += d1v;
#pragma unroll
        for (int s = 0; s < 7; ++s) gk[s] += dk[s];
    }
    je = jb;
    if (last) {
        if (tid < NLBAC_MLP_TILE * RK_MAX_NU) {
            const int mu = tid >> 2, cu = tid & 3;
            const float vu = L.u[(long)min(row0 + mu, n - 1) * nu + min(cu, nu - 1)];
            T.sU[tid] = (row0 + mu < n && cu < nu) ? vu : 0.f;
            T.sDU[tid] = 0.f;
        }
        T.sDYup[tid] = ok ? g1 : 0.f;
    } else {
        const float dy = T.sDY0[tid], dk0 = T.sDK[tid];
        T.sDYup[tid] = ok ? g1 + dy : 0.f;
        gk[6] = gk[6] + dk0;
    }
    T.sDY0[tid] = ok ? g0 : 0.f;
#pragma unroll
    for (int j = 0; j < 7; ++j) T.sDK[j * NLBAC_MLP_TILE * RK_MAX_NS + tid] = ok ? gk[j] : 0.f;
}

// behind the stages of interval k's step sj: dK of the evaluated stages to global when the weight gradients want it (an
// FSAL step's stage 0 belongs to the step before: its row stays zero); behind the interval's first step du[k], behind
// interval 0's dx0 = dout[0] + dy0 (DENSE: dx0 = slot 0's dy0; dout holds no gradient of y0).  No barrier inside.
template <int NTHR, bool DENSE = false>
__device__ __forceinline__ void rk_tile_bwd_end(const NodeRkBwdLaunch& L, const NodeTileBwd& X, const NodeTilePlace& P,
                                                const RkBwdWhere& w, const RkBwdTile& T, int row0, int k, int sj, int tid) {
    const int n = L.n, ns = L.n_s, nu = L.n_u;
    if (w.gdK)
        for (int idx = tid; idx < L.st_hi * NLBAC_MLP_TILE * ns; idx += NTHR) {
            const int j = idx / (NLBAC_MLP_TILE * ns), rem = idx - j * NLBAC_MLP_TILE * ns;
            const int m = rem / ns, c = rem - m * ns, row = row0 + m;
            if (row < n && j >= w.st_lo)
                w.gdK[((long)j * P.kn + P.krow0 + m) * ns + c] = T.sDK[(j * NLBAC_MLP_TILE + m) * RK_MAX_NS + c];
        }
    if (sj != 0) return;
    for (int idx = tid; idx < NLBAC_MLP_TILE * nu; idx += NTHR) {
        const int m = idx / nu, c = idx - m * nu, row = row0 + m;
        if (row < n) L.du[(long)k * n * nu + (long)row * nu + c] = T.sDU[m * RK_MAX_NU + c];
    }
    if (k == 0)
        for (int idx = tid; idx < NLBAC_MLP_TILE * ns; idx += NTHR) {
            const int m = idx / ns, c = idx - m * ns, row = row0 + m;
            if constexpr (DENSE) { if (row < n) X.dx0[(long)row * ns + c] = T.sDY0[m * RK_MAX_NS + c]; }
            else if (row < n) X.dx0[(long)row * ns + c] = X.dout[(long)row * ns + c] + T.sDY0[m * RK_MAX_NS + c];
        }
}
