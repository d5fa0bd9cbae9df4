// One-launch fixed-grid rollout of the single-net NODE  dx/dt = net([x | c])  (SimulatedCars, the Quadrotor-like task's
// normalised form):  H intervals of euler / rk4 (3/8 rule) with new carried columns per interval, forward and backward,
// on the register-resident layer chains.
//
// In the one-step kernels a wave owns its 16 rows for the whole launch and the stage loop has no barrier, so a
// fixed-grid horizon is the same wave carrying the same rows through H x S stages: no grid-wide wait, no atomics, and
// no barrier inside the interval loop either (the interval's result is written, and kept in LDS as the next interval's
// y0, by the wave that owns the rows).  What the one-step launches pay H times is paid once per tile: the weight
// stream's prime, layer 0's LDS fragments, the output layer's registers, the normaliser's constants.  Each interval is
// the one-step kernel's step through the same code (concat_rr_body.h with TRAJ), so the results are those of H
// one-step launches bit for bit.  dopri5 is not served: its step-size control is batch-wide (an RMS norm over all
// rows), which would need grid-wide waits.
//
// Reference: the chained odeint calls of C/sac_cbf_clf/sac_cbf_clf.py:437-458 (odeint(model, [x_k | u_k | t_k],
// [0, dt])[-1], one interval per call).
//
// nlbac_concat_rk_grid_*: the solution on a whole time grid, torchdiffeq's fixed-grid rule (one RK step per grid
// interval): the same kernels with a step size per interval and one set of carried columns for all of them (GRID in
// concat_rr_body.h), the carried columns' gradient summed over the intervals inside the launch.
//
// nlbac_concat_rk_subgrid_*: the same grid under step_size — the launch's intervals are the N fine intervals, its
// outputs the T - 1 points read off them by linear interpolation (SUB in concat_rr_body.h, NlbacSubGrid in common.h); the
// backward takes the output points' gradients in between the fine intervals.
//
// nlbac_concat_rk_hold_*: a rollout under step_size — H control intervals of m fine steps each, the carried columns held
// through a control interval (HOLD in concat_rr_body.h): the grid kernels over the H m fine intervals with the step
// schedule hs [m] repeated, the trajectory kernels' change of carried columns and outputs behind every m-th of them.
#undef RR_TIMING          // (the ablation stamps belong to the one-step kernels)
#include "concat_rr_body.h"

// waves per workgroup: a rollout is one problem (rpp == n), for which the one-step launcher's rule (crr_waves) gives four
#define CTRAJ_NW 4

struct ConcatRkTrajFwdLaunch {
    ConcatRkLaunch L;
    int H;
};

struct ConcatRkTrajBwdLaunch {
    ConcatRkBwdLaunch L;
    ConcatRkTrajBwd X;
};

struct ConcatRkGridFwdLaunch {
    ConcatRkLaunch L;
    int H;
    const float* hs;                  // [H] the intervals' step sizes (device)
};

struct ConcatRkGridBwdLaunch {
    ConcatRkBwdLaunch L;
    ConcatRkTrajBwd X;
    const float* hs;
};

struct ConcatRkSubgridFwdLaunch {
    ConcatRkLaunch L;
    int H;                            // the N fine intervals
    const float* hs;
    NlbacSubGrid sub;
};

struct ConcatRkSubgridBwdLaunch {
    ConcatRkBwdLaunch L;
    ConcatRkTrajBwd X;
    const float* hs;
    NlbacSubGrid sub;
};

struct ConcatRkHoldFwdLaunch {
    ConcatRkLaunch L;
    int H;                            // the N = (control intervals) * m fine intervals
    const float* hs;                  // [m] the fine steps of a control interval (device)
    int m;
};

struct ConcatRkHoldBwdLaunch {
    ConcatRkBwdLaunch L;
    ConcatRkTrajBwd X;                // (H: the N fine intervals; dout [N/m + 1][n][n_s])
    const float* hs;
    int m;
};

template <int NB, int R, int BITS, int NW>
__global__ __launch_bounds__(64 * NW) void concat_hold_fwd_kernel(const ConcatRkHoldFwdLaunch A) {
    concat_rr_fwd_body<NB, R, BITS, NW, true, true, false, true>(A.L, A.H, A.hs, nullptr, A.m);
}

// (waves per SIMD as concat_traj_bwd_kernel below)
template <int NB, int R, int BITS, int NW>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu((BITS == 1 && NB < 8) ? 3 : 2)))
void concat_hold_bwd_kernel(const ConcatRkHoldBwdLaunch A) {
    concat_rr_bwd_body<NB, R, BITS, NW, true, true, false, true>(A.L, &A.X, A.hs, nullptr, A.m);
}

template <int NB, int R, int BITS, int NW>
__global__ __launch_bounds__(64 * NW) void concat_subgrid_fwd_kernel(const ConcatRkSubgridFwdLaunch A) {
    concat_rr_fwd_body<NB, R, BITS, NW, true, true, true>(A.L, A.H, A.hs, &A.sub);
}

// (waves per SIMD as concat_traj_bwd_kernel below)
template <int NB, int R, int BITS, int NW>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu((BITS == 1 && NB < 8) ? 3 : 2)))
void concat_subgrid_bwd_kernel(const ConcatRkSubgridBwdLaunch A) {
    concat_rr_bwd_body<NB, R, BITS, NW, true, true, true>(A.L, &A.X, A.hs, &A.sub);
}

template <int NB, int R, int BITS, int NW>
__global__ __launch_bounds__(64 * NW) void concat_grid_fwd_kernel(const ConcatRkGridFwdLaunch A) {
    concat_rr_fwd_body<NB, R, BITS, NW, true, true>(A.L, A.H, A.hs);
}

// (waves per SIMD as concat_traj_bwd_kernel below)
template <int NB, int R, int BITS, int NW>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu((BITS == 1 && NB < 8) ? 3 : 2)))
void concat_grid_bwd_kernel(const ConcatRkGridBwdLaunch A) {
    concat_rr_bwd_body<NB, R, BITS, NW, true, true>(A.L, &A.X, A.hs);
}

template <int NB, int R, int BITS, int NW>
__global__ __launch_bounds__(64 * NW) void concat_traj_fwd_kernel(const ConcatRkTrajFwdLaunch A) {
    concat_rr_fwd_body<NB, R, BITS, NW, true>(A.L, A.H);
}

// (the mask-word instances of the two narrower shapes keep the one-step kernels' three waves per SIMD: the interval
// loop's bookkeeping would otherwise push the allocator a few registers past 168)
template <int NB, int R, int BITS, int NW>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu((BITS == 1 && NB < 8) ? 3 : 2)))
void concat_traj_bwd_kernel(const ConcatRkTrajBwdLaunch A) {
    concat_rr_bwd_body<NB, R, BITS, NW, true>(A.L, &A.X);
}

extern "C" int nlbac_concat_rk_traj_ok(const nlbac_mlp* net) {
    return (net && nlbac_concat_rr_eligible(net) && net->in_dim > net->out_dim && net->in_dim - net->out_dim <= CK_NC) ? 1 : 0;
}

static int ctraj_check(const nlbac_mlp* net, int n, int H, int n_stages, const float* beta, const float* c_out, float h,
                       int acts_bits, const char* who) {
    NLBAC_REQUIRE(net && beta && c_out, "%s: null pointer", who);
    NLBAC_REQUIRE(nlbac_concat_rk_traj_ok(net), "%s: this net does not run on the trajectory kernels (nlbac_concat_rk_traj_ok)", who);
    NLBAC_REQUIRE(n >= 1 && H >= 1 && (long)H * n_stages * n < (1L << 31), "%s: bad rows / intervals", who);
    NLBAC_REQUIRE(n_stages >= 1 && n_stages <= CK_MAX_STAGES, "%s: bad stage count", who);
    NLBAC_REQUIRE(h > 0.f, "%s: the step must be positive", who);
    NLBAC_REQUIRE(acts_bits == 0 || acts_bits == 1, "%s: acts_bits is 0 or 1", who);
    return 0;
}

// a sub-stepped time-grid launch carries the output points' offsets and weights as well
template <typename Launch>
constexpr bool ctraj_on_subgrid = std::is_same<Launch, ConcatRkSubgridFwdLaunch>::value || std::is_same<Launch, ConcatRkSubgridBwdLaunch>::value;

// a held-control launch carries the m fine steps of a control interval; its intervals are the fine ones
template <typename Launch>
constexpr bool ctraj_on_hold = std::is_same<Launch, ConcatRkHoldFwdLaunch>::value || std::is_same<Launch, ConcatRkHoldBwdLaunch>::value;

// a time-grid launch carries a step size per interval
template <typename Launch>
constexpr bool ctraj_on_grid = std::is_same<Launch, ConcatRkGridFwdLaunch>::value ||
                               std::is_same<Launch, ConcatRkGridBwdLaunch>::value || ctraj_on_subgrid<Launch> ||
                               ctraj_on_hold<Launch>;

// The forward launch of `who` (an entry point below) over H intervals: the instances of its kernel template in `table`
// (chosen as the one-step launcher chooses, concat_rr_body.h, so that the sums are the same), its step — h for every
// interval, or (time grid) hs [H] on the device for the kernel with hs_host [H] beside it for the checks here — and
// what the interval's one-step launch takes.  (Sub-stepped time grid) sg: the output points; out is [T-1][n][n_s].
// (Held controls) H: the fine intervals, a multiple of m (nlbac_hold_intervals); hs / hs_host [m]; out is [H/m][n][n_s].
template <typename Launch>
static int ctraj_fwd(const ConcatRrTable<Launch>& table, const char* who, float h, const float* hs, const float* hs_host,
                     const nlbac_mlp* net, const float* x0, const float* c, int n, int H, int n_stages, const float* beta,
                     const float* c_out, float* out, float* Xin, float* acts, long acts_ls, int acts_bits,
                     const float* norm, nlbac_stream_t s, const NlbacSubGridArgs* sg = nullptr, int m = 1) {
    constexpr bool grid = ctraj_on_grid<Launch>;
    const int n_hs = ctraj_on_hold<Launch> ? m : H;      // the step sizes the launch carries
    if (ctraj_check(net, n, H, n_stages, beta, c_out, grid ? 1.f : h, acts_bits, who)) return -1;
    if (grid && nlbac_grid_steps_check(hs, hs_host, n_hs, who)) return -1;
    if (ctraj_on_subgrid<Launch> && nlbac_subgrid_check(sg, H, who)) return -1;
    Launch A;
    memset(&A, 0, sizeof(A));
    ConcatRkLaunch& L = A.L;
    NLBAC_REQUIRE(x0 && c && out, "%s: null pointer", who);
    NLBAC_REQUIRE(acts || acts_bits == 0, "%s: acts_bits without acts", who);
    NLBAC_REQUIRE(!Xin || (acts && acts_bits == 0), "%s: Xin goes with the activation rows", who);
    L.net = *net;
    L.y0 = x0; L.c = c;
    L.n = n; L.rpp = n; L.n_s = net->out_dim; L.n_c = net->in_dim - net->out_dim;
    L.stage_begin = 0; L.stage_end = n_stages; L.S_total = n_stages;
    nlbac_tableau_copy(L.beta, L.c_out, L.n_out, n_stages, beta, c_out);
    L.h_val[0] = grid ? hs_host[0] : h;
    L.acts = acts; L.acts_ls = acts_ls; L.acts_bits = acts_bits;
    L.out = out;
    L.norm = norm; L.Xn = Xin;
    L.norm_mode = -1;
    A.H = H;
    if constexpr (grid) A.hs = hs;
    if constexpr (ctraj_on_subgrid<Launch>) { A.sub.ofs = sg->ofs; A.sub.theta = sg->theta; }
    if constexpr (ctraj_on_hold<Launch>) A.m = m;
    crr_start(table, CTRAJ_NW, A, net->hid, n, acts_bits, crr_fwd_lds, (hipStream_t)s);
    NLBAC_CHECK_LAUNCH(who);
    return 0;
}

// The backward launch of `who`: as ctraj_fwd.
template <typename Launch>
static int ctraj_bwd(const ConcatRrTable<Launch>& table, const char* who, float h, const float* hs, const float* hs_host,
                     const nlbac_mlp* net, int n, int H, int n_stages, const float* beta, const float* c_out,
                     const float* acts, long acts_ls, int acts_bits, const float* norm, const float* dout, float* dx0,
                     float* dc, float* dK, float* dz, nlbac_stream_t s, const NlbacSubGridArgs* sg = nullptr, int m = 1) {
    constexpr bool grid = ctraj_on_grid<Launch>;
    const int n_hs = ctraj_on_hold<Launch> ? m : H;
    if (ctraj_check(net, n, H, n_stages, beta, c_out, grid ? 1.f : h, acts_bits, who)) return -1;
    if (grid && nlbac_grid_steps_check(hs, hs_host, n_hs, who)) return -1;
    if (ctraj_on_subgrid<Launch> && nlbac_subgrid_check(sg, H, who)) return -1;
    Launch A;
    memset(&A, 0, sizeof(A));
    ConcatRkBwdLaunch& L = A.L;
    NLBAC_REQUIRE(!(acts_bits == 1 && dz), "%s: weight gradients need the activation rows, not mask words", who);
    NLBAC_REQUIRE(acts && dout && dx0 && dc, "%s: null pointer", who);
    NLBAC_REQUIRE((dz == nullptr) == (dK == nullptr), "%s: dz and dK go together", who);
    L.net = *net;
    L.acts = acts; L.acts_ls = acts_ls; L.acts_bits = acts_bits;
    L.dz = dz; L.dyn = dK;
    L.dc = dc;
    L.n = n; L.rpp = n; L.n_s = net->out_dim; L.n_c = net->in_dim - net->out_dim;
    L.S_total = n_stages; L.st_lo = 0; L.st_hi = n_stages; L.dx_stage0 = 1;
    nlbac_tableau_copy(L.beta, A.X.c_out, A.X.n_out, n_stages, beta, c_out);
    L.h_val[0] = grid ? hs_host[n_hs - 1] : h;
    L.norm = norm;
    A.X.H = H; A.X.dout = dout; A.X.dx0 = dx0;
    if constexpr (grid) A.hs = hs;
    if constexpr (ctraj_on_subgrid<Launch>) { A.sub.ofs = sg->ofs; A.sub.theta = sg->theta; }
    if constexpr (ctraj_on_hold<Launch>) A.m = m;
    crr_start(table, CTRAJ_NW, A, net->hid, n, acts_bits, crr_bwd_lds, (hipStream_t)s);
    NLBAC_CHECK_LAUNCH(who);
    return 0;
}

extern "C" int nlbac_concat_rk_traj_fwd(const nlbac_mlp* net, const float* x0, const float* c, int n, int H,
                                        int n_stages, const float* beta, const float* c_out, float h, float* out,
                                        float* Xin, float* acts, long acts_ls, int acts_bits, const float* norm,
                                        nlbac_stream_t s) {
    static const ConcatRrTable<ConcatRkTrajFwdLaunch> table = CONCAT_RR_TABLE(concat_traj_fwd_kernel, CTRAJ_NW);
    return ctraj_fwd(table, "nlbac_concat_rk_traj_fwd", h, nullptr, nullptr, net, x0, c, n, H, n_stages, beta, c_out, out,
                     Xin, acts, acts_ls, acts_bits, norm, s);
}

extern "C" int nlbac_concat_rk_traj_bwd(const nlbac_mlp* net, int n, int H, int n_stages, const float* beta,
                                        const float* c_out, float h, const float* acts, long acts_ls, int acts_bits,
                                        const float* norm, const float* dout, float* dx0, float* dc, float* dK,
                                        float* dz, nlbac_stream_t s) {
    static const ConcatRrTable<ConcatRkTrajBwdLaunch> table = CONCAT_RR_TABLE(concat_traj_bwd_kernel, CTRAJ_NW);
    return ctraj_bwd(table, "nlbac_concat_rk_traj_bwd", h, nullptr, nullptr, net, n, H, n_stages, beta, c_out, acts,
                     acts_ls, acts_bits, norm, dout, dx0, dc, dK, dz, s);
}

// ---- the solution on a time grid: a step size per interval (hs [H] on the device for the kernel, hs_host [H] beside it
//      for the launcher's checks, nlbac_grid_steps_check), one set of carried columns c [n][n_c], dc [n][n_c] summed over
//      the intervals
extern "C" int nlbac_concat_rk_grid_fwd(const nlbac_mlp* net, const float* x0, const float* c, int n, int H,
                                        int n_stages, const float* beta, const float* c_out, const float* hs,
                                        const float* hs_host, float* out, float* Xin, float* acts, long acts_ls,
                                        int acts_bits, const float* norm, nlbac_stream_t s) {
    static const ConcatRrTable<ConcatRkGridFwdLaunch> table = CONCAT_RR_TABLE(concat_grid_fwd_kernel, CTRAJ_NW);
    return ctraj_fwd(table, "nlbac_concat_rk_grid_fwd", 0.f, hs, hs_host, net, x0, c, n, H, n_stages, beta, c_out, out,
                     Xin, acts, acts_ls, acts_bits, norm, s);
}

extern "C" int nlbac_concat_rk_grid_bwd(const nlbac_mlp* net, int n, int H, int n_stages, const float* beta,
                                        const float* c_out, const float* hs, const float* hs_host, const float* acts,
                                        long acts_ls, int acts_bits, const float* norm, const float* dout, float* dx0,
                                        float* dc, float* dK, float* dz, nlbac_stream_t s) {
    static const ConcatRrTable<ConcatRkGridBwdLaunch> table = CONCAT_RR_TABLE(concat_grid_bwd_kernel, CTRAJ_NW);
    return ctraj_bwd(table, "nlbac_concat_rk_grid_bwd", 0.f, hs, hs_host, net, n, H, n_stages, beta, c_out, acts, acts_ls,
                     acts_bits, norm, dout, dx0, dc, dK, dz, s);
}

// ---- the same grid under step_size: H = N fine intervals with steps hs / hs_host [N]; the T - 1 output points 1 .. T-1
//      are read off them — interval i holds the outputs ofs[i] <= j < ofs[i+1], weights theta [T-1] (device arrays for
//      the kernel, ofs_host / theta_host beside them for the checks here, nlbac_subgrid_check).  out [T-1][n][n_s],
//      dout [T][n][n_s]; Xin / acts / dK / dz per fine stage, [N * n_stages][n][..]
extern "C" int nlbac_concat_rk_subgrid_fwd(const nlbac_mlp* net, const float* x0, const float* c, int n, int H,
                                           int n_stages, const float* beta, const float* c_out, const float* hs,
                                           const float* hs_host, const int* ofs, const int* ofs_host, const float* theta,
                                           const float* theta_host, int T, float* out, float* Xin, float* acts,
                                           long acts_ls, int acts_bits, const float* norm, nlbac_stream_t s) {
    static const ConcatRrTable<ConcatRkSubgridFwdLaunch> table = CONCAT_RR_TABLE(concat_subgrid_fwd_kernel, CTRAJ_NW);
    const NlbacSubGridArgs sg = {ofs, ofs_host, theta, theta_host, T};
    return ctraj_fwd(table, "nlbac_concat_rk_subgrid_fwd", 0.f, hs, hs_host, net, x0, c, n, H, n_stages, beta, c_out, out,
                     Xin, acts, acts_ls, acts_bits, norm, s, &sg);
}

extern "C" int nlbac_concat_rk_subgrid_bwd(const nlbac_mlp* net, int n, int H, int n_stages, const float* beta,
                                           const float* c_out, const float* hs, const float* hs_host, const int* ofs,
                                           const int* ofs_host, const float* theta, const float* theta_host, int T,
                                           const float* acts, long acts_ls, int acts_bits, const float* norm,
                                           const float* dout, float* dx0, float* dc, float* dK, float* dz,
                                           nlbac_stream_t s) {
    static const ConcatRrTable<ConcatRkSubgridBwdLaunch> table = CONCAT_RR_TABLE(concat_subgrid_bwd_kernel, CTRAJ_NW);
    const NlbacSubGridArgs sg = {ofs, ofs_host, theta, theta_host, T};
    return ctraj_bwd(table, "nlbac_concat_rk_subgrid_bwd", 0.f, hs, hs_host, net, n, H, n_stages, beta, c_out, acts,
                     acts_ls, acts_bits, norm, dout, dx0, dc, dK, dz, s, &sg);
}

// ---- a rollout under step_size: H control intervals of m fine steps each, steps hs / hs_host [m] (the same schedule in
//      every control interval; device array for the kernel, host copy for the checks here), the carried columns
//      c [H][n][n_c] held through their control interval.  out [H][n][n_s], dout [H+1][n][n_s], dc [H][n][n_c]; Xin /
//      acts / dK / dz per fine stage, [H * m * n_stages][n][..]
extern "C" int nlbac_concat_rk_hold_fwd(const nlbac_mlp* net, const float* x0, const float* c, int n, int H, int n_stages,
                                        const float* beta, const float* c_out, const float* hs, const float* hs_host,
                                        int m, float* out, float* Xin, float* acts, long acts_ls, int acts_bits,
                                        const float* norm, nlbac_stream_t s) {
    static const ConcatRrTable<ConcatRkHoldFwdLaunch> table = CONCAT_RR_TABLE(concat_hold_fwd_kernel, CTRAJ_NW);
    int N = 0;
    if (nlbac_hold_intervals(H, m, n_stages, n, "nlbac_concat_rk_hold_fwd", &N)) return -1;
    return ctraj_fwd(table, "nlbac_concat_rk_hold_fwd", 0.f, hs, hs_host, net, x0, c, n, N, n_stages, beta, c_out, out,
                     Xin, acts, acts_ls, acts_bits, norm, s, nullptr, m);
}

extern "C" int nlbac_concat_rk_hold_bwd(const nlbac_mlp* net, int n, int H, int n_stages, const float* beta,
                                        const float* c_out, const float* hs, const float* hs_host, int m,
                                        const float* acts, long acts_ls, int acts_bits, const float* norm,
                                        const float* dout, float* dx0, float* dc, float* dK, float* dz,
                                        nlbac_stream_t s) {
    static const ConcatRrTable<ConcatRkHoldBwdLaunch> table = CONCAT_RR_TABLE(concat_hold_bwd_kernel, CTRAJ_NW);
    int N = 0;
    if (nlbac_hold_intervals(H, m, n_stages, n, "nlbac_concat_rk_hold_bwd", &N)) return -1;
    return ctraj_bwd(table, "nlbac_concat_rk_hold_bwd", 0.f, hs, hs_host, net, n, N, n_stages, beta, c_out, acts,
                     acts_ls, acts_bits, norm, dout, dx0, dc, dK, dz, s, nullptr, m);
}
