// One-launch fixed-grid rollout of the control-affine NODE  dx/dt = f(x) + g(x) u:  H intervals of euler / rk4 (3/8
// rule) with a new action per interval, forward and backward, on the register-resident layer chains.
//
// Under a fixed grid every row of a trajectory depends on its own row only, so a 32-row tile runs all H intervals one
// after the other with no workgroup ever waiting for another (no grid-wide synchronisation, no atomics on memory other
// workgroups see).  What the one-step launches pay H times is paid once per tile: the weight stream's prime, layer 0's
// LDS fragments, the output layer's registers; the interval's state stays in the tile's LDS from one interval to the
// next.  Each interval is the one-step kernel's step, through the same code (node_rr_body.h with TRAJ, the stage algebra
// and RK combine of node_rk_shared.h), so the results are those of H one-step launches bit for bit.  dopri5 is not
// served: its step-size control is batch-wide (an RMS norm over all rows), which would need grid-wide waits.
//
// Reference: the chained odeint calls of C/sac_cbf_clf/sac_cbf_clf.py:437-458 and P/sac_cbf_clf/sac_cbf_clf.py:459-534
// (odeint(model, [x_k | u_k], [0, dt])[-1], one interval per call).
//
// nlbac_node_rk_grid_*: the solution on a whole time grid, torchdiffeq's fixed-grid rule (one RK step per grid
// interval): the same kernels with a step size per interval and one set of actions for all of them (GRID in
// node_rr_body.h), the actions' gradient summed over the intervals inside the launch.
//
// nlbac_node_rk_subgrid_*: the same grid under step_size — the launch's intervals are the N fine intervals, its outputs
// the T - 1 points read off them by linear interpolation (SUB in node_rr_body.h, NlbacSubGrid in common.h); the backward
// takes the output points' gradients in between the fine intervals.  K / Y / G, mask words and activation rows per fine
// stage, as the grid kernels keep them per interval.
//
// nlbac_node_rk_hold_*: a rollout under step_size — H control intervals of m fine steps each, the actions held through a
// control interval (HOLD in node_rr_body.h): the grid kernels over the H m fine intervals with the step schedule hs [m]
// repeated, the trajectory kernels' change of actions and outputs behind every m-th of them.
#undef RR_TIMING          // (the ablation stamps belong to the one-step kernels)
#include "node_rr_body.h"

struct NodeRkTrajFwdLaunch {
    NodeRkLaunch L;
    int H;
};

struct NodeRkTrajBwdLaunch {
    NodeRkBwdLaunch L;
    NodeRkTrajBwd X;
};

struct NodeRkGridFwdLaunch {
    NodeRkLaunch L;
    int H;
    const float* hs;                  // [H] the intervals' step sizes (device)
};

struct NodeRkGridBwdLaunch {
    NodeRkBwdLaunch L;
    NodeRkTrajBwd X;
    const float* hs;
};

struct NodeRkSubgridFwdLaunch {
    NodeRkLaunch L;
    int H;                            // the N fine intervals
    const float* hs;
    NlbacSubGrid sub;
};

struct NodeRkSubgridBwdLaunch {
    NodeRkBwdLaunch L;
    NodeRkTrajBwd X;
    const float* hs;
    NlbacSubGrid sub;
};

struct NodeRkHoldFwdLaunch {
    NodeRkLaunch L;
    int H;                            // the N = (control intervals) * m fine intervals
    const float* hs;                  // [m] the fine steps of a control interval (device)
    int m;
};

struct NodeRkHoldBwdLaunch {
    NodeRkBwdLaunch L;
    NodeRkTrajBwd X;                  // (H: the N fine intervals; dout [N/m + 1][n][n_s])
    const float* hs;
    int m;
};

template <int NB, int R, int BITS, int SPLIT>
__global__ __launch_bounds__(256) void node_hold_fwd_kernel(const NodeRkHoldFwdLaunch A) {
    node_rr_fwd_body<NB, R, BITS, SPLIT, true, true, false, true>(A.L, A.H, A.hs, nullptr, A.m);
}

template <int NB, int R, int BITS, int SPLIT>
__global__ __launch_bounds__(256) void node_hold_bwd_kernel(const NodeRkHoldBwdLaunch A) {
    node_rr_bwd_body<NB, R, BITS, SPLIT, true, true, false, true>(A.L, &A.X, A.hs, nullptr, A.m);
}

template <int NB, int R, int BITS, int SPLIT>
__global__ __launch_bounds__(256) void node_subgrid_fwd_kernel(const NodeRkSubgridFwdLaunch A) {
    node_rr_fwd_body<NB, R, BITS, SPLIT, true, true, true>(A.L, A.H, A.hs, &A.sub);
}

template <int NB, int R, int BITS, int SPLIT>
__global__ __launch_bounds__(256) void node_subgrid_bwd_kernel(const NodeRkSubgridBwdLaunch A) {
    node_rr_bwd_body<NB, R, BITS, SPLIT, true, true, true>(A.L, &A.X, A.hs, &A.sub);
}

template <int NB, int R, int BITS, int SPLIT>
__global__ __launch_bounds__(256) void node_grid_fwd_kernel(const NodeRkGridFwdLaunch A) {
    node_rr_fwd_body<NB, R, BITS, SPLIT, true, true>(A.L, A.H, A.hs);
}

template <int NB, int R, int BITS, int SPLIT>
__global__ __launch_bounds__(256) void node_grid_bwd_kernel(const NodeRkGridBwdLaunch A) {
    node_rr_bwd_body<NB, R, BITS, SPLIT, true, true>(A.L, &A.X, A.hs);
}

template <int NB, int R, int BITS, int SPLIT>
__global__ __launch_bounds__(256) void node_traj_fwd_kernel(const NodeRkTrajFwdLaunch A) {
    node_rr_fwd_body<NB, R, BITS, SPLIT, true>(A.L, A.H);
}

template <int NB, int R, int BITS, int SPLIT>
__global__ __launch_bounds__(256) void node_traj_bwd_kernel(const NodeRkTrajBwdLaunch A) {
    node_rr_bwd_body<NB, R, BITS, SPLIT, true>(A.L, &A.X);
}

extern "C" int nlbac_node_rk_traj_ok(const nlbac_mlp* f, const nlbac_mlp* g) {
    return (f && g && nlbac_node_rr_eligible(f, g)) ? 1 : 0;
}

static int traj_check(const nlbac_mlp* f, const nlbac_mlp* g, int n, int H, int n_stages, const float* beta,
                      const float* c_out, float h, int acts_bits, const char* who) {
    NLBAC_REQUIRE(f && g && beta && c_out, "%s: null pointer", who);
    NLBAC_REQUIRE(nlbac_node_rk_traj_ok(f, g), "%s: these nets do not run on the trajectory kernels (nlbac_node_rk_traj_ok)", who);
    NLBAC_REQUIRE(n >= 1 && H >= 1 && (long)H * n_stages * n < (1L << 31), "%s: bad rows / intervals", who);
    NLBAC_REQUIRE(n_stages >= 1 && n_stages <= RK_MAX_STAGES, "%s: bad stage count", who);
    NLBAC_REQUIRE(h > 0.f, "%s: the step must be positive", who);
    NLBAC_REQUIRE(acts_bits >= 0 && acts_bits <= 2, "%s: acts_bits is 0, 1 or 2", who);
    return 0;
}

// a sub-stepped time-grid launch carries the output points' offsets and weights as well
template <typename Launch>
constexpr bool traj_on_subgrid = std::is_same<Launch, NodeRkSubgridFwdLaunch>::value || std::is_same<Launch, NodeRkSubgridBwdLaunch>::value;

// a held-control launch carries the m fine steps of a control interval; its intervals are the fine ones
template <typename Launch>
constexpr bool traj_on_hold = std::is_same<Launch, NodeRkHoldFwdLaunch>::value || std::is_same<Launch, NodeRkHoldBwdLaunch>::value;

// a time-grid launch carries a step size per interval
template <typename Launch>
constexpr bool traj_on_grid = std::is_same<Launch, NodeRkGridFwdLaunch>::value ||
                              std::is_same<Launch, NodeRkGridBwdLaunch>::value || traj_on_subgrid<Launch> ||
                              traj_on_hold<Launch>;

// The forward launch of `who` (an entry point below) over H intervals: the instances of its kernel template in `table`
// (chosen as the one-step launcher chooses, node_rr_body.h, so that the sums are the same), its step — h for every
// interval, or (time grid) hs [H] on the device for the kernel with hs_host [H] beside it for the checks here — and
// what the interval's one-step launch takes.  (Sub-stepped time grid) sg: the output points; out is [T-1][n][n_s].
// (Held controls) H: the fine intervals, a multiple of m (nlbac_hold_intervals); hs / hs_host [m]; out is [H/m][n][n_s].
template <typename Launch>
static int traj_fwd(const NodeRrTable<Launch>& table, const char* who, float h, const float* hs, const float* hs_host,
                    const nlbac_mlp* f, const nlbac_mlp* g, const float* x0, const float* u, int n, int H, int n_stages,
                    const float* beta, const float* c_out, float* out, float* K, float* Y, float* G, float* acts_f,
                    long acts_f_ls, float* acts_g, long acts_g_ls, int acts_bits, nlbac_stream_t s,
                    const NlbacSubGridArgs* sg = nullptr, int m = 1) {
    constexpr bool grid = traj_on_grid<Launch>;
    const int n_hs = traj_on_hold<Launch> ? m : H;      // the step sizes the launch carries
    if (traj_check(f, g, n, H, n_stages, beta, c_out, grid ? 1.f : h, acts_bits, who)) return -1;
    if (grid && nlbac_grid_steps_check(hs, hs_host, n_hs, who)) return -1;
    if (traj_on_subgrid<Launch> && nlbac_subgrid_check(sg, H, who)) return -1;
    Launch A;
    memset(&A, 0, sizeof(A));
    NodeRkLaunch& L = A.L;
    NLBAC_REQUIRE(x0 && u && out && K && Y && G, "%s: null pointer", who);
    NLBAC_REQUIRE((acts_f == nullptr) == (acts_g == nullptr), "%s: acts_f and acts_g go together", who);
    NLBAC_REQUIRE(acts_f || acts_bits == 0, "%s: acts_bits without acts", who);
    L.net[0] = *f; L.net[1] = *g;
    L.y0 = x0; L.u = u;
    L.n = n; L.rpp = n; L.n_s = f->in_dim; L.n_u = g->out_dim / f->in_dim;
    L.stage_begin = 0; L.stage_end = n_stages; L.S_total = n_stages;
    nlbac_tableau_copy(L.beta, L.c_out, L.n_out, n_stages, beta, c_out);
    L.h_val[0] = grid ? hs_host[0] : h;
    L.K = K; L.Y = Y; L.G = G;
    L.acts[0] = acts_f; L.acts[1] = acts_g; L.acts_ls[0] = acts_f_ls; L.acts_ls[1] = acts_g_ls;
    L.acts_bits = acts_bits;
    L.out = out;
    L.norm_mode = -1;
    A.H = H;
    if constexpr (grid) {
        // the kernel rewrites the step slot sH with no barrier in front of the interval's first stage: that stage has
        // to be stage 0, the one whose input uses no step size
        NLBAC_REQUIRE(L.stage_begin == 0, "%s: a time-grid launch starts every interval at stage 0", who);
        A.hs = hs;
    }
    if constexpr (traj_on_subgrid<Launch>) { A.sub.ofs = sg->ofs; A.sub.theta = sg->theta; }
    if constexpr (traj_on_hold<Launch>) A.m = m;
    node_rr_fwd_start(table, A, f->hid, n, acts_bits, (hipStream_t)s);
    NLBAC_CHECK_LAUNCH(who);
    return 0;
}

// The backward launch of `who`: as traj_fwd.
template <typename Launch>
static int traj_bwd(const NodeRrTable<Launch>& table, const char* who, float h, const float* hs, const float* hs_host,
                    const nlbac_mlp* f, const nlbac_mlp* g, const float* u, int n, int H, int n_stages, const float* beta,
                    const float* c_out, const float* G, const float* acts_f, long acts_f_ls, const float* acts_g,
                    long acts_g_ls, int acts_bits, const float* dout, float* dx0, float* du, float* dK, float* dG,
                    float* dz_f, float* dz_g, nlbac_stream_t s, const NlbacSubGridArgs* sg = nullptr, int m = 1) {
    constexpr bool grid = traj_on_grid<Launch>;
    const int n_hs = traj_on_hold<Launch> ? m : H;
    if (traj_check(f, g, n, H, n_stages, beta, c_out, grid ? 1.f : h, acts_bits, who)) return -1;
    if (grid && nlbac_grid_steps_check(hs, hs_host, n_hs, who)) return -1;
    if (traj_on_subgrid<Launch> && nlbac_subgrid_check(sg, H, who)) return -1;
    Launch A;
    memset(&A, 0, sizeof(A));
    NodeRkBwdLaunch& L = A.L;
    NLBAC_REQUIRE(u && G && acts_f && acts_g && dout && dx0 && du, "%s: null pointer", who);
    NLBAC_REQUIRE((dz_f == nullptr) == (dz_g == nullptr) && (dz_f == nullptr) == (dG == nullptr) &&
                      (dz_f == nullptr) == (dK == nullptr), "%s: dz_f, dz_g, dG and dK go together", who);
    NLBAC_REQUIRE(!(acts_bits == 1 && dz_f), "%s: weight gradients need the activations, not bit masks", who);
    L.net[0] = *f; L.net[1] = *g;
    L.u = u; L.G = G;
    L.acts[0] = acts_f; L.acts[1] = acts_g; L.acts_ls[0] = acts_f_ls; L.acts_ls[1] = acts_g_ls;
    L.acts_bits = acts_bits;
    L.dz[0] = dz_f; L.dz[1] = dz_g; L.dG = dG; L.dK = dK;
    L.du = du;
    L.n = n; L.rpp = n; L.n_s = f->in_dim; L.n_u = g->out_dim / f->in_dim;
    L.S_total = n_stages; L.st_lo = 0; L.st_hi = n_stages; L.dx_stage0 = 1;
    nlbac_tableau_copy(L.beta, A.X.c_out, A.X.n_out, n_stages, beta, c_out);
    L.h_val[0] = grid ? hs_host[n_hs - 1] : h;
    A.X.H = H; A.X.dout = dout; A.X.dx0 = dx0;
    if constexpr (grid) A.hs = hs;
    if constexpr (traj_on_subgrid<Launch>) { A.sub.ofs = sg->ofs; A.sub.theta = sg->theta; }
    if constexpr (traj_on_hold<Launch>) A.m = m;
    node_rr_bwd_start(table, A, f->hid, n, acts_bits, (hipStream_t)s);
    NLBAC_CHECK_LAUNCH(who);
    return 0;
}

extern "C" int nlbac_node_rk_traj_fwd(const nlbac_mlp* f, const nlbac_mlp* g, const float* x0, const float* u, int n,
                                      int H, int n_stages, const float* beta, const float* c_out, float h, float* out,
                                      float* K, float* Y, float* G, float* acts_f, long acts_f_ls, float* acts_g,
                                      long acts_g_ls, int acts_bits, nlbac_stream_t s) {
    static const NodeRrTable<NodeRkTrajFwdLaunch> table = NODE_RR_FWD_TABLE(node_traj_fwd_kernel);
    return traj_fwd(table, "nlbac_node_rk_traj_fwd", h, nullptr, nullptr, f, g, x0, u, n, H, n_stages, beta, c_out, out,
                    K, Y, G, acts_f, acts_f_ls, acts_g, acts_g_ls, acts_bits, s);
}

extern "C" int nlbac_node_rk_traj_bwd(const nlbac_mlp* f, const nlbac_mlp* g, const float* u, int n, int H,
                                      int n_stages, const float* beta, const float* c_out, float h, const float* G,
                                      const float* acts_f, long acts_f_ls, const float* acts_g, long acts_g_ls,
                                      int acts_bits, const float* dout, float* dx0, float* du, float* dK, float* dG,
                                      float* dz_f, float* dz_g, nlbac_stream_t s) {
    static const NodeRrTable<NodeRkTrajBwdLaunch> table = NODE_RR_BWD_TABLE(node_traj_bwd_kernel);
    return traj_bwd(table, "nlbac_node_rk_traj_bwd", h, nullptr, nullptr, f, g, u, n, H, n_stages, beta, c_out, G,
                    acts_f, acts_f_ls, acts_g, acts_g_ls, acts_bits, dout, dx0, du, dK, dG, dz_f, dz_g, s);
}

// ---- the solution on a time grid: a step size per interval (hs [H] on the device for the kernel, hs_host [H] beside it
//      for the launcher's checks, nlbac_grid_steps_check), one set of actions u [n][n_u], du [n][n_u] summed over the
//      intervals
extern "C" int nlbac_node_rk_grid_fwd(const nlbac_mlp* f, const nlbac_mlp* g, const float* x0, const float* u, int n,
                                      int H, int n_stages, const float* beta, const float* c_out, const float* hs,
                                      const float* hs_host, float* out, float* K, float* Y, float* G, float* acts_f,
                                      long acts_f_ls, float* acts_g, long acts_g_ls, int acts_bits, nlbac_stream_t s) {
    static const NodeRrTable<NodeRkGridFwdLaunch> table = NODE_RR_FWD_TABLE(node_grid_fwd_kernel);
    return traj_fwd(table, "nlbac_node_rk_grid_fwd", 0.f, hs, hs_host, f, g, x0, u, n, H, n_stages, beta, c_out, out, K,
                    Y, G, acts_f, acts_f_ls, acts_g, acts_g_ls, acts_bits, s);
}

extern "C" int nlbac_node_rk_grid_bwd(const nlbac_mlp* f, const nlbac_mlp* g, const float* u, int n, int H,
                                      int n_stages, const float* beta, const float* c_out, const float* hs,
                                      const float* hs_host, const float* G, const float* acts_f, long acts_f_ls,
                                      const float* acts_g, long acts_g_ls, int acts_bits, const float* dout, float* dx0,
                                      float* du, float* dK, float* dG, float* dz_f, float* dz_g, nlbac_stream_t s) {
    static const NodeRrTable<NodeRkGridBwdLaunch> table = NODE_RR_BWD_TABLE(node_grid_bwd_kernel);
    return traj_bwd(table, "nlbac_node_rk_grid_bwd", 0.f, hs, hs_host, f, g, u, n, H, n_stages, beta, c_out, G, acts_f,
                    acts_f_ls, acts_g, acts_g_ls, acts_bits, dout, dx0, du, dK, dG, dz_f, dz_g, s);
}

// ---- the same grid under step_size: H = N fine intervals with steps hs / hs_host [N]; the T - 1 output points 1 .. T-1
//      are read off them — interval i holds the outputs ofs[i] <= j < ofs[i+1], weights theta [T-1] (device arrays for
//      the kernel, ofs_host / theta_host beside them for the checks here, nlbac_subgrid_check).  out [T-1][n][n_s],
//      dout [T][n][n_s]; K / Y / G / acts / dK / dG / dz per fine stage, [N * n_stages][n][..]
extern "C" int nlbac_node_rk_subgrid_fwd(const nlbac_mlp* f, const nlbac_mlp* g, const float* x0, const float* u, int n,
                                         int H, int n_stages, const float* beta, const float* c_out, const float* hs,
                                         const float* hs_host, const int* ofs, const int* ofs_host, const float* theta,
                                         const float* theta_host, int T, float* out, float* K, float* Y, float* G,
                                         float* acts_f, long acts_f_ls, float* acts_g, long acts_g_ls, int acts_bits,
                                         nlbac_stream_t s) {
    static const NodeRrTable<NodeRkSubgridFwdLaunch> table = NODE_RR_FWD_TABLE(node_subgrid_fwd_kernel);
    const NlbacSubGridArgs sg = {ofs, ofs_host, theta, theta_host, T};
    return traj_fwd(table, "nlbac_node_rk_subgrid_fwd", 0.f, hs, hs_host, f, g, x0, u, n, H, n_stages, beta, c_out, out,
                    K, Y, G, acts_f, acts_f_ls, acts_g, acts_g_ls, acts_bits, s, &sg);
}

extern "C" int nlbac_node_rk_subgrid_bwd(const nlbac_mlp* f, const nlbac_mlp* g, const float* u, int n, int H,
                                         int n_stages, const float* beta, const float* c_out, const float* hs,
                                         const float* hs_host, const int* ofs, const int* ofs_host, const float* theta,
                                         const float* theta_host, int T, const float* G, const float* acts_f,
                                         long acts_f_ls, const float* acts_g, long acts_g_ls, int acts_bits,
                                         const float* dout, float* dx0, float* du, float* dK, float* dG, float* dz_f,
                                         float* dz_g, nlbac_stream_t s) {
    static const NodeRrTable<NodeRkSubgridBwdLaunch> table = NODE_RR_BWD_TABLE(node_subgrid_bwd_kernel);
    const NlbacSubGridArgs sg = {ofs, ofs_host, theta, theta_host, T};
    return traj_bwd(table, "nlbac_node_rk_subgrid_bwd", 0.f, hs, hs_host, f, g, u, n, H, n_stages, beta, c_out, G,
                    acts_f, acts_f_ls, acts_g, acts_g_ls, acts_bits, dout, dx0, du, dK, dG, dz_f, dz_g, s, &sg);
}

// ---- a rollout under step_size: H control intervals of m fine steps each, steps hs / hs_host [m] (the same schedule in
//      every control interval; device array for the kernel, host copy for the checks here), the actions u [H][n][n_u] held
//      through their control interval.  out [H][n][n_s], dout [H+1][n][n_s], du [H][n][n_u]; K / Y / G / acts / dK / dG /
//      dz per fine stage, [H * m * n_stages][n][..]
extern "C" int nlbac_node_rk_hold_fwd(const nlbac_mlp* f, const nlbac_mlp* g, const float* x0, const float* u, int n,
                                      int H, int n_stages, const float* beta, const float* c_out, const float* hs,
                                      const float* hs_host, int m, float* out, float* K, float* Y, float* G,
                                      float* acts_f, long acts_f_ls, float* acts_g, long acts_g_ls, int acts_bits,
                                      nlbac_stream_t s) {
    static const NodeRrTable<NodeRkHoldFwdLaunch> table = NODE_RR_FWD_TABLE(node_hold_fwd_kernel);
    int N = 0;
    if (nlbac_hold_intervals(H, m, n_stages, n, "nlbac_node_rk_hold_fwd", &N)) return -1;
    return traj_fwd(table, "nlbac_node_rk_hold_fwd", 0.f, hs, hs_host, f, g, x0, u, n, N, n_stages, beta, c_out, out, K,
                    Y, G, acts_f, acts_f_ls, acts_g, acts_g_ls, acts_bits, s, nullptr, m);
}

extern "C" int nlbac_node_rk_hold_bwd(const nlbac_mlp* f, const nlbac_mlp* g, const float* u, int n, int H,
                                      int n_stages, const float* beta, const float* c_out, const float* hs,
                                      const float* hs_host, int m, const float* G, const float* acts_f, long acts_f_ls,
                                      const float* acts_g, long acts_g_ls, int acts_bits, const float* dout, float* dx0,
                                      float* du, float* dK, float* dG, float* dz_f, float* dz_g, nlbac_stream_t s) {
    static const NodeRrTable<NodeRkHoldBwdLaunch> table = NODE_RR_BWD_TABLE(node_hold_bwd_kernel);
    int N = 0;
    if (nlbac_hold_intervals(H, m, n_stages, n, "nlbac_node_rk_hold_bwd", &N)) return -1;
    return traj_bwd(table, "nlbac_node_rk_hold_bwd", 0.f, hs, hs_host, f, g, u, n, N, n_stages, beta, c_out, G, acts_f,
                    acts_f_ls, acts_g, acts_g_ls, acts_bits, dout, dx0, du, dK, dG, dz_f, dz_g, s, nullptr, m);
}
