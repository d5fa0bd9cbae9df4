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

// what the scalar-step launch and the time-grid launch share: the descriptor of the interval's one-step launch
static int traj_fwd_fill(NodeRkLaunch& L, const nlbac_mlp* f, const nlbac_mlp* g, const float* x0, const float* u, int n,
                         int n_stages, const float* beta, const float* c_out, float h, float* out, float* K, float* Y,
                         float* G, float* acts_f, long acts_f_ls, float* acts_g, long acts_g_ls, int acts_bits,
                         const char* who) {
    NLBAC_REQUIRE(x0 && u && out && K && Y && G, "%s: null pointer", who);
    NLBAC_REQUIRE((acts_f == nullptr) == (acts_g == nullptr), "%s: acts_f and acts_g go together", who);
    NLBAC_REQUIRE(acts_f || acts_bits == 0, "%s: acts_bits without acts", who);
    L.net[0] = *f; L.net[1] = *g;
    L.y0 = x0; L.u = u;
    L.n = n; L.rpp = n; L.n_s = f->in_dim; L.n_u = g->out_dim / f->in_dim;
    L.stage_begin = 0; L.stage_end = n_stages; L.S_total = n_stages;
    for (int i = 0; i < n_stages; ++i) {
        for (int j = 0; j < n_stages; ++j) L.beta[i][j] = beta[i * n_stages + j];
        L.c_out[i] = c_out[i];
    }
    L.n_out = n_stages;
    L.h_val[0] = h;
    L.K = K; L.Y = Y; L.G = G;
    L.acts[0] = acts_f; L.acts[1] = acts_g; L.acts_ls[0] = acts_f_ls; L.acts_ls[1] = acts_g_ls;
    L.acts_bits = acts_bits;
    L.out = out;
    L.norm_mode = -1;
    return 0;
}

// the one-step launcher's choice of instance (nlbac_node_rr_fwd_launch), so that the sums are the same: the instances of
// one kernel template as a table, [SPLIT][shape][BITS != 0] and the activation-row instances [shape]
template <typename KernelF>
struct NodeTrajFwdTable {
    KernelF kf[2][3][2];
    KernelF kfw[3];
};

#define NODE_TRAJ_FWD_TABLE(KERN)                                                                                       \
    {{{{KERN<4, 4, 0, 0>, KERN<4, 4, 1, 0>}, {KERN<7, 1, 0, 0>, KERN<7, 1, 1, 0>}, {KERN<8, 4, 0, 0>, KERN<8, 4, 1, 0>}},  \
      {{KERN<4, 4, 0, 1>, KERN<4, 4, 1, 1>}, {KERN<7, 1, 0, 1>, KERN<7, 1, 1, 1>}, {KERN<8, 4, 0, 1>, KERN<8, 4, 1, 1>}}}, \
     {KERN<4, 4, 2, 0>, KERN<7, 1, 2, 0>, KERN<8, 4, 2, 0>}}

template <typename KernelF>
static KernelF node_traj_fwd_pick(const NodeTrajFwdTable<KernelF>& t, const nlbac_mlp* f, int acts_bits) {
    const int shape = nlbac_node_rr_shape(f->hid);
    return (acts_bits == 2) ? t.kfw[shape] : t.kf[(nlbac_node_rr_split() && acts_bits) ? 1 : 0][shape][acts_bits ? 1 : 0];
}

static size_t traj_fwd_lds() {
    return (size_t)(RkFwdTile::floats() + NLBAC_MLP_TILE * 8 + 2 * 3 * 8 * 64 + 2 * 32 * 64 + NLBAC_MLP_TILE * RK_MAX_NS +
                    2 * 2 * 64 + 4) * sizeof(float);
}

extern "C" int nlbac_node_rk_traj_fwd(const nlbac_mlp* f, const nlbac_mlp* g, const float* x0, const float* u, int n,
                                      int H, int n_stages, const float* beta, const float* c_out, float h, float* out,
                                      float* K, float* Y, float* G, float* acts_f, long acts_f_ls, float* acts_g,
                                      long acts_g_ls, int acts_bits, nlbac_stream_t s) {
    if (traj_check(f, g, n, H, n_stages, beta, c_out, h, acts_bits, "nlbac_node_rk_traj_fwd")) return -1;
    NodeRkTrajFwdLaunch A;
    memset(&A, 0, sizeof(A));
    if (traj_fwd_fill(A.L, f, g, x0, u, n, n_stages, beta, c_out, h, out, K, Y, G, acts_f, acts_f_ls, acts_g, acts_g_ls,
                      acts_bits, "nlbac_node_rk_traj_fwd")) return -1;
    A.H = H;
    using KernelF = void (*)(const NodeRkTrajFwdLaunch);
    static const NodeTrajFwdTable<KernelF> table = NODE_TRAJ_FWD_TABLE(node_traj_fwd_kernel);
    const KernelF k = node_traj_fwd_pick(table, f, acts_bits);
    hipLaunchKernelGGL(k, dim3(nlbac_ceil_div(n, NLBAC_MLP_TILE)), dim3(256), traj_fwd_lds(), (hipStream_t)s, A);
    NLBAC_CHECK_LAUNCH("nlbac_node_rk_traj_fwd");
    return 0;
}

static int traj_bwd_fill(NodeRkBwdLaunch& L, NodeRkTrajBwd& X, const nlbac_mlp* f, const nlbac_mlp* g, const float* u,
                         int n, int H, int n_stages, const float* beta, const float* c_out, float h, const float* G,
                         const float* acts_f, long acts_f_ls, const float* acts_g, long acts_g_ls, int acts_bits,
                         const float* dout, float* dx0, float* du, float* dK, float* dG, float* dz_f, float* dz_g,
                         const char* who) {
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
    for (int i = 0; i < n_stages; ++i)
        for (int j = 0; j < n_stages; ++j) L.beta[i][j] = beta[i * n_stages + j];
    L.h_val[0] = h;
    X.H = H; X.dout = dout; X.dx0 = dx0;
    for (int j = 0; j < n_stages; ++j) X.c_out[j] = c_out[j];
    X.n_out = n_stages;
    return 0;
}

// the one-step launcher's choice of instance (nlbac_node_rr_bwd_launch): [SPLIT][shape][BITS != 0] and the
// activation-row instances [SPLIT][shape]
template <typename KernelB>
struct NodeTrajBwdTable {
    KernelB kb[2][3][2];
    KernelB kbw[2][3];
};

#define NODE_TRAJ_BWD_TABLE(KERN)                                                                                       \
    {{{{KERN<4, 4, 0, 0>, KERN<4, 4, 1, 0>}, {KERN<7, 1, 0, 0>, KERN<7, 1, 1, 0>}, {KERN<8, 4, 0, 0>, KERN<8, 4, 1, 0>}},  \
      {{KERN<4, 4, 0, 1>, KERN<4, 4, 1, 1>}, {KERN<7, 1, 0, 1>, KERN<7, 1, 1, 1>}, {KERN<8, 4, 0, 1>, KERN<8, 4, 1, 1>}}}, \
     {{KERN<4, 4, 2, 0>, KERN<7, 1, 2, 0>, KERN<8, 4, 2, 0>}, {KERN<4, 4, 2, 1>, KERN<7, 1, 2, 1>, KERN<8, 4, 2, 1>}}}

template <typename KernelB>
static KernelB node_traj_bwd_pick(const NodeTrajBwdTable<KernelB>& t, const nlbac_mlp* f, int acts_bits) {
    const int split = nlbac_node_rr_split() ? 1 : 0, shape = nlbac_node_rr_shape(f->hid);
    return (acts_bits == 2) ? t.kbw[split][shape] : t.kb[split][shape][acts_bits ? 1 : 0];
}

static size_t traj_bwd_lds() {
    return (size_t)(RkBwdTile::floats() + 2 * 4 * 8 * 64 + 2 * 32 * 64 + 2 * 16 * 64 + 4) * sizeof(float);
}

extern "C" int nlbac_node_rk_traj_bwd(const nlbac_mlp* f, const nlbac_mlp* g, const float* u, int n, int H,
                                      int n_stages, const float* beta, const float* c_out, float h, const float* G,
                                      const float* acts_f, long acts_f_ls, const float* acts_g, long acts_g_ls,
                                      int acts_bits, const float* dout, float* dx0, float* du, float* dK, float* dG,
                                      float* dz_f, float* dz_g, nlbac_stream_t s) {
    if (traj_check(f, g, n, H, n_stages, beta, c_out, h, acts_bits, "nlbac_node_rk_traj_bwd")) return -1;
    NodeRkTrajBwdLaunch A;
    memset(&A, 0, sizeof(A));
    if (traj_bwd_fill(A.L, A.X, f, g, u, n, H, n_stages, beta, c_out, h, G, acts_f, acts_f_ls, acts_g, acts_g_ls,
                      acts_bits, dout, dx0, du, dK, dG, dz_f, dz_g, "nlbac_node_rk_traj_bwd")) return -1;
    using KernelB = void (*)(const NodeRkTrajBwdLaunch);
    static const NodeTrajBwdTable<KernelB> table = NODE_TRAJ_BWD_TABLE(node_traj_bwd_kernel);
    const KernelB k = node_traj_bwd_pick(table, f, acts_bits);
    hipLaunchKernelGGL(k, dim3(nlbac_ceil_div(n, NLBAC_MLP_TILE)), dim3(256), traj_bwd_lds(), (hipStream_t)s, A);
    NLBAC_CHECK_LAUNCH("nlbac_node_rk_traj_bwd");
    return 0;
}

// ---- the solution on a time grid: a step size per interval (hs [H] on the device for the kernel, hs_host [H] beside it
//      for the launcher's checks, nlbac_grid_steps_check), one set of actions u [n][n_u], du [n][n_u] summed over the
//      intervals
extern "C" int nlbac_node_rk_grid_fwd(const nlbac_mlp* f, const nlbac_mlp* g, const float* x0, const float* u, int n,
                                      int H, int n_stages, const float* beta, const float* c_out, const float* hs,
                                      const float* hs_host, float* out, float* K, float* Y, float* G, float* acts_f,
                                      long acts_f_ls, float* acts_g, long acts_g_ls, int acts_bits, nlbac_stream_t s) {
    if (traj_check(f, g, n, H, n_stages, beta, c_out, 1.f, acts_bits, "nlbac_node_rk_grid_fwd")) return -1;
    if (nlbac_grid_steps_check(hs, hs_host, H, "nlbac_node_rk_grid_fwd")) return -1;
    NodeRkGridFwdLaunch A;
    memset(&A, 0, sizeof(A));
    if (traj_fwd_fill(A.L, f, g, x0, u, n, n_stages, beta, c_out, hs_host[0], out, K, Y, G, acts_f, acts_f_ls, acts_g,
                      acts_g_ls, acts_bits, "nlbac_node_rk_grid_fwd")) return -1;
    // the kernel rewrites the step slot sH with no barrier in front of the interval's first stage: that stage has to
    // be stage 0, the one whose input uses no step size
    NLBAC_REQUIRE(A.L.stage_begin == 0, "nlbac_node_rk_grid_fwd: a time-grid launch starts every interval at stage 0");
    A.H = H; A.hs = hs;
    using KernelF = void (*)(const NodeRkGridFwdLaunch);
    static const NodeTrajFwdTable<KernelF> table = NODE_TRAJ_FWD_TABLE(node_grid_fwd_kernel);
    const KernelF k = node_traj_fwd_pick(table, f, acts_bits);
    hipLaunchKernelGGL(k, dim3(nlbac_ceil_div(n, NLBAC_MLP_TILE)), dim3(256), traj_fwd_lds(), (hipStream_t)s, A);
    NLBAC_CHECK_LAUNCH("nlbac_node_rk_grid_fwd");
    return 0;
}

extern "C" int nlbac_node_rk_grid_bwd(const nlbac_mlp* f, const nlbac_mlp* g, const float* u, int n, int H,
                                      int n_stages, const float* beta, const float* c_out, const float* hs,
                                      const float* hs_host, const float* G, const float* acts_f, long acts_f_ls,
                                      const float* acts_g, long acts_g_ls, int acts_bits, const float* dout, float* dx0,
                                      float* du, float* dK, float* dG, float* dz_f, float* dz_g, nlbac_stream_t s) {
    if (traj_check(f, g, n, H, n_stages, beta, c_out, 1.f, acts_bits, "nlbac_node_rk_grid_bwd")) return -1;
    if (nlbac_grid_steps_check(hs, hs_host, H, "nlbac_node_rk_grid_bwd")) return -1;
    NodeRkGridBwdLaunch A;
    memset(&A, 0, sizeof(A));
    if (traj_bwd_fill(A.L, A.X, f, g, u, n, H, n_stages, beta, c_out, hs_host[H - 1], G, acts_f, acts_f_ls, acts_g,
                      acts_g_ls, acts_bits, dout, dx0, du, dK, dG, dz_f, dz_g, "nlbac_node_rk_grid_bwd")) return -1;
    A.hs = hs;
    using KernelB = void (*)(const NodeRkGridBwdLaunch);
    static const NodeTrajBwdTable<KernelB> table = NODE_TRAJ_BWD_TABLE(node_grid_bwd_kernel);
    const KernelB k = node_traj_bwd_pick(table, f, acts_bits);
    hipLaunchKernelGGL(k, dim3(nlbac_ceil_div(n, NLBAC_MLP_TILE)), dim3(256), traj_bwd_lds(), (hipStream_t)s, A);
    NLBAC_CHECK_LAUNCH("nlbac_node_rk_grid_bwd");
    return 0;
}
