// dopri5 rollouts of the control-affine NODE  dx/dt = f(x) + g(x) u  under TILE-LOCAL step control: H control intervals,
// forward and backward, in one launch each on the register-resident layer chains.
//
// torchdiffeq's dopri5 — and the chained solves of rollout(method="dopri5") — control the step with one RMS norm over the
// whole batch: every attempt ends in a reduction over all rows, which a single launch could only take behind grid-wide
// waits (node_traj_kernels.hip's header).  Here each 32-row tile of the batch is an adaptive solve of its own: its own
// error norm (over its rows' [x | u] entries), step sizes and accept decisions — the per-sample step control of batched
// ODE libraries at the granularity the kernels work in.  A tile never waits for another workgroup, so the whole adaptive
// solve of a tile, and a whole horizon of them, is one launch: no control block in HBM, no look by the host.
//
// The definition: the rows [32 j, 32 j + 32) of the result are the chained dopri5 rollout of those rows alone.  Each
// interval runs through the code of the chained solve's launches in their order (node_rr_body.h with TILE; the phases,
// norms, controller and slots: node_rk_shared.h), so that the decisions, and with them the values, are the chain's.
//
// Reference: the chained odeint calls of C/sac_cbf_clf/sac_cbf_clf.py:437-458 and P/sac_cbf_clf/sac_cbf_clf.py:459-534
// (odeint(model, [x_k | u_k], [0, dt], method="dopri5")[-1], one interval per call), on a batch of one tile's rows.
#undef RR_TIMING          // (the ablation stamps belong to the one-step kernels)
#include "node_rr_body.h"
#include "node_tile_launch.h"      // what a tile launch checks and carries, shared with node_tile_dense_kernels.hip

struct NodeTileFwdLaunch {
    NodeRkLaunch L;
    NodeTileFwd X;
};

struct NodeTileBwdLaunch {
    NodeRkBwdLaunch L;
    NodeTileBwd X;
};

template <int NB, int R, int BITS, int SPLIT>
__global__ __launch_bounds__(256) void node_tile_fwd_kernel(const NodeTileFwdLaunch A) {
    node_rr_fwd_body<NB, R, BITS, SPLIT, false, false, false, false, true>(A.L, A.X.H, nullptr, nullptr, 1, &A.X);
}

template <int NB, int R, int BITS, int SPLIT>
__global__ __launch_bounds__(256) void node_tile_bwd_kernel(const NodeTileBwdLaunch A) {
    node_rr_bwd_body<NB, R, BITS, SPLIT, false, false, false, false, true>(A.L, nullptr, nullptr, nullptr, 1, &A.X);
}

extern "C" int nlbac_node_dopri_tile_ok(const nlbac_mlp* f, const nlbac_mlp* g) {
    return (f && g && nlbac_node_rr_eligible(f, g)) ? 1 : 0;
}

// One launch: H intervals of dopri5 for every 32-row tile of the n rows.  x0 [n][n_s], u [H][n][n_u], out [H][n][n_s]
// (the state behind every interval), beta [7][7] / c_err [7]: dopri5's table and error weights.  accepted / attempts
// [tiles][H] and status [tiles] (zero on entry) receive the counts and the tiles' TILE_* status.
// G non-null: a backward follows — every accepted step is kept in a slot of max_slots per tile: G [max_slots * 7][n][n_s n_u],
// acts_* / acts_bits as in nlbac_node_rk_traj_fwd over max_slots * 7 stages (zero on entry: a stage nobody evaluated
// must read as zero), Y (weight gradients only, zero on entry) the stage inputs, hslots [tiles][max_slots],
// iv_first / iv_x [tiles][H].  G null: nothing is kept; acts_bits still picks the kernel instance (its sums).
// The *_paged_* entry points: the same launches with the slots counted per tile — page0 [tiles + 1] (device ints, the
// exclusive prefix sum of the tiles' slot counts) and `pages`, their total, in place of max_slots; the kept buffers are
// pages x 7 stages x 32 rows (node_rk_shared.h: PAGED), hslots [pages].  A forward that keeps nothing (G null) takes no
// page0 (null, pages 0): it is the launch that counts a solve's steps.
static int tile_fwd(const char* who, const nlbac_mlp* f, const nlbac_mlp* g, const float* x0, const float* u, int n, int H,
                    const float* beta, const float* c_err, double dt, float rtol, float atol, float* out, const int* page0,
                    int max_slots, float* Y, float* G, float* acts_f, long acts_f_ls, float* acts_g, long acts_g_ls,
                    int acts_bits, double* hslots, int* iv_first, float* iv_x, int* accepted, int* attempts, int* status,
                    nlbac_stream_t s) {
    static const NodeRrTable<NodeTileFwdLaunch> table = NODE_RR_FWD_TABLE(node_tile_fwd_kernel);
    NodeTileFwdLaunch A;
    memset(&A, 0, sizeof(A));
    if (tile_fill_fwd(A.L, A.X, who, H, H, "intervals", "H", f, g, x0, u, n, beta, c_err, dt, rtol, atol, out, page0,
                      max_slots, Y, G, acts_f, acts_f_ls, acts_g, acts_g_ls, acts_bits, hslots, accepted, attempts, status))
        return -1;
    NLBAC_REQUIRE(!G || (iv_first && iv_x), "%s: G, the acts and the slot arrays go together", who);
    A.X.iv_first = iv_first; A.X.iv_x = iv_x;
    node_rr_start(table, A, f->hid, n, acts_bits, node_tile_fwd_lds_floats(), (hipStream_t)s);
    NLBAC_CHECK_LAUNCH(who);
    return 0;
}

extern "C" int nlbac_node_dopri_tile_fwd(const nlbac_mlp* f, const nlbac_mlp* g, const float* x0, const float* u, int n,
                                         int H, const float* beta, const float* c_err, double dt, float rtol, float atol,
                                         float* out, int max_slots, float* Y, float* G, float* acts_f, long acts_f_ls,
                                         float* acts_g, long acts_g_ls, int acts_bits, double* hslots, int* iv_first,
                                         float* iv_x, int* accepted, int* attempts, int* status, nlbac_stream_t s) {
    return tile_fwd("nlbac_node_dopri_tile_fwd", f, g, x0, u, n, H, beta, c_err, dt, rtol, atol, out, nullptr, max_slots, Y,
                    G, acts_f, acts_f_ls, acts_g, acts_g_ls, acts_bits, hslots, iv_first, iv_x, accepted, attempts, status, s);
}

extern "C" int nlbac_node_dopri_tile_paged_fwd(const nlbac_mlp* f, const nlbac_mlp* g, const float* x0, const float* u,
                                               int n, int H, const float* beta, const float* c_err, double dt, float rtol,
                                               float atol, float* out, const int* page0, int pages, float* Y, float* G,
                                               float* acts_f, long acts_f_ls, float* acts_g, long acts_g_ls, int acts_bits,
                                               double* hslots, int* iv_first, float* iv_x, int* accepted, int* attempts,
                                               int* status, nlbac_stream_t s) {
    const char* who = "nlbac_node_dopri_tile_paged_fwd";
    NLBAC_REQUIRE(page0 ? pages > 0 : (pages == 0 && !G), "%s: page0 and pages go together, and with G", who);
    return tile_fwd(who, f, g, x0, u, n, H, beta, c_err, dt, rtol, atol, out, page0, pages, Y, G, acts_f, acts_f_ls, acts_g,
                    acts_g_ls, acts_bits, hslots, iv_first, iv_x, accepted, attempts, status, s);
}

// One launch: the backward of the horizon nlbac_node_dopri_tile_fwd kept, every tile's steps last to first.  iv_nacc: the
// forward's `accepted`.  dout [H+1][n][n_s], dx0 [n][n_s], du [H][n][n_u]; dK / dG / dz_* (all or none; zero on entry) per
// (slot, stage, row) for the weight gradients, as in nlbac_node_rk_traj_bwd.  Only tiles whose status is TILE_OK have a
// backward: the caller reads status first.
static int tile_bwd(const char* who, const nlbac_mlp* f, const nlbac_mlp* g, const float* u, int n, int H, const float* beta,
                    const int* page0, int max_slots, const double* hslots, const int* iv_first, const int* iv_nacc,
                    const float* iv_x, const float* G, const float* acts_f, long acts_f_ls, const float* acts_g,
                    long acts_g_ls, int acts_bits, const float* dout, float* dx0, float* du, float* dK, float* dG,
                    float* dz_f, float* dz_g, nlbac_stream_t s) {
    static const NodeRrTable<NodeTileBwdLaunch> table = NODE_RR_BWD_TABLE(node_tile_bwd_kernel);
    NodeTileBwdLaunch A;
    memset(&A, 0, sizeof(A));
    if (tile_fill_bwd(A.L, A.X, who, H, H, "intervals", "H", f, g, u, n, beta, page0, max_slots, hslots, iv_nacc, G, acts_f,
                      acts_f_ls, acts_g, acts_g_ls, acts_bits, dout, dx0, du, dK, dG, dz_f, dz_g))
        return -1;
    NLBAC_REQUIRE(iv_first && iv_x, "%s: null pointer", who);
    A.X.iv_first = iv_first; A.X.iv_x = iv_x;
    node_rr_start(table, A, f->hid, n, acts_bits, node_rr_bwd_lds_floats(), (hipStream_t)s);
    NLBAC_CHECK_LAUNCH(who);
    return 0;
}

extern "C" int nlbac_node_dopri_tile_bwd(const nlbac_mlp* f, const nlbac_mlp* g, const float* u, int n, int H,
                                         const float* beta, int max_slots, const double* hslots, const int* iv_first,
                                         const int* iv_nacc, const float* iv_x, const float* G, const float* acts_f,
                                         long acts_f_ls, const float* acts_g, long acts_g_ls, int acts_bits,
                                         const float* dout, float* dx0, float* du, float* dK, float* dG, float* dz_f,
                                         float* dz_g, nlbac_stream_t s) {
    return tile_bwd("nlbac_node_dopri_tile_bwd", f, g, u, n, H, beta, nullptr, max_slots, hslots, iv_first, iv_nacc, iv_x, G,
                    acts_f, acts_f_ls, acts_g, acts_g_ls, acts_bits, dout, dx0, du, dK, dG, dz_f, dz_g, s);
}

extern "C" int nlbac_node_dopri_tile_paged_bwd(const nlbac_mlp* f, const nlbac_mlp* g, const float* u, int n, int H,
                                               const float* beta, const int* page0, int pages, const double* hslots,
                                               const int* iv_first, const int* iv_nacc, const float* iv_x, const float* G,
                                               const float* acts_f, long acts_f_ls, const float* acts_g, long acts_g_ls,
                                               int acts_bits, const float* dout, float* dx0, float* du, float* dK,
                                               float* dG, float* dz_f, float* dz_g, nlbac_stream_t s) {
    const char* who = "nlbac_node_dopri_tile_paged_bwd";
    NLBAC_REQUIRE(page0, "%s: null page0", who);
    return tile_bwd(who, f, g, u, n, H, beta, page0, pages, hslots, iv_first, iv_nacc, iv_x, G, acts_f, acts_f_ls, acts_g,
                    acts_g_ls, acts_bits, dout, dx0, du, dK, dG, dz_f, dz_g, s);
}
