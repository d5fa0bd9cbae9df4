// odeint_dense of the control-affine NODE  dx/dt = f(x) + g(x) u  under TILE-LOCAL step control: ONE adaptive dopri5
// solve per 32-row tile, read at every point of a time grid, forward and backward in one launch each on the
// register-resident layer chains.
//
// The definition: the rows [32 j, 32 j + 32) of the result are odeint_dense's batch solve (the device-driven chain, then
// nlbac_dopri_dense_fwd over its step slots; ode_dense.py) of those rows alone.  The tile runs the one interval
// [0, tau[n_out - 1]] through node_tile_kernels.hip's phases (node_rr_body.h with TILE and DENSE: stage 0, mode 0, the
// probe, mode 1, attempts with FSAL, the controller in LDS) and, behind every ACCEPTED attempt, writes the outputs the
// step reaches — dopri_dense_fwd_kernel's walk (ode_kernels.hip), t accumulated in double in the controller's order.
// The backward walks the tile's slots last to first: a slot first takes the gradients of its own outputs
// (dopri_dense_bwd_kernel's sums), then the hand-over from the later step as adds (nlbac_dopri_dense_carry), then the
// step's own backward adds onto both (nlbac_node_rk_bwd without a chain description).
//
// Reference: torchdiffeq.odeint(func, y0, t) with len(t) > 2 on its adaptive path (one solve, outputs interpolated
// off the accepted steps), the call of U/sac_cbf_clf/model.py:252 on a time series, on a batch of one tile's rows.
#undef RR_TIMING          // (the ablation stamps belong to the one-step kernels)
#include "node_rr_body.h"
#include "node_tile_launch.h"      // what a tile launch checks and carries, shared with node_tile_kernels.hip

struct NodeTileDenseFwdLaunch {
    NodeRkLaunch L;
    NodeTileFwd X;
    NodeTileDenseFwd D;
};

struct NodeTileDenseBwdLaunch {
    NodeRkBwdLaunch L;
    NodeTileBwd X;
    NodeTileDenseBwd D;
};

template <int NB, int R, int BITS, int SPLIT>
__global__ __launch_bounds__(256) void node_tile_dense_fwd_kernel(const NodeTileDenseFwdLaunch A) {
    node_rr_fwd_body<NB, R, BITS, SPLIT, false, false, false, false, true, true>(A.L, 1, nullptr, nullptr, 1, &A.X, &A.D);
}

template <int NB, int R, int BITS, int SPLIT>
__global__ __launch_bounds__(256) void node_tile_dense_bwd_kernel(const NodeTileDenseBwdLaunch A) {
    node_rr_bwd_body<NB, R, BITS, SPLIT, false, false, false, false, true, true>(A.L, nullptr, nullptr, nullptr, 1, &A.X, &A.D);
}

// One launch: a dense dopri5 solve of every 32-row tile of the n rows over [0, t_end], read at tau [n_out] (DEVICE
// doubles, increasing, tau[n_out - 1] == t_end).  x0 [n][n_s], u [n][n_u], out [n_out][n][n_s].  accepted / attempts /
// status [tiles] (zero on entry) receive each tile's counts and TILE_* status; a tile that stops writes NaN into its rows
// of the outputs it has not emitted.  G non-null: a backward follows — the kept buffers of nlbac_node_dopri_tile_fwd
// (max_slots slots per tile, zero on entry), and ov_slot / ov_x [tiles][n_out]: the slot that emitted output j and its
// abscissa.  G null: nothing is kept and no slot runs out.
// The *_paged_* entry points: the same launches with the slots counted per tile, as node_tile_kernels.hip's — page0
// [tiles + 1] and `pages` in place of max_slots, the kept buffers pages x 7 stages x 32 rows, hslots [pages]; ov_slot
// stays relative to the tile.  A forward that keeps nothing takes no page0 (null, pages 0).
static int tile_dense_fwd(const char* who, const nlbac_mlp* f, const nlbac_mlp* g, const float* x0, const float* u, int n,
                          const float* beta, const float* c_err, const double* tau, int n_out, double t_end, float rtol,
                          float atol, float* out, const int* page0, int max_slots, float* Y, float* G, float* acts_f,
                          long acts_f_ls, float* acts_g, long acts_g_ls, int acts_bits, double* hslots, int* ov_slot,
                          float* ov_x, int* accepted, int* attempts, int* status, nlbac_stream_t s) {
    static const NodeRrTable<NodeTileDenseFwdLaunch> table = NODE_RR_FWD_TABLE(node_tile_dense_fwd_kernel);
    NodeTileDenseFwdLaunch A;
    memset(&A, 0, sizeof(A));
    if (tile_fill_fwd(A.L, A.X, who, 1, n_out, "output times", "1", f, g, x0, u, n, beta, c_err, t_end, rtol, atol, out,
                      page0, max_slots, Y, G, acts_f, acts_f_ls, acts_g, acts_g_ls, acts_bits, hslots, accepted, attempts, status))
        return -1;
    NLBAC_REQUIRE(tau, "%s: null pointer", who);
    NLBAC_REQUIRE(!G || (ov_slot && ov_x), "%s: G, the acts and the slot arrays go together", who);
    A.D.tau = tau; A.D.n_out = n_out; A.D.ov_slot = ov_slot; A.D.ov_x = ov_x;
    node_rr_start(table, A, f->hid, n, acts_bits, node_tile_fwd_lds_floats(), (hipStream_t)s);
    NLBAC_CHECK_LAUNCH(who);
    return 0;
}

extern "C" int nlbac_node_dopri_tile_dense_fwd(const nlbac_mlp* f, const nlbac_mlp* g, const float* x0, const float* u,
                                               int n, const float* beta, const float* c_err, const double* tau, int n_out,
                                               double t_end, float rtol, float atol, float* out, int max_slots, float* Y,
                                               float* G, float* acts_f, long acts_f_ls, float* acts_g, long acts_g_ls,
                                               int acts_bits, double* hslots, int* ov_slot, float* ov_x, int* accepted,
                                               int* attempts, int* status, nlbac_stream_t s) {
    return tile_dense_fwd("nlbac_node_dopri_tile_dense_fwd", f, g, x0, u, n, beta, c_err, tau, n_out, t_end, rtol, atol, out,
                          nullptr, max_slots, Y, G, acts_f, acts_f_ls, acts_g, acts_g_ls, acts_bits, hslots, ov_slot, ov_x,
                          accepted, attempts, status, s);
}

extern "C" int nlbac_node_dopri_tile_dense_paged_fwd(const nlbac_mlp* f, const nlbac_mlp* g, const float* x0,
                                                     const float* u, int n, const float* beta, const float* c_err,
                                                     const double* tau, int n_out, double t_end, float rtol, float atol,
                                                     float* out, const int* page0, int pages, float* Y, float* G,
                                                     float* acts_f, long acts_f_ls, float* acts_g, long acts_g_ls,
                                                     int acts_bits, double* hslots, int* ov_slot, float* ov_x,
                                                     int* accepted, int* attempts, int* status, nlbac_stream_t s) {
    const char* who = "nlbac_node_dopri_tile_dense_paged_fwd";
    NLBAC_REQUIRE(page0 ? pages > 0 : (pages == 0 && !G), "%s: page0 and pages go together, and with G", who);
    return tile_dense_fwd(who, f, g, x0, u, n, beta, c_err, tau, n_out, t_end, rtol, atol, out, page0, pages, Y, G, acts_f,
                          acts_f_ls, acts_g, acts_g_ls, acts_bits, hslots, ov_slot, ov_x, accepted, attempts, status, s);
}

// One launch: the backward of the solve nlbac_node_dopri_tile_dense_fwd kept, every tile's slots last to first.
// nacc [tiles]: the forward's `accepted`.  dout [n_out][n][n_s]: the gradients of the outputs 1 .. n_out; dx0 [n][n_s]
// (slot 0's dy0 — the gradient of out[0] is the caller's to add), du [n][n_u]; dK / dG / dz_* (all or none; zero on
// entry) per (slot, stage, row) for the weight gradients.  Only tiles whose status is TILE_OK have a backward: the
// caller reads status first.  What is read of nacc / ov_slot is clamped to the slots and the outputs.
static int tile_dense_bwd(const char* who, const nlbac_mlp* f, const nlbac_mlp* g, const float* u, int n, const float* beta,
                          int n_out, const int* page0, int max_slots, const double* hslots, const int* ov_slot,
                          const float* ov_x, const int* nacc, const float* G, const float* acts_f, long acts_f_ls,
                          const float* acts_g, long acts_g_ls, int acts_bits, const float* dout, float* dx0, float* du,
                          float* dK, float* dG, float* dz_f, float* dz_g, nlbac_stream_t s) {
    static const NodeRrTable<NodeTileDenseBwdLaunch> table = NODE_RR_BWD_TABLE(node_tile_dense_bwd_kernel);
    NodeTileDenseBwdLaunch A;
    memset(&A, 0, sizeof(A));
    if (tile_fill_bwd(A.L, A.X, who, 1, n_out, "output times", "1", f, g, u, n, beta, page0, max_slots, hslots, nacc, G, acts_f,
                      acts_f_ls, acts_g, acts_g_ls, acts_bits, dout, dx0, du, dK, dG, dz_f, dz_g))
        return -1;
    NLBAC_REQUIRE(ov_slot && ov_x, "%s: null pointer", who);
    A.D.n_out = n_out; A.D.ov_slot = ov_slot; A.D.ov_x = ov_x;
    node_rr_start(table, A, f->hid, n, acts_bits, node_rr_bwd_lds_floats(), (hipStream_t)s);
    NLBAC_CHECK_LAUNCH(who);
    return 0;
}

extern "C" int nlbac_node_dopri_tile_dense_bwd(const nlbac_mlp* f, const nlbac_mlp* g, const float* u, int n,
                                               const float* beta, int n_out, int max_slots, const double* hslots,
                                               const int* ov_slot, const float* ov_x, const int* nacc, const float* G,
                                               const float* acts_f, long acts_f_ls, const float* acts_g, long acts_g_ls,
                                               int acts_bits, const float* dout, float* dx0, float* du, float* dK,
                                               float* dG, float* dz_f, float* dz_g, nlbac_stream_t s) {
    return tile_dense_bwd("nlbac_node_dopri_tile_dense_bwd", f, g, u, n, beta, n_out, nullptr, max_slots, hslots, ov_slot,
                          ov_x, nacc, G, acts_f, acts_f_ls, acts_g, acts_g_ls, acts_bits, dout, dx0, du, dK, dG, dz_f, dz_g, s);
}

extern "C" int nlbac_node_dopri_tile_dense_paged_bwd(const nlbac_mlp* f, const nlbac_mlp* g, const float* u, int n,
                                                     const float* beta, int n_out, const int* page0, int pages,
                                                     const double* hslots, const int* ov_slot, const float* ov_x,
                                                     const int* nacc, const float* G, const float* acts_f,
                                                     long acts_f_ls, const float* acts_g, long acts_g_ls, int acts_bits,
                                                     const float* dout, float* dx0, float* du, float* dK, float* dG,
                                                     float* dz_f, float* dz_g, nlbac_stream_t s) {
    const char* who = "nlbac_node_dopri_tile_dense_paged_bwd";
    NLBAC_REQUIRE(page0, "%s: null page0", who);
    return tile_dense_bwd(who, f, g, u, n, beta, n_out, page0, pages, hslots, ov_slot, ov_x, nacc, G, acts_f, acts_f_ls,
                          acts_g, acts_g_ls, acts_bits, dout, dx0, du, dK, dG, dz_f, dz_g, s);
}
