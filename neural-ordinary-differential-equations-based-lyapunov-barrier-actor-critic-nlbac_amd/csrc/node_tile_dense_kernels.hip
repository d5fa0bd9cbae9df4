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

static int tile_dense_check(const nlbac_mlp* f, const nlbac_mlp* g, int n, int n_out, const float* beta, int max_slots,
                            bool keep, int acts_bits, const char* who) {
    NLBAC_REQUIRE(f && g && beta, "%s: null pointer", who);
    NLBAC_REQUIRE(nlbac_node_dopri_tile_ok(f, g), "%s: these nets do not run on the register-resident kernels (nlbac_node_dopri_tile_ok)", who);
    NLBAC_REQUIRE(n >= 1 && n_out >= 1 && (long)n_out * n < (1L << 31), "%s: bad rows / output times", who);
    NLBAC_REQUIRE(acts_bits >= 0 && acts_bits <= 2, "%s: acts_bits is 0, 1 or 2", who);
    if (keep)
        NLBAC_REQUIRE(max_slots >= 1 && (long)max_slots * 7 * n < (1L << 31),
                      "%s: max_slots must be at least 1, and max_slots * 7 * n below 2^31", who);
    return 0;
}

// One launch: a dense dopri5 solve of every 32-row tile of the n rows over [0, t_end], read at tau [n_out] (DEVICE
// doubles, increasing, tau[n_out - 1] == t_end).  x0 [n][n_s], u [n][n_u], out [n_out][n][n_s].  accepted / attempts /
// status [tiles] (zero on entry) receive each tile's counts and TILE_* status; a tile that stops writes NaN into its rows
// of the outputs it has not emitted.  G non-null: a backward follows — the kept buffers of nlbac_node_dopri_tile_fwd
// (max_slots slots per tile, zero on entry), and ov_slot / ov_x [tiles][n_out]: the slot that emitted output j and its
// abscissa.  G null: nothing is kept and no slot runs out.
extern "C" int nlbac_node_dopri_tile_dense_fwd(const nlbac_mlp* f, const nlbac_mlp* g, const float* x0, const float* u,
                                               int n, const float* beta, const float* c_err, const double* tau, int n_out,
                                               double t_end, float rtol, float atol, float* out, int max_slots, float* Y,
                                               float* G, float* acts_f, long acts_f_ls, float* acts_g, long acts_g_ls,
                                               int acts_bits, double* hslots, int* ov_slot, float* ov_x, int* accepted,
                                               int* attempts, int* status, nlbac_stream_t s) {
    static const NodeRrTable<NodeTileDenseFwdLaunch> table = NODE_RR_FWD_TABLE(node_tile_dense_fwd_kernel);
    const char* who = "nlbac_node_dopri_tile_dense_fwd";
    const bool keep = G != nullptr;
    if (tile_dense_check(f, g, n, n_out, beta, max_slots, keep, acts_bits, who)) return -1;
    NLBAC_REQUIRE(x0 && u && out && c_err && tau && accepted && attempts && status, "%s: null pointer", who);
    NLBAC_REQUIRE(t_end > 0.0 && t_end <= 3.0e38 && rtol >= 0.f && atol >= 0.f && rtol + atol > 0.f, "%s: bad interval / tolerances", who);
    NLBAC_REQUIRE((acts_f == nullptr) == (acts_g == nullptr), "%s: acts_f and acts_g go together", who);
    NLBAC_REQUIRE(keep ? (acts_f && hslots && ov_slot && ov_x) : (!acts_f && !Y), "%s: G, the acts and the slot arrays go together", who);
    NodeTileDenseFwdLaunch A;
    memset(&A, 0, sizeof(A));
    NodeRkLaunch& L = A.L;
    L.net[0] = *f; L.net[1] = *g;
    L.y0 = x0; L.u = u;
    L.n = n; L.rpp = n; L.n_s = f->in_dim; L.n_u = g->out_dim / f->in_dim;
    L.stage_begin = 0; L.stage_end = 7; L.S_total = 7;
    for (int i = 0; i < 7; ++i) {
        for (int j = 0; j < 7; ++j) L.beta[i][j] = beta[i * 7 + j];
        L.c_err[i] = c_err[i];
    }
    L.n_err = 7;
    L.Y = Y; L.G = G;
    L.acts[0] = acts_f; L.acts[1] = acts_g; L.acts_ls[0] = acts_f_ls; L.acts_ls[1] = acts_g_ls;
    L.acts_bits = acts_bits;
    L.out = out;
    L.norm_mode = -1;
    L.rtol = rtol; L.atol = atol; L.t_end = t_end;
    A.X.H = 1; A.X.keep = keep ? 1 : 0; A.X.max_slots = keep ? max_slots : 1;
    A.X.hslots = hslots;
    A.X.accepted = accepted; A.X.attempts = attempts; A.X.status = status;
    A.D.tau = tau; A.D.n_out = n_out; A.D.ov_slot = ov_slot; A.D.ov_x = ov_x;
    node_rr_start(table, A, f->hid, n, acts_bits, node_tile_fwd_lds_floats(), (hipStream_t)s);
    NLBAC_CHECK_LAUNCH(who);
    return 0;
}

// One launch: the backward of the solve nlbac_node_dopri_tile_dense_fwd kept, every tile's slots last to first.
// nacc [tiles]: the forward's `accepted`.  dout [n_out][n][n_s]: the gradients of the outputs 1 .. n_out; dx0 [n][n_s]
// (slot 0's dy0 — the gradient of out[0] is the caller's to add), du [n][n_u]; dK / dG / dz_* (all or none; zero on
// entry) per (slot, stage, row) for the weight gradients.  Only tiles whose status is TILE_OK have a backward: the
// caller reads status first.  What is read of nacc / ov_slot is clamped to the slots and the outputs.
extern "C" int nlbac_node_dopri_tile_dense_bwd(const nlbac_mlp* f, const nlbac_mlp* g, const float* u, int n,
                                               const float* beta, int n_out, int max_slots, const double* hslots,
                                               const int* ov_slot, const float* ov_x, const int* nacc, const float* G,
                                               const float* acts_f, long acts_f_ls, const float* acts_g, long acts_g_ls,
                                               int acts_bits, const float* dout, float* dx0, float* du, float* dK,
                                               float* dG, float* dz_f, float* dz_g, nlbac_stream_t s) {
    static const NodeRrTable<NodeTileDenseBwdLaunch> table = NODE_RR_BWD_TABLE(node_tile_dense_bwd_kernel);
    const char* who = "nlbac_node_dopri_tile_dense_bwd";
    if (tile_dense_check(f, g, n, n_out, beta, max_slots, true, acts_bits, who)) return -1;
    NLBAC_REQUIRE(u && hslots && ov_slot && ov_x && nacc && G && acts_f && acts_g && dout && dx0 && du, "%s: null pointer", who);
    NLBAC_REQUIRE((dz_f == nullptr) == (dz_g == nullptr) && (dz_f == nullptr) == (dG == nullptr) &&
                      (dz_f == nullptr) == (dK == nullptr), "%s: dz_f, dz_g, dG and dK go together", who);
    NLBAC_REQUIRE(!(acts_bits == 1 && dz_f), "%s: weight gradients need the activations, not bit masks", who);
    NodeTileDenseBwdLaunch A;
    memset(&A, 0, sizeof(A));
    NodeRkBwdLaunch& L = A.L;
    L.net[0] = *f; L.net[1] = *g;
    L.u = u; L.G = G;
    L.acts[0] = acts_f; L.acts[1] = acts_g; L.acts_ls[0] = acts_f_ls; L.acts_ls[1] = acts_g_ls;
    L.acts_bits = acts_bits;
    L.dz[0] = dz_f; L.dz[1] = dz_g; L.dG = dG; L.dK = dK;
    L.du = du;
    L.n = n; L.rpp = n; L.n_s = f->in_dim; L.n_u = g->out_dim / f->in_dim;
    L.S_total = 7; L.st_lo = 0; L.st_hi = 7; L.dx_stage0 = 1;
    for (int i = 0; i < 7; ++i)
        for (int j = 0; j < 7; ++j) L.beta[i][j] = beta[i * 7 + j];
    A.X.H = 1; A.X.max_slots = max_slots;
    A.X.hslots = hslots; A.X.iv_nacc = nacc;
    A.X.dout = dout; A.X.dx0 = dx0;
    A.D.n_out = n_out; A.D.ov_slot = ov_slot; A.D.ov_x = ov_x;
    node_rr_start(table, A, f->hid, n, acts_bits, node_rr_bwd_lds_floats(), (hipStream_t)s);
    NLBAC_CHECK_LAUNCH(who);
    return 0;
}
