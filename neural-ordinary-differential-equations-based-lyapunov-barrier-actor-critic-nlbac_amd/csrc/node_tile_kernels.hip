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

static int tile_check(const nlbac_mlp* f, const nlbac_mlp* g, int n, int H, const float* beta, int max_slots, bool keep,
                      int acts_bits, const char* who) {
    NLBAC_REQUIRE(f && g && beta, "%s: null pointer", who);
    NLBAC_REQUIRE(nlbac_node_dopri_tile_ok(f, g), "%s: these nets do not run on the register-resident kernels (nlbac_node_dopri_tile_ok)", who);
    NLBAC_REQUIRE(n >= 1 && H >= 1 && (long)H * n < (1L << 31), "%s: bad rows / intervals", who);
    NLBAC_REQUIRE(acts_bits >= 0 && acts_bits <= 2, "%s: acts_bits is 0, 1 or 2", who);
    if (keep)
        NLBAC_REQUIRE(max_slots >= H && (long)max_slots * 7 * n < (1L << 31),
                      "%s: max_slots must be at least H, and max_slots * 7 * n below 2^31", who);
    return 0;
}

// One launch: H intervals of dopri5 for every 32-row tile of the n rows.  x0 [n][n_s], u [H][n][n_u], out [H][n][n_s]
// (the state behind every interval), beta [7][7] / c_err [7]: dopri5's table and error weights.  accepted / attempts
// [tiles][H] and status [tiles] (zero on entry) receive the counts and the tiles' TILE_* status.
// G non-null: a backward follows — every accepted step is kept in a slot of max_slots per tile: G [max_slots * 7][n][n_s n_u],
// acts_* / acts_bits as in nlbac_node_rk_traj_fwd over max_slots * 7 stages (zero on entry: a stage nobody evaluated
// must read as zero), Y (weight gradients only, zero on entry) the stage inputs, hslots [tiles][max_slots],
// iv_first / iv_x [tiles][H].  G null: nothing is kept; acts_bits still picks the kernel instance (its sums).
extern "C" int nlbac_node_dopri_tile_fwd(const nlbac_mlp* f, const nlbac_mlp* g, const float* x0, const float* u, int n,
                                         int H, const float* beta, const float* c_err, double dt, float rtol, float atol,
                                         float* out, int max_slots, float* Y, float* G, float* acts_f, long acts_f_ls,
                                         float* acts_g, long acts_g_ls, int acts_bits, double* hslots, int* iv_first,
                                         float* iv_x, int* accepted, int* attempts, int* status, nlbac_stream_t s) {
    static const NodeRrTable<NodeTileFwdLaunch> table = NODE_RR_FWD_TABLE(node_tile_fwd_kernel);
    const char* who = "nlbac_node_dopri_tile_fwd";
    const bool keep = G != nullptr;
    if (tile_check(f, g, n, H, beta, max_slots, keep, acts_bits, who)) return -1;
    NLBAC_REQUIRE(x0 && u && out && c_err && accepted && attempts && status, "%s: null pointer", who);
    NLBAC_REQUIRE(dt > 0.0 && dt <= 3.0e38 && rtol >= 0.f && atol >= 0.f && rtol + atol > 0.f, "%s: bad interval / tolerances", who);
    NLBAC_REQUIRE((acts_f == nullptr) == (acts_g == nullptr), "%s: acts_f and acts_g go together", who);
    NLBAC_REQUIRE(keep ? (acts_f && hslots && iv_first && iv_x) : (!acts_f && !Y), "%s: G, the acts and the slot arrays go together", who);
    NodeTileFwdLaunch A;
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
    L.rtol = rtol; L.atol = atol; L.t_end = dt;
    A.X.H = H; A.X.keep = keep ? 1 : 0; A.X.max_slots = keep ? max_slots : 1;
    A.X.hslots = hslots; A.X.iv_first = iv_first; A.X.iv_x = iv_x;
    A.X.accepted = accepted; A.X.attempts = attempts; A.X.status = status;
    node_rr_start(table, A, f->hid, n, acts_bits, node_tile_fwd_lds_floats(), (hipStream_t)s);
    NLBAC_CHECK_LAUNCH(who);
    return 0;
}

// One launch: the backward of the horizon nlbac_node_dopri_tile_fwd kept, every tile's steps last to first.  iv_nacc: the
// forward's `accepted`.  dout [H+1][n][n_s], dx0 [n][n_s], du [H][n][n_u]; dK / dG / dz_* (all or none; zero on entry) per
// (slot, stage, row) for the weight gradients, as in nlbac_node_rk_traj_bwd.  Only tiles whose status is TILE_OK have a
// backward: the caller reads status first.
extern "C" int nlbac_node_dopri_tile_bwd(const nlbac_mlp* f, const nlbac_mlp* g, const float* u, int n, int H,
                                         const float* beta, int max_slots, const double* hslots, const int* iv_first,
                                         const int* iv_nacc, const float* iv_x, const float* G, const float* acts_f,
                                         long acts_f_ls, const float* acts_g, long acts_g_ls, int acts_bits,
                                         const float* dout, float* dx0, float* du, float* dK, float* dG, float* dz_f,
                                         float* dz_g, nlbac_stream_t s) {
    static const NodeRrTable<NodeTileBwdLaunch> table = NODE_RR_BWD_TABLE(node_tile_bwd_kernel);
    const char* who = "nlbac_node_dopri_tile_bwd";
    if (tile_check(f, g, n, H, beta, max_slots, true, acts_bits, who)) return -1;
    NLBAC_REQUIRE(u && hslots && iv_first && iv_nacc && iv_x && G && acts_f && acts_g && dout && dx0 && du, "%s: null pointer", who);
    NLBAC_REQUIRE((dz_f == nullptr) == (dz_g == nullptr) && (dz_f == nullptr) == (dG == nullptr) &&
                      (dz_f == nullptr) == (dK == nullptr), "%s: dz_f, dz_g, dG and dK go together", who);
    NLBAC_REQUIRE(!(acts_bits == 1 && dz_f), "%s: weight gradients need the activations, not bit masks", who);
    NodeTileBwdLaunch A;
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
    A.X.H = H; A.X.max_slots = max_slots;
    A.X.hslots = hslots; A.X.iv_first = iv_first; A.X.iv_nacc = iv_nacc; A.X.iv_x = iv_x;
    A.X.dout = dout; A.X.dx0 = dx0;
    node_rr_start(table, A, f->hid, n, acts_bits, node_rr_bwd_lds_floats(), (hipStream_t)s);
    NLBAC_CHECK_LAUNCH(who);
    return 0;
}
