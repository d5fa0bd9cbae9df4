// Host side of a dopri5 launch under tile-local step control: what the entry points of node_tile_kernels.hip (a rollout's
// horizon) and node_tile_dense_kernels.hip (one dense solve read at a time grid) check and fill alike.  Both launch
// structs open with the RK launch `L` and the tile block `X` (node_rk_shared.h); the fills below write those two and
// nothing else, so what a tile launch carries is described once.  What differs between the two comes in as arguments:
//   H       the intervals a tile solves (the rollout's H; 1 for the dense solve) — X.H, and the least max_slots when
//           steps are kept, since every interval takes a slot at least (`least`: how the message names that number);
//   n_out   the outputs per row (H; the dense solve's n_out), `outputs` their noun in the message.
//   page0   null: every tile has `slots` = max_slots slots; given (the *_paged_* entry points): the slots are counted per
//           tile, page0 [tiles + 1] (DEVICE ints: never read here) the exclusive prefix sum of the tiles' counts and
//           `slots` the pages of all tiles together — the slot check takes that total.
// An entry point keeps the requires and fields of the arrays only it has (iv_first / iv_x; tau / ov_slot / ov_x), behind
// the fill.  Included behind node_rr_body.h; host code only.
#pragma once

static int tile_check(const nlbac_mlp* f, const nlbac_mlp* g, int n, int H, int n_out, const char* outputs,
                      const char* least, const float* beta, const int* page0, int max_slots, bool keep, int acts_bits,
                      const char* who) {
    NLBAC_REQUIRE(f && g && beta, "%s: null pointer", who);
    NLBAC_REQUIRE(nlbac_node_dopri_tile_ok(f, g), "%s: these nets do not run on the register-resident kernels (nlbac_node_dopri_tile_ok)", who);
    NLBAC_REQUIRE(n >= 1 && n_out >= 1 && (long)n_out * n < (1L << 31), "%s: bad rows / %s", who, outputs);
    NLBAC_REQUIRE(acts_bits >= 0 && acts_bits <= 2, "%s: acts_bits is 0, 1 or 2", who);
    if (keep && page0)
        NLBAC_REQUIRE(max_slots >= (long)H * nlbac_ceil_div(n, NLBAC_MLP_TILE) &&
                          (long)max_slots * 7 * NLBAC_MLP_TILE < (1L << 31),
                      "%s: pages must be at least %s for every tile, and pages * 7 * 32 below 2^31", who, least);
    else if (keep)
        NLBAC_REQUIRE(max_slots >= H && (long)max_slots * 7 * n < (1L << 31),
                      "%s: max_slots must be at least %s, and max_slots * 7 * n below 2^31", who, least);
    return 0;
}

// The forward: all 7 stages of dopri5 (beta [7][7], c_err [7]: its table and error weights) on the interval [0, t_end]
// under rtol / atol, the step control the tile's own (norm_mode -1).  G non-null: a backward follows — every accepted
// step is kept in a slot of max_slots per tile (G, the acts, Y for weight gradients, hslots; page0 given: in a page of
// the tile's own, max_slots pages in all); G null: nothing is kept and one slot is worked in.  accepted / attempts / status receive the tiles' counts and TILE_* status.
static int tile_fill_fwd(NodeRkLaunch& L, NodeTileFwd& X, const char* who, int H, int n_out, const char* outputs,
                         const char* least, const nlbac_mlp* f, const nlbac_mlp* g, const float* x0, const float* u,
                         int n, const float* beta, const float* c_err, double t_end, float rtol, float atol, float* out,
                         const int* page0, int max_slots, float* Y, float* G, float* acts_f, long acts_f_ls, float* acts_g, long acts_g_ls,
                         int acts_bits, double* hslots, int* accepted, int* attempts, int* status) {
    const bool keep = G != nullptr;
    if (tile_check(f, g, n, H, n_out, outputs, least, beta, page0, max_slots, keep, acts_bits, who)) return -1;
    NLBAC_REQUIRE(x0 && u && out && c_err && accepted && attempts && status, "%s: null pointer", who);
    NLBAC_REQUIRE(t_end > 0.0 && t_end <= 3.0e38 && rtol >= 0.f && atol >= 0.f && rtol + atol > 0.f, "%s: bad interval / tolerances", who);
    NLBAC_REQUIRE((acts_f == nullptr) == (acts_g == nullptr), "%s: acts_f and acts_g go together", who);
    NLBAC_REQUIRE(keep ? (acts_f && hslots) : (!acts_f && !Y), "%s: G, the acts and the slot arrays go together", who);
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
    X.H = H; X.keep = keep ? 1 : 0; X.max_slots = keep ? max_slots : 1;
    X.page0 = keep ? page0 : nullptr;
    X.hslots = hslots;
    X.accepted = accepted; X.attempts = attempts; X.status = status;
    return 0;
}

// The backward of what tile_fill_fwd's launch kept, every tile's slots last to first: nacc the forward's `accepted`,
// dK / dG / dz_* (all or none) per (slot, stage, row) for the weight gradients.
static int tile_fill_bwd(NodeRkBwdLaunch& L, NodeTileBwd& X, const char* who, int H, int n_out, const char* outputs,
                         const char* least, const nlbac_mlp* f, const nlbac_mlp* g, const float* u, int n,
                         const float* beta, const int* page0, int max_slots, const double* hslots, const int* nacc, const float* G,
                         const float* acts_f, long acts_f_ls, const float* acts_g, long acts_g_ls, int acts_bits,
                         const float* dout, float* dx0, float* du, float* dK, float* dG, float* dz_f, float* dz_g) {
    if (tile_check(f, g, n, H, n_out, outputs, least, beta, page0, max_slots, true, acts_bits, who)) return -1;
    NLBAC_REQUIRE(u && hslots && nacc && G && acts_f && acts_g && dout && dx0 && du, "%s: null pointer", who);
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
    L.S_total = 7; L.st_lo = 0; L.st_hi = 7; L.dx_stage0 = 1;
    for (int i = 0; i < 7; ++i)
        for (int j = 0; j < 7; ++j) L.beta[i][j] = beta[i * 7 + j];
    X.H = H; X.max_slots = max_slots; X.page0 = page0;
    X.hslots = hslots; X.iv_nacc = nacc;
    X.dout = dout; X.dx0 = dx0;
    return 0;
}
