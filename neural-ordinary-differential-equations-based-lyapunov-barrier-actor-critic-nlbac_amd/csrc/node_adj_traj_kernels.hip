// Continuous adjoint of the control-affine NODE over a whole horizon in ONE launch: rollout(adjoint=True) and
// odeint_grid(adjoint=True) — torchdiffeq's OdeintAdjointMethod.backward on a grid, for the fixed-step methods.  The stage
// body of nlbac_node_adj_step's register-resident kernel (node_adj_rr_body.h: forward chain and its vector-Jacobian
// product fused per wave, the masks in registers) runs in a loop over a run of fine intervals, last to first; the tile's
// z = [y | a_x | a_u] stays in LDS from the run's top to its end, Z0 <- Z1 included.  Nothing of the forward is read but
// the outputs the caller holds: at every output interval's upper end y is reset to the stored output and the output's
// gradient joins a_x (adj_traj_shared.h).  A run is any number of whole output intervals; the carry buffer hands z from
// run to run, so a horizon may be cut into several launches (the host does when parameter gradients are wanted: KEEP
// writes every stage's rows for ONE nlbac_mlp_bwd_weights launch per run, and that launch has a row limit).
//
// Without KEEP nothing but carry, du (and z's LDS tile) is written.  Per fine interval the arithmetic on z is the
// one-step launch's, operation for operation: the results equal the chain of one-interval adjoint solves bit for bit.
#include "node_adj_rr_body.h"
#include <cstring>

extern "C" int nlbac_node_adj_traj_ok(const nlbac_mlp* f, const nlbac_mlp* g) {
    return (f && g && nlbac_node_rr_eligible(f, g)) ? 1 : 0;
}

extern "C" int nlbac_node_adj_traj(const nlbac_mlp* f, const nlbac_mlp* g, int n, int N, int H, int n_stages,
                                   const float* beta, const float* c_out, const float* hs, const float* hs_host,
                                   const int* begin, const int* begin_host, const float* out, int out_ld,
                                   const float* dout, const float* u, long u_stride, float* du, long du_stride,
                                   float* carry, int top, float* ZS, float* dK, float* dG, float* acts_f, long acts_f_ls,
                                   float* acts_g, long acts_g_ls, float* dz_f, float* dz_g, nlbac_stream_t s) {
    const char* who = "nlbac_node_adj_traj";
    NLBAC_REQUIRE(f && g && beta && c_out && out && dout && u && du && carry, "%s: null pointer", who);
    NLBAC_REQUIRE(nlbac_node_adj_traj_ok(f, g), "%s: these nets do not run on the register-resident adjoint (nlbac_node_adj_traj_ok)", who);
    NLBAC_REQUIRE(n_stages <= ADJ_MAX_STAGES, "%s: bad stage count", who);
    if (nlbac_adj_traj_check(n, N, H, n_stages, hs, hs_host, begin, begin_host, who)) return -1;
    const int ns = f->in_dim, nu = g->out_dim / f->in_dim;
    NLBAC_REQUIRE(out_ld >= ns, "%s: out_ld is narrower than the state", who);
    NLBAC_REQUIRE((u_stride == 0 || u_stride == (long)n * nu) && (du_stride == 0 || du_stride == (long)n * nu),
                  "%s: controls and their gradient are one block per output interval (n * n_u) or one for all (0)", who);
    const bool keep = ZS != nullptr;
    NLBAC_REQUIRE(keep == (dK != nullptr) && keep == (dG != nullptr) && keep == (acts_f != nullptr) &&
                      keep == (acts_g != nullptr) && keep == (dz_f != nullptr) && keep == (dz_g != nullptr),
                  "%s: ZS, dK, dG, acts_f, acts_g, dz_f, dz_g go together", who);
    NodeAdjTrajLaunch A;
    memset(&A, 0, sizeof(A));
    NodeAdjLaunch& L = A;
    L.net[0] = *f; L.net[1] = *g;
    L.ZS = ZS; L.dG = dG;
    L.acts[0] = acts_f; L.acts[1] = acts_g; L.acts_ls[0] = acts_f_ls; L.acts_ls[1] = acts_g_ls;
    L.dz[0] = dz_f; L.dz[1] = dz_g;
    L.n = n; L.rpp = n; L.n_s = ns; L.n_u = nu; L.W = 2 * ns + nu;
    L.st_lo = 0; L.st_hi = n_stages; L.S_total = n_stages;
    nlbac_tableau_copy(L.beta, L.c_out, L.n_out, n_stages, beta, c_out);
    L.ld = L.W | 1;
    AdjTrajArgs& T = A.T;
    T.N = N; T.top = top ? 1 : 0; T.hs = hs; T.begin = begin;
    T.out = out; T.out_ld = out_ld; T.dout = dout;
    T.ctl = u; T.ctl_stride = u_stride; T.du = du; T.du_stride = du_stride;
    T.carry = carry; T.dK = dK;
    using Kernel = void (*)(const NodeAdjTrajLaunch);
    const int hid = f->hid;
    const Kernel k = keep ? (hid == 64 ? node_adj_rr_kernel<4, 4, 1, 1> : (hid == 100 ? node_adj_rr_kernel<7, 1, 1, 1> : node_adj_rr_kernel<8, 4, 1, 1>))
                          : (hid == 64 ? node_adj_rr_kernel<4, 4, 0, 1> : (hid == 100 ? node_adj_rr_kernel<7, 1, 0, 1> : node_adj_rr_kernel<8, 4, 0, 1>));
    // (the one-step launch's LDS layout: nlbac_node_adj_rr_launch)
    const size_t lds = (size_t)((L.S_total + 2) * NLBAC_MLP_TILE * L.ld +
                                NLBAC_MLP_TILE * (ADJ_MAX_NU + 1 + 1 + ADJ_MAX_NS + ADJ_MAX_GOUT + 2 * ADJ_MAX_NS) +
                                2 * 3 * 8 * 64 + 2 * 4 * 8 * 64 + ADJ_MAX_STAGES) * sizeof(float) +
                       sizeof(AdjTrajArgs) + 4 * sizeof(int);      // (+ c_sol, the run's arguments, kcur / du_first)
    hipLaunchKernelGGL(k, dim3(nlbac_ceil_div(n, NLBAC_MLP_TILE)), dim3(256), lds, (hipStream_t)s, A);
    NLBAC_CHECK_LAUNCH(who);
    return 0;
}
