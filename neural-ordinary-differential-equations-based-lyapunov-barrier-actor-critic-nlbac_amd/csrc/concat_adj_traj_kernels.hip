// Continuous adjoint of the single-net NODE over a whole horizon in ONE launch: rollout(adjoint=True) and
// odeint_grid(adjoint=True) for dx/dt = net([x | c]) (normalised or not) — node_adj_traj_kernels.hip's scheme on the stage
// body of nlbac_concat_adj_step (concat_adj_rr_body.h): the stages run in a loop over a run of fine intervals, last to
// first, every wave's 16 rows of z = [y | a_y | a_c] in LDS from the run's top to its end, no barrier inside the run.
// Between the intervals: adj_traj_shared.h.  KEEP writes every stage's net inputs, scaled output cotangents, activations
// and scaled pre-activation gradients for ONE nlbac_mlp_bwd_weights launch per run.
#include "concat_adj_rr_body.h"

extern "C" int nlbac_concat_adj_step_ok(const nlbac_mlp* net);      // (concat_adj_rr_kernels.hip)

extern "C" int nlbac_concat_adj_traj_ok(const nlbac_mlp* net) {
    return nlbac_concat_adj_step_ok(net);
}

extern "C" int nlbac_concat_adj_traj(const nlbac_mlp* net, int n, int N, int H, int n_stages, const float* beta,
                                     const float* c_out, const float* hs, const float* hs_host, const int* begin,
                                     const int* begin_host, const float* out, int out_ld, const float* dout,
                                     const float* c, long c_stride, float* dc, long dc_stride, float* carry, int top,
                                     const float* norm, float* Xin, float* Ay, float* acts, long acts_ls, float* dz,
                                     nlbac_stream_t s) {
    const char* who = "nlbac_concat_adj_traj";
    NLBAC_REQUIRE(net && beta && c_out && out && dout && c && dc && carry, "%s: null pointer", who);
    NLBAC_REQUIRE(nlbac_concat_adj_traj_ok(net), "%s: this net does not run on the register-resident adjoint (nlbac_concat_adj_traj_ok)", who);
    NLBAC_REQUIRE(n_stages <= CK_MAX_STAGES, "%s: bad stage count", who);
    if (nlbac_adj_traj_check(n, N, H, n_stages, hs, hs_host, begin, begin_host, who)) return -1;
    const int ns = net->out_dim, nc = net->in_dim - net->out_dim;
    NLBAC_REQUIRE(ns >= 1 && ns <= CK_NS && nc >= 0 && nc <= CK_NC, "%s: net is not [x (<=16) | carried (<=4)] -> dx", who);
    NLBAC_REQUIRE(out_ld >= ns, "%s: out_ld is narrower than the state", who);
    NLBAC_REQUIRE((c_stride == 0 || c_stride == (long)n * nc) && (dc_stride == 0 || dc_stride == (long)n * nc),
                  "%s: carried inputs and their gradient are one block per output interval (n * n_c) or one for all (0)", who);
    const bool keep = Xin != nullptr;
    NLBAC_REQUIRE(keep ? (Ay && acts && dz && acts_ls > 0) : (!Ay && !acts && !dz), "%s: Xin / Ay / acts / dz go together", who);
    ConcatAdjTrajLaunch A;
    memset(&A, 0, sizeof(A));
    ConcatAdjLaunch& L = A;
    L.net = *net;
    L.Xin = Xin; L.Ay = Ay; L.acts = acts; L.dz = dz; L.acts_ls = acts_ls;
    L.norm = norm;
    L.n = n; L.rpp = n; L.n_s = ns; L.n_c = nc;
    L.W = 2 * ns + nc;
    L.WP = L.W | 1;
    L.st_lo = 0; L.st_hi = n_stages; L.S_total = n_stages;
    nlbac_tableau_copy(L.beta, L.c_out, L.n_out, n_stages, beta, c_out);
    AdjTrajArgs& T = A.T;
    T.N = N; T.top = top ? 1 : 0; T.hs = hs; T.begin = begin;
    T.out = out; T.out_ld = out_ld; T.dout = dout;
    T.ctl = c; T.ctl_stride = c_stride; T.du = dc; T.du_stride = dc_stride;
    T.carry = carry;
    constexpr int nw = 4, tile = 16 * nw;       // (as nlbac_concat_adj_step)
    using Kernel = void (*)(const ConcatAdjTrajLaunch);
    static const Kernel kt[3][2] = {{concat_adj_rr_kernel<4, 4, 0, nw, 1>, concat_adj_rr_kernel<4, 4, 1, nw, 1>},
                                    {concat_adj_rr_kernel<7, 1, 0, nw, 1>, concat_adj_rr_kernel<7, 1, 1, nw, 1>},
                                    {concat_adj_rr_kernel<8, 4, 0, nw, 1>, concat_adj_rr_kernel<8, 4, 1, nw, 1>}};
    const int shape = net->hid == 64 ? 0 : (net->hid == 100 ? 1 : 2);
    // the one-step launch's LDS layout + c_sol, the run's arguments, kcur / du_first per wave
    const size_t lds = (size_t)((n_stages + 1) * tile * L.WP + tile * (CK_NC + 2) + 2 * 4 * 8 * 64 + CK_MAX_STAGES) * sizeof(float) +
                       sizeof(AdjTrajArgs) + 2 * nw * sizeof(int);
    const Kernel k = kt[shape][keep ? 1 : 0];
    if (lds > 64 * 1024) {
        static bool attr_set[3][2] = {};
        if (!attr_set[shape][keep ? 1 : 0]) {
            (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 64);
            attr_set[shape][keep ? 1 : 0] = true;
        }
    }
    hipLaunchKernelGGL(k, dim3(nlbac_ceil_div(n, tile)), dim3(64 * nw), lds, (hipStream_t)s, A);
    NLBAC_CHECK_LAUNCH(who);
    return 0;
}
