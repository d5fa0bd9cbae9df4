// Continuous adjoint of the single-net NODE  dx/dt = out_mu + out_sig * net(([x | c] - in_mu) * in_isig)  (SimulatedCars,
// C/sac_cbf_clf/model.py:179-205, under torchdiffeq 0.2.3's OdeintAdjointMethod; the Quadrotor-like task's normalised
// form): ONE launch per attempted RK step of the augmented system
//     z = [ y (n_s) | a_y (n_s) | a_c (n_c) ],  W = 2 n_s + n_c,  integrated in s = t1 - t:
//     dy/ds = -f(y, c),   da_y/ds = (df/dy)^T a_y,   da_c/ds = (df/dc)^T a_y
// — nlbac_concat_adj_step.  It replaces, per stage, the five launches nlbac_rk_combine -> nlbac_concat_adj_in ->
// nlbac_mlp_fwd -> nlbac_mlp_bwd_data -> nlbac_concat_adj_out (ode_kernels.hip; kept as the path of other shapes and as
// the cross-check) — about thirty launches per attempted dopri5 step — for the reference's depth (in -> hid -> hid -> hid
// -> out) at widths 64 / 100 / 128.
//
// Wave roles as concat_rr_kernels.hip: one wave owns 16 rows for the whole launch, two waves per workgroup, no barrier
// inside the stage loop.  A stage is ONE uninterrupted MFMA stream per wave (the scheme of node_adj_rr_kernels.hip):
//     layer 0 -> two hid x hid layers -> output layer  (forward pack)  |  top product -> two hid x hid products -> dX  (backward pack)
// the weight queue turns from the forward pack to the backward pack and back without draining, and the ReLU masks the
// backward half gates with stay in three registers.  The stage derivatives of z live in LDS across the stages; what a
// launch leaves in memory is written in one burst at its end.  KEEP (the NODE fit's parameter quadrature): the net's
// normalised inputs, the cotangent of its output, the activations and the pre-activation gradients of every evaluated
// stage additionally go out as rows, for nlbac_mlp_bwd_weights.
// (The kernel template is concat_adj_rr_body.h, which the trajectory form concat_adj_traj_kernels.hip shares.)
#include "concat_adj_rr_body.h"

// ---------------------------------------------------------------------------------------------------------------------
extern "C" int nlbac_concat_adj_step_ok(const nlbac_mlp* net) {
    return (net && nlbac_concat_rr_eligible(net) && net->in_dim <= CADJ_MAX_IN) ? 1 : 0;
}

extern "C" int nlbac_concat_adj_step(const nlbac_mlp* net, const float* c, int P, int rows_per_problem, int st_lo, int st_hi,
                                     int n_stages_total, const float* beta, const float* c_out, int n_out,
                                     const float* c_err, int n_err, const float* h_host, const double* h_dev,
                                     int h_dev_stride, const double* ctl, const float* Z0, float* KZ, float* Z1, float* ERR,
                                     const float* norm, float* Xin, float* Ay, float* acts, long acts_ls, float* dz,
                                     float* interp_out, double t_end, nlbac_stream_t s) {
    NLBAC_REQUIRE(net && P >= 1 && P <= 8 && rows_per_problem >= 1, "nlbac_concat_adj_step: bad problem sizes");
    NLBAC_REQUIRE(nlbac_concat_adj_step_ok(net),
                  "nlbac_concat_adj_step: the net is not in -> hid -> hid -> hid -> out with hid in {64, 100, 128} "
                  "(nlbac_concat_adj_step_ok; other shapes run stage by stage: nlbac_concat_adj_in / _out)");
    NLBAC_REQUIRE(n_stages_total >= 1 && n_stages_total <= CK_MAX_STAGES && st_lo >= 0 && st_lo < st_hi &&
                      st_hi <= n_stages_total, "nlbac_concat_adj_step: bad stage range");
    NLBAC_REQUIRE(c && Z0 && KZ && beta, "nlbac_concat_adj_step: null pointer");
    NLBAC_REQUIRE(h_dev || h_host, "nlbac_concat_adj_step: no step size");
    NLBAC_REQUIRE(n_out <= n_stages_total && n_err <= n_stages_total && (!Z1 || c_out) && (!ERR || c_err),
                  "nlbac_concat_adj_step: bad coefficient counts");
    const bool keep = Xin != nullptr;
    NLBAC_REQUIRE(keep ? (Ay && acts && dz && acts_ls > 0) : (!Ay && !acts && !dz),
                  "nlbac_concat_adj_step: Xin / Ay / acts / dz go together");
    ConcatAdjLaunch L;
    memset(&L, 0, sizeof(L));
    L.net = *net;
    L.c = c; L.Z0 = Z0; L.KZ = KZ; L.Z1 = Z1; L.ERR = ERR;
    L.Xin = Xin; L.Ay = Ay; L.acts = acts; L.dz = dz; L.acts_ls = acts_ls;
    L.norm = norm;
    L.n = P * rows_per_problem; L.rpp = rows_per_problem;
    L.n_s = net->out_dim; L.n_c = net->in_dim - net->out_dim;
    NLBAC_REQUIRE(L.n_s >= 1 && L.n_s <= CK_NS && L.n_c >= 0 && L.n_c <= CK_NC, "nlbac_concat_adj_step: net is not [x (<=16) | carried (<=4)] -> dx");
    L.W = 2 * L.n_s + L.n_c;
    L.WP = L.W | 1;                       // odd LDS row stride: the lanes of a quarter hit distinct banks
    L.st_lo = st_lo; L.st_hi = st_hi; L.S_total = n_stages_total;
    for (int i = 0; i < n_stages_total; ++i)
        for (int j = 0; j < n_stages_total; ++j) L.beta[i][j] = beta[i * n_stages_total + j];
    for (int j = 0; j < n_out && c_out; ++j) L.c_out[j] = c_out[j];
    for (int j = 0; j < n_err && c_err; ++j) L.c_err[j] = c_err[j];
    L.n_out = Z1 ? n_out : 0; L.n_err = ERR ? n_err : 0;
    L.h_dev = h_dev; L.h_stride = h_dev_stride;
    for (int p = 0; p < P; ++p) L.h_val[p] = h_host ? h_host[p] : 0.f;
    L.ctl = ctl;
    if (interp_out) {
        NLBAC_REQUIRE(ctl && h_dev && Z1 && st_hi == n_stages_total && n_stages_total == 7,
                      "nlbac_concat_adj_step: interp_out goes with an attempt launch of a device-driven dopri5 solve");
        L.ip_out = interp_out; L.t_end = t_end;
    }
    // four waves per workgroup (rows of done problems are skipped per row, nothing else is per tile: a tile may straddle
    // problems)
    constexpr int nw = 4, tile = 16 * nw;
    using Kernel = void (*)(const ConcatAdjLaunch);
    static const Kernel kt[3][2] = {{concat_adj_rr_kernel<4, 4, 0, nw>, concat_adj_rr_kernel<4, 4, 1, nw>},
                                    {concat_adj_rr_kernel<7, 1, 0, nw>, concat_adj_rr_kernel<7, 1, 1, nw>},
                                    {concat_adj_rr_kernel<8, 4, 0, nw>, concat_adj_rr_kernel<8, 4, 1, nw>}};
    const int shape = net->hid == 64 ? 0 : (net->hid == 100 ? 1 : 2);
    const size_t lds = (size_t)((n_stages_total + 1) * tile * L.WP + tile * (CK_NC + 2) + 2 * 4 * 8 * 64) * sizeof(float);
    const Kernel k = kt[shape][keep ? 1 : 0];
    if (lds > 64 * 1024) {
        static bool attr_set[3][2] = {};
        if (!attr_set[shape][keep ? 1 : 0]) {
            (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 64);
            attr_set[shape][keep ? 1 : 0] = true;
        }
    }
    hipLaunchKernelGGL(k, dim3(nlbac_ceil_div(L.n, tile)), dim3(64 * nw), lds, (hipStream_t)s, L);
    NLBAC_CHECK_LAUNCH("nlbac_concat_adj_step");
    return 0;
}
