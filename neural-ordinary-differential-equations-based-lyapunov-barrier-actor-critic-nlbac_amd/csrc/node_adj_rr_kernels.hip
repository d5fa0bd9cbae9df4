// Continuous adjoint of the control-affine NODE (odeint_adjoint; see node_adjoint_kernels.hip for the mathematics and the
// reference call sites — P/sac_cbf_clf/sac_cbf_clf.py:459,499,534 under torchdiffeq's OdeintAdjointMethod, BASELINE
// configs[3]) with REGISTER-RESIDENT layer chains: the launches of nlbac_node_adj_step for the reference's NODE shapes
// (node_rr_kernels.hip: f_net five layers, g_net four, width 64 / 100 / 128) when nothing but the step's result is kept
// (rollouts: the adjoint of the states and actions; the NODE fit's parameter quadrature stays on the LDS-tiled kernel).
//
// Same wave roles as the fused RK kernels: four waves per 32-row tile, wave = (net, 16 rows).  A stage of the augmented
// state z = [y | a_x | a_u] is, per wave, ONE uninterrupted chain
//     layer 0 -> hid x hid layers -> output layer  (forward pack)  |  top product -> hid x hid products -> dX  (backward pack)
// and the ReLU masks the backward half gates with never leave the wave: one 32-bit word per layer, assembled by the
// forward half in a register (rr_mask_push) and read by the backward half from the same register.  The LDS-tiled kernel
// keeps its masks and activations in LDS tiles, ten layer steps of GEMM + epilogue + barrier per stage: 204 us per
// attempted step at 16384 rows (0.35 of the fp32-MFMA roof).  The stage algebra on z (stage input, k_y = -(f + g u),
// k_au = g^T a_x, k_ax = dX_f + dX_g, step result and error estimate) is the LDS-tiled kernel's, operation for operation.
// (The kernel template is node_adj_rr_body.h, which the trajectory form node_adj_traj_kernels.hip shares.)
#include "node_adj_rr_body.h"

int nlbac_node_adj_rr_launch(NodeAdjLaunch& L, hipStream_t s) {
    if (!nlbac_node_rr_eligible(&L.net[0], &L.net[1])) return 1;
    const bool keep = L.ZS != nullptr;
    using Kernel = void (*)(const NodeAdjLaunch);
    const int hid = L.net[0].hid;
    const Kernel k = keep ? (hid == 64 ? node_adj_rr_kernel<4, 4, 1> : (hid == 100 ? node_adj_rr_kernel<7, 1, 1> : node_adj_rr_kernel<8, 4, 1>))
                          : (hid == 64 ? node_adj_rr_kernel<4, 4, 0> : (hid == 100 ? node_adj_rr_kernel<7, 1, 0> : node_adj_rr_kernel<8, 4, 0>));
    L.ld = L.W | 1;
    const size_t lds = (size_t)((L.S_total + 2) * NLBAC_MLP_TILE * L.ld +
                                NLBAC_MLP_TILE * (ADJ_MAX_NU + 1 + 1 + ADJ_MAX_NS + ADJ_MAX_GOUT + 2 * ADJ_MAX_NS) +
                                2 * 3 * 8 * 64 + 2 * 4 * 8 * 64) * sizeof(float);
    const dim3 grid(nlbac_ceil_div(L.n, NLBAC_MLP_TILE));
    hipLaunchKernelGGL(k, grid, dim3(256), lds, s, L);
    NLBAC_CHECK_LAUNCH("nlbac_node_adj_step(rr)");
    return 0;
}

extern "C" int nlbac_node_adj_interp_ok(const nlbac_mlp* f, const nlbac_mlp* g) {
    return (f && g && nlbac_node_rr_eligible(f, g)) ? 1 : 0;
}
