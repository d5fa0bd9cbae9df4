// Fused Runge-Kutta step of the single-net NODE  dx/dt = net([x | c])  (SimulatedCars: C/sac_cbf_clf/model.py:179-205,
// odeint call sites C/sac_cbf_clf/sac_cbf_clf.py:437,458,581,603 and C/model.py:245; the Quadrotor-like task's
// normalised form) with REGISTER-RESIDENT layer chains (rr_device.h): the launches of nlbac_concat_rk_fwd / _bwd for
// the reference's depth (in -> hid -> hid -> hid -> out) and widths 64 / 100 / 128.
//
// One wave owns 16 rows for the whole launch — every stage's input, the net's four products and the stage algebra — so
// nothing is exchanged between waves: no barrier inside the stage loop (the LDS arrays of a wave's rows are private to
// it), a workgroup is just two such waves on one 32-row tile of the problem bookkeeping.  The LDS-tiled kernels give a
// 64-wide layer's two column tiles to two of a group's four waves (concat_rk_fwd 22 TFLOP/s, profiles/r02_bench_variant_cars.json).
// The kernels' bodies are in concat_rr_body.h, shared with the one-launch rollout (concat_traj_kernels.hip).
#include "concat_rr_body.h"

template <int NB, int R, int BITS, int NW>
__global__ __launch_bounds__(64 * NW) void concat_rr_fwd_kernel(const ConcatRkLaunch L) {
    concat_rr_fwd_body<NB, R, BITS, NW>(L);
}

template <int NB, int R, int BITS, int NW>
__global__ __launch_bounds__(64 * NW) void concat_rr_bwd_kernel(const ConcatRkBwdLaunch L) {
    concat_rr_bwd_body<NB, R, BITS, NW>(L);
}

// ---------------------------------------------------------------------------------------------------------------------
bool nlbac_concat_rr_eligible(const nlbac_mlp* np) {
    const nlbac_mlp& net = *np;
    return net.n_layers == 4 && crr_shape_index(net.hid) >= 0 && net.rr_kind == RR_KIND_CHAIN &&
           net.rr_fwd_off >= 0 && net.rr_bwd_off >= 0 && net.in_dim <= CRR_MAX_IN && net.out_dim <= CK_NS;
}

// which instance, how many waves and how much LDS: concat_rr_body.h's host section, shared with the trajectory launchers
int nlbac_concat_rr_fwd_launch(ConcatRkLaunch& L, hipStream_t s) {
    if (!nlbac_concat_rr_eligible(&L.net)) return 1;
    static const ConcatRrTable<ConcatRkLaunch> table[2] = {CONCAT_RR_TABLE(concat_rr_fwd_kernel, 2),
                                                           CONCAT_RR_TABLE(concat_rr_fwd_kernel, 4)};
    const int nw = crr_waves(L.n, L.rpp);
    crr_start(table[nw == 4], nw, L, L.net.hid, L.n, L.acts_bits, crr_fwd_lds, s);
    NLBAC_CHECK_LAUNCH("nlbac_concat_rk_fwd(rr)");
    return 0;
}

int nlbac_concat_rr_bwd_launch(ConcatRkBwdLaunch& L, hipStream_t s) {
    if (!nlbac_concat_rr_eligible(&L.net)) return 1;
    static const ConcatRrTable<ConcatRkBwdLaunch> table[2] = {CONCAT_RR_TABLE(concat_rr_bwd_kernel, 2),
                                                              CONCAT_RR_TABLE(concat_rr_bwd_kernel, 4)};
    const int nw = crr_waves(L.n, L.rpp);
    crr_start(table[nw == 4], nw, L, L.net.hid, L.n, L.acts_bits, crr_bwd_lds, s);
    NLBAC_CHECK_LAUNCH("nlbac_concat_rk_bwd(rr)");
    return 0;
}
