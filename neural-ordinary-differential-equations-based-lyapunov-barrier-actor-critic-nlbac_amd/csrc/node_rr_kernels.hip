// Fused Runge-Kutta step of the control-affine NODE on the register-resident layer chains: the kernels and their host
// side.  What they run — one 32-row tile per workgroup, four waves, one (net, 16 rows) chain per wave — is
// node_rr_body.h, shared with the one-launch trajectory kernels (node_traj_kernels.hip).
#include "node_rr_body.h"

#ifdef RR_TIMING
extern "C" int nlbac_debug_bwd_stamps(long long* out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_bwd_stamps), sizeof(long long) * 2 * 256) == hipSuccess ? 0 : -1;
}
#endif

template <int NB, int R, int BITS, int SPLIT>
__global__ __launch_bounds__(256) void node_rr_fwd_kernel(const NodeRkLaunch L) {
    node_rr_fwd_body<NB, R, BITS, SPLIT>(L);
}

template <int NB, int R, int BITS, int SPLIT>
__global__ __launch_bounds__(256) void node_rr_bwd_kernel(const NodeRkBwdLaunch L) {
    node_rr_bwd_body<NB, R, BITS, SPLIT>(L);
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
int nlbac_node_rr_shape(int hid) { return hid == 64 ? 0 : (hid == 100 ? 1 : (hid == 128 ? 2 : -1)); }

bool nlbac_node_rr_eligible(const nlbac_mlp* f, const nlbac_mlp* g) {
    if (!f || !g) return false;
    if (f->hid != g->hid || nlbac_node_rr_shape(f->hid) < 0) return false;
    if (f->n_layers != 5 || g->n_layers != 4) return false;      // the layer chains are unrolled for the reference's depths
    if (f->rr_fwd_off < 0 || g->rr_fwd_off < 0 || f->rr_bwd_off < 0 || g->rr_bwd_off < 0) return false;
    const int ns = f->in_dim, nu = g->out_dim / (ns > 0 ? ns : 1);
    if (ns < 1 || ns > RK_MAX_NS || nu < 1 || nu > RK_MAX_NU) return false;
    if (((ns + 3) >> 2) * nu > 4) return false;            // g_net's outputs must fit one 16-row output block's registers
    return true;
}

extern "C" int nlbac_node_rk_mask_words(const nlbac_mlp* f, const nlbac_mlp* g, int which) {
    // uint32 words per row and layer of the bit-packed ReLU masks nlbac_node_rk_fwd writes for net `which` (0: f, 1: g)
    if (nlbac_node_rr_eligible(f, g)) return 4;            // one word per lane quarter
    const nlbac_mlp* net = which ? g : f;
    return (net->hid + 31) >> 5;
}

// which instance and how much LDS: node_rr_body.h's host section, shared with the trajectory launchers
int nlbac_node_rr_fwd_launch(NodeRkLaunch& L, hipStream_t s) {
    if (!nlbac_node_rr_eligible(&L.net[0], &L.net[1])) return 1;
    static const NodeRrTable<NodeRkLaunch> table = NODE_RR_FWD_TABLE(node_rr_fwd_kernel);
    node_rr_fwd_start(table, L, L.net[0].hid, L.n, L.acts_bits, s);
    NLBAC_CHECK_LAUNCH("nlbac_node_rk_fwd(rr)");
    return 0;
}

int nlbac_node_rr_bwd_launch(NodeRkBwdLaunch& L, hipStream_t s) {
    if (!nlbac_node_rr_eligible(&L.net[0], &L.net[1])) return 1;
    static const NodeRrTable<NodeRkBwdLaunch> table = NODE_RR_BWD_TABLE(node_rr_bwd_kernel);
    node_rr_bwd_start(table, L, L.net[0].hid, L.n, L.acts_bits, s);
    NLBAC_CHECK_LAUNCH("nlbac_node_rk_bwd(rr)");
    return 0;
}
