// The launch descriptor shared by the MLP kernel families (mlp_kernels.hip: LDS-tiled; mlp_rr_kernels.hip:
// register-resident panels), and the rule by which a launch gets one of them.
#pragma once
#include "common.h"
#include "dy_heads.h"
#include "rr_device.h"

// Rows per chunk of the skinny-gradient partial sums that nlbac_mlp_bwd_data leaves for nlbac_mlp_bwd_weights
// (nlbac_mlp_io::skinny_ws): the finest tile of the data-backward kernels — the 32-row kernels write two chunks per tile.
#define NLBAC_SK_CHUNK 16

struct MlpLaunch {
    nlbac_mlp net[NLBAC_MAX_NETS];
    nlbac_mlp_io io[NLBAC_MAX_NETS];
    int B;
    int ld;          // LDS row stride in floats
    int n_slabs;     // bwd_weights only
    int rows_per_slab;
    long slab_stride;
};

// ---- which kernel family serves a launch: one rule, read by nlbac_mlp_pack_layout, nlbac_mlp_masks_ok,
//      nlbac_mlp_fwd_head_ok and the forward / data-backward launchers (mlp_kernels.hip)
enum MlpFamily {
    MLP_TILED,              // mlp_kernels.hip: 32-row tiles through LDS, the 32x32x2 packs
    MLP_HALF_PANEL,         // mlp_rr_kernels.hip: register-resident, 32-row workgroups, hid = 64
    MLP_QUARTER_PANEL       // mlp_rrq_kernels.hip: register-resident, 16-row workgroups, hid = 128 / 256
};

#define MLP_PANEL_MAX_IN 15       /* in_dim + the bias column <= 16: four k-steps of layer 0 */

// The shapes whose every launch — forward and data backward — runs on the register-resident panel kernels: one
// hid x hid layer of 64 / 128 / 256 units between skinny ends.  Their 32x32x2 packs are never read, so
// nlbac_mlp_pack_layout leaves them out (and the optimiser has half as many fragment slots to refresh per weight).
static inline bool mlp_panel_shape(int n_layers, int in_dim, int hid, int out_dim) {
    return n_layers == 3 && (hid == 64 || hid == 128 || hid == 256) && in_dim <= MLP_PANEL_MAX_IN && out_dim <= 16;
}

// The family of one launch: the panel kernels take nets of a panel shape, all of one width, whose fragments are packed.
// (A launch that mixes widths is MLP_TILED, and the tiled launchers refuse a net that has no packs.)
static inline MlpFamily mlp_family(const nlbac_mlp* nets, int n_nets) {
    for (int i = 0; i < n_nets; ++i) {
        const nlbac_mlp& n = nets[i];
        if (!mlp_panel_shape(n.n_layers, n.in_dim, n.hid, n.out_dim) || n.hid != nets[0].hid) return MLP_TILED;
        if (n.rr_kind != RR_KIND_PANEL || n.rr_fwd_off < 0) return MLP_TILED;
    }
    return nets[0].hid == 64 ? MLP_HALF_PANEL : MLP_QUARTER_PANEL;
}

// What the two panel data backwards read off a launch's io: skinny-gradient partials wanted, an output layer wider than
// four, ReLU mask words in place of the activation rows (for all nets or for none).  0, or < 0 = error.
struct MlpBwdFacts {
    bool sk, wide_out, bits;
};
static inline int mlp_bwd_facts(MlpBwdFacts& F, const MlpLaunch& L, int n_nets, const char* who) {
    int n_bits = 0;
    F.sk = F.wide_out = false;
    for (int i = 0; i < n_nets; ++i) {
        F.sk = F.sk || (L.io[i].skinny_ws != nullptr && L.io[i].dz != nullptr);
        F.wide_out = F.wide_out || L.net[i].out_dim > 4;
        n_bits += L.io[i].masks != nullptr;
    }
    NLBAC_REQUIRE(n_bits == 0 || n_bits == n_nets, "%s: ReLU mask words (nlbac_mlp_io::masks) for all nets of a launch or for none", who);
    F.bits = n_bits != 0;
    return 0;
}

// The panel launchers, for a launch of their family (mlp_family): 0 = launched, < 0 = error.
int nlbac_mlp_rr_fwd_launch(const MlpLaunch& L, int n_nets, const nlbac_gauss_head& G, const char* who, hipStream_t s);
int nlbac_mlp_rr_bwd_launch(const MlpLaunch& L, int n_nets, const nlbac_dy_head& H, const char* who, hipStream_t s);
int nlbac_mlp_rrq_fwd_launch(const MlpLaunch& L, int n_nets, const nlbac_gauss_head& G, const char* who, hipStream_t s);
int nlbac_mlp_rrq_bwd_launch(const MlpLaunch& L, int n_nets, const nlbac_dy_head& H, const char* who, hipStream_t s);

// The one-launch weight/bias gradients of narrow nets (mlp_dw16_kernels.hip: every net at most 112 wide).
bool nlbac_mlp_dw16_eligible(const nlbac_mlp* nets, int n_nets, int B);
int nlbac_mlp_dw16_launch(const MlpLaunch& L, int n_nets, hipStream_t s);
