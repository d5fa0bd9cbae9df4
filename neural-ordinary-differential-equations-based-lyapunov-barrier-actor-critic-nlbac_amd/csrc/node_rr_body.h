// Fused Runge-Kutta step of the control-affine NODE  dx/dt = f(x) + g(x) u  with REGISTER-RESIDENT layer chains
// (rr_device.h): the same launches, arguments and results as node_kernels.hip's LDS-tiled kernels — they are selected
// inside nlbac_node_rk_fwd / nlbac_node_rk_bwd for nets up to 128 units wide — but a 32-row tile is worked on by four
// waves, one per SIMD, each running ONE net's whole layer chain for 16 of the rows:
//     wave 0: f_net rows 0-15    wave 1: f_net rows 16-31    wave 2: g_net rows 0-15    wave 3: g_net rows 16-31
// Per stage a wave issues layer 0, its hid x hid layers and the output layer as one uninterrupted MFMA stream
// (v_mfma_f32_16x16x4_f32, weights streamed from the L2-resident RR pack, bias + ReLU + mask bits applied to the
// accumulators in place); the two nets meet at k = f + g u, through LDS and two workgroup barriers per stage.
// The LDS-tiled kernels spend 34k cycles per stage on a 32-row tile (five layer steps of GEMM + epilogue + barrier, the
// pipe's 16.6k cycles of 128-column / K=104 tiles spread over them, profiles/r02_phase_times_node_rk_fwd.txt); here a
// stage is f_net's three 5.6k-cycle layers + ~2k.
//
// Reference call sites: torchdiffeq.odeint at U/sac_cbf_clf/sac_cbf_clf.py:453,577 and U/sac_cbf_clf/model.py:252
// over NeuralODEModel.forward (model.py:208-217); the backward is what autograd does through the solver's stages.
//
// The bodies below are shared by the one-step kernels (node_rr_kernels.hip) and the one-launch fixed-grid trajectory
// kernels (node_traj_kernels.hip, TRAJ = true: the same stage chain inside a loop over H intervals).
#pragma once
#include "node_rk_shared.h"
#include "rr_device.h"
#include <cstdlib>
#include <type_traits>

// which output the A row hu = 4 q' + r' of the (single) output block computes, so that the result leaves lane (q, row)
// with state component c = 4 r + q in register r (f_net) resp. g[c = 4 ks0 + q][u] in register e = ks0 nu + u (g_net):
// exactly the layout of layer 0's B operand.  -1: padding row.
__device__ __forceinline__ int rr_out_row(int grp, int hu, int ns, int nu) {
    const int qp = hu >> 2, rp = hu & 3, KS0 = (ns + 3) >> 2;
    if (grp == 0) {
        const int c = 4 * rp + qp;
        return (rp < KS0 && c < ns) ? c : -1;
    }
    const int k0 = rp / nu, u = rp - k0 * nu, c = 4 * k0 + qp;
    return (rp < KS0 * nu && c < ns) ? c * nu + u : -1;
}

#ifdef RR_TIMING      // ablation build only: waves 0 (f_net) and 2 (g_net) of workgroup 0 stamp the shader clock into L.err (as int64)
#define RSTAMP(slot_) if (L.err && blockIdx.x == 0 && lane == 0 && half == 0) reinterpret_cast<long long*>(L.err)[grp * 256 + (slot_)] = (long long)__builtin_readcyclecounter();
#else
#define RSTAMP(slot_)
#endif

#define RR_MAX_W 4        /* layer 0 + up to three hid x hid layers (n_layers <= 5: the reference's f_net) */

// Where a kept stage's rows lie, in both bodies: RR_KN rows per stage, the tile's first at RR_KROW0, a lane's own at
// RR_KGROW (RR_KGROWC: clamped to the rows there are) — n, row0, grow and growc, except under TILE, where a paged launch
// (the tile's slots are pages of S stages x 32 rows: NodeTilePlace, node_rk_shared.h) has 32, 0 and the row within the
// tile.  TILE is a template argument: the instances that are not TILE read n / row0 / grow as they always did.
#define RR_KN (TILE ? P.kn : n)
#define RR_KROW0 (TILE ? P.krow0 : row0)
#define RR_KGROW (TILE ? P.krow0 + m : grow)
#define RR_KGROWC (TILE ? min(P.krow0 + m, P.kn - 1) : growc)

// dynamic LDS of the forward / backward bodies, in floats (the carve at the top of each); both are even, so the
// tile-local step control's doubles (TILE: NLBAC_DOPRI_CTL of them and TI_COUNT ints) sit aligned behind them
__host__ __device__ constexpr int node_rr_fwd_lds_floats() {
    return RkFwdTile::floats() + NLBAC_MLP_TILE * 8 + 2 * 3 * 8 * 64 + 2 * 32 * 64 + NLBAC_MLP_TILE * RK_MAX_NS + 2 * 2 * 64 + 4;
}
__host__ __device__ constexpr int node_rr_bwd_lds_floats() {
    return RkBwdTile::floats() + 2 * 4 * 8 * 64 + 2 * 32 * 64 + 2 * 16 * 64 + 4;
}
static_assert(node_rr_fwd_lds_floats() % 2 == 0, "the tile's control block is 8-byte aligned");
__host__ __device__ constexpr int node_tile_fwd_lds_floats() { return node_rr_fwd_lds_floats() + 2 * NLBAC_DOPRI_CTL + TI_COUNT; }

#ifdef RR_TIMING      // ablation build only: the backward's stamps go to a device symbol (nlbac_debug_bwd_stamps reads it back)
__device__ long long g_bwd_stamps[2 * 256];      // (defined in the one translation unit that includes this with RR_TIMING)
#define BWSTAMP(slot_) if (blockIdx.x == 0 && lane == 0 && half == 0) g_bwd_stamps[grp * 256 + (slot_)] = (long long)__builtin_readcyclecounter();
#else
#define BWSTAMP(slot_)
#endif

// SPLIT: f_net has one hid x hid layer more than g_net (U/sac_cbf_clf/model.py:186-206), so its waves ran ~175 MFMAs per
// stage longer and g_net's waited a quarter of every stage at the stage barrier.  With SPLIT the g_net wave of each half
// tile takes over the upper groups of output blocks of f_net's LAST hid x hid layer: the f_net wave hands its layer-2
// activations over through LDS (behind a flag only the two waves touch), both compute their blocks and their part of
// f_net's output layer, and the two partial outputs meet in the stage's k = f + g u step.
// BITS: what the backward gets of each layer — 0 the activation rows, 1 the ReLU mask words instead, 2 both (the NODE
// fit: its backward gates on the words, the weight gradients read the rows; the words sit behind the rows, see
// nlbac_node_rk_fwd's acts_bits).
// TRAJ: H intervals of a fixed-grid rollout in one launch (node_traj_kernels.hip).  Interval k's step is the one-step
// launch's with y0 = out[k-1] (kept in the tile's LDS, sY0) and u = L.u + k n n_u; its K / Y / G / rows / words sit at
// stage index k S + st of H S stages, and out[k] = L.out + k n n_s.  TRAJ = false, H = 1: the one-step kernel.
// GRID (with TRAJ; nlbac_node_rk_grid_fwd): interval k's step size is hs[k] (device array), put into sH at the top of
// the interval, and the actions L.u [n][n_u] are the same for every interval (node_rk_shared.h).
// SUB (with GRID; nlbac_node_rk_subgrid_fwd): the intervals are the fine intervals of a time grid under step_size; L.out
// takes the output points read off them (node_rk_shared.h).
// HOLD (with GRID, not SUB; nlbac_node_rk_hold_fwd: a rollout under step_size): H = N fine intervals, hm of them per
// control interval — interval k's step size is hs[k % hm], its actions L.u + (k / hm) n n_u, and L.out + (k / hm) n n_s
// is written behind a control interval's last fine step only (node_rk_shared.h).
// TILE (not TRAJ; nlbac_node_dopri_tile_fwd, node_tile_kernels.hip): H intervals of dopri5 under tile-local step control
// (node_rk_shared.h).  The stage loop runs in PHASES per interval — stage 0; the probe stage (index 1, quiet, the table
// row (1, 0, ..)); attempts of stages 1 .. S-1 — with rk_tile_after_phase behind each; what is kept goes to the tile's
// current slot (stage index slot S + st), nothing when tile->keep is 0.
// DENSE (with TILE, H = 1; nlbac_node_dopri_tile_dense_fwd, node_tile_dense_kernels.hip): one dense solve per tile, read
// at the output times of `dense` behind every accepted attempt (node_rk_shared.h).
template <int NB, int R, int BITS, int SPLIT, bool TRAJ = false, bool GRID = false, bool SUB = false, bool HOLD = false,
          bool TILE = false, bool DENSE = false>
__device__ __forceinline__ void node_rr_fwd_body(const NodeRkLaunch& L, int H = 1, const float* hs = nullptr,
                                                 const NlbacSubGrid* sub = nullptr, int hm = 1,
                                                 const NodeTileFwd* tile = nullptr,
                                                 const NodeTileDenseFwd* dense = nullptr) {
    static_assert(TRAJ || !GRID, "a time grid is a trajectory");
    static_assert(!(TILE && TRAJ), "tile-local step control walks its intervals itself");
    static_assert(TILE || !DENSE, "a dense solve is a tile's");
    static_assert(GRID || !SUB, "sub-steps are a time grid's");
    static_assert((GRID && !SUB) || !HOLD, "a held control's fine steps are a time grid's, its outputs their end points");
    static_assert(BITS != 2 || SPLIT == 0, "rows + words: the fit's forward is the unsplit one (same sums as mode 0)");
    constexpr bool WORDS = BITS != 0, ROWS = BITS != 1;
    using S = RRShape<NB, R>;
    constexpr int KS = S::KS, HID = S::HID;
    constexpr int TB = NB - 2;                 // first block of a layer's last group, the "tail": its accumulators are
    constexpr int NT = KS - 4 * TB;            // finished inside the NEXT product (NT values: 5 at hid 100, else 8)
    constexpr int MF = rr_split_m<S>();        // (SPLIT) f_net's last layer: MFMAs [0, MF) stay with its wave, [MF, NM) go
    using PF = RRPart<S, 0, MF>;
    using PG = RRPart<S, MF, S::NM>;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = wave >> 1, half = wave & 1;
    const int n = L.n, ns = L.n_s, nu = L.n_u, gout = ns * nu;
    const int row0 = blockIdx.x * NLBAC_MLP_TILE;
    RkFwdWhere w;
    if (!rk_fwd_where(L, row0, w)) return;
    RkFwdTile T;
    T.carve(smem);
    float* const sYin = smem + RkFwdTile::floats();      // [32][8] the stage input, columns ns..7 zero
    float* const sW0 = sYin + NLBAC_MLP_TILE * 8;        // [net][k-step < 3][block < 8][lane]: layer 0's A fragments
    // (SPLIT) the hand-over between a half tile's f_net and g_net waves
    float* const sX = sW0 + 2 * 3 * 8 * 64;              // [half][KS][lane] f_net's layer-2 activations
    float* const sF2 = sX + 2 * KS * 64;                 // [32][8] the g_net wave's part of f(x)
    unsigned* const sMw = reinterpret_cast<unsigned*>(sF2 + NLBAC_MLP_TILE * RK_MAX_NS);      // [half][f, g][lane] mask-word parts
    int* const sFlag = reinterpret_cast<int*>(sMw + 2 * 2 * 64);                               // [half] stage + 1 once sX is there
    // (TILE) the tile's control block and ints, behind everything else (node_tile_fwd_lds_floats)
    double* const sCtl = reinterpret_cast<double*>(smem + node_rr_fwd_lds_floats());
    int* const sInt = reinterpret_cast<int*>(sCtl + NLBAC_DOPRI_CTL);
    const nlbac_mlp& net = L.net[grp];
    const int nw = net.n_layers - 1;                     // layer 0 + (nw - 1) hid x hid layers, then the output layer
    const int n_rows = min(NLBAC_MLP_TILE, n - row0);
    const int q = lane >> 4, r16 = lane & 15;
    const int m = 16 * half + r16, grow = row0 + m;      // this lane's row: within the tile, global
    const bool row_ok = grow < n;
    const int KS0 = (ns + 3) >> 2;                       // registers a lane needs for its row's state components (1 or 2)
    const int KL0 = (ns + 4) >> 2;                       // k-steps of layer 0, which contracts [y | 1] with [W_0 | b_0] (1..3)
    // (TILE) where the tile keeps its steps, uniform per workgroup and read once: RR_KN / RR_KROW0 / RR_KGROW below
    [[maybe_unused]] NodeTilePlace P{};
    if constexpr (TILE) P = rk_tile_place(tile->page0, tile->max_slots, n, row0, blockIdx.x);

    // ---- what the stage loop reads of the launch descriptor, once
    const float* const params = net.params;
    int boff[RR_MAX_W];
#pragma unroll
    for (int l = 0; l < RR_MAX_W; ++l) boff[l] = net.b_off[l];
    float* const acts = L.acts[grp] ? L.acts[grp] + w.soff : nullptr;
    const long acts_ls = L.acts_ls[grp];
    // the mask words: in place of the rows (BITS 1, layer stride acts_ls), or behind the net's nw layers of rows (BITS 2,
    // [layer][S_total * n][4])
    unsigned* const words = !acts ? nullptr : reinterpret_cast<unsigned*>(BITS == 2 ? acts + (long)nw * acts_ls : acts);
    const long words_ls = (BITS == 2) ? (long)(TRAJ ? H : (TILE ? P.total : 1)) * L.S_total * RR_KN * 4 : acts_ls;
    const int stage_end = L.stage_end, S_last = L.S_total - 1;
    // the initial-step probe with its norm fused into this launch (norm_mode 1): nothing it would leave in memory — the
    // probe point, its derivative, g there — is read by anyone (the norm comes from LDS, the step's stage 1 overwrites
    // them), and stores in front of the epilogue's atomics are waited for there (vmcnt is in order)
    // (TILE: the probe phase, and every phase of a solve that keeps nothing)
    const bool quiet_launch = L.norm_mode == 1;

    // ---- the wave's weight stream: hid x hid layers 1 .. nw-1, then layer 1 again (next stage)
    const __amdgpu_buffer_rsrc_t rs = rr_rsrc(net.packed, net.packed_floats);
    const int voff = lane * 16;
    const int wbase = net.rr_fwd_off * 4;
    RRGemm<S> gemm;
    gemm.prime(rs, voff, wbase);

    // ---- constants of the launch: layer 0's A fragments (its bias rides in the k slot behind the last state component)
    //      to LDS in fragment order, the output layer's into registers
    if (half == 0) {
        const float* W0 = params + net.w_off[0];
        const float* b0 = params + boff[0];
#pragma unroll
        for (int k0 = 0; k0 < 3; ++k0)
#pragma unroll
            for (int jo = 0; jo < NB; ++jo) {
                // (unconditional loads, clamped index, select afterwards: a guarded load is a branch and a round trip of its own)
                const int uo = rr_unit_out(NB, R, jo, r16), col = 4 * k0 + q, uc = max(uo, 0);
                const float vw = W0[uc * ns + min(col, ns - 1)], vb = b0[uc];
                sW0[((grp * 3 + k0) * 8 + jo) * 64 + lane] = (uo < 0 || col > ns) ? 0.f : (col < ns ? vw : vb);
            }
    }
    float wo[KS];
    {
        const int orow = rr_out_row(grp, r16, ns, nu);
        const float* wrow = params + net.w_off[nw] + (long)max(orow, 0) * HID;
#pragma unroll
        for (int jo = 0; jo < NB; ++jo) {
            const f32x4 v = rr_row_load<S>(wrow, jo, q);
#pragma unroll
            for (int r = 0; r < ((jo < NB - 1) ? 4 : R); ++r) wo[4 * jo + r] = (orow >= 0) ? v[r] : 0.f;
        }
    }
    // this lane's outputs of the output layer (register r): their LDS slot in sF / sG (-1: none), their bias
    int o_idx[4]; float o_bias[4];
    {
        const float* bo = params + net.b_off[nw];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            int o = -1;
            if (grp == 0) { const int c = 4 * r + q; if (r < KS0 && c < ns) o = c; }
            else { const int k0 = r / nu, u = r - k0 * nu, c = 4 * k0 + q; if (r < KS0 * nu && c < ns) o = c * nu + u; }
            o_idx[r] = o;
            const float vb = bo[max(o, 0)];
            o_bias[r] = (o >= 0) ? vb : 0.f;
        }
    }

    // (SPLIT) what the g_net wave needs of f_net: its pack, its last layer's bias, its output layer's A fragments for the
    // k-steps the wave's blocks yield, the output slots (f_net's mapping of o_idx above)
    const nlbac_mlp& netF = L.net[0];
    const __amdgpu_buffer_rsrc_t rsF = rr_rsrc(netF.packed, netF.packed_floats);
    const int curF3 = netF.rr_fwd_off * 4 + 2 * S::LAYER_BYTES;          // byte offset of f_net's layer-3 stream
    float wof[KS];
    int of_idx[4];
    if constexpr (SPLIT != 0) {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) wof[ks] = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) { const int c = 4 * r + q; of_idx[r] = (r < KS0 && c < ns) ? c : -1; }
        if (grp == 1) {
            const int orow = rr_out_row(0, r16, ns, nu);
            const float* wrow = netF.params + netF.w_off[4] + (long)max(orow, 0) * HID;
#pragma unroll
            for (int jo = PG::J0; jo < NB; ++jo) {
                const f32x4 v = rr_row_load<S>(wrow, jo, q);
#pragma unroll
                for (int r = 0; r < ((jo < NB - 1) ? 4 : R); ++r) wof[4 * jo + r] = (orow >= 0) ? v[r] : 0.f;
            }
        }
        if (tid < 2) sFlag[tid] = 0;
    }

    RSTAMP(0)
    if constexpr (TILE) { if (tid == 0) sInt[TI_SLOT] = 0; }
    if constexpr (DENSE) { if (tid == 0) sInt[TI_OUT] = 0; }
    rk_fwd_tile_constants<256>(L, w, T, row0, tid);
    RSTAMP(1)

    [[maybe_unused]] unsigned tile_seq = 0u;             // (TILE) stages run so far: what the SPLIT hand-over's flags count
    for (int k = 0; k < ((TRAJ || TILE) ? H : 1); ++k) {
    const int kS_iv = TRAJ ? k * L.S_total : 0;          // interval k's first stage in the [k][stage][row] layout
    if constexpr (TRAJ) {
        w.gK = L.K + (long)kS_iv * n * ns;
        w.gY = L.Y + (long)kS_iv * n * ns;
        w.gG = L.G + (long)kS_iv * n * gout;
    }
    // (GRID) this interval's step size: behind the barrier that ended the interval before, in front of the one behind
    // the first stage's input (which, at stage 0, uses no step size; nlbac_node_rk_grid_fwd requires stage_begin == 0)
    if constexpr (GRID) { if (tid < NLBAC_MLP_TILE) T.sH[tid] = hs[HOLD ? k % hm : k]; }
    // (TILE) the phases of the interval come back to this label (a jump, not a loop: the instances that are not TILE
    // have to come out of the compiler as they did before there were phases); ph counts them
    int ph = 0;
    [[maybe_unused]] tile_phase:;
    // (TILE) the phase's stages, and the slot it keeps them in: stage index slot S + st of max_slots S stages (paged:
    // the tile's page P.page + slot in place of the slot)
    int slot = 0, tile_b = 0, tile_e = 0;
    bool tile_quiet = false;
    if constexpr (TILE) {
        if (tile->keep) slot = __builtin_amdgcn_readfirstlane(sInt[TI_SLOT]);
        tile_b = ph == 0 ? 0 : 1;
        tile_e = ph == 0 ? 1 : (ph == 1 ? 2 : L.S_total);
        tile_quiet = ph == 1 || !tile->keep;
    }
#define RR_ST_B (TILE ? tile_b : L.stage_begin)
#define RR_ST_E (TILE ? tile_e : stage_end)
#define RR_FKEY (TILE ? (int)tile_seq : kS + st + 1)      /* (SPLIT) the stage the hand-over's flag names */
    const int kS = TILE ? (P.page + slot) * L.S_total : kS_iv;
    const bool quiet = TILE ? tile_quiet : quiet_launch;
    if constexpr (TILE) {
        w.gG = L.G ? L.G + (long)kS * RR_KN * gout : nullptr;
        w.gY = (L.Y && !quiet) ? L.Y + (long)kS * RR_KN * ns : nullptr;
    }
    for (int st = RR_ST_B; st < RR_ST_E; ++st) {
        const int sb = 2 + 8 * (st - RR_ST_B);
        (void)sb;
        if constexpr (TILE) ++tile_seq;
        if (st == RR_ST_B) {
            if constexpr (TILE) rk_tile_first_input(L, T, row0, st, ph == 1, w.gY, RR_KN, RR_KROW0, sYin, tid, 256);
            else rk_fwd_first_input(L, w, T, row0, st, 8, sYin, 8, !quiet, tid, 256);
            __syncthreads();
        }
        RSTAMP(sb + 0)
        // the next stage's tableau row (scalar loads from the kernel arguments, issued now: the combine step behind the
        // layer chains was a chain of exposed load latencies)
        float bn[RK_MAX_STAGES];
        {
            const int sn = min(st + 1, S_last);
#pragma unroll
            for (int j = 0; j < RK_MAX_STAGES; ++j) bn[j] = L.beta[sn][j];
        }
        const long srow = (long)(kS + st) * RR_KN + RR_KGROW;
        float Ha[KS], Hb[KS];             // activations ping-pong between two register sets
        f32x4 acc0[NB], acc[NB], bv[NB], bpre[3];
        unsigned wd = 0u;                 // the mask word being assembled (values arrive in ascending register order)
        constexpr int G0 = rr_group_first(NB);
        // biases enter as the C operand of each block's first MFMA; those of a layer's first group of blocks are
        // requested one product ahead (bpre), the others at the layer's start
        auto prefetch_bias = [&](int l) __attribute__((always_inline)) {
#pragma unroll
            for (int jo = 0; jo < G0; ++jo) bpre[jo] = rr_bias<S>(params + boff[l], jo, q);
        };
        prefetch_bias(1);
        // (SPLIT) both waves' queues for their ranges of f_net's last layer: requested now, consumed two layers later
        PF partF; PG partG;
        if constexpr (SPLIT != 0) {
            if (grp == 0) partF.prime(rs, voff, curF3);
            else partG.prime(rsF, voff, curF3);
        }

        // what the backward needs of a finished value goes out once: a mask bit (word per layer), or the activation itself
        // (activation mode) a finished layer's activations leave in ONE burst, issued where the product that consumes
        // them starts its last group of blocks — by then the layer's pending tail is finished too.  Stores share the
        // loads' in-order vmcnt queue: issued one by one between the fragment loads, each made the MFMAs behind it wait
        // for its own trip to HBM; as a burst the trips overlap and the stream stalls once per layer.
        auto save_layer = [&](int l, const float (&H)[KS]) __attribute__((always_inline)) {
            if (!ROWS || !acts || !row_ok || (TILE && quiet)) return;
            float* rowp = acts + (long)l * acts_ls + srow * HID;
#pragma unroll
            for (int jo = 0; jo < NB; ++jo) {
                f32x4 hv{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int rr = 0; rr < ((jo < NB - 1) ? 4 : R); ++rr) hv[rr] = H[4 * jo + rr];
                rr_row_store<S>(rowp, jo, q, hv);
            }
        };
        auto save_word = [&](int l, unsigned word) __attribute__((always_inline)) {
            if (WORDS && words && row_ok && !(TILE && quiet)) words[(long)l * words_ls + srow * 4 + q] = word;
        };
        // layer 0's value ks (no bias: folded into the product), finished just before layer 1's k-step ks reads it
        auto pre_l0 = [&](int ks) __attribute__((always_inline)) {
            const int jo = (ks < 4 * (NB - 1)) ? (ks >> 2) : NB - 1, r = ks - 4 * jo;
            const float h = rr_relu(acc0[jo][r]);
            Ha[ks] = h;
            if (WORDS) rr_mask_push(wd, h);
            if (ks == KS - 1) save_word(0, wd);
        };
        // the tail of hid x hid layer lp (blocks TB, TB+1 of `acc`), finished inside the product that follows it: value t
        // at that product's k-step t (it is read at k-step 4 TB + t)
        auto pre_tail = [&](int lp, float (&H)[KS], int t) __attribute__((always_inline)) {
            if (t >= NT) return;
            const int jo = TB + (t >> 2), r = t & 3;
            const float h = rr_relu(acc[jo][r]);
            H[4 * TB + t] = h;
            if (WORDS) rr_mask_push(wd, h);
            if (t == NT - 1) save_word(lp, wd);
        };

        // ---- layer 0: K = ns + 1 (one to three k-steps), straight from the stage input
        {
            float yv[3], a0[3][NB];
#pragma unroll
            for (int k0 = 0; k0 < 3; ++k0) {
                const int col = 4 * k0 + q;
                yv[k0] = (col < ns) ? sYin[m * 8 + min(col, 7)] : (col == ns ? 1.f : 0.f);
            }
#pragma unroll
            for (int jo = 0; jo < NB; ++jo) a0[0][jo] = sW0[((grp * 3 + 0) * 8 + jo) * 64 + lane];
            if (KL0 == 1) {
#pragma unroll
                for (int jo = 0; jo < NB; ++jo)
                    acc0[jo] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[0][jo], yv[0], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
            } else {
#pragma unroll
                for (int jo = 0; jo < NB; ++jo) a0[1][jo] = sW0[((grp * 3 + 1) * 8 + jo) * 64 + lane];
                if (KL0 == 2) {
#pragma unroll
                    for (int jo = 0; jo < NB; ++jo) {
                        acc0[jo] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[0][jo], yv[0], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                        acc0[jo] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[1][jo], yv[1], acc0[jo], 0, 0, 0);
                    }
                } else {
#pragma unroll
                    for (int jo = 0; jo < NB; ++jo) a0[2][jo] = sW0[((grp * 3 + 2) * 8 + jo) * 64 + lane];
#pragma unroll
                    for (int jo = 0; jo < NB; ++jo) {
                        acc0[jo] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[0][jo], yv[0], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                        acc0[jo] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[1][jo], yv[1], acc0[jo], 0, 0, 0);
                        acc0[jo] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[2][jo], yv[2], acc0[jo], 0, 0, 0);
                    }
                }
            }
        }
        RSTAMP(sb + 1)

        // ---- the hid x hid layers and the output layer, statically unrolled (lc: the layer index as a type): wide layer l
        //      reads one activation set and writes the other
        auto wide = [&](auto lc, float (&Hin)[KS], float (&Hout)[KS]) __attribute__((always_inline)) {
            constexpr int l = decltype(lc)::value;
#pragma unroll
            for (int jo = 0; jo < NB; ++jo) bv[jo] = (jo < G0) ? bpre[jo] : rr_bias<S>(params + boff[l], jo, q);
            __builtin_amdgcn_sched_barrier(0);
            const int cur = wbase + (l - 1) * S::LAYER_BYTES;
            // (SPLIT: f_net's layer 3 has queues of its own — behind layer 2 the main stream goes on with the next stage)
            const int nxt = (l + 1 < nw && !(SPLIT != 0 && grp == 0 && l == 2)) ? cur + S::LAYER_BYTES : wbase;
            gemm.run(acc, bv, Hin, rs, voff, cur, nxt,
                     [&](int ks) __attribute__((always_inline)) {
                         if (l == 1) pre_l0(ks);
                         else pre_tail(l - 1, Hin, ks);
                     },
                     [&](int jo, int r) __attribute__((always_inline)) {
                         const float h = rr_relu(acc[jo][r]);
                         Hout[4 * jo + r] = h;
                         if (WORDS) rr_mask_push(wd, h);
                     },
                     [&]() __attribute__((always_inline)) {
                         if (l + 1 < nw) prefetch_bias(l + 1);
                         save_layer(l - 1, Hin);
                     });
            RSTAMP(sb + 1 + l)
        };
        // output layer (<= 16 outputs: one block), to LDS for k = f + g u; g(x) also to global for the backward
        auto outl = [&](auto lc, float (&Hin)[KS]) __attribute__((always_inline)) {
            constexpr int l = decltype(lc)::value;            // (= nw: the layers before it are 0 .. l-1)
            const f32x4 o = RRGemm<S>::block(wo, Hin, [&](int ks) __attribute__((always_inline)) { pre_tail(l - 1, Hin, ks); });
            save_layer(l - 1, Hin);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (o_idx[r] < 0) continue;
                const float val = o[r] + o_bias[r];
                if (grp == 0) T.sF[m * RK_MAX_NS + o_idx[r]] = val;
                else {
                    T.sG[m * RK_MAX_GOUT + o_idx[r]] = val;
                    if (row_ok && !quiet) w.gG[((long)st * RR_KN + RR_KGROW) * gout + o_idx[r]] = val;
                }
            }
        };
        using I1 = std::integral_constant<int, 1>; using I2 = std::integral_constant<int, 2>;
        using I3 = std::integral_constant<int, 3>; using I4 = std::integral_constant<int, 4>;
        // the reference's nets (U/sac_cbf_clf/model.py:186-206): f_net has three hid x hid layers, g_net two.  (One code
        // path per depth: a third, for two-layer nets, cost 26 more VGPRs and accumulator-file spills in all of them.)
        wide(I1{}, Ha, Hb);
        wide(I2{}, Hb, Ha);
        if constexpr (SPLIT == 0) {
            if (grp == 0) { wide(I3{}, Ha, Hb); outl(I4{}, Hb); }
            else outl(I3{}, Ha);
        } else {
            // one part of f_net's output layer over the k-steps [K0, K1) of the wave's blocks -> LDS (the f_net wave's with
            // the bias, into sF; the g_net wave's into sF2)
            auto out_part = [&](const f32x4& o, float* dst, bool with_bias) __attribute__((always_inline)) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (of_idx[r] >= 0) dst[m * RK_MAX_NS + of_idx[r]] = with_bias ? o[r] + o_bias[r] : o[r];
            };
            auto save_rows = [&](int l, const float (&H)[KS], int j0, int j1) __attribute__((always_inline)) {
                float* const actsF = L.acts[0] ? L.acts[0] + w.soff : nullptr;
                if (BITS || !actsF || !row_ok) return;
                float* rowp = actsF + (long)l * L.acts_ls[0] + srow * HID;
#pragma unroll
                for (int jo = 0; jo < NB; ++jo) {
                    if (jo < j0 || jo >= j1) continue;
                    f32x4 hv{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int rr = 0; rr < ((jo < NB - 1) ? 4 : R); ++rr) hv[rr] = H[4 * jo + rr];
                    rr_row_store<S>(rowp, jo, q, hv);
                }
            };
            unsigned wp = 0u;                  // this wave's part of layer 3's mask word
            if (grp == 0) {
                // layer 2 is finished now (its tail is not deferred: the g_net wave waits for ALL of it), handed over, then
                // the blocks [0, PF::J1) of layer 3 and their part of the output layer
#pragma unroll
                for (int t = 0; t < NT; ++t) pre_tail(2, Ha, t);
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) sX[(half * KS + ks) * 64 + lane] = Ha[ks];
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __hip_atomic_store(sFlag + half, RR_FKEY, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#pragma unroll
                for (int jo = 0; jo < NB; ++jo) bv[jo] = rr_bias<S>(params + boff[3], jo, q);
                auto fin3 = [&](int jo, int r) __attribute__((always_inline)) {
                    const float h = rr_relu(acc[jo][r]);
                    Hb[4 * jo + r] = h;
                    if (WORDS) rr_mask_push(wp, h);
                };
                partF.run(acc, bv, Ha, rs, voff, curF3, [&](int) __attribute__((always_inline)) {}, fin3);
                RSTAMP(sb + 4)
                save_layer(2, Ha);
                const f32x4 o = PF::block(wo, Hb, [&](int ks) __attribute__((always_inline)) {
                    if (ks >= 4 * PF::JT) fin3(PF::JT + ((ks - 4 * PF::JT) >> 2), (ks - 4 * PF::JT) & 3);
                });
                save_rows(3, Hb, 0, PF::J1);
                out_part(o, T.sF, true);
                if (BITS) sMw[(half * 2 + 0) * 64 + lane] = wp << (KS - PF::K1);
            } else {
                outl(I3{}, Ha);
                // f_net's layer-2 activations of the same rows, once its wave has put them there
                while (__hip_atomic_load(sFlag + half, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != RR_FKEY) __builtin_amdgcn_s_sleep(1);
                asm volatile("" ::: "memory");
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) Hb[ks] = sX[(half * KS + ks) * 64 + lane];
                RSTAMP(sb + 4)
#pragma unroll
                for (int jo = 0; jo < NB; ++jo) bv[jo] = (jo >= PG::J0) ? rr_bias<S>(netF.params + netF.b_off[3], jo, q) : f32x4{0.f, 0.f, 0.f, 0.f};
                auto fin3 = [&](int jo, int r) __attribute__((always_inline)) {
                    const float h = rr_relu(acc[jo][r]);
                    Ha[4 * jo + r] = h;
                    if (WORDS) rr_mask_push(wp, h);
                };
                partG.run(acc, bv, Hb, rsF, voff, curF3, [&](int) __attribute__((always_inline)) {}, fin3);
                const f32x4 o = PG::block(wof, Ha, [&](int ks) __attribute__((always_inline)) {
                    if (ks >= 4 * PG::JT) {
                        const int t = ks - 4 * PG::JT, jo = PG::JT + (t >> 2), r = t & 3;
                        if (jo < NB - 1 || r < R) fin3(jo, r);
                    }
                });
                save_rows(3, Ha, PG::J0, NB);
                out_part(o, sF2, false);
                if (BITS) sMw[(half * 2 + 1) * 64 + lane] = wp;
            }
        }
        RSTAMP(sb + 5)
        __syncthreads();
        RSTAMP(sb + 6)
        // ---- k = f + g u (same op order as affine_fwd_kernel) and, same thread, the next stage's input
        //      Y_{st+1} = y0 + h sum_j beta[st+1][j] K_j (same op order as rk_combine_kernel): one (row, component) per
        //      thread, every LDS operand requested up front, no data-dependent branch
        {
            const int mm = tid >> 3, c = tid & 7;
            const bool more = st + 1 < RR_ST_E, cv = c < ns, rv = row0 + mm < n;
            float a = T.sF[mm * RK_MAX_NS + c];
            if constexpr (SPLIT != 0) a += sF2[mm * RK_MAX_NS + c];
            float gv[RK_MAX_NU], uv[RK_MAX_NU], kj[RK_MAX_STAGES - 1];
#pragma unroll
            for (int u = 0; u < RK_MAX_NU; ++u) {
                gv[u] = T.sG[mm * RK_MAX_GOUT + min(c * nu + u, RK_MAX_GOUT - 1)];
                uv[u] = T.sU[mm * RK_MAX_NU + u];
            }
#pragma unroll
            for (int j = 0; j < RK_MAX_STAGES - 1; ++j) kj[j] = T.sK[(j * NLBAC_MLP_TILE + mm) * RK_MAX_NS + c];
            float y = T.sY0[mm * RK_MAX_NS + c];
            const float h = T.sH[mm];
#pragma unroll
            for (int u = 0; u < RK_MAX_NU; ++u) {
                const float t = a + gv[u] * uv[u];
                a = (u < nu) ? t : a;
            }
            float bst = 0.f;
#pragma unroll
            for (int j = 0; j < RK_MAX_STAGES - 1; ++j) {
                const float t = y + kj[j] * (bn[j] * h);
                y = (j < st && bn[j] != 0.f) ? t : y;
                bst = (j == st) ? bn[j] : bst;
            }
            {
                const float t = y + a * (bst * h);
                y = (bst != 0.f) ? t : y;
            }
            if (cv) {
                T.sK[(st * NLBAC_MLP_TILE + mm) * RK_MAX_NS + c] = a;
                if (rv && !quiet && !TILE) w.gK[((long)st * n + row0 + mm) * ns + c] = a;      // (TILE: K_0..6 stay in LDS)
                if (more && rv && (!TILE || w.gY)) w.gY[((long)(st + 1) * RR_KN + RR_KROW0 + mm) * ns + c] = y;
            }
            if (more) sYin[mm * 8 + c] = cv ? y : 0.f;
        }
        if constexpr (SPLIT != 0 && BITS != 0) {      // layer 3's mask word: the two waves' parts, stored by the f_net wave
            if (grp == 0 && L.acts[0] && row_ok && !(TILE && quiet))
                reinterpret_cast<unsigned*>(L.acts[0] + w.soff + 3 * L.acts_ls[0])[srow * 4 + q] =
                    sMw[(half * 2 + 0) * 64 + lane] | sMw[(half * 2 + 1) * 64 + lane];
        }
        __syncthreads();
        RSTAMP(sb + 7)
    }
#undef RR_ST_B
#undef RR_ST_E
#undef RR_FKEY
    if constexpr (TILE) {
        const int act = rk_tile_after_phase<256, DENSE>(L, *tile, P, T, sYin, sCtl, sInt, row0, n_rows, k, ph, slot, tid, dense);
        if (act >= 2) {
            if constexpr (DENSE) rk_tile_dense_stop<256>(L, *tile, *dense, sCtl, row0, sInt[TI_OUT], TILE_NO_SLOT, tid);
            else rk_tile_stop<256>(L, *tile, row0, act == 3 ? k + 1 : k, TILE_NO_SLOT, tid);
            return;
        }
        if (act == 0) {      // the next phase — at most NODE_TILE_MAX_ATTEMPTS attempts behind the two that open the interval
            if (++ph >= 2 + NODE_TILE_MAX_ATTEMPTS) {
                if constexpr (DENSE) rk_tile_dense_stop<256>(L, *tile, *dense, sCtl, row0, sInt[TI_OUT], TILE_MAX_ATTEMPTS, tid);
                else rk_tile_stop<256>(L, *tile, row0, k, TILE_MAX_ATTEMPTS, tid);
                return;
            }
            goto tile_phase;
        }
    }
    if constexpr (TRAJ) rk_traj_advance<256, GRID, SUB, HOLD>(L, T, row0, k, H, tid, sub, hm);
    }
    if constexpr (TRAJ || TILE) return;
#ifdef RR_TIMING
    if (L.err) return;
#endif
    rk_fwd_outputs_and_control<256>(L, w, T, row0, n_rows, tid);
}

// ---------------------------------------------------------------------------------------------------------------------
// Backward of the same step, same wave roles.  Per stage (descending): the output layer's gradient enters as the B
// operand of one transposed block product, then dz_{l-1} = mask_{l-1} * (W_l^T dz_l) down the chain in registers (the
// backward RR pack), then dX = W_0^T dz_0; the two nets meet in the stage algebra (rk_bwd_stage_algebra).
// ---------------------------------------------------------------------------------------------------------------------
// SPLIT (see the forward): f_net's chain has one product more than g_net's — its FIRST, dz_2 = mask_2 * (W_3^T dz_3).  The
// g_net wave of the half tile computes the lower groups of output blocks of that product before its own chain starts
// (dz_3 comes over through LDS behind a flag, the blocks go back the same way), the f_net wave the upper groups.
// TRAJ: the backward of a whole fixed-grid rollout (node_traj_kernels.hip), intervals k = H-1 .. 0 in one launch: interval
// k's step is the one-step launch's with dL/dout_k = X.dout[k+1] + the dy0 of interval k+1 (carried in sDY0), dK / dy0
// formed from it as nlbac_rk_stage_bwd forms them from the step's output combination, u = L.u + k n n_u, du -> L.du +
// k n n_u; rows / words / G / dK / dG / dz at stage index k S + st of H S stages.  X.dx0 = X.dout[0] + the dy0 of
// interval 0.  TRAJ = false (X null): the one-step kernel.
// GRID (with TRAJ; nlbac_node_rk_grid_bwd): step size hs[k] per interval, one set of actions L.u [n][n_u], and L.du
// [n][n_u] the sum of the intervals' du, formed in the tile's LDS in the order k = H-1 .. 0 (node_rk_shared.h).
// SUB (with GRID; nlbac_node_rk_subgrid_bwd): X.dout [T][n][n_s] belongs to the output points, injected between the fine
// intervals (node_rk_shared.h).
// HOLD (with GRID, not SUB; nlbac_node_rk_hold_bwd): X.H = N fine intervals, hm per control interval; X.dout [N/hm + 1]
// and L.du [N/hm] belong to the control intervals (node_rk_shared.h).
// TILE (not TRAJ; nlbac_node_dopri_tile_bwd, node_tile_kernels.hip): the backward of a dopri5 horizon under tile-local
// step control — intervals k = H-1 .. 0 and, inside each, the tile's kept steps last to first (slot = first + sj; rows /
// words / G / dK / dG / dz at stage index slot S + st); rk_tile_bwd_begin / _end (node_rk_shared.h) around each step's
// stages; a step that is not its interval's first leaves out stage 0 (its predecessor's last: FSAL).
// DENSE (with TILE, H = 1; nlbac_node_dopri_tile_dense_bwd): the backward of a tile's dense solve — every step takes the
// gradients of the outputs that fell in it before the hand-over (rk_tile_dense_bwd_begin, node_rk_shared.h).
template <int NB, int R, int BITS, int SPLIT, bool TRAJ = false, bool GRID = false, bool SUB = false, bool HOLD = false,
          bool TILE = false, bool DENSE = false>
__device__ __forceinline__ void node_rr_bwd_body(const NodeRkBwdLaunch& L, const NodeRkTrajBwd* X = nullptr,
                                                 const float* hs = nullptr, const NlbacSubGrid* sub = nullptr,
                                                 int hm = 1, const NodeTileBwd* tile = nullptr,
                                                 const NodeTileDenseBwd* dense = nullptr) {
    static_assert(TILE || !DENSE, "a dense solve is a tile's");
    static_assert(TRAJ || !GRID, "a time grid is a trajectory");
    static_assert(!(TILE && TRAJ), "tile-local step control walks its intervals itself");
    static_assert(GRID || !SUB, "sub-steps are a time grid's");
    static_assert((GRID && !SUB) || !HOLD, "a held control's fine steps are a time grid's, its outputs their end points");
    constexpr bool WORDS = BITS != 0;          // the gates come from the mask words (1, 2) or from the activation rows (0)
    constexpr bool DZ = BITS != 1;             // dz rows are stored when asked for (0; 2: the fit, words behind the rows)
    using S = RRShape<NB, R>;
    constexpr int KS = S::KS, HID = S::HID, TB = NB - 2, NT = KS - 4 * TB;
    constexpr int MB = rr_split_m<S>();        // (SPLIT) f_net's first product: MFMAs [0, MB) go to the g_net wave
    using PG = RRPart<S, 0, MB>;
    using PF = RRPart<S, MB, S::NM>;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = wave >> 1, half = wave & 1;
    const int n = L.n, ns = L.n_s, nu = L.n_u, gout = ns * nu;
    const int row0 = blockIdx.x * NLBAC_MLP_TILE;
    RkBwdWhere w;
    if (!rk_bwd_where(L, row0, w)) return;
    RkBwdTile T;
    T.carve(smem);
    float* const sWt = smem + RkBwdTile::floats();       // [net][k-step < 4][block < 8][lane]: W_out^T's A fragments
    // (SPLIT) the hand-over between a half tile's f_net and g_net waves
    float* const sX = sWt + 2 * 4 * 8 * 64;              // [half][KS][lane] f_net's dz_3
    float* const sX2 = sX + 2 * KS * 64;                 // [half][PG::K1][lane] the g_net wave's blocks of dz_2
    int* const sFlag = reinterpret_cast<int*>(sX2 + 2 * 16 * 64);      // [2][half]: sX / sX2 are there for stage key
    const nlbac_mlp& net = L.net[grp];
    const int nw = net.n_layers - 1;
    const int q = lane >> 4, r16 = lane & 15;
    const int m = 16 * half + r16, grow = row0 + m;
    const bool row_ok = grow < n;
    const int growc = min(grow, n - 1);
    const int KS0 = (ns + 3) >> 2;
    const int KSO = (grp == 0) ? KS0 : KS0 * nu;          // k-steps of the output layer's transposed product (<= 4)
    // (TILE) where the tile keeps its steps (see the forward)
    [[maybe_unused]] NodeTilePlace P{};
    if constexpr (TILE) P = rk_tile_place(tile->page0, tile->max_slots, n, row0, blockIdx.x);
    const bool keep_dz = L.dz[0] != nullptr;

    // ---- what the stage loop reads of the launch descriptor, once
    const float* const params = net.params;
    const float* const acts = L.acts[grp] + w.soff;
    float* const dz = keep_dz ? L.dz[grp] + w.soff : nullptr;
    const long acts_ls = L.acts_ls[grp];
    // (WORDS) where the forward left the words: in place of the rows (1), or behind the net's nw layers of rows (2)
    const unsigned* const words = reinterpret_cast<const unsigned*>(BITS == 2 ? acts + (long)nw * acts_ls : acts);
    const int H = TRAJ ? X->H : (TILE ? tile->H : 1);
    // (the stages the buffers hold: H S of a trajectory, max_slots S — paged: pages S — under TILE)
    const long words_ls = (BITS == 2) ? (long)(TILE ? P.total : H) * L.S_total * RR_KN * 4 : acts_ls;
    const int dx_stage0 = L.dx_stage0;

    // ---- weight stream: backward fragments of layers nw-1 .. 1, then nw-1 again (next stage)
    const __amdgpu_buffer_rsrc_t rs = rr_rsrc(net.packed, net.packed_floats);
    const int voff = lane * 16;
    const int wbase = net.rr_bwd_off * 4;
    RRGemm<S> gemm;
    // (SPLIT: f_net's first product has queues of its own — its main stream starts with the second)
    const int first_l = (SPLIT != 0 && grp == 0) ? nw - 3 : nw - 2;
    gemm.prime(rs, voff, wbase + first_l * S::LAYER_BYTES);
    const nlbac_mlp& netF = L.net[0];
    const __amdgpu_buffer_rsrc_t rsF = rr_rsrc(netF.packed, netF.packed_floats);
    const int curB3 = netF.rr_bwd_off * 4 + 2 * S::LAYER_BYTES;          // byte offset of W_3^T's stream (f_net)
    if (SPLIT != 0 && tid < 4) sFlag[tid] = 0;

    // ---- constants: W_out^T (A of the top product) to LDS in fragment order, W_0^T (A of dX) into registers
    if (half == 0) {
        const float* Wl = params + net.w_off[nw];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            int o = -1;
            if (grp == 0) { const int c = 4 * e + q; if (e < KS0 && c < ns) o = c; }
            else { const int k0 = e / nu, u = e - k0 * nu, c = 4 * k0 + q; if (e < KS0 * nu && c < ns) o = c * nu + u; }
#pragma unroll
            for (int jo = 0; jo < NB; ++jo) {
                const int uo = rr_unit_out(NB, R, jo, r16);
                const float vw = Wl[(long)max(o, 0) * HID + max(uo, 0)];
                sWt[((grp * 4 + e) * 8 + jo) * 64 + lane] = (o >= 0 && uo >= 0) ? vw : 0.f;
            }
        }
    }
    float w0t[KS];
    {
        const float* W0 = params + net.w_off[0];
        const int c = 4 * (r16 & 3) + (r16 >> 2);          // A row 4 q' + r' computes dX component 4 r' + q'
        const bool ok = (r16 & 3) < KS0 && c < ns;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const float vw = W0[(long)rr_unit_in(NB, R, ks, q) * ns + min(c, ns - 1)];
            w0t[ks] = ok ? vw : 0.f;
        }
    }

    BWSTAMP(0)
    if constexpr (!TRAJ && !TILE) rk_bwd_tile_constants<256>(L, w, T, row0, tid);
    if constexpr (TILE) w.ip = true;      // (dL/dy1 of every step comes from sDYup: rk_tile_bwd_begin)
    __syncthreads();
    BWSTAMP(1)

    // g(Y_st) for the du term comes from global memory: this thread's values of a stage are requested while the stage
    // before it runs (loads issued at the start of a stage would sit in front of the stage's first weight-fragment loads in
    // the in-order vmcnt queue); the tableau row (scalar loads) likewise, behind the stage's first LDS wait
    const bool du_thread = L.du && tid < NLBAC_MLP_TILE * nu;
    const int du_m = du_thread ? tid / nu : 0, du_c = du_thread ? tid - du_m * nu : 0;
    float gnext[RK_MAX_NS];
    __shared__ float sBeta[RK_MAX_STAGES * RK_MAX_STAGES];      // the tableau, once: per-stage scalar loads of its rows from the
    if (tid < RK_MAX_STAGES * RK_MAX_STAGES)                      // kernel arguments cost SGPRs (spills) and a wait per stage
        sBeta[tid] = (&L.beta[0][0])[tid];
    auto request_g = [&](int stn) __attribute__((always_inline)) {
        if (!du_thread || stn < w.st_lo) return;
        const float* gp = w.gG + ((long)stn * RR_KN + min(RR_KROW0 + du_m, RR_KN - 1)) * gout + du_c;
#pragma unroll
        for (int r = 0; r < RK_MAX_NS; ++r) gnext[r] = gp[min(r, ns - 1) * nu];
    };
    [[maybe_unused]] unsigned tile_seq = 0u;                      // (TILE) stages walked so far: what the SPLIT flags count
    for (int kk = 0; kk < H; ++kk) {
    const int k = H - 1 - kk, kS_iv = TRAJ ? k * L.S_total : 0;   // interval k's first stage in the [k][stage][row] layout
    // (TILE) the interval's kept steps: clamped to the tile's slots, whatever the arrays hold
    int t_first = 0, t_nacc = 1;
    float t_x = 0.f;
    if constexpr (TILE && !DENSE) {
        const long ti = (long)blockIdx.x * H + k;
        t_first = min(max(tile->iv_first[ti], 0), P.slots - 1);
        t_nacc = min(max(tile->iv_nacc[ti], 1), P.slots - t_first);
        t_x = tile->iv_x[ti];
    }
    // (DENSE) the one interval's steps are the slots 0 .. accepted - 1; d_je: the outputs no later step has taken
    [[maybe_unused]] int d_je = 0;
    if constexpr (DENSE) {
        t_nacc = min(max(tile->iv_nacc[blockIdx.x], 1), P.slots);
        d_je = max(dense->n_out, 0);
    }
    // (TILE) the interval's steps come back to this label, last to first (a jump, not a loop: see the forward)
    int sj = TILE ? t_nacc - 1 : 0;
    [[maybe_unused]] tile_step:;
    const int kS = TILE ? (P.page + t_first + sj) * L.S_total : kS_iv;
    if constexpr (TRAJ || TILE) {
        w.gG = L.G + (long)kS * RR_KN * gout;
        w.gdG = L.dG ? L.dG + (long)kS * RR_KN * gout : nullptr;
        w.gdK = L.dK ? L.dK + (long)kS * RR_KN * ns : nullptr;
        if constexpr (TILE) {
            w.st_lo = sj == 0 ? 0 : 1;
            const float h = (float)tile->hslots[P.hbase + t_first + sj];
            if constexpr (DENSE) rk_tile_dense_bwd_begin<256>(L, *tile, *dense, T, row0, sj, sj == t_nacc - 1, h, d_je, tid);
            else rk_tile_bwd_begin<256>(L, *tile, T, row0, k, kk, sj == t_nacc - 1, h, t_x, tid);
        } else {
            rk_traj_bwd_begin<256, GRID, SUB, HOLD>(L, *X, T, row0, k, kk, tid, hs, sub, hm);
        }
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < RK_MAX_NS; ++r) gnext[r] = 0.f;
    request_g(L.st_hi - 1);
    for (int st = L.st_hi - 1; st >= w.st_lo; --st) {
        const int sbw = 2 + 8 * st;
        (void)sbw;
        BWSTAMP(sbw + 0)
        const bool data = w.has_data(st);
        float gcur[RK_MAX_NS];
#pragma unroll
        for (int r = 0; r < RK_MAX_NS; ++r) gcur[r] = gnext[r];
        request_g(st - 1);
        // ---- output-layer gradients: f: dK itself, g: dK u^T (also kept for the weight gradients), and du — every LDS
        //      operand requested with a clamped index, selects afterwards (no per-column branch)
        float dy[4];
        {
            float dk[4], uu[4], dkd[RK_MAX_NS];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int k0 = (grp == 0) ? e : e / nu, u = (grp == 0) ? 0 : e - k0 * nu, c = 4 * k0 + q;
                dk[e] = T.sDK[(st * NLBAC_MLP_TILE + m) * RK_MAX_NS + min(c, ns - 1)];
                uu[e] = (grp == 0) ? 1.f : T.sU[m * RK_MAX_NU + min(u, nu - 1)];
            }
#pragma unroll
            for (int r = 0; r < RK_MAX_NS; ++r) dkd[r] = T.sDK[(st * NLBAC_MLP_TILE + du_m) * RK_MAX_NS + r];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int k0 = (grp == 0) ? e : e / nu, u = (grp == 0) ? 0 : e - k0 * nu, c = 4 * k0 + q;
                const bool ok = (grp == 0) ? (e < KS0 && c < ns) : (e < KS0 * nu && c < ns);
                const float v = (grp == 0) ? dk[e] : dk[e] * uu[e];
                dy[e] = ok ? v : 0.f;
                if (grp != 0 && ok && w.gdG && row_ok) w.gdG[((long)st * RR_KN + RR_KGROW) * gout + c * nu + u] = v;
            }
            if (du_thread) {        // du += g(Y_st)^T dK_st (rk_bwd_du's sum, same order)
                float a = 0.f;
#pragma unroll
                for (int r = 0; r < RK_MAX_NS; ++r) a = (r < ns) ? a + gcur[r] * dkd[r] : a;
                T.sDU[du_m * RK_MAX_NU + du_c] = T.sDU[du_m * RK_MAX_NU + du_c] + 1.0f * a;
            }
        }
        if (!data) continue;              // uniform: nothing below is needed for this stage
        BWSTAMP(sbw + 1)

        const long srow = (long)(kS + st) * RR_KN + RR_KGROWC;
        float Za[KS], Zb[KS];              // dz ping-pong between two register sets
        f32x4 acct[NB], acc[NB], zero[NB];
#pragma unroll
        for (int jo = 0; jo < NB; ++jo) zero[jo] = f32x4{0.f, 0.f, 0.f, 0.f};
        // ReLU masks of a layer's outputs for this lane's units: one word (mask mode) or the activations themselves,
        // requested before the product they gate so that they land under it; `*t`: those of the pending tail / top product
        unsigned mw = 0u, mwt = 0u;
        f32x4 avA[NB], avB[NB], avt[2];       // (activation mode) two sets: a product's masks are requested one product ahead
        auto fetch_masks = [&](int l, f32x4 (&av)[NB]) __attribute__((always_inline)) {
            if (WORDS) {       // (rows past the end contribute nothing: their word is cleared once)
                mw = words[(long)l * words_ls + srow * 4 + q];
                mw = row_ok ? mw : 0u;
            }
            else {
                const float* arow = acts + (long)l * acts_ls + srow * HID;
#pragma unroll
                for (int jo = 0; jo < NB; ++jo) av[jo] = rr_row_load<S>(arow, jo, q);
            }
        };
        // (activation mode, weight gradients wanted) a finished dz leaves in one burst inside the product that consumes it,
        // like the forward's activations (see there)
        auto save_dz = [&](int l, const float (&Z)[KS]) __attribute__((always_inline)) {
            if (!DZ || !dz || !row_ok) return;
            float* rowp = dz + (long)l * acts_ls + ((long)(kS + st) * RR_KN + RR_KGROW) * HID;
#pragma unroll
            for (int jo = 0; jo < NB; ++jo) {
                f32x4 zv{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int rr = 0; rr < ((jo < NB - 1) ? 4 : R); ++rr) zv[rr] = Z[4 * jo + rr];
                rr_row_store<S>(rowp, jo, q, zv);
            }
        };
        // the top product's value ks (mask mode: finished just before the next product's k-step ks reads it)
        auto pre_top = [&](int ks) __attribute__((always_inline)) {
            const int jo = (ks < 4 * (NB - 1)) ? (ks >> 2) : NB - 1, r = ks - 4 * jo;
            if (WORDS) Za[ks] = rr_mask_gate<KS>(mwt, ks, acct[jo][r]);
            else Za[ks] = (row_ok && avA[jo][r] > 0.f) ? acct[jo][r] : 0.f;
        };
        // the tail (blocks TB, TB+1 of `acc`) of the product that produced dz of layer lp, finished inside the next one
        auto pre_tail = [&](float (&Z)[KS], int t) __attribute__((always_inline)) {
            if (t >= NT) return;
            const int jo = TB + (t >> 2), r = t & 3;
            if (WORDS) Z[4 * TB + t] = rr_mask_gate<KS>(mwt, 4 * TB + t, acc[jo][r]);
            else Z[4 * TB + t] = (row_ok && avt[jo - TB][r] > 0.f) ? acc[jo][r] : 0.f;
        };

        // ---- top product: dz_top = mask_top * (W_out^T dy); the first chain product's masks are requested with its own
        fetch_masks(nw - 1, avA);
        if (!WORDS) fetch_masks(nw - 2, avB);
        {
            float at[4][NB];
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int jo = 0; jo < NB; ++jo) at[e][jo] = (e < 2 || KSO > 2) ? sWt[((grp * 4 + e) * 8 + jo) * 64 + lane] : 0.f;
            if (KSO <= 2) {
#pragma unroll
                for (int jo = 0; jo < NB; ++jo) {
                    acct[jo] = __builtin_amdgcn_mfma_f32_16x16x4f32(at[0][jo], dy[0], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                    acct[jo] = __builtin_amdgcn_mfma_f32_16x16x4f32(at[1][jo], dy[1], acct[jo], 0, 0, 0);
                }
            } else {
#pragma unroll
                for (int jo = 0; jo < NB; ++jo) {
                    acct[jo] = __builtin_amdgcn_mfma_f32_16x16x4f32(at[0][jo], dy[0], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                    acct[jo] = __builtin_amdgcn_mfma_f32_16x16x4f32(at[1][jo], dy[1], acct[jo], 0, 0, 0);
                    acct[jo] = __builtin_amdgcn_mfma_f32_16x16x4f32(at[2][jo], dy[2], acct[jo], 0, 0, 0);
                    acct[jo] = __builtin_amdgcn_mfma_f32_16x16x4f32(at[3][jo], dy[3], acct[jo], 0, 0, 0);
                }
            }
        }
#ifdef RR_BWD_NO_DEFER_TOP
        constexpr bool defer_top = false;
        mwt = mw;
#else
        constexpr bool defer_top = WORDS;
#endif
        if (!defer_top) {       // (activation mode keeps one set of mask registers: the top product is finished at once)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) pre_top(ks);
        }
        // ---- dz_{nw-1-p} = mask * (W_{nw-p}^T dz_{nw-p}), p = 1 .. nw-1, then dX = W_0^T dz_0 (one block); statically
        //      unrolled (pc: the product index as a type): a product reads one dz set and writes the other
        // (avC: this product's masks — already requested; avN: where the next product's go)
        auto prod = [&](auto pc, float (&Zin)[KS], float (&Zout)[KS], f32x4 (&avC)[NB], f32x4 (&avN)[NB]) __attribute__((always_inline)) {
            constexpr int p = decltype(pc)::value;
            const int lo = nw - 1 - p;                            // the layer whose dz this product yields
            mwt = mw;
            if (WORDS) fetch_masks(lo, avC);
            __builtin_amdgcn_sched_barrier(0);
            const int cur = wbase + lo * S::LAYER_BYTES;              // fragments of layer lo + 1 sit at index lo
            const int nxt = (lo >= 1) ? cur - S::LAYER_BYTES : wbase + first_l * S::LAYER_BYTES;
            gemm.run(acc, zero, Zin, rs, voff, cur, nxt,
                     [&](int ks) __attribute__((always_inline)) {
                         if (p == 1) { if (defer_top) pre_top(ks); }
                         else pre_tail(Zin, ks);
                     },
                     [&](int jo, int r) __attribute__((always_inline)) {
                         if (WORDS) Zout[4 * jo + r] = rr_mask_gate<KS>(mw, 4 * jo + r, acc[jo][r]);
                         else Zout[4 * jo + r] = (row_ok && avC[jo][r] > 0.f) ? acc[jo][r] : 0.f;
                     },
                     [&]() __attribute__((always_inline)) {
                         save_dz(lo + 1, Zin);                        // (Zin is complete: its tail was finished in group 0)
                         if (!WORDS && lo >= 1) fetch_masks(lo - 1, avN);
                     });
            avt[0] = avC[TB]; avt[1] = avC[TB + 1];               // (this product's own tail is finished in the next one)
        };
        const bool skip_dx = (st == 0 && !dx_stage0);       // only the dz of stage 0 were wanted
        auto dxl = [&](float (&Zin)[KS]) __attribute__((always_inline)) {
            mwt = mw;
            const f32x4 o = RRGemm<S>::block(w0t, Zin, [&](int ks) __attribute__((always_inline)) { pre_tail(Zin, ks); });
            save_dz(0, Zin);
            if (!skip_dx) {
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    const int c = 4 * r + q;
                    if (r < KS0 && c < ns) T.sDX[(grp * NLBAC_MLP_TILE + m) * RK_MAX_NS + c] = o[r];
                }
            }
        };
        using I1 = std::integral_constant<int, 1>; using I2 = std::integral_constant<int, 2>;
        using I3 = std::integral_constant<int, 3>;
        BWSTAMP(sbw + 2)
        if constexpr (SPLIT == 0) {
            prod(I1{}, Za, Zb, avB, avA);                     // (f_net: three hid x hid layers, g_net: two — see the forward)
            prod(I2{}, Zb, Za, avA, avB);
            if (grp == 0) { prod(I3{}, Za, Zb, avB, avA); dxl(Zb); }
            else dxl(Za);
        } else {
            const int key = TILE ? (int)(++tile_seq) : kk * L.S_total + L.st_hi - st;    // (1, 2, ...: what the flags count)
            const float* const actsF = L.acts[0] + w.soff;
            if (grp == 0) {
                // dz_3 complete (the top product is not deferred here), handed over; then the upper groups of dz_2's blocks
                if (defer_top) {
                    mwt = mw;
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks) pre_top(ks);
                }
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) sX[(half * KS + ks) * 64 + lane] = Za[ks];
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __hip_atomic_store(sFlag + half, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                PF partF;
                partF.prime(rs, voff, curB3);
                if (WORDS) fetch_masks(2, avB);                // (activation mode: layer 2's rows are in avB already)
                partF.run(acc, zero, Za, rs, voff, curB3, [&](int) __attribute__((always_inline)) {},
                          [&](int jo, int r) __attribute__((always_inline)) {
                              if (WORDS) Zb[4 * jo + r] = rr_mask_gate<KS>(mw, 4 * jo + r, acc[jo][r]);
                              else Zb[4 * jo + r] = (row_ok && avB[jo][r] > 0.f) ? acc[jo][r] : 0.f;
                          });
                save_dz(3, Za);
                if (!WORDS) fetch_masks(1, avA);
                avt[0] = avB[TB]; avt[1] = avB[TB + 1];
                // the lower blocks, from the g_net wave
                while (__hip_atomic_load(sFlag + 2 + half, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != key) __builtin_amdgcn_s_sleep(1);
                asm volatile("" ::: "memory");
#pragma unroll
                for (int k = 0; k < PG::K1; ++k) Zb[k] = sX2[(half * 16 + k) * 64 + lane];
                BWSTAMP(sbw + 3)
                prod(I2{}, Zb, Za, avA, avB);
                prod(I3{}, Za, Zb, avB, avA);
                BWSTAMP(sbw + 4)
                dxl(Zb);
            } else {
                // the lower groups of blocks of f_net's dz_2 for the same rows, before this wave's own chain
                unsigned mwF = 0u;
                f32x4 avF[PG::J1];
                if (WORDS) {
                    const unsigned* const wordsF = reinterpret_cast<const unsigned*>(
                        BITS == 2 ? actsF + (long)(netF.n_layers - 1) * L.acts_ls[0] : actsF);
                    mwF = wordsF[2 * (BITS == 2 ? (long)(TILE ? P.total : H) * L.S_total * RR_KN * 4 : L.acts_ls[0]) + srow * 4 + q];
                    mwF = row_ok ? mwF : 0u;
                } else {
                    const float* arow = actsF + 2 * L.acts_ls[0] + srow * HID;
#pragma unroll
                    for (int jo = 0; jo < PG::J1; ++jo) avF[jo] = rr_row_load<S>(arow, jo, q);
                }
                PG partG;
                partG.prime(rsF, voff, curB3);
                while (__hip_atomic_load(sFlag + half, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != key) __builtin_amdgcn_s_sleep(1);
                asm volatile("" ::: "memory");
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) Zb[ks] = sX[(half * KS + ks) * 64 + lane];
                partG.run(acc, zero, Zb, rsF, voff, curB3, [&](int) __attribute__((always_inline)) {},
                          [&](int, int) __attribute__((always_inline)) {});
                // (all of the range's blocks are still pending when it is a single group; with two groups the first was
                //  never finished by a hook either: every block is gated here)
#pragma unroll
                for (int jo = 0; jo < PG::J1; ++jo)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float v;
                        if (WORDS) v = rr_mask_gate<KS>(mwF, 4 * jo + r, acc[jo][r]);
                        else v = (row_ok && avF[jo][r] > 0.f) ? acc[jo][r] : 0.f;
                        sX2[(half * 16 + 4 * jo + r) * 64 + lane] = v;
                    }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __hip_atomic_store(sFlag + 2 + half, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                BWSTAMP(sbw + 3)
                prod(I1{}, Za, Zb, avB, avA);
                prod(I2{}, Zb, Za, avA, avB);
                BWSTAMP(sbw + 4)
                dxl(Za);
            }
        }
        BWSTAMP(sbw + 5)
        if (skip_dx) continue;
        __syncthreads();
        BWSTAMP(sbw + 6)
        // ---- stage algebra (rk_bwd_stage_algebra's arithmetic): dY = [dYup at the last stage] + dX_f + dX_g; dy0 += dY;
        //      dK_j += beta[st][j] h dY for j < st — one (row, component) per thread, every operand requested up front
        if (tid < NLBAC_MLP_TILE * RK_MAX_NS) {
            const int mm = tid >> 3, c = tid & 7, row = row0 + mm;
            const bool cv = c < ns, up = (w.gdYup || w.ip) && st == L.S_total - 1;
            const float xf = T.sDX[mm * RK_MAX_NS + c], xg = T.sDX[(NLBAC_MLP_TILE + mm) * RK_MAX_NS + c];
            const float y0 = T.sDY0[mm * RK_MAX_NS + c], h = T.sH[mm];
            float kj[RK_MAX_STAGES - 1], bn[RK_MAX_STAGES - 1];
#pragma unroll
            for (int j = 0; j < RK_MAX_STAGES - 1; ++j) {
                kj[j] = T.sDK[(j * NLBAC_MLP_TILE + mm) * RK_MAX_NS + c];
                bn[j] = sBeta[st * RK_MAX_STAGES + j];
            }
            float d = 0.f;
            if (up) d = w.ip ? T.sDYup[mm * RK_MAX_NS + c] : w.gdYup[(long)min(row, n - 1) * ns + min(c, ns - 1)];      // (uniform branch)
            d = (up && row < n) ? d : 0.f;
            d += xf;
            d += xg;
            if (cv) {
                T.sDY0[mm * RK_MAX_NS + c] = y0 + d;
#pragma unroll
                for (int j = 0; j < RK_MAX_STAGES - 1; ++j) {
                    const float t = kj[j] + (bn[j] * h) * d;
                    T.sDK[(j * NLBAC_MLP_TILE + mm) * RK_MAX_NS + c] = (j < st && bn[j] != 0.f) ? t : kj[j];
                }
            }
        }
        __syncthreads();
        BWSTAMP(sbw + 7)
    }
    __syncthreads();
    BWSTAMP(2 + 8 * 7)
    if constexpr (TRAJ) {
        rk_traj_bwd_end<256, GRID, SUB, HOLD>(L, *X, w, T, row0, k, tid, sub, hm);
        __syncthreads();
    }
    if constexpr (TILE) {
        rk_tile_bwd_end<256, DENSE>(L, *tile, P, w, T, row0, k, sj, tid);
        __syncthreads();
        if (--sj >= 0) goto tile_step;
    }
    }
    if constexpr (!TRAJ && !TILE) rk_bwd_outputs<256>(L, w, T, row0, tid);
}

#undef RR_KN
#undef RR_KROW0
#undef RR_KGROW
#undef RR_KGROWC

// ---------------------------------------------------------------------------------------------------------------------
// host side: which instance of a kernel template serves a launch, and with how much LDS — one definition for the
// one-step launchers (node_rr_kernels.hip) and the trajectory / time-grid launchers (node_traj_kernels.hip), whose
// results are the one-step launches' bit for bit only while they pick the same instance.
// ---------------------------------------------------------------------------------------------------------------------
// the instances of one kernel template KERN<NB, R, BITS, SPLIT>: k [shape][acts_bits].  The f_net / g_net wave balance
// (SPLIT, see the kernels) is a property of the direction and of acts_bits, not a choice: the backward is always split,
// the forward in mask mode only.  With activation rows kept (acts_bits 0 / 2; the NODE fit: 32768 rows, two workgroups
// per CU) the two waves' store bursts and the hand-over cost the forward more than the balance gains — 140 against
// 124 us per launch — and its rows + words instance has to give the sums of the rows-only one
template <typename Launch>
struct NodeRrTable {
    using Kernel = void (*)(const Launch);
    Kernel k[3][3];
};

#define NODE_RR_BITS(KERN, NB, R, S0, S1, S2) {KERN<NB, R, 0, S0>, KERN<NB, R, 1, S1>, KERN<NB, R, 2, S2>}
#define NODE_RR_TABLE(KERN, S0, S1, S2)                                                                                 \
    {{NODE_RR_BITS(KERN, 4, 4, S0, S1, S2), NODE_RR_BITS(KERN, 7, 1, S0, S1, S2), NODE_RR_BITS(KERN, 8, 4, S0, S1, S2)}}
#define NODE_RR_FWD_TABLE(KERN) NODE_RR_TABLE(KERN, 0, 1, 0)
#define NODE_RR_BWD_TABLE(KERN) NODE_RR_TABLE(KERN, 1, 1, 1)

// launch the instance of `t` for nets `hid` wide and this acts_bits over n rows, one 32-row tile per workgroup
template <typename Launch>
static void node_rr_start(const NodeRrTable<Launch>& t, const Launch& A, int hid, int n, int acts_bits,
                          size_t lds_floats, hipStream_t s) {
    hipLaunchKernelGGL(t.k[nlbac_node_rr_shape(hid)][acts_bits], dim3(nlbac_ceil_div(n, NLBAC_MLP_TILE)), dim3(256),
                       lds_floats * sizeof(float), s, A);
}

template <typename Launch>
static void node_rr_fwd_start(const NodeRrTable<Launch>& t, const Launch& A, int hid, int n, int acts_bits, hipStream_t s) {
    node_rr_start(t, A, hid, n, acts_bits, node_rr_fwd_lds_floats(), s);
}

template <typename Launch>
static void node_rr_bwd_start(const NodeRrTable<Launch>& t, const Launch& A, int hid, int n, int acts_bits, hipStream_t s) {
    node_rr_start(t, A, hid, n, acts_bits, node_rr_bwd_lds_floats(), s);
}
