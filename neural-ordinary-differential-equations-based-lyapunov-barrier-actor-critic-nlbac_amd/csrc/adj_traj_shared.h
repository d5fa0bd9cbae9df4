// What the two adjoint trajectory launches (node_adj_traj_kernels.hip, concat_adj_traj_kernels.hip) take beyond the
// one-step form: a RUN of N fine intervals walked last to first inside one launch, the tile's z = [y | a_x | a_c] in LDS
// from the run's top to its end.
//
// An OUTPUT interval (a control interval of rollout, [t[j-1], t[j]] of odeint_grid) is one or more fine intervals.  Where
// one begins in the backward sense (its upper end: begin[i] = k >= 0), y is reset to the forward's stored out[k+1], a_x
// becomes dout[k+1] + a_x (just dout[k+1] at the horizon's end: top, i = N-1) and a_c starts at zero; inside an output
// interval the whole z is carried from fine step to fine step.  Behind an output interval's last fine step a_c is its
// controls' gradient: du[k] (du_stride > 0: stacked, rollout) or du += a_c (du_stride = 0: summed, odeint_grid).  A run
// begins and ends at output-interval boundaries; `carry` hands z from one run's end to the next one's top, so that a
// horizon cut into several launches gives the bits of the one launch.
#pragma once

struct AdjTrajArgs {
    int N;                            // fine intervals of the run (walked N-1 .. 0)
    int top;                          // the run's top is the horizon's end: carry is not read, du (summed) starts here
    const float* hs;                  // [N] fine steps (device)
    const int* begin;                 // [N] the output interval whose upper end fine interval i is, or -1
    const float* out; int out_ld;     // [H+1][n][out_ld]: the forward's outputs, the state in the first n_s columns
    const float* dout;                // [H+1][n][n_s]
    const float* ctl; long ctl_stride;   // controls of output interval k at ctl + k * ctl_stride, [n][n_c]
    float* du; long du_stride;        // [H][n][n_c] stacked (stride n * n_c) or [n][n_c] summed (stride 0)
    float* carry;                     // [n][W]
    float* dK;                        // KEEP, control-affine form: [N*S][n][n_s] the cotangent of f_net's output, scaled
};

// The launchers' checks of a run's host copies (no launch): steps positive and finite, the markers in [-1, H), the top
// fine interval an output interval's upper end, N * S * n below 2^31.
static inline int nlbac_adj_traj_check(int n, int N, int H, int n_stages, const float* hs, const float* hs_host,
                                       const int* begin, const int* begin_host, const char* who) {
    NLBAC_REQUIRE(n >= 1 && N >= 1 && H >= 1 && n_stages >= 1, "%s: bad rows / intervals / stage count", who);
    NLBAC_REQUIRE((long)N * n_stages * n < (1L << 31), "%s: %d fine intervals x %d stages x %d rows is 2^31 or more", who, N, n_stages, n);
    if (nlbac_grid_steps_check(hs, hs_host, N, who)) return -1;
    NLBAC_REQUIRE(begin && begin_host, "%s: null pointer", who);
    for (int i = 0; i < N; ++i)
        NLBAC_REQUIRE(begin_host[i] >= -1 && begin_host[i] < H, "%s: fine interval %d marks output interval %d of %d", who, i, begin_host[i], H);
    NLBAC_REQUIRE(begin_host[N - 1] >= 0, "%s: a run begins at an output interval's upper end", who);
    return 0;
}
