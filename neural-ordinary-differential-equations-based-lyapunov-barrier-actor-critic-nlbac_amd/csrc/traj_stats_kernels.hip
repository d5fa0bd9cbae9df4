// Prediction-error statistics of a NODE rollout over trajectory windows, by look-ahead step and state component
// (nlbac_traj_err_stats; node_fit.traj_error_stats / validate_rollout, SAC_CBF_CLF.validate_node_windows).
//
// pred / target [H][n][n_s] float32, x0 [n][n_s], valid [n] (1 / 0, NULL: every window).  Everything is float64 from the
// load on: inputs are widened before the subtraction and no float32 sum is formed.  Two launches, no atomics, no
// election: workgroup (b, k) leaves its partials in the caller's scratch, one workgroup per step adds them in block order.
//
// Thread mapping.  One step's [n][n_s] rows are n n_s contiguous floats.  Of a workgroup's 256 lanes the first
// S = (256 / n_s) n_s are at work: lane t reads elements base + t + j S (j = 0, 1, ...), base a whole number of rows — so
// consecutive lanes read consecutive floats (coalesced; at worst 6 % of the lanes idle, n_s = 9 .. 15) and lane t stays
// on ONE component, c = t mod n_s: its five sums live in registers with no index arithmetic.  The lanes of a component
// are then added through LDS by one thread per (plane, component) in lane order.
#include "common.h"

#define TES_PLANES 5
#define TES_MAX_NS 16
#define TES_MAX_BLOCKS 128
#define TES_BLOCK_ELEMS 2048
// doubles a workgroup leaves in the scratch: five planes of n_s, then its count of valid windows
#define TES_PART(n_s) (TES_PLANES * (n_s) + 1)

static inline long traj_err_blocks(long n, int n_s) {
    long b = (n * n_s + TES_BLOCK_ELEMS - 1) / TES_BLOCK_ELEMS;
    if (b < 1) b = 1;
    return b < TES_MAX_BLOCKS ? b : TES_MAX_BLOCKS;
}

// NaN-keeping maximum (fmax drops a NaN operand)
__device__ __forceinline__ double nan_max(double a, double b) {
    if (a != a) return a;
    if (b != b) return b;
    return a > b ? a : b;
}

__global__ __launch_bounds__(256) void traj_err_partials_kernel(const float* __restrict__ pred,
                                                                const float* __restrict__ target,
                                                                const float* __restrict__ x0,
                                                                const float* __restrict__ valid, long n, int n_s,
                                                                double* __restrict__ scratch) {
    __shared__ double red[256][TES_PLANES];
    __shared__ int cnt[256];
    const int t = threadIdx.x, k = blockIdx.y, nb = gridDim.x;
    const int S = (256 / n_s) * n_s;
    const long rows_per_block = (n + nb - 1) / nb;
    const long row0 = (long)blockIdx.x * rows_per_block;
    const long row1 = row0 + rows_per_block < n ? row0 + rows_per_block : n;
    const float* pk = pred + (long)k * n * n_s;
    const float* tk = target + (long)k * n * n_s;
    double sse = 0.0, sae = 0.0, mx = 0.0, base = 0.0, tss = 0.0;
    int c_valid = 0;
    if (t < S) {
        const int c = t % n_s, rows_per_pass = S / n_s;
        long i = row0 + t / n_s;                          // the element's window: S / n_s further on with every pass
        for (long e = row0 * n_s + t; e < row1 * n_s; e += S, i += rows_per_pass) {
            if (valid && valid[i] == 0.f) continue;      // (an invalid window's values are never looked at)
            const double p = (double)pk[e], y = (double)tk[e], x = (double)x0[e];
            const double d = p - y, a = fabs(d), m = x - y;
            sse += d * d;
            sae += a;
            mx = nan_max(mx, a);
            base += m * m;
            tss += y * y;
            if (c == 0) ++c_valid;
        }
    }
    red[t][0] = sse; red[t][1] = sae; red[t][2] = mx; red[t][3] = base; red[t][4] = tss;
    cnt[t] = c_valid;
    __syncthreads();
    double* out = scratch + ((long)k * nb + blockIdx.x) * TES_PART(n_s);
    if (t < TES_PLANES * n_s) {
        const int p = t / n_s, c = t - p * n_s;
        double v = 0.0;
        if (p == 2) for (int l = c; l < S; l += n_s) v = nan_max(v, red[l][2]);
        else for (int l = c; l < S; l += n_s) v += red[l][p];
        out[t] = v;
    } else if (t == TES_PLANES * n_s) {
        long v = 0;
        for (int l = 0; l < S; l += n_s) v += cnt[l];
        out[t] = (double)v;                              // (< 2^31: exact)
    }
}

// stats [5][H][n_s]: workgroup k adds step k's partials in block order; nvalid: the counts of step 0's workgroups
__global__ __launch_bounds__(128) void traj_err_finish_kernel(const double* __restrict__ scratch, int nb, int H, int n_s,
                                                              double* __restrict__ stats, long* __restrict__ nvalid) {
    const int t = threadIdx.x, k = blockIdx.x;
    const double* part = scratch + (long)k * nb * TES_PART(n_s);
    if (t < TES_PLANES * n_s) {
        const int p = t / n_s, c = t - p * n_s;
        double v = 0.0;
        if (p == 2) for (int b = 0; b < nb; ++b) v = nan_max(v, part[(long)b * TES_PART(n_s) + t]);
        else for (int b = 0; b < nb; ++b) v += part[(long)b * TES_PART(n_s) + t];
        stats[((long)p * H + k) * n_s + c] = v;
    } else if (t == TES_PLANES * n_s && k == 0) {
        long v = 0;
        for (int b = 0; b < nb; ++b) v += (long)part[(long)b * TES_PART(n_s) + t];
        *nvalid = v;
    }
}

extern "C" int nlbac_traj_err_stats(const float* pred, const float* target, const float* x0, const float* valid, long n,
                                    int H, int n_s, double* scratch, long scratch_doubles, double* stats, long* nvalid,
                                    nlbac_stream_t s) {
    NLBAC_REQUIRE(pred && target && x0 && scratch && stats && nvalid, "nlbac_traj_err_stats: null pointer");
    NLBAC_REQUIRE(n_s >= 1 && n_s <= TES_MAX_NS, "nlbac_traj_err_stats: n_s must lie in 1 .. %d (got %d)", TES_MAX_NS, n_s);
    NLBAC_REQUIRE(H >= 1 && H <= 65535, "nlbac_traj_err_stats: H must lie in 1 .. 65535 (got %d)", H);
    NLBAC_REQUIRE(n >= 1 && n < (1L << 31), "nlbac_traj_err_stats: n must lie in 1 .. 2^31 - 1 (got %ld)", n);
    const long nb = traj_err_blocks(n, n_s);
    NLBAC_REQUIRE(scratch_doubles >= (long)H * nb * TES_PART(n_s),
                  "nlbac_traj_err_stats: scratch holds %ld doubles, H * blocks * (5 n_s + 1) = %ld are needed",
                  scratch_doubles, (long)H * nb * TES_PART(n_s));
    hipLaunchKernelGGL(traj_err_partials_kernel, dim3((unsigned)nb, (unsigned)H), dim3(256), 0, (hipStream_t)s, pred,
                       target, x0, valid, n, n_s, scratch);
    NLBAC_CHECK_LAUNCH("nlbac_traj_err_stats");
    hipLaunchKernelGGL(traj_err_finish_kernel, dim3((unsigned)H), dim3(128), 0, (hipStream_t)s, scratch, (int)nb, H, n_s,
                       stats, nvalid);
    NLBAC_CHECK_LAUNCH("nlbac_traj_err_stats");
    return 0;
}
