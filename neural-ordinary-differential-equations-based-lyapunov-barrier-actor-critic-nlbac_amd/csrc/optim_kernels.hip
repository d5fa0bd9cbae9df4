// Adam (torch.optim.Adam single-tensor arithmetic), gradient-slab reduction and
// soft target update.  Replaces torch.optim.Adam.step at
// U/sac_cbf_clf/sac_cbf_clf.py:249-255,284-308, U/sac_cbf_clf/model.py:258 and
// soft_update at U/sac_cbf_clf/utils.py:75-79.
//
// HBM-bound streaming kernels: one float4 per lane, grid capped at 2048 blocks.
#include <cstdint>
#include "common.h"
#include "philox.h"

thread_local char nlbac_err_buf[512] = "";

extern "C" int nlbac_abi_version(void) { return NLBAC_ABI_VERSION; }
extern "C" const char* nlbac_last_error(void) { return nlbac_err_buf; }

struct AdamState {
    int step;
    float step_size;   // lr / (1 - beta1^t)
    float bc2_sqrt;    // sqrt(1 - beta2^t)
    unsigned ticket;   // nlbac_adam_fused: workgroups that have finished (zero between launches)
};

__global__ void adam_prepare_kernel(AdamState* st, double lr) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        const int t = st->step + 1;
        st->step = t;
        const double bc1 = 1.0 - pow(0.9, (double)t);
        const double bc2 = 1.0 - pow(0.999, (double)t);
        st->step_size = (float)(lr / bc1);
        st->bc2_sqrt = (float)sqrt(bc2);
    }
}

__device__ __forceinline__ float adam_one(float& p, float& m, float& v, float g, float step_size, float bc2_sqrt) {
    // exp_avg.lerp_(grad, 1-beta1); exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1-beta2)
    // (the scalars are python doubles cast to fp32 at use, as ATen does)
    m = m + (g - m) * (float)(1.0 - 0.9);
    v = v * 0.999f + ((float)(1.0 - 0.999) * g) * g;
    const float denom = sqrtf(v) / bc2_sqrt + 1e-8f;
    p = p + ((-step_size) * m) / denom;   // addcdiv_: self + value * t1 / t2
    return p;
}

__global__ __launch_bounds__(256) void adam_step_kernel(float* __restrict__ p, float* __restrict__ m,
                                                        float* __restrict__ v, const float* __restrict__ grad,
                                                        int n_slabs, long slab_stride, long n,
                                                        const AdamState* __restrict__ st,
                                                        float* __restrict__ target, float tau) {
    const float step_size = st->step_size, bc2_sqrt = st->bc2_sqrt;
    const long n4 = n >> 2;
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        float4 g = reinterpret_cast<const float4*>(grad)[i];
        for (int s = 1; s < n_slabs; ++s) {
            const float4 gs = reinterpret_cast<const float4*>(grad + s * slab_stride)[i];
            g.x += gs.x; g.y += gs.y; g.z += gs.z; g.w += gs.w;
        }
        float4 pp = reinterpret_cast<float4*>(p)[i];
        float4 mm = reinterpret_cast<float4*>(m)[i];
        float4 vv = reinterpret_cast<float4*>(v)[i];
        adam_one(pp.x, mm.x, vv.x, g.x, step_size, bc2_sqrt);
        adam_one(pp.y, mm.y, vv.y, g.y, step_size, bc2_sqrt);
        adam_one(pp.z, mm.z, vv.z, g.z, step_size, bc2_sqrt);
        adam_one(pp.w, mm.w, vv.w, g.w, step_size, bc2_sqrt);
        reinterpret_cast<float4*>(p)[i] = pp;
        reinterpret_cast<float4*>(m)[i] = mm;
        reinterpret_cast<float4*>(v)[i] = vv;
        if (target) {
            float4 t = reinterpret_cast<float4*>(target)[i];
            t.x = t.x * (1.0f - tau) + pp.x * tau; t.y = t.y * (1.0f - tau) + pp.y * tau;
            t.z = t.z * (1.0f - tau) + pp.z * tau; t.w = t.w * (1.0f - tau) + pp.w * tau;
            reinterpret_cast<float4*>(target)[i] = t;
        }
    }
    // tail (n not a multiple of 4)
    for (long i = (n4 << 2) + (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        float g = grad[i];
        for (int s = 1; s < n_slabs; ++s) g += grad[s * slab_stride + i];
        float pp = p[i], mm = m[i], vv = v[i];
        adam_one(pp, mm, vv, g, step_size, bc2_sqrt);
        p[i] = pp; m[i] = mm; v[i] = vv;
        if (target) target[i] = target[i] * (1.0f - tau) + pp * tau;
    }
}

// One launch per optimiser step: ++step and its bias corrections (adam_prepare), the slab sum + Adam + Polyak update
// (adam_step), and the refresh of the MFMA-fragment copies of the weights (mlp_pack) through a scatter table: for
// parameter i, scat[SLOTS i + k] are the device addresses of its fragment slots (forward / backward pack, and the RR
// packs of nets that have them: SLOTS = 2 or 4; 0 = none;
// biases and skinny layers are read from the flat parameters).  Every workgroup derives the step constants from the
// still un-incremented counter; the workgroup that finishes last publishes the new counter.
template <int SLOTS>
__device__ __forceinline__ void scatter_n(const unsigned long long* __restrict__ scat, long i, float val) {
#pragma unroll
    for (int k = 0; k < SLOTS / 2; ++k) {
        const ulonglong2 ab = reinterpret_cast<const ulonglong2*>(scat)[i * (SLOTS / 2) + k];   // two slots per load
        if (ab.x) *reinterpret_cast<float*>(ab.x) = val;
        if (ab.y) *reinterpret_cast<float*>(ab.y) = val;
    }
}
#define scatter2 scatter_n<SLOTS>

// sum of the gradient slabs at float4 index i, in slab order (the additions are sequential as before; the loads of
// four slabs are issued together instead of one per loop trip - the trips were a chain of exposed memory latencies)
__device__ __forceinline__ float4 slab_sum4(const float* __restrict__ grad, int n_slabs, long slab_stride, long i) {
    float4 g = reinterpret_cast<const float4*>(grad)[i];
    int s = 1;
    for (; s + 3 < n_slabs; s += 4) {
        const float4 a = reinterpret_cast<const float4*>(grad + (long)s * slab_stride)[i];
        const float4 b = reinterpret_cast<const float4*>(grad + (long)(s + 1) * slab_stride)[i];
        const float4 c = reinterpret_cast<const float4*>(grad + (long)(s + 2) * slab_stride)[i];
        const float4 d = reinterpret_cast<const float4*>(grad + (long)(s + 3) * slab_stride)[i];
        g.x += a.x; g.y += a.y; g.z += a.z; g.w += a.w;
        g.x += b.x; g.y += b.y; g.z += b.z; g.w += b.w;
        g.x += c.x; g.y += c.y; g.z += c.z; g.w += c.w;
        g.x += d.x; g.y += d.y; g.z += d.z; g.w += d.w;
    }
    for (; s < n_slabs; ++s) {
        const float4 a = reinterpret_cast<const float4*>(grad + (long)s * slab_stride)[i];
        g.x += a.x; g.y += a.y; g.z += a.z; g.w += a.w;
    }
    return g;
}

// temperatures refreshed by the step itself: alpha = exp(log_alpha) for up to two log_alpha entries of this arena
// (sac_cbf_clf.py:297, 308), written by the thread that has just stepped the entry
// mirror: the last workgroup of the step also sends `n_mirror` floats at `mirror_src` (the agent's scalars block: the
// losses this update returns) to `mirror_dst`, a pinned HOST buffer the device writes directly — the update's last
// launch delivers its results itself instead of a copy launch behind it, on which the host would wait.  Entries the
// step refreshes (the temperatures) go out from the thread that computes them.
struct AlphaRefresh { long off[2]; float* dst[2]; const float* mirror_src; float* mirror_dst; int n_mirror; };
__device__ __forceinline__ void alpha_refresh(const AlphaRefresh& AR, long e, float p_new) {
#pragma unroll
    for (int k = 0; k < 2; ++k)
        if (e == AR.off[k]) {
            const float a = expf(p_new);
            *AR.dst[k] = a;
            if (AR.mirror_dst) {
                const long i = AR.dst[k] - AR.mirror_src;
                if (i >= 0 && i < AR.n_mirror) AR.mirror_dst[i] = a;
            }
        }
}

template <int SLOTS>
__global__ __launch_bounds__(256) void adam_fused_kernel(float* __restrict__ p, float* __restrict__ m,
                                                         float* __restrict__ v, const float* __restrict__ grad,
                                                         int n_slabs, long slab_stride, long n, AdamState* st, double lr,
                                                         float* __restrict__ target, float tau,
                                                         const unsigned long long* __restrict__ scat,
                                                         const unsigned long long* __restrict__ scat_t,
                                                         const AlphaRefresh AR) {
    __shared__ float s_const[2];
    __shared__ int s_step;
    if (threadIdx.x == 0) {
        const int t = __hip_atomic_load(&st->step, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1;
        const double bc1 = 1.0 - pow(0.9, (double)t);
        const double bc2 = 1.0 - pow(0.999, (double)t);
        s_const[0] = (float)(lr / bc1);
        s_const[1] = (float)sqrt(bc2);
        s_step = t;
    }
    __syncthreads();
    const float step_size = s_const[0], bc2_sqrt = s_const[1];
    const long n4 = n >> 2;
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        float4 g = slab_sum4(grad, n_slabs, slab_stride, i);
        float4 pp = reinterpret_cast<float4*>(p)[i];
        float4 mm = reinterpret_cast<float4*>(m)[i];
        float4 vv = reinterpret_cast<float4*>(v)[i];
        adam_one(pp.x, mm.x, vv.x, g.x, step_size, bc2_sqrt);
        adam_one(pp.y, mm.y, vv.y, g.y, step_size, bc2_sqrt);
        adam_one(pp.z, mm.z, vv.z, g.z, step_size, bc2_sqrt);
        adam_one(pp.w, mm.w, vv.w, g.w, step_size, bc2_sqrt);
        reinterpret_cast<float4*>(p)[i] = pp;
        reinterpret_cast<float4*>(m)[i] = mm;
        reinterpret_cast<float4*>(v)[i] = vv;
        if (AR.off[0] >= 0 || AR.off[1] >= 0) {
            alpha_refresh(AR, 4 * i + 0, pp.x); alpha_refresh(AR, 4 * i + 1, pp.y);
            alpha_refresh(AR, 4 * i + 2, pp.z); alpha_refresh(AR, 4 * i + 3, pp.w);
        }
        if (scat) {
            scatter2(scat, 4 * i + 0, pp.x); scatter2(scat, 4 * i + 1, pp.y);
            scatter2(scat, 4 * i + 2, pp.z); scatter2(scat, 4 * i + 3, pp.w);
        }
        if (target) {
            float4 t = reinterpret_cast<float4*>(target)[i];
            t.x = t.x * (1.0f - tau) + pp.x * tau; t.y = t.y * (1.0f - tau) + pp.y * tau;
            t.z = t.z * (1.0f - tau) + pp.z * tau; t.w = t.w * (1.0f - tau) + pp.w * tau;
            reinterpret_cast<float4*>(target)[i] = t;
            if (scat_t) {
                scatter2(scat_t, 4 * i + 0, t.x); scatter2(scat_t, 4 * i + 1, t.y);
                scatter2(scat_t, 4 * i + 2, t.z); scatter2(scat_t, 4 * i + 3, t.w);
            }
        }
    }
    for (long i = (n4 << 2) + (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        float g = grad[i];
        for (int s = 1; s < n_slabs; ++s) g += grad[s * slab_stride + i];
        float pp = p[i], mm = m[i], vv = v[i];
        adam_one(pp, mm, vv, g, step_size, bc2_sqrt);
        p[i] = pp; m[i] = mm; v[i] = vv;
        alpha_refresh(AR, i, pp);
        if (scat) scatter2(scat, i, pp);
        if (target) {
            const float t = target[i] * (1.0f - tau) + pp * tau;
            target[i] = t;
            if (scat_t) scatter2(scat_t, i, t);
        }
    }
    __syncthreads();                                   // every wave of this block has read the constants
    __shared__ int s_is_last;
    if (threadIdx.x == 0) {
        s_is_last = 0;
        // relaxed: every workgroup consumed st->step (it computed its constants from it) before the barrier above, so
        // the counter may move once the last ticket is drawn; no agent-scope release per workgroup (that would write the
        // XCD's L2 back behind every block's parameter stores)
        const unsigned ticket = __hip_atomic_fetch_add(&st->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (ticket == gridDim.x - 1) {                 // all workgroups have read st->step by now
            __hip_atomic_store(&st->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            st->step_size = step_size;
            st->bc2_sqrt = bc2_sqrt;
            __hip_atomic_store(&st->step, s_step, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            s_is_last = 1;
        }
    }
    if (!AR.mirror_dst) return;
    __syncthreads();
    if (s_is_last)                                     // (written by earlier launches, except the refreshed entries)
        for (int i = threadIdx.x; i < AR.n_mirror; i += blockDim.x) {
            const bool refreshed = (AR.off[0] >= 0 && AR.dst[0] == AR.mirror_src + i) ||
                                   (AR.off[1] >= 0 && AR.dst[1] == AR.mirror_src + i);
            if (!refreshed) AR.mirror_dst[i] = AR.mirror_src[i];
        }
}

__global__ __launch_bounds__(256) void reduce_slabs_kernel(float* __restrict__ out, const float* __restrict__ grad,
                                                           int n_slabs, long slab_stride, long n) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        float g = grad[i];
        for (int s = 1; s < n_slabs; ++s) g += grad[s * slab_stride + i];
        out[i] = g;
    }
}

__global__ __launch_bounds__(256) void soft_update_kernel(float* __restrict__ target, const float* __restrict__ src,
                                                          long n, float tau) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        target[i] = target[i] * (1.0f - tau) + src[i] * tau;
}

__global__ __launch_bounds__(256) void axpby_kernel(float a, const float* x, float b, const float* y, long n, float* out) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        out[i] = a * x[i] + (y ? b * y[i] : 0.f);
}

__global__ __launch_bounds__(256) void fill_kernel(float* p, float v, long n) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) p[i] = v;
}

// out[c] = mul * sum_b partials[b][c]   (fixed order; one thread per column)
__global__ void sum_partials_kernel(const float* partials, int n_blk, int n_cols, float mul, float* out) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_cols) return;
    float s = 0.f;
    for (int b = 0; b < n_blk; ++b) s += partials[(long)b * n_cols + c];
    out[c] = s * mul;
}

static inline int stream_grid(long n, int per_thread = 1) {
    long b = (n / per_thread + 255) / 256;
    if (b < 1) b = 1;
    if (b > 2048) b = 2048;
    return (int)b;
}

extern "C" int nlbac_adam_prepare(void* state, double lr, nlbac_stream_t s) {
    NLBAC_REQUIRE(state, "nlbac_adam_prepare: null state");
    hipLaunchKernelGGL(adam_prepare_kernel, dim3(1), dim3(64), 0, (hipStream_t)s, (AdamState*)state, lr);
    NLBAC_CHECK_LAUNCH("nlbac_adam_prepare");
    return 0;
}

extern "C" int nlbac_adam_step(float* p, float* m, float* v, const float* grad, int n_slabs, long slab_stride,
                               long n, const void* state, float* target, float tau, nlbac_stream_t s) {
    NLBAC_REQUIRE(p && m && v && grad && state, "nlbac_adam_step: null pointer");
    NLBAC_REQUIRE(n_slabs >= 1 && n >= 1, "nlbac_adam_step: bad sizes");
    NLBAC_REQUIRE(((uintptr_t)p | (uintptr_t)m | (uintptr_t)v | (uintptr_t)grad | (uintptr_t)target) % 16 == 0 &&
                      slab_stride % 4 == 0,
                  "nlbac_adam_step: buffers must be 16-byte aligned");
    hipLaunchKernelGGL(adam_step_kernel, dim3(stream_grid(n, 4)), dim3(256), 0, (hipStream_t)s, p, m, v, grad,
                       n_slabs, slab_stride, n, (const AdamState*)state, (tau >= 0.f) ? target : nullptr, tau);
    NLBAC_CHECK_LAUNCH("nlbac_adam_step");
    return 0;
}

extern "C" int nlbac_adam_fused(float* p, float* m, float* v, const float* grad, int n_slabs, long slab_stride, long n,
                                void* state, double lr, float* target, float tau, const void* scatter,
                                const void* scatter_target, int scatter_slots, int n_alpha, const long* alpha_off,
                                float* const* alpha_dst, const float* mirror_src, float* mirror_dst, int n_mirror,
                                nlbac_stream_t s) {
    NLBAC_REQUIRE(p && m && v && grad && state, "nlbac_adam_fused: null pointer");
    NLBAC_REQUIRE(scatter_slots == 2 || scatter_slots == 4 || (!scatter && !scatter_target),
                  "nlbac_adam_fused: scatter tables hold 2 or 4 slots per parameter");
    NLBAC_REQUIRE(n_alpha >= 0 && n_alpha <= 2 && (n_alpha == 0 || (alpha_off && alpha_dst)), "nlbac_adam_fused: bad alpha refresh");
    AlphaRefresh AR;
    AR.off[0] = AR.off[1] = -1; AR.dst[0] = AR.dst[1] = nullptr;
    NLBAC_REQUIRE((mirror_dst == nullptr) || (mirror_src && n_mirror > 0 && n_mirror <= 1024), "nlbac_adam_fused: bad mirror");
    AR.mirror_src = mirror_src; AR.mirror_dst = mirror_dst; AR.n_mirror = mirror_dst ? n_mirror : 0;
    for (int k = 0; k < n_alpha; ++k) {
        NLBAC_REQUIRE(alpha_off[k] >= 0 && alpha_off[k] < n && alpha_dst[k], "nlbac_adam_fused: alpha entry out of range");
        AR.off[k] = alpha_off[k]; AR.dst[k] = alpha_dst[k];
    }
    NLBAC_REQUIRE(n_slabs >= 1 && n >= 1 && lr > 0.0, "nlbac_adam_fused: bad sizes");
    NLBAC_REQUIRE(((uintptr_t)p | (uintptr_t)m | (uintptr_t)v | (uintptr_t)grad | (uintptr_t)target) % 16 == 0 &&
                      slab_stride % 4 == 0 && ((uintptr_t)scatter | (uintptr_t)scatter_target) % 16 == 0,   // (two slots per load)
                  "nlbac_adam_fused: buffers must be 16-byte aligned");
    NLBAC_REQUIRE(!scatter_target || (target && tau >= 0.f), "nlbac_adam_fused: scatter_target without a target");
    hipLaunchKernelGGL((scatter_slots == 4 ? adam_fused_kernel<4> : adam_fused_kernel<2>), dim3(stream_grid(n, 4)), dim3(256),
                       0, (hipStream_t)s, p, m, v, grad, n_slabs, slab_stride, n, (AdamState*)state, lr,
                       (tau >= 0.f) ? target : nullptr, tau, (const unsigned long long*)scatter,
                       (const unsigned long long*)scatter_target, AR);
    NLBAC_CHECK_LAUNCH("nlbac_adam_fused");
    return 0;
}

extern "C" int nlbac_reduce_slabs(float* out, const float* grad, int n_slabs, long slab_stride, long n, nlbac_stream_t s) {
    NLBAC_REQUIRE(out && grad && n_slabs >= 1, "nlbac_reduce_slabs: bad arguments");
    hipLaunchKernelGGL(reduce_slabs_kernel, dim3(stream_grid(n)), dim3(256), 0, (hipStream_t)s, out, grad, n_slabs, slab_stride, n);
    NLBAC_CHECK_LAUNCH("nlbac_reduce_slabs");
    return 0;
}

extern "C" int nlbac_soft_update(float* target, const float* src, long n, float tau, nlbac_stream_t s) {
    NLBAC_REQUIRE(target && src, "nlbac_soft_update: null pointer");
    hipLaunchKernelGGL(soft_update_kernel, dim3(stream_grid(n)), dim3(256), 0, (hipStream_t)s, target, src, n, tau);
    NLBAC_CHECK_LAUNCH("nlbac_soft_update");
    return 0;
}

extern "C" int nlbac_axpby(float a, const float* x, float b, const float* y, long n, float* out, nlbac_stream_t s) {
    NLBAC_REQUIRE(x && out, "nlbac_axpby: null pointer");
    hipLaunchKernelGGL(axpby_kernel, dim3(stream_grid(n)), dim3(256), 0, (hipStream_t)s, a, x, b, y, n, out);
    NLBAC_CHECK_LAUNCH("nlbac_axpby");
    return 0;
}

extern "C" int nlbac_fill(float* p, float v, long n, nlbac_stream_t s) {
    NLBAC_REQUIRE(p, "nlbac_fill: null pointer");
    hipLaunchKernelGGL(fill_kernel, dim3(stream_grid(n)), dim3(256), 0, (hipStream_t)s, p, v, n);
    NLBAC_CHECK_LAUNCH("nlbac_fill");
    return 0;
}

extern "C" int nlbac_sum_partials(const float* partials, int n_blk, int n_cols, float mul, float* out, nlbac_stream_t s) {
    NLBAC_REQUIRE(partials && out && n_blk >= 1 && n_cols >= 1, "nlbac_sum_partials: bad arguments");
    hipLaunchKernelGGL(sum_partials_kernel, dim3(nlbac_ceil_div(n_cols, 64)), dim3(64), 0, (hipStream_t)s, partials, n_blk, n_cols, mul, out);
    NLBAC_CHECK_LAUNCH("nlbac_sum_partials");
    return 0;
}


// ---------------------------------------------------------------------------
// Replay minibatch gather (replay_memory.py:21-25 on the device): dst[r] = src[idx[r]] for rows of ld floats
// (ld % 4 == 0, 16-byte aligned rows): one lane per float4, consecutive lanes on consecutive 16-byte pieces of a row.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gather_rows_kernel(const float4* __restrict__ src, int ld4,
                                                          const long* __restrict__ idx, long n_rows, long src_rows,
                                                          float4* __restrict__ dst) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_rows * ld4) return;
    const long r = t / ld4;
    const int c = (int)(t - r * ld4);
    long j = idx[r];
    j = j < 0 ? 0 : (j >= src_rows ? src_rows - 1 : j);       // never read outside the buffer
    dst[r * ld4 + c] = src[j * ld4 + c];
}

// ---------------------------------------------------------------------------
// Device-side draw of a minibatch (device_rng mode): row indices uniform on [0, src_rows) with
// replacement, the gather into minibatch layout and the N(0,1) policy noise of the update, in ONE launch (the update
// boundary is where the host is the bottleneck).  The draw itself is philox.h's sample_rows_body.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sample_rows_kernel(const float4* __restrict__ src, int ld4, long n_rows,
                                                          long src_rows, float4* __restrict__ dst,
                                                          float* __restrict__ eps, long n_eps,
                                                          unsigned long long seed, unsigned long long draw) {
    sample_rows_body((long)blockIdx.x * 256 + threadIdx.x, src, ld4, n_rows, src_rows, dst, eps, n_eps, seed, draw);
}

extern "C" int nlbac_sample_rows(const float* src, long src_rows, int ld, long n_rows, float* dst, float* eps,
                                 long n_eps, unsigned long long seed, unsigned long long draw, nlbac_stream_t s) {
    NLBAC_REQUIRE(src && dst && src_rows >= 1 && src_rows < (1L << 32) && n_rows >= 1 && n_eps >= 0,
                  "nlbac_sample_rows: bad arguments");
    NLBAC_REQUIRE(ld >= 4 && ld % 4 == 0 && ((uintptr_t)src % 16) == 0 && ((uintptr_t)dst % 16) == 0,
                  "nlbac_sample_rows: rows must be whole float4s (ld %d)", ld);
    NLBAC_REQUIRE(eps || n_eps == 0, "nlbac_sample_rows: n_eps without a buffer");
    const long total = n_rows * (ld / 4), q = (n_eps + 3) / 4;
    const long threads = total > q ? total : q;
    hipLaunchKernelGGL(sample_rows_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)s,
                       (const float4*)src, ld / 4, n_rows, src_rows, (float4*)dst, eps, n_eps, seed, draw);
    NLBAC_CHECK_LAUNCH("nlbac_sample_rows");
    return 0;
}

// n_blocks blocks of block_len contiguous dwords each, block b at src + b * src_stride -> dst + b * dst_stride
// (a row range of a stage-major buffer: one block per stage).  Moves bits: float and int32 buffers alike.
__global__ __launch_bounds__(256) void copy_blocks_kernel(const float* __restrict__ src, long src_stride,
                                                          float* __restrict__ dst, long dst_stride, long block_len,
                                                          long n_blocks) {
    const long total = block_len * n_blocks, stride = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
        const long b = i / block_len, j = i - b * block_len;
        dst[b * dst_stride + j] = src[b * src_stride + j];
    }
}

extern "C" int nlbac_copy_blocks(const void* src, long src_stride, void* dst, long dst_stride, long block_len,
                                 long n_blocks, nlbac_stream_t s) {
    NLBAC_REQUIRE(src && dst && block_len >= 1 && n_blocks >= 1 && src_stride >= block_len && dst_stride >= block_len,
                  "nlbac_copy_blocks: bad arguments");
    hipLaunchKernelGGL(copy_blocks_kernel, dim3(stream_grid(block_len * n_blocks)), dim3(256), 0, (hipStream_t)s,
                       (const float*)src, src_stride, (float*)dst, dst_stride, block_len, n_blocks);
    NLBAC_CHECK_LAUNCH("nlbac_copy_blocks");
    return 0;
}

extern "C" int nlbac_gather_rows(const float* src, long src_rows, int ld, const long* idx, long n_rows, float* dst,
                                 nlbac_stream_t s) {
    NLBAC_REQUIRE(src && idx && dst && src_rows >= 1 && n_rows >= 1, "nlbac_gather_rows: bad arguments");
    NLBAC_REQUIRE(ld >= 4 && ld % 4 == 0 && ((uintptr_t)src % 16) == 0 && ((uintptr_t)dst % 16) == 0,
                  "nlbac_gather_rows: rows must be whole float4s (ld %d)", ld);
    const long total = n_rows * (ld / 4);
    hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)s,
                       (const float4*)src, ld / 4, idx, n_rows, src_rows, (float4*)dst);
    NLBAC_CHECK_LAUNCH("nlbac_gather_rows");
    return 0;
}

// ---------------------------------------------------------------------------
// Trajectory windows from the replay ring (multi-step NODE fit): n windows of H rows each, `stride` rows between
// consecutive steps of one window (1, or the lane count of a vectorised driver that pushes one row per lane per step).
//   oldest = (src_rows == cap) ? head : 0          the oldest row (head: the ring's write position)
//   a0     = (idx - oldest) mod cap                 the start row's rank in push order
//   step k = the row of rank a0 + k stride, i.e. row (oldest + a0 + k stride) mod cap
// A window is valid iff (a) a0 + (H-1) stride < src_rows — it neither runs past the newest row nor steps over the write
// head — and (b) for every k < H-1 the obs_dim 32-bit words at nobs_col of step k equal, bit for bit (compared as
// integers), the words at obs_col of step k+1: an episode's next observation IS its next row's observation, and a reset
// or a termination — which `mask` cannot tell from a time-limit reset — breaks the chain.  Rows of an invalid window are
// still written (nothing downstream reads garbage): step k is the row of rank min(a0 + k stride, src_rows - 1).
// Outputs: dst [H][n][ld]; valid [n] 1.0f / 0.0f; counts [ceil(n / 256)] valid windows per 256-window block (plain
// stores, no atomics).  Grid (ceil(n / 256), H + 1): workgroup (b, k < H) moves step k of block b's 256 windows, one lane
// per float4, consecutive lanes on consecutive 16-byte pieces of a row; workgroup (b, H) checks the block's windows, one
// lane per compared word (consecutive lanes on consecutive words of a step), so neither a window's H rows nor its
// continuity compare run on one lane.  IDX false: the start rows are drawn here, uniform on [0, src_rows) with
// replacement, Philox counter (draw, window, 0) as sample_rows_kernel draws its rows.
// ---------------------------------------------------------------------------
template <bool IDX>
__global__ __launch_bounds__(256) void gather_windows_kernel(const float4* __restrict__ src, int ld4, long src_rows,
                                                             long cap, long head, const long* __restrict__ idx, long n,
                                                             int H, long stride, int obs_col, int nobs_col, int obs_dim,
                                                             float4* __restrict__ dst, float* __restrict__ valid,
                                                             int* __restrict__ counts, unsigned long long seed,
                                                             unsigned long long draw) {
    __shared__ long s_a0[256];
    __shared__ int s_bad[256];
    __shared__ float s_red[4];
    const long w0 = (long)blockIdx.x * 256;
    const int nw = (int)((n - w0) < 256 ? (n - w0) : 256);          // windows of this block
    const long oldest = (src_rows == cap) ? head : 0;
    const long last = src_rows - 1;
    if ((int)threadIdx.x < nw) {
        long j;
        if (IDX) {
            j = idx[w0 + threadIdx.x];
            j = j < 0 ? 0 : (j > last ? last : j);                   // never read outside the buffer
        } else {
            const uint2 key = make_uint2((unsigned)seed, (unsigned)(seed >> 32));
            const uint4 x = philox4x32_10(make_uint4((unsigned)draw, (unsigned)(draw >> 32), (unsigned)(w0 + threadIdx.x), 0u), key);
            j = (long)(((unsigned long long)x.x * (unsigned long long)src_rows) >> 32);
        }
        long a0 = j - oldest;
        if (a0 < 0) a0 += cap;
        s_a0[threadIdx.x] = a0;
        s_bad[threadIdx.x] = (a0 + (long)(H - 1) * stride < src_rows) ? 0 : 1;      // (a)
    }
    __syncthreads();
    const int k = blockIdx.y;
    if (k < H) {
        const int items = nw * ld4;
        for (int i = threadIdx.x; i < items; i += 256) {
            const int w = i / ld4, c = i - w * ld4;
            long rank = s_a0[w] + (long)k * stride;
            rank = rank > last ? last : rank;
            const long row = (oldest + rank) % cap;
            dst[((long)k * n + w0 + w) * ld4 + c] = src[row * ld4 + c];
        }
        return;
    }
    // (b): word j of the link k -> k+1 of window w; a lane that sees a difference flags the window (every writer
    // stores the same value)
    const unsigned* words = reinterpret_cast<const unsigned*>(src);
    const long ld = 4L * ld4;
    const int per_w = (H - 1) * obs_dim;
    const long items = (long)nw * per_w;
    for (long i = threadIdx.x; i < items; i += 256) {
        const int w = (int)(i / per_w), r = (int)(i - (long)w * per_w);
        const int kk = r / obs_dim, j = r - kk * obs_dim;
        long r0 = s_a0[w] + (long)kk * stride, r1 = r0 + stride;
        r0 = r0 > last ? last : r0;
        r1 = r1 > last ? last : r1;
        const unsigned a = words[((oldest + r0) % cap) * ld + nobs_col + j];
        const unsigned b = words[((oldest + r1) % cap) * ld + obs_col + j];
        if (a != b) s_bad[w] = 1;
    }
    __syncthreads();
    float v[1] = {0.f};
    if ((int)threadIdx.x < nw) {
        v[0] = s_bad[threadIdx.x] ? 0.f : 1.f;
        valid[w0 + threadIdx.x] = v[0];
    }
    block_sum_256<1>(v, s_red);                                      // (<= 256 ones: exact)
    if (threadIdx.x == 0) counts[blockIdx.x] = (int)v[0];
}

static int windows_check(const float* src, long src_rows, long cap, long head, int ld, long n, int H, long stride,
                         int obs_col, int nobs_col, int obs_dim, const float* dst, const float* valid, const int* counts,
                         const char* who) {
    NLBAC_REQUIRE(src && dst && valid && counts, "%s: null pointer", who);
    NLBAC_REQUIRE(cap >= 1 && src_rows >= 1 && src_rows <= cap && cap < (1L << 32) && head >= 0 && head < cap,
                  "%s: bad ring (rows %ld, capacity %ld, head %ld)", who, src_rows, cap, head);
    NLBAC_REQUIRE(n >= 1 && H >= 1 && H < 65535 && stride >= 1 && stride < (1L << 32) && (n + 255) / 256 < (1L << 31),
                  "%s: bad window count / horizon / stride", who);
    NLBAC_REQUIRE(ld >= 4 && ld % 4 == 0 && ((uintptr_t)src % 16) == 0 && ((uintptr_t)dst % 16) == 0,
                  "%s: rows must be whole float4s (ld %d)", who, ld);
    NLBAC_REQUIRE(obs_dim >= 0 && obs_col >= 0 && nobs_col >= 0 && obs_col + obs_dim <= ld && nobs_col + obs_dim <= ld &&
                      (long)(H - 1) * obs_dim < (1L << 22),
                  "%s: the observation columns must lie inside a row", who);
    return 0;
}

#define WINDOWS_GRID(n, H) dim3((unsigned)(((n) + 255) / 256), (unsigned)((H) + 1)), dim3(256), 0, (hipStream_t)s

extern "C" int nlbac_gather_windows(const float* src, long src_rows, long cap, long head, int ld, const long* idx, long n,
                                    int H, long stride, int obs_col, int nobs_col, int obs_dim, float* dst, float* valid,
                                    int* counts, nlbac_stream_t s) {
    if (windows_check(src, src_rows, cap, head, ld, n, H, stride, obs_col, nobs_col, obs_dim, dst, valid, counts,
                      "nlbac_gather_windows"))
        return 1;
    NLBAC_REQUIRE(idx, "nlbac_gather_windows: null pointer");
    hipLaunchKernelGGL(gather_windows_kernel<true>, WINDOWS_GRID(n, H), (const float4*)src, ld / 4, src_rows, cap, head,
                       idx, n, H, stride, obs_col, nobs_col, obs_dim, (float4*)dst, valid, counts, 0ull, 0ull);
    NLBAC_CHECK_LAUNCH("nlbac_gather_windows");
    return 0;
}

extern "C" int nlbac_sample_windows(const float* src, long src_rows, long cap, long head, int ld, long n, int H,
                                    long stride, int obs_col, int nobs_col, int obs_dim, float* dst, float* valid,
                                    int* counts, unsigned long long seed, unsigned long long draw, nlbac_stream_t s) {
    if (windows_check(src, src_rows, cap, head, ld, n, H, stride, obs_col, nobs_col, obs_dim, dst, valid, counts,
                      "nlbac_sample_windows"))
        return 1;
    NLBAC_REQUIRE(n < (1L << 32), "nlbac_sample_windows: the Philox counter holds 2^32 windows per draw");
    hipLaunchKernelGGL(gather_windows_kernel<false>, WINDOWS_GRID(n, H), (const float4*)src, ld / 4, src_rows, cap, head,
                       (const long*)nullptr, n, H, stride, obs_col, nobs_col, obs_dim, (float4*)dst, valid, counts, seed,
                       draw);
    NLBAC_CHECK_LAUNCH("nlbac_sample_windows");
    return 0;
}
