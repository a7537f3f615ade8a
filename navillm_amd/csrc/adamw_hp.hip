// AdamW for the bf16 LM group with more state precision than bf16 (include/navillm_hip_optim.h):
//   nv_adamw_master   fp32 master weights + fp32 moments, p = RNE_bf16(master), self-healing master
//   nv_adamw_sr       bf16 parameter and moments, the three stores stochastically rounded (Philox4x32-10 keyed by seed, step,
//                     global element index and array)
// Both compute one element in fp32 registers with no intermediate rounding; nv_adamw (head_loss_optim.hip) stays the reference-exact
// default.  Streaming layout of both: 8 elements per thread and iteration (one 16-byte access per bf16 array, two per fp32 array),
// grid-stride; a scalar loop takes the tail of n % 8 and everything when a base pointer is not 16-byte aligned.
#include "nv_common.h"
#include <math.h>

namespace {

struct hp_scalars {                     // prepared on the host in double, rounded to fp32 once (adamw_launch's rule)
    float decay, w1, b2, w2, eps, step_size, sqrt_bc2;
};

__device__ __forceinline__ void ld8(const bf16_t* p, float* f) {
    const u32x4 v = *(const u32x4*)p;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        f[2 * i] = __uint_as_float(v[i] << 16);
        f[2 * i + 1] = __uint_as_float(v[i] & 0xffff0000u);
    }
}
__device__ __forceinline__ void ld8f(const float* p, float* f) {
    const f32x4 a = *(const f32x4*)p, b = *(const f32x4*)(p + 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) { f[i] = a[i]; f[4 + i] = b[i]; }
}
__device__ __forceinline__ void st8f(float* p, const float* f) {
    *(f32x4*)p = f32x4{f[0], f[1], f[2], f[3]};
    *(f32x4*)(p + 4) = f32x4{f[4], f[5], f[6], f[7]};
}

// one element, fp32 throughout (the header states the formula; hipcc may contract a*b+c into an fma, which only removes roundings)
__device__ __forceinline__ void adamw_hp_elem(float& p, float g_raw, float& m, float& v, float coef, const hp_scalars& h) {
    const float g = g_raw * coef;
    p = p * h.decay;
    m = m + h.w1 * (g - m);
    v = h.b2 * v + h.w2 * g * g;
    p = p - h.step_size * m / (sqrtf(v) / h.sqrt_bc2 + h.eps);
}

// the master of an element: the stored one while it still rounds to the parameter's bits, else the parameter itself
__device__ __forceinline__ float heal(float master, float p_as_float) {
    return (__float_as_uint(rbf(master)) == __float_as_uint(p_as_float)) ? master : p_as_float;
}

template <bool ZG>
__global__ __launch_bounds__(256) void adamw_master_kernel(bf16_t* __restrict__ p, bf16_t* __restrict__ g, float* __restrict__ master,
                                                           float* __restrict__ m, float* __restrict__ v, long n, hp_scalars h,
                                                           const float* __restrict__ clip) {
    const float coef = clip ? clip[1] : 1.f;
    long done = 0;
    if (((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)master) | ((uintptr_t)m) | ((uintptr_t)v)) & 15) == 0) {
        const long n8 = n / 8;
        for (long i = blockIdx.x * 256L + threadIdx.x; i < n8; i += gridDim.x * 256L) {
            float pf[8], gf[8], wf[8], mf[8], vf[8];
            ld8(p + i * 8, pf);
            ld8(g + i * 8, gf);
            ld8f(master + i * 8, wf);
            ld8f(m + i * 8, mf);
            ld8f(v + i * 8, vf);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                wf[j] = heal(wf[j], pf[j]);
                adamw_hp_elem(wf[j], gf[j], mf[j], vf[j], coef, h);
            }
            st8f(master + i * 8, wf);
            st8f(m + i * 8, mf);
            st8f(v + i * 8, vf);
            *(u32x4*)(p + i * 8) = u32x4{pack2bf(wf[0], wf[1]), pack2bf(wf[2], wf[3]), pack2bf(wf[4], wf[5]), pack2bf(wf[6], wf[7])};
            if (ZG) *(u32x4*)(g + i * 8) = u32x4{0u, 0u, 0u, 0u};
        }
        done = n8 * 8;
    }
    for (long i = done + blockIdx.x * 256L + threadIdx.x; i < n; i += gridDim.x * 256L) {
        float w = heal(master[i], bf2f(p[i])), mi = m[i], vi = v[i];
        adamw_hp_elem(w, bf2f(g[i]), mi, vi, coef, h);
        master[i] = w;
        m[i] = mi;
        v[i] = vi;
        p[i] = f2bf(w);
        if (ZG) g[i] = 0;
    }
}

// ---- stochastic rounding (the header documents the counter layout)
__device__ __forceinline__ void sr_block(unsigned long long group, uint32_t step, uint32_t array, unsigned long long seed, uint32_t* out) {
    philox4x32_10((uint32_t)group, (uint32_t)(group >> 32), step, array, (uint32_t)seed, (uint32_t)(seed >> 32), out);
}
__device__ __forceinline__ uint32_t sr_round(float x, uint32_t r16) {
    const uint32_t u = __float_as_uint(x), mag = u & 0x7fffffffu;
    if (mag >= 0x7f800000u) return (u >> 16) | (mag > 0x7f800000u ? 0x40u : 0u);      // Inf / NaN: not rounded, a NaN stays one
    return (u + r16) >> 16;
}
__device__ __forceinline__ u32x4 sr_pack8(const float* f, const uint32_t* r) {
    u32x4 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = sr_round(f[2 * i], r[i] & 0xffffu) | (sr_round(f[2 * i + 1], r[i] >> 16) << 16);
    return o;
}

template <bool ZG>
__global__ __launch_bounds__(256) void adamw_sr_kernel(bf16_t* __restrict__ p, bf16_t* __restrict__ g, bf16_t* __restrict__ m,
                                                       bf16_t* __restrict__ v, long n, unsigned long long elem0, unsigned long long seed,
                                                       uint32_t step, hp_scalars h, const float* __restrict__ clip) {
    const float coef = clip ? clip[1] : 1.f;
    long done = 0;
    // a thread's 8 elements are one Philox group only when the piece starts at a multiple of 8 global elements
    if ((((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v)) & 15) | (elem0 & 7)) == 0) {
        const long n8 = n / 8;
        const unsigned long long group0 = elem0 >> 3;
        for (long i = blockIdx.x * 256L + threadIdx.x; i < n8; i += gridDim.x * 256L) {
            float pf[8], gf[8], mf[8], vf[8];
            ld8(p + i * 8, pf);
            ld8(g + i * 8, gf);
            ld8(m + i * 8, mf);
            ld8(v + i * 8, vf);
#pragma unroll
            for (int j = 0; j < 8; ++j) adamw_hp_elem(pf[j], gf[j], mf[j], vf[j], coef, h);
            uint32_t r[4];
            sr_block(group0 + (unsigned long long)i, step, 0u, seed, r);
            *(u32x4*)(p + i * 8) = sr_pack8(pf, r);
            sr_block(group0 + (unsigned long long)i, step, 1u, seed, r);
            *(u32x4*)(m + i * 8) = sr_pack8(mf, r);
            sr_block(group0 + (unsigned long long)i, step, 2u, seed, r);
            *(u32x4*)(v + i * 8) = sr_pack8(vf, r);
            if (ZG) *(u32x4*)(g + i * 8) = u32x4{0u, 0u, 0u, 0u};
        }
        done = n8 * 8;
    }
    for (long i = done + blockIdx.x * 256L + threadIdx.x; i < n; i += gridDim.x * 256L) {
        float pi = bf2f(p[i]), mi = bf2f(m[i]), vi = bf2f(v[i]);
        adamw_hp_elem(pi, bf2f(g[i]), mi, vi, coef, h);
        const unsigned long long e = elem0 + (unsigned long long)i;
        const int word = (int)(e & 7) >> 1, shift = 16 * (int)(e & 1);
        uint32_t r[4];
        sr_block(e >> 3, step, 0u, seed, r);
        p[i] = (bf16_t)sr_round(pi, (r[word] >> shift) & 0xffffu);
        sr_block(e >> 3, step, 1u, seed, r);
        m[i] = (bf16_t)sr_round(mi, (r[word] >> shift) & 0xffffu);
        sr_block(e >> 3, step, 2u, seed, r);
        v[i] = (bf16_t)sr_round(vi, (r[word] >> shift) & 0xffffu);
        if (ZG) g[i] = 0;
    }
}

inline int hp_grid(long n) {            // one thread per 8 elements, at most 4096 blocks (adamw_launch's cap)
    long b = ((n + 7) / 8 + 255) / 256;
    return (int)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

inline hp_scalars hp_prepare(double lr, double beta1, double beta2, double eps, double wd, int step) {
    hp_scalars h;
    h.decay = (float)(1.0 - lr * wd);
    h.w1 = (float)(1.0 - beta1);
    h.b2 = (float)beta2;
    h.w2 = (float)(1.0 - beta2);
    h.eps = (float)eps;
    h.step_size = (float)(lr / (1.0 - pow(beta1, (double)step)));
    h.sqrt_bc2 = (float)sqrt(1.0 - pow(beta2, (double)step));
    return h;
}

}  // namespace

extern "C" {

int nv_adamw_master(void* p, void* g, float* master, float* m, float* v, long n, double lr, double beta1, double beta2, double eps,
                    double wd, int step, const float* clip, int zero_grad, void* stream) {
    if (!p || !g || !master || !m || !v || step < 1 || n < 0) return NV_ERR_ARG;
    if (n == 0) return NV_OK;
    const hp_scalars h = hp_prepare(lr, beta1, beta2, eps, wd, step);
    if (zero_grad)
        NV_LAUNCH(adamw_master_kernel<true>, dim3(hp_grid(n)), dim3(256), 0, (hipStream_t)stream, (bf16_t*)p, (bf16_t*)g, master, m, v, n, h,
                  clip);
    else
        NV_LAUNCH(adamw_master_kernel<false>, dim3(hp_grid(n)), dim3(256), 0, (hipStream_t)stream, (bf16_t*)p, (bf16_t*)g, master, m, v, n, h,
                  clip);
    return nv_check_launch();
}

int nv_adamw_sr(void* p, void* g, void* m, void* v, long n, long elem0, unsigned long long seed, double lr, double beta1, double beta2,
                double eps, double wd, int step, const float* clip, int zero_grad, void* stream) {
    if (!p || !g || !m || !v || step < 1 || n < 0 || elem0 < 0) return NV_ERR_ARG;
    if (n == 0) return NV_OK;
    const hp_scalars h = hp_prepare(lr, beta1, beta2, eps, wd, step);
    if (zero_grad)
        NV_LAUNCH(adamw_sr_kernel<true>, dim3(hp_grid(n)), dim3(256), 0, (hipStream_t)stream, (bf16_t*)p, (bf16_t*)g, (bf16_t*)m, (bf16_t*)v,
                  n, (unsigned long long)elem0, seed, (uint32_t)step, h, clip);
    else
        NV_LAUNCH(adamw_sr_kernel<false>, dim3(hp_grid(n)), dim3(256), 0, (hipStream_t)stream, (bf16_t*)p, (bf16_t*)g, (bf16_t*)m, (bf16_t*)v,
                  n, (unsigned long long)elem0, seed, (uint32_t)step, h, clip);
    return nv_check_launch();
}

}  // extern "C"
