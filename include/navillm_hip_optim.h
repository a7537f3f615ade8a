/*
 * navillm_hip_optim.h -- AdamW for the bf16 LM group with more state precision than bf16: the entry points of libnavillm_hip.so that
 * came after the 119 of navillm_hip.h (whose number the suite pins) and the two of navillm_hip_topp.h.  Same conventions, same library;
 * navillm_amd/lib.py binds them from OPTIM_SIGNATURES and raises when one is missing.  Kernels: navillm_amd/csrc/adamw_hp.hip.
 *
 * Both entries compute one element's update in fp32 registers with no intermediate rounding (nv_adamw rounds to the storage type after
 * every intermediate, as torch.optim.AdamW does on bf16 tensors):
 *
 *     g = float(g_bf16) * clip_coef              clip_coef = clip ? clip[1] : 1   (the vector nv_clip_coef writes)
 *     p = p * (1 - lr*wd)
 *     m = m + (1-beta1) * (g - m)
 *     v = beta2*v + (1-beta2) * g*g
 *     p = p - step_size * m / (sqrt(v)/sqrt_bc2 + eps)
 *
 * with 1 - lr*wd, 1-beta1, 1-beta2, step_size = lr / (1 - beta1^step) and sqrt_bc2 = sqrt(1 - beta2^step) prepared in double and
 * rounded to fp32 once, exactly as nv_adamw prepares them.  zero_grad != 0 zeroes g as it is consumed (nv_adamw_zero_grad's rule).
 * NV_ERR_ARG before any launch: a null pointer (clip may be null), step < 1, n < 0, elem0 < 0.  n == 0: NV_OK, nothing launched.
 * Pointers need no alignment (16-byte aligned ones take the 8-elements-per-thread path); the arrays must not overlap.
 */
#ifndef NAVILLM_HIP_OPTIM_H
#define NAVILLM_HIP_OPTIM_H
#include "navillm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- fp32 master weights.  p, g: bf16 [n]; master, m, v: fp32 [n].  Stores master, m, v in fp32 and p = RNE_bf16(master).
 *      Self-healing master: the kernel reads p, and where RNE_bf16(master[i]) != p[i] BITWISE it takes float(p[i]) as that element's
 *      master before the update -- whoever wrote the parameter last (an initialiser, a checkpoint load, copy_, a broadcast) is
 *      authoritative without a host hook, and a zero-initialised master adopts the weights at the first step (a weight of +0 agrees
 *      with it already).  Elements nobody wrote keep the master's bits below bf16. */
int nv_adamw_master(void* p, void* g, float* master, float* m, float* v, long n, double lr, double beta1, double beta2, double eps,
                    double wd, int step, const float* clip, int zero_grad, void* stream);

/* ---- stochastic rounding.  p, g, m, v: bf16 [n].  The same arithmetic from the bf16 inputs; the three stores p, m, v are rounded
 *      stochastically: a finite fp32 result with bit pattern u and 16 random bits r is stored as the bf16 pattern (u + r) >> 16, so the
 *      magnitude rounds away from zero with probability (u & 0xffff) / 65536 -- exactly unbiased -- and a representable value
 *      (u & 0xffff == 0) is stored unchanged.  Inf and NaN are not rounded (u >> 16; a NaN keeps a mantissa bit).
 *
 *      Random bits: Philox4x32-10 (the generator of the dropout kernels), a pure function of (seed, step, global element index, array).
 *      Element i of this call has the global index e = elem0 + i.  One Philox block serves the 8 elements of one array that share e >> 3:
 *          counter  c0 = low word of (e >> 3),  c1 = high word of (e >> 3),  c2 = step,  c3 = array (0: p, 1: m, 2: v)
 *          key      k0 = low word of seed,  k1 = high word of seed
 *          r        = (out[(e & 7) >> 1] >> (16 * (e & 1))) & 0xffff      out[0..3]: the block's four 32-bit words
 *      Nothing else enters: not the thread, the block, the grid or n.  Cutting a buffer into several calls (elem0 = the offset of each
 *      piece, any value >= 0) stores the same bits as one call; pieces that start at a multiple of 8 elements AND at a 16-byte aligned
 *      address take the vector path. */
int nv_adamw_sr(void* p, void* g, void* m, void* v, long n, long elem0, unsigned long long seed, double lr, double beta1, double beta2,
                double eps, double wd, int step, const float* clip, int zero_grad, void* stream);

#ifdef __cplusplus
}
#endif
#endif
