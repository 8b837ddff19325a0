// bprx_device.h -- device functions every kernel file of libbprx.so may use (included by bprx_internal.h): the wave and
// workgroup reductions, the index clamps, the item side of a user's pairs (fold_row), bf16 rounding, Philox, and the ONE definition of each optimizer rule.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// ---- wave (64 lanes) -------------------------------------------------------------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
// Ordered selection by float value (bprx_diversify, bprx_because): larger float <-> larger key; -0.0 and +0.0 share one key
// ("values compare as floats")
__device__ __forceinline__ uint32_t dv_key(float x) {
  uint32_t u = __float_as_uint(x);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ unsigned long long dv_wave_max(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long w = __shfl_xor(v, o, 64);
    v = w > v ? w : v;
  }
  return v;
}
// LDS written by some lanes of a wave and read by others of the same wave
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Sum of one double per thread of a 1024-thread workgroup, in a fixed order (a halving tree in LDS: no atomics,
// reproducible).  Every thread gets the total; call it once per kernel, from uniform control flow.
__device__ __forceinline__ double block_sum_1024(double s) {
  __shared__ double red[1024];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  return red[0];
}

// ---- indices ---------------------------------------------------------------------------------------------------------
// v clamped into [0, n); an index outside raises the handle's deferred error flag
__device__ __forceinline__ int clamp_index(int v, int n, int32_t *errflag, int code) {
  if ((unsigned)v >= (unsigned)n) {
    *errflag = code;
    return v < 0 ? 0 : n - 1;
  }
  return v;
}
// the same value without the flag: for kernels that run after one that has already raised it
__device__ __forceinline__ int clamp_quiet(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

// ---- the item side of a fitted user row (bprx_fold_in, bprx_influence) -------------------------------------------------------
// elements lane, lane + 64, ... of z_it = [Gi_it | P_it[0:d]] (zero past k + d) and c_it = Bi_it + P_it[d] (BPRMF: Bi_it).  a: any
// argument struct with Gi [I, k], Bi [I], P [I, PS] (unread when d == 0), k, d, PS.
template <int EPL, class Args>
__device__ __forceinline__ void fold_row(const Args &a, int it, int lane, float (&z)[EPL], float &c) {
  const float *g = a.Gi + (size_t)it * a.k;
  const size_t pb = (size_t)it * a.PS;
#pragma unroll
  for (int e = 0; e < EPL; ++e) {
    const int col = lane + 64 * e;
    z[e] = col < a.k ? g[col] : (col < a.k + a.d ? a.P[pb + (col - a.k)] : 0.f);
  }
  c = a.d ? a.Bi[it] + a.P[pb + a.d] : a.Bi[it];
}

// bf16 code of x, round-to-nearest-even; x is finite
__device__ __forceinline__ uint32_t bf16_rne(float x) {
  const uint32_t b = __float_as_uint(x);
  return (b + 0x7fffu + ((b >> 16) & 1u)) >> 16;
}

// Philox4x32-10 (Salmon et al. 2011): the generator of the device samplers (bprx_philox.hip) and of the dropout stream
// (bprx_attentive.hip)
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t (&out)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    const uint32_t n0 = h1 ^ c1 ^ k0, n2 = h0 ^ c3 ^ k1;
    c0 = n0; c1 = l1; c2 = n2; c3 = l0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// ---- optimizer rules ---------------------------------------------------------------------------------------------------
// adam_tf23, sparse-variable rule (TF-2.3 Keras Adam is NOT lazy: every row of the table decays and moves every step):
//   m = m*b1 + g*(1-b1); v = v*b2 + g*g*(1-b2); var -= lr_t*m/(sqrt(v)+eps)     (g == 0 on untouched rows)
// One element, one step.  The whole-table sweep of every model (k_adam_sweep, bprx_sparse.hip) and the lazy catch-up replay
// share this function, so that a replayed step performs bit for bit the arithmetic the sweep would have performed.
__device__ __forceinline__ void adam_elem(float &p, float &m, float &v, float g, float b1, float b2, float lr_t, float eps) {
#pragma clang fp contract(off)   // no fused multiply-adds: the same roundings wherever this is inlined (scalar sweep, float4 replay)
  const float omb1 = 1.0f - b1, omb2 = 1.0f - b2;
  const float mt = m * b1 + g * omb1;
  const float vt = v * b2 + (g * g) * omb2;
  m = mt; v = vt;
  p = p - lr_t * mt / (sqrtf(vt) + eps);
}

// The DENSE variables (E / Bp, GradFashion's factors, the attention tensors of ACF and AttentiveFashion): sgd, or TF-2.3's
// dense ApplyAdam
//   m += (g-m)(1-b1); v += (g*g-v)(1-b2); var -= lr_t*m/(sqrt(v)+eps)                      (VBPR.py:142)
// for one element: returns the new value of p and moves the slots *m and *v (sgd does not look at them).  Contraction is
// left to the compiler's default here, as it always was in the kernels that share this.
__device__ __forceinline__ float dense_adam_elem(float p, float *m, float *v, float g, int adam, float lr_t, float b1, float b2,
                                                 float eps) {
  if (!adam) return p - lr_t * g;
  const float mo = *m, vo = *v;
  const float mt = mo + (g - mo) * (1.0f - b1);
  const float vt = vo + (g * g - vo) * (1.0f - b2);
  *m = mt; *v = vt;
  return p - lr_t * mt / (sqrtf(vt) + eps);
}
