// bprx_calibrate.hip -- greedy KL re-rank of top-K candidate pools toward each user's own class mix (include/bprx.h, bprx_calibrate).
#include "bprx_internal.h"

namespace {

constexpr int CB_T = 256;                    // threads of a workgroup = of a list
constexpr int CB_SLOTS = 4;                  // pool positions per thread: position c belongs to thread c & 255, slot c >> 8
constexpr int CB_NMAX = CB_T * CB_SLOTS;     // 1024, the pool bprx_topk can fill
constexpr int CB_CMAX = 1024;                // classes (BPRX_STYLES_MAX): class + 1 fits the 11 low bits of a key
constexpr int CB_CBITS = 11;
static_assert(CB_CMAX + 1 <= (1 << CB_CBITS) && ((int64_t)CB_NMAX << CB_CBITS) < ((int64_t)1 << 32), "a key's low word");

struct CalArgs {
  int N, K, C, width;
  float lambda, alpha;
  int64_t row0;
  const int32_t *pool_idx;
  const float *pool_val;
  const int64_t *hist_ptr;
  const int32_t *hist_items, *item_class;
  int32_t *idx, *cls;
  float *val, *gain, *kl;
  int32_t *errflag;
};

// den_g(m) = (1 - alpha) m / L + alpha p_g with ap = alpha p_g: one rounded product, quotient and sum
__device__ __forceinline__ float cb_den(float oma, float m, float L, float ap) {
  return __fadd_rn(__fdiv_rn(__fmul_rn(oma, m), L), ap);
}

// One workgroup per list.  Thread t holds pool positions t, t + 256, t + 512, t + 768: their relevance term, class, that class's
// share p of the history and the number n of picks of that class so far stay in registers for the whole list, so a step forms
// delta = p log(den(n) / den(n + 1)) per candidate from registers alone.  A step = that, one argmax over (objective descending,
// position ascending) -- a 64-bit key per thread, wave shuffles, four keys through LDS -- and ONE barrier (the key slots
// alternate between steps): the key's low word carries the pick's class below its position, so every thread learns both from
// the winning key and bumps the n of its own candidates of that class.  (delta is the same number for every candidate of a
// class: forming it once per class in LDS would need a second barrier per step; up to 256 candidates a thread forms one either way.)
// LDS holds the per-class counts only: the history's (cnt), and for the two KL values the plain and the calibrated list's.
__global__ __launch_bounds__(CB_T) void k_calibrate(CalArgs a) {
  extern __shared__ int cb_dyn[];            // cnt [C] | n of the plain list [C] | n of the calibrated list [C]
  __shared__ unsigned long long s_best[2][CB_T / 64];
  __shared__ float s_vmax[CB_T / 64], s_vmin[CB_T / 64];
  __shared__ int s_live[CB_SLOTS][CB_T / 64];
  __shared__ float s_kl[2][CB_T / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = a.N, K = a.K, C = a.C;
  int *s_cnt = cb_dyn, *s_np = cb_dyn + C, *s_nc = cb_dyn + 2 * C;
  const size_t r = blockIdx.x;
  const int32_t *pid = a.pool_idx + r * (size_t)N;
  const float *pv = a.pool_val + r * (size_t)N;

  for (int g = tid; g < 3 * C; g += CB_T) cb_dyn[g] = 0;

  // ---- the pool: candidates, their classes; M, v_max, v_min, every candidate's rank among the candidates ----
  float v[CB_SLOTS];
  int cls[CB_SLOTS], rank[CB_SLOTS];
  bool live[CB_SLOTS];
  float vmax = -INFINITY, vmin = INFINITY;
#pragma unroll
  for (int j = 0; j < CB_SLOTS; ++j) {
    const int c = tid + j * CB_T;
    v[j] = 0.f; cls[j] = -1; live[j] = false;
    if (c < N) {
      const int raw = pid[c];
      v[j] = pv[c];
      live[j] = raw >= 0 && v[j] != -INFINITY;
      if (live[j]) {
        vmax = fmaxf(vmax, v[j]); vmin = fminf(vmin, v[j]);
        if (raw >= a.width) *a.errflag = 2;                  // reported by bprx_sync_check, never used as an index: classless
        else {
          const int g = a.item_class[raw];
          if (g >= 0 && g < C) cls[j] = g;
          else if (g != -1) *a.errflag = 5;
        }
      }
    }
    const unsigned long long b = __ballot(live[j]);
    rank[j] = __popcll(b & ((1ull << lane) - 1ull));
    if (lane == 0) s_live[j][wave] = __popcll(b);
  }
  vmax = wave_max(vmax);
  vmin = -wave_max(-vmin);
  if (lane == 0) { s_vmax[wave] = vmax; s_vmin[wave] = vmin; }
  __syncthreads();                           // (also: the class counts are zero)

  // ---- the history's class histogram: exact, LDS integer atomics ----
  if (a.hist_ptr) {
    const int64_t t0 = a.hist_ptr[a.row0 + (int64_t)r], t1 = a.hist_ptr[a.row0 + (int64_t)r + 1];
    for (int64_t q = t0 + tid; q < t1; q += CB_T) {
      const int it = a.hist_items[q];
      if ((unsigned)it < (unsigned)a.width) {
        const int g = a.item_class[it];
        if (g >= 0 && g < C) atomicAdd(&s_cnt[g], 1);
        else if (g != -1) *a.errflag = 5;
      }
    }
  }
  int M = 0;                                 // rank: the candidates at the positions in front (lower slots, then lower waves)
#pragma unroll
  for (int j = 0; j < CB_SLOTS; ++j) {
    int before = M;
#pragma unroll
    for (int q = 0; q < CB_T / 64; ++q) { const int m = s_live[j][q]; before += q < wave ? m : 0; M += m; }
    rank[j] += before;
  }
#pragma unroll
  for (int q = 0; q < CB_T / 64; ++q) { vmax = fmaxf(vmax, s_vmax[q]); vmin = fminf(vmin, s_vmin[q]); }
  __syncthreads();                           // the histogram is complete

  // H = sum of cnt, an integer sum: every thread adds its classes, the waves theirs
  int hloc = 0;
  for (int g = tid; g < C; g += CB_T) hloc += s_cnt[g];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) hloc += __shfl_xor(hloc, o, 64);
  __shared__ int s_h[CB_T / 64];
  if (lane == 0) s_h[wave] = hloc;
  __syncthreads();
  int H = 0;
#pragma unroll
  for (int q = 0; q < CB_T / 64; ++q) H += s_h[q];
  const float Hf = (float)H;

  // rel_c = (v_c - v_min) / (v_max - v_min), 0 for a flat list; rel1_c = (1 - lambda) rel_c, each operation rounded once
  const float lambda = a.lambda, alpha = a.alpha, oml = __fsub_rn(1.f, lambda), oma = __fsub_rn(1.f, alpha);
  const float span = M > 0 ? __fsub_rn(vmax, vmin) : 0.f;
  float rel1[CB_SLOTS], p[CB_SLOTS], ap[CB_SLOTS];
  int n[CB_SLOTS];
#pragma unroll
  for (int j = 0; j < CB_SLOTS; ++j) {
    const float rel = live[j] && span > 0.f ? __fdiv_rn(__fsub_rn(v[j], vmin), span) : 0.f;
    rel1[j] = __fmul_rn(oml, rel);
    const int cn = cls[j] >= 0 ? s_cnt[cls[j]] : 0;
    p[j] = cn > 0 ? __fdiv_rn((float)cn, Hf) : 0.f;
    ap[j] = __fmul_rn(alpha, p[j]);
    n[j] = 0;
  }

  const int T = K < M ? K : M;
  const int nslots = (N + CB_T - 1) / CB_T;  // slots the pool reaches: the same in every thread
  int32_t *o_idx = a.idx + r * (size_t)K, *o_cls = a.cls + r * (size_t)K;
  float *o_val = a.val + r * (size_t)K, *o_gain = a.gain + r * (size_t)K;
  bool picked[CB_SLOTS], plain[CB_SLOTS];    // on the calibrated list; among the pool's first T candidates, the plain list
#pragma unroll
  for (int j = 0; j < CB_SLOTS; ++j) { picked[j] = false; plain[j] = live[j] && rank[j] < T; }
  for (int t = 0; t < T; ++t) {
    // obj_c = (1 - lambda) rel_c - lambda delta_c: nothing fused
    const float L = (float)(t + 1);
    float delta[CB_SLOTS];
    unsigned long long best = 0ull;
#pragma unroll
    for (int j = 0; j < CB_SLOTS; ++j) {
      delta[j] = 0.f;
      if (j < nslots && live[j]) {
        if (p[j] > 0.f)
          delta[j] = __fmul_rn(p[j], logf(__fdiv_rn(cb_den(oma, (float)n[j], L, ap[j]), cb_den(oma, (float)(n[j] + 1), L, ap[j]))));
        const float obj = __fsub_rn(rel1[j], __fmul_rn(lambda, delta[j]));
        const uint32_t low = ((uint32_t)(CB_NMAX - (tid + j * CB_T)) << CB_CBITS) | (uint32_t)(cls[j] + 1);   // never 0
        const unsigned long long key = ((unsigned long long)dv_key(obj) << 32) | low;
        best = key > best ? key : best;
      }
    }
    best = dv_wave_max(best);
    if (lane == 0) s_best[t & 1][wave] = best;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < CB_T / 64; ++q) { const unsigned long long o = s_best[t & 1][q]; best = o > best ? o : best; }
    const uint32_t low = (uint32_t)(best & 0xffffffffull);
    const int s = CB_NMAX - (int)(low >> CB_CBITS);            // the pick's pool position and class: known to every thread
    const int g = (int)(low & ((1u << CB_CBITS) - 1u)) - 1;
#pragma unroll
    for (int j = 0; j < CB_SLOTS; ++j) {
      if (tid + j * CB_T == s) {
        o_idx[t] = pid[s]; o_val[t] = v[j]; o_cls[t] = g; o_gain[t] = __fsub_rn(0.f, delta[j]);   // (+0 for a delta of 0)
        live[j] = false; picked[j] = true;
      }
      if (g >= 0 && cls[j] == g) ++n[j];
    }
  }
  for (int q = T + tid; q < K; q += CB_T) { o_idx[q] = -1; o_val[q] = 0.f; o_cls[q] = -1; o_gain[q] = 0.f; }
  if (!a.kl) return;

  // ---- KL(p || q~) of the pool's first T candidates and of the picks, L = T: class counts by LDS integer atomics, the sum over
  // the classes in an order C alone fixes (a thread's classes ascending, the wave's butterfly, the waves ascending) ----
#pragma unroll
  for (int j = 0; j < CB_SLOTS; ++j)
    if (cls[j] >= 0) {
      if (plain[j]) atomicAdd(&s_np[cls[j]], 1);
      if (picked[j]) atomicAdd(&s_nc[cls[j]], 1);
    }
  __syncthreads();
  float kp = 0.f, kc = 0.f;
  if (H > 0 && T > 0) {
    const float Tf = (float)T;
    for (int c = tid; c < C; c += CB_T) {
      const int cn = s_cnt[c];
      if (cn > 0) {
        const float pc = __fdiv_rn((float)cn, Hf), apc = __fmul_rn(alpha, pc);
        kp = __fadd_rn(kp, __fmul_rn(pc, logf(__fdiv_rn(pc, cb_den(oma, (float)s_np[c], Tf, apc)))));
        kc = __fadd_rn(kc, __fmul_rn(pc, logf(__fdiv_rn(pc, cb_den(oma, (float)s_nc[c], Tf, apc)))));
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    kp = __fadd_rn(kp, __shfl_xor(kp, o, 64));
    kc = __fadd_rn(kc, __shfl_xor(kc, o, 64));
  }
  if (lane == 0) { s_kl[0][wave] = kp; s_kl[1][wave] = kc; }
  __syncthreads();
  if (tid < 2) {
    float sum = s_kl[tid][0];
#pragma unroll
    for (int q = 1; q < CB_T / 64; ++q) sum = __fadd_rn(sum, s_kl[tid][q]);
    a.kl[r * 2 + tid] = sum;
  }
}

}  // namespace

extern "C" int bprx_calibrate(bprx_handle *h, int64_t n, int32_t N, const int32_t *pool_idx, const float *pool_val, int64_t row0,
                              const int64_t *hist_ptr, const int32_t *hist_items, const int32_t *item_class, int32_t width, int32_t C,
                              int32_t K, float lambda, float alpha, int32_t *idx, float *val, int32_t *cls, float *gain, float *kl,
                              void *stream) {
  if (!h) return BPRX_E_INVALID;
  if (n < 0 || n >= ((int64_t)1 << 31)) BPRX_FAIL(h, BPRX_E_INVALID, "calibrate: n = %lld out of range", (long long)n);
  if (row0 < 0) BPRX_FAIL(h, BPRX_E_INVALID, "calibrate: row0 = %lld is negative", (long long)row0);
  if (K < 1 || K > N || N > CB_NMAX) BPRX_FAIL(h, BPRX_E_INVALID, "calibrate: need 1 <= K <= N <= %d, got K = %d, N = %d", CB_NMAX, K, N);
  if (C < 1 || C > CB_CMAX) BPRX_FAIL(h, BPRX_E_INVALID, "calibrate: C = %d outside [1, %d]", C, CB_CMAX);
  if (width < 1) BPRX_FAIL(h, BPRX_E_INVALID, "calibrate: width = %d < 1", width);
  if (!(lambda >= 0.f && lambda <= 1.f)) BPRX_FAIL(h, BPRX_E_INVALID, "calibrate: lambda = %g outside [0, 1]", (double)lambda);
  if (!(alpha > 0.f && alpha < 1.f)) BPRX_FAIL(h, BPRX_E_INVALID, "calibrate: alpha = %g outside (0, 1)", (double)alpha);
  if (n > 0 && (!pool_idx || !pool_val || !item_class || !idx || !val || !cls || !gain || (hist_ptr && !hist_items)))
    BPRX_FAIL(h, BPRX_E_INVALID, "calibrate: null pointer");
  if (n == 0) return BPRX_OK;
  CalArgs a = {};
  a.N = N; a.K = K; a.C = C; a.width = width; a.lambda = lambda; a.alpha = alpha; a.row0 = row0;
  a.pool_idx = pool_idx; a.pool_val = pool_val; a.hist_ptr = hist_ptr; a.hist_items = hist_items; a.item_class = item_class;
  a.idx = idx; a.val = val; a.cls = cls; a.gain = gain; a.kl = kl; a.errflag = h->errflag;
  hipLaunchKernelGGL(k_calibrate, dim3((unsigned)n), dim3(CB_T), (size_t)3 * C * sizeof(int), (hipStream_t)stream, a);
  BPRX_LAUNCH_CHECK(h, "k_calibrate");
  return BPRX_OK;
}
