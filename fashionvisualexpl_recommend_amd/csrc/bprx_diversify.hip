// bprx_diversify.hip -- greedy MMR re-rank of top-K candidate pools in the model's item space (include/bprx.h, bprx_diversify).
#include <stdlib.h>

#include "bprx_internal.h"

namespace {

constexpr int DV_T = 256;                    // threads of a workgroup = of a list
constexpr int DV_SLOTS = 4;                  // pool positions per thread: position c belongs to thread c & 255, slot c >> 8
constexpr int DV_NMAX = DV_T * DV_SLOTS;     // 1024, the pool bprx_topk can fill
constexpr int DV_DYN_MAX = 63 * 1024;        // dynamic LDS of a list: with the static arrays below it stays within the 64 KiB a
                                             //    launch gets without opting in, so two lists share a CU's 160 KiB

struct DivArgs {
  SimPart g, p;                              // z = [g | p]
  const float *rn;                           // [I] bprx_sim_rnorm of the catalogue in the same space
  int I, N, K, ld;                           // ld: row stride of the LDS rows (odd), 0 in the global-row form
  float theta;
  const int32_t *pool_idx;
  const float *pool_val;
  int32_t *idx;
  float *val, *pen, *ild;
  int32_t *errflag;
};

// One workgroup per list.  Thread t holds pool positions t, t + 256, t + 512, t + 768: their relevance term, running penalty and
// running cosine sum stay in registers for the whole list.  A round = one argmax over (objective descending, position ascending)
// -- a 64-bit key per thread, wave shuffles, four keys through LDS, ONE barrier (the key slots alternate between rounds) -- and
// the dot products of the new pick's row with every live candidate's row, one candidate row per thread slot.
// ROWS_LDS: the candidates' z rows were copied to LDS once (row stride ld, odd: the 32 lanes of a ds_read_b32 group read 32
// different banks; the pick's row is one address for all lanes, a broadcast).  Otherwise every round reads them from global
// memory (L2-resident).  Both forms run the same chain acc = fmaf(z_c[x], z_s[x], acc) from +0 in ascending x, g before p:
// the same bits.
template <bool ROWS_LDS>
__global__ __launch_bounds__(DV_T) void k_diversify(DivArgs a) {
  extern __shared__ float dv_dyn[];          // ids [N] | rn [N] | rows [N][ld] (ROWS_LDS)
  __shared__ unsigned long long s_best[2][DV_T / 64];
  __shared__ float s_vmax[DV_T / 64], s_vmin[DV_T / 64];
  __shared__ int s_cnt[DV_T / 64];
  __shared__ float s_acc[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = a.N, K = a.K, w = a.g.w + a.p.w;
  int *s_id = (int *)dv_dyn;
  float *s_rn = dv_dyn + N, *s_row = dv_dyn + 2 * N;
  const size_t r = blockIdx.x;
  const int32_t *pid = a.pool_idx + r * (size_t)N;
  const float *pv = a.pool_val + r * (size_t)N;

  // ---- the pool: candidates, their ids (clamped) and norms; M, v_max, v_min ----
  int id[DV_SLOTS];
  float v[DV_SLOTS], rn[DV_SLOTS];
  bool live[DV_SLOTS];
  float vmax = -INFINITY, vmin = INFINITY;
  int cnt = 0;
#pragma unroll
  for (int j = 0; j < DV_SLOTS; ++j) {
    const int c = tid + j * DV_T;
    id[j] = 0; v[j] = 0.f; rn[j] = 0.f; live[j] = false;
    if (c < N) {
      const int raw = pid[c];
      v[j] = pv[c];
      live[j] = raw >= 0 && v[j] != -INFINITY;
      id[j] = raw < 0 ? 0 : clamp_index(raw, a.I, a.errflag, 2);
      rn[j] = a.rn[id[j]];
      s_id[c] = id[j];
      s_rn[c] = rn[j];
      if (live[j]) { vmax = fmaxf(vmax, v[j]); vmin = fminf(vmin, v[j]); ++cnt; }
    }
  }
  vmax = wave_max(vmax);
  vmin = -wave_max(-vmin);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  if (lane == 0) { s_vmax[wave] = vmax; s_vmin[wave] = vmin; s_cnt[wave] = cnt; }
  __syncthreads();                           // (also: s_id / s_rn are complete)
  int M = 0;
#pragma unroll
  for (int q = 0; q < DV_T / 64; ++q) { vmax = fmaxf(vmax, s_vmax[q]); vmin = fminf(vmin, s_vmin[q]); M += s_cnt[q]; }

  if (ROWS_LDS) {                            // consecutive threads copy consecutive x of a row: coalesced reads, stride-1 LDS writes
    const int ld = a.ld;
#pragma unroll 4
    for (int e = tid; e < N * w; e += DV_T) {
      const int c = e / w, x = e - c * w;
      const size_t row = (size_t)s_id[c];
      s_row[c * ld + x] = x < a.g.w ? a.g.p[row * a.g.ld + x] : a.p.p[row * a.p.ld + (x - a.g.w)];
    }
    __syncthreads();
  }

  // rel_c = (v_c - v_min) / (v_max - v_min), 0 for a flat list; rel1_c = (1 - theta) rel_c, each operation rounded once
  const float theta = a.theta, omt = __fsub_rn(1.f, theta);
  const float span = M > 0 ? __fsub_rn(vmax, vmin) : 0.f;
  float rel1[DV_SLOTS], pen[DV_SLOTS], acc[DV_SLOTS];
#pragma unroll
  for (int j = 0; j < DV_SLOTS; ++j) {
    const float rel = live[j] && span > 0.f ? __fdiv_rn(__fsub_rn(v[j], vmin), span) : 0.f;
    rel1[j] = __fmul_rn(omt, rel);
    pen[j] = 0.f; acc[j] = 0.f;
  }

  const int T = K < M ? K : M;
  const int nslots = (N + DV_T - 1) / DV_T;  // slots the pool reaches: the same in every thread
  int32_t *o_idx = a.idx + r * (size_t)K;
  float *o_val = a.val + r * (size_t)K, *o_pen = a.pen + r * (size_t)K;
  float total = 0.f;                         // (thread 0) sum of the picks' running cosine sums, in selection order
  for (int t = 0; t < T; ++t) {
    // obj_c = (1 - theta) rel_c - theta pen_c: two rounded products, one rounded subtraction, nothing fused
    unsigned long long best = 0ull;
#pragma unroll
    for (int j = 0; j < DV_SLOTS; ++j)
      if (live[j]) {
        const float obj = __fsub_rn(rel1[j], __fmul_rn(theta, pen[j]));
        const unsigned long long key = ((unsigned long long)dv_key(obj) << 32) | (uint32_t)(DV_NMAX - (tid + j * DV_T));   // never 0
        best = key > best ? key : best;
      }
    best = dv_wave_max(best);
    if (lane == 0) s_best[t & 1][wave] = best;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < DV_T / 64; ++q) { const unsigned long long o = s_best[t & 1][q]; best = o > best ? o : best; }
    const int s = DV_NMAX - (int)(uint32_t)(best & 0xffffffffull);   // the pick's pool position: known to every thread
    if (tid == 0 && t > 0) total = __fadd_rn(total, s_acc[(t - 1) & 1]);
    if (tid == (s & (DV_T - 1))) {
#pragma unroll
      for (int j = 0; j < DV_SLOTS; ++j)
        if (j == (s >> 8)) {
          o_idx[t] = pid[s]; o_val[t] = v[j]; o_pen[t] = pen[j];
          s_acc[t & 1] = acc[j];
          live[j] = false;
        }
    }
    if (t + 1 == T) break;
    // cos(c, s) for every live candidate c
    const float rns = s_rn[s];
    float dot[DV_SLOTS];
#pragma unroll
    for (int j = 0; j < DV_SLOTS; ++j) dot[j] = 0.f;
    // No per-lane branches in the loops: a wave without a live candidate skips them, in the others every lane runs every slot the
    // pool reaches (j < nslots, uniform), a lane without a candidate there on the pool's last row (one address: a broadcast);
    // what such a lane computes is never used.
    bool mine = false;
#pragma unroll
    for (int j = 0; j < DV_SLOTS; ++j) mine |= live[j];
    if (__any(mine)) {
      if (ROWS_LDS) {
        const float *zs = s_row + s * a.ld;
        int off[DV_SLOTS];
#pragma unroll
        for (int j = 0; j < DV_SLOTS; ++j) off[j] = min(tid + j * DV_T, N - 1) * a.ld;
#pragma unroll 8                              // (loads of eight x in flight; the fma chain keeps its order)
        for (int x = 0; x < w; ++x) {
          const float sv = zs[x];
#pragma unroll
          for (int j = 0; j < DV_SLOTS; ++j)
            if (j < nslots) dot[j] = fmaf(s_row[off[j] + x], sv, dot[j]);
        }
      } else {
        const size_t ids = (size_t)s_id[s];
#pragma unroll
        for (int part = 0; part < 2; ++part) {
          const SimPart z = part ? a.p : a.g;
          const float *zs = z.p + ids * z.ld;
#pragma unroll 8
          for (int x = 0; x < z.w; ++x) {
            const float sv = zs[x];
#pragma unroll
            for (int j = 0; j < DV_SLOTS; ++j)
              if (j < nslots) dot[j] = fmaf(z.p[(size_t)id[j] * z.ld + x], sv, dot[j]);   // (id[j] is a valid row in every lane)
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < DV_SLOTS; ++j)
      if (live[j]) {
        const float cs = __fmul_rn(dot[j], __fmul_rn(rn[j], rns));   // norms first: cos(c, s) has the bits of cos(s, c)
        pen[j] = t == 0 ? cs : fmaxf(pen[j], cs);
        acc[j] = __fadd_rn(acc[j], cs);
      }
  }
  for (int q = T + tid; q < K; q += DV_T) { o_idx[q] = -1; o_val[q] = 0.f; o_pen[q] = 0.f; }
  if (!a.ild) return;
  __syncthreads();
  if (tid == 0) {
    if (T > 1) total = __fadd_rn(total, s_acc[(T - 1) & 1]);
    a.ild[r] = T > 1 ? __fsub_rn(1.f, __fdiv_rn(total, (float)(T * (T - 1) / 2))) : 0.f;
  }
}

}  // namespace

extern "C" int bprx_diversify(bprx_handle *h, int32_t space, const float *rn_items, int64_t n, int32_t N, const int32_t *pool_idx,
                              const float *pool_val, int32_t K, float theta, int32_t *idx, float *val, float *pen, float *ild,
                              void *stream) {
  if (!h) return BPRX_E_INVALID;
  if (n < 0 || n >= ((int64_t)1 << 31)) BPRX_FAIL(h, BPRX_E_INVALID, "diversify: n = %lld out of range", (long long)n);
  if (!rn_items || (n > 0 && (!pool_idx || !pool_val || !idx || !val || !pen))) BPRX_FAIL(h, BPRX_E_INVALID, "diversify: null pointer");
  if (K < 1 || K > N || N > DV_NMAX) BPRX_FAIL(h, BPRX_E_INVALID, "diversify: need 1 <= K <= N <= %d, got K = %d, N = %d", DV_NMAX, K, N);
  if (!(theta >= 0.f && theta <= 1.f)) BPRX_FAIL(h, BPRX_E_INVALID, "diversify: theta = %g outside [0, 1]", (double)theta);
  hipStream_t s = (hipStream_t)stream;
  const int rc = bprx_sim_enter(h, "diversify", space, nullptr, h->cfg.num_items, s);
  if (rc || n == 0) return rc;
  DivArgs a = {};
  bprx_sim_parts(h, space, nullptr, a.g, a.p);
  a.rn = rn_items; a.I = h->cfg.num_items; a.N = N; a.K = K; a.theta = theta;
  a.pool_idx = pool_idx; a.pool_val = pool_val; a.idx = idx; a.val = val; a.pen = pen; a.ild = ild; a.errflag = h->errflag;
  const int w = a.g.w + a.p.w, ld = w | 1;
  const size_t head = (size_t)N * 2 * sizeof(float), rows = (size_t)N * ld * sizeof(float);
  // BPRX_DIVERSIFY_ROWS=global: the global-row form for every shape (the two forms return the same bits; for tests and A/B runs)
  const char *env = getenv("BPRX_DIVERSIFY_ROWS");
  const bool lds = head + rows <= (size_t)DV_DYN_MAX && !(env && !strcmp(env, "global"));
  if (lds) {
    a.ld = ld;
    hipLaunchKernelGGL(k_diversify<true>, dim3((unsigned)n), dim3(DV_T), head + rows, s, a);
    BPRX_LAUNCH_CHECK(h, "k_diversify<lds>");
  } else {
    hipLaunchKernelGGL(k_diversify<false>, dim3((unsigned)n), dim3(DV_T), head, s, a);
    BPRX_LAUNCH_CHECK(h, "k_diversify<global>");
  }
  return BPRX_OK;
}
