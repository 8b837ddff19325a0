// bprx_influence.hip -- "how far would this pick's score fall had the user not bought X": the influence of every history entry of
// a user on the scores of a list, on the user's own fold-in objective (include/bprx.h, bprx_influence).
//
// One workgroup of 256 threads per row, four phases:
//   1. build   The row's pairs are walked in tiles of IF_PT = 32.  Wave v forms pairs v, v + 4, ... of the tile: D_p = z_i - z_j
//              by fold_row (bprx_device.h, the function bprx_fold_in forms it with), x_p = w.D_p + dc_p as fold_group sums it, s_p
//              and c_p; D_p goes to LDS.  The lower triangle of A = sum_p c_p D_p D_p^T is cut into 4 x 4 blocks, each owned by
//              one thread (at most IF_NB = 4 blocks a thread) and kept in registers over the whole walk: a(i, j) = fma(c_p D_pi,
//              D_pj, a(i, j)) in ascending p, so an element does not depend on the tile size.  The blocks are then stored as a
//              packed triangle (row i starts at i (i + 1) / 2).
//   2. factor  trace(A) (one wave, lane-strided, wave_sum), lambda onto the diagonal, then a right-looking Cholesky in LDS: two
//              barriers a column, every pivot checked (> 0 and finite) by all threads alike.  L's diagonal lives in a row of its
//              own, so that the pivot is not overwritten while other waves still read it.
//   3. solve   List slots are taken in chunks of IF_KC = 8.  Wave v solves slots v and v + 4 of the chunk side by side: z_q in
//              registers (element lane + 64 e), forward and back substitution by lane broadcasts, no barrier; v_q goes to LDS.
//   4. split   The pairs are walked again (formed again: the item tables of catalogue size sit in L2 / the Infinity Cache).
//              Thread (slot, p) of the 8 x 32 = 256 forms t = s_p (v_q.D_p), a serial fma chain in ascending x; thread `slot`
//              then adds the tile's t to its running entry sum in pair order, and on an entry's last pair writes out_full, adds
//              |infl| to the total and inserts the entry into the slot's sorted top-L (strict >, entries arrive in ascending
//              position: equal values keep the lower position in front).
// No atomics (but the index error flag).  The outputs of (r, q) depend on the row, its pairs, the tables and q only.
//
// LDS, floats, n = k + d, n4 = n rounded up to 4, ldD = n4 or n4 + 4 (ldD / 4 odd: the 32 rows of a tile spread over the banks):
//     D tile 32 ldD | v 8 n4 | A n (n + 1) / 2 | diag n | s, c 2 x 32 | t 8 x 32 | top-L 2 x 8 x 32 | slot ids 8 | lambda 4
// At the bound n = 160 that is 81 648 bytes: under 80 KiB, so two workgroups share a CU's 160 KiB.  More than the 64 KiB a launch
// gets by default: the launcher raises the kernel's dynamic limit (as bprx_proj.hip does for its kernels).
#include "bprx_internal.h"

namespace {

constexpr int IF_T = 256;                    // threads of a workgroup
constexpr int IF_W = IF_T / 64;              // its waves
constexpr int IF_PT = 32;                    // pairs of a tile
constexpr int IF_KC = 8;                     // list slots of a chunk: IF_KC x IF_PT = IF_T
constexpr int IF_SB = IF_KC / IF_W;          // slots a wave solves side by side
constexpr int IF_NB = 4;                     // 4 x 4 blocks of A a thread owns at most
constexpr int IF_LMAX = 32, IF_KMAX = 1024;
constexpr int IF_NMAX = BPRX_INFLUENCE_MAX_WIDTH;
constexpr int IF_LDS_MAX = 80 * 1024;
static_assert(IF_KC * IF_PT == IF_T && IF_SB == 2, "one (slot, pair) per thread, two slots per wave");
static_assert(((IF_NMAX + 3) / 4) * ((IF_NMAX + 3) / 4 + 1) / 2 <= IF_NB * IF_T, "every block of A has an owner");

struct InfArgs {
  const float *Gi, *Bi, *P;                  // [I, k], [I], [I, PS] (nullptr for BPRMF): what fold_row reads
  int I, k, d, PS;
  const float *Gu, *Tu;                      // the caller's rows [n, k], [n, d]
  const int64_t *ptr;
  const int32_t *pos, *neg;
  int per_entry;
  float reg, damp;
  int K, L;
  const int32_t *list_idx;
  int32_t *out_item;
  float *out_infl, *out_total;
  int32_t *out_cnt;
  float *out_full;
  int64_t full_stride;
  int32_t *out_flag;
  int32_t *errflag;
};

__host__ __device__ inline int if_n4(int n) { return (n + 3) & ~3; }
__host__ __device__ inline int if_ldd(int n) { const int n4 = if_n4(n); return (n4 / 4) & 1 ? n4 : n4 + 4; }
// floats of dynamic LDS for rows n wide
__host__ __device__ inline size_t if_lds_floats(int n) {
  return (size_t)IF_PT * if_ldd(n) + (size_t)IF_KC * if_n4(n) + (size_t)n * (n + 1) / 2 + n + 2 * IF_PT + IF_KC * IF_PT +
         2 * IF_KC * IF_LMAX + IF_KC + 4;
}

__device__ __forceinline__ int if_tri(int i) { return (i * (i + 1)) >> 1; }

template <int EPL>
__global__ __launch_bounds__(IF_T) void k_influence(InfArgs a) {
  extern __shared__ __attribute__((aligned(16))) float if_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = a.k + a.d, n4 = if_n4(n), ldD = if_ldd(n), K = a.K, L = a.L, pe = a.per_entry;
  float *s_D = if_lds;                                           // [IF_PT][ldD]
  float *s_v = s_D + IF_PT * ldD;                                // [IF_KC][n4]
  float *s_A = s_v + IF_KC * n4;                                 // packed lower triangle
  float *s_dg = s_A + if_tri(n);                                 // [n] L's diagonal
  float *s_s = s_dg + n, *s_c = s_s + IF_PT;                     // [IF_PT] s_p, c_p of the tile
  float *s_t = s_c + IF_PT;                                      // [IF_KC][IF_PT]
  float *s_tv = s_t + IF_KC * IF_PT;                             // [IF_KC][IF_LMAX] top-L: influence
  int *s_te = (int *)(s_tv + IF_KC * IF_LMAX);                   //                          entry
  int *s_q = s_te + IF_KC * IF_LMAX;                             // [IF_KC] the chunk's list entries as given
  float *s_lam = (float *)(s_q + IF_KC);
  const size_t r = blockIdx.x;
  const int64_t p0 = a.ptr[r];
  const int64_t np64 = a.ptr[r + 1] - p0;
  const int m = np64 <= 0 ? 0 : (np64 > INT32_MAX ? INT32_MAX : (int)np64);
  const int M = (int)(((int64_t)m + pe - 1) / pe);

  // every slot of the row empty: a row without pairs, or one whose factorisation failed
  auto all_empty = [&](int flag) {
    for (int e = tid; e < K * L; e += IF_T) {
      a.out_item[r * (size_t)K * L + e] = -1;
      a.out_infl[r * (size_t)K * L + e] = 0.f;
    }
    for (int q = tid; q < K; q += IF_T) {
      a.out_total[r * (size_t)K + q] = 0.f;
      if (a.out_cnt) a.out_cnt[r * (size_t)K + q] = 0;
    }
    if (tid == 0 && a.out_flag) a.out_flag[r] = flag;
  };
  if (m == 0) { all_empty(0); return; }

  float w[EPL];                                                  // the row, one copy per wave
  {
    const float *gu = a.Gu + r * (size_t)a.k, *tu = a.Tu + r * (size_t)a.d;
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
      const int col = lane + 64 * e;
      w[e] = col < a.k ? gu[col] : (col < n ? tu[col - a.k] : 0.f);
    }
  }

  // pairs [t0, t0 + cnt) of the row: D_p to s_D (zero in [n, n4)), s_p and c_p to s_s / s_c
  auto form_tile = [&](int t0, int cnt) {
#pragma clang fp contract(off)
    for (int p = wave; p < cnt; p += IF_W) {
      const int64_t gp = p0 + t0 + p;
      const int it = clamp_index(a.pos[gp], a.I, a.errflag, 2), jt = clamp_index(a.neg[gp], a.I, a.errflag, 2);
      float zi[EPL], zj[EPL], ci, cj;
      fold_row<EPL>(a, it, lane, zi, ci);
      fold_row<EPL>(a, jt, lane, zj, cj);
      float s = 0.f;
#pragma unroll
      for (int e = 0; e < EPL; ++e) {
        const float dl = zi[e] - zj[e];
        s += w[e] * dl;
        const int col = lane + 64 * e;
        if (col < n4) s_D[p * ldD + col] = dl;
      }
      const float x = wave_sum(s) + (ci - cj);
      if (lane == 0) {
        const bool inr = (x >= -80.0f) && (x <= 1e8f);
        const float sg = inr ? 1.0f / (1.0f + expf(x)) : 0.f;    // sigmoid(-x)
        s_s[p] = sg;
        s_c[p] = sg * (1.0f - sg);
      }
    }
  };

  // ---- 1. A = sum_p c_p D_p D_p^T ----
  {
    const int nb4 = n4 / 4, nblk = nb4 * (nb4 + 1) / 2;
    int bi[IF_NB], bj[IF_NB];
    float acc[IF_NB][4][4];
#pragma unroll
    for (int b = 0; b < IF_NB; ++b) {
      const int idx = tid + IF_T * b;
      int i = (int)((sqrtf(8.f * (float)idx + 1.f) - 1.f) * 0.5f);
      while (if_tri(i) > idx) --i;
      while (if_tri(i + 1) <= idx) ++i;
      bi[b] = idx < nblk ? i : -1;
      bj[b] = idx < nblk ? idx - if_tri(i) : 0;
#pragma unroll
      for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int y = 0; y < 4; ++y) acc[b][x][y] = 0.f;
    }
    for (int t0 = 0; t0 < m; t0 += IF_PT) {
      const int cnt = min(IF_PT, m - t0);
      __syncthreads();                                           // the last tile is no longer read
      form_tile(t0, cnt);
      __syncthreads();
#pragma unroll
      for (int b = 0; b < IF_NB; ++b) {
        if (bi[b] < 0) continue;
        const float *di = s_D + 4 * bi[b], *dj = s_D + 4 * bj[b];
        for (int p = 0; p < cnt; ++p) {
          const float cp = s_c[p];
          const float4 vi = *(const float4 *)(di + p * ldD), vj = *(const float4 *)(dj + p * ldD);
          const float ti[4] = {cp * vi.x, cp * vi.y, cp * vi.z, cp * vi.w}, tj[4] = {vj.x, vj.y, vj.z, vj.w};
#pragma unroll
          for (int x = 0; x < 4; ++x)
#pragma unroll
            for (int y = 0; y < 4; ++y) acc[b][x][y] = fmaf(ti[x], tj[y], acc[b][x][y]);
        }
      }
    }
#pragma unroll
    for (int b = 0; b < IF_NB; ++b) {
      if (bi[b] < 0) continue;
#pragma unroll
      for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int y = 0; y < 4; ++y) {
          const int i = 4 * bi[b] + x, j = 4 * bj[b] + y;
          if (i < n && j <= i) s_A[if_tri(i) + j] = acc[b][x][y];
        }
    }
  }
  __syncthreads();

  // ---- 2. lambda, Cholesky ----
  if (wave == 0) {
    float s = 0.f;
    for (int i = lane; i < n; i += 64) s += s_A[if_tri(i) + i];
    s = wave_sum(s);
    if (lane == 0) s_lam[0] = 2.f * a.reg * (float)m + a.damp * s / (float)n;
  }
  __syncthreads();
  if (tid < n) s_A[if_tri(tid) + tid] += s_lam[0];               // (n <= IF_NMAX < IF_T)
  __syncthreads();
  int bad = 0;
  for (int j = 0; j < n; ++j) {
    const float piv = s_A[if_tri(j) + j];                        // every thread reads the same word: the branch is uniform
    if (!(piv > 0.f && piv <= 3.402823466e38f)) { bad = 1; break; }
    const float l = sqrtf(piv);
    for (int i = j + 1 + tid; i < n; i += IF_T) s_A[if_tri(i) + j] /= l;
    if (tid == 0) s_dg[j] = l;
    __syncthreads();
    for (int i = j + 1 + (tid >> 5); i < n; i += IF_T / 32) {
      const float lij = s_A[if_tri(i) + j];
      float *row = s_A + if_tri(i);
      for (int c = j + 1 + (tid & 31); c <= i; c += 32) row[c] = fmaf(-lij, s_A[if_tri(c) + j], row[c]);
    }
    __syncthreads();
  }
  if (bad) { all_empty(1); return; }
  if (tid == 0 && a.out_flag) a.out_flag[r] = 0;

  // ---- 3 / 4. the list, a chunk of IF_KC slots at a time ----
  for (int q0 = 0; q0 < K; q0 += IF_KC) {
    const int kc = min(IF_KC, K - q0);
    __syncthreads();                                             // the last chunk's v, ids and top-L are no longer read
    {
      float b[IF_SB][EPL];
#pragma unroll
      for (int u = 0; u < IF_SB; ++u) {
        const int slot = wave + IF_W * u;
        const int raw = slot < kc ? a.list_idx[r * (size_t)K + q0 + slot] : -1;
        if (raw < 0) {                                           // (wave-uniform)
#pragma unroll
          for (int e = 0; e < EPL; ++e) b[u][e] = 0.f;
        } else {
          float cq;
          fold_row<EPL>(a, clamp_index(raw, a.I, a.errflag, 2), lane, b[u], cq);
        }
        if (lane == 0 && slot < kc) s_q[slot] = raw;
      }
      // L y = z: column j of L leaves the elements below it
#pragma unroll
      for (int e0 = 0; e0 < EPL; ++e0) {
        for (int jj = 0; jj < 64; ++jj) {
          const int j = 64 * e0 + jj;
          if (j >= n) break;
          const float dg = s_dg[j];
          float y[IF_SB];
#pragma unroll
          for (int u = 0; u < IF_SB; ++u) y[u] = __shfl(b[u][e0], jj, 64) / dg;
#pragma unroll
          for (int e = e0; e < EPL; ++e) {
            const int col = lane + 64 * e;
            if (col > j && col < n) {
              const float lc = s_A[if_tri(col) + j];
#pragma unroll
              for (int u = 0; u < IF_SB; ++u) b[u][e] = fmaf(-lc, y[u], b[u][e]);
            }
          }
          if (lane == jj) {
#pragma unroll
            for (int u = 0; u < IF_SB; ++u) b[u][e0] = y[u];
          }
        }
      }
      // L^T v = y: row j of L leaves the elements before it
#pragma unroll
      for (int e0 = EPL - 1; e0 >= 0; --e0) {
        for (int jj = 63; jj >= 0; --jj) {
          const int j = 64 * e0 + jj;
          if (j >= n) continue;
          const float dg = s_dg[j];
          float y[IF_SB];
#pragma unroll
          for (int u = 0; u < IF_SB; ++u) y[u] = __shfl(b[u][e0], jj, 64) / dg;
#pragma unroll
          for (int e = 0; e <= e0; ++e) {
            const int col = lane + 64 * e;
            if (col < j) {
              const float lc = s_A[if_tri(j) + col];
#pragma unroll
              for (int u = 0; u < IF_SB; ++u) b[u][e] = fmaf(-lc, y[u], b[u][e]);
            }
          }
          if (lane == jj) {
#pragma unroll
            for (int u = 0; u < IF_SB; ++u) b[u][e0] = y[u];
          }
        }
      }
#pragma unroll
      for (int u = 0; u < IF_SB; ++u) {
        const int slot = wave + IF_W * u;
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
          const int col = lane + 64 * e;
          if (col < n4) s_v[slot * n4 + col] = b[u][e];          // (zero in [n, n4): never touched by the solves)
        }
      }
    }

    // thread `slot` (tid < kc) carries the slot's open entry, total and top-L
    float carry = 0.f, total = 0.f;
    int seen = 0;
    for (int t0 = 0; t0 < m; t0 += IF_PT) {
      const int cnt = min(IF_PT, m - t0);
      __syncthreads();                                           // the last tile's D and t are no longer read (first: v, ids written)
      form_tile(t0, cnt);
      __syncthreads();
      {
        const int slot = tid / IF_PT, p = tid % IF_PT;
        if (slot < kc && p < cnt) {
          const float *dv = s_D + p * ldD, *vv = s_v + slot * n4;
          float dot = 0.f;
          for (int x = 0; x < n4; x += 4) {
            const float4 d4 = *(const float4 *)(dv + x), v4 = *(const float4 *)(vv + x);
            dot = fmaf(v4.x, d4.x, dot); dot = fmaf(v4.y, d4.y, dot); dot = fmaf(v4.z, d4.z, dot); dot = fmaf(v4.w, d4.w, dot);
          }
          s_t[slot * IF_PT + p] = s_s[p] * dot;
        }
      }
      __syncthreads();
      if (tid < kc && s_q[tid] >= 0) {
        float *tv = s_tv + tid * IF_LMAX;
        int *te = s_te + tid * IF_LMAX;
        for (int p = 0; p < cnt; ++p) {
          const int g = t0 + p;
          carry += s_t[tid * IF_PT + p];
          if ((g + 1) % pe != 0 && g != m - 1) continue;
          const int e = g / pe;                                  // the entry is complete
          const float val = carry;
          carry = 0.f;
          if (a.out_full && e < a.full_stride) a.out_full[(r * (size_t)K + q0 + tid) * (size_t)a.full_stride + e] = val;
          total += fabsf(val);
          int i = min(seen, L);
          while (i > 0 && val > tv[i - 1]) {
            if (i < L) { tv[i] = tv[i - 1]; te[i] = te[i - 1]; }
            --i;
          }
          if (i < L) { tv[i] = val; te[i] = e; }
          ++seen;
        }
      }
    }
    __syncthreads();
    for (int x = tid; x < kc * L; x += IF_T) {
      const int slot = x / L, s = x - slot * L;
      const bool got = s_q[slot] >= 0 && s < min(L, M);
      const size_t o = (r * (size_t)K + q0 + slot) * L + s;
      a.out_item[o] = got ? a.pos[p0 + (int64_t)s_te[slot * IF_LMAX + s] * pe] : -1;
      a.out_infl[o] = got ? s_tv[slot * IF_LMAX + s] : 0.f;
    }
    if (tid < kc) {
      const bool empty = s_q[tid] < 0;
      a.out_total[r * (size_t)K + q0 + tid] = empty ? 0.f : total;
      if (a.out_cnt) a.out_cnt[r * (size_t)K + q0 + tid] = empty ? 0 : M;
    }
  }
}

template <int EPL>
void inf_launch(const InfArgs &a, unsigned n, size_t lds, hipStream_t s) {
  auto kfn = k_influence<EPL>;
  static size_t attr_lds = 0;                                    // per instantiation
  if (lds > 48 * 1024 && lds > attr_lds) {
    (void)hipFuncSetAttribute((const void *)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    attr_lds = lds;
  }
  hipLaunchKernelGGL(kfn, dim3(n), dim3(IF_T), lds, s, a);
}

}  // namespace

extern "C" int bprx_influence(bprx_handle *h, const float *Gu_rows, const float *Tu_rows, int64_t n, const int64_t *pair_ptr,
                              const int32_t *pos, const int32_t *neg, int32_t per_entry, float reg, float damp, int32_t K,
                              const int32_t *list_idx, int32_t L, int32_t *out_item, float *out_infl, float *out_total,
                              int32_t *out_cnt, float *out_full, int64_t full_stride, int32_t *out_flag, void *stream) {
  if (!h) return BPRX_E_INVALID;
  const bprx_config &c = h->cfg;
  if (n < 0 || n >= ((int64_t)1 << 31)) BPRX_FAIL(h, BPRX_E_INVALID, "influence: n = %lld out of range", (long long)n);
  if (K < 1 || K > IF_KMAX) BPRX_FAIL(h, BPRX_E_INVALID, "influence: K = %d outside [1, %d]", K, IF_KMAX);
  if (L < 1 || L > IF_LMAX) BPRX_FAIL(h, BPRX_E_INVALID, "influence: L = %d outside [1, %d]", L, IF_LMAX);
  if (per_entry < 1) BPRX_FAIL(h, BPRX_E_INVALID, "influence: per_entry = %d < 1", per_entry);
  if (!(reg >= 0.f) || !(damp >= 0.f) || !(reg <= 3.402823466e38f) || !(damp <= 3.402823466e38f) || (reg == 0.f && damp == 0.f))
    BPRX_FAIL(h, BPRX_E_INVALID, "influence: reg = %g, damp = %g: both finite and >= 0, not both 0", (double)reg, (double)damp);
  if (out_full && full_stride < 1) BPRX_FAIL(h, BPRX_E_INVALID, "influence: full_stride = %lld < 1", (long long)full_stride);
  if (!pair_ptr || !Gu_rows || (c.embed_d > 0) != (Tu_rows != nullptr)) BPRX_FAIL(h, BPRX_E_INVALID, "influence: null pointer");
  if (n && (!pos || !neg || !list_idx || !out_item || !out_infl || !out_total)) BPRX_FAIL(h, BPRX_E_INVALID, "influence: null pointer");
  hipStream_t s = (hipStream_t)stream;
  // (ACF and AttentiveFashion build the user side from attention: plain handles only; the needs of bprx_fold_in)
  const int rc = bprx_enter(h, "influence", NEED_BOUND | NEED_ROWS | NEED_P_ALL, KIND_PLAIN, s);
  if (rc) return rc;
  const int w = c.embed_k + c.embed_d;
  if (w > IF_NMAX || if_lds_floats(w) * sizeof(float) > (size_t)IF_LDS_MAX)
    BPRX_FAIL(h, BPRX_E_INVALID, "influence: k + d = %d > %d, what the kernel's LDS plan holds", w, IF_NMAX);
  if (n == 0) return BPRX_OK;
  InfArgs a = {};
  a.Gi = h->t.Gi; a.Bi = h->t.Bi; a.P = c.embed_d ? h->P : nullptr;
  a.I = c.num_items; a.k = c.embed_k; a.d = c.embed_d; a.PS = h->PS;
  a.Gu = Gu_rows; a.Tu = Tu_rows;
  a.ptr = pair_ptr; a.pos = pos; a.neg = neg; a.per_entry = per_entry;
  a.reg = reg; a.damp = damp; a.K = K; a.L = L; a.list_idx = list_idx;
  a.out_item = out_item; a.out_infl = out_infl; a.out_total = out_total; a.out_cnt = out_cnt;
  a.out_full = out_full; a.full_stride = out_full ? full_stride : 0; a.out_flag = out_flag; a.errflag = h->errflag;
  const size_t lds = if_lds_floats(w) * sizeof(float);
  switch ((w + 63) / 64) {
    case 1: inf_launch<1>(a, (unsigned)n, lds, s); break;
    case 2: inf_launch<2>(a, (unsigned)n, lds, s); break;
    default: inf_launch<3>(a, (unsigned)n, lds, s); break;
  }
  BPRX_LAUNCH_CHECK(h, "k_influence");
  return BPRX_OK;
}
