// bprx_explain.hip -- bprx_feat_explain (include/bprx.h): the VBPR / GradFashion score per feature column.
//
//   x_ui = Bi_i + Gu_u.Gi_i + sum_c F_ic w_uc          w_uc = Bp[c] + sum_x E[c,x] Tu[u,x]
//
// k_feat_explain: a workgroup of four waves owns a tile of FX_TILE consecutive pairs and walks the maximal runs of equal
// (clamped) user inside it.  Per run the 256 threads form w_u[0..ncols) in LDS (fp32, 4 * feat_dim bytes of dynamic LDS, the
// kernel's only LDS); after a barrier the waves take the run's pairs, one wave per pair.  A run that crosses a tile edge is
// recomputed by the next workgroup; unsorted input gives runs of one.  No workspace, no atomics.
//
// w_uc: 16 LANES per column, so that a wave reads four E rows per load instruction as whole contiguous segments (d = 64: one
// 16-byte load per lane, 1 KB contiguous per wave; one thread per row would touch 64 cache lines per instruction and re-fetch
// every line d / 4 times).  Lane g of the 16 takes x = 4g .. 4g+3, then 4g+64 .. (d % 4 != 0: x = g, g+16, ..) as one fma chain
// in ascending x, the 16 partial sums meet in an xor butterfly (1, 2, 4, 8), and Bp[c] is added last: a function of (E[c,:],
// Bp[c], Tu_u) alone, the same instruction sequence whichever lanes, wave or workgroup form the column.
//
// Per pair: lane l holds V consecutive columns of each chunk of 64 V (one 16-byte load of the feature row: V = 4 fp32, 8 bf16,
// 16 fp8; V = 1 where the row is not 16-byte aligned).  c = f * w is rounded once; the lane adds its c in ascending column order
// and the butterfly of bprx_device.h adds the 64 partials: one order per (ncols, load width).  The `top` largest c live one per
// lane in lanes 0 .. top-1, sorted by (value descending, column ascending): per element slot one ballot finds the lanes whose
// value beats the last slot, those are inserted one at a time (rank by a second ballot, the tail shifts one lane up).  The order
// is total -- equal values (+0.0 == -0.0) rank by column -- so the list does not depend on the order in which columns arrive.
#include "bprx_internal.h"

namespace {

constexpr int FX_TILE = 32;          // pairs per workgroup

struct FeatExplainArgs {
  const float *Gu, *Gi, *Bi, *Tu, *E, *Bp;
  const void *F;
  const int32_t *user, *item;
  int64_t n;
  int U, I, k, d, D, ncols, top;
  int e_vec;                         // E rows are read with 16-byte loads (d % 4 == 0)
  int map_vec;                       // map rows are written with 16-byte stores (ncols % 4 == 0, aligned base)
  float feat_scale;                  // fp8: the codes hold f * feat_scale
  float *score, *base, *visual;
  int32_t *col;
  float *contrib, *map;
  int32_t *errflag;
};

// OCP e4m3fn code -> its value (sign 1, exponent 4 with bias 7, mantissa 3; no infinities, S.1111.111 is NaN)
__device__ __forceinline__ float e4m3fn_value(uint32_t b) {
  const uint32_t s = (b & 0x80u) << 24, e = (b >> 3) & 15u, m = b & 7u;
  if (e == 15u && m == 7u) return __uint_as_float(s | 0x7fc00000u);
  if (e == 0u) {                                               // subnormal: m * 2^-9
    if (m == 0u) return __uint_as_float(s);
    const uint32_t sh = (uint32_t)__clz((int)m) - 29u;         // 2, 1, 0 for m = 1, 2..3, 4..7
    return __uint_as_float(s | ((120u - sh) << 23) | (((m << sh) & 3u) << 21));
  }
  return __uint_as_float(s | ((e + 120u) << 23) | (m << 20));
}

// V features of one row from column c0 (c0 % V == 0; the V columns lie inside the row)
template <int V> __device__ __forceinline__ void load_feats(const float *row, int c0, float scale, float (&f)[V]) {
  if constexpr (V == 4) {
    const float4 v = *reinterpret_cast<const float4 *>(row + c0);
    f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w;
  } else {
    f[0] = row[c0];
  }
}
template <int V> __device__ __forceinline__ void load_feats(const uint16_t *row, int c0, float scale, float (&f)[V]) {
  if constexpr (V == 8) {
    const uint4 v = *reinterpret_cast<const uint4 *>(row + c0);
    const uint32_t q[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      f[2 * j] = __uint_as_float(q[j] << 16);
      f[2 * j + 1] = __uint_as_float(q[j] & 0xffff0000u);
    }
  } else {
    f[0] = __uint_as_float((uint32_t)row[c0] << 16);
  }
}
template <int V> __device__ __forceinline__ void load_feats(const uint8_t *row, int c0, float scale, float (&f)[V]) {
  if constexpr (V == 16) {
    const uint4 v = *reinterpret_cast<const uint4 *>(row + c0);
    const uint32_t q[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 16; ++j) f[j] = e4m3fn_value((q[j >> 2] >> (8 * (j & 3))) & 0xffu) / scale;
  } else {
    f[0] = e4m3fn_value(row[c0]) / scale;
  }
}

// (av, ac) ranks before (bv, bc): larger value first (floats: +0.0 == -0.0), the lower column among equal values
__device__ __forceinline__ bool ranks_before(float av, int ac, float bv, int bc) { return av > bv || (av == bv && ac < bc); }

// NEW (bprx_feat_explain_new): the pairs are (user, row of a table the model was not trained on): A.item indexes the A.I rows
// of A.F, there is no Gu.Gi dot and no Bi -- score is the visual sum; base and visual are not written.  Everything else is the
// same code.
template <typename FT, int V, bool NEW>
__global__ __launch_bounds__(256) void k_feat_explain(FeatExplainArgs A) {
#pragma clang fp contract(off)   // c = f * w is rounded before it is added: visual is the sum of the stored contributions
  extern __shared__ float w[];                               // [D] w_u of the current run
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int k = A.k, d = A.d, D = A.D, ncols = A.ncols, top = A.top;
  const int64_t p0 = (int64_t)blockIdx.x * FX_TILE;
  const int tile = (int)(A.n - p0 < FX_TILE ? A.n - p0 : FX_TILE);
  // every wave keeps the tile's (clamped) pairs in its lanes 0 .. tile-1
  int pu = -1, pi = 0;
  if (lane < tile) {
    pu = clamp_index(A.user[p0 + lane], A.U, A.errflag, 1);
    pi = clamp_index(A.item[p0 + lane], A.I, A.errflag, 2);
  }
  const FT *F = static_cast<const FT *>(A.F);
  int s = 0;
  while (s < tile) {
    const int u = __builtin_amdgcn_readfirstlane(__shfl(pu, s, 64));
    const unsigned long long other = __ballot(lane >= s && lane < tile && pu != u);
    const int e = other ? __ffsll((long long)other) - 1 : tile;          // the run is [s, e)
    // ---- w_u: 16 lanes per column, four columns per wave and round ----
    const float *tu = A.Tu + (size_t)u * d;
    const int g = lane & 15;
    float4 t0 = make_float4(0.f, 0.f, 0.f, 0.f);                 // Tu_u[4g .. 4g+3]: the lane's first (for d <= 64 its only) segment
    if (A.e_vec && 4 * g < d) t0 = *reinterpret_cast<const float4 *>(tu + 4 * g);
    for (int c0 = 0; c0 < D; c0 += 16) {
      const int c = c0 + wave * 4 + (lane >> 4);
      float part = 0.f;
      if (c < ncols) {
        const float *er = A.E + (size_t)c * d;
        if (A.e_vec) {
          if (4 * g < d) {
            const float4 ev = *reinterpret_cast<const float4 *>(er + 4 * g);
            part = fmaf(ev.w, t0.w, fmaf(ev.z, t0.z, fmaf(ev.y, t0.y, ev.x * t0.x)));
          }
          for (int x = 4 * g + 64; x < d; x += 64) {
            const float4 ev = *reinterpret_cast<const float4 *>(er + x), tv = *reinterpret_cast<const float4 *>(tu + x);
            part = fmaf(ev.w, tv.w, fmaf(ev.z, tv.z, fmaf(ev.y, tv.y, fmaf(ev.x, tv.x, part))));
          }
        } else {
          for (int x = g; x < d; x += 16) part = fmaf(er[x], tu[x], part);
        }
      }
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) part += __shfl_xor(part, o, 64);    // the 16 lanes of a column end with the same bits
      if (g == 0 && c < D) w[c] = c < ncols ? A.Bp[c] + part : 0.f;
    }
    __syncthreads();
    // ---- the run's pairs: one wave per pair ----
    for (int q = s + wave; q < e; q += 4) {
      const int64_t p = p0 + q;
      const int i = __builtin_amdgcn_readfirstlane(__shfl(pi, q, 64));
      float base = 0.f;
      if constexpr (!NEW) {
        const float *gu = A.Gu + (size_t)u * k, *gi = A.Gi + (size_t)i * k;
        float dot = 0.f;
        for (int c = lane; c < k; c += 64) dot = fmaf(gu[c], gi[c], dot);
        dot = wave_sum(dot);
        base = A.Bi[i] + dot;
      }
      const FT *row = F + (size_t)i * D;
      float *mrow = A.map ? A.map + p * ncols : nullptr;
      float acc = 0.f;                                       // this lane's share of visual
      float tv = 0.f, thr_v = 0.f;                           // this lane's slot (lane < cnt); (thr_v, thr_c) = the last slot once all are taken
      int tp = -1, thr_c = 0, cnt = 0;
      for (int cb = 0; cb < ncols; cb += 64 * V) {
        const int c0 = cb + lane * V;
        float f[V], c[V];
        if (c0 < ncols) {
          load_feats<V>(row, c0, A.feat_scale, f);
          float wc[V];
          if constexpr (V >= 4) {
#pragma unroll
            for (int j = 0; j < V; j += 4) {
              const float4 wv = *reinterpret_cast<const float4 *>(w + c0 + j);
              wc[j] = wv.x; wc[j + 1] = wv.y; wc[j + 2] = wv.z; wc[j + 3] = wv.w;
            }
          } else {
            wc[0] = w[c0];
          }
#pragma unroll
          for (int j = 0; j < V; ++j) c[j] = f[j] * wc[j];
#pragma unroll
          for (int j = 0; j < V; ++j)
            if (c0 + j < ncols) acc = acc + c[j];
          if (mrow) {
            if (V >= 4 && A.map_vec) {
#pragma unroll
              for (int j = 0; j + 3 < V; j += 4)
                if (c0 + j < ncols) *reinterpret_cast<float4 *>(mrow + c0 + j) = make_float4(c[j], c[j + 1], c[j + 2], c[j + 3]);
            } else {
#pragma unroll
              for (int j = 0; j < V; ++j)
                if (c0 + j < ncols) mrow[c0 + j] = c[j];
            }
          }
        } else {
#pragma unroll
          for (int j = 0; j < V; ++j) c[j] = 0.f;
        }
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const int cc = c0 + j;
          unsigned long long m = __ballot(cc < ncols && (cnt < top || ranks_before(c[j], cc, thr_v, thr_c)));
          while (m) {
            const int src = __ffsll((long long)m) - 1;
            m &= m - 1;
            const float cv = __shfl(c[j], src, 64);
            const int ccol = cb + src * V + j;
            if (cnt < top || ranks_before(cv, ccol, thr_v, thr_c)) {       // (an earlier insert of this round may have raised the bar)
              const int rank = __popcll(__ballot(lane < cnt && ranks_before(tv, tp, cv, ccol)));
              const float uv = __shfl_up(tv, 1, 64);
              const int up = __shfl_up(tp, 1, 64);
              if (lane == rank) {
                tv = cv;
                tp = ccol;
              } else if (lane > rank && lane < top) {
                tv = uv;
                tp = up;
              }
              if (cnt < top) ++cnt;
              if (cnt == top) {
                thr_v = __shfl(tv, top - 1, 64);
                thr_c = __shfl(tp, top - 1, 64);
              }
            }
          }
        }
      }
      const float visual = wave_sum(acc);
      if (lane == 0) {
        if constexpr (NEW) {
          A.score[p] = visual;
        } else {
          A.base[p] = base;
          A.visual[p] = visual;
          A.score[p] = base + visual;
        }
      }
      if (lane < top) {
        A.col[p * top + lane] = lane < cnt ? tp : -1;
        A.contrib[p * top + lane] = lane < cnt ? tv : 0.f;
      }
    }
    __syncthreads();                                         // w is rewritten by the next run
    s = e;
  }
}

template <typename FT, bool NEW = false>
void launch(const FeatExplainArgs &A, bool vec, unsigned blocks, size_t lds, hipStream_t s) {
  constexpr int V = 16 / (int)sizeof(FT);
  if (vec) hipLaunchKernelGGL((k_feat_explain<FT, V, NEW>), dim3(blocks), dim3(256), lds, s, A);
  else hipLaunchKernelGGL((k_feat_explain<FT, 1, NEW>), dim3(blocks), dim3(256), lds, s, A);
}

}  // namespace

extern "C" int bprx_feat_explain(bprx_handle *h, const void *F, const int32_t *user, const int32_t *item, int64_t n, int32_t ncols,
                                 int32_t top, float *score, float *base, float *visual, int32_t *col, float *contrib, float *map,
                                 void *stream) {
  if (!h) return BPRX_E_INVALID;
  const bprx_config &c = h->cfg;
  if (n < 0 || n >= ((int64_t)1 << 31)) BPRX_FAIL(h, BPRX_E_INVALID, "feat_explain: n = %lld out of range", (long long)n);
  if (ncols < 1 || ncols > c.feat_dim) BPRX_FAIL(h, BPRX_E_INVALID, "feat_explain: ncols = %d outside [1, feat_dim = %d]", ncols, c.feat_dim);
  if (top < 1 || top > 32) BPRX_FAIL(h, BPRX_E_INVALID, "feat_explain: top = %d outside [1, 32]", top);
  if (c.feat_dim > 16384)
    BPRX_FAIL(h, BPRX_E_INVALID, "feat_explain: feat_dim = %d > 16384 (one user's fp32 w row must fit in 64 KB of LDS)", c.feat_dim);
  if (n && (!F || !user || !item || !score || !base || !visual || !col || !contrib))
    BPRX_FAIL(h, BPRX_E_INVALID, "feat_explain: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const int rc = bprx_enter(h, "feat_explain", NEED_BOUND | NEED_ROWS, KIND_VBPR, s);
  if (rc || n == 0) return rc;
  FeatExplainArgs A;
  A.Gu = h->t.Gu; A.Gi = h->t.Gi; A.Bi = h->t.Bi; A.Tu = h->t.Tu; A.E = h->t.E; A.Bp = h->t.Bp;
  A.F = F; A.user = user; A.item = item; A.n = n;
  A.U = c.num_users; A.I = c.num_items; A.k = c.embed_k; A.d = c.embed_d; A.D = c.feat_dim; A.ncols = ncols; A.top = top;
  A.e_vec = c.embed_d % 4 == 0;                                        // (bind checked the 16-byte alignment of E)
  A.map_vec = map && ncols % 4 == 0 && ((uintptr_t)map & 15) == 0;
  A.feat_scale = c.feat_dtype == BPRX_F_FP8 ? c.feat_scale : 1.0f;
  A.score = score; A.base = base; A.visual = visual; A.col = col; A.contrib = contrib; A.map = map;
  A.errflag = h->errflag;
  const size_t esz = c.feat_dtype == BPRX_F_FP32 ? 4 : (c.feat_dtype == BPRX_F_BF16 ? 2 : 1);
  const bool vec = ((uintptr_t)F & 15) == 0 && ((size_t)c.feat_dim * esz) % 16 == 0;   // every feature row starts 16-byte aligned
  const unsigned blocks = (unsigned)((n + FX_TILE - 1) / FX_TILE);
  const size_t lds = (size_t)c.feat_dim * sizeof(float);
  if (c.feat_dtype == BPRX_F_BF16) launch<uint16_t>(A, vec, blocks, lds, s);
  else if (c.feat_dtype == BPRX_F_FP8) launch<uint8_t>(A, vec, blocks, lds, s);
  else launch<float>(A, vec, blocks, lds, s);
  BPRX_LAUNCH_CHECK(h, "k_feat_explain");
  return BPRX_OK;
}

extern "C" int bprx_feat_explain_new(bprx_handle *h, const void *Fnew, int64_t n_new, const int32_t *user, const int32_t *row,
                                     int64_t n, int32_t ncols, int32_t top, float *score, int32_t *col, float *contrib, float *map,
                                     void *stream) {
  if (!h) return BPRX_E_INVALID;
  const bprx_config &c = h->cfg;
  if (n < 0 || n >= ((int64_t)1 << 31)) BPRX_FAIL(h, BPRX_E_INVALID, "feat_explain_new: n = %lld out of range", (long long)n);
  if (n_new < 0 || n_new >= ((int64_t)1 << 31)) BPRX_FAIL(h, BPRX_E_INVALID, "feat_explain_new: n_new = %lld out of range", (long long)n_new);
  if (ncols < 1 || ncols > c.feat_dim) BPRX_FAIL(h, BPRX_E_INVALID, "feat_explain_new: ncols = %d outside [1, feat_dim = %d]", ncols, c.feat_dim);
  if (top < 1 || top > 32) BPRX_FAIL(h, BPRX_E_INVALID, "feat_explain_new: top = %d outside [1, 32]", top);
  if (c.feat_dim > 16384)
    BPRX_FAIL(h, BPRX_E_INVALID, "feat_explain_new: feat_dim = %d > 16384 (one user's fp32 w row must fit in 64 KB of LDS)", c.feat_dim);
  if (n && n_new == 0) BPRX_FAIL(h, BPRX_E_INVALID, "feat_explain_new: %lld pairs of an empty table", (long long)n);
  if (n && (!Fnew || !user || !row || !score || !col || !contrib)) BPRX_FAIL(h, BPRX_E_INVALID, "feat_explain_new: null pointer");
  hipStream_t s = (hipStream_t)stream;
  // (NEED_ET: not read here, it is the image bprx_project_rows scores with)
  const int rc = bprx_enter(h, "feat_explain_new", NEED_BOUND | NEED_ROWS | NEED_ET, KIND_VBPR_NO_FP8, s);
  if (rc || n == 0) return rc;
  FeatExplainArgs A;
  A.Gu = nullptr; A.Gi = nullptr; A.Bi = nullptr; A.Tu = h->t.Tu; A.E = h->t.E; A.Bp = h->t.Bp;
  A.F = Fnew; A.user = user; A.item = row; A.n = n;
  A.U = c.num_users; A.I = (int)n_new; A.k = c.embed_k; A.d = c.embed_d; A.D = c.feat_dim; A.ncols = ncols; A.top = top;
  A.e_vec = c.embed_d % 4 == 0;
  A.map_vec = map && ncols % 4 == 0 && ((uintptr_t)map & 15) == 0;
  A.feat_scale = 1.0f;
  A.score = score; A.base = nullptr; A.visual = nullptr; A.col = col; A.contrib = contrib; A.map = map;
  A.errflag = h->errflag;
  const size_t esz = c.feat_dtype == BPRX_F_FP32 ? 4 : 2;
  const bool vec = ((uintptr_t)Fnew & 15) == 0 && ((size_t)c.feat_dim * esz) % 16 == 0;
  const unsigned blocks = (unsigned)((n + FX_TILE - 1) / FX_TILE);
  const size_t lds = (size_t)c.feat_dim * sizeof(float);
  if (c.feat_dtype == BPRX_F_BF16) launch<uint16_t, true>(A, vec, blocks, lds, s);
  else launch<float, true>(A, vec, blocks, lds, s);
  BPRX_LAUNCH_CHECK(h, "k_feat_explain<new>");
  return BPRX_OK;
}
