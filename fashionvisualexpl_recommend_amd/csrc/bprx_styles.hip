// bprx_styles.hip -- style clusters: spherical k-means of the item space of bprx_sim_* (include/bprx.h).
//   k_style_assign  the cosine of a range of item rows with S centroids as the fp32 MFMA GEMM of k_sim_gemm, fused with a running
//                   (best, arg-best, second) per row: nothing of size rows x S leaves the workgroup
//   k_style_update  the fp64 sum of every cluster's unit member rows in an order fixed by the cluster's member list, normalised
//                   and rounded once to fp32; no atomics
#include "bprx_internal.h"

#include <climits>

namespace {

using namespace bprx_gemm;   // f32x16, TM / TN / GKC / GLD, gemm_phase

// The running result of a row: the best (value, index) in the order "larger value first, equal values by smaller index", and the
// largest value among the others.  st_merge gives the two best of the union, so it is associative and commutative: the result
// does not depend on how the centroids are spread over lanes, waves and tiles.
struct StyleBest {
  float best;
  int idx;
  float second;
};

__device__ __forceinline__ StyleBest st_merge(const StyleBest a, const StyleBest b) {
  const bool a_wins = a.best > b.best || (a.best == b.best && a.idx < b.idx);
  const StyleBest win = a_wins ? a : b, lose = a_wins ? b : a;
  return {win.best, win.idx, fmaxf(win.second, lose.best)};   // (lose.second <= lose.best)
}

// c(q, s) = <z_q, cent_s> rn_q for the query rows q in [q0, q1) against S centroids: style[q - q0] = the arg-max over s (ties:
// the smallest s), cos[q - q0] the maximum, second[q - q0] the largest c(q, s) over s != style (-inf for S == 1; second may be
// nullptr).  One workgroup owns 128 query rows and walks the centroids in tiles of 128; a tile is k_sim_gemm's tile (one
// gemm_phase per part of z, A = the query rows, B = the centroid rows, whose Gi part comes first), so the sums are its sums:
// exact fp32 products, x-ordered from +0.  The norm is multiplied last, before any comparison.  Per tile every lane folds its two
// columns, the 32 column lanes of a row fold with xor shuffles, the two column waves meet in LDS, and thread r < 128 keeps row
// r's running result in registers.  A row with rn_q == 0 gets (-1, 0.0, 0.0).
__global__ __launch_bounds__(256) void k_style_assign(SimPart a0, SimPart a1, SimPart c0, SimPart c1, int S, int q0, int q1,
                                                      const float *__restrict__ rn_q, int32_t *__restrict__ style,
                                                      float *__restrict__ cosv, float *__restrict__ second) {
  __shared__ float As[TM][GLD];
  __shared__ float Bs[TN][GLD];
  __shared__ float rnS[TM];
  __shared__ float tbest[2][TM], tsec[2][TM];
  __shared__ int tidx[2][TM];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, wr = w >> 1, wc = w & 1;
  const int qb = q0 + blockIdx.x * TM;
  const int arows = min(TM, q1 - qb);
  if (threadIdx.x < TM) rnS[threadIdx.x] = (int)threadIdx.x < arows ? rn_q[qb + threadIdx.x] : 0.f;
  StyleBest run = {-INFINITY, INT_MAX, -INFINITY};            // of row threadIdx.x (threads below TM)
  for (int s0 = 0; s0 < S; s0 += TN) {
    const int brows = min(TN, S - s0);
    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
    // (the first barrier of a phase also orders rnS and the previous tile's reads of tbest / tidx / tsec before this tile's writes)
    if (a0.w) gemm_phase(a0.p, a0.ld, qb, arows, c0.p, c0.ld, s0, brows, a0.w, As, Bs, acc, wr, wc, lane);
    if (a1.w) gemm_phase(a1.p, a1.ld, qb, arows, c1.p, c1.ld, s0, brows, a1.w, As, Bs, acc, wr, wc, lane);
    // C/D layout of the 32x32 MFMA: col = lane & 31, row = (reg & 3) + 8*(reg >> 2) + 4*(lane >> 5)
    const int col0 = s0 + wc * 64 + (lane & 31), col1 = col0 + 32;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = wr * 64 + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        const float rn = rnS[row];
        StyleBest m = {-INFINITY, INT_MAX, -INFINITY};
        if (col0 < S) m = {__fmul_rn(acc[a][0][r], rn), col0, -INFINITY};
        if (col1 < S) m = st_merge(m, {__fmul_rn(acc[a][1][r], rn), col1, -INFINITY});
#pragma unroll
        for (int off = 1; off < 32; off <<= 1)                // the 32 lanes that hold this row (lane >> 5 is kept)
          m = st_merge(m, {__shfl_xor(m.best, off), __shfl_xor(m.idx, off), __shfl_xor(m.second, off)});
        if ((lane & 31) == 0) {
          tbest[wc][row] = m.best;
          tidx[wc][row] = m.idx;
          tsec[wc][row] = m.second;
        }
      }
    __syncthreads();
    if (threadIdx.x < TM) {
      const int row = threadIdx.x;
      run = st_merge(run, st_merge({tbest[0][row], tidx[0][row], tsec[0][row]}, {tbest[1][row], tidx[1][row], tsec[1][row]}));
    }
  }
  if ((int)threadIdx.x < arows) {
    const int row = threadIdx.x;
    const bool zero = rnS[row] == 0.f;
    const size_t o = (size_t)(qb - q0) + row;
    style[o] = zero ? -1 : run.idx;
    cosv[o] = zero ? 0.f : run.best;
    if (second) second[o] = zero ? 0.f : run.second;
  }
}

constexpr int SU_SUB = 16;           // members per sub-chunk: one wave sums a sub-chunk in ascending member order
constexpr int SU_CHUNK = 4 * SU_SUB; // members a workgroup takes per round: sub-chunk v of the round goes to wave v
constexpr int SU_WMAX = 4096;        // the widest item space: one fp64 sum per column in LDS (32 KB)

// sum_s = sum over the members i of cluster s of fl32(z_ix rn_i), in fp64, one workgroup per cluster.  The member list is cut at
// multiples of SU_SUB = 16: a sub-chunk is added up in ascending list order from +0, and the sub-chunk partials are added to the
// cluster's sum in ascending sub-chunk order (four sub-chunks travel per round, one per wave, and meet in LDS; every wave keeps
// the whole sum, so the order is the list's alone).  Lane l of a wave owns column x0 + l of a 64-column strip, so a member row is
// read in 256-byte pieces.  Then |sum|^2 is added up in fp64 (lane l takes the columns l, l + 64, .. in ascending order; the 64
// lane sums meet in an xor tree), and cent_out_s = sum_s / |sum_s|, mass[s] = |sum_s|, each rounded once to fp32.  An empty
// cluster, or |sum|^2 == 0, copies cent_prev_s and reports mass 0.  A member id outside [0, I) is skipped and flagged.
__global__ __launch_bounds__(256) void k_style_update(SimPart a, SimPart b, int I, const float *__restrict__ rn,
                                                      const int64_t *__restrict__ mptr, const int32_t *__restrict__ mitems,
                                                      const float *__restrict__ cent_prev, float *__restrict__ cent_out,
                                                      float *__restrict__ mass, int32_t *__restrict__ errflag) {
  __shared__ double sumS[SU_WMAX];
  __shared__ double part[4][64];
  __shared__ double n2S;
  const int lane = threadIdx.x & 63, v = threadIdx.x >> 6;
  const int s = blockIdx.x, w = a.w + b.w;
  const int64_t m0 = mptr[s], n = mptr[s + 1] - m0;
  for (int x0 = 0; x0 < w; x0 += 64) {
    const int x = x0 + lane;
    const bool live = x < w;
    const bool in_a = x < a.w;
    const float *__restrict__ col = in_a ? a.p + x : b.p + (x - a.w);
    const int ld = in_a ? a.ld : b.ld;
    double acc = 0.0;
    for (int64_t c = 0; c < n; c += SU_CHUNK) {
      const int64_t mm = c + v * SU_SUB + (lane & (SU_SUB - 1));
      int mine = -1;                                          // lane j of every 16 holds member j of this wave's sub-chunk
      if (mm < n) {
        mine = mitems[m0 + mm];
        if ((unsigned)mine >= (unsigned)I) {                  // reported by bprx_sync_check, never dereferenced
          *errflag = 5;
          mine = -1;
        }
      }
      float zv[SU_SUB];
#pragma unroll
      for (int j = 0; j < SU_SUB; ++j) {
        const int id = __shfl(mine, j);
        zv[j] = (id >= 0 && live) ? __fmul_rn(col[(size_t)id * ld], rn[id]) : 0.f;
      }
      double q = 0.0;
#pragma unroll
      for (int j = 0; j < SU_SUB; ++j) q += (double)zv[j];    // (a skipped member adds +0)
      part[v][lane] = q;
      __syncthreads();
#pragma unroll
      for (int u = 0; u < 4; ++u) acc += part[u][lane];
      __syncthreads();
    }
    if (v == 0 && live) sumS[x] = acc;
  }
  __syncthreads();
  if (v == 0) {
    double n2 = 0.0;
    for (int x = lane; x < w; x += 64) n2 += sumS[x] * sumS[x];
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) n2 += __shfl_xor(n2, off);
    if (lane == 0) n2S = n2;
  }
  __syncthreads();
  const double n2 = n2S;
  const bool keep = !(n2 > 0.0);                              // empty, or the rows cancel exactly
  const double len = sqrt(n2);
  for (int x = threadIdx.x; x < w; x += 256)
    cent_out[(size_t)s * w + x] = keep ? cent_prev[(size_t)s * w + x] : (float)(sumS[x] / len);
  if (threadIdx.x == 0) mass[s] = keep ? 0.f : (float)len;
}

}  // namespace

// ---- style clusters: bprx_style_assign / bprx_style_update (include/bprx.h) ----
extern "C" int bprx_style_assign(bprx_handle *h, int32_t space, const float *Pq, int64_t nq, int64_t q0, int64_t q1, const float *rn_q,
                                 const float *cent, int32_t S, int32_t *style, float *cos, float *second, void *stream) {
  if (!h) return BPRX_E_INVALID;
  if (!rn_q || !cent || !style || !cos) BPRX_FAIL(h, BPRX_E_INVALID, "style_assign: null pointer");
  if (S < 1 || S > BPRX_STYLES_MAX) BPRX_FAIL(h, BPRX_E_INVALID, "style_assign: S = %d outside [1, %d]", S, BPRX_STYLES_MAX);
  if (q0 < 0 || q0 > q1 || q1 > nq)
    BPRX_FAIL(h, BPRX_E_INVALID, "style_assign: bad query range [%lld,%lld) of %lld", (long long)q0, (long long)q1, (long long)nq);
  hipStream_t s = (hipStream_t)stream;
  const int rc = bprx_sim_enter(h, "style_assign", space, Pq, nq, s);
  if (rc || q0 == q1) return rc;
  SimPart ag, ap;
  bprx_sim_parts(h, space, Pq, ag, ap);
  const int w = ag.w + ap.w;
  const SimPart cg = {cent, ag.w, w}, cp = {cent + ag.w, ap.w, w};   // a centroid row: [Gi part | P part]
  hipLaunchKernelGGL(k_style_assign, dim3((unsigned)((q1 - q0 + TM - 1) / TM)), dim3(256), 0, s, ag, ap, cg, cp, (int)S, (int)q0,
                     (int)q1, rn_q, style, cos, second);
  BPRX_LAUNCH_CHECK(h, "k_style_assign");
  return BPRX_OK;
}

extern "C" int bprx_style_update(bprx_handle *h, int32_t space, const float *rn_items, const int64_t *member_ptr,
                                 const int32_t *member_items, int32_t S, const float *cent_prev, float *cent_out, float *mass,
                                 void *stream) {
  if (!h) return BPRX_E_INVALID;
  if (!rn_items || !member_ptr || !member_items || !cent_prev || !cent_out || !mass)
    BPRX_FAIL(h, BPRX_E_INVALID, "style_update: null pointer");
  if (S < 1 || S > BPRX_STYLES_MAX) BPRX_FAIL(h, BPRX_E_INVALID, "style_update: S = %d outside [1, %d]", S, BPRX_STYLES_MAX);
  hipStream_t s = (hipStream_t)stream;
  const int rc = bprx_sim_enter(h, "style_update", space, nullptr, h->cfg.num_items, s);
  if (rc) return rc;
  SimPart g, p;
  bprx_sim_parts(h, space, nullptr, g, p);
  if (g.w + p.w > SU_WMAX)
    BPRX_FAIL(h, BPRX_E_INVALID, "style_update: an item space of %d numbers is wider than %d (one fp64 sum per column in LDS)", g.w + p.w,
              SU_WMAX);
  hipLaunchKernelGGL(k_style_update, dim3((unsigned)S), dim3(256), 0, s, g, p, h->cfg.num_items, rn_items, member_ptr, member_items,
                     cent_prev, cent_out, mass, h->errflag);
  BPRX_LAUNCH_CHECK(h, "k_style_update");
  return BPRX_OK;
}
