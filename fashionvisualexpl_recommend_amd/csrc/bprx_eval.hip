// bprx_eval.hip -- device-side evaluation.
//   k_score_gemm   predict_all rows [u0,u1): out[u][i] = Bi[i] + <Gu[u],Gi[i]> (+ <Tu[u],P_i[0:d]> + P_i[d])
//                  (BPRMF.py:78-85 / VBPR.py:88-97) as an fp32-in / fp32-accumulate MFMA GEMM
//                  (v_mfma_f32_32x32x2_f32: exact fp32 products, k-ordered fp32 sums -- no bf16 in the ranking path)
//   k_eval_users   Evaluator._eval_by_user (Evaluator.py:82-128) from a block of score rows: exact integer rank
//                  counting, so for identical fp32 scores the metrics equal the reference's definitions bit for bit
//                  (ties included: negatives rank before the held-out items, `>=` counts against them).
// The U x I matrix is never resident: the caller walks user blocks (scores of one block: nb x I fp32 in HBM).
#include "bprx_internal.h"

namespace {

using namespace bprx_gemm;   // f32x16, TM / TN / GKC / GLD, gemm_phase (bprx_internal.h)

struct GemmArgs {
  const float *Gu, *Gi, *Bi, *Tu, *P;
  int U, I, k, d, PS;
};

__global__ __launch_bounds__(256) void k_score_gemm(GemmArgs g, int u0, int u1, float *__restrict__ out) {
  __shared__ float As[TM][GLD];
  __shared__ float Bs[TN][GLD];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, wr = w >> 1, wc = w & 1;
  const int i0 = blockIdx.x * TN, ub = u0 + blockIdx.y * TM;
  const int arows = min(TM, u1 - ub), brows = min(TN, g.I - i0);
  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
  gemm_phase(g.Gu, g.k, ub, arows, g.Gi, g.k, i0, brows, g.k, As, Bs, acc, wr, wc, lane);
  if (g.d) gemm_phase(g.Tu, g.d, ub, arows, g.P, g.PS, i0, brows, g.d, As, Bs, acc, wr, wc, lane);
  // C/D layout of the 32x32 MFMA: col = lane & 31, row = (reg & 3) + 8*(reg >> 2) + 4*(lane >> 5)
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const int ic = i0 + wc * 64 + b * 32 + (lane & 31);
    if (ic >= g.I) continue;
    const float bias = g.Bi[ic] + (g.d ? g.P[(size_t)ic * g.PS + g.d] : 0.f);
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ur = ub + wr * 64 + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (ur < u1) out[(size_t)(ur - u0) * g.I + ic] = acc[a][b][r] + bias;   // same order as BPRMF.py:85: Bi + (...)
      }
  }
}

// bprx_score_new_block: out[u][j] = <Tu[u], P[j, 0:d]> + P[j, d] for the n rows of a caller's P (items outside the catalogue: no
// Gi, no Bi).  The Tu x P phase of k_score_gemm on its own, same tiles, same C/D map; any d >= 1 (gemm_phase pads k with zeros).
__global__ __launch_bounds__(256) void k_score_new_gemm(const float *__restrict__ Tu, const float *__restrict__ P, int n, int d,
                                                        int PS, int u0, int u1, float *__restrict__ out) {
  __shared__ float As[TM][GLD];
  __shared__ float Bs[TN][GLD];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, wr = w >> 1, wc = w & 1;
  const int i0 = blockIdx.x * TN, ub = u0 + blockIdx.y * TM;
  const int arows = min(TM, u1 - ub), brows = min(TN, n - i0);
  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
  gemm_phase(Tu, d, ub, arows, P, PS, i0, brows, d, As, Bs, acc, wr, wc, lane);
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const int ic = i0 + wc * 64 + b * 32 + (lane & 31);
    if (ic >= n) continue;
    const float bias = P[(size_t)ic * PS + d];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ur = ub + wr * 64 + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (ur < u1) out[(size_t)(ur - u0) * n + ic] = acc[a][b][r] + bias;
      }
  }
}

// bprx_audience_block: k_score_gemm (g.Gi != nullptr) / k_score_new_gemm (g.Gi == nullptr: g.P holds the caller's rows) with the
// operand roles swapped: out[q - q0][u] for the item rows q in [q0, q1) against every user.  A holds the item rows (Gi, then P),
// B the user rows (Gu, then Tu); same tiles, same phase order, same C/D map, so an output row is an item, its bias Bi_q + P_q[d]
// is constant along it and the 32 lanes of a half-wave write 32 consecutive users.  Products are exact fp32 and the sums k-ordered
// from +0: for even k and d the element has the bits of the user-major kernels' out[u][q]; any k, d >= 1 (gemm_phase pads with
// zeros).  An element depends on its item row and its user row only.
__global__ __launch_bounds__(256) void k_audience_gemm(GemmArgs g, int q0, int q1, float *__restrict__ out) {
  __shared__ float As[TM][GLD];
  __shared__ float Bs[TN][GLD];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, wr = w >> 1, wc = w & 1;
  const int ub = blockIdx.x * TN, qb = q0 + blockIdx.y * TM;
  const int arows = min(TM, q1 - qb), brows = min(TN, g.U - ub);
  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
  if (g.Gi) gemm_phase(g.Gi, g.k, qb, arows, g.Gu, g.k, ub, brows, g.k, As, Bs, acc, wr, wc, lane);
  if (g.d) gemm_phase(g.P, g.PS, qb, arows, g.Tu, g.d, ub, brows, g.d, As, Bs, acc, wr, wc, lane);
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int qr = qb + wr * 64 + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      if (qr >= q1) continue;
      const float pb = g.d ? g.P[(size_t)qr * g.PS + g.d] : 0.f;
      const float bias = g.Gi ? g.Bi[qr] + pb : pb;            // as k_score_gemm / k_score_new_gemm form it
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const int uc = ub + wc * 64 + b * 32 + (lane & 31);
        if (uc < g.U) out[(size_t)(qr - q0) * g.U + uc] = acc[a][b][r] + bias;
      }
    }
}

// ---- similar items (include/bprx.h): cosine of item vectors z = [Gi | P[0:d]] (either part may be absent) ----
// (SimPart, one part of z: bprx_internal.h)
constexpr int RN_LANES = 16;   // lanes per row of k_sim_rnorm: 4 rows per wave, 16 per workgroup

// rn[r] = 1 / sqrt(sum_x z_rx^2), 0 for a zero row.  16 lanes load 16 consecutive x of a row (one 64-byte segment) and square
// them; every lane of the group then adds the 16 squares in ascending x (read by lane index), so the fp32 sum is the serial
// ascending-x sum of the row: s = (..((z_0^2 + z_1^2) + z_2^2)..), each product and each sum rounded once (no fma).  Columns
// past the width add +0.  No atomics; the loop bounds are the same for every lane (rows past n are clamped and not written).
__global__ __launch_bounds__(256) void k_sim_rnorm(SimPart a, SimPart b, int n, float *__restrict__ rn) {
  const int lane = threadIdx.x & 63, l = lane & (RN_LANES - 1), g0 = lane & ~(RN_LANES - 1);
  const int64_t row = (int64_t)blockIdx.x * (256 / RN_LANES) + (threadIdx.x / RN_LANES);
  const size_t rr = (size_t)(row < n ? row : n - 1);
  float s = 0.f;
#pragma unroll
  for (int part = 0; part < 2; ++part) {
    const SimPart z = part ? b : a;
    for (int c0 = 0; c0 < z.w; c0 += RN_LANES) {
      const int x = c0 + l;
      const float v = x < z.w ? z.p[rr * z.ld + x] : 0.f;
      const float sq = __fmul_rn(v, v);
#pragma unroll
      for (int j = 0; j < RN_LANES; ++j) s = __fadd_rn(s, __shfl(sq, g0 + j));
    }
  }
  if (row < n && l == 0) rn[row] = s > 0.f ? 1.f / sqrtf(s) : 0.f;
}

// out[q - q0][j] = <z_q, z_j> (rn_q[q] rn_items[j]) for the queries q in [q0, q1) against every catalogue item j: the tiles, the
// phases and the C/D map of k_score_gemm, one gemm_phase per part of z (any width >= 1: gemm_phase pads with zeros).  A holds
// the query rows (the catalogue's own tables, or the caller's projected rows), B the catalogue.  Products are exact fp32 and the
// sums k-ordered from +0, so <z_q, z_j> has the bits of <z_j, z_q>, and an element depends on its two rows and its two norms only.
__global__ __launch_bounds__(256) void k_sim_gemm(SimPart a0, SimPart a1, SimPart b0, SimPart b1, int I, int q0, int q1,
                                                  const float *__restrict__ rn_q, const float *__restrict__ rn_items,
                                                  float *__restrict__ out) {
  __shared__ float As[TM][GLD];
  __shared__ float Bs[TN][GLD];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, wr = w >> 1, wc = w & 1;
  const int i0 = blockIdx.x * TN, qb = q0 + blockIdx.y * TM;
  const int arows = min(TM, q1 - qb), brows = min(TN, I - i0);
  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
  if (a0.w) gemm_phase(a0.p, a0.ld, qb, arows, b0.p, b0.ld, i0, brows, a0.w, As, Bs, acc, wr, wc, lane);
  if (a1.w) gemm_phase(a1.p, a1.ld, qb, arows, b1.p, b1.ld, i0, brows, a1.w, As, Bs, acc, wr, wc, lane);
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const int ic = i0 + wc * 64 + b * 32 + (lane & 31);
    if (ic >= I) continue;
    const float rj = rn_items[ic];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int qr = qb + wr * 64 + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (qr < q1) out[(size_t)(qr - q0) * I + ic] = __fmul_rn(acc[a][b][r], __fmul_rn(rn_q[qr], rj));   // norms first: symmetric
      }
  }
}

constexpr int EVMAX = 32;   // held-out items per user handled on the device (the reference's split holds out 1)

// One workgroup per user.  out[5] = hr, prec, rec, auc, ndcg (double); out[0] = -1 marks "no held-out items"
// (Evaluator.py:88-89: such users are skipped), out[0] = -2 marks "too many held-out items for the device path".
__global__ __launch_bounds__(256) void k_eval_users(const float *__restrict__ S, int u0, int I,
                                                    const int64_t *__restrict__ tr_ptr, const int32_t *__restrict__ tr_items,
                                                    const int64_t *__restrict__ ev_ptr, const int32_t *__restrict__ ev_items,
                                                    int K, double *__restrict__ out, int32_t *__restrict__ errflag) {
  __shared__ float sp[EVMAX];
  __shared__ int ev[EVMAX];
  __shared__ int cnt_all[EVMAX], cnt_sub[EVMAX];
  __shared__ int n_tr_only;
  const int u = u0 + blockIdx.x, tid = threadIdx.x;
  const float *s = S + (size_t)blockIdx.x * I;
  double *o = out + (size_t)blockIdx.x * 5;
  const int64_t e0 = ev_ptr[u];
  const int nev = (int)(ev_ptr[u + 1] - e0);
  if (nev <= 0 || nev > EVMAX) {
    if (tid < 5) o[tid] = tid == 0 ? (nev <= 0 ? -1.0 : -2.0) : 0.0;
    return;
  }
  if (tid < nev) {
    int it = ev_items[e0 + tid];
    if ((unsigned)it >= (unsigned)I) { *errflag = 5; it = 0; }      // reported by bprx_sync_check, never dereferenced
    ev[tid] = it;
    sp[tid] = s[it];
    cnt_all[tid] = 0;
    cnt_sub[tid] = 0;
  }
  if (tid == 0) n_tr_only = 0;
  __syncthreads();
  // #(all items with score >= sp_t): one sweep of the score row per held-out item (the row is L2-resident)
  for (int t = 0; t < nev; ++t) {
    const float spt = sp[t];
    int loc = 0;
    for (int i = tid; i < I; i += 256) loc += s[i] >= spt ? 1 : 0;
    if (loc) atomicAdd(&cnt_all[t], loc);
  }
  // minus the train items that are not held-out items, minus the held-out items themselves
  const int64_t t0 = tr_ptr[u];
  const int ntr = (int)(tr_ptr[u + 1] - t0);
  for (int q = tid; q < ntr; q += 256) {
    const int it = tr_items[t0 + q];
    bool is_ev = false;
    for (int t = 0; t < nev; ++t) is_ev |= ev[t] == it;
    if (is_ev || (unsigned)it >= (unsigned)I) continue;
    atomicAdd(&n_tr_only, 1);
    const float v = s[it];
    for (int t = 0; t < nev; ++t)
      if (v >= sp[t]) atomicAdd(&cnt_sub[t], 1);
  }
  __syncthreads();
  if (tid == 0) {
    long long position = 0;
    int hits = 0;
    const long long nneg = (long long)I - n_tr_only - nev;
    const long long topn = (long long)K < nneg + nev ? (long long)K : nneg + nev;
    for (int t = 0; t < nev; ++t) {
      int ge_ev = 0, before = 0;                         // held-out items with score >= sp_t; those ranked before t
      for (int q = 0; q < nev; ++q) {
        if (sp[q] >= sp[t]) ++ge_ev;
        if (q != t && (sp[q] > sp[t] || (sp[q] == sp[t] && q < t))) ++before;
      }
      const long long neg_ge = (long long)cnt_all[t] - cnt_sub[t] - ge_ev;   // Evaluator.py:96-98
      position += neg_ge;
      if (neg_ge + before < topn) ++hits;                                    // heapq.nlargest membership, :104-115
    }
    o[0] = hits > 0 ? 1.0 : 0.0;                                             // :117
    o[1] = topn > 0 ? (double)hits / (double)topn : 0.0;                     // :123
    o[2] = (double)hits / (double)nev;                                       // :126
    o[3] = 1.0 - (double)position / ((double)nneg * (double)nev);            // :100
    o[4] = position < K ? log(2.0) / log((double)position + 2.0) : 0.0;      // :120
  }
}

// ------------------------------------------------------------------------------------------------------------
// The same metrics for an ITEM-SHARDED model (every rank holds the score columns of its own items): everything
// k_eval_users counts is additive over item shards once the held-out items' scores are known everywhere.
//   k_eval_pos     sp[user][t] = score of held-out item t where this rank owns it, 0 elsewhere   -> all-reduce(sum): exact
//   k_eval_counts  per user, over the rank's own columns: #(items >= sp_t), #(train-only items >= sp_t), #(train-only items)
//                                                                                                 -> all-reduce(sum)
//   k_eval_finish  the reference's formulas (Evaluator.py:96-126) from the summed counts: identical to k_eval_users on the
//                  concatenated score row, bit for bit.
// ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_eval_pos(const float *__restrict__ S, int u0, int nb, int Iloc, int item_lo, int Itot,
                                                  const int64_t *__restrict__ ev_ptr, const int32_t *__restrict__ ev_items,
                                                  float *__restrict__ sp, int32_t *__restrict__ errflag) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)nb * EVMAX) return;
  const int r = (int)(e / EVMAX), t = (int)(e % EVMAX);
  const int64_t e0 = ev_ptr[u0 + r];
  const int nev = (int)(ev_ptr[u0 + r + 1] - e0);
  float v = 0.f;
  if (t < nev && nev <= EVMAX) {
    int it = ev_items[e0 + t];
    if ((unsigned)it >= (unsigned)Itot) { *errflag = 5; it = 0; }
    const int li = it - item_lo;
    if ((unsigned)li < (unsigned)Iloc) v = S[(size_t)r * Iloc + li];
  }
  sp[e] = v;
}

__global__ __launch_bounds__(256) void k_eval_counts(const float *__restrict__ S, int u0, int Iloc, int item_lo, int Itot,
                                                     const int64_t *__restrict__ tr_ptr, const int32_t *__restrict__ tr_items,
                                                     const int64_t *__restrict__ ev_ptr, const int32_t *__restrict__ ev_items,
                                                     const float *__restrict__ spg, int32_t *__restrict__ counts) {
  __shared__ float sp[EVMAX];
  __shared__ int ev[EVMAX];
  __shared__ int cnt_all[EVMAX], cnt_sub[EVMAX];
  __shared__ int n_tr_only;
  const int u = u0 + blockIdx.x, tid = threadIdx.x;
  const float *s = S + (size_t)blockIdx.x * Iloc;
  int32_t *o = counts + (size_t)blockIdx.x * (2 * EVMAX + 1);
  const int64_t e0 = ev_ptr[u];
  const int nev = (int)(ev_ptr[u + 1] - e0);
  if (nev <= 0 || nev > EVMAX) {
    for (int q = tid; q < 2 * EVMAX + 1; q += 256) o[q] = 0;
    return;
  }
  if (tid < EVMAX) { cnt_all[tid] = 0; cnt_sub[tid] = 0; }
  if (tid < nev) {
    int it = ev_items[e0 + tid];
    if ((unsigned)it >= (unsigned)Itot) it = 0;                    // (reported by k_eval_pos)
    ev[tid] = it;
    sp[tid] = spg[(size_t)blockIdx.x * EVMAX + tid];
  }
  if (tid == 0) n_tr_only = 0;
  __syncthreads();
  for (int t = 0; t < nev; ++t) {
    const float spt = sp[t];
    int loc = 0;
    for (int i = tid; i < Iloc; i += 256) loc += s[i] >= spt ? 1 : 0;
    if (loc) atomicAdd(&cnt_all[t], loc);
  }
  const int64_t t0 = tr_ptr[u];
  const int ntr = (int)(tr_ptr[u + 1] - t0);
  for (int q = tid; q < ntr; q += 256) {
    const int it = tr_items[t0 + q];
    const int li = it - item_lo;
    if ((unsigned)li >= (unsigned)Iloc) continue;                  // another rank's column (or out of range: nobody's)
    bool is_ev = false;
    for (int t = 0; t < nev; ++t) is_ev |= ev[t] == it;
    if (is_ev) continue;
    atomicAdd(&n_tr_only, 1);
    const float v = s[li];
    for (int t = 0; t < nev; ++t)
      if (v >= sp[t]) atomicAdd(&cnt_sub[t], 1);
  }
  __syncthreads();
  if (tid < EVMAX) { o[tid] = tid < nev ? cnt_all[tid] : 0; o[EVMAX + tid] = tid < nev ? cnt_sub[tid] : 0; }
  if (tid == 0) o[2 * EVMAX] = n_tr_only;
}

__global__ __launch_bounds__(256) void k_eval_finish(int u0, int nb, int Itot, const int64_t *__restrict__ ev_ptr,
                                                     const float *__restrict__ spg, const int32_t *__restrict__ counts, int K,
                                                     double *__restrict__ out) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= nb) return;
  double *o = out + (size_t)r * 5;
  const int nev = (int)(ev_ptr[u0 + r + 1] - ev_ptr[u0 + r]);
  if (nev <= 0 || nev > EVMAX) {
    o[0] = nev <= 0 ? -1.0 : -2.0; o[1] = o[2] = o[3] = o[4] = 0.0;
    return;
  }
  const float *sp = spg + (size_t)r * EVMAX;
  const int32_t *c = counts + (size_t)r * (2 * EVMAX + 1);
  long long position = 0;
  int hits = 0;
  const long long nneg = (long long)Itot - c[2 * EVMAX] - nev;
  const long long topn = (long long)K < nneg + nev ? (long long)K : nneg + nev;
  for (int t = 0; t < nev; ++t) {
    int ge_ev = 0, before = 0;
    for (int q = 0; q < nev; ++q) {
      if (sp[q] >= sp[t]) ++ge_ev;
      if (q != t && (sp[q] > sp[t] || (sp[q] == sp[t] && q < t))) ++before;
    }
    const long long neg_ge = (long long)c[t] - c[EVMAX + t] - ge_ev;             // Evaluator.py:96-98
    position += neg_ge;
    if (neg_ge + before < topn) ++hits;                                          // heapq.nlargest membership, :104-115
  }
  o[0] = hits > 0 ? 1.0 : 0.0;
  o[1] = topn > 0 ? (double)hits / (double)topn : 0.0;
  o[2] = (double)hits / (double)nev;
  o[3] = 1.0 - (double)position / ((double)nneg * (double)nev);
  o[4] = position < K ? log(2.0) / log((double)position + 2.0) : 0.0;
}

// ------------------------------------------------------------------------------------------------------------
// Evaluator.store_recommendation on the device (Evaluator.py:225-239): per user, the train items are masked with -inf
// IN the score row (as the reference does: results[u][training_list[u]] = -np.inf) and the K largest scores are
// selected.  One workgroup per user: radix select of the K-th largest key over the row (four 8-bit histogram passes on
// the order-preserving integer image of the fp32 scores; the row is L2-resident), one collection pass, and a bitonic
// sort of the K candidates by (score descending, item ascending).
// The reference orders equal scores by numpy's unstable argsort (implementation- and CPU-dependent); rows whose output
// depends on such a tie -- equal scores among the K selected, or at the selection boundary, or fewer than K unmasked
// items -- are FLAGGED (flag[row] = 1) so that the caller can redo exactly those rows with numpy on the (masked) row.
// "Equal" is float equality, as numpy compares: +0.0 and -0.0 are one score (f2key gives them one key) although their
// bits differ; val_out is read from the row, so the sign of a zero is kept.  NaN scores are outside the contract.
// ------------------------------------------------------------------------------------------------------------
constexpr int TOPK_MAX = 1024;

__device__ __forceinline__ uint32_t f2key(float x) {       // larger float <-> larger key; -inf is the smallest finite-order key
  uint32_t u = __float_as_uint(x);
  if (u == 0x80000000u) u = 0u;                            // -0.0 == +0.0: one key, so a +-0 pair meets the tie checks below
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(256) void k_topk(float *__restrict__ S, int u0, int I, const int64_t *__restrict__ tr_ptr,
                                              const int32_t *__restrict__ tr_items, int K, int32_t *__restrict__ idx_out,
                                              float *__restrict__ val_out, int32_t *__restrict__ flag_out) {
  __shared__ int hist[256];
  __shared__ uint32_t s_prefix, s_mask;
  __shared__ int s_remaining, s_ngt, s_neq, s_bad;
  __shared__ uint32_t ckey[TOPK_MAX];
  __shared__ int cidx[TOPK_MAX];
  const int u = u0 + blockIdx.x, tid = threadIdx.x;
  float *s = S + (size_t)blockIdx.x * I;
  const int64_t t0 = tr_ptr ? tr_ptr[u] : 0;               // (tr_ptr == nullptr, bprx_topk_rows: nothing is masked)
  const int ntr = tr_ptr ? (int)(tr_ptr[u + 1] - t0) : 0;
  for (int q = tid; q < ntr; q += 256) {
    const int it = tr_items[t0 + q];
    if ((unsigned)it < (unsigned)I) s[it] = -INFINITY;
  }
  const int Kc = K < I ? K : I;                            // argsort()[-k:] returns min(k, I) entries
  if (tid == 0) { s_prefix = 0; s_mask = 0; s_remaining = Kc; s_ngt = 0; s_neq = 0; s_bad = K > I ? 1 : 0; }
  __syncthreads();
  for (int pass = 3; pass >= 0; --pass) {
    hist[tid] = 0;
    __syncthreads();
    const uint32_t prefix = s_prefix, mask = s_mask;
    for (int i = tid; i < I; i += 256) {
      const uint32_t key = f2key(s[i]);
      if ((key & mask) == prefix) atomicAdd(&hist[(key >> (8 * pass)) & 255], 1);
    }
    __syncthreads();
    if (tid == 0) {
      int rem = s_remaining, b = 255;
      for (; b > 0; --b) {                                  // from the largest byte value down
        if (hist[b] >= rem) break;
        rem -= hist[b];
      }
      s_remaining = rem;                                    // still wanted among the elements whose byte == b
      s_prefix = prefix | ((uint32_t)b << (8 * pass));
      s_mask = mask | (255u << (8 * pass));
    }
    __syncthreads();
  }
  const uint32_t kth = s_prefix;                            // key of the K-th largest score; `want_eq` of the elements equal to
  const int want_eq = s_remaining;                          // it belong to the list, all Kc - want_eq larger ones do
  for (int i = tid; i < I; i += 256) {
    const uint32_t key = f2key(s[i]);
    if (key > kth) {
      const int p = atomicAdd(&s_ngt, 1);
      ckey[p] = key; cidx[p] = i;
    } else if (key == kth) {
      const int e = atomicAdd(&s_neq, 1);                   // more than want_eq of them: a tie straddles the boundary (flagged)
      if (e < want_eq) { ckey[Kc - want_eq + e] = key; cidx[Kc - want_eq + e] = i; }
    }
  }
  __syncthreads();
  if (tid == 0 && (s_neq != want_eq || kth == f2key(-INFINITY))) s_bad = 1;   // boundary tie / masked items reach the list
  __syncthreads();
  // bitonic sort of the Kc candidates by (key descending, item ascending), padded to a power of two with minimal keys
  int n2 = 1;
  while (n2 < Kc) n2 <<= 1;
  for (int q = Kc + tid; q < n2; q += 256) { ckey[q] = 0u; cidx[q] = 0x7fffffff; }
  __syncthreads();
  for (int size = 2; size <= n2; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int q = tid; q < n2; q += 256) {
        const int partner = q ^ stride;
        if (partner > q) {
          const bool desc = (q & size) == 0;                // first half of each `size` block sorted "better first"
          const uint32_t ka = ckey[q], kb = ckey[partner];
          const int ia = cidx[q], ib = cidx[partner];
          const bool a_better = ka > kb || (ka == kb && ia < ib);
          if (a_better != desc) { ckey[q] = kb; ckey[partner] = ka; cidx[q] = ib; cidx[partner] = ia; }
        }
      }
      __syncthreads();
    }
  }
  for (int q = tid; q < Kc; q += 256) {
    if (q + 1 < Kc && ckey[q] == ckey[q + 1]) s_bad = 1;    // equal scores inside the list: numpy's order is unspecified
    idx_out[(size_t)blockIdx.x * K + q] = cidx[q];
    val_out[(size_t)blockIdx.x * K + q] = s[cidx[q]];
  }
  for (int q = Kc + tid; q < K; q += 256) { idx_out[(size_t)blockIdx.x * K + q] = -1; val_out[(size_t)blockIdx.x * K + q] = 0.f; }
  __syncthreads();
  if (tid == 0) flag_out[blockIdx.x] = s_bad;
}

// ------------------------------------------------------------------------------------------------------------
// bprx_topk_classes (include/bprx.h): the K best entries of every CLASS of a score row.  The row's I elements fall into C
// independent selections, read through the class CSR (s[class_items[p]]: the ids ascend inside a class, so the addresses move
// forward through the L2-resident row).  A list has a total order of its own -- (score descending as floats, item ascending),
// at the selection boundary too -- so nothing is flagged; entries that are -inf in the (masked) row are on no list.
//   k_mask_rows      row r gets -inf at the ids of list row0 + r: a launch of its own in front, so a row's mask is complete before
//                    any class of the row is read
//   k_topk_classes   one workgroup per (row, tile of TKC_TILE = 4 consecutive classes); by class size n:
//                      n <= TKC_WAVE_MAX   one wave sorts the whole class in its quarter of the candidate buffer (wave w takes
//                                          class 4g + w; the bitonic stages of the four waves run in step, to the largest of them)
//                      larger              the workgroup: k_topk's radix select over the gathered keys, STOPPED after the first
//                                          histogram pass at which the elements at or above the selected bin fit the candidate
//                                          buffer (for real-valued scores the first: the K-th best shares its sign and exponent
//                                          byte with a few per cent of a class); those are collected and sorted whole, which
//                                          settles every tie by the sort's own order.  Only when four passes leave more than
//                                          TOPK_MAX such elements (that many EQUAL scores) the select ends as k_topk's does: one
//                                          collection pass, and a second select over the item ids of exactly the tied elements.
//                    Classes are skewed: a tile of small classes costs one workgroup, not four.  The histogram's bin is picked
//                    by a wave scan, not a serial walk.  Split point and pass counts: DESIGN 9.
// No float arithmetic, no float atomics, no scratch; LDS 9.3 KB per workgroup.
// ------------------------------------------------------------------------------------------------------------
#ifndef BPRX_TKC_WAVE_MAX
#define BPRX_TKC_WAVE_MAX 256
#endif
constexpr int TKC_TILE = 4, TKC_WAVE_MAX = BPRX_TKC_WAVE_MAX;
static_assert(TKC_WAVE_MAX * TKC_TILE <= TOPK_MAX && (TKC_WAVE_MAX & (TKC_WAVE_MAX - 1)) == 0, "a wave's quarter of the buffer");
constexpr uint32_t KEY_NINF = 0x007fffffu;                 // f2key(-inf): a candidate's key is larger
constexpr int PAD_ITEM = 0x7fffffff;                       // (key 0, PAD_ITEM): sorts behind every candidate

struct TkcShared {
  int hist[256];
  uint32_t prefix, mask;
  int remaining, kc, ngt, neq, cand;                       // cand: the elements at or above the selected bin, so far
  uint32_t ckey[TOPK_MAX];
  int cidx[TOPK_MAX];
};

// Workgroup b of a launch of `total` workgroups, laid out by tkc_grid: a launch takes fewer than 2^32 threads along x, and nrows * C
// may reach 2^31, so the count is folded into (x, y); the workgroups past `total` in the last row of the grid leave at once.
constexpr int64_t TKC_GRID_X = (int64_t)1 << 22;
__device__ __forceinline__ int64_t tkc_block() { return (int64_t)blockIdx.y * gridDim.x + blockIdx.x; }

__global__ __launch_bounds__(256) void k_mask_rows(float *__restrict__ S, int64_t nrows, int64_t row0, int width,
                                                   const int64_t *__restrict__ ptr, const int32_t *__restrict__ items) {
  const int64_t row = tkc_block();
  if (row >= nrows) return;
  float *s = S + (size_t)row * width;
  const int64_t t0 = ptr[row0 + row], t1 = ptr[row0 + row + 1];
  for (int64_t q = t0 + threadIdx.x; q < t1; q += 256) {
    const int it = items[q];
    if ((unsigned)it < (unsigned)width) s[it] = -INFINITY;
  }
}

// The sort key of class entry `it`, false for an entry that is on no list (an id outside the row: reported; a score of -inf).
// TIE: only the entries whose score key is kth take part, and their key is the item id, smaller id = larger key.
template <bool TIE>
__device__ __forceinline__ bool tkc_elem(const float *__restrict__ s, int width, int it, uint32_t kth, uint32_t &key,
                                         int32_t *__restrict__ errflag) {
  if ((unsigned)it >= (unsigned)width) { *errflag = 5; return false; }   // reported by bprx_sync_check, never dereferenced
  const uint32_t k = f2key(s[it]);
  if (TIE) { key = ~(uint32_t)it; return k == kth; }
  key = k;
  return k > KEY_NINF;
}

// Wave 0, after a histogram pass: the bin (from the largest down) in which the `remaining`-th largest key lies, by a wave scan
// over 4 bins per lane.  first_k > 0 (the first pass of a selection over all candidates): remaining = kc = min(first_k, number of
// candidates) first.
__device__ __forceinline__ void tkc_pick(TkcShared &sh, int pass, int first_k) {
  const int lane = threadIdx.x;
  int c[4], local = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) { c[j] = sh.hist[255 - (4 * lane + j)]; local += c[j]; }
  int incl = local;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int t = __shfl_up(incl, off);
    if (lane >= off) incl += t;
  }
  const int total = __shfl(incl, 63);
  int rem = sh.remaining;
  if (first_k > 0) {
    rem = first_k < total ? first_k : total;
    if (lane == 0) { sh.kc = rem; sh.remaining = rem; }
  }
  if (rem <= 0 || rem > total) return;                       // (nothing wanted; rem > total cannot happen: prefix stays)
  const int excl = incl - local;
  if (excl < rem && rem <= incl) {                           // exactly one lane
    int r = rem - excl, b = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (c[j] >= r) { b = 255 - (4 * lane + j); break; }
      r -= c[j];
    }
    sh.remaining = r;                                        // still wanted among the elements whose byte == b
    sh.cand = (first_k > 0 ? rem : sh.kc) - r + sh.hist[b];  // all kc - r above the bin are on the list, the bin's may be
    sh.prefix |= (uint32_t)b << (8 * pass);
    sh.mask |= 255u << (8 * pass);
  }
}

// k_topk's radix select over the keys of tkc_elem<TIE>: afterwards sh.prefix is the key of the wanted-th largest and sh.remaining
// how many of the elements equal to it are wanted.  The caller has set prefix = mask = 0 (and remaining, unless first_k > 0).
template <bool TIE>
__device__ void tkc_select(TkcShared &sh, const float *__restrict__ s, int width, const int32_t *__restrict__ items, int n,
                           int first_k, uint32_t kth, int32_t *__restrict__ errflag) {
  const int tid = threadIdx.x;
  for (int pass = 3; pass >= 0; --pass) {
    sh.hist[tid] = 0;
    __syncthreads();
    const uint32_t prefix = sh.prefix, mask = sh.mask;
    for (int q = tid; q < n; q += 256) {
      uint32_t key;
      if (tkc_elem<TIE>(s, width, items[q], kth, key, errflag) && (key & mask) == prefix)
        atomicAdd(&sh.hist[(key >> (8 * pass)) & 255], 1);
    }
    __syncthreads();
    if (tid < 64) tkc_pick(sh, pass, pass == 3 ? first_k : 0);
    __syncthreads();
    if (pass == 3 && first_k > 0 && sh.kc == 0) return;      // no candidate (the same for every thread)
    if (!TIE && sh.cand <= TOPK_MAX) return;                 // what is left fits the buffer: the caller sorts it
  }
}

// The elements above the selected key go to slots base .. base + ngt_cap - 1, the first want_eq that equal it (in arrival order)
// behind them (tkc_select ran all four passes); sh.ngt / sh.neq count what was seen.  Slots hold the SCORE key (TIE: score_kth for all) and the item.
template <bool TIE>
__device__ void tkc_collect(TkcShared &sh, const float *__restrict__ s, int width, const int32_t *__restrict__ items, int n,
                            uint32_t score_kth, uint32_t kth, int base, int ngt_cap, int want_eq, int32_t *__restrict__ errflag) {
  for (int q = threadIdx.x; q < n; q += 256) {
    const int it = items[q];
    uint32_t key;
    if (!tkc_elem<TIE>(s, width, it, score_kth, key, errflag)) continue;
    if (key > kth) {
      const int p = atomicAdd(&sh.ngt, 1);
      if (p < ngt_cap) { sh.ckey[base + p] = TIE ? score_kth : key; sh.cidx[base + p] = it; }
    } else if (key == kth) {
      const int e = atomicAdd(&sh.neq, 1);
      if (e < want_eq) { sh.ckey[base + ngt_cap + e] = TIE ? score_kth : key; sh.cidx[base + ngt_cap + e] = it; }
    }
  }
}

// Bitonic sort of n2 (a power of two) slots by (key descending, item ascending), `nt` threads of which this one is `t`; every thread
// of the workgroup calls it with the same n2 (each stage ends in a barrier).
__device__ __forceinline__ void tkc_sort(uint32_t *ckey, int *cidx, int n2, int t, int nt) {
  for (int size = 2; size <= n2; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int q = t; q < n2; q += nt) {
        const int partner = q ^ stride;
        if (partner > q) {
          const bool desc = (q & size) == 0;
          const uint32_t ka = ckey[q], kb = ckey[partner];
          const int ia = cidx[q], ib = cidx[partner];
          const bool a_better = ka > kb || (ka == kb && ia < ib);
          if (a_better != desc) { ckey[q] = kb; ckey[partner] = ka; cidx[q] = ib; cidx[partner] = ia; }
        }
      }
      __syncthreads();
    }
  }
}

// Slots [0, n2) of a buffer <- the candidates of a whole class, padded; returns how many of this thread's entries are candidates.
__device__ __forceinline__ int tkc_load(uint32_t *ckey, int *cidx, const float *__restrict__ s, int width,
                                        const int32_t *__restrict__ items, int n, int n2, int t, int nt, int32_t *__restrict__ errflag) {
  int m = 0;
  for (int q = t; q < n2; q += nt) {
    uint32_t key = 0u;
    int it = PAD_ITEM;
    if (q < n) {
      it = items[q];
      if (tkc_elem<false>(s, width, it, 0u, key, errflag)) ++m;
      else { key = 0u; it = PAD_ITEM; }
    }
    ckey[q] = key; cidx[q] = it;
  }
  return m;
}

__device__ __forceinline__ void tkc_write(const int *cidx, const float *__restrict__ s, int width, int kc, int K, int t, int nt,
                                          int32_t *__restrict__ idx, float *__restrict__ val, int32_t *__restrict__ cnt) {
  for (int q = t; q < K; q += nt) {
    const int it = q < kc ? cidx[q] : -1;
    const bool on = (unsigned)it < (unsigned)width;          // (every candidate's id lies in the row)
    idx[q] = on ? it : -1;
    val[q] = on ? s[it] : 0.f;                               // read from the row: the sign of a zero is kept
  }
  if (t == 0) *cnt = kc;
}

__device__ __forceinline__ int tkc_pow2(int n) {
  int n2 = 1;
  while (n2 < n) n2 <<= 1;
  return n2;
}

__global__ __launch_bounds__(256) void k_topk_classes(const float *__restrict__ S, int width, const int64_t *__restrict__ cptr,
                                                      const int32_t *__restrict__ citems, int C, int tiles, int64_t total, int K,
                                                      int32_t *__restrict__ idx_out, float *__restrict__ val_out,
                                                      int32_t *__restrict__ cnt_out, int32_t *__restrict__ errflag) {
  __shared__ TkcShared sh;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t blk = tkc_block();
  if (blk >= total) return;                                  // (the whole workgroup: no barrier is left waiting)
  const int64_t row = blk / tiles;
  const int c0 = (int)(blk % tiles) * TKC_TILE;
  const float *s = S + (size_t)row * width;
  // (start, length) of class c; length -1: no such class.  A class holds at most `width` items.
  auto class_of = [&](int c, int64_t &p) -> int {
    if (c >= C) { p = 0; return -1; }
    p = cptr[c];
    const int64_t len = cptr[c + 1] - p;
    return len < 0 ? 0 : len > 0x7fffffff ? 0x7fffffff : (int)len;
  };
  int wave_n2 = 0;                                           // the bitonic width of the tile's wave-sorted classes
#pragma unroll
  for (int j = 0; j < TKC_TILE; ++j) {
    int64_t p;
    const int nj = class_of(c0 + j, p);
    if (nj >= 0 && nj <= TKC_WAVE_MAX) wave_n2 = max(wave_n2, tkc_pow2(nj));
  }
  // ---- classes of at most TKC_WAVE_MAX items: wave w sorts class c0 + w whole ----
  if (wave_n2 > 0) {
    int64_t pw;
    const int nw = class_of(c0 + w, pw);
    const bool mine = nw >= 0 && nw <= TKC_WAVE_MAX;
    uint32_t *ck = sh.ckey + w * TKC_WAVE_MAX;
    int *ci = sh.cidx + w * TKC_WAVE_MAX;
    int m = tkc_load(ck, ci, s, width, citems + pw, mine ? nw : 0, wave_n2, lane, 64, errflag);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m += __shfl_xor(m, off);
    __syncthreads();
    tkc_sort(ck, ci, wave_n2, lane, 64);
    if (mine) {
      const size_t o = ((size_t)row * C + (c0 + w)) * K;
      tkc_write(ci, s, width, m < K ? m : K, K, lane, 64, idx_out + o, val_out + o, cnt_out + (size_t)row * C + (c0 + w));
    }
  }
  // ---- larger classes: the whole workgroup, one class after the other ----
#pragma unroll 1
  for (int j = 0; j < TKC_TILE; ++j) {
    int64_t pj;
    const int nj = class_of(c0 + j, pj);
    if (nj <= TKC_WAVE_MAX) continue;                        // (the same for every thread)
    const int32_t *items = citems + pj;
    const size_t o = ((size_t)row * C + (c0 + j)) * K;
    int32_t *cnt = cnt_out + (size_t)row * C + (c0 + j);
    __syncthreads();                                         // the buffer is free again
    if (tid == 0) { sh.prefix = 0; sh.mask = 0; sh.remaining = 0; sh.kc = 0; sh.ngt = 0; sh.neq = 0; sh.cand = 0x7fffffff; }
    tkc_select<false>(sh, s, width, items, nj, K, 0u, errflag);          // (its first barrier publishes the line above)
    const int kc = sh.kc;
    if (kc > 0 && sh.cand <= TOPK_MAX) {                     // everything at or above the selected bin, sorted whole
      const uint32_t prefix = sh.prefix, mask = sh.mask;
      for (int q = tid; q < nj; q += 256) {
        const int it = items[q];
        uint32_t key;
        if (tkc_elem<false>(s, width, it, 0u, key, errflag) && (key & mask) >= prefix) {
          const int p = atomicAdd(&sh.ngt, 1);
          if (p < TOPK_MAX) { sh.ckey[p] = key; sh.cidx[p] = it; }
        }
      }
      __syncthreads();
      const int got = sh.ngt < TOPK_MAX ? sh.ngt : TOPK_MAX; // (== sh.cand >= kc)
      const int n2 = tkc_pow2(got);
      for (int q = got + tid; q < n2; q += 256) { sh.ckey[q] = 0u; sh.cidx[q] = PAD_ITEM; }
      __syncthreads();
      tkc_sort(sh.ckey, sh.cidx, n2, tid, 256);
    } else if (kc > 0) {
      const uint32_t kth = sh.prefix;                        // key of the kc-th largest score; want_eq of the elements equal to
      const int want_eq = sh.remaining;                      // it belong to the list, all kc - want_eq larger ones do
      tkc_collect<false>(sh, s, width, items, nj, 0u, kth, 0, kc - want_eq, want_eq, errflag);
      __syncthreads();
      if (sh.neq > want_eq) {                                // a tie straddles the boundary: the want_eq smallest ids of it
        __syncthreads();
        if (tid == 0) { sh.prefix = 0; sh.mask = 0; sh.remaining = want_eq; sh.ngt = 0; sh.neq = 0; }
        tkc_select<true>(sh, s, width, items, nj, 0, kth, errflag);
        const uint32_t id_kth = sh.prefix;
        const int want_id = sh.remaining;
        tkc_collect<true>(sh, s, width, items, nj, kth, id_kth, kc - want_eq, want_eq - want_id, want_id, errflag);
        __syncthreads();
      }
      const int n2 = tkc_pow2(kc);
      for (int q = kc + tid; q < n2; q += 256) { sh.ckey[q] = 0u; sh.cidx[q] = PAD_ITEM; }
      __syncthreads();
      tkc_sort(sh.ckey, sh.cidx, n2, tid, 256);
    }
    tkc_write(sh.cidx, s, width, kc, K, tid, 256, idx_out + o, val_out + o, cnt);
  }
}

}  // namespace

// The shared tail of the three top-K entries, after each one's own argument checks: the K range, then `null` (the entry found a
// null pointer with rows to list: rejected only now, as each entry orders its checks), the gate, and one k_topk launch over
// nrows rows of `width` scores, row r masking the items of list row0 + r (ptr == nullptr: nothing).
static int topk_launch(bprx_handle *h, const char *what, const char *kernel, bool null, unsigned need, int kind, int64_t nrows,
                       float *scores, int row0, int width, const int64_t *ptr, const int32_t *items, int32_t K, int32_t *idx,
                       float *val, int32_t *flag, void *stream) {
  if (K <= 0 || K > TOPK_MAX) BPRX_FAIL(h, BPRX_E_INVALID, "%s: K=%d outside [1, %d]", what, K, TOPK_MAX);
  if (null) BPRX_FAIL(h, BPRX_E_INVALID, "%s: null pointer", what);
  const int rc = bprx_enter(h, what, need, kind, (hipStream_t)stream);
  if (rc || nrows == 0) return rc;
  hipLaunchKernelGGL(k_topk, dim3((unsigned)nrows), dim3(256), 0, (hipStream_t)stream, scores, row0, width, ptr, items, K, idx, val,
                     flag);
  BPRX_LAUNCH_CHECK(h, kernel);
  return BPRX_OK;
}

extern "C" int bprx_topk(bprx_handle *h, int32_t u0, int32_t u1, float *scores, const int64_t *train_ptr,
                         const int32_t *train_items, int32_t K, int32_t *idx, float *val, int32_t *flag, void *stream) {
  if (!h) return BPRX_E_INVALID;
  if (u0 < 0 || u1 > h->cfg.num_users || u0 > u1 || !scores || !train_ptr || !train_items || !idx || !val || !flag)
    BPRX_FAIL(h, BPRX_E_INVALID, "topk: bad argument");
  return topk_launch(h, "topk", "k_topk", false, 0, KIND_ANY, u1 - u0, scores, u0, h->cfg.num_items, train_ptr, train_items, K, idx,
                     val, flag, stream);
}

extern "C" int bprx_topk_rows(bprx_handle *h, int64_t nrows, int32_t width, float *scores, int32_t K, int32_t *idx, float *val,
                              int32_t *flag, void *stream) {
  if (!h) return BPRX_E_INVALID;
  if (nrows < 0 || nrows >= ((int64_t)1 << 31)) BPRX_FAIL(h, BPRX_E_INVALID, "topk_rows: n = %lld out of range", (long long)nrows);
  if (width < 1) BPRX_FAIL(h, BPRX_E_INVALID, "topk_rows: width = %d < 1", width);
  return topk_launch(h, "topk_rows", "k_topk<rows>", nrows && (!scores || !idx || !val || !flag), NEED_BOUND, KIND_VBPR_NO_FP8, nrows,
                     scores, 0, width, nullptr, nullptr, K, idx, val, flag, stream);
}

// bprx_topk for rows that are not users of the handle: row r masks the items of its own list
extern "C" int bprx_topk_lists(bprx_handle *h, int64_t nrows, float *scores, const int64_t *list_ptr, const int32_t *list_items,
                               int32_t K, int32_t *idx, float *val, int32_t *flag, void *stream) {
  if (!h) return BPRX_E_INVALID;
  if (nrows < 0 || nrows >= ((int64_t)1 << 31)) BPRX_FAIL(h, BPRX_E_INVALID, "topk_lists: nrows = %lld out of range", (long long)nrows);
  return topk_launch(h, "topk_lists", "k_topk<lists>", nrows && (!scores || !list_ptr || !list_items || !idx || !val || !flag), 0,
                     KIND_ANY, nrows, scores, 0, h->cfg.num_items, list_ptr, list_items, K, idx, val, flag, stream);
}

// bprx_topk_rows with bprx_topk_lists' per-row mask lists: rows of the caller's width (an audience block: num_users wide)
extern "C" int bprx_topk_rows_masked(bprx_handle *h, int64_t nrows, int32_t width, float *scores, const int64_t *list_ptr,
                                     const int32_t *list_items, int32_t K, int32_t *idx, float *val, int32_t *flag, void *stream) {
  if (!h) return BPRX_E_INVALID;
  if (nrows < 0 || nrows >= ((int64_t)1 << 31))
    BPRX_FAIL(h, BPRX_E_INVALID, "topk_rows_masked: nrows = %lld out of range", (long long)nrows);
  if (width < 1) BPRX_FAIL(h, BPRX_E_INVALID, "topk_rows_masked: width = %d < 1", width);
  return topk_launch(h, "topk_rows_masked", "k_topk<rows_masked>", nrows && (!scores || !list_ptr || !list_items || !idx || !val || !flag),
                     0, KIND_ANY, nrows, scores, 0, width, list_ptr, list_items, K, idx, val, flag, stream);
}

// ---- category shelves: the K best entries of every class of a row (include/bprx.h; k_mask_rows, k_topk_classes) ----
extern "C" int bprx_topk_classes(bprx_handle *h, int64_t nrows, int32_t width, float *scores, int64_t row0, const int64_t *list_ptr,
                                 const int32_t *list_items, const int64_t *class_ptr, const int32_t *class_items, int32_t C, int32_t K,
                                 int32_t *idx, float *val, int32_t *cnt, void *stream) {
  if (!h) return BPRX_E_INVALID;
  if (K <= 0 || K > TOPK_MAX) BPRX_FAIL(h, BPRX_E_INVALID, "topk_classes: K=%d outside [1, %d]", K, TOPK_MAX);
  if (C < 1) BPRX_FAIL(h, BPRX_E_INVALID, "topk_classes: C = %d < 1", C);
  if (width < 1) BPRX_FAIL(h, BPRX_E_INVALID, "topk_classes: width = %d < 1", width);
  if (nrows < 0 || row0 < 0) BPRX_FAIL(h, BPRX_E_INVALID, "topk_classes: nrows = %lld, row0 = %lld: neither is negative", (long long)nrows, (long long)row0);
  if (nrows >= ((int64_t)1 << 31) || nrows * C > (((int64_t)1 << 31) - 1) / K)
    BPRX_FAIL(h, BPRX_E_INVALID, "topk_classes: nrows * C * K = %lld * %d * %d does not stay below 2^31", (long long)nrows, C, K);
  if (nrows && (!scores || !class_ptr || !class_items || !idx || !val || !cnt || (list_ptr && !list_items)))
    BPRX_FAIL(h, BPRX_E_INVALID, "topk_classes: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const int rc = bprx_enter(h, "topk_classes", 0, KIND_ANY, s);
  if (rc || nrows == 0) return rc;
  auto grid = [](int64_t total) {                            // tkc_block's layout: x up to 2^22 workgroups, y the rest (at most 2^9)
    const int64_t x = total < TKC_GRID_X ? total : TKC_GRID_X;
    return dim3((unsigned)x, (unsigned)((total + x - 1) / x));
  };
  if (list_ptr) {                                            // a launch of its own: every class of a row reads the finished mask
    hipLaunchKernelGGL(k_mask_rows, grid(nrows), dim3(256), 0, s, scores, nrows, row0, width, list_ptr, list_items);
    BPRX_LAUNCH_CHECK(h, "k_mask_rows");
  }
  const int tiles = (C + TKC_TILE - 1) / TKC_TILE;
  const int64_t total = nrows * tiles;                       // < 2^31: nrows * C is
  hipLaunchKernelGGL(k_topk_classes, grid(total), dim3(256), 0, s, (const float *)scores, width, class_ptr, class_items, C, tiles,
                     total, K, idx, val, cnt, h->errflag);
  BPRX_LAUNCH_CHECK(h, "k_topk_classes");
  return BPRX_OK;
}

// ---- audience: the item-major score block (include/bprx.h) ----
extern "C" int bprx_audience_block(bprx_handle *h, const float *Pq, int64_t nq, int64_t q0, int64_t q1, float *out, void *stream) {
  if (!h) return BPRX_E_INVALID;
  if (!out) BPRX_FAIL(h, BPRX_E_INVALID, "audience_block: null pointer");
  if (nq < 0 || nq >= ((int64_t)1 << 31)) BPRX_FAIL(h, BPRX_E_INVALID, "audience_block: nq = %lld out of range", (long long)nq);
  if (!Pq && nq != h->cfg.num_items)
    BPRX_FAIL(h, BPRX_E_INVALID, "audience_block: nq = %lld, the catalogue has %d items", (long long)nq, h->cfg.num_items);
  if (q0 < 0 || q0 > q1 || q1 > nq || q1 - q0 > (int64_t)65535 * TM)
    BPRX_FAIL(h, BPRX_E_INVALID, "audience_block: bad item range [%lld,%lld) of %lld", (long long)q0, (long long)q1, (long long)nq);
  hipStream_t s = (hipStream_t)stream;
  // the catalogue: what bprx_score_block needs; the caller's rows: what bprx_score_new_block needs (NEED_ET: the image Pq was
  // made from stays the current one)
  const int rc = Pq ? bprx_enter(h, "audience_block", NEED_BOUND | NEED_ROWS | NEED_ET, KIND_VBPR_NO_FP8, s)
                    : bprx_enter(h, "audience_block", NEED_BOUND | NEED_ROWS | NEED_P_ALL, KIND_PLAIN, s);
  if (rc || q0 == q1) return rc;
  GemmArgs g;
  g.Gu = h->t.Gu; g.Gi = Pq ? nullptr : h->t.Gi; g.Bi = h->t.Bi; g.Tu = h->t.Tu; g.P = Pq ? Pq : h->P;
  g.U = h->cfg.num_users; g.I = (int)nq; g.k = h->cfg.embed_k; g.d = h->cfg.embed_d; g.PS = h->PS;
  dim3 grid((unsigned)((g.U + TN - 1) / TN), (unsigned)((q1 - q0 + TM - 1) / TM));
  hipLaunchKernelGGL(k_audience_gemm, grid, dim3(256), 0, s, g, (int)q0, (int)q1, out);
  BPRX_LAUNCH_CHECK(h, "k_audience_gemm");
  return BPRX_OK;
}

extern "C" int bprx_score_new_block(bprx_handle *h, int32_t u0, int32_t u1, const float *P, int64_t n, float *out, void *stream) {
  if (!h) return BPRX_E_INVALID;
  if (n < 0 || n >= ((int64_t)1 << 31)) BPRX_FAIL(h, BPRX_E_INVALID, "score_new_block: n = %lld out of range", (long long)n);
  if (u0 < 0 || u1 > h->cfg.num_users || u0 > u1) BPRX_FAIL(h, BPRX_E_INVALID, "score_new_block: bad user range [%d,%d)", u0, u1);
  const bool empty = n == 0 || u0 == u1;
  if (!empty && (!P || !out)) BPRX_FAIL(h, BPRX_E_INVALID, "score_new_block: null pointer");
  hipStream_t s = (hipStream_t)stream;
  // (NEED_ET: the image P was made from stays the current one)
  const int rc = bprx_enter(h, "score_new_block", NEED_BOUND | NEED_ROWS | NEED_ET, KIND_VBPR_NO_FP8, s);
  if (rc || empty) return rc;
  dim3 grid((unsigned)((n + TN - 1) / TN), (unsigned)((u1 - u0 + TM - 1) / TM));
  hipLaunchKernelGGL(k_score_new_gemm, grid, dim3(256), 0, s, (const float *)h->t.Tu, P, (int)n, h->cfg.embed_d, h->PS, u0, u1, out);
  BPRX_LAUNCH_CHECK(h, "k_score_new_gemm");
  return BPRX_OK;
}

// ---- warm items: the full score of caller-owned item rows (include/bprx.h: bprx_score_warm_block / bprx_audience_warm_block) ----
// The checks the two entries share, then the gate: the rows are scored against Gu / Tu only (no catalogue projection is read); Pn
// was made by bprx_project_rows, so the handles are its handles plus BPRMF (d == 0, no Pn).
static int warm_enter(bprx_handle *h, const char *what, const float *Gi_rows, const float *Bi_rows, const float *Pn, int64_t n,
                      bool empty, const float *out, hipStream_t s) {
  if (n < 0 || n >= ((int64_t)1 << 31)) BPRX_FAIL(h, BPRX_E_INVALID, "%s: n = %lld out of range", what, (long long)n);
  if (!empty && (!Gi_rows || !Bi_rows || !out || (h->cfg.embed_d > 0) != (Pn != nullptr)))
    BPRX_FAIL(h, BPRX_E_INVALID, "%s: null pointer", what);
  if (h->cfg.model == BPRX_MODEL_VBPR && h->cfg.feat_dtype == BPRX_F_FP8)
    BPRX_FAIL(h, BPRX_E_INVALID, "%s: fp8 features are not supported for new items (a new row may exceed the max-abs the codes "
                                 "were scaled for and would saturate): fp32 or bf16", what);
  return bprx_enter(h, what, NEED_BOUND | NEED_ROWS | NEED_ET, KIND_PLAIN, s);
}

static GemmArgs warm_args(const bprx_handle *h, const float *Gi_rows, const float *Bi_rows, const float *Pn, int64_t n) {
  GemmArgs g;
  g.Gu = h->t.Gu; g.Gi = Gi_rows; g.Bi = Bi_rows; g.Tu = h->t.Tu; g.P = Pn;
  g.U = h->cfg.num_users; g.I = (int)n; g.k = h->cfg.embed_k; g.d = h->cfg.embed_d; g.PS = h->PS;
  return g;
}

extern "C" int bprx_score_warm_block(bprx_handle *h, int32_t u0, int32_t u1, const float *Gi_rows, const float *Bi_rows, const float *Pn,
                                     int64_t n, float *out, void *stream) {
  if (!h) return BPRX_E_INVALID;
  if (u0 < 0 || u1 > h->cfg.num_users || u0 > u1) BPRX_FAIL(h, BPRX_E_INVALID, "score_warm_block: bad user range [%d,%d)", u0, u1);
  const bool empty = n == 0 || u0 == u1;
  hipStream_t s = (hipStream_t)stream;
  const int rc = warm_enter(h, "score_warm_block", Gi_rows, Bi_rows, Pn, n, empty, out, s);
  if (rc || empty) return rc;
  if (h->cfg.embed_k % 2 || h->cfg.embed_d % 2)              // an odd width: the non-MFMA kernel, as bprx_score_block
    return bprx_launch_score_block(h, u0, u1, out, s, {h->t.Gu, h->t.Tu}, {Gi_rows, Bi_rows, Pn, (int)n});
  dim3 grid((unsigned)((n + TN - 1) / TN), (unsigned)((u1 - u0 + TM - 1) / TM));
  hipLaunchKernelGGL(k_score_gemm, grid, dim3(256), 0, s, warm_args(h, Gi_rows, Bi_rows, Pn, n), u0, u1, out);
  BPRX_LAUNCH_CHECK(h, "k_score_gemm");
  return BPRX_OK;
}

extern "C" int bprx_audience_warm_block(bprx_handle *h, const float *Gi_rows, const float *Bi_rows, const float *Pn, int64_t n,
                                        int64_t q0, int64_t q1, float *out, void *stream) {
  if (!h) return BPRX_E_INVALID;
  if (q0 < 0 || q0 > q1 || q1 > n || q1 - q0 > (int64_t)65535 * TM)
    BPRX_FAIL(h, BPRX_E_INVALID, "audience_warm_block: bad item range [%lld,%lld) of %lld", (long long)q0, (long long)q1, (long long)n);
  hipStream_t s = (hipStream_t)stream;
  const int rc = warm_enter(h, "audience_warm_block", Gi_rows, Bi_rows, Pn, n, q0 == q1, out, s);
  if (rc || q0 == q1) return rc;
  const GemmArgs g = warm_args(h, Gi_rows, Bi_rows, Pn, n);
  dim3 grid((unsigned)((g.U + TN - 1) / TN), (unsigned)((q1 - q0 + TM - 1) / TM));
  hipLaunchKernelGGL(k_audience_gemm, grid, dim3(256), 0, s, g, (int)q0, (int)q1, out);
  BPRX_LAUNCH_CHECK(h, "k_audience_gemm");
  return BPRX_OK;
}

// ---- similar items: bprx_sim_rnorm / bprx_sim_block (include/bprx.h) ----
// The checks the two entries share, then the gate: the space, the query rows (the catalogue: nq == num_items; the caller's rows:
// visual only), fp8 in a space that reads P, and plan_read's own (bound, handle kind).
int bprx_sim_enter(bprx_handle *h, const char *what, int32_t space, const float *Pq, int64_t nq, hipStream_t s) {
  if (space != BPRX_SIM_LATENT && space != BPRX_SIM_VISUAL && space != BPRX_SIM_BOTH)
    BPRX_FAIL(h, BPRX_E_INVALID, "%s: unknown space %d (BPRX_SIM_LATENT, _VISUAL or _BOTH)", what, space);
  if (Pq && space != BPRX_SIM_VISUAL) BPRX_FAIL(h, BPRX_E_INVALID, "%s: rows from outside the catalogue live in the visual space only", what);
  if (nq < 0 || nq >= ((int64_t)1 << 31)) BPRX_FAIL(h, BPRX_E_INVALID, "%s: nq = %lld out of range", what, (long long)nq);
  if (!Pq && nq != h->cfg.num_items)
    BPRX_FAIL(h, BPRX_E_INVALID, "%s: nq = %lld, the catalogue has %d items", what, (long long)nq, h->cfg.num_items);
  const bool latent = space == BPRX_SIM_LATENT;
  if (!latent && h->cfg.model == BPRX_MODEL_VBPR && h->cfg.feat_dtype == BPRX_F_FP8)
    BPRX_FAIL(h, BPRX_E_INVALID, "%s: the visual space of an fp8 handle is not supported (its projections carry the rounding of the "
                                 "fp8 codes): use BPRX_SIM_LATENT, or fp32 / bf16 features", what);
  return bprx_enter(h, what, NEED_BOUND | NEED_ROWS | (latent ? 0 : NEED_P_ALL), latent ? KIND_PLAIN : KIND_VBPR, s);
}

// the parts of z for the catalogue (Pq == nullptr) or the caller's rows: [Gi over k | P over d], absent parts have width 0
void bprx_sim_parts(const bprx_handle *h, int32_t space, const float *Pq, SimPart &g, SimPart &p) {
  g = {h->t.Gi, space != BPRX_SIM_VISUAL && !Pq ? h->cfg.embed_k : 0, h->cfg.embed_k};
  p = {Pq ? Pq : h->P, space != BPRX_SIM_LATENT ? h->cfg.embed_d : 0, h->PS};
}

extern "C" int bprx_sim_rnorm(bprx_handle *h, int32_t space, const float *Pq, int64_t nq, float *rn, void *stream) {
  if (!h) return BPRX_E_INVALID;
  if (!rn) BPRX_FAIL(h, BPRX_E_INVALID, "sim_rnorm: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const int rc = bprx_sim_enter(h, "sim_rnorm", space, Pq, nq, s);
  if (rc || nq == 0) return rc;
  SimPart g, p;
  bprx_sim_parts(h, space, Pq, g, p);
  constexpr int rows = 256 / RN_LANES;
  hipLaunchKernelGGL(k_sim_rnorm, dim3((unsigned)((nq + rows - 1) / rows)), dim3(256), 0, s, g, p, (int)nq, rn);
  BPRX_LAUNCH_CHECK(h, "k_sim_rnorm");
  return BPRX_OK;
}

extern "C" int bprx_sim_block(bprx_handle *h, int32_t space, const float *Pq, int64_t nq, int64_t q0, int64_t q1, const float *rn_q,
                              const float *rn_items, float *out, void *stream) {
  if (!h) return BPRX_E_INVALID;
  if (!rn_q || !rn_items || !out) BPRX_FAIL(h, BPRX_E_INVALID, "sim_block: null pointer");
  if (q0 < 0 || q0 > q1 || q1 > nq || q1 - q0 > (int64_t)65535 * TM)
    BPRX_FAIL(h, BPRX_E_INVALID, "sim_block: bad query range [%lld,%lld) of %lld", (long long)q0, (long long)q1, (long long)nq);
  hipStream_t s = (hipStream_t)stream;
  const int rc = bprx_sim_enter(h, "sim_block", space, Pq, nq, s);
  if (rc || q0 == q1) return rc;
  SimPart ag, ap, bg, bp;
  bprx_sim_parts(h, space, Pq, ag, ap);
  bprx_sim_parts(h, space, nullptr, bg, bp);
  bg.w = ag.w;                                               // (the caller's rows have no Gi part)
  const int I = h->cfg.num_items;
  dim3 grid((unsigned)((I + TN - 1) / TN), (unsigned)((q1 - q0 + TM - 1) / TM));
  hipLaunchKernelGGL(k_sim_gemm, grid, dim3(256), 0, s, ag, ap, bg, bp, I, (int)q0, (int)q1, rn_q, rn_items, out);
  BPRX_LAUNCH_CHECK(h, "k_sim_gemm");
  return BPRX_OK;
}

// used by bprx_score_block when the factor widths allow the MFMA path (K step of 2)
int bprx_launch_score_gemm(bprx_handle *h, int32_t u0, int32_t u1, float *out, hipStream_t s, UserRows rows) {
  GemmArgs g;
  g.Gu = rows.Gu; g.Gi = h->t.Gi; g.Bi = h->t.Bi; g.Tu = rows.Tu; g.P = h->P;
  g.U = h->cfg.num_users; g.I = h->cfg.num_items; g.k = h->cfg.embed_k; g.d = h->cfg.embed_d; g.PS = h->PS;
  dim3 grid((g.I + TN - 1) / TN, (u1 - u0 + TM - 1) / TM);
  hipLaunchKernelGGL(k_score_gemm, grid, dim3(256), 0, s, g, u0, u1, out);
  BPRX_LAUNCH_CHECK(h, "k_score_gemm");
  return BPRX_OK;
}

extern "C" int bprx_eval_users(bprx_handle *h, int32_t u0, int32_t u1, const float *scores, const int64_t *train_ptr,
                               const int32_t *train_items, const int64_t *eval_ptr, const int32_t *eval_items, int32_t K,
                               double *out, void *stream) {
  if (!h) return BPRX_E_INVALID;
  if (u0 < 0 || u1 > h->cfg.num_users || u0 > u1 || !scores || !train_ptr || !train_items || !eval_ptr || !eval_items ||
      !out || K <= 0)
    BPRX_FAIL(h, BPRX_E_INVALID, "eval_users: bad argument");
  const int rc = bprx_enter(h, "eval_users", 0, KIND_ANY, (hipStream_t)stream);
  if (rc || u0 == u1) return rc;
  hipLaunchKernelGGL(k_eval_users, dim3(u1 - u0), dim3(256), 0, (hipStream_t)stream, scores, u0, h->cfg.num_items, train_ptr,
                     train_items, eval_ptr, eval_items, K, out, h->errflag);
  BPRX_LAUNCH_CHECK(h, "k_eval_users");
  return BPRX_OK;
}

// ---- item-sharded evaluation (see k_eval_pos / k_eval_counts / k_eval_finish) ----
extern "C" int bprx_eval_pos(bprx_handle *h, int32_t u0, int32_t u1, const float *scores, int32_t item_lo, int32_t items_total,
                             const int64_t *eval_ptr, const int32_t *eval_items, float *sp, void *stream) {
  if (!h) return BPRX_E_INVALID;
  if (u0 < 0 || u0 > u1 || !scores || !eval_ptr || !eval_items || !sp || item_lo < 0 || items_total <= 0)
    BPRX_FAIL(h, BPRX_E_INVALID, "eval_pos: bad argument");
  const int rc = bprx_enter(h, "eval_pos", 0, KIND_ANY, (hipStream_t)stream);
  if (rc || u0 == u1) return rc;
  const int nb = u1 - u0;
  hipLaunchKernelGGL(k_eval_pos, dim3((unsigned)(((int64_t)nb * EVMAX + 255) / 256)), dim3(256), 0, (hipStream_t)stream, scores, u0,
                     nb, h->cfg.num_items, item_lo, items_total, eval_ptr, eval_items, sp, h->errflag);
  BPRX_LAUNCH_CHECK(h, "k_eval_pos");
  return BPRX_OK;
}

extern "C" int bprx_eval_counts(bprx_handle *h, int32_t u0, int32_t u1, const float *scores, int32_t item_lo, int32_t items_total,
                                const int64_t *train_ptr, const int32_t *train_items, const int64_t *eval_ptr,
                                const int32_t *eval_items, const float *sp, int32_t *counts, void *stream) {
  if (!h) return BPRX_E_INVALID;
  if (u0 < 0 || u0 > u1 || !scores || !train_ptr || !train_items || !eval_ptr || !eval_items || !sp || !counts || item_lo < 0)
    BPRX_FAIL(h, BPRX_E_INVALID, "eval_counts: bad argument");
  const int rc = bprx_enter(h, "eval_counts", 0, KIND_ANY, (hipStream_t)stream);
  if (rc || u0 == u1) return rc;
  hipLaunchKernelGGL(k_eval_counts, dim3(u1 - u0), dim3(256), 0, (hipStream_t)stream, scores, u0, h->cfg.num_items, item_lo,
                     items_total, train_ptr, train_items, eval_ptr, eval_items, sp, counts);
  BPRX_LAUNCH_CHECK(h, "k_eval_counts");
  return BPRX_OK;
}

extern "C" int bprx_eval_finish(bprx_handle *h, int32_t u0, int32_t u1, int32_t items_total, const int64_t *eval_ptr,
                                const float *sp, const int32_t *counts, int32_t K, double *out, void *stream) {
  if (!h) return BPRX_E_INVALID;
  if (u0 < 0 || u0 > u1 || !eval_ptr || !sp || !counts || !out || K <= 0 || items_total <= 0)
    BPRX_FAIL(h, BPRX_E_INVALID, "eval_finish: bad argument");
  const int rc = bprx_enter(h, "eval_finish", 0, KIND_ANY, (hipStream_t)stream);
  if (rc || u0 == u1) return rc;
  const int nb = u1 - u0;
  hipLaunchKernelGGL(k_eval_finish, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, (hipStream_t)stream, u0, nb, items_total,
                     eval_ptr, sp, counts, K, out);
  BPRX_LAUNCH_CHECK(h, "k_eval_finish");
  return BPRX_OK;
}
