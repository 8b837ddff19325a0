// bprx_acf.hip -- ACF (ACF.py:20-270) on a BPRMF handle: bprx_bind_acf, bprx_acf_profiles, and what bprx_step /
// bprx_score_pairs / bprx_score_block do on an ACF handle (include/bprx.h).
//
// Per call that needs user profiles g'_u:
//   k_acf_wcat      [Wci | Wix | 0] as the projection operand (fp32 [Cp][NP]; bf16 features: hi + lo bf16 halves, transposed)
//   k_acf_mark      the distinct items of the users' histories -> ilist (marks in imark, cleared by k_acf_unmark)
//   k_acf_proj_*    Z_l = f_l [Wci | Wix]  [M, NP] per listed item: one MFMA GEMM over the rows (l, m), f32 32x32x2 for fp32
//                   features, bf16 32x32x16 for bf16 features (W split into two bf16 halves: the features are the only operand
//                   rounded)
//   k_acf_itemvec   GP_l = Wiv^T Gi_l + Wip^T Pi_l per listed item
//   k_acf_user      one workgroup per distinct user: component softmax over m for each history item, item-level softmax over
//                   the history as an online (running max) softmax per wave, merged across the waves; g'_u = g_u + sum alpha Pi
// A step then adds:
//   k_acf_triplet   scores with g', loss terms, the detached gradients of Gi / Gu / Pi into the staging tables
//   k_acf_dense     the twelve attention tensors (g = 2 reg w: sgd or the dense ApplyAdam rule) and the loss (one workgroup, fixed
//                   summation order)
//   k_acf_apply_sgd / k_adam_sweep  sgd on the touched rows / adam_tf23's sparse rule over the whole tables (bprx_sparse.hip)
//   k_acf_finish    clears the user slots and the sgd claim marks
// With bprx_acf_set_gradient(h, BPRX_ACF_GRAD_FULL) a step also differentiates through g'_u (include/bprx.h), between
// k_acf_triplet and k_acf_dense:
//   k_acf_q         q_u = dL/dg'_u per distinct user (row = the user's first batch position)
//   k_acf_user_bwd  one workgroup per distinct user: recomputes both attention levels per history item and adds dZ, dGP, dPi rows
//                   (float atomics), writes dGu_u and the user's [duc | dui | dW1c | dW1i] row
//   k_acf_item_bwd  dGi_l += Wiv dGP_l, dPi_l += Wip dGP_l per listed item
//   k_acf_outer     sum_r R[r] (x) V[r] in split-K partials (dWcu | dWiu over the users, dWiv / dWip over the listed items);
//   k_acf_colsum    column sums of the user rows (dbc0, dbi0, dW1c, dW1i); k_acf_reduce sums partials in ascending order
//   k_acf_proj_bwd_*  [dWci | dWix] = F^T dZ over the rows (l, m) of the listed items: MFMA GEMM, K split over the workgroups
//   k_acf_clear     dZ / dGP rows of the listed items back to zero
// Users the model was not trained on (bprx_acf_fold_in, bprx_acf_profile_rows, bprx_acf_score_rows_block):
//   k_acf_fold      one workgroup per new user, the step loop inside: the forward walk, the user's pairs, a backward walk that
//                   recomputes both levels and keeps only d / dg, the update of the caller's row; no atomics
#include <climits>

#include "bprx_internal.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;

#define ACF_MAX_M 2048
#define ACF_MAX_NP 256
#define ACF_MAX_K 512

struct AcfState {
  DevPool mem;                        // owns every device buffer below
  bprx_acf a;
  int M, C, hc, ha, NP, k, fdt, Cp;   // NP = 32*ceil((h+a)/32); Cp = C rounded up to the K chunk (32)
  int64_t nw[BPRX_ACF_NW];
  float *Z;                           // [I][M][NP]  f_l [Wci | Wix | 0]
  float *GP;                          // [I][a]      Wiv^T Gi_l + Wip^T Pi_l
  float *Wc;                          // [Cp][NP]    fp32 projection operand
  uint16_t *Wh, *Wl;                  // [NP][Cp]    bf16 hi / lo halves of the same, transposed (bf16 features)
  float *gp;                          // [max_batch][k] g' of the batch positions (step: the user's first position)
  float *Gup;                         // [U][k]      g' with the evaluation histories (bprx_score_block)
  float *dPi;                         // [I][k]      staging gradient of Pi, all-zero between steps
  int32_t *uslot;                     // [U]         first batch position of the user in the step; INT_MAX between steps
  int32_t *imark;                     // [I]         item listed in this call; 0 between calls
  int32_t *ilist, *nlist;             // [I], [1]
  bool eval_valid;                    // Gup matches the bound tables
  // full-gradient mode (bprx_acf_set_gradient), allocated at the first switch to BPRX_ACF_GRAD_FULL
  int grad_mode;
  float *dZ;                          // [I][M][NP]  gradient of Z, all-zero between steps
  float *dGP;                         // [I][a]      gradient of GP, all-zero between steps
  float *q;                           // [max_batch][k]        dL/dg'_u at the user's first position
  float *aux;                         // [max_batch][k+2]      k_acf_user: sum_l alpha_l Pi_l, the item softmax's max and denominator
  float *UV;                          // [max_batch][2(h+a)]   per user [duc | dui | dW1c | dW1i]
  float *part;                        // split-K partials (part_floats)
  float *gw[BPRX_ACF_NW];             // gradients of the attention tensors (b_1 of both levels: nullptr, identically zero)
  float *gwbuf;
  size_t part_floats;
  int nsplit_proj;
  // bprx_acf_explain, allocated at its first call
  float *xt;                          // [xt_cap] item-level logits t_l by CSR position of the call's histories
  float *xu;                          // int64 xt_cap, then [U][2 + h]: the item softmax's max and denominator, uc
  int64_t xt_cap;
  // bprx_acf_score_rows_block, allocated at its first call with more rows than gp holds and regrown on demand
  float *prow;                        // [prow_cap][k] g' of the call's rows
  int64_t prow_cap;
};

// ---- projection operand --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_acf_wcat(const float *__restrict__ Wci, const float *__restrict__ Wix, int C, int Cp,
                                                  int hc, int ha, int NP, float *__restrict__ Wc, uint16_t *__restrict__ Wh,
                                                  uint16_t *__restrict__ Wl) {
  const int64_t n = (int64_t)Cp * NP;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(e / NP), j = (int)(e % NP);
    float v = 0.f;
    if (c < C) v = j < hc ? Wci[(int64_t)c * hc + j] : (j < hc + ha ? Wix[(int64_t)c * ha + (j - hc)] : 0.f);
    if (Wc) Wc[e] = v;
    if (Wh) {
      const uint16_t hi = (uint16_t)bf16_rne(v);
      const float rest = v - __uint_as_float((uint32_t)hi << 16);
      Wh[(int64_t)j * Cp + c] = hi;
      Wl[(int64_t)j * Cp + c] = (uint16_t)bf16_rne(rest);
    }
  }
}

// ---- distinct items of the users' histories ------------------------------------------------------------------------
// one wave per position b; users == nullptr: position b is user b; uslot: only the user's first position lists its history
__global__ __launch_bounds__(256) void k_acf_mark(const int32_t *__restrict__ users, int64_t n, const int32_t *__restrict__ uslot,
                                                  const int64_t *__restrict__ ptr, const int32_t *__restrict__ items, int U, int I,
                                                  int32_t *__restrict__ imark, int32_t *__restrict__ ilist, int32_t *__restrict__ nlist,
                                                  int32_t *errflag) {
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (b >= n) return;
  const int u = users ? clamp_index(users[b], U, errflag, 1) : (int)b;
  if (uslot && uslot[u] != (int32_t)b) return;
  const int64_t beg = ptr[u], end = ptr[u + 1];
  for (int64_t p = beg + lane; p < end; p += 64) {
    const int l = clamp_index(items[p], I, errflag, 5);
    if (atomicExch(imark + l, 1) == 0) ilist[atomicAdd(nlist, 1)] = l;
  }
}

__global__ __launch_bounds__(256) void k_acf_unmark(const int32_t *__restrict__ ilist, const int32_t *__restrict__ nlist,
                                                    int32_t *__restrict__ imark) {
  const int n = *nlist;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += gridDim.x * blockDim.x) imark[ilist[e]] = 0;
}

// ---- Z = f_l [Wci | Wix]: MFMA GEMM over the rows (l, m) of the listed items ----------------------------------------------
// A workgroup computes 64 rows x NP columns; wave w takes row tile w & 1 and the column tiles ct == w >> 1 (mod 2).  K runs in
// chunks of 32 staged in LDS.  Row r of the GEMM is component r % M of item list[r / M] (all items when list == nullptr).
__device__ __forceinline__ void acf_store_tile(float *__restrict__ Z, const f32x16 &acc, const int32_t *list, int64_t r0, int64_t nrows,
                                               int M, int NP, int rt, int ct, int lane) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = rt * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    const int64_t gr = r0 + row;
    if (gr >= nrows) continue;
    const int64_t li = gr / M;
    const int m = (int)(gr - li * M);
    const int64_t item = list ? (int64_t)list[li] : li;
    Z[(item * M + m) * NP + ct * 32 + (lane & 31)] = acc[r];
  }
}

template <int NCT>
__global__ __launch_bounds__(256) void k_acf_proj_f32(const float *__restrict__ F, const float *__restrict__ Wc, float *__restrict__ Z,
                                                      const int32_t *__restrict__ list, const int32_t *__restrict__ nlist, int nall,
                                                      int M, int C, int Cp) {
  constexpr int NP = 32 * NCT, NJ = (NCT + 1) / 2;
  __shared__ float As[64][33];
  __shared__ __attribute__((aligned(16))) float Bs[32][NP];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, rt = w & 1, cq = w >> 1;
  const int64_t nrows = (int64_t)(list ? *nlist : nall) * M;
  const int64_t tiles = (nrows + 63) / 64;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t r0 = tile * 64;
    const float *src[2];
    int lrow[2], lc4[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int idx = tid + 256 * q;
      lrow[q] = idx >> 3; lc4[q] = idx & 7;
      const int64_t gr = r0 + lrow[q];
      src[q] = nullptr;
      if (gr < nrows) {
        const int64_t li = gr / M;
        const int64_t item = list ? (int64_t)list[li] : li;
        src[q] = F + (item * M + (gr - li * M)) * (int64_t)C;
      }
    }
    f32x16 acc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
      for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
    for (int kc = 0; kc < Cp; kc += 32) {
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int col = kc + lc4[q] * 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (src[q] && col < C) v = *(const float4 *)(src[q] + col);
        float *d = &As[lrow[q]][lc4[q] * 4];
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
      }
      for (int e = tid; e < 8 * NP; e += 256) {
        const int r = e / (NP / 4), c4 = e % (NP / 4);
        *(float4 *)&Bs[r][c4 * 4] = *(const float4 *)(Wc + (int64_t)(kc + r) * NP + c4 * 4);
      }
      __syncthreads();
#pragma unroll
      for (int kk = 0; kk < 32; kk += 2) {
        const float a = As[rt * 32 + (lane & 31)][kk + (lane >> 5)];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          const int ct = cq + 2 * j;
          if (ct < NCT) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, Bs[kk + (lane >> 5)][ct * 32 + (lane & 31)], acc[j], 0, 0, 0);
        }
      }
      __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int ct = cq + 2 * j;
      if (ct < NCT) acf_store_tile(Z, acc[j], list, r0, nrows, M, NP, rt, ct, lane);
    }
  }
}

// bf16 features: A = the feature rows (bf16, exact), B = W as hi + lo bf16 halves (two MFMAs), fp32 accumulation
template <int NCT>
__global__ __launch_bounds__(256) void k_acf_proj_bf16(const uint16_t *__restrict__ F, const uint16_t *__restrict__ Wh,
                                                       const uint16_t *__restrict__ Wl, float *__restrict__ Z,
                                                       const int32_t *__restrict__ list, const int32_t *__restrict__ nlist, int nall,
                                                       int M, int C, int Cp) {
  constexpr int NP = 32 * NCT, NJ = (NCT + 1) / 2;
  __shared__ __attribute__((aligned(16))) uint16_t As[64][40];
  __shared__ __attribute__((aligned(16))) uint16_t Bh[NP][40];
  __shared__ __attribute__((aligned(16))) uint16_t Bl[NP][40];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, rt = w & 1, cq = w >> 1;
  const int64_t nrows = (int64_t)(list ? *nlist : nall) * M;
  const int64_t tiles = (nrows + 63) / 64;
  const int lrow = tid >> 2, lc8 = tid & 3;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t r0 = tile * 64;
    const uint16_t *src = nullptr;
    {
      const int64_t gr = r0 + lrow;
      if (gr < nrows) {
        const int64_t li = gr / M;
        const int64_t item = list ? (int64_t)list[li] : li;
        src = F + (item * M + (gr - li * M)) * (int64_t)C;
      }
    }
    f32x16 acc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
      for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
    for (int kc = 0; kc < Cp; kc += 32) {
      {
        const int col = kc + lc8 * 8;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (src && col < C) v = *(const uint4 *)(src + col);
        *(uint4 *)&As[lrow][lc8 * 8] = v;
      }
      for (int e = tid; e < NP * 4; e += 256) {
        const int r = e >> 2, c8 = e & 3;
        *(uint4 *)&Bh[r][c8 * 8] = *(const uint4 *)(Wh + (int64_t)r * Cp + kc + c8 * 8);
        *(uint4 *)&Bl[r][c8 * 8] = *(const uint4 *)(Wl + (int64_t)r * Cp + kc + c8 * 8);
      }
      __syncthreads();
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const bf16x8 a = *(const bf16x8 *)&As[rt * 32 + (lane & 31)][ks * 16 + 8 * (lane >> 5)];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          const int ct = cq + 2 * j;
          if (ct < NCT) {
            const bf16x8 bh = *(const bf16x8 *)&Bh[ct * 32 + (lane & 31)][ks * 16 + 8 * (lane >> 5)];
            const bf16x8 bl = *(const bf16x8 *)&Bl[ct * 32 + (lane & 31)][ks * 16 + 8 * (lane >> 5)];
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, bh, acc[j], 0, 0, 0);
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, bl, acc[j], 0, 0, 0);
          }
        }
      }
      __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int ct = cq + 2 * j;
      if (ct < NCT) acf_store_tile(Z, acc[j], list, r0, nrows, M, NP, rt, ct, lane);
    }
  }
}

// ---- GP_l = Wiv^T Gi_l + Wip^T Pi_l (ACF.py:167-170), one wave per listed item ---------------------------------------
__global__ __launch_bounds__(256) void k_acf_itemvec(const float *__restrict__ Gi, const float *__restrict__ Pi,
                                                     const float *__restrict__ Wiv, const float *__restrict__ Wip,
                                                     const int32_t *__restrict__ list, const int32_t *__restrict__ nlist, int nall,
                                                     int k, int ha, float *__restrict__ GP) {
  const int n = list ? *nlist : nall;
  const int lane = threadIdx.x & 63;
  for (int t = blockIdx.x * 4 + (threadIdx.x >> 6); t < n; t += gridDim.x * 4) {
    const int64_t l = list ? list[t] : t;
    const float *g = Gi + l * k, *p = Pi + l * k;
    for (int j = lane; j < ha; j += 64) {
      float sv = 0.f, sp = 0.f;
      for (int c = 0; c < k; ++c) {
        sv = fmaf(g[c], Wiv[(int64_t)c * ha + j], sv);
        sp = fmaf(p[c], Wip[(int64_t)c * ha + j], sp);
      }
      GP[l * ha + j] = sv + sp;
    }
  }
}

// ---- user profiles (calculate_beta_alpha, ACF.py:135-181) --------------------------------------------------------------
struct AcfUserArgs {
  const float *Gu, *Pi, *Z, *GP;
  const float *wcu, *bc0, *w1c, *bc1, *wiu, *bi0, *w1i, *bi1;
  const int64_t *ptr;
  const int32_t *items;
  int32_t *errflag;
  int U, I, k, M, hc, ha, NP;
};

#define ACF_JR 4                      // column slots per lane: h, a <= ACF_MAX_NP = 4 * 64

// Both attention levels of one history entry for the row whose (uc, ui) are in LDS, shared by k_acf_user,
// k_acf_user_bwd and k_acf_fold: leaves e^(s_m - max) in beta[M] (the calling wave's), 1 / their sum in inv, the lane's item-level relu inputs in
// prej, and returns t_l.
__device__ __forceinline__ float acf_entry_fwd(const AcfUserArgs &A, int l, const float *uc, const float *ui, const float *w1c,
                                               const float *w1i, float bc1, float bi1, float *beta, int lane, float &inv,
                                               float (&prej)[ACF_JR]) {
  const int M = A.M, hc = A.hc, ha = A.ha, NP = A.NP;
  const float *Zl = A.Z + (int64_t)l * M * NP;
  float lmax = -INFINITY;
  for (int m = lane; m < M; m += 64) {
    const float *z = Zl + (int64_t)m * NP;
    float s = 0.f;
    for (int j = 0; j < hc; ++j) s = fmaf(w1c[j], fmaxf(uc[j] + z[j], 0.f), s);
    s += bc1;
    beta[m] = s;
    lmax = fmaxf(lmax, s);
  }
  lmax = wave_max(lmax);
  wave_sync();
  float lsum = 0.f;
  for (int m = lane; m < M; m += 64) {
    const float e = expf(beta[m] - lmax);
    beta[m] = e;
    lsum += e;
  }
  lsum = wave_sum(lsum);
  wave_sync();
  inv = 1.0f / lsum;
  float tp = 0.f;
#pragma unroll
  for (int i = 0; i < ACF_JR; ++i) {
    const int j = lane + 64 * i;
    prej[i] = 0.f;
    if (j < ha) {
      float xz = 0.f;
      for (int m = 0; m < M; ++m) xz = fmaf(beta[m], Zl[(int64_t)m * NP + hc + j], xz);
      prej[i] = ui[j] + A.GP[(int64_t)l * ha + j] + xz * inv;
      tp = fmaf(w1i[j], fmaxf(prej[i], 0.f), tp);
    }
  }
  return wave_sum(tp) + bi1;
}

// One workgroup (4 waves) per position b.  Wave w walks history entries w, w+4, ...; for each item l:
//   s_m = w1c.relu(uc + Z_lm[:h]) + bc1 (lane per m), beta = softmax_m(s), xz = sum_m beta_m Z_lm[h:] (lane per column),
//   t = w1i.relu(ui + GP_l + xz) + bi1; the wave keeps a running max / denominator / sum of e^(t - max) Pi_l.
// LDS: gu[k] uc[h] ui[a] w1c[h] w1i[a] | per wave: beta[M], acc[k] | wmx[4] wden[4]
// MODE (compile time, so that ACF_USER_PLAIN stays the detached step's kernel unchanged):
//   ACF_USER_AUX      full-gradient mode: also store what k_acf_user_bwd needs of the forward
//   ACF_USER_EXPLAIN  bprx_acf_explain's attention pass: the same walk, but instead of g' it keeps what makes alpha_l recoverable
//                     per entry: `out` = the item-level logits t_l by CSR position, `aux` = int64 size of `out`, then per USER a
//                     row [softmax max, denominator, uc[h]]; the sum of e^(t - max) Pi_l is not formed
enum { ACF_USER_PLAIN = 0, ACF_USER_AUX = 1, ACF_USER_EXPLAIN = 2 };
template <int MODE>
__global__ __launch_bounds__(256) void k_acf_user(AcfUserArgs A, const int32_t *__restrict__ users, int64_t n,
                                                  const int32_t *__restrict__ uslot, float *__restrict__ out,
                                                  float *__restrict__ aux) {
  constexpr bool AUX = MODE == ACF_USER_AUX, EXPL = MODE == ACF_USER_EXPLAIN;
  extern __shared__ float sm[];
  const int64_t b = blockIdx.x;
  if (b >= n) return;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int u = users ? clamp_index(users[b], A.U, A.errflag, 1) : (int)b;
  if (uslot && uslot[u] != (int32_t)b) return;
  const int k = A.k, M = A.M, hc = A.hc, ha = A.ha, NP = A.NP;
  float *gu = sm, *uc = gu + k, *ui = uc + hc, *w1c = ui + ha, *w1i = w1c + hc;
  float *wbase = w1i + ha;
  float *beta = wbase + (size_t)w * (M + k), *acc = beta + M;
  float *wmx = wbase + 4 * (size_t)(M + k), *wden = wmx + 4;
  for (int c = tid; c < k; c += 256) gu[c] = A.Gu[(int64_t)u * k + c];
  for (int j = tid; j < hc; j += 256) w1c[j] = A.w1c[j];
  for (int j = tid; j < ha; j += 256) w1i[j] = A.w1i[j];
  __syncthreads();
  for (int j = tid; j < hc + ha; j += 256) {                 // W_0_u^T g_u + b_0 of both levels
    float s = 0.f;
    if (j < hc) {
      for (int c = 0; c < k; ++c) s = fmaf(gu[c], A.wcu[(int64_t)c * hc + j], s);
      uc[j] = s + A.bc0[j];
    } else {
      const int jj = j - hc;
      for (int c = 0; c < k; ++c) s = fmaf(gu[c], A.wiu[(int64_t)c * ha + jj], s);
      ui[jj] = s + A.bi0[jj];
    }
  }
  if (!EXPL)
    for (int c = lane; c < k; c += 64) acc[c] = 0.f;
  __syncthreads();
  const float bc1 = A.bc1[0], bi1 = A.bi1[0];
  const int64_t beg = A.ptr[u], end = A.ptr[u + 1];
  const int64_t ncap = EXPL ? *(const int64_t *)aux : 0;      // EXPL: entries `out` has room for
  float mx = -INFINITY, den = 0.f;
  for (int64_t p = beg + w; p < end; p += 4) {
    const int l = clamp_index(A.items[p], A.I, A.errflag, 5);
    float inv, prej[ACF_JR];
    const float t = acf_entry_fwd(A, l, uc, ui, w1c, w1i, bc1, bi1, beta, lane, inv, prej);
    const float nmx = fmaxf(mx, t);
    const float sc = expf(mx - nmx), e = expf(t - nmx);        // (mx = -inf at the first item: sc = 0)
    den = den * sc + e;
    if (EXPL) {
      if (lane == 0 && p >= 0 && p < ncap) out[p] = t;
    } else {
      const float *pl = A.Pi + (int64_t)l * k;
      for (int c = lane; c < k; c += 64) acc[c] = acc[c] * sc + e * pl[c];
    }
    mx = nmx;
    wave_sync();                                               // beta is rewritten by the next item
  }
  if (lane == 0) { wmx[w] = mx; wden[w] = den; }
  __syncthreads();
  float gm = -INFINITY;
#pragma unroll
  for (int q = 0; q < 4; ++q) gm = fmaxf(gm, wmx[q]);
  float f[4], D = 0.f;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    f[q] = wden[q] > 0.f ? expf(wmx[q] - gm) : 0.f;
    D += wden[q] * f[q];
  }
  if (EXPL) {
    float *st = aux + 2 + (int64_t)u * (2 + hc);
    if (tid == 0) { st[0] = gm; st[1] = D; }
    for (int j = tid; j < hc; j += 256) st[2 + j] = uc[j];
    return;
  }
  for (int c = tid; c < k; c += 256) {
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (f[q] != 0.f) s += wbase[(size_t)q * (M + k) + M + c] * f[q];
    out[b * k + c] = D > 0.f ? gu[c] + s / D : gu[c];
    if (AUX) aux[b * (k + 2) + c] = D > 0.f ? s / D : 0.f;   // sum_l alpha_l Pi_l
  }
  if (AUX && tid == 0) {                                     // the item softmax's max and denominator
    aux[b * (k + 2) + k] = gm;
    aux[b * (k + 2) + k + 1] = D;
  }
}

// ---- step ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_acf_claim(const int32_t *__restrict__ user, int64_t B, int U, int32_t *__restrict__ uslot,
                                                   int32_t *errflag) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) atomicMin(uslot + clamp_index(user[b], U, errflag, 1), (int32_t)b);
}

struct AcfStepArgs {
  const float *Gu, *Gi, *Pi, *gp;
  float *dGu, *dGi, *dPi, *lossb;
  const int32_t *uslot;
  int32_t *errflag;
  int U, I, k;
  float reg;
};

// one wave per triplet (ACF.py:239-270 with the detached g'_u)
__global__ __launch_bounds__(256) void k_acf_triplet(AcfStepArgs A, const int32_t *__restrict__ user, const int32_t *__restrict__ pos,
                                                     const int32_t *__restrict__ neg, int64_t B) {
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (b >= B) return;
  const int u = clamp_index(user[b], A.U, A.errflag, 1), i = clamp_index(pos[b], A.I, A.errflag, 2),
            j = clamp_index(neg[b], A.I, A.errflag, 2);
  const int k = A.k;
  const float *g = A.gp + (int64_t)A.uslot[u] * k;
  const float *gu = A.Gu + (int64_t)u * k, *gi = A.Gi + (int64_t)i * k, *gj = A.Gi + (int64_t)j * k;
  const float *pi = A.Pi + (int64_t)i * k, *pj = A.Pi + (int64_t)j * k;
  float xp = 0.f, xn = 0.f, nrm = 0.f;
  for (int c = lane; c < k; c += 64) {
    xp = fmaf(g[c], gi[c], xp);
    xn = fmaf(g[c], gj[c], xn);
    nrm += gu[c] * gu[c] + gi[c] * gi[c] + gj[c] * gj[c] + pi[c] * pi[c] + pj[c] * pj[c];
  }
  xp = wave_sum(xp); xn = wave_sum(xn); nrm = wave_sum(nrm);
  const float diff = xp - xn;
  const bool inr = (diff >= -80.0f) && (diff <= 1e8f);                 // tf.clip_by_value gradient mask
  const float cl = fminf(fmaxf(diff, -80.0f), 1e8f);
  const float z = -cl;                                                 // softplus(z), stable form
  const float sp = z > 0.f ? z + log1pf(expf(-z)) : log1pf(expf(z));
  const float gd = inr ? -1.0f / (1.0f + expf(diff)) : 0.f;           // -sigmoid(-diff)
  const float r2 = 2.f * A.reg;
  if (lane == 0) A.lossb[b] = sp + A.reg * nrm;
  float *dgu = A.dGu + (int64_t)u * k, *dgi = A.dGi + (int64_t)i * k, *dgj = A.dGi + (int64_t)j * k;
  float *dpi = A.dPi + (int64_t)i * k, *dpj = A.dPi + (int64_t)j * k;
  for (int c = lane; c < k; c += 64) {
    atomicAdd(dgi + c, gd * g[c] + r2 * gi[c]);
    atomicAdd(dgj + c, -gd * g[c] + r2 * gj[c]);
    if (r2 != 0.f) {
      atomicAdd(dgu + c, r2 * gu[c]);
      atomicAdd(dpi + c, r2 * pi[c]);
      atomicAdd(dpj + c, r2 * pj[c]);
    }
  }
}

// The attention tensors (gradient 2 reg w, plus T.g in full-gradient mode) and the step's loss, in ONE workgroup: fixed
// summation order.
struct AcfDenseArgs {
  float *w[BPRX_ACF_NW], *m[BPRX_ACF_NW], *v[BPRX_ACF_NW];
  const float *g[BPRX_ACF_NW];                                // full-gradient mode; nullptr: the gradient is 2 reg w alone
  int64_t n[BPRX_ACF_NW];
};
__global__ __launch_bounds__(1024) void k_acf_dense(AcfDenseArgs T, int adam, float lr_t, float reg, float b1, float b2, float eps,
                                                    const float *__restrict__ lossb, int64_t B, float *__restrict__ loss_out) {
  const float r2 = 2.f * reg;
  double sq = 0.0, ls = 0.0;
  for (int q = 0; q < BPRX_ACF_NW; ++q) {
    float *p = T.w[q];
    const float *gq = T.g[q];
    for (int64_t e = threadIdx.x; e < T.n[q]; e += 1024) {
      const float pv = p[e];
      float g = r2 * pv;
      if (gq) g += gq[e];
      sq += (double)pv * (double)pv;
      p[e] = dense_adam_elem(pv, T.m[q] + e, T.v[q] + e, g, adam, lr_t, b1, b2, eps);
    }
  }
  for (int64_t b = threadIdx.x; b < B; b += 1024) ls += (double)lossb[b];
  const double loss = block_sum_1024(ls + (double)reg * sq);
  if (threadIdx.x == 0 && loss_out) *loss_out = (float)loss;
}

// sgd on the touched rows: one wave per (triplet, role); the first claimant of a row applies and clears its gradient
__global__ __launch_bounds__(256) void k_acf_apply_sgd(float *Gu, float *Gi, float *Pi, float *dGu, float *dGi, float *dPi,
                                                       uint32_t *flagU, uint32_t *flagI, const int32_t *__restrict__ user,
                                                       const int32_t *__restrict__ pos, const int32_t *__restrict__ neg, int64_t B,
                                                       int U, int I, int k, float lr) {
  const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (t >= 3 * B) return;
  const int role = (int)(t / B);
  const int64_t b = t - (int64_t)role * B;
  const int r = role == 0 ? clamp_quiet(user[b], U) : clamp_quiet(role == 1 ? pos[b] : neg[b], I);
  int claim = 0;
  if (lane == 0) claim = atomicExch(role == 0 ? flagU + r : flagI + r, 1u) == 0u;
  claim = __shfl(claim, 0, 64);
  if (!claim) return;
  const int64_t o = (int64_t)r * k;
  for (int c = lane; c < k; c += 64) {
    if (role == 0) {
      Gu[o + c] -= lr * dGu[o + c]; dGu[o + c] = 0.f;
    } else {
      Gi[o + c] -= lr * dGi[o + c]; dGi[o + c] = 0.f;
      Pi[o + c] -= lr * dPi[o + c]; dPi[o + c] = 0.f;
    }
  }
}

__global__ __launch_bounds__(256) void k_acf_finish(const int32_t *__restrict__ user, const int32_t *__restrict__ pos,
                                                    const int32_t *__restrict__ neg, int64_t B, int U, int I, int32_t *uslot,
                                                    uint32_t *flagU, uint32_t *flagI) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int u = clamp_quiet(user[b], U), i = clamp_quiet(pos[b], I), j = clamp_quiet(neg[b], I);
  uslot[u] = INT_MAX;
  flagU[u] = 0u; flagI[i] = 0u; flagI[j] = 0u;
}

// score_pairs: x_b = g'_b . Gi_item (ACF.py:210)
__global__ __launch_bounds__(256) void k_acf_score(const float *__restrict__ gp, const float *__restrict__ Gi,
                                                   const int32_t *__restrict__ item, int64_t n, int I, int k, float *__restrict__ x,
                                                   int32_t *errflag) {
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (b >= n) return;
  const int i = clamp_index(item[b], I, errflag, 2);
  float s = 0.f;
  for (int c = lane; c < k; c += 64) s = fmaf(gp[b * k + c], Gi[(int64_t)i * k + c], s);
  s = wave_sum(s);
  if (lane == 0) x[b] = s;
}

// ---- bprx_acf_explain: the pair pass ----------------------------------------------------------------------------------
// x_ui = g_u.Gi_i + sum_l alpha_l (Pi_l.Gi_i): one WAVE per pair (u, i), four pairs per workgroup.  alpha_l = e^(t_l - max) / D from
// the attention pass's logits and per-user row; Pi_l.Gi_i is a lane-strided dot (Gi_i in registers) with a butterfly reduction, so
// every lane holds the same c_l and sum_l c_l is a compensated sum in history order (base is added last).  The `top` largest c_l live one per lane in lanes
// 0..top-1, sorted: an entry that beats the last slot is ranked by a ballot (slots >= it stay in front: equal values keep
// ascending positions) and the tail shifts one lane up.  No history-sized buffer.  beta_l is then recomputed from the Z rows for the
// selected entries only (a lane per component m, as k_acf_user).
// LDS: w1c[h] | per wave: uc[h] e[M]
struct AcfExplainArgs {
  const float *Gu, *Gi, *Pi, *Z, *w1c, *bc1;
  const float *tl, *ustat;            // attention pass: logits by CSR position; per user [max, D, uc[h]]
  const int64_t *ptr;
  const int32_t *items;
  int32_t *errflag;
  int64_t ncap;                       // entries of tl
  int U, I, k, M, hc, NP, top;
  float *score, *base;
  int32_t *pos, *hist_item;
  float *alpha, *contrib;
  int32_t *peak;
  float *beta_peak, *beta;
};

__global__ __launch_bounds__(256) void k_acf_explain(AcfExplainArgs A, const int32_t *__restrict__ user,
                                                     const int32_t *__restrict__ item, int64_t n) {
  extern __shared__ float sm[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int k = A.k, M = A.M, hc = A.hc, NP = A.NP, top = A.top;
  float *w1c = sm, *uc = w1c + hc + (size_t)w * (hc + M), *eb = uc + hc;
  for (int j = tid; j < hc; j += 256) w1c[j] = A.w1c[j];
  __syncthreads();
  const int64_t b = (int64_t)blockIdx.x * 4 + w;
  if (b >= n) return;
  const int u = clamp_index(user[b], A.U, A.errflag, 1), i = clamp_index(item[b], A.I, A.errflag, 2);
  const float *st = A.ustat + (int64_t)u * (2 + hc);
  const float gm = st[0], D = st[1];
  for (int j = lane; j < hc; j += 64) uc[j] = st[2 + j];
  wave_sync();
  const float *gu = A.Gu + (int64_t)u * k, *gi = A.Gi + (int64_t)i * k;
  float gir[ACF_MAX_K / 64], bs = 0.f;
#pragma unroll
  for (int q = 0; q < ACF_MAX_K / 64; ++q) {
    const int c = lane + 64 * q;
    gir[q] = c < k ? gi[c] : 0.f;
    if (c < k) bs = fmaf(gu[c], gir[q], bs);
  }
  bs = wave_sum(bs);
  int64_t beg = A.ptr[u], end = A.ptr[u + 1];
  if (beg < 0) beg = 0;
  if (end > A.ncap) end = A.ncap;                             // (a CSR that is not monotone: stay inside the workspace)
  float sc = 0.f, comp = 0.f;                                 // sum_l c_l in history order, compensated (Kahan): thousands of
                                                              // small terms must not each round at the ulp of the running sum
  float tv = 0.f, thr = 0.f;                                  // this lane's slot (lane < top); thr = the last slot once all are taken
  int tp = -1, cnt = 0;
  for (int64_t p0 = beg; p0 < end; p0 += 64) {
    const int64_t p = p0 + lane;
    int l = 0;
    float a = 0.f;
    if (p < end) {
      l = clamp_index(A.items[p], A.I, A.errflag, 5);
      a = expf(A.tl[p] - gm) / D;
    }
    const int m = (int)(end - p0 < 64 ? end - p0 : 64);
    for (int e = 0; e < m; ++e) {
      const int le = __shfl(l, e, 64);
      const float ae = __shfl(a, e, 64);
      const float *pl = A.Pi + (int64_t)le * k;
      float d = 0.f;
#pragma unroll
      for (int q = 0; q < ACF_MAX_K / 64; ++q) {
        const int c = lane + 64 * q;
        if (c < k) d = fmaf(pl[c], gir[q], d);
      }
      d = wave_sum(d);
      const float c = ae * d;
      {
        const float y = c - comp, ns = sc + y;
        comp = (ns - sc) - y;
        sc = ns;
      }
      if (cnt < top || c > thr) {
        const int rank = __popcll(__ballot(lane < cnt && tv >= c));
        if (rank < top) {
          const float uv = __shfl_up(tv, 1, 64);
          const int up = __shfl_up(tp, 1, 64);
          if (lane == rank) {
            tv = c;
            tp = (int)(p0 - beg) + e;
          } else if (lane > rank && lane < top) {
            tv = uv;
            tp = up;
          }
          if (cnt < top) ++cnt;
          if (cnt == top) thr = __shfl(tv, top - 1, 64);
        }
      }
    }
  }
  if (lane == 0) {
    A.score[b] = bs + sc;
    A.base[b] = bs;
  }
  const float bc1 = A.bc1[0];
  for (int s = 0; s < top; ++s) {
    const int64_t o = b * top + s;
    if (s >= cnt) {                                            // beyond the history
      if (lane == 0) {
        A.pos[o] = -1; A.hist_item[o] = -1; A.peak[o] = -1;
        A.alpha[o] = 0.f; A.contrib[o] = 0.f; A.beta_peak[o] = 0.f;
      }
      if (A.beta)
        for (int m = lane; m < M; m += 64) A.beta[o * M + m] = 0.f;
      continue;
    }
    const int ps = __shfl(tp, s, 64);
    const float cs = __shfl(tv, s, 64);
    const int64_t p = beg + ps;
    const int l = clamp_index(A.items[p], A.I, A.errflag, 5);
    const float al = expf(A.tl[p] - gm) / D;
    const float *Zl = A.Z + (int64_t)l * M * NP;
    float lmax = -INFINITY;
    for (int m = lane; m < M; m += 64) {                       // component scores, as k_acf_user (rows read four columns at a time)
      const float *z = Zl + (int64_t)m * NP;
      float sv = 0.f;
      for (int j = 0; j < hc; j += 4) {
        const float4 v = *(const float4 *)(z + j);             // NP % 32 == 0: the row holds ceil4(h) columns
        sv = fmaf(w1c[j], fmaxf(uc[j] + v.x, 0.f), sv);
        if (j + 1 < hc) sv = fmaf(w1c[j + 1], fmaxf(uc[j + 1] + v.y, 0.f), sv);
        if (j + 2 < hc) sv = fmaf(w1c[j + 2], fmaxf(uc[j + 2] + v.z, 0.f), sv);
        if (j + 3 < hc) sv = fmaf(w1c[j + 3], fmaxf(uc[j + 3] + v.w, 0.f), sv);
      }
      sv += bc1;
      eb[m] = sv;
      lmax = fmaxf(lmax, sv);
    }
    lmax = wave_max(lmax);
    float lsum = 0.f, bv = -INFINITY;
    int bi = INT_MAX;
    for (int m = lane; m < M; m += 64) {                       // (each lane rereads only what it wrote)
      const float e = expf(eb[m] - lmax);
      eb[m] = e;
      lsum += e;
      if (e > bv) { bv = e; bi = m; }
    }
    lsum = wave_sum(lsum);
    const float inv = 1.0f / lsum;
#pragma unroll
    for (int x = 32; x > 0; x >>= 1) {                         // arg-max, the lowest m among equal values
      const float ov = __shfl_xor(bv, x, 64);
      const int oi = __shfl_xor(bi, x, 64);
      if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    if (lane == 0) {
      A.pos[o] = ps; A.hist_item[o] = l; A.peak[o] = bi;
      A.alpha[o] = al; A.contrib[o] = cs; A.beta_peak[o] = bv * inv;
    }
    if (A.beta)
      for (int m = lane; m < M; m += 64) A.beta[o * M + m] = eb[m] * inv;
  }
}

__global__ __launch_bounds__(256) void k_acf_unclaim(const int32_t *__restrict__ user, int64_t n, int U, int32_t *__restrict__ uslot) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n) return;
  int u = user[b];
  u = u < 0 ? 0 : (u >= U ? U - 1 : u);
  uslot[u] = INT_MAX;
}

// ---- full-gradient mode: the backward through g'_u ------------------------------------------------------------------
// q_u = sum_{b: user_b = u} c_b (Gi_i - Gi_j), c_b = -sigmoid(-d_b) inside the clip range: one wave per triplet, the row of the
// user's first position
__global__ __launch_bounds__(256) void k_acf_q(AcfStepArgs A, const int32_t *__restrict__ user, const int32_t *__restrict__ pos,
                                               const int32_t *__restrict__ neg, int64_t B, float *__restrict__ q) {
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (b >= B) return;
  const int u = clamp_index(user[b], A.U, A.errflag, 1), i = clamp_index(pos[b], A.I, A.errflag, 2),
            j = clamp_index(neg[b], A.I, A.errflag, 2);
  const int k = A.k;
  const int64_t row = A.uslot[u];
  const float *g = A.gp + row * k, *gi = A.Gi + (int64_t)i * k, *gj = A.Gi + (int64_t)j * k;
  float xp = 0.f, xn = 0.f;
  for (int c = lane; c < k; c += 64) {
    xp = fmaf(g[c], gi[c], xp);
    xn = fmaf(g[c], gj[c], xn);
  }
  xp = wave_sum(xp); xn = wave_sum(xn);
  const float diff = xp - xn;
  const bool inr = (diff >= -80.0f) && (diff <= 1e8f);
  if (!inr) return;
  const float gd = -1.0f / (1.0f + expf(diff));
  for (int c = lane; c < k; c += 64) atomicAdd(q + row * k + c, gd * (gi[c] - gj[c]));
}

struct AcfBwdArgs {
  const float *q, *aux;               // [B][k], [B][k+2]
  float *dZ, *dGP, *dPi, *dGu, *UV;
};

// One workgroup (4 waves) per distinct user, at the user's first position b.  Wave w walks history entries w, w+4, ... and
// recomputes beta_l, pre_l and t_l as k_acf_user does; alpha_l = e^(t_l - max) / den comes from the forward's aux row, and
// sum_l alpha_l Pi_l . q from its stored attention part.  Per entry: dt, dpre (dGP_l, dPi_l by atomics), dbeta, ds, then a pass
// over the M rows with a lane per column adds dZ_lm.  The per-lane column sums (duc, dui, dW1c, dW1i) are merged over the waves
// in a fixed order into the user's UV row; dGu_u += q + Wcu duc + Wiu dui.
// LDS: gu[k] q[k] uc[h] ui[a] w1c[h] w1i[a] | per wave: beta[M] dbeta[M] dpre[a] | red[4][2(h+a)] fin[2(h+a)] rb[4]
__global__ __launch_bounds__(256) void k_acf_user_bwd(AcfUserArgs A, AcfBwdArgs G, const int32_t *__restrict__ users, int64_t n,
                                                      const int32_t *__restrict__ uslot) {
  extern __shared__ float sm[];
  const int64_t b = blockIdx.x;
  if (b >= n) return;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int u = clamp_index(users[b], A.U, A.errflag, 1);
  if (uslot[u] != (int32_t)b) return;
  const int k = A.k, M = A.M, hc = A.hc, ha = A.ha, NP = A.NP, W2 = 2 * (hc + ha);
  float *gu = sm, *qs = gu + k, *uc = qs + k, *ui = uc + hc, *w1c = ui + ha, *w1i = w1c + hc;
  float *wbase = w1i + ha;
  const size_t wstride = 2 * (size_t)M + ha;
  float *beta = wbase + (size_t)w * wstride, *dbeta = beta + M, *dpre = dbeta + M;
  float *red = wbase + 4 * wstride, *fin = red + 4 * (size_t)W2, *rb = fin + W2;
  const float *aux = G.aux + b * (k + 2);
  for (int c = tid; c < k; c += 256) {
    gu[c] = A.Gu[(int64_t)u * k + c];
    qs[c] = G.q[b * k + c];
  }
  for (int j = tid; j < hc; j += 256) w1c[j] = A.w1c[j];
  for (int j = tid; j < ha; j += 256) w1i[j] = A.w1i[j];
  __syncthreads();
  for (int j = tid; j < hc + ha; j += 256) {                 // as k_acf_user
    float s = 0.f;
    if (j < hc) {
      for (int c = 0; c < k; ++c) s = fmaf(gu[c], A.wcu[(int64_t)c * hc + j], s);
      uc[j] = s + A.bc0[j];
    } else {
      const int jj = j - hc;
      for (int c = 0; c < k; ++c) s = fmaf(gu[c], A.wiu[(int64_t)c * ha + jj], s);
      ui[jj] = s + A.bi0[jj];
    }
  }
  {
    float pr = 0.f;
    for (int c = tid; c < k; c += 256) pr = fmaf(aux[c], qs[c], pr);
    pr = wave_sum(pr);
    if (lane == 0) rb[w] = pr;
  }
  __syncthreads();
  const float rbar = (rb[0] + rb[1]) + (rb[2] + rb[3]);      // sum_l alpha_l Pi_l . q
  const float gm = aux[k], D = aux[k + 1];
  const float bc1 = A.bc1[0], bi1 = A.bi1[0];
  float duc_r[ACF_JR], dw1c_r[ACF_JR], dui_r[ACF_JR], dw1i_r[ACF_JR];
#pragma unroll
  for (int i = 0; i < ACF_JR; ++i) duc_r[i] = dw1c_r[i] = dui_r[i] = dw1i_r[i] = 0.f;
  const int64_t beg = A.ptr[u], end = A.ptr[u + 1];
  if (D > 0.f) {
    int run_l = -1;
    float run_a = 0.f;
    for (int64_t p = beg + w; p < end; p += 4) {
      const int l = clamp_index(A.items[p], A.I, A.errflag, 5);
      const float *Zl = A.Z + (int64_t)l * M * NP;
      float inv, prej[ACF_JR];
      const float t = acf_entry_fwd(A, l, uc, ui, w1c, w1i, bc1, bi1, beta, lane, inv, prej);
      const float alpha = expf(t - gm) / D;
      const float *pl = A.Pi + (int64_t)l * k;
      float r = 0.f;
      for (int c = lane; c < k; c += 64) r = fmaf(pl[c], qs[c], r);
      r = wave_sum(r);
      const float dt = alpha * (r - rbar);
      // dPi_l += alpha_l q: entries of one item that follow each other in this wave's walk (sorted histories with repeats)
      // are summed first -- hundreds of small adds onto a row that already holds a large term would each round at that
      // term's ulp, all in the same direction
      if (l != run_l) {
        if (run_l >= 0)
          for (int c = lane; c < k; c += 64) atomicAdd(G.dPi + (int64_t)run_l * k + c, run_a * qs[c]);
        run_l = l;
        run_a = 0.f;
      }
      run_a += alpha;
#pragma unroll
      for (int i = 0; i < ACF_JR; ++i) {
        const int j = lane + 64 * i;
        if (j < ha) {
          const float dp = prej[i] > 0.f ? dt * w1i[j] : 0.f;
          dpre[j] = dp;
          dui_r[i] += dp;
          dw1i_r[i] = fmaf(dt, fmaxf(prej[i], 0.f), dw1i_r[i]);
          if (dp != 0.f) atomicAdd(G.dGP + (int64_t)l * ha + j, dp);
        }
      }
      wave_sync();
      float bsum = 0.f;
      for (int m = lane; m < M; m += 64) {                   // dbeta_lm = Z_lm[h:] . dpre_l
        const float *z = Zl + (int64_t)m * NP + hc;
        float d = 0.f;
        for (int j = 0; j < ha; ++j) d = fmaf(z[j], dpre[j], d);
        const float bn = beta[m] * inv;
        beta[m] = bn;
        bsum = fmaf(bn, d, bsum);
        dbeta[m] = d;
      }
      bsum = wave_sum(bsum);
      for (int m = lane; m < M; m += 64) dbeta[m] = beta[m] * (dbeta[m] - bsum);      // ds_lm (the lane's own entries)
      wave_sync();
      float *dZl = G.dZ + (int64_t)l * M * NP;
      for (int m = 0; m < M; ++m) {                           // a lane per column
        const float ds = dbeta[m], bn = beta[m];
        const float *z = Zl + (int64_t)m * NP;
        float *dz = dZl + (int64_t)m * NP;
#pragma unroll
        for (int i = 0; i < ACF_JR; ++i) {
          const int j = lane + 64 * i;
          if (j < hc) {
            const float a = uc[j] + z[j];
            if (a > 0.f) {
              const float da = ds * w1c[j];
              atomicAdd(dz + j, da);
              duc_r[i] += da;
              dw1c_r[i] = fmaf(ds, a, dw1c_r[i]);
            }
          }
          if (j < ha) {
            const float v = bn * dpre[j];
            if (v != 0.f) atomicAdd(dz + hc + j, v);
          }
        }
      }
      wave_sync();                                             // beta / dbeta / dpre are rewritten by the next entry
    }
    if (run_l >= 0)
      for (int c = lane; c < k; c += 64) atomicAdd(G.dPi + (int64_t)run_l * k + c, run_a * qs[c]);
  }
#pragma unroll
  for (int i = 0; i < ACF_JR; ++i) {
    const int j = lane + 64 * i;
    if (j < hc) {
      red[(size_t)w * W2 + j] = duc_r[i];
      red[(size_t)w * W2 + hc + ha + j] = dw1c_r[i];
    }
    if (j < ha) {
      red[(size_t)w * W2 + hc + j] = dui_r[i];
      red[(size_t)w * W2 + 2 * hc + ha + j] = dw1i_r[i];
    }
  }
  __syncthreads();
  for (int e = tid; e < W2; e += 256) {
    const float v = (red[e] + red[(size_t)W2 + e]) + (red[2 * (size_t)W2 + e] + red[3 * (size_t)W2 + e]);
    fin[e] = v;
    G.UV[b * W2 + e] = v;
  }
  __syncthreads();
  for (int c = tid; c < k; c += 256) {
    float s = qs[c];
    for (int j = 0; j < hc; ++j) s = fmaf(A.wcu[(int64_t)c * hc + j], fin[j], s);
    for (int j = 0; j < ha; ++j) s = fmaf(A.wiu[(int64_t)c * ha + j], fin[hc + j], s);
    G.dGu[(int64_t)u * k + c] += s;
  }
}

// ---- users the model was not trained on (bprx_acf_fold_in) ------------------------------------------------------------
struct AcfFold {
  AcfUserArgs A;                      // Gu is not read (the rows are the caller's); ptr / items: the call's histories, by ROW
  const float *Gi;
  const int64_t *pptr;                // [n + 1] pairs of row r: [pptr[r], pptr[r + 1])
  const int32_t *pos, *neg;
  int steps, adam;
  float lr, reg, b1, b2, eps;
  float *Gu, *loss;                   // [n, k] in / out; [n] or nullptr
  int cache;                          // floats of LDS behind the fixed part (0: every pair is gathered every step)
};
constexpr int ACF_FOLD_EPL = ACF_MAX_K / 64;    // elements of a row per lane
constexpr int ACF_FOLD_EPT = ACF_MAX_K / 256;   // ... per thread

// One workgroup (4 waves) per new user r, resident across the steps (include/bprx.h, bprx_acf_fold_in).  Per step:
//   uc / ui from g; the forward walk of k_acf_user (wave w: entries w, w + 4, ...; online softmax per wave, merged) -> the item
//   softmax's max gm and denominator D, ap = sum_l alpha_l Pi_l;
//   the pairs (wave w: pairs w, w + 4, ...; D_p = Gi_i - Gi_j a lane-strided register row, from the cache area for the first nc
//   pairs after the first step): x_p = (g + ap).D_p, the wave's compensated sum of -s_p D_p and its loss terms; the four waves'
//   sums are added as (0 + 1) + (2 + 3) -> q;
//   the backward walk of k_acf_user_bwd over the entries, recomputing both levels, keeping only what reaches g: per-lane column
//   sums of dpre_l and da_lm in entry order, merged over the waves as (0 + 1) + (2 + 3);
//   grad = q + Wcu sum da + Wiu sum dpre + 2 reg n_r g, thread c owns g_c and its Adam slots.
// Nothing depends on another workgroup, on the cache size or on the grid; no atomics (but the error flag).
// LDS (floats): ls[4] (double) | g[k] ap[k] q[k] uc[h] ui[a] w1c[h] w1i[a] | per wave: beta[M] dbeta[M] dpre[a] acc[k] |
//               red[4][h + a] fin[h + a] wmx[4] wden[4] rb[4] | cache[nc][k]
__global__ __launch_bounds__(256) void k_acf_fold(AcfFold F) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const AcfUserArgs &A = F.A;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t r = blockIdx.x;
  const int64_t p0 = F.pptr[r], np64 = F.pptr[r + 1] - p0;
  if (np64 <= 0) {                                           // no pairs: the row stays, the loss is 0 (the whole workgroup leaves)
    if (tid == 0 && F.loss) F.loss[r] = 0.f;
    return;
  }
  const int np = np64 > INT32_MAX ? INT32_MAX : (int)np64;
  const int k = A.k, M = A.M, hc = A.hc, ha = A.ha, NP = A.NP, W = hc + ha;
  double *lsd = (double *)sm;
  float *g = sm + 8, *ap = g + k, *qs = ap + k, *uc = qs + k, *ui = uc + hc, *w1c = ui + ha, *w1i = w1c + hc;
  float *wbase = w1i + ha;
  const size_t wstride = 2 * (size_t)M + ha + k;
  float *beta = wbase + (size_t)w * wstride, *dbeta = beta + M, *dpre = dbeta + M, *acc = dpre + ha;
  float *red = wbase + 4 * wstride, *fin = red + 4 * (size_t)W, *wmx = fin + W, *wden = wmx + 4, *rb = wden + 4;
  float *cache = rb + 4;
  const int fit = F.cache / k, nc = np < fit ? np : fit;
  const int32_t *pos = F.pos + p0, *neg = F.neg + p0;
  const int64_t beg = A.ptr[r], end = A.ptr[r + 1];
  float gw[ACF_FOLD_EPT], am[ACF_FOLD_EPT], av[ACF_FOLD_EPT];
#pragma unroll
  for (int e = 0; e < ACF_FOLD_EPT; ++e) {
    const int c = tid + 256 * e;
    gw[e] = c < k ? F.Gu[r * k + c] : 0.f;
    am[e] = 0.f; av[e] = 0.f;
    if (c < k) g[c] = gw[e];
  }
  for (int j = tid; j < hc; j += 256) w1c[j] = A.w1c[j];
  for (int j = tid; j < ha; j += 256) w1i[j] = A.w1i[j];
  __syncthreads();
  const float bc1 = A.bc1[0], bi1 = A.bi1[0];
  const float r2n = 2.f * F.reg * (float)np, rn = F.reg * (float)np;
  for (int t = 1; t <= F.steps; ++t) {
    const bool last = t == F.steps && F.loss != nullptr;
    for (int j = tid; j < W; j += 256) {                       // W_0_u^T g + b_0 of both levels, as k_acf_user
      float s = 0.f;
      if (j < hc) {
        for (int c = 0; c < k; ++c) s = fmaf(g[c], A.wcu[(int64_t)c * hc + j], s);
        uc[j] = s + A.bc0[j];
      } else {
        const int jj = j - hc;
        for (int c = 0; c < k; ++c) s = fmaf(g[c], A.wiu[(int64_t)c * ha + jj], s);
        ui[jj] = s + A.bi0[jj];
      }
    }
    for (int c = lane; c < k; c += 64) acc[c] = 0.f;
    __syncthreads();
    // ---- forward over the history ----
    float prej[ACF_JR], inv;
    float mx = -INFINITY, den = 0.f;
    for (int64_t p = beg + w; p < end; p += 4) {
      const int l = clamp_index(A.items[p], A.I, A.errflag, 5);
      const float tl = acf_entry_fwd(A, l, uc, ui, w1c, w1i, bc1, bi1, beta, lane, inv, prej);
      const float nmx = fmaxf(mx, tl);
      const float sc = expf(mx - nmx), e = expf(tl - nmx);     // (mx = -inf at the first entry: sc = 0)
      den = den * sc + e;
      const float *pl = A.Pi + (int64_t)l * k;
      for (int c = lane; c < k; c += 64) acc[c] = acc[c] * sc + e * pl[c];
      mx = nmx;
      wave_sync();                                             // beta is rewritten by the next entry
    }
    if (lane == 0) { wmx[w] = mx; wden[w] = den; }
    __syncthreads();
    float gm = -INFINITY;
#pragma unroll
    for (int q = 0; q < 4; ++q) gm = fmaxf(gm, wmx[q]);
    float f[4], D = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      f[q] = wden[q] > 0.f ? expf(wmx[q] - gm) : 0.f;
      D += wden[q] * f[q];
    }
    for (int c = tid; c < k; c += 256) {
      float s = 0.f;
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (f[q] != 0.f) s += wbase[(size_t)q * wstride + 2 * M + ha + c] * f[q];
      ap[c] = D > 0.f ? s / D : 0.f;                           // sum_l alpha_l Pi_l
    }
    __syncthreads();
    // ---- the pairs ----
    {
      float qa[ACF_FOLD_EPL], qc[ACF_FOLD_EPL], gp[ACF_FOLD_EPL];      // -s_p D_p summed (Kahan) over this wave's pairs; g'
      double ls = 0.0;
#pragma unroll
      for (int e = 0; e < ACF_FOLD_EPL; ++e) {
        const int c = lane + 64 * e;
        qa[e] = 0.f; qc[e] = 0.f;
        gp[e] = c < k ? g[c] + ap[c] : 0.f;
      }
      for (int p = w; p < np; p += 4) {
        float d[ACF_FOLD_EPL], x = 0.f;
        if (p < nc && t > 1) {                                 // (a lane reads back what it wrote itself)
#pragma unroll
          for (int e = 0; e < ACF_FOLD_EPL; ++e) {
            const int c = lane + 64 * e;
            d[e] = c < k ? cache[(size_t)p * k + c] : 0.f;
          }
        } else {
          const int i = clamp_index(pos[p], A.I, A.errflag, 2), j = clamp_index(neg[p], A.I, A.errflag, 2);
          const float *gi = F.Gi + (int64_t)i * k, *gj = F.Gi + (int64_t)j * k;
#pragma unroll
          for (int e = 0; e < ACF_FOLD_EPL; ++e) {
            const int c = lane + 64 * e;
            d[e] = c < k ? gi[c] - gj[c] : 0.f;
            if (p < nc && c < k) cache[(size_t)p * k + c] = d[e];
          }
        }
#pragma unroll
        for (int e = 0; e < ACF_FOLD_EPL; ++e) x = fmaf(gp[e], d[e], x);
        const float diff = wave_sum(x);
        const bool inr = (diff >= -80.0f) && (diff <= 1e8f);             // tf.clip_by_value gradient mask
        const float z = -fminf(fmaxf(diff, -80.0f), 1e8f);
        ls += (double)(z > 0.f ? z + log1pf(expf(-z)) : log1pf(expf(z)));
        const float gd = inr ? -1.0f / (1.0f + expf(diff)) : 0.f;        // -s_p
#pragma unroll
        for (int e = 0; e < ACF_FOLD_EPL; ++e) {               // compensated: thousands of pairs pushing one way must not round
          const float y = gd * d[e] - qc[e];                   // every add at the ulp of the whole sum
          const float ts = qa[e] + y;
          qc[e] = (ts - qa[e]) - y;
          qa[e] = ts;
        }
      }
#pragma unroll
      for (int e = 0; e < ACF_FOLD_EPL; ++e) {
        const int c = lane + 64 * e;
        if (c < k) acc[c] = qa[e];
      }
      if (lane == 0) lsd[w] = ls;
    }
    __syncthreads();
    for (int c = tid; c < k; c += 256)
      qs[c] = (wbase[2 * M + ha + c] + wbase[wstride + 2 * M + ha + c]) +
              (wbase[2 * wstride + 2 * M + ha + c] + wbase[3 * wstride + 2 * M + ha + c]);
    __syncthreads();
    // ---- backward over the history ----
    {
      float pr = 0.f;
      for (int c = tid; c < k; c += 256) pr = fmaf(ap[c], qs[c], pr);
      pr = wave_sum(pr);
      if (lane == 0) rb[w] = pr;
    }
    __syncthreads();
    const float rbar = (rb[0] + rb[1]) + (rb[2] + rb[3]);      // sum_l alpha_l Pi_l . q
    float duc_r[ACF_JR], dui_r[ACF_JR];
#pragma unroll
    for (int i = 0; i < ACF_JR; ++i) duc_r[i] = dui_r[i] = 0.f;
    if (D > 0.f) {
      for (int64_t p = beg + w; p < end; p += 4) {
        const int l = clamp_index(A.items[p], A.I, A.errflag, 5);
        const float *Zl = A.Z + (int64_t)l * M * NP;
        const float tl = acf_entry_fwd(A, l, uc, ui, w1c, w1i, bc1, bi1, beta, lane, inv, prej);
        const float alpha = expf(tl - gm) / D;
        const float *pl = A.Pi + (int64_t)l * k;
        float rr = 0.f;
        for (int c = lane; c < k; c += 64) rr = fmaf(pl[c], qs[c], rr);
        rr = wave_sum(rr);
        const float dt = alpha * (rr - rbar);
#pragma unroll
        for (int i = 0; i < ACF_JR; ++i) {
          const int j = lane + 64 * i;
          if (j < ha) {
            const float dp = prej[i] > 0.f ? dt * w1i[j] : 0.f;
            dpre[j] = dp;
            dui_r[i] += dp;
          }
        }
        wave_sync();
        float bsum = 0.f;
        for (int m = lane; m < M; m += 64) {                   // dbeta_lm = Z_lm[h:] . dpre_l
          const float *z = Zl + (int64_t)m * NP + hc;
          float d = 0.f;
          for (int j = 0; j < ha; ++j) d = fmaf(z[j], dpre[j], d);
          const float bn = beta[m] * inv;
          beta[m] = bn;
          bsum = fmaf(bn, d, bsum);
          dbeta[m] = d;
        }
        bsum = wave_sum(bsum);
        for (int m = lane; m < M; m += 64) dbeta[m] = beta[m] * (dbeta[m] - bsum);      // ds_lm (the lane's own entries)
        wave_sync();
        for (int m = 0; m < M; ++m) {                           // a lane per column: sum_m da_lm
          const float ds = dbeta[m];
          const float *z = Zl + (int64_t)m * NP;
#pragma unroll
          for (int i = 0; i < ACF_JR; ++i) {
            const int j = lane + 64 * i;
            if (j < hc && uc[j] + z[j] > 0.f) duc_r[i] += ds * w1c[j];
          }
        }
        wave_sync();                                             // beta / dbeta / dpre are rewritten by the next entry
      }
    }
#pragma unroll
    for (int i = 0; i < ACF_JR; ++i) {
      const int j = lane + 64 * i;
      if (j < hc) red[(size_t)w * W + j] = duc_r[i];
      if (j < ha) red[(size_t)w * W + hc + j] = dui_r[i];
    }
    __syncthreads();
    for (int e = tid; e < W; e += 256) fin[e] = (red[e] + red[(size_t)W + e]) + (red[2 * (size_t)W + e] + red[3 * (size_t)W + e]);
    if (last && w == 0) {                                      // loss_T, before the last update
      float s = 0.f;
      for (int c = lane; c < k; c += 64) s = fmaf(g[c], g[c], s);
      s = wave_sum(s);
      if (lane == 0) F.loss[r] = (float)(((lsd[0] + lsd[1]) + (lsd[2] + lsd[3])) + (double)(rn * s));
    }
    __syncthreads();
    const float tt = (float)t;
    const float lr_t = F.adam ? F.lr * sqrtf(1.0f - powf(F.b2, tt)) / (1.0f - powf(F.b1, tt)) : F.lr;
#pragma unroll
    for (int e = 0; e < ACF_FOLD_EPT; ++e) {
      const int c = tid + 256 * e;
      if (c < k) {
        float s = qs[c];
        for (int j = 0; j < hc; ++j) s = fmaf(A.wcu[(int64_t)c * hc + j], fin[j], s);
        for (int j = 0; j < ha; ++j) s = fmaf(A.wiu[(int64_t)c * ha + j], fin[hc + j], s);
        const float gr = s + r2n * gw[e];
        if (F.adam) adam_elem(gw[e], am[e], av[e], gr, F.b1, F.b2, lr_t, F.eps);
        else gw[e] = gw[e] - lr_t * gr;
        g[c] = gw[e];
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int e = 0; e < ACF_FOLD_EPT; ++e) {
    const int c = tid + 256 * e;
    if (c < k) F.Gu[r * k + c] = gw[e];
  }
}

// dGi_l += Wiv dGP_l, dPi_l += Wip dGP_l: one wave per listed item (the row belongs to that wave alone in this kernel)
__global__ __launch_bounds__(256) void k_acf_item_bwd(const float *__restrict__ Wiv, const float *__restrict__ Wip,
                                                      const float *__restrict__ dGP, const int32_t *__restrict__ list,
                                                      const int32_t *__restrict__ nlist, int k, int ha, float *dGi, float *dPi) {
  __shared__ float dv[4][ACF_MAX_NP];
  const int n = *nlist, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int t = blockIdx.x * 4 + w; t < n; t += gridDim.x * 4) {
    const int64_t l = list[t];
    for (int j = lane; j < ha; j += 64) dv[w][j] = dGP[l * ha + j];
    wave_sync();
    for (int c = lane; c < k; c += 64) {
      float sv = 0.f, sp = 0.f;
      for (int j = 0; j < ha; ++j) {
        sv = fmaf(Wiv[(int64_t)c * ha + j], dv[w][j], sv);
        sp = fmaf(Wip[(int64_t)c * ha + j], dv[w][j], sp);
      }
      dGi[l * k + c] += sv;
      dPi[l * k + c] += sp;
    }
    wave_sync();
  }
}

// part[split][k][W] = sum over this split's rows r of R[ridx_r][:] (x) V[vidx_r][:].  Rows: the listed items (ridx = vidx = the
// item) or, with list == nullptr, the batch positions that own their user (ridx = user, vidx = position).  64 x 64 output tile
// per workgroup, 4 x 4 per thread, 16 rows per LDS stage.
struct AcfOuter {
  const float *R, *V;
  int ldv, W, k, U;
  int64_t B;
  const int32_t *user, *uslot, *list, *nlist;
};
__global__ __launch_bounds__(256) void k_acf_outer(AcfOuter O, float *__restrict__ part) {
  __shared__ float Rs[16][64], Vs[16][64];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int tilesj = (O.W + 63) / 64, tj = blockIdx.x % tilesj, tc = blockIdx.x / tilesj;
  const int64_t n = O.list ? (int64_t)*O.nlist : O.B;
  float acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
  for (int64_t r0 = (int64_t)blockIdx.y * 16; r0 < n; r0 += (int64_t)gridDim.y * 16) {
    for (int e = tid; e < 1024; e += 256) {
      const int rr = e >> 6, cc = e & 63;
      const int64_t r = r0 + rr;
      int64_t ridx = -1, vidx = -1;
      if (r < n) {
        if (O.list) {
          ridx = vidx = O.list[r];
        } else {
          int u = O.user[r];
          u = u < 0 ? 0 : (u >= O.U ? O.U - 1 : u);
          if (O.uslot[u] == (int32_t)r) { ridx = u; vidx = r; }
        }
      }
      const int c = tc * 64 + cc, j = tj * 64 + cc;
      Rs[rr][cc] = (ridx >= 0 && c < O.k) ? O.R[ridx * O.k + c] : 0.f;
      Vs[rr][cc] = (ridx >= 0 && j < O.W) ? O.V[vidx * O.ldv + j] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int rr = 0; rr < 16; ++rr) {
      float a[4], v[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) { a[i] = Rs[rr][ty * 4 + i]; v[i] = Vs[rr][tx * 4 + i]; }
#pragma unroll
      for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(a[i], v[j], acc[i][j]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = tc * 64 + ty * 4 + i;
    for (int j = 0; j < 4; ++j) {
      const int col = tj * 64 + tx * 4 + j;
      if (c < O.k && col < O.W) part[((int64_t)blockIdx.y * O.k + c) * O.W + col] = acc[i][j];
    }
  }
}

// part[split][W2] = column sums of the UV rows of this split's owner positions
__global__ __launch_bounds__(256) void k_acf_colsum(const float *__restrict__ UV, int W2, const int32_t *__restrict__ user,
                                                    const int32_t *__restrict__ uslot, int U, int64_t B, float *__restrict__ part) {
  for (int e = threadIdx.x; e < W2; e += 256) {
    float s = 0.f;
    for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
      int u = user[b];
      u = u < 0 ? 0 : (u >= U ? U - 1 : u);
      if (uslot[u] == (int32_t)b) s += UV[b * W2 + e];
    }
    part[(int64_t)blockIdx.x * W2 + e] = s;
  }
}

// out = sum_s part[s] in ascending s; element (c, j) of the [rows][ld] partial goes to out0[c][j] (j < w0) or out1[c][j - w0]
__global__ __launch_bounds__(256) void k_acf_reduce(const float *__restrict__ part, int nsplit, int64_t sstride, int rows, int ld,
                                                    float *__restrict__ out0, int w0, float *__restrict__ out1, int w1) {
  const int64_t n = (int64_t)rows * ld;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t c = e / ld;
    const int j = (int)(e - c * ld);
    if (j >= w0 + w1) continue;
    float s = 0.f;
    for (int q = 0; q < nsplit; ++q) s += part[(int64_t)q * sstride + e];
    if (j < w0) out0[c * w0 + j] = s;
    else out1[c * w1 + (j - w0)] = s;
  }
}

// ---- [dWci | dWix] = F^T dZ over the rows (l, m) of the listed items ---------------------------------------------------
// Workgroup (x, y, z): feature columns [128 x, 128 x + 128), K split y of gridDim.y (row chunks of 32: y, y + gridDim.y, ...),
// output column tiles [NB z, NB z + NB).  Wave w owns the 32 feature columns 128 x + 32 w.  part[y][Crows][NP].
__device__ __forceinline__ void acf_bwd_store(float *__restrict__ part, const f32x16 &acc, int64_t base, int NP, int col, int lane) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    part[(base + row) * NP + col + (lane & 31)] = acc[r];
  }
}

template <int NB>
__global__ __launch_bounds__(256) void k_acf_proj_bwd_f32(const float *__restrict__ F, const float *__restrict__ dZ,
                                                          float *__restrict__ part, const int32_t *__restrict__ list,
                                                          const int32_t *__restrict__ nlist, int M, int C, int NP, int Crows) {
  constexpr int LDA = 128 + 32, LDB = NB * 32 + 32;           // rows k and k + 1 of an operand pair fall into disjoint banks
  __shared__ __attribute__((aligned(16))) float As[32][LDA];
  __shared__ __attribute__((aligned(16))) float Bs[32][LDB];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int c0 = blockIdx.x * 128, col0 = blockIdx.z * NB * 32;
  const int nb = min(NB, NP / 32 - (int)blockIdx.z * NB);
  const int64_t nrows = (int64_t)*nlist * M, nchunks = (nrows + 31) / 32;
  f32x16 acc[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j)
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
  for (int64_t chunk = blockIdx.y; chunk < nchunks; chunk += gridDim.y) {
    const int64_t r0 = chunk * 32;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int idx = tid + 256 * q, row = idx >> 5, c4 = idx & 31;
      const int64_t gr = r0 + row;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      const int col = c0 + c4 * 4;
      if (gr < nrows && col < C) {
        const int64_t li = gr / M;
        v = *(const float4 *)(F + ((int64_t)list[li] * M + (gr - li * M)) * C + col);
      }
      *(float4 *)&As[row][c4 * 4] = v;
    }
#pragma unroll
    for (int q = 0; q < NB; ++q) {
      const int idx = tid + 256 * q, row = idx / (NB * 8), c4 = idx % (NB * 8);
      const int64_t gr = r0 + row;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      const int col = col0 + c4 * 4;
      if (gr < nrows && col < NP) {
        const int64_t li = gr / M;
        v = *(const float4 *)(dZ + ((int64_t)list[li] * M + (gr - li * M)) * NP + col);
      }
      *(float4 *)&Bs[row][c4 * 4] = v;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 32; kk += 2) {
      const float a = As[kk + (lane >> 5)][w * 32 + (lane & 31)];
#pragma unroll
      for (int j = 0; j < NB; ++j)
        if (j < nb) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, Bs[kk + (lane >> 5)][j * 32 + (lane & 31)], acc[j], 0, 0, 0);
    }
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < NB; ++j)
    if (j < nb) acf_bwd_store(part, acc[j], (int64_t)blockIdx.y * Crows + c0 + w * 32, NP, col0 + j * 32, lane);
}

// bf16 features: A = F^T (bf16, exact), B = dZ as three bf16 terms (24 bits: only the features are rounded), fp32 accumulation.
// Both operands are staged transposed ([column][row]) so that a lane reads its 8 consecutive K entries as one 16-byte word.
template <int NB>
__global__ __launch_bounds__(256) void k_acf_proj_bwd_bf16(const uint16_t *__restrict__ F, const float *__restrict__ dZ,
                                                           float *__restrict__ part, const int32_t *__restrict__ list,
                                                           const int32_t *__restrict__ nlist, int M, int C, int NP, int Crows) {
  __shared__ __attribute__((aligned(16))) uint16_t At[128][40];
  __shared__ __attribute__((aligned(16))) uint16_t Bh[NB * 32][40];
  __shared__ __attribute__((aligned(16))) uint16_t Bm[NB * 32][40];
  __shared__ __attribute__((aligned(16))) uint16_t Bl[NB * 32][40];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int c0 = blockIdx.x * 128, col0 = blockIdx.z * NB * 32;
  const int nb = min(NB, NP / 32 - (int)blockIdx.z * NB);
  const int64_t nrows = (int64_t)*nlist * M, nchunks = (nrows + 31) / 32;
  f32x16 acc[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j)
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
  for (int64_t chunk = blockIdx.y; chunk < nchunks; chunk += gridDim.y) {
    const int64_t r0 = chunk * 32;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int idx = tid + 256 * q, row = idx >> 4, c8 = idx & 15;
      const int64_t gr = r0 + row;
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      const int col = c0 + c8 * 8;
      if (gr < nrows && col < C) {
        const int64_t li = gr / M;
        v = *(const uint4 *)(F + ((int64_t)list[li] * M + (gr - li * M)) * C + col);
      }
      const uint32_t wd[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        At[c8 * 8 + 2 * i][row] = (uint16_t)(wd[i] & 0xffffu);
        At[c8 * 8 + 2 * i + 1][row] = (uint16_t)(wd[i] >> 16);
      }
    }
#pragma unroll
    for (int q = 0; q < NB; ++q) {
      const int idx = tid + 256 * q, row = idx / (NB * 8), c4 = idx % (NB * 8);
      const int64_t gr = r0 + row;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      const int col = col0 + c4 * 4;
      if (gr < nrows && col < NP) {
        const int64_t li = gr / M;
        v = *(const float4 *)(dZ + ((int64_t)list[li] * M + (gr - li * M)) * NP + col);
      }
      const float x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const uint16_t hi = (uint16_t)bf16_rne(x[i]);
        const float r1 = x[i] - __uint_as_float((uint32_t)hi << 16);
        const uint16_t mi = (uint16_t)bf16_rne(r1);
        const float r2 = r1 - __uint_as_float((uint32_t)mi << 16);
        Bh[c4 * 4 + i][row] = hi;
        Bm[c4 * 4 + i][row] = mi;
        Bl[c4 * 4 + i][row] = (uint16_t)bf16_rne(r2);
      }
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int ko = ks * 16 + 8 * (lane >> 5);
      const bf16x8 a = *(const bf16x8 *)&At[w * 32 + (lane & 31)][ko];
#pragma unroll
      for (int j = 0; j < NB; ++j)
        if (j < nb) {
          const bf16x8 bh = *(const bf16x8 *)&Bh[j * 32 + (lane & 31)][ko];
          const bf16x8 bm = *(const bf16x8 *)&Bm[j * 32 + (lane & 31)][ko];
          const bf16x8 bl = *(const bf16x8 *)&Bl[j * 32 + (lane & 31)][ko];
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, bl, acc[j], 0, 0, 0);
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, bm, acc[j], 0, 0, 0);
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, bh, acc[j], 0, 0, 0);
        }
    }
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < NB; ++j)
    if (j < nb) acf_bwd_store(part, acc[j], (int64_t)blockIdx.y * Crows + c0 + w * 32, NP, col0 + j * 32, lane);
}

// dZ and dGP rows of the listed items back to zero (both are all-zero between steps)
__global__ __launch_bounds__(256) void k_acf_clear(float *__restrict__ dZ, float *__restrict__ dGP, const int32_t *__restrict__ list,
                                                   const int32_t *__restrict__ nlist, int64_t zrow, int ha) {
  const int n = *nlist;
  for (int t = blockIdx.x; t < n; t += gridDim.x) {
    const int64_t l = list[t];
    float4 *z = (float4 *)(dZ + l * zrow);                     // zrow = M * NP, NP % 32 == 0
    for (int64_t e = threadIdx.x; e < zrow / 4; e += 256) z[e] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int j = threadIdx.x; j < ha; j += 256) dGP[l * ha + j] = 0.f;
  }
}

// sgd, full mode: the Gi / Pi rows of the listed history items move too (one wave per listed item, same claim marks)
__global__ __launch_bounds__(256) void k_acf_apply_sgd_list(float *Gi, float *Pi, float *dGi, float *dPi, uint32_t *flagI,
                                                            const int32_t *__restrict__ list, const int32_t *__restrict__ nlist,
                                                            int k, float lr) {
  const int n = *nlist, lane = threadIdx.x & 63;
  for (int t = blockIdx.x * 4 + (threadIdx.x >> 6); t < n; t += gridDim.x * 4) {
    const int64_t l = list[t];
    int claim = 0;
    if (lane == 0) claim = atomicExch(flagI + l, 1u) == 0u;
    claim = __shfl(claim, 0, 64);
    if (!claim) continue;
    for (int c = lane; c < k; c += 64) {
      Gi[l * k + c] -= lr * dGi[l * k + c]; dGi[l * k + c] = 0.f;
      Pi[l * k + c] -= lr * dPi[l * k + c]; dPi[l * k + c] = 0.f;
    }
  }
}
__global__ __launch_bounds__(256) void k_acf_finish_list(const int32_t *__restrict__ list, const int32_t *__restrict__ nlist,
                                                         uint32_t *flagI) {
  const int n = *nlist;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += gridDim.x * blockDim.x) flagI[list[e]] = 0u;
}

// ---- host side -------------------------------------------------------------------------------------------------------
static int acf_wcat(bprx_handle *h, hipStream_t s) {
  AcfState *S = h->acf;
  const bool bf = S->fdt == BPRX_F_BF16;
  hipLaunchKernelGGL(k_acf_wcat, dim3(bprx_blocks((int64_t)S->Cp * S->NP, 256, 2048)), dim3(256), 0, s, S->a.w[BPRX_ACF_C_WI],
                     S->a.w[BPRX_ACF_I_WX], S->C, S->Cp, S->hc, S->ha, S->NP, bf ? (float *)nullptr : S->Wc,
                     bf ? S->Wh : (uint16_t *)nullptr, bf ? S->Wl : (uint16_t *)nullptr);
  BPRX_LAUNCH_CHECK(h, "k_acf_wcat");
  return BPRX_OK;
}

// Z and GP of the listed items (list == nullptr: every item)
static int acf_project(bprx_handle *h, const int32_t *list, const int32_t *nlist, hipStream_t s) {
  AcfState *S = h->acf;
  const int I = h->cfg.num_items, NCT = S->NP / 32;
  const unsigned pg = bprx_blocks((int64_t)I * S->M, 64, (int64_t)h->num_cu * 4);
  {
    BprxProfScope ps(h, BPRX_PHASE_PROJ_FWD, s);
#define ACF_PROJ(N)                                                                                                           \
  case N:                                                                                                                     \
    if (S->fdt == BPRX_F_BF16)                                                                                                \
      hipLaunchKernelGGL(k_acf_proj_bf16<N>, dim3(pg), dim3(256), 0, s, (const uint16_t *)S->a.F, S->Wh, S->Wl, S->Z, list,    \
                         nlist, I, S->M, S->C, S->Cp);                                                                        \
    else                                                                                                                      \
      hipLaunchKernelGGL(k_acf_proj_f32<N>, dim3(pg), dim3(256), 0, s, (const float *)S->a.F, S->Wc, S->Z, list, nlist, I,     \
                         S->M, S->C, S->Cp);                                                                                  \
    break;
    switch (NCT) {
      ACF_PROJ(1) ACF_PROJ(2) ACF_PROJ(3) ACF_PROJ(4) ACF_PROJ(5) ACF_PROJ(6) ACF_PROJ(7) ACF_PROJ(8)
      default: BPRX_FAIL(h, BPRX_E_INVALID, "acf: h + a > %d", ACF_MAX_NP);
    }
#undef ACF_PROJ
    BPRX_LAUNCH_CHECK(h, "k_acf_proj");
  }
  hipLaunchKernelGGL(k_acf_itemvec, dim3(bprx_blocks(I, 4, 4096)), dim3(256), 0, s, h->t.Gi, S->a.Pi, S->a.w[BPRX_ACF_I_WV],
                     S->a.w[BPRX_ACF_I_WP], list, nlist, I, S->k, S->ha, S->GP);
  BPRX_LAUNCH_CHECK(h, "k_acf_itemvec");
  return BPRX_OK;
}

// Z / GP for the distinct items of the histories of users[0..n) (uslot: first positions only)
static int acf_prepare(bprx_handle *h, const int32_t *users, int64_t n, const int32_t *uslot, const int64_t *ptr,
                       const int32_t *items, hipStream_t s) {
  AcfState *S = h->acf;
  int rc;
  if ((rc = acf_wcat(h, s))) return rc;
  BPRX_HIP(h, hipMemsetAsync(S->nlist, 0, sizeof(int32_t), s));
  {
    BprxProfScope ps(h, BPRX_PHASE_ROW_COUNT, s);
    hipLaunchKernelGGL(k_acf_mark, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, users, n, uslot, ptr, items, h->cfg.num_users,
                       h->cfg.num_items, S->imark, S->ilist, S->nlist, h->errflag);
    BPRX_LAUNCH_CHECK(h, "k_acf_mark");
  }
  if ((rc = acf_project(h, S->ilist, S->nlist, s))) return rc;
  hipLaunchKernelGGL(k_acf_unmark, dim3(256), dim3(256), 0, s, S->ilist, S->nlist, S->imark);
  BPRX_LAUNCH_CHECK(h, "k_acf_unmark");
  return BPRX_OK;
}

static size_t acf_user_lds(const AcfState *S) {
  return sizeof(float) * ((size_t)S->k + 2 * (S->hc + S->ha) + 4 * (size_t)(S->M + S->k) + 8);
}

// Gu_rows: the user rows (nullptr: the handle's own Gu); with users == nullptr position b is row b of that table and of the CSR
static int acf_users(bprx_handle *h, const int32_t *users, int64_t n, const int32_t *uslot, const int64_t *ptr,
                     const int32_t *items, float *out, hipStream_t s, float *aux = nullptr, const float *Gu_rows = nullptr) {
  AcfState *S = h->acf;
  AcfUserArgs A;
  A.Gu = Gu_rows ? Gu_rows : h->t.Gu; A.Pi = S->a.Pi; A.Z = S->Z; A.GP = S->GP;
  A.wcu = S->a.w[BPRX_ACF_C_WU]; A.bc0 = S->a.w[BPRX_ACF_C_B0]; A.w1c = S->a.w[BPRX_ACF_C_W1]; A.bc1 = S->a.w[BPRX_ACF_C_B1];
  A.wiu = S->a.w[BPRX_ACF_I_WU]; A.bi0 = S->a.w[BPRX_ACF_I_B0]; A.w1i = S->a.w[BPRX_ACF_I_W1]; A.bi1 = S->a.w[BPRX_ACF_I_B1];
  A.ptr = ptr; A.items = items; A.errflag = h->errflag;
  A.U = h->cfg.num_users; A.I = h->cfg.num_items; A.k = S->k; A.M = S->M; A.hc = S->hc; A.ha = S->ha; A.NP = S->NP;
  BprxProfScope ps(h, BPRX_PHASE_TRIPLET, s);
  if (aux)
    hipLaunchKernelGGL(k_acf_user<ACF_USER_AUX>, dim3((unsigned)n), dim3(256), acf_user_lds(S), s, A, users, n, uslot, out, aux);
  else
    hipLaunchKernelGGL(k_acf_user<ACF_USER_PLAIN>, dim3((unsigned)n), dim3(256), acf_user_lds(S), s, A, users, n, uslot, out, aux);
  BPRX_LAUNCH_CHECK(h, "k_acf_user");
  return BPRX_OK;
}


static size_t acf_user_bwd_lds(const AcfState *S) {
  const size_t hw = (size_t)S->hc + S->ha;
  return sizeof(float) * (2 * (size_t)S->k + 2 * hw + 4 * (2 * (size_t)S->M + S->ha) + 5 * 2 * hw + 4);
}

static int acf_reduce(bprx_handle *h, int nsplit, int64_t sstride, int rows, int ld, float *out0, int w0, float *out1, int w1,
                      hipStream_t s) {
  hipLaunchKernelGGL(k_acf_reduce, dim3(bprx_blocks((int64_t)rows * ld, 256, 1024)), dim3(256), 0, s, h->acf->part, nsplit, sstride,
                     rows, ld, out0, w0, out1, w1);
  BPRX_LAUNCH_CHECK(h, "k_acf_reduce");
  return BPRX_OK;
}

#define ACF_SPLIT 64                                         // K splits of k_acf_outer / k_acf_colsum

// The gradient through g'_u (include/bprx.h, BPRX_ACF_GRAD_FULL): after k_acf_triplet, before k_acf_dense
static int acf_backward(bprx_handle *h, const AcfStepArgs &A, const int32_t *user, const int32_t *pos, const int32_t *neg, int64_t B,
                        hipStream_t s) {
  AcfState *S = h->acf;
  const int U = h->cfg.num_users, I = h->cfg.num_items, k = S->k, hc = S->hc, ha = S->ha, W = hc + ha, W2 = 2 * W;
  int rc;
  BPRX_HIP(h, hipMemsetAsync(S->q, 0, (size_t)B * k * sizeof(float), s));
  {
    BprxProfScope ps(h, BPRX_PHASE_REDUCE, s);
    hipLaunchKernelGGL(k_acf_q, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, s, A, user, pos, neg, B, S->q);
    BPRX_LAUNCH_CHECK(h, "k_acf_q");
    AcfUserArgs UA;
    UA.Gu = h->t.Gu; UA.Pi = S->a.Pi; UA.Z = S->Z; UA.GP = S->GP;
    UA.wcu = S->a.w[BPRX_ACF_C_WU]; UA.bc0 = S->a.w[BPRX_ACF_C_B0]; UA.w1c = S->a.w[BPRX_ACF_C_W1]; UA.bc1 = S->a.w[BPRX_ACF_C_B1];
    UA.wiu = S->a.w[BPRX_ACF_I_WU]; UA.bi0 = S->a.w[BPRX_ACF_I_B0]; UA.w1i = S->a.w[BPRX_ACF_I_W1]; UA.bi1 = S->a.w[BPRX_ACF_I_B1];
    UA.ptr = S->a.train_ptr; UA.items = S->a.train_items; UA.errflag = h->errflag;
    UA.U = U; UA.I = I; UA.k = k; UA.M = S->M; UA.hc = hc; UA.ha = ha; UA.NP = S->NP;
    AcfBwdArgs G;
    G.q = S->q; G.aux = S->aux; G.dZ = S->dZ; G.dGP = S->dGP; G.dPi = S->dPi; G.dGu = h->dGu; G.UV = S->UV;
    hipLaunchKernelGGL(k_acf_user_bwd, dim3((unsigned)B), dim3(256), acf_user_bwd_lds(S), s, UA, G, user, B, S->uslot);
    BPRX_LAUNCH_CHECK(h, "k_acf_user_bwd");
  }
  {
    BprxProfScope ps(h, BPRX_PHASE_LOSS, s);
    hipLaunchKernelGGL(k_acf_item_bwd, dim3(bprx_blocks(I, 4, 4096)), dim3(256), 0, s, S->a.w[BPRX_ACF_I_WV], S->a.w[BPRX_ACF_I_WP],
                       S->dGP, S->ilist, S->nlist, k, ha, h->dGi, S->dPi);
    BPRX_LAUNCH_CHECK(h, "k_acf_item_bwd");
    // dWiv = sum_l Gi_l (x) dGP_l, dWip = sum_l Pi_l (x) dGP_l over the listed items
    AcfOuter O;
    O.V = S->dGP; O.ldv = ha; O.W = ha; O.k = k; O.U = U; O.B = B; O.user = user; O.uslot = S->uslot; O.list = S->ilist;
    O.nlist = S->nlist;
    const int isplit = (int)bprx_blocks(I, 16, ACF_SPLIT);
    const dim3 gi((unsigned)(((k + 63) / 64) * ((ha + 63) / 64)), (unsigned)isplit);
    const float *R[2] = {h->t.Gi, S->a.Pi};
    float *out[2] = {S->gw[BPRX_ACF_I_WV], S->gw[BPRX_ACF_I_WP]};
    for (int t = 0; t < 2; ++t) {
      O.R = R[t];
      hipLaunchKernelGGL(k_acf_outer, gi, dim3(256), 0, s, O, S->part);
      BPRX_LAUNCH_CHECK(h, "k_acf_outer");
      if ((rc = acf_reduce(h, isplit, (int64_t)k * ha, k, ha, out[t], ha, nullptr, 0, s))) return rc;
    }
    // [dWcu | dWiu] = sum_u g_u (x) [duc_u | dui_u] over the distinct users
    O.R = h->t.Gu; O.V = S->UV; O.ldv = W2; O.W = W; O.list = nullptr; O.nlist = nullptr;
    const int usplit = (int)bprx_blocks(B, 16, ACF_SPLIT);
    hipLaunchKernelGGL(k_acf_outer, dim3((unsigned)(((k + 63) / 64) * ((W + 63) / 64)), (unsigned)usplit), dim3(256), 0, s, O, S->part);
    BPRX_LAUNCH_CHECK(h, "k_acf_outer");
    if ((rc = acf_reduce(h, usplit, (int64_t)k * W, k, W, S->gw[BPRX_ACF_C_WU], hc, S->gw[BPRX_ACF_I_WU], ha, s))) return rc;
    // [dbc0 | dbi0 | dW1c | dW1i] = column sums of the users' rows (gw[C_B0] is the head of that block)
    hipLaunchKernelGGL(k_acf_colsum, dim3((unsigned)usplit), dim3(256), 0, s, S->UV, W2, user, S->uslot, U, B, S->part);
    BPRX_LAUNCH_CHECK(h, "k_acf_colsum");
    if ((rc = acf_reduce(h, usplit, W2, 1, W2, S->gw[BPRX_ACF_C_B0], W2, nullptr, 0, s))) return rc;
  }
  {
    BprxProfScope ps(h, BPRX_PHASE_PROJ_BWD, s);
    const int NCT = S->NP / 32, nb = NCT < 4 ? NCT : 4, ctiles = (S->C + 127) / 128, Crows = ctiles * 128;
    const dim3 g((unsigned)ctiles, (unsigned)S->nsplit_proj, (unsigned)((NCT + nb - 1) / nb));
#define ACF_PROJ_BWD(N)                                                                                                       \
  case N:                                                                                                                     \
    if (S->fdt == BPRX_F_BF16)                                                                                                \
      hipLaunchKernelGGL(k_acf_proj_bwd_bf16<N>, g, dim3(256), 0, s, (const uint16_t *)S->a.F, S->dZ, S->part, S->ilist,       \
                         S->nlist, S->M, S->C, S->NP, Crows);                                                                 \
    else                                                                                                                      \
      hipLaunchKernelGGL(k_acf_proj_bwd_f32<N>, g, dim3(256), 0, s, (const float *)S->a.F, S->dZ, S->part, S->ilist, S->nlist, \
                         S->M, S->C, S->NP, Crows);                                                                           \
    break;
    switch (nb) { ACF_PROJ_BWD(1) ACF_PROJ_BWD(2) ACF_PROJ_BWD(3) ACF_PROJ_BWD(4) }
#undef ACF_PROJ_BWD
    BPRX_LAUNCH_CHECK(h, "k_acf_proj_bwd");
    if ((rc = acf_reduce(h, S->nsplit_proj, (int64_t)Crows * S->NP, S->C, S->NP, S->gw[BPRX_ACF_C_WI], hc, S->gw[BPRX_ACF_I_WX], ha, s)))
      return rc;
    hipLaunchKernelGGL(k_acf_clear, dim3(bprx_blocks(I, 1, 8192)), dim3(256), 0, s, S->dZ, S->dGP, S->ilist, S->nlist,
                       (int64_t)S->M * S->NP, ha);
    BPRX_LAUNCH_CHECK(h, "k_acf_clear");
  }
  return BPRX_OK;
}

int bprx_acf_step(bprx_handle *h, const int32_t *user, const int32_t *pos, const int32_t *neg, int64_t B, float *loss_out,
                  hipStream_t s) {
  AcfState *S = h->acf;
  if (B <= 0) BPRX_FAIL(h, BPRX_E_INVALID, "step: empty batch");
  if (!user || !pos || !neg) BPRX_FAIL(h, BPRX_E_INVALID, "step: null index pointer");
  const int U = h->cfg.num_users, I = h->cfg.num_items, k = S->k;
  const bool adam = h->cfg.optimizer == BPRX_OPT_ADAM_TF23;
  float lr_t = h->cfg.lr;
  if (adam) {
    h->adam_t += 1;
    lr_t = bprx_adam_lr_t(h);
  }
  h->step.lr_t = lr_t;                                     // (bprx_step_lr)
  int rc;
  hipLaunchKernelGGL(k_acf_claim, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, user, B, U, S->uslot, h->errflag);
  BPRX_LAUNCH_CHECK(h, "k_acf_claim");
  if ((rc = acf_prepare(h, user, B, S->uslot, S->a.train_ptr, S->a.train_items, s))) return rc;
  const bool full = S->grad_mode == BPRX_ACF_GRAD_FULL;
  if ((rc = acf_users(h, user, B, S->uslot, S->a.train_ptr, S->a.train_items, S->gp, s, full ? S->aux : nullptr))) return rc;
  AcfStepArgs A;
  A.Gu = h->t.Gu; A.Gi = h->t.Gi; A.Pi = S->a.Pi; A.gp = S->gp;
  A.dGu = h->dGu; A.dGi = h->dGi; A.dPi = S->dPi; A.lossb = h->lossb;
  A.uslot = S->uslot; A.errflag = h->errflag; A.U = U; A.I = I; A.k = k; A.reg = h->cfg.reg;
  {
    BprxProfScope ps(h, BPRX_PHASE_ITEM_SEG, s);
    hipLaunchKernelGGL(k_acf_triplet, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, s, A, user, pos, neg, B);
    BPRX_LAUNCH_CHECK(h, "k_acf_triplet");
  }
  if (full && (rc = acf_backward(h, A, user, pos, neg, B, s))) return rc;
  {
    BprxProfScope ps(h, BPRX_PHASE_DENSE, s);
    AcfDenseArgs T;
    for (int q = 0; q < BPRX_ACF_NW; ++q) {
      T.w[q] = S->a.w[q]; T.m[q] = S->a.m_w[q]; T.v[q] = S->a.v_w[q]; T.n[q] = S->nw[q];
      T.g[q] = full ? S->gw[q] : nullptr;
    }
    hipLaunchKernelGGL(k_acf_dense, dim3(1), dim3(1024), 0, s, T, adam ? 1 : 0, lr_t, h->cfg.reg, h->cfg.beta1, h->cfg.beta2,
                       h->cfg.epsilon, h->lossb, B, loss_out);
    BPRX_LAUNCH_CHECK(h, "k_acf_dense");
  }
  {
    BprxProfScope ps(h, BPRX_PHASE_APPLY, s);
    if (adam) {
      // every row of Gu, Gi, Pi moves every step (ACF.py:266-268)
      AdamSweepAll W = {};
      W.seg[0] = {h->t.Gu, h->t.m_Gu, h->t.v_Gu, h->dGu, (size_t)U * k};
      W.seg[1] = {h->t.Gi, h->t.m_Gi, h->t.v_Gi, h->dGi, (size_t)I * k};
      W.seg[2] = {S->a.Pi, S->a.m_Pi, S->a.v_Pi, S->dPi, (size_t)I * k};
      if ((rc = bprx_launch_adam_sweep(h, W, lr_t, s))) return rc;
    } else {
      hipLaunchKernelGGL(k_acf_apply_sgd, dim3((unsigned)((3 * B + 3) / 4)), dim3(256), 0, s, h->t.Gu, h->t.Gi, S->a.Pi, h->dGu,
                         h->dGi, S->dPi, h->flagU, h->flagI, user, pos, neg, B, U, I, k, lr_t);
      BPRX_LAUNCH_CHECK(h, "k_acf_apply_sgd");
      if (full) {
        hipLaunchKernelGGL(k_acf_apply_sgd_list, dim3(bprx_blocks(I, 4, 4096)), dim3(256), 0, s, h->t.Gi, S->a.Pi, h->dGi, S->dPi,
                           h->flagI, S->ilist, S->nlist, k, lr_t);
        BPRX_LAUNCH_CHECK(h, "k_acf_apply_sgd_list");
      }
    }
  }
  if (full && !adam) {
    hipLaunchKernelGGL(k_acf_finish_list, dim3(bprx_blocks(I, 256, 1024)), dim3(256), 0, s, S->ilist, S->nlist, h->flagI);
    BPRX_LAUNCH_CHECK(h, "k_acf_finish_list");
  }
  hipLaunchKernelGGL(k_acf_finish, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, user, pos, neg, B, U, I, S->uslot, h->flagU,
                     h->flagI);
  BPRX_LAUNCH_CHECK(h, "k_acf_finish");
  S->eval_valid = false;
  return BPRX_OK;
}

int bprx_acf_score_pairs(bprx_handle *h, const int32_t *u, const int32_t *i, int64_t B, float *x, hipStream_t s) {
  AcfState *S = h->acf;
  int rc;
  if ((rc = acf_prepare(h, u, B, nullptr, S->a.train_ptr, S->a.train_items, s))) return rc;
  if ((rc = acf_users(h, u, B, nullptr, S->a.train_ptr, S->a.train_items, S->gp, s))) return rc;
  hipLaunchKernelGGL(k_acf_score, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, s, S->gp, h->t.Gi, i, B, h->cfg.num_items, S->k, x,
                     h->errflag);
  BPRX_LAUNCH_CHECK(h, "k_acf_score");
  return BPRX_OK;
}

int bprx_acf_eval_profiles(bprx_handle *h, hipStream_t s) {
  AcfState *S = h->acf;
  if (S->eval_valid) return BPRX_OK;
  int rc;
  if ((rc = acf_wcat(h, s))) return rc;
  if ((rc = acf_project(h, nullptr, nullptr, s))) return rc;
  const int64_t *ptr = S->a.eval_ptr ? S->a.eval_ptr : S->a.train_ptr;
  const int32_t *items = S->a.eval_ptr ? S->a.eval_items : S->a.train_items;
  if ((rc = acf_users(h, nullptr, h->cfg.num_users, nullptr, ptr, items, S->Gup, s))) return rc;
  S->eval_valid = true;
  return BPRX_OK;
}

float *bprx_acf_eval_gu(bprx_handle *h) { return h->acf->Gup; }

void bprx_acf_invalidate(bprx_handle *h) {
  if (h->acf) h->acf->eval_valid = false;
}

void bprx_acf_free(bprx_handle *h) {
  delete h->acf;
  h->acf = nullptr;
}

int bprx_bind_tables_internal(bprx_handle *h, const bprx_tables *t);

extern "C" int bprx_bind_acf(bprx_handle *h, const bprx_tables *t, const bprx_acf *a) {
  if (!h || !t || !a) return BPRX_E_INVALID;
  const bprx_config &c = h->cfg;
  if (c.model != BPRX_MODEL_BPRMF) BPRX_FAIL(h, BPRX_E_INVALID, "bind_acf: needs a BPRMF handle");
  if (c.flags & (BPRX_FLAG_EXPORT_USER_GRAD | BPRX_FLAG_EXPORT_ITEM_GRAD))
    BPRX_FAIL(h, BPRX_E_INVALID, "bind_acf: exported gradients (multi-GPU) are not supported");
  if (a->feat_dtype != BPRX_F_FP32 && a->feat_dtype != BPRX_F_BF16)
    BPRX_FAIL(h, BPRX_E_INVALID, "bind_acf: features must be fp32 or bf16 (feat_dtype %d)", a->feat_dtype);
  if (a->feat_m <= 0 || a->feat_m > ACF_MAX_M) BPRX_FAIL(h, BPRX_E_INVALID, "bind_acf: M = %d outside [1, %d]", a->feat_m, ACF_MAX_M);
  if (a->feat_c <= 0 || a->feat_c % (a->feat_dtype == BPRX_F_BF16 ? 8 : 4))
    BPRX_FAIL(h, BPRX_E_INVALID, "bind_acf: C = %d must be a positive multiple of %d", a->feat_c, a->feat_dtype == BPRX_F_BF16 ? 8 : 4);
  if (a->width_c <= 0 || a->width_i <= 0 || a->width_c + a->width_i > ACF_MAX_NP)
    BPRX_FAIL(h, BPRX_E_INVALID, "bind_acf: need h, a > 0 and h + a <= %d (%d, %d)", ACF_MAX_NP, a->width_c, a->width_i);
  if (c.embed_k > ACF_MAX_K) BPRX_FAIL(h, BPRX_E_INVALID, "bind_acf: embed_k %d > %d", c.embed_k, ACF_MAX_K);
  if (!a->F || !a->train_ptr || !a->train_items || !a->Pi) BPRX_FAIL(h, BPRX_E_INVALID, "bind_acf: F, train CSR and Pi are required");
  if ((uintptr_t)a->F & 15) BPRX_FAIL(h, BPRX_E_INVALID, "bind_acf: F must be 16-byte aligned");
  if (!a->eval_ptr != !a->eval_items) BPRX_FAIL(h, BPRX_E_INVALID, "bind_acf: eval_ptr and eval_items go together");
  const bool adam = c.optimizer == BPRX_OPT_ADAM_TF23;
  for (int q = 0; q < BPRX_ACF_NW; ++q) {
    if (!a->w[q]) BPRX_FAIL(h, BPRX_E_INVALID, "bind_acf: attention tensor %d is missing", q);
    if (adam && (!a->m_w[q] || !a->v_w[q])) BPRX_FAIL(h, BPRX_E_INVALID, "bind_acf: adam_tf23 needs m_/v_ slots of tensor %d", q);
  }
  if (adam && (!a->m_Pi || !a->v_Pi)) BPRX_FAIL(h, BPRX_E_INVALID, "bind_acf: adam_tf23 needs m_/v_ slots for Pi");
  AcfState *S = h->acf;
  const int NP = 32 * ((a->width_c + a->width_i + 31) / 32);
  if (S && (S->M != a->feat_m || S->C != a->feat_c || S->hc != a->width_c || S->ha != a->width_i || S->fdt != a->feat_dtype))
    bprx_acf_free(h), S = nullptr;
  if (h->af) bprx_af_free(h);                               // the handle stops being an AttentiveFashion handle
  int rc = bprx_bind_tables_internal(h, t);
  if (rc) return rc;
  // TF-2.3's Adam moves every row every step: an ACF handle takes the whole-table sweeps (bring lazily held rows up to date first)
  if (h->adam_lazy) {
    if ((rc = bprx_launch_adam_sync(h, h->adam_t, nullptr))) return rc;
    BPRX_HIP(h, hipStreamSynchronize(nullptr));
    h->adam_lazy = false;
  }
  const size_t U = c.num_users, I = c.num_items, k = c.embed_k, MB = c.max_batch;
  if (!S) {
    S = new (std::nothrow) AcfState();
    if (!S) BPRX_FAIL(h, BPRX_E_NOMEM, "bind_acf: out of host memory");
    h->acf = S;
    S->M = a->feat_m; S->C = a->feat_c; S->hc = a->width_c; S->ha = a->width_i; S->NP = NP; S->k = (int)k; S->fdt = a->feat_dtype;
    S->Cp = (S->C + 31) / 32 * 32;
    DevPool &A = S->mem;
    A.zeros(&S->Z, I * S->M * NP);
    A.zeros(&S->GP, I * S->ha);
    if (S->fdt == BPRX_F_BF16) {
      A.zeros(&S->Wh, (size_t)S->Cp * NP);
      A.zeros(&S->Wl, (size_t)S->Cp * NP);
    } else {
      A.zeros(&S->Wc, (size_t)S->Cp * NP);
    }
    A.zeros(&S->gp, MB * k);
    A.zeros(&S->Gup, U * k);
    A.zeros(&S->dPi, I * k);
    A.zeros(&S->uslot, U);
    A.zeros(&S->imark, I);
    A.zeros(&S->ilist, I);
    A.zeros(&S->nlist, (size_t)1);
    if (!A.ok()) {
      bprx_acf_free(h);
      BPRX_FAIL(h, BPRX_E_NOMEM, "bind_acf: scratch allocation failed (Z: %zu MB)", (I * a->feat_m * NP * 4) >> 20);
    }
    if ((rc = bprx_launch_fill_i32(h, S->uslot, U, (int32_t)INT_MAX, nullptr))) {
      bprx_acf_free(h);
      return rc;
    }
    if (acf_user_lds(S) > 65536) {
      bprx_acf_free(h);
      BPRX_FAIL(h, BPRX_E_INVALID, "bind_acf: M = %d with embed_k = %d needs more LDS than a workgroup has", a->feat_m, (int)k);
    }
  }
  S->a = *a;
  S->grad_mode = BPRX_ACF_GRAD_DETACHED;                     // every bind starts with the reference's step
  const int64_t hc = S->hc, ha = S->ha, C = S->C;
  const int64_t nw[BPRX_ACF_NW] = {(int64_t)k * hc, C * hc, hc, hc, 1, (int64_t)k * ha, (int64_t)k * ha, (int64_t)k * ha, C * ha, ha, ha, 1};
  for (int q = 0; q < BPRX_ACF_NW; ++q) S->nw[q] = nw[q];
  S->eval_valid = false;
  const hipError_t e = hipStreamSynchronize(nullptr);
  if (e == hipSuccess) return BPRX_OK;
  bprx_acf_free(h);                                          // no failure leaves a model state on the handle
  BPRX_FAIL(h, BPRX_E_HIP, "bind_acf: hipStreamSynchronize(nullptr): %s", hipGetErrorString(e));
}

extern "C" int bprx_acf_profiles(bprx_handle *h, const int32_t *users, int64_t n, const int64_t *hist_ptr, const int32_t *hist_items,
                                 float *out, void *stream) {
  if (!h) return BPRX_E_INVALID;
  if (!h->bound || !h->acf) BPRX_FAIL(h, BPRX_E_STATE, "acf_profiles: the handle is not bound with bprx_bind_acf");
  if (n < 0 || n > ((int64_t)1 << 31) - 1) BPRX_FAIL(h, BPRX_E_INVALID, "acf_profiles: n = %lld out of range", (long long)n);
  if (n == 0) return BPRX_OK;
  if (!users || !hist_ptr || !hist_items || !out) BPRX_FAIL(h, BPRX_E_INVALID, "acf_profiles: null pointer");
  hipStream_t s = (hipStream_t)stream;
  int rc;
  if ((rc = acf_prepare(h, users, n, nullptr, hist_ptr, hist_items, s))) return rc;
  return acf_users(h, users, n, nullptr, hist_ptr, hist_items, out, s);
}

// ---- caller-owned rows: users folded in by bprx_acf_fold_in (include/bprx.h) -------------------------------------------------
static int acf_rows_args(bprx_handle *h, const char *what, int64_t n) {
  if (n < 0 || n >= ((int64_t)1 << 31)) BPRX_FAIL(h, BPRX_E_INVALID, "%s: n = %lld out of range", what, (long long)n);
  return BPRX_OK;
}

extern "C" int bprx_acf_profile_rows(bprx_handle *h, const float *Gu_rows, int64_t n, const int64_t *hist_ptr,
                                     const int32_t *hist_items, float *out, void *stream) {
  if (!h) return BPRX_E_INVALID;
  int rc;
  if ((rc = acf_rows_args(h, "acf_profile_rows", n))) return rc;
  if (!hist_ptr || (n && (!Gu_rows || !hist_items || !out))) BPRX_FAIL(h, BPRX_E_INVALID, "acf_profile_rows: null pointer");
  hipStream_t s = (hipStream_t)stream;
  rc = bprx_enter(h, "acf_profile_rows", NEED_BOUND, KIND_ACF, s);
  if (rc || n == 0) return rc;
  if ((rc = acf_prepare(h, nullptr, n, nullptr, hist_ptr, hist_items, s))) return rc;
  return acf_users(h, nullptr, n, nullptr, hist_ptr, hist_items, out, s, nullptr, Gu_rows);
}

int bprx_acf_row_profiles(bprx_handle *h, const float *Gu_rows, int64_t r0, int64_t r1, const int64_t *hist_ptr,
                          const int32_t *hist_items, float **gp, hipStream_t s) {
  AcfState *S = h->acf;
  const int64_t n = r1 - r0;
  float *ws = S->gp;
  if (n > h->cfg.max_batch) {
    if (n > S->prow_cap) {
      BPRX_HIP(h, hipStreamSynchronize(s));                    // (an earlier call's score kernel on this stream may still read the old buffer)
      S->prow_cap = 0;
      if (S->mem.regrow(&S->prow, (size_t)n * S->k) != hipSuccess)
        BPRX_FAIL(h, BPRX_E_NOMEM, "acf_score_rows_block: workspace allocation failed (%zu MB)", ((size_t)n * S->k * 4) >> 20);
      S->prow_cap = n;
    }
    ws = S->prow;
  }
  int rc;
  if ((rc = acf_prepare(h, nullptr, n, nullptr, hist_ptr + r0, hist_items, s))) return rc;
  if ((rc = acf_users(h, nullptr, n, nullptr, hist_ptr + r0, hist_items, ws, s, nullptr, Gu_rows + r0 * S->k))) return rc;
  *gp = ws;
  return BPRX_OK;
}

// LDS of a k_acf_fold workgroup: what the walk needs, and behind it the cached pair differences.  Where the fixed part leaves
// room the total is 40 KB, the budget of bprx_fold_in and bprx_af_fold_in.  The kernel's 162 VGPRs let three workgroups share a CU,
// so up to 53 KB would cost no occupancy; the cache is not what binds (all 80 pairs of a user against 60: BPRX_FOLD_CACHE=0 costs
// 2.6 % at the measured shape), and a larger budget has not been measured.
constexpr size_t ACF_FOLD_LDS = 40 * 1024;
static size_t acf_fold_fixed(const AcfState *S) {
  const size_t hw = (size_t)S->hc + S->ha;
  return sizeof(float) * (20 + 3 * (size_t)S->k + 7 * hw + 4 * (2 * (size_t)S->M + S->ha + S->k));
}

extern "C" int bprx_acf_fold_in(bprx_handle *h, const int64_t *hist_ptr, const int32_t *hist_items, const int64_t *pair_ptr,
                                const int32_t *pos, const int32_t *neg, int64_t n, int32_t steps, float lr, float reg,
                                int32_t optimizer, float *Gu_rows, float *loss, void *stream) {
  if (!h) return BPRX_E_INVALID;
  int rc;
  if ((rc = fold_check_args(h, "acf_fold_in", n, steps, optimizer))) return rc;
  if (!hist_ptr || !pair_ptr || !Gu_rows) BPRX_FAIL(h, BPRX_E_INVALID, "acf_fold_in: null pointer");
  if (n && (!hist_items || !pos || !neg)) BPRX_FAIL(h, BPRX_E_INVALID, "acf_fold_in: null pointer");
  hipStream_t s = (hipStream_t)stream;
  rc = bprx_enter(h, "acf_fold_in", NEED_BOUND, KIND_ACF, s);
  if (rc) return rc;
  AcfState *S = h->acf;
  const size_t fixed = acf_fold_fixed(S);
  if (fixed > 65536)
    BPRX_FAIL(h, BPRX_E_INVALID, "acf_fold_in: M = %d, embed_k = %d, h = %d, a = %d need %zu bytes of LDS, more than a workgroup has",
              S->M, S->k, S->hc, S->ha, fixed);
  if (n == 0) return BPRX_OK;
  if ((rc = acf_prepare(h, nullptr, n, nullptr, hist_ptr, hist_items, s))) return rc;   // Z / GP of the distinct history items
  const bprx_config &c = h->cfg;
  AcfFold F;
  AcfUserArgs &A = F.A;
  A.Gu = nullptr; A.Pi = S->a.Pi; A.Z = S->Z; A.GP = S->GP;
  A.wcu = S->a.w[BPRX_ACF_C_WU]; A.bc0 = S->a.w[BPRX_ACF_C_B0]; A.w1c = S->a.w[BPRX_ACF_C_W1]; A.bc1 = S->a.w[BPRX_ACF_C_B1];
  A.wiu = S->a.w[BPRX_ACF_I_WU]; A.bi0 = S->a.w[BPRX_ACF_I_B0]; A.w1i = S->a.w[BPRX_ACF_I_W1]; A.bi1 = S->a.w[BPRX_ACF_I_B1];
  A.ptr = hist_ptr; A.items = hist_items; A.errflag = h->errflag;
  A.U = c.num_users; A.I = c.num_items; A.k = S->k; A.M = S->M; A.hc = S->hc; A.ha = S->ha; A.NP = S->NP;
  F.Gi = h->t.Gi; F.pptr = pair_ptr; F.pos = pos; F.neg = neg;
  F.steps = steps; F.adam = optimizer == BPRX_OPT_ADAM_TF23;
  F.lr = lr; F.reg = reg; F.b1 = c.beta1; F.b2 = c.beta2; F.eps = c.epsilon;
  F.Gu = Gu_rows; F.loss = loss;
  const size_t total = fixed > ACF_FOLD_LDS ? fixed : ACF_FOLD_LDS;
  F.cache = h->fold_cache ? (int)((total - fixed) / sizeof(float)) : 0;
  BprxProfScope ps(h, BPRX_PHASE_TRIPLET, s);
  hipLaunchKernelGGL(k_acf_fold, dim3((unsigned)n), dim3(256), fixed + (size_t)F.cache * sizeof(float), s, F);
  BPRX_LAUNCH_CHECK(h, "k_acf_fold");
  return BPRX_OK;
}

// Workspace of the full-gradient mode, allocated at the first switch to it (a detached handle never pays for it)
static int acf_full_alloc(bprx_handle *h) {
  AcfState *S = h->acf;
  if (S->dZ) return BPRX_OK;
  if (acf_user_bwd_lds(S) > 65536)
    BPRX_FAIL(h, BPRX_E_INVALID, "acf_set_gradient: M = %d with embed_k = %d needs more LDS than a workgroup has in the backward",
              S->M, S->k);
  const size_t I = h->cfg.num_items, MB = h->cfg.max_batch, k = S->k, hc = S->hc, ha = S->ha, W = hc + ha, C = S->C;
  const int NCT = S->NP / 32, nb = NCT < 4 ? NCT : 4, ctiles = (S->C + 127) / 128, zt = (NCT + nb - 1) / nb;
  int ns = 4 * h->num_cu / (ctiles * zt);
  S->nsplit_proj = ns < 1 ? 1 : (ns > 128 ? 128 : ns);
  size_t pf = (size_t)S->nsplit_proj * ctiles * 128 * S->NP;
  if (pf < ACF_SPLIT * k * W) pf = ACF_SPLIT * k * W;
  S->part_floats = pf;
  const size_t gwn = k * hc + C * hc + 3 * k * ha + C * ha + 2 * W;
  DevPool &A = S->mem;
  const size_t mk = A.mark();
  A.zeros(&S->dGP, I * ha);
  A.zeros(&S->q, MB * k);
  A.zeros(&S->aux, MB * (k + 2));
  A.zeros(&S->UV, MB * 2 * W);
  A.zeros(&S->part, pf);
  A.zeros(&S->gwbuf, gwn);
  A.zeros(&S->dZ, I * S->M * S->NP);
  if (!A.ok()) {
    (void)A.rollback(mk);
    BPRX_FAIL(h, BPRX_E_NOMEM, "acf_set_gradient: workspace allocation failed (dZ: %zu MB)", (I * S->M * S->NP * 4) >> 20);
  }
  float *g = S->gwbuf;
  for (int q = 0; q < BPRX_ACF_NW; ++q) S->gw[q] = nullptr;
  S->gw[BPRX_ACF_C_WU] = g; g += k * hc;
  S->gw[BPRX_ACF_C_WI] = g; g += C * hc;
  S->gw[BPRX_ACF_I_WU] = g; g += k * ha;
  S->gw[BPRX_ACF_I_WV] = g; g += k * ha;
  S->gw[BPRX_ACF_I_WP] = g; g += k * ha;
  S->gw[BPRX_ACF_I_WX] = g; g += C * ha;
  S->gw[BPRX_ACF_C_B0] = g;                                 // [dbc0 | dbi0 | dW1c | dW1i]: one block, k_acf_colsum's column order
  S->gw[BPRX_ACF_I_B0] = g + hc;
  S->gw[BPRX_ACF_C_W1] = g + W;
  S->gw[BPRX_ACF_I_W1] = g + W + hc;
  // b_1 of both levels: no gradient tensor.  Both softmaxes are shift-invariant, so the derivative is identically zero; the
  // library writes exactly 2 reg b_1 instead of rounding noise (which Adam would divide by its own magnitude).
  BPRX_HIP(h, hipDeviceSynchronize());
  return BPRX_OK;
}

extern "C" int bprx_acf_set_gradient(bprx_handle *h, int mode) {
  if (!h) return BPRX_E_INVALID;
  if (!h->bound || !h->acf) BPRX_FAIL(h, BPRX_E_STATE, "acf_set_gradient: the handle is not bound with bprx_bind_acf");
  if (mode != BPRX_ACF_GRAD_DETACHED && mode != BPRX_ACF_GRAD_FULL)
    BPRX_FAIL(h, BPRX_E_INVALID, "acf_set_gradient: mode %d is neither BPRX_ACF_GRAD_DETACHED nor BPRX_ACF_GRAD_FULL", mode);
  if (mode == BPRX_ACF_GRAD_FULL) {
    const int rc = acf_full_alloc(h);
    if (rc) return rc;
  }
  h->acf->grad_mode = mode;
  return BPRX_OK;
}

extern "C" int bprx_acf_get_gradient(bprx_handle *h) {
  if (!h) return BPRX_E_INVALID;
  if (!h->bound || !h->acf) BPRX_FAIL(h, BPRX_E_STATE, "acf_get_gradient: the handle is not bound with bprx_bind_acf");
  return h->acf->grad_mode;
}

// Workspace of bprx_acf_explain, allocated at its first call and regrown when a call's histories are longer
static int acf_explain_alloc(bprx_handle *h, int64_t nnz) {
  AcfState *S = h->acf;
  const size_t nu = 2 + (size_t)h->cfg.num_users * (2 + S->hc);
  if (!S->xu && S->mem.regrow(&S->xu, nu, true) != hipSuccess)
    BPRX_FAIL(h, BPRX_E_NOMEM, "acf_explain: workspace allocation failed (%zu MB)", (nu * 4) >> 20);
  if (nnz > S->xt_cap || !S->xt) {
    BPRX_HIP(h, hipDeviceSynchronize());
    S->xt_cap = 0;
    const int64_t cap = nnz < 1 ? 1 : nnz;
    if (S->mem.regrow(&S->xt, (size_t)cap) != hipSuccess)
      BPRX_FAIL(h, BPRX_E_NOMEM, "acf_explain: workspace allocation failed (%zu MB)", ((size_t)cap * 4) >> 20);
    S->xt_cap = cap;
    BPRX_HIP(h, hipMemcpy(S->xu, &cap, sizeof(int64_t), hipMemcpyHostToDevice));   // where the attention pass reads it
  }
  return BPRX_OK;
}

extern "C" int bprx_acf_explain(bprx_handle *h, const int32_t *user, const int32_t *item, int64_t n, const int64_t *hist_ptr,
                                const int32_t *hist_items, int32_t top, float *score, float *base, int32_t *pos, int32_t *hist_item,
                                float *alpha, float *contrib, int32_t *peak, float *beta_peak, float *beta, void *stream) {
  if (!h) return BPRX_E_INVALID;
  if (!h->bound || !h->acf) BPRX_FAIL(h, BPRX_E_STATE, "acf_explain: the handle is not bound with bprx_bind_acf");
  if (top < 1 || top > 32) BPRX_FAIL(h, BPRX_E_INVALID, "acf_explain: top = %d outside [1, 32]", (int)top);
  if (n < 0 || n > ((int64_t)1 << 31) - 1) BPRX_FAIL(h, BPRX_E_INVALID, "acf_explain: n = %lld out of range", (long long)n);
  if (n == 0) return BPRX_OK;
  if (!user || !item || !hist_ptr || !hist_items || !score || !base || !pos || !hist_item || !alpha || !contrib || !peak || !beta_peak)
    BPRX_FAIL(h, BPRX_E_INVALID, "acf_explain: null pointer");
  AcfState *S = h->acf;
  hipStream_t s = (hipStream_t)stream;
  const int U = h->cfg.num_users;
  int64_t nnz = 0;                                             // the one host read: the size of the per-entry workspace
  BPRX_HIP(h, hipMemcpyAsync(&nnz, hist_ptr + U, sizeof(int64_t), hipMemcpyDeviceToHost, s));
  BPRX_HIP(h, hipStreamSynchronize(s));
  if (nnz < 0) BPRX_FAIL(h, BPRX_E_INVALID, "acf_explain: hist_ptr[U] = %lld", (long long)nnz);
  int rc;
  if ((rc = acf_explain_alloc(h, nnz))) return rc;
  hipLaunchKernelGGL(k_acf_claim, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, user, n, U, S->uslot, h->errflag);
  BPRX_LAUNCH_CHECK(h, "k_acf_claim");
  if ((rc = acf_prepare(h, user, n, S->uslot, hist_ptr, hist_items, s))) {
    // the next step's claim is an atomicMin against uslot: leave no claim of this call behind
    hipLaunchKernelGGL(k_acf_unclaim, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, user, n, U, S->uslot);
    (void)hipGetLastError();
    return rc;
  }
  AcfUserArgs UA;
  UA.Gu = h->t.Gu; UA.Pi = S->a.Pi; UA.Z = S->Z; UA.GP = S->GP;
  UA.wcu = S->a.w[BPRX_ACF_C_WU]; UA.bc0 = S->a.w[BPRX_ACF_C_B0]; UA.w1c = S->a.w[BPRX_ACF_C_W1]; UA.bc1 = S->a.w[BPRX_ACF_C_B1];
  UA.wiu = S->a.w[BPRX_ACF_I_WU]; UA.bi0 = S->a.w[BPRX_ACF_I_B0]; UA.w1i = S->a.w[BPRX_ACF_I_W1]; UA.bi1 = S->a.w[BPRX_ACF_I_B1];
  UA.ptr = hist_ptr; UA.items = hist_items; UA.errflag = h->errflag;
  UA.U = U; UA.I = h->cfg.num_items; UA.k = S->k; UA.M = S->M; UA.hc = S->hc; UA.ha = S->ha; UA.NP = S->NP;
  hipLaunchKernelGGL(k_acf_user<ACF_USER_EXPLAIN>, dim3((unsigned)n), dim3(256), acf_user_lds(S), s, UA, user, n, S->uslot, S->xt,
                     S->xu);
  BPRX_LAUNCH_CHECK(h, "k_acf_user<explain>");
  AcfExplainArgs A;
  A.Gu = h->t.Gu; A.Gi = h->t.Gi; A.Pi = S->a.Pi; A.Z = S->Z; A.w1c = S->a.w[BPRX_ACF_C_W1]; A.bc1 = S->a.w[BPRX_ACF_C_B1];
  A.tl = S->xt; A.ustat = S->xu + 2; A.ptr = hist_ptr; A.items = hist_items; A.errflag = h->errflag; A.ncap = S->xt_cap;
  A.U = U; A.I = h->cfg.num_items; A.k = S->k; A.M = S->M; A.hc = S->hc; A.NP = S->NP; A.top = top;
  A.score = score; A.base = base; A.pos = pos; A.hist_item = hist_item; A.alpha = alpha; A.contrib = contrib; A.peak = peak;
  A.beta_peak = beta_peak; A.beta = beta;
  const size_t lds = sizeof(float) * ((size_t)S->hc + 4 * (size_t)(S->hc + S->M));
  hipLaunchKernelGGL(k_acf_explain, dim3((unsigned)((n + 3) / 4)), dim3(256), lds, s, A, user, item, n);
  BPRX_LAUNCH_CHECK(h, "k_acf_explain");
  hipLaunchKernelGGL(k_acf_unclaim, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, user, n, U, S->uslot);
  BPRX_LAUNCH_CHECK(h, "k_acf_unclaim");
  return BPRX_OK;
}
