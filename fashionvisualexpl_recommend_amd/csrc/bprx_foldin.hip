// bprx_foldin.hip -- users the model was not trained on (include/bprx.h: bprx_fold_in), and items with first buyers
// (bprx_fold_in_items: k_fold_items, further down, with its own notes; bprx_af_fold_in_items' step loop k_af_fold_items after it).
//   k_fold_in   n independent small optimisations: the reference's train_step (BPRMF.py:87-125 / VBPR.py:99-144) on a batch made
//               of ONE user's pairs with every item-side parameter frozen, `steps` times, for each of n caller-owned user rows.
//
// With z_i = [Gi_i | P_i[0:d]] and c_i = Bi_i + P_i[d] (P = F.[E|Bp], the cached item projections) the score difference of pair
// p = (i, j) is linear in the user's row w = [gamma | theta]:  x_p = w.D_p + dc_p,  D_p = z_i - z_j,  dc_p = c_i - c_j, so a step is
//     g = sum_p -sigmoid(-x_p) D_p + 2 reg n_r w        (x_p inside the clip range [-80, 1e8], else no gradient)
// followed by sgd or adam_elem (the sparse-variable Adam rule of the Gu / Tu rows).
//
// Layout: one wave per user, four users per workgroup.  Lane l holds elements l, l + 64, ... of w, m, v and g (EPL of them, a
// template parameter: k + d <= 64 EPL), so every row load is one contiguous segment per wave instruction and the update needs no
// exchange between lanes; the dot product meets in wave_sum.  Pairs are walked in groups of NP: the 2 NP rows of a group are all
// requested before the first is used, and the NP dot-product reductions are independent chains.
// D_p and dc_p do not change between steps.  The pairs that fit the wave's share of LDS (64 EPL + 1 floats each; all of a user's
// pairs, or else as many whole groups as fit) are formed once and the steps read them from LDS (each lane reads back the words
// it wrote itself); the rest is gathered again every step (item tables of catalogue size sit in L2 / the Infinity Cache).  Both
// forms hand the same D_p, dc_p to the same fold_group in the same groups (group g is always pairs [g NP, g NP + NP)): the same bits.  No atomics (but the error flag): a user's result depends on its own pairs, its
// start row and the tables only.
#include "bprx_internal.h"

namespace {

struct FoldArgs {
  const float *Gi, *Bi, *P;       // [I, k], [I], [I, PS] (nullptr for BPRMF)
  int I, k, d, PS;
  const int64_t *ptr;             // [n + 1] pairs of user r: [ptr[r], ptr[r + 1])
  const int32_t *pos, *neg;
  int n, steps, adam;
  float lr, reg, b1, b2, eps;
  float *Gu, *Tu, *loss;          // [n, k], [n, d] in / out; [n] or nullptr
  int32_t *errflag;
  int share;                      // floats of LDS per wave (0: the re-gather form for every user)
};

constexpr int FOLD_WAVES = 4;     // users per workgroup

// elements lane, lane + 64, ... of z_it = [Gi_it | P_it[0:d]] (zero past k + d) and c_it
template <int EPL>
__device__ __forceinline__ void fold_row(const FoldArgs &a, int it, int lane, float (&z)[EPL], float &c) {
  const float *g = a.Gi + (size_t)it * a.k;
  const size_t pb = (size_t)it * a.PS;
#pragma unroll
  for (int e = 0; e < EPL; ++e) {
    const int col = lane + 64 * e;
    z[e] = col < a.k ? g[col] : (col < a.k + a.d ? a.P[pb + (col - a.k)] : 0.f);
  }
  c = a.d ? a.Bi[it] + a.P[pb + a.d] : a.Bi[it];
}

// One group of up to NP pairs (cnt of them, wave-uniform): x_p = w.D_p + dc_p, the gradient terms added to acc in pair order, the
// data term of the loss added to lsum (fp64) in pair order (want_loss: the last step).  The one place both forms of the kernel evaluate
// a pair; contraction off, so that the roundings do not depend on what the compiler finds around the inlined body.
template <int EPL, int NP>
__device__ __forceinline__ void fold_group(const float (&w)[EPL], const float (&dl)[NP][EPL], const float (&dc)[NP], int cnt,
                                           float (&acc)[EPL], double &lsum, bool want_loss) {
#pragma clang fp contract(off)
  float x[NP];
#pragma unroll
  for (int q = 0; q < NP; ++q) {
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < EPL; ++e) s += w[e] * dl[q][e];
    x[q] = wave_sum(s) + dc[q];
  }
#pragma unroll
  for (int q = 0; q < NP; ++q) {
    if (q >= cnt) break;
    const float diff = x[q];
    const bool inr = (diff >= -80.0f) && (diff <= 1e8f);                 // tf.clip_by_value gradient mask
    const float g = inr ? -1.0f / (1.0f + expf(diff)) : 0.f;            // -sigmoid(-diff)
#pragma unroll
    for (int e = 0; e < EPL; ++e) acc[e] += g * dl[q][e];
    if (want_loss) {
      const float z = -fminf(fmaxf(diff, -80.0f), 1e8f);                 // softplus(z), stable form
      lsum += (double)(z > 0.f ? z + log1pf(expf(-z)) : log1pf(expf(z)));
    }
  }
}

template <int EPL>
__global__ __launch_bounds__(64 * FOLD_WAVES) void k_fold_in(FoldArgs a) {
  constexpr int NP = EPL <= 4 ? 4 : 2;                       // pairs per group: 2 NP EPL row words in flight per lane
  extern __shared__ __attribute__((aligned(16))) float fold_lds[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int r = blockIdx.x * FOLD_WAVES + wv;
  if (r >= a.n) return;                                      // (no workgroup barrier anywhere below)
  const int64_t p0 = a.ptr[r];
  const int64_t np64 = a.ptr[r + 1] - p0;
  if (np64 <= 0) {                                           // no pairs: the row stays, the loss is 0
    if (lane == 0 && a.loss) a.loss[r] = 0.f;
    return;
  }
  const int np = np64 > INT32_MAX ? INT32_MAX : (int)np64;
  const int W = a.k + a.d;
  float w[EPL], m[EPL], v[EPL];
#pragma unroll
  for (int e = 0; e < EPL; ++e) {
    const int col = lane + 64 * e;
    w[e] = col < a.k ? a.Gu[(size_t)r * a.k + col] : (col < W ? a.Tu[(size_t)r * a.d + (col - a.k)] : 0.f);
    m[e] = 0.f; v[e] = 0.f;
  }
  const int32_t *pos = a.pos + p0, *neg = a.neg + p0;
  float *dls = fold_lds + (size_t)wv * a.share;              // [nc][EPL][64] differences, then [nc] dc
  // the first nc pairs live in LDS: all of them where they fit, else as many whole groups as do
  const int fit = a.share / (64 * EPL + 1);
  const int nc = np <= fit ? np : fit / NP * NP;
  float *dcs = dls + (size_t)nc * (64 * EPL);

  // walks the pairs [begin, end) (begin a multiple of NP) in groups of NP, gathering the item rows:
  // fn(first pair of the group, D, dc, pairs in the group)
  auto gather_walk = [&](int begin, int end, auto &&fn) {
    for (int base = begin; base < end; base += 64) {
      const int nb = min(64, end - base);
      int ii = 0, jj = 0;
      if (lane < nb) {
        ii = clamp_index(pos[base + lane], a.I, a.errflag, 2);
        jj = clamp_index(neg[base + lane], a.I, a.errflag, 2);
      }
      for (int q0 = 0; q0 < nb; q0 += NP) {
        const int cnt = min(NP, nb - q0);
        float zi[NP][EPL], zj[NP][EPL], ci[NP], cj[NP];
#pragma unroll
        for (int q = 0; q < NP; ++q) {                         // (a group's tail gathers its last pair again: loads in range, unused)
          const int src = min(q0 + q, nb - 1);
          const int it = __builtin_amdgcn_readfirstlane(__shfl(ii, src, 64));
          const int jt = __builtin_amdgcn_readfirstlane(__shfl(jj, src, 64));
          fold_row<EPL>(a, it, lane, zi[q], ci[q]);
          fold_row<EPL>(a, jt, lane, zj[q], cj[q]);
        }
        float dl[NP][EPL], dc[NP];
#pragma unroll
        for (int q = 0; q < NP; ++q) {
#pragma unroll
          for (int e = 0; e < EPL; ++e) dl[q][e] = zi[q][e] - zj[q][e];
          dc[q] = ci[q] - cj[q];
        }
        fn(base + q0, dl, dc, cnt);
      }
    }
  };

  if (nc) {
    gather_walk(0, nc, [&](int q0, const float (&dl)[NP][EPL], const float (&dc)[NP], int cnt) {
#pragma unroll
      for (int q = 0; q < NP; ++q) {
        if (q >= cnt) break;
#pragma unroll
        for (int e = 0; e < EPL; ++e) dls[((size_t)(q0 + q) * EPL + e) * 64 + lane] = dl[q][e];
        if (lane == 0) dcs[q0 + q] = dc[q];
      }
    });
    wave_sync();                                             // dc: written by lane 0, read by every lane
  }

  const float r2n = 2.f * a.reg * (float)np, rn = a.reg * (float)np;
  for (int t = 1; t <= a.steps; ++t) {
    const bool last = t == a.steps && a.loss != nullptr;
    float acc[EPL];
    double lsum = 0.0;                                       // (thousands of pairs: the data term of the loss is summed in fp64)
#pragma unroll
    for (int e = 0; e < EPL; ++e) acc[e] = 0.f;
    for (int q0 = 0; q0 < nc; q0 += NP) {
      const int cnt = min(NP, nc - q0);
      float dl[NP][EPL], dc[NP];
#pragma unroll
      for (int q = 0; q < NP; ++q) {
        const int src = min(q0 + q, nc - 1);
#pragma unroll
        for (int e = 0; e < EPL; ++e) dl[q][e] = dls[((size_t)src * EPL + e) * 64 + lane];
        dc[q] = dcs[src];
      }
      fold_group<EPL, NP>(w, dl, dc, cnt, acc, lsum, last);
    }
    if (nc < np) {
      gather_walk(nc, np, [&](int, const float (&dl)[NP][EPL], const float (&dc)[NP], int cnt) {
        fold_group<EPL, NP>(w, dl, dc, cnt, acc, lsum, last);
      });
    }
    if (last) {                                              // loss_T, before the last update, as train_step returns it
      float s = 0.f;
#pragma unroll
      for (int e = 0; e < EPL; ++e) s += w[e] * w[e];
      s = wave_sum(s);
      if (lane == 0) a.loss[r] = (float)(lsum + (double)(rn * s));
    }
    if (a.adam) {
      const float tt = (float)t;
      const float lr_t = a.lr * sqrtf(1.0f - powf(a.b2, tt)) / (1.0f - powf(a.b1, tt));
#pragma unroll
      for (int e = 0; e < EPL; ++e) adam_elem(w[e], m[e], v[e], acc[e] + r2n * w[e], a.b1, a.b2, lr_t, a.eps);
    } else {
#pragma unroll
      for (int e = 0; e < EPL; ++e) w[e] = w[e] - a.lr * (acc[e] + r2n * w[e]);
    }
  }
#pragma unroll
  for (int e = 0; e < EPL; ++e) {
    const int col = lane + 64 * e;
    if (col < a.k) a.Gu[(size_t)r * a.k + col] = w[e];
    else if (col < W) a.Tu[(size_t)r * a.d + (col - a.k)] = w[e];
  }
}

#define EPL_SWITCH(N, CALL)            \
  switch (N) {                         \
    case 1: CALL(1); break;            \
    case 2: CALL(2); break;            \
    case 3: CALL(3); break;            \
    case 4: CALL(4); break;            \
    case 5: case 6: CALL(6); break;    \
    case 7: case 8: CALL(8); break;    \
    case 9: case 10: case 11: case 12: CALL(12); break; \
    default: CALL(16); break;          \
  }

// Floats of LDS per wave for the cached pairs: 40 KB per workgroup, so that four workgroups still share a CU (the occupancy the
// registers allow).  Measured at I = 50 000, k = d = 64, 100 000 users, 30 adam steps, ms per call for 8 / 20 / 80 pairs per user
// (profiles/fold_in_share_sweep.jsonl): no LDS 7.57 / 17.09 / 64.69; 1 024 floats 4.90 / 14.85 / 62.38; 1 536 3.50 / 12.52 / 59.95;
// 2 560 3.50 / 7.64 / 54.68; 4 096 (64 KB per workgroup: two workgroups per CU) 5.00 / 9.55 / 88.58.
constexpr int FOLD_SHARE = 2560;
// ... and for k_fold_items: the same 40 KB per workgroup (an item's row is k + 1 wide: at k = d = 64 19 pairs fit, where a user's
// k + d row fits 19 as well -- both are two lane words)
constexpr int FOLD_ITEM_SHARE = FOLD_SHARE;

// ---- items the model was not trained on, once they have first buyers (include/bprx.h: bprx_fold_in_items) ----
//   k_fold_items   the layout twin of k_fold_in: one wave per new item, four per workgroup, the same train_step with every user-side
//                  and catalogue parameter frozen.  New item r owns w = [Gi_r | Bi_r] (k + 1 numbers); pair p = (u, o, role) is the
//                  reference's triplet (u, r, o) (role 0, s = +1) or (u, o, r) (role 1, s = -1):
//     a_p = [Gu_u | 1]      v_p = Tu_u.(Pn_r[0:d] - P_o[0:d]) + (Pn_r[d] - P_o[d]) - Bi_o - Gu_u.Gi_o      x_p = s (w.a_p + v_p)
// so with D_p = s a_p and dc_p = s v_p (a sign flip each: exact) a pair is what fold_group takes, and the step loop below is
// k_fold_in's.  Two things differ.  Setup: dc_p costs a (k + d)-wide dot over four gathered rows (Gu_u, Gi_o, Tu_u, P_o) and the
// item's own projection row Pn_r; the k part is formed from the registers that hold a_p, the d part in a strided loop (Pn_r: one
// row per wave, L1-resident).  Regulariser: per element, rv = [n_r, ..., n_r | n_pos + c_neg n_neg] (the reference regularises
// the bias of a negative by reg / 10: VBPR.py:125).  LDS share, group order and the re-gather form as in k_fold_in: the same bits
// from both forms.  No atomics but the error flag.
struct FoldItemArgs {
  const float *Gu, *Tu, *Gi, *Bi, *P;   // the bound tables: [U, k], [U, d], [I, k], [I], [I, PS] (Tu, P: nullptr for BPRMF)
  const float *Pn;                      // [n, PS] projections of the new items (nullptr for BPRMF)
  int U, I, k, d, PS;
  const int64_t *ptr;                   // [n + 1] pairs of item r: [ptr[r], ptr[r + 1])
  const int32_t *user, *other, *role;
  int n, steps, adam;
  float lr, reg, cneg, b1, b2, eps;
  float *Gi_rows, *Bi_rows, *loss;      // [n, k], [n] in / out; [n] or nullptr
  int32_t *errflag;
  int share;                            // floats of LDS per wave (0: the re-gather form for every item)
};

// D_p (elements lane, lane + 64, ... of s [Gu_u | 1], zero past k + 1) and dc_p = s v_p of one pair; pn: the item's row of Pn.
// The one place both forms of the kernel form a pair (contraction off: the same roundings wherever it is inlined).
template <int EPL>
__device__ __forceinline__ void fold_item_pair(const FoldItemArgs &a, int u, int o, float sgn, const float *pn, int lane,
                                               float (&dl)[EPL], float &dc) {
#pragma clang fp contract(off)
  const float *gu = a.Gu + (size_t)u * a.k, *gi = a.Gi + (size_t)o * a.k;
  float au[EPL], gv[EPL];
#pragma unroll
  for (int e = 0; e < EPL; ++e) {                              // (both rows requested before the first use)
    const int col = lane + 64 * e;
    au[e] = col < a.k ? gu[col] : (col == a.k ? 1.f : 0.f);
    gv[e] = col < a.k ? gi[col] : 0.f;
  }
  float s = 0.f;
  if (a.d) {
    const float *tu = a.Tu + (size_t)u * a.d, *po = a.P + (size_t)o * a.PS;
    for (int c = lane; c < a.d; c += 64) s += tu[c] * (pn[c] - po[c]);
  }
#pragma unroll
  for (int e = 0; e < EPL; ++e) {
    s -= au[e] * gv[e];
    dl[e] = sgn * au[e];
  }
  float v = wave_sum(s);
  v = a.d ? v + ((pn[a.d] - a.P[(size_t)o * a.PS + a.d]) - a.Bi[o]) : v - a.Bi[o];
  dc = sgn * v;
}

template <int EPL>
__global__ __launch_bounds__(64 * FOLD_WAVES) void k_fold_items(FoldItemArgs a) {
  constexpr int NP = EPL <= 4 ? 4 : 2;                       // pairs per group, as k_fold_in
  extern __shared__ __attribute__((aligned(16))) float fold_lds[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int r = blockIdx.x * FOLD_WAVES + wv;
  if (r >= a.n) return;                                      // (no workgroup barrier anywhere below)
  const int64_t p0 = a.ptr[r];
  const int64_t np64 = a.ptr[r + 1] - p0;
  if (np64 <= 0) {                                           // no pairs: the row stays, the loss is 0
    if (lane == 0 && a.loss) a.loss[r] = 0.f;
    return;
  }
  const int np = np64 > INT32_MAX ? INT32_MAX : (int)np64;
  const int W = a.k + 1;
  float w[EPL], m[EPL], v[EPL];
#pragma unroll
  for (int e = 0; e < EPL; ++e) {
    const int col = lane + 64 * e;
    w[e] = col < a.k ? a.Gi_rows[(size_t)r * a.k + col] : (col < W ? a.Bi_rows[r] : 0.f);
    m[e] = 0.f; v[e] = 0.f;
  }
  const int32_t *user = a.user + p0, *other = a.other + p0, *role = a.role + p0;
  const float *pn = a.d ? a.Pn + (size_t)r * a.PS : nullptr;
  int npos = 0;                                              // pairs in which the item is the positive
  for (int p = lane; p < np; p += 64) npos += clamp_index(role[p], 2, a.errflag, 2) == 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) npos += __shfl_xor(npos, o, 64);
  float *dls = fold_lds + (size_t)wv * a.share;              // [nc][EPL][64] D, then [nc] dc
  const int fit = a.share / (64 * EPL + 1);
  const int nc = np <= fit ? np : fit / NP * NP;
  float *dcs = dls + (size_t)nc * (64 * EPL);

  // walks the pairs [begin, end) (begin a multiple of NP) in groups of NP, gathering the rows: fn(first pair, D, dc, pairs)
  auto gather_walk = [&](int begin, int end, auto &&fn) {
    for (int base = begin; base < end; base += 64) {
      const int nb = min(64, end - base);
      int uu = 0, oo = 0, rr = 0;
      if (lane < nb) {
        uu = clamp_index(user[base + lane], a.U, a.errflag, 1);
        oo = clamp_index(other[base + lane], a.I, a.errflag, 2);
        rr = clamp_quiet(role[base + lane], 2);              // (reported by the count above)
      }
      for (int q0 = 0; q0 < nb; q0 += NP) {
        const int cnt = min(NP, nb - q0);
        float dl[NP][EPL], dc[NP];
#pragma unroll
        for (int q = 0; q < NP; ++q) {                         // (a group's tail forms its last pair again: loads in range, unused)
          const int src = min(q0 + q, nb - 1);
          const int ut = __builtin_amdgcn_readfirstlane(__shfl(uu, src, 64));
          const int ot = __builtin_amdgcn_readfirstlane(__shfl(oo, src, 64));
          const int rt = __builtin_amdgcn_readfirstlane(__shfl(rr, src, 64));
          fold_item_pair<EPL>(a, ut, ot, rt ? -1.f : 1.f, pn, lane, dl[q], dc[q]);
        }
        fn(base + q0, dl, dc, cnt);
      }
    }
  };

  if (nc) {
    gather_walk(0, nc, [&](int q0, const float (&dl)[NP][EPL], const float (&dc)[NP], int cnt) {
#pragma unroll
      for (int q = 0; q < NP; ++q) {
        if (q >= cnt) break;
#pragma unroll
        for (int e = 0; e < EPL; ++e) dls[((size_t)(q0 + q) * EPL + e) * 64 + lane] = dl[q][e];
        if (lane == 0) dcs[q0 + q] = dc[q];
      }
    });
    wave_sync();                                             // dc: written by lane 0, read by every lane
  }

  float r2[EPL], r1[EPL];                                    // 2 reg rv and reg rv of the lane's elements
  {
    const float rvk = (float)np, rvb = (float)npos + a.cneg * (float)(np - npos);
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
      const int col = lane + 64 * e;
      const float rv = col < a.k ? rvk : (col < W ? rvb : 0.f);
      r2[e] = 2.f * a.reg * rv; r1[e] = a.reg * rv;
    }
  }
  for (int t = 1; t <= a.steps; ++t) {
#pragma clang fp contract(off)
    const bool last = t == a.steps && a.loss != nullptr;
    float acc[EPL];
    double lsum = 0.0;
#pragma unroll
    for (int e = 0; e < EPL; ++e) acc[e] = 0.f;
    for (int q0 = 0; q0 < nc; q0 += NP) {
      const int cnt = min(NP, nc - q0);
      float dl[NP][EPL], dc[NP];
#pragma unroll
      for (int q = 0; q < NP; ++q) {
        const int src = min(q0 + q, nc - 1);
#pragma unroll
        for (int e = 0; e < EPL; ++e) dl[q][e] = dls[((size_t)src * EPL + e) * 64 + lane];
        dc[q] = dcs[src];
      }
      fold_group<EPL, NP>(w, dl, dc, cnt, acc, lsum, last);
    }
    if (nc < np) {
      gather_walk(nc, np, [&](int, const float (&dl)[NP][EPL], const float (&dc)[NP], int cnt) {
        fold_group<EPL, NP>(w, dl, dc, cnt, acc, lsum, last);
      });
    }
    if (last) {                                              // loss_T, before the last update, as train_step returns it
      float s = 0.f;
#pragma unroll
      for (int e = 0; e < EPL; ++e) s += r1[e] * (w[e] * w[e]);
      s = wave_sum(s);
      if (lane == 0) a.loss[r] = (float)(lsum + (double)s);
    }
    if (a.adam) {
      const float tt = (float)t;
      const float lr_t = a.lr * sqrtf(1.0f - powf(a.b2, tt)) / (1.0f - powf(a.b1, tt));
#pragma unroll
      for (int e = 0; e < EPL; ++e) adam_elem(w[e], m[e], v[e], acc[e] + r2[e] * w[e], a.b1, a.b2, lr_t, a.eps);
    } else {
#pragma unroll
      for (int e = 0; e < EPL; ++e) w[e] = w[e] - a.lr * (acc[e] + r2[e] * w[e]);
    }
  }
#pragma unroll
  for (int e = 0; e < EPL; ++e) {
    const int col = lane + 64 * e;
    if (col < a.k) a.Gi_rows[(size_t)r * a.k + col] = w[e];
    else if (col < W) a.Bi_rows[r] = w[e];
  }
}

// ---- AttentiveFashion items with first buyers (include/bprx.h: bprx_af_fold_in_items) ----
//   k_af_fold_items   the step loop of k_fold_items for rows that are already formed: k_af_item_pairs (bprx_attentive.hip) has
//                     written [D_p (k) | dc_p | zeros] of every pair to work [pairs, KW].  New item r owns w = Gi_r (k numbers, no
//                     bias: the model scores no Bi), rv = n_r for every element.  One wave per item, four per workgroup, the same
//                     LDS share, groups and fold_group as above: the first pairs that fit are read from work once, the others
//                     every step (work of a call sits in L2 / the Infinity Cache); both forms hand fold_group the same words.
struct AfFoldItemArgs {
  const float *work;                    // [ptr[n], KW]
  int k, KW;
  const int64_t *ptr;                   // [n + 1] pairs of item r: [ptr[r], ptr[r + 1])
  int n, steps, adam;
  float lr, reg, b1, b2, eps;
  float *Gi_rows, *loss;                // [n, k] in / out; [n] or nullptr
  int share;                            // floats of LDS per wave (0: every step reads work)
};

template <int EPL>
__global__ __launch_bounds__(64 * FOLD_WAVES) void k_af_fold_items(AfFoldItemArgs a) {
  constexpr int NP = EPL <= 4 ? 4 : 2;                       // pairs per group, as k_fold_in
  extern __shared__ __attribute__((aligned(16))) float fold_lds[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int r = blockIdx.x * FOLD_WAVES + wv;
  if (r >= a.n) return;                                      // (no workgroup barrier anywhere below)
  const int64_t p0 = a.ptr[r];
  const int64_t np64 = a.ptr[r + 1] - p0;
  if (np64 <= 0) {                                           // no pairs: the row stays, the loss is 0
    if (lane == 0 && a.loss) a.loss[r] = 0.f;
    return;
  }
  const int np = np64 > INT32_MAX ? INT32_MAX : (int)np64;
  float w[EPL], m[EPL], v[EPL];
#pragma unroll
  for (int e = 0; e < EPL; ++e) {
    const int col = lane + 64 * e;
    w[e] = col < a.k ? a.Gi_rows[(size_t)r * a.k + col] : 0.f;
    m[e] = 0.f; v[e] = 0.f;
  }
  const float *rows = a.work + (size_t)p0 * a.KW;
  float *dls = fold_lds + (size_t)wv * a.share;              // [nc][EPL][64] D, then [nc] dc
  const int fit = a.share / (64 * EPL + 1);
  const int nc = np <= fit ? np : fit / NP * NP;
  float *dcs = dls + (size_t)nc * (64 * EPL);

  // D (elements lane, lane + 64, ... : zero past k) and dc of pair p
  auto read_pair = [&](int p, float (&dl)[EPL], float &dc) {
    const float *row = rows + (size_t)p * a.KW;
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
      const int col = lane + 64 * e;
      dl[e] = col < a.k ? row[col] : 0.f;
    }
    dc = row[a.k];
  };

  for (int p = 0; p < nc; ++p) {
    float dl[EPL], dc;
    read_pair(p, dl, dc);
#pragma unroll
    for (int e = 0; e < EPL; ++e) dls[((size_t)p * EPL + e) * 64 + lane] = dl[e];
    if (lane == 0) dcs[p] = dc;
  }
  if (nc) wave_sync();                                       // dc: written by lane 0, read by every lane

  const float r2 = 2.f * a.reg * (float)np, r1 = a.reg * (float)np;
  for (int t = 1; t <= a.steps; ++t) {
#pragma clang fp contract(off)
    const bool last = t == a.steps && a.loss != nullptr;
    float acc[EPL];
    double lsum = 0.0;
#pragma unroll
    for (int e = 0; e < EPL; ++e) acc[e] = 0.f;
    for (int q0 = 0; q0 < nc; q0 += NP) {
      const int cnt = min(NP, nc - q0);
      float dl[NP][EPL], dc[NP];
#pragma unroll
      for (int q = 0; q < NP; ++q) {
        const int src = min(q0 + q, nc - 1);
#pragma unroll
        for (int e = 0; e < EPL; ++e) dl[q][e] = dls[((size_t)src * EPL + e) * 64 + lane];
        dc[q] = dcs[src];
      }
      fold_group<EPL, NP>(w, dl, dc, cnt, acc, lsum, last);
    }
    for (int q0 = nc; q0 < np; q0 += NP) {                   // (nc is a multiple of NP here: the same groups as from LDS)
      const int cnt = min(NP, np - q0);
      float dl[NP][EPL], dc[NP];
#pragma unroll
      for (int q = 0; q < NP; ++q) read_pair(min(q0 + q, np - 1), dl[q], dc[q]);   // (a group's tail reads its last pair again)
      fold_group<EPL, NP>(w, dl, dc, cnt, acc, lsum, last);
    }
    if (last) {                                              // loss_T, before the last update, as train_step returns it
      float s = 0.f;
#pragma unroll
      for (int e = 0; e < EPL; ++e) s += r1 * (w[e] * w[e]);
      s = wave_sum(s);
      if (lane == 0) a.loss[r] = (float)(lsum + (double)s);
    }
    if (a.adam) {
      const float tt = (float)t;
      const float lr_t = a.lr * sqrtf(1.0f - powf(a.b2, tt)) / (1.0f - powf(a.b1, tt));
#pragma unroll
      for (int e = 0; e < EPL; ++e) adam_elem(w[e], m[e], v[e], acc[e] + r2 * w[e], a.b1, a.b2, lr_t, a.eps);
    } else {
#pragma unroll
      for (int e = 0; e < EPL; ++e) w[e] = w[e] - a.lr * (acc[e] + r2 * w[e]);
    }
  }
#pragma unroll
  for (int e = 0; e < EPL; ++e) {
    const int col = lane + 64 * e;
    if (col < a.k) a.Gi_rows[(size_t)r * a.k + col] = w[e];
  }
}

}  // namespace

int bprx_launch_af_fold_items(bprx_handle *h, const int64_t *pair_ptr, int64_t n, const float *work, int KW, int k, int steps, bool adam,
                              float lr, float reg, float *Gi_rows, float *loss, hipStream_t s) {
  const bprx_config &c = h->cfg;
  AfFoldItemArgs a;
  a.work = work; a.k = k; a.KW = KW; a.ptr = pair_ptr;
  a.n = (int)n; a.steps = steps; a.adam = adam ? 1 : 0;
  a.lr = lr; a.reg = reg; a.b1 = c.beta1; a.b2 = c.beta2; a.eps = c.epsilon;
  a.Gi_rows = Gi_rows; a.loss = loss;
  a.share = h->fold_cache ? FOLD_ITEM_SHARE : 0;
  const unsigned grid = (unsigned)((n + FOLD_WAVES - 1) / FOLD_WAVES);
  const size_t lds = (size_t)a.share * FOLD_WAVES * sizeof(float);
#define CALL(N) hipLaunchKernelGGL(k_af_fold_items<N>, dim3(grid), dim3(64 * FOLD_WAVES), lds, s, a)
  EPL_SWITCH((k + 63) / 64, CALL)
#undef CALL
  BPRX_LAUNCH_CHECK(h, "k_af_fold_items");
  return BPRX_OK;
}

extern "C" int bprx_fold_in(bprx_handle *h, const int64_t *pair_ptr, const int32_t *pos, const int32_t *neg, int64_t n,
                            int32_t steps, float lr, float reg, int32_t optimizer, float *Gu_rows, float *Tu_rows, float *loss,
                            void *stream) {
  if (!h) return BPRX_E_INVALID;
  const bprx_config &c = h->cfg;
  if (n < 0 || n >= ((int64_t)1 << 31)) BPRX_FAIL(h, BPRX_E_INVALID, "fold_in: n = %lld out of range", (long long)n);
  if (steps < 1) BPRX_FAIL(h, BPRX_E_INVALID, "fold_in: steps = %d < 1", steps);
  if (optimizer != BPRX_OPT_SGD && optimizer != BPRX_OPT_ADAM_TF23) BPRX_FAIL(h, BPRX_E_INVALID, "fold_in: optimizer %d", optimizer);
  if (c.embed_k + c.embed_d > 1024) BPRX_FAIL(h, BPRX_E_INVALID, "fold_in: k + d = %d > 1024", c.embed_k + c.embed_d);
  if (!pair_ptr || !Gu_rows || (c.embed_d > 0) != (Tu_rows != nullptr)) BPRX_FAIL(h, BPRX_E_INVALID, "fold_in: null pointer");
  if (n && (!pos || !neg)) BPRX_FAIL(h, BPRX_E_INVALID, "fold_in: null pointer");
  hipStream_t s = (hipStream_t)stream;
  // (ACF and AttentiveFashion build the user side from attention: plain handles only)
  const int rc = bprx_enter(h, "fold_in", NEED_BOUND | NEED_ROWS | NEED_P_ALL, KIND_PLAIN, s);
  if (rc || n == 0) return rc;
  FoldArgs a;
  a.Gi = h->t.Gi; a.Bi = h->t.Bi; a.P = c.embed_d ? h->P : nullptr;
  a.I = c.num_items; a.k = c.embed_k; a.d = c.embed_d; a.PS = h->PS;
  a.ptr = pair_ptr; a.pos = pos; a.neg = neg;
  a.n = (int)n; a.steps = steps; a.adam = optimizer == BPRX_OPT_ADAM_TF23;
  a.lr = lr; a.reg = reg; a.b1 = c.beta1; a.b2 = c.beta2; a.eps = c.epsilon;
  a.Gu = Gu_rows; a.Tu = Tu_rows; a.loss = loss; a.errflag = h->errflag;
  a.share = h->fold_cache ? FOLD_SHARE : 0;
  const unsigned grid = (unsigned)((n + FOLD_WAVES - 1) / FOLD_WAVES);
  const size_t lds = (size_t)a.share * FOLD_WAVES * sizeof(float);
#define CALL(N) hipLaunchKernelGGL(k_fold_in<N>, dim3(grid), dim3(64 * FOLD_WAVES), lds, s, a)
  EPL_SWITCH((c.embed_k + c.embed_d + 63) / 64, CALL)
#undef CALL
  BPRX_LAUNCH_CHECK(h, "k_fold_in");
  return BPRX_OK;
}

extern "C" int bprx_fold_in_items(bprx_handle *h, const int64_t *pair_ptr, const int32_t *user, const int32_t *other, const int32_t *role,
                                  int64_t n, const float *Pn, int32_t steps, float lr, float reg, int32_t optimizer, float *Gi_rows,
                                  float *Bi_rows, float *loss, void *stream) {
  if (!h) return BPRX_E_INVALID;
  const bprx_config &c = h->cfg;
  if (n < 0 || n >= ((int64_t)1 << 31)) BPRX_FAIL(h, BPRX_E_INVALID, "fold_in_items: n = %lld out of range", (long long)n);
  if (steps < 1) BPRX_FAIL(h, BPRX_E_INVALID, "fold_in_items: steps = %d < 1", steps);
  if (optimizer != BPRX_OPT_SGD && optimizer != BPRX_OPT_ADAM_TF23) BPRX_FAIL(h, BPRX_E_INVALID, "fold_in_items: optimizer %d", optimizer);
  if (c.embed_k + 1 > 1024 || c.embed_k + c.embed_d > 1024)
    BPRX_FAIL(h, BPRX_E_INVALID, "fold_in_items: k + 1 = %d or k + d = %d > 1024", c.embed_k + 1, c.embed_k + c.embed_d);
  if (!pair_ptr || !Gi_rows || !Bi_rows || (c.embed_d > 0) != (Pn != nullptr)) BPRX_FAIL(h, BPRX_E_INVALID, "fold_in_items: null pointer");
  if (n && (!user || !other || !role)) BPRX_FAIL(h, BPRX_E_INVALID, "fold_in_items: null pointer");
  if (c.model == BPRX_MODEL_VBPR && c.feat_dtype == BPRX_F_FP8)
    BPRX_FAIL(h, BPRX_E_INVALID, "fold_in_items: fp8 features are not supported for new items (a new row may exceed the max-abs the "
                                 "codes were scaled for and would saturate): fp32 or bf16");
  hipStream_t s = (hipStream_t)stream;
  const int rc = bprx_enter(h, "fold_in_items", NEED_BOUND | NEED_ROWS | NEED_P_ALL, KIND_PLAIN, s);
  if (rc || n == 0) return rc;
  FoldItemArgs a;
  a.Gu = h->t.Gu; a.Tu = c.embed_d ? h->t.Tu : nullptr; a.Gi = h->t.Gi; a.Bi = h->t.Bi; a.P = c.embed_d ? h->P : nullptr;
  a.Pn = Pn;
  a.U = c.num_users; a.I = c.num_items; a.k = c.embed_k; a.d = c.embed_d; a.PS = h->PS;
  a.ptr = pair_ptr; a.user = user; a.other = other; a.role = role;
  a.n = (int)n; a.steps = steps; a.adam = optimizer == BPRX_OPT_ADAM_TF23;
  a.lr = lr; a.reg = reg; a.cneg = h->neg_bias_reg; a.b1 = c.beta1; a.b2 = c.beta2; a.eps = c.epsilon;
  a.Gi_rows = Gi_rows; a.Bi_rows = Bi_rows; a.loss = loss; a.errflag = h->errflag;
  a.share = h->fold_cache ? FOLD_ITEM_SHARE : 0;
  const unsigned grid = (unsigned)((n + FOLD_WAVES - 1) / FOLD_WAVES);
  const size_t lds = (size_t)a.share * FOLD_WAVES * sizeof(float);
#define CALL(N) hipLaunchKernelGGL(k_fold_items<N>, dim3(grid), dim3(64 * FOLD_WAVES), lds, s, a)
  EPL_SWITCH((c.embed_k + 1 + 63) / 64, CALL)
#undef CALL
  BPRX_LAUNCH_CHECK(h, "k_fold_items");
  return BPRX_OK;
}
