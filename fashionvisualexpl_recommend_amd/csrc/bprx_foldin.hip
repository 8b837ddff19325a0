// bprx_foldin.hip -- rows fitted after training with everything else frozen (include/bprx.h): users the model was not trained on
// (bprx_fold_in), items with first buyers (bprx_fold_in_items) and the step loop of bprx_af_fold_in_items.
//   k_fold_fit<EPL, Row>   n independent small optimisations: the reference's train_step (BPRMF.py:87-125 / VBPR.py:99-144) on a
//                          batch made of ONE row's pairs, `steps` times, for each of n caller-owned rows.
//
// The score difference of pair p is linear in the row w that is fitted:  x_p = w.D_p + dc_p, so a step is
//     g = sum_p -sigmoid(-x_p) D_p + 2 reg rv * w        (x_p inside the clip range [-80, 1e8], else no gradient)
// followed by sgd or adam_elem (the sparse-variable Adam rule of the Gu / Tu rows), and the loss is sum_p softplus(-x_p) + reg
// sum_e rv_e w_e^2.  What w, D_p, dc_p and rv are is the Row's business, one policy struct per entry point:
//     UserRow    w = [gamma | theta] of a new user; pair (i, j): D_p = z_i - z_j, dc_p = c_i - c_j with z_i = [Gi_i | P_i[0:d]],
//                c_i = Bi_i + P_i[d] (P = F.[E|Bp], the cached item projections); rv = n_r, the row's pairs.
//     ItemRow    w = [Gi_r | Bi_r] of a new item; pair (u, o, role) is the reference's triplet (u, r, o) (role 0, s = +1) or
//                (u, o, r) (role 1, s = -1): D_p = s [Gu_u | 1], dc_p = s v_p,
//                v_p = Tu_u.(Pn_r[0:d] - P_o[0:d]) + (Pn_r[d] - P_o[d]) - Bi_o - Gu_u.Gi_o (a sign flip each: exact);
//                rv = [n_r, ..., n_r | n_pos + c_neg n_neg] (the reference regularises the bias of a negative by reg / 10: VBPR.py:125).
//     AfItemRow  w = Gi_r of a new AttentiveFashion item (no bias: the model scores no Bi); k_af_item_pairs (bprx_attentive.hip) has
//                written [D_p (k) | dc_p | zeros] of every pair to work [pairs, KW]; rv = n_r.
// A Row supplies `at` (where the row lives: what the lane's elements are loaded from and stored to), walk() (the group former: D
// and dc of the pairs [q0, q0 + NP), group by group) and the regulariser, gradient side r2(e) and loss side reg_loss(); all else
// is written once.
//
// Layout: one wave per row, four rows per workgroup.  Lane l holds elements l, l + 64, ... of w, m, v and g (EPL of them, a template
// parameter: the row is <= 64 EPL wide), so every row load is one contiguous segment per wave instruction and the update needs no
// exchange between lanes; the dot product meets in wave_sum.  Pairs are walked in groups of NP: the rows of a group are all
// requested before the first is used, and the NP dot-product reductions are independent chains.
// D_p and dc_p do not change between steps.  The pairs that fit the wave's share of LDS (64 EPL + 1 floats each; all of a row's
// pairs, or else as many whole groups as fit) are formed once and the steps read them from LDS (each lane reads back the words it
// wrote itself); the rest is formed again every step (item tables of catalogue size and the work rows of a call sit in L2 / the
// Infinity Cache).  Both forms hand the same D_p, dc_p to the same fold_group in the same groups (group g is always pairs
// [g NP, g NP + NP)): the same bits.  No atomics (but the error flag): a row's result depends on its own pairs, its start and the
// tables only.
//
// Rounding.  The step loop and fold_group run with contraction off, and each Row says in explicit operations what is fused: the
// result does not depend on what the compiler finds around an inlined body.  ItemRow and AfItemRow fuse nothing in the loop.
// UserRow keeps the roundings its kernel was first built with (default contraction, which fused what the optimiser left fusable):
// g_e = fma(2 reg n_r, w_e, acc_e), and in the loss the last w_e^2 of an odd EPL fused into the sum (see UserRow::reg_loss).  The
// sgd update w - lr g is two roundings in every Row.
#include "bprx_internal.h"

namespace {

struct FitArgs {                  // what every fit takes
  const int64_t *ptr;             // [n + 1] pairs of row r: [ptr[r], ptr[r + 1])
  int n, steps, adam;
  float lr, reg, b1, b2, eps;
  float *loss;                    // [n] or nullptr
  int share;                      // floats of LDS per wave (0: every pair is formed again every step)
};

struct FoldArgs : FitArgs {
  const float *Gi, *Bi, *P;       // [I, k], [I], [I, PS] (nullptr for BPRMF)
  int I, k, d, PS;
  const int32_t *pos, *neg;
  float *Gu, *Tu;                 // [n, k], [n, d] in / out
  int32_t *errflag;
};

struct FoldItemArgs : FitArgs {
  const float *Gu, *Tu, *Gi, *Bi, *P;   // the bound tables: [U, k], [U, d], [I, k], [I], [I, PS] (Tu, P: nullptr for BPRMF)
  const float *Pn;                      // [n, PS] projections of the new items (nullptr for BPRMF)
  int U, I, k, d, PS;
  const int32_t *user, *other, *role;
  float cneg;
  float *Gi_rows, *Bi_rows;             // [n, k], [n] in / out
  int32_t *errflag;
};

struct AfFoldItemArgs : FitArgs {
  const float *work;                    // [ptr[n], KW]
  int k, KW;
  float *Gi_rows;                       // [n, k] in / out
};

constexpr int FOLD_WAVES = 4;     // rows per workgroup

// Where the row a wave fits lives: n0 floats at p0, then n1 at p1 (wave-uniform).  Lane l holds elements l, l + 64, ...: zero past
// n0 + n1.
struct RowPlace {
  float *p0, *p1;
  int n0, n1;
  template <int EPL>
  __device__ __forceinline__ void load(int lane, float (&w)[EPL]) const {
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
      const int col = lane + 64 * e;
      w[e] = col < n0 ? p0[col] : (col < n0 + n1 ? p1[col - n0] : 0.f);
    }
  }
  template <int EPL>
  __device__ __forceinline__ void store(int lane, const float (&w)[EPL]) const {
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
      const int col = lane + 64 * e;
      if (col < n0) p0[col] = w[e];
      else if (col < n0 + n1) p1[col - n0] = w[e];
    }
  }
};

// D_p (elements lane, lane + 64, ... of s [Gu_u | 1], zero past k + 1) and dc_p = s v_p of one pair of an item; pn: the item's row
// of Pn.  dc_p costs a (k + d)-wide dot over four gathered rows (Gu_u, Gi_o, Tu_u, P_o) and Pn_r: the k part is formed from the
// registers that hold a_p, the d part in a strided loop (Pn_r: one row per wave, L1-resident).  Contraction off: the same
// roundings wherever it is inlined.
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

// One group of up to NP pairs (cnt of them, wave-uniform): x_p = w.D_p + dc_p, the gradient terms added to acc in pair order, the
// data term of the loss added to lsum (fp64) in pair order (want_loss: the last step).  The one place a pair is evaluated, in
// both forms of every Row; contraction off, so that the roundings do not depend on what the compiler finds around the inlined body.
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

// The walk of the two Rows that gather by index: the pairs [begin, end) (begin a multiple of NP) in groups of NP, 64 pairs'
// indices per batch, one pair per lane.  index(p, ix): the NI clamped indices of pair p; form(it, dl, dc): D and dc of the NP
// pairs with the (wave-uniform) indices it[q]; fn(first pair of the group, D, dc, pairs in the group).
template <int EPL, int NP, int NI, class Index, class Form, class Fn>
__device__ __forceinline__ void index_walk(int begin, int end, int lane, Index &&index, Form &&form, Fn &&fn) {
  for (int base = begin; base < end; base += 64) {
    const int nb = min(64, end - base);
    int ix[NI] = {};
    if (lane < nb) index(base + lane, ix);
    for (int q0 = 0; q0 < nb; q0 += NP) {
      int it[NP][NI];
#pragma unroll
      for (int q = 0; q < NP; ++q) {                           // (a group's tail forms its last pair again: loads in range, unused)
        const int src = min(q0 + q, nb - 1);
#pragma unroll
        for (int c = 0; c < NI; ++c) it[q][c] = __builtin_amdgcn_readfirstlane(__shfl(ix[c], src, 64));
      }
      float dl[NP][EPL], dc[NP];
      form(it, dl, dc);
      fn(base + q0, dl, dc, min(NP, nb - q0));
    }
  }
}

// reg sum_e rv_e w_e^2 over the wave with r1(e) = reg rv_e, nothing fused: the loss side of ItemRow and AfItemRow
template <int EPL, class R1>
__device__ __forceinline__ float reg_loss_plain(const float (&w)[EPL], R1 &&r1) {
#pragma clang fp contract(off)
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < EPL; ++e) s += r1(e) * (w[e] * w[e]);
  return wave_sum(s);
}

// ---- users the model was not trained on (include/bprx.h: bprx_fold_in) ----
template <int EPL>
struct UserRow {
  using Args = FoldArgs;
  static constexpr bool FUSED_GRAD = true;                   // g_e = fma(r2, w_e, acc_e): one rounding
  const FoldArgs &a;
  const int r, lane;
  const int32_t *pos, *neg;
  const RowPlace at;                                         // [gamma | theta]
  float r2n, rn;                                             // 2 reg n_r and reg n_r

  __device__ __forceinline__ UserRow(const FoldArgs &a_, int r_, int64_t p0, int np, int lane_)
      : a(a_), r(r_), lane(lane_), pos(a_.pos + p0), neg(a_.neg + p0),
        at{a_.Gu + (size_t)r_ * a_.k, a_.Tu + (size_t)r_ * a_.d, a_.k, a_.d}, r2n(2.f * a_.reg * (float)np), rn(a_.reg * (float)np) {}

  __device__ __forceinline__ float r2(int) const { return r2n; }

  // reg n_r |w|^2: the squares are summed first and weighted once.  The kernel's first build left the products of an even EPL
  // unfused (they were formed two at a time) and fused the odd one out into the add that takes it: at EPL 3 the third square into
  // the lane's sum, at EPL 1 the only square into the first exchange of the wave sum (which sends the rounded square).
  __device__ __forceinline__ float reg_loss(const float (&w)[EPL]) const {
#pragma clang fp contract(off)
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < (EPL & ~1); ++e) s += w[e] * w[e];
    if (EPL == 1) {
      s = __builtin_fmaf(w[0], w[0], __shfl_xor(w[0] * w[0], 32, 64));
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    } else {
      if (EPL & 1) s = __builtin_fmaf(w[EPL - 1], w[EPL - 1], s);
      s = wave_sum(s);
    }
    return rn * s;
  }

  template <int NP, class Fn>
  __device__ __forceinline__ void walk(int begin, int end, Fn &&fn) const {
    index_walk<EPL, NP, 2>(begin, end, lane,
        [&](int p, int (&ix)[2]) {
          ix[0] = clamp_index(pos[p], a.I, a.errflag, 2);
          ix[1] = clamp_index(neg[p], a.I, a.errflag, 2);
        },
        [&](const int (&it)[NP][2], float (&dl)[NP][EPL], float (&dc)[NP]) {
          float zi[NP][EPL], zj[NP][EPL], ci[NP], cj[NP];    // (the 2 NP rows of the group requested before the first is used)
#pragma unroll
          for (int q = 0; q < NP; ++q) {
            fold_row<EPL>(a, it[q][0], lane, zi[q], ci[q]);
            fold_row<EPL>(a, it[q][1], lane, zj[q], cj[q]);
          }
#pragma unroll
          for (int q = 0; q < NP; ++q) {
#pragma unroll
            for (int e = 0; e < EPL; ++e) dl[q][e] = zi[q][e] - zj[q][e];
            dc[q] = ci[q] - cj[q];
          }
        },
        fn);
  }
};

// ---- items the model was not trained on, once they have first buyers (include/bprx.h: bprx_fold_in_items) ----
template <int EPL>
struct ItemRow {
  using Args = FoldItemArgs;
  static constexpr bool FUSED_GRAD = false;                  // g_e = acc_e + r2_e w_e: two roundings
  const FoldItemArgs &a;
  const int r, lane;
  const int32_t *user, *other, *role;
  const float *pn;
  const RowPlace at;                                         // [Gi_r | Bi_r]
  float rvk, rvb;                                            // rv of the Gi elements and of the bias

  __device__ __forceinline__ ItemRow(const FoldItemArgs &a_, int r_, int64_t p0, int np, int lane_)
      : a(a_), r(r_), lane(lane_), user(a_.user + p0), other(a_.other + p0), role(a_.role + p0),
        pn(a_.d ? a_.Pn + (size_t)r_ * a_.PS : nullptr), at{a_.Gi_rows + (size_t)r_ * a_.k, a_.Bi_rows + r_, a_.k, 1} {
    int npos = 0;                                            // pairs in which the item is the positive
    for (int p = lane; p < np; p += 64) npos += clamp_index(role[p], 2, a.errflag, 2) == 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) npos += __shfl_xor(npos, o, 64);
    // n_pos + c_neg n_neg in one rounding, as this kernel has always formed it
    rvk = (float)np; rvb = __builtin_fmaf(a.cneg, (float)(np - npos), (float)npos);
  }
  __device__ __forceinline__ float rv(int e) const {
    const int col = lane + 64 * e;
    return col < a.k ? rvk : (col < a.k + 1 ? rvb : 0.f);
  }

  __device__ __forceinline__ float r2(int e) const { return 2.f * a.reg * rv(e); }
  __device__ __forceinline__ float reg_loss(const float (&w)[EPL]) const {
    return reg_loss_plain<EPL>(w, [&](int e) { return a.reg * rv(e); });
  }

  template <int NP, class Fn>
  __device__ __forceinline__ void walk(int begin, int end, Fn &&fn) const {
    index_walk<EPL, NP, 3>(begin, end, lane,
        [&](int p, int (&ix)[3]) {
          ix[0] = clamp_index(user[p], a.U, a.errflag, 1);
          ix[1] = clamp_index(other[p], a.I, a.errflag, 2);
          ix[2] = clamp_quiet(role[p], 2);                   // (reported by the count in the constructor)
        },
        [&](const int (&it)[NP][3], float (&dl)[NP][EPL], float (&dc)[NP]) {
#pragma unroll
          for (int q = 0; q < NP; ++q) fold_item_pair<EPL>(a, it[q][0], it[q][1], it[q][2] ? -1.f : 1.f, pn, lane, dl[q], dc[q]);
        },
        fn);
  }
};

// ---- AttentiveFashion items with first buyers (include/bprx.h: bprx_af_fold_in_items) ----
template <int EPL>
struct AfItemRow {
  using Args = AfFoldItemArgs;
  static constexpr bool FUSED_GRAD = false;                  // g_e = acc_e + r2 w_e: two roundings
  const AfFoldItemArgs &a;
  const int r, lane;
  const float *rows;                                         // the work rows of the item's pairs
  const RowPlace at;                                         // Gi_r alone
  float r2n, rn;                                             // 2 reg n_r and reg n_r

  __device__ __forceinline__ AfItemRow(const AfFoldItemArgs &a_, int r_, int64_t p0, int np, int lane_)
      : a(a_), r(r_), lane(lane_), rows(a_.work + (size_t)p0 * a_.KW), at{a_.Gi_rows + (size_t)r_ * a_.k, nullptr, a_.k, 0},
        r2n(2.f * a_.reg * (float)np), rn(a_.reg * (float)np) {}

  __device__ __forceinline__ float r2(int) const { return r2n; }
  __device__ __forceinline__ float reg_loss(const float (&w)[EPL]) const {
    return reg_loss_plain<EPL>(w, [&](int) { return rn; });
  }

  // D (elements lane, lane + 64, ... : zero past k) and dc of pair p
  __device__ __forceinline__ void read_pair(int p, float (&dl)[EPL], float &dc) const {
    const float *row = rows + (size_t)p * a.KW;
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
      const int col = lane + 64 * e;
      dl[e] = col < a.k ? row[col] : 0.f;
    }
    dc = row[a.k];
  }

  // (the pairs are rows already: no index to gather, no batches)
  template <int NP, class Fn>
  __device__ __forceinline__ void walk(int begin, int end, Fn &&fn) const {
    for (int q0 = begin; q0 < end; q0 += NP) {
      float dl[NP][EPL], dc[NP];
#pragma unroll
      for (int q = 0; q < NP; ++q) read_pair(min(q0 + q, end - 1), dl[q], dc[q]);   // (a group's tail reads its last pair again)
      fn(q0, dl, dc, min(NP, end - q0));
    }
  }
};

template <int EPL, template <int> class Row>
__global__ __launch_bounds__(64 * FOLD_WAVES) void k_fold_fit(typename Row<EPL>::Args a) {
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
  const Row<EPL> row(a, r, p0, np, lane);
  float w[EPL], m[EPL], v[EPL];
  row.at.load(lane, w);
#pragma unroll
  for (int e = 0; e < EPL; ++e) { m[e] = 0.f; v[e] = 0.f; }
  float *dls = fold_lds + (size_t)wv * a.share;              // [nc][EPL][64] D, then [nc] dc
  // the first nc pairs live in LDS: all of them where they fit, else as many whole groups as do
  const int fit = a.share / (64 * EPL + 1);
  const int nc = np <= fit ? np : fit / NP * NP;
  float *dcs = dls + (size_t)nc * (64 * EPL);

  if (nc) {
    row.template walk<NP>(0, nc, [&](int q0, const float (&dl)[NP][EPL], const float (&dc)[NP], int cnt) {
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

  for (int t = 1; t <= a.steps; ++t) {
#pragma clang fp contract(off)
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
    if (nc < np) {                                           // (nc is a multiple of NP here: the same groups as from LDS)
      row.template walk<NP>(nc, np, [&](int, const float (&dl)[NP][EPL], const float (&dc)[NP], int cnt) {
        fold_group<EPL, NP>(w, dl, dc, cnt, acc, lsum, last);
      });
    }
    if (last) {                                              // loss_T, before the last update, as train_step returns it
      const float s = row.reg_loss(w);
      if (lane == 0) a.loss[r] = (float)(lsum + (double)s);
    }
    float g[EPL];
#pragma unroll
    for (int e = 0; e < EPL; ++e) g[e] = Row<EPL>::FUSED_GRAD ? __builtin_fmaf(row.r2(e), w[e], acc[e]) : acc[e] + row.r2(e) * w[e];
    if (a.adam) {
      const float tt = (float)t;
      const float lr_t = a.lr * sqrtf(1.0f - powf(a.b2, tt)) / (1.0f - powf(a.b1, tt));
#pragma unroll
      for (int e = 0; e < EPL; ++e) adam_elem(w[e], m[e], v[e], g[e], a.b1, a.b2, lr_t, a.eps);
    } else {
#pragma unroll
      for (int e = 0; e < EPL; ++e) w[e] = w[e] - a.lr * g[e];
    }
  }
  row.at.store(lane, w);
}

// Floats of LDS per wave for the cached pairs: 40 KB per workgroup, so that four workgroups still share a CU (the occupancy the
// registers allow).  Measured at I = 50 000, k = d = 64, 100 000 users, 30 adam steps, ms per call for 8 / 20 / 80 pairs per user
// (profiles/fold_in_share_sweep.jsonl): no LDS 7.57 / 17.09 / 64.69; 1 024 floats 4.90 / 14.85 / 62.38; 1 536 3.50 / 12.52 / 59.95;
// 2 560 3.50 / 7.64 / 54.68; 4 096 (64 KB per workgroup: two workgroups per CU) 5.00 / 9.55 / 88.58.  The item fits take the same
// share (an item's row is k + 1 wide: at k = d = 64 19 pairs fit, where a user's k + d row fits 19 as well -- both are two lane
// words).
constexpr int FOLD_SHARE = 2560;

// The launch of every fit: what the Args share, the grid (one wave per row), the LDS and the EPL for rows `width` wide.
template <template <int> class Row, class Args>
void fold_launch(bprx_handle *h, Args &a, const int64_t *pair_ptr, int64_t n, int steps, bool adam, float lr, float reg, float *loss,
                 int width, hipStream_t s) {
  const bprx_config &c = h->cfg;
  a.ptr = pair_ptr; a.n = (int)n; a.steps = steps; a.adam = adam ? 1 : 0;
  a.lr = lr; a.reg = reg; a.b1 = c.beta1; a.b2 = c.beta2; a.eps = c.epsilon;
  a.loss = loss;
  a.share = h->fold_cache ? FOLD_SHARE : 0;
  const unsigned grid = (unsigned)((n + FOLD_WAVES - 1) / FOLD_WAVES);
  const size_t lds = (size_t)a.share * FOLD_WAVES * sizeof(float);
#define CALL(N) hipLaunchKernelGGL((k_fold_fit<N, Row>), dim3(grid), dim3(64 * FOLD_WAVES), lds, s, a)
  switch ((width + 63) / 64) {
    case 1: CALL(1); break;
    case 2: CALL(2); break;
    case 3: CALL(3); break;
    case 4: CALL(4); break;
    case 5: case 6: CALL(6); break;
    case 7: case 8: CALL(8); break;
    case 9: case 10: case 11: case 12: CALL(12); break;
    default: CALL(16); break;
  }
#undef CALL
}

}  // namespace

int bprx_launch_af_fold_items(bprx_handle *h, const int64_t *pair_ptr, int64_t n, const float *work, int KW, int k, int steps, bool adam,
                              float lr, float reg, float *Gi_rows, float *loss, hipStream_t s) {
  AfFoldItemArgs a;
  a.work = work; a.k = k; a.KW = KW; a.Gi_rows = Gi_rows;
  fold_launch<AfItemRow>(h, a, pair_ptr, n, steps, adam, lr, reg, loss, k, s);
  BPRX_LAUNCH_CHECK(h, "k_fold_fit<AfItemRow>");
  return BPRX_OK;
}

extern "C" int bprx_fold_in(bprx_handle *h, const int64_t *pair_ptr, const int32_t *pos, const int32_t *neg, int64_t n,
                            int32_t steps, float lr, float reg, int32_t optimizer, float *Gu_rows, float *Tu_rows, float *loss,
                            void *stream) {
  if (!h) return BPRX_E_INVALID;
  const bprx_config &c = h->cfg;
  int rc = fold_check_args(h, "fold_in", n, steps, optimizer);
  if (rc) return rc;
  if (c.embed_k + c.embed_d > 1024) BPRX_FAIL(h, BPRX_E_INVALID, "fold_in: k + d = %d > 1024", c.embed_k + c.embed_d);
  if (!pair_ptr || !Gu_rows || (c.embed_d > 0) != (Tu_rows != nullptr)) BPRX_FAIL(h, BPRX_E_INVALID, "fold_in: null pointer");
  if (n && (!pos || !neg)) BPRX_FAIL(h, BPRX_E_INVALID, "fold_in: null pointer");
  hipStream_t s = (hipStream_t)stream;
  // (ACF and AttentiveFashion build the user side from attention: plain handles only)
  rc = bprx_enter(h, "fold_in", NEED_BOUND | NEED_ROWS | NEED_P_ALL, KIND_PLAIN, s);
  if (rc || n == 0) return rc;
  FoldArgs a;
  a.Gi = h->t.Gi; a.Bi = h->t.Bi; a.P = c.embed_d ? h->P : nullptr;
  a.I = c.num_items; a.k = c.embed_k; a.d = c.embed_d; a.PS = h->PS;
  a.pos = pos; a.neg = neg;
  a.Gu = Gu_rows; a.Tu = Tu_rows; a.errflag = h->errflag;
  fold_launch<UserRow>(h, a, pair_ptr, n, steps, optimizer == BPRX_OPT_ADAM_TF23, lr, reg, loss, c.embed_k + c.embed_d, s);
  BPRX_LAUNCH_CHECK(h, "k_fold_fit<UserRow>");
  return BPRX_OK;
}

extern "C" int bprx_fold_in_items(bprx_handle *h, const int64_t *pair_ptr, const int32_t *user, const int32_t *other, const int32_t *role,
                                  int64_t n, const float *Pn, int32_t steps, float lr, float reg, int32_t optimizer, float *Gi_rows,
                                  float *Bi_rows, float *loss, void *stream) {
  if (!h) return BPRX_E_INVALID;
  const bprx_config &c = h->cfg;
  int rc = fold_check_args(h, "fold_in_items", n, steps, optimizer);
  if (rc) return rc;
  if (c.embed_k + 1 > 1024 || c.embed_k + c.embed_d > 1024)
    BPRX_FAIL(h, BPRX_E_INVALID, "fold_in_items: k + 1 = %d or k + d = %d > 1024", c.embed_k + 1, c.embed_k + c.embed_d);
  if (!pair_ptr || !Gi_rows || !Bi_rows || (c.embed_d > 0) != (Pn != nullptr)) BPRX_FAIL(h, BPRX_E_INVALID, "fold_in_items: null pointer");
  if (n && (!user || !other || !role)) BPRX_FAIL(h, BPRX_E_INVALID, "fold_in_items: null pointer");
  if (c.model == BPRX_MODEL_VBPR && c.feat_dtype == BPRX_F_FP8)
    BPRX_FAIL(h, BPRX_E_INVALID, "fold_in_items: fp8 features are not supported for new items (a new row may exceed the max-abs the "
                                 "codes were scaled for and would saturate): fp32 or bf16");
  hipStream_t s = (hipStream_t)stream;
  rc = bprx_enter(h, "fold_in_items", NEED_BOUND | NEED_ROWS | NEED_P_ALL, KIND_PLAIN, s);
  if (rc || n == 0) return rc;
  FoldItemArgs a;
  a.Gu = h->t.Gu; a.Tu = c.embed_d ? h->t.Tu : nullptr; a.Gi = h->t.Gi; a.Bi = h->t.Bi; a.P = c.embed_d ? h->P : nullptr;
  a.Pn = Pn;
  a.U = c.num_users; a.I = c.num_items; a.k = c.embed_k; a.d = c.embed_d; a.PS = h->PS;
  a.user = user; a.other = other; a.role = role;
  a.cneg = h->neg_bias_reg;
  a.Gi_rows = Gi_rows; a.Bi_rows = Bi_rows; a.errflag = h->errflag;
  fold_launch<ItemRow>(h, a, pair_ptr, n, steps, optimizer == BPRX_OPT_ADAM_TF23, lr, reg, loss, c.embed_k + 1, s);
  BPRX_LAUNCH_CHECK(h, "k_fold_fit<ItemRow>");
  return BPRX_OK;
}
