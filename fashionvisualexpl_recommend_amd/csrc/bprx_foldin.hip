// bprx_foldin.hip -- users the model was not trained on (include/bprx.h: bprx_fold_in).
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

}  // namespace

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
