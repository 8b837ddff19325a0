// bprx_factored.hip -- gfx950 kernels of GradFashion's factored projection (GradFashion.py:57-193, 269-292) on a VBPR handle.
//   k_fact_compose  E_eff | Bp_eff = [Ec [E|Bp][:ec] ; Ee [E|Bp][ec:] ; 0]         (bind, every step, bprx_tables_dirty)
//   k_fact_grad     chain rule of the VBPR dense gradient G = dL/d[E_eff|Bp_eff] into the four factor tables
//   k_fact_update   + 2 reg p, sgd or TF-2.3's dense ApplyAdam, pre-update |p|^2 partials for the loss
//   k_fact_explain  predict_ui_grads: gradient x input of x_ui with respect to Fc_i and Fe_i, summed
// Notation: part a = colour (rows [0, Dc) of F, Ec [Dc, ea], rows [0, ea) of A = E and Ap = Bp), part b = edges (rows
// [Dc, Dc + De), Ee [De, eb], rows [ea, ea + eb)).  All fp32; every sum runs in a fixed order (no atomics): a step is
// reproducible bit for bit.  The tables are small (C2 shape: 1024 x 32 + 3072 x 32 + 64 x 65 floats), the gradient G
// ([D, d+1], ~1 MB) is read from L2.
#include "bprx_internal.h"

namespace {

struct FactArgs {
  const float *Ea, *Eb, *A, *Ap;
  int Da, Db, ea, eb, D, d;
};

__device__ __forceinline__ float g_at(const float *__restrict__ G, int D, int d, int row, int n) {
  return n < d ? G[(size_t)row * d + n] : G[(size_t)D * d + row];     // dEp layout: [D*d] dE, then [D] dBp
}

// one thread per element of [D, d+1]: rows past Dc + De (zero feature columns) get zero
__global__ __launch_bounds__(256) void k_fact_compose(FactArgs f, float *__restrict__ E, float *__restrict__ Bp) {
  const int64_t total = (int64_t)f.D * (f.d + 1);
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int r = (int)(e / (f.d + 1)), n = (int)(e % (f.d + 1));
    float acc = 0.f;
    if (r < f.Da + f.Db) {
      const bool pa = r < f.Da;
      const float *Ep = pa ? f.Ea + (size_t)r * f.ea : f.Eb + (size_t)(r - f.Da) * f.eb;
      const int ep = pa ? f.ea : f.eb, off = pa ? 0 : f.ea;
      for (int c = 0; c < ep; ++c) acc += Ep[c] * (n < f.d ? f.A[(size_t)(off + c) * f.d + n] : f.Ap[off + c]);
    }
    if (n < f.d) E[(size_t)r * f.d + n] = acc;
    else Bp[r] = acc;
  }
}

constexpr int FG_T = 1024;       // threads of a k_fact_grad workgroup
// A-gradient blocks: 16 elements x 64 row slices (C2 shape: 260 workgroups of 48 rows per thread; 64 elements x 16 slices left
// 65 workgroups of 192 dependent rows each -- 63 us, the whole of the kernel)
constexpr int FG_COLS = 16;
constexpr int FG_SL = FG_T / FG_COLS;

// gF = [dEa (Da*ea) | dEb (Db*eb) | dA ((ea+eb)*d) | dAp (ea+eb)], each WITH its 2*reg*p term.
// Blocks [0, nb1): one thread per element of Ea | Eb:  dEp[r][c] = sum_n G[row][n] [A|Ap][off+c][n]   (G_p [A|Ap]_p^T)
// Blocks [nb1, ..): FG_COLS elements of [A|Ap] per block, its rows split over FG_SL slices summed in LDS in slice order:
//                   d[A|Ap][off+c][n] = sum_r Ep[r][c] G[r0+r][n]   (Ep^T G_p)
__global__ __launch_bounds__(FG_T) void k_fact_grad(FactArgs f, const float *__restrict__ G, float reg, int nb1,
                                                    float *__restrict__ gF) {
  const int d = f.d, d1 = d + 1, D = f.D;
  const int64_t n1a = (int64_t)f.Da * f.ea, n1 = n1a + (int64_t)f.Db * f.eb;
  if ((int)blockIdx.x < nb1) {
    const int64_t e = (int64_t)blockIdx.x * FG_T + threadIdx.x;
    if (e >= n1) return;
    const bool pa = e < n1a;
    const int ep = pa ? f.ea : f.eb, off = pa ? 0 : f.ea;
    const int64_t el = pa ? e : e - n1a;
    const int r = (int)(el / ep), c = (int)(el % ep), row = pa ? r : f.Da + r;
    const float *a = f.A + (size_t)(off + c) * d;
    float acc = 0.f;
    for (int n = 0; n < d; ++n) acc += G[(size_t)row * d + n] * a[n];
    acc += G[(size_t)D * d + row] * f.Ap[off + c];
    const float p = pa ? f.Ea[el] : f.Eb[el];
    gF[e] = acc + 2.f * reg * p;
    return;
  }
  __shared__ float red[FG_SL][FG_COLS];
  const int nA = (f.ea + f.eb) * d1;
  const int q = threadIdx.x % FG_COLS, sl = threadIdx.x / FG_COLS;
  const int e = ((int)blockIdx.x - nb1) * FG_COLS + q;
  float acc = 0.f;
  int cg = 0, n = 0;
  if (e < nA) {
    cg = e / d1; n = e % d1;
    const bool pa = cg < f.ea;
    const int ep = pa ? f.ea : f.eb, c = pa ? cg : cg - f.ea, Dp = pa ? f.Da : f.Db, r0 = pa ? 0 : f.Da;
    const float *Ep = pa ? f.Ea : f.Eb;
    for (int r = sl; r < Dp; r += FG_SL) acc += Ep[(size_t)r * ep + c] * g_at(G, D, d, r0 + r, n);
  }
  red[sl][q] = acc;
  __syncthreads();
  if (sl == 0 && e < nA) {
    float t = 0.f;
    for (int x = 0; x < FG_SL; ++x) t += red[x][q];
    const float p = n < d ? f.A[(size_t)cg * d + n] : f.Ap[cg];
    const int64_t o = n < d ? n1 + (int64_t)cg * d + n : n1 + (int64_t)(f.ea + f.eb) * d + cg;
    gF[o] = t + 2.f * reg * p;
  }
}

struct FactTables {
  float *p[4], *m[4], *v[4];
  int64_t end[4];     // exclusive end offsets of the four tables in the flat gF order
};

// sgd or the dense ApplyAdam rule (dense_adam_elem; VBPR.py:142 / GradFashion.py:190).
// |p|^2 before the update leaves as one double per block in sqpart[] (k_loss_reduce sums them in block order).
__global__ __launch_bounds__(256) void k_fact_update(FactTables T, const float *__restrict__ gF, int adam, float lr_t, float b1,
                                                     float b2, float eps, double *__restrict__ sqpart) {
  double sq = 0.0;
  const int64_t total = T.end[3];
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int q = e < T.end[0] ? 0 : (e < T.end[1] ? 1 : (e < T.end[2] ? 2 : 3));
    const int64_t o = e - (q ? T.end[q - 1] : 0);
    const float p = T.p[q][o], g = gF[e];
    sq += (double)p * (double)p;
    T.p[q][o] = dense_adam_elem(p, T.m[q] + o, T.v[q] + o, g, adam, lr_t, b1, b2, eps);
  }
  __shared__ double red[4];
  sq = wave_sum(sq);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sq;
  __syncthreads();
  if (threadIdx.x == 0) sqpart[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

__device__ __forceinline__ float feat(const float *F, size_t o) { return F[o]; }
__device__ __forceinline__ float feat(const uint16_t *F, size_t o) { return __uint_as_float((uint32_t)F[o] << 16); }

// One wave per (u, i) pair; lane c holds vf_c = (F_p,i Ep)[c] and w_c = (A_p Tu_u + Ap_p)[c]; out = sum_c vf_c w_c per part.
template <typename FT>
__global__ __launch_bounds__(256) void k_fact_explain(FactArgs f, const FT *__restrict__ F, const float *__restrict__ Tu, int U,
                                                      int I, const int32_t *__restrict__ user, const int32_t *__restrict__ item,
                                                      int64_t n, float *__restrict__ out, int32_t *errflag) {
  const int64_t p = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / 64;
  const int lane = threadIdx.x & 63;
  if (p >= n) return;
  int u = user[p], i = item[p];
  if ((unsigned)u >= (unsigned)U) { if (lane == 0) *errflag = 1; u = u < 0 ? 0 : U - 1; }
  if ((unsigned)i >= (unsigned)I) { if (lane == 0) *errflag = 2; i = i < 0 ? 0 : I - 1; }
  const int d = f.d;
  const FT *Fi = F + (size_t)i * f.D;
  const float *tu = Tu + (size_t)u * d;
  float res[2];
#pragma unroll
  for (int part = 0; part < 2; ++part) {
    const int ep = part ? f.eb : f.ea, off = part ? f.ea : 0, Dp = part ? f.Db : f.Da, r0 = part ? f.Da : 0;
    const float *Ep = part ? f.Eb : f.Ea;
    float acc = 0.f;
    for (int c = lane; c < ep; c += 64) {
      float vf = 0.f;
      for (int r = 0; r < Dp; ++r) vf += feat(Fi, (size_t)(r0 + r)) * Ep[(size_t)r * ep + c];
      const float *a = f.A + (size_t)(off + c) * d;
      float w = f.Ap[off + c];
      for (int x = 0; x < d; ++x) w += a[x] * tu[x];
      acc += vf * w;
    }
    res[part] = wave_sum(acc);
  }
  if (lane == 0) { out[2 * p] = res[0]; out[2 * p + 1] = res[1]; }
}

FactArgs fact_args(const bprx_handle *h) {
  FactArgs f;
  f.Ea = h->fx.Ea; f.Eb = h->fx.Eb; f.A = h->fx.A; f.Ap = h->fx.Ap;
  f.Da = h->fx.feat_dim_a; f.Db = h->fx.feat_dim_b; f.ea = h->fx.embed_a; f.eb = h->fx.embed_b;
  f.D = h->cfg.feat_dim; f.d = h->cfg.embed_d;
  return f;
}

}  // namespace

int bprx_launch_fact_compose(bprx_handle *h, hipStream_t s) {
  const FactArgs f = fact_args(h);
  const int64_t total = (int64_t)f.D * (f.d + 1);
  int64_t blocks = (total + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(k_fact_compose, dim3((unsigned)blocks), dim3(256), 0, s, f, h->t.E, h->t.Bp);
  BPRX_LAUNCH_CHECK(h, "k_fact_compose");
  h->et_valid = h->p_valid = h->absmax_valid = false;
  return BPRX_OK;
}

int bprx_launch_fact_update(bprx_handle *h, float lr_t, hipStream_t s) {
  const FactArgs f = fact_args(h);
  BprxProfScope ps(h, BPRX_PHASE_DENSE, s);
  const int64_t n1 = (int64_t)f.Da * f.ea + (int64_t)f.Db * f.eb;
  const int nA = (f.ea + f.eb) * (f.d + 1);
  const int nb1 = (int)((n1 + FG_T - 1) / FG_T), nb2 = (nA + FG_COLS - 1) / FG_COLS;
  hipLaunchKernelGGL(k_fact_grad, dim3((unsigned)(nb1 + nb2)), dim3(FG_T), 0, s, f, (const float *)h->dEp, h->cfg.reg, nb1, h->gF);
  BPRX_LAUNCH_CHECK(h, "k_fact_grad");
  FactTables T;
  const bprx_factored &x = h->fx;
  float *P[4] = {x.Ea, x.Eb, x.A, x.Ap}, *M[4] = {x.m_Ea, x.m_Eb, x.m_A, x.m_Ap}, *V[4] = {x.v_Ea, x.v_Eb, x.v_A, x.v_Ap};
  const int64_t len[4] = {(int64_t)f.Da * f.ea, (int64_t)f.Db * f.eb, (int64_t)(f.ea + f.eb) * f.d, (int64_t)(f.ea + f.eb)};
  int64_t acc = 0;
  for (int q = 0; q < 4; ++q) { T.p[q] = P[q]; T.m[q] = M[q]; T.v[q] = V[q]; acc += len[q]; T.end[q] = acc; }
  int64_t blocks = (acc + 255) / 256;
  if (blocks > BPRX_DENSE_BLOCKS) blocks = BPRX_DENSE_BLOCKS;
  h->dense_blocks = (int)blocks;
  hipLaunchKernelGGL(k_fact_update, dim3((unsigned)blocks), dim3(256), 0, s, T, (const float *)h->gF,
                     h->cfg.optimizer == BPRX_OPT_ADAM_TF23 ? 1 : 0, lr_t, h->cfg.beta1, h->cfg.beta2, h->cfg.epsilon, h->loss_acc);
  BPRX_LAUNCH_CHECK(h, "k_fact_update");
  return bprx_launch_fact_compose(h, s);
}

int bprx_launch_explain(bprx_handle *h, const int32_t *u, const int32_t *i, int64_t n, float *out, hipStream_t s) {
  const FactArgs f = fact_args(h);
  const int64_t blocks = (n + 3) / 4;            // four waves (pairs) per 256-thread workgroup
  if (h->cfg.feat_dtype == BPRX_F_BF16)
    hipLaunchKernelGGL(k_fact_explain<uint16_t>, dim3((unsigned)blocks), dim3(256), 0, s, f, (const uint16_t *)h->t.F, h->t.Tu,
                       h->cfg.num_users, h->cfg.num_items, u, i, n, out, h->errflag);
  else
    hipLaunchKernelGGL(k_fact_explain<float>, dim3((unsigned)blocks), dim3(256), 0, s, f, (const float *)h->t.F, h->t.Tu,
                       h->cfg.num_users, h->cfg.num_items, u, i, n, out, h->errflag);
  BPRX_LAUNCH_CHECK(h, "k_fact_explain");
  return BPRX_OK;
}
