// bprx_attentive.hip -- AttentiveFashion (AttentiveFashion.py:20-371) on a BPRMF handle: bprx_bind_attentive, bprx_af_*, and what
// bprx_step / bprx_score_pairs / bprx_score_block do on such a handle (include/bprx.h).
//
// Sample rows: a step of B triplets has 2B rows, row r < B = (user r, positive r), row B + r = (user r, negative r).  An item that
// occurs in several rows is OWNED by its first row (islot[item], k_af_claim); a user by its first triplet (uslot[user]).
//   k_af_conv<FWD>    edge encoder forward, one workgroup per owner row: the 228 x 232 zero-padded uint8 image in LDS, im2col
//                     fragments of 2 x 8 pixel tiles read from it, v_mfma_f32_16x16x32_bf16 with the conv weights split into
//                     three bf16 terms (pixels 0..255 are exact in bf16, 1/255 is applied to the sum), bias + relu + 2x2 max in
//                     the accumulator registers (a lane holds the four positions of a window), global mean -> pool [row, 64]
//   k_af_conv<BWD>    edge encoder backward: recomputes each tile exactly as the forward, turns the (argmax, > 0) decisions into
//                     0/1 bf16 B operands and counts  cnt[tap, c] = sum_windows pixel(argmax + tap) * [c active]  with a second
//                     MFMA -- integer sums below 2^24, exact in any order; dW = cnt * g_c / (12544 * 255), db = #active * g_c / 12544
//   k_af_conv<CELL>   bprx_af_explain: the forward's tiles, summed per cell of a G x G grid instead of over the image
//   k_af_rank, k_af_explain   bprx_af_explain: slots of the distinct items; one wave per pair: v, the three parts, the cells, the peak
//   k_af_gemm         the one small fp32 GEMM of the dense encoders, forward and backward (plain HIP, 64 x 64 tiles)
//   k_af_triplet      attention forward + backward, one wave per triplet (both sides)
//   k_af_rowsum       sums the per-row gradients of equal items / users in ascending row order (no float atomics)
//   k_af_colsum       fixed-order column sums (biases, conv partials)
//   k_af_update       sgd / dense ApplyAdam on the thirteen encoder and attention tensors
//   k_af_block        pairwise attention of a user block against every item: f32 MFMA (32x32x2) of the item encodings with the
//                     user's diag(g_u) W_1 staged in LDS, relu . W_2, 3-way softmax and the score in the epilogue
//   k_af_fold         bprx_af_fold_in: one workgroup per new user, one wave per pair: attention forward + backward for the user's
//                     row only, the item side and the encodings frozen, the row's optimiser steps in registers
//   k_af_item_pairs   bprx_af_fold_in_items: one wave per pair of a new item, two attention forwards -> the pair's (D_p, dc_p) of
//                     the linear fit in Gi_r (the step loop is k_fold_fit over AfItemRow, bprx_foldin.hip)
//   k_af_block<., TR> bprx_af_audience_block: the same block for an item window, stored item-major
#include <climits>

#include "bprx_internal.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;

#define AF_IMG BPRX_AF_IMG
#define AF_HID BPRX_AF_HID
#define AF_CH BPRX_AF_CH
#define AF_LP 232                 // bytes per padded image row in LDS: 4 left (2 used), 224, 4 right (2 used)
#define AF_LROWS 228
#define AF_WIN 12544              // 112 x 112 pooling windows
#define AF_CPART (26 * AF_CH)     // conv gradient partial of a row: 25 taps x 64 + 64 bias
#define AF_MAX_H 128
#define AF_MAX_K 512

struct AfState {
  DevPool mem;                    // owns every device buffer below
  bprx_attentive a;
  int k, h, Dc, Dk;
  int64_t R;                      // sample rows of scratch: 2 * max_batch
  int64_t nw[BPRX_AF_NW];
  int64_t step;                   // dropout step index of the next bprx_step
  int32_t *islot, *uslot;         // [I], [U] owner row / triplet; INT_MAX between calls
  int32_t *rowitem, *rowuser;     // [R], [R/2] clamped ids of the rows
  float *pool, *PD;               // [R, 64] pooled conv output of the owner rows; after gather + dropout
  float *Hc, *Hk;                 // [R, 256] hidden units after relu and dropout
  float *C, *dC;                  // [3, R, k] encodings (colour, edges, class) and their gradients
  float *A6, *Hid, *dHid, *da;    // [3R, k] g_u * c_l; [3R, h] hidden, its gradient; [3R] gradient of a_l
  float *dGuS, *dGiS;             // [R/2, k], [R, k] per-triplet / per-row gradients
  float *dH, *dPD, *gsum;         // [R, 256], [R, 64], [R, 64]
  float *cpart, *cred;            // [R, AF_CPART] conv gradient partials; [64, AF_CPART] column-sum stage
  float *g[BPRX_AF_NW];           // gradients of the tensors
  float *Call;                    // [3, I, k] encodings of every item (evaluation)
  float *E;                       // bprx_af_explain: [E_items, G * G, 64] cell sums of a chunk of distinct items (first use)
  size_t E_bytes;
  int32_t *erank;                 // bprx_af_explain: [R] number of owner rows before a row = the slot of its item
  bool eval_valid;
};

// ---- dropout stream ----------------------------------------------------------------------------------------------------
struct AfDrop { uint32_t k0, k1, step, thr; float scale; int on; };   // thr = rate * 2^32; on == 0: no mask, no scaling

// keep bits of units 4q .. 4q+3 of (encoder enc, sample row): bit j set = unit 4q + j kept
__device__ __forceinline__ uint32_t af_keep4(const AfDrop &d, int enc, uint32_t row, uint32_t q) {
  uint32_t o[4];
  philox4x32_10(q, row, (uint32_t)enc, d.step, d.k0, d.k1, o);
  return (o[0] >= d.thr ? 1u : 0u) | (o[1] >= d.thr ? 2u : 0u) | (o[2] >= d.thr ? 4u : 0u) | (o[3] >= d.thr ? 8u : 0u);
}

__global__ __launch_bounds__(256) void k_af_mask(AfDrop d, int64_t n_rows, uint8_t *__restrict__ out) {
  const int64_t per = (int64_t)(AF_HID + AF_CH + AF_HID) / 4 * n_rows;        // groups of four units
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < per; e += (int64_t)gridDim.x * blockDim.x) {
    int enc; int64_t rem = e;
    if (rem < n_rows * (AF_HID / 4)) enc = 0;
    else if ((rem -= n_rows * (AF_HID / 4)) < n_rows * (AF_CH / 4)) enc = 1;
    else { rem -= n_rows * (AF_CH / 4); enc = 2; }
    const int w4 = enc == 1 ? AF_CH / 4 : AF_HID / 4;
    const uint32_t row = (uint32_t)(rem / w4), q = (uint32_t)(rem % w4);
    const uint32_t kb = d.on ? af_keep4(d, enc, row, q) : 15u;
    const int64_t base = (enc == 0 ? 0 : enc == 1 ? n_rows * AF_HID : n_rows * (AF_HID + AF_CH)) + (int64_t)row * (w4 * 4) + q * 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) out[base + j] = (uint8_t)((kb >> j) & 1u);
  }
}

// ---- rows and owners -----------------------------------------------------------------------------------------------------
// row r of n: item = r < nsplit ? ia[r] : ib[r - nsplit]; islot (optional): atomicMin claims the item for its first row.
// users (optional, [nu]): the same for the users' first triplet.
__global__ __launch_bounds__(256) void k_af_claim(const int32_t *__restrict__ ia, const int32_t *__restrict__ ib, int64_t nsplit,
                                                  int64_t n, const int32_t *__restrict__ users, int64_t nu, int I, int U,
                                                  int32_t *__restrict__ rowitem, int32_t *__restrict__ rowuser,
                                                  int32_t *__restrict__ islot, int32_t *__restrict__ uslot, int32_t *errflag) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r < n) {
    const int it = clamp_index(r < nsplit ? ia[r] : ib[r - nsplit], I, errflag, 2);
    rowitem[r] = it;
    if (islot) atomicMin(islot + it, (int32_t)r);
  }
  if (users && r < nu) {
    const int u = clamp_index(users[r], U, errflag, 1);
    rowuser[r] = u;
    if (uslot) atomicMin(uslot + u, (int32_t)r);
  }
}

__global__ __launch_bounds__(256) void k_af_iota(int32_t *__restrict__ rowitem, int64_t n, int32_t first) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r < n) rowitem[r] = first + (int32_t)r;
}

__global__ __launch_bounds__(256) void k_af_release(const int32_t *__restrict__ rowitem, int64_t n, const int32_t *__restrict__ rowuser,
                                                    int64_t nu, int32_t *__restrict__ islot, int32_t *__restrict__ uslot) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r < n) islot[rowitem[r]] = INT_MAX;
  if (r < nu) uslot[rowuser[r]] = INT_MAX;
}

// ---- edge encoder: conv5x5 + bias + relu + maxpool2x2 + global mean, forward and (BWD) weight gradient --------------------
// K slot 8g + j of the MFMA (g = lane >> 4) is tap (ky, kx) = (g, j) for j < 5; the fifth kernel row rides in the spare slots:
// slots 5, 6, 7 = taps (4,0) (4,1) (4,2), slots 13, 14 = taps (4,3) (4,4); every other slot is zero.
__device__ __forceinline__ int af_slot_tap(int g, int j) {
  if (j < 5) return 5 * g + j;
  if (g == 0) return 20 + (j - 5);
  if (g == 1 && j < 7) return 23 + (j - 5);
  return -1;
}
__device__ __forceinline__ uint32_t af_pk(uint32_t p0, uint32_t p1) {        // two pixels -> two bf16 (exact)
  return (__float_as_uint((float)p0) >> 16) | (__float_as_uint((float)p1) & 0xffff0000u);
}
// im2col fragment of MFMA row m = lane & 15 of the tile at window row wy, first window wx0: row m = 4 w + q is position q (row-major
// in its 2x2 window) of window wx0 + w
__device__ __forceinline__ bf16x8 af_patch_frag(const uint8_t *__restrict__ img, int wy, int wx0, int lane) {
  const int m = lane & 15, g = lane >> 4, q = m & 3;
  const int py = 2 * wy + (q >> 1), px = 2 * (wx0 + (m >> 2)) + (q & 1);
  const uint8_t *a = img + (py + g) * AF_LP + px + 2;
  const uint8_t *b = img + (py + 4) * AF_LP + px + 2 + (g == 0 ? 0 : 3);
  const uint32_t p5 = g < 2 ? b[0] : 0u, p6 = g < 2 ? b[1] : 0u, p7 = g == 0 ? b[2] : 0u;
  u32x4 v;
  v[0] = af_pk(a[0], a[1]); v[1] = af_pk(a[2], a[3]); v[2] = af_pk(a[4], p5); v[3] = af_pk(p6, p7);
  return __builtin_bit_cast(bf16x8, v);
}

// MODE: AF_CONV_FWD, AF_CONV_BWD (above), or AF_CONV_CELL: keeps A per region instead of averaging it away,
//   E[e][cell][c] = sum over the windows p of the cell of A_c(p),  cell = (wy / cs) * G + wx / cs,  cs = 112 / G,
// for the owner row's slot e = erank[r] - e0 of the chunk [e0, e0 + ecap).  A window row is computed by the four waves into an LDS
// stage [112 windows][64] (the tiles of four windows may straddle cells: nothing is summed in the MFMA layout), then thread
// (b, c) = (wave + 4 i, lane) adds the cs windows of cell column b (four interleaved partial sums, ascending wx) to its running,
// compensated sum, window rows ascending, and stores the cell after its last row: one fixed order per cell, whichever wave
// produced the window, and no atomics.
enum { AF_CONV_FWD = 0, AF_CONV_BWD = 1, AF_CONV_CELL = 2 };
#define AF_WROW 112               // pooling windows per row / column
struct AfCells { float *E; const int32_t *erank; int G, e0, ecap; };
template <int MODE> struct AfConvOut { typedef float *__restrict__ T; };      // forward: unused; backward: cpart
template <> struct AfConvOut<AF_CONV_CELL> { typedef AfCells T; };

template <int MODE>
__global__ __launch_bounds__(256) void k_af_conv(const uint8_t *__restrict__ edges, const float *__restrict__ cw,
                                                 const float *__restrict__ cb, const int32_t *__restrict__ rowitem,
                                                 const int32_t *__restrict__ islot, int64_t n, float *__restrict__ pool,
                                                 const float *__restrict__ gsum, typename AfConvOut<MODE>::T cpart) {
  constexpr bool BWD = MODE == AF_CONV_BWD, CELL = MODE == AF_CONV_CELL;
  // the image; afterwards the reduction stage.  CELL: followed by the stage of one window row
  __shared__ __attribute__((aligned(16))) uint8_t smem[AF_LROWS * AF_LP + (CELL ? AF_WROW * AF_CH * 4 : 0)];
  const int64_t r = blockIdx.x;
  if (r >= n) return;
  const int item = rowitem[r];
  if (islot && islot[item] != (int32_t)r) return;                             // another row owns this item
  int eslot = 0;
  if constexpr (CELL) {
    eslot = cpart.erank[r] - cpart.e0;
    if ((unsigned)eslot >= (unsigned)cpart.ecap) return;                      // another chunk of the call holds this item
  }
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, cl = lane & 15;
  uint32_t *sm32 = (uint32_t *)smem;
  for (int e = tid; e < AF_LROWS * AF_LP / 4; e += 256) sm32[e] = 0u;
  __syncthreads();
  const uint4 *src = (const uint4 *)(edges + (int64_t)item * (AF_IMG * AF_IMG));
  for (int e = tid; e < AF_IMG * AF_IMG / 16; e += 256) {
    const uint4 v = src[e];
    const int row = e / 14, c16 = e % 14;
    uint32_t *d = sm32 + ((row + 2) * AF_LP + 4 + c16 * 16) / 4;
    d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
  }
  // the conv weights as B operands: channel tile ct, three bf16 terms (hi, mid, lo) of w[tap][16 ct + cl]
  bf16x8 wf[4][3];
  float bias[4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) {
    const int c = 16 * ct + cl;
    bias[ct] = cb[c];
    uint32_t t3[3][8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int tap = af_slot_tap(g, j);
      const float x = tap >= 0 ? cw[tap * AF_CH + c] : 0.f;
      const uint32_t hi = bf16_rne(x);
      const float r1 = x - __uint_as_float(hi << 16);
      const uint32_t mid = bf16_rne(r1);
      const float r2 = r1 - __uint_as_float(mid << 16);
      t3[0][j] = hi; t3[1][j] = mid; t3[2][j] = bf16_rne(r2);
    }
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      u32x4 v;
#pragma unroll
      for (int p = 0; p < 4; ++p) v[p] = t3[t][2 * p] | (t3[t][2 * p + 1] << 16);
      wf[ct][t] = __builtin_bit_cast(bf16x8, v);
    }
  }
  __syncthreads();
  const float inv255 = 1.0f / 255.0f;
  float psum[4] = {0.f, 0.f, 0.f, 0.f};        // forward: sum of the pooled relu; backward: number of active windows
  f32x4 cnt[2][4];
  if (BWD) {
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
      for (int ct = 0; ct < 4; ++ct) cnt[mt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  // tiles of 4 windows: 28 per window row, 3136 per image; wave w takes the pairs (2p, 2p + 1), p = w, w + 4, ...
  // (CELL: of one window row at a time, 14 pairs, then the row is added to the cells)
  constexpr int NROUND = CELL ? AF_WROW : 1, NPR = CELL ? 14 : 1568;
  float *stage = (float *)(smem + AF_LROWS * AF_LP);
  float cacc[CELL ? AF_WROW / 4 : 1], ccmp[4];   // CELL: running cell sums and their compensations
  for (int wr = 0; wr < NROUND; ++wr) {
  for (int pq = w; pq < NPR; pq += 4) {
    const int pr = CELL ? 14 * wr + pq : pq;
    uint32_t ind[4][4];                         // backward: [ct][2 T + (q >> 1)] two 0/1 bf16 of tile T
#pragma unroll
    for (int T = 0; T < 2; ++T) {
      const int tile = 2 * pr + T, wy = tile / 28, wx0 = (tile % 28) * 4;
      const bf16x8 a = af_patch_frag(smem, wy, wx0, lane);
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, wf[ct][2], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, wf[ct][1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, wf[ct][0], acc, 0, 0, 0);
        // this lane: channel 16 ct + cl, window wx0 + g, its four positions in row-major order
        float mx = fmaf(acc[0], inv255, bias[ct]);
        int am = 0;
#pragma unroll
        for (int q = 1; q < 4; ++q) {
          const float v = fmaf(acc[q], inv255, bias[ct]);
          if (v > mx) { mx = v; am = q; }       // the first maximum wins a tie
        }
        if (CELL) {
          stage[(wx0 + g) * AF_CH + 16 * ct + cl] = fmaxf(mx, 0.f);
        } else if (!BWD) {
          psum[ct] += fmaxf(mx, 0.f);
        } else {
          const bool act = mx > 0.f;            // relu'(0) = 0
          psum[ct] += act ? 1.f : 0.f;
          const uint32_t one = 0x3F80u;
          ind[ct][2 * T] = act ? (am == 0 ? one : am == 1 ? one << 16 : 0u) : 0u;
          ind[ct][2 * T + 1] = act ? (am == 2 ? one : am == 3 ? one << 16 : 0u) : 0u;
        }
      }
    }
    if (BWD) {
      // cnt[tap, c] += sum over the 32 positions of the pair: K slot 8g + s is position 4g + (s & 3) of tile s >> 2 -- the
      // positions whose decisions this lane already holds
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        const int tap = 16 * mt + cl;
        const int ky = tap / 5, kx = tap - 5 * ky;
        u32x4 av = {0u, 0u, 0u, 0u};
        if (tap < 25) {
#pragma unroll
          for (int T = 0; T < 2; ++T) {
            const int tile = 2 * pr + T, wy = tile / 28, wx0 = (tile % 28) * 4;
            const uint8_t *p0 = smem + (2 * wy + ky) * AF_LP + 2 * (wx0 + g) + kx + 2;
            av[2 * T] = af_pk(p0[0], p0[1]);
            av[2 * T + 1] = af_pk(p0[AF_LP], p0[AF_LP + 1]);
          }
        }
        const bf16x8 a2 = __builtin_bit_cast(bf16x8, av);
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
          u32x4 bv;
          bv[0] = ind[ct][0]; bv[1] = ind[ct][1]; bv[2] = ind[ct][2]; bv[3] = ind[ct][3];
          cnt[mt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a2, __builtin_bit_cast(bf16x8, bv), cnt[mt][ct], 0, 0, 0);
        }
      }
    }
  }
  if constexpr (CELL) {
    __syncthreads();
    const int G = cpart.G, cs = AF_WROW / G, ca = wr / cs, rin = wr - ca * cs;
    float *Eo = cpart.E + ((size_t)eslot * G * G + (size_t)ca * G) * AF_CH + lane;
#pragma unroll
    for (int i = 0; i < AF_WROW / 4; ++i) {
      const int b = w + 4 * i;                   // cell column of this thread; its channel is the lane
      if (b < G) {
        const float *sp = stage + b * cs * AF_CH + lane;
        // the row's share in four interleaved partial sums, then a compensated (Kahan) add over the rows: a plain running sum
        // over the 12 544 windows of a G = 1 cell rounds every add at the ulp of the whole cell
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        int q = 0;
        for (; q + 3 < cs; q += 4) {
          a0 += sp[q * AF_CH]; a1 += sp[(q + 1) * AF_CH]; a2 += sp[(q + 2) * AF_CH]; a3 += sp[(q + 3) * AF_CH];
        }
        for (; q < cs; ++q) a0 += sp[q * AF_CH];
        // (compensated for cell columns below 16 only: a finer grid, G >= 28, sums at most four rows per cell)
        const float s0 = rin == 0 ? 0.f : cacc[i], c0 = (i < 4 && rin != 0) ? ccmp[i < 4 ? i : 0] : 0.f;
        const float y = ((a0 + a1) + (a2 + a3)) - c0, t = s0 + y;
        if (i < 4) ccmp[i] = (t - s0) - y;
        cacc[i] = t;
        if (rin == cs - 1) Eo[b * AF_CH] = t;
      }
    }
    __syncthreads();
  }
  }
  if constexpr (CELL) return;
  __syncthreads();                               // the image is no longer read: its LDS becomes the reduction stage
  float *red = (float *)smem;                    // [4 waves][4 g][64] sums, then (backward) [4 waves][32 taps][64] counts
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) red[(w * 4 + g) * AF_CH + 16 * ct + cl] = psum[ct];
  if (BWD) {
    float *cs = red + 16 * AF_CH;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
      for (int ct = 0; ct < 4; ++ct)
        for (int q = 0; q < 4; ++q) cs[(w * 32 + 16 * mt + 4 * g + q) * AF_CH + 16 * ct + cl] = cnt[mt][ct][q];
  }
  __syncthreads();
  if constexpr (MODE == AF_CONV_FWD) {
    if (tid < AF_CH) {
      float s = 0.f;
      for (int q = 0; q < 16; ++q) s += red[q * AF_CH + tid];
      pool[r * AF_CH + tid] = s * (1.0f / AF_WIN);
    }
  } else if constexpr (BWD) {
    const float *cs = red + 16 * AF_CH;
    for (int e = tid; e < AF_CPART; e += 256) {
      const int t = e / AF_CH, c = e % AF_CH;
      const float gc = gsum[r * AF_CH + c] * (1.0f / AF_WIN);
      float s = 0.f;
      if (t < 25) {
        for (int q = 0; q < 4; ++q) s += cs[(q * 32 + t) * AF_CH + c];
        cpart[r * AF_CPART + e] = s * (gc * inv255);
      } else {
        for (int q = 0; q < 16; ++q) s += red[q * AF_CH + c];
        cpart[r * AF_CPART + e] = s * gc;
      }
    }
  }
}

// PD[r] = pool[owner row of r's item] with the edge encoder's dropout (encoder 1)
__global__ __launch_bounds__(256) void k_af_pooldrop(const float *__restrict__ pool, const int32_t *__restrict__ rowitem,
                                                     const int32_t *__restrict__ islot, int64_t n, AfDrop d, float *__restrict__ PD) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;            // one thread per four channels
  if (e >= n * (AF_CH / 4)) return;
  const int64_t r = e / (AF_CH / 4);
  const uint32_t q = (uint32_t)(e % (AF_CH / 4));
  const int64_t srow = islot ? islot[rowitem[r]] : r;
  const uint32_t kb = d.on ? af_keep4(d, 1, (uint32_t)r, q) : 15u;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float v = pool[srow * AF_CH + q * 4 + j];
    PD[r * AF_CH + q * 4 + j] = d.on ? ((kb >> j) & 1u ? v * d.scale : 0.f) : v;
  }
}

// ---- the small GEMM of the dense encoders ------------------------------------------------------------------------------------
// C [M, N] = opA [M, K] . opB [K, N];  opA(m, kk) = TA ? A[arow(kk) * lda + m] : A[arow(m) * lda + kk] with arow = rows ? rows[.] : .
// opB(kk, n) = TB ? B[n * ldb + kk] : B[kk * ldb + n].  Epilogue: 0 none; 1: relu(acc + bias[n]), then dropout (encoder enc, row m);
// 2: acc * (gate[m, n] > 0 ? gscale : 0)  (backward through dropout and relu: the stored activation is zero where either cut).
struct AfGemm {
  const float *A, *B, *bias, *gate;
  const int32_t *rows;
  float *C;
  int M, N, K, lda, ldb, ldc, epi, enc;
  float gscale;
  AfDrop d;
};
template <bool TA, bool TB>
__global__ __launch_bounds__(256) void k_af_gemm(AfGemm G) {
  __shared__ float As[16][68], Bs[16][68];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
  float acc[4][4] = {};
  for (int k0 = 0; k0 < G.K; k0 += 16) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int e = tid + 256 * q;
      {
        const int mm = TA ? (e & 63) : (e >> 4), kk = TA ? (e >> 6) : (e & 15);
        float v = 0.f;
        if (m0 + mm < G.M && k0 + kk < G.K) {
          const int64_t ri = TA ? (k0 + kk) : (m0 + mm);
          const int64_t row = G.rows ? G.rows[ri] : ri;
          v = G.A[row * G.lda + (TA ? (m0 + mm) : (k0 + kk))];
        }
        As[kk][mm] = v;
      }
      {
        const int nn = TB ? (e >> 4) : (e & 63), kk = TB ? (e & 15) : (e >> 6);
        float v = 0.f;
        if (n0 + nn < G.N && k0 + kk < G.K) v = TB ? G.B[(int64_t)(n0 + nn) * G.ldb + k0 + kk] : G.B[(int64_t)(k0 + kk) * G.ldb + n0 + nn];
        Bs[kk][nn] = v;
      }
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
      float a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) { a[i] = As[kk][ty * 4 + i]; b[i] = Bs[kk][tx * 4 + i]; }
#pragma unroll
      for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(a[i], b[j], acc[i][j]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + ty * 4 + i;
    if (m >= G.M) continue;
    uint32_t kb = 15u;
    if (G.epi == 1 && G.d.on) kb = af_keep4(G.d, G.enc, (uint32_t)m, (uint32_t)((n0 + tx * 4) >> 2));
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = n0 + tx * 4 + j;
      if (n >= G.N) continue;
      float v = acc[i][j];
      if (G.epi == 1) {
        v = fmaxf(v + G.bias[n], 0.f);
        if (G.d.on) v = (kb >> j) & 1u ? v * G.d.scale : 0.f;
      } else if (G.epi == 2) {
        v = G.gate[(int64_t)m * G.ldc + n] > 0.f ? v * G.gscale : 0.f;
      }
      G.C[(int64_t)m * G.ldc + n] = v;
    }
  }
}

// ---- attention: forward of one (user, item) side --------------------------------------------------------------------------------
struct AfAtt {
  const float *Gu, *Gi, *W1, *b1, *W2, *b2;
  const float *C;                 // [3, ldr, k]
  int64_t ldr;                    // rows of C per component
  int k, h;
};
// The calling wave has gu[k] and cs[3][k] (this side's encodings) in LDS.  Returns a[3]; hid (optional, global [3, ldh, h] at row)
__device__ __forceinline__ void af_att_fwd(const AfAtt &A, const float *gu, const float *cs, int lane, float (&a)[3], float *hid,
                                           int64_t ldh, int64_t row) {
  const int k = A.k, h = A.h;
  float part[3] = {0.f, 0.f, 0.f};
  for (int j = lane; j < h; j += 64) {
    float s[3] = {0.f, 0.f, 0.f};
    for (int c = 0; c < k; ++c) {
      const float w = A.W1[(int64_t)c * h + j], g = gu[c];
#pragma unroll
      for (int l = 0; l < 3; ++l) s[l] = fmaf(g * cs[l * k + c], w, s[l]);
    }
    const float b = A.b1[j], w2 = A.W2[j];
#pragma unroll
    for (int l = 0; l < 3; ++l) {
      const float hv = fmaxf(s[l] + b, 0.f);
      if (hid) hid[((int64_t)l * ldh + row) * h + j] = hv;
      part[l] = fmaf(hv, w2, part[l]);
    }
  }
  const float b2 = A.b2[0];
#pragma unroll
  for (int l = 0; l < 3; ++l) a[l] = wave_sum(part[l]) + b2;
}
__device__ __forceinline__ void af_softmax3(const float (&a)[3], float (&al)[3]) {
  const float m = fmaxf(a[0], fmaxf(a[1], a[2]));
  const float e0 = expf(a[0] - m), e1 = expf(a[1] - m), e2 = expf(a[2] - m);
  const float inv = 1.0f / (e0 + e1 + e2);
  al[0] = e0 * inv; al[1] = e1 * inv; al[2] = e2 * inv;
}

// scores (and attentions) of n pairs whose encodings are rows 0..n of A.C: one wave per pair.  LDS: 4 waves x 4k floats
__global__ __launch_bounds__(256) void k_af_pairs(AfAtt A, const int32_t *__restrict__ rowuser, const int32_t *__restrict__ rowitem,
                                                  int64_t n, float *__restrict__ x, float *__restrict__ alpha) {
  extern __shared__ float sm[];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, k = A.k;
  const int64_t r = (int64_t)blockIdx.x * 4 + w;
  if (r >= n) return;
  float *gu = sm + (size_t)w * 4 * k, *cs = gu + k;
  const int u = rowuser[r], it = rowitem[r];
  for (int c = lane; c < k; c += 64) {
    gu[c] = A.Gu[(int64_t)u * k + c];
#pragma unroll
    for (int l = 0; l < 3; ++l) cs[l * k + c] = A.C[((int64_t)l * A.ldr + r) * k + c];
  }
  wave_sync();
  float a[3], al[3];
  af_att_fwd(A, gu, cs, lane, a, nullptr, 0, 0);
  af_softmax3(a, al);
  float s = 0.f;
  for (int c = lane; c < k; c += 64) {
    const float wf = al[0] * cs[c] + al[1] * cs[k + c] + al[2] * cs[2 * k + c];
    s = fmaf(gu[c] * wf, A.Gi[(int64_t)it * k + c], s);
  }
  s = wave_sum(s);
  if (lane == 0) {
    x[r] = s;
    if (alpha) { alpha[r * 3] = al[0]; alpha[r * 3 + 1] = al[1]; alpha[r * 3 + 2] = al[2]; }
  }
}

// ---- explanations (bprx_af_explain) ------------------------------------------------------------------------------------------------
// erank[r] = number of owner rows before row r (one workgroup, ascending rows): the slot of an owner row's item among the distinct items
__global__ __launch_bounds__(256) void k_af_rank(const int32_t *__restrict__ rowitem, const int32_t *__restrict__ islot, int64_t n,
                                                 int32_t *__restrict__ erank) {
  __shared__ int wsum[4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int base = 0;
  for (int64_t r0 = 0; r0 < n; r0 += 256) {
    const int64_t r = r0 + tid;
    const bool own = r < n && islot[rowitem[r]] == (int32_t)r;
    const unsigned long long mk = __ballot(own);
    if (lane == 0) wsum[w] = __popcll(mk);
    __syncthreads();
    int off = base;
    for (int q = 0; q < w; ++q) off += wsum[q];
    if (r < n) erank[r] = off + __popcll(mk & ((1ull << lane) - 1ull));
    base += wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();
  }
}

// One wave per pair r whose item's cell sums are in this chunk of E.  alpha is what k_af_pairs wrote for the pair (held fixed).
//   t_l = sum_k g_uk c_lk g_ik, parts = alpha_l t_l;   v_c = sum_k W2e[c, k] g_uk g_ik  (lane = channel);
//   cell j = (alpha_e / 12544) sum_c E[j, c] v_c  (lane-strided over the cells, c ascending);  peak = the largest cell, lowest j among equals
// LDS per wave: p[k] = g_u * g_i, v[64]
struct AfExpl {
  AfAtt A;
  const float *W2e, *E, *alpha;
  const int32_t *rowuser, *rowitem, *islot, *erank;
  int64_t n;
  int G, e0, ecap;
  float *parts, *map, *peak_val;
  int32_t *peak_cell;
};
__global__ __launch_bounds__(256) void k_af_explain(AfExpl X) {
  extern __shared__ float sm[];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, k = X.A.k;
  const int64_t r = (int64_t)blockIdx.x * 4 + w;
  if (r >= X.n) return;
  const int it = X.rowitem[r], u = X.rowuser[r];
  const int e = X.erank[X.islot[it]] - X.e0;
  if ((unsigned)e >= (unsigned)X.ecap) return;
  float *p = sm + (size_t)w * (k + AF_CH), *vs = p + k;
  float t[3] = {0.f, 0.f, 0.f};
  for (int c = lane; c < k; c += 64) {
    const float pg = X.A.Gu[(int64_t)u * k + c] * X.A.Gi[(int64_t)it * k + c];
    p[c] = pg;
#pragma unroll
    for (int l = 0; l < 3; ++l) t[l] = fmaf(pg, X.A.C[((int64_t)l * X.A.ldr + r) * k + c], t[l]);
  }
#pragma unroll
  for (int l = 0; l < 3; ++l) t[l] = wave_sum(t[l]);
  wave_sync();
  {
    const float *wr = X.W2e + (int64_t)lane * k;
    float v = 0.f;
    for (int c = 0; c < k; ++c) v = fmaf(wr[c], p[c], v);
    vs[lane] = v;
  }
  wave_sync();
  const float al[3] = {X.alpha[r * 3], X.alpha[r * 3 + 1], X.alpha[r * 3 + 2]};
  if (lane < 3) X.parts[r * 3 + lane] = lane == 0 ? al[0] * t[0] : lane == 1 ? al[1] * t[1] : al[2] * t[2];
  const float scale = al[1] * (1.0f / AF_WIN);
  const int G2 = X.G * X.G;
  const float *Er = X.E + (size_t)e * G2 * AF_CH;
  float bv = -INFINITY;
  int bi = INT_MAX;
  for (int j = lane; j < G2; j += 64) {
    const float4 *row = (const float4 *)(Er + (size_t)j * AF_CH);
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < AF_CH / 4; ++q) {
      const float4 a = row[q];
      s = fmaf(a.x, vs[4 * q], s); s = fmaf(a.y, vs[4 * q + 1], s); s = fmaf(a.z, vs[4 * q + 2], s); s = fmaf(a.w, vs[4 * q + 3], s);
    }
    s *= scale;
    if (X.map) X.map[r * G2 + j] = s;
    if (s > bv) { bv = s; bi = j; }               // ascending j: the first of equal cells stays
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
  }
  if (lane == 0) {
    X.peak_cell[r] = bi == INT_MAX ? 0 : bi;
    X.peak_val[r] = bv;
  }
}

// ---- attention forward + backward of a step: one wave per triplet -------------------------------------------------------------
// LDS per wave: gu[k] cs[2][3][k] dh[6][h]
struct AfTrip {
  AfAtt A;
  float *dC, *A6, *Hid, *dHid, *da, *dGuS, *dGiS, *lossb;
  const int32_t *rowuser, *rowitem;
  int64_t B;
  float reg;
};
__global__ __launch_bounds__(256) void k_af_triplet(AfTrip T) {
  extern __shared__ float sm[];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const AfAtt &A = T.A;
  const int k = A.k, h = A.h;
  const int64_t b = (int64_t)blockIdx.x * 4 + w, B = T.B, R = 2 * B;
  if (b >= B) return;
  float *gu = sm + (size_t)w * (7 * k + 6 * h), *cs = gu + k, *dh = cs + 6 * k;
  const int u = T.rowuser[b];
  const int it[2] = {T.rowitem[b], T.rowitem[B + b]};
  for (int c = lane; c < k; c += 64) {
    gu[c] = A.Gu[(int64_t)u * k + c];
#pragma unroll
    for (int s = 0; s < 2; ++s)
      for (int l = 0; l < 3; ++l) cs[(s * 3 + l) * k + c] = A.C[((int64_t)l * A.ldr + s * B + b) * k + c];
  }
  wave_sync();
  float a[2][3], al[2][3], x[2] = {0.f, 0.f}, nrm = 0.f;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    af_att_fwd(A, gu, cs + s * 3 * k, lane, a[s], T.Hid, R, s * B + b);
    af_softmax3(a[s], al[s]);
  }
  for (int c = lane; c < k; c += 64) {
    const float g = gu[c];
    nrm += g * g;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const float *c3 = cs + s * 3 * k;
      const float gi = A.Gi[(int64_t)it[s] * k + c];
      const float wf = al[s][0] * c3[c] + al[s][1] * c3[k + c] + al[s][2] * c3[2 * k + c];
      x[s] = fmaf(g * wf, gi, x[s]);
      nrm += gi * gi + c3[c] * c3[c] + c3[k + c] * c3[k + c] + c3[2 * k + c] * c3[2 * k + c];
    }
  }
  x[0] = wave_sum(x[0]); x[1] = wave_sum(x[1]); nrm = wave_sum(nrm);
  const float diff = x[0] - x[1];
  const bool inr = (diff >= -80.0f) && (diff <= 1e8f);                 // tf.clip_by_value gradient mask
  const float z = -fminf(fmaxf(diff, -80.0f), 1e8f);
  const float sp = z > 0.f ? z + log1pf(expf(-z)) : log1pf(expf(z));
  const float gd = inr ? -1.0f / (1.0f + expf(diff)) : 0.f;           // d loss / d x_pos = -sigmoid(-diff)
  if (lane == 0) T.lossb[b] = sp + T.reg * nrm;
  const float dx[2] = {gd, -gd}, r2 = 2.f * T.reg;
  // d alpha, then d a through the softmax
  float dav[2][3];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    float dal[3] = {0.f, 0.f, 0.f};
    for (int c = lane; c < k; c += 64) {
      const float t = dx[s] * gu[c] * A.Gi[(int64_t)it[s] * k + c];
#pragma unroll
      for (int l = 0; l < 3; ++l) dal[l] = fmaf(t, cs[(s * 3 + l) * k + c], dal[l]);
    }
#pragma unroll
    for (int l = 0; l < 3; ++l) dal[l] = wave_sum(dal[l]);
    const float dot = al[s][0] * dal[0] + al[s][1] * dal[1] + al[s][2] * dal[2];
#pragma unroll
    for (int l = 0; l < 3; ++l) {
      dav[s][l] = al[s][l] * (dal[l] - dot);
      if (lane == 0) T.da[(int64_t)l * R + s * B + b] = dav[s][l];
    }
  }
  for (int j = lane; j < h; j += 64) {
    const float w2 = A.W2[j];
#pragma unroll
    for (int s = 0; s < 2; ++s)
      for (int l = 0; l < 3; ++l) {
        const int64_t o = ((int64_t)l * R + s * B + b) * h + j;
        const float v = T.Hid[o] > 0.f ? dav[s][l] * w2 : 0.f;
        T.dHid[o] = v;
        dh[(s * 3 + l) * h + j] = v;
      }
  }
  wave_sync();
  for (int c = lane; c < k; c += 64) {
    float dp[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const float *wr = A.W1 + (int64_t)c * h;
    for (int j = 0; j < h; ++j) {
      const float wv = wr[j];
#pragma unroll
      for (int q = 0; q < 6; ++q) dp[q] = fmaf(wv, dh[q * h + j], dp[q]);
    }
    const float g = gu[c];
    float dgu = r2 * g;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const float *c3 = cs + s * 3 * k;
      const float gi = A.Gi[(int64_t)it[s] * k + c];
      const float wf = al[s][0] * c3[c] + al[s][1] * c3[k + c] + al[s][2] * c3[2 * k + c];
      dgu = fmaf(dx[s] * gi, wf, dgu);
      T.dGiS[(s * B + b) * k + c] = dx[s] * g * wf + r2 * gi;
#pragma unroll
      for (int l = 0; l < 3; ++l) {
        const float cv = c3[l * k + c], d = dp[s * 3 + l];
        const int64_t row = (int64_t)l * R + s * B + b;
        T.dC[((int64_t)l * A.ldr + s * B + b) * k + c] = al[s][l] * (dx[s] * g * gi) + g * d + r2 * cv;
        dgu = fmaf(cv, d, dgu);
        T.A6[row * k + c] = g * cv;
      }
    }
    T.dGuS[b * k + c] = dgu;
  }
}

// dst[key] (by_row: dst[r]) [w] = sum over the rows s (ascending) with ids[s] == ids[r] of src[s], for the owner rows r
__global__ __launch_bounds__(256) void k_af_rowsum(const int32_t *__restrict__ ids, const int32_t *__restrict__ slot, int64_t n,
                                                   const float *__restrict__ src, int wdt, float *__restrict__ dst, int by_row) {
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= n) return;
  const int id = ids[r];
  if (slot[id] != (int32_t)r) return;
  float *o = dst + (by_row ? r : (int64_t)id) * wdt;
  for (int c0 = 0; c0 < wdt; c0 += 64) {
    const int c = c0 + lane;
    float s = 0.f;
    for (int64_t base = r; base < n; base += 64) {             // the owner is the first row: earlier rows cannot match
      const int64_t q = base + lane;
      unsigned long long mk = __ballot(q < n && ids[q] == id);
      while (mk) {
        const int t = __ffsll((long long)mk) - 1;
        mk &= mk - 1;
        if (c < wdt) s += src[(base + t) * wdt + c];
      }
    }
    if (c < wdt) o[c] = s;
  }
}

// out[grp][c] = sum of src[r][c] over the rows r of group grp (gsz rows each, ascending); owner rows only when slot is given
__global__ __launch_bounds__(256) void k_af_colsum(const float *__restrict__ src, int64_t n, int ncols, int64_t gsz,
                                                   const int32_t *__restrict__ ids, const int32_t *__restrict__ slot,
                                                   float *__restrict__ out) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t grp = blockIdx.y, r0 = grp * gsz, r1 = r0 + gsz < n ? r0 + gsz : n;
  if (c >= ncols) return;
  float s = 0.f;
  for (int64_t r = r0; r < r1; ++r)
    if (!slot || slot[ids[r]] == (int32_t)r) s += src[r * ncols + c];
  out[grp * ncols + c] = s;
}

// sgd on the owner rows of a table (stage: all-zero between steps)
__global__ __launch_bounds__(256) void k_af_apply_sgd(float *__restrict__ tab, float *__restrict__ stage, const int32_t *__restrict__ ids,
                                                      const int32_t *__restrict__ slot, int64_t n, int k, float lr) {
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= n) return;
  const int id = ids[r];
  if (slot[id] != (int32_t)r) return;
  for (int c = lane; c < k; c += 64) {
    const int64_t o = (int64_t)id * k + c;
    tab[o] -= lr * stage[o];
    stage[o] = 0.f;
  }
}

// the step's loss: per-triplet terms + reg * |attention tensors|^2, one workgroup, fixed order
struct AfDense { float *w[BPRX_AF_NW], *m[BPRX_AF_NW], *v[BPRX_AF_NW], *g[BPRX_AF_NW]; int64_t n[BPRX_AF_NW]; };
__global__ __launch_bounds__(1024) void k_af_loss(AfDense T, float reg, const float *__restrict__ lossb, int64_t B,
                                                  float *__restrict__ loss_out) {
  double sq = 0.0, ls = 0.0;
  for (int q = BPRX_AF_ATT_W1; q < BPRX_AF_NW; ++q)
    for (int64_t e = threadIdx.x; e < T.n[q]; e += 1024) sq += (double)T.w[q][e] * (double)T.w[q][e];
  for (int64_t b = threadIdx.x; b < B; b += 1024) ls += (double)lossb[b];
  const double loss = block_sum_1024(ls + (double)reg * sq);
  if (threadIdx.x == 0 && loss_out) *loss_out = (float)loss;
}

// sgd or TF-2.3 dense ApplyAdam (dense_adam_elem) on every tensor; the attention tensors carry 2 reg w
__global__ __launch_bounds__(256) void k_af_update(AfDense T, int adam, float lr_t, float reg, float b1, float b2, float eps) {
  const float r2 = 2.f * reg;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x, first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int q = 0; q < BPRX_AF_NW; ++q) {
    float *p = T.w[q];
    for (int64_t e = first; e < T.n[q]; e += stride) {
      const float pv = p[e];
      const float g = q >= BPRX_AF_ATT_W1 ? T.g[q][e] + r2 * pv : T.g[q][e];
      p[e] = dense_adam_elem(pv, T.m[q] + e, T.v[q] + e, g, adam, lr_t, b1, b2, eps);
    }
  }
}

// ---- pairwise attention of a user block against every item ----------------------------------------------------------------------
// Workgroup (4 waves): user u0 + blockIdx.y, item tiles blockIdx.x, + gridDim.x, ... of 128 items (32 per wave).
// LDS: Ws[KP][HP] = g_u[c] W_1[c][j] (zero padded), b1s[HP], w2s[HP], gus[KP].  The MFMA runs transposed,
// hidden^T [HP, 32 items] = Ws^T . C_l^T, so that a lane holds 16 hidden units per tile of ONE item (column = lane & 31): the
// relu . W_2 sum stays in the lane, one exchange between the lane halves finishes it.  Lane half hb takes k in [hb KP/2, (hb+1) KP/2).
// Call [3, I, k] and A.Gi [I, k] are the item rows: the catalogue's, or a caller's (bprx_af_score_warm_block).  TR (bprx_af_audience_block):
// the same arithmetic per (u, item) for the items [q0, q1) only, stored item-major, out[(item - q0) * ldo + u] with ldo = num_users.
template <int NJ, bool TR>
__global__ __launch_bounds__(256) void k_af_block(AfAtt A, const float *__restrict__ Call, int I, int u0, int KP,
                                                  float *__restrict__ out, float *__restrict__ alpha, int q0, int q1, int64_t ldo) {
  constexpr int HP = 32 * NJ;
  extern __shared__ float sm[];
  float *Ws = sm, *b1s = Ws + (size_t)KP * HP, *w2s = b1s + HP, *gus = w2s + HP;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, it = lane & 31, hb = lane >> 5;
  const int k = A.k, h = A.h, KH = KP / 2;
  const int64_t ub = blockIdx.y, u = u0 + ub;
  for (int e = tid; e < KP * HP; e += 256) {
    const int c = e / HP, j = e % HP;
    Ws[e] = (c < k && j < h) ? A.Gu[u * k + c] * A.W1[(int64_t)c * h + j] : 0.f;
  }
  for (int j = tid; j < HP; j += 256) { b1s[j] = j < h ? A.b1[j] : 0.f; w2s[j] = j < h ? A.W2[j] : 0.f; }
  for (int c = tid; c < KP; c += 256) gus[c] = c < k ? A.Gu[u * k + c] : 0.f;
  __syncthreads();
  const float b2 = A.b2[0];
  const bool vec = (k % 8) == 0;                 // KP == k: float4 rows
  const int64_t first = TR ? q0 : 0, end = TR ? q1 : I;
  const int64_t tiles = (end - first + 127) / 128;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t item = first + tile * 128 + w * 32 + it;
    const bool ok = item < end;
    const int64_t irow = ok ? item : 0;
    const float *gi = A.Gi + irow * k + hb * KH;
    float a[3], t[3];
#pragma unroll
    for (int l = 0; l < 3; ++l) {
      const float *cl = Call + ((int64_t)l * I + irow) * k + hb * KH;
      f32x16 acc[NJ];
#pragma unroll
      for (int j = 0; j < NJ; ++j)
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
      float tl = 0.f;
      for (int s4 = 0; s4 < KH; s4 += 4) {
        float cv[4], gv[4];
        if (vec) {
          const float4 c4 = *(const float4 *)(cl + s4), g4 = *(const float4 *)(gi + s4);
          cv[0] = c4.x; cv[1] = c4.y; cv[2] = c4.z; cv[3] = c4.w;
          gv[0] = g4.x; gv[1] = g4.y; gv[2] = g4.z; gv[3] = g4.w;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const bool in = hb * KH + s4 + e < k;
            cv[e] = in ? cl[s4 + e] : 0.f;
            gv[e] = in ? gi[s4 + e] : 0.f;
          }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int kk = hb * KH + s4 + e;
          tl = fmaf(cv[e], gus[kk] * gv[e], tl);
#pragma unroll
          for (int j = 0; j < NJ; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(Ws[kk * HP + 32 * j + it], cv[e], acc[j], 0, 0, 0);
        }
      }
      float part = 0.f;
#pragma unroll
      for (int j = 0; j < NJ; ++j)
        for (int r = 0; r < 16; ++r) {
          const int hj = 32 * j + (r & 3) + 8 * (r >> 2) + 4 * hb;
          part = fmaf(fmaxf(acc[j][r] + b1s[hj], 0.f), w2s[hj], part);
        }
      a[l] = part + __shfl_xor(part, 32, 64) + b2;
      t[l] = tl + __shfl_xor(tl, 32, 64);
    }
    float al[3];
    af_softmax3(a, al);
    if (ok && hb == 0) {
      const int64_t o = TR ? (item - first) * ldo + u : ub * I + item;
      out[o] = al[0] * t[0] + al[1] * t[1] + al[2] * t[2];
      if (alpha) { alpha[o * 3] = al[0]; alpha[o * 3 + 1] = al[1]; alpha[o * 3 + 2] = al[2]; }
    }
  }
}

// ---- users the model was not trained on (bprx_af_fold_in) ---------------------------------------------------------------------
// One workgroup per user, resident across the steps; NW = blockDim.x / 64 waves, wave w takes the pairs w, w + NW, ... of a round.
// A pair is 8k floats in LDS: the six encoding rows (positive: colour, edges, class; then the negative) and the two Gi rows.  The
// first nc pairs are gathered once into the cache area and stay there; the others are gathered into the wave's stage every step.
// Either way af_fold_pair is handed an LDS pointer to the same eight rows: one code path, the same bits.  A pair's gradient goes
// to the wave's dg row; after the round's barrier thread c adds the round's rows to its acc in pair order (no atomics).
// LDS (floats): gs[k] | ls[NW] | NW x (stage[8k] hd[6h] dg[k]) | cache[nc x 8k]
struct AfFold {
  AfAtt A;                        // C = Call [3, I, k]; Gu is not read (the rows are the caller's)
  int I;
  const int64_t *ptr;             // [n + 1] pairs of user r: [ptr[r], ptr[r + 1])
  const int32_t *pos, *neg;
  int steps, adam;
  float lr, reg, b1, b2, eps;
  float *Gu, *loss;               // [n, k] in / out; [n] or nullptr
  int32_t *errflag;
  int cache;                      // floats of LDS behind the waves' areas (0: every pair is gathered every step)
};
constexpr int AF_FOLD_EPT = AF_MAX_K / 64;    // elements of g per thread in the smallest workgroup (one wave)

// Forward and backward of one pair for the row gs: returns softplus(-d) and leaves -s (dx(i)/dg - dx(j)/dg) in dg[k].
// rows = cs[2][3][k] gi[2][k], hd[6h] (hidden units, then their gradients): LDS of the calling wave.
__device__ __forceinline__ float af_fold_pair(const AfAtt &A, const float *gs, const float *rows, float *hd, float *dg, int lane) {
  const int k = A.k, h = A.h;
  const float *gi = rows + 6 * k;
  float a[2][3], al[2][3], t[2][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}}, x[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    af_att_fwd(A, gs, rows + s * 3 * k, lane, a[s], hd + s * 3 * h, 1, 0);
    af_softmax3(a[s], al[s]);
  }
  for (int c = lane; c < k; c += 64) {
    const float g = gs[c];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const float pg = g * gi[s * k + c];
#pragma unroll
      for (int l = 0; l < 3; ++l) t[s][l] = fmaf(pg, rows[(s * 3 + l) * k + c], t[s][l]);
    }
  }
#pragma unroll
  for (int s = 0; s < 2; ++s) {
#pragma unroll
    for (int l = 0; l < 3; ++l) t[s][l] = wave_sum(t[s][l]);
    x[s] = al[s][0] * t[s][0] + al[s][1] * t[s][1] + al[s][2] * t[s][2];   // (the form of k_af_block's epilogue)
  }
  const float diff = x[0] - x[1];
  const bool inr = (diff >= -80.0f) && (diff <= 1e8f);                 // tf.clip_by_value gradient mask
  const float z = -fminf(fmaxf(diff, -80.0f), 1e8f);
  const float sp = z > 0.f ? z + log1pf(expf(-z)) : log1pf(expf(z));
  const float gd = inr ? -1.0f / (1.0f + expf(diff)) : 0.f;           // -s_p = -sigmoid(-diff)
  const float dx[2] = {gd, -gd};
  float dav[2][3];                                                     // d loss / d a_l through the softmax
#pragma unroll
  for (int s = 0; s < 2; ++s)
    for (int l = 0; l < 3; ++l) dav[s][l] = dx[s] * al[s][l] * (t[s][l] - x[s]);
  for (int j = lane; j < h; j += 64) {                                 // (a lane reads back the units it wrote itself)
    const float w2 = A.W2[j];
#pragma unroll
    for (int s = 0; s < 2; ++s)
      for (int l = 0; l < 3; ++l) {
        const int o = (s * 3 + l) * h + j;
        hd[o] = hd[o] > 0.f ? dav[s][l] * w2 : 0.f;
      }
  }
  wave_sync();
  for (int c = lane; c < k; c += 64) {
    float dp[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const float *wr = A.W1 + (int64_t)c * h;
    for (int j = 0; j < h; ++j) {
      const float wv = wr[j];
#pragma unroll
      for (int q = 0; q < 6; ++q) dp[q] = fmaf(wv, hd[q * h + j], dp[q]);
    }
    float d = 0.f;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const float *c3 = rows + s * 3 * k;
      const float wf = al[s][0] * c3[c] + al[s][1] * c3[k + c] + al[s][2] * c3[2 * k + c];
      d = fmaf(dx[s] * gi[s * k + c], wf, d);
#pragma unroll
      for (int l = 0; l < 3; ++l) d = fmaf(c3[l * k + c], dp[s * 3 + l], d);
    }
    dg[c] = d;
  }
  return sp;
}

__global__ __launch_bounds__(256) void k_af_fold(AfFold F) {
  extern __shared__ float sm[];
  const AfAtt &A = F.A;
  const int k = A.k, h = A.h, tid = threadIdx.x, lane = tid & 63, w = tid >> 6, NT = blockDim.x, NW = NT >> 6;
  const int64_t r = blockIdx.x;
  const int64_t p0 = F.ptr[r], np64 = F.ptr[r + 1] - p0;
  if (np64 <= 0) {                                           // no pairs: the row stays, the loss is 0 (the whole workgroup leaves)
    if (tid == 0 && F.loss) F.loss[r] = 0.f;
    return;
  }
  const int np = np64 > INT32_MAX ? INT32_MAX : (int)np64;
  const int PW = 8 * k, WS = PW + 6 * h + k;                 // floats of a pair; of a wave's area
  float *gs = sm, *ls = gs + k, *areas = ls + NW, *cache = areas + (size_t)NW * WS;
  float *stage = areas + (size_t)w * WS, *hd = stage + PW, *dg = hd + 6 * h;
  const int fit = F.cache / PW, nc = np < fit ? np : fit;
  const int32_t *pos = F.pos + p0, *neg = F.neg + p0;
  float gw[AF_FOLD_EPT], m[AF_FOLD_EPT], v[AF_FOLD_EPT];
#pragma unroll
  for (int e = 0; e < AF_FOLD_EPT; ++e) {
    const int c = tid + NT * e;
    gw[e] = c < k ? F.Gu[r * k + c] : 0.f;
    m[e] = 0.f; v[e] = 0.f;
    if (c < k) gs[c] = gw[e];
  }
  __syncthreads();
  const float r2n = 2.f * F.reg * (float)np, rn = F.reg * (float)np;
  for (int t = 1; t <= F.steps; ++t) {
    const bool last = t == F.steps && F.loss != nullptr;
    float acc[AF_FOLD_EPT], cmp[AF_FOLD_EPT];                // the gradient sum and its (Kahan) compensation
    double lsum = 0.0;                                       // thread 0: the data term of the loss, in pair order
#pragma unroll
    for (int e = 0; e < AF_FOLD_EPT; ++e) { acc[e] = 0.f; cmp[e] = 0.f; }
    for (int base = 0; base < np; base += NW) {
      const int p = base + w;
      if (p < np) {                                          // (wave-uniform)
        float *rows = p < nc ? cache + (size_t)p * PW : stage;
        if (t == 1 || p >= nc) {
          const int it[2] = {clamp_index(pos[p], F.I, F.errflag, 2), clamp_index(neg[p], F.I, F.errflag, 2)};
          for (int c = lane; c < k; c += 64) {
#pragma unroll
            for (int s = 0; s < 2; ++s) {
#pragma unroll
              for (int l = 0; l < 3; ++l) rows[(s * 3 + l) * k + c] = A.C[((int64_t)l * A.ldr + it[s]) * k + c];
              rows[(6 + s) * k + c] = A.Gi[(int64_t)it[s] * k + c];
            }
          }
        }
        wave_sync();
        const float lp = af_fold_pair(A, gs, rows, hd, dg, lane);
        if (lane == 0) ls[w] = lp;
      }
      __syncthreads();
      const int cnt = np - base < NW ? np - base : NW;
#pragma unroll
      for (int e = 0; e < AF_FOLD_EPT; ++e) {
        const int c = tid + NT * e;
        if (c < k)
          for (int q = 0; q < cnt; ++q) {                    // compensated: thousands of pairs pushing one way must not round
            const float y = areas[(size_t)q * WS + PW + 6 * h + c] - cmp[e];     // every add at the ulp of the whole sum
            const float ts = acc[e] + y;
            cmp[e] = (ts - acc[e]) - y;
            acc[e] = ts;
          }
      }
      if (last && tid == 0)
        for (int q = 0; q < cnt; ++q) lsum += (double)ls[q];
      __syncthreads();
    }
    if (last) {                                              // loss_T, before the last update, as train_step returns it
      if (w == 0) {
        float s = 0.f;
        for (int c = lane; c < k; c += 64) s = fmaf(gs[c], gs[c], s);
        s = wave_sum(s);
        if (lane == 0) F.loss[r] = (float)(lsum + (double)(rn * s));
      }
      __syncthreads();
    }
    const float tt = (float)t;
    const float lr_t = F.adam ? F.lr * sqrtf(1.0f - powf(F.b2, tt)) / (1.0f - powf(F.b1, tt)) : F.lr;
#pragma unroll
    for (int e = 0; e < AF_FOLD_EPT; ++e) {
      const int c = tid + NT * e;
      const float g = acc[e] + r2n * gw[e];
      if (F.adam) adam_elem(gw[e], m[e], v[e], g, F.b1, F.b2, lr_t, F.eps);
      else gw[e] = gw[e] - lr_t * g;
      if (c < k) gs[c] = gw[e];
    }
    __syncthreads();
  }
#pragma unroll
  for (int e = 0; e < AF_FOLD_EPT; ++e) {
    const int c = tid + NT * e;
    if (c < k) F.Gu[r * k + c] = gw[e];
  }
}

// ---- items the model was not trained on, once they have first buyers (bprx_af_fold_in_items) ----------------------------------
// alpha is computed from g_u and the encodings only, so x_ur = Gi_r . m(u, r) is linear in the new item's row: with everything
// else frozen a pair is the (D_p, dc_p) of bprx_fold_in_items' linear-logistic fit, formed ONCE here, one wave per pair; the step
// loop (k_fold_fit over AfItemRow, bprx_foldin.hip) reads them from `work` [pairs, KW] = [D_p (k) | dc_p | zeros].
// LDS of a wave (8k floats): g_u | the new item's three encoding rows | the other item's three rows from Call | Gi_o.
struct AfItemPairs {
  AfAtt A;                        // C = Call [3, I, k]; Gu, Gi the bound tables
  const float *Cn;                // [3, n, k] encodings of the new items
  int U, I;
  int64_t n;
  const int64_t *ptr;             // [n + 1]
  const int32_t *user, *other, *role;
  float *work;
  int KW;
  int32_t *errflag;
};

// D_p and dc_p of one pair from the wave's LDS rows; the one place a pair is formed (contraction off: the same roundings wherever
// it is inlined).  sgn = +1 (role 0) or -1 (role 1): a sign flip of either output, exact.
__device__ __forceinline__ void af_item_pair(const AfAtt &A, const float *gu, const float *cr, const float *co, const float *gio, float sgn,
                                             int lane, float *__restrict__ row, int KW) {
#pragma clang fp contract(off)
  const int k = A.k;
  float a[3], alr[3], alo[3];
  af_att_fwd(A, gu, cr, lane, a, nullptr, 0, 0);
  af_softmax3(a, alr);
  af_att_fwd(A, gu, co, lane, a, nullptr, 0, 0);
  af_softmax3(a, alo);
  float t[3] = {0.f, 0.f, 0.f};
  for (int c = lane; c < k; c += 64) {
    const float wf = alr[0] * cr[c] + alr[1] * cr[k + c] + alr[2] * cr[2 * k + c];      // (the wf form of k_af_pairs)
    row[c] = sgn * (gu[c] * wf);
    const float pg = gu[c] * gio[c];
#pragma unroll
    for (int l = 0; l < 3; ++l) t[l] = fmaf(co[l * k + c], pg, t[l]);                    // (the epilogue form of k_af_block)
  }
#pragma unroll
  for (int l = 0; l < 3; ++l) t[l] = wave_sum(t[l]);
  const float xo = alo[0] * t[0] + alo[1] * t[1] + alo[2] * t[2];
  for (int c = k + lane; c < KW; c += 64) row[c] = c == k ? -sgn * xo : 0.f;
}

// Waves walk the pairs with the grid's stride (the number of pairs is ptr[n], on the device); a pair finds its item by a search of ptr
__global__ __launch_bounds__(256) void k_af_item_pairs(AfItemPairs X) {
  extern __shared__ float sm[];
  const AfAtt &A = X.A;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, k = A.k;
  float *gu = sm + (size_t)w * 8 * k, *cr = gu + k, *co = cr + 3 * k, *gio = co + 3 * k;
  const int64_t P = X.ptr[X.n];
  for (int64_t p = (int64_t)blockIdx.x * 4 + w; p < P; p += (int64_t)gridDim.x * 4) {      // (wave-uniform)
    int64_t lo = 0, hi = X.n;                                // the item r with ptr[r] <= p < ptr[r + 1]: the last r with ptr[r] <= p
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) >> 1;
      if (X.ptr[mid] <= p) lo = mid; else hi = mid;
    }
    const int64_t r = lo;
    const int u = clamp_index(X.user[p], X.U, X.errflag, 1), o = clamp_index(X.other[p], X.I, X.errflag, 2);
    const int role = clamp_index(X.role[p], 2, X.errflag, 2);
    wave_sync();                                             // the previous pair's reads of this area are done
    for (int c = lane; c < k; c += 64) {
      gu[c] = A.Gu[(int64_t)u * k + c];
      gio[c] = A.Gi[(int64_t)o * k + c];
#pragma unroll
      for (int l = 0; l < 3; ++l) {
        cr[l * k + c] = X.Cn[((int64_t)l * X.n + r) * k + c];
        co[l * k + c] = A.C[((int64_t)l * A.ldr + o) * k + c];
      }
    }
    wave_sync();
    af_item_pair(A, gu, cr, co, gio, role ? -1.f : 1.f, lane, X.work + p * X.KW, X.KW);
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------------
static AfDrop af_drop(const AfState *S, int64_t step, bool training) {
  AfDrop d;
  d.k0 = (uint32_t)S->a.seed; d.k1 = (uint32_t)(S->a.seed >> 32); d.step = (uint32_t)step;
  const double rate = S->a.dropout;
  d.on = training && rate > 0.0 ? 1 : 0;
  d.thr = (uint32_t)(rate * 4294967296.0);
  d.scale = (float)(1.0 / (1.0 - rate));
  return d;
}

static int af_gemm(bprx_handle *h, hipStream_t s, bool ta, bool tb, const float *A, int lda, const int32_t *rows, const float *B,
                   int ldb, float *C, int ldc, int M, int N, int K, int epi = 0, const float *bias = nullptr, int enc = 0,
                   const AfDrop *d = nullptr, const float *gate = nullptr, float gscale = 1.f) {
  AfGemm G;
  G.A = A; G.B = B; G.bias = bias; G.gate = gate; G.rows = rows; G.C = C;
  G.M = M; G.N = N; G.K = K; G.lda = lda; G.ldb = ldb; G.ldc = ldc; G.epi = epi; G.enc = enc; G.gscale = gscale;
  if (d) G.d = *d; else memset(&G.d, 0, sizeof(G.d));
  const dim3 grid((N + 63) / 64, (M + 63) / 64);
  if (!ta && !tb) hipLaunchKernelGGL((k_af_gemm<false, false>), grid, dim3(256), 0, s, G);
  else if (ta && !tb) hipLaunchKernelGGL((k_af_gemm<true, false>), grid, dim3(256), 0, s, G);
  else if (!ta && tb) hipLaunchKernelGGL((k_af_gemm<false, true>), grid, dim3(256), 0, s, G);
  else BPRX_FAIL(h, BPRX_E_INVALID, "af_gemm: unsupported form");
  BPRX_LAUNCH_CHECK(h, "k_af_gemm");
  return BPRX_OK;
}

// The per-item inputs the encoders read, indexed by S->rowitem: the bound tables, or a chunk of a caller's (bprx_af_encode_new)
struct AfInputs { const uint8_t *edges; const float *color, *cls; };
static AfInputs af_bound_inputs(const AfState *S) { return AfInputs{S->a.edges, S->a.color, S->a.cls}; }

// The three encodings of rows 0..n (items S->rowitem[r] of `in`) into Cout [3, ldr, k].  dedupe: conv only on the owner rows (islot)
static int af_encode_rows(bprx_handle *h, const AfInputs &in, int64_t n, bool dedupe, const AfDrop &d, float *Cout, int64_t ldr,
                          hipStream_t s) {
  AfState *S = h->af;
  const int k = S->k;
  const int32_t *islot = dedupe ? S->islot : nullptr;
  int rc;
  {
    BprxProfScope ps(h, BPRX_PHASE_PROJ_FWD, s);
    hipLaunchKernelGGL(k_af_conv<AF_CONV_FWD>, dim3((unsigned)n), dim3(256), 0, s, in.edges, S->a.w[BPRX_AF_EDG_CW], S->a.w[BPRX_AF_EDG_CB],
                       S->rowitem, islot, n, S->pool, (const float *)nullptr, (float *)nullptr);
    BPRX_LAUNCH_CHECK(h, "k_af_conv<fwd>");
  }
  hipLaunchKernelGGL(k_af_pooldrop, dim3(bprx_blocks(n * (AF_CH / 4), 256)), dim3(256), 0, s, S->pool, S->rowitem, islot, n, d, S->PD);
  BPRX_LAUNCH_CHECK(h, "k_af_pooldrop");
  if ((rc = af_gemm(h, s, false, false, in.color, S->Dc, S->rowitem, S->a.w[BPRX_AF_COL_W1], AF_HID, S->Hc, AF_HID, (int)n, AF_HID,
                    S->Dc, 1, S->a.w[BPRX_AF_COL_B1], 0, &d))) return rc;
  if ((rc = af_gemm(h, s, false, false, S->Hc, AF_HID, nullptr, S->a.w[BPRX_AF_COL_W2], k, Cout, k, (int)n, k, AF_HID))) return rc;
  if ((rc = af_gemm(h, s, false, false, S->PD, AF_CH, nullptr, S->a.w[BPRX_AF_EDG_W2], k, Cout + ldr * k, k, (int)n, k, AF_CH))) return rc;
  if ((rc = af_gemm(h, s, false, false, in.cls, S->Dk, S->rowitem, S->a.w[BPRX_AF_CLS_W1], AF_HID, S->Hk, AF_HID, (int)n, AF_HID,
                    S->Dk, 1, S->a.w[BPRX_AF_CLS_B1], 2, &d))) return rc;
  return af_gemm(h, s, false, false, S->Hk, AF_HID, nullptr, S->a.w[BPRX_AF_CLS_W2], k, Cout + 2 * ldr * k, k, (int)n, k, AF_HID);
}

static AfAtt af_att(bprx_handle *h, const float *C, int64_t ldr) {
  AfState *S = h->af;
  AfAtt A;
  A.Gu = h->t.Gu; A.Gi = h->t.Gi; A.W1 = S->a.w[BPRX_AF_ATT_W1]; A.b1 = S->a.w[BPRX_AF_ATT_B1]; A.W2 = S->a.w[BPRX_AF_ATT_W2];
  A.b2 = S->a.w[BPRX_AF_ATT_B2]; A.C = C; A.ldr = ldr; A.k = S->k; A.h = S->h;
  return A;
}

// fixed-order column sums of src [n, ncols] into out [ncols] (two levels of at most 64 groups)
static int af_colsum(bprx_handle *h, hipStream_t s, const float *src, int64_t n, int ncols, const int32_t *ids, const int32_t *slot,
                     float *out) {
  AfState *S = h->af;
  const int64_t gsz = (n + 63) / 64, ng = (n + gsz - 1) / gsz;
  hipLaunchKernelGGL(k_af_colsum, dim3((ncols + 255) / 256, (unsigned)ng), dim3(256), 0, s, src, n, ncols, gsz, ids, slot, S->cred);
  hipLaunchKernelGGL(k_af_colsum, dim3((ncols + 255) / 256, 1), dim3(256), 0, s, (const float *)S->cred, ng, ncols, ng,
                     (const int32_t *)nullptr, (const int32_t *)nullptr, out);
  BPRX_LAUNCH_CHECK(h, "k_af_colsum");
  return BPRX_OK;
}

static int af_step_body(bprx_handle *h, const int32_t *user, const int32_t *pos, const int32_t *neg, int64_t B, float *loss_out, hipStream_t s) {
  AfState *S = h->af;
  if (B <= 0) BPRX_FAIL(h, BPRX_E_INVALID, "step: empty batch");
  if (!user || !pos || !neg) BPRX_FAIL(h, BPRX_E_INVALID, "step: null index pointer");
  const int U = h->cfg.num_users, I = h->cfg.num_items, k = S->k, hh = S->h;
  const int64_t R = 2 * B;
  const bool adam = h->cfg.optimizer == BPRX_OPT_ADAM_TF23;
  float lr_t = h->cfg.lr;
  if (adam) {
    h->adam_t += 1;
    lr_t = bprx_adam_lr_t(h);
  }
  h->step.lr_t = lr_t;                                     // (bprx_step_lr)
  const AfDrop d = af_drop(S, S->step, true);
  S->step += 1;
  int rc;
  hipLaunchKernelGGL(k_af_claim, dim3(bprx_blocks(R, 256)), dim3(256), 0, s, pos, neg, B, R, user, B, I, U, S->rowitem, S->rowuser,
                     S->islot, S->uslot, h->errflag);
  BPRX_LAUNCH_CHECK(h, "k_af_claim");
  if ((rc = af_encode_rows(h, af_bound_inputs(S), R, true, d, S->C, S->R, s))) return rc;
  {
    BprxProfScope ps(h, BPRX_PHASE_TRIPLET, s);
    AfTrip T;
    T.A = af_att(h, S->C, S->R);
    T.dC = S->dC; T.A6 = S->A6; T.Hid = S->Hid; T.dHid = S->dHid; T.da = S->da; T.dGuS = S->dGuS; T.dGiS = S->dGiS; T.lossb = h->lossb;
    T.rowuser = S->rowuser; T.rowitem = S->rowitem; T.B = B; T.reg = h->cfg.reg;
    hipLaunchKernelGGL(k_af_triplet, dim3(bprx_blocks(B, 4)), dim3(256), 4 * sizeof(float) * (7 * (size_t)k + 6 * (size_t)hh), s, T);
    BPRX_LAUNCH_CHECK(h, "k_af_triplet");
  }
  AfDense D;
  for (int q = 0; q < BPRX_AF_NW; ++q) { D.w[q] = S->a.w[q]; D.m[q] = S->a.m_w[q]; D.v[q] = S->a.v_w[q]; D.g[q] = S->g[q]; D.n[q] = S->nw[q]; }
  hipLaunchKernelGGL(k_af_loss, dim3(1), dim3(1024), 0, s, D, h->cfg.reg, h->lossb, B, loss_out);
  BPRX_LAUNCH_CHECK(h, "k_af_loss");
  // attention tensors: dW_1 = A6^T dHid, db_1 = colsum dHid, dW_2 = Hid^T da, db_2 = sum da
  if ((rc = af_gemm(h, s, true, false, S->A6, k, nullptr, S->dHid, hh, S->g[BPRX_AF_ATT_W1], hh, k, hh, (int)(3 * R)))) return rc;
  if ((rc = af_colsum(h, s, S->dHid, 3 * R, hh, nullptr, nullptr, S->g[BPRX_AF_ATT_B1]))) return rc;
  if ((rc = af_gemm(h, s, true, false, S->Hid, hh, nullptr, S->da, 1, S->g[BPRX_AF_ATT_W2], 1, hh, 1, (int)(3 * R)))) return rc;
  if ((rc = af_colsum(h, s, S->da, 3 * R, 1, nullptr, nullptr, S->g[BPRX_AF_ATT_B2]))) return rc;
  // dense encoders (colour l = 0, class l = 2): dW2 = H^T dC, dH = (dC W2^T) gated, dW1 = X^T dH, db1 = colsum dH
  for (int l = 0; l < 3; l += 2) {
    const int w1 = l == 0 ? BPRX_AF_COL_W1 : BPRX_AF_CLS_W1, D_in = l == 0 ? S->Dc : S->Dk;
    const float *X = l == 0 ? S->a.color : S->a.cls, *H = l == 0 ? S->Hc : S->Hk, *dC = S->dC + (int64_t)l * S->R * k;
    if ((rc = af_gemm(h, s, true, false, H, AF_HID, nullptr, dC, k, S->g[w1 + 2], k, AF_HID, k, (int)R))) return rc;
    if ((rc = af_gemm(h, s, false, true, dC, k, nullptr, S->a.w[w1 + 2], k, S->dH, AF_HID, (int)R, AF_HID, k, 2, nullptr, 0, nullptr, H,
                      d.on ? d.scale : 1.f))) return rc;
    if ((rc = af_gemm(h, s, true, false, X, D_in, S->rowitem, S->dH, AF_HID, S->g[w1], AF_HID, D_in, AF_HID, (int)R))) return rc;
    if ((rc = af_colsum(h, s, S->dH, R, AF_HID, nullptr, nullptr, S->g[w1 + 1]))) return rc;
  }
  // edge encoder: dW2 = PD^T dC, dPD = (dC W2^T) gated, summed per item, then the conv weight gradient by recomputation
  {
    const float *dC = S->dC + S->R * k;
    if ((rc = af_gemm(h, s, true, false, S->PD, AF_CH, nullptr, dC, k, S->g[BPRX_AF_EDG_W2], k, AF_CH, k, (int)R))) return rc;
    if ((rc = af_gemm(h, s, false, true, dC, k, nullptr, S->a.w[BPRX_AF_EDG_W2], k, S->dPD, AF_CH, (int)R, AF_CH, k, 2, nullptr, 0,
                      nullptr, S->PD, d.on ? d.scale : 1.f))) return rc;
    hipLaunchKernelGGL(k_af_rowsum, dim3(bprx_blocks(R, 4)), dim3(256), 0, s, S->rowitem, S->islot, R, S->dPD, AF_CH, S->gsum, 1);
    BPRX_LAUNCH_CHECK(h, "k_af_rowsum");
    {
      BprxProfScope ps(h, BPRX_PHASE_PROJ_BWD, s);
      hipLaunchKernelGGL(k_af_conv<AF_CONV_BWD>, dim3((unsigned)R), dim3(256), 0, s, S->a.edges, S->a.w[BPRX_AF_EDG_CW], S->a.w[BPRX_AF_EDG_CB],
                         S->rowitem, S->islot, R, (float *)nullptr, S->gsum, S->cpart);
      BPRX_LAUNCH_CHECK(h, "k_af_conv<bwd>");
    }
    // g[EDG_CW] [25 * 64] and g[EDG_CB] [64] are one allocation of AF_CPART floats
    if ((rc = af_colsum(h, s, S->cpart, R, AF_CPART, S->rowitem, S->islot, S->g[BPRX_AF_EDG_CW]))) return rc;
  }
  // Gu / Gi: per-row gradients summed per distinct row in ascending row order into the staging tables
  hipLaunchKernelGGL(k_af_rowsum, dim3(bprx_blocks(R, 4)), dim3(256), 0, s, S->rowitem, S->islot, R, S->dGiS, k, h->dGi, 0);
  hipLaunchKernelGGL(k_af_rowsum, dim3(bprx_blocks(B, 4)), dim3(256), 0, s, S->rowuser, S->uslot, B, S->dGuS, k, h->dGu, 0);
  BPRX_LAUNCH_CHECK(h, "k_af_rowsum");
  {
    BprxProfScope ps(h, BPRX_PHASE_DENSE, s);
    hipLaunchKernelGGL(k_af_update, dim3(256), dim3(256), 0, s, D, adam ? 1 : 0, lr_t, h->cfg.reg, h->cfg.beta1, h->cfg.beta2,
                       h->cfg.epsilon);
    BPRX_LAUNCH_CHECK(h, "k_af_update");
  }
  {
    BprxProfScope ps(h, BPRX_PHASE_APPLY, s);
    if (adam) {
      AdamSweepAll W = {};                                   // every row of Gu and Gi moves every step
      W.seg[0] = {h->t.Gu, h->t.m_Gu, h->t.v_Gu, h->dGu, (size_t)U * k};
      W.seg[1] = {h->t.Gi, h->t.m_Gi, h->t.v_Gi, h->dGi, (size_t)I * k};
      if ((rc = bprx_launch_adam_sweep(h, W, lr_t, s))) return rc;
    } else {
      hipLaunchKernelGGL(k_af_apply_sgd, dim3(bprx_blocks(R, 4)), dim3(256), 0, s, h->t.Gi, h->dGi, S->rowitem, S->islot, R, k, lr_t);
      hipLaunchKernelGGL(k_af_apply_sgd, dim3(bprx_blocks(B, 4)), dim3(256), 0, s, h->t.Gu, h->dGu, S->rowuser, S->uslot, B, k, lr_t);
      BPRX_LAUNCH_CHECK(h, "k_af_apply_sgd");
    }
  }
  return BPRX_OK;
}

// The owner slots are released on every path: a step that failed half way must not leave items and users claimed.
int bprx_af_step(bprx_handle *h, const int32_t *user, const int32_t *pos, const int32_t *neg, int64_t B, float *loss_out, hipStream_t s) {
  AfState *S = h->af;
  const int rc = af_step_body(h, user, pos, neg, B, loss_out, s);
  S->eval_valid = false;
  if (B > 0 && user && pos && neg) {                         // the claim kernel ran (or was at least tried): rowitem / rowuser name the rows
    hipLaunchKernelGGL(k_af_release, dim3(bprx_blocks(2 * B, 256)), dim3(256), 0, s, S->rowitem, 2 * B, S->rowuser, B, S->islot, S->uslot);
    if (!rc) BPRX_LAUNCH_CHECK(h, "k_af_release");
  }
  return rc;
}

int bprx_af_pairs(bprx_handle *h, const int32_t *user, const int32_t *item, int64_t n, float *x, float *alpha, hipStream_t s) {
  AfState *S = h->af;
  if (n > S->R) BPRX_FAIL(h, BPRX_E_INVALID, "attentive pairs: n = %lld > 2 * max_batch", (long long)n);
  int rc;
  hipLaunchKernelGGL(k_af_claim, dim3(bprx_blocks(n, 256)), dim3(256), 0, s, item, item, n, n, user, n, h->cfg.num_items, h->cfg.num_users,
                     S->rowitem, S->rowuser, (int32_t *)nullptr, (int32_t *)nullptr, h->errflag);
  BPRX_LAUNCH_CHECK(h, "k_af_claim");
  const AfDrop d = af_drop(S, 0, false);
  if ((rc = af_encode_rows(h, af_bound_inputs(S), n, false, d, S->C, S->R, s))) return rc;
  hipLaunchKernelGGL(k_af_pairs, dim3(bprx_blocks(n, 4)), dim3(256), 16 * sizeof(float) * (size_t)S->k, s, af_att(h, S->C, S->R), S->rowuser,
                     S->rowitem, n, x, alpha);
  BPRX_LAUNCH_CHECK(h, "k_af_pairs");
  return BPRX_OK;
}

// bprx_af_explain after its argument checks and with the workspace in place.  Items are claimed (islot); the caller releases them.
static int af_explain_body(bprx_handle *h, const int32_t *user, const int32_t *item, int64_t n, int G, float *x, float *alpha,
                           float *parts, float *map, int32_t *peak_cell, float *peak_val, int64_t ecap, hipStream_t s) {
  AfState *S = h->af;
  int rc;
  hipLaunchKernelGGL(k_af_claim, dim3(bprx_blocks(n, 256)), dim3(256), 0, s, item, item, n, n, user, n, h->cfg.num_items, h->cfg.num_users,
                     S->rowitem, S->rowuser, S->islot, (int32_t *)nullptr, h->errflag);
  BPRX_LAUNCH_CHECK(h, "k_af_claim");
  // x and alpha: the kernels of bprx_af_attention_pairs; the conv runs on the owner rows only and gives the same bits per item
  const AfDrop d = af_drop(S, 0, false);
  if ((rc = af_encode_rows(h, af_bound_inputs(S), n, true, d, S->C, S->R, s))) return rc;
  hipLaunchKernelGGL(k_af_pairs, dim3(bprx_blocks(n, 4)), dim3(256), 16 * sizeof(float) * (size_t)S->k, s, af_att(h, S->C, S->R), S->rowuser,
                     S->rowitem, n, x, alpha);
  BPRX_LAUNCH_CHECK(h, "k_af_pairs");
  hipLaunchKernelGGL(k_af_rank, dim3(1), dim3(256), 0, s, S->rowitem, S->islot, n, S->erank);
  BPRX_LAUNCH_CHECK(h, "k_af_rank");
  // the distinct items in chunks of ecap slots (their number is not read back: at most n, the later chunks may be empty)
  for (int64_t e0 = 0; e0 < n; e0 += ecap) {
    AfCells Cc;
    Cc.E = S->E; Cc.erank = S->erank; Cc.G = G; Cc.e0 = (int)e0; Cc.ecap = (int)ecap;
    {
      BprxProfScope ps(h, BPRX_PHASE_PROJ_FWD, s);
      hipLaunchKernelGGL(k_af_conv<AF_CONV_CELL>, dim3((unsigned)n), dim3(256), 0, s, S->a.edges, S->a.w[BPRX_AF_EDG_CW],
                         S->a.w[BPRX_AF_EDG_CB], S->rowitem, S->islot, n, (float *)nullptr, (const float *)nullptr, Cc);
      BPRX_LAUNCH_CHECK(h, "k_af_conv<cell>");
    }
    AfExpl X;
    X.A = af_att(h, S->C, S->R);
    X.W2e = S->a.w[BPRX_AF_EDG_W2]; X.E = S->E; X.alpha = alpha;
    X.rowuser = S->rowuser; X.rowitem = S->rowitem; X.islot = S->islot; X.erank = S->erank;
    X.n = n; X.G = G; X.e0 = (int)e0; X.ecap = (int)ecap;
    X.parts = parts; X.map = map; X.peak_val = peak_val; X.peak_cell = peak_cell;
    hipLaunchKernelGGL(k_af_explain, dim3(bprx_blocks(n, 4)), dim3(256), 4 * sizeof(float) * ((size_t)S->k + AF_CH), s, X);
    BPRX_LAUNCH_CHECK(h, "k_af_explain");
  }
  return BPRX_OK;
}

// encodings of items first .. first + n (consecutive) or of a list, in chunks of R rows, into out [3, ld, k] at row offset
static int af_encode_many(bprx_handle *h, const int32_t *items, int64_t n, float *out, int64_t ld, hipStream_t s) {
  AfState *S = h->af;
  const AfDrop d = af_drop(S, 0, false);
  const size_t kb = (size_t)S->k * sizeof(float);
  for (int64_t r0 = 0; r0 < n; r0 += S->R) {
    const int64_t m = n - r0 < S->R ? n - r0 : S->R;
    if (items)
      hipLaunchKernelGGL(k_af_claim, dim3(bprx_blocks(m, 256)), dim3(256), 0, s, items + r0, items + r0, m, m, (const int32_t *)nullptr,
                         (int64_t)0, h->cfg.num_items, h->cfg.num_users, S->rowitem, S->rowuser, (int32_t *)nullptr, (int32_t *)nullptr,
                         h->errflag);
    else
      hipLaunchKernelGGL(k_af_iota, dim3(bprx_blocks(m, 256)), dim3(256), 0, s, S->rowitem, m, (int32_t)r0);
    BPRX_LAUNCH_CHECK(h, "k_af_claim");
    int rc;
    if ((rc = af_encode_rows(h, af_bound_inputs(S), m, false, d, S->C, S->R, s))) return rc;
    for (int l = 0; l < 3; ++l)
      BPRX_HIP(h, hipMemcpyAsync(out + ((int64_t)l * ld + r0) * S->k, S->C + (int64_t)l * S->R * S->k, m * kb, hipMemcpyDeviceToDevice, s));
  }
  return BPRX_OK;
}

// Call = the dropout-off encodings of every item for the bound parameter state (a bprx_step invalidates it)
static int af_call_current(bprx_handle *h, hipStream_t s) {
  AfState *S = h->af;
  if (S->eval_valid) return BPRX_OK;
  const int I = h->cfg.num_items;
  const int rc = af_encode_many(h, nullptr, I, S->Call, I, s);
  if (!rc) S->eval_valid = true;
  return rc;
}

// k_af_block for the users [u0, u1) of A.Gu against the I item rows (Call, A.Gi): user-major out [(u1 - u0), I], or with tr the
// items [q0, q1) item-major, out [(q1 - q0), ldo] (u0 = 0: the column of a user is its id)
static int af_block_run(bprx_handle *h, const AfAtt &A, const float *Call, int I, int32_t u0, int32_t u1, float *out, float *alpha,
                        hipStream_t s, bool tr = false, int q0 = 0, int q1 = 0, int64_t ldo = 0) {
  AfState *S = h->af;
  const int KP = (S->k + 7) / 8 * 8, NJ = (S->h + 31) / 32;
  const size_t lds = sizeof(float) * ((size_t)KP * 32 * NJ + 64 * NJ + KP);
  const int64_t tiles = tr ? ((int64_t)q1 - q0 + 127) / 128 : ((int64_t)I + 127) / 128;
  for (int32_t c0 = u0; c0 < u1; c0 += 32768) {              // gridDim.y holds the users: at most 65 535 per launch
    const int32_t c1 = u1 - c0 < 32768 ? u1 : c0 + 32768;
    const dim3 grid((unsigned)(tiles < 16 ? tiles : 16), (unsigned)(c1 - c0));
    float *o = tr ? out : out + (int64_t)(c0 - u0) * I, *al = !alpha || tr ? alpha : alpha + (int64_t)(c0 - u0) * I * 3;
#define AF_BLOCK(NJ_)                                                                                                         \
  if (tr) hipLaunchKernelGGL((k_af_block<NJ_, true>), grid, dim3(256), lds, s, A, Call, I, c0, KP, o, al, q0, q1, ldo);      \
  else hipLaunchKernelGGL((k_af_block<NJ_, false>), grid, dim3(256), lds, s, A, Call, I, c0, KP, o, al, 0, 0, (int64_t)0);
    switch (NJ) {
      case 1: AF_BLOCK(1) break;
      case 2: AF_BLOCK(2) break;
      case 3: AF_BLOCK(3) break;
      default: AF_BLOCK(4) break;
    }
#undef AF_BLOCK
    BPRX_LAUNCH_CHECK(h, "k_af_block");
  }
  return BPRX_OK;
}

int bprx_af_block(bprx_handle *h, int32_t u0, int32_t u1, float *out, float *alpha, hipStream_t s, const float *Gu_rows) {
  AfState *S = h->af;
  const int I = h->cfg.num_items;
  int rc;
  if ((rc = af_call_current(h, s))) return rc;
  AfAtt A = af_att(h, S->Call, I);
  if (Gu_rows) A.Gu = Gu_rows;
  return af_block_run(h, A, S->Call, I, u0, u1, out, alpha, s);
}

void bprx_af_invalidate(bprx_handle *h) {
  if (h->af) h->af->eval_valid = false;
}

void bprx_af_free(bprx_handle *h) {
  delete h->af;
  h->af = nullptr;
}

int bprx_bind_tables_internal(bprx_handle *h, const bprx_tables *t);

extern "C" int bprx_bind_attentive(bprx_handle *h, const bprx_tables *t, const bprx_attentive *a) {
  if (!h || !t || !a) return BPRX_E_INVALID;
  const bprx_config &c = h->cfg;
  if (c.model != BPRX_MODEL_BPRMF) BPRX_FAIL(h, BPRX_E_INVALID, "bind_attentive: needs a BPRMF handle");
  if (c.flags & (BPRX_FLAG_EXPORT_USER_GRAD | BPRX_FLAG_EXPORT_ITEM_GRAD))
    BPRX_FAIL(h, BPRX_E_INVALID, "bind_attentive: exported gradients (multi-GPU) are not supported");
  if (a->dim_color <= 0 || a->dim_class <= 0) BPRX_FAIL(h, BPRX_E_INVALID, "bind_attentive: Dc = %d, Dk = %d must be positive", a->dim_color, a->dim_class);
  if (a->width <= 0 || a->width > AF_MAX_H) BPRX_FAIL(h, BPRX_E_INVALID, "bind_attentive: width = %d outside [1, %d]", a->width, AF_MAX_H);
  if (c.embed_k > AF_MAX_K) BPRX_FAIL(h, BPRX_E_INVALID, "bind_attentive: embed_k %d > %d", c.embed_k, AF_MAX_K);
  if (!(a->dropout >= 0.f && a->dropout < 1.f)) BPRX_FAIL(h, BPRX_E_INVALID, "bind_attentive: dropout = %g outside [0, 1)", (double)a->dropout);
  if (!a->edges || !a->color || !a->cls) BPRX_FAIL(h, BPRX_E_INVALID, "bind_attentive: edges, color and cls are required");
  if ((uintptr_t)a->edges & 15) BPRX_FAIL(h, BPRX_E_INVALID, "bind_attentive: edges must be 16-byte aligned");
  const int KP = (c.embed_k + 7) / 8 * 8, HP = (a->width + 31) / 32 * 32;
  if (KP * HP > 15360) BPRX_FAIL(h, BPRX_E_INVALID, "bind_attentive: embed_k %d x width %d needs more LDS than a workgroup has", c.embed_k, a->width);
  if (4 * (7 * (size_t)c.embed_k + 6 * (size_t)a->width) * sizeof(float) > 65536)
    BPRX_FAIL(h, BPRX_E_INVALID, "bind_attentive: embed_k %d x width %d needs more LDS than a workgroup has", c.embed_k, a->width);
  const bool adam = c.optimizer == BPRX_OPT_ADAM_TF23;
  for (int q = 0; q < BPRX_AF_NW; ++q) {
    if (!a->w[q]) BPRX_FAIL(h, BPRX_E_INVALID, "bind_attentive: tensor %d is missing", q);
    if (adam && (!a->m_w[q] || !a->v_w[q])) BPRX_FAIL(h, BPRX_E_INVALID, "bind_attentive: adam_tf23 needs m_/v_ slots of tensor %d", q);
  }
  AfState *S = h->af;
  const int64_t keep_step = S ? S->step : 0;
  if (S) bprx_af_free(h), S = nullptr;
  if (h->acf) bprx_acf_free(h);
  int rc = bprx_bind_tables_internal(h, t);
  if (rc) return rc;
  // TF-2.3's Adam moves every row every step: the handle takes the whole-table sweeps (bring lazily held rows up to date first)
  if (h->adam_lazy) {
    if ((rc = bprx_launch_adam_sync(h, h->adam_t, nullptr))) return rc;
    BPRX_HIP(h, hipStreamSynchronize(nullptr));
    h->adam_lazy = false;
  }
  const size_t U = c.num_users, I = c.num_items, k = c.embed_k, R = 2 * (size_t)c.max_batch, hh = a->width;
  S = new (std::nothrow) AfState();
  if (!S) BPRX_FAIL(h, BPRX_E_NOMEM, "bind_attentive: out of host memory");
  h->af = S;
  S->a = *a; S->k = (int)k; S->h = (int)hh; S->Dc = a->dim_color; S->Dk = a->dim_class; S->R = (int64_t)R; S->step = keep_step;
  const int64_t Dc = S->Dc, Dk = S->Dk;
  const int64_t nw[BPRX_AF_NW] = {Dc * AF_HID, AF_HID, AF_HID * (int64_t)k, 25 * AF_CH, AF_CH, AF_CH * (int64_t)k, Dk * AF_HID, AF_HID,
                                  AF_HID * (int64_t)k, (int64_t)(k * hh), (int64_t)hh, (int64_t)hh, 1};
  DevPool &A = S->mem;
  for (int q = 0; q < BPRX_AF_NW; ++q) {
    S->nw[q] = nw[q];
    if (q == BPRX_AF_EDG_CW) A.zeros(&S->g[q], (size_t)AF_CPART);
    else if (q == BPRX_AF_EDG_CB) S->g[q] = S->g[BPRX_AF_EDG_CW] ? S->g[BPRX_AF_EDG_CW] + 25 * AF_CH : nullptr;   // an alias, not owned
    else A.zeros(&S->g[q], (size_t)nw[q]);
  }
  A.zeros(&S->islot, I);
  A.zeros(&S->uslot, U);
  A.zeros(&S->rowitem, R);
  A.zeros(&S->rowuser, R);
  A.zeros(&S->pool, R * AF_CH);
  A.zeros(&S->PD, R * AF_CH);
  A.zeros(&S->Hc, R * AF_HID);
  A.zeros(&S->Hk, R * AF_HID);
  A.zeros(&S->C, 3 * R * k);
  A.zeros(&S->dC, 3 * R * k);
  A.zeros(&S->A6, 3 * R * k);
  A.zeros(&S->Hid, 3 * R * hh);
  A.zeros(&S->dHid, 3 * R * hh);
  A.zeros(&S->da, 3 * R);
  A.zeros(&S->dGuS, R / 2 * k);
  A.zeros(&S->dGiS, R * k);
  A.zeros(&S->dH, R * AF_HID);
  A.zeros(&S->dPD, R * AF_CH);
  A.zeros(&S->gsum, R * AF_CH);
  A.zeros(&S->cpart, R * AF_CPART);
  A.zeros(&S->cred, 64 * (size_t)AF_CPART);
  A.zeros(&S->Call, 3 * I * k);
  if (!A.ok()) {
    bprx_af_free(h);
    BPRX_FAIL(h, BPRX_E_NOMEM, "bind_attentive: scratch allocation failed");
  }
  S->eval_valid = false;
  if ((rc = bprx_launch_fill_i32(h, S->islot, I, (int32_t)INT_MAX, nullptr)) ||
      (rc = bprx_launch_fill_i32(h, S->uslot, U, (int32_t)INT_MAX, nullptr))) {
    bprx_af_free(h);
    return rc;
  }
  const hipError_t e = hipStreamSynchronize(nullptr);
  if (e == hipSuccess) return BPRX_OK;
  bprx_af_free(h);                                          // no failure leaves a model state on the handle
  BPRX_FAIL(h, BPRX_E_HIP, "bind_attentive: hipStreamSynchronize(nullptr): %s", hipGetErrorString(e));
}

#define AF_CHECK(name)                                                                                              \
  if (!h) return BPRX_E_INVALID;                                                                                    \
  if (!h->bound || !h->af) BPRX_FAIL(h, BPRX_E_STATE, name ": the handle is not bound with bprx_bind_attentive");

extern "C" int bprx_af_encode(bprx_handle *h, const int32_t *items, int64_t n, float *out, void *stream) {
  AF_CHECK("af_encode")
  if (n < 0 || n > ((int64_t)1 << 31) - 1) BPRX_FAIL(h, BPRX_E_INVALID, "af_encode: n = %lld out of range", (long long)n);
  if (n == 0) return BPRX_OK;
  if (!items || !out) BPRX_FAIL(h, BPRX_E_INVALID, "af_encode: null pointer");
  return af_encode_many(h, items, n, out, n, (hipStream_t)stream);
}

extern "C" int bprx_af_attention_pairs(bprx_handle *h, const int32_t *user, const int32_t *item, int64_t n, float *x, float *alpha,
                                       void *stream) {
  AF_CHECK("af_attention_pairs")
  if (n < 0 || n > h->cfg.max_batch) BPRX_FAIL(h, BPRX_E_INVALID, "af_attention_pairs: n = %lld outside [0, max_batch]", (long long)n);
  if (n == 0) return BPRX_OK;
  if (!user || !item || !x) BPRX_FAIL(h, BPRX_E_INVALID, "af_attention_pairs: null pointer");
  return bprx_af_pairs(h, user, item, n, x, alpha, (hipStream_t)stream);
}

extern "C" int bprx_af_explain(bprx_handle *h, const int32_t *user, const int32_t *item, int64_t n, int32_t grid, float *x, float *alpha,
                               float *parts, float *map, int32_t *peak_cell, float *peak_val, void *stream) {
  AF_CHECK("af_explain")
  if (n < 0 || n > h->cfg.max_batch) BPRX_FAIL(h, BPRX_E_INVALID, "af_explain: n = %lld outside [0, max_batch]", (long long)n);
  if (grid < 1 || grid > AF_WROW || AF_WROW % grid != 0)
    BPRX_FAIL(h, BPRX_E_INVALID, "af_explain: grid = %d is not a divisor of %d", grid, AF_WROW);
  if (n == 0) return BPRX_OK;
  if (!user || !item || !x || !alpha || !parts || !peak_cell || !peak_val) BPRX_FAIL(h, BPRX_E_INVALID, "af_explain: null pointer");
  AfState *S = h->af;
  // E: the cell sums of at most ecap distinct items at a time, at most 1 GiB
  const size_t per = (size_t)grid * grid * AF_CH * sizeof(float);
  int64_t ecap = (int64_t)(((size_t)1 << 30) / per);
  if (ecap > n) ecap = n;
  if (!S->erank && S->mem.regrow(&S->erank, (size_t)S->R) != hipSuccess)
    BPRX_FAIL(h, BPRX_E_NOMEM, "af_explain: workspace allocation failed");
  if ((size_t)ecap * per > S->E_bytes) {
    BPRX_HIP(h, hipDeviceSynchronize());                      // earlier calls may still read the old one
    S->E_bytes = 0;
    if (S->mem.regrow(&S->E, (size_t)ecap * per / sizeof(float)) != hipSuccess)
      BPRX_FAIL(h, BPRX_E_NOMEM, "af_explain: workspace allocation failed (%zu MB)", ((size_t)ecap * per) >> 20);
    S->E_bytes = (size_t)ecap * per;
  }
  hipStream_t s = (hipStream_t)stream;
  const int rc = af_explain_body(h, user, item, n, grid, x, alpha, parts, map, peak_cell, peak_val, ecap, s);
  // the claims are released on every path (the claim kernel ran, or was at least tried: rowitem names the rows)
  hipLaunchKernelGGL(k_af_release, dim3(bprx_blocks(n, 256)), dim3(256), 0, s, S->rowitem, n, S->rowuser, (int64_t)0, S->islot, S->uslot);
  if (!rc) BPRX_LAUNCH_CHECK(h, "k_af_release");
  return rc;
}

extern "C" int bprx_af_score_block(bprx_handle *h, int32_t u0, int32_t u1, float *scores, float *alpha, void *stream) {
  AF_CHECK("af_score_block")
  if (u0 < 0 || u1 > h->cfg.num_users || u0 > u1 || !scores) BPRX_FAIL(h, BPRX_E_INVALID, "af_score_block: bad user range [%d,%d)", u0, u1);
  if (u0 == u1) return BPRX_OK;
  return bprx_af_block(h, u0, u1, scores, alpha, (hipStream_t)stream);
}

// bprx_af_score_block for caller-owned rows (users folded in by bprx_af_fold_in): k_af_block, given the caller's rows
extern "C" int bprx_af_score_rows_block(bprx_handle *h, const float *Gu_rows, int64_t n_rows, int64_t r0, int64_t r1, float *scores,
                                        float *alpha, void *stream) {
  if (!h) return BPRX_E_INVALID;
  if (n_rows < 0 || n_rows >= ((int64_t)1 << 31) || r0 < 0 || r1 > n_rows || r0 > r1)
    BPRX_FAIL(h, BPRX_E_INVALID, "af_score_rows_block: bad row range [%lld,%lld) of %lld", (long long)r0, (long long)r1, (long long)n_rows);
  if (r0 != r1 && (!Gu_rows || !scores)) BPRX_FAIL(h, BPRX_E_INVALID, "af_score_rows_block: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const int rc = bprx_enter(h, "af_score_rows_block", NEED_BOUND, KIND_AF, s);
  if (rc || r0 == r1) return rc;
  return bprx_af_block(h, (int32_t)r0, (int32_t)r1, scores, alpha, s, Gu_rows);
}

// Total LDS of a k_af_fold workgroup where the waves' own areas leave room: four workgroups share a CU (160 KB), the occupancy
// bprx_fold_in chose; what the areas do not take holds the cached pairs.  Wider models take what they need, up to 64 KB.
constexpr size_t AF_FOLD_LDS = 40 * 1024;

extern "C" int bprx_af_fold_in(bprx_handle *h, const int64_t *pair_ptr, const int32_t *pos, const int32_t *neg, int64_t n, int32_t steps,
                               float lr, float reg, int32_t optimizer, float *Gu_rows, float *loss, void *stream) {
  if (!h) return BPRX_E_INVALID;
  int rc = fold_check_args(h, "af_fold_in", n, steps, optimizer);
  if (rc) return rc;
  if (!pair_ptr || !Gu_rows) BPRX_FAIL(h, BPRX_E_INVALID, "af_fold_in: null pointer");
  if (n && (!pos || !neg)) BPRX_FAIL(h, BPRX_E_INVALID, "af_fold_in: null pointer");
  hipStream_t s = (hipStream_t)stream;
  rc = bprx_enter(h, "af_fold_in", NEED_BOUND, KIND_AF, s);
  if (rc || n == 0) return rc;
  if ((rc = af_call_current(h, s))) return rc;               // the encodings the scores are computed from
  AfState *S = h->af;
  const bprx_config &c = h->cfg;
  AfFold F;
  F.A = af_att(h, S->Call, c.num_items);
  F.I = c.num_items;
  F.ptr = pair_ptr; F.pos = pos; F.neg = neg;
  F.steps = steps; F.adam = optimizer == BPRX_OPT_ADAM_TF23;
  F.lr = lr; F.reg = reg; F.b1 = c.beta1; F.b2 = c.beta2; F.eps = c.epsilon;
  F.Gu = Gu_rows; F.loss = loss; F.errflag = h->errflag;
  // as many waves (pairs in flight) as fit a workgroup's 64 KB with their areas: four up to k = 384 at h = 32, one always fits
  const size_t per = 9 * (size_t)S->k + 6 * (size_t)S->h;
  int NW = 4;
  auto fixed = [&](int nw) { return sizeof(float) * ((size_t)S->k + nw + nw * per); };
  while (NW > 1 && fixed(NW) > 65536) --NW;
  const size_t total = fixed(NW) > AF_FOLD_LDS ? fixed(NW) : AF_FOLD_LDS;
  F.cache = h->fold_cache ? (int)((total - fixed(NW)) / sizeof(float)) : 0;
  const size_t lds = fixed(NW) + (size_t)F.cache * sizeof(float);
  hipLaunchKernelGGL(k_af_fold, dim3((unsigned)n), dim3(64 * NW), lds, s, F);
  BPRX_LAUNCH_CHECK(h, "k_af_fold");
  return BPRX_OK;
}

// ---- new items: encodings of caller-owned inputs, the warm fit, and the blocks for caller-owned item rows (include/bprx.h) ----
extern "C" int bprx_af_encode_new(bprx_handle *h, const uint8_t *edges, const float *color, const float *cls, int64_t n, float *out,
                                  void *stream) {
  if (!h) return BPRX_E_INVALID;
  if (n < 0 || n >= ((int64_t)1 << 31)) BPRX_FAIL(h, BPRX_E_INVALID, "af_encode_new: n = %lld out of range", (long long)n);
  if (n && (!edges || !color || !cls || !out)) BPRX_FAIL(h, BPRX_E_INVALID, "af_encode_new: null pointer");
  if ((uintptr_t)edges & 15) BPRX_FAIL(h, BPRX_E_INVALID, "af_encode_new: edges must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int rc0 = bprx_enter(h, "af_encode_new", NEED_BOUND, KIND_AF, s);
  if (rc0 || n == 0) return rc0;
  AfState *S = h->af;
  const AfDrop d = af_drop(S, 0, false);
  const size_t kb = (size_t)S->k * sizeof(float);
  for (int64_t r0 = 0; r0 < n; r0 += S->R) {                 // the chunks of bprx_af_encode: row r of a chunk reads row r of its inputs
    const int64_t m = n - r0 < S->R ? n - r0 : S->R;
    hipLaunchKernelGGL(k_af_iota, dim3(bprx_blocks(m, 256)), dim3(256), 0, s, S->rowitem, m, (int32_t)0);
    BPRX_LAUNCH_CHECK(h, "k_af_iota");
    const AfInputs in = {edges + r0 * (int64_t)(AF_IMG * AF_IMG), color + r0 * S->Dc, cls + r0 * S->Dk};
    int rc;
    if ((rc = af_encode_rows(h, in, m, false, d, S->C, S->R, s))) return rc;
    for (int l = 0; l < 3; ++l)
      BPRX_HIP(h, hipMemcpyAsync(out + ((int64_t)l * n + r0) * S->k, S->C + (int64_t)l * S->R * S->k, m * kb, hipMemcpyDeviceToDevice, s));
  }
  return BPRX_OK;
}

// float4 rows in k_af_block where k is a multiple of 8: the caller's item rows must then start on 16 bytes, as the bound tables do
static bool af_rows_aligned(const AfState *S, const float *C_rows, const float *Gi_rows) {
  return (S->k % 8) != 0 || ((((uintptr_t)C_rows | (uintptr_t)Gi_rows) & 15) == 0);
}

constexpr unsigned AF_ITEM_PAIR_GRID = 2048;                  // workgroups of k_af_item_pairs: four waves each, walking the pairs

extern "C" int bprx_af_fold_in_items(bprx_handle *h, const int64_t *pair_ptr, const int32_t *user, const int32_t *other, const int32_t *role,
                                     int64_t n, const float *C_rows, int32_t steps, float lr, float reg, int32_t optimizer, float *Gi_rows,
                                     float *loss, float *work, void *stream) {
  if (!h) return BPRX_E_INVALID;
  int rc = fold_check_args(h, "af_fold_in_items", n, steps, optimizer);
  if (rc) return rc;
  if (!pair_ptr) BPRX_FAIL(h, BPRX_E_INVALID, "af_fold_in_items: null pointer");
  if (n && (!user || !other || !role || !Gi_rows || !C_rows || !work)) BPRX_FAIL(h, BPRX_E_INVALID, "af_fold_in_items: null pointer");
  hipStream_t s = (hipStream_t)stream;
  rc = bprx_enter(h, "af_fold_in_items", NEED_BOUND, KIND_AF, s);
  if (rc || n == 0) return rc;
  if ((rc = af_call_current(h, s))) return rc;               // the encodings the scores are computed from
  AfState *S = h->af;
  const bprx_config &c = h->cfg;
  AfItemPairs X;
  X.A = af_att(h, S->Call, c.num_items);
  X.Cn = C_rows; X.U = c.num_users; X.I = c.num_items; X.n = n;
  X.ptr = pair_ptr; X.user = user; X.other = other; X.role = role;
  X.work = work; X.KW = (S->k + 1 + 3) / 4 * 4; X.errflag = h->errflag;
  // 8k floats per wave: 60 KB at k = 480, the widest shape bprx_bind_attentive accepts (k <= 512 fits 64 KB)
  hipLaunchKernelGGL(k_af_item_pairs, dim3(AF_ITEM_PAIR_GRID), dim3(256), 32 * sizeof(float) * (size_t)S->k, s, X);
  BPRX_LAUNCH_CHECK(h, "k_af_item_pairs");
  return bprx_launch_af_fold_items(h, pair_ptr, n, work, X.KW, S->k, steps, optimizer == BPRX_OPT_ADAM_TF23, lr, reg, Gi_rows, loss, s);
}

extern "C" int bprx_af_score_warm_block(bprx_handle *h, int32_t u0, int32_t u1, const float *C_rows, const float *Gi_rows, int64_t n,
                                        float *scores, float *alpha, void *stream) {
  if (!h) return BPRX_E_INVALID;
  if (u0 < 0 || u1 > h->cfg.num_users || u0 > u1) BPRX_FAIL(h, BPRX_E_INVALID, "af_score_warm_block: bad user range [%d,%d)", u0, u1);
  if (n < 0 || n >= ((int64_t)1 << 31)) BPRX_FAIL(h, BPRX_E_INVALID, "af_score_warm_block: n = %lld out of range", (long long)n);
  const bool work = n != 0 && u0 != u1;
  if (work && (!C_rows || !Gi_rows || !scores)) BPRX_FAIL(h, BPRX_E_INVALID, "af_score_warm_block: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const int rc = bprx_enter(h, "af_score_warm_block", NEED_BOUND, KIND_AF, s);
  if (rc || !work) return rc;
  if (!af_rows_aligned(h->af, C_rows, Gi_rows)) BPRX_FAIL(h, BPRX_E_INVALID, "af_score_warm_block: C_rows and Gi_rows must be 16-byte aligned");
  AfAtt A = af_att(h, C_rows, n);
  A.Gi = Gi_rows;
  return af_block_run(h, A, C_rows, (int)n, u0, u1, scores, alpha, s);
}

extern "C" int bprx_af_audience_block(bprx_handle *h, const float *C_rows, const float *Gi_rows, int64_t n, int64_t q0, int64_t q1,
                                      float *scores, float *alpha, void *stream) {
  if (!h) return BPRX_E_INVALID;
  if ((C_rows == nullptr) != (Gi_rows == nullptr)) BPRX_FAIL(h, BPRX_E_INVALID, "af_audience_block: C_rows and Gi_rows are both NULL (the catalogue) or both given");
  if (n < 0 || n >= ((int64_t)1 << 31) || (!C_rows && n != h->cfg.num_items))
    BPRX_FAIL(h, BPRX_E_INVALID, "af_audience_block: n = %lld (the catalogue form takes n = num_items)", (long long)n);
  if (q0 < 0 || q1 > n || q0 > q1) BPRX_FAIL(h, BPRX_E_INVALID, "af_audience_block: bad item range [%lld,%lld) of %lld", (long long)q0, (long long)q1, (long long)n);
  if (q0 != q1 && !scores) BPRX_FAIL(h, BPRX_E_INVALID, "af_audience_block: null pointer");
  hipStream_t s = (hipStream_t)stream;
  int rc = bprx_enter(h, "af_audience_block", NEED_BOUND, KIND_AF, s);
  if (rc || q0 == q1) return rc;
  AfState *S = h->af;
  const int U = h->cfg.num_users;
  if (!C_rows) {
    if ((rc = af_call_current(h, s))) return rc;
    return af_block_run(h, af_att(h, S->Call, n), S->Call, (int)n, 0, U, scores, alpha, s, true, (int)q0, (int)q1, U);
  }
  if (!af_rows_aligned(S, C_rows, Gi_rows)) BPRX_FAIL(h, BPRX_E_INVALID, "af_audience_block: C_rows and Gi_rows must be 16-byte aligned");
  AfAtt A = af_att(h, C_rows, n);
  A.Gi = Gi_rows;
  return af_block_run(h, A, C_rows, (int)n, 0, U, scores, alpha, s, true, (int)q0, (int)q1, U);
}

extern "C" int bprx_af_dropout_mask(bprx_handle *h, int64_t step, int64_t n_rows, uint8_t *out, void *stream) {
  AF_CHECK("af_dropout_mask")
  if (n_rows < 0 || n_rows > h->af->R || step < 0) BPRX_FAIL(h, BPRX_E_INVALID, "af_dropout_mask: bad step / n_rows");
  if (n_rows == 0) return BPRX_OK;
  if (!out) BPRX_FAIL(h, BPRX_E_INVALID, "af_dropout_mask: null pointer");
  const AfDrop d = af_drop(h->af, step, true);
  hipLaunchKernelGGL(k_af_mask, dim3(bprx_blocks(n_rows * 144, 256)), dim3(256), 0, (hipStream_t)stream, d, n_rows, out);
  BPRX_LAUNCH_CHECK(h, "k_af_mask");
  return BPRX_OK;
}

extern "C" int64_t bprx_af_get_step(const bprx_handle *h) { return h && h->af ? h->af->step : -1; }

extern "C" int bprx_af_set_step(bprx_handle *h, int64_t step) {
  AF_CHECK("af_set_step")
  if (step < 0) BPRX_FAIL(h, BPRX_E_INVALID, "af_set_step: step < 0");
  h->af->step = step;
  return BPRX_OK;
}
