// bprx_because.hip -- "recommended because it is like the X you own": for every entry of a list the L nearest items of that
// list's history by cosine in the model's item space (include/bprx.h, bprx_because).
#include "bprx_internal.h"

namespace {

constexpr int BC_T = 256;                    // threads of a workgroup
constexpr int BC_W = BC_T / 64;              // its waves: wave v owns the slots v, v + 4, v + 8, .. of the chunk
constexpr int BC_SB = 4;                     // slots a wave runs side by side: four independent fma chains per lane
constexpr int BC_HT = 64;                    // history entries of a tile: one per lane
constexpr int BC_LMAX = 32, BC_KMAX = 1024;
constexpr int BC_DYN_MAX = 63 * 1024;        // dynamic LDS of a workgroup at most: as for k_diversify, what a launch gets without
                                             //    opting in; a launch asks for what its chunk needs, so short lists share a CU

struct BecArgs {
  SimPart qg, qp;                            // z = [g | p] of the explained items (the catalogue, or the caller's projected rows)
  SimPart hg, hp;                            // ... of the catalogue: the history's rows
  const float *rn_q, *rn;                    // norms of the explained items' table and of the catalogue
  int nq, I, K, L;
  int KC, HT, ld;                            // slots of a chunk, entries of a history tile, row stride of the LDS rows (odd)
  int self;                                  // the explained items are catalogue items: an entry with the item's own id is no candidate
  const int32_t *list_idx;
  const int64_t *hist_ptr;
  const int32_t *hist_items;
  int32_t *out_item;
  float *out_cos;
  int32_t *out_cnt;
  int32_t *errflag;
};

// (cosine descending, history position ascending) as one integer; never 0 for a position < 2^32 - 1
__device__ __forceinline__ unsigned long long bc_key(float c, uint32_t pos) {
  return ((unsigned long long)dv_key(c) << 32) | (uint32_t)(0xffffffffu - pos);
}

// One workgroup per (list, chunk of KC list slots).  The chunk's item rows are copied to LDS once, the history's rows a tile of HT
// at a time (consecutive threads copy consecutive x: coalesced reads, stride-1 LDS writes; row stride ld odd).  Lane l of a wave
// holds history entry l of the tile; the wave walks its slots four at a time: per x one read of the entry's row (32 lanes, 32
// banks) and four of the slots' rows (one address for all lanes: broadcasts), four chains a = fmaf(z_q[x], z_l[x], a) from +0 in
// ascending x.  The cosine stays in the lane that computed it: the slot's running top-L (cosine, position; LDS, two copies that
// alternate from tile to tile) and the tile's 64 cosines are 128 keys at most, two per lane, and L wave-wide maxima of them --
// the position is part of the key -- are the new top-L.  A key's rank among all keys of the history does not depend on the tile
// it arrived in, so neither does the result.  A slot is read and written by one wave only.
__global__ __launch_bounds__(BC_T) void k_because(BecArgs a) {
  extern __shared__ float bc_dyn[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int KC = a.KC, HT = a.HT, L = a.L, ld = a.ld, w = a.hg.w + a.hp.w;
  int *s_qraw = (int *)bc_dyn, *s_qid = s_qraw + KC;             // the chunk's slots: list entry, its row (-1: empty), norm,
  float *s_qrn = (float *)(s_qid + KC);                          //    candidates seen so far
  int *s_m = (int *)(s_qrn + KC);
  int *s_hraw = s_m + KC, *s_hid = s_hraw + HT;                  // the tile's entries: id as given, row, norm
  float *s_hrn = (float *)(s_hid + HT);
  float *s_tc = s_hrn + HT;                                      // running top-L: cosine [2][KC][L], position [2][KC][L]
  uint32_t *s_tp = (uint32_t *)(s_tc + 2 * KC * L);
  float *s_q = (float *)(s_tp + 2 * KC * L), *s_h = s_q + (size_t)KC * ld;   // rows [KC][ld], [HT][ld]
  const size_t r = blockIdx.x;
  const int q0 = blockIdx.y * KC, kc = min(KC, a.K - q0);
  const int64_t hp0 = a.hist_ptr[r];
  const int64_t hl = max((int64_t)0, a.hist_ptr[r + 1] - hp0);

  for (int c = tid; c < kc; c += BC_T) {
    const int raw = a.list_idx[r * (size_t)a.K + q0 + c];
    const int id = raw < 0 ? -1 : clamp_index(raw, a.nq, a.errflag, 2);
    s_qraw[c] = raw; s_qid[c] = id; s_qrn[c] = id < 0 ? 0.f : a.rn_q[id]; s_m[c] = 0;
  }
  __syncthreads();
#pragma unroll 4
  for (int e = tid; e < kc * w; e += BC_T) {
    const int c = e / w, x = e - c * w, id = s_qid[c];
    float v = 0.f;                                               // (an empty slot reads no row)
    if (id >= 0) v = x < a.qg.w ? a.qg.p[(size_t)id * a.qg.ld + x] : a.qp.p[(size_t)id * a.qp.ld + (x - a.qg.w)];
    s_q[c * ld + x] = v;
  }

  int par = 0;                                                   // the copy of the top-L that is current
  for (int64_t t0 = 0; t0 < hl; t0 += HT) {
    const int hc = (int)min((int64_t)HT, hl - t0);
    __syncthreads();                                             // the last tile's rows are no longer read (first tile: s_q is complete)
    if (tid < hc) {
      const int raw = a.hist_items[hp0 + t0 + tid];
      const int id = clamp_index(raw, a.I, a.errflag, 2);
      s_hraw[tid] = raw; s_hid[tid] = id; s_hrn[tid] = a.rn[id];
    }
    __syncthreads();
#pragma unroll 4
    for (int e = tid; e < hc * w; e += BC_T) {
      const int c = e / w, x = e - c * w;
      const size_t row = (size_t)s_hid[c];
      s_h[c * ld + x] = x < a.hg.w ? a.hg.p[row * a.hg.ld + x] : a.hp.p[row * a.hp.ld + (x - a.hg.w)];
    }
    __syncthreads();
    // a lane past the tile's end runs the tile's last entry (no per-lane branch in the chain); what it computes is never used
    const bool have = lane < hc;
    const int he = min(lane, hc - 1);
    const float *zh = s_h + he * ld;
    const int hraw = s_hraw[he];
    const float hrn = s_hrn[he];
    const uint32_t hpos = (uint32_t)(t0 + lane);
    for (int sb = wave; sb < kc; sb += BC_W * BC_SB) {
      int off[BC_SB];
      float dot[BC_SB];
#pragma unroll
      for (int j = 0; j < BC_SB; ++j) { off[j] = min(sb + j * BC_W, kc - 1) * ld; dot[j] = 0.f; }
#pragma unroll 4                                 // (each chain keeps its order.  Measured on C2 against unroll 8: 79 instead of 99
                                                 //  VGPRs, a fifth workgroup per CU, 2.34 instead of 2.69 ms at w = 64)
      for (int x = 0; x < w; ++x) {
        const float hv = zh[x];
#pragma unroll
        for (int j = 0; j < BC_SB; ++j) dot[j] = fmaf(s_q[off[j] + x], hv, dot[j]);
      }
#pragma unroll
      for (int j = 0; j < BC_SB; ++j) {
        const int slot = sb + j * BC_W;          // (uniform in the wave, like everything that decides a branch below)
        if (slot >= kc) break;
        const int qraw = s_qraw[slot];
        if (qraw < 0) continue;
        const float cs = __fmul_rn(dot[j], __fmul_rn(s_qrn[slot], hrn));   // norms first: the bits of bprx_diversify's cosine
        const bool cand = have && !(a.self && hraw == qraw);
        const int mo = s_m[slot], To = min(L, mo);
        const float *oc = s_tc + (par * KC + slot) * L;
        const uint32_t *op = s_tp + (par * KC + slot) * L;
        float *nc = s_tc + ((par ^ 1) * KC + slot) * L;
        uint32_t *np = s_tp + ((par ^ 1) * KC + slot) * L;
        unsigned long long k0 = 0ull, k1 = 0ull;
        float c0 = 0.f;
        uint32_t p0 = 0u;
        if (lane < To) { c0 = oc[lane]; p0 = op[lane]; k0 = bc_key(c0, p0); }
        if (cand) k1 = bc_key(cs, hpos);
        const int add = __popcll(__ballot(cand));
        for (int s = 0; s < L; ++s) {
          const unsigned long long best = dv_wave_max(k0 > k1 ? k0 : k1);
          if (best == 0ull) break;
          if (k0 == best) { nc[s] = c0; np[s] = p0; k0 = 0ull; }
          else if (k1 == best) { nc[s] = cs; np[s] = hpos; k1 = 0ull; }
        }
        if (lane == 0) s_m[slot] = mo + add;
      }
    }
    par ^= 1;
  }
  __syncthreads();
  for (int slot = wave; slot < kc; slot += BC_W) {
    const bool empty = s_qraw[slot] < 0;
    const int M = empty ? 0 : s_m[slot], T = min(L, M);
    const size_t o = r * (size_t)a.K + q0 + slot;
    if (lane < L) {
      const bool got = lane < T;
      const uint32_t pos = got ? s_tp[(par * KC + slot) * L + lane] : 0u;
      a.out_item[o * L + lane] = got ? a.hist_items[hp0 + pos] : -1;
      a.out_cos[o * L + lane] = got ? s_tc[(par * KC + slot) * L + lane] : 0.f;
    }
    if (lane == 0 && a.out_cnt) a.out_cnt[o] = M;
  }
}

// bytes of dynamic LDS for a chunk of KC slots and tiles of HT entries
size_t bc_lds(int KC, int HT, int L, int ld) {
  return sizeof(float) * ((size_t)KC * (4 + 4 * L + ld) + (size_t)HT * (3 + ld));
}

}  // namespace

extern "C" int bprx_because(bprx_handle *h, int32_t space, const float *Pq, int64_t nq, const float *rn_q, const float *rn_items,
                            int64_t n, int32_t K, const int32_t *list_idx, const int64_t *hist_ptr, const int32_t *hist_items,
                            int32_t L, int32_t *out_item, float *out_cos, int32_t *out_cnt, void *stream) {
  if (!h) return BPRX_E_INVALID;
  if (n < 0 || n >= ((int64_t)1 << 31)) BPRX_FAIL(h, BPRX_E_INVALID, "because: n = %lld out of range", (long long)n);
  if (K < 1 || K > BC_KMAX) BPRX_FAIL(h, BPRX_E_INVALID, "because: K = %d outside [1, %d]", K, BC_KMAX);
  if (L < 1 || L > BC_LMAX) BPRX_FAIL(h, BPRX_E_INVALID, "because: L = %d outside [1, %d]", L, BC_LMAX);
  if (!rn_items || (Pq && !rn_q) || (n > 0 && (!list_idx || !hist_ptr || !hist_items || !out_item || !out_cos)))
    BPRX_FAIL(h, BPRX_E_INVALID, "because: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const int rc = bprx_sim_enter(h, "because", space, Pq, nq, s);
  if (rc || n == 0) return rc;
  BecArgs a = {};
  bprx_sim_parts(h, space, Pq, a.qg, a.qp);
  bprx_sim_parts(h, space, nullptr, a.hg, a.hp);
  a.hg.w = a.qg.w;                                               // (the caller's rows have no Gi part)
  a.rn_q = rn_q ? rn_q : rn_items; a.rn = rn_items;
  a.nq = (int)nq; a.I = h->cfg.num_items; a.K = K; a.L = L; a.self = Pq ? 0 : 1;
  a.list_idx = list_idx; a.hist_ptr = hist_ptr; a.hist_items = hist_items;
  a.out_item = out_item; a.out_cos = out_cos; a.out_cnt = out_cnt; a.errflag = h->errflag;
  const int w = a.hg.w + a.hp.w;
  a.ld = w | 1;
  // tiles of 64 entries unless the space is so wide that they would take more than half the LDS; the slots get the rest
  a.HT = BC_HT;
  while (a.HT > 1 && bc_lds(0, a.HT, L, a.ld) > (size_t)BC_DYN_MAX / 2) a.HT >>= 1;
  const size_t fixed = bc_lds(0, a.HT, L, a.ld), per_slot = bc_lds(1, 0, L, a.ld);
  if (fixed + per_slot > (size_t)BC_DYN_MAX)
    BPRX_FAIL(h, BPRX_E_INVALID, "because: an item space of %d numbers does not fit a workgroup's LDS", w);
  const size_t fit = ((size_t)BC_DYN_MAX - fixed) / per_slot;
  a.KC = (int)(fit < (size_t)K ? fit : (size_t)K);
  const unsigned chunks = (unsigned)((K + a.KC - 1) / a.KC);
  hipLaunchKernelGGL(k_because, dim3((unsigned)n, chunks), dim3(BC_T), bc_lds(a.KC, a.HT, L, a.ld), s, a);
  BPRX_LAUNCH_CHECK(h, "k_because");
  return BPRX_OK;
}
