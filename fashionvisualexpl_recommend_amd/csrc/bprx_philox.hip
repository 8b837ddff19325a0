// bprx_philox.hip -- device-side throughput sampler (replaces the role of
// DataLoader.all_triple_batches, dataset.py:83-114, when bit-compatibility with the reference's MT19937 stream
// is not required).  Counter-based Philox4x32-10: triplet n of stream `seed` is a pure function of (seed, n):
//   block(n, a) = philox(key = seed, ctr = (n_lo, n_hi, a, 0))
//   positive p  = mulhi64(block(n,0).xy, N)  -> (pos_user[p], items_sorted[p])   uniform over training interactions
//   negative j  = mulhi32(block(n,a).z, I), a = 0,1,.. until j is not a positive of the user (binary search in the
//                 user's ascending item list; at most 1024 attempts)              uniform over non-positives
//                 after 1024 positives in a row (a user holding nearly every item): the r-th non-positive of the user,
//                 r = mulhi32(block(n,1024).z, M) over its M = I - #distinct(list) non-positives (an O(len) walk)
// so any rank can regenerate any other rank's triplets, and the CPU twin (oracle/bpr_oracle.c orc_sample_philox)
// is bit-exact.  One thread per triplet; 12 B written per triplet.
#include <hip/hip_runtime.h>

#include "bprx_internal.h"

namespace {

// philox4x32_10: bprx_internal.h

// The negative after 1024 rejections: the r-th (0-based) item that is not in the user's ascending list (which may repeat an
// item), r = mulhi32(z, M) over the M = I - #distinct non-positives -- uniform over the non-positives like the rejection draw,
// and never a positive.  Only users whose positives cover nearly every item get here.  M == 0 (every item a positive: the
// samplers' constructors refuse such a user) keeps `last`.  CPU twin: nth_non_positive in oracle/bpr_oracle.c.
__device__ __forceinline__ int32_t nth_non_positive(const int32_t *__restrict__ lst, long long len, uint32_t I, uint32_t z,
                                                    int32_t last) {
  long long distinct = 0;
  for (long long q = 0; q < len; ++q) distinct += (q == 0 || lst[q] != lst[q - 1]);
  if (distinct >= (long long)I) return last;
  uint32_t x = __umulhi(z, I - (uint32_t)distinct);
  for (long long q = 0; q < len; ++q) {
    if (q && lst[q] == lst[q - 1]) continue;
    if ((uint32_t)lst[q] <= x) ++x; else break;
  }
  return x < I ? (int32_t)x : last;                       // (ids outside [0, I) in the list)
}

// The negative of stream position n, shared by the uniform and the hard kernels: the rejection draw over attempts a = 0, 1, ..
// with the third counter word base + a, the nth_non_positive fallback at base + 1024.  base = 0 is the uniform samplers' stream;
// candidate c of a hard sampler draws with base = c * 2048 (no word of one candidate is a word of another, nor the permutation's
// 0xFFFFFFFE).  HAVE0: r already holds the block of attempt 0 (k_sample_philox draws the positive from the same block).
template <bool HAVE0>
__device__ __forceinline__ int32_t draw_negative(const int32_t *__restrict__ lst, long long len, uint32_t I, unsigned long long n,
                                                 uint32_t base, uint32_t w3, uint32_t k0, uint32_t k1, uint32_t (&r)[4]) {
  int32_t jj = 0;
  bool hit = true;
  for (uint32_t a = 0; a < 1024u && hit; ++a) {
    if (!HAVE0 || a) philox4x32_10((uint32_t)n, (uint32_t)(n >> 32), base + a, w3, k0, k1, r);
    jj = (int32_t)__umulhi(r[2], I);
    long long lo = 0, hi = len;
    while (lo < hi) {
      const long long mid = (lo + hi) >> 1;
      if (lst[mid] < jj) lo = mid + 1; else hi = mid;
    }
    hit = lo < len && lst[lo] == jj;
  }
  if (hit) {
    philox4x32_10((uint32_t)n, (uint32_t)(n >> 32), base + 1024u, w3, k0, k1, r);
    jj = nth_non_positive(lst, len, I, r[2], jj);
  }
  return jj;
}

// the owner plane (id >> sh: one byte) and the local plane (id & (2^sh - 1): a byte at sh == 8, else 16 bits) of a triplet's items
__device__ __forceinline__ void put_planes(uint8_t *__restrict__ own8, uint8_t *__restrict__ loc8, long long pi, long long pj,
                                           int32_t ii, int32_t jj, int sh) {
  own8[pi] = (uint8_t)(ii >> sh); own8[pj] = (uint8_t)(jj >> sh);
  if (sh == 8) { loc8[pi] = (uint8_t)ii; loc8[pj] = (uint8_t)jj; }
  else {
    uint16_t *l16 = reinterpret_cast<uint16_t *>(loc8);
    const int m = (1 << sh) - 1;
    l16[pi] = (uint16_t)(ii & m); l16[pj] = (uint16_t)(jj & m);
  }
}

// The owner queues (bprx_internal.h): a counting sort of the workgroup's up to 512 occurrences by owner (id >> 8).  EVERY thread
// of the workgroup comes here (barriers); `live`: it holds a triplet.  hist is all-zero on entry (cleared at the kernel's start,
// behind a barrier).  The returning LDS add is the rank inside the bin; the exclusive scan over the 256 bins gives the bins'
// first slots; thread t stores bin t's [lo, hi) where owner t finds it.  No global atomic, no capacity: the region holds what
// the workgroup drew, whatever the item distribution.
struct QueueArgs {
  uint32_t *rec, *range;          // nullptr: no queues
  int q0, stride;                 // region of workgroup 0 of this launch, regions per owner in `range`
};
// WIDE (k_sample_hard): the workgroup has more than IXQ_BINS threads; hist has one entry per thread (those beyond the bins stay
// zero), wtot one per wave, and only the first IXQ_BINS threads hold a triplet or store a range.
template <bool WIDE = false>
__device__ __forceinline__ void put_queues(const QueueArgs &q, int *hist, int *wtot, bool live, int32_t ii, int32_t jj,
                                           long long occ_i, long long occ_j) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int bi = (ii >> 8) & (IXQ_BINS - 1), bj = (jj >> 8) & (IXQ_BINS - 1);       // (the owner byte of the planes)
  int ri = 0, rj = 0;
  if (live) { ri = atomicAdd(&hist[bi], 1); rj = atomicAdd(&hist[bj], 1); }
  __syncthreads();
  const int c = hist[tid];                                                          // IXQ_BINS == blockDim.x: one bin per thread
  int inc = c;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(inc, o, 64);
    if (lane >= o) inc += v;
  }
  if (lane == 63) wtot[wv] = inc;
  __syncthreads();
  int lo = inc - c;
  for (int x = 0; x < wv; ++x) lo += wtot[x];
  hist[tid] = lo;                                                       // (my bin alone: nobody else reads it before the next barrier)
  const int region = q.q0 + (int)blockIdx.x;
  if (!WIDE || tid < IXQ_BINS) q.range[ixq_range_at(tid, region, q.stride)] = ixq_range((uint32_t)lo, (uint32_t)(lo + c));
  __syncthreads();
  if (live) {
    q.rec[ixq_rec_at(region, hist[bi] + ri)] = ixq_pack((uint32_t)occ_i, (uint32_t)ii);
    q.rec[ixq_rec_at(region, hist[bj] + rj)] = ixq_pack((uint32_t)occ_j, (uint32_t)jj);
  }
}

__global__ __launch_bounds__(256) void k_sample_philox(const int64_t *__restrict__ indptr, const int32_t *__restrict__ items,
                                                       const int32_t *__restrict__ pos_user, unsigned long long N, uint32_t I,
                                                       uint32_t k0, uint32_t k1, unsigned long long first, long long B,
                                                       int32_t *__restrict__ u, int32_t *__restrict__ i, int32_t *__restrict__ j,
                                                       uint8_t *__restrict__ own8, uint8_t *__restrict__ loc8, long long pl_i,
                                                       long long pl_j, int sh, QueueArgs qa) {
  __shared__ int q_hist[IXQ_BINS], q_wtot[4];
  const long long b = (long long)blockIdx.x * 256 + threadIdx.x;
  const bool live = b < B;
  if (!qa.rec && !live) return;
  if (qa.rec) { q_hist[threadIdx.x] = 0; __syncthreads(); }   // (threads without a triplet stay for put_queues' barriers)
  int32_t ii = 0, jj = 0;
  if (live) {
    const unsigned long long n = first + (unsigned long long)b;
    uint32_t r[4];
    philox4x32_10((uint32_t)n, (uint32_t)(n >> 32), 0u, 0u, k0, k1, r);
    const unsigned long long x = ((unsigned long long)r[1] << 32) | r[0];
    const unsigned long long p = __umul64hi(x, N);
    const int32_t uu = pos_user[p];
    const long long lo0 = indptr[uu], len = indptr[uu + 1] - lo0;
    const int32_t *lst = items + lo0;
    jj = draw_negative<true>(lst, len, I, n, 0u, 0u, k0, k1, r);
    ii = items[p];
    u[b] = uu; i[b] = ii; j[b] = jj;
    if (own8) put_planes(own8, loc8, pl_i + b, pl_j + b, ii, jj, sh);   // byte planes of the item ids for the handle's index pass
  }
  if (qa.rec) put_queues(qa, q_hist, q_wtot, live, ii, jj, pl_i + b, pl_j + b);   // ... and its owners' queues
}

// Epoch-walk mode (the reference's order, dataset.py:93-107, as a stateless stream): within epoch e the users come in the
// order perm[0..U) and every positive of a user is emitted once, consecutively; stream position n (0 <= n < N) of the
// epoch maps to the user a with epoch_ptr[a] <= n < epoch_ptr[a+1] (binary search) and to that user's positive number
// n - epoch_ptr[a].  The negative is the Philox rejection draw keyed by (seed; n, epoch).  Batches are user-grouped like
// the reference's, every interaction is visited exactly once per epoch.
__global__ __launch_bounds__(256) void k_sample_epoch(const int64_t *__restrict__ indptr, const int32_t *__restrict__ items,
                                                      const int32_t *__restrict__ perm, const int64_t *__restrict__ epoch_ptr,
                                                      const int32_t *__restrict__ pos_slot, int U, uint32_t I, uint32_t k0, uint32_t k1, uint32_t epoch,
                                                      long long first, long long B, int32_t *__restrict__ u,
                                                      int32_t *__restrict__ i, int32_t *__restrict__ j,
                                                      uint8_t *__restrict__ own8, uint8_t *__restrict__ loc8, long long pl_i,
                                                      long long pl_j, int sh, QueueArgs qa) {
  __shared__ int q_hist[IXQ_BINS], q_wtot[4];
  const long long b = (long long)blockIdx.x * 256 + threadIdx.x;
  const bool live = b < B;
  if (!qa.rec && !live) return;
  if (qa.rec) { q_hist[threadIdx.x] = 0; __syncthreads(); }   // (threads without a triplet stay for put_queues' barriers)
  int32_t ii = 0, jj = 0;
  if (live) {
    const long long n = first + b;
    int lo = 0, hi = U;                                   // largest a with epoch_ptr[a] <= n (and a non-empty list)
    if (pos_slot) lo = pos_slot[n];                       // precomputed once per epoch
    else
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (epoch_ptr[mid] <= n) lo = mid; else hi = mid;
      }
    const int32_t uu = perm[lo];
    const long long l0 = indptr[uu], len = indptr[uu + 1] - l0;
    const int32_t *lst = items + l0;
    uint32_t r[4];
    jj = draw_negative<false>(lst, len, I, (unsigned long long)n, 0u, epoch, k0, k1, r);
    ii = lst[n - epoch_ptr[lo]];
    u[b] = uu; i[b] = ii; j[b] = jj;
    if (own8) put_planes(own8, loc8, pl_i + b, pl_j + b, ii, jj, sh);
  }
  if (qa.rec) put_queues(qa, q_hist, q_wtot, live, ii, jj, pl_i + b, pl_j + b);
}

// ---- hard negatives (DESIGN §9 "Hard negatives"): the best-scored of C candidates ----
// The hard forms of the two kernels above.  The user and the positive of stream position n are the uniform stream's; candidate c
// (0 <= c < C <= 16) of the position is draw_negative with base = c * 2048 (candidate 0 is the uniform negative), and the triplet's
// negative is the candidate with the largest
//   s_c = Gu_u.Gi_j + Bi_j (+ Tu_u.Ps_j[:d] + Ps_j[d]: VBPR, Ps = the caller's snapshot of the item projections),
// ties to the smallest c, a NaN never ahead of a number.  The tables are read AS STORED (no lazy-Adam catch-up).  One workgroup =
// 256 triplets (a region of put_queues) and 1 024 threads -- sixteen waves on a CU whose batch of 65 536 gives it one workgroup: the
// draws and the row reads are chains of dependent loads, and four waves hide none of them -- in three phases:
//   1  four threads per triplet (t, t + 256, ..) look its user up and draw every fourth candidate each into LDS;
//   2  a group of 16 lanes per triplet, 4 triplets per group: a lane keeps its slice of the user's row in registers and reads the
//      same slice of up to eight candidate rows before the first use (float4 slices where k / d are multiples of 4 and the tables
//      16-byte aligned, single floats otherwise), sums in the group by shuffles, picks;
//   3  thread t < 256 writes (u, i, j) and the planes and queue records of the chosen negative, exactly as the uniform kernels do.
constexpr int HARD_MAX_C = 16;
constexpr int HARD_T = 1024;                        // threads of a workgroup

struct StreamArgs {
  const int64_t *indptr;
  const int32_t *items, *pos_user;                  // pos_user: the Philox stream
  const int32_t *perm, *pos_slot;                   // the epoch walk
  const int64_t *epoch_ptr;
  unsigned long long N, first;
  int U;                                            // users of the epoch walk
  uint32_t I, k0, k1, w3;                           // w3: 0, or the epoch
};
struct HardArgs {
  const float *Gu, *Gi, *Bi, *Tu, *Ps;              // Tu == nullptr: BPRMF
  int k, d, PS, C, U;                               // U, and StreamArgs::I: rows of the handle's tables (row reads are clamped to them)
  int vec_k, vec_d;                                 // float4 slices of the k / d part
  int32_t *cand_out;                                // [B, C] optional: what was drawn ...
  float *score_out;                                 // [B, C] optional: ... and what was compared
};

__device__ __forceinline__ float dot_slice(float a, float b) { return a * b; }
__device__ __forceinline__ float dot_slice(const float4 &a, const float4 &b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }

// acc[c] += <urow, rows[cand[c]]> over n slices of type T, slice q of every row by lane q % 16 of the group; the rows of eight
// candidates are in flight before the first multiply.  cand: the triplet's column of the LDS candidate table (stride 256).
template <typename T>
__device__ __forceinline__ void hard_dots(const T *__restrict__ urow, const T *__restrict__ rows, size_t stride, int n, const int *cand,
                                          int C, int l16, float (&acc)[HARD_MAX_C]) {
  for (int q = l16; q < n; q += 16) {
    const T g = urow[q];
#pragma unroll
    for (int h = 0; h < HARD_MAX_C; h += 8) {
      if (h < C) {
        T v[8];
#pragma unroll
        for (int x = 0; x < 8; ++x)
          if (h + x < C) v[x] = rows[(size_t)cand[(h + x) * 256] * stride + q];
#pragma unroll
        for (int x = 0; x < 8; ++x)
          if (h + x < C) acc[h + x] += dot_slice(g, v[x]);
      }
    }
  }
}

template <bool EPOCH>
__global__ __launch_bounds__(HARD_T) void k_sample_hard(StreamArgs sa, HardArgs ha, long long B, int32_t *__restrict__ u,
                                                        int32_t *__restrict__ i, int32_t *__restrict__ j, uint8_t *__restrict__ own8,
                                                        uint8_t *__restrict__ loc8, long long pl_i, long long pl_j, int sh, QueueArgs qa) {
  __shared__ int q_hist[HARD_T], q_wtot[HARD_T / 64];
  __shared__ int s_cand[HARD_MAX_C * 256], s_user[256], s_neg[256];
  const int tid = threadIdx.x, trip = tid & 255, part = tid >> 8;
  const long long b0 = (long long)blockIdx.x * 256, b = b0 + trip;
  const bool live = tid < 256 && b < B;
  q_hist[tid] = 0;
  int32_t uu = 0, ii = 0;
  if (b < B) {                                            // phase 1
    const unsigned long long n = sa.first + (unsigned long long)b;
    uint32_t r[4];
    const int32_t *lst;
    long long len;
    if (EPOCH) {
      int lo = 0, hi = sa.U;
      if (sa.pos_slot) lo = sa.pos_slot[n];
      else
        while (hi - lo > 1) {
          const int mid = (lo + hi) >> 1;
          if (sa.epoch_ptr[mid] <= (long long)n) lo = mid; else hi = mid;
        }
      uu = sa.perm[lo];
      const long long l0 = sa.indptr[uu];
      len = sa.indptr[uu + 1] - l0;
      lst = sa.items + l0;
      ii = lst[(long long)n - sa.epoch_ptr[lo]];
    } else {
      philox4x32_10((uint32_t)n, (uint32_t)(n >> 32), 0u, 0u, sa.k0, sa.k1, r);
      const unsigned long long p = __umul64hi(((unsigned long long)r[1] << 32) | r[0], sa.N);
      uu = sa.pos_user[p];
      const long long l0 = sa.indptr[uu];
      len = sa.indptr[uu + 1] - l0;
      lst = sa.items + l0;
      ii = sa.items[p];
    }
    for (int c = part; c < ha.C; c += HARD_T / 256) {
      const int32_t jc = draw_negative<false>(lst, len, sa.I, n, (uint32_t)c * 2048u, sa.w3, sa.k0, sa.k1, r);
      s_cand[c * 256 + trip] = jc;
      if (ha.cand_out) ha.cand_out[b * ha.C + c] = jc;
    }
    if (part == 0) s_user[trip] = uu;
  }
  __syncthreads();
  {                                                       // phase 2
    const int grp = tid >> 4, l16 = tid & 15;
    const int C = ha.C;
    for (int t = grp; t < 256 && b0 + t < B; t += HARD_T / 16) {
      const int *cand = s_cand + t;
      const size_t ur = (size_t)min(max(s_user[t], 0), ha.U - 1);
      float acc[HARD_MAX_C];
#pragma unroll
      for (int c = 0; c < HARD_MAX_C; ++c) acc[c] = 0.f;
      if (ha.vec_k)
        hard_dots(reinterpret_cast<const float4 *>(ha.Gu + ur * ha.k), reinterpret_cast<const float4 *>(ha.Gi), (size_t)(ha.k >> 2),
                  ha.k >> 2, cand, C, l16, acc);
      else
        hard_dots(ha.Gu + ur * ha.k, ha.Gi, (size_t)ha.k, ha.k, cand, C, l16, acc);
      if (ha.Tu) {
        if (ha.vec_d)
          hard_dots(reinterpret_cast<const float4 *>(ha.Tu + ur * ha.d), reinterpret_cast<const float4 *>(ha.Ps), (size_t)(ha.PS >> 2),
                    ha.d >> 2, cand, C, l16, acc);
        else
          hard_dots(ha.Tu + ur * ha.d, ha.Ps, (size_t)ha.PS, ha.d, cand, C, l16, acc);
      }
#pragma unroll
      for (int c = 0; c < HARD_MAX_C; ++c)
        if (c < C) {
          if (l16 == 0) {                                 // the biases ride on one lane of the group
            const size_t jc = (size_t)cand[c * 256];
            acc[c] += ha.Bi[jc];
            if (ha.Tu) acc[c] += ha.Ps[jc * ha.PS + ha.d];
          }
#pragma unroll
          for (int o = 8; o; o >>= 1) acc[c] += __shfl_xor(acc[c], o, 16);
        }
      // largest wins, ties to the smallest c; a NaN only ever stays when nothing but NaNs follow
      int best = 0;
      float sb = acc[0];
#pragma unroll
      for (int c = 1; c < HARD_MAX_C; ++c)
        if (c < C && (acc[c] > sb || (sb != sb && acc[c] == acc[c]))) { best = c; sb = acc[c]; }
      if (l16 == 0) s_neg[t] = cand[best * 256];
      if (ha.score_out) {
#pragma unroll
        for (int c = 0; c < HARD_MAX_C; ++c)
          if (c < C && l16 == (c & 15)) ha.score_out[(b0 + t) * C + c] = acc[c];
      }
    }
  }
  __syncthreads();
  int32_t jj = 0;
  if (live) {                                             // phase 3
    jj = s_neg[tid];
    u[b] = uu; i[b] = ii; j[b] = jj;
    if (own8) put_planes(own8, loc8, pl_i + b, pl_j + b, ii, jj, sh);
  }
  if (qa.rec) put_queues<true>(qa, q_hist, q_wtot, live, ii, jj, pl_i + b, pl_j + b);
}

// The user order of an epoch: a keyed permutation of [0, U) evaluated POINTWISE -- slot a of epoch `epoch` holds user
//   perm(a) = cycle-walk of a 4-round Feistel network over 2*half bits (half = ceil(bits(U-1) / 2)), round function
//             F_r(R) = philox(key = seed, ctr = (R, r, 0xFFFFFFFE, epoch))[0] & (2^half - 1); walk until the value is < U
// (a bijection of [0, 2^(2 half)) restricted to [0, U) by cycle-walking: a bijection of [0, U); < 4 walks on average).  No keys,
// no sort: until the end of round 3 the order was the stable argsort of per-user Philox keys -- a device merge sort of 8 launches
// and 60 us per epoch inside a preparation of 23 launches and 158 us (5 us per C2 step); this is one launch of a few us.  The third
// counter word never collides with the negative draws (attempt numbers <= 1024).  CPU twin: oracle orc_epoch_perm.
__device__ __forceinline__ uint32_t epoch_perm_at(uint32_t a, uint32_t U, int half, uint32_t k0, uint32_t k1, uint32_t epoch) {
  const uint32_t mask = (1u << half) - 1u;
  uint32_t x = a;
  do {
    uint32_t L = x >> half, R = x & mask;
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) {
      uint32_t o[4];
      philox4x32_10(R, r, 0xFFFFFFFEu, epoch, k0, k1, o);
      const uint32_t t = L ^ (o[0] & mask);
      L = R; R = t;
    }
    x = (L << half) | R;
  } while (x >= U);
  return x;
}

__host__ __device__ inline int epoch_perm_half(uint32_t U) {          // half the bits of the Feistel domain (>= 1)
  int nb = 1;
  while (nb < 32 && (U - 1u) >> nb) ++nb;
  return (nb + 1) / 2;
}

// slot a -> its user and the length of that user's list (the prefix sums of the lengths are the epoch's position offsets)
__global__ __launch_bounds__(256) void k_epoch_prepare(uint32_t k0, uint32_t k1, uint32_t epoch, int U, int half,
                                                       const int64_t *__restrict__ indptr, int32_t *__restrict__ perm,
                                                       int64_t *__restrict__ lens) {
  const int a = blockIdx.x * 256 + threadIdx.x;
  if (a >= U) return;
  const uint32_t u = epoch_perm_at((uint32_t)a, (uint32_t)U, half, k0, k1, epoch);
  perm[a] = (int32_t)u;
  lens[a] = indptr[u + 1] - indptr[u];
}

// position -> slot: positions [epoch_ptr[a], epoch_ptr[a+1]) belong to slot a (one lane group of 8 per slot)
__global__ __launch_bounds__(256) void k_epoch_slots(const int64_t *__restrict__ epoch_ptr, int U, int32_t *__restrict__ pos_slot,
                                                     int64_t num_pos) {
  const int a = (blockIdx.x * 256 + threadIdx.x) >> 3, lane = threadIdx.x & 7;
  if (a >= U) return;
  const int64_t p0 = epoch_ptr[a];
  int64_t p1 = epoch_ptr[a + 1];
  p1 = p1 < num_pos ? p1 : num_pos;                        // (never beyond the array, whatever the CSR claims)
  for (int64_t p = p0 + lane; p < p1; p += 8) pos_slot[p] = a;
}

}  // namespace

extern "C" int bprx_epoch_prepare(uint64_t seed, uint32_t epoch, int32_t num_users, const int64_t *indptr, int32_t *perm,
                                  int64_t *lens, void *stream) {
  if (!indptr || !perm || !lens || num_users <= 0) return BPRX_E_INVALID;
  hipLaunchKernelGGL(k_epoch_prepare, dim3((unsigned)((num_users + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (uint32_t)seed,
                     (uint32_t)(seed >> 32), epoch, num_users, epoch_perm_half((uint32_t)num_users), indptr, perm, lens);
  return hipGetLastError() == hipSuccess ? BPRX_OK : BPRX_E_HIP;
}

extern "C" int bprx_epoch_slots(const int64_t *epoch_ptr, int32_t num_users, int32_t *pos_slot, int64_t num_pos, void *stream) {
  if (!epoch_ptr || !pos_slot || num_users <= 0 || num_pos < 0) return BPRX_E_INVALID;
  hipLaunchKernelGGL(k_epoch_slots, dim3((unsigned)(((int64_t)num_users * 8 + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     epoch_ptr, num_users, pos_slot, num_pos);
  return hipGetLastError() == hipSuccess ? BPRX_OK : BPRX_E_HIP;
}

// `h` (optional): the handle whose next step will run on these buffers.  When its index pass can use them (segment mode,
// num_items <= 65 536, whole batch a multiple of 16), the sampler also writes the high and the low byte of every item id into
// the handle's byte planes (2 B per occurrence): k_index_seg's owners then scan ONE byte per occurrence -- sixteen values per
// 16-byte load, tested together -- instead of four bytes and a compare per value.  batch_offset / batch_size: this call fills
// triplets [batch_offset, batch_offset + B) of a batch of batch_size (an epoch crossing fills a batch in two calls); the planes
// are valid for the step that is called with exactly these buffers and B = batch_size, and are consumed by it.
static void plane_args(bprx_handle *h, const int32_t *pos, const int32_t *neg, int64_t B, int64_t batch_offset, int64_t batch_size,
                       uint8_t **own8, uint8_t **loc8, long long *pl_i, long long *pl_j, int *sh, QueueArgs *qa) {
  const SamplerFeed f = sampler_feed(h, pos, neg, B, batch_offset, batch_size);      // (moves the handle's tags: bprx_internal.h)
  *own8 = f.planes ? h->own8 : nullptr; *loc8 = f.planes ? h->loc8 : nullptr;
  *pl_i = f.pl_i; *pl_j = f.pl_j; *sh = f.sh;
  // the owner queues of the same occurrences (shift 8, 2 * batch_size <= 2^24, BPRX_INDEX_QUEUE): a later call of the batch
  // numbers its regions on behind this one's
  *qa = QueueArgs{f.queues ? h->qrec : nullptr, f.queues ? h->qrange : nullptr, f.q0, f.qstride};
}

extern "C" int bprx_sample_epoch_h(bprx_handle *h, const int64_t *indptr, const int32_t *items_sorted, const int32_t *perm,
                                   const int64_t *epoch_ptr, const int32_t *pos_slot, int32_t num_users, int32_t num_items,
                                   uint64_t seed, uint32_t epoch, int64_t first, int64_t B, int32_t *user, int32_t *pos, int32_t *neg,
                                   int64_t batch_offset, int64_t batch_size, void *stream) {
  if (!indptr || !items_sorted || !perm || !epoch_ptr || !user || !pos || !neg || num_users <= 0 || num_items <= 0 ||
      B < 0 || first < 0)
    return BPRX_E_INVALID;
  if (B == 0) return BPRX_OK;
  uint8_t *own8, *loc8;
  long long pl_i, pl_j;
  int sh;
  QueueArgs qa;
  plane_args(h, pos, neg, B, batch_offset, batch_size, &own8, &loc8, &pl_i, &pl_j, &sh, &qa);
  hipLaunchKernelGGL(k_sample_epoch, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, (hipStream_t)stream, indptr,
                     items_sorted, perm, epoch_ptr, pos_slot, num_users, (uint32_t)num_items, (uint32_t)seed, (uint32_t)(seed >> 32),
                     epoch, (long long)first, (long long)B, user, pos, neg, own8, loc8, pl_i, pl_j, sh, qa);
  return hipGetLastError() == hipSuccess ? BPRX_OK : BPRX_E_HIP;
}

extern "C" int bprx_sample_epoch(const int64_t *indptr, const int32_t *items_sorted, const int32_t *perm,
                                 const int64_t *epoch_ptr, const int32_t *pos_slot, int32_t num_users, int32_t num_items, uint64_t seed,
                                 uint32_t epoch, int64_t first, int64_t B, int32_t *user, int32_t *pos, int32_t *neg,
                                 void *stream) {
  return bprx_sample_epoch_h(nullptr, indptr, items_sorted, perm, epoch_ptr, pos_slot, num_users, num_items, seed, epoch, first, B,
                             user, pos, neg, 0, 0, stream);
}

extern "C" int bprx_sample_philox_h(bprx_handle *h, const int64_t *indptr, const int32_t *items_sorted, const int32_t *pos_user,
                                    int64_t num_pos, int32_t num_items, uint64_t seed, uint64_t first, int64_t B, int32_t *user,
                                    int32_t *pos, int32_t *neg, int64_t batch_offset, int64_t batch_size, void *stream) {
  if (!indptr || !items_sorted || !pos_user || !user || !pos || !neg || num_pos <= 0 || num_items <= 0 || B < 0)
    return BPRX_E_INVALID;
  if (B == 0) return BPRX_OK;
  uint8_t *own8, *loc8;
  long long pl_i, pl_j;
  int sh;
  QueueArgs qa;
  plane_args(h, pos, neg, B, batch_offset, batch_size, &own8, &loc8, &pl_i, &pl_j, &sh, &qa);
  hipLaunchKernelGGL(k_sample_philox, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, (hipStream_t)stream, indptr,
                     items_sorted, pos_user, (unsigned long long)num_pos, (uint32_t)num_items, (uint32_t)seed,
                     (uint32_t)(seed >> 32), (unsigned long long)first, (long long)B, user, pos, neg, own8, loc8, pl_i, pl_j, sh, qa);
  return hipGetLastError() == hipSuccess ? BPRX_OK : BPRX_E_HIP;
}

extern "C" int bprx_sample_philox(const int64_t *indptr, const int32_t *items_sorted, const int32_t *pos_user,
                                  int64_t num_pos, int32_t num_items, uint64_t seed, uint64_t first, int64_t B,
                                  int32_t *user, int32_t *pos, int32_t *neg, void *stream) {
  return bprx_sample_philox_h(nullptr, indptr, items_sorted, pos_user, num_pos, num_items, seed, first, B, user, pos, neg, 0, 0,
                              stream);
}

// ---- the hard samplers: bprx_sample_philox_hard / bprx_sample_epoch_hard (include/bprx.h) ----
// Like the samplers above they stay outside the gate: nothing they read is written by a pending dense update, and a lazy-Adam
// catch-up of every row per batch would undo the lazy replay -- the rows are scored as stored.
static int hard_args(bprx_handle *h, const char *what, int32_t num_items, int32_t candidates, const float *Ps, int32_t *cand_out,
                     float *score_out, HardArgs *ha) {
  if (!h) return BPRX_E_INVALID;
  const ReadPlan rp = plan_read(*h, NEED_BOUND, KIND_PLAIN);
  if (rp.error) BPRX_FAIL(h, rp.error, rp.why, what);
  if (h->cfg.flags & (BPRX_FLAG_EXPORT_USER_GRAD | BPRX_FLAG_EXPORT_ITEM_GRAD))
    BPRX_FAIL(h, BPRX_E_INVALID, "%s: the handle's rows are staged by a multi-GPU driver, not the whole tables", what);
  if (candidates < 1 || candidates > HARD_MAX_C)
    BPRX_FAIL(h, BPRX_E_INVALID, "%s: candidates = %d outside [1, %d]", what, candidates, HARD_MAX_C);
  if (num_items != h->cfg.num_items)
    BPRX_FAIL(h, BPRX_E_INVALID, "%s: num_items = %d, the handle has %lld", what, num_items, (long long)h->cfg.num_items);
  const bool vb = h->cfg.model == BPRX_MODEL_VBPR;
  if (vb && !Ps) BPRX_FAIL(h, BPRX_E_INVALID, "%s: a VBPR handle needs the snapshot Ps (bprx_hard_snapshot)", what);
  const int k = h->cfg.embed_k, d = vb ? h->cfg.embed_d : 0;
  auto al16 = [](const void *p) { return ((uintptr_t)p & 15u) == 0; };
  *ha = HardArgs{h->t.Gu, h->t.Gi, h->t.Bi, vb ? h->t.Tu : nullptr, vb ? Ps : nullptr, k, d, vb ? h->PS : 0, candidates,
                 (int)h->cfg.num_users, k % 4 == 0 && al16(h->t.Gu) && al16(h->t.Gi), vb && d % 4 == 0 && al16(h->t.Tu) && al16(Ps),
                 cand_out, score_out};
  return BPRX_OK;
}

extern "C" int bprx_sample_philox_hard(bprx_handle *h, const int64_t *indptr, const int32_t *items_sorted, const int32_t *pos_user,
                                       int64_t num_pos, int32_t num_items, uint64_t seed, uint64_t first, int64_t B, int32_t *user,
                                       int32_t *pos, int32_t *neg, int64_t batch_offset, int64_t batch_size, void *stream,
                                       int32_t candidates, const float *Ps, int32_t *cand_out, float *score_out) {
  if (!h) return BPRX_E_INVALID;
  if (!indptr || !items_sorted || !pos_user || !user || !pos || !neg || num_pos <= 0 || num_items <= 0 || B < 0)
    BPRX_FAIL(h, BPRX_E_INVALID, "sample_philox_hard: null pointer or bad size");
  HardArgs ha;
  { const int rc = hard_args(h, "sample_philox_hard", num_items, candidates, Ps, cand_out, score_out, &ha); if (rc) return rc; }
  if (B == 0) return BPRX_OK;
  uint8_t *own8, *loc8;
  long long pl_i, pl_j;
  int sh;
  QueueArgs qa;
  plane_args(h, pos, neg, B, batch_offset, batch_size, &own8, &loc8, &pl_i, &pl_j, &sh, &qa);
  StreamArgs sa = {};
  sa.indptr = indptr; sa.items = items_sorted; sa.pos_user = pos_user;
  sa.N = (unsigned long long)num_pos; sa.first = (unsigned long long)first;
  sa.I = (uint32_t)num_items; sa.k0 = (uint32_t)seed; sa.k1 = (uint32_t)(seed >> 32); sa.w3 = 0u;
  hipLaunchKernelGGL(k_sample_hard<false>, dim3((unsigned)((B + 255) / 256)), dim3(HARD_T), 0, (hipStream_t)stream, sa, ha, (long long)B,
                     user, pos, neg, own8, loc8, pl_i, pl_j, sh, qa);
  BPRX_LAUNCH_CHECK(h, "k_sample_hard<philox>");
  return BPRX_OK;
}

extern "C" int bprx_sample_epoch_hard(bprx_handle *h, const int64_t *indptr, const int32_t *items_sorted, const int32_t *perm,
                                      const int64_t *epoch_ptr, const int32_t *pos_slot, int32_t num_users, int32_t num_items,
                                      uint64_t seed, uint32_t epoch, int64_t first, int64_t B, int32_t *user, int32_t *pos, int32_t *neg,
                                      int64_t batch_offset, int64_t batch_size, void *stream, int32_t candidates, const float *Ps,
                                      int32_t *cand_out, float *score_out) {
  if (!h) return BPRX_E_INVALID;
  if (!indptr || !items_sorted || !perm || !epoch_ptr || !user || !pos || !neg || num_users <= 0 || num_items <= 0 || B < 0 || first < 0)
    BPRX_FAIL(h, BPRX_E_INVALID, "sample_epoch_hard: null pointer or bad size");
  HardArgs ha;
  { const int rc = hard_args(h, "sample_epoch_hard", num_items, candidates, Ps, cand_out, score_out, &ha); if (rc) return rc; }
  if (B == 0) return BPRX_OK;
  uint8_t *own8, *loc8;
  long long pl_i, pl_j;
  int sh;
  QueueArgs qa;
  plane_args(h, pos, neg, B, batch_offset, batch_size, &own8, &loc8, &pl_i, &pl_j, &sh, &qa);
  StreamArgs sa = {};
  sa.indptr = indptr; sa.items = items_sorted; sa.perm = perm; sa.epoch_ptr = epoch_ptr; sa.pos_slot = pos_slot;
  sa.U = num_users; sa.first = (unsigned long long)first;
  sa.I = (uint32_t)num_items; sa.k0 = (uint32_t)seed; sa.k1 = (uint32_t)(seed >> 32); sa.w3 = epoch;
  hipLaunchKernelGGL(k_sample_hard<true>, dim3((unsigned)((B + 255) / 256)), dim3(HARD_T), 0, (hipStream_t)stream, sa, ha, (long long)B,
                     user, pos, neg, own8, loc8, pl_i, pl_j, sh, qa);
  BPRX_LAUNCH_CHECK(h, "k_sample_hard<epoch>");
  return BPRX_OK;
}
