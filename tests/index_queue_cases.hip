// index_queue_cases.hip -- prints what sampler_feed + plan_step (csrc/bprx_internal.h) decide about the samplers' owner queues, and
// what the record / addressing helpers give; built and run by tests/test_index_queue_cpu.py.  No GPU is needed: neither makes a
// HIP call, only host fields of the handle are set (as in dense_defer_cases.hip) and the buffers are tags that nobody follows.
//
// usage: index_queue_cases CASES.txt     one case per line:
//   P shift max_batch policy stale B_step ncalls n1 n2 n3 n4      a batch of n1 + .. + n_ncalls filled by ncalls sampler calls, then
//                                                                 planned as a step of B_step triplets
//   H occ local region slot owner stride lo hi max_batch          the helpers
// output: one line per case, "name=value" pairs
#include <stdio.h>
#include <stdlib.h>

#include "bprx_internal.h"

static int32_t g_user[16], g_pos[(1 << 23) + 64], g_neg[(1 << 23) + 64], g_other[16];
static uint8_t g_plane[16];
static uint32_t g_queue[16];

// stale: 0 nothing; 1 the step is called with another pos buffer; 2 a sampler call for another batch comes in between;
//        3 the second call does not continue the first (another neg pointer); 4 a step in between consumed the batch
static void plan(int shift, long long MB, int policy, int stale, long long Bstep, int ncalls, const long long *n) {
  bprx_handle h{};                                          // every field zero; only host fields are set below
  h.cfg.model = BPRX_MODEL_BPRMF;
  h.cfg.optimizer = BPRX_OPT_SGD;
  h.cfg.num_users = 200; h.cfg.num_items = shift == 8 ? 1000 : 70000; h.cfg.embed_k = 32; h.cfg.max_batch = MB;
  h.cfg.lr = 0.05f;
  h.num_cu = 256;
  h.seg_policy = 2;
  h.own8 = g_plane; h.loc8 = g_plane; h.idx8_shift = shift;
  h.qrec = g_queue; h.qrange = g_queue; h.index_queue = policy;
  long long size = 0, off = 0;
  for (int c = 0; c < ncalls; ++c) size += n[c];
  for (int c = 0; c < ncalls; ++c) {
    const int32_t *ng = g_neg + off;
    if (stale == 3 && c == 1) ng = g_other;
    sampler_feed(&h, g_pos + off, ng, n[c], off, size);
    off += n[c];
  }
  if (stale == 2) sampler_feed(&h, g_other, g_other, 16, 0, 16);
  if (stale == 4) { h.idx8_n = 0; h.idxq_n = 0; h.idxq_trip = 0; }     // (what commit_plan does)
  const StepPlan p = plan_step(h, g_user, stale == 1 ? g_other : g_pos, g_neg, Bstep);
  printf("item=%d idx8=%d queue=%d regions=%d kind=%d\n", p.item_mode, p.idx8, p.idxq, p.idxq_regions, p.idx_kind);
}

int main(int argc, char **argv) {
  FILE *f = argc > 1 ? fopen(argv[1], "r") : nullptr;
  if (!f) { fprintf(stderr, "usage: index_queue_cases CASES.txt\n"); return 2; }
  char kind;
  while (fscanf(f, " %c", &kind) == 1) {
    if (kind == 'P') {
      int shift, policy, stale, ncalls;
      long long MB, Bstep, n[4];
      if (fscanf(f, "%d %lld %d %d %lld %d %lld %lld %lld %lld", &shift, &MB, &policy, &stale, &Bstep, &ncalls, n, n + 1, n + 2, n + 3) != 10 ||
          ncalls < 1 || ncalls > 4) { fprintf(stderr, "index_queue_cases: bad P line\n"); return 2; }
      plan(shift, MB, policy, stale, Bstep, ncalls, n);
    } else if (kind == 'H') {
      unsigned occ, local, lo, hi;
      int region, slot, owner, stride;
      long long mb;
      if (fscanf(f, "%u %u %d %d %d %d %u %u %lld", &occ, &local, &region, &slot, &owner, &stride, &lo, &hi, &mb) != 9) {
        fprintf(stderr, "index_queue_cases: bad H line\n"); return 2;
      }
      const uint32_t rec = ixq_pack(occ, local), rg = ixq_range(lo, hi);
      printf("rec=%u occ=%u local=%u rec_at=%zu range_at=%zu lo=%u hi=%u regions=%lld\n", rec, ixq_occ(rec), ixq_local(rec),
             ixq_rec_at(region, slot), ixq_range_at(owner, region, stride), ixq_lo(rg), ixq_hi(rg), (long long)ixq_regions(mb));
    } else { fprintf(stderr, "index_queue_cases: bad line kind %c\n", kind); return 2; }
  }
  fclose(f);
  return 0;
}
