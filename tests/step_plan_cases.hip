// step_plan_cases.hip -- prints what plan_step (csrc/bprx_internal.h) decides for a list of cases; built and run by
// tests/test_step_plan_cpu.py.  No GPU is needed: plan_step makes no HIP call and only host fields of the handle are set.
//
// usage: step_plan_cases CASES.txt     one case per line, the integers named in FIELDS below, in that order
// output: one line per case, "name=value" pairs (see print_plan)
#include <stdio.h>
#include <stdlib.h>

#include "bprx_internal.h"

// the order of the integers of a case line (tests/test_step_plan_cpu.py: FIELDS)
struct Case {
  long long B;
  int vbpr, opt /* 0 sgd, 1 swept Adam, 2 lazy Adam */, export_user, export_item;
  int list_policy, seg_policy, proj_mask, dtype /* BPRX_F_* */, PS;
  int p_valid, proj_fresh, side, fused, factored;
  int fast_rows, slist, W_dirty, planes /* the sampler left byte planes of exactly this batch */;
  long long adam_t, adam_synced;
  int list_slot, seg_slot, slist_slot;
};

static int32_t g_user[1024], g_pos[1024], g_neg[1024], g_ilist_n[2], g_slist[4];
static uint8_t g_own8[2048];

static void print_plan(const Case &c, const StepPlan &p) {
  if (p.error) { printf("error=%s\n", p.error == PLAN_E_EMPTY ? "empty" : "?"); return; }
  static const char *const apply[] = {"none", "sgd_list", "sgd", "adam_lazy", "adam_sweep"};
  const bool kinds = p.apply == APPLY_SGD || p.apply == APPLY_ADAM_LAZY;
  printf("B=%lld idx=%d,%d,%d list=%d item=%d seg_users=%d fast=%d,%d,%d use_list=%d row_count=%d", (long long)p.B,
         p.user == g_user, p.pos == g_pos, p.neg == g_neg, p.list_mode, p.item_mode, p.seg_users, p.fast, p.fastU, p.fastI, p.use_list,
         p.row_count);
  printf(" list_bound=%lld list_cur=%d list_next=%d reset_cnt=%d", (long long)p.list_bound, p.list_cur ? (int)(p.list_cur - g_ilist_n) : -1,
         p.list_next ? (int)(p.list_next - g_ilist_n) : -1, p.list_reset_cnt);
  printf(" idx8=%d idx_kind=%d seg_cur=%d lead_over=%d slist_cur=%d", p.idx8, p.idx_kind, p.seg_cur, p.seg_lead_over, p.slist_cur);
  printf(" project=%d fwd=%d mask=%d index_first=%d", p.project, p.fwd, p.mask, p.index_first);
  printf(" adam_t=%lld sync_first=%d catchup=%d aside=%d", (long long)p.adam_t, p.adam_sync_first, p.catchup, p.catchup_aside);
  printf(" apply=%s", apply[p.apply]);
  if (kinds) printf(" kinds=%d,%d", p.fk, p.ek); else printf(" kinds=-");
  printf(" w_memset=%d leaves_w_dirty=%d SK_step=%d fused=%d dense=%d lr_t=%.9g\n", p.w_memset, p.leaves_w_dirty, p.SK_step,
         p.fused_reduce, p.dense_launch, (double)p.lr_t);
}

static void run(const Case &c) {
  bprx_handle h{};                                          // every field zero; only host fields are set below
  h.cfg.model = c.vbpr ? BPRX_MODEL_VBPR : BPRX_MODEL_BPRMF;
  h.cfg.optimizer = c.opt ? BPRX_OPT_ADAM_TF23 : BPRX_OPT_SGD;
  h.cfg.num_users = 200; h.cfg.num_items = 1000; h.cfg.embed_k = 32; h.cfg.max_batch = 1024;
  h.cfg.embed_d = c.vbpr ? c.PS - 12 : 0; h.cfg.feat_dim = c.vbpr ? 256 : 0;
  h.cfg.feat_dtype = c.dtype;
  h.cfg.lr = 0.05f; h.cfg.beta1 = 0.9f; h.cfg.beta2 = 0.999f; h.cfg.epsilon = 1e-7f;
  h.cfg.flags = (c.export_user ? BPRX_FLAG_EXPORT_USER_GRAD : 0) | (c.export_item ? BPRX_FLAG_EXPORT_ITEM_GRAD : 0);
  h.adam_lazy = c.opt == 2;
  h.PS = c.vbpr ? c.PS : 0; h.SK = 64; h.num_cu = 256; h.fwd_variant = 4;
  h.list_policy = c.list_policy; h.seg_policy = c.seg_policy; h.proj_mask = c.proj_mask;
  h.fast_rows = c.fast_rows; h.slist = c.slist ? g_slist : nullptr;
  h.p_valid = c.p_valid; h.proj_fresh = c.proj_fresh; h.W_dirty = c.W_dirty; h.factored = c.factored;
  h.side = c.side ? (hipStream_t)&g_slist : nullptr;        // (only tested against nullptr)
  h.ilist_n = g_ilist_n;
  h.adam_t = c.adam_t; h.adam_synced = c.adam_synced;
  h.list_slot = c.list_slot; h.seg_slot = c.seg_slot; h.slist_slot = c.slist_slot;
  h.step.SK_step = h.SK;                                    // (as bprx_create leaves it)
  if (c.seg_policy) { h.idx8_shift = 8; h.own8 = g_own8; }
  if (c.planes) { h.idx8_pos = g_pos; h.idx8_neg = g_neg; h.idx8_B = c.B; h.idx8_n = c.B; }
  print_plan(c, plan_step(h, g_user, g_pos, g_neg, c.B, c.fused != 0));
}

int main(int argc, char **argv) {
  FILE *f = argc > 1 ? fopen(argv[1], "r") : nullptr;
  if (!f) { fprintf(stderr, "usage: step_plan_cases CASES.txt\n"); return 2; }
  Case c;
  int n;
  while ((n = fscanf(f, "%lld %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %lld %lld %d %d %d", &c.B, &c.vbpr, &c.opt, &c.export_user,
                     &c.export_item, &c.list_policy, &c.seg_policy, &c.proj_mask, &c.dtype, &c.PS, &c.p_valid, &c.proj_fresh, &c.side,
                     &c.fused, &c.factored, &c.fast_rows, &c.slist, &c.W_dirty, &c.planes, &c.adam_t, &c.adam_synced, &c.list_slot,
                     &c.seg_slot, &c.slist_slot)) == 24)
    run(c);
  fclose(f);
  if (n != EOF) { fprintf(stderr, "step_plan_cases: bad case line (%d of 24 fields)\n", n); return 2; }
  return 0;
}
