// dense_defer_cases.hip -- prints what plan_step (csrc/bprx_internal.h) decides about the dense update across two steps; built
// and run by tests/test_dense_defer_cpu.py.  No GPU is needed: plan_step makes no HIP call and only host fields of the handle
// are set (as in step_plan_cases.hip).
//
// usage: dense_defer_cases CASES.txt     one case per line, the integers named in Case below, in that order
// output: one line per case, "name=value" pairs
#include <stdio.h>
#include <stdlib.h>

#include "bprx_internal.h"

struct Case {
  long long B;
  int opt /* 0 sgd, 1 swept Adam, 2 lazy Adam */, export_user, list_policy, seg_policy, proj_mask, dtype /* BPRX_F_* */, PS;
  int p_valid, fused, factored;
  int pending /* the last bprx_step left its update */, defer /* BPRX_DENSE_DEFER as bprx_create read it */;
};

static int32_t g_user[1024], g_pos[1024], g_neg[1024], g_ilist_n[2];

static void run(const Case &c) {
  bprx_handle h{};                                          // every field zero; only host fields are set below
  h.cfg.model = BPRX_MODEL_VBPR;
  h.cfg.optimizer = c.opt ? BPRX_OPT_ADAM_TF23 : BPRX_OPT_SGD;
  h.cfg.num_users = 200; h.cfg.num_items = 1000; h.cfg.embed_k = 32; h.cfg.max_batch = 1024;
  h.cfg.embed_d = c.PS - 12; h.cfg.feat_dim = 256;
  h.cfg.feat_dtype = c.dtype;
  h.cfg.lr = 0.05f; h.cfg.beta1 = 0.9f; h.cfg.beta2 = 0.999f; h.cfg.epsilon = 1e-7f;
  h.cfg.flags = c.export_user ? BPRX_FLAG_EXPORT_USER_GRAD : 0;
  h.adam_lazy = c.opt == 2;
  h.PS = c.PS; h.SK = 64; h.num_cu = 256; h.fwd_variant = 4;
  h.list_policy = c.list_policy; h.seg_policy = c.seg_policy; h.proj_mask = c.proj_mask;
  h.fast_rows = c.opt == 0 && !c.export_user;
  h.p_valid = c.p_valid; h.factored = c.factored;
  h.ilist_n = g_ilist_n;
  h.adam_t = 7; h.adam_synced = 7;
  h.step.SK_step = h.SK;
  h.dense_defer = c.defer;
  h.pend.on = c.pending != 0;
  const StepPlan p = plan_step(h, g_user, g_pos, g_neg, c.B, c.fused != 0);
  if (p.error) { printf("error=empty\n"); return; }
  printf("B=%lld list=%d item=%d mask=%d index_first=%d dense=%d fused=%d defer_ok=%d carry=%d settle_first=%d\n", (long long)p.B,
         p.list_mode, p.item_mode, p.mask, p.index_first, p.dense_launch, p.fused_reduce, p.defer_ok, p.carry_dense, p.settle_first);
}

int main(int argc, char **argv) {
  FILE *f = argc > 1 ? fopen(argv[1], "r") : nullptr;
  if (!f) { fprintf(stderr, "usage: dense_defer_cases CASES.txt\n"); return 2; }
  Case c;
  int n;
  while ((n = fscanf(f, "%lld %d %d %d %d %d %d %d %d %d %d %d %d", &c.B, &c.opt, &c.export_user, &c.list_policy, &c.seg_policy,
                     &c.proj_mask, &c.dtype, &c.PS, &c.p_valid, &c.fused, &c.factored, &c.pending, &c.defer)) == 13)
    run(c);
  fclose(f);
  if (n != EOF) { fprintf(stderr, "dense_defer_cases: bad case line (%d of 13 fields)\n", n); return 2; }
  return 0;
}
