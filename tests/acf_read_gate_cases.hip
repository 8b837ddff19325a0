// acf_read_gate_cases.hip -- prints what plan_read (csrc/bprx_internal.h) decides for the entries that take an ACF-bound handle
// (bprx_acf_fold_in, bprx_acf_profile_rows, bprx_acf_score_rows_block: bound tables, kind "acf"); built and run by
// tests/test_acf_fold_in_cpu.py.  No GPU is needed: plan_read makes no HIP call and only host fields of the handle are set (as in
// read_gate_cases.hip).
//
// usage: acf_read_gate_cases CASES.txt  one case per line: model (0 BPRMF, 1 VBPR bf16, 2 VBPR fp8, 3 factored, 4 ACF-bound,
//                                       5 AttentiveFashion-bound) bound pending lazy behind p_valid
// output: one line per case, "settle=. sync=. cast=. project=.", or error=state / error=invalid
#include <stdio.h>
#include <string.h>

#include "bprx_internal.h"

static char g_state;                                        // what the acf / af pointers of a bound handle point at (never followed)

int main(int argc, char **argv) {
  FILE *f = argc > 1 ? fopen(argv[1], "r") : nullptr;
  if (!f) { fprintf(stderr, "usage: acf_read_gate_cases CASES.txt\n"); return 2; }
  int model, bound, pending, lazy, behind, p_valid, n;
  while ((n = fscanf(f, "%d %d %d %d %d %d", &model, &bound, &pending, &lazy, &behind, &p_valid)) == 6) {
    bprx_handle h{};                                        // every field zero; only host fields are set below
    h.cfg.model = model >= 1 && model <= 3 ? BPRX_MODEL_VBPR : BPRX_MODEL_BPRMF;
    h.cfg.feat_dtype = model == 2 ? BPRX_F_FP8 : BPRX_F_BF16;
    h.cfg.optimizer = lazy ? BPRX_OPT_ADAM_TF23 : BPRX_OPT_SGD;
    h.factored = model == 3;
    if (model == 4) h.acf = reinterpret_cast<AcfState *>(&g_state);
    if (model == 5) h.af = reinterpret_cast<AfState *>(&g_state);
    h.bound = bound != 0;
    h.pend.on = pending != 0;
    h.adam_lazy = lazy != 0;
    h.adam_t = 7; h.adam_synced = behind ? 5 : 7;
    h.p_valid = p_valid != 0;
    const ReadPlan p = plan_read(h, NEED_BOUND, KIND_ACF);
    if (p.error) {
      if (!p.why || !strstr(p.why, "%s")) { fprintf(stderr, "acf_read_gate_cases: an error without the entry's name\n"); return 2; }
      printf("error=%s\n", p.error == BPRX_E_STATE ? "state" : p.error == BPRX_E_INVALID ? "invalid" : "other");
    } else {
      printf("settle=%d sync=%d cast=%d project=%d\n", p.settle, p.sync, p.cast_et, p.project);
    }
  }
  fclose(f);
  if (n != EOF) { fprintf(stderr, "acf_read_gate_cases: bad case line (%d of 6 fields)\n", n); return 2; }
  return 0;
}
