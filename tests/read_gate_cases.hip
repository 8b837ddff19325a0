// read_gate_cases.hip -- prints what plan_read (csrc/bprx_internal.h) decides for an entry point's needs on a handle in a given
// state; built and run by tests/test_read_gate_cpu.py.  No GPU is needed: plan_read makes no HIP call and only host fields of the
// handle are set (as in dense_defer_cases.hip).
//
// usage: read_gate_cases CASES.txt     one case per line: the integers named in Case below, then the needs (letters of
//                                      B bound, R rows, E Et, P P-all, or -) and the kind (any plain vbpr nofp8 fact)
// output: one line per case, "name=value" pairs, or error=state / error=invalid
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bprx_internal.h"

struct Case {
  int model /* 0 BPRMF, 1 VBPR bf16, 2 VBPR fp8, 3 factored (VBPR bf16), 4 ACF-bound, 5 AttentiveFashion-bound */;
  int bound, pending, lazy, behind /* adam_synced < adam_t */, p_valid;
  char need[16], kind[16];
};

static char g_state;                                        // what the acf / af pointers of a bound handle point at (never followed)

static int run(const Case &c) {
  bprx_handle h{};                                          // every field zero; only host fields are set below
  h.cfg.model = c.model >= 1 && c.model <= 3 ? BPRX_MODEL_VBPR : BPRX_MODEL_BPRMF;
  h.cfg.feat_dtype = c.model == 2 ? BPRX_F_FP8 : BPRX_F_BF16;
  h.cfg.optimizer = c.lazy ? BPRX_OPT_ADAM_TF23 : BPRX_OPT_SGD;
  h.factored = c.model == 3;
  if (c.model == 4) h.acf = reinterpret_cast<AcfState *>(&g_state);
  if (c.model == 5) h.af = reinterpret_cast<AfState *>(&g_state);
  h.bound = c.bound != 0;
  h.pend.on = c.pending != 0;
  h.adam_lazy = c.lazy != 0;
  h.adam_t = 7; h.adam_synced = c.behind ? 5 : 7;
  h.p_valid = c.p_valid != 0;
  unsigned need = 0;
  for (const char *q = c.need; *q; ++q)
    need |= *q == 'B' ? NEED_BOUND : *q == 'R' ? NEED_ROWS : *q == 'E' ? NEED_ET : *q == 'P' ? NEED_P_ALL : 0u;
  static const char *const kinds[] = {"any", "plain", "vbpr", "nofp8", "fact"};
  static const int kind_of[] = {KIND_ANY, KIND_PLAIN, KIND_VBPR, KIND_VBPR_NO_FP8, KIND_FACTORED};
  int kind = -1;
  for (int q = 0; q < 5; ++q) if (!strcmp(c.kind, kinds[q])) kind = kind_of[q];
  if (kind < 0) return 2;
  const ReadPlan p = plan_read(h, need, kind);
  if (p.error) {
    if (!p.why || !strstr(p.why, "%s")) return 2;           // every error names its entry
    printf("error=%s\n", p.error == BPRX_E_STATE ? "state" : p.error == BPRX_E_INVALID ? "invalid" : "other");
  } else {
    printf("settle=%d sync=%d cast=%d project=%d\n", p.settle, p.sync, p.cast_et, p.project);
  }
  return 0;
}

int main(int argc, char **argv) {
  FILE *f = argc > 1 ? fopen(argv[1], "r") : nullptr;
  if (!f) { fprintf(stderr, "usage: read_gate_cases CASES.txt\n"); return 2; }
  Case c;
  int n;
  while ((n = fscanf(f, "%d %d %d %d %d %d %15s %15s", &c.model, &c.bound, &c.pending, &c.lazy, &c.behind, &c.p_valid, c.need,
                     c.kind)) == 8)
    if (run(c)) { fprintf(stderr, "read_gate_cases: bad need / kind / message (%s %s)\n", c.need, c.kind); return 2; }
  fclose(f);
  if (n != EOF) { fprintf(stderr, "read_gate_cases: bad case line (%d of 8 fields)\n", n); return 2; }
  return 0;
}
