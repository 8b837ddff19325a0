#!/bin/bash
# GPU parity suite under the library's mode switches (one pytest process per setting, sequentially).  One log per setting
# under $ENV_MATRIX_LOGS (default build/env_matrix, git-ignored).
set -u
cd "$(dirname "$0")/.."
LOGS=${ENV_MATRIX_LOGS:-build/env_matrix}
mkdir -p "$LOGS"
SETTINGS=("BPRX_LIST_MODE=0" "BPRX_LIST_MODE=2" "BPRX_ITEM_MODE=0" "BPRX_ITEM_MODE=2" "BPRX_ADAM_LAZY=0" "BPRX_SIDE_STREAM=0")
# tests that assert the default a setting overrides: the benchmarked steps scan the sampler's byte planes (segment mode only);
# the lazy form of adam_tf23 (multi-GPU adam_tf23 needs it: bprx_create rejects the sweeps there); the E / Bp bound of the
# bench-shape lazy-vs-sweeps test, set for occurrence segments (the atomic staging path's fp32 atomic-order noise exceeds it
# in some runs: 0.0625 vs 0.05 lr)
BYTE_PLANES="full_size_step_on_the_epoch_walk or epoch_walk_steps_in_the_bench_form"
declare -A DESELECT=(["BPRX_LIST_MODE=2"]=$BYTE_PLANES
                     ["BPRX_ITEM_MODE=0"]="$BYTE_PLANES or lazy_adam_matches_the_sweeps_at_the_bench_shape"
                     ["BPRX_ADAM_LAZY=0"]="under_lazy_adam or two_ranks_adam_tf23")
for envs in "${SETTINGS[@]}"; do
  tag=$(echo "$envs" | tr ' =' '__')
  sel="(parity or listmode or adam or fullsize or hint or train_e2e) and not replicated and not train_rec_cli"
  [ -n "${DESELECT[$envs]:-}" ] && sel="$sel and not (${DESELECT[$envs]})"
  ( for kv in $envs; do export "$kv"; done
    timeout -k 10 600 python -m pytest tests -q -m gpu -x -k "$sel" > "$LOGS/matrix_$tag.log" 2>&1 )
  rc=$?
  echo "== $envs rc=$rc: $(tail -1 "$LOGS/matrix_$tag.log")"
  if [ $rc -eq 124 ] || [ $rc -eq 137 ]; then echo "TIMEOUT: stopping"; exit 1; fi
done
