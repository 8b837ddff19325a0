"""Records what the step walk of tests/test_gpu_step_plan.py launches: one JSON line per walk (the per-phase launch counts, the
index-pass kind and the mask kind after every call).  Run against the build the test's table is to hold, on the GPU box:

    BPRX_LIB=/path/to/libbprx.so python scripts/record_step_plan.py > profiles/step_plan_walk_<build>.jsonl

(WALKS of the test is the record of the build before plan_step: profiles/step_plan_walk_parent.jsonl.)"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

import test_gpu_step_plan as sp  # noqa: E402

if __name__ == "__main__":
    for (dtype, form, export), name in zip(sp.CASES, sp.IDS):
        print(json.dumps({"walk": name, "lib": os.path.basename(os.environ.get("BPRX_LIB", "libbprx.so")),
                          "calls": sp.walk(os.environ.__setitem__, dtype, form, export)}), flush=True)
