"""What plan_read decides for every entry point that takes a handle, checked without a GPU.

tests/read_gate_cases.hip value-initialises a bprx_handle, sets host fields only, calls plan_read and prints one line per case.
The expected lines are written from the table of DESIGN §4 "How a read is planned", never from the code under test:

  error         not bound where the entry needs bound tables (state), else a handle of the wrong kind (invalid)
  settle        a dense update is pending                                   (every entry; the step stays outside the gate)
  sync          the entry needs current rows && lazy Adam && adam_synced < adam_t
  project       the entry needs P of all items && VBPR && !p_valid
  cast          VBPR && (the entry needs the image || project)               (the launcher skips a current image itself)

Handle states that cannot exist are left out: an ACF / AttentiveFashion / GradFashion handle is bound (its bind call makes it
one), and an ACF / AttentiveFashion handle is a BPRMF handle whose bind call turned lazy Adam off.
"""
import itertools
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "read_gate_cases.hip")
BPRMF, VBPR_BF16, VBPR_FP8, FACTORED, ACF, AF = range(6)
FIELDS = "model bound pending lazy behind p_valid need kind".split()
# entry points -> (needs, kind): B bound tables, R rows current, E the [E|Bp]^T image, P projections of all items
ENTRIES = {
    "score_block": ("BRP", "any"),
    "score_rows_block fold_in": ("BRP", "plain"),
    "step_project": ("BEP", "any"),
    "score_pairs without P": ("BRE", "any"),
    "score_pairs with P": ("BR", "any"),
    "project_rows score_new_block feat_explain_new": ("BRE", "nofp8"),
    "feat_explain": ("BR", "vbpr"),
    "explain_pairs": ("BR", "fact"),
    "sync_adam": ("BR", "any"),
    "topk topk_lists eval_* tables_dirty set_adam_step clear_*_grad sync_check pack_user_msg bind": ("-", "any"),
    "topk_rows": ("B", "nofp8"),
    "apply_user_msgs": ("B", "any"),
    "sum_dense_parts": ("-", "vbpr"),
}


def _cases():
    out = []
    for model, bound, pend, (lazy, behind), pv, (need, kind) in itertools.product(
            range(6), (0, 1), (0, 1), ((0, 0), (1, 0), (1, 1)), (0, 1), sorted(set(ENTRIES.values()))):
        if model >= FACTORED and not bound:
            continue
        if model in (ACF, AF) and lazy:
            continue
        out.append(dict(model=model, bound=bound, pending=pend, lazy=lazy, behind=behind, p_valid=pv, need=need, kind=kind))
    return out


def _expect(c):
    need, kind, m = c["need"], c["kind"], c["model"]
    vbpr = m in (VBPR_BF16, VBPR_FP8, FACTORED)
    if "B" in need and not c["bound"]:
        return "error=state"
    ok = {"any": True, "plain": m not in (ACF, AF), "vbpr": vbpr, "nofp8": vbpr and m != VBPR_FP8, "fact": m == FACTORED}[kind]
    if not ok:
        return "error=invalid"
    project = "P" in need and vbpr and not c["p_valid"]
    return "settle=%d sync=%d cast=%d project=%d" % (
        bool(c["pending"]), "R" in need and bool(c["lazy"]) and bool(c["behind"]),
        vbpr and ("E" in need or project), project)


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    hipcc = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")) if c and os.path.exists(c)), None)
    assert hipcc, "hipcc is needed to build tests/read_gate_cases.hip"
    tmp = tmp_path_factory.mktemp("read_gate")
    exe, cases = str(tmp / "read_gate_cases"), _cases()
    # the compile flags of fashionvisualexpl_recommend_amd/build.py
    subprocess.check_call([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I", os.path.join(REPO, "include"), "-I",
                           os.path.join(REPO, "fashionvisualexpl_recommend_amd", "csrc"), "-fvisibility=hidden", "-Wall",
                           "-Wno-unused-function", "-x", "hip", SRC, "-o", exe])
    (tmp / "cases.txt").write_text("".join(" ".join(str(c[f]) for f in FIELDS) + "\n" for c in cases))
    out = subprocess.run([exe, str(tmp / "cases.txt")], check=True, capture_output=True, text=True, timeout=60).stdout.splitlines()
    assert len(out) == len(cases)
    return cases, out


def test_every_case_follows_the_table(lines):
    cases, out = lines
    bad = ["case %s\n  want %s\n  got  %s" % (c, _expect(c), got) for c, got in zip(cases, out) if got != _expect(c)]
    assert not bad, "%d of %d cases differ:\n%s" % (len(bad), len(cases), "\n".join(bad[:10]))


def test_the_product_reaches_the_combinations(lines):
    cases, out = lines
    assert len({got for got in out if not got.startswith("error")}) >= 10 and {"error=state", "error=invalid"} <= set(out)
