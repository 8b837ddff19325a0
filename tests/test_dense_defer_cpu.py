"""What plan_step decides about the dense E|Bp update across two steps, checked without a GPU.

tests/dense_defer_cases.hip value-initialises a bprx_handle, sets host fields only (among them the new ones: the pending record's
`on` and the BPRX_DENSE_DEFER policy), calls plan_step and prints one line per case.  The expected lines are written from the
rules of the deferred update as DESIGN §4 states them, never from the code under test.  With vb = VBPR (every case here), I = 1000:

  list_mode     list_policy == 2 || (list_policy == 1 && 2B < I)
  item_mode     !list_mode && (seg_policy == 2 || (seg_policy == 1 && 2B >= I))
  mask          item_mode && !p_valid && (proj_mask == 2 ? dtype != fp32 : (proj_mask == 1 && dtype == bf16 && PS / 16 <= 9))
  dense         !factored || dtype == bf16 || list_mode
  fused         the caller is bprx_step && !factored
  defer_ok      policy && dense && fused && !list_mode && !factored         (a step may leave ITS update to the next one)
  carry         pending && item_mode                                       (the LAST step's update rides in k_index_seg)
  settle_first  pending && !carry                                          (list mode, atomic staging, B = 0: stand-alone kernel first)
  index_first   list_mode || mask || carry                                 (the carrying index pass runs before cast_Et / forward)
  empty batch   an error without the export flag; else no list, no segments: never defers, settles a pending update first
"""
import itertools
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "dense_defer_cases.hip")
I = 1000
FP32, BF16, FP8 = 0, 1, 2
FIELDS = "B opt export_user list_policy seg_policy proj_mask dtype PS p_valid fused factored pending defer".split()
BASE = dict(B=1024, opt=0, export_user=0, list_policy=1, seg_policy=1, proj_mask=1, dtype=BF16, PS=32, p_valid=0, fused=1, factored=0,
            pending=0, defer=1)


def _cases():
    out = []
    add = lambda **kw: out.append(dict(BASE, **kw))
    # segment, list, atomic-staging steps x pending x policy x caller
    for B, lp, sp, pend, defer, fused in itertools.product((64, 499, 500, 1024), (0, 1, 2), (0, 1, 2), (0, 1), (0, 1), (0, 1)):
        add(B=B, list_policy=lp, seg_policy=sp, pending=pend, defer=defer, fused=fused)
    # the mask and the projection cache do not decide who carries, only whether the index pass moved anyway
    for pm, dt, PS, pv, pend in itertools.product((0, 1, 2), (FP32, BF16, FP8), (32, 160), (0, 1), (0, 1)):
        add(proj_mask=pm, dtype=dt, PS=PS, p_valid=pv, pending=pend)
    # GradFashion never defers; the optimizer does not matter
    for fac, dt, opt, fused in itertools.product((0, 1), (FP32, BF16), (0, 1, 2), (0, 1)):
        add(factored=fac, dtype=dt, opt=opt, fused=fused)
    # the empty batch of a replicated rank
    for eu, pend, fused in itertools.product((0, 1), (0, 1), (0, 1)):
        add(B=0, export_user=eu, pending=pend, fused=fused)
    for B, pend in itertools.product((64, 1024), (0, 1)):
        add(B=B, export_user=1, pending=pend)
    return out


def _expect(c):
    B = c["B"]
    if B == 0 and not c["export_user"]:
        return "error=empty"
    fused = bool(c["fused"]) and not c["factored"]
    dense = (not c["factored"]) or c["dtype"] == BF16
    lm = im = mask = defer_ok = carry = False
    if B:
        lm = c["list_policy"] == 2 or (c["list_policy"] == 1 and 2 * B < I)
        im = not lm and (c["seg_policy"] == 2 or (c["seg_policy"] == 1 and 2 * B >= I))
        mask = (im and not c["p_valid"] and
                (c["dtype"] != FP32 if c["proj_mask"] == 2 else (c["proj_mask"] == 1 and c["dtype"] == BF16 and c["PS"] // 16 <= 9)))
        dense = dense or lm
        defer_ok = bool(c["defer"]) and dense and fused and not lm and not c["factored"]
        carry = bool(c["pending"]) and im
    settle = bool(c["pending"]) and not carry
    return "B=%d list=%d item=%d mask=%d index_first=%d dense=%d fused=%d defer_ok=%d carry=%d settle_first=%d" % (
        B, lm, im, mask, lm or mask or carry, dense, fused, defer_ok, carry, settle)


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    hipcc = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")) if c and os.path.exists(c)), None)
    assert hipcc, "hipcc is needed to build tests/dense_defer_cases.hip"
    tmp = tmp_path_factory.mktemp("dense_defer")
    exe, cases = str(tmp / "dense_defer_cases"), _cases()
    # the compile flags of fashionvisualexpl_recommend_amd/build.py
    subprocess.check_call([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I", os.path.join(REPO, "include"), "-I",
                           os.path.join(REPO, "fashionvisualexpl_recommend_amd", "csrc"), "-fvisibility=hidden", "-Wall",
                           "-Wno-unused-function", "-x", "hip", SRC, "-o", exe])
    (tmp / "cases.txt").write_text("".join(" ".join(str(c[f]) for f in FIELDS) + "\n" for c in cases))
    out = subprocess.run([exe, str(tmp / "cases.txt")], check=True, capture_output=True, text=True, timeout=60).stdout.splitlines()
    assert len(out) == len(cases)
    return cases, out


def test_every_case_follows_the_rules(lines):
    cases, out = lines
    bad = ["case %s\n  want %s\n  got  %s" % (c, _expect(c), got) for c, got in zip(cases, out) if got != _expect(c)]
    assert not bad, "%d of %d cases differ:\n%s" % (len(bad), len(cases), "\n".join(bad[:10]))


def test_pending_updates_are_carried_by_segment_steps_only(lines):
    cases, out = lines
    seen = set()
    for c, got in zip(cases, out):
        if got.startswith("error"):
            continue
        f = dict(kv.split("=") for kv in got.split())
        if c["pending"]:
            assert (f["carry"] == "1") == (f["item"] == "1") and f["settle_first"] == str(1 - int(f["carry"])), got
            if f["carry"] == "1":
                assert f["index_first"] == "1", got
            seen.add(("carry" if f["carry"] == "1" else "list" if f["list"] == "1" else "empty" if c["B"] == 0 else "atomic"))
        else:
            assert f["carry"] == f["settle_first"] == "0", got
        if c["factored"] or not c["fused"] or f["list"] == "1" or not c["defer"] or c["B"] == 0:
            assert f["defer_ok"] == "0", got
    assert seen == {"carry", "list", "empty", "atomic"}
    assert any(" defer_ok=1 " in l for l in out) and any(" mask=0 index_first=1 " in l and " carry=1 " in l for l in out)


def test_a_value_initialised_handle_plans_as_before(lines):
    """No policy, nothing pending (what tests/step_plan_cases.hip builds): no new field is set, index_first is list || mask."""
    cases, out = lines
    n = 0
    for c, got in zip(cases, out):
        if c["pending"] or c["defer"] or got.startswith("error"):
            continue
        f = dict(kv.split("=") for kv in got.split())
        assert f["defer_ok"] == f["carry"] == f["settle_first"] == "0", got
        assert f["index_first"] == str(int(f["list"] == "1" or f["mask"] == "1")), got
        n += 1
    assert n > 50
