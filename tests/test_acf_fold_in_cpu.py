"""Folding new users into ACF without a GPU: the three new symbols (declared, bound, exported, ABI still 6; a NULL handle is
rejected), the rules of --acf_new_users, the gate's new kind (DESIGN §4 "How a read is planned"), the restatement
(tests/acf_fold_in_ref.py): its forward against tests/acf_ref.py, the closed form of include/bprx.h against float64 autograd, and
the properties of every input set of tests/test_gpu_acf_fold_in.py that make its comparisons mean something."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import acf_fold_in_ref as R
from acf_ref import ACFRef
from fashionvisualexpl_recommend_amd import _ffi, train_rec

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "bprx.h")
SYMBOLS = {"bprx_acf_fold_in": 14, "bprx_acf_profile_rows": 7, "bprx_acf_score_rows_block": 9}


def test_symbols_are_declared_bound_and_exported():
    hdr = open(HEADER).read()
    assert re.search(r"#define\s+BPRX_ABI_VERSION\s+6\b", hdr) and _ffi.ABI_VERSION == 6
    lib = _ffi.lib()
    assert lib.bprx_abi_version() == 6
    for name, nargs in SYMBOLS.items():
        assert re.search(r"BPRX_API\s+int\s+%s\s*\(" % name, hdr), name
        assert name in _ffi.EXPORTS and hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == nargs, name


def test_a_null_handle_is_rejected():
    lib = _ffi.lib()
    assert lib.bprx_acf_fold_in(None, None, None, None, None, None, 0, 1, 0.1, 0.0, 0, None, None, None) == _ffi.E_INVALID
    assert lib.bprx_acf_profile_rows(None, None, 0, None, None, None, None) == _ffi.E_INVALID
    assert lib.bprx_acf_score_rows_block(None, None, 0, None, None, 0, 0, None, None) == _ffi.E_INVALID


def test_cli_flag():
    a = train_rec.parse_args(["--rec", "acf"])
    assert a.acf_new_users is None
    a = train_rec.parse_args(["--rec", "acf", "--acf_new_users", "f.tsv", "--fold_steps", "7", "--fold_negatives", "2"])
    assert a.acf_new_users == "f.tsv" and a.new_users is None and a.af_new_users is None and a.fold_steps == 7 and a.fold_negatives == 2
    for rec in ("bprmf", "vbpr", "grad_fashion", "attentive_fashion"):
        with pytest.raises(SystemExit):
            train_rec.parse_args(["--rec", rec, "--acf_new_users", "f.tsv"])
    for flag in ("--new_users", "--af_new_users"):                    # the other two keep rejecting acf
        with pytest.raises(SystemExit):
            train_rec.parse_args(["--rec", "acf", flag, "f.tsv"])
    for argv in (["--rec", "acf", "--acf_new_users", "f.tsv", "--fold_steps", "0"],
                 ["--rec", "acf", "--acf_new_users", "f.tsv", "--fold_negatives", "0"]):
        with pytest.raises(SystemExit):
            train_rec.parse_args(argv)


# ---- the gate: kind "an ACF-bound handle", needs bound tables -----------------------------------------------------------------------
BPRMF, VBPR_BF16, VBPR_FP8, FACTORED, ACF, AF = range(6)


def _gate_cases():
    out = []
    for model in range(6):
        for bound in (0, 1):
            for pend in (0, 1):
                for lazy, behind in ((0, 0), (1, 0), (1, 1)):
                    for pv in (0, 1):
                        if model >= FACTORED and not bound:       # (states that cannot exist: tests/test_read_gate_cpu.py)
                            continue
                        if model in (ACF, AF) and lazy:
                            continue
                        out.append((model, bound, pend, lazy, behind, pv))
    return out


def _gate_expect(c):
    """The row of the DESIGN §4 table: bound tables, an ACF handle; no rows to bring up to date, no image, no P."""
    model, bound, pend = c[:3]
    if not bound:
        return "error=state"
    if model != ACF:
        return "error=invalid"
    return "settle=%d sync=0 cast=0 project=0" % pend


def test_the_gate_takes_acf_handles_only(tmp_path):
    hipcc = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")) if c and os.path.exists(c)), None)
    assert hipcc, "hipcc is needed to build tests/acf_read_gate_cases.hip"
    exe, cases = str(tmp_path / "acf_read_gate_cases"), _gate_cases()
    # the compile flags of fashionvisualexpl_recommend_amd/build.py
    subprocess.check_call([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I", os.path.join(REPO, "include"), "-I",
                           os.path.join(REPO, "fashionvisualexpl_recommend_amd", "csrc"), "-fvisibility=hidden", "-Wall",
                           "-Wno-unused-function", "-x", "hip", os.path.join(REPO, "tests", "acf_read_gate_cases.hip"), "-o", exe])
    (tmp_path / "cases.txt").write_text("".join(" ".join(str(v) for v in c) + "\n" for c in cases))
    out = subprocess.run([exe, str(tmp_path / "cases.txt")], check=True, capture_output=True, text=True, timeout=60).stdout.splitlines()
    assert len(out) == len(cases)
    bad = ["case %s: want %s, got %s" % (c, _gate_expect(c), got) for c, got in zip(cases, out) if got != _gate_expect(c)]
    assert not bad, "%d of %d cases differ:\n%s" % (len(bad), len(cases), "\n".join(bad[:10]))
    assert {"error=state", "error=invalid", "settle=0 sync=0 cast=0 project=0", "settle=1 sync=0 cast=0 project=0"} <= set(out)


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def _f64(c):
    p = {n: torch.as_tensor(np.asarray(c["t"][n])).double() for n in R.FROZEN}
    return p, torch.as_tensor(c["F"]).double()


def test_the_forward_is_the_profile_of_acf_ref():
    c = R.case((16, 8, 4, 3))
    p, F = _f64(c)
    ref = ACFRef(dict(c["t"], Gu=c["G0"]), c["F"])
    for r in (0, 3, 12, 33, 34, 36):                                   # lengths 0, 1, 3, 9, 40 and the repeated item
        got = R.profile(torch.as_tensor(c["G0"][r]).double(), c["hists"][r], p, F)
        assert (got - ref.profile(r, c["hists"][r])).abs().max().item() <= 1e-13, r


def test_the_header_formulas_agree_with_autograd():
    """grad of include/bprx.h, written out by hand (acf_fold_in_ref.hand_grad), against float64 autograd of the loss: 1e-10."""
    c = R.case((16, 8, 4, 3))
    p, F = _f64(c)
    worst = 0.0
    for r in (1, 12, 22, 33, 34, 36, 38):      # no history; 3, 4, 9, 40 entries; a repeated item; a duplicated and an i == j pair
        a, b = c["ptr"][r], c["ptr"][r + 1]
        D = p["Gi"][torch.as_tensor(c["pos"][a:b]).long()] - p["Gi"][torch.as_tensor(c["neg"][a:b]).long()]
        g = torch.as_tensor(c["G0"][r]).double().requires_grad_(True)
        (want,) = torch.autograd.grad(R.user_loss(g, c["hists"][r], D, p, F, 0.05), g)
        got = R.hand_grad(g.detach(), c["hists"][r], D, p, F, 0.05)
        assert want.abs().max().item() > 1e-3
        worst = max(worst, (got - want).abs().max().item())
    print("hand formulas against autograd: %.3g" % worst)
    assert worst <= 1e-10


@pytest.mark.parametrize("shape,dtype,which", R.gpu_cases() + R.RAW_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_the_gpu_inputs_mean_something(shape, dtype, which):
    """(a) at most 10 % of the users with pairs are exposed (float64 min |relu input| < RELU_DELTA); (b) with either attention level
    held fixed the float64 trajectory leaves the full one by >= 100 x the allowance for at least half the users: a backward that is
    wrong through either level cannot pass.  One case of (b) cannot hold and is stated instead: at M = 1 beta is the softmax of one
    logit, identically 1, so the component level has no derivative to get wrong and the fixed-beta trajectory IS the full one
    (asserted: bit-equal).
    The float32 restatement's own largest deviation is printed next to the allowance: an input set on which float32 rounding alone
    comes near it would fail for no fault of the kernel."""
    k, h, a, M = shape
    c = R.case(shape, dtype)
    has = np.diff(c["ptr"]) > 0
    n = len(has)
    r64, r32 = R.run(shape, dtype, which), R.run(shape, dtype, which, torch.float32)
    allow, dev = R.allowance(r64, r32, has)
    exposed = has & (r64["min_relu"] < R.RELU_DELTA)
    sab = np.abs(R.run(shape, dtype, which, torch.float64, "alpha_beta")["Gu"] - r64["Gu"]).max(1)
    rb = R.run(shape, dtype, which, torch.float64, "beta")
    sb = np.abs(rb["Gu"] - r64["Gu"]).max(1)
    nab, nb = int((sab >= 100 * allow).sum()), int((sb >= 100 * allow).sum())
    print("%s %s %s: %d users, %d with pairs, %d exposed; allowance %.3g, float32 deviation up to %.3g; separated: %d (alpha and "
          "beta fixed), %d (beta fixed)" % (shape, dtype, which, n, has.sum(), exposed.sum(), allow, dev[has & ~exposed].max(), nab, nb))
    assert exposed.sum() <= 0.1 * has.sum()
    assert np.isfinite(r64["Gu"]).all() and np.isfinite(r64["loss"]).all()
    assert nab >= (n + 1) // 2
    if M == 1:
        assert np.array_equal(rb["Gu"], r64["Gu"])
    else:
        assert nb >= (n + 1) // 2
    assert (r64["loss"][has] < r64["loss_first"][has]).mean() > 0.9      # the fit goes down
    assert np.array_equal(r64["Gu"][~has], c["G0"][~has].astype(np.float64)) and not r64["loss"][~has].any()
