"""Folding new users into AttentiveFashion without a GPU: the two new symbols (declared, bound, exported, ABI still 6; a NULL handle
is rejected), the rules of --af_new_users, the gate's new kind (DESIGN §4 "How a read is planned"), and the restatement
(tests/af_fold_in_ref.py): its gradient against central differences, one sgd step against the train step of tests/attentive_ref.py
on the batch made of one user's pairs, and a falling loss."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import af_fold_in_ref as R
from attentive_ref import AttentiveRef, random_inputs, random_tables
from fashionvisualexpl_recommend_amd import _ffi, train_rec

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "bprx.h")
SYMBOLS = {"bprx_af_fold_in": 12, "bprx_af_score_rows_block": 8}
ATT = ("attention.W_1", "attention.b_1", "attention.W_2", "attention.b_2")


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
    assert lib.bprx_af_fold_in(None, None, None, None, 0, 1, 0.1, 0.0, 0, None, None, None) == _ffi.E_INVALID
    assert lib.bprx_af_score_rows_block(None, None, 0, 0, 0, None, None, None) == _ffi.E_INVALID


def test_cli_flag():
    a = train_rec.parse_args(["--rec", "attentive_fashion"])
    assert a.af_new_users is None
    a = train_rec.parse_args(["--rec", "attentive_fashion", "--af_new_users", "n.tsv", "--fold_steps", "7", "--fold_negatives", "2"])
    assert a.af_new_users == "n.tsv" and a.new_users is None and a.fold_steps == 7 and a.fold_negatives == 2
    for rec in ("bprmf", "vbpr", "grad_fashion", "acf"):
        with pytest.raises(SystemExit):
            train_rec.parse_args(["--rec", rec, "--af_new_users", "n.tsv"])
    for argv in (["--rec", "attentive_fashion", "--af_new_users", "n.tsv", "--fold_steps", "0"],
                 ["--rec", "attentive_fashion", "--af_new_users", "n.tsv", "--fold_negatives", "0"]):
        with pytest.raises(SystemExit):
            train_rec.parse_args(argv)
    with pytest.raises(NotImplementedError):
        train_rec.train(["--rec", "attentive_fashion", "--af_new_users", "n.tsv", "--world_size", "2"])


# ---- the gate: kind "an AttentiveFashion-bound handle", needs bound tables ---------------------------------------------------------
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
    """The row of the DESIGN §4 table: bound tables, an AttentiveFashion handle; no rows to bring up to date, no image, no P."""
    model, bound, pend = c[:3]
    if not bound:
        return "error=state"
    if model != AF:
        return "error=invalid"
    return "settle=%d sync=0 cast=0 project=0" % pend


def test_the_gate_takes_attentive_fashion_handles_only(tmp_path):
    hipcc = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")) if c and os.path.exists(c)), None)
    assert hipcc, "hipcc is needed to build tests/af_read_gate_cases.hip"
    exe, cases = str(tmp_path / "af_read_gate_cases"), _gate_cases()
    # the compile flags of fashionvisualexpl_recommend_amd/build.py
    subprocess.check_call([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I", os.path.join(REPO, "include"), "-I",
                           os.path.join(REPO, "fashionvisualexpl_recommend_amd", "csrc"), "-fvisibility=hidden", "-Wall",
                           "-Wno-unused-function", "-x", "hip", os.path.join(REPO, "tests", "af_read_gate_cases.hip"), "-o", exe])
    (tmp_path / "cases.txt").write_text("".join(" ".join(str(v) for v in c) + "\n" for c in cases))
    out = subprocess.run([exe, str(tmp_path / "cases.txt")], check=True, capture_output=True, text=True, timeout=60).stdout.splitlines()
    assert len(out) == len(cases)
    bad = ["case %s: want %s, got %s" % (c, _gate_expect(c), got) for c, got in zip(cases, out) if got != _gate_expect(c)]
    assert not bad, "%d of %d cases differ:\n%s" % (len(bad), len(cases), "\n".join(bad[:10]))
    assert {"error=state", "error=invalid", "settle=0 sync=0 cast=0 project=0", "settle=1 sync=0 cast=0 project=0"} <= set(out)


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def _case(seed, U=6, I=10, k=8, h=12, Dc=9, Dk=5):
    rs = np.random.RandomState(seed)
    t = random_tables(rs, U, I, k, Dc, Dk, h)
    t["Gu"] *= 4.0                                                    # widen the attention logits
    t["attention.W_1"] *= 4.0
    inputs = random_inputs(rs, I, Dc, Dk)
    ref = AttentiveRef(t, *inputs, reg=0.05, rate=0.0)
    with torch.no_grad():
        C = torch.stack(ref.encode(ref.p, np.arange(I))).numpy()     # [3, I, k], dropout off
    return rs, t, ref, C


def test_gradient_against_central_differences():
    rs, t, _, C = _case(1)
    I, k = t["Gi"].shape
    nr = 7
    items = torch.as_tensor(rs.randint(I, size=2 * nr))
    f = lambda a: torch.as_tensor(np.asarray(a)).double()
    c, gi = f(C)[:, items], f(t["Gi"])[items]
    W = [f(t[n]) for n in ATT]
    g = f(t["Gu"][2]).clone().requires_grad_(True)
    loss, pre, _ = R.user_loss(g, c, gi, nr, *W, 0.05)
    (gr,) = torch.autograd.grad(loss, g)
    (gr_fixed,) = torch.autograd.grad(R.user_loss(g, c, gi, nr, *W, 0.05, fixed_alpha=True)[0], g)
    assert pre.abs().min().item() > 1e-4                              # no relu kink within the difference step
    assert (gr - gr_fixed).abs().max().item() > 1e-3                  # (the softmax derivative is a visible part of the gradient)
    eps = 1e-6
    num = torch.zeros(k, dtype=torch.float64)
    with torch.no_grad():
        for q in range(k):
            d = torch.zeros(k, dtype=torch.float64); d[q] = eps
            num[q] = (R.user_loss(g + d, c, gi, nr, *W, 0.05)[0] - R.user_loss(g - d, c, gi, nr, *W, 0.05)[0]) / (2 * eps)
    err = (num - gr).abs().max().item()
    print("autograd against central differences: %.3g (|grad| up to %.3g)" % (err, gr.abs().max().item()))
    assert err <= 1e-7 * max(1.0, gr.abs().max().item())
    # the closed form of include/bprx.h against autograd
    with torch.no_grad():
        g = f(t["Gu"][2])
        pre = (g * c) @ W[0] + W[1]
        alpha = torch.softmax(torch.relu(pre) @ W[2].reshape(-1) + W[3].reshape(()), 0)
        tl = (g * c * gi).sum(-1)
        x = (alpha * tl).sum(0)
        dxdg = (alpha[:, :, None] * c).sum(0) * gi + \
            ((alpha * (tl - x))[:, :, None] * c * (((pre > 0).double() * W[2].reshape(-1)) @ W[0].T)).sum(0)
        d = x[:nr] - x[nr:]
        s = torch.sigmoid(-d)
        want = (-(s[:, None]) * (dxdg[:nr] - dxdg[nr:])).sum(0) + 2 * 0.05 * nr * g
    assert (want - gr).abs().max().item() <= 1e-12


def test_one_sgd_step_is_the_train_step_on_that_users_pairs():
    """steps = 1, sgd: the restatement moves the row as AttentiveRef.step (rate 0, no masks) moves Gu_u on the batch made of that
    user's pairs (a duplicated pair and an i == j pair among them)."""
    rs, t, ref, C = _case(2)
    I = t["Gi"].shape[0]
    u, B, lr = 3, 9, 0.05
    pos, neg = rs.randint(I, size=B), rs.randint(I, size=B)
    pos[3], neg[3] = pos[2], neg[2]
    neg[7] = pos[7]
    before = ref.p["Gu"].clone()
    ref.step((np.full(B, u), pos, neg), None, "sgd", lr)
    r = R.fold_in(C, t["Gi"], *(t[n] for n in ATT), [0, B], pos, neg, t["Gu"][u:u + 1], 1, lr, 0.05, "sgd")
    assert (ref.p["Gu"][u] - before[u]).abs().max().item() > 1e-4           # (the step moved the row at all)
    assert np.abs(ref.p["Gu"][u].numpy() - r["Gu"][0]).max() <= 1e-12
    others = np.arange(t["Gu"].shape[0]) != u
    assert torch.equal(ref.p["Gu"][others], before[others])                  # nobody else's row is regularised by these pairs


@pytest.mark.parametrize("opt,steps,lr", [("sgd", 20, 0.02), ("adam_tf23", 3, 0.05)])
def test_the_loss_falls_and_empty_users_stay(opt, steps, lr):
    rs, t, _, C = _case(3)
    I, k = t["Gi"].shape
    ptr = [0, 7, 7, 12, 13]
    pos, neg = rs.randint(I, size=13), rs.randint(I, size=13)
    G0 = (rs.standard_normal((4, k)) * 0.3).astype(np.float32)
    G0[3] = 0                                                              # a zero start is live
    r64, r32 = (R.fold_in(C, t["Gi"], *(t[n] for n in ATT), ptr, pos, neg, G0, steps, lr, 1e-3, opt, dt)
                for dt in (torch.float64, torch.float32))
    has = np.diff(ptr) > 0
    assert (r64["loss"][has] < r64["loss_first"][has]).all(), (r64["loss"], r64["loss_first"])
    assert np.array_equal(r32["Gu"][1], G0[1]) and r64["loss"][1] == 0 and np.isinf(r64["min_pre"][1])
    assert np.abs(r64["Gu"][3]).max() > 1e-4
    assert 0 < np.abs(r64["Gu"] - r32["Gu"]).max() < 1e-4
