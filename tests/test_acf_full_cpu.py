"""ACF's full-gradient mode without a GPU: the CLI flag, directory_parameters, the new exports, and the float64 restatement of
the full gradient (tests/acf_full_ref.py) -- against central finite differences, against the detached gradient on the inputs of
the GPU tests (so that those cannot pass with the detached step), and the relu guard those tests rely on."""
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

import acf_full_ref as R
from acf_ref import ACFRef, random_tables
from fashionvisualexpl_recommend_amd import _ffi, models, train_rec

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bprx.h")


def test_cli_flag_default_and_rejection():
    assert train_rec.parse_args(["--rec", "acf"]).acf_gradient == "detached"
    assert train_rec.parse_args(["--rec", "acf", "--acf_gradient", "full"]).acf_gradient == "full"
    assert train_rec.parse_args(["--rec", "vbpr"]).acf_gradient == "detached"
    with pytest.raises(SystemExit):
        train_rec.parse_args(["--rec", "acf", "--acf_gradient", "partial"])
    for rec in ("bprmf", "vbpr", "grad_fashion", "attentive_fashion"):
        with pytest.raises(SystemExit):
            train_rec.parse_args(["--rec", rec, "--acf_gradient", "full"])


class _StubEngine:
    def __init__(self, **kw):
        self.kw = kw

    def bind_acf(self, Gu, Gi, Bi, F, Pi, weights, train_lists, eval_lists=None, slots=None, gradient="detached"):
        self.gradient = gradient
        return self


def _model(monkeypatch, **over):
    monkeypatch.setattr(models, "Engine", _StubEngine)
    U, I = 12, 15
    rs = np.random.RandomState(4)
    train = [sorted(rs.choice(I, 4, replace=False).tolist()) for _ in range(U)]
    data = Namespace(num_users=U, num_items=I, training_list=train, validation_list=[], test_list=[],
                     params=Namespace(batch_eval=128))
    p = dict(epochs=1, batch_size=256, embed_k=128, lr=0.001, reg=0, top_k=20, dataset="toy", rec="acf",
             layers_component=[64, 1], layers_item=[64, 1], optimizer="adam_tf23", dtype="fp32", init_seed=0)
    p.update(over)
    return models.ACF(data, Namespace(**p), features=np.ones((I, 2, 8), np.float32))


def test_directory_parameters_suffix_in_full_mode_only(monkeypatch):
    base = "batch_256-K_128-lr_0.001-reg_0-comp_[64, 1]-item_[64, 1]"
    m = _model(monkeypatch)                                          # params without the attribute: detached
    assert (m.directory_parameters, m.acf_gradient, m.engine.gradient) == (base, "detached", "detached")
    m = _model(monkeypatch, acf_gradient="detached")
    assert (m.directory_parameters, m.engine.gradient) == (base, "detached")
    m = _model(monkeypatch, acf_gradient="full")
    assert (m.directory_parameters, m.engine.gradient) == (base + "-grad_full", "full")
    with pytest.raises(ValueError, match="acf_gradient"):
        _model(monkeypatch, acf_gradient="half")


def test_exports_in_header_and_binding():
    text = open(HEADER).read()
    for name in ("bprx_acf_set_gradient", "bprx_acf_get_gradient"):
        assert name in _ffi.EXPORTS
        assert ("BPRX_API int %s(bprx_handle *h" % name) in text
    assert "BPRX_ACF_GRAD_DETACHED = 0, BPRX_ACF_GRAD_FULL = 1" in text
    assert _ffi.ACF_GRADIENT == {"detached": 0, "full": 1}
    assert _ffi.ABI_VERSION == 6 and "#define BPRX_ABI_VERSION 6" in text


def test_full_gradient_against_central_differences():
    rs = np.random.RandomState(2)
    U, I, M, C, k = 5, 7, 3, 6, 4
    t = random_tables(rs, U, I, k, C, 3, 4, scale=10.0)
    F = np.abs(rs.standard_normal((I, M, C)))
    lists = [[], [1], [2, 2, 5], [0, 3, 4, 6], [1, 5]]
    batch = ([0, 3, 3, 2, 4], [1, 2, 2, 6, 0], [4, 4, 5, 0, 3])
    ref = R.ACFFullRef(t, F, reg=0.05)
    _, g = ref.grads(batch, lists)
    assert ref.min_relu > 1e-3                                      # no kink within the difference step
    eps = 1e-6
    for n in R.NAMES:
        flat = ref.p[n].reshape(-1)
        num = torch.zeros_like(flat)
        for e in range(flat.numel()):
            old = flat[e].item()
            with torch.no_grad():
                flat[e] = old + eps
                lp = ref.loss_of(ref.p, batch, lists).item()
                flat[e] = old - eps
                lm = ref.loss_of(ref.p, batch, lists).item()
                flat[e] = old
            num[e] = (lp - lm) / (2 * eps)
        err = (num - g[n].reshape(-1)).abs().max().item()
        assert err <= 1e-7 * max(1.0, g[n].abs().max().item()), (n, err)


def _cases():
    for dtype in ("fp32", "bf16"):
        yield ("special", dtype), R.special_case(dtype), (0.0, 0.1)
    for s in R.SHAPES:
        for dtype in ("fp32", "bf16"):
            if dtype == "fp32" or s[1] % 8 == 0:
                yield (s, dtype), R.grid_case(s, dtype), (0.1,)


def test_gpu_inputs_exercise_every_tensor_and_keep_b1_zero():
    """On the GPU tests' inputs, reg 0: full - detached gradient is far above the tolerances for every table but the two b_1,
    whose full gradient is zero up to float64 rounding."""
    for tag, (t, F, lists, batch), _ in _cases():
        full = R.ACFFullRef(t, F, reg=0.0)
        _, gf = full.grads(batch, lists)
        _, gd = ACFRef(t, F, reg=0.0).grads(batch, lists)
        for n in R.NAMES:
            diff = (gf[n] - gd[n]).abs().max().item()
            one_component = F.shape[1] == 1 and n.startswith("component.")     # M = 1: beta = 1, a constant
            if n in R.B1_NAMES or one_component:
                assert gf[n].abs().max().item() < 1e-12, (tag, n)
            else:
                assert diff > 1e-4, (tag, n, diff)                   # far above the allowances the GPU tests print
    t, F, lists, batches = R.adam_case(0.0)
    _, gf = R.ACFFullRef(t, F).grads(batches[0], lists)
    _, gd = ACFRef(t, F).grads(batches[0], lists)
    for n in R.NAMES:
        if n in R.B1_NAMES:
            assert gf[n].abs().max().item() < 1e-12, n
        else:
            assert (gf[n] - gd[n]).abs().max().item() > 1e-4, n


def test_relu_guard_holds_on_the_gpu_inputs():
    """min |relu input| > RELU_DELTA in float64, and the float32 restatement's relu inputs are within RELU_DELTA / 10 of them."""
    for tag, (t, F, lists, batch), regs in _cases():
        for reg in regs:
            _, _, mr = R.run_sgd(t, F, lists, batch, reg, 0.5, torch.float64)
            assert mr > R.RELU_DELTA, (tag, reg, mr)
        a, b = R.ACFFullRef(t, F), R.ACFFullRef(t, F, dtype=torch.float32)
        a.relu_inputs, b.relu_inputs = [], []
        users = sorted(set(int(u) for u in batch[0]))
        a.profiles(users, lists), b.profiles(users, lists)
        dev = max(float(np.abs(x - y).max()) for x, y in zip(a.relu_inputs, b.relu_inputs))
        assert dev <= R.RELU_DELTA / 10, (tag, dev)
    for reg in (0.0, 0.05):
        t, F, lists, batches = R.adam_case(reg)
        _, _, mr = R.run_adam(t, F, lists, batches, reg, R.ADAM_LR, torch.float64)
        assert mr > R.RELU_DELTA, (reg, mr)
