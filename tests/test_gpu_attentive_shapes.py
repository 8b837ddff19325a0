"""AttentiveFashion's train step, scores and encoders on the MI355X against the float64 restatement (tests/attentive_ref.py) at the
cases of tests/af_step_cases.py: the default widths k = 128, h = 64, widths that are no multiple of any lane pass or tile, both
ends of the bind limit and k < 8 / h < 32; the dropout stream against its host restatement (tests/af_dropout_ref.py), bit for
bit; and the bind limits from both sides.  tests/test_af_step_cases_cpu.py holds on the CPU what these comparisons rely on.

The masks of every step are the RESTATED ones (asserted equal to the library's first).  Tolerances are the project's
(tests/test_gpu_attentive.py): scores, attentions and encodings 1e-5 absolute, alpha rows summing to 1 within 1e-6, the loss 1e-5
relative after the sgd step and 1e-4 at every Adam step.  Tables: that module's rule for the two conv tensors, here for all
fifteen: max(1e-6, 4 x the float32 restatement's own deviation of that tensor) after sgd, max(2e-5, 4 x ...) after three Adam
steps over the UNEXPOSED elements (af_step_cases.exposed: a float64 gradient that is non-zero and below 32 eps / sqrt(1 - beta2)
in any step: Adam's first steps turn such a gradient's sign into a +-lr move).

An exposed element must be finite and within 2 M (1 + 2^-20) + 3 ulp of float64, M = af_step_cases.adam_move_bound(lr, 3) =
3.005 lr: dense_adam_elem moves an element by lr_t |m_t| / (sqrt(v_t) + eps) a step, which Cauchy-Schwarz on m_t = (1 - b1)
sum b1^(t-i) g_i against v_t = (1 - b2) sum b2^(t-i) g_i^2 bounds by lr, 1.0014 lr and 1.0036 lr for t = 1, 2, 3 whatever the
gradients are; the GPU's and float64's elements both start at the same value, so they are at most 2 M apart; 2^-20 covers the
sixteen float32 roundings of the three updates' arithmetic and 3 ulp (of the tensor's largest magnitude) the three roundings of
the element itself.  Every comparison prints its triple (float32 deviation / allowance / GPU deviation) and the update size."""
import gc

import numpy as np
import pytest
import torch

import af_dropout_ref as D
import af_step_cases as K
from attentive_ref import AF_WEIGHTS, AttentiveRef, random_inputs, random_tables
from fashionvisualexpl_recommend_amd import _ffi
from test_gpu_attentive import _dev, _engine

pytestmark = pytest.mark.gpu
I_WIDE = 130                                                 # the first two cases' score handle: a second, partial item tile


def _bits(x):
    return x.detach().cpu().contiguous().view(torch.int32)


def _library_masks_are_the_restated(e, step, n_rows):
    want = K.masks_of(step, n_rows)
    for name, got, m in zip(("colour", "edges", "class"), e.af_dropout_mask(step, n_rows), want):
        assert torch.equal(got.cpu(), m), (name, step)
    return want


# ---- the dropout stream ----------------------------------------------------------------------------------------------------------
def test_dropout_masks_equal_the_host_restatement_bit_for_bit():
    rs = np.random.RandomState(1)
    t = random_tables(rs, 2, 2, 5, 3, 2, 7)
    inputs = random_inputs(rs, 2, 3, 2)
    n = 0
    for seed in (0, 7, (3 << 32) | 11):                      # the last: k1 != 0
        for rate in (0.5, 0.3, 1e-12):                       # 0.3: float32 rounds it; 1e-12: threshold 0
            e = _engine(t, inputs, B=40, rate=rate, seed=seed)
            for step in (0, 1, 2 ** 31 + 5):
                for n_rows in (1, 14, 80):
                    want = D.dropout_masks(seed, step, n_rows, rate)
                    got = e.af_dropout_mask(step, n_rows)
                    for name, g, w in zip(("colour", "edges", "class"), got, want):
                        assert g.dtype == torch.uint8 and tuple(g.shape) == w.shape
                        assert np.array_equal(g.cpu().numpy(), w), (name, seed, rate, step, n_rows)
                        n += w.size
            e.sync_check()
            e.close()
    print("dropout stream: %d mask bytes equal over 3 seeds x 3 rates x 3 steps x 3 row counts" % n)


# ---- scores, attentions, encodings -----------------------------------------------------------------------------------------------
def _score_case(k, h):
    """(tables, inputs) of the score handle: the case's own, for the first two cases over I_WIDE items (the images repeated, fresh
    Gi rows)"""
    c = K.case(k, h)
    if (k, h) not in K.ADAM_CASES:
        return c["t"], c["inputs"]
    from fashionvisualexpl_recommend_amd.synth import glorot_uniform
    t = dict(c["t"])
    t["Gi"] = glorot_uniform(np.random.RandomState(K.SEEDS[(k, h)] + 1000), I_WIDE, k)
    t["Bi"] = np.zeros(I_WIDE, np.float32)
    pick = np.arange(I_WIDE) % c["I"]
    return t, tuple(np.ascontiguousarray(x[pick]) for x in c["inputs"])


@pytest.mark.parametrize("k,h", list(K.CASES))
def test_scores_attentions_and_encodings_against_fp64(k, h):
    t, inputs = _score_case(k, h)
    U, I = t["Gu"].shape[0], t["Gi"].shape[0]
    e = _engine(t, inputs)
    ref = AttentiveRef(t, *inputs)
    bx, ba = ref.predict_all()
    sx, sa = e.af_score_block(0, U)
    tag = "scores k=%d h=%d I=%d" % (k, h, I)
    ex, ea = (sx.cpu().double() - bx).abs().max().item(), (sa.cpu().double() - ba).abs().max().item()
    es = (sa.sum(-1) - 1).abs().max().item()
    print("%s block: score error %.3g (|x| up to %.3g), alpha error %.3g, alpha rows sum to 1 within %.3g; alpha spans %.3f .. %.3f"
          % (tag, ex, bx.abs().max().item(), ea, es, ba.min().item(), ba.max().item()))
    assert ba.max().item() - ba.min().item() > 0.05                                # (the attention moves)
    assert ex <= 1e-5 and ea <= 1e-5 and es <= 1e-6
    assert (e.score_block(1, U).cpu().double() - bx[1:]).abs().max().item() <= 1e-5
    rs = np.random.RandomState(k + h)
    u, i = rs.randint(0, U, 60), rs.randint(0, I, 60)
    u[1], i[1] = u[0], i[0]                                                          # a pair twice
    with torch.no_grad():
        wx, wa, _ = ref.call(u, i)
    x, al = e.af_attention_pairs(u, i)
    px, pa = (x.cpu().double() - wx).abs().max().item(), (al.cpu().double() - wa).abs().max().item()
    ps = (e.score_pairs(u, i).cpu().double() - wx).abs().max().item()
    print("%s pairs: score error %.3g / %.3g (score_pairs), alpha error %.3g" % (tag, px, ps, pa))
    assert px <= 1e-5 and pa <= 1e-5 and ps <= 1e-5 and (al.sum(-1) - 1).abs().max().item() <= 1e-6
    items = list(range(min(I, 12))) + [I - 1, 3, 0, 3]
    with torch.no_grad():
        want = torch.stack(ref.encode(ref.p, items))
    ee = (e.af_encode(items).cpu().double() - want).abs().max().item()
    print("%s encode: error %.3g (|c| up to %.3g)" % (tag, ee, want.abs().max().item()))
    assert ee <= 1e-5
    e.sync_check()
    e.close()


# ---- one sgd step ------------------------------------------------------------------------------------------------------------------
def _tensors(e):
    return {n: e.t[n].clone() for n in K.TENSORS}


@pytest.mark.parametrize("k,h", list(K.CASES))
def test_sgd_step_every_tensor_against_fp64(k, h):
    c = K.case(k, h)
    r64, r32 = K.run(c, "sgd64"), K.run(c, "sgd32")
    B, batch = c["B"], c["batches"][0]
    tag = "sgd k=%d h=%d" % (k, h)
    out = []
    for _ in range(2):                                                              # two fresh handles: equal bits
        e = _engine(c["t"], c["inputs"], reg=K.SGD["reg"], lr=K.SGD["lr"], B=B, rate=K.RATE, seed=K.SEED)
        _library_masks_are_the_restated(e, 0, 2 * B)
        loss = e.step(*_dev(e, batch))
        out.append((loss.clone(), _tensors(e)))
        e.sync_check()
        e.close()
    got, want = float(out[0][0].item()), r64["loss"][0]
    print("%s: loss %.8g (float64 %.8g)" % (tag, got, want))
    assert abs(got - want) <= 1e-5 * abs(want), (got, want)
    fails = []
    for n in K.TENSORS:
        dev32, allow = K.sgd_allowance(c, n)
        err = float(np.abs(out[0][1][n].cpu().double().numpy().reshape(r64["p"][n].shape) - r64["p"][n]).max())
        print("%s %s: fp32 deviation %.3g, allowance %.3g, GPU deviation %.3g (update size %.3g)"
              % (tag, n, dev32, allow, err, np.abs(r64["p"][n] - c["p0"][n]).max()))
        if not err <= allow:
            fails.append((n, "fp32 deviation %.3g" % dev32, "allowance %.3g" % allow, "GPU deviation %.3g" % err))
    assert not fails, (tag, fails)
    assert torch.equal(_bits(out[0][0]), _bits(out[1][0])), "loss bits of two handles"
    for n in K.TENSORS:
        assert torch.equal(_bits(out[0][1][n]), _bits(out[1][1][n])), n


# ---- three Adam steps ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,h", K.ADAM_CASES)
def test_three_adam_steps_against_fp64(k, h):
    c = K.case(k, h)
    r64, r32 = K.run(c, "adam64"), K.run(c, "adam32")
    B, hp = c["B"], K.ADAM
    tag = "adam k=%d h=%d" % (k, h)
    e = _engine(c["t"], c["inputs"], optimizer=hp["optimizer"], reg=hp["reg"], lr=hp["lr"], B=B, rate=K.RATE, seed=K.SEED)
    for s in range(hp["steps"]):
        _library_masks_are_the_restated(e, s, 2 * B)
        got, want = float(e.step(*_dev(e, c["batches"][s])).item()), r64["loss"][s]
        print("%s step %d: loss %.8g (float64 %.8g)" % (tag, s, got, want))
        assert abs(got - want) <= 1e-4 * abs(want), (s, got, want)
    M = K.adam_move_bound(hp["lr"], hp["steps"])
    fails = []
    for n in K.TENSORS:
        want = r64["p"][n]
        got = e.t[n].cpu().double().numpy().reshape(want.shape)
        ex = K.exposed(c, n)
        un = ~ex
        dev32 = float(np.abs(r32["p"][n] - want)[un].max())
        allow = max(2e-5, 4.0 * dev32)
        err = float(np.abs(got - want)[un].max())
        far = 2.0 * M * (1.0 + 2.0 ** -20) + 3.0 * float(np.spacing(np.float32(np.abs(want).max())))
        err_ex = float(np.abs(got - want)[ex].max()) if ex.any() else 0.0
        print("%s %s: fp32 deviation %.3g, allowance %.3g, GPU deviation %.3g over the unexposed (update size %.3g); %d of %d exposed, "
              "GPU deviation over them %.3g (bound %.3g)" % (tag, n, dev32, allow, err, np.abs(want - c["p0"][n]).max(), ex.sum(),
                                                             ex.size, err_ex, far))
        if not (err <= allow and np.isfinite(got).all() and err_ex <= far):
            fails.append((n, "fp32 deviation %.3g" % dev32, "allowance %.3g" % allow, "GPU deviation %.3g" % err,
                          "exposed %.3g of %.3g" % (err_ex, far)))
    assert not fails, (tag, fails)
    e.sync_check()
    e.close()


# ---- the bind limits -----------------------------------------------------------------------------------------------------------------
def _limit_engine(k):
    from fashionvisualexpl_recommend_amd.engine import Engine
    return Engine(model="bprmf", num_users=3, num_items=5, embed_k=k, optimizer="sgd", lr=0.05, reg=0.0, max_batch=8)


def _bind(e, t, inputs):
    return e.bind_attentive(t["Gu"], t["Gi"], t["Bi"], *inputs, {n: t[n] for n in AF_WEIGHTS}, dropout=0.5, seed=7)


def _block_against_fp64(e, t, inputs, tag):
    bx, ba = AttentiveRef(t, *inputs).predict_all()
    sx, sa = e.af_score_block(0, 3)
    ex, ea = (sx.cpu().double() - bx).abs().max().item(), (sa.cpu().double() - ba).abs().max().item()
    print("%s: score error %.3g, alpha error %.3g" % (tag, ex, ea))
    assert ex <= 1e-5 and ea <= 1e-5 and (sa.sum(-1) - 1).abs().max().item() <= 1e-6
    e.sync_check()


@pytest.mark.parametrize("k,h,ok,words", K.LIMITS)
def test_bind_limits(k, h, ok, words):
    lib = _ffi.lib()
    rs = np.random.RandomState(k + h)
    t = random_tables(rs, 3, 5, k, 6, 4, h)
    t["Gu"] *= 4.0
    inputs = random_inputs(rs, 5, 6, 4)
    e = _limit_engine(k)
    if ok:
        _block_against_fp64(_bind(e, t, inputs), t, inputs, "bind k=%d h=%d" % (k, h))
        e.close()
        return
    gc.collect()
    live = lib.bprx_live_device_allocs()
    with pytest.raises(_ffi.BprxError) as ex:
        _bind(e, t, inputs)
    assert ex.value.code == _ffi.E_INVALID and words in str(ex.value), str(ex.value)
    assert lib.bprx_live_device_allocs() == live                                    # returned before any allocation or launch
    e.sync_check()
    out = torch.zeros((3, 1, k), device=e.device)
    items = torch.zeros(1, dtype=torch.int32, device=e.device)
    assert lib.bprx_af_encode(e.h, items.data_ptr(), 1, out.data_ptr(), None) == _ffi.E_STATE      # no model state was left
    # the handle binds afterwards: an accepted width of the same k where there is one, else the plain tables
    h_ok = next((w for w in (32, 64) if K.bind_accepts(k, w) is None), None)
    if h_ok is not None:
        t2 = random_tables(rs, 3, 5, k, 6, 4, h_ok)
        t2["Gu"] *= 4.0
        _block_against_fp64(_bind(e, t2, inputs), t2, inputs, "bind k=%d h=%d after the rejected h=%d" % (k, h_ok, h))
    else:
        e.bind(t["Gu"], t["Gi"], t["Bi"])
        want = torch.as_tensor(t["Gu"]).double() @ torch.as_tensor(t["Gi"]).double().T
        assert (e.score_block(0, 3).cpu().double() - want).abs().max().item() <= 1e-5
        e.sync_check()
    e.close()
