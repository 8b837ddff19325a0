"""Who owns device memory: every buffer the library allocates is counted by bprx_live_device_allocs(), and every count here is an
exact integer compared with the count at the start of the test (samplers and engines of other tests may be alive).

Shapes are the smallest that reach every allocation branch of bprx_create and of the three model binds: U = 40, I = 48, k = 8,
max_batch = 64, one step of B = 32 (2B >= I: segment mode by default); bf16 features d = 8, D = 128; fp8 features d = 160, D = 256
(PS = 176, eleven column tiles: the scaled-MFMA image EtS exists)."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

from acf_ref import random_tables as acf_tables
from attentive_ref import AF_WEIGHTS, random_inputs
from attentive_ref import random_tables as af_tables
from fashionvisualexpl_recommend_amd import _ffi, synth

pytestmark = pytest.mark.gpu

U, I, K, MB, B = 40, 48, 8, 64, 32
ACF_C, ACF_H = 8, 8
AF_DC, AF_DK, AF_H = 5, 3, 8
# Buffers per owner, counted from the structs (a second allocation of the same buffer would show as one more):
N_BPRMF_SGD = 10 + 12 + 2   # staging, marks, loss, error flag, row counts | occurrence segments with both byte planes | shared-row list
N_ACF = 10                  # Z GP Wc gp Gup dPi uslot imark ilist nlist (fp32 features: one projection operand)
N_ACF_FULL = 7              # dGP q aux UV part gwbuf dZ
N_AF = 12 + 22              # the gradients of 13 tensors, conv bias inside the conv kernel's | the 22 row and item buffers


def live():
    return int(_ffi.lib().bprx_live_device_allocs())


def _engine(model="bprmf", **kw):
    from fashionvisualexpl_recommend_amd.engine import Engine
    kw.setdefault("optimizer", "sgd")
    return Engine(model=model, num_users=U, num_items=I, embed_k=K, lr=0.05, reg=1e-3, max_batch=MB, **kw)


def _tables(d=0, D=0, seed=0):
    rs = np.random.RandomState(seed)
    t = dict(Gu=synth.glorot_uniform(rs, U, K), Gi=synth.glorot_uniform(rs, I, K), Bi=(rs.standard_normal(I) * 0.01).astype(np.float32))
    if d:
        F = synth.make_features(I, D, seed=seed)
        t.update(Tu=synth.glorot_uniform(rs, U, d), F=(F / np.abs(F).max()).astype(np.float32), E=synth.glorot_uniform(rs, D, d),
                 Bp=synth.glorot_uniform(rs, D, 1).reshape(-1))
    return t


def _batch(seed=1):
    """B triplets with distinct users and every item at most once per role: no sum of more than two terms, whatever the order."""
    rs = np.random.RandomState(seed)
    dev = lambda a: torch.as_tensor(a.astype(np.int32), device="cuda")
    return dev(rs.permutation(U)[:B]), dev(rs.permutation(I)[:B]), dev(rs.permutation(I)[:B])


def _step(e):
    e.step(*_batch())
    e.sync_check()


def _vbpr(dtype, d, D, **kw):
    e = _engine("vbpr", embed_d=d, feat_dim=D, feat_dtype=dtype, **kw)
    return e.bind(**_tables(d, D))


def _acf_engine(M, seed=3, e=None):
    rs = np.random.RandomState(seed)
    t = acf_tables(rs, U, I, K, ACF_C, ACF_H, ACF_H)
    F = np.abs(rs.standard_normal((I, M, ACF_C))).astype(np.float32)
    lists = [sorted(rs.choice(I, 1 + u % 3, replace=False).tolist()) for u in range(U)]
    e = e or _engine()
    return e.bind_acf(t["Gu"], t["Gi"], t["Bi"], F, t["Pi"], {n: t[n] for n in _ffi.ACF_WEIGHTS}, lists)


_AF_INPUTS = []


def _af_bind(e, width=AF_H, seed=4):
    if not _AF_INPUTS:
        _AF_INPUTS.append(random_inputs(np.random.RandomState(9), I, AF_DC, AF_DK))
    t = af_tables(np.random.RandomState(seed), U, I, K, AF_DC, AF_DK, width)
    return e.bind_attentive(t["Gu"], t["Gi"], t["Bi"], *_AF_INPUTS[0], {n: t[n] for n in AF_WEIGHTS}, dropout=0.5, seed=7)


# ---- 1. create, step, destroy ------------------------------------------------------------------------------------------------
def _case_bprmf_sgd(mp):
    _step(_engine().bind(**_tables()))


def _case_bprmf_adam_lazy(mp):
    e = _engine(optimizer="adam_tf23", adam_form="lazy").bind(**_tables())
    assert e.adam_is_lazy()                                      # lastU, lastI, lr_hist
    _step(e)


def _case_vbpr_fp32(mp):
    _step(_vbpr("fp32", 8, 128))


def _case_vbpr_bf16_segments(mp):
    mp.setenv("BPRX_ITEM_MODE", "2")                             # segment scratch and byte planes
    _step(_vbpr("bf16", 8, 128))


def _case_vbpr_bf16_list(mp):
    mp.setenv("BPRX_LIST_MODE", "2")                             # ilist
    _step(_vbpr("bf16", 8, 128))


def _case_vbpr_fp8(mp):
    _step(_vbpr("fp8", 160, 256))                                # PS = 176: EtS


def _case_vbpr_bf16_adam_lazy(mp):
    e = _vbpr("bf16", 8, 128, optimizer="adam_tf23", adam_form="lazy")
    assert e.adam_is_lazy()                                      # side stream and its events
    _step(e)


def _case_user_msgs(mp):
    """BPRX_FLAG_EXPORT_USER_GRAD, one rank: two steps, the second with a larger message capacity (msg_next regrows)."""
    e = _vbpr("fp32", 8, 128, export_user_grad=True, dense_allreduce=True)
    counts = []
    for cap in (U, 2 * U):
        u, i, j = _batch(cap)
        msg = torch.zeros(e.user_msg_floats(cap), dtype=torch.float32, device="cuda")
        n0 = live()
        e.step_begin_sparse(u, i, j)
        e.pack_user_msg(u, cap, msg)
        e.step_begin_dense()
        e.apply_user_msgs(msg, 1, cap, -0.05)
        e.sum_dense_parts(e.dense_grad().clone(), 1)
        e.step_end(want_loss=False)
        e.sync_check()
        counts.append(live() - n0)
    assert counts == [1, 0], counts                              # the first call allocates msg_next, the regrow replaces it


def _case_gradfashion(mp):
    Dc, De, ec, ee, d, D = 40, 60, 4, 4, 8, 128
    rs = np.random.RandomState(2)
    t = _tables(d, D)
    t["F"][:, Dc + De:] = 0.0
    e = _engine("vbpr", embed_d=d, feat_dim=D, feat_dtype="bf16")
    e.bind_factored(t["Gu"], t["Gi"], t["Bi"], t["Tu"], t["F"], synth.glorot_uniform(rs, Dc, ec), synth.glorot_uniform(rs, De, ee),
                    synth.glorot_uniform(rs, ec + ee, d), synth.glorot_uniform(rs, ec + ee, 1).reshape(-1), Dc, De)
    _step(e)


def _case_acf(mp):
    e = _acf_engine(M=4)
    n0 = live()
    e.acf_set_gradient("full")                                   # the full-gradient workspace
    assert live() == n0 + N_ACF_FULL
    _step(e)
    users, items = list(range(8)), list(range(8))
    e.acf_explain(users, items, top=2, lists=[[u % I] for u in range(U)])
    n1 = live()
    e.acf_explain(users, items, top=2, lists=[[(u + q) % I for q in range(5)] for u in range(U)])     # xt regrows
    e.sync_check()
    assert live() == n1


def _case_attentive(mp):
    e = _af_bind(_engine())
    _step(e)
    users, items = list(range(8)), list(range(8))
    e.af_explain(users, items, grid=7)
    n1 = live()
    e.af_explain(users, items, grid=14)                          # E regrows
    e.sync_check()
    assert live() == n1


CASES = {f.__name__[len("_case_"):]: f for f in (
    _case_bprmf_sgd, _case_bprmf_adam_lazy, _case_vbpr_fp32, _case_vbpr_bf16_segments, _case_vbpr_bf16_list, _case_vbpr_fp8,
    _case_vbpr_bf16_adam_lazy, _case_user_msgs, _case_gradfashion, _case_acf, _case_attentive)}


@pytest.mark.parametrize("case", list(CASES))
def test_create_step_destroy_returns_to_baseline(case, monkeypatch):
    gc.collect()
    base = live()
    CASES[case](monkeypatch)
    gc.collect()
    assert live() == base


# ---- 2. rebinding ------------------------------------------------------------------------------------------------------------
def test_rebinding_leaves_nothing_behind(monkeypatch):
    monkeypatch.delenv("BPRX_ITEM_MODE", raising=False)         # the default policy: segment scratch whenever the widths fit
    gc.collect()
    base = live()
    e = _engine().bind(**_tables())
    plain = live()
    assert plain == base + N_BPRMF_SGD
    _acf_engine(M=4, e=e)
    _af_bind(e)
    _acf_engine(M=6, e=e)
    acf6 = live()
    assert acf6 == plain + N_ACF
    _acf_engine(M=4, e=e)                                        # straight from one ACF shape to another
    _acf_engine(M=6, e=e)
    assert live() == acf6
    _step(e)
    e.bind(**_tables())
    assert live() == plain
    _step(e)
    del e
    gc.collect()
    assert live() == base
    e2 = _acf_engine(M=6)                                        # a handle that was bound ACF at once holds the same
    assert live() == acf6
    del e2
    gc.collect()
    assert live() == base


# ---- 3. a failed create ------------------------------------------------------------------------------------------------------
def _one_step_tables():
    e = _engine().bind(**_tables(seed=5))
    _step(e)
    return {n: e.t[n].clone() for n in ("Gu", "Gi", "Bi")}


def test_failed_create_frees_what_it_made():
    L = _ffi.lib()
    want = _one_step_tables()                                    # a handle that never saw the failure
    gc.collect()
    base = live()
    # lossb alone is 4 TiB (the allocator refuses it at once); the five buffers before it are a few bytes each
    cfg = _ffi.Config(_ffi.ABI_VERSION, _ffi.MODEL["bprmf"], 4, 4, 4, 0, 0, 0, _ffi.OPTIMIZER["sgd"], torch.cuda.current_device(),
                      2 ** 40, 0.05, 0.0, 0.9, 0.999, 1e-7, 0, 448.0)
    h = C.c_void_p()
    assert L.bprx_create(C.byref(cfg), C.byref(h)) == _ffi.E_NOMEM
    assert not h.value
    assert live() == base
    assert b"allocation failed" in L.bprx_last_error(None)
    got = _one_step_tables()
    for n in want:
        assert torch.equal(got[n], want[n]), n
    gc.collect()
    assert live() == base


# ---- 4. an argument error at bind --------------------------------------------------------------------------------------------
def test_failed_bind_does_not_poison_the_handle():
    gc.collect()
    base = live()
    e = _engine().bind(**_tables())
    plain = live()
    with pytest.raises(_ffi.BprxError) as err:
        _af_bind(e, width=129)                                   # beyond the widest attention layer
    assert err.value.code == _ffi.E_INVALID
    assert live() == plain
    _af_bind(e)
    assert live() == plain + N_AF
    _step(e)
    del e, err
    gc.collect()
    assert live() == base
