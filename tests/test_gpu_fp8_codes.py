"""Every e4m3fn code, at every byte position of a 16-byte piece, through the four hand-written fp8 routes, and every rounding
boundary through the cast -- bit for bit.  Inputs and expected values: tests/fp8_code_cases.py (held on the CPU by
tests/test_fp8_code_cases_cpu.py): feat_scale and the scale of [E|Bp] are powers of two, every product is (4-bit significand) x
(4-bit significand) and every sum has one non-zero term, so every comparison below is == (+0 == -0).

case (test :: parameter)                  what is probed -> kernel instantiation reached (NT = PS/16 column tiles, N = CU count)
----------------------------------------  --------------------------------------------------------------------------------------
forward_whole_table::v10-nt1/5/9          feature codes (A) and [E|Bp] codes (B) into mfma_f32_16x16x32_fp8_fp8:
                                          launch_v10<NT> -> k_proj_fwd_bf16_v10<NT, F8 = true, NTL = false, MASK = false>, D 512
forward_whole_table::plain-nt3/12         BPRX_FWD_VARIANT=0: k_proj_fwd_bf16<NT, MTD = NT <= 9 ? 2 : 1, true>
forward_whole_table::oddD-nt4/10          D 768 (Deq % 256 != 0): the same plain kernel
forward_whole_table::f8s-nt10/17          launch_f8s<NT> -> k_proj_fwd_f8s<NT, false> (the block-scaled fp8 MFMA)
  (each also through bprx_hard_snapshot: the same launcher writing Ps, which must hold the same bits)
forward_row_list::split / mt1 / mt2 / mt4 score_pairs on a fresh handle, NT 2: k_proj_fwd_rows<1, 1, 16, true> (tiles * NT <= 2N),
                                          <2, 1, 8, true>, <2, 2, 8, true> (> 2N row tiles), <2, 4, 8, true> (> 8N)
forward_row_list::f8s_rows-4095 / -4096   NT 10: k_proj_fwd_rows<10, 1, 8, true> / k_proj_fwd_f8s<10, false> over the list
backward::db2                             feature codes through cvt_scalef32_pk_bf16_fp8: NT 2, launch_bwd_nt ->
                                          k_proj_bwd_bf16_v3<2, 32, 8, 2, true, ROWS = false, DB 2>
backward::ns2                             NT 10: k_proj_bwd_bf16_v3<10, 32, 8, 2, true, false, DB 2, NS 2>
backward::rows                            BPRX_LIST_MODE=2, NT 4: launch_bwd_rows -> k_proj_bwd_bf16_v3<4, 32, 8, 2, true, ROWS = true>
backward::masked                          BPRX_PROJ_MASK=2, segment mode, d = 60 (the mask needs d % 4 == 0):
                                          k_proj_bwd_bf16_v3<4, .., MASK = true>; bprx_proj_mask_kind == 1 is asserted
  (each read from dense_grad(): k_reduce_parts, and from -E_new / lr after an sgd step: k_dense_update's fused slab sum)
cast_and_maximum::every-boundary          f2e4m3 in k_cast_Et8 on every tie and its float32 neighbours; maxima at several places
cast_and_maximum::E-first .. E-negative   ONE entry of magnitude 448 / 2^J: after bind k_absmax finds it (Bp-last: the last element it
                                          reads); after an sgd step that leaves E unchanged k_dense_update's maximum does, followed by a
                                          second k_cast_Et8 -- BPRX_DENSE_DEFER=0 (stand-alone launch in the step), =1 settled by
                                          score_block, =1 carried into the next step's index pass where the plan defers
feat_explain_decodes_every_code           e4m3fn_value in k_feat_explain<uint8_t, 16, false> (16-byte row loads)
bf16_image_rounds_to_nearest_even         k_cast_Et (bind) and k_dense_update's bf16 image (after a step): normal numbers only --
                                          what the bf16 MFMA does with subnormal inputs on this part has not been measured

Observation (no new entry point, as tests/test_gpu_projections.py): one-hot visual users over zero Gu / Gi / Bi through score_block /
score_pairs (row n < d: P[t, n] + P[t, d], exact; row d: P[t, d]); dense_grad() between step_begin and step_end; -E_new / lr after
an sgd step with reg = 0 and lr = 0.5.
Reference: VBPR.py:83-84 (forward), VBPR.py:141 (dE, dBp); the code values: the OCP e4m3fn definition, checked against torch."""
import ctypes as C

import numpy as np
import pytest
import torch

import fp8_code_cases as fc
import test_gpu_projections as tp

pytestmark = pytest.mark.gpu

DEV = tp.DEV
LR = tp.LR                                                   # 0.5


def _dev(a):
    return torch.as_tensor(a, device=DEV)


def _f8(codes):
    return _dev(codes).view(torch.float8_e4m3fn)


def _engine(I, D, d, U, tables, max_batch=16, dtype="fp8", fs=fc.FS):
    from fashionvisualexpl_recommend_amd.engine import Engine
    return Engine(model="vbpr", num_users=U, num_items=I, embed_k=4, embed_d=d, feat_dim=D, feat_dtype=dtype, optimizer="sgd",
                  lr=LR, reg=0.0, max_batch=max_batch, feat_scale=fs).bind(**tables)


def _tables(I, d, U, Tu, F, E, Bp):
    z = lambda *s: torch.zeros(s, device=DEV)
    return dict(Gu=z(U, 4), Gi=z(I, 4), Bi=z(I), Tu=_dev(Tu), F=F, E=_dev(E), Bp=_dev(Bp))


def _exact(got, want, what):
    """got (device fp32) == want (float64 numpy) everywhere; +0 == -0; a NaN is a mismatch"""
    g = got.detach().double().cpu().numpy().reshape(want.shape)
    bad = ~(g == want)
    if bad.any():
        idx = np.argwhere(bad)
        first = ", ".join("%s: got %r want %r" % (tuple(int(x) for x in i), float(g[tuple(i)]), float(want[tuple(i)])) for i in idx[:6])
        raise AssertionError("%s: %d of %d values differ (%s)" % (what, int(bad.sum()), bad.size, first))


_F = {}


def _features(D):
    if D not in _F:
        _F[D] = _f8(fc.feature_codes(D))
    return _F[D]


_FWD = {}


def _forward(D, d):
    """tables of the decode cases and (P, scores) expected, made once per shape and never changed"""
    if (D, d) not in _FWD:
        E, Bp = fc.eb_tables(D, d)
        P = fc.forward_expected(D, d)
        _FWD[(D, d)] = (E, Bp, P, fc.scores_of(P))
    E, Bp, P, S = _FWD[(D, d)]
    return _tables(fc.I_ITEMS, d, d + 1, fc.one_hot_users(d), _features(D), E, Bp), P, S


# ---- 1. feature-code decode, forward ------------------------------------------------------------------------------------
FWD_CASES = [pytest.param(512, nt, 4, id="v10-nt%d" % nt) for nt in (1, 5, 9)] + \
            [pytest.param(512, nt, 0, id="plain-nt%d" % nt) for nt in (3, 12)] + \
            [pytest.param(768, nt, 4, id="oddD-nt%d" % nt) for nt in (4, 10)] + \
            [pytest.param(512, nt, 4, id="f8s-nt%d" % nt) for nt in (10, 17)]


@pytest.mark.parametrize("D,nt,variant", FWD_CASES)
def test_forward_whole_table(monkeypatch, D, nt, variant):
    from fashionvisualexpl_recommend_amd.engine import _stream
    monkeypatch.setenv("BPRX_FWD_VARIANT", str(variant))
    d = 16 * nt - 1
    tables, P, S = _forward(D, d)
    e = _engine(fc.I_ITEMS, D, d, d + 1, tables)
    got = e.score_block(0, d + 1)
    assert e.proj_stride() == d + 1
    ps = torch.full((fc.I_ITEMS, d + 1), float("nan"), device=DEV)
    assert e.lib.bprx_hard_snapshot(e.h, C.c_void_p(ps.data_ptr()), _stream()) == 0
    e.sync_check()
    e.close()
    _exact(got, S, "score_block")
    _exact(ps, P, "bprx_hard_snapshot")


def _row_cases():
    n = tp._ncu()
    return {"split": (2, 16 * (2 * n // 2) - 3), "mt1": (2, 16 * (n + 1) - 3), "mt2": (2, 16 * (2 * n + 1) - 3),
            "mt4": (2, 16 * (8 * n + 1) - 3), "f8s_rows-4095": (10, 4095), "f8s_rows-4096": (10, 4096)}


@pytest.mark.parametrize("form", ["split", "mt1", "mt2", "mt4", "f8s_rows-4095", "f8s_rows-4096"])
def test_forward_row_list(monkeypatch, form):
    """Every (output n, item t) as one pair of score_pairs on a fresh handle, in a fixed random order, `rows` pairs per call (the last
    call is shorter and may take a smaller form)."""
    monkeypatch.delenv("BPRX_FWD_VARIANT", raising=False)
    nt, rows = _row_cases()[form]
    D, d = 512, 16 * nt - 1
    tables, P, S = _forward(D, d)
    q = np.random.RandomState(nt).permutation((d + 1) * fc.I_ITEMS)
    users, items = q // fc.I_ITEMS, q % fc.I_ITEMS
    e = _engine(fc.I_ITEMS, D, d, d + 1, tables, max_batch=rows)
    got = e.score_pairs(users, items)
    e.sync_check()
    e.close()
    _exact(got, S[users, items], "score_pairs, %d rows per call" % rows)


# ---- 2. feature-code decode, backward -----------------------------------------------------------------------------------
BWD_FORMS = {"db2": (31, {"BPRX_LIST_MODE": "0"}, 0), "ns2": (159, {"BPRX_LIST_MODE": "0"}, 0), "rows": (63, {"BPRX_LIST_MODE": "2"}, 0),
             "masked": (60, {"BPRX_LIST_MODE": "0", "BPRX_ITEM_MODE": "2", "BPRX_PROJ_MASK": "2"}, 1)}


@pytest.mark.parametrize("form", list(BWD_FORMS))
def test_backward(monkeypatch, form):
    """One batch per group of 32 codes x 16 positions, each on its own fresh handle: inside a group every column belongs to one item,
    so dE|dBp[c_t] = val(a_t) W[t] / feat_scale has one term."""
    d, env, kind = BWD_FORMS[form]
    monkeypatch.delenv("BPRX_FWD_VARIANT", raising=False)
    for n, v in env.items():
        monkeypatch.setenv(n, v)
    D, I = 512, fc.I_ITEMS
    for g in range(fc.n_groups()):
        c = fc.backward_case(g, D, d)
        u, i, j = _dev(c["u"]), _dev(c["i"]), _dev(c["j"])
        for path in ("dense_grad", "sgd_step"):
            t = _tables(I, d, c["B"], c["Tu"], _features(D), np.zeros((D, d), np.float32), np.zeros(D, np.float32))
            e = _engine(I, D, d, c["B"], t, max_batch=c["B"])
            if path == "dense_grad":
                e.step_begin(u, i, j)
                gr = e.dense_grad().clone()
                e.step_end()
                got = torch.cat([gr[:D * d].view(D, d), gr[D * d:, None]], 1)
            else:
                e.step(u, i, j)
                got = -torch.cat([e.t["E"], e.t["Bp"][:, None]], 1) / LR
            assert e.lib.bprx_proj_mask_kind(e.h) == kind, (form, g, path)
            e.sync_check()
            e.close()
            _exact(got, c["ref"], "%s, codes 0x%02x.., %s" % (form, int(fc.CODES[g * fc.GROUP]), path))


# ---- 3. the cast, 4. the maximum ----------------------------------------------------------------------------------------
STEP_ENV = {"BPRX_LIST_MODE": "1", "BPRX_ITEM_MODE": "1", "BPRX_SIDE_STREAM": "1", "BPRX_FWD_VARIANT": "4"}


def _zero_row_batch(U, B=512):
    """triplets that name all-zero feature rows only (items 0 .. LEAD - 1, i != j): dE = dBp = 0 exactly, E and Bp keep their bits"""
    b = np.arange(B)
    return tuple(_dev(a.astype(np.int32)) for a in (b % U, b % fc.LEAD, (b + 2) % fc.LEAD))


def _probe_run(monkeypatch, dtype, D, d, F, E, Bp, want, routes, fs):
    """score_block of the one-hot items straight after bind and, per route (BPRX_DENSE_DEFER, steps), after sgd steps that leave
    [E|Bp] unchanged (the Bi of the batch's zero-row items moves: their columns are left out)."""
    for n, v in STEP_ENV.items():
        monkeypatch.setenv(n, v)
    I, U = D + fc.LEAD, d + 1
    batch = _zero_row_batch(U)
    for defer, steps in routes:
        monkeypatch.setenv("BPRX_DENSE_DEFER", str(defer))
        e = _engine(I, D, d, U, _tables(I, d, U, fc.one_hot_users(d), F, E, Bp), max_batch=512, dtype=dtype, fs=fs)
        _exact(e.score_block(0, U), want, "after bind")
        for _ in range(steps):
            e.step(*batch, want_loss=False)
        assert e.dense_pending() == bool(defer)
        got = e.score_block(0, U)
        assert not e.dense_pending()
        _exact(got[:, fc.LEAD:], want[:, fc.LEAD:], "after %d step(s), BPRX_DENSE_DEFER=%d" % (steps, defer))
        _exact(torch.cat([e.t["E"], e.t["Bp"][:, None]], 1), np.concatenate([E, Bp[:, None]], 1).astype(np.float64), "[E|Bp] after the steps")
        e.sync_check()
        e.close()


ROUTES = [(0, 1), (1, 1), (1, 2)]


@pytest.mark.parametrize("place", [None] + fc.MAX_PLACES, ids=["every-boundary"] + [p[0] for p in fc.MAX_PLACES])
def test_cast_and_maximum(monkeypatch, place):
    """score_block = torch's CPU cast of x, over 2^J, for x on every boundary between two codes and beside it."""
    D, d = 512, 15
    E, Bp, X = fc.probe_tables(fc.cast_probes(with_max=place is None), D, d, place)
    want = fc.probe_expected(fc.torch_cast(X))
    _probe_run(monkeypatch, "fp8", D, d, _f8(fc.probe_features_fp8(D)), E, Bp, want, ROUTES, fs=1.0)


# ---- 5. e4m3fn_value ----------------------------------------------------------------------------------------------------
def test_feat_explain_decodes_every_code():
    """map[p, c_t] = val(a_t) / feat_scale * w, w = E[c_t, n] + Bp[c_t] for the one-hot user n < d, Bp[c_t] for user d; every other
    column of the row is 0."""
    D, d = 512, 15
    tables, P, S = _forward(D, d)
    code, col = fc.item_codes(D)
    items = np.arange(fc.I_ITEMS)
    users = items % (d + 1)
    e = _engine(fc.I_ITEMS, D, d, d + 1, tables)
    out = e.feat_explain(users, items, top=1, maps=True)
    e.sync_check()
    e.close()
    on = code >= 0
    want = np.zeros((fc.I_ITEMS, D), dtype=np.float64)
    w = S[users, items]                                     # E is e4m3-exact at the scale: the fp32 tables and the image agree
    want[items[on], col[on]] = w[on]
    _exact(out["map"], want, "map")
    _exact(out["visual"], w, "visual")
    top = w > 0
    assert int(top.sum()) > 1000
    assert np.array_equal(out["col"].cpu().numpy()[top, 0], col[top])
    _exact(out["contrib"][_dev(top)], w[top][:, None], "contrib")


# ---- 6. the bf16 image of [E|Bp] ----------------------------------------------------------------------------------------
def test_bf16_image_rounds_to_nearest_even(monkeypatch):
    D, d = 256, 15
    E, Bp, X = fc.probe_tables(fc.bf16_probes(), D, d, scale=1.0)
    Xq = torch.from_numpy(X).to(torch.bfloat16).float().numpy()
    want = fc.probe_expected(Xq, scale=1.0)
    F = _dev(fc.probe_features_bf16(D)).to(torch.bfloat16)
    _probe_run(monkeypatch, "bf16", D, d, F, E, Bp, want, [(0, 1)], fs=1.0)
