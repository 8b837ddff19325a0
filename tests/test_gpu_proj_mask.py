"""Segment-mode steps leave the feature rows of the items their batch does not touch out of both streaming projections
(k_proj_fwd_bf16_v10<.., MASK> and k_proj_bwd_bf16_v3<.., MASK>, selected by bprx_step_begin_sparse; BPRX_PROJ_MASK=0 keeps
the unmasked passes, 1 -- the default -- masks bf16 tables, 2 fp8 tables as well).  Observed through the public entries only: step, dense_grad between step_begin / step_end, params,
score_block, and the read-only bprx_proj_mask_kind.

Shapes: D = 256 (bf16) / 512 (fp8); d = 12 (one column tile) and 64 (five); I = 3 001 and 40 003 (one and two forward tiles
per wave, partial last tile) and 32 SK + 1 / 96 SK (a second, one-row tile per split followed by empty splits / three full tiles
per split, SK as bprx_create computes it).  (One column tile is d = 12, not 15: segment mode -- and with it the mask -- needs
d % 4 == 0; d = 15 is covered as a fall-back.)

Batches are hand-built from a touched set S: every item of S occurs exactly once, half of them as positives and the others as
the negatives of the same triplets (an odd one out is both the positive and the negative of a triplet of its own: its score
difference is exactly 0, g exactly -0.5 and its two contributions cancel exactly), every user in at most two adjacent triplets.
No sum of the step then depends on an order the hardware picks (segment ranks come from LDS atomics; already two fused
multiply-adds of one item's sum differ by their order), so two handles on identical tables agree bit for bit and `torch.equal`
is the right comparison.

Touched sets: every item; no row of some whole 32-item tiles; exactly one row at positions 0 / 15 / 16 / 31 of a tile; only item
I - 1; a random half.

fp64 reference and bound of the backward product: those of tests/test_gpu_projections.py (C |F_q|^T |W| with C = 2e-5, plus 2^-23
of the value for the fp32 rounding after the sum), on its exact-W construction.
Reference: VBPR.py:83-84 (forward), VBPR.py:141 (dE, dBp)."""
import numpy as np
import pytest
import torch

import test_gpu_projections as tp

pytestmark = pytest.mark.gpu

DEV = tp.DEV
LR, REG = 0.05, 1e-3
SETS = ("all", "hole", "one", "last", "half")


def _touched(kind, I, seed):
    rs = np.random.RandomState(seed)
    if kind == "all":
        return np.arange(I)
    if kind == "hole":                                      # tiles 1 and 2 and the last whole tile: no row touched
        keep = np.ones(I, bool)
        keep[32:96] = False
        last = (I // 32 - 1) * 32
        keep[last:last + 32] = False
        return np.nonzero(keep)[0]
    if kind == "one":                                       # one row each at positions 0, 15, 16, 31 of four different tiles
        return np.array([0, 32 + 15, 64 + 16, (I // 32 - 1) * 32 + 31])
    if kind == "last":
        return np.array([I - 1])
    return np.sort(rs.permutation(I)[:I // 2])              # "half"


def _batch(S, seed):
    """(u, i, j) on the device: every item of S in exactly one triplet (see the module docstring), users in adjacent pairs."""
    rs = np.random.RandomState(seed)
    P = S[rs.permutation(len(S))]
    h = len(P) // 2
    i, j = P[:h], P[h:2 * h]
    if len(P) % 2:
        i, j = np.append(i, P[-1]), np.append(j, P[-1])
    u = np.arange(len(i)) // 2
    return tuple(torch.as_tensor(a.astype(np.int32), device=DEV) for a in (u, i, j))


def _tables(I, D, d, U, F, seed):
    g = tp._gen(seed)
    r = lambda *s: (torch.rand(s, generator=g, device=DEV) - 0.5) * 0.2
    return dict(Gu=r(U, 4), Gi=r(I, 4), Bi=r(I), Tu=r(U, d), F=F, E=r(D, d), Bp=r(D))


def _clone(t):
    return {n: (v if n == "F" else v.clone()) for n, v in t.items()}


def _engine(monkeypatch, mask, I, D, d, dtype, U, tables, B, optimizer="sgd", list_mode="0", item_mode="2"):
    from fashionvisualexpl_recommend_amd.engine import Engine
    monkeypatch.delenv("BPRX_FWD_VARIANT", raising=False)
    monkeypatch.setenv("BPRX_ITEM_MODE", item_mode)
    monkeypatch.setenv("BPRX_LIST_MODE", list_mode)
    # 1 (the default) masks bf16 tables of up to nine column tiles; the fp8 forms are reached with 2
    monkeypatch.setenv("BPRX_PROJ_MASK", ("2" if dtype == "fp8" else "1") if mask else "0")
    return Engine(model="vbpr", num_users=U, num_items=I, embed_k=4, embed_d=d, feat_dim=D, feat_dtype=dtype, optimizer=optimizer,
                  lr=LR, reg=REG, max_batch=B, feat_scale=tp.FEAT_SCALE).bind(**_clone(tables))


def _kind(e):
    return e.lib.bprx_proj_mask_kind(e.h)


def _step(e, b):
    """One step; returns the dense gradient read between step_begin and step_end."""
    e.step_begin(*b)
    g = e.dense_grad().clone()
    e.step_end()
    return g


def _same(a, b, what):
    assert torch.equal(a + 0.0, b + 0.0), "%s: %d of %d values differ, max |diff| %.3g" % (
        what, int((a != b).sum()), a.numel(), float((a.double() - b.double()).abs().max()))


def _same_tables(ea, eb, what):
    for n, v in ea.params().items():
        _same(v, eb.params()[n], "%s %s" % (what, n))


def _shapes():
    c = []
    for dtype, D in (("bf16", 256), ("fp8", 512)):
        for d in (12, 64):
            for I in (3_001, 40_003, "t2", "t3"):
                c.append(pytest.param(dtype, D, d, I, id="%s-d%d-I%s" % (dtype, d, I)))
    return c


def _items(I, D, d, dtype):
    if isinstance(I, str):
        SK = tp._sk(D, (d + 1 + 15) // 16, dtype == "fp8")
        return {"t2": 32 * SK + 1, "t3": 96 * SK}[I]
    return I


@pytest.mark.parametrize("dtype,D,d,I", _shapes())
def test_masked_step_equals_unmasked(monkeypatch, dtype, D, d, I):
    I = _items(I, D, d, dtype)
    F, _ = tp._features(I, D, dtype, seed=d)
    U = I // 2 + 1
    t = _tables(I, D, d, U, F, seed=I % 97 + d)
    for s, kind in enumerate(SETS):
        b = _batch(_touched(kind, I, seed=s), seed=10 + s)
        em = _engine(monkeypatch, True, I, D, d, dtype, U, t, I)
        eu = _engine(monkeypatch, False, I, D, d, dtype, U, t, I)
        gm, gu = _step(em, b), _step(eu, b)
        assert _kind(em) == 1 and _kind(eu) == 0, (kind, _kind(em), _kind(eu))
        _same(gm, gu, "dE|dBp, touched set '%s'" % kind)
        _same_tables(em, eu, "touched set '%s'" % kind)
        em.sync_check(); eu.sync_check()
        em.close(); eu.close()


@pytest.mark.parametrize("optimizer", ["sgd", "adam_tf23"])
def test_four_steps_with_changing_touched_sets(monkeypatch, optimizer):
    """Stale masks, stale W rows, and (adam_tf23) the side-stream catch-up beside the reordered index pass."""
    I, D, d, dtype = 3_001, 256, 64, "bf16"
    F, _ = tp._features(I, D, dtype, seed=1)
    U = I // 2 + 1
    t = _tables(I, D, d, U, F, seed=5)
    em = _engine(monkeypatch, True, I, D, d, dtype, U, t, I, optimizer)
    eu = _engine(monkeypatch, False, I, D, d, dtype, U, t, I, optimizer)
    for s, kind in enumerate(("half", "hole", "one", "all")):
        b = _batch(_touched(kind, I, seed=20 + s), seed=30 + s)
        gm, gu = _step(em, b), _step(eu, b)
        assert _kind(em) == 1 and _kind(eu) == 0, (s, kind)
        _same(gm, gu, "step %d dE|dBp" % s)
        _same_tables(em, eu, "step %d" % s)
    em.sync_check(); eu.sync_check()
    em.close(); eu.close()


@pytest.mark.parametrize("dtype,D,d,I", [pytest.param("bf16", 256, 64, "t2", id="bf16-t2"), pytest.param("bf16", 256, 12, "t3", id="bf16-t3"),
                                         pytest.param("fp8", 512, 64, "t3", id="fp8-t3"), pytest.param("bf16", 256, 64, 40_003, id="bf16-40003")])
def test_masked_backward_against_fp64(monkeypatch, dtype, D, d, I):
    """dE|dBp of a masked step against F_q^T W in float64: the construction, reference and bound of test_gpu_projections._backward
    (zero E / Bp / Gu / Gi / Bi: g = -0.5 exactly, W exact in fp32 and bf16), on a random half of the items."""
    I = _items(I, D, d, dtype)
    F, Fq = tp._features(I, D, dtype, seed=3)
    S = _touched("half", I, seed=I % 13)
    ud, id_, jd = _batch(S, seed=4)
    U = int(ud.max()) + 1
    rs = np.random.RandomState(17)
    Tu = torch.as_tensor(rs.randint(-4, 5, size=(U, d)).astype(np.float32) / 8.0, device=DEV)
    row = torch.cat([Tu, torch.ones((U, 1), device=DEV)], 1).double()[ud.long()] * 0.5
    W = torch.zeros((I, d + 1), dtype=torch.float64, device=DEV)
    W.index_add_(0, id_.long(), -row)
    W.index_add_(0, jd.long(), row)
    assert torch.equal(W.float().to(torch.bfloat16).double(), W)
    gs = float(np.float32(1.0) / np.float32(tp.FEAT_SCALE)) if dtype == "fp8" else 1.0
    ref, A = (Fq.T @ W) * gs, (Fq.abs().T @ W.abs()) * gs
    bnd = tp.C_MFMA * A + 2.0 ** -23 * ref.abs()
    z = lambda *s: torch.zeros(s, device=DEV)
    t = dict(Gu=z(U, 4), Gi=z(I, 4), Bi=z(I), Tu=Tu, F=F, E=z(D, d), Bp=z(D))
    e = _engine(monkeypatch, True, I, D, d, dtype, U, t, len(S))
    g = _step(e, (ud, id_, jd))
    assert _kind(e) == 1
    e.sync_check()
    e.close()
    got = torch.cat([g[:D * d].view(D, d), g[D * d:, None]], 1)
    err = (got.double() - ref).abs()
    r = float((err / bnd.clamp_min(1e-300)).max())
    print("masked dE|dBp: worst error %.3g x bound, %d nonzero values" % (r, int((ref != 0).sum())))
    assert bool((err <= bnd).all()), "worst %.3g x bound" % r
    assert int((ref != 0).sum()) > ref.numel() // 2


def test_untouched_rows_are_out_of_the_sums(monkeypatch):
    """+inf in every feature row the batch does not touch: the masked step gives what it gives on the clean table."""
    I, D, d, dtype = 3_001, 256, 64, "bf16"
    F, _ = tp._features(I, D, dtype, seed=2)
    U = I // 2 + 1
    for s, kind in enumerate(("half", "hole", "one", "last")):
        S = _touched(kind, I, seed=40 + s)
        b = _batch(S, seed=50 + s)
        Finf = F.clone()
        out = torch.ones(I, dtype=torch.bool, device=DEV)
        out[torch.as_tensor(S, device=DEV)] = False
        Finf[out] = float("inf")
        t = _tables(I, D, d, U, F, seed=6)
        ti = dict(t, F=Finf)
        ec = _engine(monkeypatch, True, I, D, d, dtype, U, t, I)
        ei = _engine(monkeypatch, True, I, D, d, dtype, U, ti, I)
        gc, gi = _step(ec, b), _step(ei, b)
        assert _kind(ec) == 1 and _kind(ei) == 1
        assert bool(torch.isfinite(gi).all()), kind
        _same(gi, gc, "dE|dBp with +inf in the untouched rows ('%s')" % kind)
        for n, v in ec.params().items():
            if n != "F":
                _same(ei.params()[n], v, "'%s' %s" % (kind, n))
        ec.close(); ei.close()


def test_nothing_stale_is_served_after_a_masked_step(monkeypatch):
    """P holds zeros in the untouched rows after a masked step: score_block must re-project every item."""
    I, D, d, dtype = 3_001, 256, 64, "bf16"
    F, _ = tp._features(I, D, dtype, seed=2)
    U = 64
    t = _tables(I, D, d, U, F, seed=8)
    S = _touched("one", I, seed=0)
    u, i, j = _batch(S, seed=1)
    e = _engine(monkeypatch, True, I, D, d, dtype, U, t, 16)
    e.score_block(0, U)                                     # the projection cache is valid before the step ...
    e.step(u, i, j)
    assert _kind(e) == 0                                    # ... so this step has nothing to project (and nothing to mask)
    e.step(u, i, j)
    assert _kind(e) == 1
    got = e.score_block(0, U).clone()
    fresh = _engine(monkeypatch, True, I, D, d, dtype, U, dict(e.params(), F=F), 16)
    want = fresh.score_block(0, U)
    _same(got, want, "score_block after a masked step")
    assert float(want.abs().max()) > 0
    e.close(); fresh.close()


@pytest.mark.parametrize("case", ["list", "project", "fp32", "d15", "fp8"])
def test_fallbacks_take_no_mask(monkeypatch, case):
    I, D = 3_001, 256
    d = 15 if case == "d15" else 64
    dtype = "fp32" if case == "fp32" else ("fp8" if case == "fp8" else "bf16")
    if case == "fp8":
        D = 512
    F, _ = tp._features(I, D, dtype, seed=4)
    U = I // 2 + 1
    t = _tables(I, D, d, U, F, seed=9)
    b = _batch(_touched("half", I, seed=1), seed=2)
    lm = "2" if case == "list" else "0"
    ea = _engine(monkeypatch, True, I, D, d, dtype, U, t, I, list_mode=lm)
    if case == "fp8":                                       # the default setting leaves fp8 tables unmasked (measured slower)
        ea.close()
        monkeypatch.setenv("BPRX_PROJ_MASK", "1")
        from fashionvisualexpl_recommend_amd.engine import Engine
        ea = Engine(model="vbpr", num_users=U, num_items=I, embed_k=4, embed_d=d, feat_dim=D, feat_dtype=dtype, optimizer="sgd",
                    lr=LR, reg=REG, max_batch=I, feat_scale=tp.FEAT_SCALE).bind(**_clone(t))
    eb = _engine(monkeypatch, False, I, D, d, dtype, U, t, I, list_mode=lm)
    if case == "project":
        ea.step_project(); eb.step_project()
    ga, gb = _step(ea, b), _step(eb, b)
    assert _kind(ea) == 0 and _kind(eb) == 0, case
    if case in ("list", "d15"):
        # the touched-item list is filled, and the atomic staging path sums, in arrival order: two runs of the SAME code agree to
        # summation order only.  fp32 sums of n <= I + 1 terms: |diff| <= 2 n 2^-24 sum |terms| <= 2e-4 sum |terms|, and the sum of
        # |terms| of any dE|dBp value is at most max|W| sum_t |F[t, k]| <= 1.0 * I here (|F| < 1, |W row| <= 2 * 0.5 * max(|Tu|, 1)).
        assert float((ga.double() - gb.double()).abs().max()) <= 2e-4 * I
        for n, v in ea.params().items():
            torch.testing.assert_close(v.float(), eb.params()[n].float(), rtol=1e-4, atol=1e-4 * LR * I)
    else:
        _same(ga, gb, "dE|dBp (%s)" % case)
        _same_tables(ea, eb, case)
    ea.sync_check(); eb.sync_check()
    ea.close(); eb.close()
