"""The streaming forward projections keep a chunk's feature loads in flight across the chunk loop's barrier (the [E|Bp]^T
pieces are requested BEFORE the feature pieces, so the wait that parks them leaves the feature loads outstanding; DESIGN.md
6.4).  The arithmetic did not move, so every case asks for BIT equality (`torch.equal`) with the plain kernel k_proj_fwd_bf16
of a second engine created under BPRX_FWD_VARIANT=0.

P = F.[E|Bp] is observed as test_gpu_variants.py does: one-hot visual users 0..d-1 and a zero user d (Gu = 0 for them), so
score_block(0, d + 1) is fl(P[i,u] + P[i,d] + Bi[i]) / fl(P[i,d] + Bi[i]) -- a function of P and of tables both engines share.
Each case runs twice: on freshly bound tables (the image of [E|Bp]^T is the one the cast kernel writes), and after ONE sgd step
of the streaming engine (bf16: the image k_dense_update wrote; fp8: the cast with the max |E,Bp| that k_dense_update left).
The batch uses users d+1.. only, so the one-hot rows stay one-hot; the plain engine is then bound to copies of the stepped
tables.

Shapes, the smallest at which a two-stage pipeline goes wrong:
  feature width   bf16 256 (two chunks: the loop body runs once, its last prefetch is the clamped re-read), 512 and 768 (two
                  and three trips: the register sets rotate, nch/2 odd and even); fp8 512 and 1024 (the same chunk counts for
                  v10; four and eight chunks for k_proj_fwd_f8s)
  rows            1, 17, 33 (one tile per wave; waves and workgroups without work); 128 N + 1 and 128 N + 17 with N the CU
                  count: more than 8 N row tiles, an odd and an even number of them, so that one launch holds waves with
                  two, one and no live tiles (32 769 / 32 785 rows on a 256-CU part, 17 MB at D = 256)
  d               15 (one column tile), 64 (five), 143 (nine); 150 bf16 (column-range passes of v10<9>); 256 fp8
                  (k_proj_fwd_f8s), and 4 097 pairs through score_pairs on a fresh handle for its row-list form

k_proj_fwd_f8s sums 128 products per instruction in another order than the plain kernel (test_gpu_variants.py allows it 2e-6
of max |P|).  Its cases therefore use inputs whose sums are EXACT in fp32 in any order, which makes bit equality the right bar
for them too: feature codes in {0, 1, 2, 3}, [E|Bp] in 2^-4 {0, +-1, +-1/2, +-1/4} with the maximum present (e4m3 codes 448 /
224 / 112 under the scale 448 / 2^-4 = 7168, a power of two) -- every product is a multiple of 16 and |sum| <= 1024 * 3 * 448
< 2^21, so every partial sum is a multiple of 16 below 2^24 * 16.  Their sgd step uses lr = 2^-20: the update moves a value by
less than 2^-20 * 0.1 (|dE| <= 16 triplets * max f (3 / 448) * |g Tu| <= 0.5), i.e. by less than 2^-10 code units for a zero
and 1e-5 relative otherwise against a half-spacing of 3.5 % -- the codes stay on the grid, the scale is the stepped one.

The masked form (segment-mode steps) is reached through whole steps only: batches built as in
test_gpu_proj_mask.py (no sum depends on an order the hardware picks) that leave rows 0, 15, 16 and the last row untouched, two
steps in a row on a masked streaming engine, an unmasked streaming engine and an engine on the plain kernel.  P is read
between step_begin and step_end through bprx_item_proj (Engine.item_proj): the touched rows bit-equal on all three, the
untouched rows exactly 0 on the masked engine (and not 0 on the unmasked one); then dE|dBp and every table after the step
bit-equal.
Reference: VBPR.py:83-84 (f_i.E and f_i.Bp)."""
import ctypes as C

import numpy as np
import pytest
import torch

import test_gpu_proj_mask as tm
import test_gpu_projections as tp
from fashionvisualexpl_recommend_amd import _ffi

pytestmark = pytest.mark.gpu

DEV = tp.DEV
NB = 8                    # batch users d+1 .. d+NB, two triplets each


def _rows(tag):
    n = tp._ncu()
    return {"r1": 1, "r17": 17, "r33": 33, "odd": 128 * n + 1, "even": 128 * n + 17}[tag]


def _tables(I, D, d, dtype, exact, seed):
    g = tp._gen(seed)
    U = d + 1 + NB
    ri = lambda lo, hi, *s: torch.randint(lo, hi, s, generator=g, device=DEV)
    if exact:                                              # (module docstring: sums exact in any order)
        F = (ri(0, 4, I, D) * (ri(0, 2, I, D))).float().to(torch.float8_e4m3fn)
        grid = torch.tensor([0.0, 1.0, -1.0, 0.5, -0.5, 0.25, -0.25], device=DEV) * 2.0 ** -4
        E, Bp = grid[ri(0, 7, D, d)], grid[ri(0, 7, D)]
        E[0, 0] = 2.0 ** -4
    else:
        F = torch.rand((I, D), generator=g, device=DEV) * (torch.rand((I, D), generator=g, device=DEV) < 0.5)
        F = (F * tp.FEAT_SCALE).to(torch.float8_e4m3fn) if dtype == "fp8" else F.to(torch.bfloat16)
        E = (torch.rand((D, d), generator=g, device=DEV) - 0.5) * 0.1
        Bp = (torch.rand(D, generator=g, device=DEV) - 0.5) * 0.1
    Tu = torch.zeros((U, d), device=DEV)
    Tu[torch.arange(d), torch.arange(d)] = 1.0
    Tu[d + 1:] = ri(-4, 5, NB, d).float() / 8.0
    Gu = torch.zeros((U, 4), device=DEV)
    Gu[d + 1:] = ri(-4, 5, NB, 4).float() / 8.0
    return dict(Gu=Gu, Gi=ri(-4, 5, I, 4).float() / 8.0, Bi=torch.zeros(I, device=DEV), Tu=Tu, F=F, E=E, Bp=Bp)


def _engine(monkeypatch, plain, I, D, d, dtype, t, lr, max_batch=2 * NB):
    from fashionvisualexpl_recommend_amd.engine import Engine
    if plain:
        monkeypatch.setenv("BPRX_FWD_VARIANT", "0")
    else:
        monkeypatch.delenv("BPRX_FWD_VARIANT", raising=False)
    tt = {n: (v if n == "F" else v.clone()) for n, v in t.items()}
    return Engine(model="vbpr", num_users=d + 1 + NB, num_items=I, embed_k=4, embed_d=d, feat_dim=D, feat_dtype=dtype,
                  optimizer="sgd", lr=lr, reg=0.0, max_batch=max_batch, feat_scale=tp.FEAT_SCALE).bind(**tt)


def _batch(I, d, seed):
    rs = np.random.RandomState(seed)
    u = d + 1 + np.arange(2 * NB) // 2
    i = rs.randint(0, I, size=2 * NB)
    j = (i + 1 + rs.randint(0, max(I - 1, 1), size=2 * NB)) % I        # j != i wherever the table has two items
    return tuple(torch.as_tensor(a.astype(np.int32), device=DEV) for a in (u, i, j))


def _equal(got, want, what):
    assert torch.equal(got, want), "%s: %d of %d scores differ, max |diff| %.3g" % (
        what, int((got != want).sum()), got.numel(), float((got.double() - want.double()).abs().max()))
    assert float(want.abs().max()) > 0, what


def _run(monkeypatch, I, D, d, dtype, exact=False, seed=0):
    lr = 2.0 ** -20 if exact else 0.05
    t = _tables(I, D, d, dtype, exact, seed)
    es = _engine(monkeypatch, False, I, D, d, dtype, t, lr)
    ep = _engine(monkeypatch, True, I, D, d, dtype, t, lr)
    _equal(es.score_block(0, d + 1), ep.score_block(0, d + 1), "tables as bound")
    ep.close()
    es.step(*_batch(I, d, seed + 1))
    got = es.score_block(0, d + 1)
    stepped = dict(es.params(), F=t["F"])
    assert I == 1 or not torch.equal(stepped["E"], t["E"])   # the step moved E (one item: i = j, the two contributions cancel)
    ep = _engine(monkeypatch, True, I, D, d, dtype, stepped, lr)
    _equal(got, ep.score_block(0, d + 1), "after one sgd step")
    es.sync_check(); ep.sync_check()
    es.close(); ep.close()


WIDTHS = [("bf16", 256), ("bf16", 512), ("bf16", 768), ("fp8", 512), ("fp8", 1024)]
ROWS = ["r1", "r17", "r33", "odd", "even"]


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("d", [15, 64, 143])
@pytest.mark.parametrize("dtype,D", WIDTHS)
def test_v10_matches_the_plain_kernel(monkeypatch, dtype, D, d, rows):
    """k_proj_fwd_bf16_v10<1 / 5 / 9 tiles>, bf16 (`nt` loads) and fp8 (default-policy loads), one and two tiles per wave."""
    _run(monkeypatch, _rows(rows), D, d, dtype, seed=D + d)


@pytest.mark.parametrize("rows", ["r17", "odd", "even"])
@pytest.mark.parametrize("D", [256, 512, 768])
def test_column_range_passes_match_the_plain_kernel(monkeypatch, D, rows):
    """d = 150, bf16: ten column tiles in two right-aligned passes of v10<9>."""
    _run(monkeypatch, _rows(rows), D, 150, "bf16", seed=D)


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("D", [512, 1024])
def test_wide_fp8_forward_matches_the_plain_kernel(monkeypatch, D, rows):
    """d = 256, fp8: k_proj_fwd_f8s<17>, on inputs whose sums are exact in any order (module docstring)."""
    _run(monkeypatch, _rows(rows), D, 256, "fp8", exact=True, seed=D)


@pytest.mark.parametrize("D", [512, 1024])
def test_wide_fp8_row_list_matches_the_plain_kernel(monkeypatch, D):
    """4 097 pairs through score_pairs on a handle without valid projections: k_proj_fwd_f8s over the row list (257 row tiles,
    the last of one row), against the plain kernel's whole-table scores at the same (user, item) positions -- with one-hot and
    zero user rows both score kernels return fl(P[i,u] + P[i,d]) whatever their own order."""
    I, d, n = 3_001, 256, 4_097
    t = _tables(I, D, d, "fp8", True, seed=D + 1)
    rs = np.random.RandomState(D)
    items = rs.randint(0, I, size=n)
    items[0], items[n // 2], items[-1] = I - 1, 0, I - 1
    users = rs.randint(0, d + 1, size=n)
    ep = _engine(monkeypatch, True, I, D, d, "fp8", t, 2.0 ** -20)
    want = ep.score_block(0, d + 1)[torch.as_tensor(users, device=DEV), torch.as_tensor(items, device=DEV)]
    ep.close()
    es = _engine(monkeypatch, False, I, D, d, "fp8", t, 2.0 ** -20, max_batch=n)
    got = es.score_pairs(users, items)
    es.sync_check()
    es.close()
    _equal(got + 0.0, want + 0.0, "score_pairs over 4 097 rows")


@pytest.mark.parametrize("rows", ["I3001", "odd"])
@pytest.mark.parametrize("D", [256, 512])
def test_masked_forward_through_two_steps(monkeypatch, D, rows):
    """Segment-mode steps whose batch leaves rows 0, 15, 16 and the last row untouched (module docstring)."""
    I = 3_001 if rows == "I3001" else _rows(rows)
    d, dtype = 64, "bf16"
    F, _ = tp._features(I, D, dtype, seed=D % 7)
    U = I // 2 + 1
    t = tm._tables(I, D, d, U, F, seed=D % 97)
    keep = np.ones(I, bool)
    keep[[0, 15, 16, I - 1]] = False
    S = np.nonzero(keep)[0]
    em = tm._engine(monkeypatch, True, I, D, d, dtype, U, t, I)
    eu = tm._engine(monkeypatch, False, I, D, d, dtype, U, t, I)
    monkeypatch.setenv("BPRX_FWD_VARIANT", "0")              # (tm._engine clears it; the handle reads it at create)
    from fashionvisualexpl_recommend_amd.engine import Engine
    ep = Engine(model="vbpr", num_users=U, num_items=I, embed_k=4, embed_d=d, feat_dim=D, feat_dtype=dtype, optimizer="sgd",
                lr=tm.LR, reg=tm.REG, max_batch=I, feat_scale=tp.FEAT_SCALE).bind(**tm._clone(t))
    out = torch.as_tensor([0, 15, 16, I - 1], device=DEV)
    Sd = torch.as_tensor(S, device=DEV)
    for s in range(2):                                       # step 0: the cast kernel's image; step 1: k_dense_update's
        b = tm._batch(S, seed=60 + s)
        g, P = [], []
        for e in (em, eu, ep):                               # P as the step's forward projection left it, dE|dBp, then the update
            e.step_begin(*b)
            P.append(e.item_proj().clone())
            g.append(e.dense_grad().clone())
            e.step_end()
        assert tm._kind(em) == 1 and tm._kind(eu) == 0 and tm._kind(ep) == 0, (s, tm._kind(em), tm._kind(eu), tm._kind(ep))
        tm._same(P[0][Sd], P[1][Sd], "step %d P of the touched rows, masked against unmasked" % s)
        tm._same(P[0][Sd], P[2][Sd], "step %d P of the touched rows, masked against the plain kernel" % s)
        tm._same(P[1], P[2], "step %d P, unmasked against the plain kernel" % s)
        assert not bool(P[0][out].any()), "step %d: P of the untouched rows is not 0: %r" % (s, P[0][out].abs().max(1).values.tolist())
        assert bool((P[1][out, :d + 1] != 0).any(1).all())   # (the unmasked pass does project those rows)
        tm._same(g[0], g[1], "step %d dE|dBp, masked against unmasked" % s)
        tm._same(g[0], g[2], "step %d dE|dBp, masked against the plain kernel" % s)
        tm._same_tables(em, eu, "step %d, unmasked" % s)
        tm._same_tables(em, ep, "step %d, plain kernel" % s)
    for e in (em, eu, ep):
        e.sync_check()
        e.close()


def test_stream_probe_with_the_launch_shape_as_arguments():
    """bprx_probe_stream_read_nt_shape: the byte count (whole loop trips) for valid shapes, a negative code for invalid ones; one
    launch on a 64-MB buffer per valid shape."""
    L = _ffi.lib()
    nbytes = 64 << 20
    buf = torch.ones(nbytes // 4, dtype=torch.float32, device=DEV)
    sink = torch.zeros(4096, dtype=torch.float32, device=DEV)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda b, n, wg, thr, u, sk: L.bprx_probe_stream_read_nt_shape(C.c_void_p(b), n, wg, thr, u, C.c_void_p(sk), st)
    bp, sp = buf.data_ptr(), sink.data_ptr()
    for wg, thr, u in ((256, 1024, 1), (256, 1024, 16), (512, 512, 3), (1, 64, 12), (511, 960, 6)):
        trip = thr * u * 16
        assert call(bp, nbytes, wg, thr, u, sp) == nbytes // wg // trip * trip * wg, (wg, thr, u)
    for bad in ((0, 1024, 8), (513, 1024, 8), (256, 0, 8), (256, 1000, 8), (256, 2048, 8), (256, 1024, 0), (256, 1024, 5),
                (256, 1024, 32)):
        assert call(bp, nbytes, *bad, sp) < 0, bad
    assert call(0, nbytes, 256, 1024, 8, sp) < 0 and call(bp, nbytes, 256, 1024, 8, 0) < 0
    assert call(bp, 0, 256, 1024, 8, sp) < 0 and call(bp, 256 * 1024 * 8 * 16 - 16, 256, 1024, 8, sp) < 0     # not one trip each
    assert call(bp, 256 * 1024 * 8 * 16, 256, 1024, 8, sp) == 256 * 1024 * 8 * 16
    torch.cuda.synchronize()
    assert float(sink.abs().max()) == 0.0                    # nothing but the guarded store ever writes the sink
