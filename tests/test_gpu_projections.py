"""Every kernel form the projection launchers of bprx_proj.hip can pick, against a float64 reference of the same operation on
the same quantised operands (torch float64 on the device; the library is never asked for a reference).

  forward   P = F.[E|Bp]   (bprx_launch_proj_fwd)          backward   dE|dBp = F^T.W   (bprx_launch_proj_bwd)

case (test :: parameter)                      launcher -> instantiation reached (NT = PS/16 column tiles, N = CU count)
--------------------------------------------  ----------------------------------------------------------------------------------
fwd_table::v10 bf16 D 256 / fp8 D 512, NT 1-9  launch_fwd_nt -> launch_v10<NT> -> k_proj_fwd_bf16_v10<NT, F8, NTL=bf16>
                                               (I = 40 003: two tiles per wave; 3 001: one; 7: a single partial tile)
fwd_table::plain (BPRX_FWD_VARIANT=0)          launch_fwd_nt -> k_proj_fwd_bf16<NT, MTD = NT <= 9 ? 2 : 1, F8>
fwd_table::odd D (bf16 384, fp8 768)           the same plain kernel, chosen by Deq % 256 != 0
fwd_table::f8s fp8 D 512, NT 10/11/13/16/17    launch_f8s<NT> -> k_proj_fwd_f8s<NT, false>
fwd_table::passes bf16 NT 10 / 17              launch_v10<9> passes: columns 0-8 + 1-9 (overlap 8), 0-8 + 8-16
test_forward_streaming_loads_beyond_the_cache  300 000 x 1 024 fp8 (> 256 MiB): k_proj_fwd_bf16_v10<4, true, NTL=true>
fwd_rows::split                                launch_fwd_rows: tiles*NT <= 2N -> k_proj_fwd_rows<1, 1, 16, F8> (K split)
fwd_rows::mt1 / mt2 / mt4                      k_proj_fwd_rows<NT, 1|2|4, 8, F8>; MT 2 above 2N row tiles, MT 4 above 8N (NT <= 5)
fwd_rows::f8s_rows fp8 NT 10 / 17              4 095 rows: k_proj_fwd_rows<NT, 1, 8, true>; 4 096: k_proj_fwd_f8s<NT> over the list
fwd_table / fwd_rows ::fp32                    k_proj_fwd_f32_mfma (D % 16 == 0), k_proj_fwd_f32 (D = 100)
bwd::pd3 bf16 D 256, NT 1-9                    launch_bwd_nt -> k_proj_bwd_bf16_v3<NT, 32, 8, PD 3, bf16, DB 1>
bwd::db2 fp8 D 512, NT 1-9                     k_proj_bwd_bf16_v3<NT, 32, 8, 2, fp8, DB 2>
bwd::ns2 bf16 D 256 / fp8 D 512, NT 10-17      k_proj_bwd_bf16_v3<NT, 32, 8, 2, F8, DB 2, NS 2>
bwd::w4 bf16 D 128 / 384                       k_proj_bwd_bf16_v3<NT, 32, 4, 2, bf16, DB 1> (NS 1 at every NT)
bwd::grid (SK % 8 != 0: D 1280 at 256 CUs)     v3 with the XCD remap off
bwd::rows (BPRX_LIST_MODE=2)                   launch_bwd_rows -> k_proj_bwd_bf16_v3<NT, 32, 8|4, 2, F8, ROWS>
bwd::fp32                                      k_proj_bwd_f32 (whole table; list mode with D % 8 != 0), k_proj_bwd_f32_tile (list)

Per-split tile counts (backward, whole table): SK item splits of rps = roundup32(ceil(I / SK)) items; the cases "t1" .. "many"
choose I from SK so that a split holds 1, 2, 3, 4 or 25 tiles of 32 items, with I % 32 in {31, 1, 0, 1, 25}, the last split
partial ("t1", "t4", "many"), followed by empty ones ("t2", "many") or exactly full ("t3").

Observation (no new entry point):
  * forward, whole table: one-hot visual users (Tu[u, u] = 1, Gu = Bi = 0): score_block(0, d+1)[u, i] = P[i,u] + P[i,d]
    (u < d), P[i,d] (u = d).  Forward over a row list: score_pairs on a freshly bound handle (the projection cache is invalid:
    every call projects the listed rows).
  * backward: Gu = Gi = Bi = 0 and E = Bp = 0 make every score 0, so g = -1/(1+exp(0)) = -0.5 exactly and
    W[t] = sum of -+0.5 [Tu[u] | 1] over the occurrences of t.  Tu = m/8 with small integers m keeps every partial sum exact in
    fp32 and W exact in bf16 (asserted).  dE|dBp is read twice: dense_grad() between step_begin / step_end (k_reduce_parts)
    and -E_new / lr after one sgd step with reg = 0 (k_dense_update's fused slab sum; lr is a power of two).

Bounds: bf16 and fp8 MFMA paths |got - ref| <= C (|F_q|.|[E|Bp]_q|) (forward) or C (|F_q|^T.|W|) (backward), C = 2e-5, plus
the fp32 roundings after the sum (the fp8 rescale, the score's one fp32 add): 2^-22 of the value.  fp32 features (fp64
accumulation): one fp32 ulp per stored value (plus the score add), plus 2^-40 of the absolute sum for the fp64 rounding
of kernel and reference.  Losing or doubling a 16- or 32-row tile, a 128-wide k-chunk or shifting a column tile moves a
value by a sizeable fraction of its absolute sum, far outside either bound.
Reference: VBPR.py:83-84 (forward), VBPR.py:141 (dE, dBp)."""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
C_MFMA = 2e-5
LR = 0.5                      # power of two: -E_new / LR is the summed gradient bit for bit
FEAT_SCALE = 448.0


def _ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _sk(D, NT, fp8):
    """Item splits of the whole-table backward (bprx_create): one 8-wave workgroup per CU over D/256 column ranges,
    doubled for fp8 at <= 9 column tiles, at most 64."""
    mr = (D + 255) // 256
    sk = (_ncu() + mr - 1) // mr
    if fp8 and NT <= 9:
        sk *= 2
    return max(1, min(sk, 64))


def _items_for(tiles, SK):
    """I with `tiles` 32-item tiles per split (see the module docstring)."""
    return {"t1": 32 * SK - 1, "t2": 32 * SK + 1, "t3": 96 * SK, "t4": 128 * SK - 31, "many": 800 * SK - 7}[tiles]


def _gen(seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return g


@functools.lru_cache(maxsize=2)
def _features(I, D, dtype, seed):
    """F as bound (bf16 / e4m3fn codes of f * 448 / fp32) and its values in float64 (fp8: the code values)."""
    g = _gen(seed)
    F = torch.rand((I, D), generator=g, device=DEV) * (torch.rand((I, D), generator=g, device=DEV) < 0.5)
    if dtype == "fp8":
        F = (F * FEAT_SCALE).to(torch.float8_e4m3fn)
    elif dtype == "bf16":
        F = F.to(torch.bfloat16)
    return F, F.double()


def _ulp(x):
    """fp32 spacing at |x| (x float64)."""
    _, e = torch.frexp(x.float().abs())
    return torch.ldexp(torch.ones_like(x), (e - 24).to(torch.int64)).clamp_min(2.0 ** -149)


def _engine(I, D, d, dtype, U, tables, max_batch=16):
    from fashionvisualexpl_recommend_amd.engine import Engine
    return Engine(model="vbpr", num_users=U, num_items=I, embed_k=4, embed_d=d, feat_dim=D, feat_dtype=dtype,
                  optimizer="sgd", lr=LR, reg=0.0, max_batch=max_batch, feat_scale=FEAT_SCALE).bind(**tables)


# ---- forward --------------------------------------------------------------------------------------------------------
def _forward_setup(I, D, d, dtype, seed):
    """Tables with one-hot visual users and the float64 reference P, |F_q|.|[E|Bp]_q| on the kernel's operands."""
    F, Fq = _features(I, D, dtype, seed)
    g = _gen(seed + 1000 * d + 1)
    E = (torch.rand((D, d), generator=g, device=DEV) - 0.5) * 0.1
    Bp = (torch.rand(D, generator=g, device=DEV) - 0.5) * 0.1
    EB = torch.cat([E, Bp[:, None]], 1)
    scale = 1.0
    if dtype == "bf16":
        Eq = EB.to(torch.bfloat16).double()
    elif dtype == "fp8":                                   # k_absmax + k_cast_Et8, restated in fp32
        EBn = EB.cpu().numpy()
        sE = np.float32(448.0) / np.float32(np.abs(EBn).max())
        Eq = torch.from_numpy(orc.e4m3_round((EBn * sE).astype(np.float32))).double().to(DEV)
        scale = float(np.float32(1.0) / (np.float32(FEAT_SCALE) * sE))     # qs[1]
    else:
        Eq = EB.double()
    P = (Fq @ Eq) * scale
    A = (Fq.abs() @ Eq.abs()) * scale
    U = d + 1
    Tu = torch.zeros((U, d), device=DEV)
    Tu[torch.arange(d), torch.arange(d)] = 1.0
    tables = dict(Gu=torch.zeros((U, 4), device=DEV), Gi=torch.zeros((I, 4), device=DEV), Bi=torch.zeros(I, device=DEV),
                  Tu=Tu, F=F, E=E, Bp=Bp)
    return tables, P, A


def _check_scores(got, pu, au, pd, ad, fp32, what):
    """got = fl(P[i,u] + P[i,d]) (pu = au = 0 for u = d) against the float64 reference."""
    want = pu + pd
    err = (got.double() - want).abs()
    if fp32:
        bnd = _ulp(pu) * (pu != 0) + _ulp(pd) + _ulp(want) + 2.0 ** -40 * (au + ad)
    else:
        bnd = C_MFMA * (au + ad) + 2.0 ** -22 * (pu.abs() + pd.abs())
    bad = err > bnd
    nbad = int(bad.sum())
    if nbad:
        r = err / bnd
        k = int(torch.argmax(r.flatten()))
        raise AssertionError("%s: %d of %d values outside the bound; worst %.3g x bound (got %r, want %r)"
                             % (what, nbad, bad.numel(), float(r.flatten()[k]), float(got.flatten()[k]),
                                float(want.flatten()[k])))


def _forward_table(monkeypatch, I, D, d, dtype, variant=4, seed=0):
    monkeypatch.setenv("BPRX_FWD_VARIANT", str(variant))
    tables, P, A = _forward_setup(I, D, d, dtype, seed)
    e = _engine(I, D, d, dtype, d + 1, tables)
    got = e.score_block(0, d + 1)
    e.sync_check()
    e.close()
    pd, ad = P[:, d][None, :], A[:, d][None, :]
    _check_scores(got[:d], P[:, :d].T, A[:, :d].T, pd, ad, dtype == "fp32", "users < d")
    _check_scores(got[d:], torch.zeros_like(pd), torch.zeros_like(ad), pd, ad, dtype == "fp32", "user d")


def _nt_cases():
    c = []
    for dt, D in (("bf16", 256), ("fp8", 512)):
        for nt in range(1, 10):
            c.append(pytest.param(dt, D, nt, 40_003, 4, id="v10-%s-nt%d-I40003" % (dt, nt)))
        for nt in (1, 5, 9):
            for I in (7, 3_001):
                c.append(pytest.param(dt, D, nt, I, 4, id="v10-%s-nt%d-I%d" % (dt, nt, I)))
    for nt in (1, 4, 9, 10, 17):
        c.append(pytest.param("bf16", 256, nt, 3_001, 0, id="plain-bf16-nt%d" % nt))
    for nt in (3, 12):
        c.append(pytest.param("fp8", 512, nt, 3_001, 0, id="plain-fp8-nt%d" % nt))
    for nt in (2, 9, 17):
        c.append(pytest.param("bf16", 384, nt, 3_001, 4, id="oddD-bf16-D384-nt%d" % nt))
    for nt in (4, 10):
        c.append(pytest.param("fp8", 768, nt, 3_001, 4, id="oddD-fp8-D768-nt%d" % nt))
    for nt in (10, 11, 13, 16, 17):
        c.append(pytest.param("fp8", 512, nt, 40_003, 4, id="f8s-nt%d" % nt))
    for nt in (10, 17):
        c.append(pytest.param("bf16", 256, nt, 40_003, 4, id="passes-bf16-nt%d" % nt))
    for D in (128, 100):
        for d in (20, 40):
            c.append(pytest.param("fp32", D, d, 1_001, 4, id="fp32-D%d-d%d" % (D, d)))
    return c


@pytest.mark.parametrize("dtype,D,nt,I,variant", _nt_cases())
def test_forward_whole_table(monkeypatch, dtype, D, nt, I, variant):
    d = nt if dtype == "fp32" else 16 * nt - 1              # PS = 16 * nt: exactly this instantiation
    _forward_table(monkeypatch, I, D, d, dtype, variant, seed=nt + I % 101)


def test_forward_streaming_loads_beyond_the_cache(monkeypatch):
    """A 300 000 x 1 024 fp8 table (307 MB > 256 MiB) takes v10's `nt`-load instantiation."""
    _forward_table(monkeypatch, 300_000, 1024, 63, "fp8", seed=3)


# (NT, row tiles as (a, b, c) = a*N // b + c with N the CU count, form): the launch_fwd_rows thresholds, met on both sides
ROW_SHAPES = [(1, (0, 1, 5), "mt1"), (2, (1, 1, 0), "split"), (2, (1, 1, 1), "mt1"), (3, (2, 3, 0), "split"),
              (9, (2, 9, 0), "split"), (9, (2, 9, 1), "mt1"), (3, (2, 1, 0), "mt1"), (3, (2, 1, 1), "mt2"), (6, (2, 1, 1), "mt2"),
              (7, (2, 1, 3), "mt2"), (8, (2, 1, 1), "mt2"), (9, (8, 1, 1), "mt2"), (5, (8, 1, 0), "mt2"), (5, (8, 1, 1), "mt4"),
              (1, (8, 1, 1), "mt4"), (4, (8, 1, 5), "mt4"), (2, (8, 1, 9), "mt4"), (3, (8, 1, 1), "mt4"), (10, (0, 1, 3), "split"),
              (17, (0, 1, 40), "mt1")]


def _row_cases():
    c = []
    for dt, D in (("bf16", 256), ("fp8", 512)):
        for nt, (a, b, k), form in ROW_SHAPES:
            c.append(pytest.param(dt, D, nt, (a, b, k), id="%s-%s-nt%d-tiles%d*N/%d+%d" % (form, dt, nt, a, b, k)))
    for nt in (10, 17):
        for nrows in (4_095, 4_096):
            c.append(pytest.param("fp8", 512, nt, nrows, id="f8s_rows-nt%d-rows%d" % (nt, nrows)))
    for D in (128, 100):
        c.append(pytest.param("fp32", D, 20, 1_000, id="fp32-D%d" % D))
    return c


@pytest.mark.parametrize("dtype,D,nt,nrows", _row_cases())
def test_forward_row_list(monkeypatch, dtype, D, nt, nrows):
    """score_pairs on a fresh handle: one forward projection row per pair, over an unsorted list full of duplicates that
    holds items 0 and I-1."""
    if isinstance(nrows, tuple):                             # row tiles from the CU count; a partial last tile
        a, b, k = nrows
        tiles = a * _ncu() // b + k
        nrows = 16 * tiles - (tiles * 7) % 16
    monkeypatch.delenv("BPRX_FWD_VARIANT", raising=False)
    I = 3_001
    d = nt if dtype == "fp32" else 16 * nt - 1
    tables, P, A = _forward_setup(I, D, d, dtype, seed=nt)
    rs = np.random.RandomState(nrows)
    items = rs.randint(0, I, size=nrows)
    items[0], items[nrows // 2], items[-1] = I - 1, 0, I - 1
    users = rs.randint(0, d + 1, size=nrows)
    e = _engine(I, D, d, dtype, d + 1, tables, max_batch=nrows)
    got = e.score_pairs(users, items)
    e.sync_check()
    e.close()
    u, i = torch.as_tensor(users, device=DEV), torch.as_tensor(items, device=DEV)
    on = u < d
    uc = u.clamp(max=d - 1)
    pu = torch.where(on, P[i, uc], torch.zeros((), dtype=P.dtype, device=DEV))
    au = torch.where(on, A[i, uc], torch.zeros((), dtype=A.dtype, device=DEV))
    _check_scores(got, pu, au, P[i, d], A[i, d], dtype == "fp32", "pairs")


# ---- backward -------------------------------------------------------------------------------------------------------
def _backward(monkeypatch, I, D, d, dtype, u, i, j, list_mode, mmax=4, seed=0):
    """One step on zero E / Bp / Gu / Gi / Bi: dE|dBp through dense_grad() and through an sgd update, against F_q^T W."""
    monkeypatch.delenv("BPRX_FWD_VARIANT", raising=False)
    monkeypatch.setenv("BPRX_LIST_MODE", "2" if list_mode else "0")
    F, Fq = _features(I, D, dtype, seed)
    U = int(u.max()) + 1
    rs = np.random.RandomState(seed + 17)
    Tu = torch.as_tensor(rs.randint(-mmax, mmax + 1, size=(U, d)).astype(np.float32) / 8.0, device=DEV)
    ud, id_, jd = (torch.as_tensor(a.astype(np.int32), device=DEV) for a in (u, i, j))
    row = torch.cat([Tu, torch.ones((U, 1), device=DEV)], 1).double()[ud.long()] * 0.5      # -g [Tu | 1]
    W = torch.zeros((I, d + 1), dtype=torch.float64, device=DEV)
    W.index_add_(0, id_.long(), -row)
    W.index_add_(0, jd.long(), row)
    assert torch.equal(W.float().to(torch.bfloat16).double(), W), "W must be exact in bf16 (fewer occurrences or smaller m)"
    gs = float(np.float32(1.0) / np.float32(FEAT_SCALE)) if dtype == "fp8" else 1.0
    ref = (Fq.T @ W) * gs
    A = (Fq.abs().T @ W.abs()) * gs
    touched = torch.as_tensor(np.union1d(i, j), device=DEV)
    assert float((W[touched] != 0).double().mean(0).min()) > 0.5     # every column of W is mostly non-zero
    if dtype == "fp32":
        bnd = _ulp(ref) + 2.0 ** -40 * A
    else:
        bnd = C_MFMA * A + 2.0 ** -23 * ref.abs()

    def tables():
        return dict(Gu=torch.zeros((U, 4), device=DEV), Gi=torch.zeros((I, 4), device=DEV), Bi=torch.zeros(I, device=DEV),
                    Tu=Tu, F=F, E=torch.zeros((D, d), device=DEV), Bp=torch.zeros(D, device=DEV))

    for path in ("dense_grad", "sgd_step"):
        e = _engine(I, D, d, dtype, U, tables(), max_batch=len(u))
        if path == "dense_grad":
            e.step_begin(ud, id_, jd)
            g = e.dense_grad().clone()
            e.step_end()
            got = torch.cat([g[:D * d].view(D, d), g[D * d:, None]], 1)
        else:
            e.step(ud, id_, jd)
            got = -torch.cat([e.t["E"], e.t["Bp"][:, None]], 1) / LR
        e.sync_check()
        e.close()
        err = (got.double() - ref).abs()
        bad = err > bnd
        if bool(bad.any()):
            r = err / bnd
            k = int(torch.argmax(r.flatten()))
            raise AssertionError("%s: %d of %d values of dE|dBp outside the bound; worst %.3g x bound at (k %d, n %d): got %r, "
                                 "want %r" % (path, int(bad.sum()), bad.numel(), float(r.flatten()[k]), k // (d + 1), k % (d + 1),
                                              float(got.flatten()[k]), float(ref.flatten()[k])))


def _whole_batch(I, seed):
    """Every item once as a positive; the negatives are drawn from half of the items (about twice each).  (Once as a positive
    and once as a negative would cancel W's Bp column on every row.)"""
    rs = np.random.RandomState(seed)
    return rs.randint(0, 64, size=I), rs.permutation(I), rs.permutation(I)[rs.randint(0, I // 2, size=I)]


def _grid_D():
    """The smallest D % 256 == 0 whose split count is not a multiple of 8 (the XCD remap is off): 1 280 at 256 CUs."""
    for D in range(256, 8192 + 1, 256):
        if _sk(D, 5, False) % 8:
            return D
    return 1280


def _bwd_cases():
    c = []
    for nt in range(1, 10):                                  # bf16, 8 waves, PD = 3
        for t in ("t1", "t2", "t3", "t4", "many") if nt in (1, 4, 9) else ("t2", "t4"):
            c.append(pytest.param("bf16", 256, nt, t, id="pd3-nt%d-%s" % (nt, t)))
    for nt in range(1, 10):                                  # fp8: DB = 2
        for t in ("t3", "many") if nt in (1, 9) else ("t2", "t3"):
            c.append(pytest.param("fp8", 512, nt, t, id="db2-fp8-nt%d-%s" % (nt, t)))
    for dt, D in (("bf16", 256), ("fp8", 512)):              # NS = 2
        for nt in (10, 11, 13, 17):
            for t in ("t3", "t4"):
                c.append(pytest.param(dt, D, nt, t, id="ns2-%s-nt%d-%s" % (dt, nt, t)))
    for D in (128, 384):                                     # 4 waves
        for nt in (3, 9, 10, 17):
            c.append(pytest.param("bf16", D, nt, "t2" if nt % 2 else "t4", id="w4-D%d-nt%d" % (D, nt)))
    for nt in (5, 12):
        c.append(pytest.param("bf16", "grid", nt, "t4", id="grid-nt%d" % nt))
    for D in (128, 100):
        c.append(pytest.param("fp32", D, 2, "t2", id="fp32-D%d" % D))
    return c


@pytest.mark.parametrize("dtype,D,nt,tiles", _bwd_cases())
def test_backward_whole_table(monkeypatch, dtype, D, nt, tiles):
    if D == "grid":
        D = _grid_D()
    if dtype == "fp32":
        d, I = 20, 3_001 + nt
    else:
        d = 16 * nt - (4 if nt % 2 == 0 else 1)              # d % 4 == 0: k_item_seg writes W; odd d: the atomic staging path
        I = _items_for(tiles, _sk(D, nt, dtype == "fp8"))
    u, i, j = _whole_batch(I, seed=I % 1000 + nt)
    _backward(monkeypatch, I, D, d, dtype, u, i, j, list_mode=False, seed=nt)


def _rows_cases():
    c = []
    for nt in (2, 9, 11, 17):
        c.append(pytest.param("bf16", 256, nt, False, id="rows-nw8-bf16-nt%d" % nt))
    for nt in (4, 10, 13):
        c.append(pytest.param("fp8", 512, nt, False, id="rows-nw8-fp8-nt%d" % nt))
    for nt in (3, 10):
        c.append(pytest.param("bf16", 384, nt, False, id="rows-nw4-bf16-nt%d" % nt))
    for dt, D, nt in (("bf16", 256, 5), ("fp8", 512, 11), ("bf16", 384, 10)):
        c.append(pytest.param(dt, D, nt, True, id="rows-dups-%s-D%d-nt%d" % (dt, D, nt)))
    for D in (128, 100):                                     # fp32: k_proj_bwd_f32_tile (D % 8 == 0) / k_proj_bwd_f32 rows
        c.append(pytest.param("fp32", D, 2, False, id="rows-fp32-D%d" % D))
        c.append(pytest.param("fp32", D, 2, True, id="rows-dups-fp32-D%d" % D))
    return c


@pytest.mark.parametrize("dtype,D,nt,dups", _rows_cases())
def test_backward_row_list(monkeypatch, dtype, D, nt, dups):
    """List mode: the backward runs over the batch's distinct items.  B = 4 096 over 20 011 items gives ~7 500 listed rows (4
    tiles per split); the duplicate-heavy batch draws its items from 50 ids, far below the host bound of 8 192 rows, so most
    of the splits are empty."""
    I, B = 20_011, 4_096
    d = 20 if dtype == "fp32" else 16 * nt - 1
    rs = np.random.RandomState(nt + 31 * dups)
    if dups:
        pool = np.concatenate([[0, I - 1], rs.choice(np.arange(1, I - 1), 48, replace=False)])
        i, j = pool[rs.randint(0, 50, size=B)], pool[rs.randint(0, 50, size=B)]
    else:
        i, j = rs.randint(0, I, size=B), rs.randint(0, I, size=B)
        i[0], j[1] = 0, I - 1
    u = rs.randint(0, 64, size=B)
    _backward(monkeypatch, I, D, d, dtype, u, i, j, list_mode=True, mmax=1 if dups else 4, seed=nt)
