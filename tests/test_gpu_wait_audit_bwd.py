"""The masked whole-table backward (k_proj_bwd_bf16_v3<.., MASK>) after its prologue was reordered: the tile's
row-bit word is read ahead of the tile's loads, the prologue reads its PD words first and issues its PD tiles one by one.  A
prologue that is issued in another order goes wrong where a split holds fewer tiles than are in flight, so the item counts
are those of test_gpu_projections.test_backward_whole_table[pd3-*]: 1, 2, 3, 4 and 25 tiles of 32 items per split (SK as
bprx_create computes it), and "t2h": I = 48 SK - 16, two tiles per split, the last split's second tile half full.

Per case, for each touched set of test_gpu_proj_mask (every item / no row of some whole tiles / a random half / only item
I - 1), on that file's hand-built batches (every touched item in exactly one triplet) and test_gpu_projections' exact-W
construction (zero E / Bp / Gu / Gi / Bi: g = -0.5, W exact in fp32 and in bf16):
  * dE|dBp of the masked step == dE|dBp of the unmasked step (BPRX_PROJ_MASK=0), torch.equal: the skipped products are x * 0
    (DESIGN §4), only the sign of a zero may differ, which == ignores;
  * both against F_q^T W in float64 at test_gpu_projections' bound, 2e-5 of the absolute sum (+ 2^-23 of the value).
"only item I - 1": the item is the positive and the negative of its one triplet, its W row is exactly zero and so is dE|dBp; the
case still walks a split whose only set bit is the table's last row.

Shapes: bf16 features, D = 256 and 512; d = 15, 64, 143 (one, five, nine column tiles).  The mask needs segment mode, i.e.
d % 4 == 0 (test_gpu_proj_mask's docstring): d = 15 and 143 run the unmasked kernel on both sides (kind 0), so d = 12 and 140
stand beside them for the masked one- and nine-tile forms (kind 1 is asserted).  One fp8 case (the PD = 2, double-buffered
form) through BPRX_PROJ_MASK=2."""
import numpy as np
import pytest
import torch

import test_gpu_proj_mask as pm
import test_gpu_projections as tp

pytestmark = pytest.mark.gpu

DEV = tp.DEV
SETS = ("all", "hole", "half", "last")
TILES = ("t1", "t2", "t2h", "t3", "t4", "many")


def _items(tiles, SK):
    return 48 * SK - 16 if tiles == "t2h" else tp._items_for(tiles, SK)


def _cases():
    c = [pytest.param("bf16", D, d, t, id="bf16-D%d-d%d-%s" % (D, d, t)) for D in (256, 512) for d in (15, 12, 64, 143, 140)
         for t in TILES]
    return c + [pytest.param("fp8", 512, 64, "t3", id="fp8-D512-d64-t3")]


@pytest.mark.parametrize("dtype,D,d,tiles", _cases())
def test_masked_backward_equals_unmasked_and_fp64(monkeypatch, dtype, D, d, tiles):
    I = _items(tiles, tp._sk(D, (d + 1 + 15) // 16, dtype == "fp8"))
    F, Fq = tp._features(I, D, dtype, seed=d)
    gs = float(np.float32(1.0) / np.float32(tp.FEAT_SCALE)) if dtype == "fp8" else 1.0
    z = lambda *s: torch.zeros(s, device=DEV)
    for s, kind in enumerate(SETS):
        S = pm._touched(kind, I, seed=s)
        ud, id_, jd = pm._batch(S, seed=40 + s)
        U = int(ud.max()) + 1
        rs = np.random.RandomState(17 + s)
        Tu = torch.as_tensor(rs.randint(-4, 5, size=(U, d)).astype(np.float32) / 8.0, device=DEV)
        row = torch.cat([Tu, torch.ones((U, 1), device=DEV)], 1).double()[ud.long()] * 0.5      # -g [Tu | 1]
        W = torch.zeros((I, d + 1), dtype=torch.float64, device=DEV)
        W.index_add_(0, id_.long(), -row)
        W.index_add_(0, jd.long(), row)
        assert torch.equal(W.float().to(torch.bfloat16).double(), W)
        ref, A = (Fq.T @ W) * gs, (Fq.abs().T @ W.abs()) * gs
        bnd = tp.C_MFMA * A + 2.0 ** -23 * ref.abs()
        if kind != "last":
            assert int((ref != 0).sum()) > ref.numel() // 2
        t = dict(Gu=z(U, 4), Gi=z(I, 4), Bi=z(I), Tu=Tu, F=F, E=z(D, d), Bp=z(D))
        got = {}
        for mask in (True, False):
            e = pm._engine(monkeypatch, mask, I, D, d, dtype, U, t, len(ud))
            g = pm._step(e, (ud, id_, jd))
            assert pm._kind(e) == (1 if mask and d % 4 == 0 else 0), (kind, mask)
            e.sync_check()
            e.close()
            got[mask] = torch.cat([g[:D * d].view(D, d), g[D * d:, None]], 1)
        pm._same(got[True], got[False], "dE|dBp masked vs unmasked, touched set '%s'" % kind)
        for mask in (True, False):
            err = (got[mask].double() - ref).abs()
            r = float((err / bnd.clamp_min(1e-300)).max())
            assert bool((err <= bnd).all()), "touched set '%s', mask %d: worst %.3g x bound" % (kind, mask, r)
