"""The group and cache edges of the one fit loop behind bprx_fold_in, bprx_fold_in_items and bprx_af_fold_in_items (k_fold_fit,
bprx_foldin.hip), at the lane widths the other fold-in tests do not reach together: per call four rows with 0, 1, NP + 1 and
`SPLIT` pairs, so that the empty row, a tail group and a row split between the LDS form and the per-step form (with a tail group of
its own) meet in one launch.  fit = 2560 // (64 EPL + 1) pairs of a row live in LDS, whole groups of NP where the row has more:

    EPL 1 (row <= 64 wide)    NP 4, fit 39: rows of 0, 1, 5 and 45 pairs (36 from LDS, then groups of 4, 4 and 1)
    EPL 2 (65 .. 128)         NP 4, fit 19: rows of 0, 1, 5 and 25 pairs (16 from LDS, then 4, 4 and 1)
    EPL 6 (257 .. 384)        NP 2, fit 6:  rows of 0, 1, 3 and 9 pairs (6 from LDS, then 2 and 1)

Every fit is compared with its float64 restatement (fold_in_ref, item_fold_ref, af_item_fold_ref) under the allowance of its own
test module (32 x the float32 restatement's deviation, Adam on the entries the module's rule keeps), and the split row's bits must
not depend on the rows around it nor on BPRX_FOLD_CACHE.  AttentiveFashion rows are k wide, not k + 1: k = 256 is four lane words
(NP 4, fit 9: rows of 0, 1, 5 and 14 pairs) and k = 260 the EPL 6 shape; both run."""
import numpy as np
import pytest

import af_item_fold_cases as AK
import fold_in_ref
import item_fold_cases as IC
import test_gpu_af_item_fold as TA
import test_gpu_fold_in as TU
import test_gpu_item_fold as TI
from test_gpu_feat_explain import _bits

pytestmark = pytest.mark.gpu

COUNTS = {1: [0, 1, 5, 45], 2: [0, 1, 5, 25], 4: [0, 1, 5, 14], 6: [0, 1, 3, 9]}
SPLIT = 3                                                     # the row with more pairs than fit


def _ptr(epl):
    return np.concatenate([[0], np.cumsum(COUNTS[epl])]).astype(np.int64)


def _adam_keep(grads, ptr, width):
    """The rule of the fold-in test modules: entries whose float64 |g| at any step is below 1e-3 of the row's largest are left out."""
    keep = np.ones((len(ptr) - 1, width), bool)
    for r in np.nonzero(np.diff(ptr) > 0)[0]:
        g = np.abs(grads[r])
        keep[r] = ~(g < 1e-3 * g.max(1, keepdims=True)).any(0)
    return keep


@pytest.mark.parametrize("epl,k,d", [(1, 16, 12), (2, 40, 25), (6, 200, 100)])
def test_new_users_at_the_group_and_cache_edges(monkeypatch, epl, k, d):
    t = TU._item_tables(k, d, seed=k)
    e = TU._engine(t)
    P = TU._proj(e, t)
    rs = np.random.RandomState(300 + k)
    ptr = _ptr(epl)
    pos, neg = (rs.randint(TU.I, size=int(ptr[-1])).astype(np.int32) for _ in range(2))
    W0 = (rs.standard_normal((4, k + d)) * 0.3).astype(np.float32)
    full = {}
    for name, hp in (("sgd", TU.SGD), ("adam", TU.ADAM)):
        r64, r32 = (fold_in_ref.fold_in(t["Gi"], t["Bi"], P, ptr, pos, neg, W0[:, :k], W0[:, k:], hp["steps"], hp["lr"], hp["reg"],
                                        hp["optimizer"], dt) for dt in (np.float64, np.float32))
        got = full[name] = TU._fold(e, ptr, pos, neg, W0, **hp)
        keep = _adam_keep(r64["grads"], ptr, k + d) if name == "adam" else np.ones((4, k + d), bool)
        assert 1.0 - keep[1:].mean() <= 0.02
        gdev, allow = TU._report("%s rows EPL %d" % (name, epl), TU._rows(r64, d)[keep], TU._rows(r32, d)[keep], TU._rows(got, d)[keep])
        assert gdev <= allow
        ldev, lallow = TU._report("%s loss EPL %d" % (name, epl), r64["loss"], r32["loss"], got[2])
        assert ldev <= lallow
        assert got[2][0] == 0 and np.array_equal(_bits(TU._rows(got, d)[0]), _bits(W0[0]))     # no pairs: the row stays, loss 0
        for rows in ([SPLIT], [SPLIT, 0, 2]):
            part = TU._fold(e, *TU._sub(ptr, pos, neg, W0, rows), **hp)
            assert np.array_equal(_bits(TU._rows(part, d)), _bits(TU._rows(got, d)[rows])), (name, rows)
            assert np.array_equal(_bits(part[2]), _bits(got[2][rows])), (name, rows)
    monkeypatch.setenv("BPRX_FOLD_CACHE", "0")                                    # read at create: every pair is gathered per step
    e0 = TU._engine(t)
    for name, hp in (("sgd", TU.SGD), ("adam", TU.ADAM)):
        plain = TU._fold(e0, ptr, pos, neg, W0, **hp)
        assert np.array_equal(_bits(TU._rows(plain, d)), _bits(TU._rows(full[name], d))), name
        assert np.array_equal(_bits(plain[2]), _bits(full[name][2])), name
    for eng in (e, e0):
        eng.sync_check()
        eng.close()


@pytest.mark.parametrize("epl,k,d", [(1, 16, 12), (2, 64, 20), (6, 256, 20)])
def test_warm_items_at_the_group_and_cache_edges(monkeypatch, epl, k, d):
    t = IC.tables(k, d, seed=k)
    t["Fn"] = t["Fn"][:4]
    e = TI._engine(t)
    _, P = TI._proj(e, t["F"])
    Pn_dev, Pn = TI._proj(e, t["Fn"])
    rs = np.random.RandomState(300 + k)
    ptr = _ptr(epl)
    n = int(ptr[-1])
    user, other, role = (rs.randint(m, size=n).astype(np.int32) for m in (IC.U, IC.I, 2))
    W0 = (rs.standard_normal((4, k + 1)) * 0.3).astype(np.float32)
    a = (ptr, user, other, role, W0)
    full = {}
    for name, hp in (("sgd", IC.SGD), ("adam", IC.ADAM)):
        r64, r32 = (IC.restate(t, P, Pn, *a, hp, dt) for dt in (np.float64, np.float32))
        got = full[name] = TI._fold(e, Pn_dev, *a, **hp)
        keep = _adam_keep(r64["grads"], ptr, k + 1) if name == "adam" else np.ones((4, k + 1), bool)
        assert 1.0 - keep[1:].mean() <= 0.02
        gdev, allow = TI._report("%s rows EPL %d" % (name, epl), IC.rows(r64)[keep], IC.rows(r32)[keep], IC.rows(got)[keep])
        assert gdev <= allow
        ldev, lallow = TI._report("%s loss EPL %d" % (name, epl), r64["loss"], r32["loss"], got[2])
        assert ldev <= lallow
        assert got[2][0] == 0 and np.array_equal(_bits(IC.rows(got)[0]), _bits(W0[0]))          # no pairs: the rows stay, loss 0
        for rows in ([SPLIT], [SPLIT, 0, 2]):
            part = TI._fold(e, *TI._sub(Pn_dev, *a, rows), **hp)
            assert np.array_equal(_bits(IC.rows(part)), _bits(IC.rows(got)[rows])), (name, rows)
            assert np.array_equal(_bits(part[2]), _bits(got[2][rows])), (name, rows)
    monkeypatch.setenv("BPRX_FOLD_CACHE", "0")                                    # read at create: every pair is formed per step
    e0 = TI._engine(t)
    Pn0, _ = TI._proj(e0, t["Fn"])
    for name, hp in (("sgd", IC.SGD), ("adam", IC.ADAM)):
        plain = TI._fold(e0, Pn0, *a, **hp)
        assert np.array_equal(_bits(IC.rows(plain)), _bits(IC.rows(full[name]))), name
        assert np.array_equal(_bits(plain[2]), _bits(full[name][2])), name
    for eng in (e, e0):
        eng.sync_check()
        eng.close()


# (The seed of a width's tables: k, unless Adam's rule then leaves out more than 4.5 % of the float64 restatement's entries, half
# a point inside the module's 5 %: a row with one pair alone leaves out 3 .. 8 % here.  On the GPU's encodings: 5.6 % at k = 65
# seed 65, 5.1 % at k = 256 seed 256, 4.7 % at k = 260 seed 260; 2.6 %, 4.4 % and 3.6 % with the seeds below.)
@pytest.mark.parametrize("epl,k,seed", [(1, 16, 16), (2, 65, 1065), (4, 256, 1256), (6, 260, 2260)])
def test_attentive_warm_items_at_the_group_and_cache_edges(monkeypatch, epl, k, seed):
    h = 32
    t, inputs, new, _ = AK.tables(k, h, seed=seed, n_new=4)
    e = TA._engine(t, inputs)
    Cg = e.af_encode(np.arange(AK.I)).cpu().numpy()
    Cn_dev = e.af_encode_new(*new)
    Cn = Cn_dev.cpu().numpy()
    rs = np.random.RandomState(300 + k)
    ptr = _ptr(epl)
    n = int(ptr[-1])
    user, other, role = (rs.randint(m, size=n).astype(np.int32) for m in (AK.U, AK.I, 2))
    W0 = (rs.standard_normal((4, k)) * 0.3).astype(np.float32)
    c = dict(ptr=ptr, W0=W0)
    args = (Cn, ptr, user, other, role, W0)
    full = {}
    for name, hp in (("sgd", AK.SGD), ("adam", AK.ADAM)):
        r64, r32 = (AK.restate(t, Cg, Cn, *args[1:], hp, dt) for dt in (np.float64, np.float32))
        got = full[name] = TA._fold(e, Cn_dev, *args[1:], **hp)
        TA._check("%s EPL %d k=%d" % (name, epl, k), hp, c, r64, r32, got[0], got[1])
        for rows in ([SPLIT], [SPLIT, 0, 2]):
            part = TA._fold(e, *TA._sub(*args, rows), **hp)
            assert np.array_equal(_bits(part[0]), _bits(got[0][rows])), (name, rows)
            assert np.array_equal(_bits(part[1]), _bits(got[1][rows])), (name, rows)
    monkeypatch.setenv("BPRX_FOLD_CACHE", "0")                                    # read at create: every step reads work again
    e0 = TA._engine(t, inputs)
    for name, hp in (("sgd", AK.SGD), ("adam", AK.ADAM)):
        plain = TA._fold(e0, *args, **hp)
        assert np.array_equal(_bits(plain[0]), _bits(full[name][0])), name
        assert np.array_equal(_bits(plain[1]), _bits(full[name][1])), name
    for eng in (e, e0):
        eng.sync_check()
        eng.close()
