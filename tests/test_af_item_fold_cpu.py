"""Warm items and audiences for AttentiveFashion without a GPU: the four entries in the header, the binding and the library, the
three command-line flags and their tables, the lists and files of AttentiveFashion.recommend_warm / audience_warm / audience over a
stub engine (the pattern of tests/test_audience_cpu.py, with the attentions as side columns), the restatement
(tests/af_item_fold_ref.py) against finite differences of its own loss, and what tests/test_gpu_af_item_fold.py relies on in its
inputs (tests/af_item_fold_cases.py), asserted with the CPU encoder restatement attentive_ref.AttentiveRef.encode."""
import os
import re
from argparse import Namespace

import numpy as np
import pytest
import torch

import af_item_fold_cases as K
import af_item_fold_ref as R
import item_fold_ref as IR
import topk_ref as tr
from fashionvisualexpl_recommend_amd import _ffi, models, ranking, train_rec

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "bprx.h")
ENTRIES = (("bprx_af_encode_new", 7), ("bprx_af_fold_in_items", 15), ("bprx_af_score_warm_block", 9), ("bprx_af_audience_block", 9))


# ---- names, ABI, errors ----------------------------------------------------------------------------------------------------------
def test_the_header_the_binding_and_the_library_agree_on_the_four_entries():
    header = open(HEADER).read()
    lib = _ffi.lib()
    assert "#define BPRX_ABI_VERSION 6" in header and _ffi.ABI_VERSION == 6 and lib.bprx_abi_version() == 6
    for name, nargs in ENTRIES:
        assert name in _ffi.EXPORTS and hasattr(lib, name)
        decl = re.search(r"BPRX_API int %s\(([^;]*)\);" % name, header)
        assert decl, name
        assert len(decl.group(1).split(",")) == nargs == len(getattr(lib, name).argtypes), name
    # a NULL handle is rejected before anything is read
    assert lib.bprx_af_encode_new(None, None, None, None, 0, None, None) == _ffi.E_INVALID
    assert lib.bprx_af_fold_in_items(None, None, None, None, None, 0, None, 1, 0.1, 0.0, 0, None, None, None, None) == _ffi.E_INVALID
    assert lib.bprx_af_score_warm_block(None, 0, 0, None, None, 0, None, None, None) == _ffi.E_INVALID
    assert lib.bprx_af_audience_block(None, None, None, 0, 0, 0, None, None, None) == _ffi.E_INVALID


def _npy(tmp_path, n=3, Dc=5, Dk=4, **over):
    rs = np.random.RandomState(1)
    a = dict(edges=rs.randint(0, 256, size=(n, 224, 224)).astype(np.uint8), colour=(rs.random_sample((n, Dc)) * 9).astype(np.float32),
             classes=rs.random_sample((n, Dk)).astype(np.float32))
    a.update(over)
    paths = []
    for name in ("edges", "colour", "classes"):
        p = str(tmp_path / (name + "-%d.npy" % len(os.listdir(tmp_path))))
        np.save(p, a[name])
        paths.append(p)
    return paths


def test_flags_default_to_off_and_are_rejected_elsewhere(tmp_path, capsys):
    warm = tmp_path / "warm.tsv"
    warm.write_text("0\t3\n2\t1\n")
    new = _npy(tmp_path)
    for rec in ("bprmf", "vbpr", "grad_fashion", "acf", "attentive_fashion"):
        a = train_rec.parse_args(["--rec", rec])
        assert a.af_new_items is None and a.af_warm_items is None and a.af_audience == 0
    for rec in ("bprmf", "vbpr", "grad_fashion", "acf"):
        for argv, word in ((["--af_new_items"] + new, "af_new_items"), (["--af_new_items"] + new + ["--af_warm_items", str(warm)], "af_"),
                           (["--af_audience", "5"], "af_audience")):
            with pytest.raises(SystemExit):
                train_rec.parse_args(["--rec", rec] + argv)
            assert word in capsys.readouterr().err, (rec, argv)
    af = ["--rec", "attentive_fashion"]
    for argv in (["--af_warm_items", str(warm)],                                      # without --af_new_items
                 ["--af_new_items"] + new + ["--af_warm_items", str(tmp_path / "missing.tsv")],
                 ["--af_audience", "-1"], ["--af_audience", "1025"], ["--af_new_items"] + new[:2]):
        with pytest.raises(SystemExit):
            train_rec.parse_args(af + argv)
        assert "af_" in capsys.readouterr().err, argv
    a = train_rec.parse_args(af + ["--af_new_items"] + new + ["--af_warm_items", str(warm), "--af_audience", "1024"])
    assert a.af_new_items == new and a.af_audience == 1024
    # the existing flags keep rejecting the model
    for argv in (["--audience", "5"], ["--warm_items", str(warm)], ["--new_items", new[1]]):
        with pytest.raises(SystemExit):
            train_rec.parse_args(af + argv)
    capsys.readouterr()
    for argv, word in ((["--af_audience", "5"], "af_audience"), (["--af_new_items"] + new, "af_new_items"),
                       (["--af_new_items"] + new + ["--af_warm_items", str(warm)], "af_")):
        with pytest.raises(NotImplementedError, match=word):
            train_rec.train(af + argv + ["--world_size", "2"])


def test_the_new_items_tables_are_checked(tmp_path):
    ed, col, cl = train_rec.read_af_new_items(_npy(tmp_path))
    assert ed.dtype == np.uint8 and ed.shape == (3, 224, 224) and col.shape == (3, 5) and cl.shape == (3, 4)
    zero = np.ones((3, 5), np.float32)
    zero[1] = 0
    for over, word in ((dict(edges=np.zeros((3, 224, 224), np.float32)), "uint8"), (dict(edges=np.zeros((3, 224, 200), np.uint8)), "224"),
                       (dict(colour=np.ones((2, 5), np.float32)), "colour"), (dict(classes=np.ones((3,), np.float32)), "classes"),
                       (dict(colour=zero), "row 1 is all zero"), (dict(classes=np.array([["a"] * 4] * 3)), "classes")):
        with pytest.raises(ValueError, match=word):
            train_rec.read_af_new_items(_npy(tmp_path, **over))
    with pytest.raises(ValueError):
        train_rec.read_af_new_items(_npy(tmp_path)[:2])
    with pytest.raises(ValueError, match="past the table"):          # a row past the tables, before anything is loaded
        bad = tmp_path / "bad.tsv"
        bad.write_text("3\t0\n")
        train_rec.train(["--rec", "attentive_fashion", "--af_new_items"] + _npy(tmp_path) + ["--af_warm_items", str(bad)])


# ---- lists and files over a stub engine ------------------------------------------------------------------------------------------
U_USERS, I_ITEMS, N_WARM, KK, HH, DC, DK = 20, 9, 6, 6, 5, 5, 4


class _StubEngine:
    """The engine calls the warm lists make, on the CPU: float32 scores and attentions from af_item_fold_ref.scores, the top-K entry
    of tests/test_audience_cpu.py (mask IN the scores; undetermined rows come back flagged with idx -1 / val nan)."""
    device = "cpu"

    def __init__(self, **kw):
        self.kw, self.calls, self.flags = kw, [], []
        self.k = kw["embed_k"]

    def bind_attentive(self, Gu, Gi, Bi, edges, color, cls, weights, dropout=0.5, seed=0):
        self.t = dict(Gu=np.asarray(Gu), Gi=np.asarray(Gi), **{n: np.asarray(v) for n, v in weights.items()})
        self.U, self.I = self.t["Gu"].shape[0], self.t["Gi"].shape[0]
        rs = np.random.RandomState(5)
        self.Call = (rs.standard_normal((3, self.I, self.k)) * 0.5).astype(np.float32)
        return self

    def csr(self, lists):
        return [[int(u) for u in l] for l in lists]

    def af_encode_new(self, edges, color, cls):
        n = len(edges)
        self.calls.append(("encode", n))
        return torch.from_numpy((np.random.RandomState(6).standard_normal((3, n, self.k)) * 0.5).astype(np.float32))

    def af_fold_in_items(self, ptr, user, other, role, steps, C_rows, Gi_rows, lr=None, reg=None, optimizer=None, want_loss=True):
        self.calls.append(("fold", steps, len(user), lr, reg, optimizer))
        ptr = np.asarray(ptr)
        fit = (np.random.RandomState(8).standard_normal(tuple(Gi_rows.shape)) * 0.5).astype(np.float32)
        fit[np.diff(ptr) == 0] = 0                              # an item without pairs keeps its (zero) row
        Gi_rows.copy_(torch.from_numpy(fit))

    def _block(self, C, Gi):
        att = tuple(self.t[n] for n in R.ATT)
        x, al = R.scores(self.t["Gu"], att, C, Gi, np.float32)
        return x, al

    def af_score_warm_block(self, u0, u1, C_rows, Gi_rows):
        self.calls.append(("warm", u0, u1))
        x, al = self._block(C_rows.numpy(), Gi_rows.numpy())
        return torch.from_numpy(x[u0:u1].copy()), torch.from_numpy(al[u0:u1].copy())

    def af_audience_block(self, q0, q1, C_rows=None, Gi_rows=None):
        self.calls.append(("audience", q0, q1, C_rows is None))
        x, al = self._block(self.Call, self.t["Gi"]) if C_rows is None else self._block(C_rows.numpy(), Gi_rows.numpy())
        return torch.from_numpy(x.T[q0:q1].copy()), torch.from_numpy(al.transpose(1, 0, 2)[q0:q1].copy())

    def topk_rows_masked(self, scores, own, k):
        s = scores.numpy()
        n, width = s.shape
        assert len(own) == n
        for r, l in enumerate(own):
            s[r, l] = -np.inf
        idx, val, flag = np.full((n, k), -1, np.int32), np.full((n, k), np.nan, np.float32), np.ones(n, np.int32)
        for r in range(n):
            if tr.classify(s[r], k, width - len(set(own[r]))) == tr.DETERMINED:
                idx[r] = tr.unique_topk(s[r], k)
                val[r], flag[r] = s[r][idx[r]], 0
        self.flags.append(flag.copy())
        return torch.from_numpy(idx), torch.from_numpy(val), torch.from_numpy(flag)


def _model(monkeypatch, **over):
    monkeypatch.setattr(models, "Engine", _StubEngine)
    rs = np.random.RandomState(12)
    tl = [rs.choice(I_ITEMS, size=rs.randint(1, 4), replace=False).tolist() for _ in range(U_USERS)]
    data = Namespace(num_users=U_USERS, num_items=I_ITEMS, training_list=tl, validation_list=[], test_list=[],
                     params=Namespace(batch_eval=128))
    p = dict(epochs=1, batch_size=16, embed_k=KK, lr=0.001, reg=0.01, top_k=3, dataset="toy", rec="attentive_fashion", optimizer="sgd",
             init_seed=0, attention_layers=[HH, 1], dropout=0.5, dtype="fp32")
    p.update(over)
    inputs = (np.zeros((I_ITEMS, 224, 224), np.uint8), np.ones((I_ITEMS, DC), np.float32), np.ones((I_ITEMS, DK), np.float32))
    Gu = (rs.standard_normal((U_USERS, KK)) * 0.5).astype(np.float32)
    m = models.AttentiveFashion(data, Namespace(**p), init={"Gu": Gu, "Gi": (rs.standard_normal((I_ITEMS, KK)) * 0.5).astype(np.float32)},
                                inputs=inputs)
    return m, data


def _new_inputs(n=N_WARM):
    rs = np.random.RandomState(3)
    return (rs.randint(0, 256, size=(n, 224, 224)).astype(np.uint8), (rs.random_sample((n, DC)) * 7).astype(np.float32),
            rs.random_sample((n, DK)).astype(np.float32))


def _reference(x, al, own, k):
    """numpy_topk on every masked float32 row (ids -1 where the masked value is -inf) and the attentions at those ids."""
    sc = x.copy()
    for r, l in enumerate(own):
        sc[r, list(l)] = -np.inf
    kk = min(k, sc.shape[1])
    ids = np.stack([ranking.numpy_topk(sc[r], k)[:kk] for r in range(sc.shape[0])]).astype(np.int64)
    vals = np.take_along_axis(sc, ids, axis=1)
    att = np.stack([al[r][ids[r]] for r in range(sc.shape[0])])
    ids[np.isneginf(vals)] = -1
    return ids, vals, att


BUYERS = [[3, 7, 3], [], [0, 1, 2, 4, 5, 6, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18], [5], [19, 0], [2]]


def test_prepare_new_items_normalises_and_checks(monkeypatch):
    m, _ = _model(monkeypatch)
    ed, col, cl = _new_inputs()
    got = m.prepare_new_items(ed, col, cl)
    assert isinstance(got, models.AfNewItems) and got[0].dtype == torch.uint8 and got[1].dtype == got[2].dtype == torch.float32
    assert np.array_equal(got[1].numpy(), (col / np.abs(col).max(1, keepdims=True)).astype(np.float32))
    assert np.array_equal(got[0].numpy(), ed) and np.array_equal(got[2].numpy(), cl)
    zero = col.copy()
    zero[4] = 0
    for args, word in (((ed, zero, cl), "row 4 is all zero"), ((ed.astype(np.int32), col, cl), "uint8"), ((ed, col[:, :4], cl), "colour"),
                       ((ed, col, cl[:5]), "classes"), ((ed[:, :, :100], col, cl), "224")):
        with pytest.raises(ValueError, match=word):
            m.prepare_new_items(*args)
    with pytest.raises(ValueError):
        m.fold_in_items(BUYERS)                                  # no features
    with pytest.raises(ValueError):
        m.fold_in_items(BUYERS[:2], _new_inputs())               # two buyer lists for six items


@pytest.mark.parametrize("block", [4, 1, 4096])
def test_warm_lists_and_audiences_honour_masks_and_carry_the_attentions(monkeypatch, block):
    m, data = _model(monkeypatch, af_audience=4)
    assert m.audience_k == 4
    m.evaluator.user_block = block
    eng = m.engine
    rows = m.fold_in_items(BUYERS, _new_inputs(), steps=7, negatives=2, seed=1)
    Gi, Cn = rows
    assert tuple(Gi.shape) == (N_WARM, KK) and tuple(Cn.shape) == (3, N_WARM, KK) and not Gi[1].any() and Gi[0].any()
    assert eng.calls[0] == ("encode", N_WARM) and eng.calls[1][:2] == ("fold", 7) and eng.calls[1][3:] == (0.001, 0.01, "sgd")
    x, al = eng._block(Cn.numpy(), Gi.numpy())
    assert not x[:, 1].any()                                     # a row without buyers scores 0.0 for everyone
    bought = [[j for j, who in enumerate(BUYERS) if u in who] for u in range(U_USERS)]
    ids, vals, att = m._rank_warm_recs(rows, BUYERS)
    wid, wval, watt = _reference(x, al, bought, 3)
    assert ids.shape == (U_USERS, 3) and att.shape == (U_USERS, 3, 3)
    assert np.array_equal(ids, wid) and np.array_equal(vals.view(np.uint32), wval.view(np.uint32))
    assert np.array_equal(att.view(np.uint32), watt.view(np.uint32))
    for u in range(U_USERS):
        assert not set(ids[u][ids[u] >= 0].tolist()) & set(bought[u]), u
    aid, aval, aatt = m._rank_warm_audience(rows, BUYERS)
    wid, wval, watt = _reference(x.T.copy(), al.transpose(1, 0, 2), [set(b) for b in BUYERS], 4)
    assert aid.shape == (N_WARM, 4) and np.array_equal(aid, wid) and np.array_equal(aval.view(np.uint32), wval.view(np.uint32))
    assert np.array_equal(aatt[aid >= 0].view(np.uint32), watt[wid >= 0].view(np.uint32))
    assert (aid[2] >= 0).sum() == 3 and set(aid[2, :3].tolist()) == {3, 7, 19} and np.isneginf(aval[2, 3])   # 17 of 20 users bought item 2
    # the catalogue: owners excluded
    cx, cal = eng._block(eng.Call, eng.t["Gi"])
    own = [[u for u in range(U_USERS) if i in data.training_list[u]] for i in range(I_ITEMS)]
    cid, cval, catt = m.audience()
    wid, wval, watt = _reference(cx.T.copy(), cal.transpose(1, 0, 2), own, 4)
    assert np.array_equal(cid, wid) and np.array_equal(cval.view(np.uint32), wval.view(np.uint32))
    assert np.array_equal(catt[cid >= 0].view(np.uint32), watt[wid >= 0].view(np.uint32))
    pick = [8, 0, 0, 5]
    pid, pval, patt = m.audience(pick, k=2)
    assert pid.shape == (4, 2) and np.array_equal(pid, wid[pick][:, :2]) and np.array_equal(patt, watt[pick][:, :2])
    with pytest.raises(ValueError, match="audience"):
        m.audience([I_ITEMS])
    assert any(c[0] == "audience" and c[3] for c in eng.calls) and any(c[0] == "audience" and not c[3] for c in eng.calls)
    assert any(f.any() for f in eng.flags)                       # some rows went through numpy
    # the public pair of calls: one fit each
    r2 = m.recommend_warm(BUYERS, _new_inputs(), steps=7, negatives=2, seed=1)
    assert np.array_equal(r2[0], ids) and np.array_equal(r2[2], att)
    a2 = m.audience_warm(BUYERS, _new_inputs(), k=4, steps=7, negatives=2, seed=1)
    assert np.array_equal(a2[0], aid)


def test_the_three_files(monkeypatch, tmp_path):
    ed, col, cl = _new_inputs()
    paths = [str(tmp_path / n) for n in ("e.npy", "c.npy", "k.npy")]
    for p, a in zip(paths, (ed, col, cl)):
        np.save(p, a)
    warm = tmp_path / "warm.tsv"
    warm.write_text("".join("%d\t%d\n" % (j, u) for j, who in enumerate(BUYERS) for u in who))
    m, data = _model(monkeypatch, af_audience=4, af_new_items=paths, af_warm_items=str(warm), fold_steps=7, fold_negatives=2, init_seed=1)
    tail = "2-batch_16-K_6.tsv"
    for best in ("", "best-"):
        base = str(tmp_path / (best + "recs-" + tail))
        m._store_warm(base)
        m._store_audience(base)
        rows = m.fold_in_items(BUYERS, (ed, col, cl), steps=7, negatives=2, seed=1)
        for name, (ids, vals, att) in (("warm-recs-", m._rank_warm_recs(rows, BUYERS)), ("warm-audience-", m._rank_warm_audience(rows, BUYERS)),
                                       ("audience-", m.audience())):
            want = "".join("%d\t%d\t%s\t%s\t%s\t%s\n" % (r, ids[r, q], str(vals[r, q]), *(str(a) for a in att[r, q]))
                           for r in range(ids.shape[0]) for q in range(ids.shape[1]) if ids[r, q] >= 0)
            text = open(str(tmp_path / (best + name + tail))).read()
            assert text == want and text, name
            assert all(len(l.split("\t")) == 6 for l in text.splitlines())
    m0, _ = _model(monkeypatch)                                  # the flags off: no file
    m0._store_warm(str(tmp_path / ("recs-off-" + tail)))
    m0._store_audience(str(tmp_path / ("recs-off-" + tail)))
    assert not [f for f in os.listdir(tmp_path) if "off" in f]


# ---- the restatement against finite differences of its own loss -----------------------------------------------------------------
def test_the_restated_gradient_is_the_derivative_of_the_restated_loss():
    rs = np.random.RandomState(4)
    U, I, k, h, n = 7, 6, 5, 4, 9
    Gu, Gi = rs.standard_normal((U, k)), rs.standard_normal((I, k))
    C, c_r = rs.standard_normal((3, I, k)), rs.standard_normal((3, k))
    att = (rs.standard_normal((k, h)), rs.standard_normal(h), rs.standard_normal((h, 1)), rs.standard_normal(1))
    user, other, role = rs.randint(U, size=n), rs.randint(I, size=n), rs.randint(2, size=n)
    D, dc = R.pair_terms(Gu, Gi, C, att, c_r, user, other, role)
    w = rs.standard_normal(k)
    # x_p = w.D_p + dc_p is s_p (x_ur - x_uo) of the model's own score, computed the long way
    al_r = R.attention(Gu[user], np.broadcast_to(c_r[:, None, :], (3, n, k)), att)
    x_r = (Gu[user] * (al_r[:, :, None] * c_r[:, None, :]).sum(0) * w).sum(1)
    x_o = R.scores(Gu, att, C, Gi)[0][user, other]
    s = np.where(role == 0, 1.0, -1.0)
    assert np.allclose(D @ w + dc, s * (x_r - x_o), rtol=1e-12, atol=1e-13)
    flip = R.pair_terms(Gu, Gi, C, att, c_r, user, other, 1 - role)
    assert np.array_equal(flip[0], -D) and np.array_equal(flip[1], -dc)          # role 1 is a sign flip of role 0
    rv = np.full(k, float(n))
    loss, g = IR.loss_and_grad(w, D, dc, rv, 0.05)
    for c in range(k):
        e = np.zeros(k)
        e[c] = 1e-6
        fd = (IR.loss_and_grad(w + e, D, dc, rv, 0.05)[0] - IR.loss_and_grad(w - e, D, dc, rv, 0.05)[0]) / 2e-6
        assert abs(fd - g[c]) <= 1e-7 * max(1.0, abs(g[c])), (c, fd, g[c])
    # the step loop: sgd moves the row by -lr g, and loss is loss_T before the last update
    ptr = np.array([0, n, n], np.int64)
    r1 = R.fold_in_items(Gu, Gi, C, att, np.stack([c_r, c_r], 1), ptr, user, other, role, np.stack([w, w]), 1, 0.01, 0.05)
    assert np.allclose(r1["Gi"][0], w - 0.01 * g, rtol=1e-6, atol=1e-7) and np.isclose(r1["loss"][0], loss, rtol=1e-6)
    assert np.allclose(r1["Gi"][1], w, rtol=1e-7) and r1["loss"][1] == 0           # no pairs: the row stays, loss 0


# ---- what the GPU test relies on in its inputs ----------------------------------------------------------------------------------
@pytest.mark.parametrize("k,h", K.WIDTHS)
def test_input_preconditions(k, h):
    """On the host encodings of attentive_ref.AttentiveRef.encode: the float64 loss falls for every item with pairs; the float32
    restatement stays within 5e-6 of float64 on the compared entries (sgd: every entry; Adam: the kept ones, at most 5 % left out);
    a fit with alpha = 1/3 leaves the true one by at least 10 x the allowance for at least half the items with pairs."""
    c = K.case(k, h)
    args = (c["t"], c["C"], c["Cn"], c["ptr"], c["user"], c["other"], c["role"], c["W0"])
    has = np.diff(c["ptr"]) > 0
    assert c["ptr"][K.BIG + 1] - c["ptr"][K.BIG] == 3000 and not has[0] and has[1:].all()
    for name, hp in (("sgd", K.SGD), ("adam", K.ADAM)):
        r64, r32, runi = K.restate(*args, hp), K.restate(*args, hp, np.float32), K.restate(*args, hp, uniform_alpha=True)
        assert (r64["loss"][has] < r64["loss_first"][has]).all(), name
        dev = np.abs(r32["Gi"].astype(np.float64) - r64["Gi"])
        if name == "adam":
            keep, left = K.adam_keep(r64, c["ptr"])
            dev = np.where(keep, dev, 0.0)
            print("adam k=%d h=%d: left out %.2f %%" % (k, h, 100 * left))
            assert left <= 0.05, left
        d32 = float(dev.max())
        allow = max(32.0 * d32, float(np.spacing(np.float32(np.abs(r64["Gi"]).max()))))
        uni = np.abs(runi["Gi"] - r64["Gi"]).max(1)
        share = float((uni[has] >= 10.0 * allow).mean())
        print("%s k=%d h=%d: float32 deviation %.3e / allowance %.3e / alpha = 1/3 leaves the fit by (median) %.3e, >= 10 x allowance "
              "for %.0f %% of the items" % (name, k, h, d32, allow, np.median(uni[has]), 100 * share))
        assert d32 <= 5e-6, (name, d32)
        assert share >= 0.5, (name, share)
