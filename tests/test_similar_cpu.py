"""Similar items without a GPU: the binding and the library's exports, the command line, the lists and the file of
BPRMF.similar_items / Evaluator.store_similar_items over a stub engine (in the manner of tests/test_ranking_cpu.py: determined
rows answered with the unique list, every other row flagged and POISONED, so a flagged row's kernel output must not be read),
and tests/similar_ref.py against a plain double loop."""
import io
import os
import re
from argparse import Namespace

import numpy as np
import pytest
import torch

import similar_ref as S
import topk_ref as tr
from fashionvisualexpl_recommend_amd import _ffi, models, ranking, train_rec

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- binding and exports -------------------------------------------------------------------------------------------------------
def test_the_binding_declares_and_the_library_exports_the_two_entries():
    header = open(os.path.join(REPO, "include", "bprx.h")).read()
    lib = _ffi.lib()
    for name, nargs in (("bprx_sim_rnorm", 6), ("bprx_sim_block", 10)):
        assert name in _ffi.EXPORTS
        assert re.search(r"BPRX_API int %s\(" % name, header), name
        fn = getattr(lib, name)                               # AttributeError: the library does not export it
        assert len(fn.argtypes) == nargs
    for space, value in _ffi.SIM_SPACE.items():
        assert re.search(r"#define BPRX_SIM_%s %d\b" % (space.upper(), value), header), space
    assert sorted(_ffi.SIM_SPACE) == sorted(S.SPACES) and "#define BPRX_ABI_VERSION 6" in header and _ffi.ABI_VERSION == 6
    # a NULL handle is rejected before anything is read
    assert lib.bprx_sim_rnorm(None, 0, None, 0, None, None) == _ffi.E_INVALID
    assert lib.bprx_sim_block(None, 0, None, 0, 0, 0, None, None, None, None) == _ffi.E_INVALID


# ---- command line --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("argv", [
    ["--rec", "acf", "--similar_items", "5"],
    ["--rec", "attentive_fashion", "--similar_items", "5"],
    ["--rec", "acf", "--similar_space", "latent"],
    ["--rec", "bprmf", "--similar_items", "5", "--similar_space", "visual"],
    ["--rec", "bprmf", "--similar_items", "5", "--similar_space", "both"],
    ["--rec", "vbpr", "--dtype", "fp8", "--similar_items", "5"],
    ["--rec", "vbpr", "--dtype", "fp8", "--similar_items", "5", "--similar_space", "both"],
    ["--rec", "grad_fashion", "--dtype", "fp8", "--similar_items", "5", "--similar_space", "visual"],
    ["--rec", "vbpr", "--similar_items", "-1"],
    ["--rec", "vbpr", "--similar_items", "1025"],
    ["--rec", "vbpr", "--similar_items", "5", "--similar_space", "pixels"],
], ids=lambda a: " ".join(a))
def test_parse_args_rejects(argv, capsys):
    with pytest.raises(SystemExit):
        train_rec.parse_args(argv)
    assert "similar" in capsys.readouterr().err


def test_parse_args_defaults_by_model():
    for rec, space in (("bprmf", "latent"), ("vbpr", "visual"), ("grad_fashion", "visual")):
        a = train_rec.parse_args(["--rec", rec])
        assert a.similar_items == 0 and a.similar_space == space
        assert train_rec.parse_args(["--rec", rec, "--similar_items", "1024"]).similar_space == space
    assert train_rec.parse_args(["--rec", "acf"]).similar_space is None
    assert train_rec.parse_args(["--rec", "vbpr", "--dtype", "fp8"]).similar_items == 0        # off: fp8 trains as before
    a = train_rec.parse_args(["--rec", "vbpr", "--dtype", "fp8", "--similar_items", "7", "--similar_space", "latent"])
    assert (a.similar_items, a.similar_space) == (7, "latent")
    assert train_rec.parse_args(["--rec", "vbpr", "--similar_items", "1", "--similar_space", "both"]).similar_space == "both"
    with pytest.raises(NotImplementedError, match="similar_items"):
        train_rec.train(["--rec", "vbpr", "--similar_items", "5", "--world_size", "2"])


# ---- lists and file over a stub engine -----------------------------------------------------------------------------------------
class _StubEngine:
    """The four engine calls similar_items makes, on the CPU: float32 cosines of Gi from similar_ref, the top-K entry of
    tests/test_ranking_cpu.py (masks IN the scores; undetermined rows come back flagged with idx -1 / val nan)."""
    device = "cpu"

    def __init__(self, **kw):
        self.kw, self.blocks, self.flags = kw, [], []

    def bind(self, **t):
        self.t = t
        return self

    def csr(self, lists):
        return [list(l) for l in lists]

    def sim_rnorm(self, space):
        assert space == "latent"
        return torch.from_numpy(S.rnorm(self.t["Gi"], torch.float32))

    def sim_block(self, space, q0, q1, rn_items):
        assert space == "latent" and np.array_equal(rn_items.numpy(), S.rnorm(self.t["Gi"], torch.float32))
        self.blocks.append((q0, q1))
        return torch.from_numpy(S.cosine(self.t["Gi"], torch.float32)[q0:q1].copy())

    def topk_lists(self, scores, own, k):
        s = scores.numpy()
        n, I = s.shape
        assert len(own) == n and [len(l) for l in own] == [1] * n
        for r, l in enumerate(own):
            s[r, l] = -np.inf
        idx, val, flag = np.full((n, k), -1, np.int32), np.full((n, k), np.nan, np.float32), np.ones(n, np.int32)
        for r in range(n):
            if tr.classify(s[r], k, I - 1) == tr.DETERMINED:
                idx[r] = tr.unique_topk(s[r], k)
                val[r], flag[r] = s[r][idx[r]], 0
        self.flags.append((own[0][0], flag.copy()))
        return torch.from_numpy(idx), torch.from_numpy(val), torch.from_numpy(flag)


I_ITEMS = 40


def _model(monkeypatch, **over):
    monkeypatch.setattr(models, "Engine", _StubEngine)
    rs = np.random.RandomState(11)
    Gi = rs.standard_normal((I_ITEMS, 6)).astype(np.float32)
    Gi[19] = Gi[7]                                            # twins: every other row holds a pair of equal cosines
    Gi[5] = 0                                                 # a zero row: 0.0 to everything
    p = dict(epochs=1, batch_size=16, embed_k=6, lr=0.001, reg=0, top_k=3, dataset="toy", rec="bprmf", optimizer="sgd", init_seed=0)
    p.update(over)
    data = Namespace(num_users=4, num_items=I_ITEMS, training_list=[[0]] * 4, validation_list=[], test_list=[],
                     params=Namespace(batch_eval=128))
    m = models.BPRMF(data, Namespace(**p), init={"Gi": Gi})
    m.evaluator.user_block = 16                               # three blocks of item rows: 16, 16, 8
    return m, Gi


def _reference_lists(Gi, k):
    """numpy_topk on every masked float32 row, cut to min(k, I - 1): the list whether or not the kernel flags the row."""
    sc = S.cosine(Gi, torch.float32).copy()
    sc[np.arange(I_ITEMS), np.arange(I_ITEMS)] = -np.inf
    kk = min(k, I_ITEMS - 1)
    ids = np.stack([ranking.numpy_topk(sc[r], k)[:kk] for r in range(I_ITEMS)]).astype(np.int64)
    return ids, np.take_along_axis(sc, ids, axis=1), sc


@pytest.mark.parametrize("k", [5, I_ITEMS - 1, I_ITEMS, 64])
def test_similar_items_lists(monkeypatch, k):
    m, Gi = _model(monkeypatch, similar_items=k)
    assert m.similar_k == k and m.similar_space == "latent"
    ids, vals = m.similar_items()
    wid, wval, sc = _reference_lists(Gi, k)
    kk = min(k, I_ITEMS - 1)
    assert ids.shape == vals.shape == (I_ITEMS, kk) and ids.dtype == np.int64 and vals.dtype == np.float32
    assert not (ids == np.arange(I_ITEMS)[:, None]).any(), "an item lists itself"
    assert np.array_equal(ids, wid) and np.array_equal(vals.view(np.uint32), wval.view(np.uint32))
    assert not np.isnan(vals).any() and np.isfinite(vals).all()
    assert m.engine.blocks == [(0, 16), (16, 32), (32, 40)]
    flag = np.concatenate([f for _, f in m.engine.flags])
    if k == 5:                                                # both kinds of row: the twins make ties, most rows have none inside 5
        assert 0 < flag.sum() < I_ITEMS and flag[5] == 1      # (the zero row: 39 equal cosines)
        r = int(np.nonzero(flag)[0][0])
        assert np.array_equal(ids[r], ranking.numpy_topk(sc[r], k))      # a flagged row: numpy_topk on the masked row
    elif k >= I_ITEMS:
        assert flag.all()                                     # fewer than k unmasked entries, or k > I
    else:                                                     # the whole row: only the twins' own rows hold no equal pair
        assert np.array_equal(np.nonzero(flag == 0)[0], [7, 19])
    assert ids[7, 0] == 19 and ids[19, 0] == 7 and (vals[5] == 0.0).all()
    # an explicit id list: the blocks that hold the ids are ranked, those rows kept, in the order asked for
    m.engine.blocks.clear()
    i2, v2 = m.similar_items([33, 2, 2, 39], k=k)
    assert m.engine.blocks == [(0, 16), (32, 40)]
    assert np.array_equal(i2, wid[[33, 2, 2, 39]]) and np.array_equal(v2.view(np.uint32), wval[[33, 2, 2, 39]].view(np.uint32))
    assert m.similar_items([], k=k)[0].shape == (0, kk)
    with pytest.raises(ValueError):
        m.similar_items([I_ITEMS])


def test_store_similar_items_bytes(monkeypatch, tmp_path):
    m, Gi = _model(monkeypatch, similar_items=5)
    wid, wval, _ = _reference_lists(Gi, 5)
    want = io.StringIO()
    ranking.write_ranked(want, range(I_ITEMS), wid, wval)
    path = str(tmp_path / "sim-1-x.tsv")
    m.evaluator.store_similar_items(path, "latent")
    assert open(path, "rb").read() == want.getvalue().encode()
    rows = [l.split("\t") for l in want.getvalue().splitlines()]
    assert len(rows) == I_ITEMS * 5 and all(len(r) == 3 and r[0] != r[1] for r in rows)
    # what train() writes: sim-* next to recs-*, best-sim-* next to best-recs-*; nothing with the flag off
    for f in ("recs-2-x.tsv", "best-recs-1-x.tsv"):
        m._store_similar(str(tmp_path / f))
        assert open(str(tmp_path / f.replace("recs-", "sim-", 1)), "rb").read() == want.getvalue().encode()
    off, _ = _model(monkeypatch)
    assert off.similar_k == 0
    off._store_similar(str(tmp_path / "recs-9-x.tsv"))
    assert not os.path.exists(str(tmp_path / "sim-9-x.tsv"))


# ---- the reference against a double loop ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("space", S.SPACES)
def test_similar_ref_against_a_double_loop(space):
    rs = np.random.RandomState(3)
    I, k, d, D = 6, 3, 2, 5
    t = dict(Gi=rs.standard_normal((I, k)).astype(np.float32), F=rs.standard_normal((I, D)).astype(np.float32),
             E=rs.standard_normal((D, d)).astype(np.float32), Bp=rs.standard_normal(D).astype(np.float32))
    t["Gi"][4], t["F"][4] = 0, 0                               # a zero row in every space
    z = S.item_vectors(t, space, "fp32", torch.float64)
    parts = ([t["Gi"].astype(np.float64)] if space != "visual" else []) + \
            ([t["F"].astype(np.float64) @ t["E"].astype(np.float64)] if space != "latent" else [])
    assert z.dtype == np.float64 and np.allclose(z, np.concatenate(parts, 1), rtol=1e-14, atol=0)
    want = np.zeros((I, I))
    for q in range(I):
        for j in range(I):
            nq, nj = sum(x * x for x in z[q]), sum(x * x for x in z[j])
            rq, rj = (1 / np.sqrt(nq) if nq > 0 else 0.0), (1 / np.sqrt(nj) if nj > 0 else 0.0)
            want[q, j] = sum(a * b for a, b in zip(z[q], z[j])) * (rq * rj)
    got = S.cosine(z)
    assert np.allclose(got, want, rtol=1e-13, atol=1e-15)
    assert (got[4] == 0.0).all() and (got[:, 4] == 0.0).all() and not np.isnan(got).any()
    keep = [q for q in range(I) if q != 4]
    assert np.allclose(np.diag(got)[keep], 1.0, rtol=1e-14) and np.allclose(got, got.T, rtol=1e-14, atol=0)
    g32 = S.cosine(S.item_vectors(t, space, "fp32", torch.float32), torch.float32)
    assert g32.dtype == np.float32 and np.abs(g32 - want).max() < 1e-5
    if space == "visual":                                     # rows from outside the catalogue: their own norms, the same scale
        out = S.cosine(z, zq=S.item_vectors(t, "visual", "fp32", torch.float64, F=t["F"][[2, 4]]))
        assert np.allclose(out, want[[2, 4]], rtol=1e-13, atol=1e-15)
        zb = S.item_vectors(t, "visual", "bf16", torch.float64)
        from oracle import oracle as orc
        assert np.allclose(zb, t["F"].astype(np.float64) @ orc.bf16_round(t["E"]).astype(np.float64), rtol=1e-14, atol=0)
