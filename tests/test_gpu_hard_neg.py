"""Hard negatives on the device (bprx_sample_philox_hard / bprx_sample_epoch_hard / bprx_hard_snapshot) against the numpy twin of
tests/hard_neg_ref.py, over the shapes of tests/hard_neg_cases.py, five steps in lockstep: before every batch the tables and the
sampler's snapshot are read, the batch is drawn with its candidates and scores, checked, and stepped on.

  draw     cand_out is the twin's, bit for bit; u and i are the uniform stream's
  scores   |score_out - scores64| <= 4 (k + d + 2) 2^-24 magnitude, entry by entry: the fp32 dot-product bound (n 2^-24 sum|a_i b_i|
           for any order of n terms), with a factor 4 for the bias adds and fused or unfused products
  choice   neg == cand_out[b, choose(score_out[b])] EXACTLY: the device is held to the numbers it says it compared
  again    the same position without cand_out / score_out gives the same negatives
"""
import ctypes as C
import functools
import glob
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

import hard_neg_cases as cases
import hard_neg_ref as ref
from fashionvisualexpl_recommend_amd import _ffi, configs, synth
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
STEPS = 5
E_INVALID, E_STATE = -1, -2
MODELS = [("k1", None), ("dense", None), ("plane9", None), ("fallback", None), ("odd", "fp32"), ("odd", "bf16"),
          ("bench", "fp32"), ("bench", "bf16"), ("bench", "fp8")]
MODEL_IDS = ["%s-%s" % (n, dt or "bprmf") for n, dt in MODELS]


def _sampler(kind, lists, I):
    from fashionvisualexpl_recommend_amd.engine import EpochWalkSampler, PhiloxSampler
    return (EpochWalkSampler if kind == "epoch" else PhiloxSampler)(lists, I, seed=cases.SEED)


def _engine(name, dtype, opt, adam_form=None, lr=None):
    from fashionvisualexpl_recommend_amd.engine import Engine
    U, I, k, d, _, B = cases.SHAPES[name]
    t = cases.tables_of(name)
    kw = dict(model="bprmf")
    if dtype is None:
        t = {n: t[n] for n in ("Gu", "Gi", "Bi")}
    else:
        kw = dict(model="vbpr", embed_d=d, feat_dim=cases.FEAT_DIM[name], feat_dtype=dtype)
    lr = lr if lr is not None else (0.05 if opt == "sgd" else 5e-3)
    e = Engine(num_users=U, num_items=I, embed_k=k, optimizer=opt, lr=lr, reg=1e-3, max_batch=B, adam_form=adam_form, **kw)
    return e.bind(**t), t


@functools.lru_cache(maxsize=None)
def _twin(name, kind, position):
    """(u, i, cand) of the batch at `position`: the same for every model and optimizer of a shape, computed once."""
    U, I, _, _, C_, B = cases.SHAPES[name]
    out = ref.stream(cases.lists_of(name), I, cases.SEED, position, B, C_, kind)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _sets(name):
    return [frozenset(l) for l in cases.lists_of(name)]


def _np(x):
    return x.detach().cpu().numpy().copy()


def _lockstep(name, dtype, kind, e, exact_rows):
    """The five steps.  exact_rows: the stored rows are engine.t's (sgd, adam_tf23 by sweeps): the scores are checked too."""
    U, I, k, d, C_, B = cases.SHAPES[name]
    d = d if dtype else 0
    smp = _sampler(kind, cases.lists_of(name), I).hard(e, C_)
    sets = _sets(name)
    fell_back = 0
    for step in range(STEPS):
        if step == 3:
            smp.refresh()                                        # a second snapshot, of the tables three steps on
        t = {n: _np(e.t[n]) for n in (("Gu", "Gi", "Bi", "Tu") if d else ("Gu", "Gi", "Bi"))} if exact_rows else None
        pos = smp.position
        u, i, j, cand, score = smp.sample(B, want_candidates=True)
        Ps = _np(smp.snapshot) if d else None
        assert (smp.snapshot is None) == (d == 0)
        wu, wi, wcand = _twin(name, kind, pos)
        un, inn, jn, cn, sn = _np(u), _np(i), _np(j), _np(cand), _np(score)
        np.testing.assert_array_equal(cn, wcand, err_msg="cand, step %d" % step)                       # 1 draw
        np.testing.assert_array_equal(un, wu, err_msg="u, step %d" % step)
        np.testing.assert_array_equal(inn, wi, err_msg="i, step %d" % step)
        if exact_rows:                                                                                  # 2 scores
            want = ref.scores64(t, Ps, un, cn, d)
            bound = 4 * (k + d + 2) * 2.0 ** -24 * ref.magnitude(t, Ps, un, cn, d)
            err = np.abs(sn.astype(np.float64) - want)
            print("%s %s %s step %d: max score error / bound = %.3g" % (name, dtype, kind, step, (err / np.maximum(bound, 1e-300)).max()))
            assert (err <= bound).all(), (step, float(err.max()), float(bound[err > bound].min()))
        best = ref.choose(sn)                                                                           # 3 choice
        np.testing.assert_array_equal(jn, cn[np.arange(B), best], err_msg="neg, step %d" % step)
        bad = [b for b in range(B) if jn[b] in sets[un[b]]]                                            # 4 never a positive
        assert not bad, (step, len(bad), un[bad[0]], jn[bad[0]])
        smp.seek(pos)
        u2, i2, j2 = smp.sample(B)                                                                      # 3 ... and again, bare
        assert torch.equal(j2, j) and torch.equal(u2, u) and torch.equal(i2, i), step
        assert smp.position == pos + B
        if name == "fallback":
            fell_back += int((un == 0).sum())
        loss = e.step(u2, i2, j2)
        assert np.isfinite(loss.item()), step
    if name == "fallback" and kind == "philox":
        assert fell_back > B                                     # user 0 (all but one item) owns most of the Philox stream
    e.sync_check()


@pytest.mark.parametrize("opt", ["sgd", "adam_tf23"])
@pytest.mark.parametrize("kind", ["epoch", "philox"])
@pytest.mark.parametrize("name,dtype", MODELS, ids=MODEL_IDS)
def test_draw_scores_and_choice_in_lockstep(monkeypatch, name, dtype, kind, opt):
    monkeypatch.setenv("BPRX_ADAM_LAZY", "0")                    # adam_tf23 by sweeps: the stored rows are the current ones
    e, _ = _engine(name, dtype, opt)
    assert not e.adam_is_lazy()
    _lockstep(name, dtype, kind, e, exact_rows=True)


@pytest.mark.parametrize("kind", ["epoch", "philox"])
@pytest.mark.parametrize("name,dtype", [("k1", None), ("bench", "bf16")], ids=["k1-bprmf", "bench-bf16"])
def test_lazy_adam_rows_are_scored_as_stored(name, dtype, kind):
    """Lazy adam_tf23: rows the batches have not touched lag engine.t, so only the draw, the choice among the scores the device
    reports and the never-a-positive rule are checked."""
    e, _ = _engine(name, dtype, "adam_tf23", adam_form="lazy")
    assert e.adam_is_lazy()
    _lockstep(name, dtype, kind, e, exact_rows=False)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_the_snapshot_is_the_projection_of_the_tables_as_they_are(dtype):
    """Ps = F.[E|Bp] of the tables at the time of refresh(), not the step's working P (whose untouched rows are stale under the
    masked projections): after three steps a new snapshot matches the new E / Bp and the old one does not.  Bound: fp32 features
    are summed in fp64 (one fp32 rounding of the result, here 2^-20 of the magnitude); bf16 rounds E and Bp to 8 bits
    (2^-9 relative each) and sums D products in fp32: 2^-8 of the magnitude."""
    name, kind = "bench", "epoch"
    U, I, k, d, C_, B = cases.SHAPES[name]
    e, _ = _engine(name, dtype, "sgd", lr=0.5)
    smp = _sampler(kind, cases.lists_of(name), I).hard(e, C_)

    def want():
        F, E, Bp = (_np(e.t[n].float()).astype(np.float64) for n in ("F", "E", "Bp"))
        W = np.concatenate([E, Bp[:, None]], 1)
        return F @ W, np.abs(F) @ np.abs(W)
    rel = 2.0 ** -20 if dtype == "fp32" else 2.0 ** -8
    smp.refresh()
    first = _np(smp.snapshot)
    p0, m0 = want()
    assert (np.abs(first[:, :d + 1] - p0) <= rel * m0 + 1e-30).all()
    ptr = smp.snapshot.data_ptr()
    for _ in range(3):
        e.step(*smp.sample(B))
    assert smp.snapshot.data_ptr() == ptr and np.array_equal(_np(smp.snapshot), first)       # nothing but refresh() writes it
    p1, m1 = want()
    if dtype == "fp32":
        assert not (np.abs(first[:, :d + 1] - p1) <= rel * m1 + 1e-30).all()                    # (the model has moved)
    smp.refresh()
    assert smp.snapshot.data_ptr() == ptr and not np.array_equal(_np(smp.snapshot), first)
    assert (np.abs(_np(smp.snapshot)[:, :d + 1] - p1) <= rel * m1 + 1e-30).all()
    e.sync_check()


@pytest.mark.parametrize("kind", ["epoch", "philox"])
@pytest.mark.parametrize("name,dtype", MODELS[:-1], ids=MODEL_IDS[:-1])
def test_one_candidate_is_the_uniform_stream(name, dtype, kind):
    U, I, _, _, _, B = cases.SHAPES[name]
    e, _ = _engine(name, dtype, "sgd")
    lists = cases.lists_of(name)
    hard, plain = _sampler(kind, lists, I).hard(e, 1), _sampler(kind, lists, I)
    for step in range(STEPS):                                    # (the epoch walk crosses an epoch boundary on the way)
        got, want = hard.sample(B), plain.sample(B)
        for g, w, what in zip(got, want, "uij"):
            assert torch.equal(g, w), (what, step)
    e.sync_check()


@pytest.mark.parametrize("kind", ["epoch", "philox"])
@pytest.mark.parametrize("name", ["dense", "plane9"])
def test_a_hard_sampler_feeds_the_step_like_a_uniform_one(monkeypatch, name, kind):
    """Segment mode (BPRX_ITEM_MODE=2): the index pass of a step fed by the hard sampler reads what it reads on a twin engine fed
    by the uniform sampler (the byte planes at both shapes: shift 8 at 37 items, shift 9 at 65 537; the owner queues where the
    twin reads them), and the step is the oracle's step on the hard triplets, within the tolerances of
    test_byte_plane_shift_edges_against_the_oracle, the batch that crosses the epoch boundary included."""
    monkeypatch.setenv("BPRX_ITEM_MODE", "2")
    U, I, k, _, C_, B = cases.SHAPES[name]
    lr, reg = 0.05, 1e-3
    e, t = _engine(name, None, "sgd", lr=lr)
    e2, _ = _engine(name, None, "sgd", lr=lr)
    o = orc.OracleModel(**t, quant=0)
    lists = cases.lists_of(name)
    assert B < sum(len(l) for l in lists) < 4 * B
    hard, plain = _sampler(kind, lists, I).hard(e, C_), _sampler(kind, lists, I).feeds(e2)
    differs = 0
    for step in range(STEPS):
        u, i, j = hard.sample(B)
        pu, pi, pj = plain.sample(B)
        differs += int((j != pj).sum())
        loss = e.step(u, i, j).item()
        e2.step(pu, pi, pj)
        kinds = [(x.lib.bprx_index_pass_kind(x.h), x.lib.bprx_index_pass_queue(x.h)) for x in (e, e2)]
        assert kinds[0] == kinds[1] and kinds[0][0] == 2, (step, kinds)
        want = o.step(_np(u), _np(i), _np(j), "sgd", lr, reg)
        assert loss == pytest.approx(want, rel=2e-5), step
        for n in ("Gu", "Gi", "Bi"):
            np.testing.assert_allclose(_np(e.t[n]).reshape(-1), getattr(o, n).reshape(-1), rtol=2e-5, atol=2e-6,
                                       err_msg="%s %d" % (n, step))
    assert differs > 0                                           # (the hard stream is another stream)
    e.sync_check()
    e2.sync_check()


@pytest.mark.parametrize("kind", ["epoch", "philox"])
def test_planes_of_a_vbpr_step_fed_by_the_hard_sampler(monkeypatch, kind):
    monkeypatch.setenv("BPRX_ITEM_MODE", "2")
    name = "bench"
    U, I, _, _, C_, B = cases.SHAPES[name]
    e, _ = _engine(name, "bf16", "sgd")
    e2, _ = _engine(name, "bf16", "sgd")
    lists = cases.lists_of(name)
    hard, plain = _sampler(kind, lists, I).hard(e, C_), _sampler(kind, lists, I).feeds(e2)
    for step in range(STEPS):
        assert np.isfinite(e.step(*hard.sample(B)).item())
        e2.step(*plain.sample(B))
        kinds = [(x.lib.bprx_index_pass_kind(x.h), x.lib.bprx_index_pass_queue(x.h), x.lib.bprx_proj_mask_kind(x.h)) for x in (e, e2)]
        assert kinds[0] == kinds[1] and kinds[0][0] == 2, (step, kinds)
    e.sync_check()


@pytest.mark.parametrize("name,dtype", [("k1", None), ("bench", "bf16")], ids=["k1-bprmf", "bench-bf16"])
def test_the_chosen_negative_scores_at_least_the_uniform_one(name, dtype):
    """After two epochs of uniform training: score_out[b, chosen] >= score_out[b, 0] for every triplet, on the device's own
    numbers, and for some triplets it is larger (the hard sampler is not the uniform one)."""
    U, I, _, _, C_, B = cases.SHAPES[name]
    e, _ = _engine(name, dtype, "sgd", lr=0.1)
    lists = cases.lists_of(name)
    plain = _sampler("epoch", lists, I).feeds(e)
    for _ in range(2 * sum(len(l) for l in lists) // B):
        e.step(*plain.sample(B))
    hard = _sampler("epoch", lists, I).hard(e, C_)
    u, i, j, cand, score = hard.sample(B, want_candidates=True)
    cn, sn, jn = _np(cand), _np(score), _np(j)
    chosen = ref.choose(sn)
    np.testing.assert_array_equal(jn, cn[np.arange(B), chosen])
    top = sn[np.arange(B), chosen]
    assert (top >= sn[:, 0]).all() and (top == sn.max(1)).all()
    assert (top > sn[:, 0]).sum() > B // 4


# ---- errors ------------------------------------------------------------------------------------------------------------------
def _call(e, smp, B, candidates, ps, epoch=False):
    from fashionvisualexpl_recommend_amd.engine import _ptr, _stream
    u, i, j = (torch.zeros(B, dtype=torch.int32, device="cuda") for _ in range(3))
    lib = e.lib
    if epoch:
        if getattr(smp, "perm", None) is None:
            smp._start_epoch(0)
        return lib.bprx_sample_epoch_hard(e.h, _ptr(smp.indptr), _ptr(smp.items), _ptr(smp.perm), _ptr(smp.epoch_ptr), _ptr(smp.pos_slot),
                                          smp.indptr.numel() - 1, smp.num_items, smp.seed, 0, 0, B, _ptr(u), _ptr(i), _ptr(j), 0, B,
                                          _stream(), candidates, _ptr(ps), None, None)
    return lib.bprx_sample_philox_hard(e.h, _ptr(smp.indptr), _ptr(smp.items), _ptr(smp.pos_user), smp.num_pos, smp.num_items, smp.seed,
                                       0, B, _ptr(u), _ptr(i), _ptr(j), 0, B, _stream(), candidates, _ptr(ps), None, None)


def _last_error(e):
    return e.lib.bprx_last_error(e.h).decode()


@pytest.mark.parametrize("epoch", [False, True], ids=["philox", "epoch"])
def test_errors_leave_the_handle_usable(epoch):
    from fashionvisualexpl_recommend_amd.engine import Engine, _stream
    name = "odd"
    U, I, k, d, C_, B = cases.SHAPES[name]
    lists = cases.lists_of(name)
    smp = _sampler("epoch" if epoch else "philox", lists, I)
    t = cases.tables_of(name)
    e = Engine(model="vbpr", num_users=U, num_items=I, embed_k=k, embed_d=d, feat_dim=cases.FEAT_DIM[name], feat_dtype="bf16",
               optimizer="sgd", lr=0.05, reg=1e-3, max_batch=B)
    ps = torch.zeros((I, 16), dtype=torch.float32, device="cuda")
    assert _call(e, smp, B, 4, ps, epoch) == E_STATE and "not bound" in _last_error(e)                   # unbound
    assert e.lib.bprx_hard_snapshot(e.h, C.c_void_p(ps.data_ptr()), _stream()) == E_STATE
    e.bind(**t)
    assert e.proj_stride() == 16
    for cands in (0, 17, -1):
        assert _call(e, smp, B, cands, ps, epoch) == E_INVALID and "candidates" in _last_error(e)
    assert _call(e, smp, B, 4, None, epoch) == E_INVALID and "snapshot" in _last_error(e)             # VBPR without Ps
    assert e.lib.bprx_hard_snapshot(e.h, None, _stream()) == E_INVALID
    hard = _sampler("epoch" if epoch else "philox", lists, I).hard(e, 4)                                 # ... and still works
    assert np.isfinite(e.step(*hard.sample(B)).item())
    e.sync_check()
    with pytest.raises(ValueError):
        smp.sample(B, want_candidates=True)                      # not a hard sampler


def test_bprmf_needs_no_snapshot():
    from fashionvisualexpl_recommend_amd.engine import _stream
    e, _ = _engine("k1", None, "sgd")
    assert e.lib.bprx_hard_snapshot(e.h, None, _stream()) == 0
    hard = _sampler("philox", cases.lists_of("k1"), cases.SHAPES["k1"][1]).hard(e, 2)
    hard.refresh()
    assert hard.snapshot is None
    hard.sample(64)
    e.sync_check()


def test_acf_and_attentive_handles_are_refused():
    from acf_ref import random_tables as acf_tables
    from attentive_ref import AF_WEIGHTS, random_inputs
    from attentive_ref import random_tables as af_tables
    from fashionvisualexpl_recommend_amd.engine import Engine, _stream
    U, I, K, B = 40, 48, 8, 32
    rs = np.random.RandomState(3)
    lists = [sorted(rs.choice(I, 1 + u % 3, replace=False).tolist()) for u in range(U)]
    mk = lambda: Engine(model="bprmf", num_users=U, num_items=I, embed_k=K, optimizer="sgd", lr=0.05, reg=1e-3, max_batch=64)
    t = acf_tables(rs, U, I, K, 8, 8, 8)
    F = np.abs(rs.standard_normal((I, 4, 8))).astype(np.float32)
    acf = mk().bind_acf(t["Gu"], t["Gi"], t["Bi"], F, t["Pi"], {n: t[n] for n in _ffi.ACF_WEIGHTS}, lists)
    ta = af_tables(np.random.RandomState(4), U, I, K, 5, 3, 8)
    af = mk().bind_attentive(ta["Gu"], ta["Gi"], ta["Bi"], *random_inputs(np.random.RandomState(9), I, 5, 3),
                             {n: ta[n] for n in AF_WEIGHTS}, dropout=0.5, seed=7)
    for e in (acf, af):
        for epoch in (False, True):
            smp = _sampler("epoch" if epoch else "philox", lists, I)
            assert _call(e, smp, B, 4, None, epoch) == E_INVALID and "ACF" in _last_error(e)
        assert e.lib.bprx_hard_snapshot(e.h, None, _stream()) == E_INVALID
        u, i, j = _sampler("philox", lists, I).sample(B)
        assert np.isfinite(e.step(u, i, j).item())               # the handle still steps
        e.sync_check()


# ---- the CLI -----------------------------------------------------------------------------------------------------------------
def _dataset(tmp_path, name, features=False):
    tr, va, te = synth.make_interactions_clustered(300, 500, per_user=14, clusters=10, p_in=0.9, seed=7)
    feats = np.abs(np.random.RandomState(1).standard_normal((500, 128))).astype(np.float32) if features else None
    synth.write_dataset(str(tmp_path), name, tr, va, te, 500, features=feats)


@pytest.mark.parametrize("rec,extra", [("bprmf", []), ("vbpr", ["--embed_d", "8", "--dtype", "bf16"])])
def test_cli_trains_on_hard_negatives_and_names_its_files(tmp_path, rec, extra):
    from fashionvisualexpl_recommend_amd import train_rec
    _dataset(tmp_path, "hn", features=rec == "vbpr")
    argv = ["--dataset", "hn", "--rec", rec, "--batch_size", "128", "--epochs", "3", "--embed_k", "16", "--lr", "0.01", "--top_k", "10",
            "--sampler", "philox", "--data_root", str(tmp_path), "--results_root", str(tmp_path / "res")] + extra
    res = train_rec.train(argv + ["--hard_negatives", "4", "--hard_refresh", "7"])[0]
    assert sorted(res) == [1, 2, 3]
    assert all(np.isfinite(v) for r in res.values() for v in r.values()) and {"hr_t", "ndcg_t", "auc_t"} <= set(res[3])
    rdir = os.path.join(configs.results_dir(), "hn", rec)
    wdir = os.path.join(configs.weight_dir(), "hn", rec)
    reg = glob.glob(os.path.join(rdir, "recs-3-*.tsv"))
    assert len(reg) == 1 and reg[0].endswith("-hard_4.tsv")
    tag = os.path.basename(reg[0])[len("recs-3-"):-len("-hard_4.tsv")]
    assert tag.startswith("batch_128-") and os.path.exists(os.path.join(rdir, "results-metrics-%s-hard_4.pkl" % tag))
    assert glob.glob(os.path.join(wdir, "best-weights-*-%s-hard_4.pt" % tag))
    train_rec.train(argv)
    assert os.path.exists(os.path.join(rdir, "recs-3-%s.tsv" % tag)) and os.path.exists(os.path.join(rdir, "results-metrics-%s.pkl" % tag))
    assert len(glob.glob(os.path.join(rdir, "recs-3-*.tsv"))) == 2


@pytest.mark.parametrize("opt,lr", [("adam_tf23", 5e-3), ("sgd", 0.5)])
def test_a_resumed_hard_run_continues_the_same_run(tmp_path, opt, lr):
    """A run interrupted after epoch 2 and resumed (the stream position skipped, not sampled; the snapshot taken at the epoch's
    start) ends where the uninterrupted 4-epoch run ends: the tolerances of test_resume_continues_the_same_run."""
    from fashionvisualexpl_recommend_amd.dataset import DataLoader
    from fashionvisualexpl_recommend_amd.models import BPRMF
    _dataset(tmp_path, "hnr")
    configs.set_roots(str(tmp_path), str(tmp_path / "results"))

    def params(epochs, restore):
        return Namespace(dataset="hnr", validation=True, batch_size=128, epochs=epochs, batch_eval=128, embed_k=16, lr=lr,
                         reg=1e-3, top_k=10, verbose=2, restore_epochs=restore, rec="bprmf", best_metric="ndcg",
                         optimizer=opt, init_seed=0, sampler="philox", hard_negatives=4, hard_refresh=5)
    full = BPRMF(DataLoader(params(4, 1)), params(4, 1))
    assert full.directory_parameters.endswith("-hard_4")
    res_full = full.train()
    BPRMF(DataLoader(params(2, 1)), params(2, 1)).train()            # writes weights-2-*.pt (verbose=2)
    second = BPRMF(DataLoader(params(4, 2)), params(4, 2))
    res = second.train(resume=True)
    assert sorted(res) == [3, 4]
    if opt == "adam_tf23":
        assert second.engine.adam_step == full.engine.adam_step
    for n in ("Gu", "Gi", "Bi"):
        np.testing.assert_allclose(_np(second.engine.t[n]), _np(full.engine.t[n]), rtol=1e-4, atol=1e-5, err_msg=n)
    for key in ("hr_t", "ndcg_t", "auc_t"):
        assert abs(res[4][key] - res_full[4][key]) <= 1e-3
