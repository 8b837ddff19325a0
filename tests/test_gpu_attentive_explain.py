"""bprx_af_explain on the MI355X against the float64 restatement (tests/attentive_explain_ref.py): U = 5, I = 8 (item 0 blank, item 1
dense noise, the rest sparse strokes), Dc = 37, Dk = 11, h = 64, k in {16, 128}, random non-zero biases; every item appears, item 3 is
named by four users, user 0 is repeated; grids 1, 7, 14, 16, 112 (7 and 14 put cell borders inside a four-window tile, 112 is one
window per cell); calls of 0, 1 and max_batch pairs; neutrality towards the training state, errors, the workspace, the CLI.

Allowances: for parts, map and peak_val, attentive_explain_ref.TOL_MULT (32) x the max-abs deviation of the SAME restatement run in
float32 on the CPU from the float64 one, over the pairs of the case; nothing is fixed in advance.  Every case prints its triples
(float32 deviation / allowance / GPU deviation).  The two identities on the GPU output itself, sum(parts) against x and
sum(cells) against parts[:, 1], are both held to the allowance of `parts`: both compare quantities of the size of a part, and the
float32 rounding of s_edges alone (about 2e-9 here) is far above the per-cell allowance of a fine grid (4e-11 at G = 112), which no
float32 output could meet.  peak_cell is never compared across precisions: the peak is checked on the returned map, and its value
against the float64 maximum."""
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

import attentive_explain_ref as X
from attentive_ref import AF_WEIGHTS, random_inputs, random_tables
from fashionvisualexpl_recommend_amd import _ffi, synth

pytestmark = pytest.mark.gpu

U, I, DC, DK, H, B = 5, 8, 37, 11, 64, 16
USERS = [0, 1, 2, 3, 4, 0, 1, 2, 0, 1, 2, 4, 3, 3, 4, 1]            # the first 12: the case; all 16: a call of max_batch pairs
ITEMS = [0, 1, 2, 3, 4, 5, 6, 7, 3, 3, 3, 0, 1, 0, 2, 5]            # item 3 by users 3, 0, 1, 2; the blank item 0 by users 0 and 4
N = 12
GRIDS = [1, 7, 14, 16, 112]


def _engine(t, inputs, optimizer="sgd", lr=0.05, reg=0.0, max_batch=B, rate=0.5, seed=7):
    from fashionvisualexpl_recommend_amd.engine import Engine
    e = Engine(model="bprmf", num_users=t["Gu"].shape[0], num_items=t["Gi"].shape[0], embed_k=t["Gu"].shape[1], optimizer=optimizer,
               lr=lr, reg=reg, max_batch=max_batch)
    return e.bind_attentive(t["Gu"], t["Gi"], t["Bi"], *inputs, {n: t[n] for n in AF_WEIGHTS}, dropout=rate, seed=seed)


_CASES = {}


def _case(k):
    """Tables, inputs, an engine and the float64 / float32 restatements of the 16 pairs at G = 112 (computed once, never changed)."""
    if k not in _CASES:
        rs = np.random.RandomState(100 + k)
        t = random_tables(rs, U, I, k, DC, DK, H, bias=True)
        inputs = random_inputs(rs, I, DC, DK)
        r64 = X.explain(t, inputs, USERS, ITEMS, 112, torch.float64)
        r32 = X.explain(t, inputs, USERS, ITEMS, 112, torch.float32)
        _CASES[k] = (t, inputs, _engine(t, inputs), r64, r32)
    return _CASES[k]


def _at_grid(r, G, rows, dtype):
    """The restatement's outputs for the pairs `rows` at grid G (explain() re-bins the same windows in the same dtype)."""
    m = X.rebin(torch.as_tensor(r["windows"][rows]).to(dtype), G).double().numpy()
    return {"parts": r["parts"][rows], "map": m, "peak_val": m.max(1) if len(m) else m.reshape(0)}


def _np(out):
    return {n: v.cpu().numpy() for n, v in out.items()}


def _check(g, e, k, G, rows, tag):
    t, inputs, _, r64, r32 = _case(k)
    users, items = [USERS[r] for r in rows], [ITEMS[r] for r in rows]
    n = len(rows)
    w64, w32 = _at_grid(r64, G, rows, torch.float64), _at_grid(r32, G, rows, torch.float32)
    allow = X.allowances(w64, w32)
    assert g["score"].shape == (n,) and g["alpha"].shape == (n, 3) and g["parts"].shape == (n, 3)
    assert g["map"].shape == (n, G * G) and g["peak_cell"].shape == (n,) and g["peak_val"].shape == (n,)
    assert g["peak_cell"].dtype == np.int32
    dev = {f: float(np.abs(g[f].astype(np.float64) - w64[f]).max()) for f in X.FIELDS}
    for f in X.FIELDS:
        print("%s %-8s fp32 restatement %.3e  allowance %.3e  gpu %.3e" % (tag, f, allow[f] / X.TOL_MULT, allow[f], dev[f]))
    # x and alpha: the bits of bprx_af_attention_pairs
    x, al = e.af_attention_pairs(users, items)
    assert np.array_equal(g["score"].view(np.int32), x.cpu().numpy().view(np.int32)), tag
    assert np.array_equal(g["alpha"].view(np.int32), al.cpu().numpy().view(np.int32)), tag
    # identities on the GPU output itself
    d_parts = float(np.abs(g["parts"].astype(np.float64).sum(1) - g["score"]).max())
    d_cells = float(np.abs(g["map"].astype(np.float64).sum(1) - g["parts"][:, 1]).max())
    print("%s sum(parts) - x %.3e (allowance %.3e)   sum(cells) - s_edges %.3e (allowance %.3e)"
          % (tag, d_parts, allow["parts"], d_cells, allow["parts"]))
    # the peak, on the returned map
    pc = g["peak_cell"].astype(np.int64)
    assert ((pc >= 0) & (pc < G * G)).all(), (tag, pc)
    assert np.array_equal(g["peak_val"].view(np.int32), g["map"][np.arange(n), pc].view(np.int32)), tag
    assert (g["map"] <= g["peak_val"][:, None]).all(), tag
    for r in range(n):                                               # the lowest index among bit-equal cells
        assert pc[r] == int(np.nonzero(g["map"][r] == g["peak_val"][r])[0][0]), (tag, r)
    bad = [(f, dev[f], allow[f]) for f in X.FIELDS if not dev[f] <= allow[f]]
    assert not bad, (tag, bad)
    assert d_parts <= allow["parts"], (tag, "sum of parts", d_parts, allow["parts"])
    assert d_cells <= allow["parts"], (tag, "sum of cells", d_cells, allow["parts"])
    e.sync_check()


@pytest.mark.parametrize("G", GRIDS)
@pytest.mark.parametrize("k", [16, 128])
def test_against_fp64(k, G):
    e = _case(k)[2]
    rows = list(range(N))
    out = e.af_explain(USERS[:N], ITEMS[:N], grid=G)
    g = _np(out)
    _check(g, e, k, G, rows, "k=%d G=%d" % (k, G))
    again = e.af_explain(USERS[:N], ITEMS[:N], grid=G)               # the same arguments: the same bits
    for f in out:
        assert torch.equal(out[f], again[f]), f
    lean = e.af_explain(USERS[:N], ITEMS[:N], grid=G, maps=False)    # without the map: everything else unchanged
    assert "map" not in lean
    for f in lean:
        assert torch.equal(out[f], lean[f]), f
    if G == 112:
        # the blank item: every window has the same A, so every cell holds the same bits whichever wave produced it
        for r in (0, 11):
            assert ITEMS[r] == 0
            assert (g["map"][r].view(np.int32) == g["map"][r, 0].view(np.int32)).all(), r
            assert g["peak_cell"][r] == 0
    # a coarser grid is the finer one re-binned (same windows, another summation order)
    if G == 16:
        fine = _np(e.af_explain(USERS[:N], ITEMS[:N], grid=112))["map"].astype(np.float64)
        d = float(np.abs(X.rebin(torch.as_tensor(fine).reshape(N, 112, 112), G).numpy() - g["map"]).max())
        t, inputs, _, r64, r32 = _case(k)
        allow = X.allowances(_at_grid(r64, G, rows, torch.float64), _at_grid(r32, G, rows, torch.float32))
        assert d <= allow["map"], (d, allow["map"])


@pytest.mark.parametrize("n", [0, 1, B])
def test_call_sizes(n):
    e = _case(16)[2]
    rows = list(range(n)) if n != 1 else [9]
    g = _np(e.af_explain([USERS[r] for r in rows], [ITEMS[r] for r in rows], grid=14))
    if n == 0:
        assert g["score"].shape == (0,) and g["parts"].shape == (0, 3) and g["map"].shape == (0, 196)
        return
    _check(g, e, 16, 14, rows, "n=%d" % n)


def test_engine_chunks_over_max_batch():
    t, inputs, e, _, _ = _case(16)
    small = _engine(t, inputs, max_batch=5)
    a, b = e.af_explain(USERS, ITEMS, grid=7), small.af_explain(USERS, ITEMS, grid=7)      # 16 pairs in chunks of 5
    for f in a:
        assert torch.equal(a[f], b[f]), f
    small.close()


def _state(e):
    return {n: v.clone() for n, v in e.t.items()}


@pytest.mark.parametrize("opt", ["sgd", "adam_tf23"])
def test_neutral_towards_training_state(opt):
    t, inputs, _, _, _ = _case(16)
    rs = np.random.RandomState(41)
    batches = [tuple(torch.as_tensor(rs.randint(0, hi, B), dtype=torch.int32, device="cuda") for hi in (U, I, I)) for _ in range(6)]
    runs = []
    for with_call in (False, True):
        e = _engine(t, inputs, optimizer=opt, lr=0.01, reg=0.01)
        losses = []
        for s, b in enumerate(batches):
            if with_call and s == 3:                                 # between steps 3 and 4
                before, step = _state(e), e.af_step
                e.af_explain(USERS, ITEMS, grid=7)
                e.af_explain(USERS[:N], ITEMS[:N], grid=112, maps=False)
                assert e.af_step == step == 3
                for n, v in before.items():
                    assert torch.equal(e.t[n], v), n
            losses.append(e.step(*b).item())
        runs.append((losses, _state(e), e.af_step))
        e.close()
    assert runs[0][0] == runs[1][0] and runs[0][2] == runs[1][2] == 6
    if opt == "adam_tf23":
        assert any(n.startswith("m_") for n in runs[0][1])
    for n in runs[0][1]:
        assert torch.equal(runs[0][1][n], runs[1][1][n]), n


def test_errors_and_handle_stays_usable():
    from fashionvisualexpl_recommend_amd.engine import Engine
    t, inputs, _, _, _ = _case(16)
    e = _engine(t, inputs)
    for G in (0, -1, 3, 5, 113, 224):
        with pytest.raises(_ffi.BprxError) as ex:
            e.af_explain([1, 2], [3, 4], grid=G)
        assert ex.value.code == _ffi.E_INVALID
    with pytest.raises(_ffi.BprxError) as ex:                        # more than max_batch pairs in one library call
        u = torch.zeros(B + 1, dtype=torch.int32, device=e.device)
        f = lambda *s: torch.empty(s, dtype=torch.float32, device=e.device)
        p = lambda z: _ffi.C.c_void_p(z.data_ptr())
        _ffi.check(e.h, e.lib.bprx_af_explain(e.h, p(u), p(u), B + 1, 7, p(f(B + 1)), p(f(B + 1, 3)), p(f(B + 1, 3)), None,
                                              p(u.clone()), p(f(B + 1)), None))
    assert ex.value.code == _ffi.E_INVALID
    rs = np.random.RandomState(3)
    plain = Engine(model="bprmf", num_users=8, num_items=9, embed_k=16, optimizer="sgd", lr=0.1, reg=0.0, max_batch=16)
    plain.bind(Gu=synth.glorot_uniform(rs, 8, 16), Gi=synth.glorot_uniform(rs, 9, 16), Bi=np.zeros(9, np.float32))
    with pytest.raises(_ffi.BprxError) as ex:
        plain.af_explain([1], [2], grid=7)
    assert ex.value.code == _ffi.E_STATE
    for users, items in (([0, 1], [2, 10 ** 6]), ([0, U + 3], [2, 3]), ([-1], [-5])):      # clamped and reported, nothing faults
        e.af_explain(users, items, grid=7)
        with pytest.raises(_ffi.BprxError) as ex:
            e.sync_check()
        assert ex.value.code == _ffi.E_RANGE
    # the claims were released: the handle explains and steps as a fresh one does
    g = _np(e.af_explain(USERS[:N], ITEMS[:N], grid=7))
    _check(g, e, 16, 7, list(range(N)), "after-range-error")
    fresh = _engine(t, inputs)
    rs = np.random.RandomState(43)
    b = tuple(torch.as_tensor(rs.randint(0, hi, B), dtype=torch.int32, device="cuda") for hi in (U, I, I))
    assert e.step(*b).item() == fresh.step(*b).item()
    for n in fresh.t:
        assert torch.equal(e.t[n], fresh.t[n]), n
    e.sync_check()
    e.close(); fresh.close(); plain.close()


def test_closed_handles_give_the_workspace_back():
    """A destroyed handle frees the cell sums of bprx_af_explain (38 MB for 12 rows at G = 112), also after the workspace grew."""
    t, inputs, _, _, _ = _case(16)
    warm = _engine(t, inputs)
    warm.af_explain(USERS[:N], ITEMS[:N], grid=112)                  # first use: code objects, allocator pools
    warm.close()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for n in range(4):
        e = _engine(t, inputs)
        e.af_explain(USERS[:N], ITEMS[:N], grid=14, maps=False)
        e.af_explain(USERS[:N], ITEMS[:N], grid=112, maps=False)     # grows the workspace
        e.close()
    torch.cuda.synchronize()
    lost = free0 - torch.cuda.mem_get_info()[0]
    assert lost < 16 << 20, "%.1f MB of device memory not returned after 4 handles" % (lost / 2 ** 20)


def _toy(tmp_path, U=24, I=16, seed=3):
    train, val, test = synth.make_interactions(U, I, per_user=5, seed=seed)
    root = str(tmp_path / "data")
    synth.write_dataset(root, "toy", train, val, test, I)
    synth.write_attentive_features(root, "toy", I, dim_color=24, dim_class=10, image_size=48, seed=seed)
    return root


def test_cli_writes_explanations_next_to_unchanged_recommendations(tmp_path):
    from fashionvisualexpl_recommend_amd import train_rec
    root = _toy(tmp_path)
    common = ["--rec", "attentive_fashion", "--dataset", "toy", "--data_root", root, "--epochs", "1", "--batch_size", "32",
              "--embed_k", "16", "--attention_layers", "32", "1", "--reg", "0.01", "--top_k", "4"]
    res = [str(tmp_path / "res0"), str(tmp_path / "res1")]
    train_rec.train(common + ["--results_root", res[0]])
    plain_dp = train_rec._last_model.directory_parameters
    train_rec.train(common + ["--results_root", res[1], "--af_explain", "7"])
    m = train_rec._last_model
    assert m.params.af_explain == 7 and m.directory_parameters == plain_dp
    rdir = [os.path.join(r, "rec_results", "toy", "attentive_fashion") for r in res]
    files = [sorted(os.listdir(d)) for d in rdir]
    assert not [f for f in files[0] if "expl-" in f]
    assert [f for f in files[1] if "expl-" not in f] == files[0]
    pairs = [(f, f.replace("recs-", "expl-", 1)) for f in files[0] if f.startswith("recs-") or f.startswith("best-recs-")]
    assert len(pairs) == 2 and all(x in files[1] for _, x in pairs)
    assert "expl-1-%s.tsv" % plain_dp in files[1] and any(f.startswith("best-expl-") for f in files[1])
    for recs, expl in pairs:
        assert open(os.path.join(rdir[0], recs), "rb").read() == open(os.path.join(rdir[1], recs), "rb").read()
        rrows = [l.rstrip("\n").split("\t") for l in open(os.path.join(rdir[1], recs))]
        erows = [l.rstrip("\n").split("\t") for l in open(os.path.join(rdir[1], expl))]
        assert len(rrows) == 24 * 4 and all(len(r) == 9 + 49 for r in erows)
        assert [(r[0], r[1]) for r in erows] == [(r[0], r[1]) for r in rrows]
        for a, b in zip(erows, rrows):
            v = [float(z) for z in a[2:]]
            # float32 values printed in full: the score bound of this project (tests/test_gpu_attentive.py), 1e-5 absolute
            assert abs(v[0] - float(b[2])) <= 1e-5
            assert abs(v[1] + v[2] + v[3] - v[0]) <= 1e-5, a[:6]
            assert abs(sum(v[7:]) - v[2]) <= 1e-5, a[:6]
            assert 0 <= int(a[6]) < 7 and 0 <= int(a[7]) < 7 and v[6] == v[7 + 7 * int(a[6]) + int(a[7])] == max(v[7:])


def test_model_explain_surface():
    from fashionvisualexpl_recommend_amd import models
    t, inputs, e, _, _ = _case(16)
    train = [[u % I, (u + 3) % I] for u in range(U)]
    data = Namespace(num_users=U, num_items=I, training_list=train, validation_list=[[] for _ in range(U)],
                     test_list=[[(u + 1) % I] for u in range(U)], params=Namespace(batch_eval=128))
    params = Namespace(epochs=1, batch_size=16, embed_k=16, lr=1e-3, reg=0.05, top_k=3, dataset="toy", rec="attentive_fashion",
                       attention_layers=[H, 1], dropout=0.5, optimizer="sgd", dtype="fp32", af_explain=2)
    m = models.AttentiveFashion(data, params, init={n: t[n] for n in ("Gu", "Gi") + tuple(AF_WEIGHTS)}, inputs=inputs)
    ex = m.explain(USERS[:N], ITEMS[:N], grid=7)
    assert isinstance(ex["score"], np.ndarray) and ex["map"].shape == (N, 49)
    want = _np(e.af_explain(USERS[:N], ITEMS[:N], grid=7))
    for f in want:
        assert np.array_equal(ex[f], want[f]), f
    one = m.explain_ui(1, [1, 3], maps=False)                        # rows 1 and 9 of the case, default grid 14
    assert "map" not in one and one["parts"].shape == (2, 3)
    assert np.array_equal(one["parts"], _np(e.af_explain([1, 1], [1, 3], grid=14, maps=False))["parts"])
