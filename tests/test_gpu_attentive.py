"""AttentiveFashion on the MI355X against the float64 restatement of AttentiveFashion.py (tests/attentive_ref.py) on identical
tables, images and dropout masks: the three encoders, pair and block scores with their attentions, one sgd step and 20 adam_tf23 steps
with reg > 0 and rate = 0.5 (every tensor), the dropout stream's own properties, bit-reproducible steps, range errors, snapshots and
the CLI.

Tolerances are the project's (tests/test_gpu_acf.py): scores and encodings 1e-5 absolute, loss 1e-5 relative after one step and 1e-4
over the Adam run, tables 1e-6 (sgd) / 2e-5 (Adam).  The conv kernel and bias are the exception: relu and max-pool kinks make even
plain float32 deviate from float64 by an input-dependent amount, so for these two tensors each test runs the SAME restatement in
float32 on its own inputs and allows the GPU max(project bound, 4 x that deviation) -- four because the split-operand MFMA rounds the
weights a second time and sums in another order.  The three numbers are printed and are part of the assertion message."""
import os

import numpy as np
import pytest
import torch

from attentive_ref import AF_WEIGHTS, AttentiveRef, random_inputs, random_tables
from fashionvisualexpl_recommend_amd import _ffi, synth

pytestmark = pytest.mark.gpu
KINK = ("edges.conv", "edges.conv_b")


def _engine(t, inputs, optimizer="sgd", lr=0.05, reg=0.0, B=64, rate=0.5, seed=7):
    from fashionvisualexpl_recommend_amd.engine import Engine
    U, k = t["Gu"].shape
    e = Engine(model="bprmf", num_users=U, num_items=t["Gi"].shape[0], embed_k=k, optimizer=optimizer, lr=lr, reg=reg, max_batch=B)
    return e.bind_attentive(t["Gu"], t["Gi"], t["Bi"], *inputs, {n: t[n] for n in AF_WEIGHTS}, dropout=rate, seed=seed)


def _dev(e, batch):
    return tuple(torch.as_tensor(np.asarray(b), dtype=torch.int32, device=e.device) for b in batch)


def _masks(e, step, n_rows):
    return tuple(m.cpu() for m in e.af_dropout_mask(step, n_rows))


@pytest.mark.parametrize("k,bias", [(16, True), (128, True), (128, False)])
def test_encode_against_fp64(k, bias):
    rs = np.random.RandomState(k + bias)
    U, I, Dc, Dk = 5, 8, 37, 11                                      # Dc, Dk not multiples of 16
    t = random_tables(rs, U, I, k, Dc, Dk, 64, bias=bias)
    inputs = random_inputs(rs, I, Dc, Dk)                            # item 0 blank, item 1 dense, the rest sparse edges
    e = _engine(t, inputs)
    ref = AttentiveRef(t, *inputs)
    items = [0, 1, 2, 3, 4, 5, 6, 7, 3, 0]
    got = e.af_encode(items).cpu().double()
    with torch.no_grad():
        want = torch.stack(ref.encode(ref.p, items))
    err = (got - want).abs().max().item()
    print("encode k=%d bias=%s: max abs error %.3g (|c| up to %.3g)" % (k, bias, err, want.abs().max().item()))
    assert err <= 1e-5, err
    e.sync_check()


@pytest.mark.parametrize("h", [32, 64])
def test_scores_and_attention_pairs_and_block(h):
    rs = np.random.RandomState(h)
    U, I, Dc, Dk, k = 7, 9, 20, 6, 16                                # I is not a multiple of any tile
    t = random_tables(rs, U, I, k, Dc, Dk, h)
    t["Gu"] *= 4.0                                                   # widen the attention logits
    inputs = random_inputs(rs, I, Dc, Dk)
    e = _engine(t, inputs)
    ref = AttentiveRef(t, *inputs)
    u = np.array([0, 3, 3, 6, 1, 3, 0, 5]); i = np.array([8, 2, 2, 0, 1, 7, 8, 4])      # duplicated users and pairs
    with torch.no_grad():
        wx, wa, _ = ref.call(u, i)
        bx, ba = ref.predict_all()
    x, al = e.af_attention_pairs(u, i)
    assert (x.cpu().double() - wx).abs().max().item() <= 1e-5
    assert (al.cpu().double() - wa).abs().max().item() <= 1e-5
    assert (e.score_pairs(u, i).cpu().double() - wx).abs().max().item() <= 1e-5
    sx, sa = e.af_score_block(0, U)
    assert (sx.cpu().double() - bx).abs().max().item() <= 1e-5
    assert (sa.cpu().double() - ba).abs().max().item() <= 1e-5
    assert (sa.sum(-1) - 1).abs().max().item() <= 1e-6
    assert (e.score_block(2, 5).cpu().double() - bx[2:5]).abs().max().item() <= 1e-5
    e.sync_check()


@pytest.mark.parametrize("h", [96, 128])
def test_block_beyond_the_first_tile(h):
    """I = 300 (three item tiles of 128, the last one partial: every wave, the tile loop), k = 20 (not a multiple of 8: padded K,
    the scalar operand loads) and h = 96 / 128 (three and four hidden tiles)."""
    rs = np.random.RandomState(h)
    U, I, Dc, Dk, k = 5, 300, 20, 6, 20
    t = random_tables(rs, U, I, k, Dc, Dk, h)
    t["Gu"] *= 4.0
    edges, color, cls = random_inputs(rs, 12, Dc, Dk)
    pick = rs.randint(0, 12, I)                                      # 300 items over 12 distinct images
    inputs = (edges[pick], color[rs.randint(0, 12, I)], cls[rs.randint(0, 12, I)])
    e = _engine(t, inputs)
    ref = AttentiveRef(t, *inputs)
    with torch.no_grad():
        bx, ba = ref.predict_all()
    sx, sa = e.af_score_block(0, U)
    assert (sx.cpu().double() - bx).abs().max().item() <= 1e-5
    assert (sa.cpu().double() - ba).abs().max().item() <= 1e-5
    assert (e.score_block(1, 4).cpu().double() - bx[1:4]).abs().max().item() <= 1e-5
    u = rs.randint(0, U, 60); i = rs.randint(0, I, 60)
    x, al = e.af_attention_pairs(u, i)
    assert (x.cpu().double() - bx[u, i]).abs().max().item() <= 1e-5
    assert (al.cpu().double() - ba[u, i]).abs().max().item() <= 1e-5
    e.sync_check()


def _compare(e, ref, ref32, ref0, atol, tag):
    """every tensor against the float64 restatement; conv kernel / bias: max(atol, 4 x the float32 restatement's own deviation)"""
    for n in ("Gu", "Gi") + tuple(AF_WEIGHTS):
        want = ref.p[n]
        got = e.t[n].cpu().double().reshape(want.shape)
        err = (got - want).abs().max().item()
        allow = atol
        if n in KINK:
            dev32 = (ref32.p[n].double() - want).abs().max().item()
            allow = max(atol, 4.0 * dev32)
            print("%s %s: fp32 deviation %.3g, allowance %.3g, GPU deviation %.3g (update size %.3g)"
                  % (tag, n, dev32, allow, err, (want - ref0[n]).abs().max().item()))
            assert err <= allow, (tag, n, "fp32 deviation %.3g" % dev32, "allowance %.3g" % allow, "GPU deviation %.3g" % err)
        else:
            assert err <= allow, (tag, n, err)


def _step_case(rs, U=12, I=10, Dc=37, Dk=11, k=16, h=32):
    t = random_tables(rs, U, I, k, Dc, Dk, h)
    return t, random_inputs(rs, I, Dc, Dk)


def test_sgd_step_every_tensor():
    rs = np.random.RandomState(11)
    t, inputs = _step_case(rs)
    B = 24
    u = rs.randint(0, 12, B); i = rs.randint(0, 10, B); j = rs.randint(0, 10, B)
    i[:4] = 3; j[4:7] = 3; j[0] = 5; i[9] = 5                        # repeated items, items on both sides
    e = _engine(t, inputs, reg=0.05, lr=0.05, B=B)
    masks = _masks(e, 0, 2 * B)
    ref = AttentiveRef(t, *inputs, reg=0.05)
    ref32 = AttentiveRef(t, *inputs, reg=0.05, dtype=torch.float32)
    ref0 = {n: v.clone() for n, v in ref.p.items()}
    want = ref.step((u, i, j), masks, "sgd", 0.05)
    ref32.step((u, i, j), masks, "sgd", 0.05)
    got = float(e.step(*_dev(e, (u, i, j))).item())
    print("sgd step: loss %.8g (float64 %.8g)" % (got, want))
    assert abs(got - want) <= 1e-5 * abs(want), (got, want)
    _compare(e, ref, ref32, ref0, 1e-6, "sgd")
    e.sync_check()


def test_sgd_step_larger_batch():
    """B = 48: 96 sample rows (two 64-row GEMM tiles, two ballot rounds of the row sums, column-sum groups of more than one row),
    every item many times on both sides."""
    rs = np.random.RandomState(12)
    U, I = 50, 14
    t, inputs = _step_case(rs, U=U, I=I)
    B = 48
    batch = (rs.randint(0, U, B), rs.randint(0, I, B), rs.randint(0, I, B))
    e = _engine(t, inputs, reg=0.05, lr=0.05, B=B)
    masks = _masks(e, 0, 2 * B)
    ref = AttentiveRef(t, *inputs, reg=0.05)
    ref32 = AttentiveRef(t, *inputs, reg=0.05, dtype=torch.float32)
    ref0 = {n: v.clone() for n, v in ref.p.items()}
    want = ref.step(batch, masks, "sgd", 0.05)
    ref32.step(batch, masks, "sgd", 0.05)
    got = float(e.step(*_dev(e, batch)).item())
    print("sgd step B=48: loss %.8g (float64 %.8g)" % (got, want))
    assert abs(got - want) <= 1e-5 * abs(want), (got, want)
    _compare(e, ref, ref32, ref0, 1e-6, "sgd B=48")
    e.sync_check()


def test_adam_20_steps():
    rs = np.random.RandomState(13)
    t, inputs = _step_case(rs)
    B = 16
    e = _engine(t, inputs, optimizer="adam_tf23", reg=0.05, lr=1e-3, B=B)
    assert not e.adam_is_lazy()                                      # the handle always sweeps
    ref = AttentiveRef(t, *inputs, reg=0.05)
    ref32 = AttentiveRef(t, *inputs, reg=0.05, dtype=torch.float32)
    ref0 = {n: v.clone() for n, v in ref.p.items()}
    for s in range(20):
        batch = (rs.randint(0, 12, B), rs.randint(0, 10, B), rs.randint(0, 10, B))
        masks = _masks(e, s, 2 * B)
        want = ref.step(batch, masks, "adam_tf23", 1e-3)
        ref32.step(batch, masks, "adam_tf23", 1e-3)
        got = float(e.step(*_dev(e, batch)).item())
        assert abs(got - want) <= 1e-4 * abs(want), (s, got, want)
    _compare(e, ref, ref32, ref0, 2e-5, "adam")
    e.sync_check()


def test_dropout_stream():
    rs = np.random.RandomState(17)
    t, inputs = _step_case(rs)
    B = 1024
    e1 = _engine(t, inputs, B=B, seed=5)
    e2 = _engine(t, inputs, B=B, seed=5)
    e3 = _engine(t, inputs, B=B, seed=6)
    m0 = torch.cat([m.reshape(-1) for m in e1.af_dropout_mask(0, 2 * B)])
    assert torch.equal(m0, torch.cat([m.reshape(-1) for m in e2.af_dropout_mask(0, 2 * B)]))      # same seed, same masks
    m1 = torch.cat([m.reshape(-1) for m in e1.af_dropout_mask(1, 2 * B)])
    assert not torch.equal(m0, m1)                                   # another step, another mask
    assert not torch.equal(m0, torch.cat([m.reshape(-1) for m in e3.af_dropout_mask(0, 2 * B)]))
    n = m0.numel() + m1.numel()
    assert n >= 10 ** 6
    frac = (m0.sum().item() + m1.sum().item()) / n
    print("keep fraction %.5f over %d bits" % (frac, n))
    assert abs(frac - 0.5) <= 0.01                                   # binomial sigma 5e-4: a sanity bound
    assert set(m0.unique().tolist()) <= {0, 1}


def test_rate_zero_equals_all_ones_mask_bit_for_bit():
    """rate = 0 takes the path without mask and scaling; rate = 1e-12 takes the mask path with an all-ones mask (threshold 0) and
    the scale float32(1 / (1 - 1e-12)) = 1: the two steps must agree bit for bit."""
    rs = np.random.RandomState(19)
    t, inputs = _step_case(rs)
    B = 16
    batch = (rs.randint(0, 12, B), rs.randint(0, 10, B), rs.randint(0, 10, B))
    out = []
    for rate in (0.0, 1e-12):
        e = _engine(t, inputs, reg=0.01, B=B, rate=rate)
        assert all(bool(m.all()) for m in e.af_dropout_mask(0, 2 * B))
        loss = e.step(*_dev(e, batch)).item()
        out.append((loss, {n: e.t[n].clone() for n in ("Gu", "Gi") + tuple(AF_WEIGHTS)}))
    assert out[0][0] == out[1][0]
    for n in out[0][1]:
        assert torch.equal(out[0][1][n], out[1][1][n]), n


@pytest.mark.parametrize("opt", ["sgd", "adam_tf23"])
def test_steps_are_bit_reproducible(opt):
    rs = np.random.RandomState(23)
    t, inputs = _step_case(rs)
    B = 48
    batches = [(rs.randint(0, 12, B), rs.randint(0, 10, B), rs.randint(0, 10, B)) for _ in range(3)]      # every item many times
    out = []
    for _ in range(2):
        e = _engine(t, inputs, optimizer=opt, reg=0.01, lr=0.01, B=B)
        losses = [e.step(*_dev(e, b)).item() for b in batches]
        out.append((losses, {n: e.t[n].clone() for n in ("Gu", "Gi") + tuple(AF_WEIGHTS)}))
    assert out[0][0] == out[1][0]
    for n in out[0][1]:
        assert torch.equal(out[0][1][n], out[1][1][n]), n


def test_range_error_and_handle_stays_usable():
    rs = np.random.RandomState(29)
    t, inputs = _step_case(rs)
    e = _engine(t, inputs)
    ref = AttentiveRef(t, *inputs)
    e.score_pairs([0, 1], [2, 10 ** 6])
    with pytest.raises(_ffi.BprxError) as ex:
        e.sync_check()
    assert ex.value.code == _ffi.E_RANGE
    e.af_encode([-1, 3])
    with pytest.raises(_ffi.BprxError):
        e.sync_check()
    with torch.no_grad():
        want = ref.call([0, 1], [2, 3])[0]
    assert (e.score_pairs([0, 1], [2, 3]).cpu().double() - want).abs().max().item() <= 1e-5
    e.sync_check()


def test_closed_handles_give_their_device_memory_back():
    """A destroyed handle frees its AttentiveFashion scratch (13 MB of conv partials alone at max_batch 1024); so does a handle
    that is bound again as a plain BPRMF handle."""
    rs = np.random.RandomState(37)
    t, inputs = _step_case(rs)
    _engine(t, inputs, B=1024).close()                               # first use: code objects, allocator pools
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for n in range(6):
        e = _engine(t, inputs, B=1024)
        e.score_block(0, 2)
        if n % 2:
            e.bind(t["Gu"], t["Gi"], t["Bi"])                        # a BPRMF handle again
        e.close()
    torch.cuda.synchronize()
    lost = free0 - torch.cuda.mem_get_info()[0]
    assert lost < 16 << 20, "%.1f MB of device memory not returned after 6 handles" % (lost / 2 ** 20)


def _toy(tmp_path, U=40, I=24, seed=3):
    train, val, test = synth.make_interactions(U, I, per_user=6, seed=seed)
    root = str(tmp_path / "data")
    synth.write_dataset(root, "toy", train, val, test, I)
    synth.write_attentive_features(root, "toy", I, dim_color=24, dim_class=10, image_size=48, seed=seed)
    return root, train, val, test


def test_snapshot_restore_continues_the_run(tmp_path):
    from argparse import Namespace
    from fashionvisualexpl_recommend_amd import configs, models
    rs = np.random.RandomState(31)
    root, train, val, test = _toy(tmp_path)
    U, I = 40, 24
    configs.set_roots(root, str(tmp_path / "res"))
    try:
        data = Namespace(num_users=U, num_items=I, training_list=train, validation_list=val, test_list=test,
                         params=Namespace(batch_eval=128))
        params = Namespace(epochs=1, batch_size=16, embed_k=16, lr=1e-3, reg=0.05, top_k=5, dataset="toy", rec="attentive_fashion",
                           attention_layers=[32, 1], dropout=0.5, optimizer="adam_tf23", dtype="fp32")
        m = models.AttentiveFashion(data, params)
    finally:
        configs.set_roots("../data", "../results")
    batches = [(rs.randint(0, U, 16), rs.randint(0, I, 16), rs.randint(0, I, 16)) for _ in range(6)]
    for b in batches[:3]:
        m.train_step(b)
    sd = m.state_dict()
    for b in batches[3:]:
        m.train_step(b)
    want = {n: v.clone() for n, v in m.engine.t.items()}
    m.load_state_dict(sd)
    for b in batches[3:]:
        m.train_step(b)
    for n, v in want.items():                                        # same masks (the step index is part of the snapshot), fixed-order sums
        assert torch.equal(m.engine.t[n], v), n


def test_cli_end_to_end(tmp_path):
    import pickle
    from fashionvisualexpl_recommend_amd import train_rec
    root, train, val, test = _toy(tmp_path)
    res = str(tmp_path / "res")
    out = train_rec.train(["--rec", "attentive_fashion", "--dataset", "toy", "--data_root", root, "--results_root", res, "--epochs", "2",
                           "--batch_size", "32", "--embed_k", "16", "--attention_layers", "32", "1", "--reg", "0.01", "--top_k", "5"])
    m = train_rec._last_model
    rdir = os.path.join(res, "rec_results", "toy", "attentive_fashion")
    files = os.listdir(rdir)
    dp = m.directory_parameters
    assert dp.endswith("-attlayers_[32, 1]")
    assert "results-metrics-%s.pkl" % dp in files
    recs = [f for f in files if f.startswith("recs-2-")]
    assert recs and any(f.startswith("best-recs-") for f in files)
    with open(os.path.join(rdir, "results-metrics-%s.pkl" % dp), "rb") as f:
        r = pickle.load(f)
    assert set(r) == {1, 2} and 0.0 <= r[1]["hr_v"] <= 1.0
    rows = [l.rstrip("\n").split("\t") for l in open(os.path.join(rdir, recs[0]))]
    assert len(rows) == 40 * 5 and all(len(x) == 6 for x in rows)    # u  i  score  alpha_colour  alpha_edges  alpha_class
    assert max(abs(sum(float(v) for v in x[3:]) - 1.0) for x in rows) <= 1e-6
    # the trained model's predict_all_batch equals the float64 restatement on the trained tables
    tabs = {n: v.cpu().numpy() for n, v in m.engine.t.items() if n in ("Gu", "Gi") + tuple(AF_WEIGHTS)}
    ref = AttentiveRef(tabs, m.edges.numpy(), m.color.numpy(), m.classes.numpy())
    wx, wa = ref.predict_all()
    gx, ga = m.predict_all_batch()
    assert (torch.as_tensor(gx).double() - wx).abs().max().item() <= 1e-5
    assert (torch.as_tensor(ga).double() - wa).abs().max().item() <= 1e-5
    assert out
