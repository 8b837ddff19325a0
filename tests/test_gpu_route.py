"""The fixed-capacity row-routing kernels (bprx_route.hip) against a plain host model, W ranks simulated in ONE process on one
GPU: every rank has its own buffers, and each all-to-all of equal splits is a transpose of the ranks' [W*cap, ...] buffers.
One step per rank is what UserRowExchange.plan_native / fetch_native / give_back_native do:

  plan -> a2a(send_idx) -> gather -> a2a(rows) -> unpack -> pack -> a2a(gradient rows) -> scatter_add

Slot positions depend on the order of the atomics, so the checks are the properties every valid order has.  Copies must be
bit-exact; table updates are compared with the fp64 sum within an fp32 bound that grows with the row's multiplicity."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RT_MAXW = 64
U_FP32 = 2.0 ** -24


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ok(rc, what):
    assert rc == 0, "%s returned %d" % (what, rc)


def _buf(shape, off, dev="cuda"):
    """Zero fp32 tensor of `shape` that starts `off` floats into its storage (off = 1: never 16-byte aligned)."""
    n = int(np.prod(shape))
    return torch.zeros(n + off + 4, dtype=torch.float32, device=dev)[off:off + n].view(shape)


def _a2a(bufs, W, cap):
    """all_to_all_single with equal splits: out[r][s*cap + p] = bufs[s][r*cap + p]."""
    x = torch.stack(bufs).view((W, W, cap) + tuple(bufs[0].shape[1:]))
    return [x[:, r].reshape((W * cap,) + tuple(bufs[0].shape[1:])).clone() for r in range(W)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


class _Rank:
    def __init__(self, r, W, ush, rows, cap, n_max, w0, w1, off, rs):
        ps = (w0 + w1 + 3) & ~3
        i32 = lambda n: torch.zeros(max(n, 1), dtype=torch.int32, device="cuda")
        self.rows = rows
        self.t0 = _buf((rows, w0), off)
        self.t0.copy_(torch.as_tensor(rs.standard_normal((rows, w0)).astype(np.float32)))
        self.t1 = None
        if w1:
            self.t1 = _buf((rows, w1), off)
            self.t1.copy_(torch.as_tensor(rs.standard_normal((rows, w1)).astype(np.float32)))
        self.send_idx, self.cursor, self.overflow, self.err = i32(W * cap), i32(W), i32(1), i32(1)
        self.slot = i32(n_max)
        self.rows_out = torch.zeros((W * cap, ps), dtype=torch.float32, device="cuda")
        self.grad_out = torch.zeros((W * cap, ps), dtype=torch.float32, device="cuda")
        self.own_cnt, self.cnt = i32(ush), i32(ush)
        self.dst0, self.dst1 = _buf((max(n_max, 1), w0), off), (_buf((max(n_max, 1), w1), off) if w1 else None)
        self.g0, self.g1 = _buf((max(n_max, 1), w0), off), (_buf((max(n_max, 1), w1), off) if w1 else None)

    def table(self):
        """[rows, w0 + w1] host copy of the shard."""
        t = self.t0.cpu().numpy()
        return np.concatenate([t, self.t1.cpu().numpy()], axis=1) if self.t1 is not None else t.copy()


class _Sim:
    """W ranks of one row exchange: shard r holds global rows [r*ush, r*ush + rows_r) (the last shard may be short)."""

    def __init__(self, W, total, w0, w1, n_max, slack=2.0, off=0, seed=0, cap=None):
        from fashionvisualexpl_recommend_amd import _ffi
        from fashionvisualexpl_recommend_amd.dist import shard_size
        self.L = _ffi.lib()
        self.W, self.total, self.w0, self.w1 = W, total, w0, w1
        self.ush = shard_size(total, W)
        self.cap = cap if cap is not None else int(min(n_max, -(-n_max // W) * slack + 8))
        rs = np.random.RandomState(seed)
        rows = [min(total, (r + 1) * self.ush) - r * self.ush for r in range(W)]
        assert min(rows) > 0
        self.R = [_Rank(r, W, self.ush, rows[r], self.cap, n_max, w0, w1, off, rs) for r in range(W)]
        for R in self.R:
            _ok(self.L.bprx_route_reset(_p(R.send_idx), W * self.cap, _p(R.cursor), W, _s()), "route_reset")

    def global_table(self):
        """[W*ush, w0 + w1] fp64: every shard at its global rows, zero rows past a short last shard."""
        G = np.zeros((self.W * self.ush, self.w0 + self.w1), np.float64)
        for r, R in enumerate(self.R):
            G[r * self.ush:r * self.ush + R.rows] = R.table()
        return G

    def step(self, ids, split, grads, scale, own=True, hot=None):
        """One exchange step on every rank.  ids[r]: int64 global ids (may hold out-of-range ones), split[r]: how many of them
        go in the first id array; grads[r]: [n_r, w0 + w1] fp32 gradient rows.  own=False: unpack / pack get no own tables.
        hot: a row id whose counts may be left non-zero (asked for more than 65 535 times in some step)."""
        L, W, cap, ush, w0, w1 = self.L, self.W, self.cap, self.ush, self.w0, self.w1
        ncol = w0 + w1
        T0 = self.global_table()
        before = {r: (R.own_cnt.cpu().numpy().copy(), R.cnt.cpu().numpy().copy()) for r, R in enumerate(self.R)}
        for R in self.R:
            R.overflow.zero_()
            R.err.zero_()
        # ---- plan
        dev_ids = []
        for r, R in enumerate(self.R):
            a = torch.as_tensor(ids[r][:split[r]].astype(np.int32), device="cuda")
            b = torch.as_tensor(ids[r][split[r]:].astype(np.int32), device="cuda")
            dev_ids.append((a, b))
            _ok(L.bprx_route_plan(_p(a) if a.numel() else None, a.numel(), _p(b) if b.numel() else None, b.numel(), ush, W, cap, r,
                                  _p(R.slot), _p(R.send_idx), _p(R.cursor), _p(R.overflow), _p(R.own_cnt), _s()), "route_plan")
        slots = [R.slot.cpu().numpy()[:len(ids[r])].astype(np.int64) for r, R in enumerate(self.R)]
        send = [R.send_idx.cpu().numpy() for R in self.R]
        for r, R in enumerate(self.R):
            self._check_plan(r, ids[r], slots[r], send[r], int(R.overflow.item()), R.own_cnt.cpu().numpy() - before[r][0])
        recv = _a2a([R.send_idx[:W * cap] for R in self.R], W, cap)
        # ---- gather, all-to-all, unpack
        for r, R in enumerate(self.R):
            _ok(L.bprx_route_gather_checked(_p(R.t0), w0, _p(R.t1), w1, R.rows, _p(recv[r]), W * cap, _p(R.rows_out), _p(R.cnt), _p(R.err),
                                    _s()), "route_gather")
        for r, R in enumerate(self.R):            # the owner counts every row the other ranks ask for that it holds
            ri = recv[r].cpu().numpy()
            ri = ri[(ri >= 0) & (ri < R.rows)]
            want = np.bincount(ri, minlength=ush).astype(np.int64)
            assert np.array_equal(R.cnt.cpu().numpy() - before[r][1], want), "gather counts, rank %d" % r
        got = _a2a([R.rows_out for R in self.R], W, cap)
        for r, R in enumerate(self.R):
            n = len(ids[r])
            _ok(L.bprx_route_unpack_checked(_p(got[r]), _p(R.slot), n, _p(R.dst0), w0, _p(R.dst1), w1, _p(R.t0) if own else None,
                                    _p(R.t1) if own else None, R.rows, _p(R.err), _s()), "route_unpack")
        # expected rows of every request, and which requests contribute a gradient
        err_want = np.zeros(W, bool)
        rows = np.array([R.rows for R in self.R], np.int64)
        contrib = []
        for r, R in enumerate(self.R):
            g, s = ids[r], slots[r]
            local = g - (g // ush) * ush
            owner = g // ush
            mine = s <= -2
            inside = np.zeros(len(g), bool)
            ok_id = (g >= 0) & (owner < W)
            inside[ok_id] = local[ok_id] < rows[owner[ok_id]]
            c = ((s >= 0) & inside) | (mine & inside & own)
            contrib.append(c)
            want = np.zeros((len(g), ncol), np.float32)
            want[c] = T0[g[c]]
            if (mine & ~inside & own).any():
                err_want[r] = True
            for o in np.unique(owner[(s >= 0) & ~inside]):
                err_want[o] = True
            if len(g):
                have = R.dst0[:len(g)].cpu().numpy()
                if w1:
                    have = np.concatenate([have, R.dst1[:len(g)].cpu().numpy()], axis=1)
                assert np.array_equal(_bits(have), _bits(want)), "unpacked rows, rank %d" % r
        for r, R in enumerate(self.R):
            assert bool(R.err.item()) == err_want[r], "row-range error flag, rank %d" % r
        # ---- gradients into the staging rows, pack, all-to-all back, scatter-add
        for r, R in enumerate(self.R):
            n = len(ids[r])
            if n:
                R.g0[:n].copy_(torch.as_tensor(grads[r][:, :w0]))
                if w1:
                    R.g1[:n].copy_(torch.as_tensor(grads[r][:, w0:]))
            _ok(L.bprx_route_pack(_p(R.g0), w0, _p(R.g1), w1, _p(R.slot), n, _p(R.grad_out), _p(R.t0) if own else None,
                                  _p(R.t1) if own else None, R.rows, float(scale), _p(R.own_cnt), _p(R.send_idx),
                                  W * cap, _p(R.cursor),
                                  W, _s()), "route_pack")
        for r, R in enumerate(self.R):
            s = slots[r]
            sent = s >= 0
            if sent.any():                     # sent rows are copied unscaled
                assert np.array_equal(_bits(R.grad_out.cpu().numpy()[s[sent], :ncol]), _bits(grads[r][sent])), "packed rows, rank %d" % r
            assert float(R.g0.abs().max()) == 0.0 and (R.g1 is None or float(R.g1.abs().max()) == 0.0), "staging not zero"
            assert bool((R.send_idx == -1).all()) and bool((R.cursor == 0).all()), "send list not re-armed, rank %d" % r
        back = _a2a([R.grad_out for R in self.R], W, cap)
        for r, R in enumerate(self.R):
            _ok(L.bprx_route_scatter_add(_p(R.t0), w0, _p(R.t1), w1, R.rows, _p(recv[r]), _p(back[r]), W * cap, float(scale), _p(R.cnt),
                                         _s()), "route_scatter_add")
        # ---- the tables against the fp64 sum
        acc = torch.zeros(T0.shape, dtype=torch.float64)
        mag = torch.zeros(T0.shape, dtype=torch.float64)
        mult = np.zeros(W * ush, np.int64)
        for r in range(W):
            c = contrib[r]
            g = torch.as_tensor(ids[r][c])
            x = torch.as_tensor(grads[r][c]).double()
            acc.index_add_(0, g, x)
            mag.index_add_(0, g, x.abs())
            mult += np.bincount(ids[r][c], minlength=W * ush)
        acc, mag = acc.numpy(), mag.numpy()
        want = T0 + scale * acc
        tol = (mult[:, None] + 1) * 2 * U_FP32 * (np.abs(T0) + abs(scale) * mag)
        have = self.global_table()
        bad = np.abs(have - want) > tol
        assert not bad.any(), "table rows %s: got %s want %s (multiplicity %s)" % (
            np.nonzero(bad.any(1))[0][:5], have[bad][:5], want[bad][:5], mult[np.nonzero(bad.any(1))[0][:5]])
        # ---- both count arrays return to all-zero (rows asked for fewer than 65 536 times)
        for r, R in enumerate(self.R):
            for name, a in (("own_cnt", R.own_cnt), ("cnt", R.cnt)):
                a = a.cpu().numpy().copy()
                if hot is not None and hot // ush == r:
                    a[hot - r * ush] = 0
                assert not a.any(), "%s not zero after the step, rank %d: rows %s" % (name, r, np.nonzero(a)[0][:5])
        return have, want

    def _check_plan(self, r, g, s, send, overflow, own_added):
        W, cap, ush = self.W, self.cap, self.ush
        valid = (g >= 0) & (g // ush < W)
        owner = np.where(valid, g // ush, -1)
        local = g - owner * ush
        assert not (s == -1)[valid & (owner == r)].any()
        mine = valid & (owner == r)
        assert np.array_equal(s[mine], -2 - local[mine]), "own rows, rank %d" % r
        assert (s[~valid] == -1).all(), "out-of-range ids must get no slot"
        fs = s[s >= 0]
        assert len(np.unique(fs)) == len(fs), "slots not distinct, rank %d" % r
        dropped = 0
        for o in range(W):
            req = valid & (owner == o) & (o != r)
            sl = s[req]
            ins = sl[sl >= 0]
            assert ((ins >= o * cap) & (ins < o * cap + cap)).all(), "slot outside its owner's bucket"
            assert np.array_equal(send[ins], local[req][sl >= 0]), "send_idx of the slots"
            assert np.array_equal(np.sort(ins), o * cap + np.arange(min(cap, int(req.sum())))), "bucket %d not filled from 0" % o
            dropped += max(0, int(req.sum()) - cap)
            bucket = send[o * cap:(o + 1) * cap]
            assert int((bucket >= 0).sum()) == len(ins), "stray send_idx entries in bucket %d" % o
        assert int((s == -1).sum()) == dropped + int((~valid).sum())
        assert overflow == int((s == -1).any()), "overflow flag, rank %d" % r
        assert np.array_equal(own_added[:ush], np.bincount(local[mine], minlength=ush)), "own_cnt, rank %d" % r


def _grads(rs, n, ncol):
    return rs.standard_normal((n, ncol)).astype(np.float32)


def _batches(W, total, ush, n, step, rs, bad=False):
    """Ragged per-rank requests (some ranks empty), a few of them repeated; bad: also ids past a short last shard and
    ids out of range."""
    ids, split = [], []
    for r in range(W):
        nr = n - (13 * r) % (n // 2) - 7 * step
        if (r == 1 and step == 1) or (W >= 5 and r == W - 2 and step == 2) or (W == 1 and step == 1):
            nr = 0
        x = rs.randint(total, size=nr).astype(np.int64)
        if nr > 8:
            x[:4] = x[4]                                   # the same row four more times
        if bad and nr > 12:
            x[5:8] = [total + (W * ush - total - 1 if W * ush > total else 0), -1, W * ush + 3]
            if W * ush == total:
                x[5] = rs.randint(total)
        ids.append(x)
        split.append(nr // 2)
    return ids, split


CASE_WIDTHS = [(128, 1), (64, 0), (16, 16), (5, 3), (4, 0)]


@pytest.mark.parametrize("W", [1, 2, 3, 5, 8, RT_MAXW])
@pytest.mark.parametrize("w0,w1", CASE_WIDTHS)
def test_route_three_steps(W, w0, w1):
    """Three consecutive steps with no route_reset between them (k_route_pack re-arms send_idx and the cursors), ragged
    batches with empty ranks, duplicate rows, and in the middle step ids past the short last shard and out of range."""
    _run_three(W, w0, w1, off=0)


@pytest.mark.parametrize("W,w0,w1", [(3, w0, w1) for w0, w1 in CASE_WIDTHS] + [(8, 128, 1)])
def test_route_three_steps_misaligned_tables(W, w0, w1):
    """Tables and staging rows one float off 16-byte alignment: every part takes the element-wise path."""
    _run_three(W, w0, w1, off=1)


def _run_three(W, w0, w1, off):
    rs = np.random.RandomState(1000 * W + 10 * w0 + w1 + off)
    n = 300 if W < 64 else 120
    total = 150 * W - 1                                   # W > 1: the last shard is one row short
    sim = _Sim(W, total, w0, w1, n_max=n, off=off, seed=W + w0)
    for step in range(3):
        ids, split = _batches(W, total, sim.ush, n, step, rs, bad=(step == 1))
        sim.step(ids, split, [_grads(rs, len(x), w0 + w1) for x in ids], -0.05)


def test_route_unpack_without_own_tables():
    """own0 = NULL: the requester's own rows unpack as zero rows and their gradients are dropped."""
    rs = np.random.RandomState(7)
    W, total, n = 3, 50, 200
    sim = _Sim(W, total, 16, 16, n_max=n)
    for step in range(2):
        ids, split = _batches(W, total, sim.ush, n, step, rs)
        sim.step(ids, split, [_grads(rs, len(x), 32) for x in ids], -0.05, own=False)


@pytest.mark.parametrize("W", [3, 8])
def test_route_zipf_overflow(W):
    """Zipf-skewed ids at slack 0.5: the hottest owner's bucket overflows; the surplus requests get -1 (zero rows, dropped
    gradients), the flag is raised, and the next step (re-armed by pack) plans from empty buckets again."""
    rs = np.random.RandomState(W)
    total, n = 64 * W, 600
    sim = _Sim(W, total, 16, 1, n_max=n, slack=0.5)
    for step in range(3):
        ids = [(rs.zipf(1.3, size=n) - 1) % total for _ in range(W)]
        ids = [x.astype(np.int64) for x in ids]
        sim.step(ids, [n // 2] * W, [_grads(rs, n, 17) for _ in range(W)], -0.05)
    owners = np.bincount(ids[W - 1] // sim.ush, minlength=W)
    assert owners[0] > sim.cap                              # (the case really overflows)


@pytest.mark.parametrize("where", ["own", "foreign"])
def test_route_row_asked_70000_times(where):
    """One row asked for 70 000 times in a step (its count overflows the 16-bit halves), then once, then twice.  With dyadic
    values every sum is exact in fp32, so the tables must equal the fp64 sums bit for bit in all three steps."""
    rs = np.random.RandomState(70)
    W, total, hot_n, extra = 2, 200, 70000, 300
    n = hot_n + extra
    sim = _Sim(W, total, 16, 4, n_max=n, cap=n)
    for R in sim.R:                                        # dyadic tables: multiples of 1/256
        R.t0.copy_(torch.round(R.t0 * 256) / 256)
        R.t1.copy_(torch.round(R.t1 * 256) / 256)
    hot = 3                                                # a row of rank 0
    asker = 0 if where == "own" else 1
    for step, mult in enumerate((hot_n, 1, 2)):
        ids = []
        for r in range(W):
            x = rs.randint(total, size=extra).astype(np.int64)
            x = x[x != hot]
            if r == asker:
                x = np.concatenate([np.full(mult, hot, np.int64), x])
                rs.shuffle(x)
            ids.append(x)
        grads = [(rs.randint(-4, 5, size=(len(x), 20)) / 256.0).astype(np.float32) for x in ids]
        have, want = sim.step(ids, [len(x) // 3 for x in ids], grads, -0.5, hot=hot)
        assert np.array_equal(have, want), "step %d (multiplicity %d)" % (step, mult)


def test_route_scatter_add_grid_stride_c3shard():
    """The c3shard batch (B = 65 536: 2B requests per rank) with W = 8 and BPRMF's [Gi | Bi] rows (128 + 1): cap = 32 776,
    W*cap = 262 208 slots > 16 384 blocks x 16 rows, so k_route_scatter_add loops.  Rank 7 fills its bucket at owner 0, so
    the slots past 262 144 carry rows."""
    rs = np.random.RandomState(65536)
    W, B = 8, 65536
    n = 2 * B
    total = 8 * 6000 - 11
    sim = _Sim(W, total, 128, 1, n_max=n)
    assert sim.cap == 32776 and W * sim.cap > 16384 * 16
    ids = [rs.randint(total, size=n).astype(np.int64) for _ in range(W)]
    ids[7][:sim.cap] = rs.randint(sim.ush, size=sim.cap)    # rank 7: a full bucket at owner 0
    sim.step(ids, [B] * W, [_grads(rs, n, 129) for _ in range(W)], -0.05)
