"""Greedy Maximal Marginal Relevance over a top-N pool restated in numpy on the CPU (a helper module, not a test module), as
include/bprx.h defines bprx_diversify:

    candidates: the pool slots with id >= 0 and score > -inf (M of them)
    rel_c = (v_c - v_min) / (v_max - v_min) over the candidates, 0 for a flat pool
    cos(c, s) = <z_c, z_s> (rn_c rn_s),  rn = 1 / |z|, 0 for a zero row          (z: similar_ref.item_vectors)
    pen_c = max over the selected s of cos(c, s), 0 before the first pick
    obj_c = (1 - theta) rel_c - theta pen_c; min(K, M) picks, each the unselected candidate with the largest obj_c, ties to the
    lower pool position;  ild = 1 - mean over the list's pairs of cos, 0 for fewer than two picks

in float64 (the reference) or float32 (one sample of float32 rounding: the scale of the tests' allowances).  `follow` replays a
given list (pool positions) instead of choosing: the objective of every remaining candidate is then computed at each step given
that prefix, which is how a GPU list is judged without comparing list identities across precisions."""
import numpy as np


def candidates(ids, vals):
    return (np.asarray(ids) >= 0) & ~np.isneginf(np.asarray(vals, dtype=np.float64))


def pool_cosines(z_pool, dtype=np.float64):
    """cos [N, N] of the pool's rows z_pool [N, w], computed in `dtype`."""
    z = np.asarray(z_pool, dtype=dtype)
    s = (z * z).sum(1)
    rn = np.where(s > 0, 1.0 / np.sqrt(np.where(s > 0, s, 1)), 0).astype(dtype)
    return ((z @ z.T) * (rn[:, None] * rn[None, :])).astype(dtype)


def relevance(ids, vals, dtype=np.float64):
    cand = candidates(ids, vals)
    rel = np.zeros(len(vals), dtype)
    if cand.any():
        v = np.asarray(vals)[cand].astype(dtype)
        span = v.max() - v.min()
        if span > 0:
            rel[cand] = (v - v.min()) / span
    return rel


def mmr(ids, vals, z_pool, K, theta, dtype=np.float64, follow=None):
    """One list.  ids [N], vals [N] (float32 scores, best first), z_pool [N, w] the rows of the pool's items (any row for a slot that
    is no candidate).  Returns a dict: pos [T] the picks' pool positions, idx int64 [K] / val fp32 [K] / pen [K] as the entry
    returns them (-1 / 0 / 0 past T), ild, and obj [T, N]: the objective of every candidate still unselected at step t (nan
    elsewhere).  follow: pool positions to pick (a prefix-conditioned replay) instead of the argmax."""
    ids, vals = np.asarray(ids), np.asarray(vals, dtype=np.float32)
    N = len(ids)
    theta = dtype(theta)
    cand = candidates(ids, vals)
    T = min(int(K), int(cand.sum())) if follow is None else len(follow)
    cos = pool_cosines(z_pool, dtype)
    rel = relevance(ids, vals, dtype)
    live = cand.copy()
    pen = np.zeros(N, dtype)
    out = dict(pos=np.zeros(T, np.int64), idx=np.full(K, -1, np.int64), val=np.zeros(K, np.float32), pen=np.zeros(K, dtype),
               obj=np.full((T, N), np.nan, dtype))
    total = dtype(0)
    for t in range(T):
        obj = (dtype(1) - theta) * rel - theta * pen
        out["obj"][t, live] = obj[live]
        if follow is None:
            s = int(np.flatnonzero(live)[np.argmax(obj[live])])          # (argmax returns the first maximum: the lower position)
        else:
            s = int(follow[t])
            assert live[s], "follow: position %d is no unselected candidate at step %d" % (s, t)
        out["pos"][t], out["idx"][t], out["val"][t], out["pen"][t] = s, ids[s], vals[s], pen[s]
        a_t = dtype(0)                                        # the pick's running cosine sum, in selection order
        for q in out["pos"][:t]:
            a_t = a_t + cos[s, q]
        total = total + a_t
        live[s] = False
        pen = cos[:, s].copy() if t == 0 else np.maximum(pen, cos[:, s])
    out["ild"] = dtype(1) - total / dtype(T * (T - 1) // 2) if T > 1 else dtype(0)
    return out


def replay(ids, vals, z, pos, theta, dtype=np.float64):
    """mmr(follow=...) for n lists at once.  ids [n, N] / vals [n, N] the pools, z [I, w] the catalogue's item vectors, pos int
    [n, K] the pool positions of the lists to replay, best first, -1 past a list's end.  Returns obj [n, K, N] (the objective
    of every candidate still unselected at step t given the prefix; nan elsewhere and past the list's end), pen [n, K] the
    picks' penalties (0 past the end) and ild [n].  Only the cosines with the picks are formed (N x K per list, not N x N)."""
    ids, vals, pos = np.asarray(ids), np.asarray(vals, dtype=np.float32), np.asarray(pos)
    n, N = ids.shape
    K = pos.shape[1]
    theta, one = dtype(theta), dtype(1)
    zc = np.asarray(z, dtype=dtype)[np.clip(ids, 0, len(z) - 1)]                     # [n, N, w]
    s = (zc * zc).sum(2)
    rn = np.where(s > 0, 1.0 / np.sqrt(np.where(s > 0, s, 1)), 0).astype(dtype)
    rows = np.arange(n)
    pc = np.clip(pos, 0, N - 1)
    zp, rp = zc[rows[:, None], pc], rn[rows[:, None], pc]                            # [n, K, w], [n, K]
    cos = (np.matmul(zc, zp.transpose(0, 2, 1)) * (rn[:, :, None] * rp[:, None, :])).astype(dtype)
    rel = np.stack([relevance(ids[r], vals[r], dtype) for r in range(n)])
    live = np.stack([candidates(ids[r], vals[r]) for r in range(n)])
    pen = np.zeros((n, N), dtype)
    obj, ppen, total = np.full((n, K, N), np.nan, dtype), np.zeros((n, K), dtype), np.zeros(n, dtype)
    for t in range(K):
        on = pos[:, t] >= 0
        o = (one - theta) * rel - theta * pen
        obj[:, t] = np.where(live & on[:, None], o, np.nan)
        assert live[rows[on], pc[on, t]].all(), "replay: a pick is no unselected candidate at step %d" % t
        ppen[on, t] = pen[rows[on], pc[on, t]]
        if t:                                                 # (cumsum adds serially, in selection order, as the definition does)
            total[on] = total[on] + np.cumsum(cos[rows[on], pc[on, t], :t], axis=1, dtype=dtype)[:, -1]
        live[rows[on], pc[on, t]] = False
        pen = cos[:, :, t].copy() if t == 0 else np.maximum(pen, cos[:, :, t])
    T = (pos >= 0).sum(1)
    pairs = np.maximum(T * (T - 1) // 2, 1).astype(dtype)
    return obj, ppen, np.where(T > 1, one - total / pairs, 0).astype(dtype)


def ild_direct(z_list, dtype=np.float64):
    """1 - the mean of cos over the pairs of the rows z_list [T, w]; 0 for fewer than two rows."""
    T = len(z_list)
    if T < 2:
        return dtype(0)
    cos = pool_cosines(z_list, dtype)
    iu = np.triu_indices(T, 1)
    return dtype(1) - cos[iu].mean(dtype=dtype)
