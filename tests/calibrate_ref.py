"""Greedy calibration of a top-N pool toward the class mix of a history, restated in numpy on the CPU (a helper module, not a test
module), as include/bprx.h defines bprx_calibrate:

    candidates: the pool slots with id >= 0 and score > -inf (M of them); the class of a slot is item_class[id], -1 for an id
    outside the table or a value outside [0, C)
    cnt_c = the history's entries of class c (ids outside the table and classless items are not counted), H = sum cnt_c, p = cnt / H
    rel_c = (v_c - v_min) / (v_max - v_min) over the candidates, 0 for a flat pool
    den_g(m) = (1 - alpha) m / L + alpha p_g,  L = t + 1 at step t, n_g = the picks of class g so far
    delta_g = p_g log(den_g(n_g) / den_g(n_g + 1)), 0 when p_g = 0 or for a classless candidate
    obj_c = (1 - lambda) rel_c - lambda delta_class(c); min(K, M) picks, each the unselected candidate with the largest obj_c, ties
    to the lower pool position; gain = -delta of the pick at its step
    kl = sum over p_c > 0 of p_c log(p_c / den_c(n_c)) at L = T, of the pool's first T candidates ([0]) and of the list ([1]); 0
    when H = 0 or T = 0

in float64 (the reference) or float32 (one sample of float32 rounding: the scale of the tests' allowances).  `replay` follows a
given list (pool positions) instead of choosing: the objective of every remaining candidate is then computed at each step given
that prefix, which is how a GPU list is judged without comparing list identities across precisions."""
import numpy as np


def candidates(ids, vals):
    return (np.asarray(ids) >= 0) & ~np.isneginf(np.asarray(vals, dtype=np.float64))


def relevance(ids, vals, dtype=np.float64):
    """rel [n, N] of the pools ids / vals [n, N]."""
    ids, vals = np.atleast_2d(np.asarray(ids)), np.atleast_2d(np.asarray(vals, dtype=np.float32))
    cand = candidates(ids, vals)
    v = vals.astype(dtype)
    with np.errstate(all="ignore"):
        vmax = np.where(cand, v, -np.inf).max(1, keepdims=True)
        vmin = np.where(cand, v, np.inf).min(1, keepdims=True)
        span = (vmax - vmin).astype(dtype)
        rel = np.where(cand & (span > 0), (v - vmin) / span, 0)
    return rel.astype(dtype)


def classes_of(ids, item_class, C):
    """The class of every pool slot [n, N]: -1 for a slot without an id, an id outside the table or a value outside [0, C)."""
    ids, table = np.asarray(ids, dtype=np.int64), np.asarray(item_class, dtype=np.int64)
    ok = (ids >= 0) & (ids < table.size)
    c = np.where(ok, table[np.clip(ids, 0, table.size - 1)], -1)
    return np.where((c >= 0) & (c < C), c, -1)


def history_counts(hists, item_class, C):
    """cnt int64 [n, C] of the n histories (lists of ids; a repeated id counts every time)."""
    table = np.asarray(item_class, dtype=np.int64)
    cnt = np.zeros((len(hists), C), np.int64)
    for r, h in enumerate(hists):
        it = np.asarray(h, dtype=np.int64).reshape(-1)
        c = table[it[(it >= 0) & (it < table.size)]]
        cnt[r] = np.bincount(c[(c >= 0) & (c < C)], minlength=C)
    return cnt


def _den(oma, m, L, ap, dtype):
    return ((oma * m.astype(dtype)).astype(dtype) / L).astype(dtype) + ap


def _kl(p, ncls, T, alpha, dtype):
    """kl [n] of the lists whose class counts are ncls [n, C], T [n] picks each."""
    oma = dtype(1) - dtype(alpha)
    L = np.maximum(T, 1).astype(dtype)[:, None]
    with np.errstate(all="ignore"):
        den = _den(oma, ncls, L, (dtype(alpha) * p).astype(dtype), dtype)
        term = np.where(p > 0, p * np.log(np.where(p > 0, p / den, 1).astype(dtype)).astype(dtype), 0).astype(dtype)
    return np.where(T > 0, term.sum(1, dtype=dtype), 0).astype(dtype)


def _run(ids, vals, item_class, hists, K, lam, alpha, dtype, pos=None, C=None):
    ids, vals = np.atleast_2d(np.asarray(ids)), np.atleast_2d(np.asarray(vals, dtype=np.float32))
    n, N = ids.shape
    table = np.asarray(item_class, dtype=np.int64)
    C = max(1, int(table.max()) + 1 if table.size else 1) if C is None else int(C)
    lam, alpha, one = dtype(lam), dtype(alpha), dtype(1)
    oml, oma = one - lam, one - alpha
    cc = classes_of(ids, table, C)                                    # [n, N]
    cnt = history_counts(hists, table, C)
    H = cnt.sum(1)
    with np.errstate(all="ignore"):
        p = np.where(H[:, None] > 0, cnt.astype(dtype) / np.maximum(H, 1).astype(dtype)[:, None], 0).astype(dtype)   # [n, C]
    rows = np.arange(n)
    pcand = np.where(cc >= 0, p[rows[:, None], np.maximum(cc, 0)], 0).astype(dtype)     # p of every slot's class
    ap = (alpha * pcand).astype(dtype)
    rel1 = (oml * relevance(ids, vals, dtype)).astype(dtype)
    live = candidates(ids, vals)
    M = live.sum(1)
    follow = pos is not None
    if follow:
        pos = np.asarray(pos, dtype=np.int64)
        K = pos.shape[1]
    else:
        pos = np.full((n, K), -1, np.int64)
    ncls = np.zeros((n, C), np.int64)
    obj, gain = np.full((n, K, N), np.nan, dtype), np.zeros((n, K), dtype)
    for t in range(K):
        on = (pos[:, t] >= 0) if follow else (M > t)
        if not on.any():
            break
        L = dtype(t + 1)
        m = np.where(cc >= 0, ncls[rows[:, None], np.maximum(cc, 0)], 0)
        with np.errstate(all="ignore"):
            ratio = np.where(pcand > 0, _den(oma, m, L, ap, dtype) / _den(oma, m + 1, L, ap, dtype), 1).astype(dtype)
            delta = np.where(pcand > 0, pcand * np.log(ratio).astype(dtype), 0).astype(dtype)
        o = (rel1 - (lam * delta).astype(dtype)).astype(dtype)
        obj[:, t] = np.where(live & on[:, None], o, np.nan)
        if not follow:
            pos[on, t] = np.argmax(np.where(live, o, -np.inf), axis=1)[on]   # (the first maximum: the lower position)
        s = np.maximum(pos[:, t], 0)
        assert live[rows[on], s[on]].all(), "a pick is no unselected candidate at step %d" % t
        gain[on, t] = dtype(0) - delta[rows[on], s[on]]
        live[rows[on], s[on]] = False
        g = cc[rows, s]
        bump = on & (g >= 0)
        ncls[rows[bump], g[bump]] += 1
    T = (pos >= 0).sum(1)
    cand = candidates(ids, vals)
    first = cand & (np.cumsum(cand, axis=1) <= T[:, None])             # the pool's first T candidates: the plain list
    nplain = np.zeros((n, C), np.int64)
    for r in range(n):
        c = cc[r][first[r]]
        nplain[r] = np.bincount(c[c >= 0], minlength=C)
    kl = np.stack([_kl(p, nplain, T, alpha, dtype), _kl(p, ncls, T, alpha, dtype)], axis=1)
    return dict(pos=pos, obj=obj, gain=gain, kl=kl, cls=np.where(pos >= 0, cc[rows[:, None], np.maximum(pos, 0)], -1), H=H, T=T)


def greedy(ids, vals, item_class, hists, K, lam, alpha, dtype=np.float64, C=None):
    """The calibrated lists of the pools ids / vals [n, N] (one pool: [N]) with the histories hists (n lists of ids).  Returns a dict:
    pos int64 [n, K] the picks' pool positions (-1 past T), idx / val / cls / gain [n, K] as the entry returns them (-1 / 0 / -1 /
    0 past T), kl [n, 2], H [n], T [n] and obj [n, K, N] (the objective of every candidate still unselected at step t; nan
    elsewhere).  C: the number of classes (None: the table's largest + 1)."""
    ids2, vals2 = np.atleast_2d(np.asarray(ids)), np.atleast_2d(np.asarray(vals, dtype=np.float32))
    out = _run(ids2, vals2, item_class, hists, int(K), lam, alpha, dtype, None, C)
    pc = np.maximum(out["pos"], 0)
    out["idx"] = np.where(out["pos"] >= 0, np.take_along_axis(ids2.astype(np.int64), pc, axis=1), -1)
    out["val"] = np.where(out["pos"] >= 0, np.take_along_axis(vals2, pc, axis=1), np.float32(0)).astype(np.float32)
    return out


def replay(ids, vals, item_class, hists, pos, lam, alpha, dtype=np.float64, C=None):
    """The lists whose pool positions are pos int [n, K] (best first, -1 past a list's end), followed instead of chosen.  Returns
    obj [n, K, N] (the objective of every candidate still unselected at step t given the prefix; nan for non-candidates, the picked
    and past the list's end), gain [n, K] (0 past the end) and kl [n, 2]."""
    out = _run(ids, vals, item_class, hists, None, lam, alpha, dtype, pos, C)
    return out["obj"], out["gain"], out["kl"]
