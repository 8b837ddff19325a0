"""The nearest owned items of a list entry restated in numpy on the CPU (a helper module, not a test module), as include/bprx.h
defines bprx_because:

    the history of a list: catalogue ids, an entry is identified by its position
    candidates of an entry: every position of the history, except (catalogue items only) those whose id is the entry's own
    cos(q, l) = <z_q, z_l> (rn_q rn_l),  rn = 1 / |z|, 0 for a zero row                      (z: similar_ref.item_vectors)
    the min(L, M) candidates with the largest cosine, by descending cosine, equal values to the lower position

in float64 (the reference) or float32 (one sample of float32 rounding: the scale of the tests' allowances)."""
import numpy as np


def _rn(z, dtype):
    s = (z * z).sum(-1)
    return np.where(s > 0, 1.0 / np.sqrt(np.where(s > 0, s, 1)), 0).astype(dtype)


def cosines(zq, zh, dtype=np.float64):
    """cos [K, H] of the rows zq [K, w] with the rows zh [H, w], computed in `dtype`."""
    zq, zh = np.asarray(zq, dtype=dtype), np.asarray(zh, dtype=dtype)
    return ((zq @ zh.T) * (_rn(zq, dtype)[:, None] * _rn(zh, dtype)[None, :])).astype(dtype)


def nearest(cos_row, cand, L):
    """Positions of the min(L, M) candidates of one entry: descending cosine (-0 == +0), equal values by ascending position."""
    pos = np.flatnonzero(cand)
    return pos[np.argsort(-(cos_row[pos] + 0.0), kind="stable")][:L]


def because(items, hist, z, L, dtype=np.float64, zq=None):
    """One list.  items int [K]: catalogue ids (zq None) or rows of zq [nq, w] (items outside the catalogue), < 0 = an empty slot;
    hist int [H]: the history's catalogue ids; z [I, w] the catalogue's item vectors.  Returns a dict: item int64 [K, L] /
    cos [K, L] as the entry returns them (-1 / 0 past the candidates), cnt int64 [K], pos int64 [K, L] (the picks' history
    positions, -1 past them) and all [K, H]: the cosine of every candidate (nan where the position is none)."""
    items, hist = np.asarray(items, dtype=np.int64).reshape(-1), np.asarray(hist, dtype=np.int64).reshape(-1)
    K, H = len(items), len(hist)
    src = z if zq is None else zq
    rows = np.asarray(src, dtype=dtype)[np.clip(items, 0, len(src) - 1)]
    cos = cosines(rows, np.asarray(z, dtype=dtype)[np.clip(hist, 0, len(z) - 1)], dtype) if H else np.zeros((K, 0), dtype)
    cand = np.repeat((items >= 0)[:, None], H, axis=1)
    if zq is None:
        cand &= hist[None, :] != items[:, None]
    out = dict(item=np.full((K, L), -1, np.int64), cos=np.zeros((K, L), dtype), cnt=cand.sum(1).astype(np.int64),
               pos=np.full((K, L), -1, np.int64), all=np.where(cand, cos, np.nan).astype(dtype))
    for q in range(K):
        p = nearest(cos[q], cand[q], L)
        out["pos"][q, :len(p)], out["item"][q, :len(p)], out["cos"][q, :len(p)] = p, hist[p], cos[q, p]
    return out


def because_lists(list_idx, hists, z, L, dtype=np.float64, zq=None):
    """because() for the n lists of a call: list_idx int [n, K], hists: n histories.  Returns item [n, K, L], cos [n, K, L],
    cnt [n, K], pos [n, K, L] and all [n, K, Hmax] (nan past a history's end and where a position is no candidate)."""
    n, K = np.shape(list_idx)
    Hmax = max([len(h) for h in hists] + [1])
    res = [because(list_idx[r], hists[r], z, L, dtype, zq) for r in range(n)]
    allc = np.full((n, K, Hmax), np.nan, dtype)
    for r, o in enumerate(res):
        allc[r, :, :o["all"].shape[1]] = o["all"]
    st = lambda name: np.stack([o[name] for o in res]) if n else np.zeros((0, K, L))
    return st("item"), st("cos"), st("cnt"), st("pos"), allc
