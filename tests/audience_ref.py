"""Audiences restated in torch / numpy on the CPU (a helper module, not a test module): the score block item-major,

    catalogue item q:   out[q][u] = Bi_q + Gu_u.Gi_q (+ Tu_u.(f_q E) + f_q.Bp)          (bprx_score_block's score, transposed)
    new row j of F:     out[j][u] = Tu_u.(f_j E) + f_j.Bp                               (bprx_score_new_block's, transposed)

in float64 (the reference) or float32 (one sample of float32 rounding: the scale of the tests' allowances), the owners of every
item (the transpose of the training lists) and the masked lists (value descending, id ascending).  The visual part is
tests/new_items_ref.py's (bf16 features meet the bf16-ROUNDED [E|Bp], as every projection of the engine does); a table set
without Tu is BPRMF's."""
import numpy as np
import torch

import new_items_ref as N


def _t(x, dtype):
    return (x.detach().cpu() if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))).to(dtype)


def user_major(t, feat_dtype="fp32", dtype=torch.float64, F=None):
    """[U, I] scores of the catalogue (F None) or [U, n] visual scores of the rows of F, as a numpy array of `dtype`."""
    U = _t(t["Gu"], dtype).shape[0]
    if F is not None:
        return N.scores(t["Tu"], F, t["E"], t["Bp"], 0, U, feat_dtype, dtype)
    s = _t(t["Bi"], dtype).reshape(-1)[None, :] + _t(t["Gu"], dtype) @ _t(t["Gi"], dtype).T
    if t.get("Tu") is not None:
        s = s + torch.as_tensor(N.scores(t["Tu"], t["F"], t["E"], t["Bp"], 0, U, feat_dtype, dtype))
    return s.numpy()


def scores(t, feat_dtype="fp32", dtype=torch.float64, F=None):
    """The audience block of every item: [I, U] (F None) or [n, U], the transpose of user_major."""
    return np.ascontiguousarray(user_major(t, feat_dtype, dtype, F).T)


def owners(training_list, num_items):
    """Per item the sorted list of the users whose training list names it, each once."""
    own = [set() for _ in range(num_items)]
    for u, items in enumerate(training_list):
        for i in items:
            if 0 <= int(i) < num_items:
                own[int(i)].add(u)
    return [sorted(s) for s in own]


def masked(S, own):
    """A copy of the rows S [n, U] with -inf at each row's owners."""
    out = np.array(S, copy=True)
    for r, l in enumerate(own):
        out[r, list(l)] = -np.inf
    return out


def lists(S, own, k):
    """(ids int64 [n, kk], vals [n, kk]) of the masked rows, kk = min(k, U): value descending, id ascending; the slots past a
    row's non-owners hold -1 / -inf."""
    m = masked(S, own)
    n, U = m.shape
    kk = min(k, U)
    ids, vals = np.full((n, kk), -1, np.int64), np.full((n, kk), -np.inf, m.dtype)
    for r in range(n):
        order = np.lexsort((np.arange(U), -m[r].astype(np.float64)))[:kk]
        live = order[m[r][order] != -np.inf]
        ids[r, :live.size], vals[r, :live.size] = live, m[r][live]
    return ids, vals
