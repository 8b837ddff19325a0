"""Warm items -- Gi / Bi rows for items the model was not trained on, from their first buyers -- restated in numpy on the CPU (a
helper module, not a test module).

New item r owns w = [Gi_r (k) | Bi_r (1)] and, with a visual part, its projection row Pn_r; every user-side and catalogue
parameter is frozen.  Its pairs p in [pair_ptr[r], pair_ptr[r+1]) are triples (u_p, o_p, role_p): role 0, the new item is the
positive of the reference's triplet (u, r, o), s_p = +1; role 1, the negative of (u, o, r), s_p = -1.  With n_r pairs, n_pos in
role 0 and n_neg in role 1:

    a_p = [Gu_u | 1]
    v_p = Tu_u.(Pn_r[0:d] - P_o[0:d]) + (Pn_r[d] - P_o[d]) - Bi_o - Gu_u.Gi_o         (d = 0: -Bi_o - Gu_u.Gi_o)
    D_p = s_p a_p      dc_p = s_p v_p                                                 (formed once)
    rv  = [n_r, ..., n_r | n_pos + c_neg n_neg]
    for t = 1 .. T:
        x_p = w.D_p + dc_p      s = sigmoid(-clip(x_p, -80, 1e8))     (inclusive bounds, zero gradient outside)
        g = sum_p (-s D_p) + 2 reg rv o w                              (summed in pair order)
        loss_t = sum_p softplus(-clip(x_p)) + reg sum(rv o w o w)
        sgd:  w <- w - lr g
        adam: m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g g;  w <- w - lr_t m / (sqrt(v) + eps),  slots from zero,
              lr_t = lr sqrt(1 - b2^t) / (1 - b1^t)

in float64 (the reference) or float32 (one sample of float32 rounding: the scale of the tests' allowances).  P / Pn: the [I, >= d + 1]
/ [n, >= d + 1] projections F.[E|Bp] (fp32 values).  An item without pairs keeps its rows and has loss 0."""
import numpy as np


def pair_terms(Gu, Tu, Gi, Bi, P, Pn_r, user, other, role, dtype=np.float64):
    """(D [n_r, k + 1], dc [n_r]) of one item's pairs."""
    f = dtype
    s = np.where(np.asarray(role) == 0, f(1), f(-1)).astype(f)
    gu = Gu[user]
    v = -Bi[other] - (gu * Gi[other]).sum(1, dtype=f)
    if Tu is not None:
        d = Tu.shape[1]
        v = v + (Tu[user] * (Pn_r[None, :d] - P[other, :d])).sum(1, dtype=f) + (Pn_r[d] - P[other, d])
    a = np.concatenate([gu, np.ones((len(user), 1), f)], 1)
    return (s[:, None] * a).astype(f), (s * v).astype(f)


def loss_and_grad(w, D, dc, rv, reg, dtype=np.float64):
    """(loss, g) of one item at the row w."""
    f = dtype
    one = f(1)
    x = D @ w + dc
    inr = (x >= f(-80)) & (x <= f(1e8))
    xc = np.clip(x, f(-80), f(1e8))
    with np.errstate(over="ignore"):
        s = np.where(inr, one / (one + np.exp(x)), f(0)).astype(f)
    g = (-(s[:, None] * D)).sum(0, dtype=f) + f(2) * f(reg) * rv * w
    lt = np.logaddexp(f(0), -xc).sum(dtype=f) + f(reg) * (rv * w * w).sum(dtype=f)
    return f(lt), g.astype(f)


def fold_in_items(Gu, Tu, Gi, Bi, P, Pn, pair_ptr, user, other, role, Gi0, Bi0, steps, lr, reg, optimizer="sgd", dtype=np.float64,
                  c_neg=0.1, beta1=0.9, beta2=0.999, eps=1e-7):
    """{'Gi' [n, k], 'Bi' [n], 'loss' [n] (loss_T, before the last update), 'loss_first' [n] (loss_1), 'grads' [n][T, k + 1] (g of
    every step)} as arrays of `dtype`.  Tu / P / Pn: None for a model without a visual part."""
    f = dtype
    c = lambda x: None if x is None else np.asarray(x, np.float32).astype(f)
    Gu, Tu, Gi, P, Pn = c(Gu), c(Tu), c(Gi), c(P), c(Pn)
    Bi = c(Bi).reshape(-1)
    W = np.concatenate([c(Gi0), c(Bi0).reshape(-1, 1)], 1)
    k = Gi.shape[1]
    ptr = np.asarray(pair_ptr, np.int64)
    user, other, role = (np.asarray(x, np.int64) for x in (user, other, role))
    n = len(ptr) - 1
    lr, b1, b2, eps = f(lr), f(beta1), f(beta2), f(eps)
    one = f(1)
    loss, first, grads = np.zeros(n, f), np.zeros(n, f), []
    for r in range(n):
        sl = slice(ptr[r], ptr[r + 1])
        nr = int(ptr[r + 1] - ptr[r])
        G = np.zeros((steps if nr else 0, k + 1), f)
        grads.append(G)
        if nr == 0:
            continue
        D, dc = pair_terms(Gu, Tu, Gi, Bi, P, None if Pn is None else Pn[r], user[sl], other[sl], role[sl], f)
        npos = int((role[sl] == 0).sum())
        rv = np.full(k + 1, f(nr), f)
        rv[k] = f(npos) + f(c_neg) * f(nr - npos)
        w = W[r].copy()
        m, v = np.zeros_like(w), np.zeros_like(w)
        for t in range(1, steps + 1):
            lt, g = loss_and_grad(w, D, dc, rv, reg, f)
            if t == 1:
                first[r] = lt
            loss[r] = lt
            G[t - 1] = g
            if optimizer == "sgd":
                w = w - lr * g
            else:
                lr_t = lr * np.sqrt(one - b2 ** f(t)) / (one - b1 ** f(t))
                m = m * b1 + g * (one - b1)
                v = v * b2 + (g * g) * (one - b2)
                w = w - lr_t * m / (np.sqrt(v) + eps)
            w = w.astype(f)
        W[r] = w
    return {"Gi": W[:, :k].copy(), "Bi": W[:, k].copy(), "loss": loss, "loss_first": first, "grads": grads}


def scores(Gu, Tu, Gi_rows, Bi_rows, Pn, dtype=np.float64):
    """The warm block [U, n]: Bi_j + Gu_u.Gi_j (+ Tu_u.Pn_j[0:d] + Pn_j[d])."""
    f = dtype
    c = lambda x: np.asarray(x).astype(f)
    s = c(Bi_rows).reshape(-1)[None, :] + c(Gu) @ c(Gi_rows).T
    if Tu is not None:
        d = np.asarray(Tu).shape[1]
        Pn = c(Pn)
        s = s + c(Tu) @ Pn[:, :d].T + Pn[:, d][None, :]
    return s
