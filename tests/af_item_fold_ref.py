"""Warm items for AttentiveFashion -- Gi rows for items the model was not trained on, from their first buyers -- restated in numpy on
the CPU (a helper module, not a test module), as include/bprx.h defines bprx_af_fold_in_items.

The score x_ui = sum_k g_uk (sum_l alpha_l(u, i) c_lk(i)) g_ik is linear in g_i: alpha is computed from g_u and the encodings only.
New item r owns w = Gi_r (k numbers, no bias); pair p = (u, o, role) has s_p = +1 (role 0: r is the positive against the catalogue
item o) or -1 (role 1):

    alpha^r = softmax_l( relu((g_u o c_l(r)) W_1 + b_1).W_2 + b_2 )
    m_p     = g_u o (alpha^r_0 c_0(r) + alpha^r_1 c_1(r) + alpha^r_2 c_2(r))
    x_o     = sum_l alpha_l(u, o) t_l,    t_l = sum_k c_lk(o) g_uk Gi_ok
    D_p     = s_p m_p       dc_p = -s_p x_o                                       (formed once)
    the step loop of tests/item_fold_ref.py with rv = n_r for every element

in float64 (the reference) or float32 (one sample of float32 rounding: the scale of the tests' allowances).  C / Cn: the encodings
[3, I, k] / [3, n, k] (colour, edges, class), fp32 values.  uniform_alpha: both attentions replaced by 1/3 (what a wrong attention
forward must not be able to hide behind)."""
import numpy as np

import item_fold_ref as R

ATT = ("attention.W_1", "attention.b_1", "attention.W_2", "attention.b_2")


def attention(gu, c, att, dtype=np.float64, uniform_alpha=False):
    """alpha [3, P] of the rows gu [P, k] against the encodings c [3, P, k]."""
    f = dtype
    if uniform_alpha:
        return np.full(c.shape[:2], f(1) / f(3), f)
    W1, b1, W2, b2 = (np.asarray(a).astype(f) for a in att)
    hid = np.maximum((gu[None] * c) @ W1 + b1, f(0))
    a = hid @ W2.reshape(-1) + b2.reshape(())
    e = np.exp(a - a.max(0, keepdims=True))
    return (e / e.sum(0, keepdims=True)).astype(f)


def pair_terms(Gu, Gi, C, att, c_r, user, other, role, dtype=np.float64, uniform_alpha=False):
    """(D [n_r, k], dc [n_r]) of one item's pairs; c_r [3, k]: the item's encodings."""
    f = dtype
    s = np.where(np.asarray(role) == 0, f(1), f(-1)).astype(f)
    gu = Gu[user]
    cr = np.broadcast_to(c_r[:, None, :], (3, len(user), c_r.shape[1]))
    al_r = attention(gu, cr, att, f, uniform_alpha)
    m = gu * (al_r[:, :, None] * cr).sum(0, dtype=f)
    co = C[:, other, :]
    al_o = attention(gu, co, att, f, uniform_alpha)
    t = (co * (gu * Gi[other])[None]).sum(-1, dtype=f)
    xo = (al_o * t).sum(0, dtype=f)
    return (s[:, None] * m).astype(f), (-s * xo).astype(f)


def fold_in_items(Gu, Gi, C, att, Cn, pair_ptr, user, other, role, Gi0, steps, lr, reg, optimizer="sgd", dtype=np.float64,
                  uniform_alpha=False, beta1=0.9, beta2=0.999, eps=1e-7):
    """{'Gi' [n, k], 'loss' [n] (loss_T, before the last update), 'loss_first' [n], 'grads' [n][T, k], 'D' [n][n_r, k], 'dc' [n][n_r]}
    as arrays of `dtype`."""
    f = dtype
    c = lambda x: np.asarray(x, np.float32).astype(f)
    Gu, Gi, C, Cn, W = c(Gu), c(Gi), c(C), c(Cn), c(Gi0).copy()
    att = tuple(c(a) for a in att)
    k = Gi.shape[1]
    ptr = np.asarray(pair_ptr, np.int64)
    user, other, role = (np.asarray(x, np.int64) for x in (user, other, role))
    n = len(ptr) - 1
    lr, b1, b2, eps = f(lr), f(beta1), f(beta2), f(eps)
    one = f(1)
    loss, first, grads, Ds, dcs = np.zeros(n, f), np.zeros(n, f), [], [], []
    for r in range(n):
        sl = slice(ptr[r], ptr[r + 1])
        nr = int(ptr[r + 1] - ptr[r])
        G = np.zeros((steps if nr else 0, k), f)
        grads.append(G)
        if nr == 0:
            Ds.append(np.zeros((0, k), f)); dcs.append(np.zeros(0, f))
            continue
        D, dc = pair_terms(Gu, Gi, C, att, Cn[:, r, :], user[sl], other[sl], role[sl], f, uniform_alpha)
        Ds.append(D); dcs.append(dc)
        rv = np.full(k, f(nr), f)
        w = W[r].copy()
        m, v = np.zeros_like(w), np.zeros_like(w)
        for t in range(1, steps + 1):
            lt, g = R.loss_and_grad(w, D, dc, rv, reg, f)
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
    return {"Gi": W, "loss": loss, "loss_first": first, "grads": grads, "D": Ds, "dc": dcs}


def scores(Gu, att, C_rows, Gi_rows, dtype=np.float64):
    """(x [U, n], alpha [U, n, 3]) of every user against the item rows C_rows [3, n, k] / Gi_rows [n, k]."""
    f = dtype
    Gu, C, Gi = (np.asarray(a).astype(f) for a in (Gu, C_rows, Gi_rows))
    xs, als = [], []
    for u in range(Gu.shape[0]):
        gu = np.broadcast_to(Gu[u], Gi.shape)
        al = attention(gu, C, att, f)
        t = (C * (gu * Gi)[None]).sum(-1, dtype=f)
        xs.append((al * t).sum(0, dtype=f)); als.append(al.T)
    return np.stack(xs), np.stack(als)
