"""Folding in users the model was not trained on, restated in numpy on the CPU (a helper module, not a test module).

For new user r with pairs (i_p, j_p), p in [pair_ptr[r], pair_ptr[r+1]), n_r of them, and every item-side parameter frozen:

    z_i = [Gi_i | P_i[0:d]]     c_i = Bi_i + P_i[d]     (BPRMF: d = 0, no P, c_i = Bi_i)
    D_p = z_i - z_j             dc_p = c_i - c_j        (formed once)
    w = [gamma | theta] starts at the caller's row; for t = 1 .. T:
        x_p = w.D_p + dc_p      s_p = sigmoid(-clip(x_p, -80, 1e8))     (inclusive bounds, zero gradient outside)
        g = sum_p (-s_p D_p) + 2 reg n_r w                                (summed in pair order)
        loss_t = sum_p softplus(-clip(x_p)) + reg n_r |w|^2
        sgd:  w <- w - lr g
        adam: m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g g;  w <- w - lr_t m / (sqrt(v) + eps),  slots from zero,
              lr_t = lr sqrt(1 - b2^t) / (1 - b1^t)

in float64 (the reference) or float32 (one sample of float32 rounding: the scale of the tests' allowances).  P: the [I, >= d + 1]
table of item projections F.[E|Bp] the engine holds (fp32 values).  A user without pairs keeps its row and has loss 0."""
import numpy as np


def fold_in(Gi, Bi, P, pair_ptr, pos, neg, Gu0, Tu0, steps, lr, reg, optimizer="sgd", dtype=np.float64,
            beta1=0.9, beta2=0.999, eps=1e-7):
    """{'Gu' [n, k], 'Tu' [n, d] or None, 'loss' [n] (loss_T, before the last update), 'loss_first' [n] (loss_1),
    'grads' [n][T, k + d] (g of every step)} as arrays of `dtype`."""
    f = dtype
    Gi, Bi = np.asarray(Gi, np.float32).astype(f), np.asarray(Bi, np.float32).reshape(-1).astype(f)
    k = Gi.shape[1]
    d = 0 if Tu0 is None else np.asarray(Tu0).shape[1]
    if d:
        P = np.asarray(P, np.float32).astype(f)
        Z, c = np.concatenate([Gi, P[:, :d]], 1), Bi + P[:, d]
        W = np.concatenate([np.asarray(Gu0, np.float32), np.asarray(Tu0, np.float32)], 1).astype(f)
    else:
        Z, c = Gi, Bi
        W = np.asarray(Gu0, np.float32).astype(f)
    ptr = np.asarray(pair_ptr, np.int64)
    pos, neg = np.asarray(pos, np.int64), np.asarray(neg, np.int64)
    n = len(ptr) - 1
    lr, reg, b1, b2, eps = f(lr), f(reg), f(beta1), f(beta2), f(eps)
    one, two = f(1), f(2)
    loss, first, grads = np.zeros(n, f), np.zeros(n, f), []
    for r in range(n):
        i, j = pos[ptr[r]:ptr[r + 1]], neg[ptr[r]:ptr[r + 1]]
        nr = len(i)
        G = np.zeros((steps if nr else 0, W.shape[1]), f)
        grads.append(G)
        if nr == 0:
            continue
        D, dc = Z[i] - Z[j], c[i] - c[j]
        w = W[r].copy()
        m, v = np.zeros_like(w), np.zeros_like(w)
        for t in range(1, steps + 1):
            x = D @ w + dc
            inr = (x >= f(-80)) & (x <= f(1e8))
            xc = np.clip(x, f(-80), f(1e8))
            with np.errstate(over="ignore"):
                s = np.where(inr, one / (one + np.exp(x)), f(0)).astype(f)
            g = (-(s[:, None] * D)).sum(0, dtype=f) + two * reg * f(nr) * w
            lt = np.logaddexp(f(0), -xc).sum(dtype=f) + reg * f(nr) * (w * w).sum(dtype=f)
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
    return {"Gu": W[:, :k].copy(), "Tu": W[:, k:].copy() if d else None, "loss": loss, "loss_first": first, "grads": grads}


def scores(Gi, Bi, P, Gu, Tu, dtype=np.float64):
    """The score rows [n, I] of folded-in users: Bi + Gu.Gi (+ Tu.P[:, :d] + P[:, d])."""
    f = dtype
    s = np.asarray(Bi, np.float32).reshape(-1).astype(f)[None, :] + np.asarray(Gu).astype(f) @ np.asarray(Gi, np.float32).astype(f).T
    if Tu is not None:
        d = np.asarray(Tu).shape[1]
        P = np.asarray(P, np.float32).astype(f)
        s = s + np.asarray(Tu).astype(f) @ P[:, :d].T + P[:, d][None, :]
    return s
