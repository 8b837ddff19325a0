"""Folding new users into AttentiveFashion, restated in torch on the CPU (a helper module, not a test module).

For new user r with pairs (i_p, j_p), p in [pair_ptr[r], pair_ptr[r+1]), n_r of them, with Gi, the four attention tensors and the
dropout-off encodings C [3, I, k] (colour, edges, class: what bprx_af_encode returns) held fixed, g starting at the caller's row:

    pre_l(item) = (g * c_l) W_1 + b_1      a_l = relu(pre_l).W_2 + b_2      alpha = softmax_l(a)
    t_l = sum_k g_k c_lk Gi_k              x = sum_l alpha_l t_l
    d_p = clip(x(i_p) - x(j_p), -80, 1e8)  loss_t = sum_p softplus(-d_p) + reg n_r |g|^2
    grad = d loss_t / d g                  (autograd on g only; the clip passes no gradient outside its inclusive bounds)
    sgd:  g <- g - lr grad
    adam: m = b1 m + (1 - b1) grad;  v = b2 v + (1 - b2) grad^2;  g <- g - lr_t m / (sqrt(v) + eps),  slots from zero,
          lr_t = lr sqrt(1 - b2^t) / (1 - b1^t)

in float64 (the reference) or float32 (one sample of float32 rounding: the scale of the tests' allowances).  `fixed_alpha=True` drops
the softmax derivative (alpha is a constant of the tape): the trajectory a backward without the attention term would give.  A user
without pairs keeps its row and has loss 0."""
import numpy as np
import torch
import torch.nn.functional as Fn

KINK = 1e-5            # a pre-activation closer to zero than this may fall on the other side of the relu in float32


def user_loss(g, c, gi, nr, W1, b1, W2, b2, reg, fixed_alpha=False):
    """loss_t of one user.  c [3, 2 n_r, k] and gi [2 n_r, k]: the rows of the n_r positives, then of the n_r negatives.
    Returns (loss, pre [3, 2 n_r, h], t - x [3, 2 n_r])."""
    pre = (g * c) @ W1 + b1
    a = torch.relu(pre) @ W2.reshape(-1) + b2.reshape(())
    alpha = torch.softmax(a, 0)
    if fixed_alpha:
        alpha = alpha.detach()
    t = (g * c * gi).sum(-1)
    x = (alpha * t).sum(0)
    d = torch.clamp(x[:nr] - x[nr:], -80.0, 1e8)
    loss = Fn.softplus(-d).sum() + reg * nr * (g * g).sum()
    return loss, pre, t - x


def fold_in(C, Gi, W1, b1, W2, b2, pair_ptr, pos, neg, G0, steps, lr, reg, optimizer="sgd", dtype=torch.float64, fixed_alpha=False,
            beta1=0.9, beta2=0.999, eps=1e-7):
    """{'Gu' [n, k], 'loss' [n] (loss_T, before the last update), 'loss_first' [n] (loss_1), and per user over all steps:
    'min_pre' the smallest |pre| (inf without pairs), 'kinks' the number of pre-activations with |pre| < KINK, 'min_grad' the
    smallest |grad element|, 'tx' the largest |t_l - x|} as numpy arrays."""
    f = dtype
    cv = lambda a: torch.as_tensor(np.asarray(a)).to(f)         # (the values as given: fp32 tables, or a float64 C)
    C, Gi, W1, b1, W2, b2 = (cv(a) for a in (C, Gi, W1, b1, W2, b2))
    G = cv(G0).clone()
    ptr = np.asarray(pair_ptr, np.int64)
    pos, neg = np.asarray(pos, np.int64), np.asarray(neg, np.int64)
    n = len(ptr) - 1
    loss, first = np.zeros(n), np.zeros(n)
    min_pre, kinks, min_grad, tx = np.full(n, np.inf), np.zeros(n, np.int64), np.full(n, np.inf), np.zeros(n)
    for r in range(n):
        items = torch.as_tensor(np.concatenate([pos[ptr[r]:ptr[r + 1]], neg[ptr[r]:ptr[r + 1]]]))
        nr = items.numel() // 2
        if nr == 0:
            continue
        c, gi = C[:, items], Gi[items]
        g = G[r].clone()
        m, v = torch.zeros_like(g), torch.zeros_like(g)
        for t in range(1, steps + 1):
            g = g.detach().requires_grad_(True)
            lt, pre, dtx = user_loss(g, c, gi, nr, W1, b1, W2, b2, reg, fixed_alpha)
            (gr,) = torch.autograd.grad(lt, g)
            ap = pre.detach().abs()
            min_pre[r] = min(min_pre[r], ap.min().item())
            kinks[r] += int((ap < KINK).sum().item())
            min_grad[r] = min(min_grad[r], gr.abs().min().item())
            tx[r] = max(tx[r], dtx.detach().abs().max().item())
            if t == 1:
                first[r] = lt.item()
            loss[r] = lt.item()
            g = g.detach()
            if optimizer == "sgd":
                g = g - lr * gr
            else:
                lr_t = lr * np.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t)
                m = m * beta1 + gr * (1 - beta1)
                v = v * beta2 + gr * gr * (1 - beta2)
                g = g - lr_t * m / (torch.sqrt(v) + eps)
            g = g.to(f)
        G[r] = g
    return {"Gu": G.numpy(), "loss": loss, "loss_first": first, "min_pre": min_pre, "kinks": kinks, "min_grad": min_grad, "tx": tx}
