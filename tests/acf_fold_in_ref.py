"""Folding new users into ACF, restated in torch on the CPU (a helper module, not a test module).

For new user r with history entries l (item ids, repeats allowed) and pairs (i_p, j_p), n_r of them, with every table frozen and g
starting at the caller's row (include/bprx.h, bprx_acf_fold_in):

    s_lm = W1c.relu(Wcu^T g + Wci^T f_lm + bc0) + bc1     beta_l = softmax_m(s_l)
    t_l  = W1i.relu(Wiu^T g + Wiv^T Gi_l + Wip^T Pi_l + Wix^T sum_m beta_lm f_lm + bi0) + bi1     alpha = softmax_l(t)
    g'   = g + sum_l alpha_l Pi_l                 (g' = g for an empty history)
    x_p  = g'.(Gi_i - Gi_j)    d_p = clip(x_p, -80, 1e8)    loss_t = sum_p softplus(-d_p) + reg n_r |g|^2
    grad = d loss_t / d g      (autograd on g only, nothing detached; the clip passes no gradient outside its inclusive bounds)
    sgd:  g <- g - lr grad
    adam: m = b1 m + (1 - b1) grad;  v = b2 v + (1 - b2) grad^2;  g <- g - lr_t m / (sqrt(v) + eps),  slots from zero,
          lr_t = lr sqrt(1 - b2^t) / (1 - b1^t)

in float64 (the reference) or float32 (one sample of float32 rounding: the unit of the tests' allowances).  The forward is the one of
tests/acf_ref.py (ACFRef.profile, which tests/test_acf_fold_in_cpu.py holds it against) with two switches: fixed="alpha_beta" makes
both attention levels constants of the tape at the step's values (the trajectory a backward without any attention term gives),
fixed="beta" the component level alone (a backward that stops at the item level).  Per user the smallest |relu input| over both
levels and all steps is recorded: a relu input that float32 and float64 put on different sides of zero is nobody's bug, so users
below RELU_DELTA (tests/acf_full_ref.py) are "exposed" and compared for finiteness only.  A user without pairs keeps its row and has
loss 0.  Feed bf16 features as their exactly dequantised fp32 values.

Also here: the inputs of tests/test_gpu_acf_fold_in.py, so that tests/test_acf_fold_in_cpu.py can check them without a GPU."""
import functools

import numpy as np
import torch
import torch.nn.functional as Fn

from acf_full_ref import RELU_DELTA, TOL_MULT, features            # noqa: F401  (the tests read the two constants from here)
from acf_ref import random_tables
from fashionvisualexpl_recommend_amd._ffi import ACF_WEIGHTS

FROZEN = ("Gi", "Pi") + tuple(ACF_WEIGHTS)


def profile(g, hist, p, F, fixed=None, seen=None):
    """g' of the row g with the history `hist` (item ids).  p: the frozen tables, F [I, M, C]; seen: a list that collects the two
    levels' relu inputs."""
    if len(hist) == 0:
        return g
    h = torch.as_tensor(list(hist), dtype=torch.long)
    f = F[h]                                                                              # [L, M, C]
    a_c = p["component.W_0_u"].T @ g + f @ p["component.W_0_i"] + p["component.b_0"]      # [L, M, h]
    s = torch.relu(a_c) @ p["component.W_1"].reshape(-1) + p["component.b_1"].reshape(())
    beta = torch.softmax(s, dim=1)                                                        # [L, M]
    if fixed in ("beta", "alpha_beta"):
        beta = beta.detach()
    x = (beta.unsqueeze(2) * f).sum(1)                                                    # [L, C]
    pi = p["Pi"][h]
    pre = p["item.W_0_u"].T @ g + p["Gi"][h] @ p["item.W_0_iv"] + pi @ p["item.W_0_ip"] + x @ p["item.W_0_ix"] + p["item.b_0"]
    t = torch.relu(pre) @ p["item.W_1"].reshape(-1) + p["item.b_1"].reshape(())
    alpha = torch.softmax(t, dim=0)
    if fixed == "alpha_beta":
        alpha = alpha.detach()
    if seen is not None:
        seen += [a_c.detach(), pre.detach()]
    return g + (alpha.unsqueeze(1) * pi).sum(0)


def user_loss(g, hist, D, p, F, reg, fixed=None, seen=None):
    """loss_t of one user; D [n_r, k] = Gi_i - Gi_j of the user's pairs."""
    x = D @ profile(g, hist, p, F, fixed, seen)
    return Fn.softplus(-torch.clamp(x, -80.0, 1e8)).sum() + reg * D.shape[0] * (g * g).sum()


def hand_grad(g, hist, D, p, F, reg):
    """The closed form of include/bprx.h (no autograd): d loss_t / d g."""
    gp = profile(g, hist, p, F)
    x = D @ gp
    s_p = torch.where((x >= -80.0) & (x <= 1e8), torch.sigmoid(-x), torch.zeros_like(x))
    q = -(s_p.unsqueeze(1) * D).sum(0)
    grad = q + 2.0 * reg * D.shape[0] * g
    if len(hist) == 0:
        return grad
    h = torch.as_tensor(list(hist), dtype=torch.long)
    f, pi = F[h], p["Pi"][h]
    hc = p["component.W_0_u"].shape[1]
    Z = f @ torch.cat([p["component.W_0_i"], p["item.W_0_ix"]], dim=1)                     # [L, M, h + a]
    a_c = p["component.W_0_u"].T @ g + Z[:, :, :hc] + p["component.b_0"]
    w1c, w1i = p["component.W_1"].reshape(-1), p["item.W_1"].reshape(-1)
    beta = torch.softmax(torch.relu(a_c) @ w1c + p["component.b_1"].reshape(()), dim=1)
    pre = p["item.W_0_u"].T @ g + p["Gi"][h] @ p["item.W_0_iv"] + pi @ p["item.W_0_ip"] + (beta.unsqueeze(2) * Z[:, :, hc:]).sum(1) \
        + p["item.b_0"]
    alpha = torch.softmax(torch.relu(pre) @ w1i + p["item.b_1"].reshape(()), dim=0)
    dt = alpha * (pi @ q - (alpha.unsqueeze(1) * pi).sum(0) @ q)
    dpre = dt.unsqueeze(1) * w1i * (pre > 0).to(g.dtype)                                   # [L, a]
    dbeta = (Z[:, :, hc:] * dpre.unsqueeze(1)).sum(2)                                      # [L, M]
    ds = beta * (dbeta - (beta * dbeta).sum(1, keepdim=True))
    da = ds.unsqueeze(2) * w1c * (a_c > 0).to(g.dtype)                                     # [L, M, h]
    return grad + p["item.W_0_u"] @ dpre.sum(0) + p["component.W_0_u"] @ da.sum((0, 1))


def fold_in(tables, F, hists, pair_ptr, pos, neg, G0, steps, lr, reg, optimizer="sgd", dtype=torch.float64, fixed=None,
            beta1=0.9, beta2=0.999, eps=1e-7):
    """{'Gu' [n, k], 'loss' [n] (loss_T, before the last update), 'loss_first' [n], 'min_relu' [n] (inf without relu inputs)} as
    float64 numpy arrays."""
    cv = lambda a: torch.as_tensor(np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a)).to(dtype)
    p = {n: cv(tables[n]) for n in FROZEN}
    F = cv(F)
    G = cv(G0).clone()
    ptr = np.asarray(pair_ptr, np.int64)
    pos, neg = np.asarray(pos, np.int64), np.asarray(neg, np.int64)
    n = len(ptr) - 1
    loss, first, min_relu = np.zeros(n), np.zeros(n), np.full(n, np.inf)
    for r in range(n):
        if ptr[r + 1] == ptr[r]:
            continue
        D = p["Gi"][torch.as_tensor(pos[ptr[r]:ptr[r + 1]])] - p["Gi"][torch.as_tensor(neg[ptr[r]:ptr[r + 1]])]
        g = G[r].clone()
        m, v = torch.zeros_like(g), torch.zeros_like(g)
        for t in range(1, steps + 1):
            g = g.detach().requires_grad_(True)
            seen = []
            lt = user_loss(g, hists[r], D, p, F, reg, fixed, seen)
            (gr,) = torch.autograd.grad(lt, g)
            for s in seen:
                min_relu[r] = min(min_relu[r], s.abs().min().item())
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
            g = g.to(dtype)
        G[r] = g
    return {"Gu": G.double().numpy(), "loss": loss, "loss_first": first, "min_relu": min_relu}


def allowance(r64, r32, has):
    """The project's rule: 32 x the median over the users with pairs of the float32 restatement's max-abs deviation from float64,
    never below one fp32 ulp of the largest row magnitude.  Returns (allow, the per-user float32 deviation)."""
    dev = np.abs(r32["Gu"] - r64["Gu"]).max(1)
    ulp = float(np.spacing(np.float32(np.abs(r64["Gu"]).max())))
    return max(TOL_MULT * float(np.median(dev[has])), ulp), dev


# ---- the inputs of tests/test_gpu_acf_fold_in.py ------------------------------------------------------------------------------
I_ITEMS, C_FEAT, U_TRAINED = 60, 8, 6
NONLINEAR = [(5, 3, 2, 1), (16, 8, 4, 3), (16, 8, 4, 6)]            # (k, h, a, M): few relu inputs per user
INDEXING = [(64, 64, 64, 70), (20, 96, 32, 130), (130, 32, 64, 49)]  # M past one and two 64-lane passes, h + a % 32, k > 128
RUNS = {"sgd": dict(optimizer="sgd", steps=20), "adam": dict(optimizer="adam_tf23", steps=3), "sgd2": dict(optimizer="sgd", steps=2)}
# (history length, pairs) of the ordinary users: every listed length and count; lengths 0 and 1 (a constant attention: the three
# trajectories coincide) and the 40-entry histories (most relu inputs) are kept few
USERS = [(0, 0), (0, 17), (0, 4), (1, 1), (1, 5), (1, 64), (2, 1), (2, 3), (2, 4), (2, 17), (2, 65), (2, 200), (3, 3), (3, 5),
         (3, 17), (3, 64), (3, 65), (3, 0), (4, 1), (4, 4), (4, 5), (4, 64), (4, 200), (4, 17), (5, 3), (5, 4), (5, 5), (5, 17),
         (5, 65), (5, 200), (5, 1), (9, 3), (9, 17), (9, 64), (40, 5), (40, 65)]
# Per shape: the scale of Pi (random_tables: N(0, 0.01) x pi); wu on W_0_u of both levels (how strongly both attentions look at g);
# wx on every other W_0 tensor and b_0 (with wu the width of the relu inputs: wide inputs seldom lie within RELU_DELTA of zero); w1
# on both W_1 (relu is positively homogeneous: the attention logits scale with w0 * w1 and must stay O(1) for either softmax to have a
# derivative worth testing); the runs' learning rate and reg (reg n_r bounds the row of the 3 000-pair user: a row of magnitude 10
# would be compared at ulps of 1e-6).
_KNOB = lambda **kw: dict(dict(pi=30.0, wu=4.0, wx=1.0, w1=4.0, lr=0.01, lr_adam=0.05, reg=0.005), **kw)
KNOBS = {(5, 3, 2, 1): _KNOB(wu=4.0, wx=3.0, w1=0.5), (16, 8, 4, 3): _KNOB(), (16, 8, 4, 6): _KNOB(),
         (64, 64, 64, 70): _KNOB(wu=20.0, wx=20.0, w1=0.8, lr=0.02), (20, 96, 32, 130): _KNOB(wu=40.0, wx=40.0, w1=0.4, lr=0.02),
         (130, 32, 64, 49): _KNOB(wu=20.0, wx=20.0, w1=0.8)}
# (shape, dtype) -> seed, picked on the CPU so that at most 10 % of the users with pairs are exposed and at least half the users
# separate when an attention level is held fixed (tests/test_acf_fold_in_cpu.py); every other case: 11
SEEDS = {((5, 3, 2, 1), "fp32"): 13, ((5, 3, 2, 1), "bf16"): 13, ((16, 8, 4, 3), "bf16raw"): 13, ((16, 8, 4, 3), "fp32"): 13, ((16, 8, 4, 3), "bf16"): 13, ((16, 8, 4, 6), "fp32"): 13, ((16, 8, 4, 6), "bf16"): 13, ((20, 96, 32, 130), "fp32"): 16}


def as_held(t):
    """The tables with [Wci | Wix] as a bf16-feature handle holds them for Z: the sum of two bf16 halves (k_acf_wcat)."""
    t = dict(t)
    for n in ("component.W_0_i", "item.W_0_ix"):
        w = torch.as_tensor(np.asarray(t[n], np.float32))
        hi = w.bfloat16().float()
        t[n] = (hi + (w - hi).bfloat16().float()).numpy()
    return t


@functools.lru_cache(maxsize=None)
def case(shape, dtype="fp32", seed=None):
    """The inputs of one GPU case: tables (U_TRAINED trained users), F as exactly dequantised fp32, the new users' histories, pairs
    and start rows.  After the ordinary USERS: a repeated history item, 3 000 consistent pairs (more than any LDS cache holds), a
    duplicated pair and an i == j pair, and a history without pairs."""
    k, h, a, M = shape
    rs = np.random.RandomState(SEEDS.get((shape, dtype), 11) if seed is None else seed)
    I, C = I_ITEMS, C_FEAT
    kn = KNOBS[shape]
    t = random_tables(rs, U_TRAINED, I, k, C, h, a, scale=kn["pi"])
    for n in ACF_WEIGHTS:
        if n.endswith(".W_0_u"):
            t[n] = (t[n] * kn["wu"]).astype(np.float32)
        elif ".W_0" in n or n.endswith(".b_0"):
            t[n] = (t[n] * kn["wx"]).astype(np.float32)
        elif n.endswith(".W_1"):
            t[n] = (t[n] * kn["w1"]).astype(np.float32)
    if dtype == "bf16":
        # The library's bf16-feature projection holds [Wci | Wix] as two bf16 halves (k_acf_wcat: 16 mantissa bits, 6e-6 relative):
        # Z of every ACF call on such a handle is exact for weights of that form only.  These inputs carry such weights, as they
        # carry features that are exact in bf16: the comparison is about the fold-in, not about the rounding of Z.  dtype "bf16raw"
        # keeps arbitrary fp32 weights (RAW_CASES): there the rows of a 3-step Adam run at lr = 0.05 leave float64 by up to 2.6e-6,
        # 1.3 x the allowance, and float64 fed the two-half weights reproduces that figure.
        t = as_held(t)
    # items 50 .. 56 lie a short step along one direction from items 0 .. 6: the 3 000 pairs (q, 50 + q) all push that way.  The step
    # is short because everything that is wrong with the forward of such a user is multiplied by |q| = |sum_p s_p D_p| in the attention
    # terms of its gradient: with a step of 0.01 (|q| = 15) the float32 restatement itself left float64 by up to 1.8e-5 for this user
    # (8 x the allowance), and the library's bf16-feature Z, which carries [Wci | Wix] as two bf16 halves (16 mantissa bits), by
    # 2.4e-6; float64 with those weights gives the same 2.5e-6.
    v = rs.standard_normal(k)
    t["Gi"][50:57] = t["Gi"][0:7] - (0.001 * v / np.linalg.norm(v)).astype(np.float32)
    F = features(rs, I, M, C, "bf16" if dtype == "bf16raw" else dtype)
    hists, ptr, pos, neg = [], [0], [], []
    def add(hist, p, n):
        hists.append([int(x) for x in hist]); pos.extend(int(x) for x in p); neg.extend(int(x) for x in n); ptr.append(len(pos))
    for L, npairs in USERS:
        add(rs.choice(I, L, replace=False), rs.randint(0, I, npairs), rs.randint(0, I, npairs))
    add([7, 7, 21, 33, 7], rs.randint(0, I, 17), rs.randint(0, I, 17))                    # a repeated item: several entries
    add(rs.choice(I, 3, replace=False), np.arange(3000) % 7, 50 + np.arange(3000) % 7)   # 3 000 pairs pushing one way
    p5, n5 = rs.randint(0, I, 5), rs.randint(0, I, 5)
    p5[3], n5[3] = p5[2], n5[2]                                                           # a duplicated pair
    n5[4] = p5[4]                                                                         # i == j
    add(rs.choice(I, 4, replace=False), p5, n5)
    add(rs.choice(I, 9, replace=False), [], [])                                           # history, no pairs
    n = len(hists)
    G0 = (rs.standard_normal((n, k)) * 0.3).astype(np.float32)
    G0[6] = 0                                                                             # a zero start is live
    return dict(shape=shape, dtype=dtype, t=t, F=F, hists=hists, ptr=np.asarray(ptr, np.int64), pos=np.asarray(pos, np.int32),
                neg=np.asarray(neg, np.int32), G0=G0, I=I, C=C)


@functools.lru_cache(maxsize=None)
def run(shape, dtype, which, torch_dtype=torch.float64, fixed=None, held=False):
    """fold_in of case(shape, dtype) with RUNS[which]; computed once per process and shared: do not write into the result.
    held: with [Wci | Wix] as a bf16-feature handle holds them (as_held)."""
    c, r = case(shape, dtype), RUNS[which]
    return fold_in(as_held(c["t"]) if held else c["t"], c["F"], c["hists"], c["ptr"], c["pos"], c["neg"], c["G0"], r["steps"], KNOBS[shape]["lr_adam" if which == "adam" else "lr"], KNOBS[shape]["reg"], r["optimizer"],
                   torch_dtype, fixed)


def gpu_cases():
    """(shape, feature dtype, run) of every input set the GPU tests use."""
    out = [(s, d, w) for s in NONLINEAR for d in ("fp32", "bf16") for w in ("sgd", "adam")]
    return out + [(s, "fp32", "sgd2") for s in INDEXING]


# bf16 features with ARBITRARY fp32 projection weights, what a user binds: compared with float64 fed the weights as the handle holds
# them under the plain allowance, and with float64 on the exact weights under the allowance plus what those 16 mantissa bits move
# the float64 rows by
RAW_CASES = [((16, 8, 4, 3), "bf16raw", "sgd"), ((16, 8, 4, 3), "bf16raw", "adam")]
