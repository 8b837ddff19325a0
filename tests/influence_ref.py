"""Influence of a user's history entries on the scores of a list, restated in numpy on the CPU (a helper module, not a test
module).

For row r: w = [Gu_r | Tu_r] (n = k + d numbers), its m pairs (i_p, j_p) in pair_ptr order, `per_entry` consecutive pairs one
history entry (a short last group is an entry of its own: M = ceil(m / per_entry)), every item-side parameter frozen:

    z_i = [Gi_i | P_i[0:d]]     c_i = Bi_i + P_i[d]     D_p = z_i - z_j     x_p = w.D_p + (c_i - c_j)
    s_p = sigmoid(-x_p)         c_p = s_p (1 - s_p)     (x_p outside [-80, 1e8]: both 0)
    A = sum_p c_p D_p D_p^T     lambda = 2 reg m + damp trace(A) / n
    g_e = sum_{p in entry e} s_p D_p
    infl(q, e) = z_q^T (A + lambda I)^-1 g_e            total(q) = sum_e |infl(q, e)|

by a Cholesky factorisation and two triangular solves per list slot, in float64 (the reference) or, the same algorithm, in
float32 (one sample of float32 rounding: the scale of the tests' allowances).  A factorisation that meets a pivot that is not
positive and finite flags the row: its slots are empty."""
import numpy as np


def item_side(Gi, Bi, P, d, dtype=np.float64):
    """(Z [I, k + d], c [I]) of the catalogue."""
    f = dtype
    Gi, Bi = np.asarray(Gi, np.float32).astype(f), np.asarray(Bi, np.float32).reshape(-1).astype(f)
    if not d:
        return Gi, Bi
    P = np.asarray(P, np.float32).astype(f)
    return np.concatenate([Gi, P[:, :d]], 1), Bi + P[:, d]


def cholesky(A):
    """Lower Cholesky factor of A in A's dtype, by columns (right-looking); None for a pivot that is not positive and finite."""
    f = A.dtype.type
    L = np.tril(A).astype(f)
    n = L.shape[0]
    for j in range(n):
        piv = L[j, j]
        if not (piv > 0 and np.isfinite(piv)):
            return None
        l = np.sqrt(piv)
        L[j, j] = l
        L[j + 1:, j] = L[j + 1:, j] / l
        c = L[j + 1:, j]
        L[j + 1:, j + 1:] -= np.tril(np.outer(c, c)).astype(f)
    return L


def solve(L, B):
    """(L L^T)^-1 B for B [n, K], in L's dtype: forward, then back substitution."""
    f = L.dtype.type
    B = B.astype(f).copy()
    n = L.shape[0]
    for j in range(n):
        B[j] = B[j] / L[j, j]
        B[j + 1:] -= np.outer(L[j + 1:, j], B[j]).astype(f)
    for j in range(n - 1, -1, -1):
        B[j] = B[j] / L[j, j]
        B[:j] -= np.outer(L[j, :j], B[j]).astype(f)
    return B


def row_terms(Z, c, w, i, j, dtype=np.float64):
    """(D [m, n], s [m], cp [m]) of one row's pairs."""
    f = dtype
    D, dc = Z[i] - Z[j], c[i] - c[j]
    x = (D @ w + dc).astype(f)
    inr = (x >= f(-80)) & (x <= f(1e8))
    with np.errstate(over="ignore"):
        s = np.where(inr, f(1) / (f(1) + np.exp(x)), f(0)).astype(f)
    return D, s, (s * (f(1) - s)).astype(f)


def entry_sums(t, per_entry):
    """Sums of consecutive groups of per_entry of t [.., m] along the last axis, a short last group included: [.., M]."""
    m = t.shape[-1]
    starts = np.arange(0, m, per_entry)
    return np.add.reduceat(t, starts, axis=-1) if m else t[..., :0]


def influence(Gi, Bi, P, Gu, Tu, pair_ptr, pos, neg, per_entry, reg, damp, lists, dtype=np.float64):
    """{'full': list of [K, M_r] arrays (nan in an empty slot's row; [K, 0] for a flagged row or one without pairs),
    'total' [n, K], 'cnt' int [n, K], 'flag' int [n], 'ids': list of [M_r] entry ids} in `dtype`."""
    f = dtype
    d = 0 if Tu is None else np.asarray(Tu).shape[1]
    Z, c = item_side(Gi, Bi, P, d, f)
    W = np.asarray(Gu, np.float32).astype(f)
    if d:
        W = np.concatenate([W, np.asarray(Tu, np.float32).astype(f)], 1)
    nw = W.shape[1]
    ptr = np.asarray(pair_ptr, np.int64)
    pos, neg = np.asarray(pos, np.int64), np.asarray(neg, np.int64)
    lists = np.asarray(lists, np.int64)
    n, K = lists.shape
    out = {"full": [], "ids": [], "total": np.zeros((n, K), f), "cnt": np.zeros((n, K), np.int64), "flag": np.zeros(n, np.int64)}
    for r in range(n):
        i, j = pos[ptr[r]:ptr[r + 1]], neg[ptr[r]:ptr[r + 1]]
        m = len(i)
        empty = np.zeros((K, 0), f)
        if m == 0:
            out["full"].append(empty); out["ids"].append(np.zeros(0, np.int64))
            continue
        D, s, cp = row_terms(Z, c, W[r], i, j, f)
        A = ((D * cp[:, None]).T @ D).astype(f)
        lam = f(2) * f(reg) * f(m) + f(damp) * np.trace(A).astype(f) / f(nw)
        with np.errstate(invalid="ignore", over="ignore"):
            L = cholesky((A + lam * np.eye(nw, dtype=f)).astype(f))
        if L is None:
            out["flag"][r] = 1
            out["full"].append(empty); out["ids"].append(np.zeros(0, np.int64))
            continue
        on = lists[r] >= 0
        V = solve(L, Z[np.maximum(lists[r], 0)].T)                          # [nw, K]
        t = ((D @ V).astype(f) * s[:, None]).T                               # [K, m]
        full = entry_sums(t, per_entry).astype(f)
        full[~on] = np.nan
        out["full"].append(full)
        out["ids"].append(i[::per_entry].copy())
        out["total"][r] = np.where(on, np.abs(np.nan_to_num(full)).sum(1, dtype=f), f(0))
        out["cnt"][r] = np.where(on, full.shape[1], 0)
    return out


def top_entries(row, L):
    """Positions of the min(L, M) largest values of row [M], descending; values compare as floats, equal values by position."""
    return np.argsort(-np.asarray(row), kind="stable")[:L]


def newton_fit(Z, c, i, j, reg_m, w0, keep=None, iters=60):
    """The minimiser (float64, Newton) of sum_{p in keep} softplus(-x_p) + reg_m |w|^2 over w, started at w0.  reg_m: the ridge
    weight reg m of the FULL row (the same ridge with and without an entry)."""
    D, dc = Z[i] - Z[j], c[i] - c[j]
    if keep is not None:
        D, dc = D[keep], dc[keep]
    w = np.asarray(w0, np.float64).copy()
    for _ in range(iters):
        x = D @ w + dc
        s = 1.0 / (1.0 + np.exp(x))
        g = -(s[:, None] * D).sum(0) + 2.0 * reg_m * w
        H = (D * (s * (1 - s))[:, None]).T @ D + 2.0 * reg_m * np.eye(len(w))
        step = np.linalg.solve(H, g)
        w = w - step
        if np.abs(step).max() < 1e-14:
            break
    return w
