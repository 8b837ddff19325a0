"""Float64 restatement of the style clusters (include/bprx.h: bprx_style_assign / bprx_style_update, models.item_styles), computed
from the same float32 inputs: the item vectors z [I, w] (float32 values), the norms rn [I] and the centroids (float32 values).

    rnorm(z)                      1 / |z_i| in float64, 0 for a zero row
    unit(z, rn)                   fl32(z_ix rn_i): the member rows the update sums (one float32 rounding, as the kernel makes it)
    assign(z, rn, cent)           style, best, second, gap = best - second per row; ties to the smallest index, a row with
                                  rn == 0 gets (-1, 0, 0) and gap +inf
    update(z, rn, members, prev)  cent [S, w] float64 and mass [S]; an empty cluster or a zero sum keeps prev's row, mass 0
    seeds(z, rn, S)               farthest-first seeds, ties to the smallest id
    loop(z, rn, S, iters, seeds)  Lloyd's loop as models.item_styles runs it: style, cos, cent, objective

tol(w) = (w + 4) 2^-23 is the bound of a float32 cosine of two vectors of norm <= 1 over w products: the fma chain errs by at most
about w 2^-24, the norm factor adds about (w / 2 + 3) 2^-24, and the bound doubles their sum."""
import numpy as np


def tol(w):
    return (w + 4) * 2.0 ** -23


def rnorm(z):
    n2 = (np.asarray(z, np.float64) ** 2).sum(axis=1)
    return np.where(n2 > 0, 1.0 / np.sqrt(np.where(n2 > 0, n2, 1.0)), 0.0)


def unit(z, rn):
    return (np.asarray(z, np.float32) * np.asarray(rn, np.float32)[:, None]).astype(np.float32)


def cosines(z, rn, cent):
    """c(q, s) = <z_q, cent_s> rn_q in float64, [I, S]."""
    return (np.asarray(z, np.float64) @ np.asarray(cent, np.float64).T) * np.asarray(rn, np.float64)[:, None]


def assign(z, rn, cent):
    c = cosines(z, rn, cent)
    I, S = c.shape
    style = np.argmax(c, axis=1).astype(np.int64)             # (numpy's argmax returns the first maximum: the smallest index)
    best = c[np.arange(I), style]
    if S > 1:
        rest = c.copy()
        rest[np.arange(I), style] = -np.inf
        second = rest.max(axis=1)
    else:
        second = np.full(I, -np.inf)
    zero = np.asarray(rn) == 0
    style[zero], best[zero], second[zero] = -1, 0.0, 0.0
    gap = np.where(zero, np.inf, best - second)
    return style, best, second, gap


def excused(gap, w):
    """The rows whose style a float32 kernel may legitimately choose differently: the reference gap is below 2 tol(w)."""
    return np.asarray(gap) < 2 * tol(w)


def update(z, rn, members, prev):
    """members: one int array per cluster.  Returns (cent float64 [S, w], mass float64 [S])."""
    x = unit(z, rn).astype(np.float64)
    prev = np.asarray(prev, np.float64)
    cent, mass = prev.copy(), np.zeros(len(members))
    for s, m in enumerate(members):
        m = np.asarray(m, np.int64)
        if m.size == 0:
            continue
        tot = x[m].sum(axis=0)
        n2 = float((tot ** 2).sum())
        if n2 > 0:
            cent[s], mass[s] = tot / np.sqrt(n2), np.sqrt(n2)
    return cent, mass


def members_of(style, S):
    return [np.flatnonzero(style == s) for s in range(S)]


def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32)


def seeds(z, rn, S):
    rn = np.asarray(rn)
    live = rn > 0
    if live.sum() < S:
        raise ValueError("fewer than S items with a non-zero norm")
    out = [int(np.flatnonzero(live)[0])]
    far = np.where(live, -np.inf, np.inf)
    zeros = np.zeros((1, np.asarray(z).shape[1]))
    while len(out) < S:
        far[out[-1]] = np.inf
        cent = _f32(update(z, rn, [np.array(out[-1:])], zeros)[0])      # the float32 row the library assigns against
        far = np.maximum(far, cosines(z, rn, cent)[:, 0])
        out.append(int(np.flatnonzero(far == far.min())[0]))
    return np.asarray(out, np.int64)


def loop(z, rn, S, iters=20, seed_ids=None):
    """(style int64 [I], cos [I], cent float32 values [S, w], objective [iterations run]); the centroids are rounded to float32
    after every update, as the library stores them."""
    seed_ids = seeds(z, rn, S) if seed_ids is None else np.asarray(seed_ids, np.int64)
    w = np.asarray(z).shape[1]
    cent = _f32(update(z, rn, [np.array([i]) for i in seed_ids], np.zeros((S, w)))[0])
    style, cos, _, _ = assign(z, rn, cent)
    objective = []
    for _ in range(iters):
        c64, mass = update(z, rn, members_of(style, S), cent)
        cent = _f32(c64)
        objective.append(mass.sum() / max(1, int((style >= 0).sum())))
        new_style, cos, _, _ = assign(z, rn, cent)
        same = np.array_equal(new_style, style)
        style = new_style
        if same:
            break
    return style, cos, cent, np.asarray(objective)


def planted(sizes, w, noise, seed):
    """Clusters of the given sizes around random unit centres in w dimensions, Gaussian noise of the given scale per component,
    shuffled: (z float32 [I, w], label int64 [I])."""
    rs = np.random.RandomState(seed)
    centres = rs.standard_normal((len(sizes), w))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    label = np.repeat(np.arange(len(sizes)), sizes)
    z = centres[label] + noise * rs.standard_normal((label.size, w))
    z *= rs.uniform(0.5, 2.0, size=(label.size, 1))           # (lengths differ: the cosine does not see them)
    perm = rs.permutation(label.size)
    return z[perm].astype(np.float32), label[perm].astype(np.int64)


def same_partition(a, b):
    """Whether two labelings are one partition up to the names of the parts."""
    a, b = np.asarray(a), np.asarray(b)
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len(set(a.tolist())) == len(set(b.tolist()))


# ---- the inputs the GPU tests assign (shared with the excusal check of tests/test_styles_cpu.py) ------------------------------
# A thin cross of I x w x S through (389, 9, 7): the edges of the 128-row query tiles, of the 16-column K chunk and of the
# 128-centroid tiles.  w == 1 has cosines of +-1 only, so more than two centroids tie on every row: it runs with S = 2.
ASSIGN_CASES = [(1, 9, 7), (127, 9, 7), (128, 9, 7), (129, 9, 7), (389, 9, 7), (1300, 9, 7),
                (389, 1, 2), (389, 16, 7), (389, 17, 7),
                (389, 9, 1), (389, 9, 2), (389, 9, 33), (389, 9, 127), (389, 9, 128), (389, 9, 129), (389, 9, 257), (389, 9, 1024),
                (1000, 16, 33), (700, 24, 130)]
BOTH_CASE = (1300, 24, 16, 257)                               # I, k, d, S on a VBPR handle: w = 40
BOTH_FEAT = 128                                               # feature columns of that handle


def unit_rows(rs, S, w):
    c = rs.standard_normal((S, w))
    return (c / np.linalg.norm(c, axis=1, keepdims=True)).astype(np.float32)


def assign_case(I, w, S):
    """(z float32 [I, w], cent float32 [S, w]): Gaussian rows and unit Gaussian centroids, seeded by the shape."""
    rs = np.random.RandomState(1000 * I + 10 * w + S)
    z = rs.standard_normal((I, w)).astype(np.float32)
    cent = unit_rows(rs, S, w)
    if w == 1 and S == 2:
        cent[1] = -cent[0]                                    # (two equal centroids would tie on every row)
    return z, cent


def both_case():
    """The tables of the both-space case: Gi [I, k] Gaussian; every feature row has one non-zero column c_i holding a power of
    two p_i, so that the projection P[i, 0:d] = p_i E[c_i] is exact in float32 and the test knows z = [Gi_i | p_i E[c_i]] bit
    for bit.  Returns (Gi, F, E, z, cent)."""
    I, k, d, S = BOTH_CASE
    rs = np.random.RandomState(77)
    Gi = (0.3 * rs.standard_normal((I, k))).astype(np.float32)
    E = (0.3 * rs.standard_normal((BOTH_FEAT, d))).astype(np.float32)
    col, p = rs.randint(BOTH_FEAT, size=I), (2.0 ** rs.randint(-2, 1, size=I)).astype(np.float32)
    F = np.zeros((I, BOTH_FEAT), np.float32)
    F[np.arange(I), col] = p
    z = np.concatenate([Gi, p[:, None] * E[col]], axis=1).astype(np.float32)
    return Gi, F, E, z, unit_rows(rs, S, k + d)
