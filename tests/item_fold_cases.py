"""The inputs of tests/test_gpu_item_fold.py, built on the host so that tests/test_item_fold_cpu.py can check what the GPU test
relies on (a helper module, not a test module).

U = I = 300, tables ~ N(0, 0.3) (E and Bp scaled so that P = F.[E|Bp] is), 130 new items with start rows ~ N(0, 0.3) and 0, 1, 3, 4,
5, 17, 64, 65, 200 and 121 random counts in 1..40 pairs, roles mixed; item 7 has one pair twice, item 6 one (u, o) in both roles.
Item BIG has 3 000 pairs, past any LDS share: the 3 000 largest x_p under its start row out of 30 000 random candidates (3 000
RANDOM pairs have a summed curvature of 0.25 x 3 000 along the bias alone: plain sgd oscillates on them in exact arithmetic)."""
import numpy as np

import item_fold_ref as R

U = I = 300
N_NEW = 130
BIG = 9
D_FEAT = 32
WIDTHS = [(5, 0), (16, 12), (63, 20), (64, 64), (128, 20), (200, 271)]
# The seed of each width's case: k, unless a kept Adam entry then sits at the left-out threshold (its float32 row is a +-lr move
# away: deviations of 6.7e-6 at (128, 20) seed 128 and 4.7e-5 at (200, 271) seed 2200 against 2e-7 .. 1.3e-6 elsewhere);
# test_item_fold_cpu.py holds every case to 5e-6.
SEEDS = {(5, 0): 5, (16, 12): 16, (63, 20): 63, (64, 64): 64, (128, 20): 1128, (200, 271): 1200}
SGD = dict(steps=20, lr=0.002, reg=1e-3, optimizer="sgd")
ADAM = dict(steps=3, lr=0.05, reg=1e-3, optimizer="adam_tf23")


def tables(k, d, seed, users=U):
    """The bound tables (fold_in's recipe, tests/test_gpu_fold_in.py) and, with a visual part, 'Fn': the new items' feature rows."""
    rs = np.random.RandomState(seed)
    n = lambda *s: (rs.standard_normal(s) * 0.3).astype(np.float32)
    t = dict(Gu=n(users, k), Gi=n(I, k), Bi=n(I))
    if d:
        F = np.abs(rs.standard_normal((I, D_FEAT))).astype(np.float32)
        F /= F.max()
        scale = 1.0 / np.sqrt((F.astype(np.float64) ** 2).sum(1).mean())
        t.update(Tu=n(users, d), F=F, E=(n(D_FEAT, d) * scale).astype(np.float32), Bp=(n(D_FEAT) * scale).astype(np.float32))
        Fn = np.abs(rs.standard_normal((N_NEW, D_FEAT))).astype(np.float32)
        t["Fn"] = Fn / Fn.max()
    return t


def bound(t):
    """The tables Engine.bind takes."""
    return {n: v for n, v in t.items() if n != "Fn"}


def host_projections(t):
    """(P [I, d + 1], Pn [N_NEW, d + 1]) as float32 of the float64 products: what the fp32-feature projection kernels return up to
    their last bit; (None, None) without a visual part."""
    if "F" not in t:
        return None, None
    EB = np.concatenate([t["E"], t["Bp"][:, None]], 1).astype(np.float64)
    return (t["F"].astype(np.float64) @ EB).astype(np.float32), (t["Fn"].astype(np.float64) @ EB).astype(np.float32)


def items(t, P, Pn, k, d, seed):
    """(ptr, user, other, role, W0 [N_NEW, k + 1]) of the 130 new items of the module docstring."""
    rs = np.random.RandomState(seed + 100)
    counts = [0, 1, 3, 4, 5, 17, 64, 65, 200] + list(rs.randint(1, 41, size=N_NEW - 9))
    W0 = (rs.standard_normal((N_NEW, k + 1)) * 0.3).astype(np.float32)
    user = [rs.randint(U, size=c) for c in counts]
    other = [rs.randint(I, size=c) for c in counts]
    role = [rs.randint(2, size=c) for c in counts]
    cu, co, cr = rs.randint(U, size=30000), rs.randint(I, size=30000), rs.randint(2, size=30000)
    c64 = lambda x: None if x is None else np.asarray(x, np.float64)
    Dm, dc = R.pair_terms(c64(t["Gu"]), c64(t.get("Tu")), c64(t["Gi"]), c64(t["Bi"]), c64(P), None if Pn is None else c64(Pn[BIG]),
                          cu, co, cr)
    best = np.sort(np.argsort(Dm @ W0[BIG].astype(np.float64) + dc)[-3000:])
    counts[BIG] = 3000
    user[BIG], other[BIG], role[BIG] = cu[best], co[best], cr[best]
    user[7][3], other[7][3], role[7][3] = user[7][2], other[7][2], role[7][2]            # a pair twice
    user[6][5], other[6][5], role[6][5] = user[6][4], other[6][4], 1 - role[6][4]        # one (u, o) in both roles
    ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    cat = lambda x: np.concatenate(x).astype(np.int32)
    return ptr, cat(user), cat(other), cat(role), W0


def restate(t, P, Pn, ptr, user, other, role, W0, hp, dtype):
    k = t["Gi"].shape[1]
    return R.fold_in_items(t["Gu"], t.get("Tu"), t["Gi"], t["Bi"], P, Pn, ptr, user, other, role, W0[:, :k], W0[:, k], hp["steps"],
                           hp["lr"], hp["reg"], hp["optimizer"], dtype)


def rows(res):
    """[n, k + 1] from a restatement dict or a (Gi, Bi, ...) tuple."""
    Gi, Bi = (res["Gi"], res["Bi"]) if isinstance(res, dict) else res[:2]
    return np.concatenate([Gi, np.asarray(Bi).reshape(-1, 1)], 1)


def adam_keep(r64, ptr):
    """The (item, element) entries Adam's rows are compared on: Adam's first steps turn the sign of a near-zero gradient into a
    +-lr move, so entries whose float64 |g| at any step is below 1e-3 of that item's largest |g| at that step are left out.
    Returns (keep [n, k + 1] bool, left-out share over the items with pairs)."""
    has = np.diff(ptr) > 0
    keep = np.ones((len(has), r64["Gi"].shape[1] + 1), bool)
    for r in np.nonzero(has)[0]:
        g = np.abs(r64["grads"][r])
        keep[r] = ~(g < 1e-3 * g.max(1, keepdims=True)).any(0)
    return keep, 1.0 - keep[has].mean()
