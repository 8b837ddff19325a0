"""The inputs of tests/test_gpu_af_item_fold.py, built on the host so that tests/test_af_item_fold_cpu.py can check what the GPU
test relies on (a helper module, not a test module).

U = I = 300 catalogue users and items and 130 new items over 12 distinct images, colour histograms and class vectors
(attentive_ref.random_inputs); Gu, Gi and the start rows ~ N(0, 0.3), edges.W2 and attention.W_1 scaled x 4 so that the attention
moves with g_u and with the item.  Pair counts 0, 1, 3, 4, 5, 17, 64, 65, 200 and 121 random counts in 1..40, roles mixed; item 7
has one pair twice, item 6 one (u, o) in both roles.  Item BIG has 3 000 pairs, past any LDS share: the 3 000 largest x_p under its
start row out of 30 000 random candidates (random pairs that many make plain sgd oscillate, see tests/item_fold_cases.py).  The
shapes of WIDE run sgd on twelve items."""
import numpy as np
import torch

import af_item_fold_ref as R
from attentive_ref import AttentiveRef, random_inputs, random_tables

U = I = 300
N_NEW = 130
BIG = 9
DC, DK = 20, 6
WIDTHS = [(5, 7), (16, 32), (64, 64), (20, 96), (120, 128)]
WIDE = [(448, 32), (480, 32)]
WIDE_COUNTS = [0, 1, 5, 17, 40, 7, 3, 64, 2, 9, 11, 30]
# The seed of each width's case: k, unless a kept Adam entry then sits at the left-out threshold or more than 5 % are left out
# (tests/test_af_item_fold_cpu.py holds every case to its bounds).
SEEDS = {(5, 7): 5, (16, 32): 16, (64, 64): 64, (20, 96): 20, (120, 128): 120, (448, 32): 448, (480, 32): 480}
SGD = dict(steps=20, lr=0.002, reg=1e-3, optimizer="sgd")
ADAM = dict(steps=3, lr=0.05, reg=1e-3, optimizer="adam_tf23")


def att(t):
    return tuple(np.asarray(t[n]) for n in R.ATT)


def tables(k, h, seed, n_new=N_NEW):
    """(t, inputs, new, src): the bound tables, the catalogue's (edges, colour, classes), the new items', and src = (the 12 distinct
    inputs, the catalogue's three index vectors into them, the new items')."""
    rs = np.random.RandomState(seed)
    t = random_tables(rs, U, I, k, DC, DK, h)
    t["Gi"] = (rs.standard_normal((I, k)) * 0.3).astype(np.float32)
    t["Gu"] = (rs.standard_normal((U, k)) * 0.3).astype(np.float32)
    t["edges.W2"] = t["edges.W2"] * 4.0                      # (the pooled conv output is small)
    t["attention.W_1"] = t["attention.W_1"] * 4.0
    base = random_inputs(rs, 12, DC, DK)
    pick = lambda n: tuple(rs.randint(0, 12, n) for _ in range(3))
    ci, ni = pick(I), pick(n_new)
    take = lambda ix: tuple(np.ascontiguousarray(b[j]) for b, j in zip(base, ix))
    return t, take(ci), take(ni), (base, ci, ni)


def host_encodings(t, src):
    """(C [3, I, k], Cn [3, n, k]) fp32 of the CPU encoder restatement attentive_ref.AttentiveRef.encode (float64, one image at a
    time): what bprx_af_encode / bprx_af_encode_new return up to float32 rounding."""
    base, ci, ni = src
    ref = AttentiveRef(t, *base, rate=0.0)
    with torch.no_grad():
        enc = [torch.cat(x) for x in zip(*(ref.encode(ref.p, [i]) for i in range(len(base[0]))))]      # colour, edges, class [12, k]
    enc = [e.numpy() for e in enc]
    rows = lambda ix: np.stack([enc[l][ix[l]] for l in range(3)]).astype(np.float32)
    return rows(ci), rows(ni)


def items(t, C, Cn, k, seed, counts=None):
    """(ptr, user, other, role, W0 [n, k]) of the new items of the module docstring (counts: the twelve items of a WIDE shape)."""
    rs = np.random.RandomState(seed + 100)
    wide = counts is not None
    n = len(counts) if wide else N_NEW
    counts = list(counts) if wide else [0, 1, 3, 4, 5, 17, 64, 65, 200] + list(rs.randint(1, 41, size=N_NEW - 9))
    W0 = (rs.standard_normal((n, k)) * 0.3).astype(np.float32)
    user = [rs.randint(U, size=c) for c in counts]
    other = [rs.randint(I, size=c) for c in counts]
    role = [rs.randint(2, size=c) for c in counts]
    if not wide:
        cu, co, cr = rs.randint(U, size=30000), rs.randint(I, size=30000), rs.randint(2, size=30000)
        c64 = lambda x: np.asarray(x, np.float64)
        Dm, dc = R.pair_terms(c64(t["Gu"]), c64(t["Gi"]), c64(C), tuple(c64(a) for a in att(t)), c64(Cn[:, BIG, :]), cu, co, cr)
        best = np.sort(np.argsort(Dm @ W0[BIG].astype(np.float64) + dc)[-3000:])
        counts[BIG] = 3000
        user[BIG], other[BIG], role[BIG] = cu[best], co[best], cr[best]
        user[7][3], other[7][3], role[7][3] = user[7][2], other[7][2], role[7][2]            # a pair twice
        user[6][5], other[6][5], role[6][5] = user[6][4], other[6][4], 1 - role[6][4]        # one (u, o) in both roles
    ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    cat = lambda x: np.concatenate(x).astype(np.int32)
    return ptr, cat(user), cat(other), cat(role), W0


def restate(t, C, Cn, ptr, user, other, role, W0, hp, dtype=np.float64, uniform_alpha=False):
    return R.fold_in_items(t["Gu"], t["Gi"], C, att(t), Cn, ptr, user, other, role, W0, hp["steps"], hp["lr"], hp["reg"],
                           hp["optimizer"], dtype, uniform_alpha)


def adam_keep(r64, ptr):
    """The (item, element) entries Adam's rows are compared on, the rule of item_fold_cases.adam_keep on k columns: entries whose
    float64 |g| at any step is below 1e-3 of that item's largest |g| at that step are left out.  Returns (keep [n, k] bool,
    left-out share over the items with pairs)."""
    has = np.diff(ptr) > 0
    keep = np.ones((len(has), r64["Gi"].shape[1]), bool)
    for r in np.nonzero(has)[0]:
        g = np.abs(r64["grads"][r])
        keep[r] = ~(g < 1e-3 * g.max(1, keepdims=True)).any(0)
    return keep, 1.0 - keep[has].mean()


_cache = {}


def case(k, h):
    """Everything of one width that needs no GPU, made once and never changed: tables, inputs, host encodings, the items."""
    if (k, h) not in _cache:
        wide = (k, h) in WIDE
        seed = SEEDS[(k, h)]
        t, inputs, new, src = tables(k, h, seed, len(WIDE_COUNTS) if wide else N_NEW)
        C, Cn = host_encodings(t, src)
        ptr, user, other, role, W0 = items(t, C, Cn, k, seed, WIDE_COUNTS if wide else None)
        _cache[(k, h)] = dict(t=t, inputs=inputs, new=new, src=src, C=C, Cn=Cn, ptr=ptr, user=user, other=other, role=role, W0=W0)
    return _cache[(k, h)]
