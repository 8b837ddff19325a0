"""What bprx_topk owes a masked fp32 score row, in plain numpy, and the rows the top-K tests feed it.

classify(row, K, n_unmasked) names the class of a row that has ALREADY been masked (train items at -inf).  Float `==` applies,
so +0.0 == -0.0.  With Kc = min(K, I):

  DETERMINED   K <= I, at least K entries unmasked, the Kc largest values pairwise unequal, and the Kc-th and (Kc+1)-th
               largest unequal.  The list is unique: unique_topk(row, K) = np.argsort(-row, kind="stable")[:K].  The kernel
               must return exactly that, unflagged.
  EITHER       not determined, K <= I, and the Kc-th largest value is -inf: the kernel flags such a row whether or not that
               -inf is the only one, and either answer is accepted.
  MUST_FLAG    every other row (K > I included): the reference's list depends on numpy's order of equal scores, so the row
               must come back flagged.

gen_rows(I, K, counts, seed) builds the rows: one family per row (FAMILIES), values laid out by rank over the UNMASKED
positions, so the family's structure is a property of the masked row; the train items hold large scores (a kernel that
forgot to mask one would rank it first).  NaN scores and repeated held-out items are outside the contract."""
import numpy as np

DETERMINED, EITHER, MUST_FLAG = "determined", "either", "must_flag"

# rows per family in one (I, K) launch: 104 rows, of which only `k_minus_1` (4) is EITHER by construction
FAMILIES = (("distinct", 8), ("zeros_inside_pm", 8), ("zeros_inside_mp", 8), ("zeros_straddle_pm", 8),
            ("zeros_straddle_mp", 8), ("zeros_below", 8), ("denormal", 8), ("inf_one", 8), ("inf_two", 8), ("neg_inf", 8),
            ("five_levels", 8), ("exact_k", 6), ("k_minus_1", 4), ("dup_train", 6))
# families whose rows may never be EITHER (the signed zeros, the denormals, the infinities)
NEVER_EITHER = ("zeros_inside_pm", "zeros_inside_mp", "zeros_straddle_pm", "zeros_straddle_mp", "zeros_below", "denormal",
                "inf_one", "inf_two", "neg_inf")
SHAPES = [(I, K) for I in (70, 300, 1030) for K in (1, 2, 5, 64, 257, 1024)]     # K > I: (70, 257), (70, 1024), (300, 1024)


def classify(row, K, n_unmasked):
    I = row.shape[0]
    if K > I:
        return MUST_FLAG
    v = np.sort(row)[::-1]
    Kc = min(K, I)
    top_distinct = bool(np.all(v[:Kc - 1] != v[1:Kc]))
    boundary_distinct = Kc == I or bool(v[Kc - 1] != v[Kc])
    if n_unmasked >= K and top_distinct and boundary_distinct:
        return DETERMINED
    if v[Kc - 1] == -np.inf:
        return EITHER
    return MUST_FLAG


def unique_topk(row, K):
    return np.argsort(-row, kind="stable")[:K]


def mask(scores, train):
    out = scores.copy()
    for r, t in enumerate(train):
        out[r, t] = -np.inf
    return out


def _ladder(n, top, scale):
    """n distinct fp32 values, descending from top * scale in steps of `scale` (multiples of scale: exactly ordered)."""
    return ((top - np.arange(n)) * scale).astype(np.float32)


def _rank_values(fam, M, Kc, rs):
    """Values by rank (descending) for the M unmasked positions of a row of `fam`; None where the family does not fit."""
    scale = np.float32(rs.uniform(0.2, 3.0))
    plain = _ladder(M, M // 2 + 0.25 + rs.randint(-M // 4 - 1, M // 4 + 2), scale)      # both signs, no zero
    if fam in ("distinct", "exact_k", "k_minus_1", "dup_train"):
        return plain
    if fam.startswith("zeros_"):
        if fam.startswith("zeros_inside"):
            lo, hi = 0, min(Kc, M) - 2
        elif fam.startswith("zeros_straddle"):
            lo, hi = Kc - 1, min(Kc - 1, M - 2)
        else:
            lo, hi = Kc, M - 2
        if hi < lo:
            return None
        r = rs.randint(lo, hi + 1)                            # the pair sits at ranks r, r + 1
        v = np.empty(M, np.float32)
        v[:r] = _ladder(r, r, scale)                          # r, ..., 1 times scale: positive
        v[r], v[r + 1] = 0.0, -0.0
        v[r + 2:] = _ladder(M - r - 2, -1, scale)             # -1, -2, ... times scale
        return v
    if fam == "denormal":                                     # odd multiples of 2^-149, both signs, no zero
        return ((2.0 * (M // 2 - np.arange(M)) + 1.0) * 2.0 ** -149).astype(np.float32)
    if fam == "inf_one":
        plain[0] = np.inf
        return plain
    if fam == "inf_two":
        if M < 2:
            return None
        plain[:2] = np.inf
        return plain
    if fam == "neg_inf":
        if M < Kc + 1:
            return None
        plain[-1] = -np.inf
        return plain
    if fam == "five_levels":
        levels = np.array([1.5, 0.25, 0.0, -0.75, -2.0], np.float32) * scale
        return np.sort(levels[rs.randint(0, 5, size=M)])[::-1]
    raise ValueError(fam)


def gen_row(fam, I, K, rs):
    """One row of family `fam`: (scores fp32 [I], train list).  Families that cannot be laid out at (I, K) fall back:
    zeros_inside <-> zeros_straddle, zeros_below -> zeros_inside, the others -> distinct."""
    Kc = min(K, I)
    tmax = max(0, min(12, I - Kc - 2))                        # ordinary rows keep at least Kc + 2 items unmasked
    if fam == "exact_k":
        t = I - K if K <= I else 0
    elif fam == "k_minus_1":
        t = I - K + 1 if K <= I else 1
    elif fam == "dup_train":
        t = max(1, rs.randint(0, tmax + 1)) if K <= I else 2
    else:
        t = rs.randint(0, tmax + 1)
    M = I - t
    order = rs.permutation(I)
    train, free = order[:t], order[t:]                        # free[j] holds the value of rank j
    v = None
    for f in (fam, {"zeros_inside_pm": "zeros_straddle_pm", "zeros_inside_mp": "zeros_straddle_mp",
                    "zeros_straddle_pm": "zeros_inside_pm", "zeros_straddle_mp": "zeros_inside_mp",
                    "zeros_below": "zeros_inside_pm"}.get(fam, "distinct"), "distinct"):
        v = _rank_values(f, M, Kc, rs) if M > 0 else np.zeros(0, np.float32)
        if v is not None:
            fam_used = f
            break
    row = np.empty(I, np.float32)
    row[free] = v
    row[train] = (1.0e6 + rs.permutation(t)).astype(np.float32)          # masked away: must never be ranked
    if fam_used.startswith("zeros_"):
        z = np.nonzero(row == 0)[0]
        z = z[np.argsort(np.signbit(row[z]))]                            # z[0] holds +0.0, z[1] holds -0.0
        plus_first = fam_used.endswith("_pm") or (fam_used == "zeros_below" and rs.randint(2) == 0)
        a, b = (min(z), max(z)) if plus_first else (max(z), min(z))
        row[a], row[b] = 0.0, -0.0                                       # index order of the pair
    train = train.tolist()
    if fam == "dup_train":
        train = train + train[:2] + train[:1]
    return row, train


def gen_rows(I, K, families=FAMILIES, seed=0):
    """-> (scores fp32 [n, I], train lists, family name per row) for the (I, K) launch."""
    rs = np.random.RandomState(1000 * I + K + 7919 * seed)
    rows, train, fams = [], [], []
    for fam, n in families:
        for _ in range(n):
            r, t = gen_row(fam, I, K, rs)
            rows.append(r)
            train.append(t)
            fams.append(fam)
    return np.stack(rows), train, fams


def n_unmasked(I, train):
    return I - len(set(train))


def check_launch(scores, train, fams, K, idx, val, flag, masked_after):
    """What one bprx_topk launch over gen_rows' rows must satisfy; `masked_after` is the score buffer after the call.
    Returns the list of failures as (row, family, class, what) so that a caller can report all of them at once."""
    n, I = scores.shape
    m = mask(scores, train)
    bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    bad = []
    if not np.array_equal(bits(masked_after), bits(m)):
        bad.append((-1, "-", "-", "score buffer is not the masked matrix"))
    for r in range(n):
        nu = n_unmasked(I, train[r])
        c = classify(m[r], K, nu)
        what = None
        if c == DETERMINED:
            want = unique_topk(m[r], K)
            if flag[r] != 0:
                what = "determined row flagged"
            elif not np.array_equal(idx[r], want):
                what = "idx %s != %s" % (idx[r][:8].tolist(), want[:8].tolist())
            elif not np.array_equal(bits(val[r]), bits(m[r][want])):
                what = "val is not the row at idx, bit for bit"
        elif c == MUST_FLAG and flag[r] != 1:
            what = "must-flag row came back with flag %d" % flag[r]
        if what is None and nu < K and flag[r] != 1:
            what = "fewer than K unmasked items, flag %d" % flag[r]      # the header's contract, EITHER rows included
        if what is None and K > I:
            live = idx[r, :I]
            if not (np.all(idx[r, I:] == -1) and np.array_equal(bits(val[r, I:]), np.zeros(K - I, np.uint32))):
                what = "entries past I are not -1 / +0.0"
            elif not (np.array_equal(np.sort(live), np.arange(I)) and np.array_equal(bits(val[r, :I]), bits(m[r][live]))
                      and np.all(val[r, :I - 1] >= val[r, 1:I])):
                what = "the first I entries are not the row in descending order"
        if what is not None:
            bad.append((r, fams[r], c, what))
    return bad


def emulate_topk(row, K, float_equality=True):
    """The list and flag a selection by integer keys produces on a masked row: keys ordered like the floats, ties by item
    ascending; flagged on K > I, equal keys inside the list or across its boundary, or a -inf in the list.  With
    float_equality=False the key is the bare bit image, which ranks +0.0 strictly above -0.0: the checker must catch that."""
    I = row.shape[0]
    u = row.view(np.uint32).astype(np.int64)
    if float_equality:
        u = np.where(u == 0x80000000, 0, u)
    key = np.where(u & 0x80000000, 0xFFFFFFFF - u, u | 0x80000000)
    Kc = min(K, I)
    order = np.lexsort((np.arange(I), -key))
    pick = order[:Kc]
    kk = key[pick]
    flag = int(K > I or np.any(kk[:-1] == kk[1:]) or (Kc < I and key[order[Kc]] == kk[-1]) or row[pick[-1]] == -np.inf)
    idx = np.full(K, -1, np.int32)
    val = np.zeros(K, np.float32)
    idx[:Kc], val[:Kc] = pick, row[pick]
    return idx, val, flag
