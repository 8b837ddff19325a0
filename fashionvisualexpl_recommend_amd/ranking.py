"""The one place where score rows become top-K lists and lists become rows of text: every recs-* / new-recs-* /
new-user-recs-* / div-* / because-* file, single GPU or sharded, catalogue items or new ones, is ranked and written here, block
by block (blocks, wanted_blocks), and gets its name here (RUN_FILES, run_file).  So are the item-side lists, audience-* /
new-audience-* (owners_of: the transposed mask; ITEM_FILES, item_file: their names).

The contract is the reference's (Evaluator.py:225-239): mask the row, then take numpy_topk of it; numpy's unstable argsort
decides the order of EQUAL scores.  The top-K kernel returns the list wherever it does not depend on that order and flags
every other row (include/bprx.h, bprx_topk); a flagged row is redone by numpy_topk on the row the kernel has masked.
The category lists (shelf-* / cap-*: class_csr, rank_class_rows, shelf_order, cap_rows; SHELF_FILES, shelf_file) have a total
order of their own (score descending, item ascending: include/bprx.h, bprx_topk_classes), so nothing is flagged or redone there.
Plain numpy + torch: no library call is made here, the caller brings the top-K entry (and the MMR entry of diversify_rows) as a
callable.
"""
import numpy as np
import torch


def numpy_topk(row, k):
    """The reference's list of one masked score row, best first (Evaluator.py:234)."""
    return row.argsort()[-k:][::-1]


def rows_per_block(user_block, width):
    """Rows of `width` scores per block: user_block, cut so that one block's scores stay below 2^27 elements."""
    return max(1, min(user_block, (1 << 27) // max(1, width)))


def blocks(n, block, width=None):
    """(b0, b1) of the rows [0, n), `block` rows at a time, the last block the shorter one; with `width` (scores per row) the block
    is cut by rows_per_block."""
    step = block if width is None else rows_per_block(block, width)
    for b0 in range(0, n, step):
        yield b0, min(n, b0 + step)


def wanted_blocks(want, n, block, width=None):
    """The blocks of blocks(n, block, width) that hold an id of `want` (int64 array, any order, repeats allowed), ascending, each
    as (b0, b1, rows, local): want[rows] are the ids in [b0, b1), rows ascending (the caller's order), local = want[rows] - b0."""
    step = block if width is None else rows_per_block(block, width)
    for b0 in sorted({int(q) // step * step for q in want}):
        b1 = min(n, b0 + step)
        rows = np.nonzero((want >= b0) & (want < b1))[0]
        yield b0, b1, rows, want[rows] - b0


def lists_to_csr(lists, device, dedup=False):
    """Python lists of item ids per row -> (int64 ptr [n + 1], int32 items) tensors on `device`.  dedup: a repeated id counts
    once, the first time (the reference masks with set(training_list[user]), Evaluator.py:41).  `items` is never empty (one
    zero when every list is: a kernel is handed a pointer it does not read); counts come from ptr[-1]."""
    if dedup:
        lists = [list(dict.fromkeys(l)) for l in lists]
    lens = np.fromiter((len(l) for l in lists), dtype=np.int64, count=len(lists))
    ptr = np.zeros(len(lists) + 1, np.int64)
    np.cumsum(lens, out=ptr[1:])
    items = np.fromiter((int(i) for l in lists for i in l), dtype=np.int64, count=int(ptr[-1])).astype(np.int32)
    if items.size == 0:
        items = np.zeros(1, np.int32)
    return torch.as_tensor(ptr, device=device), torch.as_tensor(items, device=device)


def owners_of(training_list, num_items):
    """For each item of [0, num_items) its owners: the users whose training list names it, each once, ascending (int64 arrays, one
    per item).  The transpose of what store_recommendation masks (set(training_list[user])): an id outside the catalogue has no
    row here, as it has no column there."""
    if num_items <= 0:
        return []
    lens = np.fromiter((len(l) for l in training_list), dtype=np.int64, count=len(training_list))
    users = np.repeat(np.arange(len(training_list), dtype=np.int64), lens)
    items = np.fromiter((int(i) for l in training_list for i in l), dtype=np.int64, count=int(lens.sum()))
    keep = (items >= 0) & (items < num_items)
    pairs = np.unique(items[keep] * max(1, len(training_list)) + users[keep])     # by item, then by user, each pair once
    it, us = pairs // max(1, len(training_list)), pairs % max(1, len(training_list))
    return np.split(us, np.searchsorted(it, np.arange(1, num_items)))


def rank_rows(topk, scores, k, side=None):
    """The lists of a block of device score rows [n, width]: numpy ids int64 [n, kk], vals fp32 [n, kk], kk = min(k, width),
    best first, and side_rows [n, kk, c] (None without `side`).  topk(scores, k) is the top-K entry: it masks IN `scores` and
    returns the device (idx, val, flag).  Unflagged rows are the kernel's; a flagged row is downloaded (masked) and redone by
    numpy_topk, its kernel output is not read.  side: a device tensor [n, width, c] gathered at the final ids (the
    AttentiveFashion attentions).  One download of idx / val / flag (and of the gathered side) per call, one row per flagged row."""
    width = int(scores.shape[1])
    kk = min(k, width)
    idx, val, flag = topk(scores, k)
    side_rows = None
    if side is not None:
        pick = idx[:, :kk].long().clamp_(0, width - 1).unsqueeze(-1).expand(-1, -1, side.shape[2])
        side_rows = torch.gather(side, 1, pick).cpu().numpy()
    idx, val, flag = idx.cpu().numpy(), val.cpu().numpy(), flag.cpu().numpy()
    ids, vals = idx[:, :kk].astype(np.int64), val[:, :kk].copy()
    for r in np.nonzero(flag)[0]:                             # few: ties are rare in real-valued scores
        row = scores[int(r)].cpu().numpy()
        ids[r] = numpy_topk(row, k)
        vals[r] = row[ids[r]]
        if side is not None:
            side_rows[r] = side[int(r)].cpu().numpy()[ids[r]]
    return ids, vals, side_rows


def ranked_zeros(n, kk, c=0):
    """(ids int64 [n, kk], vals fp32 [n, kk]) and, with c > 0 side columns, side fp32 [n, kk, c] of zeros: what rank_rows' blocks are
    put into."""
    return (np.zeros((n, kk), np.int64), np.zeros((n, kk), np.float32)) + ((np.zeros((n, kk, c), np.float32),) if c else ())


def diverse_zeros(n, kk):
    """(ids int64 [n, kk], vals fp32 [n, kk], pen fp32 [n, kk], ild fp32 [n]) of zeros: what diversify_rows' blocks are put into."""
    return np.zeros((n, kk), np.int64), np.zeros((n, kk), np.float32), np.zeros((n, kk), np.float32), np.zeros(n, np.float32)


def diversify_rows(diversify, ids, vals, k, device):
    """The diversified lists of a block of pools: `ids` int64 [n, N] / `vals` fp32 [n, N] are what rank_rows returned for a pool
    of N (flagged rows already redone by numpy there; a masked entry keeps its -inf and is no candidate).  They are uploaded
    once, diversify(pool_idx int32, pool_val, kk) is the MMR entry (Engine.diversify with its space, norms and theta bound) and
    returns the device (idx, val, pen, ild).  Returns numpy ids int64 [n, kk], vals fp32 [n, kk], pen fp32 [n, kk] and ild fp32
    [n], kk = min(k, N); slots past a pool's candidates hold -1 / 0 / 0."""
    n, N = ids.shape
    kk = min(int(k), N)
    if n == 0 or kk == 0:
        return diverse_zeros(n, kk)
    pool_idx = torch.as_tensor(np.ascontiguousarray(ids, dtype=np.int32), device=device)
    pool_val = torch.as_tensor(np.ascontiguousarray(vals, dtype=np.float32), device=device)
    idx, val, pen, ild = diversify(pool_idx, pool_val, kk)
    return idx.cpu().numpy().astype(np.int64), val.cpu().numpy(), pen.cpu().numpy(), ild.cpu().numpy()


# ---- category shelves and quota lists: the per-class lists of bprx_topk_classes ------------------------------------------------
def class_csr(item_class, num_items, device, classes=None):
    """The class table of a catalogue as bprx_topk_classes takes it: item_class is an int array [num_items], the class of every
    item, -1 = no class (the item is on no list) -> (int64 ptr [C + 1], int32 items, C) with ptr / items tensors on `device`, C =
    the largest class id + 1 (at least 1; a class id nobody has is an empty class), the items of a class ascending.  `items` is
    never empty (one zero when every item is classless: a kernel is handed a pointer it does not read).  classes = S: exactly S
    classes (the clusters of bprx_style_update, whose last ones may be empty); a class id >= S is a ValueError."""
    cls = np.asarray(item_class).reshape(-1)
    if cls.size != num_items or cls.dtype.kind not in "iu":
        raise ValueError("class_csr: one integer class per item, [%d] (got %s %s)" % (num_items, cls.dtype, cls.shape))
    cls = cls.astype(np.int64)
    if cls.size and cls.min() < -1:
        raise ValueError("class_csr: a class id is >= 0, or -1 for no class (got %d)" % cls.min())
    C = max(1, int(cls.max()) + 1 if cls.size else 1)
    if classes is not None:
        if C > int(classes):
            raise ValueError("class_csr: class id %d with %d classes" % (C - 1, int(classes)))
        C = int(classes)
    have = np.flatnonzero(cls >= 0)
    items = have[np.argsort(cls[have], kind="stable")].astype(np.int32)            # by class, ascending item inside a class
    ptr = np.zeros(C + 1, np.int64)
    np.cumsum(np.bincount(cls[have], minlength=C), out=ptr[1:])
    if items.size == 0:
        items = np.zeros(1, np.int32)
    return torch.as_tensor(ptr, device=device), torch.as_tensor(items, device=device), C


def class_rows_per_block(user_block, width, C, K):
    """rows_per_block, cut further so that one call's outputs (rows x C x K elements) stay below 2^27 as well; never below one row."""
    return max(1, min(rows_per_block(user_block, width), ((1 << 27) - 1) // max(1, int(C) * int(K))))


def rank_class_rows(topk_classes, scores, k):
    """The per-class lists of a block of device score rows [n, width]: numpy ids int64 [n, C, kk], vals fp32 [n, C, kk] and cnt
    int64 [n, C], kk = min(k, width); list (r, c) holds cnt[r, c] entries, best first, equal scores by ascending item, then -1 /
    0.0.  topk_classes(scores, kk) is the entry (Engine.topk_classes with its mask lists and class table): it masks IN `scores`
    and returns the device (idx, val, cnt).  One download per call; no row is redone (the order is total)."""
    kk = min(int(k), int(scores.shape[1]))
    idx, val, cnt = topk_classes(scores, kk)
    return idx.cpu().numpy().astype(np.int64), val.cpu().numpy(), cnt.cpu().numpy().astype(np.int64)


def shelf_order(vals, cnt):
    """Per row the classes with a non-empty list, the row's shelves in the row's order: by the score of the list's first entry,
    descending (compared as floats: +0.0 == -0.0), equal scores by ascending class id.  vals [n, C, kk] / cnt [n, C] as
    rank_class_rows returns them -> a list of n int64 arrays."""
    out = []
    for r in range(cnt.shape[0]):
        cls = np.flatnonzero(cnt[r] > 0)
        out.append(cls[np.lexsort((cls, -(vals[r, cls, 0] + np.float32(0.0))))].astype(np.int64))
    return out


def cap_rows(ids, vals, cnt, k, cap):
    """The quota lists of rank_class_rows' lists (ranked with K >= min(cap, k)): per row the first k of the union of every class's
    first min(cap, k) entries by (score descending as floats, item ascending) -- the top-k with at most `cap` items of any class,
    exactly.  Returns numpy ids int64 [n, k], vals fp32 [n, k] and cls int64 [n, k] (the class of each entry); -1 / 0.0 / -1 past
    a row's entries."""
    n, C, kk = ids.shape
    k, m = int(k), min(int(cap), int(k), kk)
    on = np.arange(m)[None, None, :] < np.minimum(cnt, m)[:, :, None]
    it = np.where(on, ids[:, :, :m], np.iinfo(np.int64).max).reshape(n, C * m)
    sc = np.where(on, vals[:, :, :m], np.float32(-np.inf)).reshape(n, C * m)
    cl = np.broadcast_to(np.arange(C, dtype=np.int64)[None, :, None], (n, C, m)).reshape(n, C * m)
    o = np.argsort(it, axis=1, kind="stable")                 # by item, then (stable) by score: equal scores stay item-ascending
    it, sc, cl = (np.take_along_axis(a, o, axis=1) for a in (it, sc, cl))
    o = np.argsort(-(sc + np.float32(0.0)), axis=1, kind="stable")[:, :k]
    it, sc, cl = (np.take_along_axis(a, o, axis=1) for a in (it, sc, cl))
    out_i, out_v, out_c = np.full((n, k), -1, np.int64), np.zeros((n, k), np.float32), np.full((n, k), -1, np.int64)
    have = np.minimum(k, on.reshape(n, -1).sum(axis=1))
    keep = np.arange(it.shape[1])[None, :] < have[:, None]
    out_i[:, :it.shape[1]][keep], out_v[:, :it.shape[1]][keep], out_c[:, :it.shape[1]][keep] = it[keep], sc[keep], cl[keep]
    return out_i, out_v, out_c


def write_shelves(out, labels, ids, vals, cnt, count=0):
    """One row 'label\tclass\titem\tscore' per shelf entry: label by label, the label's shelves in shelf_order (count > 0: only the
    first `count` of them), each shelf best first.  Fields are formatted as write_ranked formats them."""
    order = shelf_order(vals, cnt)
    for r, label in enumerate(labels):
        head = str(label) + '\t'
        for c in (order[r][:count] if count > 0 else order[r]):
            for q in range(int(cnt[r, c])):
                out.write(head + str(c) + '\t' + str(ids[r, c, q]) + '\t' + str(vals[r, c, q]) + '\n')


def write_capped(out, labels, ids, vals, cls):
    """One row 'label\titem\tscore\tclass' per entry of cap_rows' lists, list by list up to its first empty slot, formatted as
    write_ranked formats them."""
    for r, label in enumerate(labels):
        head = str(label) + '\t'
        for q, item in enumerate(ids[r]):
            if item < 0:
                break
            out.write(head + str(item) + '\t' + str(vals[r, q]) + '\t' + str(cls[r, q]) + '\n')


BECAUSE_MAX_LIST = 1024                                       # slots of one list in bprx_because


def because_rows(because, users, items, lists, top, device, dedup=False):
    """The nearest owned items of arbitrary (user, item) pairs: runs of equal users become the lists of one call, padded with -1
    and split at BECAUSE_MAX_LIST entries, the history of a list is lists[user] (dedup: a repeated id counts once, the first time).
    because(list_idx int32 [n, K], (ptr, items)) is the entry (Engine.because with its space, norms and top bound) and returns
    the device (item [n, K, L], cos [n, K, L], cnt [n, K]), L = top.  Returns numpy hist int64 [pairs, L], cos fp32 [pairs, L]
    and count int64 [pairs], pair by pair; without pairs the entry is not called."""
    users, items = np.asarray(users, dtype=np.int64).reshape(-1), np.asarray(items, dtype=np.int64).reshape(-1)
    if users.size != items.size:
        raise ValueError("because: %d users for %d items" % (users.size, items.size))
    if users.size == 0:
        return np.zeros((0, int(top)), np.int64), np.zeros((0, int(top)), np.float32), np.zeros(0, np.int64)
    run = np.cumsum(np.r_[True, users[1:] != users[:-1]]) - 1              # the run of every pair
    first = np.flatnonzero(np.r_[True, run[1:] != run[:-1]])               # where each run starts
    within = np.arange(users.size) - first[run]
    chunk = within // BECAUSE_MAX_LIST
    new = np.r_[True, (run[1:] != run[:-1]) | (chunk[1:] != chunk[:-1])]
    li, off = np.cumsum(new) - 1, within % BECAUSE_MAX_LIST                # list and slot of every pair
    heads = np.flatnonzero(new)
    list_idx = np.full((heads.size, int(off.max()) + 1), -1, np.int32)
    list_idx[li, off] = items
    csr = lists_to_csr([lists[int(u)] for u in users[heads]], device, dedup)
    item, cos, cnt = because(torch.as_tensor(list_idx, device=device), csr)
    item, cos, cnt = item.cpu().numpy(), cos.cpu().numpy(), cnt.cpu().numpy()
    return item[li, off].astype(np.int64), cos[li, off], cnt[li, off].astype(np.int64)


def influence_rows(influence, users, items, lists, top, device, draw, rows, maps=False):
    """The influence of the history entries of arbitrary (user, item) pairs: runs of equal users become the lists of one call,
    padded with -1 and split at BECAUSE_MAX_LIST entries, as because_rows forms them.  The pairs of the call are draw(the
    histories lists[user] of the runs, in order) = (pair_ptr, pos, neg) (models.draw_fold_pairs: one draw per run; the lists a
    long run is split into share the run's pairs), rows(user ids int64) the device (Gu rows, Tu rows or None) of those users.
    influence(Gu, Tu, ptr, pos, neg, list_idx int32 [n, K]) is the entry (Engine.influence with its per_entry, top, reg, damp and
    maps) and returns the device dict.  Returns numpy hist int64 [pairs, L], infl fp32 [pairs, L], total fp32 [pairs] and count
    int64 [pairs], pair by pair, and with maps the per-entry influences fp32 [pairs, M] (M: the longest history of the call in
    entries, 0 past a pair's own); without pairs the entry is not called."""
    users, items = np.asarray(users, dtype=np.int64).reshape(-1), np.asarray(items, dtype=np.int64).reshape(-1)
    if users.size != items.size:
        raise ValueError("influence: %d users for %d items" % (users.size, items.size))
    top = int(top)
    if users.size == 0:
        out = (np.zeros((0, top), np.int64), np.zeros((0, top), np.float32), np.zeros(0, np.float32), np.zeros(0, np.int64))
        return out + (np.zeros((0, 0), np.float32),) if maps else out
    run = np.cumsum(np.r_[True, users[1:] != users[:-1]]) - 1              # the run of every pair
    first = np.flatnonzero(np.r_[True, run[1:] != run[:-1]])               # where each run starts
    within = np.arange(users.size) - first[run]
    chunk = within // BECAUSE_MAX_LIST
    new = np.r_[True, (run[1:] != run[:-1]) | (chunk[1:] != chunk[:-1])]
    li, off = np.cumsum(new) - 1, within % BECAUSE_MAX_LIST                # list and slot of every pair
    heads = np.flatnonzero(new)
    list_idx = np.full((heads.size, int(off.max()) + 1), -1, np.int32)
    list_idx[li, off] = items
    ptr, pos, neg = draw([lists[int(u)] for u in users[first]])
    of = run[heads]                                                         # the run of every list
    if heads.size != first.size:                                            # a run split into lists: each gets the run's pairs
        take = np.concatenate([np.arange(ptr[r], ptr[r + 1]) for r in of] + [np.zeros(0, np.int64)]).astype(np.int64)
        ptr, pos, neg = np.concatenate([[0], np.cumsum(ptr[of + 1] - ptr[of])]).astype(np.int64), pos[take], neg[take]
    Gu, Tu = rows(users[heads])
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=device)
    res = influence(Gu, Tu, dev(ptr), dev(pos), dev(neg), dev(list_idx))
    host = {n: v.cpu().numpy() for n, v in res.items()}
    out = (host["item"][li, off].astype(np.int64), host["infl"][li, off], host["total"][li, off], host["cnt"][li, off].astype(np.int64))
    return out + (host["full"][li, off],) if maps else out


def rank_rows_host(scores, mask_lists, k):
    """rank_rows on the host: row r of the numpy block `scores` gets -inf (IN `scores`) at mask_lists[r] (None: nothing is
    masked) and is listed by numpy_topk.  Returns (ids int64 [n, kk], vals [n, kk])."""
    n, width = scores.shape
    ids = np.empty((n, len(range(width)[-k:])), np.int64)     # (the length of numpy_topk's slice)
    for r in range(n):
        row = scores[r]
        if mask_lists is not None:
            row[mask_lists[r]] = -np.inf
        ids[r] = numpy_topk(row, k)
    return ids, np.take_along_axis(scores, ids, axis=1)


def write_ranked(out, labels, ids, vals, side=None):
    """One row 'label\\tid\\tval[\\tside_0 ...]' per list entry, list by list, each field the str() of its numpy scalar (vals
    and side stay float32: the text of a float depends on its type).  Returns (labels, items) of the rows written, one entry
    per row, as a block_hook takes them."""
    users, items = [], []
    for r, label in enumerate(labels):
        head = str(label) + '\t'
        for q, item in enumerate(ids[r]):
            tail = '' if side is None else ''.join('\t' + str(a) for a in side[r, q])
            out.write(head + str(item) + '\t' + str(vals[r, q]) + tail + '\n')
        users.extend([label] * len(ids[r]))
        items.extend(int(v) for v in ids[r])
    return users, items


def write_item_lists(out, labels, ids, vals, side=None):
    """write_ranked for lists that may end in empty slots (id < 0: an item with fewer non-owners than the list is long): the
    rows 'label\\tid\\tval[\\tside_0 ...]' of every list up to its first empty slot, formatted as write_ranked formats them."""
    for r, label in enumerate(labels):
        n = int((ids[r] >= 0).sum())
        write_ranked(out, [label], ids[r:r + 1, :n], vals[r:r + 1, :n], None if side is None else side[r:r + 1, :n])


def write_feature_rows(out, users, items, e):
    """The expl-* rows of VBPR and GradFashion for the pairs (users, items): 'u\\ti\\tscore\\tbase\\trank\\tcolumn\\tcontribution',
    rank 0 (the largest F_ic w_uc) first, one row per rank the pair has.  e: the numpy dict of Engine.feat_explain, or of
    feat_explain_new, which has no base: new items get no base column.  Fields are formatted as write_ranked formats them."""
    for r, (u, i) in enumerate(zip(users, items)):
        head = str(u) + '\t' + str(i) + '\t' + str(e["score"][r]) + '\t' + (str(e["base"][r]) + '\t' if "base" in e else '')
        for s in range(e["col"].shape[1]):
            if e["col"][r, s] < 0:
                break
            out.write(head + str(s) + '\t' + str(e["col"][r, s]) + '\t' + str(e["contrib"][r, s]) + '\n')


# Every file a run can write next to its recs-<epoch>-<params>.tsv: the file is named [best-]<kind>-<epoch>-<params>.tsv.  The value
# is the list file whose pairs (or users) the file is about; None: the file stands for itself.
RUN_FILES = {"recs": None, "expl": "recs",
             "new-recs": None, "new-expl": "new-recs",
             "new-user-recs": None,
             "sim": None, "new-sim": None,
             "div-recs": "recs", "div-ild": "recs", "div-new-user-recs": "new-user-recs", "div-new-user-ild": "new-user-recs",
             "because": "recs", "because-new-recs": "new-recs", "because-new-user-recs": "new-user-recs"}


def _split_run_file(path):
    """(directory and 'best-' if any, kind, '-<epoch>-<params>.tsv') of a run file's path; the kind is None for any other name."""
    d, sep, f = path.rpartition('/')
    best = "best-" if f.startswith("best-") else ""
    for kind in sorted(RUN_FILES, key=len, reverse=True):     # ('because-new-recs' before 'because')
        if f.startswith(best + kind + "-"):
            return d + sep + best, kind, f[len(best) + len(kind):]
    return d + sep + best, None, f


def run_file(path, kind):
    """The file of `kind` (a key of RUN_FILES) next to the recs-* / best-recs-* file at `path`; 'best-' stays in front.  ValueError
    for a path whose file name starts with neither."""
    head, base, tail = _split_run_file(path)
    if base != "recs":
        raise ValueError("%r is neither a recs-* nor a best-recs-* path" % path)
    if kind not in RUN_FILES:
        raise ValueError("run_file: %r is none of %s" % (kind, ", ".join(RUN_FILES)))
    return head + kind + tail


# The files of a run whose lists have one block per ITEM (rows 'item user score'), named like the files of RUN_FILES:
# [best-]<kind>-<epoch>-<params>.tsv next to the recs-* / best-recs-* file.  A table of its own: RUN_FILES holds the user-side files.
ITEM_FILES = {"audience": None, "new-audience": None}


def item_file(path, kind):
    """run_file for the kinds of ITEM_FILES: the file of `kind` next to the recs-* / best-recs-* file at `path`, 'best-' stays in
    front; ValueError for a path whose file name starts with neither, and for a kind that is none of ITEM_FILES."""
    head, base, tail = _split_run_file(path)
    if base != "recs":
        raise ValueError("%r is neither a recs-* nor a best-recs-* path" % path)
    if kind not in ITEM_FILES:
        raise ValueError("item_file: %r is none of %s" % (kind, ", ".join(ITEM_FILES)))
    return head + kind + tail


# The files of a run about WARM items (new items whose Gi / Bi rows were fitted from their first buyers): warm-recs-* has one block
# per user (rows 'user row score'), warm-audience-* one per warm item (rows 'row user score'), named like the files above.
WARM_FILES = {"warm-recs": None, "warm-audience": None}


def warm_file(path, kind):
    """run_file for the kinds of WARM_FILES: the file of `kind` next to the recs-* / best-recs-* file at `path`, 'best-' stays in
    front; ValueError for a path whose file name starts with neither, and for a kind that is none of WARM_FILES."""
    head, base, tail = _split_run_file(path)
    if base != "recs":
        raise ValueError("%r is neither a recs-* nor a best-recs-* path" % path)
    if kind not in WARM_FILES:
        raise ValueError("warm_file: %r is none of %s" % (kind, ", ".join(WARM_FILES)))
    return head + kind + tail


# The files of a run whose lists know the items' CLASSES (--item_classes): shelf-* has one block per user and class (rows 'user class
# item score'), cap-* the top-k with a per-class cap (rows 'user item score class'), named like the files above.
SHELF_FILES = {"shelf-recs": None, "cap-recs": None, "shelf-new-user-recs": None, "cap-new-user-recs": None}


def shelf_file(path, kind):
    """run_file for the kinds of SHELF_FILES: the file of `kind` next to the recs-* / best-recs-* file at `path`, 'best-' stays in
    front; ValueError for a path whose file name starts with neither, and for a kind that is none of SHELF_FILES."""
    head, base, tail = _split_run_file(path)
    if base != "recs":
        raise ValueError("%r is neither a recs-* nor a best-recs-* path" % path)
    if kind not in SHELF_FILES:
        raise ValueError("shelf_file: %r is none of %s" % (kind, ", ".join(SHELF_FILES)))
    return head + kind + tail


# The files of a run about the STYLES of the item space (--styles: spherical k-means, models.item_styles): styles-* has one row per
# catalogue item (rows 'item style cosine'), style-items-* every style's members nearest its centroid (rows 'style size rank item
# cosine'), user-styles-* every user's style profile (rows 'user style owned share'), new-styles-* the style of every new item
# (rows 'row style cosine'), named like the files above.
STYLE_FILES = {"styles": None, "style-items": None, "user-styles": None, "new-styles": None}


def style_file(path, kind):
    """run_file for the kinds of STYLE_FILES: the file of `kind` next to the recs-* / best-recs-* file at `path`, 'best-' stays in
    front; ValueError for a path whose file name starts with neither, and for a kind that is none of STYLE_FILES."""
    head, base, tail = _split_run_file(path)
    if base != "recs":
        raise ValueError("%r is neither a recs-* nor a best-recs-* path" % path)
    if kind not in STYLE_FILES:
        raise ValueError("style_file: %r is none of %s" % (kind, ", ".join(STYLE_FILES)))
    return head + kind + tail


# The files of a run about INFLUENCE (--influence L: the history entries a pick's score rests on, on the user's own fold-in
# objective; include/bprx.h, bprx_influence): influence-* is about the pairs of recs-*, influence-new-user-recs-* about those of
# new-user-recs-* (rows 'label item score rank hist_item influence share'), named like the files above.
INFLUENCE_FILES = {"influence": None, "influence-new-user-recs": None}


def influence_file(path, kind):
    """run_file for the kinds of INFLUENCE_FILES: the file of `kind` next to the recs-* / best-recs-* file at `path`, 'best-' stays
    in front; ValueError for a path whose file name starts with neither, and for a kind that is none of INFLUENCE_FILES."""
    head, base, tail = _split_run_file(path)
    if base != "recs":
        raise ValueError("%r is neither a recs-* nor a best-recs-* path" % path)
    if kind not in INFLUENCE_FILES:
        raise ValueError("influence_file: %r is none of %s" % (kind, ", ".join(INFLUENCE_FILES)))
    return head + kind + tail


def write_influence(out, labels, ids, vals, hist, infl, total):
    """One row 'label\tid\tval\trank\thist_item\tinfluence\tshare' per history entry that explains a list entry, rank 0 (the
    largest influence) first, for every entry of every list in write_ranked's order: ids / vals [n, kk] as write_ranked takes
    them, hist int / infl fp32 [n, kk, L] with -1 past an entry's candidates, total fp32 [n, kk] the sum of |influence| over ALL
    of the user's entries; share = influence / total in float32, 0.0 where total is 0.  An entry without a candidate (a user
    without pairs, or a row whose factorisation failed) gets one row with rank -1, hist_item -1, influence 0.0 and share 0.0, so
    that the file names every pair of the list file.  Fields are formatted as write_ranked formats them."""
    for r, label in enumerate(labels):
        head = str(label) + '\t'
        for q, item in enumerate(ids[r]):
            pair = head + str(item) + '\t' + str(vals[r, q]) + '\t'
            if hist.shape[2] == 0 or hist[r, q, 0] < 0:
                out.write(pair + '-1\t-1\t0.0\t0.0\n')
                continue
            tot = np.float32(total[r, q])
            for s in range(hist.shape[2]):
                if hist[r, q, s] < 0:
                    break
                v = np.float32(infl[r, q, s])
                share = v / tot if tot != 0 else np.float32(0.0)
                out.write(pair + str(s) + '\t' + str(hist[r, q, s]) + '\t' + str(v) + '\t' + str(share) + '\n')


def write_styles(out, style, cos):
    """One row 'item\tstyle\tcosine' per row of `style` (int) / `cos` (fp32), in order; a zero row has style -1.  Fields are
    formatted as write_ranked formats them."""
    for i in range(len(style)):
        out.write(str(i) + '\t' + str(style[i]) + '\t' + str(cos[i]) + '\n')


def write_style_items(out, sizes, ids, vals, cnt):
    """One row 'style\tsize\trank\titem\tcosine' per entry of every style's list, style by style, rank 0 first: ids [S, R] /
    vals [S, R] / cnt [S] are the one score row's lists of rank_class_rows (best first, equal cosines by ascending item), sizes
    [S] the styles' member counts.  An empty style has no rows."""
    for s in range(len(sizes)):
        head = str(s) + '\t' + str(sizes[s]) + '\t'
        for q in range(int(cnt[s])):
            out.write(head + str(q) + '\t' + str(ids[s, q]) + '\t' + str(vals[s, q]) + '\n')


def user_style_rows(lists, style):
    """The style profile of every list of item ids: per list the (style, owned) pairs of the styles its items have, by descending
    count, equal counts by ascending style, and the list's length (repeats and items without a style count towards the length;
    items without a style are in no pair).  style: int array [num_items], -1 = none."""
    style = np.asarray(style, dtype=np.int64)
    out = []
    for l in lists:
        own = style[np.asarray(l, dtype=np.int64)] if len(l) else np.zeros(0, np.int64)
        st, n = np.unique(own[own >= 0], return_counts=True)
        o = np.lexsort((st, -n))
        out.append((st[o], n[o], len(l)))
    return out


def write_user_styles(out, labels, rows):
    """One row 'label\tstyle\towned\tshare' per pair of user_style_rows, label by label; share = owned / list length as float32."""
    for label, (st, n, total) in zip(labels, rows):
        head = str(label) + '\t'
        for s, c in zip(st, n):
            out.write(head + str(s) + '\t' + str(c) + '\t' + str(np.float32(c) / np.float32(total)) + '\n')


def _about(path, family, what, table=None):
    """The files of `table` (None: RUN_FILES) that are about the list file at `path` and whose kind starts with `family`, in the
    table's order."""
    head, base, tail = _split_run_file(path)
    table = RUN_FILES if table is None else table
    out = tuple(head + kind + tail for kind, of in table.items() if base is not None and of == base and kind.startswith(family))
    if not out:
        raise ValueError("%s: %r is no recs-* path" % (what, path))
    return out


def div_paths(path):
    """(div-recs-*, div-ild-*) next to the recs-* / best-recs-* / new-user-recs-* / best-new-user-recs-* file at `path`: 'div-'
    goes in front of the file's own 'recs-' / 'new-user-recs-' part, the ild file has 'ild-' where that part is."""
    return _about(path, "div-", "div_paths")


def write_diverse(out, out_ild, labels, ids, vals, pen, ild):
    """One row 'label\tid\tval\tredundancy' per pick, list by list in selection order (empty slots, id < 0, are left out), into
    `out`; one row 'label\tild' per list into `out_ild`.  Fields are formatted as write_ranked formats them."""
    for r, label in enumerate(labels):
        head = str(label) + '\t'
        for q, item in enumerate(ids[r]):
            if item < 0:
                break
            out.write(head + str(item) + '\t' + str(vals[r, q]) + '\t' + str(pen[r, q]) + '\n')
        out_ild.write(head + str(ild[r]) + '\n')


# The files of a run whose lists are CALIBRATED (--calibrate: greedy KL re-rank toward the class mix of the user's history;
# include/bprx.h, bprx_calibrate): cal-recs-* has the lists (rows 'label item score class gain'), cal-kl-* one row per list (rows
# 'label kl_plain kl_calibrated hist_classed'); the value is the list file the file is about, as in RUN_FILES.
CAL_FILES = {"cal-recs": "recs", "cal-kl": "recs", "cal-new-user-recs": "new-user-recs", "cal-new-user-kl": "new-user-recs"}


def cal_paths(path):
    """(cal-recs-*, cal-kl-*) next to the recs-* / best-recs-* / new-user-recs-* / best-new-user-recs-* file at `path`: 'cal-'
    goes in front of the file's own 'recs-' / 'new-user-recs-' part, the kl file has 'kl-' where that part's 'recs-' is."""
    return _about(path, "cal-", "cal_paths", CAL_FILES)


def calibrated_zeros(n, kk):
    """(ids int64 [n, kk], vals fp32 [n, kk], cls int64 [n, kk], gain fp32 [n, kk], kl fp32 [n, 2]) of zeros: what calibrate_rows'
    blocks are put into."""
    return (np.zeros((n, kk), np.int64), np.zeros((n, kk), np.float32), np.zeros((n, kk), np.int64), np.zeros((n, kk), np.float32),
            np.zeros((n, 2), np.float32))


def calibrate_rows(calibrate, ids, vals, k, device):
    """The calibrated lists of a block of pools, the twin of diversify_rows: `ids` int64 [n, N] / `vals` fp32 [n, N] are what
    rank_rows returned for a pool of N (a masked entry keeps its -inf and is no candidate).  They are uploaded once,
    calibrate(pool_idx int32, pool_val, kk) is the entry (Engine.calibrate with its histories, class table, lambda and alpha bound)
    and returns the device (idx, val, cls, gain, kl).  Returns numpy ids int64 [n, kk], vals fp32 [n, kk], cls int64 [n, kk], gain
    fp32 [n, kk] and kl fp32 [n, 2], kk = min(k, N); slots past a pool's candidates hold -1 / 0 / -1 / 0."""
    n, N = ids.shape
    kk = min(int(k), N)
    if n == 0 or kk == 0:
        return calibrated_zeros(n, kk)
    pool_idx = torch.as_tensor(np.ascontiguousarray(ids, dtype=np.int32), device=device)
    pool_val = torch.as_tensor(np.ascontiguousarray(vals, dtype=np.float32), device=device)
    idx, val, cls, gain, kl = calibrate(pool_idx, pool_val, kk)
    return (idx.cpu().numpy().astype(np.int64), val.cpu().numpy(), cls.cpu().numpy().astype(np.int64), gain.cpu().numpy(),
            kl.cpu().numpy())


def hist_classed(lists, item_class):
    """H of bprx_calibrate for every list of item ids as a run hands it over, every id once (the training CSR and the new users'
    histories are deduplicated): the number of its distinct ids that lie in the class table and have a class, int64 [len(lists)]."""
    item_class = np.asarray(item_class, dtype=np.int64)
    out = np.zeros(len(lists), np.int64)
    for r, l in enumerate(lists):
        it = np.unique(np.asarray(l, dtype=np.int64).reshape(-1))
        it = it[(it >= 0) & (it < item_class.size)]
        out[r] = int((item_class[it] >= 0).sum())
    return out


def write_calibrated(out, out_kl, labels, ids, vals, cls, gain, kl, hist_classed):
    """One row 'label\tid\tval\tclass\tgain' per pick, list by list in selection order (empty slots, id < 0, are left out), into
    `out`; one row 'label\tkl_plain\tkl_calibrated\thist_classed' per list into `out_kl`.  Fields are formatted as write_ranked
    formats them."""
    for r, label in enumerate(labels):
        head = str(label) + '\t'
        for q, item in enumerate(ids[r]):
            if item < 0:
                break
            out.write(head + str(item) + '\t' + str(vals[r, q]) + '\t' + str(cls[r, q]) + '\t' + str(gain[r, q]) + '\n')
        out_kl.write(head + str(kl[r, 0]) + '\t' + str(kl[r, 1]) + '\t' + str(hist_classed[r]) + '\n')


def because_paths(path):
    """The because-* file next to the list file at `path`: 'because-' takes the place of the 'recs-' of recs-* / best-recs-* and
    goes in front of the 'new-user-recs-' / 'new-recs-' of the other list files (best-new-recs-2-x -> best-because-new-recs-2-x)."""
    return _about(path, "because", "because_paths")[0]


def write_because(out, labels, ids, vals, hist, cos):
    """One row 'label\tid\tval\trank\thist_item\tcosine' per owned item that explains a list entry, rank 0 (the nearest) first,
    for every entry of every list in write_ranked's order: ids / vals [n, kk] as write_ranked takes them, hist int / cos fp32
    [n, kk, L] with -1 past an entry's candidates.  An entry without a candidate gets one row with rank -1, hist_item -1 and
    cosine 0.0, so that the file names every pair of the list file.  Fields are formatted as write_ranked formats them."""
    for r, label in enumerate(labels):
        head = str(label) + '\t'
        for q, item in enumerate(ids[r]):
            pair = head + str(item) + '\t' + str(vals[r, q]) + '\t'
            if hist.shape[2] == 0 or hist[r, q, 0] < 0:
                out.write(pair + '-1\t-1\t0.0\n')
                continue
            for s in range(hist.shape[2]):
                if hist[r, q, s] < 0:
                    break
                out.write(pair + str(s) + '\t' + str(hist[r, q, s]) + '\t' + str(cos[r, q, s]) + '\n')
