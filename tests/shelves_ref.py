"""The category lists of bprx_topk_classes restated in numpy (include/bprx.h): what tests/test_shelves_cpu.py pins on the CPU and
tests/test_gpu_shelves.py compares the kernel with, exactly.

  mask         row r gets -inf at the in-range ids of its mask list
  class_lists  per (row, class) the class's items ordered by np.lexsort((items, -(scores + 0.0))): score descending compared as
               floats (the + 0.0 turns -0.0 into +0.0, so the two zeros tie), equal scores by ascending item; entries that are
               -inf in the masked row are dropped; the first K stay
  shelf_order  per row the classes with a non-empty list by (first entry's score descending, class ascending)
  cap_lists    the quota merge: the first k of the union of every class's first min(cap, k) entries by (score descending, item
               ascending)
"""
import numpy as np


def mask(scores, lists, width=None):
    """A copy of `scores` [n, width] with -inf at lists[r] (None: nothing), ids outside [0, width) ignored."""
    out = np.array(scores, dtype=np.float32, copy=True)
    if lists is not None:
        for r, l in enumerate(lists):
            ids = np.asarray(l, dtype=np.int64).reshape(-1)
            out[r, ids[(ids >= 0) & (ids < out.shape[1])]] = -np.inf
    return out


def classes_of(item_class, C=None):
    """Per class the ascending items of an int array [width] (-1: no class) -> a list of C int64 arrays."""
    cls = np.asarray(item_class, dtype=np.int64)
    C = int(cls.max()) + 1 if C is None else C
    return [np.flatnonzero(cls == c).astype(np.int64) for c in range(C)]


def class_lists(masked, classes, K):
    """(ids int64 [n, C, K], vals fp32 [n, C, K], cnt int64 [n, C]) of the masked rows; classes: a list of item arrays (ids outside
    the row are skipped); -1 / 0.0 past cnt."""
    n, width = masked.shape
    C = len(classes)
    ids, vals, cnt = np.full((n, C, K), -1, np.int64), np.zeros((n, C, K), np.float32), np.zeros((n, C), np.int64)
    for c, items in enumerate(classes):
        items = np.asarray(items, dtype=np.int64)
        items = items[(items >= 0) & (items < width)]
        for r in range(n):
            s = masked[r, items]
            o = np.lexsort((items, -(s + np.float32(0.0))))
            o = o[s[o] > -np.inf][:K]
            cnt[r, c] = o.size
            ids[r, c, :o.size], vals[r, c, :o.size] = items[o], s[o]
    return ids, vals, cnt


def shelf_order(vals, cnt):
    """Per row the classes with cnt > 0 by (first entry's score descending as floats, class id ascending)."""
    out = []
    for r in range(cnt.shape[0]):
        cls = [c for c in range(cnt.shape[1]) if cnt[r, c] > 0]
        out.append(np.array(sorted(cls, key=lambda c: (-(float(vals[r, c, 0]) + 0.0), c)), dtype=np.int64))
    return out


def cap_lists(masked, classes, k, cap):
    """(ids int64 [n, k], vals fp32 [n, k], cls int64 [n, k]) of the masked rows, -1 / 0.0 / -1 past a row's entries."""
    n = masked.shape[0]
    m = min(cap, k)
    ci, cv, cc = class_lists(masked, classes, m)
    ids, vals, cls = np.full((n, k), -1, np.int64), np.zeros((n, k), np.float32), np.full((n, k), -1, np.int64)
    for r in range(n):
        ent = [(-(float(cv[r, c, q]) + 0.0), int(ci[r, c, q]), c, cv[r, c, q]) for c in range(len(classes)) for q in range(cc[r, c])]
        ent.sort(key=lambda e: (e[0], e[1]))
        for q, e in enumerate(ent[:k]):
            ids[r, q], vals[r, q], cls[r, q] = e[1], e[3], e[2]
    return ids, vals, cls


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
