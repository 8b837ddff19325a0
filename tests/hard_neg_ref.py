"""Hard negatives on the host, in numpy (a helper module, not a test module), restated from draw_negative / k_sample_hard of
csrc/bprx_philox.hip and include/bprx.h: candidate c of stream position n is the uniform samplers' rejection draw with the third
counter word c * 2048 + a (attempts a = 0, 1, ..; after 1 024 positives in a row the word c * 2048 + 1024 picks the r-th
non-positive); the negative is the candidate with the largest score, ties to the smallest c, a NaN never ahead of a number.
The user and the positive of a position are the uniform stream's and are taken from the oracle's samplers, which the existing
tests hold the device to."""
import numpy as np

from af_dropout_ref import philox4x32_10
from oracle import oracle as orc

ATTEMPTS, STRIDE, PERM_WORD = 1024, 2048, 0xFFFFFFFE


def counter_word(c, a):
    """The third Philox counter word of attempt a (0 .. 1024; 1024: the fallback) of candidate c."""
    return c * STRIDE + a


def _mulhi32(z, n):
    return ((z.astype(np.uint64) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def candidates(lists, I, seed, first, B, C, epoch=None):
    """(u [B], i [B], cand [B, C]) int32 of stream positions first .. first + B: the Philox stream (epoch None) or positions of
    epoch `epoch` of the epoch walk (first + B within the epoch)."""
    if epoch is None:
        u, i, _ = orc.sample_philox(lists, I, seed, first, B)
        w3 = 0
    else:
        u, i, _ = orc.sample_epoch(lists, I, seed, epoch, first, B)
        w3 = int(epoch)
    seed = int(seed) & (2 ** 64 - 1)
    key = (seed & 0xFFFFFFFF, seed >> 32)
    member = np.zeros((len(lists), I), bool)
    for uu, l in enumerate(lists):
        member[uu, np.asarray(l, np.int64)] = True
    n = np.repeat(first + np.arange(B, dtype=np.uint64), C)                    # [B * C] position, candidate-minor
    c = np.tile(np.arange(C, dtype=np.int64), B)
    uu = np.repeat(u.astype(np.int64), C)
    n_lo, n_hi = (n & np.uint64(0xFFFFFFFF)).astype(np.int64), (n >> np.uint64(32)).astype(np.int64)
    cand = np.zeros(B * C, np.int64)
    active = np.arange(B * C)
    for a in range(ATTEMPTS):
        if not active.size:
            break
        z = philox4x32_10((n_lo[active], n_hi[active], counter_word(c[active], a), w3), key)[:, 2]
        jj = _mulhi32(z, I)
        cand[active] = jj
        active = active[member[uu[active], jj]]
    if active.size:                                                            # 1 024 positives in a row
        z = philox4x32_10((n_lo[active], n_hi[active], counter_word(c[active], ATTEMPTS), w3), key)[:, 2]
        for x, zz in zip(active, z):
            free = np.flatnonzero(~member[uu[x]])
            cand[x] = free[int(_mulhi32(np.asarray([zz]), len(free))[0])]
    return u, i, cand.reshape(B, C).astype(np.int32)


def stream(lists, I, seed, position, B, C, kind):
    """candidates() of B positions of a sampler's stream from `position` on: kind "philox", or "epoch" (position = epoch *
    interactions + position inside the epoch; a window that crosses an epoch boundary is split there, as the sampler splits it)."""
    if kind == "philox":
        return candidates(lists, I, seed, position, B, C)
    N = sum(len(l) for l in lists)
    parts, p = [], position
    while p < position + B:
        e, q = divmod(p, N)
        n = min(position + B - p, N - q)
        parts.append(candidates(lists, I, seed, q, n, C, epoch=e))
        p += n
    return tuple(np.concatenate([w[x] for w in parts]) for x in range(3))


def _rows(t, Ps, u, cand, d):
    """The factor pairs and the bias terms of every score: (a [B, C, k + d], b the same, bias [B, C, 1 or 2]) in float64."""
    u, cand = u.astype(np.int64), cand.astype(np.int64)
    a = [np.broadcast_to(t["Gu"].astype(np.float64)[u][:, None, :], cand.shape + (t["Gu"].shape[1],))]
    b = [t["Gi"].astype(np.float64)[cand]]
    bias = [t["Bi"].astype(np.float64)[cand][..., None]]
    if d:
        a.append(np.broadcast_to(t["Tu"].astype(np.float64)[u][:, None, :], cand.shape + (d,)))
        b.append(Ps.astype(np.float64)[cand][..., :d])
        bias.append(Ps.astype(np.float64)[cand][..., d:d + 1])
    return np.concatenate(a, -1), np.concatenate(b, -1), np.concatenate(bias, -1)


def scores64(t, Ps, u, cand, d=0):
    """s_c = Gu_u.Gi_j + Bi_j (+ Tu_u.Ps_j[:d] + Ps_j[d] with d > 0) in float64, [B, C].  t: the tables as the kernel reads them."""
    a, b, bias = _rows(t, Ps, u, cand, d)
    return (a * b).sum(-1) + bias.sum(-1)


def magnitude(t, Ps, u, cand, d=0):
    """sum_i |a_i b_i| + |bias terms| of the same sums: what the rounding error of an fp32 evaluation scales with."""
    a, b, bias = _rows(t, Ps, u, cand, d)
    return np.abs(a * b).sum(-1) + np.abs(bias).sum(-1)


def choose(scores):
    """The chosen candidate of every row of scores [B, C] (or of one row [C]): the largest wins, ties go to the smallest c, a NaN
    never wins against a number (a row of NaNs keeps candidate 0)."""
    s = np.asarray(scores)
    if s.ndim == 1:
        return int(choose(s[None])[0])
    best = np.zeros(len(s), np.int64)
    sb = s[:, 0].copy()
    for c in range(1, s.shape[1]):
        with np.errstate(invalid="ignore"):
            win = (s[:, c] > sb) | (np.isnan(sb) & ~np.isnan(s[:, c]))
        best[win] = c
        sb[win] = s[win, c]
    return best
