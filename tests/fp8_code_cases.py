"""The inputs and expected outputs of tests/test_gpu_fp8_codes.py, built on the host so that tests/test_fp8_code_cases_cpu.py can hold
what the GPU test relies on before any GPU run (a helper module, not a test module; the pattern of tests/af_step_cases.py).

Everything here is exact: feat_scale FS and the scale 2^J of [E|Bp] are powers of two, every product is (4-bit significand) x (4-bit
significand), every sum has one non-zero term (two where a score adds P[t, n] and P[t, d]: multiples of 2^-9 below 2^10 times a 4-bit
significand, 23 bits), so the expected arrays are float64 values that are float32 numbers, compared with ==.

  code table     VAL[c] = (-1)^s 2^(e-7) (1 + m/8), subnormals 2^-6 m/8; CODES = the 254 codes that are numbers (0x7f, 0xff: NaN)
  one-hot items  item (code a, byte position p) = row LEAD + 16 index(a) + p holds code a in column p + 16 (index(a) % (D/16)) and
                 zeros elsewhere; LEAD zero rows in front (a (code, 0..15) group straddles two 16-row tiles), TAIL behind: I = 4 101
  [E|Bp]         the value of code CODES[(c + 3 n) % 254] over 2^J at (column c, output n): all 254 codes at every byte position c % 16
  cast probes    x / 2^J in E under a one-hot feature 1.0: the midpoint of every pair of adjacent code values and its two float32
                 neighbours in both signs, +-0, 2^-10, 3 2^-10, the last float32 below 2^-6, +-448
  bf16 probes    float32 values on bf16 ties (to even both ways, one carrying into the exponent) and their float32 neighbours"""
import numpy as np
import torch

NAN_CODES = (0x7f, 0xff)
CODES = np.array([c for c in range(256) if c not in NAN_CODES], dtype=np.int64)
NC = len(CODES)                                              # 254
LEAD, TAIL = 5, 32                                           # all-zero rows in front of and behind the 254 x 16 one-hot items
I_ITEMS = LEAD + 16 * NC + TAIL                              # 4 101: I % 32 == 5
FS = 256.0                                                   # feat_scale of the decode cases: the codes hold f * FS
J = 3                                                        # max|E,Bp| = 448 / 2^J: sE = 2^J, qs[1] = 1 / (FS 2^J)
ONE = 0x38                                                   # the code of 1.0
GROUP = 32                                                   # codes per backward batch (x 16 positions = one item per column at D 512)


def code_value(c):
    """the value of e4m3fn code c from the format's definition (float; NaN for S.1111.111)"""
    s, e, m = c >> 7, (c >> 3) & 15, c & 7
    if e == 15 and m == 7:
        return float("nan")
    v = 2.0 ** -6 * m / 8.0 if e == 0 else 2.0 ** (e - 7) * (1.0 + m / 8.0)
    return -v if s else v


VAL = np.array([code_value(c) for c in range(256)], dtype=np.float64)


def item_of(ci, p):
    """row of the one-hot item of code CODES[ci] at byte position p"""
    return LEAD + 16 * ci + p


def zero_items():
    return np.concatenate([np.arange(LEAD), np.arange(LEAD + 16 * NC, I_ITEMS)])


def item_codes(D):
    """(code, column) of every item, -1 / -1 for the all-zero rows"""
    code = np.full(I_ITEMS, -1, dtype=np.int64)
    col = np.full(I_ITEMS, -1, dtype=np.int64)
    ci, p = np.meshgrid(np.arange(NC), np.arange(16), indexing="ij")
    t = item_of(ci, p).ravel()
    code[t] = CODES[ci.ravel()]
    col[t] = (p + 16 * (ci % (D // 16))).ravel()
    return code, col


def feature_codes(D):
    """uint8 [I, D]: the one-hot code table (bound as torch.float8_e4m3fn through .view)"""
    code, col = item_codes(D)
    F = np.zeros((I_ITEMS, D), dtype=np.uint8)
    on = code >= 0
    F[np.nonzero(on)[0], col[on]] = code[on].astype(np.uint8)
    return F


def eb_codes(D, d):
    """uint8 [D, d + 1]: the codes of [E|Bp] 2^J"""
    c, n = np.meshgrid(np.arange(D), np.arange(d + 1), indexing="ij")
    return CODES[(c + 3 * n) % NC].astype(np.uint8)


def eb_tables(D, d):
    """E [D, d] and Bp [D] as float32: e4m3-exact at the scale 2^J, the largest magnitude 448 / 2^J"""
    v = (VAL[eb_codes(D, d)] / 2.0 ** J).astype(np.float32)
    return np.ascontiguousarray(v[:, :d]), np.ascontiguousarray(v[:, d])


def forward_expected(D, d, fs=FS):
    """P [I, d + 1] in float64: val(a_t) val(b(c_t, n)) / (fs 2^J); the rows of the all-zero items are 0"""
    code, col = item_codes(D)
    on = code >= 0
    P = np.zeros((I_ITEMS, d + 1), dtype=np.float64)
    P[on] = VAL[code[on]][:, None] * VAL[eb_codes(D, d)][col[on]] / (fs * 2.0 ** J)
    return P


def scores_of(P):
    """score_block(0, d + 1) of one-hot visual users over zero Gu / Gi / Bi: [d + 1, I], row n < d = P[:, n] + P[:, d], row d = P[:, d]"""
    d = P.shape[1] - 1
    return np.concatenate([(P[:, :d] + P[:, d:]).T, P[:, d:].T], 0)


def one_hot_users(d):
    Tu = np.zeros((d + 1, d), dtype=np.float32)
    Tu[np.arange(d), np.arange(d)] = 1.0
    return Tu


def is_f32(a):
    """every float64 value of a is a float32 number"""
    a = np.asarray(a, dtype=np.float64)
    with np.errstate(over="ignore"):
        return bool(np.array_equal(a.astype(np.float32).astype(np.float64), a))


# ---- backward: one batch per group of GROUP codes x 16 positions ----------------------------------------------------------
def n_groups():
    return (NC + GROUP - 1) // GROUP


def backward_case(g, D, d, seed=0, fs=FS):
    """Group g: every one-hot item of codes CODES[32 g .. 32 g + 31] is the positive of one triplet of a user of its own, the negative
    is an all-zero row.  Zero E / Bp / Gu / Gi / Bi: g = -0.5, W[pos] = -0.5 [Tu_u | 1], so dE|dBp[c_t] = val(a_t) W[t] / fs (float64
    [D, d + 1]; the columns no item of the group owns stay 0).  Needs D == 16 * GROUP: one item per column."""
    assert D == 16 * GROUP
    cis = np.arange(g * GROUP, min(NC, (g + 1) * GROUP))
    ci, p = np.meshgrid(cis, np.arange(16), indexing="ij")
    pos = item_of(ci, p).ravel()
    B = len(pos)
    z = zero_items()
    neg = z[LEAD + np.arange(B) % TAIL]                     # the trailing zero rows in turn
    rs = np.random.RandomState(seed + 100 * g + d)
    m = rs.randint(-4, 5, size=(B, d))
    m[m == 0] = 3                                           # no zero in W: a lost term cannot hide
    Tu = (m / 8.0).astype(np.float32)
    W = -0.5 * np.concatenate([Tu.astype(np.float64), np.ones((B, 1))], 1)
    code, col = item_codes(D)
    assert len(np.unique(col[pos])) == B
    ref = np.zeros((D, d + 1), dtype=np.float64)
    ref[col[pos]] = VAL[code[pos]][:, None] * W / fs
    return dict(u=np.arange(B, dtype=np.int32), i=pos.astype(np.int32), j=neg.astype(np.int32), Tu=Tu, W=W, ref=ref, B=B)


# ---- the cast -------------------------------------------------------------------------------------------------------------
NONNEG = VAL[:0x7f]                                         # the 127 non-negative code values, ascending: 126 boundaries
MIDPOINTS = ((NONNEG[:-1] + NONNEG[1:]) / 2.0).astype(np.float32)


def cast_probes(with_max=True):
    """float32 x: the list of the module docstring (with_max=False: without +-448, for the cases that place one maximum)"""
    mid = MIDPOINTS
    lo, hi = np.nextafter(mid, np.float32(-np.inf)), np.nextafter(mid, np.float32(np.inf))
    pos = np.stack([lo, mid, hi], 1).ravel()
    extra = [0.0, -0.0, 2.0 ** -10, 3 * 2.0 ** -10, float(np.nextafter(np.float32(2.0 ** -6), np.float32(0)))]
    if with_max:
        extra += [448.0, -448.0]
    return np.concatenate([pos, -pos, np.array(extra, dtype=np.float32)]).astype(np.float32)


def torch_cast(x):
    """torch's CPU float32 -> float8_e4m3fn cast, as float32 values (numpy in, numpy out)"""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.float8_e4m3fn).float().numpy()


# where the one entry of magnitude 448 / 2^J sits: (name, table, index, sign)
MAX_PLACES = [("E-first", "E", (0, 0), 1.0), ("E-last", "E", (-1, -1), 1.0), ("Bp-first", "Bp", (0,), 1.0), ("Bp-last", "Bp", (-1,), 1.0),
              ("E-negative", "E", (257, 7), -1.0)]


def probe_tables(probes, D, d, place=None, scale=2.0 ** J):
    """E [D, d] (the probes over `scale`, repeated in row-major order) and Bp [D] (zeros); place: one of MAX_PLACES, its entry set to
    sign * 448 / scale.  Returns E, Bp and X = [E|Bp] * scale [D, d + 1] (float32, exact)."""
    n = len(probes)
    X = np.zeros((D, d + 1), dtype=np.float32)
    X[:, :d] = probes[np.arange(D * d) % n].reshape(D, d)
    if place is not None:
        _, tab, idx, sign = place
        if tab == "E":
            X[:, :d][idx] = sign * 448.0
        else:
            X[:, d][idx] = sign * 448.0
    EB = (X / np.float32(scale)).astype(np.float32)
    return np.ascontiguousarray(EB[:, :d]), np.ascontiguousarray(EB[:, d]), X


def probe_items(D, lead=LEAD):
    """one-hot items of the probe cases: item lead + c holds `one` in column c; `lead` zero rows in front: I = D + lead (I % 32 != 0)"""
    return D + lead


def probe_features_fp8(D, lead=LEAD):
    F = np.zeros((D + lead, D), dtype=np.uint8)
    F[lead + np.arange(D), np.arange(D)] = ONE
    return F


def probe_expected(Xq, lead=LEAD, fs=1.0, scale=2.0 ** J):
    """score_block(0, d + 1) [d + 1, D + lead] for the rounded image Xq [D, d + 1] of [E|Bp] * scale under one-hot features of 1.0"""
    P = np.zeros((Xq.shape[0] + lead, Xq.shape[1]), dtype=np.float64)
    P[lead:] = Xq.astype(np.float64) / (fs * scale)
    return scores_of(P)


# ---- the bf16 image -------------------------------------------------------------------------------------------------------
def bf16_probes():
    """float32 values whose low 16 bits are 0x8000 (a tie), 0x7fff and 0x8001 (its neighbours) over bf16 patterns with an even and an odd
    last bit (ties to even go down / up), with mantissa 0x7f (the tie carries into the exponent), exponents 2^-12 .. 2^9, both signs.
    Normal numbers only: what the bf16 MFMA does with subnormal inputs on this part has not been measured."""
    his = [0x3f80, 0x3f81, 0x3f82, 0x3f83, 0x3ffe, 0x3fff, 0x407f, 0x3eff, 0x3a00, 0x3a01, 0x39ff, 0x447e, 0x447f, 0x4400, 0x4401,
           0x3dcc, 0x3dcd, 0x4049, 0x402d]
    lows = [0x8000, 0x7fff, 0x8001, 0x0000, 0xffff, 0x0001]
    u = np.array([(h << 16) | l for h in his for l in lows], dtype=np.uint32)
    u = np.concatenate([u, u | np.uint32(0x80000000)])
    return u.view(np.float32)


def probe_features_bf16(D, lead=LEAD):
    F = np.zeros((D + lead, D), dtype=np.float32)
    F[lead + np.arange(D), np.arange(D)] = 1.0
    return F
