"""The AttentiveFashion dropout stream on the host, in numpy (a helper module, not a test module), restated from af_keep4 /
k_af_mask / af_drop of csrc/bprx_attentive.hip: unit u of sample row r of encoder e (0 colour, 1 edges, 2 class) at step s is kept
iff word u % 4 of Philox4x32-10 with the counter (u // 4, r, e, s) and the key (seed & 0xffffffff, seed >> 32) is >= thr,
thr = uint32(float64(float32(rate)) * 2^32).  tests/test_gpu_attentive_shapes.py holds the library to these bits, which pins the
stream that a resumed run relies on (the step index is part of state_dict)."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
LO, S32 = np.uint64(0xFFFFFFFF), np.uint64(32)
WIDTHS = (256, 64, 256)                                      # colour hidden units, pooled edge channels, class hidden units


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., SC'11) of counter words (c0, c1, c2, c3) and key words (k0, k1), each a Python int or an
    array of values below 2^32 (broadcast against each other): the four output words as a uint32 array [..., 4]."""
    c0, c1, c2, c3 = np.broadcast_arrays(*(np.asarray(c, np.uint64) for c in counter))
    k0, k1 = int(key[0]), int(key[1])
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                            # 32 x 32 -> 64 bit products
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ np.uint64(k0), p1 & LO, (p0 >> S32) ^ c3 ^ np.uint64(k1), p0 & LO
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], -1).astype(np.uint32)


def threshold(rate):
    return int(np.float64(np.float32(rate)) * 4294967296.0)


def dropout_masks(seed, step, n_rows, rate):
    """(colour [n_rows, 256], edges [n_rows, 64], class [n_rows, 256]) uint8 keep masks of one step; rate 0: all ones (the library
    then runs without mask and scaling)."""
    seed = int(seed) & (2 ** 64 - 1)
    key = (seed & 0xFFFFFFFF, seed >> 32)
    thr = threshold(rate)
    out = []
    for enc, w in enumerate(WIDTHS):
        if not rate > 0.0:
            out.append(np.ones((n_rows, w), np.uint8))
            continue
        q, r = np.meshgrid(np.arange(w // 4), np.arange(n_rows))                    # [n_rows, w / 4]
        words = philox4x32_10((q, r, enc, int(step) & 0xFFFFFFFF), key)             # [n_rows, w / 4, 4]
        out.append((words >= np.uint32(thr)).astype(np.uint8).reshape(n_rows, w))
    return tuple(out)
