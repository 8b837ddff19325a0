"""The shared adam_tf23 sweep (k_adam_sweep, bprx_sparse.hip) through its thin front engine.adam_rows / bprx_adam_rows: every
model's whole-table sweep is this kernel with this element function (adam_elem, bprx_device.h).  Compared as integers against
a numpy float32 restatement of adam_elem in which every operation is rounded to float32 and nothing is fused: the kernel
compiles with contraction off and correctly rounded sqrt and divide, so the expected distance is 0 ULP.

MAX_ULP = 0 is that reasoning, not a figure taken from the merged kernel: both sides perform the same sequence of correctly
rounded IEEE-754 binary32 operations (multiply, add, subtract, sqrt, divide) on normal numbers, so any distance at all is a
difference in the arithmetic.  The bound has NOT yet been measured on an MI355X against the build that preceded the merged
kernel (k_adam_sparse behind bprx_adam_rows).  The test prints every distance
before it asserts, so the first run records it."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B1, B2, EPS, LR = np.float32(0.9), np.float32(0.999), np.float32(1e-7), 0.01
MAX_ULP = 0
STEPS = 3
# one element; one short of / exactly / one past a workgroup; every thread of the capped grid (4096 x 256) takes a second stride
SIZES = [1, 255, 256, 257, 4096 * 256 + 3]


def _lr_t(t):
    b1, b2, t = np.float32(B1), np.float32(B2), np.float32(t)
    return np.float32(np.float32(LR) * np.sqrt(np.float32(1) - np.power(b2, t)) / (np.float32(1) - np.power(b1, t)))


def _adam_elem(p, m, v, g, lr_t):
    """adam_elem, one float32 rounding per operation, in the function's own order."""
    omb1, omb2 = np.float32(1) - B1, np.float32(1) - B2
    mt = m * B1 + g * omb1
    vt = v * B2 + (g * g) * omb2
    pt = p - lr_t * mt / (np.sqrt(vt) + EPS)
    assert mt.dtype == vt.dtype == pt.dtype == np.float32
    return pt, mt, vt


def _ordered(a):
    i = a.view(np.int32).astype(np.int64)
    return np.where(i < 0, np.int64(-2 ** 31) - i, i)              # monotonic in the float's value; -0.0 and +0.0 coincide


def _ulp(a, b):
    return int(np.abs(_ordered(a) - _ordered(b)).max())


def _grad(rs, n):
    g = (10.0 ** rs.uniform(-3.0, 0.0, n)).astype(np.float32)      # |g| in [1e-3, 1]: no subnormal intermediate
    g[g < np.float32(1e-3)] = np.float32(1e-3)
    g *= rs.choice(np.array([-1.0, 1.0], np.float32), n)
    g[rs.random_sample(n) < 0.5] = 0.0                             # untouched rows: exact zeros on about half
    if n > 1:
        g[0], g[-1] = 0.0, 0.5                                     # both kinds at any size above one
    return g


@pytest.mark.parametrize("n", SIZES)
def test_adam_rows_is_adam_elem_bit_for_bit(n):
    from fashionvisualexpl_recommend_amd import engine
    rs = np.random.RandomState(1000 + n % 997)
    p = rs.uniform(-0.1, 0.1, n).astype(np.float32)
    m = rs.uniform(-0.05, 0.05, n).astype(np.float32)
    v = rs.uniform(1e-5, 1e-2, n).astype(np.float32)
    fresh = rs.random_sample(n) < 0.25                             # never-touched elements: m = v = 0
    if n > 1:
        fresh[0] = True
    m[fresh] = 0.0
    v[fresh] = 0.0
    dp, dm, dv = (torch.as_tensor(a.copy(), device="cuda") for a in (p, m, v))
    for t in range(1, STEPS + 1):
        g = _grad(rs, n)
        lr_t = _lr_t(t)
        dg = torch.as_tensor(g, device="cuda")
        engine.adam_rows(dp, dm, dv, dg, float(lr_t), beta1=float(B1), beta2=float(B2), eps=float(EPS))
        want = _adam_elem(p, m, v, g, lr_t)
        got = tuple(x.cpu().numpy() for x in (dp, dm, dv))
        dist = {name: _ulp(a, b) for name, a, b in zip("pmv", got, want)}
        print("n=%d step %d lr_t=%.9g max ULP distance %s" % (n, t, lr_t, dist))
        assert int(torch.count_nonzero(dg).item()) == 0, "g is not all-zero after the call"
        assert max(dist.values()) <= MAX_ULP, dist
        if MAX_ULP == 0:
            for a, b in zip(got, want):
                assert np.array_equal(a.view(np.int32), b.view(np.int32))
        p, m, v = got                                              # the next step starts from the device's own state
