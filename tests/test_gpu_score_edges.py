"""Both score-row kernels behind bprx_score_block -- k_score_gemm (128 x 128 tiles of the fp32 MFMA GEMM; even k and d) and
k_score_block (one thread per score; odd k or d) -- against float64 numpy of

    x[u, i] = Bi[i] + Gu[u].Gi[i] (+ Tu[u].P_i[:d] + P_i[d])

at the tile edges: more than one user tile (blockIdx.y > 0), a full 128-row tile followed by a partial one, a block that
starts at u0 != 0 and crosses tiles (the (ur - u0) * I write offset), one-row and one-column tiles, and factor widths whose
last 16-wide K chunk is partial.

Bound, per element, derived and not measured: an fp32 sum of m terms in ANY order, each term one rounded product, is within
gamma_m * sum |terms| of the exact value, gamma_m = m u / (1 - m u), u = 2^-24 (Higham, Accuracy and Stability of Numerical
Algorithms, section 3.1).  A score has n = k + d + 2 terms; the tests allow gamma_{n+1}:

    |got - ref| <= gamma_{n+1} (|Bi| + sum |gu gi| + sum |tu p| + |p_d|)          -- no absolute term.

A dropped or doubled K step moves an element by about one of its terms, 1e5 times the bound at these widths; a stale or
misplaced element is caught by the NaN prefill: `out` is a buffer with two sentinel rows behind the block, all NaN before the
call; afterwards every element of the block is finite and the sentinels are NaN still.

VBPR isolates the score kernel from the projection: F in {0, 1, 2, 3}, E and Bp in {-2, ..., 2} / 4 make every product and
partial sum of P = F.[E|Bp] exact in bf16 and fp32 alike, whatever the order.  That is asserted first: a handle with one-hot
Tu rows reads P back through score_block (as tests/test_gpu_projections.py does) and must return the float64 P bit for bit.
The issue's feature width D = 64 exists for fp32 features only (bf16 needs D % 128 == 0) and test_gpu_projections.py runs none of
these d with bf16, so the grid is fp32; one extra case, k 18, d 28, D 256 with bf16 features (a width that module runs with
bf16 at two column tiles), puts the GEMM behind the bf16 projection.
Reference: BPRMF.py:78-85, VBPR.py:88-97."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U_B, I_B = 300, 257                     # user tiles 128 / 128 / 44, item tiles 128 / 128 / 1
RANGES_B = [(0, 300), (5, 262), (127, 129), (299, 300)]      # (5, 262): 257 rows from u0 = 5 -> tiles of 128 / 128 / 1
K_GEMM, K_SCALAR = (2, 14, 16, 18, 34, 128), (1, 3, 17)
U_V, I_V = 140, 130
RANGES_V = [(0, 140), (3, 135)]


def _gamma(m):
    u = 2.0 ** -24
    return m * u / (1.0 - m * u)


@functools.lru_cache(maxsize=None)
def _bprmf_tables(U, I, k):
    rs = np.random.RandomState(100 * k + I)
    return (rs.standard_normal((U, k)).astype(np.float32), rs.standard_normal((I, k)).astype(np.float32),
            rs.standard_normal(I).astype(np.float32))


@functools.lru_cache(maxsize=None)
def _bprmf_ref(U, I, k):
    """float64 scores and the sum of the absolute terms of every score, computed once per table set."""
    Gu, Gi, Bi = (a.astype(np.float64) for a in _bprmf_tables(U, I, k))
    ref, mag = Bi[None, :] + Gu @ Gi.T, np.abs(Bi)[None, :] + np.abs(Gu) @ np.abs(Gi).T
    ref.setflags(write=False)
    mag.setflags(write=False)
    return ref, mag


def _check_block(e, u0, u1, I, ref, mag, n_terms, what):
    n = u1 - u0
    buf = torch.full((n + 2, I), float("nan"), dtype=torch.float32, device="cuda")
    e.score_block(u0, u1, out=buf)
    e.sync_check()
    got = buf.cpu().numpy()
    assert np.isfinite(got[:n]).all(), "%s: %d elements of the block were not written" % (what, int((~np.isfinite(got[:n])).sum()))
    assert np.isnan(got[n:]).all(), "%s: a write landed behind the block" % what
    err = np.abs(got[:n].astype(np.float64) - ref[u0:u1])
    bnd = _gamma(n_terms + 1) * mag[u0:u1]
    ratio = err / bnd
    w = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    print("%s: worst |err| / bound = %.3f at (u %d, i %d)" % (what, ratio[w], u0 + w[0], w[1]))
    assert (err <= bnd).all(), "%s: %d of %d scores outside the bound, worst %.3g x bound at (u %d, i %d): got %r, want %r" % (
        what, int((err > bnd).sum()), err.size, ratio[w], u0 + w[0], w[1], float(got[w]), float(ref[u0 + w[0], w[1]]))


def _bprmf(U, I, k):
    from fashionvisualexpl_recommend_amd.engine import Engine
    Gu, Gi, Bi = _bprmf_tables(U, I, k)
    return Engine(model="bprmf", num_users=U, num_items=I, embed_k=k, optimizer="sgd", max_batch=8).bind(Gu=Gu, Gi=Gi, Bi=Bi)


@pytest.mark.parametrize("k", K_GEMM + K_SCALAR, ids=["gemm-k%d" % k for k in K_GEMM] + ["scalar-k%d" % k for k in K_SCALAR])
def test_bprmf_score_block_at_tile_edges(k):
    e = _bprmf(U_B, I_B, k)
    ref, mag = _bprmf_ref(U_B, I_B, k)
    for u0, u1 in RANGES_B:
        _check_block(e, u0, u1, I_B, ref, mag, k + 2, "k %d rows [%d, %d)" % (k, u0, u1))
    e.close()


@pytest.mark.parametrize("k", [14, 3], ids=["gemm-k14", "scalar-k3"])
def test_bprmf_score_block_three_items(k):
    e = _bprmf(U_B, 3, k)
    ref, mag = _bprmf_ref(U_B, 3, k)
    for u0, u1 in RANGES_B:
        _check_block(e, u0, u1, 3, ref, mag, k + 2, "I 3, k %d rows [%d, %d)" % (k, u0, u1))
    e.close()


# ---- VBPR ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _vbpr_tables(k, d, D):
    rs = np.random.RandomState(1000 * k + d)
    F = rs.randint(0, 4, size=(I_V, D)).astype(np.float32)
    E = (rs.randint(-2, 3, size=(D, d)) / 4.0).astype(np.float32)
    Bp = (rs.randint(-2, 3, size=D) / 4.0).astype(np.float32)
    P = F.astype(np.float64) @ np.concatenate([E, Bp[:, None]], 1).astype(np.float64)          # [I, d + 1], exact
    t = dict(Gu=rs.standard_normal((U_V, k)).astype(np.float32), Gi=rs.standard_normal((I_V, k)).astype(np.float32),
             Bi=rs.standard_normal(I_V).astype(np.float32), Tu=rs.standard_normal((U_V, d)).astype(np.float32))
    f = {n: a.astype(np.float64) for n, a in t.items()}
    ref = f["Bi"][None, :] + f["Gu"] @ f["Gi"].T + f["Tu"] @ P[:, :d].T + P[:, d][None, :]
    mag = (np.abs(f["Bi"])[None, :] + np.abs(f["Gu"]) @ np.abs(f["Gi"]).T + np.abs(f["Tu"]) @ np.abs(P[:, :d]).T +
           np.abs(P[:, d])[None, :])
    for a in (P, ref, mag):
        a.setflags(write=False)
    return t, F, E, Bp, P, ref, mag


def _vbpr(U, k, d, D, dtype, tables, F, E, Bp):
    from fashionvisualexpl_recommend_amd.engine import Engine
    return Engine(model="vbpr", num_users=U, num_items=I_V, embed_k=k, embed_d=d, feat_dim=D, feat_dtype=dtype,
                  optimizer="sgd", max_batch=8).bind(F=F, E=E, Bp=Bp, **tables)


VBPR_CASES = [pytest.param(34, 20, 64, "fp32", id="gemm-k34-d20"), pytest.param(16, 64, 64, "fp32", id="gemm-k16-d64"),
              pytest.param(18, 12, 64, "fp32", id="gemm-k18-d12"), pytest.param(8, 5, 64, "fp32", id="scalar-k8-d5"),
              pytest.param(5, 8, 64, "fp32", id="scalar-k5-d8"), pytest.param(18, 28, 256, "bf16", id="gemm-k18-d28-bf16")]


@pytest.mark.parametrize("k,d,D,dtype", VBPR_CASES)
def test_vbpr_score_block_at_tile_edges(k, d, D, dtype):
    t, F, E, Bp, P, ref, mag = _vbpr_tables(k, d, D)
    # the projection is exact: one-hot visual users read P back, score[u, i] = P[i, u] + P[i, d] (u < d), P[i, d] (u = d)
    Tu1 = np.zeros((d + 1, d), np.float32)
    Tu1[np.arange(d), np.arange(d)] = 1.0
    zero = dict(Gu=np.zeros((d + 1, k), np.float32), Gi=np.zeros((I_V, k), np.float32), Bi=np.zeros(I_V, np.float32), Tu=Tu1)
    e1 = _vbpr(d + 1, k, d, D, dtype, zero, F, E, Bp)
    back = e1.score_block(0, d + 1).cpu().numpy()
    e1.sync_check()
    e1.close()
    want = np.concatenate([P[:, :d].T + P[:, d][None, :], P[:, d][None, :]], 0)
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
    assert np.array_equal(back.view(np.uint32), want.astype(np.float32).view(np.uint32)), "the projection is not exact"
    e = _vbpr(U_V, k, d, D, dtype, t, F, E, Bp)
    for u0, u1 in RANGES_V:
        _check_block(e, u0, u1, I_V, ref, mag, k + d + 2, "k %d d %d %s rows [%d, %d)" % (k, d, dtype, u0, u1))
    e.close()
