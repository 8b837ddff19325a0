"""Restatement of bprx_af_explain (include/bprx.h) on tests/attentive_ref.py's AttentiveRef, float64 by default: the exact split of
an AttentiveFashion score over its three modalities and of the edges share over the 112 x 112 pooling windows,

    x_ui    = sum_l s_l,       s_l  = alpha_l * sum_k g_uk c_lk g_ik          l = colour, edges, class
    s_edges = sum_p S(p),      S(p) = (alpha_e / 12544) * sum_c v_c A_c(p)
    v_c     = sum_k W2e[c, k] g_uk g_ik
    A_c(p)  = max over the 2x2 window p of relu(conv_c + b_c)

with alpha the value AttentiveRef.score reports, held fixed.  The conv is AttentiveRef.pooled's with its max_pool2d and without the
mean; everything after it is the formulas above, literally.  `dtype=torch.float32` runs the same statement in float32: its max-abs
deviation from the float64 run, times TOL_MULT, is the allowance of the GPU tests (the convention of tests/acf_explain_ref.py: one
sample of float32 rounding times a factor for the other summation order and the three-term bf16 weight split)."""
import numpy as np
import torch
import torch.nn.functional as Fn

from attentive_ref import AttentiveRef

WIN = 112
GRIDS = (1, 2, 4, 7, 8, 14, 16, 28, 56, 112)
TOL_MULT = 32.0
FIELDS = ("parts", "map", "peak_val")


def window_maps(ref, items):
    """A [n, 64, 112, 112] of the listed items."""
    p = ref.p
    x = (ref.edges[torch.as_tensor(np.asarray(items)).long()].to(ref.dt) / 255.0).unsqueeze(1)
    w = p["edges.conv"].reshape(5, 5, 64).permute(2, 0, 1).unsqueeze(1)
    return Fn.max_pool2d(torch.relu(Fn.conv2d(x, w, p["edges.conv_b"], padding=2)), 2)


def rebin(S, G):
    """[n, 112, 112] window values -> [n, G * G] cell sums, cells row-major."""
    n, cs = S.shape[0], WIN // G
    return S.reshape(n, G, cs, G, cs).sum((2, 4)).reshape(n, G * G)


def explain(tables, inputs, users, items, grid, dtype=torch.float64, chunk=4):
    """dict of numpy float64 arrays for the pairs: score [n], alpha [n, 3], parts [n, 3], windows [n, 112, 112] (= S), map
    [n, grid * grid], peak_val [n] (the largest cell)."""
    ref = AttentiveRef(tables, *inputs, dtype=dtype)
    u, i = torch.as_tensor(np.asarray(users)).long(), torch.as_tensor(np.asarray(items)).long()
    n = u.numel()
    with torch.no_grad():
        x, alpha, enc = ref.call(u, i)
        gu, gi = ref.p["Gu"][u], ref.p["Gi"][i]
        t = torch.stack([(gu * c * gi).sum(1) for c in enc], 1)                        # [n, 3]
        parts = alpha * t
        v = (gu * gi) @ ref.p["edges.W2"].t()                                          # [n, 64]
        S = torch.empty((n, WIN, WIN), dtype=dtype)
        for r0 in range(0, n, chunk):
            A = window_maps(ref, i[r0:r0 + chunk])
            S[r0:r0 + chunk] = (alpha[r0:r0 + chunk, 1] / (WIN * WIN)).reshape(-1, 1, 1) * (v[r0:r0 + chunk, :, None, None] * A).sum(1)
        m = rebin(S, grid) if n else torch.empty((0, grid * grid), dtype=dtype)
        pv = m.max(1).values if n else torch.empty(0, dtype=dtype)
    f = lambda z: z.double().numpy()
    return {"score": f(x), "alpha": f(alpha), "parts": f(parts), "windows": f(S), "map": f(m), "peak_val": f(pv)}


def allowances(r64, r32):
    """TOL_MULT x the max-abs deviation of the float32 restatement from the float64 one, per output field."""
    return {f: TOL_MULT * float(np.abs(r64[f] - r32[f]).max()) if r64[f].size else 0.0 for f in FIELDS}
