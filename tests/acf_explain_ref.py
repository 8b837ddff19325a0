"""The explanation read-out of ACF, restated on tests/acf_ref.py's ACFRef in the literal order of ACF.py:135-181: for a pair
(u, i) and the history P(u)
    x_ui = g'_u . Gi_i = g_u . Gi_i + sum_l alpha_l (Pi_l . Gi_i) = base + sum_l c_l
with alpha the item-level and beta_l the component-level attention exactly as ACFRef.profile forms them.  `dtype=torch.float32`
runs the same code on float32 tensors: its deviation from float64 is the unit of the GPU test's allowances
(tests/test_gpu_acf_explain.py).  Per-item quantities are computed once per DISTINCT history item and gathered (a 3 000-entry
history over 40 items would otherwise hold 3 000 feature maps); every row's arithmetic is the one of ACFRef.profile."""
import numpy as np
import torch

from acf_ref import ACFRef

TOL_MULT = 32.0          # the convention of tests/acf_full_ref.py (reasons there)
FIELDS = ("score", "base", "alpha", "contrib", "beta")


class ACFExplainRef(ACFRef):
    def __init__(self, tables, F, dtype=torch.float64):
        super().__init__(tables, F)
        self.dtype = dtype
        if dtype != torch.float64:
            self.p = {n: v.to(dtype) for n, v in self.p.items()}
            self.F = self.F.to(dtype)
        self._att = {}

    def attention(self, u, hist):
        """(alpha [L], beta [L, M]) of user u over the history entries, ACF.py:135-181."""
        key = (int(u), tuple(int(x) for x in hist))
        if key in self._att:
            return self._att[key]
        p = self.p
        g_u = p["Gu"][u]
        M = self.F.shape[1]
        if len(hist) == 0:
            out = (torch.zeros(0, dtype=self.dtype), torch.zeros((0, M), dtype=self.dtype))
            self._att[key] = out
            return out
        distinct = sorted(set(key[1]))
        where = {l: n for n, l in enumerate(distinct)}
        h = torch.as_tensor(distinct, dtype=torch.long)
        f_i = self.F[h]                                                                   # [Ld, M, C]
        b = p["component.W_0_u"].T @ g_u + torch.tensordot(f_i, p["component.W_0_i"], dims=([2], [0])) + p["component.b_0"]
        b = torch.relu(b)
        b = torch.tensordot(b, p["component.W_1"], dims=([2], [1])) + p["component.b_1"]   # [Ld, M, 1]
        beta = torch.softmax(b.squeeze(-1), dim=1)
        x_l = (beta.unsqueeze(2) * f_i).sum(1)                                            # [Ld, C]
        g_i, p_i = p["Gi"][h], p["Pi"][h]
        a = (p["item.W_0_u"].T @ g_u + g_i @ p["item.W_0_iv"] + p_i @ p["item.W_0_ip"] + x_l @ p["item.W_0_ix"]
             + p["item.b_0"])
        a = torch.relu(a) @ p["item.W_1"].T + p["item.b_1"]                                # [Ld, 1]
        idx = torch.as_tensor([where[l] for l in key[1]], dtype=torch.long)
        alpha = torch.softmax(a.reshape(-1)[idx], dim=0)                                  # over the ENTRIES
        out = (alpha, beta[idx])
        self._att[key] = out
        return out

    def explain(self, u, i, hist):
        """dict: base, score (0-d), alpha [L], contrib [L], beta [L, M] as float64 numpy."""
        p = self.p
        alpha, beta = self.attention(u, hist)
        g_i = p["Gi"][int(i)]
        base = (p["Gu"][int(u)] * g_i).sum()
        if len(hist):
            d = p["Pi"][torch.as_tensor([int(x) for x in hist], dtype=torch.long)] @ g_i
            contrib = alpha * d
            score = base + contrib.sum()
        else:
            contrib = torch.zeros(0, dtype=self.dtype)
            score = base.clone()
        return {"base": base.double().numpy(), "score": score.double().numpy(), "alpha": alpha.double().numpy(),
                "contrib": contrib.double().numpy(), "beta": beta.double().numpy()}


def explain_pairs(tables, F, users, items, lists, dtype):
    ref = ACFExplainRef(tables, F, dtype)
    return [ref.explain(int(u), int(i), lists[int(u)]) for u, i in zip(users, items)]


def allowances(r64, r32):
    """Per output: TOL_MULT x the float32 twin's max-abs deviation from float64 over all pairs of the case."""
    out = {}
    for n in FIELDS:
        dev = 0.0
        for a, b in zip(r64, r32):
            if a[n].size:
                dev = max(dev, float(np.abs(a[n] - b[n]).max()))
        out[n] = TOL_MULT * dev
    return out
