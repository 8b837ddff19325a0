"""bprx_feat_explain restated in torch on the CPU (a helper module, not a test module): the exact split of the VBPR / GradFashion
score over the feature columns,

    x_ui = Bi_i + Gu_u.Gi_i + sum_c F_ic w_uc        w_uc = Bp[c] + sum_x E[c,x] Tu[u,x]
           `---- base ----'   `--- visual ---'

in float64 (the reference) or float32 (one sample of float32 rounding: the scale of the tests' allowances).  `tables`: Gu [U,k],
Gi [I,k], Bi [I], Tu [U,d], E [D,d], Bp [D] (a factored model: E_eff / Bp_eff) and F [I,D], the DEQUANTISED features (bf16 -> float,
fp8 codes.float() / feat_scale); numpy or torch."""
import numpy as np
import torch

NAMES = ("Gu", "Gi", "Bi", "Tu", "E", "Bp", "F")


def as_tables(tables, dtype=torch.float64):
    f = lambda x: (x.detach().cpu() if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))).to(dtype)
    t = {n: f(tables[n]) for n in NAMES}
    t["Bp"], t["Bi"] = t["Bp"].reshape(-1), t["Bi"].reshape(-1)
    return t


def feat_explain_ref(tables, users, items, ncols, dtype=torch.float64):
    """{'map' [n, ncols], 'base' [n], 'visual' [n], 'score' [n]} as numpy arrays of `dtype`."""
    t = as_tables(tables, dtype)
    u, i = torch.as_tensor(np.asarray(users)).long().reshape(-1), torch.as_tensor(np.asarray(items)).long().reshape(-1)
    w = t["Bp"][None, :ncols] + t["Tu"][u] @ t["E"][:ncols].T                    # [n, ncols]
    m = t["F"][i][:, :ncols] * w
    base = t["Bi"][i] + (t["Gu"][u] * t["Gi"][i]).sum(1)
    visual = m.sum(1)
    return {"map": m.numpy(), "base": base.numpy(), "visual": visual.numpy(), "score": (base + visual).numpy()}


def top_columns(row, top):
    """The list bprx_feat_explain returns for one map row: (columns, values) of the `top` largest entries, values compared as floats
    (+0.0 == -0.0), equal values in ascending column order."""
    order = np.argsort(-np.asarray(row), kind="stable")[:top]
    return order, np.asarray(row)[order]
