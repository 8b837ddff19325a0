"""Scoring items the model was not trained on, restated in torch on the CPU (a helper module, not a test module):

    P[j, 0:d] = f_j E      P[j, d] = f_j.Bp      x_uj = Tu_u.P[j, 0:d] + P[j, d]      map[p, c] = F[row_p, c] w_{u_p c}
                                                                                        w_uc = Bp[c] + sum_x E[c,x] Tu[u,x]

in float64 (the reference) or float32 (one sample of float32 rounding: the scale of the tests' allowances).  There is no Gi / Bi
term.  bf16 features: bprx_project_rows multiplies the bf16-exact features with the bf16-ROUNDED [E|Bp] (the image that projects
the catalogue), so `projection` and `scores` round E and Bp with orc.bf16_round first; `explain` reads the fp32 masters, as
bprx_feat_explain_new and tests/feat_explain_ref.py do.  F: the DEQUANTISED [n, D] table."""
import numpy as np
import torch

from oracle import oracle as orc


def _t(x, dtype):
    return (x.detach().cpu() if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))).to(dtype)


def _weights(E, Bp, feat_dtype):
    E, Bp = _t(E, torch.float32).numpy(), _t(Bp, torch.float32).numpy().reshape(-1)
    if feat_dtype == "bf16":
        E, Bp = orc.bf16_round(E), orc.bf16_round(Bp)
    return E, Bp


def projection(F, E, Bp, feat_dtype="fp32", dtype=torch.float64):
    """P [n, d + 1] (the columns that exist; the padding up to the row stride is zero) as a numpy array of `dtype`."""
    E, Bp = _weights(E, Bp, feat_dtype)
    F = _t(F, dtype)
    return torch.cat([F @ _t(E, dtype), (F @ _t(Bp, dtype))[:, None]], 1).numpy()


def scores(Tu, F, E, Bp, u0, u1, feat_dtype="fp32", dtype=torch.float64):
    """The visual score block [u1 - u0, n] as a numpy array of `dtype`."""
    P = torch.as_tensor(projection(F, E, Bp, feat_dtype, dtype))
    d = P.shape[1] - 1
    return (_t(Tu, dtype)[u0:u1] @ P[:, :d].T + P[:, d][None, :]).numpy()


def explain(Tu, F, E, Bp, users, rows, ncols, dtype=torch.float64):
    """{'map' [n, ncols], 'score' [n]} from the master weights, as numpy arrays of `dtype`."""
    u, r = torch.as_tensor(np.asarray(users)).long().reshape(-1), torch.as_tensor(np.asarray(rows)).long().reshape(-1)
    w = _t(Bp, dtype).reshape(-1)[None, :ncols] + _t(Tu, dtype)[u] @ _t(E, dtype)[:ncols].T
    m = _t(F, dtype)[r][:, :ncols] * w
    return {"map": m.numpy(), "score": m.sum(1).numpy()}
