"""Similar items restated in torch on the CPU (a helper module, not a test module):

    z_i = Gi_i (latent) | f_i E (visual) | [Gi_i | f_i E] (both)
    rn_i = 1 / sqrt(sum_x z_ix^2), 0 for a zero row        s(q, j) = <z_q, z_j> (rn_q rn_j)

in float64 (the reference) or float32 (one sample of float32 rounding: the scale of the tests' allowances).  bf16 features: the
projections of the catalogue and of rows from outside it multiply the bf16-exact features with the bf16-ROUNDED E, so
item_vectors rounds E as new_items_ref._weights does.  F: the DEQUANTISED [n, D] table."""
import numpy as np
import torch

import new_items_ref as N

SPACES = ("latent", "visual", "both")


def item_vectors(tables, space, feat_dtype="fp32", dtype=torch.float64, F=None):
    """z [n, w] as a numpy array of `dtype` for the items of `tables` (F: the visual vectors of these feature rows instead)."""
    if space not in SPACES:
        raise ValueError(space)
    if F is not None and space != "visual":
        raise ValueError("rows from outside the catalogue have a visual vector only")
    if space == "latent":
        return N._t(tables["Gi"], dtype).numpy()
    E, _ = N._weights(tables["E"], tables["Bp"], feat_dtype)
    V = N._t(tables["F"] if F is None else F, dtype) @ N._t(E, dtype)
    return (V if space == "visual" else torch.cat([N._t(tables["Gi"], dtype), V], 1)).numpy()


def rnorm(z, dtype=torch.float64):
    z = N._t(z, dtype)
    s = (z * z).sum(1)
    return torch.where(s > 0, 1.0 / torch.sqrt(s), torch.zeros_like(s)).numpy()


def cosine(z, dtype=torch.float64, zq=None):
    """s [nq, n]: the cosine of every row of zq (None: of z itself) with every row of z, as a numpy array of `dtype`."""
    zt = N._t(z, dtype)
    qt = zt if zq is None else N._t(zq, dtype)
    f = torch.as_tensor(rnorm(qt, dtype))[:, None] * torch.as_tensor(rnorm(zt, dtype))[None, :]
    return ((qt @ zt.T) * f).numpy()
