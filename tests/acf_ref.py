"""float64 restatement of the reference's ACF (src/recommender/models/ACF.py) in its literal order: the component attention forms
x_l = sum_m beta_lm f_lm and only then applies W_0_ix (ACF.py:150-170).  The step is the reference's DETACHED one: g'_u is
computed outside the tape and rebuilt as a new leaf (ACF.py:203-208), so autograd sees the scores as g'_u . Gi_i with g'_u a
constant and the attention tensors only through the regulariser.  Optimizers: sgd, and TF-2.3 Adam (the sparse-variable rule on
Gu / Gi / Pi, the dense ApplyAdam rule on the attention tensors), restated from tests/torch_ref.py's arithmetic in float64."""
import numpy as np
import torch

from fashionvisualexpl_recommend_amd._ffi import ACF_WEIGHTS

B1, B2, EPS = 0.9, 0.999, 1e-7
SPARSE = ("Gu", "Gi", "Pi")


class ACFRef:
    def __init__(self, tables, F, reg=0.0):
        """tables: Gu, Gi, Pi and the twelve ACF_WEIGHTS entries (numpy / torch); F: [I, M, C] feature maps."""
        self.p = {n: torch.as_tensor(np.asarray(tables[n], dtype=np.float64)).clone() for n in ("Gu", "Gi", "Pi") + tuple(ACF_WEIGHTS)}
        self.F = torch.as_tensor(np.asarray(F, dtype=np.float64))
        self.reg = reg
        self.slots = {}
        self.t = 0

    # ---- calculate_beta_alpha, ACF.py:135-181 ---------------------------------------------------------------------------
    def profile(self, u, hist, p=None):
        p = self.p if p is None else p
        g_u = p["Gu"][u]
        if len(hist) == 0:
            return g_u.clone()
        h = torch.as_tensor(list(hist), dtype=torch.long)
        f_i = self.F[h]                                                                   # [L, M, C]
        b = p["component.W_0_u"].T @ g_u + torch.tensordot(f_i, p["component.W_0_i"], dims=([2], [0])) + p["component.b_0"]
        b = torch.relu(b)
        b = torch.tensordot(b, p["component.W_1"], dims=([2], [1])) + p["component.b_1"]   # [L, M, 1]
        beta = torch.softmax(b.squeeze(-1), dim=1)
        x_l = (beta.unsqueeze(2) * f_i).sum(1)                                            # [L, C]
        g_i, p_i = p["Gi"][h], p["Pi"][h]
        a = (p["item.W_0_u"].T @ g_u + g_i @ p["item.W_0_iv"] + p_i @ p["item.W_0_ip"] + x_l @ p["item.W_0_ix"]
             + p["item.b_0"])
        a = torch.relu(a) @ p["item.W_1"].T + p["item.b_1"]
        alpha = torch.softmax(a.reshape(-1), dim=0)
        return g_u + (alpha.unsqueeze(1) * p_i).sum(0)

    def profiles(self, users, lists):
        return torch.stack([self.profile(int(u), lists[int(u)]) for u in users])

    def call(self, users, items, lists):
        gp = self.profiles(users, lists)
        return (gp * self.p["Gi"][torch.as_tensor(items).long()]).sum(1)

    def predict_all(self, lists):
        return self.profiles(range(self.p["Gu"].shape[0]), lists) @ self.p["Gi"].T

    # ---- train_step, ACF.py:239-270 ---------------------------------------------------------------------------------------
    def grads(self, batch, lists):
        """(loss, {name: gradient}) of one step with the detached g'_u."""
        u, i, j = (torch.as_tensor(np.asarray(x)).long() for x in batch)
        with torch.no_grad():
            gp = self.profiles(u.tolist(), lists)                                         # new leaf (ACF.py:208)
        leaves = {n: v.clone().requires_grad_(True) for n, v in self.p.items()}
        xp = (gp * leaves["Gi"][i]).sum(1)
        xn = (gp * leaves["Gi"][j]).sum(1)
        res = torch.clamp(xp - xn, -80.0, 1e8)
        loss = torch.nn.functional.softplus(-res).sum()
        reg = sum((leaves[n] ** 2).sum() for n in ACF_WEIGHTS)
        reg = reg + (leaves["Gu"][u] ** 2).sum() + (leaves["Gi"][i] ** 2).sum() + (leaves["Gi"][j] ** 2).sum() \
            + (leaves["Pi"][i] ** 2).sum() + (leaves["Pi"][j] ** 2).sum()
        loss = loss + self.reg * reg
        g = torch.autograd.grad(loss, list(leaves.values()), allow_unused=True)
        return loss.item(), {n: (torch.zeros_like(self.p[n]) if gr is None else gr) for n, gr in zip(leaves, g)}

    def step(self, batch, lists, optimizer="sgd", lr=0.01):
        loss, g = self.grads(batch, lists)
        self.t += 1
        if optimizer == "sgd":
            for n in self.p:
                self.p[n] = self.p[n] - lr * g[n]
            return loss
        lr_t = lr * np.sqrt(1.0 - B2 ** self.t) / (1.0 - B1 ** self.t)
        for n in self.p:
            m, v = self.slots.get("m_" + n, torch.zeros_like(self.p[n])), self.slots.get("v_" + n, torch.zeros_like(self.p[n]))
            if n in SPARSE:
                m = m * B1 + g[n] * (1 - B1)
                v = v * B2 + g[n] * g[n] * (1 - B2)
            else:
                m = m + (g[n] - m) * (1 - B1)
                v = v + (g[n] * g[n] - v) * (1 - B2)
            self.slots["m_" + n], self.slots["v_" + n] = m, v
            self.p[n] = self.p[n] - lr_t * m / (torch.sqrt(v) + EPS)
        return loss


def random_tables(rs, U, I, k, C, h, a, scale=1.0):
    """Tables with the reference's initialiser magnitudes (Glorot attention tensors, Pi ~ N(0, 0.01)); `scale` widens Pi."""
    from fashionvisualexpl_recommend_amd.synth import glorot_uniform
    g1 = lambda n: rs.uniform(-np.sqrt(3.0 / n), np.sqrt(3.0 / n), size=n).astype(np.float32)
    t = {"Gu": glorot_uniform(rs, U, k), "Gi": glorot_uniform(rs, I, k), "Bi": np.zeros(I, np.float32),
         "Pi": (rs.normal(0, 0.01, size=(I, k)) * scale).astype(np.float32)}
    t.update({"component.W_0_u": glorot_uniform(rs, k, h), "component.W_0_i": glorot_uniform(rs, C, h), "component.b_0": g1(h),
              "component.W_1": glorot_uniform(rs, 1, h), "component.b_1": g1(1),
              "item.W_0_u": glorot_uniform(rs, k, a), "item.W_0_iv": glorot_uniform(rs, k, a), "item.W_0_ip": glorot_uniform(rs, k, a),
              "item.W_0_ix": glorot_uniform(rs, C, a), "item.b_0": g1(a), "item.W_1": glorot_uniform(rs, 1, a), "item.b_1": g1(1)})
    return t
