"""GradFashion restated literally in torch float64 on the CPU, differentiated by autograd: the checker of the GradFashion tests
(a helper module, not a test module).

Reference: src/recommender/models/GradFashion.py -- call :83-131, train_step :133-193, predict_all :305-320,
predict_ui_grads :269-292.  Optimizers: sgd, or TF-2.3 Adam with the DENSE ApplyAdam form for the dense tables Ec, Ee, E, Bp
and the non-lazy sparse (IndexedSlices) form for the row tables Gu, Gi, Bi, Tu; its bias-corrected lr_t is
tests/torch_ref.adam_lr_t.
"""
import numpy as np
import torch

from torch_ref import B1, B2, EPS, adam_lr_t

ROW = ("Gu", "Gi", "Bi", "Tu")
DENSE = ("Ec", "Ee", "E", "Bp")
PARAMS = ROW + DENSE


class GradFashionRef:
    """tables: Gu [U,k], Gi [I,k], Bi [I], Tu [U,d], Fc [I,Dc], Fe [I,De], Ec [Dc,ec], Ee [De,ee], E [ec+ee,d], Bp [ec+ee]
    (numpy or torch; Bp may be [ec+ee, 1] as in the reference)."""

    def __init__(self, tables, reg, dtype=torch.float64):
        """`dtype=torch.float32` runs the same restatement in float32: its deviation from float64 is one sample of float32 rounding."""
        self.dtype = dtype
        f = lambda x: torch.as_tensor(np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x), dtype=torch.float64).to(dtype).clone()
        self.p = {n: f(tables[n]) for n in PARAMS}
        self.p["Bp"] = self.p["Bp"].reshape(-1, 1)
        self.Fc, self.Fe = f(tables["Fc"]), f(tables["Fe"])
        self.reg = float(reg)
        self.m = {n: torch.zeros_like(v) for n, v in self.p.items()}
        self.v = {n: torch.zeros_like(v) for n, v in self.p.items()}
        self.t = 0

    def load(self, t, step):
        """Continue from an engine's state (`Engine.t` names: Ec, Ee, E, Bp and m_ / v_ slots) at Adam step `step`."""
        f = lambda x: x.detach().to("cpu", self.dtype).clone()
        for n in PARAMS:
            self.p[n] = f(t[n]).reshape(self.p[n].shape)
            if ("m_" + n) in t:
                self.m[n], self.v[n] = f(t["m_" + n]).reshape(self.p[n].shape), f(t["v_" + n]).reshape(self.p[n].shape)
        self.t = step
        return self

    def state(self):
        """Parameters and slots as float32-shaped float64 tensors under Engine.t names (Bp flat)."""
        out = {}
        for n in PARAMS:
            out[n] = self.p[n].reshape(-1) if n in ("Bp", "Bi") else self.p[n]
            out["m_" + n] = self.m[n].reshape(out[n].shape)
            out["v_" + n] = self.v[n].reshape(out[n].shape)
        return out

    def explain_scale(self, users, items):
        """sum_c |vf_c| |w_c| per part: the scale of the fp32 rounding of an attribution, [n, 2]."""
        p = self.p
        u, i = torch.as_tensor(users).long(), torch.as_tensor(items).long()
        ec = p["Ec"].shape[1]
        w = (p["Tu"][u].abs() @ p["E"].T.abs() + p["Bp"].reshape(1, -1).abs())
        c = ((self.Fc[i].abs() @ p["Ec"].abs()) * w[:, :ec]).sum(1)
        e = ((self.Fe[i].abs() @ p["Ee"].abs()) * w[:, ec:]).sum(1)
        return torch.stack([c, e], 1).numpy()

    # GradFashion.call (training=True), :83-131
    def call(self, user, item, p=None, color_i=None, edges_i=None):
        p = self.p if p is None else p
        user, item = torch.as_tensor(user).long(), torch.as_tensor(item).long()
        gamma_u, theta_u = p["Gu"][user], p["Tu"][user]
        gamma_i = p["Gi"][item]
        color_i = self.Fc[item] if color_i is None else color_i
        edges_i = self.Fe[item] if edges_i is None else edges_i
        visual_features_i = torch.cat([color_i @ p["Ec"], edges_i @ p["Ee"]], 1)
        theta_i = visual_features_i @ p["E"]
        beta_i = p["Bi"][item]
        xui = beta_i + (gamma_u * gamma_i).sum(1) + (theta_u * theta_i).sum(1) + (visual_features_i @ p["Bp"]).squeeze(1)
        return xui, gamma_u, gamma_i, color_i, edges_i, theta_u, theta_i, beta_i

    def predict_all(self):                                               # :305-320
        p = self.p
        visual_features_i = torch.cat([self.Fc @ p["Ec"], self.Fe @ p["Ee"]], 1)
        theta_i = visual_features_i @ p["E"]
        return p["Bi"] + p["Gu"] @ p["Gi"].T + p["Tu"] @ theta_i.T + (visual_features_i @ p["Bp"]).squeeze(1)

    def loss(self, user, pos, neg, p):                                   # :145-180
        l2 = lambda x: (x * x).sum() / 2                                 # tf.nn.l2_loss
        xu_pos, gamma_u, gamma_i_pos, _, _, theta_u, _, beta_pos = self.call(user, pos, p)
        xu_neg, _, gamma_i_neg, _, _, _, _, beta_neg = self.call(user, neg, p)
        result = torch.clamp(xu_pos - xu_neg, -80.0, 1e8)
        loss = torch.nn.functional.softplus(-result).sum()
        reg = self.reg
        reg_loss = reg * (l2(gamma_u) + l2(gamma_i_pos) + l2(gamma_i_neg) + l2(theta_u)) * 2 + \
            reg * (l2(beta_pos) + l2(beta_neg)) * 2 + \
            reg * (l2(p["Ec"]) + l2(p["Ee"]) + l2(p["E"]) + l2(p["Bp"])) * 2
        return loss + reg_loss

    def grads(self, user, pos, neg):
        """(loss, {table: gradient}) at the current parameters."""
        p = {n: v.clone().requires_grad_(True) for n, v in self.p.items()}
        loss = self.loss(user, pos, neg, p)
        g = torch.autograd.grad(loss, [p[n] for n in PARAMS])
        return float(loss.detach()), dict(zip(PARAMS, g))

    def train_step(self, user, pos, neg, optimizer="adam_tf23", lr=1e-3):
        """One step (:133-193); returns (loss, gradients)."""
        loss, g = self.grads(user, pos, neg)
        if optimizer == "sgd":
            for n in PARAMS:
                self.p[n] = self.p[n] - lr * g[n]
            return loss, g
        self.t += 1
        lr_t = adam_lr_t(lr, self.t)
        for n in PARAMS:
            m, v = self.m[n], self.v[n]
            if n in DENSE:                                               # ApplyAdam (dense)
                m = m + (g[n] - m) * (1 - B1)
                v = v + (g[n] * g[n] - v) * (1 - B2)
            else:                                                        # sparse apply, every row moves
                m = m * B1 + g[n] * (1 - B1)
                v = v * B2 + g[n] * g[n] * (1 - B2)
            self.m[n], self.v[n] = m, v
            self.p[n] = self.p[n] - lr_t * m / (torch.sqrt(v) + EPS)
        return loss, g

    def predict_ui_grads(self, u, i):
        """Gradient x input of the score with respect to Fc_i and Fe_i, each summed (:269-292): np [1, 2]."""
        color_i = self.Fc[i:i + 1].clone().requires_grad_(True)
        edges_i = self.Fe[i:i + 1].clone().requires_grad_(True)
        x = self.call([u], [i], color_i=color_i, edges_i=edges_i)[0].sum()
        gc, ge = torch.autograd.grad(x, [color_i, edges_i])
        return np.array([[float((gc * color_i).sum().detach()), float((ge * edges_i).sum().detach())]])

    def explain_closed_form(self, users, items):
        """The same attribution in closed form (exact for the linear score):
        colour = (Fc_i Ec).(E[:ec] Tu_u + Bp[:ec]), edges = (Fe_i Ee).(E[ec:] Tu_u + Bp[ec:]): [n, 2]."""
        p = self.p
        u, i = torch.as_tensor(users).long(), torch.as_tensor(items).long()
        ec = p["Ec"].shape[1]
        w = p["Tu"][u] @ p["E"].T + p["Bp"].reshape(1, -1)               # [n, ec+ee]
        c = ((self.Fc[i] @ p["Ec"]) * w[:, :ec]).sum(1)
        e = ((self.Fe[i] @ p["Ee"]) * w[:, ec:]).sum(1)
        return torch.stack([c, e], 1).numpy()

    def effective(self):
        """(E_eff [Dc+De, d], Bp_eff [Dc+De]) of the factored projection."""
        p = self.p
        ec = p["Ec"].shape[1]
        E = torch.cat([p["Ec"] @ p["E"][:ec], p["Ee"] @ p["E"][ec:]], 0)
        Bp = torch.cat([p["Ec"] @ p["Bp"][:ec], p["Ee"] @ p["Bp"][ec:]], 0).reshape(-1)
        return E, Bp
