"""Plain torch restatement of one train step, the checker of the full-size GPU tests (not a conftest, not a test module).

The oracle cannot run the bench's shapes in seconds, so these functions recompute the SAME step on the device in high
precision: the two VBPR projections with the HIP path's operand rounding (bf16 / e4m3 operands), fp32 matmuls, fp64
scatter sums for every row gradient.  Each `*_step` takes a state (dict of tensors, as `Engine.t` names them) and a batch
(u, i, j int32 device tensors) and returns (gradients, loss, new state); the new state holds the updated tables and, with
adam_tf23, their m / v slots.  Reference: BPRMF.py:87-125, VBPR.py:99-144; TF-2.3 Adam as oracle/bpr_oracle.c restates it.
"""
import ctypes
import ctypes.util

import torch

B1, B2, EPS = 0.9, 0.999, 1e-7
ROW_TABLES = ("Gu", "Gi", "Bi", "Tu")          # sparse (IndexedSlices) Adam, non-lazy: every row decays and moves each step
DENSE_TABLES = ("E", "Bp")                      # dense ApplyAdam form

_libm = ctypes.CDLL(ctypes.util.find_library("m"))
_libm.powf.restype = ctypes.c_float
_libm.powf.argtypes = [ctypes.c_float, ctypes.c_float]
_libm.sqrtf.restype = ctypes.c_float
_libm.sqrtf.argtypes = [ctypes.c_float]


def adam_lr_t(lr, t):
    """lr * sqrt(1 - b2^t) / (1 - b1^t) in fp32, operation by operation as the oracle computes it (adam.py _prepare_local)."""
    f = lambda x: ctypes.c_float(x).value
    tf = f(float(t))
    num = f(f(lr) * _libm.sqrtf(f(1.0 - _libm.powf(f(B2), tf))))
    return f(num / f(1.0 - _libm.powf(f(B1), tf)))


def scatter(n_rows, idx, vals):
    """fp64 row sums of vals [n, c] into [n_rows, c]."""
    out = torch.zeros((n_rows, vals.shape[1]), device=vals.device, dtype=torch.float64)
    return out.index_add_(0, idx, vals.double())


def vbpr_project(state, fp8):
    """(Eq, frow): the projection operand [D, d+1] with the HIP path's rounding, and the feature-row reader."""
    F = state["F"]
    EB = torch.cat([state["E"], state["Bp"][:, None]], 1)                                          # [D, d+1]
    if fp8:
        sE = torch.tensor(448.0, device=F.device) / EB.abs().max()                                # k_absmax / k_cast_Et8
        Eq = (EB * sE).to(torch.float8_e4m3fn).float() / sE
        frow = lambda idx: F[idx].float() / 448.0                                                  # codes of f * 448
    else:
        Eq = EB.to(torch.bfloat16).float()
        frow = lambda idx: F[idx].float()
    return Eq, frow


def vbpr_forward(state, batch, fp8):
    """The step's forward pass: x+ and x- of every triplet and the projected rows it reads."""
    u, i, j = (x.long() for x in batch)
    d = state["Tu"].shape[1]
    I = state["Gi"].shape[0]
    Eq, frow = vbpr_project(state, fp8)
    touched = torch.unique(torch.cat([i, j]))
    Pt = torch.cat([frow(touched[s0:s0 + 8192]) @ Eq for s0 in range(0, touched.numel(), 8192)])  # [nT, d+1]
    slot = torch.full((I,), -1, device=Eq.device, dtype=torch.long)
    slot[touched] = torch.arange(touched.numel(), device=Eq.device)
    Pi, Pj = Pt[slot[i]], Pt[slot[j]]
    gu, tu, gi, gj = state["Gu"][u], state["Tu"][u], state["Gi"][i], state["Gi"][j]
    xp = state["Bi"][i] + (gu * gi).sum(1) + (tu * Pi[:, :d]).sum(1) + Pi[:, d]
    xn = state["Bi"][j] + (gu * gj).sum(1) + (tu * Pj[:, :d]).sum(1) + Pj[:, d]
    return dict(Eq=Eq, frow=frow, Pi=Pi, Pj=Pj, xp=xp, xn=xn)


def _abs_sums(absg, parts):
    """absg[name] = sum over the triplets of |each term| of the gradient: the scale of its fp32 summation noise."""
    for name, rows, idx_terms in parts:
        acc = torch.zeros((rows, idx_terms[0][1].shape[1]), device=idx_terms[0][1].device, dtype=torch.float64)
        for idx, terms in idx_terms:
            acc.index_add_(0, idx, terms.double().abs())
        absg[name] = acc


def vbpr_grads(state, batch, reg, fp8, fwd=None, absg=None):
    """(gradients, loss) of one VBPR step.  Row gradients fp64 [rows, c] (Bi: [I, 1]); E, Bp fp32.  absg (a dict): also
    the sums of the absolute terms of every gradient element, the scale of its summation noise."""
    fwd = vbpr_forward(state, batch, fp8) if fwd is None else fwd
    u, i, j = (x.long() for x in batch)
    U, d = state["Tu"].shape
    I = state["Gi"].shape[0]
    D = state["E"].shape[0]
    Pi, Pj, frow = fwd["Pi"], fwd["Pj"], fwd["frow"]
    gu, tu, gi, gj = state["Gu"][u], state["Tu"][u], state["Gi"][i], state["Gi"][j]
    diff = fwd["xp"] - fwd["xn"]
    gg = -torch.sigmoid(-diff)
    loss = torch.nn.functional.softplus(-diff).double().sum() + reg * (
        (gu.double() ** 2).sum() + (gi.double() ** 2).sum() + (gj.double() ** 2).sum() + (tu.double() ** 2).sum()
        + (state["Bi"][i].double() ** 2).sum() + (state["Bi"][j].double() ** 2).sum() / 10
        + (state["E"].double() ** 2).sum() + (state["Bp"].double() ** 2).sum())
    g = {"Gu": scatter(U, u, gg[:, None] * (gi - gj) + 2 * reg * gu),
         "Tu": scatter(U, u, gg[:, None] * (Pi[:, :d] - Pj[:, :d]) + 2 * reg * tu),
         "Gi": scatter(I, i, gg[:, None] * gu + 2 * reg * gi) + scatter(I, j, -gg[:, None] * gu + 2 * reg * gj),
         "Bi": scatter(I, i, (gg + 2 * reg * state["Bi"][i])[:, None]) +
         scatter(I, j, (-gg + 0.2 * reg * state["Bi"][j])[:, None])}
    if absg is not None:
        _abs_sums(absg, [
            ("Gu", U, [(u, gg[:, None] * gi), (u, gg[:, None] * gj), (u, 2 * reg * gu)]),
            ("Tu", U, [(u, gg[:, None] * Pi[:, :d]), (u, gg[:, None] * Pj[:, :d]), (u, 2 * reg * tu)]),
            ("Gi", I, [(i, gg[:, None] * gu), (i, 2 * reg * gi), (j, gg[:, None] * gu), (j, 2 * reg * gj)]),
            ("Bi", I, [(i, gg[:, None]), (i, 2 * reg * state["Bi"][i][:, None]), (j, gg[:, None]),
                       (j, 0.2 * reg * state["Bi"][j][:, None])])])
    gth = torch.cat([gg[:, None] * tu, gg[:, None]], 1)
    W = (scatter(I, i, gth) - scatter(I, j, gth)).float().to(torch.bfloat16).float()              # bf16 like the MFMA operand
    del gth
    dEq = torch.zeros((D, d + 1), device=W.device, dtype=torch.float32)
    aEq = torch.zeros_like(dEq) if absg is not None else None
    for s0 in range(0, I, 8192):                                                                   # F^T W in fp32 chunks
        Fc = frow(torch.arange(s0, min(I, s0 + 8192), device=W.device))
        dEq += Fc.T @ W[s0:s0 + 8192]
        if aEq is not None:
            aEq += Fc.abs().T @ W[s0:s0 + 8192].abs()
    g["E"] = dEq[:, :d] + 2 * reg * state["E"]
    g["Bp"] = dEq[:, d] + 2 * reg * state["Bp"]
    if absg is not None:
        absg["E"] = aEq[:, :d] + (2 * reg * state["E"]).abs()
        absg["Bp"] = aEq[:, d] + (2 * reg * state["Bp"]).abs()
    return g, loss


def bprmf_grads(state, batch, reg, absg=None):
    """(gradients, loss) of one BPRMF step; row gradients fp64 [rows, c] (Bi: [I, 1]); absg as in vbpr_grads."""
    u, i, j = (x.long() for x in batch)
    U, I = state["Gu"].shape[0], state["Gi"].shape[0]
    gu, gi, gj = state["Gu"][u], state["Gi"][i], state["Gi"][j]
    diff = (state["Bi"][i] + (gu * gi).sum(1)) - (state["Bi"][j] + (gu * gj).sum(1))
    gg = -torch.sigmoid(-diff)
    loss = torch.nn.functional.softplus(-diff).double().sum() + reg * (
        (gu.double() ** 2).sum() + (gi.double() ** 2).sum() + (gj.double() ** 2).sum()
        + (state["Bi"][i].double() ** 2).sum() + (state["Bi"][j].double() ** 2).sum() / 10)
    g = {"Gu": scatter(U, u, gg[:, None] * (gi - gj) + 2 * reg * gu),
         "Gi": scatter(I, i, gg[:, None] * gu + 2 * reg * gi) + scatter(I, j, -gg[:, None] * gu + 2 * reg * gj),
         "Bi": scatter(I, i, (gg + 2 * reg * state["Bi"][i])[:, None]) +
         scatter(I, j, (-gg + 0.2 * reg * state["Bi"][j])[:, None])}
    if absg is not None:
        _abs_sums(absg, [
            ("Gu", U, [(u, gg[:, None] * gi), (u, gg[:, None] * gj), (u, 2 * reg * gu)]),
            ("Gi", I, [(i, gg[:, None] * gu), (i, 2 * reg * gi), (j, gg[:, None] * gu), (j, 2 * reg * gj)]),
            ("Bi", I, [(i, gg[:, None]), (i, 2 * reg * state["Bi"][i][:, None]), (j, gg[:, None]),
                       (j, 0.2 * reg * state["Bi"][j][:, None])])])
    return g, loss


def sgd(state, grads, lr):
    new = dict(state)
    for n, g in grads.items():
        new[n] = state[n] - lr * g.float().reshape(state[n].shape)
    return new


def adam_tf23(state, grads, lr, t):
    """Step t (1-based) of TF-2.3 Adam from the m_* / v_* slots in `state`; every table of `grads` moves, touched or not."""
    lr_t = adam_lr_t(lr, t)
    f = lambda x: ctypes.c_float(x).value
    omb1, omb2 = f(1.0 - f(B1)), f(1.0 - f(B2))                                   # 1.0f - b1, 1.0f - b2 in fp32
    new = dict(state)
    for n, g in grads.items():
        p, m, v = state[n], state["m_" + n], state["v_" + n]
        g = g.float().reshape(p.shape)
        if n in DENSE_TABLES:
            mt = m + (g - m) * omb1
            vt = v + (g * g - v) * omb2
        else:
            mt = m * f(B1) + g * omb1
            vt = v * f(B2) + (g * g) * omb2
        new[n], new["m_" + n], new["v_" + n] = p - lr_t * mt / (torch.sqrt(vt) + EPS), mt, vt
    return new


def _apply(state, grads, optimizer, lr, t):
    return sgd(state, grads, lr) if optimizer == "sgd" else adam_tf23(state, grads, lr, t)


def vbpr_step(state, batch, lr, reg, fp8=False, optimizer="sgd", t=1, absg=None):
    grads, loss = vbpr_grads(state, batch, reg, fp8, absg=absg)
    return grads, loss, _apply(state, grads, optimizer, lr, t)


def bprmf_step(state, batch, lr, reg, optimizer="sgd", t=1, absg=None):
    grads, loss = bprmf_grads(state, batch, reg, absg=absg)
    return grads, loss, _apply(state, grads, optimizer, lr, t)


def assert_adam_close(got, want, grads, absg, lr, noise, max_outlier_frac, tag=""):
    """Tables and slots of an Adam step against the restatement.  Elementwise |got - want| <= 2e-3 lr on the tables; the
    only exceptions allowed are elements whose reference gradient is within `noise` x its absolute-term sum of cancelling
    (from zero slots Adam turns any such noise into a full +-lr move), and at most max_outlier_frac of a table's elements.
    m / v: the gradient noise carried through (1 - b1) and (1 - b2).  Returns {table: outliers}."""
    counts = {}
    for n, g in grads.items():
        g = g.float().reshape(want[n].shape)
        tol_g = (noise[n] if isinstance(noise, dict) else noise) * absg[n].float().reshape(want[n].shape) + 1e-12
        err = (got[n] - want[n]).abs()
        bad = err > 2e-3 * lr
        near = g.abs() <= tol_g
        assert not bool((bad & ~near).any()), "%s %s: %d elements off by up to %g (lr %g) with a clear gradient" % (
            tag, n, int((bad & ~near).sum()), float(err[bad & ~near].max()), lr)
        counts[n] = int(bad.sum())
        assert counts[n] <= max_outlier_frac * bad.numel(), (tag, n, counts[n], bad.numel())
        m_err = (got["m_" + n] - want["m_" + n]).abs()
        assert bool((m_err <= 0.1 * tol_g + 1e-5 * want["m_" + n].abs() + 1e-12).all()), (tag, "m_" + n, float(m_err.max()))
        v_err = (got["v_" + n] - want["v_" + n]).abs()
        v_tol = 1e-3 * (2 * g.abs() * tol_g + tol_g * tol_g) + 1e-5 * want["v_" + n].abs() + 1e-20
        assert bool((v_err <= v_tol).all()), (tag, "v_" + n, float(v_err.max()))
    return counts
