"""Engine: one libbprx handle + the torch-ROCm tensors it is bound to.

PyTorch is plumbing here (device memory, streams); every computation of the hot path runs in
libbprx.so through the C ABI (include/bprx.h).  A missing library or a missing GPU raises.
"""
import ctypes as C
import weakref

import numpy as np
import torch

from . import _ffi
from .ranking import lists_to_csr

PARAM_NAMES = ("Gu", "Gi", "Bi", "Tu", "E", "Bp")
FACTORED_PARAM_NAMES = ("Gu", "Gi", "Bi", "Tu", "Ec", "Ee", "E", "Bp")     # GradFashion.py:182-186 (bind_factored)


def _ptr(t):
    """NULL for None or an empty tensor, else the tensor's address."""
    return None if (t is None or t.numel() == 0) else C.c_void_p(t.data_ptr())


def _addr(t):
    """NULL for None, else the tensor's address: an empty tensor still reaches the library's own argument checks."""
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def as_index(x, device):
    """int64/any index array -> contiguous int32 device tensor (reference batches are int64, dataset.py:105-107)."""
    if isinstance(x, torch.Tensor):
        t = x.reshape(-1)
        if t.dtype != torch.int32:
            t = t.to(torch.int32)
        return t.to(device, non_blocking=True).contiguous()
    return torch.as_tensor(np.ascontiguousarray(np.asarray(x).reshape(-1), dtype=np.int32), device=device)


class _Bound(dict):
    """The bound tensors by name.  A step may leave its dense E|Bp update to the next step (Engine.settle); every way of getting
    at a tensor through this dict first settles it (a host call that returns at once when nothing is pending): d[name], get,
    items, values, iteration, keys, copy and dict(d).  `name in d` and len(d) touch no tensor and do not.  The engine is held by
    a weak reference: the dict keeps no engine alive, and after the engine is gone it is a plain dict."""

    def __init__(self, engine, tensors):
        super().__init__(tensors)
        self._engine = weakref.ref(engine)

    def _settle(self):
        e = self._engine()
        if e is not None:
            e.settle()

    def __getitem__(self, name):
        self._settle()
        return dict.__getitem__(self, name)

    def get(self, name, default=None):
        self._settle()
        return dict.get(self, name, default)

    def items(self):
        self._settle()
        return dict.items(self)

    def values(self):
        self._settle()
        return dict.values(self)

    def keys(self):
        self._settle()
        return dict.keys(self)

    def __iter__(self):
        self._settle()
        return dict.__iter__(self)

    def copy(self):
        self._settle()
        return dict(dict.items(self))


class Engine:
    def __init__(self, model, num_users, num_items, embed_k, embed_d=0, feat_dim=0, feat_dtype="fp32",
                 optimizer="adam_tf23", lr=1e-3, reg=0.0, max_batch=256, device=None,
                 beta1=0.9, beta2=0.999, epsilon=1e-7, export_user_grad=False, export_item_grad=False, feat_scale=448.0,
                 dense_allreduce=False, adam_form=None):
        if not torch.cuda.is_available():
            raise RuntimeError("fashionvisualexpl_recommend_amd needs a ROCm GPU (MI355X); there is no CPU fallback")
        self.lib = _ffi.lib()
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        self.model, self.optimizer = model, optimizer
        self.U, self.I, self.k = int(num_users), int(num_items), int(embed_k)
        self.d, self.D = (int(embed_d), int(feat_dim)) if model == "vbpr" else (0, 0)
        self.feat_dtype = feat_dtype
        self.feat_scale = float(feat_scale)
        self.max_batch = int(max_batch)
        self._lr_reg = (float(lr), float(reg))               # what fold_in falls back on (set_hyper keeps it current)
        cfg = _ffi.Config(_ffi.ABI_VERSION, _ffi.MODEL[model], self.U, self.I, self.k, self.d, self.D,
                          _ffi.FEAT_DTYPE[feat_dtype], _ffi.OPTIMIZER[optimizer], self.device.index, self.max_batch,
                          lr, reg, beta1, beta2, epsilon,
                          (_ffi.FLAG_EXPORT_USER_GRAD if export_user_grad else 0) |
                          (_ffi.FLAG_EXPORT_ITEM_GRAD if export_item_grad else 0) |
                          (_ffi.FLAG_DENSE_ALLREDUCE if dense_allreduce else 0) |
                          {None: 0, "sweep": _ffi.FLAG_ADAM_SWEEP, "lazy": _ffi.FLAG_ADAM_LAZY}[adam_form], self.feat_scale)
        h = C.c_void_p()
        _ffi.check(None, self.lib.bprx_create(C.byref(cfg), C.byref(h)))
        self.h = h
        self._t = {}
        self._loss = torch.zeros(1, dtype=torch.float32, device=self.device)

    @property
    def t(self):
        """The bound tensors.  adam_tf23 is lazy-exact inside the library: reading the tensors from outside first brings
        every row up to date (bprx_sync_adam; a host call that returns at once when nothing is pending)."""
        if getattr(self, "h", None) and self._t:
            self.settle()
            if self.optimizer == "adam_tf23":
                self.sync_adam()
        return self._t                                       # (a _Bound: a later look-up settles again)

    @t.setter
    def t(self, v):
        self._t = _Bound(self, v)

    def adam_is_lazy(self):
        return bool(self.lib.bprx_adam_is_lazy(self.h))

    def sync_adam(self):
        _ffi.check(self.h, self.lib.bprx_sync_adam(self.h, _stream()))

    def settle(self):
        """bprx_settle: a step(want_loss=False) may leave its dense E|Bp update to the next step's index pass; before E / Bp are
        read from outside the library it runs now (a host call that returns at once when nothing is pending)."""
        if getattr(self, "h", None) and hasattr(self.lib, "bprx_settle"):
            _ffi.check(self.h, self.lib.bprx_settle(self.h, _stream()))

    def dense_pending(self):
        return bool(self.lib.bprx_dense_pending(self.h)) if hasattr(self.lib, "bprx_dense_pending") else False

    def set_loss_lag(self, on):
        """bprx_set_loss_lag: steps given loss_out may defer their dense update too; a step's loss then lands in loss_out when the
        NEXT step (or settle()) is enqueued -- for loops that read their loss buffer once per epoch, after settle().  The buffer
        must outlive the lag: turn it off (which settles first) before the buffer goes, in a finally clause."""
        if not on:
            self.settle()                                    # a lagging loss lands now, while its buffer is still the caller's
        if getattr(self, "h", None) and hasattr(self.lib, "bprx_set_loss_lag"):
            _ffi.check(self.h, self.lib.bprx_set_loss_lag(self.h, 1 if on else 0))

    def close(self):
        if getattr(self, "h", None):
            self.lib.bprx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- state -------------------------------------------------------------------------------------------------
    def bind(self, Gu, Gi, Bi, Tu=None, F=None, E=None, Bp=None, slots=None):
        """Bind caller-owned device tensors (fp32, contiguous; F fp32 or bf16).  Adam slots are created here
        (zeros, like tf.optimizers.Adam's m/v) unless given."""
        def prep(x, shape, dtype=torch.float32):
            if x is None:
                return None
            x = torch.as_tensor(x)
            x = x.to(device=self.device, dtype=dtype).reshape(shape).contiguous()
            return x
        t = {"Gu": prep(Gu, (self.U, self.k)), "Gi": prep(Gi, (self.I, self.k)), "Bi": prep(Bi, (self.I,))}
        if self.model == "vbpr":
            if self.feat_dtype == "fp8":
                # e4m3fn codes of f * feat_scale (a float8 tensor is taken as is; anything else is quantised here,
                # round-to-nearest-even, on the device)
                Ft = torch.as_tensor(F)
                if Ft.dtype != torch.float8_e4m3fn:
                    Ft = (Ft.to(device=self.device, dtype=torch.float32) * self.feat_scale).to(torch.float8_e4m3fn)
                Fp = Ft.to(self.device).reshape(self.I, self.D).contiguous()
            else:
                Fp = prep(F, (self.I, self.D), torch.bfloat16 if self.feat_dtype == "bf16" else torch.float32)
            t.update(Tu=prep(Tu, (self.U, self.d)), F=Fp, E=prep(E, (self.D, self.d)), Bp=prep(Bp, (self.D,)))
        if self.optimizer == "adam_tf23":
            for n in PARAM_NAMES:
                if t.get(n) is None:
                    continue
                for s in ("m_", "v_"):
                    given = None if slots is None else slots.get(s + n)
                    t[s + n] = torch.zeros_like(t[n]) if given is None else prep(given, tuple(t[n].shape))
        tb = _ffi.Tables()
        for n in _ffi.TABLE_FIELDS:
            setattr(tb, n, None if t.get(n) is None else t[n].data_ptr())
        torch.cuda.current_stream(self.device).synchronize()   # bind tiles F on the null stream: the tables must be complete
        _ffi.check(self.h, self.lib.bprx_bind_tables(self.h, C.byref(tb)))
        self.t = t
        return self

    def bind_factored(self, Gu, Gi, Bi, Tu, F, Ec, Ee, E, Bp, feat_dim_a, feat_dim_b, neg_bias_reg=1.0, slots=None):
        """GradFashion (bprx_bind_factored): the handle trains the factor tables Ec [Dc,ec], Ee [De,ee], E [ec+ee,d],
        Bp [ec+ee] (GradFashion.py:59-81); F = [Fc | Fe | zero padding] is [I, feat_dim].  The handle's own E / Bp are the
        EFFECTIVE projection E_eff [D,d] / Bp_eff [D], library-written buffers kept here as t['E_eff'] / t['Bp_eff'].
        fp32 or bf16 features.  Adam slots (m_ / v_ for Gu, Gi, Bi, Tu, Ec, Ee, E, Bp) are zeros unless given."""
        if self.model != "vbpr":
            raise ValueError("bind_factored needs an Engine(model='vbpr', ...)")
        def prep(x, shape, dtype=torch.float32):
            return torch.as_tensor(x).to(device=self.device, dtype=dtype).reshape(shape).contiguous()
        Ec, Ee = torch.as_tensor(Ec), torch.as_tensor(Ee)
        ea, eb = int(Ec.shape[1]), int(Ee.shape[1])
        t = {"Gu": prep(Gu, (self.U, self.k)), "Gi": prep(Gi, (self.I, self.k)), "Bi": prep(Bi, (self.I,)),
             "Tu": prep(Tu, (self.U, self.d)),
             "F": prep(F, (self.I, self.D), torch.bfloat16 if self.feat_dtype == "bf16" else torch.float32),
             "Ec": prep(Ec, (feat_dim_a, ea)), "Ee": prep(Ee, (feat_dim_b, eb)),
             "E": prep(E, (ea + eb, self.d)), "Bp": prep(Bp, (ea + eb,)),
             "E_eff": torch.zeros((self.D, self.d), dtype=torch.float32, device=self.device),
             "Bp_eff": torch.zeros(self.D, dtype=torch.float32, device=self.device)}
        if self.optimizer == "adam_tf23":
            for n in FACTORED_PARAM_NAMES:
                for s_ in ("m_", "v_"):
                    given = None if slots is None else slots.get(s_ + n)
                    t[s_ + n] = torch.zeros_like(t[n]) if given is None else prep(given, tuple(t[n].shape))
        tb = _ffi.Tables()
        for n in _ffi.TABLE_FIELDS:
            v = {"E": t["E_eff"], "Bp": t["Bp_eff"]}.get(n) if n in ("E", "Bp", "m_E", "v_E", "m_Bp", "v_Bp") else t.get(n)
            setattr(tb, n, None if v is None else v.data_ptr())
        fx = _ffi.Factored(int(feat_dim_a), int(feat_dim_b), ea, eb, float(neg_bias_reg))
        for n, name in zip(_ffi.FACTORED_FIELDS, ("Ec", "Ee", "E", "Bp", "m_Ec", "v_Ec", "m_Ee", "v_Ee", "m_E", "v_E", "m_Bp", "v_Bp")):
            setattr(fx, n, None if t.get(name) is None else t[name].data_ptr())
        torch.cuda.current_stream(self.device).synchronize()
        _ffi.check(self.h, self.lib.bprx_bind_factored(self.h, C.byref(tb), C.byref(fx)))
        self.factored = True
        self.t = t
        return self

    def csr(self, lists):
        """Python lists of item ids per user -> (int64 indptr [n+1], int32 items) device tensors (ranking.lists_to_csr: items is
        never empty)."""
        return lists_to_csr(lists, self.device)

    def bind_acf(self, Gu, Gi, Bi, F, Pi, weights, train_lists, eval_lists=None, slots=None, gradient="detached"):
        """ACF (bprx_bind_acf) on a BPRMF engine: F [I, M, C] feature maps (fp32, or bf16 with feat_dtype='bf16'), Pi [I, k],
        weights = the twelve attention tensors as {'component.W_0_u': array, ..., 'item.b_1': array} (_ffi.ACF_WEIGHTS, shapes of
        include/bprx.h),
        train_lists / eval_lists = the histories P(u) of steps / score_pairs and of score_block (None: the training lists).
        Adam slots (m_ / v_ for Gu, Gi, Bi, Pi and every weight, keyed 'm_Pi', 'm_item.W_1', ...) are zeros unless given.
        gradient: 'detached' (the reference's step: g'_u is a constant of the tape) or 'full' (the same loss differentiated through
        both attention levels, bprx_acf_set_gradient)."""
        if self.model != "bprmf":
            raise ValueError("bind_acf needs an Engine(model='bprmf', ...)")
        if gradient not in _ffi.ACF_GRADIENT:
            raise ValueError("ACF gradient is 'detached' or 'full' (got %r)" % (gradient,))
        if self.feat_dtype not in ("fp32", "bf16"):
            raise ValueError("ACF features are fp32 or bf16 (got %s)" % self.feat_dtype)
        def prep(x, shape=None, dtype=torch.float32):
            x = torch.as_tensor(x).to(device=self.device, dtype=dtype)
            return (x.reshape(shape) if shape is not None else x).contiguous()
        Ft = prep(F, None, torch.bfloat16 if self.feat_dtype == "bf16" else torch.float32)
        if Ft.dim() != 3 or Ft.shape[0] != self.I:
            raise ValueError("F must be [num_items, M, C], got %s" % (tuple(Ft.shape),))
        M, Cf = int(Ft.shape[1]), int(Ft.shape[2])
        t = {"Gu": prep(Gu, (self.U, self.k)), "Gi": prep(Gi, (self.I, self.k)), "Bi": prep(Bi, (self.I,)),
             "Pi": prep(Pi, (self.I, self.k))}
        for key in _ffi.ACF_WEIGHTS:
            t[key] = prep(weights[key])
        hc, ha = int(t["component.W_0_u"].shape[1]), int(t["item.W_0_u"].shape[1])
        if self.optimizer == "adam_tf23":
            for n in ["Gu", "Gi", "Bi", "Pi"] + list(_ffi.ACF_WEIGHTS):
                for s_ in ("m_", "v_"):
                    key = s_ + n
                    given = None if slots is None else slots.get(key)
                    t[key] = torch.zeros_like(t[n]) if given is None else prep(given, tuple(t[n].shape))
        self.acf_train = self.csr(train_lists)
        self.acf_eval = self.csr(eval_lists) if eval_lists is not None else None
        self.acf_F = Ft
        tb = _ffi.Tables()
        for n in _ffi.TABLE_FIELDS:
            setattr(tb, n, None if t.get(n) is None else t[n].data_ptr())
        ac = _ffi.Acf(M, Cf, hc, ha, _ffi.FEAT_DTYPE[self.feat_dtype], Ft.data_ptr(), self.acf_train[0].data_ptr(),
                      self.acf_train[1].data_ptr(),
                      None if self.acf_eval is None else self.acf_eval[0].data_ptr(),
                      None if self.acf_eval is None else self.acf_eval[1].data_ptr(),
                      t["Pi"].data_ptr(), None if t.get("m_Pi") is None else t["m_Pi"].data_ptr(),
                      None if t.get("v_Pi") is None else t["v_Pi"].data_ptr())
        for q, key in enumerate(_ffi.ACF_WEIGHTS):
            ac.w[q] = t[key].data_ptr()
            if self.optimizer == "adam_tf23":
                ac.m_w[q], ac.v_w[q] = t["m_" + key].data_ptr(), t["v_" + key].data_ptr()
        torch.cuda.current_stream(self.device).synchronize()
        _ffi.check(self.h, self.lib.bprx_bind_acf(self.h, C.byref(tb), C.byref(ac)))
        self.acf = True
        self.t = t
        if gradient != "detached":
            self.acf_set_gradient(gradient)
        return self

    def acf_set_gradient(self, gradient):
        """bprx_acf_set_gradient: 'detached' or 'full' for the following steps of an ACF-bound engine."""
        if gradient not in _ffi.ACF_GRADIENT:
            raise ValueError("ACF gradient is 'detached' or 'full' (got %r)" % (gradient,))
        _ffi.check(self.h, self.lib.bprx_acf_set_gradient(self.h, _ffi.ACF_GRADIENT[gradient]))

    def acf_gradient(self):
        mode = _ffi.check(self.h, self.lib.bprx_acf_get_gradient(self.h))
        return {v: n for n, v in _ffi.ACF_GRADIENT.items()}[mode]

    def acf_profiles(self, users, lists=None, csr=None):
        """calculate_beta_alpha (bprx_acf_profiles): g'_u [n, k] for `users` with the histories `lists` (per user id, or a
        prebuilt `csr`; default: the bound training histories)."""
        u = as_index(users, self.device)
        ptr, items = csr if csr is not None else (self.csr(lists) if lists is not None else self.acf_train)
        out = torch.empty((u.numel(), self.k), dtype=torch.float32, device=self.device)
        _ffi.check(self.h, self.lib.bprx_acf_profiles(self.h, _ptr(u), u.numel(), _ptr(ptr), _ptr(items), _ptr(out), _stream()))
        return out

    def acf_explain(self, users, items, top=5, lists=None, csr=None, maps=False):
        """bprx_acf_explain: why the pairs (users[p], items[p]) score what they score.  x_ui = base + sum_l c_l over the user's
        history (`lists` per user id, or a prebuilt `csr`; default: the bound training histories), c_l = alpha_l (Pi_l . Gi_i).
        Returns a dict of device tensors: score, base [n]; pos, hist_item, alpha, contrib, peak, beta_peak [n, top] for the `top`
        entries with the largest c_l (non-increasing; slots beyond the history: -1 in the int fields, 0 in the float ones); with
        maps=True also beta [n, top, M], the component attention of every returned entry."""
        u, i = as_index(users, self.device), as_index(items, self.device)
        if u.numel() != i.numel():
            raise ValueError("acf_explain: %d users for %d items" % (u.numel(), i.numel()))
        ptr, hist = csr if csr is not None else (self.csr(lists) if lists is not None else getattr(self, "acf_train", None)
                                                 or self.csr([[]] * self.U))
        n, top = u.numel(), int(top)
        shape = (n, max(top, 0))
        f = lambda *s: torch.empty(s, dtype=torch.float32, device=self.device)
        g = lambda *s: torch.empty(s, dtype=torch.int32, device=self.device)
        out = {"score": f(n), "base": f(n), "pos": g(*shape), "hist_item": g(*shape), "alpha": f(*shape), "contrib": f(*shape),
               "peak": g(*shape), "beta_peak": f(*shape)}
        if maps:
            out["beta"] = f(n, max(top, 0), int(self.acf_F.shape[1]) if getattr(self, "acf", False) else 1)
        _ffi.check(self.h, self.lib.bprx_acf_explain(self.h, _addr(u), _addr(i), n, _addr(ptr), _addr(hist), top,
                                                     *(_addr(out[name]) for name in ("score", "base", "pos", "hist_item", "alpha",
                                                                                     "contrib", "peak", "beta_peak")),
                                                     _addr(out["beta"]) if maps else None, _stream()))
        return out

    def _acf_rows(self, what, Gu_rows, lists, csr):
        """(hist_ptr, hist_items, n) of a caller-owned table Gu_rows [n, k] and its histories by row."""
        ptr, items = csr if csr is not None else self.csr(lists)
        n = int(ptr.numel()) - 1
        self._check_rows(what, n, ("Gu_rows", Gu_rows, self.k))
        return ptr, items, n

    def _check_rows(self, what, n, *rows):
        """Each (name, tensor, width) of `rows` is a caller-owned row table [n, width] the library may write: ValueError unless it
        is a contiguous fp32 device tensor of that shape (None: the model has no such table)."""
        for name, t, w in rows:
            if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (n, w)):
                raise ValueError("%s: %s must be a contiguous fp32 device tensor [%d, %d]" % (what, name, n, w))

    def _fold_in(self, what, entry, lead, pair_ptr, pos, neg, steps, rows, lr, reg, optimizer, want_loss, hist_rows=None):
        """The body of fold_in / acf_fold_in / af_fold_in (`what`, for the messages): entry(h, *lead, pair_ptr, pos, neg, n, steps,
        lr, reg, optimizer, *row tables, loss, stream) after the checks they share.  rows: the (name, tensor, width) row tables as
        _check_rows takes them; hist_rows: the rows the histories behind `lead` were given for."""
        ptr = torch.as_tensor(pair_ptr, dtype=torch.int64).to(self.device).contiguous()
        n = int(ptr.numel()) - 1
        if hist_rows is not None and n != hist_rows:
            raise ValueError("%s: pair_ptr for %d rows, histories for %d" % (what, n, hist_rows))
        p_, n_ = as_index(pos, self.device), as_index(neg, self.device)
        if p_.numel() != n_.numel():
            raise ValueError("%s: %d positives for %d negatives" % (what, p_.numel(), n_.numel()))
        self._check_rows(what, n, *rows)
        lr = self._hyper()[0] if lr is None else float(lr)
        reg = self._hyper()[1] if reg is None else float(reg)
        opt = _ffi.OPTIMIZER[self.optimizer if optimizer is None else optimizer]
        loss = torch.empty(max(n, 0), dtype=torch.float32, device=self.device) if want_loss else None
        if p_.numel() == 0:                                  # (nobody has a pair: the library still wants the pointers)
            p_ = n_ = torch.zeros(1, dtype=torch.int32, device=self.device)
        _ffi.check(self.h, entry(self.h, *lead, _addr(ptr), _addr(p_), _addr(n_), n, int(steps), lr, reg, opt,
                                 *(_addr(t) for _, t, _ in rows), _addr(loss), _stream()))
        return loss

    def _fold_in_items(self, what, pair_ptr, user, other, role, n, lr, reg, optimizer, want_loss, call):
        """The body of fold_in_items / af_fold_in_items (`what`, for the messages) for n checked item rows: (loss, what
        call(ptr, user, other, role: addresses, pairs given, lr, reg, optimizer: resolved, loss: fp32 [n] or None) returned)."""
        ptr = torch.as_tensor(pair_ptr, dtype=torch.int64).to(self.device).contiguous()
        if int(ptr.numel()) - 1 != n:
            raise ValueError("%s: pair_ptr for %d items, rows for %d" % (what, int(ptr.numel()) - 1, n))
        u_, o_, r_ = (as_index(x, self.device) for x in (user, other, role))
        if not u_.numel() == o_.numel() == r_.numel():
            raise ValueError("%s: %d users, %d items, %d roles" % (what, u_.numel(), o_.numel(), r_.numel()))
        pairs = int(u_.numel())
        lr = self._hyper()[0] if lr is None else float(lr)
        reg = self._hyper()[1] if reg is None else float(reg)
        opt = _ffi.OPTIMIZER[self.optimizer if optimizer is None else optimizer]
        loss = torch.empty(n, dtype=torch.float32, device=self.device) if want_loss else None
        if pairs == 0:                                       # (no item has a pair: the library still wants the pointers)
            u_ = o_ = r_ = torch.zeros(1, dtype=torch.int32, device=self.device)
        return loss, call(_addr(ptr), _addr(u_), _addr(o_), _addr(r_), pairs, lr, reg, opt, loss)

    def acf_fold_in(self, pair_ptr, pos, neg, steps, Gu_rows, lists=None, csr=None, lr=None, reg=None, optimizer=None,
                    want_loss=True):
        """bprx_acf_fold_in: `steps` optimiser steps on each row of Gu_rows [n, k] (a contiguous fp32 device tensor, updated IN
        PLACE) over the pairs (pos[p], neg[p]), p in [pair_ptr[r], pair_ptr[r + 1]), of row r, through both attention levels over
        the row's history (`lists` per row, or a prebuilt `csr`), everything but the row frozen.  pair_ptr: int64 [n + 1].
        lr / reg / optimizer default to the engine's.  Returns loss fp32 [n] (loss_steps, before the last update) or None."""
        hp, hi, n = self._acf_rows("acf_fold_in", Gu_rows, lists, csr)
        return self._fold_in("acf_fold_in", self.lib.bprx_acf_fold_in, (_addr(hp), _addr(hi)), pair_ptr, pos, neg, steps,
                             (("Gu_rows", Gu_rows, self.k),), lr, reg, optimizer, want_loss, hist_rows=n)

    def acf_profile_rows(self, Gu_rows, lists=None, csr=None):
        """bprx_acf_profile_rows: g'_r [n, k] of the rows of a caller-owned table with the histories `lists` (per row, or a
        prebuilt `csr`)."""
        hp, hi, n = self._acf_rows("acf_profile_rows", Gu_rows, lists, csr)
        out = torch.empty((n, self.k), dtype=torch.float32, device=self.device)
        _ffi.check(self.h, self.lib.bprx_acf_profile_rows(self.h, _addr(Gu_rows), n, _addr(hp), _addr(hi), _addr(out), _stream()))
        return out

    def acf_score_rows_block(self, Gu_rows, r0, r1, lists=None, csr=None):
        """bprx_acf_score_rows_block: score_block for rows [r0, r1) of a caller-owned user table with the histories `lists` (per
        row of the whole table, or a prebuilt `csr`): scores [r1 - r0, I]."""
        hp, hi, n = self._acf_rows("acf_score_rows_block", Gu_rows, lists, csr)
        x = torch.empty((max(r1 - r0, 0), self.I), dtype=torch.float32, device=self.device)
        _ffi.check(self.h, self.lib.bprx_acf_score_rows_block(self.h, _addr(Gu_rows), n, _addr(hp), _addr(hi), int(r0), int(r1),
                                                              _addr(x), _stream()))
        return x

    def bind_attentive(self, Gu, Gi, Bi, edges, color, cls, weights, dropout=0.5, seed=0, slots=None):
        """AttentiveFashion (bprx_bind_attentive) on a BPRMF engine: edges uint8 [I, 224, 224], color fp32 [I, Dc] (each row already
        divided by its own max-abs), cls fp32 [I, Dk], weights = the thirteen tensors keyed by _ffi.AF_WEIGHTS (shapes of
        include/bprx.h).  Adam slots (m_ / v_ for Gu, Gi, Bi and every weight) are zeros unless given."""
        if self.model != "bprmf":
            raise ValueError("bind_attentive needs an Engine(model='bprmf', ...)")
        def prep(x, shape=None, dtype=torch.float32):
            x = torch.as_tensor(x).to(device=self.device, dtype=dtype)
            return (x.reshape(shape) if shape is not None else x).contiguous()
        Ed = prep(edges, (self.I, 224, 224), torch.uint8)
        Xc, Xk = prep(color), prep(cls)
        if Xc.dim() != 2 or Xk.dim() != 2 or Xc.shape[0] != self.I or Xk.shape[0] != self.I:
            raise ValueError("color / cls must be [num_items, D], got %s and %s" % (tuple(Xc.shape), tuple(Xk.shape)))
        Dc, Dk, k = int(Xc.shape[1]), int(Xk.shape[1]), self.k
        hh = int(torch.as_tensor(weights["attention.W_1"]).shape[1])
        shapes = {"color.W1": (Dc, 256), "color.b1": (256,), "color.W2": (256, k), "edges.conv": (25, 64), "edges.conv_b": (64,),
                  "edges.W2": (64, k), "class.W1": (Dk, 256), "class.b1": (256,), "class.W2": (256, k),
                  "attention.W_1": (k, hh), "attention.b_1": (hh,), "attention.W_2": (hh, 1), "attention.b_2": (1,)}
        t = {"Gu": prep(Gu, (self.U, self.k)), "Gi": prep(Gi, (self.I, self.k)), "Bi": prep(Bi, (self.I,))}
        for key in _ffi.AF_WEIGHTS:
            t[key] = prep(weights[key], shapes[key])
        if self.optimizer == "adam_tf23":
            for n in ["Gu", "Gi", "Bi"] + list(_ffi.AF_WEIGHTS):
                for s_ in ("m_", "v_"):
                    given = None if slots is None else slots.get(s_ + n)
                    t[s_ + n] = torch.zeros_like(t[n]) if given is None else prep(given, tuple(t[n].shape))
        self.af_inputs = (Ed, Xc, Xk)
        tb = _ffi.Tables()
        for n in _ffi.TABLE_FIELDS:
            setattr(tb, n, None if t.get(n) is None else t[n].data_ptr())
        af = _ffi.Attentive(Dc, Dk, hh, float(dropout), int(seed) & (2 ** 64 - 1), Ed.data_ptr(), Xc.data_ptr(), Xk.data_ptr())
        for q, key in enumerate(_ffi.AF_WEIGHTS):
            af.w[q] = t[key].data_ptr()
            if self.optimizer == "adam_tf23":
                af.m_w[q], af.v_w[q] = t["m_" + key].data_ptr(), t["v_" + key].data_ptr()
        torch.cuda.current_stream(self.device).synchronize()
        _ffi.check(self.h, self.lib.bprx_bind_attentive(self.h, C.byref(tb), C.byref(af)))
        self.attentive = True
        self.t = t
        return self

    def af_encode(self, items):
        """The three encodings of the listed items, dropout off (bprx_af_encode): fp32 device tensor [3, n, k]."""
        i = as_index(items, self.device)
        out = torch.empty((3, i.numel(), self.k), dtype=torch.float32, device=self.device)
        _ffi.check(self.h, self.lib.bprx_af_encode(self.h, _ptr(i), i.numel(), _ptr(out), _stream()))
        return out

    def af_attention_pairs(self, user, item):
        """Scores [n] and attentions [n, 3] (colour, edges, class) of the pairs, dropout off (bprx_af_attention_pairs)."""
        u, i = as_index(user, self.device), as_index(item, self.device)
        x = torch.empty(u.numel(), dtype=torch.float32, device=self.device)
        al = torch.empty((u.numel(), 3), dtype=torch.float32, device=self.device)
        _ffi.check(self.h, self.lib.bprx_af_attention_pairs(self.h, _ptr(u), _ptr(i), u.numel(), _ptr(x), _ptr(al), _stream()))
        return x, al

    def af_explain(self, user, item, grid=14, maps=True):
        """bprx_af_explain: the exact split of every pair's score over the three modalities, and of its edges share over a
        grid x grid partition of the 112 x 112 pooling windows (alpha held fixed at the value the model reports).  Returns a dict of
        device tensors: score [n], alpha [n, 3], parts [n, 3] (colour, edges, class; they sum to score), peak_cell int32 [n] (row-major
        index of the largest cell, the lowest among equals), peak_val [n], and with maps=True map [n, grid * grid] (its cells sum to
        parts[:, 1]).  Any n: the pairs go to the library in chunks of max_batch."""
        u, i = as_index(user, self.device), as_index(item, self.device)
        if u.numel() != i.numel():
            raise ValueError("af_explain: %d users for %d items" % (u.numel(), i.numel()))
        n, G = u.numel(), int(grid)
        G2 = G * G if 0 < G <= 112 else 0
        f = lambda *s: torch.empty(s, dtype=torch.float32, device=self.device)
        out = {"score": f(n), "alpha": f(n, 3), "parts": f(n, 3), "peak_cell": torch.empty(n, dtype=torch.int32, device=self.device),
               "peak_val": f(n)}
        if maps:
            out["map"] = f(n, G2)
        at = lambda t, r0: C.c_void_p(t.data_ptr() + r0 * t.stride(0) * t.element_size() if t.numel() else t.data_ptr())
        for r0 in range(0, max(n, 1), self.max_batch):          # (an empty call still reaches the library's argument checks)
            m = min(self.max_batch, n - r0)
            _ffi.check(self.h, self.lib.bprx_af_explain(self.h, at(u, r0), at(i, r0), m, G, at(out["score"], r0), at(out["alpha"], r0),
                                                        at(out["parts"], r0), at(out["map"], r0) if maps else None,
                                                        at(out["peak_cell"], r0), at(out["peak_val"], r0), _stream()))
        return out

    def af_score_block(self, u0, u1):
        """Scores [u1-u0, I] and attentions [u1-u0, I, 3] of a user block (bprx_af_score_block)."""
        x = torch.empty((u1 - u0, self.I), dtype=torch.float32, device=self.device)
        al = torch.empty((u1 - u0, self.I, 3), dtype=torch.float32, device=self.device)
        _ffi.check(self.h, self.lib.bprx_af_score_block(self.h, int(u0), int(u1), _ptr(x), _ptr(al), _stream()))
        return x, al

    def af_fold_in(self, pair_ptr, pos, neg, steps, Gu_rows, lr=None, reg=None, optimizer=None, want_loss=True):
        """bprx_af_fold_in: `steps` optimiser steps on each row of Gu_rows [n, k] (a contiguous fp32 device tensor, updated IN
        PLACE) over the pairs (pos[p], neg[p]), p in [pair_ptr[r], pair_ptr[r + 1]), of row r, the item side, the encoders and the
        attention tensors frozen and dropout off.  pair_ptr: int64 [n + 1].  lr / reg / optimizer default to the engine's.
        Returns loss fp32 [n] (loss_steps, before the last update) or None."""
        return self._fold_in("af_fold_in", self.lib.bprx_af_fold_in, (), pair_ptr, pos, neg, steps, (("Gu_rows", Gu_rows, self.k),),
                             lr, reg, optimizer, want_loss)

    def af_score_rows_block(self, Gu_rows, r0, r1, want_alpha=True):
        """bprx_af_score_rows_block: af_score_block for rows [r0, r1) of a caller-owned user table: scores [r1 - r0, I] and
        attentions [r1 - r0, I, 3] (None with want_alpha=False)."""
        x = torch.empty((r1 - r0, self.I), dtype=torch.float32, device=self.device)
        al = torch.empty((r1 - r0, self.I, 3), dtype=torch.float32, device=self.device) if want_alpha else None
        _ffi.check(self.h, self.lib.bprx_af_score_rows_block(self.h, _addr(Gu_rows), int(Gu_rows.shape[0]), int(r0), int(r1),
                                                             _addr(x), _addr(al), _stream()))
        return x, al

    # ---- AttentiveFashion: new items with first buyers (include/bprx.h, bprx_af_fold_in_items) ---------------------------------
    def af_encode_new(self, edges, color, cls):
        """bprx_af_encode_new: the three dropout-off encodings [3, n, k] of caller-owned inputs: edges uint8 [n, 224, 224], color
        fp32 [n, Dc] (each row already divided by its own max-abs), cls fp32 [n, Dk] (tensors or arrays; copied to the device)."""
        Dc, Dk = int(self.af_inputs[1].shape[1]), int(self.af_inputs[2].shape[1])
        prep = lambda x, dt: torch.as_tensor(x).to(device=self.device, dtype=dt).contiguous()
        Ed, Xc, Xk = prep(edges, torch.uint8), prep(color, torch.float32), prep(cls, torch.float32)
        n = int(Ed.shape[0]) if Ed.dim() == 3 else -1
        if n < 0 or tuple(Ed.shape) != (n, 224, 224) or tuple(Xc.shape) != (n, Dc) or tuple(Xk.shape) != (n, Dk):
            raise ValueError("af_encode_new: edges [n, 224, 224], color [n, %d], cls [n, %d] expected, got %s, %s, %s"
                             % (Dc, Dk, tuple(Ed.shape), tuple(Xc.shape), tuple(Xk.shape)))
        out = torch.empty((3, n, self.k), dtype=torch.float32, device=self.device)
        _ffi.check(self.h, self.lib.bprx_af_encode_new(self.h, _addr(Ed), _addr(Xc), _addr(Xk), n, _addr(out), _stream()))
        return out

    def af_work_stride(self):
        """KW: floats per pair of af_fold_in_items' work rows, k + 1 rounded up to a multiple of 4."""
        return (self.k + 1 + 3) // 4 * 4

    def _af_item_rows(self, what, C_rows, Gi_rows):
        """n of the caller-owned item rows C_rows [3, n, k] / Gi_rows [n, k], checked."""
        ok = lambda t, nd: t is not None and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.dim() == nd
        if not ok(Gi_rows, 2) or not ok(C_rows, 3) or tuple(C_rows.shape) != (3, int(Gi_rows.shape[0]), self.k) \
                or int(Gi_rows.shape[1]) != self.k:
            raise ValueError("%s: C_rows [3, n, %d] and Gi_rows [n, %d] must be contiguous fp32 device tensors" % (what, self.k, self.k))
        return int(Gi_rows.shape[0])

    def af_fold_in_items(self, pair_ptr, user, other, role, steps, C_rows, Gi_rows, lr=None, reg=None, optimizer=None,
                         want_loss=True, want_work=False):
        """bprx_af_fold_in_items: `steps` optimiser steps on each row of Gi_rows [n, k] (a contiguous fp32 device tensor, updated
        IN PLACE) over the pairs (user[p], other[p], role[p]), p in [pair_ptr[r], pair_ptr[r + 1]), of new item r with the
        encodings C_rows [3, n, k] (af_encode_new): role 0 the new item is the positive against the catalogue item other[p], role 1
        the negative.  Everything else is frozen, dropout off.  pair_ptr: int64 [n + 1].  lr / reg / optimizer default to the
        engine's.  The work rows [pairs, af_work_stride()] = [D_p | dc_p | zeros] are allocated here.  Returns loss fp32 [n]
        (loss_steps, before the last update) or None; with want_work=True (loss, work)."""
        n = self._af_item_rows("af_fold_in_items", C_rows, Gi_rows)
        ptr_host = torch.as_tensor(pair_ptr, dtype=torch.int64).cpu()

        def call(ptr, u_, o_, r_, given, lr, reg, opt, loss):
            pairs = int(ptr_host[-1])
            if pairs != given:
                raise ValueError("af_fold_in_items: pair_ptr ends at %d, %d pairs given" % (pairs, given))
            work = torch.empty((max(pairs, 1), self.af_work_stride()), dtype=torch.float32, device=self.device)
            _ffi.check(self.h, self.lib.bprx_af_fold_in_items(self.h, ptr, u_, o_, r_, n, _addr(C_rows), int(steps), lr, reg, opt,
                                                              _addr(Gi_rows), _addr(loss), _addr(work), _stream()))
            return work[:pairs]

        loss, work = self._fold_in_items("af_fold_in_items", ptr_host, user, other, role, n, lr, reg, optimizer, want_loss, call)
        return (loss, work) if want_work else loss

    def af_score_warm_block(self, u0, u1, C_rows, Gi_rows, want_alpha=True):
        """bprx_af_score_warm_block: af_score_block for caller-owned item rows: scores [u1 - u0, n] and attentions [u1 - u0, n, 3]
        (None with want_alpha=False)."""
        n = self._af_item_rows("af_score_warm_block", C_rows, Gi_rows)
        x = torch.empty((max(u1 - u0, 0), n), dtype=torch.float32, device=self.device)
        al = torch.empty((max(u1 - u0, 0), n, 3), dtype=torch.float32, device=self.device) if want_alpha else None
        _ffi.check(self.h, self.lib.bprx_af_score_warm_block(self.h, int(u0), int(u1), _addr(C_rows), _addr(Gi_rows), n, _addr(x),
                                                             _addr(al), _stream()))
        return x, al

    def af_audience_block(self, q0, q1, C_rows=None, Gi_rows=None, want_alpha=True):
        """bprx_af_audience_block: the same scores item-major for the rows [q0, q1) of the caller's item rows (both None: of the
        catalogue): scores [q1 - q0, U] and attentions [q1 - q0, U, 3] (None with want_alpha=False)."""
        if C_rows is None and Gi_rows is None:
            n = self.I
        else:
            n = self._af_item_rows("af_audience_block", C_rows, Gi_rows)
        x = torch.empty((max(q1 - q0, 0), self.U), dtype=torch.float32, device=self.device)
        al = torch.empty((max(q1 - q0, 0), self.U, 3), dtype=torch.float32, device=self.device) if want_alpha else None
        _ffi.check(self.h, self.lib.bprx_af_audience_block(self.h, _addr(C_rows), _addr(Gi_rows), n, int(q0), int(q1), _addr(x),
                                                           _addr(al), _stream()))
        return x, al

    def af_dropout_mask(self, step, n_rows):
        """The keep masks of step index `step` for n_rows = 2B sample rows (bprx_af_dropout_mask): three uint8 device tensors
        [n_rows, 256], [n_rows, 64], [n_rows, 256] (colour hidden units, pooled edge channels, class hidden units)."""
        out = torch.empty(int(n_rows) * 576, dtype=torch.uint8, device=self.device)
        _ffi.check(self.h, self.lib.bprx_af_dropout_mask(self.h, int(step), int(n_rows), _ptr(out), _stream()))
        n = int(n_rows)
        return out[:n * 256].view(n, 256), out[n * 256:n * 320].view(n, 64), out[n * 320:].view(n, 256)

    @property
    def af_step(self):
        return int(self.lib.bprx_af_get_step(self.h))

    @af_step.setter
    def af_step(self, v):
        _ffi.check(self.h, self.lib.bprx_af_set_step(self.h, int(v)))

    def explain_pairs(self, user, item):
        """GradFashion.predict_ui_grads for every pair (bprx_explain_pairs): fp32 device tensor [n, 2] = (colour, edges)."""
        u, i = as_index(user, self.device), as_index(item, self.device)
        out = torch.empty((u.numel(), 2), dtype=torch.float32, device=self.device)
        _ffi.check(self.h, self.lib.bprx_explain_pairs(self.h, _ptr(u), _ptr(i), u.numel(), _ptr(out), _stream()))
        return out

    def feat_explain(self, user, item, top=5, ncols=None, maps=False):
        """bprx_feat_explain on a VBPR engine, plain or factored: x_ui = base + sum_c F_ic w_uc, w_uc = Bp[c] + E[c,:].Tu_u.  Returns
        a dict of device tensors: score, base, visual [n]; col int32 and contrib [n, top]: the `top` feature columns with the largest
        F_ic w_uc (rank 0 first, equal values in ascending column order; slots beyond ncols: -1 / 0); with maps=True also map
        [n, ncols], every F_ic w_uc.  ncols (default feat_dim): the columns that exist, the rest being zero padding.  Any n."""
        u, i = as_index(user, self.device), as_index(item, self.device)
        if u.numel() != i.numel():
            raise ValueError("feat_explain: %d users for %d items" % (u.numel(), i.numel()))
        n, top = u.numel(), int(top)
        ncols = self.D if ncols is None else int(ncols)
        f = lambda *s: torch.empty(s, dtype=torch.float32, device=self.device)
        out = {"score": f(n), "base": f(n), "visual": f(n),
               "col": torch.empty((n, max(top, 0)), dtype=torch.int32, device=self.device), "contrib": f(n, max(top, 0))}
        if maps:
            out["map"] = f(n, max(ncols, 0))
        F = self._t.get("F")
        _ffi.check(self.h, self.lib.bprx_feat_explain(self.h, _addr(F), _addr(u), _addr(i), n, ncols, top,
                                                      _addr(out["score"]), _addr(out["base"]), _addr(out["visual"]), _addr(out["col"]),
                                                      _addr(out["contrib"]), _addr(out["map"]) if maps else None, _stream()))
        return out

    # ---- items outside the catalogue (include/bprx.h: x_uj = Tu_u.(f_j E) + f_j.Bp, no Gi / Bi term) --------------------------
    def _new_table(self, F):
        """A [n, feat_dim] table of new items as a contiguous device tensor of the engine's feature dtype, quantised as bind does
        (an fp8 engine: left in fp32 -- the library rejects the call, BPRX_E_INVALID)."""
        Ft = torch.as_tensor(F)
        if self.model == "vbpr" and (Ft.dim() != 2 or Ft.shape[1] != self.D):
            raise ValueError("new items: the table must be [n, %d], got %s" % (self.D, tuple(Ft.shape)))
        return Ft.to(device=self.device, dtype=torch.bfloat16 if self.feat_dtype == "bf16" else torch.float32).contiguous()

    def proj_stride(self):
        return int(_ffi.check(self.h, self.lib.bprx_proj_stride(self.h)))

    def project_rows(self, F):
        """bprx_project_rows: P fp32 [n, proj_stride()] = F.[E|Bp|0] for the rows of a [n, feat_dim] table of items the model was
        not trained on (normalised like the training table; quantised here as bind quantises)."""
        Ft = self._new_table(F)
        n = int(Ft.shape[0])
        P = torch.empty((n, self.proj_stride()), dtype=torch.float32, device=self.device)
        _ffi.check(self.h, self.lib.bprx_project_rows(self.h, _addr(Ft), n, _addr(P), _stream()))
        return P

    def score_new_block(self, u0, u1, P, out=None):
        """bprx_score_new_block: fp32 [u1-u0, n], out[u][j] = Tu_u.P[j, :d] + P[j, d] for P = project_rows(F)."""
        n = int(P.shape[0])
        if out is None:
            out = torch.empty((u1 - u0, n), dtype=torch.float32, device=self.device)
        _ffi.check(self.h, self.lib.bprx_score_new_block(self.h, int(u0), int(u1), _addr(P), n, _addr(out), _stream()))
        return out

    def topk_rows(self, scores, K):
        """bprx_topk_rows: bprx_topk's lists for the rows of a contiguous fp32 [nrows, width] device tensor, nothing masked:
        (idx int32 [nrows, K], val fp32 [nrows, K], flag int32 [nrows])."""
        nrows, width = (int(x) for x in scores.shape)
        K = int(K)
        idx, val, flag = self._topk_out(nrows, K)
        _ffi.check(self.h, self.lib.bprx_topk_rows(self.h, nrows, width, _addr(scores), K, _addr(idx), _addr(val), _addr(flag), _stream()))
        return idx, val, flag

    def feat_explain_new(self, F, user, row, top=5, ncols=None, maps=False):
        """bprx_feat_explain_new: feat_explain for the pairs (user[p], row[p] of the new-item table F).  There is no base: the dict
        holds score (== visual, the same tensor) [n], col int32 and contrib [n, top], with maps=True also map [n, ncols]."""
        Ft = self._new_table(F)
        u, r = as_index(user, self.device), as_index(row, self.device)
        if u.numel() != r.numel():
            raise ValueError("feat_explain_new: %d users for %d rows" % (u.numel(), r.numel()))
        n, top = u.numel(), int(top)
        ncols = self.D if ncols is None else int(ncols)
        f = lambda *s: torch.empty(s, dtype=torch.float32, device=self.device)
        out = {"score": f(n), "col": torch.empty((n, max(top, 0)), dtype=torch.int32, device=self.device), "contrib": f(n, max(top, 0))}
        out["visual"] = out["score"]
        if maps:
            out["map"] = f(n, max(ncols, 0))
        _ffi.check(self.h, self.lib.bprx_feat_explain_new(self.h, _addr(Ft), int(Ft.shape[0]), _addr(u), _addr(r), n, ncols, top,
                                                          _addr(out["score"]), _addr(out["col"]), _addr(out["contrib"]),
                                                          _addr(out["map"]) if maps else None, _stream()))
        return out

    # ---- users outside the training set (include/bprx.h: the reference's step on one user's pairs, the item side frozen) -------
    def fold_in(self, pair_ptr, pos, neg, steps, Gu_rows, Tu_rows=None, lr=None, reg=None, optimizer=None, want_loss=True):
        """bprx_fold_in: `steps` optimiser steps on each row of Gu_rows [n, k] / Tu_rows [n, d] (contiguous fp32 device tensors,
        updated IN PLACE; Tu_rows is None iff d == 0) over the pairs (pos[p], neg[p]), p in [pair_ptr[r], pair_ptr[r + 1]), of row
        r.  pair_ptr: int64 [n + 1].  lr / reg / optimizer default to the engine's.  Returns loss fp32 [n] (loss_steps, before the
        last update) or None."""
        return self._fold_in("fold_in", self.lib.bprx_fold_in, (), pair_ptr, pos, neg, steps,
                             (("Gu_rows", Gu_rows, self.k), ("Tu_rows", Tu_rows, self.d)), lr, reg, optimizer, want_loss)

    def score_rows_block(self, Gu_rows, Tu_rows, r0, r1, out=None):
        """bprx_score_rows_block: score_block for rows [r0, r1) of caller-owned user tables: fp32 [r1 - r0, I]."""
        if out is None:
            out = torch.empty((r1 - r0, self.I), dtype=torch.float32, device=self.device)
        _ffi.check(self.h, self.lib.bprx_score_rows_block(self.h, _addr(Gu_rows), _addr(Tu_rows), int(Gu_rows.shape[0]), int(r0), int(r1),
                                                          _addr(out), _stream()))
        return out

    def topk_lists(self, scores, lists_csr, K):
        """bprx_topk_lists: bprx_topk for the rows of a contiguous fp32 [nrows, I] device tensor; row r masks (IN `scores`) the
        items of list r of lists_csr = (int64 ptr [nrows + 1], int32 items): (idx int32 [nrows, K], val, flag int32 [nrows])."""
        nrows, K = int(scores.shape[0]), int(K)
        idx, val, flag = self._topk_out(nrows, K)
        ptr, items = lists_csr
        _ffi.check(self.h, self.lib.bprx_topk_lists(self.h, nrows, _addr(scores), _addr(ptr), _addr(items), K, _addr(idx), _addr(val),
                                                    _addr(flag), _stream()))
        return idx, val, flag

    # ---- similar items (include/bprx.h: the cosine of two item vectors, z = Gi | f E | both) --------------------------------------
    def sim_rnorm(self, space, Pq=None):
        """bprx_sim_rnorm: fp32 [I], 1 / |z_i| of every catalogue item in `space` ('latent', 'visual', 'both' or BPRX_SIM_*; 0 for a
        zero row); with Pq = project_rows(F): fp32 [n] of those rows (visual only)."""
        n = self.I if Pq is None else int(Pq.shape[0])
        rn = torch.empty(n, dtype=torch.float32, device=self.device)
        _ffi.check(self.h, self.lib.bprx_sim_rnorm(self.h, _ffi.SIM_SPACE.get(space, space), _addr(Pq), n, _addr(rn), _stream()))
        return rn

    def sim_block(self, space, q0, q1, rn_items, Pq=None, rn_q=None, out=None):
        """bprx_sim_block: fp32 [q1 - q0, I], the cosine of the catalogue items q0 .. q1-1 (Pq: of rows q0 .. q1-1 of Pq, with
        rn_q = sim_rnorm(space, Pq)) with every catalogue item; the item itself is not masked.  rn_items = sim_rnorm(space)."""
        if rn_q is None:
            if Pq is not None:
                raise ValueError("sim_block: rows from outside the catalogue come with their norms (rn_q = sim_rnorm(space, Pq))")
            rn_q = rn_items
        nq = self.I if Pq is None else int(Pq.shape[0])
        if out is None:
            out = torch.empty((max(q1 - q0, 0), self.I), dtype=torch.float32, device=self.device)
        _ffi.check(self.h, self.lib.bprx_sim_block(self.h, _ffi.SIM_SPACE.get(space, space), _addr(Pq), nq, int(q0), int(q1), _addr(rn_q),
                                                   _addr(rn_items), _addr(out), _stream()))
        return out

    # ---- style clusters (include/bprx.h: spherical k-means of the item space, bprx_style_assign / bprx_style_update) ---------------
    def _style_width(self, space):
        """The numbers of an item vector in `space`: k, d or k + d."""
        sp = _ffi.SIM_SPACE.get(space, space)
        return {0: self.k, 1: self.d, 2: self.k + self.d}.get(sp, 0)

    def _style_table(self, what, space, cent):
        """S of the centroid table `cent`, a contiguous fp32 device tensor [S, w] (w = the width of `space`), checked."""
        w = self._style_width(space)
        if not (isinstance(cent, torch.Tensor) and cent.is_cuda and cent.dtype == torch.float32 and cent.is_contiguous()
                and cent.dim() == 2 and (w == 0 or int(cent.shape[1]) == w)):
            raise ValueError("%s: the centroids are a contiguous fp32 device tensor [S, %d]" % (what, w))
        return int(cent.shape[0])

    def style_assign(self, space, cent, q0, q1, rn_items, Pq=None, rn_q=None, want_second=True):
        """bprx_style_assign: (style int32 [q1 - q0], cos fp32 [q1 - q0], second fp32 [q1 - q0]) of the catalogue items q0 .. q1-1
        (Pq = project_rows(F): of rows q0 .. q1-1 of Pq, with rn_q = sim_rnorm(space, Pq), visual only) against the centroid rows
        of `cent` (fp32 [S, w], unit or zero rows): the nearest centroid by cosine (ties: the smallest index; -1 for a zero row),
        that cosine, and the largest cosine with another centroid (-inf for S == 1; None with want_second=False)."""
        if rn_q is None:
            if Pq is not None:
                raise ValueError("style_assign: rows from outside the catalogue come with their norms (rn_q = sim_rnorm(space, Pq))")
            rn_q = rn_items
        S = self._style_table("style_assign", space, cent)
        nq = self.I if Pq is None else int(Pq.shape[0])
        n = max(int(q1) - int(q0), 0)
        buf = lambda dtype: torch.empty(max(n, 1), dtype=dtype, device=self.device)        # (an empty range still hands pointers over)
        style, cos, second = buf(torch.int32), buf(torch.float32), buf(torch.float32) if want_second else None
        _ffi.check(self.h, self.lib.bprx_style_assign(self.h, _ffi.SIM_SPACE.get(space, space), _addr(Pq), nq, int(q0), int(q1),
                                                      _addr(rn_q), _addr(cent), S, _addr(style), _addr(cos), _addr(second), _stream()))
        return style[:n], cos[:n], None if second is None else second[:n]

    def style_update(self, space, rn_items, member_csr, cent_prev):
        """bprx_style_update: (cent fp32 [S, w], mass fp32 [S]) for the clusters of member_csr = (int64 ptr [S + 1], int32 items, S)
        as ranking.class_csr makes it: every cluster's fp64 sum of its members' unit rows, normalised; an empty cluster (or one
        whose rows cancel) keeps its row of cent_prev and has mass 0.  rn_items = sim_rnorm(space)."""
        ptr, items, S = member_csr
        if self._style_table("style_update", space, cent_prev) != int(S):
            raise ValueError("style_update: %d clusters, %d centroid rows" % (int(S), int(cent_prev.shape[0])))
        cent = torch.empty_like(cent_prev)
        mass = torch.empty(int(S), dtype=torch.float32, device=self.device)
        _ffi.check(self.h, self.lib.bprx_style_update(self.h, _ffi.SIM_SPACE.get(space, space), _addr(rn_items), _addr(ptr), _addr(items),
                                                      int(S), _addr(cent_prev), _addr(cent), _addr(mass), _stream()))
        return cent, mass

    # ---- audiences (include/bprx.h: the score block item-major, one row per item against every user) -----------------------------
    def audience_block(self, q0, q1, P=None, out=None):
        """bprx_audience_block: fp32 [q1 - q0, U], the scores of the catalogue items q0 .. q1-1 (P = project_rows(F): of rows
        q0 .. q1-1 of P, the visual score of items outside the catalogue) for every user: score_block / score_new_block
        item-major, bit for bit where k and d are even."""
        nq = self.I if P is None else int(P.shape[0])
        if out is None:
            out = torch.empty((max(q1 - q0, 0), self.U), dtype=torch.float32, device=self.device)
        _ffi.check(self.h, self.lib.bprx_audience_block(self.h, _addr(P), nq, int(q0), int(q1), _addr(out), _stream()))
        return out

    # ---- warm items (include/bprx.h: Gi / Bi rows for new items with first buyers, everything else frozen) ----------------------
    def _warm_rows(self, what, Gi_rows, Bi_rows, Pn):
        """n of the caller-owned item rows Gi_rows [n, k] / Bi_rows [n] / Pn [n, proj_stride()] (None iff d == 0), checked."""
        n = int(Bi_rows.shape[0]) if Bi_rows is not None and Bi_rows.dim() == 1 else -1
        if n < 0 or not (Bi_rows.is_cuda and Bi_rows.dtype == torch.float32 and Bi_rows.is_contiguous()):
            raise ValueError("%s: Bi_rows must be a contiguous fp32 device tensor [n]" % what)
        if (self.d > 0) != (Pn is not None):
            raise ValueError("%s: Pn = project_rows(F) is needed iff the model has a visual part (d = %d)" % (what, self.d))
        self._check_rows(what, n, ("Gi_rows", Gi_rows, self.k), ("Pn", Pn, self.proj_stride() if self.d else 0))
        if Gi_rows is None:
            raise ValueError("%s: Gi_rows is None" % what)
        return n

    def fold_in_items(self, pair_ptr, user, other, role, steps, Gi_rows, Bi_rows, Pn=None, lr=None, reg=None, optimizer=None,
                      want_loss=True):
        """bprx_fold_in_items: `steps` optimiser steps on each row of Gi_rows [n, k] / Bi_rows [n] (contiguous fp32 device tensors,
        updated IN PLACE) over the pairs (user[p], other[p], role[p]), p in [pair_ptr[r], pair_ptr[r + 1]), of new item r: role 0
        the new item is the positive against the catalogue item other[p], role 1 the negative.  Pn = project_rows(F) of the new
        items (None iff d == 0).  pair_ptr: int64 [n + 1].  lr / reg / optimizer default to the engine's.  Plain sgd sums the
        batch loss and oscillates once lr * 0.25 * pairs * (1 + |Gu|^2) passes 2: few pairs or a small lr; Adam does not care.
        Returns loss fp32 [n] (loss_steps, before the last update) or None."""
        n = self._warm_rows("fold_in_items", Gi_rows, Bi_rows, Pn)
        call = lambda ptr, u_, o_, r_, _, lr, reg, opt, loss: _ffi.check(self.h, self.lib.bprx_fold_in_items(
            self.h, ptr, u_, o_, r_, n, _addr(Pn), int(steps), lr, reg, opt, _addr(Gi_rows), _addr(Bi_rows), _addr(loss), _stream()))
        return self._fold_in_items("fold_in_items", pair_ptr, user, other, role, n, lr, reg, optimizer, want_loss, call)[0]

    def score_warm_block(self, u0, u1, Gi_rows, Bi_rows, Pn=None, out=None):
        """bprx_score_warm_block: fp32 [u1 - u0, n], out[u][j] = Bi_j + Gu_u.Gi_j + Tu_u.Pn[j, :d] + Pn[j, d] for caller-owned item
        rows (fold_in_items' result; Pn None iff d == 0): score_block's kernels, given these rows."""
        n = self._warm_rows("score_warm_block", Gi_rows, Bi_rows, Pn)
        if out is None:
            out = torch.empty((max(u1 - u0, 0), n), dtype=torch.float32, device=self.device)
        _ffi.check(self.h, self.lib.bprx_score_warm_block(self.h, int(u0), int(u1), _addr(Gi_rows), _addr(Bi_rows), _addr(Pn), n,
                                                          _addr(out), _stream()))
        return out

    def audience_warm_block(self, Gi_rows, Bi_rows, Pn, q0, q1, out=None):
        """bprx_audience_warm_block: fp32 [q1 - q0, U], score_warm_block item-major for rows q0 .. q1-1 (bit for bit where k and d
        are even)."""
        n = self._warm_rows("audience_warm_block", Gi_rows, Bi_rows, Pn)
        if out is None:
            out = torch.empty((max(q1 - q0, 0), self.U), dtype=torch.float32, device=self.device)
        _ffi.check(self.h, self.lib.bprx_audience_warm_block(self.h, _addr(Gi_rows), _addr(Bi_rows), _addr(Pn), n, int(q0), int(q1),
                                                             _addr(out), _stream()))
        return out

    def topk_rows_masked(self, scores, lists_csr, K):
        """bprx_topk_rows_masked: topk_rows for the rows of a contiguous fp32 [nrows, width] device tensor, row r masking (IN
        `scores`) the ids of list r of lists_csr = (int64 ptr [nrows + 1], int32 ids): (idx int32 [nrows, K], val, flag)."""
        nrows, width = (int(x) for x in scores.shape)
        K = int(K)
        idx, val, flag = self._topk_out(nrows, K)
        ptr, items = lists_csr
        _ffi.check(self.h, self.lib.bprx_topk_rows_masked(self.h, nrows, width, _addr(scores), _addr(ptr), _addr(items), K, _addr(idx),
                                                          _addr(val), _addr(flag), _stream()))
        return idx, val, flag

    def topk_classes(self, scores, lists_csr, class_csr, K, row0=0):
        """bprx_topk_classes: the K best entries of every class of every row of a contiguous fp32 [nrows, width] device tensor.  Row
        r masks (IN `scores`) the ids of list row0 + r of lists_csr = (int64 ptr, int32 ids), None: nothing is masked; class_csr =
        (int64 ptr [C + 1], int32 items, C) as ranking.class_csr makes it.  Returns (idx int32 [nrows, C, K], val fp32 [nrows, C, K],
        cnt int32 [nrows, C]): per class best first, equal scores by ascending item, -1 / 0.0 past cnt; masked items are on no list."""
        nrows, width = (int(x) for x in scores.shape)
        K = int(K)
        ptr, items = (None, None) if lists_csr is None else lists_csr
        cptr, citems, C = class_csr
        C = int(C)
        idx = torch.empty((nrows, max(C, 0), max(K, 0)), dtype=torch.int32, device=self.device)
        val = torch.empty((nrows, max(C, 0), max(K, 0)), dtype=torch.float32, device=self.device)
        cnt = torch.empty((nrows, max(C, 0)), dtype=torch.int32, device=self.device)
        _ffi.check(self.h, self.lib.bprx_topk_classes(self.h, nrows, width, _addr(scores), int(row0), _addr(ptr), _addr(items),
                                                      _addr(cptr), _addr(citems), C, K, _addr(idx), _addr(val), _addr(cnt), _stream()))
        return idx, val, cnt

    def diversify(self, space, rn, pool_idx, pool_val, k, theta):
        """bprx_diversify: greedy MMR over the pools (pool_idx int32, pool_val fp32: contiguous device tensors [n, N], best first,
        as the top-K entries return them) in `space`, rn = sim_rnorm(space): (idx int32 [n, k], val fp32 [n, k] the picks' pool
        scores, pen fp32 [n, k] each pick's largest cosine with the picks above it, ild fp32 [n] the lists' intra-list
        diversity).  theta in [0, 1]: 0 keeps the pool's order, 1 ranks by dissimilarity alone.  Slots past the candidates of
        a pool hold -1 / 0 / 0."""
        n, N = (int(x) for x in pool_idx.shape)
        if tuple(pool_val.shape) != (n, N) or pool_idx.dtype != torch.int32 or pool_val.dtype != torch.float32:
            raise ValueError("diversify: pool_idx int32 [n, N] and pool_val fp32 [n, N]")
        if not (pool_idx.is_contiguous() and pool_val.is_contiguous()):
            raise ValueError("diversify: the pools must be contiguous")
        k = int(k)
        idx = torch.empty((n, max(k, 0)), dtype=torch.int32, device=self.device)
        val, pen = (torch.empty((n, max(k, 0)), dtype=torch.float32, device=self.device) for _ in range(2))
        ild = torch.empty(n, dtype=torch.float32, device=self.device)
        _ffi.check(self.h, self.lib.bprx_diversify(self.h, _ffi.SIM_SPACE.get(space, space), _addr(rn), n, N, _addr(pool_idx),
                                                   _addr(pool_val), k, float(theta), _addr(idx), _addr(val), _addr(pen), _addr(ild),
                                                   _stream()))
        return idx, val, pen, ild

    def calibrate(self, pool_idx, pool_val, hist_csr, item_class, C, k, lam, alpha=0.01, row0=0):
        """bprx_calibrate: greedy KL re-rank of the pools (pool_idx int32, pool_val fp32: contiguous device tensors [n, N], best
        first, as the top-K entries return them) toward the class mix of each list's history.  hist_csr = (int64 ptr, int32 items)
        on the device, list r's history is list row0 + r of it (None: every history is empty); item_class: a contiguous int32
        device tensor [width], -1 = no class, otherwise in [0, C).  lam in [0, 1]: 0 keeps the pool's order, 1 ranks by the KL
        gain alone; alpha in (0, 1) smooths the list's class shares.  Returns the device (idx int32 [n, k], val fp32 [n, k] the
        picks' pool scores, cls int32 [n, k] their classes, gain fp32 [n, k] the KL term each pick removed, kl fp32 [n, 2] the
        KL(p || q~) of the pool's first k candidates and of the calibrated list).  Slots past the candidates of a pool hold -1 / 0 /
        -1 / 0."""
        n, N = (int(x) for x in pool_idx.shape)
        if tuple(pool_val.shape) != (n, N) or pool_idx.dtype != torch.int32 or pool_val.dtype != torch.float32:
            raise ValueError("calibrate: pool_idx int32 [n, N] and pool_val fp32 [n, N]")
        if not (pool_idx.is_contiguous() and pool_val.is_contiguous()):
            raise ValueError("calibrate: the pools must be contiguous")
        if item_class.dim() != 1 or item_class.dtype != torch.int32 or not item_class.is_contiguous():
            raise ValueError("calibrate: item_class is a contiguous int32 tensor [width]")
        ptr, items = (None, None) if hist_csr is None else hist_csr
        if ptr is not None and (ptr.dtype != torch.int64 or items.dtype != torch.int32):
            raise ValueError("calibrate: hist_csr = (int64 ptr, int32 items)")
        k = int(k)
        idx, cls = (torch.empty((n, max(k, 0)), dtype=torch.int32, device=self.device) for _ in range(2))
        val, gain = (torch.empty((n, max(k, 0)), dtype=torch.float32, device=self.device) for _ in range(2))
        kl = torch.empty((n, 2), dtype=torch.float32, device=self.device)
        _ffi.check(self.h, self.lib.bprx_calibrate(self.h, n, N, _addr(pool_idx), _addr(pool_val), int(row0), _addr(ptr), _addr(items),
                                                   _addr(item_class), int(item_class.shape[0]), int(C), k, float(lam), float(alpha),
                                                   _addr(idx), _addr(val), _addr(cls), _addr(gain), _addr(kl), _stream()))
        return idx, val, cls, gain, kl

    def because(self, space, rn, list_idx, hist_csr, top, Pq=None, rn_q=None):
        """bprx_because: for every entry of the lists (list_idx: contiguous int32 device tensor [n, K], catalogue ids, or rows of
        Pq = project_rows(F) with rn_q = sim_rnorm('visual', Pq); a slot < 0 is empty) the `top` (1..32) nearest items of the
        list's history by cosine in `space`, rn = sim_rnorm(space).  hist_csr = (int64 ptr [n + 1], int32 items) on the device,
        list r's history.  Returns device (item int32 [n, K, top], cos fp32 [n, K, top], cnt int32 [n, K]): the history's ids by
        descending cosine (ties: the earlier entry), -1 / 0 past the candidates, and the number of candidates (the history
        without the explained item itself)."""
        if list_idx.dim() != 2 or list_idx.dtype != torch.int32 or not list_idx.is_contiguous():
            raise ValueError("because: list_idx is a contiguous int32 tensor [n, K]")
        if Pq is not None and rn_q is None:
            raise ValueError("because: rows from outside the catalogue come with their norms (rn_q = sim_rnorm('visual', Pq))")
        n, K = (int(x) for x in list_idx.shape)
        ptr, items = hist_csr
        if ptr.dtype != torch.int64 or items.dtype != torch.int32 or int(ptr.numel()) != n + 1:
            raise ValueError("because: hist_csr is (int64 ptr [n + 1], int32 items), one history per list")
        top = int(top)
        item = torch.empty((n, K, max(top, 0)), dtype=torch.int32, device=self.device)
        cos = torch.empty((n, K, max(top, 0)), dtype=torch.float32, device=self.device)
        cnt = torch.empty((n, K), dtype=torch.int32, device=self.device)
        nq = self.I if Pq is None else int(Pq.shape[0])
        _ffi.check(self.h, self.lib.bprx_because(self.h, _ffi.SIM_SPACE.get(space, space), _addr(Pq), nq, _addr(rn_q), _addr(rn), n, K,
                                                 _addr(list_idx), _addr(ptr), _addr(items), top, _addr(item), _addr(cos), _addr(cnt),
                                                 _stream()))
        return item, cos, cnt

    def influence(self, Gu_rows, Tu_rows, pair_ptr, pos, neg, per_entry, list_idx, top, reg=None, damp=1.0, maps=False):
        """bprx_influence: for every entry of the lists (list_idx: contiguous int32 device tensor [n, K] of catalogue ids, a slot
        < 0 is empty) the `top` (1..32) history entries of row r the entry's score rests on most, on the fold-in objective of the
        row [Gu_rows_r | Tu_rows_r] (contiguous fp32 device tensors [n, k] / [n, d], Tu_rows None iff d == 0) over its pairs
        (pos[p], neg[p]), p in [pair_ptr[r], pair_ptr[r + 1]); `per_entry` consecutive pairs are one history entry.  reg defaults
        to the engine's.  Returns the device dict item int32 [n, K, top] (the entries' ids by descending influence, -1 past
        them), infl fp32 [n, K, top], total fp32 [n, K] (sum of |influence| over all entries), cnt int32 [n, K] (entries),
        flag int32 [n] (1: the row's factorisation failed, its slots are empty) and, with maps, full fp32 [n, K, M] (every
        entry's influence, M the longest row's entries; 0 past a row's own)."""
        if list_idx.dim() != 2 or list_idx.dtype != torch.int32 or not list_idx.is_contiguous():
            raise ValueError("influence: list_idx is a contiguous int32 tensor [n, K]")
        n, K = (int(x) for x in list_idx.shape)
        if pair_ptr.dtype != torch.int64 or pos.dtype != torch.int32 or neg.dtype != torch.int32 or int(pair_ptr.numel()) != n + 1:
            raise ValueError("influence: pair_ptr is int64 [n + 1], pos / neg are int32, one row per list")
        for name, rows, width in (("Gu_rows", Gu_rows, self.k), ("Tu_rows", Tu_rows, self.d)):
            if (rows is None) != (width == 0):
                raise ValueError("influence: %s is None exactly when its width is 0" % name)
            if rows is not None and (rows.dtype != torch.float32 or not rows.is_contiguous() or tuple(rows.shape) != (n, width)):
                raise ValueError("influence: %s is a contiguous fp32 tensor [%d, %d]" % (name, n, width))
        top, per_entry = int(top), int(per_entry)
        reg = self._hyper()[1] if reg is None else float(reg)
        out = {"item": torch.empty((n, K, max(top, 0)), dtype=torch.int32, device=self.device),
               "infl": torch.empty((n, K, max(top, 0)), dtype=torch.float32, device=self.device),
               "total": torch.empty((n, K), dtype=torch.float32, device=self.device),
               "cnt": torch.empty((n, K), dtype=torch.int32, device=self.device),
               "flag": torch.empty(n, dtype=torch.int32, device=self.device)}
        stride = 1
        if maps:
            m = (pair_ptr[1:] - pair_ptr[:-1]).max().item() if n else 0
            stride = max(1, -(-int(m) // max(per_entry, 1)))
            out["full"] = torch.zeros((n, K, stride), dtype=torch.float32, device=self.device)
        _ffi.check(self.h, self.lib.bprx_influence(self.h, _addr(Gu_rows), _addr(Tu_rows), n, _addr(pair_ptr), _addr(pos), _addr(neg),
                                                   per_entry, reg, float(damp), K, _addr(list_idx), top, _addr(out["item"]),
                                                   _addr(out["infl"]), _addr(out["total"]), _addr(out["cnt"]),
                                                   _addr(out["full"]) if maps else None, stride, _addr(out["flag"]), _stream()))
        return out

    def _hyper(self):
        return self._lr_reg

    def tables_dirty(self):
        """Call after writing any bound table from outside the library (bprx_tables_dirty): the handle reuses images
        derived from E/Bp (their bf16/fp8 copy, the item projections) until a step changes them."""
        _ffi.check(self.h, self.lib.bprx_tables_dirty(self.h, _stream()))

    def params(self):
        names = FACTORED_PARAM_NAMES if getattr(self, "factored", False) else PARAM_NAMES
        return {n: self.t[n] for n in names if self.t.get(n) is not None}

    def set_hyper(self, lr, reg):
        _ffi.check(self.h, self.lib.bprx_set_hyper(self.h, lr, reg))
        self._lr_reg = (float(lr), float(reg))

    @property
    def adam_step(self):
        return int(self.lib.bprx_get_adam_step(self.h))

    @adam_step.setter
    def adam_step(self, v):
        _ffi.check(self.h, self.lib.bprx_set_adam_step(self.h, int(v), _stream()))

    # ---- hot path ------------------------------------------------------------------------------------------------
    def score_pairs(self, user, item):
        u, i = as_index(user, self.device), as_index(item, self.device)
        x = torch.empty(u.numel(), dtype=torch.float32, device=self.device)
        for s in range(0, u.numel(), self.max_batch):            # the handle's pair scratch holds max_batch rows
            n = min(self.max_batch, u.numel() - s)
            _ffi.check(self.h, self.lib.bprx_score_pairs(self.h, _ptr(u[s:s + n]), _ptr(i[s:s + n]), n,
                                                         _ptr(x[s:s + n]), _stream()))
        return x

    def step(self, user, pos, neg, want_loss=True, loss_out=None, loss_index=0):
        """One train step on device int32 index tensors.  Returns the device loss scalar (no host sync).
        loss_out / loss_index: write the step's loss to element `loss_index` of this fp32 device tensor instead (a training
        loop that reads its losses once per epoch never waits for a step)."""
        if loss_out is not None:
            lp = C.c_void_p(loss_out.data_ptr() + 4 * int(loss_index))
        else:
            lp = _ptr(self._loss) if want_loss else None
        _ffi.check(self.h, self.lib.bprx_step(self.h, _ptr(user), _ptr(pos), _ptr(neg), user.numel(), lp, _stream()))
        return self._loss if loss_out is None else loss_out

    def step_lr(self):
        """The bias-corrected learning rate of the step begun last (bprx_step_lr; sgd: lr)."""
        v = C.c_float()
        _ffi.check(self.h, self.lib.bprx_step_lr(self.h, C.byref(v)))
        return v.value

    def step_begin(self, user, pos, neg):
        _ffi.check(self.h, self.lib.bprx_step_begin(self.h, _ptr(user), _ptr(pos), _ptr(neg), user.numel(), _stream()))

    def step_begin_sparse(self, user, pos, neg):
        """First half of step_begin (the user-side gradients are final afterwards); the index tensors must stay alive and
        unchanged until step_begin_dense has been called."""
        self._pend_idx = (user, pos, neg)
        _ffi.check(self.h, self.lib.bprx_step_begin_sparse(self.h, _ptr(user), _ptr(pos), _ptr(neg), user.numel(), _stream()))

    def step_begin_dense(self):
        _ffi.check(self.h, self.lib.bprx_step_begin_dense(self.h, _stream()))
        self._pend_idx = None

    def dense_grad(self):
        """fp32 view of the handle-owned dense gradient buffer [D*d + D] (dE then dBp) for the RCCL all-reduce."""
        p, n = C.c_void_p(), C.c_int64()
        _ffi.check(self.h, self.lib.bprx_dense_grad(self.h, C.byref(p), C.byref(n)))
        if n.value == 0:
            return None
        if getattr(self, "_dense_view", None) is None:
            self._dense_view = _DevView(p.value, n.value, self.device).tensor
        return self._dense_view

    def item_proj(self):
        """fp32 view [I, PS] of the handle-owned item projections (bprx_item_proj: what the last forward projection wrote)."""
        p, n = C.c_void_p(), C.c_int64()
        _ffi.check(self.h, self.lib.bprx_item_proj(self.h, C.byref(p), C.byref(n)))
        return None if n.value == 0 else _DevView(p.value, n.value, self.device).tensor.view(self.I, n.value // self.I)

    def step_project(self):
        _ffi.check(self.h, self.lib.bprx_step_project(self.h, _stream()))

    def user_grad(self):
        """Zero-copy views [U,k], [U,d] of the staging tables that hold the exported user-row gradients."""
        if getattr(self, "_ugrad", None) is None:
            a, b = C.c_void_p(), C.c_void_p()
            _ffi.check(self.h, self.lib.bprx_user_grad(self.h, C.byref(a), C.byref(b)))
            g = _DevView(a.value, self.U * self.k, self.device).tensor.view(self.U, self.k)
            t = _DevView(b.value, self.U * self.d, self.device).tensor.view(self.U, self.d) if self.d else None
            self._ugrad = (g, t)
        return self._ugrad

    # ---- replicated-user multi-GPU step (include/bprx.h: bprx_pack_user_msg / bprx_apply_user_msgs) -------------
    def user_msg_floats(self, cap):
        return int(self.lib.bprx_user_msg_floats(self.h, int(cap)))

    def pack_user_msg(self, user, cap, msg):
        _ffi.check(self.h, self.lib.bprx_pack_user_msg(self.h, _ptr(user), user.numel(), int(cap), _ptr(msg), _stream()))

    def apply_user_msgs(self, msgs, nranks, cap, scale):
        _ffi.check(self.h, self.lib.bprx_apply_user_msgs(self.h, _ptr(msgs), int(nranks), int(cap), float(scale), _stream()))

    def sum_dense_parts(self, parts, nranks):
        _ffi.check(self.h, self.lib.bprx_sum_dense_parts(self.h, _ptr(parts), int(nranks), _stream()))

    def item_grad(self):
        """Zero-copy views [I,k], [I] of the staging tables that hold the exported item-row gradients."""
        if getattr(self, "_igrad", None) is None:
            a, b = C.c_void_p(), C.c_void_p()
            _ffi.check(self.h, self.lib.bprx_item_grad(self.h, C.byref(a), C.byref(b)))
            self._igrad = (_DevView(a.value, self.I * self.k, self.device).tensor.view(self.I, self.k),
                           _DevView(b.value, self.I, self.device).tensor)
        return self._igrad

    def clear_item_grad(self, n_rows):
        _ffi.check(self.h, self.lib.bprx_clear_item_grad(self.h, int(n_rows), 0, _stream()))

    def clear_user_grad(self, n_rows):
        _ffi.check(self.h, self.lib.bprx_clear_user_grad(self.h, int(n_rows), 0, _stream()))

    def clear_item_marks(self, n_rows):
        """After bprx_route_pack (which returns the exported gradient rows to zero): only the touched-row marks are left."""
        _ffi.check(self.h, self.lib.bprx_clear_item_grad(self.h, int(n_rows), 1, _stream()))

    def clear_user_marks(self, n_rows):
        _ffi.check(self.h, self.lib.bprx_clear_user_grad(self.h, int(n_rows), 1, _stream()))

    def step_end(self, want_loss=True, loss_out=None, loss_index=0):
        """loss_out / loss_index: as in step() -- the loss lands in element `loss_index` of a device tensor."""
        if loss_out is not None:
            lp = C.c_void_p(loss_out.data_ptr() + 4 * int(loss_index))
        else:
            lp = _ptr(self._loss) if want_loss else None
        _ffi.check(self.h, self.lib.bprx_step_end(self.h, lp, _stream()))
        return self._loss if loss_out is None else loss_out

    def score_block(self, u0, u1, out=None):
        if out is None:
            out = torch.empty((u1 - u0, self.I), dtype=torch.float32, device=self.device)
        _ffi.check(self.h, self.lib.bprx_score_block(self.h, u0, u1, _ptr(out), _stream()))
        return out

    def eval_users(self, u0, u1, scores, train_csr, eval_csr, K):
        """bprx_eval_users: per-user (hr, prec, rec, auc, ndcg) as a float64 device tensor [(u1-u0), 5]."""
        out = torch.empty((u1 - u0, 5), dtype=torch.float64, device=self.device)
        _ffi.check(self.h, self.lib.bprx_eval_users(self.h, u0, u1, _ptr(scores), _ptr(train_csr[0]), _ptr(train_csr[1]),
                                                    _ptr(eval_csr[0]), _ptr(eval_csr[1]), int(K), _ptr(out), _stream()))
        return out

    # ---- item-sharded evaluation: counts that are additive over item shards (include/bprx.h) ----------------------
    def eval_pos(self, u0, u1, scores, item_lo, items_total, eval_csr):
        sp = torch.empty((u1 - u0, 32), dtype=torch.float32, device=self.device)
        _ffi.check(self.h, self.lib.bprx_eval_pos(self.h, u0, u1, _ptr(scores), int(item_lo), int(items_total),
                                                  _ptr(eval_csr[0]), _ptr(eval_csr[1]), _ptr(sp), _stream()))
        return sp

    def eval_counts(self, u0, u1, scores, item_lo, items_total, train_csr, eval_csr, sp):
        counts = torch.empty((u1 - u0, 65), dtype=torch.int32, device=self.device)
        _ffi.check(self.h, self.lib.bprx_eval_counts(self.h, u0, u1, _ptr(scores), int(item_lo), int(items_total),
                                                     _ptr(train_csr[0]), _ptr(train_csr[1]), _ptr(eval_csr[0]),
                                                     _ptr(eval_csr[1]), _ptr(sp), _ptr(counts), _stream()))
        return counts

    def eval_finish(self, u0, u1, items_total, eval_csr, sp, counts, K):
        out = torch.empty((u1 - u0, 5), dtype=torch.float64, device=self.device)
        _ffi.check(self.h, self.lib.bprx_eval_finish(self.h, u0, u1, int(items_total), _ptr(eval_csr[0]), _ptr(sp), _ptr(counts),
                                                     int(K), _ptr(out), _stream()))
        return out

    def _topk_out(self, n, K):
        """The outputs of the three top-K entries: (idx int32 [n, K], val fp32 [n, K], flag int32 [n]); K <= 0 is left to the
        library to reject."""
        return (torch.empty((n, max(K, 0)), dtype=torch.int32, device=self.device),
                torch.empty((n, max(K, 0)), dtype=torch.float32, device=self.device),
                torch.empty(n, dtype=torch.int32, device=self.device))

    def topk(self, u0, u1, scores, train_csr, K):
        """bprx_topk: masks the train items IN `scores` and returns (idx int32 [n,K], val fp32 [n,K], flag int32 [n])."""
        idx, val, flag = self._topk_out(u1 - u0, int(K))
        _ffi.check(self.h, self.lib.bprx_topk(self.h, u0, u1, _ptr(scores), _ptr(train_csr[0]), _ptr(train_csr[1]), int(K),
                                              _ptr(idx), _ptr(val), _ptr(flag), _stream()))
        return idx, val, flag

    def profile(self, on):
        _ffi.check(self.h, self.lib.bprx_profile_enable(self.h, 1 if on else 0))

    def profile_read(self):
        """{phase: (total_ms, launches)} accumulated since the last read (HIP events on the launch stream)."""
        ms = np.zeros(len(_ffi.PHASES), np.float64)
        n = np.zeros(len(_ffi.PHASES), np.int64)
        _ffi.check(self.h, self.lib.bprx_profile_read(self.h, ms.ctypes.data, n.ctypes.data))
        return {p: (float(ms[i]), int(n[i])) for i, p in enumerate(_ffi.PHASES) if n[i]}

    def sync_check(self):
        _ffi.check(self.h, self.lib.bprx_sync_check(self.h, _stream()))


def scatter_add(table, idx, rows, scale):
    """table[idx] += scale * rows on the device (bprx_scatter_add); duplicates in idx are summed."""
    lib = _ffi.lib()
    assert table.is_contiguous() and rows.is_contiguous() and idx.dtype == torch.int32 and table.dtype == torch.float32
    ncols = table.shape[1] if table.dim() == 2 else 1
    rc = lib.bprx_scatter_add(_ptr(table), table.shape[0], ncols, _ptr(idx), _ptr(rows), idx.numel(), float(scale), _stream())
    if rc < 0:
        raise _ffi.BprxError(rc, "bprx_scatter_add failed")


def adam_rows(p, m, v, g, lr_t, beta1=0.9, beta2=0.999, eps=1e-7):
    """One adam_tf23 step of a whole row shard from its summed gradient table g (returned to zero): bprx_adam_rows."""
    lib = _ffi.lib()
    assert all(t.is_contiguous() and t.dtype == torch.float32 and t.numel() == p.numel() for t in (p, m, v, g))
    rc = lib.bprx_adam_rows(_ptr(p), _ptr(m), _ptr(v), _ptr(g), p.numel(), float(lr_t), float(beta1), float(beta2), float(eps),
                            _stream())
    if rc < 0:
        raise _ffi.BprxError(rc, "bprx_adam_rows failed")


class _DevView:
    """Zero-copy torch view of library-owned device memory via __cuda_array_interface__."""

    def __init__(self, ptr, n, device):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<f4", "data": (ptr, False), "version": 2}
        self.tensor = torch.as_tensor(self, device=device)


class PhiloxSampler:
    """bprx_sample_philox: device-side stateless throughput sampler over a CSR of training interactions."""

    def __init__(self, train_lists, num_items, device=None, seed=0):
        self.lib = _ffi.lib()
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        indptr = np.zeros(len(train_lists) + 1, dtype=np.int64)
        for u, l in enumerate(train_lists):
            indptr[u + 1] = indptr[u] + len(l)
        items = np.fromiter((i for l in train_lists for i in sorted(l)), dtype=np.int32, count=int(indptr[-1]))
        pos_user = np.repeat(np.arange(len(train_lists), dtype=np.int32), np.diff(indptr))
        self.num_pos, self.num_items, self.seed, self.next = int(indptr[-1]), int(num_items), int(seed), 0
        if self.num_pos == 0:
            raise ValueError("no training interactions")
        full = [u for u, l in enumerate(train_lists) if len(l) >= num_items and len(set(l)) >= num_items]
        if full:
            raise ValueError("user %d holds every item as a positive: it has no negative to sample" % full[0])
        self.indptr, self.items, self.pos_user = (torch.as_tensor(a, device=self.device) for a in (indptr, items, pos_user))

    @classmethod
    def from_csr(cls, indptr, items_sorted, pos_user, num_items, seed=0):
        """Device tensors: indptr int64 [U+1], items_sorted int32 [N] (ascending inside each user), pos_user int32 [N]."""
        self = cls.__new__(cls)
        self.lib = _ffi.lib()
        self.device = indptr.device
        self.indptr, self.items, self.pos_user = indptr.contiguous(), items_sorted.contiguous(), pos_user.contiguous()
        self.num_pos, self.num_items, self.seed, self.next = int(items_sorted.numel()), int(num_items), int(seed), 0
        lens = self.indptr[1:] - self.indptr[:-1]
        if self.num_pos and int(lens.max()) >= self.num_items:       # only then can a list hold every item: count distinct ids
            it = self.items.long()
            new = torch.ones_like(it, dtype=torch.int64)
            new[1:] = (it[1:] != it[:-1]) | (self.pos_user[1:] != self.pos_user[:-1])
            distinct = torch.zeros(lens.numel(), dtype=torch.int64, device=self.device).index_add_(0, self.pos_user.long(), new)
            full = torch.nonzero(distinct >= self.num_items).flatten()
            if full.numel():
                raise ValueError("user %d holds every item as a positive: it has no negative to sample" % int(full[0]))
        return self

    def feeds(self, engine):
        """Name the engine whose steps consume this sampler's batches (bprx_sample_*_h): the sampler then also leaves the byte
        planes of the item ids that engine's index pass scans (segment mode, <= 65 536 items).  Returns self."""
        self._handle = engine.h if engine is not None else None
        return self

    # ---- hard negatives (include/bprx.h bprx_sample_*_hard; DESIGN §9 "Hard negatives") ----
    def hard(self, engine, candidates):
        """Every negative becomes the best-scored of `candidates` (1..16) draws under the engine's model as stored (BPRMF, VBPR,
        GradFashion); the user and the positive stay the uniform stream's, candidates == 1 is the uniform stream.  Implies
        feeds(engine).  Returns self."""
        self.feeds(engine)
        self._engine, self._hard, self.snapshot, self._snapped = engine, int(candidates), None, False
        return self

    def refresh(self):
        """bprx_hard_snapshot: the item projections the candidates are scored with (VBPR: `snapshot`, fp32 [I, proj_stride], a
        tensor this sampler owns) are made again from the tables as they are now.  BPRMF has none; the call is then a check."""
        eng = self._engine
        if eng.d and self.snapshot is None:
            self.snapshot = torch.zeros((eng.I, eng.proj_stride()), dtype=torch.float32, device=self.device)
        _ffi.check(eng.h, self.lib.bprx_hard_snapshot(eng.h, _ptr(self.snapshot), _stream()))
        self._snapped = True

    def _hard_args(self, B, want_candidates):
        """(candidates, Ps, cand, score) of one hard sample of B triplets; the first one takes the snapshot."""
        if not self._snapped:
            self.refresh()
        C_ = self._hard
        cand = torch.empty((B, C_), dtype=torch.int32, device=self.device) if want_candidates else None
        score = torch.empty((B, C_), dtype=torch.float32, device=self.device) if want_candidates else None
        return C_, self.snapshot, cand, score

    @property
    def position(self):
        """The stream position of the next sample()."""
        return self.next

    def seek(self, position):
        """Continue at stream position `position`; nothing is drawn."""
        self.next = int(position)

    def skip(self, B):
        """Advance the stream by B triplets without drawing them (a resumed run's fast-forward)."""
        self.seek(self.position + int(B))

    def sample(self, B, first=None, out=None, want_candidates=False):
        """B triplets starting at stream position `first` (default: continue).  Returns int32 device tensors (u, i, j); a hard
        sampler asked for want_candidates returns (u, i, j, cand int32 [B, C], score fp32 [B, C]): what it drew and compared."""
        if first is None:
            first, self.next = self.next, self.next + B
        u, i, j = out if out is not None else tuple(torch.empty(B, dtype=torch.int32, device=self.device) for _ in range(3))
        if getattr(self, "_hard", 0):
            C_, ps, cand, score = self._hard_args(B, want_candidates)
            _ffi.check(self._handle, self.lib.bprx_sample_philox_hard(
                self._handle, _ptr(self.indptr), _ptr(self.items), _ptr(self.pos_user), self.num_pos, self.num_items, self.seed,
                first, B, _ptr(u), _ptr(i), _ptr(j), 0, B, _stream(), C_, _ptr(ps), _ptr(cand), _ptr(score)))
            return (u, i, j, cand, score) if want_candidates else (u, i, j)
        if want_candidates:
            raise ValueError("want_candidates needs a hard sampler: call hard(engine, candidates) first")
        rc = self.lib.bprx_sample_philox_h(getattr(self, "_handle", None), _ptr(self.indptr), _ptr(self.items), _ptr(self.pos_user),
                                           self.num_pos, self.num_items, self.seed, first, B, _ptr(u), _ptr(i), _ptr(j), 0, B,
                                           _stream())
        if rc < 0:
            raise _ffi.BprxError(rc, "bprx_sample_philox failed")
        return u, i, j


class EpochWalkSampler(PhiloxSampler):
    """bprx_sample_epoch: the reference's visiting order as a device stream -- per epoch a fresh permutation of the users
    (a keyed Feistel permutation evaluated on the device, bprx_epoch_prepare), every positive of every user exactly once,
    consecutively; negatives by Philox rejection.  Batches are user-grouped like the reference's."""

    def _prepare(self, epoch):
        """Everything epoch `epoch` needs, ENQUEUED without a host synchronisation or an upload: the user order is a keyed Feistel
        permutation evaluated pointwise on the device (bprx_epoch_prepare: slot -> user and the length of its list; CPU twin: the
        oracle's orc_epoch_perm), the prefix sums of the lengths are one device scan, the position -> slot map one more launch
        (bprx_epoch_slots).  Prepared ONE EPOCH AHEAD, so that an epoch switch inside a training loop is a pointer swap.
        (History: until round 3 the permutation was drawn on the host and copied synchronously at every epoch start -- bench.py's
        20-step timed regions cannot hide a host stall; an asynchronous pinned-memory upload behind a deep launch queue was worse:
        intermittent 25-80 ms stalls; then the stable argsort of per-user Philox keys on the device: exact, but a merge sort of 8
        launches inside a preparation of 23 launches and 158 us per epoch = 5 us per C2 step.)"""
        U = self.indptr.numel() - 1
        perm_d = torch.empty(U, dtype=torch.int32, device=self.device)
        lens = torch.empty(U, dtype=torch.int64, device=self.device)
        rc = self.lib.bprx_epoch_prepare(self.seed, epoch, U, _ptr(self.indptr), _ptr(perm_d), _ptr(lens), _stream())
        if rc < 0:
            raise _ffi.BprxError(rc, "bprx_epoch_prepare failed")
        epoch_ptr = torch.zeros(U + 1, dtype=torch.int64, device=self.device)
        torch.cumsum(lens, 0, out=epoch_ptr[1:])
        # position -> slot of its user in the epoch order, once per epoch (4 B per interaction): saves the per-triplet
        # binary search over epoch_ptr in the kernel
        pos_slot = torch.empty(self.num_pos, dtype=torch.int32, device=self.device)
        rc = self.lib.bprx_epoch_slots(_ptr(epoch_ptr), U, _ptr(pos_slot), self.num_pos, _stream())
        if rc < 0:
            raise _ffi.BprxError(rc, "bprx_epoch_slots failed")
        return dict(epoch=epoch, perm=perm_d, epoch_ptr=epoch_ptr, pos_slot=pos_slot)

    def _start_epoch(self, epoch):
        nxt = getattr(self, "_next", None)
        cur = nxt if (nxt is not None and nxt["epoch"] == epoch) else self._prepare(epoch)
        self.perm, self.epoch_ptr, self.pos_slot = cur["perm"], cur["epoch_ptr"], cur["pos_slot"]
        self.epoch, self.pos_in_epoch = epoch, 0
        self._next = self._prepare(epoch + 1)

    @property
    def position(self):
        """The stream position of the next sample(): epoch * interactions + position inside the epoch."""
        return 0 if getattr(self, "perm", None) is None else self.epoch * self.num_pos + self.pos_in_epoch

    def seek(self, position):
        """Continue at stream position `position`; nothing is drawn (the epoch it lies in is prepared if it is another one)."""
        epoch, pos = divmod(int(position), self.num_pos)
        if getattr(self, "perm", None) is None or epoch != self.epoch:
            self._start_epoch(epoch)
        self.pos_in_epoch = pos

    def sample(self, B, first=None, out=None, want_candidates=False):
        if first is not None:
            raise ValueError("the epoch walk is a sequential stream")
        if getattr(self, "perm", None) is None:
            self._start_epoch(0)
        u, i, j = out if out is not None else tuple(torch.empty(B, dtype=torch.int32, device=self.device) for _ in range(3))
        hard = getattr(self, "_hard", 0)
        if want_candidates and not hard:
            raise ValueError("want_candidates needs a hard sampler: call hard(engine, candidates) first")
        if hard:
            C_, ps, cand, score = self._hard_args(B, want_candidates)
        done = 0
        while done < B:
            n = min(B - done, self.num_pos - self.pos_in_epoch)
            if hard:
                _ffi.check(self._handle, self.lib.bprx_sample_epoch_hard(
                    self._handle, _ptr(self.indptr), _ptr(self.items), _ptr(self.perm), _ptr(self.epoch_ptr), _ptr(self.pos_slot),
                    self.indptr.numel() - 1, self.num_items, self.seed, self.epoch, self.pos_in_epoch, n, _ptr(u[done:]),
                    _ptr(i[done:]), _ptr(j[done:]), done, B, _stream(), C_, _ptr(ps),
                    _ptr(cand[done:]) if want_candidates else None, _ptr(score[done:]) if want_candidates else None))
            else:
                rc = self.lib.bprx_sample_epoch_h(getattr(self, "_handle", None), _ptr(self.indptr), _ptr(self.items), _ptr(self.perm),
                                                  _ptr(self.epoch_ptr), _ptr(self.pos_slot), self.indptr.numel() - 1, self.num_items,
                                                  self.seed, self.epoch, self.pos_in_epoch, n, _ptr(u[done:]), _ptr(i[done:]),
                                                  _ptr(j[done:]), done, B, _stream())
                if rc < 0:
                    raise _ffi.BprxError(rc, "bprx_sample_epoch failed")
            done += n
            self.pos_in_epoch += n
            if self.pos_in_epoch >= self.num_pos:
                self._start_epoch(self.epoch + 1)
        return (u, i, j, cand, score) if (hard and want_candidates) else (u, i, j)


class HostSampler:
    """bprx_sampler_*: the reference-compatible host index stream (dataset.py:83-114)."""

    def __init__(self, train_lists, num_items):
        self.lib = _ffi.lib()
        U = len(train_lists)
        indptr = np.zeros(U + 1, dtype=np.int64)
        for u, l in enumerate(train_lists):
            indptr[u + 1] = indptr[u] + len(l)
        items = np.fromiter((i for l in train_lists for i in l), dtype=np.int32, count=int(indptr[-1]))
        self.indptr, self.items = indptr, items
        s = C.c_void_p()
        rc = self.lib.bprx_sampler_create(indptr.ctypes.data, items.ctypes.data, U, num_items, C.byref(s))
        if rc < 0:
            raise _ffi.BprxError(rc, "bprx_sampler_create: invalid training lists (item id out of range?)")
        self.s = s

    def count(self, batch_size, epochs):
        return int(self.lib.bprx_sampler_count(self.s, batch_size, epochs))

    def ref_stream(self, batch_size, epochs, py_seed=0, np_seed=0):
        n = self.count(batch_size, epochs)
        u, i, j = (np.empty(n, np.int32) for _ in range(3))
        got = self.lib.bprx_sampler_ref_stream(self.s, batch_size, epochs, py_seed, np_seed,
                                               u.ctypes.data, i.ctypes.data, j.ctypes.data, n)
        if got < 0:
            raise _ffi.BprxError(int(got), "bprx_sampler_ref_stream failed (a user whose positives cover every item?)")
        return u[:got], i[:got], j[:got]

    def __del__(self):
        try:
            if getattr(self, "s", None):
                self.lib.bprx_sampler_destroy(self.s)
                self.s = None
        except Exception:
            pass
