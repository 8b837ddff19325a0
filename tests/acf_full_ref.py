"""The FULL gradient of ACF's step: tests/acf_ref.py's restatement with g'_u built inside the graph (once per distinct user of
the batch), so that float64 autograd differentiates the reference's loss through both attention levels.  Everything else --
forward, loss, regulariser, optimizers -- is inherited.  `dtype=torch.float32` runs the same restatement in float32: its
deviation from float64 is the unit of the GPU tests' tolerances.  The instance records the smallest |relu input| it has met
(`min_relu`): a relu input that float32 and float64 put on different sides of zero would show as a gradient error that is nobody's
bug, so every comparison first asserts that this stays above RELU_DELTA.

Also here: the inputs of tests/test_gpu_acf_full.py, so that tests/test_acf_full_cpu.py can check them without a GPU."""
import numpy as np
import torch

from acf_ref import ACFRef, random_tables
from fashionvisualexpl_recommend_amd._ffi import ACF_WEIGHTS

# Smallest |relu input| a compared run may contain.  The float32 restatement's relu inputs deviate from float64 by at most ~1e-6 on
# these inputs (test_acf_full_cpu.py asserts <= RELU_DELTA / 10 on every case), the GPU forward's profiles by <= 1e-5 in g'_u.
RELU_DELTA = 2e-5
# Allowed multiple of the float32 restatement's deviation.  That deviation is ONE sample of float32 rounding; the GPU computes the
# same sums in other orders: sequential 32-row chunks inside a split-K slice where torch sums pairwise (error ~ sqrt(n) eps against
# ~ log(n) eps: up to ~8x at n = 10^4 terms), float atomics in arrival order, expf / division within 1-2 ulp where the CPU's are
# correctly rounded.  32 covers these with the sample's own spread (AttentiveFashion's tests use 4-30x for fixed-order kernels).
TOL_MULT = 32.0
NAMES = ("Gu", "Gi", "Pi") + tuple(ACF_WEIGHTS)
B1_NAMES = ("component.b_1", "item.b_1")


class ACFFullRef(ACFRef):
    def __init__(self, tables, F, reg=0.0, dtype=torch.float64):
        super().__init__(tables, F, reg)
        self.dtype = dtype
        if dtype != torch.float64:
            self.p = {n: v.to(dtype) for n, v in self.p.items()}
            self.F = self.F.to(dtype)
        self.min_relu = float("inf")
        self.relu_inputs = None                 # a list collects every relu input (float64 numpy) when set to []

    def _see(self, x):
        if x.numel():
            self.min_relu = min(self.min_relu, float(x.detach().abs().min()))
            if self.relu_inputs is not None:
                self.relu_inputs.append(x.detach().double().reshape(-1).numpy().copy())

    def profile(self, u, hist, p=None):         # ACFRef.profile, with the two relu inputs observed
        p = self.p if p is None else p
        g_u = p["Gu"][u]
        if len(hist) == 0:
            return g_u.clone()
        h = torch.as_tensor(list(hist), dtype=torch.long)
        f_i = self.F[h]
        b = p["component.W_0_u"].T @ g_u + torch.tensordot(f_i, p["component.W_0_i"], dims=([2], [0])) + p["component.b_0"]
        self._see(b)
        b = torch.relu(b)
        b = torch.tensordot(b, p["component.W_1"], dims=([2], [1])) + p["component.b_1"]
        beta = torch.softmax(b.squeeze(-1), dim=1)
        x_l = (beta.unsqueeze(2) * f_i).sum(1)
        g_i, p_i = p["Gi"][h], p["Pi"][h]
        a = (p["item.W_0_u"].T @ g_u + g_i @ p["item.W_0_iv"] + p_i @ p["item.W_0_ip"] + x_l @ p["item.W_0_ix"]
             + p["item.b_0"])
        self._see(a)
        a = torch.relu(a) @ p["item.W_1"].T + p["item.b_1"]
        alpha = torch.softmax(a.reshape(-1), dim=0)
        return g_u + (alpha.unsqueeze(1) * p_i).sum(0)

    def loss_of(self, leaves, batch, lists):
        u, i, j = (torch.as_tensor(np.asarray(x)).long() for x in batch)
        prof = {uu: self.profile(uu, lists[uu], leaves) for uu in sorted(set(u.tolist()))}     # once per distinct user
        gp = torch.stack([prof[int(x)] for x in u])
        xp = (gp * leaves["Gi"][i]).sum(1)
        xn = (gp * leaves["Gi"][j]).sum(1)
        res = torch.clamp(xp - xn, -80.0, 1e8)
        loss = torch.nn.functional.softplus(-res).sum()
        reg = sum((leaves[n] ** 2).sum() for n in ACF_WEIGHTS)
        reg = reg + (leaves["Gu"][u] ** 2).sum() + (leaves["Gi"][i] ** 2).sum() + (leaves["Gi"][j] ** 2).sum() \
            + (leaves["Pi"][i] ** 2).sum() + (leaves["Pi"][j] ** 2).sum()
        return loss + self.reg * reg

    def grads(self, batch, lists):
        """(loss, {name: gradient}) of one step with NOTHING detached."""
        leaves = {n: v.clone().requires_grad_(True) for n, v in self.p.items()}
        loss = self.loss_of(leaves, batch, lists)
        g = torch.autograd.grad(loss, list(leaves.values()), allow_unused=True)
        return loss.item(), {n: (torch.zeros_like(self.p[n]) if gr is None else gr) for n, gr in zip(leaves, g)}


def features(rs, I, M, C, dtype):
    F = (np.abs(rs.standard_normal((I, M, C))) * (rs.random_sample((I, M, C)) < 0.5)).astype(np.float32)
    return torch.as_tensor(F).bfloat16().float().numpy() if dtype == "bf16" else F


def lists_of(rs, I, lens):
    return [sorted(rs.choice(I, n, replace=n > I).tolist()) if n else [] for n in lens]


# ---- the inputs of tests/test_gpu_acf_full.py (seeds picked on the CPU so that min |relu input| > RELU_DELTA) -----------------
SPECIAL_SEEDS = {"fp32": 101, "bf16": 101}


def special_case(dtype, seed=None):
    """Empty, duplicated, shared and 3 000-item histories, duplicated users in the batch."""
    rs = np.random.RandomState(SPECIAL_SEEDS[dtype] if seed is None else seed)
    U, I, M, C, k, h, a, B = 10, 24, 4, 64, 16, 32, 32, 48
    t = random_tables(rs, U, I, k, C, h, a, scale=10.0)
    F = features(rs, I, M, C, dtype)
    lists = lists_of(rs, I, [0, 1, 2, 3000, 5, 24, 7, 1, 0, 3])
    lists[4] = [3, 3, 3, 9, 9]                                      # duplicated history items
    lists[6] = list(lists[5][:7])                                   # shared with user 5
    batch = (rs.randint(0, U, B), rs.randint(0, I, B), rs.randint(0, I, B))
    batch[0][:4] = [3, 3, 8, 0]                                     # the long history twice, both empty ones
    return t, F, lists, batch


SHAPES = [  # M, C, k, h, a  (tests/test_gpu_acf.py's grid)
    (1, 200, 16, 64, 64), (9, 512, 128, 64, 64), (49, 512, 16, 32, 48), (49, 2048, 128, 64, 64), (196, 200, 16, 64, 64),
]
GRID_SEEDS = {((49, 2048, 128, 64, 64), "fp32"): 8, ((49, 2048, 128, 64, 64), "bf16"): 8,
              ((196, 200, 16, 64, 64), "fp32"): 14, ((196, 200, 16, 64, 64), "bf16"): 10}      # every other case: 7


def grid_case(shape, dtype, seed=None):
    M, C, k, h, a = shape
    rs = np.random.RandomState(GRID_SEEDS.get((shape, dtype), 7) if seed is None else seed)
    U, I, B = 6, 12, 16
    t = random_tables(rs, U, I, k, C, h, a, scale=10.0)
    F = features(rs, I, M, C, dtype)
    lists = lists_of(rs, I, [2, 0, 3, 1, 2, 3])
    batch = (rs.randint(0, U, B), rs.randint(0, I, B), rs.randint(0, I, B))
    return t, F, lists, batch


ADAM_SEEDS = {0.0: 5, 0.05: 5}
ADAM_STEPS, ADAM_LR, ADAM_B = 20, 1e-3, 24


def adam_case(reg, seed=None):
    rs = np.random.RandomState(ADAM_SEEDS[reg] if seed is None else seed)
    U, I, M, C, k, h, a = 16, 24, 4, 64, 16, 16, 16
    t = random_tables(rs, U, I, k, C, h, a, scale=10.0)
    F = features(rs, I, M, C, "fp32")
    lists = lists_of(rs, I, rs.randint(0, 6, U))
    batches = [(rs.randint(0, U, ADAM_B), rs.randint(0, I, ADAM_B), rs.randint(0, I, ADAM_B)) for _ in range(ADAM_STEPS)]
    return t, F, lists, batches


def run_sgd(t, F, lists, batch, reg, lr, dtype):
    """One sgd step of the restatement -> (loss, tables as float64 numpy, min |relu input|)."""
    ref = ACFFullRef(t, F, reg=reg, dtype=dtype)
    loss = ref.step(batch, lists, "sgd", lr)
    return loss, {n: ref.p[n].double().numpy() for n in NAMES}, ref.min_relu


def run_adam(t, F, lists, batches, reg, lr, dtype):
    ref = ACFFullRef(t, F, reg=reg, dtype=dtype)
    losses = [ref.step(b, lists, "adam_tf23", lr) for b in batches]
    return losses, {n: ref.p[n].double().numpy() for n in NAMES}, ref.min_relu


def allowances(t64, t32):
    """Per table: TOL_MULT x the float32 restatement's max-abs deviation from float64."""
    return {n: TOL_MULT * float(np.abs(t32[n] - t64[n]).max()) for n in NAMES}
