"""The inputs of tests/test_gpu_attentive_shapes.py, built on the host so that tests/test_af_step_cases_cpu.py can hold what the
GPU test relies on before any GPU run (a helper module, not a test module; the pattern of tests/af_item_fold_cases.py).

Per case (k, h): tables = attentive_ref.random_tables with Gu x 4 and edges.W2 x 4 (so that the attention moves), inputs =
attentive_ref.random_inputs over I distinct images, batches with repeated users, an item on both sides, one triplet twice and one
i == j triplet (case SAME_ITEM: every one of the 2B rows names one item, a single owner row), the dropout masks RESTATED on the
host (tests/af_dropout_ref.py, the seed tests/test_gpu_attentive.py::_engine binds with, rate 0.5), and the restatements of one
sgd step (float64, float32, float64 with alpha detached) and, for ADAM_CASES, of three adam_tf23 steps (float64, float32), each
with the pre-activations of its three relu layers and its gradients recorded.  Batches stay at B <= 40: the loss is a sum over the
batch, so the float32 restatement's own deviation from float64 grows with B and passes the project's 1e-6 near B = 256.

LIMITS lists shapes on both sides of the three conditions of bprx_bind_attentive."""
import numpy as np
import torch

from af_dropout_ref import dropout_masks
from attentive_ref import AF_WEIGHTS, AttentiveRef, random_inputs, random_tables

TENSORS = ("Gu", "Gi") + tuple(AF_WEIGHTS)
SEED, RATE = 7, 0.5                                          # the dropout stream's seed (test_gpu_attentive._engine) and rate
SGD = dict(optimizer="sgd", lr=0.05, reg=0.05, steps=1)
ADAM = dict(optimizer="adam_tf23", lr=1e-3, reg=0.05, steps=3)
B1, B2, EPS = 0.9, 0.999, 1e-7
T_EXPOSED = 32.0 * EPS / np.sqrt(1.0 - B2)                   # 1.0e-4: below it Adam's first steps turn a gradient's sign into +-lr
ATTENTION_SEES = ("Gu", "color.W1", "color.W2", "edges.W2", "class.W2", "edges.conv")

# what each case crosses:
#   (128, 64): the default widths; two lane passes and two GEMM tiles in k; Dc three M tiles (the last partial), Dk two; R = 80:
#              two row tiles, two ballot rounds
#   (100, 96): k and h no multiples of 64 or 16: partial second lane pass in both, partial N tile, k_af_block<3>
#   (120, 128): ceil(k/8) 8 x ceil(h/32) 32 = 15 360 exactly; R = 14 and 6B = 42 no multiples of 4 or 16; a wave of the last
#              workgroup leaves at b >= B
#   (480, 32): the other end of the same limit; eight lane passes in k; 56.8 KB of dynamic LDS in k_af_triplet
#   (5, 7):    k < 8 and h < 32: the padded, non-float4 path of k_af_block; single partial tiles everywhere
CASES = {(128, 64): dict(Dc=130, Dk=70, B=40, I=12, U=20), (100, 96): dict(Dc=130, Dk=70, B=40, I=12, U=20),
         (120, 128): dict(Dc=37, Dk=11, B=7, I=5, U=6), (480, 32): dict(Dc=70, Dk=20, B=10, I=6, U=6),
         (5, 7): dict(Dc=37, Dk=11, B=7, I=5, U=6)}
ADAM_CASES = [(128, 64), (100, 96)]
SAME_ITEM = (120, 128)
# The seed of each case: the lowest of k, k + 1, ... with which tests/test_af_step_cases_cpu.py holds (no relu kink in reach,
# every tensor moves, a wrong attention backward is visible, at most one Adam element in eight exposed).  The three small cases
# hold with k itself.  The two wide ones have some 21 000 distinct pre-activations a step and the smallest sits near 1.3e-5, 32 x
# the float32 deviation near 2e-5: about one seed in five passes (128 .. 136 and 100, 101 put a unit inside that reach; 128, 132,
# 134, 136 also expose more than an eighth of edges.W2).
SEEDS = {(128, 64): 137, (100, 96): 102, (120, 128): 120, (480, 32): 480, (5, 7): 5}

AF_MAX_H, AF_MAX_K = 128, 512
# (k, h, accepted, the words of the library's message).  The conditions of bprx_bind_attentive, in its order: h <= 128 ("outside"),
# k <= 512 ("embed_k"), ceil(k/8) 8 x ceil(h/32) 32 <= 15 360 and 4 (7k + 6h) 4 <= 65 536 (both "needs more LDS").  With the padded
# width at least 32 the third condition admits k <= 480 only: (512, 8) pads to 512 x 32 = 16 384 and is on the reject side, as
# include/bprx.h documents; (480, 8) is the accepted shape at that edge.
LIMITS = [(120, 128, True, None), (480, 32, True, None), (480, 8, True, None),
          (512, 8, False, "needs more LDS"), (128, 128, False, "needs more LDS"), (488, 32, False, "needs more LDS"),
          (512, 30, False, "needs more LDS"), (513, 8, False, "embed_k"), (16, 129, False, "outside")]


def bind_accepts(k, h):
    """the three conditions of bprx_bind_attentive: None if the shape binds, else the words of its message"""
    if h <= 0 or h > AF_MAX_H:
        return "outside"
    if k > AF_MAX_K:
        return "embed_k"
    if (k + 7) // 8 * 8 * ((h + 31) // 32 * 32) > 15360 or 4 * (7 * k + 6 * h) * 4 > 65536:
        return "needs more LDS"
    return None


class StepRef(AttentiveRef):
    """AttentiveRef that records, per step, the pre-activations of the colour / class hidden layers [2B, 256] and of the attention's
    hidden layer [6B, h] (positives then negatives, as the sample rows) and the gradients; detach_alpha: the score treats
    softmax(a) as a constant (what a missing attention backward computes)."""
    detach_alpha = False

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.pre, self.glog, self._cur = [], [], None

    def encode(self, p, items, masks=None):
        if self._cur is not None:
            it = torch.as_tensor(np.asarray(items)).long()
            self._cur["color"].append((self.color[it] @ p["color.W1"] + p["color.b1"]).detach())
            self._cur["class"].append((self.cls[it] @ p["class.W1"] + p["class.b1"]).detach())
        return super().encode(p, items, masks)

    def score(self, p, gu, gi, enc):
        c = torch.stack(enc, 1)
        pre = (gu.unsqueeze(1) * c) @ p["attention.W_1"] + p["attention.b_1"]
        if self._cur is not None:
            self._cur["attention"].append(pre.detach().reshape(-1, pre.shape[-1]))
        a = torch.relu(pre) @ p["attention.W_2"].reshape(-1, 1) + p["attention.b_2"]
        alpha = torch.softmax(a, 1)
        x = (gu * ((alpha.detach() if self.detach_alpha else alpha) * c).sum(1) * gi).sum(1)
        return x, alpha[:, :, 0]

    def grads(self, batch, masks):
        self._cur = {"color": [], "class": [], "attention": []}
        loss, g = super().grads(batch, masks)
        self.pre.append({n: torch.cat(v).double().numpy() for n, v in self._cur.items()})
        self.glog.append({n: v.double().numpy() for n, v in g.items()})
        self._cur = None
        return loss, g


class DetachedAlphaRef(StepRef):
    detach_alpha = True


def make_batch(rs, U, I, B, same_item=False):
    u, i, j = rs.randint(0, U, B), rs.randint(0, I, B), rs.randint(0, I, B)
    u[1] = u[0]                                              # a repeated user
    j[2] = i[3]                                              # an item on both sides
    u[5], i[5], j[5] = u[4], i[4], j[4]                      # a triplet twice
    j[6] = i[6]                                              # i == j
    if same_item:
        i[:] = I - 1
        j[:] = I - 1                                         # one owner row for all 2B
    return u, i, j


def masks_of(step, n_rows):
    return tuple(torch.as_tensor(m) for m in dropout_masks(SEED, step, n_rows, RATE))


def _run(cls, t, inputs, batches, hp, dtype=torch.float64):
    ref = cls(t, *inputs, reg=hp["reg"], rate=RATE, dtype=dtype)
    B = len(batches[0][0])
    loss = [ref.step(batches[s], masks_of(s, 2 * B), hp["optimizer"], hp["lr"]) for s in range(hp["steps"])]
    return dict(loss=loss, p={n: v.double().numpy() for n, v in ref.p.items()}, pre=ref.pre, grads=ref.glog)


def build(k, h, seed):
    """tables, inputs and batches of one case for a given seed (no restatement run)"""
    c = CASES[(k, h)]
    rs = np.random.RandomState(seed)
    t = random_tables(rs, c["U"], c["I"], k, c["Dc"], c["Dk"], h)
    t["Gu"] = t["Gu"] * 4.0
    t["edges.W2"] = t["edges.W2"] * 4.0
    inputs = random_inputs(rs, c["I"], c["Dc"], c["Dk"])
    batches = [make_batch(rs, c["U"], c["I"], c["B"], (k, h) == SAME_ITEM) for _ in range(ADAM["steps"])]
    return dict(c, k=k, h=h, t=t, inputs=inputs, batches=batches, p0={n: np.asarray(t[n], np.float64) for n in TENSORS})


RUNS = {"sgd64": (StepRef, SGD, torch.float64), "sgd32": (StepRef, SGD, torch.float32), "sgdfix": (DetachedAlphaRef, SGD, torch.float64),
        "adam64": (StepRef, ADAM, torch.float64), "adam32": (StepRef, ADAM, torch.float32)}


def run(c, name):
    """the restatement `name` of RUNS on a built case: made at first use, kept, never changed"""
    if name not in c:
        cls, hp, dtype = RUNS[name]
        c[name] = _run(cls, c["t"], c["inputs"], c["batches"], hp, dtype)
    return c[name]


def sgd_allowance(c, n):
    """(float32 deviation, allowance) of tensor n after the sgd step: max(the project's 1e-6, 4 x the float32 restatement's own
    deviation from float64), the rule of tests/test_gpu_attentive.py for the two conv tensors, here for all fifteen"""
    dev32 = float(np.abs(run(c, "sgd32")["p"][n] - run(c, "sgd64")["p"][n]).max())
    return dev32, max(1e-6, 4.0 * dev32)


def exposed(c, n):
    """bool mask over tensor n: the float64 gradient is non-zero and below T_EXPOSED in any of the Adam steps"""
    g = np.abs(np.stack([s[n] for s in run(c, "adam64")["grads"]]))
    return ((g > 0) & (g < T_EXPOSED)).any(0)


def adam_move_bound(lr, steps):
    """The largest |p_T - p_0| of one element under dense_adam_elem (and adam_elem, the same m and v written differently) in exact
    arithmetic: m_t = (1 - b1) sum_i b1^(t-i) g_i and v_t = (1 - b2) sum_i b2^(t-i) g_i^2, so by Cauchy-Schwarz
    |m_t| <= (1 - b1) sqrt(sum_{j<t} (b1^2 / b2)^j) sqrt(v_t / (1 - b2)), and step t moves the element by
    lr_t |m_t| / (sqrt(v_t) + eps) <= lr sqrt(1 - b2^t) / (1 - b1^t) (1 - b1) / sqrt(1 - b2) sqrt(sum_{j<t} (b1^2 / b2)^j):
    lr, 1.0014 lr, 1.0036 lr for t = 1, 2, 3."""
    r = B1 * B1 / B2
    return sum(lr * np.sqrt(1 - B2 ** t) / (1 - B1 ** t) * (1 - B1) / np.sqrt(1 - B2) * np.sqrt(sum(r ** j for j in range(t)))
               for t in range(1, steps + 1))


_cache = {}


def case(k, h):
    """Everything of one case that needs no GPU, made once and never changed (its restatements: run(case, name))."""
    if (k, h) not in _cache:
        _cache[(k, h)] = build(k, h, SEEDS[(k, h)])
    return _cache[(k, h)]
