"""The seeded shapes of the hard-negative tests (a helper module, not a test module), shared by the CPU and the GPU tier.

(U, I, k, d, C, B), the smallest at which each part can go wrong:
  k1       k = 1, the largest C, a short last workgroup (B = 255)
  odd      odd k and d (the scalar row reads), one triplet past a workgroup (B = 257)
  bench    the float4 row reads at the bench's k = d = 64, several workgroups
  dense    users 0..2 hold all but 1 / 2 / 3 of 37 items (user 2 with repeated ids): candidates c >= 1 are rejected many times; k = 200
  plane9   65 537 items: byte planes with shift 9, no owner queues
  fallback user 0 holds all but 1 of 2 000 items: 60 % of its candidates exhaust the 1 024 attempts (at 37 items a run of 1 024
           positives has probability (36/37)^1024 ~ 1e-12: "dense" never gets there)
Every set of lists but the last has between B and 4 B interactions, so that five batches cross an epoch boundary of the epoch walk."""
import numpy as np

SHAPES = {
    "k1": (64, 300, 1, 0, 16, 255),
    "odd": (64, 300, 5, 3, 5, 257),
    "bench": (500, 2000, 64, 64, 8, 1024),
    "dense": (64, 37, 200, 0, 16, 256),
    "plane9": (64, 65_537, 8, 0, 4, 512),
    "fallback": (64, 2000, 8, 0, 4, 256),
}
FEAT_DIM = {"odd": 128, "bench": 256}                        # D of the VBPR shapes
SEED = 2024                                                  # the samplers' seed


def lists_of(name):
    """The training lists (ascending item ids per user) of a shape."""
    U, I, _, _, _, B = SHAPES[name]
    rs = np.random.RandomState(sum(map(ord, name)))
    if name == "fallback":
        lists = [np.sort(rs.choice(I, I - 1, replace=False)).tolist()]
        lists += [sorted(rs.choice(I, 5, replace=False).tolist()) for _ in range(U - 1)]
    elif name == "dense":
        lists = []
        for u, missing in enumerate((1, 2, 3)):
            keep = np.sort(rs.choice(I, I - missing, replace=False))
            if u == 2:
                keep = np.sort(np.concatenate([keep, keep[::9]]))
            lists.append(keep.tolist())
        lists += [sorted(rs.choice(I, 8, replace=False).tolist()) for _ in range(U - 3)]      # 109 + 61 * 8 = 597 interactions
    else:
        per = max(2, (5 * B) // (2 * U))
        lists = [sorted(set(rs.choice(I, per, replace=False).tolist())) for _ in range(U)]
        lists[0] = sorted(set(lists[0]) | {0, I - 1})
        if I > 65_536:
            lists[1] = sorted(set(lists[1]) | {65_535, 65_536})
    return lists


def tables_of(name, seed=3):
    """fp32 tables (Gu, Gi, Bi and, with d > 0, Tu, F, E, Bp; F scaled to max |F| = 1) of a shape."""
    from fashionvisualexpl_recommend_amd import synth
    U, I, k, d, _, _ = SHAPES[name]
    rs = np.random.RandomState(seed)
    t = dict(Gu=synth.glorot_uniform(rs, U, k), Gi=synth.glorot_uniform(rs, I, k), Bi=(rs.standard_normal(I) * 0.01).astype(np.float32))
    if d:
        D = FEAT_DIM[name]
        F = synth.make_features(I, D, seed=seed)
        t.update(Tu=synth.glorot_uniform(rs, U, d), F=(F / np.abs(F).max()).astype(np.float32), E=synth.glorot_uniform(rs, D, d),
                 Bp=synth.glorot_uniform(rs, D, 1).reshape(-1))
    return t
