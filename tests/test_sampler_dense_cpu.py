"""The samplers' negative for users that hold nearly every item, on the CPU twins (oracle/bpr_oracle.c) and the Python
constructors: never a positive (dataset.py:102 draws until it is not), and no sampler for a user holding every item."""
import numpy as np
import pytest

from oracle import oracle as orc


def test_oracle_negatives_of_dense_users_are_never_positives():
    I = 2000
    rs = np.random.RandomState(3)
    lists = [sorted(rs.choice(I, I - m, replace=False).tolist()) for m in (1, 2, 3)] + \
            [sorted(rs.choice(I, 9, replace=False).tolist()) for _ in range(20)]
    lists[2] = sorted(lists[2] + lists[2][::50])             # repeated ids in a list
    sets = [set(l) for l in lists]
    N = sum(len(l) for l in lists)
    for u, i, j in (orc.sample_philox(lists, I, 4, 0, 3 * N),
                    *(orc.sample_epoch(lists, I, 4, e, 0, N) for e in range(3))):
        assert ((0 <= j) & (j < I)).all()
        assert not any(j[k] in sets[u[k]] for k in range(len(u)))
        assert all(i[k] in sets[u[k]] for k in range(len(u)))


def test_sampler_refuses_a_user_holding_every_item():
    from fashionvisualexpl_recommend_amd.engine import EpochWalkSampler, PhiloxSampler
    for cls in (PhiloxSampler, EpochWalkSampler):
        with pytest.raises(ValueError):
            cls([[2, 0, 1, 1], [0]], 3, device="cpu")          # user 0 holds items 0, 1, 2 (one of them twice)
