"""What tests/test_gpu_fp8_codes.py relies on, held without a GPU (the builders: tests/fp8_code_cases.py)."""
import numpy as np
import pytest
import torch

import fp8_code_cases as fc
from oracle import oracle as orc


def test_code_table_matches_torch():
    want = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float().numpy().astype(np.float64)
    assert np.isnan(want[list(fc.NAN_CODES)]).all() and np.isnan(fc.VAL[list(fc.NAN_CODES)]).all()
    assert np.array_equal(fc.VAL[fc.CODES], want[fc.CODES])
    assert np.array_equal(np.signbit(fc.VAL[fc.CODES]), np.signbit(want[fc.CODES]))        # 0x80 is -0
    assert fc.NC == 254 and np.isfinite(fc.VAL[fc.CODES]).all() and len(set(fc.CODES.tolist())) == 254
    assert fc.VAL[fc.ONE] == 1.0 and fc.VAL[0x7e] == 448.0 and fc.VAL[0x01] == 2.0 ** -9 and fc.VAL[0x07] == 7 * 2.0 ** -9


@pytest.mark.parametrize("D", [512, 768])
def test_one_hot_items_put_every_code_at_every_byte_position(D):
    F = fc.feature_codes(D)
    code, col = fc.item_codes(D)
    assert F.shape == (fc.I_ITEMS, D) and fc.I_ITEMS % 32 != 0 and 4000 < fc.I_ITEMS < 4200
    assert ((F != 0).sum(1) <= 1).all()                     # one-hot (code 0x00 is an all-zero row of its own)
    seen = {(int(code[t]), int(col[t]) % 16) for t in range(fc.I_ITEMS) if code[t] >= 0}
    assert seen == {(int(a), p) for a in fc.CODES for p in range(16)}                      # 254 x 16, none skipped
    for t in np.nonzero(code > 0)[0]:
        assert F[t, col[t]] == code[t]
    for w in (128, 256):                                    # every 128- and 256-wide chunk of D holds items
        assert set((col[code >= 0] // w).tolist()) == set(range(D // w))
    z = fc.zero_items()
    assert len(z) == fc.LEAD + fc.TAIL and not F[z].any() and (code[z] == -1).all()


@pytest.mark.parametrize("D,d", [(512, 15), (512, 79), (768, 63), (512, 159)])
def test_e_and_bp_hold_every_code_exactly_at_the_scale(D, d):
    cb = fc.eb_codes(D, d)
    E, Bp = fc.eb_tables(D, d)
    EB = np.concatenate([E, Bp[:, None]], 1)
    assert np.array_equal(EB.astype(np.float64) * 2.0 ** fc.J, fc.VAL[cb])                  # exact at the scale
    assert float(np.abs(EB).max()) == 448.0 / 2.0 ** fc.J                                    # sE = 2^J
    sE = np.float32(448.0) / np.float32(np.abs(EB).max())
    assert sE == 2.0 ** fc.J and np.float32(1.0) / (np.float32(fc.FS) * sE) == 1.0 / (fc.FS * 2.0 ** fc.J)
    assert np.array_equal(orc.e4m3_round(EB * sE).astype(np.float64), fc.VAL[cb])           # the image is the table
    for p in range(16):                                     # the B operand: every code at every byte position of a 16-byte piece
        assert set(cb[p::16].ravel().tolist()) == set(fc.CODES.tolist())
    P = fc.forward_expected(D, d)
    assert fc.is_f32(P) and fc.is_f32(fc.scores_of(P))      # products and the score's one add are exact
    code, col = fc.item_codes(D)
    assert (P[fc.zero_items()] == 0).all() and (P[code == 0x80] == 0).all()
    assert int((P != 0).sum()) > 0.95 * 252 * 16 * (d + 1) * 252 / 254


@pytest.mark.parametrize("d", [31, 159, 60])
def test_backward_groups_own_their_columns(d):
    D = 512
    seen = set()
    for g in range(fc.n_groups()):
        c = fc.backward_case(g, D, d)
        assert c["B"] <= 512 and len(set(c["i"].tolist())) == c["B"]
        assert not fc.feature_codes(D)[c["j"]].any()        # the negatives are all-zero rows
        assert np.array_equal(np.abs(c["Tu"]) * 8, np.round(np.abs(c["Tu"]) * 8)) and (c["Tu"] != 0).all()
        W = torch.from_numpy(c["W"])
        assert torch.equal(W.float().to(torch.bfloat16).double(), W)                        # W is exact in bf16
        assert fc.is_f32(c["ref"])
        seen |= set(c["i"].tolist())
    code, _ = fc.item_codes(D)
    assert seen == set(np.nonzero(code >= 0)[0].tolist())   # every one-hot item is the positive of exactly one group


def test_cast_probes():
    x = fc.cast_probes()
    want = fc.torch_cast(x)
    got = orc.e4m3_round(x)
    assert np.array_equal(got, want) and np.array_equal(np.signbit(got), np.signbit(want))
    # exactly representable: x / 2^J is a float32 number and comes back as x under sE = 2^J
    E, Bp, X = fc.probe_tables(x, 512, 15)
    EB = np.concatenate([E, Bp[:, None]], 1)
    assert np.array_equal(EB * np.float32(2.0 ** fc.J), X) and np.array_equal(EB.astype(np.float64) * 2.0 ** fc.J, X.astype(np.float64))
    assert set(X[:, :15].ravel().view(np.uint32).tolist()) == set(x.view(np.uint32).tolist())   # every probe is in E
    assert float(np.abs(EB).max()) == 448.0 / 2.0 ** fc.J
    # every code 0x00 .. 0x7e is hit in both signs
    codes = torch.from_numpy(x).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    assert set(codes.tolist()) == set(fc.CODES.tolist())
    # every one of the 126 boundaries, with a neighbour on either side, in both signs
    assert len(fc.MIDPOINTS) == 126
    xs = set(x.view(np.uint32).tolist())
    for k, m in enumerate(fc.MIDPOINTS):
        assert m == (fc.VAL[k] + fc.VAL[k + 1]) / 2.0
        lo, hi = np.nextafter(m, np.float32(-np.inf)), np.nextafter(m, np.float32(np.inf))
        for s in (1.0, -1.0):
            for v in (lo, m, hi):
                assert int(np.float32(s * v).view(np.uint32)) in xs
        even = k if k % 2 == 0 else k + 1                   # a tie goes to the even code
        assert fc.torch_cast(np.array([lo, m, hi], np.float32)).tolist() == [fc.VAL[k], fc.VAL[even], fc.VAL[k + 1]]
    assert fc.torch_cast(np.array([2.0 ** -10, 3 * 2.0 ** -10], np.float32)).tolist() == [0.0, 2.0 ** -8]
    below = np.nextafter(np.float32(2.0 ** -6), np.float32(0))
    assert below in x and fc.torch_cast(np.array([below])).tolist() == [2.0 ** -6]
    assert fc.is_f32(fc.probe_expected(want[np.arange(512 * 15) % len(x)].reshape(512, 15)))


@pytest.mark.parametrize("place", fc.MAX_PLACES, ids=[p[0] for p in fc.MAX_PLACES])
def test_one_maximum_per_placement(place):
    x = fc.cast_probes(with_max=False)
    assert float(np.abs(x).max()) < 448.0
    D, d = 512, 15
    E, Bp, X = fc.probe_tables(x, D, d, place)
    EB = np.concatenate([E, Bp[:, None]], 1)
    hit = np.abs(EB) == 448.0 / 2.0 ** fc.J
    assert int(hit.sum()) == 1                              # a maximum that misses this entry changes sE
    r, c = (int(v[0]) for v in np.nonzero(hit))
    _, tab, idx, sign = place
    assert (c == d) == (tab == "Bp") and r == idx[0] % D and EB[r, c] == sign * 448.0 / 2.0 ** fc.J
    if tab == "E":
        assert c == idx[1] % d
    if place[0] == "Bp-last":
        assert (r, c) == (D - 1, d)                         # the last element k_absmax reads
    assert np.array_equal(EB * np.float32(2.0 ** fc.J), X)
    Xq = fc.torch_cast(X)
    assert np.array_equal(orc.e4m3_round(X), Xq)
    assert fc.is_f32(fc.probe_expected(Xq))                 # a score beside the Bp maximum adds two code values: exact
    second = np.sort(np.abs(EB).ravel())[-2]
    assert not float(np.float32(448.0) / np.float32(second)).is_integer()                  # the scale without it is no power of two


def test_bf16_probes():
    x = fc.bf16_probes()
    want = torch.from_numpy(x.copy()).to(torch.bfloat16).float().numpy()
    assert np.array_equal(orc.bf16_round(x), want)
    u = x.view(np.uint32)
    assert np.isfinite(x).all() and (((u >> 23) & 0xff) >= 1).all() and (((want.view(np.uint32) >> 23) & 0xff) >= 1).all()   # normal
    ties = (u & 0xffff) == 0x8000
    down = ties & (((u >> 16) & 1) == 0)
    up = ties & (((u >> 16) & 1) == 1)
    assert down.sum() >= 8 and up.sum() >= 8
    assert np.array_equal(want.view(np.uint32)[down], u[down] & 0xffff0000)
    assert np.array_equal(want.view(np.uint32)[up], (u[up] & 0xffff0000) + 0x10000)
    carry = up & (((u >> 16) & 0x7f) == 0x7f)
    assert carry.sum() >= 2 and (((want.view(np.uint32)[carry] >> 23) & 0xff) == ((u[carry] >> 23) & 0xff) + 1).all()
    for t in u[ties]:                                       # both float32 neighbours of every tie
        assert t - 1 in u and t + 1 in u
    E, Bp, X = fc.probe_tables(x, 256, 15, scale=1.0)
    assert np.array_equal(E, X[:, :15]) and not Bp.any()
    assert set(E.ravel().view(np.uint32).tolist()) == set(u.tolist())
