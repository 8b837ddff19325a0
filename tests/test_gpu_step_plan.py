"""What a step launches, form by form: one VBPR handle walks through every form of the training step (touched-item list,
occurrence segments with and without masked projections, a step on a current projection cache, a step after bprx_step_project,
the split-phase calls, B = 1, the empty batch of a replicated rank) and after every call of the walk the per-phase launch
counts of the profiler, bprx_index_pass_kind and bprx_proj_mask_kind must be the ones in WALKS below.

WALKS was recorded with scripts/record_step_plan.py from the library as it was before the step was planned in one place
(plan_step, csrc/bprx_internal.h; the record is profiles/step_plan_walk_parent.jsonl): the planner must launch what the
scattered decisions launched.  The numbers are checked as well: the tables against the CPU oracle after every step, at the
tolerances test_gpu_listmode.test_mode_switches_from_step_to_step uses for these shapes (its shapes, its batches).

Shapes: U = 200, I = 1000, k = 32, d = 20, D = 256, max_batch = 1024: list mode below B = 500, segments from there."""
import pytest
import torch

import test_gpu_listmode as lm
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

U, I, K, DD, D, MAXB = 200, 1000, 32, 20, 256, 1024
REG = 1e-3
# the library's switches at their defaults, whatever the environment of the run says
ENV = {"BPRX_LIST_MODE": "1", "BPRX_ITEM_MODE": "1", "BPRX_PROJ_MASK": "1", "BPRX_SIDE_STREAM": "1", "BPRX_FWD_VARIANT": "4"}
WALK = (("step", 128), ("step", 1024), ("step", 64), ("score",), ("step", 1024), ("project",), ("step", 400), ("split", 1024),
        ("step", 1), ("step", 1024))
# exported user gradients: every step in phases, the user rows through a one-rank message; an empty batch in the middle
WALK_EXPORT = (("split", 128), ("split", 1024), ("split", 64), ("score",), ("split", 1024), ("split", 0), ("project",),
               ("split", 400), ("split", 1), ("split", 1024))
CASES = [(dtype, form, False) for form in ("sgd", "lazy", "swept") for dtype in ("bf16", "fp32")] + [("bf16", "lazy", True)]
IDS = ["%s-%s%s" % (d, f, "-export" if x else "") for d, f, x in CASES]


def walk(setenv, dtype, form, export):
    """Runs the walk; returns one line per call: the call, the launches per phase since the last line, the two kinds."""
    for n, v in ENV.items():
        setenv(n, v)
    setenv("BPRX_ADAM_LAZY", "0" if form == "swept" else "1")
    opt = "sgd" if form == "sgd" else "adam_tf23"
    lr = 0.05 if opt == "sgd" else 0.01
    t = lm._tables(U, I, K, DD, D, seed=8, dtype=dtype)
    e = lm._engine(model="vbpr", num_users=U, num_items=I, embed_k=K, embed_d=DD, feat_dim=D, feat_dtype=dtype, optimizer=opt, lr=lr,
                   reg=REG, max_batch=MAXB, export_user_grad=export).bind(**t)
    assert e.adam_is_lazy() == (form == "lazy")
    o = orc.OracleModel(**t, quant=lm.QUANT[dtype])
    rt, at = (2e-5, 2e-6) if dtype == "fp32" else (2e-3, 1e-4)
    if opt != "sgd":
        at = max(at, 2e-3 * lr)
    of, oa = (0.0, 0.0) if dtype == "fp32" else ((1e-3, 3 * lr) if opt != "sgd" else (3e-2, 1e-2 * lr))
    msg = torch.zeros(e.user_msg_floats(U), dtype=torch.float32, device="cuda") if export else None
    e.profile(True)
    lines = []
    for n, call in enumerate(WALK_EXPORT if export else WALK):
        if call[0] == "score":
            e.score_block(0, U)
        elif call[0] == "project":
            e.step_project()
        else:
            B = call[1]
            if dtype != "fp32":
                lm._resync(o, e, opt)
            u, i, j = lm._batch(U, I, max(B, 32), 70 + n)
            u, i, j = u[:B], i[:B], j[:B]
            du, di, dj = lm._dev(u), lm._dev(i), lm._dev(j)
            loss = None
            if call[0] == "step":
                loss = e.step(du, di, dj).item()
            elif export:
                e.step_begin_sparse(du, di, dj)
                e.step_begin_dense()
                e.pack_user_msg(du, U, msg)                 # (the message carries dE|dBp: after the dense half)
                e.apply_user_msgs(msg, 1, U, -lr)
                e.step_end(want_loss=False)
            else:
                e.step_begin_sparse(du, di, dj)
                e.step_begin_dense()
                loss = e.step_end().item()
            want = o.step(u, i, j, opt, lr, REG)
            if loss is not None:
                assert loss == pytest.approx(want, rel=1e-4 if dtype != "fp32" else 2e-5), (n, call)
            for name in ("Gu", "Gi", "Bi", "Tu", "E", "Bp"):
                lm._close(e.t[name].cpu().numpy().reshape(-1), getattr(o, name).reshape(-1), rt, at, "%s, call %d %s" % (name, n, call),
                          of, oa)
        prof = e.profile_read()
        lines.append("%s %s idx=%d mask=%d" % ("".join(str(c) for c in call), " ".join("%s=%d" % (p, prof[p][1]) for p in sorted(prof)),
                                                e.lib.bprx_index_pass_kind(e.h), e.lib.bprx_proj_mask_kind(e.h)))
    e.sync_check()
    e.close()
    return lines


WALKS = {
    "bf16-sgd": [
        "step128 apply=1 cast_Et=1 dense_update=1 loss_reduce=1 proj_bwd=1 proj_fwd=1 row_count=1 triplet_grad=1 idx=0 mask=0",
        "step1024 dense_update=1 item_seg=1 loss_reduce=1 proj_bwd=1 proj_fwd=1 row_count=1 triplet_grad=1 idx=1 mask=1",
        "step64 apply=1 dense_update=1 loss_reduce=1 proj_bwd=1 proj_fwd=1 row_count=1 triplet_grad=1 idx=1 mask=0",
        "score proj_fwd=1 idx=1 mask=0",
        "step1024 dense_update=1 item_seg=1 loss_reduce=1 proj_bwd=1 row_count=1 triplet_grad=1 idx=1 mask=0",
        "project proj_fwd=1 idx=1 mask=0",
        "step400 apply=1 dense_update=1 loss_reduce=1 proj_bwd=1 row_count=1 triplet_grad=1 idx=1 mask=0",
        "split1024 dense_update=1 item_seg=1 loss_reduce=1 proj_bwd=1 proj_fwd=1 reduce_parts=1 row_count=1 triplet_grad=1 idx=1 mask=1",
        "step1 apply=1 dense_update=1 loss_reduce=1 proj_bwd=1 proj_fwd=1 row_count=1 triplet_grad=1 idx=1 mask=0",
        "step1024 dense_update=1 item_seg=1 loss_reduce=1 proj_bwd=1 proj_fwd=1 row_count=1 triplet_grad=1 idx=1 mask=1",
    ],
    "fp32-sgd": [
        "step128 apply=1 dense_update=1 loss_reduce=1 proj_bwd=1 proj_fwd=1 row_count=1 triplet_grad=1 idx=0 mask=0",
        "step1024 dense_update=1 item_seg=1 loss_reduce=1 proj_bwd=1 proj_fwd=1 row_count=1 triplet_grad=1 idx=1 mask=0",
        "step64 apply=1 dense_update=1 loss_reduce=1 proj_bwd=1 proj_fwd=1 row_count=1 triplet_grad=1 idx=1 mask=0",
        "score proj_fwd=1 idx=1 mask=0",
        "step1024 dense_update=1 item_seg=1 loss_reduce=1 proj_bwd=1 row_count=1 triplet_grad=1 idx=1 mask=0",
        "project proj_fwd=1 idx=1 mask=0",
        "step400 apply=1 dense_update=1 loss_reduce=1 proj_bwd=1 row_count=1 triplet_grad=1 idx=1 mask=0",
        "split1024 dense_update=1 item_seg=1 loss_reduce=1 proj_bwd=1 proj_fwd=1 row_count=1 triplet_grad=1 idx=1 mask=0",
        "step1 apply=1 dense_update=1 loss_reduce=1 proj_bwd=1 proj_fwd=1 row_count=1 triplet_grad=1 idx=1 mask=0",
        "step1024 dense_update=1 item_seg=1 loss_reduce=1 proj_bwd=1 proj_fwd=1 row_count=1 triplet_grad=1 idx=1 mask=0",
    ],
    "bf16-lazy": [
        "step128 adam_catchup=1 apply=1 cast_Et=1 dense_update=1 loss_reduce=1 proj_bwd=1 proj_fwd=1 row_count=1 triplet_grad=1 idx=0 mask=0",
        "step1024 adam_catchup=1 apply=1 dense_update=1 item_seg=1 loss_reduce=1 proj_bwd=1 proj_fwd=1 row_count=1 triplet_grad=1 idx=1 mask=1",
        "step64 adam_catchup=1 apply=1 dense_update=1 loss_reduce=1 proj_bwd=1 proj_fwd=1 row_count=1 triplet_grad=1 idx=1 mask=0",
        "score proj_fwd=1 idx=1 mask=0",
        "step1024 adam_catchup=1 apply=1 dense_update=1 item_seg=1 loss_reduce=1 proj_bwd=1 row_count=1 triplet_grad=1 idx=1 mask=0",
        "project proj_fwd=1 idx=1 mask=0",
        "step400 adam_catchup=1 apply=1 dense_update=1 loss_reduce=1 proj_bwd=1 triplet_grad=1 idx=1 mask=0",
        "split1024 adam_catchup=1 apply=1 dense_update=1 item_seg=1 loss_reduce=1 proj_bwd=1 proj_fwd=1 reduce_parts=1 row_count=1 triplet_grad=1 idx=1 mask=1",
        "step1 adam_catchup=1 apply=1 dense_update=1 loss_reduce=1 proj_bwd=1 proj_fwd=1 row_count=1 triplet_grad=1 idx=1 mask=0",
        "step1024 adam_catchup=1 apply=1 dense_update=1 item_seg=1 loss_reduce=1 proj_bwd=1 proj_fwd=1 row_count=1 triplet_grad=1 idx=1 mask=1",
    ],
    "fp32-lazy": [
        "step128 adam_catchup=1 apply=1 dense_update=1 loss_reduce=1 proj_bwd=1 proj_fwd=1 row_count=1 triplet_grad=1 idx=0 mask=0",
        "step1024 adam_catchup=1 apply=1 dense_update=1 item_seg=1 loss_reduce=1 proj_bwd=1 proj_fwd=1 row_count=1 triplet_grad=1 idx=1 mask=0",
        "step64 adam_catchup=1 apply=1 dense_update=1 loss_reduce=1 proj_bwd=1 proj_fwd=1 row_count=1 triplet_grad=1 idx=1 mask=0",
        "score proj_fwd=1 idx=1 mask=0",
        "step1024 adam_catchup=1 apply=1 dense_update=1 item_seg=1 loss_reduce=1 proj_bwd=1 row_count=1 triplet_grad=1 idx=1 mask=0",
        "project proj_fwd=1 idx=1 mask=0",
        "step400 adam_catchup=1 apply=1 dense_update=1 loss_reduce=1 proj_bwd=1 triplet_grad=1 idx=1 mask=0",
        "split1024 adam_catchup=1 apply=1 dense_update=1 item_seg=1 loss_reduce=1 proj_bwd=1 proj_fwd=1 row_count=1 triplet_grad=1 idx=1 mask=0",
        "step1 adam_catchup=1 apply=1 dense_update=1 loss_reduce=1 proj_bwd=1 proj_fwd=1 row_count=1 triplet_grad=1 idx=1 mask=0",
        "step1024 adam_catchup=1 apply=1 dense_update=1 item_seg=1 loss_reduce=1 proj_bwd=1 proj_fwd=1 row_count=1 triplet_grad=1 idx=1 mask=0",
    ],
    "bf16-swept": [
        "step128 apply=1 cast_Et=1 dense_update=1 loss_reduce=1 proj_bwd=1 proj_fwd=1 row_count=1 triplet_grad=1 idx=0 mask=0",
        "step1024 apply=1 dense_update=1 item_seg=1 loss_reduce=1 proj_bwd=1 proj_fwd=1 row_count=1 triplet_grad=1 idx=1 mask=1",
        "step64 apply=1 dense_update=1 loss_reduce=1 proj_bwd=1 proj_fwd=1 row_count=1 triplet_grad=1 idx=1 mask=0",
        "score proj_fwd=1 idx=1 mask=0",
        "step1024 apply=1 dense_update=1 item_seg=1 loss_reduce=1 proj_bwd=1 row_count=1 triplet_grad=1 idx=1 mask=0",
        "project proj_fwd=1 idx=1 mask=0",
        "step400 apply=1 dense_update=1 loss_reduce=1 proj_bwd=1 triplet_grad=1 idx=1 mask=0",
        "split1024 apply=1 dense_update=1 item_seg=1 loss_reduce=1 proj_bwd=1 proj_fwd=1 reduce_parts=1 row_count=1 triplet_grad=1 idx=1 mask=1",
        "step1 apply=1 dense_update=1 loss_reduce=1 proj_bwd=1 proj_fwd=1 row_count=1 triplet_grad=1 idx=1 mask=0",
        "step1024 apply=1 dense_update=1 item_seg=1 loss_reduce=1 proj_bwd=1 proj_fwd=1 row_count=1 triplet_grad=1 idx=1 mask=1",
    ],
    "fp32-swept": [
        "step128 apply=1 dense_update=1 loss_reduce=1 proj_bwd=1 proj_fwd=1 row_count=1 triplet_grad=1 idx=0 mask=0",
        "step1024 apply=1 dense_update=1 item_seg=1 loss_reduce=1 proj_bwd=1 proj_fwd=1 row_count=1 triplet_grad=1 idx=1 mask=0",
        "step64 apply=1 dense_update=1 loss_reduce=1 proj_bwd=1 proj_fwd=1 row_count=1 triplet_grad=1 idx=1 mask=0",
        "score proj_fwd=1 idx=1 mask=0",
        "step1024 apply=1 dense_update=1 item_seg=1 loss_reduce=1 proj_bwd=1 row_count=1 triplet_grad=1 idx=1 mask=0",
        "project proj_fwd=1 idx=1 mask=0",
        "step400 apply=1 dense_update=1 loss_reduce=1 proj_bwd=1 triplet_grad=1 idx=1 mask=0",
        "split1024 apply=1 dense_update=1 item_seg=1 loss_reduce=1 proj_bwd=1 proj_fwd=1 row_count=1 triplet_grad=1 idx=1 mask=0",
        "step1 apply=1 dense_update=1 loss_reduce=1 proj_bwd=1 proj_fwd=1 row_count=1 triplet_grad=1 idx=1 mask=0",
        "step1024 apply=1 dense_update=1 item_seg=1 loss_reduce=1 proj_bwd=1 proj_fwd=1 row_count=1 triplet_grad=1 idx=1 mask=0",
    ],
    "bf16-lazy-export": [
        "split128 adam_catchup=1 apply=1 cast_Et=1 dense_update=1 proj_bwd=1 proj_fwd=1 reduce_parts=1 row_count=1 triplet_grad=1 idx=0 mask=0",
        "split1024 adam_catchup=1 apply=1 dense_update=1 item_seg=1 proj_bwd=1 proj_fwd=1 reduce_parts=1 row_count=1 triplet_grad=1 idx=1 mask=1",
        "split64 adam_catchup=1 apply=1 dense_update=1 proj_bwd=1 proj_fwd=1 reduce_parts=1 row_count=1 triplet_grad=1 idx=1 mask=0",
        "score proj_fwd=1 idx=1 mask=0",
        "split1024 adam_catchup=1 apply=1 dense_update=1 item_seg=1 proj_bwd=1 reduce_parts=1 row_count=1 triplet_grad=1 idx=1 mask=0",
        "split0 adam_catchup=1 dense_update=1 idx=1 mask=0",
        "project proj_fwd=1 idx=1 mask=0",
        "split400 adam_catchup=1 apply=1 dense_update=1 proj_bwd=1 reduce_parts=1 triplet_grad=1 idx=1 mask=0",
        "split1 adam_catchup=1 apply=1 dense_update=1 proj_bwd=1 proj_fwd=1 reduce_parts=1 row_count=1 triplet_grad=1 idx=1 mask=0",
        "split1024 adam_catchup=1 apply=1 dense_update=1 item_seg=1 proj_bwd=1 proj_fwd=1 reduce_parts=1 row_count=1 triplet_grad=1 idx=1 mask=1",
    ],
}


@pytest.mark.parametrize("dtype,form,export", CASES, ids=IDS)
def test_the_walk_launches_what_it_launched_before_the_planner(monkeypatch, dtype, form, export):
    got = walk(monkeypatch.setenv, dtype, form, export)
    want = WALKS["%s-%s%s" % (dtype, form, "-export" if export else "")]
    assert got == want, "\n" + "\n".join("%s %s\n   want %s" % ("  " if g == w else "!=", g, w) for g, w in zip(got, want))
