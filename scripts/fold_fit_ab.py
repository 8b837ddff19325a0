"""Same bits from two builds of the library for the three row fits of bprx_foldin.hip: bprx_fold_in (new users),
bprx_fold_in_items (warm items) and bprx_af_fold_in_items (AttentiveFashion warm items).

  git worktree add ../parent HEAD~1 && python ../parent/fashionvisualexpl_recommend_amd/build.py
  python scripts/fold_fit_ab.py --parent ../parent/fashionvisualexpl_recommend_amd/libbprx.so \
                                --new fashionvisualexpl_recommend_amd/libbprx.so

_ffi reads BPRX_LIB at import, so each library runs in a fresh child process of its own (this file with --child), under its own
time limit, one after the other; a child that fails ends the script.  A child runs every case on fixed seeded inputs and saves
the fitted rows and the losses; this process compares their bytes and writes one JSON line per case to --out
(profiles/fold_fit_ab.json): {"case", "equal", "row_bytes", "loss_bytes"}.  Exit status 1 if any case differs.

Cases: sgd and adam_tf23; BPRX_FOLD_CACHE 1 (pairs that fit stay in LDS) and 0 (every pair is formed again every step); rows one,
two and five-or-six lane words wide (EPL 1, 2, 6 of k_fold_fit; for the AttentiveFashion fit, whose rows are k wide, also k = 256:
EPL 4).  Every call has rows with 0, 1, NP + 1 and fit + 1 + NP (or one more) pairs -- the empty row, a tail group, a row split
between the LDS form and the per-step form -- and 60 rows of 0 .. 80 random pairs."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = I = 200
EDGE = {1: [0, 1, 5, 45], 2: [0, 1, 5, 25], 4: [0, 1, 5, 14], 6: [0, 1, 3, 9]}     # by EPL: NP 4 / 4 / 4 / 2, fit 39 / 19 / 9 / 6
USER = [(1, 16, 12), (2, 40, 25), (6, 200, 100)]              # (EPL, k, d): rows k + d wide
ITEM = [(1, 16, 12), (2, 64, 20), (6, 256, 20)]               # rows k + 1 wide
AF = [(1, 16), (2, 65), (4, 256), (6, 260)]                   # (EPL, k): rows k wide
OPT = {"sgd": dict(steps=20, lr=0.002, reg=1e-3), "adam_tf23": dict(steps=5, lr=0.05, reg=1e-3)}


def pairs(rs, epl):
    counts = EDGE[epl] + list(rs.randint(0, 81, size=60))
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def child(out_dir):
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from af_item_fold_cost import af_engine, af_tables, random_inputs
    from fashionvisualexpl_recommend_amd.engine import Engine
    torch.cuda.set_device(0)
    dev = lambda x: torch.as_tensor(np.ascontiguousarray(x), device="cuda")
    out = {}

    def keep(name, rows, loss):
        out[name + "/rows"] = np.concatenate([r.cpu().numpy().reshape(len(loss), -1) for r in rows if r is not None], 1)
        out[name + "/loss"] = loss.cpu().numpy()

    def vbpr(rs, k, d):
        n = lambda *s: (rs.standard_normal(s) * 0.3).astype(np.float32)
        F = np.abs(rs.standard_normal((I, 32))).astype(np.float32)
        t = dict(Gu=n(U, k), Gi=n(I, k), Bi=n(I), Tu=n(U, d), F=F / F.max(), E=n(32, d) * 0.2, Bp=n(32) * 0.2)
        return Engine(model="vbpr", num_users=U, num_items=I, embed_k=k, embed_d=d, feat_dim=32, feat_dtype="fp32", optimizer="sgd",
                      lr=0.05, reg=1e-3, max_batch=64).bind(**t)

    for cache in ("1", "0"):
        os.environ["BPRX_FOLD_CACHE"] = cache                 # read when a handle is created
        for epl, k, d in USER:
            rs = np.random.RandomState(1000 + epl)
            e = vbpr(rs, k, d)
            ptr = pairs(rs, epl)
            n, m = len(ptr) - 1, int(ptr[-1])
            pos, neg = (rs.randint(I, size=m).astype(np.int32) for _ in range(2))
            W0 = (rs.standard_normal((n, k + d)) * 0.3).astype(np.float32)
            for opt, hp in OPT.items():
                Gu, Tu = dev(W0[:, :k]), dev(W0[:, k:])
                loss = e.fold_in(ptr, pos, neg, hp["steps"], Gu, Tu, lr=hp["lr"], reg=hp["reg"], optimizer=opt)
                keep("fold_in epl=%d %s cache=%s" % (epl, opt, cache), (Gu, Tu), loss)
            e.sync_check()
            e.close()
        for epl, k, d in ITEM:
            rs = np.random.RandomState(2000 + epl)
            e = vbpr(rs, k, d)
            ptr = pairs(rs, epl)
            n, m = len(ptr) - 1, int(ptr[-1])
            user, other, role = (rs.randint(hi, size=m).astype(np.int32) for hi in (U, I, 2))
            W0 = (rs.standard_normal((n, k + 1)) * 0.3).astype(np.float32)
            Fn = np.abs(rs.standard_normal((n, 32))).astype(np.float32)
            Pn = e.project_rows(Fn / Fn.max())
            for opt, hp in OPT.items():
                Gi, Bi = dev(W0[:, :k]), dev(W0[:, k])
                loss = e.fold_in_items(ptr, user, other, role, hp["steps"], Gi, Bi, Pn, lr=hp["lr"], reg=hp["reg"], optimizer=opt)
                keep("fold_in_items epl=%d %s cache=%s" % (epl, opt, cache), (Gi, Bi), loss)
            e.sync_check()
            e.close()
        for epl, k in AF:
            rs = np.random.RandomState(3000 + k)
            t = af_tables(rs, U, I, k=k, h=32)
            t["Gu"], t["Gi"] = ((rs.standard_normal(s) * 0.3).astype(np.float32) for s in ((U, k), (I, k)))
            e = af_engine(t, random_inputs(rs, I), U, I, optimizer="sgd", B=64, k=k)
            ptr = pairs(rs, epl)
            n, m = len(ptr) - 1, int(ptr[-1])
            user, other, role = (rs.randint(hi, size=m).astype(np.int32) for hi in (U, I, 2))
            W0 = (rs.standard_normal((n, k)) * 0.3).astype(np.float32)
            Cn = e.af_encode_new(*random_inputs(rs, n))
            for opt, hp in OPT.items():
                Gi = dev(W0)
                loss = e.af_fold_in_items(ptr, user, other, role, hp["steps"], Cn, Gi, lr=hp["lr"], reg=hp["reg"], optimizer=opt)
                keep("af_fold_in_items k=%d epl=%d %s cache=%s" % (k, epl, opt, cache), (Gi,), loss)
            e.sync_check()
            e.close()
    np.savez(os.path.join(out_dir, "fits.npz"), **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="the parent commit's libbprx.so")
    ap.add_argument("--new", help="this tree's libbprx.so")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fold_fit_ab.json"))
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    if not a.parent or not a.new:
        ap.error("--parent and --new are both needed")
    fits = {}
    with tempfile.TemporaryDirectory() as tmp:
        for side, lib in (("parent", a.parent), ("new", a.new)):
            d = os.path.join(tmp, side)
            os.mkdir(d)
            env = dict(os.environ, BPRX_LIB=os.path.abspath(lib))
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", d], env=env, timeout=a.timeout).returncode
            if rc != 0:
                sys.exit("fold_fit_ab: the child of the %s library ended with status %d" % (side, rc))
            with np.load(os.path.join(d, "fits.npz")) as z:
                fits[side] = {n: z[n] for n in z.files}
    cases = sorted({n.rsplit("/", 1)[0] for n in fits["parent"]})
    lines, same = [], True
    for c in cases:
        eq = all(fits["parent"][c + part].tobytes() == fits["new"][c + part].tobytes() for part in ("/rows", "/loss"))
        moved = bool(np.isfinite(fits["new"][c + "/rows"]).all() and np.abs(fits["new"][c + "/loss"]).max() > 0)
        same = same and eq and moved
        lines.append({"case": c, "equal": eq, "finite_and_fitted": moved, "row_bytes": int(fits["new"][c + "/rows"].nbytes),
                      "loss_bytes": int(fits["new"][c + "/loss"].nbytes)})
        print(json.dumps(lines[-1]), flush=True)
    with open(a.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
    sys.exit(0 if same else 1)


if __name__ == "__main__":
    main()
