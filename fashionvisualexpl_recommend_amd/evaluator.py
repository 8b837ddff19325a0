"""Evaluator: mirror of the reference's src/recommender/Evaluator.py:131-239 (metric definitions :82-128).

Same constructor, `eval(epoch, results, epoch_text, start_time)` and `store_recommendation(path)`; same result
keys (hr_v ... ndcg_t, including the reference's 'auc_t': auc_v aliasing at :220).  Scores come from the
model's predict_all() (libbprx bprx_score_block); the ranking arithmetic below is host NumPy, evaluated on
blocks of users so that U x I is never resident at once.  No multiprocessing Pool (the reference forks one in
the model constructor, Evaluator.py:21; forking after HIP initialisation is not safe).

Metric definitions restated (Evaluator.py:82-128), for user u with train set T, eval items e_1..e_n:
  negatives = all items - T - {e}; position = sum_t #(neg >= score(e_t));
  auc = 1 - position/(|neg| n); top-K = stable descending order of (negatives by ascending id, then e_1..e_n);
  hr = any e in top-K; prec = hits/min(K,|cand|); rec = hits/n; ndcg = ln2/ln(position+2) if position < K else 0.
"""
import contextlib
import datetime
import math
from time import time

import numpy as np

from .ranking import (blocks, lists_to_csr, rank_rows, rank_rows_host, write_because, write_influence, write_capped, write_diverse, write_feature_rows,
                      write_item_lists, write_ranked, write_shelves, style_file, user_style_rows, write_style_items, write_styles,
                      write_user_styles, hist_classed, write_calibrated)


def _eval_block(scores, u0, train, evl, K):
    """Rows of one user block -> list of (hr, prec, rec, auc, ndcg) tuples (users with empty eval lists skipped)."""
    nb, I = scores.shape
    out = []
    cand = np.ones((nb, I), dtype=bool)
    for r in range(nb):
        cand[r, train[u0 + r]] = False
    single = all(len(evl[u0 + r]) <= 1 for r in range(nb))
    if single:
        rows = np.array([r for r in range(nb) if len(evl[u0 + r]) == 1], dtype=np.int64)
        if rows.size == 0:
            return out
        ev = np.array([evl[u0 + r][0] for r in rows], dtype=np.int64)
        c = cand[rows]
        c[np.arange(rows.size), ev] = False
        sp = scores[rows, ev]
        position = ((scores[rows] >= sp[:, None]) & c).sum(axis=1)
        nneg = c.sum(axis=1)
        for p, n in zip(position.tolist(), nneg.tolist()):
            topn = min(K, n + 1)
            hit = 1 if p < topn else 0
            auc = 1 - (p / (n * 1))
            out.append((float(hit), hit / topn, hit / 1, auc, math.log(2) / math.log(p + 2) if p < K else 0))
        return out
    for r in range(nb):
        ev = list(evl[u0 + r])
        if len(ev) == 0:
            continue
        c = cand[r].copy()
        c[ev] = False
        s = scores[r]
        neg = s[c]
        sp = s[ev]
        position = int(sum((neg >= sp[t]).sum() for t in range(len(ev))))
        auc = 1 - (position / (len(neg) * len(ev)))
        topn = min(K, len(neg) + len(ev))
        hits = 0
        for t in range(len(ev)):
            rank = int((neg >= sp[t]).sum()) + sum(1 for q in range(len(ev))
                                                   if q != t and (sp[q] > sp[t] or (sp[q] == sp[t] and q < t)))
            hits += 1 if rank < topn else 0
        out.append((1. if hits > 0 else 0., hits / topn, hits / len(ev), auc,
                    math.log(2) / math.log(position + 2) if position < K else 0))
    return out


class Evaluator:
    def __init__(self, model, data, k, user_block=4096):
        self.data = data
        self.batch_eval = getattr(data.params, "batch_eval", 128)
        self.k = k
        self.model = model
        self.user_block = user_block

    def _user_blocks(self, width=None):
        """ranking.blocks over the model's users, user_block at a time (width: cut for rows of that many scores)."""
        return blocks(self.model.data.num_users, self.user_block, width)

    # ---- device path (libbprx bprx_score_block + bprx_eval_users): used whenever the model runs on the engine ----
    def _device_csr(self, lists, device, dedup=False):
        return lists_to_csr(lists, device, dedup)

    def _metrics_device(self):
        import torch
        eng = self.model.engine
        self._metrics_device_csr()
        rows = {"test": [], "val": []}
        for u0, u1 in self._user_blocks():
            sc = eng.score_block(u0, u1)
            for key in ("test", "val"):
                if self._csr[key] is not None:
                    rows[key].append(eng.eval_users(u0, u1, sc, self._csr["train"], self._csr[key], self.k))
        out = {}
        for key, suf in (("test", "_t"), ("val", "_v")):
            if not rows[key]:
                continue
            r = torch.cat(rows[key]).cpu().numpy()
            if (r[:, 0] == -2).any():
                return None                                # > 32 held-out items for some user: host path
            r = r[r[:, 0] >= 0]
            hr, p, rr, auc, ndcg = r.mean(axis=0).tolist()
            out.update({"hr" + suf: hr, "p" + suf: p, "r" + suf: rr, "auc" + suf: auc, "ndcg" + suf: ndcg})
        return out

    def metrics(self):
        """The ten means of Evaluator.py:189-193 with the TRUE auc_t (eval() applies the reference's aliasing)."""
        if getattr(self.model, "engine", None) is not None and not getattr(self, "force_host", False):
            m = self._metrics_device()
            if m is not None:
                return m
        res_t, res_v = [], []
        val = bool(self.data.validation_list)
        for u0, u1 in self._user_blocks():
            sc = self.model.predict_block(u0, u1)
            res_t += _eval_block(sc, u0, self.data.training_list, self.data.test_list, self.k)
            if val:
                res_v += _eval_block(sc, u0, self.data.training_list, self.data.validation_list, self.k)
        hr_t, p_t, r_t, auc_t, ndcg_t = np.array(res_t).mean(axis=0).tolist()
        out = {"hr_t": hr_t, "p_t": p_t, "r_t": r_t, "auc_t": auc_t, "ndcg_t": ndcg_t}
        if val:
            hr_v, p_v, r_v, auc_v, ndcg_v = np.array(res_v).mean(axis=0).tolist()
            out.update({"hr_v": hr_v, "p_v": p_v, "r_v": r_v, "auc_v": auc_v, "ndcg_v": ndcg_v})
        return out

    def eval(self, epoch=0, results=None, epoch_text='', start_time=0):
        """Evaluator.py:149-223."""
        if results is None:
            results = {}
        eval_start_time = time()
        m = self.metrics()
        z = lambda k_: m.get(k_, 0.0)     # the reference crashes here without a validation set (:179,:195)
        print_results = \
            "%s \tTrain Time: %s \tEvaluation Time: %s" \
            "\nMetrics@%d (Validation)\n\t\tHR\tPrec\tRec\tAUC\tnDCG\n\t\t%f\t%f\t%f\t%f\t%f" \
            "\nMetrics@%d (Test)\n\t\tHR\tPrec\tRec\tAUC\tnDCG\n\t\t%f\t%f\t%f\t%f\t%f\n" % (
                epoch_text,
                datetime.timedelta(seconds=(time() - start_time)),
                datetime.timedelta(seconds=(time() - eval_start_time)),
                self.k, z("hr_v"), z("p_v"), z("r_v"), z("auc_v"), z("ndcg_v"),
                self.k, z("hr_t"), z("p_t"), z("r_t"), z("auc_t"), z("ndcg_t"))
        print(print_results)
        results[epoch] = {
            'hr_v': z("hr_v"), 'auc_v': z("auc_v"), 'p_v': z("p_v"), 'r_v': z("r_v"), 'ndcg_v': z("ndcg_v"),
            'hr_t': z("hr_t"), 'auc_t': z("auc_v"), 'p_t': z("p_t"), 'r_t': z("r_t"), 'ndcg_t': z("ndcg_t")
        }                                   # 'auc_t': auc_v is the reference's own aliasing (Evaluator.py:220)
        return print_results

    def _store_recommendation_device(self, out, block_hook=None):
        """bprx_score_block + bprx_topk per user block, listed by ranking.rank_rows (rows whose list depends on the order of
        EQUAL scores are redone there with numpy) and written by ranking.write_ranked.  block_hook(users, items): called once
        per user block with the (u, item) of the rows just written, in their order."""
        eng = self.model.engine
        self._metrics_device_csr()
        for u0, u1 in self._user_blocks():
            ids, vals, _ = rank_rows(self._topk(u0, u1), eng.score_block(u0, u1), self.k)
            self._write_block(out, range(u0, u1), ids, vals, None, block_hook)

    def _topk(self, u0, u1):
        """bprx_topk over the users [u0, u1) with their train items masked, as ranking.rank_rows calls it."""
        return lambda scores, k: self.model.engine.topk(u0, u1, scores, self._csr["train"], k)

    @staticmethod
    def _write_block(out, labels, ids, vals, side, block_hook):
        written = write_ranked(out, labels, ids, vals, side)
        if block_hook is not None and written[0]:
            block_hook(*written)

    def _metrics_device_csr(self):
        if getattr(self, "_csr", None) is None:
            eng = self.model.engine
            U = self.model.data.num_users
            pad = lambda l: list(l[:U]) + [[] for _ in range(U - len(l))]
            self._csr = {"train": self._device_csr(pad(self.data.training_list), eng.device, dedup=True),
                         "test": self._device_csr(pad(self.data.test_list), eng.device),
                         "val": self._device_csr(pad(self.data.validation_list), eng.device)
                         if self.data.validation_list else None}

    def store_recommendation(self, path=""):
        """Evaluator.py:225-239: per user mask train items, top-k by argsort, 'u\\titem\\tscore' rows."""
        with open(path, 'w') as out:
            self._store_recommendation_rows(out)

    def _store_recommendation_rows(self, out, block_hook=None):
        """The rows of store_recommendation: on the device where the model has an engine and top_k fits bprx_topk, else (or with
        force_host) on the host.  block_hook as in _store_recommendation_device."""
        if getattr(self.model, "engine", None) is not None and not getattr(self, "force_host", False) and self.k <= 1024:
            self._store_recommendation_device(out, block_hook)
            return
        for u0, u1 in self._user_blocks():
            ids, vals = rank_rows_host(self.model.predict_block(u0, u1), self.data.training_list[u0:u1], self.k)
            self._write_block(out, range(u0, u1), ids, vals, None, block_hook)

    def store_recommendation_features(self, path_recs="", path_expl="", top=5):
        """VBPR: `path_recs` exactly as store_recommendation writes it (the same device or host path), and for every row written
        there the rows of ranking.write_feature_rows in `path_expl` (rank below min(top, feature columns); score = base + the sum
        of all the pair's contributions), one bprx_feat_explain call per user block."""
        with open(path_recs, 'w') as out, open(path_expl, 'w') as ex:
            self._store_recommendation_rows(out, lambda users, items: write_feature_rows(ex, users, items,
                                                                                         self.model.explain(users, items, top)))

    def store_recommendation_new(self, path="", features=None, path_expl=None, top=0):
        """VBPR / GradFashion: the top-k NEW items of every user (model.recommend_new: the visual score, nothing masked) as rows
        'u\\tj\\tscore', j = the row of `features` (raw rows, as model.prepare_new_items takes them), best first, formatted as
        store_recommendation formats them.  path_expl with top > 0: also 'u\\tj\\tscore\\trank\\tcolumn\\tcontribution' for
        the same pairs in the same order, rank 0 first, one row per rank below min(top, feature columns); there is no base."""
        m = self.model
        F = m.prepare_new_items(features)
        with open(path, 'w') as out, (open(path_expl, 'w') if path_expl and top > 0 else contextlib.nullcontext()) as ex:
            for u0, u1 in self._user_blocks():
                res = m.recommend_new(F, self.k, u0, u1, explain=top if ex is not None else 0)
                idx, val = res[0], res[1]
                write_ranked(out, range(u0, u1), idx, val)
                if ex is not None and idx.size:
                    write_feature_rows(ex, np.repeat(np.arange(u0, u1), idx.shape[1]), idx.reshape(-1), res[2])

    def store_similar_items(self, path="", space=None):
        """Every catalogue item's nearest neighbours by cosine in `space` (model.similar_items: None = the model's own space, the
        item itself excluded) as rows 'i\tj\tcosine', item by item, best first, formatted as store_recommendation formats."""
        ids, vals = self.model.similar_items(None, None, space)
        with open(path, 'w') as out:
            write_ranked(out, range(ids.shape[0]), ids, vals)

    def store_recommendation_diverse(self, path="", path_ild="", k=None, pool=None, theta=None, space=None):
        """BPRMF / VBPR / GradFashion: every user's diversified list (model.recommend_diverse: greedy MMR over the user's top-`pool`,
        None = the run's --diversify / --diversify_pool / --similar_space) as rows 'u\ti\tscore\tredundancy' in `path`, in list
        order (redundancy = the pick's largest cosine with the picks above it), and one row 'u\tild' per user in `path_ild` (1 -
        the mean pairwise cosine of the list), formatted as store_recommendation formats.  Device only: force_host or
        top_k > 1024 raise ValueError (there is no host MMR)."""
        ids, vals, pen, ild = self.model.recommend_diverse(None, k, pool, theta, space)
        with open(path, 'w') as out, open(path_ild, 'w') as out_ild:
            write_diverse(out, out_ild, range(ids.shape[0]), ids, vals, pen, ild)

    def store_recommendation_calibrated(self, path="", path_kl="", k=None, pool=None, lam=None, alpha=None):
        """BPRMF / VBPR / GradFashion: every user's calibrated list (model.recommend_calibrated: greedy KL re-rank of the user's
        top-`pool` toward the class mix of the user's training items, None = the run's --calibrate / --calibrate_pool /
        --calibrate_alpha) as rows 'u\ti\tscore\tclass\tgain' in `path`, in list order (gain = the KL term the pick removed at its
        step), and one row 'u\tkl_plain\tkl_calibrated\thist_classed' per user in `path_kl` (KL(p || q~) of the plain top_k and of
        the calibrated list; the user's training items that have a class), formatted as store_recommendation formats.  Device
        only: force_host or top_k > 1024 raise ValueError (there is no host form)."""
        ids, vals, cls, gain, kl = self.model.recommend_calibrated(None, k, pool, lam, alpha)
        U = ids.shape[0]
        lists = list(self.data.training_list[:U]) + [[] for _ in range(U - len(self.data.training_list))]
        with open(path, 'w') as out, open(path_kl, 'w') as out_kl:
            write_calibrated(out, out_kl, range(U), ids, vals, cls, gain, kl, hist_classed(lists, self.model.item_classes()))

    def store_recommendation_shelves(self, path="", k=None, count=0):
        """BPRMF / VBPR / GradFashion: every user's shelves (model.recommend_by_class: the k best items of every item class, None =
        the run's --shelves; training items masked) as rows 'u\tclass\ti\tscore' in `path`: user by user, the user's classes
        ordered by their best entry's score (count > 0: only the first `count` of them), each shelf best first, formatted as
        store_recommendation formats.  Device only: force_host raises ValueError (there is no host form)."""
        ids, vals, cnt = self.model.recommend_by_class(None, k)
        with open(path, 'w') as out:
            write_shelves(out, range(ids.shape[0]), ids, vals, cnt, int(count))

    def store_recommendation_capped(self, path="", cap=None):
        """BPRMF / VBPR / GradFashion: every user's quota list (model.recommend_capped: the top_k with at most `cap` items of any one
        class, None = the run's --class_cap) as rows 'u\ti\tscore\tclass' in `path`, best first.  Device only: force_host raises
        ValueError."""
        ids, vals, cls = self.model.recommend_capped(None, None, cap)
        with open(path, 'w') as out:
            write_capped(out, range(ids.shape[0]), ids, vals, cls)

    def store_styles(self, path="", style=None, cos=None, top=None):
        """BPRMF / VBPR / GradFashion: the style files next to the recs-* / best-recs-* file at `path` for the assignment (style int
        [I], cos fp32 [I]) of model.item_styles (None: clustered now with the run's --styles / --style_iters / --similar_space):
        styles-* (rows 'i\tstyle\tcosine', every item in id order, -1 for a zero row), style-items-* (rows 'style\tsize\trank\ti\t
        cosine': every style's `top`, None = --style_top, members nearest its centroid, best first, equal cosines by ascending
        item; model.style_members) and user-styles-* (rows 'u\tstyle\towned\tshare': the styles of every user's training list by
        descending count, then ascending style; share = owned / list length), formatted as store_recommendation formats."""
        if style is None:
            style, cos = self.model.item_styles()[:2]
        with open(style_file(path, "styles"), 'w') as out:
            write_styles(out, style, cos)
        with open(style_file(path, "style-items"), 'w') as out:
            write_style_items(out, *self.model.style_members(style, cos, top))
        with open(style_file(path, "user-styles"), 'w') as out:
            write_user_styles(out, range(self.data.num_users), user_style_rows(self.data.training_list, style))

    def store_styles_new(self, path="", style=None, cos=None):
        """VBPR / GradFashion: new-styles-*, rows 'j_new\tstyle\tcosine' for the rows of the --new_items table (model.styles_of_new)."""
        with open(path, 'w') as out:
            write_styles(out, style, cos)

    def store_recommendation_because(self, path="", top=5, space=None):
        """BPRMF / VBPR / GradFashion: for every (u, i) of every user's top-k list (the lists store_recommendation writes, ranked
        again the same way) the `top` items of the user's training list nearest to i by cosine in `space` (None: the model's own)
        as rows 'u\\ti\\tscore\\trank\\thist_item\\tcosine' in `path` (ranking.write_because).  One bprx_because call per user block
        with the training CSR the lists were masked with.  Device only: force_host or top_k > 1024 raise ValueError."""
        top, space = self.model._because_args(top, space)
        eng = self.model.engine
        self._metrics_device_csr()
        lists = lambda u0, u1: rank_rows(self._topk(u0, u1), eng.score_block(u0, u1), self.k)[:2]
        self._store_because(path, lists, top, space, eng.sim_rnorm(space))

    def store_because_new(self, path="", features=None, top=5):
        """VBPR / GradFashion: store_recommendation_because for the pairs of store_recommendation_new (every user's top-k NEW
        items, j = the row of `features`): the user's training items nearest to the new item in the visual space."""
        m = self.model
        top, _ = m._because_args(top, "visual")
        self._metrics_device_csr()
        F = m.prepare_new_items(features)
        P = m.engine.project_rows(F)
        lists = lambda u0, u1: m.recommend_new(F, self.k, u0, u1)[:2]
        self._store_because(path, lists, top, "visual", m.engine.sim_rnorm("visual"), P, m.engine.sim_rnorm("visual", P))

    def _store_because(self, path, lists, top, space, rn, Pq=None, rn_q=None):
        """The because-* file of the lists (ids, vals) = lists(u0, u1) of every user block: one bprx_because call per block (none
        for a block without a list entry) with the training CSR, rn / Pq / rn_q as Engine.because takes them."""
        import torch
        eng = self.model.engine
        ptr, items = self._csr["train"]
        with open(path, 'w') as out:
            for u0, u1 in self._user_blocks():
                ids, vals = lists(u0, u1)
                if not ids.size:
                    continue
                idx = torch.as_tensor(np.ascontiguousarray(ids, dtype=np.int32), device=eng.device)
                hist, cos, _ = eng.because(space, rn, idx, (ptr[u0:u1 + 1], items), top, Pq, rn_q)
                write_because(out, range(u0, u1), ids, vals, hist.cpu().numpy(), cos.cpu().numpy())

    def store_recommendation_influence(self, path="", top=5, damp=1.0):
        """BPRMF / VBPR / GradFashion: for every (u, i) of every user's top-k list (the lists store_recommendation writes, ranked
        again the same way) the `top` entries of u's training list the score rests on most (bprx_influence on the user's own row)
        as rows 'u\\ti\\tscore\\trank\\thist_item\\tinfluence\\tshare' in `path` (ranking.write_influence).  The pairs of ALL
        users are drawn once, before blocking, by draw_fold_pairs(training lists, num_items, --fold_negatives, --init_seed): a
        user's rows do not depend on the block size.  One bprx_influence call per user block.  Device only: force_host or top_k >
        1024 raise ValueError."""
        import torch
        from .models import draw_fold_pairs
        m = self.model
        top = m._influence_args(top)
        eng = m.engine
        self._metrics_device_csr()
        U = m.data.num_users
        train = self.data.training_list
        negatives = int(getattr(m.params, "fold_negatives", 4))
        ptr, pos, neg = draw_fold_pairs(list(train[:U]) + [[] for _ in range(U - len(train))], m.data.num_items, negatives,
                                        getattr(m.params, "init_seed", 0))
        ptr, pos, neg = (torch.as_tensor(a, device=eng.device) for a in (ptr, pos, neg))
        Gu, Tu = eng.t["Gu"], (eng.t["Tu"] if eng.d else None)
        with open(path, 'w') as out:
            for u0, u1 in self._user_blocks():
                ids, vals = rank_rows(self._topk(u0, u1), eng.score_block(u0, u1), self.k)[:2]
                if not ids.size:
                    continue
                idx = torch.as_tensor(np.ascontiguousarray(ids, dtype=np.int32), device=eng.device)
                e = eng.influence(Gu[u0:u1], None if Tu is None else Tu[u0:u1], ptr[u0:u1 + 1], pos, neg, negatives, idx, top,
                                  reg=m.reg, damp=damp)
                write_influence(out, range(u0, u1), ids, vals, e["item"].cpu().numpy(), e["infl"].cpu().numpy(), e["total"].cpu().numpy())

    def store_similar_new(self, path="", features=None):
        """VBPR / GradFashion: the catalogue neighbours of every row of `features` (raw rows of items outside the catalogue, as
        model.prepare_new_items takes them) in the visual space as rows 'j_new\ti\tcosine', row by row, best first."""
        ids, vals = self.model.similar_to_new(features)
        with open(path, 'w') as out:
            write_ranked(out, range(ids.shape[0]), ids, vals)

    def store_audience(self, path="", items=None):
        """BPRMF / VBPR / GradFashion / AttentiveFashion (rows with the attentions): the audience of every item of `items` (None: the whole catalogue; model.audience: the
        params' K users with the highest score, the item's owners excluded) as rows 'i\tu\tscore', item by item, best first,
        formatted as store_recommendation formats; an item with fewer non-owners than K has that many rows."""
        res = self.model.audience(items)                     # (ids, vals) and, AttentiveFashion, the attentions
        labels = range(res[0].shape[0]) if items is None else [int(i) for i in np.asarray(items).reshape(-1)]
        with open(path, 'w') as out:
            write_item_lists(out, labels, *res)

    def store_audience_new(self, path="", features=None):
        """VBPR / GradFashion: the audience of every row of `features` (raw rows of items outside the catalogue, as
        model.prepare_new_items takes them; model.audience_new: the visual score, nothing masked) as rows 'j\tu\tscore', j = the
        row of `features`, row by row, best first."""
        ids, vals = self.model.audience_new(features)
        with open(path, 'w') as out:
            write_item_lists(out, range(ids.shape[0]), ids, vals)

    def store_recommendation_warm(self, path="", buyers=None, features=None, rows=None, **fold):
        """BPRMF / VBPR / GradFashion / AttentiveFashion (whose rows end in the three attentions): the top-k WARM items of every user (model.recommend_warm: new items whose Gi / Bi rows are
        fitted from buyers[j], the users who bought item j; the ones a user bought are masked) as rows 'u\tj\tscore', j = the row
        of `buyers` (and of `features`, raw rows as model.prepare_new_items takes them), best first, formatted as
        store_recommendation formats them.  rows: what model.fold_in_items returned for these buyers (None: fitted here with
        **fold).  Returns the rows, so that store_audience_warm can read the same fit."""
        m = self.model
        if rows is None:
            rows = m.fold_in_items(buyers, features, **fold)
        res = m._rank_warm_recs(rows, buyers)                # (ids, vals) and, AttentiveFashion, the attentions
        with open(path, 'w') as out:
            write_item_lists(out, range(res[0].shape[0]), *res)
        return rows

    def store_audience_warm(self, path="", buyers=None, features=None, rows=None, **fold):
        """BPRMF / VBPR / GradFashion / AttentiveFashion (rows with the attentions): the audience of every warm item (model.audience_warm: the params' K users with the highest
        score, the item's buyers masked) as rows 'j\tu\tscore', item by item, best first.  rows / **fold as
        store_recommendation_warm takes them."""
        m = self.model
        if rows is None:
            rows = m.fold_in_items(buyers, features, **fold)
        res = m._rank_warm_audience(rows, buyers)
        with open(path, 'w') as out:
            write_item_lists(out, range(res[0].shape[0]), *res)
        return rows

    def store_recommendation_grads(self, path="", path_expl=None, top=5):
        """Evaluator.py:261-275 (GradFashion): for every user the items training_list[u] + validation_list[u] + test_list[u],
        in that order, one row 'u\\ti\\tcolour\\tedges' each (get_explanations.py:19-21 reads USER_ID, ITEM_ID, COLOR, EDGES).
        The attributions come from the device, one bprx_explain_pairs call per block of users.  path_expl: also the rows of
        ranking.write_feature_rows for the same pairs in the same order, one bprx_feat_explain call per block."""
        lists = (self.data.training_list, self.data.validation_list, self.data.test_list)
        with open(path, 'w') as out, (open(path_expl, 'w') if path_expl else contextlib.nullcontext()) as ex:
            for u0, u1 in blocks(self.data.num_users, self.user_block):
                users, items = [], []
                for u in range(u0, u1):
                    pos_items_u = [i for l in lists for i in (l[u] if u < len(l) else [])]
                    users += [u] * len(pos_items_u)
                    items += pos_items_u
                if not items:
                    continue
                g = self.model.engine.explain_pairs(users, items).cpu().numpy()
                for r, (u, i) in enumerate(zip(users, items)):
                    out.write(str(u) + '\t' + str(i) + '\t' + str(g[r, 0]) + '\t' + str(g[r, 1]) + '\n')
                if ex is not None:
                    write_feature_rows(ex, users, items, self.model.explain(users, items, top))

    def store_recommendation_attention(self, path=""):
        """Evaluator.py:241-259 (AttentiveFashion): the top-k rows 'u\\titem\\tscore\\talpha_colour\\talpha_edges\\talpha_class'.
        Scores and attentions come from one bprx_af_score_block call per user block; the top-k and the gather of its
        attentions run on the device, rows whose order depends on equal scores are redone on the host
        (ranking.rank_rows, the attentions as its `side`)."""
        with open(path, 'w') as out:
            self._store_attention_rows(out)

    def _store_attention_rows(self, out, block_hook=None):
        """The rows of store_recommendation_attention; block_hook(users, items) is called once per user block with the rows
        just written, in their order."""
        eng = self.model.engine
        self._metrics_device_csr()
        for u0, u1 in self._user_blocks(width=self.model.data.num_items):
            sc, al = eng.af_score_block(u0, u1)
            ids, vals, att = rank_rows(self._topk(u0, u1), sc, self.k, side=al)
            self._write_block(out, range(u0, u1), ids, vals, att, block_hook)

    def store_recommendation_attention_explain(self, path_recs="", path_expl="", grid=14):
        """AttentiveFashion: `path_recs` exactly as store_recommendation_attention writes it, and for every row written there one row
        'u\\ti\\tscore\\ts_colour\\ts_edges\\ts_class\\tpeak_row\\tpeak_col\\tpeak_value\\tcell_0 ... cell_{G*G-1}' in `path_expl`
        (bprx_af_explain, one call per block of rows): score = s_colour + s_edges + s_class exactly as the model weighs the three
        modalities, and the cells (row-major, G x G over the 112 x 112 pooled edge image) sum to s_edges, alpha held fixed."""
        eng, G = self.model.engine, int(grid)
        with open(path_recs, 'w') as out, open(path_expl, 'w') as ex:
            def block(users, items):
                e = {n: v.cpu().numpy() for n, v in eng.af_explain(users, items, G, maps=True).items()}
                for r, (u, i) in enumerate(zip(users, items)):
                    pc = int(e["peak_cell"][r])
                    ex.write('\t'.join([str(u), str(i), str(e["score"][r])] + [str(v) for v in e["parts"][r]] +
                                       [str(pc // G), str(pc % G), str(e["peak_val"][r])] + [str(v) for v in e["map"][r]]) + '\n')
            self._store_attention_rows(out, block)

    def store_recommendation_acf(self, path_recs="", path_expl="", top=5):
        """ACF: `path_recs` exactly as store_recommendation writes it (the same device or host path), and for every row written there the rows
        'u\\ti\\tscore\\tbase\\trank\\thist_item\\talpha\\tcontribution\\tpeak_m\\tbeta_peak' in `path_expl`: the `top` entries of the
        user's history that contribute most to x_ui = base + sum_l alpha_l (Pi_l . Gi_i), rank 0 first (bprx_acf_explain, one call
        per user block, with the evaluation histories the scores were made with: training + validation, ACF.py:220).  A user
        with an empty history gets one row with rank = hist_item = peak_m = -1 and zeros, so that base is still recorded."""
        eng = self.model.engine
        csr = eng.acf_eval if eng.acf_eval is not None else eng.acf_train
        with open(path_recs, 'w') as out, open(path_expl, 'w') as ex:
            def block(users, items):
                e = {n: v.cpu().numpy() for n, v in eng.acf_explain(users, items, top, csr=csr).items()}
                for r, (u, i) in enumerate(zip(users, items)):
                    head = str(u) + '\t' + str(i) + '\t' + str(e["score"][r]) + '\t' + str(e["base"][r]) + '\t'
                    if e["pos"][r, 0] < 0:
                        ex.write(head + '-1\t-1\t0.0\t0.0\t-1\t0.0\n')
                        continue
                    for s in range(e["pos"].shape[1]):
                        if e["pos"][r, s] < 0:
                            break
                        ex.write(head + str(s) + '\t' + str(e["hist_item"][r, s]) + '\t' + str(e["alpha"][r, s]) + '\t' +
                                 str(e["contrib"][r, s]) + '\t' + str(e["peak"][r, s]) + '\t' + str(e["beta_peak"][r, s]) + '\n')
            self._store_recommendation_rows(out, block)
