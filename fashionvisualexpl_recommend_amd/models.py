"""BPRMF and VBPR: host-side mirror of the reference's model classes
(src/recommender/RecommenderModel.py:16-25, models/BPRMF.py:21-192, models/VBPR.py:19-144).

Same constructor `Model(data, params)`, same methods (`call`, `predict_all`, `train_step`, `train`) and the same
attribute names (Bi, Gu, Gi, Tu, F, E, Bp, evaluator, directory_parameters).  The tables are torch-ROCm tensors;
every computation on them runs in libbprx.so through the C ABI (include/bprx.h) -- no autograd, no eager
op chain.  `params` may carry three extra knobs the reference does not have:
    optimizer  'adam_tf23' (default: the reference's tf.optimizers.Adam semantics) | 'sgd'
    dtype      'fp32' (default) | 'bf16'   storage/compute type of the frozen feature table F
    init_seed  seed of the Glorot-uniform initialiser (TF's own RNG stream is not reproducible without TF)
"""
import os
import pickle
from time import time

import numpy as np
import torch

from . import configs
from .engine import Engine, as_index
from .evaluator import Evaluator
from .ranking import (because_paths, because_rows, blocks, cal_paths, calibrate_rows, calibrated_zeros, cap_rows, class_csr,
                      class_rows_per_block, diverse_zeros, diversify_rows, div_paths, hist_classed, influence_file, influence_rows,
                      item_file, owners_of, rank_class_rows, rank_rows, ranked_zeros, run_file, shelf_file, style_file, wanted_blocks,
                      warm_file, write_because, write_calibrated, write_capped, write_diverse, write_influence, write_ranked,
                      write_shelves)
from .synth import glorot_uniform


class _Scores:
    """What predict_all() returns: the reference returns a tf.Tensor whose only use is `.numpy()`
    (Evaluator.py:174,231)."""

    def __init__(self, t):
        self.tensor = t

    def numpy(self):
        return self.tensor.cpu().numpy()


def draw_fold_pairs(histories, num_items, negatives, seed):
    """The (positive, negative) pairs of users the model was not trained on, drawn on the host with
    numpy.random.default_rng(seed): users in order, each user's positives in history order, and for each positive `negatives`
    uniform draws over the items that are not in that user's history (by rejection), kept next to each other.  A history that
    covers the catalogue (or is empty) gives no pairs.  Returns (pair_ptr int64 [n + 1], pos int32, neg int32); an id outside
    [0, num_items) raises ValueError."""
    I, negatives = int(num_items), int(negatives)
    if negatives < 1:
        raise ValueError("draw_fold_pairs: negatives = %d < 1" % negatives)
    rng = np.random.default_rng(seed)
    ptr = np.zeros(len(histories) + 1, np.int64)
    pos, neg = [], []
    mask = np.zeros(I, bool)
    for r, hist in enumerate(histories):
        h = np.asarray(list(hist), dtype=np.int64).reshape(-1)
        if h.size and (h.min() < 0 or h.max() >= I):
            raise ValueError("draw_fold_pairs: user %d has an item outside [0, %d)" % (r, I))
        mask[h] = True
        need = 0 if int(mask.sum()) >= I else h.size * negatives
        out = np.empty(need, np.int64)
        filled = 0
        while filled < need:
            c = rng.integers(0, I, size=need - filled)
            c = c[~mask[c]]
            out[filled:filled + c.size] = c
            filled += c.size
        mask[h] = False
        if need:
            pos.append(np.repeat(h, negatives))
            neg.append(out)
        ptr[r + 1] = ptr[r] + need
    cat = lambda parts: (np.concatenate(parts) if parts else np.zeros(0, np.int64)).astype(np.int32)
    return ptr, cat(pos), cat(neg)


def draw_item_fold_pairs(buyers, training_list, num_items, negatives, seed):
    """The pairs of items the model was not trained on, from their first buyers (buyers[r]: the catalogue users who bought new
    item r), drawn on the host with numpy.random.default_rng(seed).  Items are taken in order, each item's buyers deduplicated in
    first-appearance order.
      role 0  the new item is the positive: for each buyer u `negatives` pairs (u, o, 0), o uniform over the catalogue items
              outside training_list[u] (by rejection); a buyer whose list covers the catalogue gives none;
      role 1  the new item is the negative, as often as it was the positive (what training does to an item of average
              popularity; with role 0 alone nothing but the regulariser holds the item's bias down): as many pairs (u', o', 1)
              as the item got in role 0, u' uniform over the users that are not buyers of this item and have a non-empty
              training list (by rejection), o' uniform from training_list[u']; no such user: none.
    Returns (pair_ptr int64 [n + 1], user int32, other int32, role int32), each item's role-0 pairs first; a buyer outside
    [0, len(training_list)) or a listed item outside [0, num_items) raises ValueError."""
    I, U, negatives = int(num_items), len(training_list), int(negatives)
    if negatives < 1:
        raise ValueError("draw_item_fold_pairs: negatives = %d < 1" % negatives)
    lens = np.fromiter((len(l) for l in training_list), dtype=np.int64, count=U)
    tptr = np.zeros(U + 1, np.int64)
    np.cumsum(lens, out=tptr[1:])
    flat = np.fromiter((int(i) for l in training_list for i in l), dtype=np.int64, count=int(tptr[-1]))
    if flat.size and (flat.min() < 0 or flat.max() >= I):
        raise ValueError("draw_item_fold_pairs: a training list has an item outside [0, %d)" % I)
    rng = np.random.default_rng(seed)
    ptr = np.zeros(len(buyers) + 1, np.int64)
    users, others, roles = [], [], []
    owned, is_buyer = np.zeros(I, bool), np.zeros(U, bool)

    def rejected(high, need, bad):
        """`need` uniform draws from [0, high) outside the mask `bad`"""
        out, filled = np.empty(need, np.int64), 0
        while filled < need:
            c = rng.integers(0, high, size=need - filled)
            c = c[~bad[c]]
            out[filled:filled + c.size] = c
            filled += c.size
        return out

    for r, who in enumerate(buyers):
        b = np.asarray(list(dict.fromkeys(int(u) for u in who)), dtype=np.int64)
        if b.size and (b.min() < 0 or b.max() >= U):
            raise ValueError("draw_item_fold_pairs: item %d has a buyer outside [0, %d)" % (r, U))
        n0 = 0
        for u in b:
            mine = flat[tptr[u]:tptr[u + 1]]
            owned[mine] = True
            if int(owned.sum()) < I:
                users.append(np.full(negatives, u, np.int64))
                others.append(rejected(I, negatives, owned))
                roles.append(np.zeros(negatives, np.int64))
                n0 += negatives
            owned[mine] = False
        is_buyer[b] = True
        out_of_play = is_buyer | (lens == 0)
        n1 = n0 if not out_of_play.all() else 0
        if n1:
            up = rejected(U, n1, out_of_play)
            users.append(up)
            others.append(flat[tptr[up] + rng.integers(0, lens[up])])
            roles.append(np.ones(n1, np.int64))
        is_buyer[b] = False
        ptr[r + 1] = ptr[r] + n0 + n1
    cat = lambda parts: (np.concatenate(parts) if parts else np.zeros(0, np.int64)).astype(np.int32)
    return ptr, cat(users), cat(others), cat(roles)


def fold_start_rows(x, n, w, device):
    """The rows a fold-in starts from: zeros [n, w] for x = None, else a contiguous fp32 device copy of x (tensor or array)
    shaped [n, w]; None for a table the model does not have (w == 0)."""
    if w == 0:
        return None
    if x is None:
        return torch.zeros((n, w), dtype=torch.float32, device=device)
    return torch.as_tensor(np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x, dtype=np.float32).reshape(n, w),
                           device=device).contiguous().clone()


class RecommenderModel:
    def __init__(self, data, params):                       # RecommenderModel.py:16-25
        self.data = data
        self.num_items = data.num_items
        self.num_users = data.num_users
        self.params = params
        self.epochs = params.epochs
        self.batch_size = params.batch_size
        self.verbose = getattr(params, "verbose", -1)
        self.restore_epochs = getattr(params, "restore_epochs", 1)
        self.model_name = getattr(params, "rec", None)
        self.dataset_name = getattr(params, "dataset", None)


class BPRMF(RecommenderModel):
    model_kind = "bprmf"

    def __init__(self, data, params, init=None):
        """`init`: optional dict of initial tables (numpy/torch) overriding the seeded Glorot initialiser."""
        super().__init__(data, params)
        self.embed_k = params.embed_k
        self.learning_rate = params.lr
        self.reg = params.reg
        self.optimizer_name = getattr(params, "optimizer", "adam_tf23")
        self.evaluator = Evaluator(self, data, params.top_k)                       # BPRMF.py:40
        self.similar_k = int(getattr(params, "similar_items", 0) or 0)             # neighbours per item in sim-*; 0: none
        self.similar_space = getattr(params, "similar_space", None) or self.sim_space
        self.diversify_theta = float(getattr(params, "diversify", 0.0) or 0.0)     # theta of the div-* files; 0: none
        self.diversify_pool = int(getattr(params, "diversify_pool", 100) or 100)   # candidates per list the MMR step picks from
        self.because_top = int(getattr(params, "because", 0) or 0)                 # owned items per pair in because-*; 0: none
        self.influence_top = int(getattr(params, "influence", 0) or 0)             # history entries per pair in influence-*; 0: none
        self.influence_damp = float(getattr(params, "influence_damp", 1.0))        # the relative damping of bprx_influence
        self.audience_k = int(getattr(params, "audience", 0) or 0)                 # users per item in audience-*; 0: none
        self.shelves_k = int(getattr(params, "shelves", 0) or 0)                   # entries per class in shelf-*; 0: none
        self.shelf_count = int(getattr(params, "shelf_count", 0) or 0)             # shelves per user in shelf-*; 0: all
        self.class_cap = int(getattr(params, "class_cap", 0) or 0)                 # items per class in cap-*; 0: none
        self.calibrate_lambda = float(getattr(params, "calibrate", 0.0) or 0.0)    # lambda of the cal-* files; 0: none
        self.calibrate_pool = int(getattr(params, "calibrate_pool", 100) or 100)   # candidates per list the KL step picks from
        self.calibrate_alpha = float(getattr(params, "calibrate_alpha", 0.01) or 0.01)   # the smoothing of the list's class shares
        self.styles_S = int(getattr(params, "styles", 0) or 0)                     # clusters of the styles-* files; 0: none
        self.style_iters = int(getattr(params, "style_iters", 20) or 20)           # Lloyd iterations at the most
        self.style_top = int(getattr(params, "style_top", 10) or 10)               # members per style in style-items-*
        # hard negatives (--hard_negatives C): every negative is the best-scored of C sampled candidates; 0: the uniform draw
        self.hard_negatives = int(getattr(params, "hard_negatives", 0) or 0)
        self.hard_refresh = int(getattr(params, "hard_refresh", 0) or 0)           # steps between snapshots inside an epoch; 0: none
        if self.hard_negatives and not (2 <= self.hard_negatives <= 16 and self.hard_models):
            raise ValueError("%s: hard_negatives is 0 (off) or 2 .. 16 with BPRMF, VBPR or GradFashion (got %r)"
                             % (type(self).__name__, self.hard_negatives))
        if self.hard_negatives and getattr(params, "sampler", "ref_stream") != "philox":
            raise ValueError("%s: hard_negatives needs the philox sampler" % type(self).__name__)
        if self.hard_refresh < 0 or (self.hard_refresh and not self.hard_negatives):
            raise ValueError("%s: hard_refresh is >= 0 and needs hard_negatives (got %r)" % (type(self).__name__, self.hard_refresh))
        self.directory_parameters = f'batch_{params.batch_size}-K_{params.embed_k}-lr_{params.lr}-reg_{params.reg}' \
                                    + self._hard_suffix()
        self._build(init or {})

    hard_models = True                                           # ACF / AttentiveFashion: False (their scores are not the kernel's)

    def _hard_suffix(self):
        """What a run with hard negatives adds to directory_parameters (uniform runs keep the reference's file names)."""
        return f'-hard_{self.hard_negatives}' if self.hard_negatives else ''

    # ---- parameters (BPRMF.py:48-52) ---------------------------------------------------------------------------
    def _init_tables(self, init):
        rs = np.random.RandomState(getattr(self.params, "init_seed", 0))
        t = {"Bi": np.zeros(self.num_items, np.float32),
             "Gu": glorot_uniform(rs, self.num_users, self.embed_k),
             "Gi": glorot_uniform(rs, self.num_items, self.embed_k)}
        t.update({k: v for k, v in init.items() if k in t})
        return t, rs

    def _engine_kwargs(self):
        return dict(model="bprmf", num_users=self.num_users, num_items=self.num_items, embed_k=self.embed_k)

    def _adam_form(self):
        """adam_tf23 lazily-exact or by whole-table sweeps (identical arithmetic; include/bprx.h BPRX_FLAG_ADAM_*): a row's replay
        is a serial recurrence over the steps since its last touch -- one epoch = interactions / batch steps in the reference's
        visiting order (~0.45 us each, measured: bprx_api.hip) -- against a sweep that moves every row's (p, m, v) once per step.  The library estimates
        this from max_batch; here the batch size and the interaction count are known."""
        if self.optimizer_name != "adam_tf23" or os.environ.get("BPRX_ADAM_LAZY") is not None:
            return None
        kw = self._engine_kwargs()
        n_pos = sum(len(pos) for pos in self.data.training_list)
        chain_us = 0.45 * n_pos / max(1, self.batch_size)
        elems = kw["num_users"] * (kw["embed_k"] + kw.get("embed_d", 0)) + kw["num_items"] * (kw["embed_k"] + 1)
        return "lazy" if chain_us < elems * 24.0 / 4e6 else "sweep"

    def _new_engine(self, min_batch=4096):
        """self.engine for the tables _init_tables has just made (the kwargs and the Adam form are read off them), not yet bound."""
        self.engine = Engine(optimizer=self.optimizer_name, lr=self.learning_rate, reg=self.reg,
                             max_batch=max(self.batch_size, min_batch), adam_form=self._adam_form(), **self._engine_kwargs())
        return self.engine

    def _build(self, init):
        t, _ = self._init_tables(init)
        self._new_engine().bind(**t)
        self._alias()

    def _alias(self):
        """The reference's attribute surface (model.Gu, .Gi, .Bi, .Tu, .F, .E, .Bp) is served by the class properties below:
        they go through engine.t, which first brings every row up to date when adam_tf23 runs lazily (bprx_sync_adam) -- a
        raw alias of the tensor would show rows that have not been replayed yet."""

    # ---- BPRMF.py:55-76 ------------------------------------------------------------------------------------------
    def _pairs(self, inputs):
        """(u, i) of call()'s inputs = (user, item, ...): int64 device tensors, as the tables are indexed."""
        dev = self.engine.device
        return as_index(inputs[0], dev).long(), as_index(inputs[1], dev).long()

    def call(self, inputs, training=None, mask=None):
        u, i = self._pairs(inputs)
        xui = self.engine.score_pairs(u, i)
        return xui, self.Bi[i], self.Gu[u], self.Gi[i]

    __call__ = call

    # ---- BPRMF.py:78-85 --------------------------------------------------------------------------------------------
    def predict_block(self, u0, u1):
        return self.engine.score_block(u0, u1).cpu().numpy()

    def predict_all(self):
        return _Scores(self.engine.score_block(0, self.num_users))

    # ---- BPRMF.py:87-125 -------------------------------------------------------------------------------------------
    def train_step(self, batch):
        user, pos, neg = (as_index(b, self.engine.device) for b in batch)
        return float(self.engine.step(user, pos, neg).item())      # loss.numpy(): one host sync, like the reference

    # ---- state snapshots (the reference deep-copies the whole model, BPRMF.py:156) --------------------------------
    def state_dict(self):
        sd = {n: v.detach().clone() for n, v in self.engine.t.items() if n != "F"}
        sd["adam_step"] = self.engine.adam_step
        return sd

    def load_state_dict(self, sd):
        for n, v in sd.items():
            if n == "adam_step":
                self.engine.adam_step = v
            else:
                self.engine.t[n].copy_(v)
        self.engine.tables_dirty()                      # the handle caches images derived from E/Bp

    def weights_path(self, epoch):
        rec = getattr(self.params, "rec", self.model_kind)
        return os.path.join(configs.weight_dir(), self.params.dataset, rec, f'weights-{epoch}-{self.directory_parameters}.pt')

    # ---- BPRMF.py:127-192 ------------------------------------------------------------------------------------------
    def train(self, resume=False):
        """The reference's training loop.  `resume=True` (the reference parses --restore_epochs but
        never restores, BPRMF.py:130): continue from the snapshot `weights-{restore_epochs}-...pt` -- tables, Adam slots
        and step counter are reloaded and the deterministic triplet stream is fast-forwarded by restore_epochs epochs,
        so the remaining epochs see exactly the batches an uninterrupted run would."""
        max_metrics = {'hr': 0, 'p': 0, 'r': 0, 'auc': 0, 'ndcg': 0}
        best_state = None
        best_epoch = self.restore_epochs
        best_epoch_print = 'No best epoch found!'
        results = {}
        steps_total = (sum(len(pos) for pos in self.data.training_list) // self.params.batch_size) * self.params.epochs
        if getattr(self.params, "sampler", "ref_stream") == "philox":
            # --sampler philox: the device epoch walk (the reference's visiting order as a stateless Philox stream; bit-exact
            # CPU twin in the oracle) instead of the host MT19937 stream -- no index upload per step
            from .engine import EpochWalkSampler
            smp = EpochWalkSampler(self.data.training_list, self.num_items, device=self.engine.device,
                                   seed=getattr(self.params, "init_seed", 0)).feeds(self.engine)
            if self.hard_negatives:
                # --hard_negatives C: the snapshot the candidates are scored with is taken again at the start of every epoch of
                # this loop, and with --hard_refresh N every N steps counted from there (the step is read off the stream's
                # position when the first batch is asked for: a resumed run has skipped to its own by then)
                smp.hard(self.engine, self.hard_negatives)

                def hard_batches(B=self.params.batch_size, spe=max(1, steps_total // max(1, self.params.epochs))):
                    for s in range(smp.position // B, steps_total):
                        if s % spe == 0 or (self.hard_refresh and (s % spe) % self.hard_refresh == 0):
                            smp.refresh()
                        yield smp.sample(B)
                next_batch = hard_batches()
            else:
                next_batch = (smp.sample(self.params.batch_size) for _ in range(steps_total))
        else:
            next_batch = self.data.next_triple_batch(self.engine.device)
        steps = 0
        loss = 0
        it = 1
        steps_per_epoch = sum([len(pos) for pos in self.data.training_list]) // self.params.batch_size
        rec = getattr(self.params, "rec", self.model_kind)
        wdir = os.path.join(configs.weight_dir(), self.params.dataset, rec)
        rdir = os.path.join(configs.results_dir(), self.params.dataset, rec)
        os.makedirs(wdir, exist_ok=True)
        os.makedirs(rdir, exist_ok=True)
        if resume:
            path = self.weights_path(self.restore_epochs)
            self.load_state_dict(torch.load(path, map_location=self.engine.device, weights_only=True))
            if self.hard_negatives:                               # nothing is drawn: the stream position moves (the skipped
                smp.skip(self.restore_epochs * steps_per_epoch * self.params.batch_size)   # batches would be scored by THIS model)
            else:
                for _ in range(self.restore_epochs * steps_per_epoch):
                    next(next_batch)
            it = self.restore_epochs + 1
            print('Restored epoch {0} from {1}'.format(self.restore_epochs, path))
        start_ep = time()
        print('Start training...')
        # (the reference reads loss.numpy() after every step, BPRMF.py:125 -- a host synchronisation per step; here the
        #  step losses land in a device buffer and are read once per epoch, so the host runs ahead of the device)
        loss_buf = torch.zeros(max(1, steps_per_epoch), dtype=torch.float32, device=self.engine.device)
        # (loss_buf outlives every step of this loop, so a step's loss may land one launch later: its dense update then rides in
        #  the next step's index pass; settle() before the buffer is read, and the lag ends with the loop)
        self.engine.set_loss_lag(True)
        try:
            for batch in next_batch:
                steps += 1
                user, pos, neg = (as_index(b, self.engine.device) for b in batch)
                self.engine.step(user, pos, neg, loss_out=loss_buf, loss_index=steps - 1)
                if steps == steps_per_epoch:                                        # epoch is over
                    self.engine.settle()
                    loss = float(loss_buf[:steps].double().sum().item())
                    epoch_text = 'Epoch {0}/{1} \tLoss: {2:.3f}'.format(it, self.params.epochs, loss / steps)
                    epoch_print = self.evaluator.eval(it, results, epoch_text, start_ep)
                    for metric in max_metrics.keys():
                        if max_metrics[metric] <= results[it][metric + '_v']:
                            max_metrics[metric] = results[it][metric + '_v']
                            if metric == self.params.best_metric:
                                best_epoch, best_state, best_epoch_print = it, self.state_dict(), epoch_print
                    if (it % self.verbose == 0 or it == 1) and self.verbose != -1:
                        torch.save(self.state_dict(), os.path.join(wdir, f'weights-{it}-{self.directory_parameters}.pt'))
                    start_ep = time()
                    it += 1
                    loss = 0
                    steps = 0
        finally:
            # however the loop ends (an exception in the evaluator, an interrupt): the last step's update and loss land while
            # loss_buf is still alive, and steps asked for their loss afterwards (train_step) get it at once again
            self.engine.set_loss_lag(False)
        print('Training end...')
        self._store_run_files(os.path.join(rdir, f'recs-{it - 1}-{self.directory_parameters}.tsv'))
        with open(os.path.join(rdir, f'results-metrics-{self.directory_parameters}') + '.pkl', 'wb') as f:
            pickle.dump(results, f)                                             # utils/write.py:14-22
        print("Store Best Model at Epoch {0}".format(best_epoch))
        print(best_epoch_print)
        last_state = self.state_dict()
        if best_state is not None:
            torch.save(best_state, os.path.join(wdir, f'best-weights-{best_epoch}-{self.directory_parameters}.pt'))
            self.load_state_dict(best_state)
        self._store_run_files(os.path.join(rdir, f'best-recs-{best_epoch}-{self.directory_parameters}.tsv'))
        self.load_state_dict(last_state)
        print('End Store Best Model!')
        print('Best Values for Each Metric:\nHR\tPrec\tRec\tAUC\tnDCG\n{}\t{}\t{}\t{}\t{}\n'.format(
            max_metrics['hr'], max_metrics['p'], max_metrics['r'], max_metrics['auc'], max_metrics['ndcg']))
        self.results = results
        return results

    def _store_run_files(self, path):
        """Every file of ranking.RUN_FILES the run's flags ask for, next to (and with) the recs-* / best-recs-* file at `path`, from
        the tables the model holds now.  ValueError for a path that is neither."""
        run_file(path, "recs")
        self._styles_open, self._styles_now = True, None         # one style table per store call, from the tables held now
        try:
            self._store_recs(path)
            self._store_new_user_recs(path)
            self._store_similar(path)
            self._store_diverse(path)
            self._store_calibrated(path)
            self._store_because(path)
            self._store_influence(path)
            self._store_audience(path)
            self._store_warm(path)
            self._store_styles(path)
            self._store_shelves(path)
        finally:
            self._styles_open, self._styles_now = False, None

    def _store_recs(self, path):
        """What train() leaves at the recs-* / best-recs-* paths: the top-K lists (BPRMF.py:167-187)."""
        self.evaluator.store_recommendation(path=path)

    # ---- users the model was not trained on: the reference's step on one user's pairs, the item side frozen (include/bprx.h) ----
    def fold_in_users(self, histories, steps=30, negatives=4, lr=None, reg=None, optimizer=None, seed=0, init=None):
        """Rows for users who arrive after training with a history of catalogue items each: (Gu_new [n, k], Tu_new [n, d]) device
        tensors (Tu_new is None for BPRMF), fitted by Engine.fold_in over the pairs of draw_fold_pairs(histories, num_items,
        negatives, seed).  lr / reg / optimizer: None = the run's.  init: None = zero rows, or (Gu rows, Tu rows) to start from."""
        eng = self.engine
        n = len(histories)
        ptr, pos, neg = draw_fold_pairs(histories, self.num_items, negatives, seed)
        g0, t0 = (None, None) if init is None else init
        Gu, Tu = fold_start_rows(g0, n, eng.k, eng.device), fold_start_rows(t0, n, eng.d, eng.device)
        eng.fold_in(ptr, pos, neg, steps, Gu, Tu, lr=self.learning_rate if lr is None else lr, reg=self.reg if reg is None else reg,
                    optimizer=self.optimizer_name if optimizer is None else optimizer, want_loss=False)
        return Gu, Tu

    def _fold_rows(self, histories, **fold):
        """What recommend_new_users hands to _score_fold_rows: the fitted rows (a model whose scores need more says so here)."""
        return self.fold_in_users(histories, **fold)

    def _score_fold_rows(self, rows, r0, r1):
        """(scores [r1 - r0, I], side [r1 - r0, I, c] or None) of rows [r0, r1) of what _fold_rows returned."""
        return self.engine.score_rows_block(rows[0], rows[1], r0, r1), None

    def recommend_new_users(self, histories, k=None, diversify=None, by_class=None, class_cap=None, classes=None, calibrate=None,
                            **fold):
        """The k (default top_k) best catalogue items of every new user, their own histories masked: numpy idx int [n, kk] and
        val [n, kk], kk = min(k, I), best first; a model whose scores come with attentions (AttentiveFashion) also returns alpha
        [n, kk, 3] (colour, edges, class).  The rows are fitted by fold_in_users(histories, **fold), scored in row blocks and
        listed by ranking.rank_rows: on the device, rows whose list depends on the order of equal scores redone with numpy on the
        GPU's (masked) row.
        diversify: None, or theta (a float in [0, 1]), or a dict with any of theta / pool / space as recommend_diverse takes
        them: the lists are then picked by greedy MMR from each row's top-`pool` and (ids, vals, pen, ild) is returned, as by
        recommend_diverse (BPRMF, VBPR, GradFashion).
        by_class = K: the new users' shelves instead, (ids [n, C, kk], vals, cnt) as recommend_by_class returns them; class_cap = M:
        their quota lists, (ids [n, kk], vals, cls) as recommend_capped returns them; classes as recommend_by_class takes them.
        calibrate: None, or lambda (a float in [0, 1]), or a dict with any of lam / pool / alpha as recommend_calibrated takes
        them: the lists are then re-ranked toward the class mix of each history (a repeated item counted once) and (ids, vals, cls,
        gain, kl) is returned, as by recommend_calibrated."""
        if sum(x is not None for x in (diversify, by_class, class_cap, calibrate)) > 1:
            raise ValueError("recommend_new_users: one of diversify, by_class, class_cap and calibrate")
        div = self._fold_diverse_args(k, diversify)              # (checked before anything is fitted)
        if calibrate is not None:
            cal = self._fold_calibrate_args(k, calibrate, classes)
            return self._rank_fold_rows(self._fold_rows(histories, **fold), histories, k, cal=cal)
        if by_class is not None or class_cap is not None:
            self._class_args(by_class if by_class is not None else 1, class_cap)
            ccsr = self._class_csr(classes)
            rows = self._fold_rows(histories, **fold)
            return self._rank_fold_classes(rows, histories, ccsr, by_class) if by_class is not None \
                else self._cap_fold_rows(rows, histories, ccsr, k, class_cap)
        return self._rank_fold_rows(self._fold_rows(histories, **fold), histories, k, div)

    def _fold_diverse_args(self, k, diversify):
        """recommend_new_users' `diversify` as _diverse_args returns it, checked; None for None."""
        if diversify is None:
            return None
        opts = dict(diversify) if isinstance(diversify, dict) else {"theta": diversify}
        return self._diverse_args(k, opts.get("pool"), opts.get("theta"), opts.get("space"))

    def _rank_fold_rows(self, rows, histories, k=None, div=None, cal=None):
        """What recommend_new_users returns for the fitted rows of _fold_rows(histories): the plain lists, with div (from
        _fold_diverse_args) the diversified ones, with cal (from _fold_calibrate_args) the calibrated ones.  The rows are only
        read: one fit serves all."""
        eng = self.engine
        n, I = len(histories), self.num_items
        k = self.evaluator.k if k is None else int(k)
        if cal is not None:
            kk, pool, lam, alpha, (table, C) = cal
            once = [list(dict.fromkeys(l)) for l in histories]   # a repeated item counts once
            out = calibrated_zeros(n, kk)
        elif div is None:
            out = ranked_zeros(n, min(k, I), self.new_users_side)
        else:
            kk, pool, theta, space = div
            rn = eng.sim_rnorm(space)
            mmr = lambda pi, pv, kq: eng.diversify(space, rn, pi, pv, kq, theta)
            out = diverse_zeros(n, kk)
        for b0, b1 in blocks(n, self.evaluator.user_block, I):
            sc, side = self._score_fold_rows(rows, b0, b1)
            topk = lambda s, kq: eng.topk_lists(s, eng.csr(histories[b0:b1]), kq)
            if cal is not None:
                pi, pv, _ = rank_rows(topk, sc, pool)
                hist = eng.csr(once[b0:b1])
                res = calibrate_rows(lambda qi, qv, kq: eng.calibrate(qi, qv, hist, table, C, kq, lam, alpha), pi, pv, kk, eng.device)
            elif div is None:
                res = rank_rows(topk, sc, k, side)
            else:
                pi, pv, _ = rank_rows(topk, sc, pool)
                res = diversify_rows(mmr, pi, pv, kk, eng.device)
            for o, r in zip(out, res):
                o[b0:b1] = r
        return out

    new_users_param = "new_users"                                # the params entry that names the new users' file
    new_users_side = 0                                           # columns of the side _score_fold_rows returns; 0: none

    def _store_new_user_recs(self, path):
        """params.new_users (AttentiveFashion: params.af_new_users): new-user-recs-* next to the recs-* file at `path`, rows
        'label\ti\tscore' (AttentiveFashion: + '\talpha_colour\talpha_edges\talpha_class'), best first, one block per label
        in file order."""
        src = getattr(self.params, self.new_users_param, None)
        if not src:
            return
        from .train_rec import read_new_users
        labels, lists = read_new_users(src)
        rows = self._fold_rows(lists, steps=getattr(self.params, "fold_steps", 30), negatives=getattr(self.params, "fold_negatives", 4),
                               seed=getattr(self.params, "init_seed", 0))
        res = self._rank_fold_rows(rows, lists)
        new_path = run_file(path, "new-user-recs")
        with open(new_path, 'w') as out:
            write_ranked(out, labels, *res)
        if self.because_top > 0:                                 # because-new-user-recs-*: each label's own history, deduplicated
            ids, vals = res[0], res[1]
            hist, cos, _ = self.because(np.repeat(np.arange(len(labels)), ids.shape[1]), ids.reshape(-1), self.because_top,
                                        lists=[list(dict.fromkeys(l)) for l in lists])
            with open(because_paths(new_path), 'w') as out:
                write_because(out, labels, ids, vals, hist.reshape(ids.shape + (-1,)), cos.reshape(ids.shape + (-1,)))
        if self.influence_top > 0:                               # influence-new-user-recs-*: the fitted rows and the pairs that fitted them
            top = self._influence_args(self.influence_top)
            ids, vals = res[0], res[1]
            negatives = getattr(self.params, "fold_negatives", 4)
            ptr, pos, neg = draw_fold_pairs(lists, self.num_items, negatives, getattr(self.params, "init_seed", 0))
            dev = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a, dtype=dt), device=self.engine.device)
            e = self.engine.influence(rows[0], rows[1], dev(ptr, np.int64), dev(pos, np.int32), dev(neg, np.int32), negatives,
                                      dev(ids, np.int32), top, reg=self.reg, damp=self.influence_damp)
            with open(influence_file(path, "influence-new-user-recs"), 'w') as out:
                write_influence(out, labels, ids, vals, e["item"].cpu().numpy(), e["infl"].cpu().numpy(), e["total"].cpu().numpy())
        if self.diversify_theta > 0:                             # div-new-user-recs-* / div-new-user-ild-*: the same fitted rows
            p_recs, p_ild = div_paths(new_path)
            with open(p_recs, 'w') as out, open(p_ild, 'w') as out_ild:
                write_diverse(out, out_ild, labels, *self._rank_fold_rows(rows, lists, div=self._fold_diverse_args(None, {})))
        if self.calibrate_lambda > 0:                            # cal-new-user-recs-* / cal-new-user-kl-*: the same fitted rows
            p_recs, p_kl = cal_paths(new_path)
            cal = self._fold_calibrate_args(None, {}, None)
            with open(p_recs, 'w') as out, open(p_kl, 'w') as out_kl:
                write_calibrated(out, out_kl, labels, *self._rank_fold_rows(rows, lists, cal=cal),
                                 hist_classed(lists, cal[4][0].cpu().numpy()))
        if self.shelves_k > 0:                                   # shelf-new-user-recs-*: the same fitted rows
            with open(shelf_file(path, "shelf-new-user-recs"), 'w') as out:
                write_shelves(out, labels, *self._rank_fold_classes(rows, lists, self._class_csr(), self.shelves_k), self.shelf_count)
        if self.class_cap > 0:                                   # cap-new-user-recs-*
            with open(shelf_file(path, "cap-new-user-recs"), 'w') as out:
                write_capped(out, labels, *self._cap_fold_rows(rows, lists, self._class_csr(), None, self.class_cap))

    # ---- category shelves and quota lists: per-class top-K over the score rows (include/bprx.h, bprx_topk_classes) ---------------
    def _class_args(self, k, cap):
        """recommend_by_class' / recommend_capped's checks: a model on the engine's plain score block, the device path, K and cap."""
        if not self.diverse:
            raise NotImplementedError("%s: category lists come from BPRMF, VBPR and GradFashion" % type(self).__name__)
        if getattr(self.evaluator, "force_host", False):
            raise ValueError("category lists are ranked on the device only (no force_host): there is no host form")
        if not 1 <= int(k) <= 1024:
            raise ValueError("category lists: K lies in [1, 1024] (got %d)" % int(k))
        if cap is not None and int(cap) < 1:
            raise ValueError("category lists: the cap per class is >= 1 (got %d)" % int(cap))

    def item_classes(self):
        """The run's class table, an int64 array [num_items] with -1 for an item without a class: params.item_classes is such an
        array, the path of a TSV of `item<TAB>class` rows (train_rec.read_item_classes) or the literal 'dataset' (the argmax of every
        item's one-hot class vector, train_rec.dataset_item_classes).  Read once."""
        if getattr(self, "_item_classes", None) is None:
            src = getattr(self.params, "item_classes", None)
            if src is None:
                raise ValueError("%s: no class table (params.item_classes, --item_classes)" % type(self).__name__)
            if isinstance(src, str) and src == "styles":         # never cached: the best model's styles are not the last epoch's
                return self._run_styles()[0]
            if isinstance(src, str):
                from .train_rec import dataset_item_classes, read_item_classes
                src = dataset_item_classes(self.params.dataset, self.num_items) if src == "dataset" \
                    else read_item_classes(src, self.num_items)
            self._item_classes = np.asarray(src, dtype=np.int64).reshape(-1)
        return self._item_classes

    def _class_csr(self, classes=None):
        """ranking.class_csr of `classes` (an int array [num_items], -1 = no class); None: of the run's table, made once."""
        if classes is not None:
            return class_csr(np.asarray(classes), self.num_items, self.engine.device)
        if isinstance(getattr(self.params, "item_classes", None), str) and self.params.item_classes == "styles":
            return class_csr(self.item_classes(), self.num_items, self.engine.device, classes=self.styles_S or None)
        if getattr(self, "_class_csr_dev", None) is None:
            self._class_csr_dev = class_csr(self.item_classes(), self.num_items, self.engine.device)
        return self._class_csr_dev

    def _class_blocks(self, want, n, C, K):
        """ranking.wanted_blocks over n score rows of the catalogue's width, cut so that one call's outputs stay below 2^27 too."""
        return wanted_blocks(want, n, class_rows_per_block(self.evaluator.user_block, self.num_items, C, K))

    def recommend_by_class(self, users=None, k=None, classes=None):
        """The shelves of every user of `users` (None: all, in id order): the k (default: params.shelves, else top_k) best items of
        every class, the training items masked: numpy ids int64 [n, C, kk], vals fp32 [n, C, kk] and cnt int64 [n, C], kk = min(k,
        I); list (u, c) holds cnt[u, c] entries best first, equal scores by ascending item, then -1 / 0.0.  classes: an int array
        [num_items], the class of every item, -1 = none (None: the run's table, item_classes()); C = the largest class id + 1.  The
        scores are predict_all's (Engine.score_block), ranked by Engine.topk_classes through ranking.rank_class_rows; the user's
        order of the shelves is ranking.shelf_order(vals, cnt)."""
        k = (self.shelves_k or self.evaluator.k) if k is None else int(k)
        self._class_args(k, None)
        return self._rank_user_classes(users, self._class_csr(classes), k)

    def recommend_capped(self, users=None, k=None, cap=None, classes=None):
        """The quota lists of every user of `users` (None: all, in id order): the user's top-k (default top_k) with at most `cap`
        (default: params.class_cap) items of any one class, the training items masked and items without a class left out: numpy ids
        int64 [n, k], vals fp32 [n, k] and cls int64 [n, k], best first (equal scores by ascending item), -1 / 0.0 / -1 past a
        user's entries.  Exact: the k best of the union of every class's first min(cap, k) entries (ranking.cap_rows)."""
        k = self.evaluator.k if k is None else int(k)
        cap = (self.class_cap or k) if cap is None else int(cap)
        self._class_args(k, cap)
        ids, vals, cnt = self._rank_user_classes(users, self._class_csr(classes), min(cap, k))
        return cap_rows(ids, vals, cnt, k, cap)

    def _rank_user_classes(self, users, ccsr, K):
        """recommend_by_class' lists for the class table ccsr: user blocks of Engine.score_block, the training CSR as the mask."""
        eng, ev, U = self.engine, self.evaluator, self.num_users
        want = np.arange(U, dtype=np.int64) if users is None else np.asarray(users, dtype=np.int64).reshape(-1)
        if want.size and (want.min() < 0 or want.max() >= U):
            raise ValueError("category lists: user ids lie in [0, %d)" % U)
        ev._metrics_device_csr()
        C, kk = ccsr[2], min(K, self.num_items)
        out = np.full((want.size, C, kk), -1, np.int64), np.zeros((want.size, C, kk), np.float32), np.zeros((want.size, C), np.int64)
        for b0, b1, rows, local in self._class_blocks(want, U, C, kk):
            res = rank_class_rows(lambda s, kq: eng.topk_classes(s, ev._csr["train"], ccsr, kq, row0=b0), eng.score_block(b0, b1), K)
            for o, r in zip(out, res):
                o[rows] = r[local]
        return out

    def _rank_fold_classes(self, rows, histories, ccsr, K):
        """recommend_by_class' lists for the fitted rows of _fold_rows(histories), each row's own history masked."""
        eng, n = self.engine, len(histories)
        C, kk = ccsr[2], min(int(K), self.num_items)
        out = np.full((n, C, kk), -1, np.int64), np.zeros((n, C, kk), np.float32), np.zeros((n, C), np.int64)
        for b0, b1, _, _ in self._class_blocks(np.arange(n, dtype=np.int64), n, C, kk):
            sc, _ = self._score_fold_rows(rows, b0, b1)
            res = rank_class_rows(lambda s, kq: eng.topk_classes(s, eng.csr(histories[b0:b1]), ccsr, kq), sc, K)
            for o, r in zip(out, res):
                o[b0:b1] = r
        return out

    def _cap_fold_rows(self, rows, histories, ccsr, k, cap):
        """recommend_capped's lists for the fitted rows of _fold_rows(histories)."""
        k = self.evaluator.k if k is None else int(k)
        return cap_rows(*self._rank_fold_classes(rows, histories, ccsr, min(int(cap), k)), k, int(cap))

    def _store_shelves(self, path):
        """params.shelves = K > 0: shelf-recs-* (rows 'u\tclass\ti\tscore': per user the first params.shelf_count shelves, 0 = all,
        in the user's order) and params.class_cap = M > 0: cap-recs-* (rows 'u\ti\tscore\tclass') next to the recs-* file at `path`."""
        if self.shelves_k > 0:
            self.evaluator.store_recommendation_shelves(shelf_file(path, "shelf-recs"), self.shelves_k, self.shelf_count)
        if self.class_cap > 0:
            self.evaluator.store_recommendation_capped(shelf_file(path, "cap-recs"), self.class_cap)

    # ---- style clusters: spherical k-means of the item space (include/bprx.h, bprx_style_assign / bprx_style_update) -------------
    STYLE_BLOCK = 1 << 16                                        # catalogue rows per bprx_style_assign call

    def _style_args(self, S, space):
        """(S, space) of a clustering, checked: S (None: params.styles) in [1, 1024], space (None: similar_items' own)."""
        if not self.diverse:
            raise NotImplementedError("%s has no item space: styles come from BPRMF, VBPR and GradFashion" % type(self).__name__)
        S = self.styles_S if S is None else int(S)
        if not 1 <= S <= 1024:
            raise ValueError("styles: S lies in [1, 1024] (got %d)" % S)
        return S, self.similar_space if space is None else space

    def _style_assign_all(self, space, cent, rn):
        """(style int32 [I], cos fp32 [I]) device tensors: Engine.style_assign over the whole catalogue, block by block."""
        I = self.num_items
        parts = [self.engine.style_assign(space, cent, b0, min(b0 + self.STYLE_BLOCK, I), rn, want_second=False)
                 for b0 in range(0, I, self.STYLE_BLOCK)]
        return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])

    def _seed_centroids(self, space, rn, seeds):
        """fp32 [S, w] on the device: the unit rows of the items `seeds`, each made by Engine.style_update as the centroid of the
        cluster that holds that one item (so a seed's row is what a one-member cluster gets in the loop)."""
        eng, seeds = self.engine, np.asarray(seeds, dtype=np.int64).reshape(-1)
        if seeds.size and (seeds.min() < 0 or seeds.max() >= self.num_items):
            raise ValueError("styles: seed ids lie in [0, %d)" % self.num_items)
        S = int(seeds.size)
        csr = (torch.arange(S + 1, dtype=torch.int64, device=eng.device), torch.as_tensor(seeds.astype(np.int32), device=eng.device), S)
        zeros = torch.zeros((S, eng._style_width(space)), dtype=torch.float32, device=eng.device)
        return eng.style_update(space, rn, csr, zeros)[0]

    def style_seeds(self, S, space=None):
        """S deterministic farthest-first seeds, an int64 array of item ids: the first is the smallest id with a non-zero norm, each
        next one the item with a non-zero norm whose largest cosine to the seeds so far is smallest, equal values by the smallest
        id (a seed is not taken twice).  One S = 1 Engine.style_assign per round: S I w multiply-adds in all.  ValueError for fewer
        than S items with a non-zero norm."""
        S, space = self._style_args(S, space)
        eng, I = self.engine, self.num_items
        rn = eng.sim_rnorm(space)
        live = rn > 0
        if int(live.sum()) < S:
            raise ValueError("style_seeds: %d items with a non-zero norm, %d seeds asked" % (int(live.sum()), S))
        inf = torch.full((I,), float("inf"), dtype=torch.float32, device=eng.device)
        far = torch.where(live, torch.full_like(inf, -float("inf")), inf)       # the largest cosine to a seed; +inf: not a candidate
        seeds = [int(torch.nonzero(live)[0])]
        while len(seeds) < S:
            far[seeds[-1]] = float("inf")
            _, cos, _ = eng.style_assign(space, self._seed_centroids(space, rn, seeds[-1:]), 0, I, rn, want_second=False)
            far = torch.maximum(far, cos)                        # (+inf stays +inf)
            seeds.append(int(torch.nonzero(far == far.min())[0]))               # the smallest id among the equal minima
        return np.asarray(seeds, dtype=np.int64)

    def item_styles(self, S=None, iters=None, space=None, seeds=None):
        """Spherical k-means of the catalogue in `space` (None: similar_items' own) with S (None: params.styles) clusters: Lloyd's
        loop from the unit rows of `seeds` (None: style_seeds(S, space)).  The catalogue is assigned once; then every iteration
        builds ranking.class_csr of the assignment, runs Engine.style_update and assigns the whole catalogue again in blocks,
        until no assignment changes or `iters` (None: params.style_iters, 20) iterations have run.  Returns numpy arrays: style
        int64 [I] (-1 for a zero row), cos fp32 [I] (to the item's centroid), cent fp32 [S, w] and objective float64 [iterations
        run], objective[t] = sum_s mass[s] / (items with a style) after iteration t's update: it never decreases.  style and
        cos are those of the returned centroids."""
        S, space = self._style_args(S, space)
        iters = self.style_iters if iters is None else int(iters)
        if iters < 0:
            raise ValueError("styles: iters >= 0 (got %d)" % iters)
        eng, I = self.engine, self.num_items
        seeds = self.style_seeds(S, space) if seeds is None else np.asarray(seeds, dtype=np.int64).reshape(-1)
        if seeds.size != S:
            raise ValueError("styles: %d seeds for %d styles" % (seeds.size, S))
        rn = eng.sim_rnorm(space)
        cent = self._seed_centroids(space, rn, seeds)
        style, cos = self._style_assign_all(space, cent, rn)
        objective = []
        for _ in range(iters):
            st = style.cpu().numpy()
            cent, mass = eng.style_update(space, rn, class_csr(st, I, eng.device, classes=S), cent)
            objective.append(float(mass.double().sum()) / max(1, int((st >= 0).sum())))
            new_style, cos = self._style_assign_all(space, cent, rn)
            same = bool(torch.equal(new_style, style))
            style = new_style
            if same:
                break
        eng.sync_check()
        return style.cpu().numpy().astype(np.int64), cos.cpu().numpy(), cent.cpu().numpy(), np.asarray(objective, dtype=np.float64)

    def _run_styles(self):
        """(style, cos, cent, objective) of the run's flags from the tables the model holds now; inside a store call (see
        _store_run_files) computed once and shared by every file of the call."""
        if getattr(self, "_styles_now", None) is not None:
            return self._styles_now
        res = self.item_styles()
        if getattr(self, "_styles_open", False):
            self._styles_now = res
        return res

    def style_members(self, style, cos, top=None, S=None):
        """Every style's `top` (None: params.style_top) members nearest its centroid: (sizes int64 [S], ids int64 [S, R], vals fp32
        [S, R], cnt int64 [S]), R = min(top, I), best first, equal cosines by ascending item, -1 / 0.0 past cnt: Engine.topk_classes
        over the one-row score block `cos` with the styles as the classes (S: their number, None: params.styles)."""
        top = self.style_top if top is None else int(top)
        self._class_args(top, None)
        S, eng = int(S) if S is not None else (self.styles_S or max(1, int(np.max(style)) + 1)), self.engine
        ccsr = class_csr(np.asarray(style), self.num_items, eng.device, classes=S)
        row = torch.as_tensor(np.ascontiguousarray(cos, dtype=np.float32), device=eng.device).reshape(1, -1)
        ids, vals, cnt = rank_class_rows(lambda sc, kq: eng.topk_classes(sc, None, ccsr, kq), row, top)
        return np.bincount(np.asarray(style)[np.asarray(style) >= 0], minlength=S).astype(np.int64), ids[0], vals[0], cnt[0]

    def _store_styles(self, path):
        """params.styles = S > 0: styles-*, style-items-* and user-styles-* next to the recs-* file at `path`."""
        if self.styles_S <= 0:
            return
        style, cos = self._run_styles()[:2]
        self.evaluator.store_styles(path, style, cos)

    # ---- similar items: the cosine of two items in the model's item space (include/bprx.h, bprx_sim_*) -------------------------
    sim_space = "latent"                                         # the space similar_items walks by default

    def similar_items(self, items=None, k=None, space=None):
        """The k (default: params.similar_items, else top_k) catalogue items most like each item of `items` (None: the whole
        catalogue, in id order) by cosine in `space` ('latent': Gi; 'visual': f E; 'both': [Gi | f E]; None: the model's own,
        latent for BPRMF, visual for VBPR / GradFashion): numpy ids int64 [n, kk] and vals fp32 [n, kk], kk = min(k, I - 1), best
        first, the item itself excluded.  The catalogue is walked in blocks of item rows (Engine.sim_block), every block listed by
        ranking.rank_rows with Engine.topk_lists and lists in which every row names itself; an explicit id list ranks the blocks
        that hold its ids and keeps those rows."""
        eng, I = self.engine, self.num_items
        k = (self.similar_k or self.evaluator.k) if k is None else int(k)
        space = self.similar_space if space is None else space
        want = np.arange(I, dtype=np.int64) if items is None else np.asarray(items, dtype=np.int64).reshape(-1)
        if want.size and (want.min() < 0 or want.max() >= I):
            raise ValueError("similar_items: item ids lie in [0, %d)" % I)
        kk = min(k, I - 1)
        rn = eng.sim_rnorm(space)
        ids, vals = ranked_zeros(want.size, kk)
        for b0, b1, rows, local in wanted_blocks(want, I, self.evaluator.user_block, I):
            own = eng.csr([[q] for q in range(b0, b1)])
            bi, bv, _ = rank_rows(lambda s, kq: eng.topk_lists(s, own, kq), eng.sim_block(space, b0, b1, rn), k)
            ids[rows], vals[rows] = bi[local, :kk], bv[local, :kk]                          # (k >= I: the masked self is last)
        return ids, vals

    def _store_similar(self, path):
        """params.similar_items = K > 0: sim-* next to the recs-* file at `path`, rows 'i\tj\tcosine', item by item, best first."""
        if self.similar_k <= 0:
            return
        self.evaluator.store_similar_items(run_file(path, "sim"), self.similar_space)

    # ---- audiences: the top-K users of an item, the score block item-major (include/bprx.h, bprx_audience_block) ----------------
    def _owners(self):
        """ranking.owners_of the training lists: per item the users store_recommendation masks it for (made once)."""
        if getattr(self, "_owners_of", None) is None:
            self._owners_of = owners_of(self.data.training_list[:self.num_users], self.num_items)
        return self._owners_of

    def audience(self, items=None, k=None):
        """The k (default: params.audience (AttentiveFashion: af_audience), else top_k) users with the highest score for each item
        of `items` (None: the whole catalogue, in id order), the item's owners (the users whose training list names it) excluded:
        numpy ids int64 [n, kk] and vals fp32 [n, kk], kk = min(k, U), best first; AttentiveFashion adds alpha fp32 [n, kk, 3]
        (colour, edges, class); an item with fewer than kk non-owners has -1 / -inf in the slots past them.  The scores are
        predict_all's, item-major (Engine.audience_block; AttentiveFashion: af_score_block's, Engine.af_audience_block); the
        catalogue is walked in blocks of item rows, every block listed by ranking.rank_rows with Engine.topk_rows_masked and the
        block's owner lists; an explicit id list ranks the blocks that hold its ids and keeps those rows."""
        eng, I, U = self.engine, self.num_items, self.num_users
        k = (self.audience_k or self.evaluator.k) if k is None else int(k)
        want = np.arange(I, dtype=np.int64) if items is None else np.asarray(items, dtype=np.int64).reshape(-1)
        if want.size and (want.min() < 0 or want.max() >= I):
            raise ValueError("audience: item ids lie in [0, %d)" % I)
        out = ranked_zeros(want.size, min(k, U), self.warm_side)
        owners = self._owners() if want.size else None
        for b0, b1, rows, local in wanted_blocks(want, I, self.evaluator.user_block, U):
            own = eng.csr(owners[b0:b1])
            sc, side = self._audience_block(b0, b1)
            for o, res in zip(out, rank_rows(lambda s, kq: eng.topk_rows_masked(s, own, kq), sc, k, side)):
                o[rows] = res[local]
        out[0][out[1] == -np.inf] = -1                           # (a masked entry reached the list: the row came through numpy)
        return out

    warm_side = 0                                                # columns of the side the three block hooks below return; 0: none

    def _audience_block(self, b0, b1):
        """(scores [b1 - b0, U], side [b1 - b0, U, c] or None) of the catalogue items [b0, b1), item-major."""
        return self.engine.audience_block(b0, b1), None

    def _score_warm_block(self, rows, b0, b1):
        """(scores [b1 - b0, n], side or None) of the users [b0, b1) for the warm rows fold_in_items returned."""
        return self.engine.score_warm_block(b0, b1, *rows), None

    def _audience_warm_block(self, rows, b0, b1):
        """(scores [b1 - b0, U], side or None) of the warm rows [b0, b1) of what fold_in_items returned, item-major."""
        return self.engine.audience_warm_block(*rows, b0, b1), None

    def _store_audience(self, path):
        """params.audience = K > 0: audience-* next to the recs-* file at `path`, rows 'i\tu\tscore', item by item (the ids of
        params.audience_items, else the whole catalogue), best first."""
        if self.audience_k <= 0:
            return
        src = getattr(self.params, "audience_items", None)
        items = None
        if src:
            from .train_rec import read_audience_items
            items = read_audience_items(src, self.num_items)
        self.evaluator.store_audience(item_file(path, "audience"), items)

    # ---- warm items: Gi / Bi rows for new items from their first buyers, everything else frozen (include/bprx.h) ------------------
    def _warm_projections(self, features, n):
        """Pn of the n new items as Engine.fold_in_items takes it: None for a model without a visual part, which takes no features."""
        if features is not None:
            raise ValueError("%s: a model without a visual part takes no features" % type(self).__name__)
        return None

    def fold_in_items(self, buyers, features=None, steps=30, negatives=4, lr=None, reg=None, optimizer=None, seed=0, init=None):
        """Rows for items that arrive after training, from their first buyers (buyers[r]: the catalogue users who bought new item
        r): (Gi_new [n, k], Bi_new [n], P_new [n, proj_stride] or None) device tensors, fitted by Engine.fold_in_items over the
        pairs of draw_item_fold_pairs(buyers, training_list, num_items, negatives, seed).  VBPR / GradFashion need `features` (raw
        rows, or a table from prepare_new_items), one row per item.  lr / reg / optimizer: None = the run's.  init: None = zero
        rows, or (Gi rows, Bi rows) to start from.  An item without buyers keeps its start rows: from zeros it scores exactly as
        score_new_items scores it.  With plain sgd the step size must shrink with the number of pairs (the batch loss is summed:
        lr * 0.25 * pairs * (1 + |Gu|^2) < 2); Adam, the default, does not care.  For first buyers, not for refitting
        bestsellers."""
        eng = self.engine
        n = len(buyers)
        P = self._warm_projections(features, n)
        ptr, user, other, role = draw_item_fold_pairs(buyers, self.data.training_list[:self.num_users], self.num_items, negatives, seed)
        g0, b0 = (None, None) if init is None else init
        Gi, Bi = fold_start_rows(g0, n, eng.k, eng.device), fold_start_rows(b0, n, 1, eng.device).reshape(n)
        eng.fold_in_items(ptr, user, other, role, steps, Gi, Bi, P, lr=self.learning_rate if lr is None else lr,
                          reg=self.reg if reg is None else reg, optimizer=self.optimizer_name if optimizer is None else optimizer,
                          want_loss=False)
        return Gi, Bi, P

    def recommend_warm(self, buyers, features=None, k=None, **fold):
        """The k (default top_k) best warm items of every user, the ones the user bought masked: numpy ids int64 [U, kk] (rows of
        `buyers`) and vals fp32 [U, kk] (AttentiveFashion: and alpha fp32 [U, kk, 3], colour, edges, class), kk = min(k, n), best
        first, -1 / -inf past a user's unmasked items.  The rows are fitted by fold_in_items(buyers, features, **fold), scored by
        Engine.score_warm_block (AttentiveFashion: Engine.af_score_warm_block) and listed by ranking.rank_rows with
        Engine.topk_rows_masked."""
        return self._rank_warm_recs(self.fold_in_items(buyers, features, **fold), buyers, k)

    def audience_warm(self, buyers, features=None, k=None, **fold):
        """The k (default: params.audience (AttentiveFashion: af_audience), else top_k) users with the highest score for every
        warm item, its buyers masked: numpy ids int64 [n, kk] and vals fp32 [n, kk] (AttentiveFashion: and alpha fp32 [n, kk, 3]),
        kk = min(k, U), best first, -1 / -inf past an item's non-buyers.  Fitted as recommend_warm fits, scored item-major by
        Engine.audience_warm_block (AttentiveFashion: Engine.af_audience_block)."""
        return self._rank_warm_audience(self.fold_in_items(buyers, features, **fold), buyers, k)

    def _rank_warm_recs(self, rows, buyers, k=None):
        """recommend_warm's lists for the fitted rows of fold_in_items(buyers): the rows are only read, one fit serves both lists."""
        eng, U, n = self.engine, self.num_users, len(buyers)
        k = self.evaluator.k if k is None else int(k)
        out = ranked_zeros(U, min(k, n), self.warm_side)
        if n == 0:
            return out
        bought = owners_of(buyers, U)                            # per user the warm items that user bought
        for b0, b1 in blocks(U, self.evaluator.user_block, n):
            own = eng.csr(bought[b0:b1])
            sc, side = self._score_warm_block(rows, b0, b1)
            for o, res in zip(out, rank_rows(lambda s, kq: eng.topk_rows_masked(s, own, kq), sc, k, side)):
                o[b0:b1] = res
        out[0][out[1] == -np.inf] = -1
        return out

    def _rank_warm_audience(self, rows, buyers, k=None):
        """audience_warm's lists for the fitted rows of fold_in_items(buyers)."""
        eng, U, n = self.engine, self.num_users, len(buyers)
        k = (self.audience_k or self.evaluator.k) if k is None else int(k)
        out = ranked_zeros(n, min(k, U), self.warm_side)
        for b0, b1 in blocks(n, self.evaluator.user_block, U):
            own = eng.csr([list(dict.fromkeys(int(u) for u in who)) for who in buyers[b0:b1]])
            sc, side = self._audience_warm_block(rows, b0, b1)
            for o, res in zip(out, rank_rows(lambda s, kq: eng.topk_rows_masked(s, own, kq), sc, k, side)):
                o[b0:b1] = res
        out[0][out[1] == -np.inf] = -1
        return out

    warm_param = "warm_items"                                    # the params entry that names the first buyers' file

    def _store_warm(self, path):
        """params.warm_items (AttentiveFashion: params.af_warm_items): warm-recs-* (rows 'u\tj\tscore') and, with params.audience
        (af_audience) = K > 0, warm-audience-* (rows 'j\tu\tscore') next to the recs-* file at `path`, j = the row of the file
        (VBPR / GradFashion / AttentiveFashion: of the new items' table; AttentiveFashion adds the three attentions to a row); one
        fit serves both."""
        src = getattr(self.params, self.warm_param, None)
        if not src:
            return
        from .train_rec import read_warm_items
        feats = self._load_new_items()
        buyers = read_warm_items(src, None if feats is None else len(feats[0] if isinstance(feats, tuple) else feats))
        fold = dict(steps=getattr(self.params, "fold_steps", 30), negatives=getattr(self.params, "fold_negatives", 4),
                    seed=getattr(self.params, "init_seed", 0))
        rows = self.evaluator.store_recommendation_warm(warm_file(path, "warm-recs"), buyers, feats, **fold)
        if self.audience_k > 0:
            self.evaluator.store_audience_warm(warm_file(path, "warm-audience"), buyers, rows=rows)

    def _load_new_items(self):
        """The tables of params.new_items; a model without a visual part has none."""
        return None

    # ---- diversified lists: greedy MMR over each list's top-N pool in the model's item space (include/bprx.h, bprx_diversify) --
    diverse = True                                               # False: the model has no item space (ACF, AttentiveFashion)

    def _diverse_args(self, k, pool, theta, space):
        """(kk, N, theta, space) of a diversified ranking, checked: k (None: top_k) and pool (None: params.diversify_pool, 100)
        cut to the catalogue, theta (None: params.diversify, 0.5 where that is off), space (None: similar_items' own)."""
        if not self.diverse:
            raise NotImplementedError("%s has no item space: diversified lists come from BPRMF, VBPR and GradFashion"
                                      % type(self).__name__)
        k = self.evaluator.k if k is None else int(k)
        if getattr(self.evaluator, "force_host", False) or k > 1024:
            raise ValueError("--diversify ranks on the device only (no force_host, top_k <= 1024): there is no host MMR")
        pool = self.diversify_pool if pool is None else int(pool)
        theta = (self.diversify_theta or 0.5) if theta is None else float(theta)
        if not 0.0 <= theta <= 1.0:
            raise ValueError("diversify: theta lies in [0, 1] (got %s)" % theta)
        if not 1 <= k <= pool <= 1024:
            raise ValueError("diversify: need 1 <= k <= pool <= 1024 (got k = %d, pool = %d)" % (k, pool))
        I = self.num_items
        return min(k, I), min(pool, I), theta, self.similar_space if space is None else space

    def recommend_diverse(self, users=None, k=None, pool=None, theta=None, space=None):
        """The k (default top_k) items of every user of `users` (None: all, in id order) picked by greedy Maximal Marginal Relevance
        from the user's top-`pool` (default params.diversify_pool, 100; training items masked): each pick maximises
        (1 - theta) rel - theta max-cosine-with-the-picks-above, cosines in `space` (None: the model's own, as similar_items).
        Returns numpy ids int64 [n, kk], vals fp32 [n, kk] (the model's scores), pen fp32 [n, kk] (each pick's redundancy: its
        largest cosine with the picks above it) and ild fp32 [n] (1 - the mean pairwise cosine of the list), kk = min(k, I);
        slots past a user's unmasked items hold -1 / 0 / 0.  The pools are ranking.rank_rows' lists (Engine.topk, K = pool), the
        picks Engine.diversify's through ranking.diversify_rows; an explicit user list ranks the blocks that hold its users."""
        kk, N, theta, space = self._diverse_args(k, pool, theta, space)
        eng, ev = self.engine, self.evaluator
        U = self.num_users
        want = np.arange(U, dtype=np.int64) if users is None else np.asarray(users, dtype=np.int64).reshape(-1)
        if want.size and (want.min() < 0 or want.max() >= U):
            raise ValueError("recommend_diverse: user ids lie in [0, %d)" % U)
        ev._metrics_device_csr()
        rn = eng.sim_rnorm(space)
        div = lambda pi, pv, kq: eng.diversify(space, rn, pi, pv, kq, theta)
        out = diverse_zeros(want.size, kk)
        for b0, b1, rows, local in wanted_blocks(want, U, ev.user_block):
            pi, pv, _ = rank_rows(ev._topk(b0, b1), eng.score_block(b0, b1), N)
            res = diversify_rows(div, pi, pv, kk, eng.device)
            for o, r in zip(out, res):
                o[rows] = r[local]
        return out

    def _store_diverse(self, path):
        """params.diversify = theta > 0: div-recs-* (rows 'u\ti\tscore\tredundancy', in list order) and div-ild-* (rows 'u\tild')
        next to the recs-* file at `path`."""
        if self.diversify_theta <= 0:
            return
        self.evaluator.store_recommendation_diverse(*div_paths(path))

    # ---- calibrated lists: greedy KL re-rank of each list's top-N pool toward the user's class mix (include/bprx.h, bprx_calibrate) --
    CALIBRATE_CLASSES_MAX = 1024                                 # classes bprx_calibrate takes (BPRX_STYLES_MAX)

    def _calibrate_args(self, k, pool, lam, alpha, classes=None):
        """(kk, N, lambda, alpha, (class table int32 [I] on the device, C)) of a calibrated ranking, checked: k (None: top_k) and pool
        (None: params.calibrate_pool, 100) cut to the catalogue, lam (None: params.calibrate, 0.5 where that is off), alpha (None:
        params.calibrate_alpha, 0.01), classes (None: the run's table, item_classes(); with --item_classes styles the styles)."""
        if not self.diverse:
            raise NotImplementedError("%s: calibrated lists come from BPRMF, VBPR and GradFashion" % type(self).__name__)
        k = self.evaluator.k if k is None else int(k)
        if getattr(self.evaluator, "force_host", False) or k > 1024:
            raise ValueError("--calibrate ranks on the device only (no force_host, top_k <= 1024): there is no host form")
        pool = self.calibrate_pool if pool is None else int(pool)
        lam = (self.calibrate_lambda or 0.5) if lam is None else float(lam)
        alpha = self.calibrate_alpha if alpha is None else float(alpha)
        if not 0.0 <= lam <= 1.0:
            raise ValueError("calibrate: lambda lies in [0, 1] (got %s)" % lam)
        if not 0.0 < alpha < 1.0:
            raise ValueError("calibrate: alpha lies in (0, 1) (got %s)" % alpha)
        if not 1 <= k <= pool <= 1024:
            raise ValueError("calibrate: need 1 <= k <= pool <= 1024 (got k = %d, pool = %d)" % (k, pool))
        I = self.num_items
        return min(k, I), min(pool, I), lam, alpha, self._class_table(classes)

    def _class_table(self, classes=None):
        """(int32 device tensor [num_items], C) of `classes` (an int array [num_items], -1 = no class; None: the run's table): what
        bprx_calibrate reads.  C = the largest class id + 1, at least 1 (the styles: params.styles); more than 1024 is a ValueError."""
        styles = classes is None and isinstance(getattr(self.params, "item_classes", None), str) and self.params.item_classes == "styles"
        cls = np.asarray(self.item_classes() if classes is None else classes).reshape(-1)
        if cls.size != self.num_items or cls.dtype.kind not in "iu":
            raise ValueError("calibrate: one integer class per item, [%d] (got %s %s)" % (self.num_items, cls.dtype, cls.shape))
        if cls.size and cls.min() < -1:
            raise ValueError("calibrate: a class id is >= 0, or -1 for no class (got %d)" % cls.min())
        C = max(1, int(cls.max()) + 1 if cls.size else 1)
        if styles and self.styles_S:
            C = max(C, self.styles_S)
        if C > self.CALIBRATE_CLASSES_MAX:
            raise ValueError("calibrate: %d classes, the limit is %d" % (C, self.CALIBRATE_CLASSES_MAX))
        return torch.as_tensor(np.ascontiguousarray(cls, dtype=np.int32), device=self.engine.device), C

    def _fold_calibrate_args(self, k, calibrate, classes):
        """recommend_new_users' `calibrate` as _calibrate_args returns it, checked."""
        opts = dict(calibrate) if isinstance(calibrate, dict) else {"lam": calibrate}
        return self._calibrate_args(k, opts.get("pool"), opts.get("lam"), opts.get("alpha"), classes)

    def recommend_calibrated(self, users=None, k=None, pool=None, lam=None, alpha=None, classes=None):
        """The k (default top_k) items of every user of `users` (None: all, in id order) picked from the user's top-`pool` (default
        params.calibrate_pool, 100; training items masked) so that the list's class mix follows the mix of the user's training
        items (Steck 2018): each pick maximises (1 - lam) rel - lam (the change of KL(p || q~) the pick makes), q~ = (1 - alpha) q
        + alpha p.  classes: an int array [num_items], -1 = none (None: the run's table, item_classes()).  Returns numpy ids int64
        [n, kk], vals fp32 [n, kk] (the model's scores), cls int64 [n, kk] (the picks' classes), gain fp32 [n, kk] (the KL each
        pick removed at its step) and kl fp32 [n, 2] (KL(p || q~) of the plain top-kk and of the calibrated list), kk = min(k, I);
        slots past a user's unmasked items hold -1 / 0 / -1 / 0.  The pools are ranking.rank_rows' lists (Engine.topk, K = pool),
        the picks Engine.calibrate's through ranking.calibrate_rows, the histories the training CSR."""
        kk, N, lam, alpha, (table, C) = self._calibrate_args(k, pool, lam, alpha, classes)
        eng, ev = self.engine, self.evaluator
        U = self.num_users
        want = np.arange(U, dtype=np.int64) if users is None else np.asarray(users, dtype=np.int64).reshape(-1)
        if want.size and (want.min() < 0 or want.max() >= U):
            raise ValueError("recommend_calibrated: user ids lie in [0, %d)" % U)
        ev._metrics_device_csr()
        out = calibrated_zeros(want.size, kk)
        for b0, b1, rows, local in wanted_blocks(want, U, ev.user_block):
            pi, pv, _ = rank_rows(ev._topk(b0, b1), eng.score_block(b0, b1), N)
            cal = lambda qi, qv, kq: eng.calibrate(qi, qv, ev._csr["train"], table, C, kq, lam, alpha, row0=b0)
            res = calibrate_rows(cal, pi, pv, kk, eng.device)
            for o, r in zip(out, res):
                o[rows] = r[local]
        return out

    def _store_calibrated(self, path):
        """params.calibrate = lambda > 0: cal-recs-* (rows 'u\ti\tscore\tclass\tgain', in list order) and cal-kl-* (rows
        'u\tkl_plain\tkl_calibrated\thist_classed') next to the recs-* file at `path`."""
        if self.calibrate_lambda <= 0:
            return
        self.evaluator.store_recommendation_calibrated(*cal_paths(path))


    # ---- "because you own X": the nearest owned items of a recommended one (include/bprx.h, bprx_because) ----------------------
    def _because_args(self, top, space):
        """(top, space) of a because-call, checked: 1 <= top <= 32, space None: similar_items' own."""
        if not self.diverse:
            raise NotImplementedError("%s has no item space: its explanations by the user's history come from %s"
                                      % (type(self).__name__, self.because_instead))
        if getattr(self.evaluator, "force_host", False) or self.evaluator.k > 1024:
            raise ValueError("--because runs on the device only (no force_host, top_k <= 1024): there is no host form")
        top = int(top)
        if not 1 <= top <= 32:
            raise ValueError("because: top lies in [1, 32] (got %d)" % top)
        return top, self.similar_space if space is None else space

    because_instead = "--feat_explain"                           # (what a model without an item space names instead)

    def because(self, users, items, top=5, space=None, lists=None):
        """For every pair (users[p], items[p]) the `top` items of the user's history that are nearest to the item by cosine in
        `space` (None: the model's own, as similar_items): numpy hist int64 [n, top] (catalogue ids, nearest first, -1 past the
        candidates), cos fp32 [n, top] and count int64 [n] (the history's entries without the item itself).  lists: the
        histories, indexed by user (default: the training lists, a repeated item counted once).  Pairs may come in any order:
        runs of equal users share one list of the call (ranking.because_rows, Engine.because)."""
        top, space = self._because_args(top, space)
        eng = self.engine
        dedup = lists is None
        if lists is None:
            lists = _Padded(self.data.training_list, self.num_users)
        u = np.asarray(users, dtype=np.int64).reshape(-1)
        if u.size and (u.min() < 0 or u.max() >= len(lists)):
            raise ValueError("because: user ids lie in [0, %d)" % len(lists))
        rn = eng.sim_rnorm(space)
        return because_rows(lambda li, csr: eng.because(space, rn, li, csr, top), u, items, lists, top, eng.device, dedup)

    def _store_because(self, path):
        """params.because = L > 0: because-* next to the recs-* file at `path`, rows 'u\ti\tscore\trank\thist_item\tcosine' for
        every (u, i) of every user's top-k list."""
        if self.because_top <= 0:
            return
        self.evaluator.store_recommendation_because(because_paths(path), self.because_top, self.similar_space)


    # ---- influence: the history entries a score rests on, on the user's own fold-in objective (include/bprx.h, bprx_influence) --
    def _influence_args(self, top):
        """`top` of an influence call, checked: a model whose user row alone makes the score, the device path, 1 <= top <= 32."""
        if not self.diverse:
            raise NotImplementedError("%s: the score is not linear in the user's row; its explanations by the user's history come "
                                      "from %s" % (type(self).__name__, self.because_instead))
        if getattr(self.evaluator, "force_host", False) or self.evaluator.k > 1024:
            raise ValueError("--influence runs on the device only (no force_host, top_k <= 1024): there is no host form")
        top = int(top)
        if not 1 <= top <= 32:
            raise ValueError("influence: top lies in [1, 32] (got %d)" % top)
        return top

    def influence(self, users, items, top=5, negatives=None, seed=None, reg=None, damp=1.0, lists=None, rows=None, maps=False):
        """For every pair (users[p], items[p]) the `top` entries of the user's history the item's score rests on most: how far
        x_ui would fall, to first order, had the user not bought the entry (one damped Newton step on the user's fold-in
        objective with the entry's pairs left out; include/bprx.h, bprx_influence).  Returns numpy hist int64 [n, top] (catalogue
        ids by descending influence, -1 past the history's entries), infl fp32 [n, top], total fp32 [n] (sum of |influence| over
        all entries) and count int64 [n] (entries; 0 for a user without pairs or a row whose factorisation failed); with maps also
        fp32 [n, M], every entry's influence in history order (M: the longest history of the call, 0 past a user's own).
        lists: the histories, indexed by user (default: the training lists; a repeated item is an entry each time).  rows: None =
        the model's own rows of those users, or device (Gu rows, Tu rows or None) indexed like lists: folded-in users.  The
        objective's pairs are draw_fold_pairs(the histories of the call's users in order, num_items, negatives, seed); negatives /
        seed / reg: None = the run's --fold_negatives / --init_seed / reg.  Pairs may come in any order: runs of equal users
        share one list of the call (ranking.influence_rows, Engine.influence)."""
        top = self._influence_args(top)
        eng = self.engine
        negatives = int(getattr(self.params, "fold_negatives", 4) if negatives is None else negatives)
        seed = getattr(self.params, "init_seed", 0) if seed is None else seed
        reg = self.reg if reg is None else reg
        if lists is None:
            lists = _Padded(self.data.training_list, self.num_users)
        u = np.asarray(users, dtype=np.int64).reshape(-1)
        if u.size and (u.min() < 0 or u.max() >= len(lists)):
            raise ValueError("influence: user ids lie in [0, %d)" % len(lists))
        Gu, Tu = (eng.t["Gu"], eng.t["Tu"] if eng.d else None) if rows is None else rows
        if int(Gu.shape[0]) < len(lists):
            raise ValueError("influence: %d rows for %d histories" % (int(Gu.shape[0]), len(lists)))

        def take(ids):
            ix = torch.as_tensor(ids, dtype=torch.int64, device=eng.device)
            return Gu.index_select(0, ix).contiguous(), (Tu.index_select(0, ix).contiguous() if Tu is not None else None)

        return influence_rows(lambda g, t, ptr, pos, neg, li: eng.influence(g, t, ptr, pos, neg, negatives, li, top, reg=reg, damp=damp,
                                                                            maps=maps),
                              u, items, lists, top, eng.device, lambda h: draw_fold_pairs(h, self.num_items, negatives, seed), take, maps)

    def _store_influence(self, path):
        """params.influence = L > 0: influence-* next to the recs-* file at `path`, rows 'u\ti\tscore\trank\thist_item\tinfluence\t
        share' for every (u, i) of every user's top-k list."""
        if self.influence_top <= 0:
            return
        self.evaluator.store_recommendation_influence(influence_file(path, "influence"), self.influence_top, self.influence_damp)


class _Padded:
    """lists[u] for u < n: the list, [] past the end of a shorter table."""
    def __init__(self, lists, n):
        self.lists, self.n = lists, n

    def __len__(self):
        return self.n

    def __getitem__(self, u):
        return self.lists[u] if u < len(self.lists) else []


def _table_property(name):
    return property(lambda self: self.engine.t[name], doc="bound tensor %s (current: lazy adam_tf23 rows are replayed first)" % name)


for _n in ("Gu", "Gi", "Bi", "Tu", "F", "E", "Bp"):
    setattr(BPRMF, _n, _table_property(_n))


class VBPR(BPRMF):
    model_kind = "vbpr"

    def __init__(self, data, params, init=None, features=None):
        """`features`: optional [I,D] array used instead of the cnn_features .npy (already max-abs normalised
        unless `normalize=True` is left to do it)."""
        self.embed_d = params.embed_d
        self._features = features
        self.feat_explain = int(getattr(params, "feat_explain", 0) or 0)          # rows per pair in expl-*; 0: none
        if not 0 <= self.feat_explain <= 32:
            raise ValueError("%s: feat_explain is 0 (off) .. 32 (got %r)" % (type(self).__name__, self.feat_explain))
        super().__init__(data, params, init)
        self.directory_parameters = f'batch_{params.batch_size}-D_{params.embed_d}-K_{params.embed_k}' \
                                    f'-lr_{params.lr}-reg_{params.reg}' + self._hard_suffix()      # VBPR.py:35-39

    def process_cnn_visual_features(self):
        """visual_loader_mixin.py:22-31: np.load, divide by the GLOBAL max-abs, D = shape[1]."""
        f = self._features
        if f is None:
            f = np.load(configs.cnn_features_path(self.params.dataset, getattr(self.params, "cnn_model", "vgg19"),
                                                  getattr(self.params, "output_layer", "fc2")))
        f = np.asarray(f)
        self.feat_norm = np.max(np.abs(f))                                      # kept: new items are divided by the same value
        self.cnn_features = f / self.feat_norm
        self.dim_cnn_features = self.cnn_features.shape[1]

    def _init_tables(self, init):
        t, rs = super()._init_tables(init)
        self.process_cnn_visual_features()                                      # VBPR.py:41
        D, d = self.dim_cnn_features, self.embed_d
        v = {"Bp": glorot_uniform(rs, D, 1).reshape(-1),                        # VBPR.py:44-54, same creation order
             "Tu": glorot_uniform(rs, self.num_users, d),
             "F": self.cnn_features.astype(np.float32),
             "E": glorot_uniform(rs, D, d)}
        v.update({k: val for k, val in init.items() if k in v})
        t.update(v)
        return t, rs

    def _engine_kwargs(self):
        return dict(model="vbpr", num_users=self.num_users, num_items=self.num_items, embed_k=self.embed_k,
                    embed_d=self.embed_d, feat_dim=self.dim_cnn_features,
                    feat_dtype=getattr(self.params, "dtype", "fp32"))

    def call(self, inputs, training=None, mask=None):                           # VBPR.py:59-86
        u, i = self._pairs(inputs)
        xui = self.engine.score_pairs(u, i)
        return xui, self.Gu[u], self.Gi[i], self.F[i], self.Tu[u], self.Bi[i]

    __call__ = call

    @property
    def feat_cols(self):
        """The feature columns that exist: the width of the feature files, before any zero padding of F."""
        return self.dim_cnn_features

    def explain(self, users, items, top=5, maps=False):
        """The `top` feature columns that contribute most to each pair's score (Engine.feat_explain) as numpy arrays: score, base,
        visual [n], col / contrib [n, top] (rank 0 first), with maps=True also map [n, feat_cols]: x_ui = base + sum_c map[c]."""
        return {n: v.cpu().numpy() for n, v in self.engine.feat_explain(users, items, top, self.feat_cols, maps=maps).items()}

    def explain_ui(self, u, items, top=5, maps=False):
        """explain() for one user and several items."""
        items = list(items)
        return self.explain([int(u)] * len(items), items, top, maps)

    def _store_recs(self, path):
        """recs-* / best-recs-* as every model writes them; with params.feat_explain = L > 0 also expl-* / best-expl-* next to them;
        with params.new_items also new-recs-* (and new-expl-*) for the items of those files."""
        if self.feat_explain <= 0:
            super()._store_recs(path)
        else:
            self.evaluator.store_recommendation_features(path, run_file(path, "expl"), self.feat_explain)
        self._store_new_recs(path)

    # ---- items the model was not trained on: x_uj = Tu_u.(f_j E) + f_j.Bp, no Gi_j / Bi_j term (include/bprx.h) ---------------
    NORM_KEYS = ("feat_norm",)                                                  # the divisors of the training tables, in snapshots

    def state_dict(self):
        sd = super().state_dict()
        for n in self.NORM_KEYS:
            sd[n] = torch.as_tensor(np.asarray(getattr(self, n)))
        return sd

    def load_state_dict(self, sd):
        sd = dict(sd)
        for n in self.NORM_KEYS:                                                # (a snapshot from before the keys: the model's own)
            v = sd.pop(n, None)
            if v is not None:
                setattr(self, n, torch.as_tensor(v).cpu().numpy()[()])
        super().load_state_dict(sd)

    def _new_item_table(self, features):
        """[n, dim_cnn_features] float32: the raw rows divided by the training divisor (VBPR's table has no padding columns)."""
        return normalize_new_rows(features, self.feat_norm, self.dim_cnn_features, "features")

    def prepare_new_items(self, features):
        """Raw feature rows of items outside the catalogue (as the training file holds them, before any normalisation) -> the device
        table Engine.project_rows / feat_explain_new take: divided by the TRAINING divisor (a row may then exceed 1), float32, laid
        out like the training table, in the engine's feature dtype.  A raw row equal to a training row gives a bit-equal table row."""
        if getattr(self.params, "dtype", "fp32") == "fp8":
            raise ValueError("%s: new items need --dtype fp32 or bf16 (an fp8 table is scaled for the training max-abs: a new row "
                             "may saturate)" % type(self).__name__)
        return self.engine._new_table(self._new_item_table(features))

    def _as_new_table(self, features):
        return features if isinstance(features, torch.Tensor) and features.is_cuda else self.prepare_new_items(features)

    def score_new_items(self, features, u0=0, u1=None):
        """Device fp32 [u1-u0, n]: the visual score of every user of [u0, u1) for the n new items (raw rows, or a table from
        prepare_new_items)."""
        u1 = self.num_users if u1 is None else u1
        return self.engine.score_new_block(u0, u1, self.engine.project_rows(self._as_new_table(features)))

    def recommend_new(self, features, k=None, u0=0, u1=None, explain=0):
        """The k (default top_k) best new items of every user of [u0, u1): numpy idx int [nu, min(k, n)] (row of `features`) and val,
        best first; explain = L > 0: also the Engine.feat_explain_new dict (numpy) of those pairs, user by user.  Listed block by
        block by ranking.rank_rows (rows whose list depends on the order of equal scores: numpy on the GPU's row)."""
        eng = self.engine
        F = self._as_new_table(features)
        n = int(F.shape[0])
        k = self.evaluator.k if k is None else int(k)
        u1 = self.num_users if u1 is None else u1
        P = eng.project_rows(F)
        kk = min(k, n)
        idx_all, val_all = ranked_zeros(max(u1 - u0, 0), kk)
        for b0, b1 in blocks(u1 - u0, self.evaluator.user_block, n):
            idx_all[b0:b1], val_all[b0:b1], _ = rank_rows(eng.topk_rows, eng.score_new_block(u0 + b0, u0 + b1, P), k)
        if explain <= 0:
            return idx_all, val_all
        users = np.repeat(np.arange(u0, u1), kk)
        ex = eng.feat_explain_new(F, users, idx_all.reshape(-1), explain, self.feat_cols) if users.size else None
        return idx_all, val_all, ({} if ex is None else {nm: v.cpu().numpy() for nm, v in ex.items() if nm != "visual"})

    # ---- similar items (BPRMF.similar_items): the visual space is the model's own, and rows from outside the catalogue have one ----
    sim_space = "visual"

    def similar_to_new(self, features, k=None):
        """The k (default: params.similar_items, else top_k) catalogue items most like each row of `features` (raw rows of items
        outside the catalogue, or a table from prepare_new_items) by cosine in the visual space: numpy ids int64 [n, kk] and vals
        fp32 [n, kk], kk = min(k, I), best first.  Engine.project_rows puts the rows on the catalogue's scale; sim_rnorm and
        sim_block give the cosines, ranking.rank_rows with Engine.topk_rows the lists (nothing is masked)."""
        eng, I = self.engine, self.num_items
        k = (self.similar_k or self.evaluator.k) if k is None else int(k)
        P = eng.project_rows(self._as_new_table(features))
        n = int(P.shape[0])
        rn, rq = eng.sim_rnorm("visual"), eng.sim_rnorm("visual", P)
        ids, vals = ranked_zeros(n, min(k, I))
        for b0, b1 in blocks(n, self.evaluator.user_block, I):
            ids[b0:b1], vals[b0:b1], _ = rank_rows(eng.topk_rows, eng.sim_block("visual", b0, b1, rn, P, rq), k)
        return ids, vals

    def styles_of_new(self, features, cent):
        """The style of every row of `features` (raw rows of items outside the catalogue, or a table from prepare_new_items) among
        the centroids `cent` (fp32 [S, d], of item_styles in the visual space): numpy style int64 [n] (-1 for a zero projection)
        and cos fp32 [n].  Engine.project_rows puts the rows on the catalogue's scale, Engine.style_assign's Pq form assigns."""
        eng = self.engine
        P = eng.project_rows(self._as_new_table(features))
        n = int(P.shape[0])
        if n == 0:
            return np.zeros(0, np.int64), np.zeros(0, np.float32)
        rq = eng.sim_rnorm("visual", P)
        ct = torch.as_tensor(np.ascontiguousarray(cent, dtype=np.float32), device=eng.device)
        style, cos, _ = eng.style_assign("visual", ct, 0, n, rq, P, rq, want_second=False)
        return style.cpu().numpy().astype(np.int64), cos.cpu().numpy()

    def _store_styles(self, path):
        """styles-* as every model writes them; with params.new_items also new-styles-*, rows 'j_new\tstyle\tcosine' (the visual
        space)."""
        super()._store_styles(path)
        feats = self._load_new_items() if self.styles_S > 0 else None
        if feats is None:
            return
        if self.similar_space != "visual":
            raise ValueError("new-styles-* needs the visual space (similar_space = %r)" % self.similar_space)
        style, cos = self.styles_of_new(feats, self._run_styles()[2])
        self.evaluator.store_styles_new(style_file(path, "new-styles"), style, cos)

    def audience_new(self, features, k=None):
        """BPRMF.audience for items outside the catalogue: the k (default: params.audience, else top_k) users with the highest
        visual score for each row of `features` (raw rows, or a table from prepare_new_items): numpy ids int64 [n, kk] and vals
        fp32 [n, kk], kk = min(k, U), best first.  Engine.project_rows, audience_block on those rows and ranking.rank_rows with
        Engine.topk_rows: a new item has no owners, nothing is masked."""
        eng, U = self.engine, self.num_users
        k = (self.audience_k or self.evaluator.k) if k is None else int(k)
        P = eng.project_rows(self._as_new_table(features))
        n = int(P.shape[0])
        ids, vals = ranked_zeros(n, min(k, U))
        for b0, b1 in blocks(n, self.evaluator.user_block, U):
            ids[b0:b1], vals[b0:b1], _ = rank_rows(eng.topk_rows, eng.audience_block(b0, b1, P), k)
        return ids, vals

    def _warm_projections(self, features, n):
        """Pn [n, proj_stride] of the new items' features (raw rows, or a table from prepare_new_items), one row per item."""
        if features is None:
            raise ValueError("%s: warm items need their features (raw rows, or a table from prepare_new_items)" % type(self).__name__)
        P = self.engine.project_rows(self._as_new_table(features))
        if int(P.shape[0]) != n:
            raise ValueError("%s: %d feature rows for %d warm items" % (type(self).__name__, int(P.shape[0]), n))
        return P

    def _store_audience(self, path):
        """audience-* as every model writes it; with params.new_items also new-audience-*, rows 'j_new\tu\tscore'."""
        super()._store_audience(path)
        feats = self._load_new_items() if self.audience_k > 0 else None
        if feats is None:
            return
        self.evaluator.store_audience_new(item_file(path, "new-audience"), feats)

    def because_new(self, features, users, rows, top=5):
        """BPRMF.because for items outside the catalogue: for every pair (users[p], rows[p] of `features`: raw rows, or a table
        from prepare_new_items) the `top` items of the user's training list nearest to the new item in the visual space."""
        top, _ = self._because_args(top, "visual")
        eng = self.engine
        P = eng.project_rows(self._as_new_table(features))
        r = np.asarray(rows, dtype=np.int64).reshape(-1)
        u = np.asarray(users, dtype=np.int64).reshape(-1)
        if r.size and (r.min() < 0 or r.max() >= int(P.shape[0])):
            raise ValueError("because_new: rows lie in [0, %d)" % int(P.shape[0]))
        if u.size and (u.min() < 0 or u.max() >= self.num_users):
            raise ValueError("because_new: user ids lie in [0, %d)" % self.num_users)
        rn, rq = eng.sim_rnorm("visual"), eng.sim_rnorm("visual", P)
        return because_rows(lambda li, csr: eng.because("visual", rn, li, csr, top, P, rq), u, r,
                            _Padded(self.data.training_list, self.num_users), top, eng.device, True)

    def _store_because(self, path):
        """because-* as every model writes it; with params.new_items also because-new-recs-* for the pairs of new-recs-*."""
        super()._store_because(path)
        feats = self._load_new_items() if self.because_top > 0 else None
        if feats is None:
            return
        self.evaluator.store_because_new(run_file(path, "because-new-recs"), feats, self.because_top)

    def _store_similar(self, path):
        """sim-* as every model writes it; with params.new_items also new-sim-*, rows 'j_new\ti\tcosine' (always the visual space)."""
        super()._store_similar(path)
        feats = self._load_new_items() if self.similar_k > 0 else None
        if feats is None:
            return
        self.evaluator.store_similar_new(run_file(path, "new-sim"), feats)

    def _load_new_items(self):
        paths = list(getattr(self.params, "new_items", None) or [])
        return np.load(paths[0]) if paths else None

    def _store_new_recs(self, path):
        """params.new_items: new-recs-* (with feat_explain also new-expl-*) next to the recs-* file at `path`."""
        feats = self._load_new_items()
        if feats is None:
            return
        expl = run_file(path, "new-expl") if self.feat_explain > 0 else None
        self.evaluator.store_recommendation_new(run_file(path, "new-recs"), feats, expl, self.feat_explain)


class GradFashion(VBPR):
    """GradFashion.py:23-320: VBPR whose projection is factored through a colour and an edge embedding,
        vf_i = [Fc_i Ec | Fe_i Ee],   x_ui = Bi_i + Gu_u.Gi_i + Tu_u.(vf_i E) + vf_i.Bp,
    trained on the VBPR hot path with the effective projection E_eff = [Ec E[:ec] ; Ee E[ec:]] (include/bprx.h,
    bprx_bind_factored).  Same surface as the reference: color_weights {'Fc','Ec'}, edges_weights {'Fe','Ee'},
    visual_profile {'Bp','E','Tu'}, embed_color, embed_edges, call, predict_all, train_step, predict_ui_grads,
    get_grads_user, train.  F = [Fc | Fe] is padded with zero columns to the kernels' width granularity (16 fp32, 128 bf16).
    `features`: optional (Fc, Fe) arrays used instead of the two .npy files (normalised here like the files)."""
    model_kind = "grad_fashion"
    GRANULE = {"fp32": 16, "bf16": 128}

    def __init__(self, data, params, init=None, features=None):
        self.embed_color = params.embed_color                                   # GradFashion.py:28-29
        self.embed_edges = params.embed_edges
        super().__init__(data, params, init, features)
        self.directory_parameters = f'batch_{params.batch_size}-D_{params.embed_d}-K_{params.embed_k}' \
                                    f'-lr_{params.lr}-reg_{params.reg}' + self._hard_suffix()      # GradFashion.py:48-52

    # ---- visual_loader_mixin.py:51-54, 60-69: np.load, each table divided by its OWN global max-abs -------------------
    def process_edge_visual_features(self):
        f = self._features[1] if self._features is not None else np.load(configs.edge_features_path(
            self.params.dataset, getattr(self.params, "cnn_model", "vgg19"), getattr(self.params, "output_layer", "fc2")))
        f = np.asarray(f)
        self.edge_norm = np.max(np.abs(f))
        self.edge_features = f / self.edge_norm
        self.dim_edge_features = self.edge_features.shape[1]

    def process_color_visual_features(self):
        f = self._features[0] if self._features is not None else np.load(configs.hist_color_features_path(self.params.dataset))
        f = np.asarray(f)
        self.color_norm = np.max(np.abs(f))
        self.color_features = f / self.color_norm
        self.dim_color_features = self.color_features.shape[1]

    def padded_features(self):
        """[I, D] float32: [Fc | Fe | zeros], D = Dc + De rounded up to the feature dtype's granule."""
        Dc, De = self.dim_color_features, self.dim_edge_features
        g = self.GRANULE[getattr(self.params, "dtype", "fp32")]
        D = -(-(Dc + De) // g) * g
        F = np.zeros((self.num_items, D), np.float32)
        F[:, :Dc] = self.color_features
        F[:, Dc:Dc + De] = self.edge_features
        return F

    def _init_tables(self, init):
        t, rs = BPRMF._init_tables(self, init)                                  # Bi, Gu, Gi (BPRMF.py:48-50)
        dtype = getattr(self.params, "dtype", "fp32")
        if dtype not in self.GRANULE:
            raise ValueError("GradFashion runs with --dtype fp32 or bf16 (got %s)" % dtype)
        self.process_edge_visual_features()                                     # GradFashion.py:33-34
        self.process_color_visual_features()
        e, d = self.embed_color + self.embed_edges, self.embed_d
        v = {"Bp": glorot_uniform(rs, e, 1).reshape(-1),                        # create_visual_profile, GradFashion.py:73-81
             "E": glorot_uniform(rs, e, d),
             "Tu": glorot_uniform(rs, self.num_users, d)}
        v["Ec"] = glorot_uniform(rs, self.dim_color_features, self.embed_color)  # create_color_features, :59-65
        v["Ee"] = glorot_uniform(rs, self.dim_edge_features, self.embed_edges)   # create_edges_features, :67-71
        v["F"] = self.padded_features()
        self.dim_cnn_features = v["F"].shape[1]
        v.update({k: val for k, val in init.items() if k in v})
        t.update(v)
        return t, rs

    def _build(self, init):
        t, _ = self._init_tables(init)
        self._new_engine().bind_factored(t["Gu"], t["Gi"], t["Bi"], t["Tu"], t["F"], t["Ec"], t["Ee"], t["E"], t["Bp"],
                                  self.dim_color_features, self.dim_edge_features, neg_bias_reg=1.0)

    # ---- the reference's attribute surface ---------------------------------------------------------------------------
    @property
    def feat_cols(self):
        return self.dim_color_features + self.dim_edge_features                 # colour [0, Dc), edges [Dc, Dc + De); F is padded

    @property
    def color_weights(self):
        return {"Fc": self.F[:, :self.dim_color_features], "Ec": self.engine.t["Ec"]}

    @property
    def edges_weights(self):
        Dc = self.dim_color_features
        return {"Fe": self.F[:, Dc:Dc + self.dim_edge_features], "Ee": self.engine.t["Ee"]}

    @property
    def visual_profile(self):
        t = self.engine.t
        return {"Bp": t["Bp"][:, None], "E": t["E"], "Tu": t["Tu"]}

    # ---- GradFashion.py:83-131 ---------------------------------------------------------------------------------------
    def call(self, inputs, training=True, mask=None):
        """xui from the engine (bprx_score_pairs); the other outputs are the reference's gathered rows (theta_i = F_i E_eff:
        the projected rows, recomputed here for inspection only -- the training step never calls this)."""
        u, i = self._pairs(inputs)
        xui = self.engine.score_pairs(u, i)
        t = self.engine.t
        Dc, De = self.dim_color_features, self.dim_edge_features
        Fi = t["F"][i].float()
        theta_i = Fi @ t["E_eff"]
        return xui, t["Gu"][u], t["Gi"][i], Fi[:, :Dc], Fi[:, Dc:Dc + De], t["Tu"][u], theta_i, t["Bi"][i]

    __call__ = call

    # ---- GradFashion.py:269-303 ----------------------------------------------------------------------------------------
    def predict_ui_grads(self, inputs):
        """Gradient x input of x_ui with respect to Fc_i and Fe_i, summed per table: np.float32 [1, 2] (colour, edges)."""
        u, i = inputs
        return self.engine.explain_pairs([int(u)], [int(i)]).cpu().numpy()

    def get_grads_user(self, u, top_k_items):
        """[len(items), 2] for the user's items: one device call for the whole list (the reference maps predict_ui_grads over
        a thread pool, one tape per pair)."""
        items = list(top_k_items)
        if not items:
            return np.zeros((0, 2), np.float32)
        return self.engine.explain_pairs([int(u)] * len(items), items).cpu().numpy()

    def _store_recs(self, path):
        """GradFashion.py:236-240, 252-258: the reference writes the top-K list to the recs path and then OVERWRITES the same
        path with the explanation rows (get_explanations.py:19-21 reads them from there); only the final content is written.
        With params.feat_explain = L > 0 also expl-* / best-expl-* next to it: the L strongest feature columns of the same pairs."""
        expl = run_file(path, "expl") if self.feat_explain > 0 else None
        self.evaluator.store_recommendation_grads(path=path, path_expl=expl, top=self.feat_explain)
        self._store_new_recs(path)

    NORM_KEYS = ("color_norm", "edge_norm")

    def _new_item_table(self, features):
        """(colour rows, edge rows) -> [n, dim_cnn_features] float32 [Fc | Fe | 0], each table divided by its own training divisor."""
        if not isinstance(features, (tuple, list)) or len(features) != 2:
            raise ValueError("GradFashion: new items are a pair (colour rows, edge rows)")
        Dc, De = self.dim_color_features, self.dim_edge_features
        Fc = normalize_new_rows(features[0], self.color_norm, Dc, "colour features")
        Fe = normalize_new_rows(features[1], self.edge_norm, De, "edge features")
        if Fc.shape[0] != Fe.shape[0]:
            raise ValueError("GradFashion: %d colour rows for %d edge rows" % (Fc.shape[0], Fe.shape[0]))
        F = np.zeros((Fc.shape[0], self.dim_cnn_features), np.float32)
        F[:, :Dc], F[:, Dc:Dc + De] = Fc, Fe
        return F

    def _load_new_items(self):
        paths = list(getattr(self.params, "new_items", None) or [])
        return tuple(np.load(p) for p in paths) if paths else None


def normalize_new_rows(raw, norm, width, what="features"):
    """Raw feature rows of new items -> float32 [n, width]: np.asarray(raw) / norm, the arithmetic the training table
    went through (visual_loader_mixin.py:22-31 with the TRAINING max-abs `norm`), then the cast the tables get.  Equal raw rows
    give bit-equal rows.  ValueError unless raw is [n, width]."""
    raw = np.asarray(raw)
    if raw.ndim != 2 or raw.shape[1] != width:
        raise ValueError("new items: %s must be [n, %d], got %s" % (what, width, raw.shape))
    return (raw / norm).astype(np.float32)


def _glorot_1d(rs, n):
    """tf.initializers.GlorotUniform of a 1-D shape [n]: fan_in = fan_out = n."""
    lim = np.sqrt(6.0 / (n + n))
    return rs.uniform(-lim, lim, size=n).astype(np.float32)


def load_acf_features(path, num_items, dtype="fp32", chunk=1024):
    """The per-item feature maps of ACF.py:140-148: `{path}{i}.npy` of shape (1, H, W, C) for every item, NOT normalised,
    as one [I, H*W, C] CPU tensor (float32, or bfloat16 converted chunk by chunk: peak host memory stays near one copy of
    the table).  A missing file or any other shape raises ValueError naming the path and the shape."""
    first = os.path.join(path, "0.npy")
    if not os.path.exists(first):
        raise ValueError("ACF feature map %s is missing" % first)
    shape = np.load(first, mmap_mode="r").shape
    if len(shape) != 4 or shape[0] != 1:
        raise ValueError("ACF feature map %s has shape %s, expected (1, H, W, C)" % (first, shape))
    M, C = shape[1] * shape[2], shape[3]
    out = torch.empty((num_items, M, C), dtype=torch.bfloat16 if dtype == "bf16" else torch.float32)
    buf = np.empty((min(chunk, num_items), M, C), np.float32)
    for s0 in range(0, num_items, chunk):
        n = min(chunk, num_items - s0)
        for q in range(n):
            f = os.path.join(path, "%d.npy" % (s0 + q))
            if not os.path.exists(f):
                raise ValueError("ACF feature map %s is missing" % f)
            a = np.load(f)
            if a.shape != shape:
                raise ValueError("ACF feature map %s has shape %s, expected %s (the shape of 0.npy)" % (f, a.shape, shape))
            buf[q] = a.reshape(M, C)
        out[s0:s0 + n] = torch.from_numpy(buf[:n])
    return out, shape


class ACF(BPRMF):
    """ACF.py:20-270, Attentive Collaborative Filtering: the user profile g'_u = g_u + sum_l alpha_l Pi_l with a component-level
    attention over each history item's feature map and an item-level attention over the history; x_ui = g'_u . Gi_i.  Trained on
    the engine's ACF path (include/bprx.h, bprx_bind_acf) with the reference's DETACHED gradient (g'_u is rebuilt as a new leaf,
    ACF.py:208) unless `params.acf_gradient == "full"`: then the same loss is differentiated through both attention levels
    (bprx_acf_set_gradient; directory_parameters ends in -grad_full and the snapshot records the mode).  Same surface as the reference: Pi, component_weights, item_weights, layers_component, layers_item, call,
    predict_all, train_step, train.  `features`: optional [I, M, C] (or [I, H, W, C]) array used instead of the per-item .npy
    files (not normalised, like the files)."""
    model_kind = "acf"
    hard_models = False

    def __init__(self, data, params, init=None, features=None):
        self.layers_component = [int(x) for x in getattr(params, "layers_component", [64, 1])]
        self.layers_item = [int(x) for x in getattr(params, "layers_item", [64, 1])]
        for name, l in (("layers_component", self.layers_component), ("layers_item", self.layers_item)):
            if len(l) != 2 or l[1] != 1 or l[0] <= 0:
                raise ValueError("ACF: --%s must be two ints 'h 1' with h > 0 (got %s)" % (name, l))
        self._features = features
        self.acf_gradient = getattr(params, "acf_gradient", None) or "detached"
        if self.acf_gradient not in ("detached", "full"):
            raise ValueError("ACF: acf_gradient is 'detached' or 'full' (got %r)" % (self.acf_gradient,))
        self.acf_explain = int(getattr(params, "acf_explain", 0) or 0)            # rows per recommendation in expl-*; 0: none
        if not 0 <= self.acf_explain <= 32:
            raise ValueError("ACF: acf_explain is 0 (off) .. 32 (got %r)" % (self.acf_explain,))
        super().__init__(data, params, init)
        self.directory_parameters = f'batch_{params.batch_size}' \
                                    f'-K_{params.embed_k}' \
                                    f'-lr_{params.lr}' \
                                    f'-reg_{params.reg}' \
                                    f'-comp_{list(self.layers_component)}' \
                                    f'-item_{list(self.layers_item)}'          # ACF.py:46-51
        if self.acf_gradient == "full":                                        # detached runs keep the reference's file names
            self.directory_parameters += '-grad_full'

    def process_cnn_feature_maps(self):
        dtype = getattr(self.params, "dtype", "fp32")
        if dtype not in ("fp32", "bf16"):
            raise ValueError("ACF runs with --dtype fp32 or bf16 (got %s)" % dtype)
        f = self._features
        if f is None:
            path = configs.cnn_features_path_split(self.params.dataset, getattr(self.params, "cnn_model", "vgg19"),
                                                   getattr(self.params, "output_layer", "fc2"))
            self.acf_features, self.feature_shape = load_acf_features(path, self.num_items, dtype)
        else:
            t = torch.as_tensor(np.asarray(f) if not isinstance(f, torch.Tensor) else f)
            if t.dim() == 4:
                self.feature_shape = (1,) + tuple(t.shape[1:])
                t = t.reshape(t.shape[0], t.shape[1] * t.shape[2], t.shape[3])
            elif t.dim() == 3:
                self.feature_shape = (1, int(t.shape[1]), 1, int(t.shape[2]))
            else:
                raise ValueError("ACF features must be [I, M, C] or [I, H, W, C], got shape %s" % (tuple(t.shape),))
            if t.shape[0] != self.num_items:
                raise ValueError("ACF features have %d rows for %d items" % (t.shape[0], self.num_items))
            self.acf_features = t.to(torch.bfloat16 if dtype == "bf16" else torch.float32)

    def _init_tables(self, init):
        t, rs = super()._init_tables(init)                                     # Bi, Gu, Gi (BPRMF.py:48-50)
        self.process_cnn_feature_maps()
        C, k, h, a = int(self.acf_features.shape[2]), self.embed_k, self.layers_component[0], self.layers_item[0]
        v = {"Pi": rs.normal(0.0, 0.01, size=(self.num_items, k)).astype(np.float32)}    # ACF.py:35,54
        v["component.W_0_u"] = glorot_uniform(rs, k, h)                         # build_attention_weights, ACF.py:62-132
        v["component.W_0_i"] = glorot_uniform(rs, C, h)
        v["component.b_0"] = _glorot_1d(rs, h)
        v["component.W_1"] = glorot_uniform(rs, 1, h)
        v["component.b_1"] = _glorot_1d(rs, 1)
        v["item.W_0_u"] = glorot_uniform(rs, k, a)
        v["item.W_0_iv"] = glorot_uniform(rs, k, a)
        v["item.W_0_ip"] = glorot_uniform(rs, k, a)
        v["item.W_0_ix"] = glorot_uniform(rs, C, a)
        v["item.b_0"] = _glorot_1d(rs, a)
        v["item.W_1"] = glorot_uniform(rs, 1, a)
        v["item.b_1"] = _glorot_1d(rs, 1)
        v.update({n: val for n, val in init.items() if n in v})
        t.update(v)
        return t, rs

    def eval_lists(self):
        """P(u) of predict_all: training_list[u] + validation_list[u] (ACF.py:220); the training lists without validation."""
        tr, va = self.data.training_list, self.data.validation_list
        if not va:
            return [list(l) for l in tr]
        return [list(l) + list(va[u]) for u, l in enumerate(tr)]

    def _engine_kwargs(self):
        return dict(model="bprmf", num_users=self.num_users, num_items=self.num_items, embed_k=self.embed_k,
                    feat_dtype=getattr(self.params, "dtype", "fp32"))

    def _adam_form(self):
        return "sweep" if self.optimizer_name == "adam_tf23" else None      # an ACF handle always sweeps (include/bprx.h)

    def _build(self, init):
        t, _ = self._init_tables(init)
        kw = {"gradient": "full"} if self.acf_gradient == "full" else {}
        self._new_engine().bind_acf(t["Gu"], t["Gi"], t["Bi"], self.acf_features, t["Pi"], {n: t[n] for n in _ACF_W},
                             self.data.training_list, self.eval_lists(), **kw)

    # ---- snapshots: the gradient mode is part of a full-mode snapshot; one without the key is detached --------------------
    def state_dict(self):
        sd = super().state_dict()
        if self.acf_gradient == "full":
            sd["acf_gradient"] = "full"
        return sd

    def load_state_dict(self, sd):
        mode = sd.get("acf_gradient", "detached")
        if mode != self.acf_gradient:
            raise ValueError("ACF: the snapshot was taken with acf_gradient=%s, this model runs %s" % (mode, self.acf_gradient))
        super().load_state_dict({n: v for n, v in sd.items() if n != "acf_gradient"})

    # ---- the reference's attribute surface ---------------------------------------------------------------------------
    @property
    def Pi(self):
        return self.engine.t["Pi"]

    @property
    def component_weights(self):
        return {n.split(".", 1)[1]: self.engine.t[n] for n in _ACF_W if n.startswith("component.")}

    @property
    def item_weights(self):
        return {n.split(".", 1)[1]: self.engine.t[n] for n in _ACF_W if n.startswith("item.")}

    def calculate_beta_alpha(self, users, lists=None):
        """g'_u of ACF.py:135-181 for several users at once ([n, k] device tensor; default histories: the training lists)."""
        return self.engine.acf_profiles(users, lists)

    # ---- ACF.py:183-212 ----------------------------------------------------------------------------------------------------
    def call(self, inputs, training=None, mask=None):
        u, i = self._pairs(inputs)
        xui = self.engine.score_pairs(u, i)
        return xui, self.Gu[u], self.Gi[i], self.Pi[i]

    __call__ = call

    # ---- explanations: x_ui = g_u.Gi_i + sum_l alpha_l (Pi_l.Gi_i), both attention levels read out ----------------------------
    def explain(self, users, items, top=5, lists=None, maps=False):
        """The `top` history entries that contribute most to each pair's score (Engine.acf_explain) as numpy arrays: score, base
        [n]; pos, hist_item, alpha, contrib, peak, beta_peak [n, top]; beta [n, top, M] with maps=True (reshape a row to
        feature_shape[:2] for the H x W map).  Default histories: the training lists."""
        return {n: v.cpu().numpy() for n, v in self.engine.acf_explain(users, items, top, lists, maps=maps).items()}

    def explain_ui(self, u, items, top=5, lists=None, maps=False):
        """explain() for one user and several items."""
        items = [int(i) for i in np.asarray(items).reshape(-1)]
        return self.explain([int(u)] * len(items), items, top, lists, maps)

    # ---- users the model was not trained on: the full derivative of the user's own loss, everything but the row frozen ----------
    def fold_in_users(self, histories, steps=30, negatives=4, lr=None, reg=None, optimizer=None, seed=0, init=None):
        """Rows for users who arrive after training with a history of catalogue items each: Gu_new [n, k] (device), fitted by
        Engine.acf_fold_in over the pairs of draw_fold_pairs(histories, num_items, negatives, seed) with the same histories as the
        attention histories.  lr / reg / optimizer: None = the run's.  init: None = zero rows (at g = 0 the gradient is q plus the
        attention terms, not zero: a zero start is live), or the rows to start from.  steps = 0 returns the start rows without a
        kernel call: scored with the history they give the history-only profile g' = g + sum_l alpha_l Pi_l."""
        eng = self.engine
        Gu = fold_start_rows(init, len(histories), eng.k, eng.device)
        if int(steps) == 0:
            return Gu
        ptr, pos, neg = draw_fold_pairs(histories, self.num_items, negatives, seed)
        eng.acf_fold_in(ptr, pos, neg, steps, Gu, lists=histories, lr=self.learning_rate if lr is None else lr,
                        reg=self.reg if reg is None else reg, optimizer=self.optimizer_name if optimizer is None else optimizer,
                        want_loss=False)
        return Gu

    def _fold_rows(self, histories, **fold):
        """The fitted rows and the CSR of their attention histories: ACF scores a row together with its history."""
        return self.fold_in_users(histories, **fold), self.engine.csr(histories)

    def _score_fold_rows(self, rows, r0, r1):
        return self.engine.acf_score_rows_block(rows[0], r0, r1, csr=rows[1]), None

    new_users_param, new_users_side = "acf_new_users", 0
    diverse = False
    because_instead = "--acf_explain"

    def _store_recs(self, path):
        """recs-* / best-recs-* as every model writes them; with params.acf_explain = L > 0 also expl-* / best-expl-* next to them."""
        if self.acf_explain <= 0:
            return super()._store_recs(path)
        self.evaluator.store_recommendation_acf(path, run_file(path, "expl"), self.acf_explain)


AF_EXPLAIN_GRIDS = (0, 1, 2, 4, 7, 8, 14, 16)      # --af_explain: the divisors of 112 whose expl-* rows stay readable


def load_attentive_inputs(dataset, num_items):
    """AttentiveFashion's three per-item inputs (dataset.py:158-208) as CPU tensors: edges uint8 [I, 224, 224] (PIL convert('L'),
    resize((224, 224)); the reference's `/ np.float32(255)` of a uint8 image is applied by the kernels, exactly), colour fp32 [I, Dc]
    with every histogram divided by its OWN max-abs, classes fp32 [I, Dk] as they are.  A missing file raises ValueError naming it; an
    all-zero histogram (a division by zero in the reference) is rejected."""
    from PIL import Image
    ed, cd, kd = configs.edges_path(dataset), configs.hist_color_features_path_dir(dataset), configs.class_features_path_dir(dataset)
    edges = torch.empty((num_items, 224, 224), dtype=torch.uint8)
    color, classes = None, None
    for i in range(num_items):
        for f in (ed + "%d.tiff" % i, cd + "%d.npy" % i, kd + "%d.npy" % i):
            if not os.path.exists(f):
                raise ValueError("AttentiveFashion input %s is missing" % f)
        with Image.open(ed + "%d.tiff" % i) as im:
            edges[i] = torch.from_numpy(np.array(im.convert('L').resize((224, 224)), dtype=np.uint8))
        col = np.asarray(np.load(cd + "%d.npy" % i)).reshape(-1)
        cl = np.asarray(np.load(kd + "%d.npy" % i)).reshape(-1)
        if color is None:
            color = np.empty((num_items, col.size), np.float32)
            classes = np.empty((num_items, cl.size), np.float32)
        if col.size != color.shape[1] or cl.size != classes.shape[1]:
            raise ValueError("AttentiveFashion inputs of item %d have sizes %d / %d, expected %d / %d (the sizes of item 0)"
                             % (i, col.size, cl.size, color.shape[1], classes.shape[1]))
        mx = np.max(np.abs(col))
        if not mx > 0:
            raise ValueError("colour histogram %s is all zero: its max-abs normalisation divides by zero" % (cd + "%d.npy" % i))
        color[i] = col / mx
        classes[i] = cl
    return edges, torch.from_numpy(color), torch.from_numpy(classes)


class AfNewItems(tuple):
    """What AttentiveFashion.prepare_new_items returns: (edges uint8 [n, 224, 224], colour fp32 [n, Dc] normalised, classes fp32
    [n, Dk]) CPU tensors, marked as prepared."""


class AttentiveFashion(BPRMF):
    """AttentiveFashion.py:20-371: x_ui = sum_k g_u * (sum_l alpha_l c_l) * g_i with the encodings c_l of the item's colour
    histogram, edge image and class vector and a three-way attention over them, trained on the engine's AttentiveFashion path
    (include/bprx.h, bprx_bind_attentive) with the reference's full gradient and active dropout.  Same surface as the reference:
    color_encoder / edges_encoder / class_encoder / attention_network (dicts of the bound tensors), attention_layers, call, train_step,
    train, predict_all_batch.  `inputs`: optional (edges uint8 [I, 224, 224], colour [I, Dc] already normalised, classes [I, Dk]) used
    instead of the per-item files."""
    model_kind = "attentive_fashion"
    hard_models = False

    def __init__(self, data, params, init=None, inputs=None):
        self.attention_layers = [int(x) for x in getattr(params, "attention_layers", [64, 1])]
        l = self.attention_layers
        if len(l) != 2 or l[1] != 1 or l[0] <= 0:
            raise ValueError("AttentiveFashion: --attention_layers must be two ints 'h 1' with h > 0 (got %s)" % (l,))
        if getattr(params, "dtype", "fp32") != "fp32":
            raise ValueError("AttentiveFashion runs with --dtype fp32 (got %s)" % params.dtype)
        self.dropout = float(getattr(params, "dropout", 0.5))
        self.af_explain = int(getattr(params, "af_explain", 0) or 0)              # grid of the edge maps in expl-*; 0: none
        if self.af_explain not in AF_EXPLAIN_GRIDS:
            raise ValueError("AttentiveFashion: af_explain is 0 (off) or one of %s (got %r)"
                             % (", ".join(str(g) for g in AF_EXPLAIN_GRIDS[1:]), self.af_explain))
        self._inputs = inputs
        super().__init__(data, params, init)
        self.audience_k = int(getattr(params, "af_audience", 0) or 0)             # users per item in audience-* / warm-audience-*
        self.directory_parameters = f'batch_{params.batch_size}' \
                                    f'-K_{params.embed_k}' \
                                    f'-lr_{params.lr}' \
                                    f'-reg_{params.reg}' \
                                    f'-attlayers_{list(self.attention_layers)}'       # AttentiveFashion.py:275-279

    def _init_tables(self, init):
        # BPRMF.py:48-50 creates Bi, Gu, Gi with ITS initialiser (Glorot uniform): AttentiveFashion.py:24 assigns RandomNormal(0.01)
        # only afterwards, and nothing reads it.  Then the Keras layers in creation order (Glorot-uniform kernels, zero biases),
        # then the attention tensors (Glorot uniform, biases included: AttentiveFashion.py:118-144).
        t, rs = super()._init_tables(init)
        if self._inputs is None:
            self._inputs = load_attentive_inputs(self.params.dataset, self.num_items)
        self.edges, self.color, self.classes = (torch.as_tensor(np.asarray(x) if not isinstance(x, torch.Tensor) else x)
                                                for x in self._inputs)
        Dc, Dk, k, h = int(self.color.shape[1]), int(self.classes.shape[1]), self.embed_k, self.attention_layers[0]
        lim = np.sqrt(6.0 / (25 * 1 + 25 * 64))                                  # Conv2D fans: 5*5*in, 5*5*out
        v = {"color.W1": glorot_uniform(rs, Dc, 256), "color.b1": np.zeros(256, np.float32), "color.W2": glorot_uniform(rs, 256, k),
             "edges.conv": rs.uniform(-lim, lim, size=(25, 64)).astype(np.float32), "edges.conv_b": np.zeros(64, np.float32),
             "edges.W2": glorot_uniform(rs, 64, k),
             "class.W1": glorot_uniform(rs, Dk, 256), "class.b1": np.zeros(256, np.float32), "class.W2": glorot_uniform(rs, 256, k),
             "attention.W_1": glorot_uniform(rs, k, h), "attention.b_1": _glorot_1d(rs, h),
             "attention.W_2": glorot_uniform(rs, h, 1), "attention.b_2": _glorot_1d(rs, 1)}
        v.update({n: val for n, val in init.items() if n in v})
        t.update(v)
        return t, rs

    def _adam_form(self):
        return "sweep" if self.optimizer_name == "adam_tf23" else None      # the handle always sweeps (include/bprx.h)

    def _build(self, init):
        t, _ = self._init_tables(init)
        self._new_engine(min_batch=1024).bind_attentive(t["Gu"], t["Gi"], t["Bi"], self.edges, self.color, self.classes, {n: t[n] for n in _AF_W},
                                   dropout=self.dropout, seed=getattr(self.params, "init_seed", 0))

    # ---- the reference's attribute surface ---------------------------------------------------------------------------
    def _group(self, prefix):
        return {n.split(".", 1)[1]: self.engine.t[n] for n in _AF_W if n.startswith(prefix + ".")}

    color_encoder = property(lambda self: self._group("color"))
    edges_encoder = property(lambda self: self._group("edges"))
    class_encoder = property(lambda self: self._group("class"))
    attention_network = property(lambda self: self._group("attention"))

    # ---- AttentiveFashion.py:168-209 (dropout off, as a call outside train_step) -------------------------------------------------
    def call(self, inputs, training=None, mask=None):
        u, i = self._pairs(inputs)
        xui, alpha = self.engine.af_attention_pairs(u, i)
        c = self.engine.af_encode(i)
        return xui, self.Gu[u], self.Gi[i], c[0], c[1], c[2], alpha

    __call__ = call

    # ---- AttentiveFashion.py:325-371 ------------------------------------------------------------------------------------------------
    def predict_all_batch(self, step=None, next_image=None, user_block=256):
        """Scores [U, I] and attentions [U, I, 3] as numpy arrays, user block by user block.  Every item is encoded once per call
        (the reference re-encodes every item for every user, and fails when num_items % batch_eval == 0); `step` / `next_image` are
        accepted for the reference's signature and ignored."""
        xs, als = [], []
        for u0, u1 in blocks(self.num_users, user_block):
            x, al = self.engine.af_score_block(u0, u1)
            xs.append(x.cpu().numpy()); als.append(al.cpu().numpy())
        return np.concatenate(xs), np.concatenate(als)

    def state_dict(self):
        sd = super().state_dict()
        sd["dropout_step"] = self.engine.af_step
        return sd

    def load_state_dict(self, sd):
        sd = dict(sd)
        step = sd.pop("dropout_step", None)
        super().load_state_dict(sd)
        if step is not None:
            self.engine.af_step = step

    # ---- explanations: x_ui = sum_l alpha_l t_l, and the edges share over a grid of the pooled edge image ----------------------
    def explain(self, users, items, grid=14, maps=True):
        """The exact split of each pair's score (Engine.af_explain) as numpy arrays: score [n], alpha [n, 3], parts [n, 3] (colour,
        edges, class: alpha_l * t_l, they sum to score), peak_cell, peak_val [n] and with maps=True map [n, grid * grid] (reshape a
        row to (grid, grid) for the image; the cells sum to parts[:, 1]).  alpha is held fixed at the value the model reports."""
        return {n: v.cpu().numpy() for n, v in self.engine.af_explain(users, items, grid, maps=maps).items()}

    def explain_ui(self, u, items, grid=14, maps=True):
        """explain() for one user and several items."""
        items = [int(i) for i in np.asarray(items).reshape(-1)]
        return self.explain([int(u)] * len(items), items, grid, maps)

    # ---- users the model was not trained on: the reference's step on one user's pairs, everything else frozen, dropout off -------
    def fold_in_users(self, histories, steps=30, negatives=4, lr=None, reg=None, optimizer=None, seed=0, init=None):
        """Rows for users who arrive after training with a history of catalogue items each: Gu_new [n, k] (device), fitted by
        Engine.af_fold_in over the pairs of draw_fold_pairs(histories, num_items, negatives, seed).  lr / reg / optimizer: None =
        the run's.  init: None = zero rows (at g = 0 the gradient is (sum_l alpha_l c_l) * Gi, not zero: a zero start is live), or
        the rows to start from."""
        eng = self.engine
        n = len(histories)
        ptr, pos, neg = draw_fold_pairs(histories, self.num_items, negatives, seed)
        Gu = fold_start_rows(init, n, eng.k, eng.device)
        eng.af_fold_in(ptr, pos, neg, steps, Gu, lr=self.learning_rate if lr is None else lr, reg=self.reg if reg is None else reg,
                       optimizer=self.optimizer_name if optimizer is None else optimizer, want_loss=False)
        return Gu

    def _score_fold_rows(self, rows, r0, r1):
        return self.engine.af_score_rows_block(rows, r0, r1)

    new_users_param, new_users_side = "af_new_users", 3
    diverse = False
    because_instead = "--af_explain"

    # ---- items the model was not trained on, once they have first buyers: x_ur is linear in Gi_r (include/bprx.h) ----------------
    warm_param = "af_warm_items"

    def prepare_new_items(self, edges, color, classes):
        """The inputs of n new items as the encoders take them, an AfNewItems of CPU tensors: edges uint8 [n, 224, 224] as they
        are, colour fp32 [n, Dc] with every raw histogram divided by its OWN max-abs (an all-zero row is rejected: the rule of
        load_attentive_inputs), classes fp32 [n, Dk].  ValueError for shapes that do not match the bound Dc and Dk."""
        Dc, Dk = int(self.color.shape[1]), int(self.classes.shape[1])
        ed, col, cl = np.asarray(edges), np.asarray(color), np.asarray(classes)
        if ed.dtype != np.uint8 or ed.ndim != 3 or ed.shape[1:] != (224, 224):
            raise ValueError("new items: edges must be uint8 [n, 224, 224], got %s %s" % (ed.dtype, ed.shape))
        n = ed.shape[0]
        if col.shape != (n, Dc) or cl.shape != (n, Dk):
            raise ValueError("new items: colour must be [%d, %d] and classes [%d, %d], got %s and %s" % (n, Dc, n, Dk, col.shape, cl.shape))
        mx = np.max(np.abs(col), axis=1) if n else np.zeros(0)
        if not np.all(mx > 0):
            raise ValueError("new items: the colour histogram of row %d is all zero: its max-abs normalisation divides by zero"
                             % int(np.flatnonzero(~(mx > 0))[0]))
        return AfNewItems((torch.from_numpy(np.ascontiguousarray(ed)), torch.from_numpy((col / mx[:, None]).astype(np.float32)),
                           torch.from_numpy(np.ascontiguousarray(cl, dtype=np.float32))))

    def fold_in_items(self, buyers, features=None, steps=30, negatives=4, lr=None, reg=None, optimizer=None, seed=0, init=None):
        """Rows for items that arrive after training, from their first buyers (buyers[r]: the catalogue users who bought new item
        r): (Gi_new [n, k], C_new [3, n, k]) device tensors.  features: (edges, colour, classes) raw, as prepare_new_items takes
        them, or what it returned.  C_new = Engine.af_encode_new of them; Gi_new is fitted by Engine.af_fold_in_items over the
        pairs of draw_item_fold_pairs(buyers, training_list, num_items, negatives, seed), everything else frozen, dropout off.
        lr / reg / optimizer: None = the run's.  init: None = zero rows, or the Gi rows to start from.  An item without buyers
        keeps its start row: from zeros it scores 0.0 for everyone.  With plain sgd the step size must shrink with the number of
        pairs (the batch loss is summed); Adam, the default, does not care."""
        eng = self.engine
        n = len(buyers)
        if features is None:
            raise ValueError("AttentiveFashion: fold_in_items needs the new items' (edges, colour, classes)")
        feats = features if isinstance(features, AfNewItems) else self.prepare_new_items(*features)
        if len(feats[0]) != n:
            raise ValueError("AttentiveFashion: %d buyer lists for %d new items" % (n, len(feats[0])))
        ptr, user, other, role = draw_item_fold_pairs(buyers, self.data.training_list[:self.num_users], self.num_items, negatives, seed)
        Gi = fold_start_rows(init, n, eng.k, eng.device)
        if n == 0:
            return Gi, torch.zeros((3, 0, eng.k), dtype=torch.float32, device=eng.device)
        C = eng.af_encode_new(*feats)
        eng.af_fold_in_items(ptr, user, other, role, steps, C, Gi, lr=self.learning_rate if lr is None else lr,
                             reg=self.reg if reg is None else reg, optimizer=self.optimizer_name if optimizer is None else optimizer,
                             want_loss=False)
        return Gi, C

    warm_side = 3                                                # (Gi_new, C_new) rows; every block comes with its attentions

    def _score_warm_block(self, rows, b0, b1):
        return self.engine.af_score_warm_block(b0, b1, rows[1], rows[0])

    def _audience_warm_block(self, rows, b0, b1):
        return self.engine.af_audience_block(b0, b1, rows[1], rows[0])

    def _audience_block(self, b0, b1):
        return self.engine.af_audience_block(b0, b1)

    def _store_audience(self, path):
        """params.af_audience = K > 0: audience-* next to the recs-* file at `path`, rows 'i\tu\tscore\talpha_colour\talpha_edges\t
        alpha_class', item by item over the whole catalogue, best first."""
        if self.audience_k > 0:
            self.evaluator.store_audience(item_file(path, "audience"), None)

    def _load_new_items(self):
        """The tables of params.af_new_items (edges, colour, classes), prepared; None without the flag."""
        src = getattr(self.params, "af_new_items", None)
        if not src:
            return None
        return self.prepare_new_items(*(np.load(p) for p in src))

    def _store_recs(self, path):
        """recs-* / best-recs-* with the attentions; with params.af_explain = G > 0 also expl-* / best-expl-* next to them."""
        if self.af_explain <= 0:
            return self.evaluator.store_recommendation_attention(path=path)
        self.evaluator.store_recommendation_attention_explain(path, run_file(path, "expl"), self.af_explain)


from ._ffi import ACF_WEIGHTS as _ACF_W     # noqa: E402
from ._ffi import AF_WEIGHTS as _AF_W       # noqa: E402
