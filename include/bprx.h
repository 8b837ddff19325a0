/*
 * bprx.h -- C ABI of libbprx.so: the MI355X (gfx950) BPRMF / VBPR training hot path.
 *
 * The reference (peternara/FashionVisualExpl-recommend) has NO native plugin/FFI interface for this
 * path: it is TensorFlow-2.3 eager Python.  Its boundary is the Python class surface
 *     src/recommender/models/BPRMF.py:55  call            :78  predict_all   :87  train_step
 *     src/recommender/models/VBPR.py:59   call            :88  predict_all   :99  train_step
 *     src/dataset/dataset.py:83           all_triple_batches (index stream)
 *     src/recommender/Evaluator.py:82     _eval_by_user     (HR/nDCG/AUC/P/R definition)
 * Each entry point below names the reference lines it replaces.  INTEGRATION.md shows the ctypes stub a
 * maintainer of the reference would add.  Plain pointers and sizes only: no torch / TF types.
 *
 * Conventions
 *   - Every function returns 0 on success, a negative BPRX_E_* code otherwise; bprx_last_error() gives text.
 *     No exception crosses the ABI.  Index range errors are detected on the device and reported by the next
 *     bprx_sync_check() (indices are clamped so that no kernel ever faults).
 *   - All table / index / output pointers are DEVICE pointers owned by the caller (e.g. torch tensors); the
 *     handle owns only its scratch.  `stream` is a hipStream_t passed as void* (NULL = default stream);
 *     all work is enqueued, nothing synchronises unless stated.
 *   - A handle is bound to one device and is not re-entrant.  One process per GPU.
 *   - Tables are row-major fp32 exactly like the reference's tf.Variables (BPRMF.py:48-50, VBPR.py:44-54).
 *     F may be fp32 [I,D] or bf16 [I,D] (raw uint16 bit patterns).
 */
#ifndef BPRX_H_
#define BPRX_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BPRX_ABI_VERSION 6

#if defined(__GNUC__)
#define BPRX_API __attribute__((visibility("default")))
#else
#define BPRX_API
#endif

enum { BPRX_MODEL_BPRMF = 0, BPRX_MODEL_VBPR = 1 };
enum { BPRX_OPT_SGD = 0, BPRX_OPT_ADAM_TF23 = 1 };
enum { BPRX_F_FP32 = 0, BPRX_F_BF16 = 1, BPRX_F_FP8 = 2 };   /* FP8: OCP e4m3fn codes, see feat_scale */

enum {
  BPRX_OK = 0,
  BPRX_E_INVALID = -1,   /* bad argument / unsupported configuration */
  BPRX_E_STATE = -2,     /* call order (tables not bound, ...) */
  BPRX_E_HIP = -3,       /* HIP runtime error */
  BPRX_E_RANGE = -4,     /* an index was out of range (seen by bprx_sync_check) */
  BPRX_E_NOMEM = -5
};

typedef struct bprx_handle bprx_handle;
typedef struct bprx_sampler bprx_sampler;

typedef struct {
  int32_t abi_version;   /* BPRX_ABI_VERSION */
  int32_t model;         /* BPRX_MODEL_*            train_rec.py:75-78 (--rec bprmf|vbpr) */
  int32_t num_users;     /* rows of Gu/Tu held by THIS handle (a shard when user-sharded) */
  int32_t num_items;     /* rows of Gi/Bi/F held by THIS handle (a shard when item-sharded) */
  int32_t embed_k;       /* --embed_k  train_rec.py:42 */
  int32_t embed_d;       /* --embed_d  train_rec.py:43 (VBPR only, else 0) */
  int32_t feat_dim;      /* D = F.shape[1]  visual_loader_mixin.py:31 (VBPR only, else 0) */
  int32_t feat_dtype;    /* BPRX_F_* */
  int32_t optimizer;     /* BPRX_OPT_* ; reference = Adam (BPRMF.py:52, VBPR.py:56) */
  int32_t device;        /* HIP device ordinal */
  int64_t max_batch;     /* largest B any bprx_step/bprx_score_pairs call will use */
  float lr;              /* --lr   train_rec.py:28 */
  float reg;             /* --reg  train_rec.py:44,69 */
  float beta1, beta2, epsilon; /* adam_tf23: 0.9, 0.999, 1e-7 (tf.optimizers.Adam defaults) */
  int32_t flags;         /* BPRX_FLAG_* */
  float feat_scale;      /* BPRX_F_FP8: F holds e4m3fn(f * feat_scale), i.e. f ~ F / feat_scale (448 for max-abs-normalised
                            features, visual_loader_mixin.py:30); ignored otherwise */
} bprx_config;

/* BPRX_FLAG_EXPORT_USER_GRAD (item-sharded multi-GPU; with adam_tf23 see bprx_adam_rows): the bound Gu/Tu are per-step STAGING rows fetched from
   their owner ranks (row b = the user row of triplet b); the step leaves their summed gradients in the buffers of
   bprx_user_grad() instead of applying them, and the caller routes those rows back to the owners
   (bprx_scatter_add with scale = -lr) and clears them with bprx_clear_user_grad(). */
enum { BPRX_FLAG_EXPORT_USER_GRAD = 1, BPRX_FLAG_EXPORT_ITEM_GRAD = 2, BPRX_FLAG_DENSE_ALLREDUCE = 4,
       BPRX_FLAG_ADAM_SWEEP = 8, BPRX_FLAG_ADAM_LAZY = 16 };
/* BPRX_FLAG_ADAM_SWEEP / BPRX_FLAG_ADAM_LAZY: the caller's choice of adam_tf23's form (whole-table sweeps / lazily-exact replay:
   the same arithmetic) instead of bprx_create's estimate from num_users and max_batch -- a caller that knows the real batch size
   and the number of training interactions knows the replay depth (interactions / batch) exactly.  See bprx_adam_is_lazy. */
/* BPRX_FLAG_DENSE_ALLREDUCE (with BPRX_FLAG_EXPORT_USER_GRAD, replicated-user step): the per-rank message carries NO dense
   part; the caller all-reduces (sum, RCCL) the buffer of bprx_dense_grad() between bprx_pack_user_msg and bprx_step_end --
   the "RCCL all-reduce on E / beta'" form of SURVEY 8(e).  Without it dE|dBp rides in the all-gathered message and is summed
   in rank order (bit-identical replicas whatever the collective's reduction order). */
/* BPRX_FLAG_EXPORT_ITEM_GRAD (user-sharded multi-GPU BPRMF; with adam_tf23 see bprx_adam_rows): the mirror image -- the bound Gi/Bi are per-step
   STAGING rows fetched from the item owners (row b = the positive item row of triplet b, row B+b its negative item row);
   their gradients are left in the buffers of bprx_item_grad() and cleared with bprx_clear_item_grad(). */

/* Device pointers to the model state.  Unused entries (BPRMF: Tu,F,E,Bp; sgd: every m_/v_) are NULL. */
typedef struct {
  float *Gu;       /* [U,k]  BPRMF.py:49 */
  float *Gi;       /* [I,k]  BPRMF.py:50 */
  float *Bi;       /* [I]    BPRMF.py:48 */
  float *Tu;       /* [U,d]  VBPR.py:46  */
  const void *F;   /* [I,D]  VBPR.py:49, frozen; fp32, bf16 or fp8 (e4m3fn) per feat_dtype */
  float *E;        /* [D,d]  VBPR.py:52  */
  float *Bp;       /* [D]    VBPR.py:44 ([D,1]) */
  float *m_Gu, *v_Gu, *m_Gi, *v_Gi, *m_Bi, *v_Bi, *m_Tu, *v_Tu, *m_E, *v_E, *m_Bp, *v_Bp; /* Adam slots */
} bprx_tables;

BPRX_API int bprx_abi_version(void);

/* Model(data, params) constructor scratch (BPRMF.py:23-53, VBPR.py:19-57). */
BPRX_API int bprx_create(const bprx_config *cfg, bprx_handle **out);
BPRX_API int bprx_destroy(bprx_handle *h);
BPRX_API const char *bprx_last_error(const bprx_handle *h); /* h == NULL: error of the last failed bprx_create */
BPRX_API int64_t bprx_live_device_allocs(void); /* device buffers the library holds right now, all handles of the process */

/* Binds caller-owned device tables (they stay owned by the caller and are updated in place by the steps).
   bf16 / fp8 features: F is frozen (visual_loader_mixin.py:22-31) -- this call copies it ONCE into a tiled layout the
   projections read (synchronous; work is enqueued on the null stream, so F must be complete with respect to it); the
   caller's F is not read again until the next bprx_bind_tables and may be released.
   A handle is not thread-safe; all other entry points only enqueue work on the stream they are given. */
BPRX_API int bprx_bind_tables(bprx_handle *h, const bprx_tables *t);
/* The bound tables stay owned by the caller, who may write them between calls (restoring a snapshot: the reference
   deep-copies / checkpoints the whole model, BPRMF.py:156-160,177-179).  The handle keeps images DERIVED from them across
   calls -- the bf16/fp8 image of [E|Bp]^T and the item projections P = F.[E|Bp] that bprx_score_block / bprx_score_pairs
   reuse until a step changes E/Bp -- so after writing any bound table from outside the library call bprx_tables_dirty()
   before the next library call.  (bprx_bind_tables implies it.)  `stream`: the stream the outside writes were enqueued on --
   the lazy-Adam bookkeeping reset is ordered behind them there (NULL: the null stream, synchronised). */
BPRX_API int bprx_tables_dirty(bprx_handle *h, void *stream);
BPRX_API int bprx_set_hyper(bprx_handle *h, float lr, float reg);           /* train_rec.py:69 (args.reg = reg) */
BPRX_API int bprx_set_adam_step(bprx_handle *h, int64_t iterations, void *stream);   /* optimizer.iterations (resume); stream as above */
/* adam_tf23 is implemented LAZILY but exactly: TF-2.3's Adam moves every row of every table every step (non-lazy sparse
   apply, BPRMF.py:123 / VBPR.py:142); here a row that received no gradient is brought up to date -- by replaying the
   skipped steps with the arithmetic of the whole-table sweep, bit for bit -- when it is next read.  The library does that
   itself wherever IT reads the tables (steps, bprx_score_pairs, bprx_score_block); a caller that reads the bound tensors
   directly (snapshot, inspection) calls bprx_sync_adam first: afterwards every row holds what TF's tables would hold after
   optimizer.iterations steps.  No-op for sgd, or when nothing is pending.  (BPRX_ADAM_LAZY=0: the sweeps, for A/B.) */
BPRX_API int bprx_sync_adam(bprx_handle *h, void *stream);
/* The deferred dense update.  A bprx_step of a plain VBPR handle that is not asked for its loss does not launch its dense E|Bp
   update: the next segment-mode bprx_step runs it inside its index-pass launch (k_index_seg), on compute units that launch leaves
   idle, with the hyper-parameters of the step it belongs to (a bprx_set_hyper in between does not reach it).  Every other entry
   that takes a handle first runs a pending update with the stand-alone kernel on ITS stream, so the library itself never sees a
   stale E / Bp; bprx_destroy drops it.  A caller that reads the bound E / Bp (or their Adam slots) directly calls bprx_settle
   first, as it calls bprx_sync_adam: it returns at once when nothing is pending.  bprx_dense_pending: 1 while an update waits.
   bprx_set_loss_lag(h, 1) lets a step WITH a loss pointer defer too: its loss is then written behind the launch that runs its
   update (the next step, or a settling call), so the pointer must stay valid until then; the value has the same bits.  Before the
   buffer goes: bprx_settle, then bprx_set_loss_lag(h, 0) -- on every way out of the loop that set it.
   BPRX_DENSE_DEFER=0 (read by bprx_create): never defer.  The split-phase calls never defer.
   Every entry checks its arguments, then passes one gate that brings the handle to the state the entry reads (pending update,
   lazy-Adam rows, the [E|Bp]^T image, P), then returns if there is no work.  So a call rejected for its arguments (or for the
   handle, BPRX_E_STATE not bound / BPRX_E_INVALID a handle of the wrong kind) launches nothing and leaves an update pending; a
   valid call with no work (B == 0, n == 0, u0 == u1) settles like any other.
     entries                                                          handle              tables bound  rows  image  P of all items
     bprx_score_block                                                 any                 yes           yes   via P  yes (VBPR)
     bprx_score_rows_block, bprx_fold_in                              BPRMF / VBPR        yes           yes   via P  yes
     bprx_audience_block, Pq == NULL                                  BPRMF / VBPR        yes           yes   via P  yes
     bprx_audience_block, Pq != NULL                                  VBPR, not fp8       yes           yes   yes    -
     bprx_af_fold_in, bprx_af_score_rows_block                        AttentiveFashion    yes           -     -      -
     bprx_af_encode_new, bprx_af_fold_in_items, bprx_af_score_warm_block, bprx_af_audience_block   AttentiveFashion   yes   -   -   -
     bprx_acf_fold_in, bprx_acf_profile_rows, bprx_acf_score_rows_block   ACF             yes           -     -      -
     bprx_step_project                                                any                 yes           -     yes    yes
     bprx_score_pairs                                                 any                 yes           yes   unless P is current  -
     bprx_project_rows, bprx_score_new_block, bprx_feat_explain_new   VBPR, not fp8       yes           yes   yes    -
     bprx_feat_explain                                                VBPR                yes           yes   -      -
     bprx_explain_pairs                                               GradFashion         yes           yes   -      -
     bprx_sim_*, bprx_style_*, bprx_diversify, bprx_because           BPRMF / VBPR        yes           yes   via P  VISUAL / BOTH
     bprx_sync_adam                                                   any                 yes           yes   -      -
     bprx_topk_rows                                                   VBPR, not fp8       yes           -     -      -
     bprx_apply_user_msgs                                             any                 yes           -     -      -
     bprx_sum_dense_parts                                             VBPR                -             -     -      -
     bprx_topk, bprx_topk_lists, bprx_topk_rows_masked, bprx_topk_classes, bprx_eval_*, bprx_tables_dirty, bprx_set_adam_step, bprx_clear_*_grad, bprx_sync_check,
     bprx_pack_user_msg, the bind calls                               any                 -             -     -      -
   Not behind the gate: bprx_step and bprx_step_begin[_sparse] (a step may carry the update), the samplers, the profile calls, bprx_last_error, bprx_set_hyper,
   bprx_set_loss_lag, the getters, bprx_settle and bprx_dense_pending; bprx_calibrate (it reads pools, histories and a class table of
   the caller's, no state of the handle). */
BPRX_API int bprx_settle(bprx_handle *h, void *stream);
BPRX_API int bprx_dense_pending(const bprx_handle *h);
BPRX_API int bprx_set_loss_lag(bprx_handle *h, int on);
BPRX_API int64_t bprx_get_adam_step(const bprx_handle *h);
/* 1: adam_tf23 runs lazily-exact on this handle (per-row replay, bprx_sync_adam meaningful), 0: by whole-table sweeps.  Chosen at
   bprx_create from the table sizes and max_batch (BPRX_ADAM_LAZY=0 / 1 forces it); the arithmetic is the same. */
BPRX_API int bprx_adam_is_lazy(const bprx_handle *h);

/* ---- GradFashion (GradFashion.py:57-193) on a VBPR handle ----------------------------------------------------------
   The reference's score is linear in its factored projection:
       vf_i = [Fc_i Ec | Fe_i Ee]            x_ui = Bi_i + Gu_u.Gi_i + Tu_u.(vf_i E) + vf_i.Bp       (GradFashion.py:98-131)
   i.e. VBPR with F = [Fc | Fe | zero padding] and the EFFECTIVE projection
       E_eff  = [Ec E[:ec] ; Ee E[ec:] ; 0]  [D, d]        Bp_eff = [Ec Bp[:ec] ; Ee Bp[ec:] ; 0]  [D].
   bprx_bind_factored binds a VBPR handle (fp32 or bf16 features; fp8 is rejected with BPRX_E_INVALID) whose t->E / t->Bp are
   caller-owned buffers of E_eff / Bp_eff that the LIBRARY writes (composed at bind, after every step and by bprx_tables_dirty);
   t->m_E / v_E / m_Bp / v_Bp are unused.  The trainable dense tables are the four factors below; each step takes the chain rule
   of the VBPR dense gradient G = dL/d[E_eff|Bp_eff] into them:
       dEc = G_c [E|Bp][:ec]^T + 2 reg Ec       d[E|Bp][:ec] = Ec^T G_c + 2 reg [E|Bp][:ec]     (edges likewise, rows Dc..Dc+De)
   with sgd or TF-2.3's dense ApplyAdam form (GradFashion.py:182-190), and the loss gains reg*(|Ec|^2+|Ee|^2+|E|^2+|Bp|^2)
   (GradFashion.py:177-180).  The negative item's bias is regularised with factor neg_bias_reg (1.0 in GradFashion.py:175-176;
   VBPR.py:125 / BPRMF have 0.1, the default of every handle).  Everything else (bprx_step, _begin / _end, score_pairs,
   score_block, eval_*, topk, sync_adam) works unchanged; the caller's F must stay valid while bprx_explain_pairs is used
   (it reads the caller's F).  Multi-GPU (exported gradients) is not supported. */
typedef struct {
  int32_t feat_dim_a, feat_dim_b;   /* Dc, De: F = [Fc | Fe | zero padding] (visual_loader_mixin.py:51-54, 60-69); Dc + De <= feat_dim */
  int32_t embed_a, embed_b;         /* --embed_color, --embed_edges (GradFashion.py:28-29); 1..256 each */
  float neg_bias_reg;               /* 1.0 for GradFashion (GradFashion.py:175-176) */
  float *Ea, *Eb, *A, *Ap;          /* Ec [Dc,ec], Ee [De,ee], E [ec+ee,d], Bp [ec+ee] (GradFashion.py:59-81) */
  float *m_Ea, *v_Ea, *m_Eb, *v_Eb, *m_A, *v_A, *m_Ap, *v_Ap;   /* adam_tf23 slots (NULL with sgd) */
} bprx_factored;
BPRX_API int bprx_bind_factored(bprx_handle *h, const bprx_tables *t, const bprx_factored *f);
/* GradFashion.predict_ui_grads (GradFashion.py:269-292): gradient x input of x_ui with respect to Fc_i and Fe_i, summed --
   exact for the linear score:  out[p] = { (Fc_i Ec).(E[:ec] Tu_u + Bp[:ec]),  (Fe_i Ee).(E[ec:] Tu_u + Bp[ec:]) }, fp32 [n,2].
   user / item: device int32 [n]; any n >= 0 (not bounded by max_batch). */
BPRX_API int bprx_explain_pairs(bprx_handle *h, const int32_t *user, const int32_t *item, int64_t n, float *out, void *stream);

/* ---- VBPR and GradFashion: the score per feature column ------------------------------------------------------------------
   The linear score of a bound VBPR handle, plain or factored, decomposes exactly:
       x_ui = Bi_i + Gu_u.Gi_i + sum_c F_ic w_uc        w_uc = Bp[c] + sum_x E[c,x] Tu[u,x]
              `---- base ----'   `--- visual ---'
   F_ic w_uc is gradient x input of x_ui with respect to feature column c -- the quantity GradFashion.predict_ui_grads sums per
   modality (a factored handle's E / Bp are E_eff / Bp_eff: columns [0, Dc) are the colour histogram, [Dc, Dc + De) the edges).
   F: device pointer to the caller's ROW-MAJOR [num_items, feat_dim] table in the handle's feat_dtype (fp32, bf16, or e4m3fn codes
   of f * feat_scale); it is passed here because bprx_bind_tables allows a bf16 / fp8 F to be released once the tiled copy is
   made -- this call never reads the tiled copy.  Only columns [0, ncols) exist for the explanation (1 <= ncols <= feat_dim: the
   rest is the models' zero padding); 1 <= top <= 32; 0 <= n < 2^31, not bounded by max_batch (n == 0: BPRX_OK, no output
   is written); feat_dim <= 16384 (one user's fp32 w row lives in LDS).  BPRX_E_INVALID otherwise and for a NULL pointer other than
   map, and on a BPRMF, ACF or AttentiveFashion handle; BPRX_E_STATE on an unbound one.  After any error the handle stays usable.
   Outputs (device): score, base, visual fp32 [n]; col int32 [n, top] and contrib fp32 [n, top]: the `top` columns with the
   largest F_ic w_uc, rank 0 first, non-increasing; values compare as floats (+0.0 == -0.0, as in bprx_topk) and equal values come
   in ascending column order; slots r >= ncols hold col = -1, contrib = 0.  map fp32 [n, ncols] (row stride ncols; NULL: not
   written): every F_ic w_uc.
   Precision: E, Bp, Tu, Gu, Gi, Bi are read as the fp32 master tables, and the features are dequantised exactly (bf16 -> fp32;
   an fp8 code's value / feat_scale).  With bf16 / fp8 features bprx_score_pairs goes through a ROUNDED image of [E|Bp]^T: `score`
   here does not, and differs from bprx_score_pairs by that rounding.  w_uc is a function of (E[c,:], Bp[c], Tu_u) alone (one
   fma chain in the order of x): columns with bit-equal E rows, Bp and features give bit-equal contributions.  score == base +
   visual as one fp32 add; visual is the sum of the row's contributions in a fixed order; contrib[p, r] is bit-equal to
   map[p, col[p, r]].  No float atomics: two calls return the same bits.
   Indices out of range are clamped and reported by bprx_sync_check (BPRX_E_RANGE), as for bprx_explain_pairs.  Lazy adam_tf23
   rows are brought up to date first (as bprx_score_pairs does); apart from that the call writes its outputs only: no table, Adam
   slot, step counter or cached projection changes, and nothing is allocated. */
BPRX_API int bprx_feat_explain(bprx_handle *h, const void *F, const int32_t *user, const int32_t *item, int64_t n, int32_t ncols,
                               int32_t top, float *score, float *base, float *visual, int32_t *col, float *contrib, float *map,
                               void *stream);

/* ---- VBPR and GradFashion: items the model was not trained on ------------------------------------------------------------
   An item that is not in the bound catalogue has no Gi_j and no Bi_j; what the trained weights say about it is the visual part
   of the score (the cold-start score of the VBPR paper):
       x_uj = Tu_u.(f_j E) + f_j.Bp
   (a factored handle: E_eff / Bp_eff).  The five calls below score, rank and explain the n rows of a caller-owned ROW-MAJOR
   device table Fnew [n, feat_dim] of the handle's feat_dtype, normalised by the caller as the training table was.
   Handles: a bound VBPR handle, plain or factored, with fp32 or bf16 features.  BPRX_E_INVALID for a NULL handle, a BPRMF, ACF or
   AttentiveFashion handle, an fp8 handle (a new row may exceed the max-abs the codes were scaled for and would saturate), a NULL
   pointer, n < 0, n >= 2^31; BPRX_E_STATE for an unbound handle; n == 0 / u0 == u1: BPRX_OK, no output is written.  After any error
   the handle stays usable.
   State: bprx_project_rows, bprx_score_new_block and bprx_feat_explain_new bring lazy adam_tf23 rows up to date first (they read
   Tu, E, Bp) and make the bf16 image of [E|Bp]^T current where the step has not left it so (the image every projection of the
   handle reads); apart from that they write their outputs only.  No table, Adam slot, step counter or cached projection
   changes, nothing is allocated: a training run with these calls between its steps ends bit-identical to one without them. */
/* PS = 16 * ceil((embed_d + 1) / 16), the row stride of P below; negative (BPRX_E_INVALID) for a NULL or non-VBPR handle. */
BPRX_API int32_t bprx_proj_stride(const bprx_handle *h);
/* P[j, 0:d] = f_j.E, P[j, d] = f_j.Bp, P[j, d+1:PS] = 0 for the n rows of Fnew.  P: fp32 [n, PS], caller-owned.
   bf16 features (k_proj_new_bf16): one pass over the table, every feature byte read once, against the SAME bf16-rounded
   [E|Bp] that projects the catalogue (fp32 accumulation): new and old items sit on one scale.  fp32 features: the fp64-accumulating
   kernels of the catalogue.  A row's result depends on its own bytes, E and Bp only: the same feature row gives the same bits
   wherever it stands in the table and whatever n is. */
BPRX_API int bprx_project_rows(bprx_handle *h, const void *Fnew, int64_t n, float *P, void *stream);
/* out fp32 [(u1-u0), n]: out[u][j] = Tu_u.P[j, 0:d] + P[j, d] (P from bprx_project_rows): the fp32 MFMA GEMM of
   bprx_score_block, exact fp32 products.  0 <= u0 <= u1 <= num_users. */
BPRX_API int bprx_score_new_block(bprx_handle *h, int32_t u0, int32_t u1, const float *P, int64_t n, float *out, void *stream);
/* bprx_topk on nrows rows of explicit `width` (row stride width), nothing masked: the K (1..1024) largest scores of each row
   best first, idx int32 [nrows, K] (-1 past min(K, width)), val fp32 same shape, flag int32 [nrows] with the selection, order
   and flag rules of bprx_topk.  1 <= width < 2^31. */
BPRX_API int bprx_topk_rows(bprx_handle *h, int64_t nrows, int32_t width, float *scores, int32_t K, int32_t *idx, float *val,
                            int32_t *flag, void *stream);
/* bprx_feat_explain for the pairs (user[p], row[p] of Fnew [n_new, feat_dim]): contributions F_jc w_uc, w_uc = Bp[c] + E[c,:].Tu_u
   from the fp32 master tables.  There is no base: score is the sum of the contributions (what bprx_feat_explain calls visual).
   Outputs, order and tie rules, limits (ncols, top, feat_dim) and bit-level guarantees as for bprx_feat_explain: score fp32 [n],
   col int32 / contrib fp32 [n, top], map fp32 [n, ncols] or NULL.  user >= num_users and row >= n_new are clamped and reported by
   bprx_sync_check (BPRX_E_RANGE).  With bf16 features score differs from bprx_score_new_block by the rounding of [E|Bp] there. */
BPRX_API int bprx_feat_explain_new(bprx_handle *h, const void *Fnew, int64_t n_new, const int32_t *user, const int32_t *row,
                                   int64_t n, int32_t ncols, int32_t top, float *score, int32_t *col, float *contrib, float *map,
                                   void *stream);

/* ---- BPRMF, VBPR and GradFashion: users the model was not trained on ------------------------------------------------------
   A user who arrives after training with a short history of catalogue items has no row of Gu / Tu.  With every item-side
   parameter frozen, the reference's loss for one user (VBPR.py:117-127 with Gi, Bi, E, Bp held fixed) is a convex problem in that
   user's k + d numbers.  For new user r with pairs (i_p, j_p), p in [pair_ptr[r], pair_ptr[r+1]), n_r of them:
       z_i = [Gi_i | P_i[0:d]]        c_i = Bi_i + P_i[d]          (P = F.[E|Bp], the cached projections; BPRMF: d = 0, c_i = Bi_i)
       D_p = z_i - z_j                dc_p = c_i - c_j             (one fp32 subtraction per element, formed once)
       w = [gamma | theta] starts at the caller's row; for t = 1 .. steps:
         x_p = w.D_p + dc_p           s_p = sigmoid(-clip(x_p, -80, 1e8))      (inclusive bounds, no gradient outside)
         g = sum_p (-s_p D_p) + 2 reg n_r w                                     (summed in pair order)
         loss_t = sum_p softplus(-clip(x_p)) + reg n_r |w|^2
         BPRX_OPT_SGD:        w <- w - lr g
         BPRX_OPT_ADAM_TF23:  the sparse-variable rule of the Gu / Tu rows, slots starting at zero,
                              lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t); beta1, beta2, epsilon are the handle's
   i.e. one train_step of the reference on a batch made of this user's pairs with everything but the user's row frozen: for
   steps = 1, started from a trained user's row, the row moves as bprx_step on the same batch moves it.
   bprx_fold_in: pair_ptr int64 [n+1], pos / neg int32 (device); Gu_rows fp32 [n, k] and Tu_rows fp32 [n, d] in / out (Tu_rows NULL
   iff d == 0); loss fp32 [n] or NULL: loss_steps, evaluated before the last update, as train_step returns it.  A user without
   pairs keeps its row and has loss 0.  lr, reg, optimizer are the call's (the handle's own are not read).
   Handles: a bound BPRMF or VBPR handle, plain or factored, any feature dtype (the call reads P, never F).  BPRX_E_INVALID for a
   NULL handle, an ACF or AttentiveFashion handle, a NULL pointer, n < 0, steps < 1, an unknown optimizer, k + d > 1024;
   BPRX_E_STATE for an unbound handle; n == 0: BPRX_OK.  Item ids out of range are clamped and reported by bprx_sync_check
   (BPRX_E_RANGE).  Like bprx_score_block the call first settles a pending dense update, brings lazy adam_tf23 rows up to date and
   makes P current; apart from that it writes its outputs only and allocates nothing.  No atomics: a user's result depends on its
   own pairs, its start row and the tables only -- not on n, on its position, or on BPRX_FOLD_CACHE (0: every step gathers the
   item rows again instead of keeping D_p in LDS where a user's pairs fit; read by bprx_create). */
BPRX_API int bprx_fold_in(bprx_handle *h, const int64_t *pair_ptr, const int32_t *pos, const int32_t *neg, int64_t n, int32_t steps,
                          float lr, float reg, int32_t optimizer, float *Gu_rows, float *Tu_rows, float *loss, void *stream);
/* bprx_score_block for caller-owned user rows: out fp32 [(r1-r0), num_items] for rows [r0, r1) of Gu_rows [n_rows, k] /
   Tu_rows [n_rows, d] (NULL iff d == 0).  The same kernels (the non-MFMA one for an odd k or d), P made current first: a slice of
   the handle's own Gu / Tu gives the bits of bprx_score_block.  0 <= r0 <= r1 <= n_rows < 2^31; errors as for bprx_fold_in. */
BPRX_API int bprx_score_rows_block(bprx_handle *h, const float *Gu_rows, const float *Tu_rows, int64_t n_rows, int64_t r0, int64_t r1,
                                   float *out, void *stream);
/* bprx_topk for nrows (not bounded by num_users) rows of catalogue width: row r masks the items list_items[list_ptr[r] ..
   list_ptr[r+1]) IN `scores` (list_ptr int64 [nrows+1], device).  Selection, order and flag rules, K and outputs as bprx_topk. */
BPRX_API int bprx_topk_lists(bprx_handle *h, int64_t nrows, float *scores, const int64_t *list_ptr, const int32_t *list_items,
                             int32_t K, int32_t *idx, float *val, int32_t *flag, void *stream);

/* ---- BPRMF, VBPR and GradFashion: similar items, the cosine of two items in the model's item space --------------------------
   "Which items are like this one": the item vector z_i by space,
       BPRX_SIM_LATENT  z_i = Gi_i                      (k numbers)      a BPRMF or VBPR handle, plain or factored, any feat_dtype
       BPRX_SIM_VISUAL  z_i = P[i, 0:d] = f_i E         (not the Bp column; a factored handle: E_eff)
       BPRX_SIM_BOTH    z_i = [Gi_i | P[i, 0:d]]        (the item side of x_ui)
                                                        VISUAL / BOTH: a VBPR handle, plain or factored, fp32 or bf16 features
       rn_i = 1 / sqrt(sum_x z_ix^2)   the fp32 sum taken in ascending x, each square and each sum rounded once; rn_i = 0 for sum 0
       s(q, j) = <z_q, z_j> (rn_q rn_j)                 the two norms are multiplied first: the factor is symmetric
   <z_q, z_j> is the fp32 MFMA GEMM of bprx_score_block (exact fp32 products, sums in x order, Gi before P): s(q, j) has the bits
   of s(j, q), two items with bit-equal z have bit-equal rows, a zero row has similarity 0.0 to everything (never NaN), and a
   row's bits depend on its own z, the catalogue and the norms only -- not on q0, q1, nq or the tile it lands in.  The entry of
   an item with itself is NOT masked: rank a block with bprx_topk_lists and lists in which row r names item q0 + r, rows from
   outside the catalogue with bprx_topk_rows.
   Errors: BPRX_E_INVALID for a NULL handle or pointer, an unknown space, an ACF or AttentiveFashion handle, a BPRMF handle in
   VISUAL / BOTH, an fp8 handle in VISUAL / BOTH, a bad range, Pq != NULL with another space than VISUAL, Pq == NULL with
   nq != num_items; BPRX_E_STATE for unbound tables; q0 == q1: BPRX_OK, nothing is written.  After any error the handle stays
   usable.  State: like bprx_score_block both calls first settle a pending dense update, bring lazy adam_tf23 rows up to date and
   (VISUAL / BOTH) make P current; apart from that they write their outputs only and allocate nothing. */
#define BPRX_SIM_LATENT 0
#define BPRX_SIM_VISUAL 1
#define BPRX_SIM_BOTH 2
/* Pq == NULL: rn fp32 [num_items] of the catalogue, nq must equal num_items.  Pq != NULL: rn fp32 [nq] of the nq rows of
   bprx_project_rows' output Pq [nq, PS] (items outside the catalogue, on the catalogue's scale); space must be BPRX_SIM_VISUAL. */
BPRX_API int bprx_sim_rnorm(bprx_handle *h, int32_t space, const float *Pq, int64_t nq, float *rn, void *stream);
/* out fp32 [(q1-q0), num_items]: out[r][j] = s(q0 + r, j).  Pq == NULL: the queries are the catalogue items q0 .. q1-1
   (nq == num_items; rn_q is indexed by item id and may equal rn_items).  Pq != NULL: the queries are rows q0 .. q1-1 of Pq, rn_q
   fp32 [nq] their norms, visual space only.  rn_items: bprx_sim_rnorm of the catalogue in the same space.
   0 <= q0 <= q1 <= nq < 2^31, q1 - q0 <= 65535 * 128. */
BPRX_API int bprx_sim_block(bprx_handle *h, int32_t space, const float *Pq, int64_t nq, int64_t q0, int64_t q1, const float *rn_q,
                            const float *rn_items, float *out, void *stream);

/* ---- BPRMF, VBPR and GradFashion: audiences, the score block item-major ---------------------------------------------------
   "Who should see this item": the scores of a range of items against EVERY user, one output row per item, so that a top-K over
   a row is the item's audience.  The user-major blocks of bprx_score_block / bprx_score_new_block cannot be transposed
   afterwards (the U x I matrix is never resident); this is their kernel with the operand roles swapped.
   out fp32 [(q1-q0), num_users] (row stride num_users), q = q0 + r:
       Pq == NULL  the catalogue, nq must equal num_items:
                   out[r][u] = Bi_q + Gu_u.Gi_q (+ Tu_u.P_q[0:d] + P_q[d])     bprx_score_block's score
       Pq != NULL  rows of bprx_project_rows' output Pq [nq, PS], items outside the catalogue:
                   out[r][u] = Tu_u.Pq_q[0:d] + Pq_q[d]                        bprx_score_new_block's score
   The fp32 MFMA GEMM of bprx_score_block with A = the item rows, B = the user rows: exact fp32 products, sums in x order from
   +0, Gi before P, then acc + (Bi_q + P_q[d]).  Contract: for EVEN embed_k and embed_d, out[r][u] has the bits of
   bprx_score_block's out[u][q] (Pq: of bprx_score_new_block's out[u][q]).  For an odd embed_k or embed_d bprx_score_block
   runs its non-MFMA kernel, whose summation order differs; this entry stays on the MFMA path (K padded with zeros) and is
   then close to it, not bit-equal (bprx_score_new_block is always on the MFMA path: bit-equal for any d).  A row's bits
   depend on its item row and the user tables only: not on q0, q1, nq or the tile it lands in.
   Handles: a bound BPRMF or VBPR handle, plain or factored; the catalogue form takes every feature dtype bprx_score_block takes,
   the Pq form a VBPR handle with fp32 or bf16 features (the rule of bprx_score_new_block).
   0 <= q0 <= q1 <= nq < 2^31, q1 - q0 <= 65535 * 128.  BPRX_E_INVALID for a NULL handle or pointer (Pq excepted), an ACF or
   AttentiveFashion handle, Pq with a BPRMF or an fp8 handle, Pq == NULL with nq != num_items, a bad range; BPRX_E_STATE for
   unbound tables; q0 == q1: BPRX_OK, nothing is written.  After any error the handle stays usable.
   State: the catalogue form enters like bprx_score_block (settles a pending dense update, brings lazy adam_tf23 rows up to
   date, makes P current), the Pq form like bprx_score_new_block (rows, the [E|Bp]^T image); apart from that the call writes its
   output only and allocates nothing: a training run with these calls between its steps ends bit-identical to one without. */
BPRX_API int bprx_audience_block(bprx_handle *h, const float *Pq, int64_t nq, int64_t q0, int64_t q1, float *out, void *stream);
/* bprx_topk_rows with bprx_topk_lists' per-row mask lists: nrows rows of explicit `width` (row stride width; an audience block:
   width = num_users), row r gets -inf IN `scores` at list_items[list_ptr[r] .. list_ptr[r+1]) (list_ptr int64 [nrows+1], device;
   an id outside [0, width) is ignored, a repeated id is harmless).  Selection, order and flag rules, K (1..1024) and outputs as
   bprx_topk; a row with fewer than min(K, width) unmasked entries is flagged.  1 <= width < 2^31, 0 <= nrows < 2^31.  Any handle,
   bound or not (as bprx_topk_lists). */
BPRX_API int bprx_topk_rows_masked(bprx_handle *h, int64_t nrows, int32_t width, float *scores, const int64_t *list_ptr,
                                   const int32_t *list_items, int32_t K, int32_t *idx, float *val, int32_t *flag, void *stream);

/* ---- category shelves: the K best entries of every CLASS of a score row (a segmented top-K) --------------------------------
   "Dresses for you, shoes for you": every list surface above is blind to item category; this one call over a block of score rows
   returns, per row, one list per class, and the quota list (the top-k with at most M items of any class) is the k best of the union
   of every class's first min(M, k) entries.  Model-agnostic: it ranks a score block and touches no table or slot.
   scores fp32 [nrows, width] (row stride width, device).  Mask: row r gets -inf IN `scores` at list_items[list_ptr[row0 + r] ..
   list_ptr[row0 + r + 1]) (list_ptr int64, device; an id outside [0, width) is ignored, a repeated id is harmless; list_ptr ==
   NULL masks nothing and list_items is not read); afterwards the row holds -inf at the masked ids and is otherwise bit-unchanged.
   Classes: class_ptr int64 [C + 1], class_items int32 [class_ptr[C]] (device): the items of class c in ascending order, every item
   in at most one class; an item in no class is on no list, an empty class is allowed.  A class_items entry outside [0, width) is
   skipped and reported by bprx_sync_check (BPRX_E_RANGE); it is never dereferenced.
   Outputs idx int32 [nrows, C, K], val fp32 [nrows, C, K], cnt int32 [nrows, C]:
       cnt[r][c] = min(K, number of items of class c whose score in the masked row is > -inf)    (a masked item is on no shelf)
       slots past cnt hold -1 / 0.0f.
   Order: a total order of this surface's own, so there is NO flag and no host redo: score descending compared as floats (+0.0 ==
   -0.0), equal scores by ascending item id -- at the selection boundary too: when more items equal the K-th score than there are
   slots left, the smallest ids are taken.  val is read from the row: val[r][c][q] has the bits of scores[r][idx[r][c][q]] (the sign
   of a zero is kept).  NaN scores are outside the contract.  List (r, c) depends on row r's scores at the items of class c and on
   row r's mask only: not on nrows, on the row's position, on the other classes or on their numbering.
   1 <= K <= 1024, C >= 1, width >= 1, nrows >= 0, row0 >= 0, nrows * C * K < 2^31, else BPRX_E_INVALID; a NULL pointer with rows
   to list: BPRX_E_INVALID; nrows == 0: BPRX_OK, nothing is launched.  Every accepted shape launches (the workgroup counts, up
   to 2^31, are folded into two grid dimensions).  Any handle, bound or not (as bprx_topk_lists); the call
   allocates nothing and after an error the handle stays usable. */
BPRX_API int bprx_topk_classes(bprx_handle *h, int64_t nrows, int32_t width, float *scores, int64_t row0, const int64_t *list_ptr,
                               const int32_t *list_items, const int64_t *class_ptr, const int32_t *class_items, int32_t C,
                               int32_t K, int32_t *idx, float *val, int32_t *cnt, void *stream);

/* ---- BPRMF, VBPR and GradFashion: style clusters, spherical k-means of the item space -----------------------------------------
   "Which styles has the model found, which style is this dress": Lloyd's loop over the unit vectors z_i rn_i of bprx_sim_* (space,
   z_i, rn_i and the handle rules are those of bprx_sim_block) is these two calls in turn; the caller keeps the S centroids, fp32
   [S, w] row-major on the device, w = k (LATENT), d (VISUAL) or k + d (BOTH, the Gi part before the P part), 1 <= S <= 1024.
   bprx_style_assign, for the query rows q in [q0, q1) and centroid rows that are unit vectors or zero rows:
       c(q, s)         = <z_q, cent_s> rn_q     the fp32 MFMA GEMM of bprx_sim_block (exact fp32 products, sums in x order from
                                                +0, Gi before P) against the centroids; the norm is multiplied last
       style[q - q0]   = the s with the largest c(q, s), int32; cos[q - q0] = that maximum
       second[q - q0]  = the largest c(q, s) over s != style, -inf for S == 1 (second may be NULL: style and cos keep their bits)
   Ties go to the smallest s: (value, index) pairs are compared, inside a wave's reduction and across centroid tiles alike.  A
   query with rn_q == 0 gets style -1, cos 0.0, second 0.0; a zero centroid scores 0.0 against everything; NaN is outside the
   contract.  One workgroup owns 128 query rows and walks the centroids in tiles of 128 with the running result in registers:
   nothing of size rows x S is written.  A row's three outputs depend on that row, its norm and the centroid table only: not on
   q0, q1, nq, the tile the row lands in, or where a centroid sits inside its tile.  Pq == NULL: the catalogue, nq == num_items,
   rn_q indexed by item id; Pq != NULL: rows of bprx_project_rows' output, rn_q their norms, VISUAL only (as bprx_sim_block).
   bprx_style_update, for the clusters given as a CSR (member_ptr int64 [S + 1], member_items int32, ascending within a cluster,
   device: the layout of a class table), with rn_items = bprx_sim_rnorm of the catalogue:
       sum_s      = sum over i in members(s) of fl32(z_ix rn_i)     accumulated in fp64
       cent_out_s = sum_s / |sum_s|, mass[s] = |sum_s|              formed in fp64, each rounded once to fp32; 0 <= mass[s] <= size
   The fp64 order is fixed by the cluster's own member list: the list is cut at multiples of 16, a piece is added up in list order
   from +0, and the pieces are added to the sum in ascending order; |sum|^2 adds the squares of the columns l, l + 64, .. in
   ascending order for l < 64 and folds the 64 sums in an xor tree.  No float atomics.  An empty cluster, or one whose |sum|^2 is
   exactly 0 in fp64 (a row and its negation), copies cent_prev_s and reports mass 0 (cent_out may be cent_prev).  A member id
   outside [0, num_items) is skipped and reported by bprx_sync_check (BPRX_E_RANGE); it is never dereferenced.  The bits of
   cluster s depend on its member list and those members' rows and norms only: not on S, the other clusters, its number or the
   launch; two calls give equal bits.  The objective of a run is sum_s mass[s] / (number of assigned items).
   Errors: BPRX_E_INVALID for a NULL handle or pointer (second excepted), S outside [1, 1024], an unknown space, an ACF or
   AttentiveFashion handle, a BPRMF handle in VISUAL / BOTH, an fp8 handle in VISUAL / BOTH, a bad range, Pq != NULL with another
   space than VISUAL, Pq == NULL with nq != num_items, bprx_style_update in a space wider than 4096 numbers; BPRX_E_STATE for
   unbound tables; q0 == q1: BPRX_OK, nothing is written.  After any error the handle stays usable.  State: like bprx_sim_block
   both calls first settle a pending dense update, bring lazy adam_tf23 rows up to date and (VISUAL / BOTH) make P current; apart
   from that they write their outputs only and allocate nothing: a training run with these calls between its steps ends
   bit-identical to one without. */
#define BPRX_STYLES_MAX 1024
BPRX_API int bprx_style_assign(bprx_handle *h, int32_t space, const float *Pq, int64_t nq, int64_t q0, int64_t q1, const float *rn_q,
                               const float *cent, int32_t S, int32_t *style, float *cos, float *second /* may be NULL */,
                               void *stream);
BPRX_API int bprx_style_update(bprx_handle *h, int32_t space, const float *rn_items, const int64_t *member_ptr,
                               const int32_t *member_items, int32_t S, const float *cent_prev, float *cent_out, float *mass,
                               void *stream);

/* ---- BPRMF, VBPR and GradFashion: warm items, new items with first buyers --------------------------------------------------
   The twin of bprx_fold_in on the item side.  An item outside the catalogue is scored by its picture alone
   (bprx_score_new_block); once it has buyers, its Gi_r and Bi_r can be fitted with every user-side and catalogue parameter
   frozen.  New item r owns w = [Gi_r (k) | Bi_r (1)] and, for VBPR, its projection row Pn_r (bprx_project_rows).  Its pairs
   p in [pair_ptr[r], pair_ptr[r+1]) are triples (u_p, o_p, role_p): a catalogue user, a catalogue item and the role the new item
   plays against it: role 0, the new item is the positive (the reference's triplet (u, r, o)), s_p = +1; role 1, the negative
   (the triplet (u, o, r)), s_p = -1.  With n_r pairs, n_pos of them in role 0 and n_neg in role 1:
       a_p = [Gu_u | 1]
       v_p = Tu_u.(Pn_r[0:d] - P_o[0:d]) + (Pn_r[d] - P_o[d]) - Bi_o - Gu_u.Gi_o          (d = 0: -Bi_o - Gu_u.Gi_o)
       D_p = s_p a_p                 dc_p = s_p v_p                 (formed once: nothing in them moves)
       rv  = [n_r, ..., n_r | n_pos + c_neg n_neg]                  c_neg: 0.1 (VBPR.py:125, BPRMF.py:111: the bias of a negative
                                                                    is regularised by reg / 10); a factored handle: its neg_bias_reg
       w starts at the caller's row; for t = 1 .. steps:
         x_p = w.D_p + dc_p          s = sigmoid(-clip(x_p, -80, 1e8))                    (inclusive bounds, no gradient outside)
         g = sum_p (-s D_p) + 2 reg rv o w                                                (summed in pair order)
         loss_t = sum_p softplus(-clip(x_p)) + reg sum(rv o w o w)
         BPRX_OPT_SGD: w <- w - lr g;  BPRX_OPT_ADAM_TF23: the sparse-variable rule, slots from zero, lr_t as for bprx_fold_in
   i.e. one train_step of the reference on a batch in which the new item occurs once per triplet, in either role: for steps = 1,
   started from a catalogue item's own Gi / Bi / P row, the row moves as bprx_step on that batch moves it.  Both roles matter: with
   the new item only ever the positive nothing but the regulariser holds Bi_r down.
   Plain sgd sums the batch loss: the curvature along the bias is up to 0.25 n_r, and the iteration oscillates once
   lr 0.25 n_r (1 + |Gu|^2) passes 2 (lr = 0.02 with 200 pairs already does).  Adam, the reference's optimiser, does not care.  The
   call is for first buyers, not for refitting bestsellers.
   bprx_fold_in_items: pair_ptr int64 [n+1], user / other / role int32 (device); Pn fp32 [n, PS] from bprx_project_rows (NULL iff
   d == 0); Gi_rows fp32 [n, k] and Bi_rows fp32 [n] in / out; loss fp32 [n] or NULL: loss_steps, before the last update.  An item
   without pairs keeps its rows and has loss 0.  lr, reg, optimizer are the call's.
   Handles: a bound BPRMF or VBPR handle, plain or factored, fp32 or bf16 features.  BPRX_E_INVALID for a NULL handle, an ACF or
   AttentiveFashion handle, an fp8 handle, a NULL pointer, n < 0, steps < 1, an unknown optimizer, k + 1 > 1024, k + d > 1024;
   BPRX_E_STATE for an unbound handle; n == 0: BPRX_OK.  User and item ids out of range and a role other than 0 or 1 are clamped
   and reported by bprx_sync_check (BPRX_E_RANGE).  The call enters like bprx_fold_in (settles a pending dense update, brings lazy
   adam_tf23 rows up to date, makes P current); apart from that it writes its outputs only and allocates nothing.  No atomics: an
   item's result depends on its own pairs, its start row and the tables only -- not on n, on its position, or on BPRX_FOLD_CACHE
   (0: every step forms D_p and dc_p again instead of keeping them in LDS where an item's pairs fit). */
BPRX_API int bprx_fold_in_items(bprx_handle *h, const int64_t *pair_ptr, const int32_t *user, const int32_t *other, const int32_t *role,
                                int64_t n, const float *Pn, int32_t steps, float lr, float reg, int32_t optimizer, float *Gi_rows,
                                float *Bi_rows, float *loss, void *stream);
/* The full score of n caller-owned item rows: out fp32 [(u1-u0), n], out[u][j] = Bi_j + Gu_u.Gi_j + Tu_u.Pn_j[0:d] + Pn_j[d]
   (Gi_rows [n, k], Bi_rows [n], Pn [n, PS] or NULL iff d == 0).  bprx_score_block's kernels given the caller's rows (the non-MFMA
   one for an odd k or d): a slice of the catalogue's own Gi / Bi / P gives the bits of those columns of bprx_score_block, zero
   Gi / Bi rows give the bits of bprx_score_new_block for even k, d.  0 <= u0 <= u1 <= num_users, 0 <= n < 2^31.  Handles and errors as
   for bprx_fold_in_items; the call brings lazy adam_tf23 rows and the [E|Bp]^T image up to date and writes its output only. */
BPRX_API int bprx_score_warm_block(bprx_handle *h, int32_t u0, int32_t u1, const float *Gi_rows, const float *Bi_rows, const float *Pn,
                                   int64_t n, float *out, void *stream);
/* The same item-major: out fp32 [(q1-q0), num_users], out[r][u] = the score above of row q0 + r: bprx_audience_block's kernel
   given the caller's rows (always the MFMA path; bit for bit bprx_score_warm_block's out[u][q] for even k and d).
   0 <= q0 <= q1 <= n < 2^31, q1 - q0 <= 65535 * 128. */
BPRX_API int bprx_audience_warm_block(bprx_handle *h, const float *Gi_rows, const float *Bi_rows, const float *Pn, int64_t n, int64_t q0,
                                      int64_t q1, float *out, void *stream);

/* ---- BPRMF, VBPR and GradFashion: diversified lists, greedy Maximal Marginal Relevance over a top-N pool -------------------
   "K of the N best that are good and unlike the picks above them".  One list has the pool (id_c, v_c), c = 0 .. N-1, best first,
   as bprx_topk / bprx_topk_lists / bprx_topk_rows return it with K = N.  A slot with id_c < 0 or v_c == -inf is no candidate;
   M = the number of candidates.  z_i and rn_i are those of bprx_sim_rnorm / bprx_sim_block for `space` (same handle rules).
       rel_c     = (v_c - v_min) / (v_max - v_min) over the candidates, 0 when v_max == v_min: relevance on [0, 1] per list
                   (scores have no fixed scale, cosines do); the two differences and the quotient are each rounded once
       cos(c, s) = <z_c, z_s> (rn_c rn_s)   fp32: <z_c, z_s> is the serial chain a = fma(z_cx, z_sx, a) from +0 in ascending x, Gi
                   before P (one rounding per term); the two norms are multiplied first, then the sum by their product.  A
                   function of the two rows and their norms alone, with the bits of cos(s, c).  (bprx_sim_block's MFMA sum
                   rounds products and sums separately: close, not bit-equal.)
       pen_c     = max over the items s selected so far of cos(c, s); 0 before the first pick (a candidate's first cosine
                   replaces that 0, also a negative one)
       obj_c     = (1 - theta) rel_c - theta pen_c    1 - theta, both products and the difference are each rounded once (four
                   roundings, nothing fused)
   At each of min(K, M) steps the unselected candidate with the largest obj_c is selected; values compare as floats (-0 == +0),
   equal values go to the lower pool position.  theta = 0 returns the pool's first min(K, M) candidates unchanged.
   Outputs per list r: idx int32 [K] the picks' pool ids in selection order, val fp32 [K] their pool scores (bits unchanged), pen
   fp32 [K] each pick's pen at the moment it was picked (its redundancy; 0 for the first), slots past min(K, M) hold -1 / 0.0f /
   0.0f.  ild fp32 [n] (may be NULL): the intra-list diversity 1 - (sum of cos over the pairs of the list) / (T (T - 1) / 2), T =
   min(K, M), 0 for T < 2.  The sum runs in selection order: a_t = ((cos(s_t, s_0) + cos(s_t, s_1)) + ..) + cos(s_t, s_t-1) from
   +0 (the pick's running sum), total = ((a_0 + a_1) + ..) + a_T-1 from +0; one rounded quotient, one rounded difference.
   A list's outputs depend on its own pool, the rows of its candidates and their norms only: not on n, its position in the call,
   the other lists, the call, or on whether the kernel kept the rows in LDS or re-read them from memory.
   rn_items: bprx_sim_rnorm of the catalogue in the same space.  pool_idx int32 [n, N], pool_val fp32 [n, N].
   1 <= K <= N <= 1024, 0 <= n < 2^31 (n == 0: BPRX_OK, nothing is written), 0 <= theta <= 1.
   Errors: BPRX_E_INVALID for a NULL handle or pointer (ild excepted; with n == 0 only rn_items is looked at), an unknown space, an ACF or AttentiveFashion handle, a
   BPRMF handle in VISUAL / BOTH, an fp8 handle in VISUAL / BOTH, K / N / n out of range, theta outside [0, 1] or NaN;
   BPRX_E_STATE for unbound tables.  A candidate id >= num_items is clamped (its row is item num_items - 1, the returned id is
   the pool's) and reported by bprx_sync_check (BPRX_E_RANGE).  After any error the handle stays usable.
   State: like bprx_sim_block the call first settles a pending dense update, brings lazy adam_tf23 rows up to date and (VISUAL /
   BOTH) makes P current; apart from that it writes its outputs only and allocates nothing. */
BPRX_API int bprx_diversify(bprx_handle *h, int32_t space, const float *rn_items, int64_t n, int32_t N, const int32_t *pool_idx,
                            const float *pool_val, int32_t K, float theta, int32_t *idx, float *val, float *pen, float *ild,
                            void *stream);

/* ---- calibrated lists: greedy KL re-rank of a top-N pool toward the class mix of the user's own history --------------------------
   Calibration (Steck, "Calibrated Recommendations", RecSys 2018) with one-hot classes: each of n lists is picked greedily from its
   pool so that (1 - lambda) relevance - lambda KL(p || q~) grows the most, p the class shares of the user's history, q the class
   shares of the list so far and q~ = (1 - alpha) q + alpha p.
   The pool of list r: pool_idx int32 [n, N] / pool_val fp32 [n, N] in pool order (bprx_topk's output with K = N); an entry with
   pool_idx < 0 or pool_val == -inf is no candidate, M = the number of candidates.  The class table: item_class int32 [width]
   (device), -1 = no class, otherwise in [0, C).  The history of list r: hist_items[hist_ptr[row0 + r] .. hist_ptr[row0 + r + 1])
   (hist_ptr int64, device; hist_ptr == NULL: every history is empty and hist_items is not read).
       cnt_c     = the number of history entries of class c (an id outside [0, width) or a classless item is not counted; a repeated
                   id counts every time); H = sum of cnt_c, p_c = cnt_c / H
       rel_c     = (v_c - v_min) / (v_max - v_min) over the candidates, 0 for a flat pool: bprx_diversify's
       den_g(m)  = (1 - alpha) m / L + alpha p_g                                  with t picks made, n_g of them of class g, L = t + 1
       delta_g   = p_g log(den_g(n_g) / den_g(n_g + 1))                           <= 0; 0 when p_g = 0 or the candidate has no class
       obj_c     = (1 - lambda) rel_c - lambda delta_class(c)
   (the terms of the KL that do not depend on the candidate cancel out of the arg-max: one number per class and step.)  Every
   operation is rounded once in fp32, nothing is fused, log is logf.  At each of T = min(K, M) steps the unselected candidate with
   the largest obj_c is selected; values compare as floats (-0 == +0), equal values go to the lower pool position.  lambda = 0
   returns the pool's first T candidates unchanged; with H = 0 every delta is 0 and the same holds.
   Outputs per list r: idx int32 [K] the picks' pool ids in selection order, val fp32 [K] their pool scores (bits unchanged), cls
   int32 [K] their classes (-1: none), gain fp32 [K] -delta of the pick at its step (>= 0); slots past T hold -1 / 0.0f / -1 /
   0.0f.  kl fp32 [n, 2] (may be NULL): kl[r][0] = KL(p || q~) of the pool's first T candidates (the plain list), kl[r][1] of the
   calibrated list, KL = sum over the classes with p_c > 0 of p_c log(p_c / den_c(n_c)) at L = T, summed in an order that depends
   on C only (no float atomics); both are 0.0 when H = 0 or T = 0.  Without kl the other outputs have the same bits.
   A list's outputs depend on its own pool, its history and the class table only: not on n, its position in the call or row0.
   1 <= K <= N <= 1024, 1 <= C <= 1024, 0 <= lambda <= 1, 0 < alpha < 1, width >= 1, 0 <= n < 2^31, row0 >= 0; a value out of range
   or NaN, or a NULL pointer with n > 0 (kl and hist_ptr excepted; hist_items with hist_ptr): BPRX_E_INVALID, the message starts
   with "calibrate".  n == 0: BPRX_OK, nothing is launched.  A candidate's id >= width, or an item_class value outside [-1, C) at a
   candidate or a history entry, is treated as classless, never used as an index, and reported by bprx_sync_check (BPRX_E_RANGE);
   the returned id is the pool's own.
   The call reads no model table: any handle, bound or not, of any model.  It is not behind the gate: it settles nothing, changes
   no state and allocates nothing; after an error the handle stays usable. */
BPRX_API int bprx_calibrate(bprx_handle *h, int64_t n, int32_t N, const int32_t *pool_idx, const float *pool_val, int64_t row0,
                            const int64_t *hist_ptr, const int32_t *hist_items, const int32_t *item_class, int32_t width, int32_t C,
                            int32_t K, float lambda, float alpha, int32_t *idx, float *val, int32_t *cls, float *gain,
                            float *kl /* may be NULL */, void *stream);

/* ---- BPRMF, VBPR and GradFashion: "because you own X", the nearest owned items of every entry of a list ---------------------
   For each entry of each of n lists of K slots, the L items of that list's history that are nearest to it by cosine in the
   model's item space.  space, z_i, rn_i and the handle rules are those of bprx_sim_block.
   The explained items: Pq == NULL: list_idx[r, q] is a catalogue item (nq == num_items; rn_q is indexed by item id, may equal
   rn_items, NULL: rn_items).  Pq != NULL (visual space only): list_idx[r, q] is a row of Pq [nq, PS] = bprx_project_rows'
   output, rn_q fp32 [nq] = bprx_sim_rnorm of those rows.  A slot < 0 is empty.
   The history of list r is hist_items[hist_ptr[r] .. hist_ptr[r+1]) (hist_ptr int64 [n + 1], catalogue ids); an entry is
   identified by its position in it (fewer than 2^31 entries per list; an id may repeat, each position is an entry of its own).
   With Pq == NULL an entry whose id equals the explained item is no candidate (as --similar_items excludes the item itself).
   M = the number of candidates.
       cos(q, l) = <z_q, z_l> (rn_q rn_l)   exactly bprx_diversify's: <z_q, z_l> is the serial chain a = fma(z_qx, z_lx, a) from +0
                   in ascending x, Gi before P; the two norms are multiplied first, then the sum by their product.  It has the
                   bits of cos(l, q) and of the pen bprx_diversify reports for the same two rows.
   out_item int32 / out_cos fp32 [n, K, L]: slots s < min(L, M) of (r, q) hold the candidates' ids (as the history gives them)
   and cosines by descending cosine; values compare as floats (-0 == +0), equal values go to the lower history position.  Slots
   past min(L, M), and every slot of an empty list slot, hold -1 / 0.0f.  out_cnt int32 [n, K] (may be NULL): M, 0 for an empty
   slot.  The outputs of (r, q) depend on that item's row, the history's rows and the norms only: not on K, n, the other slots,
   or on how the kernel chunks a list or tiles a history.
   1 <= L <= 32, 1 <= K <= 1024, 0 <= n < 2^31 (n == 0: BPRX_OK, nothing is written), any history length.
   Errors: BPRX_E_INVALID for a NULL handle or pointer (out_cnt excepted; rn_q may be NULL with Pq == NULL; with n == 0 only the
   norms are looked at), K / L / n out of range, every space / handle / Pq / nq combination bprx_sim_block rejects, and an item
   space too wide for two rows in a workgroup's LDS (more than about 8000 numbers); BPRX_E_STATE for unbound tables.  An id >=
   num_items (a list entry >= nq) is clamped (the returned id is the history's) and reported by bprx_sync_check (BPRX_E_RANGE).
   After any error the handle stays usable.
   State: like bprx_sim_block the call first settles a pending dense update, brings lazy adam_tf23 rows up to date and (VISUAL /
   BOTH) makes P current; apart from that it writes its outputs only and allocates nothing. */
BPRX_API int bprx_because(bprx_handle *h, int32_t space, const float *Pq, int64_t nq, const float *rn_q, const float *rn_items,
                          int64_t n, int32_t K, const int32_t *list_idx, const int64_t *hist_ptr, const int32_t *hist_items,
                          int32_t L, int32_t *out_item, float *out_cos, int32_t *out_cnt, void *stream);

/* ---- BPRMF, VBPR and GradFashion: influence, the owned items a pick's score rests on -----------------------------------------
   "How far would this pick's score fall had the user not bought X": the training-point influence (Koh & Liang 2017; for latent
   factor models Cheng et al., KDD 2019) of every history entry on the scores of a list, taken on the user's own objective, the
   per-user convex problem of bprx_fold_in with every item-side parameter frozen.  For row r: w = [Gu_rows_r | Tu_rows_r] (k + d
   numbers), its m_r pairs (pos[p], neg[p]), p in [pair_ptr[r], pair_ptr[r+1]); `per_entry` consecutive pairs form one history
   entry, a short last group is an entry of its own: M_r = ceil(m_r / per_entry) entries, entry e owns the row's pairs
   [e per_entry, (e+1) per_entry) and is named by pos of its first pair.  z_i, c_i, D_p, dc_p, x_p and the clip as above:
       s_p = sigmoid(-x_p)   c_p = s_p (1 - s_p)           (x_p outside [-80, 1e8]: s_p = c_p = 0)
       A = sum_p c_p D_p D_p^T                              (n x n, n = k + d)
       lambda = 2 reg m_r + damp trace(A) / n               (the objective's own ridge + a Levenberg-Marquardt term relative to A)
       g_e = sum_{p in entry e} s_p D_p
       infl(q, e) = z_q^T (A + lambda I)^-1 g_e             total(q) = sum_e |infl(q, e)|
   infl(q, e) is the first-order fall of x_rq when entry e's pairs leave the row's objective and the row is refitted by one damped
   Newton step: positive = the purchase holds the pick up.  With damp > 0 the condition number of A + lambda I is at most
   n / damp + 1, which keeps the fp32 Cholesky factorisation safe (and defined for reg == 0, where A alone may be singular).
   list_idx int32 [n, K]: catalogue ids, a slot < 0 is empty.  Outputs:
     out_item int32 / out_infl fp32 [n, K, L]  the min(L, M_r) entries of largest influence by descending value (values compare
                as floats, equal values go to the lower entry position; every entry is a candidate, one whose id equals q too);
                the id is the entry's own; -1 / 0.0f past them and in every slot of an empty list slot
     out_total fp32 [n, K]; out_cnt int32 [n, K] (may be NULL): M_r, 0 for an empty slot
     out_full (may be NULL): out_full[(r K + q) full_stride + e] = infl(q, e) for e < M_r (the caller makes full_stride >= M_r;
                an entry past it is not written), nothing else is written
     out_flag int32 [n] (may be NULL): 1 where the factorisation met a pivot that is not positive and finite; all of that row's
                slots are then empty (cnt 0, total 0, out_full untouched, never a NaN); 0 otherwise.  A row without pairs has
                empty slots and flag 0.
   No atomics: the outputs of (r, q) depend on the row, its pairs, the tables and q only -- not on n, K, the row's position, the
   other slots, or on how the kernel tiles pairs or chunks a list.
   Handles and state as bprx_fold_in: a bound BPRMF or VBPR handle, plain or factored, any feature dtype (the call reads P, never
   F); it first settles a pending dense update, brings lazy adam_tf23 rows up to date and makes P current, then writes its outputs
   only and allocates nothing.
   Errors: BPRX_E_INVALID for a NULL handle or required pointer (Tu_rows NULL iff d == 0), an ACF or AttentiveFashion handle,
   n < 0 or >= 2^31, K outside [1, 1024], L outside [1, 32], per_entry < 1, reg or damp negative or not finite or both zero,
   out_full with full_stride < 1, k + d > BPRX_INFLUENCE_MAX_WIDTH (one workgroup keeps A's triangle in half a CU's LDS);
   BPRX_E_STATE for an unbound handle; n == 0: BPRX_OK, nothing is written.  Item ids out of range are clamped and reported by
   bprx_sync_check (BPRX_E_RANGE).  After any error the handle stays usable. */
#define BPRX_INFLUENCE_MAX_WIDTH 160
BPRX_API int bprx_influence(bprx_handle *h, const float *Gu_rows, const float *Tu_rows, int64_t n, const int64_t *pair_ptr,
                            const int32_t *pos, const int32_t *neg, int32_t per_entry, float reg, float damp, int32_t K,
                            const int32_t *list_idx, int32_t L, int32_t *out_item, float *out_infl, float *out_total,
                            int32_t *out_cnt, float *out_full, int64_t full_stride, int32_t *out_flag, void *stream);

/* ---- ACF (ACF.py:20-270) on a BPRMF handle ------------------------------------------------------------------------------
   Attentive Collaborative Filtering over per-item feature maps f_l [M, C] (M = H*W spatial components).  For user u with
   history P(u) (ACF.py:135-181):
       s_lm = W1c.relu(Wcu^T g_u + Wci^T f_lm + bc0) + bc1        beta_l = softmax_m(s_l)        x_l = sum_m beta_lm f_lm
       t_l  = W1i.relu(Wiu^T g_u + Wiv^T Gi_l + Wip^T Pi_l + Wix^T x_l + bi0) + bi1               alpha = softmax_l(t)
       g'_u = g_u + sum_l alpha_l Pi_l        (g'_u = g_u for an empty history)        x_ui = g'_u . Gi_i   (no bias)
   The library never forms x_l: Z_l = f_l [Wci | Wix] ([M, h+a], one MFMA GEMM per distinct item) gives both the component
   term and sum_m beta_lm Z_lm[h:] = Wix^T x_l.  bprx_bind_acf binds a BPRMF handle (t: Gu, Gi, Bi and their slots; Bi stays
   zero and is neither read nor trained); afterwards
     bprx_step         the reference's step with its DETACHED gradient (g'_u is rebuilt as a new leaf, ACF.py:208): Gi gets
                       -+sigmoid(-d) g'_u + 2 reg Gi, Gu only 2 reg g_u, Pi only 2 reg Pi on the pos / neg rows, every attention
                       tensor only 2 reg w; loss = sum softplus(-clip(d)) + reg (|g_u|^2 + |Gi_i|^2 + |Gi_j|^2 + |Pi_i|^2 +
                       |Pi_j|^2 per triplet + sum |w|^2).  sgd, or adam_tf23 (sparse rule on Gu / Gi / Pi, dense rule on the
                       weights) by whole-table sweeps: an ACF handle never runs the lazy form.
     bprx_score_pairs  scores with the training histories (train_ptr / train_items)
     bprx_score_block  scores with the evaluation histories (eval_ptr / eval_items: training + validation, ACF.py:220), so
                       eval_* and topk work unchanged.
   bprx_step_begin / _end and the multi-GPU entry points are rejected (BPRX_E_STATE).  History and batch indices out of range
   are clamped and reported by bprx_sync_check (BPRX_E_RANGE).
   Limits: M <= 2048, C % 4 == 0 (fp32) or C % 8 == 0 (bf16), h + a <= 256, embed_k <= 512.

   bprx_acf_set_gradient(h, BPRX_ACF_GRAD_FULL) makes bprx_step differentiate the SAME loss with nothing detached (the paper's
   end-to-end training; not what the reference's tape computes).  With d_b = g'_u.(Gi_i - Gi_j), c_b = -sigmoid(-d_b) inside
   the clip range (0 outside) and q_u = sum_{b: user_b = u} c_b (Gi_i - Gi_j) = dL/dg'_u, per distinct user u of the batch and
   history item l (pre_l = the item level's relu input, a_lm = the component level's):
       dGu_u += q_u                dPi_l += alpha_l q_u            dt_l = alpha_l (Pi_l.q_u - sum_l' alpha_l' Pi_l'.q_u)
       dpre_l = dt_l W1i * [pre_l > 0]      dW1i += dt_l relu(pre_l)      dbi0 += dpre_l
       dWiu += g_u (x) dpre_l   dGu_u += Wiu dpre_l     dWiv += Gi_l (x) dpre_l   dGi_l += Wiv dpre_l
       dWip += Pi_l (x) dpre_l  dPi_l += Wip dpre_l     dZ_lm[h:] += beta_lm dpre_l   dbeta_lm = Z_lm[h:].dpre_l
       ds_lm = beta_lm (dbeta_lm - sum_m' beta_lm' dbeta_lm')      da_lm = ds_lm W1c * [a_lm > 0]      dW1c += ds_lm relu(a_lm)
       dZ_lm[:h] += da_lm      dbc0 += da_lm      dWcu += g_u (x) da_lm      dGu_u += Wcu da_lm      [dWci | dWix] = sum F_lm^T dZ_lm
   on top of everything the detached step adds (same loss value, same clip mask, same 2 reg terms, same range-error
   behaviour).  b_1 of both levels: each softmax is invariant under a shift of its inputs, so these two derivatives are
   identically zero and the library writes EXACTLY 2 reg b_1 for them, not rounding noise.  sgd then also moves the Gi / Pi
   rows of the history items of the batch's users; adam_tf23 sweeps as before.  dZ, the per-item gradients and the row tables
   accumulate with float atomics (as the detached step's dGi does), so a full step is not bit-reproducible; the gradients of
   the attention tensors are split-K partials summed in a fixed order.  The mode costs a second buffer the size of Z and a
   few small ones, allocated at the first switch to FULL; in the backward M is limited by 4 (2 M + a) + 2 k + 12 (h + a) + 4
   floats of LDS <= 64 KB (BPRX_E_INVALID otherwise).  The default is BPRX_ACF_GRAD_DETACHED, bit for bit the step above; every
   bprx_bind_acf starts detached again.
   BPRX_E_STATE on a handle that is not ACF-bound, BPRX_E_INVALID for another mode; _get_ returns the mode. */
enum {
  BPRX_ACF_C_WU = 0, BPRX_ACF_C_WI = 1, BPRX_ACF_C_B0 = 2, BPRX_ACF_C_W1 = 3, BPRX_ACF_C_B1 = 4,      /* component_weights */
  BPRX_ACF_I_WU = 5, BPRX_ACF_I_WV = 6, BPRX_ACF_I_WP = 7, BPRX_ACF_I_WX = 8, BPRX_ACF_I_B0 = 9,      /* item_weights */
  BPRX_ACF_I_W1 = 10, BPRX_ACF_I_B1 = 11, BPRX_ACF_NW = 12
};
typedef struct {
  int32_t feat_m, feat_c;           /* M = H*W, C: the feature maps (ACF.py:140-148) */
  int32_t width_c, width_i;         /* h = layers_component[0], a = layers_item[0] */
  int32_t feat_dtype;               /* BPRX_F_FP32 or BPRX_F_BF16 */
  const void *F;                    /* [I, M, C], frozen; read in place (must stay valid while bound) */
  const int64_t *train_ptr;         /* CSR [U+1] / items: training_list (steps, score_pairs) */
  const int32_t *train_items;
  const int64_t *eval_ptr;          /* CSR [U+1] / items: training + validation lists (score_block); NULL = the training lists */
  const int32_t *eval_items;
  float *Pi, *m_Pi, *v_Pi;          /* [I, k] (ACF.py:54) and its adam_tf23 slots */
  float *w[BPRX_ACF_NW];            /* shapes: [k,h] [C,h] [h] [1,h] [1]  [k,a] [k,a] [k,a] [C,a] [a] [1,a] [1] */
  float *m_w[BPRX_ACF_NW], *v_w[BPRX_ACF_NW];
} bprx_acf;
BPRX_API int bprx_bind_acf(bprx_handle *h, const bprx_tables *t, const bprx_acf *a);
/* calculate_beta_alpha for n users (duplicates allowed, any n >= 0) with the histories of the given CSR (indexed by user id):
   out fp32 [n, k] = g'_u. */
BPRX_API int bprx_acf_profiles(bprx_handle *h, const int32_t *users, int64_t n, const int64_t *hist_ptr,
                               const int32_t *hist_items, float *out, void *stream);
/* Why pair p = (user[p], item[p]) scores what it scores, with the histories of the given CSR (indexed by user id, as for
   bprx_acf_profiles).  The score decomposes exactly over the history:
       x_ui = g_u.Gi_i + sum_{l in P(u)} alpha_l (Pi_l.Gi_i) = base + sum_l c_l
   Outputs (device, fp32 / int32): score[n] (the quantity bprx_score_pairs returns with that history), base[n], and per pair the
   `top` history ENTRIES with the largest c_l in non-increasing order of c_l, bit-equal c_l by ascending position (every CSR
   position is an entry: a repeated item is several entries, as it is in the softmax), each [n, top]:
       pos        position in the user's list, 0-based          hist_item  the item id there
       alpha      alpha_l                                       contrib    c_l
       peak       argmax_m beta_lm (the lowest m among equals)  beta_peak  beta_l at the peak (== beta[.., peak] bit for bit)
       beta       [n, top, M], the whole row beta_l; NULL: not written
   Slots beyond the history length (all of them for an empty history): pos = hist_item = peak = -1 and 0.0f in every float field.
   Any n >= 0 (not bounded by max_batch), duplicate pairs and users allowed; 1 <= top <= 32 (BPRX_E_INVALID otherwise);
   BPRX_E_STATE on a handle that is not ACF-bound; indices out of range are clamped and reported by bprx_sync_check.  The call
   reads the tables and writes its outputs and library workspace only (Z / GP scratch, a logit per history entry and h + 2 floats
   per user, allocated at the first call): step index, Adam slots and gradient workspaces are untouched.  It reads hist_ptr[U]
   on the host to size that workspace, so it waits once for the work queued on `stream`.  No float atomics: the outputs are
   reproducible run to run. */
BPRX_API int bprx_acf_explain(bprx_handle *h, const int32_t *user, const int32_t *item, int64_t n, const int64_t *hist_ptr,
                              const int32_t *hist_items, int32_t top, float *score, float *base, int32_t *pos,
                              int32_t *hist_item, float *alpha, float *contrib, int32_t *peak, float *beta_peak, float *beta,
                              void *stream);
enum { BPRX_ACF_GRAD_DETACHED = 0, BPRX_ACF_GRAD_FULL = 1 };
BPRX_API int bprx_acf_set_gradient(bprx_handle *h, int mode);
BPRX_API int bprx_acf_get_gradient(bprx_handle *h);
/* Users the model was not trained on.  For ACF the user representation is made from the history, g' = g + sum_l alpha_l Pi_l with
   both attention levels looking at g, so a new user is its history plus the k numbers g.  The reference's own tape detaches g'
   (ACF.py:203-208): its train step gives Gu nothing but 2 reg g_u, and a fold-in "by the reference's step" would only shrink the
   start row.  DEFINITION: the fold-in therefore differentiates the loss of the user's pairs with respect to g with NOTHING
   detached and everything but g frozen -- the BPRX_ACF_GRAD_FULL derivative restricted to the user's row, whatever gradient mode
   the handle is in (the mode is neither read nor changed, the FULL-mode workspace is neither needed nor allocated).  New user r
   has history entries l in [hist_ptr[r], hist_ptr[r+1]) (a CSR indexed by ROW; every position is an entry, a repeated item is
   several entries, as in bprx_acf_explain) and pairs (i_p, j_p), p in [pair_ptr[r], pair_ptr[r+1]), n_r of them; g starts at
   Gu_rows[r]; for t = 1 .. steps:
       s_lm = W1c.relu(Wcu^T g + Wci^T f_lm + bc0) + bc1        beta_l = softmax_m(s_l)
       t_l  = W1i.relu(Wiu^T g + Wiv^T Gi_l + Wip^T Pi_l + Wix^T sum_m beta_lm f_lm + bi0) + bi1        alpha = softmax_l(t)
       g'   = g + sum_l alpha_l Pi_l                 (g' = g for an empty history)
       x_p  = g'.(Gi_i - Gi_j)    d_p = clip(x_p, -80, 1e8)    s_p = sigmoid(-d_p) inside the clip range (inclusive bounds), 0 outside
       loss_t = sum_p softplus(-d_p) + reg n_r |g|^2
       q    = sum_p -s_p (Gi_i - Gi_j)
       dt_l = alpha_l (Pi_l.q - (sum_l' alpha_l' Pi_l').q)        dpre_l = dt_l W1i * [pre_l > 0]
       dbeta_lm = Z_lm[h:].dpre_l     ds_lm = beta_lm (dbeta_lm - sum_m' beta_lm' dbeta_lm')     da_lm = ds_lm W1c * [a_lm > 0]
       grad = q + Wiu sum_l dpre_l + Wcu sum_l sum_m da_lm + 2 reg n_r g
       BPRX_OPT_SGD: g <- g - lr grad       BPRX_OPT_ADAM_TF23: the sparse-variable rule of the Gu rows, slots starting at zero,
                                            lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t); beta1, beta2, epsilon are the handle's
   The regularisers that do not depend on g are left out of `loss`.  For steps = 1 and sgd, started from a trained user's row with
   that user's training history, the row moves as a BPRX_ACF_GRAD_FULL bprx_step on the batch of the user's pairs moves Gu_u.
   bprx_acf_fold_in: hist_ptr / pair_ptr int64 [n+1], hist_items / pos / neg int32 (device); Gu_rows fp32 [n, k] in / out; loss
   fp32 [n] or NULL: loss_steps, evaluated before the last update.  A user without pairs keeps its row bit for bit and has loss 0,
   whatever its history; a user with pairs and an empty history is bprx_fold_in's BPRMF problem with Bi = 0.  lr, reg, optimizer
   are the call's.  The call first makes Z / GP of the distinct history items current (the preparation every ACF call runs over
   the items it reads, so a bprx_step between two folds is seen by the second); apart from that it writes its outputs only and
   allocates nothing.  fp32 throughout, no float atomics, every sum in one fixed order: two calls return the same bits, and a
   user's result depends on its own history, pairs, start row and the tables only -- not on n, on its position, or on
   BPRX_FOLD_CACHE (1, the default: the first Gi_i - Gi_j rows of a user that fit are kept in LDS across the steps; 0: every step
   gathers every pair's rows again; read by bprx_create).  Any history length and any n_r.  LDS of a workgroup:
       4 (20 + 7 k + 8 M + 7 h + 11 a) bytes  <= 64 KB  (BPRX_E_INVALID otherwise; M = 196, k = 128, h = a = 64: 14.2 KB)
   and behind it the cached pair rows, k floats each, up to a total of 40 KB.  Item ids out of range, in the histories and in the
   pairs, are clamped and reported by bprx_sync_check (BPRX_E_RANGE).  With bf16 features Z is made, as in every ACF call, from
   [Wci | Wix] held as two bf16 halves (16 mantissa bits): the fit sees those two tensors at that precision.
   BPRX_E_INVALID for a NULL handle, a handle that is not bound with bprx_bind_acf, a NULL pointer, n < 0, steps < 1, an unknown
   optimizer, a shape beyond the LDS bound; BPRX_E_STATE for an unbound handle; n == 0: BPRX_OK. */
BPRX_API int bprx_acf_fold_in(bprx_handle *h, const int64_t *hist_ptr, const int32_t *hist_items, const int64_t *pair_ptr,
                              const int32_t *pos, const int32_t *neg, int64_t n, int32_t steps, float lr, float reg,
                              int32_t optimizer, float *Gu_rows, float *loss, void *stream);
/* bprx_acf_profiles for caller-owned rows: out fp32 [n, k] = g'_r of row r of Gu_rows [n, k] with the history
   [hist_ptr[r], hist_ptr[r+1]) of a CSR indexed by ROW.  The same kernel: a slice of the handle's own Gu with the matching slice
   of the training CSR gives the bits of bprx_acf_profiles.  0 <= n < 2^31; errors as for bprx_acf_fold_in. */
BPRX_API int bprx_acf_profile_rows(bprx_handle *h, const float *Gu_rows, int64_t n, const int64_t *hist_ptr,
                                   const int32_t *hist_items, float *out, void *stream);
/* bprx_score_block of an ACF handle for caller-owned rows: out fp32 [(r1-r0), num_items] = g'_r . Gi_i for rows [r0, r1) of
   Gu_rows [n_rows, k] with the histories of a CSR [n_rows + 1] indexed by row, through the scoring kernel of bprx_score_block: the
   handle's own rows with the evaluation histories give its bits.  0 <= r0 <= r1 <= n_rows < 2^31; errors as for
   bprx_acf_fold_in.  A block of more rows than max_batch keeps its profiles in one workspace allocated at the first such call
   and regrown when a block is larger (BPRX_E_NOMEM); smaller blocks allocate nothing.  A call that regrows it first waits for the
   work queued on `stream` (an earlier block's scores may still read the old buffer): issue such blocks on one stream, and not
   under stream capture. */
BPRX_API int bprx_acf_score_rows_block(bprx_handle *h, const float *Gu_rows, int64_t n_rows, const int64_t *hist_ptr,
                                       const int32_t *hist_items, int64_t r0, int64_t r1, float *out, void *stream);

/* ---- AttentiveFashion (AttentiveFashion.py:20-371) on a BPRMF handle ----------------------------------------------------
   Per item i three inputs: an edge image (uint8 [224, 224]; the model sees pixel / 255), a colour histogram [Dc] and a class
   vector [Dk].  Three encoders into k = embed_k columns:
       colour, class   c = dropout(relu(x W1 + b1)) W2                        (W1 [D, 256], b1 [256], W2 [256, k])
       edges           c = dropout(mean(maxpool2x2(relu(conv5x5_same(img) + cb)))) W2    (conv [5, 5, 1, 64], cb [64], W2 [64, k])
   and a three-way attention over c_l, l = (colour, edges, class) in that order:
       a_l = relu((g_u * c_l) W_1 + b_1) W_2 + b_2      alpha = softmax_l(a)      x_ui = sum_k g_u * (sum_l alpha_l c_l) * g_i
   There is no item bias (Bi is bound but neither scored nor trained).  After bprx_bind_attentive
     bprx_step         the reference's step (AttentiveFashion.py:211-258): BPR loss + reg * (|g_u|^2 + |g_i|^2 + |g_j|^2 + the six
                       encoder OUTPUTS + the four attention tensors), the full gradient (nothing detached) into Gu, Gi, every
                       encoder weight and the attention tensors.  Dropout is active (rate, seed below; the stream is the
                       library's own: Philox4x32-10 keyed by seed, counter (unit / 4, sample row, encoder 0/1/2, step index),
                       word unit % 4 >= rate * 2^32 keeps the unit, kept units are scaled by 1 / (1 - rate); sample rows are
                       the B positives, then the B negatives).  sgd, or adam_tf23: the sparse-variable rule on Gu / Gi by
                       whole-table sweeps (the handle never runs the lazy form), the dense ApplyAdam rule on the rest.
                       Every sum of a step runs in a fixed order: a step is bit-reproducible.
     bprx_score_pairs  scores with dropout off
     bprx_score_block  every item is encoded once per parameter state, then one pairwise MFMA attention kernel per user block;
                       eval_* and topk work unchanged on the scores.
   bprx_step_begin / _end and the multi-GPU entry points are rejected (BPRX_E_STATE).  Indices out of range are clamped and
   reported by bprx_sync_check (BPRX_E_RANGE).
   Limits: width <= 128, embed_k <= 512, (embed_k rounded up to 8) * (width rounded up to 32) <= 15 360. */
enum {
  BPRX_AF_COL_W1 = 0, BPRX_AF_COL_B1 = 1, BPRX_AF_COL_W2 = 2,      /* color_encoder.trainable_weights */
  BPRX_AF_EDG_CW = 3, BPRX_AF_EDG_CB = 4, BPRX_AF_EDG_W2 = 5,      /* edges_encoder: conv kernel [25, 64] (tap-major), bias, dense */
  BPRX_AF_CLS_W1 = 6, BPRX_AF_CLS_B1 = 7, BPRX_AF_CLS_W2 = 8,      /* class_encoder */
  BPRX_AF_ATT_W1 = 9, BPRX_AF_ATT_B1 = 10, BPRX_AF_ATT_W2 = 11, BPRX_AF_ATT_B2 = 12,   /* attention_network [k,h] [h] [h,1] [1] */
  BPRX_AF_NW = 13
};
#define BPRX_AF_IMG 224       /* edge images are [224, 224] */
#define BPRX_AF_HID 256       /* hidden units of the colour / class encoders */
#define BPRX_AF_CH 64         /* conv filters */
typedef struct {
  int32_t dim_color, dim_class;     /* Dc, Dk */
  int32_t width;                    /* h = attention_layers[0] */
  float dropout;                    /* rate in [0, 1); 0: no mask and no scaling */
  uint64_t seed;                    /* key of the dropout stream */
  const uint8_t *edges;             /* [I, 224, 224], frozen; read in place (must stay valid while bound) */
  const float *color;               /* [I, Dc], each row already divided by its own max-abs */
  const float *cls;                 /* [I, Dk] */
  float *w[BPRX_AF_NW];
  float *m_w[BPRX_AF_NW], *v_w[BPRX_AF_NW];   /* adam_tf23 slots */
} bprx_attentive;
BPRX_API int bprx_bind_attentive(bprx_handle *h, const bprx_tables *t, const bprx_attentive *a);
/* The three encodings of n listed items with dropout off: out fp32 [3, n, k] (colour, edges, class).  Any n >= 0. */
BPRX_API int bprx_af_encode(bprx_handle *h, const int32_t *items, int64_t n, float *out, void *stream);
/* Scores and attentions of n <= max_batch pairs, dropout off: x fp32 [n], alpha fp32 [n, 3] (colour, edges, class). */
BPRX_API int bprx_af_attention_pairs(bprx_handle *h, const int32_t *user, const int32_t *item, int64_t n, float *x, float *alpha,
                                     void *stream);
/* Why pair p = (user[p], item[p]) scores what it scores (dropout off, n <= max_batch as for bprx_af_attention_pairs).  The score
   is a sum over the three modalities (AttentiveFashion.py:168-209, call), an algebraic identity:
       x_ui    = sum_l s_l,        s_l = alpha_l * sum_k g_uk c_lk g_ik           l = colour, edges, class
   and the edge encoder (AttentiveFashion.py:56-63: Conv2D 5x5 same + relu, MaxPooling2D 2x2, GlobalAveragePooling2D, Dropout,
   Dense(k, no bias)) is the class-activation-map architecture, so the edges share splits over the 112 x 112 pooling windows:
       s_edges = sum_p S(p),       S(p) = (alpha_e / 12544) * sum_c v_c A_c(p)
       v_c     = sum_k W2e[c, k] g_uk g_ik
       A_c(p)  = max over the 2x2 window p of relu(conv_c + b_c)
   alpha is the value the model reports, HELD FIXED: the map decomposes s_edges given alpha_e; it is not a derivative through
   the softmax.  `grid` = G divides 112 (1, 2, 4, 7, 8, 14, 16, 28, 56, 112; BPRX_E_INVALID otherwise).  Outputs (device):
       x fp32 [n], alpha fp32 [n, 3]   exactly the bits bprx_af_attention_pairs returns for the same pairs
       parts fp32 [n, 3]               s_colour, s_edges, s_class
       map fp32 [n, G * G]             cell (a, b), stored at a * G + b, = sum of S(p) over the window rows [a 112/G, (a+1) 112/G)
                                       and columns [b 112/G, (b+1) 112/G); NULL: not written
       peak_cell int32 [n]             index of the largest cell, the lowest index among equal cells; peak_val fp32 [n] its value
   Indices out of range are clamped and reported by bprx_sync_check, as for bprx_af_attention_pairs; the handle stays usable and
   the item claims of the call are released on every exit path.  The conv runs once per DISTINCT item of the call, into a
   workspace of cell sums fp32 [items, G * G, 64] that is allocated at the first use for min(n, 1 GiB / (G * G * 256 B)) items
   (grown when a later call needs more, freed with the handle); a call with more distinct items than that runs in chunks.  The
   call reads the tables and writes its outputs and that workspace only: dropout step index, tables and Adam slots are untouched.
   No float atomics and one summation order per cell: two calls with the same arguments return the same bits. */
BPRX_API int bprx_af_explain(bprx_handle *h, const int32_t *user, const int32_t *item, int64_t n, int32_t grid, float *x,
                             float *alpha, float *parts, float *map, int32_t *peak_cell, float *peak_val, void *stream);
/* bprx_score_block with the attentions next to the scores: scores fp32 [u1-u0, I], alpha fp32 [u1-u0, I, 3] (NULL: scores only). */
BPRX_API int bprx_af_score_block(bprx_handle *h, int32_t u0, int32_t u1, float *scores, float *alpha, void *stream);
/* Users the model was not trained on.  For AttentiveFashion a user is the k numbers g = Gu_u, and the score is not linear in them
   (alpha depends on g), so bprx_fold_in's pair differences do not apply: every step runs the attention forward and backward for
   every pair.  DEFINITION: the reference's train step (AttentiveFashion.py:211-258) on a batch made of this user's pairs, with
   everything but the user's row frozen and DROPOUT OFF -- the encoders do not move, so the fit uses the encodings c_l(item) that
   bprx_af_encode returns and that the scores are computed from.  For new user r with pairs (i_p, j_p),
   p in [pair_ptr[r], pair_ptr[r+1]), n_r of them, g starting at Gu_rows[r]; for t = 1 .. steps:
       pre_l(item) = (g * c_l) W_1 + b_1      a_l = relu(pre_l).W_2 + b_2      alpha = softmax_l(a)
       t_l = sum_k g_k c_lk Gi_k              x = sum_l alpha_l t_l
       d_p = clip(x(i_p) - x(j_p), -80, 1e8)  s_p = sigmoid(-d_p) inside the clip range (inclusive bounds), 0 outside
       loss_t = sum_p softplus(-d_p) + reg n_r |g|^2
       grad   = sum_p -s_p (dx(i_p)/dg - dx(j_p)/dg) + 2 reg n_r g                                   (summed in pair order)
       dx/dg_k = (sum_l alpha_l c_lk) Gi_k + sum_l alpha_l (t_l - x) c_lk sum_h W_1[k,h] [pre_lh > 0] W_2[h]
       BPRX_OPT_SGD: g <- g - lr grad       BPRX_OPT_ADAM_TF23: the sparse-variable rule of the Gu rows, slots starting at zero,
                                            lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t); beta1, beta2, epsilon are the handle's
   The constant regularisers of the reference's loss (Gi, the encoder outputs, the attention tensors) do not move g and are left
   out of `loss`.  For steps = 1 and sgd, started from a trained user's row on a handle bound with dropout = 0, the row moves as
   bprx_step on the same batch moves it.
   bprx_af_fold_in: pair_ptr int64 [n+1], pos / neg int32 (device); Gu_rows fp32 [n, k] in / out; loss fp32 [n] or NULL:
   loss_steps, evaluated before the last update.  A user without pairs keeps its row and has loss 0.  lr, reg, optimizer are the
   call's (the handle's own are not read).  Like bprx_score_block the call first makes the encodings of every item current (a
   bprx_step invalidates them); apart from that it writes its outputs only and allocates nothing.  fp32 throughout, no float
   atomics, every sum in one fixed order: two calls return the same bits, and a user's result depends on its own pairs, its start
   row and the tables only -- not on n, on its position, or on BPRX_FOLD_CACHE (0: every step gathers every pair's encoding and Gi
   rows again instead of keeping the first pairs of a user in LDS; read by bprx_create).  Any n_r, every shape
   bprx_bind_attentive accepts.  Item ids out of range are clamped and reported by bprx_sync_check (BPRX_E_RANGE).
   BPRX_E_INVALID for a NULL handle, a handle that is not bound with bprx_bind_attentive, a NULL pointer, n < 0, steps < 1, an
   unknown optimizer; BPRX_E_STATE for an unbound handle; n == 0: BPRX_OK. */
BPRX_API int bprx_af_fold_in(bprx_handle *h, const int64_t *pair_ptr, const int32_t *pos, const int32_t *neg, int64_t n, int32_t steps,
                             float lr, float reg, int32_t optimizer, float *Gu_rows, float *loss, void *stream);
/* bprx_af_score_block for caller-owned user rows: scores fp32 [(r1-r0), num_items] and alpha fp32 [(r1-r0), num_items, 3] (NULL:
   scores only) for rows [r0, r1) of Gu_rows [n_rows, k].  The same kernel: a slice of the handle's own Gu gives the bits of
   bprx_af_score_block.  0 <= r0 <= r1 <= n_rows < 2^31; errors as for bprx_af_fold_in. */
BPRX_API int bprx_af_score_rows_block(bprx_handle *h, const float *Gu_rows, int64_t n_rows, int64_t r0, int64_t r1, float *scores,
                                      float *alpha, void *stream);
/* Items the model was not trained on, once they have first buyers.  An item without a Gi row scores 0 for everybody, and for
   AttentiveFashion nothing but Gi_i is missing: the encoders give c_l(i) from the item's own inputs.  alpha is computed from g_u
   and the encodings only (AttentiveFashion.py:146-166), Gi_i does not enter it, so the score is LINEAR in the new item's row:
       x_ur = Gi_r . m(u, r)       m(u, r) = g_u o sum_l alpha_l(u, r) c_l(r)
   and fitting the row with everything else frozen and dropout off is the linear-logistic problem of bprx_fold_in_items.

   bprx_af_encode_new: the three dropout-off encodings of n caller-owned inputs (device): edges uint8 [n, 224, 224] (16-byte
   aligned), color fp32 [n, Dc] (each row already divided by its own max-abs), cls fp32 [n, Dk] -> out fp32 [3, n, k].  The kernels
   and workspaces of bprx_af_encode, in chunks of 2 * max_batch rows: fed copies of catalogue items' own inputs it returns the bits
   of bprx_af_encode.  Allocates nothing.  Any 0 <= n < 2^31.

   bprx_af_fold_in_items: pair p of new item r, p in [pair_ptr[r], pair_ptr[r+1]), n_r of them, is (u_p, o_p, role_p) as for
   bprx_fold_in_items; s_p = +1 for role 0 (r is the positive against the catalogue item o_p), -1 for role 1.  C_rows fp32
   [3, n, k]: the encodings of the new items (bprx_af_encode_new).
       alpha^r = softmax_l( relu((g_u o c_l(r)) W_1 + b_1).W_2 + b_2 )
       m_p     = g_u o (alpha^r_0 c_0(r) + alpha^r_1 c_1(r) + alpha^r_2 c_2(r))
       x_o     = sum_l alpha_l(u, o) t_l,   t_l = sum_k c_lk(o) (g_uk Gi_ok)          (the catalogue item's score)
       D_p     = s_p m_p          dc_p = -s_p x_o                                     (formed once: nothing in them moves)
       w starts at Gi_rows[r]; for t = 1 .. steps:
         x_p = w.D_p + dc_p          s = sigmoid(-x_p) inside [-80, 1e8] (inclusive bounds), 0 outside
         g = sum_p (-s D_p) + 2 reg n_r w                                             (summed in pair order)
         loss_t = sum_p softplus(-clip(x_p)) + reg n_r |w|^2
         BPRX_OPT_SGD: w <- w - lr g;  BPRX_OPT_ADAM_TF23: the sparse-variable rule, slots from zero, lr_t as for bprx_fold_in
   The model scores no Bi: there is no bias and no reg / 10 rule.  The constant regularisers of the reference's loss (g_u, the
   encoder outputs, the attention tensors) are left out of `loss`.  For steps = 1 and sgd, started from a catalogue item's own row
   and encodings on a handle bound with dropout = 0, the row moves as bprx_step moves it on the batch that has the item once per
   triplet, in either role.  Role 1 is a sign flip of role 0: D_p and dc_p of (u, o, 1) are the bit negations of those of (u, o, 0).
   pair_ptr int64 [n+1], user / other / role int32 (device); Gi_rows fp32 [n, k] in / out; loss fp32 [n] or NULL: loss_steps,
   before the last update.  An item without pairs keeps its row and has loss 0.  lr, reg, optimizer are the call's.
   work: caller-owned, fp32, at least pair_ptr[n] * KW floats, KW = (k + 1) rounded up to a multiple of 4.  After the call row p
   holds [D_p (k) | dc_p | zeros].
   The call first makes the catalogue encodings current, as bprx_af_fold_in does; apart from that it writes its outputs (Gi_rows,
   loss, work) only and allocates nothing.  No float atomics, every sum in one fixed order: two calls return the same bits, and an
   item's result depends on its own pairs, its start row, its encodings and the tables only -- not on n, on its position, or on
   BPRX_FOLD_CACHE (0: every step reads every pair from work again instead of keeping the first pairs of an item in LDS).  Any
   n_r, every shape bprx_bind_attentive accepts, independent of max_batch.

   bprx_af_score_warm_block: k_af_block given the caller's item rows: scores fp32 [(u1-u0), n] and alpha fp32 [(u1-u0), n, 3]
   (NULL: scores only) of the users [u0, u1) against C_rows [3, n, k] / Gi_rows [n, k] (16-byte aligned where k is a multiple of
   8).  Rows sliced out of bprx_af_encode and Gi give the bits of those columns of bprx_af_score_block.

   bprx_af_audience_block: the same score item-major for the rows [q0, q1): scores fp32 [(q1-q0), num_users], alpha fp32
   [(q1-q0), num_users, 3] (NULL: scores only); out[r][u] has the bits of bprx_af_score_warm_block's out[u][q0 + r].  C_rows and
   Gi_rows both NULL: the items are the catalogue (n must equal num_items; the encodings are made current first) and out[r][u]
   has the bits of bprx_af_score_block's out[u][q0 + r].  0 <= q0 <= q1 <= n.

   All four: BPRX_E_INVALID for a NULL handle, a handle that is not bound with bprx_bind_attentive, a NULL pointer, a bad range,
   steps < 1, an unknown optimizer; BPRX_E_STATE for an unbound handle; n == 0 or an empty range: BPRX_OK, nothing is written.
   User and item ids and roles out of range are clamped and reported once by bprx_sync_check (BPRX_E_RANGE); after any error the
   handle stays usable. */
BPRX_API int bprx_af_encode_new(bprx_handle *h, const uint8_t *edges, const float *color, const float *cls, int64_t n, float *out,
                                void *stream);
BPRX_API int bprx_af_fold_in_items(bprx_handle *h, const int64_t *pair_ptr, const int32_t *user, const int32_t *other,
                                   const int32_t *role, int64_t n, const float *C_rows, int32_t steps, float lr, float reg,
                                   int32_t optimizer, float *Gi_rows, float *loss, float *work, void *stream);
BPRX_API int bprx_af_score_warm_block(bprx_handle *h, int32_t u0, int32_t u1, const float *C_rows, const float *Gi_rows, int64_t n,
                                      float *scores, float *alpha, void *stream);
BPRX_API int bprx_af_audience_block(bprx_handle *h, const float *C_rows, const float *Gi_rows, int64_t n, int64_t q0, int64_t q1,
                                    float *scores, float *alpha, void *stream);
/* The keep-mask bytes (1 = kept) of step index `step` for a batch of n_rows / 2 triplets: out uint8
   [n_rows * 256 | n_rows * 64 | n_rows * 256] (colour hidden units, pooled edge channels, class hidden units). */
BPRX_API int bprx_af_dropout_mask(bprx_handle *h, int64_t step, int64_t n_rows, uint8_t *out, void *stream);
/* The step index the next bprx_step uses (starts at 0 at the first bind; part of a snapshot). */
BPRX_API int64_t bprx_af_get_step(const bprx_handle *h);
BPRX_API int bprx_af_set_step(bprx_handle *h, int64_t step);

/* Model.call((user,item)) -> xui        BPRMF.py:55-76 / VBPR.py:59-86.   x: fp32 [B] */
BPRX_API int bprx_score_pairs(bprx_handle *h, const int32_t *user, const int32_t *item, int64_t B, float *x, void *stream);

/* Model.train_step((user,pos,neg)) -> loss   BPRMF.py:87-125 / VBPR.py:99-144.
   Batch-synchronous: all gradients from pre-update values, duplicate rows summed, one optimizer update.
   loss_out: device fp32 scalar (data term + regularisation, as the reference's loss.numpy()); may be NULL. */
BPRX_API int bprx_step(bprx_handle *h, const int32_t *user, const int32_t *pos, const int32_t *neg, int64_t B,
              float *loss_out, void *stream);

/* The same step in two halves, for item-sharded multi-GPU VBPR: after _begin the dense gradient of the
   shared parameters ([D,d] dE followed by [D] dBp, fp32, WITHOUT the 2*reg*E term) sits in the buffer
   returned by bprx_dense_grad(); the caller all-reduces it (RCCL) and calls _end, which adds the
   regularisation term and applies the optimizer to E/Bp.  bprx_step == _begin + _end. */
BPRX_API int bprx_step_begin(bprx_handle *h, const int32_t *user, const int32_t *pos, const int32_t *neg, int64_t B,
                    void *stream);
BPRX_API int bprx_dense_grad(bprx_handle *h, float **ptr, int64_t *count);
/* The handle-owned item projections P = F.[E|Bp]: [num_items, bprx_proj_stride] fp32, column d the visual bias (0 floats for
   BPRMF).  Read-only introspection for tests: between bprx_step_begin_sparse and bprx_step_end the rows hold what the step's
   forward projection wrote (a masked segment-mode step: zeros in the rows of items its batch does not touch); at other
   times the rows may be stale. */
BPRX_API int bprx_item_proj(bprx_handle *h, float **ptr, int64_t *count);
BPRX_API int bprx_step_end(bprx_handle *h, float *loss_out, void *stream);
/* _begin itself in two halves (bprx_step_begin == _begin_sparse + _begin_dense), so that a collective on the user-side
   gradients overlaps the backward projection:
     _begin_sparse  index pass, item projections P = F.[E|Bp], per-triplet gradients: the USER-side gradients of the batch
                    are final afterwards (bprx_user_grad / bprx_pack_user_msg may follow at once)
     _begin_dense   item rows, W, dE|dBp = F^T W (bprx_dense_grad() is final afterwards); reads the index buffers of
                    _begin_sparse again: they must stay valid and unchanged until it returns */
BPRX_API int bprx_step_begin_sparse(bprx_handle *h, const int32_t *user, const int32_t *pos, const int32_t *neg, int64_t B,
                           void *stream);
BPRX_API int bprx_step_begin_dense(bprx_handle *h, void *stream);
/* Item-sharded multi-GPU helpers.
   bprx_step_project: the item-projection prologue of the step (P = F.[E|Bp]) on its own, so that it can overlap the
   all-to-all that fetches the user rows; a following bprx_step_begin does not repeat it.
   bprx_user_grad / bprx_clear_user_grad: see BPRX_FLAG_EXPORT_USER_GRAD.
   bprx_scatter_add: table[idx[r], :] += scale * rows[r, :] for r < n (fp32 atomics; duplicates in idx are summed):
   the owner-side application of routed gradient rows.  Stateless; all pointers are device pointers. */
BPRX_API int bprx_step_project(bprx_handle *h, void *stream);
BPRX_API int bprx_user_grad(bprx_handle *h, float **dGu, float **dTu);
BPRX_API int bprx_clear_user_grad(bprx_handle *h, int64_t n_rows, int32_t marks_only, void *stream);   /* marks_only: the gradient
   rows were already returned to zero (bprx_route_pack); only the touched-row marks are cleared */
/* Replicated-user multi-GPU step (item-sharded VBPR with every rank holding ALL user rows; needs
   BPRX_FLAG_EXPORT_USER_GRAD and a handle created with num_users = the GLOBAL user count): ONE fixed-size all-gather per
   step, no data-dependent routing, no host synchronisation.
     bprx_user_msg_floats   size (in 4-byte words, a multiple of 4) of one rank's message for `cap` distinct users per batch
     bprx_pack_user_msg     after bprx_step_begin (without the dense part, BPRX_FLAG_DENSE_ALLREDUCE: already after
                            bprx_step_begin_sparse): moves the summed gradient rows of the batch's distinct users out of the
                            staging tables (which are left all-zero) into msg = [count,0,0,0 | ids[cap rounded up to 4] |
                            dGu[cap,k] | dTu[cap,d] | dE|dBp]; more than `cap` distinct users are reported by
                            bprx_sync_check (BPRX_E_RANGE).  msg should be 16-byte aligned (vector copies).
     bprx_apply_user_msgs   after the all-gather (msgs = nranks messages back to back): Gu/Tu[id] += scale * row for
                            every rank's rows, per user in ascending rank order (the occurrences of a user across the
                            messages are chained and one lane group applies them one after the other: every replica
                            performs the same additions in the same order and the replicas stay bit-identical; two
                            launches whatever nranks is), and bprx_dense_grad() = sum over ranks of their dE|dBp parts in
                            rank order; then bprx_step_end.
     bprx_sum_dense_parts   BPRX_FLAG_DENSE_ALLREDUCE handles that want the ORDERED sum instead of an RCCL all-reduce:
                            parts = an all-gather of bprx_dense_grad() (nranks x count floats); bprx_dense_grad() becomes
                            their sum in rank order. */
BPRX_API int64_t bprx_user_msg_floats(const bprx_handle *h, int64_t cap);
BPRX_API int bprx_pack_user_msg(bprx_handle *h, const int32_t *user, int64_t B, int64_t cap, float *msg, void *stream);
BPRX_API int bprx_apply_user_msgs(bprx_handle *h, const float *msgs, int32_t nranks, int64_t cap, float scale, void *stream);
BPRX_API int bprx_sum_dense_parts(bprx_handle *h, const float *parts, int32_t nranks, void *stream);
/* adam_tf23 in the all-to-all modes: the handle (lazy form) takes the Adam steps of the rows it keeps and of E|Bp; the rows whose
   gradients it exports are stepped by their OWNER rank, over its whole shard (TF-2.3's Adam is not lazy: every row decays and
   moves every step, BPRMF.py:123 / VBPR.py:142): the owner adds the returned gradient rows into a zero gradient table
   (bprx_route_scatter_add, scale 1) and calls
     bprx_adam_rows  p, m, v, g: n floats each (the shard, its two moment tables, the gradient table: returned to zero);
                     lr_t from bprx_step_lr of this step -- every rank steps every global step (an empty batch is a step with
                     B = 0), so all ranks hold the same step count;
     bprx_step_lr    the bias-corrected learning rate of the step begun last (sgd: lr). */
BPRX_API int bprx_adam_rows(float *p, float *m, float *v, float *g, int64_t n, float lr_t, float beta1, float beta2, float eps,
                            void *stream);
BPRX_API int bprx_step_lr(const bprx_handle *h, float *lr_t);
BPRX_API int bprx_item_grad(bprx_handle *h, float **dGi, float **dBi);
BPRX_API int bprx_clear_item_grad(bprx_handle *h, int64_t n_rows, int32_t marks_only, void *stream);
BPRX_API int bprx_scatter_add(float *table, int32_t num_rows, int32_t num_cols, const int32_t *idx, const float *rows,
                              int64_t n, float scale, void *stream);

/* Fixed-capacity row routing for the all-to-all multi-GPU modes (user-sharded BPRMF moves item rows, the
   partitioned-user form of item-sharded VBPR moves user rows).  Stateless, device pointers only.  Every rank sends exactly `cap`
   slots to every rank: the collectives take equal splits and nothing is read back to the host to size them.  A routed row is
   [w0 floats | w1 floats | pad] with a stride of (w0 + w1 + 3) & ~3 floats (buffers of nranks*cap such rows).  Per step:
     requester  bprx_route_reset(send_idx, nranks*cap, cursor, nranks)   send_idx <- -1 (unused slot), cursors <- 0
                bprx_route_plan(ids[n] global row ids, rows_per_rank = rows of a full shard, ...) -> slot[n] (owner*cap + position,
                  -1 and *overflow = 1 when the owner's bucket is full or the id is out of range), send_idx[slot] = owner-local row id
                all-to-all(send_idx) -> recv_idx: the rows the other ranks ask this rank for
     owner      bprx_route_gather(t0, w0, t1, w1, num_rows, recv_idx, nranks*cap, out): out[q] = [t0[idx] | t1[idx]] (w1 = 0: one table)
                all-to-all(out) -> got
     requester  bprx_route_unpack(got, slot, n, dst0, w0, dst1, w1): row r of the staging tables = got[slot[r]] (zero row for -1)
                ... local step (BPRX_FLAG_EXPORT_*_GRAD) ...
                bprx_route_pack(grad0, w0, grad1, w1, slot, n, send): send[slot[r]] = [grad0[r] | grad1[r]]; the gradient rows are
                  returned to zero (replaces bprx_clear_*_grad); all-to-all(send) -> back, aligned with recv_idx
     owner      bprx_route_scatter_add(t0, w0, t1, w1, num_rows, recv_idx, back, nranks*cap, scale): t[idx] += scale * row
                  (duplicates summed; unused slots skipped).
   Rows the requesting rank owns itself (my_rank; -1: none) never enter the send buffers: bprx_route_plan gives them slot
   -2 - local row id, bprx_route_unpack copies them from own0 / own1 (the rank's shard tables, own_rows rows) and bprx_route_pack
   adds scale * gradient into own0 / own1 directly.
   bprx_route_plan takes the ids as two arrays back to back (ids[n], then ids_b[n_b]; either may be empty): a triplet batch's
   positives and negatives need no concatenation.
   Row multiplicities (own_cnt / cnt: optional, int32 [rows_per_rank] each, all-zero at the start; NULL = every row is added with
   fp32 atomics): plan counts the requester's own rows into own_cnt, gather counts the rows the other ranks ask for into cnt; pack
   (own rows) and scatter_add (returned rows) then add a row that occurs ONCE with plain 16-byte read-modify-writes and leave the
   counts all-zero again by themselves (see bprx_route.hip).  Pass the same array to the pair (plan, pack) and another one to the
   pair (gather, scatter_add).
   bprx_route_pack with send_idx != NULL also returns send_idx (nslots entries) to -1 and the nranks cursors to 0 for the next
   step's plan: bprx_route_reset is then needed once, before the first step.
   A short last shard (num_rows < rows_per_rank): plan routes an id in [total, nranks * rows_per_rank) to the last rank, whose
   gather writes a zero row for it; unpack does the same for such an id among the requester's own rows (own0 given).  The row's
   gradient is dropped.  bprx_route_gather_checked / bprx_route_unpack_checked are the same calls with one more argument,
   `err` (int32, optional): set to 1 when that happens. */
BPRX_API int bprx_route_reset(int32_t *send_idx, int64_t nslots, int32_t *cursor, int32_t nranks, void *stream);
BPRX_API int bprx_route_plan(const int32_t *ids, int64_t n, const int32_t *ids_b, int64_t n_b, int32_t rows_per_rank, int32_t nranks,
                             int32_t cap, int32_t my_rank, int32_t *slot, int32_t *send_idx, int32_t *cursor, int32_t *overflow,
                             int32_t *own_cnt, void *stream);
BPRX_API int bprx_route_gather(const float *t0, int32_t w0, const float *t1, int32_t w1, int32_t num_rows, const int32_t *idx,
                               int64_t n, float *out, int32_t *cnt, void *stream);
BPRX_API int bprx_route_unpack(const float *got, const int32_t *slot, int64_t n, float *dst0, int32_t w0, float *dst1, int32_t w1,
                               const float *own0, const float *own1, int32_t own_rows, void *stream);
BPRX_API int bprx_route_gather_checked(const float *t0, int32_t w0, const float *t1, int32_t w1, int32_t num_rows,
                                       const int32_t *idx, int64_t n, float *out, int32_t *cnt, int32_t *err, void *stream);
BPRX_API int bprx_route_unpack_checked(const float *got, const int32_t *slot, int64_t n, float *dst0, int32_t w0, float *dst1,
                                       int32_t w1, const float *own0, const float *own1, int32_t own_rows, int32_t *err, void *stream);
BPRX_API int bprx_route_pack(float *src0, int32_t w0, float *src1, int32_t w1, const int32_t *slot, int64_t n, float *send,
                             float *own0, float *own1, int32_t own_rows, float scale, int32_t *own_cnt, int32_t *send_idx,
                             int64_t nslots, int32_t *cursor, int32_t nranks, void *stream);
BPRX_API int bprx_route_scatter_add(float *t0, int32_t w0, float *t1, int32_t w1, int32_t num_rows, const int32_t *idx,
                                    const float *rows, int64_t n, float scale, int32_t *cnt, void *stream);

/* Model.predict_all() rows [u0,u1)   BPRMF.py:78-85 / VBPR.py:88-97.   out: fp32 [(u1-u0), I] */
BPRX_API int bprx_score_block(bprx_handle *h, int32_t u0, int32_t u1, float *out, void *stream);

/* Per-kernel timing with HIP events recorded on the caller's stream around every kernel of bprx_step
   (used by bench.py for the roofline figure; off by default, costs two event records per kernel when on).
   bprx_profile_read synchronises the pending events, ADDS the elapsed milliseconds and launch counts of each
   phase into ms[BPRX_PHASE_COUNT] / launches[BPRX_PHASE_COUNT] and clears the pending list. */
enum {
  BPRX_PHASE_CAST_ET = 0, BPRX_PHASE_PROJ_FWD = 1, BPRX_PHASE_TRIPLET = 2, BPRX_PHASE_PROJ_BWD = 3,
  BPRX_PHASE_REDUCE = 4, BPRX_PHASE_APPLY = 5, BPRX_PHASE_DENSE = 6, BPRX_PHASE_LOSS = 7, BPRX_PHASE_ITEM_SEG = 8,
  BPRX_PHASE_SEG_ALLOC = 9, BPRX_PHASE_ROW_COUNT = 10, BPRX_PHASE_ADAM_CATCHUP = 11, BPRX_PHASE_COUNT = 12
};
BPRX_API int bprx_profile_enable(bprx_handle *h, int on);
BPRX_API int bprx_profile_read(bprx_handle *h, double *ms, int64_t *launches);

/* Evaluator._eval_by_user on the device (Evaluator.py:82-128) for users [u0,u1) from their score rows
   (`scores` = the output of bprx_score_block for the same range).  CSR lists are DEVICE pointers: indptr int64 [U+1]
   indexed by the global user id, items int32.  out: double [(u1-u0), 5] = hr, prec, rec, auc, ndcg per user;
   out[.][0] == -1: the user has no held-out item (skipped by the reference, :88-89); == -2: more than 32 held-out
   items (use the host evaluator).  Exact integer rank counting: for identical fp32 scores the values equal the
   reference's, ties included. */
BPRX_API int bprx_eval_users(bprx_handle *h, int32_t u0, int32_t u1, const float *scores, const int64_t *train_ptr,
                             const int32_t *train_items, const int64_t *eval_ptr, const int32_t *eval_items, int32_t K,
                             double *out, void *stream);

/* The same metrics for an ITEM-SHARDED model (train_rec --world_size N --shard item): every rank holds the score columns of its
   own items [item_lo, item_lo + num_items) of items_total; `scores` = bprx_score_block of the same user range on that rank.
   The CSR lists carry GLOBAL item ids.  Everything Evaluator._eval_by_user counts is additive over item shards:
     bprx_eval_pos     sp fp32 [(u1-u0), 32]: the score of held-out item t where this rank owns it, 0 elsewhere
                       -> the caller all-reduces (sum) sp: exact, one rank contributes each value
     bprx_eval_counts  counts int32 [(u1-u0), 65]: per held-out item #(own items >= sp_t) [0..32), #(own train-only items >= sp_t)
                       [32..64), and #(own train-only items) [64]        -> the caller all-reduces (sum) counts
     bprx_eval_finish  out double [(u1-u0), 5] from the summed counts, as bprx_eval_users (same markers -1 / -2): equal to
                       bprx_eval_users on the concatenated score row (Evaluator.py:96-126). */
BPRX_API int bprx_eval_pos(bprx_handle *h, int32_t u0, int32_t u1, const float *scores, int32_t item_lo, int32_t items_total,
                           const int64_t *eval_ptr, const int32_t *eval_items, float *sp, void *stream);
BPRX_API int bprx_eval_counts(bprx_handle *h, int32_t u0, int32_t u1, const float *scores, int32_t item_lo, int32_t items_total,
                              const int64_t *train_ptr, const int32_t *train_items, const int64_t *eval_ptr,
                              const int32_t *eval_items, const float *sp, int32_t *counts, void *stream);
BPRX_API int bprx_eval_finish(bprx_handle *h, int32_t u0, int32_t u1, int32_t items_total, const int64_t *eval_ptr,
                              const float *sp, const int32_t *counts, int32_t K, double *out, void *stream);

/* Evaluator.store_recommendation on the device (Evaluator.py:225-239) for users [u0,u1): the train items of each user are
   overwritten with -inf IN `scores` (the output of bprx_score_block for the same range; the reference does the same to its
   score matrix, :233) and the K (<= 1024) largest remaining scores are returned best first: idx int32 [(u1-u0), K] (-1 past
   min(K, I)), val fp32 same shape.  flag int32 [(u1-u0)]: 1 = the row's list depends on how EQUAL scores are ordered (ties
   inside the list or at its boundary, or fewer than K unmasked items) -- the reference's order there is numpy's unstable
   argsort; the caller redoes flagged rows with numpy on the (already masked) row.  Equality is float equality: +0.0 and
   -0.0 are equal scores (val keeps the sign of the zero it read).  Unflagged rows equal the reference's output exactly.
   CSR as in bprx_eval_users. */
BPRX_API int bprx_topk(bprx_handle *h, int32_t u0, int32_t u1, float *scores, const int64_t *train_ptr,
                       const int32_t *train_items, int32_t K, int32_t *idx, float *val, int32_t *flag, void *stream);

/* Measurement helper (bench.py): one launch of a plain streaming-read kernel over buf[0, bytes) (device memory, >= 64 MiB;
   sink: >= 8 KiB of device scratch).  Returns the number of bytes the launch reads, or a negative BPRX_E_* code.  Timed by
   the caller on `stream`: the rate this device's HBM delivers to a streaming kernel, quoted beside the 8 TB/s spec. */
BPRX_API int64_t bprx_probe_stream_read(const void *buf, int64_t bytes, void *sink, void *stream);
/* ... with `nt` (streaming, no-retain) loads, the policy of the bf16 feature passes */
BPRX_API int64_t bprx_probe_stream_read_nt(const void *buf, int64_t bytes, void *sink, void *stream);
/* ... with `nt` loads and the launch shape as arguments: `workgroups` (1..512) of `threads` (a multiple of 64, 64..1024), each
   lane keeping `loads_in_flight` (1, 2, 3, 4, 6, 8, 12 or 16) 16-byte loads outstanding -- workgroups * threads *
   loads_in_flight * 16 bytes in flight on the device (scripts/nt_inflight_sweep.py).  buf[0, bytes) must hold at least one
   loop trip of every workgroup; the launch reads whole trips only.  Returns the bytes read, or a negative BPRX_E_* code. */
BPRX_API int64_t bprx_probe_stream_read_nt_shape(const void *buf, int64_t bytes, int32_t workgroups, int32_t threads,
                                                 int32_t loads_in_flight, void *sink, void *stream);
/* Measurement helper: n lane groups each move one row of table[num_rows][row_floats] (fp32, row_floats a multiple of 4)
   picked by idx[] -- mode 0: read; mode 1: read and write back in place (idx distinct).  The access shape of the sparse
   kernels (a table row per index): the rate quoted beside their gather/scatter roofline.  Returns the bytes moved. */
BPRX_API int64_t bprx_probe_row_gather(void *table, int64_t num_rows, int32_t row_floats, const int32_t *idx, int64_t n,
                                       int32_t mode, void *sink, void *stream);

/* Synchronise `stream` and report deferred device-side errors (index out of range). */
BPRX_API int bprx_sync_check(bprx_handle *h, void *stream);

/* ---- index stream (HOST side) --------------------------------------------------------------------------
   DataLoader.all_triple_batches  dataset.py:83-114: per epoch random.shuffle(users) (Python MT19937), walk
   every positive of each user, negative by rejection on np.random.randint (NumPy-legacy MT19937).
   CSR of training_list on the HOST.  bprx_sampler_count = floor(N/bs)*bs*epochs (all epochs when that is 0).
   Output arrays are HOST int32 (the stream is inherently sequential; 12 B/triplet). */
BPRX_API int bprx_sampler_create(const int64_t *indptr, const int32_t *items, int32_t num_users, int32_t num_items,
                        bprx_sampler **out);
BPRX_API int bprx_sampler_destroy(bprx_sampler *s);
BPRX_API int64_t bprx_sampler_count(const bprx_sampler *s, int32_t batch_size, int32_t epochs);
BPRX_API int64_t bprx_sampler_ref_stream(bprx_sampler *s, int32_t batch_size, int32_t epochs, uint32_t py_seed,
                                uint32_t np_seed, int32_t *user, int32_t *pos, int32_t *neg, int64_t cap);

/* ---- throughput sampler (DEVICE side; not in the reference: its sampler tops out at ~4e5 triplets/s) ---------
   Stateless counter-based Philox4x32-10: triplet n = first + b of stream `seed` depends on (seed, n) only.
   Positive: uniform over the num_pos training interactions (pos_user[p], items_sorted[p]); negative: uniform over the
   items that are not positives of that user (rejection with binary search, <= 1024 attempts; after 1024 positives in a
   row -- a user holding nearly every item -- the r-th non-positive of the user, r = mulhi32(block(n, 1024).z, M) over its
   M = num_items - #distinct(list) non-positives: the negative is NEVER a positive, lists may repeat an item.  A user whose
   list holds every item has no negative: the Python sampler constructors raise ValueError for it; passed here, that
   user's negative is an unspecified item in range).  Replaces the role of
   dataset.py:83-122 for throughput runs; its distribution differs from the reference's epoch-permutation walk.
   All pointers are DEVICE pointers: indptr int64 [U+1], items_sorted int32 [num_pos] (ascending inside each user),
   pos_user int32 [num_pos]. */
BPRX_API int bprx_sample_philox(const int64_t *indptr, const int32_t *items_sorted, const int32_t *pos_user,
                                int64_t num_pos, int32_t num_items, uint64_t seed, uint64_t first, int64_t B,
                                int32_t *user, int32_t *pos, int32_t *neg, void *stream);

/* Epoch-walk mode of the device sampler (the reference's visiting order, dataset.py:93-107, as a stateless stream):
   in epoch `epoch` users come in the order perm[0..U) (see bprx_epoch_prepare) and every positive of a user is emitted once, consecutively;
   position n = first + b of the epoch belongs to the user a with epoch_ptr[a] <= n < epoch_ptr[a+1], epoch_ptr being the
   exclusive prefix sums of the list lengths in perm order (int64 [U+1], epoch_ptr[U] = number of interactions).
   pos_slot (optional, int32 [epoch_ptr[U]]): pos_slot[n] = that a, precomputed once per epoch; NULL = binary search per
   triplet (17 dependent loads at U = 100 000: 11.6 vs 6 us per batch of 65 536).
   The caller must keep first + B <= epoch_ptr[U] (a batch that crosses an epoch boundary is two calls).  Negatives as in
   bprx_sample_philox, keyed by (seed; n, epoch).  All pointers are DEVICE pointers. */
/* The user order of epoch `epoch`, prepared on the device without a sort and without the host:
     bprx_epoch_prepare  perm[a] (int32 [num_users]) = the user in slot a: a keyed permutation evaluated pointwise (4-round Feistel
                         network over 2*ceil(bits(U-1)/2) bits with Philox round functions keyed by (seed, epoch), cycle-walked
                         into [0, U); CPU twin: the oracle's orc_epoch_perm), and lens[a] (int64 [num_users]) = the length of
                         that user's list; the caller's inclusive prefix sums of lens behind a leading 0 are epoch_ptr;
     bprx_epoch_slots    pos_slot[p] = a for the positions p in [epoch_ptr[a], epoch_ptr[a+1]) (pos_slot: int32 [num_pos]).
   Three launches and one scan per epoch; an epoch switch never waits for the host. */
BPRX_API int bprx_epoch_prepare(uint64_t seed, uint32_t epoch, int32_t num_users, const int64_t *indptr, int32_t *perm,
                                int64_t *lens, void *stream);
BPRX_API int bprx_epoch_slots(const int64_t *epoch_ptr, int32_t num_users, int32_t *pos_slot, int64_t num_pos, void *stream);
BPRX_API int bprx_sample_epoch(const int64_t *indptr, const int32_t *items_sorted, const int32_t *perm,
                               const int64_t *epoch_ptr, const int32_t *pos_slot, int32_t num_users, int32_t num_items, uint64_t seed,
                               uint32_t epoch, int64_t first, int64_t B, int32_t *user, int32_t *pos, int32_t *neg,
                               void *stream);

/* The same two samplers, told which handle's NEXT step will consume the batch (h may be NULL: exactly the calls above).
   When that handle steps in segment mode (num_items up to 2 M), the sampler also writes the owner byte (id >> shift, shift = 8 up to
   65 536 items) and the local part (a byte, or 16 bits) of every sampled item id into planes the handle owns (2-3 B per occurrence); the index pass of the step called with exactly these
   pos / neg pointers and B == batch_size (a multiple of 16) then scans one byte per occurrence instead of four (its owner
   workgroups each read the whole batch).  batch_offset / batch_size: this call fills triplets [batch_offset, batch_offset + B)
   of a batch of batch_size, whose arrays start at user - batch_offset, pos - batch_offset, neg - batch_offset (an epoch
   crossing fills a batch in two calls; the call with batch_offset 0 comes first).  The caller must not change pos / neg between
   the sampler and the step; any other step on the handle simply ignores (and drops) the planes.  Results are identical.
   Up to 65 536 items (and 2 * batch_size <= 2^24) each call also leaves its item occurrences sorted by owner in queues the handle
   owns (4 B per occurrence; a later call of the batch continues behind the earlier ones): bprx_index_pass_queue below. */
BPRX_API int bprx_sample_philox_h(bprx_handle *h, const int64_t *indptr, const int32_t *items_sorted, const int32_t *pos_user,
                                  int64_t num_pos, int32_t num_items, uint64_t seed, uint64_t first, int64_t B, int32_t *user,
                                  int32_t *pos, int32_t *neg, int64_t batch_offset, int64_t batch_size, void *stream);
BPRX_API int bprx_sample_epoch_h(bprx_handle *h, const int64_t *indptr, const int32_t *items_sorted, const int32_t *perm,
                                 const int64_t *epoch_ptr, const int32_t *pos_slot, int32_t num_users, int32_t num_items,
                                 uint64_t seed, uint32_t epoch, int64_t first, int64_t B, int32_t *user, int32_t *pos, int32_t *neg,
                                 int64_t batch_offset, int64_t batch_size, void *stream);
/* Hard negatives (dynamic negative sampling): the hard forms of the two samplers above.  The user and the positive of a stream
   position are the uniform stream's.  Candidate c (0 <= c < candidates <= 16) of position n is the uniform samplers' rejection
   draw with the third counter word c * 2048 + a instead of a (attempts a = 0, 1, .., the 1024 fallback included): candidate 0 is
   the uniform negative, every candidate is uniform over the user's non-positives, candidates may repeat.  The negative is the
   candidate with the largest
     s_c = Gu_u.Gi_j + Bi_j                                  (BPRMF)
     s_c = Gu_u.Gi_j + Bi_j + Tu_u.Ps_j[:d] + Ps_j[d]        (VBPR, plain or factored)
   in fp32 (the summation order is the kernel's); ties go to the smallest c, a NaN never wins against a number.  candidates == 1
   reproduces bprx_sample_*_h bit for bit.  Planes and queues of the chosen negatives are left for the handle's next step as above.
   h is required: a bound BPRMF or VBPR handle whose tables are whole (not a multi-GPU staging handle) and whose num_items is the
   sampler's.  The rows of Gu / Gi / Bi / Tu are read AS STORED: the call runs no lazy adam_tf23 catch-up, so rows the batches have
   not touched lately lag by their pending momentum steps.  It runs on `stream` behind the previous step.
   Ps (VBPR: required; BPRMF: ignored): fp32 [num_items, bprx_proj_stride] device memory of the caller, filled by
   bprx_hard_snapshot; between two refreshes it lags E / Bp.  Both lags steer the choice only: the step computes its gradient
   from current values.
   cand_out (int32 [B, candidates]) / score_out (fp32 [B, candidates]), both optional: what was drawn and what was compared.
   BPRX_E_INVALID for a NULL handle or pointer, an ACF or AttentiveFashion handle, candidates outside 1..16, a VBPR handle without
   Ps, another num_items; BPRX_E_STATE for an unbound handle.  After any error the handle stays usable. */
BPRX_API int bprx_sample_philox_hard(bprx_handle *h, const int64_t *indptr, const int32_t *items_sorted, const int32_t *pos_user,
                                     int64_t num_pos, int32_t num_items, uint64_t seed, uint64_t first, int64_t B, int32_t *user,
                                     int32_t *pos, int32_t *neg, int64_t batch_offset, int64_t batch_size, void *stream,
                                     int32_t candidates, const float *Ps, int32_t *cand_out, float *score_out);
BPRX_API int bprx_sample_epoch_hard(bprx_handle *h, const int64_t *indptr, const int32_t *items_sorted, const int32_t *perm,
                                    const int64_t *epoch_ptr, const int32_t *pos_slot, int32_t num_users, int32_t num_items,
                                    uint64_t seed, uint32_t epoch, int64_t first, int64_t B, int32_t *user, int32_t *pos,
                                    int32_t *neg, int64_t batch_offset, int64_t batch_size, void *stream, int32_t candidates,
                                    const float *Ps, int32_t *cand_out, float *score_out);
/* Fills Ps = F.[E|Bp] of every item from the bound tables as they are now (fp32, bf16 or fp8 features, plain or factored): the
   forward projection written straight into the caller's buffer.  Like every gated call it first settles a deferred dense update
   and makes the [E|Bp]^T image current.  It is not the handle's own P and leaves the plan of the next step alone.  BPRMF: BPRX_OK,
   nothing is touched (Ps may be NULL).  BPRX_E_INVALID for a NULL handle, a VBPR handle with Ps == NULL, an ACF or AttentiveFashion
   handle; BPRX_E_STATE for an unbound handle. */
BPRX_API int bprx_hard_snapshot(bprx_handle *h, float *Ps, void *stream);

/* What the index pass of the handle's last step read: 0 = no segment-mode step yet, 1 = the int32 index arrays,
   2 = the sampler's byte planes.  (Introspection for tests and benchmarks.) */
BPRX_API int bprx_index_pass_kind(const bprx_handle *h);
/* Whether the owner workgroups of that index pass read the sampler's owner queues (1) or scanned the planes / the index arrays
   (0).  Up to 65 536 items and 2 * batch_size <= 2^24 the samplers above also leave every 256 triplets' item occurrences sorted
   by owner (id >> 8), so that an owner reads its own records instead of the whole batch; bprx_index_pass_kind is 2 either way.
   BPRX_INDEX_QUEUE=0 (read by bprx_create) keeps the plane scan.  Results are identical up to the order in which equal items'
   occurrences are ranked, as between two runs of the scan.  (Introspection for tests and benchmarks.) */
BPRX_API int bprx_index_pass_queue(const bprx_handle *h);
/* Whether the projections of the handle's last step left out the feature rows of the items its batch did not touch:
   0 = both streamed every row (list mode, a step after bprx_step_project or bprx_score_block, fp32 features, fp8 features or
   more than nine column tiles unless BPRX_PROJ_MASK=2, BPRX_PROJ_MASK=0, no step yet), 1 = both passes masked, 2 = the forward pass alone (a split of the backward pass too long for its row bits),
   3 = the backward pass alone (forward kernel forms without the mask: feat_dim not a multiple of 256 / 512, wide fp8
   projections).  Results are the same either way.  (Introspection for tests and benchmarks.) */
BPRX_API int bprx_proj_mask_kind(const bprx_handle *h);

#ifdef __cplusplus
}
#endif
#endif /* BPRX_H_ */
