// bprx_internal.h -- private state of libbprx.so (C ABI: include/bprx.h).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <atomic>
#include <utility>
#include <vector>

#include "bprx.h"
#include "bprx_device.h"

#define BPRX_DENSE_BLOCKS 2048

// Every device buffer of the library belongs to a DevPool, a member of the struct that holds the buffer's pointer (the handle,
// AcfState, AfState).  The pool records each allocation with the address of that pointer and frees them all when it is cleared or
// destroyed: there is no list of names to keep in step.  bprx_live_allocs (bprx_live_device_allocs) counts them process-wide.
inline std::atomic<int64_t> bprx_live_allocs{0};

struct DevPool {
  struct Rec { void **slot; void *p; };
  std::vector<Rec> recs;
  hipError_t err = hipSuccess;    // the first failure: sticky, zeros() does nothing more until a rollback takes it

  DevPool() = default;
  DevPool(const DevPool &) = delete;
  DevPool &operator=(const DevPool &) = delete;
  ~DevPool() { (void)rollback(0); }

  // *slot = n zero-filled elements (n == 0: nullptr, a success).  Allocate everything, then test ok() once.
  template <typename T> void zeros(T **slot, size_t n) { get((void **)slot, n * sizeof(T), true); }
  bool ok() const { return err == hipSuccess; }
  size_t mark() const { return recs.size(); }
  // Frees what was allocated after `mark`, nulls the owning pointers, and returns (and forgets) the failure, if any.  A mark
  // holds within one function only: regrow() takes records out of the middle.
  hipError_t rollback(size_t mark) {
    for (; recs.size() > mark; recs.pop_back()) drop(recs.back());
    return std::exchange(err, hipSuccess);
  }
  // One buffer on its own: what *slot owns (if anything) goes, n new elements (not zeroed unless asked) take its place.  A failure
  // is returned, not kept, and leaves *slot null.  The caller has made sure that no enqueued work still reads the old buffer.
  // Also the first allocation of a buffer made on demand (gF, xu, erank), whose failure must not stop later calls.
  template <typename T> hipError_t regrow(T **slot, size_t n, bool zero = false) {
    for (size_t i = 0; i < recs.size(); ++i)
      if (recs[i].slot == (void **)slot) { drop(recs[i]); recs.erase(recs.begin() + i); break; }
    const size_t mk = mark();
    get((void **)slot, n * sizeof(T), zero);
    return ok() ? hipSuccess : rollback(mk);
  }

 private:
  void get(void **slot, size_t bytes, bool zero) {
    if (!ok() || bytes == 0) return;
    void *p = nullptr;
    if ((err = hipMalloc(&p, bytes)) != hipSuccess) { (void)hipGetLastError(); return; }   // (or the next launch check reports it)
    recs.push_back({slot, p});
    *slot = p;
    ++bprx_live_allocs;
    if (zero) err = hipMemset(p, 0, bytes);
  }
  void drop(const Rec &r) { (void)hipFree(r.p); *r.slot = nullptr; --bprx_live_allocs; }
};

struct AcfState;   // bprx_acf.hip
struct AfState;    // bprx_attentive.hip

constexpr int ADAM_HIST = 8192;   // lazy adam_tf23: steps of lr_t the device ring lr_hist holds (a power of two)
constexpr int IX_RMAX = 8192;     // k_index_seg: items an owner workgroup can own (LDS counters)
constexpr int IX_LPAD = 4;        // chunk-list slots of an owner beyond one per item (hot items' extra chunks; more: overflow list)

// ---- the samplers' owner queues (DESIGN §4 "Owner queues") ----
// Every 256-thread sampler workgroup leaves its up to 512 item occurrences as ONE region of 4-byte records, sorted by owner
// (id >> 8: a counting sort in LDS), and for every owner the [lo, hi) slots it holds in that region: an owner workgroup of
// k_index_seg then reads its own records only, not the whole batch.
//   record        (occ << 8) | (id & 255), occ in [0, 2B): b for the positive of triplet b, B + b for its negative (seg_rank's index)
//   records       [regions][IXQ_REC]: slot s of region r at r * IXQ_REC + s
//   ranges        [IXQ_BINS][stride]: owner w's range in region r at w * stride + r (an owner reads consecutive words), lo | hi << 16
// A batch filled by several sampler calls numbers its regions on: stride = ixq_regions(max_batch) holds a batch of two calls.
constexpr int IXQ_WG = 256;                  // triplets per sampler workgroup = per region
constexpr int IXQ_REC = 2 * IXQ_WG;          // records of a region
constexpr int IXQ_BINS = 256;                // owners (the planes' owner byte at shift 8)
constexpr int64_t IXQ_MAX_OCC = 1 << 24;     // occ has 24 bits: 2B <= 2^24
__host__ __device__ inline uint32_t ixq_pack(uint32_t occ, uint32_t id) { return (occ << 8) | (id & 255u); }
__host__ __device__ inline uint32_t ixq_occ(uint32_t rec) { return rec >> 8; }
__host__ __device__ inline uint32_t ixq_local(uint32_t rec) { return rec & 255u; }
__host__ __device__ inline uint32_t ixq_range(uint32_t lo, uint32_t hi) { return lo | (hi << 16); }
__host__ __device__ inline uint32_t ixq_lo(uint32_t range) { return range & 0xffffu; }
__host__ __device__ inline uint32_t ixq_hi(uint32_t range) { return range >> 16; }
__host__ __device__ inline int64_t ixq_regions(int64_t max_batch) { return max_batch / IXQ_WG + 2; }
__host__ __device__ inline size_t ixq_rec_at(int region, int slot) { return (size_t)region * IXQ_REC + (size_t)slot; }
__host__ __device__ inline size_t ixq_range_at(int owner, int region, int stride) { return (size_t)owner * (size_t)stride + (size_t)region; }

// What ONE BPRMF / VBPR training step does: every decision about its form, made once by plan_step (below the handle) from the
// configuration, the create-time policies and the state carried from step to step.  bprx_step_begin_sparse commits it to
// bprx_handle::step; bprx_step_begin_dense, bprx_step_end and every launcher read it and decide nothing themselves.
struct StepPlan {
  int error;                      // 0, or why there is no step: PLAN_E_EMPTY (nothing else is filled in)
  int64_t B;                      // triplets (0: the empty batch of a replicated rank)
  const int32_t *user, *pos, *neg;   // the step's index buffers (nullptr for the empty batch)
  // optimizer
  int64_t adam_t;                 // optimizer.iterations of this step (sgd: unchanged)
  float lr_t;                     // sgd: lr; adam_tf23: the bias-corrected step size at adam_t (bprx_step_lr)
  bool adam_sync_first;           // lazy Adam: the lr_t ring would wrap, every row is caught up to adam_t - 1 first
  bool catchup, catchup_aside;    // lazy Adam: k_adam_catchup runs; on the side stream beside the forward projection
  // form of the step
  bool list_mode;                 // touched-item list: both projections over the batch's DISTINCT items only
  bool item_mode;                 // item-side gradients by per-item occurrence segments (k_item_seg); false: global float
                                  //    atomics into the staging tables + claim-apply
  bool seg_users;                 // segment-mode step whose users are finished inside k_triplet_seg (sgd, gradients not
                                  //    exported): no apply pass for them
  bool mask;                      // segment mode: the projections leave out the rows of the items the batch does not touch
                                  //    (where a masked kernel form exists: proj_fwd_takes_mask / proj_bwd_takes_mask)
  bool index_first;               // the index pass runs before the forward projection (list, mask), otherwise after it
  bool row_count;                 // atomic staging / list mode: the index pass is k_row_count (neither: no index pass)
  bool idx8;                      // the index pass scans the sampler's byte planes of this very batch
  bool idxq;                      // ... its owners read the sampler's owner queues of this very batch instead (bprx_index_pass_queue)
  int idxq_regions;               // ... which hold this many regions
  int idx_kind;                   // bprx_index_pass_kind: of this step if it is a segment-mode step, else of the last one
  bool project, fwd;              // VBPR, no bprx_step_project before: [E|Bp]^T images are made; P is projected (not current)
  int fast, fastU, fastI;         // sgd: rows used by exactly one triplet are updated in place; per side (off for exported rows)
  bool use_list;                  // both sides fast: the apply pass walks the list of the batch's SHARED rows
  bool list_reset_cnt;            // list mode: k_cast_W_rows resets cntI (no exclusive-row fast path on the item side)
  bool w_memset, leaves_w_dirty;  // fp32 W is cleared before the triplet kernel; this step leaves it not all-zero
  int64_t list_bound;             // list mode: host-side bound of the list length, min(2B, I)
  int32_t *list_cur, *list_next;  // list mode: ilist_n cursor of this step, and the one k_dense_update clears for the next
  int seg_cur;                    // segment mode: cursor triple (seg_cursor + 3 * seg_cur) this step's kernels read
  int ix_R, ix_nown;              // k_index_seg: items per owner workgroup, owner workgroups
  int seg_lead_over;              // slots of the owners' regions in seg_lead (the overflow list follows)
  int slist_cur;                  // slist_n cursor of this step
  int SK_step;                    // split-K slabs written by this step's backward projection (<= SK)
  bool fused_reduce;              // bprx_step: k_dense_update sums the split-K slabs itself (no k_reduce_parts)
  int apply;                      // APPLY_*: what bprx_launch_apply does
  int fk, ek;                     // row kinds [fk, ek) of the apply pass (0 users, 1 / 2 positive / negative items)
  bool dense_launch;              // bprx_step_end: k_dense_update runs (GradFashion: only for its housekeeping)
  // the dense update across two steps (bprx_step only; DESIGN §4 "The deferred dense update")
  bool defer_ok;                  // this step's update may wait for the next step's index pass (bprx_step decides with the loss pointer)
  bool carry_dense;               // the LAST step's update is pending and rides in this step's k_index_seg launch
  bool settle_first;              // ... is pending and this step has no such launch: k_dense_update runs before anything else
};
enum { PLAN_E_EMPTY = 1 };           // an empty batch on a handle without exported gradients
enum { APPLY_NONE = 0, APPLY_SGD_LIST, APPLY_SGD, APPLY_ADAM_LAZY, APPLY_ADAM_SWEEP };

// What one dense E|Bp update is given (k_dense_update, and the dense workgroups of k_index_seg: bprx_sparse.hip), every value
// fixed when the step that owns the update ends: bprx_dense_args.
struct DenseArgs {
  float *E, *Bp, *mE, *vE, *mBp, *vBp;
  const float *dEp, *part;        // the (all-reduced) gradient, or the split-K slabs to sum (part != nullptr)
  int SK, D, d, PS, adam;
  float lr_t, reg, b1, b2, eps;
  double *sqpart;                 // [nvb] per-block sums of squares (the loss), or nullptr
  float gscale;
  uint16_t *Et, *EtF;             // bf16 features: the images to refresh
  const int32_t *ilist, *ilist_n; // list mode: the rows of W to clear
  int32_t *ilist_n_next;
  int bound;
  float *W;
  int32_t *cnt_reset;
  uint32_t *absmax_out;           // fp8 features: the max|E,Bp| slot
  int upd;
  int nvb, vT;                    // blocks of the update and threads of one (a multiple of 64, 256 .. 1024)
};

// A dense update that bprx_step did not launch: the next segment-mode bprx_step runs it inside its k_index_seg launch, every other
// call settles it first with k_dense_update (bprx_settle_pending).  Carried flags (et_valid, absmax_valid, p_valid, dense_blocks)
// are already as if it had run.
struct DensePending {
  bool on;
  DenseArgs a;                    // with the hyper-parameters of ITS step (a later bprx_set_hyper does not reach it)
  float *loss_out;                // loss lag: where that step's loss goes once the update has run (or nullptr)
  int64_t loss_B;
  int loss_nsq;
  float loss_reg;
};

struct bprx_handle {
  bprx_config cfg;
  bprx_tables t;
  bool bound;
  // lazy-exact adam_tf23 (bprx_sparse.hip): rows are brought up to date when they are read
  bool adam_lazy;
  int32_t *lastU, *lastI;  // [U], [I] step up to which the row (Gu/Tu resp. Gi/Bi and their slots) is current
  float *lr_hist;          // ring of the last ADAM_HIST steps' lr_t
  char err[512];

  // ---- scratch owned by the handle (device): every pointer below that the library allocates belongs to `mem` ----
  DevPool mem;
  float *dGu, *dGi, *dBi, *dTu;   // dense fp32 gradient staging, same shapes as the tables; all-zero between steps
  uint32_t *flagU, *flagI;        // "row touched this step" marks (sgd claim)
  float *lossb;                   // [max_batch] per-triplet loss (data + per-occurrence regularisation)
  double *loss_acc;               // [BPRX_DENSE_BLOCKS] per-block partial sums of ||E||^2+||Bp||^2 (k_dense_update)
  int dense_blocks;               // blocks of the last k_dense_update launch
  int dense_defer;                // env BPRX_DENSE_DEFER, read at create: 1 (default) bprx_step may defer its dense update, 0 never
  int loss_lag;                   // bprx_set_loss_lag: a step with a loss pointer may defer too (its loss lands one launch later)
  DensePending pend;              // the deferred update, if any: set by bprx_step, taken by the next index pass / bprx_settle_pending

  // ---- the step in flight ----
  StepPlan step;                  // committed by bprx_step_begin_sparse; read-only until the next one (the launchers, bprx_step_lr,
                                  //    bprx_index_pass_kind / bprx_proj_mask_kind; ACF / AttentiveFashion steps record lr_t only)
  int step_stage;                 // 0 = none, 1 = bprx_step_begin_sparse done (user gradients final), 2 = whole _begin done

  // ---- carried from step to step (each with its writers; DESIGN §4 "How a step is planned") ----
  int64_t adam_t;                 // optimizer.iterations: commit_plan (+1 per adam_tf23 step), bprx_set_adam_step
  int64_t adam_synced;            // lazy Adam: every row is current at least up to this step: bprx_launch_adam_sync / _reset
  bool proj_fresh;                // bprx_step_project already ran for the coming step: set there, cleared by commit_plan
  bool et_valid;                  // the bf16/fp8 image Et matches the bound E/Bp: set by bprx_launch_cast_Et, by bprx_step_end for
                                  //    the images k_dense_update wrote; cleared by bprx_step_end, bind, tables_dirty
  bool p_valid;                   // P holds the projections of ALL items for the bound E/Bp: set by bprx_step_project /
                                  //    bprx_score_block, cleared by bprx_step_end, bind, tables_dirty
  bool absmax_valid;              // fp8: qs[2 + qs_slot] already holds max|E,Bp| of the bound values: set by bprx_step_end (left
                                  //    there by k_dense_update), consumed by bprx_launch_cast_Et
  int qs_slot;                    // fp8: the max|E,Bp| slot of the next k_cast_Et8: flipped by bprx_launch_cast_Et (also run
                                  //    outside steps: bprx_score_pairs / _block, bprx_step_project)
  bool W_dirty;                   // the fp32 W table is not all-zero (left so by a dense fp32-feature step): commit_plan
  int list_slot;                  // ilist_n cursor of the next list-mode step: flipped by bprx_step_end after a list-mode step
  int seg_slot;                   // seg_cursor triple of the next segment-mode step: flipped by commit_plan
  int slist_slot;                 // slist_n cursor of the next shared-row-list step: flipped by commit_plan
  // byte planes of the item ids of the NEXT step's batch, written by the library's own device samplers (bprx_sample_*_h) when
  // own8 = id >> idx8_shift (the owner workgroup of k_index_seg, 2^shift items each: at most 256 owners), loc8 = the rest; [2 * max_batch]
  // each (positives, then negatives).  idx8_pos / idx8_neg / idx8_B: the buffers and batch size they belong to; idx8_n: triplets
  // filled so far (-1: invalid): written by the samplers; consumed (idx8_n = 0) by commit_plan, whatever the step does with them.
  const int32_t *idx8_pos, *idx8_neg;
  int64_t idx8_B, idx8_n;
  // the owner queues of the same batch (same tags): regions filled so far (-1: a call of this batch left none) and the triplets
  // they hold; written and consumed with the planes
  int64_t idxq_n, idxq_trip;

  int32_t *errflag;               // device-side deferred error (index out of range)
  // VBPR projection state
  int PS;                         // padded row stride of P/W/Et: 16*ceil((d+1)/16)
  float *P;                       // [I][PS]  item projections f_i.[E|Bp]
  float *W;                       // [I][PS]  sum_b +-g_b*[theta_u|1] per item; all-zero between steps
  void *Wb;                       // bf16 [I][PS] copy of W for the backward MFMA
  float *Ppair;                   // [max_batch][PS] projections for bprx_score_pairs
  void *Ft;                       // tiled copy of F (bf16 / fp8 features): 8-KB blocks of 32 items x 256 B, see k_tile_F
  void *Et;                       // bf16 [PS][D]: [E|Bp|0]^T, refreshed every step
  void *EtF;                      // the same values in MFMA-fragment-major order (k_proj_fwd_rows), see k_cast_Et
  void *EtS;                      // fp8 features, PS/16 >= 10: the codes in the order of k_proj_fwd_f8s (scaled fp8 MFMA)
  float *dEp;                     // [D*d + D] dense gradient of E then Bp (no regularisation term)
  float *part;                    // [SK][D][PS] split-K slabs of the backward projection
  int SK;
  float *qs;                      // fp8 features: [1] = 1/(feat_scale*sE) for P, [2], [3] = max|E,Bp| bits (uint32, atomicMax;
                                  //               two slots used alternately, the idle one is cleared by k_cast_Et8)
  int fast_rows;                  // sgd: rows used by exactly one triplet of the batch are updated in place
  int32_t *cntU, *cntI;           // [U], [I] row multiplicities of the current batch (all-zero between steps)
  int seg_policy;                 // 0 never, 1 per step (2B >= I), 2 always (env BPRX_ITEM_MODE)
  // Occurrence segments (segment mode), built by ONE launch of k_index_seg (bprx_sparse.hip): workgroup w OWNS the item
  // range [w*R, (w+1)*R): it scans all 2B item occurrences, counts and ranks those of its items in LDS (no global atomics),
  // prefix-sums its counts, reserves the entries with one cursor atomic and lists its items' chunks for k_item_seg.
  int32_t *seg_rank;              // [2 * max_batch] rank of occurrence (role*B + b) among its item's occurrences
  int32_t *seg_cnt;               // [I] occurrences of the item in this batch (rewritten for every item by each index pass)
  int32_t *seg_ptr;               // [I] start of the item's segment in seg_ent
  int32_t *seg_cursor;            // [6] two (overflow entries, overflow chunks, listed users) cursor triples used by alternate
                                  //     steps: an index pass clears the triple of the NEXT step
  void *seg_lead;                 // int4 [seg_lead_cap] {item, first entry, entries of the chunk, entries of the item}: k_item_seg's work list
  int64_t seg_lead_cap;
  int64_t seg_ent_cap;            // entries allocated in seg_ent
  // user side of a segment-mode sgd step: k_triplet_seg sums the runs of equal users in LDS and adds the run sums to the staging
  // rows; finishing lane groups at the front of k_item_seg's grid apply the totals (no apply launch).  k_item_seg's item groups,
  // which need the PRE-update user rows, read them from uold (saved by the run that starts at the user's slot).
  int32_t *uslot_of;              // [U] batch position of the user's first run head = the user's slot (valid for users of the batch)
  int32_t *ulist;                 // [max_batch] the batch's users (first-run order): walked by k_item_seg's finishing groups
  float *uold;                    // [max_batch][k + d] pre-update [gamma_u | theta_u] of the slot's user
  uint8_t *own8, *loc8;           // the sampler's byte planes (idx8_* above)
  int idx8_shift;                 // own8 = id >> idx8_shift (8: loc8 holds bytes; 9..13, num_items up to 2 M: loc8 holds uint16 id & (2^shift - 1))
  // Untouched items' feature rows out of both streaming projections (segment-mode steps): the index pass runs BEFORE
  // the forward projection and both projections read seg_cnt as the per-item "occurs in this batch" mask.
  int proj_mask;                  // env BPRX_PROJ_MASK, read at create: 0 never, 1 (default) bf16 features up to nine column tiles, 2 every masked form
  bool idx8_ready(bool item_mode, const int32_t *pos, const int32_t *neg, int64_t B) const {
    return item_mode && own8 && B > 0 && idx8_n == B && idx8_B == B && idx8_pos == pos && idx8_neg == neg && B % 16 == 0;
  }
  uint32_t *qrec, *qrange;        // the samplers' owner queues: records [ixq_regions(max_batch)][IXQ_REC], ranges [IXQ_BINS][the same];
                                  //    not allocations of their own: they lie behind the owner plane in own8's buffer
  int index_queue;                // env BPRX_INDEX_QUEUE, read at create: 1 (default) the owners of k_index_seg read the queues, 0 they scan the planes
  // the samplers fill queues for a batch of B on this handle at all (byte locals, occ in 24 bits)
  bool idxq_feeds(int64_t B) const { return index_queue && qrec && qrange && idx8_shift == 8 && 2 * B <= IXQ_MAX_OCC; }
  // the planes of this very batch are ready (idx8_ready) and every sampler call that filled them left its regions too
  bool idxq_ready(bool idx8, int64_t B) const { return idx8 && idxq_feeds(B) && idxq_n > 0 && idxq_trip == B; }
  int32_t *hot_done;              // [I] finished chunks of a hot item (k_item_seg), all-zero between steps
  void *seg_ent;                  // [seg_ent_cap] 8-byte entries {user or user slot | role << 31, g_b}: the owners' regions (twice
                                  //     the expected occupancy each) + 2 * max_batch for the owners that overflow theirs
  // touched-item list (sparse batches, 2B < I): both projections run over the batch's DISTINCT items only
  int list_policy;                // 0 never, 1 per step (2B < I), 2 always (env BPRX_LIST_MODE)
  int32_t *ilist;                 // [min(2*max_batch, I)] distinct items of the batch, in arrival order (k_row_count)
  int32_t *ilist_n;               // [2] their number, two cursors used by alternate list-mode steps: k_dense_update (the
                                  //     last kernel of a step) clears the cursor the NEXT list-mode step appends through
  int32_t *slist, *slist_n;       // sgd fast path: list of the batch's SHARED rows (kind << 30 | row), two alternating cursors
  int num_cu;                     // compute units of the device (balanced forward grid)
  int fwd_variant;                // 0: the plain forward kernel (env BPRX_FWD_VARIANT, read at create), else the per-shape policy
  int fold_cache;                 // env BPRX_FOLD_CACHE, read at create: 1 (default) bprx_fold_in / bprx_af_fold_in run their steps from LDS where a user's pairs fit
  float neg_bias_reg;             // factor of reg on the negative item's bias: 0.1 (VBPR.py:125), 1.0 for GradFashion
  // GradFashion (bprx_bind_factored, bprx_factored.hip): E / Bp of t are E_eff / Bp_eff, composed from the factors fx
  bool factored;
  bprx_factored fx;
  float *gF;                      // [Dc*ec + De*ee + (ec+ee)*(d+1)] gradient of the factors (Ea | Eb | A | Ap), one step
  // ACF (bprx_bind_acf, bprx_acf.hip): bound model state and scratch; nullptr unless the handle is bound ACF
  struct AcfState *acf;
  // AttentiveFashion (bprx_bind_attentive, bprx_attentive.hip): nullptr unless the handle is bound for it
  struct AfState *af;
  // replicated-user message exchange (bprx_pack_user_msg / bprx_apply_user_msgs)
  int32_t *msg_cursor;            // [2] next free slot of the message being packed, workgroups done (both zero between calls)
  int32_t *msg_next;              // [nranks*cap] chain links of the occurrences of one user across the ranks' messages
  size_t msg_next_n;
  // side stream (lazy adam_tf23 with VBPR, unless BPRX_SIDE_STREAM=0; else nullptr): the lazy-Adam catch-up runs on it beside
  // the forward projection; forked and joined by the two events within bprx_step_begin_sparse
  hipStream_t side;
  hipEvent_t ev_fork, ev_join;
  // per-kernel HIP-event timing (bprx_profile_*)
  bool prof;
  struct ProfRec { int phase; hipEvent_t a, b; };
  std::vector<ProfRec> prof_pending;
  std::vector<hipEvent_t> prof_free;
};

// RAII: records an event pair around one kernel launch when profiling is on.
struct BprxProfScope {
  bprx_handle *h; hipStream_t s; hipEvent_t a, b; int phase; bool on;
  BprxProfScope(bprx_handle *h_, int phase_, hipStream_t s_) : h(h_), s(s_), phase(phase_), on(h_->prof) {
    if (!on) return;
    auto get = [&]() { hipEvent_t e; if (!h->prof_free.empty()) { e = h->prof_free.back(); h->prof_free.pop_back(); }
                       else (void)hipEventCreate(&e); return e; };
    a = get(); b = get();
    (void)hipEventRecord(a, s);
  }
  ~BprxProfScope() {
    if (!on) return;
    (void)hipEventRecord(b, s);
    h->prof_pending.push_back({phase, a, b});
  }
};

#define BPRX_FAIL(h, code, ...)                                   \
  do {                                                            \
    snprintf((h)->err, sizeof((h)->err), __VA_ARGS__);            \
    return (code);                                                \
  } while (0)

#define BPRX_HIP(h, call)                                                                          \
  do {                                                                                             \
    hipError_t e__ = (call);                                                                       \
    if (e__ != hipSuccess) BPRX_FAIL(h, BPRX_E_HIP, "%s: %s", #call, hipGetErrorString(e__));      \
  } while (0)

#define BPRX_LAUNCH_CHECK(h, name)                                                                 \
  do {                                                                                             \
    hipError_t e__ = hipGetLastError();                                                            \
    if (e__ != hipSuccess) BPRX_FAIL(h, BPRX_E_HIP, "launch %s: %s", name, hipGetErrorString(e__)); \
  } while (0)

// The argument checks every fold-in entry point shares (`what`: the entry's name in the messages).
static inline int fold_check_args(bprx_handle *h, const char *what, int64_t n, int32_t steps, int32_t optimizer) {
  if (n < 0 || n >= ((int64_t)1 << 31)) BPRX_FAIL(h, BPRX_E_INVALID, "%s: n = %lld out of range", what, (long long)n);
  if (steps < 1) BPRX_FAIL(h, BPRX_E_INVALID, "%s: steps = %d < 1", what, steps);
  if (optimizer != BPRX_OPT_SGD && optimizer != BPRX_OPT_ADAM_TF23) BPRX_FAIL(h, BPRX_E_INVALID, "%s: optimizer %d", what, optimizer);
  return BPRX_OK;
}

// ---- launchers implemented in the kernel translation units ----
// sparse part (bprx_sparse.hip)
int bprx_launch_score(bprx_handle *h, const int32_t *u, const int32_t *i, int64_t B, const float *Prow,
                      int p_by_pair, float *x, hipStream_t s);
// the step's launchers read the plan of the step in flight (h->step) and decide nothing themselves
int bprx_launch_index_pass(bprx_handle *h, const StepPlan &p, hipStream_t s);
int bprx_launch_triplet_grad(bprx_handle *h, const StepPlan &p, hipStream_t s);
int bprx_launch_item_seg(bprx_handle *h, const StepPlan &p, hipStream_t s);
int bprx_launch_apply(bprx_handle *h, const StepPlan &p, hipStream_t s);
int bprx_launch_dense_update(bprx_handle *h, const StepPlan &p, hipStream_t s);
DenseArgs bprx_dense_args(bprx_handle *h, const StepPlan &p);               // what that launch is given (also sets dense_blocks)
int bprx_launch_dense_args(bprx_handle *h, const DenseArgs &a, hipStream_t s);
// Runs a pending dense update (and its lagging loss) with the stand-alone kernel on `s`; returns at once when nothing is pending
// or h is null.  Called by bprx_enter, the step path and bprx_settle only (bprx_api.hip).
int bprx_settle_pending(bprx_handle *h, hipStream_t s);
// One adam_tf23 step (sparse rule, adam_elem) of up to four whole tables from their staging gradients, which return to zero,
// and the clearing of up to two claim-mark arrays, in ONE launch of k_adam_sweep: the sweep of every model and of
// bprx_adam_rows.  A segment with n == 0 (a flag array with nflag == 0) costs nothing.
struct AdamSweepSeg { float *p, *m, *v, *g; size_t n; };
struct AdamSweepAll { AdamSweepSeg seg[4]; uint32_t *flag[2]; size_t nflag[2]; };
int bprx_launch_adam_sweep(bprx_handle *h, const AdamSweepAll &sw, float lr_t, hipStream_t s);
int bprx_launch_fill_i32(bprx_handle *h, int32_t *p, size_t n, int32_t v, hipStream_t s);
int bprx_launch_adam_catchup(bprx_handle *h, const StepPlan &p, hipStream_t s);
int bprx_launch_adam_sync(bprx_handle *h, int64_t t, hipStream_t s);
int bprx_launch_adam_reset(bprx_handle *h, int64_t t, hipStream_t s);
int bprx_launch_loss_reduce(bprx_handle *h, int64_t B, float *loss_out, hipStream_t s);
int bprx_launch_loss_reduce_at(bprx_handle *h, int64_t B, int nsq, float reg, float *loss_out, hipStream_t s);   // a lagging loss
// the user side of a block score: rows [u0, u1) of these tables (the handle's own Gu / Tu, or a caller's)
struct UserRows { const float *Gu, *Tu; };
// the item side: the catalogue (Gi == nullptr), or n caller-owned rows Gi [n, k] / Bi [n] / P [n, PS] (bprx_score_warm_block)
struct ItemRows { const float *Gi, *Bi, *P; int n; };
int bprx_launch_score_block(bprx_handle *h, int32_t u0, int32_t u1, float *out, hipStream_t s, UserRows rows, ItemRows items = {});
int bprx_launch_score_gemm(bprx_handle *h, int32_t u0, int32_t u1, float *out, hipStream_t s, UserRows rows);
// projection part (bprx_proj.hip)
int bprx_launch_tile_F(bprx_handle *h);
int bprx_launch_cast_Et(bprx_handle *h, hipStream_t s);
// rows == nullptr: items 0..nrows; else the listed items.  nrows_dev (device, optional): the actual row count (<= nrows, the
// host-side bound the grid is sized for).  scatter: row t of the result goes to Pout[rows[t]] instead of Pout[t].
// occ (device, optional; whole-table form only): occ[t] == 0 marks an item whose row this step does not need -- the forward
// projection then writes P[t] = 0 without reading its features, the backward one leaves it out of the sums (its W row must be
// all zeros).  nullptr: every row.
int bprx_launch_proj_fwd(bprx_handle *h, const int32_t *rows, int64_t nrows, const int32_t *nrows_dev, int scatter, float *Pout,
                         hipStream_t s, const int32_t *occ = nullptr);
int bprx_launch_proj_bwd(bprx_handle *h, const StepPlan &p, hipStream_t s);
// P = Fnew.[E|Bp] for the n rows of a caller's ROW-MAJOR table (bprx_project_rows): bf16 features from the image Et in one pass
// over the table (k_proj_new_bf16), fp32 features with the kernels of the catalogue
int bprx_launch_proj_new(bprx_handle *h, const void *Fnew, int64_t n, float *P, hipStream_t s);
// whether the kernel form the whole-table forward / backward projection takes for this handle's shape has a masked variant
// (bprx_proj.hip, next to the form tables): what the launchers do with `occ`, and what bprx_proj_mask_kind reports
bool bprx_proj_fwd_takes_mask(const bprx_handle &h);
bool bprx_proj_bwd_takes_mask(const bprx_handle &h);
// GradFashion factors (bprx_factored.hip)
int bprx_launch_fact_compose(bprx_handle *h, hipStream_t s);                // E_eff | Bp_eff from the factors
int bprx_launch_fact_update(bprx_handle *h, float lr_t, hipStream_t s);     // chain rule from dEp, optimizer, loss partials
int bprx_launch_explain(bprx_handle *h, const int32_t *u, const int32_t *i, int64_t n, float *out, hipStream_t s);
// ACF (bprx_acf.hip): what bprx_step / bprx_score_pairs / bprx_score_block do on a handle bound with bprx_bind_acf
int bprx_acf_step(bprx_handle *h, const int32_t *u, const int32_t *i, const int32_t *j, int64_t B, float *loss_out, hipStream_t s);
int bprx_acf_score_pairs(bprx_handle *h, const int32_t *u, const int32_t *i, int64_t B, float *x, hipStream_t s);
int bprx_acf_eval_profiles(bprx_handle *h, hipStream_t s);   // g'_u of every user (evaluation histories) into acf_eval_gu()
float *bprx_acf_eval_gu(bprx_handle *h);
// g'_r of rows [r0, r1) of a caller's table with the histories of a CSR indexed by row: *gp = where they are, [(r1 - r0), k]
int bprx_acf_row_profiles(bprx_handle *h, const float *Gu_rows, int64_t r0, int64_t r1, const int64_t *hist_ptr,
                          const int32_t *hist_items, float **gp, hipStream_t s);
void bprx_acf_invalidate(bprx_handle *h);                    // bound tables written from outside
void bprx_acf_free(bprx_handle *h);
// AttentiveFashion (bprx_attentive.hip): what bprx_step / bprx_score_pairs / bprx_score_block do on a handle bound with bprx_bind_attentive
int bprx_af_step(bprx_handle *h, const int32_t *u, const int32_t *i, const int32_t *j, int64_t B, float *loss_out, hipStream_t s);
int bprx_af_pairs(bprx_handle *h, const int32_t *u, const int32_t *i, int64_t n, float *x, float *alpha, hipStream_t s);
// Gu_rows: the user rows the block is scored for (nullptr: the handle's own Gu); [u0, u1) are rows of that table
int bprx_af_block(bprx_handle *h, int32_t u0, int32_t u1, float *out, float *alpha, hipStream_t s, const float *Gu_rows = nullptr);
void bprx_af_invalidate(bprx_handle *h);
void bprx_af_free(bprx_handle *h);
// The step loop of bprx_af_fold_in_items (k_fold_fit over AfItemRow, bprx_foldin.hip):
// work [pair_ptr[n], KW] holds [D_p (k) | dc_p | zeros] of every pair, Gi_rows [n, k] in / out, loss [n] or nullptr
int bprx_launch_af_fold_items(bprx_handle *h, const int64_t *pair_ptr, int64_t n, const float *work, int KW, int k, int steps, bool adam,
                              float lr, float reg, float *Gi_rows, float *loss, hipStream_t s);
// The item space of bprx_sim_* and bprx_diversify (bprx_eval.hip).  One part of z: n rows of `w` floats, row stride ld (w == 0:
// the part is absent); z = [g | p].
struct SimPart {
  const float *p;
  int w, ld;
};
// the checks every entry of an item space shares (space, query rows, fp8, handle kind), then the read gate
int bprx_sim_enter(bprx_handle *h, const char *what, int32_t space, const float *Pq, int64_t nq, hipStream_t s);
// the parts of z for the catalogue (Pq == nullptr) or the caller's projected rows
void bprx_sim_parts(const bprx_handle *h, int32_t space, const float *Pq, SimPart &g, SimPart &p);

// ---- the fp32 MFMA GEMM tile of the block scores (bprx_eval.hip) and of bprx_style_assign (bprx_styles.hip) ----
namespace bprx_gemm {

typedef __attribute__((ext_vector_type(16))) float f32x16;

constexpr int TM = 128, TN = 128, GKC = 16, GLD = GKC + 1;   // 17-float LDS rows: conflict-free column reads

// one K phase: acc += A[rows, 0:K] . B[cols, 0:K]^T   (A row stride lda, B row stride ldb)
__device__ __forceinline__ void gemm_phase(const float *__restrict__ A, int lda, int arow0, int arows,
                                           const float *__restrict__ Bm, int ldb, int brow0, int brows, int K,
                                           float (*As)[GLD], float (*Bs)[GLD], f32x16 (&acc)[2][2], int wr, int wc, int lane) {
  const int t = threadIdx.x;
  for (int k0 = 0; k0 < K; k0 += GKC) {
    __syncthreads();
    // 128 rows x 16 floats per operand: thread t -> row t/2, 8 floats at (t%2)*8
    {
      const int r = t >> 1, c0 = (t & 1) * 8;
#pragma unroll
      for (int x = 0; x < 8; ++x) {
        const int kk = k0 + c0 + x;
        As[r][c0 + x] = (r < arows && kk < K) ? A[(size_t)(arow0 + r) * lda + kk] : 0.f;
        Bs[r][c0 + x] = (r < brows && kk < K) ? Bm[(size_t)(brow0 + r) * ldb + kk] : 0.f;
      }
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < GKC; kk += 2) {
      const int kq = kk + (lane >> 5), rr = lane & 31;
      const float a0 = As[wr * 64 + rr][kq], a1 = As[wr * 64 + 32 + rr][kq];
      const float b0 = Bs[wc * 64 + rr][kq], b1 = Bs[wc * 64 + 32 + rr][kq];
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
    }
  }
}

}  // namespace bprx_gemm

// ---- host helpers ----
// Adam's bias-corrected step size at optimizer.iterations = it
static inline float bprx_adam_lr_at(const bprx_config &c, int64_t it) {
  const float t = (float)it;
  return c.lr * sqrtf(1.0f - powf(c.beta2, t)) / (1.0f - powf(c.beta1, t));
}
// ... at h->adam_t (the caller decides when adam_t advances)
static inline float bprx_adam_lr_t(const bprx_handle *h) { return bprx_adam_lr_at(h->cfg, h->adam_t); }
// workgroups for `work` items at `per_block` each: at least one, at most `cap`
static inline unsigned bprx_blocks(int64_t work, int64_t per_block, int64_t cap = INT32_MAX) {
  int64_t g = (work + per_block - 1) / per_block;
  if (g > cap) g = cap;
  return (unsigned)(g < 1 ? 1 : g);
}

// ---- how a step is planned ----
// The one place that decides what a BPRMF / VBPR step launches.  Pure: reads the configuration, the create-time policies and the
// carried state of `h`, makes no HIP call and writes nothing.  fused_reduce: the caller is bprx_step (no all-reduce between the
// backward projection and the dense update).  The pointers are compared (byte planes) and kept, never followed.
inline StepPlan plan_step(const bprx_handle &h, const int32_t *user, const int32_t *pos, const int32_t *neg, int64_t B,
                          bool fused_reduce = false) {
  StepPlan p = {};
  const bprx_config &c = h.cfg;
  const bool vb = c.model == BPRX_MODEL_VBPR, sgd = c.optimizer == BPRX_OPT_SGD, lazy = !sgd && h.adam_lazy;
  const bool exU = c.flags & BPRX_FLAG_EXPORT_USER_GRAD, exI = c.flags & BPRX_FLAG_EXPORT_ITEM_GRAD;
  const int64_t I = c.num_items;
  const bool bf = c.feat_dtype != BPRX_F_FP32;            // bf16 W image (bf16 and fp8 features)
  // A rank of a replicated-user multi-GPU step whose item shard holds no positive of this global batch: it contributes an
  // empty message and a zero dense gradient, but takes part in every collective and takes the same optimizer step as the
  // other replicas (bprx_pack_user_msg -> count 0, bprx_step_begin_dense -> dE|dBp = 0, bprx_apply_user_msgs, bprx_step_end).
  if (B == 0 && !exU && !exI) { p.error = PLAN_E_EMPTY; return p; }
  p.B = B;
  if (B) { p.user = user; p.pos = pos; p.neg = neg; }
  p.adam_t = h.adam_t;
  p.lr_t = c.lr;
  if (!sgd) {
    p.adam_t = h.adam_t + 1;
    p.lr_t = bprx_adam_lr_at(c, p.adam_t);
    // the ring holds lr_s of the last ADAM_HIST steps: before it would wrap, everything is caught up (amortised: one
    // sweep per ~8000 steps); then the rows of THIS batch are brought to step t-1 for the forward pass (the empty batch: a
    // zero-row catch-up that records lr_t of this step)
    p.adam_sync_first = lazy && p.adam_t - h.adam_synced >= ADAM_HIST - 2;
    p.catchup = lazy;
  }
  p.fused_reduce = fused_reduce && !h.factored;          // (GradFashion's chain rule reads the summed gradient from dEp)
  p.idx_kind = h.step.idx_kind;
  p.seg_cur = h.step.seg_cur; p.seg_lead_over = h.step.seg_lead_over;   // (as the last segment-mode step left them)
  p.slist_cur = h.slist_slot;
  p.SK_step = B ? h.SK : h.step.SK_step;                 // (no backward projection: the slabs are the last step's)
  p.leaves_w_dirty = h.W_dirty;
  // GradFashion: bprx_launch_fact_update has moved the factors, composed E_eff / Bp_eff and left the loss partials;
  // k_dense_update only does the step's housekeeping (nothing to do: no launch)
  p.dense_launch = vb && (!h.factored || c.feat_dtype == BPRX_F_BF16);
  p.settle_first = h.pend.on;                            // (until a k_index_seg launch turns up below)
  if (B == 0) return p;                                  // no list, no segments, no mask; the dense half zeroes dEp

  // list mode: both projections over the batch's distinct items only (needs the index pass BEFORE the forward projection)
  p.list_mode = vb && !h.proj_fresh && (h.list_policy == 2 || (h.list_policy == 1 && 2 * B < I));
  p.item_mode = !p.list_mode && (h.seg_policy == 2 || (h.seg_policy == 1 && 2 * B >= I));
  p.seg_users = p.item_mode && sgd && !exU;
  p.dense_launch = p.dense_launch || p.list_mode;
  // every item row of a segment-mode step is finished by k_item_seg, which gathers PRE-update user rows after k_triplet_grad:
  // the user side may therefore not be updated in place either (staging + k_apply_sgd)
  p.fast = p.item_mode ? 0 : h.fast_rows;
  p.fastU = p.fast && !exU;
  p.fastI = p.fast && !exI;
  // shared-row list: both sides on the exclusive-row fast path (sgd, atomic staging, no exported gradients)
  p.use_list = h.slist && p.fastU && p.fastI;
  p.row_count = !p.item_mode && (h.fast_rows || p.list_mode);
  // byte planes of this very batch, left by bprx_sample_*_h
  p.idx8 = h.idx8_ready(p.item_mode, pos, neg, B);
  // ... and its owner queues: the owners read their own records instead of scanning the planes (BPRX_INDEX_QUEUE, shift 8, 2B <= 2^24)
  p.idxq = h.idxq_ready(p.idx8, B);
  p.idxq_regions = p.idxq ? (int)h.idxq_n : 0;
  if (p.list_mode) {
    p.list_bound = 2 * B < I ? 2 * B : I;
    p.list_cur = h.ilist_n + h.list_slot; p.list_next = h.ilist_n + (h.list_slot ^ 1);
    p.list_reset_cnt = !(h.fast_rows && !exI);
    // few rows: fewer item splits (each split writes a D x PS fp32 slab that the dense update reads back)
    if (bf) { const int sk = (int)((p.list_bound + 127) / 128); p.SK_step = sk < 1 ? 1 : (sk > h.SK ? h.SK : sk); }
  }
  // the (ALU-bound) lazy-Adam catch-up runs on the side stream beside the (HBM-bound) forward projection
  p.catchup_aside = lazy && h.side && !h.proj_fresh && !p.list_mode && !h.p_valid;
  p.project = vb && !h.proj_fresh;
  p.fwd = p.project && !h.p_valid;
  // Segment mode: k_index_seg depends on the index arrays only, so it runs BEFORE the forward projection and both projections
  // skip the feature rows of the items this batch does not touch (seg_cnt[item] == 0: nobody reads that row of P in this step
  // and p_valid stays false; its W row is all zeros).  Everything the index pass writes -- the Wb rows it zeroes, cntU / ulist /
  // uslot_of, seg_rank / seg_cnt / seg_ptr, the chunk list and both cursor triples -- was last read by the previous step's
  // kernels (k_triplet_seg, k_item_seg, the backward projection) on this same stream: stream order is the only ordering there
  // is today and it still holds.  The side stream's catch-up touches none of these buffers (rows, slots, lastU / lastI, lr_hist).
  p.mask = p.project && !p.list_mode && p.item_mode && !h.p_valid &&
           (h.proj_mask == 2 ? bf : (h.proj_mask == 1 && c.feat_dtype == BPRX_F_BF16 && h.PS / 16 <= 9));
  p.index_first = p.list_mode || p.mask;
  // The dense update across two steps.  This step's own update may wait (bprx_step, which alone sums the slabs in the update:
  // fused_reduce) unless it has list housekeeping to do or GradFashion composes E / Bp elsewhere.  A pending one rides in this
  // step's k_index_seg launch, which then runs before k_cast_Et* and the forward projection whatever the mask says (they read
  // what the update writes; the index pass itself reads none of it).  No such launch: the stand-alone kernel first.
  p.defer_ok = h.dense_defer && p.dense_launch && p.fused_reduce && !p.list_mode && !h.factored;
  p.carry_dense = h.pend.on && p.item_mode;
  p.settle_first = h.pend.on && !p.carry_dense;
  p.index_first = p.index_first || p.carry_dense;
  if (p.item_mode) {
    // k_index_seg: one owner workgroup per CU, more when a range would not fit LDS; the byte planes fix 2^shift items per owner
    p.idx_kind = p.idx8 ? 2 : 1;
    int64_t nown = h.num_cu > 0 ? h.num_cu : 256;
    if (nown > 1024) nown = 1024;
    if ((I + nown - 1) / nown > IX_RMAX) nown = (I + IX_RMAX - 1) / IX_RMAX;
    if (nown > I) nown = I;
    p.ix_R = p.idx8 ? 1 << h.idx8_shift : (int)((I + nown - 1) / nown);
    p.ix_nown = (int)((I + p.ix_R - 1) / p.ix_R);
    p.seg_lead_over = p.ix_nown * (p.ix_R + IX_LPAD);
    p.seg_cur = h.seg_slot;
  }
  // W (fp32) must be all-zero before the triplet kernel.  bf16 features: k_cast_W re-zeroes it while converting and k_item_seg
  // re-zeroes the rows it folds in.  Dense form with fp32 features: W is consumed in place and cleared at the next step; list
  // mode returns its rows to zero itself (k_cast_W_rows) and only needs the memset after such a step
  p.leaves_w_dirty = vb && !p.list_mode && !bf;
  p.w_memset = p.leaves_w_dirty || (vb && h.W_dirty);
  // apply pass, row kinds [fk, ek): fk = 1 skips the user rows (exported to the caller, or finished by k_triplet_seg); ek = 1
  // skips the item rows (finished in place by k_item_seg, or exported: their owner takes their steps)
  p.ek = (p.item_mode || exI) ? 1 : 3;
  if (sgd) {
    p.fk = (exU || p.item_mode) ? 1 : 0;
    p.apply = p.seg_users ? APPLY_NONE : (p.use_list ? APPLY_SGD_LIST : APPLY_SGD);
  } else {
    p.fk = exU ? 1 : 0;                                  // replicated multi-GPU: users via bprx_apply_user_msgs
    p.apply = lazy ? APPLY_ADAM_LAZY : APPLY_ADAM_SWEEP;  // lazy: touched rows only, everything else is replayed later
  }
  return p;
}

// ---- what a sampler call leaves for the handle's next step (bprx_sample_*_h) ----
// This call fills triplets [batch_offset, batch_offset + B) of a batch of batch_size.  Moves the handle's tags (host fields only,
// no HIP call) and says where the call's planes and regions go.  The call with batch_offset 0 begins the batch; a later call
// that does not continue it drops the planes, one whose regions do not fit (more calls than the stride allows for) drops the
// queues alone.
struct SamplerFeed {
  bool planes, queues;
  long long pl_i, pl_j;           // plane positions, and the `occ` of a record, of the call's first positive / negative
  int sh;                         // idx8_shift
  int q0, qstride;                // first region of this call, regions per owner in qrange
};
inline SamplerFeed sampler_feed(bprx_handle *h, const int32_t *pos, const int32_t *neg, int64_t B, int64_t batch_offset,
                                int64_t batch_size) {
  SamplerFeed f = {};
  f.sh = 8;
  if (!h || !h->own8 || batch_size <= 0 || batch_size > h->cfg.max_batch || batch_offset < 0 || batch_offset + B > batch_size) return f;
  if (batch_offset == 0) {
    h->idx8_pos = pos; h->idx8_neg = neg; h->idx8_B = batch_size; h->idx8_n = 0;
    h->idxq_n = 0; h->idxq_trip = 0;
  } else if (h->idx8_n < 0 || h->idx8_B != batch_size || pos != h->idx8_pos + batch_offset || neg != h->idx8_neg + batch_offset) {
    h->idx8_n = -1;                                        // not a continuation of the batch begun at offset 0: no planes
    h->idxq_n = -1;
    return f;
  }
  h->idx8_n += B;
  f.planes = true;
  f.pl_i = batch_offset; f.pl_j = batch_size + batch_offset; f.sh = h->idx8_shift;
  const int64_t nreg = (B + IXQ_WG - 1) / IXQ_WG, cap = ixq_regions(h->cfg.max_batch);
  if (h->idxq_n >= 0 && h->idxq_trip == batch_offset && h->idxq_feeds(batch_size) && h->idxq_n + nreg <= cap) {
    f.queues = true;
    f.q0 = (int)h->idxq_n; f.qstride = (int)cap;
    h->idxq_n += nreg; h->idxq_trip += B;
  } else
    h->idxq_n = -1;
  return f;
}

// ---- how a read is planned ----
// What an entry point needs from the handle before it may read the bound tables, and the handles it takes.
enum : unsigned {
  NEED_BOUND = 1,                 // tables are bound
  NEED_ROWS = 2,                  // lazy Adam: every row is current at adam_t
  NEED_ET = 4,                    // VBPR: the [E|Bp]^T image matches E / Bp
  NEED_P_ALL = 8,                 // VBPR: P holds the projection of every item (makes the image current on the way)
};
constexpr const char *BPRX_NOT_BOUND = "%s: tables not bound (call bprx_bind_tables first)";   // (also the step path's message)
enum { KIND_ANY = 0, KIND_PLAIN, KIND_VBPR, KIND_VBPR_NO_FP8, KIND_FACTORED, KIND_AF, KIND_ACF };   // PLAIN: BPRMF / VBPR, not ACF /
                                                   // AttentiveFashion; AF: bound with bprx_bind_attentive; ACF: with bprx_bind_acf
struct ReadPlan {
  int error;                      // 0, or BPRX_E_STATE (not bound) / BPRX_E_INVALID (a handle of the wrong kind): nothing is launched
  const char *why;                // ... and its message, a format with one %s for the name of the entry
  bool settle, sync, cast_et;     // in launch order: bprx_settle_pending, bprx_launch_adam_sync to adam_t, bprx_launch_cast_Et,
  bool project;                   //    the forward projection of all items, after which p_valid = true
};
// The one place that decides what a call does to the carried state before its own launches; bprx_enter (bprx_api.hip) runs it.
// Pure, like plan_step.  ACF / AttentiveFashion handles are BPRMF handles without lazy Adam: beyond settle nothing applies to them.
inline ReadPlan plan_read(const bprx_handle &h, unsigned need, int kind) {
  ReadPlan p = {};
  const bool vb = h.cfg.model == BPRX_MODEL_VBPR, plain = !h.acf && !h.af;
  auto fail = [&p](int code, const char *why) { p.error = code; p.why = why; return p; };
  if ((need & NEED_BOUND) && !h.bound) return fail(BPRX_E_STATE, BPRX_NOT_BOUND);
  if (kind == KIND_PLAIN && !plain) return fail(BPRX_E_INVALID, "%s: needs a BPRMF or VBPR handle, not ACF or AttentiveFashion");
  if ((kind == KIND_VBPR || kind == KIND_VBPR_NO_FP8) && !(vb && plain))
    return fail(BPRX_E_INVALID, "%s: needs a VBPR handle (bprx_bind_tables or bprx_bind_factored)");
  if (kind == KIND_VBPR_NO_FP8 && h.cfg.feat_dtype == BPRX_F_FP8)
    return fail(BPRX_E_INVALID, "%s: fp8 features are not supported for new items (a new row may exceed the max-abs the codes "
                                "were scaled for and would saturate): fp32 or bf16");
  if (kind == KIND_FACTORED && !h.factored) return fail(BPRX_E_INVALID, "%s: the handle is not bound with bprx_bind_factored");
  if (kind == KIND_AF && !h.af) return fail(BPRX_E_INVALID, "%s: the handle is not bound with bprx_bind_attentive");
  if (kind == KIND_ACF && !h.acf) return fail(BPRX_E_INVALID, "%s: the handle is not bound with bprx_bind_acf");
  p.settle = h.pend.on;
  p.sync = (need & NEED_ROWS) && plain && h.adam_lazy && h.adam_synced < h.adam_t;
  p.project = (need & NEED_P_ALL) && plain && vb && !h.p_valid;
  p.cast_et = plain && vb && ((need & NEED_ET) || p.project);     // (the launcher returns at once when the image is current)
  return p;
}
// The executor of that plan and the gate of every entry point that takes a handle (bprx_api.hip).
int bprx_enter(bprx_handle *h, const char *what, unsigned need, int kind, hipStream_t s);
