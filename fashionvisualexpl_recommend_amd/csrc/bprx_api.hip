// bprx_api.hip -- host side of the C ABI (include/bprx.h): handle, scratch, step orchestration.
#include <math.h>
#include <stdlib.h>
#include <algorithm>
#include <new>

#include "bprx_internal.h"

static char g_create_err[512] = "";

extern "C" int bprx_abi_version(void) { return BPRX_ABI_VERSION; }

extern "C" const char *bprx_last_error(const bprx_handle *h) { return h ? h->err : g_create_err; }

extern "C" int64_t bprx_live_device_allocs(void) { return bprx_live_allocs.load(); }

// The library's environment switches (README "Environment switches"), all read here, once, by bprx_create.
static int env_int(const char *name, int fallback) {
  const char *e = getenv(name);
  return e ? atoi(e) : fallback;
}

extern "C" int bprx_create(const bprx_config *cfg, bprx_handle **out) {
#define CFAIL(code, ...)                                        \
  do {                                                          \
    snprintf(g_create_err, sizeof(g_create_err), __VA_ARGS__);  \
    return (code);                                              \
  } while (0)
  if (!cfg || !out) CFAIL(BPRX_E_INVALID, "bprx_create: null argument");
  *out = nullptr;
  if (cfg->abi_version != BPRX_ABI_VERSION)
    CFAIL(BPRX_E_INVALID, "bprx_create: abi_version %d, library is %d", cfg->abi_version, BPRX_ABI_VERSION);
  if (cfg->model != BPRX_MODEL_BPRMF && cfg->model != BPRX_MODEL_VBPR) CFAIL(BPRX_E_INVALID, "unknown model %d", cfg->model);
  if (cfg->optimizer != BPRX_OPT_SGD && cfg->optimizer != BPRX_OPT_ADAM_TF23)
    CFAIL(BPRX_E_INVALID, "unknown optimizer %d", cfg->optimizer);
  if (cfg->num_users <= 0 || cfg->num_items <= 0 || cfg->embed_k <= 0 || cfg->max_batch <= 0)
    CFAIL(BPRX_E_INVALID, "num_users, num_items, embed_k and max_batch must be positive");
  const bool vb = cfg->model == BPRX_MODEL_VBPR;
  if (vb) {
    if (cfg->embed_d <= 0 || cfg->feat_dim <= 0) CFAIL(BPRX_E_INVALID, "VBPR needs embed_d > 0 and feat_dim > 0");
    if (cfg->embed_d > 271) CFAIL(BPRX_E_INVALID, "embed_d %d > 271 unsupported", cfg->embed_d);
    if (cfg->feat_dtype != BPRX_F_FP32 && cfg->feat_dtype != BPRX_F_BF16 && cfg->feat_dtype != BPRX_F_FP8)
      CFAIL(BPRX_E_INVALID, "unknown feat_dtype");
    if (cfg->feat_dtype == BPRX_F_BF16 && cfg->feat_dim % 128 != 0)
      CFAIL(BPRX_E_INVALID, "bf16 features need feat_dim %% 128 == 0 (got %d)", cfg->feat_dim);
    if (cfg->feat_dtype == BPRX_F_FP8 && cfg->feat_dim % 256 != 0)
      CFAIL(BPRX_E_INVALID, "fp8 features need feat_dim %% 256 == 0 (got %d)", cfg->feat_dim);
    if (cfg->feat_dtype == BPRX_F_FP8 && !(cfg->feat_scale > 0.f)) CFAIL(BPRX_E_INVALID, "fp8 features need feat_scale > 0");
  }
  const bool exported = cfg->flags & (BPRX_FLAG_EXPORT_USER_GRAD | BPRX_FLAG_EXPORT_ITEM_GRAD);
  // adam_tf23: lazily exact (per-row replay on touch) or by whole-table sweeps -- the same arithmetic either way.  A row's replay
  // is a serial recurrence over the steps since its last touch: with ~20 positives per user that is 20 U / B steps of ~0.45 us
  // each, against a sweep that moves every row's (p, m, v) once per step.  Large batches (C2: 30 steps, 14 us, against a 96-us
  // sweep) want the replay; the reference's own defaults (batch 256: 1 562 steps = 700 us, against a 25-us sweep of its small
  // tables) want the sweeps: measured on the CLI, 20 000 x 10 000, an epoch of 1 562 steps takes 0.76 s lazily and 0.22 s with
  // sweeps (BPRMF 0.46 / 0.10).  BPRX_ADAM_LAZY=0 / 1 forces either; exported user gradients (multi-GPU) need the lazy form.
  bool adam_lazy = false;
  if (cfg->optimizer == BPRX_OPT_ADAM_TF23) {
    // (0.45 us per replayed step: k_adam_catchup on C2's tables takes 86 / 235 / 702 us at replay depths 122 / 488 / 1953 =
    //  batches of 16 384 / 4 096 / 1 024, where the sweeps take 81-88 us: measured crossover between 16 384 and 4 096)
    const double chain_us = 20.0 * (double)cfg->num_users / (double)cfg->max_batch * 0.45;
    const double sweep_us =
        ((double)cfg->num_users * (cfg->embed_k + (vb ? cfg->embed_d : 0)) + (double)cfg->num_items * (cfg->embed_k + 1)) * 24.0 / 4e6;
    adam_lazy = exported ? true : chain_us < sweep_us;
    if (cfg->flags & BPRX_FLAG_ADAM_SWEEP) adam_lazy = false;
    if (cfg->flags & BPRX_FLAG_ADAM_LAZY) adam_lazy = true;
    adam_lazy = env_int("BPRX_ADAM_LAZY", adam_lazy) != 0;
  }
  // exported gradients + adam_tf23: the handle takes the Adam steps of the rows it keeps; the exported side's owner applies its
  // rows' steps (bprx_apply_user_msgs, or bprx_adam_rows over its shard).  A rank may see an empty batch and must still move
  // every row it owns: the lazy form only (a sweep per step would have to run on ranks that launch nothing else).
  if (exported && cfg->optimizer != BPRX_OPT_SGD && !adam_lazy)
    CFAIL(BPRX_E_INVALID, "BPRX_FLAG_EXPORT_*_GRAD with adam_tf23 needs the lazy form (BPRX_ADAM_LAZY != 0)");
  if ((cfg->flags & BPRX_FLAG_EXPORT_ITEM_GRAD) && cfg->model != BPRX_MODEL_BPRMF)
    CFAIL(BPRX_E_INVALID, "BPRX_FLAG_EXPORT_ITEM_GRAD is for BPRMF (VBPR keeps its items and features local)");
  hipError_t e = hipSetDevice(cfg->device);
  if (e != hipSuccess) CFAIL(BPRX_E_HIP, "hipSetDevice(%d): %s", cfg->device, hipGetErrorString(e));

  bprx_handle *h = new (std::nothrow) bprx_handle();
  if (!h) CFAIL(BPRX_E_NOMEM, "out of host memory");
// the one failure exit once the handle exists: bprx_destroy frees whatever has been made so far
#define HFAIL(code, ...)         \
  do {                           \
    bprx_destroy(h);             \
    CFAIL(code, __VA_ARGS__);    \
  } while (0)
  h->cfg = *cfg;
  h->adam_lazy = adam_lazy;
  h->neg_bias_reg = 0.1f;                                  // VBPR.py:125 (BPRMF.py:111); GradFashion: bprx_bind_factored
  if (!vb) { h->cfg.embed_d = 0; h->cfg.feat_dim = 0; }
  const size_t U = cfg->num_users, I = cfg->num_items, k = cfg->embed_k, d = h->cfg.embed_d, D = h->cfg.feat_dim;
  const size_t MB = cfg->max_batch;
  hipDeviceProp_t prop;
  h->num_cu = hipGetDeviceProperties(&prop, cfg->device) == hipSuccess ? prop.multiProcessorCount : 256;
  // The pool stops at the first failure and is tested once, after the last allocation: until then the calls after a failure do
  // nothing, and nothing in between may use a buffer (sizes and policies only).
  DevPool &A = h->mem;
  A.zeros(&h->dGu, U * k);
  A.zeros(&h->dGi, I * k);
  A.zeros(&h->dBi, I);
  A.zeros(&h->flagU, U);
  A.zeros(&h->flagI, I);
  A.zeros(&h->lossb, MB);
  A.zeros(&h->loss_acc, (size_t)BPRX_DENSE_BLOCKS);
  A.zeros(&h->errflag, (size_t)1);
  if (cfg->flags & BPRX_FLAG_EXPORT_USER_GRAD) A.zeros(&h->msg_cursor, (size_t)2);
  A.zeros(&h->cntU, U);
  A.zeros(&h->cntI, I);
  if (vb) {
    h->PS = 16 * (int)((d + 1 + 15) / 16);
    const size_t PS = h->PS;
    // split-K of the backward projection: ONE 8-wave workgroup per CU over the D/256 column ranges (C2: 16 ranges x 16
    // item splits on 256 CUs).  More splits only add slab traffic (SK*D*PS*4 B written, then read by the dense update):
    // measured on C2 SK 16 / 32 with 3 / 2 tiles in flight: backward 73.8 / 77.0 us, dense update 9.7 / 12.1 us.
    const int mr = (int)((D + 255) / 256);
    h->SK = (h->num_cu + mr - 1) / mr;
    // fp8 tiles are half the bytes, wide projections (more than 9 column tiles) have no registers for a third tile in
    // flight: both keep two workgroups per CU with two tiles in flight (measured: c2fp8 53 vs 58 us, c5 124 vs 362 us)
    // (wide projections, re-measured with the 8-wave kernel at two tiles in flight -- c5: SK 16 / 24 / 32 = 120 / 154 / 127 us
    //  backward and 24 / 30 / 38 us dense update: one workgroup per CU there as well)
    if (cfg->feat_dtype == BPRX_F_FP8 && PS / 16 <= 9) h->SK *= 2;
    if (h->SK > 64) h->SK = 64;
    if (h->SK < 1) h->SK = 1;
    // BPRX_FWD_VARIANT=0: the plain forward kernel (the reference the streaming kernels are tested against); anything else:
    // the per-shape policy of bprx_proj.hip (launch_fwd_nt / launch_bwd_nt)
    h->fwd_variant = env_int("BPRX_FWD_VARIANT", 4);
    // BPRX_PROJ_MASK: the rows of items the batch does not touch are left out of both projections of a segment-mode step
    // (bprx_step_begin_sparse).  0 never (the form the masked passes are tested against); 1 (default) where it was measured to
    // pay: bf16 features, up to nine column tiles (C2 0.2091 -> 0.2064 ms/step, --zipf 1.0 0.2386 -> 0.2250; fp8 tables lose:
    // the masked backward pass is slower where the MFMAs pace it, c2fp8 49.3 -> 53.0 us, c5 944 -> 1 139 us, and a table that
    // sits in the Infinity Cache has no HBM bytes to save); 2 wherever a masked form exists
    h->proj_mask = std::min(std::max(env_int("BPRX_PROJ_MASK", 1), 0), 2);
    // BPRX_DENSE_DEFER: a bprx_step that is not asked for its loss leaves its dense E|Bp update to the next step's index pass
    // (k_index_seg hosts it on the CUs its owners leave idle).  0: the stand-alone kernel at the end of every step.
    h->dense_defer = env_int("BPRX_DENSE_DEFER", 1) != 0;
    A.zeros(&h->dTu, U * d);
    A.zeros(&h->P, I * PS);
    A.zeros(&h->W, I * PS);
    A.zeros((uint16_t **)&h->Wb, I * PS);
    A.zeros(&h->Ppair, MB * PS);
    A.zeros((uint16_t **)&h->Et, PS * D);
    A.zeros((uint16_t **)&h->EtF, PS * D);
    if (cfg->feat_dtype == BPRX_F_FP8 && PS / 16 >= 10) A.zeros((uint8_t **)&h->EtS, PS * D);
    A.zeros(&h->dEp, D * d + D);
    A.zeros(&h->part, (size_t)h->SK * D * PS);
    A.zeros(&h->qs, (size_t)4);
    if (cfg->feat_dtype != BPRX_F_FP32)   // tiled copy of F, item count padded to whole 32-item blocks
      A.zeros((uint8_t **)&h->Ft, (size_t)((I + 31) / 32 * 32) * D * (cfg->feat_dtype == BPRX_F_FP8 ? 1 : 2));
  }
  {
    // Item-side gradients through per-item occurrence segments (k_item_seg) instead of global float atomics: the
    // default whenever the row widths fit the 16-B-per-lane layout and the item rows are not staging rows of a sharded
    // run.  BPRX_ITEM_MODE=0 forces the atomic staging path (A/B measurements: profiles/r01_sweeps.md).
    const bool fits = k % 4 == 0 && d % 4 == 0 && k <= 256 && d <= 256;
    // seg_policy: 0 never, 1 per step (segments when the batch revisits items: 2B >= I; sparse batches keep the atomic
    // staging path with its in-place update of exclusive rows -- C3 shard: 0.104 vs 0.121 ms/step), 2 always
    h->seg_policy = (fits && !(cfg->flags & BPRX_FLAG_EXPORT_ITEM_GRAD)) ? std::min(std::max(env_int("BPRX_ITEM_MODE", 1), 0), 2) : 0;
    if (h->seg_policy) {
      // chunk list: the owners' regions (one slot per item + 4 per owner, <= 1024 owners; a last partial range) + the overflow list
      h->seg_lead_cap = (int64_t)(I + 8192 + 4 * 1024 + 2 * MB / 64 + 64 + 64);
      h->seg_ent_cap = (int64_t)(6 * MB + 64 * 1024 + 2048);
      // byte planes for the index pass (bprx_sample_*_h): at most 256 owners of 2^shift items
      h->idx8_shift = 0;
      for (int sh = 8; sh <= 13 && !h->idx8_shift; ++sh)
        if ((((int64_t)I - 1) >> sh) <= 255) h->idx8_shift = sh;
      A.zeros(&h->seg_rank, (size_t)2 * MB);
      A.zeros(&h->seg_cnt, I); A.zeros(&h->seg_ptr, I);
      A.zeros(&h->seg_cursor, (size_t)6);
      A.zeros((int4 **)&h->seg_lead, (size_t)h->seg_lead_cap);
      A.zeros(&h->hot_done, I);
      A.zeros((int2 **)&h->seg_ent, (size_t)h->seg_ent_cap);
      A.zeros(&h->uslot_of, U); A.zeros(&h->ulist, MB);
      A.zeros(&h->uold, MB * (k + d));
      // BPRX_INDEX_QUEUE: the samplers also leave their occurrences binned by owner and the owners of k_index_seg read their
      // own records instead of scanning the planes (DESIGN §4 "Owner queues"; byte locals only: up to 65 536 items).  0: the scan.
      // The queues live behind the owner plane, in its allocation: records, then ranges.
      h->index_queue = env_int("BPRX_INDEX_QUEUE", 1) != 0;
      const size_t nreg = (h->index_queue && h->idx8_shift == 8) ? (size_t)ixq_regions((int64_t)MB) : 0;
      const size_t plane = ((size_t)2 * MB + 15) / 16 * 16;
      if (h->idx8_shift) {
        A.zeros(&h->own8, plane + nreg * (IXQ_REC + IXQ_BINS) * sizeof(uint32_t));
        A.zeros(&h->loc8, (size_t)2 * MB * (h->idx8_shift > 8 ? 2 : 1));
      }
      if (nreg && h->own8) {
        h->qrec = reinterpret_cast<uint32_t *>(h->own8 + plane);
        h->qrange = h->qrec + nreg * IXQ_REC;
      }
    }
  }
  // Touched-item list (sparse batches): when the batch touches few of the items, both projections run over the batch's
  // distinct items only (the reference gathers 2B feature rows per step, VBPR.py:78; its own default is --batch_size 256,
  // train_rec.py:23) instead of streaming all of F twice.  Per step: list mode iff 2B < I, i.e. whenever the batch cannot touch every item (measured on C2's tables: B = 16 384 / 24 576:
  // 0.182 / 0.223 ms with the list, 0.231 / 0.239 ms streaming; B = 32 768 = 2B >= I: 0.287 vs 0.240 ms with occurrence segments);
  // BPRX_LIST_MODE = 0 never / 1 per step / 2 always.
  h->list_policy = vb ? std::min(std::max(env_int("BPRX_LIST_MODE", 1), 0), 2) : 0;
  // BPRX_FOLD_CACHE: bprx_fold_in keeps a user's pair differences in LDS across its steps where they fit (bprx_foldin.hip).
  // 0: every step gathers the item rows again (the form large users take anyway; the same bits).
  h->fold_cache = env_int("BPRX_FOLD_CACHE", 1) != 0;
  if (h->list_policy) {
    const size_t cap = 2 * MB < I ? 2 * MB : I;
    A.zeros(&h->ilist, cap); A.zeros(&h->ilist_n, (size_t)2);
  }
  h->step.SK_step = h->SK;
  if (h->adam_lazy) {
    A.zeros(&h->lastU, U); A.zeros(&h->lastI, I);
    A.zeros(&h->lr_hist, (size_t)ADAM_HIST);
  }
  // exclusive-row fast path: sgd only (adam sweeps every row anyway); not with exported user gradients
  h->fast_rows = (cfg->optimizer == BPRX_OPT_SGD && !(cfg->flags & BPRX_FLAG_EXPORT_USER_GRAD)) ? 1 : 0;   // per side: make_args
  if (h->fast_rows && !exported) {
    A.zeros(&h->slist, (size_t)3 * MB); A.zeros(&h->slist_n, (size_t)2);
  }
  if ((e = A.err) != hipSuccess) HFAIL(BPRX_E_NOMEM, "scratch allocation failed: %s", hipGetErrorString(e));
  // Side stream: lazy Adam's catch-up (ALU-bound: correctly rounded sqrt / divide per replayed element and step) runs beside the
  // HBM-bound forward projection of a streaming step: adam_tf23 0.330 -> 0.317 ms/step on C2.  BPRX_SIDE_STREAM=0: on the
  // step's own stream.  (Measured and removed, DESIGN §5.1: the sparse optimizer pass beside the backward projection, and the
  // segment-mode index pass beside the forward projection.)
  if (vb && cfg->optimizer == BPRX_OPT_ADAM_TF23 && h->adam_lazy && env_int("BPRX_SIDE_STREAM", 1) != 0 &&
      (hipStreamCreateWithFlags(&h->side, hipStreamNonBlocking) != hipSuccess ||
       hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming) != hipSuccess ||
       hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming) != hipSuccess))
    HFAIL(BPRX_E_HIP, "side stream / event creation failed");
  *out = h;
  return BPRX_OK;
#undef HFAIL
#undef CFAIL
}

extern "C" int bprx_destroy(bprx_handle *h) {
  if (!h) return BPRX_OK;
  (void)hipSetDevice(h->cfg.device);
  h->pend.on = false;                                      // a pending dense update is dropped: its tables are the caller's
  if (h->side) (void)hipStreamSynchronize(h->side);
  (void)h->mem.rollback(0);
  bprx_acf_free(h);
  bprx_af_free(h);
  if (h->side) (void)hipStreamDestroy(h->side);
  if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
  if (h->ev_join) (void)hipEventDestroy(h->ev_join);
  for (auto &r : h->prof_pending) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
  for (auto e : h->prof_free) (void)hipEventDestroy(e);
  delete h;
  return BPRX_OK;
}

extern "C" int bprx_profile_enable(bprx_handle *h, int on) {
  if (!h) return BPRX_E_INVALID;
  h->prof = on != 0;
  return BPRX_OK;
}

extern "C" int bprx_profile_read(bprx_handle *h, double *ms, int64_t *launches) {
  if (!h || !ms || !launches) return BPRX_E_INVALID;
  for (auto &r : h->prof_pending) {
    BPRX_HIP(h, hipEventSynchronize(r.b));
    float t = 0.f;
    BPRX_HIP(h, hipEventElapsedTime(&t, r.a, r.b));
    ms[r.phase] += (double)t;
    launches[r.phase] += 1;
    h->prof_free.push_back(r.a);
    h->prof_free.push_back(r.b);
  }
  h->prof_pending.clear();
  return BPRX_OK;
}

static int bind_tables(bprx_handle *h, const bprx_tables *t, bool factored) {
  if (!h || !t) return BPRX_E_INVALID;
  if (!t->Gu || !t->Gi || !t->Bi) BPRX_FAIL(h, BPRX_E_INVALID, "bind_tables: Gu, Gi, Bi are required");
  const bool vb = h->cfg.model == BPRX_MODEL_VBPR;
  if (vb && (!t->Tu || !t->F || !t->E || !t->Bp)) BPRX_FAIL(h, BPRX_E_INVALID, "bind_tables: VBPR needs Tu, F, E, Bp");
  if (h->cfg.optimizer == BPRX_OPT_ADAM_TF23) {
    if (!t->m_Gu || !t->v_Gu || !t->m_Gi || !t->v_Gi || !t->m_Bi || !t->v_Bi)
      BPRX_FAIL(h, BPRX_E_INVALID, "bind_tables: adam_tf23 needs m_/v_ slots for Gu, Gi, Bi");
    if (vb && (!t->m_Tu || !t->v_Tu || (!factored && (!t->m_E || !t->v_E || !t->m_Bp || !t->v_Bp))))
      BPRX_FAIL(h, BPRX_E_INVALID, "bind_tables: adam_tf23 needs m_/v_ slots for Tu, E, Bp");
  }
  if (((uintptr_t)t->Gu | (uintptr_t)t->Gi | (uintptr_t)t->Tu | (uintptr_t)t->F | (uintptr_t)t->E) & 15)
    BPRX_FAIL(h, BPRX_E_INVALID, "bind_tables: table base pointers must be 16-byte aligned");
  { const int rc = bprx_enter(h, "bind_tables", 0, KIND_ANY, nullptr); if (rc) return rc; }   // (the tables bound so far, the null stream)
  h->t = *t;
  h->factored = factored;
  if (!factored) h->neg_bias_reg = 0.1f;
  h->et_valid = h->p_valid = h->absmax_valid = false;
  {
    const int rc = bprx_launch_tile_F(h);   // the projections read a tiled copy of the frozen F (made here, once)
    if (rc) return rc;
  }
  h->bound = true;
  return bprx_launch_adam_reset(h, h->adam_t, 0);   // every bound row counts as current at optimizer.iterations
}

extern "C" int bprx_bind_tables(bprx_handle *h, const bprx_tables *t) {
  if (h && h->acf) bprx_acf_free(h);                        // a plain bind makes the handle a BPRMF / VBPR handle again
  if (h && h->af) bprx_af_free(h);
  return bind_tables(h, t, false);
}

// bprx_bind_acf (bprx_acf.hip) binds the BPRMF tables through here
int bprx_bind_tables_internal(bprx_handle *h, const bprx_tables *t) { return bind_tables(h, t, false); }

extern "C" int bprx_bind_factored(bprx_handle *h, const bprx_tables *t, const bprx_factored *f) {
  if (!h || !t || !f) return BPRX_E_INVALID;
  const bprx_config &c = h->cfg;
  if (c.model != BPRX_MODEL_VBPR) BPRX_FAIL(h, BPRX_E_INVALID, "bind_factored: needs a VBPR handle");
  if (c.feat_dtype == BPRX_F_FP8) BPRX_FAIL(h, BPRX_E_INVALID, "bind_factored: fp8 features are not supported (fp32 or bf16)");
  if (c.flags & (BPRX_FLAG_EXPORT_USER_GRAD | BPRX_FLAG_EXPORT_ITEM_GRAD))
    BPRX_FAIL(h, BPRX_E_INVALID, "bind_factored: exported gradients (multi-GPU) are not supported");
  if (f->feat_dim_a <= 0 || f->feat_dim_b <= 0 || (int64_t)f->feat_dim_a + f->feat_dim_b > c.feat_dim)
    BPRX_FAIL(h, BPRX_E_INVALID, "bind_factored: need Dc, De > 0 and Dc + De <= feat_dim (%d, %d, %d)", f->feat_dim_a,
              f->feat_dim_b, c.feat_dim);
  if (f->embed_a <= 0 || f->embed_b <= 0 || f->embed_a > 256 || f->embed_b > 256)
    BPRX_FAIL(h, BPRX_E_INVALID, "bind_factored: embed_a, embed_b must lie in [1, 256] (%d, %d)", f->embed_a, f->embed_b);
  if (!(f->neg_bias_reg >= 0.f)) BPRX_FAIL(h, BPRX_E_INVALID, "bind_factored: neg_bias_reg must be >= 0");
  if (!f->Ea || !f->Eb || !f->A || !f->Ap) BPRX_FAIL(h, BPRX_E_INVALID, "bind_factored: Ea, Eb, A, Ap are required");
  if (c.optimizer == BPRX_OPT_ADAM_TF23 &&
      (!f->m_Ea || !f->v_Ea || !f->m_Eb || !f->v_Eb || !f->m_A || !f->v_A || !f->m_Ap || !f->v_Ap))
    BPRX_FAIL(h, BPRX_E_INVALID, "bind_factored: adam_tf23 needs m_/v_ slots for Ea, Eb, A, Ap");
  if (!h->gF) {
    const size_t n = (size_t)f->feat_dim_a * f->embed_a + (size_t)f->feat_dim_b * f->embed_b +
                     (size_t)(f->embed_a + f->embed_b) * (c.embed_d + 1);
    const hipError_t e = h->mem.regrow(&h->gF, n);
    if (e != hipSuccess) BPRX_FAIL(h, BPRX_E_HIP, "bind_factored: factor gradient (%zu floats): %s", n, hipGetErrorString(e));
  } else if (f->feat_dim_a != h->fx.feat_dim_a || f->feat_dim_b != h->fx.feat_dim_b || f->embed_a != h->fx.embed_a ||
             f->embed_b != h->fx.embed_b) {
    BPRX_FAIL(h, BPRX_E_INVALID, "bind_factored: the factor shapes of a handle cannot change");
  }
  int rc = bind_tables(h, t, true);
  if (rc) return rc;
  h->fx = *f;
  h->neg_bias_reg = f->neg_bias_reg;
  if ((rc = bprx_launch_fact_compose(h, nullptr))) return rc;
  BPRX_HIP(h, hipStreamSynchronize(nullptr));
  return BPRX_OK;
}

extern "C" int bprx_explain_pairs(bprx_handle *h, const int32_t *user, const int32_t *item, int64_t n, float *out, void *stream) {
  if (!h) return BPRX_E_INVALID;
  if (n < 0 || n > ((int64_t)1 << 32)) BPRX_FAIL(h, BPRX_E_INVALID, "explain_pairs: n = %lld out of range", (long long)n);
  if (n && (!user || !item || !out)) BPRX_FAIL(h, BPRX_E_INVALID, "explain_pairs: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const int rc = bprx_enter(h, "explain_pairs", NEED_BOUND | NEED_ROWS, KIND_FACTORED, s);
  if (rc || n == 0) return rc;
  return bprx_launch_explain(h, user, item, n, out, s);
}

extern "C" int bprx_tables_dirty(bprx_handle *h, void *stream) {
  { const int rc = bprx_enter(h, "tables_dirty", 0, KIND_ANY, (hipStream_t)stream); if (rc) return rc; }
  h->et_valid = h->p_valid = h->absmax_valid = false;
  if (h->acf) bprx_acf_invalidate(h);                      // ACF: the evaluation profiles follow the tables
  if (h->af) bprx_af_invalidate(h);                        // AttentiveFashion: so do the item encodings
  if (h->bound && h->factored) {                           // the factors were written: E_eff / Bp_eff follow them
    const int rc = bprx_launch_fact_compose(h, (hipStream_t)stream);
    if (rc) return rc;
  }
  // outside values are current by definition; the bookkeeping reset is ordered on the caller's stream, behind whatever
  // wrote the tables there (a NULL stream is synchronised instead)
  return h->bound ? bprx_launch_adam_reset(h, h->adam_t, (hipStream_t)stream) : BPRX_OK;
}

extern "C" int bprx_set_hyper(bprx_handle *h, float lr, float reg) {
  if (!h) return BPRX_E_INVALID;
  h->cfg.lr = lr;
  h->cfg.reg = reg;
  return BPRX_OK;
}

extern "C" int bprx_set_adam_step(bprx_handle *h, int64_t it, void *stream) {
  if (it < 0) return BPRX_E_INVALID;
  { const int rc = bprx_enter(h, "set_adam_step", 0, KIND_ANY, (hipStream_t)stream); if (rc) return rc; }
  h->adam_t = it;
  return h->bound ? bprx_launch_adam_reset(h, it, (hipStream_t)stream) : BPRX_OK;
}

extern "C" int64_t bprx_get_adam_step(const bprx_handle *h) { return h ? h->adam_t : -1; }
extern "C" int bprx_adam_is_lazy(const bprx_handle *h) { return h ? (h->adam_lazy ? 1 : 0) : BPRX_E_INVALID; }

// the preamble of a step, which stays outside the read gate: plan_step carries or settles a pending update
static int check_step(bprx_handle *h, int64_t B) {
  if (!h) return BPRX_E_INVALID;
  if (!h->bound) BPRX_FAIL(h, BPRX_E_STATE, BPRX_NOT_BOUND, "step");
  if (B < 0 || B > h->cfg.max_batch) BPRX_FAIL(h, BPRX_E_INVALID, "B=%lld outside [0, max_batch=%lld]", (long long)B, (long long)h->cfg.max_batch);
  return BPRX_OK;
}

// A deferred dense update runs now, on the stream of the call that needs it, and its lagging loss behind it.
int bprx_settle_pending(bprx_handle *h, hipStream_t s) {
  if (!h || !h->pend.on) return BPRX_OK;
  const DensePending q = h->pend;
  h->pend.on = false;
  int rc = bprx_launch_dense_args(h, q.a, s);
  if (!rc && q.loss_out) rc = bprx_launch_loss_reduce_at(h, q.loss_B, q.loss_nsq, q.loss_reg, q.loss_out, s);
  return rc;
}

// The gate of every entry point that takes a handle: what plan_read decides, run in its order on `s`.  An entry validates its
// arguments, enters, returns if there is no work, then launches.  Outside the gate: bprx_step and the split-phase begin (check_step:
// they may carry the update), the samplers, the profile calls, bprx_last_error, bprx_set_hyper / bprx_set_loss_lag, the pure
// getters and bprx_settle / bprx_dense_pending.
int bprx_enter(bprx_handle *h, const char *what, unsigned need, int kind, hipStream_t s) {
  if (!h) return BPRX_E_INVALID;
  const ReadPlan p = plan_read(*h, need, kind);
  if (p.error) BPRX_FAIL(h, p.error, p.why, what);
  int rc;
  if (p.settle && (rc = bprx_settle_pending(h, s))) return rc;
  if (p.sync && (rc = bprx_launch_adam_sync(h, h->adam_t, s))) return rc;
  if (p.cast_et && (rc = bprx_launch_cast_Et(h, s))) return rc;
  if (p.project) {                                         // P = F.[E|Bp] once per parameter state
    if ((rc = bprx_launch_proj_fwd(h, nullptr, h->cfg.num_items, nullptr, 0, h->P, s))) return rc;
    h->p_valid = true;
  }
  return BPRX_OK;
}

extern "C" int bprx_settle(bprx_handle *h, void *stream) {
  if (!h) return BPRX_E_INVALID;
  return bprx_settle_pending(h, (hipStream_t)stream);
}

extern "C" int bprx_dense_pending(const bprx_handle *h) { return h ? (h->pend.on ? 1 : 0) : BPRX_E_INVALID; }

extern "C" int bprx_set_loss_lag(bprx_handle *h, int on) {
  if (!h) return BPRX_E_INVALID;
  h->loss_lag = on != 0;
  return BPRX_OK;
}

extern "C" int bprx_sync_adam(bprx_handle *h, void *stream) {
  return bprx_enter(h, "sync_adam", NEED_BOUND | NEED_ROWS, KIND_ANY, (hipStream_t)stream);
}

extern "C" int bprx_score_pairs(bprx_handle *h, const int32_t *user, const int32_t *item, int64_t B, float *x, void *stream) {
  if (!h) return BPRX_E_INVALID;
  if (B < 0 || B > h->cfg.max_batch) BPRX_FAIL(h, BPRX_E_INVALID, "B=%lld outside [0, max_batch=%lld]", (long long)B, (long long)h->cfg.max_batch);
  int rc;
  if (B && (!user || !item || !x)) BPRX_FAIL(h, BPRX_E_INVALID, "score_pairs: null pointer");
  hipStream_t s = (hipStream_t)stream;
  // every item's projection is at hand (p_valid), or one projection row per pair is made from the image
  rc = bprx_enter(h, "score_pairs", NEED_BOUND | NEED_ROWS | (h->p_valid ? 0 : NEED_ET), KIND_ANY, s);
  if (rc || B == 0) return rc;
  if (h->acf) return bprx_acf_score_pairs(h, user, item, B, x, s);
  if (h->af) return bprx_af_pairs(h, user, item, B, x, nullptr, s);
  if (h->cfg.model != BPRX_MODEL_VBPR || h->p_valid) return bprx_launch_score(h, user, item, B, nullptr, 0, x, s);
  if ((rc = bprx_launch_proj_fwd(h, item, B, nullptr, 0, h->Ppair, s))) return rc;
  return bprx_launch_score(h, user, item, B, h->Ppair, 1, x, s);
}

// A planned step becomes the step in flight: the only place that moves the carried state at the start of a step.
static void commit_plan(bprx_handle *h, const StepPlan &p) {
  h->step = p;
  h->step_stage = 1;
  h->adam_t = p.adam_t;
  if (p.B == 0) return;
  h->idx8_n = 0;                                           // the byte planes are consumed, whatever this step does with them
  h->idxq_n = 0; h->idxq_trip = 0;                         // ... and the owner queues with them
  h->proj_fresh = false;
  h->W_dirty = p.leaves_w_dirty;
  if (p.item_mode) h->seg_slot ^= 1;                       // (k_index_seg clears the other cursor triple for the next such step)
  if (p.use_list) h->slist_slot ^= 1;                      // (k_apply_sgd_list likewise)
}

// the launches of bprx_step_begin_sparse, in order
static int launch_sparse_half(bprx_handle *h, const StepPlan &p, hipStream_t s) {
  int rc;
  if (p.adam_sync_first && (rc = bprx_launch_adam_sync(h, p.adam_t - 1, s))) return rc;
  if (p.catchup_aside) {                                 // work that does not depend on P, beside the projection
    BPRX_HIP(h, hipEventRecord(h->ev_fork, s));
    BPRX_HIP(h, hipStreamWaitEvent(h->side, h->ev_fork, 0));
    if ((rc = bprx_launch_adam_catchup(h, p, h->side))) return rc;
    BPRX_HIP(h, hipEventRecord(h->ev_join, h->side));
  } else if (p.catchup && (rc = bprx_launch_adam_catchup(h, p, s))) return rc;
  if (p.project && p.list_mode && (rc = bprx_launch_cast_Et(h, s))) return rc;
  if (p.index_first && (rc = bprx_launch_index_pass(h, p, s))) return rc;      // list: counts + the distinct-item list
  if (p.carry_dense) {                                   // the pending update ran in that launch; its lagging loss right behind it,
    const DensePending q = h->pend;                      // before k_triplet_seg rewrites lossb
    h->pend.on = false;
    if (q.loss_out && (rc = bprx_launch_loss_reduce_at(h, q.loss_B, q.loss_nsq, q.loss_reg, q.loss_out, s))) return rc;
  }
  if (p.project && !p.list_mode && (rc = bprx_launch_cast_Et(h, s))) return rc;
  if (p.fwd) {                                           // P rows of the listed items only / of every (touched) item
    rc = p.list_mode ? bprx_launch_proj_fwd(h, h->ilist, p.list_bound, p.list_cur, 1, h->P, s)
                     : bprx_launch_proj_fwd(h, nullptr, h->cfg.num_items, nullptr, 0, h->P, s, p.mask ? h->seg_cnt : nullptr);
    if (rc) return rc;
  }
  if (p.catchup_aside) BPRX_HIP(h, hipStreamWaitEvent(s, h->ev_join, 0));
  if (p.B == 0) return BPRX_OK;
  if (!p.index_first && (rc = bprx_launch_index_pass(h, p, s))) return rc;
  return bprx_launch_triplet_grad(h, p, s);
}

// First half of bprx_step_begin: index pass, item projections, per-triplet gradients.  Afterwards the USER-side gradients
// of the batch are final (staging tables with BPRX_FLAG_EXPORT_USER_GRAD): a replicated-user step packs and all-gathers
// them while bprx_step_begin_dense (item rows, W, dE|dBp = F^T W) is still running.
static int step_begin_sparse(bprx_handle *h, const int32_t *user, const int32_t *pos, const int32_t *neg, int64_t B, bool fused_reduce,
                             hipStream_t s) {
  int rc = check_step(h, B);
  if (rc) return rc;
  if (h->step_stage) BPRX_FAIL(h, BPRX_E_STATE, "step_begin called twice without step_end");
  if (h->acf) BPRX_FAIL(h, BPRX_E_STATE, "step_begin: an ACF handle takes whole steps only (bprx_step)");
  if (h->af) BPRX_FAIL(h, BPRX_E_STATE, "step_begin: an AttentiveFashion handle takes whole steps only (bprx_step)");
  if (B && (!user || !pos || !neg)) BPRX_FAIL(h, BPRX_E_INVALID, "step: null index pointer");
  const StepPlan plan = plan_step(*h, user, pos, neg, B, fused_reduce);
  if (plan.error == PLAN_E_EMPTY) BPRX_FAIL(h, BPRX_E_INVALID, "step: empty batch");
  if (plan.settle_first && (rc = bprx_settle_pending(h, s))) return rc;
  commit_plan(h, plan);
  rc = launch_sparse_half(h, h->step, s);
  if (rc) h->step_stage = 0;                               // a failed _begin leaves no step pending
  return rc;
}

extern "C" int bprx_step_begin_sparse(bprx_handle *h, const int32_t *user, const int32_t *pos, const int32_t *neg, int64_t B, void *stream) {
  const int rc = bprx_settle_pending(h, (hipStream_t)stream);          // the split-phase calls neither defer nor carry
  return rc ? rc : step_begin_sparse(h, user, pos, neg, B, false, (hipStream_t)stream);
}

extern "C" int bprx_step_begin_dense(bprx_handle *h, void *stream) {
  if (!h) return BPRX_E_INVALID;
  if (h->step_stage != 1) BPRX_FAIL(h, BPRX_E_STATE, "step_begin_dense without step_begin_sparse");
  hipStream_t s = (hipStream_t)stream;
  const StepPlan &p = h->step;
  const bool vb = h->cfg.model == BPRX_MODEL_VBPR;
  int rc;
  if (p.B == 0) {                                          // empty batch of a replicated-user rank: zero dense gradient
    if (vb) BPRX_HIP(h, hipMemsetAsync(h->dEp, 0, ((size_t)h->cfg.feat_dim * (h->cfg.embed_d + 1)) * sizeof(float), s));
  } else {
    if (p.item_mode && (rc = bprx_launch_item_seg(h, p, s))) return rc;                 // item rows + W, no float atomics
    if (vb && (rc = bprx_launch_proj_bwd(h, p, s))) return rc;                           // dE|dBp = F^T W
    if (p.apply != APPLY_NONE && (rc = bprx_launch_apply(h, p, s))) return rc;
  }
  h->step_stage = 2;
  return BPRX_OK;
}

static int step_begin(bprx_handle *h, const int32_t *user, const int32_t *pos, const int32_t *neg, int64_t B, bool fused_reduce,
                      void *stream) {
  int rc = step_begin_sparse(h, user, pos, neg, B, fused_reduce, (hipStream_t)stream);
  if (!rc && (rc = bprx_step_begin_dense(h, stream))) h->step_stage = 0;   // a failed _begin leaves no step pending
  return rc;
}

extern "C" int bprx_step_begin(bprx_handle *h, const int32_t *user, const int32_t *pos, const int32_t *neg, int64_t B, void *stream) {
  const int rc = bprx_settle_pending(h, (hipStream_t)stream);
  return rc ? rc : step_begin(h, user, pos, neg, B, false, stream);
}

extern "C" int bprx_step_project(bprx_handle *h, void *stream) {
  const int rc = bprx_enter(h, "step_project", NEED_BOUND | NEED_ET | NEED_P_ALL, KIND_ANY, (hipStream_t)stream);
  if (!rc && h->cfg.model == BPRX_MODEL_VBPR) h->proj_fresh = true;
  return rc;
}

// The hard samplers' snapshot (bprx_philox.hip): Ps = F.[E|Bp] of every item from the tables as they are now, straight into the
// caller's buffer.  Not NEED_P_ALL plus a copy of h->P: that would mark P current (p_valid) and so change the plan of the next
// step (no masked projection, no catch-up beside it), and it would cost a second pass over I * PS floats.
extern "C" int bprx_hard_snapshot(bprx_handle *h, float *Ps, void *stream) {
  if (!h) return BPRX_E_INVALID;
  hipStream_t s = (hipStream_t)stream;
  const bool vb = h->cfg.model == BPRX_MODEL_VBPR && !h->acf && !h->af;
  if (vb && h->bound && !Ps) BPRX_FAIL(h, BPRX_E_INVALID, "hard_snapshot: a VBPR handle needs a buffer [num_items, proj_stride]");
  const int rc = bprx_enter(h, "hard_snapshot", NEED_BOUND | (vb ? NEED_ET : 0), KIND_PLAIN, s);
  if (rc || !vb) return rc;
  return bprx_launch_proj_fwd(h, nullptr, h->cfg.num_items, nullptr, 0, Ps, s);
}

extern "C" int bprx_user_grad(bprx_handle *h, float **dGu, float **dTu) {
  if (!h || !dGu || !dTu) return BPRX_E_INVALID;
  *dGu = h->dGu;
  *dTu = h->dTu;
  return BPRX_OK;
}

extern "C" int bprx_clear_user_grad(bprx_handle *h, int64_t n_rows, int32_t marks_only, void *stream) {
  if (!h || n_rows < 0 || n_rows > h->cfg.num_users) return BPRX_E_INVALID;
  hipStream_t s = (hipStream_t)stream;
  { const int rc = bprx_enter(h, "clear_user_grad", 0, KIND_ANY, s); if (rc) return rc; }
  if (!marks_only) {                                       // (bprx_route_pack has already returned the gradient rows to zero)
    BPRX_HIP(h, hipMemsetAsync(h->dGu, 0, (size_t)n_rows * h->cfg.embed_k * sizeof(float), s));
    if (h->cfg.embed_d) BPRX_HIP(h, hipMemsetAsync(h->dTu, 0, (size_t)n_rows * h->cfg.embed_d * sizeof(float), s));
  }
  BPRX_HIP(h, hipMemsetAsync(h->flagU, 0, (size_t)n_rows * sizeof(uint32_t), s));
  return BPRX_OK;
}

extern "C" int bprx_item_grad(bprx_handle *h, float **dGi, float **dBi) {
  if (!h || !dGi || !dBi) return BPRX_E_INVALID;
  *dGi = h->dGi;
  *dBi = h->dBi;
  return BPRX_OK;
}

extern "C" int bprx_clear_item_grad(bprx_handle *h, int64_t n_rows, int32_t marks_only, void *stream) {
  if (!h || n_rows < 0 || n_rows > h->cfg.num_items) return BPRX_E_INVALID;
  hipStream_t s = (hipStream_t)stream;
  { const int rc = bprx_enter(h, "clear_item_grad", 0, KIND_ANY, s); if (rc) return rc; }
  if (!marks_only) {
    BPRX_HIP(h, hipMemsetAsync(h->dGi, 0, (size_t)n_rows * h->cfg.embed_k * sizeof(float), s));
    BPRX_HIP(h, hipMemsetAsync(h->dBi, 0, (size_t)n_rows * sizeof(float), s));
  }
  BPRX_HIP(h, hipMemsetAsync(h->flagI, 0, (size_t)n_rows * sizeof(uint32_t), s));
  return BPRX_OK;
}

extern "C" int bprx_dense_grad(bprx_handle *h, float **ptr, int64_t *count) {
  if (!h || !ptr || !count) return BPRX_E_INVALID;
  *ptr = h->dEp;
  *count = h->cfg.model == BPRX_MODEL_VBPR ? (int64_t)h->cfg.feat_dim * (h->cfg.embed_d + 1) : 0;
  return BPRX_OK;
}

extern "C" int bprx_item_proj(bprx_handle *h, float **ptr, int64_t *count) {
  if (!h || !ptr || !count) return BPRX_E_INVALID;
  *ptr = h->P;
  *count = h->cfg.model == BPRX_MODEL_VBPR ? (int64_t)h->cfg.num_items * h->PS : 0;
  return BPRX_OK;
}

// may_defer: the caller is bprx_step -- the dense update may be left to the next step's index pass (StepPlan::defer_ok)
static int step_end(bprx_handle *h, float *loss_out, void *stream, bool may_defer) {
  if (!h) return BPRX_E_INVALID;
  if (!h->step_stage) BPRX_FAIL(h, BPRX_E_STATE, "step_end without step_begin");
  if (h->step_stage != 2) BPRX_FAIL(h, BPRX_E_STATE, "step_end before step_begin_dense");
  hipStream_t s = (hipStream_t)stream;
  const StepPlan &p = h->step;
  int rc;
  h->step_stage = 0;
  if (h->factored && (rc = bprx_launch_fact_update(h, p.lr_t, s))) return rc;   // the factors, then E_eff / Bp_eff
  // a step asked for its loss keeps today's sequence unless the caller allowed the loss to lag (bprx_set_loss_lag)
  const bool defer = may_defer && p.dense_launch && p.defer_ok && (!loss_out || h->loss_lag);
  if (defer) {                                             // recorded with what the launch would be given now; the carried flags
    h->pend.a = bprx_dense_args(h, p);                     // below are set as if it had run
    h->pend.loss_out = loss_out; h->pend.loss_B = p.B; h->pend.loss_nsq = h->dense_blocks; h->pend.loss_reg = h->cfg.reg;
    h->pend.on = true;
  } else if (p.dense_launch && (rc = bprx_launch_dense_update(h, p, s))) return rc;
  if (h->cfg.model == BPRX_MODEL_VBPR) {                    // what the end of a step leaves for the next one
    if (p.dense_launch) h->absmax_valid = h->cfg.feat_dtype == BPRX_F_FP8;   // k_dense_update left max|E,Bp| in qs[2 + qs_slot]
    if (p.list_mode) h->list_slot ^= 1;                     // the step's list is consumed
    h->et_valid = p.dense_launch && h->cfg.feat_dtype == BPRX_F_BF16;   // E / Bp moved: the images were refreshed, or are stale
    h->p_valid = false;                                     //               the item projections are stale
  }
  if (loss_out && !defer && (rc = bprx_launch_loss_reduce(h, p.B, loss_out, s))) return rc;
  return BPRX_OK;
}

extern "C" int bprx_step_end(bprx_handle *h, float *loss_out, void *stream) { return step_end(h, loss_out, stream, false); }

extern "C" int bprx_step(bprx_handle *h, const int32_t *user, const int32_t *pos, const int32_t *neg, int64_t B,
                         float *loss_out, void *stream) {
  if (!h) return BPRX_E_INVALID;
  if (h->acf || h->af) {                                     // ACF, AttentiveFashion: their own launch sequences
    const int rc = check_step(h, B);
    if (rc) return rc;
    return h->acf ? bprx_acf_step(h, user, pos, neg, B, loss_out, (hipStream_t)stream)
                  : bprx_af_step(h, user, pos, neg, B, loss_out, (hipStream_t)stream);
  }
  // no all-reduce in between: the dense update may sum the split-K slabs itself (StepPlan::fused_reduce)
  int rc = step_begin(h, user, pos, neg, B, true, stream);
  if (!rc) rc = step_end(h, loss_out, stream, true);
  return rc;
}

// rows [u0, u1) of the given user tables against every item: the fp32 MFMA GEMM (K step 2) where the widths allow it
static int score_rows(bprx_handle *h, int32_t u0, int32_t u1, float *out, hipStream_t s, UserRows rows) {
  return (h->cfg.embed_k % 2 == 0 && h->cfg.embed_d % 2 == 0) ? bprx_launch_score_gemm(h, u0, u1, out, s, rows)
                                                            : bprx_launch_score_block(h, u0, u1, out, s, rows);
}

extern "C" int bprx_score_block(bprx_handle *h, int32_t u0, int32_t u1, float *out, void *stream) {
  if (!h) return BPRX_E_INVALID;
  if (u0 < 0 || u1 > h->cfg.num_users || u0 > u1 || !out) BPRX_FAIL(h, BPRX_E_INVALID, "score_block: bad user range [%d,%d)", u0, u1);
  hipStream_t s = (hipStream_t)stream;
  int rc = bprx_enter(h, "score_block", NEED_BOUND | NEED_ROWS | NEED_P_ALL, KIND_ANY, s);
  if (rc || u0 == u1) return rc;
  if (h->af) return bprx_af_block(h, u0, u1, out, nullptr, s);
  if (h->acf) {
    // ACF.py:216-227: Gu' (evaluation histories) once per parameter state, then the BPRMF scoring kernels with Gu' in place of
    // Gu (Bi is zero: Bi + Gu'.Gi is the reference's Gu' Gi^T exactly)
    if ((rc = bprx_acf_eval_profiles(h, s))) return rc;
    return score_rows(h, u0, u1, out, s, {bprx_acf_eval_gu(h), h->t.Tu});
  }
  return score_rows(h, u0, u1, out, s, {h->t.Gu, h->t.Tu});
}

// bprx_score_block for caller-owned user rows (users folded in by bprx_fold_in): the same kernels, given the caller's rows.
extern "C" int bprx_score_rows_block(bprx_handle *h, const float *Gu_rows, const float *Tu_rows, int64_t n_rows, int64_t r0, int64_t r1,
                                     float *out, void *stream) {
  if (!h) return BPRX_E_INVALID;
  if (n_rows < 0 || n_rows >= ((int64_t)1 << 31) || r0 < 0 || r1 > n_rows || r0 > r1)
    BPRX_FAIL(h, BPRX_E_INVALID, "score_rows_block: bad row range [%lld,%lld) of %lld", (long long)r0, (long long)r1, (long long)n_rows);
  if (r0 != r1 && (!Gu_rows || !out || (h->cfg.embed_d > 0) != (Tu_rows != nullptr)))
    BPRX_FAIL(h, BPRX_E_INVALID, "score_rows_block: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const int rc = bprx_enter(h, "score_rows_block", NEED_BOUND | NEED_ROWS | NEED_P_ALL, KIND_PLAIN, s);
  if (rc || r0 == r1) return rc;
  return score_rows(h, (int32_t)r0, (int32_t)r1, out, s, {Gu_rows, Tu_rows});
}

// bprx_score_block of an ACF handle for caller-owned rows (users folded in by bprx_acf_fold_in): g' of the rows with the caller's
// histories, then the same scoring kernels
extern "C" int bprx_acf_score_rows_block(bprx_handle *h, const float *Gu_rows, int64_t n_rows, const int64_t *hist_ptr,
                                         const int32_t *hist_items, int64_t r0, int64_t r1, float *out, void *stream) {
  if (!h) return BPRX_E_INVALID;
  if (n_rows < 0 || n_rows >= ((int64_t)1 << 31) || r0 < 0 || r1 > n_rows || r0 > r1)
    BPRX_FAIL(h, BPRX_E_INVALID, "acf_score_rows_block: bad row range [%lld,%lld) of %lld", (long long)r0, (long long)r1, (long long)n_rows);
  if (r0 != r1 && (!Gu_rows || !hist_ptr || !hist_items || !out)) BPRX_FAIL(h, BPRX_E_INVALID, "acf_score_rows_block: null pointer");
  hipStream_t s = (hipStream_t)stream;
  int rc = bprx_enter(h, "acf_score_rows_block", NEED_BOUND, KIND_ACF, s);
  if (rc || r0 == r1) return rc;
  float *gp = nullptr;
  if ((rc = bprx_acf_row_profiles(h, Gu_rows, r0, r1, hist_ptr, hist_items, &gp, s))) return rc;
  return score_rows(h, 0, (int32_t)(r1 - r0), out, s, {gp, h->t.Tu});
}

// ---- items outside the catalogue (include/bprx.h): bprx_project_rows here, bprx_score_new_block / bprx_topk_rows in
// bprx_eval.hip, bprx_feat_explain_new in bprx_explain.hip ----
extern "C" int32_t bprx_proj_stride(const bprx_handle *h) {
  return h && h->cfg.model == BPRX_MODEL_VBPR ? h->PS : BPRX_E_INVALID;
}

extern "C" int bprx_project_rows(bprx_handle *h, const void *Fnew, int64_t n, float *P, void *stream) {
  if (!h) return BPRX_E_INVALID;
  if (n < 0 || n >= ((int64_t)1 << 31)) BPRX_FAIL(h, BPRX_E_INVALID, "project_rows: n = %lld out of range", (long long)n);
  if (n && (!Fnew || !P)) BPRX_FAIL(h, BPRX_E_INVALID, "project_rows: null pointer");
  if ((uintptr_t)Fnew & 15) BPRX_FAIL(h, BPRX_E_INVALID, "project_rows: the table must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int rc = bprx_enter(h, "project_rows", NEED_BOUND | NEED_ROWS | NEED_ET, KIND_VBPR_NO_FP8, s);
  if (rc || n == 0) return rc;
  return bprx_launch_proj_new(h, Fnew, n, P, s);
}

extern "C" int bprx_step_lr(const bprx_handle *h, float *lr_t) {
  if (!h || !lr_t) return BPRX_E_INVALID;
  *lr_t = h->step.lr_t;
  return BPRX_OK;
}

extern "C" int bprx_index_pass_kind(const bprx_handle *h) { return h ? h->step.idx_kind : 0; }
extern "C" int bprx_index_pass_queue(const bprx_handle *h) { return h && h->step.idxq ? 1 : 0; }
extern "C" int bprx_proj_mask_kind(const bprx_handle *h) {
  if (!h || !h->step.mask) return 0;
  const bool fwd = bprx_proj_fwd_takes_mask(*h), bwd = bprx_proj_bwd_takes_mask(*h);
  return fwd ? (bwd ? 1 : 2) : (bwd ? 3 : 0);
}

extern "C" int bprx_sync_check(bprx_handle *h, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  { const int rc = bprx_enter(h, "sync_check", 0, KIND_ANY, s); if (rc) return rc; }
  int32_t flag = 0;
  BPRX_HIP(h, hipMemcpyAsync(&flag, h->errflag, sizeof(flag), hipMemcpyDeviceToHost, s));
  BPRX_HIP(h, hipStreamSynchronize(s));
  if (flag) {
    BPRX_HIP(h, hipMemsetAsync(h->errflag, 0, sizeof(flag), s));
    BPRX_FAIL(h, BPRX_E_RANGE, "a user/item index was out of range (code %d); it was clamped, results are invalid", flag);
  }
  return BPRX_OK;
}
