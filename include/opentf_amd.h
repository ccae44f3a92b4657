/* opentf_amd.h — C ABI of the MI355X-native engine for OpeNTF's fnn/bnn minibatch hot path.
 *
 * The reference (fani-lab/OpeNTF) is pure Python and has no FFI; the boundary it offers is the model
 * plugin API of src/mdl/ntf.py:5-31 (constructor, learn, test).  This library is what a C-ABI
 * replacement of the body of that API binds (last row).  Each entry point names the
 * reference code it replaces (paths relative to the reference root).
 *
 * Conventions
 *   - every function returns 0 on success, a negative NTF_E* code on failure; ntf_last_error() gives
 *     the message (per engine; for a failed create, pass NULL).  No exceptions cross the ABI.
 *   - plain pointers and sizes only.  "host" pointers are ordinary host memory, copied in/out.
 *     "dev" pointers are HBM addresses owned by the engine (exposed for RCCL all-reduce).
 *   - an engine is bound to one GPU and one HIP stream; it is not thread-safe; no global state.
 *   - there is no CPU fallback: without a usable HIP device ntf_engine_create fails.
 */
#ifndef OPENTF_AMD_H
#define OPENTF_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NTF_ABI_VERSION 2
#define NTF_MAX_LAYERS 8

enum { NTF_OK = 0, NTF_EINVAL = -1, NTF_EHIP = -2, NTF_ESTATE = -3, NTF_ENOMEM = -4 };

/* how a minibatch's input rows X[B, D] are produced on the device */
enum ntf_input_mode {
    NTF_INPUT_DENSE = 0,   /* rows of a resident dense [N, D] f32 matrix (D2v vectors; src/mdl/ntf.py:24 else-branch) */
    NTF_INPUT_MEANPOOL = 1,/* mean of the team's skill-embedding rows: CSR(skill) @ E / nnz (src/mdl/emb/gnn.py:484-486) */
    NTF_INPUT_MULTIHOT = 2 /* multi-hot skill row (src/mdl/ntf.py:23); layer 0 becomes a CSR gather-sum of W0 columns */
};

/* negative sampling distribution, src/mdl/fnn.py:34-36 */
enum ntf_nsd { NTF_NSD_NONE = 0, NTF_NSD_UNIFORM = 1, NTF_NSD_UNIGRAM = 2, NTF_NSD_UNIGRAM_B = 3 };

/* parameter kinds of one layer; Fnn uses WEIGHT/BIAS, Bnn all four in the state_dict order
 * mu_weight, rho_weight, mu_bias, rho_bias (src/mdl/bnn.py:25 via bayesian-torch LinearFlipout) */
enum ntf_param_kind { NTF_P_WEIGHT = 0, NTF_P_BIAS = 1, NTF_P_RHO_WEIGHT = 2, NTF_P_RHO_BIAS = 3 };

enum ntf_mfma { NTF_MFMA_DEFAULT = 0, NTF_MFMA_F32 = 1, NTF_MFMA_BF16X6_RETIRED = 2 /* rejected by ntf_engine_create since round 6 */, NTF_MFMA_FP16X3 = 3 };

typedef struct ntf_config {
    int32_t abi_version;        /* NTF_ABI_VERSION */
    int32_t device;             /* HIP device ordinal ("cuda:N" of src/__config__.yaml:10) */
    void*   stream;             /* hipStream_t to run on, or NULL: the engine creates its own */
    int32_t n_layers;           /* number of Linear layers = len(h) + 1 (src/mdl/fnn.py:20-22) */
    int32_t dims[NTF_MAX_LAYERS + 1]; /* D, h[0], ..., h[-1], M */
    int32_t bayesian;           /* 0 = Fnn, 1 = Bnn/Flipout (src/mdl/bnn.py:17-27) */
    int32_t input_mode;         /* enum ntf_input_mode */
    int32_t max_batch;          /* cfg.b (src/mdl/__config__.yaml:1) */
    int32_t ns;                 /* cfg.ns */
    int32_t nsd;                /* enum ntf_nsd */
    float   tpw, tnw;           /* cfg.tpw, cfg.tnw (src/mdl/fnn.py:45) */
    float   lr;                 /* cfg.lr; Adam defaults beta 0.9/0.999 eps 1e-8 (src/mdl/fnn.py:104) */
    uint64_t seed;              /* seed of the device-side generators (negatives, Flipout eps and signs) */
    int32_t fused;              /* 1 = use the fused output-layer kernels when the shape allows, 0 = generic path */
    int32_t fuse_adam;          /* single-GPU train steps only.  0: one flat Adam kernel after backward.  1: the output layer's Adam runs inside
                                   the dW kernel's epilogue (its gradients are not materialised).  2: the dW kernel is launched in expert chunks
                                   and Adam of a finished chunk runs on a side stream beside the next chunk's dW */
    int32_t mfma;               /* arithmetic of the fused output-layer products: NTF_MFMA_DEFAULT (0) = NTF_MFMA_FP16X3 = each operand times an exact power of two
                                   split into two fp16 values (22 bits), three fp16 MFMA products per f32 product, f32 accumulate (error against f64 ~1.2x that of
                                   the f32 MFMA; operands outside the fp16 window send the step to the exact-f32 kernels, ntf_range_fallbacks);
                                   NTF_MFMA_F32 = v_mfma_f32_32x32x2_f32 (a bit-exact f32 fma chain).  2 (bf16x6, rounds 1-5) is rejected */
    /* Expert-sharded output layer (every field 0 = off).  This engine owns the experts [expert_lo, expert_lo + dims[n_layers]) of an
       output layer of `experts_global` experts that is split over `ep_world` engines (one per GPU); hidden layers are replicated.  Every engine
       steps the WHOLE minibatch: labels (member CSR) and sampled negatives keep global expert ids, the device generators are keyed by global
       ids, and the only exchange of a train step is the sum over engines of d(hidden) [B, h[-1]] between ntf_step_staged_ep phases 1 and 3.
       expert_lo must be a multiple of 256; needs the fused output-layer path (h[-1] in {32, 64, 128, 256}). */
    int32_t expert_lo;
    int32_t experts_global;
    int32_t ep_world;
    int32_t reserved[2];
} ntf_config;

/* Random tensors of one step, injected instead of generated (parity tests).  Any pointer may be NULL
 * (= generate on device).  All are HOST pointers.  Layouts follow bayesian-torch LinearFlipout.forward:
 * eps_w[l] [out,in], eps_b[l] [out], s_in[l] [B,in] (+1/-1 as f32), s_out[l] [B,out] (+1/-1 as f32);
 * neg_idx [B, ns] int64 as returned by src/mdl/fnn.py:48-76. */
typedef struct ntf_inject {
    const int64_t* neg_idx;
    const float* eps_w[NTF_MAX_LAYERS];
    const float* eps_b[NTF_MAX_LAYERS];
    const float* s_in[NTF_MAX_LAYERS];
    const float* s_out[NTF_MAX_LAYERS];
} ntf_inject;

typedef struct ntf_engine ntf_engine;

/* ---- lifetime:  Fnn.init / Bnn.init + model.to(device)            src/mdl/fnn.py:15-30,100-102 */
int  ntf_engine_create(const ntf_config* cfg, ntf_engine** out);
void ntf_engine_destroy(ntf_engine* e);
const char* ntf_last_error(const ntf_engine* e);
int  ntf_abi_version(void);

/* ---- data residency (once per learn/test call): replaces NtfDataset's per-sample densify
 *      src/mdl/ntf.py:16-25.  CSR = int64 indptr [n_rows+1], int32 indices [nnz]; values are 1. */
int ntf_set_member_csr(ntf_engine* e, const int64_t* indptr, const int32_t* indices, int64_t n_rows);
int ntf_set_skill_csr(ntf_engine* e, const int64_t* indptr, const int32_t* indices, int64_t n_rows);
int ntf_set_skill_table(ntf_engine* e, const float* table, int64_t n_skills, int32_t d); /* E of gnn.py:485 */
int ntf_set_dense_input(ntf_engine* e, const float* X, int64_t n_rows, int32_t d);
int ntf_set_unigram(ntf_engine* e, const double* freq, int64_t n);                         /* src/mdl/fnn.py:82 */

/* ---- state:  state_dict() / load_state_dict()                     src/mdl/fnn.py:101,160,168,187 */
int ntf_set_param(ntf_engine* e, int layer, int kind, const float* host, int64_t count);
int ntf_get_param(ntf_engine* e, int layer, int kind, float* host, int64_t count);
int ntf_get_grad(ntf_engine* e, int layer, int kind, float* host, int64_t count); /* p.grad after backward, fnn.py:137.  Valid after ntf_backward (or a step with fuse_adam = 0):
                                                                                     a fused step (fuse_adam = 1, ntf_train_step) consumes the gradients of the tensors it updates in a kernel's
                                                                                     epilogue - the output layer's weight / rho_weight (never written), a multi-hot Flipout first layer's (read and
                                                                                     cleared by its one-pass update) - and this call then returns zeros or the previous backward's values for them */
/* d loss / d z [B, M] of the output layer (z = its pre-activation) as the last backward / train step left it: what autograd holds for
 * `y_` of src/mdl/fnn.py:132 before leaky_relu.  The fused kernels' only dense product, exposed so that it can be checked element-wise. */
int ntf_get_dlogits(ntf_engine* e, float* host, int64_t count);
/* The sampled negatives [B, ns] (GLOBAL expert ids) of the last step: `topk_indices` of src/mdl/fnn.py:48-76 as the device samplers drew them (or as they were injected).
 * Exposed so that the samplers can be checked draw by draw over a sequence of steps (batch support, distinctness, frequencies), not only through the loss. */
int ntf_get_negatives(ntf_engine* e, int64_t* host, int64_t count);
/* The device generators' own draws of ONE random tensor of bayesian-torch's LinearFlipout.forward (called from src/mdl/fnn.py:126,135 through mdl/bnn.py:17-27) for step
 * index `step` of this engine's seed - what a native, non-injected step with that index consumes: kind 0 eps_weight [out, in], 1 eps_bias [out], 2 sign_input
 * [rows, in], 3 sign_output [rows, out] (+1 / -1; row r = position r of the step's minibatch), in the reference's layouts.  Exposed so that a sequence of native
 * steps can be replayed through the oracle with exactly the tensors the kernels regenerate in place (forward sign words, the dW epilogue's re-drawn eps, the
 * operands the previous step's epilogue produced): tests/test_gpu_replay.py. */
int ntf_get_noise(ntf_engine* e, uint64_t step, int32_t layer, int32_t kind, int32_t rows, float* host, int64_t count);
int ntf_reset_optimizer(ntf_engine* e);                  /* fresh Adam per fold, src/mdl/fnn.py:104 */
int ntf_set_lr(ntf_engine* e, float lr);                 /* ReduceLROnPlateau result, fnn.py:105,163 */
int ntf_set_seed(ntf_engine* e, uint64_t seed, uint64_t step);
/* the device generators (Flipout eps, signs, sampled negatives) are keyed by (seed, step counter, global row position); every step call
 * advances the counter.  A data-parallel rank whose shard of a global minibatch is EMPTY makes no step call: it calls this instead, so
 * that all ranks keep drawing the same eps for the same global step. */
int ntf_skip_step(ntf_engine* e);
/* fp16x3 arithmetic (NTF_MFMA_FP16X3 / default) splits weights * 2^8 and activations * 2^4 into fp16 pairs: exact for |w| < 255.9,
 * |h| < 4094.  Operands are range-checked where they are split; a step (or inference call) in which one leaves that window runs on the
 * exact-f32 kernels instead - never on saturated values.  This reports how many steps / calls did so since the engine was created. */
int ntf_range_fallbacks(ntf_engine* e, int64_t* steps);
/* A fused train step's dW + Adam kernel holds the output layer's UPDATED mu / rho in its epilogue and writes, from them, the NEXT step's Flipout operands
 * (eps of step + 1, sigma * eps, the split planes, the layer's KL - bayesian-torch's LinearFlipout.forward / kl_loss, called at src/mdl/fnn.py:126,136) -
 * that step then starts without the operand producer's own pass over the layer.  Reports how many steps started that way (same results either way:
 * the arithmetic is the producer's; NTF_PREFETCH=0 in the environment turns it off). */
int ntf_prefetched_steps(ntf_engine* e, int64_t* steps);
/* ... and, behind its hidden-layer backward, its side stream runs what the NEXT batch of the staged order (ntf_step_staged walks it front to back, as the loader of
 * src/mdl/fnn.py:118 does) needs before its forward kernel: the negative sampler (fnn.py:48-72), the team2vec gather and the hidden layer (src/mdl/emb/gnn.py:485,
 * fnn.py:25) - beside the dW kernel instead of between two steps' big kernels.  Reports how many steps found their head done that way (same results either way;
 * NTF_HEAD_PREFETCH=0 turns it off; per-batch unigram_b tables, injected tensors, expert shards and data-parallel shards always run their head in their own step). */
int ntf_head_prefetch_hits(ntf_engine* e, int64_t* steps);
/* Multi-hot input with a Flipout first layer (BASELINE config 3: 90 671 x 128 mu / rho pairs, src/mdl/ntf.py:23 + src/mdl/fnn.py:25,136-139): in a fused train step the
 * layer's gradient finalisation (Flipout chain rule + KL), its Adam update and the NEXT step's sigma * eps + KL term are ONE pass over the layer beside the dW kernel
 * (launch_flipout_sweep) instead of three.  Reports how many steps started on a first-layer operand produced that way (same results either way; NTF_L0_SWEEP=0 turns it off). */
int ntf_first_layer_sweeps(ntf_engine* e, int64_t* steps);

/* ---- the step:  body of the hot loop                              src/mdl/fnn.py:118-151
 * rows = B global team ids (host).  loss_out may be NULL: then nothing is synchronised and the loss is
 * only added to the epoch accumulator (ntf_epoch_loss). */
int ntf_train_step(ntf_engine* e, const int64_t* rows, int32_t B, const ntf_inject* inj, float* loss_out);
int ntf_eval_step(ntf_engine* e, const int64_t* rows, int32_t B, const ntf_inject* inj, float* loss_out);
/* split form for data parallelism: backward leaves d(loss_sum_over_rows / global_B)/dparam in the flat
 * gradient buffer (sum over ranks = the single-process gradient); apply runs Adam. */
int ntf_backward(ntf_engine* e, const int64_t* rows, int32_t B, int32_t global_B, const ntf_inject* inj, float* loss_out);
int ntf_apply(ntf_engine* e);
/* one Adam step restricted to n [lo, hi) float ranges of the flat buffers (lo_hi = 2n offsets, lo a multiple of 4): a data-parallel rank
 * updates only the shard of the optimiser state it owns after a reduce-scatter of the gradients; parameters are then all-gathered */
int ntf_apply_ranges(ntf_engine* e, const int64_t* lo_hi, int32_t n);
/* whole phase without host round trips: `for batch in loader` of src/mdl/fnn.py:118 run natively.
 * order = n row ids in the order the loader yields them; mean of batch losses is returned (fnn.py:153). */
int ntf_train_epoch(ntf_engine* e, const int64_t* order, int64_t n, int32_t B, float* mean_loss);
int ntf_eval_epoch(ntf_engine* e, const int64_t* order, int64_t n, int32_t B, float* mean_loss);
int ntf_epoch_loss(ntf_engine* e, double* sum, int64_t* steps); /* reads and clears the accumulator */
/* the same without any per-step host copy: stage the epoch's row order once, then step by offset.  The local
 * shard is order[offset, offset+B); the global minibatch it belongs to is order[global_offset, +global_B)
 * (they coincide on one GPU).  apply != 0 runs Adam right after backward (single GPU). */
int ntf_stage_order(ntf_engine* e, const int64_t* order, int64_t n);
int ntf_step_staged(ntf_engine* e, int64_t offset, int32_t B, int64_t global_offset, int32_t global_B, int32_t train, int32_t apply, float* loss_out);

/* data-parallel pipelining.  ntf_step_staged_deferred = ntf_step_staged(train=1, apply=0) except that the output layer's
 * weight-gradient kernel is left pending; ntf_dw_chunk(k), k = 0..n-1 in order, then launches it for the k-th range of experts, so that
 * the host can all-reduce the gradients of chunk k while chunk k+1 is being computed.  ntf_dw_chunks: n for this model (0 when the
 * fused output-layer path does not apply: nothing is deferred then).  ntf_dw_chunk_range: where chunk k's gradients sit in the flat
 * gradient buffer (offsets in floats; off_rho = -1 for Fnn) - a pure function of the model shape, identical on every rank.
 * After the last chunk the whole gradient buffer is complete - on the engine's stream: the hidden layers' backward of a deferred step runs on a side stream beside the
 * chunks (round 5) and is joined behind the LAST ntf_dw_chunk, so work queued on the engine's stream after that call (the caller's collectives) sees every gradient;
 * ntf_get_grad / ntf_apply / ntf_apply_ranges / ntf_epoch_loss / ntf_synchronize / the next step join it themselves if the chunks were abandoned.
 * ntf_param_segment: where a parameter sits in the flat buffers. */
int ntf_step_staged_deferred(ntf_engine* e, int64_t offset, int32_t B, int64_t global_offset, int32_t global_B, float* loss_out);
int ntf_dw_chunks(ntf_engine* e, int32_t* n_chunks);
int ntf_dw_chunk_range(ntf_engine* e, int32_t k, int64_t* off_weight, int64_t* off_rho, int64_t* count);
int ntf_dw_chunk(ntf_engine* e, int32_t k);
/* ... and of the step's HEAD (round 5).  Under data parallelism the output layer's parameters arrive by all-gather in the ranges of ntf_dw_chunk_range; a rank need not
 * wait for all of them before its next step: ntf_step_staged_deferred_cb runs the Flipout operand producer and the forward kernel RANGE BY RANGE (ntf_fwd_ranges: up to
 * four ranges of whole dW chunks, k0_k1[2 j], k0_k1[2 j + 1] = the dW chunks [k0, k1) of range j; 0 ranges: the model / arithmetic does not allow it - use
 * ntf_step_staged_deferred) and calls `before_range(j, user)` on the calling thread in front of range j: the caller makes the engine's stream wait for the all-gathers of
 * that range's chunks there (e.g. torch's Work.wait()), so that RCCL moves range j + 1 while the forward kernel works on range j.  A non-zero return aborts the step
 * (NTF_ESTATE).  Everything else is ntf_step_staged_deferred.  No counterpart in the reference (src/__config__.yaml:10 "TODO: multiple gpus"). */
int ntf_fwd_ranges(ntf_engine* e, int32_t B, int32_t* n_ranges, int32_t* k0_k1);
int ntf_step_staged_deferred_cb(ntf_engine* e, int64_t offset, int32_t B, int64_t global_offset, int32_t global_B, float* loss_out,
                                int (*before_range)(int32_t range, void* user), void* user);
int ntf_param_segment(ntf_engine* e, int layer, int kind, int64_t* off, int64_t* count);

/* expert-sharded output layer (ntf_config.expert_lo ..): one train step on the whole minibatch order[offset, offset + B) in three phases.
 * phase 1: forward, loss, sparse fix-up - leaves this engine's PARTIAL d(hidden) in the buffer ntf_dh_buffer names ([B, h[-1]] floats, row-major);
 * (the host starts the sum of that buffer over the engines: one all-reduce of B * h[-1] floats, the only exchange of the step;)
 * phase 2: the output layer's backward on this engine's experts, its Adam included - independent of the exchange, which it hides;
 * (the host makes the engine's stream wait for the all-reduce;)
 * phase 3: backward through the replicated hidden layers from the summed d(hidden), Adam on them (identical on every engine).
 * The loss accumulated for ntf_epoch_loss is this engine's share: sum over engines = the single-engine loss.  Evaluation steps need no
 * exchange: ntf_step_staged(train = 0) as usual.  src/mdl/fnn.py:122-140 (the step this splits) */
int ntf_step_staged_ep(ntf_engine* e, int64_t offset, int32_t B, int32_t phase);
int ntf_dh_buffer(ntf_engine* e, void** dev_ptr, int64_t* n_floats);

/* ---- inference:  Fnn.test batch body                              src/mdl/fnn.py:200-211
 * probs_host [B, M] = sigmoid(forward) (Bnn: mean over nmc stochastic forwards);
 * pred_unc/model_unc [B] = predictive entropy / mutual information (may be NULL). */
int ntf_forward(ntf_engine* e, const int64_t* rows, int32_t B, int32_t nmc, const ntf_inject* inj_per_mc,
                float* probs_host, float* pred_unc, float* model_unc);
/* pre-sigmoid post-leaky_relu logits of ONE forward (the quantity the 1e-4 parity bar is stated on); computed by the same kernel as
 * ntf_forward (for H = 128: the split-product forward kernel), not by a separate reference path */
int ntf_logits(ntf_engine* e, const int64_t* rows, int32_t B, const ntf_inject* inj, float* logits_host);
/* top-K per row of the probabilities, without moving [B, M] to the host   src/pkgmgr.py:125-134 */
int ntf_forward_topk(ntf_engine* e, const int64_t* rows, int32_t B, int32_t nmc, int32_t K,
                     float* values_host, int32_t* indices_host, float* pred_unc, float* model_unc);
/* Fused Monte-Carlo inference (NTF_INFER_MC=1 in the environment at engine creation; off by default).  Bnn.test averages nmc stochastic forwards
 * (src/mdl/fnn.py:202-211); the default path runs them as nmc passes over the output layer, each reading and rewriting the running mean of every probability.
 * With the switch on, Flipout models with h[-1] = 128 on the default (fp16x3) arithmetic run up to NTF_MC_MAX_GROUP passes inside one kernel launch, the running
 * sums in registers (ntf_forward / ntf_forward_topk with nmc > 1 and no injected noise; everything else keeps the default path).  The probabilities, the top-K and
 * pred_unc are bit-identical either way; model_unc differs by the rounding of one f32 sum taken in another order.  The per-pass operands (fp16 planes of
 * sigma * eps, bias operand) of a launch live in a ring bounded by NTF_INFER_MC_BYTES (default 2 GiB); ntf_infer_mc_plan is the host function that sizes it:
 * *passes_per_group in [1, min(passes, NTF_MC_MAX_GROUP)] passes per launch and *experts_per_range experts per launch (a positive multiple of 256; the last
 * range of a layer may be shorter) such that passes_per_group * experts_per_range * (4 h + 4) + experts_per_range * 4 h <= budget_bytes - as many passes per
 * launch as fit before longer ranges, since only a group holding all passes removes the read-modify-write entirely.  NTF_EINVAL when one pass over 256 experts
 * does not fit or an argument is not positive.  Needs no engine and no GPU. */
#define NTF_MC_MAX_GROUP 16
#define NTF_MC_TILE_GROUP 4      /* 32-expert tiles whose running sums a workgroup holds in registers across the passes of a launch */
int ntf_infer_mc_plan(int64_t experts, int32_t h, int32_t passes, int64_t budget_bytes, int32_t* passes_per_group, int64_t* experts_per_range);
/* Monte-Carlo passes served by fused-MC launches whose call was not redone on the exact-f32 kernels behind a raised range flag (ntf_range_fallbacks) */
int ntf_mc_fused_passes(ntf_engine* e, int64_t* passes);

/* ---- the team2vec gather on its own:  Gnn.get_dense_vecs           src/mdl/emb/gnn.py:484-486
 * out_host [n, d] (may be NULL to keep the result on the device only); rows NULL = 0..n-1. */
int ntf_gather_meanpool(ntf_engine* e, const int64_t* rows, int64_t n, float* out_host);

/* ---- raw device views for RCCL (torch.distributed) and measurement */
/* ntf_grad_buffer: every step computes its gradient from zero, whatever the buffer held before (src/mdl/fnn.py:122-140).  The multi-hot
 * first layer's one-pass sweep clears the rows it reads, and the next step skips the memset in front of its scatter; taking this view
 * makes the next step zero the layer's gradient again, so the caller may write the buffer between steps.  A view held across steps
 * (dp.py) is safe only on engines that never sweep; data-parallel steps do not (they ignore fuse_adam). */
int ntf_grad_buffer(ntf_engine* e, void** dev_ptr, int64_t* n_floats);
int ntf_param_buffer(ntf_engine* e, void** dev_ptr, int64_t* n_floats);
/* A caller that WRITES parameters through the view above (an all-gather, a broadcast: torch.optim's `p.data.copy_`, src/mdl/fnn.py:104) says so before the next
 * step: operands a fused train step prepared for its successor from the old values (eps, sigma eps, split planes, KL) are dropped and made again.
 * ntf_param_buffer itself also drops what is pending at the time of the call; ntf_set_param / ntf_apply_ranges / ntf_set_seed do it on their own. */
int ntf_params_touched(ntf_engine* e);
/* Adam's first / second moments (torch.optim.Adam's exp_avg / exp_avg_sq, src/mdl/fnn.py:104), same flat layout as the parameters: an expert-sharded
 * run re-broadcasts the replicated hidden layers' parameters AND moments once per epoch (opentf_amd/ep.py) */
int ntf_moment_buffers(ntf_engine* e, void** dev_m1, void** dev_v2, int64_t* n_floats);
int ntf_synchronize(ntf_engine* e);
/* HIP-event timing of the kernels launched by the engine since the last reset, by kernel family:
 * names[i] (static strings), ms[i] total, calls[i].  Returns the number of families (<= cap).
 * enable: 0 off, 1 every family (two event records around each of ~15 scopes per step), 2 only the output layer's two MFMA kernels
 * (what a roofline needs; keeps the timed region of a benchmark free of the other families' event records), 3 / 4 only its forward / only its dW + Adam kernel
 * (an event pair costs the step ~8 us: a benchmark that alternates 3 and 4 between its timed regions measures both kernels live at half that price) */
int ntf_kernel_times(ntf_engine* e, int enable, const char** names, double* ms, int64_t* calls, int cap);

/* ---- stateless kernels on caller-owned device memory (used by tests and micro-benchmarks) */
int ntf_k_gemm_f32(void* stream, int m, int n, int k, const float* A, int64_t sam, int64_t sak,
                   const float* B, int64_t sbk, int64_t sbn, float* C, int64_t ldc);

/* ---- ranking metrics of the eval stage on the device (next row after the hot path)            src/evl/metric.py:5-35,44-73
 * topk_idx [n, K]: expert ids ranked by decreasing score (ntf_forward_topk order).  The truth / required-skill row of instance i is
 * rows[i] (NULL: i) of the CSR.  out_metrics [n, 5*n_cut] = P, recall, ndcg_cut, map_cut, success, each over the cutoffs (trec_eval
 * definitions, binary relevance);  out_cov [n, n_cut] = |skills of the top-k experts ∩ required| / |required|.
 * At most 8 cutoffs, each >= 1.  ntf_skill_coverage returns NTF_EINVAL when a selected required-skill row is empty (0 / 0). */
int ntf_rank_metrics(int device, const int32_t* topk_idx, int64_t n, int32_t K, const int64_t* truth_indptr, const int32_t* truth_indices,
                     int64_t n_truth_rows, const int64_t* rows, const int32_t* cutoffs, int32_t n_cut, float* out_metrics);
int ntf_skill_coverage(int device, const int32_t* topk_idx, int64_t n, int32_t K, const int64_t* skill_indptr, const int32_t* skill_indices,
                       int64_t n_skill_rows, const int64_t* rows, const int64_t* cov_indptr, const int32_t* cov_indices, int64_t n_experts,
                       const int32_t* cutoffs, int32_t n_cut, float* out_cov);

/* ---- micro-averaged ROC AUC of the eval stage on the device                                                      src/evl/metric.py:36-41
 * `roc_auc_score(Y.toarray(), Y_.toarray(), average='micro')` as the Mann-Whitney statistic with mid-ranks over all n * M (score, label)
 * pairs, in integers: out_counts = { P, N, U2 } with P = positives, N = n * M - P, U2 = sum over positives of (2 * #negatives scored lower
 * + #negatives scored equal); *out_auc = (double)U2 / (2.0 * (double)P * (double)N).  Scores are f32 compared as real numbers: -0.0 ties
 * with +0.0, denormals are distinct values, +-inf are ordinary values.  The truth row of instance i is rows[i] (NULL: i) of the CSR.
 * ntf_auc_micro_dense: scores host, row-major [n, M], ld >= M floats per row (the padding is never read).  ntf_auc_micro_csr: scores as
 * CSR (int64 indptr [n+1], int32 indices, f32 values); an entry that is not stored scores 0.0, stored values may be 0.0 or negative.
 * chunk_bytes: device staging budget for score data per upload - the scores are streamed in chunks of whole rows (dense, M * 4 bytes each)
 * or of stored entries (CSR: their f32 values, 4 bytes each; the column ids stay on the host) of at most that size; 0 = NTF_AUC_CHUNK_BYTES.
 * A budget below one row / one entry is refused.
 * NTF_EINVAL (out_counts / out_auc untouched): a null pointer or non-positive size, ld < M, a rows value outside [0, n_truth_rows), a
 * truth or score column outside [0, M), indices not strictly increasing inside a row, a NaN score, P == 0 or N == 0, or 2 * P * N >= 2^64. */
#define NTF_AUC_CHUNK_BYTES ((int64_t)256 << 20)
int ntf_auc_micro_dense(int device, const float* scores, int64_t n, int64_t M, int64_t ld,
                        const int64_t* truth_indptr, const int32_t* truth_indices, int64_t n_truth_rows, const int64_t* rows,
                        int64_t chunk_bytes, uint64_t out_counts[3], double* out_auc);
int ntf_auc_micro_csr(int device, const int64_t* s_indptr, const int32_t* s_indices, const float* s_values, int64_t n, int64_t M,
                      const int64_t* truth_indptr, const int32_t* truth_indices, int64_t n_truth_rows, const int64_t* rows,
                      int64_t chunk_bytes, uint64_t out_counts[3], double* out_auc);

/* ---- scoring a prediction set where it is produced: the three sections above on the engine's own probabilities      src/mdl/ntf.py:32-92
 * Scores the prediction set rows[0, n) in batches rows[o, o + B) (the last one may be shorter; B in [1, max_batch]) without a prediction file, a host sort or an
 * upload: the truth of instance i is row rows[i] of the resident member CSR (ntf_set_member_csr).  Whole-model engines only (NTF_ESTATE on an expert shard).
 * The matrix that is scored is the one the eval stage reads from the `.pred` file test() writes:
 *   K >= 1 (K <= min(M, 2048)): the top-K-sparsified prediction - a row's K largest probabilities in ntf_forward_topk's order (ties to the lower id), every other
 *     entry 0.0: what ntf_auc_micro_csr computes on that file.  The ranked list of a row is its K stored ids; cutoffs above K behave as in ntf_rank_metrics.
 *   K == 0: the dense probabilities - what ntf_auc_micro_dense computes on the concatenated ntf_forward outputs.  The ranked list of a row is its top
 *     max(cutoffs), which must be <= min(M, 2048).
 * out_metrics [n, 5 * n_cut] (or NULL): ntf_rank_metrics' layout and definitions over the cutoffs (at most 8, each >= 1).  out_counts = { P, N, U2 } and
 * *out_auc = U2 / (2 P N) (both or neither NULL): the integers of the AUC section above.  out_vals / out_idx [n, K_out] (either may be NULL; K_out = 0 when both
 * are): the first K_out ranked entries of every row, K_out <= K (dense: <= max(cutoffs)) - for ntf_skill_coverage or a `.pred` file without a second inference.
 * Generators: the call takes the step indices a loop of ntf_forward_topk (K >= 1) / ntf_forward (K == 0) calls over the same batches would take from the engine's
 * current step, produces bit-identical probabilities, and leaves the step counter where that loop would.  No injected noise.
 * Top-K mode infers once, into an [n, K] device store (n * K * 8 bytes; NTF_ENOMEM when it does not fit).  Dense mode holds no [n, M] store: when the AUC is asked
 * for it runs the inference twice from the same steps (the second sweep feeds the counting kernel) and relies on the replay being bit-identical.  Every positive must
 * be found among the counted scores and exactly n * M scores must be counted; a replay that is not bit-identical (whatever the inference arm: NTF_INFER_MC,
 * NTF_INFER_F32, a range fallback, the generic chain) fails these checks and the call returns NTF_EHIP - the AUC is refused, never approximated.
 * NTF_EINVAL, every output untouched: a null or non-positive argument outside the above, a row id out of range, K > min(M, 2048), n_cut > 8 or a cutoff < 1, a dense
 * call whose largest cutoff exceeds min(M, 2048), nothing asked for, a NaN probability, and with the AUC asked for P == 0, N == 0 or 2 P N >= 2^64. */
int ntf_score_rows(ntf_engine* e, const int64_t* rows, int64_t n, int32_t B, int32_t nmc, int32_t K, const int32_t* cutoffs, int32_t n_cut,
                   float* out_metrics, uint64_t out_counts[3], double* out_auc, int32_t K_out, float* out_vals, int32_t* out_idx);

/* ---- member-skill co-occurrence on the device                                                 src/cmn/team.py:302-337
 * `Team.gen_skill_coverage`: C = member^T . skill over the teams NOT listed in skip_rows (the reference empties the test teams' rows,
 * team.py:327-331), as scipy computes it on the two uint8 matrices: counts wrap mod 256, entries whose wrapped count is 0 are not stored.
 * CSR inputs are host pointers (column ids unique inside a row); the result [n_members, n_skills] stays on the device behind an opaque
 * handle: *nnz tells the caller how much to allocate, ntf_csr_result_fetch copies indptr [n_members+1] / indices / data (column ids
 * ascending inside a row = scipy's result after sort_indices()) and reports the device time of the build. */
typedef struct ntf_csr_result ntf_csr_result;
int ntf_skill_cooccurrence(int device, int64_t n_teams, int32_t n_members, int32_t n_skills, const int64_t* m_indptr, const int32_t* m_indices,
                           const int64_t* s_indptr, const int32_t* s_indices, const int64_t* skip_rows, int64_t n_skip,
                           ntf_csr_result** out, int64_t* nnz);
int ntf_csr_result_fetch(ntf_csr_result* r, int64_t* indptr, int32_t* indices, uint8_t* data, double* device_ms);
void ntf_csr_result_free(ntf_csr_result* r);

/* ---- node2vec skill-embedding producer on the device                    src/mdl/emb/gnn.py:153-168 (model), 401-453 (_train_rw)
 * torch_geometric.nn.Node2Vec as the reference configures it (src/mdl/emb/__config__.yaml:58-70; p = q = 1 unless ntf_n2v_set_walk_bias says otherwise): uniform random walks over
 * a homogeneous CSR graph (rowptr [num_nodes+1] int64, col int32), windows of `context` nodes, negatives = start node + uniformly random
 * nodes, loss = -mean log(sigmoid(<start, rest>) + 1e-15) - mean log(1 - sigmoid(.) + 1e-15), dense Adam on embedding.weight [num_nodes, d]
 * (1 <= d <= 256: device rows are padded to a multiple of 64 floats, the pad stays zero; init_weight = the nn.Embedding initial draw, supplied by the host so that a seed reproduces torch's).
 * ntf_n2v_train_batch: one loader batch (gnn.py:416-419).  inj_pos / inj_neg non-NULL: the window rows [n, context] are given instead of
 * generated (parity tests); apply = 0 leaves the gradient in place (ntf_n2v_get(what = 1)) and skips Adam: a further apply = 0 call ADDS its
 * gradient to what is there, and ntf_n2v_get(what = 1) reads the sum and clears it.  walk_length counts NODES per
 * walk (= cfg.wl, as Node2Vec's constructor takes it).  Every accepted call takes the handle's next step index (the Philox counter word of its
 * walks and negatives: call t of a handle draws what ntf_n2v_walks(step = t) draws); a REFUSED call (NTF_EINVAL: context < 2 or > walk_length,
 * B < 1, walks_per_node < 1, num_neg < 0, a start node or an injected node id outside [0, num_nodes)) changes nothing - not the step index,
 * the table, the gradient or the moments - so the draws of later calls do not depend on it.  ntf_n2v_last_windows: the window rows [n, context] of the last accepted
 * ntf_n2v_train_batch as the device holds them, positive and negative (replay tests: row j * n_walks + r is nodes j .. j + context - 1 of walk r); the sizes come back
 * through n_pos / n_neg / context, a NULL row pointer asks for the sizes alone; NTF_ESTATE once ntf_n2v_walks or ntf_n2v_edge_bce has reused the scratch.  ntf_n2v_edge_bce: v_loss of gnn.py:420-431 before its second division. */
typedef struct ntf_n2v ntf_n2v;
int  ntf_n2v_create(int device, int64_t num_nodes, int32_t d, const int64_t* rowptr, const int32_t* col, const float* init_weight, uint64_t seed, ntf_n2v** out);
void ntf_n2v_destroy(ntf_n2v* h);
const char* ntf_n2v_last_error(const ntf_n2v* h);
int  ntf_n2v_walks(ntf_n2v* h, const int64_t* start, int64_t n, int32_t walk_length, uint64_t step, int64_t* out_host /* [n, walk_length] */);
int  ntf_n2v_train_batch(ntf_n2v* h, const int64_t* batch, int32_t B, int32_t walk_length, int32_t context, int32_t walks_per_node, int32_t num_neg, float lr,
                         const int64_t* inj_pos, int64_t n_pos, const int64_t* inj_neg, int64_t n_neg, int32_t apply, float* loss_out);
int  ntf_n2v_last_windows(ntf_n2v* h, int64_t* n_pos, int64_t* n_neg, int32_t* context, int64_t* pos_rows, int64_t* neg_rows);
int  ntf_n2v_get(ntf_n2v* h, int what /* 0 embedding.weight, 1 gradient */, float* host /* [num_nodes, d] */);
int  ntf_n2v_edge_bce(ntf_n2v* h, const int64_t* src, const int64_t* dst, int64_t n, float* mean_bce);
/* The optimiser of a handle (n2v or m2v).  kind 0: dense Adam, the default - every row moves every applied step through its moments.  kind 1: sparse Adam,
 * torch.optim.SparseAdam as torch_geometric's examples train Node2Vec / MetaPath2Vec(sparse=True) - a different optimiser, not a faster dense Adam.  An applied
 * step then updates only the TOUCHED rows: those whose id occurs anywhere (start or rest, positive or negative, the dummy row of a metapath handle included) in the
 * window rows whose gradient is in the buffer, the rows of earlier apply = 0 calls still pending included.  Touched goes by the id, not by g != 0: a touched row
 * whose summed gradient is exactly zero still decays its moments and moves.  Per element of a touched row, with b1 0.9, b2 0.999, eps 1e-8, t = applied steps so far:
 *   m += (1 - b1) (g - m);  v += (1 - b2) (g g - v);  p -= lr sqrt(1 - b2^t) / (1 - b1^t) * m / (sqrt(v) + eps)        (torch.optim._functional.sparse_adam)
 * every other row keeps the bits of p, m and v.  Afterwards the gradient is zero everywhere and no row is marked; ntf_n2v_get(what = 1) clears the marks with the
 * gradient.  NTF_EINVAL: another kind.  NTF_ESTATE: an applied step has been taken, or a gradient is pending from apply = 0 calls.  A refused call changes nothing.
 * ntf_n2v_moments: exp_avg and exp_avg_sq, [num_nodes, d] each without the pad columns, either pointer may be NULL; reads only, in both modes. */
int  ntf_n2v_set_optimizer(ntf_n2v* h, int32_t kind /* 0 dense Adam, 1 sparse Adam */);
int  ntf_n2v_moments(ntf_n2v* h, float* exp_avg /* [num_nodes, d] or NULL */, float* exp_avg_sq /* [num_nodes, d] or NULL */);
/* Lazy dense Adam: the table, the moments and the held-out loss of kind 0 above - bit for bit, given bit-identical gradients - while an applied step writes only
 * the rows its windows name.  It is a mode of the DENSE optimiser (kind stays 0), not a third optimiser: under dense Adam a row whose gradient is zero in step t
 * still moves,  m = b1 m;  v = b2 v;  p -= lr_t / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps),  from nothing but its own p, m, v and the step's two constants.
 * A lazy handle leaves such a row where it is, keeps the steps applied to every row (`applied[row]` <= steps) and the constants of the last `window` steps in a ring,
 * and brings a row up to date - the skipped steps, in order, each with its own constants, with the dense kernel's operations - before anything reads it:
 *   ntf_n2v_train_batch  the rows the call's windows name (with those of pending apply = 0 calls), before its pairs; an applied step then runs on exactly those rows.
 *                        When `window` steps have been applied since every row was last current, one full flush (every row to the present step) comes first
 *   ntf_n2v_get(what = 0), ntf_n2v_moments   a full flush first: what they return is dense Adam's
 *   ntf_n2v_edge_bce     the endpoints' rows alone when no gradient is pending; a full flush while one is (the pending rows' marks are left alone)
 *   ntf_n2v_get(what = 1), ntf_n2v_walks, ntf_n2v_last_windows   read no table row: nothing is brought up to date
 * A row whose moments are all +0 is unchanged by a zero-gradient step and is not rewritten; a full flush leaves its `applied` where it was (a row no window or
 * edge ever named stays at 0).  Works on both handle kinds (the dummy row of a metapath handle is a row like any other) and with both forms of the pair kernel.
 * ntf_n2v_set_lazy: window 0 = off (plain dense Adam, the default), window >= 1 = on with a ring of that many steps (a full flush every `window` applied steps at
 * the latest; 8 bytes a step).  NTF_EINVAL: window < 0.  NTF_ESTATE: a sparse handle (kind 1), an applied step has been taken, or a gradient is pending -
 * ntf_n2v_set_optimizer's rule; and ntf_n2v_set_optimizer(h, 1) on a lazy handle is NTF_ESTATE.  A refused call changes nothing.  On a lazy handle an applied
 * ntf_n2v_train_batch whose step count would no longer fit the per-row uint32 is refused with NTF_ESTATE.
 * ntf_n2v_lazy_state: reads only and flushes NOTHING: applied [num_nodes] (may be NULL) as the device holds it, *steps = applied steps of the handle, *flushes =
 * full flushes so far (either may be NULL).  NTF_ESTATE on a handle that is not lazy.  It exists so that a test can see rows really being left behind. */
int  ntf_n2v_set_lazy(ntf_n2v* h, int32_t window /* 0 off, >= 1 ring of that many steps */);
int  ntf_n2v_lazy_state(ntf_n2v* h, uint32_t* applied /* [num_nodes] or NULL */, int64_t* steps, int64_t* flushes);
/* node2vec's walk bias: the return parameter p and the in-out parameter q of torch_geometric.nn.Node2Vec (src/mdl/emb/__config__.yaml:69-70), i.e. torch_cluster's
 * random_walk(rowptr, col, start, walk_length, p, q) as published, restated in tests/n2v_bias_reference.py (the package is not installed: that file is the pin).
 * With p == 1 && q == 1 (the default) a handle walks uniformly: k_n2v_walks, its draw slots, its bits - whether the entry was never called, called with (1, 1), or
 * set to something else in between.  With any other pair the walks of ntf_n2v_walks and the positive walks of ntf_n2v_train_batch are the biased walks below;
 * negatives, windows, pairs, both optimisers, ntf_n2v_edge_bce and ntf_n2v_last_windows are untouched, and call t of a handle still draws what ntf_n2v_walks(step = t)
 * draws.  Walks carry no state between calls: the entry may be called at any time and takes no step index.
 * A walk stands on v and came from t (t == v at the start and after a stay).  deg(v) == 0: it stays.  deg(v) == 1: it takes the only neighbour.  Position 1: a
 * uniform neighbour of v.  Later positions with deg(v) >= 2: x is drawn over the ENTRIES of v's CSR row (a repeated id counts once per entry) with probability
 * proportional to 1 / p when x == t (class 0), 1 when t occurs in the CSR row of x (class 1; torch_cluster's is_neighbor(x, t) looks in the row of x), 1 / q otherwise
 * (class 2).  torch_cluster rejects against max(1 / p, 1, 1 / q) without a bound on the attempts; the device rejects NTF_N2V_BIAS_TRIES times and then takes the
 * step by an exact inverse-CDF scan of v's row over the same integer weights (the whole wave scans the row), so the mixture is the same distribution.
 * The draws: thr[k] = (uint64) floor(prob_k * 4294967296.0), prob_0 = (1 / p) / mx, prob_1 = 1 / mx, prob_2 = (1 / q) / mx, mx = max(1 / p, 1, 1 / q), in IEEE
 * double in that order of operations; thr lies in [1, 2^32].  Walk r of call `step` consumes 32-bit words w_0, w_1, ..: w_i is word i & 3 of Philox4x32-10(counter
 * (r lo, r hi, NTF_N2V_BIAS_BASE + (i >> 2), (uint32) step), key n2v_key(seed, step, 0)).  Only steps that draw consume words (no slot per position, unlike the
 * uniform walk).  deg(v) <= 1: no word.  Position 1, deg >= 2: one word u, x = col[a + ((u * deg) >> 32)].  Position >= 2, deg >= 2: per attempt two words u_c, u_a,
 * candidate c = col[a + ((u_c * deg) >> 32)], accepted iff (uint64) u_a < thr[class(c, t)].  After NTF_N2V_BIAS_TRIES rejections two more words u_hi, u_lo (in
 * that order), U = (u_hi << 32) | u_lo, total = sum over the row's entries of thr[class(col[a + j], t)] (< 2^63), target = (U * total) >> 64, x = col[a + j*] for
 * the smallest j* whose inclusive prefix sum exceeds target.  NTF_N2V_BIAS_TRIES is a design constant, not a tolerance.
 * Refused, changing nothing (the bias in force stays; the text is in ntf_n2v_last_error): NTF_EINVAL for a p or q that is not finite or lies outside [1e-4, 1e4]
 * (the range keeps every thr >= 1); NTF_ESTATE on a metapath handle (MetaPath2Vec has no p / q); NTF_EINVAL when some CSR row's neighbour ids are not in ascending
 * order (repeats allowed) - the search for t in the row of x is a binary search; the order is checked on the device once, the first time a pair other than (1, 1)
 * is set, and a handle refused for it goes on working unbiased. */
#define NTF_N2V_BIAS_TRIES 16
#define NTF_N2V_BIAS_BASE  0x42494153u
int  ntf_n2v_set_walk_bias(ntf_n2v* h, double p, double q);

/* ---- metapath2vec skill-embedding producer on the device                                   src/mdl/emb/gnn.py (`m2v` branch of the Gnn plugin, trained by _train_rw)
 * torch_geometric.nn.MetaPath2Vec 2.6.1 as published (restated in tests/m2v_reference.py): after the walks it IS node2vec - the same windows, loss, dense Adam and
 * held-out-edge loss over one table with global row ids - so ntf_m2v_create returns an ntf_n2v handle that carries a metapath, and every ntf_n2v_* entry works on it.
 * Types and rows: n_types node types in TABLE ORDER (PyG sorts the type names), type t owns rows [start[t], start[t] + type_count[t]), start = the running sum,
 * total = sum(type_count); the table is [total + 1, d] (`Embedding(count + 1, d)`), row `total` is the DUMMY row - an ordinary trained row.
 * Metapath: n_hops hops (1 .. NTF_M2V_MAX_HOPS), hop i goes from type hop_src[i] to type hop_dst[i] over its own CSR: hop_rowptr[i] [type_count[hop_src[i]] + 1]
 * int64, hop_col[i] int32 LOCAL ids of type hop_dst[i] (NULL allowed where the hop has no edge).  hop_dst[i] must be hop_src[i + 1].
 * Positive walks (ntf_n2v_walks, ntf_n2v_train_batch): start ids are LOCAL ids of type hop_src[0] in [0, type_count[hop_src[0]]); position 0 is stored as
 * start[hop_src[0]] + local, position s >= 1 as start[hop_dst[(s - 1) % n_hops]] + local, the dummy as `total`.  Step s (1-based) uses hop (s - 1) % n_hops: from a
 * real node of degree deg > 0 the neighbour at index (u * deg) >> 32 of its CSR row; from a node of degree 0, or from the dummy, the dummy (absorbing).  u is word
 * (s - 1) & 3 of Philox4x32-10(counter (r lo, r hi, (s - 1) >> 2, step), key n2v_key(seed, step, 0)), r = the walk's row - node2vec's layout; a dead end or a dummy
 * consumes its draw slot like any step, so position s of walk r always reads the same word.  Row r starts at batch[r % B].
 * Negative walks: start as above, position s >= 1 is start[hop_dst[(s - 1) % n_hops]] + ((u * type_count[that type]) >> 32), never the dummy; u from counter
 * (r lo, r hi, 0x4E454700 + ((s - 1) >> 2), step), key n2v_key(seed, step, 1).
 * walk_length keeps this ABI's meaning, NODES per walk: PyG's MetaPath2Vec counts steps, so a caller passes its walk_length + 1.
 * ntf_n2v_edge_bce, ntf_n2v_get, ntf_n2v_last_windows and injected windows speak GLOBAL row ids and [total + 1, d]; injected windows may name the dummy row.
 * Refused with NTF_EINVAL, before anything is allocated / before the step index is taken, changing nothing: n_types outside 1 .. NTF_M2V_MAX_TYPES, n_hops outside
 * 1 .. NTF_M2V_MAX_HOPS, a type id outside [0, n_types), a negative count, hop_dst[i] != hop_src[i + 1], a rowptr that does not start at 0 or is not monotone, a column
 * outside its destination type, d outside 1 .. 256; at ntf_n2v_train_batch / ntf_n2v_walks: walk_length - 1 > n_hops on a metapath that is not a cycle
 * (hop_dst[n_hops - 1] != hop_src[0]), a start id outside the start type.  The optimiser is the dense Adam of the n2v section, or its sparse Adam
 * after ntf_n2v_set_optimizer(1).
 * The pairs of a metapath handle run through the DUMMY form of the pair kernel (k_n2v_pairs<NV, true>), which sums the terms that land on the dummy row per workgroup before
 * they reach the gradient (same terms, another order of the f32 sums on that one row); the environment variable NTF_M2V_PAIRS=0, read by ntf_m2v_create, keeps node2vec's
 * plain form (k_n2v_pairs<NV, false>) for A/B runs. */
#define NTF_M2V_MAX_TYPES 8
#define NTF_M2V_MAX_HOPS  8
int  ntf_m2v_create(int device, int32_t n_types, const int64_t* type_count /* [n_types], table order */,
                    int32_t n_hops, const int32_t* hop_src, const int32_t* hop_dst /* [n_hops] type ids */,
                    const int64_t* const* hop_rowptr /* [n_hops] -> [type_count[hop_src[i]] + 1] */,
                    const int32_t* const* hop_col    /* [n_hops] -> LOCAL ids of type hop_dst[i] */,
                    int32_t d, const float* init_weight /* [total + 1, d] */, uint64_t seed, ntf_n2v** out);

/* ---- doc2vec team-vector producer on the device                          src/mdl/emb/d2v.py:69-84 (gensim.models.Doc2Vec: build_vocab + train)
 * gensim 4.3.3's PV-DM (dm = 1, mean of doc vector + shrunk-window word vectors) and PV-DBOW with dbow_words = 1 (dm = 0), negative sampling from the
 * count^0.75 table, frequent-word subsampling, 1000-bin sigmoid table, |f| >= 6 skipped - as the reference's call leaves gensim's defaults (oracle/d2v_oracle.py
 * restates the algorithm and lists what is pinned).  The host prepares what gensim's build_vocab prepares: documents as CSR over VOCABULARY indices
 * (doc_ptr [n_docs+1] int64, words int32), sample_int [n_vocab] (keep a word iff sample_int >= a uniform uint32), cum_table [n_vocab] (uint32, last = 2^31 - 1),
 * and the initial vectors (numpy default_rng(seed) / (seed + 7919), so that a seed gives gensim's initial table); syn1neg starts at zero.
 * ntf_d2v_train_epoch = one pass over the documents (gensim train(epochs=1)), taken in `order` (nullable: 0..n_docs-1): the document of rank r trains at
 * alpha_start - (alpha_start - alpha_end) * progress[r] (nullable: r / n_docs) - gensim fixes alpha per job of <= 10 000 words, the host passes the fraction of
 * the pass at which the document's job was cut.  Random draws are Philox words keyed by (seed, epoch) and counted by (document, position, unit, slot).  serial != 0: one wave walks
 * all documents in order - the oracle's sequential pass (parity tests); otherwise one wave per document, Hogwild through f32 atomic adds as gensim's worker threads
 * are through plain stores.  mean_loss (nullable): mean -log sigmoid(+-f) over the pairs trained; device_ms (nullable): device time of the pass.
 * d: any vector size 1..256 (data.embedding.d is free in the reference, its CI trains d = 9): on the device a row is padded to a multiple of 64 floats, the pad
 * stays zero; the host side sees [rows, d] arrays only.
 * ntf_d2v_get / ntf_d2v_set: what = 0 doc vectors [n_docs, d] (= Doc2Vec.dv.vectors, row i = team i), 1 word vectors [n_vocab, d], 2 syn1neg [n_vocab, d]. */
typedef struct ntf_d2v ntf_d2v;
int  ntf_d2v_create(int device, int64_t n_docs, int64_t n_vocab, int32_t d, const int64_t* doc_ptr, const int32_t* words, const uint32_t* sample_int,
                    const uint32_t* cum_table, const float* init_wv, const float* init_dv, uint64_t seed, ntf_d2v** out);
void ntf_d2v_destroy(ntf_d2v* h);
const char* ntf_d2v_last_error(const ntf_d2v* h);
int  ntf_d2v_train_epoch(ntf_d2v* h, int32_t dm, int32_t window, int32_t negative, double alpha_start, double alpha_end, uint64_t epoch, int32_t serial,
                         const int64_t* order, const double* progress, double* mean_loss, double* device_ms);
int  ntf_d2v_get(ntf_d2v* h, int what, float* host);
int  ntf_d2v_set(ntf_d2v* h, int what, const float* host);
/* ntf_d2v_infer: doc vectors of n documents that were NOT in the corpus, against the handle's FROZEN tables                       src/mdl/emb/d2v.py:96-98 (infer_d2v:
 * gensim's Doc2Vec.infer_vector as the reference's call leaves its defaults), batched: one wave per query, one launch, the epoch loop inside the kernel.
 * Queries as CSR over VOCABULARY indices (q_ptr [n+1] int64, q_words int32; the host drops out-of-vocabulary words, as gensim does); ids (nullable: i) = what the
 * random draws of query i are counted by, so a query's vector does not depend on its place in a batch; init / out [n, d] on the host.  For query i:
 *   v = init[i]; a = alpha; delta = (alpha - min_alpha) / max(epochs - 1, 1)   (double)
 *   for e in 0 .. epochs-1, with the Philox key of (seed, e) - the CALL's seed, not the handle's:
 *     kept = the first 10 000 words whose sample_int >= draw(id, raw position, unit 0, KEEP); per kept position pos: b = draw(id, pos, 0, WINDOW) % window,
 *     lo = max(0, pos - window + b), hi = min(K, pos + window + 1 - b);
 *     dm = 1: l1 = (v + sum of wv[kept[m]], m in [lo, hi) \ {pos}) * (1.f / (hi - lo)) in ntf_d2v_train_epoch's order of operations;  dm = 0: l1 = v
 *       (PV-DBOW: infer_vector leaves train_words = False - the window-word units do not run and take no draws);
 *     work = 0; targets kept[pos] (label 1), then `negative` draws (id, pos, unit 0, NEG0 / NEG1) through cum_table, a draw equal to the word skipped:
 *       f = l1 . syn1neg[t], skipped when f <= -6 or f >= 6; work += (label - sigmoid_table(f)) * (float)a * syn1neg[t];   v += work
 *     (syn1neg and the word vectors are NOT updated: learn_hidden = learn_words = False);  a -= delta (successive subtractions in double, gensim's Python loop)
 *   out[i] = v.  A query with no kept word in an epoch skips that epoch; a query of zero words returns init[i] bit for bit.
 * The result is a pure function of (words, id, init row, tables, hyper-parameters, seed): bit-identical under any split of a batch, any position in it, and
 * serial != 0 (one wave walks the queries in order).  No table is written.  The queries and vectors go through buffers the handle keeps and grows (freed by
 * ntf_d2v_destroy).  NTF_EINVAL (message: ntf_d2v_last_error) and `out` untouched for: a NULL handle / q_ptr / q_words / init / out, n < 1, q_ptr[0] != 0 or not
 * monotone, a word index outside [0, n_vocab), window / negative outside what ntf_d2v_train_epoch accepts (window 1..255, dm = 0: 1..127; negative 0..8), dm not
 * 0 or 1, epochs < 1, a non-finite alpha or min_alpha.  device_ms (nullable): device time of the launch. */
int  ntf_d2v_infer(ntf_d2v* h, int64_t n, const int64_t* q_ptr, const int32_t* q_words, const int64_t* ids /* nullable */,
                   int32_t dm, int32_t window, int32_t negative, int32_t epochs, double alpha, double min_alpha, uint64_t seed, int32_t serial,
                   const float* init /* [n, d] host */, float* out /* [n, d] host */, double* device_ms /* nullable */);

/* ---- batched cosine nearest-neighbour search over a resident table                    src/mdl/emb/d2v.py:96-98 (infer_d2v: docvecs.most_similar of the inferred vector)
 * What KeyedVectors.most_similar does one query a call on the host, for a batch, over any [n_rows, d] f32 table (doc2vec's doc vectors, node2vec's embedding.weight):
 * ntf_knn_create uploads the table once (rows padded on the device to a multiple of 32 floats, the pad exact zeros) and computes its reciprocal row norms;
 * ntf_knn_query returns, per query, the topn most similar rows.  [n, n_rows] is never formed.
 * Similarity, all in f32:  sim(i, q) = (dot(i, q) * rq) * rt_i, rounded after each product, where
 *   dot(i, q) = one k-ordered fmaf chain from 0 over k = 0 .. d-1: acc = fmaf(t_i[k], q[k], acc) (what v_mfma_f32_32x32x2_f32 computes; pad columns add exact zeros);
 *   rt_i, rq  = 1.f / sqrtf(n2) (IEEE square root, then IEEE division) of n2 = the k-ordered chain acc = fmaf(v[k], v[k], acc) from 0 over the row's / the query's d values.
 *   A row or query with n2 < FLT_MIN (zero included) has r = 0 and sim exactly +0.0f with everything; -0.0f is returned as +0.0f and ties with it.
 * The bits of sim(i, q) depend on row i's and the query's values alone - not on where either sits in a tile, a range, a group or a batch.
 * Ranking: the topn largest sims of a query first-largest-first; equal sims (compared as f32 values) by ascending row id; out_sims holds the values the ranking used.
 * exclude[q] (exclude nullable; -1: none) is a row id never returned for query q (gensim drops the keys of a most_similar(positive=[key]) call the same way).
 * When fewer than topn rows are eligible the trailing slots hold id -1 and sim -inf.
 * Limits: 1 <= d <= 256, 1 <= n_rows <= 2^31 - 1, 1 <= n, 1 <= topn <= 2048.
 * Memory: beyond the table, its n_rows reciprocal norms and what is per query (the queries, their norms, exclusions, results and one running candidate list of topn
 * 8-byte entries for each query of a group), the device holds only the sims workspace, which never exceeds workspace_bytes (0 = NTF_KNN_WORKSPACE_BYTES).
 * The smallest unit of work is 32 queries x 256 table rows of f32 sims = 32 KiB.  The queries are walked in groups of 32 g, the table in ranges of 256 r rows:
 *   g = min(max(workspace_bytes / 8 MiB, 1), 32, ceil(n / 32));   r = min(workspace_bytes / (gw * 32 KiB), 1024, ceil(n_rows / 256))     (integer divisions)
 * where gw = g rounded up to a multiple of c, and c = 4 (d <= 128 and min(32 g, n) > 64), 2 (min(32 g, n) > 32) or 1 is how many 32-query tiles a workgroup of the sims
 * kernel keeps resident: the workspace is 32 gw x 256 r x 4 bytes <= workspace_bytes (g > 1 only from 16 MiB on, so r >= 1).  The handle keeps no larger workspace from an earlier call.  Per range the sims of the group go to the workspace, each query's topn of the range are selected and merged into its
 * running list by the 64-bit composite (order-preserving key of the sim << 32 | 0x7fffffff - id) - a total order, so the result is bit-identical for every budget.
 * Purity: no table is written; the result of query q is a pure function of (table, query row, topn, exclude[q]): bit-identical under any split or permutation of
 * a batch and under any workspace_bytes.  device_ms (nullable): device time of the sims / selection kernels of the call.
 * NTF_EINVAL (message: ntf_knn_last_error; of a failed create: ntf_knn_last_error(NULL)) with every output untouched for: a null pointer (exclude and device_ms
 * excepted) or a size outside the limits; a non-finite value in the table (create) or in a query; a table row (create) or a query whose f32 n2 overflows; an exclude
 * value outside [-1, n_rows); workspace_bytes negative or below the 32 KiB unit.  No HIP device: NTF_EHIP from create (there is no CPU fallback). */
#define NTF_KNN_WORKSPACE_BYTES ((int64_t)256 << 20)
typedef struct ntf_knn ntf_knn;
int  ntf_knn_create(int device, const float* table /* [n_rows, d] host */, int64_t n_rows, int32_t d, ntf_knn** out);
void ntf_knn_destroy(ntf_knn* h);
const char* ntf_knn_last_error(const ntf_knn* h);
int  ntf_knn_query(ntf_knn* h, const float* queries /* [n, d] host */, int64_t n, int32_t topn, const int64_t* exclude /* [n] nullable */,
                   int64_t workspace_bytes, int32_t* out_idx /* [n, topn] */, float* out_sims /* [n, topn] */, double* device_ms /* nullable */);

/* device generators behind Flipout's eps / signs (dev_out = device pointers), for statistical tests */
int ntf_k_fill_normal(void* stream, uint64_t seed, uint64_t step, int layer, int64_t n, float* dev_out);
int ntf_k_fill_sign(void* stream, uint64_t seed, uint64_t step, int layer, int rows, int cols, float* dev_out);

#ifdef __cplusplus
}
#endif
#endif /* OPENTF_AMD_H */
