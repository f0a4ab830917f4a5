/*
 * chromoformer_hip.h  --  C ABI of libchromoformer_hip.so (MI355X / gfx950).
 *
 * The reference (dohlee/chromoformer) has no native boundary: its hot path is the
 * Python call  model(promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks,
 * interaction_masks, interaction_freq)  ->  loss.backward()  ->  optimizer.step()
 * (chromoformer/train.py:182-196, chromoformer/net.py:332-380).  This header is the
 * boundary a binding for that path uses: plain pointers and sizes, no torch types.
 * Every entry point names the reference interface it replaces.
 *
 * Conventions
 *   - all data pointers are DEVICE pointers unless a comment says "host";
 *   - `stream` is a hipStream_t passed as void*; every call is asynchronous on it and
 *     never allocates (workspace is sized in cf_create for cfg.max_batch genes);
 *   - return value 0 = ok, negative = error; cf_last_error() gives the message;
 *   - a handle is thread-compatible (one thread at a time), handles are independent.
 */
#ifndef CHROMOFORMER_HIP_H
#define CHROMOFORMER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CF_MAX_RES 3
#define CF_ABI_VERSION 1

/* Model / problem description.  Mirrors the constructor arguments of
 * ChromoformerBase (net.py:273-299) and the data-processing keys of
 * configs/default.yaml:9-12 (i_max, w_max / binsizes -> n_bins). */
typedef struct cf_config {
    int n_feats;            /* histone marks per bin (7)                          net.py:276  */
    int d_emb;              /* 128                                                net.py:277  */
    int d_head;             /* 128 (any multiple of 4 <= 1024; != 128: slower head) net.py:278  */
    int n_out;              /* 2 = classifier, 1 = regressor                      net.py:329,427 */
    int n_res;              /* number of resolutions (3)                          net.py:297  */
    int binsizes[CF_MAX_RES];   /* e.g. 2000, 500, 100 (only used for names)               */
    int n_bins[CF_MAX_RES];     /* L_b = w_max / binsize, e.g. 20, 80, 400    data.py:140  */
    int i_max;              /* pCRE slots per gene (8)                            data.py:63  */
    int embed_layers, embed_heads, embed_dmodel, embed_dff;      /* net.py:279-284 */
    int pair_layers, pair_heads, pair_dmodel, pair_dff;          /* net.py:285-290 */
    int reg_layers, reg_heads, reg_dmodel, reg_dff;              /* net.py:291-296 */
    int max_batch;          /* largest B a call will pass                                     */
} cf_config;

/* One entry of the parameter table, in the reference's state_dict() order
 * (net.py:311-330).  `offset` indexes the flat fp32 parameter buffer; the
 * same offset addresses the gradient and the two AdamW moment buffers.  Tensors that
 * never receive a gradient in the reference (w_bias, Embedding/Pairwise gamma_f,
 * Pairwise ln; train.py:157 skips them) have trainable = 0 and live after
 * cf_layout.n_active so that optimiser and all-reduce run on one contiguous range. */
typedef struct cf_param_desc {
    char name[120];
    int ndim;
    int shape[2];
    long long offset;       /* in floats */
    long long numel;
    int trainable;
} cf_param_desc;

typedef struct cf_layout {
    int n_tensors;
    long long n_total;      /* floats in the flat buffer (incl. alignment padding)      */
    long long n_active;     /* floats [0, n_active) hold every trainable tensor          */
    long long n_elems;      /* sum of numel (5,342,672 for the default config)           */
} cf_layout;

/* One batch, reference layout (net.py:332-340; produced by data.py:124-212).
 * Masks are the reference's bool tensors viewed as bytes (non-zero = masked).  Only
 * the centre query row of the two pad masks is ever consumed, so
 * they are passed as "row pointers": element (sequence n, key bin j) is read at
 *     mask[n * stride + j].
 * For the reference's [B,1,1,L,L] / [B,S,1,L,L] tensors pass  ptr + (L/2)*L  and
 * stride = L*L (zero-copy); a compact [B(,S),L] row array uses stride = L. */
typedef struct cf_batch {
    int B;
    const float*   promoter_feats[CF_MAX_RES];      /* [B,1,L,F]  fp32                 */
    const float*   pcre_feats[CF_MAX_RES];          /* [B,S,L,F]  fp32                 */
    const uint8_t* promoter_mask_row[CF_MAX_RES];   /* see above; n = gene            */
    long long      promoter_mask_stride[CF_MAX_RES];
    const uint8_t* pcre_mask_row[CF_MAX_RES];       /* n = gene * S + slot            */
    long long      pcre_mask_stride[CF_MAX_RES];
    const uint8_t* interaction_mask[CF_MAX_RES];    /* [B,1,T,T]  T = i_max + 1       */
    const float*   interaction_freq;                /* [B,T,T]                        */
} cf_batch;

typedef struct cf_handle cf_handle;

/* ---- host-only helpers (no GPU needed) ------------------------------------------ */
int         cf_abi_version(void);
const char* cf_last_error(void);
/* Parameter table for a config: fills `layout`, writes up to `cap` entries into `table`
 * (may be NULL to query the count).  Replaces walking model.state_dict(). */
int cf_param_layout(const cf_config* cfg, cf_layout* layout, cf_param_desc* table, int cap);

/* ---- lifetime --------------------------------------------------------------------- */
/* Replaces Model(...).cuda() (train.py:142-154): allocates the workspace for
 * cfg.max_batch genes and the positional tables (net.py:23-29) which the caller supplies
 * from host memory: pe[r] is float[n_bins[r] * d_emb], row-major, same values the
 * reference adds at net.py:47-53 / :124-130. */
int  cf_create(const cf_config* cfg, const float* const* pe_host, cf_handle** out);
void cf_destroy(cf_handle* h);
/* Flat fp32 buffers owned by the caller (cf_layout.n_total floats each).  grads / m / v
 * may be NULL for inference-only use.  Replaces model.parameters() / optimizer state. */
int cf_bind(cf_handle* h, float* params, float* grads, float* exp_avg, float* exp_avg_sq);

/* ---- hot path ------------------------------------------------------------------- */
/* ChromoformerBase.forward (net.py:332-380).  logits: [B, n_out].  save_for_backward: 0 = inference only; 1 = keep what
 * cf_backward needs; 2 = as 1, and the prediction head (net.py:377-380) is LEFT to the cf_backward / cf_backward_part(parts & 1)
 * call that must follow with labels: head forward, loss and head backward then run as one launch, and `logits` (which has to
 * stay valid until then) is written by that call -- the training step of a caller that does not need the logits in between. */
int cf_forward(cf_handle* h, const cf_batch* batch, float* logits, int save_for_backward, void* stream);
/* cf_forward(save_for_backward = 2) for a training step whose labels are known at forward time (train.py:182-193: they always are).
 * Where cf_head_rides(h) -- the 512-thread Regulation kernels, three resolutions, d_head = 128 -- the prediction head (net.py:377-380),
 * the loss (train.py:156) and the head's backward run at the TAIL of the Regulation forward launch, on the last of a gene's three
 * workgroups to finish, instead of in a launch of their own; the cf_backward_part / cf_backward call that follows skips the head
 * (its labels / loss arguments are ignored).  Elsewhere identical to cf_forward(..., 2, ...).  logits / loss_out may be null. */
int cf_forward_train(cf_handle* h, const cf_batch* batch, float* logits, const void* labels, float loss_scale,
                     float* loss_out, void* stream);
int cf_head_rides(cf_handle* h);
/* criterion(out, label) + loss.backward() (train.py:156, 193-195).  labels: int64 [B]
 * (n_out = 2, CrossEntropyLoss) or float [B] (n_out = 1, MSELoss).  `loss_scale`
 * multiplies the mean-over-B loss gradient (1.0 single GPU; 1/world for an all-reduce SUM).
 * Writes the scalar loss to loss_out (device, 1 float) and every trainable gradient into
 * the bound grads buffer (overwrites; nothing accumulates across calls).  Must follow a
 * cf_forward(..., save_for_backward = 1 or 2) on the same batch. */
int cf_backward(cf_handle* h, const cf_batch* batch, const void* labels, float loss_scale,
                float* loss_out, void* stream);
/* The two halves of cf_backward, for callers that replay the first as a hipGraph:
 *   cf_backward_chain  -- loss + the activation-gradient chain (head -> Regulation ->
 *                         Pairwise -> Embedding); every dY a weight gradient needs is left
 *                         in the workspace;
 *   cf_backward_reduce -- the deferred reductions: all weight gradients (dW = dY^T X, one
 *                         launch over a tile table) and all bias / LayerNorm / gamma_f
 *                         gradients (one launch). */
int cf_backward_chain(cf_handle* h, const cf_batch* batch, const void* labels, float loss_scale,
                      float* loss_out, void* stream);
int cf_backward_reduce(cf_handle* h, int B, void* stream);
/* Gradient buckets.  The trainable parameters lie in state_dict order in the flat buffers, so the model splits
 * into two adjacent ranges: CF_BUCKET_PE = Embedding + Pairwise stacks, [0, split), whose gradients exist only
 * after the whole backward chain, and CF_BUCKET_REG = Regulation stacks + fc_head, [split, n_active), 78 % of the
 * bytes, whose gradients can be reduced as soon as piece 2 of cf_backward_part has run.  A data-parallel caller
 * reduces + all-reduces (+ steps) CF_BUCKET_REG on a second stream while piece 4 still runs on the first.
 *   cf_grad_bucket          -- the flat range (in floats) of one bucket;
 *   cf_backward_reduce_part -- cf_backward_reduce restricted to a bucket mask. */
#define CF_BUCKET_REG 1
#define CF_BUCKET_PE 2
/* Round 5: the Regulation bucket in two halves, for a data-parallel caller that wants bytes on the wire while the backward pass still runs.
 * Trainable tensors lie [Embedding | Pairwise | Regulation layers below n_layers / 2 (every resolution) | the layers from there up | fc_head]
 * in the flat buffers (cf_param_layout reports every offset; the state_dict order of the table is unchanged):
 *   CF_BUCKET_REG_HI = upper Regulation layers + fc_head -- complete after cf_backward_part(parts = 1 | CF_PART_REG_HI);
 *   CF_BUCKET_REG_LO = lower Regulation layers           -- complete after cf_backward_part(parts = CF_PART_REG_LO);
 *   CF_BUCKET_REG    = both (one adjacent range), as before.
 * cf_reg_halves(h) returns the first layer of the upper half when the model's Regulation backward can run as two launches (the fused
 * kernels, two layers or more), else 0: then only CF_BUCKET_REG / parts = 2 exist. */
#define CF_BUCKET_REG_HI 4
#define CF_BUCKET_REG_LO 8
#define CF_PART_REG_HI 8
#define CF_PART_REG_LO 16
int cf_reg_halves(cf_handle* h);
int cf_grad_bucket(cf_handle* h, int bucket, long long* offset, long long* numel);
int cf_backward_reduce_part(cf_handle* h, int B, int buckets, void* stream);
/* cf_backward_chain in pieces (bit mask `parts`: 1 = loss + head, 2 = Regulation stack, 4 = Pairwise +
 * Embedding), so that a caller replaying graphs can launch one piece eagerly between two graphs (bench.py times
 * the Regulation backward kernel with HIP events that way).  Pieces must run in the order 1, 2, 4. */
int cf_backward_part(cf_handle* h, const cf_batch* batch, const void* labels, float loss_scale,
                     float* loss_out, int parts, void* stream);
/* Same, but from a caller-supplied d(loss)/d(logits) [B, n_out]. */
int cf_backward_from(cf_handle* h, const cf_batch* batch, const float* dlogits, void* stream);
/* Gradients of the float inputs (saliency maps), device buffers; a NULL field is not wanted. */
typedef struct cf_input_grads {
    float* promoter_feats[CF_MAX_RES];   /* [B, n_bins[r], n_feats]        */
    float* pcre_feats[CF_MAX_RES];       /* [B, i_max, n_bins[r], n_feats] */
    float* interaction_freq;             /* [B, T, T], T = i_max + 1       */
} cf_input_grads;
/* cf_backward_from (same preconditions, bit-identical parameter gradients) that also OVERWRITES every requested input
 * gradient in full, with zeros where the reference's autograd gives zeros: masked bins of a pad row that has a valid bin,
 * interaction entries masked at every resolution, pCRE slots no unmasked interaction entry reaches (the dataset's dummy
 * slots).  A fully padded slot whose token IS visible has a uniform softmax row and non-zero gradients.  want == NULL or all
 * fields NULL: exactly the launches of cf_backward_from.  Deterministic (no atomics).  promoter_feats needs
 * embed.n_layers = 1; a configuration the kernels do not cover fails before anything is launched. */
int cf_backward_from_inputs(cf_handle* h, const cf_batch* batch, const float* dlogits, const cf_input_grads* want,
                            void* stream);
/* Attention maps and the regulatory embedding (interpretation), device buffers; a NULL field is not wanted.  T = i_max + 1. */
typedef struct cf_attn_maps {
    float* embed[CF_MAX_RES];       /* [B, embed.n_heads, n_bins[r]]: the centre query's row of the Embedding layer      */
    float* pairwise[CF_MAX_RES];    /* [B, pw.n_layers, i_max, pw.n_heads, n_bins[r]]: the promoter centre row per pCRE  */
    float* regulation[CF_MAX_RES];  /* [B, reg.n_layers, reg.n_heads, T]: row 0 (the promoter token) per layer           */
    float* embedding;               /* [B, n_res * d_emb]: the fc_head input, cat(x_out[r][:, 0]) + cat(x_in[r][:, 0])   */
} cf_attn_maps;
/* cf_forward(save_for_backward = 1) (same launches, logits, saved activations) followed by ONE launch that OVERWRITES every
 * requested output in full with the softmax probabilities the forward used (bit-equal: copies, no arithmetic; masked keys 0,
 * fully masked rows uniform) and the fc_head input.  want == NULL or all fields NULL: exactly the launches of cf_forward(save = 1).
 * Deterministic (no atomics).  embed needs embed.n_layers = 1; a resolution index >= n_res fails; both before anything is launched. */
int cf_attention_maps(cf_handle* h, const cf_batch* batch, float* logits, const cf_attn_maps* want, void* stream);
/* In-silico pCRE deletion (interpretation).  logits: [B, V, n_out], V = i_max + 2, gene-major (b * V + v): the inference forward of
 * gene b with its Regulation interaction mask (every resolution) replaced by
 *   v = 0           the given mask (baseline: bit-equal to cf_forward(save = 0));
 *   v = 1 + j       the given mask OR row j+1 OR column j+1 (pCRE slot j deleted; a slot that is already a dummy gives the baseline);
 *   v = i_max + 1   the given mask OR rows and columns 1..i_max (promoter only).
 * Features, pad masks and interaction_freq are gene b's.  Launches: the trunk part of cf_forward(save = 0) (prologue, Embedding +
 * Pairwise) once, k_pcre_stash once (the Regulation input), then per chunk of at most max_batch gene-variants one k_coalition_expand
 * (the variants are the coalition words 2^i_max - 1, that word without bit j, 0 of cf_pcre_coalitions below, in a device table written
 * when the buffers are allocated: no copy per call) and the Regulation + head launches of cf_forward(save = 0) on that chunk:
 *   cf_launch_counts fwd = n_trunk + 1 + ceil(B * V / max_batch) * (1 + n_reg_head),
 * where n_trunk + n_reg_head is what cf_forward(save = 0) issues (n_reg_head: 2 on the fused Regulation shapes -- k_reg_fwd, the
 * head --, 3 * reg.n_layers + 1 layer by layer).  Overwrites the activations a cf_forward(save >= 1) kept: no cf_backward* may
 * follow without a new saving forward.  Deterministic (no atomics).  The first call allocates the stash and chunk buffers (freed by
 * cf_destroy; ~1 MB at max_batch 64) and writes the table with a blocking copy: it synchronises, whichever of cf_pcre_ablation and
 * the coalition entry points comes first; later calls allocate nothing.  A null handle / batch / logits or B > max_batch fails by name,
 * before anything is launched. */
int cf_pcre_ablation(cf_handle* h, const cf_batch* batch, float* logits, void* stream);
/* pCRE coalition forwards, exact Shapley values and pair epistasis (interpretation).  S = i_max.  A coalition is a 32-bit word m: bit
 * j set = pCRE slot j kept.  Row (b, m) is the inference forward of gene b with its Regulation interaction mask (every resolution)
 * replaced by the given mask OR row j+1 OR column j+1 for every j < S whose bit is clear; features, pad masks and interaction_freq
 * are gene b's.  So m = 2^S - 1 is variant 0 of cf_pcre_ablation (the prediction), one clear bit j its variant 1 + j, m = 0 its
 * variant S + 1 (the promoter alone), bit for bit; a bit of a slot that is already a dummy changes nothing.
 * cf_pcre_coalitions: keep is a HOST array of n_coal words (read before the call returns); logits [B, n_coal, n_out], gene-major
 * (b * n_coal + c).  Launches: the trunk part of cf_forward(save = 0) once, k_pcre_stash once, then per chunk of at most max_batch
 * rows one k_coalition_expand and the Regulation + head launches of cf_forward(save = 0) on that chunk:
 *   cf_launch_counts fwd = n_trunk + 1 + ceil(B * n_coal / max_batch) * (1 + n_reg_head)      (n_trunk, n_reg_head: see cf_pcre_ablation)
 * The words travel in a device table the handle owns (grown on demand); the stash and chunk buffers are those of cf_pcre_ablation
 * (whichever call comes first allocates them; cf_destroy frees them).  Overwrites the activations a cf_forward(save >= 1) kept: no
 * cf_backward* may follow without a new saving forward.  Parameters, gradients and moments are untouched.  Deterministic (no
 * atomics); the result does not depend on max_batch.  Refused by name, before anything is launched: a null handle / batch / logits,
 * B > max_batch, n_coal < 1, a null keep, a word with a bit >= i_max set. */
int cf_pcre_coalitions(cf_handle* h, const cf_batch* batch, const uint32_t* keep, int n_coal, float* logits, void* stream);
/* Exact Shapley values of the pCRE slots: all 2^S coalitions through the routine above (word m at column m), then one k_shapley:
 *   phi[b, j, o] = sum over m with bit j clear of w(|m|) (v[b, m | 1 << j, o] - v[b, m, o]),   w(k) = k! (S - k - 1)! / S!
 * with the S weights computed on the host in double and rounded to fp32, every device operation rounded to fp32, in a fixed order
 * (per thread an ascending stride of the words, then a fixed tree).  phi [B, S, n_out].  All S slots are players; a dummy slot is a
 * null player (phi exactly 0), which leaves the live slots' values those of the game among the live slots.  Efficiency:
 * sum_j phi[b, j] = v[b, 2^S - 1] - v[b, 0] up to rounding.  logits_all: [B, 2^S, n_out], or NULL: the rows go to a buffer the handle
 * owns (allocated by the first such call for max_batch genes, freed by cf_destroy).  fwd = that of cf_pcre_coalitions with
 * n_coal = 2^S, plus 1.  Accepted for every i_max (65,536 rows per gene at 16).  Refusals as above (null phi). */
int cf_pcre_shapley(cf_handle* h, const cf_batch* batch, float* phi, float* logits_all, void* stream);
/* Pair-deletion epistasis.  With N = 2^S - 1 the rows are: 0: N; 1 + i: N without i; then N without i and j for the pairs i < j in
 * lexicographic order (1 + S + S (S - 1) / 2 rows), through the routine above, then one k_epistasis:
 *   eps[b, i, j, o] = ((v_N - v_{N\i}) - v_{N\j}) + v_{N\{i,j}}   for i < j, every operation rounded to fp32 (no contraction);
 *   eps[b, j, i] carries the bits of eps[b, i, j];  eps[b, i, i] = v_N - v_{N\i}.
 * eps [B, S, S, n_out]; rows and columns of dummy slots are exactly 0.  logits_pairs: [B, 1 + S + S (S - 1) / 2, n_out], or NULL (a
 * handle-owned buffer, as above).  fwd = that of cf_pcre_coalitions with that n_coal, plus 1.  Refusals as above (null eps). */
int cf_pcre_epistasis(cf_handle* h, const cf_batch* batch, float* eps, float* logits_pairs, void* stream);
/* Pairwise Shapley interaction indices of the players of an exact game (interpretation): a second reduction of the [B, 2^P, n_out]
 * table the Shapley entry points reduce with k_shapley (word m at column m).  For players i != j, S running over the coalitions that
 * hold neither, per output column:
 *   delta_ij(S)    = (v(S + i + j) - v(S + j)) - (v(S + i) - v(S))      i's marginal contribution with j present, minus that with j absent
 *   inter[b, i, j] = sum_S w(|S|) delta_ij(S)
 * `index` selects the weight table alone (computed on the host in double, rounded to fp32, passed by value):
 *   CF_INTERACTION_SII  w(s) = s! (P - s - 2)! / (P - 1)!    the Shapley interaction index; inter[b, i, i] = phi[b, i], the bits of k_shapley
 *   CF_INTERACTION_STI  w(s) = (2 / P) / C(P - 1, s)         Shapley-Taylor, order 2; inter[b, i, i] = v({i}) - v(0), one fp32 subtraction,
 *                                                            and sum_i inter[i, i] + sum_{i<j} inter[i, j] = v(N) - v(0) up to rounding
 * One k_shapley_pairs: a workgroup per (gene, pair i <= j), every operation rounded to fp32 (no contraction) in the grouping written
 * above, a thread's subsets in ascending stride, then a fixed tree: deterministic, no atomics; inter[b, j, i] carries the bits of
 * inter[b, i, j].  The grouping is part of the definition: delta is exactly 0 when either player is null (its rows bit-equal present
 * and absent), so a null player's row and column are exact zeros; at P = 2 the off-diagonal entry agrees with *_epistasis within
 * rounding, not bit for bit (k_epistasis groups differently).  inter [B, P, P, n_out].
 * cf_shapley_interactions_from_rows: the operator on a caller's device table rows [B, 2^P, n_out] (for instance a kept logits_all): no
 * batch, no workspace, no activation is touched; n_out is the handle's.  cf_launch_counts fwd = 1.  Refused by name, before anything is
 * launched: a null handle / rows / inter, B < 1, P outside 2..16, an index other than the two constants. */
#define CF_INTERACTION_SII 0
#define CF_INTERACTION_STI 1
int cf_shapley_interactions_from_rows(cf_handle* h, const float* rows, int B, int P, int index, float* inter, void* stream);
/* Harsanyi dividends (the Moebius transform) of the same table, and interaction indices of any order from them (interpretation).
 *   m(S) = sum over T <= S of (-1)^(|S| - |T|) v(T),      v(S) = sum over T <= S of m(T):      one number per set of players.
 * cf_dividends_from_rows: rows, div and the optional mass [B, 2^P, n_out] (device; word m at column m; n_out is the handle's),
 * 1 <= P <= 16.  The fp32 result is DEFINED by the in-place recurrence
 *   for k = 0 .. P - 1, for every word S with bit k set:  a[S] = a[S] - a[S ^ (1 << k)]       one fp32 subtraction each
 * so it equals a float32 restatement bit for bit: div[0] = v(0), div[{i}] = v({i}) - v(0) (the sti diagonal of k_shapley_pairs),
 * div[{i, j}] = (v(ij) - v(j)) - (v(i) - v(0)) for i < j (its delta_ij(0)), and every dividend of a set that holds a null player (rows
 * bit-equal with and without it, finite) is exactly +0.  mass(S) = sum over T <= S of |v(T)| is the same butterfly with + on |v|: the
 * scale of the rounding error, |div(S) - exact| <= ((1 + 2^-24)^|S| - 1) mass(S).  k_moebius (tiles of 4,096 words in LDS, stages
 * 0..11) and, for P > 12, k_moebius_high (the remaining stages in registers, in place): cf_launch_counts fwd = 1 for P <= 12, 2 above,
 * with or without mass.  rows may not alias div or mass.  Refused by name, before anything is launched: a null handle / rows / div,
 * B < 1, P outside 1..16.
 * cf_set_interactions_from_dividends: sets is a HOST array of n_sets words (read before the call returns; they travel in the
 * handle's word table), each with 1 <= |S| <= order;  out[b, s, o] = sum over U >= S_s of wt[|S_s|][|U|] div[b, U, o], the weights
 * computed in double, rounded to fp32 and passed by value:
 *   CF_INTERACTION_SII  wt = 1 / (|U| - |S| + 1)        order 1: the Shapley value; order 2: the pairwise sii
 *   CF_INTERACTION_STI  |S| < order: the dividend itself (its bits, no arithmetic); |S| = order: wt = 1 / C(|U|, order); the sum over
 *                       all non-empty sets of size <= order is v(N) - v(0) up to rounding
 * One k_set_index, a workgroup per (gene, set): a thread sums its supersets in ascending stride, one rounded product and one rounded
 * add per term (no contraction), then k_shapley's tree: deterministic; a set that holds a null player is exactly 0.  out
 * [B, n_sets, n_out].  fwd = 1.  Both are operators as cf_shapley_interactions_from_rows: no batch, no activation is touched, a
 * pending backward is left alone.  Refused by name, before anything is launched: a null handle / div / sets / out, B < 1, P outside
 * 1..16, n_sets outside 1..65535, order outside 1..P, an index other than the two constants, the empty set, a set word with a bit
 * >= P or more than `order` bits (the error names the set's position). */
int cf_dividends_from_rows(cf_handle* h, const float* rows, int B, int P, float* div, float* mass /* or NULL */, void* stream);
int cf_set_interactions_from_dividends(cf_handle* h, const float* div, int B, int P, const uint32_t* sets /* host */, int n_sets, int index,
                                       int order, float* out /* [B, n_sets, n_out] */, void* stream);
/* cf_pcre_shapley's rows (S = i_max players, all 2^S coalitions through the same routine, logits_all as there), then k_shapley_pairs;
 * phi [B, S, n_out] is optional: if given, k_shapley runs on the same rows too.  fwd = that of cf_pcre_coalitions with n_coal = 2^S, plus
 * 1 per reducer launched (1, or 2 with phi).  Refused by name, before anything is launched: what cf_pcre_shapley refuses (phi may be
 * null), a null inter, an index other than the two constants, i_max < 2. */
int cf_pcre_shapley_interactions(cf_handle* h, const cf_batch* batch, int index, float* inter, float* phi, float* logits_all, void* stream);
/* Contact games (interpretation): coalition forwards whose players delete pCRE slots and / or edit the promoter-pCRE contact frequencies
 * -- does an enhancer matter through its chromatin state or through its contact with the promoter?  A player p has two 32-bit words over
 * the pCRE slots (HOST arrays of n_players words, read before the call returns): bit j of player_drop[p] set = slot j is deleted while p
 * is absent; bit j of player_contact[p] set = slot j's contact is edited while p is absent.  Players may overlap.  A coalition is one
 * word, bit p set = player p PRESENT.  Row (b, m), with D the OR of player_drop and C the OR of player_contact over the absent players,
 * is the inference forward of gene b with
 *   deletion      for every j in D: row and column j + 1 of the interaction mask set at every resolution (the rule of cf_pcre_coalitions);
 *   contact edit  entry (q, k) of interaction_freq[b] edited when token q or token k is j + 1 for some j in C -- token 0, the promoter, is
 *                 never named; row and column both, mirroring the mask rule (the kernels read all T x T entries) --, once per entry:
 *                   donor_freq == NULL   scale * f, one fp32 multiplication: 0 erases, 2 doubles, 1 is a bit-exact no-op, any finite
 *                                        value is accepted (the bias is signed);
 *                   donor_freq != NULL   donor_freq[b, q, k]: a device [B, T, T] fp32 tensor, the same genes' frequencies in another
 *                                        cell type or a hypothetical contact map (scale is not read);
 *   everything else gene b's own.  The full word 2^P - 1 is the prediction, bit-equal to cf_forward(save = 0).
 * Three facts hold bit for bit: a game whose players only drop is the pCRE game (the rows of cf_pcre_coalitions on the complementary
 * masks); a masked score is replaced, not biased, so next to an absent player that drops slot j a player that edits slot j's contact is
 * null (every Harsanyi dividend of a set holding `contact j` without `pcre j` is exactly 0); a dummy slot, scale = 1 and a donor_freq
 * equal to the batch's own are null players.
 * Launches: those of cf_pcre_coalitions with k_contact_expand in place of k_coalition_expand -- the trunk once, k_pcre_stash once, per
 * chunk of at most max_batch rows one k_contact_expand (workgroup per chunk row and resolution; every output element written once, no
 * atomics) and the Regulation + head launches:
 *   cf_launch_counts fwd = n_trunk + 1 + ceil(B * n_coal / max_batch) * (1 + n_reg_head), plus 1 per reducer.
 * The coalition words and the 2 * n_players player words travel in the handle's word table; stash, chunk buffers and the handle-owned
 * row buffer are those of cf_pcre_ablation / cf_pcre_shapley: no other allocation.  Overwrites the activations a cf_forward(save >= 1)
 * kept.  Deterministic; the result does not depend on max_batch.
 * cf_contact_coalitions: keep is a HOST array of n_coal words; logits [B, n_coal, n_out], gene-major.
 * cf_contact_shapley: all 2^P coalitions (word m at column m), then k_shapley: phi [B, P, n_out]; logits_all [B, 2^P, n_out] or NULL
 * (the handle-owned buffer).  cf_contact_epistasis: the pair-deletion rows of cf_pcre_epistasis on the P players, then k_epistasis: eps
 * [B, P, P, n_out]; logits_pairs [B, 1 + P + P (P - 1) / 2, n_out] or NULL.  cf_contact_shapley_interactions: the 2^P rows, then
 * k_shapley_pairs (and k_shapley if phi is given), index as in cf_shapley_interactions_from_rows.  Dividends, set indices and
 * back-selection: the *_from_rows operators on a kept table.
 * Refused by name, before anything is launched: a null handle / batch / opts / output, B > max_batch, n_players outside 1..16, null
 * player arrays, a player with both words 0, a player bit >= i_max, a non-finite scale, n_coal < 1, a null keep, a keep word naming a
 * player >= n_players, fewer than 2 players for cf_contact_epistasis and cf_contact_shapley_interactions, an index other than the two
 * constants. */
typedef struct cf_contact_opts {
    int n_players;                   /* 1..16 */
    const uint32_t* player_drop;     /* host [n_players]: bit j = pCRE slot j deleted while the player is absent */
    const uint32_t* player_contact;  /* host [n_players]: bit j = pCRE slot j's contact edited while the player is absent */
    float scale;                     /* the scale rule (donor_freq == NULL) */
    const float* donor_freq;         /* device [B, T, T], or NULL */
} cf_contact_opts;
int cf_contact_coalitions(cf_handle* h, const cf_batch* batch, const cf_contact_opts* opts, const uint32_t* keep, int n_coal, float* logits,
                          void* stream);
int cf_contact_shapley(cf_handle* h, const cf_batch* batch, const cf_contact_opts* opts, float* phi, float* logits_all, void* stream);
int cf_contact_epistasis(cf_handle* h, const cf_batch* batch, const cf_contact_opts* opts, float* eps, float* logits_pairs, void* stream);
int cf_contact_shapley_interactions(cf_handle* h, const cf_batch* batch, const cf_contact_opts* opts, int index, float* inter, float* phi,
                                    float* logits_all, void* stream);
/* Integrated gradients (interpretation).  For the target logit column t, nodes a_k and weights w_k (k < n_steps) on [0, 1], per
 * interpolated input x with baseline xb (T = i_max + 1):
 *   x_k   = xb + a_k (x - xb)                         fp32, each operation rounded
 *   g_k   = d(w_k logits[:, t]) / d x_k               (the backward from dlogits = w_k at column t, 0 elsewhere)
 *   attr  = (x - xb) ((g_0 + g_1) + ... + g_{n-1})    fp32, in k order
 *   delta = sum(attr over every interpolated element) - (F(x)[t] - F(xb)[t])        per gene
 * `interpolate` selects the inputs: bit 0 promoter_feats, bit 1 pcre_feats, bit 2 interaction_freq (every resolution); the others and
 * every mask stay at the given batch.  The outputs of `out` must be exactly those of the interpolated inputs (every resolution);
 * each is OVERWRITTEN in full, in the layout of cf_input_grads: zeros for padded bins, dummy slots, masked interaction entries.
 * logits_x / logits_base [B, n_out]: the forward of x / of xb; delta [B]. */
#define CF_IG_PROMOTER 1
#define CF_IG_PCRE 2
#define CF_IG_FREQ 4
typedef struct cf_ig_opts {
    int n_steps, target, interpolate;
    const float* alphas;             /* host [n_steps]: nodes a_k (read before the call returns)   */
    const float* weights;            /* host [n_steps]: weights w_k                                */
    const float* base_promoter_feats[CF_MAX_RES];   /* device baselines, layout of the inputs; NULL: zeros */
    const float* base_pcre_feats[CF_MAX_RES];
    const float* base_interaction_freq;
    int base_broadcast;              /* 1: the baselines hold one gene, used for every gene                              */
} cf_ig_opts;
/* Rows are (gene, variant) pairs, gene-major, V = n_steps + 2 per gene (x, xb, then x_0 .. x_{n-1}), processed in chunks of at most
 * max_batch rows.  Per chunk: k_ig_expand (the rows' inputs, masks and dlogits into buffers the first call allocates), the launches
 * of cf_forward(save = 1) and of the backward chain with the input-gradient launches of cf_backward_from_inputs -- but no gradient
 * reduction: the bound gradient buffer, the moments and the parameters are left as they were -- then k_ig_accumulate; k_ig_delta
 * once at the end.  When only interaction_freq is interpolated the trunk runs once, its output is stashed, and the chunks run the
 * Regulation + head forward and backward only (bit-equal to the general path, which CF_IG_TRUNK_ONCE=0 at cf_create selects).
 * Deterministic (no atomics, fixed order).  Where the gene-batched attention kernel k_attc2 runs (configurations off the fused
 * trunk: i_max > 8, embed.n_layers > 1, head counts other than 2), its regions per workgroup follow the number of sequences in the
 * launch; the chunks take the count cf_forward would take for the B genes of the batch.  So the result does not depend on max_batch
 * and equals cf_forward(save = 1) + cf_backward_from_inputs on the batch, per node, bit for bit.
 * Overwrites the activations a cf_forward(save >= 1) kept: no cf_backward* may follow without a new saving forward.
 * Refused by name, before anything is launched: a null argument, n_steps < 1, target outside [0, n_out), B > max_batch, an output
 * that does not match `interpolate` or names a resolution >= n_res, promoter_feats with embed.n_layers > 1, no bound gradient
 * buffer (its workspace), armed riders. */
int cf_integrated_gradients(cf_handle* h, const cf_batch* batch, const cf_ig_opts* opts, const cf_input_grads* out,
                            float* logits_x, float* logits_base, float* delta, void* stream);
/* Integrated gradients in raw-signal space, zero-signal baseline (interpretation).  The feature inputs hold u = log(1 + m), m >= 0
 * the mean of a bin of the raw signal x.  The path is x(a) = a x: linear in the bin means, curved in the features.  Same cf_ig_opts,
 * rows, chunks, buffers and launches as cf_integrated_gradients, with k_ig_expand_raw / k_ig_accumulate_raw in place of k_ig_expand /
 * k_ig_accumulate.  Per element of an interpolated feature input, with m = expm1f(u):
 *   u_k   = log1pf(a_k m)                              the row of node k (fp32, each operation rounded); F(0) runs on zeros
 *   g_k   = d(w_k logits[:, t]) / d u_k
 *   C     = (g_0 / (1 + a_0 m) + g_1 / (1 + a_1 m)) + ...   fp32, in k order
 *   attr  = m C           -> out:   integrated gradients with respect to the bin MEAN; complete: the attr of a gene (plus those of
 *                                   interaction_freq, which keeps its straight path and baseline when its bit is set) sum to
 *                                   F(x)[t] - F(0)[t] up to the quadrature error; delta is that sum minus the difference
 *   coeff = (1 + m) C     -> coeff: dfeat for cf_bin_regions_multi_backward(times_input = 1), which divides by cnt (1 + m) and
 *                                   multiplies by the sample: IG_raw[f, s] = x[f, s] sum_r C_r[p_r(s), f] / cnt, every bin's attr
 *                                   spread over its samples in proportion to x
 * `coeff` may be NULL, or have any of the feature fields of the interpolated inputs set (each OVERWRITTEN in full; exact zeros for
 * padded bins and dummy slots, as in `out`).  Limits: the zero-signal baseline only (a donor cell type's signal as the baseline:
 * cf_integrated_gradients_raw_donor below); u < ~80 (expm1f overflows past 88); 1 + a m <= 0
 * gives inf / NaN as the forward's log does.  Deterministic; the result does not depend on max_batch.
 * Refused by name, before anything is launched: everything cf_integrated_gradients refuses; a non-NULL base_promoter_feats /
 * base_pcre_feats; an `interpolate` without CF_IG_PROMOTER or CF_IG_PCRE; a coeff field set for an input that is not interpolated;
 * a non-NULL coeff->interaction_freq. */
int cf_integrated_gradients_raw(cf_handle* h, const cf_batch* batch, const cf_ig_opts* opts, const cf_input_grads* out,
                                const cf_input_grads* coeff, float* logits_x, float* logits_base, float* delta, void* stream);
/* Integrated gradients in raw-signal space against a donor cell type (interpretation).  The path is x(a) = xd + a (x - xd) between two
 * raw signals over the same regions; binning is linear, so a bin with means m (gene) and md (donor) has the mean md + a (m - md) along
 * it.  The donor's binned features ud = log(1 + md) travel in opts->base_promoter_feats / base_pcre_feats ([B, ...], the layout of
 * the inputs, one row per gene).  Rows, chunks, buffers and launches of cf_integrated_gradients_raw, with k_ig_expand_raw_donor /
 * k_ig_accumulate_raw_donor.  Per element of an interpolated feature input, fp32, each operation rounded:
 *   m = expm1f(u)   md = expm1f(ud)   d = m - md   mk = md + a_k d
 *   u_k   = log1pf(mk)                                 the row of node k; F(x) runs on u verbatim, F(xd) on ud verbatim
 *   g_k   = d(w_k logits[:, t]) / d u_k
 *   C     = (g_0 / (1 + mk_0) + g_1 / (1 + mk_1)) + ...     in k order
 *   attr  = d C           -> out:   complete: the attr of a gene (plus those of interaction_freq, which keeps its straight path and
 *                                   baseline) sum to F(x)[t] - F(xd)[t] up to the quadrature error; delta is that sum minus the difference
 *   cmean = C             -> cmean: per bin, what cf_bin_spread_difference spreads over the difference of the two raw signals
 * logits_base is the donor's features under the batch's masks and frequencies.  An element with the same bits in both cell types
 * (a padded row, a dummy slot, an unchanged mark) gets exactly 0; a donor of zeros gives the bits of cf_integrated_gradients_raw
 * in out, logits_x, logits_base and delta.  `cmean` as `coeff` above.  Limits: u, ud < ~80; 1 + mk <= 0 gives inf / NaN.
 * Deterministic; the result does not depend on max_batch.
 * Refused by name, before anything is launched: everything cf_integrated_gradients_raw refuses except the feature baseline; a NULL
 * base_promoter_feats / base_pcre_feats[r] of an interpolated feature input; base_broadcast != 0; a cmean field set for an input that
 * is not interpolated; a non-NULL cmean->interaction_freq. */
int cf_integrated_gradients_raw_donor(cf_handle* h, const cf_batch* batch, const cf_ig_opts* opts, const cf_input_grads* out,
                                      const cf_input_grads* cmean, float* logits_x, float* logits_base, float* delta, void* stream);
/* In-silico perturbation scan (interpretation): what would the prediction be if the marks of a mark set were scaled by s -- erased
 * (s = 0), doubled (s = 2) -- over a window of the promoter or of one pCRE?  The perturbation is defined in RAW-SIGNAL space and is
 * exact there: binning is linear, so scaling the window's samples by s scales the means of its bins by s, and a covered feature
 * u = log(1 + m) becomes
 *   u' = log1pf(s expm1f(u))                          fp32, each operation rounded (no contraction)
 * which is the feature the binning produces from the scaled signal.  Every other element of every input, and every mask, is the gene's own.
 * Geometry: c = the coarsest resolution (fewest bins), W = n_bins[c], R_r = n_bins[r] / W (20 / 80 / 400 bins: 1, 4, 20).  At
 * resolution r the centre pad-mask row of the region gives q_r / e_r, its first / last unmasked row, and n_r = e_r - q_r + 1 (0: all
 * masked; holes inside count as real rows).  Genomic bin j is row q_r + j, or row q_r + n_r - 1 - j where the region is stored
 * mirrored (flip[b] != 0: the dataset mirrors '-' strand promoters, never pCREs).  Window g of width w covers the coarse genomic bins
 * [g, min(g + w, n_c)) and at resolution r the genomic bins [g R_r, min(min(g + w, n_c) R_r, n_r)): bin sizes nest, every finer bin
 * lies wholly inside one coarse bin (short last bins included), no sample counts are needed. */
typedef struct cf_scan_opts {
    int region;                 /* 0 promoter, 1 + j pCRE slot j                                  */
    int width;                  /* window width in coarsest bins, >= 1                            */
    int n_sets;                 /* >= 1                                                           */
    const unsigned* mark_sets;  /* host [n_sets]; bit f set: mark f is scaled; 0 = nothing (read before the call returns) */
    float scale;                /* s >= 0, finite                                                 */
    const uint8_t* flip;        /* device [B], non-zero: the region is stored mirrored; NULL: none */
    float* feats_out[CF_MAX_RES]; /* optional, device, [B, V, n_bins[r], n_feats]                  */
} cf_scan_opts;
/* logits: [B, V, n_out], V = 1 + n_sets * W, gene-major (b * V + v):
 *   v = 0               the unperturbed gene (bit-equal to cf_forward(save = 0));
 *   v = 1 + k * W + g   mark set k applied to window g; a window with g >= n_c (a dummy slot, a narrowed promoter, a short pCRE) or
 *                       an empty set changes nothing: the baseline's logits, bit for bit.
 * feats_out[r] (optional): the features of the scanned region that the forward of row (b, v) read, OVERWRITTEN in full.
 * Rows run in chunks of at most max_batch.  Per chunk one k_scan_expand writes the rows' inputs -- features of every region and
 * resolution with the covered rows of the scanned region rewritten, compact pad-mask rows (all L rows of a full promoter mask with
 * embed.n_layers > 1), interaction masks, frequencies -- into the chunk buffers of cf_integrated_gradients (whichever call comes
 * first allocates them; cf_destroy frees them), then the launches of cf_forward(save = 0) run on the chunk and write its slice of
 * `logits`:   cf_launch_counts fwd = ceil(B * V / max_batch) * (1 + n_fwd),  n_fwd = what cf_forward(save = 0) issues.
 * Deterministic (no atomics).  Off the fused trunk k_attc2's regions per workgroup are chosen as for the caller's B genes, so the
 * result does not depend on max_batch and row (b, v) equals cf_forward(save = 0) on the batch with feats_out[:, v] substituted, bit
 * for bit.  Overwrites the activations a cf_forward(save >= 1) kept: no cf_backward* may follow without a new saving forward.
 * Limits: u < ~80 (expm1f overflows past 88); a negative feature with 1 + s m <= 0 gives NaN, as the forward's log does.
 * Refused by name, before anything is launched: a null handle / batch / opts / logits / mark_sets, B > max_batch, region outside
 * [0, i_max], width < 1, n_sets < 1, a negative or non-finite scale, a mark bit >= n_feats, an n_bins[r] that is no multiple of the
 * smallest, a feats_out index >= n_res, armed riders. */
int cf_perturbation_scan(cf_handle* h, const cf_batch* batch, const cf_scan_opts* opts, float* logits, void* stream);
/* The scan of several regions of every gene from one call, the pCRE variants slot-packed. */
typedef struct cf_scan_regions_opts {
    unsigned regions;           /* bit 0: the promoter; bit 1 + j: pCRE slot j.  At least one bit; no bit above i_max */
    int width, n_sets;
    const unsigned* mark_sets;  /* host [n_sets], as in cf_scan_opts */
    float scale;
    const uint8_t* flip;        /* device [B] or NULL: applies to the promoter block only (pCREs are never stored mirrored) */
} cf_scan_regions_opts;
/* logits: [n_reg, B, V, n_out], n_reg = the set bits of `regions`, the regions in ascending bit order, V = 1 + n_sets * W as above.
 * Block q carries, bit for bit, what cf_perturbation_scan writes for that region with the same width, mark_sets and scale -- with
 * flip = opts->flip for the promoter block, flip = NULL for a pCRE block.  So row v = 0 of every block is the unperturbed gene, and
 * dead windows, empty sets and dummy slots give the baseline's bits.  There is no feats_out (cf_perturbation_scan serves that).
 * The promoter block runs the launches of cf_perturbation_scan.  A pCRE slot j does not: its Pairwise output depends on the promoter
 * and on slot j alone, so only row j + 1 of the Regulation input [B, T, d_emb] differs between the gene and a variant, and the S slots
 * of a (gene, resolution) workgroup are S independent (promoter, pCRE) pairs that pass through the same operations in the same order.
 * With any pCRE bit the trunk runs once on the B genes and its output is stashed (k_pcre_stash, the buffers of cf_pcre_ablation).
 * Then per pCRE slot j, with U = ceil((V - 1) / S), S = i_max:
 *   pack phase   pseudo rows (b, u), gene-major, in chunks of at most max_batch: k_scan_pack writes gene b's promoter and, into slot s,
 *                its slot j under variant v = 1 + u * S + s (v >= V: verbatim) with slot j's pad-mask row in every slot, into the chunk
 *                buffers of cf_integrated_gradients; the trunk part of cf_forward(save = 0) runs on the chunk (k_attc2's regions per
 *                workgroup as for the caller's B genes); k_scan_unpack copies rows 1..S of each pseudo-gene's output to a handle-owned
 *                buffer [n_res][B * (V - 1), d_emb] (grown on demand, freed by cf_destroy; 15.7 MB at B = 64, V = 161);
 *   row phase    rows (b, v) in output order, in chunks of at most max_batch: k_scan_rows writes the stash back with row j + 1 taken
 *                from that buffer for v >= 1, and the gene's interaction masks and frequencies; the Regulation + head launches of
 *                cf_forward(save = 0) write the chunk's slice of the block.
 * With np / nc the promoter / pCRE bits set, C = ceil(B * V / max_batch), P = ceil(B * U / max_batch):
 *   cf_launch_counts fwd = np * C * (1 + n_fwd) + [nc > 0] * (n_trunk + 1) + nc * (P * (n_trunk + 2) + C * (1 + n_reg_head))
 * (n_fwd = n_trunk + n_reg_head: see cf_pcre_ablation): a pCRE region issues P trunk passes, not C.  CF_SCAN_PACK=0 at cf_create runs
 * the pCRE blocks through the launches of cf_perturbation_scan as well (the cross-check: the same bits; fwd = n_reg * C * (1 + n_fwd)).
 * Deterministic (no atomics); the result does not depend on max_batch.  Overwrites the activations a cf_forward(save >= 1) kept: no
 * cf_backward* may follow without a new saving forward.  Parameters, gradients and moments are untouched.
 * Refused by name, before anything is launched: everything cf_perturbation_scan refuses (a null handle / batch / opts / logits /
 * mark_sets, B > max_batch, width < 1, n_sets < 1, a negative or non-finite scale, a mark bit >= n_feats, non-nested n_bins, armed
 * riders), regions == 0, a region bit above i_max. */
int cf_perturbation_scan_regions(cf_handle* h, const cf_batch* batch, const cf_scan_regions_opts* opts, float* logits, void* stream);
/* pCRE transplant screen (interpretation): what would a gene's prediction be if another enhancer were brought into contact with its
 * promoter, and how does the answer depend on contact strength?  A library of C candidate regions -- features [C, n_bins[r], n_feats]
 * and centre pad-mask rows [C, n_bins[r]] (non-zero = masked) per resolution -- is tried in ONE pCRE slot of every gene, each candidate
 * at Q contact frequencies.  logits: [B, 1 + C * Q, n_out], gene-major; row (b, 0) is gene b verbatim (cf_forward(save = 0), bit-equal),
 * row (b, 1 + c * Q + q) is the inference forward of gene b with candidate c in slot j = the gene's slot at f = freq[b, c, q]:
 *   features     pcre_feats[r][b, j] = lib_feats[r][c] and the slot's centre pad-mask row = lib_mask[r][c] at every resolution (for a
 *                full [B, S, 1, L, L] mask: rows_promoter | lib columns; the forward reads the centre row, which lies inside every
 *                promoter's real rows).  A candidate without a real bin is a fully masked row: the uniform softmax of a dummy slot;
 *   interaction  per resolution, with dead(t) = interaction_mask[r][b, t, t] for t != j + 1:  entries (j + 1, t) and (t, j + 1) become
 *                dead(t), entry (j + 1, j + 1) becomes 0, every other entry is unchanged -- on the dataset's block masks: the mask
 *                after replacing partner j (j < n_part) or appending one (j = n_part);
 *   frequencies  entry (0, j + 1) becomes f, every other entry of row and column j + 1 becomes 0, the rest is unchanged: what the
 *                dataset writes for a partner with score f.
 * The slot: slot[b] (device data; a value outside [-1, i_max) is read as -1), or slot_all for every gene when slot == NULL, where
 * slot_all = -1 is "append": the first token t >= 1 whose diagonal entry of the coarsest resolution's interaction mask is set, formed
 * on the device.  Slot -1 (explicit, or a gene with every token live under "append") = not placed: every row of that gene carries the
 * bits of row 0.  slot_out [B], if given, receives the slot used per gene.
 * A slot's Pairwise output depends on the promoter and on that slot alone and the Regulation stack has no positional encoding, so
 * i_max candidates ride as the slots of one pseudo-gene through one trunk pass and a candidate's trunk row serves all Q frequencies.
 * With S = i_max, U = ceil(C / S): the trunk runs once on the B genes and its output is stashed (k_pcre_stash), then
 *   pack phase   pseudo rows (b, u), gene-major, in chunks of at most max_batch: k_transplant_pack writes gene b's promoter (all L rows
 *                of a full mask with embed.n_layers > 1) and candidate u * S + s into slot s (past C: a dummy, zero features and a fully
 *                masked row) into the chunk buffers of cf_integrated_gradients; the trunk part of cf_forward(save = 0) runs on the chunk
 *                (k_attc2's regions per workgroup as for the caller's B genes); k_scan_unpack copies rows 1..S of each pseudo-gene's
 *                output to the handle-owned buffer of cf_perturbation_scan_regions, here [n_res][B * C, d_emb];
 *   row phase    rows (b, v) in output order, in chunks of at most max_batch: k_transplant_rows writes the stash back with row j + 1
 *                taken from that buffer for v >= 1 of a placed gene, the edited interaction masks and frequencies; the Regulation +
 *                head launches of cf_forward(save = 0) write the chunk's slice.
 *   cf_launch_counts fwd = (n_trunk + 1) + ceil(B * U / max_batch) * (n_trunk + 2) + ceil(B * (1 + C * Q) / max_batch) * (1 + n_reg_head)
 * (n_trunk, n_reg_head: see cf_pcre_ablation).  Deterministic (no atomics); the result does not depend on max_batch.  Overwrites the
 * activations a cf_forward(save >= 1) kept: no cf_backward* may follow without a new saving forward.  Parameters, gradients and moments
 * are untouched.  Limits: one slot per row (no combinations of transplants); promoters are not transplanted; candidates are never
 * stored mirrored; there is no feats_out.
 * Refused by name, before anything is launched: a null handle / batch / opts / logits / freq, a null lib_feats[r] / lib_mask[r] for
 * r < n_res or a non-null one for r >= n_res, B > max_batch, n_cand < 1, n_freq < 1, B * (1 + C * Q) beyond int, slot_all outside
 * [-1, i_max), armed riders. */
typedef struct cf_transplant_opts {
    int n_cand, n_freq;                         /* C >= 1, Q >= 1 */
    const float*   lib_feats[CF_MAX_RES];       /* device [C, L_r, F] fp32 */
    const uint8_t* lib_mask[CF_MAX_RES];        /* device [C, L_r] */
    const float*   freq;                        /* device [B, C, Q] */
    const int*     slot;                        /* device [B], each in [-1, i_max), or NULL: slot_all for every gene */
    int            slot_all;                    /* a slot, or -1 = "append" */
    int*           slot_out;                    /* device [B] or NULL: the slot used per gene, -1 = not placed */
} cf_transplant_opts;
int cf_pcre_transplant(cf_handle* h, const cf_batch* batch, const cf_transplant_opts* opts, float* logits, void* stream);
/* Fine-resolution perturbation scan (interpretation): the scan above with windows given in bins of the FINEST resolution -- "where
 * inside this coarse bin?".  The perturbation is the scan's (the window's raw samples of a mark set scaled by s); a fine window covers
 * a coarser bin only in part, and such a bin is recomputed from its finest children, weighted by sample counts.
 * The rule.  f = the resolution with the smallest bin size, b_r the bin sizes, R_r = n_bins[f] / n_bins[r] (an n_bins[f] that is not a
 * multiple of every n_bins[r] is refused).  The real rows [q_r, q_r + n_r) of the region come from the centre pad-mask rows as above;
 * genomic bin j is row q_r + j, or q_r + n_r - 1 - j under flip[b].
 * Sample counts: finest bin k holds cnt_k = b_f samples, except the last real one, which with `lengths` given holds
 * len - (n_f - 1) b_f samples (1 <= cnt <= b_f, else refused).  Bin j at resolution r has the children K_j = [j R_r, min((j + 1) R_r, n_f))
 * and cnt_j = sum of cnt_k over K_j.  lengths = NULL: every real finest bin is full -- exact whenever the region's length is a multiple
 * of b_f (the promoter's always is).
 * A window [lo, hi) is given in finest genomic bins.  With C = K_j n [lo, hi), for a mark of the set:
 *   C empty, or lo >= n_f    the element keeps its bits;
 *   C = K_j                  u' = log1pf(s expm1f(u)), the scan's function: a fine window that is a union of whole coarse bins
 *                            reproduces the scan bit for bit; the finest resolution always falls under this case;
 *   otherwise                S  = sum over k in C of (double)cnt_k (double)expm1f(u_k), in ascending genomic k,
 *                            m' = (float)((double)expm1f(u_j) + ((double)s - 1.0) S / (double)cnt_j),
 *                            u' = log1pf(m'); no contraction, no clamp; u_k are the source gene's finest-resolution elements of the
 *                            same region and mark.
 * Binning is linear per mark, so this is the feature that binning produces when the raw samples inside the window are scaled by s, up
 * to the rounding of the stored fp32 features.  Limits: those of the scan (u < ~80; 1 + m' <= 0 gives NaN as log does); and a partly
 * covered bin that is nearly emptied carries an absolute error of order eps (1 + m_j) / (1 + m'). */
typedef struct cf_scan_fine_opts {
    int region;                 /* 0 promoter, 1 + j pCRE slot j                                  */
    int n_sets;                 /* >= 1                                                           */
    const unsigned* mark_sets;  /* host [n_sets], as in cf_scan_opts                              */
    float scale;                /* s >= 0, finite                                                 */
    const uint8_t* flip;        /* device [B] or NULL, as in cf_scan_opts                         */
    int width, stride, n_windows; /* each >= 1; width and stride in finest bins                   */
    const int* start;           /* host [B] or NULL (all 0): the gene's first finest genomic bin  */
    const int* lengths;         /* host [B] or NULL: the scanned region's length in samples       */
    float* feats_out[CF_MAX_RES]; /* optional, device, [B, V, n_bins[r], n_feats]                  */
} cf_scan_fine_opts;
/* Window g of gene b covers the finest genomic bins [start[b] + g stride, start[b] + g stride + width), clipped to n_bins[f].
 * logits: [B, V, n_out], V = 1 + n_sets * n_windows, gene-major; v = 0 the unperturbed gene, v = 1 + k * n_windows + g mark set k over
 * window g.  Windows past the real bins, empty sets and dummy slots give the baseline's bits.  feats_out as in cf_scan_opts.
 * Rows run in chunks of at most max_batch in the chunk buffers of cf_integrated_gradients; start and the tail counts travel in the
 * workspace's word table behind the mark sets (no device buffer of its own).  Per chunk one k_scan_fine_expand, then the launches of
 * cf_forward(save = 0):   cf_launch_counts fwd = ceil(B * V / max_batch) * (1 + n_fwd).
 * Deterministic (no atomics); k_attc2's regions per workgroup are chosen as for the caller's B genes, so the result does not depend on
 * max_batch and row (b, v) equals cf_forward(save = 0) on the batch with feats_out[:, v] substituted, bit for bit.  Overwrites the
 * activations a cf_forward(save >= 1) kept.  Parameters, gradients and moments are untouched.
 * Refused by name, before anything is launched: everything cf_perturbation_scan refuses; width, stride or n_windows < 1; a negative
 * start; a lengths[b] outside ((n_f - 1) b_f, n_f b_f] for that gene's real n_f (read back from the finest pad-mask rows, a copy and a
 * stream synchronisation; a dummy slot is exempt: it is ignored); an n_bins[f] that is no multiple of every n_bins[r]. */
int cf_perturbation_scan_fine(cf_handle* h, const cf_batch* batch, const cf_scan_fine_opts* opts, float* logits, void* stream);
/* Histone-mark coalitions, exact Shapley values of the marks and their pair epistasis (interpretation): which marks carry the
 * prediction, and do they act alone or together?  The players of the game are MARKS, each optionally restricted to a set of regions.
 * Player p is a pair of words: player_marks[p] (bit f: mark f; non-zero, no bit >= n_feats) and player_regions[p] (bit 0: the promoter,
 * bit 1 + j: pCRE slot j; non-zero, no bit above i_max).  A coalition is a 32-bit word m, bit p set = player p PRESENT.  Row (b, m) is
 * the inference forward of gene b with these inputs: for every region rho,
 *   gone(rho) = OR of player_marks[p] over the absent players p whose player_regions[p] has bit rho
 * and every element of region rho (every row, every resolution) whose mark f has its bit in gone(rho) becomes
 *   u' = log1pf(s expm1f(u))                          fp32, each operation rounded (no contraction): the rule of the perturbation scan
 * Every other element keeps its bits; all masks and interaction_freq are gene b's.  Binning is linear, so this is exactly the feature
 * the binning produces when the raw samples of those marks are scaled by s over the whole region.  s = 0 erases the mark: a
 * non-negative finite feature becomes exactly +0.  Padded rows hold zeros and keep their bits.  Players may overlap: an element is
 * scaled once if any player that covers it is absent.  Limits: those of the scan (u < ~80; a negative feature with 1 + s m <= 0 gives
 * NaN). */
typedef struct cf_mark_opts {
    int n_players;                   /* 1..16 */
    const unsigned* player_marks;    /* host [n_players], read before the call returns */
    const unsigned* player_regions;  /* host [n_players] */
    float scale;                     /* s >= 0, finite: what an ABSENT player's elements are scaled by; 0 erases */
} cf_mark_opts;                      /* 32 bytes */
/* cf_mark_coalitions: keep is a HOST array of n_coal words (read before the call returns); logits [B, n_coal, n_out], gene-major
 * (b * n_coal + c).  The full word 2^P - 1 is cf_forward(save = 0), bit for bit.  Rows run in chunks of at most max_batch; per chunk
 * one k_mark_expand writes the rows' inputs -- features of every region and resolution, each element once, compact pad-mask rows (all L
 * rows of a full promoter mask with embed.n_layers > 1), interaction masks, frequencies -- into the chunk buffers of
 * cf_integrated_gradients (whichever call comes first allocates them; cf_destroy frees them), then the launches of
 * cf_forward(save = 0) run on the chunk and write its slice of `logits`:
 *   cf_launch_counts fwd = ceil(B * n_coal / max_batch) * (1 + n_fwd),  n_fwd = what cf_forward(save = 0) issues.
 * The coalition words and the player words travel in the device table the handle owns (grown on demand).  Deterministic (no atomics).
 * Off the fused trunk k_attc2's regions per workgroup are chosen as for the caller's B genes, so the result does not depend on
 * max_batch.  Overwrites the activations a cf_forward(save >= 1) kept: no cf_backward* may follow without a new saving forward.
 * Parameters, gradients and moments are untouched.
 * Refused by name, before anything is launched: a null handle / batch / opts / keep / logits, B > max_batch, n_players outside 1..16,
 * a null or zero player word, a mark bit >= n_feats, a region bit above i_max, n_coal < 1, a keep bit >= n_players, a negative or
 * non-finite scale, armed riders. */
int cf_mark_coalitions(cf_handle* h, const cf_batch* batch, const cf_mark_opts* opts, const uint32_t* keep, int n_coal, float* logits,
                       void* stream);
/* Exact Shapley values of the P players: all 2^P coalitions through the routine above (word m at column m), then one k_shapley with
 * the P weights w(k) = k! (P - k - 1)! / P! computed on the host in double and rounded to fp32 (see cf_pcre_shapley: the same kernel, a
 * fixed order, every operation rounded to fp32).  phi [B, P, n_out]; efficiency: sum_p phi[b, p] = v[b, 2^P - 1] - v[b, 0] up to
 * rounding; a player whose elements are all zeros (a dummy slot) is a null player, phi exactly 0.  logits_all: [B, 2^P, n_out], or
 * NULL: the rows go to the handle-owned buffer of cf_pcre_shapley.  fwd = that of cf_mark_coalitions with n_coal = 2^P, plus 1.
 * Refusals as above (null phi). */
int cf_mark_shapley(cf_handle* h, const cf_batch* batch, const cf_mark_opts* opts, float* phi, float* logits_all, void* stream);
/* Pair epistasis of the players.  With N = 2^P - 1 the rows are: 0: N; 1 + i: N without i; then N without i and j for the pairs i < j
 * in lexicographic order (1 + P + P (P - 1) / 2 rows), through the routine above, then one k_epistasis (see cf_pcre_epistasis):
 *   eps[b, i, j] = ((v_N - v_{N\i}) - v_{N\j}) + v_{N\{i,j}} for i < j, fp32, each operation rounded; eps[b, j, i] carries its bits;
 *   eps[b, i, i] = v_N - v_{N\i}.
 * eps [B, P, P, n_out].  logits_pairs: [B, 1 + P + P (P - 1) / 2, n_out], or NULL (the handle-owned buffer).  fwd = that of
 * cf_mark_coalitions with that n_coal, plus 1.  Refusals as above (null eps). */
int cf_mark_epistasis(cf_handle* h, const cf_batch* batch, const cf_mark_opts* opts, float* eps, float* logits_pairs, void* stream);
/* Pairwise Shapley interaction indices of the P players (see cf_shapley_interactions_from_rows): cf_mark_shapley's rows (all 2^P
 * coalitions, logits_all as there), then k_shapley_pairs; phi [B, P, n_out] is optional: if given, k_shapley runs on the same rows too.
 * inter [B, P, P, n_out].  fwd = that of cf_mark_coalitions with n_coal = 2^P, plus 1 per reducer launched (1, or 2 with phi).
 * Refused by name, before anything is launched: what cf_mark_shapley refuses (phi may be null), a null inter, an index other than the
 * two constants, n_players < 2. */
int cf_mark_shapley_interactions(cf_handle* h, const cf_batch* batch, const cf_mark_opts* opts, int index, float* inter, float* phi,
                                 float* logits_all, void* stream);
/* The same game against a DONOR (interpretation): gene G is predicted on in one cell type and off in another -- which mark changes
 * account for the difference?  Players, coalition words and gone(rho) are those of cf_mark_coalitions; the caller passes, beside the
 * batch, the same B genes' features in the other cell type, and every element of region rho (every row, every resolution, padded rows
 * included) whose mark f has its bit in gone(rho) takes the BITS of the donor's element at the same (gene, region, row, resolution,
 * mark).  A select, not arithmetic: NaN payloads, -0 and inf pass through unchanged.  Every other element keeps the gene's bits; all
 * masks and interaction_freq are gene b's.  Players may overlap: an element is the donor's if any player that covers it is absent.
 * Binning works per mark, so where the two cell types share a region's coordinates this is exactly the feature the binning produces
 * when those marks' rows of the raw region are replaced by the donor's.  The donor may alias the batch's own feature pointers (every
 * row is then the plain forward). */
typedef struct cf_mark_donor_opts {
    int n_players;                                   /* 1..16 */
    const unsigned* player_marks;                    /* host [n_players], read before the call returns */
    const unsigned* player_regions;                  /* host [n_players] */
    const float* donor_promoter_feats[CF_MAX_RES];   /* device, layout of cf_batch.promoter_feats: what an ABSENT player's elements become */
    const float* donor_pcre_feats[CF_MAX_RES];       /* device, layout of cf_batch.pcre_feats */
} cf_mark_donor_opts;                                /* 72 bytes */
/* cf_mark_donor_coalitions: keep, logits, the chunking, the launch count, the effect on saved activations and on parameters are those
 * of cf_mark_coalitions, with k_mark_donor_expand in place of k_mark_expand: it reads the donor's bytes only in regions with
 * gone(rho) != 0.  The full word 2^P - 1 is cf_forward(save = 0) on the batch, bit for bit; with every element covered by some player,
 * word 0 is the donor's features under the gene's masks and frequencies.  Only the workspace of cf_mark_coalitions is used: no device
 * buffer is added.
 * Refused by name, before anything is launched: what cf_mark_coalitions refuses (there is no scale), and a null
 * donor_promoter_feats[r] or donor_pcre_feats[r] for an r below the model's resolution count. */
int cf_mark_donor_coalitions(cf_handle* h, const cf_batch* batch, const cf_mark_donor_opts* opts, const uint32_t* keep, int n_coal,
                             float* logits, void* stream);
/* cf_mark_shapley with the donor rule: phi [B, P, n_out], sum_p phi[b, p] = v[b, 2^P - 1] - v[b, 0] up to rounding -- the prediction
 * minus the prediction on the donor's marks; a player whose elements carry the same bits in both feature sets (a slot that is a dummy
 * in both) is a null player, phi exactly 0.  logits_all and fwd as there.  Refusals as above (null phi). */
int cf_mark_donor_shapley(cf_handle* h, const cf_batch* batch, const cf_mark_donor_opts* opts, float* phi, float* logits_all, void* stream);
/* cf_mark_epistasis with the donor rule: eps [B, P, P, n_out], rows, logits_pairs and fwd as there.  Refusals as above (null eps). */
int cf_mark_donor_epistasis(cf_handle* h, const cf_batch* batch, const cf_mark_donor_opts* opts, float* eps, float* logits_pairs, void* stream);
/* cf_mark_shapley_interactions with the donor rule: cf_mark_donor_shapley's rows, then k_shapley_pairs (and k_shapley with phi); a
 * player whose elements carry the same bits in both feature sets is a null player: its row and column of inter are exactly 0.  fwd
 * and refusals as there, with cf_mark_donor_shapley's in place of cf_mark_shapley's. */
int cf_mark_donor_shapley_interactions(cf_handle* h, const cf_batch* batch, const cf_mark_donor_opts* opts, int index, float* inter, float* phi,
                                       float* logits_all, void* stream);
/* The same game over up to 128 players (interpretation): which mark matters at which region?  "Mark f in region rho" is
 * n_feats * (i_max + 1) players -- 63 on the default model, 119 at i_max = 16 -- more than one word holds and far more than 2^P rows
 * can enumerate.  Players, gone(rho), the scale rule and the donor rule are exactly those above; a coalition is kw = ceil(P / 32)
 * consecutive 32-bit words, bit p % 32 of word p / 32 set = player p PRESENT.  One struct serves both rules. */
typedef struct cf_mark_wide_opts {
    int n_players;                                   /* 1..128 */
    const unsigned* player_marks;                    /* host [n_players], read before the call returns */
    const unsigned* player_regions;                  /* host [n_players] */
    float scale;                                     /* the scale rule: used when every donor pointer is NULL */
    const float* donor_promoter_feats[CF_MAX_RES];   /* all NULL: scale rule; all non-NULL below n_res: donor rule; mixed: refused */
    const float* donor_pcre_feats[CF_MAX_RES];
} cf_mark_wide_opts;                                 /* 80 bytes */
/* cf_mark_coalitions_wide: keep is a HOST array of n_coal * kw words, coalition k at [k kw, (k + 1) kw) (read before the call returns);
 * logits [B, n_coal, n_out], gene-major.  The full word is cf_forward(save = 0), bit for bit; with P <= 16 the rows carry the bits of
 * cf_mark_coalitions / cf_mark_donor_coalitions on the same words.  Rows run in chunks of at most max_batch in the chunk buffers of
 * cf_mark_coalitions; per chunk one k_mark_expand (the donor rule: k_mark_donor_expand) reading kw words per row, then the launches of
 * cf_forward(save = 0) on the chunk:
 *   cf_launch_counts fwd = ceil(B * n_coal / max_batch) * (1 + n_fwd),  n_fwd = what cf_forward(save = 0) issues.
 * The words and the 2 P player words travel in the device table the handle owns (grown on demand); no other device buffer is added.
 * Deterministic (no atomics); k_attc2's regions per workgroup are chosen as for the caller's B genes, so the result does not depend on
 * max_batch.  Overwrites the activations a cf_forward(save >= 1) kept.  Parameters, gradients and moments are untouched.
 * Refused by name, before anything is launched: what cf_mark_coalitions refuses, with n_players in 1..128; a keep bit >= n_players in
 * any word (the coalition's index is named); donor pointers of which some but not all below the model's resolution count are NULL;
 * under the scale rule a negative or non-finite scale. */
int cf_mark_coalitions_wide(cf_handle* h, const cf_batch* batch, const cf_mark_wide_opts* opts, const uint32_t* keep, int n_coal, float* logits,
                            void* stream);
/* Permutation-SAMPLED Shapley values of the P players.  perms: HOST bytes [n_perm, P], each row a permutation of 0..P-1: an order of
 * adding the players (read before the call returns).  Per gene R = 2 + n_perm * (P - 1) rows run through the routine above:
 *   column 0                          nobody present
 *   column 1                          everybody present: cf_forward(save = 0), bit for bit
 *   column 2 + q * (P - 1) + (k - 1)  the first k players of permutation q, k = 1 .. P - 1
 * (the two end rows are shared by all permutations), then one k_perm_shapley per (gene, player).  With r the position of player p
 * in permutation q and col(q, 0) = 0, col(q, P) = 1:
 *   d_q = v[col(q, r + 1)] - v[col(q, r)]                          one fp32 subtraction
 *   phi[b, p] = (sum_q d_q) / n_perm
 *   se[b, p]  = sqrt(sum_q (d_q - phi)^2 / (n_perm (n_perm - 1)))  0 for n_perm = 1
 * every operation rounded to fp32, a fixed summation order (a strided partial sum per thread, then a fixed tree), no atomics: the
 * result does not depend on max_batch.  phi [B, P, n_out]; se [B, P, n_out] or NULL; logits_rows [B, R, n_out] or NULL (the
 * handle-owned buffer of cf_pcre_shapley).  The inverse permutations travel as bytes in the word table.
 * Efficiency: sum_p phi[b, p] = v[b, 1] - v[b, 0] up to rounding (it telescopes in every permutation).  A player whose elements carry
 * the same bits present and absent (a dummy slot; identical donor bits) has phi and se exactly 0.  With all P! permutations phi is the
 * exact Shapley value.  Otherwise phi is an ESTIMATE: its sampling error is what se reports (the standard error of the mean, assuming
 * independent uniform permutations) and is not bounded by the library.
 * fwd = that of cf_mark_coalitions_wide with n_coal = R, plus 1.
 * Refused by name, before anything is launched: what cf_mark_coalitions_wide refuses (null phi), null perms, n_perm < 1, a row of
 * perms that is not a permutation (its index q is named). */
int cf_mark_shapley_sampled(cf_handle* h, const cf_batch* batch, const cf_mark_wide_opts* opts, const uint8_t* perms, int n_perm, float* phi,
                            float* se, float* logits_rows, void* stream);
/* The same game with WINDOWS as players (interpretation): where inside a region does the signal lie?  c = the coarsest resolution,
 * W = n_bins[c], R_r = n_bins[r] / W.  Player p is (player_marks[p], player_regions[p], [player_lo[p], player_hi[p])): those marks in
 * those regions over the coarse genomic bins lo .. hi - 1, the windows of cf_perturbation_scan; 0 <= lo < hi <= W.  Coalitions are
 * the kw = ceil(P / 32) words of cf_mark_coalitions_wide.  Row (b, k) is the inference forward of gene b with, for every region rho
 * and coarse genomic bin g,
 *   gone(rho, g) = OR of player_marks[p] over the absent players p with bit rho in player_regions[p] and lo_p <= g < hi_p
 * Region rho's real rows at resolution r are [q_r, q_r + n_r) and n_c is its real bin count at c, from the centre pad-mask rows of
 * the batch as cf_perturbation_scan reads them.  Genomic bin j is row q_r + j, or row q_r + n_r - 1 - j where flip[b] is set (the
 * promoter only: a pCRE is never stored mirrored).  The element of a real row with genomic bin j and mark f, g = j / R_r, g < n_c and
 * bit f in gone(rho, g) changes -- the scale rule: log1pf(s expm1f(u)), once however many absent players cover it; the donor rule:
 * the bits of the donor's element at the same position -- and every other element keeps its bits; masks and interaction_freq are
 * gene b's.  Bin sizes nest and binning is linear per mark: this is exactly the feature the binning produces when the raw samples
 * of those marks inside the windows are scaled by s, or replaced by the donor's.  A window with lo_p >= n_c (a dummy slot, a short
 * pCRE, a narrowed promoter) changes nothing: a null player.  One absent player with one region bit gives the row of
 * cf_perturbation_scan(region, width = hi - lo) at window lo, bit for bit; with every window [0, W) and zeros in the padded rows (the
 * donor rule: a donor that agrees with the gene outside the real rows) the rows are those of cf_mark_coalitions_wide. */
typedef struct cf_mark_window_opts {
    int n_players;                                   /* 1..128 (cf_mark_window_shapley: 1..16) */
    const unsigned* player_marks;                    /* host [n_players], read before the call returns */
    const unsigned* player_regions;                  /* host [n_players] */
    const int* player_lo;                            /* host [n_players]: the first coarse genomic bin of the player's window */
    const int* player_hi;                            /* host [n_players]: one past the last */
    const uint8_t* flip;                             /* device [B] or NULL: gene b's promoter is stored mirrored (the '-' strand) */
    float scale;                                     /* the scale rule: used when every donor pointer is NULL */
    const float* donor_promoter_feats[CF_MAX_RES];   /* all NULL: scale rule; all non-NULL below n_res: donor rule; mixed: refused */
    const float* donor_pcre_feats[CF_MAX_RES];
} cf_mark_window_opts;                               /* 104 bytes */
/* cf_mark_window_coalitions: keep (HOST, n_coal * kw words), logits [B, n_coal, n_out], the chunking and the chunk buffers are those of
 * cf_mark_coalitions_wide; per chunk one k_mark_window_expand (the donor rule: k_mark_window_donor_expand), then the launches of
 * cf_forward(save = 0) on the chunk:
 *   cf_launch_counts fwd = ceil(B * n_coal / max_batch) * (1 + n_fwd),  n_fwd = what cf_forward(save = 0) issues.
 * The words and the 4 P player words (marks, regions, lo, hi) travel in the device table the handle owns; no device buffer is added.
 * Deterministic (no atomics); the result does not depend on max_batch.  Overwrites the activations a cf_forward(save >= 1) kept.
 * Parameters, gradients and moments are untouched.
 * Refused by name, before anything is launched: what cf_mark_coalitions_wide refuses; a null player_lo or player_hi; a window with
 * lo < 0, hi > W or lo >= hi (the player's index is named); an n_bins[r] that is no multiple of W; W > 64. */
int cf_mark_window_coalitions(cf_handle* h, const cf_batch* batch, const cf_mark_window_opts* opts, const uint32_t* keep, int n_coal,
                              float* logits, void* stream);
/* Exact Shapley values of P <= 16 window players: all 2^P words through the routine above (word m at column m), then the k_shapley
 * of cf_mark_shapley.  phi [B, P, n_out]; logits_all [B, 2^P, n_out] or NULL (the handle-owned buffer).  A null player's phi is
 * exactly 0.  fwd = that of cf_mark_window_coalitions with n_coal = 2^P, plus 1.  Refusals as above (null phi, n_players > 16). */
int cf_mark_window_shapley(cf_handle* h, const cf_batch* batch, const cf_mark_window_opts* opts, float* phi, float* logits_all, void* stream);
/* Pairwise Shapley interaction indices of P <= 16 window players (see cf_shapley_interactions_from_rows): cf_mark_window_shapley's
 * rows, then k_shapley_pairs (and k_shapley with the optional phi).  inter [B, P, P, n_out]; a null player's row and column are exactly
 * 0.  fwd = that of cf_mark_window_coalitions with n_coal = 2^P, plus 1 per reducer launched (1, or 2 with phi).  Refused by name,
 * before anything is launched: what cf_mark_window_shapley refuses (phi may be null), a null inter, an index other than the two
 * constants, n_players < 2. */
int cf_mark_window_shapley_interactions(cf_handle* h, const cf_batch* batch, const cf_mark_window_opts* opts, int index, float* inter, float* phi,
                                        float* logits_all, void* stream);
/* Permutation-sampled Shapley values of the window players: perms, the R = 2 + n_perm * (P - 1) rows per gene, k_perm_shapley, phi, the
 * optional se and logits_rows and the launch count are those of cf_mark_shapley_sampled; a null player's phi and se are exactly 0.
 * Refusals as above and as there. */
int cf_mark_window_shapley_sampled(cf_handle* h, const cf_batch* batch, const cf_mark_window_opts* opts, const uint8_t* perms, int n_perm,
                                   float* phi, float* se, float* logits_rows, void* stream);
/* The window game at the FINEST resolution (interpretation): which 200 bp of this peak?  Neighbouring fine windows of one peak are
 * redundant almost by construction, which is where the leave-one-out map of cf_perturbation_scan_fine misleads most.  Notation is
 * that of cf_perturbation_scan_fine: f = the finest resolution, R_r = n_bins[f] / n_bins[r], K_j = [j R_r, min((j + 1) R_r, n_f)) the
 * finest children of bin j at resolution r, cnt_k = b_f except the last real finest bin (lengths[b] - (n_f - 1) b_f samples), cnt_j =
 * the sum of cnt_k over K_j.
 * The game plays in ONE region per call (region: 0 the promoter, 1 + j pCRE slot j).  Player p is (player_marks[p], [player_lo[p],
 * player_hi[p])), 0 <= lo < hi, in finest genomic bins RELATIVE to start[b]: for gene b its window is [start[b] + lo, start[b] + hi),
 * clipped to the region's real n_f.  Geometry (the extent from the centre pad-mask rows, flip for a mirrored promoter) is the
 * scan's.  Coalitions are the kw = ceil(P / 32) words of cf_mark_coalitions_wide, bit set = PRESENT.  For a coalition
 *   gone_f(k) = OR of player_marks[p] over the absent players whose clipped window holds finest bin k
 * and for bin j of resolution r and mark m, C = {k in K_j : bit m in gone_f(k)}.  The element becomes
 *   C empty        its own bits;
 *   C = K_j        (always so at r = f) the scale rule: log1pf(s expm1f(u)), once however many absent players cover it; the donor
 *                  rule: the bits of the donor's element at the same position;
 *   otherwise      the scale rule:  S  = sum over k in C, ascending genomic k, of (double)cnt_k (double)expm1f(u_k),
 *                                   m' = (float)((double)expm1f(u_j) + ((double)s - 1.0) S / (double)cnt_j),  u' = log1pf(m')
 *                                   -- the partial rule of cf_perturbation_scan_fine operation for operation, no contraction, no clamp;
 *                  the donor rule:  d_k bit-equal to u_k for every k in C: its own bits; else
 *                                   D  = sum over k in C, ascending, of (double)cnt_k ((double)expm1f(d_k) - (double)expm1f(u_k)),
 *                                   m' = (float)((double)expm1f(u_j) + D / (double)cnt_j),  u' = log1pf(m'),
 *                                   d_k the donor's finest element of the same region, mark and position.
 * C may differ from mark to mark in one bin, and any number of bins may be partly covered.  Masks and interaction_freq are the
 * gene's own; every other region is copied verbatim.  Binning is linear per mark and bin sizes nest: this is the feature that binning
 * the edited raw region gives, up to the rounding of the stored fp32 features, and exactly where a bin is wholly covered or untouched.
 * One absent player gives the row and feats_out of cf_perturbation_scan_fine at that window, mark set and start, bit for bit; players
 * whose windows are unions of whole coarse bins give the rows of cf_mark_window_coalitions restricted to the region. */
typedef struct cf_mark_fine_opts {
    int region;                                      /* 0 promoter, 1 + j pCRE slot j */
    int n_players;                                   /* 1..128 (cf_mark_fine_shapley: 1..16) */
    const unsigned* player_marks;                    /* host [n_players], read before the call returns */
    const int* player_lo;                            /* host [n_players]: the window's first finest bin, relative to start[b] */
    const int* player_hi;                            /* host [n_players]: one past the last */
    const int* start;                                /* host [B] or NULL (all 0): gene b's first finest genomic bin */
    const int* lengths;                              /* host [B] or NULL: the region's length in samples, as in cf_scan_fine_opts */
    const uint8_t* flip;                             /* device [B] or NULL: the region of gene b is stored mirrored, as in cf_scan_fine_opts */
    float scale;                                     /* the scale rule: used when every donor pointer is NULL */
    const float* donor_promoter_feats[CF_MAX_RES];   /* all NULL: scale rule; all non-NULL below n_res: donor rule; mixed: refused */
    const float* donor_pcre_feats[CF_MAX_RES];
    float* feats_out[CF_MAX_RES];                    /* optional, device, [B, n_coal, n_bins[r], n_feats]: the edited region */
} cf_mark_fine_opts;
/* cf_mark_fine_coalitions: keep (HOST, n_coal * kw words), logits [B, n_coal, n_out], the chunking and the chunk buffers are those of
 * cf_mark_window_coalitions; per chunk one k_mark_fine_expand (the donor rule: k_mark_fine_donor_expand), then the launches of
 * cf_forward(save = 0) on the chunk:
 *   cf_launch_counts fwd = ceil(B * n_coal / max_batch) * (1 + n_fwd).
 * The words, the 3 P player words (marks, lo, hi), start and the tail counts travel in the device table the handle owns; no device
 * buffer is added.  Deterministic (no atomics); the result does not depend on max_batch and row (b, c) equals cf_forward(save = 0) on
 * the batch with feats_out[:, c] substituted, bit for bit.  Overwrites the activations a cf_forward(save >= 1) kept.  Parameters,
 * gradients and moments are untouched.  A window past the real bins, a player in a dummy slot and a donor-rule player whose touched
 * elements agree in both cell types are null players.
 * Refused by name, before anything is launched: what cf_mark_coalitions_wide and cf_perturbation_scan_fine refuse (a region outside
 * [0, i_max], a negative start, a lengths[b] outside ((n_f - 1) b_f, n_f b_f], non-nested n_bins, a feats_out above n_res); a null
 * player_lo or player_hi; a window with lo < 0 or lo >= hi (the player's index is named); n_bins[f] > 512; mixed donor pointers. */
int cf_mark_fine_coalitions(cf_handle* h, const cf_batch* batch, const cf_mark_fine_opts* opts, const uint32_t* keep, int n_coal, float* logits,
                            void* stream);
/* Exact Shapley values of P <= 16 fine window players: all 2^P words through the routine above (word m at column m; feats_out, if
 * given, [B, 2^P, ...]), then the k_shapley of cf_mark_shapley.  phi [B, P, n_out]; logits_all [B, 2^P, n_out] or NULL (the
 * handle-owned buffer).  A null player's phi is exactly 0.  fwd = that of cf_mark_fine_coalitions with n_coal = 2^P, plus 1.
 * Refusals as above (null phi, n_players > 16). */
int cf_mark_fine_shapley(cf_handle* h, const cf_batch* batch, const cf_mark_fine_opts* opts, float* phi, float* logits_all, void* stream);
/* Pairwise Shapley interaction indices of P <= 16 fine window players (see cf_shapley_interactions_from_rows): cf_mark_fine_shapley's
 * rows (feats_out, if given, [B, 2^P, ...]), then k_shapley_pairs (and k_shapley with the optional phi).  inter [B, P, P, n_out]; a null
 * player's row and column are exactly 0.  fwd = that of cf_mark_fine_coalitions with n_coal = 2^P, plus 1 per reducer launched (1, or 2
 * with phi).  Refused by name, before anything is launched: what cf_mark_fine_shapley refuses (phi may be null), a null inter, an index
 * other than the two constants, n_players < 2. */
int cf_mark_fine_shapley_interactions(cf_handle* h, const cf_batch* batch, const cf_mark_fine_opts* opts, int index, float* inter, float* phi,
                                      float* logits_all, void* stream);
/* Permutation-sampled Shapley values of the fine window players: perms, the R = 2 + n_perm * (P - 1) rows per gene, k_perm_shapley,
 * phi, the optional se and logits_rows and the launch count are those of cf_mark_shapley_sampled; a null player's phi and se are
 * exactly 0.  Refusals as above and as there. */
int cf_mark_fine_shapley_sampled(cf_handle* h, const cf_batch* batch, const cf_mark_fine_opts* opts, const uint8_t* perms, int n_perm, float* phi,
                                 float* se, float* logits_rows, void* stream);
/* Permutation-SAMPLED pairwise Shapley interaction indices of a few FOCAL players of a wide game (up to 128 players): for the players
 * that carry the prediction, which other players do they interact with?  perms as in cf_mark_shapley_sampled; focal: HOST ints
 * [n_focal], distinct players.  For focal player i and order pi, o = pi with i removed, T_k the first k players of o, r the position of
 * i in pi.  For j = o[a]:
 *   d(j) = (v(T_{a+1} + i) - v(T_{a+1})) - (v(T_a + i) - v(T_a))         three fp32 subtractions, in this grouping
 *   CF_INTERACTION_SII  s_q = d(j)             (T_a has the law a! (P - 2 - a)! / (P - 1)! over uniform orders: unbiased)
 *   CF_INTERACTION_STI  s_q = w_a d(j),  w_a = 2 (P - 1 - a) / P in double, rounded to fp32; one rounded product
 *   inter[b, f, j] = (sum_q s_q) / n_perm,   se[b, f, j] = sqrt(sum_q (s_q - inter)^2 / (n_perm (n_perm - 1)))    0 for n_perm = 1
 * in the summation order of k_perm_shapley, no atomics: the result does not depend on max_batch.  The diagonal j = focal[f]: SII the
 * bits of cf_mark_shapley_sampled's phi and se on the same orders; STI v({i}) - v(nobody), se 0.  If i or j is a null player d(j) = 0
 * bit for bit: inter and se are exactly 0.  The estimate is NOT symmetric: inter[i, j] from focal i and inter[j, i] from focal j are
 * different samples.  Its sampling error is what se reports; the library does not bound it.
 * Rows per gene (R of them, through the routine of cf_mark_coalitions_wide):
 *   the R0 = 2 + n_perm (P - 1) rows of cf_mark_shapley_sampled, unchanged, then per focal player f in the order given:
 *   {i} alone;  everybody but i;  then per order q the rows T_k + i, k = 1 .. r - 1, then the rows T_k, k = r + 1 .. P - 2
 * (T_k = pi[:k] for k <= r and T_k + i = pi[:k + 1] for k >= r are rows of the leading block): P - 3 rows per (f, q) for
 * 1 <= r <= P - 2, P - 2 for r = 0 or P - 1.  The host builds the words and a column table col[f, q, k, {without, with}] (uint32) that
 * travels in the word table behind the inverse permutations; k_perm_pairs reads columns through it.
 * inter, se [B, n_focal, P, n_out]; se NULL: not computed.  phi, phi_se [B, P, n_out] or NULL: the sampled Shapley values of every
 * player from the leading rows (k_perm_shapley; the bits of cf_mark_shapley_sampled).  logits_rows [B, R, n_out] or NULL.
 * fwd = that of cf_mark_coalitions_wide with n_coal = R, plus 1, plus 1 if phi is given.
 * Refused by name, before anything is launched: what cf_mark_shapley_sampled refuses (phi may be null), null inter, null focal,
 * n_focal outside 1..P, a focal index outside 0..P-1 or repeated (its position is named), index outside {SII, STI}, P < 2, phi_se
 * without phi, more than 2^30 coalition words. */
int cf_mark_shapley_interactions_sampled(cf_handle* h, const cf_batch* batch, const cf_mark_wide_opts* opts, const uint8_t* perms, int n_perm,
                                         const int* focal, int n_focal, int index, float* inter, float* se, float* phi, float* phi_se,
                                         float* logits_rows, void* stream);
/* The same for window players (cf_mark_window_coalitions' game) and fine window players (cf_mark_fine_coalitions' game; feats_out
 * then holds R rows per gene). */
int cf_mark_window_shapley_interactions_sampled(cf_handle* h, const cf_batch* batch, const cf_mark_window_opts* opts, const uint8_t* perms,
                                                int n_perm, const int* focal, int n_focal, int index, float* inter, float* se, float* phi,
                                                float* phi_se, float* logits_rows, void* stream);
int cf_mark_fine_shapley_interactions_sampled(cf_handle* h, const cf_batch* batch, const cf_mark_fine_opts* opts, const uint8_t* perms,
                                              int n_perm, const int* focal, int n_focal, int index, float* inter, float* se, float* phi,
                                              float* phi_se, float* logits_rows, void* stream);
/* The operator on a caller's device table rows [B, R, n_out] in the layout above (for instance a kept logits_rows), 2 <= P <= 128: no
 * batch, no chunk workspace; of the handle only the word table is used (the inverse permutations and col).  fwd = 1, plus 1 if phi is
 * given.  Refusals: null handle / rows, B < 1, n_out < 1, P > 128 and those above. */
int cf_perm_interactions_from_rows(cf_handle* h, const float* rows, int B, int P, int n_out, const uint8_t* perms, int n_perm, const int* focal,
                                   int n_focal, int index, float* inter, float* se, float* phi, float* phi_se, void* stream);
/* Greedy player SELECTION (interpretation): which few players are enough on their own to make this call, and in what order does the
 * prediction fall apart when players are taken away?  The sufficient-input-subset question: backward selection, then the smallest
 * suffix of the removal order that still carries the prediction, with the deletion / insertion curve that comes with it.
 * Deterministic, no sampling error; P (P + 1) / 2 + 1 forwards per gene (2,017 at P = 63).
 *   mode CF_BACKSELECT_BACKWARD  the path starts from everybody and every move REMOVES one player
 *   mode CF_BACKSELECT_FORWARD   the path starts from nobody and every move ADDS one player
 * Round t = 0 .. P - 2 evaluates, per gene, the P - t coalitions one move away from the gene's current one (candidates in ascending
 * player order) and moves to the candidate with the largest key s_b * v[target], an fp32 product:
 *   s_b      +1 if everybody[target] >= nobody[target], else -1; direction = +1 / -1 overrides it for every gene
 *   ties     the candidates are scanned in ascending player index with strict >: the lowest index wins.  A NaN key counts as -inf;
 *            if every key is -inf the lowest index wins
 * The last move is forced.  order[b, i] is the player of move i; values[b, t] the logits after t moves (values[b, 0] the start row,
 * values[b, P] the other end row: both carry the bits of the nobody / everybody rows, everybody = cf_forward(save = 0)).
 *   thr      threshold[b] if given, else nobody + frac (everybody - nobody) on column target, evaluated as fp32
 *            add(nobody, mul(frac, sub(everybody, nobody))), each operation rounded
 *   sufficient   a set with value v is sufficient when s_b * (v - thr) >= 0 (fp32 sub, then mul; a NaN is not); the set of everybody
 *            is sufficient by definition
 *   size[b]  the smallest k such that the set of k players on the path is sufficient, counted from the small end (the path need not
 *            be monotone); subset[b] that set, kw = ceil(P / 32) words, bit p % 32 of word p / 32 = player p
 * Backward mode: the subset is the LAST size[b] players of order[b] (the sufficient input subset); forward mode: the first size[b]. */
#define CF_BACKSELECT_BACKWARD 0
#define CF_BACKSELECT_FORWARD 1
typedef struct cf_backselect_opts {
    int mode;                                        /* CF_BACKSELECT_BACKWARD / CF_BACKSELECT_FORWARD */
    int target;                                      /* the logit column of the key and of the threshold, 0 .. n_out - 1 */
    int direction;                                   /* 0: s_b from the two end rows; +1 / -1: for every gene */
    float frac;                                      /* finite; read when threshold is NULL */
    const float* threshold;                          /* device [B] or NULL */
} cf_backselect_opts;                                /* 24 bytes */
typedef struct cf_backselect_out {                   /* device buffers */
    int* order;                                      /* [B, P] */
    float* values;                                   /* [B, P + 1, n_out] */
    int* size;                                       /* [B] */
    uint32_t* subset;                                /* [B, kw] */
    float* rows;                                     /* optional: every evaluated row, round-major -- block 0 [B, 2, n_out] (nobody,
                                                        everybody), block 1 + t [B, P - t, n_out], t = 0 .. P - 2: B (P (P + 1) / 2 + 1)
                                                        rows.  NULL: the handle-owned buffer of cf_pcre_shapley.  Not read by
                                                        cf_backselect_from_rows */
    float* threshold;                                /* optional [B]: thr as used */
    int* direction;                                  /* optional [B]: s_b as used */
} cf_backselect_out;                                 /* 56 bytes */
/* cf_mark_backselect: the game of cf_mark_coalitions_wide (players, both rules; with at most 32 players one word per coalition, the
 * narrow game).  The two end rows run first (nobody, then everybody).  Then per round t one k_backselect_step -- one workgroup per gene:
 * the pick among the gene's rows of round t - 1 and the gene's P - t candidate words of round t, written into a per-gene word table on
 * the device -- and the B (P - t) rows of the round (gene-major) through the chunk loop of cf_mark_coalitions_wide, whose expand kernel
 * reads gene b's words at b * P * kw; one more k_backselect_step makes the last pick, k_backselect_finish the rest.  The host sees no
 * logit: no synchronisation and no copy to the host inside the call.
 *   cf_launch_counts fwd = P + 1 + (1 + n_fwd) * (ceil(2 B / max_batch) + sum over t = 0 .. P - 2 of ceil(B (P - t) / max_batch)),
 *   n_fwd = what cf_forward(save = 0) issues.
 * The current coalitions, the candidate words and s_b travel in the device table the handle owns, behind the player words (grown on
 * demand); no other device buffer is added.  Deterministic (no atomics); k_attc2's regions per workgroup are chosen as for the
 * caller's B genes, so the result does not depend on max_batch.  Every row carries the bits cf_mark_coalitions_wide gives for its word.
 * Overwrites the activations a cf_forward(save >= 1) kept.  Parameters, gradients and moments are untouched.
 * Refused by name, before anything is launched: what cf_mark_coalitions_wide refuses (n_players < 1 among it); null bopts / out; a
 * mode or direction outside its values; target outside [0, n_out); a frac that is not finite; a null order, values, size or subset. */
int cf_mark_backselect(cf_handle* h, const cf_batch* batch, const cf_mark_wide_opts* opts, const cf_backselect_opts* bopts,
                       const cf_backselect_out* out, void* stream);
/* The same for window players (cf_mark_window_coalitions' game) and fine window players (cf_mark_fine_coalitions' game; a non-null
 * feats_out is refused: the rounds have different row counts). */
int cf_mark_window_backselect(cf_handle* h, const cf_batch* batch, const cf_mark_window_opts* opts, const cf_backselect_opts* bopts,
                              const cf_backselect_out* out, void* stream);
int cf_mark_fine_backselect(cf_handle* h, const cf_batch* batch, const cf_mark_fine_opts* opts, const cf_backselect_opts* bopts,
                            const cf_backselect_out* out, void* stream);
/* The same selection and finish on a caller's device table rows [B, 2^P, n_out], word m at column m, 1 <= P <= 16 (the logits_all of
 * any exact *_shapley call): k_backselect_table, one workgroup per gene runs all rounds; no forward, no batch, no workspace, nothing
 * of the handle is read.  subset is [B] (one word).  fwd = 1.  Refusals: null handle / rows, B < 1, P outside 1..16, n_out < 1 and
 * those of bopts / out above. */
int cf_backselect_from_rows(cf_handle* h, const float* rows, int B, int P, int n_out, const cf_backselect_opts* bopts, const cf_backselect_out* out,
                            void* stream);
/* torch.optim.AdamW.step (train.py:157, 196): decoupled weight decay, bias correction
 * from `step` (1-based), over [0, n_active). */
int cf_adamw_step(cf_handle* h, float lr, float beta1, float beta2, float eps, float weight_decay,
                  long long step, void* stream);
/* The same update restricted to a bucket mask (elementwise, so two calls with complementary masks and the same
 * `step` equal one cf_adamw_step). */
int cf_adamw_step_part(cf_handle* h, float lr, float beta1, float beta2, float eps, float weight_decay,
                       long long step, int buckets, void* stream);

/* EmbeddingTransformer.forward's first return value (net.py:57-59): the embedding of EVERY promoter bin, out[r] =
 * [B, 1, L_r, 128] (a NULL entry is skipped).  The training path never needs it (only the centre row is consumed,
 * net.py:59, 138); it is computed by the all-rows path -- token embeddings + the dense transformer layer of
 * cf_op_dense_layer_fwd per Embedding layer -- which is also what cf_forward / cf_backward run for the whole Embedding
 * stack when embed.n_layers > 1 (keys and values of a layer are then all rows of the previous one).  Pad masks: the full
 * [B,1,1,L,L] tensor (mask stride L*L) is honoured entry by entry; a compact centre row is expanded as the dataset's
 * structured mask not(valid x valid).  Forward only. */
int cf_embed_full(cf_handle* h, const cf_batch* batch, float* const* out, void* stream);

/* ---- hipGraph capture ---------------------------------------------------------------- */
/* The launch sequence of a step is static, so it can be captured once and replayed: every
 * library call issued on `stream` between begin and end is recorded (nothing executes);
 * cf_graph_launch replays it.  Pointers are baked in: replay reads the same device buffers,
 * so callers refill those buffers (hipMemcpyAsync) instead of passing new ones. */
int cf_capture_begin(cf_handle* h, void* stream);
int cf_capture_end(cf_handle* h, void* stream, int* graph_id);
int cf_graph_launch(cf_handle* h, int graph_id, void* stream);

/* ---- introspection (tests / profiling) -------------------------------------------- */
/* HIP-event timing of one eagerly launched kernel ("k_wgrad", "k_colsum", "k_adamw", "k_reg_fwd", "k_reg_bwd", "k_trunk_fwd", "k_trunk_bwd"; NULL
 * = off): events are recorded on the launch stream around every launch of that kernel;
 * cf_timing_read waits for them and returns the summed duration and the launch count. */
int cf_timing_select(cf_handle* h, const char* kernel);
int cf_timing_read(cf_handle* h, float* total_ms, int* count);
/* Under capture the selected kernel (k_reg_fwd / k_reg_bwd) is not recorded: the capture is split around it and
 * cf_graph_launch replays [piece 1] -> the kernel, eagerly, between two events -> [piece 2].  Select the kernel
 * before cf_capture_begin. */
/* Executed flops (2*M*N*K summed over the tile table) of one k_wgrad launch at batch B. */
double cf_wgrad_flops(cf_handle* h, int B);
/* Algorithmic flops (2 * MAC over the valid rows) of one launch of "k_wgrad", "k_reg_fwd", "k_reg_bwd", "k_trunk_fwd" or
 * "k_trunk_bwd" (the centre-row trunk: row products + two-pass centre-row attention of the Embedding row and the i_max Pairwise
 * rows of every gene and resolution; riders of the launch are not counted). */
double cf_kernel_flops(cf_handle* h, const char* kernel, int B);
/* Compute units of the device the handle lives on (hipDeviceAttributeMultiprocessorCount): callers that add rider workgroups to
 * a launch of one-per-CU workgroups (cf_rider_arm) size them with it. */
int cf_cu_count(cf_handle* h);
/* Regions per workgroup (1, 2, 4 or 8) that the stand-alone centre-row attention launch takes for n_sequences sequences, forward
 * and backward alike: n_sequences = B for the Embedding launch, B * i_max for every Pairwise launch.  1 is the one-region kernel
 * (k_attc1), the others are k_attc2<., 2 / 4 / 8>; a launch whose n_sequences is no multiple of the answer ends in a workgroup with
 * fewer regions.  0 where the handle does not use the gene-batched kernel (other head counts or row widths, rows too long for its
 * LDS image).  h == NULL: the rule with the default cap, no device needed.  Read-only; the fused trunk does not go through this
 * launch.  Tests use it to assert which kernel a batch size reaches. */
int cf_attc_regions(cf_handle* h, int n_sequences);
/* Copies a named workspace buffer (e.g. "E0.qt", "dP2.1.xbar") to dst (device);
 * *n_floats receives its size; dst may be NULL to query. */
int cf_debug_copy(cf_handle* h, const char* name, float* dst, long long* n_floats, void* stream);
/* Names of all workspace buffers, '\n' separated (host string owned by the handle). */
const char* cf_debug_names(cf_handle* h);
/* cf_backward_reduce_part(reduce_buckets) and cf_adamw_step_part(adam_buckets) as ONE launch: the tiles of the bucket under
 * reduction and the optimiser stream of the OTHER bucket (whose gradients must be complete, and all-reduced under data
 * parallelism) run side by side.  reduce_buckets: exactly one bucket; adam_buckets: disjoint from it.  Same results as the two
 * separate calls, bit for bit.  Not capturable (the optimiser's scalars are launch arguments). */
int cf_reduce_adamw_part(cf_handle* h, int B, int reduce_buckets, float lr, float beta1, float beta2, float eps,
                         float weight_decay, long long step, int adam_buckets, void* stream);
/* cf_backward_reduce_part(bucket) with cf_adamw_step_part(bucket) folded into it: the tile that finishes a gradient element applies
 * torch.optim.AdamW's update (train.py:157, 194) to the parameter and moment elements at the same offset -- one launch, no second
 * pass over gradients and optimiser state.  For single-GPU training (under data parallelism the all-reduce stands between the two).
 * bucket: one bucket or both (CF_BUCKET_REG | CF_BUCKET_PE: every tile of the step in one launch, behind the whole backward pass);
 * keep_grads != 0 also stores the gradients (otherwise the flat gradient buffer keeps what it held).  Same
 * parameters / moments as the two separate calls, bit for bit.  Fails when the all-rows Embedding path is active (embed n_layers > 1:
 * its gradients are written outside the reduction tables).  Not capturable (the optimiser's scalars are launch arguments). */
int cf_reduce_opt_part(cf_handle* h, int B, int bucket, float lr, float beta1, float beta2, float eps, float weight_decay,
                       long long step, int keep_grads, void* stream);
/* Arms "riders" for the NEXT cf_backward_part(parts & 4) call: while the Pairwise + Embedding backward occupies 192 of the 256 CUs
 * with latency chains, an extra row of workgroups of the same launch reduces up to max_tiles leading weight-gradient tiles of the
 * Regulation + head bucket (they depend on the Regulation backward only) and applies this step's AdamW update in their epilogues,
 * as cf_reduce_opt_part does.  The cf_reduce_opt_part call that follows (same `step`, a mask with CF_BUCKET_REG) skips those tiles;
 * it must follow, and nothing else may read or reduce that bucket in between.  Requires the fused trunk kernels (default
 * configuration); not capturable.  Same parameters and moments as without riders, bit for bit. */
int cf_rider_arm(cf_handle* h, float lr, float beta1, float beta2, float eps, float weight_decay, long long step, int keep_grads,
                 int max_tiles);
/* Number of kernels the LAST forward / backward (chain pieces + bucket reductions) / optimiser step launched, counted at the
 * launch sites (zero before the first call; calls replayed from a graph do not pass the host code and leave the counts
 * of the capture pass). */
int cf_launch_counts(cf_handle* h, int* fwd, int* bwd, int* opt);

/* ---- standalone operators (same kernels, for unit tests and micro-benchmarks) ------ */
/* C[M,N] = A[M,K] . W[N,K]^T (+ bias[N]) (relu)      -- the Linear of modules.py:20-24 */
int cf_op_linear(const float* A, const float* W, const float* bias, float* C, int M, int N, int K,
                 int relu, void* stream);
/* dW[N,K] = dY[M,N]^T . X[M,K]                       -- its weight gradient           */
int cf_op_wgrad(const float* dY, const float* X, float* dW, int M, int N, int K, void* stream);
/* dX[M,K] = dY[M,N] . W[N,K]                         -- its input gradient            */
int cf_op_dgrad(const float* dY, const float* W, float* dX, int M, int N, int K, void* stream);

/* ---- dense (all rows) transformer layer, forward --------------------------------------- */
/* One AttentionBlock / PairwiseAttentionBlock over ALL query rows (modules.py:104-112, 198-208), d_emb = d_model =
 * 128, 2 heads of 64:   a = Attn(x_q Wq^T, x_kv Wk^T, x_kv Wv^T);  y1 = LN(x_q + a Wo^T + bo);
 * y = LN(y1 + relu(y1 W1^T + b1) W2^T + b2).  Self-attention: x_q = x_kv and (wq, wkv) are the row blocks
 * [0,128) and [128,384) of `att.weight`; pairwise: wq = p_att.weight, wkv = c_att.weight.  (The training path of the
 * model never needs all rows; these operators serve the stress configuration and consumers of full embeddings.)  `ws` is a device
 * workspace of cf_op_dense_layer_workspace(...) floats; masks as in cf_op_attention_fwd. */
typedef struct cf_dense_layer {
    const float *wq, *wkv;            /* [128,128], [256,128] */
    const float *wo, *bo, *ln1_g, *ln1_b;
    const float *w1, *b1, *w2, *b2, *ln2_g, *ln2_b;
    int d_ff;                         /* 128 or 256 */
} cf_dense_layer;
long long cf_op_dense_layer_workspace(int N, int Lq, int Lk, int d_ff);
int cf_op_dense_layer_fwd(const cf_dense_layer* w, const float* x_q, const float* x_kv, const unsigned char* qvalid,
                          const unsigned char* kvalid, const unsigned char* mask, int N, int Lq, int Lk, float* y,
                          float* ws, void* stream);
/* Training form: cf_op_dense_layer_fwd_train keeps the activations the backward pass needs in `ws`
 * (cf_op_dense_layer_train_workspace floats); cf_op_dense_layer_bwd turns dy [N*Lq, 128] into dx_q [N*Lq, 128],
 * dx_kv [N*Lk, 128] (a self-attention caller adds the two) and the gradients of all twelve tensors (`grads`, same
 * shapes as the weights, overwritten).  `tables`: device scratch of 4 MiB for the tile tables.  Weight gradients
 * are split-K sums in a fixed order: bit-reproducible.  The tables are written by a device kernel from by-value arguments:
 * nothing synchronises, the call can be captured. */
typedef struct cf_dense_layer_grads {
    float *wq, *wkv, *wo, *bo, *ln1_g, *ln1_b, *w1, *b1, *w2, *b2, *ln2_g, *ln2_b;
} cf_dense_layer_grads;
long long cf_op_dense_layer_train_workspace(int N, int Lq, int Lk, int d_ff);
int cf_op_dense_layer_fwd_train(const cf_dense_layer* w, const float* x_q, const float* x_kv,
                                const unsigned char* qvalid, const unsigned char* kvalid, const unsigned char* mask,
                                int N, int Lq, int Lk, float* y, float* ws, void* stream);
int cf_op_dense_layer_bwd(const cf_dense_layer* w, const float* x_q, const float* x_kv, const unsigned char* qvalid,
                          const unsigned char* kvalid, const unsigned char* mask, int N, int Lq, int Lk,
                          const float* dy, float* dx_q, float* dx_kv, const cf_dense_layer_grads* grads, float* ws,
                          float* tables, void* stream);

/* ---- input pipeline ------------------------------------------------------------------ */
/* ChromoformerDataset._bin_and_pad + strand flip (data.py:68-113) on the device: per region, the window
 * [col0, col0 + ncols) of the raw fp16 signal [n_feats, ld] is averaged over bins of `bin_size` samples (short last
 * bin included), passed through log(1 + x), centred in n_bins_out bins (ceil-left / floor-right zero padding) and
 * mirrored if `flip`; out receives [n_bins_out, n_feats] fp32 (the slot of the region in a batch / store array),
 * mask (optional) the pad bytes [n_bins_out] (1 = padding).  `jobs` is a DEVICE array.  The caller guarantees
 * ceil(ncols / bin_size) <= n_bins_out (the reference raises for longer regions, data.py:168-169). */
typedef struct cf_bin_job {
    const void* raw;
    long long ld;
    int col0, ncols;
    int flip, reserved;
    float* out;
    unsigned char* mask;
} cf_bin_job;
int cf_bin_regions(const cf_bin_job* jobs, int n_jobs, int n_feats, int bin_size, int n_bins_out, void* stream);
/* All resolutions of every region in ONE launch and -- when the bin sizes nest (each a multiple of the next, the finest a
 * multiple of 4 samples: the default 2000 / 500 / 100) and the rows are 8-byte aligned -- ONE pass over the raw bytes: the
 * reference calls _bin_and_pad once per bin size on the same window (data.py:134-140, 168-176 -> 68-100); here a wave reads a
 * coarsest bin's samples once and derives the finer resolutions' sums from the same chunk sums.  bin_sizes / n_bins_out:
 * host arrays [n_res], coarsest resolution first; out[r] / mask[r] of a job as in cf_bin_job, per resolution; max_cols: an
 * upper bound of `ncols` over the jobs (sizes the launch).  Same results as n_res calls of cf_bin_regions up to the order
 * of the fp32 additions inside a bin (1e-7 relative).  Other configurations / unaligned rows: the per-resolution walk of
 * cf_bin_regions inside the same launch. */
typedef struct cf_bin_job_multi {
    const void* raw;
    long long ld;
    int col0, ncols;
    int flip, reserved;
    float* out[3];
    unsigned char* mask[3];
} cf_bin_job_multi;
int cf_bin_regions_multi(const cf_bin_job_multi* jobs, int n_jobs, int n_feats, int n_res, const int* bin_sizes,
                         const int* n_bins_out, int max_cols, void* stream);
/* Its backward: the gradient with respect to the RAW signal (raw-signal saliency).  With dfeat[r][p, f] the gradient with
 * respect to out[r] of the forward job (batch layout: centred, padded, mirrored if `flip`), bin g of resolution r holding
 * cnt samples of mean m and written to row p of out[r],
 *     draw[f, s] = sum_r dfeat[r][p_r(s), f] / (cnt_{r,g_r(s)} * (1 + m_{r,g_r(s)}))        s in [0, ncols)
 * the exact chain rule through mean -> log(1 + x) -> padding -> mirror (data.py:68-113), in raw (genomic) orientation,
 * window-relative, fp32.  Pad rows of dfeat are never read; a null dfeat[r] counts as zero; times_input != 0 multiplies by
 * (float)raw[f, col0 + s] (gradient x input).  Exactly the elements draw[f * ld_out + s], s < ncols, are written, each
 * once: no atomics, results are bit-reproducible.  Where 1 + m <= 0 the result is inf / NaN, as the reference's log
 * gives under autograd; preprocessed signals are non-negative.  Nested bin sizes with 8-byte aligned raw rows, a 16-byte
 * aligned draw and ld_out % 4 == 0 read the raw bytes once (the forward's sums in the forward's order of additions) and
 * write 16 bytes per lane; anything else takes a per-region walk inside the same launch.  Arguments as the forward's;
 * ld_out < ncols and ncols > max_cols are refused (the job table is read back for that: the call synchronises `stream`). */
typedef struct cf_bin_grad_job {
    const void* raw;
    long long ld;
    int col0, ncols;
    int flip, reserved;
    const float* dfeat[3];          /* [n_bins_out[r], n_feats], coarsest resolution first */
    float* draw;                    /* [n_feats, ld_out] */
    long long ld_out;               /* >= ncols */
} cf_bin_grad_job;                  /* 72 bytes */
int cf_bin_regions_multi_backward(const cf_bin_grad_job* jobs, int n_jobs, int n_feats, int n_res, const int* bin_sizes,
                                  const int* n_bins_out, int max_cols, int times_input, void* stream);
/* Per-bin integrated gradients spread over the difference of two raw signals (k_bin_spread_diff).  With cmean[r][p, f] = C of
 * cf_integrated_gradients_raw_donor in the layout of out[r] of the forward job, g_r(s) = s / b_r, p_r the centred (mirrored if `flip`)
 * row of bin g_r and cnt_r = min((g_r + 1) b_r, ncols) - g_r b_r its sample count,
 *     draw[f, s] = (x[f, col0 + s] - xd[f, col0 + s]) * ((C_0[p_0(s), f] / cnt_0 + C_1[p_1(s), f] / cnt_1) + C_2[p_2(s), f] / cnt_2)
 * coarsest resolution first, fp32, every operation rounded; the shares of a bin's samples sum to its attr.  Raw (genomic)
 * orientation, window-relative.  A sample past the last real bin of a resolution gets nothing from it.  Exactly the elements
 * draw[f * ld_out + s], s < ncols, are written, each once: no atomics, bit-reproducible.  Nested bin sizes (the finest a multiple of
 * 4) with 8-byte aligned rows of both signals, a 16-byte aligned draw and ld_out % 4 == 0 move 4 bytes in and 4 bytes out per
 * sample with 16-byte stores; anything else takes a per-sample walk inside the same launch.  `jobs` is a DEVICE array; the other
 * arguments as the backward's.  Refused: ld_out < ncols, ncols > max_cols, a window that does not fit its rows, null raw / draw (the
 * job table is read back for that: the call synchronises `stream`). */
typedef struct cf_bin_spread_job {
    const void* raw;        long long ld;          /* gene's fp16 [n_feats, ld]                                 */
    const void* raw_donor;  long long ld_donor;    /* donor's, same col0 / ncols; NULL: the zero signal         */
    int col0, ncols, flip, reserved;
    const float* cmean[3];                         /* [n_bins_out[r], n_feats], coarsest first; NULL counts as 0 */
    float* draw;            long long ld_out;
} cf_bin_spread_job;                               /* 88 bytes */
int cf_bin_spread_difference(const cf_bin_spread_job* jobs, int n_jobs, int n_feats, int n_res, const int* bin_sizes,
                             const int* n_bins_out, int max_cols, void* stream);

/* ---- resident split, batch gather inside the step graph --------------------------------- */
/* The binned genes of a split, resident in HBM (what chromoformer_amd.data.GeneStore builds with cf_bin_regions):
 * the arrays of cf_batch with a leading gene dimension, pad masks as compact centre rows, one interaction mask per
 * gene (it is the same at every resolution, data.py:200-203). */
typedef struct cf_store {
    long long n_genes;
    const float*   promoter_feats[CF_MAX_RES];      /* [n,1,L,F]                       */
    const float*   pcre_feats[CF_MAX_RES];          /* [n,S,L,F]                       */
    const uint8_t* promoter_mask[CF_MAX_RES];       /* [n,L]    centre query row       */
    const uint8_t* pcre_mask[CF_MAX_RES];           /* [n,S,L]  centre query row       */
    const uint8_t* interaction_mask;                /* [n,T,T]                         */
    const float*   interaction_freq;                /* [n,T,T]                         */
    const void*    labels;                          /* int64 [n] (n_out = 2) or float [n] */
} cf_store;
/* The DataLoader and the per-tensor .cuda() copies of a step (train.py:137-140, 171-177) as ONE capturable launch:
 * copies genes order[cursor[0] * B ... + B) of `store` into the batch buffers `dst` (which must use compact mask
 * rows, stride L, and are written despite the const in cf_batch) and their labels into labels_dst, then advances
 * cursor[0] (a second, one-thread launch).  `order` (int32, batch-major) and `cursor` (int32[4]) are device memory: a
 * replayed graph walks the epoch without any host involvement.  cursor[0] = next batch (zero it whenever a new order is
 * uploaded), cursor[1] = number of batches in `order` (the bound: a call with cursor[0] >= cursor[1] copies nothing, does
 * not advance and sets bit 0 of cursor[2]; a gene index outside [0, store->n_genes) is skipped and sets bit 1),
 * cursor[2] = error flags (sticky until the caller clears them), cursor[3] reserved. */
int cf_gather_batch(cf_handle* h, const cf_store* store, const int* order, int* cursor, const cf_batch* dst,
                    void* labels_dst, void* stream);
/* cf_gather_batch for the batch of a TRAINING step: launches nothing; the cf_forward / cf_forward_train that must follow on the same
 * stream (with `dst` as its batch) copies the genes in the launch that refreshes its tiled weight copies -- neither depends on the other --
 * and its trunk launch advances the cursor: the three launches in front of every step of the training loop become one.  Configurations
 * without the fused trunk kernels: the forward issues the two gather launches itself, as cf_gather_batch would. */
int cf_gather_batch_fwd(cf_handle* h, const cf_store* store, const int* order, int* cursor, const cf_batch* dst,
                        void* labels_dst, void* stream);
/* Appends the step's logits [B, n_out], labels [B] and loss to per-epoch device logs at row cursor[0] - 1 (capturable;
 * what the loop's running metrics, train.py:198-232, read every tenth step instead of cloning tensors every step).
 * The logs must hold cursor[1] rows; nothing is written for a step past the epoch (cursor[2] bit 0). */
int cf_record_step(cf_handle* h, const int* cursor, const float* logits, const void* labels, const float* loss, int B,
                   float* logits_log, void* labels_log, float* loss_log, void* stream);
/* cf_record_step without a launch of its own: the cf_backward_part(parts & 4) that must follow on the same stream writes the rows at the
 * start of the Pairwise + Embedding backward launch (the step's loss is final by then). */
int cf_record_step_bwd(cf_handle* h, const int* cursor, const float* logits, const void* labels, const float* loss, int B,
                       float* logits_log, void* labels_log, float* loss_log, void* stream);

/* Dense attention core with ALL query rows (MultiHeadAttention._attention, modules.py:58-77;
 * PairwiseMultiHeadAttention, modules.py:170-188), head width 64:
 *     O = softmax(masked_fill(Q K^T / sqrt(64), mask, -1e9)) V        per (sequence n, head h)
 * q, k, v, o are [N, L, ld*] row-major with head h in columns [64 h, 64 h + 64) -- i.e. the chunks of the
 * reference's fused projection can be passed in place (pointer offset + ld).  mask = not (qvalid x kvalid) from
 * two byte vectors (1 = real bin; null = all real), or an arbitrary byte mask [N, Lq, Lk] (1 = masked).
 * stats [N, H, Lq, 2] receives the softmax row statistics the backward pass needs.  The training path does not
 * call this (it evaluates the centre query row only); it serves the 800-bin stress configuration and consumers
 * of full-length embeddings. */
typedef struct cf_attn_shape {
    int N, H, Lq, Lk;
    int ldq, ldk, ldv, ldo;
} cf_attn_shape;
int cf_op_attention_fwd(const cf_attn_shape* shape, const float* q, const float* k, const float* v,
                        const unsigned char* qvalid, const unsigned char* kvalid, const unsigned char* mask,
                        float* o, float* stats, void* stream);
/* Its backward: dq, dk, dv in the layouts of q, k, v (only the 64 H columns of the heads are written);
 * delta_ws: workspace of N*H*Lq floats.  No atomics: bit-reproducible. */
int cf_op_attention_bwd(const cf_attn_shape* shape, const float* q, const float* k, const float* v,
                        const unsigned char* qvalid, const unsigned char* kvalid, const unsigned char* mask,
                        const float* o, const float* stats, const float* d_o, float* dq, float* dk, float* dv,
                        float* delta_ws, void* stream);

/* Round 4.  The fused optimiser (cf_reduce_opt_part over CF_BUCKET_PE) keeps the tiled copies of the Embedding + Pairwise weights fresh:
 * its epilogue writes every stepped element in both layouts and forward passes skip the re-tiling of those tensors (no launch in front of
 * a training step, or one that only gathers the batch).  Contract: whoever else writes parameters calls cf_params_changed before the next
 * forward pass, which then re-tiles once (cf_retile_early does it at once, e.g. before replaying a hipGraph captured without it).  cf_bind
 * and the library's separate AdamW launches clear the flag themselves.  cf_keep_tiled(h, 1) returns -1 where the reduction tiles do not
 * cover those tensors (embed n_layers > 1, no gradient buffer bound).  No reference counterpart (train.py:194 steps torch parameters). */
/* cf_gather_batch for a training loop without a launch in front of a step: cf_gather_batch_next stores its arguments and the cf_reduce_opt_part
 * that follows carries the copy of the NEXT step's batch behind its tiles; cf_gather_batch_only copies now (the first step of an epoch).  In
 * both cases the cursor is advanced by the forward pass that follows (its trunk launch).  Replaces train.py:137-140, 171-177 as cf_gather_batch does. */
int cf_gather_batch_next(cf_handle* h, const cf_store* store, const int* order, int* cursor, const cf_batch* dst, void* labels_dst, void* stream);
int cf_gather_batch_only(cf_handle* h, const cf_store* store, const int* order, int* cursor, const cf_batch* dst, void* labels_dst, void* stream);
int cf_keep_tiled(cf_handle* h, int on);
int cf_params_changed(cf_handle* h);
int cf_retile_early(cf_handle* h, void* stream);

/* ---- training on a frozen trunk ------------------------------------------------------------ */
/* The trunk = every Embedding and Pairwise tensor (CF_BUCKET_PE); the top = the Regulation stacks and fc_head (CF_BUCKET_REG).  For fixed
 * trunk weights the Regulation input of a gene -- per resolution [T, d_emb], T = i_max + 1 -- depends on the gene alone: it can be
 * computed once (cf_trunk_outputs), kept, and a training step can start from it (cf_forward_train_x0).  No reference counterpart
 * (train.py trains every parameter).
 *
 * cf_trunk_outputs: the trunk part of cf_forward(save = 0) -- every configuration cf_forward accepts -- then ONE launch that copies the
 * Regulation input of the batch's genes to x0[r], [B, T, d_emb] (16-byte aligned; r < n_res).  Overwrites the activations a
 * cf_forward(save >= 1) kept: no cf_backward* may follow without a new saving forward. */
int cf_trunk_outputs(cf_handle* h, const cf_batch* batch, float* const* x0, void* stream);
/* cf_forward_train from the Regulation input: reads B, interaction_mask[r] and interaction_freq of `batch` (its other fields may be
 * null) and x0[r], [B, T, d_emb]; runs the Regulation + head forward with activations saved -- the head at the tail of the Regulation
 * launch where cf_head_rides(h) -- and leaves the handle as cf_backward_part(parts = 1 | 2) expects (same batch; the bits of
 * cf_forward_train on the batch whose trunk outputs x0 holds).  cf_backward_part(parts & 4) after it FAILS by name: the trunk kept no
 * activations.  Launches: [k_x0_copy when x0 != NULL] -> the re-tiling of the Regulation + head weights (with the copy blocks of a pending
 * cf_x0_gather_fwd behind them) -> the Regulation + head launches of cf_forward_train.  x0 == NULL: the Regulation input is what
 * cf_x0_gather / cf_x0_gather_fwd put in place.  Capturable. */
int cf_forward_train_x0(cf_handle* h, const cf_batch* batch, const float* const* x0, float* logits, const void* labels,
                        float loss_scale, float* loss_out, void* stream);
/* What a frozen-trunk step reads per gene, resident in HBM: the trunk outputs and the gene's interaction masks (one array may serve
 * every resolution), frequencies and labels -- the corresponding arrays of cf_store can be passed as they are. */
typedef struct cf_x0_store {
    long long n_genes;
    const float*   x0[CF_MAX_RES];                  /* [n,T,d_emb]  (16-byte aligned)     */
    const uint8_t* interaction_mask[CF_MAX_RES];    /* [n,T,T]                            */
    const float*   interaction_freq;                /* [n,T,T]                            */
    const void*    labels;                          /* int64 [n] (n_out = 2) or float [n] */
} cf_x0_store;
/* cf_gather_batch for a frozen-trunk step (same order / cursor protocol, same error flags in cursor[2]): copies genes
 * order[cursor[0] * B ... + B) of the cache into the library's Regulation input buffers, dst's interaction masks and frequencies and
 * labels_dst (may be null), then advances the cursor (a second, one-thread launch).  Bytes only, no atomics; capturable. */
int cf_x0_gather(cf_handle* h, const cf_x0_store* cache, const int* order, int* cursor, const cf_batch* dst, void* labels_dst,
                 void* stream);
/* The same without a launch of its own: the cf_forward_train_x0(x0 = NULL) that must follow on the same stream copies the genes in the
 * launch that re-tiles the Regulation + head weights.  The cursor -- which that launch reads -- is advanced by the
 * cf_reduce_opt_x0(cursor) that ends the step. */
int cf_x0_gather_fwd(cf_handle* h, const cf_x0_store* cache, const int* order, int* cursor, const cf_batch* dst, void* labels_dst,
                     void* stream);
/* The last launch of a frozen-trunk step: cf_reduce_opt_part(CF_BUCKET_REG) -- the same tiles, the same arithmetic, the same bits;
 * nothing of the Embedding + Pairwise range (parameters, moments, gradients, tiled copies) is read or written, no weight decay on it
 * either -- with ONE more workgroup that advances `cursor` (null: nothing to advance) and writes a pending cf_record_step_bwd's log
 * rows.  Also serves the all-rows Embedding (embed n_layers > 1): that path's gradients are the trunk's.  Not capturable. */
int cf_reduce_opt_x0(cf_handle* h, int B, float lr, float beta1, float beta2, float eps, float weight_decay, long long step,
                     int keep_grads, int* cursor, void* stream);
/* cf_backward_from for a frozen trunk: head + Regulation backward and the reductions of CF_BUCKET_REG only. */
int cf_backward_from_top(cf_handle* h, const cf_batch* batch, const float* dlogits, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CHROMOFORMER_HIP_H */
