// cf_api_attrib.h -- host side of the attribution entry points (input gradients, attention maps, pCRE deletion, pCRE coalitions, integrated
// gradients, perturbation scan and its fine-resolution form) and what the row-expanding ones share with the histone-mark games of
// cf_api_marks.h: the chunk workspace and loop, the region geometry, the exact games' words and reducers.  Part of cf_api.hip's single
// translation unit: included there behind cf_api_bwd.h, not on its own.
#pragma once

// k_input_grad's dynamic LDS size; the first call sets the kernel's attribute.  0: that failed (`who`: the entry point, for the error text).
static size_t input_grad_prepare(cf_handle* h, const char* who) {
    const cf_config& c = h->cfg;
    size_t smem = 0;
    for (int r = 0; r < c.n_res; ++r) smem = std::max(smem, input_grad_smem(c.n_bins[r], c.n_feats, c.d_emb));
    if (!h->ig_smem_ok) {
        if (hipFuncSetAttribute((const void*)k_input_grad, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem) != hipSuccess) {
            fail("%s: promoter_feats / pcre_feats: k_input_grad needs %zu bytes of LDS", who, smem);
            return 0;
        }
        h->ig_smem_ok = true;
    }
    return smem;
}
// The feature gradients of the B genes of `bt` from the attention operands its backward pass saved (cf_input_grad.h); a null output is skipped.
static int launch_input_grad(cf_handle* h, const cf_batch& bt, int B, float* const out_p[], float* const out_c[], size_t smem, hipStream_t st) {
    const cf_config& c = h->cfg;
    const int S = c.i_max, nres = c.n_res, F = c.n_feats, kD = c.d_emb;
    InGradArgs a;
    memset(&a, 0, sizeof a);
    for (int r = 0; r < nres; ++r) {
        a.feats_p[r] = bt.promoter_feats[r];
        a.feats_c[r] = bt.pcre_feats[r];
        a.mask_p[r] = static_cast<const uint8_t*>(bt.promoter_mask_row[r]);
        a.mask_c[r] = static_cast<const uint8_t*>(bt.pcre_mask_row[r]);
        a.mstride_p[r] = bt.promoter_mask_stride[r];
        a.mstride_c[r] = bt.pcre_mask_stride[r];
        a.pet[r] = h->pet[r];
        a.w_p[r] = h->refs.lin_proj[r];
        a.w_c[r] = h->refs.P[r][0].wlp;
        a.edx0[r] = h->edx0[r];
        a.ep[r] = h->E[r].p;
        a.eqt[r] = h->E[r].qt;
        a.edxbar[r] = h->E[r].dxbar;
        for (int l = 0; l < c.pair_layers; ++l) {
            a.pp[r][l] = h->P[r][l].p;
            a.pqt[r][l] = h->P[r][l].qt;
            a.pdxbar[r][l] = h->P[r][l].dxbar;
        }
        a.out_p[r] = out_p[r];
        a.out_c[r] = out_c[r];
        a.L[r] = c.n_bins[r];
    }
    a.B = B;
    a.S = S;
    a.F = F;
    a.D = kD;
    a.nh_e = c.embed_heads;
    a.nh_p = c.pair_heads;
    a.n_pl = c.pair_layers;
    a.rs_e = 1.0f / sqrtf((float)(kD / c.embed_heads));
    a.rs_p = 1.0f / sqrtf((float)(kD / c.pair_heads));
    hipLaunchKernelGGL(k_input_grad, dim3(1 + S, B, nres), dim3(kIgThreads), smem, st, a);
    LAUNCH_CHECK("k_input_grad");
    return 0;
}
// The trunk's output (the Regulation input Rx[r][0]) of B genes, copied to dst[r]
static int stash_trunk_output(cf_handle* h, int B, float* const dst[], hipStream_t st) {
    const cf_config& c = h->cfg;
    const int nres = c.n_res, row4 = (c.i_max + 1) * c.d_emb / 4;
    AblateStashArgs sa;
    memset(&sa, 0, sizeof sa);
    for (int r = 0; r < nres; ++r) {
        sa.src[r] = reinterpret_cast<const float4*>(h->Rx[r][0]);
        sa.dst[r] = reinterpret_cast<float4*>(dst[r]);
    }
    sa.n4 = (long long)B * row4;
    hipLaunchKernelGGL(k_pcre_stash, dim3((int)std::min<long long>((sa.n4 + kAblThreads - 1) / kAblThreads, 256), nres), dim3(kAblThreads), 0, st, sa);
    LAUNCH_CHECK("k_pcre_stash");
    return 0;
}

// cf_backward_from + the gradients of the float inputs (cf_input_grad.h).  The parameter gradients come from the very launches of
// cf_backward_from; the interaction_freq gradient from the Regulation backward's DFREQ variant, the feature gradients from the saved
// attention operands, in front of the reductions.  Every requested output is overwritten in full.
extern "C" int cf_backward_from_inputs(cf_handle* h, const cf_batch* bt, const float* dlogits, const cf_input_grads* want, void* stream) {
    bool any_p = false, any_c = false;
    if (want)
        for (int r = 0; r < kMaxRes; ++r) {
            any_p |= want->promoter_feats[r] != nullptr;
            any_c |= want->pcre_feats[r] != nullptr;
        }
    const bool any_f = want && want->interaction_freq;
    if (!any_p && !any_c && !any_f) return cf_backward_from(h, bt, dlogits, stream);
    if (check_bwd(h, bt)) return -1;
    if (!dlogits) return fail("cf_backward_from_inputs: dlogits is null");
    const cf_config& c = h->cfg;
    const int B = bt->B, T = c.i_max + 1, nres = c.n_res;
    for (int r = nres; r < kMaxRes; ++r)
        if (want->promoter_feats[r] || want->pcre_feats[r]) return fail("cf_backward_from_inputs: promoter_feats / pcre_feats[%d]: the model has %d resolutions", r, nres);
    if (any_p && h->embed_dense)
        return fail("cf_backward_from_inputs: promoter_feats: input gradients are implemented for embed.n_layers = 1 (the centre-row Embedding); "
                    "this model has embed.n_layers = %d (the all-rows path keeps no first-layer input-row gradient)", c.embed_layers);
    if (any_f && h->reg_fused && !h->reg_dfreq_ok)
        return fail("cf_backward_from_inputs: interaction_freq: the fused Regulation backward variant could not be configured");
    const size_t smem = any_p || any_c ? input_grad_prepare(h, "cf_backward_from_inputs") : 0;
    if ((any_p || any_c) && !smem) return -1;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(h->dlogits, dlogits, (size_t)B * c.n_out * sizeof(float), hipMemcpyDeviceToDevice, st));
    PassOpts po;
    po.dfreq = any_f ? h->dfreq_part : nullptr;
    if (backward_impl(h, bt, st, 7, nullptr, 1.f, nullptr, po)) return -1;
    if (any_p || any_c) {
        if (launch_input_grad(h, *bt, B, want->promoter_feats, want->pcre_feats, smem, st)) return -1;
    }
    if (any_f) {
        const int n = B * T * T;
        hipLaunchKernelGGL(k_dfreq_sum, dim3((n + 255) / 256), dim3(256), 0, st, h->dfreq_part, want->interaction_freq, n, nres);
        LAUNCH_CHECK("k_dfreq_sum");
    }
    return reduce_impl(h, B, st);
}

// The epilogue of the forward-only entry points: the activations a saving forward kept are gone (a later cf_backward* is refused),
// the launches since `launches0` are the forward's count (mirrored into a capture).
static void forward_counted(cf_handle* h, long long launches0) {
    h->last_fwd_B = 0;
    h->n_fwd = (int)(g_launches - launches0);
    if (h->capturing) h->cap.n_fwd = h->n_fwd;
}
// One more launch (a copy-out or a reducer) on the account of the forward
static void forward_one_more(cf_handle* h) {
    ++h->n_fwd;
    if (h->capturing) h->cap.n_fwd = h->n_fwd;
}

// cf_forward(save = 1) + k_attn_maps (cf_attn_maps.h): the attention probabilities the forward kept for the backward pass and the
// fc_head input, copied into the caller's dense layouts.  Nothing requested: exactly the launches of cf_forward(save = 1).
extern "C" int cf_attention_maps(cf_handle* h, const cf_batch* bt, float* logits, const cf_attn_maps* want, void* stream) {
    if (!h) return fail("null handle");
    const cf_config& c = h->cfg;
    const int nres = c.n_res;
    bool any_e = false, any = false;
    if (want) {
        for (int r = 0; r < kMaxRes; ++r) {
            if (r >= nres && (want->embed[r] || want->pairwise[r] || want->regulation[r]))
                return fail("cf_attention_maps: embed / pairwise / regulation[%d]: the model has %d resolutions", r, nres);
            any_e |= want->embed[r] != nullptr;
            any |= want->embed[r] || want->pairwise[r] || want->regulation[r];
        }
        any |= want->embedding != nullptr;
    }
    if (any_e && h->embed_dense)
        return fail("cf_attention_maps: embed: attention maps are implemented for embed.n_layers = 1 (the centre-row Embedding); "
                    "this model has embed.n_layers = %d (the all-rows path keeps no probabilities)", c.embed_layers);
    if (c.pair_layers > kMapPair || c.reg_layers > kMapReg)
        return fail("cf_attention_maps: pairwise / regulation: at most %d / %d layers", kMapPair, kMapReg);
    if (forward_impl(h, bt, logits, 1, stream, nullptr)) return -1;
    if (!any) return 0;
    const int B = bt->B;
    AttnMapArgs a;
    memset(&a, 0, sizeof a);
    long long most = want->embedding ? (long long)B * nres * c.d_emb : 0;      // elements of the largest requested output
    for (int r = 0; r < nres; ++r) {
        const int L = c.n_bins[r];
        a.ep[r] = h->E[r].p;
        for (int l = 0; l < c.pair_layers; ++l) a.pp[r][l] = h->P[r][l].p;
        for (int l = 0; l < c.reg_layers; ++l) a.rp[r][l] = h->reg_fused ? h->R[r][l].hq : h->R[r][l].p;
        a.embed[r] = want->embed[r];
        a.pair[r] = want->pairwise[r];
        a.reg[r] = want->regulation[r];
        a.L[r] = L;
        if (a.embed[r]) most = std::max(most, (long long)B * c.embed_heads * L);
        if (a.pair[r]) most = std::max(most, (long long)B * c.pair_layers * c.i_max * c.pair_heads * L);
        if (a.reg[r]) most = std::max(most, (long long)B * c.reg_layers * c.reg_heads * (c.i_max + 1));
    }
    a.hin = h->hin;
    a.emb = want->embedding;
    a.B = B;
    a.S = c.i_max;
    a.T = c.i_max + 1;
    a.nh_e = c.embed_heads;
    a.nh_p = c.pair_heads;
    a.n_pl = c.pair_layers;
    a.H = c.reg_heads;
    a.n_rl = c.reg_layers;
    a.K = nres * c.d_emb;
    a.reg_fused = h->reg_fused ? 1 : 0;
    const int gx = (int)std::min<long long>((most + kMapThreads - 1) / kMapThreads, 1024);
    hipLaunchKernelGGL(k_attn_maps, dim3(gx, kMapSegs), dim3(kMapThreads), 0, (hipStream_t)stream, a);
    LAUNCH_CHECK("k_attn_maps");
    forward_one_more(h);
    return 0;
}

// What the chunked attribution entry points check alike, first: the handle, the batch, its size, riders where the call runs a backward
// pass or leaves the launch sequence of a step (`no_riders`), the batch's pointers.
static int attrib_open(cf_handle* h, const cf_batch* bt, bool no_riders, const char* who) {
    if (!h) return fail("%s: null handle", who);
    if (!bt) return fail("%s: null batch", who);
    if (bt->B > h->cfg.max_batch) return fail("%s: batch size %d exceeds max_batch=%d", who, bt->B, h->cfg.max_batch);
    if (no_riders && (h->rider.armed || h->rider.done)) return fail("%s: riders are armed for a training step (cf_rider_arm); finish the step first", who);
    return check_batch(h, bt);
}

// The chunk workspace (cf_handle::AttribWs), allocated by the first attribution call that needs chunk buffers (the model's other entry
// points never do): the chunk's rows and per-row gradients, the three mask sets, one stash, the chunk logits, the per-slice sums and the
// i_max + 2 coalition words of cf_pcre_ablation (cf_coalition.h), written here, once -- a call copies nothing from the host.
static int attrib_ws(cf_handle* h, const char* who) {
    cf_handle::AttribWs& w = h->aw;
    if (w.mem) return 0;
    const cf_config& c = h->cfg;
    const size_t M = c.max_batch, S = c.i_max, T = S + 1, F = c.n_feats;
    size_t nf = 0, nb = 0;      // floats, then bytes (every float segment a multiple of 4 floats: 16-byte aligned rows)
    auto up4 = [](size_t n) { return (n + 3) & ~(size_t)3; };
    for (int r = 0; r < c.n_res; ++r) nf += 2 * up4(M * c.n_bins[r] * F) + 2 * up4(M * S * c.n_bins[r] * F) + up4(M * T * c.d_emb);
    nf += 2 * up4(M * T * T) + up4(M * c.n_out) + up4(M * kIgSlices) + up4(T + 1);
    // (the all-rows Embedding reads every row of a full [B, L, L] promoter mask: its chunks keep L rows per chunk row)
    auto pm_rows = [&](int r) { return h->embed_dense ? (size_t)c.n_bins[r] : (size_t)1; };
    for (int r = 0; r < c.n_res; ++r) nb += M * pm_rows(r) * c.n_bins[r] + M * S * c.n_bins[r] + M * T * T;
    DevBuf<float> mem;
    if (mem.alloc(nf + (nb + 3) / 4, who)) return -1;
    float* f = mem;
    auto take = [&](size_t n) { float* p = f; f += up4(n); return p; };
    for (int r = 0; r < c.n_res; ++r) {
        const size_t L = c.n_bins[r];
        w.row[r] = take(M * L * F);
        w.grad[r] = take(M * L * F);
        w.row[kMaxRes + r] = take(M * S * L * F);
        w.grad[kMaxRes + r] = take(M * S * L * F);
        w.stash[r] = take(M * T * c.d_emb);
    }
    w.row[2 * kMaxRes] = take(M * T * T);
    w.grad[2 * kMaxRes] = take(M * T * T);
    w.logits = take(M * c.n_out);
    w.slice_sums = take(M * kIgSlices);
    float* words_at = take(T + 1);
    uint8_t* u = (uint8_t*)f;
    for (int r = 0; r < c.n_res; ++r) {
        const size_t L = c.n_bins[r];
        w.pmask[r] = u, u += M * pm_rows(r) * L;
        w.cmask[r] = u, u += M * S * L;
        w.imask[r] = u, u += M * T * T;
    }
    const unsigned N = (1u << c.i_max) - 1u;
    std::vector<unsigned> words(T + 1, N);      // everything kept | slot j deleted | nothing kept
    for (int j = 0; j < c.i_max; ++j) words[1 + j] = N & ~(1u << j);
    words[T] = 0;
    if (hipMemcpy(words_at, words.data(), (T + 1) * sizeof(unsigned), hipMemcpyHostToDevice) != hipSuccess)
        return fail("%s: writing the deletion table failed", who);      // (`mem` frees itself; the workspace stays unallocated)
    w.deletion_words = (const unsigned*)words_at;
    w.mem = std::move(mem);
    return 0;
}

// One launch of an expand kernel (kIgxThreads / kAblThreads / kRowThreads threads, no LDS) with its argument struct, counted.
template <class Args>
static int launch_expand(void (*kernel)(Args), const char* name, dim3 grid, int threads, const Args& a, hipStream_t st) {
    hipLaunchKernelGGL(kernel, grid, dim3(threads), 0, st, a);
    LAUNCH_CHECK(name);
    return 0;
}

// The chunk loop of the row-expanding entry points.  Per chunk of at most max_batch of the `rows` rows: expand(g0, n) launches the
// kernel that writes rows g0 .. g0 + n - 1 into the chunk workspace, then an inference forward on the chunk's batch `cb` writes the
// chunk's contiguous slice of `logits` -- the launches of cf_forward(save = 0) when `trunk` (k_attc2 takes as many regions per
// workgroup as for the caller's `genes` genes, ag_genes), else Regulation + head alone, on rows the kernel has put in place.
template <class Expand>
static int chunk_forward(cf_handle* h, cf_batch* cb, long long rows, float* logits, bool trunk, int genes, hipStream_t st, Expand expand) {
    const int cap = h->cfg.max_batch, n_out = h->cfg.n_out;
    for (long long g0 = 0; g0 < rows; g0 += cap) {
        const int n = (int)std::min<long long>(cap, rows - g0);
        if (expand(g0, n)) return -1;
        cb->B = n;
        if ((trunk && forward_trunk(h, cb, 0, st, genes)) || forward_reg_head(h, cb, logits + (size_t)g0 * n_out, 0, st, nullptr)) return -1;
    }
    return 0;
}

// The shared host routine of cf_pcre_ablation and the coalition entry points (cf_coalition.h): the trunk once on the B genes,
// k_pcre_stash, then per chunk of at most max_batch of the B * n_coal rows (gene-major; row (b, k) is word tab[k], a device table) one
// k_coalition_expand and the Regulation + head launches of an inference forward on that chunk, writing the chunk's contiguous slice of
// `logits`.  The callers have checked the batch and called attrib_ws.  coalition_rows_by is the routine with the expand launch as a
// parameter -- launch(ea, n) issues the one expand launch of a chunk of n rows on the filled CoalExpandArgs --: coalition_rows passes
// k_coalition_expand, the contact games (cf_api_contact.h) k_contact_expand.
template <class Launch>
static int coalition_rows_by(cf_handle* h, const cf_batch* bt, const unsigned* tab, int n_coal, float* logits, hipStream_t st, Launch launch) {
    const cf_config& c = h->cfg;
    const int B = bt->B, T = c.i_max + 1, nres = c.n_res;
    const long long launches0 = g_launches;
    if (forward_trunk(h, bt, 0, st) || stash_trunk_output(h, B, h->aw.stash, st)) return -1;
    CoalExpandArgs ea;
    memset(&ea, 0, sizeof ea);
    cf_batch cb = *bt;      // the chunk's batch: only B, the masks and the frequencies are read past the trunk
    for (int r = 0; r < nres; ++r) {
        ea.stash[r] = reinterpret_cast<const float4*>(h->aw.stash[r]);
        ea.x0[r] = reinterpret_cast<float4*>(h->Rx[r][0]);
        ea.mask_in[r] = bt->interaction_mask[r];
        ea.mask_out[r] = h->aw.imask[r];
        cb.interaction_mask[r] = h->aw.imask[r];
    }
    ea.freq_in = bt->interaction_freq;
    ea.freq_out = h->aw.row[2 * kMaxRes];
    cb.interaction_freq = h->aw.row[2 * kMaxRes];
    ea.keep = tab;
    ea.n_coal = n_coal, ea.T = T, ea.row4 = T * c.d_emb / 4;
    if (chunk_forward(h, &cb, (long long)B * n_coal, logits, false, B, st, [&](long long g0, int n) {
            ea.g0 = g0;
            return launch(ea, n);
        }))
        return -1;
    forward_counted(h, launches0);
    return 0;
}
static int coalition_rows(cf_handle* h, const cf_batch* bt, const unsigned* tab, int n_coal, float* logits, hipStream_t st) {
    const int nres = h->cfg.n_res;
    return coalition_rows_by(h, bt, tab, n_coal, logits, st, [&](const CoalExpandArgs& ea, int n) {
        return launch_expand(k_coalition_expand, "k_coalition_expand", dim3(n, nres), kAblThreads, ea, st);
    });
}

// The fixed table of attrib_ws through coalition_rows: variant v of gene b is row (b, v).
extern "C" int cf_pcre_ablation(cf_handle* h, const cf_batch* bt, float* logits, void* stream) {
    const char* who = "cf_pcre_ablation";
    if (attrib_open(h, bt, false, who)) return -1;
    if (!logits) return fail("%s: null logits", who);
    if (attrib_ws(h, who)) return -1;
    return coalition_rows(h, bt, h->aw.deletion_words, h->cfg.i_max + 2, logits, (hipStream_t)stream);
}

// A host `keep` array validated and uploaded into the handle's word table (in front of coalition_rows).
static int coalition_upload(cf_handle* h, const uint32_t* keep, int n_coal, hipStream_t st, const char* who) {
    const cf_config& c = h->cfg;
    if (n_coal < 1) return fail("%s: n_coal = %d: at least 1 coalition", who, n_coal);
    if (!keep) return fail("%s: null keep", who);
    for (int k = 0; k < n_coal; ++k)
        if (keep[k] >> c.i_max) return fail("%s: keep[%d] = 0x%x names a pCRE slot >= i_max = %d", who, k, keep[k], c.i_max);
    if (attrib_ws(h, who) || h->aw.words.need(n_coal, 256, who)) return -1;
    HIP_TRY(hipMemcpyAsync(h->aw.words, keep, (size_t)n_coal * sizeof(unsigned), hipMemcpyHostToDevice, st));
    return 0;
}

extern "C" int cf_pcre_coalitions(cf_handle* h, const cf_batch* bt, const uint32_t* keep, int n_coal, float* logits, void* stream) {
    const char* who = "cf_pcre_coalitions";
    if (attrib_open(h, bt, false, who)) return -1;
    if (!logits) return fail("%s: null logits", who);
    hipStream_t st = (hipStream_t)stream;
    if (coalition_upload(h, keep, n_coal, st, who)) return -1;
    return coalition_rows(h, bt, h->aw.words, n_coal, logits, st);
}

// The rows of a Shapley / epistasis call: the caller's buffer, else the handle's own [max_batch, per, n_out] (null: out of memory)
static float* coalition_out_rows(cf_handle* h, float* callers, long long per, const char* who) {
    if (callers) return callers;
    return h->aw.own_rows.need((size_t)h->cfg.max_batch * per * h->cfg.n_out, 0, who) ? nullptr : (float*)h->aw.own_rows;
}

// The two exact games on P players (the pCRE slots, or the players of a mark game), their coalition words and their reducers.
// all_words: every coalition, word m at column m; launch_shapley: k_shapley on the [B, 2^P, n_out] rows.
static std::vector<uint32_t> all_words(int P) {
    std::vector<uint32_t> keep((size_t)1 << P);
    for (size_t m = 0; m < keep.size(); ++m) keep[m] = (uint32_t)m;
    return keep;
}
static void shapley_weights(int P, float* w) {      // w(k) = k! (P - k - 1)! / P!, in double, rounded to fp32
    double fact[kCoalMaxS + 1] = {1.0};
    for (int k = 1; k <= P; ++k) fact[k] = fact[k - 1] * k;
    for (int k = 0; k < P; ++k) w[k] = (float)(fact[k] * fact[P - k - 1] / fact[P]);
}
static int launch_shapley(cf_handle* h, int B, int P, const float* rows, float* phi, hipStream_t st) {
    ShapleyArgs sa;
    memset(&sa, 0, sizeof sa);
    sa.v = rows, sa.phi = phi, sa.S = P, sa.n_out = h->cfg.n_out;
    shapley_weights(P, sa.w);
    hipLaunchKernelGGL(k_shapley, dim3(B, P), dim3(kShapThreads), 0, st, sa);
    LAUNCH_CHECK("k_shapley");
    forward_one_more(h);
    return 0;
}
// The pairwise interaction index of the P >= 2 players on the same rows: what the interactions entry points check beside their
// sibling's checks, and k_shapley_pairs with the weight table of `index` (cf_coalition.h), in double, rounded to fp32:
//   sii  w2(s) = s! (P - s - 2)! / (P - 1)!        sti  w2(s) = (2 / P) / C(P - 1, s),   s = |S| <= P - 2.
static int interactions_check(int index, int P, const float* inter, const char* who) {
    if (!inter) return fail("%s: null inter", who);
    if (index != CF_INTERACTION_SII && index != CF_INTERACTION_STI)
        return fail("%s: index = %d: CF_INTERACTION_SII (%d) or CF_INTERACTION_STI (%d)", who, index, CF_INTERACTION_SII, CF_INTERACTION_STI);
    if (P < 2) return fail("%s: %d player%s: a pair needs at least 2", who, P, P == 1 ? "" : "s");
    return 0;
}
static int launch_shapley_pairs(cf_handle* h, int B, int P, int index, const float* rows, float* inter, hipStream_t st) {
    ShapleyPairsArgs pa;
    memset(&pa, 0, sizeof pa);
    pa.v = rows, pa.inter = inter, pa.P = P, pa.n_out = h->cfg.n_out, pa.sti = index == CF_INTERACTION_STI;
    shapley_weights(P, pa.w1);
    double fact[kCoalMaxS + 1] = {1.0};
    for (int k = 1; k <= P; ++k) fact[k] = fact[k - 1] * k;
    for (int s = 0; s <= P - 2; ++s)
        pa.w2[s] = pa.sti ? (float)((2.0 / P) / (fact[P - 1] / (fact[s] * fact[P - 1 - s]))) : (float)(fact[s] * fact[P - s - 2] / fact[P - 1]);
    hipLaunchKernelGGL(k_shapley_pairs, dim3(B, P * (P + 1) / 2), dim3(kShapThreads), 0, st, pa);
    LAUNCH_CHECK("k_shapley_pairs");
    forward_one_more(h);
    return 0;
}
// The reducers of an interactions call on its 2^P rows: k_shapley_pairs, and k_shapley too if the caller wants phi.
static int launch_interactions(cf_handle* h, int B, int P, int index, const float* rows, float* inter, float* phi, hipStream_t st) {
    if (launch_shapley_pairs(h, B, P, index, rows, inter, st)) return -1;
    return phi ? launch_shapley(h, B, P, rows, phi, st) : 0;
}
// The operator on a caller's table: no batch, no workspace, nothing of the handle but n_out is read and no activation is written.
extern "C" int cf_shapley_interactions_from_rows(cf_handle* h, const float* rows, int B, int P, int index, float* inter, void* stream) {
    const char* who = "cf_shapley_interactions_from_rows";
    if (!h) return fail("%s: null handle", who);
    if (!rows) return fail("%s: null rows", who);
    if (B < 1) return fail("%s: B = %d: at least 1 gene", who, B);
    if (P < 2 || P > kCoalMaxS) return fail("%s: P = %d outside 2..%d", who, P, kCoalMaxS);
    if (interactions_check(index, P, inter, who)) return -1;
    h->n_fwd = 0;
    return launch_shapley_pairs(h, B, P, index, rows, inter, (hipStream_t)stream);
}
// The Harsanyi dividends of a caller's table (cf_dividends.h): k_moebius, and above one LDS tile k_moebius_high in place on its output.
// An operator as the one above: no batch, no workspace, no activation is touched.
extern "C" int cf_dividends_from_rows(cf_handle* h, const float* rows, int B, int P, float* div, float* mass, void* stream) {
    const char* who = "cf_dividends_from_rows";
    if (!h) return fail("%s: null handle", who);
    if (!rows) return fail("%s: null rows", who);
    if (!div) return fail("%s: null div", who);
    if (B < 1) return fail("%s: B = %d: at least 1 gene", who, B);
    if (P < 1 || P > kCoalMaxS) return fail("%s: P = %d outside 1..%d", who, P, kCoalMaxS);
    static_assert(kCoalMaxS - kDivTileBits == 4, "k_moebius_high is instantiated for 1..4 stages");
    hipStream_t st = (hipStream_t)stream;
    MoebiusArgs ma;
    ma.v = rows, ma.div = div, ma.mass = mass, ma.P = P, ma.n_out = h->cfg.n_out;      // n_out <= kDivMaxOut: cf_create
    const int tables = mass ? 2 : 1, high = P - kDivTileBits;
    h->n_fwd = 0;
    hipLaunchKernelGGL(k_moebius, dim3(B, high > 0 ? 1 << high : 1, tables), dim3(kDivThreads), 0, st, ma);
    LAUNCH_CHECK("k_moebius");
    forward_one_more(h);
    if (high <= 0) return 0;
    const dim3 grid(B, kDivTile * ma.n_out / kDivThreads, tables), block(kDivThreads);
    switch (high) {
        case 1: hipLaunchKernelGGL(k_moebius_high<1>, grid, block, 0, st, ma); break;
        case 2: hipLaunchKernelGGL(k_moebius_high<2>, grid, block, 0, st, ma); break;
        case 3: hipLaunchKernelGGL(k_moebius_high<3>, grid, block, 0, st, ma); break;
        default: hipLaunchKernelGGL(k_moebius_high<4>, grid, block, 0, st, ma); break;
    }
    LAUNCH_CHECK("k_moebius_high");
    forward_one_more(h);
    return 0;
}
// An interaction index of listed sets from the dividends (k_set_index).  The weight table of `index` with top order `order`, in
// double, rounded to fp32:  sii wt[|S|][|U|] = 1 / (|U| - |S| + 1);  sti |S| = order: 1 / C(|U|, order), below: the dividend's bits.
// The set words travel in the handle's word table.
extern "C" int cf_set_interactions_from_dividends(cf_handle* h, const float* div, int B, int P, const uint32_t* sets, int n_sets, int index,
                                                  int order, float* out, void* stream) {
    const char* who = "cf_set_interactions_from_dividends";
    if (!h) return fail("%s: null handle", who);
    if (!div) return fail("%s: null div", who);
    if (!sets) return fail("%s: null sets", who);
    if (!out) return fail("%s: null out", who);
    if (B < 1) return fail("%s: B = %d: at least 1 gene", who, B);
    if (P < 1 || P > kCoalMaxS) return fail("%s: P = %d outside 1..%d", who, P, kCoalMaxS);
    if (n_sets < 1 || n_sets > 65535) return fail("%s: n_sets = %d outside 1..65535", who, n_sets);
    if (order < 1 || order > P) return fail("%s: order = %d outside 1..P = %d", who, order, P);
    if (index != CF_INTERACTION_SII && index != CF_INTERACTION_STI)
        return fail("%s: index = %d: CF_INTERACTION_SII (%d) or CF_INTERACTION_STI (%d)", who, index, CF_INTERACTION_SII, CF_INTERACTION_STI);
    for (int s = 0; s < n_sets; ++s) {
        if (!sets[s]) return fail("%s: sets[%d] is the empty set", who, s);
        if (sets[s] >> P) return fail("%s: sets[%d] = 0x%x names a player >= P = %d", who, s, sets[s], P);
        if (__builtin_popcount(sets[s]) > order) return fail("%s: sets[%d] = 0x%x holds %d players, more than order = %d", who, s, sets[s], __builtin_popcount(sets[s]), order);
    }
    if (h->aw.words.need(n_sets, 256, who)) return -1;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(h->aw.words, sets, (size_t)n_sets * sizeof(unsigned), hipMemcpyHostToDevice, st));
    SetIndexArgs sa;
    memset(&sa, 0, sizeof sa);
    sa.div = div, sa.sets = h->aw.words, sa.out = out, sa.P = P, sa.n_out = h->cfg.n_out, sa.n_sets = n_sets;
    const bool sti = index == CF_INTERACTION_STI;
    sa.copy_below = sti ? order : 0;
    double fact[kCoalMaxS + 1] = {1.0};
    for (int k = 1; k <= P; ++k) fact[k] = fact[k - 1] * k;
    for (int s = sti ? order : 1; s <= order; ++s)
        for (int u = s; u <= P; ++u) sa.wt[s - 1][u - 1] = sti ? (float)(1.0 / (fact[u] / (fact[s] * fact[u - s]))) : (float)(1.0 / (u - s + 1));
    h->n_fwd = 0;
    hipLaunchKernelGGL(k_set_index, dim3(B, n_sets), dim3(kShapThreads), 0, st, sa);
    LAUNCH_CHECK("k_set_index");
    forward_one_more(h);
    return 0;
}
// pair_words: the 1 + P + P (P - 1) / 2 pair-deletion coalitions (N = 2^P - 1; N without i; N without i and j, i < j);
// launch_epistasis: k_epistasis on those rows.
static std::vector<uint32_t> pair_words(int P) {
    const uint32_t N = (1u << P) - 1u;
    std::vector<uint32_t> keep;
    keep.push_back(N);
    for (int i = 0; i < P; ++i) keep.push_back(N & ~(1u << i));
    for (int i = 0; i < P; ++i)
        for (int j = i + 1; j < P; ++j) keep.push_back(N & ~(1u << i) & ~(1u << j));
    return keep;
}
static int launch_epistasis(cf_handle* h, int B, int P, const float* rows, float* eps, hipStream_t st) {
    EpistasisArgs ea;
    ea.v = rows, ea.eps = eps, ea.B = B, ea.S = P, ea.n_out = h->cfg.n_out;
    const long long n = (long long)B * P * P * h->cfg.n_out;
    hipLaunchKernelGGL(k_epistasis, dim3((int)std::min<long long>((n + kShapThreads - 1) / kShapThreads, 1024)), dim3(kShapThreads), 0, st, ea);
    LAUNCH_CHECK("k_epistasis");
    forward_one_more(h);
    return 0;
}

// All 2^i_max coalitions through coalition_upload + coalition_rows, then k_shapley.
extern "C" int cf_pcre_shapley(cf_handle* h, const cf_batch* bt, float* phi, float* logits_all, void* stream) {
    const char* who = "cf_pcre_shapley";
    if (attrib_open(h, bt, false, who)) return -1;
    if (!phi) return fail("%s: null phi", who);
    const int S = h->cfg.i_max, n = 1 << S;
    float* rows = coalition_out_rows(h, logits_all, n, who);
    if (!rows) return -1;
    const std::vector<uint32_t> keep = all_words(S);
    hipStream_t st = (hipStream_t)stream;
    if (coalition_upload(h, keep.data(), n, st, who) || coalition_rows(h, bt, h->aw.words, n, rows, st)) return -1;
    return launch_shapley(h, bt->B, S, rows, phi, st);
}

// cf_pcre_shapley's rows, then k_shapley_pairs (and k_shapley if phi is wanted).
extern "C" int cf_pcre_shapley_interactions(cf_handle* h, const cf_batch* bt, int index, float* inter, float* phi, float* logits_all, void* stream) {
    const char* who = "cf_pcre_shapley_interactions";
    if (attrib_open(h, bt, false, who)) return -1;
    const int S = h->cfg.i_max, n = 1 << S;
    if (interactions_check(index, S, inter, who)) return -1;
    float* rows = coalition_out_rows(h, logits_all, n, who);
    if (!rows) return -1;
    const std::vector<uint32_t> keep = all_words(S);
    hipStream_t st = (hipStream_t)stream;
    if (coalition_upload(h, keep.data(), n, st, who) || coalition_rows(h, bt, h->aw.words, n, rows, st)) return -1;
    return launch_interactions(h, bt->B, S, index, rows, inter, phi, st);
}

// The pair-deletion coalitions through coalition_upload + coalition_rows, then k_epistasis.
extern "C" int cf_pcre_epistasis(cf_handle* h, const cf_batch* bt, float* eps, float* logits_pairs, void* stream) {
    const char* who = "cf_pcre_epistasis";
    if (attrib_open(h, bt, false, who)) return -1;
    if (!eps) return fail("%s: null eps", who);
    const std::vector<uint32_t> keep = pair_words(h->cfg.i_max);
    const int R = (int)keep.size();
    float* rows = coalition_out_rows(h, logits_pairs, R, who);
    if (!rows) return -1;
    hipStream_t st = (hipStream_t)stream;
    if (coalition_upload(h, keep.data(), R, st, who) || coalition_rows(h, bt, h->aw.words, R, rows, st)) return -1;
    return launch_epistasis(h, bt->B, h->cfg.i_max, rows, eps, st);
}

// A chunk of rows in the workspace (cf_integrated_gradients, the scans): the chunk's batch `cb` (all but B) and the
// description `ra` of the mask rows its expand kernel copies from the caller's batch (cf_rows.h).
static void chunk_rows(cf_handle* h, const cf_batch* bt, RowCopyArgs* ra, cf_batch* cb) {
    const cf_config& c = h->cfg;
    memset(ra, 0, sizeof *ra);
    memset(cb, 0, sizeof *cb);
    for (int r = 0; r < c.n_res; ++r) {
        const int L = c.n_bins[r];
        // The all-rows Embedding (embed.n_layers > 1) honours a full [B, L, L] promoter mask entry by entry: the chunk rows carry
        // all L rows of their gene's mask, not the centre row alone (from which only the dataset's not(valid x valid) form can be rebuilt).
        const bool pm_full = h->embed_dense && bt->promoter_mask_stride[r] == (long long)L * L;
        ra->pm_rows[r] = pm_full ? L : 1;
        ra->pm_in[r] = static_cast<const uint8_t*>(bt->promoter_mask_row[r]) - (pm_full ? (size_t)(L / 2) * L : 0);
        ra->cm_in[r] = bt->pcre_mask_row[r];
        ra->pm_stride[r] = bt->promoter_mask_stride[r];
        ra->cm_stride[r] = bt->pcre_mask_stride[r];
        ra->pm_out[r] = h->aw.pmask[r];
        ra->cm_out[r] = h->aw.cmask[r];
        ra->im_in[r] = bt->interaction_mask[r];
        ra->im_out[r] = h->aw.imask[r];
        ra->L[r] = L;
        cb->promoter_feats[r] = h->aw.row[r];
        cb->pcre_feats[r] = h->aw.row[kMaxRes + r];
        cb->promoter_mask_row[r] = h->aw.pmask[r] + (pm_full ? (size_t)(L / 2) * L : 0);
        cb->promoter_mask_stride[r] = pm_full ? (long long)L * L : L;
        cb->pcre_mask_row[r] = h->aw.cmask[r];
        cb->pcre_mask_stride[r] = L;
        cb->interaction_mask[r] = h->aw.imask[r];
    }
    cb->interaction_freq = h->aw.row[2 * kMaxRes];
    ra->S = c.i_max;
    ra->TT = (c.i_max + 1) * (c.i_max + 1);
}

// Integrated gradients (cf_ig.h).  General path, per chunk of at most max_batch of the B * V rows: k_ig_expand, the launches of
// cf_forward(save = 1), backward_impl (head, Regulation, trunk), k_input_grad / k_dfreq_sum into the per-row scratch, k_ig_accumulate;
// no reduce_impl; k_ig_delta once at the end.  k_attc2 takes as many regions per workgroup as for the caller's B genes (ag_genes),
// so the chunks run the attention variant model(...) on the batch runs: the result does not depend on max_batch and equals the
// hand-written loop of grad-enabled model(...) calls on the batch.  Frequency-only path: the trunk once (save = 1, the launches of cf_forward's first part) and its output stashed, then
// per chunk k_ig_expand (stashed rows, masks, frequencies, dlogits), the Regulation + head forward, backward parts 1 and 2,
// k_dfreq_sum, k_ig_accumulate.
//
// raw: the signal path of the feature segments (cf_integrated_gradients_raw: k_ig_expand_raw, k_ig_accumulate_raw with the node table and
// the optional second output `coeff`); everything else -- chunking, buffers, launches -- is shared.  path = kIgSignalDonor
// (cf_integrated_gradients_raw_donor): the feature baselines are the donor's features, `coeff` receives cmean, and k_ig_expand_raw_donor /
// k_ig_accumulate_raw_donor take the two places; nothing else differs.
static int integrated_gradients_impl(cf_handle* h, const cf_batch* bt, const cf_ig_opts* o, const cf_input_grads* out, const cf_input_grads* coeff,
                                     float* logits_x, float* logits_base, float* delta, void* stream, int path, const char* who) {
    const bool donor = path == kIgSignalDonor, raw = path != kIgLinear;
    const char* const second = donor ? "cmean" : "coeff";
    if (attrib_open(h, bt, true, who)) return -1;
    if (!o) return fail("%s: null opts", who);
    if (!out) return fail("%s: null out", who);
    if (!logits_x || !logits_base || !delta) return fail("%s: null logits_x / logits_base / delta", who);
    const cf_config& c = h->cfg;
    const int nres = c.n_res, S = c.i_max, T = S + 1, F = c.n_feats, kD = c.d_emb, cap = c.max_batch;
    if (o->n_steps < 1) return fail("%s: n_steps = %d: at least 1 quadrature node", who, o->n_steps);
    if (!o->alphas || !o->weights) return fail("%s: null alphas / weights", who);
    if (o->target < 0 || o->target >= c.n_out) return fail("%s: target = %d outside [0, n_out = %d)", who, o->target, c.n_out);
    if (o->interpolate & ~(CF_IG_PROMOTER | CF_IG_PCRE | CF_IG_FREQ) || !o->interpolate)
        return fail("%s: interpolate = %d: a non-empty mask of CF_IG_PROMOTER | CF_IG_PCRE | CF_IG_FREQ", who, o->interpolate);
    const bool ip = o->interpolate & CF_IG_PROMOTER, ic = o->interpolate & CF_IG_PCRE, ifr = o->interpolate & CF_IG_FREQ;
    if (raw) {
        if (!ip && !ic) return fail("%s: interpolate = %d: the signal path needs CF_IG_PROMOTER or CF_IG_PCRE (frequencies alone: cf_integrated_gradients)", who, o->interpolate);
        for (int r = 0; r < kMaxRes; ++r) {
            if (!donor && (o->base_promoter_feats[r] || o->base_pcre_feats[r]))
                return fail("%s: base_promoter_feats / base_pcre_feats[%d]: the signal path starts at the zero signal; a feature baseline is not accepted", who, r);
            if (coeff && ((coeff->promoter_feats[r] && (!ip || r >= nres)) || (coeff->pcre_feats[r] && (!ic || r >= nres))))
                return fail("%s: %s promoter_feats / pcre_feats[%d]: given for an input that is not interpolated", who, second, r);
            if (donor && r < nres && ((ip && !o->base_promoter_feats[r]) || (ic && !o->base_pcre_feats[r])))
                return fail("%s: base_promoter_feats / base_pcre_feats[%d]: the donor's features are required for every interpolated feature input", who, r);
        }
        if (coeff && coeff->interaction_freq) return fail("%s: %s interaction_freq: interaction_freq has no signal path, so no coefficient", who, second);
        if (donor && o->base_broadcast) return fail("%s: base_broadcast = %d: the donor holds the same genes as the batch, one row each", who, o->base_broadcast);
    }
    for (int r = 0; r < kMaxRes; ++r) {
        if (r >= nres && (out->promoter_feats[r] || out->pcre_feats[r] || o->base_promoter_feats[r] || o->base_pcre_feats[r]))
            return fail("%s: promoter_feats / pcre_feats[%d]: the model has %d resolutions", who, r, nres);
        if (r < nres && (out->promoter_feats[r] != nullptr) != ip)
            return fail("%s: promoter_feats[%d]: the output must be given exactly when promoter_feats is interpolated", who, r);
        if (r < nres && (out->pcre_feats[r] != nullptr) != ic)
            return fail("%s: pcre_feats[%d]: the output must be given exactly when pcre_feats is interpolated", who, r);
    }
    if ((out->interaction_freq != nullptr) != ifr)
        return fail("%s: interaction_freq: the output must be given exactly when interaction_freq is interpolated", who);
    if (ip && h->embed_dense)
        return fail("%s: promoter_feats: input gradients are implemented for embed.n_layers = 1 (the centre-row Embedding); "
                    "this model has embed.n_layers = %d (the all-rows path keeps no first-layer input-row gradient)", who, c.embed_layers);
    if (ifr && h->reg_fused && !h->reg_dfreq_ok)
        return fail("%s: interaction_freq: the fused Regulation backward variant could not be configured", who);
    if (!h->grads) return fail("%s: no gradient buffer bound (the backward workspace is set up by cf_bind; the buffer is not written)", who);
    const size_t smem = ip || ic ? input_grad_prepare(h, who) : 0;
    if ((ip || ic) && !smem) return -1;
    const int B = bt->B, n = o->n_steps, V = n + 2, TT = T * T;
    if (attrib_ws(h, who) || h->aw.words.need(2 * (size_t)n, 128, who)) return -1;
    hipStream_t st = (hipStream_t)stream;
    float* const alpha = reinterpret_cast<float*>((unsigned*)h->aw.words);      // the word table as [nodes | weights]
    float* const weight = alpha + n;
    const bool freq_only = o->interpolate == CF_IG_FREQ && h->ig_trunk_once;      // (never on the signal path: a feature bit is set)
    HIP_TRY(hipMemcpyAsync(alpha, o->alphas, n * sizeof(float), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(weight, o->weights, n * sizeof(float), hipMemcpyHostToDevice, st));
    long long n_fwd = 0, n_bwd = 0;
    IgExpandArgs ea;
    IgAccArgs aa;
    memset(&ea, 0, sizeof ea);
    memset(&aa, 0, sizeof aa);
    cf_batch cb;      // the chunk's batch: the rows' copies
    chunk_rows(h, bt, &ea.rows, &cb);
    for (int r = 0; r < nres; ++r) {
        const int L = c.n_bins[r];
        IgSeg* sp = &ea.seg[r];
        IgSeg* sc = &ea.seg[kMaxRes + r];
        *sp = IgSeg{bt->promoter_feats[r], o->base_promoter_feats[r], h->aw.row[r], h->aw.grad[r], out->promoter_feats[r], L * F};
        *sc = IgSeg{bt->pcre_feats[r], o->base_pcre_feats[r], h->aw.row[kMaxRes + r], h->aw.grad[kMaxRes + r], out->pcre_feats[r], S * L * F};
        ea.stash[r] = reinterpret_cast<const float4*>(h->aw.stash[r]);
        ea.x0[r] = reinterpret_cast<float4*>(h->Rx[r][0]);
    }
    ea.seg[2 * kMaxRes] = IgSeg{bt->interaction_freq, o->base_interaction_freq, h->aw.row[2 * kMaxRes], h->aw.grad[2 * kMaxRes], out->interaction_freq, TT};
    ea.alpha = alpha;
    ea.weight = weight;
    ea.dlogits = h->dlogits;
    ea.V = V, ea.n_out = c.n_out, ea.target = o->target, ea.nres = nres, ea.bcast = o->base_broadcast ? 1 : 0;
    ea.freq_only = freq_only ? 1 : 0;
    ea.row4 = T * kD / 4;
    memcpy(aa.seg, ea.seg, sizeof aa.seg);
    aa.logits = h->aw.logits;
    aa.logits_x = logits_x;
    aa.logits_b = logits_base;
    aa.part = h->aw.slice_sums;
    aa.V = V, aa.n_out = c.n_out, aa.bcast = ea.bcast;
    IgAccRawArgs ra;
    memset(&ra, 0, sizeof ra);
    ra.alpha = alpha;
    if (raw && coeff)
        for (int r = 0; r < nres; ++r) ra.coeff[r] = coeff->promoter_feats[r], ra.coeff[kMaxRes + r] = coeff->pcre_feats[r];
    // k_attc2 takes as many regions per workgroup as for the caller's B genes; the all-rows Embedding backward writes parameter gradients: not run
    PassOpts po;
    po.dfreq = ifr ? h->dfreq_part : nullptr;
    po.no_dense_embed_bwd = true;
    po.ag_genes = B;
    float* const no_grad[kMaxRes] = {};
    auto run = [&]() -> int {
        long long l0 = g_launches;
        if (freq_only) {      // the trunk once on the B genes, its output (the Regulation input) stashed
            if (forward_trunk(h, bt, 1, st, B) || stash_trunk_output(h, B, h->aw.stash, st)) return -1;
        }
        n_fwd += g_launches - l0;
        for (int g0 = 0; g0 < B * V; g0 += cap) {
            const int nr = std::min(cap, B * V - g0);
            l0 = g_launches;
            ea.g0 = g0;
            if (donor) {
                hipLaunchKernelGGL(k_ig_expand_raw_donor, dim3(nr, nres), dim3(kIgxThreads), 0, st, ea);
                LAUNCH_CHECK("k_ig_expand_raw_donor");
            } else if (raw) {
                hipLaunchKernelGGL(k_ig_expand_raw, dim3(nr, nres), dim3(kIgxThreads), 0, st, ea);
                LAUNCH_CHECK("k_ig_expand_raw");
            } else {
                hipLaunchKernelGGL(k_ig_expand, dim3(nr, nres), dim3(kIgxThreads), 0, st, ea);
                LAUNCH_CHECK("k_ig_expand");
            }
            cb.B = nr;
            if ((!freq_only && forward_trunk(h, &cb, 1, st, B)) || forward_reg_head(h, &cb, h->aw.logits, 1, st, nullptr)) return -1;
            n_fwd += g_launches - l0;
            l0 = g_launches;
            if (backward_impl(h, &cb, st, freq_only ? 3 : 7, nullptr, 1.f, nullptr, po)) return -1;
            if (ip || ic) {
                if (launch_input_grad(h, cb, nr, ip ? h->aw.grad : no_grad, ic ? h->aw.grad + kMaxRes : no_grad, smem, st)) return -1;
            }
            if (ifr) {
                const int ne = nr * TT;
                hipLaunchKernelGGL(k_dfreq_sum, dim3((ne + 255) / 256), dim3(256), 0, st, h->dfreq_part, h->aw.grad[2 * kMaxRes], ne, nres);
                LAUNCH_CHECK("k_dfreq_sum");
            }
            aa.g0 = g0;
            aa.n = nr;
            const dim3 acc_grid((g0 + nr - 1) / V - g0 / V + 1, kIgSlices);
            if (donor) {
                ra.a = aa;
                hipLaunchKernelGGL(k_ig_accumulate_raw_donor, acc_grid, dim3(kIgxThreads), 0, st, ra);
                LAUNCH_CHECK("k_ig_accumulate_raw_donor");
            } else if (raw) {
                ra.a = aa;
                hipLaunchKernelGGL(k_ig_accumulate_raw, acc_grid, dim3(kIgxThreads), 0, st, ra);
                LAUNCH_CHECK("k_ig_accumulate_raw");
            } else {
                hipLaunchKernelGGL(k_ig_accumulate, acc_grid, dim3(kIgxThreads), 0, st, aa);
                LAUNCH_CHECK("k_ig_accumulate");
            }
            n_bwd += g_launches - l0;
        }
        l0 = g_launches;
        hipLaunchKernelGGL(k_ig_delta, dim3((B + 63) / 64), dim3(64), 0, st, h->aw.slice_sums, logits_x, logits_base, delta, B, c.n_out, o->target);
        LAUNCH_CHECK("k_ig_delta");
        n_bwd += g_launches - l0;
        return 0;
    };
    const bool pend_record = h->pend_record;      // (a step record queued for the next training backward stays queued for it)
    h->pend_record = false;
    const int rc = run();
    h->pend_record = pend_record;
    h->last_fwd_B = 0;
    h->n_fwd = (int)n_fwd;
    h->n_bwd = (int)n_bwd;
    return rc ? -1 : 0;
}

extern "C" int cf_integrated_gradients(cf_handle* h, const cf_batch* bt, const cf_ig_opts* o, const cf_input_grads* out,
                                       float* logits_x, float* logits_base, float* delta, void* stream) {
    return integrated_gradients_impl(h, bt, o, out, nullptr, logits_x, logits_base, delta, stream, kIgLinear, "cf_integrated_gradients");
}

// Integrated gradients along the zero-signal path a m in bin-mean space (cf_ig.h, kIgSignal): the launches of cf_integrated_gradients
// with k_ig_expand_raw / k_ig_accumulate_raw in place of k_ig_expand / k_ig_accumulate.
extern "C" int cf_integrated_gradients_raw(cf_handle* h, const cf_batch* bt, const cf_ig_opts* o, const cf_input_grads* out,
                                           const cf_input_grads* coeff, float* logits_x, float* logits_base, float* delta, void* stream) {
    return integrated_gradients_impl(h, bt, o, out, coeff, logits_x, logits_base, delta, stream, kIgSignal, "cf_integrated_gradients_raw");
}

// Integrated gradients along x(a) = xd + a (x - xd) between two raw signals, in bin-mean space (cf_ig.h, kIgSignalDonor): the launches of
// cf_integrated_gradients_raw with k_ig_expand_raw_donor / k_ig_accumulate_raw_donor; the donor's features travel in opts->base_promoter_feats /
// base_pcre_feats.
extern "C" int cf_integrated_gradients_raw_donor(cf_handle* h, const cf_batch* bt, const cf_ig_opts* o, const cf_input_grads* out,
                                                 const cf_input_grads* cmean, float* logits_x, float* logits_base, float* delta, void* stream) {
    return integrated_gradients_impl(h, bt, o, out, cmean, logits_x, logits_base, delta, stream, kIgSignalDonor, "cf_integrated_gradients_raw_donor");
}

// The geometry the scans and the window games stand on.  coarsest: the resolution with the fewest bins (*rc), every n_bins a multiple of
// its W; finest: the resolution with the smallest bins (*rf), its L_f a multiple of every n_bins.
static int coarsest(cf_handle* h, const char* who, int* rc) {
    const cf_config& c = h->cfg;
    *rc = 0;
    for (int r = 1; r < c.n_res; ++r)
        if (c.n_bins[r] < c.n_bins[*rc]) *rc = r;
    const int W = c.n_bins[*rc];
    for (int r = 0; r < c.n_res; ++r)
        if (c.n_bins[r] % W) return fail("%s: n_bins[%d] = %d is not a multiple of the coarsest resolution's %d bins", who, r, c.n_bins[r], W);
    return 0;
}
static int finest(cf_handle* h, const char* who, int* rf) {
    const cf_config& c = h->cfg;
    *rf = 0;
    for (int r = 1; r < c.n_res; ++r)
        if (c.binsizes[r] < c.binsizes[*rf]) *rf = r;
    const int Lf = c.n_bins[*rf];
    for (int r = 0; r < c.n_res; ++r)
        if (Lf % c.n_bins[r])
            return fail("%s: n_bins[%d] = %d of the finest resolution is not a multiple of n_bins[%d] = %d", who, *rf, Lf, r, c.n_bins[r]);
    return 0;
}
// The centre pad-mask row of region `region` (0 the promoter, 1 + j pCRE slot j) of gene b at resolution r: *row + b * *stride.
static void region_mask_row(const cf_batch* bt, int region, int r, int S, const uint8_t** row, long long* stride) {
    if (region == 0) {
        *row = bt->promoter_mask_row[r];
        *stride = bt->promoter_mask_stride[r];
    } else {
        *row = bt->pcre_mask_row[r] + (long long)(region - 1) * bt->pcre_mask_stride[r];
        *stride = (long long)S * bt->pcre_mask_stride[r];
    }
}

// The samples of the last real finest bin of each gene, cnt_last[b], from the region's finest centre pad-mask rows m [B, Lf] (a host
// copy) and its lengths: gene b has n_f real bins (first to last unmasked byte), lengths[b] must lie in ((n_f - 1) b_f, n_f b_f].  A
// gene without a real bin (a dummy slot: nothing is edited there) keeps its count and its length is not read.  Host arithmetic only.
static int fine_tail_counts(const uint8_t* m, int B, int Lf, int bf, const int* lengths, unsigned* cnt_last, const char* who) {
    for (int b = 0; b < B; ++b) {
        int lo = Lf, hi = 0;
        for (int k = 0; k < Lf; ++k)
            if (!m[(size_t)b * Lf + k]) lo = std::min(lo, k), hi = k + 1;
        const long long nf = hi > lo ? hi - lo : 0, len = lengths[b];
        if (!nf) continue;
        if (len <= (nf - 1) * bf || len > nf * bf)
            return fail("%s: lengths[%d] = %lld outside ((n_f - 1) b_f, n_f b_f] = (%lld, %lld]: the region has n_f = %lld real bins of b_f = %d samples",
                        who, b, len, (nf - 1) * bf, nf * bf, nf, bf);
        cnt_last[b] = (unsigned)(len - (nf - 1) * bf);
    }
    return 0;
}
// out[0, 2 B) = [start[B] | cnt_last[B]], the words the fine kernels read behind their tables: start (null: all 0) and the samples of
// the last real finest bin (b_f; with `lengths`: fine_tail_counts on the finest centre pad-mask rows of the region, read back once -- a
// copy, no launch).
static int fine_tail_words(cf_handle* h, const cf_batch* bt, int region, int rf, const int* start, const int* lengths, hipStream_t st, const char* who,
                           unsigned* out) {
    const int B = bt->B, Lf = h->cfg.n_bins[rf], bf = h->cfg.binsizes[rf];
    for (int b = 0; b < B; ++b) out[b] = start ? (unsigned)start[b] : 0u, out[B + b] = (unsigned)bf;
    if (!lengths || B <= 0) return 0;
    const uint8_t* rm;
    long long rm_stride;
    region_mask_row(bt, region, rf, h->cfg.i_max, &rm, &rm_stride);
    std::vector<uint8_t> m((size_t)B * Lf);
    HIP_TRY(hipMemcpy2DAsync(m.data(), Lf, rm, (size_t)rm_stride, Lf, B, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return fine_tail_counts(m.data(), B, Lf, bf, lengths, out + B, who);
}

// What the scan entry points check alike, in front of anything launched.  scan_check: the window, the mark sets, the scale, nested
// bin counts (*rc_out: the coarsest resolution); scan_upload_sets: the workspace is allocated and holds the mark sets.
static int scan_check(cf_handle* h, int width, int n_sets, const unsigned* mark_sets, float scale, const char* who, int* rc_out) {
    const cf_config& c = h->cfg;
    const int F = c.n_feats;
    if (width < 1) return fail("%s: width = %d: at least 1 coarsest bin", who, width);
    if (n_sets < 1) return fail("%s: n_sets = %d: at least 1 mark set", who, n_sets);
    if (!(scale >= 0.f) || !std::isfinite(scale)) return fail("%s: scale = %g: a finite factor >= 0", who, (double)scale);
    for (int k = 0; k < n_sets; ++k)
        if (F < 32 && mark_sets[k] >> F) return fail("%s: mark_sets[%d] = 0x%x names a mark >= n_feats = %d", who, k, mark_sets[k], F);
    return coarsest(h, who, rc_out);
}
static int scan_upload_sets(cf_handle* h, const unsigned* mark_sets, int n_sets, hipStream_t st, const char* who) {
    if (attrib_ws(h, who) || h->aw.words.need(n_sets, 128, who)) return -1;
    HIP_TRY(hipMemcpyAsync(h->aw.words, mark_sets, n_sets * sizeof(unsigned), hipMemcpyHostToDevice, st));
    return 0;
}

// One region of a scan, every row through the whole forward (chunk_forward).  Per chunk of at most max_batch of the B * V rows
// (gene-major; V = 1 + n_sets * W): the scan's expand kernel into the chunk workspace (the mark sets are in its word table, uploaded by
// the caller), then the launches of cf_forward(save = 0) on the chunk.  The result does not depend on max_batch and row (b, v) carries
// the bits of cf_forward(save = 0) on the batch with the perturbed features substituted.
// `ea`: ScanExpandArgs or ScanFineExpandArgs (cf_scan_fine.h) with the fields of its kernel alone set by the caller; what the two share
// is filled in here.
template <class Args>
static int scan_rows(cf_handle* h, const cf_batch* bt, void (*kernel)(Args), const char* name, Args& ea, int region, float* const feats_out[], int V,
                     float* logits, hipStream_t st) {
    const cf_config& c = h->cfg;
    const int nres = c.n_res;
    cf_batch cb;      // the chunk's batch: the rows' copies
    chunk_rows(h, bt, &ea.rows, &cb);
    for (int r = 0; r < nres; ++r) {
        ea.pf_in[r] = bt->promoter_feats[r];
        ea.cf_in[r] = bt->pcre_feats[r];
        ea.pf_out[r] = h->aw.row[r];
        ea.cf_out[r] = h->aw.row[kMaxRes + r];
        ea.feats_out[r] = feats_out[r];
        region_mask_row(bt, region, r, c.i_max, &ea.rm_in[r], &ea.rm_stride[r]);
    }
    ea.freq_in = bt->interaction_freq;
    ea.freq_out = h->aw.row[2 * kMaxRes];
    ea.sets = h->aw.words;
    ea.V = V, ea.F = c.n_feats, ea.region = region;
    return chunk_forward(h, &cb, (long long)bt->B * V, logits, true, bt->B, st, [&](long long g0, int n) {
        ea.g0 = (int)g0;
        return launch_expand(kernel, name, dim3(n, nres), kIgxThreads, ea, st);
    });
}
static int scan_region_rows(cf_handle* h, const cf_batch* bt, const cf_scan_opts* o, int rc, float* logits, hipStream_t st) {
    const int W = h->cfg.n_bins[rc];
    ScanExpandArgs ea;
    memset(&ea, 0, sizeof ea);
    ea.flip = o->flip;
    ea.scale = o->scale;
    ea.W = W, ea.width = o->width, ea.rc = rc;
    return scan_rows(h, bt, k_scan_expand, "k_scan_expand", ea, o->region, o->feats_out, 1 + o->n_sets * W, logits, st);
}

// In-silico perturbation scan of one region (cf_scan.h): scan_region_rows.
extern "C" int cf_perturbation_scan(cf_handle* h, const cf_batch* bt, const cf_scan_opts* o, float* logits, void* stream) {
    const char* who = "cf_perturbation_scan";
    if (attrib_open(h, bt, true, who)) return -1;
    if (!o) return fail("%s: null opts", who);
    if (!logits) return fail("%s: null logits", who);
    if (!o->mark_sets) return fail("%s: null mark_sets", who);
    const cf_config& c = h->cfg;
    if (o->region < 0 || o->region > c.i_max) return fail("%s: region = %d outside [0, i_max = %d]", who, o->region, c.i_max);
    int rc = 0;
    if (scan_check(h, o->width, o->n_sets, o->mark_sets, o->scale, who, &rc)) return -1;
    for (int r = c.n_res; r < kMaxRes; ++r)
        if (o->feats_out[r]) return fail("%s: feats_out[%d]: the model has %d resolutions", who, r, c.n_res);
    hipStream_t st = (hipStream_t)stream;
    if (scan_upload_sets(h, o->mark_sets, o->n_sets, st, who)) return -1;
    const long long launches0 = g_launches;
    const int rv = scan_region_rows(h, bt, o, rc, logits, st);
    h->x0_fwd = false;
    forward_counted(h, launches0);
    return rv ? -1 : 0;
}

// The variants of pCRE slot `slot`, slot-packed (cf_scan.h), into `logits` [B, V, n_out].  The caller has stashed the B genes' trunk
// output in the workspace's stash and uploaded the mark sets.  Pack phase, per chunk of at most max_batch of the B * U pseudo rows: k_scan_pack,
// the trunk (k_attc2's regions per workgroup as for the caller's B genes, as scan_region_rows), k_scan_unpack into slot_rows.  Row phase,
// per chunk of at most max_batch of the B * V rows: k_scan_rows, the Regulation + head launches of an inference forward.
static int scan_slot_packed(cf_handle* h, const cf_batch* bt, const cf_scan_regions_opts* o, int slot, int rc, float* logits, hipStream_t st) {
    const cf_config& c = h->cfg;
    const int nres = c.n_res, S = c.i_max, T = S + 1, cap = c.max_batch, W = c.n_bins[rc], d4 = c.d_emb / 4;
    const int B = bt->B, V = 1 + o->n_sets * W, U = (V - 1 + S - 1) / S;
    ScanPackArgs pa;
    ScanUnpackArgs ua;
    ScanRowsArgs ra;
    memset(&pa, 0, sizeof pa);
    memset(&ua, 0, sizeof ua);
    memset(&ra, 0, sizeof ra);
    cf_batch cb;      // the chunk's batch: pseudo-genes for the trunk, then rows (masks and frequencies) for Regulation + head
    chunk_rows(h, bt, &pa.rows, &cb);
    ra.rows = pa.rows;
    const size_t xv_res = (size_t)B * (V - 1) * c.d_emb;
    for (int r = 0; r < nres; ++r) {
        pa.pf_in[r] = bt->promoter_feats[r];
        pa.cf_in[r] = bt->pcre_feats[r];
        pa.pf_out[r] = h->aw.row[r];
        pa.cf_out[r] = h->aw.row[kMaxRes + r];
        ua.x0[r] = reinterpret_cast<const float4*>(h->Rx[r][0]);
        ua.xv[r] = reinterpret_cast<float4*>(h->aw.slot_rows + r * xv_res);
        ra.stash[r] = reinterpret_cast<const float4*>(h->aw.stash[r]);
        ra.xv[r] = ua.xv[r];
        ra.x0[r] = reinterpret_cast<float4*>(h->Rx[r][0]);
    }
    pa.sets = h->aw.words;
    pa.scale = o->scale;
    pa.U = U, pa.V = V, pa.F = c.n_feats, pa.W = W, pa.width = o->width, pa.rc = rc, pa.slot = slot;
    ua.U = U, ua.V = V, ua.S = S, ua.T = T, ua.d4 = d4;
    ra.freq_in = bt->interaction_freq;
    ra.freq_out = h->aw.row[2 * kMaxRes];
    ra.V = V, ra.row4 = T * d4, ra.d4 = d4, ra.slot = slot;
    for (int g0 = 0; g0 < B * U; g0 += cap) {
        const int n = std::min(cap, B * U - g0);
        pa.g0 = ua.g0 = g0;
        hipLaunchKernelGGL(k_scan_pack, dim3(n, nres), dim3(kIgxThreads), 0, st, pa);
        LAUNCH_CHECK("k_scan_pack");
        cb.B = n;
        if (forward_trunk(h, &cb, 0, st, B)) return -1;
        hipLaunchKernelGGL(k_scan_unpack, dim3(n, nres), dim3(kRowThreads), 0, st, ua);
        LAUNCH_CHECK("k_scan_unpack");
    }
    return chunk_forward(h, &cb, (long long)B * V, logits, false, B, st, [&](long long g0, int n) {
        ra.g0 = (int)g0;
        return launch_expand(k_scan_rows, "k_scan_rows", dim3(n, nres), kRowThreads, ra, st);
    });
}

// The scan of several regions of every gene from one call: the promoter block through scan_region_rows, the pCRE blocks slot-packed
// (scan_slot_packed; CF_SCAN_PACK=0 at cf_create: through scan_region_rows as well, the cross-check).
extern "C" int cf_perturbation_scan_regions(cf_handle* h, const cf_batch* bt, const cf_scan_regions_opts* o, float* logits, void* stream) {
    const char* who = "cf_perturbation_scan_regions";
    if (attrib_open(h, bt, true, who)) return -1;
    if (!o) return fail("%s: null opts", who);
    if (!logits) return fail("%s: null logits", who);
    if (!o->mark_sets) return fail("%s: null mark_sets", who);
    const cf_config& c = h->cfg;
    const int S = c.i_max;
    if (!o->regions) return fail("%s: regions = 0: at least one region bit (bit 0 the promoter, bit 1 + j pCRE slot j)", who);
    if (o->regions >> S >> 1) return fail("%s: regions = 0x%x names a region above i_max = %d", who, o->regions, S);
    int rc = 0;
    if (scan_check(h, o->width, o->n_sets, o->mark_sets, o->scale, who, &rc)) return -1;
    const bool packed = h->scan_pack && (o->regions >> 1);
    const int B = bt->B, V = 1 + o->n_sets * c.n_bins[rc];
    hipStream_t st = (hipStream_t)stream;
    if (scan_upload_sets(h, o->mark_sets, o->n_sets, st, who)) return -1;
    if (packed && h->aw.slot_rows.need((size_t)c.n_res * B * (V - 1) * c.d_emb, 0, who)) return -1;
    const long long launches0 = g_launches;
    const size_t block = (size_t)B * V * c.n_out;
    cf_scan_opts so;
    memset(&so, 0, sizeof so);
    so.width = o->width, so.n_sets = o->n_sets, so.mark_sets = o->mark_sets, so.scale = o->scale;
    int rv = 0, q = 0;
    if (packed) rv = forward_trunk(h, bt, 0, st) || stash_trunk_output(h, B, h->aw.stash, st);
    for (int region = 0; region <= S && !rv; ++region) {
        if (!(o->regions >> region & 1u)) continue;
        float* out = logits + q++ * block;
        so.region = region;
        so.flip = region == 0 ? o->flip : nullptr;      // (pCREs are never stored mirrored)
        rv = region == 0 || !packed ? scan_region_rows(h, bt, &so, rc, out, st) : scan_slot_packed(h, bt, o, region - 1, rc, out, st);
    }
    h->x0_fwd = false;
    forward_counted(h, launches0);
    return rv ? -1 : 0;
}

// Fine-resolution perturbation scan (cf_scan_fine.h): scan_rows with k_scan_fine_expand where scan_region_rows hands it k_scan_expand.
// The word table of the workspace holds [mark sets | start | samples of the last real finest bin] (fine_tail_words), uploaded here: no
// device buffer of its own.
extern "C" int cf_perturbation_scan_fine(cf_handle* h, const cf_batch* bt, const cf_scan_fine_opts* o, float* logits, void* stream) {
    const char* who = "cf_perturbation_scan_fine";
    if (attrib_open(h, bt, true, who)) return -1;
    if (!o) return fail("%s: null opts", who);
    if (!logits) return fail("%s: null logits", who);
    if (!o->mark_sets) return fail("%s: null mark_sets", who);
    const cf_config& c = h->cfg;
    const int nres = c.n_res, S = c.i_max, B = bt->B;
    if (o->region < 0 || o->region > S) return fail("%s: region = %d outside [0, i_max = %d]", who, o->region, S);
    if (o->width < 1) return fail("%s: width = %d: at least 1 finest bin", who, o->width);
    if (o->stride < 1) return fail("%s: stride = %d: at least 1 finest bin", who, o->stride);
    if (o->n_windows < 1) return fail("%s: n_windows = %d: at least 1 window", who, o->n_windows);
    int rc = 0, rf = 0;
    if (scan_check(h, 1, o->n_sets, o->mark_sets, o->scale, who, &rc) || finest(h, who, &rf)) return -1;
    for (int r = nres; r < kMaxRes; ++r)
        if (o->feats_out[r]) return fail("%s: feats_out[%d]: the model has %d resolutions", who, r, nres);
    for (int b = 0; o->start && b < B; ++b)
        if (o->start[b] < 0) return fail("%s: start[%d] = %d: a finest genomic bin >= 0", who, b, o->start[b]);
    const long long rows = (long long)B * (1 + (long long)o->n_sets * o->n_windows);
    if (rows > 0x7fffffffLL) return fail("%s: B * (1 + n_sets * n_windows) = %lld rows do not fit an int", who, rows);
    hipStream_t st = (hipStream_t)stream;
    std::vector<unsigned> words(o->n_sets + 2 * (size_t)B);
    memcpy(words.data(), o->mark_sets, o->n_sets * sizeof(unsigned));
    if (fine_tail_words(h, bt, o->region, rf, o->start, o->lengths, st, who, words.data() + o->n_sets)) return -1;
    if (attrib_ws(h, who) || h->aw.words.need(words.size(), 128, who)) return -1;
    HIP_TRY(hipMemcpyAsync(h->aw.words, words.data(), words.size() * sizeof(unsigned), hipMemcpyHostToDevice, st));
    ScanFineExpandArgs ea;
    memset(&ea, 0, sizeof ea);
    ea.start = reinterpret_cast<const int*>((unsigned*)h->aw.words) + o->n_sets;
    ea.cnt_last = ea.start + B;
    ea.flip = o->flip;
    ea.scale = o->scale;
    ea.NW = o->n_windows, ea.width = o->width, ea.stride = o->stride, ea.rf = rf, ea.bf = c.binsizes[rf];
    const long long launches0 = g_launches;
    const int rv = scan_rows(h, bt, k_scan_fine_expand, "k_scan_fine_expand", ea, o->region, o->feats_out, (int)(rows / std::max(B, 1)), logits, st);
    h->x0_fwd = false;
    forward_counted(h, launches0);
    return rv ? -1 : 0;
}
