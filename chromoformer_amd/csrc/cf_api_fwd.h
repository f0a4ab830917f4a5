// cf_api_fwd.h -- the forward pass: prologue, trunk (fused / layer by layer), Regulation stack (fused / layer by layer), head.
// Part of cf_api.hip's single translation unit: included there behind cf_api_ops.h, not on its own.
#pragma once

// ------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------
// the tiled copies of the Embedding + Pairwise weights, now (cf_keep_tiled: whenever somebody other than the fused optimiser has written them)
static int retile_early(cf_handle* h, hipStream_t st) {
    if (h->n_retile_early > 0) {
        hipLaunchKernelGGL(k_retile, dim3(h->n_retile_early), dim3(256), 0, st, (const float*)h->params, h->tiled, h->reg8 ? h->tiledT : (float*)nullptr,
                           (const RetileUnit*)h->retile_units);
        LAUNCH_CHECK("k_retile");
    }
    h->tiled_pe_fresh = true;
    return 0;
}
// Regulation + head re-tiling units ride in the Embedding layer's chain launch / the fused trunk's launch (CF_DEFER_RETILE=0: all in the prologue)
static bool defer_retile(const cf_handle* h) {
    return h->defer_retile && !h->embed_dense && kPostWaves == 8 && h->cfg.embed_heads == 2 && h->cfg.d_emb == 128;
}
// What comes in front of the Embedding + Pairwise stage: the tiled weight copies are refreshed (the parameters may have been changed by
// anyone since the last call), a pending batch gather is issued or taken into the same launch, the Embedding centre-row input is computed
// (stand-alone kernels only).  *adv_cursor: the feed cursor the fused trunk's launch is to move on (null: none).
static int forward_prologue(cf_handle* h, const cf_batch* bt, hipStream_t st, int** adv_cursor) {
    const cf_config& c = h->cfg;
    const int B = bt->B, nres = c.n_res;
    const bool defer = defer_retile(h), trunk = h->trunk;
    *adv_cursor = nullptr;
    // cf_keep_tiled: the Embedding + Pairwise units (the leading ones) are kept fresh by the optimiser epilogue; if something else has
    // written parameters since (cf_params_changed, cf_bind, a separate AdamW launch) they are re-tiled here, once, in a launch of their own
    if (h->keep_tiled && !h->tiled_pe_fresh && retile_early(h, st)) return -1;
    if (h->pend_gnext) {      // (a cf_gather_batch_next that found no reduction launch to ride in: a launch of its own, here)
        hipLaunchKernelGGL(k_gather_batch, dim3(h->pend_gn.B, h->pend_gn_n), dim3(256), 0, st, h->pend_gn);
        LAUNCH_CHECK("k_gather_batch");
        h->adv_next = h->pend_gn.cursor;
        h->pend_gnext = false;
    }
    // The pre-gathered feed's pending state belongs to ONE batch: only the forward pass over that batch takes the gather into its
    // launch / moves the cursor on.  A pass over another batch (Trainer.evaluate_store or model(...) between two steps of a fed epoch)
    // leaves it for the step it was queued for -- consumed here it advanced the cursor a second time under graph replay (the
    // captured trunk launch advances it by itself) and the epoch silently skipped a batch.
    const bool mine = !h->pend_key || h->pend_key == (const void*)bt->promoter_feats[0];
    const int u0 = h->keep_tiled ? h->n_retile_early : 0;
    const int n_now = (defer ? h->n_retile_early : h->n_retile) - u0;
    const RetileUnit* units = (const RetileUnit*)h->retile_units + u0;
    float* tiledT = h->reg8 ? h->tiledT : (float*)nullptr;
    const bool with_gather = mine && h->pend_gather && trunk && h->pend_ga.B == B;
    if (mine && h->pend_gather && !with_gather && gather_launch(h->pend_ga, h->pend_ga_n, st)) return -1;      // (launches of their own, as cf_gather_batch)
    if (with_gather) {      // the step's batch gather in the same launch (cf_gather_batch_fwd); the trunk's forward launch advances the cursor
        hipLaunchKernelGGL(k_prologue_gather, dim3(n_now + B * h->pend_ga_n), dim3(256), 0, st, (const float*)h->params, h->tiled, tiledT, units, n_now,
                           h->pend_ga);
        LAUNCH_CHECK("k_prologue_gather");
    } else if (n_now + (trunk ? 0 : B * nres) > 0) {      // (nothing to re-tile and nothing to gather: no launch)
        // (the fused trunk computes the Embedding input row itself: no x0 workgroups then, and nobody reads `a`)
        X0Args a;
        for (int r = 0; r < nres; ++r) {
            a.feats[r] = bt->promoter_feats[r];
            a.pe[r] = h->pe[r];
            a.wlp[r] = h->refs.lin_proj[r];
            a.x0[r] = h->ex0[r];
            a.featc[r] = h->featc[r];
            a.L[r] = c.n_bins[r];
        }
        a.F = c.n_feats;
        if (with_int<64, 128, 256>("d_emb", c.d_emb, [&](auto d) {
                hipLaunchKernelGGL(k_fwd_prologue<decltype(d)::value>, dim3(n_now + (trunk ? 0 : B * nres)), dim3(256), 0, st, (const float*)h->params, h->tiled,
                                   tiledT, units, n_now, a, B);
                return 0;
            }))
            return -1;
        LAUNCH_CHECK("k_fwd_prologue");
    }
    if (mine) h->pend_gather = false;
    if (with_gather) *adv_cursor = h->pend_ga.cursor;
    else if (mine && h->adv_next) {      // the batch is in place already (cf_gather_batch_only / cf_gather_batch_next): only the cursor moves on
        if (trunk) *adv_cursor = h->adv_next;
        else {
            hipLaunchKernelGGL(k_gather_advance, dim3(1), dim3(1), 0, st, h->adv_next);
            LAUNCH_CHECK("k_gather_advance");
        }
    }
    if (mine) {
        h->adv_next = nullptr;
        h->pend_key = nullptr;
    }
    return 0;
}
// Embedding + Pairwise stage as ONE launch (cf_trunk.h)
static int trunk_fwd_fused(cf_handle* h, const cf_batch* bt, int save, int* adv_cursor, hipStream_t st) {
    const cf_config& c = h->cfg;
    const bool defer = defer_retile(h);
    TrunkArgs ta;
    trunk_args(h, bt, ta, save);
    if (defer) {
        ta.rt_units = h->retile_units + h->n_retile_early;
        ta.rt_n = h->n_retile - h->n_retile_early;
        ta.rt_params = h->params;
        ta.rt_tiled = h->tiled;
        ta.rt_tiledT = h->reg8 ? h->tiledT : nullptr;
    }
    ta.adv_cursor = adv_cursor;
    void* kargs[] = {&ta};
    h->time_mark("k_trunk_fwd", st);
    HIP_TRY(hipLaunchKernel(trunk_kernel(false, c.embed_dff, c.pair_dff, c.pair_layers), dim3(bt->B, c.n_res + (defer && ta.rt_n > 0 ? 1 : 0)), dim3(kAT), kargs,
                            h->trunk_smem_bytes, st));
    h->time_mark("k_trunk_fwd", st);
    LAUNCH_CHECK("k_trunk_fwd");
    return 0;
}

// One centre-row stage -- the Embedding layer (l < 0) or Pairwise layer l, over every resolution -- as centre_fwd / centre_bwd launch it
struct CentreStage {
    CentreBuf* buf[kMaxRes];
    const CentreParams* prm[kMaxRes];
    const float* const* feats;            // the batch's features and pad-mask rows of the stage's regions
    const uint8_t* const* mask;
    const long long* mstride;
    int N, dff, nh;                       // rows per resolution, FFN width, heads
    // forward: input and output rows
    const float* xin[kMaxRes];
    float* out[kMaxRes];
    RowMap xmap, omap;
    bool copy_x = false;                  // materialise the row-mapped input rows (CentreBuf::xin)
    bool q_done = false;                  // the previous stage's chain kernel has already run this stage's query chain
    const CentreStage* next = nullptr;    // ... and this one's runs that stage's (only for identity row maps: the output tile IS its input)
    const float* lin_w[kMaxRes] = {};     // optional trailing Linear on the output rows (PostArgs::lin_w / lin_y)
    float* lin_y[kMaxRes] = {};
    bool host_retile = false;             // the Regulation + head re-tiling units ride in the chain launch (PostArgs::rt_units)
    // backward: gradient of the output rows
    const float* dout[kMaxRes];
    RowMap dmap;
};
static CentreStage centre_stage(cf_handle* h, const cf_batch* bt, int l) {
    const cf_config& c = h->cfg;
    const bool emb = l < 0;
    CentreStage s{};
    for (int r = 0; r < c.n_res; ++r) {
        s.buf[r] = emb ? &h->E[r] : &h->P[r][l];
        s.prm[r] = emb ? &h->refs.E[r] : &h->refs.P[r][l];
    }
    s.feats = emb ? bt->promoter_feats : bt->pcre_feats;
    s.mask = emb ? bt->promoter_mask_row : bt->pcre_mask_row;
    s.mstride = emb ? bt->promoter_mask_stride : bt->pcre_mask_stride;
    s.N = emb ? bt->B : bt->B * c.i_max;
    s.dff = emb ? c.embed_dff : c.pair_dff;
    s.nh = emb ? c.embed_heads : c.pair_heads;
    return s;
}
// the attention launch's arguments of a stage, either direction (vin / w / vout are the caller's); returns the one-sequence kernel's LDS bytes
static size_t centre_attc_args(const cf_handle* h, const CentreStage& s, bool bwd, AttcArgs& at) {
    const cf_config& c = h->cfg;
    size_t smem = 0;
    for (int r = 0; r < c.n_res; ++r) {
        at.feats[r] = s.feats[r], at.mask[r] = s.mask[r], at.mstride[r] = s.mstride[r];
        at.pe[r] = h->pe[r], at.pet[r] = h->pet[r], at.wlp[r] = s.prm[r]->wlp, at.p[r] = s.buf[r]->p, at.L[r] = c.n_bins[r];
        smem = std::max(smem, attc_smem(c.n_bins[r], c.n_feats, bwd, s.nh, c.d_emb));
    }
    at.F = c.n_feats;
    at.scale = sqrtf((float)(c.d_emb / s.nh));      // sqrt(d_head), modules.py:60-61
    return smem;
}
// what a post chain reads from the parameters and saves for the backward pass: CentreParams / RegParams and CentreBuf / RegBuf name it alike
template <class Params, class Buf>
static void post_fwd_common(PostArgs& po, int r, const Params& p, const Buf& b) {
    po.bo[r] = p.bo, po.g1[r] = p.g1, po.be1[r] = p.be1, po.b1[r] = p.b1, po.b2[r] = p.b2, po.g2[r] = p.g2, po.be2[r] = p.be2;
    po.xh1[r] = b.xh1, po.rs1[r] = b.rs1, po.y1[r] = b.y1, po.hdn[r] = b.hdn, po.xh2[r] = b.xh2, po.rs2[r] = b.rs2;
}
static size_t centre_fwd_args(const cf_handle* h, const CentreStage& s, int save, QChainArgs& q, AttcArgs& at, PostArgs& po) {
    const size_t smem = centre_attc_args(h, s, false, at);
    for (int r = 0; r < h->cfg.n_res; ++r) {
        const CentreBuf& b = *s.buf[r];
        const CentreParams& p = *s.prm[r];
        q.x[r] = s.xin[r], q.q[r] = b.q, q.qt[r] = b.qt, q.xcopy[r] = s.copy_x ? b.xin : nullptr;
        q.wq[r] = p.wq_t, q.wk[r] = p.wk;      // NT product: tiled copy; NN product: row-major
        at.vin[r] = b.qt, at.w[r] = b.w, at.vout[r] = b.xbar;
        post_fwd_common(po, r, p, b);
        po.x[r] = s.xin[r], po.ain[r] = b.xbar, po.a_out[r] = b.a, po.out[r] = s.out[r];
        po.wv[r] = p.wv_t, po.wo[r] = p.wo_t, po.w1[r] = p.w1_t, po.w2[r] = p.w2_t;
        po.lin_w[r] = s.lin_w[r], po.lin_y[r] = s.lin_y[r];
        if (s.next) {
            po.nq_wq[r] = s.next->prm[r]->wq_t, po.nq_wk[r] = s.next->prm[r]->wk;
            po.nq_q[r] = s.next->buf[r]->q, po.nq_qt[r] = s.next->buf[r]->qt;
        }
    }
    q.xmap = po.xmap = s.xmap, po.omap = s.omap;
    q.N = po.N = s.N;
    po.save = save;
    return smem;
}
// one centre-row layer: query chain -> attention -> post chain
static int centre_fwd(cf_handle* h, const CentreStage& s, int B, int save, int ag_genes, hipStream_t st) {
    const cf_config& c = h->cfg;
    const int kD = c.d_emb, nres = c.n_res, N = s.N;      // (kD: row width, shadows cf::kD)
    QChainArgs q;
    AttcArgs at;
    PostArgs po;
    const size_t smem = centre_fwd_args(h, s, save, q, at, po);
    if (kD != 128 && smem > 64 * 1024)
        return fail("cf_forward: a region of %d bins does not fit the one-sequence attention at d_emb = %d", c.n_bins[nres - 1], kD);
    if (kD != 128 || s.nh != 2)      // every shape but the default: the stand-alone kernels instantiated for it
        return with_centre_shape(kD, s.nh, [&](auto d, auto nh) {
            return centre_fwd_heads<decltype(nh)::value, decltype(d)::value>(st, N, nres, s.dff, s.q_done, q, at, smem, po);
        });
    if (!s.q_done) {
        hipLaunchKernelGGL((k_qchain_fwd<kPostWaves>), dim3(tiles_of(N), nres), dim3(kPostWaves * 64), 0, st, q);
        LAUNCH_CHECK("k_qchain_fwd");
    }
    if (launch_attc<false>(h, at, N, B, smem, ag_genes, st)) return -1;
    dim3 pgrid(tiles_of(N), nres);
    if (s.host_retile) {
        po.rt_units = h->retile_units + h->n_retile_early;
        po.rt_n = h->n_retile - h->n_retile_early;
        po.rt_params = h->params;
        po.rt_tiled = h->tiled;
        po.rt_tiledT = h->reg8 ? h->tiledT : nullptr;
        po.rt_y0 = nres;
        pgrid.y += (po.rt_n + pgrid.x - 1) / pgrid.x;
    }
    if (launch_post_fwd<true, 128>(s.dff, pgrid, st, po)) return -1;
    LAUNCH_CHECK("k_post_fwd<centre>");
    return 0;
}
// Embedding + Pairwise stage on the stand-alone kernels, layer by layer
static int trunk_fwd_layers(cf_handle* h, const cf_batch* bt, int save, int ag_genes, hipStream_t st) {
    const cf_config& c = h->cfg;
    const int kD = c.d_emb;      // (row width: shadows cf::kD in this function; 128, or 64 / 256 through the stand-alone kernels)
    const int B = bt->B, S = c.i_max, T = S + 1, nres = c.n_res;
    if (h->embed_dense) {   // Embedding with more than one layer: every row of every layer (cf_embed_full.h + dense layers)
        if (embed_dense_forward(h, bt, save != 0, st)) return -1;
        LinArgs a;          // lin_proj_p on the promoter centre embedding (net.py:118)
        for (int r = 0; r < nres; ++r) {
            a.x[r] = h->Rx[r][0];
            a.w[r] = h->tiled_of(h->refs.lin_proj_p[r]);
            a.b[r] = nullptr;
            a.y[r] = h->xp0[r];
        }
        a.xmap = RowMap{1, T, 0, 0};
        a.ldx = kD;
        a.ldy = kD;
        a.N = B;
        a.K = kD;
        a.Nout = kD;
        a.relu = 0;
        hipLaunchKernelGGL((k_linear_fwd<2>), dim3(tiles_of(B), 1, nres), dim3(256), 0, st, a);
        LAUNCH_CHECK("k_linear_fwd<lin_proj_p>");
    } else {   // Embedding, with lin_proj_p on the promoter centre embedding (net.py:118) as the last product of the layer's chain kernel
        CentreStage s = centre_stage(h, bt, -1);
        for (int r = 0; r < nres; ++r) {
            s.xin[r] = h->ex0[r];
            s.out[r] = h->Rx[r][0];
            s.lin_w[r] = h->tiled_of(h->refs.lin_proj_p[r]);
            s.lin_y[r] = h->xp0[r];
        }
        s.xmap = identity_map();
        s.omap = RowMap{1, T, 0, 0};
        s.host_retile = defer_retile(h);
        if (centre_fwd(h, s, B, save, ag_genes, st)) return -1;
    }
    for (int l = 0; l < c.pair_layers; ++l) {   // Pairwise layers
        const bool last = l + 1 == c.pair_layers;
        CentreStage s = centre_stage(h, bt, l), next;
        for (int r = 0; r < nres; ++r) {
            s.xin[r] = l == 0 ? h->xp0[r] : h->P[r][l - 1].out;
            s.out[r] = last ? h->Rx[r][0] : h->P[r][l].out;
        }
        s.xmap = l == 0 ? RowMap{S, 1, 0, 0} : identity_map();
        s.omap = last ? RowMap{S, T, 1, 1} : identity_map();
        s.copy_x = l == 0;
        s.q_done = l > 0;
        if (!last) {
            next = centre_stage(h, bt, l + 1);
            s.next = &next;
        }
        if (centre_fwd(h, s, B, save, ag_genes, st)) return -1;
    }
    return 0;
}
// The forward pass in two parts: the trunk (prologue, Embedding + Pairwise stage) writes the Regulation input Rx[r][0]; the
// Regulation stack and the head read it with the batch's interaction masks and frequencies (cf_pcre_ablation runs the second part
// on gene-variant chunks of the first one's output).
static int forward_trunk(cf_handle* h, const cf_batch* bt, int save, hipStream_t st, int ag_genes = 0) {
    int* adv_cursor = nullptr;
    if (forward_prologue(h, bt, st, &adv_cursor)) return -1;
    return h->trunk ? trunk_fwd_fused(h, bt, save, adv_cursor, st) : trunk_fwd_layers(h, bt, save, ag_genes, st);
}

// what the fused Regulation launches of both directions share (the caller sets save, tdbg, head, l_top / l_bot, dfreq)
static void reg_args(const cf_handle* h, const cf_batch* bt, RegArgs& ra) {
    const cf_config& c = h->cfg;
    ra.tab = h->reg_tab;
    ra.n_layers = c.reg_layers, ra.T = c.i_max + 1, ra.B = bt->B, ra.n_res = c.n_res, ra.xcd_map = h->xcd_map;
    for (int r = 0; r < c.n_res; ++r) ra.mask[r] = bt->interaction_mask[r];
    ra.freq = bt->interaction_freq;
    memset(&ra.head, 0, sizeof ra.head);
    ra.row0_last = h->reg_row0 ? 1 : 0;
    ra.l_top = c.reg_layers - 1, ra.l_bot = 0;
    ra.dfreq = nullptr;
}
// Regulation: all layers in one launch, one workgroup per (gene, resolution)
static int reg_fwd_fused(cf_handle* h, const cf_batch* bt, int save, hipStream_t st, const HeadRide* ride) {
    const cf_config& c = h->cfg;
    RegArgs ra;
    reg_args(h, bt, ra);
    ra.save = save;
    ra.tdbg = getenv("CF_STAMP") ? reinterpret_cast<unsigned long long*>(h->tdbg) : nullptr;
    if (ride) ra.head = *ride;
    return launch_reg(h, "k_reg_fwd", reg_kernel(false, c.reg_dff, save != 0), dim3(8 * ((bt->B * c.n_res + 7) / 8)), reg8_fwd_smem(c.reg_dff), ra, st);
}
// the attention stage of Regulation layer l on the stand-alone kernel, either direction (a / dqkvg / dgam / dfreq are the caller's)
static void reg_attr_args(const cf_handle* h, const cf_batch* bt, int l, AttrArgs& at) {
    const cf_config& c = h->cfg;
    for (int r = 0; r < c.n_res; ++r)
        at.qkvg[r] = h->R[r][l].qkvg, at.mask[r] = bt->interaction_mask[r], at.gamma[r] = h->refs.R[r][l].gamma, at.p[r] = h->R[r][l].p;
    at.freq = bt->interaction_freq;
    at.T = c.i_max + 1, at.H = c.reg_heads, at.DM = c.reg_dmodel;
}
static void reg_fwd_args(const cf_handle* h, const cf_batch* bt, int l, int save, LinArgs& la, AttrArgs& at, PostArgs& po) {
    const cf_config& c = h->cfg;
    const int kD = c.d_emb, NR = bt->B * (c.i_max + 1), RW = 4 * c.reg_dmodel;
    reg_attr_args(h, bt, l, at);
    for (int r = 0; r < c.n_res; ++r) {
        const RegParams& p = h->refs.R[r][l];
        const RegBuf& b = h->R[r][l];
        la.x[r] = h->Rx[r][l], la.w[r] = h->tiled_of(p.watt), la.b[r] = nullptr, la.y[r] = b.qkvg;
        at.a[r] = b.a, at.dqkvg[r] = nullptr, at.dgam[r] = nullptr;
        post_fwd_common(po, r, p, b);
        po.x[r] = h->Rx[r][l], po.ain[r] = b.a, po.a_out[r] = nullptr, po.out[r] = h->Rx[r][l + 1];
        po.wv[r] = nullptr, po.wo[r] = h->tiled_of(p.wo), po.w1[r] = h->tiled_of(p.w1), po.w2[r] = h->tiled_of(p.w2);
    }
    la.xmap = po.xmap = po.omap = identity_map();
    la.ldx = la.K = kD, la.ldy = la.Nout = RW, la.relu = 0;
    la.N = po.N = NR;
    po.save = save;
}
// Regulation layer by layer on the stand-alone kernels (every shape the fused kernels are not written for; CF_REG_FUSED=0)
static int reg_fwd_layers(cf_handle* h, const cf_batch* bt, int save, hipStream_t st) {
    const cf_config& c = h->cfg;
    const int kD = c.d_emb, B = bt->B, T = c.i_max + 1, nres = c.n_res, NR = B * T, RDm = c.reg_dmodel, RW = 4 * RDm;
    for (int l = 0; l < c.reg_layers; ++l) {
        LinArgs la;
        AttrArgs at;
        PostArgs po;
        reg_fwd_args(h, bt, l, save, la, at, po);
        if (kD == 64) hipLaunchKernelGGL((k_linear_fwd<4, 64>), dim3(tiles_of(NR), RW / 256, nres), dim3(256), 0, st, la);
        else hipLaunchKernelGGL((k_linear_fwd<4>), dim3(tiles_of(NR), RW / 256, nres), dim3(256), 0, st, la);
        LAUNCH_CHECK("k_linear_fwd<qkvg>");
        hipLaunchKernelGGL((k_attr<false>), dim3(B, nres), dim3(256), attr_smem(T, at.H, RDm, false), st, at);
        LAUNCH_CHECK("k_attr<fwd>");
        if (with_reg_shape(kD, RDm, [&](auto d, auto dm) {
                return launch_post_fwd<false, decltype(dm)::value, decltype(d)::value>(c.reg_dff, dim3(tiles_of(NR), nres), st, po);
            }))
            return -1;
        LAUNCH_CHECK("k_post_fwd<reg>");
    }
    return 0;
}
// the prediction head as a launch of its own (save = 2: left to cf_backward_part, or riding in the Regulation launch)
static int head_fwd(cf_handle* h, int B, float* logits, int save, hipStream_t st, const HeadRide* ride) {
    const cf_config& c = h->cfg;
    h->head_deferred = save == 2 && !ride;
    h->head_done = ride != nullptr;
    h->deferred_logits_user = logits;
    if (save == 2) return 0;      // (together with the loss and its backward in cf_backward_part, one launch)
    if (c.d_head != 128 || c.d_emb != 128) {
        HeadGenArgs a;
        head_gen_args(h, B, logits, a);
        hipLaunchKernelGGL(k_head_gen_fwd, dim3(B), dim3(256), 0, st, a);
        LAUNCH_CHECK("k_head_gen_fwd");
    } else {
        HeadFwdArgs a;
        head_fwd_args(h, B, logits, a);
        hipLaunchKernelGGL(k_head_fwd, dim3(tiles_of(B)), dim3(kHeadThreads), 0, st, a);
        LAUNCH_CHECK("k_head_fwd");
    }
    return 0;
}
static int forward_reg_head(cf_handle* h, const cf_batch* bt, float* logits, int save, hipStream_t st, const HeadRide* ride) {
    if (h->reg_fused ? reg_fwd_fused(h, bt, save, st, ride) : reg_fwd_layers(h, bt, save, st)) return -1;
    return head_fwd(h, bt->B, logits, save, st, ride);
}
static int forward_impl(cf_handle* h, const cf_batch* bt, float* logits, int save, void* stream, const HeadRide* ride) {
    if (check_batch(h, bt)) return -1;
    hipStream_t st = (hipStream_t)stream;
    const long long launches0 = g_launches;
    if (forward_trunk(h, bt, save, st) || forward_reg_head(h, bt, logits, save, st, ride)) return -1;
    h->x0_fwd = false;
    h->last_fwd_B = save ? bt->B : 0;
    h->n_fwd = (int)(g_launches - launches0);
    if (h->capturing) h->cap.n_fwd = h->n_fwd;
    return 0;
}

// The head ride's per-gene arrival counters are monotonic (cf_head_ride.h): every launch adds n_res to each, and 2^32 is no multiple of 3 -- after
// 1.4e9 launches (eight days of uninterrupted steps) the winner test would drift.  Every 2^28 launches the counters are put back to zero by a
// stream-ordered memset IN FRONT of a launch: between two launches of a stream every counter is a multiple of n_res and nobody is arriving (zeroing
// from inside the launch, round 4, raced with the arrivals of a second process on the device).
// The launches of a handle may come in on more than one stream (two Trainers on one model, a caller's own stream): the reset waits for what the
// OTHER streams have queued so far and they wait for the reset, so it can never land under a ride launch in flight elsewhere.
static int ride_tick(cf_handle* h, hipStream_t st) {
    if (h->capturing) return 0;      // (a captured launch is counted when its graph is replayed: cf_graph_launch)
    if (std::find(h->ride_streams.begin(), h->ride_streams.end(), st) == h->ride_streams.end()) {
        if (h->ride_streams.size() >= 16) h->ride_streams.erase(h->ride_streams.begin());
        h->ride_streams.push_back(st);
    }
    if (++h->ride_launches >= h->ride_reset_every) {      // (CF_RIDE_RESET_EVERY at cf_create: the tests run with a handful)
        if (h->ride_streams.size() > 1) {
            if (!h->ride_ev) HIP_TRY(hipEventCreateWithFlags(&h->ride_ev, hipEventDisableTiming));
            for (size_t i = 0; i < h->ride_streams.size();) {
                hipStream_t o = h->ride_streams[i];
                if (o != st) {
                    if (hipEventRecord(h->ride_ev, o) != hipSuccess) {      // a stream its owner has destroyed since: nothing of it can be in flight
                        (void)hipGetLastError();
                        h->ride_streams.erase(h->ride_streams.begin() + i);
                        continue;
                    }
                    HIP_TRY(hipStreamWaitEvent(st, h->ride_ev, 0));
                }
                ++i;
            }
        }
        HIP_TRY(hipMemsetAsync(h->head_cnt, 0, (size_t)(h->cfg.max_batch + 1) * sizeof(int), st));
        if (h->ride_streams.size() > 1) {
            HIP_TRY(hipEventRecord(h->ride_ev, st));
            for (hipStream_t o : h->ride_streams)
                if (o != st) HIP_TRY(hipStreamWaitEvent(o, h->ride_ev, 0));
        }
        h->ride_launches = 0;
    }
    return 0;
}
// the head's ride at the tail of the Regulation forward launch (cf_forward_train, cf_forward_train_x0)
static void head_ride_args(cf_handle* h, float* logits, const void* labels, float loss_scale, float* loss_out, HeadRide& hd) {
    const cf_config& c = h->cfg;
    memset(&hd, 0, sizeof hd);
    hd.on = 1;
    hd.n_out = c.n_out;
    hd.gscale = loss_scale;
    hd.labels = labels;
    hd.w1_t = h->tiled_of(h->refs.head.w1);
    hd.w1 = h->refs.head.w1;
    hd.b1 = h->refs.head.b1;
    hd.w2 = h->refs.head.w2;
    hd.b2 = h->refs.head.b2;
    hd.hin = h->hin, hd.h1 = h->h1, hd.logits = h->logits, hd.logits_user = logits, hd.dlogits = h->dlogits, hd.dh1 = h->dh1, hd.dhin = h->dhin;
    for (int r = 0; r < c.n_res; ++r) hd.dxl[r] = h->dRx[r][c.reg_layers];
    hd.loss = h->loss, hd.loss_part = h->loss_part, hd.loss_user = loss_out;
    hd.cnt = h->head_cnt;
}
