// cf_api_bwd.h -- the backward pass (head, Regulation stack, trunk; fused / layer by layer) and the deferred gradient reductions.
// Part of cf_api.hip's single translation unit: included there behind cf_api_fwd.h, not on its own.
#pragma once

// loss + head backward as launches of their own (with the head's forward where cf_forward(save = 2) left it to this call)
static int head_bwd(cf_handle* h, int B, hipStream_t st, const void* labels, float loss_scale, float* loss_out) {
    const cf_config& c = h->cfg;
    if (h->head_deferred && !labels) return fail("cf_backward: cf_forward(save_for_backward = 2) needs the fused loss (labels)");
    if (c.d_head != 128 || c.d_emb != 128) {      // any hidden width / row width
        HeadGenArgs a;
        head_gen_args(h, B, h->head_deferred ? h->deferred_logits_user : nullptr, a);
        a.labels = labels;
        a.loss_user = loss_out;
        a.gscale = loss_scale;
        if (h->head_deferred) {
            hipLaunchKernelGGL(k_head_gen_fwd, dim3(B), dim3(256), 0, st, a);
            LAUNCH_CHECK("k_head_gen_fwd");
            h->head_deferred = false;
        }
        hipLaunchKernelGGL(k_head_gen_bwd, dim3(B), dim3(256), 0, st, a);
        LAUNCH_CHECK("k_head_gen_bwd");
        return 0;
    }
    HeadBwdArgs a;
    a.logits = h->logits;
    a.labels = labels;
    a.w2 = h->refs.head.w2;
    a.h1 = h->h1;
    a.w1 = h->refs.head.w1;
    a.dlogits = h->dlogits;
    a.dh1 = h->dh1;
    a.dhin = h->dhin;
    for (int r = 0; r < c.n_res; ++r) a.dxl[r] = h->dRx[r][c.reg_layers];
    a.loss = h->loss;
    a.loss_part = h->loss_part;
    a.loss_user = loss_out;
    a.gscale = loss_scale;
    a.B = B;
    a.T = c.i_max + 1;
    a.n_res = c.n_res;
    a.n_out = c.n_out;
    a.tdbg = getenv("CF_STAMP_HEAD") ? reinterpret_cast<unsigned long long*>(h->tdbg) + 128 : nullptr;
    if (h->head_deferred) {      // the forward pass left the head to this call: forward, loss, backward in one launch
        HeadFwdArgs f;
        head_fwd_args(h, B, h->deferred_logits_user, f);
        hipLaunchKernelGGL(k_head_train, dim3(tiles_of(B)), dim3(kHeadThreads), 0, st, f, a);
        LAUNCH_CHECK("k_head_train");
        h->head_deferred = false;
    } else {
        hipLaunchKernelGGL(k_head_bwd, dim3(tiles_of(B)), dim3(kHeadThreads), 0, st, a);
        LAUNCH_CHECK("k_head_bwd");
    }
    return 0;
}
// Regulation backward on the fused kernel: the whole stack (parts & 2) or one of its halves (CF_PART_REG_HI / _LO, cf_reg_halves)
static int reg_bwd_fused(cf_handle* h, const cf_batch* bt, hipStream_t st, int parts, float* loss_out, const PassOpts& opts) {
    const cf_config& c = h->cfg;
    const int half = c.reg_layers / 2;
    const dim3 grid(8 * ((bt->B * c.n_res + 7) / 8));
    RegArgs ra;
    reg_args(h, bt, ra);
    ra.l_top = (parts & 2) || (parts & CF_PART_REG_HI) ? c.reg_layers - 1 : half - 1;
    ra.l_bot = (parts & 2) || (parts & CF_PART_REG_LO) ? 0 : half;
    ra.save = 1;
    ra.tdbg = getenv("CF_STAMP_BWD") ? reinterpret_cast<unsigned long long*>(h->tdbg) : nullptr;
    if (h->head_loss_due) {
        ra.head = h->ride;
        if (loss_out) ra.head.loss_user = loss_out;
        h->head_loss_due = false;
    }
    if (!opts.dfreq) return launch_reg(h, "k_reg_bwd", reg_kernel(true, c.reg_dff), grid, reg8_bwd_smem(c.reg_dff), ra, st);
    // cf_backward_from_inputs: the variant that also leaves d(interaction_freq) per resolution
    if (!h->reg_dfreq_ok) return fail("cf_backward_from_inputs: interaction_freq: the fused Regulation backward variant could not be configured");
    ra.dfreq = opts.dfreq;
    void* kargs[] = {&ra};
    HIP_TRY(hipLaunchKernel(reg_kernel_dfreq(c.reg_dff), grid, dim3(512), kargs, reg8_bwd_smem(c.reg_dff), st));
    LAUNCH_CHECK("k_reg_bwd_dfreq");
    return 0;
}
// what a post chain's backward reads and writes: CentreParams / RegParams and CentreBuf / RegBuf name it alike
template <class Params, class Buf>
static void post_bwd_common(PostBwdArgs& pb, int r, const Params& p, const Buf& b) {
    pb.xh2[r] = b.xh2, pb.rs2[r] = b.rs2, pb.g2[r] = p.g2, pb.hdn[r] = b.hdn, pb.w2[r] = p.w2, pb.w1[r] = p.w1;
    pb.xh1[r] = b.xh1, pb.rs1[r] = b.rs1, pb.g1[r] = p.g1, pb.wo[r] = p.wo;
    pb.dt2[r] = b.dt2, pb.dpre1[r] = b.dpre1, pb.dt1[r] = b.dt1, pb.da[r] = b.da, pb.partial[r] = b.partial;
}
static void reg_bwd_args(const cf_handle* h, const cf_batch* bt, int l, float* dfreq, PostBwdArgs& pb, AttrArgs& at, DgradArgs& dg) {
    const cf_config& c = h->cfg;
    const int kD = c.d_emb, NR = bt->B * (c.i_max + 1), RW = 4 * c.reg_dmodel;
    reg_attr_args(h, bt, l, at);
    for (int r = 0; r < c.n_res; ++r) {
        const RegParams& p = h->refs.R[r][l];
        const RegBuf& b = h->R[r][l];
        post_bwd_common(pb, r, p, b);
        pb.dout[r] = h->dRx[r][l + 1], pb.wv[r] = nullptr, pb.dxbar[r] = nullptr;
        at.a[r] = b.da, at.dqkvg[r] = b.dqkvg, at.dgam[r] = b.dgam;
        dg.dy[r] = b.dqkvg, dg.w[r] = p.watt, dg.res[r] = b.dt1, dg.dx[r] = h->dRx[r][l];
    }
    pb.dmap = dg.rmap = identity_map();
    pb.N = dg.N = NR;
    at.dfreq = dfreq;
    at.dfreq_add = l + 1 < c.reg_layers;      // (the top layer's launch comes first: it writes, the ones below add)
    dg.lddy = dg.K = RW, dg.ldw = dg.ldres = dg.lddx = dg.Ncols = kD;
}
// Regulation backward layer by layer on the stand-alone kernels
static int reg_bwd_layers(cf_handle* h, const cf_batch* bt, hipStream_t st, const PassOpts& opts) {
    const cf_config& c = h->cfg;
    const int kD = c.d_emb, B = bt->B, T = c.i_max + 1, nres = c.n_res, NR = B * T, RDm = c.reg_dmodel;
    for (int l = c.reg_layers - 1; l >= 0; --l) {
        PostBwdArgs pb;
        AttrArgs at;
        DgradArgs dg;
        reg_bwd_args(h, bt, l, opts.dfreq, pb, at, dg);
        if (with_reg_shape(kD, RDm, [&](auto d, auto dm) {
                return launch_post_bwd<false, decltype(dm)::value, decltype(d)::value>(c.reg_dff, dim3(tiles_of(NR), nres), st, pb);
            }))
            return -1;
        LAUNCH_CHECK("k_post_bwd<reg>");
        if (at.dfreq) hipLaunchKernelGGL((k_attr<true, true>), dim3(B, nres), dim3(256), attr_smem(T, at.H, RDm, true), st, at);
        else hipLaunchKernelGGL((k_attr<true>), dim3(B, nres), dim3(256), attr_smem(T, at.H, RDm, true), st, at);
        LAUNCH_CHECK("k_attr<bwd>");
        if (RDm == 128) hipLaunchKernelGGL((k_dgrad<8>), dim3(tiles_of(NR), kD / 32, nres), dim3(256), 0, st, dg);
        else hipLaunchKernelGGL((k_dgrad<16>), dim3(tiles_of(NR), kD / 32, nres), dim3(256), 0, st, dg);
        LAUNCH_CHECK("k_dgrad<qkvg>");
    }
    return 0;
}
// Pairwise + Embedding backward, the join and the 7-mark projection partials: one launch (cf_trunk.h)
static int trunk_bwd_fused(cf_handle* h, const cf_batch* bt, hipStream_t st) {
    const cf_config& c = h->cfg;
    const int B = bt->B;
    TrunkArgs ta;
    trunk_args(h, bt, ta, 1);
    if (h->pend_record) {
        ta.rec = h->pend_rec;
        h->pend_record = false;
    }
    ta.lp_jobs = h->lp_jobs;
    ta.rd_tiles = nullptr;
    ta.rd_n = 0;
    ta.rd_batch = B;
    memset(&ta.rd_opt, 0, sizeof ta.rd_opt);
    const bool riding = h->rider.armed;
    if (riding) {      // (cf_rider_arm) one tile per rider wave at a time: any leading part of the bucket's table
        if (h->capturing) return fail("cf_backward_part: armed riders carry this step's AdamW scalars as launch arguments and cannot be captured");
        ta.rd_n = std::min(h->rider.max_tiles, h->n_wg_r - h->n_wg_short);
        ta.rd_tiles = h->wg_tiles + h->n_wg_short;
        ta.rd_opt = h->rider.o;
    }
    void* kargs[] = {&ta};
    const size_t rider_lds = (size_t)(kAT / 64) * kWgWaveLds * sizeof(float);      // eight wave-private stages
    // one tile per rider wave: rows of B workgroups x 8 waves until every tile has a wave.  The first (CUs - 3 B) workgroups start at once on
    // the idle CUs, the others as the short-resolution workgroups of the trunk (dispatched last, done first) leave theirs
    const int rider_rows = ta.rd_n > 0 ? (ta.rd_n + B * (kAT / 64) - 1) / (B * (kAT / 64)) : 0;
    h->time_mark("k_trunk_bwd", st);
    const hipError_t le = hipLaunchKernel(trunk_kernel(true, c.embed_dff, c.pair_dff, c.pair_layers), dim3(B, c.n_res + rider_rows), dim3(kAT), kargs,
                                          ta.rd_n > 0 ? std::max(h->trunk_smem_bytes, rider_lds) : h->trunk_smem_bytes, st);
    h->time_mark("k_trunk_bwd", st);
    ++g_launches;
    if (le != hipSuccess || hipGetLastError() != hipSuccess) {
        // nothing was reduced or stepped: the riders stay armed for a retry, rider.done stays 0 and the reduction launch of the
        // step covers every tile
        return fail("launch k_trunk_bwd failed: %s", hipGetErrorString(le));
    }
    if (riding) {      // only a launch that was accepted counts as having reduced (and stepped) its tiles
        h->rider.armed = false;
        h->rider.done = ta.rd_n;
    }
    return 0;
}
// one centre-row layer backward: post chain -> attention -> query chain
static int centre_bwd(cf_handle* h, const CentreStage& s, int B, int ag_genes, hipStream_t st) {
    const cf_config& c = h->cfg;
    const int kD = c.d_emb, nres = c.n_res, N = s.N;      // (kD: row width, shadows cf::kD)
    PostBwdArgs pb;
    AttcArgs at;
    QBwdArgs qb;
    const size_t smem = centre_attc_args(h, s, true, at);
    for (int r = 0; r < nres; ++r) {
        const CentreBuf& b = *s.buf[r];
        const CentreParams& p = *s.prm[r];
        post_bwd_common(pb, r, p, b);
        pb.dout[r] = s.dout[r], pb.wv[r] = p.wv, pb.dxbar[r] = b.dxbar;
        at.vin[r] = b.dxbar, at.w[r] = b.du, at.vout[r] = b.dqt;
        qb.dqt[r] = b.dqt, qb.dres[r] = b.dt1, qb.dq[r] = b.dq, qb.dx[r] = b.dx;
        qb.wk[r] = p.wk_t, qb.wq[r] = p.wq;      // NT product in the backward: tiled copy
    }
    pb.dmap = s.dmap;
    pb.N = qb.N = N;
    if (kD != 128 || s.nh != 2)      // every shape but the default: the stand-alone kernels instantiated for it
        return with_centre_shape(kD, s.nh, [&](auto d, auto nh) {
            return centre_bwd_heads<decltype(nh)::value, decltype(d)::value>(st, N, nres, s.dff, pb, at, smem, qb);
        });
    if (launch_post_bwd<true, 128>(s.dff, dim3(tiles_of(N), nres), st, pb)) return -1;
    LAUNCH_CHECK("k_post_bwd<centre>");
    if (launch_attc<true>(h, at, N, B, smem, ag_genes, st)) return -1;
    hipLaunchKernelGGL((k_qchain_bwd<kPostWaves>), dim3(tiles_of(N), nres), dim3(kPostWaves * 64), 0, st, qb);
    LAUNCH_CHECK("k_qchain_bwd");
    return 0;
}
// Pairwise + Embedding backward on the stand-alone kernels, layer by layer
static int trunk_bwd_layers(cf_handle* h, const cf_batch* bt, hipStream_t st, const PassOpts& opts) {
    const cf_config& c = h->cfg;
    const int kD = c.d_emb;      // (row width: shadows cf::kD in this function)
    const int B = bt->B, S = c.i_max, T = S + 1, nres = c.n_res;
    for (int l = c.pair_layers - 1; l >= 0; --l) {   // Pairwise
        const bool last = l + 1 == c.pair_layers;
        CentreStage s = centre_stage(h, bt, l);
        for (int r = 0; r < nres; ++r) s.dout[r] = last ? h->dRx[r][0] : h->P[r][l + 1].dx;
        s.dmap = last ? RowMap{S, T, 1, 1} : identity_map();
        if (centre_bwd(h, s, B, opts.ag_genes, st)) return -1;
    }
    {   // join the streams meeting at the promoter embedding, back through lin_proj_p: one launch
        JoinDgradArgs a;
        for (int r = 0; r < nres; ++r) {
            a.dxp[r] = h->P[r][0].dx;
            a.dx0[r] = h->dRx[r][0];
            a.w[r] = h->refs.lin_proj_p[r];
            a.dxp0[r] = h->dxp0[r];
            a.dx[r] = h->edout[r];
        }
        a.dhin = h->dhin;
        a.B = B;
        a.S = S;
        a.T = T;
        a.n_res = nres;
        if (with_int<64, 128, 256>("d_emb", kD, [&](auto d) {
                hipLaunchKernelGGL(k_join_dgrad<decltype(d)::value>, dim3(tiles_of(B), kD / 32, nres), dim3(256), 0, st, a);
                return 0;
            }))
            return -1;
        LAUNCH_CHECK("k_join_dgrad");
    }
    if (h->embed_dense) {
        if (!opts.no_dense_embed_bwd && embed_dense_backward(h, bt, st)) return -1;      // writes the Embedding gradients directly (no deferred tiles)
    } else {   // Embedding
        CentreStage s = centre_stage(h, bt, -1);
        for (int r = 0; r < nres; ++r) s.dout[r] = h->edout[r];
        s.dmap = identity_map();
        if (centre_bwd(h, s, B, opts.ag_genes, st)) return -1;
    }
    return 0;
}
// parts: 1 = head, 2 = Regulation stack, 4 = Pairwise + Embedding (the activation-gradient chain in order)
static int backward_impl(cf_handle* h, const cf_batch* bt, hipStream_t st, int parts = 7, const void* labels = nullptr,
                         float loss_scale = 1.f, float* loss_out = nullptr, const PassOpts& opts = PassOpts()) {
    if ((parts & 1) && h->head_done) {         // cf_forward_train has run head forward, loss and head backward already
        h->head_done = false;
        h->head_loss_due = true;
        parts &= ~1;
    }
    if ((parts & 1) && head_bwd(h, bt->B, st, labels, loss_scale, loss_out)) return -1;
    if ((parts & (CF_PART_REG_HI | CF_PART_REG_LO)) && !(parts & 2)) {      // the Regulation backward in halves (data-parallel schedule, cf_reg_halves)
        if (!cf_reg_halves(h)) return fail("cf_backward_part: this model's Regulation backward does not come in halves (cf_reg_halves)");
        if ((parts & (CF_PART_REG_HI | CF_PART_REG_LO)) == (CF_PART_REG_HI | CF_PART_REG_LO)) parts |= 2;
    }
    if (h->reg_fused) {
        if ((parts & (2 | CF_PART_REG_HI | CF_PART_REG_LO)) && reg_bwd_fused(h, bt, st, parts, loss_out, opts)) return -1;
    } else if ((parts & 2) && reg_bwd_layers(h, bt, st, opts)) return -1;
    if (!(parts & 4)) return 0;
    if (h->trunk) return trunk_bwd_fused(h, bt, st);
    if (h->pend_record) {      // (cf_record_step_bwd without the fused trunk: a launch of its own, here)
        hipLaunchKernelGGL(k_record_step, dim3(1), dim3(256), 0, st, h->pend_rec);
        LAUNCH_CHECK("k_record_step");
        h->pend_record = false;
    }
    return trunk_bwd_layers(h, bt, st, opts);
}

#ifndef CF_MERGE_REDUCE
#define CF_MERGE_REDUCE 1
#endif
constexpr bool kMergeReduce = CF_MERGE_REDUCE;
// deferred weight / bias gradients: one launch per bucket over the two tile tables
static int reduce_impl(cf_handle* h, int B, hipStream_t st, int buckets = CF_BUCKET_REG | CF_BUCKET_PE) {
    if (h->rider.done) return fail("gradient reduction: the riders of step %lld have updated part of the Regulation + head bucket; finish the step with cf_reduce_opt_part", h->rider.step);
    if ((buckets & CF_BUCKET_PE) && !h->trunk) {      // (the fused trunk backward writes these partials itself)
        hipLaunchKernelGGL(k_wgrad_lp, dim3((B + kLpGenes - 1) / kLpGenes, h->n_lp), dim3(256), 0, st, (const LpJob*)h->lp_jobs, B, h->cfg.d_emb);
        LAUNCH_CHECK("k_wgrad_lp");
    }
    if (buckets & CF_BUCKET_REG) buckets |= CF_BUCKET_REG_HI | CF_BUCKET_REG_LO;
    if ((buckets & (CF_BUCKET_REG_HI | CF_BUCKET_REG_LO)) == (CF_BUCKET_REG_HI | CF_BUCKET_REG_LO)) buckets |= CF_BUCKET_REG;
    for (int bk = 0; bk < 4; ++bk) {      // the whole Regulation + head bucket (one launch), else its halves; Embedding + Pairwise
        int w0, wn, c0, cn;
        if (bk == 0) {
            if (!(buckets & CF_BUCKET_REG)) continue;
            w0 = 0, wn = h->n_wg_r, c0 = 0, cn = h->n_cs_r;
        } else if (bk == 1) {
            if ((buckets & CF_BUCKET_REG) || !(buckets & CF_BUCKET_REG_HI)) continue;
            w0 = 0, wn = h->n_wg_hi, c0 = 0, cn = h->n_cs_hi;
        } else if (bk == 2) {
            if ((buckets & CF_BUCKET_REG) || !(buckets & CF_BUCKET_REG_LO)) continue;
            w0 = h->n_wg_hi, wn = h->n_wg_r - h->n_wg_hi, c0 = h->n_cs_hi, cn = h->n_cs_r - h->n_cs_hi;
        } else {
            if (!(buckets & CF_BUCKET_PE)) continue;
            w0 = h->n_wg_r, wn = h->n_wg - h->n_wg_r, c0 = h->n_cs_r, cn = h->n_cs - h->n_cs_r;
        }
        if (!kMergeReduce || h->timed == "k_wgrad" || h->timed == "k_colsum") {      // timed separately
            h->time_mark("k_wgrad", st);
            hipLaunchKernelGGL(k_wgrad, dim3(xcd_grid(wn)), dim3(256), 0, st, (const WgTile*)h->wg_tiles + w0, wn, B, h->xcd_reduce);
            h->time_mark("k_wgrad", st);
            LAUNCH_CHECK("k_wgrad");
            h->time_mark("k_colsum", st);
            hipLaunchKernelGGL(k_colsum, dim3(cn), dim3(256), 0, st, (const CsTile*)h->cs_tiles + c0, B);
            h->time_mark("k_colsum", st);
        } else {
            hipLaunchKernelGGL(k_reduce, dim3(xcd_grid(wn) + cn), dim3(256), 0, st, (const WgTile*)h->wg_tiles + w0, wn, (const CsTile*)h->cs_tiles + c0, B, h->xcd_reduce);
        }
        LAUNCH_CHECK("k_colsum");
    }
    return 0;
}

// `first`: the call starts a backward pass (later pieces may follow a replayed graph, which bypasses the host-side record)
static int check_bwd(cf_handle* h, const cf_batch* bt, bool first = true) {
    if (h && h->x0_fwd ? check_batch_x0(h, bt, "cf_backward") : check_batch(h, bt)) return -1;
    if (!h->grads) return fail("cf_backward: no gradient buffer bound");
    if (first && h->last_fwd_B != bt->B) return fail("cf_backward must follow cf_forward(save_for_backward=1) on the same batch");
    return 0;
}
