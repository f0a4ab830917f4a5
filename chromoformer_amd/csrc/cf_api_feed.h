// cf_api_feed.h -- batch checks, the pre-gathered feed (batch gather, step log) and the trunk-output cache (x0 store).
// Part of cf_api.hip's single translation unit: included there in front of the forward pass, not on its own.
#pragma once

// ------------------------------------------------------------------------------------
// batch checks
// ------------------------------------------------------------------------------------
static int check_batch(const cf_handle* h, const cf_batch* b) {
    if (!h || !b) return fail("null handle / batch");
    if (!h->params) return fail("cf_bind has not been called");
    if (b->B < 1 || b->B > h->cfg.max_batch) return fail("batch size %d outside 1..max_batch=%d", b->B, h->cfg.max_batch);
    for (int r = 0; r < h->cfg.n_res; ++r)
        if (!b->promoter_feats[r] || !b->pcre_feats[r] || !b->promoter_mask_row[r] || !b->pcre_mask_row[r] || !b->interaction_mask[r])
            return fail("batch pointer for resolution %d is null", r);
    if (!b->interaction_freq) return fail("interaction_freq is null");
    return 0;
}
static int check_batch_x0(const cf_handle* h, const cf_batch* b, const char* who) {
    if (!h || !b) return fail("%s: null handle / batch", who);
    if (!h->params) return fail("%s: cf_bind has not been called", who);
    if (b->B < 1 || b->B > h->cfg.max_batch) return fail("%s: batch size %d outside 1..max_batch=%d", who, b->B, h->cfg.max_batch);
    for (int r = 0; r < h->cfg.n_res; ++r)
        if (!b->interaction_mask[r]) return fail("%s: interaction_mask of resolution %d is null", who, r);
    if (!b->interaction_freq) return fail("%s: interaction_freq is null", who);
    return 0;
}

// ------------------------------------------------------------------------------------
// frozen trunk: the trunk-output cache and its gather (cf_x0_gather.h)
// ------------------------------------------------------------------------------------
static int x0_copy(cf_handle* h, int B, const float* const* src, float* const* dst, hipStream_t st) {
    X0CopyArgs a;
    memset(&a, 0, sizeof a);
    for (int r = 0; r < h->cfg.n_res; ++r) {
        a.src[r] = reinterpret_cast<const float4*>(src[r]);
        a.dst[r] = reinterpret_cast<float4*>(dst[r]);
    }
    a.n4 = (long long)B * (h->cfg.i_max + 1) * h->cfg.d_emb / 4;      // (d_emb is a multiple of 4: check_config)
    hipLaunchKernelGGL(k_x0_copy, dim3((int)std::min<long long>((a.n4 + kX0Threads - 1) / kX0Threads, 256), h->cfg.n_res), dim3(kX0Threads), 0, st, a);
    LAUNCH_CHECK("k_x0_copy");
    return 0;
}
static int x0_gather_args(cf_handle* h, const cf_x0_store* cs, const int* order, int* cursor, const cf_batch* dst, void* labels_dst, X0GatherArgs& ga) {
    if (!h || !cs || !order || !cursor || !dst) return fail("cf_x0_gather: null argument");
    const cf_config& c = h->cfg;
    const long long T = c.i_max + 1;
    if (dst->B < 1 || dst->B > c.max_batch) return fail("cf_x0_gather: B = %d outside [1, max_batch = %d]", dst->B, c.max_batch);
    memset(&ga, 0, sizeof ga);
    int n = 0;
    for (int r = 0; r < c.n_res; ++r) {
        if (!cs->x0[r] || !cs->interaction_mask[r] || !dst->interaction_mask[r]) return fail("cf_x0_gather: null array at resolution %d", r);
        ga.seg[n++] = X0Seg{(const char*)cs->x0[r], (char*)h->Rx[r][0], T * c.d_emb * 4};
        ga.seg[n++] = X0Seg{(const char*)cs->interaction_mask[r], (char*)const_cast<uint8_t*>(dst->interaction_mask[r]), T * T};
    }
    if (!cs->interaction_freq || !dst->interaction_freq) return fail("cf_x0_gather: interaction_freq is null");
    ga.seg[n++] = X0Seg{(const char*)cs->interaction_freq, (char*)const_cast<float*>(dst->interaction_freq), T * T * 4};
    if (labels_dst) {
        if (!cs->labels) return fail("cf_x0_gather: the cache holds no labels");
        ga.seg[n++] = X0Seg{(const char*)cs->labels, (char*)labels_dst, c.n_out == 1 ? 4 : 8};
    }
    ga.n_seg = n;
    ga.order = order;
    ga.cursor = cursor;
    ga.n_genes = cs->n_genes;
    ga.B = dst->B;
    return 0;
}
extern "C" int cf_x0_gather(cf_handle* h, const cf_x0_store* cs, const int* order, int* cursor, const cf_batch* dst, void* labels_dst, void* stream) {
    X0GatherArgs ga;
    if (x0_gather_args(h, cs, order, cursor, dst, labels_dst, ga)) return -1;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_x0_gather, dim3(ga.B, ga.n_seg), dim3(kX0Threads), 0, st, ga);
    LAUNCH_CHECK("k_x0_gather");
    hipLaunchKernelGGL(k_gather_advance, dim3(1), dim3(1), 0, st, cursor);
    LAUNCH_CHECK("k_gather_advance");
    return 0;
}
extern "C" int cf_x0_gather_fwd(cf_handle* h, const cf_x0_store* cs, const int* order, int* cursor, const cf_batch* dst, void* labels_dst, void* stream) {
    (void)stream;
    if (x0_gather_args(h, cs, order, cursor, dst, labels_dst, h->pend_x0_ga)) return -1;
    h->pend_x0 = true;
    return 0;
}

// ------------------------------------------------------------------------------------
// resident split: batch gather / step log inside the graph
// ------------------------------------------------------------------------------------
static int gather_args(cf_handle* h, const cf_store* st_, const int* order, int* cursor, const cf_batch* dst, void* labels_dst, GatherArgs& ga, int& n) {
    if (!h || !st_ || !order || !cursor || !dst) return fail("cf_gather_batch: null argument");
    const cf_config& c = h->cfg;
    const int B = dst->B, S = c.i_max, T = S + 1, F = c.n_feats;
    if (B < 1 || B > c.max_batch) return fail("cf_gather_batch: B = %d outside [1, max_batch = %d]", B, c.max_batch);
    memset(&ga, 0, sizeof ga);
    n = 0;
    bool overflow = false;
    auto push = [&](const void* src, const void* d, long long gene_bytes) {
        const int chunk = kGatherChunk;
        for (long long off = 0; off < gene_bytes; off += chunk) {
            if (n >= kGatherMaxSeg) {
                overflow = true;
                return;
            }
            ga.seg[n++] = GatherSeg{(const char*)src, (char*)const_cast<void*>(d), (int)gene_bytes, (int)off, (int)std::min<long long>(chunk, gene_bytes - off), 0};
        }
    };
    for (int r = 0; r < c.n_res; ++r) {
        const long long L = c.n_bins[r];
        if (dst->promoter_mask_stride[r] != L || dst->pcre_mask_stride[r] != L)
            return fail("cf_gather_batch: the destination batch must use compact mask rows (stride = n_bins)");
        push(st_->promoter_feats[r], dst->promoter_feats[r], L * F * 4);
        push(st_->pcre_feats[r], dst->pcre_feats[r], (long long)S * L * F * 4);
        push(st_->promoter_mask[r], dst->promoter_mask_row[r], L);
        push(st_->pcre_mask[r], dst->pcre_mask_row[r], (long long)S * L);
        push(st_->interaction_mask, dst->interaction_mask[r], (long long)T * T);
    }
    push(st_->interaction_freq, dst->interaction_freq, (long long)T * T * 4);
    if (labels_dst) push(st_->labels, labels_dst, c.n_out == 1 ? 4 : 8);
    if (overflow) return fail("cf_gather_batch: segment table overflow");
    ga.order = order;
    ga.cursor = cursor;
    ga.n_genes = st_->n_genes;
    ga.B = B;
    return 0;
}
static int gather_launch(const GatherArgs& ga, int n, hipStream_t st) {
    hipLaunchKernelGGL(k_gather_batch, dim3(ga.B, n), dim3(256), 0, st, ga);
    LAUNCH_CHECK("k_gather_batch");
    hipLaunchKernelGGL(k_gather_advance, dim3(1), dim3(1), 0, st, ga.cursor);
    LAUNCH_CHECK("k_gather_advance");
    return 0;
}
extern "C" int cf_gather_batch(cf_handle* h, const cf_store* st_, const int* order, int* cursor, const cf_batch* dst, void* labels_dst,
                               void* stream) {
    GatherArgs ga;
    int n;
    if (gather_args(h, st_, order, cursor, dst, labels_dst, ga, n)) return -1;
    return gather_launch(ga, n, (hipStream_t)stream);
}
// cf_gather_batch for the batch of a TRAINING step: nothing is launched here; the cf_forward / cf_forward_train that must follow on
// the same stream (same batch buffers) copies the genes in the launch that refreshes its tiled weight copies -- the two do not depend
// on each other -- and advances the cursor.  Three launches in front of every step of the training loop become one.
extern "C" int cf_gather_batch_fwd(cf_handle* h, const cf_store* st_, const int* order, int* cursor, const cf_batch* dst, void* labels_dst,
                                   void* stream) {
    (void)stream;
    int n;
    if (gather_args(h, st_, order, cursor, dst, labels_dst, h->pend_ga, n)) return -1;
    h->pend_ga_n = n;
    h->pend_gather = true;
    h->pend_key = dst->promoter_feats[0];
    return 0;
}

// The batch of the NEXT step, gathered while this step ends: nothing is launched here; the cf_reduce_opt_part that follows on the same stream
// carries the copy blocks behind its tiles (nothing in that launch reads the batch buffers, and every kernel of this step that does has
// finished), and the cursor -- which the gather reads, so it cannot move in the same launch -- is advanced by the trunk's forward launch
// of the next cf_forward / cf_forward_train.  A step of the training loop then has no launch in front of it.  cf_gather_batch_only is the
// same for the first step of an epoch: the copy as a launch of its own, now, the cursor left to the forward pass that follows.
extern "C" int cf_gather_batch_next(cf_handle* h, const cf_store* st_, const int* order, int* cursor, const cf_batch* dst, void* labels_dst,
                                    void* stream) {
    (void)stream;
    int n;
    if (gather_args(h, st_, order, cursor, dst, labels_dst, h->pend_gn, n)) return -1;
    h->pend_gn_n = n;
    h->pend_gnext = true;
    h->pend_key = dst->promoter_feats[0];
    return 0;
}
extern "C" int cf_gather_batch_only(cf_handle* h, const cf_store* st_, const int* order, int* cursor, const cf_batch* dst, void* labels_dst,
                                    void* stream) {
    GatherArgs ga;
    int n;
    if (gather_args(h, st_, order, cursor, dst, labels_dst, ga, n)) return -1;
    hipLaunchKernelGGL(k_gather_batch, dim3(ga.B, n), dim3(256), 0, (hipStream_t)stream, ga);
    LAUNCH_CHECK("k_gather_batch");
    h->adv_next = cursor;
    h->pend_key = dst->promoter_feats[0];
    return 0;
}

extern "C" int cf_record_step(cf_handle* h, const int* cursor, const float* logits, const void* labels, const float* loss, int B,
                              float* logits_log, void* labels_log, float* loss_log, void* stream) {
    if (!h || !cursor || !logits || !labels || !loss || !logits_log || !labels_log || !loss_log) return fail("cf_record_step: null argument");
    RecordArgs ra{cursor, logits, (const char*)labels, loss, logits_log, (char*)labels_log, loss_log, B, h->cfg.n_out, h->cfg.n_out == 1 ? 4 : 8};
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_record_step, dim3(1), dim3(256), 0, st, ra);
    LAUNCH_CHECK("k_record_step");
    return 0;
}
// cf_record_step without a launch of its own: the cf_backward_part(parts & 4) that must follow on the same stream writes the log rows at the
// start of the trunk's backward launch (the loss is final by then).  Configurations without the fused trunk kernels: that call issues
// k_record_step itself.
extern "C" int cf_record_step_bwd(cf_handle* h, const int* cursor, const float* logits, const void* labels, const float* loss, int B,
                                  float* logits_log, void* labels_log, float* loss_log, void* stream) {
    (void)stream;
    if (!h || !cursor || !logits || !labels || !loss || !logits_log || !labels_log || !loss_log) return fail("cf_record_step_bwd: null argument");
    h->pend_rec = RecordArgs{cursor, logits, (const char*)labels, loss, logits_log, (char*)labels_log, loss_log, B, h->cfg.n_out, h->cfg.n_out == 1 ? 4 : 8};
    h->pend_record = true;
    return 0;
}
