// cf_api_transplant.h -- host side of the pCRE transplant screen (cf_transplant.h): cf_pcre_transplant.  Part of cf_api.hip's single
// translation unit: included there behind cf_api_attrib.h, whose workspace (attrib_ws), stash, chunk description (chunk_rows) and chunk
// loop (chunk_forward) it uses; not on its own.
#pragma once

// The trunk once on the B genes and its output stashed.  Pack phase, per chunk of at most max_batch of the B * U pseudo rows
// (U = ceil(C / i_max)): k_transplant_pack, the trunk (k_attc2's regions per workgroup as for the caller's B genes), k_scan_unpack with
// V = C + 1 into slot_rows [n_res][B * C, d_emb].  Row phase, per chunk of at most max_batch of the B * (1 + C * Q) rows:
// k_transplant_rows, the Regulation + head launches of an inference forward.
extern "C" int cf_pcre_transplant(cf_handle* h, const cf_batch* bt, const cf_transplant_opts* o, float* logits, void* stream) {
    const char* who = "cf_pcre_transplant";
    if (attrib_open(h, bt, true, who)) return -1;
    if (!o) return fail("%s: null opts", who);
    if (!logits) return fail("%s: null logits", who);
    if (!o->freq) return fail("%s: null freq", who);
    const cf_config& c = h->cfg;
    const int nres = c.n_res, S = c.i_max, T = S + 1, cap = c.max_batch, d4 = c.d_emb / 4, B = bt->B;
    for (int r = 0; r < kMaxRes; ++r) {
        if (r < nres && (!o->lib_feats[r] || !o->lib_mask[r])) return fail("%s: null lib_feats / lib_mask[%d]", who, r);
        if (r >= nres && (o->lib_feats[r] || o->lib_mask[r])) return fail("%s: lib_feats / lib_mask[%d]: the model has %d resolutions", who, r, nres);
    }
    if (o->n_cand < 1) return fail("%s: n_cand = %d: at least 1 candidate", who, o->n_cand);
    if (o->n_freq < 1) return fail("%s: n_freq = %d: at least 1 frequency", who, o->n_freq);
    const long long rows = (long long)B * (1 + (long long)o->n_cand * o->n_freq);
    if (rows > 0x7fffffffLL) return fail("%s: B * (1 + n_cand * n_freq) = %lld rows do not fit an int", who, rows);
    if (o->slot_all < -1 || o->slot_all >= S) return fail("%s: slot_all = %d outside [-1, i_max = %d)", who, o->slot_all, S);
    const int C = o->n_cand, Q = o->n_freq, V = 1 + C * Q, U = (C + S - 1) / S;
    int rc = 0;      // the coarsest resolution: the fewest bins (append mode reads its interaction mask)
    for (int r = 1; r < nres; ++r)
        if (c.n_bins[r] < c.n_bins[rc]) rc = r;
    if (attrib_ws(h, who) || h->aw.slot_rows.need((size_t)nres * B * C * c.d_emb, 0, who)) return -1;
    hipStream_t st = (hipStream_t)stream;
    TransplantPackArgs pa;
    ScanUnpackArgs ua;
    TransplantRowsArgs ra;
    memset(&pa, 0, sizeof pa);
    memset(&ua, 0, sizeof ua);
    memset(&ra, 0, sizeof ra);
    cf_batch cb;      // the chunk's batch: pseudo-genes for the trunk, then rows (masks and frequencies) for Regulation + head
    chunk_rows(h, bt, &pa.rows, &cb);
    ra.rows = pa.rows;
    const size_t xv_res = (size_t)B * C * c.d_emb;
    for (int r = 0; r < nres; ++r) {
        pa.pf_in[r] = bt->promoter_feats[r];
        pa.pf_out[r] = h->aw.row[r];
        pa.cf_out[r] = h->aw.row[kMaxRes + r];
        pa.lib_feats[r] = o->lib_feats[r];
        pa.lib_mask[r] = o->lib_mask[r];
        ua.x0[r] = reinterpret_cast<const float4*>(h->Rx[r][0]);
        ua.xv[r] = reinterpret_cast<float4*>(h->aw.slot_rows + r * xv_res);
        ra.stash[r] = reinterpret_cast<const float4*>(h->aw.stash[r]);
        ra.xv[r] = ua.xv[r];
        ra.x0[r] = reinterpret_cast<float4*>(h->Rx[r][0]);
    }
    pa.U = U, pa.C = C, pa.F = c.n_feats;
    ua.U = U, ua.V = C + 1, ua.S = S, ua.T = T, ua.d4 = d4;
    ra.im_coarse = bt->interaction_mask[rc];
    ra.freq_in = bt->interaction_freq;
    ra.freq_out = h->aw.row[2 * kMaxRes];
    ra.freq = o->freq;
    ra.slot = o->slot;
    ra.slot_out = o->slot_out;
    ra.slot_all = o->slot_all;
    ra.V = V, ra.C = C, ra.Q = Q, ra.T = T, ra.row4 = T * d4, ra.d4 = d4;
    const long long launches0 = g_launches;
    auto run = [&]() -> int {
        if (forward_trunk(h, bt, 0, st) || stash_trunk_output(h, B, h->aw.stash, st)) return -1;
        for (int g0 = 0; g0 < B * U; g0 += cap) {
            const int n = std::min(cap, B * U - g0);
            pa.g0 = ua.g0 = g0;
            if (launch_expand(k_transplant_pack, "k_transplant_pack", dim3(n, nres), kRowThreads, pa, st)) return -1;
            cb.B = n;
            if (forward_trunk(h, &cb, 0, st, B)) return -1;
            if (launch_expand(k_scan_unpack, "k_scan_unpack", dim3(n, nres), kRowThreads, ua, st)) return -1;
        }
        return chunk_forward(h, &cb, rows, logits, false, B, st, [&](long long g0, int n) {
            ra.g0 = (int)g0;
            return launch_expand(k_transplant_rows, "k_transplant_rows", dim3(n, nres), kRowThreads, ra, st);
        });
    };
    const int rv = run();
    h->x0_fwd = false;
    forward_counted(h, launches0);
    return rv ? -1 : 0;
}
