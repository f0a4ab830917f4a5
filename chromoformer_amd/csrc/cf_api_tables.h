// cf_api_tables.h -- tables built at cf_bind: deferred-gradient tiles, the device tables of the fused Regulation stack and the fused trunk.
// Part of cf_api.hip's single translation unit: included there behind cf_api_handle.h, not on its own.
#pragma once

// ------------------------------------------------------------------------------------
// deferred gradient tables
// ------------------------------------------------------------------------------------
struct WgJob {
    WgSeg seg[4];
    int nseg;
    float* C;
    int ldc, Nn, Kk;
};
static void push_wg(std::vector<WgTile>& out, const WgJob& j) {
    for (int n0 = 0; n0 < j.Nn; n0 += 64)
        for (int k0 = 0; k0 < j.Kk; k0 += kWgTk) {
            WgTile t;
            memset(&t, 0, sizeof t);
            for (int s = 0; s < j.nseg; ++s) t.seg[s] = j.seg[s];
            t.nseg = j.nseg;
            t.C = j.C;
            t.ldc = j.ldc;
            t.Nn = j.Nn;
            t.Kk = j.Kk;
            t.n0 = n0;
            t.k0 = k0;
            t.toff = -1;
            out.push_back(t);
        }
}
static WgJob wg1(const float* A, int lda, const float* B, int ldb, int rpg, float* C, int ldc, int Nn, int Kk) {
    WgJob j;
    memset(&j, 0, sizeof j);
    j.seg[0] = WgSeg{A, B, lda, ldb, rpg};
    j.nseg = 1;
    j.C = C;
    j.ldc = ldc;
    j.Nn = Nn;
    j.Kk = Kk;
    return j;
}
static void push_cs(std::vector<CsTile>& out, const float* src, int ld, int ncols, int rpg, int div, float* dst, const float* src2 = nullptr) {
    for (int c0 = 0; c0 < ncols; c0 += 64) out.push_back(CsTile{src, dst, ld, ncols, c0, rpg, div, src2});
}
// the bias / LayerNorm gradients carried by one post-chain partial buffer
// (rows of the partial buffer: one per 16-row tile, M = ceil(rpg * batch / 16); one per gene with the fused trunk: rpg = div = 1)
template <class Params>      // CentreParams or RegParams
static void push_post_cs(std::vector<CsTile>& out, const cf_handle* h, const float* part, int dff, int rpg, const Params& p, int div = kTile) {
    const int kD = h->cfg.d_emb;      // (row width: shadows cf::kD in this function)
    const int pw = post_partial_width(dff, kD);
    push_cs(out, part + 0, pw, kD, rpg, div, h->grad_of(p.g2));
    push_cs(out, part + kD, pw, kD, rpg, div, h->grad_of(p.be2));
    push_cs(out, part + 2 * kD, pw, kD, rpg, div, h->grad_of(p.b2));
    push_cs(out, part + 3 * kD, pw, dff, rpg, div, h->grad_of(p.b1));
    push_cs(out, part + 3 * kD + dff, pw, kD, rpg, div, h->grad_of(p.g1));
    push_cs(out, part + 4 * kD + dff, pw, kD, rpg, div, h->grad_of(p.be1));
    push_cs(out, part + 5 * kD + dff, pw, kD, rpg, div, h->grad_of(p.bo));
}
// weight gradients of one centre-row layer (q / k / v projections, out-projection, FFN)
static void push_centre_wg(std::vector<WgTile>& out, const cf_handle* h, const CentreBuf& b, const float* xin, int ldxin,
                           int rpg, int dff, const CentreParams& p, int nh) {
    const int kD = h->cfg.d_emb;      // (row width: shadows cf::kD in this function)
    const int dh = kD / nh, qw = nh * kD;
    float *gWq = h->grad_of(p.wq), *gWk = h->grad_of(p.wk), *gWv = h->grad_of(p.wv);
    push_wg(out, wg1(b.dq, kD, xin, ldxin, rpg, gWq, kD, kD, kD));
    for (int hd = 0; hd < nh; ++hd) {
        push_wg(out, wg1(b.q + hd * dh, kD, b.dqt + hd * kD, qw, rpg, gWk + (size_t)hd * dh * kD, kD, dh, kD));
        push_wg(out, wg1(b.da + hd * dh, kD, b.xbar + hd * kD, qw, rpg, gWv + (size_t)hd * dh * kD, kD, dh, kD));
    }
    push_wg(out, wg1(b.dt1, kD, b.a, kD, rpg, h->grad_of(p.wo), kD, kD, kD));
    push_wg(out, wg1(b.dpre1, dff, b.y1, kD, rpg, h->grad_of(p.w1), kD, dff, kD));
    push_wg(out, wg1(b.dt2, kD, b.hdn, dff, rpg, h->grad_of(p.w2), dff, kD, dff));
}

// the fused Regulation kernels (cf_reg8.h): forward with / without the activation saves, backward; per FFN width
static const void* reg_kernel(bool bwd, int dff, bool save = true) {
    if (!bwd) {
        if (save) return dff == 128 ? (const void*)k_reg8_fwd<128, true> : (const void*)k_reg8_fwd<256, true>;
        return dff == 128 ? (const void*)k_reg8_fwd<128, false> : (const void*)k_reg8_fwd<256, false>;
    }
    return dff == 128 ? (const void*)k_reg8_bwd<128> : (const void*)k_reg8_bwd<256>;
}
static const void* reg_kernel_dfreq(int dff) { return dff == 128 ? (const void*)k_reg8_bwd<128, true> : (const void*)k_reg8_bwd<256, true>; }

static int build_reg_table(cf_handle* h) {
    const cf_config& c = h->cfg;
    if (h->reg_fused) {
        std::vector<RegLayerDev> rt;
        for (int r = 0; r < c.n_res; ++r)
            for (int l = 0; l < c.reg_layers; ++l) {
                const RegParams& p = h->refs.R[r][l];
                const RegBuf& b = h->R[r][l];
                RegLayerDev d;
                d.watt = p.watt, d.gamma = p.gamma, d.wo = p.wo, d.bo = p.bo, d.g1 = p.g1, d.be1 = p.be1;
                d.w1 = p.w1, d.b1 = p.b1, d.w2 = p.w2, d.b2 = p.b2, d.g2 = p.g2, d.be2 = p.be2;
                d.watt_t = h->tiled_of(p.watt), d.wo_t = h->tiled_of(p.wo), d.w1_t = h->tiled_of(p.w1), d.w2_t = h->tiled_of(p.w2);
                d.watt_tt = h->tiledT_of(p.watt), d.wo_tt = h->tiledT_of(p.wo), d.w1_tt = h->tiledT_of(p.w1), d.w2_tt = h->tiledT_of(p.w2);
                d.xin = h->Rx[r][l], d.xout = h->Rx[r][l + 1], d.dxout = h->dRx[r][l + 1], d.dxin = h->dRx[r][l];
                d.qkvg = b.qkvg, d.p = b.p, d.a = b.a, d.xh1 = b.xh1, d.rs1 = b.rs1, d.y1 = b.y1, d.hdn = b.hdn, d.xh2 = b.xh2, d.rs2 = b.rs2;
                d.dt2 = b.dt2, d.dpre1 = b.dpre1, d.dt1 = b.dt1, d.da = b.da, d.dqkvg = b.dqkvg, d.partial = b.partial, d.dgam = b.dgam;
                d.hq = b.hq, d.dy1 = b.dy1;
                rt.push_back(d);
            }
        if (h->reg_tab.upload(rt, "cf_bind: the Regulation layer table")) return -1;
    }
    return 0;
}

static int build_tables(cf_handle* h) {
    const cf_config& c = h->cfg;
    const int kD = c.d_emb;      // (row width: shadows cf::kD in this function)
    const int S = c.i_max, T = S + 1, F = c.n_feats;
    // two gradient buckets: `wg` / `cs` take Embedding + Pairwise (ready after the whole backward chain), `wgR` / `csR`
    // the Regulation stacks and the head (ready after k_reg_bwd, i.e. before Pairwise + Embedding backward starts)
    std::vector<WgTile> wg, wgHi, wgLo, wgShort;
    std::vector<CsTile> cs, csHi, csLo;
    std::vector<LpJob> lpj;
    const ModelRefs& m = h->refs;
    for (int r = 0; r < c.n_res; ++r) {
        if (!h->embed_dense) {   // Embedding (the all-rows path writes its gradients itself)
            const CentreParams& p = m.E[r];
            const CentreBuf& b = h->E[r];
            LpJob j;
            memset(&j, 0, sizeof j);
            j.seg[0] = WgSeg{h->edx0[r], h->featc[r], kD, 8, 1};
            j.seg[1] = WgSeg{b.dxbar, b.w, kD, 8, c.embed_heads};      // (rows of [N, heads, .] arrays: heads per gene)
            j.seg[2] = WgSeg{b.qt, b.du, kD, 8, c.embed_heads};
            j.nseg = 3;
            j.partial = h->lp_part_e[r];
            j.F = F;
            lpj.push_back(j);
            push_cs(cs, j.partial, kD * F, kD * F, 1, kLpGenes, h->grad_of(m.lin_proj[r]));
            push_centre_wg(wg, h, b, h->ex0[r], kD, 1, c.embed_dff, p, c.embed_heads);
            if (h->trunk) push_post_cs(cs, h, b.partial, c.embed_dff, 1, p, 1);
            else push_post_cs(cs, h, b.partial, c.embed_dff, 1, p);
        }
        {   // Pairwise
            push_wg(wg, wg1(h->dxp0[r], kD, h->Rx[r][0], T * kD, 1, h->grad_of(m.lin_proj_p[r]), kD, kD, kD));
            LpJob j;
            memset(&j, 0, sizeof j);
            // lin_proj_pcre collects two terms per layer (pair_layers <= 8 -> <= kLpMaxSeg segments)
            int ns = 0;
            for (int l = 0; l < c.pair_layers; ++l) {
                j.seg[ns++] = WgSeg{h->P[r][l].dxbar, h->P[r][l].w, kD, 8, c.pair_heads * S};
                j.seg[ns++] = WgSeg{h->P[r][l].qt, h->P[r][l].du, kD, 8, c.pair_heads * S};
            }
            j.nseg = ns;
            j.partial = h->lp_part_p[r];
            j.F = F;
            lpj.push_back(j);
            push_cs(cs, j.partial, kD * F, kD * F, 1, kLpGenes, h->grad_of(m.P[r][0].wlp));
            for (int l = 0; l < c.pair_layers; ++l) {
                const CentreParams& p = m.P[r][l];
                const CentreBuf& b = h->P[r][l];
                const float* xin = l == 0 ? b.xin : h->P[r][l - 1].out;
                push_centre_wg(wg, h, b, xin, kD, S, c.pair_dff, p, c.pair_heads);
                if (h->trunk) push_post_cs(cs, h, b.partial, c.pair_dff, 1, p, 1);
                else push_post_cs(cs, h, b.partial, c.pair_dff, S, p);
            }
        }
        for (int l = 0; l < c.reg_layers; ++l) {   // Regulation: the upper half of the stack (complete first in the backward pass) and the lower one
            std::vector<WgTile>& wgR = l >= c.reg_layers / 2 ? wgHi : wgLo;
            std::vector<CsTile>& csR = l >= c.reg_layers / 2 ? csHi : csLo;
            const RegParams& p = m.R[r][l];
            const RegBuf& b = h->R[r][l];
            const int dff = c.reg_dff;
            const int RDm = c.reg_dmodel, RW = 4 * RDm;
            if (l + 1 == c.reg_layers && h->reg_row0 && h->reg8) {
                // The last layer, reduced to what token 0 of its output needs (cf_reg8.h: b_run_row0 / b_run_kv_rows): every gradient above the attention
                // -- out-projection, FFN, the query and gate quarters of the input projection -- has ONE live row per gene, the rows of tokens 1 .. T - 1
                // are zeros the kernel writes.  Their reductions walk that row alone (rows_per_gene = 1 at a stride of T rows: 64 reduction rows
                // instead of 576, a ninth of the operand bytes); the key and value quarters keep all rows.  Same sums: what is left out are exact zeros.
                float* ga = h->grad_of(p.watt);
                push_wg(wgShort, wg1(b.dqkvg, T * RW, h->Rx[r][l], T * kD, 1, ga, kD, RDm, kD));                                                            // q
                push_wg(wgR, wg1(b.dqkvg + RDm, RW, h->Rx[r][l], kD, T, ga + (size_t)RDm * kD, kD, 2 * RDm, kD));                                           // k | v
                push_wg(wgShort, wg1(b.dqkvg + 3 * RDm, T * RW, h->Rx[r][l], T * kD, 1, ga + (size_t)3 * RDm * kD, kD, RDm, kD));                            // gate
                push_wg(wgShort, wg1(b.dt1, T * kD, b.a, T * RDm, 1, h->grad_of(p.wo), RDm, kD, RDm));
                push_wg(wgShort, wg1(b.dpre1, T * dff, b.y1, T * kD, 1, h->grad_of(p.w1), kD, dff, kD));
                push_wg(wgShort, wg1(b.dt2, T * kD, b.hdn, T * dff, 1, h->grad_of(p.w2), dff, kD, dff));
            } else {
            push_wg(wgR, wg1(b.dqkvg, RW, h->Rx[r][l], kD, T, h->grad_of(p.watt), kD, RW, kD));
            push_wg(wgR, wg1(b.dt1, kD, b.a, RDm, T, h->grad_of(p.wo), RDm, kD, RDm));
            push_wg(wgR, wg1(b.dpre1, dff, b.y1, kD, T, h->grad_of(p.w1), kD, dff, kD));
            push_wg(wgR, wg1(b.dt2, kD, b.hdn, dff, T, h->grad_of(p.w2), dff, kD, dff));
            }
            if (h->reg8) {            // column sums straight from the row-level arrays the backward kernel writes anyway
                push_cs(csR, h->dRx[r][l + 1], kD, kD, T, 1, h->grad_of(p.g2), b.xh2);
                push_cs(csR, h->dRx[r][l + 1], kD, kD, T, 1, h->grad_of(p.be2));
                push_cs(csR, b.dt2, kD, kD, T, 1, h->grad_of(p.b2));
                push_cs(csR, b.dpre1, dff, dff, T, 1, h->grad_of(p.b1));
                push_cs(csR, b.dy1, kD, kD, T, 1, h->grad_of(p.g1), b.xh1);
                push_cs(csR, b.dy1, kD, kD, T, 1, h->grad_of(p.be1));
                push_cs(csR, b.dt1, kD, kD, T, 1, h->grad_of(p.bo));
            } else {
                push_post_cs(csR, h, b.partial, dff, T, p);
            }
            push_cs(csR, b.dgam, c.reg_heads, c.reg_heads, 1, 1, h->grad_of(p.gamma));
        }
    }
    push_wg(wgShort, wg1(h->dh1, c.d_head, h->hin, 3 * kD, 1, h->grad_of(m.head.w1), 3 * kD, c.d_head, 3 * kD));
    push_wg(wgShort, wg1(h->dlogits, c.n_out, h->h1, c.d_head, 1, h->grad_of(m.head.w2), c.d_head, c.n_out, c.d_head));
    // the short tiles -- one reduction row per gene -- lead the upper bucket: the riders of k_trunk_bwd take the window BEHIND them (a rider is a
    // single wave: a long tile each keeps the rider waves equally busy), the reduction launch what lies on either side of that window
    h->n_wg_short = (int)wgShort.size();
    wgHi.insert(wgHi.begin(), wgShort.begin(), wgShort.end());
    push_cs(csHi, h->dh1, c.d_head, c.d_head, 1, 1, h->grad_of(m.head.b1));
    push_cs(csHi, h->dlogits, c.n_out, c.n_out, 1, 1, h->grad_of(m.head.b2));

    if (h->lp_jobs.upload(lpj, "cf_bind: the lin_proj gradient jobs")) return -1;
    h->n_lp = (int)lpj.size();
    // Embedding + Pairwise tiles whose tensor has a tiled copy: where the tensor starts in the flat buffers and which of its rows the tile's row 0 is
    // (AdamFuse::tiled: the optimiser epilogue writes the stepped elements into the tiled copy as well)
    for (WgTile& t : wg) {
        const long long e0 = t.C - h->grads;
        for (const PDesc& p : h->table) {
            if (e0 < p.offset || e0 >= p.offset + p.numel) continue;
            const bool tiled_copy = p.ndim == 2 && p.shape[0] % 16 == 0 && p.shape[1] % 16 == 0 && p.trainable;
            if (tiled_copy && t.ldc == p.shape[1] && (e0 - p.offset) % p.shape[1] == 0) {
                t.toff = p.offset;
                t.trow0 = (int)((e0 - p.offset) / p.shape[1]);
            }
            break;
        }
    }
    {   // ... and every tensor the forward pass re-tiles up front must be covered completely, or the mode is not offered (cf_keep_tiled)
        h->keep_tiled_ok = !h->embed_dense;
        for (const PDesc& p : h->table) {
            const bool is_late = p.name.rfind("regulation.", 0) == 0 || p.name.rfind("fc_head.", 0) == 0;
            if (is_late || !(p.ndim == 2 && p.shape[0] % 16 == 0 && p.shape[1] % 16 == 0 && p.trainable)) continue;
            long long covered = 0;
            for (const WgTile& t : wg)
                if (t.toff == p.offset) covered += (long long)std::min(64, t.Nn - t.n0) * std::min(kWgTk, t.Kk - t.k0);
            if (covered != p.numel) h->keep_tiled_ok = false;
        }
    }
    if (h->keep_tiled_ok) {      // the float4 map of the separate AdamW launch (data parallel): flat -> tiled, for the same tensors
        std::vector<int> map((size_t)h->bucket_split / 4, -1);
        for (const PDesc& p : h->table) {
            const bool is_late = p.name.rfind("regulation.", 0) == 0 || p.name.rfind("fc_head.", 0) == 0;
            if (is_late || !(p.ndim == 2 && p.shape[0] % 16 == 0 && p.shape[1] % 16 == 0 && p.trainable)) continue;
            const int N = p.shape[0], K = p.shape[1];
            for (int n = 0; n < N; ++n)
                for (int k = 0; k < K; k += 4) {
                    const long long flat = p.offset + (long long)n * K + k;
                    const long long til = p.offset + ((long long)(n / 16) * (K / 16) + k / 16) * 256 + (((k % 16) / 4) * 16 + n % 16) * 4;
                    map[(size_t)(flat / 4)] = (int)(til / 4);
                }
        }
        if (h->tiled_map.upload(map, "cf_bind: the flat-to-tiled map")) return -1;
    }
    h->n_wg_hi = (int)wgHi.size();
    h->n_cs_hi = (int)csHi.size();
    h->n_wg_r = (int)(wgHi.size() + wgLo.size());
    h->n_cs_r = (int)(csHi.size() + csLo.size());
    wg.insert(wg.begin(), wgLo.begin(), wgLo.end());      // table layout: [upper Regulation layers + head | lower Regulation layers | Embedding + Pairwise]
    wg.insert(wg.begin(), wgHi.begin(), wgHi.end());
    cs.insert(cs.begin(), csLo.begin(), csLo.end());
    cs.insert(cs.begin(), csHi.begin(), csHi.end());
    h->wg_flops_per_gene = 0.0;
    for (const WgTile& t : wg) {
        if (t.n0 || t.k0) continue;      // count each job once
        for (int sgi = 0; sgi < t.nseg; ++sgi) h->wg_flops_per_gene += 2.0 * t.seg[sgi].rows_per_gene * (double)t.Nn * t.Kk;
    }
    if (h->wg_tiles.upload(wg, "cf_bind: the weight-gradient tiles") || h->cs_tiles.upload(cs, "cf_bind: the column-sum tiles")) return -1;
    h->n_wg = (int)wg.size();
    h->n_cs = (int)cs.size();
    return 0;
}

// device table of the fused centre-row trunk (cf_trunk.h)
static const void* trunk_kernel(bool bwd, int dff_e, int dff_p, int pair_layers) {
    if (dff_e == 128 && dff_p == 256 && pair_layers == 2) return bwd ? (const void*)k_trunk_bwd<128, 256, 2> : (const void*)k_trunk_fwd<128, 256, 2>;
    return nullptr;      // (other shapes run the stand-alone kernels)
}
static void fill_centre_dev(CentreLayerDev& d, const CentreParams& p, const CentreBuf& b) {
    d.wq_t = p.wq_t, d.wk = p.wk, d.wv_t = p.wv_t, d.wo_t = p.wo_t, d.bo = p.bo, d.g1 = p.g1, d.be1 = p.be1;
    d.w1_t = p.w1_t, d.b1 = p.b1, d.w2_t = p.w2_t, d.b2 = p.b2, d.g2 = p.g2, d.be2 = p.be2;
    d.wq = p.wq, d.wk_t = p.wk_t, d.wv = p.wv, d.wo = p.wo, d.w1 = p.w1, d.w2 = p.w2;
    d.q = b.q, d.qt = b.qt, d.p = b.p, d.w = b.w, d.xbar = b.xbar, d.a = b.a, d.xh1 = b.xh1, d.rs1 = b.rs1, d.y1 = b.y1;
    d.hdn = b.hdn, d.xh2 = b.xh2, d.rs2 = b.rs2, d.out = b.out, d.xin = b.xin;
    d.dt2 = b.dt2, d.dpre1 = b.dpre1, d.dt1 = b.dt1, d.da = b.da, d.dxbar = b.dxbar, d.dqt = b.dqt, d.du = b.du, d.dq = b.dq;
    d.dx = b.dx, d.partial = b.partial;
}
static int build_trunk_table(cf_handle* h) {
    const cf_config& c = h->cfg;
    h->trunk = false;
    if (h->embed_dense || !h->attc2 || c.i_max > kAGMax || c.pair_layers > kMaxPairLayers || kPostWaves != 8) return 0;
    if (c.embed_heads != 2 || c.pair_heads != 2 || c.d_emb != kD) return 0;      // (the fused kernels are written for two heads and 128-wide rows)
    if (!trunk_kernel(false, c.embed_dff, c.pair_dff, c.pair_layers)) return 0;
    if (const char* e = getenv("CF_TRUNK"))      // CF_TRUNK=0: the stand-alone kernels (A/B runs, cross-checks in the tests)
        if (atoi(e) == 0) return 0;
    size_t need = 0;
    for (int r = 0; r < c.n_res; ++r) need = std::max(need, trunk_smem(c.n_bins[r], c.n_feats, std::max(c.embed_dff, c.pair_dff)));
    if (need > 160 * 1024) return 0;
    const size_t need_bwd = std::max(need, (size_t)(kAT / 64) * kWgWaveLds * sizeof(float));      // (riders of the backward launch: cf_rider_arm)
    if (need_bwd > 160 * 1024) return 0;
    if (hipFuncSetAttribute(trunk_kernel(false, c.embed_dff, c.pair_dff, c.pair_layers), hipFuncAttributeMaxDynamicSharedMemorySize, (int)need) != hipSuccess ||
        hipFuncSetAttribute(trunk_kernel(true, c.embed_dff, c.pair_dff, c.pair_layers), hipFuncAttributeMaxDynamicSharedMemorySize, (int)need_bwd) != hipSuccess)
        return 0;
    std::vector<TrunkResDev> tab(c.n_res);
    for (int r = 0; r < c.n_res; ++r) {
        TrunkResDev& t = tab[r];
        memset(&t, 0, sizeof t);
        fill_centre_dev(t.E, h->refs.E[r], h->E[r]);
        for (int l = 0; l < c.pair_layers; ++l) fill_centre_dev(t.P[l], h->refs.P[r][l], h->P[r][l]);
        t.pe = h->pe[r], t.pe2 = h->pe2[r], t.pet2 = h->pet2[r];
        t.wlp_e = h->refs.E[r].wlp;
        t.wlp_p = h->refs.P[r][0].wlp;
        t.lin_p = h->refs.lin_proj_p[r];
        t.lin_p_t = h->tiled_of(t.lin_p);
        t.ex0 = h->ex0[r], t.featc = h->featc[r], t.xp0 = h->xp0[r], t.dxp0 = h->dxp0[r], t.edout = h->edout[r];
        t.rx0 = h->Rx[r][0], t.drx0 = h->dRx[r][0];
        t.lp_part_e = h->lp_part_e[r], t.lp_part_p = h->lp_part_p[r];
        t.L = c.n_bins[r], t.Lpad = attc2_lpad(c.n_bins[r]), t.LT = attc2_lt(c.n_bins[r]);
    }
    if (h->trunk_tab.upload(tab, "cf_bind: the trunk table")) return -1;
    h->trunk_smem_bytes = need;
    h->trunk = true;
    return 0;
}
