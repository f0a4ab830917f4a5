// cf_api_launch.h -- launch helpers shared by the model path and the stand-alone operators: the width / head-count dispatch, the row-tile chain
// and centre-row attention launches, the argument builders of the fused trunk, the fused Regulation stack and the head.
// Part of cf_api.hip's single translation unit: included there behind cf_api_feed.h, not on its own.
#pragma once

// ------------------------------------------------------------------------------------
// launch helpers
// ------------------------------------------------------------------------------------
static inline int tiles_of(int n) { return (n + kTile - 1) / kTile; }
static size_t attc_smem(int L, int F, bool bwd, int nh = 2, int D = kD) {
    const int parts = 256 / D > 2 ? 256 / D - 1 : 1;
    return (size_t)((1 + parts) * nh * D + 20 * nh + nh * L + (bwd ? nh * L : 0) + L * F) * sizeof(float);
}
static size_t attr_smem(int T, int H, int DM, bool bwd) {
    return (size_t)(T * 4 * DM + H * T * T + (bwd ? H * T * T + T * DM + H * T : 0)) * sizeof(float);
}

// Calls f(std::integral_constant<int, V>()) for the V of the list that equals v and returns what it returns: the one place where a run-time
// row width, head count, model or FFN width becomes a template argument.  Only the listed values are instantiated; any other is an error.
template <int... Vs, class F>
static int with_int(const char* what, int v, F&& f) {
    bool hit = false;
    int rc = 0;
    (void)((v == Vs ? (hit = true, rc = f(std::integral_constant<int, Vs>()), true) : false) || ...);
    return hit ? rc : fail("no kernel of this library is instantiated for %s = %d", what, v);
}
// f(row width, heads) of a centre-row layer on the stand-alone chain kernels: 1 or 4 heads at 128 (two heads take the default launches),
// 1 or 2 heads at 64 / 256 (check_config)
template <class F>
static int with_centre_shape(int D, int nh, F&& f) {
    if (D == 128) return with_int<1, 4>("heads", nh, [&](auto n) { return f(std::integral_constant<int, 128>(), n); });
    return with_int<64, 256>("d_emb", D, [&](auto d) { return with_int<1, 2>("heads", nh, [&](auto n) { return f(d, n); }); });
}
// f(row width, d_model) of a Regulation layer on the stand-alone kernels
template <class F>
static int with_reg_shape(int D, int DM, F&& f) {
    return with_int<64, 128, 256>("d_emb", D, [&](auto d) { return with_int<128, 256>("regulation d_model", DM, [&](auto dm) { return f(d, dm); }); });
}

template <bool VPROJ, int DM, int D = 128>
static int launch_post_fwd(int dff, dim3 grid, hipStream_t st, const PostArgs& a) {
    return with_int<128, 256>("d_ff", dff, [&](auto ff) {
        constexpr int DFF = decltype(ff)::value;
        if constexpr (D != 128) {      // (rows of another width: the chain kernels with the width as a template parameter; four waves at 64)
            constexpr int NWV = D == 64 ? 4 : 8;
            hipLaunchKernelGGL((k_post_fwd<VPROJ, DM, DFF, NWV, false, 2, D>), grid, dim3(NWV * 64), 0, st, a);
            return 0;
        } else {
            if constexpr (VPROJ && DM == 128) {      // the hosting instantiation (eight waves; the Embedding layer's launch asks for it, nobody else)
                if (a.rt_units) {
                    hipLaunchKernelGGL((k_post_fwd<VPROJ, DM, DFF, 8, true>), grid, dim3(512), 0, st, a);
                    return 0;
                }
            }
            // (kPostWaves is a compile-time switch: only the selected form is instantiated)
            hipLaunchKernelGGL((k_post_fwd<VPROJ, DM, DFF, kPostWaves>), grid, dim3(kPostWaves * 64), 0, st, a);
            return 0;
        }
    });
}
template <bool VPROJ, int DM, int D = 128>
static int launch_post_bwd(int dff, dim3 grid, hipStream_t st, const PostBwdArgs& a) {
    return with_int<128, 256>("d_ff", dff, [&](auto ff) {
        constexpr int DFF = decltype(ff)::value;
        if constexpr (D != 128) {
            constexpr int NWV = D == 64 ? 4 : 8;
            hipLaunchKernelGGL((k_post_bwd<VPROJ, DM, DFF, NWV, 2, D>), grid, dim3(NWV * 64), 0, st, a);
        } else {
            hipLaunchKernelGGL((k_post_bwd<VPROJ, DM, DFF, kPostWaves>), grid, dim3(kPostWaves * 64), 0, st, a);
        }
        return 0;
    });
}

// The stand-alone stages of one centre-row layer for a head count other than 2 (eight-wave chain kernels, the one-sequence-per-workgroup
// attention): the same argument structures as the default launches, [N, NH, .] arrays.
// D: the row width (d_emb; the Embedding / Pairwise attention width is the same, net.py:305 / 361-370).  Every shape but the default
// (two heads, 128) takes this route.
template <int NH, int D = 128>
static int centre_fwd_heads(hipStream_t st, int N, int nres, int dff, bool q_done, const QChainArgs& q, const AttcArgs& at, size_t smem,
                            const PostArgs& po) {
    constexpr int NWV = D == 64 ? 4 : 8;      // (a wave owns at least one 16-column tile of a D-wide product)
    if (!q_done) {
        hipLaunchKernelGGL((k_qchain_fwd<NWV, NH, D>), dim3(tiles_of(N), nres), dim3(NWV * 64), 0, st, q);
        LAUNCH_CHECK("k_qchain_fwd");
    }
    hipLaunchKernelGGL((k_attc<false, NH, D>), dim3(N, nres), dim3(256), smem, st, at);
    LAUNCH_CHECK("k_attc<fwd>");
    if (with_int<128, 256>("d_ff", dff, [&](auto ff) {
            hipLaunchKernelGGL((k_post_fwd<true, D, decltype(ff)::value, NWV, false, NH, D>), dim3(tiles_of(N), nres), dim3(NWV * 64), 0, st, po);
            return 0;
        }))
        return -1;
    LAUNCH_CHECK("k_post_fwd<centre>");
    return 0;
}
template <int NH, int D = 128>
static int centre_bwd_heads(hipStream_t st, int N, int nres, int dff, const PostBwdArgs& pb, const AttcArgs& at, size_t smem, const QBwdArgs& qb) {
    constexpr int NWV = D == 64 ? 4 : 8;
    if (with_int<128, 256>("d_ff", dff, [&](auto ff) {
            hipLaunchKernelGGL((k_post_bwd<true, D, decltype(ff)::value, NWV, NH, D>), dim3(tiles_of(N), nres), dim3(NWV * 64), 0, st, pb);
            return 0;
        }))
        return -1;
    LAUNCH_CHECK("k_post_bwd<centre>");
    hipLaunchKernelGGL((k_attc<true, NH, D>), dim3(N, nres), dim3(256), smem, st, at);
    LAUNCH_CHECK("k_attc<bwd>");
    hipLaunchKernelGGL((k_qchain_bwd<NWV, NH, D>), dim3(tiles_of(N), nres), dim3(NWV * 64), 0, st, qb);
    LAUNCH_CHECK("k_qchain_bwd");
    return 0;
}

// Options of one pass that are not handle state: the attribution entry points (cf_api_attrib.h) set them, training passes the default.
struct PassOpts {
    float* dfreq = nullptr;                    // the Regulation backward also leaves d(interaction_freq) per resolution here (cf_handle::dfreq_part)
    bool no_dense_embed_bwd = false;           // the all-rows Embedding backward (it writes parameter gradients) is not run
    int ag_genes = 0;                          // k_attc2 regions per workgroup chosen as for a batch of this many genes (0: the batch's own)
};
// The centre-row attention launch of the default shape (two heads, 128): gene-batched (cf_attc2.h, one region per workgroup on cf_attc1.h)
// where its LDS image fits, else k_attc.  Forward and backward pass take the same route.
template <bool BWD>
static int launch_attc(cf_handle* h, const AttcArgs& at, int N, int B, size_t smem, int ag_genes, hipStream_t st) {
    const int nres = h->cfg.n_res;
    if (h->attc2) {
        const int ag = attc2_regions_per_wg(ag_genes ? N / B * ag_genes : N, h->attc_cap);
        Attc2Args a2;
        size_t sm2 = 0;
        for (int r = 0; r < nres; ++r) {
            a2.feats[r] = at.feats[r];
            a2.mask[r] = at.mask[r];
            a2.mstride[r] = at.mstride[r];
            a2.pe[r] = h->pe2[r];
            a2.pet[r] = h->pet2[r];
            a2.wlp[r] = at.wlp[r];
            a2.vin[r] = at.vin[r];
            a2.p[r] = at.p[r];
            a2.w[r] = at.w[r];
            a2.vout[r] = at.vout[r];
            a2.L[r] = at.L[r];
            a2.Lpad[r] = attc2_lpad(at.L[r]);
            a2.LT[r] = attc2_lt(at.L[r]);
            sm2 = std::max(sm2, attc2_smem(at.L[r], at.F, ag));
        }
        a2.N = N;
        a2.F = at.F;
        a2.scale = at.scale;
        a2.rscale = 1.0f / a2.scale;
        a2.tdbg = (getenv("CF_STAMP_ATTC") && (!getenv("CF_STAMP_ATTC_AG") || atoi(getenv("CF_STAMP_ATTC_AG")) == ag))
                      ? reinterpret_cast<unsigned long long*>(h->tdbg) + 256 : nullptr;
        a2.tall = (getenv("CF_STAMP_ATTC_ALL") && atoi(getenv("CF_STAMP_ATTC_ALL")) == (BWD ? 1 : 0) && (!getenv("CF_STAMP_ATTC_AG") || atoi(getenv("CF_STAMP_ATTC_AG")) == ag))
                      ? reinterpret_cast<unsigned long long*>(h->tdbg) + 256 : nullptr;
        void* kargs2[] = {&a2};
        if (ag == 1 && h->attc1) {      // one region per workgroup: the vector-ALU kernel (cf_attc1.h)
            size_t sm1 = 0;
            for (int r = 0; r < nres; ++r) sm1 = std::max(sm1, attc1_smem(at.L[r], at.F));
            HIP_TRY(hipLaunchKernel((const void*)k_attc1<BWD>, dim3(N, nres), dim3(kAT), kargs2, sm1, st));
        } else {
            HIP_TRY(hipLaunchKernel(attc2_kernel<BWD>(ag), dim3((N + ag - 1) / ag, nres), dim3(kAT), kargs2, sm2, st));
        }
    } else {
        hipLaunchKernelGGL((k_attc<BWD>), dim3(N, nres), dim3(256), smem, st, at);
    }
    LAUNCH_CHECK(BWD ? "k_attc<bwd>" : "k_attc<fwd>");
    return 0;
}

static void trunk_args(const cf_handle* h, const cf_batch* bt, TrunkArgs& a, int save) {
    const cf_config& c = h->cfg;
    memset(&a, 0, sizeof a);
    a.tab = h->trunk_tab;
    for (int r = 0; r < c.n_res; ++r) {
        a.pfeats[r] = bt->promoter_feats[r], a.pmask[r] = bt->promoter_mask_row[r], a.pmstride[r] = bt->promoter_mask_stride[r];
        a.cfeats[r] = bt->pcre_feats[r], a.cmask[r] = bt->pcre_mask_row[r], a.cmstride[r] = bt->pcre_mask_stride[r];
    }
    a.dhin = h->dhin;
    a.B = bt->B, a.S = c.i_max, a.T = c.i_max + 1, a.F = c.n_feats, a.n_res = c.n_res, a.pair_layers = c.pair_layers, a.save = save;
    a.scale = sqrtf(64.f);
    a.rscale = 1.0f / a.scale;
    a.tdbg = getenv("CF_STAMP_TRUNK") ? reinterpret_cast<unsigned long long*>(h->tdbg) : nullptr;      // tools/trunk_stamps.py
}

// Launch of a fused Regulation kernel.  Under capture, if it is the kernel selected with cf_timing_select, the
// capture is split around it: the launch is remembered instead of recorded and cf_graph_launch issues it eagerly,
// between two HIP events, between the two graph pieces.
static int launch_reg(cf_handle* h, const char* name, const void* fn, dim3 grid, size_t smem, RegArgs& ra, hipStream_t st) {
    const dim3 block(512);
    if (h->capturing && h->timed == name && !h->cap.has_hole) {
        hipGraph_t g = nullptr;
        HIP_TRY(hipStreamEndCapture(st, &g));
        hipError_t e = hipGraphInstantiate(&h->cap.first, g, nullptr, nullptr, 0);
        (void)hipGraphDestroy(g);
        if (e != hipSuccess) return fail("hipGraphInstantiate failed: %s", hipGetErrorString(e));
        h->cap.has_hole = true;
        h->cap.hole.func = fn;
        h->cap.hole.grid = grid;
        h->cap.hole.block = block;
        h->cap.hole.smem = smem;
        h->cap.hole.args = ra;
        HIP_TRY(hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed));
        ++g_launches;      // (issued by cf_graph_launch between the two graph pieces)
        return 0;
    }
    void* kargs[] = {&ra};
    h->time_mark(name, st);
    HIP_TRY(hipLaunchKernel(fn, grid, block, kargs, smem, st));
    h->time_mark(name, st);
    LAUNCH_CHECK(name);
    return 0;
}

static void head_gen_args(const cf_handle* h, int B, float* logits_user, HeadGenArgs& a) {      // d_head != 128: the vector-ALU head (cf_head.h)
    const cf_config& c = h->cfg;
    memset(&a, 0, sizeof a);
    for (int r = 0; r < c.n_res; ++r) {
        a.xl[r] = h->Rx[r][c.reg_layers];
        a.x0[r] = h->Rx[r][0];
        a.dxl[r] = h->dRx[r][c.reg_layers];
    }
    a.w1 = h->refs.head.w1;
    a.b1 = h->refs.head.b1;
    a.w2 = h->refs.head.w2;
    a.b2 = h->refs.head.b2;
    a.hin = h->hin, a.h1 = h->h1, a.logits = h->logits, a.logits_user = logits_user;
    a.dlogits = h->dlogits, a.dh1 = h->dh1, a.dhin = h->dhin;
    a.loss = h->loss, a.loss_part = h->loss_part;
    a.B = B, a.T = c.i_max + 1, a.n_res = c.n_res, a.n_out = c.n_out, a.DH = c.d_head;
    a.D = c.d_emb;
}
static void head_fwd_args(const cf_handle* h, int B, float* logits_user, HeadFwdArgs& a) {
    const cf_config& c = h->cfg;
    for (int r = 0; r < c.n_res; ++r) {
        a.xl[r] = h->Rx[r][c.reg_layers];
        a.x0[r] = h->Rx[r][0];
    }
    a.w1_t = h->tiled_of(h->refs.head.w1);
    a.b1 = h->refs.head.b1;
    a.w2 = h->refs.head.w2;
    a.b2 = h->refs.head.b2;
    a.hin = h->hin;
    a.h1 = h->h1;
    a.logits = h->logits;
    a.logits_user = logits_user;
    a.B = B;
    a.T = c.i_max + 1;
    a.n_res = c.n_res;
    a.n_out = c.n_out;
    a.tdbg = getenv("CF_STAMP_HEAD") ? reinterpret_cast<unsigned long long*>(h->tdbg) + 128 : nullptr;      // tools/head_stamps.py
}

