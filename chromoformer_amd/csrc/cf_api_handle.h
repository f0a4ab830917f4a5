// cf_api_handle.h -- errors, parameter layout, the handle, the workspace plan and the parameter references resolved at cf_bind.
// Part of cf_api.hip's single translation unit: included there first, not on its own.
#pragma once

// ------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------
static thread_local std::string g_err;
static int fail(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return -1;
}
#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) return fail("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)
// every kernel launch of the library passes through LAUNCH_CHECK exactly once: the counter behind cf_launch_counts
static thread_local long long g_launches = 0;
#define LAUNCH_CHECK(name)                                                                     \
    do {                                                                                       \
        ++g_launches;                                                                          \
        hipError_t e_ = hipGetLastError();                                                     \
        if (e_ != hipSuccess) return fail("launch %s failed: %s", name, hipGetErrorString(e_)); \
    } while (0)
#include "cf_devbuf.h"      // DevBuf<T>, the owner of every device allocation below (it reports through fail)

// ------------------------------------------------------------------------------------
// parameter layout (host only)
// ------------------------------------------------------------------------------------
constexpr int kMaxEmbedLayers = 8;
#ifndef CF_POST_WAVES
#define CF_POST_WAVES 8
#endif
constexpr int kPostWaves = CF_POST_WAVES;      // waves per workgroup of the row-tile chains (k_post_*, k_qchain_*): 4 or 8; the fused trunk needs 8

struct PDesc {
    std::string name;
    int ndim;
    int shape[2];
    long long numel, offset;
    bool trainable;
};

static int getenv_int(const char* name, int dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}
static std::string fmt(const char* f, ...) {
    char buf[256];
    va_list ap;
    va_start(ap, f);
    vsnprintf(buf, sizeof buf, f, ap);
    va_end(ap);
    return buf;
}
static void add(std::vector<PDesc>& v, const std::string& name, int d0, int d1, bool trainable) {
    PDesc p;
    p.name = name;
    p.ndim = d1 > 0 ? 2 : 1;
    p.shape[0] = d0;
    p.shape[1] = d1 > 0 ? d1 : 0;
    p.numel = (long long)d0 * (d1 > 0 ? d1 : 1);
    p.offset = -1;
    p.trainable = trainable;
    v.push_back(p);
}
// the seven tensors of an attention block, four/three-chunk self attention (modules.py:16-25)
static void add_self_att(std::vector<PDesc>& v, const std::string& pre, int d_emb, int heads, int dm, bool gate, bool gamma_trains) {
    add(v, pre + "gamma_f", heads, 0, gamma_trains);
    add(v, pre + "w_bias.weight", heads, 2, false);
    add(v, pre + "att.weight", (gate ? 4 : 3) * dm, d_emb, true);
    add(v, pre + "ff.weight", d_emb, dm, true);
    add(v, pre + "ff.bias", d_emb, 0, true);
    add(v, pre + "ln.weight", d_emb, 0, true);
    add(v, pre + "ln.bias", d_emb, 0, true);
}
static void add_ffn(std::vector<PDesc>& v, const std::string& pre, int d_emb, int dff) {
    add(v, pre + "l1.weight", dff, d_emb, true);
    add(v, pre + "l1.bias", dff, 0, true);
    add(v, pre + "l2.weight", d_emb, dff, true);
    add(v, pre + "l2.bias", d_emb, 0, true);
    add(v, pre + "ln.weight", d_emb, 0, true);
    add(v, pre + "ln.bias", d_emb, 0, true);
}

static int check_config(const cf_config& c) {
    // (net.py:277-278 leave d_emb and d_head free; every kernel of this library is written for 128-wide rows -- one MFMA row tile
    //  of 16 x 128 in LDS, eight waves x 16 columns -- so other widths are refused here, by name, instead of failing later)
    // round 5: d_emb = 256 as well, through the stand-alone kernels (row-tile chains, one-sequence attention, layer-by-layer Regulation, the
    // vector-ALU head), which carry the row width as a template parameter; the fused kernels are written for 128-wide rows
    if (c.d_emb != 64 && c.d_emb != 128 && c.d_emb != 256)
        return fail("d_emb = %d is not supported: the HIP path implements d_emb = 128 (the reference's default, net.py:277; every fused kernel) and "
                    "64 / 256 (stand-alone kernels)", c.d_emb);
    if (c.d_emb != 128 && (c.embed_layers != 1 || c.embed_heads > 2 || c.pair_heads > 2))
        return fail("d_emb = %d: one Embedding layer and at most two heads in the Embedding / Pairwise stacks are implemented at this width "
                    "(got embed.n_layers = %d, n_heads = %d / %d)", c.d_emb, c.embed_layers, c.embed_heads, c.pair_heads);
    if (c.d_head < 4 || c.d_head > kHeadGenMaxDH || (c.d_head & 3))
        return fail("d_head = %d is not supported (net.py:278): multiples of 4 in 4..%d (128, the reference's default, runs the matrix-core head "
                    "kernels, other widths a vector-ALU head)", c.d_head, kHeadGenMaxDH);
    if (c.n_feats < 1 || c.n_feats > 8) return fail("n_feats must be in 1..8 (got %d)", c.n_feats);
    if (c.n_out != 1 && c.n_out != 2) return fail("n_out must be 1 or 2");
    if (c.n_res != 3) return fail("exactly 3 resolutions are supported (fc_head is Linear(3*d_emb, .), net.py:327)");
    if (c.i_max < 1 || c.i_max > 16) return fail("i_max must be in 1..16");
    if (c.embed_layers < 1 || c.embed_layers > kMaxEmbedLayers)
        return fail("embed.n_layers must be in 1..%d (got %d); more than one layer runs the all-rows path", kMaxEmbedLayers, c.embed_layers);
    // (heads: 2 is what the fused trunk and the gene-batched attention kernels are written for; 1 and 4 run the stand-alone chain
    //  kernels instantiated for that head count and the one-sequence-per-workgroup attention)
    auto heads_ok = [](int n) { return n == 1 || n == 2 || n == 4; };
    if (!heads_ok(c.embed_heads) || c.embed_dmodel != c.d_emb)
        return fail("embed: n_heads in {1, 2, 4} and d_model = d_emb (net.py:305) are supported (got n_heads = %d, d_model = %d)", c.embed_heads, c.embed_dmodel);
    if (!heads_ok(c.pair_heads) || c.pair_dmodel != c.d_emb)
        return fail("pairwise_interaction: n_heads in {1, 2, 4} and d_model = d_emb = %d are supported -- the Pairwise rows are concatenated with the promoter "
                    "embedding (net.py:361-370), so the two widths must agree (got n_heads = %d, d_model = %d)", c.d_emb, c.pair_heads, c.pair_dmodel);
    if (c.embed_layers > 1 && c.embed_heads != 2)
        return fail("embed: n_layers > 1 (the all-rows path) is implemented for n_heads = 2 only (got n_heads = %d)", c.embed_heads);
    if (c.pair_layers < 1 || 2 * c.pair_layers > kLpMaxSeg) return fail("pairwise_interaction.n_layers must be in 1..%d (got %d)", kLpMaxSeg / 2, c.pair_layers);
    // (the fused Regulation kernels are written for 8 heads x 32; the other shapes run the layer-by-layer kernels, whose attention
    //  stage takes heads and width at run time and whose products are instantiated for both widths)
    // (round 6: the layer-by-layer attention stage, k_attr, takes any head count that divides the width; 1, 2 and 16 are tested beside 4 and 8)
    auto reg_heads_ok = [](int n) { return n == 1 || n == 2 || n == 4 || n == 8 || n == 16; };
    if (!reg_heads_ok(c.reg_heads) || (c.reg_dmodel != 128 && c.reg_dmodel != 256))
        return fail("regulation: n_heads in {1, 2, 4, 8, 16} and d_model in {128, 256} are supported (got n_heads = %d, d_model = %d)", c.reg_heads, c.reg_dmodel);
    if (c.reg_layers < 1 || c.reg_layers > 32) return fail("regulation.n_layers must be in 1..32");
    const int dffs[3] = {c.embed_dff, c.pair_dff, c.reg_dff};
    for (int d : dffs)
        if (d != 128 && d != 256) return fail("d_ff must be 128 or 256 (got %d)", d);
    for (int r = 0; r < c.n_res; ++r)
        if (c.n_bins[r] < 1 || c.n_bins[r] > 1024) return fail("n_bins[%d] must be in 1..1024", r);
    if (c.max_batch < 1 || c.max_batch > 4096) return fail("max_batch must be in 1..4096");
    return 0;
}

static int build_layout(const cf_config& c, std::vector<PDesc>& v, cf_layout& lay) {
    if (check_config(c)) return -1;
    v.clear();
    const int D = c.d_emb;
    for (int r = 0; r < c.n_res; ++r) {
        const std::string pre = fmt("embed.%d.", c.binsizes[r]);
        add(v, pre + "lin_proj.weight", D, c.n_feats, true);
        for (int l = 0; l < c.embed_layers; ++l) {
            const std::string lp = pre + fmt("transformer.layers.%d.", l);
            add_self_att(v, lp + "self_att.", D, c.embed_heads, c.embed_dmodel, false, false);
            add_ffn(v, lp + "ff.", D, c.embed_dff);
        }
    }
    for (int r = 0; r < c.n_res; ++r) {
        const std::string pre = fmt("pairwise_interaction.%d.", c.binsizes[r]);
        add(v, pre + "ln.weight", c.pair_dmodel, 0, false);
        add(v, pre + "ln.bias", c.pair_dmodel, 0, false);
        add(v, pre + "lin_proj_p.weight", c.pair_dmodel, D, true);
        add(v, pre + "lin_proj_pcre.weight", c.pair_dmodel, c.n_feats, true);
        for (int l = 0; l < c.pair_layers; ++l) {
            const std::string lp = pre + fmt("transformer.layers.%d.", l);
            add(v, lp + "self_att.gamma_f", c.pair_heads, 0, false);
            add(v, lp + "self_att.p_att.weight", c.pair_dmodel, c.pair_dmodel, true);
            add(v, lp + "self_att.c_att.weight", 2 * c.pair_dmodel, c.pair_dmodel, true);
            add(v, lp + "self_att.ff.weight", c.pair_dmodel, c.pair_dmodel, true);
            add(v, lp + "self_att.ff.bias", c.pair_dmodel, 0, true);
            add(v, lp + "self_att.ln.weight", c.pair_dmodel, 0, true);
            add(v, lp + "self_att.ln.bias", c.pair_dmodel, 0, true);
            add_ffn(v, lp + "ff.", c.pair_dmodel, c.pair_dff);
        }
    }
    for (int r = 0; r < c.n_res; ++r) {
        const std::string pre = fmt("regulation.%d.", c.binsizes[r]);
        for (int l = 0; l < c.reg_layers; ++l) {
            const std::string lp = pre + fmt("transformer.layers.%d.", l);
            add_self_att(v, lp + "self_att.", D, c.reg_heads, c.reg_dmodel, true, true);
            add_ffn(v, lp + "ff.", D, c.reg_dff);
        }
    }
    add(v, "fc_head.0.weight", c.d_head, 3 * D, true);
    add(v, "fc_head.0.bias", c.d_head, 0, true);
    add(v, "fc_head.2.weight", c.n_out, c.d_head, true);
    add(v, "fc_head.2.bias", c.n_out, 0, true);

    // Offsets: trainable tensors first -- Embedding, Pairwise (state_dict order), then the Regulation layers BELOW reg_layers / 2 of every
    // resolution, then the layers from there up, then fc_head (three adjacent gradient buckets: cf_grad_bucket) --, never-trained ones behind.
    // The TABLE stays in state_dict order; only where a tensor lies in the flat buffers follows the order its gradient becomes complete in.
    const auto group = [&](const PDesc& p) {
        if (!p.trainable) return 4;
        if (p.name.rfind("fc_head.", 0) == 0) return 3;
        if (p.name.rfind("regulation.", 0) != 0) return 0;
        const size_t at = p.name.find(".transformer.layers.");
        const int l = at == std::string::npos ? 0 : atoi(p.name.c_str() + at + 20);
        return l < c.reg_layers / 2 ? 1 : 2;
    };
    long long off = 0, elems = 0;
    for (int pass = 0; pass < 5; ++pass) {
        for (auto& p : v) {
            if (group(p) != pass) continue;
            p.offset = off;
            off += (p.numel + 3) / 4 * 4;     // 16-byte aligned tensors
            elems += p.numel;
        }
        if (pass == 3) lay.n_active = off;
    }
    lay.n_tensors = (int)v.size();
    lay.n_total = off;
    lay.n_elems = elems;
    return 0;
}

// ------------------------------------------------------------------------------------
// handle
// ------------------------------------------------------------------------------------
struct CentreBuf {   // one centre-row attention layer of one resolution
    float *q, *qt, *p, *w, *xbar, *a, *xh1, *rs1, *y1, *hdn, *xh2, *rs2, *out, *xin;
    float *dt2, *dpre1, *dt1, *da, *dxbar, *dqt, *du, *dq, *dx, *partial;
};
struct RegBuf {
    float *qkvg, *p, *a, *xh1, *rs1, *y1, *hdn, *xh2, *rs2;
    float *dt2, *dpre1, *dt1, *da, *dqkvg, *partial, *dgam;
    float *hq, *dy1;
};
struct WsEntry {
    std::string name;
    size_t n, off;
};
// References to the model's parameters, resolved by name ONCE, at cf_bind (resolve_refs): pointers into the bound `params` buffer.
// The tiled, transposed-tiled and gradient views of a tensor lie at the same offset of their buffers (cf_handle::tiled_of / tiledT_of / grad_of).
struct CentreParams {   // weights of one centre-row layer (_t: tiled copies for the forward products)
    const float *wq, *wk, *wv, *wo, *bo, *g1, *be1, *w1, *b1, *w2, *b2, *g2, *be2, *wlp;
    const float *wq_t, *wk_t, *wv_t, *wo_t, *w1_t, *w2_t;
};
struct RegParams {      // one Regulation layer
    const float *watt, *gamma, *wo, *bo, *g1, *be1, *w1, *b1, *w2, *b2, *g2, *be2;
};
struct HeadParams {     // fc_head.0 / fc_head.2
    const float *w1, *b1, *w2, *b2;
};
struct ModelRefs {
    CentreParams E[kMaxRes];                    // Embedding centre-row layer (not with the all-rows Embedding: embed.n_layers > 1)
    std::vector<cf_dense_layer> ED[kMaxRes];    // the Embedding layers as the all-rows path reads them (the model path of n_layers > 1; cf_embed_full)
    const float* lin_proj[kMaxRes];             // embed.<bs>.lin_proj.weight (either Embedding path)
    std::vector<CentreParams> P[kMaxRes];       // Pairwise layers
    const float* lin_proj_p[kMaxRes];
    std::vector<RegParams> R[kMaxRes];          // Regulation layers
    HeadParams head;
};

constexpr int kAttcCapDefault = 64;      // cf_handle::attc_cap unless CF_ATTC_CAP says otherwise; cf_attc_regions(NULL, .) applies it

struct cf_handle {
    cf_config cfg;
    std::vector<PDesc> table;
    std::map<std::string, int> index;    // name -> row of `table` (read by resolve_refs only)
    cf_layout lay;
    float *params = nullptr, *grads = nullptr, *m = nullptr, *v = nullptr;
    ModelRefs refs;                      // where every tensor of the model lies in `params` (cf_bind)
    DevBuf<float> tiled;                 // tiled copy of the Linear weights (forward products), same offsets
    DevBuf<float> tiledT;                // tiled copy of the transposed Regulation weights (backward products), same offsets
    bool reg8 = false;                   // Regulation stack on the 512-thread kernels of cf_reg8.h
    bool reg_row0 = true;                // ... whose last layer computes only what token 0 of its output needs (CF_REG_ROW0=0: all rows, the cross-check)
    bool keep_tiled_ok = false;          // (build_tables: the reduction tiles cover every tensor of that group)
    bool keep_tiled = false;             // cf_keep_tiled: the fused optimiser keeps the Embedding + Pairwise tiled copies fresh, forward passes do not re-tile them
    DevBuf<int> tiled_map;               // [bucket_split / 4]: where each flat float4 of the Embedding + Pairwise range lies in the tiled buffer (k_adamw_tiled)
    bool tiled_pe_fresh = false;         // ... and they ARE fresh (cleared by whatever else writes parameters: cf_bind, cf_params_changed, the separate AdamW launches)
    // Embedding stack over ALL promoter bins (cf_embed_full.h + the dense transformer layer): used by the model path when
    // embed.n_layers > 1 and by cf_embed_full; device buffers outside the arena, allocated on first need
    struct EmbedDense {
        bool ready = false;
        int B = 0;
        float* x[kMaxRes][kMaxEmbedLayers + 1] = {};      // token embeddings / layer outputs [B, L, 128]
        float* ws[kMaxRes][kMaxEmbedLayers] = {};          // dense-layer workspaces (training size)
        float* dy[kMaxRes][3] = {};                        // gradient ping-pong [B, L, 128]
        float* lp_partial[kMaxRes] = {};
        uint8_t* valid[kMaxRes] = {};
        float* tables = nullptr;                           // 4 MiB of tile tables for the backward pass
        std::vector<DevBuf<float>> owned;                  // the allocations the pointers above point into, one each
    } ed;
    bool embed_dense = false;            // the training path goes through it (embed.n_layers > 1)
    DevBuf<RetileUnit> retile_units;
    int n_retile = 0, n_retile_early = 0;      // all units | the leading ones a forward pass needs at once (Embedding + Pairwise)
    DevBuf<TrunkResDev> trunk_tab;             // fused centre-row trunk (cf_trunk.h): device table, one entry per resolution
    bool trunk = false;                        // the Embedding + Pairwise stage runs as k_trunk_fwd / k_trunk_bwd (CF_TRUNK=0: the stand-alone kernels)
    size_t trunk_smem_bytes = 0;
    bool head_deferred = false;                // cf_forward(save = 2) left the head to cf_backward_part (k_head_train)
    bool head_done = false;                    // cf_forward_train ran head forward + loss + head backward at the tail of the Regulation launch
    bool head_loss_due = false;                // ... and the mean loss is still to be summed (by the Regulation backward launch)
    bool pend_record = false;                  // cf_record_step_bwd: the step log rides in the trunk's backward launch
    RecordArgs pend_rec;
    bool pend_gnext = false;                   // cf_gather_batch_next: the NEXT step's gather rides in this step's reduction launch (cf_reduce_opt_part)
    GatherArgs pend_gn;
    int pend_gn_n = 0;
    int* adv_next = nullptr;                   // a batch gathered without advancing the cursor: the next forward pass advances it (trunk launch)
    bool pend_gather = false;                  // cf_gather_batch_fwd: the gather of the step shares a launch with the next forward's prologue
    const void* pend_key = nullptr;            // the batch (its first feature array) the pending gather / cursor advance above belongs to: a forward
                                               // pass over ANOTHER batch (validation between two steps of a fed epoch) must not consume them
    GatherArgs pend_ga;
    int pend_ga_n = 0;
    bool x0_fwd = false;                       // the last saving forward was cf_forward_train_x0: the trunk kept no activations, cf_backward_part(parts & 4) refuses
    bool pend_x0 = false;                      // cf_x0_gather_fwd: the cache gather of the step shares a launch with the prologue of the next cf_forward_train_x0
    X0GatherArgs pend_x0_ga;
    bool head_ride = true;                     // CF_HEAD_RIDE=0 (read at cf_create): the head stays a launch of its own (k_head_train)
    HeadRide ride;
    int* head_cnt = nullptr;
    unsigned long long ride_launches = 0;      // launches that added to head_cnt since it was last zero (ride_tick)
    unsigned long long ride_reset_every = 1ull << 28;
    std::vector<hipStream_t> ride_streams;     // every stream a head-ride launch of this handle was issued on (ride_tick orders its reset against all of them)
    hipEvent_t ride_ev = nullptr;
    float* deferred_logits_user = nullptr;
    // riders of the next k_trunk_bwd launch (cf_rider_arm): leading Regulation weight-gradient tiles with AdamW in their epilogues
    struct Rider {
        bool armed = false;
        int max_tiles = 0, done = 0;           // done: tiles the last trunk launch took (the reduction call that follows skips them)
        long long step = -1;
        AdamFuse o;
    } rider;
    int xcd_reduce = 0;                        // XCD-aware order of the weight-gradient tiles (measured slower: cf_kernels.h, xcd_tile)
    int xcd_reduce_opt = 0;                    // ... in the fused reduction + AdamW launch it paid in round 3 (0.568 -> 0.563 ms); on the round-6 kernels (riders with
                                               // cached accesses) the table order wins: 0.5012 -> 0.4892 ms (profiles/r06n_env_ab.txt); CF_XCD_REDUCE=1 forces it on
    int defer_retile = 1;                      // Regulation + head units ride in the Embedding layer's chain launch (CF_DEFER_RETILE=0: all in the prologue)
    // workspace
    DevBuf<float> arena;
    size_t arena_floats = 0;
    std::vector<WsEntry> ws;
    std::map<std::string, int> ws_index;
    std::string ws_names;
    bool planning = true;
    // stage buffers
    float *pe[kMaxRes], *pet[kMaxRes];
    float *pe2[kMaxRes], *pet2[kMaxRes];      // padded layouts of the gene-batched attention kernel (cf_attc2.h)
    bool attc2 = false;
    bool attc1 = true;                        // one-region launches on the vector-ALU kernel (CF_ATTC1=0: k_attc2<., 1>)
    int attc_cap = kAttcCapDefault;           // most workgroups per resolution for which attc2 trades regions per workgroup for parallelism
    int xcd_map = 1;                          // XCD-aware placement of the Regulation workgroups (CF_XCD_MAP=0 turns it off)
    int n_wg_r = 0, n_cs_r = 0;               // leading entries of wg_tiles / cs_tiles that belong to the Regulation + head bucket
    long long bucket_split = 0;               // flat offset of the first Regulation parameter (bucket boundary)
    long long bucket_split_hi = 0;            // ... of the first parameter of the upper Regulation layers (CF_BUCKET_REG_HI = [this, n_active))
    int n_wg_hi = 0, n_cs_hi = 0;             // tiles of CF_BUCKET_REG_HI at the front of the tables
    int n_wg_short = 0;                       // ... and, at the front of those, the SHORT ones (64 reduction rows: the head's, the last Regulation layer's one-row gradients)
    float *featc[kMaxRes], *ex0[kMaxRes], *edx0[kMaxRes], *edout[kMaxRes];
    CentreBuf E[kMaxRes];
    float *xp0[kMaxRes], *dxp0[kMaxRes], *resid[kMaxRes];
    std::vector<CentreBuf> P[kMaxRes];
    std::vector<float*> Rx[kMaxRes], dRx[kMaxRes];
    std::vector<RegBuf> R[kMaxRes];
    float *hin, *h1, *logits, *dlogits, *dh1, *dhin, *loss, *loss_part, *tdbg;
    // input gradients (cf_backward_from_inputs)
    float* dfreq_part = nullptr;               // [n_res][max_batch][T * T]: d(interaction_freq) per resolution, summed by k_dfreq_sum
    bool reg_dfreq_ok = false;                 // k_reg8_bwd_dfreq got its LDS attribute
    bool ig_smem_ok = false;                   // k_input_grad got its LDS attribute (first use)
    // The chunk workspace of the attribution entry points (attrib_ws, cf_api_attrib.h), allocated by the first call that needs it: a
    // chunk is at most max_batch rows (gene-variants) that run through the model as one batch.  One allocation, `mem`; float
    // segments are promoter_feats[r], pcre_feats[r], interaction_freq (cf_ig.h).
    struct AttribWs {
        DevBuf<float> mem;
        float* row[kIgSegs] = {};              // [max_batch, len]: the chunk's float inputs
        float* grad[kIgSegs] = {};             // [max_batch, len]: their per-row gradients
        uint8_t* pmask[kMaxRes] = {};          // [max_batch, L]: promoter pad-mask centre rows ([max_batch, L, L] with the all-rows Embedding)
        uint8_t* cmask[kMaxRes] = {};          // [max_batch * i_max, L]: pCRE pad-mask centre rows
        uint8_t* imask[kMaxRes] = {};          // [max_batch, T, T]: interaction masks
        float* stash[kMaxRes] = {};            // [max_batch, T, d_emb]: the trunk's output Rx[r][0] of the call's genes
        float* logits = nullptr;               // [max_batch, n_out]: the chunk's logits
        float* slice_sums = nullptr;           // [max_batch, kIgSlices]: per-slice sums of a gene's attributions (k_ig_delta)
        const unsigned* deletion_words = nullptr;      // [i_max + 2]: the coalition words of cf_pcre_ablation's variants, written once
        DevBuf<unsigned> words;                // the 32-bit table of a call: coalition words | quadrature nodes, then weights | mark sets | mark-coalition words, then player words (the sampled game: then the inverse permutations, bytes; sampled interactions: then the column table; back-selection: then the current coalitions, the per-gene candidate words and s_b); grows on demand
        DevBuf<float> own_rows;                // [max_batch, per, n_out]: the rows of a Shapley / epistasis call without a caller's buffer; grows on demand
        DevBuf<float> slot_rows;               // [n_res][B * (V - 1), d_emb]: the changed Regulation input row of every variant of one pCRE slot (scan), or with V - 1 = C of every candidate of a transplant screen; grows on demand
    } aw;
    bool ig_trunk_once = true;                 // frequency-only IG runs the trunk once (CF_IG_TRUNK_ONCE=0 at cf_create: the general path, for A/B checks)
    bool scan_pack = true;                     // pCRE variants run slot-packed (CF_SCAN_PACK=0 at cf_create: the per-region path, for A/B checks)
    // deferred-gradient tile tables
    DevBuf<WgTile> wg_tiles;
    int n_wg = 0;
    DevBuf<CsTile> cs_tiles;
    int n_cs = 0;
    DevBuf<LpJob> lp_jobs;
    int n_lp = 0;
    DevBuf<RegLayerDev> reg_tab;         // fused Regulation stack (one workgroup per gene), when it fits in LDS
    bool reg_fused = false;
    float *lp_part_e[kMaxRes], *lp_part_p[kMaxRes];
    int last_fwd_B = 0;
    int n_fwd = 0, n_bwd = 0, n_opt = 0;
    int n_cu = 256;                     // hipDeviceAttributeMultiprocessorCount of the device the handle was created on
    double wg_flops_per_gene = 0.0;     // 2*M*N*K summed over the weight-gradient jobs, per gene
    // optional HIP-event timing of one of the eagerly launched kernels
    std::string timed;
    std::vector<hipEvent_t> ev;
    size_t ev_used = 0;
    // captured launch sequences
    bool capturing = false;

    // A captured sequence is replayed as [graph piece 1] -> [the timed kernel, launched eagerly between two HIP
    // events] -> [graph piece 2] when it contains the kernel selected with cf_timing_select (event-record nodes
    // inside a graph cost ~60 us per replay on this runtime, an eager launch between two graphs costs nothing
    // measurable), and as one graph otherwise.
    struct Hole {
        const void* func = nullptr;
        dim3 grid, block;
        size_t smem = 0;
        RegArgs args;
    };
    struct Replay {
        hipGraphExec_t first = nullptr, second = nullptr;
        bool has_hole = false;
        Hole hole;
        // launch accounting of the captured sequence (cf_launch_counts must describe ONE step under replay as well): the forward
        // launches it holds (-1: none), whether it starts a backward pass (head: the per-step counters restart), the backward launches it holds
        int n_fwd = -1, n_bwd = 0;
        bool starts_bwd = false;
        bool x0_fwd = false;       // the forward it holds is cf_forward_train_x0
    };
    std::vector<Replay> replays;
    Replay cap;                    // under construction

    cf_handle() = default;
    cf_handle(const cf_handle&) = delete;
    cf_handle& operator=(const cf_handle&) = delete;
    ~cf_handle() {      // (the DevBuf members free the device memory)
        for (Replay& rp : replays) {
            if (rp.first) (void)hipGraphExecDestroy(rp.first);
            if (rp.second) (void)hipGraphExecDestroy(rp.second);
        }
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
        if (ride_ev) (void)hipEventDestroy(ride_ev);
    }

    void time_mark(const char* name, hipStream_t st) {
        if (timed.empty() || capturing || timed != name) return;
        if (ev_used >= 16384) return;      // nobody is reading: stop recording rather than grow without bound
        if (ev_used == ev.size()) {
            hipEvent_t e;
            if (hipEventCreate(&e) != hipSuccess) return;
            ev.push_back(e);
        }
        (void)hipEventRecord(ev[ev_used++], st);
    }

    float* ws_get(const std::string& name, size_t n) {
        n = (n + 3) / 4 * 4;
        if (planning) {
            ws_index[name] = (int)ws.size();
            ws.push_back(WsEntry{name, n, arena_floats});
            arena_floats += n;
            return nullptr;
        }
        const WsEntry& e = ws[ws_index.at(name)];
        return arena + e.off;
    }
    // the other views of a parameter reference `p` (a pointer into `params`): same offset in every flat buffer
    const float* tiled_of(const float* p) const { return tiled + (p - params); }
    const float* tiledT_of(const float* p) const { return tiledT + (p - params); }
    float* grad_of(const float* p) const { return grads + (p - params); }      // (callers have checked that a gradient buffer is bound)
};

static void plan_centre(cf_handle* h, CentreBuf& b, const std::string& pre, size_t N, int L, int dff, bool own_out, bool own_xin, int nh) {
    const size_t kD = h->cfg.d_emb;      // (row width: shadows cf::kD in this function)
    const size_t tiles = (N + kTile - 1) / kTile;
    b.q = h->ws_get(pre + "q", N * kD);
    b.qt = h->ws_get(pre + "qt", N * nh * kD);
    b.p = h->ws_get(pre + "p", N * nh * L);
    b.w = h->ws_get(pre + "w", N * nh * 8);
    b.xbar = h->ws_get(pre + "xbar", N * nh * kD);
    b.a = h->ws_get(pre + "a", N * kD);
    b.xh1 = h->ws_get(pre + "xh1", N * kD);
    b.rs1 = h->ws_get(pre + "rs1", N);
    b.y1 = h->ws_get(pre + "y1", N * kD);
    b.hdn = h->ws_get(pre + "hdn", N * dff);
    b.xh2 = h->ws_get(pre + "xh2", N * kD);
    b.rs2 = h->ws_get(pre + "rs2", N);
    b.out = own_out ? h->ws_get(pre + "out", N * kD) : nullptr;
    b.xin = own_xin ? h->ws_get(pre + "xin", N * kD) : nullptr;
    const std::string d = "d" + pre;
    b.dt2 = h->ws_get(d + "t2", N * kD);
    b.dpre1 = h->ws_get(d + "pre1", N * dff);
    b.dt1 = h->ws_get(d + "t1", N * kD);
    b.da = h->ws_get(d + "a", N * kD);
    b.dxbar = h->ws_get(d + "xbar", N * nh * kD);
    b.dqt = h->ws_get(d + "qt", N * nh * kD);
    b.du = h->ws_get(d + "u", N * nh * 8);
    b.dq = h->ws_get(d + "q", N * kD);
    b.dx = h->ws_get(d + "x", N * kD);
    b.partial = h->ws_get(d + "partial", std::max(tiles, (size_t)h->cfg.max_batch) * post_partial_width(dff, (int)kD));      // (the fused trunk writes one row per gene)
}

// executed twice: once to size the arena, once to hand out pointers
static void plan_workspace(cf_handle* h) {
    const cf_config& c = h->cfg;
    const size_t kD = c.d_emb;      // (row width: shadows cf::kD in this function)
    const size_t MB = c.max_batch, S = c.i_max, T = S + 1;
    const size_t NE = MB, NP = MB * S, NR = MB * T;
    for (int r = 0; r < c.n_res; ++r) {
        const int L = c.n_bins[r];
        h->pe[r] = h->ws_get(fmt("pe%d", r), (size_t)L * kD);
        h->pet[r] = h->ws_get(fmt("pet%d", r), (size_t)L * kD);
        h->pe2[r] = h->ws_get(fmt("pe2_%d", r), (size_t)attc2_lpad(L) * kD);
        h->pet2[r] = h->ws_get(fmt("pet2_%d", r), (size_t)kD * attc2_lt(L));
        h->featc[r] = h->ws_get(fmt("E%d.featc", r), NE * 8);
        h->lp_part_e[r] = h->ws_get(fmt("dE%d.lp_partial", r), ((MB + kLpGenes - 1) / kLpGenes) * kD * 8);
        h->lp_part_p[r] = h->ws_get(fmt("dP%d.lp_partial", r), ((MB + kLpGenes - 1) / kLpGenes) * kD * 8);
        h->ex0[r] = h->ws_get(fmt("E%d.x0", r), NE * kD);
        plan_centre(h, h->E[r], fmt("E%d.", r), NE, L, c.embed_dff, false, false, c.embed_heads);
        h->edout[r] = h->ws_get(fmt("dE%d.out", r), NE * kD);
        h->xp0[r] = h->ws_get(fmt("P%d.xp0", r), NE * kD);
        h->dxp0[r] = h->ws_get(fmt("dP%d.xp0", r), NE * kD);
        h->resid[r] = h->ws_get(fmt("dE%d.resid", r), NE * kD);
        h->P[r].resize(c.pair_layers);
        for (int l = 0; l < c.pair_layers; ++l)
            plan_centre(h, h->P[r][l], fmt("P%d.%d.", r, l), NP, L, c.pair_dff, l + 1 < c.pair_layers, l == 0, c.pair_heads);
        h->Rx[r].resize(c.reg_layers + 1);
        h->dRx[r].resize(c.reg_layers + 1);
        for (int l = 0; l <= c.reg_layers; ++l) {
            h->Rx[r][l] = h->ws_get(fmt("R%d.x%d", r, l), NR * kD);
            h->dRx[r][l] = h->ws_get(fmt("dR%d.x%d", r, l), NR * kD);
        }
        h->R[r].resize(c.reg_layers);
        for (int l = 0; l < c.reg_layers; ++l) {
            RegBuf& b = h->R[r][l];
            const std::string pre = fmt("R%d.%d.", r, l), d = "d" + pre;
            const int dff = c.reg_dff;
            const int RH = c.reg_heads, RDm = c.reg_dmodel, RW = 4 * RDm;
            b.qkvg = h->ws_get(pre + "qkvg", NR * RW);
            b.p = h->ws_get(pre + "p", MB * RH * T * T);
            b.a = h->ws_get(pre + "a", NR * RDm);
            b.xh1 = h->ws_get(pre + "xh1", NR * kD);
            b.rs1 = h->ws_get(pre + "rs1", NR);
            b.y1 = h->ws_get(pre + "y1", NR * kD);
            b.hdn = h->ws_get(pre + "hdn", NR * dff);
            b.xh2 = h->ws_get(pre + "xh2", NR * kD);
            b.rs2 = h->ws_get(pre + "rs2", NR);
            b.dt2 = h->ws_get(d + "t2", NR * kD);
            b.dpre1 = h->ws_get(d + "pre1", NR * dff);
            b.dt1 = h->ws_get(d + "t1", NR * kD);
            b.da = h->ws_get(d + "a", NR * RDm);
            b.dqkvg = h->ws_get(d + "qkvg", NR * RW);
            b.partial = h->ws_get(d + "partial", std::max((NR + kTile - 1) / kTile, MB) * post_partial_width(dff, (int)kD));
            b.dgam = h->ws_get(d + "gam", MB * RH);
            b.hq = h->ws_get(pre + "hq", MB * RH * kHqFloats);
            b.dy1 = h->ws_get(d + "y1", NR * kD);
        }
    }
    h->hin = h->ws_get("H.in", MB * 3 * kD);
    h->h1 = h->ws_get("H.h1", MB * c.d_head);
    h->logits = h->ws_get("H.logits", MB * c.n_out);
    h->dlogits = h->ws_get("dH.logits", MB * c.n_out);
    h->dh1 = h->ws_get("dH.h1", MB * c.d_head);
    h->dhin = h->ws_get("dH.in", MB * 3 * kD);
    h->loss = h->ws_get("H.loss", 4);
    h->loss_part = h->ws_get("H.loss_part", MB + 1);      // (per 16-gene tile; per gene in the generic-width head)
    h->head_cnt = reinterpret_cast<int*>(h->ws_get("H.cnt", MB + 1));      // arrivals per gene (cf_head_ride.h): monotonic, see ride_tick
    h->ride_reset_every = (unsigned long long)std::max(1, getenv_int("CF_RIDE_RESET_EVERY", 1 << 28));
    h->tdbg = h->ws_get("reg_tdbg", 2 * 16 * 64);      // shader-clock stamps (uint64) of the fused Regulation kernels
    h->dfreq_part = h->ws_get("dR.freq", (size_t)c.n_res * MB * T * T);      // (last: the entries above keep their offsets)
}

// ------------------------------------------------------------------------------------
// parameter references (cf_bind): the only place that formats parameter names
// ------------------------------------------------------------------------------------
static int resolve_refs(cf_handle* h) {
    const cf_config& c = h->cfg;
    const size_t D = c.d_emb;
    ModelRefs& m = h->refs;
    std::string missing;
    const auto at = [&](const std::string& name) -> const float* {
        const auto it = h->index.find(name);
        if (it != h->index.end()) return h->params + h->table[it->second].offset;
        if (missing.empty()) missing = name;
        return h->params;
    };
    // the tensors every centre-row layer has; wq / wk / wv / wlp are the caller's (Embedding: thirds of att.weight, Pairwise: p_att | c_att)
    const auto centre = [&](const std::string& lp, const float* wq, const float* wk, const float* wv, const float* wlp) {
        const std::string ap = lp + "self_att.", fp = lp + "ff.";
        CentreParams p;
        p.wq = wq, p.wk = wk, p.wv = wv, p.wlp = wlp;
        p.wo = at(ap + "ff.weight"), p.bo = at(ap + "ff.bias"), p.g1 = at(ap + "ln.weight"), p.be1 = at(ap + "ln.bias");
        p.w1 = at(fp + "l1.weight"), p.b1 = at(fp + "l1.bias"), p.w2 = at(fp + "l2.weight"), p.b2 = at(fp + "l2.bias");
        p.g2 = at(fp + "ln.weight"), p.be2 = at(fp + "ln.bias");
        p.wq_t = h->tiled_of(p.wq), p.wk_t = h->tiled_of(p.wk), p.wv_t = h->tiled_of(p.wv);
        p.wo_t = h->tiled_of(p.wo), p.w1_t = h->tiled_of(p.w1), p.w2_t = h->tiled_of(p.w2);
        return p;
    };
    for (int r = 0; r < c.n_res; ++r) {
        const std::string epre = fmt("embed.%d.", c.binsizes[r]), ppre = fmt("pairwise_interaction.%d.", c.binsizes[r]);
        m.lin_proj[r] = at(epre + "lin_proj.weight");
        m.ED[r].clear();
        for (int l = 0; l < c.embed_layers; ++l) {
            const std::string lp = epre + fmt("transformer.layers.%d.", l);
            const float* att = at(lp + "self_att.att.weight");      // rows [q | k | v] of the fused projection (modules.py:38)
            const CentreParams p = centre(lp, att, att + D * D, att + 2 * D * D, m.lin_proj[r]);
            // (the all-rows path is written for 128-wide rows, cf::kD: its key | value rows start there whatever d_emb is)
            m.ED[r].push_back(cf_dense_layer{p.wq, att + (size_t)kD * kD, p.wo, p.bo, p.g1, p.be1, p.w1, p.b1, p.w2, p.b2, p.g2, p.be2, c.embed_dff});
            if (!h->embed_dense) m.E[r] = p;      // (the one layer of the centre-row path)
        }
        m.lin_proj_p[r] = at(ppre + "lin_proj_p.weight");
        m.P[r].clear();
        for (int l = 0; l < c.pair_layers; ++l) {
            const std::string lp = ppre + fmt("transformer.layers.%d.", l);
            const float* c_att = at(lp + "self_att.c_att.weight");
            m.P[r].push_back(centre(lp, at(lp + "self_att.p_att.weight"), c_att, c_att + D * D, at(ppre + "lin_proj_pcre.weight")));
        }
        m.R[r].clear();
        for (int l = 0; l < c.reg_layers; ++l) {
            const std::string lp = fmt("regulation.%d.transformer.layers.%d.", c.binsizes[r], l), ap = lp + "self_att.", fp = lp + "ff.";
            m.R[r].push_back(RegParams{at(ap + "att.weight"), at(ap + "gamma_f"), at(ap + "ff.weight"), at(ap + "ff.bias"), at(ap + "ln.weight"),
                                       at(ap + "ln.bias"), at(fp + "l1.weight"), at(fp + "l1.bias"), at(fp + "l2.weight"), at(fp + "l2.bias"),
                                       at(fp + "ln.weight"), at(fp + "ln.bias")});
        }
    }
    m.head = HeadParams{at("fc_head.0.weight"), at("fc_head.0.bias"), at("fc_head.2.weight"), at("fc_head.2.bias")};
    if (!missing.empty()) return fail("cf_bind: no parameter '%s'", missing.c_str());
    return 0;
}
