// cf_api.hip -- host side of libchromoformer_hip.so: the C ABI of include/chromoformer_hip.h.  One translation unit: the cf_api_*.h
// headers below hold the handle and parameter layout, the tables built at cf_bind and the launch sequences of the forward and backward
// pass, in the order in which they build on each other.  No torch, no allocation on the hot path.
#include "../../include/chromoformer_hip.h"
#include "cf_kernels.h"
#include "cf_input_grad.h"
#include "cf_attn_maps.h"
#include "cf_rows.h"
#include "cf_coalition.h"
#include "cf_contact.h"
#include "cf_dividends.h"
#include "cf_ig.h"
#include "cf_scan.h"
#include "cf_transplant.h"
#include "cf_marks.h"
#include "cf_scan_fine.h"
#include "cf_marks_wide.h"
#include "cf_mark_pairs.h"
#include "cf_mark_windows.h"
#include "cf_mark_fine.h"
#include "cf_backselect.h"
#include "cf_x0_gather.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

using namespace cf;

#include "cf_api_handle.h"
#include "cf_api_tables.h"
#include "cf_api_feed.h"
#include "cf_api_launch.h"
#include "cf_api_ops.h"
#include "cf_api_fwd.h"
#include "cf_api_bwd.h"
#include "cf_api_attrib.h"
#include "cf_api_contact.h"
#include "cf_api_transplant.h"
#include "cf_api_marks.h"

// ------------------------------------------------------------------------------------
// C ABI: host-only part
// ------------------------------------------------------------------------------------
extern "C" int cf_abi_version(void) { return CF_ABI_VERSION; }
extern "C" const char* cf_last_error(void) { return g_err.c_str(); }

extern "C" int cf_param_layout(const cf_config* cfg, cf_layout* layout, cf_param_desc* table, int cap) {
    if (!cfg || !layout) return fail("cf_param_layout: null argument");
    std::vector<PDesc> v;
    if (build_layout(*cfg, v, *layout)) return -1;
    if (table) {
        if (cap < (int)v.size()) return fail("cf_param_layout: table capacity %d < %d", cap, (int)v.size());
        for (size_t i = 0; i < v.size(); ++i) {
            cf_param_desc& d = table[i];
            memset(&d, 0, sizeof d);
            snprintf(d.name, sizeof d.name, "%s", v[i].name.c_str());
            d.ndim = v[i].ndim;
            d.shape[0] = v[i].shape[0];
            d.shape[1] = v[i].shape[1];
            d.offset = v[i].offset;
            d.numel = v[i].numel;
            d.trainable = v[i].trainable ? 1 : 0;
        }
    }
    return 0;
}

// ------------------------------------------------------------------------------------
// lifetime
// ------------------------------------------------------------------------------------
extern "C" int cf_create(const cf_config* cfg, const float* const* pe_host, cf_handle** out) {
    if (!cfg || !pe_host || !out) return fail("cf_create: null argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail("cf_create: no HIP device visible -- libchromoformer_hip has no CPU fallback");
    std::unique_ptr<cf_handle> owner(new cf_handle());      // (every error return below drops the handle and, through its members, the device memory)
    cf_handle* h = owner.get();
    h->cfg = *cfg;
    {   // compute units of the current device: sizes the rows of rider workgroups that share a launch with one-per-CU workgroups
        int dev = 0, ncu = 0;
        if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && ncu > 0)
            h->n_cu = ncu;
    }
    if (build_layout(h->cfg, h->table, h->lay)) return -1;
    for (size_t i = 0; i < h->table.size(); ++i) h->index[h->table[i].name] = (int)i;
    {   // bucket boundary: trainable tensors are laid out in state_dict order (embed | pairwise | regulation | fc_head)
        long long split = -1, pe_end = 0;
        for (const PDesc& p : h->table) {
            if (!p.trainable) continue;
            const bool late = p.name.rfind("regulation.", 0) == 0 || p.name.rfind("fc_head.", 0) == 0;
            if (late && split < 0) split = p.offset;
            if (!late) pe_end = std::max(pe_end, p.offset + (p.numel + 3) / 4 * 4);
        }
        if (split < 0 || pe_end > split) return fail("cf_create: parameter layout does not split into [embed, pairwise | regulation, head] ranges");
        h->bucket_split = split;
        h->bucket_split_hi = h->lay.n_active;
        for (const PDesc& p : h->table) {
            if (!p.trainable || p.name.rfind("regulation.", 0) != 0) continue;
            const size_t at = p.name.find(".transformer.layers.");
            if (at != std::string::npos && atoi(p.name.c_str() + at + 20) >= h->cfg.reg_layers / 2) h->bucket_split_hi = std::min(h->bucket_split_hi, p.offset);
        }
    }
    {
        // units of the Embedding + Pairwise weights first (needed by the first kernels of a forward pass), Regulation + head behind
        // them (needed ~250 us later: they can ride in a later, under-filled launch, see PostArgs::rt_units)
        std::vector<RetileUnit> units;
        for (int late = 0; late < 2; ++late) {
            for (const PDesc& p : h->table) {
                const bool is_late = p.name.rfind("regulation.", 0) == 0 || p.name.rfind("fc_head.", 0) == 0;
                if (is_late != (late == 1)) continue;
                if (p.ndim == 2 && p.shape[0] % 16 == 0 && p.shape[1] % 16 == 0 && p.trainable)
                    for (int n0 = 0; n0 < p.shape[0]; n0 += 16) units.push_back(RetileUnit{p.offset + (long long)n0 * p.shape[1], p.offset, p.shape[1], p.shape[0], n0,
                                                    p.name.rfind("regulation.", 0) == 0 ? 1 : 0});
            }
            if (late == 0) h->n_retile_early = (int)units.size();
        }
        h->n_retile = (int)units.size();
        const char* who = "cf_create: the tiled weight copies";
        if (h->tiled.alloc(h->lay.n_total, who) || h->tiledT.alloc(h->lay.n_total, who) || h->retile_units.upload(units, who)) return -1;
    }
    h->embed_dense = h->cfg.embed_layers > 1;
    h->planning = true;
    plan_workspace(h);
    if (h->arena.alloc(h->arena_floats, fmt("cf_create: the workspace of %zu bytes", h->arena_floats * sizeof(float)).c_str())) return -1;
    HIP_TRY(hipMemset(h->arena, 0, h->arena_floats * sizeof(float)));
    h->planning = false;
    plan_workspace(h);
    for (const auto& en : h->ws) h->ws_names += en.name + "\n";
    for (int r = 0; r < h->cfg.n_res; ++r) {
        const int L = h->cfg.n_bins[r];
        const int kD = h->cfg.d_emb;      // (row width of the positional table: shadows cf::kD here)
        h->edx0[r] = h->E[r].dx;
        std::vector<float> t((size_t)L * kD);
        for (int j = 0; j < L; ++j)
            for (int d = 0; d < kD; ++d) t[(size_t)d * L + j] = pe_host[r][(size_t)j * kD + d];
        std::vector<float> t2((size_t)kD * attc2_lt(L), 0.f);
        for (int j = 0; j < L; ++j)
            for (int d = 0; d < kD; ++d) t2[(size_t)d * attc2_lt(L) + j] = pe_host[r][(size_t)j * kD + d];
        if (hipMemcpy(h->pe2[r], pe_host[r], (size_t)L * kD * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||       // rows >= L stay zero
            hipMemcpy(h->pet2[r], t2.data(), t2.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(h->pe[r], pe_host[r], (size_t)L * kD * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(h->pet[r], t.data(), (size_t)L * kD * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
            return fail("cf_create: positional table upload failed");
    }
    const cf_config& c = h->cfg;
    {   // the fused Regulation kernels need up to ~150 KB of dynamic LDS
        const int T = c.i_max + 1;
        // 512-thread kernels (cf_reg8.h) for the default head count / width and T <= 16 tokens; CF_REG_FUSED=0 runs the stack layer by layer
        // on the stand-alone kernels instead (k_attr + the row-tile chains: what every other shape runs) -- the cross-check implementation
        h->reg_row0 = getenv_int("CF_REG_ROW0", 1) != 0;
        const size_t need = std::max(reg8_fwd_smem(c.reg_dff), reg8_bwd_smem(c.reg_dff));
        h->reg_fused = T <= kTile && need <= 160 * 1024 && c.reg_heads == kRH && c.reg_dmodel == kRDm && c.d_emb == kD && getenv_int("CF_REG_FUSED", 1) != 0;
        if (h->reg_fused) {
            const size_t sf = reg8_fwd_smem(c.reg_dff), sb = reg8_bwd_smem(c.reg_dff);
            hipError_t e1 = hipFuncSetAttribute(reg_kernel(false, c.reg_dff), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sf);
            if (e1 == hipSuccess) e1 = hipFuncSetAttribute(reg_kernel(false, c.reg_dff, false), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sf);
            hipError_t e2 = hipFuncSetAttribute(reg_kernel(true, c.reg_dff), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sb);
            if (e1 != hipSuccess || e2 != hipSuccess) h->reg_fused = false;
            // the interaction-frequency variant of the backward (cf_backward_from_inputs only): same LDS image
            if (h->reg_fused) h->reg_dfreq_ok = hipFuncSetAttribute(reg_kernel_dfreq(c.reg_dff), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sb) == hipSuccess;
        }
        h->reg8 = h->reg_fused;
    }
    {   // gene-batched attention kernel when its LDS image (8 regions of features + 16 score rows) fits
        size_t need = 0;
        for (int r = 0; r < c.n_res; ++r) need = std::max(need, attc2_smem(c.n_bins[r], c.n_feats, kAGMax));
        h->attc2 = need <= 160 * 1024 && c.d_emb == kD;      // (and the default row width: cf_attc1.h / cf_attc2.h are written for 128)
        if (h->attc2) {
            for (int ag = 1; ag <= kAGMax; ag *= 2) {
                size_t nd = 0;
                for (int r = 0; r < c.n_res; ++r) nd = std::max(nd, attc2_smem(c.n_bins[r], c.n_feats, ag));
                hipError_t e1 = hipFuncSetAttribute(attc2_kernel<false>(ag), hipFuncAttributeMaxDynamicSharedMemorySize, (int)nd);
                hipError_t e2 = hipFuncSetAttribute(attc2_kernel<true>(ag), hipFuncAttributeMaxDynamicSharedMemorySize, (int)nd);
                if (e1 != hipSuccess || e2 != hipSuccess) h->attc2 = false;
            }
        }
    }
    if (h->embed_dense && embed_dense_alloc(h)) return -1;      // the training path needs the all-rows buffers: allocate them now, not on the hot path
    if (const char* e = getenv("CF_XCD_MAP")) h->xcd_map = atoi(e) != 0;
    if (const char* e = getenv("CF_ATTC_CAP")) h->attc_cap = atoi(e);
    if (const char* e = getenv("CF_ATTC1")) h->attc1 = atoi(e) != 0;
    h->ig_trunk_once = getenv_int("CF_IG_TRUNK_ONCE", 1) != 0;
    h->scan_pack = getenv_int("CF_SCAN_PACK", 1) != 0;
    if (const char* e = getenv("CF_DEFER_RETILE")) h->defer_retile = atoi(e) != 0;
    if (const char* e = getenv("CF_HEAD_RIDE")) h->head_ride = atoi(e) != 0;
    if (const char* e = getenv("CF_XCD_REDUCE")) h->xcd_reduce = h->xcd_reduce_opt = atoi(e) != 0;
    h->n_fwd = h->n_bwd = h->n_opt = 0;      // counted at the launch sites by the first calls (cf_launch_counts)
    *out = owner.release();
    return 0;
}

extern "C" void cf_destroy(cf_handle* h) { delete h; }

extern "C" int cf_bind(cf_handle* h, float* params, float* grads, float* exp_avg, float* exp_avg_sq) {
    if (!h || !params) return fail("cf_bind: null handle / params");
    h->tiled_pe_fresh = false;
    h->params = params;
    h->grads = grads;
    h->m = exp_avg;
    h->v = exp_avg_sq;
    // (no forward pass on half-filled references or tables: on failure the handle is unbound again, safe to destroy and to bind again)
    if (resolve_refs(h) || build_reg_table(h) || build_trunk_table(h) || (grads && build_tables(h))) {
        h->params = h->grads = h->m = h->v = nullptr;
        return -1;
    }
    return 0;
}

// ------------------------------------------------------------------------------------
// forward and backward entry points
// ------------------------------------------------------------------------------------
extern "C" int cf_forward(cf_handle* h, const cf_batch* bt, float* logits, int save, void* stream) {
    return forward_impl(h, bt, logits, save, stream, nullptr);
}
// Can cf_forward_train run the head at the tail of the Regulation launch?  (512-thread Regulation kernels, three resolutions, the
// default head width; CF_HEAD_RIDE=0 at cf_create switches it off: A/B runs, cross-checks.)
extern "C" int cf_head_rides(cf_handle* h) {
    if (!h) return 0;
    return h->reg_fused && h->cfg.n_res == kMaxRes && h->cfg.d_head == kD && h->cfg.d_emb == kD && h->head_ride ? 1 : 0;
}
// cf_forward(save_for_backward = 2) for a training step whose labels are known at forward time: where cf_head_rides(h), the
// prediction head -- forward, loss, its backward down to the gradient of token 0 of every Regulation output -- runs at the tail of the
// Regulation forward launch, by the last of a gene's three workgroups to finish (cf_head_ride.h), and the cf_backward_part /
// cf_backward call that follows skips the head (its labels / loss arguments are ignored then).  Elsewhere it is cf_forward(save = 2).
// logits: caller's [B, n_out] buffer (may be null); loss_out: one float (may be null); loss_scale as in cf_backward.
extern "C" int cf_forward_train(cf_handle* h, const cf_batch* bt, float* logits, const void* labels, float loss_scale, float* loss_out,
                                void* stream) {
    if (!h) return fail("null handle");
    if (!labels || !cf_head_rides(h)) return forward_impl(h, bt, logits, 2, stream, nullptr);
    if (ride_tick(h, (hipStream_t)stream)) return -1;
    if (!h->grads) return fail("cf_forward_train: no gradient buffer bound");
    HeadRide hd;
    head_ride_args(h, logits, labels, loss_scale, loss_out, hd);
    h->ride = hd;                 // (the backward launch finishes the mean loss)
    return forward_impl(h, bt, logits, 2, stream, &hd);
}

extern "C" int cf_backward_part(cf_handle* h, const cf_batch* bt, const void* labels, float loss_scale, float* loss_out, int parts,
                                void* stream) {
    if (h && (parts & 4) && h->x0_fwd)
        return fail("cf_backward_part: parts & 4 (the Pairwise + Embedding backward) cannot follow cf_forward_train_x0: that forward started at the "
                    "Regulation input and the trunk kept no activations (frozen trunk: run parts 1 | 2 and reduce CF_BUCKET_REG only)");
    if (check_bwd(h, bt, (parts & 1) != 0)) return -1;
    hipStream_t st = (hipStream_t)stream;
    if ((parts & 1) && !labels && !h->head_done) return fail("cf_backward: labels is null");
    const long long launches0 = g_launches;
    if (parts & 1) h->n_bwd = h->n_opt = 0;      // a backward pass starts with the head: its pieces, the bucket reductions and the optimiser launches add up
    const int rc = backward_impl(h, bt, st, parts, labels, loss_scale, loss_out);
    h->n_bwd += (int)(g_launches - launches0);
    if (h->capturing) {
        if (parts & 1) h->cap.starts_bwd = true, h->cap.n_bwd = 0;
        h->cap.n_bwd += (int)(g_launches - launches0);
    }
    return rc;
}

extern "C" int cf_backward_chain(cf_handle* h, const cf_batch* bt, const void* labels, float loss_scale, float* loss_out,
                                 void* stream) {
    return cf_backward_part(h, bt, labels, loss_scale, loss_out, 7, stream);
}

extern "C" int cf_backward_reduce(cf_handle* h, int B, void* stream) {
    if (!h || !h->grads) return fail("cf_backward_reduce: no gradient buffer bound");
    if (B < 1 || B > h->cfg.max_batch) return fail("cf_backward_reduce: bad batch size %d", B);
    const long long launches0 = g_launches;
    const int rc = reduce_impl(h, B, (hipStream_t)stream);
    h->n_bwd += (int)(g_launches - launches0);
    return rc;
}

extern "C" int cf_backward_reduce_part(cf_handle* h, int B, int buckets, void* stream) {
    if (!h || !h->grads) return fail("cf_backward_reduce_part: no gradient buffer bound");
    if (B < 1 || B > h->cfg.max_batch) return fail("cf_backward_reduce_part: bad batch size %d", B);
    if (buckets & ~(CF_BUCKET_REG | CF_BUCKET_PE | CF_BUCKET_REG_HI | CF_BUCKET_REG_LO)) return fail("cf_backward_reduce_part: bad bucket mask %d", buckets);
    if ((buckets & (CF_BUCKET_REG_HI | CF_BUCKET_REG_LO)) && !(buckets & CF_BUCKET_REG) && !cf_reg_halves(h))
        return fail("cf_backward_reduce_part: this model's Regulation bucket does not come in halves (cf_reg_halves)");
    const long long launches0 = g_launches;
    const int rc = reduce_impl(h, B, (hipStream_t)stream, buckets);
    h->n_bwd += (int)(g_launches - launches0);
    if (h->capturing) h->cap.n_bwd += (int)(g_launches - launches0);
    return rc;
}

extern "C" int cf_reg_halves(cf_handle* h) { return h && h->reg_fused && h->cfg.reg_layers >= 2 ? h->cfg.reg_layers / 2 : 0; }
extern "C" int cf_grad_bucket(cf_handle* h, int bucket, long long* offset, long long* numel) {
    if (!h || !offset || !numel) return fail("cf_grad_bucket: null argument");
    if (bucket == CF_BUCKET_PE) {
        *offset = 0;
        *numel = h->bucket_split;
    } else if (bucket == CF_BUCKET_REG) {
        *offset = h->bucket_split;
        *numel = h->lay.n_active - h->bucket_split;
    } else if (bucket == CF_BUCKET_REG_HI) {
        *offset = h->bucket_split_hi;
        *numel = h->lay.n_active - h->bucket_split_hi;
    } else if (bucket == CF_BUCKET_REG_LO) {
        *offset = h->bucket_split;
        *numel = h->bucket_split_hi - h->bucket_split;
    } else {
        return fail("cf_grad_bucket: bucket must be CF_BUCKET_PE, CF_BUCKET_REG, CF_BUCKET_REG_HI or CF_BUCKET_REG_LO");
    }
    return 0;
}

extern "C" int cf_backward(cf_handle* h, const cf_batch* bt, const void* labels, float loss_scale, float* loss_out, void* stream) {
    if (cf_backward_chain(h, bt, labels, loss_scale, loss_out, stream)) return -1;
    return reduce_impl(h, bt->B, (hipStream_t)stream);
}

extern "C" int cf_backward_from(cf_handle* h, const cf_batch* bt, const float* dlogits, void* stream) {
    if (check_bwd(h, bt)) return -1;
    if (!dlogits) return fail("cf_backward_from: dlogits is null");
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(h->dlogits, dlogits, (size_t)bt->B * h->cfg.n_out * sizeof(float), hipMemcpyDeviceToDevice, st));
    if (backward_impl(h, bt, st)) return -1;
    return reduce_impl(h, bt->B, st);
}

// cf_backward_from for a frozen trunk: head + Regulation backward and the Regulation + head bucket's reductions only (same launches as the
// corresponding pieces of cf_backward_from: same bits in that range); the Embedding + Pairwise range of the gradient buffer is not written.
extern "C" int cf_backward_from_top(cf_handle* h, const cf_batch* bt, const float* dlogits, void* stream) {
    if (check_bwd(h, bt)) return -1;
    if (!dlogits) return fail("cf_backward_from_top: dlogits is null");
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(h->dlogits, dlogits, (size_t)bt->B * h->cfg.n_out * sizeof(float), hipMemcpyDeviceToDevice, st));
    if (backward_impl(h, bt, st, 3)) return -1;
    return reduce_impl(h, bt->B, st, CF_BUCKET_REG);
}

// ------------------------------------------------------------------------------------
// hipGraph capture of launch sequences (the per-step sequence is static)
// ------------------------------------------------------------------------------------
extern "C" int cf_capture_begin(cf_handle* h, void* stream) {
    if (!h) return fail("null handle");
    if (h->capturing) return fail("cf_capture_begin: already capturing");
    h->cap = cf_handle::Replay();
    HIP_TRY(hipStreamBeginCapture((hipStream_t)stream, hipStreamCaptureModeRelaxed));
    h->capturing = true;
    return 0;
}
extern "C" int cf_capture_end(cf_handle* h, void* stream, int* graph_id) {
    if (!h || !graph_id) return fail("null argument");
    if (!h->capturing) return fail("cf_capture_end: not capturing");
    h->capturing = false;
    hipGraph_t g = nullptr;
    HIP_TRY(hipStreamEndCapture((hipStream_t)stream, &g));
    hipGraphExec_t ge = nullptr;
    hipError_t e = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (e != hipSuccess) return fail("hipGraphInstantiate failed: %s", hipGetErrorString(e));
    if (h->cap.has_hole) h->cap.second = ge;
    else h->cap.first = ge;
    h->replays.push_back(h->cap);
    *graph_id = (int)h->replays.size() - 1;
    return 0;
}
extern "C" int cf_graph_launch(cf_handle* h, int graph_id, void* stream) {
    if (!h || graph_id < 0 || graph_id >= (int)h->replays.size()) return fail("cf_graph_launch: bad graph id %d", graph_id);
    cf_handle::Replay& rp = h->replays[graph_id];
    hipStream_t st = (hipStream_t)stream;
    if (rp.n_fwd >= 0) {
        h->n_fwd = rp.n_fwd;
        h->x0_fwd = rp.x0_fwd;
        h->adv_next = nullptr;      // (a replayed forward pass moves the cursor on by itself if it was captured that way)
        h->pend_key = nullptr;
    }
    if (rp.starts_bwd) h->n_bwd = h->n_opt = 0;
    h->n_bwd += rp.n_bwd;
    if (rp.n_fwd >= 0 && h->head_cnt && ride_tick(h, st)) return -1;      // (a replayed forward pass may hold a head ride: counted as one)
    HIP_TRY(hipGraphLaunch(rp.first, st));
    if (rp.has_hole) {
        void* kargs[] = {&rp.hole.args};
        h->time_mark(h->timed.c_str(), st);
        HIP_TRY(hipLaunchKernel(rp.hole.func, rp.hole.grid, rp.hole.block, kargs, rp.hole.smem, st));
        h->time_mark(h->timed.c_str(), st);
        HIP_TRY(hipGraphLaunch(rp.second, st));
    }
    return 0;
}

// ------------------------------------------------------------------------------------
// HIP-event timing of one eagerly launched kernel ("k_wgrad", "k_colsum", "k_adamw")
// ------------------------------------------------------------------------------------
extern "C" int cf_timing_select(cf_handle* h, const char* kernel) {
    if (!h) return fail("null handle");
    h->timed = kernel ? kernel : "";
    h->ev_used = 0;
    return 0;
}
extern "C" int cf_timing_read(cf_handle* h, float* total_ms, int* count) {
    if (!h || !total_ms || !count) return fail("null argument");
    float tot = 0.f;
    int n = 0;
    for (size_t i = 0; i + 1 < h->ev_used; i += 2) {
        HIP_TRY(hipEventSynchronize(h->ev[i + 1]));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, h->ev[i], h->ev[i + 1]));
        tot += ms;
        ++n;
    }
    h->ev_used = 0;
    *total_ms = tot;
    *count = n;
    return 0;
}
extern "C" double cf_wgrad_flops(cf_handle* h, int B) { return h ? h->wg_flops_per_gene * B : 0.0; }
// Algorithmic flops (2 * MAC, valid rows only -- the dead rows of a 16-row tile are not counted) of one launch.
extern "C" double cf_kernel_flops(cf_handle* h, const char* kernel, int B) {
    if (!h || !kernel) return 0.0;
    const cf_config& c = h->cfg;
    const double kD = c.d_emb;      // (row width: shadows cf::kD in this function)
    const double T = c.i_max + 1, dff = c.reg_dff;
    const std::string k = kernel;
    if (k == "k_wgrad") return h->wg_flops_per_gene * B;
    const double RDm = c.reg_dmodel;
    const double lin_fwd = 2.0 * T * (kD * 4.0 * RDm + RDm * (double)kD + kD * dff + dff * kD);        // q|k|v|g, out-proj, FFN
    const double att_fwd = 2.0 * T * T * RDm * 2.0;                                                    // q k^T and p v
    // With the last layer reduced to what token 0 of its output needs (cf_reg8.h, b_run_row0) that layer's algorithmic work is smaller and is
    // counted as such: keys / values (forward) and the k, v quarters of the input-gradient product (backward) over all T rows, everything else
    // -- q, gate, out-projection, FFN, the attention products -- for ONE row.
    const bool row0 = h->reg_fused && h->reg_row0;
    const double full_layers = c.reg_layers - (row0 ? 1 : 0);
    const double lin_last = 2.0 * (T * kD * 2.0 * RDm + kD * 2.0 * RDm + RDm * (double)kD + kD * dff + dff * kD);
    if (k == "k_reg_fwd") return ((lin_fwd + att_fwd) * full_layers + (row0 ? lin_last + 2.0 * T * RDm * 2.0 : 0.0)) * c.n_res * B;
    if (k == "k_reg_bwd")                                                                              // dX products + p v, dp, dq, dk, dv
        return ((lin_fwd + 2.0 * T * T * RDm * 5.0) * full_layers + (row0 ? lin_last + 2.0 * T * RDm * 5.0 : 0.0)) * c.n_res * B;
    if (k == "k_trunk_fwd" || k == "k_trunk_bwd") {
        // The centre-row trunk of one (gene, resolution): ONE Embedding row and S = i_max Pairwise rows per layer.  Per row and layer the
        // 128-wide products q = x Wq^T, qt[h] = q[h] Wk[h], a[h] = xbar[h] Wv[h]^T, a Wo^T (4 x 128 x 128 MACs), the FFN (2 x 128 x d_ff) and the
        // attention of 2 heads over the L bins of the region in two passes of (128 + F) MACs per bin and head (scores, weighted sum; the key /
        // value projections are absorbed into the query); lin_proj_p on the Embedding row (128 x 128), the
        // Embedding input row (F x 128, forward only).  Backward: the dX product of each of these maps and the attention backward
        // (the same two passes with (dxbar, p) in and (dqt, du) out); weight gradients belong to k_wgrad, riders are not counted.
        const double S = c.i_max, F = c.n_feats, PL = c.pair_layers;
        const bool bwd = k == "k_trunk_bwd";
        double mac = 0.0;
        for (int r = 0; r < c.n_res; ++r) {
            const double L = c.n_bins[r];
            const double row_e = 4.0 * kD * kD + 2.0 * kD * c.embed_dff + kD * kD + (bwd ? 0.0 : F * kD);
            const double row_p = 4.0 * kD * kD + 2.0 * kD * c.pair_dff;
            const double att = 2.0 * 2.0 * L * (kD + F);
            mac += row_e + att + S * PL * (row_p + att);
        }
        return 2.0 * mac * B;
    }
    return 0.0;
}
extern "C" int cf_cu_count(cf_handle* h) { return h ? h->n_cu : 0; }
// What launch_attc (cf_api_launch.h) takes for a launch of n_sequences; h == NULL: the rule with the default cap (host only).
extern "C" int cf_attc_regions(cf_handle* h, int n_sequences) {
    if (!h) return attc2_regions_per_wg(n_sequences, kAttcCapDefault);
    return h->attc2 ? attc2_regions_per_wg(n_sequences, h->attc_cap) : 0;
}

// ------------------------------------------------------------------------------------
// optimiser
// ------------------------------------------------------------------------------------
static int adam_hyper(cf_handle* h, float lr, float beta1, float beta2, float eps, float weight_decay, long long step, AdamHyper& hy) {
    if (!h || !h->params || !h->grads || !h->m || !h->v) return fail("cf_adamw_step: params / grads / moments not bound");
    if (step < 1) return fail("cf_adamw_step: step is 1-based");
    const double bc1 = 1.0 - std::pow((double)beta1, (double)step);
    const double bc2 = 1.0 - std::pow((double)beta2, (double)step);
    hy.decay = (float)(1.0 - (double)lr * (double)weight_decay);
    hy.one_m_b1 = (float)(1.0 - (double)beta1);
    hy.b2 = beta2;
    hy.one_m_b2 = (float)(1.0 - (double)beta2);
    hy.step_size = (float)((double)lr / bc1);
    hy.bc2_sqrt = (float)std::sqrt(bc2);
    hy.eps = eps;
    hy.pad = 0.f;
    return 0;
}
// the buckets are adjacent ranges of the flat buffers: [0, split) = Embedding + Pairwise, [split, n_active) = Regulation + head;
// every tensor starts 16-byte aligned, so both bounds are multiples of 4
static int adam_range(cf_handle* h, int buckets, long long& lo, long long& n4, int& grid) {
    if (!buckets || (buckets & ~(CF_BUCKET_REG | CF_BUCKET_PE | CF_BUCKET_REG_HI | CF_BUCKET_REG_LO))) return fail("cf_adamw_step_part: bad bucket mask %d", buckets);
    if (buckets & CF_BUCKET_REG) buckets |= CF_BUCKET_REG_HI | CF_BUCKET_REG_LO;
    // the buckets lie [PE | REG_LO | REG_HI]: the mask must name an adjacent run of them
    const bool pe = buckets & CF_BUCKET_PE, lo_ = buckets & CF_BUCKET_REG_LO, hi_ = buckets & CF_BUCKET_REG_HI;
    if (pe && hi_ && !lo_) return fail("cf_adamw_step_part: the buckets of mask %d are not adjacent in the flat buffers", buckets);
    lo = pe ? 0 : (lo_ ? h->bucket_split : h->bucket_split_hi);
    const long long hi = hi_ ? h->lay.n_active : (lo_ ? h->bucket_split_hi : h->bucket_split);
    n4 = (hi - lo) / 4;
    grid = (int)std::min<long long>((n4 + 255) / 256, 256 * 8);
    return 0;
}
extern "C" int cf_adamw_step_part(cf_handle* h, float lr, float beta1, float beta2, float eps, float weight_decay, long long step,
                                  int buckets, void* stream) {
    AdamHyper hy;
    long long lo, n4;
    int grid;
    if (adam_hyper(h, lr, beta1, beta2, eps, weight_decay, step, hy) || adam_range(h, buckets, lo, n4, grid)) return -1;
    // cf_keep_tiled: a launch over exactly the Embedding + Pairwise bucket writes the tiled copies of what it steps (k_adamw_tiled); any other
    // range that touches that bucket steps the parameters only and leaves the copies stale
    const bool tiled = h->keep_tiled && h->tiled_map && buckets == CF_BUCKET_PE;
    if (buckets & CF_BUCKET_PE) h->tiled_pe_fresh = tiled;
    h->time_mark("k_adamw", (hipStream_t)stream);
    if (tiled)
        hipLaunchKernelGGL(k_adamw_tiled, dim3(grid), dim3(256), 0, (hipStream_t)stream, h->params + lo, (const float*)h->grads + lo, h->m + lo,
                           h->v + lo, n4, hy.decay, hy.one_m_b1, hy.b2, hy.one_m_b2, hy.step_size, hy.bc2_sqrt, hy.eps, (const int*)h->tiled_map, h->tiled);
    else
        hipLaunchKernelGGL(k_adamw, dim3(grid), dim3(256), 0, (hipStream_t)stream, h->params + lo, (const float*)h->grads + lo, h->m + lo,
                           h->v + lo, n4, hy.decay, hy.one_m_b1, hy.b2, hy.one_m_b2, hy.step_size, hy.bc2_sqrt, hy.eps);
    h->time_mark("k_adamw", (hipStream_t)stream);
    LAUNCH_CHECK("k_adamw");
    h->n_opt += 1;      // (reset when a backward pass starts: the optimiser launches of a step add up)
    return 0;
}
// The deferred gradients of `reduce_buckets` and the AdamW update of `adam_buckets` (disjoint from them, gradients already
// complete) in ONE launch (k_reduce_adamw).
extern "C" int cf_reduce_adamw_part(cf_handle* h, int B, int reduce_buckets, float lr, float beta1, float beta2, float eps, float weight_decay,
                                    long long step, int adam_buckets, void* stream) {
    if (!h || !h->grads) return fail("cf_reduce_adamw_part: no gradient buffer bound");
    if (B < 1 || B > h->cfg.max_batch) return fail("cf_reduce_adamw_part: bad batch size %d", B);
    if (reduce_buckets != CF_BUCKET_PE && reduce_buckets != CF_BUCKET_REG) return fail("cf_reduce_adamw_part: exactly one reduction bucket");
    if (adam_buckets & reduce_buckets) return fail("cf_reduce_adamw_part: the optimiser range overlaps the bucket under reduction");
    if (adam_buckets & CF_BUCKET_PE) h->tiled_pe_fresh = false;
    AdamHyper hy;
    long long lo, n4;
    int agrid;
    if (adam_hyper(h, lr, beta1, beta2, eps, weight_decay, step, hy) || adam_range(h, adam_buckets, lo, n4, agrid)) return -1;
    hipStream_t st = (hipStream_t)stream;
    const long long launches0 = g_launches;
    if ((reduce_buckets & CF_BUCKET_PE) && !h->trunk) {
        hipLaunchKernelGGL(k_wgrad_lp, dim3((B + kLpGenes - 1) / kLpGenes, h->n_lp), dim3(256), 0, st, (const LpJob*)h->lp_jobs, B, h->cfg.d_emb);
        LAUNCH_CHECK("k_wgrad_lp");
    }
    const bool reg = reduce_buckets == CF_BUCKET_REG;
    const int w0 = reg ? 0 : h->n_wg_r, wn = reg ? h->n_wg_r : h->n_wg - h->n_wg_r;
    const int c0 = reg ? 0 : h->n_cs_r, cn = reg ? h->n_cs_r : h->n_cs - h->n_cs_r;
    AdamArgs o{h->params + lo, h->m + lo, h->v + lo, h->grads + lo, n4, hy.decay, hy.one_m_b1, hy.b2, hy.one_m_b2, hy.step_size, hy.bc2_sqrt, hy.eps};
    hipLaunchKernelGGL(k_reduce_adamw, dim3(xcd_grid(wn) + cn + agrid), dim3(256), 0, st, (const WgTile*)h->wg_tiles + w0, wn,
                       (const CsTile*)h->cs_tiles + c0, cn, B, h->xcd_reduce, o);
    LAUNCH_CHECK("k_reduce_adamw");
    h->n_bwd += (int)(g_launches - launches0);
    return 0;
}
// The deferred gradients of ONE bucket and the AdamW update of the same bucket in the epilogues of the reduction tiles
// (k_reduce_opt): single-GPU training, where nothing stands between a gradient element and its update.
extern "C" int cf_reduce_opt_part(cf_handle* h, int B, int bucket, float lr, float beta1, float beta2, float eps, float weight_decay,
                                  long long step, int keep_grads, void* stream) {
    if (!h || !h->grads || !h->params || !h->m || !h->v) return fail("cf_reduce_opt_part: params / grads / moments not bound");
    if (B < 1 || B > h->cfg.max_batch) return fail("cf_reduce_opt_part: bad batch size %d", B);
    if (!bucket || (bucket & ~(CF_BUCKET_REG | CF_BUCKET_PE))) return fail("cf_reduce_opt_part: bad bucket mask %d", bucket);
    if (h->embed_dense) return fail("cf_reduce_opt_part: the all-rows Embedding path (embed n_layers > 1) writes its gradients outside the reduction tables; use cf_backward_reduce_part + cf_adamw_step_part");
    AdamHyper hy;
    if (adam_hyper(h, lr, beta1, beta2, eps, weight_decay, step, hy)) return -1;
    hipStream_t st = (hipStream_t)stream;
    const long long launches0 = g_launches;
    if ((bucket & CF_BUCKET_PE) && !h->trunk) {
        hipLaunchKernelGGL(k_wgrad_lp, dim3((B + kLpGenes - 1) / kLpGenes, h->n_lp), dim3(256), 0, st, (const LpJob*)h->lp_jobs, B, h->cfg.d_emb);
        LAUNCH_CHECK("k_wgrad_lp");
    }
    // the tables hold the Regulation + head bucket's tiles first: one bucket is a prefix / suffix, both are everything
    const bool reg = (bucket & CF_BUCKET_REG) != 0, pe = (bucket & CF_BUCKET_PE) != 0;
    int w0 = reg ? 0 : h->n_wg_r, wn = (reg ? h->n_wg_r : 0) + (pe ? h->n_wg - h->n_wg_r : 0);
    const int c0 = reg ? 0 : h->n_cs_r, cn = (reg ? h->n_cs_r : 0) + (pe ? h->n_cs - h->n_cs_r : 0);
    int2 skip = make_int2(0x7fffffff, 0);
    if (h->rider.done) {       // tiles the riders of the last k_trunk_bwd launch have reduced and stepped already: the window behind the short tiles
        if (!reg || h->rider.step != step) return fail("cf_reduce_opt_part: riders were armed for step %lld of the Regulation + head bucket; this call must finish that step", h->rider.step);
        skip = make_int2(h->n_wg_short, h->rider.done);
        wn -= h->rider.done;
        h->rider.done = 0;
    }
    // cf_keep_tiled: the Embedding + Pairwise bucket's tiles write the tiled copies of the weights they step (their next reader is the next
    // forward pass, which then skips the re-tiling of those tensors)
    AdamFuse o{h->params, h->m, h->v, h->grads, hy.decay, hy.one_m_b1, hy.b2, hy.one_m_b2, hy.step_size, hy.bc2_sqrt, hy.eps, keep_grads ? 1 : 0,
               h->keep_tiled && pe ? h->tiled : nullptr};
    if (h->pend_gnext) {      // the next step's batch gather behind the tiles of this launch (cf_gather_batch_next)
        hipLaunchKernelGGL(k_reduce_opt_gather, dim3(xcd_grid(wn) + cn + h->pend_gn.B * h->pend_gn_n), dim3(256), 0, st, (const WgTile*)h->wg_tiles + w0, wn,
                           (const CsTile*)h->cs_tiles + c0, cn, B, h->xcd_reduce_opt, o, h->pend_gn, skip);
        h->adv_next = h->pend_gn.cursor;
        h->pend_gnext = false;
    } else {
        hipLaunchKernelGGL(k_reduce_opt, dim3(xcd_grid(wn) + cn), dim3(256), 0, st, (const WgTile*)h->wg_tiles + w0, wn, (const CsTile*)h->cs_tiles + c0, B,
                           h->xcd_reduce_opt, o, skip);
    }
    LAUNCH_CHECK("k_reduce_opt");
    if (pe) h->tiled_pe_fresh = h->keep_tiled;      // (every tensor of that bucket with a tiled copy has just been rewritten in both forms -- or in one only)
    h->n_bwd += (int)(g_launches - launches0);
    return 0;
}
// Arms the riders of the NEXT cf_backward_part(parts & 4) call (k_trunk_bwd; cf_trunk.h): up to max_tiles leading weight-gradient
// tiles of the Regulation + head bucket are reduced, with this step's AdamW update in their epilogues, on the CUs the trunk leaves
// idle.  The cf_reduce_opt_part call of the same step (a mask that contains CF_BUCKET_REG) then skips them.
extern "C" int cf_rider_arm(cf_handle* h, float lr, float beta1, float beta2, float eps, float weight_decay, long long step, int keep_grads,
                            int max_tiles) {
    if (!h || !h->grads || !h->params || !h->m || !h->v) return fail("cf_rider_arm: params / grads / moments not bound");
    if (!h->trunk) return fail("cf_rider_arm: the fused trunk kernels are not in use for this configuration");
    if (h->embed_dense) return fail("cf_rider_arm: not with the all-rows Embedding path");
    if (h->rider.done) return fail("cf_rider_arm: the riders of step %lld have not been followed by cf_reduce_opt_part", h->rider.step);
    AdamHyper hy;
    if (adam_hyper(h, lr, beta1, beta2, eps, weight_decay, step, hy)) return -1;
    h->rider.o = AdamFuse{h->params, h->m, h->v, h->grads, hy.decay, hy.one_m_b1, hy.b2, hy.one_m_b2, hy.step_size, hy.bc2_sqrt, hy.eps, keep_grads ? 1 : 0, nullptr};
    h->rider.max_tiles = std::max(0, max_tiles);
    h->rider.step = step;
    h->rider.armed = max_tiles > 0;      // (max_tiles <= 0: disarms; the checks above tell a caller whether riders are available at all)
    return 0;
}
// The fused optimiser (cf_reduce_opt_part over the Embedding + Pairwise bucket) can keep the tiled copies of that bucket's weights fresh: its
// epilogue writes every stepped element in both layouts, and forward passes then skip the re-tiling of those tensors -- the launch in front
// of a training step disappears (or carries only the batch gather).  The caller's side of the contract: whoever else writes parameters --
// a checkpoint load, an in-place edit, another optimiser -- says so with cf_params_changed before the next forward pass (the Python layer
// compares the version counter of its flat parameter tensor; the library's own separate AdamW launches and cf_bind clear the flag
// themselves); the next forward pass then re-tiles once, in a launch of its own.  Not offered (-1) where the reduction tiles do not cover those
// tensors (the all-rows Embedding path).
extern "C" int cf_keep_tiled(cf_handle* h, int on) {
    if (!h) return fail("null handle");
    if (on && !h->keep_tiled_ok) return fail("cf_keep_tiled: not available for this configuration (gradient buffer not bound, or the all-rows Embedding path)");
    h->keep_tiled = on != 0;
    h->tiled_pe_fresh = false;
    return 0;
}
extern "C" int cf_params_changed(cf_handle* h) {
    if (!h) return fail("null handle");
    h->tiled_pe_fresh = false;
    return 0;
}
// the re-tiling a forward pass would do on finding the flag cleared, now (before a hipGraph that was captured without it is replayed)
extern "C" int cf_retile_early(cf_handle* h, void* stream) {
    if (!h || !h->params) return fail("cf_retile_early: no parameters bound");
    return retile_early(h, (hipStream_t)stream);
}
extern "C" int cf_adamw_step(cf_handle* h, float lr, float beta1, float beta2, float eps, float weight_decay, long long step,
                             void* stream) {
    return cf_adamw_step_part(h, lr, beta1, beta2, eps, weight_decay, step, CF_BUCKET_REG | CF_BUCKET_PE, stream);
}

// ------------------------------------------------------------------------------------
// frozen trunk: trunk outputs, the training forward from the Regulation input, the cache gather (cf_x0_gather.h)
// ------------------------------------------------------------------------------------
extern "C" int cf_trunk_outputs(cf_handle* h, const cf_batch* bt, float* const* x0, void* stream) {
    if (!h) return fail("cf_trunk_outputs: null handle");
    if (!bt || !x0) return fail("cf_trunk_outputs: null batch / output table");
    if (check_batch(h, bt)) return -1;
    const float* src[kMaxRes] = {};
    for (int r = 0; r < h->cfg.n_res; ++r) {
        if (!x0[r]) return fail("cf_trunk_outputs: x0[%d] is null", r);
        if ((uintptr_t)x0[r] & 15) return fail("cf_trunk_outputs: x0[%d] is not 16-byte aligned", r);
        src[r] = h->Rx[r][0];
    }
    hipStream_t st = (hipStream_t)stream;
    const long long launches0 = g_launches;
    if (forward_trunk(h, bt, 0, st) || x0_copy(h, bt->B, src, x0, st)) return -1;
    h->x0_fwd = false;
    forward_counted(h, launches0);
    return 0;
}
extern "C" int cf_forward_train_x0(cf_handle* h, const cf_batch* bt, const float* const* x0, float* logits, const void* labels, float loss_scale,
                                   float* loss_out, void* stream) {
    // a pending cf_x0_gather_fwd belongs to THIS call, which consumes it or fails: either way it is gone on return and cannot surface in a
    // later, unrelated call
    struct DropPending {
        cf_handle* h;
        ~DropPending() { if (h) h->pend_x0 = false; }
    } drop{h};
    if (check_batch_x0(h, bt, "cf_forward_train_x0")) return -1;
    if (!h->grads) return fail("cf_forward_train_x0: no gradient buffer bound");
    const cf_config& c = h->cfg;
    hipStream_t st = (hipStream_t)stream;
    const long long launches0 = g_launches;
    const RetileUnit* units = (const RetileUnit*)h->retile_units + h->n_retile_early;      // the Regulation + head weights (the trunk's are not read)
    const int n_units = h->n_retile - h->n_retile_early;
    float* tT = h->reg8 ? h->tiledT : (float*)nullptr;
    if (x0) {
        float* dst[kMaxRes] = {};
        for (int r = 0; r < c.n_res; ++r) {
            if (!x0[r]) return fail("cf_forward_train_x0: x0[%d] is null", r);
            if ((uintptr_t)x0[r] & 15) return fail("cf_forward_train_x0: x0[%d] is not 16-byte aligned", r);
            dst[r] = h->Rx[r][0];
        }
        if (h->pend_x0) return fail("cf_forward_train_x0: a cf_x0_gather_fwd is pending; pass x0 = NULL to take its batch");
        if (x0_copy(h, bt->B, x0, dst, st)) return -1;
    }
    if (h->pend_x0 && h->pend_x0_ga.B != bt->B) return fail("cf_forward_train_x0: the pending cf_x0_gather_fwd holds %d genes, the batch %d", h->pend_x0_ga.B, bt->B);
    if (h->pend_x0) {      // the step's cache gather behind the re-tiling blocks: one launch
        hipLaunchKernelGGL(k_x0_prologue, dim3(n_units + bt->B * h->pend_x0_ga.n_seg), dim3(kX0Threads), 0, st, (const float*)h->params, h->tiled, tT, units, n_units,
                           h->pend_x0_ga);
        LAUNCH_CHECK("k_x0_prologue");
    } else if (n_units > 0) {
        hipLaunchKernelGGL(k_retile, dim3(n_units), dim3(256), 0, st, (const float*)h->params, h->tiled, tT, units);
        LAUNCH_CHECK("k_retile");
    }
    HeadRide hd;
    const bool ride = labels && cf_head_rides(h);
    if (ride) {
        if (ride_tick(h, st)) return -1;
        head_ride_args(h, logits, labels, loss_scale, loss_out, hd);
        h->ride = hd;
    }
    if (forward_reg_head(h, bt, logits, 2, st, ride ? &hd : nullptr)) return -1;
    h->x0_fwd = true;
    h->last_fwd_B = bt->B;
    h->n_fwd = (int)(g_launches - launches0);
    if (h->capturing) h->cap.n_fwd = h->n_fwd, h->cap.x0_fwd = true;
    return 0;
}
extern "C" int cf_reduce_opt_x0(cf_handle* h, int B, float lr, float beta1, float beta2, float eps, float weight_decay, long long step, int keep_grads,
                                int* cursor, void* stream) {
    if (!h || !h->grads || !h->params || !h->m || !h->v) return fail("cf_reduce_opt_x0: params / grads / moments not bound");
    if (B < 1 || B > h->cfg.max_batch) return fail("cf_reduce_opt_x0: bad batch size %d", B);
    if (h->pend_gnext) return fail("cf_reduce_opt_x0: a cf_gather_batch_next is pending; this launch carries no batch gather (a frozen-trunk step gathers with "
                                   "cf_gather_batch_fwd or cf_x0_gather_fwd in front of its forward)");
    if (h->rider.done || h->rider.armed) return fail("cf_reduce_opt_x0: riders are armed (cf_rider_arm); a frozen-trunk step has no trunk backward launch for them");
    AdamHyper hy;
    if (adam_hyper(h, lr, beta1, beta2, eps, weight_decay, step, hy)) return -1;
    hipStream_t st = (hipStream_t)stream;
    // the Regulation + head bucket's tiles lead the tables; nothing of the Embedding + Pairwise range -- parameters, moments, gradients, tiled
    // copies -- is read or written
    const int wn = h->n_wg_r, cn = h->n_cs_r;
    AdamFuse o{h->params, h->m, h->v, h->grads, hy.decay, hy.one_m_b1, hy.b2, hy.one_m_b2, hy.step_size, hy.bc2_sqrt, hy.eps, keep_grads ? 1 : 0, nullptr};
    RecordArgs rec;
    memset(&rec, 0, sizeof rec);
    if (h->pend_record) {      // cf_record_step_bwd: the step log, written here (no trunk backward launch to carry it)
        rec = h->pend_rec;
        h->pend_record = false;
    }
    hipLaunchKernelGGL(k_reduce_opt_x0, dim3(xcd_grid(wn) + cn + 1), dim3(256), 0, st, (const WgTile*)h->wg_tiles, wn, (const CsTile*)h->cs_tiles, cn, B,
                       h->xcd_reduce_opt, o, cursor, rec);
    LAUNCH_CHECK("k_reduce_opt_x0");
    h->n_bwd += 1;
    return 0;
}

// ------------------------------------------------------------------------------------
// introspection
// ------------------------------------------------------------------------------------
extern "C" int cf_debug_copy(cf_handle* h, const char* name, float* dst, long long* n_floats, void* stream) {
    if (!h || !name) return fail("cf_debug_copy: null argument");
    auto it = h->ws_index.find(name);
    if (it == h->ws_index.end()) return fail("cf_debug_copy: no workspace buffer named '%s'", name);
    const WsEntry& e = h->ws[it->second];
    if (n_floats) *n_floats = (long long)e.n;
    if (dst) HIP_TRY(hipMemcpyAsync(dst, h->arena + e.off, e.n * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}
extern "C" const char* cf_debug_names(cf_handle* h) { return h ? h->ws_names.c_str() : ""; }
extern "C" int cf_launch_counts(cf_handle* h, int* fwd, int* bwd, int* opt) {
    if (!h) return fail("null handle");
    if (fwd) *fwd = h->n_fwd;
    if (bwd) *bwd = h->n_bwd;
    if (opt) *opt = h->n_opt;
    return 0;
}
