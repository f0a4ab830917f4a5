// cf_api_ops.h -- the stand-alone operators, the binning entry points and the dense transformer layer (nothing of these touches a
// cf_handle), and behind them the all-rows Embedding path of the model, which runs on the dense layer.
// Part of cf_api.hip's single translation unit: included there behind cf_api_launch.h, not on its own.
#pragma once

// ------------------------------------------------------------------------------------
// standalone operators
// ------------------------------------------------------------------------------------
extern "C" int cf_op_linear(const float* A, const float* W, const float* bias, float* C, int M, int N, int K, int relu, void* stream) {
    if (K % 128 || N % 32) return fail("cf_op_linear: K %% 128 == 0 and N %% 32 == 0 required");
    // standalone use: build the tiled copy of W on the fly (test / micro-benchmark helper, synchronous)
    std::vector<RetileUnit> units;
    for (int n0 = 0; n0 < N; n0 += 16) units.push_back(RetileUnit{(long long)n0 * K, 0, K, N, n0, 0});
    DevBuf<float> Wt;      // (freed on every return; the synchronisation below keeps them alive while the kernels run)
    DevBuf<RetileUnit> du;
    if (Wt.alloc((size_t)N * K, "cf_op_linear") || du.upload(units, "cf_op_linear")) return -1;
    hipLaunchKernelGGL(k_retile, dim3((int)units.size()), dim3(256), 0, (hipStream_t)stream, W, (float*)Wt, (float*)nullptr, (const RetileUnit*)du);
    LinArgs a;
    memset(&a, 0, sizeof a);
    a.x[0] = A;
    a.w[0] = Wt;
    a.b[0] = bias;
    a.y[0] = C;
    a.xmap = identity_map();
    a.ldx = K;
    a.ldy = N;
    a.N = M;
    a.K = K;
    a.Nout = N;
    a.relu = relu;
    hipLaunchKernelGGL((k_linear_fwd<2>), dim3(tiles_of(M), (N + 127) / 128, 1), dim3(256), 0, (hipStream_t)stream, a);
    LAUNCH_CHECK("cf_op_linear");
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return 0;
}
extern "C" int cf_op_dgrad(const float* dY, const float* W, float* dX, int M, int N, int K, void* stream) {
    if ((N != 128 && N != 256 && N != 1024) || K % 32) return fail("cf_op_dgrad: N in {128, 256, 1024} and K %% 32 == 0 required");
    DgradArgs a;
    memset(&a, 0, sizeof a);
    a.dy[0] = dY;
    a.lddy = N;
    a.w[0] = W;
    a.ldw = K;
    a.rmap = identity_map();
    a.dx[0] = dX;
    a.lddx = K;
    a.N = M;
    a.K = N;
    a.Ncols = K;
    const dim3 grid(tiles_of(M), K / 32, 1);
    if (N == 128) hipLaunchKernelGGL((k_dgrad<2>), grid, dim3(256), 0, (hipStream_t)stream, a);
    else if (N == 256) hipLaunchKernelGGL((k_dgrad<4>), grid, dim3(256), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((k_dgrad<16>), grid, dim3(256), 0, (hipStream_t)stream, a);
    LAUNCH_CHECK("cf_op_dgrad");
    return 0;
}
extern "C" int cf_op_wgrad(const float* dY, const float* X, float* dW, int M, int N, int K, void* stream) {
    if (K % 4) return fail("cf_op_wgrad: K %% 4 == 0 required");
    std::vector<WgTile> tiles;
    push_wg(tiles, wg1(dY, N, X, K, M, dW, K, N, K));
    DevBuf<WgTile> d;
    if (d.upload(tiles, "cf_op_wgrad")) return -1;
    hipLaunchKernelGGL(k_wgrad, dim3(xcd_grid((int)tiles.size())), dim3(256), 0, (hipStream_t)stream, (const WgTile*)d, (int)tiles.size(), 1, 0);
    LAUNCH_CHECK("cf_op_wgrad");
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return 0;
}

static int attn_args(const cf_attn_shape* sh, AttnArgs& a) {
    if (!sh) return fail("cf_op_attention: null shape");
    if (sh->N < 1 || sh->H < 1 || sh->Lq < 1 || sh->Lk < 1) return fail("cf_op_attention: bad shape");
    if (sh->N > 65535 || sh->H > 65535) return fail("cf_op_attention: N and H are grid dimensions (<= 65535)");
    if ((sh->ldq | sh->ldk | sh->ldv | sh->ldo) & 3) return fail("cf_op_attention: row strides must be multiples of 4 floats");
    if (sh->ldq < sh->H * kADh || sh->ldk < sh->H * kADh || sh->ldv < sh->H * kADh || sh->ldo < sh->H * kADh)
        return fail("cf_op_attention: row stride smaller than H * 64");
    memset(&a, 0, sizeof a);
    a.N = sh->N;
    a.H = sh->H;
    a.Lq = sh->Lq;
    a.Lk = sh->Lk;
    a.ldq = sh->ldq;
    a.ldk = sh->ldk;
    a.ldv = sh->ldv;
    a.ldo = sh->ldo;
    a.rscale = 1.0f / sqrtf((float)kADh);
    return 0;
}
// The dense attention forward: k_attn_fwd (round 5: transposed score tiles, 128 query rows per workgroup); CF_ATTN_FWD_V1=1 runs the round-1
// kernel (64 rows per workgroup, P through a per-wave LDS patch) -- the cross-check of the tests.  Same results up to the order of the fp32
// additions inside P V.
static int attn_fwd_launch(const AttnArgs& a, hipStream_t st) {
    if (getenv_int("CF_ATTN_FWD_V1", 0)) {
        hipLaunchKernelGGL(k_attn_fwd_v1, dim3((a.Lq + kABq - 1) / kABq, a.H, a.N), dim3(256), 0, st, a);
        LAUNCH_CHECK("k_attn_fwd_v1");
        return 0;
    }
    const dim3 grid((a.Lq + kABq2 - 1) / kABq2, a.H, a.N);
    if (a.mask) hipLaunchKernelGGL(k_attn_fwd<true>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_attn_fwd<false>, grid, dim3(256), 0, st, a);
    LAUNCH_CHECK("k_attn_fwd");
    return 0;
}
extern "C" int cf_op_attention_fwd(const cf_attn_shape* sh, const float* q, const float* k, const float* v, const unsigned char* qvalid,
                                   const unsigned char* kvalid, const unsigned char* mask, float* o, float* stats, void* stream) {
    AttnArgs a;
    if (attn_args(sh, a)) return -1;
    if (!q || !k || !v || !o) return fail("cf_op_attention_fwd: null tensor");
    a.q = q;
    a.k = k;
    a.v = v;
    a.qvalid = qvalid;
    a.kvalid = kvalid;
    a.mask = mask;
    a.o = o;
    a.stats = stats;
    if (attn_fwd_launch(a, (hipStream_t)stream)) return -1;
    return 0;
}
// dQ, dK, dV of the dense attention core (delta = rowsum(dO * O) is in a.delta already).  One fused pass per (sequence, head)
// (k_attn_bwd: 5 tile products per key / query tile pair) when the launch has enough (sequence, head) workgroups to fill the chip;
// otherwise the two kernels split by output owner (7 products per pair, but (Lk / 64 + Lq / 64) workgroups per sequence and head).
// CF_ATTN_BWD_SPLIT=1 forces the split kernels, -1 the fused one (A/B runs, cross-checks in the tests; read at every call).  Same
// results either way up to the order of the fp32 additions inside dQ.
static int attn_bwd_launch(const AttnArgs& a, hipStream_t st) {
    const int mode = getenv_int("CF_ATTN_BWD_SPLIT", 0);
    const bool vec_ok = (a.ldq & 3) == 0 && (reinterpret_cast<uintptr_t>(a.dq) & 15) == 0;      // (the dQ update is 16 bytes per lane)
    if (vec_ok && (mode < 0 || (mode == 0 && (long long)a.N * a.H >= 512))) {
        // round 6: 128 keys per pass, eight waves, 141 KB of dynamic LDS (k_attn_bwd2); CF_ATTN_BWD_V1=1 runs the 64-key kernel of rounds 4-5 (the
        // cross-check of the tests: same results up to the order of the fp32 additions inside dQ)
        const bool v2_ok = ((reinterpret_cast<uintptr_t>(a.dk) | reinterpret_cast<uintptr_t>(a.dv)) & 15) == 0 && getenv_int("CF_ATTN_BWD_V1", 0) == 0;
        if (v2_ok) {
            static int ready = 0;      // 0: not tried, 1: attribute set, -1: refused by the runtime (fall through to the 64-key kernel)
            if (ready == 0) {
                hipError_t e1 = hipFuncSetAttribute(reinterpret_cast<const void*>(k_attn_bwd2<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kAB2Smem);
                hipError_t e2 = hipFuncSetAttribute(reinterpret_cast<const void*>(k_attn_bwd2<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kAB2Smem);
                ready = (e1 == hipSuccess && e2 == hipSuccess) ? 1 : -1;
                if (ready < 0) (void)hipGetLastError();
            }
            if (ready > 0) {
                if (a.mask) hipLaunchKernelGGL(k_attn_bwd2<true>, dim3(a.H, a.N), dim3(512), kAB2Smem, st, a);
                else hipLaunchKernelGGL(k_attn_bwd2<false>, dim3(a.H, a.N), dim3(512), kAB2Smem, st, a);
                LAUNCH_CHECK("k_attn_bwd2");
                return 0;
            }
        }
        hipLaunchKernelGGL(k_attn_bwd, dim3(a.H, a.N), dim3(256), 0, st, a);
        LAUNCH_CHECK("k_attn_bwd");
        return 0;
    }
    hipLaunchKernelGGL(k_attn_bwd_kv, dim3((a.Lk + kABk - 1) / kABk, a.H, a.N), dim3(256), 0, st, a);
    LAUNCH_CHECK("k_attn_bwd_kv");
    hipLaunchKernelGGL(k_attn_bwd_q, dim3((a.Lq + kABq - 1) / kABq, a.H, a.N), dim3(256), 0, st, a);
    LAUNCH_CHECK("k_attn_bwd_q");
    return 0;
}
extern "C" int cf_op_attention_bwd(const cf_attn_shape* sh, const float* q, const float* k, const float* v, const unsigned char* qvalid,
                                   const unsigned char* kvalid, const unsigned char* mask, const float* o, const float* stats,
                                   const float* d_o, float* dq, float* dk, float* dv, float* delta_ws, void* stream) {
    AttnArgs a;
    if (attn_args(sh, a)) return -1;
    if (!q || !k || !v || !o || !stats || !d_o || !dq || !dk || !dv || !delta_ws) return fail("cf_op_attention_bwd: null tensor");
    a.q = q;
    a.k = k;
    a.v = v;
    a.qvalid = qvalid;
    a.kvalid = kvalid;
    a.mask = mask;
    a.o = const_cast<float*>(o);
    a.stats = const_cast<float*>(stats);
    a.d_o = d_o;
    a.dq = dq;
    a.dk = dk;
    a.dv = dv;
    a.delta = delta_ws;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_attn_delta, dim3((a.Lq + 15) / 16, a.H, a.N), dim3(256), 0, st, a);
    LAUNCH_CHECK("k_attn_delta");
    if (attn_bwd_launch(a, st)) return -1;
    return 0;
}

static_assert(sizeof(cf_bin_job) == sizeof(BinJob), "cf_bin_job layout");
extern "C" int cf_bin_regions(const cf_bin_job* jobs, int n_jobs, int n_feats, int bin_size, int n_bins_out, void* stream) {
    if (!jobs) return fail("cf_bin_regions: null job table");
    if (n_jobs < 0 || n_feats < 1 || n_feats > 64 || bin_size < 1 || n_bins_out < 1) return fail("cf_bin_regions: bad argument");
    if (n_jobs == 0) return 0;
    hipLaunchKernelGGL(k_bin_regions, dim3(n_jobs), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const BinJob*>(jobs), n_feats,
                       bin_size, n_bins_out);
    LAUNCH_CHECK("k_bin_regions");
    return 0;
}

static_assert(sizeof(cf_bin_job_multi) == sizeof(BinJobMulti), "cf_bin_job_multi layout");
extern "C" int cf_bin_regions_multi(const cf_bin_job_multi* jobs, int n_jobs, int n_feats, int n_res, const int* bin_sizes, const int* n_bins_out,
                                    int max_cols, void* stream) {
    if (!jobs || !bin_sizes || !n_bins_out) return fail("cf_bin_regions_multi: null argument");
    if (n_jobs < 0 || n_feats < 1 || n_feats > 64 || n_res < 1 || n_res > kBinMaxRes || max_cols < 0) return fail("cf_bin_regions_multi: bad argument");
    if (n_jobs == 0) return 0;
    BinPlan pl;
    memset(&pl, 0, sizeof pl);
    pl.n_res = n_res;
    pl.F = n_feats;
    for (int r = 0; r < n_res; ++r) {
        if (bin_sizes[r] < 1 || n_bins_out[r] < 1 || n_bins_out[r] > kBinMaxBins) return fail("cf_bin_regions_multi: bad bin size / bin count at resolution %d", r);
        if (r && bin_sizes[r] >= bin_sizes[r - 1]) return fail("cf_bin_regions_multi: bin sizes must be listed coarsest first (%d after %d)", bin_sizes[r], bin_sizes[r - 1]);
        pl.b[r] = bin_sizes[r];
        pl.L[r] = n_bins_out[r];
    }
    // one pass over the raw bytes when the bins nest and a unit (one coarsest bin) fits a wave's registers and lanes
    bool nested = n_res >= 2 && n_feats <= kBinMaxF && (pl.b[n_res - 1] & 3) == 0 && pl.b[0] <= kBinMaxLoads * 256 && pl.b[0] / pl.b[n_res - 1] <= 64;
    for (int r = 0; r + 1 < n_res; ++r) nested = nested && pl.b[r] % pl.b[r + 1] == 0;
    pl.nested = nested ? 1 : 0;
    const int units = nested ? std::max(1, (max_cols + pl.b[0] - 1) / pl.b[0]) : 1;
    const dim3 grid((units + 3) / 4, n_jobs);
    const int nload = nested ? (pl.b[0] / 4 + 63) / 64 : 4;
    const BinJobMulti* jm = reinterpret_cast<const BinJobMulti*>(jobs);
    if (nload <= 4) hipLaunchKernelGGL(k_bin_multi<4>, grid, dim3(256), 0, (hipStream_t)stream, jm, pl);
    else if (nload <= 8) hipLaunchKernelGGL(k_bin_multi<8>, grid, dim3(256), 0, (hipStream_t)stream, jm, pl);
    else hipLaunchKernelGGL(k_bin_multi<16>, grid, dim3(256), 0, (hipStream_t)stream, jm, pl);
    LAUNCH_CHECK("k_bin_multi");
    return 0;
}

static_assert(sizeof(cf_bin_grad_job) == sizeof(BinGradJob) && sizeof(cf_bin_grad_job) == 72, "cf_bin_grad_job layout");
extern "C" int cf_bin_regions_multi_backward(const cf_bin_grad_job* jobs, int n_jobs, int n_feats, int n_res, const int* bin_sizes,
                                             const int* n_bins_out, int max_cols, int times_input, void* stream) {
    if (!jobs || !bin_sizes || !n_bins_out) return fail("cf_bin_regions_multi_backward: null argument");
    if (n_jobs < 0 || n_feats < 1 || n_feats > 64 || n_res < 1 || n_res > kBinMaxRes || max_cols < 0) return fail("cf_bin_regions_multi_backward: bad argument");
    if (n_jobs == 0) return 0;
    BinPlan pl;
    memset(&pl, 0, sizeof pl);
    pl.n_res = n_res;
    pl.F = n_feats;
    for (int r = 0; r < n_res; ++r) {
        if (bin_sizes[r] < 1 || n_bins_out[r] < 1 || n_bins_out[r] > kBinMaxBins) return fail("cf_bin_regions_multi_backward: bad bin size / bin count at resolution %d", r);
        if (r && bin_sizes[r] >= bin_sizes[r - 1]) return fail("cf_bin_regions_multi_backward: bin sizes must be listed coarsest first (%d after %d)", bin_sizes[r], bin_sizes[r - 1]);
        pl.b[r] = bin_sizes[r];
        pl.L[r] = n_bins_out[r];
    }
    {   // this call WRITES through the job table: rows shorter than the window would overlap.  The table is read back (72 bytes per region,
        // stream-ordered, one synchronisation) -- an attribution call, not a step of a training loop
        std::vector<cf_bin_grad_job> host((size_t)n_jobs);
        if (hipMemcpyAsync(host.data(), jobs, sizeof(cf_bin_grad_job) * (size_t)n_jobs, hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess ||
            hipStreamSynchronize((hipStream_t)stream) != hipSuccess) {
            (void)hipGetLastError();
            return fail("cf_bin_regions_multi_backward: the job table could not be read back (it must be a device array of n_jobs records)");
        }
        for (int k = 0; k < n_jobs; ++k) {
            if (host[k].ncols < 0 || host[k].ncols > max_cols) return fail("cf_bin_regions_multi_backward: ncols = %d of job %d outside [0, max_cols = %d]", host[k].ncols, k, max_cols);
            if (host[k].ld_out < host[k].ncols) return fail("cf_bin_regions_multi_backward: ld_out = %lld < ncols = %d in job %d", host[k].ld_out, host[k].ncols, k);
            if (host[k].ncols > 0 && (!host[k].raw || !host[k].draw)) return fail("cf_bin_regions_multi_backward: null raw / draw in job %d", k);
        }
    }
    bool nested = n_res >= 2 && n_feats <= kBinMaxF && (pl.b[n_res - 1] & 3) == 0 && pl.b[0] <= kBinMaxLoads * 256 && pl.b[0] / pl.b[n_res - 1] <= 64;
    for (int r = 0; r + 1 < n_res; ++r) nested = nested && pl.b[r] % pl.b[r + 1] == 0;
    pl.nested = nested ? 1 : 0;
    const int units = nested ? std::max(1, (max_cols + pl.b[0] - 1) / pl.b[0]) : 1;
    const dim3 grid((units + 3) / 4, n_jobs);
    const int nload = nested ? (pl.b[0] / 4 + 63) / 64 : 4;
    const BinGradJob* jm = reinterpret_cast<const BinGradJob*>(jobs);
    const int times = times_input ? 1 : 0;
    if (nload <= 4) hipLaunchKernelGGL(k_bin_multi_bwd<4>, grid, dim3(256), 0, (hipStream_t)stream, jm, pl, times);
    else if (nload <= 8) hipLaunchKernelGGL(k_bin_multi_bwd<8>, grid, dim3(256), 0, (hipStream_t)stream, jm, pl, times);
    else hipLaunchKernelGGL(k_bin_multi_bwd<16>, grid, dim3(256), 0, (hipStream_t)stream, jm, pl, times);
    LAUNCH_CHECK("k_bin_multi_bwd");
    return 0;
}

static_assert(sizeof(cf_bin_spread_job) == sizeof(BinSpreadJob) && sizeof(cf_bin_spread_job) == 88, "cf_bin_spread_job layout");
extern "C" int cf_bin_spread_difference(const cf_bin_spread_job* jobs, int n_jobs, int n_feats, int n_res, const int* bin_sizes,
                                        const int* n_bins_out, int max_cols, void* stream) {
    if (!jobs || !bin_sizes || !n_bins_out) return fail("cf_bin_spread_difference: null argument");
    if (n_jobs < 0 || n_jobs > 65535 || n_feats < 1 || n_feats > 64 || n_res < 1 || n_res > kBinMaxRes || max_cols < 0)
        return fail("cf_bin_spread_difference: bad argument");
    if (n_jobs == 0) return 0;
    BinPlan pl;
    memset(&pl, 0, sizeof pl);
    pl.n_res = n_res;
    pl.F = n_feats;
    for (int r = 0; r < n_res; ++r) {
        if (bin_sizes[r] < 1 || n_bins_out[r] < 1 || n_bins_out[r] > kBinMaxBins) return fail("cf_bin_spread_difference: bad bin size / bin count at resolution %d", r);
        if (r && bin_sizes[r] >= bin_sizes[r - 1]) return fail("cf_bin_spread_difference: bin sizes must be listed coarsest first (%d after %d)", bin_sizes[r], bin_sizes[r - 1]);
        pl.b[r] = bin_sizes[r];
        pl.L[r] = n_bins_out[r];
    }
    {   // this call WRITES through the job table, as cf_bin_regions_multi_backward does: the table is read back and checked first
        std::vector<cf_bin_spread_job> host((size_t)n_jobs);
        if (hipMemcpyAsync(host.data(), jobs, sizeof(cf_bin_spread_job) * (size_t)n_jobs, hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess ||
            hipStreamSynchronize((hipStream_t)stream) != hipSuccess) {
            (void)hipGetLastError();
            return fail("cf_bin_spread_difference: the job table could not be read back (it must be a device array of n_jobs records)");
        }
        for (int k = 0; k < n_jobs; ++k) {
            const cf_bin_spread_job& j = host[k];
            if (j.ncols < 0 || j.ncols > max_cols) return fail("cf_bin_spread_difference: ncols = %d of job %d outside [0, max_cols = %d]", j.ncols, k, max_cols);
            if (j.ld_out < j.ncols) return fail("cf_bin_spread_difference: ld_out = %lld < ncols = %d in job %d", j.ld_out, j.ncols, k);
            if (j.ncols > 0 && (!j.raw || !j.draw)) return fail("cf_bin_spread_difference: null raw / draw in job %d", k);
            if (j.ncols > 0 && (j.col0 < 0 || j.ld < (long long)j.col0 + j.ncols || (j.raw_donor && j.ld_donor < (long long)j.col0 + j.ncols)))
                return fail("cf_bin_spread_difference: the window [%d, %d + %d) of job %d does not fit its rows (ld = %lld, ld_donor = %lld)", j.col0, j.col0,
                            j.ncols, k, j.ld, j.ld_donor);
        }
    }
    // a chunk of 4 samples lies in one bin of every resolution when the bin sizes nest and the finest is a multiple of 4
    bool nested = (pl.b[n_res - 1] & 3) == 0;
    for (int r = 0; r + 1 < n_res; ++r) nested = nested && pl.b[r] % pl.b[r + 1] == 0;
    pl.nested = nested ? 1 : 0;
    const int chunks = std::max(1, (max_cols + 3) / 4);
    hipLaunchKernelGGL(k_bin_spread_diff, dim3((chunks + 255) / 256, n_jobs), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const BinSpreadJob*>(jobs), pl);
    LAUNCH_CHECK("k_bin_spread_diff");
    return 0;
}

// ------------------------------------------------------------------------------------
// dense (all rows) layer: projections -> attention core -> out-projection / LN / FFN / LN chain, and its backward
// ------------------------------------------------------------------------------------
namespace {
struct DenseWs {       // workspace layout in floats; `train` adds what the backward pass needs
    long long wq_t, wkv_t, wo_t, w1_t, w2_t, q, kv, o, tab;                                  // forward
    long long stats, xh1, rs1, y1, hdn, xh2, rs2;                                             // saved
    long long dt2, dpre1, dt1, da, dq, dkv, delta, partial, wpart;                           // backward
    long long total;
    int splits;
};
constexpr int kDenseTab = 16384;        // floats reserved for the unit / tile tables
constexpr int kDenseSplitRows = 4096;   // reduction rows per split-K chunk of the weight gradients
DenseWs dense_ws(int N, int Lq, int Lk, int dff, bool train) {
    const long long rq = (long long)N * Lq, rk = (long long)N * Lk;
    DenseWs w;
    long long o = 0;
    auto take = [&](long long n) {
        const long long at = o;
        o += (n + 3) / 4 * 4;
        return at;
    };
    w.wq_t = take(128 * 128);
    w.wkv_t = take(256 * 128);
    w.wo_t = take(128 * 128);
    w.w1_t = take((long long)dff * 128);
    w.w2_t = take((long long)128 * dff);
    w.q = take(rq * 128);
    w.kv = take(rk * 256);
    w.o = take(rq * 128);
    w.tab = take(kDenseTab);
    w.splits = 0;
    if (train) {
        const long long tiles = (rq + kTile - 1) / kTile;
        w.stats = take((long long)N * 2 * Lq * 2);
        w.xh1 = take(rq * 128);
        w.rs1 = take(rq);
        w.y1 = take(rq * 128);
        w.hdn = take(rq * dff);
        w.xh2 = take(rq * 128);
        w.rs2 = take(rq);
        w.dt2 = take(rq * 128);
        w.dpre1 = take(rq * dff);
        w.dt1 = take(rq * 128);
        w.da = take(rq * 128);
        w.dq = take(rq * 128);
        w.dkv = take(rk * 256);
        w.delta = take((long long)N * 2 * Lq);
        w.partial = take(tiles * post_partial_width(dff));
        w.splits = (int)((std::max(rq, rk) + kDenseSplitRows - 1) / kDenseSplitRows);
        w.wpart = take((long long)w.splits * 256 * 128);        // the largest weight is 256 x 128 (or 128 x 256)
    }
    w.total = o;
    return w;
}
}  // namespace

extern "C" long long cf_op_dense_layer_workspace(int N, int Lq, int Lk, int d_ff) { return dense_ws(N, Lq, Lk, d_ff, false).total; }
extern "C" long long cf_op_dense_layer_train_workspace(int N, int Lq, int Lk, int d_ff) { return dense_ws(N, Lq, Lk, d_ff, true).total; }

static int dense_layer_fwd(const cf_dense_layer* w, const float* x_q, const float* x_kv, const unsigned char* qvalid, const unsigned char* kvalid,
                           const unsigned char* mask, int N, int Lq, int Lk, float* y, float* ws, bool train, hipStream_t st) {
    if (!w || !x_q || !x_kv || !y || !ws) return fail("cf_op_dense_layer_fwd: null argument");
    if (w->d_ff != 128 && w->d_ff != 256) return fail("cf_op_dense_layer_fwd: d_ff must be 128 or 256");
    if (N < 1 || Lq < 1 || Lk < 1 || N > 65535) return fail("cf_op_dense_layer_fwd: bad shape");
    const int dff = w->d_ff;
    const long long rq = (long long)N * Lq, rk = (long long)N * Lk;
    if (rq > 0x7fffffffLL / 256 || rk > 0x7fffffffLL / 256) return fail("cf_op_dense_layer_fwd: too many rows");
    const DenseWs L = dense_ws(N, Lq, Lk, dff, train);
    // tiled copies of the five weights (no table: workgroup b of a launch takes rows 16 b .. of its matrix)
    struct Job { const float* src; float* dst; int rows, K; } jobs[5] = {{w->wq, ws + L.wq_t, 128, 128}, {w->wkv, ws + L.wkv_t, 256, 128},
                                                                         {w->wo, ws + L.wo_t, 128, 128}, {w->w1, ws + L.w1_t, dff, 128},
                                                                         {w->w2, ws + L.w2_t, 128, dff}};
    for (int j = 0; j < 5; ++j) {
        hipLaunchKernelGGL(k_retile_rows, dim3(jobs[j].rows / 16), dim3(256), 0, st, jobs[j].src, jobs[j].dst, jobs[j].K);
        LAUNCH_CHECK("k_retile_rows<dense layer>");
    }
    auto linear = [&](const float* x, const float* wt, float* out, long long rows, int nout) {
        LinArgs a;
        memset(&a, 0, sizeof a);
        a.x[0] = x;
        a.w[0] = wt;
        a.y[0] = out;
        a.xmap = identity_map();
        a.ldx = 128;
        a.ldy = nout;
        a.N = (int)rows;
        a.K = 128;
        a.Nout = nout;
        hipLaunchKernelGGL((k_linear_fwd<2>), dim3(tiles_of((int)rows), (nout + 127) / 128, 1), dim3(256), 0, st, a);
    };
    linear(x_q, ws + L.wq_t, ws + L.q, rq, 128);
    LAUNCH_CHECK("k_linear_fwd<q>");
    linear(x_kv, ws + L.wkv_t, ws + L.kv, rk, 256);
    LAUNCH_CHECK("k_linear_fwd<kv>");
    {
        AttnArgs a;
        cf_attn_shape sh = {N, 2, Lq, Lk, 128, 256, 256, 128};
        if (attn_args(&sh, a)) return -1;
        a.q = ws + L.q;
        a.k = ws + L.kv;
        a.v = ws + L.kv + 128;
        a.qvalid = qvalid;
        a.kvalid = kvalid;
        a.mask = mask;
        a.o = ws + L.o;
        a.stats = train ? ws + L.stats : nullptr;
        if (attn_fwd_launch(a, st)) return -1;
    }
    {
        PostArgs p;
        memset(&p, 0, sizeof p);
        p.x[0] = x_q;
        p.xmap = identity_map();
        p.ain[0] = ws + L.o;
        p.wo[0] = ws + L.wo_t;
        p.bo[0] = w->bo;
        p.g1[0] = w->ln1_g;
        p.be1[0] = w->ln1_b;
        p.w1[0] = ws + L.w1_t;
        p.b1[0] = w->b1;
        p.w2[0] = ws + L.w2_t;
        p.b2[0] = w->b2;
        p.g2[0] = w->ln2_g;
        p.be2[0] = w->ln2_b;
        if (train) {
            p.xh1[0] = ws + L.xh1;
            p.rs1[0] = ws + L.rs1;
            p.y1[0] = ws + L.y1;
            p.hdn[0] = ws + L.hdn;
            p.xh2[0] = ws + L.xh2;
            p.rs2[0] = ws + L.rs2;
        }
        p.out[0] = y;
        p.omap = identity_map();
        p.N = (int)rq;
        p.save = train ? 1 : 0;
        launch_post_fwd<false, 128>(dff, dim3(tiles_of((int)rq), 1), st, p);
        LAUNCH_CHECK("k_post_fwd<dense layer>");
    }
    return 0;
}
extern "C" int cf_op_dense_layer_fwd(const cf_dense_layer* w, const float* x_q, const float* x_kv, const unsigned char* qvalid,
                                     const unsigned char* kvalid, const unsigned char* mask, int N, int Lq, int Lk, float* y, float* ws,
                                     void* stream) {
    return dense_layer_fwd(w, x_q, x_kv, qvalid, kvalid, mask, N, Lq, Lk, y, ws, false, (hipStream_t)stream);
}
extern "C" int cf_op_dense_layer_fwd_train(const cf_dense_layer* w, const float* x_q, const float* x_kv, const unsigned char* qvalid,
                                           const unsigned char* kvalid, const unsigned char* mask, int N, int Lq, int Lk, float* y, float* ws,
                                           void* stream) {
    return dense_layer_fwd(w, x_q, x_kv, qvalid, kvalid, mask, N, Lq, Lk, y, ws, true, (hipStream_t)stream);
}

// dW[N_, K_] = dY^T X over `rows` rows: split-K over chunks of kDenseSplitRows rows (one k_wgrad tile per (n0, k0, chunk), partial
// results in `part`), then a column sum over the chunks.  Fixed order: deterministic.
static int dense_wgrad(const float* dY, int lddy, const float* X, int ldx, long long rows, float* dW, int N_, int K_, float* part,
                       WgTile* tiles_d, CsTile* cs_d, hipStream_t st) {
    const int splits = (int)((rows + kDenseSplitRows - 1) / kDenseSplitRows);
    const int ntiles = ((N_ + 63) / 64) * ((K_ + kWgTk - 1) / kWgTk) * splits, ncs = (N_ * K_ + 63) / 64;
    if ((size_t)ntiles * sizeof(WgTile) > (size_t)(kDenseTab / 2) * sizeof(float) * 64 || (size_t)ncs * sizeof(CsTile) > (size_t)(kDenseTab / 2) * sizeof(float) * 64)
        return fail("cf_op_dense_layer_bwd: tile table overflow");
    DenseWgTab tb{dY, X, part, dW, tiles_d, cs_d, rows, lddy, ldx, N_, K_, splits, kDenseSplitRows};
    hipLaunchKernelGGL(k_dense_wg_tables, dim3(std::max(1, std::min(64, (ntiles + 255) / 256))), dim3(256), 0, st, tb);
    LAUNCH_CHECK("k_dense_wg_tables");
    hipLaunchKernelGGL(k_wgrad, dim3(xcd_grid(ntiles)), dim3(256), 0, st, (const WgTile*)tiles_d, ntiles, 1, 0);
    LAUNCH_CHECK("k_wgrad<dense layer>");
    hipLaunchKernelGGL(k_colsum, dim3(ncs), dim3(256), 0, st, (const CsTile*)cs_d, 1);
    LAUNCH_CHECK("k_colsum<dense layer>");
    return 0;
}

extern "C" int cf_op_dense_layer_bwd(const cf_dense_layer* w, const float* x_q, const float* x_kv, const unsigned char* qvalid,
                                     const unsigned char* kvalid, const unsigned char* mask, int N, int Lq, int Lk, const float* dy,
                                     float* dx_q, float* dx_kv, const cf_dense_layer_grads* g, float* ws, float* tables, void* stream) {
    if (!w || !x_q || !x_kv || !dy || !dx_q || !dx_kv || !g || !ws || !tables) return fail("cf_op_dense_layer_bwd: null argument");
    if (w->d_ff != 128 && w->d_ff != 256) return fail("cf_op_dense_layer_bwd: d_ff must be 128 or 256");
    hipStream_t st = (hipStream_t)stream;
    const int dff = w->d_ff;
    const long long rq = (long long)N * Lq, rk = (long long)N * Lk;
    const DenseWs L = dense_ws(N, Lq, Lk, dff, true);
    const int tiles_q = tiles_of((int)rq);
    {   // out-projection / LN / FFN / LN chain
        PostBwdArgs p;
        memset(&p, 0, sizeof p);
        p.dout[0] = dy;
        p.dmap = identity_map();
        p.xh2[0] = ws + L.xh2;
        p.rs2[0] = ws + L.rs2;
        p.g2[0] = w->ln2_g;
        p.hdn[0] = ws + L.hdn;
        p.w2[0] = w->w2;
        p.w1[0] = w->w1;
        p.xh1[0] = ws + L.xh1;
        p.rs1[0] = ws + L.rs1;
        p.g1[0] = w->ln1_g;
        p.wo[0] = w->wo;
        p.dt2[0] = ws + L.dt2;
        p.dpre1[0] = ws + L.dpre1;
        p.dt1[0] = ws + L.dt1;
        p.da[0] = ws + L.da;
        p.partial[0] = ws + L.partial;
        p.N = (int)rq;
        launch_post_bwd<false, 128>(dff, dim3(tiles_q, 1), st, p);
        LAUNCH_CHECK("k_post_bwd<dense layer>");
    }
    {   // attention core
        AttnArgs a;
        cf_attn_shape sh = {N, 2, Lq, Lk, 128, 256, 256, 128};
        if (attn_args(&sh, a)) return -1;
        a.q = ws + L.q;
        a.k = ws + L.kv;
        a.v = ws + L.kv + 128;
        a.qvalid = qvalid;
        a.kvalid = kvalid;
        a.mask = mask;
        a.o = ws + L.o;
        a.stats = ws + L.stats;
        a.d_o = ws + L.da;
        a.dq = ws + L.dq;
        a.dk = ws + L.dkv;
        a.dv = ws + L.dkv + 128;
        a.delta = ws + L.delta;
        hipLaunchKernelGGL(k_attn_delta, dim3((Lq + 15) / 16, 2, N), dim3(256), 0, st, a);
        LAUNCH_CHECK("k_attn_delta");
        if (attn_bwd_launch(a, st)) return -1;
    }
    {   // input gradients: dx_q = dt1 (residual) + dq Wq;  dx_kv = dkv Wkv
        DgradArgs d;
        memset(&d, 0, sizeof d);
        d.dy[0] = ws + L.dq;
        d.lddy = 128;
        d.w[0] = w->wq;
        d.ldw = 128;
        d.res[0] = ws + L.dt1;
        d.rmap = identity_map();
        d.ldres = 128;
        d.dx[0] = dx_q;
        d.lddx = 128;
        d.N = (int)rq;
        d.K = 128;
        d.Ncols = 128;
        hipLaunchKernelGGL((k_dgrad<2>), dim3(tiles_q, 128 / 32, 1), dim3(256), 0, st, d);
        LAUNCH_CHECK("k_dgrad<q>");
        memset(&d, 0, sizeof d);
        d.dy[0] = ws + L.dkv;
        d.lddy = 256;
        d.w[0] = w->wkv;
        d.ldw = 128;
        d.rmap = identity_map();
        d.dx[0] = dx_kv;
        d.lddx = 128;
        d.N = (int)rk;
        d.K = 256;
        d.Ncols = 128;
        hipLaunchKernelGGL((k_dgrad<4>), dim3(tiles_of((int)rk), 128 / 32, 1), dim3(256), 0, st, d);
        LAUNCH_CHECK("k_dgrad<kv>");
    }
    // weight gradients (split-K), bias / LayerNorm gradients (column sums of the per-tile partials)
    WgTile* tiles_d = reinterpret_cast<WgTile*>(tables);
    CsTile* cs_d = reinterpret_cast<CsTile*>(tables + (size_t)(kDenseTab / 2) * 64);
    float* part = ws + L.wpart;
    if (dense_wgrad(ws + L.dq, 128, x_q, 128, rq, g->wq, 128, 128, part, tiles_d, cs_d, st)) return -1;
    if (dense_wgrad(ws + L.dkv, 256, x_kv, 128, rk, g->wkv, 256, 128, part, tiles_d, cs_d, st)) return -1;
    if (dense_wgrad(ws + L.dt1, 128, ws + L.o, 128, rq, g->wo, 128, 128, part, tiles_d, cs_d, st)) return -1;
    if (dense_wgrad(ws + L.dpre1, dff, ws + L.y1, 128, rq, g->w1, dff, 128, part, tiles_d, cs_d, st)) return -1;
    if (dense_wgrad(ws + L.dt2, 128, ws + L.hdn, dff, rq, g->w2, 128, dff, part, tiles_d, cs_d, st)) return -1;
    {
        // two stages: the per-tile partial rows (one per 16 input rows: 100,000 of them at the stress shape) are first summed in
        // chunks of 512 rows by many workgroups, then the chunk sums per quantity -- one workgroup walking 100,000 rows took 11 ms
        const int pw = post_partial_width(dff);
        const float* pp = ws + L.partial;
        constexpr int kChunkRows = 512;
        const int nchunks = (tiles_q + kChunkRows - 1) / kChunkRows;
        float* part2 = ws + L.wpart;                 // free again: the weight gradients above are done with it
        if ((long long)nchunks * pw > (long long)L.splits * 256 * 128) return fail("cf_op_dense_layer_bwd: chunk buffer too small");
        const int per = (pw + 63) / 64, n1 = nchunks * per;
        int n2 = 0;
        DenseCsTab tb;
        tb.partial = pp;
        tb.part2 = part2;
        tb.cs1 = reinterpret_cast<CsTile*>(tiles_d);
        tb.cs2 = cs_d;
        tb.tiles_q = tiles_q;
        tb.chunk_rows = kChunkRows;
        tb.nchunks = nchunks;
        tb.pw = pw;
        const int offs[7] = {0, 128, 256, 384, 384 + dff, 512 + dff, 640 + dff}, ncl[7] = {kD, kD, kD, dff, kD, kD, kD};
        float* dsts[7] = {g->ln2_g, g->ln2_b, g->b2, g->b1, g->ln1_g, g->ln1_b, g->bo};
        for (int k = 0; k < 7; ++k) {
            tb.off[k] = offs[k];
            tb.ncols[k] = ncl[k];
            tb.dst[k] = dsts[k];
            n2 += (ncl[k] + 63) / 64;
        }
        if ((size_t)n1 * sizeof(CsTile) > (size_t)(kDenseTab / 2) * sizeof(float) * 64) return fail("cf_op_dense_layer_bwd: tile table overflow");
        hipLaunchKernelGGL(k_dense_cs_tables, dim3(std::max(1, std::min(64, (n1 + 255) / 256))), dim3(256), 0, st, tb);
        LAUNCH_CHECK("k_dense_cs_tables");
        hipLaunchKernelGGL(k_colsum, dim3(n1), dim3(256), 0, st, (const CsTile*)tb.cs1, 1);
        LAUNCH_CHECK("k_colsum<dense layer bias, stage 1>");
        hipLaunchKernelGGL(k_colsum, dim3(n2), dim3(256), 0, st, (const CsTile*)cs_d, 1);
        LAUNCH_CHECK("k_colsum<dense layer bias>");
    }
    return 0;
}

// ------------------------------------------------------------------------------------
// Embedding over all promoter bins (embed.n_layers > 1, cf_embed_full): net.py:9-59 without the centre-row shortcut
// ------------------------------------------------------------------------------------
static int embed_dense_alloc(cf_handle* h) {
    cf_handle::EmbedDense& e = h->ed;
    if (e.ready) return 0;
    const cf_config& c = h->cfg;
    const int B = c.max_batch, E = c.embed_layers;
    auto get = [&](size_t floats) -> float* {      // (separate allocations: the all-rows path keeps the addresses and alignment it has)
        DevBuf<float> q;
        if (q.alloc(floats, "embed_dense_alloc") || hipMemset(q, 0, floats * sizeof(float)) != hipSuccess) {
            e.owned.clear();      // nothing half-made stays behind: the next call starts from an empty list
            return nullptr;
        }
        e.owned.push_back(std::move(q));
        return e.owned.back();
    };
    for (int r = 0; r < c.n_res; ++r) {
        const int L = c.n_bins[r];
        const size_t rows = (size_t)B * L;
        for (int l = 0; l <= E; ++l)
            if (!(e.x[r][l] = get(rows * kD))) return fail("embed_dense_alloc: out of memory");
        for (int l = 0; l < E; ++l)
            if (!(e.ws[r][l] = get((size_t)dense_ws(B, L, L, c.embed_dff, true).total))) return fail("embed_dense_alloc: out of memory");
        for (int k = 0; k < 3; ++k)
            if (!(e.dy[r][k] = get(rows * kD))) return fail("embed_dense_alloc: out of memory");
        if (!(e.lp_partial[r] = get(((rows + kEmbWgRows - 1) / kEmbWgRows) * kD * 8))) return fail("embed_dense_alloc: out of memory");
        if (!(e.valid[r] = reinterpret_cast<uint8_t*>(get((rows + 3) / 4 + 4)))) return fail("embed_dense_alloc: out of memory");
    }
    if (!(e.tables = get((size_t)1 << 20))) return fail("embed_dense_alloc: out of memory");
    e.B = B;
    e.ready = true;
    return 0;
}
// Pad mask of the promoters as the dense layer wants it: the full [B, L, L] byte mask when the caller passed the reference's
// tensor (row stride L * L: the centre-row pointer is L/2 rows into it), else validity bytes from the compact centre row
// -- exact for the dataset's structured masks  not(valid x valid)  with a real centre bin (data.py:156-161).
static void embed_dense_mask(cf_handle* h, const cf_batch* bt, int r, const uint8_t** full, const uint8_t** valid, hipStream_t st) {
    const int L = h->cfg.n_bins[r];
    if (bt->promoter_mask_stride[r] == (long long)L * L) {
        *full = bt->promoter_mask_row[r] - (size_t)(L / 2) * L;
        *valid = nullptr;
    } else {
        hipLaunchKernelGGL(k_mask_to_valid, dim3(bt->B), dim3(256), 0, st, bt->promoter_mask_row[r], bt->promoter_mask_stride[r], L, h->ed.valid[r]);
        *full = nullptr;
        *valid = h->ed.valid[r];
    }
}
static int embed_dense_forward(cf_handle* h, const cf_batch* bt, bool train, hipStream_t st) {
    if (embed_dense_alloc(h)) return -1;
    const cf_config& c = h->cfg;
    const int B = bt->B, E = c.embed_layers, T = c.i_max + 1;
    for (int r = 0; r < c.n_res; ++r) {
        const int L = c.n_bins[r];
        EmbTokArgs ta{bt->promoter_feats[r], h->pe[r], h->refs.lin_proj[r], h->ed.x[r][0], B, L, c.n_feats};
        hipLaunchKernelGGL(k_embed_tokens, dim3(std::min<long long>((long long)B * L, 4096)), dim3(128), 0, st, ta);
        LAUNCH_CHECK("k_embed_tokens");
        const uint8_t *full, *valid;
        embed_dense_mask(h, bt, r, &full, &valid, st);
        for (int l = 0; l < E; ++l) {
            const cf_dense_layer& w = h->refs.ED[r][l];
            if (dense_layer_fwd(&w, h->ed.x[r][l], h->ed.x[r][l], valid, valid, full, B, L, L, h->ed.x[r][l + 1], h->ed.ws[r][l], train, st)) return -1;
        }
        hipLaunchKernelGGL(k_rows_gather, dim3(B), dim3(128), 0, st, (const float*)h->ed.x[r][E], L, L / 2, h->Rx[r][0], T * kD);
        LAUNCH_CHECK("k_rows_gather");
    }
    return 0;
}
static int embed_dense_backward(cf_handle* h, const cf_batch* bt, hipStream_t st) {
    const cf_config& c = h->cfg;
    const int B = bt->B, E = c.embed_layers;
    for (int r = 0; r < c.n_res; ++r) {
        const int L = c.n_bins[r];
        const long long n = (long long)B * L * kD;
        float *dy = h->ed.dy[r][0], *da = h->ed.dy[r][1], *db = h->ed.dy[r][2];
        hipLaunchKernelGGL(k_rows_scatter, dim3(B * L), dim3(128), 0, st, (const float*)h->edout[r], L, L / 2, dy);      // only the centre row is consumed (net.py:59)
        LAUNCH_CHECK("k_rows_scatter");
        const uint8_t *full, *valid;
        embed_dense_mask(h, bt, r, &full, &valid, st);
        for (int l = E - 1; l >= 0; --l) {
            const cf_dense_layer& w = h->refs.ED[r][l];
            cf_dense_layer_grads g{h->grad_of(w.wq), h->grad_of(w.wkv), h->grad_of(w.wo), h->grad_of(w.bo), h->grad_of(w.ln1_g), h->grad_of(w.ln1_b),
                                   h->grad_of(w.w1), h->grad_of(w.b1), h->grad_of(w.w2), h->grad_of(w.b2), h->grad_of(w.ln2_g), h->grad_of(w.ln2_b)};
            if (cf_op_dense_layer_bwd(&w, h->ed.x[r][l], h->ed.x[r][l], valid, valid, full, B, L, L, dy, da, db, &g, h->ed.ws[r][l], h->ed.tables, st)) return -1;
            hipLaunchKernelGGL(k_add_inplace, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, da, (const float*)db, n);      // self-attention: x is query and key/value input
            LAUNCH_CHECK("k_add_inplace");
            std::swap(dy, da);
        }
        const long long rows = (long long)B * L;
        const int chunks = (int)((rows + kEmbWgRows - 1) / kEmbWgRows);
        EmbTokWgArgs wa{dy, bt->promoter_feats[r], h->ed.lp_partial[r], rows, c.n_feats};
        hipLaunchKernelGGL(k_embed_tokens_wgrad, dim3(chunks), dim3(128), 0, st, wa);
        hipLaunchKernelGGL(k_embed_tokens_wgrad2, dim3(1), dim3(128), 0, st, (const float*)h->ed.lp_partial[r], chunks, c.n_feats,
                           h->grad_of(h->refs.lin_proj[r]));
        LAUNCH_CHECK("k_embed_tokens_wgrad");
    }
    return 0;
}

// EmbeddingTransformer.forward's FIRST return value (net.py:57-59): the embeddings of every promoter bin, [B, 1, L, 128] per
// resolution, for consumers that want more than the centre row.  Forward only; not capturable.
extern "C" int cf_embed_full(cf_handle* h, const cf_batch* bt, float* const* out, void* stream) {
    if (check_batch(h, bt) || !out) return fail("cf_embed_full: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    if (embed_dense_forward(h, bt, false, st)) return -1;
    for (int r = 0; r < h->cfg.n_res; ++r) {
        if (!out[r]) continue;
        HIP_TRY(hipMemcpyAsync(out[r], h->ed.x[r][h->cfg.embed_layers], (size_t)bt->B * h->cfg.n_bins[r] * kD * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    return 0;
}
