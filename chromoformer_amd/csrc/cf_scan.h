// cf_scan.h -- in-silico perturbation scan (cf_perturbation_scan, cf_perturbation_scan_regions; included by cf_api.hip behind cf_ig.h).
//
// One region of every gene -- the promoter or one pCRE slot -- is scanned: the histone marks of a mark set are scaled by s >= 0 in
// RAW-SIGNAL space over a window of the region, and the gene is run forward.  Binning is linear, so scaling the samples of a bin by
// s scales the bin's mean by s, and the feature u = log(1 + m) of a covered bin becomes
//     u' = log1pf(s expm1f(u))                                  fp32, each operation rounded (no contraction): ig_signal of cf_ig.h
// exactly the feature the binning would produce from the scaled signal.
//
// Geometry.  c = the coarsest resolution (fewest bins), W = n_bins[c], R_r = n_bins[r] / W.  At resolution r the region's centre
// pad-mask row gives q_r / e_r, the first / last unmasked row, n_r = e_r - q_r + 1 (0: all masked; holes inside count).  Genomic
// bin j sits in row q_r + j, or in row q_r + n_r - 1 - j where the region is stored mirrored (flip[b]).  Window g of width w covers
// the coarse genomic bins [g, min(g + w, n_c)) and at resolution r the genomic bins [g R_r, min(min(g + w, n_c) R_r, n_r)): bin
// sizes nest, so every finer bin lies in one coarse bin (short last bins included).
//
// Rows are (gene, variant) pairs, gene-major (gv = b * V + v, V = 1 + n_sets * W):
//   v = 0               gene b verbatim
//   v = 1 + k * W + g   mark set k scaled over window g (g >= n_c, or an empty set: gene b verbatim)
// in chunks of at most max_batch rows.  One kernel, no atomics, no LDS beyond the two row-extent reductions:
//   k_scan_expand   per (chunk row, resolution): the row's features of every region, its compact pad-mask rows and interaction
//                   mask, resolution 0 also its interaction_freq -- float4 where the row allows; the covered rows of the scanned region
//                   are rewritten on the way (every element is written once), and the scanned region's rows also go to feats_out.
#pragma once

namespace cf {

struct ScanExpandArgs {
    const float* pf_in[kMaxRes];       // the caller's promoter_feats [B, L, F]
    const float* cf_in[kMaxRes];       // pcre_feats [B, S, L, F]
    float* pf_out[kMaxRes];            // the chunk's copies, [max_batch, L, F] / [max_batch, S, L, F]
    float* cf_out[kMaxRes];
    float* feats_out[kMaxRes];         // [B, V, L, F]: the scanned region as row (b, v) reads it; nullptr: not wanted
    RowCopyArgs rows;                  // the masks of the chunk's rows (cf_rows.h)
    const uint8_t* rm_in[kMaxRes];     // the scanned region's centre pad-mask row of gene b: rm_in[r] + b * rm_stride[r]
    long long rm_stride[kMaxRes];
    const float* freq_in;              // [B, T, T]
    float* freq_out;
    const unsigned* sets;              // device [n_sets]: bit f set: mark f is scaled
    const uint8_t* flip;               // device [B] or nullptr
    float scale;
    int g0, V, F, W, width, rc, region;
};

// first unmasked row and one past the last of a mask row of L bytes (lo = L, hi = 0: all masked); every thread gets the result
__device__ __forceinline__ void scan_extent(const uint8_t* __restrict__ m, int L, int* red, int& lo, int& hi) {
    int a = L, b = 0;
    for (int k = threadIdx.x; k < L; k += kIgxThreads)
        if (!m[k]) a = min(a, k), b = max(b, k + 1);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) a = min(a, __shfl_xor(a, o, 64)), b = max(b, __shfl_xor(b, o, 64));
    __syncthreads();      // (red may still be read from the previous call)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a, red[kIgxThreads / 64 + (threadIdx.x >> 6)] = b;
    __syncthreads();
    lo = L, hi = 0;
#pragma unroll
    for (int k = 0; k < kIgxThreads / 64; ++k) lo = min(lo, red[k]), hi = max(hi, red[kIgxThreads / 64 + k]);
}

// one element of the scanned segment: e in [c0, c1) (the covered rows, in elements of the segment) with its mark in `bits` is scaled
__device__ __forceinline__ float scan_elem(float x, int e, int off, int c0, int c1, unsigned bits, int F, float s) {
    if (e < c0 || e >= c1) return x;
    const int f = (e - off) % F;
    return (bits >> f) & 1u ? ig_signal(s, x) : x;
}

// dst[0, n) = src[0, n); elements [c0, c1) pass through scan_elem; elements [off, off + len) also go to fo (nullptr: not wanted)
__device__ __forceinline__ void scan_copy(const float* __restrict__ src, float* __restrict__ dst, int n, int off, int len, int c0, int c1,
                                          unsigned bits, int F, float s, float* __restrict__ fo) {
    const bool vec = (n & 3) == 0 && ((off | len) & 3) == 0 &&
                     ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(fo)) & 15) == 0;
    if (vec) {
        const float4* s4 = reinterpret_cast<const float4*>(src);
        float4* d4 = reinterpret_cast<float4*>(dst);
        float4* f4 = reinterpret_cast<float4*>(fo);
        for (int k = threadIdx.x; k < n / 4; k += kIgxThreads) {
            float4 x = s4[k];
            const int e = 4 * k;
            if (e + 4 > c0 && e < c1) {
                x.x = scan_elem(x.x, e, off, c0, c1, bits, F, s);
                x.y = scan_elem(x.y, e + 1, off, c0, c1, bits, F, s);
                x.z = scan_elem(x.z, e + 2, off, c0, c1, bits, F, s);
                x.w = scan_elem(x.w, e + 3, off, c0, c1, bits, F, s);
            }
            d4[k] = x;
            if (fo && e >= off && e < off + len) f4[(e - off) / 4] = x;
        }
    } else {
        for (int e = threadIdx.x; e < n; e += kIgxThreads) {
            const float x = scan_elem(src[e], e, off, c0, c1, bits, F, s);
            dst[e] = x;
            if (fo && e >= off && e < off + len) fo[e - off] = x;
        }
    }
}

__global__ __launch_bounds__(kIgxThreads) void k_scan_expand(ScanExpandArgs a) {
    __shared__ int red[2 * (kIgxThreads / 64)];
    const int i = blockIdx.x, r = blockIdx.y;
    const int gv = a.g0 + i, b = gv / a.V, v = gv - b * a.V;
    const int L = a.rows.L[r], S = a.rows.S, F = a.F, LF = L * F;
    // the covered rows [p0, p1) of the scanned region at this resolution (block-uniform)
    int p0 = 0, p1 = 0;
    unsigned bits = 0;
    if (v > 0) {
        const int k = (v - 1) / a.W, g = (v - 1) - k * a.W;
        bits = a.sets[k];
        int lo, hi;
        scan_extent(a.rm_in[a.rc] + (size_t)b * a.rm_stride[a.rc], a.rows.L[a.rc], red, lo, hi);
        const int nc = hi > lo ? hi - lo : 0;
        if (bits && g < nc) {
            if (r != a.rc) scan_extent(a.rm_in[r] + (size_t)b * a.rm_stride[r], L, red, lo, hi);
            const int nr = hi > lo ? hi - lo : 0, R = L / a.W;
            const int j0 = g * R, j1 = min(min(g + a.width, nc) * R, nr);
            if (j0 < j1) {
                const bool fl = a.flip && a.flip[b];
                p0 = fl ? lo + nr - j1 : lo + j0;
                p1 = fl ? lo + nr - j0 : lo + j1;
            }
        }
    }
    float* fo = a.feats_out[r] ? a.feats_out[r] + (size_t)gv * LF : nullptr;
    const bool prom = a.region == 0;
    const int off = prom ? 0 : (a.region - 1) * LF;
    scan_copy(a.pf_in[r] + (size_t)b * LF, a.pf_out[r] + (size_t)i * LF, LF, 0, LF, prom ? p0 * F : 0, prom ? p1 * F : 0, bits, F, a.scale,
              prom ? fo : nullptr);
    scan_copy(a.cf_in[r] + (size_t)b * S * LF, a.cf_out[r] + (size_t)i * S * LF, S * LF, off, LF, prom ? 0 : off + p0 * F,
              prom ? 0 : off + p1 * F, bits, F, a.scale, prom ? nullptr : fo);
    rows_masks_freq(a.rows, a.freq_in, a.freq_out, r, b, i);
}

// Several regions per call (cf_perturbation_scan_regions): the variants of ONE pCRE slot j, slot-packed.  The Pairwise output of a slot
// depends on the promoter and on that slot alone, and the S slots of a gene are S independent rows of one tile: a pseudo-gene with gene
// b's promoter and S differently perturbed copies of its slot j as slots yields, in one trunk pass, the changed Regulation input row of
// S variants.  Pseudo rows are (gene, u) pairs, gene-major (gp = b * U + u, U = ceil((V - 1) / S)); slot s of pseudo row (b, u) is
// variant v = 1 + u * S + s (v >= V: slot j verbatim).  Byte movers plus the window rule above, no atomics:
//   k_scan_pack     per (pseudo row, resolution): the promoter's features and pad-mask rows verbatim, slot j's features under each of
//                   the S variants, slot j's pad-mask row into every slot
//   k_scan_unpack   per (pseudo row, resolution): rows 1..S of the pseudo-gene's trunk output -> xv[(b, v - 1)], one d_emb row per variant
//   k_scan_rows     per (row (b, v), resolution): the stashed trunk output of gene b -> Rx[r][0] with row j + 1 from xv (v >= 1), the
//                   gene's interaction mask, resolution 0 also its interaction_freq
struct ScanPackArgs {
    const float* pf_in[kMaxRes];       // as ScanExpandArgs
    const float* cf_in[kMaxRes];
    float* pf_out[kMaxRes];
    float* cf_out[kMaxRes];
    RowCopyArgs rows;                  // the pad masks (the interaction masks are not read by the trunk: not copied)
    const unsigned* sets;
    float scale;
    int g0, U, V, F, W, width, rc, slot;
};

__global__ __launch_bounds__(kIgxThreads) void k_scan_pack(ScanPackArgs a) {
    __shared__ int red[2 * (kIgxThreads / 64)];
    const int i = blockIdx.x, r = blockIdx.y;
    const int gp = a.g0 + i, b = gp / a.U, u = gp - b * a.U;
    const int L = a.rows.L[r], S = a.rows.S, F = a.F, LF = L * F, PL = a.rows.pm_rows[r] * L;
    // slot j's extent at the coarsest resolution and at this one (block-uniform; k_scan_expand's geometry, never mirrored)
    const uint8_t* cm = a.rows.cm_in[r] + ((size_t)b * S + a.slot) * a.rows.cm_stride[r];
    int clo, chi, lo, hi;
    scan_extent(a.rows.cm_in[a.rc] + ((size_t)b * S + a.slot) * a.rows.cm_stride[a.rc], a.rows.L[a.rc], red, clo, chi);
    scan_extent(cm, L, red, lo, hi);
    const int nc = chi > clo ? chi - clo : 0, nr = hi > lo ? hi - lo : 0, R = L / a.W;
    scan_copy(a.pf_in[r] + (size_t)b * LF, a.pf_out[r] + (size_t)i * LF, LF, 0, LF, 0, 0, 0u, F, a.scale, nullptr);
    const float* src = a.cf_in[r] + ((size_t)b * S + a.slot) * LF;
    for (int s = 0; s < S; ++s) {
        const int v = 1 + u * S + s;
        int p0 = 0, p1 = 0;
        unsigned bits = 0;
        if (v < a.V) {
            const int k = (v - 1) / a.W, g = (v - 1) - k * a.W;
            bits = a.sets[k];
            if (bits && g < nc) {
                const int j0 = g * R, j1 = min(min(g + a.width, nc) * R, nr);
                if (j0 < j1) p0 = lo + j0, p1 = lo + j1;
            }
        }
        scan_copy(src, a.cf_out[r] + ((size_t)i * S + s) * LF, LF, 0, LF, p0 * F, p1 * F, bits, F, a.scale, nullptr);
    }
    for (int k = threadIdx.x; k < PL; k += kIgxThreads) a.rows.pm_out[r][(size_t)i * PL + k] = a.rows.pm_in[r][(size_t)b * a.rows.pm_stride[r] + k];
    for (int k = threadIdx.x; k < S * L; k += kIgxThreads) a.rows.cm_out[r][(size_t)i * S * L + k] = cm[k % L];
}

struct ScanUnpackArgs {
    const float4* x0[kMaxRes];         // Rx[r][0] of the chunk's pseudo-genes, [n, T, D / 4]
    float4* xv[kMaxRes];               // [B * (V - 1), D / 4]
    int g0, U, V, S, T, d4;
};

__global__ __launch_bounds__(kRowThreads) void k_scan_unpack(ScanUnpackArgs a) {
    const int i = blockIdx.x, r = blockIdx.y;
    const int gp = a.g0 + i, b = gp / a.U, u = gp - b * a.U;
    const int n = min(a.S, a.V - 1 - u * a.S) * a.d4;      // rows 1..S are adjacent, and so are their variants
    const float4* __restrict__ src = a.x0[r] + ((size_t)i * a.T + 1) * a.d4;
    float4* __restrict__ dst = a.xv[r] + ((size_t)b * (a.V - 1) + (size_t)u * a.S) * a.d4;
    for (int k = threadIdx.x; k < n; k += kRowThreads) dst[k] = src[k];
}

struct ScanRowsArgs {
    const float4* stash[kMaxRes];      // [B, T * D / 4]: the genes' own trunk output
    const float4* xv[kMaxRes];
    float4* x0[kMaxRes];               // Rx[r][0], rows of the chunk
    RowCopyArgs rows;                  // the interaction masks
    const float* freq_in;              // [B, T, T]
    float* freq_out;
    int g0, V, row4, d4, slot;
};

__global__ __launch_bounds__(kRowThreads) void k_scan_rows(ScanRowsArgs a) {
    const int i = blockIdx.x, r = blockIdx.y;
    const int gv = a.g0 + i, b = gv / a.V, v = gv - b * a.V;
    const float4* __restrict__ src = a.stash[r] + (size_t)b * a.row4;
    const float4* __restrict__ var = a.xv[r] + ((size_t)b * (a.V - 1) + (v > 0 ? v - 1 : 0)) * a.d4;
    float4* __restrict__ dst = a.x0[r] + (size_t)i * a.row4;
    const int k0 = v > 0 ? (a.slot + 1) * a.d4 : a.row4;      // (v = 0: no row is replaced)
    for (int k = threadIdx.x; k < a.row4; k += kRowThreads) dst[k] = k >= k0 && k < k0 + a.d4 ? var[k - k0] : src[k];
    rows_interaction_mask(a.rows, r, b, i);
    if (r == 0) rows_copy_tt(a.freq_in, a.freq_out, b, i, a.rows.TT);
}

}  // namespace cf
