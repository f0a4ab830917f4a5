// cf_ig.h -- integrated gradients (cf_integrated_gradients; included by cf_api.hip).
//
// For a target logit column t, quadrature nodes a_k and weights w_k (k = 0 .. n-1) on [0, 1], per interpolated input x with
// baseline xb:
//     x_k  = xb + a_k (x - xb)                                  fp32, each operation rounded (no contraction)
//     g_k  = d(w_k logits[:, t]) / d x_k                        the backward from dlogits = w_k at column t
//     attr = (x - xb) ((g_0 + g_1) + ... + g_{n-1})             fp32, k order
//     delta = sum(attr) - (F(x)[t] - F(xb)[t])                  per gene, over every interpolated element
// Rows are (gene, variant) pairs, gene-major (gv = b * V + v, V = n + 2):
//   v = 0        x verbatim  (F(x); dlogits 0)
//   v = 1        xb verbatim (F(xb); dlogits 0)
//   v = 2 + k    x_k         (dlogits w_k at column t)
// in chunks of at most max_batch rows; a gene's rows may straddle chunks.  Three kernels, no atomics:
//   k_ig_expand      per (chunk row, resolution): the row's features (interpolated or copied), pad-mask rows, interaction mask;
//                    resolution 0 also its interaction_freq and dlogits row.  In the frequency-only mode (nothing the trunk reads
//                    depends on the row's alpha) it copies the stashed trunk output of the row's gene instead of features and masks.
//   k_ig_accumulate  per (gene touched by the chunk, element slice): the gene's rows in v order -- v = 0 / 1 copy the logits, the
//                    first interior row writes the per-row gradient into the output, later ones add, the last multiplies by
//                    x - xb and leaves the slice's sum of attributions (one block sum in a fixed order).  kIgSlices workgroups per
//                    gene, each a fixed subset of the gene's elements.
//   k_ig_delta       per gene, once per call: the slice sums in slice order, minus F(x)[t] - F(xb)[t].
// The order of every sum depends on the gene's layout alone: the same bits whatever max_batch is.
#pragma once

namespace cf {

constexpr int kIgxThreads = 256;
constexpr int kIgSegs = 2 * kMaxRes + 1;      // promoter_feats[r], pcre_feats[r], interaction_freq

struct IgSeg {
    const float* x;           // the caller's input, [B, len]
    const float* xb;          // baseline [B or 1, len]; nullptr: zeros
    float* row;               // the chunk's copy, [max_batch, len]
    const float* grad;        // per-row gradient scratch, [max_batch, len]
    float* out;               // attribution [B, len] (nullptr: this input is not interpolated)
    int len;
};

struct IgExpandArgs {
    IgSeg seg[kIgSegs];
    const uint8_t* pm_in[kMaxRes];     // the caller's pad-mask centre rows (promoter: row = gene; pCRE: row = gene * S + slot)
    const uint8_t* cm_in[kMaxRes];
    long long pm_stride[kMaxRes], cm_stride[kMaxRes];
    uint8_t* pm_out[kMaxRes];          // the chunk's compact rows, stride L
    uint8_t* cm_out[kMaxRes];
    int pm_rows[kMaxRes];              // 1; L where the all-rows Embedding reads the caller's full [B, L, L] promoter mask: pm_in is then
                                       // row 0 of gene 0 and the chunk's copy keeps all L rows per chunk row (stride L * L)
    const uint8_t* im_in[kMaxRes];     // interaction masks [B, T, T]
    uint8_t* im_out[kMaxRes];
    const float4* stash[kMaxRes];      // frequency-only mode: the trunk output of the B genes, [B, T * D / 4]
    float4* x0[kMaxRes];               // ... copied into Rx[r][0], [n, T * D / 4]
    const float* alpha;                // device [n_steps]
    const float* weight;               // device [n_steps]
    float* dlogits;                    // [n, n_out]
    int L[kMaxRes];
    int g0, V, S, TT, n_out, target, nres, bcast, freq_only, row4;
};

// dst = x (v = 0), xb (v = 1), xb + a (x - xb) (interior) or x (not interpolated); float4 where the row allows
__device__ __forceinline__ void ig_row(const IgSeg& s, int b, int i, int v, float a, bool bcast) {
#pragma clang fp contract(off)
    const int n = s.len;
    const float* __restrict__ x = s.x + (size_t)b * n;
    const float* __restrict__ xb = s.xb ? s.xb + (bcast ? (size_t)0 : (size_t)b * n) : nullptr;
    float* __restrict__ d = s.row + (size_t)i * n;
    const int mode = !s.out || v == 0 ? 0 : v == 1 ? 1 : 2;
    const bool vec = (n & 3) == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(xb) | reinterpret_cast<uintptr_t>(d)) & 15) == 0;
    if (vec) {
        const float4* x4 = reinterpret_cast<const float4*>(x);
        const float4* b4 = reinterpret_cast<const float4*>(xb);
        float4* d4 = reinterpret_cast<float4*>(d);
        for (int e = threadIdx.x; e < n / 4; e += kIgxThreads) {
            const float4 xv = x4[e];
            const float4 bv = b4 ? b4[e] : make_float4(0.f, 0.f, 0.f, 0.f);
            float4 o;
            if (mode == 0) o = xv;
            else if (mode == 1) o = bv;
            else o = make_float4(bv.x + a * (xv.x - bv.x), bv.y + a * (xv.y - bv.y), bv.z + a * (xv.z - bv.z), bv.w + a * (xv.w - bv.w));
            d4[e] = o;
        }
    } else {
        for (int e = threadIdx.x; e < n; e += kIgxThreads) {
            const float xv = x[e], bv = xb ? xb[e] : 0.f;
            d[e] = mode == 0 ? xv : mode == 1 ? bv : bv + a * (xv - bv);
        }
    }
}

__global__ __launch_bounds__(kIgxThreads) void k_ig_expand(IgExpandArgs a) {
    const int i = blockIdx.x, r = blockIdx.y, tid = threadIdx.x;
    const int gv = a.g0 + i, b = gv / a.V, v = gv - b * a.V;
    const float alpha = v >= 2 ? a.alpha[v - 2] : 0.f;
    const bool bc = a.bcast != 0;
    if (a.freq_only) {
        const float4* __restrict__ src = a.stash[r] + (size_t)b * a.row4;
        float4* __restrict__ dst = a.x0[r] + (size_t)i * a.row4;
        for (int k = tid; k < a.row4; k += kIgxThreads) dst[k] = src[k];
    } else {
        const int L = a.L[r], S = a.S;
        ig_row(a.seg[r], b, i, v, alpha, bc);
        ig_row(a.seg[kMaxRes + r], b, i, v, alpha, bc);
        const int PL = a.pm_rows[r] * L;
        for (int k = tid; k < PL; k += kIgxThreads) a.pm_out[r][(size_t)i * PL + k] = a.pm_in[r][(size_t)b * a.pm_stride[r] + k];
        for (int k = tid; k < S * L; k += kIgxThreads) {
            const int s = k / L, j = k - s * L;
            a.cm_out[r][((size_t)i * S + s) * L + j] = a.cm_in[r][((size_t)b * S + s) * a.cm_stride[r] + j];
        }
    }
    for (int k = tid; k < a.TT; k += kIgxThreads) a.im_out[r][(size_t)i * a.TT + k] = a.im_in[r][(size_t)b * a.TT + k];
    if (r == 0) {
        ig_row(a.seg[2 * kMaxRes], b, i, v, alpha, bc);
        for (int k = tid; k < a.n_out; k += kIgxThreads) a.dlogits[(size_t)i * a.n_out + k] = v >= 2 && k == a.target ? a.weight[v - 2] : 0.f;
    }
}

constexpr int kIgSlices = 32;      // workgroups per gene in k_ig_accumulate (a gene's ~31.5 k elements: ~1 float4 per thread)

struct IgAccArgs {
    IgSeg seg[kIgSegs];
    const float* logits;               // the chunk's rows, [n, n_out]
    float* logits_x;                   // [B, n_out]
    float* logits_b;                   // [B, n_out]
    float* part;                       // [B, kIgSlices]: each slice's sum of attributions
    int g0, n, V, n_out, bcast;
};

// rows i0 .. i0 + nv - 1 of the chunk are variants v0 .. v0 + nv - 1 (all interior) of gene b; this workgroup takes the elements
// (float4 or scalar) slice, slice + kIgSlices, ... of the segment in blocks of kIgxThreads.  Returns this thread's sum of attr when
// the last of the rows is the gene's last row, else 0
__device__ __forceinline__ float ig_acc(const IgSeg& s, int b, int i0, int v0, int nv, int V, bool bcast, int slice) {
#pragma clang fp contract(off)
    if (!s.out || nv <= 0) return 0.f;
    const int n = s.len;
    const bool first = v0 == 2, last = v0 + nv == V;
    const float* __restrict__ x = s.x + (size_t)b * n;
    const float* __restrict__ xb = s.xb ? s.xb + (bcast ? (size_t)0 : (size_t)b * n) : nullptr;
    const float* __restrict__ g = s.grad + (size_t)i0 * n;
    float* __restrict__ o = s.out + (size_t)b * n;
    float part = 0.f;
    const int e0 = slice * kIgxThreads + threadIdx.x, step = kIgSlices * kIgxThreads;
    const bool vec = (n & 3) == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(xb) | reinterpret_cast<uintptr_t>(g) |
                                       reinterpret_cast<uintptr_t>(o)) & 15) == 0;
    if (vec) {
        const int n4 = n / 4;
        for (int e = e0; e < n4; e += step) {
            float4 acc = first ? reinterpret_cast<const float4*>(g)[e] : reinterpret_cast<const float4*>(o)[e];
            for (int k = first ? 1 : 0; k < nv; ++k) {
                const float4 gk = reinterpret_cast<const float4*>(g + (size_t)k * n)[e];
                acc = make_float4(acc.x + gk.x, acc.y + gk.y, acc.z + gk.z, acc.w + gk.w);
            }
            if (last) {
                const float4 xv = reinterpret_cast<const float4*>(x)[e];
                const float4 bv = xb ? reinterpret_cast<const float4*>(xb)[e] : make_float4(0.f, 0.f, 0.f, 0.f);
                acc = make_float4((xv.x - bv.x) * acc.x, (xv.y - bv.y) * acc.y, (xv.z - bv.z) * acc.z, (xv.w - bv.w) * acc.w);
                part += ((acc.x + acc.y) + acc.z) + acc.w;
            }
            reinterpret_cast<float4*>(o)[e] = acc;
        }
    } else {
        for (int e = e0; e < n; e += step) {
            float acc = first ? g[e] : o[e];
            for (int k = first ? 1 : 0; k < nv; ++k) acc = acc + g[(size_t)k * n + e];
            if (last) {
                acc = (x[e] - (xb ? xb[e] : 0.f)) * acc;
                part += acc;
            }
            o[e] = acc;
        }
    }
    return part;
}

__global__ __launch_bounds__(kIgxThreads) void k_ig_accumulate(IgAccArgs a) {
#pragma clang fp contract(off)
    __shared__ float red[kIgxThreads / 64];
    const int b = a.g0 / a.V + blockIdx.x, slice = blockIdx.y, tid = threadIdx.x;
    const int vlo = max(0, a.g0 - b * a.V), vhi = min(a.V, a.g0 + a.n - b * a.V);      // the gene's variants in this chunk: [vlo, vhi)
    const int irow = b * a.V - a.g0;                                                     // chunk row of variant 0 (may be negative)
    const bool bc = a.bcast != 0;
    if (slice == 0)
        for (int k = tid; k < a.n_out; k += kIgxThreads) {
            if (vlo == 0) a.logits_x[(size_t)b * a.n_out + k] = a.logits[(size_t)irow * a.n_out + k];
            if (vlo <= 1 && vhi > 1) a.logits_b[(size_t)b * a.n_out + k] = a.logits[(size_t)(irow + 1) * a.n_out + k];
        }
    const int v0 = max(vlo, 2), nv = vhi - v0;
    float part = 0.f;
    for (int s = 0; s < kIgSegs; ++s) part += ig_acc(a.seg[s], b, irow + v0, v0, nv, a.V, bc, slice);
    if (vhi != a.V || nv <= 0) return;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) part += __shfl_xor(part, o, 64);
    if ((tid & 63) == 0) red[tid >> 6] = part;
    __syncthreads();
    if (tid == 0) {
        float sum = 0.f;
        for (int k = 0; k < kIgxThreads / 64; ++k) sum += red[k];
        a.part[(size_t)b * kIgSlices + slice] = sum;
    }
}

// delta[b] = (slice sums in slice order) - (F(x)[t] - F(xb)[t]); one thread per gene
__global__ __launch_bounds__(64) void k_ig_delta(const float* part, const float* logits_x, const float* logits_b, float* delta, int B,
                                                 int n_out, int target) {
#pragma clang fp contract(off)
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    float sum = 0.f;
    for (int k = 0; k < kIgSlices; ++k) sum += part[(size_t)b * kIgSlices + k];
    delta[b] = sum - (logits_x[(size_t)b * n_out + target] - logits_b[(size_t)b * n_out + target]);
}

}  // namespace cf
