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
//
// Signal path (cf_integrated_gradients_raw; template parameter kIgSignal, the kernels k_ig_expand_raw / k_ig_accumulate_raw).  The two
// feature segments hold u = log(1 + m), m >= 0 the mean of a bin of the raw signal; the baseline is the empty signal and the path
// is the straight line a m in MEAN space, which is curved in feature space:
//     u_k   = log1p(a_k expm1(u))                               the row of node k (v = 0: u verbatim, v = 1: zeros)
//     g_k   = d(w_k logits[:, t]) / d u_k                       the same backward
//     C     = (g_0 / (1 + a_0 m) + g_1 / (1 + a_1 m)) + ...     fp32, k order, m = expm1f(u); no contraction
//     attr  = m C                                               integrated gradients with respect to the bin mean: complete
//     coeff = (1 + m) C                                         second output: dfeat of cf_bin_regions_multi_backward(times_input = 1),
//                                                               which divides by cnt (1 + m) and multiplies by the raw sample
// interaction_freq keeps the straight path and its baseline.  Between a gene's chunks `out` holds the running C; the last row turns it
// into attr (and writes coeff).  The row helpers ig_row / ig_acc are templates on the path; the linear kernels' code is unchanged.
//
// Donor path (cf_integrated_gradients_raw_donor; kIgSignalDonor, the kernels k_ig_expand_raw_donor / k_ig_accumulate_raw_donor).  The
// baseline of the two feature segments is a second signal over the same regions, binned the same way: IgSeg::xb holds ud = log(1 + md).
// The path is the straight line md + a (m - md) in MEAN space, which is the binned x(a) = xd + a (x - xd) because binning is linear:
//     m = expm1f(u), md = expm1f(ud), d = m - md, mk = md + a_k d
//     u_k   = log1pf(mk)                                        the row of node k (v = 0: u verbatim, v = 1: ud verbatim)
//     C     = (g_0 / (1 + mk_0) + g_1 / (1 + mk_1)) + ...       fp32, k order; no contraction
//     attr  = d C                                               complete: sums to F(x)[t] - F(xd)[t] up to the quadrature error
//     cmean = C                                                 second output: what k_bin_spread_diff (cf_bin_spread.h) spreads over
//                                                               the difference of the two raw signals
// An element with the same bits in both has d = 0 and gets exactly 0.  With ud = 0: md = 0, d = m and mk = 0 + a m carries the bits
// of a m, so rows, attr, logits and delta are those of the signal path.  The bodies ig_row_donor / ig_acc_donor are functions of
// their own: no instruction of the kernels above moves.
#pragma once

namespace cf {

constexpr int kIgxThreads = kRowThreads;
constexpr int kIgSegs = 2 * kMaxRes + 1;      // promoter_feats[r], pcre_feats[r], interaction_freq
constexpr int kIgLinear = 0, kIgSignal = 1;   // path of a feature segment: xb + a (x - xb) | log1p(a expm1(x)) from the zero signal
constexpr int kIgSignalDonor = 2;             // ... | log1p(md + a (m - md)), m = expm1(x), md = expm1(xb): from a donor signal

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
    RowCopyArgs rows;                  // the masks of the chunk's rows (cf_rows.h)
    const float4* stash[kMaxRes];      // frequency-only mode: the trunk output of the B genes, [B, T * D / 4]
    float4* x0[kMaxRes];               // ... copied into Rx[r][0], [n, T * D / 4]
    const float* alpha;                // device [n_steps]
    const float* weight;               // device [n_steps]
    float* dlogits;                    // [n, n_out]
    int g0, V, n_out, target, nres, bcast, freq_only, row4;
};

// the signal path's interior value of one element
__device__ __forceinline__ float ig_signal(float a, float x) {
#pragma clang fp contract(off)
    return log1pf(a * expm1f(x));
}

// dst = x (v = 0), xb (v = 1), xb + a (x - xb) (interior) or x (not interpolated); float4 where the row allows.  PATH = kIgSignal:
// xb is the zero signal (s.xb is not read) and the interior is log1p(a expm1(x))
template <int PATH>
__device__ __forceinline__ void ig_row(const IgSeg& s, int b, int i, int v, float a, bool bcast) {
#pragma clang fp contract(off)
    const int n = s.len;
    const float* __restrict__ x = s.x + (size_t)b * n;
    const float* __restrict__ xb = PATH == kIgLinear && s.xb ? s.xb + (bcast ? (size_t)0 : (size_t)b * n) : nullptr;
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
            else if (PATH == kIgSignal) o = make_float4(ig_signal(a, xv.x), ig_signal(a, xv.y), ig_signal(a, xv.z), ig_signal(a, xv.w));
            else o = make_float4(bv.x + a * (xv.x - bv.x), bv.y + a * (xv.y - bv.y), bv.z + a * (xv.z - bv.z), bv.w + a * (xv.w - bv.w));
            d4[e] = o;
        }
    } else {
        for (int e = threadIdx.x; e < n; e += kIgxThreads) {
            const float xv = x[e], bv = xb ? xb[e] : 0.f;
            d[e] = mode == 0 ? xv : mode == 1 ? bv : PATH == kIgSignal ? ig_signal(a, xv) : bv + a * (xv - bv);
        }
    }
}

template <int PATH>
__device__ __forceinline__ void ig_expand(const IgExpandArgs a) {
    const int i = blockIdx.x, r = blockIdx.y, tid = threadIdx.x;
    const int gv = a.g0 + i, b = gv / a.V, v = gv - b * a.V;
    const float alpha = v >= 2 ? a.alpha[v - 2] : 0.f;
    const bool bc = a.bcast != 0;
    if (a.freq_only) {
        rows_copy_x0(a.stash[r], a.x0[r], b, i, a.row4);
    } else {
        ig_row<PATH>(a.seg[r], b, i, v, alpha, bc);
        ig_row<PATH>(a.seg[kMaxRes + r], b, i, v, alpha, bc);
        rows_pad_masks(a.rows, r, b, i);
    }
    rows_interaction_mask(a.rows, r, b, i);
    if (r == 0) {
        ig_row<kIgLinear>(a.seg[2 * kMaxRes], b, i, v, alpha, bc);
        for (int k = tid; k < a.n_out; k += kIgxThreads) a.dlogits[(size_t)i * a.n_out + k] = v >= 2 && k == a.target ? a.weight[v - 2] : 0.f;
    }
}
__global__ __launch_bounds__(kIgxThreads) void k_ig_expand(IgExpandArgs a) { ig_expand<kIgLinear>(a); }
__global__ __launch_bounds__(kIgxThreads) void k_ig_expand_raw(IgExpandArgs a) { ig_expand<kIgSignal>(a); }

// the donor path's interior value of one element
__device__ __forceinline__ float ig_signal_donor(float a, float x, float xd) {
#pragma clang fp contract(off)
    const float md = expm1f(xd);
    const float d = expm1f(x) - md;
    return log1pf(md + a * d);
}

// ig_row for kIgSignalDonor: dst = x (v = 0 or not interpolated), xb (v = 1: the donor's features verbatim) or log1p(md + a (m - md));
// xb is per gene ([B, len], never broadcast) and is read only where the segment is interpolated
__device__ __forceinline__ void ig_row_donor(const IgSeg& s, int b, int i, int v, float a) {
#pragma clang fp contract(off)
    const int n = s.len;
    const float* __restrict__ x = s.x + (size_t)b * n;
    const float* __restrict__ xb = s.out ? s.xb + (size_t)b * n : nullptr;
    float* __restrict__ d = s.row + (size_t)i * n;
    const int mode = !s.out || v == 0 ? 0 : v == 1 ? 1 : 2;
    const bool vec = (n & 3) == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(xb) | reinterpret_cast<uintptr_t>(d)) & 15) == 0;
    if (vec) {
        const float4* x4 = reinterpret_cast<const float4*>(x);
        const float4* b4 = reinterpret_cast<const float4*>(xb);
        float4* d4 = reinterpret_cast<float4*>(d);
        for (int e = threadIdx.x; e < n / 4; e += kIgxThreads) {
            const float4 xv = x4[e];
            float4 o = xv;
            if (mode != 0) {
                const float4 bv = b4[e];
                o = mode == 1 ? bv
                              : make_float4(ig_signal_donor(a, xv.x, bv.x), ig_signal_donor(a, xv.y, bv.y), ig_signal_donor(a, xv.z, bv.z),
                                            ig_signal_donor(a, xv.w, bv.w));
            }
            d4[e] = o;
        }
    } else {
        for (int e = threadIdx.x; e < n; e += kIgxThreads) {
            const float xv = x[e];
            d[e] = mode == 0 ? xv : mode == 1 ? xb[e] : ig_signal_donor(a, xv, xb[e]);
        }
    }
}

// k_ig_expand for the donor path: the feature segments by ig_row_donor, everything else as ig_expand (never frequency-only: a feature
// bit is set)
__global__ __launch_bounds__(kIgxThreads) void k_ig_expand_raw_donor(IgExpandArgs a) {
    const int i = blockIdx.x, r = blockIdx.y, tid = threadIdx.x;
    const int gv = a.g0 + i, b = gv / a.V, v = gv - b * a.V;
    const float alpha = v >= 2 ? a.alpha[v - 2] : 0.f;
    ig_row_donor(a.seg[r], b, i, v, alpha);
    ig_row_donor(a.seg[kMaxRes + r], b, i, v, alpha);
    rows_pad_masks(a.rows, r, b, i);
    rows_interaction_mask(a.rows, r, b, i);
    if (r == 0) {
        ig_row<kIgLinear>(a.seg[2 * kMaxRes], b, i, v, alpha, a.bcast != 0);
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

struct IgAccRawArgs {                  // k_ig_accumulate_raw: the arguments above, the node table and the second output
    IgAccArgs a;
    const float* alpha;                // device [n_steps]
    float* coeff[2 * kMaxRes];         // per feature segment [B, len]; nullptr: not wanted
};

// rows i0 .. i0 + nv - 1 of the chunk are variants v0 .. v0 + nv - 1 (all interior) of gene b; this workgroup takes the elements
// (float4 or scalar) slice, slice + kIgSlices, ... of the segment in blocks of kIgxThreads.  Returns this thread's sum of attr when
// the last of the rows is the gene's last row, else 0.  PATH = kIgSignal: row k adds g_k / (1 + alpha[v0 - 2 + k] m), m = expm1f(x),
// the last row writes m acc (and (1 + m) acc into coeff)
template <int PATH>
__device__ __forceinline__ float ig_acc(const IgSeg& s, float* coeff, const float* alpha, int b, int i0, int v0, int nv, int V, bool bcast, int slice) {
#pragma clang fp contract(off)
    if (!s.out || nv <= 0) return 0.f;
    const int n = s.len;
    const bool first = v0 == 2, last = v0 + nv == V;
    const float* __restrict__ x = s.x + (size_t)b * n;
    const float* __restrict__ xb = PATH == kIgLinear && s.xb ? s.xb + (bcast ? (size_t)0 : (size_t)b * n) : nullptr;
    const float* __restrict__ g = s.grad + (size_t)i0 * n;
    float* __restrict__ o = s.out + (size_t)b * n;
    float* __restrict__ co = PATH == kIgSignal && coeff ? coeff + (size_t)b * n : nullptr;
    float part = 0.f;
    const int e0 = slice * kIgxThreads + threadIdx.x, step = kIgSlices * kIgxThreads;
    if (PATH == kIgSignal) {
        const bool vec = (n & 3) == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(o) |
                                           reinterpret_cast<uintptr_t>(co)) & 15) == 0;
        if (vec) {
            const int n4 = n / 4;
            for (int e = e0; e < n4; e += step) {
                const float4 xv = reinterpret_cast<const float4*>(x)[e];
                const float4 m = make_float4(expm1f(xv.x), expm1f(xv.y), expm1f(xv.z), expm1f(xv.w));
                float4 acc = first ? make_float4(0.f, 0.f, 0.f, 0.f) : reinterpret_cast<const float4*>(o)[e];
                for (int k = 0; k < nv; ++k) {
                    const float4 gk = reinterpret_cast<const float4*>(g + (size_t)k * n)[e];
                    const float ak = alpha[v0 - 2 + k];
                    const float4 t = make_float4(gk.x / (1.0f + ak * m.x), gk.y / (1.0f + ak * m.y), gk.z / (1.0f + ak * m.z), gk.w / (1.0f + ak * m.w));
                    acc = first && k == 0 ? t : make_float4(acc.x + t.x, acc.y + t.y, acc.z + t.z, acc.w + t.w);
                }
                if (last) {
                    if (co) reinterpret_cast<float4*>(co)[e] = make_float4((1.0f + m.x) * acc.x, (1.0f + m.y) * acc.y, (1.0f + m.z) * acc.z, (1.0f + m.w) * acc.w);
                    acc = make_float4(m.x * acc.x, m.y * acc.y, m.z * acc.z, m.w * acc.w);
                    part += ((acc.x + acc.y) + acc.z) + acc.w;
                }
                reinterpret_cast<float4*>(o)[e] = acc;
            }
        } else {
            for (int e = e0; e < n; e += step) {
                const float m = expm1f(x[e]);
                float acc = first ? 0.f : o[e];
                for (int k = 0; k < nv; ++k) {
                    const float t = g[(size_t)k * n + e] / (1.0f + alpha[v0 - 2 + k] * m);
                    acc = first && k == 0 ? t : acc + t;
                }
                if (last) {
                    if (co) co[e] = (1.0f + m) * acc;
                    acc = m * acc;
                    part += acc;
                }
                o[e] = acc;
            }
        }
        return part;
    }
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
    for (int s = 0; s < kIgSegs; ++s) part += ig_acc<kIgLinear>(a.seg[s], nullptr, nullptr, b, irow + v0, v0, nv, a.V, bc, slice);
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

// k_ig_accumulate for the signal path: the feature segments divide each row's gradient by 1 + a_k m (node table in the arguments) and
// finish with attr = m acc, coeff = (1 + m) acc; interaction_freq as in k_ig_accumulate.  (A kernel of its own, not a second
// instantiation of one body: k_ig_accumulate's code stays exactly what it was.)
__global__ __launch_bounds__(kIgxThreads) void k_ig_accumulate_raw(IgAccRawArgs ra) {
#pragma clang fp contract(off)
    __shared__ float red[kIgxThreads / 64];
    const IgAccArgs& a = ra.a;
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
    for (int s = 0; s < 2 * kMaxRes; ++s) part += ig_acc<kIgSignal>(a.seg[s], ra.coeff[s], ra.alpha, b, irow + v0, v0, nv, a.V, bc, slice);
    part += ig_acc<kIgLinear>(a.seg[2 * kMaxRes], nullptr, nullptr, b, irow + v0, v0, nv, a.V, bc, slice);
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

// ig_acc for kIgSignalDonor: row k adds g_k / (1 + mk), mk = md + alpha[v0 - 2 + k] d; between a gene's chunks `out` holds the running
// C; the last row writes C into cmean (where given) and d C into out
__device__ __forceinline__ float ig_acc_donor(const IgSeg& s, float* cmean, const float* alpha, int b, int i0, int v0, int nv, int V, int slice) {
#pragma clang fp contract(off)
    if (!s.out || nv <= 0) return 0.f;
    const int n = s.len;
    const bool first = v0 == 2, last = v0 + nv == V;
    const float* __restrict__ x = s.x + (size_t)b * n;
    const float* __restrict__ xb = s.xb + (size_t)b * n;
    const float* __restrict__ g = s.grad + (size_t)i0 * n;
    float* __restrict__ o = s.out + (size_t)b * n;
    float* __restrict__ co = cmean ? cmean + (size_t)b * n : nullptr;
    float part = 0.f;
    const int e0 = slice * kIgxThreads + threadIdx.x, step = kIgSlices * kIgxThreads;
    const bool vec = (n & 3) == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(xb) | reinterpret_cast<uintptr_t>(g) |
                                       reinterpret_cast<uintptr_t>(o) | reinterpret_cast<uintptr_t>(co)) & 15) == 0;
    if (vec) {
        const int n4 = n / 4;
        for (int e = e0; e < n4; e += step) {
            const float4 xv = reinterpret_cast<const float4*>(x)[e];
            const float4 bv = reinterpret_cast<const float4*>(xb)[e];
            const float4 md = make_float4(expm1f(bv.x), expm1f(bv.y), expm1f(bv.z), expm1f(bv.w));
            const float4 d = make_float4(expm1f(xv.x) - md.x, expm1f(xv.y) - md.y, expm1f(xv.z) - md.z, expm1f(xv.w) - md.w);
            float4 acc = first ? make_float4(0.f, 0.f, 0.f, 0.f) : reinterpret_cast<const float4*>(o)[e];
            for (int k = 0; k < nv; ++k) {
                const float4 gk = reinterpret_cast<const float4*>(g + (size_t)k * n)[e];
                const float ak = alpha[v0 - 2 + k];
                const float4 t = make_float4(gk.x / (1.0f + (md.x + ak * d.x)), gk.y / (1.0f + (md.y + ak * d.y)), gk.z / (1.0f + (md.z + ak * d.z)),
                                             gk.w / (1.0f + (md.w + ak * d.w)));
                acc = first && k == 0 ? t : make_float4(acc.x + t.x, acc.y + t.y, acc.z + t.z, acc.w + t.w);
            }
            if (last) {
                if (co) reinterpret_cast<float4*>(co)[e] = acc;
                acc = make_float4(d.x * acc.x, d.y * acc.y, d.z * acc.z, d.w * acc.w);
                part += ((acc.x + acc.y) + acc.z) + acc.w;
            }
            reinterpret_cast<float4*>(o)[e] = acc;
        }
    } else {
        for (int e = e0; e < n; e += step) {
            const float md = expm1f(xb[e]);
            const float d = expm1f(x[e]) - md;
            float acc = first ? 0.f : o[e];
            for (int k = 0; k < nv; ++k) {
                const float t = g[(size_t)k * n + e] / (1.0f + (md + alpha[v0 - 2 + k] * d));
                acc = first && k == 0 ? t : acc + t;
            }
            if (last) {
                if (co) co[e] = acc;
                acc = d * acc;
                part += acc;
            }
            o[e] = acc;
        }
    }
    return part;
}

// k_ig_accumulate for the donor path: the arguments of k_ig_accumulate_raw, `coeff` holding the cmean outputs; the feature segments by
// ig_acc_donor, interaction_freq as in k_ig_accumulate
__global__ __launch_bounds__(kIgxThreads) void k_ig_accumulate_raw_donor(IgAccRawArgs ra) {
#pragma clang fp contract(off)
    __shared__ float red[kIgxThreads / 64];
    const IgAccArgs& a = ra.a;
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
    for (int s = 0; s < 2 * kMaxRes; ++s) part += ig_acc_donor(a.seg[s], ra.coeff[s], ra.alpha, b, irow + v0, v0, nv, a.V, slice);
    part += ig_acc<kIgLinear>(a.seg[2 * kMaxRes], nullptr, nullptr, b, irow + v0, v0, nv, a.V, bc, slice);
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
