// cf_scan_fine.h -- fine-resolution perturbation scan (cf_perturbation_scan_fine; included by cf_api.hip behind cf_scan.h and cf_marks.h,
// whose partial_tail ends the third case of the rule below).
//
// The scan of cf_scan.h with windows given in bins of the FINEST resolution f (the smallest bin size), so a window may cover a coarser
// bin only in part.  The perturbation is the scan's: the window's raw samples of a mark set are scaled by s >= 0.  With R_r =
// n_bins[f] / n_bins[r], bin j of resolution r has the finest children K_j = [j R_r, min((j + 1) R_r, n_f)) and holds cnt_j = sum of
// cnt_k samples, cnt_k = b_f except the last real finest bin (cnt_last[b], 1 .. b_f: the short tail of a region).  For a window
// [lo, hi) of finest genomic bins and C = K_j n [lo, hi):
//   C empty          the element keeps its bits
//   C = K_j          u' = log1pf(s expm1f(u))                          ig_signal of cf_ig.h: the scan's rule (always so at resolution f)
//   otherwise        S  = sum_{k in C} (double)cnt_k (double)expm1f(u_k)        ascending genomic k, u_k the source gene's finest features
//                    m' = (float)((double)expm1f(u_j) + ((double)s - 1.0) S / (double)cnt_j)
//                    u' = log1pf(m')                                    no contraction, no clamp
// Binning is linear per mark, so this is the feature the binning produces from the scaled samples, up to the rounding of the stored
// fp32 features.  A window has two ends, so at most two bins of a resolution are partly covered.
//
// Geometry: the scan's.  The centre pad-mask row gives q_r and n_r; genomic bin j is row q_r + j, mirrored q_r + n_r - 1 - j.
// Rows are (gene, variant) pairs, gene-major (gv = b * V + v, V = 1 + n_sets * n_windows):
//   v = 0                       gene b verbatim
//   v = 1 + k * n_windows + g   mark set k scaled over [start[b] + g stride, start[b] + g stride + width), clipped to n_f
// One kernel, no atomics, no scratch; LDS: the two row-extent reductions and the <= 2 x 32 recomputed values.
//   k_scan_fine_expand   per (chunk row, resolution), k_scan_expand's shape.  The (<= 2 bins) x (marks of the set) partly covered values
//                        are computed first, one lane each (a short dependent sum over <= R_r - 1 children), into LDS; meanwhile the
//                        other waves copy the segment that is not scanned, the masks and the frequencies; one barrier; then the scanned
//                        segment is copied with its covered rows rewritten (every element is written once).
#pragma once

namespace cf {

constexpr int kScanFineMaxMarks = 32;      // a mark set is one 32-bit word

struct ScanFineExpandArgs {
    const float* pf_in[kMaxRes];       // as ScanExpandArgs
    const float* cf_in[kMaxRes];
    float* pf_out[kMaxRes];
    float* cf_out[kMaxRes];
    float* feats_out[kMaxRes];
    RowCopyArgs rows;
    const uint8_t* rm_in[kMaxRes];
    long long rm_stride[kMaxRes];
    const float* freq_in;
    float* freq_out;
    const unsigned* sets;              // device [n_sets]
    const int* start;                  // device [B]: the first finest genomic bin of window 0
    const int* cnt_last;               // device [B]: the samples of the last real finest bin (1 .. bf)
    const uint8_t* flip;               // device [B] or nullptr
    float scale;
    int g0, V, F, NW, width, stride, rf, bf, region;
};

// one covered element of the scanned segment: row p of the region, mark f
__device__ __forceinline__ float scan_fine_elem(float x, int e, int off, int c0, int c1, unsigned bits, int F, float s, int pr0, int pr1,
                                                const float* pv) {
    if (e < c0 || e >= c1) return x;
    const int p = (e - off) / F, f = (e - off) - p * F;
    if (!((bits >> f) & 1u)) return x;
    if (p == pr0) return pv[f];
    if (p == pr1) return pv[kScanFineMaxMarks + f];
    return ig_signal(s, x);
}

// scan_copy of cf_scan.h with the partly covered rows pr0 / pr1 (-1: none) of the region taken from pv
__device__ __forceinline__ void scan_fine_copy(const float* __restrict__ src, float* __restrict__ dst, int n, int off, int len, int c0, int c1,
                                               unsigned bits, int F, float s, int pr0, int pr1, const float* pv, float* __restrict__ fo) {
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
                x.x = scan_fine_elem(x.x, e, off, c0, c1, bits, F, s, pr0, pr1, pv);
                x.y = scan_fine_elem(x.y, e + 1, off, c0, c1, bits, F, s, pr0, pr1, pv);
                x.z = scan_fine_elem(x.z, e + 2, off, c0, c1, bits, F, s, pr0, pr1, pv);
                x.w = scan_fine_elem(x.w, e + 3, off, c0, c1, bits, F, s, pr0, pr1, pv);
            }
            d4[k] = x;
            if (fo && e >= off && e < off + len) f4[(e - off) / 4] = x;
        }
    } else {
        for (int e = threadIdx.x; e < n; e += kIgxThreads) {
            const float x = scan_fine_elem(src[e], e, off, c0, c1, bits, F, s, pr0, pr1, pv);
            dst[e] = x;
            if (fo && e >= off && e < off + len) fo[e - off] = x;
        }
    }
}

// the partly covered bin j of this resolution, mark f: the rule's third case.  uj: the bin's own feature; uf: the region's finest
// features [Lf, F] of the source gene; children [k0, k1) of the window, all of the bin [K0, K1).
__device__ __forceinline__ float scan_fine_partial(float uj, const float* __restrict__ uf, int f, int F, int k0, int k1, int K0, int K1, int qf,
                                                   int nf, bool fl, int bf, int cl, float s) {
#pragma clang fp contract(off)
    double S = 0.0;
    for (int k = k0; k < k1; ++k) {
        const int row = fl ? qf + nf - 1 - k : qf + k;
        const double cnt = (double)(k == nf - 1 ? cl : bf);
        S += cnt * (double)expm1f(uf[(size_t)row * F + f]);
    }
    return partial_tail(uj, ((double)s - 1.0) * S, K0, K1, nf, bf, cl);
}

__global__ __launch_bounds__(kIgxThreads) void k_scan_fine_expand(ScanFineExpandArgs a) {
    __shared__ int red[2 * (kIgxThreads / 64)];
    __shared__ float pv[2 * kScanFineMaxMarks];
    const int i = blockIdx.x, r = blockIdx.y;
    const int gv = a.g0 + i, b = gv / a.V, v = gv - b * a.V;
    const int L = a.rows.L[r], S = a.rows.S, F = a.F, LF = L * F, Lf = a.rows.L[a.rf];
    const bool prom = a.region == 0;
    // the covered rows [p0, p1) of the scanned region at this resolution and its partly covered rows (block-uniform)
    int p0 = 0, p1 = 0, pr0 = -1, pr1 = -1;
    unsigned bits = 0;
    if (v > 0) {
        const int k = (v - 1) / a.NW, g = (v - 1) - k * a.NW;
        bits = a.sets[k];
        int qf, ef;
        scan_extent(a.rm_in[a.rf] + (size_t)b * a.rm_stride[a.rf], Lf, red, qf, ef);
        const int nf = ef > qf ? ef - qf : 0;
        const long long wl = (long long)a.start[b] + (long long)g * a.stride;
        const int lo = (int)min(wl, (long long)nf), hi = (int)min(wl + a.width, (long long)nf);
        if (bits && lo < hi) {
            int q = qf, e = ef;
            if (r != a.rf) scan_extent(a.rm_in[r] + (size_t)b * a.rm_stride[r], L, red, q, e);
            const int n = e > q ? e - q : 0, R = Lf / L;
            const int ja = lo / R, jb = min((hi + R - 1) / R, n);
            if (ja < jb) {
                const bool fl = a.flip && a.flip[b];
                p0 = fl ? q + n - jb : q + ja;
                p1 = fl ? q + n - ja : q + jb;
                if (R > 1) {
                    const float* ur = prom ? a.pf_in[r] + (size_t)b * LF : a.cf_in[r] + ((size_t)b * S + a.region - 1) * LF;
                    const float* uf = prom ? a.pf_in[a.rf] + (size_t)b * Lf * F : a.cf_in[a.rf] + ((size_t)b * S + a.region - 1) * Lf * F;
                    const int cl = a.cnt_last[b];
                    int np = 0;
#pragma unroll
                    for (int t = 0; t < 2; ++t) {      // the bins that hold the window's two ends
                        const int j = t ? jb - 1 : ja;
                        if (t == 1 && j == ja) break;
                        const int K0 = j * R, K1 = min(K0 + R, nf), k0 = max(lo, K0), k1 = min(hi, K1);
                        if (k0 == K0 && k1 == K1) continue;      // wholly covered
                        const int row = fl ? q + n - 1 - j : q + j;
                        if (np == 0) pr0 = row; else pr1 = row;
                        const int f = threadIdx.x - np * kScanFineMaxMarks;
                        if (f >= 0 && f < F && ((bits >> f) & 1u))
                            pv[np * kScanFineMaxMarks + f] = scan_fine_partial(ur[(size_t)row * F + f], uf, f, F, k0, k1, K0, K1, qf, nf, fl, a.bf, cl, a.scale);
                        ++np;
                    }
                }
            }
        }
    }
    float* fo = a.feats_out[r] ? a.feats_out[r] + (size_t)gv * LF : nullptr;
    const int off = prom ? 0 : (a.region - 1) * LF;
    // what is not scanned first: the waves without a partly covered value to compute do not wait for those that have one
    if (prom) scan_fine_copy(a.cf_in[r] + (size_t)b * S * LF, a.cf_out[r] + (size_t)i * S * LF, S * LF, 0, 0, 0, 0, 0u, F, a.scale, -1, -1, pv, nullptr);
    else scan_fine_copy(a.pf_in[r] + (size_t)b * LF, a.pf_out[r] + (size_t)i * LF, LF, 0, 0, 0, 0, 0u, F, a.scale, -1, -1, pv, nullptr);
    rows_masks_freq(a.rows, a.freq_in, a.freq_out, r, b, i);
    __syncthreads();      // pv
    if (prom) scan_fine_copy(a.pf_in[r] + (size_t)b * LF, a.pf_out[r] + (size_t)i * LF, LF, 0, LF, p0 * F, p1 * F, bits, F, a.scale, pr0, pr1, pv, fo);
    else scan_fine_copy(a.cf_in[r] + (size_t)b * S * LF, a.cf_out[r] + (size_t)i * S * LF, S * LF, off, LF, off + p0 * F, off + p1 * F, bits, F, a.scale,
                        pr0, pr1, pv, fo);
}

}  // namespace cf
