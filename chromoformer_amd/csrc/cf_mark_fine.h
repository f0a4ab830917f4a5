// cf_mark_fine.h -- histone-mark coalitions whose players are windows of FINEST-resolution bins inside one region
// (cf_mark_fine_coalitions, cf_mark_fine_shapley, cf_mark_fine_shapley_sampled; included by cf_api.hip behind cf_mark_windows.h).
//
// The game joins the window game of cf_mark_windows.h with the rule of cf_scan_fine.h.  f = the finest resolution, R_r = n_bins[f] /
// n_bins[r]; bin j of resolution r has the finest children K_j = [j R_r, min((j + 1) R_r, n_f)) and holds cnt_j = sum of cnt_k
// samples, cnt_k = b_f except the last real finest bin (cnt_last[b]).  The game plays in ONE region (0 the promoter, 1 + j pCRE slot
// j).  Player p is (marks_p, [lo_p, hi_p)), 0 <= lo_p < hi_p, in finest genomic bins relative to start[b]: gene b's window is
// [start[b] + lo_p, start[b] + hi_p) clipped to the region's real n_f.  A coalition is kw = ceil(P / 32) words, bit set = PRESENT.
//     gone_f(k) = OR of marks_p over the absent players whose clipped window holds finest bin k
// and for bin j of resolution r and mark m, C = {k in K_j : bit m in gone_f(k)}:
//   C empty          the element keeps its bits
//   C = K_j          the scale rule   log1pf(s expm1f(u)), ig_signal of cf_ig.h: ONCE however many absent players cover it
//                    the donor rule   the bits of the donor's element at the same position (donor_elem of cf_marks.h)
//   otherwise        the scale rule   S  = sum_{k in C} (double)cnt_k (double)expm1f(u_k)        ascending genomic k
//                                     m' = (float)((double)expm1f(u_j) + ((double)s - 1.0) S / (double)cnt_j),  u' = log1pf(m')
//                                     -- scan_fine_partial of cf_scan_fine.h operation for operation, no contraction, no clamp
//                    the donor rule   d_k bit-equal to u_k for every k in C: the element keeps its bits; else
//                                     D  = sum_{k in C} (double)cnt_k ((double)expm1f(d_k) - (double)expm1f(u_k))
//                                     m' = (float)((double)expm1f(u_j) + D / (double)cnt_j),  u' = log1pf(m')
// C may differ from mark to mark in one bin and any number of bins may be partly covered.  Geometry (extents from the centre pad-mask
// rows, flip for a mirrored promoter) is the scan's; masks and interaction_freq are the gene's own; every other region is copied.
//   k_mark_fine_expand         the grid (chunk row x resolution x kMarkSlices), the 256 threads and the slice-0 mask and frequency
//   k_mark_fine_donor_expand   copies of k_mark_window_expand, in four phases:
//     1  extents   (q_r, n_r) and (q_f, n_f) of the region by waves 0 and 1, two shuffle reductions each over mask rows read four
//                  bytes per load; the 3 P player words and the row's kw coalition words are staged in LDS on the way
//     2  gone_f    one thread per finest bin k < n_bins[f] <= 512 walks the P players (k >= n_f: 0); a block-wide "touched" flag
//     3  some/all  for R_r > 1, one thread per bin j of this resolution: OR and AND of gone_f over K_j (R_r = 1: gone_f itself)
//     4  copy      the workgroup's slice of the row's features, every element written once, float4 where alignment allows.  Regions
//                  other than the game's, and the whole row when the flag is clear, are plain copies (the donor is not loaded); in
//                  the region mark m of bin j takes the whole rule if its bit is in all_j, the partial rule if in some_j & ~all_j
//                  (the thread walks the <= R_r children: gone_f from LDS, the finest features from global memory), else its bits.
//                  The optional feats_out[r] ([B, n_coal, n_bins[r], F], the region only) is written in the same pass.
// No atomics, no scratch, deterministic.  5,668 bytes of LDS (gone_f 2,048, some / all 2,048, staged words 1,552, extents and flag
// 20); 50 / 55 VGPRs (scale / donor rule), no spills (tools/kernel_resources.sh k_mark_fine).  The extent reduction is win_extent of
// cf_rows.h; the end of the partial rule is partial_tail of cf_marks.h, the very text scan_fine_partial runs.
#pragma once

namespace cf {

constexpr int kFineMaxL = 512;         // finest bins per region the gone_f table holds

struct MarkFineArgs {
    MarkExpandArgs m;                  // as for k_mark_expand; m.players: device [3 P + 2 B]: marks_p, lo_p, hi_p, start[B], cnt_last[B]
    const uint8_t* rm_in[kMaxRes];     // the region's centre pad-mask rows: rm_in[r] + b * rm_stride[r]
    long long rm_stride[kMaxRes];
    float* feats_out[kMaxRes];         // optional [B, n_coal, L, F]: the edited region
    const int* start;                  // device [B]: gene b's first finest genomic bin
    const int* cnt_last;               // device [B]: the samples of the last real finest bin (1 .. bf)
    const uint8_t* flip;               // device [B] or nullptr
    int rf, bf, region;                // the finest resolution's index and bin size; 0 promoter, 1 + j pCRE slot j
};

struct MarkFineDonorArgs {
    MarkFineArgs w;
    const float* pf_don[kMaxRes];      // the donor's promoter_feats [B, L, F]
    const float* cf_don[kMaxRes];      // pcre_feats [B, S, L, F]
};

struct FineTable {
    unsigned gone[kFineMaxL];                  // gone_f[k]
    unsigned some[kFineMaxL / 2];              // R_r > 1 (L <= 256): OR of gone_f over K_j
    unsigned all[kFineMaxL / 2];               //                     AND of gone_f over K_j (K_j empty: 0)
    unsigned pl[3 * kMarkWideMaxP];            // marks_p, lo_p, hi_p
    unsigned kept[kMarkWideMaxP / 32];         // the row's coalition words
    int ext[4];                                // q_r, n_r, q_f, n_f
    unsigned any;                              // some gone_f word is non-zero
};

// what the copy needs to know about the region, block-uniform
struct FineGeom {
    const unsigned* some;      // per bin j of this resolution
    const unsigned* all;
    const float* uf;           // the gene's region at the finest resolution [Lf, F]
    const float* df;           // the donor's (donor rule)
    int q, n, qf, nf, R, F, bf, cl;
    bool fl;
    float s;
};

// phases 1 to 3: t filled for chunk row gv = (gene b, coalition gv - b n_coal) at resolution r; ends with a barrier
__device__ __forceinline__ void fine_table(const MarkFineArgs& fa, FineTable& t, int r, int b, long long gv) {
    const MarkExpandArgs& a = fa.m;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, P = a.P, rf = fa.rf, L = a.rows.L[r], Lf = a.rows.L[rf];
    if (wave == 0) {
        int lo, hi;
        win_extent(fa.rm_in[rf] + (size_t)b * fa.rm_stride[rf], Lf, lane, lo, hi);
        if (lane == 0) t.ext[2] = lo, t.ext[3] = hi > lo ? hi - lo : 0, t.any = 0u;
    } else if (wave == 1) {
        int lo, hi;
        win_extent(fa.rm_in[r] + (size_t)b * fa.rm_stride[r], L, lane, lo, hi);
        if (lane == 0) t.ext[0] = lo, t.ext[1] = hi > lo ? hi - lo : 0;
    }
    const int kw = (P + 31) >> 5;
    for (int k = tid; k < 3 * P; k += kIgxThreads) t.pl[k] = a.players[k];
    if (tid < kw) t.kept[tid] = a.words[b * a.word_stride + (gv - (long long)b * a.n_coal) * kw + tid];
    __syncthreads();
    const int nf = t.ext[3];
    const long long st = fa.start[b];
    for (int k = tid; k < Lf; k += kIgxThreads) {
        unsigned w = 0;
        if (k < nf)
            for (int p = 0; p < P; ++p)
                if (!((t.kept[p >> 5] >> (p & 31)) & 1u) && st + (int)t.pl[P + p] <= k && k < st + (int)t.pl[2 * P + p]) w |= t.pl[p];
        t.gone[k] = w;
        if (w) t.any = 1u;      // (every writer stores the same value)
    }
    __syncthreads();
    const int R = Lf / L;
    if (R > 1) {
        for (int j = tid; j < L; j += kIgxThreads) {      // (L = Lf / R <= kFineMaxL / 2)
            const int K0 = j * R, K1 = min(K0 + R, nf);
            unsigned o = 0, n = K0 < K1 ? ~0u : 0u;
            for (int k = K0; k < K1; ++k) o |= t.gone[k], n &= t.gone[k];
            t.some[j] = o, t.all[j] = n;
        }
        __syncthreads();
    }
}

// the partly covered bin j of this resolution, mark f (its bit in some_j & ~all_j); uj: the bin's own feature
template <bool DONOR>
__device__ __forceinline__ float fine_partial(float uj, const FineTable& t, const FineGeom& g, int j, int f) {
#pragma clang fp contract(off)
    const int K0 = j * g.R, K1 = min(K0 + g.R, g.nf);
    double S = 0.0;
    bool same = true;
    for (int k = K0; k < K1; ++k) {
        if (!((t.gone[k] >> f) & 1u)) continue;
        const int row = g.fl ? g.qf + g.nf - 1 - k : g.qf + k;
        const double cnt = (double)(k == g.nf - 1 ? g.cl : g.bf);
        const float u = g.uf[(size_t)row * g.F + f];
        if (DONOR) {
            const float d = g.df[(size_t)row * g.F + f];
            same = same && __float_as_uint(d) == __float_as_uint(u);
            S += cnt * ((double)expm1f(d) - (double)expm1f(u));
        } else {
            S += cnt * (double)expm1f(u);
        }
    }
    if (DONOR && same) return uj;
    return partial_tail(uj, DONOR ? S : ((double)g.s - 1.0) * S, K0, K1, g.nf, g.bf, g.cl);
}

// element e of the region ([L, F], e = row * F + f): x its value, d the donor's (donor rule)
template <bool DONOR>
__device__ __forceinline__ float fine_elem(float x, float d, int e, const FineTable& t, const FineGeom& g) {
    const int row = e / g.F, f = e - row * g.F;
    int j = row - g.q;
    if (j < 0 || j >= g.n) return x;
    if (g.fl) j = g.n - 1 - j;
    const unsigned sm = g.some[j];
    if (!((sm >> f) & 1u)) return x;
    if ((g.all[j] >> f) & 1u) return DONOR ? d : ig_signal(g.s, x);
    return fine_partial<DONOR>(x, t, g, j, f);
}

// does row `row` of the region hold a bin some absent player touches?
__device__ __forceinline__ unsigned fine_row_some(int row, const FineGeom& g) {
    int j = row - g.q;
    if (j < 0 || j >= g.n) return 0u;
    if (g.fl) j = g.n - 1 - j;
    return g.some[j];
}

// dst[0, n) = src[0, n); the elements [off, off + LF) are the game's region (off < 0: not in this segment) and pass through fine_elem
// when `touched`; they also go to fo (nullptr: not wanted).  The workgroup takes the blocks blockIdx.z, blockIdx.z + kMarkSlices, ...
// of kIgxThreads float4s (or floats), as mark_copy.
template <bool DONOR>
__device__ __forceinline__ void fine_copy(const float* __restrict__ src, const float* __restrict__ don, float* __restrict__ dst, int n, int off, int LF,
                                          bool touched, const FineTable& t, const FineGeom& g, float* __restrict__ fo) {
    const int first = blockIdx.z * kIgxThreads + threadIdx.x, step = kMarkSlices * kIgxThreads;
    const bool in = off >= 0;
    bool vec = (n & 3) == 0 && ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0;
    if (in) vec = vec && ((off | LF) & 3) == 0 && g.F >= 4 && (reinterpret_cast<uintptr_t>(fo) & 15) == 0 &&
                  (!DONOR || (reinterpret_cast<uintptr_t>(don) & 15) == 0);
    if (vec) {
        const float4* s4 = reinterpret_cast<const float4*>(src);
        const float4* n4 = reinterpret_cast<const float4*>(don);
        float4* d4 = reinterpret_cast<float4*>(dst);
        float4* f4 = reinterpret_cast<float4*>(fo);
        for (int k = first; k < n / 4; k += step) {
            float4 x = s4[k];
            const int e = 4 * k - off;      // (a float4 lies wholly inside the region or wholly outside: off and LF are multiples of 4)
            if (in && e >= 0 && e < LF) {
                if (touched) {
                    const int row = e / g.F;      // F >= 4: the float4 spans this row and at most the next
                    if (fine_row_some(row, g) | ((e + 3) / g.F != row ? fine_row_some(row + 1, g) : 0u)) {
                        float4 d = x;
                        if (DONOR) d = n4[k];
                        x.x = fine_elem<DONOR>(x.x, d.x, e, t, g);
                        x.y = fine_elem<DONOR>(x.y, d.y, e + 1, t, g);
                        x.z = fine_elem<DONOR>(x.z, d.z, e + 2, t, g);
                        x.w = fine_elem<DONOR>(x.w, d.w, e + 3, t, g);
                    }
                }
                if (fo) f4[e / 4] = x;
            }
            d4[k] = x;
        }
    } else {
        for (int k = first; k < n; k += step) {
            float x = src[k];
            const int e = k - off;
            if (in && e >= 0 && e < LF) {
                if (touched && fine_row_some(e / g.F, g)) x = fine_elem<DONOR>(x, DONOR ? don[k] : x, e, t, g);
                if (fo) fo[e] = x;
            }
            dst[k] = x;
        }
    }
}

template <bool DONOR>
__device__ __forceinline__ void fine_expand(const MarkFineArgs& fa, const float* const* pf_don, const float* const* cf_don, FineTable& t) {
    const MarkExpandArgs& a = fa.m;
    // (the row and the closing lines are written out, not mark_row / rows_masks_freq: with the helpers this kernel measured 0.5 us of its
    // 39.8 us slower, profiles/r22_mark_kernels_shared.txt)
    const int i = blockIdx.x, r = blockIdx.y, rf = fa.rf;
    const long long gv = a.g0 + i;
    const int b = (int)(gv / a.n_coal);
    const int L = a.rows.L[r], Lf = a.rows.L[rf], S = a.rows.S, F = a.F, LF = L * F, LfF = Lf * F;
    fine_table(fa, t, r, b, gv);
    const bool prom = fa.region == 0;
    const size_t reg = prom ? (size_t)b : (size_t)b * S + fa.region - 1;      // the region's index in pf / cf
    FineGeom g;
    g.R = Lf / L;
    g.some = g.R > 1 ? t.some : t.gone;
    g.all = g.R > 1 ? t.all : t.gone;
    g.uf = (prom ? a.pf_in[rf] : a.cf_in[rf]) + reg * LfF;
    g.df = DONOR ? (prom ? pf_don[rf] : cf_don[rf]) + reg * LfF : nullptr;
    g.q = t.ext[0], g.n = t.ext[1], g.qf = t.ext[2], g.nf = t.ext[3];
    g.F = F, g.bf = fa.bf, g.cl = fa.cnt_last[b];
    g.fl = fa.flip && fa.flip[b];
    g.s = a.scale;
    const bool touched = t.any != 0u;
    float* fo = fa.feats_out[r] ? fa.feats_out[r] + (size_t)gv * LF : nullptr;
    fine_copy<DONOR>(a.pf_in[r] + (size_t)b * LF, DONOR ? pf_don[r] + (size_t)b * LF : nullptr, a.pf_out[r] + (size_t)i * LF, LF, prom ? 0 : -1, LF,
                     touched, t, g, prom ? fo : nullptr);
    fine_copy<DONOR>(a.cf_in[r] + (size_t)b * S * LF, DONOR ? cf_don[r] + (size_t)b * S * LF : nullptr, a.cf_out[r] + (size_t)i * S * LF, S * LF,
                     prom ? -1 : (fa.region - 1) * LF, LF, touched, t, g, prom ? nullptr : fo);
    if (blockIdx.z) return;
    rows_pad_masks(a.rows, r, b, i);
    rows_interaction_mask(a.rows, r, b, i);
    if (r == 0) rows_copy_tt(a.freq_in, a.freq_out, b, i, a.rows.TT);
}

__global__ __launch_bounds__(kIgxThreads) void k_mark_fine_expand(MarkFineArgs fa) {
    __shared__ FineTable t;
    fine_expand<false>(fa, nullptr, nullptr, t);
}

__global__ __launch_bounds__(kIgxThreads) void k_mark_fine_donor_expand(MarkFineDonorArgs da) {
    __shared__ FineTable t;
    fine_expand<true>(da.w, da.pf_don, da.cf_don, t);
}

}  // namespace cf
