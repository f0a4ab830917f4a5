// cf_marks.h -- histone-mark coalitions (cf_mark_coalitions, cf_mark_shapley, cf_mark_epistasis and their cf_mark_donor_* siblings;
// included by cf_api.hip behind cf_scan.h), and the device code every mark game shares.
//
// The players of the game are MARKS, each optionally restricted to a set of regions.  Player p is a pair of words: marks_p (bit f:
// mark f) and regions_p (bit 0: the promoter, bit 1 + j: pCRE slot j), both non-zero.  A coalition over P players is kw = ceil(P / 32)
// consecutive 32-bit words, bit p % 32 of word p / 32 set = player p PRESENT: one word for the narrow entry points (P <= 16), up to
// four for the wide ones of cf_marks_wide.h.  Row (b, m) is the inference forward of gene b with these inputs: for every region rho,
//     gone(rho) = OR of marks_p over the absent players p whose regions_p has bit rho
// and every element of region rho, at every resolution and in every row, whose mark f has its bit in gone(rho) becomes
//     u' = log1pf(s expm1f(u))                                  fp32, each operation rounded (no contraction): ig_signal of cf_ig.h
// Every other element keeps its bits; all masks and interaction_freq are the gene's own.
//   * Binning is linear: this is exactly the feature the binning produces when the raw samples of those marks are scaled by s over the
//     whole region (the rule of cf_scan.h with a window that covers the region).
//   * s = 0 (the default of the Python layer) erases the mark: a non-negative finite feature becomes exactly +0.
//   * Padded rows hold zeros and keep their bits (log1pf(s expm1f(0)) = 0), so no row extents are needed: every row is treated alike.
//   * Players may overlap: an element is scaled ONCE if any player that covers it is absent.
//   * Limits are the scan's: u < ~80 (expm1f overflows past 88); a negative feature with 1 + s m <= 0 gives NaN.
//
// Rows are (gene, coalition) pairs, gene-major (gv = b * n_coal + k, words [k kw, (k + 1) kw) of a device table), in chunks of at most
// max_batch rows.  The table is shared by the genes (word_stride = 0: every entry point but the back-selection) or holds n_coal coalitions
// per gene, gene b's at words + b word_stride (cf_backselect.h, whose next rows depend on the gene's previous logits): a runtime field of
// MarkExpandArgs that all six expand kernels read -- one 64-bit multiply-add on the scalar unit per workgroup, no second set of kernels.  One kernel, no atomics, no scratch, 68 bytes of LDS:
//   k_mark_expand   per (chunk row, resolution, slice): the T = i_max + 1 words gone(rho) once per workgroup from the row's kw coalition
//                   words and the 2 P player words; then its slice of the row's promoter and pCRE features (every element written once,
//                   float4 where the row allows; the mark of element e is e % F; a region with gone = 0 is a plain copy); slice 0 also
//                   the row's compact pad-mask rows and interaction mask, at resolution 0 its interaction_freq.  kMarkSlices
//                   workgroups share a (row, resolution): one workgroup per pair leaves the finest resolution's 25,200 floats to 256
//                   threads, ~25 dependent load / store rounds, and the launch latency-bound.
// The reducers are k_shapley and k_epistasis of cf_coalition.h with S = P.
//
// The donor family (cf_mark_donor_coalitions, cf_mark_donor_shapley, cf_mark_donor_epistasis): the same players, words and gone(rho), but
// an element whose mark is in gone(rho) takes the BITS of a second feature set's element at the same (gene, region, row, resolution,
// mark) -- the same gene's signal in another cell type -- instead of the scaled value.  A select, no arithmetic: NaN payloads, -0 and
// inf pass through.  Binning works per mark, so this is exactly the feature the binning produces when those marks' rows of the raw
// region are replaced by the donor's.
//   k_mark_donor_expand   the grid, the gone(rho) words and the element order of k_mark_expand (one body, mark_expand<DONOR>); the donor's
//                         float4 (or float) is loaded only where the element's region has gone != 0, together with the gene's own (both
//                         loads in flight before either is used), and selected per lane by the mark bit.
//
// Shared with the other games (cf_mark_windows.h, cf_mark_fine.h) and the fine scan (cf_scan_fine.h, included behind this file):
//   mark_row       the chunk row of a workgroup: i, r, gv, b (the window game; mark_expand and fine_expand write it out, see there)
//   mark_elem / donor_elem   the two element rules
//   partial_tail   the end of the partial-bin rule of cf_scan_fine.h and cf_mark_fine.h: ONE text, so the two cannot drift apart
#pragma once

namespace cf {

constexpr int kMarkSlices = 8;         // workgroups per (chunk row, resolution): blockIdx.z

struct MarkExpandArgs {
    const float* pf_in[kMaxRes];       // the caller's promoter_feats [B, L, F]
    const float* cf_in[kMaxRes];       // pcre_feats [B, S, L, F]
    float* pf_out[kMaxRes];            // the chunk's copies, [max_batch, L, F] / [max_batch, S, L, F]
    float* cf_out[kMaxRes];
    RowCopyArgs rows;                  // the masks of the chunk's rows (cf_rows.h)
    const float* freq_in;              // [B, T, T]
    float* freq_out;
    const unsigned* words;             // device [n_coal * kw], kw = ceil(P / 32): bit p set: player p present
    long long word_stride;             // 0: one table for all genes; else gene b's n_coal coalitions start at words + b * word_stride
    const unsigned* players;           // device [2 P]: marks_p, then regions_p
    long long g0;                      // first row of the chunk
    float scale;
    int n_coal, P, F;
};

struct MarkDonorArgs {
    MarkExpandArgs m;                  // as for k_mark_expand (scale is not read)
    const float* pf_don[kMaxRes];      // the donor's promoter_feats [B, L, F]
    const float* cf_don[kMaxRes];      // pcre_feats [B, S, L, F]
};

// the workgroup's chunk row i at resolution r: row gv = (gene b, coalition gv - b n_coal) of the call
struct MarkRow {
    long long gv;
    int i, r, b;
};

__device__ __forceinline__ MarkRow mark_row(const MarkExpandArgs& a) {
    MarkRow w;
    w.i = blockIdx.x, w.r = blockIdx.y;
    w.gv = a.g0 + w.i;
    w.b = (int)(w.gv / a.n_coal);
    return w;
}

__device__ __forceinline__ float mark_elem(float x, unsigned gone, int f, float s) { return (gone >> f) & 1u ? ig_signal(s, x) : x; }

// The donor's bits where the mark is gone, else the gene's (an integer select: no canonicalisation of NaNs, -0 stays -0)
__device__ __forceinline__ float donor_elem(float x, float d, unsigned gone, int f) {
    return __uint_as_float((gone >> f) & 1u ? __float_as_uint(d) : __float_as_uint(x));
}

// The end of the partial-bin rule (cf_scan_fine.h; the fine game of cf_mark_fine.h): bin j of a coarser resolution with the finest
// children [K0, K1) of the region's nf real finest bins, bf samples each but cl in the last; uj the bin's own feature, t the change of
// its sample sum.  fp64 division, one narrowing, no contraction, no clamp.
__device__ __forceinline__ float partial_tail(float uj, double t, int K0, int K1, int nf, int bf, int cl) {
#pragma clang fp contract(off)
    const double cj = (double)((K1 - K0) * bf - (K1 == nf ? bf - cl : 0));
    const float m = (float)((double)expm1f(uj) + t / cj);
    return log1pf(m);
}

// gone[rho] = gone(rho), rho = 0 .. i_max, of row gv = (gene b, coalition gv - b n_coal); ends with a barrier
__device__ __forceinline__ void mark_gone(const MarkExpandArgs& a, long long gv, int b, unsigned* gone) {
    const int tid = threadIdx.x, P = a.P;
    if (tid <= a.rows.S) {
        const unsigned* __restrict__ m = a.words + b * a.word_stride + (gv - (long long)b * a.n_coal) * ((P + 31) >> 5);
        unsigned g = 0;
        for (int p0 = 0; p0 < P; p0 += 32) {
            const unsigned absent = ~m[p0 >> 5];      // one load per word, not per player: the walk is serial and latency-bound
            for (int p = p0; p < min(p0 + 32, P); ++p)
                if (((absent >> (p - p0)) & 1u) && ((a.players[P + p] >> tid) & 1u)) g |= a.players[p];
        }
        gone[tid] = g;
    }
    __syncthreads();
}

// dst[0, n) = src[0, n), n = a whole number of regions of LF elements each: element e lies in region e / LF (its word: gone[e / LF])
// and carries mark e % F (LF is a multiple of F).  DONOR: a changed element takes the bits of don[e] (laid out as src, read only in
// regions with gone != 0), else it is scaled by s.  The workgroup takes the blocks blockIdx.z, blockIdx.z + kMarkSlices, ... of
// kIgxThreads float4s (or floats).
template <bool DONOR>
__device__ __forceinline__ void mark_copy(const float* __restrict__ src, const float* __restrict__ don, float* __restrict__ dst, int n, int LF, int F,
                                          const unsigned* gone, float s) {
    const int first = blockIdx.z * kIgxThreads + threadIdx.x, step = kMarkSlices * kIgxThreads;
    const bool vec = (n & 3) == 0 && LF >= 4 &&
                     ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst) | (DONOR ? reinterpret_cast<uintptr_t>(don) : 0)) & 15) == 0;
    if (vec) {
        const float4* s4 = reinterpret_cast<const float4*>(src);
        const float4* n4 = reinterpret_cast<const float4*>(don);
        float4* d4 = reinterpret_cast<float4*>(dst);
        for (int k = first; k < n / 4; k += step) {
            float4 x = s4[k];                                        // (in flight over the index arithmetic)
            const int e = 4 * k, rho = e / LF, rem = e - rho * LF;
            const int over = LF - rem;                               // elements over .. 3 of the float4 lie in region rho + 1 (LF % 4 != 0)
            const unsigned ga = gone[rho], gb = over < 4 ? gone[rho + 1] : ga;
            if (ga | gb) {
                const int f0 = rem % F, f1 = f0 + 1 == F ? 0 : f0 + 1, f2 = f1 + 1 == F ? 0 : f1 + 1, f3 = f2 + 1 == F ? 0 : f2 + 1;
                if (DONOR) {
                    const float4 d = n4[k];
                    x.x = donor_elem(x.x, d.x, ga, f0);
                    x.y = donor_elem(x.y, d.y, over > 1 ? ga : gb, f1);
                    x.z = donor_elem(x.z, d.z, over > 2 ? ga : gb, f2);
                    x.w = donor_elem(x.w, d.w, over > 3 ? ga : gb, f3);
                } else {
                    x.x = mark_elem(x.x, ga, f0, s);
                    x.y = mark_elem(x.y, over > 1 ? ga : gb, f1, s);
                    x.z = mark_elem(x.z, over > 2 ? ga : gb, f2, s);
                    x.w = mark_elem(x.w, over > 3 ? ga : gb, f3, s);
                }
            }
            d4[k] = x;
        }
    } else {
        for (int e = first; e < n; e += step) {
            const int rho = e / LF;
            const unsigned g = gone[rho];
            float x = src[e];
            if (g) x = DONOR ? donor_elem(x, don[e], g, (e - rho * LF) % F) : mark_elem(x, g, (e - rho * LF) % F, s);
            dst[e] = x;
        }
    }
}

template <bool DONOR>
__device__ __forceinline__ void mark_expand(const MarkExpandArgs& a, const float* const* pf_don, const float* const* cf_don, unsigned* gone) {
    // (the row and the closing lines are written out, not mark_row / rows_masks_freq: with the helpers k_mark_donor_expand measured 0.1 us
    // of its 11.2 us slower, profiles/r22_mark_kernels_shared.txt)
    const int i = blockIdx.x, r = blockIdx.y;
    const long long gv = a.g0 + i;
    const int b = (int)(gv / a.n_coal);
    const int S = a.rows.S, F = a.F, LF = a.rows.L[r] * F;
    mark_gone(a, gv, b, gone);
    mark_copy<DONOR>(a.pf_in[r] + (size_t)b * LF, DONOR ? pf_don[r] + (size_t)b * LF : nullptr, a.pf_out[r] + (size_t)i * LF, LF, LF, F, gone, a.scale);
    mark_copy<DONOR>(a.cf_in[r] + (size_t)b * S * LF, DONOR ? cf_don[r] + (size_t)b * S * LF : nullptr, a.cf_out[r] + (size_t)i * S * LF, S * LF, LF, F,
                     gone + 1, a.scale);
    if (blockIdx.z) return;
    rows_pad_masks(a.rows, r, b, i);
    rows_interaction_mask(a.rows, r, b, i);
    if (r == 0) rows_copy_tt(a.freq_in, a.freq_out, b, i, a.rows.TT);
}

__global__ __launch_bounds__(kIgxThreads) void k_mark_expand(MarkExpandArgs a) {
    __shared__ unsigned gone[kCoalMaxS + 1];      // gone(rho), rho = 0 .. i_max: 68 bytes
    mark_expand<false>(a, nullptr, nullptr, gone);
}

__global__ __launch_bounds__(kIgxThreads) void k_mark_donor_expand(MarkDonorArgs da) {
    __shared__ unsigned gone[kCoalMaxS + 1];
    mark_expand<true>(da.m, da.pf_don, da.cf_don, gone);
}

}  // namespace cf
