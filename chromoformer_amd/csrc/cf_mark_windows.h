// cf_mark_windows.h -- histone-mark coalitions whose players are WINDOWS of a region (cf_mark_window_coalitions, cf_mark_window_shapley,
// cf_mark_window_shapley_sampled; included by cf_api.hip behind cf_marks_wide.h).
//
// The game joins the wide game of cf_marks_wide.h with the window rule of cf_scan.h.  c = the coarsest resolution, W = n_bins[c],
// R_r = n_bins[r] / W.  Player p is (marks_p, regions_p, [lo_p, hi_p)): the marks of marks_p in the regions of regions_p over the coarse
// genomic bins lo_p .. hi_p - 1, 0 <= lo_p < hi_p <= W.  A coalition is kw = ceil(P / 32) words, bit set = player PRESENT.  Row (b, k)
// is the inference forward of gene b with, for every region rho and coarse genomic bin g,
//     gone(rho, g) = OR of marks_p over the absent players p with bit rho in regions_p and lo_p <= g < hi_p
// Region rho's real rows at resolution r are [q_r, q_r + n_r) and n_c is its real bin count at c (the centre pad-mask rows, as
// scan_extent reads them: holes inside count).  Genomic bin j is row q_r + j, or row q_r + n_r - 1 - j where flip[b] is set (the
// promoter only: a pCRE is never stored mirrored).  The element of a real row with genomic bin j and mark f, g = j / R_r, g < n_c and
// bit f in gone(rho, g) becomes
//     the scale rule   log1pf(s expm1f(u)), ig_signal of cf_ig.h: scaled ONCE however many absent players cover it
//     the donor rule   the bits of the donor's element at the same position (donor_elem of cf_marks.h)
// and every other element keeps its bits; masks and interaction_freq are the gene's own.  Bin sizes nest, so a window of coarse bins
// holds whole finer bins, and binning is linear per mark: either rule is exact in raw-signal space, as in cf_scan.h.  A window with
// lo_p >= n_c changes nothing (a dummy slot, a short pCRE, a narrowed promoter): such a player is a null player.
//   k_mark_window_expand         the grid (chunk row x resolution x kMarkSlices), the 256 threads and the slice-0 mask and frequency
//   k_mark_window_donor_expand   copies of k_mark_expand (one body, win_expand<DONOR>), in three phases:
//     1  extents   (q_r, n_r, n_c) of every region into LDS: wave w takes regions w, w + 4, ..., each with two shuffle reductions
//                  over mask rows read four bytes per load -- no block-wide barrier per region; the 4 P player words and the row's
//                  kw coalition words are staged in LDS on the way
//     2  table     gone[rho][g], T W <= 17 * 64 words of LDS, one thread per (rho, g) walking the P players (g >= n_c: 0), and a
//                  per-region "some word is non-zero" flag
//     3  copy      the workgroup's slice of the row's features, every element written once.  A region whose flag is clear is a plain
//                  float4 copy (the donor is not loaded); in a touched region every element takes the word of ITS row -- a float4
//                  spans up to two rows and two regions when F is no multiple of 4.  A segment whose length is no multiple of 4
//                  floats (or F < 4) goes element by element.
// No atomics, no scratch, 6,688 bytes of LDS (extents 204, table 4,352, flags 68, staged words 2,064); 48 / 36 VGPRs (scale / donor
// rule), 8 waves per SIMD.  The float4 walk is its own, not mark_copy's: an element's word comes from a table
// lookup per row here, from one word per region there.
#pragma once

namespace cf {

constexpr int kWinMaxW = 64;           // coarse bins per region the gone table holds
constexpr int kWinMaxT = kCoalMaxS + 1;

struct MarkWindowArgs {
    MarkExpandArgs m;                  // as for k_mark_expand; m.players: device [4 P]: marks_p, regions_p, lo_p, hi_p
    const uint8_t* pmc[kMaxRes];       // the promoter's centre pad-mask rows: pmc[r] + b * m.rows.pm_stride[r]
    const uint8_t* flip;               // device [B] or nullptr: the promoter of gene b is stored mirrored
    int W, rc;                         // n_bins of the coarsest resolution, its index
};

struct MarkWindowDonorArgs {
    MarkWindowArgs w;
    const float* pf_don[kMaxRes];      // the donor's promoter_feats [B, L, F]
    const float* cf_don[kMaxRes];      // pcre_feats [B, S, L, F]
};

struct WinTable {
    int ext[kWinMaxT][3];                  // q_r, n_r, n_c of region rho
    unsigned gone[kWinMaxT * kWinMaxW];    // gone[rho * W + g]
    unsigned any[kWinMaxT];                // some gone word of region rho is non-zero
    unsigned pl[4 * kMarkWideMaxP];        // the 4 P player words and
    unsigned kept[kMarkWideMaxP / 32];     // the row's coalition words: staged once, walked by T W threads
};

// phases 1 and 2: t filled for chunk row gv = (gene b, coalition gv - b n_coal) at resolution r; ends with a barrier
__device__ __forceinline__ void win_table(const MarkWindowArgs& wa, WinTable& t, int r, int b, long long gv) {
    const MarkExpandArgs& a = wa.m;
    const int tid = threadIdx.x, lane = tid & 63, S = a.rows.S, T = S + 1, P = a.P, W = wa.W, rc = wa.rc;
    for (int rho = tid >> 6; rho < T; rho += kIgxThreads / 64) {
        const uint8_t* mr = rho == 0 ? wa.pmc[r] + (size_t)b * a.rows.pm_stride[r] : a.rows.cm_in[r] + ((size_t)b * S + rho - 1) * a.rows.cm_stride[r];
        const uint8_t* mc = rho == 0 ? wa.pmc[rc] + (size_t)b * a.rows.pm_stride[rc] : a.rows.cm_in[rc] + ((size_t)b * S + rho - 1) * a.rows.cm_stride[rc];
        int lo, hi, clo, chi;
        win_extent(mr, a.rows.L[r], lane, lo, hi);
        if (r == rc) clo = lo, chi = hi;
        else win_extent(mc, a.rows.L[rc], lane, clo, chi);
        if (lane == 0) {
            t.ext[rho][0] = lo;
            t.ext[rho][1] = hi > lo ? hi - lo : 0;
            t.ext[rho][2] = chi > clo ? chi - clo : 0;
            t.any[rho] = 0u;
        }
    }
    const int kw = (P + 31) >> 5;
    for (int k = tid; k < 4 * P; k += kIgxThreads) t.pl[k] = a.players[k];
    if (tid < kw) t.kept[tid] = a.words[b * a.word_stride + (gv - (long long)b * a.n_coal) * kw + tid];
    __syncthreads();
    const unsigned* m = t.kept;
    const unsigned* pl = t.pl;
    for (int k = tid; k < T * W; k += kIgxThreads) {
        const int rho = k / W, g = k - rho * W;
        unsigned w = 0;
        if (g < t.ext[rho][2])
            for (int p = 0; p < P; ++p)
                if (!((m[p >> 5] >> (p & 31)) & 1u) && ((pl[P + p] >> rho) & 1u) && (int)pl[2 * P + p] <= g && g < (int)pl[3 * P + p]) w |= pl[p];
        t.gone[k] = w;
        if (w) t.any[rho] = 1u;      // (every writer stores the same value)
    }
    __syncthreads();
}

// gone(rho, g) of the genomic bin that row `row` of region rho holds at a resolution with R rows per coarse bin; 0 outside the real rows
__device__ __forceinline__ unsigned win_word(const WinTable& t, int rho, int row, int W, int R, bool flip) {
    const int n = t.ext[rho][1];
    int j = row - t.ext[rho][0];
    if (j < 0 || j >= n) return 0u;
    if (flip && rho == 0) j = n - 1 - j;
    return t.gone[rho * W + j / R];      // (j < n <= L: j / R < W; the table holds 0 from n_c on)
}

// dst[0, n) = src[0, n), n = a whole number of regions of LF = L F elements, the first of them region rho0.  DONOR: a changed element
// takes don's bits, else it is scaled by s.  The workgroup takes the blocks blockIdx.z, blockIdx.z + kMarkSlices, ... of kIgxThreads
// float4s (or floats), as mark_copy.
template <bool DONOR>
__device__ __forceinline__ void win_copy(const float* __restrict__ src, const float* __restrict__ don, float* __restrict__ dst, int n, int L, int F,
                                         int rho0, const WinTable& t, int W, bool flip, float s) {
    const int first = blockIdx.z * kIgxThreads + threadIdx.x, step = kMarkSlices * kIgxThreads, LF = L * F, R = L / W;
    const bool vec = (n & 3) == 0 && F >= 4 &&
                     ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst) | (DONOR ? reinterpret_cast<uintptr_t>(don) : 0)) & 15) == 0;
    if (vec) {
        const float4* s4 = reinterpret_cast<const float4*>(src);
        const float4* n4 = reinterpret_cast<const float4*>(don);
        float4* d4 = reinterpret_cast<float4*>(dst);
        for (int k = first; k < n / 4; k += step) {
            float4 x = s4[k];
            const int e = 4 * k, seg = e / LF, rem = e - seg * LF, rho = rho0 + seg;
            const int row = rem / F, f0 = rem - row * F;
            const int here = F - f0;                                 // elements here .. 3 of the float4 lie in the next row (F >= 4: one more row at most)
            const bool last = row + 1 == L;                          // ... which is row 0 of region rho + 1
            if (t.any[rho] | (here < 4 && last ? t.any[rho + 1] : 0u)) {
                const unsigned ga = win_word(t, rho, row, W, R, flip);
                const unsigned gb = here < 4 ? (last ? win_word(t, rho + 1, 0, W, R, flip) : win_word(t, rho, row + 1, W, R, flip)) : ga;
                if (ga | gb) {
                    const int f1 = f0 + 1 == F ? 0 : f0 + 1, f2 = f1 + 1 == F ? 0 : f1 + 1, f3 = f2 + 1 == F ? 0 : f2 + 1;
                    if (DONOR) {
                        const float4 d = n4[k];
                        x.x = donor_elem(x.x, d.x, ga, f0);
                        x.y = donor_elem(x.y, d.y, here > 1 ? ga : gb, f1);
                        x.z = donor_elem(x.z, d.z, here > 2 ? ga : gb, f2);
                        x.w = donor_elem(x.w, d.w, here > 3 ? ga : gb, f3);
                    } else {
                        x.x = mark_elem(x.x, ga, f0, s);
                        x.y = mark_elem(x.y, here > 1 ? ga : gb, f1, s);
                        x.z = mark_elem(x.z, here > 2 ? ga : gb, f2, s);
                        x.w = mark_elem(x.w, here > 3 ? ga : gb, f3, s);
                    }
                }
            }
            d4[k] = x;
        }
    } else {
        for (int e = first; e < n; e += step) {
            const int seg = e / LF, rem = e - seg * LF, rho = rho0 + seg, row = rem / F;
            float x = src[e];
            if (t.any[rho]) {
                const unsigned g = win_word(t, rho, row, W, R, flip);
                if (g) x = DONOR ? donor_elem(x, don[e], g, rem - row * F) : mark_elem(x, g, rem - row * F, s);
            }
            dst[e] = x;
        }
    }
}

template <bool DONOR>
__device__ __forceinline__ void win_expand(const MarkWindowArgs& wa, const float* const* pf_don, const float* const* cf_don, WinTable& t) {
    const MarkExpandArgs& a = wa.m;
    const MarkRow w = mark_row(a);
    const int r = w.r, b = w.b, i = w.i, L = a.rows.L[r], S = a.rows.S, F = a.F, LF = L * F;
    win_table(wa, t, r, b, w.gv);
    const bool fl = wa.flip && wa.flip[b];
    win_copy<DONOR>(a.pf_in[r] + (size_t)b * LF, DONOR ? pf_don[r] + (size_t)b * LF : nullptr, a.pf_out[r] + (size_t)i * LF, LF, L, F, 0, t, wa.W, fl,
                    a.scale);
    win_copy<DONOR>(a.cf_in[r] + (size_t)b * S * LF, DONOR ? cf_don[r] + (size_t)b * S * LF : nullptr, a.cf_out[r] + (size_t)i * S * LF, S * LF, L, F, 1,
                    t, wa.W, fl, a.scale);
    if (blockIdx.z == 0) rows_masks_freq(a.rows, a.freq_in, a.freq_out, r, b, i);
}

__global__ __launch_bounds__(kIgxThreads) void k_mark_window_expand(MarkWindowArgs wa) {
    __shared__ WinTable t;
    win_expand<false>(wa, nullptr, nullptr, t);
}

__global__ __launch_bounds__(kIgxThreads) void k_mark_window_donor_expand(MarkWindowDonorArgs da) {
    __shared__ WinTable t;
    win_expand<true>(da.w, da.pf_don, da.cf_don, t);
}

}  // namespace cf
