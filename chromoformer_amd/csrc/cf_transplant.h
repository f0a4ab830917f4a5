// cf_transplant.h -- pCRE transplant screen (cf_pcre_transplant; included by cf_api.hip behind cf_scan.h, whose k_scan_unpack it reuses).
//
// A library of C candidate regions ([C, L_r, F] features and [C, L_r] centre pad-mask rows per resolution) is tried in ONE pCRE slot of
// every gene, each candidate at Q contact frequencies: what would this gene's prediction be if that enhancer were brought into contact
// with its promoter?  Rows are (gene, variant) pairs, gene-major (gv = b * V + v, V = 1 + C * Q):
//   v = 0               gene b verbatim
//   v = 1 + c * Q + q   candidate c in slot j = the gene's slot at frequency f = freq[b, c, q]
// The rule of row (b, v >= 1) with a slot j >= 0 (transplant_slot: -1 = the gene has no slot to take, the row is gene b verbatim):
//   features       pcre_feats[r][b, j] = lib_feats[r][c]; the slot's centre pad-mask row = lib_mask[r][c]
//   interaction    per resolution, J = j + 1, dead(t) = im_r[b, t, t] for t != J: im_r[J, t] = im_r[t, J] = dead(t), im_r[J, J] = 0,
//                  every other entry unchanged (transplant_mask)
//   frequencies    freq'[0, J] = f, every other entry of row and column J is 0, the rest unchanged (transplant_freq)
// The Pairwise output of a slot depends on the promoter and on that slot alone and the Regulation stack has no positional encoding (the
// two facts k_scan_pack stands on), so the S = i_max slots of a pseudo-gene carry S different candidates through one trunk pass, and a
// candidate's trunk row serves all Q frequencies.  Pseudo rows are (gene, u) pairs, gene-major (gp = b * U + u, U = ceil(C / S)); slot
// s of pseudo row (b, u) is candidate u * S + s, a dummy (zero features, a fully masked row) past C.  Byte movers, no atomics, no LDS:
//   k_transplant_pack   per (pseudo row, resolution): gene b's promoter features and pad-mask rows verbatim, the S candidates' features
//                       and mask rows into the slots -- float4 where the row allows
//   k_scan_unpack       (cf_scan.h, V = C + 1) rows 1..S of the pseudo-gene's trunk output -> xv[(b, c)], one d_emb row per candidate
//   k_transplant_rows   per (row (b, v), resolution): the stashed trunk output of gene b -> Rx[r][0] with row J from xv (every element
//                       written once), the edited interaction mask, resolution 0 also the edited frequencies and, on v = 0, slot_out[b]
#pragma once

namespace cf {

struct TransplantPackArgs {
    const float* pf_in[kMaxRes];       // the caller's promoter_feats [B, L, F]
    float* pf_out[kMaxRes];            // the chunk's copies, [max_batch, L, F] / [max_batch, S, L, F]
    float* cf_out[kMaxRes];
    const float* lib_feats[kMaxRes];   // [C, L, F]
    const uint8_t* lib_mask[kMaxRes];  // [C, L]
    RowCopyArgs rows;                  // the promoter's pad masks in, both pad masks out (the interaction masks are not read by the trunk)
    int g0, U, C, F;
};

// dst[0, n) = src[0, n), or zeros (src == nullptr); float4 where n and both pointers allow
__device__ __forceinline__ void transplant_copy(const float* __restrict__ src, float* __restrict__ dst, int n) {
    const bool vec = (n & 3) == 0 && ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0;
    if (vec) {
        const float4* s4 = reinterpret_cast<const float4*>(src);
        float4* d4 = reinterpret_cast<float4*>(dst);
        for (int k = threadIdx.x; k < n / 4; k += kRowThreads) d4[k] = src ? s4[k] : make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
        for (int k = threadIdx.x; k < n; k += kRowThreads) dst[k] = src ? src[k] : 0.f;
    }
}

__global__ __launch_bounds__(kRowThreads) void k_transplant_pack(TransplantPackArgs a) {
    const int i = blockIdx.x, r = blockIdx.y;
    const int gp = a.g0 + i, b = gp / a.U, u = gp - b * a.U;
    const int L = a.rows.L[r], S = a.rows.S, LF = L * a.F, PL = a.rows.pm_rows[r] * L;
    transplant_copy(a.pf_in[r] + (size_t)b * LF, a.pf_out[r] + (size_t)i * LF, LF);
    for (int k = threadIdx.x; k < PL; k += kRowThreads) a.rows.pm_out[r][(size_t)i * PL + k] = a.rows.pm_in[r][(size_t)b * a.rows.pm_stride[r] + k];
    for (int s = 0; s < S; ++s) {
        const int c = u * S + s;      // (block-uniform)
        const bool real = c < a.C;
        transplant_copy(real ? a.lib_feats[r] + (size_t)c * LF : nullptr, a.cf_out[r] + ((size_t)i * S + s) * LF, LF);
        const uint8_t* __restrict__ m = a.lib_mask[r] + (size_t)(real ? c : 0) * L;
        uint8_t* __restrict__ mo = a.rows.cm_out[r] + ((size_t)i * S + s) * L;
        for (int k = threadIdx.x; k < L; k += kRowThreads) mo[k] = real ? m[k] : (uint8_t)1;
    }
}

struct TransplantRowsArgs {
    const float4* stash[kMaxRes];      // [B, T * D / 4]: the genes' own trunk output
    const float4* xv[kMaxRes];         // [B * C, D / 4]: the candidates' trunk rows behind gene b's promoter
    float4* x0[kMaxRes];               // Rx[r][0], rows of the chunk
    RowCopyArgs rows;                  // the interaction masks
    const uint8_t* im_coarse;          // the coarsest resolution's interaction mask [B, T, T] (append mode)
    const float* freq_in;              // [B, T, T]
    float* freq_out;
    const float* freq;                 // [B, C, Q]
    const int* slot;                   // device [B] or nullptr: slot_all for every gene
    int* slot_out;                     // device [B] or nullptr
    int slot_all, g0, V, C, Q, T, row4, d4;
};

// The slot gene b's transplants take, -1: none (block-uniform).  A slot[b] outside [-1, S) is -1; slot_all = -1 is "append": the
// first dead token t >= 1 of the coarsest resolution's interaction mask (its diagonal entry set), none: not placed.
__device__ __forceinline__ int transplant_slot(const TransplantRowsArgs& a, int b) {
    const int T = a.T;
    if (a.slot) {
        const int j = a.slot[b];
        return j >= 0 && j < T - 1 ? j : -1;
    }
    if (a.slot_all >= 0) return a.slot_all;
    const uint8_t* __restrict__ im = a.im_coarse + (size_t)b * T * T;
    for (int t = 1; t < T; ++t)
        if (im[t * (T + 1)]) return t - 1;
    return -1;
}

// entry (q, t) of the interaction mask of a row that holds a transplant in token J; im: the gene's own [T, T] mask at this resolution
__device__ __forceinline__ uint8_t transplant_mask(const uint8_t* __restrict__ im, int q, int t, int J, int T) {
    if (q != J && t != J) return im[q * T + t];
    if (q == t) return 0;
    const int o = q == J ? t : q;      // the other token: masked where it is dead
    return im[o * (T + 1)] ? 1 : 0;
}

// entry (q, t) of interaction_freq of such a row at frequency f; fr: the gene's own [T, T] frequencies
__device__ __forceinline__ float transplant_freq(const float* __restrict__ fr, int q, int t, int J, int T, float f) {
    if (q != J && t != J) return fr[q * T + t];
    return q == 0 && t == J ? f : 0.f;
}

__global__ __launch_bounds__(kRowThreads) void k_transplant_rows(TransplantRowsArgs a) {
    const int i = blockIdx.x, r = blockIdx.y;
    const int gv = a.g0 + i, b = gv / a.V, v = gv - b * a.V, T = a.T, TT = a.rows.TT;
    const int j = transplant_slot(a, b);
    const bool placed = v > 0 && j >= 0;
    const int c = placed ? (v - 1) / a.Q : 0, J = j + 1;
    const float4* __restrict__ src = a.stash[r] + (size_t)b * a.row4;
    const float4* __restrict__ var = a.xv[r] + ((size_t)b * a.C + c) * a.d4;
    float4* __restrict__ dst = a.x0[r] + (size_t)i * a.row4;
    const int k0 = placed ? J * a.d4 : a.row4;      // (not placed: no row is replaced)
    for (int k = threadIdx.x; k < a.row4; k += kRowThreads) dst[k] = k >= k0 && k < k0 + a.d4 ? var[k - k0] : src[k];
    if (!placed) {
        rows_interaction_mask(a.rows, r, b, i);
        if (r == 0) rows_copy_tt(a.freq_in, a.freq_out, b, i, TT);
    } else {
        const uint8_t* __restrict__ im = a.rows.im_in[r] + (size_t)b * TT;
        uint8_t* __restrict__ mo = a.rows.im_out[r] + (size_t)i * TT;
        for (int k = threadIdx.x; k < TT; k += kRowThreads) mo[k] = transplant_mask(im, k / T, k % T, J, T);
        if (r == 0) {
            const float f = a.freq[(size_t)b * (a.V - 1) + (v - 1)];      // [B, C, Q]: (c, q) = v - 1
            const float* __restrict__ fr = a.freq_in + (size_t)b * TT;
            float* __restrict__ fo = a.freq_out + (size_t)i * TT;
            for (int k = threadIdx.x; k < TT; k += kRowThreads) fo[k] = transplant_freq(fr, k / T, k % T, J, T, f);
        }
    }
    if (r == 0 && v == 0 && a.slot_out && threadIdx.x == 0) a.slot_out[b] = j;
}

}  // namespace cf
