// cf_rows.h -- a chunk of rows copied from the caller's batch: what the expand kernels of the attribution entry points share
// (cf_coalition.h, cf_ig.h, cf_scan.h, cf_transplant.h, cf_scan_fine.h and the mark games cf_marks.h, cf_mark_windows.h, cf_mark_fine.h; included by
// cf_api.hip in front of them).  Chunk row i is a copy of gene b; blockIdx.y is the resolution r.  Bytes only, kRowThreads threads per
// workgroup.  Also here: rows_masks_freq, the three copies that close the mark and scan expand kernels, and win_extent, the real rows of
// a pad-mask row by one wave (the window and fine games).
#pragma once

namespace cf {

constexpr int kRowThreads = 256;

struct RowCopyArgs {
    const uint8_t* pm_in[kMaxRes];     // the caller's pad-mask centre rows (promoter: row = gene; pCRE: row = gene * S + slot)
    const uint8_t* cm_in[kMaxRes];
    long long pm_stride[kMaxRes], cm_stride[kMaxRes];
    uint8_t* pm_out[kMaxRes];          // the chunk's compact rows, stride L
    uint8_t* cm_out[kMaxRes];
    int pm_rows[kMaxRes];              // 1; L where the all-rows Embedding reads the caller's full [B, L, L] promoter mask: pm_in is then
                                       // row 0 of gene 0 and the chunk's copy keeps all L rows per chunk row (stride L * L)
    const uint8_t* im_in[kMaxRes];     // interaction masks [B, T, T]
    uint8_t* im_out[kMaxRes];
    int L[kMaxRes];
    int S, TT;
};

// the promoter and pCRE pad-mask rows
__device__ __forceinline__ void rows_pad_masks(const RowCopyArgs& a, int r, int b, int i) {
    const int L = a.L[r], S = a.S, PL = a.pm_rows[r] * L;
    for (int k = threadIdx.x; k < PL; k += kRowThreads) a.pm_out[r][(size_t)i * PL + k] = a.pm_in[r][(size_t)b * a.pm_stride[r] + k];
    for (int k = threadIdx.x; k < S * L; k += kRowThreads) {
        const int s = k / L, j = k - s * L;
        a.cm_out[r][((size_t)i * S + s) * L + j] = a.cm_in[r][((size_t)b * S + s) * a.cm_stride[r] + j];
    }
}

__device__ __forceinline__ void rows_interaction_mask(const RowCopyArgs& a, int r, int b, int i) {
    for (int k = threadIdx.x; k < a.TT; k += kRowThreads) a.im_out[r][(size_t)i * a.TT + k] = a.im_in[r][(size_t)b * a.TT + k];
}

// out[i] = in[b], [T, T] floats (interaction_freq)
__device__ __forceinline__ void rows_copy_tt(const float* in, float* out, int b, int i, int TT) {
    for (int k = threadIdx.x; k < TT; k += kRowThreads) out[(size_t)i * TT + k] = in[(size_t)b * TT + k];
}

// what closes an expand kernel: chunk row i's compact pad-mask rows and interaction mask, at resolution 0 its interaction_freq
__device__ __forceinline__ void rows_masks_freq(const RowCopyArgs& a, const float* freq_in, float* freq_out, int r, int b, int i) {
    rows_pad_masks(a, r, b, i);
    rows_interaction_mask(a, r, b, i);
    if (r == 0) rows_copy_tt(freq_in, freq_out, b, i, a.TT);
}

// first unmasked byte and one past the last of a mask row of L bytes, by one wave (lo = L, hi = 0: all masked); every lane gets the result
__device__ __forceinline__ void win_extent(const uint8_t* __restrict__ m, int L, int lane, int& lo, int& hi) {
    int a = L, b = 0;
    if ((L & 3) == 0 && (reinterpret_cast<uintptr_t>(m) & 3) == 0) {      // four mask bytes per load: L = 400 in two rounds, not seven
        const unsigned* __restrict__ m4 = reinterpret_cast<const unsigned*>(m);
        for (int k = lane; k < L / 4; k += 64) {
            const unsigned w = m4[k];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (!((w >> (8 * j)) & 0xFFu)) a = min(a, 4 * k + j), b = max(b, 4 * k + j + 1);
        }
    } else {
        for (int k = lane; k < L; k += 64)
            if (!m[k]) a = min(a, k), b = max(b, k + 1);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) a = min(a, __shfl_xor(a, o, 64)), b = max(b, __shfl_xor(b, o, 64));
    lo = a, hi = b;
}

// x0[i] = stash[b]: the stashed trunk output of gene b into the Regulation input Rx[r][0] of chunk row i, row4 = T * D / 4
__device__ __forceinline__ void rows_copy_x0(const float4* stash, float4* x0, int b, int i, int row4) {
    const float4* __restrict__ src = stash + (size_t)b * row4;
    float4* __restrict__ dst = x0 + (size_t)i * row4;
    for (int k = threadIdx.x; k < row4; k += kRowThreads) dst[k] = src[k];
}

}  // namespace cf
