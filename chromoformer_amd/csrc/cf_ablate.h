// cf_ablate.h -- in-silico pCRE deletion (cf_pcre_ablation; included by cf_api.hip).
//
// Deleting pCRE slot j of gene b is exactly the reference forward on the same tensors with interaction_masks[b, 0, j+1, :] and
// interaction_masks[b, 0, :, j+1] set (data.py: a dummy slot is a masked row and column): the Embedding +
// Pairwise output of every slot depends on the promoter and that slot alone, and the Regulation stack has no positional encoding.
// So the trunk runs once, its output (the Regulation input Rx[r][0], [B, T, d_emb] per resolution) is stashed, and the Regulation
// stack + head run on B * V gene-variants, V = i_max + 2, gene-major (gv = b * V + v):
//   v = 0            the given mask (baseline)
//   v = 1 + j        given mask OR row j+1 OR column j+1 (slot j deleted)
//   v = i_max + 1    given mask OR rows and columns 1..i_max (promoter only)
// in chunks of at most max_batch gene-variants.  Both kernels move bytes only (no arithmetic, no atomics):
//   k_pcre_stash   Rx[r][0] -> stash[r], float4 per thread, blockIdx.y = resolution;
//   k_pcre_expand  per (chunk gene-variant, resolution): the stashed rows of its gene -> Rx[r][0], the OR-ed mask -> the chunk's
//                  mask[r]; resolution 0 also copies the gene's interaction_freq -> the chunk's freq.
#pragma once

namespace cf {

constexpr int kAblThreads = 256;

struct AblateStashArgs {
    const float4* src[kMaxRes];              // Rx[r][0]           [B * T * D / 4]
    float4* dst[kMaxRes];                    // stash of resolution r
    long long n4;                            // B * T * D / 4
};

__global__ __launch_bounds__(kAblThreads) void k_pcre_stash(AblateStashArgs a) {
    const int r = blockIdx.y;
    const float4* __restrict__ src = a.src[r];
    float4* __restrict__ dst = a.dst[r];
    for (long long i = (long long)blockIdx.x * kAblThreads + threadIdx.x; i < a.n4; i += (long long)gridDim.x * kAblThreads) dst[i] = src[i];
}

struct AblateExpandArgs {
    const float4* stash[kMaxRes];            // [B, T * D / 4] per resolution
    float4* x0[kMaxRes];                     // Rx[r][0], rows of the chunk's gene-variants
    const uint8_t* mask_in[kMaxRes];         // the caller's interaction_mask[r]   [B, T, T]
    uint8_t* mask_out[kMaxRes];              // the chunk's                        [n, T, T]
    const float* freq_in;                    // the caller's interaction_freq      [B, T, T]
    float* freq_out;                         // the chunk's                        [n, T, T]
    int g0;                                  // first gene-variant of the chunk
    int V, S, T;
    int row4;                                // T * D / 4
};

__global__ __launch_bounds__(kAblThreads) void k_pcre_expand(AblateExpandArgs a) {
    const int i = blockIdx.x, r = blockIdx.y, tid = threadIdx.x;
    const int gv = a.g0 + i, b = gv / a.V, v = gv - b * a.V, T = a.T, TT = T * T, S = a.S;
    const float4* __restrict__ src = a.stash[r] + (size_t)b * a.row4;
    float4* __restrict__ dst = a.x0[r] + (size_t)i * a.row4;
    for (int k = tid; k < a.row4; k += kAblThreads) dst[k] = src[k];
    const uint8_t* __restrict__ min = a.mask_in[r] + (size_t)b * TT;
    uint8_t* __restrict__ mout = a.mask_out[r] + (size_t)i * TT;
    for (int k = tid; k < TT; k += kAblThreads) {
        const int row = k / T, col = k - row * T;
        const bool del = v <= S ? v > 0 && (row == v || col == v) : row > 0 || col > 0;
        mout[k] = del ? (uint8_t)1 : min[k];
    }
    if (r == 0)
        for (int k = tid; k < TT; k += kAblThreads) a.freq_out[(size_t)i * TT + k] = a.freq_in[(size_t)b * TT + k];
}

}  // namespace cf
