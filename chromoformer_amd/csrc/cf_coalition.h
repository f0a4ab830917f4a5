// cf_coalition.h -- in-silico pCRE deletion, pCRE coalition forwards, exact Shapley values and pair epistasis (cf_pcre_ablation,
// cf_pcre_coalitions, cf_pcre_shapley, cf_pcre_epistasis; included by cf_api.hip behind cf_rows.h).
//
// Deleting pCRE slot j of gene b is exactly the reference forward on the same tensors with interaction_masks[b, 0, j+1, :] and
// interaction_masks[b, 0, :, j+1] set (data.py: a dummy slot is a masked row and column): the Embedding +
// Pairwise output of every slot depends on the promoter and that slot alone, and the Regulation stack has no positional encoding.
// A coalition is a 32-bit word m, bit j set = pCRE slot j kept.  Row (b, m) is the inference forward of gene b with its interaction
// mask (every resolution) OR-ed with row j+1 and column j+1 for every clear bit j < S.  The trunk runs once, its output (the
// Regulation input Rx[r][0], [B, T, d_emb] per resolution) is stashed, and the Regulation stack + head run on the B * n_coal rows,
// gene-major (row = b * n_coal + c), in chunks of at most max_batch rows.  cf_pcre_ablation is the fixed table of i_max + 2 words
//   v = 0            2^S - 1               the given mask (baseline)
//   v = 1 + j        2^S - 1 without bit j (slot j deleted)
//   v = i_max + 1    0                     rows and columns 1..i_max (promoter only)
// Kernels:
//   k_pcre_stash        Rx[r][0] -> stash[r], float4 per thread, blockIdx.y = resolution.  Bytes only.
//   k_coalition_expand  per (chunk row, resolution): the stashed rows of its gene -> Rx[r][0], the OR-ed mask from the row's word (read
//                       from a device table) -> the chunk's mask[r]; resolution 0 also copies the gene's interaction_freq.  Bytes
//                       and bit tests only.
//   k_shapley           per (gene, slot j): phi[b, j, o] = sum over m with bit j clear of w(|m|) (v[b, m | 1 << j, o] - v[b, m, o]),
//                       w(k) = k! (S - k - 1)! / S! (computed by the host in double, rounded to fp32, passed by value).  fp32
//                       throughout (the compiler fuses the accumulate, see shapley_player_sum); thread t sums the words of rank t,
//                       t + 256, ... in ascending order, then a fixed-order LDS tree: deterministic, no atomics.  All S slots are players: a dummy slot's
//                       differences are exact zeros, so its phi is exactly 0 and the live slots' values are those of the game
//                       among the live slots alone.
//   k_shapley_pairs     per (gene, pair i <= j) from k_shapley's table: the pairwise Shapley interaction index (sii) or the order-2
//                       Shapley-Taylor index (sti), see the kernel.
//   k_epistasis         per (gene, pair i <= j) from the pair-deletion rows (N = 2^S - 1; row 0: N, row 1 + i: N \ i, then N \ {i, j}
//                       for i < j in lexicographic order): eps[b, i, j, o] = ((v_N - v_{N\i}) - v_{N\j}) + v_{N\ij}, each operation
//                       rounded to fp32, written to [i, j] and [j, i]; the diagonal is v_N - v_{N\i}.
#pragma once

namespace cf {

constexpr int kCoalMaxS = 16;                // cf_create accepts i_max in 1..16
constexpr int kShapThreads = 256;
constexpr int kAblThreads = kRowThreads;

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

struct CoalExpandArgs {
    const float4* stash[kMaxRes];            // [B, T * D / 4] per resolution
    float4* x0[kMaxRes];                     // Rx[r][0], rows of the chunk
    const uint8_t* mask_in[kMaxRes];         // the caller's interaction_mask[r]   [B, T, T]
    uint8_t* mask_out[kMaxRes];              // the chunk's                        [n, T, T]
    const float* freq_in;                    // the caller's interaction_freq      [B, T, T]
    float* freq_out;                         // the chunk's                        [n, T, T]
    const unsigned* keep;                    // [n_coal] coalition words (device)
    long long g0;                            // first row of the chunk
    int n_coal, T;
    int row4;                                // T * D / 4
};

__global__ __launch_bounds__(kAblThreads) void k_coalition_expand(CoalExpandArgs a) {
    const int i = blockIdx.x, r = blockIdx.y, tid = threadIdx.x;
    const long long g = a.g0 + i;
    const int b = (int)(g / a.n_coal), T = a.T, TT = T * T;
    // bit 0 of `gone` is the promoter token (never deleted), bit j + 1 pCRE slot j
    const unsigned gone = ~(a.keep[g - (long long)b * a.n_coal] << 1) & ((1u << T) - 2u);
    rows_copy_x0(a.stash[r], a.x0[r], b, i, a.row4);
    const uint8_t* __restrict__ min = a.mask_in[r] + (size_t)b * TT;
    uint8_t* __restrict__ mout = a.mask_out[r] + (size_t)i * TT;
    for (int k = tid; k < TT; k += kAblThreads) {
        const int row = k / T, col = k - row * T;
        mout[k] = (gone >> row | gone >> col) & 1u ? (uint8_t)1 : min[k];
    }
    if (r == 0) rows_copy_tt(a.freq_in, a.freq_out, b, i, TT);
}

struct ShapleyArgs {
    const float* v;                          // [B, 2^S, n_out]: the logits of every coalition, indexed by the word
    float* phi;                              // [B, S, n_out]
    float w[kCoalMaxS];                      // w[k], k = |m| < S
    int S, n_out;
};

// One player's sum for output column o, by the whole workgroup: thread t sums the words of rank t, t + 256, ... with bit j clear in
// ascending order, then the fixed-order LDS tree.  On return red[0] holds the sum (a barrier has been passed; the caller passes another
// before red is written again).  Shared by k_shapley and the sii diagonal of k_shapley_pairs: the same operations in the same order,
// compiled the same way (the compiler fuses acc + w d into one v_fmac_f32 here, as it always has in k_shapley: one rounding fewer per
// term, inside every bound stated for phi; left as it is, since phi keeps its bits).
__device__ __forceinline__ void shapley_player_sum(const float* __restrict__ v, const float* sw, float* red, int S, int j, int n_out, int o, int tid) {
    const unsigned half = 1u << (S - 1), low = (1u << j) - 1u, bit = 1u << j;
    float acc = 0.f;
    for (unsigned q = tid; q < half; q += kShapThreads) {
        const unsigned m = (q & ~low) << 1 | (q & low);      // the q-th word with bit j clear
        const float d = __fsub_rn(v[(size_t)(m | bit) * n_out + o], v[(size_t)m * n_out + o]);
        acc = __fadd_rn(acc, __fmul_rn(sw[__popc(m)], d));
    }
    red[tid] = acc;
    __syncthreads();
    for (int s = kShapThreads / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] = __fadd_rn(red[tid], red[tid + s]);
        __syncthreads();
    }
}

__global__ __launch_bounds__(kShapThreads) void k_shapley(ShapleyArgs a) {
    __shared__ float sw[kCoalMaxS];
    __shared__ float red[kShapThreads];
    const int b = blockIdx.x, j = blockIdx.y, tid = threadIdx.x, S = a.S, n_out = a.n_out;
#pragma unroll
    for (int k = 0; k < kCoalMaxS; ++k)      // (constant indices into the kernel arguments: scalar loads, no private copy)
        if (tid == k) sw[k] = a.w[k];
    __syncthreads();
    const float* __restrict__ v = a.v + ((size_t)b << S) * n_out;
    for (int o = 0; o < n_out; ++o) {
        shapley_player_sum(v, sw, red, S, j, n_out, o, tid);
        if (tid == 0) a.phi[((size_t)b * S + j) * n_out + o] = red[0];
        __syncthreads();
    }
}

// k_shapley_pairs: the pairwise Shapley interaction index of every pair of players, a second reduction of k_shapley's table.  One
// workgroup per (gene, pair i <= j) -- blockIdx.y counts the pairs row by row of the upper triangle --, one pass over the table per
// output column, as k_shapley.  Off the diagonal, with S running over the 2^(P - 2) words that hold neither player,
//   delta(S)       = (v(S + i + j) - v(S + j)) - (v(S + i) - v(S))      the marginal contribution of i with j present, minus that with j absent
//   inter[b, i, j] = sum_S w2(|S|) delta(S)
// every operation rounded to fp32 (no contraction), thread t summing the subsets of rank t, t + 256, ... in ascending order, then
// k_shapley's LDS tree; written to [i, j] and [j, i].  In this grouping delta is exactly 0 when either player is null (its rows bit-equal
// present and absent): 0 - 0 when it is i, a - a when it is j.  The weight table alone tells the two indices apart:
//   sii  w2(s) = s! (P - s - 2)! / (P - 1)!;   the diagonal is k_shapley's phi[b, i], by shapley_player_sum on w1 (its weights)
//   sti  w2(s) = (2 / P) / C(P - 1, s);        the diagonal is v({i}) - v(0), one subtraction
// No atomics, no scratch: deterministic.
struct ShapleyPairsArgs {
    const float* v;                          // [B, 2^P, n_out]: the logits of every coalition, indexed by the word
    float* inter;                            // [B, P, P, n_out]
    float w1[kCoalMaxS];                     // k_shapley's w[k], k = |m| < P (the sii diagonal)
    float w2[kCoalMaxS];                     // w2[s], s = |S| <= P - 2
    int P, n_out;
    int sti;                                 // 0: sii, 1: sti
};

__global__ __launch_bounds__(kShapThreads) void k_shapley_pairs(ShapleyPairsArgs a) {
    __shared__ float sw[kCoalMaxS];
    __shared__ float red[kShapThreads];
    const int b = blockIdx.x, tid = threadIdx.x, P = a.P, n_out = a.n_out;
    int i = 0, j = blockIdx.y;               // row i of the upper triangle holds the P - i pairs (i, i), (i, i + 1), ...
    while (j >= P - i) j -= P - i, ++i;
    j += i;
    const bool diag = i == j;
#pragma unroll
    for (int k = 0; k < kCoalMaxS; ++k)      // (constant indices into the kernel arguments: scalar loads, no private copy)
        if (tid == k) sw[k] = diag ? a.w1[k] : a.w2[k];
    __syncthreads();
    const float* __restrict__ v = a.v + ((size_t)b << P) * n_out;
    float* __restrict__ out = a.inter + (size_t)b * P * P * n_out;
    if (diag) {
        if (a.sti) {
            for (int o = tid; o < n_out; o += kShapThreads) out[((size_t)i * P + i) * n_out + o] = __fsub_rn(v[((size_t)1 << i) * n_out + o], v[o]);
            return;
        }
        for (int o = 0; o < n_out; ++o) {
            shapley_player_sum(v, sw, red, P, i, n_out, o, tid);
            if (tid == 0) out[((size_t)i * P + i) * n_out + o] = red[0];
            __syncthreads();
        }
        return;
    }
    const unsigned quarter = 1u << (P - 2), lowi = (1u << i) - 1u, lowj = (1u << j) - 1u, bi = 1u << i, bj = 1u << j;
    for (int o = 0; o < n_out; ++o) {
        // plain operators under contract(off): each is one fp32 rounding.  (__fmul_rn / __fadd_rn are inline `*` and `+` of a header
        // compiled under the default contract(fast): the compiler fuses them into v_fmac_f32, as in shapley_player_sum.)
#pragma clang fp contract(off)
        float acc = 0.f;
        for (unsigned q = tid; q < quarter; q += kShapThreads) {
            const unsigned m1 = (q & ~lowi) << 1 | (q & lowi);        // a zero opened at bit i,
            const unsigned m = (m1 & ~lowj) << 1 | (m1 & lowj);      // then at bit j > i: the q-th word with bits i and j clear
            const float with_j = v[(size_t)(m | bi | bj) * n_out + o] - v[(size_t)(m | bj) * n_out + o];
            const float without_j = v[(size_t)(m | bi) * n_out + o] - v[(size_t)m * n_out + o];
            const float delta = with_j - without_j;
            const float term = sw[__popc(m)] * delta;
            acc = acc + term;
        }
        red[tid] = acc;
        __syncthreads();
        for (int s = kShapThreads / 2; s > 0; s >>= 1) {
            if (tid < s) red[tid] = __fadd_rn(red[tid], red[tid + s]);
            __syncthreads();
        }
        if (tid == 0) {
            const float x = red[0];
            out[((size_t)i * P + j) * n_out + o] = x;
            out[((size_t)j * P + i) * n_out + o] = x;
        }
        __syncthreads();
    }
}

struct EpistasisArgs {
    const float* v;                          // [B, 1 + S + S (S - 1) / 2, n_out]: the pair-deletion rows
    float* eps;                              // [B, S, S, n_out]
    int B, S, n_out;
};

__global__ __launch_bounds__(kShapThreads) void k_epistasis(EpistasisArgs a) {
    const int S = a.S, n_out = a.n_out, R = 1 + S + S * (S - 1) / 2;
    const long long n = (long long)a.B * S * S * n_out;
    for (long long e = (long long)blockIdx.x * kShapThreads + threadIdx.x; e < n; e += (long long)gridDim.x * kShapThreads) {
        const int o = (int)(e % n_out);
        long long t = e / n_out;
        const int c = (int)(t % S);
        t /= S;
        const int r = (int)(t % S), b = (int)(t / S);
        const int i = r < c ? r : c, j = r < c ? c : r;      // [j, i] carries the bits of [i, j]
        const float* __restrict__ v = a.v + (size_t)b * R * n_out + o;
        float x = __fsub_rn(v[0], v[(size_t)(1 + i) * n_out]);
        if (i < j) {
            const int p = 1 + S + i * S - i * (i + 1) / 2 + (j - i - 1);      // pairs before row i: i S - i (i + 1) / 2
            x = __fadd_rn(__fsub_rn(x, v[(size_t)(1 + j) * n_out]), v[(size_t)p * n_out]);
        }
        a.eps[e] = x;
    }
}

}  // namespace cf
