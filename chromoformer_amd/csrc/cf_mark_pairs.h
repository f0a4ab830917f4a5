// cf_mark_pairs.h -- permutation-sampled pairwise Shapley interaction indices of a few FOCAL players of a wide mark game
// (cf_mark_*_shapley_interactions_sampled, cf_perm_interactions_from_rows; included by cf_api.hip behind cf_marks_wide.h).
//
// 2^P coalitions cannot be enumerated and a full P x P matrix costs O(P^2) forwards per order, so the index is ESTIMATED for the rows
// of a few focal players.  Fix a focal player i and an order pi of all P players; o = pi with i removed, T_k the first k players of o,
// r the position of i in pi.  For j = o[a]:
//     d(j) = (v(T_{a+1} + i) - v(T_{a+1})) - (v(T_a + i) - v(T_a))        i's marginal with j present, minus that with j absent
// Over uniform orders T_a has the law a! (P - 2 - a)! / (P - 1)!, the weight of the Shapley interaction index: the mean of d(j) over the
// orders is unbiased for "sii", and w_a d(j) with w_a = 2 (P - 1 - a) / P for Shapley-Taylor of order 2 ("sti").  One order gives one
// sample for every j at once.  The estimate is NOT symmetric: inter[i, j] (focal i) and inter[j, i] (focal j) are different samples.
//   rows of gene b   the table of k_perm_shapley (cf_marks_wide.h: nobody, everybody, the prefixes of every order) UNCHANGED, then per
//                    focal player {i} alone, everybody but i, and per order the rows T_k + i (k = 1 .. r - 1) and T_k
//                    (k = r + 1 .. P - 2) that are no prefix of pi: T_k = pi[:k] for k <= r, T_k + i = pi[:k + 1] for k >= r.
//   col              uint32 [n_focal, n_perm, P, 2], built by the host: col[f, q, k, 0] the column of v(T_k), col[f, q, k, 1] that of
//                    v(T_k + i), k = 0 .. P - 1.  The kernel reads columns through this table and does no layout arithmetic.
//   k_perm_pairs     per (gene, focal f, player j), rank the inverse permutations (bytes), a = rank_q[j] - (rank_q[j] > r):
//                        d_q = (v[col(a + 1, 1)] - v[col(a + 1, 0)]) - (v[col(a, 1)] - v[col(a, 0)])        three fp32 subtractions
//                        s_q = d_q ("sii"), w_a d_q ("sti": one rounded product)
//                        inter = (sum_q s_q) / n_perm,   se = sqrt(sum_q (s_q - inter)^2 / (n_perm (n_perm - 1)))   0 for n_perm = 1
//                    in the operations and the order of k_perm_shapley: thread t sums q = t, t + kShapThreads, ..., then the LDS tree.
//                    Every operation is rounded on its own (fp contraction off in this kernel); the quotient and the root of se go
//                    through double, which rounds both correctly.
//                    The "sii" diagonal alone goes through perm_mean_se (cf_marks_wide.h), the function k_perm_shapley itself is:
//                    that kernel's bits by construction (e e fused into the sum of squares, the approximate root of __fsqrt_rn).
//                    No atomics, no scratch.  The diagonal j = i: "sii" s_q = v[col(r, 1)] - v[col(r, 0)], i's marginal at its own
//                    position -- the columns k_perm_shapley reads, so the bits of its phi and se; "sti" v({i}) - v(nobody), se 0.
//                    A null i has both marginals exactly 0, a null j makes them the same float: d_q = 0 bit for bit either way.
#pragma once

namespace cf {

struct PermPairsArgs {
    const float* v;                          // [B, R, n_out]: the rows
    const uint8_t* rank;                     // [n_perm, P]: rank[q, p] = the position of player p in permutation q
    const unsigned* col;                     // [n_focal, n_perm, P, 2]: the columns of v(T_k) and v(T_k + i)
    float* inter;                            // [B, n_focal, P, n_out]
    float* se;                               // [B, n_focal, P, n_out], or null
    size_t R;                                // rows per gene
    float n, nn1;                            // n_perm and n_perm (n_perm - 1) as floats (the host rounds them once)
    int P, n_perm, n_out, n_focal, sti;
    uint8_t focal[kMarkWideMaxP];            // [n_focal]: the focal players
    float w[kMarkWideMaxP];                  // "sti": w[a] = 2 (P - 1 - a) / P, in double, rounded to fp32
};

// One rounded operation each.  (This toolchain's __fadd_rn / __fsub_rn / __fmul_rn are plain operators in a header compiled with
// contraction allowed: once inlined, a product fuses into the sum behind it.  The pragma is lexical.)
__device__ __forceinline__ float pp_add(float x, float y) {
#pragma clang fp contract(off)
    return x + y;
}
__device__ __forceinline__ float pp_sub(float x, float y) {
#pragma clang fp contract(off)
    return x - y;
}
__device__ __forceinline__ float pp_mul(float x, float y) {
#pragma clang fp contract(off)
    return x * y;
}

__global__ __launch_bounds__(kShapThreads) void k_perm_pairs(PermPairsArgs a) {
    __shared__ float red[kShapThreads];
    const int b = blockIdx.x, f = blockIdx.y / a.P, j = blockIdx.y % a.P, tid = threadIdx.x, P = a.P, n_perm = a.n_perm, n_out = a.n_out;
    const int i = a.focal[f];
    const bool diag = i == j;
    const float* __restrict__ v = a.v + (size_t)b * a.R * n_out;
    const unsigned* __restrict__ col = a.col + (size_t)f * n_perm * P * 2;
    const size_t at0 = (((size_t)b * a.n_focal + f) * P + j) * n_out;
    if (diag && a.sti) {      // v({i}) - v(nobody): the rows of k = 0, the same in every order
        for (int o = tid; o < n_out; o += kShapThreads) {
            a.inter[at0 + o] = pp_sub(v[(size_t)col[1] * n_out + o], v[(size_t)col[0] * n_out + o]);
            if (a.se) a.se[at0 + o] = 0.f;
        }
        return;
    }
    if (diag) {      // "sii": i's marginal at its own position, through k_perm_shapley's own function: that kernel's bits
        for (int o = 0; o < n_out; ++o)
            perm_mean_se(n_perm, a.n, a.nn1, red,
                         [&](int q) {
                             const unsigned* c = col + ((size_t)q * P + a.rank[(size_t)q * P + i]) * 2;
                             return __fsub_rn(v[(size_t)c[1] * n_out + o], v[(size_t)c[0] * n_out + o]);
                         },
                         a.inter + at0 + o, a.se ? a.se + at0 + o : nullptr);
        return;
    }
    // the sample of order q at output o
    auto sample = [&](int q, int o) -> float {
        const int r = a.rank[(size_t)q * P + i], rj = a.rank[(size_t)q * P + j], k = rj - (rj > r);
        const unsigned* c = col + ((size_t)q * P + k) * 2;
        const float with_j = pp_sub(v[(size_t)c[3] * n_out + o], v[(size_t)c[2] * n_out + o]);
        const float without_j = pp_sub(v[(size_t)c[1] * n_out + o], v[(size_t)c[0] * n_out + o]);
        const float d = pp_sub(with_j, without_j);
        return a.sti ? pp_mul(a.w[k], d) : d;
    };
    for (int o = 0; o < n_out; ++o) {
        float acc = 0.f;
        for (int q = tid; q < n_perm; q += kShapThreads) acc = pp_add(acc, sample(q, o));
        red[tid] = acc;
        __syncthreads();
        for (int s = kShapThreads / 2; s > 0; s >>= 1) {
            if (tid < s) red[tid] = pp_add(red[tid], red[tid + s]);
            __syncthreads();
        }
        const float mean = __fdiv_rn(red[0], a.n);
        __syncthreads();
        if (tid == 0) a.inter[at0 + o] = mean;
        if (!a.se) continue;
        acc = 0.f;
        for (int q = tid; q < n_perm; q += kShapThreads) {
            const float e = pp_sub(sample(q, o), mean);
            acc = pp_add(acc, pp_mul(e, e));
        }
        red[tid] = acc;
        __syncthreads();
        for (int s = kShapThreads / 2; s > 0; s >>= 1) {
            if (tid < s) red[tid] = pp_add(red[tid], red[tid + s]);
            __syncthreads();
        }
        // the quotient and the root through double, which rounds a float quotient and a float root correctly (53 >= 2 * 24 + 2)
        if (tid == 0) a.se[at0 + o] = n_perm > 1 ? (float)sqrt((double)(float)((double)red[0] / (double)a.nn1)) : 0.f;
        __syncthreads();
    }
}

}  // namespace cf
