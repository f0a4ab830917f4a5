// cf_marks_wide.h -- histone-mark coalitions over up to 128 players and their permutation-sampled Shapley values
// (cf_mark_coalitions_wide, cf_mark_shapley_sampled; included by cf_api.hip behind cf_marks.h).
//
// The game is that of cf_marks.h -- the same (marks_p, regions_p) player words, the same gone(rho), the same scale rule and donor rule,
// element by element -- with more players than one word holds: "mark f in region rho" is n_feats (i_max + 1) players, 63 on the default
// model, 119 at i_max = 16.  A coalition over P <= kMarkWideMaxP players is kw = ceil(P / 32) consecutive 32-bit words, bit p % 32 of
// word p / 32 set = player p PRESENT; row (b, k) reads words [k kw, (k + 1) kw) of the device table.
// The rows are built by k_mark_expand / k_mark_donor_expand of cf_marks.h themselves: mark_gone reads the row's kw words, and the narrow
// game is the case kw = 1.
// 2^P coalitions cannot be enumerated, so the Shapley values are ESTIMATED from n_perm orders of adding the players (permutations):
//   rows of gene b   column 0 nobody present, column 1 everybody (both shared by all permutations), column 2 + q (P - 1) + (k - 1) the
//                    first k players of permutation q, k = 1 .. P - 1: R = 2 + n_perm (P - 1) rows
//   k_perm_shapley   per (gene, player p), rank_q[p] = r the position of p in permutation q (bytes, the inverse permutations):
//                        d_q = v[col(q, r + 1)] - v[col(q, r)]                              one fp32 subtraction
//                        phi = (sum_q d_q) / n_perm
//                        se  = sqrt(sum_q (d_q - phi)^2 / (n_perm (n_perm - 1)))            0 for n_perm = 1
//                    each operation rounded to fp32, a fixed order: thread t sums q = t, t + kShapThreads, ..., then the LDS tree of
//                    k_shapley.  No atomics.  A player whose two adjacent rows carry the same bits in every permutation has d_q = 0
//                    throughout: phi and se exactly 0.  Efficiency telescopes within every permutation: sum_p phi = v_N - v_0 up to
//                    rounding.  The SAMPLING error is what se reports; nothing in the code bounds it.
#pragma once

namespace cf {

constexpr int kMarkWideMaxP = 128;     // players of the wide game: four words

struct PermShapleyArgs {
    const float* v;                          // [B, R, n_out], R = 2 + n_perm (P - 1): the prefix rows
    const uint8_t* rank;                     // [n_perm, P]: rank[q, p] = the position of player p in permutation q
    float* phi;                              // [B, P, n_out]
    float* se;                               // [B, P, n_out], or null
    float n, nn1;                            // n_perm and n_perm (n_perm - 1) as floats (the host rounds them once)
    int P, n_perm, n_out;
    size_t stride;                           // rows per gene of `v`; 0: R (a longer table leads with the prefix rows: cf_mark_pairs.h)
};

// The estimator of one (gene, player, output) by one workgroup: d(q) is the sample of order q (one fp32 subtraction), `red` kShapThreads
// floats of LDS.  Writes the mean, and the standard error if se_at is not null.  k_perm_shapley and the "sii" diagonal of k_perm_pairs
// (cf_mark_pairs.h) both call it, so the two carry the same bits.  The square e e is fused into the sum of squares with an explicit
// fmaf: what the compiler made of the separate __fmul_rn / __fadd_rn (plain operators here) before this function existed, written
// down so that it no longer depends on the compiler; the root is __fsqrt_rn (the hardware's approximate v_sqrt_f32 in this toolchain).
template <class Sample>
__device__ __forceinline__ void perm_mean_se(int n_perm, float n, float nn1, float* red, Sample d, float* mean_at, float* se_at) {
    const int tid = threadIdx.x;
    float acc = 0.f;
    for (int q = tid; q < n_perm; q += kShapThreads) acc = __fadd_rn(acc, d(q));
    red[tid] = acc;
    __syncthreads();
    for (int s = kShapThreads / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] = __fadd_rn(red[tid], red[tid + s]);
        __syncthreads();
    }
    const float phi = __fdiv_rn(red[0], n);
    __syncthreads();
    if (tid == 0) *mean_at = phi;
    if (!se_at) return;
    acc = 0.f;
    for (int q = tid; q < n_perm; q += kShapThreads) {
        const float e = __fsub_rn(d(q), phi);
        acc = fmaf(e, e, acc);
    }
    red[tid] = acc;
    __syncthreads();
    for (int s = kShapThreads / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] = __fadd_rn(red[tid], red[tid + s]);
        __syncthreads();
    }
    if (tid == 0) *se_at = n_perm > 1 ? __fsqrt_rn(__fdiv_rn(red[0], nn1)) : 0.f;
    __syncthreads();
}

__global__ __launch_bounds__(kShapThreads) void k_perm_shapley(PermShapleyArgs a) {
    __shared__ float red[kShapThreads];
    const int b = blockIdx.x, p = blockIdx.y, P = a.P, n_perm = a.n_perm, n_out = a.n_out;
    const size_t R = a.stride ? a.stride : 2 + (size_t)n_perm * (P - 1);
    const float* __restrict__ v = a.v + (size_t)b * R * n_out;
    // the column of the first k players of permutation q: nobody, everybody, else the permutation's own row
    auto col = [&](int q, int k) -> size_t { return k == 0 ? 0 : k == P ? 1 : 2 + (size_t)q * (P - 1) + (k - 1); };
    for (int o = 0; o < n_out; ++o) {
        const size_t at = ((size_t)b * P + p) * n_out + o;
        perm_mean_se(n_perm, a.n, a.nn1, red,
                     [&](int q) {
                         const int r = a.rank[(size_t)q * P + p];
                         return __fsub_rn(v[col(q, r + 1) * n_out + o], v[col(q, r) * n_out + o]);
                     },
                     a.phi + at, a.se ? a.se + at : nullptr);
    }
}

}  // namespace cf
