// cf_bin_spread.h -- per-bin integrated gradients spread over the difference of two raw signals (cf_bin_spread_difference; included
// by cf_kernels.h after cf_bin_grad.h, whose BinPlan / limits it shares).
//
// The donor path of cf_ig.h leaves, per bin of every resolution, cmean = C with attr = (m - md) C: integrated gradients with respect
// to the bin mean along md + a (m - md).  A bin mean is the sum of its samples over their count, so sample s of feature row f of the
// window [col0, col0 + ncols) of the two raw signals x, xd receives
//     draw[f, s] = (x[f, s] - xd[f, s]) ((C_0[p_0(s), f] / cnt_0 + C_1[p_1(s), f] / cnt_1) + C_2[p_2(s), f] / cnt_2)
// coarsest resolution first, fp32, every operation rounded (no contraction): seven roundings for three resolutions.  With the
// geometry of the binning (cf_bin_grad.h): g_r(s) = s / b_r, n_r = min(ceil(ncols / b_r), L_r) real bins, left_r = ceil((L_r - n_r) / 2),
// p_r = left_r + g_r (or L_r - 1 - that for a mirrored region), cnt_r = min((g_r + 1) b_r, ncols) - g_r b_r.  A sample past the last
// real bin of a resolution gets nothing from it; a null cmean[r] counts as zero; a null raw_donor is the zero signal.  Per bin the
// samples' shares sum to attr; draw is in raw (genomic) orientation, window-relative.
//
// Nothing is summed: cnt is geometric and C arrives per bin, so there are no LDS coefficients and no barrier.  A lane owns the 4
// consecutive window samples of one chunk and walks the feature rows; bin sizes that nest and are multiples of 4 put the 4 samples
// in one bin of every resolution.  One-pass path per lane and row: one 8-byte load from each signal, at most three cached gathers of
// cmean, one 16-byte store, unit stride across lanes: 4 bytes in and 4 bytes out per sample.  Rows that are not 8-byte aligned, a
// draw that is not 16-byte aligned, ld_out % 4 != 0 or bin sizes that do not nest take the per-sample walk of the same lanes.  Every
// window sample is written exactly once by exactly one lane: no atomics, run-to-run bit-identical.
#pragma once

namespace cf {

struct BinSpreadJob {                    // = cf_bin_spread_job of the C ABI
    const void* raw;                     // the gene's fp16 [F, ld]
    long long ld;
    const void* raw_donor;               // the donor's, same col0 / ncols; nullptr: the zero signal
    long long ld_donor;
    int col0, ncols;
    int flip, reserved;
    const float* cmean[kBinMaxRes];      // [L_r, F], coarsest first
    float* draw;                         // [F, ld_out]
    long long ld_out;
};

// where sample s of the window sits at resolution r: the offset of cmean[r][p, 0], or -1 (no real bin); *cnt: its bin's sample count
__device__ __forceinline__ int bin_spread_at(const BinPlan& pl, int r, int ncols, int flip, int s, float* cnt) {
    const int b = pl.b[r], L = pl.L[r];
    const int n_all = min((ncols + b - 1) / b, L);
    const int g = s / b;
    *cnt = (float)min(b, ncols - g * b);
    if (g >= n_all) return -1;
    const int q = (L - n_all + 1) / 2 + g;
    return (flip ? L - 1 - q : q) * pl.F;
}

// (C_0 / cnt_0 + C_1 / cnt_1) + C_2 / cnt_2 of feature row f; a missing term is 0
__device__ __forceinline__ float bin_spread_sum(const BinSpreadJob& j, int nres, const int (&at)[kBinMaxRes], const float (&cnt)[kBinMaxRes], int f) {
#pragma clang fp contract(off)
    float v = 0.f;
#pragma unroll
    for (int r = 0; r < kBinMaxRes; ++r) {
        if (r >= nres) break;
        const float* c = j.cmean[r];
        const float t = c && at[r] >= 0 ? *(const CF_GLOBAL float*)(c + at[r] + f) / cnt[r] : 0.f;
        v = r == 0 ? t : v + t;
    }
    return v;
}

// grid = (ceil(chunks of the longest window / 256), regions); a lane per chunk of 4 window samples
__global__ __launch_bounds__(256) void k_bin_spread_diff(const BinSpreadJob* __restrict__ jobs, BinPlan pl) {
#pragma clang fp contract(off)
    const BinSpreadJob j = jobs[blockIdx.y];
    const int ncols = j.ncols;
    const int s0 = 4 * (blockIdx.x * 256 + threadIdx.x);
    if (s0 >= ncols) return;                                                 // (also ncols <= 0: nothing to write)
    const int F = pl.F, nres = pl.n_res, rem = ncols - s0;
    const _Float16* x = reinterpret_cast<const _Float16*>(j.raw) + j.col0 + s0;
    const _Float16* xd = j.raw_donor ? reinterpret_cast<const _Float16*>(j.raw_donor) + j.col0 + s0 : nullptr;
    float* out = j.draw + s0;
    const bool fast = pl.nested && ((j.ld | j.col0 | j.ld_out) & 3) == 0 && (reinterpret_cast<uintptr_t>(j.raw) & 7) == 0 &&
                      (!xd || ((j.ld_donor & 3) == 0 && (reinterpret_cast<uintptr_t>(j.raw_donor) & 7) == 0)) &&
                      (reinterpret_cast<uintptr_t>(j.draw) & 15) == 0;
    typedef unsigned int v2u __attribute__((ext_vector_type(2)));
    if (fast) {
        int at[kBinMaxRes] = {-1, -1, -1};
        float cnt[kBinMaxRes] = {1.f, 1.f, 1.f};
#pragma unroll
        for (int r = 0; r < kBinMaxRes; ++r)
            if (r < nres) at[r] = bin_spread_at(pl, r, ncols, j.flip, s0, &cnt[r]);
        for (int f = 0; f < F; ++f) {
            const float c = bin_spread_sum(j, nres, at, cnt, f);
            const _Float16* xr = x + (size_t)f * j.ld;
            const _Float16* dr = xd ? xd + (size_t)f * j.ld_donor : nullptr;
            float* orow = out + (size_t)f * j.ld_out;
            if (rem > 3) {
                const v2u xv = __builtin_nontemporal_load((const CF_GLOBAL v2u*)xr);
                v2u dv = {0u, 0u};
                if (dr) dv = __builtin_nontemporal_load((const CF_GLOBAL v2u*)dr);
                const _Float16* xh = reinterpret_cast<const _Float16*>(&xv);
                const _Float16* dh = reinterpret_cast<const _Float16*>(&dv);
                const v4f o{((float)xh[0] - (float)dh[0]) * c, ((float)xh[1] - (float)dh[1]) * c, ((float)xh[2] - (float)dh[2]) * c,
                            ((float)xh[3] - (float)dh[3]) * c};
                __builtin_nontemporal_store(o, (CF_GLOBAL v4f*)orow);
            } else {                                                         // the window ends inside this chunk: nothing past it is touched
                for (int k = 0; k < rem; ++k) {
                    const float d = (float)*(const CF_GLOBAL _Float16*)(xr + k) - (dr ? (float)*(const CF_GLOBAL _Float16*)(dr + k) : 0.f);
                    *(CF_GLOBAL float*)(orow + k) = d * c;
                }
            }
        }
        return;
    }
    // per-sample walk: the same lanes, every sample with its own bins
    for (int k = 0; k < min(rem, 4); ++k) {
        int at[kBinMaxRes] = {-1, -1, -1};
        float cnt[kBinMaxRes] = {1.f, 1.f, 1.f};
#pragma unroll
        for (int r = 0; r < kBinMaxRes; ++r)
            if (r < nres) at[r] = bin_spread_at(pl, r, ncols, j.flip, s0 + k, &cnt[r]);
        for (int f = 0; f < F; ++f) {
            const float c = bin_spread_sum(j, nres, at, cnt, f);
            const float d = (float)*(const CF_GLOBAL _Float16*)(x + (size_t)f * j.ld + k) -
                            (xd ? (float)*(const CF_GLOBAL _Float16*)(xd + (size_t)f * j.ld_donor + k) : 0.f);
            *(CF_GLOBAL float*)(out + (size_t)f * j.ld_out + k) = d * c;
        }
    }
}

}  // namespace cf
