// cf_bin_grad.h -- backward of the GPU binning (cf_bin.h), all resolutions: gradient with respect to the RAW signal
// (included by cf_kernels.h after cf_bin.h, whose BinPlan / limits it shares).
//
// The forward maps the window [col0, col0 + ncols) of raw x[f, .] to, per resolution r (bin size b_r, L_r output bins),
//     n_r = min(ceil(ncols / b_r), L_r) real bins, left_r = ceil((L_r - n_r) / 2)                       (data.py:87)
//     bin g = samples [g b_r, min((g + 1) b_r, ncols)), count cnt, mean m  ->  out_r[p, f] = log(1 + m)
//     p = left_r + g, or L_r - 1 - (left_r + g) for a mirrored ('-' strand) region.
// With dfeat_r[p, f] the gradient with respect to out_r, the chain rule gives, exactly,
//     draw[f, s] = sum_r dfeat_r[p_r(s), f] / (cnt_{r,g_r(s)} (1 + m_{r,g_r(s)}))        s in [0, ncols)
// in raw (genomic) orientation -- the mirror is undone --, fp32, window-relative.  Pad rows of dfeat are never read; samples
// past the last real bin of a resolution get nothing from it; a null dfeat[r] counts as zero.  times_input multiplies by
// (float)x[f, col0 + s] (gradient x input).  Where 1 + m <= 0 the result is inf / NaN, as the reference's log gives under
// autograd; preprocessed signals are non-negative.
//
// A pure HBM scan like the forward: 2 bytes in and 4 bytes out per sample, plus the small dfeat gathers.  Every window
// sample is written exactly once by exactly one lane: no atomics, no workgroup barrier on the one-pass path, run-to-run
// bit-identical.
#pragma once

namespace cf {

struct BinGradJob {                      // = cf_bin_grad_job of the C ABI
    const void* raw;
    long long ld;
    int col0, ncols;
    int flip, reserved;
    const float* dfeat[kBinMaxRes];      // [L_r, F], coarsest first
    float* draw;                         // [F, ld_out]
    long long ld_out;
};
__host__ __device__ constexpr int bin_grad_wave_lds_floats(int nload) { return nload * 64 + 4 * 64 + 4; }
constexpr int kBinGradCoef = kBinMaxRes * kBinMaxBins;       // generic path: a coefficient per (resolution, bin) of one feature row
__host__ __device__ constexpr int bin_grad_lds_floats(int nload) {
    return 4 * bin_grad_wave_lds_floats(nload) > kBinGradCoef ? 4 * bin_grad_wave_lds_floats(nload) : kBinGradCoef;
}

// dfeat_r[p(g), f] / (cnt (1 + sum / cnt)): the factor every sample of bin g of resolution r receives
__device__ __forceinline__ float bin_grad_coef(const float* dfeat, int F, int f, int L, int left, int n_all, int flip, int g, int cnt, float sum) {
    if (!dfeat || g >= n_all || cnt <= 0) return 0.f;
    const int q = left + g, p = flip ? L - 1 - q : q;
    const float d = *(const CF_GLOBAL float*)(dfeat + (size_t)p * F + f);
    return d / ((float)cnt * (1.0f + sum / (float)cnt));
}

// One-pass path, mirror of bin_unit_wave: a wave owns one unit (b0 samples) of one region and walks its feature rows --
//   sums     the forward's loads (8 bytes per lane, next row requested before the current one is reduced, chunks past the
//            window clamped) and the forward's order of additions: chunk sums -> finest -> middle -> coarsest bins
//   coefs    the lanes that own a finest / middle / coarsest bin gather dfeat and leave dfeat / (cnt (1 + m)) in LDS
//   write    lane l of load k writes the 4 samples of chunk 64 k + l: coarse + middle + fine, one 16-byte store
template <int NLOAD>
__device__ __forceinline__ void bin_unit_wave_bwd(const BinGradJob& j, const BinPlan& pl, const int unit, const int times, float* lds) {
    const int lane = threadIdx.x & 63;
    const int F = pl.F, nres = pl.n_res;                         // (nres is 2 or 3 here: `nested` needs two resolutions)
    const int b0 = pl.b[0], bf = nres == 3 ? pl.b[2] : pl.b[1];
    const int cpu = b0 >> 2, cpf = bf >> 2;
    const int nf = b0 / bf;
    const int nm = nres == 3 ? b0 / pl.b[1] : 0;
    const int fpm = nres == 3 ? pl.b[1] / bf : 1;
    float* cs = lds;                                             // [NLOAD * 64] chunk sums of the row
    float* fs = cs + NLOAD * 64;                                 // [64] finest-bin sums
    float* ms = fs + 64;                                         // [64] middle-bin sums
    float* kf = ms + 64;                                         // [64] coefficients, finest resolution
    float* km = kf + 64;                                         // [64] middle
    float* kc = km + 64;                                         // [1]  coarsest
    const int s0 = unit * b0;
    const int ncols = j.ncols;
    const int flip = j.flip;
    const int Lc = pl.L[0], Lf = nres == 3 ? pl.L[2] : pl.L[1], Lm = pl.L[1];
    const int nac = min((ncols + b0 - 1) / b0, Lc), naf = min((ncols + bf - 1) / bf, Lf);
    const int nam = nres == 3 ? min((ncols + pl.b[1] - 1) / pl.b[1], Lm) : 0;
    const int lc = (Lc - nac + 1) / 2, lf = (Lf - naf + 1) / 2, lm = (Lm - nam + 1) / 2;
    const float* dc = j.dfeat[0];
    const float* dm = nres == 3 ? j.dfeat[1] : nullptr;
    const float* df = nres == 3 ? j.dfeat[2] : j.dfeat[1];
    const _Float16* base = reinterpret_cast<const _Float16*>(j.raw) + j.col0 + s0;
    typedef unsigned int v2u __attribute__((ext_vector_type(2)));
    v2u cur[NLOAD], nxt[NLOAD];
    auto request = [&](v2u (&dst)[NLOAD], int f) {
        const _Float16* row = base + (size_t)f * j.ld;
#pragma unroll
        for (int k = 0; k < NLOAD; ++k) {
            const int c = k * 64 + lane;
            const int cc = min(c, min(cpu - 1, max((ncols - s0 - 1) >> 2, 0)));
            dst[k] = __builtin_nontemporal_load((const CF_GLOBAL v2u*)(row + 4 * cc));
        }
    };
    int fine[NLOAD];                                             // finest bin (inside the unit) of the chunks this lane writes
#pragma unroll
    for (int k = 0; k < NLOAD; ++k) fine[k] = min((k * 64 + lane) / cpf, nf - 1);
    request(cur, 0);
    for (int f = 0; f < F; ++f) {
        if (f + 1 < F) request(nxt, f + 1);
#pragma unroll
        for (int k = 0; k < NLOAD; ++k) {
            const int c = k * 64 + lane;
            const int rem = ncols - s0 - 4 * c;
            const _Float16* hp = reinterpret_cast<const _Float16*>(&cur[k]);
            float s = 0.f;
            if (c < cpu && rem > 0) {
                s = (float)hp[0];
                if (rem > 1) s += (float)hp[1];
                if (rem > 2) s += (float)hp[2];
                if (rem > 3) s += (float)hp[3];
            }
            if (c < cpu) cs[c] = s;
        }
        __builtin_amdgcn_wave_barrier();
        {
            float s = 0.f;
            if (lane < nf)
                for (int i = 0; i < cpf; ++i) s += cs[lane * cpf + i];
            const int g = unit * nf + lane;
            if (lane < nf) {
                fs[lane] = s;
                kf[lane] = bin_grad_coef(df, F, f, Lf, lf, naf, flip, g, min(bf, ncols - g * bf), s);
            }
        }
        __builtin_amdgcn_wave_barrier();
        if (nres == 3) {
            float s = 0.f;
            if (lane < nm)
                for (int i = 0; i < fpm; ++i) s += fs[lane * fpm + i];
            const int g = unit * nm + lane;
            if (lane < nm) {
                ms[lane] = s;
                km[lane] = bin_grad_coef(dm, F, f, Lm, lm, nam, flip, g, min(pl.b[1], ncols - g * pl.b[1]), s);
            }
            __builtin_amdgcn_wave_barrier();
        }
        if (lane == 0) {
            const float* src = nres == 3 ? ms : fs;
            const int n = nres == 3 ? nm : nf;
            float s = 0.f;
            for (int i = 0; i < n; ++i) s += src[i];
            kc[0] = bin_grad_coef(dc, F, f, Lc, lc, nac, flip, unit, min(b0, ncols - s0), s);
        }
        __builtin_amdgcn_wave_barrier();
        {
            const float c0 = kc[0];
            float* orow = j.draw + (size_t)f * j.ld_out + s0;
#pragma unroll
            for (int k = 0; k < NLOAD; ++k) {
                const int c = k * 64 + lane;
                const int rem = ncols - s0 - 4 * c;
                if (c < cpu && rem > 0) {
                    float v = c0;
                    if (nres == 3) v += km[fine[k] / fpm];
                    v += kf[fine[k]];
                    v4f o{v, v, v, v};
                    if (times) {
                        const _Float16* hp = reinterpret_cast<const _Float16*>(&cur[k]);
                        o = v4f{v * (float)hp[0], v * (float)hp[1], v * (float)hp[2], v * (float)hp[3]};
                    }
                    if (rem > 3) {
                        __builtin_nontemporal_store(o, (CF_GLOBAL v4f*)(orow + 4 * c));
                    } else {                                     // the window ends inside this chunk
                        __builtin_nontemporal_store(o.x, (CF_GLOBAL float*)(orow + 4 * c));
                        if (rem > 1) __builtin_nontemporal_store(o.y, (CF_GLOBAL float*)(orow + 4 * c + 1));
                        if (rem > 2) __builtin_nontemporal_store(o.z, (CF_GLOBAL float*)(orow + 4 * c + 2));
                    }
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int k = 0; k < NLOAD; ++k) cur[k] = nxt[k];
    }
}

// Generic path (rows or output not aligned, bin sizes that do not nest, more than kBinMaxF feature rows): one workgroup per
// region and, per feature row, (1) a wave per (resolution, bin) adds the bin's samples the way bin_region_scalar does and
// leaves the coefficient in LDS, (2) after a barrier every sample of the row is written, 4 bytes per lane, unit stride.
__device__ __forceinline__ void bin_region_grad_scalar(const BinGradJob& j, const BinPlan& pl, const int times, float* coef) {
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int F = pl.F, nres = pl.n_res, ncols = j.ncols;
    const _Float16* raw = reinterpret_cast<const _Float16*>(j.raw);
    for (int f = 0; f < F; ++f) {
        const _Float16* row = raw + (size_t)f * j.ld + j.col0;
#pragma unroll
        for (int r = 0; r < kBinMaxRes; ++r) {
            if (r >= nres) break;
            const int b = pl.b[r], L = pl.L[r];
            const int n_full = ncols / b, tail = ncols - n_full * b;
            const int n_bins = min(n_full + (tail > 0 ? 1 : 0), L);
            const int left = (L - n_bins + 1) / 2;
            for (int bin = w; bin < n_bins; bin += 4) {
                const int cnt = bin < n_full ? b : tail;
                const _Float16* src = row + (size_t)bin * b;
                float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
                int c = lane;
                for (; c + 192 < cnt; c += 256) {
                    s0 += (float)*(const CF_GLOBAL _Float16*)(src + c);
                    s1 += (float)*(const CF_GLOBAL _Float16*)(src + c + 64);
                    s2 += (float)*(const CF_GLOBAL _Float16*)(src + c + 128);
                    s3 += (float)*(const CF_GLOBAL _Float16*)(src + c + 192);
                }
                for (; c < cnt; c += 64) s0 += (float)*(const CF_GLOBAL _Float16*)(src + c);
                const float s = wave_sum((s0 + s1) + (s2 + s3));
                if (lane == 0) coef[r * kBinMaxBins + bin] = bin_grad_coef(j.dfeat[r], F, f, L, left, n_bins, j.flip, bin, cnt, s);
            }
        }
        __syncthreads();
        float* orow = j.draw + (size_t)f * j.ld_out;
        for (int s = tid; s < ncols; s += 256) {
            float v = 0.f;
#pragma unroll
            for (int r = 0; r < kBinMaxRes; ++r) {
                if (r >= nres) break;
                const int g = s / pl.b[r];
                if (g < pl.L[r]) v += coef[r * kBinMaxBins + g];          // (a real bin: g < ceil(ncols / b) holds for every s)
            }
            if (times) v *= (float)*(const CF_GLOBAL _Float16*)(row + s);
            *(CF_GLOBAL float*)(orow + s) = v;
        }
        __syncthreads();                                                   // the coefficients of this row have been consumed
    }
}

// grid = (ceil(units of the longest window / 4), regions), as k_bin_multi
template <int NLOAD>
__global__ __launch_bounds__(256) void k_bin_multi_bwd(const BinGradJob* __restrict__ jobs, BinPlan pl, int times) {
    __shared__ float lds[bin_grad_lds_floats(NLOAD)];
    const BinGradJob j = jobs[blockIdx.y];
    if (j.ncols <= 0) return;                                              // nothing to write
    const bool fast = pl.nested && ((j.ld | j.col0 | j.ld_out) & 3) == 0 && (reinterpret_cast<uintptr_t>(j.raw) & 7) == 0 &&
                      (reinterpret_cast<uintptr_t>(j.draw) & 15) == 0;
    if (!fast) {
        if (blockIdx.x == 0) bin_region_grad_scalar(j, pl, times, lds);
        return;
    }
    const int w = threadIdx.x >> 6;
    const int unit = blockIdx.x * 4 + w;
    const int n_units = (j.ncols + pl.b[0] - 1) / pl.b[0];                 // every sample of the window is written, also past L[0] bins
    if (unit >= n_units) return;
    bin_unit_wave_bwd<NLOAD>(j, pl, unit, times, lds + w * bin_grad_wave_lds_floats(NLOAD));
}

}  // namespace cf
