// cf_input_grad.h -- gradients with respect to the model's float inputs (cf_backward_from_inputs; included by cf_api.hip).
//
// Histone features enter only through the bias-free projections lin_proj (Embedding) and lin_proj_pcre (Pairwise):
//     x_j = W f_j + PE_j
// and, with one centre-row attention layer over them, only through the centre query (Embedding: bin L/2) and the keys and
// values of every bin.  The weight gradient the reduction tables assemble from rank-structured factors (build_tables:
// edx0 (x) f_centre + sum_h dxbar_h (x) w_h + qt_h (x) du_h) is, left uncontracted over the bins j,
//     dfeat_j = W^T ( [j = centre] edx0 + sum_h p_hj dxbar_h + ds_hj qt_h )
//     ds_hj   = p_hj (dp_hj - sum_k p_hk dp_hk) / sqrt(dh)   (0 where the bin is masked),   dp_hj = x_j . dxbar_h
// -- the same ds the attention backward forms (cf_attc2.h: score = x . qt / sqrt(dh), qt unscaled).  For a pCRE the sum runs
// over the (layer, head) pairs of the Pairwise stack: keys and values come from the same x_c in every layer.  Every operand
// (p, qt, dxbar, edx0) is saved per sequence by the forward / backward pass and none of them is written by the reductions.
//
// k_input_grad: one workgroup per (sequence, gene, resolution), bins across lanes; per (layer, head) term: W^T dxbar and
// W^T qt into LDS, PE_j . dxbar from the transposed table (coalesced), one block reduction for <p, dp>.  The gradient rows
// are accumulated in LDS in a fixed order and stored once, coalesced, in the caller's [.., L, F] layout: no atomics,
// bit-identical run to run.
//
// k_dfreq_sum: interaction_freq enters as gamma_f[h] freq[i][j] added to every Regulation score, so its gradient is
// sum over resolutions, layers and heads of gamma_f dS; the Regulation backward leaves one [T, T] block per (resolution,
// gene) (k_reg8_bwd<., true> / k_attr<true, true>), this sums the resolutions in order.
#pragma once

namespace cf {

constexpr int kIgMaxPair = kLpMaxSeg / 2;      // Pairwise layers (check_config: 2 * pair_layers <= kLpMaxSeg)
constexpr int kIgThreads = 256;

struct InGradArgs {
    const float* feats_p[kMaxRes];            // [B, L, F]
    const float* feats_c[kMaxRes];            // [B, S, L, F]
    const uint8_t* mask_p[kMaxRes];           // centre rows of the pad masks: [B] rows of L at stride mstride
    const uint8_t* mask_c[kMaxRes];
    long long mstride_p[kMaxRes], mstride_c[kMaxRes];
    const float* pet[kMaxRes];                // positional table, transposed: [D][L]
    const float* w_p[kMaxRes];                // lin_proj.weight       [D][F]
    const float* w_c[kMaxRes];                // lin_proj_pcre.weight  [D][F]
    const float* edx0[kMaxRes];               // d(Embedding input, centre row) [B][D]
    const float* ep[kMaxRes];                 // Embedding: p [B, nh_e, L], qt / dxbar [B, nh_e, D]
    const float* eqt[kMaxRes];
    const float* edxbar[kMaxRes];
    const float* pp[kMaxRes][kIgMaxPair];     // Pairwise layer l: p [B*S, nh_p, L], qt / dxbar [B*S, nh_p, D]
    const float* pqt[kMaxRes][kIgMaxPair];
    const float* pdxbar[kMaxRes][kIgMaxPair];
    float* out_p[kMaxRes];                    // nullptr: not requested
    float* out_c[kMaxRes];
    int L[kMaxRes];
    int B, S, F, D, nh_e, nh_p, n_pl;
    float rs_e, rs_p;                         // 1 / sqrt(head width)
};

__host__ __device__ inline size_t input_grad_smem(int L, int F, int D) {
    return (size_t)(2 * L * F + L + 2 * D + D * F + 16 + kIgThreads / 64) * sizeof(float);
}

__device__ __forceinline__ float ig_block_sum(float v, float* red) {      // fixed order: wave butterfly, then the 4 waves in turn
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < kIgThreads / 64; ++k) s += red[k];
    return s;
}

__global__ __launch_bounds__(kIgThreads) void k_input_grad(InGradArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int r = blockIdx.z, g = blockIdx.y, tid = threadIdx.x;
    const bool prom = blockIdx.x == 0;                      // sequence 0: the promoter, 1 .. S: the pCRE slots
    float* out = prom ? a.out_p[r] : a.out_c[r];
    if (!out) return;
    const int L = a.L[r], F = a.F, D = a.D;
    const long long n = prom ? g : (long long)g * a.S + (blockIdx.x - 1);      // row of the centre-layer buffers
    const float* f = (prom ? a.feats_p[r] : a.feats_c[r]) + n * L * F;
    const uint8_t* mk = prom ? a.mask_p[r] + n * a.mstride_p[r] : a.mask_c[r] + n * a.mstride_c[r];
    const float* W = prom ? a.w_p[r] : a.w_c[r];
    const float* pet = a.pet[r];
    const int nh = prom ? a.nh_e : a.nh_p, nterms = prom ? nh : a.n_pl * nh;
    const float rs = prom ? a.rs_e : a.rs_p;
    float* f_s = smem;                 // [L][F]  features
    float* acc_s = f_s + L * F;        // [L][F]  gradient rows
    float* dp_s = acc_s + L * F;       // [L]     dp of the current term
    float* v_s = dp_s + L;             // [2][D]  dxbar | qt of the current term
    float* w_s = v_s + 2 * D;          // [D][F]  W
    float* u_s = w_s + D * F;          // [2][8]  W^T dxbar | W^T qt
    float* red = u_s + 16;             // [4]     block reduction
    for (int i = tid; i < L * F; i += kIgThreads) f_s[i] = f[i];
    for (int i = tid; i < D * F; i += kIgThreads) w_s[i] = W[i];
    __syncthreads();
    const int centre = L / 2;
    for (int j = tid; j < L; j += kIgThreads)
        for (int k = 0; k < F; ++k) {
            float v = 0.f;
            if (prom && j == centre) {                      // the query / residual row of the Embedding layer
                const float* e = a.edx0[r] + (size_t)g * D;
                for (int d = 0; d < D; ++d) v = fmaf(w_s[d * F + k], e[d], v);
            }
            acc_s[j * F + k] = v;
        }
    for (int t = 0; t < nterms; ++t) {
        const int l = t / nh, hd = t - l * nh;
        const size_t row = (size_t)n * nh + hd;
        const float* p = (prom ? a.ep[r] : a.pp[r][l]) + row * L;
        const float* dxbar = (prom ? a.edxbar[r] : a.pdxbar[r][l]) + row * D;
        const float* qt = (prom ? a.eqt[r] : a.pqt[r][l]) + row * D;
        __syncthreads();                                    // (the previous term is done with v_s / u_s / dp_s)
        for (int i = tid; i < D; i += kIgThreads) {
            v_s[i] = dxbar[i];
            v_s[D + i] = qt[i];
        }
        __syncthreads();
        if (tid < 2 * F) {                                  // u = W^T dxbar, W^T qt
            const int which = tid >= F, k = tid - which * F;
            const float* v = v_s + which * D;
            float s = 0.f;
            for (int d = 0; d < D; ++d) s = fmaf(w_s[d * F + k], v[d], s);
            u_s[which * 8 + k] = s;
        }
        for (int j = tid; j < L; j += kIgThreads) {       // PE_j . dxbar
            float s = 0.f;
            for (int d = 0; d < D; ++d) s = fmaf(pet[(size_t)d * L + j], v_s[d], s);
            dp_s[j] = s;
        }
        __syncthreads();
        float part = 0.f;
        for (int j = tid; j < L; j += kIgThreads) {
            float s = dp_s[j];
            for (int k = 0; k < F; ++k) s = fmaf(f_s[j * F + k], u_s[k], s);
            dp_s[j] = s;
            part = fmaf(p[j], s, part);
        }
        const float dot = ig_block_sum(part, red);
        for (int j = tid; j < L; j += kIgThreads) {
            const float pj = p[j];
            const float ds = mk[j] ? 0.f : pj * (dp_s[j] - dot) * rs;
            for (int k = 0; k < F; ++k) acc_s[j * F + k] = fmaf(ds, u_s[8 + k], fmaf(pj, u_s[k], acc_s[j * F + k]));
        }
    }
    __syncthreads();
    float* o = out + n * L * F;
    for (int i = tid; i < L * F; i += kIgThreads) o[i] = acc_s[i];
}

// dfreq[g][ij] = sum over resolutions of part[r][g][ij] (resolution order fixed)
__global__ __launch_bounds__(256) void k_dfreq_sum(const float* part, float* dfreq, int n, int nres) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = part[i];
    for (int r = 1; r < nres; ++r) s += part[(size_t)r * n + i];
    dfreq[i] = s;
}

}  // namespace cf
