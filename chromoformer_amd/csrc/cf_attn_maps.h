// cf_attn_maps.h -- attention maps and the regulatory embedding of a saving forward pass (cf_attention_maps; included by cf_api.hip).
//
// Every probability a user can read off the reference (modules.py:73, 184: att_prob) whose output the model consumes is already
// in the workspace after cf_forward(save = 1), kept for the backward pass:
//   * Embedding, centre query row:            E%d.p      [B, nh_e, L]           (k_trunk_fwd, k_attc1 / k_attc2 / k_attc: same layout)
//   * Pairwise, centre row of every pCRE:     P%d.%d.p   [B * S, nh_p, L]
//   * Regulation, layer-by-layer (k_attr):    R%d.%d.p   [B, H, T, T]           all rows
//   * Regulation, fused (cf_reg8.h):          R%d.%d.hq  [B, 8, kHqFloats]     per (gene, head): the p^T tile at kHqP, quarter-major --
//     float (4 lq + lr) * 4 + ii holds p[4 lq + ii][lr] (lane (lr, lq), register ii; cf_reg8.h stores it in the forward's attend(),
//     reads it back as pT in the backward).  Row 0 is quarter 0, register 0: p[0][j] at kHqP + 4 j, j < T -- stored by every
//     layer, the last (row-0-only) one included; the other rows of that layer are not computed for real and are not read.
//   * the fc_head input:                      H.in       [B, n_res * d_emb]     (k_head_fwd / k_head_gen_fwd of every save = 1 pass)
// k_attn_maps copies them into the caller's dense layouts: no arithmetic (the maps are bit-equal to the probabilities the forward
// used), no atomics.  One launch: blockIdx.y picks the output (embed[r], pairwise[r], regulation[r], embedding), the threads of
// blockIdx.x stride over its elements in output order (coalesced stores).
#pragma once

namespace cf {

constexpr int kMapPair = kLpMaxSeg / 2;      // Pairwise layers (check_config: 2 * pair_layers <= kLpMaxSeg)
constexpr int kMapReg = 32;                  // Regulation layers (check_config)
constexpr int kMapThreads = 256;
constexpr int kMapSegs = 3 * kMaxRes + 1;    // blockIdx.y

struct AttnMapArgs {
    const float* ep[kMaxRes];                // E%d.p
    const float* pp[kMaxRes][kMapPair];      // P%d.%d.p
    const float* rp[kMaxRes][kMapReg];       // R%d.%d.p (layer-by-layer) or R%d.%d.hq (fused)
    const float* hin;                        // H.in
    float* embed[kMaxRes];                   // [B, nh_e, L]                 null: not requested
    float* pair[kMaxRes];                    // [B, n_pl, S, nh_p, L]
    float* reg[kMaxRes];                     // [B, n_rl, H, T]
    float* emb;                              // [B, K]
    int L[kMaxRes];
    int B, S, T, nh_e, nh_p, n_pl, H, n_rl, K;
    int reg_fused;                           // rp points at the fused kernels' hq blocks
};

__global__ __launch_bounds__(kMapThreads) void k_attn_maps(AttnMapArgs a) {
    const int seg = blockIdx.y, kind = seg / kMaxRes, r = seg % kMaxRes;
    const long long stride = (long long)gridDim.x * kMapThreads;
    const long long i0 = (long long)blockIdx.x * kMapThreads + threadIdx.x;
    if (kind == 0) {                         // Embedding: the saved rows are the output rows
        float* out = a.embed[r];
        if (!out) return;
        const float* src = a.ep[r];
        const long long n = (long long)a.B * a.nh_e * a.L[r];
        for (long long i = i0; i < n; i += stride) out[i] = src[i];
    } else if (kind == 1) {                  // Pairwise: [g, l, s, h, j] <- P[l].p[(g S + s) nh + h][j]
        float* out = a.pair[r];
        if (!out) return;
        const int L = a.L[r], nh = a.nh_p, S = a.S;
        const long long n = (long long)a.B * a.n_pl * S * nh * L;
        for (long long i = i0; i < n; i += stride) {
            const long long row = i / L;
            const int j = (int)(i - row * L), h = (int)(row % nh);
            const long long gs_l = row / nh;
            const int s = (int)(gs_l % S);
            const long long gl = gs_l / S;
            const int l = (int)(gl % a.n_pl);
            const long long g = gl / a.n_pl;
            out[i] = a.pp[r][l][((g * S + s) * nh + h) * L + j];
        }
    } else if (kind == 2) {                  // Regulation, row 0: [g, l, h, j] <- p[g][h][0][j]
        float* out = a.reg[r];
        if (!out) return;
        const int T = a.T, H = a.H;
        const long long n = (long long)a.B * a.n_rl * H * T;
        for (long long i = i0; i < n; i += stride) {
            const long long row = i / T;
            const int j = (int)(i - row * T), h = (int)(row % H);
            const long long gl = row / H;
            const int l = (int)(gl % a.n_rl);
            const long long g = gl / a.n_rl;
            const float* src = a.reg_fused ? a.rp[r][l] + (g * kRH + h) * kHqFloats + kHqP + 4 * j      // p^T tile: quarter 0, register 0
                                           : a.rp[r][l] + (g * H + h) * T * T + j;
            out[i] = *src;
        }
    } else {                                 // the fc_head input
        float* out = a.emb;
        if (!out || r != 0) return;
        const long long n = (long long)a.B * a.K;
        for (long long i = i0; i < n; i += stride) out[i] = a.hin[i];
    }
}

}  // namespace cf
