// cf_contact.h -- contact games: coalition forwards whose players delete pCRE slots and / or edit promoter-pCRE contact frequencies
// (cf_contact_coalitions, cf_contact_shapley, cf_contact_epistasis, cf_contact_shapley_interactions; included by cf_api.hip behind
// cf_coalition.h, whose stash, reducers and chunk loop the host side shares).
//
// A player p has two 32-bit words over the pCRE slots: drop_p (bit j: slot j is deleted while p is absent) and contact_p (bit j: slot
// j's contact is edited while p is absent).  A coalition is one word, bit p set = player p PRESENT.  For row (b, m), with D the OR of
// drop_p and C the OR of contact_p over the absent players:
//   deletion      for every j in D, row and column j + 1 of the interaction mask are set, at every resolution: the rule of
//                 k_coalition_expand with gone = D << 1;
//   contact edit  entry (q, k) of interaction_freq[b] is edited when token q or token k is j + 1 for some j in C (token 0, the promoter,
//                 is never named; row and column both, mirroring the mask rule: the kernels read all T x T entries), once per entry:
//                   scale rule   scale * f, one fp32 multiplication (no contraction: there is nothing to fuse it with)
//                   donor rule   donor_freq[b, q, k], the bits as they are
//   everything else in the row is gene b's own.
// The Regulation layers REPLACE a masked score (kMaskFill, cf_reg8.h), they do not bias it: once slot j is deleted its contact entries
// are never read, so `contact j` is a null player next to an absent `pcre j`, bit for bit.
// Kernel:
//   k_contact_expand  per (chunk row, resolution), kAblThreads threads: the row's word from the device table, D and C OR-ed over the at
//                     most 16 players (their words sit behind the coalition words: [words | drop_p | contact_p], the narrow layout of the
//                     mark games; uniform across the workgroup: scalar loads and scalar ALU), the stashed rows of the gene -> Rx[r][0],
//                     the OR-ed mask from D; resolution 0 writes the chunk row's [T, T] frequencies.  Every output element is written
//                     once; no atomics, no scratch, no LDS.
#pragma once

namespace cf {

struct ContactExpandArgs {
    CoalExpandArgs c;                        // stash, x0, masks, frequencies, g0, n_coal, T, row4; c.keep: the coalition words (device)
    const unsigned* players;                 // [2 P] (device): drop_p, then contact_p
    const float* donor_freq;                 // [B, T, T] (device): the donor rule; null: the scale rule
    float scale;
    int P;
};

__global__ __launch_bounds__(kAblThreads) void k_contact_expand(ContactExpandArgs a) {
    const int i = blockIdx.x, r = blockIdx.y, tid = threadIdx.x;
    const long long g = a.c.g0 + i;
    const int b = (int)(g / a.c.n_coal), T = a.c.T, TT = T * T, P = a.P;
    const unsigned absent = ~a.c.keep[g - (long long)b * a.c.n_coal];
    unsigned D = 0u, C = 0u;
#pragma unroll 4
    for (int p = 0; p < P; ++p) {            // (unconditional loads, selected by a mask: they issue together, not one after the other)
        const unsigned gone_p = 0u - (absent >> p & 1u);
        D |= a.players[p] & gone_p, C |= a.players[P + p] & gone_p;
    }
    // bit 0 is the promoter token (never named), bit j + 1 pCRE slot j
    const unsigned live = (1u << T) - 2u, gone = D << 1 & live, edit = C << 1 & live;
    rows_copy_x0(a.c.stash[r], a.c.x0[r], b, i, a.c.row4);
    const uint8_t* __restrict__ min = a.c.mask_in[r] + (size_t)b * TT;
    uint8_t* __restrict__ mout = a.c.mask_out[r] + (size_t)i * TT;
    for (int k = tid; k < TT; k += kAblThreads) {
        const int row = k / T, col = k - row * T;
        mout[k] = (gone >> row | gone >> col) & 1u ? (uint8_t)1 : min[k];
    }
    if (r != 0) return;
    const float* __restrict__ fin = a.c.freq_in + (size_t)b * TT;
    const float* __restrict__ don = a.donor_freq ? a.donor_freq + (size_t)b * TT : nullptr;
    float* __restrict__ fout = a.c.freq_out + (size_t)i * TT;
    const float scale = a.scale;
    for (int k = tid; k < TT; k += kAblThreads) {
#pragma clang fp contract(off)
        const int row = k / T, col = k - row * T;
        const float f = fin[k];
        float x = f;
        if ((edit >> row | edit >> col) & 1u) x = don ? don[k] : scale * f;
        fout[k] = x;
    }
}

}  // namespace cf
