// cf_backselect.h -- greedy player selection of the mark games and of a kept exact table (cf_mark_backselect, cf_mark_window_backselect,
// cf_mark_fine_backselect, cf_backselect_from_rows; included by cf_api.hip behind cf_mark_fine.h).
//
// Which few players are enough on their own to make the call, and in what order does the prediction fall apart when players are taken
// away?  Per gene, a greedy PATH through the coalitions and the smallest sufficient set on it (the sufficient input subset: backward
// selection, then the smallest suffix of the removal order that still carries the prediction).  Deterministic: no sampling error.
//   path       move 0 starts from everybody (mode 0, backward: each move REMOVES a player) or from nobody (mode 1, forward: each move
//              ADDS one).  Round t evaluates the P - t candidate coalitions one move away from the current one, candidates in ascending
//              player order; the next move is the candidate with the largest key s_b v[target].  The last move is forced.
//   s_b        +1 if everybody[target] >= nobody[target], else -1 (the sign that makes "towards everybody" upwards); or the caller's
//   tie rule   ascending candidate index with strict >: the lowest player index wins a tie.  A NaN key counts as -inf; if every key is
//              -inf the lowest index wins
//   values     values[b, t] = the logits after t moves: [b, 0] the start row, [b, P] the other end row
//   threshold  thr = nobody + frac (everybody - nobody) on column target, as __fadd_rn(nobody, __fmul_rn(frac, __fsub_rn(everybody,
//              nobody))), or the caller's per-gene value.  A set is sufficient when s_b (v - thr) >= 0 (one __fsub_rn, one __fmul_rn;
//              a NaN is not sufficient); the set of everybody is sufficient by definition
//   size       the smallest k such that the set of k players on the path is sufficient, counted from the small end (the path is not
//              monotone: this is FindSIS); subset = that set
// No atomics, a fixed order, every operation rounded to fp32.
//   k_backselect_step    one workgroup per gene, once per round t.  Pick (t > 0): the keys of the gene's P - (t - 1) rows of the previous
//                        round into LDS, one thread scans them, appends the player to order[b], flips its bit in cur[b]; the winning
//                        row's logits go to values[b, t].  Words: thread c writes candidate c of round t -- cur[b] with its c-th set
//                        bit cleared (backward) or its c-th clear bit among the P players set (forward) -- into the per-gene table
//                        cand[b, c] that the expand kernels read with word_stride = P kw (cf_marks.h).  t = 0 writes s_b,
//                        values[b, 0] and the first cur[b] instead of picking.
//   k_backselect_finish  one workgroup per gene: the forced last move, values[b, P], the threshold, size and subset.
//   k_backselect_table   the same selection and finish on a table [B, 2^P, n_out] (word m at column m, P <= 16): one workgroup per gene
//                        runs all rounds, the candidates' keys are loads from the table; no forward runs.
// 528 / 16 / 132 bytes of LDS, 38 / 18 / 21 VGPRs, no scratch.
#pragma once

namespace cf {

constexpr int kBsThreads = 128;        // k_backselect_step / _finish: one thread per candidate (P <= kMarkWideMaxP)
constexpr int kBsTableThreads = 64;    // k_backselect_table: P <= kCoalMaxS candidates
static_assert(kBsThreads >= kMarkWideMaxP && kBsTableThreads >= kCoalMaxS, "one thread per candidate");

struct BackselectArgs {
    const float* ends;                 // [B, 2, n_out]: nobody, everybody
    const float* prev;                 // [B, P - (t - 1), n_out]: the rows of round t - 1 (t > 0)
    unsigned* cur;                     // [B, kw]: the current coalition
    unsigned* cand;                    // [B, P, kw]: the candidates of round t in the first P - t entries of gene b
    int* dir;                          // [B]: s_b
    int* order;                        // [B, P]
    float* values;                     // [B, P + 1, n_out]
    int* dir_out;                      // [B] or null: s_b for the caller
    int P, kw, n_out, t, mode, target, direction;
};

struct BackselectFinishArgs {
    const float* ends;                 // [B, 2, n_out]
    const int* dir;                    // [B]
    int* order;                        // [B, P]: P - 1 moves in; the last one out
    float* values;                     // [B, P + 1, n_out]
    int* size;                         // [B]
    unsigned* subset;                  // [B, kw]
    const float* threshold;            // [B] or null: the caller's thresholds
    float* thr_out;                    // [B] or null: the threshold used
    float frac;
    int P, kw, n_out, mode, target;
};

struct BackselectTableArgs {
    const float* v;                    // [B, 2^P, n_out], word m at column m
    int* order;                        // [B, P]
    float* values;                     // [B, P + 1, n_out]
    int* size;                         // [B]
    unsigned* subset;                  // [B]
    const float* threshold;            // [B] or null
    float* thr_out;                    // [B] or null
    int* dir_out;                      // [B] or null
    float frac;
    int P, n_out, mode, target, direction;
};

// the bits of word k of a coalition over P players
__device__ __forceinline__ unsigned bs_valid(int P, int k) { return P - 32 * k >= 32 ? ~0u : (1u << (P - 32 * k)) - 1u; }

// the player at the c-th (from 0, ascending) set bit of the kw words w -- `clear`: the c-th clear bit among the P players; c is in range
__device__ __forceinline__ int bs_nth(const unsigned* w, int kw, int P, int c, bool clear) {
    for (int k = 0; k < kw; ++k) {
        unsigned x = clear ? ~w[k] & bs_valid(P, k) : w[k];
        const int n = __popc(x);
        if (c < n) {
            for (; c > 0; --c) x &= x - 1u;
            return 32 * k + __ffs(x) - 1;
        }
        c -= n;
    }
    return 0;
}

__device__ __forceinline__ float bs_key(int s, float v) {
    const float k = __fmul_rn((float)s, v);
    return k != k ? -INFINITY : k;
}

// the candidate with the largest key: ascending index, strict >
__device__ __forceinline__ int bs_pick(const float* key, int n) {
    int best = 0;
    for (int c = 1; c < n; ++c)
        if (key[c] > key[best]) best = c;
    return best;
}

__device__ __forceinline__ int bs_direction(int direction, const float* nobody, const float* everybody, int target) {
    return direction ? direction : (everybody[target] >= nobody[target] ? 1 : -1);
}

// thr = __fadd_rn(nobody, __fmul_rn(frac, __fsub_rn(everybody, nobody))): three operations, each rounded.  Written with plain operators
// under contract(off): in this toolchain the intrinsics are inline functions over plain operators that carry the translation unit's
// contraction flag, and the compiler made one v_fmac_f32 of the product and the sum.
__device__ __forceinline__ float bs_threshold(float nobody, float everybody, float frac) {
#pragma clang fp contract(off)
    const float d = everybody - nobody;
    const float m = frac * d;
    return nobody + m;
}

// The end of a gene's selection, by thread 0 of its workgroup (the other threads copy values[P]): order[0, P - 1) holds the moves made;
// the forced last move, the threshold, size and subset.  `values` is the gene's [P + 1, n_out]; rows 0 and P are read from the end rows.
// `left`: kw words of LDS.
__device__ __forceinline__ void bs_finish(const float* nobody, const float* everybody, int s, int* order, float* values, int* size, unsigned* subset,
                                          const float* threshold, float* thr_out, float frac, int P, int kw, int n_out, int mode, int target,
                                          unsigned* left) {
    const float* first = mode ? nobody : everybody;
    const float* last = mode ? everybody : nobody;
    for (int o = threadIdx.x; o < n_out; o += blockDim.x) values[(size_t)P * n_out + o] = last[o];
    if (threadIdx.x) return;
    for (int k = 0; k < kw; ++k) left[k] = bs_valid(P, k);
    for (int i = 0; i < P - 1; ++i) left[order[i] >> 5] &= ~(1u << (order[i] & 31));
    const int final_move = bs_nth(left, kw, P, 0, false);
    order[P - 1] = final_move;
    const float thr = threshold ? *threshold : bs_threshold(nobody[target], everybody[target], frac);
    if (thr_out) *thr_out = thr;
    int k = 0;      // the set of k players sits after j = k (forward) or P - k (backward) moves
    for (; k < P; ++k) {
        const int j = mode ? k : P - k;
        const float v = j == 0 ? first[target] : j == P ? last[target] : values[(size_t)j * n_out + target];
        if (__fmul_rn((float)s, __fsub_rn(v, thr)) >= 0.f) break;
    }
    *size = k;
    for (int w = 0; w < kw; ++w) left[w] = 0u;
    for (int i = 0; i < k; ++i) {      // forward: the first k moves; backward: the last k
        const int p = mode ? order[i] : (i == 0 ? final_move : order[P - 1 - i]);
        left[p >> 5] |= 1u << (p & 31);
    }
    for (int w = 0; w < kw; ++w) subset[w] = left[w];
}

__global__ __launch_bounds__(kBsThreads) void k_backselect_step(BackselectArgs a) {
    __shared__ float key[kMarkWideMaxP];
    __shared__ unsigned cur[kMarkWideMaxP / 32];
    const int b = blockIdx.x, tid = threadIdx.x, P = a.P, kw = a.kw, n_out = a.n_out, t = a.t;
    const float* nobody = a.ends + (size_t)b * 2 * n_out;
    const float* everybody = nobody + n_out;
    if (t == 0) {
        if (tid < kw) cur[tid] = a.mode ? 0u : bs_valid(P, tid);
        if (tid == 0) {
            const int s = bs_direction(a.direction, nobody, everybody, a.target);
            a.dir[b] = s;
            if (a.dir_out) a.dir_out[b] = s;
        }
        for (int o = tid; o < n_out; o += kBsThreads) a.values[(size_t)b * (P + 1) * n_out + o] = (a.mode ? nobody : everybody)[o];
        __syncthreads();
    } else {
        const int n = P - (t - 1);
        const float* prev = a.prev + (size_t)b * n * n_out;
        if (tid < kw) cur[tid] = a.cur[(size_t)b * kw + tid];
        if (tid < n) key[tid] = bs_key(a.dir[b], prev[(size_t)tid * n_out + a.target]);
        __syncthreads();
        const int win = bs_pick(key, n);      // (every thread: LDS broadcasts, no barrier for the result)
        const int player = bs_nth(cur, kw, P, win, a.mode != 0);
        __syncthreads();
        if (tid == 0) {
            a.order[(size_t)b * P + t - 1] = player;
            cur[player >> 5] ^= 1u << (player & 31);
        }
        for (int o = tid; o < n_out; o += kBsThreads) a.values[((size_t)b * (P + 1) + t) * n_out + o] = prev[(size_t)win * n_out + o];
        __syncthreads();
    }
    if (tid < kw) a.cur[(size_t)b * kw + tid] = cur[tid];
    if (tid < P - t) {
        const int player = bs_nth(cur, kw, P, tid, a.mode != 0);
        unsigned* c = a.cand + ((size_t)b * P + tid) * kw;
        for (int k = 0; k < kw; ++k) c[k] = cur[k] ^ (k == player >> 5 ? 1u << (player & 31) : 0u);
    }
}

__global__ __launch_bounds__(kBsThreads) void k_backselect_finish(BackselectFinishArgs a) {
    __shared__ unsigned left[kMarkWideMaxP / 32];
    const int b = blockIdx.x, P = a.P, n_out = a.n_out;
    const float* nobody = a.ends + (size_t)b * 2 * n_out;
    bs_finish(nobody, nobody + n_out, a.dir[b], a.order + (size_t)b * P, a.values + (size_t)b * (P + 1) * n_out, a.size + b, a.subset + (size_t)b * a.kw,
              a.threshold ? a.threshold + b : nullptr, a.thr_out ? a.thr_out + b : nullptr, a.frac, P, a.kw, n_out, a.mode, a.target, left);
}

__global__ __launch_bounds__(kBsTableThreads) void k_backselect_table(BackselectTableArgs a) {
    __shared__ float key[kCoalMaxS];
    __shared__ unsigned word[kCoalMaxS];
    __shared__ unsigned left[1];
    const int b = blockIdx.x, tid = threadIdx.x, P = a.P, n_out = a.n_out;
    const unsigned full = (1u << P) - 1u;
    const float* v = a.v + ((size_t)b << P) * n_out;
    const float* nobody = v;
    const float* everybody = v + (size_t)full * n_out;
    float* values = a.values + (size_t)b * (P + 1) * n_out;
    int* order = a.order + (size_t)b * P;
    const int s = bs_direction(a.direction, nobody, everybody, a.target);
    if (tid == 0 && a.dir_out) a.dir_out[b] = s;
    unsigned cur = a.mode ? 0u : full;
    for (int o = tid; o < n_out; o += kBsTableThreads) values[o] = v[(size_t)cur * n_out + o];
    for (int t = 1; t < P; ++t) {
        const int n = P - (t - 1);
        if (tid < n) {
            const int player = bs_nth(&cur, 1, P, tid, a.mode != 0);
            word[tid] = cur ^ (1u << player);
            key[tid] = bs_key(s, v[(size_t)word[tid] * n_out + a.target]);
        }
        __syncthreads();
        const int win = bs_pick(key, n);
        const unsigned next = word[win];
        if (tid == 0) order[t - 1] = __ffs(cur ^ next) - 1;
        cur = next;
        for (int o = tid; o < n_out; o += kBsTableThreads) values[(size_t)t * n_out + o] = v[(size_t)cur * n_out + o];
        __syncthreads();      // (key and word are rewritten next round; order[] is read by thread 0 below, which wrote it)
    }
    bs_finish(nobody, everybody, s, order, values, a.size + b, a.subset + b, a.threshold ? a.threshold + b : nullptr, a.thr_out ? a.thr_out + b : nullptr,
              a.frac, P, 1, n_out, a.mode, a.target, left);
}

}  // namespace cf
