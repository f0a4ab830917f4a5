// cf_dividends.h -- Harsanyi dividends (the Moebius transform) of the coalition table of an exact game, and interaction indices of any
// order from them (cf_dividends_from_rows, cf_set_interactions_from_dividends; included by cf_api.hip behind cf_coalition.h).
//
// rows [B, 2^P, n_out] is the table k_shapley reduces: the logits of every coalition, word m at column m.  The dividend of a set S is
//   m(S) = sum over T <= S of (-1)^(|S| - |T|) v(T),          and back:  v(S) = sum over T <= S of m(T).
// The DEFINITION of the fp32 result is the in-place recurrence
//   for k = 0, 1, ..., P - 1, for every word S with bit k set:   a[S] = a[S] - a[S ^ (1 << k)]          one fp32 subtraction each
// (within a stage no element is both read and written, so the order inside a stage is free and every element's bits are fixed).
// Consequences, bit for bit: div[0] = v(0); div[{i}] = v({i}) - v(0); div[{i, j}] = (v(ij) - v(j)) - (v(i) - v(0)) for i < j, the
// grouping of k_shapley_pairs; a null player i (rows bit-equal with and without i, finite) makes stage i write a - a = +0 into every
// set that holds i, and the later stages keep 0 - 0 = +0.
// `mass` is the same butterfly with + on |v|: mass(S) = sum over T <= S of |v(T)|, the scale of the dividend's rounding error (an
// element passes through |S| subtractions: |div - exact| <= ((1 + 2^-24)^|S| - 1) mass).  Same body, template flag.
// Kernels:
//   k_moebius       one workgroup per (gene, tile of kDivTile = 4,096 consecutive words, table): the tile with all n_out <= 2 columns
//                   (32 KB of static LDS) runs stages 0 .. min(P, 12) - 1 in LDS, one barrier per stage.  blockIdx.z = 0 the dividends,
//                   1 the mass (only launched when asked for): one launch either way.
//   k_moebius_high  P > 12 only, in place on k_moebius's output: the remaining P - 12 <= 4 stages in registers.  A thread owns one
//                   (low word, column) and its 2^(P - 12) values, 4,096 n_out floats apart: loads and stores are unit-stride across
//                   lanes.  Instantiated per stage count, fully unrolled: no private array in memory.
//   The launch contract: one launch for P <= 12, two above.
//   k_set_index     per (gene, listed set S, 1 <= |S| <= order):  out[b, s, o] = sum over U >= S of wt[|S|][|U|] div[b, U, o].
//                   The weights (host, double, rounded to fp32, passed by value) tell the indices apart:
//                     sii              wt = 1 / (|U| - |S| + 1)          order 1: the Shapley value, order 2: the pairwise sii
//                     sti, top order k |S| < k: the dividend itself -- its bits are copied, no arithmetic;
//                                      |S| = k: wt = 1 / C(|U|, k); the sum over all sets of size 1..k is v(N) - v(0) up to rounding.
//                   Thread t sums the supersets of rank t, t + kShapThreads, ... in ascending order (the rank over the free bits is
//                   deposited into the complement of S), each term one rounded product then one rounded add (contraction off), then
//                   the fixed LDS tree of k_shapley.  A set holding a null player sums exact zeros: exactly 0.
// No atomics, no scratch, no dynamic LDS: deterministic.
#pragma once

namespace cf {

constexpr int kDivTileBits = 12;
constexpr int kDivTile = 1 << kDivTileBits;      // words per LDS tile
constexpr int kDivMaxOut = 2;                    // cf_create accepts n_out 1 or 2
constexpr int kDivThreads = 256;

struct MoebiusArgs {
    const float* v;                          // [B, 2^P, n_out]  (k_moebius_high: unused)
    float* div;                              // [B, 2^P, n_out]
    float* mass;                             // [B, 2^P, n_out], or null (then gridDim.z = 1)
    int P, n_out;
};

template <bool kMass>
__device__ __forceinline__ float moebius_step(float hi, float lo) {
    return kMass ? __fadd_rn(hi, lo) : __fsub_rn(hi, lo);
}

// The LDS stages of one tile: n = min(2^P, kDivTile) words of n_out columns at src -> dst.
template <bool kMass>
__device__ __forceinline__ void moebius_tile(const float* __restrict__ src, float* __restrict__ dst, float* t, int stages, int n_out, int tid) {
    const int ne = (1 << stages) * n_out;            // floats of the tile: element e = word * n_out + column
    for (int e = tid; e < ne; e += kDivThreads) t[e] = kMass ? fabsf(src[e]) : src[e];
    __syncthreads();
    const int half = 1 << (stages - 1);
    for (int k = 0; k < stages; ++k) {
        const int low = (1 << k) - 1;
        for (int x = tid; x < half * n_out; x += kDivThreads) {
            const int q = x / n_out, o = x - q * n_out;
            const int m = (q & ~low) << 1 | (q & low);      // the q-th word of the tile with bit k clear
            const int hi = (m | 1 << k) * n_out + o;
            t[hi] = moebius_step<kMass>(t[hi], t[m * n_out + o]);
        }
        __syncthreads();
    }
    for (int e = tid; e < ne; e += kDivThreads) dst[e] = t[e];
}

__global__ __launch_bounds__(kDivThreads) void k_moebius(MoebiusArgs a) {
    __shared__ float t[kDivTile * kDivMaxOut];
    const int stages = a.P < kDivTileBits ? a.P : kDivTileBits;
    // gene b, tile blockIdx.y: the tiles of a gene are consecutive
    const size_t at = (((size_t)blockIdx.x << a.P) + ((size_t)blockIdx.y << stages)) * a.n_out;
    if (blockIdx.z == 0)
        moebius_tile<false>(a.v + at, a.div + at, t, stages, a.n_out, threadIdx.x);
    else
        moebius_tile<true>(a.v + at, a.mass + at, t, stages, a.n_out, threadIdx.x);
}

// Stages kDivTileBits .. kDivTileBits + kStages - 1 of one table of one gene, in place.
template <int kStages, bool kMass>
__device__ __forceinline__ void moebius_high(float* __restrict__ p, size_t step, int l) {
    constexpr int R = 1 << kStages;
    float x[R];
#pragma unroll
    for (int r = 0; r < R; ++r) x[r] = p[(size_t)r * step + l];
#pragma unroll
    for (int s = 0; s < kStages; ++s)
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (r >> s & 1) x[r] = moebius_step<kMass>(x[r], x[r ^ 1 << s]);
#pragma unroll
    for (int r = 0; r < R; ++r) p[(size_t)r * step + l] = x[r];
}

template <int kStages>
__global__ __launch_bounds__(kDivThreads) void k_moebius_high(MoebiusArgs a) {
    const int step = kDivTile * a.n_out;                                // floats between a thread's values
    const int l = blockIdx.y * kDivThreads + threadIdx.x;               // (low word, column); gridDim.y * kDivThreads = step
    const size_t at = ((size_t)blockIdx.x << a.P) * a.n_out;
    if (blockIdx.z == 0)
        moebius_high<kStages, false>(a.div + at, step, l);
    else
        moebius_high<kStages, true>(a.mass + at, step, l);
}

struct SetIndexArgs {
    const float* div;                        // [B, 2^P, n_out]
    const unsigned* sets;                    // [n_sets] (device): the words of the listed sets
    float* out;                              // [B, n_sets, n_out]
    float wt[kCoalMaxS][kCoalMaxS];          // wt[|S| - 1][|U| - 1]
    int P, n_out, n_sets;
    int copy_below;                          // a set with fewer players carries its dividend's bits (sti: the top order; sii: 0)
};

__global__ __launch_bounds__(kShapThreads) void k_set_index(SetIndexArgs a) {
    static_assert(kShapThreads == kCoalMaxS * kCoalMaxS, "one thread per weight");
    __shared__ float sw[kCoalMaxS * kCoalMaxS];
    __shared__ float red[kShapThreads];
    const int b = blockIdx.x, s = blockIdx.y, tid = threadIdx.x, P = a.P, n_out = a.n_out;
    const unsigned S = a.sets[s];
    const int size = __popc(S);
    const float* __restrict__ d = a.div + ((size_t)b << P) * n_out;
    float* __restrict__ out = a.out + ((size_t)b * a.n_sets + s) * n_out;
    if (size < a.copy_below) {
        for (int o = tid; o < n_out; o += kShapThreads) out[o] = d[(size_t)S * n_out + o];
        return;
    }
    sw[tid] = (&a.wt[0][0])[tid];
    __syncthreads();
    const float* w = sw + (size - 1) * kCoalMaxS;      // w[|U| - 1]
    const unsigned n = 1u << (P - size);
    for (int o = 0; o < n_out; ++o) {
#pragma clang fp contract(off)
        float acc = 0.f;
        for (unsigned q = tid; q < n; q += kShapThreads) {
            unsigned m = q;      // a zero opened at every bit of S, lowest first: the q-th word that holds no player of S
            for (unsigned rest = S; rest; rest &= rest - 1) {
                const unsigned low = (rest & -rest) - 1u;
                m = (m & ~low) << 1 | (m & low);
            }
            const unsigned U = m | S;
            const float term = w[__popc(U) - 1] * d[(size_t)U * n_out + o];
            acc = acc + term;
        }
        red[tid] = acc;
        __syncthreads();
        for (int h = kShapThreads / 2; h > 0; h >>= 1) {
            if (tid < h) red[tid] = __fadd_rn(red[tid], red[tid + h]);
            __syncthreads();
        }
        if (tid == 0) out[o] = red[0];
        __syncthreads();
    }
}

}  // namespace cf
