// cf_x0_gather.h -- training on a frozen trunk from cached trunk outputs (cf_trunk_outputs, cf_forward_train_x0, cf_x0_gather*,
// cf_reduce_opt_x0; included by cf_api.hip).
//
// With the Embedding + Pairwise weights fixed, the Regulation input Rx[r][0] ([T, d_emb] per gene and resolution) depends on the gene
// alone (cf_coalition.h): it is computed once per gene, kept in a device-resident cache store beside the gene's interaction mask,
// interaction frequencies and label, and a training step starts at the Regulation stack.  The kernels here move bytes only (no
// arithmetic on them, no atomics):
//   k_x0_copy            [B, T, d_emb] rows between Rx[r][0] and a caller's buffers, float4 per thread, blockIdx.y = resolution;
//   k_x0_gather          one workgroup per (gene slot of the batch, segment): that gene's bytes of one cache array -> the buffer the
//                        step reads (Rx[r][0], the slot's interaction masks / frequencies / labels); 16-byte loads and stores where the
//                        rows allow (the x0 rows: T * d_emb * 4 bytes), 4-byte ones for the frequencies and labels (T * T * 4 = 324
//                        bytes at the default shape: no multiple of 16), the T * T = 81-byte masks byte by byte;
//   k_x0_prologue        the same copy blocks behind the re-tiling of the Regulation + head weights the step's kernels read: the one
//                        launch in front of a frozen-trunk step (as k_prologue_gather is for the full step);
//   k_reduce_opt_x0      k_reduce_opt (same tile functions, same arithmetic) with ONE more workgroup that advances the feed's cursor --
//                        which the gather reads, so it cannot move in the gather's launch; the full step leaves that to the trunk's
//                        forward launch, which does not run here -- and appends the step's log rows (cf_record_step).
// The order / cursor protocol and the error flags are cf_gather_batch's (cf_gather.h).
#pragma once

namespace cf {

constexpr int kX0Threads = 256;
constexpr int kX0MaxSeg = 2 * kMaxRes + 2;      // x0 and interaction mask per resolution, interaction_freq, labels

struct X0CopyArgs {
    const float4* src[kMaxRes];
    float4* dst[kMaxRes];
    long long n4;                            // B * T * d_emb / 4
};
__global__ __launch_bounds__(kX0Threads) void k_x0_copy(X0CopyArgs a) {
    const int r = blockIdx.y;
    const float4* __restrict__ src = a.src[r];
    float4* __restrict__ dst = a.dst[r];
    for (long long i = (long long)blockIdx.x * kX0Threads + threadIdx.x; i < a.n4; i += (long long)gridDim.x * kX0Threads) dst[i] = src[i];
}

struct X0Seg {
    const char* src;      // cache array, [n_genes, gene_bytes]
    char* dst;            // step buffer, [B, gene_bytes]
    long long gene_bytes;
};
struct X0GatherArgs {
    X0Seg seg[kX0MaxSeg];
    int n_seg;
    const int* order;     // [n_batches * B] gene indices of the epoch, batch-major
    int* cursor;          // [0] = next batch, [1] = batches uploaded (bound), [2] = error flags (1: ran past the epoch, 2: bad gene index)
    long long n_genes;    // genes in the cache
    int B;
};
// segment segi of gene slot b of the batch (any workgroup of kX0Threads threads)
__device__ __forceinline__ void x0_gather_block(const X0GatherArgs& a, const int b, const int segi) {
    const int cur = a.cursor[0];
    if (cur < 0 || cur >= a.cursor[1]) {      // a step past the uploaded epoch: nothing is read (the step buffers keep the last batch)
        if (threadIdx.x == 0 && b == 0 && segi == 0) a.cursor[2] |= 1;
        return;
    }
    const long long gene = a.order[(long long)cur * a.B + b];
    if (gene < 0 || gene >= a.n_genes) {
        if (threadIdx.x == 0) a.cursor[2] |= 2;      // (same value from every writer)
        return;
    }
    const X0Seg s = a.seg[segi];
    const char* src = s.src + gene * s.gene_bytes;
    char* dst = s.dst + (long long)b * s.gene_bytes;
    if ((((uintptr_t)src | (uintptr_t)dst | (uintptr_t)s.gene_bytes) & 15) == 0) {
        const uint4* __restrict__ s4 = reinterpret_cast<const uint4*>(src);
        uint4* __restrict__ d4 = reinterpret_cast<uint4*>(dst);
        for (long long i = threadIdx.x; i < s.gene_bytes / 16; i += kX0Threads) d4[i] = s4[i];
    } else if ((((uintptr_t)src | (uintptr_t)dst | (uintptr_t)s.gene_bytes) & 3) == 0) {
        const uint32_t* __restrict__ s1 = reinterpret_cast<const uint32_t*>(src);
        uint32_t* __restrict__ d1 = reinterpret_cast<uint32_t*>(dst);
        for (long long i = threadIdx.x; i < s.gene_bytes / 4; i += kX0Threads) d1[i] = s1[i];
    } else {
        for (long long i = threadIdx.x; i < s.gene_bytes; i += kX0Threads) dst[i] = src[i];
    }
}
__global__ __launch_bounds__(kX0Threads) void k_x0_gather(X0GatherArgs a) { x0_gather_block(a, blockIdx.x, blockIdx.y); }
__global__ __launch_bounds__(kX0Threads) void k_x0_prologue(const float* __restrict__ params, float* __restrict__ tiled, float* __restrict__ tiledT,
                                                            const RetileUnit* __restrict__ units, int n_units, X0GatherArgs ga) {
    if ((int)blockIdx.x < n_units) {
        retile_unit(params, tiled, tiledT, units[blockIdx.x]);
    } else {
        const int i = (int)blockIdx.x - n_units;
        x0_gather_block(ga, i % ga.B, i / ga.B);
    }
}

// Tile dispatch: EXACTLY k_reduce_opt's (cf_kernels.h) without the riders' skip window -- workgroups [0, xcd_grid(n_wg)) take weight-gradient
// tile xcd_tile(b), the next n_cs the column-sum tiles, both through wgrad_tile<true> / colsum_tile<true>; whoever changes one dispatcher
// changes the other (tests/test_frozen_trunk_gpu.py compares the two launches' gradients, parameters and moments bit for bit).  It is a
// kernel of its own because the cursor of a cached feed has to move on in a launch BEHIND the one whose gather blocks read it, and a
// frozen-trunk step has no trunk launch to carry that (the full step's k_trunk_fwd does); k_reduce_opt itself stays as shipped.
//
// The workgroup behind the tiles (the last of the step's last launch): the cursor moves on (every gather block of the step has long finished), then the
// step's logits / labels / loss go to the logs at the row of the step just taken (record_block reads the advanced cursor)
__global__ __launch_bounds__(256) void k_reduce_opt_x0(const WgTile* __restrict__ wg, int n_wg, const CsTile* __restrict__ cs, int n_cs, int batch, int xcd,
                                                       AdamFuse o, int* adv_cursor, RecordArgs rec) {
    const int nb = xcd_grid(n_wg);
    if ((int)blockIdx.x < nb) {
        const int t = xcd_tile(blockIdx.x, n_wg, xcd);
        if (t < n_wg) wgrad_tile<true>(wg[t], batch, &o);
    } else if ((int)blockIdx.x < nb + n_cs) {
        colsum_tile<true>(cs[blockIdx.x - nb], batch, &o);
    } else {
        if (adv_cursor) {
            if (threadIdx.x == 0 && adv_cursor[0] < adv_cursor[1]) adv_cursor[0] += 1;
            __threadfence();
            __syncthreads();
        }
        if (rec.cursor) record_block(rec);
    }
}

}  // namespace cf
