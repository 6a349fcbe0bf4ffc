// hops_attended.h -- "attended slots": the k memory rows a hop weighted most, per query, chosen inside the shared-plane kernels
// (batch_hops_shared.hip::k_hops_shared, batch_hops_shared_split.hip::k_shared_split_finish) behind finish_hop of the query's
// hop, so that no [n_hop][n_query][n_slots] probability array is ever written.
//
// The order is that of the `probs` tap: larger probability first, equal probabilities (equal FLOATS, also from different score
// bins: the zero region of exp_plan, underflow, a zero scale) lower slot first.  A NaN probability (0 / 0 under the shift-based
// normaliser) ranks below every number, as a sort of the tap puts it.
//
// When finish_hop has returned, hist[0..255] still holds the merged counts per score code, ptab[0..255] the probability per
// code (0 for an empty bin) and `sc` the score byte of every slot: finish_hop writes none of them.  So the top k over S slots
// is a top k over at most 255 bins plus one ordered walk over the score bytes:
//   1. thread d:  above[d] = slots whose probability is larger than bin d's (256 counts and probabilities, read 4 at a time);
//   2. the threshold p_thr = the smallest probability among the non-empty bins with above < k (one block reduction); `gt` slots
//      lie above it (gt < k), and the first m = min(k, S) - gt slots BY INDEX that equal it complete the row;
//   3. chunks of 256 threads x 16 score bytes (one 16-byte read each): every thread counts its slots above and at the threshold,
//      a block exclusive prefix of the two counts gives each such slot its place -- no atomics, so the places are in slot order
//      -- and the walk ends (workgroup-uniform) once all gt and m are placed.  At most ceil(S / 4096) chunks, one barrier each;
//   4. thread j < k ranks entry j among the at most 16 by (probability descending, slot ascending) and writes it at its rank;
//      places past min(k, S) get slot 0xFFFFFFFF and probability 0.
// LDS: the query's own live_row (entries), live_kp (class per bin), misc[2], misc[4..11] and red, all free behind finish_hop.
#pragma once
#include "hops_shared.h"
#include "hops_att_top.h"

namespace {

// Called by the whole workgroup (kBlock threads) behind finish_hop; `row` = q . n_hop + h.  Ends with a barrier.
__device__ __forceinline__ void attended_select(const AttTop<true> &tp, size_t row, uint32_t S, const uint32_t *hist, const float *ptab,
                                                const int8_t *sc, uint32_t *live_row, uint8_t *cls, uint32_t *misc, double *red,
                                                uint32_t tid, uint32_t lane, uint32_t wave)
{
    static_assert(kBlock == 256, "one thread per score bin");
    static_assert(QMANN_MAX_TOP_SLOTS * 2 <= kLiveCap, "the entries live in live_row");
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    uint32_t *ent_slot = live_row;
    float *ent_p = (float *)(live_row + QMANN_MAX_TOP_SLOTS);
    const uint32_t k = tp.k, n_out = k < S ? k : S;

    // 1. slots above this thread's bin
    const float kd = att_key(ptab[tid]);
    const uint32_t cnt = hist[tid];
    uint32_t above = 0;
#pragma unroll 8                                                // (the reads are independent: eight pairs in flight)
    for (uint32_t d = 0; d < 256; d += 4) {
        const f32x4 p4 = *(const f32x4 *)(ptab + d);
        const u32x4 h4 = *(const u32x4 *)(hist + d);
#pragma unroll
        for (int i = 0; i < 4; i++) above += att_key(p4[i]) > kd ? h4[i] : 0u;
    }
    // 2. the threshold: the lowest bin that still reaches into the first k
    const float cand = (cnt && above < k) ? kd : INFINITY;
    const float thr = -block_max<float>(-cand, (float *)red, lane, wave);
    if (cnt && kd == thr) misc[2] = above;                      // (every bin at the threshold holds the same count)
    cls[tid] = kd > thr ? 2 : (kd == thr ? 1 : 0);
    __syncthreads();
    const uint32_t gt = misc[2], m = n_out - gt;

    // 3. the ordered walk
    uint32_t run_gt = 0, run_eq = 0;
    for (uint32_t c0 = 0, it = 0; c0 < S; c0 += (uint32_t)kBlock * 16u, it++) {
        const uint32_t rb = c0 + tid * 16u;
        i32x4 v = {0, 0, 0, 0};
        if (rb < S) v = *(const i32x4 *)(sc + rb);            // (the score array is padded to 16 rows)
        uint32_t cl = 0, x = 0;                                 // class per byte, 2 bits each; counts: at | above << 16
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const int code = (int)(int8_t)((uint32_t)v[i / 4] >> (8 * (i % 4)));
            const uint32_t c = rb + i < S ? cls[code + 127] : 0u;
            cl |= c << (2 * i);
            x += c == 1u ? 1u : (c == 2u ? 0x10000u : 0u);
        }
        uint32_t inc = x;
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1) {
            const uint32_t t = __shfl_up(inc, o);
            if (lane >= (uint32_t)o) inc += t;
        }
        uint32_t *wt = misc + 4 + (it & 1u) * kWaves;          // (two sets in turn: one barrier per chunk)
        if (lane == kWave - 1) wt[wave] = inc;
        __syncthreads();
        uint32_t before = 0, tot = 0;
        for (uint32_t w = 0; w < (uint32_t)kWaves; w++) {
            const uint32_t t = wt[w];
            before += w < wave ? t : 0u;
            tot += t;
        }
        if (x) {
            const uint32_t exc = before + inc - x;
            uint32_t r_eq = run_eq + (exc & 0xFFFFu), r_gt = run_gt + (exc >> 16);
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const uint32_t c = (cl >> (2 * i)) & 3u;
                if (c) {
                    const int code = (int)(int8_t)((uint32_t)v[i / 4] >> (8 * (i % 4)));
                    uint32_t at = QMANN_MAX_TOP_SLOTS;
                    if (c == 2u) at = r_gt++;
                    else if (r_eq++ < m) at = gt + r_eq - 1u;
                    if (at < (uint32_t)QMANN_MAX_TOP_SLOTS) { ent_slot[at] = rb + i; ent_p[at] = ptab[code + 127]; }
                }
            }
        }
        run_eq += tot & 0xFFFFu;
        run_gt += tot >> 16;
        if (run_gt == gt && run_eq >= m) break;                 // workgroup-uniform
    }
    __syncthreads();

    // 4. rank and write
    if (tid < k) {
        uint32_t slot = 0xFFFFFFFFu, rank = tid;
        float p = 0.0f;
        if (tid < n_out) {
            slot = ent_slot[tid];
            p = ent_p[tid];
            const float kk = att_key(p);
            rank = 0;
            for (uint32_t j = 0; j < n_out; j++) {
                const float kj = att_key(ent_p[j]);
                rank += (kj > kk || (kj == kk && ent_slot[j] < slot)) ? 1u : 0u;
            }
        }
        tp.slot[row * k + rank] = slot;
        tp.p[row * k + rank] = p;
    }
    __syncthreads();
}

}  // namespace
