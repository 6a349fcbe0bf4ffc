// hops_attended_story.h -- "attended slots" per story: the k memory rows a hop weighted most, chosen inside the kernels that give
// every query its OWN memory (hops_small.h::k_hops_small up to 64 slots, batch_hops.hip::k_hops_fixed beyond), so that no
// [n_hop][rows_total] probability array is written.  The shared-plane kernels have hops_attended.h; the contract is the same.
//
// The order is that of the `probs` tap: larger probability first, equal probabilities (equal FLOATS, also from different score
// bins) lower slot first, the slot counted from the story's first row.  A NaN probability (0 / 0 under the shift-based
// normaliser) ranks below every number.  Entries past min(k, S) hold slot 0xFFFFFFFF and probability 0.
//
//   story_select_wave   one wavefront, slot r in lane r with its probability in a register (k_hops_small behind its softmax, every
//                       MODE): min(k, S) rounds of "wavefront maximum over the lanes not yet taken, lowest such lane".  No LDS,
//                       no barrier; the maximum runs on the DPP network.
//   story_select_hist   a workgroup of one or four wavefronts behind finish_hop of k_hops_fixed, from what the histogram softmax
//                       leaves in LDS: hist[0..255] the merged counts per score code, ptab[0..255] the probability per code (0
//                       for an empty bin), `sc` the score byte of every slot.  The steps are those of
//                       hops_attended.h::attended_select -- slots above each bin, the threshold bin, one ordered walk over the
//                       score bytes with a block prefix (no atomics: places are in slot order), a rank sort of at most 16
//                       entries -- with each thread owning 256 / blockDim.x bins and the walk's chunk blockDim.x . 16 slots.
#pragma once
#include "hops_common.h"

namespace {

// launch argument of the kernels' TOP builds; the other builds take an EMPTY one and keep their device code
template <bool TOP> struct StoryTop {};
template <> struct StoryTop<true> {
    uint32_t *slot;          // [n_query][n_hop][k]
    float *p;                // [n_query][n_hop][k]
    uint32_t k;              // 1 .. QMANN_MAX_TOP_SLOTS
};

// the order key of a probability (hops_attended.h::att_key)
__device__ __forceinline__ float story_key(float p) { return p == p ? p : -INFINITY; }

// wavefront maximum on the DPP network (row shifts, then the two row broadcasts; lane 63 holds it and hands it to every lane
// through an SGPR): the pattern of hops_lean.h::wave_max_f32
__device__ __forceinline__ float story_wave_max(float v)
{
    float r = v;                                        // identity for lanes the shift does not reach: -inf
#define QM_STORY_MAXF(CTRL, RM) r = fmaxf(r, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp((int)0xFF800000, __builtin_bit_cast(int, r), CTRL, RM, 0xF, false)))
    QM_STORY_MAXF(0x111, 0xF); QM_STORY_MAXF(0x112, 0xF); QM_STORY_MAXF(0x114, 0xF); QM_STORY_MAXF(0x118, 0xF); QM_STORY_MAXF(0x142, 0xA); QM_STORY_MAXF(0x143, 0xC);
#undef QM_STORY_MAXF
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, r), 63));
}

// Called by the whole wavefront; `row` = q . n_hop + h; lane r < S holds the probability of slot r (S <= 64).
__device__ __forceinline__ void story_select_wave(const StoryTop<true> &tp, size_t row, uint32_t S, float p, uint32_t lane)
{
    const uint32_t k = tp.k, n_out = k < S ? k : S;
    const float key = story_key(p);
    uint64_t taken = S < (uint32_t)kWave ? ~0ull << S : 0ull;             // (wavefront-uniform: lanes without a slot never compete)
    for (uint32_t j = 0; j < n_out; j++) {
        const bool open = !((taken >> lane) & 1ull);
        const float mx = story_wave_max(open ? key : -INFINITY);
        const uint64_t at = __ballot(open && key == mx);                  // (never empty: j < S lanes are taken so far)
        const uint32_t pick = (uint32_t)__builtin_ctzll(at);
        if (lane == pick) {
            tp.slot[row * k + j] = lane;
            tp.p[row * k + j] = p;
        }
        taken |= 1ull << pick;
    }
    if (lane >= n_out && lane < k) {
        tp.slot[row * k + lane] = 0xFFFFFFFFu;
        tp.p[row * k + lane] = 0.0f;
    }
}

// Called by the whole workgroup (blockDim.x = 64 or 256) behind finish_hop; `row` = q . n_hop + h.  Ends with a barrier.
// LDS: live_row (the entries), cls = live_kp (class per bin), misc[2], misc[4..11] and red, all free behind finish_hop.
__device__ __forceinline__ void story_select_hist(const StoryTop<true> &tp, size_t row, uint32_t S, const uint32_t *hist, const float *ptab,
                                                  const int8_t *sc, uint32_t *live_row, uint8_t *cls, uint32_t *misc, double *red,
                                                  uint32_t tid, uint32_t lane, uint32_t wave)
{
    static_assert(QMANN_MAX_TOP_SLOTS * 2 <= kLiveCap, "the entries live in live_row");
    static_assert(QMANN_MAX_TOP_SLOTS <= kWave, "one thread of the first wavefront per entry");
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const uint32_t nthreads = blockDim.x, nwaves = nthreads / kWave;
    const uint32_t k = tp.k, n_out = k < S ? k : S;
    if (S == 0) {                                               // (workgroup-uniform) no softmax has run: the tables are stale
        if (tid < k) {
            tp.slot[row * k + tid] = 0xFFFFFFFFu;
            tp.p[row * k + tid] = 0.0f;
        }
        return;
    }
    uint32_t *ent_slot = live_row;
    float *ent_p = (float *)(live_row + QMANN_MAX_TOP_SLOTS);

    // 1. slots above each of this thread's bins; its lowest bin that still reaches into the first k
    float cand = INFINITY;
    uint32_t cand_above = 0;
    for (uint32_t b = tid; b < 256; b += nthreads) {
        if (!hist[b]) continue;
        const float kd = story_key(ptab[b]);
        uint32_t above = 0;
#pragma unroll 8                                                // (the reads are independent: eight pairs in flight)
        for (uint32_t d = 0; d < 256; d += 4) {
            const f32x4 p4 = *(const f32x4 *)(ptab + d);
            const u32x4 h4 = *(const u32x4 *)(hist + d);
#pragma unroll
            for (int i = 0; i < 4; i++) above += story_key(p4[i]) > kd ? h4[i] : 0u;
        }
        if (above < k && kd < cand) { cand = kd; cand_above = above; }
    }
    // 2. the threshold: the lowest probability that still reaches into the first k
    const float thr = -block_max<float>(-cand, (float *)red, lane, wave);
    if (cand == thr) misc[2] = cand_above;                      // (every bin at the threshold holds the same count)
    for (uint32_t b = tid; b < 256; b += nthreads) {
        const float kd = story_key(ptab[b]);
        cls[b] = kd > thr ? 2 : (kd == thr ? 1 : 0);           // (an empty bin's class is never looked up)
    }
    __syncthreads();
    const uint32_t gt = misc[2], m = n_out - gt;

    // 3. the ordered walk
    uint32_t run_gt = 0, run_eq = 0;
    for (uint32_t c0 = 0, it = 0; c0 < S; c0 += nthreads * 16u, it++) {
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
        for (uint32_t w = 0; w < nwaves; w++) {
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
            const float kk = story_key(p);
            rank = 0;
            for (uint32_t j = 0; j < n_out; j++) {
                const float kj = story_key(ent_p[j]);
                rank += (kj > kk || (kj == kk && ent_slot[j] < slot)) ? 1u : 0u;
            }
        }
        tp.slot[row * k + rank] = slot;
        tp.p[row * k + rank] = p;
    }
    __syncthreads();
}

// what the top call refuses behind its base call and its mode and length limits (as hops_attended.h::att_top_args_ok)
inline bool story_top_args_ok(uint32_t k, const uint32_t *top_slot, const float *top_p)
{
    return k >= 1 && k <= (uint32_t)QMANN_MAX_TOP_SLOTS && top_slot && top_p;
}

}  // namespace
