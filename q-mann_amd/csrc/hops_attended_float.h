// hops_attended_float.h -- "attended slots" for float attention (ATTENTION_MODE 1): the k memory rows a hop weighted most, chosen
// inside k_hops_float and k_hops_shared_float behind the softmax of the query's hop, so that no probability array is written.
// hops_attended.h and hops_attended_story.h pick from the 256 score bins of the fixed-point softmax; here there are no bins:
// the query's LDS slice holds S arbitrary floats p (S up to 38 368), and the selection runs over them.
//
// The order is that of the `probs` tap: larger probability first, equal FLOATS lower slot first, a NaN probability (0 / 0 under
// the shift-based normaliser, which float attention does reach: a total below sqrt 2 divides by llrint(log2 total) = 0) below
// every number (att_key).  Entries past min(k, S) hold slot 0xFFFFFFFF and probability 0.  top_p is the float in LDS itself.
//
// Method: rounds of a block arg-max, with every thread's own best kept in registers between the rounds.
//   1. thread t reads its slots t, t + 256, ... once and keeps the first of them in the order, (key, slot);
//   2. round j = 0 .. min(k, S) - 1: the first of the 256 kept entries is the j-th attended slot -- a wavefront reduction on the
//      DPP network (maximum of the keys, then the minimum slot among the lanes that hold it), the four wavefronts' results
//      through `red` (two sets of four pairs used in turn: ONE barrier per round);
//   3. only the picked thread's kept entry is now stale.  Its WAVEFRONT re-reads that thread's slots, 64 per step, keeps the
//      first entry BEHIND the pick in the order, and hands it to the picked thread; the other three wavefronts go on to the
//      barrier.
// Exact, no atomics, no scratch but `red`; reads p only.  Per (query, hop): S / 256 LDS reads per thread, then per round two
// wavefront reductions, one barrier and S / 16 384 reads per lane of one wavefront.
//
// Why not the plain form of the rounds (every thread re-reads all its slots in every round: k S / 256 reads per thread -- 640 at
// 10 000 slots and k = 16, twice the 312 16-byte loads per thread of the hop's key scan), and why not a radix select on the
// integer image of the key: the radix select needs four histogram passes over all S floats with LDS atomics (or 256-way private
// counts) before the ordered walk, whatever k is, and k is at most 16; the rounds above read every float once and then touch
// S / 256 floats per round.  Measured: DESIGN.md section 5, "Measured, attended slots, float".
#pragma once
#include "hops_att_top.h"

namespace {

// wavefront reductions on the DPP network (row shifts, then the two row broadcasts; lane 63 holds the result and hands it to
// every lane through an SGPR): the pattern of hops_attended_story.h::story_wave_max
__device__ __forceinline__ float attf_wave_max(float v)
{
    float r = v;                                        // identity for lanes the shift does not reach: -inf
#define QM_ATTF_MAX(CTRL, RM) r = fmaxf(r, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp((int)0xFF800000, __builtin_bit_cast(int, r), CTRL, RM, 0xF, false)))
    QM_ATTF_MAX(0x111, 0xF); QM_ATTF_MAX(0x112, 0xF); QM_ATTF_MAX(0x114, 0xF); QM_ATTF_MAX(0x118, 0xF); QM_ATTF_MAX(0x142, 0xA); QM_ATTF_MAX(0x143, 0xC);
#undef QM_ATTF_MAX
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, r), 63));
}
__device__ __forceinline__ uint32_t attf_wave_min(uint32_t v)
{
    uint32_t r = v;                                     // identity: 0xFFFFFFFF
#define QM_ATTF_MIN(CTRL, RM) do { const uint32_t t_ = (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)r, CTRL, RM, 0xF, false); r = t_ < r ? t_ : r; } while (0)
    QM_ATTF_MIN(0x111, 0xF); QM_ATTF_MIN(0x112, 0xF); QM_ATTF_MIN(0x114, 0xF); QM_ATTF_MIN(0x118, 0xF); QM_ATTF_MIN(0x142, 0xA); QM_ATTF_MIN(0x143, 0xC);
#undef QM_ATTF_MIN
    return (uint32_t)__builtin_amdgcn_readlane((int)r, 63);
}

// an entry of the order: the key of a probability and its slot; "no entry" is (-inf, 0xFFFFFFFF), behind every slot there is
struct AttfEntry {
    float key;
    uint32_t slot;
};
__device__ __forceinline__ bool attf_before(float ka, uint32_t sa, float kb, uint32_t sb) { return ka > kb || (ka == kb && sa < sb); }

// the first of the wavefront's 64 entries; every lane gets it
__device__ __forceinline__ AttfEntry attf_wave_first(float key, uint32_t slot)
{
    const float mx = attf_wave_max(key);
    const uint32_t ms = attf_wave_min(key == mx ? slot : 0xFFFFFFFFu);
    return AttfEntry{mx, ms};
}

// Called by the whole workgroup (kBlock threads) behind the barrier that follows the softmax, before anything overwrites p;
// `row` = q . n_hop + h; pf[0 .. S): the query's probabilities; red: the query's 8 doubles.  Needs no barrier behind it: it
// writes nothing but `red`, which the next hop's softmax is the first to touch again.
__device__ __forceinline__ void attended_select_float(const AttTop<true> &tp, size_t row, uint32_t S, const float *pf, double *red,
                                                      uint32_t tid, uint32_t lane, uint32_t wave)
{
    static_assert(2 * kWaves * sizeof(uint2) <= 8 * sizeof(double), "two sets of one pair per wavefront fit `red`");
    static_assert(QMANN_MAX_TOP_SLOTS <= kBlock, "one thread per place of padding");
    const uint32_t k = tp.k, n_out = k < S ? k : S;
    if (tid >= n_out && tid < k) {
        tp.slot[row * k + tid] = 0xFFFFFFFFu;
        tp.p[row * k + tid] = 0.0f;
    }

    // 1. the first of this thread's slots
    float bk = -INFINITY;
    uint32_t bs = 0xFFFFFFFFu;
    for (uint32_t r = tid; r < S; r += (uint32_t)kBlock) {
        const float kk = att_key(pf[r]);
        if (attf_before(kk, r, bk, bs)) { bk = kk; bs = r; }
    }

    uint2 *post = (uint2 *)red;
    for (uint32_t j = 0; j < n_out; j++) {
        // 2. the first of all kept entries (there is one: j < S slots are taken so far)
        const AttfEntry w = attf_wave_first(bk, bs);
        uint2 *set = post + (j & 1u) * kWaves;
        if (lane == 0) set[wave] = uint2{__builtin_bit_cast(uint32_t, w.key), w.slot};
        __syncthreads();
        float pk = __builtin_bit_cast(float, set[0].x);
        uint32_t ps = set[0].y;
#pragma unroll
        for (int i = 1; i < kWaves; i++) {
            const float ki = __builtin_bit_cast(float, set[i].x);
            const uint32_t si = set[i].y;
            if (attf_before(ki, si, pk, ps)) { pk = ki; ps = si; }
        }
        if (ps >= S) break;                                     // (workgroup-uniform; never taken: see 2.)
        const uint32_t owner = ps % (uint32_t)kBlock;
        if (tid == owner) {
            tp.slot[row * k + j] = ps;
            tp.p[row * k + j] = pf[ps];
        }
        if (j + 1 == n_out) break;
        // 3. the picked thread's next entry, found by its wavefront
        if (wave == owner / (uint32_t)kWave) {
            float ck = -INFINITY;
            uint32_t cs = 0xFFFFFFFFu;
            for (uint32_t r = owner + lane * (uint32_t)kBlock; r < S; r += (uint32_t)(kBlock * kWave)) {
                const float kk = att_key(pf[r]);
                if (attf_before(pk, ps, kk, r) && attf_before(kk, r, ck, cs)) { ck = kk; cs = r; }
            }
            const AttfEntry n = attf_wave_first(ck, cs);
            if (tid == owner) { bk = n.key; bs = n.slot; }
        }
    }
}

}  // namespace
