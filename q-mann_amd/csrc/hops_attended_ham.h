// hops_attended_ham.h -- "attended slots" for the packed Hamming forms (V0 / V1): the k memory rows a hop weighted most, per query,
// chosen inside the shared-plane Hamming kernels (batch_hops_shared_ham.hip::k_hops_shared_ham,
// batch_hops_shared_split_ham.hip::k_shared_split_finish_ham), so that no [n_hop][n_query][n_slots] probability array is ever
// written.  The fixed-point form is hops_attended.h; the contract is the same.
//
// The order is that of the `probs` tap: larger probability first, equal probabilities (equal FLOATS, whatever their scores: the
// zero region of exp_plan, underflow, a single plane under V1) lower slot first.  A NaN probability (0 / 0 under the shift-based
// normaliser) ranks below every number.  ham_att_key maps a probability to an unsigned key with exactly that order.
//
// A slot's probability is a function of its int16 score alone -- V0: the table v0_p the histogram softmax leaves behind, V1:
// sm_quot(sm_exp(x - xmax), total), the expression of the tap path, handed over by ham_slot_softmax_survivors as a callable while
// xmax, total and the scores are still there (ham_common.h: before the survivor overflow parks Q(p) in the scores).  So both
// modes run one selection, ham_attended_select(items, p_of):
//   1. the threshold.  Every thread looks at its own items (V0: the non-empty bins d = tid, tid + 256, ..., at most 9, each with
//      its count; V1: the slots r = tid, tid + 256, ...) and keeps its two largest keys below the level taken last and how many
//      of its slots carry each.  A block-wide maximum takes the next level; a thread that held it moves its second key up, and
//      looks at its items again only when it has held two levels since its last look (a V1 look costs an exp and a double
//      division per slot while the other threads wait, so looks are what to save).  The sum of the counts at a level rides along
//      with the next maximum, so a level costs one reduction (two barriers).  At most k + 1 reductions, fewer when a level holds
//      many slots: the walk over levels ends when min(k, S) slots are covered.  That gives the threshold key and `gt`, the slots
//      above it (gt < k); the first m = min(k, S) - gt slots BY INDEX at the threshold complete the row.  No pass over bins x
//      bins, and no pass over the scores per level but by a thread that holds every third level.
//   2. the ordered walk: chunks of 256 threads x 8 scores (one 16-byte read each).  Every thread counts its slots above and at
//      the threshold, a block exclusive prefix of the two counts gives each such slot its place -- no atomics, so the places are
//      in slot order -- and the walk ends (workgroup-uniform) once all gt and m are placed.  One barrier per chunk.
//   3. thread j < k ranks entry j among the at most 16 by (key descending, slot ascending) and writes it at its rank; places
//      past min(k, S) get slot 0xFFFFFFFF and probability 0.
// LDS: 48 words of the query's own slice that the Hamming kernels carve (ham_lds_bytes) and use for nothing behind the scan:
// bytes 512 .. 703 of the histogram area, behind the attention bytes and plane words (`ub`, `upl`).  The survivor list, misc
// and red are left alone, so the V1 selection can run between the survivor search and finish_hop.
#pragma once
#include "hops_shared_ham.h"

namespace {

// launch argument of the kernels' TOP builds; the other builds take an EMPTY one and keep their device code
template <bool TOP> struct HamTop {};
template <> struct HamTop<true> {
    uint32_t *slot;          // [n_query][n_hop][k]
    float *p;                // [n_query][n_hop][k]
    uint32_t k;              // 1 .. QMANN_MAX_TOP_SLOTS
};

constexpr uint32_t kOffAttHam = kOffUpl + 4 * 8 * 8;             // u32 [48]: reductions [8], walk totals [8], entries [16 + 16]
static_assert(kOffAttHam % 16 == 0 && kOffAttHam + 48 * 4 <= kOffPtab, "the selection's words must fit the histogram area");
__device__ __forceinline__ uint32_t *ham_att_words(const HamQueryLds &L) { return (uint32_t *)(L.ub - kOffUb + kOffAttHam); }

// larger probability <-> larger key; NaN: 1, below every number (-inf: 0x00800000); 0: "no item"
__device__ __forceinline__ uint32_t ham_att_key(float p)
{
    if (!(p == p)) return 1u;
    const uint32_t b = __float_as_uint(p + 0.0f);                // (-0 + 0 = +0: the two zeros are equal floats)
    return ((b & 0x80000000u) ? ~b : (b | 0x80000000u)) + 1u;
}

// Called by the whole workgroup (kBlock threads); `row` = q . n_hop + h; S > 0 scores in `sc` (padded to 8).
// for_items(f): calls f(key, n) for each of this thread's items -- its order key and the number of its SLOTS that carry it.
// p_of(score): the probability of a slot with that score.  Ends with a barrier.
template <typename ForItems, typename POf>
__device__ __forceinline__ void ham_attended_select(const HamTop<true> &tp, size_t row, uint32_t S, const int16_t *sc,
                                                    ForItems for_items, POf p_of, uint32_t *words, uint32_t tid, uint32_t lane,
                                                    uint32_t wave)
{
    static_assert(kWaves == 4, "four wavefronts' partial results per reduction");
    uint32_t *red_max = words, *red_sum = words + 4, *wtot = words + 8, *ent_slot = words + 16;
    float *ent_p = (float *)(words + 16 + QMANN_MAX_TOP_SLOTS);
    const uint32_t k = tp.k, n_out = k < S ? k : S;

    // 1. the threshold key and the slots above it
    uint32_t thr = 0, gt = 0;
    {
        // this thread's two largest distinct keys below `below` and their slot counts (key 0: none)
        uint32_t best, cnt, next, ncnt;
        auto look = [&](uint32_t below) {
            best = cnt = next = ncnt = 0;
            for_items([&](uint32_t key, uint32_t n) {
                if (key >= below) return;
                if (key > best) { next = best; ncnt = cnt; best = key; cnt = n; }
                else if (key == best) cnt += n;
                else if (key > next) { next = key; ncnt = n; }
                else if (key == next) ncnt += n;
            });
        };
        uint32_t pend = 0, cum = 0, level = 0;
        bool have_next = true;
        look(0xFFFFFFFFu);
        for (;;) {
            uint32_t m = best, s = pend;                        // the next level; the slots at the level taken last
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const uint32_t t = __shfl_xor(m, o);
                m = t > m ? t : m;
                s += __shfl_xor(s, o);
            }
            if (lane == 0) { red_max[wave] = m; red_sum[wave] = s; }
            __syncthreads();
            m = red_max[0]; s = red_sum[0];
#pragma unroll
            for (int i = 1; i < kWaves; i++) { m = red_max[i] > m ? red_max[i] : m; s += red_sum[i]; }
            __syncthreads();
            if (cum + s >= n_out) { thr = level; gt = cum; break; }         // workgroup-uniform
            cum += s;
            level = m;
            if (m == 0) { thr = 0; gt = cum; break; }                       // (cannot happen: S >= n_out slots carry a key)
            pend = 0;
            if (best == m) {
                pend = cnt;
                if (have_next) { best = next; cnt = ncnt; have_next = false; }
                else { look(m); have_next = true; }
            }
        }
    }
    const uint32_t m_eq = n_out - gt;

    // 2. the ordered walk
    uint32_t run_gt = 0, run_eq = 0;
    for (uint32_t c0 = 0, it = 0; c0 < S; c0 += (uint32_t)kBlock * 8u, it++) {
        const uint32_t rb = c0 + tid * 8u;
        i32x4 v = {0, 0, 0, 0};
        if (rb < S) v = *(const i32x4 *)(sc + rb);            // (the score array is padded to 8 rows)
        float p[8];
        uint32_t cl = 0, x = 0;                                 // class per score, 2 bits each; counts: at | above << 16
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int code = rb + i < S ? (int)(int16_t)((uint32_t)v[i / 2] >> (16 * (i % 2))) : 0;
            p[i] = p_of(code);
            const uint32_t key = ham_att_key(p[i]);
            const uint32_t c = rb + i < S ? (key > thr ? 2u : (key == thr ? 1u : 0u)) : 0u;
            cl |= c << (2 * i);
            x += c == 1u ? 1u : (c == 2u ? 0x10000u : 0u);
        }
        uint32_t inc = x;
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1) {
            const uint32_t t = __shfl_up(inc, o);
            if (lane >= (uint32_t)o) inc += t;
        }
        uint32_t *wt = wtot + (it & 1u) * kWaves;              // (two sets in turn: one barrier per chunk)
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
            for (int i = 0; i < 8; i++) {
                const uint32_t c = (cl >> (2 * i)) & 3u;
                if (c) {
                    uint32_t at = QMANN_MAX_TOP_SLOTS;
                    if (c == 2u) at = r_gt++;
                    else if (r_eq++ < m_eq) at = gt + r_eq - 1u;
                    if (at < (uint32_t)QMANN_MAX_TOP_SLOTS) { ent_slot[at] = rb + i; ent_p[at] = p[i]; }
                }
            }
        }
        run_eq += tot & 0xFFFFu;
        run_gt += tot >> 16;
        if (run_gt == gt && run_eq >= m_eq) break;              // workgroup-uniform
    }
    __syncthreads();

    // 3. rank and write
    if (tid < k) {
        uint32_t slot = 0xFFFFFFFFu, rank = tid;
        float pv = 0.0f;
        if (tid < n_out) {
            slot = ent_slot[tid];
            pv = ent_p[tid];
            const uint32_t kk = ham_att_key(pv);
            rank = 0;
            for (uint32_t j = 0; j < n_out; j++) {
                const uint32_t kj = ham_att_key(ent_p[j]);
                rank += (kj > kk || (kj == kk && ent_slot[j] < slot)) ? 1u : 0u;
            }
        }
        tp.slot[row * k + rank] = slot;
        tp.p[row * k + rank] = pv;
    }
    __syncthreads();
}

// V0, behind ham_hist_softmax_survivors: the items are the non-empty bins of v0_hist, a slot's probability is v0_p[score]
__device__ __forceinline__ void ham_attended_select_v0(const HamTop<true> &tp, size_t row, uint32_t S, uint32_t nbins, const int16_t *sc,
                                                       const uint32_t *v0_hist, const float *v0_p, uint32_t *words, uint32_t tid,
                                                       uint32_t lane, uint32_t wave)
{
    auto for_items = [&](auto f) {
        for (uint32_t d = tid; d < nbins; d += kBlock) {
            const uint32_t n = v0_hist[d];
            if (n) f(ham_att_key(v0_p[d]), n);
        }
    };
    ham_attended_select(tp, row, S, sc, for_items, [&](int code) { return v0_p[code]; }, words, tid, lane, wave);
}

// V1: what ham_slot_softmax_survivors calls with the probability of a score (its `select` argument); the items are the slots
struct HamSelectV1 {
    const HamTop<true> &tp;
    size_t row;
    uint32_t S;
    const int16_t *sc;
    uint32_t *words;
    uint32_t tid, lane, wave;
    template <typename POf>
    __device__ __forceinline__ void operator()(POf p_of) const
    {
        auto for_items = [&](auto f) {
            for (uint32_t r = tid; r < S; r += kBlock) f(ham_att_key(p_of((int)sc[r])), 1u);
        };
        ham_attended_select(tp, row, S, sc, for_items, p_of, words, tid, lane, wave);
    }
};

// what both top calls refuse beyond their base calls
inline bool ham_top_args_ok(uint32_t k, const uint32_t *top_slot, const float *top_p)
{
    return k >= 1 && k <= (uint32_t)QMANN_MAX_TOP_SLOTS && top_slot && top_p;
}

}  // namespace
