// answer_serial.h -- the answer layer's serial-order kernels: k_answer (one workgroup per query; with PRECOMPUTED logits it is
// also the second kernel of the int8 layer's two-kernel form) and k_answer_small (dictionaries up to 256), their ranked builds,
// and what the host needs to launch them: the LDS of a query and its limit, k_answer's grid, the k_answer_small build of a shape.
// batch_answer.hip launches the float layer with them, batch_answer_i8.hip the PRECOMPUTED builds.
#pragma once
#include "hops_common.h"

namespace {

// ---------------------------------------------------------------------------
// Answer layer.  One workgroup per query.  Thread v owns logit v and sums over
// the embedding axis serially in float (separate multiply and add), which is the
// exact operation order of the reference's serial loop (lib/layer_cuda.cu:70-80),
// so logits are bit-identical to it.  Softmax: e^(x-max), double normaliser,
// float quotient (:2006-2042) or the CPU form 2^(x-max) with float arithmetic
// (lib/layer.c:1225-1243).  Arg-max ties go to the highest index (:1918-1939).
// ---------------------------------------------------------------------------
// PRECOMPUTED: logits come from a buffer (written by the MFMA projection, answer_i8.h::k_logits_mfma_i8) instead of being
// computed here.
// TOPK (qmann_answer_topk_f32): instead of pred[q], the k best (probability, index) pairs of the query in the arg-max's own
// order -- larger probability first, equal probabilities: higher index first -- go to tk.idx / tk.p [n_query][k].  The
// probabilities are the ones the statements below leave in LDS, so they are the serial layer's bit for bit; k rounds of the
// arg-max reduction, a taken entry marked by a negative value (probabilities are >= 0).  k <= V: every round finds an untaken one.
// The ranked builds are instantiations of their own: the others take an EMPTY last argument and keep their device code.
// PRECOMPUTED && TOPK (qmann_answer_topk_i8's two-kernel form): the probabilities are formed by the same statements, but the k
// rounds rank by the LOGITS still in the buffer (float code . scale, exact: the order of the integer codes), ties to the higher
// index; what is listed is the probability LDS holds for the winner.  Distinct codes whose probabilities round to one float stay
// in logit order that way.
template <bool TOPK> struct AnsTopK {};
template <> struct AnsTopK<true> { uint32_t *idx; float *p; uint32_t k; };

// small_lpq / small_vpt (PRECOMPUTED only; 0: not used): the shape of the k_answer_small build that serves this dictionary in the
// float layer (lanes per query, adjacent logits per lane).  The double normaliser is then added up in THAT kernel's order -- a
// lane's logits one after the other, the lanes pairwise as its butterfly joins them -- instead of this kernel's strided one: two
// orders give totals one unit in the last place apart (2 and 2 + 2^-51 where two tied answers carry the sum), and the quotient
// of a denormal e by them rounds to different floats (e / 2 of an odd denormal is a rounding midpoint).  With the same tree the
// probabilities of qmann_answer_i8's two-kernel form are qmann_answer_f32_serial's bit for bit at every magnitude.
template <bool PRECOMPUTED, bool TOPK = false>
__global__ void __launch_bounds__(kBlock)
k_answer(const float *__restrict__ w_ans, const float *__restrict__ u, const uint32_t *__restrict__ answer,
         uint32_t *__restrict__ pred, float *__restrict__ probs, float *cost, uint32_t *match, uint32_t D,
         uint32_t V, uint32_t softmax_base, uint32_t n_query, uint32_t small_lpq, uint32_t small_vpt, const AnsTopK<TOPK> tk)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *us = (float *)smem;            // [D]
    float *lg = us + ((D + 3) & ~3u);     // [V]
    __shared__ double red_d[kWaves];
    __shared__ float red_f[kWaves];
    __shared__ uint32_t red_i[kWaves];
    const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    float cost_acc = 0.0f;              // thread 0 only; added once per workgroup (see k_answer_small)
    uint32_t match_acc = 0;
    for (uint32_t q = blockIdx.x; q < n_query; q += gridDim.x) {
    __syncthreads();                    // the previous query's LDS rows are free again
    if (!PRECOMPUTED) {
        for (uint32_t c = tid; c < D; c += kBlock) us[c] = u[(size_t)q * D + c];
        __syncthreads();
    }

    float mx = -INFINITY;
    for (uint32_t v = tid; v < V; v += kBlock) {
        float sum = 0.0f;
        if (PRECOMPUTED) {
            sum = w_ans[(size_t)q * V + v];          // w_ans aliases the logits buffer [n_query][V]
        } else {
            const float *wr = w_ans + (size_t)v * D;
#pragma unroll 8
            for (uint32_t c = 0; c < D; c++) {       // unrolled: loads of a row run ahead of the serial adds
                const float t = wr[c] * us[c];
                sum += t;
            }
        }
        lg[v] = sum;
        mx = sum > mx ? sum : mx;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float t = __shfl_xor(mx, o);
        mx = t > mx ? t : mx;
    }
    if (lane == 0) red_f[wave] = mx;
    __syncthreads();
    mx = red_f[0];
    for (int i = 1; i < kWaves; i++) mx = red_f[i] > mx ? red_f[i] : mx;

    double part = 0.0;
    for (uint32_t v = tid; v < V; v += kBlock) {
        const float e = sm_exp(lg[v] - mx, SmCfg{softmax_base, false, false, 1.0f});    // sf_out is never shift-based
        lg[v] = e;
        part += (double)e;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
    if (lane == 0) red_d[wave] = part;
    __syncthreads();
    double total = (red_d[0] + red_d[1]) + (red_d[2] + red_d[3]);
    if (PRECOMPUTED && small_lpq) {                  // (uniform) every wavefront forms k_answer_small's tree from the terms in LDS
        const uint32_t sub = lane % small_lpq;       // 16 lanes per query there: the four rows of this wavefront do the same work
        double t = 0.0;
        for (uint32_t k = 0; k < small_vpt; k++) {
            const uint32_t v = sub * small_vpt + k;
            t += v < V ? (double)lg[v] : 0.0;        // (a lane's logits past V are zero terms there too)
        }
        t += __shfl(t, (int)(lane ^ 1u));                                // quad_perm [1,0,3,2]
        t += __shfl(t, (int)(lane ^ 2u));                                // quad_perm [2,3,0,1]
        t += __shfl(t, (int)((lane & ~7u) | (7u - (lane & 7u))));        // row_half_mirror
        t += __shfl(t, (int)((lane & ~15u) | (15u - (lane & 15u))));     // row_mirror
        for (uint32_t o = 16; o < small_lpq; o <<= 1) t += __shfl_xor(t, (int)o);
        total = t;                                   // (every lane holds it)
        __syncthreads();                             // all wavefronts have read the terms before the quotients replace them
    }

    constexpr bool BY_LOGIT = PRECOMPUTED && TOPK;
    float bv = -INFINITY;
    uint32_t bi = 0;
    for (uint32_t v = tid; v < V; v += kBlock) {
        const float p = (softmax_base == QMANN_SOFTMAX_EXP) ? (float)((double)lg[v] / total)
                                                            : lg[v] / (float)total;
        lg[v] = p;
        if (!TOPK && probs) probs[(size_t)q * V + v] = p;
        if constexpr (BY_LOGIT) {
            const float x = w_ans[(size_t)q * V + v];
            if (!(bv > x)) { bv = x; bi = v; }
        } else {
            if (!(bv > p)) { bv = p; bi = v; }       // later index wins a tie
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float tv = __shfl_xor(bv, o);
        const uint32_t ti = __shfl_xor(bi, o);
        if (tv > bv || (tv == bv && ti > bi)) { bv = tv; bi = ti; }
    }
    __syncthreads();
    if (lane == 0) { red_f[wave] = bv; red_i[wave] = bi; }
    __syncthreads();
    if (tid == 0) {
        for (int i = 1; i < kWaves; i++)
            if (red_f[i] > bv || (red_f[i] == bv && red_i[i] > bi)) { bv = red_f[i]; bi = red_i[i]; }
        if constexpr (TOPK) {
            tk.idx[(size_t)q * tk.k] = bi;
            tk.p[(size_t)q * tk.k] = BY_LOGIT ? lg[bi] : bv;
            lg[bi] = -1.0f;
        } else {
            pred[q] = bi;
        }
        if (!TOPK && answer) {
            const uint32_t y = answer[q];
            if (y < V) {
                cost_acc += -lg[y];
                match_acc += (y == bi) ? 1u : 0u;
            }
        }
    }
    if constexpr (TOPK) {
        for (uint32_t j = 1; j < tk.k; j++) {
            __syncthreads();                // the last round's entry is marked, its red_f / red_i are read
            bv = -INFINITY;
            bi = 0;
            for (uint32_t v = tid; v < V; v += kBlock) {
                const float p = lg[v];
                if constexpr (BY_LOGIT) {
                    const float x = w_ans[(size_t)q * V + v];
                    if (p >= 0.0f && !(bv > x)) { bv = x; bi = v; }      // (k <= V: an untaken logit, all finite, is always left)
                } else {
                    if (!(bv > p)) { bv = p; bi = v; }
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float tv = __shfl_xor(bv, o);
                const uint32_t ti = __shfl_xor(bi, o);
                if (tv > bv || (tv == bv && ti > bi)) { bv = tv; bi = ti; }
            }
            if (lane == 0) { red_f[wave] = bv; red_i[wave] = bi; }
            __syncthreads();
            if (tid == 0) {
                for (int i = 1; i < kWaves; i++)
                    if (red_f[i] > bv || (red_f[i] == bv && red_i[i] > bi)) { bv = red_f[i]; bi = red_i[i]; }
                tk.idx[(size_t)q * tk.k + j] = bi;
                tk.p[(size_t)q * tk.k + j] = BY_LOGIT ? lg[bi] : bv;
                lg[bi] = -1.0f;
            }
        }
    }
    }
    if (!TOPK && tid == 0 && answer) {
        if (cost) atomicAdd(cost, cost_acc);
        if (match && match_acc) atomicAdd(match, match_acc);
    }
}

// Answer layer for small dictionaries (V <= 256: bAbI single-task and joint sizes): SIXTEEN LANES per query, four
// queries per wavefront; lane s of a group owns the VPT adjacent logits VPT.s .. VPT.s + VPT - 1 (16 . VPT >= V).  The
// arithmetic is k_answer's (serial float sum over the embedding axis per logit, softmax with a double normaliser,
// arg-max with ties to the highest index) without block barriers.  W is staged transposed in LDS once per (persistent)
// workgroup; per embedding column a lane reads its VPT weights and its query's component from LDS and the products /
// sums go through the packed fp32 pipeline.  The kernel is bound by vector-instruction issue: with one query per
// wavefront (round 1) the reductions and the per-logit divisions cost ~450 instructions per query whatever V was; a
// 16-lane group is one DPP row, so every reduction is four DPP steps serving four queries.
// 16 wavefronts per workgroup share one copy of W^T (up to 61 KB): 2 workgroups fill a CU's 32 wavefront slots
constexpr int kAnsBlock = 1024, kAnsWaves = kAnsBlock / kWave;

// butterfly over the 16 lanes of a DPP row: after the four steps every lane holds the row's result
// (quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror)
#define QM_ROW_STEPS(X) X(0xB1) X(0x4E) X(0x141) X(0x140)
// one step of the (value, index) arg-max on bv / bi
#define QM_ROW_ARGMAX_STEP(C) { const float tv = row_peer_f32<C>(bv); const uint32_t ti = row_peer_u32<C>(bi); \
                                if (tv > bv || (tv == bv && ti > bi)) { bv = tv; bi = ti; } }   /* ties go to the highest index */
template <int CTRL> __device__ __forceinline__ float row_peer_f32(float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
template <int CTRL> __device__ __forceinline__ uint32_t row_peer_u32(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, true);
}
template <int CTRL> __device__ __forceinline__ double row_peer_f64(double v)
{
    const uint64_t b = __builtin_bit_cast(uint64_t, v);
    const uint32_t lo = row_peer_u32<CTRL>((uint32_t)b), hi = row_peer_u32<CTRL>((uint32_t)(b >> 32));
    return __builtin_bit_cast(double, (uint64_t)lo | ((uint64_t)hi << 32));
}

// (value, index) arg-max over a query's LPQ lanes, ties to the highest index; every lane ends with the result (the ranked builds'
// further rounds: the steps k_answer_small spells out for its first)
template <int LPQ> __device__ __forceinline__ void row_argmax(float &bv, uint32_t &bi)
{
    QM_ROW_STEPS(QM_ROW_ARGMAX_STEP)
#pragma unroll
    for (int o = 16; o < LPQ; o <<= 1) {
        const float tv = __shfl_xor(bv, o);
        const uint32_t ti = __shfl_xor(bi, o);
        if (tv > bv || (tv == bv && ti > bi)) { bv = tv; bi = ti; }
    }
}

// TOPK: as in k_answer -- the rounds run on the lane's probabilities in registers, every lane of the group knows each winner
template <int LPQ, int VPT, int QB, bool TOPK = false>
__global__ void __launch_bounds__(kAnsBlock, 8)             // 64 registers: two workgroups per CU
k_answer_small(const float *__restrict__ w_ans, const float *__restrict__ u, const uint32_t *__restrict__ answer,
               uint32_t *__restrict__ pred, float *__restrict__ probs, float *cost, uint32_t *match, uint32_t D,
               uint32_t V, uint32_t softmax_base, uint32_t n_query, const AnsTopK<TOPK> tk)
{
    static_assert(VPT % 2 == 0, "logits are handled in pairs");
    typedef float f2 __attribute__((ext_vector_type(2)));
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    static_assert(LPQ == 16 || LPQ == 32 || LPQ == 64, "a query's lanes are whole DPP rows");
    constexpr uint32_t VP = LPQ * VPT;                  // logits padded to a whole group (zero columns)
    constexpr uint32_t QPW = (kWave / LPQ) * QB;        // queries per wavefront: QB per lane group, sharing each weight read
    typedef float fq __attribute__((ext_vector_type(QB)));
    float *wt = (float *)smem;                          // [D][VP]: W transposed
    const uint32_t wave_u = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));      // uniform: query bookkeeping in SGPRs (no spill at 64 registers)
    float *us = wt + (size_t)D * VP + wave_u * QPW * D;   // [kAnsWaves][D][QPW]: this wavefront's queries, interleaved
    const uint32_t lane = threadIdx.x & (kWave - 1), grp = lane / LPQ, sub = lane % LPQ;
    const size_t stride = (size_t)gridDim.x * kAnsWaves * QPW;
    for (uint32_t i = threadIdx.x; i < D * VP; i += kAnsBlock) {
        const uint32_t c = i / VP, v = i % VP;
        wt[i] = v < V ? w_ans[(size_t)v * D + c] : 0.0f;
    }
    __syncthreads();
    const SmCfg smc{softmax_base, false, false, 1.0f};  // sf_out is never shift-based (MemN2N.c:910)
    const uint32_t v0 = sub * VPT;                      // first logit of this lane
    bool live[VPT];
#pragma unroll
    for (int k = 0; k < VPT; k++) live[k] = v0 + k < V;
    // cost / match are summed per wavefront and added once: one device-scope atomic per query on a
    // single word would serialise the whole batch (~12 ns each)
    float cost_acc = 0.0f;
    uint32_t match_acc = 0;
    for (size_t qb = ((size_t)blockIdx.x * kAnsWaves + wave_u) * QPW; qb < n_query; qb += stride) {
        const uint32_t nq = n_query - qb < QPW ? (uint32_t)(n_query - qb) : QPW;
        for (uint32_t i = lane; i < nq * D; i += kWave) us[(i % D) * QPW + i / D] = u[qb * D + i];   // consecutive queries: one contiguous block
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        f2 acc[QB][VPT / 2];
#pragma unroll
        for (int j = 0; j < QB; j++)
#pragma unroll
            for (int k = 0; k < VPT / 2; k++) acc[j][k] = f2{0.0f, 0.0f};
        const float *uq = us + grp * QB;
        const float *wl = wt + v0;
#pragma unroll 2
        for (uint32_t c = 0; c < D; c++) {               // serial over the embedding axis, as the reference sums
            const fq uc = *(const fq *)(uq + c * QPW);
#pragma unroll
            for (int k = 0; k < VPT / 2; k++) {
                const f2 w = *(const f2 *)(wl + c * VP + 2 * k);
#pragma unroll
                for (int j = 0; j < QB; j++) {
                    const f2 t = w * uc[j];
                    acc[j][k] += t;
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // reads of us[] done before the next queries overwrite it
#pragma unroll
        for (int j = 0; j < QB; j++) {
            const bool q_ok = grp * QB + j < nq;         // (a missing query's lanes compute on stale LDS and store nothing)
            const size_t q = qb + grp * QB + j;
            float sum[VPT];
#pragma unroll
            for (int k = 0; k < VPT; k++) sum[k] = acc[j][k / 2][k % 2];
            float mx = -INFINITY;
#pragma unroll
            for (int k = 0; k < VPT; k++) mx = (live[k] && sum[k] > mx) ? sum[k] : mx;
#define QM_STEP(C) { const float t = row_peer_f32<C>(mx); mx = t > mx ? t : mx; }
            QM_ROW_STEPS(QM_STEP)
#undef QM_STEP
#pragma unroll
            for (int o = 16; o < LPQ; o <<= 1) { const float t = __shfl_xor(mx, o); mx = t > mx ? t : mx; }
            float e[VPT];
            double total = 0.0;
#pragma unroll
            for (int k = 0; k < VPT; k++) {
                e[k] = live[k] ? sm_exp(sum[k] - mx, smc) : 0.0f;
                total += (double)e[k];
            }
#define QM_STEP(C) total += row_peer_f64<C>(total);
            QM_ROW_STEPS(QM_STEP)
#undef QM_STEP
#pragma unroll
            for (int o = 16; o < LPQ; o <<= 1) total += __shfl_xor(total, o);
            float bv = -INFINITY;
            uint32_t bi = 0;
            float p[VPT];
#pragma unroll
            for (int k = 0; k < VPT; k++) {
                p[k] = (softmax_base == QMANN_SOFTMAX_EXP) ? (float)((double)e[k] / total) : e[k] / (float)total;
                if (live[k]) {
                    if (!TOPK && probs && q_ok) probs[q * V + v0 + k] = p[k];
                    if (!(bv > p[k])) { bv = p[k]; bi = v0 + k; }               // later index wins a tie
                }
            }
            QM_ROW_STEPS(QM_ROW_ARGMAX_STEP)
#pragma unroll
            for (int o = 16; o < LPQ; o <<= 1) {
                const float tv = __shfl_xor(bv, o);
                const uint32_t ti = __shfl_xor(bi, o);
                if (tv > bv || (tv == bv && ti > bi)) { bv = tv; bi = ti; }
            }
            if constexpr (TOPK) {
                for (uint32_t r = 0;;) {
                    if (sub == 0 && q_ok) { tk.idx[q * tk.k + r] = bi; tk.p[q * tk.k + r] = bv; }
                    if (++r == tk.k) break;
                    const uint32_t taken = bi;
                    bv = -INFINITY;
                    bi = 0;
#pragma unroll
                    for (int k = 0; k < VPT; k++) {
                        p[k] = (v0 + k == taken) ? -1.0f : p[k];
                        if (live[k] && !(bv > p[k])) { bv = p[k]; bi = v0 + k; }
                    }
                    row_argmax<LPQ>(bv, bi);
                }
            } else {
                if (sub == 0 && q_ok) pred[q] = bi;
            }
            if (!TOPK && answer) {
                const uint32_t y = q_ok ? answer[q] : 0xFFFFFFFFu;
                const uint32_t ys = y < V ? y : 0u;
                float psel = p[0];
#pragma unroll
                for (int k = 1; k < VPT; k++) psel = (ys % VPT == (uint32_t)k) ? p[k] : psel;
                const float py = __shfl(psel, (int)(grp * LPQ + ys / VPT));
                if (sub == 0 && y < V) {
                    cost_acc += -py;
                    match_acc += (y == bi) ? 1u : 0u;
                }
            }
        }
    }
    if (!TOPK && answer) {
#pragma unroll
        for (int o = LPQ; o < kWave; o <<= 1) { cost_acc += __shfl_xor(cost_acc, o); match_acc += __shfl_xor(match_acc, o); }
        if (lane == 0) {
            if (cost) atomicAdd(cost, cost_acc);
            if (match && match_acc) atomicAdd(match, match_acc);
        }
    }
}
#undef QM_ROW_ARGMAX_STEP
#undef QM_ROW_STEPS

// ---- host side --------------------------------------------------------------------------------------------------------------
// the bookkeeping outputs of an answer call, in the kernels' order (all null in a ranked call, whose outputs are AnsTopK<true>'s)
struct AnsOut { const uint32_t *answer; uint32_t *pred; float *probs, *cost; uint32_t *match; };
// k_answer's dynamic LDS for a query -- us [D rounded up to 4], lg [V], floats -- and the most an answer call accepts: every
// entry point of the layer answers QMANN_ERANGE beyond it, whichever kernel it would take
constexpr size_t kAnsSerialLdsLimit = 128 * 1024;
static inline size_t ans_serial_lds(uint32_t D, uint32_t V) { return ((size_t)((D + 3) & ~3u) + V) * sizeof(float); }
// k_answer's grid: a workgroup per query, the rest of a large batch in its loop
static inline uint32_t ans_serial_grid(uint32_t n_query) { return n_query < 8192u ? n_query : 8192u; }

// the k_answer_small build of a shape, and whether the float layer takes it (otherwise: k_answer, one workgroup per query)
struct AnsSmallPlan {
    uint32_t lpq, vpt, qpw;     // lanes per query, logits per lane, queries per wavefront
    size_t lds;
    bool fits;
};
static inline AnsSmallPlan ans_small_plan(uint32_t D, uint32_t V)
{
    AnsSmallPlan p;
    p.lpq = V <= 128 ? 16u : 64u;
    const uint32_t qb = V <= 96 ? 2u : (V <= 128 ? 1u : 4u);
    const uint32_t vpt = (V + p.lpq - 1) / p.lpq;
    // (the one 64-lane build is <64, 4, 4>: where it fits, V is 129 .. 256, three or four logits per lane, and the rounding gives 4)
    p.vpt = vpt <= 2 ? 2u : vpt <= 4 ? 4u : vpt <= 6 ? 6u : 8u;
    p.qpw = kWave / p.lpq * qb;
    p.lds = ((size_t)D * p.lpq * p.vpt + (size_t)kAnsWaves * p.qpw * D) * sizeof(float);
    p.fits = V <= 256u && p.lds <= 78 * 1024;
    return p;
}

}  // namespace
