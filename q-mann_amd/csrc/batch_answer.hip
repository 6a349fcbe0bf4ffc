// batch_answer.hip -- the stage after the hop loop, batched over queries: the answer layer
// (projection, softmax, arg-max, test-phase bookkeeping).
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
// PRECOMPUTED: logits come from a buffer (written by the MFMA projection below) instead of being
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
#define QM_STEP(C) { const float tv = row_peer_f32<C>(bv); const uint32_t ti = row_peer_u32<C>(bi); \
                     if (tv > bv || (tv == bv && ti > bi)) { bv = tv; bi = ti; } }   /* ties go to the highest index */
    QM_ROW_STEPS(QM_STEP)
#undef QM_STEP
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
#define QM_STEP(C) { const float tv = row_peer_f32<C>(bv); const uint32_t ti = row_peer_u32<C>(bi); \
                     if (tv > bv || (tv == bv && ti > bi)) { bv = tv; bi = ti; } }   /* ties go to the highest index */
            QM_ROW_STEPS(QM_STEP)
#undef QM_STEP
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
#undef QM_ROW_STEPS

// ---------------------------------------------------------------------------
// The FLOAT answer layer on the bf16 matrix cores (bAbI widths: 64-byte rows, dictionaries up to 256), within north_star's 1e-5
// on the float softmax instead of bit-equal to the reference's serial sum.  The kernels above reproduce
// lib/layer_cuda.cu:70-80's order of additions exactly and pay for it: 545 vector instructions per query at the joint
// dictionary (profiles/r05_units_j20_k_answer_small.txt), a fifth of that forward.  Here:
//   * u, the last hop's output, lies on an 8-bit grid (|code| <= 127): every component is exactly a bf16;
//   * W (arbitrary float32) is split once per workgroup into three bf16 images W1 + W2 + W3 = W exactly (each takes the top 8
//     significant bits of what the one before left), 144-byte rows in LDS (16 B of padding: fragment reads without bank conflicts);
//   * logits = u . W3 + u . W2 + u . W1 on v_mfma_f32_16x16x32_bf16, rows = 16 answers, columns = 16 queries: every product is
//     exact (15 significant bits), only the float accumulation rounds -- the result sits closer to the exact sum than the serial
//     float loop does; against that loop: a few units in the last place of the logit (measured: probabilities within 5e-6
//     relative at the tests' and the bench's magnitudes, tools/answer_fused_error.py);
//   * a lane ends with its query's logits of answers 16t + 4(lane >> 4) + r in registers: maximum, 2^((l - max) log2 e) through
//     v_exp_f32, float total, arg-max on the LOGITS (equal logits <=> equal probabilities; ties to the highest index as
//     lib/layer_cuda.cu:1918-1939) and the label's probability never leave them; two cross-lane steps join the four lane groups.
// 36 vector instructions per query instead of 545 at V = 238.  QMANN_ANSWER_EXACT (or the drop-in queue, which promises the
// serial loop's results) keeps the serial-order kernels.
// ---------------------------------------------------------------------------
typedef short bf16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));
constexpr int kAmWaves = 16, kAmBlock = kAmWaves * kWave;
constexpr uint32_t kAmPitch = 144;                  // bytes per row of a W image: 64 bf16 + 16 B (rows 16 B apart modulo 256)

template <int T>                                     // tiles of 16 answers: V <= 16 T
__global__ void __launch_bounds__(kAmBlock, 4)
k_answer_mfma(const float *__restrict__ w_ans, const float *__restrict__ u, const uint32_t *__restrict__ answer,
              uint32_t *__restrict__ pred, float *__restrict__ probs, float *cost, uint32_t *match, uint32_t D, uint32_t V,
              uint32_t softmax_base, uint32_t n_query)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr uint32_t kImg = T * 16u * kAmPitch;        // one bf16 image of W
    const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1);
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid / kWave));
    for (uint32_t i = tid; i < T * 16u * 64u; i += kAmBlock) {
        const uint32_t v = i >> 6, c = i & 63u;
        const float w = (v < V && c < D) ? w_ans[(size_t)v * D + c] : 0.0f;
        const uint32_t b1 = __builtin_bit_cast(uint32_t, w) & 0xFFFF0000u;
        const float r1 = w - __builtin_bit_cast(float, b1);                 // exact
        const uint32_t b2 = __builtin_bit_cast(uint32_t, r1) & 0xFFFF0000u;
        const float r2 = r1 - __builtin_bit_cast(float, b2);                // exact; at most 8 significant bits are left
        const uint32_t b3 = __builtin_bit_cast(uint32_t, r2) & 0xFFFF0000u;
        uint8_t *dst = smem + v * kAmPitch + c * 2u;
        *(uint16_t *)dst = (uint16_t)(b1 >> 16);
        *(uint16_t *)(dst + kImg) = (uint16_t)(b2 >> 16);
        *(uint16_t *)(dst + 2u * kImg) = (uint16_t)(b3 >> 16);
    }
    __syncthreads();
    const uint32_t qi = lane & 15u, grp = lane >> 4;
    const bool vec4 = (D & 3u) == 0u;
    const uint8_t *arow = smem + qi * kAmPitch + grp * 16u;          // this lane's piece of an answer row: k = 8 grp .. + 7 of a K step
    float cost_acc = 0.0f;
    uint32_t match_acc = 0;
    const uint32_t n_task = (n_query + 15u) / 16u;
    for (uint32_t task = blockIdx.x * kAmWaves + wave; task < n_task; task += gridDim.x * kAmWaves) {
        asm volatile("" ::: "memory");                                   // (the W fragments are read per task: hoisted out of this loop they would take 24 T registers)
        const uint32_t q = task * 16u + qi;
        const bool q_ok = q < n_query;
        // B fragments: u[q][32 ks + 8 grp + j], j = 0 .. 7, as bf16 (exact: u lies on an 8-bit grid)
        bf16x8_t bf[2];
#pragma unroll
        for (int ks = 0; ks < 2; ks++) {
            const uint32_t k0 = 32u * ks + 8u * grp;
            uint32_t w[8];
            if (vec4) {
                const float *src = u + (size_t)q * D + k0;
                // (plain ifs: `cond ? *(const f32x4_t *)p : zero` compiles to ONE dword load splatted over the vector with hipcc 7.2)
                float4 lo = {0.0f, 0.0f, 0.0f, 0.0f}, hi = {0.0f, 0.0f, 0.0f, 0.0f};
                if (q_ok && k0 + 3u < D) lo = *(const float4 *)src;
                if (q_ok && k0 + 7u < D) hi = *(const float4 *)(src + 4);
#pragma unroll
                for (int j = 0; j < 4; j++) { w[j] = __builtin_bit_cast(uint32_t, (&lo.x)[j]); w[4 + j] = __builtin_bit_cast(uint32_t, (&hi.x)[j]); }
            } else {
#pragma unroll
                for (int j = 0; j < 8; j++) w[j] = (q_ok && k0 + j < D) ? __builtin_bit_cast(uint32_t, u[(size_t)q * D + k0 + j]) : 0u;
            }
            i32x4 pk;
#pragma unroll
            for (int j = 0; j < 4; j++) pk[j] = (int)__builtin_amdgcn_perm(w[2 * j + 1], w[2 * j], 0x07060302u);    // the two high halves
            bf[ks] = __builtin_bit_cast(bf16x8_t, pk);
        }
        f32x4_t acc[T];
#pragma unroll
        for (int t = 0; t < T; t++) {
            acc[t] = f32x4_t{0, 0, 0, 0};
#pragma unroll
            for (int s_ = 2; s_ >= 0; s_--)                              // the smallest terms first
#pragma unroll
                for (int ks = 0; ks < 2; ks++) {
                    const bf16x8_t af = *(const bf16x8_t *)(arow + s_ * kImg + t * 16u * kAmPitch + ks * 64u);
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bf[ks], acc[t], 0, 0, 0);
                }
        }
        // ---- softmax statistics of this lane's T x 4 logits (answer 16 t + 4 grp + r), then across the four lane groups ----
        float mx = -INFINITY;
#pragma unroll
        for (int t = 0; t < T; t++) {
            if ((uint32_t)t * 16u + 16u > V) {                           // (wavefront-uniform) the dictionary ends inside this tile
#pragma unroll
                for (int r = 0; r < 4; r++) acc[t][r] = ((uint32_t)t * 16u + grp * 4u + r < V) ? acc[t][r] : -INFINITY;
            }
#pragma unroll
            for (int r = 0; r < 4; r++) mx = fmaxf(mx, acc[t][r]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        // arg-max on the logits: the highest position of this lane that holds the maximum (positions ascend with the answer index)
        int bpos = -1;
#pragma unroll
        for (int t = 0; t < T; t++) {
#pragma unroll
            for (int r = 0; r < 4; r++) bpos = acc[t][r] == mx ? 4 * t + r : bpos;
            __builtin_amdgcn_sched_barrier(0);                           // (a tile's compares next to its selects: all 4 T lane masks at once do not fit the scalar file)
        }
        uint32_t bi = bpos >= 0 ? (uint32_t)(bpos >> 2) * 16u + grp * 4u + (uint32_t)(bpos & 3) : 0u;
        { const uint32_t o = (uint32_t)__shfl_xor((int)bi, 16); const int ob = __shfl_xor(bpos, 16); if (ob >= 0 && (bpos < 0 || o > bi)) { bi = o; bpos = ob; } }
        { const uint32_t o = (uint32_t)__shfl_xor((int)bi, 32); const int ob = __shfl_xor(bpos, 32); if (ob >= 0 && (bpos < 0 || o > bi)) { bi = o; bpos = ob; } }
        // the label's logit, if this lane holds it (a binary tree of selects over the lane's positions)
        const uint32_t y = (answer && q_ok) ? answer[q] : 0xFFFFFFFFu;
        float ly = -INFINITY;
        if (answer) {                                                    // (wavefront-uniform)
            const bool mine = y < V && ((y >> 2) & 3u) == grp;
            const uint32_t ty = y >> 4, ry = y & 3u;
            f32x4_t sel = acc[0];
#pragma unroll
            for (int t = 1; t < T; t++) {
                const bool pick = ty == (uint32_t)t;
#pragma unroll
                for (int r = 0; r < 4; r++) sel[r] = pick ? acc[t][r] : sel[r];
                __builtin_amdgcn_sched_barrier(0);
            }
            float l1 = (ry & 1u) ? sel[1] : sel[0], l2 = (ry & 1u) ? sel[3] : sel[2];
            ly = mine ? ((ry & 2u) ? l2 : l1) : -INFINITY;
            ly = fmaxf(ly, __shfl_xor(ly, 16));
            ly = fmaxf(ly, __shfl_xor(ly, 32));
        }
        // e = base^(l - max); the 2^x base needs no scaling (lib/layer.c:1225), e^x goes through 2^(x log2 e)
        const float sc = softmax_base == QMANN_SOFTMAX_EXP ? 1.44269504088896341f : 1.0f;
        float tot = 0.0f;
#pragma unroll
        for (int t = 0; t < T; t++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                acc[t][r] = __builtin_amdgcn_exp2f((acc[t][r] - mx) * sc);
                tot += acc[t][r];
            }
        tot += __shfl_xor(tot, 16);
        tot += __shfl_xor(tot, 32);
        const float inv = __builtin_amdgcn_rcpf(tot);
        if (probs && q_ok) {
#pragma unroll
            for (int t = 0; t < T; t++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const uint32_t v = (uint32_t)t * 16u + grp * 4u + r;
                    if (v < V) probs[(size_t)q * V + v] = acc[t][r] * inv;
                }
        }
        if (grp == 0 && q_ok) {
            pred[q] = bi;
            if (y < V) {
                cost_acc += -(__builtin_amdgcn_exp2f((ly - mx) * sc) * inv);
                match_acc += (y == bi) ? 1u : 0u;
            }
        }
    }
    if (answer) {
        // cost / match: summed per workgroup, one atomic each
        __shared__ float red_c[kAmWaves];
        __shared__ uint32_t red_m[kAmWaves];
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) { cost_acc += __shfl_xor(cost_acc, o); match_acc += __shfl_xor(match_acc, o); }   // lanes 0 .. 15 hold the figures
        if (lane == 0) { red_c[wave] = cost_acc; red_m[wave] = match_acc; }
        __syncthreads();
        if (tid == 0) {
            float c = 0.0f; uint32_t m = 0;
            for (int i = 0; i < kAmWaves; i++) { c += red_c[i]; m += red_m[i]; }
            if (cost) atomicAdd(cost, c);
            if (match && m) atomicAdd(match, m);
        }
    }
}

// ---------------------------------------------------------------------------
// Answer projection on the matrix cores, for an answer matrix that lives on an int8 grid:
// logits[q][v] = sum_c U[q][c] . W[v][c] with both operands small integers (codes), so the
// reference's float serial sum (lib/layer_cuda.cu:70-80) is an exact integer times
// 2^-(frac_u + frac_w) (|sum| <= 256.127.127 < 2^24) and an int32 MFMA accumulation reproduces it
// bit for bit.  One wavefront owns a 16 x 16 tile (16 queries x 16 answers) and issues
// v_mfma_i32_16x16x64_i8 over the embedding axis; both fragments are plain 16-byte row segments
// (lane l: row l & 15, bytes 16.(l >> 4) .. +15 of the 64-deep K step), so they are loaded straight
// from global memory -- the query side is converted from the hop kernel's float-on-grid vector in
// registers once and stays resident while the wavefront walks the answer tiles.
// C/D: lane l holds column l & 15, rows 4.(l >> 4) + r.
// ---------------------------------------------------------------------------
typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int kTilesPerBlockY = 16;      // answer tiles (of 16) one wavefront walks with its query fragment resident

template <int KSTEPS>
__global__ void __launch_bounds__(kBlock)
k_logits_mfma_i8(const float *__restrict__ u, const int8_t *__restrict__ w, float *__restrict__ logits,
                 uint32_t n_query, uint32_t D, uint32_t V, QFmt fu, float scale)
{
    constexpr uint32_t Dp = KSTEPS * 64;
    const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const uint32_t m0 = (blockIdx.x * kWaves + wave) * 16;       // this wavefront's 16 queries
    if (m0 >= n_query) return;                                   // whole wavefront
    const uint32_t row = lane & 15, kq = lane >> 4;
    const uint32_t qrow = m0 + row;
    // A fragments (query codes) for every K step, converted once
    i32x4 a[KSTEPS];
#pragma unroll
    for (int ks = 0; ks < KSTEPS; ks++) {
        const uint32_t kb = ks * 64 + 16 * kq;
#pragma unroll
        for (int d = 0; d < 4; d++) {
            uint32_t pk = 0;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const uint32_t c = kb + 4 * d + i;
                const int code = (qrow < n_query && c < D) ? qm_code(u[(size_t)qrow * D + c], fu.iwl, fu.frac) : 0;
                pk |= ((uint32_t)code & 0xFFu) << (8 * i);
            }
            a[ks][d] = (int)pk;
        }
    }
    const uint32_t t0 = blockIdx.y * kTilesPerBlockY;
    for (uint32_t t = t0; t < t0 + kTilesPerBlockY && t * 16 < V; t++) {
        const uint32_t n0 = t * 16;
        const uint32_t vrow = n0 + row;
        i32x4 acc = {0, 0, 0, 0};
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ks++) {
            i32x4 b = {0, 0, 0, 0};
            if (vrow < V) b = *(const i32x4 *)(w + (size_t)vrow * Dp + ks * 64 + 16 * kq);
            acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[ks], b, acc, 0, 0, 0);
        }
        const uint32_t col = n0 + (lane & 15);
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const uint32_t qr = m0 + 4 * (lane >> 4) + r;
            if (qr < n_query && col < V) logits[(size_t)qr * V + col] = (float)acc[r] * scale;
        }
    }
}

// ---------------------------------------------------------------------------
// The int8 answer layer in one pass, without the [n_query][V] logits round trip: projection on the matrix cores, softmax
// statistics and arg-max in the accumulator registers.  What makes a one-pass form exact enough:
//   * logits are integers k times 2^-(frac_u + frac_w), so the arg-max of the rounded probabilities, ties to the highest
//     index (lib/layer_cuda.cu:1918-1939), is the highest index whose k equals the maximum: two different k cannot round
//     to the same probability (their ratio is at least e^(2^-14));
//   * the normaliser sum_v e^(l_v - max) is accumulated against the RUNNING maximum and rescaled when the maximum moves
//     (relative error ~1e-7, inside the 1e-5 softmax tolerance); it only enters the cost -p[answer], an atomically
//     accumulated float anyway.  A caller that wants the probabilities themselves takes the two-kernel path.
// A workgroup of 4 wavefronts owns 64 queries (their code fragments stay in registers) and a slice of the dictionary; the
// slice's W rows pass through a double-buffered LDS tile shared by the 4 wavefronts (64 rows, pitch Dp + 16).  Slices keep
// every CU busy at 8 192 queries; a second, tiny kernel merges the per-slice records.
// ---------------------------------------------------------------------------
struct AnsPart {            // per (slice, query)
    int m;                  // maximum logit code of the slice
    uint32_t idx;           // its highest index
    double sum;             // sum over the slice of e^((k - m) . scale)
};
constexpr uint32_t kAnsTile = 64;                       // dictionary rows per LDS tile = 4 accumulator blocks of 16
constexpr int kAnsFloor = -(1 << 28);                   // below every logit code (|sum of 256 products of 7-bit codes| < 2^23); e^(floor . scale) = 0

// e^((k - m) . scale) for a code difference dk <= 0.  Base e^x: the hardware exponential with scale . log2 e folded into one
// factor (v_cvt, v_mul, v_exp; ~2 ulp -- the reference's own kernel uses the fast __expf there, lib/layer_cuda.cu:2006);
// the other bases through the shared definitions.
template <bool EXPB>
__device__ __forceinline__ float ans_term(int dk, float scale, float scale_log2e, const SmCfg &c)
{
    if (EXPB) return __builtin_amdgcn_exp2f((float)dk * scale_log2e);
    return sm_exp((float)dk * scale, c);
}

// ---- ranked builds (qmann_answer_topk_i8) ------------------------------------------------------------------------------------------
// A candidate is the 64-bit key ((code + 2^28) << 32) | index: "larger key first" is the whole order -- larger code first, equal
// codes: higher index first -- and 0 is below every candidate (no code is as low as kAnsFloor).
// The 16 lanes that share a group of 4 query rows (equal lane >> 4: one DPP row) hold each row's sorted list DISTRIBUTED: lane c
// holds entry c, 4 keys = 8 registers per lane at any k <= 16.  Entries beyond k - 1 are kept too (they cost nothing), the bar
// a candidate must pass is entry k - 1.
__device__ __forceinline__ uint64_t ans_key(int code, uint32_t v)
{
    return ((uint64_t)(uint32_t)(code - kAnsFloor) << 32) | v;
}
// the left neighbour's entry within the DPP row (row_shr:1); lane 0 of a row reads "above everything"
__device__ __forceinline__ uint64_t ans_left_entry(uint64_t e)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)(uint32_t)e, 0x111, 0xF, 0xF, false);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)(uint32_t)(e >> 32), 0x111, 0xF, 0xF, false);
    return (uint64_t)lo | ((uint64_t)hi << 32);
}
// Every lane brings N candidates `key` for the list `e` of its lane group (0: none).  Those above the group's k-th entry are
// inserted one at a time: a lane offers its best one, a lane is picked from the group's 16 ballot bits, its key broadcast within
// the group, and every lane shifts or keeps its entry.  The four lane groups insert in parallel; the trip count is wavefront-
// uniform (the ballot): one trip per insertion of the busiest group, and one shuffle for the bar that each insertion raises.
template <int N>
__device__ __forceinline__ void ans_list_insert(uint64_t &e, uint64_t (&key)[N], uint32_t lane, uint32_t k)
{
    const uint32_t base = lane & 48u;
    uint64_t bar = __shfl(e, (int)(base + k - 1));
    for (;;) {
        uint64_t m = key[0];
#pragma unroll
        for (int i = 1; i < N; i++) m = key[i] > m ? key[i] : m;
        const uint64_t bal = __ballot(m > bar);
        if (bal == 0) break;                                         // (wavefront-uniform)
        const uint32_t bits = (uint32_t)(bal >> base) & 0xFFFFu;
        const uint32_t src = bits ? base + (uint32_t)__builtin_ctz(bits) : lane;
        uint64_t c = __shfl(m, (int)src);
        c = bits ? c : 0;                                            // a group with nothing pending keeps its list
        if (bits && src == lane) {
#pragma unroll
            for (int i = 0; i < N; i++) key[i] = key[i] == m ? 0 : key[i];      // (keys are distinct)
        }
        const uint64_t left = ans_left_entry(e);
        e = c > e ? (left > c ? c : left) : e;                       // entries above c stay, c lands, the rest move right
        bar = __shfl(e, (int)(base + k - 1));
    }
}

template <bool TOPK> struct AnsTopKI8 {};
template <> struct AnsTopKI8<true> { uint64_t *keys; uint32_t k; };    // keys [n_slice][n_query][k]: a slice's list per query, best first, 0 = empty

// TOPK: the ranked build also keeps the k best keys of the slice per query and writes them to tk.keys; max and sum as ever.
template <int KSTEPS, bool EXPB, bool TOPK = false>
__global__ void __launch_bounds__(kBlock)
k_answer_i8_part(const float *__restrict__ u, const int8_t *__restrict__ w, AnsPart *__restrict__ part,
                 uint32_t n_query, uint32_t D, uint32_t V, QFmt fu, float scale, uint32_t softmax_base, uint32_t tiles_per_slice,
                 const AnsTopKI8<TOPK> tk)
{
    constexpr uint32_t Dp = KSTEPS * 64, PITCH = Dp + 16, NB = kAnsTile / 16;
    __shared__ __attribute__((aligned(16))) uint8_t tile[2][kAnsTile * PITCH];
    const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const uint32_t m0 = (blockIdx.x * kWaves + wave) * 16;
    const uint32_t row = lane & 15, kq = lane >> 4;
    const SmCfg smc{softmax_base, false, false, 1.0f};
    const float scale_log2e = scale * 1.44269504088896341f;
    // A fragments: the wavefront's 16 query rows are read coalesced, turned into codes and passed through a private
    // corner of the second tile buffer (nobody writes it before the barrier below), so that each lane can pick up its
    // row's 16-byte pieces; they stay in registers for the whole slice
    i32x4 a[KSTEPS];
    {
        uint8_t *stage = tile[1] + wave * 16 * PITCH;
        const bool vec = (D & 3u) == 0;
#pragma unroll 4
        for (uint32_t i = lane; i < 16 * (Dp / 4); i += kWave) {
            const uint32_t r = i / (Dp / 4), c = (i % (Dp / 4)) * 4;
            const bool ok = m0 + r < n_query;
            const float *src = u + (size_t)(m0 + r) * D + c;
            float x[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (vec) {
                if (ok && c < D) { const float4 v = *(const float4 *)src; x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w; }
            } else {
#pragma unroll
                for (int j = 0; j < 4; j++) if (ok && c + j < D) x[j] = src[j];
            }
            uint32_t pk = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) pk |= ((uint32_t)qm_code(x[j], fu.iwl, fu.frac) & 0xFFu) << (8 * j);
            *(uint32_t *)(stage + r * PITCH + c) = pk;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ks++) a[ks] = *(const i32x4 *)(stage + row * PITCH + ks * 64 + 16 * kq);
    }
    // accumulator layout: lane l holds answer column l & 15 of a 16-answer block and query rows 4 (l >> 4) + r
    int mx[4] = {kAnsFloor, kAnsFloor, kAnsFloor, kAnsFloor};       // (no logit is that low: the first one becomes the maximum)
    uint32_t bi[4] = {0, 0, 0, 0};
    double sm[4] = {0.0, 0.0, 0.0, 0.0};
    uint64_t lst[TOPK ? 4 : 1] = {};                                 // (ranked build) entry `row` of the sorted lists of query rows 4 kq + r

    const uint32_t n_tiles = (V + kAnsTile - 1) / kAnsTile;
    const uint32_t t_lo = blockIdx.y * tiles_per_slice, t_hi = (t_lo + tiles_per_slice < n_tiles) ? t_lo + tiles_per_slice : n_tiles;
    constexpr uint32_t PIECES = kAnsTile * Dp / 16 / kBlock;             // 16-byte pieces of a tile per thread: 1, 2 or 4
    i32x4 stage_r[PIECES];
    auto fetch = [&](uint32_t t) {
#pragma unroll
        for (uint32_t p = 0; p < PIECES; p++) {
            const uint32_t i = p * kBlock + tid, r = i / (Dp / 16), c = i % (Dp / 16);
            const uint32_t v = t * kAnsTile + r;
            stage_r[p] = i32x4{0, 0, 0, 0};
            if (v < V) stage_r[p] = *(const i32x4 *)(w + (size_t)v * Dp + c * 16);
        }
    };
    auto put = [&](uint32_t b) {
#pragma unroll
        for (uint32_t p = 0; p < PIECES; p++) {
            const uint32_t i = p * kBlock + tid, r = i / (Dp / 16), c = i % (Dp / 16);
            *(i32x4 *)(tile[b] + r * PITCH + c * 16) = stage_r[p];
        }
    };
    if (t_lo < t_hi) { fetch(t_lo); put(0); }
    __syncthreads();
    for (uint32_t t = t_lo; t < t_hi; t++) {
        const uint32_t b = (t - t_lo) & 1u;
        if (t + 1 < t_hi) fetch(t + 1);
        // four independent accumulator chains: the matrix pipe runs them back to back
        i32x4 acc[NB];
#pragma unroll
        for (uint32_t nb = 0; nb < NB; nb++) acc[nb] = i32x4{0, 0, 0, 0};
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ks++)
#pragma unroll
            for (uint32_t nb = 0; nb < NB; nb++) {
                const i32x4 bm = *(const i32x4 *)(tile[b] + (nb * 16 + row) * PITCH + ks * 64 + kq * 16);
                acc[nb] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[ks], bm, acc[nb], 0, 0, 0);
            }
        const uint32_t v0 = t * kAnsTile + row;                          // this lane's column in block nb: v0 + 16 nb
        if (t * kAnsTile + kAnsTile > V) {                               // the ragged last tile: columns past V drop out
#pragma unroll
            for (uint32_t nb = 0; nb < NB; nb++)
#pragma unroll
                for (int r = 0; r < 4; r++) acc[nb][r] = (v0 + 16 * nb < V) ? acc[nb][r] : kAnsFloor;
        }
        // Per query row: the new maximum over the four columns first, ONE rescale of the running sum, then the four terms
        // (summed in float: four values <= 1) -- 2 conversions and 1 multiply-add in double per row and tile.
#pragma unroll
        for (int r = 0; r < 4; r++) {
            int mn = mx[r];
#pragma unroll
            for (uint32_t nb = 0; nb < NB; nb++) mn = acc[nb][r] > mn ? acc[nb][r] : mn;
            const float fs = ans_term<EXPB>(mx[r] - mn, scale, scale_log2e, smc);      // 1 when the maximum stays (no overflow: |codes| < 2^23)
            float e = 0.0f;
#pragma unroll
            for (uint32_t nb = 0; nb < NB; nb++) {
                e += ans_term<EXPB>(acc[nb][r] - mn, scale, scale_log2e, smc);
                bi[r] = (acc[nb][r] == mn) ? v0 + 16 * nb : bi[r];        // columns arrive in ascending order: the later index wins a tie
            }
            sm[r] = sm[r] * (double)fs + (double)e;
            mx[r] = mn;
        }
        if constexpr (TOPK) {
            // this lane's 4 fresh codes of each row against the row's k-th entry: a row of queries is skipped where no lane of
            // the wavefront brings one above it -- most rows, once the first tiles of the slice are through
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const uint64_t bar = __shfl(lst[r], (int)((lane & 48u) + tk.k - 1));
                uint64_t fresh[NB];
                bool any = false;
#pragma unroll
                for (uint32_t nb = 0; nb < NB; nb++) {
                    const uint64_t key = v0 + 16 * nb < V ? ans_key(acc[nb][r], v0 + 16 * nb) : 0;
                    fresh[nb] = key > bar ? key : 0;
                    any |= key > bar;
                }
                if (__ballot(any)) ans_list_insert<NB>(lst[r], fresh, lane, tk.k);     // (wavefront-uniform)
            }
        }
        if (t + 1 < t_hi) put(b ^ 1u);
        __syncthreads();
    }
    // the 16 lanes that hold the same query rows (equal l >> 4) merge their columns
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int m2 = __shfl_xor(mx[r], o);
            const uint32_t i2 = __shfl_xor(bi[r], o);
            const double s2 = __shfl_xor(sm[r], o);
            const int M = m2 > mx[r] ? m2 : mx[r];
            const double f1 = (double)ans_term<EXPB>(mx[r] - M, scale, scale_log2e, smc);
            const double f2 = (double)ans_term<EXPB>(m2 - M, scale, scale_log2e, smc);
            sm[r] = sm[r] * f1 + s2 * f2;
            bi[r] = (m2 == mx[r]) ? (i2 > bi[r] ? i2 : bi[r]) : (m2 > mx[r] ? i2 : bi[r]);
            mx[r] = M;
        }
    }
    if (row == 0) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const uint32_t q = m0 + 4 * kq + r;
            if (q < n_query) part[(size_t)blockIdx.y * n_query + q] = AnsPart{mx[r], bi[r], sm[r]};
        }
    }
    if constexpr (TOPK) {                                                // the lists are merged across the lanes already
        if (row < tk.k) {
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const uint32_t q = m0 + 4 * kq + r;
                if (q < n_query) tk.keys[((size_t)blockIdx.y * n_query + q) * tk.k + row] = lst[r];
            }
        }
    }
}

// The ranked combine: 16 lanes per query merge the slices' lists into one distributed list (ans_list_insert again; a slice's
// list is sorted, so its lanes stop passing the bar early), the maximum and the total merge as in k_answer_i8_combine, and lane j
// writes pick j: its index and e^((code - max) . scale) / total, formed as that kernel forms the labelled answer's probability.
__global__ void __launch_bounds__(kBlock)
k_answer_i8_combine_topk(const AnsPart *__restrict__ part, const uint64_t *__restrict__ keys, uint32_t *__restrict__ top_idx,
                         float *__restrict__ top_p, uint32_t n_query, uint32_t n_slice, uint32_t k, float scale, uint32_t softmax_base)
{
    const SmCfg smc{softmax_base, false, false, 1.0f};
    const uint32_t lane = threadIdx.x & (kWave - 1), sub = lane & 15;
    const uint32_t wave_g = (blockIdx.x * kBlock + threadIdx.x) / kWave, n_wave = gridDim.x * (kBlock / kWave);
    for (uint32_t qb = wave_g * 4; qb < n_query; qb += n_wave * 4) {              // wavefront-uniform trip count
        const uint32_t q = qb + (lane >> 4);
        const bool q_ok = q < n_query;
        uint64_t e = 0;
        for (uint32_t s = 0; s < n_slice; s++) {
            uint64_t key[1] = {(q_ok && sub < k) ? keys[((size_t)s * n_query + q) * k + sub] : 0};
            ans_list_insert<1>(e, key, lane, k);
        }
        if (!q_ok) continue;
        int M = kAnsFloor;
        for (uint32_t s = 0; s < n_slice; s++) {
            const int m = part[(size_t)s * n_query + q].m;
            M = m > M ? m : M;
        }
        double total = 0.0;
        for (uint32_t s = 0; s < n_slice; s++) {
            const AnsPart p = part[(size_t)s * n_query + q];
            total += p.sum * (p.m == M ? 1.0 : (double)sm_exp((float)(p.m - M) * scale, smc));
        }
        if (sub < k) {
            const int code = (int)(uint32_t)(e >> 32) + kAnsFloor;
            const float x = sm_exp((float)(code - M) * scale, smc);
            top_idx[(size_t)q * k + sub] = (uint32_t)e;
            top_p[(size_t)q * k + sub] = (softmax_base == QMANN_SOFTMAX_EXP) ? (float)((double)x / total) : x / (float)total;
        }
    }
}

// merges the slices of a query (ascending dictionary ranges: the later slice wins a tie), writes the prediction and
// accumulates cost / match (cross_entropy_run mode 3).  16 lanes per query: they also form the labelled answer's logit
// code (one row of W against the query's codes -- the same integer the matrix cores produced for that column), so the
// projection kernel carries no label bookkeeping.
__global__ void __launch_bounds__(kBlock)
k_answer_i8_combine(const AnsPart *__restrict__ part, const float *__restrict__ u, const int8_t *__restrict__ w,
                    const uint32_t *__restrict__ answer, uint32_t *__restrict__ pred, float *cost, uint32_t *match,
                    uint32_t n_query, uint32_t n_slice, uint32_t D, uint32_t Dp, uint32_t V, QFmt fu, float scale, uint32_t softmax_base)
{
    const SmCfg smc{softmax_base, false, false, 1.0f};
    const uint32_t lane = threadIdx.x & (kWave - 1), sub = lane & 15;
    const uint32_t wave_g = (blockIdx.x * kBlock + threadIdx.x) / kWave, n_wave = gridDim.x * (kBlock / kWave);
    float cost_acc = 0.0f;
    uint32_t match_acc = 0;
    for (uint32_t qb = wave_g * 4; qb < n_query; qb += n_wave * 4) {              // wavefront-uniform trip count
        const uint32_t q = qb + (lane >> 4);
        const bool q_ok = q < n_query;
        const uint32_t y = (answer && q_ok) ? answer[q] : 0xFFFFFFFFu;
        int ky = 0;
        if (y < V) {
            const uint32_t per = Dp / 16;
            for (uint32_t i = 0; i < per; i++) {
                const uint32_t c = sub * per + i;
                const int code = c < D ? qm_code(u[(size_t)q * D + c], fu.iwl, fu.frac) : 0;
                ky += code * (int)w[(size_t)y * Dp + c];
            }
        }
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) ky += __shfl_xor(ky, o);
        if (sub != 0 || !q_ok) continue;
        int M = kAnsFloor;
        uint32_t bi = 0;
        for (uint32_t s = 0; s < n_slice; s++) {
            const AnsPart p = part[(size_t)s * n_query + q];
            if (p.m >= M && p.m != kAnsFloor) { M = p.m; bi = p.idx; }
        }
        double total = 0.0;
        for (uint32_t s = 0; s < n_slice; s++) {
            const AnsPart p = part[(size_t)s * n_query + q];
            total += p.sum * (p.m == M ? 1.0 : (double)sm_exp((float)(p.m - M) * scale, smc));
        }
        pred[q] = bi;
        if (y < V) {
            const float e = sm_exp((float)(ky - M) * scale, smc);
            const float py = (softmax_base == QMANN_SOFTMAX_EXP) ? (float)((double)e / total) : e / (float)total;
            cost_acc += -py;
            match_acc += (y == bi) ? 1u : 0u;
        }
    }
    if (answer) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { cost_acc += __shfl_xor(cost_acc, o); match_acc += __shfl_xor(match_acc, o); }
        if (lane == 0) {
            if (cost) atomicAdd(cost, cost_acc);
            if (match && match_acc) atomicAdd(match, match_acc);
        }
    }
}

}  // namespace

// the k_answer_small build of a shape, and whether the float layer takes it (otherwise: k_answer, one workgroup per query)
struct AnsSmallPlan {
    uint32_t lpq, vpt, qpw;     // lanes per query, logits per lane (the 64-lane build is <64, 4, 4> whatever vpt says), queries per wavefront
    size_t lds;
    bool fits;
};
static AnsSmallPlan ans_small_plan(uint32_t D, uint32_t V)
{
    AnsSmallPlan p;
    p.lpq = V <= 128 ? 16u : 64u;
    const uint32_t qb = V <= 96 ? 2u : (V <= 128 ? 1u : 4u);
    const uint32_t vpt = (V + p.lpq - 1) / p.lpq;
    p.vpt = vpt <= 2 ? 2u : vpt <= 4 ? 4u : vpt <= 6 ? 6u : 8u;
    p.qpw = kWave / p.lpq * qb;
    p.lds = ((size_t)D * p.lpq * p.vpt + (size_t)kAnsWaves * p.qpw * D) * sizeof(float);
    p.fits = V <= 256u && p.lds <= 78 * 1024;
    return p;
}

// the one-pass int8 form's grid: 64 queries per workgroup, the dictionary's 64-row tiles cut into slices
struct AnsSlices { uint32_t qblocks, n_slice, tps; };
static AnsSlices ans_i8_slices(uint32_t n_query, uint32_t V)
{
    const uint32_t qblocks = (n_query + 16 * kWaves - 1) / (16 * kWaves), n_tiles = (V + kAnsTile - 1) / kAnsTile;
    // ~2 workgroups per CU (measured at 8 192 x 4 096 x 256: 128 workgroups 86 us, 256: 55, 512: 45, 1 024: 46)
    uint32_t n_slice = qblocks >= 512u ? 1u : (512u + qblocks - 1) / qblocks;
    if (n_slice > n_tiles) n_slice = n_tiles;
    const uint32_t tps = (n_tiles + n_slice - 1) / n_slice;
    return AnsSlices{qblocks, (n_tiles + tps - 1) / tps, tps};
}

// qmann_answer_i8's refusals that depend on the net and the matrix format alone (its codes, its order)
static int answer_i8_net_check(const qmann_net *net, qmann_fmt w_fmt)
{
    const uint32_t D = net->dim_emb, Dp = net->dim_emb_pad, V = net->dim_input;
    if (D == 0 || V == 0 || Dp % 64 != 0 || D > Dp) return QMANN_EINVAL;
    if (!qm_fmt8(net->act[net->n_hop - 1]) || !qm_fmt8(w_fmt)) return QMANN_ERANGE;
    if (((size_t)((D + 3) & ~3u) + V) * sizeof(float) > 128 * 1024) return QMANN_ERANGE;
    return QMANN_OK;
}

// qmann_answer_topk_i8's form and workspace for (net, k, n_query): the two-kernel form exactly where qmann_answer_i8 takes it
// whatever `probs` is; otherwise the slices of that call with records of 16 + 8 k bytes -- AnsPart [n_slice][n_query], then the
// keys [n_slice][n_query][k].  The workspace covers both forms, so a switch flipped between the helper and the call changes nothing.
struct AnsTopKI8Plan { bool one_pass; AnsSlices sl; size_t bytes; };
static AnsTopKI8Plan answer_topk_i8_plan(const qmann_net *net, uint32_t k, uint32_t n_query)
{
    AnsTopKI8Plan p{false, AnsSlices{0, 0, 0}, 0};
    if (n_query == 0) return p;
    const uint32_t V = net->dim_input;
    p.one_pass = net->softmax_base != QMANN_SOFTMAX_EXP_PLAN && !qm_tuning().answer_two_pass && (size_t)V * sizeof(float) >= sizeof(AnsPart);
    p.sl = ans_i8_slices(n_query, V);
    const size_t logits = ((size_t)n_query * V * sizeof(float) + 7) & ~(size_t)7;
    const size_t records = (size_t)p.sl.n_slice * n_query * (sizeof(AnsPart) + (size_t)k * sizeof(uint64_t));
    p.bytes = (V >= 4 && records > logits) ? records : logits;
    return p;
}

extern "C" {

// tk: null, or the outputs of qmann_answer_topk_f32 -- the serial-order kernel of the shape in its top-k build (the bookkeeping
// arguments are then unused)
static int answer_f32_impl(const qmann_net *net, const float *w_ans, const float *u, const uint32_t *answer, uint32_t *pred,
                           float *probs, float *cost, uint32_t *match, uint32_t n_query, void *stream, bool allow_fused,
                           const AnsTopK<true> *tk = nullptr)
{
    QmBatched qm_scope;
    if (!net || !w_ans || !u || (!pred && !tk)) return QMANN_EINVAL;
    const uint32_t D = net->dim_emb, V = net->dim_input;
    if (D == 0 || V == 0) return QMANN_EINVAL;
    const size_t lds = ((size_t)((D + 3) & ~3u) + V) * sizeof(float);
    if (lds > 128 * 1024) return QMANN_ERANGE;
    if (n_query == 0) return QMANN_OK;
    if (qm_too_many_queries(n_query)) return QMANN_ERANGE;
    hipStream_t st = (hipStream_t)stream;
    // bAbI shapes (D <= 64, V <= 256), the e^x and 2^x bases: the fused form on the bf16 matrix cores (k_answer_mfma), within
    // 1e-5 on the softmax; qmann_answer_f32_serial / QMANN_ANSWER_EXACT keep the serial-order kernels below
    if (allow_fused && D <= 64u && V <= 256u && net->softmax_base != QMANN_SOFTMAX_EXP_PLAN && !qm_tuning().answer_exact) {
        const uint32_t tiles = (V + 15u) / 16u;
        const uint32_t n_task = (n_query + 15u) / 16u, need = (n_task + kAmWaves - 1) / kAmWaves;
        // the smallest listed tile count that holds the dictionary
        const uint32_t tt = tiles <= 5 ? (tiles <= 2 ? 2u : tiles) : tiles <= 8 ? 8u : tiles <= 12 ? 12u : tiles <= 15 ? 15u : 16u;
        qm_dispatch<2, 3, 4, 5, 8, 12, 15, 16>(tt, [&](auto t) {
            constexpr int TT = decltype(t)::value;
            qm_launch_persistent(k_answer_mfma<TT>, need, QmPersistent{kAmWaves, 4, 256}, 3u * (size_t)TT * 16u * kAmPitch, st,
                                 w_ans, u, answer, pred, probs, cost, match, D, V, net->softmax_base, n_query);
        });
        QM_LAUNCH_CHECK();
        return qm_scope.rc();
    }
    // lanes per query / logits per lane / queries per lane group.  Short dictionaries: 16 lanes (one DPP row), four
    // lane groups side by side in a wavefront (the reductions are most of the work there); the joint-task sizes: the whole
    // wavefront on four queries at once, every weight read from LDS used four times (that kernel is bound by LDS reads)
    // (two queries per lane group up to 96 logits: -6 % on this kernel at V = 80; with 8 logits per lane the second query's state spills)
    const AnsSmallPlan sp = ans_small_plan(D, V);
    const uint32_t lpq = sp.lpq, vpt = sp.vpt, qpw = sp.qpw;
    const size_t lds_small = sp.lds;
    if (sp.fits) {                                          // W^T fits LDS twice per CU
        const uint32_t need = (n_query + kAnsWaves * qpw - 1) / (kAnsWaves * qpw);
        auto go = [&](auto kernel, auto kernel_topk) {      // persistent: two 16-wavefront workgroups per CU
            const QmPersistent wg{kAnsWaves, 8};
            if (tk) qm_launch_persistent(kernel_topk, need, wg, lds_small, st, w_ans, u, answer, pred, probs, cost, match, D, V, net->softmax_base, n_query, *tk);
            else qm_launch_persistent(kernel, need, wg, lds_small, st, w_ans, u, answer, pred, probs, cost, match, D, V, net->softmax_base, n_query, AnsTopK<false>{});
        };
        if (lpq == 64) {
            go(k_answer_small<64, 4, 4>, k_answer_small<64, 4, 4, true>);                   // V in 129 .. 256
        } else {
            switch (vpt) {
            case 2: go(k_answer_small<16, 2, 2>, k_answer_small<16, 2, 2, true>); break;
            case 4: go(k_answer_small<16, 4, 2>, k_answer_small<16, 4, 2, true>); break;
            case 6: go(k_answer_small<16, 6, 2>, k_answer_small<16, 6, 2, true>); break;
            default: go(k_answer_small<16, 8, 1>, k_answer_small<16, 8, 1, true>); break;
            }
        }
        QM_LAUNCH_CHECK();
        return qm_scope.rc();
    }
    const uint32_t grid = n_query < 8192u ? n_query : 8192u;
    if (tk) qm_launch(k_answer<false, true>, grid, kBlock, lds, st, w_ans, u, answer, pred, probs, cost, match, D, V, net->softmax_base, n_query, 0u, 0u, *tk);
    else qm_launch(k_answer<false>, grid, kBlock, lds, st,
              w_ans, u, answer, pred, probs, cost, match, D, V, net->softmax_base, n_query, 0u, 0u, AnsTopK<false>{});
    QM_LAUNCH_CHECK();
    return qm_scope.rc();
}

int qmann_answer_f32(const qmann_net *net, const float *w_ans, const float *u, const uint32_t *answer,
                     uint32_t *pred, float *probs, float *cost, uint32_t *match, uint32_t n_query, void *stream)
{
    return answer_f32_impl(net, w_ans, u, answer, pred, probs, cost, match, n_query, stream, true);
}

int qmann_answer_f32_serial(const qmann_net *net, const float *w_ans, const float *u, const uint32_t *answer,
                            uint32_t *pred, float *probs, float *cost, uint32_t *match, uint32_t n_query, void *stream)
{
    return answer_f32_impl(net, w_ans, u, answer, pred, probs, cost, match, n_query, stream, false);
}

int qmann_answer_topk_f32(const qmann_net *net, const float *w_ans, const float *u, uint32_t k, uint32_t *top_idx, float *top_p,
                          uint32_t n_query, void *stream)
{
    if (!net || !w_ans || !u || !top_idx || !top_p) return QMANN_EINVAL;
    if (k == 0 || k > QMANN_MAX_TOPK || k > net->dim_input) return QMANN_EINVAL;
    const AnsTopK<true> tk{top_idx, top_p, k};
    return answer_f32_impl(net, w_ans, u, nullptr, nullptr, nullptr, nullptr, nullptr, n_query, stream, false, &tk);
}

int qmann_answer_i8(const qmann_net *net, const int8_t *w_ans_i8, qmann_fmt w_fmt, const float *u, float *logits_ws,
                    const uint32_t *answer, uint32_t *pred, float *probs, float *cost, uint32_t *match,
                    uint32_t n_query, void *stream)
{
    QmBatched qm_scope;
    if (!net || !w_ans_i8 || !u || !logits_ws || !pred) return QMANN_EINVAL;
    const uint32_t D = net->dim_emb, Dp = net->dim_emb_pad, V = net->dim_input;
    if (D == 0 || V == 0 || Dp % 64 != 0 || D > Dp) return QMANN_EINVAL;
    const qmann_fmt fu = net->act[net->n_hop - 1];           // u is the last sum_vec output
    if (!qm_fmt8(fu) || !qm_fmt8(w_fmt)) return QMANN_ERANGE;
    const size_t lds = ((size_t)((D + 3) & ~3u) + V) * sizeof(float);
    if (lds > 128 * 1024) return QMANN_ERANGE;
    if (n_query == 0) return QMANN_OK;
    if (qm_too_many_queries(n_query)) return QMANN_ERANGE;
    const float scale = 1.0f / (float)(1u << (fu.frac + w_fmt.frac));
    hipStream_t st = (hipStream_t)stream;
    const QFmt fuq = qm_qfmt(fu);
    // (the running-maximum normaliser needs a true exponential: the piece-wise linear exp_plan takes the two-pass form; so does a
    // dictionary of 1, 2 or 3 answers, whose documented workspace of V floats per query is smaller than one record)
    const bool records_fit = (size_t)V * sizeof(float) >= sizeof(AnsPart);
    if (!probs && net->softmax_base != QMANN_SOFTMAX_EXP_PLAN && !qm_tuning().answer_two_pass && records_fit) {
        // one pass: no logits round trip; the workspace holds the per-slice records
        // the records fit logits_ws: V >= 4 here, and n_slice <= ceil(V / 64) gives 16 n_slice <= 4 V bytes per query
        const AnsSlices sl = ans_i8_slices(n_query, V);
        const uint32_t qblocks = sl.qblocks, n_slice = sl.n_slice, tps = sl.tps;
        AnsPart *part = (AnsPart *)logits_ws;
        const dim3 grid1(qblocks, n_slice);
        const bool eb = net->softmax_base == QMANN_SOFTMAX_EXP;
        if (!qm_dispatch<64, 128, 256>(Dp, [&](auto dp) {
                constexpr int KS = decltype(dp)::value / 64;
                qm_dispatch<false, true>(eb, [&](auto e) {
                    k_answer_i8_part<KS, decltype(e)::value><<<grid1, kBlock, 0, st>>>(u, w_ans_i8, part, n_query, D, V, fuq, scale, net->softmax_base, tps,
                                                                                       AnsTopKI8<false>{});
                });
            }))
            return QMANN_EUNSUPPORTED;
        const uint32_t cb = (n_query * 16 + kBlock - 1) / kBlock;
        k_answer_i8_combine<<<cb < 2048u ? cb : 2048u, kBlock, 0, st>>>(part, u, w_ans_i8, answer, pred, cost, match, n_query, n_slice, D, Dp, V,
                                                                        fuq, scale, net->softmax_base);
        QM_LAUNCH_CHECK();
        return qm_scope.rc();
    }
    const dim3 grid((n_query + 16 * kWaves - 1) / (16 * kWaves), (V + 16 * kTilesPerBlockY - 1) / (16 * kTilesPerBlockY));
    if (!qm_dispatch<64, 128, 256>(Dp, [&](auto dp) {
            k_logits_mfma_i8<decltype(dp)::value / 64><<<grid, kBlock, 0, st>>>(u, w_ans_i8, logits_ws, n_query, D, V, fuq, scale);
        }))
        return QMANN_EUNSUPPORTED;
    // the normaliser in the order of the float layer's kernel for this shape: probabilities bit-identical to it (see k_answer)
    const AnsSmallPlan sp = ans_small_plan(D, V);
    qm_launch(k_answer<true>, n_query < 8192u ? n_query : 8192u, kBlock, lds, st,
              logits_ws, nullptr, answer, pred, probs, cost, match, D, V, net->softmax_base, n_query,
              sp.fits ? sp.lpq : 0u, sp.lpq == 64u ? 4u : sp.vpt, AnsTopK<false>{});
    QM_LAUNCH_CHECK();
    return qm_scope.rc();
}

size_t qmann_answer_topk_i8_ws_bytes(const qmann_net *net, uint32_t k, uint32_t n_query)
{
    if (!net || net->n_hop == 0 || net->n_hop > QMANN_MAX_HOP) return 0;
    const uint32_t D = net->dim_emb, Dp = net->dim_emb_pad, V = net->dim_input;
    if (D == 0 || V == 0 || Dp % 64 != 0 || D > Dp || !qm_fmt8(net->act[net->n_hop - 1])) return 0;
    if (((size_t)((D + 3) & ~3u) + V) * sizeof(float) > 128 * 1024) return 0;
    if (k == 0 || k > QMANN_MAX_TOPK || k > V || (Dp != 64 && Dp != 128 && Dp != 256)) return 0;
    return answer_topk_i8_plan(net, k, n_query).bytes;
}

int qmann_answer_topk_i8(const qmann_net *net, const int8_t *w_ans_i8, qmann_fmt w_fmt, const float *u, void *ws, size_t ws_bytes,
                         uint32_t k, uint32_t *top_idx, float *top_p, uint32_t n_query, void *stream)
{
    if (!net || !w_ans_i8 || !u || !top_idx || !top_p) return QMANN_EINVAL;
    if (const int rc = answer_i8_net_check(net, w_fmt)) return rc;
    const uint32_t D = net->dim_emb, Dp = net->dim_emb_pad, V = net->dim_input;
    if (k == 0 || k > QMANN_MAX_TOPK || k > V) return QMANN_EINVAL;
    const AnsTopKI8Plan plan = answer_topk_i8_plan(net, k, n_query);
    if (!ws || ((uintptr_t)ws & 7u) || ws_bytes < qmann_answer_topk_i8_ws_bytes(net, k, n_query)) return QMANN_EINVAL;
    if (n_query == 0) return QMANN_OK;
    if (qm_too_many_queries(n_query)) return QMANN_ERANGE;
    if (Dp != 64 && Dp != 128 && Dp != 256) return QMANN_EUNSUPPORTED;
    QmBatched qm_scope;
    const qmann_fmt fu = net->act[net->n_hop - 1];
    const float scale = 1.0f / (float)(1u << (fu.frac + w_fmt.frac));
    hipStream_t st = (hipStream_t)stream;
    const QFmt fuq = qm_qfmt(fu);
    if (plan.one_pass) {
        const AnsSlices sl = plan.sl;
        AnsPart *part = (AnsPart *)ws;
        const AnsTopKI8<true> tk{(uint64_t *)(part + (size_t)sl.n_slice * n_query), k};
        const dim3 grid1(sl.qblocks, sl.n_slice);
        const bool eb = net->softmax_base == QMANN_SOFTMAX_EXP;
        qm_dispatch<64, 128, 256>(Dp, [&](auto dp) {
            constexpr int KS = decltype(dp)::value / 64;
            qm_dispatch<false, true>(eb, [&](auto e) {
                k_answer_i8_part<KS, decltype(e)::value, true><<<grid1, kBlock, 0, st>>>(u, w_ans_i8, part, n_query, D, V, fuq, scale, net->softmax_base,
                                                                                         sl.tps, tk);
            });
        });
        const uint32_t cb = (n_query * 16 + kBlock - 1) / kBlock;
        k_answer_i8_combine_topk<<<cb < 2048u ? cb : 2048u, kBlock, 0, st>>>(part, tk.keys, top_idx, top_p, n_query, sl.n_slice, k, scale, net->softmax_base);
        QM_LAUNCH_CHECK();
        return qm_scope.rc();
    }
    float *logits = (float *)ws;
    const dim3 grid((n_query + 16 * kWaves - 1) / (16 * kWaves), (V + 16 * kTilesPerBlockY - 1) / (16 * kTilesPerBlockY));
    qm_dispatch<64, 128, 256>(Dp, [&](auto dp) {
        k_logits_mfma_i8<decltype(dp)::value / 64><<<grid, kBlock, 0, st>>>(u, w_ans_i8, logits, n_query, D, V, fuq, scale);
    });
    // k_answer<true>'s launch, in its ranked build: the same normaliser order, hence qmann_answer_i8's probabilities bit for bit
    const AnsSmallPlan sp = ans_small_plan(D, V);
    const size_t lds = ((size_t)((D + 3) & ~3u) + V) * sizeof(float);
    qm_launch(k_answer<true, true>, n_query < 8192u ? n_query : 8192u, kBlock, lds, st,
              logits, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, D, V, net->softmax_base, n_query,
              sp.fits ? sp.lpq : 0u, sp.lpq == 64u ? 4u : sp.vpt, AnsTopK<true>{top_idx, top_p, k});
    QM_LAUNCH_CHECK();
    return qm_scope.rc();
}

}  // extern "C"
