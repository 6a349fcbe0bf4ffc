// answer_i8.h -- the int8 answer layer's own kernels: the projection of the two-kernel form (k_logits_mfma_i8; its softmax is
// answer_serial.h's k_answer on the precomputed logits), the one-pass form (k_answer_i8_part, its two combine kernels, the
// distributed sorted lists of the ranked builds) and that form's grid.  batch_answer_i8.hip launches them.
#pragma once
#include "hops_common.h"

namespace {

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

// ---- host side --------------------------------------------------------------------------------------------------------------
// the one-pass form's grid: 64 queries per workgroup, the dictionary's 64-row tiles cut into slices
struct AnsSlices { uint32_t qblocks, n_slice, tps; };
static inline AnsSlices ans_i8_slices(uint32_t n_query, uint32_t V)
{
    // (n_query + 63 would wrap to 0 workgroups within 63 of 2^32, and the division below would trap: the plan also sizes the
    // workspace of a batch that is then refused for its 2^24 queries)
    const uint32_t qblocks = n_query / (16 * kWaves) + (n_query % (16 * kWaves) != 0), n_tiles = (V + kAnsTile - 1) / kAnsTile;
    // ~2 workgroups per CU (measured at 8 192 x 4 096 x 256: 128 workgroups 86 us, 256: 55, 512: 45, 1 024: 46)
    uint32_t n_slice = qblocks >= 512u ? 1u : (512u + qblocks - 1) / qblocks;
    if (n_slice > n_tiles) n_slice = n_tiles;
    const uint32_t tps = (n_tiles + n_slice - 1) / n_slice;
    return AnsSlices{qblocks, (n_tiles + tps - 1) / tps, tps};
}

}  // namespace
