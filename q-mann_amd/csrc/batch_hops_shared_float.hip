// batch_hops_shared_float.hip -- qmann_hops_shared_float_i8: float attention (ATTENTION_MODE 1) when every query reads the SAME
// memory.  To batch_hops_float.hip what batch_hops_shared.hip is to batch_hops.hip.
//
// k_hops_float gives a workgroup one query and streams that query's private key AND value planes from HBM (p is not quantised:
// every value row counts).  Here both planes are one for all queries and stay in L2, so the hop is vector-issue work, and what
// depends on the memory alone is done once for a tile of QT queries.  One 256-thread workgroup owns QT queries and per hop
//
//   1. scans the key plane ONCE for its tile: per loaded dword the sign mask and the magnitudes are taken once, then one select and
//      one v_dot4 per query against that query's constants (the scores are the exact integers of k_hops_float's dot_lane_sum);
//   2. runs the softmax per query on the query's own slice of LDS (hops_float_common.h::float_softmax_slots: k_hops_float's stage,
//      same thread-to-slot mapping, same reductions, same quotient);
//   3. reads the value plane ONCE for its tile: each loaded dword becomes four floats once (6 word operations + 4 converts), then
//      one FMA per byte and query.  Every query's additions run in k_hops_float's order -- the same rows on the same lanes in the
//      same tiles, the same __shfl_xor fold, the same per-wavefront partials summed in wavefront order -- which makes o, and with
//      it everything behind it, bit-equal to the per-story kernel's;
//   4. linear map and hop update per query (hops_common.h::linmap_update).
//
// A last tile with fewer than QT queries scans and reads out with a live query's constants and weights in the spare places and
// drops their sums: nothing is stored for them.
#include "hops_float_common.h"
#include "hops_host.h"

namespace {

// per_q: bytes of LDS per query (qmann_hops_shared_float_lds_bytes(n_slots, 1)); a.max_slots = n_slots >= 1
template <int LPR, int QT>
__global__ void __launch_bounds__(kBlock)
k_hops_shared_float(const HopArgs a, const uint32_t n_query, const uint32_t per_q)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr uint32_t Dp = LPR * 16;
    const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const uint32_t q0 = blockIdx.x * QT;
    const uint32_t nq = n_query - q0 < (uint32_t)QT ? n_query - q0 : (uint32_t)QT;     // queries of this tile (the last may be short)
    const uint32_t S = a.max_slots, D = a.D;
    // the slice of place t: a spare place of a short tile reads the last live query's
    auto slice = [&](uint32_t t) { return smem + (t < nq ? t : nq - 1) * per_q; };

    for (uint32_t t = 0; t < nq; t++) FloatQueryLds(slice(t)).u_f[tid] = (tid < D) ? a.u0[(size_t)(q0 + t) * D + tid] : 0.0f;
    __syncthreads();

    for (uint32_t h = 0; h < a.n_hop; h++) {
        const QFmt fw = a.w[h], fb = a.bin;
        const QFmt fsrc = h == 0 ? a.w[0] : a.act[h - 1];              // grid u sits on (emb_q or sv[h-1])
        for (uint32_t t = 0; t < nq; t++) {
            const FloatQueryLds L(slice(t));
            const float uv = L.u_f[tid];
            L.ku[tid] = (short)((tid < D) ? qm_code_or_sign(uv, fb.iwl, fb.frac) : 0);
            L.kuq[tid] = (int8_t)((tid < D) ? qm_code(relu_if(uv, hop_relu(a, h)), fsrc.iwl, fsrc.frac) : 0);   // exact: u is on that grid
        }
        __syncthreads();

        // the key scan: one pass over the plane for the whole tile
        const float scale = qm_scale_down(1.0f, fw.frac + fsrc.frac);
        {
            FloatDotConst c[QT];
#pragma unroll
            for (int t = 0; t < QT; t++) make_float_dot_const(c[t], FloatQueryLds(slice((uint32_t)t)).kuq, (lane % LPR) * 16);
            const uint8_t *kb = (const uint8_t *)a.keys + (size_t)h * a.hop_stride;
            auto retire = [&](uint32_t t, uint32_t r, int v) { FloatQueryLds(smem + t * per_q).sc[r] = v; };
            if (S >= (kWave / LPR) * 4) {
                scan_rows_shared_float<LPR, 4, QT>(kb, S, c, nq, retire, lane, wave);
            } else {                                                 // below one tile of rows: right, not fast
#pragma unroll
                for (int t = 0; t < QT; t++)
                    if ((uint32_t)t < nq)
                        scan_rows_short<LPR>(kb, S, [&](const i32x4 x) { return float_dot_lane_sum(x, c[t]); },
                                             [&](uint32_t r, int v) { retire((uint32_t)t, r, v); }, lane, wave, (uint32_t)kWaves);
            }
        }
        __syncthreads();

        // softmax per query on its slice; p replaces the score in place
        for (uint32_t t = 0; t < nq; t++) {
            const FloatQueryLds L(slice(t));
            float_softmax_slots(a, h, S, scale, ((size_t)h * n_query + q0 + t) * S, L.sc, L.red, tid, lane, wave);
        }
        __syncthreads();

        // dense float read-out for the whole tile: k_hops_float's value tiles (lane (sub, chunk) owns 16 columns of every
        // (64 / LPR)-th row; UN loads per lane, the next tile in flight), each loaded dword converted once
        {
            constexpr uint32_t RPW = kWave / LPR;
            constexpr int UN = 4;
            constexpr uint32_t TILE = RPW * UN, STEP = kWaves * TILE;
            const uint32_t sub = lane / LPR, chunk = lane % LPR;
            const float vscale = qm_scale_down(1.0f, fw.frac);
            float acc[QT][16];
            const float *pf[QT];
#pragma unroll
            for (int t = 0; t < QT; t++) {
                pf[t] = (const float *)FloatQueryLds(slice((uint32_t)t)).sc;
#pragma unroll
                for (int i = 0; i < 16; i++) acc[t][i] = 0.0f;
            }
            const uint8_t *vb = (const uint8_t *)a.vals + (size_t)h * a.hop_stride + chunk * 16;
            // acc[t][i] += (p_t . 2^-frac) . code; `live`: false for the rows a moved-back tile repeats, which add zero
            auto accumulate = [&](const i32x4 x, uint32_t r, bool live) {
                float ps[QT];
#pragma unroll
                for (int t = 0; t < QT; t++) ps[t] = live ? pf[t][r] * vscale : 0.0f;
#pragma unroll
                for (int d = 0; d < 4; d++) {
                    float v0, v1, v2, v3;
                    float_vals4((uint32_t)x[d], v0, v1, v2, v3);    // memory-only work: once per tile of queries
#pragma unroll
                    for (int t = 0; t < QT; t++) {
                        acc[t][4 * d + 0] = __builtin_fmaf(ps[t], v0, acc[t][4 * d + 0]);
                        acc[t][4 * d + 1] = __builtin_fmaf(ps[t], v1, acc[t][4 * d + 1]);
                        acc[t][4 * d + 2] = __builtin_fmaf(ps[t], v2, acc[t][4 * d + 2]);
                        acc[t][4 * d + 3] = __builtin_fmaf(ps[t], v3, acc[t][4 * d + 3]);
                    }
                }
            };
            if (S >= TILE) {
                const uint32_t n_tiles = (S + TILE - 1) / TILE;
                auto tile_start = [&](uint32_t base) { return base + TILE <= S ? base : S - TILE; };
                auto issue = [&](i32x4 (&x)[UN], uint32_t base) {
                    const uint8_t *pp = vb + (size_t)(tile_start(base) + sub) * Dp;
#pragma unroll
                    for (int j = 0; j < UN; j++) x[j] = *(const i32x4 *)(pp + (size_t)j * RPW * Dp);     // plain: the plane is to stay in L2
                };
                auto consume = [&](const i32x4 (&x)[UN], uint32_t base) {
                    const uint32_t start = tile_start(base);
#pragma unroll
                    for (int j = 0; j < UN; j++) {
                        const uint32_t r = start + j * RPW + sub;
                        accumulate(x[j], r, r >= base);
                    }
                };
                if (wave < n_tiles) {
                    i32x4 xa[UN], xb[UN];
                    uint32_t base = wave * TILE;
                    issue(xa, base);
                    for (uint32_t t = wave; t < n_tiles; t += 2 * kWaves) {
                        issue(xb, base + STEP);
                        consume(xa, base);
                        if (t + kWaves >= n_tiles) break;
                        issue(xa, base + 2 * STEP);
                        consume(xb, base + STEP);
                        base += 2 * STEP;
                    }
                }
            } else {
                for (uint32_t r = wave * RPW + sub; r < S; r += kWaves * RPW)
                    accumulate(*(const i32x4 *)(vb + (size_t)r * Dp), r, true);
            }
            // per query: fold the RPW row groups of a wavefront (lanes with equal chunk), then the wavefronts in their order
#pragma unroll
            for (int t = 0; t < QT; t++) {
#pragma unroll
                for (int i = 0; i < 16; i++) {
                    float v = acc[t][i];
                    for (uint32_t o = LPR; o < kWave; o <<= 1) v += __shfl_xor(v, (int)o);
                    acc[t][i] = v;
                }
            }
            __syncthreads();                                   // the histogram areas are free now
#pragma unroll
            for (int t = 0; t < QT; t++) {
                if ((uint32_t)t < nq && sub == 0) {            // (spare places: nothing is stored)
                    float *part = FloatQueryLds(smem + (uint32_t)t * per_q).part;
#pragma unroll
                    for (int i = 0; i < 16; i++) part[wave * 256 + chunk * 16 + i] = acc[t][i];
                }
            }
            __syncthreads();
            for (uint32_t t = 0; t < nq; t++) {
                const FloatQueryLds L(slice(t));
                if (tid < Dp) {
                    float s = 0.0f;
                    for (int w = 0; w < kWaves; w++) s += L.part[w * 256 + tid];
                    L.o_f[tid] = s;
                }
            }
            __syncthreads();
        }
        for (uint32_t t = 0; t < nq; t++) {
            const FloatQueryLds L(slice(t));
            linmap_update<Dp>(a, q0 + t, h, L.ku, L.u_f, L.o_f, tid);
        }
    }
    for (uint32_t t = 0; t < nq; t++) {
        const FloatQueryLds L(slice(t));
        if (tid < D) a.u_out[(size_t)(q0 + t) * D + tid] = relu_if(L.u_f[tid], a.en_non_lin != 0);
    }
}

// Queries per workgroup.  What LDS allows is the frame (a float per slot and query: 2 at 10 000 slots, 8 up to 2 752); inside it
// the choice is by measurement (tools/shared_float_ab.py, 4 096 queries x 3 hops, five interleaved rounds; every round is in
// DESIGN.md section 5, "Measured, shared plane, float"), and the measurement says ONE query per workgroup at all three shapes:
// 10 000 x 128: 2.54 ms (2: 3.47); 1 000 x 60: 0.229 ms (2: 0.240, 4: 0.370, 8: 0.356); 200 x 60: 0.131 ms (2: 0.150, 4: 0.231,
// 8: 0.221) -- against 4.81 / 0.292 / 0.149 ms for qmann_hops_i8 on copies.  A larger tile does less vector work per query but
// leaves fewer wavefronts on a SIMD (182 registers from two queries on, and at 10 000 slots two slices fill a CU's LDS), and the
// L2 latency of two tiles in flight is then no longer covered.  Between and beyond those shapes nothing is measured: the choice is
// 1 everywhere.  QMANN_SHARED_QT (1, 2, 4, 8) forces a tile size that fits, for that measurement and for the tests.
uint32_t choose_float_qt(uint32_t n_slots, uint32_t n_query)
{
    (void)n_query;
    uint32_t fit = 8;
    while (fit > 1 && qmann_hops_shared_float_lds_bytes(n_slots, fit) > kHopLdsLimit) fit >>= 1;
    const uint32_t forced = qm_tuning().shared_qt;
    if (forced) return forced < fit ? forced : fit;
    return 1;
}

}  // namespace

extern "C" {

size_t qmann_hops_shared_float_lds_bytes(uint32_t n_slots, uint32_t queries_per_group)
{
    return (size_t)queries_per_group * (qmann_hops_lds_bytes(0) + (((size_t)n_slots * 4 + 15) & ~(size_t)15));
}

uint32_t qmann_hops_shared_float_tile(uint32_t n_slots, uint32_t n_query)
{
    if (n_slots == 0 || n_query == 0 || qmann_hops_shared_float_lds_bytes(n_slots, 1) > kHopLdsLimit) return 0;
    return choose_float_qt(n_slots, n_query);
}

int qmann_hops_shared_float_i8(const qmann_net *net, const int8_t *keys, const int8_t *vals, size_t hop_stride, uint32_t n_slots,
                               const float *u0, float *u_out, const qmann_taps *taps, uint32_t n_query, void *stream)
{
    QmBatched qm_scope;
    static_assert(kOffScores % 16 == 0, "a query's slice starts 16-byte aligned");
    // (the steps of hops_host.h's shared-plane prelude; the float calls' mode is refused BEHIND the formats, inside the fill)
    if (const int rc = shared_open(net, keys, vals, u0, u_out)) return rc;
    HopArgs a;
    if (const int rc = shared_fill(a, net, keys, vals, hop_stride, hop_stride, n_slots, u0, u_out, taps, nullptr,
                                   net->attention_mode == QMANN_ATT_FLOAT)) return rc;
    if (qmann_hops_shared_float_lds_bytes(n_slots, 1) > kHopLdsLimit) return QMANN_ERANGE;
    if (int rc; shared_no_queries(n_query, rc)) return rc;

    const uint32_t qt = choose_float_qt(n_slots, n_query), per_q = (uint32_t)qmann_hops_shared_float_lds_bytes(n_slots, 1);
    qm_dispatch<4, 8, 16>(net->dim_emb_pad / 16, [&](auto lpr) {
        qm_dispatch<1, 2, 4, 8>(qt, [&](auto t) {
            constexpr int LPR = decltype(lpr)::value, QT = decltype(t)::value;
            qm_launch(k_hops_shared_float<LPR, QT>, qm_cdiv(n_query, qt), dim3(kBlock), (size_t)qt * per_q, (hipStream_t)stream, a,
                      n_query, per_q);
        });
    });
    QM_LAUNCH_CHECK();
    return qm_scope.rc();
}

}  // extern "C"
