// batch_hops_top_float.hip -- attended slots for float attention (ATTENTION_MODE 1): qmann_hops_top_float_i8 (every query its own
// memory) and qmann_hops_shared_top_float_i8 (one memory for all queries).  The hop kernels of batch_hops_float.hip and
// batch_hops_shared_float.hip with the selection of hops_attended_float.h behind the softmax of each query's hop: the k rows
// a hop weighted most leave the kernel, and no [n_hop][rows] probability array is written.
//
// ONE kernel text serves both calls, in a unit of its own.  A TOP switch on k_hops_float or k_hops_shared_float -- even as a thin
// kernel around one shared body -- changes the plain builds' device code (register allocation from the first kernarg load on:
// tools/device_asm_equal.sh), and those are the measured kernels.  So this is k_hops_shared_float's text (the tile of QT queries,
// the key-only and memory-only work done once per tile, every query's float additions in k_hops_float's order) with AttTop<true>
// as its last argument, and its STORY build is the per-story kernel: one query per workgroup on rows row_off[q] ..
// row_off[q + 1] of private planes, the length cut to max_slots, an empty story allowed, the planes streamed past the caches as
// k_hops_float streams them.  k_hops_shared_float promises k_hops_float's bits under every tile, so both builds give the
// `probs` tap's floats and the base calls' u_out.  Keep the three texts in step.  No taps are written.
#include "hops_attended_float.h"
#include "hops_float_common.h"
#include "hops_host.h"

namespace {

// STORY: QT = 1, per_q unused.  Shared: per_q = bytes of LDS per query, a.max_slots = n_slots >= 1, a.row_off unused
template <int LPR, int QT, bool STORY>
__global__ void __launch_bounds__(kBlock)
k_hops_top_float(const HopArgs a, const uint32_t n_query, const uint32_t per_q, const AttTop<true> tp)
{
    static_assert(!STORY || QT == 1, "a story is one query's");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr uint32_t Dp = LPR * 16;
    const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const uint32_t q0 = blockIdx.x * QT;
    const uint32_t nq = n_query - q0 < (uint32_t)QT ? n_query - q0 : (uint32_t)QT;     // queries of this tile (the last may be short)
    uint32_t r0 = 0, S = a.max_slots;
    if constexpr (STORY) {
        r0 = a.row_off[q0];
        const uint32_t S_in = a.row_off[q0 + 1] - r0;
        S = S_in < a.max_slots ? S_in : a.max_slots;              // never index LDS past what the launch reserved
    }
    const uint32_t D = a.D;
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
        if (S > 0) {
            FloatDotConst c[QT];
#pragma unroll
            for (int t = 0; t < QT; t++) make_float_dot_const(c[t], FloatQueryLds(slice((uint32_t)t)).kuq, (lane % LPR) * 16);
            const uint8_t *kb = (const uint8_t *)a.keys + (size_t)h * a.hop_stride + (size_t)r0 * Dp;
            auto retire = [&](uint32_t t, uint32_t r, int v) { FloatQueryLds(smem + t * per_q).sc[r] = v; };
            if (S >= (kWave / LPR) * 4) {
                if constexpr (STORY)
                    scan_rows<LPR, 4, true, kWaves>(kb, S, [&](const i32x4 x) { return float_dot_lane_sum(x, c[0]); },
                                                    [&](uint32_t r, int v) { retire(0u, r, v); }, lane, wave);
                else
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

        // softmax per query on its slice; p replaces the score in place (no taps: the offset is unused)
        if (S > 0) {
            for (uint32_t t = 0; t < nq; t++) {
                const FloatQueryLds L(slice(t));
                float_softmax_slots(a, h, S, scale, 0, L.sc, L.red, tid, lane, wave);
            }
        }
        __syncthreads();

        // the attended slots of every live query, each from its own slice (spare places: nothing runs, nothing is stored)
        for (uint32_t t = 0; t < nq; t++) {
            const FloatQueryLds L(smem + t * per_q);
            attended_select_float(tp, (size_t)(q0 + t) * a.n_hop + h, S, (const float *)L.sc, L.red, tid, lane, wave);
        }

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
            const uint8_t *vb = (const uint8_t *)a.vals + (size_t)h * a.hop_stride + (size_t)r0 * Dp + chunk * 16;
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
                    for (int j = 0; j < UN; j++) x[j] = load16<STORY>(pp + (size_t)j * RPW * Dp);     // a shared plane is to stay in L2
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

}  // namespace

// the per-story call's last steps, on the HopArgs that qm_hops_i8 has checked and filled (taps: none)
extern "C" int qmann_hops_top_float_impl(const HopArgs &a, uint32_t Dp, uint32_t max_slots, uint32_t k, uint32_t *top_slot, float *top_p,
                                         uint32_t n_query, void *stream)
{
    QmBatched qm_scope;
    const size_t lds = float_story_lds_bytes(max_slots);
    if (lds > kHopLdsLimit) return QMANN_ERANGE;                      // (the float launcher's own refusal)
    if (!att_top_args_ok(k, top_slot, top_p)) return QMANN_EINVAL;         // behind every refusal of the base call
    const AttTop<true> tp{top_slot, top_p, k};
    qm_dispatch<4, 8, 16>(Dp / 16, [&](auto lpr) {
        qm_launch(k_hops_top_float<decltype(lpr)::value, 1, true>, n_query, dim3(kBlock), lds, (hipStream_t)stream, a, n_query, 0u, tp);
    });
    QM_LAUNCH_CHECK();
    return qm_scope.rc();
}

extern "C" {

int qmann_hops_shared_top_float_i8(const qmann_net *net, const int8_t *keys, const int8_t *vals, size_t hop_stride, uint32_t n_slots,
                                   const float *u0, float *u_out, uint32_t k, uint32_t *top_slot, float *top_p, uint32_t n_query,
                                   void *stream)
{
    QmBatched qm_scope;
    // qmann_hops_shared_float_i8's refusals, in its order
    if (const int rc = shared_open(net, keys, vals, u0, u_out)) return rc;
    HopArgs a;
    if (const int rc = shared_fill(a, net, keys, vals, hop_stride, hop_stride, n_slots, u0, u_out, nullptr, nullptr,
                                   net->attention_mode == QMANN_ATT_FLOAT)) return rc;
    if (qmann_hops_shared_float_lds_bytes(n_slots, 1) > kHopLdsLimit) return QMANN_ERANGE;
    if (int rc; shared_no_queries(n_query, rc)) return rc;
    if (!att_top_args_ok(k, top_slot, top_p)) return QMANN_EINVAL;         // behind every refusal of the base call

    const AttTop<true> tp{top_slot, top_p, k};
    const uint32_t qt = qmann_hops_shared_float_tile(n_slots, n_query);    // the base call's tile (QMANN_SHARED_QT forces one)
    const uint32_t per_q = (uint32_t)qmann_hops_shared_float_lds_bytes(n_slots, 1);
    qm_dispatch<4, 8, 16>(net->dim_emb_pad / 16, [&](auto lpr) {
        qm_dispatch<1, 2, 4, 8>(qt, [&](auto t) {
            constexpr int LPR = decltype(lpr)::value, QT = decltype(t)::value;
            qm_launch(k_hops_top_float<LPR, QT, false>, qm_cdiv(n_query, qt), dim3(kBlock), (size_t)qt * per_q, (hipStream_t)stream, a,
                      n_query, per_q, tp);
        });
    });
    QM_LAUNCH_CHECK();
    return qm_scope.rc();
}

}  // extern "C"
