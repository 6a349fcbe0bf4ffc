// batch_hops_shared.hip -- qmann_hops_shared_i8: the fused hops when every query reads the SAME memory (one knowledge base or
// document, many questions).
//
// batch_hops.hip gives a workgroup one query and streams that query's private key plane from HBM.  Here the plane is one for
// all queries -- 1.28 MB per hop at 10 000 x 128, resident in an XCD's 4 MiB L2 -- so the scan is bound by vector issue, and
// work that depends on the key alone can be shared: one 256-thread workgroup owns QT queries, and per hop
//
//   1. scans the key plane ONCE for its tile of queries: a 16-byte key load (plain, not `nt`: the plane is to stay in L2) is
//      split once into even / odd magnitudes and sign bits (hops_lean.h::split_key_row) and then meets QT sets of lane
//      constants (ScanConst, one per query): 6 (word length 7) or 8 vector operations per 4 key bytes and query, plus 4
//      shared by the tile, against 9 / 11 in k_hops_fixed.  The arithmetic is that of hops_common.h, unchanged: the scores
//      are those of qmann_hops_i8 bit for bit;
//   2. runs the rest of the hop per query, one after the other, on that query's own slice of LDS (the carve-up of
//      hops_common.h, QT times): histogram softmax, survivor search, sparse read-out, linear map, hop update.
//
// A last tile with fewer than QT queries scans with a live query's constants in the spare places and drops their sums.
#include "hops_attended.h"

namespace {

// (QueryLds and scan_rows_shared: hops_shared.h, shared with batch_hops_shared_split.hip; the call prelude: hops_host.h)
// per_q: bytes of LDS per query (qmann_hops_lds_bytes(n_slots)); a.max_slots = n_slots >= 1
// TOP (qmann_hops_shared_top_i8): behind every query's hop its k most attended slots go to tp.slot / tp.p (hops_attended.h).
// The TOP builds are instantiations of their own: the others take an EMPTY last argument and keep their device code.
template <int LPR, int QT, bool W7, bool TOP = false>
__global__ void __launch_bounds__(kBlock, 1)
k_hops_shared(const HopArgs a, const uint32_t n_query, const uint32_t per_q, const AttTop<TOP> tp)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr uint32_t Dp = LPR * 16, UN = kUnrollDefault;
    const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const uint32_t q0 = blockIdx.x * QT;
    const uint32_t nq = n_query - q0 < (uint32_t)QT ? n_query - q0 : (uint32_t)QT;     // queries of this tile (the last may be short)
    const uint32_t S = a.max_slots, D = a.D;

    for (uint32_t t = 0; t < nq; t++) {
        const QueryLds L(smem + t * per_q);
        for (uint32_t c = tid; c < 256; c += kBlock) L.u_f[c] = (c < D) ? a.u0[(size_t)(q0 + t) * D + c] : 0.0f;
    }
    __syncthreads();

    for (uint32_t h = 0; h < a.n_hop; h++) {
        const QFmt fm = a.att[h], fb = a.bin;
        const int fv = (int)fb.frac;
        const int maxm = (1 << (fm.iwl + fm.frac)) - 1;

        // query codes Q_bin(u), histogram reset
        for (uint32_t t = 0; t < nq; t++) {
            const QueryLds L(smem + t * per_q);
            for (uint32_t c = tid; c < 256; c += kBlock) {
                L.ku[c] = (short)((c < D) ? qm_code_or_sign(L.u_f[c], fb.iwl, fb.frac) : 0);
                for (uint32_t i = 0; i < (uint32_t)kWaves; i++) L.hist[i * 256 + c] = 0u;
            }
            if (tid == 0) L.misc[0] = 0u;
        }
        __syncthreads();

        // the scan: one pass over the plane for the whole tile
        ScanConst c[QT];
        uint32_t sh = 0;
#pragma unroll
        for (int t = 0; t < QT; t++) {
            const short *ku = QueryLds(smem + ((uint32_t)t < nq ? (uint32_t)t : nq - 1) * per_q).ku;    // spare places: a live query's constants
            if (W7) make_scan_const7(c[t], ku, (lane % LPR) * 16, fv, hop_relu(a, h), fb.iwl + fb.frac == 0);
            else sh = make_scan_const(c[t], ku, (lane % LPR) * 16, fm.iwl + fm.frac, fv, hop_relu(a, h), fb.iwl + fb.frac == 0);
        }
        const uint8_t *kb = (const uint8_t *)a.keys + (size_t)h * a.hop_stride;
        auto retire = [&](uint32_t t, uint32_t r, int v) {          // Qm of the row sum (lib/layer_cuda.cu:135)
            const QueryLds L(smem + t * per_q);
            const int code = v > maxm ? maxm : (v < -maxm ? -maxm : v);
            L.sc[r] = (int8_t)code;
            atomicAdd(&L.hist[wave * 256 + code + 127], 1u);
        };
        if (S < (kWave / LPR) * UN) {                                // below one tile of rows: right, not fast
#pragma unroll
            for (int t = 0; t < QT; t++)
                if ((uint32_t)t < nq)
                    scan_rows_short<LPR>(kb, S, [&](const i32x4 x) { return lane_sum_w<W7>(x, c[t], sh); },
                                         [&](uint32_t r, int v) { retire((uint32_t)t, r, v); }, lane, wave, (uint32_t)kWaves);
        } else {
            scan_rows_shared<LPR, (int)UN, QT, W7>(kb, S, c, sh, nq, retire, lane, wave);
        }
        __syncthreads();

        // the rest of the hop, query by query
        for (uint32_t t = 0; t < nq; t++) {
            const QueryLds L(smem + t * per_q);
            const uint32_t n_live = hist_softmax_survivors(a, h, S, ((size_t)h * n_query + q0 + t) * S, L.hist, L.ptab, L.kplut, L.sc, L.live_row,
                                                           L.live_kp, L.misc, L.red, tid, lane, wave, (uint32_t)kBlock, (uint32_t)kWaves);
            auto kp_of_row = [&](uint32_t r) { return (int)L.kplut[(int)L.sc[r] + 127]; };
            finish_hop<Dp>(a, q0 + t, h, 0u, S, n_live, L.live_row, L.live_kp, kp_of_row, L.ku, L.u_f, L.o_f, tid);
            if constexpr (TOP)
                attended_select(tp, (size_t)(q0 + t) * a.n_hop + h, S, L.hist, L.ptab, L.sc, L.live_row, L.live_kp, L.misc, L.red, tid, lane, wave);
        }
    }
    for (uint32_t t = 0; t < nq; t++) {
        const QueryLds L(smem + t * per_q);
        for (uint32_t c = tid; c < D; c += kBlock) a.u_out[(size_t)(q0 + t) * D + c] = relu_if(L.u_f[c], a.en_non_lin != 0);
    }
}

// Queries per workgroup.  What LDS allows is the frame (about 20 KB per query at 10 000 slots: 8 fill a CU's 160 KiB with one
// workgroup, 4 leave two workgroups per CU); inside it the choice is by measurement (tools/shared_ab.py, 8 192 queries; the
// table and the figures are in DESIGN.md section 5, "Measured, shared plane"): 4 at 10 000 x 128 (2.08 ms; 2: 2.10, 1: 2.45,
// 8: 2.88), 2 at 1 000 x 64 and 200 x 64 (0.227 / 0.163 ms; 4: 0.245 / 0.185).  Between 1 000 and 10 000 slots nothing is
// measured: the line is drawn at 4 096.  A batch too small to give every CU a workgroup takes smaller tiles (not measured
// either: every timing is at 8 192 queries).
// QMANN_SHARED_QT (1, 2, 4, 8) forces a tile size that fits, for that measurement and for the tests.
uint32_t choose_qt(uint32_t n_slots, uint32_t n_query)
{
    uint32_t fit = 8;
    while (fit > 1 && qmann_hops_shared_lds_bytes(n_slots, fit) > kHopLdsLimit) fit >>= 1;
    const uint32_t forced = qm_tuning().shared_qt;
    if (forced) return forced < fit ? forced : fit;
    const uint32_t want = n_slots >= 4096u ? 4u : 2u;
    uint32_t qt = fit < want ? fit : want;
    while (qt > 1 && n_query / qt < qm_cu_count()) qt >>= 1;
    return qt;
}

}  // namespace

extern "C" {

size_t qmann_hops_shared_lds_bytes(uint32_t n_slots, uint32_t queries_per_group)
{
    return (size_t)queries_per_group * qmann_hops_lds_bytes(n_slots);
}

uint32_t qmann_hops_shared_tile(uint32_t n_slots, uint32_t n_query)
{
    if (n_slots == 0 || n_query == 0 || qmann_hops_shared_lds_bytes(n_slots, 1) > kHopLdsLimit) return 0;
    return choose_qt(n_slots, n_query);
}

// tp: null, or the outputs of qmann_hops_shared_top_i8 -- the same launch in its TOP build
static int hops_shared_impl(const qmann_net *net, const int8_t *keys, const int8_t *vals, size_t hop_stride, uint32_t n_slots,
                            const float *u0, float *u_out, const qmann_taps *taps, uint32_t n_query, void *stream,
                            const AttTop<true> *tp)
{
    QmBatched qm_scope;
    // (the steps of hops_host.h's shared-plane prelude, this family's own refusals between them)
    if (const int rc = shared_open(net, keys, vals, u0, u_out)) return rc;
    if (net->attention_mode != QMANN_ATT_FIXED) return QMANN_EUNSUPPORTED;
    HopArgs a;
    if (const int rc = shared_fill(a, net, keys, vals, hop_stride, hop_stride, n_slots, u0, u_out, taps)) return rc;
    if (qmann_hops_shared_lds_bytes(n_slots, 1) > kHopLdsLimit) return QMANN_ERANGE;
    if (int rc; shared_no_queries(n_query, rc)) return rc;
    if (tp && !att_top_args_ok(tp->k, tp->slot, tp->p)) return QMANN_EINVAL;     // behind every refusal of the base call

    const bool w7 = !qm_tuning().no_w7 && all_w7(a, kW7Att);
    const uint32_t qt = choose_qt(n_slots, n_query), per_q = (uint32_t)qmann_hops_lds_bytes(n_slots);
    qm_dispatch<4, 8, 16>(net->dim_emb_pad / 16, [&](auto lpr) {
        qm_dispatch<1, 2, 4, 8>(qt, [&](auto t) {
            qm_dispatch<false, true>(w7, [&](auto w) {
                constexpr int LPR = decltype(lpr)::value, QT = decltype(t)::value;
                constexpr bool W7 = decltype(w)::value;
                if (tp) qm_launch(k_hops_shared<LPR, QT, W7, true>, qm_cdiv(n_query, qt), dim3(kBlock), (size_t)qt * per_q,
                                  (hipStream_t)stream, a, n_query, per_q, *tp);
                else qm_launch(k_hops_shared<LPR, QT, W7>, qm_cdiv(n_query, qt), dim3(kBlock),
                          (size_t)qt * per_q, (hipStream_t)stream, a, n_query, per_q, AttTop<false>{});
            });
        });
    });
    QM_LAUNCH_CHECK();
    return qm_scope.rc();
}

int qmann_hops_shared_i8(const qmann_net *net, const int8_t *keys, const int8_t *vals, size_t hop_stride, uint32_t n_slots,
                         const float *u0, float *u_out, const qmann_taps *taps, uint32_t n_query, void *stream)
{
    return hops_shared_impl(net, keys, vals, hop_stride, n_slots, u0, u_out, taps, n_query, stream, nullptr);
}

int qmann_hops_shared_top_i8(const qmann_net *net, const int8_t *keys, const int8_t *vals, size_t hop_stride, uint32_t n_slots,
                             const float *u0, float *u_out, uint32_t k, uint32_t *top_slot, float *top_p, uint32_t n_query,
                             void *stream)
{
    const AttTop<true> tp{top_slot, top_p, k};
    return hops_shared_impl(net, keys, vals, hop_stride, n_slots, u0, u_out, nullptr, n_query, stream, &tp);
}

}  // extern "C"
