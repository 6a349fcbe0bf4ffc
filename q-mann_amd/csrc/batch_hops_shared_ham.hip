// batch_hops_shared_ham.hip -- qmann_hops_shared_packed: the fused hops on PACKED BINARY CODES when every query reads the SAME
// memory (one knowledge base or document, many questions).  It is to k_hops_ham (batch_hops_ham.hip) what k_hops_shared
// (batch_hops_shared.hip) is to k_hops_fixed.
//
// The key planes are packed once for every query (qmann_pack_bitplanes) and are small: 320 KB per hop at 10 000 x 256 with one
// bit, 2.56 MB with eight -- inside an XCD's 4 MiB L2.  One 256-thread workgroup owns QT queries and per hop
//
//   1. builds each query's attention operand exactly as k_hops_ham does (ham_ubyte, the ballots), on that query's LDS slice;
//   2. scans the key planes ONCE for its tile of queries: a 16-byte load (plain, not `nt`: the plane is to stay in L2) is
//      assembled into its two 64-bit words -- and for V1 the key's sign plane is fetched by the quad-permute moves -- once
//      (ham_common.h::plane_key_split), then meets QT queries' plane words (plane_lane_sum_split: the integer operations of
//      plane_lane_sum, so the scores are those of qmann_hops_packed bit for bit);
//   3. runs the rest of the hop per query, one after the other, on that query's slice: int16 scores, the V0 histogram softmax or
//      the per-slot softmax with its threshold shortcut (ham_common.h), survivor list, sparse read-out, linear map, hop update.
//
// Unlike the fixed-point form the tile saves little vector work -- a packed row costs a handful of operations per query --;
// what it shares is one read of the plane from L2 and that load's latency.
// A last tile with fewer than QT queries scans with a live query's constants in the spare places and drops their sums.
#include "hops_attended_ham.h"

namespace {

// (HamQueryLds, PlaneQuery and scan_planes_shared: hops_shared_ham.h, shared with batch_hops_shared_split_ham.hip; the call
// prelude: hops_host.h)

// LPRK: lanes per key row (16 LPRK bytes); DP: padded embedding width; MODE: kModeV0 / kModeV1; NB: planes; QT: queries per
// workgroup.  per_q: bytes of LDS per query (ham_lds_bytes); a.max_slots = n_slots >= 1
// TOP (qmann_hops_shared_top_packed): every query's k most attended slots of the hop go to tp.slot / tp.p (hops_attended_ham.h).
// The TOP builds are instantiations of their own: the others take an EMPTY last argument and keep their device code.
template <int LPRK, int DP, int MODE, int NB, int QT, bool TOP = false>
__global__ void __launch_bounds__(kBlock, 1)
k_hops_shared_ham(const HopArgs a, const uint32_t n_query, const uint32_t per_q, const HamTop<TOP> tp)
{
    static_assert(mode_is_planes(MODE), "packed planes only");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr uint32_t UN = kUnrollDefault;
    const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const uint32_t q0 = blockIdx.x * QT;
    const uint32_t nq = n_query - q0 < (uint32_t)QT ? n_query - q0 : (uint32_t)QT;     // queries of this tile (the last may be short)
    const uint32_t S = a.max_slots, D = a.D;
    const uint32_t nbins = NB * D + 1;
    auto slice = [&](uint32_t t) { return HamQueryLds(smem + t * per_q, S, nbins); };

    for (uint32_t t = 0; t < nq; t++) slice(t).u_f[tid] = (tid < D) ? a.u0[(size_t)(q0 + t) * D + tid] : 0.0f;
    __syncthreads();

    for (uint32_t h = 0; h < a.n_hop; h++) {
        const QFmt fm = a.att[h], fb = a.bin;
        // per query: codes of u (Q_bin for the linear map), sign-magnitude Q_att bytes and their planes for the attention
        for (uint32_t t = 0; t < nq; t++) {
            const HamQueryLds L = slice(t);
            const float uv = L.u_f[tid];
            L.ku[tid] = (short)((tid < D) ? qm_code_or_sign(uv, fb.iwl, fb.frac) : 0);
            const float ua = relu_if(uv, hop_relu(a, h));                    // what the attention reads
            const uint32_t ubyte = ham_ubyte(ua, fm, tid < D);
            L.ub[tid] = (uint8_t)ubyte;
#pragma unroll
            for (int i = 0; i < NB; i++) {
                const uint64_t word = __ballot((ubyte >> (7 - i)) & 1u);
                if (lane == 0) L.upl[wave * 8 + i] = word;         // wavefront w covers columns 64w .. 64w+63
            }
            if (tid == 0) L.misc[0] = 0u;
            if (mode_is_v0(MODE))
                for (uint32_t d = tid; d < nbins; d += kBlock) L.v0_hist[d] = 0u;
        }
        __syncthreads();

        // the scan: one pass over the key planes for the whole tile
        const float scale = MODE == kModeV1 ? qm_scale_down(1.0f, NB) : 1.0f;
        const uint8_t *kb = (const uint8_t *)a.keys + (size_t)h * a.key_hop_stride;
        auto retire = [&](uint32_t t, uint32_t r, int v) {
            const HamQueryLds L = slice(t);
            L.sc[r] = (int16_t)v;
            if (mode_is_v0(MODE)) atomicAdd(&L.v0_hist[v], 1u);
        };
        if (S < (kWave / LPRK) * UN) {                               // below one tile of rows: right, not fast
            for (uint32_t t = 0; t < nq; t++) {
                PlaneConst c;
                make_plane_const<NB>(c, slice(t).upl, lane % LPRK, D);
                scan_rows_short<LPRK>(kb, S, [&](const i32x4 x) { return plane_lane_sum<MODE, NB>(x, c); },
                                      [&](uint32_t r, int v) { retire(t, r, v); }, lane, wave, (uint32_t)kWaves);
            }
        } else {
            PlaneQuery c[QT];
            uint64_t valid[2];
            int wgt[2];
#pragma unroll
            for (int t = 0; t < QT; t++) {
                PlaneConst pc;                                       // spare places: a live query's constants
                make_plane_const<NB>(pc, slice((uint32_t)t < nq ? (uint32_t)t : nq - 1).upl, lane % LPRK, D);
                c[t].u[0] = pc.u[0]; c[t].u[1] = pc.u[1]; c[t].us[0] = pc.us[0]; c[t].us[1] = pc.us[1];
                if (t == 0) { valid[0] = pc.valid[0]; valid[1] = pc.valid[1]; wgt[0] = pc.wgt[0]; wgt[1] = pc.wgt[1]; }   // (the lane's alone)
            }
            scan_planes_shared<LPRK, (int)UN, QT, MODE, NB>(kb, S, c, valid, wgt, nq, retire, lane, wave);
        }
        __syncthreads();

        // the rest of the hop, query by query
        for (uint32_t t = 0; t < nq; t++) {
            const HamQueryLds L = slice(t);
            const size_t tap_base = ((size_t)h * n_query + q0 + t) * S;
            uint32_t n_live;
            if constexpr (TOP && !mode_is_v0(MODE))                  // (V1: the selection runs inside, while the scores are there)
                n_live = ham_slot_softmax_survivors(a, h, S, scale, tap_base, L.sc, L.live_row, L.live_kp, L.misc, L.red, tid, lane, wave,
                                                    HamSelectV1{tp, (size_t)(q0 + t) * a.n_hop + h, S, L.sc, ham_att_words(L), tid, lane, wave});
            else
                n_live = mode_is_v0(MODE)
                    ? ham_hist_softmax_survivors(a, h, S, nbins, tap_base, L.sc, L.v0_hist, L.v0_p, L.v0_kp, L.live_row, L.live_kp, L.misc, L.red, tid, lane, wave)
                    : ham_slot_softmax_survivors(a, h, S, scale, tap_base, L.sc, L.live_row, L.live_kp, L.misc, L.red, tid, lane, wave);
            auto kp_of_row = [&](uint32_t r) { return mode_is_v0(MODE) ? (int)L.v0_kp[L.sc[r]] : (int)L.sc[r]; };
            finish_hop<DP>(a, q0 + t, h, 0u, S, n_live, L.live_row, L.live_kp, kp_of_row, L.ku, L.u_f, L.o_f, tid);
            if constexpr (TOP && mode_is_v0(MODE))
                ham_attended_select_v0(tp, (size_t)(q0 + t) * a.n_hop + h, S, nbins, L.sc, L.v0_hist, L.v0_p, ham_att_words(L), tid, lane, wave);
        }
    }
    for (uint32_t t = 0; t < nq; t++)
        if (tid < D) a.u_out[(size_t)(q0 + t) * D + tid] = relu_if(slice(t).u_f[tid], a.en_non_lin != 0);
}

// Queries per workgroup.  What LDS allows is the frame (about 31 KB per query at 10 000 slots with the V0 tables: 4 fit a CU's
// 160 KiB, 8 do not); QMANN_SHARED_QT (1, 2, 4, 8) forces a tile that fits; a batch too small to give every CU a workgroup takes
// smaller tiles.  Inside that frame: 4.  NOT MEASURED -- no timing of this kernel exists yet (tools/shared_ham_ab.py is the
// tool; DESIGN.md section 5, "Measured, shared plane, Hamming" says what was and was not run).  The choice is by reasoning from the code: the
// tile shares one L2 read of the plane and its latency among its queries, and 4 is the largest tile that fits at 10 000 slots.
uint32_t choose_qt_ham(size_t per_q, uint32_t n_query)
{
    uint32_t fit = 8;
    while (fit > 1 && fit * per_q > kHopLdsLimit) fit >>= 1;
    const uint32_t forced = qm_tuning().shared_qt;
    if (forced) return forced < fit ? forced : fit;
    uint32_t qt = fit < 4u ? fit : 4u;
    while (qt > 1 && n_query / qt < qm_cu_count()) qt >>= 1;
    return qt;
}

}  // namespace

extern "C" {

size_t qmann_hops_shared_packed_lds_bytes(const qmann_net *net, uint32_t n_slots, uint32_t queries_per_group)
{
    if (!net) return 0;
    return (size_t)queries_per_group * ham_lds_bytes(n_slots, v0_bins_of(net));
}

uint32_t qmann_hops_shared_packed_tile(const qmann_net *net, uint32_t n_slots, uint32_t n_query)
{
    if (!net || !packed_form_ok(net) || n_slots == 0 || n_query == 0) return 0;
    const size_t per_q = ham_lds_bytes(n_slots, v0_bins_of(net));
    if (per_q > kHopLdsLimit) return 0;
    return choose_qt_ham(per_q, n_query);
}

// tp: null, or the outputs of qmann_hops_shared_top_packed -- the same launch in its TOP build
static int hops_shared_packed_impl(const qmann_net *net, const uint64_t *key_planes, size_t key_hop_stride, const int8_t *vals,
                                   size_t val_hop_stride, uint32_t n_slots, const float *u0, float *u_out, const qmann_taps *taps,
                                   uint32_t n_query, void *stream, const HamTop<true> *tp)
{
    QmBatched qm_scope;
    // (the steps of hops_host.h's shared-plane prelude, this family's own refusals between them)
    if (const int rc = shared_open(net, key_planes, vals, u0, u_out)) return rc;
    if (!packed_form_ok(net)) return QMANN_EUNSUPPORTED;
    const uint32_t nb = net->num_bit, Dp = net->dim_emb_pad;
    if (key_hop_stride != val_hop_stride / Dp * (Dp / 64) * nb * 8) return QMANN_EINVAL;
    if ((uintptr_t)key_planes & 15u) return QMANN_EINVAL;     // 16-byte loads
    HopArgs a;
    if (const int rc = shared_fill(a, net, key_planes, vals, key_hop_stride, val_hop_stride, n_slots, u0, u_out, taps, check_ham_hop)) return rc;
    const size_t per_q = ham_lds_bytes(n_slots, v0_bins_of(net));
    if (per_q > kHopLdsLimit) return QMANN_ERANGE;
    if (Dp / 64 * nb * 8 < 16) return QMANN_EUNSUPPORTED;     // Dp = 64 with a single plane: a key row is half a 16-byte load
    if (int rc; shared_no_queries(n_query, rc)) return rc;
    if (tp && !ham_top_args_ok(tp->k, tp->slot, tp->p)) return QMANN_EINVAL;     // behind every refusal of the base call

    const bool v1 = net->attention_mode == QMANN_ATT_HAMMING_V1;
    const uint32_t qt = choose_qt_ham(per_q, n_query);
    hipStream_t st = (hipStream_t)stream;
    qm_dispatch<64, 128, 256>(Dp, [&](auto dp) {
        qm_dispatch<1, 2, 4, 8>(nb, [&](auto n) {
            qm_dispatch<1, 2, 4, 8>(qt, [&](auto t) {
                constexpr int DP = decltype(dp)::value, NB = decltype(n)::value, QT = decltype(t)::value, LPRK = (DP / 64) * NB * 8 / 16;
                if constexpr (LPRK >= 1) {                      // (no instantiation for the case refused above)
                    const dim3 grid(qm_cdiv(n_query, qt));
                    const size_t lds = (size_t)qt * per_q;
                    if (tp) {
                        if (v1) qm_launch(k_hops_shared_ham<LPRK, DP, kModeV1, NB, QT, true>, grid, dim3(kBlock), lds, st, a, n_query, (uint32_t)per_q, *tp);
                        else qm_launch(k_hops_shared_ham<LPRK, DP, kModeV0, NB, QT, true>, grid, dim3(kBlock), lds, st, a, n_query, (uint32_t)per_q, *tp);
                    } else {
                        if (v1) qm_launch(k_hops_shared_ham<LPRK, DP, kModeV1, NB, QT>, grid, dim3(kBlock), lds, st, a, n_query, (uint32_t)per_q, HamTop<false>{});
                        else qm_launch(k_hops_shared_ham<LPRK, DP, kModeV0, NB, QT>, grid, dim3(kBlock), lds, st, a, n_query, (uint32_t)per_q, HamTop<false>{});
                    }
                }
            });
        });
    });
    QM_LAUNCH_CHECK();
    return qm_scope.rc();
}

int qmann_hops_shared_packed(const qmann_net *net, const uint64_t *key_planes, size_t key_hop_stride, const int8_t *vals,
                             size_t val_hop_stride, uint32_t n_slots, const float *u0, float *u_out, const qmann_taps *taps,
                             uint32_t n_query, void *stream)
{
    return hops_shared_packed_impl(net, key_planes, key_hop_stride, vals, val_hop_stride, n_slots, u0, u_out, taps, n_query, stream, nullptr);
}

int qmann_hops_shared_top_packed(const qmann_net *net, const uint64_t *key_planes, size_t key_hop_stride, const int8_t *vals,
                                 size_t val_hop_stride, uint32_t n_slots, const float *u0, float *u_out, uint32_t k,
                                 uint32_t *top_slot, float *top_p, uint32_t n_query, void *stream)
{
    const HamTop<true> tp{top_slot, top_p, k};
    return hops_shared_packed_impl(net, key_planes, key_hop_stride, vals, val_hop_stride, n_slots, u0, u_out, nullptr, n_query, stream, &tp);
}

}  // extern "C"
