// batch_hops_shared_split.hip -- qmann_hops_shared_split_i8: the shared-plane hops (batch_hops_shared.hip: one memory, many
// queries) with the SLOTS cut into slices, for the two cases a workgroup that walks the whole memory alone leaves open: a memory
// whose score bytes do not fit LDS, and a batch of so few questions that most compute units would stand idle.
//
// Fixed-point attention (QMANN_ATT_FIXED) only.  The packed Hamming forms have their own unit (batch_hops_shared_split_ham.hip:
// qmann_hops_shared_split_packed); APPX and float attention are follow-ups: their float sums are not covered by the argument below.
//
// Why the cut is exact: a hop's scores are int8 codes, its softmax is computed from a 256-bin histogram of those codes
// (hops_common.h::hist_softmax_survivors) and its read-out is an integer sum over the surviving rows.  Histogram counts are
// integers: added across workgroups in any order they give the same 256 numbers.  So per hop, two launches on the caller's
// stream, whose order is the only synchronisation (no workgroup waits for another: no spin loop, no cooperative launch):
//
//   k_shared_split_scan    grid = query tiles x slices.  A workgroup builds its tile's Q_bin(u) codes and lane constants as
//                          k_hops_shared does, scans rows [s0, s1) of the hop's key plane with the parent's arithmetic
//                          (hops_shared.h::scan_rows_shared on a base moved to s0), writes the score bytes to the workspace
//                          and adds its histogram's non-zero bins to the query's global bins.
//   k_shared_split_finish  one workgroup per query.  The merged bins go into row 0 of an LDS histogram (rows 1 to 3 zero) and
//                          hist_softmax_survivors / finish_hop run as they are, reading the query's score bytes from the
//                          workspace: the same functions on the same counts and bytes, hence the same ptab, kplut, survivors,
//                          o and u' as qmann_hops_shared_i8 -- by construction, not within a tolerance.
//
// The score bytes go to the workspace straight from the scan's retire step, one byte per row and query (a wavefront's 64 bytes
// of a step lie within one 64-row stretch).  Staging a slice in LDS and storing 16 bytes at a time has NOT been measured.
// The 2^x and exp_plan bases keep their serial float total in slot order: block_serial_total_f32 then walks the score bytes in
// the workspace (global memory, L2 hits) instead of LDS -- right, but not fast at length.
#include "hops_attended.h"

namespace {

constexpr uint32_t kSplitMaxSlots = 1u << 24;
constexpr uint32_t kSplitSliceFloor = 256;                     // rows: the library's own choice cuts no finer (NOT MEASURED)
constexpr uint32_t kSplitUWords = 256;                         // floats of u state per query

// the caller's workspace: score bytes [n_query][pitch], uint32 bins [n_hop][n_query][256], float u [n_query][256]
struct SplitWs {
    int8_t *scores;
    uint32_t *hist;
    float *u;
    uint32_t pitch;          // n_slots rounded up to 16
    uint32_t slice;          // rows per slice, a multiple of 16
    uint32_t n_slices;
};

inline uint32_t split_pitch(uint32_t n_slots) { return (n_slots + 15u) & ~15u; }
inline size_t split_bytes_per_query(uint32_t n_hop, uint32_t n_slots)
{
    return (size_t)split_pitch(n_slots) + ((size_t)n_hop + 1) * 256 * 4;
}

// Queries per workgroup of the scan.  LDS is no frame here (a tile needs 4.5 KB per query whatever the length), so the rule is
// choose_qt's (batch_hops_shared.hip) without it: 4 on long memories, 2 on short ones, smaller while the tiles are fewer than
// the compute units.  QMANN_SHARED_QT forces a tile.
uint32_t split_qt(uint32_t n_slots, uint32_t n_query)
{
    const uint32_t forced = qm_tuning().shared_qt;
    if (forced) return forced;
    uint32_t qt = n_slots >= 4096u ? 4u : 2u;
    while (qt > 1 && n_query / qt < qm_cu_count()) qt >>= 1;
    return qt;
}

// rows per slice for `want` slices: a multiple of 16; the slices that result are ceil(n_slots / rows) <= want
inline uint32_t slice_rows(uint32_t n_slots, uint32_t want)
{
    const uint32_t per = (n_slots + want - 1) / want;
    return (per + 15u) & ~15u;
}

// The library's own choice: about two workgroups per compute unit, no slice shorter than kSplitSliceFloor rows.
// NOT MEASURED: tools/shared_split_ab.py fills the table of DESIGN.md section 5, "Measured, shared plane, split".
uint32_t choose_slices(uint32_t n_slots, uint32_t n_query)
{
    const uint32_t tiles = qm_cdiv(n_query, split_qt(n_slots, n_query));
    uint32_t want = qm_cdiv(2u * qm_cu_count(), tiles ? tiles : 1u);
    const uint32_t most = n_slots / kSplitSliceFloor;
    if (want > most) want = most;
    return want ? want : 1u;
}

template <int LPR, int QT, bool W7>
__global__ void __launch_bounds__(kBlock)
k_shared_split_scan(const HopArgs a, const uint32_t n_query, const uint32_t h, const SplitWs w)
{
    __shared__ short ku_s[QT][256];
    __shared__ uint32_t hist_s[QT][kWaves * 256];
    constexpr uint32_t UN = kUnrollDefault;
    const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const uint32_t tile = blockIdx.x / w.n_slices, slice = blockIdx.x % w.n_slices;
    const uint32_t q0 = tile * QT;
    const uint32_t nq = n_query - q0 < (uint32_t)QT ? n_query - q0 : (uint32_t)QT;     // queries of this tile (the last may be short)
    const uint32_t S = a.max_slots, D = a.D;
    const uint32_t s0 = slice * w.slice;                                                  // (< S: the host sizes the grid)
    const uint32_t n = S - s0 < w.slice ? S - s0 : w.slice;                               // rows of this slice
    const QFmt fm = a.att[h], fb = a.bin;
    const int fv = (int)fb.frac;
    const int maxm = (1 << (fm.iwl + fm.frac)) - 1;

    // query codes Q_bin(u) of the tile's current u (hop 0: u0), histogram reset
    for (uint32_t t = 0; t < nq; t++) {
        for (uint32_t c = tid; c < 256; c += kBlock) {
            float u = 0.0f;
            if (c < D) u = h == 0 ? a.u0[(size_t)(q0 + t) * D + c] : w.u[(size_t)(q0 + t) * kSplitUWords + c];
            ku_s[t][c] = (short)((c < D) ? qm_code_or_sign(u, fb.iwl, fb.frac) : 0);
            for (uint32_t i = 0; i < (uint32_t)kWaves; i++) hist_s[t][i * 256 + c] = 0u;
        }
    }
    __syncthreads();

    ScanConst c[QT];
    uint32_t sh = 0;
#pragma unroll
    for (int t = 0; t < QT; t++) {
        const short *ku = ku_s[(uint32_t)t < nq ? (uint32_t)t : nq - 1];                // spare places: a live query's constants
        if (W7) make_scan_const7(c[t], ku, (lane % LPR) * 16, fv, hop_relu(a, h), fb.iwl + fb.frac == 0);
        else sh = make_scan_const(c[t], ku, (lane % LPR) * 16, fm.iwl + fm.frac, fv, hop_relu(a, h), fb.iwl + fb.frac == 0);
    }
    const uint8_t *kb = (const uint8_t *)a.keys + (size_t)h * a.hop_stride + (size_t)s0 * (LPR * 16);
    auto retire = [&](uint32_t t, uint32_t r, int v) {              // r: row of the slice.  Qm of the row sum, as k_hops_shared
        const int code = v > maxm ? maxm : (v < -maxm ? -maxm : v);
        w.scores[(size_t)(q0 + t) * w.pitch + s0 + r] = (int8_t)code;
        atomicAdd(&hist_s[t][wave * 256 + code + 127], 1u);
    };
    if (n < (kWave / LPR) * UN) {                                    // a slice below one tile of rows: right, not fast
#pragma unroll
        for (int t = 0; t < QT; t++)
            if ((uint32_t)t < nq)
                scan_rows_short<LPR>(kb, n, [&](const i32x4 x) { return lane_sum_w<W7>(x, c[t], sh); },
                                     [&](uint32_t r, int v) { retire((uint32_t)t, r, v); }, lane, wave, (uint32_t)kWaves);
    } else {
        scan_rows_shared<LPR, (int)UN, QT, W7>(kb, n, c, sh, nq, retire, lane, wave);
    }
    // the padding bytes of the score rows (the finish kernel reads 16 at a time): the last slice writes them
    if (slice == w.n_slices - 1 && tid < w.pitch - S)
        for (uint32_t t = 0; t < nq; t++) w.scores[(size_t)(q0 + t) * w.pitch + S + tid] = 0;
    __syncthreads();

    // this slice's counts into the query's bins (kBlock = 256 threads: one bin each)
    for (uint32_t t = 0; t < nq; t++) {
        uint32_t cnt = 0;
        for (uint32_t i = 0; i < (uint32_t)kWaves; i++) cnt += hist_s[t][i * 256 + tid];
        if (cnt) atomicAdd(&w.hist[((size_t)h * n_query + q0 + t) * 256 + tid], cnt);
    }
}

// TOP (qmann_hops_shared_split_top_i8): the query's k most attended slots of this hop go to tp.slot / tp.p (hops_attended.h,
// the score bytes read from the workspace); the other builds take an EMPTY last argument and keep their device code.
template <uint32_t Dp, bool TOP = false>
__global__ void __launch_bounds__(kBlock)
k_shared_split_finish(const HopArgs a, const uint32_t n_query, const uint32_t h, const SplitWs w, const AttTop<TOP> tp)
{
    __shared__ __attribute__((aligned(16))) unsigned char smem[kOffScores];
    const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const uint32_t q = blockIdx.x;
    const uint32_t S = a.max_slots, D = a.D;
    const QFmt fb = a.bin;
    const QueryLds L(smem);
    const int8_t *sc = w.scores + (size_t)q * w.pitch;               // 16-byte aligned: the pitch and the workspace are
    float *u_g = w.u + (size_t)q * kSplitUWords;

    for (uint32_t c = tid; c < 256; c += kBlock) {
        float u = 0.0f;
        if (c < D) u = h == 0 ? a.u0[(size_t)q * D + c] : u_g[c];
        L.u_f[c] = u;
        L.ku[c] = (short)((c < D) ? qm_code_or_sign(u, fb.iwl, fb.frac) : 0);
        L.hist[c] = w.hist[((size_t)h * n_query + q) * 256 + c];    // the merged counts: one "wavefront" holds them all
        for (uint32_t i = 1; i < (uint32_t)kWaves; i++) L.hist[i * 256 + c] = 0u;
    }
    if (tid == 0) L.misc[0] = 0u;
    __syncthreads();

    const uint32_t n_live = hist_softmax_survivors(a, h, S, ((size_t)h * n_query + q) * S, L.hist, L.ptab, L.kplut, sc, L.live_row,
                                                   L.live_kp, L.misc, L.red, tid, lane, wave, (uint32_t)kBlock, (uint32_t)kWaves);
    auto kp_of_row = [&](uint32_t r) { return (int)L.kplut[(int)sc[r] + 127]; };
    finish_hop<Dp>(a, q, h, 0u, S, n_live, L.live_row, L.live_kp, kp_of_row, L.ku, L.u_f, L.o_f, tid);
    if constexpr (TOP)
        attended_select(tp, (size_t)q * a.n_hop + h, S, L.hist, L.ptab, sc, L.live_row, L.live_kp, L.misc, L.red, tid, lane, wave);

    if (h + 1 < a.n_hop) {
        for (uint32_t c = tid; c < D; c += kBlock) u_g[c] = L.u_f[c];
    } else {
        for (uint32_t c = tid; c < D; c += kBlock) a.u_out[(size_t)q * D + c] = relu_if(L.u_f[c], a.en_non_lin != 0);
    }
}

// the slices a call takes: the caller's wish (0: the library's choice), at most ceil(n_slots / 16), and few enough that
// the scan's grid (tiles x slices) stays below 2^31 workgroups
void plan_slices(SplitWs &w, uint32_t n_slots, uint32_t n_query, uint32_t qt, uint32_t n_slices)
{
    uint32_t want = n_slices ? n_slices : choose_slices(n_slots, n_query);
    const uint32_t most = qm_cdiv(n_slots, 16u), tiles = qm_cdiv(n_query, qt);
    if (want > most) want = most;
    const uint32_t grid_cap = 0x7FFFFFFFu / tiles;
    if (want > grid_cap) want = grid_cap;
    w.slice = slice_rows(n_slots, want);
    w.n_slices = qm_cdiv(n_slots, w.slice);
}

}  // namespace

extern "C" {

size_t qmann_hops_shared_split_ws_bytes(const qmann_net *net, uint32_t n_slots, uint32_t n_query)
{
    if (!net || net->n_hop == 0 || net->n_hop > QMANN_MAX_HOP) return 0;
    return (size_t)n_query * split_bytes_per_query(net->n_hop, n_slots);
}

uint32_t qmann_hops_shared_split_slices(uint32_t n_slots, uint32_t dim_emb_pad, uint32_t n_query)
{
    (void)dim_emb_pad;                                        // (the rule does not depend on the row width until it is measured)
    if (n_slots == 0 || n_query == 0) return 0;
    SplitWs w{};
    plan_slices(w, n_slots, n_query, split_qt(n_slots, n_query), 0);
    return w.n_slices;
}

// tp: null, or the outputs of qmann_hops_shared_split_top_i8 -- the same launches, the finish kernel in its TOP build
static int hops_shared_split_impl(const qmann_net *net, const int8_t *keys, const int8_t *vals, size_t hop_stride, uint32_t n_slots,
                                  const float *u0, float *u_out, const qmann_taps *taps, uint32_t n_query, uint32_t n_slices,
                                  void *ws, size_t ws_bytes, void *stream, const AttTop<true> *tp)
{
    QmBatched qm_scope;
    // (the steps of hops_host.h's shared-plane prelude, this family's own refusals between them; no LDS refusal: the slots are cut)
    if (const int rc = shared_open(net, keys, vals, u0, u_out)) return rc;
    if (net->attention_mode != QMANN_ATT_FIXED) return QMANN_EUNSUPPORTED;
    HopArgs a;
    if (const int rc = shared_fill(a, net, keys, vals, hop_stride, hop_stride, n_slots, u0, u_out, taps)) return rc;
    if (!ws || ((uintptr_t)ws & 15u)) return QMANN_EINVAL;
    if (n_slots > kSplitMaxSlots) return QMANN_ERANGE;
    if (int rc; shared_no_queries(n_query, rc)) return rc;
    if (ws_bytes < qmann_hops_shared_split_ws_bytes(net, n_slots, n_query)) return QMANN_EINVAL;
    if (tp && !att_top_args_ok(tp->k, tp->slot, tp->p)) return QMANN_EINVAL;     // behind every refusal of the base call

    SplitWs w{};
    w.pitch = split_pitch(n_slots);
    w.scores = (int8_t *)ws;
    w.hist = (uint32_t *)(w.scores + (size_t)n_query * w.pitch);
    w.u = (float *)(w.hist + (size_t)a.n_hop * n_query * 256);
    const uint32_t qt = split_qt(n_slots, n_query);
    plan_slices(w, n_slots, n_query, qt, n_slices);

    hipStream_t st = (hipStream_t)stream;
    const bool w7 = !qm_tuning().no_w7 && all_w7(a, kW7Att);
    QM_HIP(hipMemsetAsync(w.hist, 0, (size_t)a.n_hop * n_query * 256 * sizeof(uint32_t), st));
    for (uint32_t h = 0; h < a.n_hop; h++) {
        qm_dispatch<4, 8, 16>(net->dim_emb_pad / 16, [&](auto lpr) {
            constexpr int LPR = decltype(lpr)::value;
            qm_dispatch<1, 2, 4, 8>(qt, [&](auto t) {
                qm_dispatch<false, true>(w7, [&](auto w7c) {
                    qm_launch(k_shared_split_scan<LPR, decltype(t)::value, decltype(w7c)::value>, qm_cdiv(n_query, qt) * w.n_slices,
                              dim3(kBlock), 0, st, a, n_query, h, w);
                });
            });
            if (tp) qm_launch(k_shared_split_finish<(uint32_t)LPR * 16u, true>, n_query, dim3(kBlock), 0, st, a, n_query, h, w, *tp);
            else qm_launch(k_shared_split_finish<(uint32_t)LPR * 16u>, n_query, dim3(kBlock), 0, st, a, n_query, h, w, AttTop<false>{});
        });
    }
    QM_LAUNCH_CHECK();
    return qm_scope.rc();
}

int qmann_hops_shared_split_i8(const qmann_net *net, const int8_t *keys, const int8_t *vals, size_t hop_stride, uint32_t n_slots,
                               const float *u0, float *u_out, const qmann_taps *taps, uint32_t n_query, uint32_t n_slices, void *ws,
                               size_t ws_bytes, void *stream)
{
    return hops_shared_split_impl(net, keys, vals, hop_stride, n_slots, u0, u_out, taps, n_query, n_slices, ws, ws_bytes, stream, nullptr);
}

int qmann_hops_shared_split_top_i8(const qmann_net *net, const int8_t *keys, const int8_t *vals, size_t hop_stride, uint32_t n_slots,
                                   const float *u0, float *u_out, uint32_t k, uint32_t *top_slot, float *top_p, uint32_t n_query,
                                   uint32_t n_slices, void *ws, size_t ws_bytes, void *stream)
{
    const AttTop<true> tp{top_slot, top_p, k};
    return hops_shared_split_impl(net, keys, vals, hop_stride, n_slots, u0, u_out, nullptr, n_query, n_slices, ws, ws_bytes, stream, &tp);
}

}  // extern "C"
