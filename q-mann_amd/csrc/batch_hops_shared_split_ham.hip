// batch_hops_shared_split_ham.hip -- qmann_hops_shared_split_packed: the shared-plane Hamming hops on packed codes
// (batch_hops_shared_ham.hip: one packed memory, many queries) with the SLOTS cut into slices, as batch_hops_shared_split.hip cuts
// the fixed-point form: for a memory whose int16 scores do not fit LDS (from about 76 000 slots for V1, earlier for V0 with its
// tables) and for a batch of so few questions that most compute units would stand idle.
//
// Why the cut is exact, per mode:
//   V0  ham_common.h::ham_hist_softmax_survivors computes the softmax from nbins = num_bit . D + 1 integer counts of the scores.
//       Counts added across workgroups in any order are the same integers.
//   V1  ham_slot_softmax_survivors takes its maximum and its float / double sums over sc[r] with a fixed thread-to-slot mapping
//       (r = tid, tid + 256, ...).  One 256-thread workgroup per query that calls THE SAME FUNCTION on the same int16 scores
//       performs the same operations in the same order; that `sc` points into the workspace instead of LDS changes no value.
//       Its overflow path parks Q(p) in sc: the workspace is writable, and the row belongs to that workgroup alone.
// So per hop, two launches on the caller's stream, whose order is the only synchronisation (no workgroup waits for another: no
// spin loop, no cooperative launch):
//
//   k_shared_split_scan_ham    grid = query tiles x slices.  A workgroup builds its tile's attention bytes and plane words as
//                              k_hops_shared_ham does (u from the workspace; hop 0: u0), scans rows [s0, s1) of the hop's key
//                              planes (hops_shared_ham.h::scan_planes_shared on a base moved to s0), stores the int16 scores to
//                              the workspace and, for V0, adds its LDS histogram's non-zero bins to the query's global bins.
//   k_shared_split_finish_ham  one workgroup per query.  u_f / ku are rebuilt from the workspace, the merged bins (V0) are copied
//                              to v0_hist, and ham_hist_softmax_survivors / ham_slot_softmax_survivors / finish_hop run as they
//                              are on the query's score row in the workspace: the same functions on the same counts and
//                              scores, hence the same survivors, o and u' as qmann_hops_shared_packed -- by construction.
//
// The scores go to the workspace straight from the scan's retire step, two bytes per row and query.  The 2^x and exp_plan bases
// keep their serial float total in slot order: block_serial_total_f32 then walks the scores in the workspace (global memory, L2
// hits) instead of LDS -- right, but not fast at length.
#include "hops_attended_ham.h"

namespace {

constexpr uint32_t kSplitMaxSlots = 1u << 24;
constexpr uint32_t kSplitUWords = 256;                         // floats of u state per query
constexpr uint32_t kScanUplBytes = 4 * 8 * 8;                  // the scan's LDS per query: u64 [4][8] plane words, then the V0 bins

// the caller's workspace: int16 scores [n_query][pitch], uint32 bins [n_hop][n_query][binsp] (V0 only), float u [n_query][256]
struct HamSplitWs {
    int16_t *scores;
    uint32_t *hist;
    float *u;
    uint32_t pitch;          // n_slots rounded up to 16 (scores per query)
    uint32_t binsp;          // V0: bins rounded up to 4; V1: 0
    uint32_t slice;          // rows per slice, a multiple of 16
    uint32_t n_slices;
};

inline uint32_t split_pitch(uint32_t n_slots) { return (n_slots + 15u) & ~15u; }
inline uint32_t split_binsp(const qmann_net *net) { return (v0_bins_of(net) + 3u) & ~3u; }
inline size_t split_bytes_per_query(const qmann_net *net, uint32_t n_slots)
{
    return (size_t)split_pitch(n_slots) * sizeof(int16_t) + (size_t)net->n_hop * split_binsp(net) * sizeof(uint32_t)
         + (size_t)kSplitUWords * sizeof(float);
}
inline uint32_t lanes_per_key_row(const qmann_net *net) { return net->dim_emb_pad / 64 * net->num_bit * 8 / 16; }

// Queries per workgroup of the scan.  Its LDS is 256 bytes of plane words per query plus the V0 bins (at most 8.2 KB): eight
// queries always fit, so the rule is choose_qt_ham's (batch_hops_shared_ham.hip) without the LDS frame: 4, smaller while the
// tiles are fewer than the compute units.  QMANN_SHARED_QT forces a tile.  NOT MEASURED (no forced tile has been timed).
uint32_t split_qt(uint32_t n_query)
{
    const uint32_t forced = qm_tuning().shared_qt;
    if (forced) return forced;
    uint32_t qt = 4u;
    while (qt > 1 && n_query / qt < qm_cu_count()) qt >>= 1;
    return qt;
}

// The library's own choice cuts no finer than one step of a workgroup's four wavefronts (4 x 4 loads x 64 / LPRK rows), so that
// no wavefront of a slice is without a tile of rows; never below 64 rows.  Measured only through choose_slices below.
inline uint32_t slice_floor(uint32_t lprk)
{
    const uint32_t step = (uint32_t)kWaves * (uint32_t)kUnrollDefault * ((uint32_t)kWave / (lprk ? lprk : 1u));
    return step > 64u ? step : 64u;
}

// rows per slice for `want` slices: a multiple of 16; the slices that result are ceil(n_slots / rows) <= want
inline uint32_t slice_rows(uint32_t n_slots, uint32_t want)
{
    const uint32_t per = (n_slots + want - 1) / want;
    return (per + 15u) & ~15u;
}

// The library's own choice: about two workgroups per compute unit, no slice shorter than slice_floor rows.
// Measured (tools/shared_split_ham_ab.py; DESIGN.md section 5, "Measured, shared plane, split, Hamming"): at 10 000 slots and 1
// to 8 192 queries, and at 200 001 slots with 1 and 64 queries, this choice is the best of {this, 8, 32, 128 slices} or within
// 8 % of it (worst: 200 001 x 256 x 1 bit, one query, 379 slices: 0.239 ms against 0.221 ms with 128).  Other lengths, widths
// and plane counts: NOT MEASURED.
uint32_t choose_slices(uint32_t n_slots, uint32_t n_query, uint32_t lprk)
{
    const uint32_t tiles = qm_cdiv(n_query, split_qt(n_query));
    uint32_t want = qm_cdiv(2u * qm_cu_count(), tiles ? tiles : 1u);
    const uint32_t most = n_slots / slice_floor(lprk);
    if (want > most) want = most;
    return want ? want : 1u;
}

// the slices a call takes: the caller's wish (0: the library's choice), at most ceil(n_slots / 16), and few enough that
// the scan's grid (tiles x slices) stays below 2^31 workgroups
void plan_slices(HamSplitWs &w, uint32_t n_slots, uint32_t n_query, uint32_t qt, uint32_t n_slices, uint32_t lprk)
{
    uint32_t want = n_slices ? n_slices : choose_slices(n_slots, n_query, lprk);
    const uint32_t most = qm_cdiv(n_slots, 16u), tiles = qm_cdiv(n_query, qt);
    if (want > most) want = most;
    const uint32_t grid_cap = 0x7FFFFFFFu / tiles;
    if (want > grid_cap) want = grid_cap;
    w.slice = slice_rows(n_slots, want);
    w.n_slices = qm_cdiv(n_slots, w.slice);
}

// LPRK: lanes per key row (16 LPRK bytes); MODE: kModeV0 / kModeV1; NB: planes; QT: queries per workgroup.  Dynamic LDS:
// QT x (kScanUplBytes + 4 w.binsp) bytes.  a.max_slots = n_slots >= 1
template <int LPRK, int MODE, int NB, int QT>
__global__ void __launch_bounds__(kBlock)
k_shared_split_scan_ham(const HopArgs a, const uint32_t n_query, const uint32_t h, const HamSplitWs w)
{
    static_assert(mode_is_planes(MODE), "packed planes only");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr uint32_t UN = kUnrollDefault;
    const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const uint32_t tile = blockIdx.x / w.n_slices, slice = blockIdx.x % w.n_slices;
    const uint32_t q0 = tile * QT;
    const uint32_t nq = n_query - q0 < (uint32_t)QT ? n_query - q0 : (uint32_t)QT;     // queries of this tile (the last may be short)
    const uint32_t S = a.max_slots, D = a.D;
    const uint32_t nbins = NB * D + 1;
    const uint32_t s0 = slice * w.slice;                                                  // (< S: the host sizes the grid)
    const uint32_t n = S - s0 < w.slice ? S - s0 : w.slice;                               // rows of this slice
    const uint32_t per_q = kScanUplBytes + w.binsp * 4u;
    auto upl_of = [&](uint32_t t) { return (uint64_t *)(smem + t * per_q); };
    auto hist_of = [&](uint32_t t) { return (uint32_t *)(smem + t * per_q + kScanUplBytes); };
    const QFmt fm = a.att[h];

    // per query: sign-magnitude Q_att bytes of the current u (hop 0: u0) and their planes, as k_hops_shared_ham builds them
    for (uint32_t t = 0; t < nq; t++) {
        float uv = 0.0f;
        if (tid < D) uv = h == 0 ? a.u0[(size_t)(q0 + t) * D + tid] : w.u[(size_t)(q0 + t) * kSplitUWords + tid];
        const float ua = relu_if(uv, hop_relu(a, h));                        // what the attention reads
        const uint32_t ubyte = ham_ubyte(ua, fm, tid < D);
        uint64_t *upl = upl_of(t);
#pragma unroll
        for (int i = 0; i < NB; i++) {
            const uint64_t word = __ballot((ubyte >> (7 - i)) & 1u);
            if (lane == 0) upl[wave * 8 + i] = word;               // wavefront w covers columns 64w .. 64w+63
        }
        if (mode_is_v0(MODE))
            for (uint32_t d = tid; d < nbins; d += kBlock) hist_of(t)[d] = 0u;
    }
    __syncthreads();

    const uint8_t *kb = (const uint8_t *)a.keys + (size_t)h * a.key_hop_stride + (size_t)s0 * (LPRK * 16);
    auto retire = [&](uint32_t t, uint32_t r, int v) {              // r: row of the slice
        w.scores[(size_t)(q0 + t) * w.pitch + s0 + r] = (int16_t)v;
        if (mode_is_v0(MODE)) atomicAdd(&hist_of(t)[v], 1u);
    };
    if (n < (kWave / LPRK) * UN) {                                   // a slice below one tile of rows: right, not fast
        for (uint32_t t = 0; t < nq; t++) {
            PlaneConst c;
            make_plane_const<NB>(c, upl_of(t), lane % LPRK, D);
            scan_rows_short<LPRK>(kb, n, [&](const i32x4 x) { return plane_lane_sum<MODE, NB>(x, c); },
                                  [&](uint32_t r, int v) { retire(t, r, v); }, lane, wave, (uint32_t)kWaves);
        }
    } else {
        PlaneQuery c[QT];
        uint64_t valid[2];
        int wgt[2];
#pragma unroll
        for (int t = 0; t < QT; t++) {
            PlaneConst pc;                                           // spare places: a live query's constants
            make_plane_const<NB>(pc, upl_of((uint32_t)t < nq ? (uint32_t)t : nq - 1), lane % LPRK, D);
            c[t].u[0] = pc.u[0]; c[t].u[1] = pc.u[1]; c[t].us[0] = pc.us[0]; c[t].us[1] = pc.us[1];
            if (t == 0) { valid[0] = pc.valid[0]; valid[1] = pc.valid[1]; wgt[0] = pc.wgt[0]; wgt[1] = pc.wgt[1]; }   // (the lane's alone)
        }
        scan_planes_shared<LPRK, (int)UN, QT, MODE, NB>(kb, n, c, valid, wgt, nq, retire, lane, wave);
    }
    // the padding of the score rows (the finish kernel reads 8 scores at a time): the last slice writes it
    if (slice == w.n_slices - 1 && tid < w.pitch - S)
        for (uint32_t t = 0; t < nq; t++) w.scores[(size_t)(q0 + t) * w.pitch + S + tid] = 0;
    if (mode_is_v0(MODE)) {
        __syncthreads();
        // this slice's counts into the query's bins
        for (uint32_t t = 0; t < nq; t++) {
            uint32_t *bins = w.hist + ((size_t)h * n_query + q0 + t) * w.binsp;
            for (uint32_t d = tid; d < nbins; d += kBlock) {
                const uint32_t cnt = hist_of(t)[d];
                if (cnt) atomicAdd(&bins[d], cnt);
            }
        }
    }
}

// DP: padded embedding width; MODE: kModeV0 / kModeV1.  nbins: num_bit . D + 1; scale: the unit of a V1 score, 2^-num_bit.
// Dynamic LDS: kOffScores bytes (HamQueryLds without the score array) plus, for V0, v0_table_bytes(nbins).
// TOP (qmann_hops_shared_split_top_packed): the query's k most attended slots of this hop go to tp.slot / tp.p
// (hops_attended_ham.h, the scores read from the workspace); the other builds take an EMPTY last argument and keep their device
// code.
template <int DP, int MODE, bool TOP = false>
__global__ void __launch_bounds__(kBlock)
k_shared_split_finish_ham(const HopArgs a, const uint32_t n_query, const uint32_t h, const HamSplitWs w, const uint32_t nbins,
                          const float scale, const HamTop<TOP> tp)
{
    static_assert(mode_is_planes(MODE), "packed planes only");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const uint32_t q = blockIdx.x;
    const uint32_t S = a.max_slots, D = a.D;
    const QFmt fb = a.bin;
    const HamQueryLds L(smem, 0u, nbins);                            // no scores in LDS: the V0 tables sit at kOffScores
    int16_t *sc = w.scores + (size_t)q * w.pitch;                    // 16-byte aligned: the pitch and the workspace are
    float *u_g = w.u + (size_t)q * kSplitUWords;

    {
        float uv = 0.0f;
        if (tid < D) uv = h == 0 ? a.u0[(size_t)q * D + tid] : u_g[tid];
        L.u_f[tid] = uv;
        L.ku[tid] = (short)((tid < D) ? qm_code_or_sign(uv, fb.iwl, fb.frac) : 0);
    }
    if (tid == 0) L.misc[0] = 0u;
    if (mode_is_v0(MODE)) {
        const uint32_t *bins = w.hist + ((size_t)h * n_query + q) * w.binsp;       // the merged counts
        for (uint32_t d = tid; d < nbins; d += kBlock) L.v0_hist[d] = bins[d];
    }
    __syncthreads();

    const size_t tap_base = ((size_t)h * n_query + q) * S;
    uint32_t n_live;
    if constexpr (TOP && !mode_is_v0(MODE))                          // (V1: the selection runs inside, while the scores are there)
        n_live = ham_slot_softmax_survivors(a, h, S, scale, tap_base, sc, L.live_row, L.live_kp, L.misc, L.red, tid, lane, wave,
                                            HamSelectV1{tp, (size_t)q * a.n_hop + h, S, sc, ham_att_words(L), tid, lane, wave});
    else
        n_live = mode_is_v0(MODE)
            ? ham_hist_softmax_survivors(a, h, S, nbins, tap_base, sc, L.v0_hist, L.v0_p, L.v0_kp, L.live_row, L.live_kp, L.misc, L.red, tid, lane, wave)
            : ham_slot_softmax_survivors(a, h, S, scale, tap_base, sc, L.live_row, L.live_kp, L.misc, L.red, tid, lane, wave);
    auto kp_of_row = [&](uint32_t r) { return mode_is_v0(MODE) ? (int)L.v0_kp[sc[r]] : (int)sc[r]; };
    finish_hop<DP>(a, q, h, 0u, S, n_live, L.live_row, L.live_kp, kp_of_row, L.ku, L.u_f, L.o_f, tid);
    if constexpr (TOP && mode_is_v0(MODE))
        ham_attended_select_v0(tp, (size_t)q * a.n_hop + h, S, nbins, sc, L.v0_hist, L.v0_p, ham_att_words(L), tid, lane, wave);

    if (h + 1 < a.n_hop) {
        if (tid < D) u_g[tid] = L.u_f[tid];
    } else {
        if (tid < D) a.u_out[(size_t)q * D + tid] = relu_if(L.u_f[tid], a.en_non_lin != 0);
    }
}

// the net's part of the call's checks: what the helpers and the call agree to size or launch for
inline bool split_net_ok(const qmann_net *net)
{
    if (!net || net->n_hop == 0 || net->n_hop > QMANN_MAX_HOP || !packed_form_ok(net)) return false;
    if (net->dim_emb == 0 || net->dim_emb > net->dim_emb_pad) return false;
    if (net->dim_emb_pad != 64 && net->dim_emb_pad != 128 && net->dim_emb_pad != 256) return false;
    for (uint32_t h = 0; h < net->n_hop; h++)
        if (check_ham_hop(net, h)) return false;
    return lanes_per_key_row(net) >= 1;
}

}  // namespace

extern "C" {

size_t qmann_hops_shared_split_packed_ws_bytes(const qmann_net *net, uint32_t n_slots, uint32_t n_query)
{
    if (!split_net_ok(net) || n_slots == 0 || n_slots > kSplitMaxSlots) return 0;
    return (size_t)n_query * split_bytes_per_query(net, n_slots);
}

uint32_t qmann_hops_shared_split_packed_slices(const qmann_net *net, uint32_t n_slots, uint32_t n_query)
{
    if (!split_net_ok(net) || n_slots == 0 || n_slots > kSplitMaxSlots || n_query == 0 || qm_too_many_queries(n_query)) return 0;
    HamSplitWs w{};
    plan_slices(w, n_slots, n_query, split_qt(n_query), 0, lanes_per_key_row(net));
    return w.n_slices;
}

// tp: null, or the outputs of qmann_hops_shared_split_top_packed -- the same launches, the finish kernel in its TOP build
static int hops_shared_split_packed_impl(const qmann_net *net, const uint64_t *key_planes, size_t key_hop_stride, const int8_t *vals,
                                         size_t val_hop_stride, uint32_t n_slots, const float *u0, float *u_out,
                                         const qmann_taps *taps, uint32_t n_query, uint32_t n_slices, void *ws, size_t ws_bytes,
                                         void *stream, const HamTop<true> *tp)
{
    QmBatched qm_scope;
    // (the steps of hops_host.h's shared-plane prelude, this family's own refusals between them; no LDS refusal: the slots are cut)
    if (const int rc = shared_open(net, key_planes, vals, u0, u_out)) return rc;
    if (!packed_form_ok(net)) return QMANN_EUNSUPPORTED;
    const uint32_t nb = net->num_bit, Dp = net->dim_emb_pad;
    if (key_hop_stride != val_hop_stride / Dp * (Dp / 64) * nb * 8) return QMANN_EINVAL;
    if ((uintptr_t)key_planes & 15u) return QMANN_EINVAL;     // 16-byte loads
    HopArgs a;
    if (const int rc = shared_fill(a, net, key_planes, vals, key_hop_stride, val_hop_stride, n_slots, u0, u_out, taps, check_ham_hop)) return rc;
    if (Dp / 64 * nb * 8 < 16) return QMANN_EUNSUPPORTED;     // Dp = 64 with a single plane: a key row is half a 16-byte load
    if (!ws || ((uintptr_t)ws & 15u)) return QMANN_EINVAL;
    if (n_slots > kSplitMaxSlots) return QMANN_ERANGE;
    if (int rc; shared_no_queries(n_query, rc)) return rc;
    if (ws_bytes < (size_t)n_query * split_bytes_per_query(net, n_slots)) return QMANN_EINVAL;
    if (tp && !ham_top_args_ok(tp->k, tp->slot, tp->p)) return QMANN_EINVAL;     // behind every refusal of the base call

    const bool v1 = net->attention_mode == QMANN_ATT_HAMMING_V1;
    const uint32_t nbins = nb * net->dim_emb + 1u;
    HamSplitWs w{};
    w.pitch = split_pitch(n_slots);
    w.binsp = split_binsp(net);
    w.scores = (int16_t *)ws;
    w.hist = (uint32_t *)(w.scores + (size_t)n_query * w.pitch);
    w.u = (float *)(w.hist + (size_t)a.n_hop * n_query * w.binsp);
    const uint32_t qt = split_qt(n_query);
    plan_slices(w, n_slots, n_query, qt, n_slices, lanes_per_key_row(net));

    hipStream_t st = (hipStream_t)stream;
    const size_t scan_lds = (size_t)qt * (kScanUplBytes + (size_t)w.binsp * 4);
    const size_t finish_lds = (size_t)kOffScores + (v1 ? 0 : v0_table_bytes(nbins));
    const float scale = qm_scale_down(1.0f, nb);
    const uint32_t scan_grid = qm_cdiv(n_query, qt) * w.n_slices;
    if (!v1) QM_HIP(hipMemsetAsync(w.hist, 0, (size_t)a.n_hop * n_query * w.binsp * sizeof(uint32_t), st));
    for (uint32_t h = 0; h < a.n_hop; h++) {
        qm_dispatch<64, 128, 256>(Dp, [&](auto dp) {
            constexpr int DP = decltype(dp)::value;
            qm_dispatch<1, 2, 4, 8>(nb, [&](auto n) {
                qm_dispatch<1, 2, 4, 8>(qt, [&](auto t) {
                    constexpr int NB = decltype(n)::value, QT = decltype(t)::value, LPRK = (DP / 64) * NB * 8 / 16;
                    if constexpr (LPRK >= 1) {                  // (no instantiation for the case refused above)
                        if (v1) qm_launch(k_shared_split_scan_ham<LPRK, kModeV1, NB, QT>, scan_grid, dim3(kBlock), scan_lds, st, a, n_query, h, w);
                        else qm_launch(k_shared_split_scan_ham<LPRK, kModeV0, NB, QT>, scan_grid, dim3(kBlock), scan_lds, st, a, n_query, h, w);
                    }
                });
            });
            if (tp) {
                if (v1) qm_launch(k_shared_split_finish_ham<DP, kModeV1, true>, n_query, dim3(kBlock), finish_lds, st, a, n_query, h, w, nbins, scale, *tp);
                else qm_launch(k_shared_split_finish_ham<DP, kModeV0, true>, n_query, dim3(kBlock), finish_lds, st, a, n_query, h, w, nbins, scale, *tp);
            } else {
                if (v1) qm_launch(k_shared_split_finish_ham<DP, kModeV1>, n_query, dim3(kBlock), finish_lds, st, a, n_query, h, w, nbins, scale, HamTop<false>{});
                else qm_launch(k_shared_split_finish_ham<DP, kModeV0>, n_query, dim3(kBlock), finish_lds, st, a, n_query, h, w, nbins, scale, HamTop<false>{});
            }
        });
    }
    QM_LAUNCH_CHECK();
    return qm_scope.rc();
}

int qmann_hops_shared_split_packed(const qmann_net *net, const uint64_t *key_planes, size_t key_hop_stride, const int8_t *vals,
                                   size_t val_hop_stride, uint32_t n_slots, const float *u0, float *u_out, const qmann_taps *taps,
                                   uint32_t n_query, uint32_t n_slices, void *ws, size_t ws_bytes, void *stream)
{
    return hops_shared_split_packed_impl(net, key_planes, key_hop_stride, vals, val_hop_stride, n_slots, u0, u_out, taps, n_query,
                                         n_slices, ws, ws_bytes, stream, nullptr);
}

int qmann_hops_shared_split_top_packed(const qmann_net *net, const uint64_t *key_planes, size_t key_hop_stride, const int8_t *vals,
                                       size_t val_hop_stride, uint32_t n_slots, const float *u0, float *u_out, uint32_t k,
                                       uint32_t *top_slot, float *top_p, uint32_t n_query, uint32_t n_slices, void *ws,
                                       size_t ws_bytes, void *stream)
{
    const HamTop<true> tp{top_slot, top_p, k};
    return hops_shared_split_packed_impl(net, key_planes, key_hop_stride, vals, val_hop_stride, n_slots, u0, u_out, nullptr, n_query,
                                         n_slices, ws, ws_bytes, stream, &tp);
}

}  // extern "C"
