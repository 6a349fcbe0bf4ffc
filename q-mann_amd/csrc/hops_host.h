// hops_host.h -- the host side every hop entry point shares: the checks of a hop call and HopArgs from a qmann_net (all units),
// the prelude of the shared-plane calls (batch_hops_shared*.hip, batch_hops_top_float.hip), and the choice of kernel for short
// memories (batch_hops.hip, batch_hops_ham.hip).
#pragma once
#include "hops_lean.h"

// qm_hops_i8's attention families on sign-magnitude int8 keys (batch_hops_ham.hip): APPX, Hamming V0 / V1
extern "C" int qmann_hops_appx_impl(const qmann_net *net, const int8_t *keys, const int8_t *vals, size_t hop_stride, const uint32_t *row_off, uint32_t max_slots,
                                    const float *u0, float *u_out, const qmann_taps *taps, uint32_t n_query, void *stream, const QmHopHints &hints);
extern "C" int qmann_hops_hambytes_impl(const qmann_net *net, const int8_t *keys, const int8_t *vals, size_t hop_stride, const uint32_t *row_off, uint32_t max_slots,
                                        const float *u0, float *u_out, const qmann_taps *taps, uint32_t n_query, void *stream, const QmHopHints &hints);

namespace {

// the pointers and sizes of a hop call (the first checks of every entry point, ahead of those of its attention family)
inline int check_hop_call(const qmann_net *net, const void *keys, const int8_t *vals, const uint32_t *row_off, const float *u0,
                          const float *u_out)
{
    if (!net || !keys || !vals || !row_off || !u0 || !u_out) return QMANN_EINVAL;
    if (net->n_hop == 0 || net->n_hop > QMANN_MAX_HOP) return QMANN_EINVAL;
    if (net->dim_emb == 0 || net->dim_emb > net->dim_emb_pad) return QMANN_EINVAL;
    if (net->dim_emb_pad != 64 && net->dim_emb_pad != 128 && net->dim_emb_pad != 256) return QMANN_EUNSUPPORTED;
    return QMANN_OK;
}

// The format half of HopArgs: the softmax base and the formats checked, then every field that is no pointer, stride or size.
// `family_check`: what an attention family asks of hop h besides (batch_hops_ham.hip::check_ham_hop), between the hop's format
// check and its linear-map check.
inline int fill_hop_formats(HopArgs &a, const qmann_net *net, int (*family_check)(const qmann_net *, uint32_t) = nullptr)
{
    if (net->softmax_base > QMANN_SOFTMAX_EXP_PLAN) return QMANN_EINVAL;
    if (!qm_fmt8(net->bin) && net->bin.iwl + net->bin.frac != 0) return QMANN_ERANGE;     // (0,0) = BINARY_MODE: u binarised
    for (uint32_t h = 0; h < net->n_hop; h++) {
        if (!qm_fmt8(net->act[h]) || !qm_fmt8(net->w[h]) || !qm_fmt8(net->att[h])) return QMANN_ERANGE;
        if (family_check)
            if (const int rc = family_check(net, h)) return rc;
        if (net->en_lin_map && !net->lin_map[h]) return QMANN_EINVAL;
    }
    a = HopArgs{};
    a.n_hop = net->n_hop; a.D = net->dim_emb; a.Dp = net->dim_emb_pad;
    a.softmax_base = net->softmax_base; a.en_lin_map = net->en_lin_map;
    a.softmax_shift = net->softmax_shift_based; a.en_att_scale = net->en_att_scale; a.en_non_lin = net->en_non_linearity;
    for (uint32_t h = 0; h < net->n_hop; h++) {
        a.att_scale[h] = net->att_scale[h];
        a.lin_map[h] = net->lin_map[h];
        a.act[h] = qm_qfmt(net->act[h]);
        a.w[h] = qm_qfmt(net->w[h]);
        a.att[h] = qm_qfmt(net->att[h]);
    }
    a.bin = qm_qfmt(net->bin);
    return QMANN_OK;
}

// A hop call checked (check_hop_call, then fill_hop_formats) and HopArgs filled -- all but max_slots, which the entry point sets
// with its LDS size.  `plane_rows`: rt.h::QmHopHints, the plane's size for calls with val_hop_stride = 0.
// (qmann_hops_i8 has already run check_hop_call, ahead of its taps check and its dispatch by attention mode, to keep the order
// of its return codes; running it again here costs four compares and keeps this function whole for every other caller.)
inline int fill_hop_args(HopArgs &a, const qmann_net *net, const void *keys, const int8_t *vals, size_t key_hop_stride,
                         size_t val_hop_stride, const uint32_t *row_off, const float *u0, float *u_out, const qmann_taps *taps,
                         size_t plane_rows = 0, int (*family_check)(const qmann_net *, uint32_t) = nullptr)
{
    if (const int rc = check_hop_call(net, keys, vals, row_off, u0, u_out)) return rc;
    if (const int rc = fill_hop_formats(a, net, family_check)) return rc;
    a.keys = (const int8_t *)keys; a.vals = vals; a.row_off = row_off;
    a.hop_stride = val_hop_stride; a.key_hop_stride = key_hop_stride;
    a.u0 = u0; a.u_out = u_out;
    if (taps) {
        a.tap_codes = taps->score_codes; a.tap_scores = taps->scores; a.tap_probs = taps->probs;
        a.tap_o = taps->o; a.tap_u = taps->u;
    }
    a.rows_total = (uint32_t)(val_hop_stride ? val_hop_stride / net->dim_emb_pad : plane_rows);   // (tied hops: the caller's hint, or 0 = unknown)
    return QMANN_OK;
}

// ---- the shared-plane calls (one memory, every query reads it: n_slots in place of row_off and max_slots) ---------------------
// The steps all eleven entry points take, in this order; a family's own refusals stay in its entry point, between them:
//   shared_open        the pointers and sizes (check_hop_call)
//                        [fixed-point: the attention mode; packed: packed_form_ok, key stride and alignment]
//   shared_fill        fill_hop_args [float: the attention mode], then n_slots == 0, then HopArgs' row_off / max_slots / rows_total
//                        [LDS size (not the split calls); packed: LPRK < 1; split: workspace pointer, kSplitMaxSlots]
//   shared_no_queries  n_query == 0 is "OK, launch nothing"; too many queries
//                        [split: workspace bytes; top: the top arguments, last]
// The order is the order of the calls' return codes: tests/test_shared_call_refusals.py pins it.
constexpr uint32_t no_row_off = 0;                             // these calls have no row_off: the shared checks want a non-null one

inline int shared_open(const qmann_net *net, const void *keys, const int8_t *vals, const float *u0, const float *u_out)
{
    return check_hop_call(net, keys, vals, &no_row_off, u0, u_out);
}

// `mode_ok`: the float calls' attention-mode check, which they pass in because its refusal comes BEHIND the formats and ahead of
// n_slots (the fixed-point and packed calls refuse their mode themselves, ahead of this step: both orders are documented)
inline int shared_fill(HopArgs &a, const qmann_net *net, const void *keys, const int8_t *vals, size_t key_hop_stride, size_t val_hop_stride,
                       uint32_t n_slots, const float *u0, float *u_out, const qmann_taps *taps,
                       int (*family_check)(const qmann_net *, uint32_t) = nullptr, bool mode_ok = true)
{
    if (const int rc = fill_hop_args(a, net, keys, vals, key_hop_stride, val_hop_stride, &no_row_off, u0, u_out, taps, 0, family_check)) return rc;
    if (!mode_ok) return QMANN_EUNSUPPORTED;
    if (n_slots == 0) return QMANN_EINVAL;
    a.row_off = nullptr;
    a.max_slots = a.rows_total = n_slots;
    return QMANN_OK;
}

// true: the call ends here with `rc`
inline bool shared_no_queries(uint32_t n_query, int &rc)
{
    rc = n_query == 0 ? QMANN_OK : QMANN_ERANGE;
    return n_query == 0 || qm_too_many_queries(n_query);
}

// May the fixed-point hop kernel end a key scan early (batch_hops.hip, step 1b and ScanStop)?  Only the e^x softmax without the
// shift, only without taps (they need every score), and only where for at least one hop the bound can be reached inside the
// memory at all: a hop's scan sums e^(x_r - Xb) <= 1 per row and stops at 2^frac (1 + 2^-6), so even a memory of all-zero scores
// (e^x = 1) needs 2^frac . e^Xb . (1 + 2^-6) rows.  Xb as the kernel forms it (one float product for the scale layer), the rest
// in double; a NaN scale compares false.  Q2.5 wants 1 720 rows, Q5.2 4 e^31.75: such a launch keeps the plain kernel.
// The kernel's credit for unread rows (ScanStop: each at least f = e^(Xmin - Xb)) leaves this decision as it is: a memory of all-zero
// scores read to the end reaches that bound within max_slots exactly when max_slots . e^(-Xb) >= thr, the test below -- the
// floor only moves the row at which a reachable bound is reached, or (S f >= thr) settles the hop unread, and S f <= S e^(-Xb).
inline bool scan_stop_gate(const HopArgs &a, uint32_t max_slots)
{
    if (a.tap_codes || a.tap_scores || a.tap_probs || a.tap_o || a.tap_u) return false;
    if (a.softmax_base != QMANN_SOFTMAX_EXP || a.softmax_shift != 0) return false;
    for (uint32_t h = 0; h < a.n_hop; h++) {
        const QFmt fm = a.att[h], fa = a.act[h];
        const float top = qm_scale_down((float)((1u << (fm.iwl + fm.frac)) - 1u), fm.frac);
        const float pos = a.en_att_scale ? top * a.att_scale[h] : top, neg = a.en_att_scale ? -top * a.att_scale[h] : -top;
        const double xb = pos > neg ? (double)pos : (double)neg;                 // (NaN: neg, and the compare below is false)
        const double rows = (double)(1u << fa.frac) * exp(xb) * (1.0 + 0.015625);
        if (rows <= (double)max_slots) return true;
    }
    return false;
}

// The ONE decision of a hop launch: the form it takes.  No HIP call, no state but qm_tuning(): asking twice gives the same
// answer, which is how the host model knows ahead of the launch that a batch will be split (batch_hops.hip::qm_hops_will_split).
// Up to 64 slots the lean kernels where they cover the call -- not for packed planes, which have no lean form -- else one
// wavefront per query; longer memories: hops_mid.h where it covers them, else the family's general kernel.
// `every_prob`: the call wants every slot's probability without a tap in HopArgs (attended slots per story, qmann_hops_top_i8):
// it plans as a call with taps does -- one wavefront per query up to 64 slots, the general kernel beyond.
inline HopPlan hop_plan(const HopArgs &a, int mode, uint32_t key_row_bytes, uint32_t max_slots, uint32_t n_query, bool every_prob = false)
{
    // (known from the plane size; tied hops without a hint carry none and take the bAbI guess: stories short next to their cap)
    const uint32_t mean_slots = (a.rows_total && n_query) ? a.rows_total / n_query : max_slots / 8u;
    auto plan = [&](HopForm f) { return HopPlan{f, mean_slots}; };
    if (every_prob || mode_is_planes(mode) || !lean_supported(a, max_slots, key_row_bytes)) {
        if (max_slots <= (uint32_t)kWave) return plan(HopForm::Small);
        return plan(mode == kModeFixed && !every_prob && mid_supported(a, max_slots) ? HopForm::Mid : HopForm::General);    // hops_mid.h: 65 .. 1 024 slots at bAbI width
    }
    // Small batches keep one story per wavefront: the GPU holds 6 144 wavefronts at once, so up to a few thousand stories each has
    // one of its own and the batch takes ONE story's latency, where four stories per wavefront take their linear maps in turn
    // (task-1 forward, interleaved: 256 stories 34.8 -> 27.2 us, 1 024 36.8 -> 29.3, 4 096 40.4 -> 38.9, 8 192 53.7 -> 50.0,
    // 16 384 72.1 <- 75.2: the quad form from there on; 64-story serving batches replayed from a graph 39.2 -> 31.1 us)
    if (!quad_supported(a, mode, max_slots, n_query) || n_query <= qm_tuning().quad_min_queries) return plan(HopForm::Lean);
    if (max_slots <= kQuadSlots) return plan(HopForm::Quad);
    // A batch is split only where short stories can be many: mean length within the short form's 16 rows.  A batch of long
    // stories -- the |mem| = 50 shape of BASELINE's metric -- goes whole through the four-chunk form (QMANN_NO_QUAD_LONG: the lean kernel).
    if (mean_slots > kQuadSlots)
        // (fixed-point scores only: the form is 2 % ahead of the lean kernel at 50 rows -- 7 % fewer vector instructions per query,
        // four wavefronts per SIMD against six -- which does not pay for ten more instantiations in the Hamming modes)
        return plan(mode == kModeFixed && !qm_tuning().no_quad_long ? HopForm::QuadLong : HopForm::Lean);
    return plan(HopForm::Split);
}

// One hop launch by its plan (the cases in the order their kernels have always been instantiated: tools/device_asm_equal.sh).
// `general(form)` launches long memories: HopForm::General, or Mid -- planned for fixed-point scores only, whose entry point
// has hops_mid.h.  LPR / LPRK: lanes per value / key row; key_row_bytes: 16 LPRK
template <int MODE, int NB, int LPR, int LPRK, typename General>
inline void launch_hops(const HopArgs &a, uint32_t max_slots, uint32_t n_query, hipStream_t st, const QmHopHints &hints, General &&general)
{
    constexpr uint32_t key_row_bytes = 16u * LPRK;
    const HopPlan plan = hop_plan(a, MODE, key_row_bytes, max_slots, n_query, hints.top_on);
    switch (plan.form) {
    case HopForm::Lean: case HopForm::Quad: case HopForm::QuadLong: case HopForm::Split:
        if constexpr (!mode_is_planes(MODE)) launch_lean<MODE, NB>(a, plan, max_slots, n_query, st, hints.split_ws);
        break;
    case HopForm::Small:
        if constexpr (!mode_is_planes(MODE)) {              // (attended slots per story: int8 keys only)
            if (hints.top_on) {
                k_hops_small<LPR, LPRK, MODE, NB, true><<<n_query, kWave, 0, st>>>(a, key_row_bytes, StoryTop<true>{hints.top_slot, hints.top_p, hints.top_k});
                break;
            }
        }
        k_hops_small<LPR, LPRK, MODE, NB><<<n_query, kWave, 0, st>>>(a, key_row_bytes, StoryTop<false>{});
        break;
    case HopForm::Mid: case HopForm::General: general(plan.form); break;
    }
}

}  // namespace
