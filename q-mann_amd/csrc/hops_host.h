// hops_host.h -- the host side every hop entry point shares (batch_hops.hip, batch_hops_ham.hip): the checks of a hop call,
// HopArgs from a qmann_net, and the choice of kernel for short memories.
#pragma once
#include "hops_lean.h"

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

// A hop call checked (check_hop_call, then the softmax base and the formats) and HopArgs filled from the net -- all but
// max_slots, which the entry point sets with its LDS size.  `family_check`: what an attention family asks of hop h besides,
// between the hop's format check and its linear-map check (batch_hops_ham.hip::check_ham_hop).
// (qmann_hops_i8 has already run check_hop_call, ahead of its taps check and its dispatch by attention mode, to keep the order
// of its return codes; running it again here costs four compares and keeps this function whole for every other caller.)
inline int fill_hop_args(HopArgs &a, const qmann_net *net, const void *keys, const int8_t *vals, size_t key_hop_stride,
                         size_t val_hop_stride, const uint32_t *row_off, const float *u0, float *u_out, const qmann_taps *taps,
                         int (*family_check)(const qmann_net *, uint32_t) = nullptr)
{
    if (const int rc = check_hop_call(net, keys, vals, row_off, u0, u_out)) return rc;
    if (net->softmax_base > QMANN_SOFTMAX_EXP_PLAN) return QMANN_EINVAL;
    if (!qm_fmt8(net->bin) && net->bin.iwl + net->bin.frac != 0) return QMANN_ERANGE;     // (0,0) = BINARY_MODE: u binarised
    for (uint32_t h = 0; h < net->n_hop; h++) {
        if (!qm_fmt8(net->act[h]) || !qm_fmt8(net->w[h]) || !qm_fmt8(net->att[h])) return QMANN_ERANGE;
        if (family_check)
            if (const int rc = family_check(net, h)) return rc;
        if (net->en_lin_map && !net->lin_map[h]) return QMANN_EINVAL;
    }
    a = HopArgs{};
    a.keys = (const int8_t *)keys; a.vals = vals; a.row_off = row_off;
    a.hop_stride = val_hop_stride; a.key_hop_stride = key_hop_stride;
    a.u0 = u0; a.u_out = u_out;
    if (taps) {
        a.tap_codes = taps->score_codes; a.tap_scores = taps->scores; a.tap_probs = taps->probs;
        a.tap_o = taps->o; a.tap_u = taps->u;
    }
    a.rows_total = val_hop_stride ? (uint32_t)(val_hop_stride / net->dim_emb_pad) : (uint32_t)qm_rows_hint;   // (tied hops: the caller's hint, or 0 = unknown)
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

// The kernel of a hop launch by memory size: up to 64 slots the lean kernel (hops_lean.h) where it covers the call -- not for
// packed planes, which have no lean form -- else one wavefront per query (hops_small.h); `general` launches longer memories.
// LPR / LPRK: lanes per value / key row; key_row_bytes: 16 LPRK
template <int MODE, int NB, int LPR, int LPRK, typename General>
inline void launch_hops(const HopArgs &a, uint32_t max_slots, uint32_t n_query, hipStream_t st, General &&general)
{
    constexpr uint32_t key_row_bytes = 16u * LPRK;
    if constexpr (!mode_is_planes(MODE)) {
        if (lean_supported(a, max_slots, key_row_bytes)) { launch_lean<MODE, NB>(a, max_slots, n_query, st); return; }
    }
    if (max_slots <= (uint32_t)kWave) k_hops_small<LPR, LPRK, MODE, NB><<<n_query, kWave, 0, st>>>(a, key_row_bytes);
    else general();
}

}  // namespace
