// hops_shared_ham.h -- pieces of the shared-plane Hamming hops on packed codes (one memory, many queries) that more than one
// unit calls: batch_hops_shared_ham.hip (a workgroup walks the whole memory for its tile of queries) and
// batch_hops_shared_split_ham.hip (the memory cut into slices of slots, a workgroup per tile and slice).
#pragma once
#include "ham_common.h"
#include "hops_host.h"

namespace {

// one query's slice of the workgroup's LDS (the carve-up of k_hops_ham: ham_common.h::ham_lds_bytes)
struct HamQueryLds {
    uint8_t *ub, *live_kp, *v0_kp;
    uint64_t *upl;
    float *u_f, *o_f, *v0_p;
    short *ku;
    uint32_t *live_row, *misc, *v0_hist;
    double *red;
    int16_t *sc;
    __device__ __forceinline__ HamQueryLds(unsigned char *b, uint32_t lds_slots, uint32_t nbins)
        : ub(b + kOffUb), live_kp(b + kOffLiveKp), upl((uint64_t *)(b + kOffUpl)), u_f((float *)(b + kOffU)), o_f((float *)(b + kOffO)),
          ku((short *)(b + kOffKu)), live_row((uint32_t *)(b + kOffLiveRow)), misc((uint32_t *)(b + kOffMisc)),
          red((double *)(b + kOffRed)), sc((int16_t *)(b + kOffScores))
    {
        unsigned char *tab = b + kOffScores + (((size_t)lds_slots * sizeof(int16_t) + 15) & ~(size_t)15);   // V0 tables behind the scores
        v0_hist = (uint32_t *)tab;
        v0_p = (float *)(tab + v0_hist_bytes(nbins));
        v0_kp = tab + 2 * v0_hist_bytes(nbins);
    }
};

// what a query brings to the scan: its plane words and sign planes at this lane's (group, plane) positions
struct PlaneQuery { uint64_t u[2], us[2]; };

// hops_common.h::scan_rows<LPR, UN, .., kWaves> for a tile of QT queries on one plane: the same tiles, the same two in flight, the
// same clamped last tile; the key-only work is done once per loaded row.  retire(t, r, v): row r of query t has sum v.
// Needs S >= one tile of rows.
template <int LPR, int UN, int QT, int MODE, int NB, typename Retire>
__device__ __forceinline__ void scan_planes_shared(const uint8_t *__restrict__ kb, uint32_t S, const PlaneQuery (&c)[QT],
                                                   const uint64_t (&valid)[2], const int (&wgt)[2], uint32_t nq, Retire retire,
                                                   uint32_t lane, uint32_t wave)
{
    constexpr uint32_t RPW = kWave / LPR, TILE = RPW * UN, RowBytes = LPR * 16, STEP = kWaves * TILE;
    const uint32_t sub = lane / LPR, chunk = lane % LPR;
    const uint32_t n_tiles = (S + TILE - 1) / TILE;
    const uint8_t *lane_base = kb + chunk * 16;
    auto tile_start = [&](uint32_t base) { return base + TILE <= S ? base : S - TILE; };
    auto issue = [&](i32x4 (&x)[UN], uint32_t base) {
        const uint8_t *p = lane_base + (size_t)(tile_start(base) + sub) * RowBytes;
#pragma unroll
        for (int j = 0; j < UN; j++) x[j] = load16<false>(p + (size_t)j * RPW * RowBytes);
    };
    auto reduce = [&](const i32x4 (&x)[UN], uint32_t base) {
        int s[QT][UN];
#pragma unroll
        for (int j = 0; j < UN; j++) {
            uint64_t k[2], ks;
            plane_key_split<MODE, NB>(x[j], k, ks);                // key-only work: once per tile of queries
#pragma unroll
            for (int t = 0; t < QT; t++) s[t][j] = row_lanes_sum<LPR>(plane_lane_sum_split<MODE, NB>(k, ks, c[t].u, c[t].us, valid, wgt));
        }
        const uint32_t start = tile_start(base);
#pragma unroll
        for (int t = 0; t < QT; t++) {
            if ((uint32_t)t >= nq) break;                          // (workgroup-uniform)
#pragma unroll
            for (int j0 = 0; j0 < UN; j0 += LPR) {                 // lane (sub, chunk) retires row j0 + chunk, as scan_rows does
                int v = s[t][j0];
#pragma unroll
                for (int i = 1; i < LPR && j0 + i < UN; i++) v = (chunk == (uint32_t)i) ? s[t][j0 + i] : v;
                const uint32_t j = j0 + chunk;
                const uint32_t r = start + j * RPW + sub;
                if (j < (uint32_t)UN && r >= base) retire((uint32_t)t, r, v);
            }
        }
    };

    if (wave >= n_tiles) return;
    i32x4 xa[UN], xb[UN];
    uint32_t base = wave * TILE;
    issue(xa, base);
    for (uint32_t t = wave; t < n_tiles; t += 2 * kWaves) {
        issue(xb, base + STEP);
        reduce(xa, base);
        if (t + kWaves >= n_tiles) break;
        issue(xa, base + 2 * STEP);
        reduce(xb, base + STEP);
        base += 2 * STEP;
    }
}

// bins of the V0 score histogram (0: the net keeps no table of bins)
inline uint32_t v0_bins_of(const qmann_net *net)
{
    return net->attention_mode == QMANN_ATT_HAMMING_V0 ? net->num_bit * net->dim_emb + 1u : 0u;       // (the only mode with a table of bins)
}

// the attention modes and plane counts the packed shared-plane calls take
inline bool packed_form_ok(const qmann_net *net)
{
    if (net->attention_mode != QMANN_ATT_HAMMING_V0 && net->attention_mode != QMANN_ATT_HAMMING_V1) return false;
    const uint32_t nb = net->num_bit;
    return nb == 1 || nb == 2 || nb == 4 || nb == 8;
}

}  // namespace
