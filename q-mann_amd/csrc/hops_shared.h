// hops_shared.h -- pieces of the shared-plane fixed-point hops (one memory, many queries) that more than one unit calls:
// batch_hops_shared.hip (a workgroup walks the whole memory for its tile of queries) and batch_hops_shared_split.hip (the
// memory cut into slices of slots, a workgroup per tile and slice).  Device pieces only: the calls' host side -- their prelude and
// the LDS cap -- is hops_host.h's and rt.h's, shared with the float and packed units.
#pragma once
#include "hops_host.h"

namespace {

// one query's slice of the workgroup's LDS (hops_common.h's carve-up)
struct QueryLds {
    uint32_t *hist, *live_row, *misc;
    float *ptab, *u_f, *o_f;
    short *ku;
    uint8_t *kplut, *live_kp;
    double *red;
    int8_t *sc;
    __device__ __forceinline__ explicit QueryLds(unsigned char *b)
        : hist((uint32_t *)(b + kOffHist)), live_row((uint32_t *)(b + kOffLiveRow)), misc((uint32_t *)(b + kOffMisc)),
          ptab((float *)(b + kOffPtab)), u_f((float *)(b + kOffU)), o_f((float *)(b + kOffO)), ku((short *)(b + kOffKu)),
          kplut(b + kOffKp), live_kp(b + kOffLiveKp), red((double *)(b + kOffRed)), sc((int8_t *)(b + kOffScores)) {}
};

// hops_common.h::scan_rows for a tile of QT queries on one plane: the same tiles, the same two in flight, the same clamped last
// tile; every loaded row is split once and reduced against each query's constants.  retire(t, r, v): row r of query t has sum v.
// Needs S >= one tile of rows.
template <int LPR, int UN, int QT, bool W7, typename Retire>
__device__ __forceinline__ void scan_rows_shared(const uint8_t *__restrict__ kb, uint32_t S, const ScanConst (&c)[QT], uint32_t sh,
                                                 uint32_t nq, Retire retire, uint32_t lane, uint32_t wave)
{
    constexpr uint32_t RPW = kWave / LPR, TILE = RPW * UN, Dp = LPR * 16, STEP = kWaves * TILE;
    const uint32_t sub = lane / LPR, chunk = lane % LPR;
    const uint32_t n_tiles = (S + TILE - 1) / TILE;
    const uint8_t *lane_base = kb + chunk * 16;
    auto tile_start = [&](uint32_t base) { return base + TILE <= S ? base : S - TILE; };
    auto issue = [&](i32x4 (&x)[UN], uint32_t base) {
        const uint8_t *p = lane_base + (size_t)(tile_start(base) + sub) * Dp;
#pragma unroll
        for (int j = 0; j < UN; j++) x[j] = load16<false>(p + (size_t)j * RPW * Dp);
    };
    auto reduce = [&](const i32x4 (&x)[UN], uint32_t base) {
        int s[QT][UN];
#pragma unroll
        for (int j = 0; j < UN; j++) {
            i32x4 ev, od, sn;
            split_key_row(x[j], ev, od, sn);                       // key-only work: once per tile of queries
#pragma unroll
            for (int t = 0; t < QT; t++) s[t][j] = row_lanes_sum<LPR>(lane_sum_split<W7>(ev, od, sn, c[t], sh));
        }
        const uint32_t start = tile_start(base);
#pragma unroll
        for (int t = 0; t < QT; t++) {
            if ((uint32_t)t >= nq) break;                          // (workgroup-uniform)
#pragma unroll
            for (int j0 = 0; j0 < UN; j0 += LPR) {                 // lane (sub, chunk) retires row j0 + chunk, as scan_rows does
                int v = s[t][j0];
#pragma unroll
                for (int k = 1; k < LPR && j0 + k < UN; k++) v = (chunk == (uint32_t)k) ? s[t][j0 + k] : v;
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

}  // namespace
