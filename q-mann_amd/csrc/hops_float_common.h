// hops_float_common.h -- stages of float attention (ATTENTION_MODE 1) as functions, for the kernels that run them on a query's
// slice of LDS (batch_hops_shared_float.hip, batch_hops_top_float.hip), and the LDS size of a per-story float launch
// (batch_hops_float.hip and batch_hops_top_float.hip refuse by it).
//
// (COPIES of what k_hops_float carries inline, batch_hops_float.hip -- calling these from there changes that kernel's device
// assembly (tools/device_asm_equal.sh), so it keeps its own text, as k_hops_fixed does beside hist_softmax_survivors; keep the
// two in step: the shared-plane kernel promises k_hops_float's bits.)
#pragma once
#include "hops_common.h"

namespace {

// two's-complement bytes of u and of -u for the 16 columns of a lane (batch_hops_float.hip::DotConst)
struct FloatDotConst {
    uint32_t up[4];
    uint32_t un[4];
};

// from the integer codes of u on its own grid, columns c0 .. c0 + 15
__device__ __forceinline__ void make_float_dot_const(FloatDotConst &c, const int8_t *kuq, uint32_t c0)
{
#pragma unroll
    for (int d = 0; d < 4; d++) {
        uint32_t up = 0, un = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int k = kuq[c0 + 4 * d + i];
            up |= ((uint32_t)k & 0xFFu) << (8 * i);
            un |= ((uint32_t)(-k) & 0xFFu) << (8 * i);
        }
        c.up[d] = up; c.un[d] = un;
    }
}

// The key-only half of batch_hops_float.hip::dot_lane_sum for four sign-magnitude key bytes: 0xFF where the key is negative, and
// the magnitudes
__device__ __forceinline__ void float_key_split(uint32_t w, uint32_t &neg, uint32_t &mag)
{
    neg = __builtin_amdgcn_perm(0u, 0u, w & 0x80808080u);
    mag = w & 0x7F7F7F7Fu;
}
// ... and the query's half: -u where the key is negative, u elsewhere, one dot product
__device__ __forceinline__ int float_dot4(uint32_t neg, uint32_t mag, uint32_t up, uint32_t un, int acc)
{
    const uint32_t uu = (un & neg) | (up & ~neg);
    return __builtin_amdgcn_sdot4((int)mag, (int)uu, acc, false);
}
__device__ __forceinline__ int float_dot_lane_sum(const i32x4 x, const FloatDotConst &c)
{
    int acc = 0;
#pragma unroll
    for (int d = 0; d < 4; d++) {
        uint32_t neg, mag;
        float_key_split((uint32_t)x[d], neg, mag);
        acc = float_dot4(neg, mag, c.up[d], c.un[d], acc);
    }
    return acc;
}

// Four sign-magnitude value bytes as four floats: two's complement in 6 word-wide steps (offset binary first: 128 + m or 128 - m
// never carries into the neighbour byte, "minus zero" included; then the top bits flip), then one sign-extending
// v_cvt_f32_i32 (SDWA byte select) per byte
__device__ __forceinline__ void float_vals4(uint32_t w, float &v0, float &v1, float &v2, float &v3)
{
    const uint32_t t = w & 0x80808080u, one = t >> 7;                    // 0x80 / 0x01 in the negative bytes
    const uint32_t ob = (w ^ 0x80808080u ^ (t - one)) + one;             // 128 + m | (127 - m) + 1
    const uint32_t tc = ob ^ 0x80808080u;
    asm("v_cvt_f32_i32_sdwa %0, sext(%1) dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_0" : "=v"(v0) : "v"(tc));
    asm("v_cvt_f32_i32_sdwa %0, sext(%1) dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_1" : "=v"(v1) : "v"(tc));
    asm("v_cvt_f32_i32_sdwa %0, sext(%1) dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_2" : "=v"(v2) : "v"(tc));
    asm("v_cvt_f32_i32_sdwa %0, sext(%1) dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_3" : "=v"(v3) : "v"(tc));
}

// Softmax per slot of one query (lib/layer_cuda.cu:1895-1916, 1969-2060): the S > 0 integer scores in `sc` become p (float, in
// place); the per-slot taps are written from index `tap_base` on.  `scale`: 2^-(frac_w + frac_u) of the hop; `red`: the query's
// 8 doubles.  Called by the whole 256-thread workgroup behind a barrier after the scan; the caller puts a barrier behind it.
// The thread-to-slot mapping, the reductions and the quotient are k_hops_float's, so that p has its bits.
__device__ __forceinline__ void float_softmax_slots(const HopArgs &a, uint32_t h, uint32_t S, float scale, size_t tap_base, int32_t *sc,
                                                    double *red, uint32_t tid, uint32_t lane, uint32_t wave)
{
    float *pf = (float *)sc;
    const SmCfg smc = sm_cfg(a, h);
    auto slot_x = [&](int sv) { return sm_scaled((float)sv * scale, smc); };   // (float)sv . scale is exact
    float xmax = -INFINITY;
    for (uint32_t r = tid; r < S; r += kBlock) xmax = fmaxf(xmax, slot_x(sc[r]));
    xmax = block_max<float>(xmax, (float *)red, lane, wave);
    double psum = 0.0;
    for (uint32_t r = tid; r < S; r += kBlock) psum += (double)sm_exp(slot_x(sc[r]) - xmax, smc);
    const double total = smc.base == QMANN_SOFTMAX_EXP ? block_sum_double(psum, red, lane, wave)       // (CPU bases: the CPU softmax's serial float total)
                                                       : block_serial_total_f32(S, lane, wave, red, [&](uint32_t r) { return sm_exp(slot_x(sc[r]) - xmax, smc); });
    // stock e^x softmax: e . (1/total) is within an ulp of e / total, and p is not quantised in this
    // mode (tolerance 1e-5); the variants go through the general quotient
    const bool stock = smc.base == QMANN_SOFTMAX_EXP && !smc.shift;
    const double inv_total = 1.0 / total;
    for (uint32_t r = tid; r < S; r += kBlock) {
        const int sv = sc[r];
        const float e = sm_exp(slot_x(sv) - xmax, smc);
        const float p = stock ? (float)((double)e * inv_total) : sm_quot(e, total, smc);
        if (a.tap_codes) a.tap_codes[tap_base + r] = sv;
        if (a.tap_scores) a.tap_scores[tap_base + r] = (float)sv * scale;
        if (a.tap_probs) a.tap_probs[tap_base + r] = p;
        pf[r] = p;
    }
}

// one query's slice of the workgroup's LDS: k_hops_float's use of hops_common.h's carve-up
struct FloatQueryLds {
    float *u_f, *o_f, *part;
    short *ku;
    int8_t *kuq;              // integer codes of u on its own grid (reuses the histogram area)
    double *red;
    int32_t *sc;              // scores, then p (float, in place)
    __device__ __forceinline__ explicit FloatQueryLds(unsigned char *b)
        : u_f((float *)(b + kOffU)), o_f((float *)(b + kOffO)), part((float *)(b + kOffHist + 1024)), ku((short *)(b + kOffKu)),
          kuq((int8_t *)(b + kOffHist)), red((double *)(b + kOffRed)), sc((int32_t *)(b + kOffScores)) {}
};
static_assert(kOffHist + 1024 + kWaves * 256 * 4 <= kOffU, "partial sums must fit the histogram + p-table area");

// host side: the dynamic LDS of a per-story float launch -- the carve-up, then a score (later p) of four bytes per slot
inline size_t float_story_lds_bytes(uint32_t max_slots) { return (size_t)kOffScores + (((size_t)max_slots * 4 + 15) & ~(size_t)15); }

// hops_common.h::scan_rows<LPR, UN, false, kWaves> for a tile of QT queries on one plane: the same tiles, the same two in flight,
// the same moved-back last tile.  retire(t, r, v): row r of query t has sum v; places t >= nq are computed and dropped.
// Needs S >= one tile of rows.
template <int LPR, int UN, int QT, typename Retire>
__device__ __forceinline__ void scan_rows_shared_float(const uint8_t *__restrict__ kb, uint32_t S, const FloatDotConst (&c)[QT], uint32_t nq,
                                                       Retire retire, uint32_t lane, uint32_t wave)
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
            uint32_t neg[4], mag[4];
#pragma unroll
            for (int d = 0; d < 4; d++) float_key_split((uint32_t)x[j][d], neg[d], mag[d]);      // key-only work: once per tile of queries
#pragma unroll
            for (int t = 0; t < QT; t++) {
                int acc = 0;
#pragma unroll
                for (int d = 0; d < 4; d++) acc = float_dot4(neg[d], mag[d], c[t].up[d], c[t].un[d], acc);
                s[t][j] = row_lanes_sum<LPR>(acc);
            }
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
