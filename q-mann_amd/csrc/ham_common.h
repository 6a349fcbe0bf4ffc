// ham_common.h -- lane arithmetic of the Hamming-family attention scores, shared by the streaming
// kernel (batch_hops_ham.hip) and the one-wavefront kernel for short memories (hops_small.h).
// See batch_hops_ham.hip for what each mode computes and the reference lines it follows.
#pragma once
#include "hops_common.h"

namespace {

// kModeV0 / kModeV1 read packed bit planes; kModeV0Bytes / kModeV1Bytes compute the same scores straight from
// the sign-magnitude int8 memories (no packing pass; the choice for short memories and for num_bit = 8, where
// planes are no smaller than bytes).  3 = kModeFixed (hops_small.h).
// kModeAppxMq: APPX whose hops differ in operand grids (mixed quantisation, see "APPX under EN_MQ" below); kModeAppx is the
// same kernel with every hop of kind kHamSame compiled in.
enum { kModeAppx = 0, kModeV0 = 1, kModeV1 = 2, kModeV0Bytes = 4, kModeV1Bytes = 5, kModeAppxMq = 6 };
constexpr bool mode_is_appx(int m) { return m == kModeAppx || m == kModeAppxMq; }
constexpr bool mode_is_v0(int m) { return m == kModeV0 || m == kModeV0Bytes; }
constexpr bool mode_is_planes(int m) { return m == kModeV0 || m == kModeV1; }

// V0 scores are small counts (0 .. num_bit . D <= 2048): the softmax is evaluated once per distinct
// count through a histogram (as the fixed-point kernel does per code).  The tables (hist u32, p float,
// Q(p) u8, each nbins = num_bit . D + 1 entries) sit behind the score array.
__host__ __device__ inline uint32_t v0_hist_bytes(uint32_t nbins) { return ((nbins * 4 + 15) / 16) * 16; }
__host__ __device__ inline uint32_t v0_table_bytes(uint32_t nbins) { return 2 * v0_hist_bytes(nbins) + ((nbins + 15) / 16) * 16; }

// LDS of the streaming kernels of the family (batch_hops_ham.hip, batch_hops_shared_ham.hip): hops_common.h's carve-up with the
// attention operand in the histogram area, int16 scores, and the V0 tables behind them
constexpr uint32_t kOffUb = kOffHist;                 // u8  [256]  sign-magnitude bytes of Q_att(u)   (reuses the
constexpr uint32_t kOffUpl = kOffHist + 256;          // u64 [4][8] bit-planes of u                    histogram area)
static_assert(kOffUpl % 8 == 0 && kOffUpl + 4 * 8 * 8 <= kOffPtab, "u planes must fit the histogram area");
inline size_t ham_lds_bytes(uint32_t max_slots, uint32_t v0_bins)
{
    return (size_t)kOffScores + (((size_t)max_slots * 2 + 15) & ~(size_t)15) + (v0_bins ? v0_table_bytes(v0_bins) : 0);
}

// what the Hamming family asks of a hop besides (hops_host.h::fill_hop_args): attention word length 7 with an integer bit
inline int check_ham_hop(const qmann_net *net, uint32_t h)
{
    return (net->att[h].iwl + net->att[h].frac != 7 || net->att[h].iwl < 1) ? QMANN_EUNSUPPORTED : QMANN_OK;
}

// ---- APPX: 4 key bytes against 4 query bytes -------------------------------------------------
struct AppxConst {
    uint32_t um[4];   // |u| bytes
    uint32_t u127[4]; // |u| + 127 per byte (<= 254): what a sign-differing byte is replaced by in the same-sign sum
    uint32_t nb[4];   // 128 - |u| per byte
    uint32_t us[4];   // 0x80 where u < 0
    uint32_t m7[4];   // 0x7F in real columns, 0 in padding
    uint32_t m8[4];   // 0x80 in real columns, 0 in padding
    int bias;         // 127 . (16 - padding columns of this lane): the same-sign terms' constant part
};

// APPX under EN_MQ (mixed quantisation, MemN2N/MemN2N.c:748-754: weight formats Q(iwl+1.frac-1), Q(iwl.frac), Q(iwl-1.frac+1)
// for hops 0, 1, 2 while the attention format stays Q(iwl.frac)).  The reference re-encodes both operands of a column as
// Q(iwl_att, 31 - iwl_att) sign-magnitude WORDS (lib/layer_cuda.cu:355-420) and only bits 30..24 of the adjusted words are
// compared, but the adjustment (common magnitude removed / moved onto the larger operand) runs on all 31 bits.  What a byte per
// operand can carry exactly, by the hop's KIND (qfmt.h::ham_hop_kind):
//   kHamSame    both operand grids lie inside the attention grid: the word is byte << 24 (the case of the rounds before).
//   kHamCoarse  both grids are at least one fractional bit coarser, wider range: on-grid codes are even, so the odd code 127 is
//               free and stands for the SATURATED word 0x7FFFFFFF (Q_att clamps to 127 by itself).  Its low 24 ones never
//               matter -- same sign: 0x7FFFFFFF - (b << 24) has top bits 127 - b; opposite: + (b << 24) carries nothing up --
//               except when BOTH operands are saturated with opposite signs: 0x7FFFFFFF + 0x7FFFFFFF = 0xFFFFFFFE, top bits
//               carry + 127 where 127 + 127 gives carry + 126.  `km & um & 1` is that case (every other code is even).
//   kHamFine    the key grid is one fractional bit finer and at least one integer bit narrower; u lies inside the attention
//               grid.  The key byte is the key's OWN code k8 (units 2^-(frac+1), <= 127), u's word is (2 u7) << 23:
//                 opposite sign  top bits of k8 + 2 u7 are (k8 >> 1) + u7, carry and comparison likewise: the byte
//                                arithmetic on kh = k8 >> 1;
//                 same sign      |k8 - 2 u7| >> 1 = |kh - u7| - [k8 odd and kh < u7].
// A value of exactly -2^iwl_att (reachable on a wider grid only) is "minus zero" in the reference's word: byte 0x80
// (ham_ubyte below; the embedding kernels' key bytes follow the same rule).
__device__ __forceinline__ uint32_t ham_kind_of(const HopArgs &a, uint32_t h) { return (a.ham_kinds >> (2u * h)) & 3u; }

// operations per 4 columns in the compiled loop: kHamSame 12 (the boolean pairs fuse into v_bitop3_b32; round 1: 15 + 2 per
// row, round 2: 13), kHamCoarse 13, kHamFine 17.  Padding columns are forced to "same sign, both magnitudes 0" by the masks
// (a term of exactly 127), which `bias` leaves out.
template <int KIND>
__device__ __forceinline__ int appx_lane_sum_k(const i32x4 x, const AppxConst &c)
{
    int dot = 0;
    uint32_t sad = 0, fix = 0;
#pragma unroll
    for (int d = 0; d < 4; d++) {
        const uint32_t w = (uint32_t)x[d];
        const uint32_t km = KIND == kHamFine ? ((w >> 1) & ((c.m7[d] >> 1) & 0x3F3F3F3Fu)) : (w & c.m7[d]);
        const uint32_t sd = (w ^ c.us[d]) & c.m8[d];                        // signs differ
        const uint32_t dmask = __builtin_amdgcn_perm(0u, 0u, sd);           // 0xFF in those bytes
        // same sign: 127 - |ka - kb|; `bias` holds a 127 for every real column.  Where the signs differ the key byte is
        // replaced by |u| + 127: a difference of exactly 127, which gives that column's 127 back inside the same v_sad_u8
        // (round 2 spent a v_dot4 on counting those columns)
        sad = __builtin_amdgcn_sad_u8((km & ~dmask) | (c.u127[d] & dmask), c.um[d], sad);
        // opposite sign: +-(127 - ((ka + kb) & 127)); per byte ka + kb <= 254 (+ 1 for two saturated operands), no carry across bytes
        const uint32_t s4 = KIND == kHamCoarse ? km + c.um[d] + (km & c.um[d] & 0x01010101u) : km + c.um[d];   // bit 7 of a byte = carry out of 7 bits
        const uint32_t val = ~s4 & (dmask & 0x7F7F7F7Fu);
        const uint32_t ge = km + c.nb[d];                                   // bit 7: |k| + 128 - |u| >= 128, i.e. |k| >= |u| (<= 255: no carry)
        const uint32_t lneg = (w & ge) | (c.us[d] & ~ge);                   // bit 7: sign of the larger operand
        const uint32_t neg = ((s4 & lneg) | ~s4) & 0x80808080u;             // negative unless carry and larger > 0
        const uint32_t sg = __builtin_amdgcn_perm(0x01010101u, 0x01010101u, neg);
        dot = __builtin_amdgcn_sdot4((int)val, (int)sg, dot, false);
        if (KIND == kHamFine) {
            // same sign, odd key code, kh < u7: the halved difference is one less than |kh - u7| (128 per such column)
            const uint32_t odd7 = (w << 7) & c.m8[d];                       // bit 7 of a byte = bit 0 of that key byte
            fix = __builtin_amdgcn_sad_u8(odd7 & ~ge & ~sd, 0u, fix);
        }
    }
    return dot + c.bias - (int)sad + (int)(fix >> 7);
}
__device__ __forceinline__ int appx_lane_sum(const i32x4 x, const AppxConst &c) { return appx_lane_sum_k<kHamSame>(x, c); }

// sign-magnitude byte of the attention operand u of a Hamming-family mode: magnitude Q_att (clamped at 127, truncated toward
// zero), sign from the VALUE; exactly -2^iwl is the reference's "minus zero" (its operand word is Q(iwl, 31 - iwl):
// lib/layer_cuda.h:233-253 -- the value is not below the macro's float limit, converts to INT32_MIN, whose sign-magnitude
// word has magnitude 0).  Only reachable when u's own grid is wider than the attention grid.
__device__ __forceinline__ uint32_t ham_ubyte(float ua, QFmt fm, bool real)
{
    if (!real) return 0u;
    const int kc = qm_code(ua, fm.iwl, fm.frac);
    const uint32_t mag = ua == -(float)(1u << fm.iwl) ? 0u : (uint32_t)(kc < 0 ? -kc : kc);
    return mag | (!(ua >= 0.0f) ? 0x80u : 0u);
}

// Final quantisation of a mode-3 score, Q(iwl, 31-iwl) (lib/layer_cuda.cu:2515): saturation at +-2^iwl -- except that a sum of
// EXACTLY -2^iwl is not below the macro's float limit (the limit (2^31 - 1) / 2^(31-iwl) rounds to 2^iwl itself), converts to
// INT32_MIN, and the sign-magnitude word of INT32_MIN is "minus zero": the reference returns 0 there
// (lib/layer_cuda.h:233-253; +2^iwl converts to INT32_MAX and stays 2^iwl).  v and lim in units of 2^-10.
__device__ __forceinline__ int appx_clamp(int v, int lim)
{
    return v > lim ? lim : (v < -lim ? -lim : (v == -lim ? 0 : v));
}

// ---- V0 / V1: two 64-bit plane words per lane -------------------------------------------------
struct PlaneConst {
    uint64_t u[2];      // query plane words at this lane's (group, plane) positions
    uint64_t valid[2];  // real-column mask of the word's group
    uint64_t us[2];     // query SIGN plane of the word's group
    int wgt[2];         // V1 weight 2^(n-1-i) of the word's plane (0 for the sign plane)
};

template <int MODE, int NB>
__device__ __forceinline__ int plane_lane_sum(const i32x4 x, const PlaneConst &c)
{
    uint64_t k[2];
    k[0] = (uint64_t)(uint32_t)x[0] | ((uint64_t)(uint32_t)x[1] << 32);
    k[1] = (uint64_t)(uint32_t)x[2] | ((uint64_t)(uint32_t)x[3] << 32);
    if (MODE == kModeV0) {
        return __popcll(~(k[0] ^ c.u[0]) & c.valid[0]) + __popcll(~(k[1] ^ c.u[1]) & c.valid[1]);
    }
    // V1: the key's sign plane of each word's group sits in the lane that holds plane 0 of that
    // group: this lane (NB <= 2), the even lane of the pair (NB == 4) or the first lane of the
    // quad (NB == 8) -- fetched with quad-permute DPP moves
    uint64_t ks[2];
    if (NB == 1) {
        return 0;                                   // no magnitude planes: every weight is zero
    } else if (NB == 2) {
        ks[0] = k[0]; ks[1] = k[0];
    } else {
        constexpr int ctrl = (NB == 4) ? 0xA0 /* quad_perm [0,0,2,2] */ : 0x00 /* [0,0,0,0] */;
        const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, x[0], ctrl, 0xF, 0xF, true);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, x[1], ctrl, 0xF, 0xF, true);
        ks[0] = (uint64_t)lo | ((uint64_t)hi << 32);
        ks[1] = ks[0];
    }
    int acc = 0;
#pragma unroll
    for (int t = 0; t < 2; t++) {
        const uint64_t eq = ~(k[t] ^ c.u[t]);
        const uint64_t sdiff = (ks[t] ^ c.us[t]) & c.valid[t];
        const uint64_t ssame = ~(ks[t] ^ c.us[t]) & c.valid[t];
        acc += c.wgt[t] * (__popcll(eq & ssame) - __popcll(eq & sdiff));
    }
    return acc;
}


// ---- V0 / V1 on int8 keys ---------------------------------------------------------------------------
// The top num_bit bits of a sign-magnitude byte ARE planes 0..num_bit-1 of that column, so
//   V0 = sum over real columns of (n - popcount((k ^ u) & top_n))                      (lib/common.c:223-246)
//   V1 = sum over real columns of sgn.sgn.( (2^(n-1) - 1) - (((|k| ^ |u|) >> (8 - n)) & (2^(n-1) - 1)) )
//        in units of 2^-n: the weights 2^(n-1-i) of bits i = 1..n-1 add up to that difference (lib/common.c:249-312)
struct HamByteConst {
    uint32_t ub[4];   // sign-magnitude bytes of Q_att(u) for this lane's 16 columns
    uint32_t m[4];    // V0: top-n-bit mask, V1: low (n-1)-bit mask; 0 in padding columns
    int bias;         // V0: n . (real columns of this lane)
};
template <int MODE, int NB>
__device__ __forceinline__ void make_hambyte_const(HamByteConst &c, const uint8_t *ub, uint32_t c0, uint32_t D)
{
    constexpr uint32_t pat = mode_is_v0(MODE) ? ((0xFF00u >> NB) & 0xFFu) : ((1u << (NB - 1)) - 1u);
#pragma unroll
    for (int d = 0; d < 4; d++) {
        c.ub[d] = *(const uint32_t *)(ub + c0 + 4 * d);
        uint32_t vm = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) vm |= (c0 + 4 * d + i < D ? pat : 0u) << (8 * i);
        c.m[d] = vm;
    }
    c.bias = NB * (int)(D >= c0 + 16 ? 16u : (D > c0 ? D - c0 : 0u));
}
template <int MODE, int NB>
__device__ __forceinline__ int hambyte_lane_sum(const i32x4 x, const HamByteConst &c)
{
    if (mode_is_v0(MODE)) {
        uint32_t diff = 0;
#pragma unroll
        for (int d = 0; d < 4; d++) diff += (uint32_t)__builtin_popcount(((uint32_t)x[d] ^ c.ub[d]) & c.m[d]);
        return c.bias - (int)diff;
    }
    if (NB == 1) return 0;                          // no magnitude bits compared: every weight is zero
    int dot = 0;
#pragma unroll
    for (int d = 0; d < 4; d++) {
        const uint32_t xo = (uint32_t)x[d] ^ c.ub[d];
        const uint32_t y = ((xo & 0x7F7F7F7Fu) >> (8 - NB));                // per byte: the compared magnitude bits that differ
        const uint32_t t = ~y & c.m[d];                                     // W - y, 0 in padding columns
        const uint32_t sg = __builtin_amdgcn_perm(0x01010101u, 0x01010101u, xo & 0x80808080u);   // -1 where the signs differ
        dot = __builtin_amdgcn_sdot4((int)t, (int)sg, dot, false);
    }
    return dot;
}

// AppxConst of the 16 columns starting at c0, from the sign-magnitude Q_att(u) bytes `ub`
__device__ __forceinline__ void make_appx_const(AppxConst &c, const uint8_t *ub, uint32_t c0, uint32_t D)
{
#pragma unroll
    for (int d = 0; d < 4; d++) {
        const uint32_t b4 = *(const uint32_t *)(ub + c0 + 4 * d);
        c.um[d] = b4 & 0x7F7F7F7Fu;
        c.u127[d] = (b4 & 0x7F7F7F7Fu) + 0x7F7F7F7Fu;                         // per byte <= 254: no carry
        c.nb[d] = (~b4 & 0x7F7F7F7Fu) + 0x01010101u;                          // (127 - |u|) + 1 per byte
        c.us[d] = b4 & 0x80808080u;
        uint32_t vm = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) vm |= (c0 + 4 * d + i < D ? 0xFFu : 0u) << (8 * i);
        c.m7[d] = vm & 0x7F7F7F7Fu;
        c.m8[d] = vm & 0x80808080u;
    }
    c.bias = 127 * (int)(D >= c0 + 16 ? 16u : (D > c0 ? D - c0 : 0u));
}

// PlaneConst of the two plane words a lane owns (word index 2.chunk + t inside the row), from the
// query planes `upl` ([group][8] uint64)
template <int NB>
__device__ __forceinline__ void make_plane_const(PlaneConst &c, const uint64_t *upl, uint32_t chunk, uint32_t D)
{
#pragma unroll
    for (int t = 0; t < 2; t++) {
        const uint32_t wi = 2 * chunk + t;
        const uint32_t grp = wi / NB, pl = wi % NB;
        c.u[t] = upl[grp * 8 + pl];
        c.us[t] = upl[grp * 8 + 0];
        const uint32_t ncol = D > 64 * grp ? D - 64 * grp : 0;
        c.valid[t] = ncol >= 64 ? ~0ull : ((1ull << ncol) - 1ull);
        c.wgt[t] = pl == 0 ? 0 : (1 << (NB - 1 - pl));
    }
}

// ---- plane_lane_sum split for a tile of queries on ONE plane (batch_hops_shared_ham.hip) ------------------------------------
// The key half: the two 64-bit words of a loaded row and, for V1, the key's sign plane of the word's group (the quad-permute
// fetch of plane_lane_sum) -- once per loaded row.
template <int MODE, int NB>
__device__ __forceinline__ void plane_key_split(const i32x4 x, uint64_t (&k)[2], uint64_t &ks)
{
    k[0] = (uint64_t)(uint32_t)x[0] | ((uint64_t)(uint32_t)x[1] << 32);
    k[1] = (uint64_t)(uint32_t)x[2] | ((uint64_t)(uint32_t)x[3] << 32);
    ks = k[0];                                          // (NB <= 2: this lane holds its group's sign plane)
    if (MODE == kModeV1 && NB >= 4) {
        constexpr int ctrl = (NB == 4) ? 0xA0 /* quad_perm [0,0,2,2] */ : 0x00 /* [0,0,0,0] */;
        const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, x[0], ctrl, 0xF, 0xF, true);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, x[1], ctrl, 0xF, 0xF, true);
        ks = (uint64_t)lo | ((uint64_t)hi << 32);
    }
}
// The query half: one query's plane words `u` and sign planes `us` against the split key; `valid` and `wgt` depend on the lane
// alone (one copy for the tile).  The integer operations of plane_lane_sum, term by term.
template <int MODE, int NB>
__device__ __forceinline__ int plane_lane_sum_split(const uint64_t (&k)[2], uint64_t ks, const uint64_t (&u)[2], const uint64_t (&us)[2],
                                                    const uint64_t (&valid)[2], const int (&wgt)[2])
{
    if (MODE == kModeV0) return __popcll(~(k[0] ^ u[0]) & valid[0]) + __popcll(~(k[1] ^ u[1]) & valid[1]);
    if (NB == 1) return 0;                              // no magnitude planes: every weight is zero
    int acc = 0;
#pragma unroll
    for (int t = 0; t < 2; t++) {
        const uint64_t eq = ~(k[t] ^ u[t]);
        const uint64_t sdiff = (ks ^ us[t]) & valid[t];
        const uint64_t ssame = ~(ks ^ us[t]) & valid[t];
        acc += wgt[t] * (__popcll(eq & ssame) - __popcll(eq & sdiff));
    }
    return acc;
}

// ---- the softmax stages of the streaming kernels, per query ------------------------------------------------------------------
// (COPIES of the two stages k_hops_ham carries inline, batch_hops_ham.hip, with the same thread-to-slot mapping and the same
// float and double operations in the same order -- that kernel keeps its inline text so that its device assembly stays what was
// measured (tools/device_asm_equal.sh), as hist_softmax_survivors does for k_hops_fixed; keep them in step.)
// Both are called by the whole 256-thread workgroup after a barrier behind the scan, with misc[0] = 0 and S > 0 int16 scores in
// `sc`; taps are written from index `tap_base` on; both end with a barrier and return the number of rows whose quantised weight
// is non-zero (listed in live_row / live_kp up to kLiveCap).

// V0: one exp per distinct count through the histogram `v0_hist` (nbins bins, filled by the scan); v0_p / v0_kp: p and Q(p)
// per count afterwards
__device__ __forceinline__ uint32_t ham_hist_softmax_survivors(const HopArgs &a, uint32_t h, uint32_t S, uint32_t nbins, size_t tap_base,
                                                               const int16_t *sc, const uint32_t *v0_hist, float *v0_p, uint8_t *v0_kp,
                                                               uint32_t *live_row, uint8_t *live_kp, uint32_t *misc, double *red,
                                                               uint32_t tid, uint32_t lane, uint32_t wave)
{
    const QFmt fa = a.act[h];
    // one exp per distinct count; normaliser sum_d count[d] . e[d] in double (lib/layer_cuda.cu:2024-2042)
    const SmCfg smc = sm_cfg(a, h);
    float xmax = -INFINITY;
    for (uint32_t d = tid; d < nbins; d += kBlock)
        if (v0_hist[d]) xmax = fmaxf(xmax, sm_scaled((float)d, smc));
    xmax = block_max<float>(xmax, (float *)red, lane, wave);
    double part = 0.0;
    for (uint32_t d = tid; d < nbins; d += kBlock) {
        const float e = sm_exp(sm_scaled((float)d, smc) - xmax, smc);
        v0_p[d] = e;
        if (v0_hist[d]) part += (double)v0_hist[d] * (double)e;
    }
    const double total = smc.base == QMANN_SOFTMAX_EXP ? block_sum_double(part, red, lane, wave)
                                                       : block_serial_total_f32(S, lane, wave, red, [&](uint32_t r) { return v0_p[sc[r]]; });
    for (uint32_t d = tid; d < nbins; d += kBlock) {
        const float p = v0_hist[d] ? sm_quot(v0_p[d], total, smc) : 0.0f;
        v0_p[d] = p;
        v0_kp[d] = (uint8_t)qm_code(p, fa.iwl, fa.frac);
    }
    __syncthreads();
    if (a.tap_codes || a.tap_scores || a.tap_probs) {
        for (uint32_t r = tid; r < S; r += kBlock) {
            const int v = sc[r];
            if (a.tap_codes) a.tap_codes[tap_base + r] = v;
            if (a.tap_scores) a.tap_scores[tap_base + r] = (float)v;
            if (a.tap_probs) a.tap_probs[tap_base + r] = v0_p[v];
        }
    }
    // rows whose quantised weight is non-zero: 8 scores per LDS read, their 8 table look-ups in flight together
    for (uint32_t rb = tid * 8; rb < S; rb += kBlock * 8) {
        const i32x4 v = *(const i32x4 *)(sc + rb);               // (the score array is padded to 8 rows)
        uint8_t kp[8];
#pragma unroll
        for (int i = 0; i < 8; i++) kp[i] = v0_kp[rb + i < S ? ((uint32_t)v[i / 2] >> (16 * (i % 2))) & 0xFFFFu : 0u];
#pragma unroll
        for (int i = 0; i < 8; i++) {
            if (rb + i < S && kp[i]) {
                const uint32_t n = atomicAdd(&misc[0], 1u);
                if (n < (uint32_t)kLiveCap) { live_row[n] = rb + i; live_kp[n] = kp[i]; }
            }
        }
    }
    __syncthreads();
    return misc[0];
}

// Every other mode: per slot (max, sum of exp in double, quotient) with the threshold / code_lo shortcut of k_hops_ham (its
// comments hold the reasoning); `scale`: the unit of a score.  When the survivor list overflows, sc holds Q(p) per row afterwards.
// `select` (hops_attended_ham.h; by default nothing): called by the whole workgroup behind the survivor search, while the scores
// are still in sc, with p_of(score) -- the probability of a slot with that int16 score, by the expression the tap path writes.
struct HamNoSelect {
    template <typename POf> __device__ __forceinline__ void operator()(POf) const {}
};
template <typename Select = HamNoSelect>
__device__ __forceinline__ uint32_t ham_slot_softmax_survivors(const HopArgs &a, uint32_t h, uint32_t S, float scale, size_t tap_base,
                                                               int16_t *sc, uint32_t *live_row, uint8_t *live_kp, uint32_t *misc,
                                                               double *red, uint32_t tid, uint32_t lane, uint32_t wave,
                                                               const Select select = Select{})
{
    const QFmt fa = a.act[h];
    const SmCfg smc = sm_cfg(a, h);
    // (float)score . scale is exact (integers below 2^24 times a power of two)
    auto slot_x = [&](uint32_t r) { return sm_scaled((float)sc[r] * scale, smc); };
    float xmax = -INFINITY;
    for (uint32_t r = tid; r < S; r += kBlock) xmax = fmaxf(xmax, slot_x(r));
    xmax = block_max<float>(xmax, (float *)red, lane, wave);
    double part = 0.0;
    for (uint32_t r = tid; r < S; r += kBlock) part += (double)sm_exp(slot_x(r) - xmax, smc);
    const double total = smc.base == QMANN_SOFTMAX_EXP ? block_sum_double(part, red, lane, wave)
                                                       : block_serial_total_f32(S, lane, wave, red, [&](uint32_t r) { return sm_exp(slot_x(r) - xmax, smc); });
    const bool every = a.tap_codes || a.tap_scores || a.tap_probs || smc.shift;
    const float thr = every ? 0.0f : (float)(total * (double)qm_scale_down(1.0f, fa.frac) * (1.0 - 9.5367431640625e-07));
    int code_lo = INT_MIN;
    if (!every && smc.base == QMANN_SOFTMAX_EXP && !smc.en_scale)
        code_lo = (int)floorf((logf(thr) - 1e-3f + xmax) / scale) - 1;
    for (uint32_t r = tid; r < S; r += kBlock) {
        if ((int)sc[r] < code_lo) continue;
        const float e = sm_exp(slot_x(r) - xmax, smc);
        if (!(e >= thr)) continue;
        const float p = sm_quot(e, total, smc);
        if (a.tap_codes) a.tap_codes[tap_base + r] = sc[r];
        if (a.tap_scores) a.tap_scores[tap_base + r] = (float)sc[r] * scale;
        if (a.tap_probs) a.tap_probs[tap_base + r] = p;
        const int kp = qm_code(p, fa.iwl, fa.frac);
        if (kp) {
            const uint32_t i = atomicAdd(&misc[0], 1u);
            if (i < (uint32_t)kLiveCap) { live_row[i] = r; live_kp[i] = (uint8_t)kp; }
        }
    }
    __syncthreads();
    const uint32_t n_live = misc[0];
    select([&](int score) { return sm_quot(sm_exp(sm_scaled((float)score * scale, smc) - xmax, smc), total, smc); });
    if (n_live > (uint32_t)kLiveCap) {                  // keep the overflow path exact: park Q(p) in sc
        for (uint32_t r = tid; r < S; r += kBlock) {
            const float p = sm_quot(sm_exp(slot_x(r) - xmax, smc), total, smc);
            sc[r] = (int16_t)qm_code(p, fa.iwl, fa.frac);
        }
        __syncthreads();
    }
    return n_live;
}

}  // namespace
