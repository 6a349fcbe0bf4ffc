// batch_embed_idx.hip -- the stage before the hop loop, batched over queries: story / question embedding from word
// indices into int8 memories (gather-sum and matrix-core kernels), and the int8 embedding tables.
#include "embed_common.h"

namespace {

// ---------------------------------------------------------------------------
// Story embedding from WORD INDICES.  A bag-of-words row has at most a
// handful of non-zeros, so the dense X . W^T of dense_mat_fwd is a gather-sum over table rows.
// Wire format: uint16 [rows][max_words], unused entries 0xFFFF; with `time_last` the last valid
// entry of a row is its time-encoding index, whose bag-of-words entry is SET to 1 while word
// entries COUNT occurrences (MemN2N/sample.c:466-475, 544-548).  Tables are int8 [V][Dp]
// two's-complement codes of Q(w[h]) (transposed, so a word's row is contiguous).  For an integer
// count c the reference term Qw(Qw(c) . Qw(W)) is clamp(c' . kw, +-max) with c' = the count
// saturated to the format (a code needs no truncation when one factor is an integer), so the
// result is bit-identical to the float path.  One wavefront per story row, lane = column.
// ---------------------------------------------------------------------------
typedef short s16x2 __attribute__((ext_vector_type(2)));
constexpr int kMaxWords = 16;

struct EmbedIdxArgs {
    const uint16_t *words;
    const int8_t *t_a[QMANN_MAX_HOP];
    const int8_t *t_c[QMANN_MAX_HOP];
    int8_t *keys;
    int8_t *vals;
    size_t hop_stride;
    uint32_t n_hop, D, Dp, V, rows, max_words, time_last;
    QFmt act[QMANN_MAX_HOP], w[QMANN_MAX_HOP], att[QMANN_MAX_HOP];   // att: the format of the KEY BYTES (fill_key_formats)
    uint32_t key_mz;              // bit h: hop h's keys follow the minus-zero rule
    uint32_t qkinds;              // 2 bits per (hop, table): how the matrix-core kernel's epilogue may quantise (kQk*, below)
};

// integer count c >= 0 as a code of the format in units of 2^-frac: Qw(c), saturating at the format maximum
__device__ __forceinline__ int count_code(uint32_t c, uint32_t frac, int maxw)
{
    const uint64_t k = (uint64_t)c << frac;
    return k > (uint64_t)maxw ? maxw : (int)k;
}
// 16 lanes per story row (a lane owns 4 adjacent columns = one dword of a table row), 4 rows per wavefront step,
// persistent workgroups.  The kernel is bound by VALU issue, so the work per word slot is kept small:
//   * which slot adds what (word, count, first occurrence) is settled once per row group: the usual case -- no word
//     twice in a row -- is found with one LDS atomic per lane on a 256-bit hash bitmap per row; only a group with a
//     possible repeat compares its slots pairwise;
//   * the 8 (16) slots of a row are read back as one (two) 16-byte LDS loads and the table reads of all slots are in
//     flight together, for the A and the C table of a hop at once;
//   * small dictionaries: all 2.n_hop tables sit in LDS expanded to int16 (one ds_read_b64 per slot and table, no
//     unpacking; row V is zero so that an empty slot needs no predicate).  Large ones are gathered from L2 as int8.
constexpr uint32_t kEwWords = 16;                       // word slots per row
// per-wavefront LDS: wd u16 [4][16], ct u8 [4][16], duplicate-detection bitmaps u32 [4][8]
constexpr uint32_t kEwWd = 0, kEwCt = 128, kEwBm = 192, kEwWaveBytes = 320;

// One row group (4 rows, 16 lanes each): returns word | count << 16 for a slot that adds, 0xFFFF for one that does not
// (unused, out of range, or a repeat of a word an earlier slot of the row carries with its count).
__device__ __forceinline__ uint32_t ew_pack_row(uint32_t w, uint32_t V, bool time_last, uint32_t nw, uint32_t lane, uint32_t *bm)
{
    const uint32_t sub = lane & 15u, grp = lane >> 4;
    const uint32_t m16 = (uint32_t)(__ballot(w != 0xFFFFu) >> (16 * grp)) & 0xFFFFu;
    const uint32_t n_valid = 32u - (uint32_t)__clz(m16);
    const bool valid = w != 0xFFFFu && w < V;
    const bool is_time = time_last && valid && (sub + 1 == n_valid);
    if (lane < 32u) bm[lane] = 0u;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    bool clash = false;
    if (valid) {
        const uint32_t bit = 1u << (w & 31u);
        clash = (atomicOr(&bm[grp * 8u + ((w >> 5) & 7u)], bit) & bit) != 0u;
    }
    uint32_t cnt = 1;
    bool dup = false;
    if (__any(clash)) {                                  // a row of this group may hold a word twice: the exact, slow way
        const uint32_t me = w | (valid ? 1u << 16 : 0u) | (is_time ? 1u << 17 : 0u);
        bool timed = false;
        cnt = 0;
        for (uint32_t j = 0; j < nw; j++) {
            const uint32_t o = (uint32_t)__shfl((int)me, (int)j, 16);
            const bool same = (((o ^ me) & 0xFFFFu) == 0u) && ((o >> 16) & 1u);
            const bool o_time = (o >> 17) & 1u;
            cnt += (same && !o_time) ? 1u : 0u;          // word entries COUNT occurrences ...
            timed |= same && o_time;                     // ... the time entry SETS its slot to 1
            dup |= same && j < sub;
        }
        if (timed) cnt = 1;
    }
    return (valid && !dup) ? (w | (cnt << 16)) : 0xFFFFu;
}

// Qw of the sum, then the memory byte: magnitude moved to the target grid (toward zero), clamped, sign bit from the
// VALUE (a negative sum that truncates to zero is "minus zero")
// `mz`: the key bytes of a Hamming-family attention whose weight grid is wider than the attention grid -- a value of exactly
// -2^iwl_att is "minus zero" in the reference's operand word (ham_common.h::ham_ubyte): magnitude 0, sign kept
__device__ __forceinline__ uint32_t ew_to_bytes(s16x2 x, int maxw, QFmt fw, QFmt dst, bool mz = false)
{
    const short mw = (short)maxw;
    x = __builtin_elementwise_min(__builtin_elementwise_max(x, s16x2{(short)-mw, (short)-mw}), s16x2{mw, mw});
    u16x2 mag = __builtin_bit_cast(u16x2, __builtin_elementwise_max(x, (s16x2)(-x)));
    mag = dst.frac >= fw.frac ? (u16x2)(mag << (unsigned short)(dst.frac - fw.frac)) : (u16x2)(mag >> (unsigned short)(fw.frac - dst.frac));
    const unsigned short md = (unsigned short)((1u << (dst.iwl + dst.frac)) - 1u);
    if (mz) {
        const unsigned short edge = (unsigned short)(md + 1u);
        const u16x2 hit = __builtin_bit_cast(u16x2, (s16x2)(mag == u16x2{edge, edge})) & __builtin_bit_cast(u16x2, (s16x2)(x < s16x2{0, 0}));
        mag = mag & ~hit;
    }
    mag = __builtin_elementwise_min(mag, u16x2{md, md});
    const u16x2 sgn = __builtin_bit_cast(u16x2, (s16x2)(x >> 8)) & (unsigned short)0x0080;
    return __builtin_bit_cast(uint32_t, (u16x2)(mag | sgn));
}

// ew_to_bytes for the usual format pairs, on FOUR values at once in the byte domain (the matrix-core kernel's epilogue is a
// third of its instructions).  With word lengths of at most 8 the clamped sum fits a byte; its sign-magnitude form is
// (x ^ s) + (s & 1) per byte (s = 0xFF where x < 0: a negative byte becomes |x| - 1, then + 1, never a carry), and the target
// grid is at most one bit away in EN_MQ (MemN2N.c:748-754) and equal without it:
//   kQkSame   dst.frac == fw.frac, dst clamp not below the source's:   nothing to do
//   kQkLeft   dst.frac == fw.frac + 1, dst word length 8:              m + m per byte (<= 254), bytes >= 128 saturate to 127
//   kQkRight  dst.frac == fw.frac - 1, dst clamp not below maxw >> 1:  (m >> 1) per byte; the sign stays the VALUE's
//   kQkGeneral anything else (and keys under the minus-zero rule):     ew_to_bytes
enum { kQkSame = 0, kQkLeft = 1, kQkRight = 2, kQkGeneral = 3 };
__host__ __device__ inline uint32_t qkind_of(QFmt fw, QFmt dst, bool mz)
{
    const uint32_t maxw = (1u << (fw.iwl + fw.frac)) - 1u, md = (1u << (dst.iwl + dst.frac)) - 1u;
    if (mz || maxw > 127u) return kQkGeneral;
    if (dst.frac == fw.frac && md >= maxw) return kQkSame;
    if (dst.frac == fw.frac + 1u && md == 127u) return kQkLeft;
    if (dst.frac + 1u == fw.frac && md >= (maxw >> 1)) return kQkRight;
    return kQkGeneral;
}
// x01 / x23: the four sums as packed int16 pairs (columns 0, 1 and 2, 3 of a dword); returns the dword of memory bytes
__device__ __forceinline__ uint32_t ew_to_bytes4(s16x2 x01, s16x2 x23, int maxw, uint32_t kind)
{
    const short mw = (short)maxw;
    x01 = __builtin_elementwise_min(__builtin_elementwise_max(x01, s16x2{(short)-mw, (short)-mw}), s16x2{mw, mw});
    x23 = __builtin_elementwise_min(__builtin_elementwise_max(x23, s16x2{(short)-mw, (short)-mw}), s16x2{mw, mw});
    const uint32_t d = __builtin_amdgcn_perm(__builtin_bit_cast(uint32_t, x23), __builtin_bit_cast(uint32_t, x01), 0x06040200u);   // two's complement bytes
    const uint32_t sg = d & 0x80808080u;
    const uint32_t sm = __builtin_amdgcn_perm(0u, 0u, sg);               // 0xFF where negative (selector bytes >= 0x80 give 0xFF, 0 gives byte 0 = 0)
    uint32_t m = (d ^ sm) + (sm & 0x01010101u);                           // |x| per byte
    if (kind == kQkLeft) {
        m += m;
        m = (m | __builtin_amdgcn_perm(0u, 0u, m & 0x80808080u)) & 0x7F7F7F7Fu;
    } else if (kind == kQkRight) {
        m = (m >> 1) & 0x3F3F3F3Fu;
    }
    return m | sg;
}

template <bool TAB16>
__global__ void __launch_bounds__(kBlock)
k_embed_story_idx(const EmbedIdxArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave, sub = lane & 15u, grp = lane >> 4;
    const uint32_t V = a.V, H = a.n_hop, nw = a.max_words;
    const uint32_t dw = a.Dp / 4;                                        // dwords (4 columns) per row: 16, 32 or 64
    const uint32_t dw_sh = 31u - (uint32_t)__clz(dw);                    // (a full 32-bit multiply costs four plain operations)
    const uint32_t tab_bytes = TAB16 ? (V + 1u) * dw * 8u : 0u;          // int16 [V + 1][dw]{even-columns pair, odd-columns pair}
    uint8_t *tabs = smem;                                                // [H][2] tables (A, C)
    uint8_t *ws = smem + 2u * H * tab_bytes + wave * kEwWaveBytes;
    uint16_t *wd = (uint16_t *)(ws + kEwWd);
    uint8_t *ct = ws + kEwCt;
    uint32_t *bm = (uint32_t *)(ws + kEwBm);
    if (TAB16) {
        for (uint32_t t = 0; t < 2u * H; t++) {
            const uint32_t *src = (const uint32_t *)((t & 1u) ? a.t_c[t >> 1] : a.t_a[t >> 1]);
            uint2 *dst = (uint2 *)(tabs + t * tab_bytes);
            for (uint32_t i = tid; i < (V + 1u) * dw; i += kBlock) {
                const uint32_t x = i < V * dw ? src[i] : 0u;
                const s16x2 ev = (__builtin_bit_cast(s16x2, x) << 8) >> 8, od = __builtin_bit_cast(s16x2, x) >> 8;
                dst[i] = uint2{__builtin_bit_cast(uint32_t, ev), __builtin_bit_cast(uint32_t, od)};
            }
        }
        __syncthreads();
    }

    const size_t rows_per_pass = (size_t)gridDim.x * kWaves * 4;
    for (size_t s0 = ((size_t)blockIdx.x * kWaves + wave) * 4; s0 < a.rows; s0 += rows_per_pass) {
        const size_t s = s0 + grp;
        const bool row_ok = s < a.rows;
        uint32_t w = 0xFFFFu;
        if (row_ok && sub < nw) w = a.words[s * nw + sub];
        const uint32_t pk = ew_pack_row(w, V, a.time_last != 0, nw, lane, bm);
        wd[grp * kEwWords + sub] = (uint16_t)pk;
        ct[grp * kEwWords + sub] = (uint8_t)(pk >> 16);
        const bool multi = __any((pk >> 16) > 1u);
        // slots 8..15 matter only when some row of the group uses them
        const uint32_t n_pass = __any(sub >= 8u && (pk & 0xFFFFu) != 0xFFFFu) ? 2u : 1u;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

        for (uint32_t c0 = 0; c0 < dw; c0 += 16)                          // 64 columns per round (one round at bAbI width)
        for (uint32_t h = 0; h < H; h++) {
            const uint32_t c4 = c0 + sub;                                 // (dw is a multiple of 16: Dp is 64, 128 or 256)
            uint32_t colmask = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) colmask |= (4 * c4 + (uint32_t)k < a.D ? 0xFFu : 0u) << (8 * k);
            const QFmt fw = a.w[h];
            const int maxw = (1 << (fw.iwl + fw.frac)) - 1;
            // Qw(1 . kw) = kw needs 1.0 to be a value of the format (iwl >= 1); a purely fractional format saturates the
            // count itself, like a repeated word: then every term is Qw(Qw(count) . kw) per column (rare)
            const bool slow = multi || (1 << fw.frac) > maxw;
            const void *ta = TAB16 ? (const void *)(tabs + (2u * h) * tab_bytes) : (const void *)a.t_a[h];
            const void *tc = TAB16 ? (const void *)(tabs + (2u * h + 1u) * tab_bytes) : (const void *)a.t_c[h];
            s16x2 ae = {0, 0}, ao = {0, 0}, ce = {0, 0}, co = {0, 0};
            for (uint32_t pass = 0; pass < n_pass; pass++) {
                const i32x4 wv = *(const i32x4 *)(wd + grp * kEwWords + pass * 8u);
                s16x2 xa_e[8], xa_o[8], xc_e[8], xc_o[8];
#pragma unroll
                for (int e = 0; e < 8; e++) {
                    const uint32_t we = ((uint32_t)wv[e >> 1] >> (16 * (e & 1))) & 0xFFFFu;
                    if (TAB16) {
                        const uint32_t off = (((we < V ? we : V) << dw_sh) + c4) * 8u;
                        const uint2 t1 = *(const uint2 *)((const uint8_t *)ta + off), t2 = *(const uint2 *)((const uint8_t *)tc + off);
                        xa_e[e] = __builtin_bit_cast(s16x2, t1.x); xa_o[e] = __builtin_bit_cast(s16x2, t1.y);
                        xc_e[e] = __builtin_bit_cast(s16x2, t2.x); xc_o[e] = __builtin_bit_cast(s16x2, t2.y);
                    } else {
                        const bool ok = we < V;
                        const uint32_t off = ((ok ? we : 0u) << dw_sh) + c4;
                        const uint32_t t1 = ok ? ((const uint32_t *)ta)[off] : 0u, t2 = ok ? ((const uint32_t *)tc)[off] : 0u;
                        // sign-extended bytes: even columns (0, 2) and odd columns (1, 3)
                        xa_e[e] = (__builtin_bit_cast(s16x2, t1) << 8) >> 8; xa_o[e] = __builtin_bit_cast(s16x2, t1) >> 8;
                        xc_e[e] = (__builtin_bit_cast(s16x2, t2) << 8) >> 8; xc_o[e] = __builtin_bit_cast(s16x2, t2) >> 8;
                    }
                }
                if (slow) {
#pragma unroll
                    for (int e = 0; e < 8; e++) {
                        const uint32_t c1 = ct[grp * kEwWords + pass * 8u + e];
                        const int cc = count_code(c1 ? c1 : 1u, fw.frac, maxw);
#pragma unroll
                        for (int k = 0; k < 2; k++) {
                            xa_e[e][k] = (short)qm_mul_code(cc, xa_e[e][k], fw.frac, maxw); xa_o[e][k] = (short)qm_mul_code(cc, xa_o[e][k], fw.frac, maxw);
                            xc_e[e][k] = (short)qm_mul_code(cc, xc_e[e][k], fw.frac, maxw); xc_o[e][k] = (short)qm_mul_code(cc, xc_o[e][k], fw.frac, maxw);
                        }
                    }
                }
                // Sums of <= 16 codes fit 16 bits: columns 0/2 and 1/3 of the dword are kept as packed int16 pairs
#pragma unroll
                for (int e = 0; e < 8; e++) { ae += xa_e[e]; ao += xa_o[e]; ce += xc_e[e]; co += xc_o[e]; }
            }
            if (row_ok) {
                const bool kmz = (a.key_mz >> h) & 1u;
                *(uint32_t *)(a.keys + (size_t)h * a.hop_stride + s * a.Dp + 4 * c4) = (ew_to_bytes(ae, maxw, fw, a.att[h], kmz) | (ew_to_bytes(ao, maxw, fw, a.att[h], kmz) << 8)) & colmask;
                *(uint32_t *)(a.vals + (size_t)h * a.hop_stride + s * a.Dp + 4 * c4) = (ew_to_bytes(ce, maxw, fw, a.act[h]) | (ew_to_bytes(co, maxw, fw, a.act[h]) << 8)) & colmask;
            }
        }
        __builtin_amdgcn_wave_barrier();                                 // the next group rewrites wd / ct
    }
}

// ---------------------------------------------------------------------------
// The same embedding on the int8 matrix cores, for dictionaries of up to 256 entries (every bAbI configuration).
// A tile of 16 story rows is a bag-of-words matrix X [16][K] of small counts (K = dictionary size padded to 64) and
//     E^T [columns][rows] = T^T [columns][K] . X^T
// is one v_mfma_i32_16x16x64_i8 per 16 columns and 64 dictionary entries, exact in int32.  The operands fall out of the
// wire format: X is built in LDS with one byte-add per word slot (the time entry is stored as 1 afterwards: it SETS its
// slot), T^T is staged once per workgroup.  The accumulator layout hands every lane 4 adjacent columns of one row -- one
// output dword -- so the quantisation epilogue (ew_to_bytes) runs on 2 packed registers per 16 x 16 tile and table.
// Per 16 rows and hop: ~200 vector instructions instead of ~2 000 for the gather-sum above (that kernel is bound by VALU
// issue: SQ_INSTS_VALU x 4.2 cycles is 70 % of its run time).
// What the product cannot express is the per-product clamp of a REPEATED word, Qw(Qw(count) . kw) != count . kw when
// |count . kw| exceeds the format: the second occurrence of a word in a row is noticed by the byte-add itself (it returns
// the old count) and those few (row, word) pairs get a per-column correction.  Purely fractional weight formats
// (1.0 not representable, so even a single word is Qw(Qw(1) . kw)) keep the gather-sum kernel.
// Grid: x = workgroups over tiles (persistent), y = hop.
// ---------------------------------------------------------------------------
constexpr uint32_t kEmRows = 16;                        // story rows per tile
// LDS images of the two MFMA operands, laid out for ds_read_b128's lane groups.  The hardware serves a wavefront's b128 read in
// four groups of 16 lanes -- {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32 (MI355X_MICROARCH.md, LDS) -- and a
// fragment's lane l reads row l & 15, K bytes 16 (l >> 4) .. + 15: every group holds each row 0 .. 15 exactly once, with a K
// piece that depends on the row.  So a row's pieces must not share banks across K pieces: each (16 rows x 16 bytes) block of
// one K piece is 256 contiguous bytes, row r at 16 r -- a group's 16 lanes then cover the 64 banks once whatever pieces they
// read.  (Through round 4 these images were row-major with a 16-byte pad: rows 11 and 12 of adjacent pieces met in every
// group, SQ_LDS_BANK_CONFLICT was half of the LDS-active cycles and the LDS array was busy 64 % of the kernel.)
//   T^T: [table][16-column block][K / 16 pieces][16 columns][16 bytes]       em_tt_off(K, table, column, k)
//   X  : [K / 16 pieces][16 rows][16 bytes]                                   em_x_off(row, k)
__device__ __forceinline__ uint32_t em_tt_off(uint32_t K, uint32_t t, uint32_t col, uint32_t k)
{
    return ((((t * 4u + (col >> 4)) * (K >> 4) + (k >> 4)) * 16u + (col & 15u)) << 4) + (k & 15u);
}
__device__ __forceinline__ uint32_t em_x_off(uint32_t row, uint32_t k) { return ((((k >> 4) << 4) + row) << 4) + (k & 15u); }
constexpr uint32_t kEmDupCap = 128;                     // repeated (row, word) pairs a tile can hold: 16 rows x 16 slots / 2

// wavefronts per SIMD each instantiation is compiled for (its register budget; the launcher sizes the persistent grid by it)
// (KS = 1, task-1 dictionaries: 80 registers buy a third 8-wavefront workgroup per CU -- the kernel is latency-bound: +4.5 % on the task-1 forward
// in an interleaved A/B against five per SIMD; the 16-wavefront forms are held to one workgroup per CU by their LDS tiles)
constexpr int em_waves_per_simd(int KS) { return KS == 1 ? 6 : 4; }

template <int KS, int NW>                               // K / 64: 1, 2 or 4; wavefronts per workgroup (they share T^T)
__global__ void __launch_bounds__(NW * kWave, em_waves_per_simd(KS))
k_embed_story_mfma(const EmbedIdxArgs a)
{
    constexpr uint32_t kBlockEm = NW * kWave;
    constexpr uint32_t K = 64u * KS;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // (readfirstlane: the compiler treats threadIdx.x / 64 as divergent and would keep every per-wavefront address in vector registers)
    const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1), wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid / kWave));
    constexpr uint32_t Dp = 64;                         // bAbI width (wider embeddings take the gather-sum kernel): the product loops
                                                        // unroll, so a tile's fragment loads and MFMAs are in flight together
    const uint32_t h = blockIdx.y, V = a.V, nw = a.max_words;
    int8_t *tt = (int8_t *)smem;                                         // [2][Dp][K]: A then C of this hop, transposed (em_tt_off)
    constexpr uint32_t SP = Dp + 16u;                                    // row pitch of the output staging tile (conflict-free dword writes)
    uint8_t *ws = smem + 2u * Dp * K + wave * (kEmRows * K + kEmRows * SP + kEmDupCap * 4u + 16u);
    uint32_t *X = (uint32_t *)ws;                                        // [16][K] bytes (em_x_off)
    uint8_t *stage = ws + kEmRows * K;                                   // [16][SP] one table's output rows
    uint32_t *dup = (uint32_t *)(stage + kEmRows * SP);                  // [kEmDupCap] row << 16 | word
    uint32_t *n_dup = dup + kEmDupCap;

    // ---- T^T of the hop's two tables ------------------------------------------------------------------------------
    for (uint32_t t = 0; t < 2; t++) {
        const uint32_t *src = (const uint32_t *)(t ? a.t_c[h] : a.t_a[h]);       // [V][Dp] two's complement
        for (uint32_t i = tid; i < K * (Dp / 4); i += kBlockEm) {
            const uint32_t k = i / (Dp / 4), c4 = i % (Dp / 4);
            const uint32_t x = k < V ? src[(size_t)k * (Dp / 4) + c4] : 0u;
#pragma unroll
            for (uint32_t j = 0; j < 4; j++) tt[em_tt_off(K, t, 4 * c4 + j, k)] = (int8_t)(x >> (8 * j));
        }
    }
    __syncthreads();

    const QFmt fw = a.w[h], f_att = a.att[h], f_act = a.act[h];
    const bool kmz = (a.key_mz >> h) & 1u;
    const int maxw = (1 << (fw.iwl + fw.frac)) - 1;
    const uint32_t r4 = lane >> 2, qd = lane & 3u;                       // word phase: row r4 of the tile, slots 4 qd .. 4 qd + 3
    const uint32_t nrow = lane & 15u, kq = lane >> 4;                    // matrix phase: story row nrow, K bytes 16 kq .. / columns 4 kq ..
    const size_t n_tiles = ((size_t)a.rows + kEmRows - 1) / kEmRows;
    // This lane's 4 word slots of a tile (row r4, slots 4 qd ..): one 8-byte load (the launcher sends word lists whose
    // pitch is not a multiple of 4 slots to the gather-sum kernel).  Requested one tile ahead so that a wavefront does
    // not start every tile with a round trip to HBM: the load is unconditional (address clamped into the array) and its
    // result is not touched before the next iteration -- a predicated load, or any use of the value, makes the compiler
    // wait for it on the spot.
    const uint32_t slot0 = 4 * qd < nw ? 4 * qd : 0u;
    uint2 raw_next = {0u, 0u};
    auto request_words = [&](size_t tile_) {
        size_t row = tile_ * kEmRows + r4;
        row = row < a.rows ? row : a.rows - 1;
        raw_next = *(const uint2 *)(a.words + row * nw + slot0);
    };
    auto take_words = [&](size_t tile_, uint32_t (&w_)[4]) {
        const bool in = tile_ * kEmRows + r4 < a.rows;
        w_[0] = raw_next.x & 0xFFFFu; w_[1] = raw_next.x >> 16; w_[2] = raw_next.y & 0xFFFFu; w_[3] = raw_next.y >> 16;
#pragma unroll
        for (uint32_t i = 0; i < 4; i++) w_[i] = (in && 4 * qd + i < nw) ? w_[i] : 0xFFFFu;
    };
    const size_t tile_step = (size_t)gridDim.x * NW;
    request_words((size_t)blockIdx.x * NW + wave);
    // A tile's finished rows (16 bytes per lane and table) are stored at the START of the next iteration, behind that
    // iteration's word request: vector loads and stores retire in order through one counter, so waiting for the words
    // of a tile also waits for every older store -- stores issued a whole iteration earlier have long completed, stores
    // issued just before the wait would put their full latency in front of every tile.
    i32x4 pend[2];
    size_t pend_row0 = 0;
    bool pending = false;
    // (raw BUFFER stores on a resource that spans the tile's rows: a row past the plane's last one is dropped by the bounds check and
    // the stores stand under no lane predicate -- with one the compiler cannot count the stores in flight and waits for ALL of them,
    // `vmcnt(0)`, wherever it waits for the next tile's words: k_embed_story_mfma_hops below has the measurement)
    auto flush_pending = [&]() {
        if (!pending) return;
        const size_t left = (size_t)a.rows - pend_row0;
        const int bytes = (int)((left < kEmRows ? left : (size_t)kEmRows) * Dp);
        const __amdgpu_buffer_rsrc_t rk = __builtin_amdgcn_make_buffer_rsrc((void *)(a.keys + (size_t)h * a.hop_stride + pend_row0 * Dp), 0, bytes, kRawBufferFlags);
        const __amdgpu_buffer_rsrc_t rv = __builtin_amdgcn_make_buffer_rsrc((void *)(a.vals + (size_t)h * a.hop_stride + pend_row0 * Dp), 0, bytes, kRawBufferFlags);
        // (nt: 0.6-0.9 GB of rows per batch, read back once by the hop kernel after the whole plane is written -- streamed past
        // the caches: task-1 forward +2.2 %, 20-task +0.5 % in an interleaved A/B against the default policy)
        __builtin_amdgcn_raw_buffer_store_b128(pend[0], rk, (int)(lane * 16u), 0, kBufferNt);
        __builtin_amdgcn_raw_buffer_store_b128(pend[1], rv, (int)(lane * 16u), 0, kBufferNt);
        pending = false;
    };
    for (size_t tile = (size_t)blockIdx.x * NW + wave; tile < n_tiles; tile += tile_step) {
        const size_t row0 = tile * kEmRows;
        QM_MARK("X: zero, words of the tile");
        // ---- X: counts per (row, word) -----------------------------------------------------------------------------
        for (uint32_t i = lane; i < kEmRows * K / 16u; i += kWave) *(i32x4 *)((uint8_t *)X + i * 16u) = i32x4{0, 0, 0, 0};
        if (lane == 0) *n_dup = 0u;
        uint32_t w[4];
        take_words(tile, w);
        asm volatile("" : "+v"(w[0]), "+v"(w[1]), "+v"(w[2]), "+v"(w[3]));    // (the words are taken HERE, before the next request is issued: see k_embed_story_mfma_hops)
        __builtin_amdgcn_sched_barrier(0);
        request_words(tile + tile_step);
        flush_pending();                                                 // the previous tile's rows (see below)
        QM_MARK("X: last slot, byte adds, time entry");
        uint32_t last = 0;                                               // 1 + this row's last non-empty slot
#pragma unroll
        for (uint32_t i = 0; i < 4; i++) last = w[i] != 0xFFFFu ? 4 * qd + i + 1 : last;
        {   // maximum over the 4 lanes of the row
            uint32_t o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)last, 0xB1, 0xF, 0xF, true);       // quad_perm [1,0,3,2]
            last = o > last ? o : last;
            o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)last, 0x4E, 0xF, 0xF, true);                // quad_perm [2,3,0,1]
            last = o > last ? o : last;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        uint32_t time_w = 0xFFFFu;
#pragma unroll
        for (uint32_t i = 0; i < 4; i++) {
            if (w[i] >= V) continue;                                     // empty (0xFFFF) or out of range: ignored
            if (a.time_last && 4 * qd + i + 1 == last) { time_w = w[i]; continue; }
            const uint32_t sh = 8u * (w[i] & 3u);
            const uint32_t old = atomicAdd(&X[em_x_off(r4, w[i]) >> 2], 1u << sh);
            if (((old >> sh) & 0xFFu) == 1u) {                           // the second occurrence announces the repeat, once
                const uint32_t n = atomicAdd(n_dup, 1u);
                if (n < kEmDupCap) dup[n] = (r4 << 16) | w[i];
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (time_w != 0xFFFFu) ((uint8_t *)X)[em_x_off(r4, time_w)] = 1;  // the time entry SETS its slot (sample.c:474)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

        QM_MARK("B fragments, repeated words");
        i32x4 bx[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ks++) bx[ks] = *(const i32x4 *)((const uint8_t *)X + em_x_off(nrow, ks * 64u + kq * 16u));

        // ---- repeated words: does any product Qw(Qw(count) . kw) differ from count . kw?  (it does only when the product
        // leaves the format: |count . kw| > max_w -- rare; lane = column) ------------------------------------------------
        const uint32_t nd = *n_dup < kEmDupCap ? *n_dup : kEmDupCap;
        uint32_t fix_rows = 0;                                           // rows to be summed term by term (wavefront-uniform)
        for (uint32_t d = 0; d < nd; d++) {
            const uint32_t e = dup[d], r = e >> 16, wd = e & 0xFFFFu;
            const int c = (int)((const uint8_t *)X)[em_x_off(r, wd)];
            const int cc = count_code((uint32_t)c, fw.frac, maxw);
            const int ka = (int)tt[em_tt_off(K, 0, lane, wd)], kc = (int)tt[em_tt_off(K, 1, lane, wd)];
            if (__any(qm_mul_code(cc, ka, fw.frac, maxw) != c * ka || qm_mul_code(cc, kc, fw.frac, maxw) != c * kc)) fix_rows |= 1u << r;
        }

        QM_MARK("products (MFMA)");
        // ---- the products, the epilogue, the stores ---------------------------------------------------------------
        // A lane's 4 columns are one dword; the 16 rows of a tile are contiguous in memory, so the tile leaves through an
        // LDS staging tile as whole rows, 16 bytes per lane (a store of 64 scattered dwords per 16 columns ran at the
        // rate of one cache line per lane group: the kernel was bound by it).
        i32x4 acc[2][4];
#pragma unroll
        for (uint32_t t = 0; t < 2; t++)
#pragma unroll
            for (uint32_t cb = 0; cb < 4; cb++) {
                acc[t][cb] = i32x4{0, 0, 0, 0};
#pragma unroll
                for (int ks = 0; ks < KS; ks++) {
                    const i32x4 am = *(const i32x4 *)(tt + em_tt_off(K, t, cb * 16u + nrow, ks * 64u + kq * 16u));
                    acc[t][cb] = __builtin_amdgcn_mfma_i32_16x16x64_i8(am, bx[ks], acc[t][cb], 0, 0, 0);
                }
            }
        QM_MARK("epilogue: quantise, stage, rows back");
#pragma unroll
        for (uint32_t t = 0; t < 2; t++) {
            const QFmt dstf = t ? f_act : f_att;
            const uint32_t qk = (a.qkinds >> (4u * h + 2u * t)) & 3u;    // (workgroup-uniform)
#pragma unroll
            for (uint32_t cb = 0; cb < 4; cb++) {
                const i32x4 v = acc[t][cb];                              // v[r]: story row nrow, column 16 cb + 4 kq + r
                const s16x2 x01 = __builtin_bit_cast(s16x2, __builtin_amdgcn_perm((uint32_t)v[1], (uint32_t)v[0], 0x05040100u));
                const s16x2 x23 = __builtin_bit_cast(s16x2, __builtin_amdgcn_perm((uint32_t)v[3], (uint32_t)v[2], 0x05040100u));
                uint32_t out;
                if (qk != kQkGeneral) {
                    out = ew_to_bytes4(x01, x23, maxw, qk);
                } else {
                    const uint32_t b01 = ew_to_bytes(x01, maxw, fw, dstf, t == 0 && kmz), b23 = ew_to_bytes(x23, maxw, fw, dstf, t == 0 && kmz);
                    out = __builtin_amdgcn_perm(b23, b01, 0x06040200u);
                }
                *(uint32_t *)(stage + nrow * SP + cb * 16u + kq * 4u) = out;
            }
            // a row whose repeated word leaves the format: its sums term by term, Qw(Qw(count) . kw) over the row's distinct
            // words (the non-zero bytes of its X row), lane = column; replaces the row in the staging tile
            for (uint32_t m = fix_rows; m; m &= m - 1) {
                const uint32_t r = (uint32_t)__builtin_ctz(m);
                const uint32_t xr = lane < K / 4 ? X[em_x_off(r, 4u * lane) >> 2] : 0u;       // counts of words 4 lane .. 4 lane + 3
                int sum = 0;
                for (uint64_t nz = __ballot(xr != 0u); nz; nz &= nz - 1) {
                    const uint32_t j = (uint32_t)__builtin_ctzll(nz);
                    const uint32_t xv = (uint32_t)__builtin_amdgcn_readlane((int)xr, (int)j);
#pragma unroll
                    for (uint32_t b = 0; b < 4; b++) {
                        const uint32_t c = (xv >> (8 * b)) & 0xFFu;
                        if (c) sum += qm_mul_code(count_code(c, fw.frac, maxw), (int)tt[em_tt_off(K, t, lane, 4 * j + b)], fw.frac, maxw);
                    }
                }
                __builtin_amdgcn_wave_barrier();                         // (every lane's dword of this row is written)
                stage[r * SP + lane] = (uint8_t)ew_to_bytes(s16x2{(short)sum, (short)0}, maxw, fw, dstf, t == 0 && kmz);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            // whole rows, 16 bytes per lane: lane i holds piece i % 4 of row i / 4 (16 rows x 64 bytes = 64 lanes x 16 bytes)
            pend[t] = *(const i32x4 *)(stage + (lane / (Dp / 16u)) * SP + (lane % (Dp / 16u)) * 16u);
            __builtin_amdgcn_wave_barrier();                             // the second table reuses the staging tile
        }
        pend_row0 = row0;
        pending = true;
        __builtin_amdgcn_wave_barrier();                                 // the next tile rewrites X
        QM_MARK("end of tile");
    }
    flush_pending();
}

// ---------------------------------------------------------------------------
// The same for the joint-task dictionaries (129 .. 256 entries), EVERY HOP of a tile in one workgroup.  With one workgroup per
// hop (the kernel above) a tile's count matrix X is rebuilt for every hop -- 135 of its 349 vector instructions per tile and hop
// (tools/stage_budget.py; the kernel's vector and matrix issue together keep a SIMD 75 % busy, profiles/r05_units_j20_*) -- because
// T^T of three hops (104 KB) and sixteen wavefronts' whole X tiles (70 KB) do not fit one CU's LDS together.  They do once X is
// built in four CHUNKS of 64 dictionary entries: a chunk is 16 rows x 80 bytes, becomes the wavefront's B fragment of that K
// step at once (4 registers), and its LDS bytes are reused by the next chunk and, after the products, by the staging tile.
// Per tile: 4 short build rounds (zero 1.3 KB, byte-add the words of the chunk, set the time entry, read the fragment) for all
// hops together instead of a 4.3 KB build per hop; then per hop 32 MFMAs, the epilogue and the stores as above.  Hops before
// the last store their rows at once (younger than the next tile's word request, so the wait for those words does not wait for
// them); the last hop's rows wait in registers for the start of the next tile, as above.
// Repeated words: noticed by the byte-add as above, checked per chunk against every hop's tables; a row whose repeated word
// leaves a hop's weight format is summed term by term from the tile's word list (kept in LDS for that, 512 bytes).
// ---------------------------------------------------------------------------
template <int NW, int KS_, int WPS>                     // wavefronts per workgroup; K / 64 (chunks); wavefronts per SIMD compiled for
__global__ void __launch_bounds__(NW * kWave, WPS)
k_embed_story_mfma_hops(const EmbedIdxArgs a)
{
    constexpr uint32_t kBlockEm = NW * kWave;
    constexpr uint32_t KS = (uint32_t)KS_, K = 64u * KS, Dp = 64u;
    constexpr uint32_t XC = kEmRows * 64u;              // an X chunk: [4 pieces][16 rows][16 bytes] (em_x_off on k & 63)
    constexpr uint32_t SP = Dp + 16u;                   // row pitch of the staging tile, which follows the two chunks in their bytes
    constexpr uint32_t kWaveLds = 2u * XC + kEmDupCap * 4u + 16u + kEmRows * 16u * 2u;
    static_assert(2u * XC >= kEmRows * SP, "the staging tile lies over the two X chunks");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1), wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid / kWave));
    const uint32_t H = a.n_hop, V = a.V, nw = a.max_words;
    int8_t *tt = (int8_t *)smem;                                         // [H][2][Dp][K]: A then C of every hop, transposed (em_tt_off)
    uint8_t *ws = smem + (size_t)H * 2u * Dp * K + wave * kWaveLds;
    uint8_t *xs = ws;                                                    // two X chunks in turn (one is zeroed while the other is filled); later one table's output rows [16][SP]
    uint32_t *dup = (uint32_t *)(ws + 2u * XC);                          // [kEmDupCap] row << 16 | word
    uint32_t *n_dup = dup + kEmDupCap;
    uint16_t *wl = (uint16_t *)(n_dup + 4);                              // [16][16] the tile's words (the term-by-term path reads them)

    for (uint32_t t = 0; t < 2u * H; t++) {
        const uint32_t *src = (const uint32_t *)((t & 1u) ? a.t_c[t >> 1] : a.t_a[t >> 1]);      // [V][Dp] two's complement
        int8_t *dst = tt + (size_t)(t >> 1) * 2u * Dp * K;
        for (uint32_t i = tid; i < K * (Dp / 4); i += kBlockEm) {
            const uint32_t k = i / (Dp / 4), c4 = i % (Dp / 4);
            const uint32_t x = k < V ? src[(size_t)k * (Dp / 4) + c4] : 0u;
#pragma unroll
            for (uint32_t j = 0; j < 4; j++) dst[em_tt_off(K, t & 1u, 4 * c4 + j, k)] = (int8_t)(x >> (8 * j));
        }
    }
    __syncthreads();
    QM_CLK_DECL();
    QM_CLK(0);                                                           // 0: T^T staging

    const uint32_t r4 = lane >> 2, qd = lane & 3u;                       // word phase: row r4 of the tile, slots 4 qd .. 4 qd + 3
    const uint32_t nrow = lane & 15u, kq = lane >> 4;                    // matrix phase: story row nrow, K bytes 16 kq .. / columns 4 kq ..
    const size_t n_tiles = ((size_t)a.rows + kEmRows - 1) / kEmRows;
    const uint32_t slot0 = 4 * qd < nw ? 4 * qd : 0u;
    uint2 raw_next = {0u, 0u};
    auto request_words = [&](size_t tile_) {
        size_t row = tile_ * kEmRows + r4;
        row = row < a.rows ? row : a.rows - 1;
        raw_next = *(const uint2 *)(a.words + row * nw + slot0);
    };
    auto take_words = [&](size_t tile_, uint32_t (&w_)[4]) {
        const bool in = tile_ * kEmRows + r4 < a.rows;
        w_[0] = raw_next.x & 0xFFFFu; w_[1] = raw_next.x >> 16; w_[2] = raw_next.y & 0xFFFFu; w_[3] = raw_next.y >> 16;
#pragma unroll
        for (uint32_t i = 0; i < 4; i++) w_[i] = (in && 4 * qd + i < nw) ? w_[i] : 0xFFFFu;
    };
    auto wsync = [&]() {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    };
    const size_t tile_step = (size_t)gridDim.x * NW;
    request_words((size_t)blockIdx.x * NW + wave);
    // the last hop's rows of the previous tile (keeping the last TWO hops' rows back, so that the youngest stores in flight at the
    // wait for a tile's words are two thirds of a tile old, measured 3 % SLOWER on the joint forwards)
    i32x4 pend[2];
    size_t pend_row0 = 0;
    bool pending = false;
    const uint32_t srow = lane / (Dp / 16u), spiece = lane % (Dp / 16u);  // whole rows out: lane i holds piece i % 4 of row i / 4
    // Rows leave through raw BUFFER stores on a resource that spans exactly the tile's rows inside the plane: a row past the
    // last one (the last tile only) is dropped by the bounds check, so the stores stand under no branch.  With a lane predicate
    // around them the compiler cannot count the stores in flight, and the wait for the NEXT tile's words -- a load older than
    // these stores -- became `s_waitcnt vmcnt(0)`: every tile waited for its predecessor's stores to reach memory (15 % of a
    // wavefront's time, tools/stage_clocks.py).
    auto store_rows = [&](uint32_t h, size_t row0_, const i32x4 (&rows_)[2]) {
        const size_t left = (size_t)a.rows - row0_;                      // (row0_ < rows for every tile that runs)
        const int bytes = (int)((left < kEmRows ? left : (size_t)kEmRows) * Dp);
        const __amdgpu_buffer_rsrc_t rk = __builtin_amdgcn_make_buffer_rsrc((void *)(a.keys + (size_t)h * a.hop_stride + row0_ * Dp), 0, bytes, kRawBufferFlags);
        const __amdgpu_buffer_rsrc_t rv = __builtin_amdgcn_make_buffer_rsrc((void *)(a.vals + (size_t)h * a.hop_stride + row0_ * Dp), 0, bytes, kRawBufferFlags);
        __builtin_amdgcn_raw_buffer_store_b128(rows_[0], rk, (int)(lane * 16u), 0, kBufferNt);
        __builtin_amdgcn_raw_buffer_store_b128(rows_[1], rv, (int)(lane * 16u), 0, kBufferNt);
    };
    for (size_t tile = (size_t)blockIdx.x * NW + wave; tile < n_tiles; tile += tile_step) {
        const size_t row0 = tile * kEmRows;
        QM_MARK("words of the tile");
        QM_CLK(1);                                                       // 1: loop overhead / end of the previous tile
        uint32_t w[4];
        take_words(tile, w);
        // (the words are TAKEN before anything else is issued: hoisted above them, the next tile's request and the pending stores
        // stood between the old load and its wait, and the compiler -- which cannot count the stores of the hop loop behind it --
        // waited `vmcnt(1)`: for the request it had just issued.  15 % of a wavefront's time, tools/stage_clocks.py)
        asm volatile("" : "+v"(w[0]), "+v"(w[1]), "+v"(w[2]), "+v"(w[3]));    // (materialised HERE: the wait for the old load sits in front of the new request)
        __builtin_amdgcn_sched_barrier(0);
        request_words(tile + tile_step);
        if (pending) { store_rows(H - 1u, pend_row0, pend); pending = false; }
        *(uint2 *)(wl + r4 * 16u + 4u * qd) = uint2{w[0] | (w[1] << 16), w[2] | (w[3] << 16)};
        if (lane == 0) *n_dup = 0u;
        uint32_t last = 0;                                               // 1 + this row's last non-empty slot
#pragma unroll
        for (uint32_t i = 0; i < 4; i++) last = w[i] != 0xFFFFu ? 4 * qd + i + 1 : last;
        {   // maximum over the 4 lanes of the row
            uint32_t o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)last, 0xB1, 0xF, 0xF, true);       // quad_perm [1,0,3,2]
            last = o > last ? o : last;
            o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)last, 0x4E, 0xF, 0xF, true);                // quad_perm [2,3,0,1]
            last = o > last ? o : last;
        }
        // The time entry (the row's last non-empty slot, if its word is in range) SETS its byte to 1 (sample.c:474), the other
        // slots count.  Here the time slot simply adds its 1 and every other slot of the row that holds the same word is dropped:
        // the same byte, without a separate store (and its wait) behind the adds.
        uint32_t time_w = 0xFFFFu;
#pragma unroll
        for (uint32_t i = 0; i < 4; i++) {
            if (w[i] >= V) { w[i] = 0xFFFFu; continue; }                 // empty or out of range: ignored
            if (a.time_last && 4 * qd + i + 1 == last) time_w = w[i];
        }
        {   // the row's time word to its four lanes (one of them holds it, the others 0xFFFF: a minimum)
            uint32_t o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)time_w, 0xB1, 0xF, 0xF, true);
            uint32_t tw = o < time_w ? o : time_w;
            o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)tw, 0x4E, 0xF, 0xF, true);
            tw = o < tw ? o : tw;
#pragma unroll
            for (uint32_t i = 0; i < 4; i++)
                if (w[i] == tw && !(a.time_last && 4 * qd + i + 1 == last)) w[i] = 0xFFFFu;
        }
        QM_CLK(2);                                                       // 2: words taken (waits for the prefetched load), pending stores, time word
        // ---- X in four chunks of 64 dictionary entries: each becomes the B fragment of its K step ------------------------
        i32x4 bx[KS];
        uint32_t fix_rows[QMANN_MAX_HOP] = {};                           // per hop: rows to be summed term by term (wavefront-uniform)
        uint32_t nd_seen = 0;
        bool repeats = false;                                            // some lane's byte add met a count of 1 (wavefront-uniform once balloted)
#pragma unroll
        for (uint32_t ks = 0; ks < KS; ks++) {
            QM_MARK("X chunk: zero the next, byte adds, fragment");
            uint8_t *xc = xs + (ks & 1u) * XC, *xn = xs + ((ks + 1u) & 1u) * XC;
            if (ks == 0) {                                               // (the later chunks were zeroed a round ahead)
                *(i32x4 *)(xc + lane * 16u) = i32x4{0, 0, 0, 0};
                wsync();
            }
            if (ks + 1u < KS) *(i32x4 *)(xn + lane * 16u) = i32x4{0, 0, 0, 0};
#pragma unroll
            for (uint32_t i = 0; i < 4; i++) {
                if (w[i] == 0xFFFFu || (w[i] >> 6) != ks) continue;
                const uint32_t sh = 8u * (w[i] & 3u);
                const uint32_t old = atomicAdd((uint32_t *)(xc + (em_x_off(r4, w[i] & 63u) & ~3u)), 1u << sh);
                if (((old >> sh) & 0xFFu) == 1u) {                       // the second occurrence announces the repeat, once
                    const uint32_t n = atomicAdd(n_dup, 1u);
                    if (n < kEmDupCap) dup[n] = (r4 << 16) | w[i];
                    repeats = true;
                }
            }
            QM_CLK(3);                                                   // 3: chunk zero + byte adds issued
            wsync();
            QM_CLK(4);                                                   // 4: wait for the adds
            bx[ks] = *(const i32x4 *)(xc + em_x_off(nrow, kq * 16u));
            // repeated words of this chunk: does any product Qw(Qw(count) . kw) differ from count . kw in some hop?  (only when the
            // product leaves the format: rare; lane = column)
            // (the list's length is read only when some lane announced a repeat: otherwise an LDS round trip per chunk for nothing)
            uint32_t nd = nd_seen;
            if (__any(repeats)) { nd = *n_dup < kEmDupCap ? *n_dup : kEmDupCap; }
            for (uint32_t d = nd_seen; d < nd; d++) {
                const uint32_t e = dup[d], r = e >> 16, wd = e & 0xFFFFu;
                const int c = (int)xc[em_x_off(r, wd & 63u)];
                for (uint32_t h = 0; h < H; h++) {
                    const QFmt fw = a.w[h];
                    const int maxw = (1 << (fw.iwl + fw.frac)) - 1;
                    const int cc = count_code((uint32_t)c, fw.frac, maxw);
                    const int8_t *th = tt + (size_t)h * 2u * Dp * K;
                    const int ka = (int)th[em_tt_off(K, 0, lane, wd)], kc = (int)th[em_tt_off(K, 1, lane, wd)];
                    if (__any(qm_mul_code(cc, ka, fw.frac, maxw) != c * ka || qm_mul_code(cc, kc, fw.frac, maxw) != c * kc)) fix_rows[h] |= 1u << r;
                }
            }
            nd_seen = nd;
            QM_CLK(5);                                                   // 5: fragment read + repeated-word check
        }
        wsync();                                                         // the staging tile rewrites chunk bytes
        QM_CLK(6);
        // ---- per hop: the products, the epilogue, the stores ---------------------------------------------------------------
        for (uint32_t h = 0; h < H; h++) {
            QM_MARK("products (MFMA)");
            const int8_t *th = tt + (size_t)h * 2u * Dp * K;
            const QFmt fw = a.w[h], f_att = a.att[h], f_act = a.act[h];
            const bool kmz = (a.key_mz >> h) & 1u;
            const int maxw = (1 << (fw.iwl + fw.frac)) - 1;
            i32x4 acc[2][4];
#pragma unroll
            for (uint32_t t = 0; t < 2; t++)
#pragma unroll
                for (uint32_t cb = 0; cb < 4; cb++) {
                    acc[t][cb] = i32x4{0, 0, 0, 0};
#pragma unroll
                    for (uint32_t ks = 0; ks < KS; ks++) {
                        const i32x4 am = *(const i32x4 *)(th + em_tt_off(K, t, cb * 16u + nrow, ks * 64u + kq * 16u));
                        acc[t][cb] = __builtin_amdgcn_mfma_i32_16x16x64_i8(am, bx[ks], acc[t][cb], 0, 0, 0);
                    }
                }
            QM_CLK(7);                                                   // 7: 32 fragment reads + MFMAs issued
            QM_MARK("epilogue: quantise, stage, rows back");
            i32x4 rows[2];
#pragma unroll
            for (uint32_t t = 0; t < 2; t++) {
                const QFmt dstf = t ? f_act : f_att;
                const uint32_t qk = (a.qkinds >> (4u * h + 2u * t)) & 3u;    // (workgroup-uniform)
#pragma unroll
                for (uint32_t cb = 0; cb < 4; cb++) {
                    const i32x4 v = acc[t][cb];                              // v[r]: story row nrow, column 16 cb + 4 kq + r
                    const s16x2 x01 = __builtin_bit_cast(s16x2, __builtin_amdgcn_perm((uint32_t)v[1], (uint32_t)v[0], 0x05040100u));
                    const s16x2 x23 = __builtin_bit_cast(s16x2, __builtin_amdgcn_perm((uint32_t)v[3], (uint32_t)v[2], 0x05040100u));
                    uint32_t out;
                    if (qk != kQkGeneral) {
                        out = ew_to_bytes4(x01, x23, maxw, qk);
                    } else {
                        const uint32_t b01 = ew_to_bytes(x01, maxw, fw, dstf, t == 0 && kmz), b23 = ew_to_bytes(x23, maxw, fw, dstf, t == 0 && kmz);
                        out = __builtin_amdgcn_perm(b23, b01, 0x06040200u);
                    }
                    *(uint32_t *)(xs + nrow * SP + cb * 16u + kq * 4u) = out;
                }
                // a row whose repeated word leaves the format: its sums term by term, Qw(Qw(count) . kw) over the row's distinct
                // words (from the tile's word list; the time slot sets its word's count to 1), lane = column
                for (uint32_t m = fix_rows[h]; m; m &= m - 1) {
                    const uint32_t r = (uint32_t)__builtin_ctz(m);
                    uint32_t last_r = 0;
                    for (uint32_t j = 0; j < nw; j++) last_r = wl[r * 16u + j] != 0xFFFFu ? j + 1u : last_r;
                    int sum = 0;
                    for (uint32_t j = 0; j < nw; j++) {
                        const uint32_t wj = wl[r * 16u + j];
                        if (wj >= V) continue;
                        bool first = true, timed = false;
                        uint32_t cnt = 0;
                        for (uint32_t k = 0; k < nw; k++) {
                            if (wl[r * 16u + k] != wj) continue;
                            first = first && k >= j;
                            if (a.time_last && k + 1u == last_r) timed = true; else cnt++;
                        }
                        if (!first) continue;
                        if (timed) cnt = 1;
                        sum += qm_mul_code(count_code(cnt, fw.frac, maxw), (int)th[em_tt_off(K, t, lane, wj)], fw.frac, maxw);
                    }
                    __builtin_amdgcn_wave_barrier();                     // (every lane's dword of this row is written)
                    xs[r * SP + lane] = (uint8_t)ew_to_bytes(s16x2{(short)sum, (short)0}, maxw, fw, dstf, t == 0 && kmz);
                }
                QM_CLK(8);                                               // 8: quantise + staging writes (waits for the MFMA results)
                wsync();
                rows[t] = *(const i32x4 *)(xs + srow * SP + spiece * 16u);
                __builtin_amdgcn_wave_barrier();                         // the second table reuses the staging tile
                QM_CLK(9);                                               // 9: rows read back
            }
            if (h + 1u < H) store_rows(h, row0, rows);
            else { pend[0] = rows[0]; pend[1] = rows[1]; pend_row0 = row0; pending = true; }
            QM_CLK(10);                                                  // 10: stores issued
        }
        __builtin_amdgcn_wave_barrier();                                 // the next tile rewrites the chunk bytes and the word list
        QM_MARK("end of tile");
    }
    if (pending) store_rows(H - 1u, pend_row0, pend);
    QM_CLK(11);
    QM_CLK_FLUSH();
}

// question: word entries only (no time entry, sample.c:557-565); u0[j] = Qw0(sum_k Qw0(Qw0(W[j][k]) . Qw0(c_k))),
// written as floats on the Q(w[0]) grid.  Same lane layout as the story kernel: 16 lanes per question.
template <bool TAB_LDS>
__global__ void __launch_bounds__(kBlock)
k_embed_query_idx(const uint16_t *__restrict__ words, const int8_t *__restrict__ t_q, float *__restrict__ u0,
                  uint32_t n_query, uint32_t max_words, uint32_t D, uint32_t Dp, uint32_t V, QFmt fw, uint32_t pe_dim_word)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1), sub = lane & 15u, grp = lane >> 4;
    const uint32_t dw = Dp / 4;
    uint32_t *tab = (uint32_t *)smem;
    if (TAB_LDS) {
#pragma unroll 4                                                 // (eight loads in flight were the kernel's 33rd register)
        for (uint32_t i = tid; i < V * dw; i += kBlock) tab[i] = ((const uint32_t *)t_q)[i];
        __syncthreads();
    }
    const int maxw = (1 << (fw.iwl + fw.frac)) - 1;
    const bool vec_rows = (D & 3u) == 0u && ((uintptr_t)u0 & 15u) == 0u;
    // (a 32-bit query counter, 64-bit only where an address is formed: the kernel fits 32 registers, and its workgroups find room
    // on a CU beside the story embedding's -- model_host.hip runs the two side by side)
    const uint32_t per_pass = gridDim.x * kWaves * 4;
    for (uint32_t q0 = (blockIdx.x * kWaves + tid / kWave) * 4; q0 < n_query; q0 += per_pass) {
        const uint32_t q = q0 + grp;
        const bool q_ok = q < n_query;
        uint32_t w = 0xFFFFu;
        if (q_ok && sub < max_words) w = words[(size_t)q * max_words + sub];
        const bool valid = w != 0xFFFFu && w < V;
        const uint32_t me = w | (valid ? 1u << 16 : 0u);
        // slots past the last valid word of the wavefront's four questions add nothing: the loops below stop there (the word
        // arrays are 8 or 16 slots wide, a bAbI question has 3 .. 5 words)
        uint32_t n_used = 0;
        {
            const uint64_t vm = __ballot(valid);
#pragma unroll
            for (int g4 = 0; g4 < 4; g4++) {
                const uint32_t m = (uint32_t)(vm >> (16 * g4)) & 0xFFFFu;
                const uint32_t n = m ? 32u - (uint32_t)__builtin_clz(m) : 0u;
                n_used = n > n_used ? n : n_used;
            }
        }
        uint32_t cnt = 0;
        bool dup = false, later = false;
        for (uint32_t j = 0; j < n_used; j++) {
            const uint32_t o = (uint32_t)__shfl((int)me, (int)j, 16);
            const bool same = (((o ^ me) & 0xFFFFu) == 0u) && ((o >> 16) & 1u);
            cnt += same ? 1u : 0u;
            dup |= same && j < sub;
            later |= same && j > sub;
        }
        uint32_t pack = (w & 0xFFFFu) | (cnt << 16) | ((valid && !dup) ? 1u << 24 : 0u);
        if (pe_dim_word) {
            // EN_PE (MemN2N/define.h:298): the bag-of-words entry of a question word is SET to the position weight
            // pe_w[word][slot] = 1 + 4 (word / dim_input - 0.5)(slot / dim_word - 0.5) (MemN2N.c:615, float quotients, the
            // rest in double, stored as float; sample.c:559-560), so the last occurrence of a word decides; the term of
            // the word is then Qw(Qw(W) . Qw(weight)).  The slot field carries the weight's code instead of a count.
            const float pw = (float)(1.0 + (4.0 * ((double)((float)w / (float)V) - 0.5)) * ((double)((float)sub / (float)pe_dim_word) - 0.5));
            const uint32_t kx = valid ? (uint32_t)qm_code(pw, fw.iwl, fw.frac) : 0u;
            pack = (w & 0xFFFFu) | (kx << 16) | ((valid && !later) ? 1u << 24 : 0u);
        }
        for (uint32_t c0 = 0; c0 < dw; c0 += 16) {
            const uint32_t c4 = c0 + sub;
            const bool col_ok = c4 < dw;
            int acc[4] = {0, 0, 0, 0};
            for (uint32_t e = 0; e < n_used; e++) {
                const uint32_t pe = (uint32_t)__shfl((int)pack, (int)e, 16);
                if (!((pe >> 24) & 1u) || !col_ok) continue;
                const uint32_t we = pe & 0xFFFFu, ce = (pe >> 16) & 0xFFu;
                const uint32_t t = TAB_LDS ? tab[we * dw + c4] : ((const uint32_t *)t_q)[(size_t)we * dw + c4];
                const int cc = pe_dim_word ? (int)ce : count_code(ce, fw.frac, maxw);
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int kw = (int)(int8_t)(t >> (8 * k));
                    acc[k] += (!pe_dim_word && ce == 1u && (1 << fw.frac) <= maxw) ? kw : qm_mul_code(cc, kw, fw.frac, maxw);   // see k_embed_story_idx
                }
            }
            if (q_ok && col_ok) {
                float o[4];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int v = acc[k] > maxw ? maxw : (acc[k] < -maxw ? -maxw : acc[k]);
                    o[k] = qm_scale_down((float)v, fw.frac);
                }
                if (vec_rows) {                                          // rows of whole 16-byte groups (bAbI: D = 60): one store per lane
                    if (4u * c4 < D) *(float4 *)(u0 + (size_t)q * D + 4u * c4) = float4{o[0], o[1], o[2], o[3]};
                } else {
#pragma unroll
                    for (int k = 0; k < 4; k++)
                        if (4u * c4 + (uint32_t)k < D) u0[(size_t)q * D + 4u * c4 + (uint32_t)k] = o[k];
                }
            }
        }
    }
}

// float [D][V] -> int8 two's-complement codes, transposed to [V][Dp] (padding columns zero)
__global__ void k_quantize_transpose(const float *__restrict__ src, int8_t *__restrict__ dst, uint32_t D, uint32_t V,
                                     uint32_t Dp, QFmt f)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= V * Dp) return;
    const uint32_t v = i / Dp, c = i % Dp;
    dst[i] = (c < D) ? (int8_t)qm_code(src[(size_t)c * V + v], f.iwl, f.frac) : (int8_t)0;
}

// the way back: int8 codes [V][Dp] -> the grid values as a float matrix [D][V] (exact: code . 2^-frac)
__global__ void k_dequantize_transpose(const int8_t *__restrict__ src, float *__restrict__ dst, uint32_t D, uint32_t V,
                                       uint32_t Dp, uint32_t frac)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= D * V) return;
    const uint32_t c = i / V, v = i % V;
    dst[i] = qm_decode((int32_t)src[(size_t)v * Dp + c], frac);
}

static void fill_qkinds(EmbedIdxArgs &a)
{
    a.qkinds = 0;
    for (uint32_t h = 0; h < a.n_hop; h++) {
        a.qkinds |= qkind_of(a.w[h], a.att[h], (a.key_mz >> h) & 1u) << (4u * h);
        a.qkinds |= qkind_of(a.w[h], a.act[h], false) << (4u * h + 2u);
    }
    if (qm_tuning().embed_general_epilogue) a.qkinds = 0xFFFFFFFFu;     // A/B: ew_to_bytes everywhere
}

// ---- which kernel form a story-embedding call takes: the ONE decision (the launcher switches over it, qmann_embed_story_idx_form
// reports it).  No HIP call, no state but qm_tuning(). --------------------------------------------------------------------------
static inline uint32_t em_dict_k(uint32_t V) { return V <= 64u ? 64u : (V <= 128u ? 128u : 256u); }   // dictionary padded to the MFMA's K step
// LDS of the gather-sum kernel: all 2 . n_hop tables as int16 [V + 1][Dp]; the per-wavefront word scratch
static inline size_t ew_tab_lds(const qmann_net *net) { return (size_t)net->n_hop * 2 * (net->dim_input + 1u) * net->dim_emb_pad * 2u; }
static inline size_t ew_wave_lds() { return (size_t)kWaves * kEwWaveBytes; }

static int embed_story_form(const qmann_net *net, const uint16_t *words, uint32_t max_words)
{
    if (!net) return QMANN_EINVAL;
    if (net->n_hop == 0 || net->n_hop > QMANN_MAX_HOP || net->dim_emb > net->dim_emb_pad) return QMANN_EINVAL;
    if (max_words == 0 || max_words > (uint32_t)kMaxWords) return QMANN_ERANGE;
    for (uint32_t h = 0; h < net->n_hop; h++)
        if (!qm_fmt8(net->act[h]) || !qm_fmt8(net->w[h]) || !qm_fmt8(net->att[h])) return QMANN_ERANGE;
    if (net->dim_emb_pad & 3u) return QMANN_EINVAL;
    if (net->dim_emb_pad % 64 != 0) return QMANN_EUNSUPPORTED;          // 16 lanes x 4 columns per round
    // dictionaries of up to 256 entries with 1.0 representable in every weight format: the matrix-core kernels
    bool mfma_ok = net->dim_input <= 256 && net->dim_emb_pad == 64 && (max_words & 3u) == 0u && ((uintptr_t)words & 7u) == 0u &&
                   !qm_tuning().embed_valu;
    for (uint32_t h = 0; h < net->n_hop; h++) mfma_ok = mfma_ok && net->w[h].iwl >= 1;
    if (mfma_ok) {
        // joint-task dictionaries, several hops: every hop of a tile in one workgroup; QMANN_EMBED_PER_HOP keeps a workgroup per hop (A/B)
        // (64-entry dictionaries -- task 1 -- gain nothing from it: 444 against 443 M q/s in an interleaved A/B with the K = 64
        // instantiation at six wavefronts per SIMD; they keep a workgroup per hop)
        if (em_dict_k(net->dim_input) == 256u && net->n_hop >= 2u && net->n_hop <= 3u && !qm_tuning().embed_per_hop) return QMANN_EMBED_MFMA_ALL_HOPS;
        return QMANN_EMBED_MFMA_PER_HOP;
    }
    // small dictionaries: all tables in LDS as int16; larger ones are gathered from L2 (for dictionaries whose tables
    // exceed LDS both alternatives to L2 gathers were measured on the 20-task joint set in round 1 and were slower:
    // staging one hop's tables at a time, and one copy per CU shared by a 1024-thread workgroup)
    return ew_tab_lds(net) + ew_wave_lds() <= 64 * 1024 ? QMANN_EMBED_GATHER_LDS : QMANN_EMBED_GATHER_L2;
}

}  // namespace

extern "C" {

#ifdef QM_STAGE_CLOCKS
// debug builds only (tools/stage_clocks.py): the per-stage shader-cycle sums of the instrumented kernels of this file, then cleared
int qmann_debug_stage_clocks(unsigned long long *out, int n)
{
    unsigned long long h[kQmClkStages] = {};
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(qm_stage_clk), sizeof h) != hipSuccess) return -1;
    for (int i = 0; i < n && i < kQmClkStages; i++) out[i] = h[i];
    unsigned long long z[kQmClkStages] = {};
    if (hipMemcpyToSymbol(HIP_SYMBOL(qm_stage_clk), z, sizeof z) != hipSuccess) return -1;
    return kQmClkStages;
}
#endif

int qmann_quantize_table_i8(const float *w, int8_t *table, uint32_t dim_emb, uint32_t dim_emb_pad, uint32_t dim_input,
                            qmann_fmt fmt, void *stream)
{
    QmBatched qm_scope;
    if (!w || !table || dim_emb > dim_emb_pad) return QMANN_EINVAL;
    if (!qm_fmt8(fmt)) return QMANN_ERANGE;
    const uint32_t n = dim_input * dim_emb_pad;
    if (n == 0) return QMANN_OK;
    k_quantize_transpose<<<(n + 255) / 256, 256, 0, (hipStream_t)stream>>>(w, table, dim_emb, dim_input, dim_emb_pad,
                                                                         qm_qfmt(fmt));
    QM_LAUNCH_CHECK();
    return qm_scope.rc();
}

int qmann_dequantize_table_f32(const int8_t *table, float *w, uint32_t dim_emb, uint32_t dim_emb_pad, uint32_t dim_input,
                               qmann_fmt fmt, void *stream)
{
    QmBatched qm_scope;
    if (!w || !table || dim_emb > dim_emb_pad) return QMANN_EINVAL;
    if (!qm_fmt8(fmt)) return QMANN_ERANGE;
    const uint32_t n = dim_input * dim_emb;
    if (n == 0) return QMANN_OK;
    k_dequantize_transpose<<<(n + 255) / 256, 256, 0, (hipStream_t)stream>>>(table, w, dim_emb, dim_input, dim_emb_pad, fmt.frac);
    QM_LAUNCH_CHECK();
    return qm_scope.rc();
}

int qmann_embed_story_idx(const qmann_net *net, const uint16_t *words, uint32_t rows_total, uint32_t max_words,
                          int time_last, const int8_t *const *t_a, const int8_t *const *t_c, int8_t *keys, int8_t *vals,
                          size_t hop_stride, void *stream)
{
    QmBatched qm_scope;
    if (!net || (!words && rows_total) || !t_a || !t_c || !keys || !vals) return QMANN_EINVAL;   // (no rows: no word array needed)
    if (net->n_hop == 0 || net->n_hop > QMANN_MAX_HOP || net->dim_emb > net->dim_emb_pad) return QMANN_EINVAL;
    if (max_words == 0 || max_words > (uint32_t)kMaxWords) return QMANN_ERANGE;
    if (hop_stride < (size_t)rows_total * net->dim_emb_pad) return QMANN_EINVAL;
    EmbedIdxArgs a{};
    a.words = words; a.keys = keys; a.vals = vals; a.hop_stride = hop_stride;
    a.n_hop = net->n_hop; a.D = net->dim_emb; a.Dp = net->dim_emb_pad; a.V = net->dim_input; a.rows = rows_total;
    a.max_words = max_words; a.time_last = time_last ? 1u : 0u;
    for (uint32_t h = 0; h < net->n_hop; h++) {
        if (!t_a[h] || !t_c[h]) return QMANN_EINVAL;
        if (!qm_fmt8(net->act[h]) || !qm_fmt8(net->w[h]) || !qm_fmt8(net->att[h])) return QMANN_ERANGE;
        a.t_a[h] = t_a[h]; a.t_c[h] = t_c[h];
    }
    fill_key_formats(a, net);
    fill_qkinds(a);
    if (rows_total == 0) return QMANN_OK;
    if ((net->dim_emb_pad & 3u) || (hop_stride & 3u) || ((uintptr_t)keys & 3u) || ((uintptr_t)vals & 3u)) return QMANN_EINVAL;
    const int form = embed_story_form(net, words, max_words);           // (what is left to refuse: a width that is no multiple of 64)
    if (form < 0) return form;
    hipStream_t st = (hipStream_t)stream;
    const uint32_t Dp = net->dim_emb_pad;
    switch (form) {
    case QMANN_EMBED_MFMA_ALL_HOPS: {
        // every hop of a tile in one workgroup, X built once per tile in chunks (k_embed_story_mfma_hops)
        constexpr uint32_t nwh = 16u, K = 256u;
        const size_t tiles = ((size_t)rows_total + kEmRows - 1) / kEmRows;
        const size_t lds = (size_t)net->n_hop * 2u * Dp * K + (size_t)nwh * (2u * kEmRows * 64u + kEmDupCap * 4u + 16u + kEmRows * 32u);
        qm_launch_persistent(k_embed_story_mfma_hops<16, 4, 4>, (uint32_t)((tiles + nwh - 1) / nwh), QmPersistent{nwh, 4u}, lds, st, a);
        break;
    }
    case QMANN_EMBED_MFMA_PER_HOP: {
        const uint32_t K = em_dict_k(net->dim_input);
        const size_t tiles = ((size_t)rows_total + kEmRows - 1) / kEmRows;
        // T^T (2 x 64 x K bytes) is per workgroup: large dictionaries share it among 16 wavefronts
        const uint32_t nwv = K == 64 ? 8u : 16u;
        const size_t lds = 2u * (size_t)Dp * K + (size_t)nwv * (kEmRows * K + kEmRows * (Dp + 16u) + kEmDupCap * 4u + 16u);
        // persistent in x: never more workgroups than are resident at once (rt.h: through round 3 the cap was LDS-only and
        // rounded UP -- 86 x 3 = 258 workgroups for 256 one-per-CU slots on the joint dictionaries, 1 026 for 512 on task 1)
        qm_dispatch<64, 128, 256>(K, [&](auto k) {
            constexpr int KS = decltype(k)::value / 64, NW = KS == 1 ? 8 : 16;
            qm_launch_persistent(k_embed_story_mfma<KS, NW>, (uint32_t)((tiles + nwv - 1) / nwv),
                                 QmPersistent{NW, (unsigned)em_waves_per_simd(KS), 0, net->n_hop}, lds, st, a);
        });
        break;
    }
    case QMANN_EMBED_GATHER_LDS: {                                        // (118 registers: four wavefronts per SIMD)
        const uint32_t need = (rows_total + kWaves * 4 - 1) / (kWaves * 4);
        qm_launch_persistent(k_embed_story_idx<true>, need, QmPersistent{kWaves, 4}, ew_tab_lds(net) + ew_wave_lds(), st, a);
        break;
    }
    case QMANN_EMBED_GATHER_L2: {
        const uint32_t need = (rows_total + kWaves * 4 - 1) / (kWaves * 4);
        qm_launch_persistent(k_embed_story_idx<false>, need, QmPersistent{kWaves, 4}, ew_wave_lds(), st, a);
        break;
    }
    default:
        return QMANN_EINVAL;
    }
    QM_LAUNCH_CHECK();
    return qm_scope.rc();
}

int qmann_embed_story_idx_form(const qmann_net *net, const uint16_t *words, uint32_t max_words)
{
    return embed_story_form(net, words, max_words);
}

int qmann_embed_query_idx(const qmann_net *net, const uint16_t *words, uint32_t max_words, const int8_t *t_q, float *u0,
                          uint32_t n_query, void *stream)
{
    QmBatched qm_scope;
    if (!net || !words || !t_q || !u0) return QMANN_EINVAL;
    if (max_words == 0 || max_words > (uint32_t)kMaxWords) return QMANN_ERANGE;
    if (!qm_fmt8(net->w[0])) return QMANN_ERANGE;
    if (n_query == 0) return QMANN_OK;
    if (net->dim_emb_pad & 3u) return QMANN_EINVAL;
    if (n_query > 0xFFF00000u) return QMANN_ERANGE;       // (the kernel's 32-bit query counter steps past n_query by up to a grid's worth)
    const uint32_t need = (n_query + kWaves * 4 - 1) / (kWaves * 4);
    const uint32_t blocks = need < 2048u ? need : 2048u;
    const size_t tab_lds = (size_t)net->dim_input * net->dim_emb_pad;
    const QFmt fw = qm_qfmt(net->w[0]);
    if (net->en_pe && net->pe_dim_word == 0) return QMANN_EINVAL;
    const uint32_t pe_dw = net->en_pe ? net->pe_dim_word : 0u;
    if (tab_lds <= kLdsDefaultLimit)
        k_embed_query_idx<true><<<blocks, kBlock, tab_lds, (hipStream_t)stream>>>(
            words, t_q, u0, n_query, max_words, net->dim_emb, net->dim_emb_pad, net->dim_input, fw, pe_dw);
    else
        k_embed_query_idx<false><<<blocks, kBlock, 0, (hipStream_t)stream>>>(
            words, t_q, u0, n_query, max_words, net->dim_emb, net->dim_emb_pad, net->dim_input, fw, pe_dw);
    QM_LAUNCH_CHECK();
    return qm_scope.rc();
}

}  // extern "C"
