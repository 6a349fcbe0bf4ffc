// batch_embed.hip -- the stage before the hop loop, batched over queries: story / question embedding of float
// bag-of-words rows into int8 memories, and the bag-of-words to word-list conversion.
#include "embed_common.h"

namespace {

// ---------------------------------------------------------------------------
// Story embedding: E[s][j] = Qw( sum_k Qw( Qw(X[s][k]) . Qw(W[j][k]) ) )
// (lib/layer_cuda.cu:105-172 via :3531) for the A and C tables of every hop, then
// re-quantised to the format its consumer applies (keys: att[h], lib/layer_cuda.cu:120;
// values: act[h], :562) and stored as sign-magnitude int8.  X is a bag of words: a handful of
// non-zeros per row, so rows are first compacted to (index, value) pairs in LDS
// and the sum becomes a short gather over table columns.  One workgroup per
// story row; thread j < D owns output column j for all 2.n_hop tables.
// ---------------------------------------------------------------------------
constexpr int kMaxNnz = 64;

// sign-magnitude byte of Q(f)(x): the top byte of the reference's FLOAT2FIXED word
// (`mz`: see ew_to_bytes -- exactly -2^iwl is "minus zero" for the keys of a Hamming-family attention on a wider weight grid)
__device__ __forceinline__ int8_t sm_byte(float x, QFmt f, bool mz = false)
{
    const int k = qm_code(x, f.iwl, f.frac);
    const uint32_t mag = (mz && x == -(float)(1u << f.iwl)) ? 0u : (uint32_t)(k < 0 ? -k : k);
    return (int8_t)(mag | ((x >= 0.0f) ? 0u : 0x80u));
}

struct EmbedArgs {
    const float *story;
    const float *w_a[QMANN_MAX_HOP];
    const float *w_c[QMANN_MAX_HOP];
    int8_t *keys;
    int8_t *vals;
    size_t hop_stride;
    uint32_t n_hop, D, Dp, V, rows;
    QFmt act[QMANN_MAX_HOP], w[QMANN_MAX_HOP], att[QMANN_MAX_HOP];   // att: the format of the KEY BYTES (fill_key_formats)
    uint32_t key_mz;              // bit h: hop h's keys follow the minus-zero rule
    const uint32_t *row_list;     // optional: only these rows (device array; its length is read from *n_list)
    const uint32_t *n_list;
};

__global__ void __launch_bounds__(kBlock)
k_embed_story(const EmbedArgs a)
{
    __shared__ uint32_t nz_idx[kMaxNnz];
    __shared__ float nz_val[kMaxNnz];
    __shared__ uint32_t nnz;
    const uint32_t tid = threadIdx.x;
    const size_t n_it = a.row_list ? (size_t)*a.n_list : (size_t)a.rows;
    for (size_t it = blockIdx.x; it < n_it; it += gridDim.x) {     // grid-stride over story rows
    const size_t s = a.row_list ? (size_t)a.row_list[it] : it;
    const float *x = a.story + s * a.V;
    __syncthreads();
    if (tid == 0) nnz = 0;
    __syncthreads();
    for (uint32_t k = tid; k < a.V; k += kBlock) {
        const float v = x[k];
        if (v != 0.0f) {
            const uint32_t i = atomicAdd(&nnz, 1u);
            if (i < (uint32_t)kMaxNnz) { nz_idx[i] = k; nz_val[i] = v; }
        }
    }
    __syncthreads();
    const uint32_t n = nnz;
    const bool dense = n > (uint32_t)kMaxNnz;       // not a bag of words: fall back to the full row
    for (uint32_t j = tid; j < a.Dp; j += kBlock) {
        for (uint32_t h = 0; h < a.n_hop; h++) {
            const QFmt fw = a.w[h];
            int8_t kcode = 0, vcode = 0;
            if (j < a.D) {
                const float *wa = a.w_a[h] + (size_t)j * a.V;
                const float *wc = a.w_c[h] + (size_t)j * a.V;
                float sa = 0.0f, sc = 0.0f;           // exact: multiples of 2^-frac below 2^24 units
                if (!dense) {
                    for (uint32_t i = 0; i < n; i++) {
                        const uint32_t k = nz_idx[i];
                        sa += qm_fixed_mul(nz_val[i], wa[k], fw, fw);
                        sc += qm_fixed_mul(nz_val[i], wc[k], fw, fw);
                    }
                } else {
                    for (uint32_t k = 0; k < a.V; k++) {
                        sa += qm_fixed_mul(x[k], wa[k], fw, fw);
                        sc += qm_fixed_mul(x[k], wc[k], fw, fw);
                    }
                }
                const float ea = qm_quant(sa, fw.iwl, fw.frac);
                const float ec = qm_quant(sc, fw.iwl, fw.frac);
                kcode = sm_byte(ea, a.att[h], (a.key_mz >> h) & 1u);
                vcode = sm_byte(ec, a.act[h]);
            }
            a.keys[(size_t)h * a.hop_stride + s * a.Dp + j] = kcode;
            a.vals[(size_t)h * a.hop_stride + s * a.Dp + j] = vcode;
        }
    }
    }
}

// Question embedding u0[j] = Qw0( sum_k Qw0( Qw0(W[j][k]) . Qw0(q[k]) ) ) (lib/layer_cuda.cu:49-83 via :3184)
__global__ void __launch_bounds__(kBlock)
k_embed_query(const float *__restrict__ question, const float *__restrict__ w_q, float *__restrict__ u0,
              uint32_t D, uint32_t V, QFmt fw, uint32_t n_query, const uint32_t *__restrict__ row_list,
              const uint32_t *__restrict__ n_list)
{
    __shared__ uint32_t nz_idx[kMaxNnz];
    __shared__ float nz_val[kMaxNnz];
    __shared__ uint32_t nnz;
    const uint32_t tid = threadIdx.x;
    const size_t n_it = row_list ? (size_t)*n_list : (size_t)n_query;
    for (size_t it = blockIdx.x; it < n_it; it += gridDim.x) {     // grid-stride over questions
    const size_t q = row_list ? (size_t)row_list[it] : it;
    const float *x = question + q * V;
    __syncthreads();
    if (tid == 0) nnz = 0;
    __syncthreads();
    for (uint32_t k = tid; k < V; k += kBlock) {
        const float v = x[k];
        if (v != 0.0f) {
            const uint32_t i = atomicAdd(&nnz, 1u);
            if (i < (uint32_t)kMaxNnz) { nz_idx[i] = k; nz_val[i] = v; }
        }
    }
    __syncthreads();
    const uint32_t n = nnz;
    for (uint32_t j = tid; j < D; j += kBlock) {
        const float *wr = w_q + (size_t)j * V;
        float s = 0.0f;
        if (n <= (uint32_t)kMaxNnz) {
            for (uint32_t i = 0; i < n; i++) s += qm_fixed_mul(wr[nz_idx[i]], nz_val[i], fw, fw);
        } else {
            for (uint32_t k = 0; k < V; k++) s += qm_fixed_mul(wr[k], x[k], fw, fw);
        }
        u0[q * D + j] = qm_quant(s, fw.iwl, fw.frac);
    }
    }
}

// ---------------------------------------------------------------------------
// Bag-of-words rows -> word lists.  The reference hands its stories over as float rows of dim_input entries
// (cuda_data_in pools, MemN2N.c:2337-2349) although sample.c knows every sentence as a handful of word indices; a row
// whose non-zero entries are small positive integers (counts; the time entry is a 1) IS such a list, and the word-index
// kernels embed it on the integer / matrix-core path, bit-identical to the float path.  One wavefront per row: the
// non-zeros are compacted in ascending index order, an index repeated by its count; a row that is not a plain bag of
// words (fractional or negative entries -- position encoding --, more than 16 words) gets an empty list and is
// recorded in `irr_rows` for the float kernel to redo.
// ---------------------------------------------------------------------------
// L lanes per row (16 / 32 / 64: the smallest that covers a dictionary of up to 64 words; longer rows take passes of 64),
// 64 / L rows per wavefront.  A pass whose entries are all 0.0 or 1.0 -- every pass of a real bAbI row but the few with a word
// said twice -- takes its positions from one ballot instead of a six-step scan.
template <int L>
__global__ void __launch_bounds__(kBlock)
k_bow_to_words(const float *__restrict__ bow, uint32_t rows, uint32_t V, uint16_t *__restrict__ words,
               uint32_t *__restrict__ irr_rows, uint32_t *__restrict__ n_irr)
{
    constexpr int RPW = kWave / L;
    constexpr uint64_t kGroupMask = L == 64 ? ~0ull : ((1ull << (L & 63)) - 1ull);
    __shared__ __attribute__((aligned(16))) uint16_t buf[kWaves][RPW][24];       // 16 list slots + a dump slot (index 16) for the lanes with nothing to write
    const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave, sub = lane & (L - 1), grp = lane / L;
    const uint64_t below = (1ull << sub) - 1ull;
    for (size_t r0 = ((size_t)blockIdx.x * kWaves + wave) * RPW; r0 < rows; r0 += (size_t)gridDim.x * kWaves * RPW) {
        const size_t r = r0 + grp;
        const bool r_ok = r < rows;
        if (sub < 16) buf[wave][grp][sub] = 0xFFFFu;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        uint32_t base = 0;
        bool bad = false;
        for (uint32_t c0 = 0; c0 < V; c0 += L) {                         // wavefront-uniform
            const uint32_t k = c0 + sub;
            float x = 0.0f;
            if (r_ok && k < V) x = bow[r * V + k];
            // nothing but 0.0 and 1.0 in the pass (told by the bit patterns; the compare's lane mask IS the ballot): positions from
            // the ballot, a branch-free write; anything else -- counts, fractions, -0.0, NaN -- takes the general tests and the scan
            const uint32_t bits = __builtin_bit_cast(uint32_t, x);
            const bool one = bits == 0x3F800000u;
            if (!__any(bits != 0u && !one)) {
                const uint64_t gm = (__ballot(one) >> (grp * L)) & kGroupMask;
                const uint32_t pos = base + (uint32_t)__popcll(gm & below);
                buf[wave][grp][(one && pos < 16u) ? pos : 16u] = (uint16_t)k;
                base += (uint32_t)__popcll(gm);
                continue;
            }
            const bool nz = x != 0.0f;                                   // (a NaN is "non-zero" and fails the next test)
            const int c = (x >= 1.0f && x <= 16.0f) ? (int)x : 0;
            const bool ok = nz && c > 0 && (float)c == x;
            bad |= nz && !ok;
            const uint32_t cnt = ok ? (uint32_t)c : 0u;
            uint32_t incl = cnt;
#pragma unroll
            for (int o = 1; o < L; o <<= 1) {
                const uint32_t t = __shfl_up(incl, o, L);
                if (sub >= (uint32_t)o) incl += t;
            }
            const uint32_t pos = base + incl - cnt;
            for (uint32_t t = 0; t < cnt; t++)
                if (pos + t < 16u) buf[wave][grp][pos + t] = (uint16_t)k;
            base += __shfl(incl, L - 1, L);
        }
        const bool irregular = ((__ballot(bad) >> (grp * L)) & kGroupMask) != 0ull || base > 16u;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (r_ok && sub < 8) ((uint32_t *)(words + r * 16))[sub] = irregular ? 0xFFFFFFFFu : ((const uint32_t *)buf[wave][grp])[sub];
        if (r_ok && irregular && sub == 0) irr_rows[atomicAdd(n_irr, 1u)] = (uint32_t)r;
        __builtin_amdgcn_wave_barrier();                                 // the next rows rewrite the buffer
    }
}

// Dictionaries of more than 64 words (the 20-task set: 238): a lane takes FOUR consecutive entries of the row in one 16-byte
// buffer load (rows are only 4-byte aligned: 952 bytes at V = 238; the resource ends with the array, so the last rows' overhang
// reads as zeros), a pass covers 256 entries, and the next row's load is issued before this row is worked on -- the kernel is
// bound by the float rows it reads (0.96 ms -> see DESIGN.md for 2.44 M rows of 238).  Ascending order = lane-major, then the
// lane's four entries: positions from four ballots (all counts 0 / 1) or from a scan of the lanes' totals.
__global__ void __launch_bounds__(kBlock)
k_bow_to_words_wide(const float *__restrict__ bow, uint32_t rows, uint32_t V, uint16_t *__restrict__ words,
                    uint32_t *__restrict__ irr_rows, uint32_t *__restrict__ n_irr)
{
    __shared__ __attribute__((aligned(16))) uint16_t buf[kWaves][24];    // 16 list slots + a dump slot (index 16) for the lanes with nothing to write
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    const size_t stride = (size_t)gridDim.x * kWaves;
    const size_t row_bytes = (size_t)V * 4u, total = (size_t)rows * row_bytes;
    const uint32_t n_pass = (V + 255u) / 256u;
    // one resource over the whole array while 32-bit offsets reach every row (< 4 GiB: 4.5 M rows of 238); per row beyond
    const bool one_rsrc = total <= 0xFFFFFFFFull;
    const __amdgpu_buffer_rsrc_t rs_all = __builtin_amdgcn_make_buffer_rsrc((void *)bow, 0, (int)(uint32_t)(one_rsrc ? total : 0u), kRawBufferFlags);
    auto request = [&](size_t r, uint32_t pass) -> i32x4 {
        const uint32_t in_row = (pass * 256u + lane * 4u) * 4u;
        // (the row's offset in the VECTOR offset: that is the one the bounds check covers, and the last rows' overhang must read as zeros)
        if (one_rsrc) return __builtin_amdgcn_raw_buffer_load_b128(rs_all, (int)((uint32_t)(r * row_bytes) + in_row), 0, kBufferNt);
        const size_t off = r * row_bytes, left = total - off;           // (wavefront-uniform)
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void *)((const char *)bow + off), 0,
                                                                             (int)(left < 0x7FFFFFFFu ? left : 0x7FFFFFFFu), kRawBufferFlags);
        return __builtin_amdgcn_raw_buffer_load_b128(rs, (int)in_row, 0, kBufferNt);
    };
    size_t r = (size_t)blockIdx.x * kWaves + wave;
    if (r >= rows) return;
    const uint64_t below = (1ull << lane) - 1ull;
    i32x4 x = request(r, 0);
    for (; r < rows; r += stride) {
        if (lane < 16) buf[wave][lane] = 0xFFFFu;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        uint32_t base = 0;
        bool bad = false;
        for (uint32_t pass = 0; pass < n_pass; pass++) {                 // wavefront-uniform
            const i32x4 cur = x;
            // the next load: this row's next pass, or the next row's first
            if (pass + 1u < n_pass) x = request(r, pass + 1u);
            else if (r + stride < rows) x = request(r + stride, 0);
            const uint32_t k0 = pass * 256u + lane * 4u;
            // almost every pass of a real row holds nothing but 0.0 and 1.0: told by the bit patterns, one compare per entry each
            // (its lane mask IS the ballot); anything else -- counts, fractions, -0.0, NaN -- takes the general tests
            uint32_t bits[4];
            bool one[4], other = false;
#pragma unroll
            for (int e = 0; e < 4; e++) {
                // (element by element, a plain `if`: `cond ? bit_cast(cur[e]) : 0` compiled to cur[0] for every e -- hipcc 7.2)
                bits[e] = (uint32_t)cur[e];
                if (k0 + (uint32_t)e >= V) bits[e] = 0u;                 // (past the row's end the load holds the next row's entries)
                one[e] = bits[e] == 0x3F800000u;
                other |= bits[e] != 0u && !one[e];
            }
            if (!__any(other)) {
                const uint64_t m0 = __ballot(one[0]), m1 = __ballot(one[1]), m2 = __ballot(one[2]), m3 = __ballot(one[3]);
                uint32_t pos = base + (uint32_t)(__popcll(m0 & below) + __popcll(m1 & below) + __popcll(m2 & below) + __popcll(m3 & below));
#pragma unroll
                for (int e = 0; e < 4; e++) {                            // no branches: a lane without an entry writes the dump slot
                    buf[wave][(one[e] && pos < 16u) ? pos : 16u] = (uint16_t)(k0 + (uint32_t)e);
                    pos += one[e] ? 1u : 0u;
                }
                base += (uint32_t)(__popcll(m0) + __popcll(m1) + __popcll(m2) + __popcll(m3));
                continue;
            }
            uint32_t cnt[4];
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const float v = __builtin_bit_cast(float, bits[e]);
                const bool nz = v != 0.0f;                               // (a NaN is "non-zero" and fails the next test)
                const int c = (v >= 1.0f && v <= 16.0f) ? (int)v : 0;
                const bool ok = nz && c > 0 && (float)c == v;
                bad |= nz && !ok;
                cnt[e] = ok ? (uint32_t)c : 0u;
            }
            const uint32_t mine = cnt[0] + cnt[1] + cnt[2] + cnt[3];
            uint32_t incl = mine;
#pragma unroll
            for (int o = 1; o < kWave; o <<= 1) {
                const uint32_t t = __shfl_up(incl, o);
                if (lane >= (uint32_t)o) incl += t;
            }
            uint32_t pos = base + incl - mine;
#pragma unroll
            for (int e = 0; e < 4; e++) {
                for (uint32_t t = 0; t < cnt[e]; t++)
                    if (pos + t < 16u) buf[wave][pos + t] = (uint16_t)(k0 + (uint32_t)e);
                pos += cnt[e];
            }
            base += __shfl(incl, kWave - 1);
        }
        const bool irregular = __any(bad) || base > 16u;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (lane < 8) ((uint32_t *)(words + r * 16))[lane] = irregular ? 0xFFFFFFFFu : ((const uint32_t *)buf[wave])[lane];
        if (irregular && lane == 0) irr_rows[atomicAdd(n_irr, 1u)] = (uint32_t)r;
        __builtin_amdgcn_wave_barrier();                                 // the next row rewrites the buffer
    }
}

}  // namespace

extern "C" {

static int embed_story_impl(const qmann_net *net, const float *story, uint32_t rows_total, const uint32_t *row_list,
                            const uint32_t *n_list, const float *const *w_a, const float *const *w_c, int8_t *keys, int8_t *vals,
                            size_t hop_stride, void *stream)
{
    QmBatched qm_scope;
    if (!net || (!story && rows_total) || !w_a || !w_c || !keys || !vals) return QMANN_EINVAL;   // (no rows: no story array needed)
    if ((row_list == nullptr) != (n_list == nullptr)) return QMANN_EINVAL;
    if (net->n_hop == 0 || net->n_hop > QMANN_MAX_HOP || net->dim_emb > net->dim_emb_pad) return QMANN_EINVAL;
    if (hop_stride < (size_t)rows_total * net->dim_emb_pad) return QMANN_EINVAL;
    EmbedArgs a{};
    a.story = story; a.keys = keys; a.vals = vals; a.hop_stride = hop_stride;
    a.n_hop = net->n_hop; a.D = net->dim_emb; a.Dp = net->dim_emb_pad; a.V = net->dim_input; a.rows = rows_total;
    a.row_list = row_list; a.n_list = n_list;
    for (uint32_t h = 0; h < net->n_hop; h++) {
        if (!w_a[h] || !w_c[h]) return QMANN_EINVAL;
        if (!qm_fmt8(net->act[h]) || !qm_fmt8(net->w[h]) || !qm_fmt8(net->att[h])) return QMANN_ERANGE;
        a.w_a[h] = w_a[h]; a.w_c[h] = w_c[h];
    }
    fill_key_formats(a, net);
    if (rows_total == 0) return QMANN_OK;
    // a listed launch does not know the list's length on the host: a fixed grid walks it (and leaves at once if it is empty)
    const uint32_t grid = row_list ? (rows_total < 4096u ? rows_total : 4096u) : (rows_total < (1u << 22) ? rows_total : (1u << 22));
    k_embed_story<<<grid, kBlock, 0, (hipStream_t)stream>>>(a);
    QM_LAUNCH_CHECK();
    return qm_scope.rc();
}

int qmann_embed_story(const qmann_net *net, const float *story, uint32_t rows_total, const float *const *w_a,
                      const float *const *w_c, int8_t *keys, int8_t *vals, size_t hop_stride, void *stream)
{
    return embed_story_impl(net, story, rows_total, nullptr, nullptr, w_a, w_c, keys, vals, hop_stride, stream);
}

int qmann_embed_story_rows(const qmann_net *net, const float *story, uint32_t rows_total, const uint32_t *row_list,
                           const uint32_t *n_list, const float *const *w_a, const float *const *w_c, int8_t *keys,
                           int8_t *vals, size_t hop_stride, void *stream)
{
    if (!row_list || !n_list) return QMANN_EINVAL;
    return embed_story_impl(net, story, rows_total, row_list, n_list, w_a, w_c, keys, vals, hop_stride, stream);
}

static int embed_query_impl(const qmann_net *net, const float *question, const uint32_t *row_list, const uint32_t *n_list,
                            const float *w_q, float *u0, uint32_t n_query, void *stream)
{
    QmBatched qm_scope;
    if (!net || !question || !w_q || !u0) return QMANN_EINVAL;
    if ((row_list == nullptr) != (n_list == nullptr)) return QMANN_EINVAL;
    if (!qm_fmt8(net->w[0])) return QMANN_ERANGE;
    if (n_query == 0) return QMANN_OK;
    if (qm_too_many_queries(n_query)) return QMANN_ERANGE;
    const uint32_t grid = row_list ? (n_query < 4096u ? n_query : 4096u) : n_query;
    k_embed_query<<<grid, kBlock, 0, (hipStream_t)stream>>>(question, w_q, u0, net->dim_emb, net->dim_input,
                                                           qm_qfmt(net->w[0]), n_query, row_list, n_list);
    QM_LAUNCH_CHECK();
    return qm_scope.rc();
}

int qmann_embed_query(const qmann_net *net, const float *question, const float *w_q, float *u0, uint32_t n_query,
                      void *stream)
{
    return embed_query_impl(net, question, nullptr, nullptr, w_q, u0, n_query, stream);
}

int qmann_embed_query_rows(const qmann_net *net, const float *question, const uint32_t *row_list, const uint32_t *n_list,
                           const float *w_q, float *u0, uint32_t n_query, void *stream)
{
    if (!row_list || !n_list) return QMANN_EINVAL;
    return embed_query_impl(net, question, row_list, n_list, w_q, u0, n_query, stream);
}

int qmann_bow_to_words(const float *bow, uint32_t rows, uint32_t dim_input, uint16_t *words, uint32_t *irregular_rows,
                       uint32_t *n_irregular, void *stream)
{
    QmBatched qm_scope;
    if ((!bow && rows) || !words || !irregular_rows || !n_irregular) return QMANN_EINVAL;
    if (dim_input == 0 || dim_input >= 0xFFFFu) return QMANN_ERANGE;          // 0xFFFF marks an unused slot
    if (rows == 0) return QMANN_OK;
    auto go = [&](auto kernel, uint32_t rows_per_wave) {
        const uint32_t per_block = kWaves * rows_per_wave, need = (rows + per_block - 1) / per_block;
        kernel<<<need < 16384u ? need : 16384u, kBlock, 0, (hipStream_t)stream>>>(bow, rows, dim_input, words, irregular_rows, n_irregular);
    };
    if (dim_input <= 16u) go(k_bow_to_words<16>, 4u);
    else if (dim_input <= 32u) go(k_bow_to_words<32>, 2u);
    else if (dim_input <= 64u) go(k_bow_to_words<64>, 1u);
    else go(k_bow_to_words_wide, 1u);
    QM_LAUNCH_CHECK();
    return qm_scope.rc();
}

}  // extern "C"
