// model_host.hip -- include/qmann_model.h: host-side C++ that owns a model's device parameters and
// runs the whole test-phase forward of a batch through the batched kernels.  No kernels here.
//
// The parameters live in ONE device allocation, the "parameter blob": a header (dimensions, formats, options: the
// qmann_net), the int8 embedding tables, the sign-magnitude linear-map codes and the float answer matrix -- i.e. the
// QUANTISED model, position independent (offsets, no pointers).  It is what a multi-GPU host broadcasts
// (qmann_dist.h: one ncclBroadcast of these bytes) and what qmann_model_create_from_params builds a replica from,
// with no float embedding matrix and no re-quantisation on the receiving side.
#include "qfmt.h"
#include "rt.h"
#include "../../include/qmann_model.h"

#include <new>
#include <stdlib.h>
#include <string.h>
#include <vector>

namespace {

constexpr uint32_t kBlobMagic = 0x42504D51u;        // "QMPB"
constexpr uint32_t kBlobVersion = 1u;
constexpr size_t kBlobAlign = 256;

struct BlobHeader {
    uint32_t magic, version;
    uint64_t bytes;                                  // the whole blob, header included
    uint32_t tied, reserved;
    qmann_net net;                                   // lin_map pointers are null in a blob (offsets below)
    uint64_t off_tq, off_ta[QMANN_MAX_HOP], off_tc[QMANN_MAX_HOP], off_lm[QMANN_MAX_HOP], off_wans;
};

size_t align_up(size_t x) { return (x + kBlobAlign - 1) & ~(kBlobAlign - 1); }

// section offsets of a model of these dimensions; returns the blob size
size_t blob_layout(const qmann_net &n, BlobHeader *h)
{
    const size_t tab = align_up((size_t)n.dim_input * n.dim_emb_pad), lm = align_up((size_t)n.dim_emb * n.dim_emb_pad);
    size_t o = align_up(sizeof(BlobHeader));
    auto take = [&](size_t bytes) { const size_t at = o; o += bytes; return (uint64_t)at; };
    const uint64_t tq = take(tab);
    uint64_t ta[QMANN_MAX_HOP] = {}, tc[QMANN_MAX_HOP] = {}, l[QMANN_MAX_HOP] = {};
    for (uint32_t i = 0; i < n.n_hop; i++) { ta[i] = take(tab); tc[i] = take(tab); }
    for (uint32_t i = 0; i < n.n_hop; i++) l[i] = n.en_lin_map ? take(lm) : 0;
    const uint64_t wa = take(align_up((size_t)n.dim_input * n.dim_emb * sizeof(float)));
    if (h) {
        h->off_tq = tq; h->off_wans = wa;
        for (uint32_t i = 0; i < QMANN_MAX_HOP; i++) { h->off_ta[i] = ta[i]; h->off_tc[i] = tc[i]; h->off_lm[i] = l[i]; }
        h->bytes = o;
    }
    return o;
}

// the calling thread's current device for the length of a call into a device-bound model
struct DeviceScope {
    int prev = -1;
    bool changed = false;
    explicit DeviceScope(int device)
    {
        if (device < 0) return;
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != device) { QM_HIP(hipSetDevice(device)); changed = true; }
    }
    ~DeviceScope() { if (changed && prev >= 0) (void)hipSetDevice(prev); }
    DeviceScope(const DeviceScope &) = delete;
};

}  // namespace

struct qmann_model {
    qmann_net net{};
    qmann_net emb_net{};     // formats the embedding kernels quantise the memories to (see bind_sections)
    uint32_t H = 0, D = 0, Dp = 0, V = 0;
    int device = 0;          // the GPU the parameters and the workspace live on; every call runs there
    // Layer-wise weight tying (TYPE_WEIGHT_TYING 2, MemN2N/define.h:287: after every update the reference copies hop 0's
    // embedding matrices over the other hops', MemN2N.c:1770-1773): with equal formats on every hop the hops' memories
    // are the same bytes, so they are embedded ONCE and every hop reads the one plane (hop stride 0)
    bool tied = false;
    // the parameter blob (one allocation) and the sections inside it
    uint8_t *blob = nullptr;
    size_t blob_bytes = 0;
    const float *w_ans = nullptr;
    const int8_t *t_q = nullptr, *t_a[QMANN_MAX_HOP] = {}, *t_c[QMANN_MAX_HOP] = {};
    // float matrices [D][V] for the float embedding kernels (bag-of-words rows that are no plain bags of words): the grid
    // values of the tables, made on the first qmann_model_forward_bow
    float *w_q = nullptr, *w_a[QMANN_MAX_HOP] = {}, *w_c[QMANN_MAX_HOP] = {};
    // workspace, grown on demand
    int8_t *keys = nullptr, *vals = nullptr;
    uint64_t *planes = nullptr;
    float *u0 = nullptr, *u = nullptr;
    // bag-of-words input: word lists made from the rows, the rows that are no plain bags of words, two counters
    uint16_t *bow_words = nullptr;
    uint32_t *bow_irr = nullptr;
    size_t cap_rows = 0, cap_plane_words = 0, cap_query = 0, cap_bow = 0;
    // the memorised knowledge base (qmann_model_memorize_words): its own buffers beside the per-batch workspace above, which the
    // forward calls regrow and overwrite.  int8 memories of every hop (one plane when tied); for V0 / V1 models the packed key
    // planes as well -- the asks then read mem_planes and mem_vals.  mem_rows = 0: nothing memorised
    int8_t *mem_keys = nullptr, *mem_vals = nullptr;
    uint64_t *mem_planes = nullptr;
    uint32_t mem_rows = 0;
    size_t mem_cap_rows = 0;
    // qmann_model_enable_split_asks / _packed: the workspace of qmann_hops_shared_split_i8 / _split_packed (a model has one
    // attention mode, hence one of the two), allocated by that call and never inside an ask; split_bytes = 0: the mode is off
    void *split_ws = nullptr;
    size_t split_bytes = 0;
    // qmann_model_enable_float_asks: a QMANN_ATT_FLOAT model may memorise a memory and ask it through qmann_hops_shared_float_i8
    bool float_asks = false;
    uint32_t last_n_query = 0;   // queries of the last forward that enqueued an answer layer (qmann_model_last_topk ranks m->u's rows)
    bool answer_exact = false;   // rt.h::qm_model_answer_exact: the float answer layer keeps the serial order of additions
};

namespace {

bool packed_mode(const qmann_net &n) { return n.attention_mode == QMANN_ATT_HAMMING_V0 || n.attention_mode == QMANN_ATT_HAMMING_V1; }

// false when the allocation failed (the pointer is then null and the caller must not record the new capacity)
template <typename T>
bool regrow(T **p, size_t n)
{
    if (*p) QM_HIP(hipFree(*p));
    *p = nullptr;
    const hipError_t e = hipMalloc((void **)p, (n ? n : 1) * sizeof(T));
    if (e != hipSuccess) {
        fprintf(stderr, "[*E] HIP : qmann_model workspace of %zu bytes : %s\n", (n ? n : 1) * sizeof(T), hipGetErrorString(e));
        (void)hipGetLastError();
        *p = nullptr;
        return false;
    }
    return true;
}

// Asks of at most this many questions take the split call although the memory fits LDS.  NOT MEASURED (tools/shared_split_ab.py,
// DESIGN.md section 5 "Measured, shared plane, split"): 0 = only memories that do not fit LDS take it.
constexpr uint32_t kSplitAskMaxQueries = 0;
// The same for packed memories (qmann_hops_shared_split_packed).  Measured at 10 000 slots only (tools/shared_split_ham_ab.py,
// DESIGN.md section 5 "Measured, shared plane, split, Hamming"): there the split call beats the unsplit one beyond the two spreads
// at EVERY batch size for V1 (128 x 8 bits) and only from 1 024 questions up for V0 (256 x 1 bit), where it loses 8 to 17 % below
// 64 -- so no threshold "small batches take the split call" holds for both, and shorter memories are NOT MEASURED.  It stays 0:
// only memories that do not fit LDS take the split call.  (A rule by mode and length is the follow-up the table asks for.)
constexpr uint32_t kSplitAskPackedMaxQueries = 0;

// a Hamming model the packed shared-plane calls accept (what qmann_hops_shared_packed would refuse, said ahead of a launch)
bool packed_model_ok(const qmann_model *m)
{
    const qmann_net &n = m->net;
    if (!packed_mode(n)) return false;
    const uint32_t nb = n.num_bit;
    if ((nb != 1 && nb != 2 && nb != 4 && nb != 8) || (m->Dp / 64) * nb * 8 < 16) return false;
    for (uint32_t h = 0; h < m->H; h++)
        if (n.att[h].iwl + n.att[h].frac != 7 || n.att[h].iwl < 1) return false;
    return true;
}

// one query's LDS in the unsplit shared-plane call of the model's mode, and its share of a split call's workspace
size_t ask_lds_bytes(const qmann_model *m, uint32_t n_rows)
{
    if (m->net.attention_mode == QMANN_ATT_FLOAT) return qmann_hops_shared_float_lds_bytes(n_rows, 1);      // (a float per slot)
    return packed_mode(m->net) ? qmann_hops_shared_packed_lds_bytes(&m->net, n_rows, 1) : qmann_hops_shared_lds_bytes(n_rows, 1);
}
size_t ask_split_share(const qmann_model *m, uint32_t n_rows)
{
    return packed_mode(m->net) ? qmann_hops_shared_split_packed_ws_bytes(&m->net, n_rows, 1) : qmann_hops_shared_split_ws_bytes(&m->net, n_rows, 1);
}

// does an ask of the memorised memory go through the split call of the model's mode?  (split_bytes is non-zero only on a model
// whose mode has one: the two enable calls see to that)
bool ask_splits(const qmann_model *m, uint32_t n_rows, uint32_t n_query)
{
    if (!m->split_bytes) return false;
    const size_t share = ask_split_share(m, n_rows);
    if (!share || share > m->split_bytes) return false;
    return ask_lds_bytes(m, n_rows) > kHopLdsLimit || n_query <= (packed_mode(m->net) ? kSplitAskPackedMaxQueries : kSplitAskMaxQueries);
}

// the two enable calls (they differ in `served`, the models each accepts -- never a float model: ask_words_impl relies on it):
// the workspace replaced by one of scratch_bytes (0: none), a memory that can no longer be asked forgotten
int enable_split_asks(qmann_model *m, bool (*served)(const qmann_model *), size_t scratch_bytes, void *stream)
{
    QmBatched qm_scope;
    if (!m) return QMANN_EINVAL;
    if (!served(m)) return QMANN_EUNSUPPORTED;
    DeviceScope on(m->device);
    if (m->split_ws) {
        QM_HIP(hipStreamSynchronize((hipStream_t)stream));  // asks enqueued on it may still use the workspace that goes
        QM_HIP(hipFree(m->split_ws));
    }
    m->split_ws = nullptr;
    m->split_bytes = 0;
    if (scratch_bytes) {
        const hipError_t e = hipMalloc(&m->split_ws, scratch_bytes);
        if (e != hipSuccess) {
            fprintf(stderr, "[*E] HIP : qmann_model split workspace of %zu bytes : %s\n", scratch_bytes, hipGetErrorString(e));
            (void)hipGetLastError();
            m->split_ws = nullptr;
        } else {
            m->split_bytes = scratch_bytes;
        }
    }
    // a memory only the split call can attend to, and no (or too small a) workspace for it: forgotten
    if (m->mem_rows && ask_lds_bytes(m, m->mem_rows) > kHopLdsLimit && !ask_splits(m, m->mem_rows, 1)) m->mem_rows = 0;
    return (scratch_bytes && !m->split_ws) ? QMANN_EHIP : qm_scope.rc();
}

float *upload(const float *host, size_t n, hipStream_t st)
{
    float *d = nullptr;
    QM_HIP(hipMalloc((void **)&d, n * sizeof(float)));
    if (!d) return nullptr;                  // (recorded by QM_HIP: the entry point returns QMANN_EHIP)
    QM_HIP(hipMemcpyAsync(d, host, n * sizeof(float), hipMemcpyHostToDevice, st));
    return d;
}

// Everything a net must satisfy to be created -- and therefore to be replicated: qmann_model_create_on() and the blob receivers
// (qmann_params_validate, qmann_model_create_from_params) run this SAME check, so a net the root can build is never refused on
// a receiver after the broadcast has run, and a bad one fails on the root before any collective.
int check_net(const qmann_net *net)
{
    if (net->n_hop == 0 || net->n_hop > QMANN_MAX_HOP || net->dim_emb == 0 || net->dim_emb > net->dim_emb_pad || net->dim_input == 0)
        return QMANN_EINVAL;
    if (net->dim_emb_pad != 64 && net->dim_emb_pad != 128 && net->dim_emb_pad != 256) return QMANN_EUNSUPPORTED;
    const qmann_net &n = *net;
    switch (n.attention_mode) {
    case QMANN_ATT_FLOAT: case QMANN_ATT_FIXED: case QMANN_ATT_APPX: case QMANN_ATT_HAMMING_V0: case QMANN_ATT_HAMMING_V1: break;
    default: return QMANN_EINVAL;
    }
    if (n.softmax_base > QMANN_SOFTMAX_EXP_PLAN || n.en_lin_map > 1u || n.num_bit > 8u || n.softmax_shift_based > 1u ||
        n.en_att_scale > 1u || n.en_non_linearity > 1u || n.en_pe > 1u)
        return QMANN_EINVAL;
    auto fmt_ok = [](qmann_fmt f) { return f.iwl + f.frac <= 7u && f.iwl <= 7u; };
    for (uint32_t h = 0; h < n.n_hop; h++)
        if (!fmt_ok(n.act[h]) || !fmt_ok(n.w[h]) || !fmt_ok(n.att[h])) return QMANN_EINVAL;
    if (!fmt_ok(n.bin)) return QMANN_EINVAL;
    return QMANN_OK;
}

// a blob header as it must be: what qmann_params_validate answers and qmann_model_create_from_params relies on
int check_header(const BlobHeader &hd, size_t bytes)
{
    if (hd.magic != kBlobMagic || hd.version != kBlobVersion || hd.bytes != bytes || hd.tied > 1u || hd.reserved != 0u) return QMANN_EINVAL;
    const int rc = check_net(&hd.net);
    if (rc != QMANN_OK) return rc;
    const qmann_net &n = hd.net;
    for (uint32_t h = 0; h < n.n_hop; h++)
        if (n.lin_map[h] != nullptr) return QMANN_EINVAL;             // a blob carries offsets, never pointers
    BlobHeader want = hd;
    if (blob_layout(n, &want) != bytes || memcmp(&want, &hd, sizeof hd) != 0) return QMANN_EINVAL;   // offsets must be the canonical ones
    return QMANN_OK;
}

// dimensions, the embedding formats and the section pointers of a model whose blob is in place
void bind_sections(qmann_model *m, const BlobHeader &h)
{
    m->net = h.net;
    m->emb_net = h.net;
    // mode 1 runs its attention on the embedding outputs as they are (weight grid, no attention
    // re-quantisation: lib/layer.c:177-195 forces f_fixed = false on both dot_mat_vec layers)
    if (h.net.attention_mode == QMANN_ATT_FLOAT)
        for (uint32_t i = 0; i < h.net.n_hop; i++) m->emb_net.att[i] = m->emb_net.act[i] = h.net.w[i];
    m->H = h.net.n_hop; m->D = h.net.dim_emb; m->Dp = h.net.dim_emb_pad; m->V = h.net.dim_input;
    m->tied = h.tied != 0;
    if (m->tied) m->emb_net.n_hop = 1;       // the embedding kernels fill one plane
    m->blob_bytes = (size_t)h.bytes;
    m->t_q = (const int8_t *)(m->blob + h.off_tq);
    m->w_ans = (const float *)(m->blob + h.off_wans);
    for (uint32_t i = 0; i < m->H; i++) {
        m->t_a[i] = (const int8_t *)(m->blob + h.off_ta[i]);
        m->t_c[i] = (const int8_t *)(m->blob + h.off_tc[i]);
        m->net.lin_map[i] = h.net.en_lin_map ? (const int8_t *)(m->blob + h.off_lm[i]) : nullptr;
    }
    for (uint32_t i = m->H; i < QMANN_MAX_HOP; i++) m->net.lin_map[i] = nullptr;
}

// Packed planes pay off when they are smaller than the bytes (num_bit < 8), the memory is long enough for bandwidth to
// matter, AND a plane is read more than once: packing reads every key byte once more and writes the planes, so with a plane
// per hop (each read by its own hop only) the packed path moves 2 + num_bit/4 bytes per key byte where the byte form moves 2
// (embedding store + one scan).  Only tied hops -- one plane scanned by every hop -- win: 2 + (1 + H) num_bit/8 against 1 + H.
// Otherwise the same scores come straight from the int8 keys (the V0 / V1 byte forms).  A plane row must fill a 16-byte load
// (qmann_hops_packed refuses Dp = 64 with a single plane: 8 bytes per row): that case takes the byte form too.
bool use_planes(const qmann_model *m, uint32_t max_slots)
{
    return packed_mode(m->net) && m->net.num_bit < 8 && max_slots > 64 && (m->Dp / 64) * m->net.num_bit * 8 >= 16 && m->tied && m->H > 1;
}

// the question side of the workspace: u0 and u of n_query queries
int ensure_queries(qmann_model *m, uint32_t n_query)
{
    if (n_query > m->cap_query || !m->u0 || !m->u) {
        const size_t cap = (size_t)n_query + n_query / 4;
        m->cap_query = 0;
        const bool ok_0 = regrow(&m->u0, cap * m->D), ok_u = regrow(&m->u, cap * m->D);
        if (!ok_0 || !ok_u) return QMANN_EHIP;
        m->cap_query = cap;
    }
    return QMANN_OK;
}

int ensure(qmann_model *m, size_t rows, uint32_t n_query, bool planes)
{
    // A capacity is recorded only when every buffer it describes exists: after a failed allocation the next call tries again
    // (the test is on every pointer, not only the first of a group) and this one returns QMANN_EHIP.
    const size_t n_plane = m->tied ? 1 : m->H;          // hop planes held
    if (rows > m->cap_rows || !m->keys || !m->vals) {   // (a first batch may hold no rows at all: the planes still exist)
        const size_t cap = rows + rows / 4 + 1;
        m->cap_rows = 0;
        const bool ok_k = regrow(&m->keys, n_plane * cap * m->Dp), ok_v = regrow(&m->vals, n_plane * cap * m->Dp);
        if (!ok_k || !ok_v) return QMANN_EHIP;
        m->cap_rows = cap;
    }
    if (planes) {
        const size_t words = n_plane * m->cap_rows * (m->Dp / 64) * m->net.num_bit;
        if (words > m->cap_plane_words || !m->planes) {
            m->cap_plane_words = 0;
            if (!regrow(&m->planes, words)) return QMANN_EHIP;
            m->cap_plane_words = words;
        }
    }
    return ensure_queries(m, n_query);
}

// the float matrices of the float embedding kernels: the tables' grid values (qmann_dequantize_table_f32)
int ensure_float_matrices(qmann_model *m, void *stream)
{
    if (m->w_q) return QMANN_OK;
    const size_t DV = (size_t)m->D * m->V;
    float *all = nullptr;
    if (!regrow(&all, DV * (1 + 2 * (size_t)m->H))) return QMANN_EHIP;
    int rc = qmann_dequantize_table_f32(m->t_q, all, m->D, m->Dp, m->V, m->net.w[0], stream);
    for (uint32_t h = 0; h < m->H && rc == QMANN_OK; h++) {
        float *a = all + DV * (1 + 2 * (size_t)h), *c = a + DV;
        rc = qmann_dequantize_table_f32(m->t_a[h], a, m->D, m->Dp, m->V, m->net.w[h], stream);
        if (rc == QMANN_OK) rc = qmann_dequantize_table_f32(m->t_c[h], c, m->D, m->Dp, m->V, m->net.w[h], stream);
        m->w_a[h] = a; m->w_c[h] = c;
    }
    if (rc != QMANN_OK) { QM_HIP(hipFree(all)); for (uint32_t h = 0; h < m->H; h++) m->w_a[h] = m->w_c[h] = nullptr; return rc; }
    m->w_q = all;                            // (owns the one allocation)
    return QMANN_OK;
}

// The end of every forward and ask, behind its hops: the float answer layer on m->u (`exact`: the serial-order kernels), then the
// HIP failures the call's scope has seen, then last_n_query -- set only where all of it succeeded.
int answer_and_finish(qmann_model *m, const QmBatched &scope, bool exact, uint32_t n_query, const uint32_t *answer, uint32_t *pred,
                      float *cost, uint32_t *match, void *stream)
{
    int rc = (exact ? qmann_answer_f32_serial : qmann_answer_f32)(&m->net, m->w_ans, m->u, answer, pred, nullptr, cost, match, n_query, stream);
    if (!rc) rc = scope.rc();
    if (!rc) m->last_n_query = n_query;
    return rc;
}

// the top fields of rt.h::QmHopHints for the forward_words_top calls (top_float: the float form), as the caller gave them
QmHopHints top_hints(bool top_float, uint32_t k, uint32_t *top_slot, float *top_p)
{
    QmHopHints t;
    t.top_on = true; t.top_float = top_float; t.top_k = k; t.top_slot = top_slot; t.top_p = top_p;
    return t;
}

// hops + answer on the memories sitting in the workspace (hop planes rows_total . Dp apart; one shared plane when tied), and the
// forward's last steps (answer_and_finish).
// `split_ws`: the batch's index lists where with_side_branch below has made them, else null.
// `top`: the attended slots of qmann_model_forward_words_top (top_hints), or null.
int hops_and_answer(qmann_model *m, const QmBatched &scope, uint32_t rows_total, const uint32_t *row_off, uint32_t max_slots, uint32_t n_query,
                    const uint32_t *answer, uint32_t *pred, float *cost, uint32_t *match, void *stream, uint32_t *split_ws,
                    const QmHopHints *top = nullptr)
{
    const size_t hop_stride = m->tied ? 0 : (size_t)rows_total * m->Dp;
    QmHopHints hints = top ? *top : QmHopHints{};
    hints.plane_rows = rows_total;                   // (a tied model passes hop_stride = 0: the hop kernels still learn the plane's size)
    hints.split_ws = split_ws;
    int rc;
    if (use_planes(m, max_slots)) {
        const size_t key_hop_stride = m->tied ? 0 : (size_t)rows_total * (m->Dp / 64) * m->net.num_bit * 8;
        rc = qmann_pack_bitplanes(m->keys, m->planes, (size_t)(m->tied ? 1 : m->H) * rows_total, m->Dp, m->net.num_bit, stream);
        if (rc) return rc;
        rc = qm_hops_packed(&m->net, m->planes, key_hop_stride, m->vals, hop_stride, row_off, max_slots, m->u0, m->u,
                            nullptr, n_query, stream, hints);
    } else {
        rc = qm_hops_i8(&m->net, m->keys, m->vals, hop_stride, row_off, max_slots, m->u0, m->u, nullptr, n_query, stream, hints);
    }
    if (rc) return rc;
    return answer_and_finish(m, scope, m->answer_exact, n_query, answer, pred, cost, match, stream);
}

// The embedding step of a forward: `story(stream)` on the caller's stream and -- for large batches -- `question(side stream)`
// BESIDE it on a second stream (forked and joined by events: one ordered step to the caller's stream, both branches to a stream
// capture).  The story kernels are latency-bound persistent grids that leave 32 .. 80 registers per SIMD lane unallocated; the
// question kernel is built to fit 32 (batch_embed_idx.hip) and is bound by its own stores, so its workgroups run in that room.
// Launched AFTER the story kernel, so that one keeps its full residency.  Behind the question, still beside the story embedding,
// the two index lists of a batch that the hop launch will split by story length (rt.h::qm_hops_will_split; they depend on
// row_off alone; 12 us of memset + kernel + launch gaps off the caller's stream): *split_ws, null where there are none.
template <typename Story, typename Question>
int with_side_branch(const qmann_model *m, uint32_t rows_total, const uint32_t *row_off, uint32_t max_slots, uint32_t n_query, void *stream,
                     uint32_t **split_ws, Story &&story, Question &&question, bool may_split = true)
{
    hipStream_t st = (hipStream_t)stream;
    QmSide *sd = (n_query >= kQmCorunMinQueries && !qm_tuning().no_corun) ? qm_side_stream(st) : nullptr;
    if (sd) {
        QM_HIP(hipEventRecord(sd->fork, st));
        QM_HIP(hipStreamWaitEvent(sd->side, sd->fork, 0));
    }
    const int rc = story(stream);
    const int rc_q = question(sd ? (void *)sd->side : stream);
    *split_ws = nullptr;
    if (sd && !rc_q && may_split && !use_planes(m, max_slots) && qm_hops_will_split(&m->net, rows_total, max_slots, n_query))
        *split_ws = qm_split_early(row_off, n_query, max_slots, st, sd->side);
    if (sd) {                                            // (joined on every path: a capture must not end with an open branch)
        QM_HIP(hipEventRecord(sd->join, sd->side));
        QM_HIP(hipStreamWaitEvent(st, sd->join, 0));
    }
    return rc ? rc : rc_q;
}

int resolve_device(int device, int *out)
{
    if (device < 0) return hipGetDevice(out) == hipSuccess ? QMANN_OK : QMANN_EHIP;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return QMANN_EHIP;
    if (device >= n) return QMANN_EINVAL;
    *out = device;
    return QMANN_OK;
}

}  // namespace

extern "C" {

int qmann_model_create_on(qmann_model **out, int device, const qmann_net *net, const qmann_weights *w, void *stream)
{
    QmBatched qm_scope;
    if (!out || !net || !w) return QMANN_EINVAL;
    *out = nullptr;
    int rc = check_net(net);
    if (rc) return rc;
    if (w->n_hop != net->n_hop || w->dim_emb != net->dim_emb || w->dim_input != net->dim_input) return QMANN_EINVAL;
    if (!w->w_q || !w->w_ans) return QMANN_EINVAL;
    for (uint32_t h = 0; h < net->n_hop; h++)
        if (!w->w_a[h] || !w->w_c[h] || (net->en_lin_map && !w->w_h[h])) return QMANN_EINVAL;
    int dev = 0;
    if ((rc = resolve_device(device, &dev)) != QMANN_OK) return rc;
    DeviceScope on(dev);

    qmann_model *m = new (std::nothrow) qmann_model();
    if (!m) return QMANN_ERANGE;
    m->device = dev;
    BlobHeader hd{};
    hd.magic = kBlobMagic; hd.version = kBlobVersion;
    hd.net = *net;
    for (uint32_t h = 0; h < QMANN_MAX_HOP; h++) hd.net.lin_map[h] = nullptr;
    blob_layout(*net, &hd);
    const uint32_t H = net->n_hop, D = net->dim_emb, Dp = net->dim_emb_pad, V = net->dim_input;
    const size_t DV = (size_t)D * V, DD = (size_t)D * D;
    // tied embedding matrices (see the struct); mode 1 compares the formats its embedding really uses
    bool tied = H > 1 && !qm_tuning().no_tied;
    for (uint32_t h = 1; h < H && tied; h++) {
        const bool fl = net->attention_mode == QMANN_ATT_FLOAT;
        const qmann_fmt a0 = fl ? net->w[0] : net->att[0], ah = fl ? net->w[h] : net->att[h];
        const qmann_fmt c0 = fl ? net->w[0] : net->act[0], ch = fl ? net->w[h] : net->act[h];
        tied = net->w[h].iwl == net->w[0].iwl && net->w[h].frac == net->w[0].frac && ah.iwl == a0.iwl && ah.frac == a0.frac &&
               ch.iwl == c0.iwl && ch.frac == c0.frac &&
               memcmp(w->w_a[h], w->w_a[0], DV * sizeof(float)) == 0 && memcmp(w->w_c[h], w->w_c[0], DV * sizeof(float)) == 0;
    }
    hd.tied = tied ? 1u : 0u;

    hipStream_t st = (hipStream_t)stream;
    QM_HIP(hipMalloc((void **)&m->blob, (size_t)hd.bytes));
    if (!m->blob) { delete m; return QMANN_EHIP; }
    QM_HIP(hipMemsetAsync(m->blob, 0, (size_t)hd.bytes, st));                 // (padding bytes are part of what is broadcast)
    QM_HIP(hipMemcpyAsync(m->blob, &hd, sizeof hd, hipMemcpyHostToDevice, st));
    bind_sections(m, hd);
    std::vector<float *> staged;             // float copies needed only for the conversions below
    auto table = [&](const float *host, const int8_t *dst, qmann_fmt f) {
        float *d = upload(host, DV, st);
        if (!d) return (int)QMANN_EHIP;
        staged.push_back(d);
        return qmann_quantize_table_i8(d, (int8_t *)dst, D, Dp, V, f, stream);
    };
    rc = table(w->w_q, m->t_q, net->w[0]);                                    // emb_q uses the first hop's format (MemN2N.c:826)
    for (uint32_t h = 0; h < H && rc == QMANN_OK; h++) {
        rc = table(w->w_a[h], m->t_a[h], net->w[h]);
        if (rc == QMANN_OK) rc = table(w->w_c[h], m->t_c[h], net->w[h]);
        if (rc == QMANN_OK && net->en_lin_map) {
            float *wh = upload(w->w_h[h], DD, st);
            if (!wh) { rc = QMANN_EHIP; break; }
            staged.push_back(wh);
            rc = qmann_quantize_i8(wh, (int8_t *)m->net.lin_map[h], D, D, Dp, net->w[h], QMANN_CODE_SIGNMAG, stream);
        }
    }
    if (rc == QMANN_OK) QM_HIP(hipMemcpyAsync((void *)m->w_ans, w->w_ans, DV * sizeof(float), hipMemcpyHostToDevice, st));
    QM_HIP(hipStreamSynchronize(st));        // the host arrays and the staged floats are free again
    for (float *p : staged) QM_HIP(hipFree(p));
    if (qm_scope.rc() != QMANN_OK) rc = qm_scope.rc();     // (a failed allocation shows up as EHIP, not as the EINVAL of the null it left)
    if (rc != QMANN_OK) { qmann_model_destroy(m); return rc; }
    *out = m;
    return QMANN_OK;
}

int qmann_model_create(qmann_model **out, const qmann_net *net, const qmann_weights *w, void *stream)
{
    return qmann_model_create_on(out, -1, net, w, stream);
}

int qmann_model_create_from_params(qmann_model **out, int device, const void *blob, size_t bytes, void *stream)
{
    QmBatched qm_scope;
    if (!out || !blob || bytes < sizeof(BlobHeader)) return QMANN_EINVAL;
    *out = nullptr;
    int dev = 0, rc;
    if ((rc = resolve_device(device, &dev)) != QMANN_OK) return rc;
    DeviceScope on(dev);
    hipStream_t st = (hipStream_t)stream;
    BlobHeader hd;
    QM_HIP(hipMemcpyAsync(&hd, blob, sizeof hd, hipMemcpyDefault, st));
    QM_HIP(hipStreamSynchronize(st));
    if (qm_scope.rc()) return qm_scope.rc();
    if ((rc = check_header(hd, bytes)) != QMANN_OK) return rc;

    qmann_model *m = new (std::nothrow) qmann_model();
    if (!m) return QMANN_ERANGE;
    m->device = dev;
    QM_HIP(hipMalloc((void **)&m->blob, bytes));
    if (!m->blob) { delete m; return QMANN_EHIP; }
    QM_HIP(hipMemcpyAsync(m->blob, blob, bytes, hipMemcpyDefault, st));       // (same device, a peer device, or host memory)
    QM_HIP(hipStreamSynchronize(st));
    bind_sections(m, hd);
    if (qm_scope.rc()) { qmann_model_destroy(m); return qm_scope.rc(); }
    *out = m;
    return QMANN_OK;
}

int qmann_params_validate(const void *host_blob, size_t bytes, qmann_net *net)
{
    if (!host_blob || bytes < sizeof(BlobHeader)) return QMANN_EINVAL;
    BlobHeader hd;
    memcpy(&hd, host_blob, sizeof hd);
    const int rc = check_header(hd, bytes);
    if (rc == QMANN_OK && net) *net = hd.net;
    return rc;
}

void qmann_model_destroy(qmann_model *m)
{
    if (!m) return;
    DeviceScope on(m->device);
    auto drop = [](void *p) { if (p) QM_HIP(hipFree(p)); };
    drop(m->blob); drop(m->w_q);             // (w_a / w_c point into w_q's allocation)
    drop(m->mem_keys); drop(m->mem_vals); drop(m->mem_planes); drop(m->split_ws);
    drop(m->keys); drop(m->vals); drop(m->planes); drop(m->u0); drop(m->u); drop(m->bow_words); drop(m->bow_irr);
    delete m;
}

int qmann_model_device(const qmann_model *m) { return m ? m->device : -1; }

int qmann_model_params(const qmann_model *m, const void **blob, size_t *bytes)
{
    if (!m || !blob || !bytes) return QMANN_EINVAL;
    *blob = m->blob; *bytes = m->blob_bytes;
    return QMANN_OK;
}

int qmann_model_net(const qmann_model *m, qmann_net *net, const float **w_ans)
{
    if (!m || !net) return QMANN_EINVAL;
    *net = m->net;
    if (w_ans) *w_ans = m->w_ans;
    return QMANN_OK;
}

// qmann_model_forward_words (top null), qmann_model_forward_words_top and qmann_model_forward_words_top_float (the top fields of
// `top` as the caller gave them; top_float: the float form)
static int forward_words_impl(qmann_model *m, const uint16_t *story_words, uint32_t rows_total, uint32_t max_words,
                              const uint16_t *question_words, uint32_t max_q_words, const uint32_t *row_off,
                              uint32_t max_slots, uint32_t n_query, const uint32_t *answer, uint32_t *pred,
                              float *cost, uint32_t *match, void *stream, const QmHopHints *top)
{
    QmBatched qm_scope;
    if (!m) return QMANN_EINVAL;
    if (n_query == 0) return QMANN_OK;                  // (an empty batch needs no arrays)
    m->last_n_query = 0;                                // (set again where this call succeeds)
    if ((!story_words && rows_total) || !question_words || !row_off || !pred) return QMANN_EINVAL;   // (every story may be empty)
    if (top) {
        // what qmann_hops_top_i8 would refuse behind its base call, said here ahead of any launch: the modes and lengths it does
        // not serve, then its own arguments.  (Beyond 64 slots only fixed-point models pass: the packed-plane route is never taken.)
        // qmann_hops_top_float_i8 serves float attention at every length its base call does, and nothing else.
        const uint32_t am = m->net.attention_mode;
        if (top->top_float ? am != QMANN_ATT_FLOAT : am == QMANN_ATT_FLOAT) return QMANN_EUNSUPPORTED;
        if (!top->top_float && am != QMANN_ATT_FIXED && max_slots > 64) return QMANN_EUNSUPPORTED;
        if (top->top_k < 1 || top->top_k > (uint32_t)QMANN_MAX_TOP_SLOTS || !top->top_slot || !top->top_p) return QMANN_EINVAL;
    }
    DeviceScope on(m->device);
    int rc = ensure(m, rows_total, n_query, use_planes(m, max_slots));
    if (rc) return rc;
    uint32_t *split_ws;
    rc = with_side_branch(m, rows_total, row_off, max_slots, n_query, stream, &split_ws,
        [&](void *s) { return qmann_embed_story_idx(&m->emb_net, story_words, rows_total, max_words, 1, m->t_a, m->t_c, m->keys, m->vals, (size_t)rows_total * m->Dp, s); },
        [&](void *s) { return qmann_embed_query_idx(&m->net, question_words, max_q_words, m->t_q, m->u0, n_query, s); },
        !top);                                              // (the top call's hop launch is never split by story length)
    if (rc) return rc;
    return hops_and_answer(m, qm_scope, rows_total, row_off, max_slots, n_query, answer, pred, cost, match, stream, split_ws, top);
}

int qmann_model_forward_words(qmann_model *m, const uint16_t *story_words, uint32_t rows_total, uint32_t max_words,
                              const uint16_t *question_words, uint32_t max_q_words, const uint32_t *row_off,
                              uint32_t max_slots, uint32_t n_query, const uint32_t *answer, uint32_t *pred,
                              float *cost, uint32_t *match, void *stream)
{
    return forward_words_impl(m, story_words, rows_total, max_words, question_words, max_q_words, row_off, max_slots, n_query,
                              answer, pred, cost, match, stream, nullptr);
}

int qmann_model_forward_words_top(qmann_model *m, const uint16_t *story_words, uint32_t rows_total, uint32_t max_words,
                                  const uint16_t *question_words, uint32_t max_q_words, const uint32_t *row_off,
                                  uint32_t max_slots, uint32_t n_query, const uint32_t *answer, uint32_t *pred,
                                  float *cost, uint32_t *match, uint32_t k, uint32_t *top_slot, float *top_p, void *stream)
{
    const QmHopHints top = top_hints(false, k, top_slot, top_p);
    return forward_words_impl(m, story_words, rows_total, max_words, question_words, max_q_words, row_off, max_slots, n_query,
                              answer, pred, cost, match, stream, &top);
}

int qmann_model_forward_words_top_float(qmann_model *m, const uint16_t *story_words, uint32_t rows_total, uint32_t max_words,
                                        const uint16_t *question_words, uint32_t max_q_words, const uint32_t *row_off,
                                        uint32_t max_slots, uint32_t n_query, const uint32_t *answer, uint32_t *pred,
                                        float *cost, uint32_t *match, uint32_t k, uint32_t *top_slot, float *top_p, void *stream)
{
    const QmHopHints top = top_hints(true, k, top_slot, top_p);
    return forward_words_impl(m, story_words, rows_total, max_words, question_words, max_q_words, row_off, max_slots, n_query,
                              answer, pred, cost, match, stream, &top);
}

int qmann_model_forward_shared_words(qmann_model *m, const uint16_t *story_words, uint32_t n_rows, uint32_t max_words,
                                     const uint16_t *question_words, uint32_t max_q_words, uint32_t n_query,
                                     const uint32_t *answer, uint32_t *pred, float *cost, uint32_t *match, void *stream)
{
    QmBatched qm_scope;
    if (!m) return QMANN_EINVAL;
    if (n_query == 0) return QMANN_OK;
    m->last_n_query = 0;                                // (set again where this call succeeds)
    if (!story_words || !question_words || !pred) return QMANN_EINVAL;
    if (m->net.attention_mode != QMANN_ATT_FIXED) return QMANN_EUNSUPPORTED;     // (what qmann_hops_shared_i8 covers)
    if (n_rows == 0) return QMANN_EINVAL;
    DeviceScope on(m->device);
    int rc = ensure(m, n_rows, n_query, false);             // ONE memory of n_rows rows, whatever the number of questions
    if (rc) return rc;
    // everything on the caller's stream: the one story is a few rows, there is nothing to run beside it
    const size_t plane = (size_t)n_rows * m->Dp;
    rc = qmann_embed_story_idx(&m->emb_net, story_words, n_rows, max_words, 1, m->t_a, m->t_c, m->keys, m->vals, plane, stream);
    if (rc) return rc;
    rc = qmann_embed_query_idx(&m->net, question_words, max_q_words, m->t_q, m->u0, n_query, stream);
    if (rc) return rc;
    rc = qmann_hops_shared_i8(&m->net, m->keys, m->vals, m->tied ? 0 : plane, n_rows, m->u0, m->u, nullptr, n_query, stream);
    if (rc) return rc;
    return answer_and_finish(m, qm_scope, false, n_query, answer, pred, cost, match, stream);     // (this call has always ignored answer_exact)
}

int qmann_model_memorize_words(qmann_model *m, const uint16_t *story_words, uint32_t n_rows, uint32_t max_words, void *stream)
{
    QmBatched qm_scope;
    if (!m) return QMANN_EINVAL;
    const qmann_net &n = m->net;
    const bool packed = packed_mode(n);
    const bool fl = n.attention_mode == QMANN_ATT_FLOAT && m->float_asks;           // (qmann_model_enable_float_asks)
    if (!packed && !fl && n.attention_mode != QMANN_ATT_FIXED) return QMANN_EUNSUPPORTED;      // (what the shared-plane hop calls cover)
    if (packed && !packed_model_ok(m)) return QMANN_EUNSUPPORTED;       // what qmann_hops_shared_packed would refuse, said here
    if (!story_words || n_rows == 0) return QMANN_EINVAL;
    // the memory's length against LDS now, so that an ask cannot fail late
    const size_t lds = ask_lds_bytes(m, n_rows);
    // (with split asks enabled a memory may be longer: then one query's share of the workspace must fit the budget)
    if (lds > kHopLdsLimit && !(n_rows <= (1u << 24) && ask_splits(m, n_rows, 1))) return QMANN_ERANGE;
    DeviceScope on(m->device);
    m->mem_rows = 0;                                         // (a failure below leaves nothing memorised)
    const size_t n_plane = m->tied ? 1 : m->H;
    if (n_rows > m->mem_cap_rows || !m->mem_keys || !m->mem_vals || (packed && !m->mem_planes)) {
        const size_t cap = n_rows;
        m->mem_cap_rows = 0;
        const bool ok_k = regrow(&m->mem_keys, n_plane * cap * m->Dp), ok_v = regrow(&m->mem_vals, n_plane * cap * m->Dp);
        const bool ok_p = !packed || regrow(&m->mem_planes, n_plane * cap * (m->Dp / 64) * n.num_bit);
        if (!ok_k || !ok_v || !ok_p) return QMANN_EHIP;
        m->mem_cap_rows = cap;
    }
    const size_t plane = (size_t)n_rows * m->Dp;
    int rc = qmann_embed_story_idx(&m->emb_net, story_words, n_rows, max_words, 1, m->t_a, m->t_c, m->mem_keys, m->mem_vals, plane, stream);
    if (rc) return rc;
    if (packed) {
        rc = qmann_pack_bitplanes(m->mem_keys, m->mem_planes, n_plane * n_rows, m->Dp, n.num_bit, stream);
        if (rc) return rc;
    }
    if (qm_scope.rc()) return qm_scope.rc();
    m->mem_rows = n_rows;
    return QMANN_OK;
}

// qmann_model_ask_words (kAskPlain), qmann_model_ask_words_top (kAskTop: fixed-point models),
// qmann_model_ask_words_top_packed (kAskTopPacked: Hamming V0 / V1 models) and qmann_model_ask_words_top_float (kAskTopFloat:
// float models with float asks enabled); k, top_slot, top_p as the top calls take them
enum AskTop { kAskPlain, kAskTop, kAskTopPacked, kAskTopFloat };
static int ask_words_impl(qmann_model *m, const uint16_t *question_words, uint32_t max_q_words, uint32_t n_query,
                          const uint32_t *answer, uint32_t *pred, float *cost, uint32_t *match, AskTop top, uint32_t k,
                          uint32_t *top_slot, float *top_p, void *stream)
{
    QmBatched qm_scope;
    if (!m) return QMANN_EINVAL;
    if (m->mem_rows == 0) { m->last_n_query = 0; return QMANN_EINVAL; }
    if (n_query == 0) return QMANN_OK;
    m->last_n_query = 0;                                // (set again where this call succeeds)
    if (!question_words || !pred) return QMANN_EINVAL;
    if (top) {                                          // behind the base call's refusals, and here: an ask must not fail behind its embedding
        // (float attention has a form of its own, qmann_hops_shared_top_float_i8: that one serves float models only, the other two none)
        if ((m->net.attention_mode == QMANN_ATT_FLOAT) != (top == kAskTopFloat)) return QMANN_EUNSUPPORTED;
        if (top != kAskTopFloat && packed_mode(m->net) != (top == kAskTopPacked)) return QMANN_EUNSUPPORTED;     // each form serves its own models
        if (k == 0 || k > QMANN_MAX_TOP_SLOTS || !top_slot || !top_p) return QMANN_EINVAL;
    }
    DeviceScope on(m->device);
    int rc = ensure_queries(m, n_query);
    if (rc) return rc;
    const uint32_t S = m->mem_rows;
    const size_t plane = m->tied ? 0 : (size_t)S * m->Dp;
    rc = qmann_embed_query_idx(&m->net, question_words, max_q_words, m->t_q, m->u0, n_query, stream);
    if (rc) return rc;
    const qmann_net *net = &m->net;
    const bool packed = packed_mode(m->net), fl = net->attention_mode == QMANN_ATT_FLOAT;
    const size_t key_plane = plane / m->Dp * (m->Dp / 64) * m->net.num_bit * 8;     // (packed: bytes of one hop's key planes)
    // Float models never split: both enable calls refuse them, so they have no workspace -- and no split call exists to pick.
    const bool split = !fl && ask_splits(m, S, n_query);
    // THE place that picks an ask's hop call -- by family (float, packed, fixed-point), top and split -- for questions q0 .. q0 + nq
    auto hops = [&](uint32_t q0, uint32_t nq) {
        const float *u0 = m->u0 + (size_t)q0 * m->D;
        float *u = m->u + (size_t)q0 * m->D;
        const size_t row0 = (size_t)q0 * m->H * k;         // (top: the chunk's own block of rows)
        uint32_t *ts = top_slot + row0;
        float *tp = top_p + row0;
        void *ws = m->split_ws;
        const size_t wb = m->split_bytes;
        if (fl)
            return top ? qmann_hops_shared_top_float_i8(net, m->mem_keys, m->mem_vals, plane, S, u0, u, k, ts, tp, nq, stream)
                       : qmann_hops_shared_float_i8(net, m->mem_keys, m->mem_vals, plane, S, u0, u, nullptr, nq, stream);
        if (packed) {
            if (split)
                return top ? qmann_hops_shared_split_top_packed(net, m->mem_planes, key_plane, m->mem_vals, plane, S, u0, u, k, ts, tp, nq, 0, ws, wb, stream)
                           : qmann_hops_shared_split_packed(net, m->mem_planes, key_plane, m->mem_vals, plane, S, u0, u, nullptr, nq, 0, ws, wb, stream);
            return top ? qmann_hops_shared_top_packed(net, m->mem_planes, key_plane, m->mem_vals, plane, S, u0, u, k, ts, tp, nq, stream)
                       : qmann_hops_shared_packed(net, m->mem_planes, key_plane, m->mem_vals, plane, S, u0, u, nullptr, nq, stream);
        }
        if (split)
            return top ? qmann_hops_shared_split_top_i8(net, m->mem_keys, m->mem_vals, plane, S, u0, u, k, ts, tp, nq, 0, ws, wb, stream)
                       : qmann_hops_shared_split_i8(net, m->mem_keys, m->mem_vals, plane, S, u0, u, nullptr, nq, 0, ws, wb, stream);
        return top ? qmann_hops_shared_top_i8(net, m->mem_keys, m->mem_vals, plane, S, u0, u, k, ts, tp, nq, stream)
                   : qmann_hops_shared_i8(net, m->mem_keys, m->mem_vals, plane, S, u0, u, nullptr, nq, stream);
    };
    // A split ask: chunks of as many questions as the workspace holds, one after the other on the caller's stream.  An unsplit
    // ask: the same loop with one chunk of all of them.
    const size_t fit = split ? m->split_bytes / ask_split_share(m, S) : n_query;
    const uint32_t chunk = fit < n_query ? (uint32_t)fit : n_query;
    for (uint32_t q0 = 0; q0 < n_query && !rc; q0 += chunk) rc = hops(q0, n_query - q0 < chunk ? n_query - q0 : chunk);
    if (rc) return rc;
    return answer_and_finish(m, qm_scope, m->answer_exact, n_query, answer, pred, cost, match, stream);
}

int qmann_model_ask_words(qmann_model *m, const uint16_t *question_words, uint32_t max_q_words, uint32_t n_query,
                          const uint32_t *answer, uint32_t *pred, float *cost, uint32_t *match, void *stream)
{
    return ask_words_impl(m, question_words, max_q_words, n_query, answer, pred, cost, match, kAskPlain, 0, nullptr, nullptr, stream);
}

int qmann_model_ask_words_top(qmann_model *m, const uint16_t *question_words, uint32_t max_q_words, uint32_t n_query,
                              const uint32_t *answer, uint32_t *pred, float *cost, uint32_t *match, uint32_t k,
                              uint32_t *top_slot, float *top_p, void *stream)
{
    return ask_words_impl(m, question_words, max_q_words, n_query, answer, pred, cost, match, kAskTop, k, top_slot, top_p, stream);
}

int qmann_model_ask_words_top_packed(qmann_model *m, const uint16_t *question_words, uint32_t max_q_words, uint32_t n_query,
                                     const uint32_t *answer, uint32_t *pred, float *cost, uint32_t *match, uint32_t k,
                                     uint32_t *top_slot, float *top_p, void *stream)
{
    return ask_words_impl(m, question_words, max_q_words, n_query, answer, pred, cost, match, kAskTopPacked, k, top_slot, top_p, stream);
}

int qmann_model_ask_words_top_float(qmann_model *m, const uint16_t *question_words, uint32_t max_q_words, uint32_t n_query,
                                    const uint32_t *answer, uint32_t *pred, float *cost, uint32_t *match, uint32_t k,
                                    uint32_t *top_slot, float *top_p, void *stream)
{
    return ask_words_impl(m, question_words, max_q_words, n_query, answer, pred, cost, match, kAskTopFloat, k, top_slot, top_p, stream);
}

uint32_t qmann_model_memory_rows(const qmann_model *m) { return m ? m->mem_rows : 0u; }

int qmann_model_enable_split_asks(qmann_model *m, size_t scratch_bytes, void *stream)
{
    return enable_split_asks(m, [](const qmann_model *x) { return x->net.attention_mode == QMANN_ATT_FIXED; }, scratch_bytes, stream);
}

int qmann_model_enable_float_asks(qmann_model *m, int on)
{
    if (!m) return QMANN_EINVAL;
    if (m->net.attention_mode != QMANN_ATT_FLOAT) return QMANN_EUNSUPPORTED;
    m->float_asks = on != 0;
    if (!on) m->mem_rows = 0;                                // off: the memory is forgotten, memorize_words refuses again
    return QMANN_OK;
}

int qmann_model_enable_split_asks_packed(qmann_model *m, size_t scratch_bytes, void *stream)
{
    return enable_split_asks(m, packed_model_ok, scratch_bytes, stream);
}

int qmann_model_forward_bow(qmann_model *m, const float *story, uint32_t rows_total, const float *question,
                            const uint32_t *row_off, uint32_t max_slots, uint32_t n_query, const uint32_t *answer,
                            uint32_t *pred, float *cost, uint32_t *match, void *stream)
{
    QmBatched qm_scope;
    if (!m) return QMANN_EINVAL;
    if (n_query == 0) return QMANN_OK;
    m->last_n_query = 0;                                // (set again where this call succeeds)
    if ((!story && rows_total) || !question || !row_off || !pred) return QMANN_EINVAL;
    DeviceScope on(m->device);
    int rc = ensure(m, rows_total, n_query, use_planes(m, max_slots));
    if (rc) return rc;
    if ((rc = ensure_float_matrices(m, stream)) != QMANN_OK) return rc;
    // Rows that are plain bags of words (integer counts) go through the word-index kernels -- the int8 gather / matrix-core
    // path, bit-identical to the float path and several times faster; the others (fractional entries: position encoding,
    // long rows) are listed on the device and redone by the float kernels.  No host round trip.
    const size_t n_all = (size_t)rows_total + n_query;
    if (n_all > m->cap_bow || !m->bow_words || !m->bow_irr) {
        const size_t cap = n_all + n_all / 4 + 1;
        m->cap_bow = 0;
        const bool ok_w = regrow(&m->bow_words, cap * 16), ok_i = regrow(&m->bow_irr, cap + 2);
        if (!ok_w || !ok_i) return QMANN_EHIP;
        m->cap_bow = cap;
    }
    uint32_t *n_irr = m->bow_irr, *irr_s = m->bow_irr + 2, *irr_q = irr_s + rows_total;
    uint16_t *sw = m->bow_words, *qw = m->bow_words + (size_t)rows_total * 16;
    QM_HIP(hipMemsetAsync(n_irr, 0, 2 * sizeof(uint32_t), (hipStream_t)stream));
    // Both conversions first, then the embeddings (with_side_branch: the question's beside the story's).  (The question's
    // CONVERSION beside the story's was measured too: 0.735 against 0.714 ms on task 1 -- its workgroups sit on the CUs when the
    // story embedding's persistent grid arrives.)
    const size_t hop_stride = (size_t)rows_total * m->Dp;
    rc = qmann_bow_to_words(story, rows_total, m->V, sw, irr_s, n_irr, stream);
    if (rc) return rc;
    rc = qmann_bow_to_words(question, n_query, m->V, qw, irr_q, n_irr + 1, stream);
    if (rc) return rc;
    uint32_t *split_ws;
    rc = with_side_branch(m, rows_total, row_off, max_slots, n_query, stream, &split_ws,
        [&](void *s) {
            const int e = qmann_embed_story_idx(&m->emb_net, sw, rows_total, 16, /*time_last=*/0, m->t_a, m->t_c, m->keys, m->vals, hop_stride, s);
            return e ? e : qmann_embed_story_rows(&m->emb_net, story, rows_total, irr_s, n_irr, m->w_a, m->w_c, m->keys, m->vals, hop_stride, s);
        },
        [&](void *s) {
            qmann_net qnet = m->net;
            qnet.en_pe = 0;                             // (position weights, if any, are IN the rows: such rows take the float kernel)
            const int e = qmann_embed_query_idx(&qnet, qw, 16, m->t_q, m->u0, n_query, s);
            return e ? e : qmann_embed_query_rows(&m->net, question, irr_q, n_irr + 1, m->w_q, m->u0, n_query, s);
        });
    if (rc) return rc;
    return hops_and_answer(m, qm_scope, rows_total, row_off, max_slots, n_query, answer, pred, cost, match, stream, split_ws);
}

const float *qmann_model_last_u(const qmann_model *m) { return m ? m->u : nullptr; }

uint32_t qmann_model_last_n_query(const qmann_model *m) { return m ? m->last_n_query : 0u; }

int qmann_model_last_topk(qmann_model *m, uint32_t k, uint32_t *top_idx, float *top_p, void *stream)
{
    if (!m || m->last_n_query == 0 || !m->u) return QMANN_EINVAL;
    DeviceScope on(m->device);
    return qmann_answer_topk_f32(&m->net, m->w_ans, m->u, k, top_idx, top_p, m->last_n_query, stream);
}

}  // extern "C"

void qm_model_answer_exact(qmann_model *m, bool exact) { if (m) m->answer_exact = exact; }
