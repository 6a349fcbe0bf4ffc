// batch_answer_i8.hip -- the answer layer for an answer matrix on an int8 grid: qmann_answer_i8, qmann_answer_topk_i8 and its
// workspace helper.  Two forms, each plain or ranked (answer_i8.h has the kernels and says why each is exact):
//   one pass     k_answer_i8_part, then a combine kernel: no [n_query][V] logits round trip;
//   two kernels  k_logits_mfma_i8 writes the logits, answer_serial.h's k_answer<true, .> forms the float layer's softmax on them.
#include "answer_i8.h"
#include "answer_serial.h"

namespace {

// What a call does for (net, w_fmt, k, probs wanted, n_query).  Its refusals, in include/qmann_batch.h's order: `rc` (the net, the
// formats, a query's LDS, k), then the ranked call's workspace against `ws_bytes` (the helper's figure, the same for both forms;
// 0 for a dim_emb_pad without a build), then QMANN_OK for n_query = 0, then `rc_batch` (2^24 queries; that dim_emb_pad).
// The rest is set for a batch that runs: small_lpq / small_vpt are k_answer's (two kernels: the float layer's normaliser order).
struct AnsI8Plan {
    int rc, rc_batch;
    size_t ws_bytes, serial_lds;
    uint32_t D, Dp, V, softmax_base, n_query, small_lpq, small_vpt;
    QFmt fu;                    // u is read through the last hop's activation format (it is the last sum_vec output)
    float scale;                // a logit is its integer code times this
    bool one_pass;
    AnsSlices sl;               // one pass: the grid; the workspace is AnsPart [n_slice][n_query], then the ranked keys [n_slice][n_query][k]
};

// w_fmt: null for the workspace helper, which has none; k: null for the plain call
AnsI8Plan answer_i8_plan(const qmann_net *net, const qmann_fmt *w_fmt, const uint32_t *k, bool want_probs, uint32_t n_query)
{
    AnsI8Plan p{};
    const uint32_t D = p.D = net->dim_emb, Dp = p.Dp = net->dim_emb_pad, V = p.V = net->dim_input;
    p.serial_lds = ans_serial_lds(D, V);
    if (D == 0 || V == 0 || Dp % 64 != 0 || D > Dp) p.rc = QMANN_EINVAL;
    else if (!qm_fmt8(net->act[net->n_hop - 1]) || (w_fmt && !qm_fmt8(*w_fmt))) p.rc = QMANN_ERANGE;
    else if (p.serial_lds > kAnsSerialLdsLimit) p.rc = QMANN_ERANGE;
    else if (k && (*k == 0 || *k > QMANN_MAX_TOPK || *k > V)) p.rc = QMANN_EINVAL;
    const bool built = Dp == 64 || Dp == 128 || Dp == 256;   // k_logits_mfma_i8 / k_answer_i8_part<Dp / 64>
    p.rc_batch = qm_too_many_queries(n_query) ? QMANN_ERANGE : built ? QMANN_OK : QMANN_EUNSUPPORTED;
    if (p.rc || !built || n_query == 0) return p;
    const qmann_fmt fu = net->act[net->n_hop - 1];
    p.softmax_base = net->softmax_base, p.n_query = n_query, p.fu = qm_qfmt(fu);
    p.scale = w_fmt ? 1.0f / (float)(1u << (fu.frac + w_fmt->frac)) : 0.0f;
    // (the running-maximum normaliser needs a true exponential: the piece-wise linear exp_plan takes the two-kernel form; so does a
    // dictionary of 1, 2 or 3 answers, whose documented workspace of V floats per query is smaller than one record)
    const bool records_fit = (size_t)V * sizeof(float) >= sizeof(AnsPart);
    p.one_pass = !want_probs && net->softmax_base != QMANN_SOFTMAX_EXP_PLAN && !qm_tuning().answer_two_pass && records_fit;
    p.sl = ans_i8_slices(n_query, V);
    const AnsSmallPlan sp = ans_small_plan(D, V);
    p.small_lpq = sp.fits ? sp.lpq : 0u, p.small_vpt = sp.vpt;
    // (the plain call's records fit its logits_ws: V >= 4 there, and n_slice <= ceil(V / 64) gives 16 n_slice <= 4 V bytes per query)
    const size_t logits = ((size_t)n_query * V * sizeof(float) + 7) & ~(size_t)7;
    const size_t records = (size_t)p.sl.n_slice * n_query * (sizeof(AnsPart) + (k ? *k : 0u) * sizeof(uint64_t));
    p.ws_bytes = (records_fit && records > logits) ? records : logits;
    return p;
}

struct AnsI8Call { const int8_t *w; const float *u; void *ws; AnsOut out; hipStream_t st; };    // (out: all null in the ranked call)

// one pass: the per-slice records go to the workspace, the combine kernel merges them (16 lanes per query)
template <bool TOPK> void answer_i8_one_pass(const AnsI8Plan &p, const AnsI8Call &c, const AnsTopK<TOPK> &tk)
{
    AnsPart *part = (AnsPart *)c.ws;
    AnsTopKI8<TOPK> lists;
    if constexpr (TOPK) lists = AnsTopKI8<true>{(uint64_t *)(part + (size_t)p.sl.n_slice * p.n_query), tk.k};
    qm_dispatch<64, 128, 256>(p.Dp, [&](auto dp) {
        constexpr int KS = decltype(dp)::value / 64;
        qm_dispatch<false, true>(p.softmax_base == QMANN_SOFTMAX_EXP, [&](auto e) {
            qm_launch(k_answer_i8_part<KS, decltype(e)::value, TOPK>, dim3(p.sl.qblocks, p.sl.n_slice), kBlock, 0, c.st,
                      c.u, c.w, part, p.n_query, p.D, p.V, p.fu, p.scale, p.softmax_base, p.sl.tps, lists);
        });
    });
    const uint32_t cb = qm_cdiv(p.n_query * 16, kBlock), grid = cb < 2048u ? cb : 2048u;
    if constexpr (TOPK)
        qm_launch(k_answer_i8_combine_topk, grid, kBlock, 0, c.st, part, lists.keys, tk.idx, tk.p, p.n_query, p.sl.n_slice, tk.k, p.scale, p.softmax_base);
    else
        qm_launch(k_answer_i8_combine, grid, kBlock, 0, c.st, part, c.u, c.w, c.out.answer, c.out.pred, c.out.cost, c.out.match, p.n_query,
                  p.sl.n_slice, p.D, p.Dp, p.V, p.fu, p.scale, p.softmax_base);
}

// two kernels: the logits to the workspace, then k_answer on them -- the normaliser in the order of the float layer's kernel for
// this shape, so the probabilities are bit-identical to it (see k_answer); the ranked build ranks by the logits
template <bool TOPK> void answer_i8_two_kernel(const AnsI8Plan &p, const AnsI8Call &c, const AnsTopK<TOPK> &tk)
{
    float *logits = (float *)c.ws;
    const dim3 grid(qm_cdiv(p.n_query, 16 * kWaves), qm_cdiv(p.V, 16 * kTilesPerBlockY));
    qm_dispatch<64, 128, 256>(p.Dp, [&](auto dp) {
        qm_launch(k_logits_mfma_i8<decltype(dp)::value / 64>, grid, kBlock, 0, c.st, c.u, c.w, logits, p.n_query, p.D, p.V, p.fu, p.scale);
    });
    qm_launch(k_answer<true, TOPK>, ans_serial_grid(p.n_query), kBlock, p.serial_lds, c.st, logits, nullptr, c.out.answer, c.out.pred,
              c.out.probs, c.out.cost, c.out.match, p.D, p.V, p.softmax_base, p.n_query, p.small_lpq, p.small_vpt, tk);
}

template <bool TOPK> int answer_i8_run(const AnsI8Plan &p, const AnsI8Call &c, const AnsTopK<TOPK> &tk)
{
    QmBatched qm_scope;
    if (p.one_pass) answer_i8_one_pass<TOPK>(p, c, tk);
    else answer_i8_two_kernel<TOPK>(p, c, tk);
    QM_LAUNCH_CHECK();
    return qm_scope.rc();
}

}  // namespace

extern "C" {

int qmann_answer_i8(const qmann_net *net, const int8_t *w_ans_i8, qmann_fmt w_fmt, const float *u, float *logits_ws,
                    const uint32_t *answer, uint32_t *pred, float *probs, float *cost, uint32_t *match,
                    uint32_t n_query, void *stream)
{
    if (!net || !w_ans_i8 || !u || !logits_ws || !pred) return QMANN_EINVAL;
    const AnsI8Plan p = answer_i8_plan(net, &w_fmt, nullptr, probs != nullptr, n_query);
    if (p.rc) return p.rc;
    if (n_query == 0) return QMANN_OK;
    if (p.rc_batch) return p.rc_batch;
    return answer_i8_run(p, AnsI8Call{w_ans_i8, u, logits_ws, AnsOut{answer, pred, probs, cost, match}, (hipStream_t)stream}, AnsTopK<false>{});
}

size_t qmann_answer_topk_i8_ws_bytes(const qmann_net *net, uint32_t k, uint32_t n_query)
{
    if (!net || net->n_hop == 0 || net->n_hop > QMANN_MAX_HOP) return 0;
    const AnsI8Plan p = answer_i8_plan(net, nullptr, &k, false, n_query);
    return p.rc ? 0 : p.ws_bytes;
}

int qmann_answer_topk_i8(const qmann_net *net, const int8_t *w_ans_i8, qmann_fmt w_fmt, const float *u, void *ws, size_t ws_bytes,
                         uint32_t k, uint32_t *top_idx, float *top_p, uint32_t n_query, void *stream)
{
    if (!net || !w_ans_i8 || !u || !top_idx || !top_p) return QMANN_EINVAL;
    const AnsI8Plan p = answer_i8_plan(net, &w_fmt, &k, false, n_query);
    if (p.rc) return p.rc;
    if (!ws || ((uintptr_t)ws & 7u) || ws_bytes < p.ws_bytes) return QMANN_EINVAL;
    if (n_query == 0) return QMANN_OK;
    if (p.rc_batch) return p.rc_batch;
    return answer_i8_run(p, AnsI8Call{w_ans_i8, u, ws, AnsOut{}, (hipStream_t)stream}, AnsTopK<true>{top_idx, top_p, k});
}

}  // extern "C"
