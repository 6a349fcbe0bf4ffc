// batch_answer.hip -- the stage after the hop loop, batched over queries: the FLOAT answer layer (projection, softmax, arg-max,
// test-phase bookkeeping) -- qmann_answer_f32, qmann_answer_f32_serial, qmann_answer_topk_f32.  The kernels are answer_fused.h's
// (bf16 matrix cores) and answer_serial.h's (the reference's order of additions); the int8 layer is batch_answer_i8.hip.
#include "answer_fused.h"
#include "answer_serial.h"

namespace {

struct AnsF32Call { const qmann_net *net; const float *w_ans, *u; AnsOut out; uint32_t n_query; hipStream_t st; };

// bAbI shapes (D <= 64, V <= 256), the e^x and 2^x bases: the fused form on the bf16 matrix cores (k_answer_mfma), within
// 1e-5 on the softmax
void answer_fused_launch(const AnsF32Call &c)
{
    const uint32_t D = c.net->dim_emb, V = c.net->dim_input, tiles = (V + 15u) / 16u;
    const uint32_t n_task = (c.n_query + 15u) / 16u, need = (n_task + kAmWaves - 1) / kAmWaves;
    // the smallest listed tile count that holds the dictionary
    const uint32_t tt = tiles <= 5 ? (tiles <= 2 ? 2u : tiles) : tiles <= 8 ? 8u : tiles <= 12 ? 12u : tiles <= 15 ? 15u : 16u;
    qm_dispatch<2, 3, 4, 5, 8, 12, 15, 16>(tt, [&](auto t) {
        constexpr int TT = decltype(t)::value;
        qm_launch_persistent(k_answer_mfma<TT>, need, QmPersistent{kAmWaves, 4, 256}, 3u * (size_t)TT * 16u * kAmPitch, c.st, c.w_ans, c.u,
                             c.out.answer, c.out.pred, c.out.probs, c.out.cost, c.out.match, D, V, c.net->softmax_base, c.n_query);
    });
}

// The serial-order kernel of the shape, plain or ranked (TOPK: tk holds qmann_answer_topk_f32's outputs, c.out is unused).
// lanes per query / logits per lane / queries per lane group.  Short dictionaries: 16 lanes (one DPP row), four
// lane groups side by side in a wavefront (the reductions are most of the work there); the joint-task sizes: the whole
// wavefront on four queries at once, every weight read from LDS used four times (that kernel is bound by LDS reads)
// (two queries per lane group up to 96 logits: -6 % on this kernel at V = 80; with 8 logits per lane the second query's state spills)
template <bool TOPK> void answer_serial_launch(const AnsF32Call &c, const AnsTopK<TOPK> &tk)
{
    const uint32_t D = c.net->dim_emb, V = c.net->dim_input, base = c.net->softmax_base;
    const AnsSmallPlan sp = ans_small_plan(D, V);
    if (!sp.fits) {                                         // W^T does not fit LDS twice per CU: one workgroup per query
        qm_launch(k_answer<false, TOPK>, ans_serial_grid(c.n_query), kBlock, ans_serial_lds(D, V), c.st, c.w_ans, c.u, c.out.answer,
                  c.out.pred, c.out.probs, c.out.cost, c.out.match, D, V, base, c.n_query, 0u, 0u, tk);
        return;
    }
    auto go = [&](auto kernel) {                            // persistent: two 16-wavefront workgroups per CU
        qm_launch_persistent(kernel, qm_cdiv(c.n_query, kAnsWaves * sp.qpw), QmPersistent{kAnsWaves, 8}, sp.lds, c.st, c.w_ans, c.u,
                             c.out.answer, c.out.pred, c.out.probs, c.out.cost, c.out.match, D, V, base, c.n_query, tk);
    };
    switch (sp.lpq + sp.vpt) {                              // the five builds: (lanes per query) + (logits per lane)
    case 16 + 2: go(k_answer_small<16, 2, 2, TOPK>); break;
    case 16 + 4: go(k_answer_small<16, 4, 2, TOPK>); break;
    case 16 + 6: go(k_answer_small<16, 6, 2, TOPK>); break;
    case 16 + 8: go(k_answer_small<16, 8, 1, TOPK>); break;
    default: go(k_answer_small<64, 4, 4, TOPK>); break;    // V in 129 .. 256
    }
}

// TOPK: qmann_answer_topk_f32 -- pred is not asked for, and the fused form has no ranked build
template <bool TOPK> int answer_f32_impl(const AnsF32Call &c, bool allow_fused, const AnsTopK<TOPK> &tk)
{
    QmBatched qm_scope;
    if (!c.net || !c.w_ans || !c.u || (!c.out.pred && !TOPK)) return QMANN_EINVAL;
    const uint32_t D = c.net->dim_emb, V = c.net->dim_input;
    if (D == 0 || V == 0) return QMANN_EINVAL;
    if (ans_serial_lds(D, V) > kAnsSerialLdsLimit) return QMANN_ERANGE;
    if (c.n_query == 0) return QMANN_OK;
    if (qm_too_many_queries(c.n_query)) return QMANN_ERANGE;
    // qmann_answer_f32_serial / QMANN_ANSWER_EXACT keep the serial-order kernels
    if (allow_fused && D <= 64u && V <= 256u && c.net->softmax_base != QMANN_SOFTMAX_EXP_PLAN && !qm_tuning().answer_exact) answer_fused_launch(c);
    else answer_serial_launch<TOPK>(c, tk);
    QM_LAUNCH_CHECK();
    return qm_scope.rc();
}

}  // namespace

extern "C" {

int qmann_answer_f32(const qmann_net *net, const float *w_ans, const float *u, const uint32_t *answer,
                     uint32_t *pred, float *probs, float *cost, uint32_t *match, uint32_t n_query, void *stream)
{
    return answer_f32_impl({net, w_ans, u, {answer, pred, probs, cost, match}, n_query, (hipStream_t)stream}, true, AnsTopK<false>{});
}

int qmann_answer_f32_serial(const qmann_net *net, const float *w_ans, const float *u, const uint32_t *answer,
                            uint32_t *pred, float *probs, float *cost, uint32_t *match, uint32_t n_query, void *stream)
{
    return answer_f32_impl({net, w_ans, u, {answer, pred, probs, cost, match}, n_query, (hipStream_t)stream}, false, AnsTopK<false>{});
}

int qmann_answer_topk_f32(const qmann_net *net, const float *w_ans, const float *u, uint32_t k, uint32_t *top_idx, float *top_p,
                          uint32_t n_query, void *stream)
{
    if (!net || !w_ans || !u || !top_idx || !top_p) return QMANN_EINVAL;
    if (k == 0 || k > QMANN_MAX_TOPK || k > net->dim_input) return QMANN_EINVAL;
    return answer_f32_impl({net, w_ans, u, AnsOut{}, n_query, (hipStream_t)stream}, false, AnsTopK<true>{top_idx, top_p, k});
}

}  // extern "C"
