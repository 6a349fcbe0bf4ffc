/*
 * qmann_model.h -- the test-phase forward of a whole model as ONE host call per batch.
 *
 * What MemN2N/MemN2N.c does per query in its test loop (:2378-2699: pointer wiring :2410-2548,
 * 31 layer calls :2626-2697, bookkeeping :2701-2702) this does per batch: story embedding ->
 * question embedding -> every hop -> answer layer -> prediction / match / cost, through the batched
 * kernels of qmann_batch.h.  The object owns the device copies of the parameters in the layouts the
 * kernels want (int8 gather tables, sign-magnitude lin_map codes; packed bit planes are made per
 * batch, and only where one plane serves several hops -- tied matrices, long memories, num_bit < 8 --
 * since packing re-reads the key bytes: otherwise the Hamming scores come from the int8 keys
 * themselves) and a workspace for the int8 memories that grows on demand.  Every attention mode of
 * qmann_batch.h, the Hamming ones also under EN_MQ's per-hop weight formats.  Host language is C++ inside
 * the library; the interface is plain C.
 *
 * Inputs are DEVICE pointers (the reference's cuda_data_in pools, or word-index arrays); every call
 * takes a stream and returns without synchronising.  One object per host thread / stream.
 *
 * Batches of >= 32 768 queries use a SECOND stream of the library's own beside the caller's (one per device and
 * caller stream, created on first use): the question embedding and the split of a mixed batch by story length run
 * there while the stories are embedded, and the long stories' hop kernel runs there beside the short stories'.
 * Every such branch is forked from and joined back into the caller's stream by events inside the call, so the
 * caller still sees ONE ordered step on its stream, and a stream capture of a forward records both branches
 * (tests/test_gpu_graph.py).  QMANN_NO_CORUN keeps everything on the caller's stream.
 */
#ifndef QMANN_MODEL_H
#define QMANN_MODEL_H

#include "qmann_batch.h"
#include "qmann_weights.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct qmann_model qmann_model;

/* net: dimensions, attention mode, softmax variant and every Q-format (lin_map pointers are ignored:
 * the object builds its own); w: HOST float matrices as the layer structs hold them (e.g. straight
 * from qmann_weights_load, or the reference's emb_q.w_mat[0] ... after training).  The weights are
 * uploaded and converted on `stream`; the host arrays may be freed when the call returns.
 * Layer-wise weight tying (what the reference trains: TYPE_WEIGHT_TYING 2, MemN2N/define.h:287, MemN2N.c:1770-1773) is
 * detected here: when every hop's embedding matrices equal hop 0's and the hops share their formats (EN_MQ off), the
 * memories are embedded once and all hops read the one plane -- same results, a third of the embedding work. */
int qmann_model_create(qmann_model **out, const qmann_net *net, const qmann_weights *w, void *stream);
void qmann_model_destroy(qmann_model *m);

/* The same on a named GPU (hipSetDevice index; -1 = the calling thread's current device, which is what
 * qmann_model_create uses).  A model is BOUND to its device: parameters and workspace live there, and every later call on
 * the object runs there whatever the calling thread's current device is (it is switched for the length of the call and put
 * back) -- `stream` and the data pointers of those calls must belong to that device.  One object per host thread / stream;
 * different objects (on the same or on different GPUs) may be driven from different threads concurrently: this is how a
 * host shards the reference's serial test loop (MemN2N/MemN2N.c:2378) over the GPUs of a node, one thread per GPU
 * (examples/forward_sharded.c, qmann_dist.h). */
int qmann_model_create_on(qmann_model **out, int device, const qmann_net *net, const qmann_weights *w, void *stream);
int qmann_model_device(const qmann_model *m);

/* The model's QUANTISED parameters as one position-independent blob in device memory (owned by the model, valid until it is
 * destroyed): a header with the qmann_net (dimensions, modes, every Q-format, scale factors), the int8 embedding tables
 * [V][Dp] of emb_q / emb_m[h] / emb_c[h], the sign-magnitude linear-map codes [D][Dp] and the float answer matrix [V][D]
 * (ds_ans is a float layer, MemN2N.c:902-906).  About (1 + 2 H) V Dp + H D Dp + 4 V D bytes: 40 KB for bAbI task 1, 0.5 MB
 * for D = V = 256.  This is what a multi-GPU host broadcasts once (qmann_comm_broadcast_params). */
int qmann_model_params(const qmann_model *m, const void **blob, size_t *bytes);

/* A replica from such a blob -- `blob` may be device memory of this or of a peer GPU, or host memory (a file read back);
 * it is copied, the caller keeps ownership.  No float matrix and no quantisation step is involved: the replica computes
 * from the very bytes the source model computes from, so its results are identical.  (The float embedding kernels that
 * qmann_model_forward_bow uses for irregular rows get the tables' grid values, qmann_dequantize_table_f32.)
 * Returns QMANN_EINVAL for a blob that is not one (magic, version, size or section offsets do not match). */
int qmann_model_create_from_params(qmann_model **out, int device, const void *blob, size_t bytes, void *stream);

/* Is this HOST buffer a parameter blob qmann_model_create_from_params would accept?  Pure host code, no GPU needed (a
 * receiver can vet bytes that came over a wire or out of a file before any device is touched): magic and version, the size
 * field against `bytes`, the net's dimensions (check of qmann_model_create), every Q-format (iwl + frac <= 7, the int8 word),
 * enumerated fields in range, null lin_map pointers, and the section offsets against the canonical layout of those
 * dimensions.  QMANN_OK, or QMANN_EINVAL / QMANN_EUNSUPPORTED exactly as create_from_params would answer.  When `net` is
 * not NULL it receives the header's net (dimensions and formats of the model the blob holds). */
int qmann_params_validate(const void *host_blob, size_t bytes, qmann_net *net);

/* The net as the model uses it -- lin_map[h] filled with the device pointers into the blob -- and the answer matrix: for
 * hosts that drive qmann_hops_i8 / qmann_answer_f32 themselves on memories of their own but take the parameters from a
 * (broadcast) model.  Pointers are valid until the model is destroyed. */
int qmann_model_net(const qmann_model *m, qmann_net *net, const float **w_ans);

/* Forward from word indices (qmann_embed_story_idx's wire format).
 *   story_words [rows_total][max_words] uint16, question_words [n_query][max_q_words] uint16,
 *   row_off [n_query + 1], max_slots >= every story's slot count,
 *   answer [n_query] uint32 or NULL; pred [n_query] uint32;
 *   cost / match: single device words that are ACCUMULATED into (cross_entropy_run mode 3), or NULL. */
int qmann_model_forward_words(qmann_model *m, const uint16_t *story_words, uint32_t rows_total, uint32_t max_words,
                              const uint16_t *question_words, uint32_t max_q_words, const uint32_t *row_off,
                              uint32_t max_slots, uint32_t n_query, const uint32_t *answer, uint32_t *pred,
                              float *cost, uint32_t *match, void *stream);

/* qmann_model_forward_words that also returns the attended slots of every question and hop: top_slot uint32 / top_p float
 * [n_query][n_hop][k], device memory, the rows qmann_hops_top_i8 (qmann_batch.h) defines -- the k rows of the question's own
 * story each hop weighted most, counted from the story's first row, larger probability first, equal probabilities: lower row
 * first; past the story's length (cut to max_slots) slot 0xFFFFFFFF and p 0.  It embeds exactly as qmann_model_forward_words
 * does (the question embedding beside the story embedding for large batches), runs the hops through qmann_hops_top_i8 on the
 * model's int8 keys (one plane when the model is tied; the packed-plane route is never taken) and the same answer layer:
 * pred, cost, match, qmann_model_last_u and what qmann_model_last_topk ranks are those of qmann_model_forward_words.  It
 * allocates nothing once the workspace has its size, so it can be captured in a graph and replayed.
 * What qmann_model_forward_words refuses or answers without work is answered FIRST and as there (null model: QMANN_EINVAL;
 * n_query = 0: QMANN_OK whatever k; null question_words, row_off or pred: QMANN_EINVAL); then QMANN_EUNSUPPORTED for a float
 * model, and for max_slots > 64 on a model that is not fixed-point; then QMANN_EINVAL for k = 0, k > QMANN_MAX_TOP_SLOTS, a
 * null top_slot or top_p.  Such a call launches nothing and leaves every output as it was. */
int qmann_model_forward_words_top(qmann_model *m, const uint16_t *story_words, uint32_t rows_total, uint32_t max_words,
                                  const uint16_t *question_words, uint32_t max_q_words, const uint32_t *row_off,
                                  uint32_t max_slots, uint32_t n_query, const uint32_t *answer, uint32_t *pred,
                                  float *cost, uint32_t *match, uint32_t k, uint32_t *top_slot, float *top_p, void *stream);

/* qmann_model_forward_words_top for a QMANN_ATT_FLOAT model: the same arguments and outputs, the rows those of
 * qmann_hops_top_float_i8 (qmann_batch.h), at every story length qmann_model_forward_words takes for such a model.  pred, cost,
 * match, qmann_model_last_u and what qmann_model_last_topk ranks are those of qmann_model_forward_words; it can be captured in a
 * graph as that call can.  What qmann_model_forward_words refuses or answers without work is answered FIRST and as there; then
 * QMANN_EUNSUPPORTED for a model that is not QMANN_ATT_FLOAT; then QMANN_EINVAL for k = 0, k > QMANN_MAX_TOP_SLOTS, a null
 * top_slot or top_p.  Such a call launches nothing and leaves every output as it was. */
int qmann_model_forward_words_top_float(qmann_model *m, const uint16_t *story_words, uint32_t rows_total, uint32_t max_words,
                                        const uint16_t *question_words, uint32_t max_q_words, const uint32_t *row_off,
                                        uint32_t max_slots, uint32_t n_query, const uint32_t *answer, uint32_t *pred,
                                        float *cost, uint32_t *match, uint32_t k, uint32_t *top_slot, float *top_p, void *stream);

/* One story, many questions: story_words [n_rows][max_words] is embedded ONCE (every hop, or one plane when the hops are tied)
 * and all n_query questions attend to it.  Same results as qmann_model_forward_words on n_query copies of the story.
 * The workspace holds n_rows rows of memory, not n_query x n_rows.  Attention mode QMANN_ATT_FIXED only (what
 * qmann_hops_shared_i8 covers): any other model returns QMANN_EUNSUPPORTED; n_rows = 0 returns QMANN_EINVAL.  answer, pred,
 * cost, match as above; qmann_model_last_u holds the final state afterwards.  All work goes to `stream` itself. */
int qmann_model_forward_shared_words(qmann_model *m, const uint16_t *story_words, uint32_t n_rows, uint32_t max_words,
                                     const uint16_t *question_words, uint32_t max_q_words, uint32_t n_query,
                                     const uint32_t *answer, uint32_t *pred, float *cost, uint32_t *match, void *stream);

/* Memorise once, ask many times: a knowledge base is embedded (and, for Hamming V0 / V1 models, packed into bit planes) ONCE
 * and kept by the model; every later ask embeds only its questions and attends to the kept memory.
 *
 * qmann_model_memorize_words: story_words [n_rows][max_words] as above.  Embeds every hop's memory (one plane when the hops are
 * tied) into buffers the model owns BESIDE its per-batch workspace -- qmann_model_forward_words / _bow / _shared_words calls in
 * between do not disturb them -- and replaces an earlier memory.  Attention modes QMANN_ATT_FIXED (asks run qmann_hops_shared_i8)
 * and QMANN_ATT_HAMMING_V0 / _V1 (packed planes, qmann_hops_shared_packed); QMANN_ATT_FLOAT (unless
 * qmann_model_enable_float_asks below has turned its asks on) and _APPX return QMANN_EUNSUPPORTED, and so does a Hamming model the packed call would refuse (num_bit outside {1, 2, 4, 8}; 64 padded columns
 * with one bit).  n_rows = 0: QMANN_EINVAL.  A memory too long for LDS with one query per workgroup: QMANN_ERANGE, here, so that
 * an ask cannot fail late.  A call that fails leaves the model with nothing memorised.
 *
 * qmann_model_ask_words: question_words [n_query][max_q_words]; answer, pred, cost, match as in qmann_model_forward_words;
 * same results as qmann_model_forward_words on n_query copies of the memorised story; qmann_model_last_u holds the final state
 * afterwards.  Nothing memorised: QMANN_EINVAL.  It allocates nothing once the question workspace has its size (one earlier ask
 * of at least n_query questions), so it can be captured in a graph and replayed.
 *
 * All work of both calls goes to the caller's `stream` itself.  ORDERING IS THE CALLER'S: an ask on another stream than the
 * memorize before it must be ordered behind it by the caller (an event, a synchronisation), and a memorize must not be issued
 * while asks on the earlier memory are still running on other streams -- it frees or overwrites what they read.
 * qmann_model_memory_rows: rows of the kept memory, 0 = nothing memorised. */
int qmann_model_memorize_words(qmann_model *m, const uint16_t *story_words, uint32_t n_rows, uint32_t max_words, void *stream);
int qmann_model_ask_words(qmann_model *m, const uint16_t *question_words, uint32_t max_q_words, uint32_t n_query,
                          const uint32_t *answer, uint32_t *pred, float *cost, uint32_t *match, void *stream);
uint32_t qmann_model_memory_rows(const qmann_model *m);

/* qmann_model_ask_words that also returns the attended slots of every question and hop: top_slot uint32 / top_p float
 * [n_query][n_hop][k], device memory, the rows qmann_hops_shared_top_i8 (qmann_batch.h) defines -- the k rows of the memorised
 * story each hop weighted most, larger probability first, equal probabilities: lower row first; past the memory's length slot
 * 0xFFFFFFFF and p 0.  It takes the path qmann_model_ask_words takes: the unsplit call, or with split asks enabled the split
 * call in chunks of floor(budget / share) questions, each chunk writing its own block of rows.  pred, cost, match,
 * qmann_model_last_u and what qmann_model_last_topk ranks are those of qmann_model_ask_words; it allocates nothing once the
 * question workspace has its size, so it can be captured in a graph and replayed.
 * QMANN_ATT_FIXED models only: a Hamming V0 / V1 model returns QMANN_EUNSUPPORTED here and is served by
 * qmann_model_ask_words_top_packed below (its softmax is per slot (V1) or over up to 2 049 bins (V0), a different selection).
 * What qmann_model_ask_words refuses or answers without work is answered FIRST and as there (nothing memorised: QMANN_EINVAL;
 * n_query = 0: QMANN_OK whatever k; null question_words or pred: QMANN_EINVAL); then QMANN_EUNSUPPORTED for a Hamming model
 * and for a QMANN_ATT_FLOAT model (qmann_model_ask_words_top_float below serves those), ahead of any launch; then QMANN_EINVAL for k = 0,
 * k > QMANN_MAX_TOP_SLOTS, a null top_slot or top_p.  A refused call launches nothing and leaves every output as it was. */
int qmann_model_ask_words_top(qmann_model *m, const uint16_t *question_words, uint32_t max_q_words, uint32_t n_query,
                              const uint32_t *answer, uint32_t *pred, float *cost, uint32_t *match,
                              uint32_t k, uint32_t *top_slot, float *top_p, void *stream);

/* qmann_model_ask_words_top for a Hamming V0 / V1 model: the same arguments and outputs, the rows those of
 * qmann_hops_shared_top_packed (qmann_batch.h) on the packed memory the model holds.  It takes the path qmann_model_ask_words
 * takes for such a model: the unsplit packed call, or with qmann_model_enable_split_asks_packed on and a memory beyond LDS the
 * split call in chunks of floor(budget / share) questions, each chunk writing its block of rows at q0 . n_hop . k.  pred, cost,
 * match, qmann_model_last_u and what qmann_model_last_topk ranks are those of qmann_model_ask_words; nothing is allocated once
 * the question workspace has its size, so the call can be captured in a graph and replayed.
 * What qmann_model_ask_words refuses or answers without work is answered FIRST and as there; then QMANN_EUNSUPPORTED for a
 * QMANN_ATT_FIXED model (qmann_model_ask_words_top serves those) and for a QMANN_ATT_FLOAT model; then QMANN_EINVAL for k = 0,
 * k > QMANN_MAX_TOP_SLOTS, a null top_slot or top_p.  A refused call launches nothing and leaves every output as it was. */
int qmann_model_ask_words_top_packed(qmann_model *m, const uint16_t *question_words, uint32_t max_q_words, uint32_t n_query,
                                     const uint32_t *answer, uint32_t *pred, float *cost, uint32_t *match,
                                     uint32_t k, uint32_t *top_slot, float *top_p, void *stream);

/* Opt-in: asks through qmann_hops_shared_split_i8 (qmann_batch.h).  Without this call every call above behaves as described.
 * The model allocates `scratch_bytes` of workspace HERE (freed by qmann_model_destroy; never regrown inside an ask, so asks
 * still allocate nothing and stay capturable).  From then on qmann_model_memorize_words accepts QMANN_ATT_FIXED memories beyond
 * the LDS cap, up to 2^24 rows, and returns QMANN_ERANGE where ONE query's share of workspace
 * (qmann_hops_shared_split_ws_bytes(net, n_rows, 1)) exceeds the budget; qmann_model_ask_words takes the split call where the
 * memory does not fit LDS (and, once measured, for small batches), in chunks of floor(budget / share) questions one after the
 * other on the caller's stream.  Results are those of the unsplit ask, bit for bit.
 * scratch_bytes = 0 turns the mode off and frees the workspace; a memorised memory that can no longer be asked (too long for
 * LDS, or its share above a new budget) is forgotten.  A model whose attention mode is not QMANN_ATT_FIXED: QMANN_EUNSUPPORTED.
 * The call waits for `stream` before it frees an earlier workspace; asks running on OTHER streams are the caller's to order. */
int qmann_model_enable_split_asks(qmann_model *m, size_t scratch_bytes, void *stream);

/* The same opt-in for QMANN_ATT_HAMMING_V0 / _V1 models (the ones qmann_model_memorize_words accepts): asks through
 * qmann_hops_shared_split_packed.  The contract is that of qmann_model_enable_split_asks with that call's helper: memories beyond
 * the LDS cap of qmann_hops_shared_packed, up to 2^24 rows, are embedded and packed; QMANN_ERANGE at memorize where ONE query's
 * share (qmann_hops_shared_split_packed_ws_bytes(net, n_rows, 1)) exceeds the budget; asks of such a memory go in chunks of
 * floor(budget / share) questions; a memory that fits LDS is asked as before, bit for bit.  scratch_bytes = 0 turns the mode off
 * and forgets a memory that can no longer be asked.  Any other model: QMANN_EUNSUPPORTED. */
int qmann_model_enable_split_asks_packed(qmann_model *m, size_t scratch_bytes, void *stream);

/* Opt-in for QMANN_ATT_FLOAT models (the reference's ATTENTION_MODE 1): memorise once, ask many through
 * qmann_hops_shared_float_i8 (qmann_batch.h).  Without this call such a model is refused by qmann_model_memorize_words as
 * described above.  With on != 0, qmann_model_memorize_words embeds a float model's memory on the weight grid, as
 * qmann_model_forward_words does for such a model (one plane when the hops are tied), and checks its length against
 * qmann_hops_shared_float_lds_bytes(n_rows, 1): beyond 160 KiB - 1 KiB (38 368 rows) it returns QMANN_ERANGE -- at memorize,
 * never at ask.  qmann_model_ask_words then gives the same pred, cost, match and qmann_model_last_u as
 * qmann_model_forward_words on n_query copies of the story, bit for bit (cost: up to the order of its float atomics), allocates
 * nothing once the question workspace has its size, and can be captured in a graph; qmann_model_last_topk works after it.
 * qmann_model_ask_words_top / _top_packed keep returning QMANN_EUNSUPPORTED for such a model, before anything is launched
 * (qmann_model_ask_words_top_float below returns its attended slots), and so do qmann_model_forward_shared_words and both qmann_model_enable_split_asks calls.
 * on = 0 forgets a memorised memory and restores the behaviour above exactly.  The call allocates nothing.
 * Any model whose attention mode is not QMANN_ATT_FLOAT: QMANN_EUNSUPPORTED. */
int qmann_model_enable_float_asks(qmann_model *m, int on);

/* qmann_model_ask_words_top for a QMANN_ATT_FLOAT model with float asks enabled: the same arguments and outputs, the rows those
 * of qmann_hops_shared_top_float_i8 (qmann_batch.h) on the memory the model holds.  pred, cost, match, qmann_model_last_u and
 * what qmann_model_last_topk ranks are those of qmann_model_ask_words; nothing is allocated once the question workspace has its
 * size, so the call can be captured in a graph and replayed.
 * What qmann_model_ask_words refuses or answers without work is answered FIRST and as there (nothing memorised -- which is all a
 * float model without qmann_model_enable_float_asks can have --: QMANN_EINVAL; n_query = 0: QMANN_OK whatever k; null
 * question_words or pred: QMANN_EINVAL); then QMANN_EUNSUPPORTED for a model that is not QMANN_ATT_FLOAT; then QMANN_EINVAL for
 * k = 0, k > QMANN_MAX_TOP_SLOTS, a null top_slot or top_p.  A refused call launches nothing and leaves every output as it was. */
int qmann_model_ask_words_top_float(qmann_model *m, const uint16_t *question_words, uint32_t max_q_words, uint32_t n_query,
                                    const uint32_t *answer, uint32_t *pred, float *cost, uint32_t *match,
                                    uint32_t k, uint32_t *top_slot, float *top_p, void *stream);

/* Forward from the reference's float bag-of-words pools (dev_m_test / dev_q_test, MemN2N.c:2337-2349):
 *   story [rows_total][dim_input] float, question [n_query][dim_input] float. */
int qmann_model_forward_bow(qmann_model *m, const float *story, uint32_t rows_total, const float *question,
                            const uint32_t *row_off, uint32_t max_slots, uint32_t n_query, const uint32_t *answer,
                            uint32_t *pred, float *cost, uint32_t *match, void *stream);

/* device pointer to the last batch's final hop state u [n_query][D] (valid until the next call) */
const float *qmann_model_last_u(const qmann_model *m);

/* Ranked answers of the model's most recent batch: qmann_answer_topk_f32 (qmann_batch.h) on qmann_model_last_u with the model's
 * own answer matrix -- top_idx / top_p [n_query][k] of the n_query that the last qmann_model_forward_words / _forward_shared_words
 * / _ask_words / _forward_bow enqueued an answer layer for (a call of those that fails leaves no batch to rank).  One call for
 * all four forwards.  The ranking is that of the SERIAL-ORDER layer: its first entry equals the forward's own pred wherever the
 * two best probabilities differ by more than 1e-6 (the forward may have taken the fused bf16 form), and always under
 * QMANN_ANSWER_EXACT.  Ordering is as for qmann_model_last_u: `stream` is the forward's stream, or the caller orders this call
 * behind the forward; the next forward overwrites what it reads.  It allocates nothing.
 * QMANN_EINVAL before any batch has run, and for what qmann_answer_topk_f32 refuses (k = 0, k > QMANN_MAX_TOPK, k > dim_input,
 * null outputs). */
int qmann_model_last_topk(qmann_model *m, uint32_t k, uint32_t *top_idx, float *top_p, void *stream);
/* rows qmann_model_last_topk will write (the n_query of that last batch); 0 = no batch to rank */
uint32_t qmann_model_last_n_query(const qmann_model *m);

#ifdef __cplusplus
}
#endif
#endif /* QMANN_MODEL_H */
