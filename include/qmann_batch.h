/*
 * qmann_batch.h -- batched, int8-native entry points of libqmann_hip.so.
 *
 * These have no counterpart in the reference (which runs one query at a time
 * through ~31 kernel launches, MemN2N/MemN2N.c:2378-2697); they are the
 * throughput face of the same arithmetic: many independent queries per launch,
 * memories stored as true int8 codes of the reference's Q(iwl.frac) grid
 * values (lossless for word length 8), the multi-hop loop fused
 * into one kernel.  Plain C ABI: device pointers, sizes, an opaque stream
 * handle (hipStream_t passed as void*; NULL = the null stream).  Every call is
 * asynchronous and, to its caller, ONE ordered step on that stream; a hop launch
 * over >= 32 768 stories of mixed length puts one of its two kernels on a second
 * stream of the library's own, forked from and joined back into the caller's
 * stream by events inside the call (qmann_model.h; QMANN_NO_CORUN turns it off).
 *
 * Return value of every function: 0 on success, a negative QMANN_E* code on a
 * caller error (nothing is launched) or QMANN_EHIP when the HIP runtime fails
 * (message on stderr; unlike the drop-in cuda_* verbs, which exit() as the
 * reference does, these calls return).
 *
 * Data layout ("memory" = the per-query story slots):
 *   keys, vals : int8 [n_hop][rows_total][Dp]    SIGN-MAGNITUDE codes: bit 7 = sign, bits 6..0 =
 *                |code| -- the top byte of the reference's own FLOAT2FIXED word
 *                (lib/common.h:210), so "minus zero" (0x80) is representable as it is there.
 *                Dp = dim_emb_pad (multiple of 16, >= D); columns D..Dp-1 are 0.
 *                keys[h] carry Q(att[h]) codes, vals[h] carry Q(act[h]) codes (valid codes of those
 *                formats: |code| <= 2^(iwl+frac) - 1, which matters for word lengths below 8) --
 *                i.e. what the reference's dot_mat_vec layers see after their
 *                own operand quantisation (lib/layer_cuda.cu:120, :562).
 *   row_off    : uint32 [n_query + 1]            first row of each query's
 *                slots; query q owns rows row_off[q] .. row_off[q+1]-1 in every
 *                hop plane (ragged, like the reference's pools
 *                MemN2N/MemN2N.c:2294-2333).
 *   u vectors  : float [n_query][D]              values on the producer's grid,
 *                exactly the floats the reference passes between layers.
 */
#ifndef QMANN_BATCH_H
#define QMANN_BATCH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QMANN_MAX_HOP 8

enum { QMANN_OK = 0, QMANN_EINVAL = -1, QMANN_ERANGE = -2, QMANN_EUNSUPPORTED = -3, QMANN_EIO = -4,
       QMANN_EHIP = -5 /* a HIP runtime call failed (message on stderr); the process goes on */,
       QMANN_ECOMM = -6 /* RCCL: the library could not be loaded or a collective call failed (qmann_dist.h) */ };

/* attention_mode: MemN2N/define.h:10-15 (1..3) plus the packed-code Hamming forms */
enum {
    QMANN_ATT_FLOAT = 1,      /* float dot product over the grid values, float read-out           */
    QMANN_ATT_FIXED = 2,      /* per-product quantised dot product, quantised read-out            */
    QMANN_ATT_APPX = 3,       /* CUDA "approximate" Hamming attention (lib/layer_cuda.cu:355-541) */
    QMANN_ATT_HAMMING_V0 = 10,/* bit-agreement count over the top n bits (lib/common.c:223-246)   */
    QMANN_ATT_HAMMING_V1 = 11 /* signed, weighted bit agreement (lib/common.c:249-312)            */
};
/* BINARY_MODE (define.h:87-88: the query binarised to +-1 in the scores and the linear map) is not a mode
 * of its own: set qmann_net.bin = {0, 0}, exactly what the reference does (MemN2N.c:769-775). */

/* byte layout of an int8 code */
enum { QMANN_CODE_TWOS = 0 /* two's complement (weights) */, QMANN_CODE_SIGNMAG = 1 /* memories */ };

enum { QMANN_SOFTMAX_EXP = 0 /* lib/layer_cuda.cu:2006 */, QMANN_SOFTMAX_POW2 = 1 /* lib/layer.c:1225 */,
       QMANN_SOFTMAX_EXP_PLAN = 2 /* piece-wise linear exp, lib/layer.c:1196-1199 + lib/common.c:51-73 */ };

typedef struct qmann_fmt {
    uint32_t iwl;
    uint32_t frac;
} qmann_fmt;

typedef struct qmann_net {
    uint32_t n_hop;
    uint32_t dim_emb;        /* D */
    uint32_t dim_emb_pad;    /* Dp: 64, 128 or 256 */
    uint32_t dim_input;      /* V: dictionary + time slots */
    uint32_t attention_mode;
    uint32_t softmax_base;
    uint32_t en_lin_map;     /* MemN2N/define.h:291 */
    uint32_t num_bit;        /* Hamming forms: bits compared (<= 8) */
    qmann_fmt act[QMANN_MAX_HOP];   /* (iwl[h], frac[h])          MemN2N/MemN2N.c:715-716 */
    qmann_fmt w[QMANN_MAX_HOP];     /* (iwl_w[h], frac_w[h])      :718-719, 748-754       */
    qmann_fmt att[QMANN_MAX_HOP];   /* (iwl_att[h], frac_att[h])  :721-722                */
    qmann_fmt bin;                  /* (iwl_bin, frac_bin)        :769-775; {0,0} binarises u   */
    const int8_t *lin_map[QMANN_MAX_HOP]; /* device, [D][Dp] sign-magnitude codes (QMANN_CODE_SIGNMAG) in format w[h]; NULL when !en_lin_map */
    /* in-hop softmax variants; all zero = the stock configuration */
    uint32_t softmax_shift_based;   /* EN_SHIFT_BASED_SM (define.h:54-55): power-of-two style normaliser, sf_in only (MemN2N.c:856) */
    uint32_t en_att_scale;          /* EN_SC_ATT (define.h:58-59): scores times one learnt scalar before the softmax (MemN2N.c:2647-2649) */
    float att_scale[QMANN_MAX_HOP]; /* that scalar per hop (scale.w, lib/layer.h:786-810) */
    uint32_t en_non_linearity;      /* EN_NON_LINEARITY (define.h): RELU layers non_lin[h] (MemN2N.c:894-896, 2668-2671): the attention of
                                     * hop h >= 1 and the answer layer read RELU(sv), lin_map keeps reading sv (:2435-2437, 2471-2473, 2535-2537);
                                     * u_out is then RELU(sv[n_hop-1]) */
    uint32_t en_pe;                 /* EN_PE (define.h:298): position encoding.  In the reference it changes the QUESTION's bag-of-words
                                     * row only (the story lines are commented out, sample.c:529-541): entry of word w at slot j is SET to
                                     * pe_w[w][j] = 1 + 4 (w / dim_input - 0.5)(j / dim_word - 0.5) (MemN2N.c:606-616, sample.c:559-560).
                                     * qmann_embed_query_idx applies it to word-index questions; bag-of-words callers pass such rows themselves */
    uint32_t pe_dim_word;           /* dim_word of that formula: longest sentence + 1 with the time entry (MemN2N.c:575-580) */
} qmann_net;

/* optional per-query taps for parity tests; any pointer may be NULL */
typedef struct qmann_taps {
    int32_t *score_codes;   /* [n_hop][rows_total]  integer score in units of 2^-frac_att (fixed) or 2^-10 (appx) */
    float   *scores;        /* [n_hop][rows_total]  the same as float, as the reference's dev_out_vec */
    float   *probs;         /* [n_hop][rows_total] */
    float   *o;             /* [n_query][n_hop][D] */
    float   *u;             /* [n_query][n_hop][D] */
} qmann_taps;

/* float -> int8 code of Q(iwl.frac)(x) in the given byte layout; rows of `cols` values are written
 * with pitch `pitch` (>= cols, padding zeroed).  Rejects formats with iwl + frac > 7. */
int qmann_quantize_i8(const float *src, int8_t *dst, size_t rows, uint32_t cols, uint32_t pitch,
                      qmann_fmt fmt, int layout, void *stream);

/* The hot path: all hops of all queries in one launch (one workgroup per query).
 *   max_slots                  -- bound on row_off[q+1] - row_off[q]; sizes the per-query LDS.  A story longer than the bound
 *                                 is CUT to max_slots by every kernel: the call still returns 0 and
 *                                 the result is that of the shortened story -- pass the true maximum (qmann_check_slots below
 *                                 verifies a bound on the device)
 *   u0    [n_query][D] float   -- question embedding (emb_q output)
 *   u_out [n_query][D] float   -- sv[n_hop-1] output, input of the answer layer
 * Replaces, per query and hop, the reference sequence dot_mat_vec_fwd -> softmax_fwd ->
 * dot_mat_vec_fwd(trans) -> dense_fwd(lin_map) -> sum_vec_fwd (MemN2N/MemN2N.c:2644-2666).
 * attention_mode QMANN_ATT_FIXED (define.h mode 2), QMANN_ATT_APPX (mode 3; needs att formats with
 * iwl + frac = 7; the key bytes are the ones the embedding entry points store -- sign of the value | magnitude
 * on the attention grid, or the key's own code where w[h] is one bit finer than att[h], exactly -2^iwl_att as
 * 0x80 -- and carry the reference's 32-bit operand words for these grids: u and the keys inside the attention
 * grid; both at least one fractional bit coarser (wider range: they saturate); u inside and the keys one bit
 * finer.  EN_MQ's formats, MemN2N/MemN2N.c:748-754, are the second, first and third case at hops 0, 1, 2.
 * Any other combination: QMANN_EUNSUPPORTED) or
 * QMANN_ATT_FLOAT (mode 1: float scores / softmax / read-out over the same int8 memories, which
 * then carry Q(w[h]) codes -- the embedding outputs, not re-quantised), or QMANN_ATT_HAMMING_V0 / _V1
 * computed straight from the int8 keys (the top num_bit bits of a sign-magnitude byte are its bit planes):
 * same scores as qmann_hops_packed without a packing pass -- the choice for short memories and for
 * num_bit = 8, where planes are no smaller than bytes.
 * hop_stride may be 0: every hop then reads the same key / value plane -- layer-wise weight tying with equal
 * formats on every hop (TYPE_WEIGHT_TYING 2, MemN2N/define.h:287; MemN2N.c:1770-1773 copies hop 0's embedding
 * matrices over the others), where the per-hop memories are the same bytes.  `taps` need distinct planes. */
int qmann_hops_i8(const qmann_net *net, const int8_t *keys, const int8_t *vals, size_t hop_stride,
                  const uint32_t *row_off, uint32_t max_slots, const float *u0, float *u_out,
                  const qmann_taps *taps, uint32_t n_query, void *stream);

/* qmann_hops_i8 when every query reads the SAME memory: keys, vals int8 [n_hop][n_slots][Dp] sign-magnitude (the layout of
 * qmann_hops_i8; hop_stride bytes between hop planes, 0 = tied hops), u0 / u_out [n_query][D].  Results are those of
 * qmann_hops_i8 on n_query copies of the plane, bit for bit.
 * taps (any pointer may be NULL): score_codes / scores / probs [n_hop][n_query][n_slots], o / u [n_query][n_hop][D]; they are
 * indexed by query, not by plane row, so they are allowed with hop_stride = 0.
 * One workgroup owns a tile of 1, 2, 4 or 8 queries and scans the plane once per hop for all of them (the plane stays in L2;
 * csrc/batch_hops_shared.hip); the library chooses the tile, QMANN_SHARED_QT (environment) forces one that fits.
 * attention_mode QMANN_ATT_FIXED only -- every qmann_net field qmann_hops_i8 honours in that mode is honoured; any other
 * attention mode returns QMANN_EUNSUPPORTED with nothing launched (Hamming V0 / V1 on packed codes: qmann_hops_shared_packed
 * below; float attention: qmann_hops_shared_float_i8 below; the APPX form is a follow-up).
 * n_slots = 0: QMANN_EINVAL.  A memory too long for LDS with one query per workgroup: QMANN_ERANGE (sizing helper below).
 * One ordered step on `stream`, no second stream, no library scratch: it can be captured in a graph. */
int qmann_hops_shared_i8(const qmann_net *net, const int8_t *keys, const int8_t *vals, size_t hop_stride,
                         uint32_t n_slots, const float *u0, float *u_out, const qmann_taps *taps,
                         uint32_t n_query, void *stream);

/* qmann_hops_shared_i8 for float attention (QMANN_ATT_FLOAT, csrc/batch_hops_shared_float.hip).  Layout as qmann_hops_shared_i8:
 * keys, vals int8 [n_hop][n_slots][Dp] sign-magnitude carrying Q(w[h]) codes, as qmann_hops_i8 documents for mode 1; hop_stride
 * bytes between hop planes, 0 = tied hops; u0 / u_out [n_query][D].  taps (any pointer may be NULL): score_codes / scores / probs
 * [n_hop][n_query][n_slots], o / u [n_query][n_hop][D], allowed with hop_stride = 0.
 * u_out and EVERY tap are bit-equal to qmann_hops_i8 with attention_mode = QMANN_ATT_FLOAT on n_query copies of the planes
 * (row_off[q] = q . n_slots, max_slots = n_slots): one workgroup owns a tile of 1, 2, 4 or 8 queries, scans the key plane and
 * reads the value plane once per hop for all of them, and keeps every query's float additions in the per-story kernel's order.
 * Every qmann_net field qmann_hops_i8 honours in this mode is honoured (the three softmax bases, the shift-based normaliser,
 * en_att_scale, en_non_linearity, binary u, en_lin_map off, per-hop formats).  The library chooses the tile, QMANN_SHARED_QT
 * forces one that fits.
 * Refusals, with nothing launched and no output touched, in this order: those of qmann_hops_shared_i8's argument and format
 * checks; QMANN_EUNSUPPORTED for any attention mode but QMANN_ATT_FLOAT (and for a dim_emb_pad outside {64, 128, 256});
 * QMANN_EINVAL for n_slots = 0; QMANN_ERANGE for a memory whose float-per-slot LDS exceeds 160 KiB - 1 KiB with one query per
 * workgroup (more than 38 368 slots; sizing helper below -- a slot-split float form for longer memories is out of scope);
 * QMANN_OK for n_query = 0; QMANN_ERANGE for 2^24 queries or more.
 * One kernel on `stream`, no second stream, no scratch, no allocation: it can be captured in a graph. */
int qmann_hops_shared_float_i8(const qmann_net *net, const int8_t *keys, const int8_t *vals, size_t hop_stride,
                               uint32_t n_slots, const float *u0, float *u_out, const qmann_taps *taps,
                               uint32_t n_query, void *stream);

/* qmann_hops_shared_i8 with the SLOTS cut into slices (csrc/batch_hops_shared_split.hip): for memories too long for LDS (up to
 * 2^24 slots) and for batches of so few questions that one workgroup per tile of queries leaves most compute units idle.
 * Arguments and taps as qmann_hops_shared_i8; QMANN_ATT_FIXED only, and every qmann_net field that call honours is honoured.
 * Results equal those of qmann_hops_shared_i8 bit for bit wherever that call runs (scores are int8 codes and the softmax is
 * computed from integer histogram counts, which add across workgroups in any order); beyond its cap they are those of
 * qmann_hops_i8 on copies of the plane, had LDS no limit.
 * Per hop two kernels on `stream` (scan: query tiles x slices; finish: one workgroup per query), behind one hipMemsetAsync of
 * the histograms: 1 + 2 n_hop ordered nodes, no library scratch, no second stream, no allocation -- it can be captured in a graph.
 * ws: the CALLER's workspace, 16-byte aligned, at least qmann_hops_shared_split_ws_bytes(net, n_slots, n_query) bytes (linear in
 * n_query: score bytes [n_query][n_slots rounded up to 16], uint32 histograms [n_hop][n_query][256], float u [n_query][256]).
 * Its contents need not survive between calls; two calls that may run at the same time need a workspace each.
 * n_slices: slices wanted, 0 = the library's choice (qmann_hops_shared_split_slices).  A slice is a multiple of 16 rows except
 * the last, so a wish larger than ceil(n_slots / 16) is clamped to that (and to what keeps tiles x slices below 2^31).
 * The query tile is the library's choice; QMANN_SHARED_QT forces one.
 * Nothing is launched and the code returned is: QMANN_EUNSUPPORTED for another attention mode or a dim_emb_pad outside
 * {64, 128, 256}; QMANN_EINVAL for null pointers, a null or misaligned ws, ws_bytes below the helper's figure, n_slots = 0;
 * QMANN_ERANGE for n_slots > 2^24, 2^24 queries or more, a word length above 8.  n_query = 0: QMANN_OK. */
size_t qmann_hops_shared_split_ws_bytes(const qmann_net *net, uint32_t n_slots, uint32_t n_query);
uint32_t qmann_hops_shared_split_slices(uint32_t n_slots, uint32_t dim_emb_pad, uint32_t n_query);
int qmann_hops_shared_split_i8(const qmann_net *net, const int8_t *keys, const int8_t *vals, size_t hop_stride,
                               uint32_t n_slots, const float *u0, float *u_out, const qmann_taps *taps, uint32_t n_query,
                               uint32_t n_slices, void *ws, size_t ws_bytes, void *stream);

/* Attended slots: qmann_hops_shared_i8 / qmann_hops_shared_split_i8 that also return, per query and hop, the k memory rows the
 * hop weighted most and their weights -- the supporting facts -- without a [n_hop][n_query][n_slots] array anywhere.
 *   top_slot [n_query][n_hop][k] uint32, top_p [n_query][n_hop][k] float, device memory; 1 <= k <= QMANN_MAX_TOP_SLOTS.
 * In terms of what qmann_hops_shared_i8 writes to taps.probs for the same arguments: row (q, h) lists the k slots of
 * probs[h][q][:] that come first in the order "larger probability first, equal probabilities: lower slot index first", and
 * top_p[q][h][j] is bit-equal to probs[h][q][top_slot[q][h][j]].  The order is over the probability VALUES: slots whose scores
 * differ tie where their probabilities are equal floats (the zero region of exp_plan, underflow to 0, att_scale = 0), and a
 * negative att_scale needs no rule of its own.  Where k > n_slots the entries past n_slots hold slot 0xFFFFFFFF and p 0.0f.
 * u_out is the base call's bit for bit, and every qmann_net field the base call honours is honoured (the three softmax bases,
 * the shift-based normaliser, en_att_scale, ReLU, binary u, tied hops with hop_stride = 0, per-hop formats).  There is no taps
 * argument: a host that wants taps calls the base functions.  (Hamming V0 / V1 on packed codes: qmann_hops_shared_top_packed /
 * qmann_hops_shared_split_top_packed below.)
 * The selection runs inside the base call's kernels behind each query's hop (csrc/hops_attended.h), from the score histogram and
 * the score bytes the hop already holds; LDS per query, tiles and caps are the base call's.  The split call takes the SAME
 * workspace and qmann_hops_shared_split_ws_bytes figure as qmann_hops_shared_split_i8.  Both are ordered steps on `stream` with
 * the node counts of their base calls (1; 1 + 2 n_hop), no allocation, no library scratch, no second stream: they can be captured
 * in a graph.
 * Nothing is launched, no output is touched and the code returned is: every refusal of the respective base call, unchanged and
 * FIRST (a call with a fault of the base call and a fault below returns the base call's code; n_query = 0 is QMANN_OK whatever
 * k); then QMANN_EINVAL for k = 0, k > QMANN_MAX_TOP_SLOTS, a null top_slot or top_p.  k > n_slots is no error. */
#define QMANN_MAX_TOP_SLOTS 16
int qmann_hops_shared_top_i8(const qmann_net *net, const int8_t *keys, const int8_t *vals, size_t hop_stride,
                             uint32_t n_slots, const float *u0, float *u_out, uint32_t k,
                             uint32_t *top_slot, float *top_p, uint32_t n_query, void *stream);
int qmann_hops_shared_split_top_i8(const qmann_net *net, const int8_t *keys, const int8_t *vals, size_t hop_stride,
                                   uint32_t n_slots, const float *u0, float *u_out, uint32_t k,
                                   uint32_t *top_slot, float *top_p, uint32_t n_query, uint32_t n_slices,
                                   void *ws, size_t ws_bytes, void *stream);

/* Attended slots per story: qmann_hops_i8 (every query its OWN memory) that also returns, per query and hop, the k rows of the
 * query's story the hop weighted most and their weights, without a [n_hop][rows_total] probability array anywhere.
 *   top_slot [n_query][n_hop][k] uint32, top_p [n_query][n_hop][k] float, device memory; 1 <= k <= QMANN_MAX_TOP_SLOTS.
 * In terms of what qmann_hops_i8 writes to taps.probs for the same arguments, with r0 = row_off[q] and S = min(row_off[q+1] - r0,
 * max_slots): row (q, h) lists the slots s in [0, S) -- counted from the story's first row -- that come first in the order
 * "larger probability first, equal probabilities: lower slot first", and top_p[q][h][j] is bit-equal to
 * probs[h][r0 + top_slot[q][h][j]].  The order is over the probability VALUES, as floats (slots whose scores differ tie where
 * their probabilities are equal; a negative att_scale needs no rule of its own); a NaN probability ranks below every number.
 * Entries past S hold slot 0xFFFFFFFF and p 0.0f: an empty story, k > S, a story cut by max_slots (no slot >= max_slots appears).
 * u_out is bit-equal to that of qmann_hops_i8 called with taps on the same arguments, and every qmann_net field the base call
 * honours is honoured.  hop_stride = 0 (tied hops) is allowed -- the outputs are indexed by query, not by plane row -- and gives
 * the result of the call on n_hop copies of the plane.  There is no taps argument.
 * Served: QMANN_ATT_FIXED at every length the base call takes (up to its LDS cap); QMANN_ATT_APPX (EN_MQ's operand grids
 * included) and QMANN_ATT_HAMMING_V0 / _V1 on int8 keys up to max_slots = 64, which covers every bAbI story.  The selection runs
 * inside the kernels a call with taps launches (csrc/hops_attended_story.h): in registers of the one-wavefront kernel up to 64
 * slots, from the score histogram and the score bytes of the streaming fixed-point kernel beyond (which never ends a scan early
 * for such a call: the selection needs every score).
 * Nothing is launched, no output is touched and the code returned is: whatever qmann_hops_i8 answers for the same arguments
 * without taps, unchanged and FIRST (its refusals; n_query = 0 is QMANN_OK whatever k); then QMANN_EUNSUPPORTED for
 * QMANN_ATT_FLOAT at any length and for QMANN_ATT_APPX / _HAMMING_V0 / _V1 with max_slots > 64; then QMANN_EINVAL for k = 0,
 * k > QMANN_MAX_TOP_SLOTS, a null top_slot or top_p.
 * One kernel on `stream`: no second stream, no library scratch, no allocation -- it can be captured in a graph. */
int qmann_hops_top_i8(const qmann_net *net, const int8_t *keys, const int8_t *vals, size_t hop_stride,
                      const uint32_t *row_off, uint32_t max_slots, const float *u0, float *u_out,
                      uint32_t k, uint32_t *top_slot, float *top_p, uint32_t n_query, void *stream);

/* Attended slots for float attention (QMANN_ATT_FLOAT, csrc/batch_hops_top_float.hip): qmann_hops_i8 (every query its own
 * memory) and qmann_hops_shared_float_i8 (one memory for all queries) that also return, per query and hop, the k memory rows the
 * hop weighted most and their weights, without a probability array anywhere -- in this mode p is not quantised, every slot
 * carries weight, and the `probs` tap is the largest array the library can be asked to write.
 *   top_slot [n_query][n_hop][k] uint32, top_p [n_query][n_hop][k] float, device memory; 1 <= k <= QMANN_MAX_TOP_SLOTS.
 * qmann_hops_top_float_i8, in terms of what qmann_hops_i8 (attention_mode = QMANN_ATT_FLOAT) writes to taps.probs for the same
 * arguments, with r0 = row_off[q] and S = min(row_off[q+1] - r0, max_slots): row (q, h) lists the slots s in [0, S) -- counted
 * from the story's first row -- that come first in the order "larger probability first, equal probabilities: lower slot first",
 * and top_p[q][h][j] is bit-equal to probs[h][r0 + top_slot[q][h][j]].  qmann_hops_shared_top_float_i8, in terms of what
 * qmann_hops_shared_float_i8 writes for the same arguments: S = n_slots, and top_p[q][h][j] is bit-equal to
 * probs[h][q][top_slot[q][h][j]], under every query tile (QMANN_SHARED_QT).
 * The order is over the probability VALUES, as floats: slots tie where their probabilities are equal floats (equal rows,
 * underflow to 0, att_scale = 0); a negative att_scale needs no rule of its own; a NaN probability -- the shift-based normaliser
 * divides by llrint(log2(total)), which is 0 for a total below sqrt 2, and 0 / 0 is then reached by every slot whose e^x
 * underflowed -- ranks below every number (+inf, the other quotient by 0, ranks above).  Entries past S hold slot 0xFFFFFFFF and
 * p 0.0f: an empty story, k > S, a story cut by max_slots (no slot >= max_slots appears).
 * u_out is bit-equal to the base call's, and every qmann_net field the base call honours is honoured (the three softmax bases,
 * the shift-based normaliser, en_att_scale, en_non_linearity, binary u, en_lin_map off, per-hop formats).  hop_stride = 0 (tied
 * hops) is allowed -- the outputs are indexed by query -- and gives the result of the call on n_hop copies of the plane.  There is
 * no taps argument: a host that wants taps calls the base functions.
 * The selection runs inside the hop kernel behind each query's softmax, over the floats the query's LDS slice holds
 * (csrc/hops_attended_float.h): exact, no atomics, no scratch.  LDS per query, the 38 368-slot cap and the shared call's tile are
 * the base calls'.  One kernel on `stream`: no second stream, no library scratch, no allocation -- it can be captured in a graph.
 * Nothing is launched, no output is touched and the code returned is: whatever the base call answers for the same arguments
 * without taps, unchanged and FIRST (its refusals; n_query = 0 is QMANN_OK whatever k); then QMANN_EUNSUPPORTED for any
 * attention mode but QMANN_ATT_FLOAT; then QMANN_EINVAL for k = 0, k > QMANN_MAX_TOP_SLOTS, a null top_slot or top_p.
 * (qmann_hops_top_i8 and the other attended-slots calls keep refusing QMANN_ATT_FLOAT as documented above.) */
int qmann_hops_top_float_i8(const qmann_net *net, const int8_t *keys, const int8_t *vals, size_t hop_stride,
                            const uint32_t *row_off, uint32_t max_slots, const float *u0, float *u_out,
                            uint32_t k, uint32_t *top_slot, float *top_p, uint32_t n_query, void *stream);
int qmann_hops_shared_top_float_i8(const qmann_net *net, const int8_t *keys, const int8_t *vals, size_t hop_stride,
                                   uint32_t n_slots, const float *u0, float *u_out, uint32_t k,
                                   uint32_t *top_slot, float *top_p, uint32_t n_query, void *stream);

/* Packed binary codes for the Hamming forms: sign-magnitude bytes [rows][Dp] -> bit planes
 * uint64 [rows][Dp/64][num_bit] (plane 0 = sign bits, plane i = magnitude bit 7-i; bit b of a word
 * is column 64.g + b).  num_bit in 1..8.  sm_codes 16-byte aligned, planes 8-byte aligned (QMANN_EINVAL otherwise). */
int qmann_pack_bitplanes(const int8_t *sm_codes, uint64_t *planes, size_t rows, uint32_t dim_emb_pad,
                         uint32_t num_bit, void *stream);

/* qmann_hops_i8 for QMANN_ATT_HAMMING_V0 / _V1: keys are packed planes (layout above, per hop
 * key_hop_stride bytes apart, num_bit = net->num_bit in {1,2,4,8}), values stay int8.  Scores:
 * V0 = number of agreeing bits over the top num_bit bits of every column (lib/common.c:223-246),
 * V1 = sum over columns of sgn.sgn.sum_{i>=1} 2^-(i+1) [bit i agrees] (lib/common.c:249-312),
 * both on the left-aligned words the CUDA path builds (frac = 31 - iwl, lib/layer_cuda.cu:2515). */
int qmann_hops_packed(const qmann_net *net, const uint64_t *key_planes, size_t key_hop_stride,
                      const int8_t *vals, size_t val_hop_stride, const uint32_t *row_off,
                      uint32_t max_slots, const float *u0, float *u_out, const qmann_taps *taps,
                      uint32_t n_query, void *stream);

/* qmann_hops_packed when every query reads the SAME memory: key_planes uint64 [n_hop][n_slots][Dp/64][num_bit] (the layout of
 * qmann_pack_bitplanes, 16-byte aligned, hop planes key_hop_stride bytes apart), vals int8 [n_hop][n_slots][Dp] sign-magnitude
 * (val_hop_stride bytes apart); both strides 0 = one plane for every hop (tied).  The planes are packed once for all queries and
 * held once -- qmann_hops_packed wants a private copy of keys AND values per query.
 * Results equal qmann_hops_packed on n_query copies of the planes and values, bit for bit; every qmann_net field that call
 * honours is honoured.  Taps as in qmann_hops_shared_i8: score_codes / scores / probs [n_hop][n_query][n_slots], o / u
 * [n_query][n_hop][D]; allowed with stride 0.  One workgroup owns a tile of 1, 2, 4 or 8 queries and scans the planes once per
 * hop for all of them (csrc/batch_hops_shared_ham.hip); the library chooses the tile, QMANN_SHARED_QT forces one that fits.
 * Nothing is launched and the code returned is: QMANN_EUNSUPPORTED for an attention mode other than QMANN_ATT_HAMMING_V0 / _V1,
 * num_bit outside {1, 2, 4, 8}, a single plane of 64 columns (a key row is half a 16-byte load), attention formats the Hamming
 * family refuses (word length 7 with an integer bit is wanted); QMANN_EINVAL for null or misaligned pointers, n_slots = 0, a
 * key_hop_stride that is not val_hop_stride / Dp rows of planes; QMANN_ERANGE for a memory too long for LDS with one query per
 * workgroup (sizing helper below) and for 2^24 queries or more; QMANN_OK for n_query = 0.
 * One ordered step on `stream`, no second stream, no library scratch: it can be captured in a graph. */
int qmann_hops_shared_packed(const qmann_net *net, const uint64_t *key_planes, size_t key_hop_stride,
                             const int8_t *vals, size_t val_hop_stride, uint32_t n_slots, const float *u0,
                             float *u_out, const qmann_taps *taps, uint32_t n_query, void *stream);

/* qmann_hops_shared_packed with the SLOTS cut into slices (csrc/batch_hops_shared_split_ham.hip): for packed memories too long
 * for LDS (up to 2^24 slots) and for batches of so few questions that one workgroup per tile of queries leaves most compute units
 * idle.  Arguments, layouts and taps as qmann_hops_shared_packed; n_slices, ws and ws_bytes as qmann_hops_shared_split_i8.
 * Results equal those of qmann_hops_shared_packed bit for bit wherever that call runs (V0: the softmax is computed from integer
 * counts of the scores, which add across workgroups in any order; V1: the per-slot softmax runs in one workgroup per query on the
 * same int16 scores, in the same order); beyond its cap they are those of qmann_hops_packed on copies, had LDS no limit.
 * Per hop two kernels on `stream` (scan: query tiles x slices; finish: one workgroup per query), for V0 behind one
 * hipMemsetAsync of the bins: at most 1 + 2 n_hop ordered nodes, no library scratch, no second stream, no allocation -- it can be
 * captured in a graph.
 * ws: the CALLER's workspace, 16-byte aligned, at least qmann_hops_shared_split_packed_ws_bytes(net, n_slots, n_query) bytes =
 *   n_query . ( 2 . (n_slots rounded up to 16)                                   int16 scores
 *             + (V0 only) 4 . n_hop . ((num_bit . dim_emb + 1) rounded up to 4)  uint32 bins
 *             + 1024 )                                                           float u [256]
 * Its contents need not survive between calls; two calls that may run at the same time need a workspace each.
 * n_slices: slices wanted, 0 = the library's choice (qmann_hops_shared_split_packed_slices).  A slice is a multiple of 16 rows
 * except the last, so a wish larger than ceil(n_slots / 16) is clamped to that (and to what keeps tiles x slices below 2^31).
 * The query tile is the library's choice (the scan's LDS holds eight queries at any size); QMANN_SHARED_QT forces one.
 * Nothing is launched and the code returned is: every refusal of qmann_hops_shared_packed except the QMANN_ERANGE of a memory too
 * long for LDS; QMANN_EINVAL for a null or misaligned ws or a ws_bytes below the helper's figure; QMANN_ERANGE for n_slots > 2^24
 * and for 2^24 queries or more.  n_query = 0: QMANN_OK.  The helpers answer 0 where a call would launch nothing. */
size_t qmann_hops_shared_split_packed_ws_bytes(const qmann_net *net, uint32_t n_slots, uint32_t n_query);
uint32_t qmann_hops_shared_split_packed_slices(const qmann_net *net, uint32_t n_slots, uint32_t n_query);
int qmann_hops_shared_split_packed(const qmann_net *net, const uint64_t *key_planes, size_t key_hop_stride,
                                   const int8_t *vals, size_t val_hop_stride, uint32_t n_slots, const float *u0,
                                   float *u_out, const qmann_taps *taps, uint32_t n_query, uint32_t n_slices, void *ws,
                                   size_t ws_bytes, void *stream);

/* Attended slots for the packed Hamming forms: qmann_hops_shared_packed / qmann_hops_shared_split_packed that also return, per
 * query and hop, the k memory rows the hop weighted most and their weights, as qmann_hops_shared_top_i8 does for the fixed-point
 * attention -- without a [n_hop][n_query][n_slots] array anywhere.
 *   top_slot [n_query][n_hop][k] uint32, top_p [n_query][n_hop][k] float, device memory; 1 <= k <= QMANN_MAX_TOP_SLOTS.
 * In terms of what qmann_hops_shared_packed writes to taps.probs for the same arguments: row (q, h) lists the k slots of
 * probs[h][q][:] that come first in the order "larger probability first, equal probabilities: lower slot index first", and
 * top_p[q][h][j] is bit-equal to probs[h][q][top_slot[q][h][j]].  The order is over the probability VALUES: slots whose scores
 * differ tie where their probabilities are equal floats, a NaN probability ranks below every number, and a negative att_scale
 * needs no rule of its own.  Where k > n_slots the entries past n_slots hold slot 0xFFFFFFFF and p 0.0f.
 * u_out is the base call's bit for bit, and every qmann_net field the base call honours is honoured (the three softmax bases,
 * the shift-based normaliser, att_scale of either sign, ReLU, binary u, tied hops with both strides 0, the per-hop formats of
 * the mixed quantisation, num_bit in {1, 2, 4, 8}).  There is no taps argument: a host that wants taps calls the base functions.
 * The selection runs inside the base call's kernels (csrc/hops_attended_ham.h).  V0: from the bins and the probability per bin
 * the histogram softmax leaves behind.  V1: from the int16 scores and the softmax's own maximum and total, ALL slots ranked,
 * those below the threshold shortcut of the survivor search included.  LDS per query, tiles, caps and the split workspace are
 * the base call's: the split call takes the SAME workspace and qmann_hops_shared_split_packed_ws_bytes figure as
 * qmann_hops_shared_split_packed.  Both are ordered steps on `stream` with the node counts of their base calls (1; at most
 * 1 + 2 n_hop), no allocation, no library scratch, no second stream: they can be captured in a graph.
 * Nothing is launched, no output is touched and the code returned is: every refusal of the respective base call, unchanged and
 * FIRST (a call with a fault of the base call and a fault below returns the base call's code; n_query = 0 is QMANN_OK whatever
 * k); then QMANN_EINVAL for k = 0, k > QMANN_MAX_TOP_SLOTS, a null top_slot or top_p.  k > n_slots is no error. */
int qmann_hops_shared_top_packed(const qmann_net *net, const uint64_t *key_planes, size_t key_hop_stride,
                                 const int8_t *vals, size_t val_hop_stride, uint32_t n_slots, const float *u0,
                                 float *u_out, uint32_t k, uint32_t *top_slot, float *top_p, uint32_t n_query, void *stream);
int qmann_hops_shared_split_top_packed(const qmann_net *net, const uint64_t *key_planes, size_t key_hop_stride,
                                       const int8_t *vals, size_t val_hop_stride, uint32_t n_slots, const float *u0,
                                       float *u_out, uint32_t k, uint32_t *top_slot, float *top_p, uint32_t n_query,
                                       uint32_t n_slices, void *ws, size_t ws_bytes, void *stream);

/* Answer layer for a batch: logits = W_ans . u (float, ds_ans is always float: MemN2N.c:902-906),
 * softmax over V, arg-max with ties to the highest index, and -- when `answer` is given -- the
 * test-phase bookkeeping of cross_entropy_run mode 3 (cost += -p[answer], match += pred==answer).
 *   w_ans [V][D] float, answer [n_query] uint32 or NULL, pred [n_query] uint32,
 *   probs [n_query][V] float or NULL, cost/match: single device words (accumulated) or NULL.
 * Arithmetic.  qmann_answer_f32_serial sums every logit over the embedding axis serially in float, separate multiply and add:
 * the reference's own order (lib/layer_cuda.cu:70-80), bit-equal logits; e^x through expf, a double total, the quotient of the
 * double division (:2006-2042).  qmann_answer_f32 takes, at the bAbI shapes (dim_emb <= 64, dim_input <= 256, e^x / 2^x base),
 * the FUSED form on the bf16 matrix cores instead (csrc/answer_fused.h::k_answer_mfma): u -- which must lie on an 8-bit grid, as
 * the hop kernels write it -- times W split exactly into three bf16 parts, float accumulation, hardware 2^x; closer to the
 * exact sum than the serial float loop, and within north_star's 1e-5 of it on the probabilities (absolute; relative 1e-5 while
 * |logit| <= 16, where a unit in the last place of a logit is still below 1e-6); predictions agree wherever the two best
 * probabilities differ by more than 1e-6, exact ties go to the highest index in both.  Nine times fewer vector instructions
 * per query at the joint dictionary.  QMANN_ANSWER_EXACT (environment) makes qmann_answer_f32 the serial form everywhere;
 * the drop-in queue behind the cuda_* verbs always runs the serial form. */
int qmann_answer_f32(const qmann_net *net, const float *w_ans, const float *u, const uint32_t *answer,
                     uint32_t *pred, float *probs, float *cost, uint32_t *match, uint32_t n_query,
                     void *stream);
int qmann_answer_f32_serial(const qmann_net *net, const float *w_ans, const float *u, const uint32_t *answer,
                            uint32_t *pred, float *probs, float *cost, uint32_t *match, uint32_t n_query,
                            void *stream);

/* Ranked answers: per query the k most probable answers and their probabilities, without a [n_query][V] array anywhere.
 *   top_idx [n_query][k] uint32, top_p [n_query][k] float; 1 <= k <= QMANN_MAX_TOPK, k <= dim_input.
 * In terms of what qmann_answer_f32_serial writes for the same net, w_ans and u: top_p[q][j] is bit-equal to its
 * probs[q][top_idx[q][j]], and row q lists the k entries of probs[q][:] that come first in the order "larger probability first,
 * equal probabilities: higher index first" -- the tie rule of pred (lib/layer_cuda.cu:1918-1939), so top_idx[q][0] is the serial
 * call's pred[q] always, also among probabilities that underflowed to 0.  Every softmax base.  The kernels are the serial-order
 * ones of the shape with k rounds of their arg-max reduction behind the quotients (csrc/answer_serial.h); the fused bf16 form
 * has no ranked build; qmann_answer_i8's int8 matrices have one of their own, qmann_answer_topk_i8 below.
 * One ordered step on `stream`, no allocation, no library scratch, no second stream: it can be captured in a graph.
 * Nothing is launched and the code returned is: QMANN_EINVAL for null pointers, k = 0, k > QMANN_MAX_TOPK, k > dim_input,
 * dim_emb = 0, dim_input = 0; QMANN_ERANGE where qmann_answer_f32_serial answers it (a query's LDS beyond 128 KiB, 2^24 queries
 * or more); QMANN_OK for n_query = 0. */
#define QMANN_MAX_TOPK 16
int qmann_answer_topk_f32(const qmann_net *net, const float *w_ans, const float *u, uint32_t k,
                          uint32_t *top_idx, float *top_p, uint32_t n_query, void *stream);

/* The same answer layer when the answer matrix is on an int8 grid: w_ans_i8 [V][Dp] two's-complement
 * codes of Q(w_fmt); the projection runs on the int8 matrix cores (v_mfma_i32_16x16x64_i8).
 *   probs == NULL: one pass -- projection, running-maximum softmax statistics and arg-max in the accumulator registers, W
 *       tiles shared through LDS, no [n_query][V] logits round trip.  Predictions (ties to the highest index) and the match
 *       count equal the float path exactly (logits are exact integers); the cost -p[answer] agrees within the 1e-5 softmax
 *       tolerance (normaliser accumulated against the running maximum, hardware exp as the reference's __expf).
 *   probs != NULL: two kernels -- logits to the workspace, then the float path's softmax on them: probabilities bit-identical
 *       to qmann_answer_f32_serial on the same grid values.
 * logits_ws: caller-provided workspace, float [n_query][V], 8-byte aligned: the one-pass form keeps its per-slice records there
 * (16 bytes each, holding a double), one per dictionary slice and query, at most ceil(V / 64) slices.  A dictionary of 1, 2 or 3
 * answers has less workspace per query than one record: such a call takes the two-kernel form whatever `probs` is (the logits
 * round trip costs nothing there), and its results are that form's, bit-identical to qmann_answer_f32_serial.  So do the exp_plan
 * softmax base (no true exponential to rescale a running maximum by) and every call under QMANN_ANSWER_TWO_PASS (environment).
 * Nothing is launched, no output is touched and the code returned is: QMANN_EINVAL for a null net, w_ans_i8, u, logits_ws or pred,
 * dim_emb = 0, dim_input = 0, dim_emb_pad not a multiple of 64, dim_emb > dim_emb_pad; QMANN_ERANGE for an activation format (the
 * last hop's) or a w_fmt that is no byte format (1 <= iwl + frac <= 7), a query's LDS beyond 128 KiB (dim_emb rounded up to 4,
 * plus dim_input, floats), 2^24 queries or more; QMANN_OK for n_query = 0; QMANN_EUNSUPPORTED for a dim_emb_pad other than 64, 128
 * or 256.  The checks run in this order; the first that fails decides. */
int qmann_answer_i8(const qmann_net *net, const int8_t *w_ans_i8, qmann_fmt w_fmt, const float *u,
                    float *logits_ws, const uint32_t *answer, uint32_t *pred, float *probs, float *cost,
                    uint32_t *match, uint32_t n_query, void *stream);

/* Ranked answers for the int8 answer layer: per query the k answers with the largest logits and their probabilities, projection,
 * softmax statistics and selection in ONE pass on the int8 matrix cores -- no [n_query][V] array in that form.
 *   net, w_ans_i8 [V][Dp], w_fmt, u: exactly qmann_answer_i8's operands (u is read through the last hop's activation format:
 *       truncation toward zero, symmetric saturation, so off-grid and saturating u behave as they do there).
 *   top_idx [n_query][k] uint32, top_p [n_query][k] float; 1 <= k <= QMANN_MAX_TOPK, k <= dim_input.
 * Ranking.  K[q][v] is the integer logit code, query codes times row v of w_ans_i8 -- the integer the matrix cores produce.  Row q
 * of top_idx lists the k answers that come first in the order "larger K first, equal K: higher index first"; top_idx[q][0] is
 * qmann_answer_i8's pred[q] always.  The order is exact by construction: a candidate is the 64-bit key ((K + 2^28) << 32) | v.
 * This differs from qmann_answer_topk_f32 ON PURPOSE: that call ranks the ROUNDED PROBABILITIES, so two different logits whose
 * probabilities round to the same float (denormals or 0, once the exponential underflows) are ordered by index there; here they
 * stay ordered by logit.  Wherever the listed probabilities are pairwise distinct or the codes are equal the two orders coincide.
 * Probabilities.
 *   One-pass form: top_p[q][j] = e^((K - max) . scale) / total (or the 2^x base's), with the running-maximum normaliser of
 *       qmann_answer_i8's one-pass form: within rtol 1e-5 / atol 1e-7 of the float64 softmax of the exact logits.
 *   Two-kernel form -- taken exactly where qmann_answer_i8 takes it whatever `probs` is: the exp_plan base, QMANN_ANSWER_TWO_PASS,
 *       a dictionary of 1, 2 or 3 answers: logits to the workspace, then the float path's softmax on them; top_p[q][j] is BIT-EQUAL
 *       to probs[q][top_idx[q][j]] of qmann_answer_i8(..., probs != NULL) on the same inputs.  The order is still the logit order.
 * ws: the caller's workspace, 8-byte aligned, at least qmann_answer_topk_i8_ws_bytes(net, k, n_query) bytes: the larger of the
 * two-kernel form's float [n_query][V] (rounded up to 8 bytes) and the one-pass records -- per dictionary slice and query 16 bytes
 * (maximum, sum) plus k keys of 8 bytes, the slices being those of qmann_answer_i8 for the same batch (at most ceil(V / 64)).  The
 * figure does not depend on the form, so a switch flipped between the two calls does no harm.  The helper answers 0 for a net or k
 * the call would refuse.  The contents need not survive between calls.
 * One ordered step on `stream` (two kernels), no allocation, no library scratch, no second stream: it can be captured in a graph.
 * Nothing is launched, no output is touched and the code returned is, in this order, the first that applies:
 *   1. every refusal of qmann_answer_i8 for net, w_ans_i8, w_fmt, u, the dimensions, the formats and a query's LDS, with its codes
 *      (top_idx / top_p take pred's place in the null check);
 *   2. QMANN_EINVAL for k = 0, k > QMANN_MAX_TOPK or k > dim_input;
 *   3. QMANN_EINVAL for a null or misaligned ws, or ws_bytes below the helper's figure for this call;
 *   4. QMANN_OK for n_query = 0;
 *   5. QMANN_ERANGE for 2^24 queries or more;
 *   6. QMANN_EUNSUPPORTED for a dim_emb_pad other than 64, 128 or 256. */
size_t qmann_answer_topk_i8_ws_bytes(const qmann_net *net, uint32_t k, uint32_t n_query);
int qmann_answer_topk_i8(const qmann_net *net, const int8_t *w_ans_i8, qmann_fmt w_fmt, const float *u,
                         void *ws, size_t ws_bytes, uint32_t k, uint32_t *top_idx, float *top_p,
                         uint32_t n_query, void *stream);

/* Story / question embedding for a batch of bag-of-words inputs (dense_mat_fwd / dense_fwd,
 * lib/layer_cuda.cu:3511, :3162), writing the int8 memories directly.
 *   story [rows_total][V] float (word counts + time bit), w_a[h], w_c[h], w_q : [D][V] float. */
int qmann_embed_story(const qmann_net *net, const float *story, uint32_t rows_total,
                      const float *const *w_a, const float *const *w_c, int8_t *keys, int8_t *vals,
                      size_t hop_stride, void *stream);
int qmann_embed_query(const qmann_net *net, const float *question, const float *w_q, float *u0,
                      uint32_t n_query, void *stream);

/* Bag-of-words rows -> word lists, for callers that hold the reference's float pools (dev_m_test / dev_q_test,
 * MemN2N.c:2337-2349) and want the word-index kernels' speed: a row whose non-zero entries are integers 1..16 (counts;
 * the time entry is a 1) becomes words[row][0..15] (ascending indices, an index repeated by its count, 0xFFFF = unused) --
 * feed them to qmann_embed_story_idx with max_words = 16 and time_last = 0 (every entry counts), or to
 * qmann_embed_query_idx.  Any other row (fractional or negative entries such as EN_PE position weights, more than 16 words)
 * gets an empty list and its index is appended to irregular_rows[(*n_irregular)++] (device memory, capacity `rows`;
 * *n_irregular is NOT reset here): redo exactly those rows with the float kernels through qmann_embed_story_rows /
 * qmann_embed_query_rows, which take the list and read its length on the device -- no host round trip. */
int qmann_bow_to_words(const float *bow, uint32_t rows, uint32_t dim_input, uint16_t *words, uint32_t *irregular_rows,
                       uint32_t *n_irregular, void *stream);
int qmann_embed_story_rows(const qmann_net *net, const float *story, uint32_t rows_total, const uint32_t *row_list,
                           const uint32_t *n_list, const float *const *w_a, const float *const *w_c, int8_t *keys,
                           int8_t *vals, size_t hop_stride, void *stream);
int qmann_embed_query_rows(const qmann_net *net, const float *question, const uint32_t *row_list, const uint32_t *n_list,
                           const float *w_q, float *u0, uint32_t n_query, void *stream);

/* Compact wire format for stories: word indices instead of float bag-of-words
 * rows.  words: uint16 [rows][max_words] (max_words <= 16, unused entries 0xFFFF); with time_last the
 * last valid entry of a row is its time-encoding index (bag-of-words entry SET to 1; word entries
 * COUNT occurrences -- MemN2N/sample.c:466-475, 544-548).  Tables: int8 [V][Dp] two's-complement
 * codes of Q(w[h]) made by qmann_quantize_table_i8 from the float [D][V] matrices.  Results are
 * bit-identical to qmann_embed_story / qmann_embed_query on the equivalent bag-of-words input (with net->en_pe: on the
 * question row that carries the position weights). */
int qmann_quantize_table_i8(const float *w, int8_t *table, uint32_t dim_emb, uint32_t dim_emb_pad,
                            uint32_t dim_input, qmann_fmt fmt, void *stream);
/* The way back: a table's codes as the float matrix [D][V] of grid values (code . 2^-frac, exact).  Quantising that matrix
 * again gives the same table, and the float embedding kernels (which quantise their weights on entry, as dense_mat_fwd does)
 * give the same memories from it as from the original matrix -- so a model can live on its int8 tables alone. */
int qmann_dequantize_table_f32(const int8_t *table, float *w, uint32_t dim_emb, uint32_t dim_emb_pad, uint32_t dim_input,
                               qmann_fmt fmt, void *stream);
int qmann_embed_story_idx(const qmann_net *net, const uint16_t *words, uint32_t rows_total, uint32_t max_words,
                          int time_last, const int8_t *const *t_a, const int8_t *const *t_c, int8_t *keys,
                          int8_t *vals, size_t hop_stride, void *stream);
int qmann_embed_query_idx(const qmann_net *net, const uint16_t *words, uint32_t max_words, const int8_t *t_q,
                          float *u0, uint32_t n_query, void *stream);
/* the kernel form qmann_embed_story_idx would take for this call (QMANN_EMBED_VALU / _PER_HOP included), or the negative
 * code the call would return -- for tests and timing tools that must know which kernel ran */
enum { QMANN_EMBED_GATHER_LDS = 0, QMANN_EMBED_GATHER_L2 = 1, QMANN_EMBED_MFMA_PER_HOP = 2, QMANN_EMBED_MFMA_ALL_HOPS = 3 };
int qmann_embed_story_idx_form(const qmann_net *net, const uint16_t *words, uint32_t max_words);

/* Validation helper: *n_over (a device word, accumulated into) += the number of queries whose story is longer than
 * max_slots, i.e. would be cut by the hop kernels. */
int qmann_check_slots(const uint32_t *row_off, uint32_t n_query, uint32_t max_slots, uint32_t *n_over, void *stream);

/* bytes of LDS one workgroup of qmann_hops_i8 needs for `max_slots` slots (for sizing checks) */
size_t qmann_hops_lds_bytes(uint32_t max_slots);
/* ... and one workgroup of qmann_hops_shared_i8 that owns `queries_per_group` queries of an `n_slots`-slot memory; the call
 * needs this to stay within 160 KiB - 1 KiB for queries_per_group = 1 */
size_t qmann_hops_shared_lds_bytes(uint32_t n_slots, uint32_t queries_per_group);
/* queries per workgroup qmann_hops_shared_i8 would take for this call on the current device, QMANN_SHARED_QT included
 * (1, 2, 4 or 8; 0 where the call would launch nothing) -- for tests and timing tools that must know which tile ran */
uint32_t qmann_hops_shared_tile(uint32_t n_slots, uint32_t n_query);

/* the same two for qmann_hops_shared_float_i8, which keeps a float per slot and query:
 * queries_per_group . (qmann_hops_lds_bytes(0) + 4 . n_slots rounded up to 16); within 160 KiB - 1 KiB for one query (up to
 * 38 368 slots) or the call returns QMANN_ERANGE; the tile is 0 where the call would launch nothing */
size_t qmann_hops_shared_float_lds_bytes(uint32_t n_slots, uint32_t queries_per_group);
uint32_t qmann_hops_shared_float_tile(uint32_t n_slots, uint32_t n_query);

/* the same two for qmann_hops_shared_packed, whose LDS depends on the net (V0 keeps tables of num_bit . dim_emb + 1 bins per
 * query): bytes of one workgroup that owns `queries_per_group` queries (within 160 KiB - 1 KiB for one query, or the call
 * returns QMANN_ERANGE), and the tile the call would take (0 where it would launch nothing) */
size_t qmann_hops_shared_packed_lds_bytes(const qmann_net *net, uint32_t n_slots, uint32_t queries_per_group);
uint32_t qmann_hops_shared_packed_tile(const qmann_net *net, uint32_t n_slots, uint32_t n_query);

/* The library's A/B switches (environment variables QMANN_NO_LEAN, QMANN_NO_MID, QMANN_NO_W7, QMANN_NO_TIED, QMANN_NO_TIGHT,
 * QMANN_SHARED_QT, QMANN_LEAN_SPARSE, QMANN_EMBED_VALU, QMANN_EMBED_PER_HOP, QMANN_EMBED_GENERAL_EPILOGUE, QMANN_ANSWER_TWO_PASS: INTEGRATION.md) are read ONCE,
 * at the first call that needs one; no launch touches the environment afterwards.  A host that changes one later calls
 * this to have them read again -- from one thread, while no other thread is inside the library. */
void qmann_tuning_reload(void);

#ifdef __cplusplus
}
#endif
#endif /* QMANN_BATCH_H */
