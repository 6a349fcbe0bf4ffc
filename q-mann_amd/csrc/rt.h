// rt.h -- tiny runtime layer: error convention, allocation, launch helpers.
// Error convention of the boundary (lib/layer_cuda.h:13-22 in the reference):
// message on stderr, then exit(code).
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <type_traits>
#include "../../include/qmann_batch.h"

// The batched entry points (qmann_*: they return QMANN_E* codes) do not end the host process on a HIP failure: inside a
// QmBatched scope the failure is reported on stderr, remembered, and the entry point returns QMANN_EHIP.  The drop-in
// cuda_* verbs keep the reference's convention (exit), they have no way to return an error.
inline thread_local int qm_batched_depth = 0;
inline thread_local int qm_batched_err = 0;
struct QmBatched {
    // The outermost scope starts clean: hipGetLastError() reads AND clears the thread's last error, so a failure an earlier
    // call reported (or one the host application left behind) is not reported again by this call's launch checks.
    QmBatched() { if (qm_batched_depth++ == 0) { qm_batched_err = 0; (void)hipGetLastError(); } }
    ~QmBatched() { --qm_batched_depth; }
    QmBatched(const QmBatched &) = delete;
    int rc(int ok = 0) const { return qm_batched_err ? -5 /* QMANN_EHIP */ : ok; }
};

#define QM_HIP(call)                                                                  \
    do {                                                                              \
        hipError_t e_ = (call);                                                       \
        if (e_ != hipSuccess) {                                                       \
            fprintf(stderr, "[*E] HIP : %s : %s (%s:%d)\n", __func__,                 \
                    hipGetErrorString(e_), __FILE__, __LINE__);                       \
            if (qm_batched_depth > 0) qm_batched_err = (int)e_;                       \
            else exit((int)e_ ? (int)e_ : 1);                                         \
        }                                                                             \
    } while (0)

// (hipGetLastError, not hipPeekAtLastError: the error is consumed when it is reported, a later valid call is not blamed for it)
#define QM_LAUNCH_CHECK() QM_HIP(hipGetLastError())

static inline void qm_fail(const char *fn, const char *msg)
{
    fprintf(stderr, "[*E] qmann : %s : %s\n", fn, msg);
    exit(1);
}

template <typename T>
static inline void qm_alloc(T **p, size_t n)
{
    // zero-sized requests still hand back a valid pointer, like cudaMalloc(0) would not:
    // the reference never frees a null, so keep every slot non-null
    QM_HIP(hipMalloc((void **)p, (n ? n : 1) * sizeof(T)));
}

// The library's A/B and tuning switches (INTEGRATION.md lists them) are read from the environment ONCE per process -- on
// first use, through a thread-safe function-local static -- and then live in this struct: no launch calls getenv(), which
// is not safe against a setenv() running in another thread of a threaded host (examples/forward_sharded.c is one).
// qmann_tuning_reload() (include/qmann_batch.h) reads the environment again, for hosts and tests that change a switch
// after the first launch; it must not run while another thread launches.
struct QmTuning {
    bool no_w7, no_mid, no_lean, no_tied, embed_general_epilogue, embed_valu, answer_two_pass;
    bool embed_per_hop;                               // QMANN_EMBED_PER_HOP: the joint-dictionary story embedding keeps one workgroup per hop (k_embed_story_mfma<4, 16>)
    bool answer_exact;                                // QMANN_ANSWER_EXACT: the float answer layer keeps the reference's serial order of additions (no bf16 MFMA form)
    bool no_quad_long;                                // QMANN_NO_QUAD_LONG: stories of 17 .. 64 rows keep the one-wavefront-per-query kernel (hops_quad.h's four-chunk form off)
    bool no_corun;                                    // QMANN_NO_CORUN: no second stream (the two hop kernels of a split batch, the question embedding beside the story embedding: in sequence)
    bool no_quad;                                     // QMANN_NO_QUAD: short stories keep the one-wavefront-per-query kernel (hops_quad.h off)
    bool no_tight;                                    // QMANN_NO_TIGHT (set, any value): the lean kernels keep their four-wave (128-register) builds
    bool no_scan_stop;                                // QMANN_NO_SCAN_STOP (set, any value): the fixed-point hop kernel scans every key row even where the read-out is already known to be zero (batch_hops.hip, step 1b)
    int lean_sparse;                                  // -1 = the launcher chooses, 0 / 1 forced
    uint32_t shared_qt;                               // QMANN_SHARED_QT (1, 2, 4 or 8): queries per workgroup of qmann_hops_shared_i8 where they fit in LDS; 0 = the launcher chooses
    uint32_t quad_min_queries;                        // QMANN_QUAD_MIN_QUERIES (default 8192): batches of at most this many stories keep one story per wavefront (hops_lean.h)
};
const QmTuning &qm_tuning();                          // (tuning.hip)

// compute units of the CURRENT device (256 on an MI355X in SPX mode; fewer in a partitioned mode), asked once per device ordinal
unsigned qm_cu_count();                               // (tuning.hip)

// Persistent kernels: how many workgroups of `waves` wavefronts are resident AT ONCE on the device, for a kernel compiled for
// `waves_per_simd` wavefronts per SIMD (its __launch_bounds__) that takes `lds` bytes of LDS per workgroup.  A persistent grid
// must not exceed this: a workgroup that has to wait for a slot runs after the others, alone on a mostly idle chip -- two extra
// workgroups on a one-per-CU kernel double its run time (round 4 found three launchers sized by LDS alone).
static inline unsigned qm_resident_groups(unsigned waves, unsigned waves_per_simd, size_t lds)
{
    const unsigned by_regs = waves_per_simd * 4u / waves, by_lds = (unsigned)(160u * 1024u / (lds + 256u)), by_hw = 32u / waves;
    unsigned per_cu = by_regs < by_lds ? by_regs : by_lds;
    per_cu = per_cu < by_hw ? per_cu : by_hw;
    return qm_cu_count() * (per_cu ? per_cu : 1u);
}

// Device scratch of at least `words` 32-bit words for the launch being enqueued on `stream` (index lists of a batch split by
// story length): one buffer per (device, stream), grown when a launch needs more (the only time this allocates -- like a model's
// workspace it reaches its size on the first batches), kept for the life of the process.  nullptr when the allocation fails.
uint32_t *qm_scratch_u32(size_t words, hipStream_t stream);

// A second stream beside `stream` with the two events that fork work onto it and join it back (cached per (device, stream)).
struct QmSide {
    hipStream_t side;
    hipEvent_t fork, join;
    // pinned host words: the two list lengths (short, long) of the LAST batch split by length on this stream, stored by its
    // short-story kernel (hops_quad.h: QuadArgs::publish) -- no copy, no synchronisation; 0xFFFFFFFF until one has landed.  A hint for the next launch's choice between
    // "side by side" and "in sequence" only -- never a result.
    volatile uint32_t *last_counts;
};
// What a caller inside the library knows about a hop call beyond the public arguments; the public qmann_hops_* pass an empty one.
struct QmHopHints {
    // The plane's size in rows for calls that pass hop_stride = 0 (tied hops: one plane for every hop); 0 = unknown.  hops_quad.h
    // addresses rows by 32-bit byte offsets and must know that the plane stays below 2 GiB: without it such a call keeps the lean kernel.
    size_t plane_rows = 0;
    // The index lists of THIS call's (row_off, n_query, max_slots) from qm_split_early, made ahead of the launch; null = none
    uint32_t *split_ws = nullptr;
    // qmann_hops_top_i8: the call also returns each hop's attended slots -- top_slot / top_p [n_query][n_hop][top_k], unchecked
    // until the base call's own refusals are through (the entry points check them last); top_on = false: a plain call
    bool top_on = false;
    // qmann_hops_top_float_i8: the attended slots of float attention -- every other mode answers QMANN_EUNSUPPORTED where it would
    // check top_k / top_slot / top_p, and float attention serves the call instead of refusing it (needs top_on)
    bool top_float = false;
    uint32_t top_k = 0;
    uint32_t *top_slot = nullptr;
    float *top_p = nullptr;
};
// qmann_hops_i8 / qmann_hops_packed (include/qmann_batch.h) with the caller's hints         (batch_hops.hip, batch_hops_ham.hip)
int qm_hops_i8(const qmann_net *net, const int8_t *keys, const int8_t *vals, size_t hop_stride, const uint32_t *row_off, uint32_t max_slots,
               const float *u0, float *u_out, const qmann_taps *taps, uint32_t n_query, void *stream, const QmHopHints &hints);
int qm_hops_packed(const qmann_net *net, const uint64_t *key_planes, size_t key_hop_stride, const int8_t *vals, size_t val_hop_stride, const uint32_t *row_off,
                   uint32_t max_slots, const float *u0, float *u_out, const qmann_taps *taps, uint32_t n_query, void *stream, const QmHopHints &hints);
// Will qm_hops_i8 on int8 planes of `plane_rows` rows split this batch by story length (hops_host.h::hop_form of the call)?  Then
// the lists can be made early: [0] short count, [1] long count, the two lists (hops_quad.h::split_lists), in the scratch words of
// stream `owner`, computed on `run_on`.
bool qm_hops_will_split(const qmann_net *net, size_t plane_rows, uint32_t max_slots, uint32_t n_query);       // (batch_hops.hip)
uint32_t *qm_split_early(const uint32_t *row_off, uint32_t n_query, uint32_t max_slots, hipStream_t owner, hipStream_t run_on);
// qmann_model_forward_* of `m` keep the serial-order float answer kernels (bit-equal to lib/layer_cuda.cu:70-80's loop): set by the
// drop-in queue (abi_defer.hip), whose results are promised to be those of the verb-by-verb loop.     (model_host.hip)
struct qmann_model;
void qm_model_answer_exact(qmann_model *m, bool exact);
constexpr uint32_t kQmCorunMinQueries = 32768;        // batches below run their kernels in sequence (measured equal at 32 768 and 65 536 queries, +4 % at 262 000)
QmSide *qm_side_stream(hipStream_t stream);       // (tuning.hip)

static inline unsigned qm_cdiv(unsigned a, unsigned b) { return (a + b - 1) / b; }

// The batched entry points give one workgroup (or wavefront) to a query: a launch holds < 2^32 threads
static inline bool qm_too_many_queries(uint32_t n_query) { return n_query >= (1u << 24); }

// ---- launches -------------------------------------------------------------------------------------------------------------
// dynamic LDS a kernel may use without hipFuncSetAttribute (static arrays come on top, hence the margin)
constexpr size_t kLdsDefaultLimit = 48 * 1024;
// dynamic LDS a hop launch may take (a CU has 160 KiB; a little static LDS is used besides).  ONE value for every hop entry
// point's QMANN_ERANGE and for the host model (model_host.hip), which refuses a memory ahead of the ask that would.
constexpr size_t kHopLdsLimit = 160 * 1024 - 1024;

// One launch: beyond the default limit the kernel's dynamic-LDS limit is raised first (no cached state: thread- and
// device-safe).  The caller checks the launch (QM_LAUNCH_CHECK).
template <typename... P, typename... A>
static inline void qm_launch(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t stream, const A &...args)
{
    if (lds > kLdsDefaultLimit)
        QM_HIP(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    kernel<<<grid, block, lds, stream>>>(args...);
}

// A persistent kernel's workgroup: `waves` wavefronts, compiled for `waves_per_simd` (its __launch_bounds__); `static_lds`: LDS
// the residency rule counts on top of the launch's dynamic bytes; `grid_y`: the residents are shared among this many planes of
// a two-dimensional grid.
// (static_lds has one user, k_answer_mfma's 256 bytes, kept as its launcher always had it -- on top of the 256 that
// qm_resident_groups adds itself, so that margin is counted twice; grid_y has one user, k_embed_story_mfma.  Whether the
// first should go is a question of grid size, hence of timing: for a change of its own.)
struct QmPersistent { unsigned waves, waves_per_simd; size_t static_lds = 0; unsigned grid_y = 1; };

// A persistent launch: `need` workgroups' worth of work (per plane), never more workgroups than are resident at once
// (qm_resident_groups above)
template <typename... P, typename... A>
static inline void qm_launch_persistent(void (*kernel)(P...), uint32_t need, QmPersistent wg, size_t lds, hipStream_t stream, const A &...args)
{
    const uint32_t resident = qm_resident_groups(wg.waves, wg.waves_per_simd, lds + wg.static_lds);
    const uint32_t cap = resident / wg.grid_y ? resident / wg.grid_y : 1u;
    qm_launch(kernel, dim3(need < cap ? need : cap, wg.grid_y), dim3(wg.waves * 64u), lds, stream, args...);
}

// Run-time value -> template argument: f(std::integral_constant<.., V>{}) for the listed V that equals v; false when none does
template <auto... Vs, typename T, typename F>
static inline bool qm_dispatch(T v, F &&f)
{
    return ((v == (T)Vs ? (f(std::integral_constant<decltype(Vs), Vs>{}), true) : false) || ...);
}
