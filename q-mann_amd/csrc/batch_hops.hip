// batch_hops.hip -- the hot path: every hop of every query in one launch.
//
// One 256-thread workgroup (4 wavefronts) owns one query and walks its hops in
// order (hops are sequentially dependent: u_{h+1} = H.u_h + o_h).  Per hop:
//
//   1. key scan (HBM-bound): the query's key plane, sign-magnitude int8 [S][Dp]
//      row-major, is streamed with 16-byte non-temporal loads -- a wavefront
//      instruction covers 1 KiB = 64/LPR whole rows (LPR = Dp/16 lanes per row);
//      each wavefront keeps two tiles of four such loads in flight (the next
//      tile is issued before the current one is reduced).  Each lane combines
//      its 16 key codes with the 16 query codes it keeps in registers, with the
//      reference's per-product quantisation Qm(Qm(k).Qv(u)) (lib/layer_cuda.cu:120):
//      magnitudes are multiplied in packed 16-bit lanes by the pre-shifted |u| so
//      that truncation is a logical shift and the clamp is the multiplier's own
//      unsigned saturation (see ScanConst), signs become +-1 bytes through one
//      v_perm_b32 and are applied by one v_dot4 per 4 bytes (12 VALU ops per 4 bytes).  Row sums meet across the LPR lanes
//      with DPP adds (no LDS), are clamped to the attention format (:135) and
//      land in LDS as one byte per slot, plus a per-wavefront histogram of the
//      (at most 255) score codes.
//   2. softmax over slots from the histogram: scores live on an 8-bit grid, so
//      exp(x - max) takes at most 255 distinct values; the normaliser is
//      sum_d count[d].e[d] in double (lib/layer_cuda.cu:2024-2042) and the
//      read-out weight code Q(p) is a 255-entry table.
//   3. weighted read-out: Q(p) is zero for every slot with p < 2^-frac, so only
//      the few surviving rows of the value plane are read (bit-identical to
//      summing all rows: the skipped terms are exact zeros, :562).
//   4. linear map H.u (int8 [D][Dp], L2-resident) and u' = Q(Q(Hu) + Q(o)).
//
// All integer work is exact; the only floating-point step is the softmax table.
//
//   1b. (the STOP instantiation: e^x softmax, no taps, a bound some hop can reach -- hops_host.h::scan_stop_gate)  While it
//      scans, the workgroup also sums e^(x_r - Xb) over the rows retired so far, Xb the largest score the attention format
//      can hold, and credits every row NOT yet read with the least it can weigh, f = e^(Xmin - Xb), Xmin the smallest such
//      score.  Once the two together pass 2^frac (1 + 2^-6) every read-out weight of the hop is known to quantise to code 0
//      whatever the unread rows hold (derivation: ScanStop below): the wavefronts leave the scan, steps 2 and 3 are skipped
//      and the hop continues with o = 0, the result the full scan would have produced.  (Kept as one word: the retired rows'
//      e^(x_r - Xb) - f against the threshold less S f.  Where S f alone passes it, no row is read at all.)  This scan works in units of
//      two loads per lane (half a tile), three per wavefront -- one being retired, two in flight: the lanes that retire
//      a unit's rows add the rows' terms to the workgroup's sum, THEN the wavefront looks at that sum (its own unit included),
//      and only then asks for another unit.
#include "hops_mid.h"
#include "hops_float_common.h"      // (float_story_lds_bytes: the float launcher's refusal, said here for the top call)
#include "hops_host.h"

namespace {

// Why a hop's key scan may end early.  The e^x softmax gives slot r the weight p_r = (float)(e_r / total), e_r =
// expf(x_r - xmax) <= 1 and total = sum_r e_r in double (hops_common.h::sm_quot).  qm_code (qfmt.h) truncates p . 2^frac toward
// zero, so p_r < 2^-frac is weight code 0; with e_r <= 1 that holds for EVERY slot as soon as total > 2^frac, and the read-out
// is then exactly 0 (readout_sparse with no surviving row).  Scores are clamped to the attention format, so whatever the unread
// rows hold, xmax <= Xb = max(sm_scaled(+maxm / 2^frac_m), sm_scaled(-maxm / 2^frac_m)) (the second term for a negative scale
// layer; sm_scaled is one float product, monotone in the code), and over any set P of rows already retired
//     total >= sum_{r in P} e^(x_r - xmax) >= sum_{r in P} e^(x_r - Xb).
// The sum on the right is what the scan accumulates -- in float, one v_exp_f32 per row (1 ulp, arguments <= 0, a flushed
// denormal only lowers it), an exponent folded into one FMA (argument off by < 2e-5) and ONE addition per row into the
// workgroup's float (each within 2^-24 relative; a term too small to move the sum only lowers it).  LDS holds at most 153 472
// score bytes (hops_common.h's carve-up in 159 KB), so even if every addition rounded up the sum is high by less than
// 153 472 . 2^-24 = 0.92 %: the threshold 2^frac (1 + 2^-6) leaves 1.5 %, so a sum that passes it stands for a true one above
// 2^frac (1 + 0.6 %), which also puts 1 / total far enough below 2^-frac that the float quotient cannot round up to it.  A NaN
// or infinite scale makes the sum NaN, which never compares >= thr: such a hop runs the full path.
// The unread rows' floor.  An unread row is not worth nothing: its clamped code lies in [-maxm, +maxm], so its score is at least
// Xmin = min(sm_scaled(+top), sm_scaled(-top)), and with f = e^(Xmin - Xb), over the S rows the softmax runs over (S clipped to
// max_slots: rows beyond it are no part of the softmax and earn nothing),
//     total >= sum_{r in P} e^(x_r - Xb) + (S - |P|) f.
// The kernel holds a float f_dev <= f, adds the NET term e_r - f_dev per retired row and compares the word with
// thr' = thr - S f_dev: word >= thr' says exactly sum_P e_r + (S - |P|) f_dev >= thr.  f_dev is formed once per hop from the very
// sequence the retire hook uses, raw = exp2(fma(code_min, stop_k1, stop_k0)) at the code of the smaller score (-maxm, or +maxm
// for a negative scale layer: the sign of stop_k1), as raw (1 - 2^-12) where raw >= kFloorMin = 2^-100, else 0.  Two facts carry
// the proof:
//   (a) f_dev <= e^(Xmin - Xb) exactly.  The FMA's argument is off from (Xmin - Xb) log2 e by < 4e-5 (three float roundings and
//       the constant's, on a magnitude of at most 100 + 1), which moves 2^arg by < 3e-5 relative; v_exp_f32 adds 1 ulp (1.2e-7),
//       the derating product 2^-24: together far inside the 2^-12 = 2.4e-4 taken off.
//   (b) f_dev <= every value the retire hook can compute, for any code.  Not because v_exp_f32 were monotone -- nothing here
//       assumes that: a correctly rounded FMA IS monotone in the code (stop_k1, stop_k0 fixed), so every code's argument is >=
//       code_min's, arg_min; the instruction is good to 1 ulp, so every computed e_r >= 2^arg_min (1 - 2^-22) while raw <=
//       2^arg_min (1 + 2^-22), and (1 + 2^-22) (1 - 2^-12) < 1 - 2^-22.  That needs results no 1-ulp bound fails for: with
//       raw >= 2^-100 every e_r is a normal float far above 2^-126.  Where raw is smaller -- a float denormal or 0 is the
//       case, and there a row's own term may flush to 0 -- f_dev = 0: the credit vanishes and the hop is the plain bound's.
// By (b) every net term is >= 0 (a float difference of a >= b is never negative), and an added non-negative float never lowers
// the word: "the sum only grows" below still holds.  It has to: a wavefront that left early has not scored its rows, and a word
// that could sink below thr' again would send the workgroup into the softmax over an incomplete score array.
// The error budget for this sum: each net term carries one more rounding (2^-24 relative to itself, as the term's v_exp_f32
// does), the additions as above at most 153 472 . 2^-24 = 0.92 % -- relative to a word that is now SMALLER than the plain sum --
// and S f_dev and thr - S f_dev round within 2^-23 of thr together, while (a) keeps the credit itself low by 2e-4 of its size:
// a word that passes thr' stands for sum_P e_r + (S - |P|) f above thr (1 - 0.93 %) = 2^frac (1 + 0.6 %), as before.  The
// threshold, its 1.5 % and Xb are unchanged.
// When S f_dev alone reaches thr (thr' <= 0: a scale layer that narrows the score range, or 91 000 rows and more at Q2.5) the
// hop is settled before a row is read: the kernel skips the scan -- no request, no retire, no flush -- and the comparison all
// threads make anyway, word = 0 >= thr', says "zero".  A NaN or infinite scale makes raw NaN, which fails raw >= kFloorMin: f_dev
// = 0, thr' = thr, and the NaN sum runs the full path as before; S = 0 keeps thr' = thr > 0.
// Adding and looking (hops_common.h::scan_rows_stop looks once per unit, behind the unit's retiring).  add(): the lane that
// retires a row adds the row's term to one LDS float (ds_add_f32: nothing returned, nothing waited for; the lanes of one
// instruction that hit the one address are serialised by the LDS, not by the wavefront -- no cross-lane reduction, no VALU
// work).  look(): a plain LDS read of that word, issued BEHIND the unit's adds.  The LDS operations of one wavefront complete
// in order, so what the read returns includes the unit the wavefront has just retired -- the look is fresh -- and every add of
// the other wavefronts that reached the LDS before it; its wait (lgkmcnt alone, no key load is waited for) and the comparison
// follow at once, in front of the next request, and the read's latency is left to the other wavefronts of the SIMD to cover.
// The order in which the lanes' terms arrive is not fixed, so the word's last bits differ from run to run; the decision's
// RESULT does not: whichever way a hop decides, u is what the full scan gives (above).
// The sum only grows, so the other wavefronts follow within a unit of their own, and the workgroup's decision behind the
// scan's barrier -- the same LDS word, read by all -- is "zero" whenever any wavefront left.
struct ScanStop {
    typedef __attribute__((address_space(3))) float lds_float;
    // the unit of the stopping scan: 16-byte loads per lane and request (half of kUnrollDefault: 16 rows at 128-byte rows, 8 at
    // 256, 32 at 64), and units per wavefront -- one being retired, kDepth - 1 in flight
    static constexpr int kUnitLoads = 2;
    static constexpr int kDepth = 3;
    // the unread rows' floor (above): what is taken off the raw value, and the smallest raw value that earns a credit at all
    static constexpr float kFloorDerate = 1.0f - 0x1p-12f;
    static constexpr float kFloorMin = 0x1p-100f;
    float *word;              // the workgroup's sum of net terms (LDS)
    float thr;                // thr' = thr - S f_dev
    // One retired row's e^(x_r - Xb) joins the workgroup's sum: the lane that retires the row adds it (ds_add_f32: nothing
    // returned, nothing waited for).  Written out: as an atomicAdd the compiler wraps it in its loop over the active lanes.
    // The compiler's wait counting cannot see this instruction.  Inside the scan that is harmless: LDS operations complete
    // in order, so more of them in flight only make a counted wait stricter, and nothing there reads the word but look(),
    // whose counted wait for its own read covers the adds in front of it.  INVARIANT: every way from scan_rows to the barrier
    // behind the scan, or to any other read of the word, goes through flush(), which waits for the adds by hand -- the kernel
    // calls it on its one path between the scan and that barrier, whichever way a wavefront left the scan.
    static __device__ __forceinline__ void add(float *word, float v)
    {
        const uint32_t at = (uint32_t)(__UINTPTR_TYPE__)(lds_float *)word;
        asm volatile("ds_add_f32 %0, %1" : : "v"(at), "v"(v) : "memory");
    }
    // behind the scan
    static __device__ __forceinline__ void flush() { asm volatile("s_waitcnt lgkmcnt(0)" : : : "memory"); }
    // the workgroup's sum with this wavefront's last unit in it: leave? (an address-space-3 load: a generic pointer would make
    // it a flat load, which waits for every key load in flight; volatile keeps it behind the retire hook's adds)
    __device__ __forceinline__ bool look() const
    {
        const float seen = *(const volatile lds_float *)(lds_float *)word;
        return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, seen))) >= thr;
    }
};

// W7: every attention format of the launch has word length 7 -- the clamp comes from the signed saturation of the
// multiply and the quotient is a byte gather (hops_common.h::lane_row_sum7): 9 instead of 11 operations per 4 key bytes
// STOP: step 1b of the header (four-wavefront launches only)
// TOP: the attended slots of every hop besides (hops_attended_story.h::story_select_hist, behind finish_hop); never with STOP,
// the selection needs every score
template <int LPR, int kUnroll, bool NT, int MINW, bool W7, bool STOP = false, bool TOP = false>
__global__ void __launch_bounds__(kBlock, MINW)
k_hops_fixed(const HopArgs a, const StoryTop<TOP> tp)
{
    static_assert(!(STOP && TOP), "a hop that ends its scan early has no histogram to select from");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t *hist = (uint32_t *)(smem + kOffHist);
    float *ptab = (float *)(smem + kOffPtab);
    float *u_f = (float *)(smem + kOffU);
    float *o_f = (float *)(smem + kOffO);
    short *ku = (short *)(smem + kOffKu);
    uint8_t *kplut = (uint8_t *)(smem + kOffKp);
    uint32_t *live_row = (uint32_t *)(smem + kOffLiveRow);
    uint8_t *live_kp = (uint8_t *)(smem + kOffLiveKp);
    uint32_t *misc = (uint32_t *)(smem + kOffMisc);
    double *red = (double *)(smem + kOffRed);
    int8_t *sc = (int8_t *)(smem + kOffScores);

    constexpr uint32_t Dp = LPR * 16;
    const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const uint32_t nthreads = blockDim.x, nwaves = nthreads / kWave;      // 256 / 4, or 64 / 1 for short memories
    const uint32_t q = blockIdx.x;
    const uint32_t r0 = a.row_off[q];
    const uint32_t S_in = a.row_off[q + 1] - r0;
    const uint32_t S = S_in < a.max_slots ? S_in : a.max_slots;   // never index LDS past what the launch reserved
    const uint32_t D = a.D;

    for (uint32_t c = tid; c < 256; c += nthreads) u_f[c] = (c < D) ? a.u0[(size_t)q * D + c] : 0.0f;
    __syncthreads();

    for (uint32_t h = 0; h < a.n_hop; h++) {
        const QFmt fa = a.act[h], fm = a.att[h], fb = a.bin;
        const int fv = (int)fb.frac;
        const int maxm = (1 << (fm.iwl + fm.frac)) - 1;

        // query codes Q_bin(u), histogram reset
        for (uint32_t c = tid; c < 256; c += nthreads) {
            ku[c] = (short)((c < D) ? qm_code_or_sign(u_f[c], fb.iwl, fb.frac) : 0);
            for (uint32_t i = 0; i < nwaves; i++) hist[i * 256 + c] = 0u;
        }
        if (tid == 0) misc[0] = 0u;
        // the bound of step 1b: e^(x - Xb) = 2^(code . stop_k1 + stop_k0)
        float *stop_word = (float *)(misc + 1);
        float stop_thr = 0.0f, stop_k1 = 0.0f, stop_k0 = 0.0f, stop_f = 0.0f;
        if constexpr (STOP) {
            const SmCfg smc = sm_cfg(a, h);
            const float top = qm_scale_down((float)maxm, fm.frac), log2e = 1.44269504f;
            const float xb = fmaxf(sm_scaled(top, smc), sm_scaled(-top, smc));
            stop_k1 = sm_scaled(qm_scale_down(1.0f, fm.frac), smc) * log2e;
            stop_k0 = -xb * log2e;
            // the floor f_dev (ScanStop): the retire hook's own sequence at the code of the smallest score (a negative scale
            // layer swaps the ends; a NaN compares false throughout and leaves f_dev = 0), derated, 0 below kFloorMin
            const float raw = __builtin_amdgcn_exp2f(__builtin_fmaf(stop_k1 >= 0.0f ? (float)-maxm : (float)maxm, stop_k1, stop_k0));
            stop_f = raw >= ScanStop::kFloorMin ? raw * ScanStop::kFloorDerate : 0.0f;
            // thr' = thr - S f_dev: the S rows of this query the softmax runs over (S is clipped to max_slots above)
            stop_thr = (float)(1u << fa.frac) * (1.0f + 0.015625f) - (float)S * stop_f;
            if (tid == 0) stop_word[0] = 0.0f;
        }
        __syncthreads();

        // (STOP, thr' <= 0: the floor alone settles the hop -- no request, no retire, no flush; the word stays 0 >= thr')
        if (S > 0 && !(STOP && stop_thr <= 0.0f)) {
            // lane constants: |u| pre-shifted so that saturation == the per-product clamp
            ScanConst c;
            uint32_t sh = 0;
            if (W7) make_scan_const7(c, ku, (lane % LPR) * 16, fv, hop_relu(a, h), fb.iwl + fb.frac == 0);
            else sh = make_scan_const(c, ku, (lane % LPR) * 16, fm.iwl + fm.frac, fv, hop_relu(a, h), fb.iwl + fb.frac == 0);
            const uint8_t *kb = (const uint8_t *)a.keys + (size_t)h * a.hop_stride + (size_t)r0 * Dp;
            uint32_t *hw = hist + wave * 256;
            auto row_sum = [&](const i32x4 x) { return W7 ? lane_row_sum7(x, c) : lane_row_sum(x, c, sh); };
            auto retire = [&](uint32_t r, int v) {          // Qm of the row sum (lib/layer_cuda.cu:135)
                const int code = v > maxm ? maxm : (v < -maxm ? -maxm : v);
                sc[r] = (int8_t)code;
                atomicAdd(&hw[code + 127], 1u);
                if constexpr (STOP) ScanStop::add(stop_word, __builtin_amdgcn_exp2f(__builtin_fmaf((float)code, stop_k1, stop_k0)) - stop_f);   // the net term, >= 0
            };
            if (S < (kWave / LPR) * kUnroll) scan_rows_short<LPR>(kb, S, row_sum, retire, lane, wave, nwaves);
            else if (STOP || nwaves == kWaves) {        // (a stopping launch always has four wavefronts)
                if constexpr (STOP) scan_rows<LPR, kUnroll, NT, kWaves>(kb, S, row_sum, retire, lane, wave, ScanStop{stop_word, stop_thr});
                else scan_rows<LPR, kUnroll, NT, kWaves>(kb, S, row_sum, retire, lane, wave);
            }
            else scan_rows<LPR, kUnroll, NT, 1>(kb, S, row_sum, retire, lane, wave);
            // the wait for every add (ScanStop's invariant): the decision below is taken on the whole sum
            if constexpr (STOP) ScanStop::flush();
        }
        __syncthreads();
        // every weight code of this hop is 0 (ScanStop above): no softmax, no survivors, o = 0.  All threads read the one word.
        bool all_zero = false;
        if constexpr (STOP) all_zero = stop_word[0] >= stop_thr;

        // softmax over slots from the histogram of score codes (bin d <-> code d - 127)
        uint32_t n_live = 0;
        if (S > 0 && !all_zero) {
            // each thread owns bins tid, tid + nthreads, ... (4 bins per thread in a one-wavefront group)
            const SmCfg smc = sm_cfg(a, h);
            auto bin_x = [&](uint32_t d) { return sm_scaled(qm_scale_down((float)((int)d - 127), fm.frac), smc); };
            float xmax = -INFINITY;
            for (uint32_t d = tid; d < 256; d += nthreads) {
                uint32_t cnt = 0;
                for (uint32_t i = 0; i < nwaves; i++) cnt += hist[i * 256 + d];
                hist[d] = cnt;                                  // bins are thread-private from here on
                if (cnt) xmax = fmaxf(xmax, bin_x(d));
            }
            xmax = block_max<float>(xmax, (float *)red, lane, wave);
            double part = 0.0;
            for (uint32_t d = tid; d < 256; d += nthreads) {
                const float e = sm_exp(bin_x(d) - xmax, smc);  // score - max: exact on the score grid
                ptab[d] = e;
                if (hist[d]) part += (double)hist[d] * (double)e;
            }
            // e^x base: the CUDA kernel's double total; the CPU bases: the CPU softmax's float total, slot by slot (hops_common.h)
            const double total = smc.base == QMANN_SOFTMAX_EXP ? block_sum_double(part, red, lane, wave)
                                                               : block_serial_total_f32(S, lane, wave, red, [&](uint32_t r) { return ptab[(int)sc[r] + 127]; });
            for (uint32_t d = tid; d < 256; d += nthreads) {
                const float p = hist[d] ? sm_quot(ptab[d], total, smc) : 0.0f;
                ptab[d] = p;
                kplut[d] = (uint8_t)qm_code(p, fa.iwl, fa.frac);
            }
            __syncthreads();

            if (a.tap_codes || a.tap_scores || a.tap_probs) {
                const size_t tb = (size_t)h * a.rows_total + r0;
                for (uint32_t r = tid; r < S; r += nthreads) {
                    const int code = sc[r];
                    if (a.tap_codes) a.tap_codes[tb + r] = code;
                    if (a.tap_scores) a.tap_scores[tb + r] = qm_scale_down((float)code, fm.frac);
                    if (a.tap_probs) a.tap_probs[tb + r] = ptab[code + 127];
                }
            }
            // rows whose quantised weight is non-zero: 16 score bytes per LDS read and their 16 table look-ups in flight
            // together (one score -> look-up -> branch chain per row left every row two LDS latencies long)
            for (uint32_t rb = tid * 16; rb < S; rb += nthreads * 16) {
                const i32x4 v = *(const i32x4 *)(sc + rb);           // (the score array is padded to 16 rows)
                uint8_t kp[16];
#pragma unroll
                for (int i = 0; i < 16; i++) kp[i] = kplut[(int)(int8_t)((uint32_t)v[i / 4] >> (8 * (i % 4))) + 127];
#pragma unroll
                for (int i = 0; i < 16; i++) {
                    if (rb + i < S && kp[i]) {
                        const uint32_t n = atomicAdd(&misc[0], 1u);
                        if (n < (uint32_t)kLiveCap) { live_row[n] = rb + i; live_kp[n] = kp[i]; }
                    }
                }
            }
            __syncthreads();
            n_live = misc[0];
        }

        // weighted read-out over the surviving rows, linear map, hop update (hops_common.h)
        auto kp_of_row = [&](uint32_t r) { return (int)kplut[(int)sc[r] + 127]; };
        finish_hop<Dp>(a, q, h, r0, S, n_live, live_row, live_kp, kp_of_row, ku, u_f, o_f, tid);
        if constexpr (TOP) story_select_hist(tp, (size_t)q * a.n_hop + h, S, hist, ptab, sc, live_row, live_kp, misc, red, tid, lane, wave);
    }
    for (uint32_t c = tid; c < D; c += nthreads) a.u_out[(size_t)q * D + c] = relu_if(u_f[c], a.en_non_lin != 0);
}

__global__ void k_quantize_i8(const float *__restrict__ src, int8_t *__restrict__ dst, size_t rows, uint32_t cols,
                              uint32_t pitch, QFmt f, int signmag)
{
    const size_t n = rows * pitch;
    const size_t stride = (size_t)gridDim.x * blockDim.x;          // grid-stride: n may exceed 2^32
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const size_t r = i / pitch;
        const uint32_t c = (uint32_t)(i % pitch);
        int k = 0;
        uint32_t neg = 0;
        if (c < cols) {
            const float x = src[r * cols + c];
            k = qm_code(x, f.iwl, f.frac);
            neg = !(x >= 0.0f);                  // the reference keys the sign on the float (lib/common.h:210)
        }
        if (signmag) dst[i] = (int8_t)((uint32_t)(k < 0 ? -k : k) | (neg ? 0x80u : 0u));
        else dst[i] = (int8_t)k;
    }
}

// qmann_check_slots: how many stories exceed the caller's bound (and would be cut by the hop kernels)
__global__ void k_check_slots(const uint32_t *__restrict__ row_off, uint32_t n_query, uint32_t max_slots, uint32_t *n_over)
{
    uint32_t mine = 0;
    for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < n_query; q += (size_t)gridDim.x * blockDim.x)
        mine += (row_off[q + 1] - row_off[q] > max_slots) ? 1u : 0u;
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
    if ((threadIdx.x & 63u) == 0 && mine) atomicAdd(n_over, mine);
}

}  // namespace

// rt.h: the plan of the qm_hops_i8 call that the host model is about to make (int8 keys: a key row is Dp bytes; no taps), asked
// of hops_host.h::hop_plan itself -- with the checks that would end that call before its launch
bool qm_hops_will_split(const qmann_net *net, size_t plane_rows, uint32_t max_slots, uint32_t n_query)
{
    const bool fixed = net->attention_mode == QMANN_ATT_FIXED;
    if (!fixed && net->attention_mode != QMANN_ATT_APPX && net->attention_mode != QMANN_ATT_HAMMING_V0 && net->attention_mode != QMANN_ATT_HAMMING_V1)
        return false;                                       // (float attention has its own kernels: batch_hops_float.hip)
    HopArgs a;
    if (n_query == 0 || qm_too_many_queries(n_query) || fill_hop_formats(a, net)) return false;
    a.rows_total = (uint32_t)plane_rows;
    return hop_plan(a, fixed ? (int)kModeFixed : (int)kModeAppx, net->dim_emb_pad, max_slots, n_query).form == HopForm::Split;   // (the byte forms of the Hamming family plan alike)
}

uint32_t *qm_split_early(const uint32_t *row_off, uint32_t n_query, uint32_t max_slots, hipStream_t owner, hipStream_t run_on)
{
    return split_lists(row_off, n_query, max_slots, owner, run_on);
}

extern "C" {

int qmann_check_slots(const uint32_t *row_off, uint32_t n_query, uint32_t max_slots, uint32_t *n_over, void *stream)
{
    QmBatched qm_scope;
    if (!row_off || !n_over) return QMANN_EINVAL;
    if (n_query == 0) return QMANN_OK;
    const uint32_t blocks = (n_query + 255u) / 256u;
    k_check_slots<<<blocks < 1024u ? blocks : 1024u, 256, 0, (hipStream_t)stream>>>(row_off, n_query, max_slots, n_over);
    QM_LAUNCH_CHECK();
    return qm_scope.rc();
}

size_t qmann_hops_lds_bytes(uint32_t max_slots)
{
    return (size_t)kOffScores + (((size_t)max_slots + 15) & ~(size_t)15);
}

int qmann_quantize_i8(const float *src, int8_t *dst, size_t rows, uint32_t cols, uint32_t pitch, qmann_fmt fmt,
                      int layout, void *stream)
{
    QmBatched qm_scope;
    if (!src || !dst || pitch < cols) return QMANN_EINVAL;
    if (!qm_fmt8(fmt)) return QMANN_ERANGE;
    if (layout != QMANN_CODE_TWOS && layout != QMANN_CODE_SIGNMAG) return QMANN_EINVAL;
    const size_t n = rows * pitch;
    if (n == 0) return QMANN_OK;
    const size_t blocks = (n + 255) / 256;
    k_quantize_i8<<<(unsigned)(blocks < 262144 ? blocks : 262144), 256, 0, (hipStream_t)stream>>>(src, dst, rows, cols, pitch,
                                                                              qm_qfmt(fmt), layout);
    QM_LAUNCH_CHECK();
    return qm_scope.rc();
}

}  // extern "C"

int qm_hops_i8(const qmann_net *net, const int8_t *keys, const int8_t *vals, size_t hop_stride, const uint32_t *row_off, uint32_t max_slots,
               const float *u0, float *u_out, const qmann_taps *taps, uint32_t n_query, void *stream, const QmHopHints &hints)
{
    QmBatched qm_scope;
    if (const int rc = check_hop_call(net, keys, vals, row_off, u0, u_out)) return rc;
    if (taps && hop_stride == 0) return QMANN_EINVAL;       // taps are indexed [hop][row]: they need distinct hop planes
    if (net->attention_mode == QMANN_ATT_APPX)
        return qmann_hops_appx_impl(net, keys, vals, hop_stride, row_off, max_slots, u0, u_out, taps, n_query, stream, hints);
    if (net->attention_mode == QMANN_ATT_HAMMING_V0 || net->attention_mode == QMANN_ATT_HAMMING_V1)
        return qmann_hops_hambytes_impl(net, keys, vals, hop_stride, row_off, max_slots, u0, u_out, taps, n_query, stream, hints);
    if (net->attention_mode != QMANN_ATT_FIXED && net->attention_mode != QMANN_ATT_FLOAT) return QMANN_EUNSUPPORTED;
    HopArgs a;
    if (const int rc = fill_hop_args(a, net, keys, vals, hop_stride, hop_stride, row_off, u0, u_out, taps, hints.plane_rows)) return rc;
    a.max_slots = max_slots;
    const size_t lds = qmann_hops_lds_bytes(max_slots);
    if (lds > kHopLdsLimit) return QMANN_ERANGE;
    if (n_query == 0) return QMANN_OK;
    if (qm_too_many_queries(n_query)) return QMANN_ERANGE;

    if (net->attention_mode == QMANN_ATT_FLOAT) {
        if (hints.top_float) return qmann_hops_top_float_impl(a, net->dim_emb_pad, max_slots, hints.top_k, hints.top_slot, hints.top_p, n_query, stream);
        // (attended slots through qmann_hops_top_i8: float attention is not served -- behind the one refusal the float launcher
        // has of its own; qmann_hops_top_float_i8 is the call that serves it)
        if (hints.top_on) return float_story_lds_bytes(max_slots) > kHopLdsLimit ? QMANN_ERANGE : QMANN_EUNSUPPORTED;
        return qmann_hops_float_impl(a, net->dim_emb_pad, max_slots, n_query, stream);
    }
    if (hints.top_float) return QMANN_EUNSUPPORTED;       // (qmann_hops_top_float_i8: float attention only)
    if (hints.top_on && !story_top_args_ok(hints.top_k, hints.top_slot, hints.top_p)) return QMANN_EINVAL;     // behind every refusal of the base call

    hipStream_t st = (hipStream_t)stream;
    const bool w7 = !qm_tuning().no_w7 && all_w7(a, kW7Att);
    qm_dispatch<4, 8, 16>(net->dim_emb_pad / 16, [&](auto lpr) {
        constexpr int LPR = decltype(lpr)::value;
        launch_hops<kModeFixed, 8, LPR, LPR>(a, max_slots, n_query, st, hints, [&](HopForm form) {
            if (form == HopForm::Mid) { launch_mid(a, max_slots, n_query, st); return; }      // hops_mid.h: 65 .. 1 024 slots at bAbI width
            // memories of 65..256 slots run one wavefront per query with the histogram softmax: four times
            // as many queries resident per CU and no cross-wavefront barriers
            const dim3 block(max_slots <= 256 ? kWave : kBlock);
            if (hints.top_on) {                             // (the plain kernel's block at every length: p is the tap's, bit for bit)
                const StoryTop<true> tp{hints.top_slot, hints.top_p, hints.top_k};
                qm_dispatch<false, true>(w7, [&](auto w) { qm_launch(k_hops_fixed<LPR, kUnrollDefault, true, 1, decltype(w)::value, false, true>, n_query, block, lds, st, a, tp); });
                return;
            }
            // (bounding the kernel to 96 VGPRs for a fifth wavefront per SIMD measured 1-3 % slower: MINW stays 1)
            // (step 1b of the header: only where some hop's bound lies within the memory; every other launch keeps its kernel)
            if (block.x == (unsigned)kBlock && !qm_tuning().no_scan_stop && scan_stop_gate(a, max_slots))
                qm_dispatch<false, true>(w7, [&](auto w) { qm_launch(k_hops_fixed<LPR, kUnrollDefault, true, 1, decltype(w)::value, true>, n_query, block, lds, st, a, StoryTop<false>{}); });
            else
                qm_dispatch<false, true>(w7, [&](auto w) { qm_launch(k_hops_fixed<LPR, kUnrollDefault, true, 1, decltype(w)::value>, n_query, block, lds, st, a, StoryTop<false>{}); });
        });
    });
    QM_LAUNCH_CHECK();
    return qm_scope.rc();
}

extern "C" int qmann_hops_i8(const qmann_net *net, const int8_t *keys, const int8_t *vals, size_t hop_stride, const uint32_t *row_off,
                             uint32_t max_slots, const float *u0, float *u_out, const qmann_taps *taps, uint32_t n_query, void *stream)
{
    return qm_hops_i8(net, keys, vals, hop_stride, row_off, max_slots, u0, u_out, taps, n_query, stream, QmHopHints{});
}

// qmann_hops_i8 without taps plus the attended slots of every hop: one kernel on `stream` (hops_attended_story.h)
extern "C" int qmann_hops_top_i8(const qmann_net *net, const int8_t *keys, const int8_t *vals, size_t hop_stride, const uint32_t *row_off,
                                 uint32_t max_slots, const float *u0, float *u_out, uint32_t k, uint32_t *top_slot, float *top_p,
                                 uint32_t n_query, void *stream)
{
    QmHopHints hints;
    hints.top_on = true; hints.top_k = k; hints.top_slot = top_slot; hints.top_p = top_p;
    return qm_hops_i8(net, keys, vals, hop_stride, row_off, max_slots, u0, u_out, nullptr, n_query, stream, hints);
}

// qmann_hops_i8 (float attention) without taps plus the attended slots of every hop: one kernel on `stream`
// (batch_hops_top_float.hip, hops_attended_float.h)
extern "C" int qmann_hops_top_float_i8(const qmann_net *net, const int8_t *keys, const int8_t *vals, size_t hop_stride, const uint32_t *row_off,
                                       uint32_t max_slots, const float *u0, float *u_out, uint32_t k, uint32_t *top_slot, float *top_p,
                                       uint32_t n_query, void *stream)
{
    QmHopHints hints;
    hints.top_on = hints.top_float = true; hints.top_k = k; hints.top_slot = top_slot; hints.top_p = top_p;
    return qm_hops_i8(net, keys, vals, hop_stride, row_off, max_slots, u0, u_out, nullptr, n_query, stream, hints);
}
