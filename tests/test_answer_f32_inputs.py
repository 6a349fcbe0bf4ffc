"""CPU precondition of test_gpu_answer_f32.py: the seeded inputs of answer_f32_cases.py do what each case is for (O1, M1, M2, the
planted ties and labels, the excuse cap), the kernel tables restate the launcher, and the numpy references agree with the oracle
(itself pinned to the reference's C code).  No GPU, no library call: a seed that trips a check here is replaced in
answer_f32_cases.SEEDS; the checks stay."""
import numpy as np
import pytest

import answer_f32_cases as cs
from answer_f32_cases import CASES, OUTSIDE, SWEEP, case

EXCUSE_CAP = 0.10


def test_kernel_tables_restate_the_launcher():
    """the fits edges of ans_small_plan (78 KiB of LDS), one serial kernel per `order` shape, the T class of every fused sweep, one
    trip of every persistent loop on 256 compute units"""
    assert [cs.fits_edge(V) for V in (32, 64, 96, 128, 129, 256)] == [124, 104, 89, 104, 62, 62]
    assert [cs.serial_kernel(60, V) for V in (30, 64, 96, 128, 200, 300)] == [
        "k_answer_small<16,2,2>", "k_answer_small<16,4,2>", "k_answer_small<16,6,2>", "k_answer_small<16,8,1>", "k_answer_small<64,4,4>",
        "k_answer<false>"]
    assert cs.serial_kernel(17, 70) == "k_answer_small<16,6,2>" and cs.serial_kernel(64, 200) == "k_answer<false>"
    assert cs.serial_kernel(62, 200) == "k_answer_small<64,4,4>" and cs.serial_kernel(63, 129) == "k_answer<false>"
    for name, (call, V, _) in SWEEP.items():
        assert cs.sweep_queries(call, cs.SWEEP_D, V, 256) == cs.SWEEP_256[name], name
        assert cs.sweep_b(name, 256) == cs.SWEEP_256[name] + 37 <= cs.MAX_SWEEP_B
        assert cs.sweep_b(name, 1 << 20) == (cs.MAX_SWEEP_B if V <= 256 else 8229)      # (k_answer's grid is capped at 8 192 anywhere)
    assert {cs.fused_tiles(V) for V in cs.FUSED_T_OF_SWEEP} == {2, 3, 4, 5, 8, 12, 15, 16}
    assert all(cs.fused_tiles(V) == T for V, T in cs.FUSED_T_OF_SWEEP.items())
    assert sorted(cs.serial_kernel(cs.SWEEP_D, V) for c, V, _ in SWEEP.values() if c == "serial") == sorted(
        cs.serial_kernel(60, V) for V in (30, 64, 96, 128, 200, 300))
    # dictionaries sit on both sides of every T class and every vpt class
    Vs = sorted(c["V"] for c in CASES.values() if c["family"] == "dictionaries")
    for lo in (16, 32, 48, 64, 80, 96, 128, 192, 240, 256):
        assert lo in Vs and lo + 1 in Vs
    # the serial widths sit on both sides of every fits edge
    for V in (32, 64, 96, 128, 256):
        e = cs.fits_edge(V)
        assert cs.small_plan(e, V).fits and not cs.small_plan(e + 1, V).fits
        assert f"width_serial_V{V}_D{e}" in CASES and f"width_serial_V{V}_D{e + 1}" in CASES


def references(oracle, c):
    """(call, base, probabilities) of every reference the GPU tests hold the case against"""
    out = []
    for base in c.bases:
        if "fused" in c.calls and cs.takes_fused(c.D, c.V, base):
            out.append(("fused", base, cs.probs_r64(c, base)))
        out.append(("serial", base, cs.probs_rser(oracle, c, base)))
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_inputs_do_what_the_case_is_for(oracle, name):
    c = case(name)
    assert c.W.shape == (c.V, c.D) and c.u.shape == (c.B, c.D) and c.W.dtype == c.u.dtype == np.float32
    # u lies on an 8-bit grid: every component is exactly a bf16 (the fused form's premise)
    assert not (c.u.view(np.uint32) & 0xFFFF).any()
    codes = c.u.astype(np.float64) * (np.exp2(c.frac)[:, None] if c.family == "magnitudes" else 4.0)
    assert np.array_equal(codes, np.rint(codes)) and np.abs(codes).max() <= 127
    if "fused" in c.calls:
        assert c.max_abs_logit <= 16.0                                       # the header's relative bound applies to the whole case
    # the excuse cap, from the references alone; a lone query is never excused
    for call, base, p in references(oracle, c):
        decided, pred = cs.decide(c, p)
        assert (~decided).mean() <= EXCUSE_CAP, f"{call} base {base}: {(~decided).sum()} of {c.B} queries excused"
        assert c.B > 1 or decided.all()
        assert (pred[c.zero_rows] == c.V - 1).all()
    # labels: inside and outside the dictionary, matches among the former
    if c.B >= 11:
        assert (c.labels == c.V + 3).any() and (c.labels == OUTSIDE).any() and c.inside.any()
        _, pred = cs.decide(c, cs.probs_rser(oracle, c, 0))
        assert (pred[c.inside] == c.labels[c.inside]).any()
    if c.B == 1:
        assert c.inside.all()
    if c.family not in ("ties_labels",):
        assert not c.pairs and (c.D < 4 or not c.zero_rows.any())           # (a lone component is zero now and then)


@pytest.mark.parametrize("name", sorted(n for n, c in CASES.items() if c["family"] == "order"))
def test_order_cases_are_the_rounding_history(name):
    """O1: reversed columns, one rounding per multiply-add, even columns then odd and the float64 sum each move a probability of
    EVERY query by at least 1e-3 relative (a hundred times the tolerance), with every logit within +-8; the partial sums swing
    beyond 2^15 while the exact logits stay within +-4"""
    c = case(name)
    assert np.abs(c.Lser).max() <= 8.0 and np.abs(c.L64).max() <= 4.0
    assert np.abs(c.u[:, 0, None] * c.W[None, :, 0]).max() > 2.0 ** 15
    if c.D % 2:
        assert not c.u[:, -1].any() and c.W[:, -1].any()
    p = cs.softmax64(c.Lser, 0)
    for kind in cs.ORDER_VARIANTS:
        pv = cs.softmax64(cs.variant_logits(c.W, c.u, kind), 0)
        moved = (np.abs(pv - p) / p).max(1)
        print(f"{name} {kind}: a probability of every query moves by at least {moved.min():.2e} relative; logits within {np.abs(c.Lser).max():.2f}")
        assert moved.min() >= 1e-3, kind


@pytest.mark.parametrize("name", sorted(n for n, c in CASES.items() if c["family"] == "ties_labels"))
def test_ties_and_labels_are_planted(oracle, name):
    c = case(name)
    V = c.V
    assert c.pairs == cs.TIE_PAIRS + ((0, V - 1),)
    assert [(b - a) for a, b in cs.TIE_PAIRS] == [1, 4, 16, 64] and cs.TIE_PAIRS[0][0] // 4 == cs.TIE_PAIRS[0][1] // 4
    for a, b in c.pairs:
        assert np.array_equal(c.W[a], c.W[b]) and np.array_equal(c.Lser[:, a], c.Lser[:, b]) and np.array_equal(c.L64[:, a], c.L64[:, b])
    for call, base, p in references(oracle, c):
        decided, pred = cs.decide(c, p)
        for i, (a, b) in enumerate(c.pairs):                                  # each pair wins its query: the higher index, by a clear margin
            assert pred[i] == b and decided[i], (call, base, i)
            assert p[i, a] == p[i, b] == p[i].max()
    zero = np.arange(c.B) % 11 == 5
    assert np.array_equal(zero, c.zero_rows) and not c.Lser[zero].any()
    assert np.array_equal(c.labels[:V], np.arange(V))                         # every (tile, lane group, register) position holds the label once
    late = c.labels[V:]
    assert (late == V + 3).any() and (late == OUTSIDE).any() and (late < V).any()


def test_magnitudes_need_all_three_images():
    """the contents of W; M1: W cut to its first two bf16 images moves a probability by at least 1e-4 relative in three quarters of
    the queries (e^x; 2^x moves them by ln 2 of that), and at either base a tenth of ALL probabilities by more than the GPU
    test's rtol 1e-5 / atol 1e-7; M2: the serial loop and a float32 pairwise sum both stay within 3e-6 relative of the float64
    softmax, so the tolerance of 1e-5 leaves correct float arithmetic room.
    Measured (seed as committed): M1 in 0.92 of the queries at e^x (0.19 at 2^x), 1 029 / 909 of 4 480 probabilities beyond
    the tolerance; M2 serial 2.3e-6 / 1.6e-6, pairwise 8.1e-7 / 5.5e-7."""
    c = case("magnitudes")
    bits = c.W.view(np.uint32)
    expo = ((bits >> 23) & 0xFF).astype(int)
    normal = (expo > 0) & (c.W != 0)
    assert expo[normal].max() - expo[normal].min() >= 24                      # a wide exponent range
    assert ((bits & 0xFF) != 0)[normal].mean() > 0.7                          # entries that need all 24 bits
    assert not (bits[0:10, 0:20] & 0xFFFF).any() and not (bits[10:20, 20:40] & 0xFF).any() and (bits[10:20, 20:40] & 0xFF00).any()
    assert (bits[20:24, 40:44] == 0x80000000).all()                          # -0.0
    den = bits[24:28, 44:48]
    assert (((den >> 23) & 0xFF) == 0).all() and (den & 0x7FFFFF).all() and (den >> 31).any()
    assert set(c.frac) == set(range(8))
    codes = np.rint(c.u.astype(np.float64) * np.exp2(c.frac)[:, None]).astype(int)
    for f in range(8):
        k = codes[c.frac == f]
        assert all((k == x).any() for x in (127, -127, 1, -1)), f
    assert 4.0 < c.max_abs_logit <= 16.0
    for base in (0, 1):
        p = cs.probs_r64(c, base)
        p2 = cs.softmax64(cs.logits64(cs.two_images(c.W), c.u), base)
        moved = (np.abs(p2 - p) / p).max(1)
        beyond = int((np.abs(p2 - p) > 1e-5 * p + 1e-7).sum())
        print(f"base {base}: M1 holds in {(moved >= 1e-4).mean():.2f} of the queries (median {np.median(moved):.2e}); {beyond} of {p.size} beyond the tolerance")
        assert base == 1 or (moved >= 1e-4).mean() >= 0.75
        assert beyond >= p.size // 10
        for what, L in (("serial", c.Lser), ("pairwise", cs.pairwise_logits(c.W, c.u))):
            err = (np.abs(cs.softmax64(L, base) - p) / p).max()
            print(f"base {base}: M2 {what} {err:.2e}")
            assert err <= 3e-6, what


@pytest.mark.parametrize("name", sorted(CASES))
def test_rser_is_the_oracle_loop(oracle, name):
    """Rser bit-equal to oracle.dense_fwd on every query of every case of at most 128 queries (8 queries of the larger ones), the
    oracle's arg-max rule on its own softmax is the reference's pred, and the float64 softmax is within rtol 1e-5 / atol 1e-7 of
    the oracle's e^x softmax"""
    c = case(name)
    qs = range(c.B) if c.B <= 128 else sorted({0, 1, 5, 16, c.B // 2, c.B - 17, c.B - 2, c.B - 1})
    p = cs.probs_rser(oracle, c, 0)
    for q in qs:
        lo = oracle.dense_fwd(c.W, c.u[q], False, (0, 0), (0, 0))
        assert np.array_equal(lo.view(np.uint32), c.Lser[q].view(np.uint32)), f"query {q}"
        po = oracle.softmax_fwd(lo, variant=0)
        np.testing.assert_allclose(po, p[q], rtol=1e-5, atol=1e-7, err_msg=f"query {q}")
        assert oracle.argmax_hi(po) == cs.highest_argmax(po[None])[0]


@pytest.mark.parametrize("name", sorted(SWEEP) + [f"sweep_ranked_V{V}" for V in cs.SWEEP_RANKED])
def test_second_sweep_cases(oracle, name):
    """on 256 compute units: 37 queries beyond one trip, labels in the first 64 queries and in the second trip (the same lanes),
    matches among both, the excuse cap, and Rser of the sampled queries is the oracle's loop"""
    c = cs.sweep_case(name, 256)
    one = c.one_sweep
    assert c.B == one + 37 and c.max_abs_logit <= 16.0
    assert c.inside[:64].any() and c.inside[one:].any() and not c.inside[64:one].any()
    for base in (0, 1):
        assert (~c.decided[base]).mean() <= EXCUSE_CAP
        hit = c.inside & (c.pred64[base] == c.labels)
        assert hit[:64].any() and hit[one:].any()
    assert len(c.sample) == 384 and len(set(c.sample)) == 384 and (c.sample[-128:] == np.arange(c.B - 128, c.B)).all()
    for i in (0, 100, 255, 256, 383):
        lo = oracle.dense_fwd(c.W, c.u[c.sample[i]], False, (0, 0), (0, 0))
        assert np.array_equal(lo.view(np.uint32), c.Lser[i].view(np.uint32))
