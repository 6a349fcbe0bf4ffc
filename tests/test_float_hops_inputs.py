"""CPU preconditions of test_gpu_float_hops.py (float_hops_cases.py, float_hop_ref.py), in the pattern of test_embed_inputs.py.
Nothing here needs a GPU or the library: numpy and the oracle alone.

1. Every case meets the generator's two conditions -- spread attention (among the (query, hop) pairs with S >= 8 at least three
   quarters have 1 / sum p^2 >= 4, every hop index has one) and at most 1 % of the columns `near` a truncation step -- computed
   from float_hop_ref alone and chained through its own u_next.
2. Each stated edge is present: the tile-edge slot counts with an empty story between two others and rows in front of
   row_off[0]; 0x80 bytes on rows that carry weight, the whole rows, the words; the tie at the top; the equal scores; format
   draws that cover frac 0 and activations finer and coarser than the weights; the cut on both sides of the tile.
3. float_hop_ref against the oracle (Oracle.forward_mem, attention_mode 1, bytes decoded to floats; the 0x80 cases left out: the
   oracle takes floats): scores bit-equal, p within rtol 1e-5, lu bit-equal, u bit-equal on every column outside `near`.
4. The comparison routine of the GPU test, run on stand-in outputs: a correct read-out passes, and a value row added twice, a
   0x80 byte read as -128, one differing state code outside `near` and a touched guard byte are each reported.
"""
import numpy as np
import pytest

import float_hop_ref as ref
import float_hops_cases as fc
from float_hops_cases import CASES, FAMILIES, build, reference_chain


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_meets_the_spread_and_near_conditions(name):
    case = build(name)
    share, per_hop, near = fc.conditions(case, reference_chain(name))
    print(f"{name}: 1/sum p^2 >= 4 in {100 * share:.1f} % of the (query, hop) pairs with S >= 8; near share {100 * near:.3f} %")
    assert case.B <= 16
    assert near <= fc.NEAR_SHARE, f"{name}: {100 * near:.2f} % of the columns are near a step"
    if case.exempt_spread:                       # +-127 everywhere: one-hot by construction, and it says so
        assert name == "extreme_127"
        return
    assert share >= fc.SPREAD_SHARE, f"{name}: spread in {share:.2f} of the pairs"
    assert all(per_hop), f"{name}: a hop index without one spread query {per_hop}"


def test_shares_per_family():
    """the two shares per case family, as the summary of this work states them"""
    for fam, names in FAMILIES.items():
        ok, n, near, cols = 0, 0, 0, 0
        for name in names:
            case, ch = build(name), reference_chain(name)
            for q in range(case.B):
                S = case.slots(q)[1]
                for hp in ch[q]:
                    if S >= fc.SPREAD_MIN_SLOTS:
                        ok += ref.n_eff(hp.p) >= fc.SPREAD_NEFF; n += 1
                    if S > 0:
                        near += int(hp.near.sum()); cols += hp.near.size
        print(f"family {fam}: spread share {100 * ok / max(n, 1):.1f} % of {n} pairs, near share {100 * near / cols:.3f} % of {cols} columns")
        assert near <= fc.NEAR_SHARE * cols


# ---- 2. the edges ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FAMILIES["tile_edges"])
def test_tile_edge_cases_hold_every_stated_slot_count(name):
    case = build(name)
    Dp = case.kb.shape[2]
    T = {64: 64, 128: 32, 256: 16}[Dp]
    assert fc.tile_rows(Dp) == T
    n = np.diff(case.row_off.astype(np.int64))
    assert set(n) >= {1, T - 1, T, T + 1, 2 * T - 1, 4 * T, 4 * T + 1, 5 * T - 1, 8 * T, 8 * T + 1, 9 * T - 1, 12 * T + 1}
    z = int(np.nonzero(n == 0)[0][0])
    assert 0 < z < len(n) - 1 and n[z - 1] > 0 and n[z + 1] > 0, "the empty story sits between two others"
    assert case.row_off[0] > 0 and case.kb[:, :case.row_off[0]].all(), "rows in front of row_off[0], none of them zero"
    assert case.max_slots == 12 * T + 1 == int(n.max())
    q1 = int(np.nonzero(n == 1)[0][0])          # the one-slot story's value row is off the activation grid
    assert (ref.decode(case.vb[:, case.row_off[q1], :case.cfg["dim_emb"]]) % 2 == 1).all()


def test_widths_and_pad_columns():
    assert sorted(build(n).cfg["dim_emb"] for n in FAMILIES["widths"]) == [1, 17, 60, 64, 100, 128, 200, 255, 256]
    for name in CASES:
        case = build(name)
        D, Dp = case.cfg["dim_emb"], case.kb.shape[2]
        assert Dp == fc.pad_dim(D)
        r0 = int(case.row_off[0])
        assert not case.kb[:, r0:, D:].any() and not case.vb[:, r0:, D:].any(), f"{name}: pad columns must be zero"
        assert case.kb[:, :, :D].any() and case.vb[:, :, :D].any()


def weighted_minus_zero(case, ch, plane):
    """0x80 bytes of `plane` on rows whose weight is at least 1 / (4 S)"""
    D, n = case.cfg["dim_emb"], 0
    for q in range(case.B):
        r0, S, _ = case.slots(q)
        for h, hp in enumerate(ch[q]):
            rows = np.nonzero(hp.p >= 0.25 / max(S, 1))[0]
            n += int((plane[case.plane(h), r0 + rows, :D] == 0x80).sum())
    return n


@pytest.mark.parametrize("name", FAMILIES["minus_zero"])
def test_minus_zero_bytes_sit_on_weighted_rows(name):
    case, ch = build(name), reference_chain(name)
    D = case.cfg["dim_emb"]
    for plane in (case.kb, case.vb):
        assert weighted_minus_zero(case, ch, plane) >= 100
    if name == "mz_sprinkled":
        for plane in (case.kb, case.vb):
            share = float((plane[:, :, :D] == 0x80).mean())
            assert 0.10 < share < 0.15, "about one byte in eight"
    if name == "mz_whole_rows":
        rows_k, rows_v = case.marks["whole_rows"]
        assert len(rows_k) == case.B and (case.kb[:, rows_k, :D] == 0x80).all() and (case.vb[:, rows_v, :D] == 0x80).all()
        for q in range(case.B):                  # a whole 0x80 key row scores 0; the whole 0x80 value row carries weight
            r0 = case.slots(q)[0]
            for hp in ch[q]:
                assert hp.codes[rows_k[q] - r0] == 0 and hp.p[rows_v[q] - r0] > 0
    if name == "mz_words":
        for plane in (case.kb, case.vb):
            w = plane[:, :, :D].reshape(-1, 4)
            all80 = np.nonzero((w == 0x80).all(axis=1))[0]
            all80 = all80[(all80 > 0) & (all80 < len(w) - 1)]
            assert ((w[all80 - 1] == 0x7F).all(axis=1) & (w[all80 + 1] == 0xFF).all(axis=1)).any(), "0x80 word between +127 and -127 words"
            mixed = (w == 0x80).any(axis=1) & (w == 0x7F).any(axis=1) & (w == 0xFF).any(axis=1)
            assert mixed.sum() >= 100


def test_extremes():
    case, ch = build("extreme_127"), reference_chain("extreme_127")
    D = case.cfg["dim_emb"]
    assert D == 256 and case.cfg.get("att_scale") is None
    r0 = int(case.row_off[0])
    assert np.isin(case.kb[:, r0:, :D], (0x7F, 0xFF)).all() and np.isin(case.vb[:, r0:, :D], (0x7F, 0xFF)).all()
    assert (np.abs(ref.on_grid_codes(case.u0, case.cfg["fmt_w"][0])) == 127).all()
    top = max(int(np.abs(ch[q][0].codes).max()) for q in range(case.B))
    assert 127 * 127 * 16 < top <= 127 * 127 * 256 < 1 << 24
    assert all(ch[q][0].p.max() == 1.0 for q in range(case.B)), "one-hot by construction"

    case, ch = build("equal_scores"), reference_chain("equal_scores")
    for q in range(case.B):
        S = case.slots(q)[1]
        for hp in ch[q]:
            assert (hp.codes == hp.codes[0]).all() and np.allclose(hp.p, 1.0 / S, rtol=1e-12)
        assert ch[q][0].codes[0] != 0

    case, ch = build("two_maxima"), reference_chain("two_maxima")
    for q in range(case.B):
        a, b = case.marks["pairs"][q]
        c = ch[q][0].codes
        assert c[a] == c[b] == c.max() and (c == c.max()).sum() == 2, f"q{q}: two equal maxima at hop 0"
        assert all(hp.codes[a] == hp.codes[b] for hp in ch[q])


def test_format_draws_cover_the_stated_grids():
    draws = [build(n).cfg for n in FAMILIES["formats"] if n.startswith("formats_")]
    assert len(draws) == 12
    wl = lambda f: f[0] + f[1]
    assert {wl(f) for c in draws for k in ("fmt", "fmt_w") for f in c[k]} == set(range(1, 8)), "word lengths 1 .. 7"
    for k in ("fmt", "fmt_w", "fmt_att"):
        assert any(f[1] == 0 for c in draws for f in c[k]), f"frac 0 in {k}"
    assert any(c["fmt_bin"][1] == 0 for c in draws)
    rel = {np.sign(c["fmt"][h][1] - c["fmt_w"][h][1]) for c in draws for h in range(3)}
    assert rel == {-1, 0, 1}, "activations coarser than, equal to and finer than the weights"
    src = {np.sign(ref.src_fmt(c, h)[1] - c["fmt_w"][h][1]) for c in draws for h in range(3)}
    assert src == {-1, 0, 1}, "the state entering a hop coarser / finer than the hop's keys"
    for c in draws:                              # the score scale is re-tuned per draw
        assert c["att_scale"] is not None and all(np.isfinite(c["att_scale"]))
    assert len({tuple(c["att_scale"]) for c in draws}) == 12
    assert build("binary_mode").cfg["fmt_bin"] == (0, 0)
    assert build("no_lin_map").cfg["en_lin_map"] is False and build("no_lin_map").lin is None
    assert sorted(build(f"non_lin_{n}").cfg["softmax_variant"] for n in ("exp", "pow2", "plan")) == [0, 1, 2]
    assert all(build(f"non_lin_{n}").cfg["en_non_lin"] for n in ("exp", "pow2", "plan"))
    for n in ("non_lin_exp", "non_lin_pow2", "non_lin_plan"):      # the RELU changes something: a negative state enters a later hop
        assert any((hp.u_next < 0).any() for hops in reference_chain(n) for hp in hops[:-1])
    assert all(build(n).cfg.get("att_scale") is None for n in ("unscaled_d60", "unscaled_d256"))
    assert [np.sign(s) for s in build("scale_negative").cfg["att_scale"]] == [-1, 1, -1]


def test_cut_tied_and_tap_cases():
    T = fc.tile_rows(64)
    below, above = build("cut_below_tile"), build("cut_above_tile")
    assert below.max_slots < T < above.max_slots
    for case in (below, above):
        n = np.diff(case.row_off.astype(np.int64))
        assert (n > case.max_slots).sum() >= 2 and (n == case.max_slots).any() and (n == case.max_slots + 1).any() and (n < case.max_slots).any()
        q = int(np.argmax(n))
        assert len(reference_chain(case.name)[q][0].p) == case.max_slots, "the reference reads the first max_slots rows"
    tied = build("tied_planes")
    assert tied.tied and tied.kb.shape[0] == 1 and len(set(tied.cfg["fmt_w"])) == 1
    u = fc.untied(tied)
    assert u.kb.shape[0] == 3 and all(np.array_equal(u.kb[h], tied.kb[0]) for h in range(3))
    assert set(fc.TAP_COMBOS) == {fc.ALL_TAPS, (), ("codes",), ("scores",), ("probs",), ("o",), ("u",)}


# ---- 3. the reference against the oracle ---------------------------------------------------------------------------------------
ORACLE_CASES = sorted(n for n in CASES if CASES[n]["family"] not in ("minus_zero", "tied"))


@pytest.mark.parametrize("name", ORACLE_CASES)
def test_reference_against_the_oracle(oracle, name):
    """Hop-wise, as the GPU comparison: hop h of the reference starts from the ORACLE's state of the hop before, so the oracle's
    own float32 read-out (a serial float sum) may differ on `near` columns without cascading."""
    case = build(name)
    cfg = case.cfg
    H, D = cfg["n_hop"], cfg["dim_emb"]
    r_first = int(case.row_off[0])
    assert not (case.kb[:, r_first:] == 0x80).any() and not (case.vb[:, r_first:] == 0x80).any()
    m = oracle.make_model(cfg, case.wts)
    differ = 0
    for q in range(case.B):
        r0, S, _ = case.slots(q)
        if S == 0:
            continue                             # the reference never runs an empty story
        kf = np.stack([ref.decode(case.kb[h, r0:r0 + S, :D]).astype(np.float32) / np.float32(1 << cfg["fmt_w"][h][1]) for h in range(H)])
        vf = np.stack([ref.decode(case.vb[h, r0:r0 + S, :D]).astype(np.float32) / np.float32(1 << cfg["fmt_w"][h][1]) for h in range(H)])
        _, t = oracle.forward_mem(m, kf, vf, case.u0[q], taps=("scores", "probs", "o", "lu", "u"))
        u = case.u0[q]
        for h in range(H):
            hp = case.hop(q, h, u)
            fa = cfg["fmt"][h]
            at = f"{name} q{q} h{h}"
            np.testing.assert_array_equal(t["scores"][h], hp.scores, err_msg=f"scores {at}")
            # (atol: the oracle's p is a float32, which ends at 2^-126 where the float64 p goes on to 1e-300)
            np.testing.assert_allclose(t["probs"][h], hp.p, rtol=1e-5, atol=2.0 ** -126, err_msg=f"p {at}")
            # lu on its own grid Qw (the oracle's tap), then on the activation grid as the update reads it
            np.testing.assert_array_equal(ref.code_of(t["lu"][h], fa), hp.lu, err_msg=f"lu {at}")
            ok = ref.on_grid_codes(t["u"][h], fa)
            bad = (ok != hp.u_next) & ~hp.near
            assert not bad.any(), f"u {at}: columns {np.nonzero(bad)[0].tolist()} differ outside near"
            a, b = hp.allowed()
            assert ((ok == a) | (ok == b)).all(), f"u {at}: a near column is not one code across its step"
            differ += int((ok != hp.u_next).sum())
            u = t["u"][h]
    print(f"{name}: {differ} near columns where the oracle's float32 read-out lands across the step")


# ---- 4. the comparison routine --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiles_d60", "mz_words", "formats_03", "non_lin_plan", "cut_above_tile", "extreme_127"])
def test_comparison_accepts_a_correct_float32_read_out(name):
    case = build(name)
    stats = fc.check_outputs(case, fc.simulate(case))
    assert stats["cols"] > 0 and stats["differ"] <= stats["near"]


@pytest.mark.parametrize("fault,name,told", [("row_twice", "tiles_d60", "o "), ("row_twice", "width_d256", "o "),
                                             ("minus128", "mz_sprinkled", "o "), ("minus128", "mz_words", "o "),
                                             ("u_code", "tiles_d100", "u "), ("u_code", "formats_05", "u "),
                                             ("guard", "width_d17", "guard of u_out")])
def test_comparison_reports_each_fault(fault, name, told):
    case = build(name)
    with pytest.raises(AssertionError, match=told):
        fc.check_outputs(case, fc.simulate(case, fault=fault))


def test_comparison_reports_a_tap_written_past_a_cut():
    case = build("cut_below_tile")
    raw = fc.simulate(case)
    q = int(np.argmax(np.diff(case.row_off.astype(np.int64))))
    r0, S, s_in = case.slots(q)
    assert s_in > S
    fc.payload(case, raw, "probs")[1, r0 + S] = 0.0
    with pytest.raises(AssertionError, match="row no query reads"):
        fc.check_outputs(case, raw)
