"""CPU preconditions of test_gpu_embed_forms.py (embed_cases.py), in the pattern of test_shared_split_ham_inputs.py.  The
oracle and the library's host-side helper alone run here.

1. The numpy reference of embed_cases.py is pinned to the oracle: integer codes against dense_mat_fwd + code8 on random formats
   of word lengths 2 .. 7 per role; the SIGN BIT as well, against bit 31 of float2fixed's word, for every destination format
   of word length 8; whole key bytes of the Hamming forms against the top byte of float2fixed(value, iwl_att, 31 - iwl_att);
   question rows against dense_fwd.
2. Every case keeps its promise, asserted on the reference alone (a seed that fails is changed in embed_cases.py):
   * the duplicate-cap cases hold exactly 128 repeated (row, word) pairs in their tile and at least one row whose term-by-term
     sum differs from count . kw;
   * every epilogue-kind case contains on each hop and table a saturated sum (the clamped sum at +-maxw: what the byte's
     magnitude is made of -- a right shift can never reach the target maximum, Q4.3 -> Q5.2 ends at 63), a byte whose magnitude
     is the target maximum wherever the grids allow one, and a 0x80 wherever one can exist: where the target grid is coarser
     than the weight grid or the minus-zero rule holds (on an equal or finer grid a non-zero sum keeps a non-zero magnitude);
   * the minus-zero cases contain a key that is exactly -2^iwl_att on the weight grid;
   * no case's keys or values are all zero.
3. qmann_embed_story_idx_form (no launch, no GPU) names for every case the form the case is meant to reach."""
import ctypes as C

import numpy as np
import pytest

import embed_cases as ec
from embed_cases import CASES, KIND_CASES, QUERY_CASES, query_case, story_case


def from_signmag(b):
    u = np.asarray(b).view(np.uint8).astype(np.int64)
    return np.where(u & 0x80, -(u & 0x7F), u & 0x7F)


def table_floats(t, D, frac):
    """int8 [V][Dp] codes -> the float matrix [D][V] of grid values"""
    return np.ascontiguousarray((t[:, :D].astype(np.float32) / np.float32(1 << frac)).T)


def small_inputs(rng, V, W, D, fw, sigma, time_last, n_random=14):
    words = np.concatenate([ec.special_rows(V, W), ec.random_rows(rng, n_random, V, W)])
    m = ec.maxcode(fw)
    t = np.zeros((V, 64), np.int8)
    t[:, :D] = np.clip(np.rint(rng.normal(0, sigma, (V, D))), -m, m)
    return words, t


def rand_fmt(rng, lo=2, hi=7):
    wl = int(rng.integers(lo, hi + 1))              # word length with the sign bit
    iwl = int(rng.integers(0, wl))
    return (iwl, wl - 1 - iwl)


@pytest.mark.parametrize("draw", range(40))
def test_reference_codes_equal_the_oracle(oracle, draw):
    """dense_mat_fwd on the equivalent bag-of-words rows, then Q(target): the integer codes"""
    rng = np.random.default_rng(9100 + draw)
    fw, dst = rand_fmt(rng), rand_fmt(rng)
    V, D, W = (30, 90, 200)[draw % 3], 6, (16, 8, 5)[draw % 3]
    time_last = draw % 4 != 3
    words, t = small_inputs(rng, V, W, D, fw, (3.0, 12.0, 40.0)[draw % 3], time_last)
    sums = ec.embed_sums(ec.counts(words, V, time_last), t, fw)
    want = oracle.dense_mat_fwd(table_floats(t, D, fw[1]), ec.words_to_bow(words, V, time_last), True, fw)
    assert np.array_equal(sums[:, :D], np.rint(want.astype(np.float64) * (1 << fw[1])).astype(np.int64)), (fw, V)
    got = from_signmag(ec.to_bytes(sums, fw, dst))[:, :D]
    assert np.array_equal(got, oracle.code8(want, *dst)), (fw, dst, V)


@pytest.mark.parametrize("iwl_dst", range(8))
def test_reference_sign_bit_equals_the_oracle_word(oracle, iwl_dst):
    """word length 8: the whole byte -- magnitude AND sign bit -- against float2fixed's word (bit 31, low 7 bits)"""
    dst = (iwl_dst, 7 - iwl_dst)
    rng = np.random.default_rng(9200 + iwl_dst)
    seen80 = False
    for fw in [(5, 2), (6, 1), (4, 3), (0, 7), (7, 0), (2, 2), (1, 1)]:
        words, t = small_inputs(rng, 30, 8, 6, fw, 0.4 * ec.maxcode(fw), True)
        sums = ec.embed_sums(ec.counts(words, 30, True), t, fw)
        val = (sums[:, :6].astype(np.float32) / np.float32(1 << fw[1])).astype(np.float32)
        word = oracle.float2fixed(val, *dst).astype(np.int64) & 0xFFFFFFFF
        want = ((word >> 31) << 7) | (word & 0x7F)
        assert ((word & 0x7FFFFF80) == 0).all()
        got = ec.to_bytes(sums, fw, dst)[:, :6]
        assert np.array_equal(got, want.astype(np.uint8)), (fw, dst)
        seen80 |= bool((got == 0x80).any())
    assert seen80 or iwl_dst < 2, "no draw produced a minus zero on this target"


@pytest.mark.parametrize("mode", [10, 11, 3])
def test_hamming_key_bytes_equal_the_oracle_operand(oracle, mode):
    """modes 10 / 11 (and the hops of mode 3 whose keys sit on the attention grid): the key byte is the top byte of the
    operand word Q(iwl_att, 31 - iwl_att) of the value on the weight grid -- truncation, clamp, sign of the value, minus zero
    at exactly -2^iwl_att"""
    rng = np.random.default_rng(9300 + mode)
    n_mz = n_checked = 0
    fmts = [[(6, 1), (5, 2), (4, 3)]] + [[rand_fmt(rng, 3, 7) for _ in range(3)] for _ in range(12)]
    for i, fmt_w in enumerate(fmts):
        ia = 5 if i == 0 else int(rng.integers(1, 7))
        cfg = ec.make_cfg(30, 6, 3, mode, fmt_w=fmt_w, fmt=[(ia, 7 - ia)] * 3)
        for h in range(3):
            fw, att = cfg["fmt_w"][h], cfg["fmt_att"][h]
            kf, mz = ec.key_format(cfg, h)
            if kf != tuple(att):
                assert mode == 3
                continue                                            # mode 3, keys kept on the weight grid: not an operand byte
            words, t = small_inputs(rng, 30, 8, 6, fw, 0.5 * ec.maxcode(fw), True)
            t[3, :6] = -ec.maxcode(fw)                              # (full-scale rows: exact powers of two are reachable)
            sums = ec.embed_sums(ec.counts(words, 30, True), t, fw)
            val = (sums[:, :6].astype(np.float32) / np.float32(1 << fw[1])).astype(np.float32)
            word = oracle.float2fixed(val, att[0], 31 - att[0]).astype(np.int64) & 0xFFFFFFFF
            got = ec.to_bytes(sums, fw, kf, mz)[:, :6]
            assert np.array_equal(got, (word >> 24).astype(np.uint8)), (mode, fmt_w, att, h)
            n_mz += int(((val == -float(1 << att[0])) & (got == 0x80)).sum())
            n_checked += got.size
    assert n_checked > 1000 and n_mz > 0


@pytest.mark.parametrize("name", sorted(QUERY_CASES))
def test_question_rows_equal_the_oracle(oracle, name):
    c = query_case(name)
    cfg = c["cfg"]
    V, D, fw = cfg["dim_input"], cfg["dim_emb"], cfg["fmt_w"][0]
    w = table_floats(c["t_q"], D, fw[1])
    pick = np.unique(np.linspace(0, c["B"] - 1, 24).astype(int))
    for q in pick:
        row = c["words"][q]
        if cfg.get("en_pe"):
            x = np.zeros(V, np.float32)
            for j, wd in enumerate(row):
                if wd != ec.EMPTY and wd < V:
                    a = np.float64(np.float32(wd) / np.float32(V)) - 0.5
                    b = np.float64(np.float32(j) / np.float32(cfg["pe_dim_word"])) - 0.5
                    x[wd] = np.float32(1.0 + (4.0 * a) * b)
        else:
            x = ec.words_to_bow(row[None], V, False)[0]
        want = oracle.dense_fwd(w, x, True, fw, fw)
        assert np.array_equal(c["u0"][q], want), (name, q)
    assert np.abs(c["u0"]).sum() > 0
    if c.get("repeat8"):                                            # the repeated word's product leaves the format somewhere
        m = ec.maxcode(fw)
        cc = min(8 << fw[1], m)
        t = c["t_q"].astype(np.int64)
        assert (ec.mul_code(cc, t[c["words"][0, 0]], fw[1], m) != 8 * t[c["words"][0, 0]]).any()


# ---- the promises of the cases ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_no_case_is_all_zero_and_columns_past_d_are(name):
    c = story_case(name)
    D = c["cfg"]["dim_emb"]
    rows = ec.BLOCK_ROWS if c["many"] else c["rows"]
    assert c["keys"].shape == c["vals"].shape == (c["H"], rows, c["Dp"])
    for h in range(c["H"]):
        assert c["keys"][h].any() and c["vals"][h].any(), (name, h)
    assert not c["keys"][:, :, D:].any() and not c["vals"][:, :, D:].any()
    if c["content"] == "rows" and rows >= 40:                       # the special block is in, and straddles two tiles
        sp = ec.special_rows(c["V"], c["W"])
        at = ec.special_at(rows, len(sp))
        assert np.array_equal(c["words"][at:at + len(sp)], sp) and at // 16 != (at + len(sp) - 1) // 16


@pytest.mark.parametrize("name", sorted(n for n in CASES if n.startswith("dupcap")))
def test_duplicate_cap_cases(name):
    c = story_case(name)
    assert c["words"].shape == (16, 16) and not c["time_last"]
    cnt = ec.counts(c["words"], c["V"], False)
    assert int((cnt >= 2).sum()) == 128 and int((cnt == 2).sum()) == 128          # kEmDupCap, exactly
    slow_rows = set()
    for h in range(c["H"]):
        fw = c["cfg"]["fmt_w"][h]
        m = ec.maxcode(fw)
        for t in (c["t_a"][h], c["t_c"][h]):
            term = ec.embed_sums(cnt, t, fw)                                       # term by term
            plain = np.clip(cnt @ t.astype(np.int64), -m, m)                       # count . kw, clamped at the end only
            slow_rows |= set(np.flatnonzero((term != plain).any(1)).tolist())
    assert slow_rows, "no repeated product leaves the format: the term-by-term path would not run"
    print(f"{name}: {len(slow_rows)} of 16 rows differ from count . kw")


@pytest.mark.parametrize("name", sorted(n for n in CASES if n.startswith("kinds_")))
def test_epilogue_kind_cases(name):
    c = story_case(name)
    cfg = c["cfg"]
    D = cfg["dim_emb"]
    kinds = []
    for h in range(c["H"]):
        fw = cfg["fmt_w"][h]
        kf, mz = ec.key_format(cfg, h)
        for what, dst, rule, sums, by in (("key", kf, mz, c["ksum"][h], c["keys"][h]), ("val", tuple(cfg["fmt"][h]), False, c["vsum"][h], c["vals"][h])):
            kinds.append(ec.qkind(fw, dst, rule))
            m, md = ec.maxcode(fw), ec.maxcode(dst)
            assert (np.abs(sums[:, :D]) == m).any(), (name, h, what, "no saturated sum")
            top = (m << (dst[1] - fw[1])) if dst[1] >= fw[1] else (m >> (fw[1] - dst[1]))
            if top >= md:
                assert ((by[:, :D] & 0x7F) == md).any(), (name, h, what, "no byte at the target maximum")
            if dst[1] < fw[1] or rule:
                assert (by[:, :D] == 0x80).any(), (name, h, what, "no minus zero")
            if rule:
                edge = -(1 << (dst[0] + fw[1]))                                     # -2^iwl_att on the weight grid
                assert (sums[:, :D] == edge).any(), (name, h, "no key at exactly -2^iwl_att")
    base = next(n for n in KIND_CASES if name.startswith(n + "_"))
    want = {"kinds_mq": ["left", "left", "same", "same", "right", "right"], "kinds_general": ["general", "general"],
            "kinds_mz10": ["general", "left", "same", "same", "right", "right"],
            "kinds_mz11": ["general", "left", "same", "same", "right", "right"],
            "kinds_fine3": ["general", "left", "same", "same", "same", "right"]}[base]
    assert kinds == want, (name, kinds)
    if name.startswith("kinds_fine3"):
        assert ec.key_format(cfg, 2)[0] == tuple(cfg["fmt_w"][2]) != tuple(cfg["fmt_att"][2])


# ---- the form helper (no launch) ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from conftest import load_pkg
    load_pkg()
    import qmann_amd.abi as abi
    import qmann_amd.model as model
    return abi, model


@pytest.mark.parametrize("name", sorted(CASES))
def test_form_helper_names_the_form_of_every_case(lib, monkeypatch, name):
    abi, model = lib
    c = story_case(name)
    for k in ("QMANN_EMBED_VALU", "QMANN_EMBED_PER_HOP", "QMANN_EMBED_GENERAL_EPILOGUE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)
    abi.lib.qmann_tuning_reload()
    net = model._net_from_cfg(c["cfg"])
    words = C.c_void_p(0x10000 + 2 * c["offset"])                                 # (the helper reads the pointer's alignment only)
    assert abi.lib.qmann_embed_story_idx_form(C.byref(net), words, c["W"]) == c["form"], ec.FORM_NAMES[c["form"]]


def test_form_helper_refusals(lib):
    abi, model = lib
    net = model._net_from_cfg(ec.make_cfg(30, 60, 3))
    form = abi.lib.qmann_embed_story_idx_form
    assert form(None, None, 8) == abi.QMANN_EINVAL
    assert form(C.byref(net), None, 0) == abi.QMANN_ERANGE and form(C.byref(net), None, 17) == abi.QMANN_ERANGE
    assert form(C.byref(net), None, 8) == abi.EMBED_MFMA_PER_HOP
    net.dim_emb_pad = 96
    assert form(C.byref(net), None, 8) == abi.QMANN_EUNSUPPORTED
    net.dim_emb_pad, net.n_hop = 64, 9
    assert form(C.byref(net), None, 8) == abi.QMANN_EINVAL
    net.n_hop = 3
    net.w[1] = abi.Fmt(5, 3)
    assert form(C.byref(net), None, 8) == abi.QMANN_ERANGE


def test_plane_check_notices_one_wrong_byte_and_one_touched_guard():
    """the GPU test's own comparison (test_gpu_embed_forms.check_planes), on CPU tensors: a minus zero read as zero, a byte
    behind the last plane and a byte between two planes each fail it"""
    import torch
    from test_gpu_embed_forms import FILL, GUARD, check_planes

    class Env:
        pass
    env = Env()
    env.torch = torch
    H, rows, Dp = 2, 3, 64
    want = torch.arange(H * rows * Dp, dtype=torch.int64).remainder(251).to(torch.uint8).reshape(H, rows, Dp)
    want[1, 2, 5] = 0x80

    def buf():
        b = torch.full((GUARD + H * (rows * Dp + GUARD),), FILL, dtype=torch.uint8)
        b[GUARD:].view(H, rows * Dp + GUARD)[:, :rows * Dp] = want.reshape(H, -1)
        return b
    check_planes(env, "clean", buf(), H, rows, Dp, want)
    for at, msg in ((GUARD + rows * Dp + GUARD + 2 * Dp + 5, "differ"), (GUARD - 1, "guard"), (GUARD + rows * Dp, "guard"), (-1, "guard")):
        b = buf()
        b[at] = 0
        with pytest.raises(AssertionError, match=msg):
            check_planes(env, "touched", b, H, rows, Dp, want)
