"""The seeded inputs and the exact-integer reference of the story / question embedding from word indices
(qmann_embed_story_idx, qmann_embed_query_idx) -- ONE definition, read by the GPU test (test_gpu_embed_forms.py) and by the
CPU precondition test (test_embed_inputs.py).  Not collected by pytest.

The reference is plain numpy on int64, independent of both GPU embedding kernels, with no float arithmetic after the table
codes (test_embed_inputs.py pins it to the oracle's dense_mat_fwd / float2fixed):
  counts     every non-0xFFFF slot whose word is < V counts; with time_last the LAST non-0xFFFF slot of a row is its time slot,
             even when its word is out of range; a time slot whose word is < V SETS that word's count to 1
  sum        per hop and table: sum_w mul_code(min(count_w << frac_w, maxw), T[w]) with qfmt.h::qm_mul_code (product, shift
             toward zero, clamp to +-maxw), then clamped to +-maxw
  byte       |sum| moved to the target grid toward zero, the minus-zero rule on keys where qfmt.h::ham_key_format says so,
             clamp to the target maximum, sign bit from the clamped SUM (so 0x80 exists)
Keys go to the format ham_key_format gives, values to act[h]; columns D .. Dp-1 are zero.

Every case names the kernel form it is meant to reach (FORM_*: include/qmann_batch.h's QMANN_EMBED_*); the tests assert that
qmann_embed_story_idx_form agrees, so a change of the dispatch that moves a case to another kernel fails instead of thinning
the suite.  A seed whose draw fails a precondition of test_embed_inputs.py is changed here; the assertions stay."""
from __future__ import annotations

import functools

import numpy as np

FORM_GATHER_LDS, FORM_GATHER_L2, FORM_MFMA_PER_HOP, FORM_MFMA_ALL_HOPS = 0, 1, 2, 3
FORM_NAMES = {0: "gather-sum, tables in LDS", 1: "gather-sum from L2", 2: "matrix cores per hop", 3: "matrix cores, all hops"}
EMPTY = 0xFFFF
BLOCK_ROWS = 1009                       # distinct rows of the block the many-rows cases repeat
MANY = "many"                           # rows = 16 . 48 . CUs + 37 (resolved on the device: many_rows)


def pad_dim(D):
    return 64 if D <= 64 else (128 if D <= 128 else 256)


def many_rows(cus):
    """more tiles than any form's persistent grid holds at once: 48 = 3 workgroups x 16 wavefronts per CU, above every
    form's residency in rt.h::qm_resident_groups"""
    return 16 * 48 * int(cus) + 37


# ---- the reference -----------------------------------------------------------------------------------------------------------
def maxcode(fmt):
    return (1 << (fmt[0] + fmt[1])) - 1


def counts(words, V, time_last):
    """uint16 [rows][W] -> int64 [rows][V] bag-of-words counts"""
    words = np.asarray(words).astype(np.int64)
    rows, W = words.shape
    used = words != EMPTY
    cnt = np.zeros((rows, V), np.int64)
    r, s = np.nonzero(used & (words < V))
    np.add.at(cnt, (r, words[r, s]), 1)
    if time_last:
        any_used = used.any(1)
        last = W - 1 - np.argmax(used[:, ::-1], axis=1)
        tw = words[np.arange(rows), last]
        ok = any_used & (tw < V)
        cnt[np.flatnonzero(ok), tw[ok]] = 1
    return cnt


def mul_code(ka, kb, frac, maxa):
    """qfmt.h::qm_mul_code: product, shift toward zero, clamp"""
    p = np.asarray(ka, np.int64) * np.asarray(kb, np.int64)
    t = np.sign(p) * (np.abs(p) >> frac)
    return np.clip(t, -maxa, maxa)


def embed_sums(cnt, table, fw):
    """cnt int64 [rows][V], table int [V][Dp] two's-complement codes of Q(fw) -> the clamped sums int64 [rows][Dp]"""
    frac, maxw = fw[1], maxcode(fw)
    r, w = np.nonzero(cnt)
    cc = np.minimum(cnt[r, w] << frac, maxw)
    terms = mul_code(cc[:, None], np.asarray(table, np.int64)[w], frac, maxw)
    out = np.zeros((cnt.shape[0], table.shape[1]), np.int64)
    np.add.at(out, r, terms)
    return np.clip(out, -maxw, maxw)


def to_bytes(sums, fw, dst, minus_zero=False):
    """clamped sums on the grid of fw -> memory bytes (uint8, sign-magnitude) on the grid of dst"""
    mag = np.abs(sums)
    mag = mag << (dst[1] - fw[1]) if dst[1] >= fw[1] else mag >> (fw[1] - dst[1])
    md = maxcode(dst)
    if minus_zero:
        mag = np.where((mag == md + 1) & (sums < 0), 0, mag)
    mag = np.minimum(mag, md)
    return (mag | np.where(sums < 0, 0x80, 0)).astype(np.uint8)


# qfmt.h::ham_hop_kind / ham_key_format
HAM_SAME, HAM_COARSE, HAM_FINE, HAM_NONE = 0, 1, 2, 3


def ham_hop_kind(src, wk, att):
    u_in = src[0] <= att[0] and src[1] <= att[1]
    k_in = wk[0] <= att[0] and wk[1] <= att[1]
    if u_in and k_in:
        return HAM_SAME
    if src[1] + 1 <= att[1] and wk[1] + 1 <= att[1]:
        return HAM_COARSE
    if u_in and wk[1] == att[1] + 1 and wk[0] + 1 <= att[0]:
        return HAM_FINE
    return HAM_NONE


def key_format(cfg, h):
    """-> (format of hop h's key bytes, minus-zero rule?)"""
    mode = cfg["attention_mode"]
    src = cfg["fmt_w"][0] if h == 0 else cfg["fmt"][h - 1]
    wk, att = cfg["fmt_w"][h], cfg["fmt_att"][h]
    ham = mode in (3, 10, 11)
    mz = ham and wk[0] > att[0]
    if mode == 3 and ham_hop_kind(src, wk, att) == HAM_FINE:
        return tuple(wk), mz
    return tuple(att), mz


def qkind(fw, dst, mz):
    """batch_embed_idx.hip::qkind_of -- how the matrix-core epilogue quantises: 'same', 'left', 'right' or 'general'"""
    maxw, md = maxcode(fw), maxcode(dst)
    if mz or maxw > 127:
        return "general"
    if dst[1] == fw[1] and md >= maxw:
        return "same"
    if dst[1] == fw[1] + 1 and md == 127:
        return "left"
    if dst[1] + 1 == fw[1] and md >= (maxw >> 1):
        return "right"
    return "general"


def story_reference(cfg, words, t_a, t_c, time_last):
    """-> keys, vals uint8 [H][rows][Dp] (columns D.. zero), and the clamped key / value sums int64 [H][rows][Dp]"""
    H, D, V = cfg["n_hop"], cfg["dim_emb"], cfg["dim_input"]
    cnt = counts(words, V, time_last)
    keys, vals, ks, vs = [], [], [], []
    for h in range(H):
        fw = cfg["fmt_w"][h]
        kf, mz = key_format(cfg, h)
        sa, sc = embed_sums(cnt, t_a[h], fw), embed_sums(cnt, t_c[h], fw)
        kb, vb = to_bytes(sa, fw, kf, mz), to_bytes(sc, fw, cfg["fmt"][h])
        kb[:, D:] = 0
        vb[:, D:] = 0
        keys.append(kb); vals.append(vb); ks.append(sa); vs.append(sc)
    return np.stack(keys), np.stack(vals), np.stack(ks), np.stack(vs)


def pe_code(word, slot, V, dim_word, fw):
    """EN_PE: the code on Q(fw) of the position weight 1 + 4 (word / V - 0.5)(slot / dim_word - 0.5) (float quotients, the
    rest in double, stored as float: MemN2N/MemN2N.c:615), as qfmt.h::qm_code truncates it"""
    a = np.float64(np.float32(word) / np.float32(V)) - 0.5
    b = np.float64(np.float32(slot) / np.float32(dim_word)) - 0.5
    pw = np.float32(1.0 + (4.0 * a) * b)
    M = maxcode(fw)
    maxf = np.float32(M) / np.float32(1 << fw[1])
    if pw > maxf:
        return M
    if pw < -maxf:
        return -M
    return int(np.float32(pw) * np.float32(1 << fw[1]))


def question_reference(cfg, words, t_q):
    """-> float32 [n_query][D]: the sum on w[0] as code . 2^-frac (word entries only, no time entry)"""
    D, V, fw = cfg["dim_emb"], cfg["dim_input"], cfg["fmt_w"][0]
    frac, maxw = fw[1], maxcode(fw)
    if not cfg.get("en_pe"):
        s = embed_sums(counts(words, V, False), t_q, fw)
    else:                                       # the last occurrence of a word decides its weight
        s = np.zeros((words.shape[0], t_q.shape[1]), np.int64)
        tq = np.asarray(t_q, np.int64)
        for q, row in enumerate(np.asarray(words).astype(np.int64)):
            kx = {}
            for j, w in enumerate(row):
                if w != EMPTY and w < V:
                    kx[int(w)] = pe_code(int(w), j, V, cfg["pe_dim_word"], fw)
            for w, k in kx.items():
                s[q] += mul_code(k, tq[w], frac, maxw)
        s = np.clip(s, -maxw, maxw)
    return (s[:, :D].astype(np.float32) / np.float32(1 << frac)).astype(np.float32)


def words_to_bow(words, V, time_last):
    """the equivalent float bag-of-words rows (what qmann_embed_story takes)"""
    return counts(words, V, time_last).astype(np.float32)


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def make_cfg(V, D, H, mode=2, fmt_w=None, fmt=None, fmt_att=None, **extra):
    """the dict shape of qmann_amd.model.babi_cfg.  Default formats: the reference's mixed quantisation (EN_MQ) around iwl 5,
    continued cyclically over the hops -- weights on Q6.1, Q5.2, Q4.3, everything else on Q5.2"""
    mq = [(6, 1), (5, 2), (4, 3)]
    fmt_w = list(fmt_w) if fmt_w is not None else [mq[h % 3] for h in range(H)]
    fmt = list(fmt) if fmt is not None else [(5, 2)] * H
    fmt_att = list(fmt_att) if fmt_att is not None else list(fmt)
    return dict(n_hop=H, dim_emb=D, dim_input=int(V), attention_mode=mode, softmax_variant=0, f_fixed=True, en_lin_map=True,
                fmt=fmt, fmt_w=fmt_w, fmt_att=fmt_att, fmt_bin=fmt[0], **extra)


def make_tables(rng, cfg, sigma_rel):
    """int8 [H][V][Dp] two's-complement codes of Q(w[h]) drawn directly (sigma = sigma_rel . maxw), columns D.. zero"""
    H, D, V = cfg["n_hop"], cfg["dim_emb"], cfg["dim_input"]
    Dp = pad_dim(D)
    out = []
    for _ in range(2):
        t = np.zeros((H, V, Dp), np.int8)
        for h in range(H):
            m = maxcode(cfg["fmt_w"][h])
            t[h, :, :D] = np.clip(np.rint(rng.normal(0, sigma_rel * m, (V, D))), -m, m)
        out.append(t)
    return out


def _row(W, ent):
    r = np.full(W, EMPTY, np.uint16)
    ent = list(ent)[:W]
    r[:len(ent)] = ent
    return r


def special_rows(V, W):
    """the deterministic block of row contents (what fits W slots of it).  `t` stands where a time entry would; with
    time_last = 0 it is one more word."""
    a, b, c, t = 1 % V, 2 % V, 3 % V, V - 1
    rows = [_row(W, [])]                                                  # all empty
    if W >= 4:
        rows.append(_row(W, [a, EMPTY, b, t]))                            # a hole in the middle
        rows.append(_row(W, [a, EMPTY, EMPTY, t]))
        rows.append(_row(W, [a, t, b, t]))                                # a word slot equal to the time entry
        rows.append(_row(W, [t, t, t, t]))
    if W >= 3:
        rows.append(_row(W, [V + 3, a, t]))                               # out of range in the first slot
        rows.append(_row(W, [a, b, V + 5]))                               # out of range in the last non-empty slot: no time entry
        rows.append(_row(W, [a, b, 0xFFFE]))
    rows.append(_row(W, [V]))                                             # (the first word past the dictionary, alone)
    for k in (2, 5, 15):                                                  # a word repeated beside the time entry
        if k + 1 <= W:
            rows.append(_row(W, [c] * k + [t]))
            rows.append(_row(W, [b] + [c] * (k - 1) + [t]))
    rows.append(_row(W, [c] * W))                                         # a word in every slot (time_last = 0: W repeats)
    return np.stack(rows)


def random_rows(rng, n, V, W, small=4):
    """ragged rows: 0 .. W-1 words and a time entry from the top of the dictionary; every third row draws from a tiny
    vocabulary (repeats), some carry an out-of-range word, a hole, or the time word in a word slot"""
    out = np.full((n, W), EMPTY, np.uint16)
    top = max(V - 12, 1)
    for r in range(n):
        k = int(rng.integers(0, W))
        ws = rng.integers(0, top if r % 3 else min(top, small), k)
        t = top + int(rng.integers(0, V - top)) if V > top else 0
        ent = [int(x) for x in ws] + [t]
        if r % 17 == 5:
            ent[0] = V + int(rng.integers(0, 9))
        if r % 29 == 7 and len(ent) > 1:
            ent[-2] = t
        if r % 13 == 3 and len(ent) > 2:
            ent[1] = EMPTY
        if r % 31 == 11:
            ent[-1] = V + 1                                               # the last non-empty slot out of range
        out[r, :len(ent)] = ent
    return out


def special_at(rows, n_special):
    """where the special block starts: two rows before a tile boundary near the end, so that it straddles two tiles"""
    return 16 * ((rows - n_special - 2) // 16) - 2


def build_rows(rng, rows, V, W):
    """`rows` rows: random ones, and from 40 rows on the special block across a tile boundary near the end"""
    if rows < 40:
        out = random_rows(rng, rows, V, W)
        if rows and (out == EMPTY).all():
            out[0, 0] = 0
        return out
    sp = special_rows(V, W)
    out = random_rows(rng, rows, V, W)
    at = special_at(rows, len(sp))
    out[at:at + len(sp)] = sp
    return out


def dupcap_rows(rng, V):
    """one tile of 16 rows, each holding 8 distinct words twice (max_words 16, no time entry): 128 repeated (row, word) pairs"""
    out = np.zeros((16, 16), np.uint16)
    for r in range(16):
        w = rng.choice(V, size=8, replace=False)
        out[r] = rng.permutation(np.concatenate([w, w]))
    return out


def _c(form, V, D=60, H=3, rows=None, W=8, mode=2, time_last=1, env=None, offset=0, sigma=0.4, content="rows", **cfg_kw):
    return dict(form=form, V=V, D=D, H=H, rows=rows, W=W, mode=mode, time_last=time_last, env=dict(env or {}), offset=offset,
                sigma=sigma, content=content, cfg_kw=cfg_kw)


PH, AH, GL, G2 = FORM_MFMA_PER_HOP, FORM_MFMA_ALL_HOPS, FORM_GATHER_LDS, FORM_GATHER_L2
PER_HOP, VALU, GEN = {"QMANN_EMBED_PER_HOP": "1"}, {"QMANN_EMBED_VALU": "1"}, {"QMANN_EMBED_GENERAL_EPILOGUE": "1"}
CASES = {}


def _add(name, **kw):
    assert name not in CASES, name
    CASES[name] = kw


# forms by hop count and dictionary class (rows: 16 . wavefronts + 1 -- 129 for the 8-wavefront form, 257 for the others)
for _H in (1, 2, 3, 4, 8):
    _add(f"per_hop_k64_h{_H}", **_c(PH, 30, H=_H, rows=129))
    _add(f"per_hop_k128_h{_H}", **_c(PH, 90, H=_H, rows=257, W=16))
for _H in (1, 4, 8):
    _add(f"per_hop_k256_h{_H}", **_c(PH, 238, H=_H, rows=257, W=16))
for _H in (2, 3):
    _add(f"per_hop_k256_h{_H}_switch", **_c(PH, 238, H=_H, rows=257, W=16, env=PER_HOP))
    _add(f"all_hops_v238_h{_H}", **_c(AH, 238, H=_H, rows=257, W=16))
    _add(f"all_hops_v129_h{_H}", **_c(AH, 129, H=_H, rows=257, W=8))
_add("gather_lds_v40_w11", **_c(GL, 40, rows=257, W=11))
_add("gather_l2_v500", **_c(G2, 500, rows=257, W=8))
# the gather kernels on matrix-core shapes
_add("gather_lds_valu_v30", **_c(GL, 30, rows=129, env=VALU))
_add("gather_l2_valu_v238", **_c(G2, 238, rows=257, W=16, env=VALU))
_add("gather_lds_unaligned_v30", **_c(GL, 30, rows=129, offset=1))
_add("gather_l2_unaligned_v238", **_c(G2, 238, rows=257, W=16, offset=1))
_add("gather_lds_iwl0_v30", **_c(GL, 30, rows=129, fmt_w=[(0, 7), (0, 6), (0, 5)], fmt=[(0, 7)] * 3))
_add("gather_l2_iwl0_v238", **_c(G2, 238, rows=257, W=16, fmt_w=[(5, 2), (0, 7), (4, 3)]))
# wider embeddings (gather kernels only)
_add("gather_lds_dp128", **_c(GL, 40, D=100, rows=257, W=11))
_add("gather_l2_dp128", **_c(G2, 500, D=100, rows=129, W=5))
_add("gather_lds_dp256", **_c(GL, 40, D=256, H=1, rows=129, W=16))
_add("gather_l2_dp256", **_c(G2, 300, D=256, rows=129, W=8))
# D at Dp = 64
for _D in (1, 17, 64):
    _add(f"per_hop_k64_d{_D}", **_c(PH, 30, D=_D, rows=129))
    _add(f"all_hops_d{_D}", **_c(AH, 238, D=_D, rows=257, W=16))
    _add(f"gather_lds_d{_D}", **_c(GL, 40, D=_D, rows=129, W=11))
# rows
for _R in (1, 15, 16, 17):
    _add(f"per_hop_k64_rows{_R}", **_c(PH, 30, rows=_R))
    _add(f"per_hop_k256_rows{_R}", **_c(PH, 238, H=1, rows=_R, W=16))
    _add(f"all_hops_rows{_R}", **_c(AH, 238, rows=_R, W=16))
    _add(f"gather_lds_rows{_R}", **_c(GL, 40, rows=_R, W=11))
    _add(f"gather_l2_rows{_R}", **_c(G2, 500, rows=_R, W=8))
# max_words
for _W in (4, 8, 12, 16):
    _add(f"per_hop_k64_w{_W}", **_c(PH, 30, rows=129, W=_W))
    _add(f"per_hop_k128_w{_W}", **_c(PH, 90, rows=257, W=_W))
    _add(f"all_hops_w{_W}", **_c(AH, 238, rows=257, W=_W))
for _W in (1, 5, 11, 16):
    _add(f"gather_lds_w{_W}", **_c(GL, 40, rows=129, W=_W, env=VALU if _W % 4 == 0 else None))
    _add(f"gather_l2_w{_W}", **_c(G2, 500, rows=129, W=_W))
# no time entry: every slot counts (a word repeated 16 times is in the special block)
_add("per_hop_k64_no_time", **_c(PH, 30, rows=129, W=16, time_last=0))
_add("all_hops_no_time", **_c(AH, 238, rows=257, W=16, time_last=0))
_add("gather_lds_no_time", **_c(GL, 40, rows=129, W=16, time_last=0, env=VALU))
# the duplicate list at its cap (weights large enough that a repeated product leaves the format)
_add("dupcap_per_hop_k64", **_c(PH, 30, rows=16, W=16, time_last=0, sigma=0.8, content="dupcap"))
_add("dupcap_per_hop_k256", **_c(PH, 238, H=1, rows=16, W=16, time_last=0, sigma=0.8, content="dupcap"))
_add("dupcap_all_hops", **_c(AH, 238, rows=16, W=16, time_last=0, sigma=0.8, content="dupcap"))
_add("dupcap_gather_lds", **_c(GL, 30, rows=16, W=16, time_last=0, sigma=0.8, content="dupcap", env=VALU))
# epilogue kinds: name -> (mode, hops, formats), on a per-hop and on the all-hops form, with and without the general epilogue
KIND_CASES = {
    "kinds_mq": dict(mode=2, H=3),                                             # left, same, right on hops 0, 1, 2
    "kinds_general": dict(mode=2, H=1, fmt_w=[(4, 1)], fmt=[(2, 2)]),          # Q4.1 -> Q2.2
    "kinds_mz10": dict(mode=10, H=3),                                          # minus-zero general on hop 0
    "kinds_mz11": dict(mode=11, H=3),
    "kinds_fine3": dict(mode=3, H=3),                                          # hop 2's keys stay on the weight grid
}
for _n, _k in KIND_CASES.items():
    for _sw, _env in (("", None), ("_general_epilogue", GEN)):
        _add(f"{_n}_per_hop{_sw}", **_c(PH, 30 if _k["H"] == 3 else 238, rows=129, W=8, sigma=0.5, env=_env, **_k))
        if _k["H"] == 3:
            _add(f"{_n}_all_hops{_sw}", **_c(AH, 238, rows=257, W=16, sigma=0.5, env=_env, **_k))
# more tiles than the grid holds at once: one case per matrix-core form and per gather form
_add("many_per_hop_k64", **_c(PH, 30, rows=MANY, W=8))
_add("many_per_hop_k128", **_c(PH, 90, rows=MANY, W=8))
_add("many_per_hop_k256", **_c(PH, 238, rows=MANY, W=16, env=PER_HOP))
_add("many_all_hops", **_c(AH, 238, rows=MANY, W=16))
_add("many_gather_lds", **_c(GL, 40, rows=MANY, W=11))
_add("many_gather_l2", **_c(G2, 500, rows=MANY, W=8))

SEEDS = {}                                      # name -> seed, where the default (a hash of the name) failed a precondition


def _seed(name):
    return SEEDS.get(name, sum((i + 1) * ord(ch) for i, ch in enumerate(name)) + 7000)


@functools.lru_cache(maxsize=None)
def story_case(name):
    """-> dict: spec fields, cfg, words uint16 [rows][W] (for a many-rows case: the 1 009-row block), t_a / t_c int8
    [H][V][Dp], keys / vals uint8 [H][rows][Dp] and the clamped sums ksum / vsum of the reference.  Arrays are shared: read only."""
    c = CASES[name]
    rng = np.random.default_rng(_seed(name))
    kw = dict(c["cfg_kw"])
    H, mode = kw.pop("H", c["H"]), kw.pop("mode", c["mode"])
    cfg = make_cfg(c["V"], c["D"], H, mode, **kw)
    t_a, t_c = make_tables(rng, cfg, c["sigma"])
    if c["content"] == "dupcap":
        words = dupcap_rows(rng, c["V"])
    else:
        words = build_rows(rng, BLOCK_ROWS if c["rows"] == MANY else c["rows"], c["V"], c["W"])
    keys, vals, ksum, vsum = story_reference(cfg, words, t_a, t_c, c["time_last"])
    for a in (words, t_a, t_c, keys, vals, ksum, vsum):
        a.setflags(write=False)
    out = dict(c)
    out.update(name=name, H=H, mode=mode, cfg=cfg, Dp=pad_dim(c["D"]), words=words, t_a=t_a, t_c=t_c, keys=keys, vals=vals,
               ksum=ksum, vsum=vsum, many=c["rows"] == MANY)
    return out


def tile_block(a, rows):
    """a [..., BLOCK_ROWS, x] repeated along the rows axis to `rows` rows"""
    reps = -(-rows // a.shape[-2])
    return np.concatenate([a] * reps, axis=-2)[..., :rows, :]


# ---- the question kernel -------------------------------------------------------------------------------------------------------
# n_query, D, V (V . Dp on either side of 48 KiB: 700 / 800 at Dp = 64), offset of u0 in floats, special content
QUERY_CASES = {}
for _B in (1, 3, 4, 5, 1000):
    for _D in (60, 17):
        QUERY_CASES[f"q{_B}_d{_D}"] = dict(B=_B, D=_D, V=90, W=8)
QUERY_CASES["lds_v700"] = dict(B=37, D=60, V=700, W=8)
QUERY_CASES["l2_v800"] = dict(B=37, D=60, V=800, W=8)
QUERY_CASES["l2_v800_d17"] = dict(B=37, D=17, V=800, W=5)
QUERY_CASES["u0_offset"] = dict(B=37, D=60, V=90, W=8, u0_offset=1)
QUERY_CASES["u0_offset_l2"] = dict(B=37, D=60, V=800, W=16, u0_offset=1)
QUERY_CASES["repeat8_saturating"] = dict(B=21, D=60, V=90, W=8, repeat8=True, sigma=0.8)
QUERY_CASES["pe"] = dict(B=37, D=60, V=90, W=8, en_pe=True)
QUERY_CASES["pe_l2"] = dict(B=37, D=17, V=800, W=11, en_pe=True)
QUERY_CASES["iwl0"] = dict(B=37, D=60, V=90, W=8, fmt_w0=(0, 7))


@functools.lru_cache(maxsize=None)
def query_case(name):
    c = QUERY_CASES[name]
    rng = np.random.default_rng(_seed("query_" + name))
    extra = dict(en_pe=True, pe_dim_word=c["W"]) if c.get("en_pe") else {}
    fw0 = c.get("fmt_w0", (5, 2))
    cfg = make_cfg(c["V"], c["D"], 1, 2, fmt_w=[fw0], fmt=[(5, 2)], **extra)
    t_q = make_tables(rng, cfg, c.get("sigma", 0.4))[0][0]
    B, V, W = c["B"], c["V"], c["W"]
    words = np.full((B, W), EMPTY, np.uint16)
    for q in range(B):
        k = int(rng.integers(0, W + 1))
        words[q, :k] = rng.integers(0, V if q % 3 else min(V, 3), k)
        if q % 7 == 3 and k:
            words[q, 0] = V + 2                                           # out of range
        if q % 5 == 2 and k > 2:
            words[q, 1] = EMPTY                                           # a hole
    if c.get("repeat8"):
        words[::2] = (np.arange(B)[::2, None] % V).astype(np.uint16)      # one word in all 8 slots
    u0 = question_reference(cfg, words, t_q)
    for a in (words, t_q, u0):
        a.setflags(write=False)
    out = dict(c)
    out.update(name=name, cfg=cfg, Dp=pad_dim(c["D"]), words=words, t_q=t_q, u0=u0, u0_offset=c.get("u0_offset", 0))
    return out
