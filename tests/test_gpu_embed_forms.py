"""Every kernel form of the story embedding from word indices (csrc/batch_embed_idx.hip) and the question kernel, byte for byte
against the exact-integer numpy reference of embed_cases.py (pinned to the oracle without a GPU by test_embed_inputs.py).

For every case of embed_cases.CASES:
  form     qmann_embed_story_idx_form names the kernel form the case is meant to reach (after the case's switches are set);
  call     qmann_embed_story_idx with hop_stride = rows . Dp + 256; keys and vals are views inside buffers filled with 0xA5,
           256 guard bytes in front of plane 0, between the planes and behind the last one;
  planes   every plane equals the reference byte for byte -- raw bytes, no sign-magnitude decoding (0x80 is not 0x00), the zero
           columns D .. Dp-1 included;
  guards   every guard byte is still 0xA5 (the matrix-core kernels' rows leave through unpredicated buffer stores);
  witness  qmann_embed_story on the equivalent bag-of-words rows gives the same bytes (not for the many-rows cases, whose float
           rows would be 200 MB).
The many-rows cases hold rows = 16 . 48 . CUs + 37 rows, more tiles than any form's persistent grid takes at once, so that every
wavefront loops: the word prefetch one tile ahead, the rows kept back for the start of the next tile, the final flush.
Questions: qmann_embed_query_idx equals the reference bit for bit; the floats in front of and behind u0 are untouched.
No tolerance anywhere: the operation is exact integer arithmetic."""
import ctypes as C

import numpy as np
import pytest

import embed_cases as ec
from conftest import load_pkg
from embed_cases import CASES, QUERY_CASES, query_case, story_case

pytestmark = pytest.mark.gpu

GUARD = 256
FILL = 0xA5


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available()
    load_pkg()
    import qmann_amd.abi as abi
    import qmann_amd.model as model

    class Env:
        pass
    e = Env()
    e.torch, e.abi, e.model, e.dev = torch, abi, model, torch.device("cuda:0")
    e.cus = torch.cuda.get_device_properties(0).multi_processor_count
    return e


def set_switches(env, monkeypatch, switches):
    for k in ("QMANN_EMBED_VALU", "QMANN_EMBED_PER_HOP", "QMANN_EMBED_GENERAL_EPILOGUE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in switches.items():
        monkeypatch.setenv(k, v)
    env.abi.lib.qmann_tuning_reload()               # (conftest re-reads the restored environment after the test)


def guarded_planes(env, H, plane):
    """uint8 buffer of 0xA5: [guard][plane 0][guard][plane 1] ... [plane H-1][guard]; -> buffer, pointer of plane 0, hop stride"""
    stride = plane + GUARD
    buf = env.torch.full((GUARD + H * stride,), FILL, dtype=env.torch.uint8, device=env.dev)
    return buf, buf.data_ptr() + GUARD, stride


def check_planes(env, what, buf, H, rows, Dp, want):
    """want: uint8 device tensor [H][rows][Dp]"""
    torch = env.torch
    plane, stride = rows * Dp, rows * Dp + GUARD
    body = buf[GUARD:].view(H, stride)
    got = body[:, :plane].reshape(H, rows, Dp)
    if not torch.equal(got, want):
        bad = torch.nonzero(got != want)
        h, r, c = (int(x) for x in bad[0])
        raise AssertionError(f"{what}: {bad.shape[0]} bytes differ from the reference, first at hop {h} row {r} column {c}: "
                             f"got {int(got[h, r, c]):#04x}, want {int(want[h, r, c]):#04x}; rows hit: {torch.unique(bad[:, 1])[:12].tolist()}")
    guards = torch.cat([buf[:GUARD], body[:, plane:].reshape(-1)])
    hit = torch.nonzero(guards != FILL)
    assert hit.numel() == 0, f"{what}: {hit.shape[0]} guard bytes were overwritten, first at guard byte {int(hit[0])} (256 per guard, guard 0 in front of plane 0)"


@pytest.mark.parametrize("name", sorted(CASES))
def test_story_embedding_form(env, monkeypatch, name):
    torch, abi = env.torch, env.abi
    c = story_case(name)
    cfg, H, Dp, W, V = c["cfg"], c["H"], c["Dp"], c["W"], c["V"]
    set_switches(env, monkeypatch, c["env"])
    net = env.model._net_from_cfg(cfg)

    block = torch.from_numpy(c["words"].copy().view(np.int16)).to(env.dev)          # (the cases' arrays are shared and read-only)
    want_k, want_v = torch.from_numpy(c["keys"].copy()).to(env.dev), torch.from_numpy(c["vals"].copy()).to(env.dev)
    rows = ec.many_rows(env.cus) if c["many"] else c["rows"]
    if c["many"]:                                   # the 1 009-row block, repeated: the reference is computed once and tiled
        reps = -(-rows // ec.BLOCK_ROWS)
        block = block.repeat(reps, 1)[:rows]
        want_k, want_v = want_k.repeat(1, reps, 1)[:, :rows].contiguous(), want_v.repeat(1, reps, 1)[:, :rows].contiguous()
    # the word array inside a larger allocation, `offset` elements past an aligned address
    wbuf = torch.full((rows * W + 16,), -1, dtype=torch.int16, device=env.dev)
    off = 8 + c["offset"]
    wbuf[off:off + rows * W] = block.reshape(-1)
    words_ptr = wbuf.data_ptr() + 2 * off
    assert (words_ptr & 7) == (2 * c["offset"])

    t_a = [torch.from_numpy(c["t_a"][h].copy()).to(env.dev) for h in range(H)]
    t_c = [torch.from_numpy(c["t_c"][h].copy()).to(env.dev) for h in range(H)]
    ta, tc = (C.c_void_p * H)(*[t.data_ptr() for t in t_a]), (C.c_void_p * H)(*[t.data_ptr() for t in t_c])

    form = abi.lib.qmann_embed_story_idx_form(C.byref(net), C.c_void_p(words_ptr), W)
    assert form == c["form"], f"{name}: the call would take '{ec.FORM_NAMES.get(form, form)}', the case is meant for '{ec.FORM_NAMES[c['form']]}'"

    kbuf, kptr, stride = guarded_planes(env, H, rows * Dp)
    vbuf, vptr, _ = guarded_planes(env, H, rows * Dp)
    abi.check(abi.lib.qmann_embed_story_idx(C.byref(net), C.c_void_p(words_ptr), rows, W, c["time_last"], ta, tc, C.c_void_p(kptr),
                                            C.c_void_p(vptr), stride, None), "qmann_embed_story_idx")
    torch.cuda.synchronize()
    check_planes(env, f"{name} keys", kbuf, H, rows, Dp, want_k)
    check_planes(env, f"{name} vals", vbuf, H, rows, Dp, want_v)
    if c["many"]:
        return

    # third witness: the float bag-of-words kernels on the equivalent rows and the tables' grid values
    D = cfg["dim_emb"]
    story = torch.from_numpy(ec.words_to_bow(c["words"], V, c["time_last"])).to(env.dev)
    fl = lambda t, h: torch.from_numpy(np.ascontiguousarray((t[h][:, :D].astype(np.float32) / np.float32(1 << cfg["fmt_w"][h][1])).T)).to(env.dev)
    w_a, w_c = [fl(c["t_a"], h) for h in range(H)], [fl(c["t_c"], h) for h in range(H)]
    wa, wc = (C.c_void_p * H)(*[w.data_ptr() for w in w_a]), (C.c_void_p * H)(*[w.data_ptr() for w in w_c])
    kbuf2, kptr2, _ = guarded_planes(env, H, rows * Dp)
    vbuf2, vptr2, _ = guarded_planes(env, H, rows * Dp)
    abi.check(abi.lib.qmann_embed_story(C.byref(net), C.c_void_p(story.data_ptr()), rows, wa, wc, C.c_void_p(kptr2), C.c_void_p(vptr2),
                                        stride, None), "qmann_embed_story")
    torch.cuda.synchronize()
    check_planes(env, f"{name} keys (bag-of-words kernel)", kbuf2, H, rows, Dp, want_k)
    check_planes(env, f"{name} vals (bag-of-words kernel)", vbuf2, H, rows, Dp, want_v)


@pytest.mark.parametrize("name", sorted(QUERY_CASES))
def test_question_embedding(env, name):
    torch, abi = env.torch, env.abi
    c = query_case(name)
    cfg, B, D, W = c["cfg"], c["B"], c["cfg"]["dim_emb"], c["W"]
    net = env.model._net_from_cfg(cfg)
    words = torch.from_numpy(c["words"].copy().view(np.int16)).to(env.dev)
    t_q = torch.from_numpy(c["t_q"].copy()).to(env.dev)
    front = 4 + c["u0_offset"]                      # floats in front of u0: 16 bytes, plus the case's offset
    buf = torch.full((front + B * D + 8,), -1515870811, dtype=torch.int32, device=env.dev)       # 0xA5A5A5A5
    u0_ptr = buf.data_ptr() + 4 * front
    assert (u0_ptr & 15) == 4 * c["u0_offset"]
    abi.check(abi.lib.qmann_embed_query_idx(C.byref(net), C.c_void_p(words.data_ptr()), W, C.c_void_p(t_q.data_ptr()),
                                            C.c_void_p(u0_ptr), B, None), "qmann_embed_query_idx")
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    want = np.ascontiguousarray(c["u0"]).view(np.int32).reshape(-1)
    body = got[front:front + B * D]
    bad = np.flatnonzero(body != want)
    assert bad.size == 0, (f"{name}: {bad.size} of {B * D} floats differ bit for bit, first at query {bad[0] // D} column {bad[0] % D}: "
                           f"got {body[bad[0]:bad[0] + 1].view(np.float32)[0]}, want {want[bad[0]:bad[0] + 1].view(np.float32)[0]}")
    assert (got[:front] == -1515870811).all() and (got[front + B * D:] == -1515870811).all(), f"{name}: a float outside u0 was written"
