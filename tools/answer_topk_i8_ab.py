"""Runs ON THE GPU BOX: ranked answers of the int8 answer layer in one call against what a host had before, interleaved on one box.

  (A) qmann_answer_i8 with probs [n_query][V] of ANOTHER build of the library (the parent commit's, built into a second
      directory) followed by torch.topk(probs, k) -- the baseline is never the code under test;
  (B) qmann_answer_topk_i8 of this tree's library, the same k;
  (P) the parent build's plain one-pass qmann_answer_i8 (probs NULL, pred only): B - P is what the ranking costs;
  (F) qmann_answer_topk_f32 of this tree's library on the dequantised matrix: what the header advised until now.

    python3 tools/answer_topk_i8_ab.py --lib-a <parent build>/libqmann_hip.so [--lib-b <this build>] [--rounds 5] [--reps 10] [--k 5]

Shapes: 8 192 queries x V 4 096 x D 256 and 65 536 x V 238 x D 60 (Dp 64); w codes N(0, 6.4) on the Q1.6 grid (the float tool's
N(0, 0.1)), u on the Q5.2 grid, e^x softmax.
Every GPU step is a fresh child process under its own `timeout -k 10`; the script stops at the first step that ends abnormally.
First a check step for A and B, which leave their indices and probabilities in --tmp: on every row whose k probabilities of leg
A are pairwise distinct the indices must be equal (the last listed one may be tied with an unlisted answer: there the
probabilities must agree instead), every probability within rtol 1e-5 / atol 1e-7, and most rows must be such rows.  Then
`rounds` alternating rounds A, B, P, F; a child times `reps` calls between two HIP events after 3 warm-up calls.  Prints one JSON
line: per shape and leg the median over rounds and the spread (max - min) in ms, and whether leg B beats leg A by more than the
sum of the two spreads.  The children bind the library themselves (ctypes): the two builds do not export the same symbols."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile

SHAPES = {"q8192_v4096_d256": (8192, 4096, 256, 256), "q65536_v238_d60": (65536, 238, 60, 64)}     # n_query, V, D, Dp
FRAC_U, FRAC_W = 2, 6
LEGS = ("A", "B", "P", "F")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAG = "ANSWER_TOPK_I8_AB_CHILD "


class Fmt(C.Structure):
    _fields_ = [("iwl", C.c_uint32), ("frac", C.c_uint32)]


# (a copy of q-mann_amd/abi.py::Net -- that module cannot be imported against a build that lacks its newest symbols -- keep the two
# in step with include/qmann_batch.h::qmann_net)
class Net(C.Structure):
    _fields_ = [("n_hop", C.c_uint32), ("dim_emb", C.c_uint32), ("dim_emb_pad", C.c_uint32), ("dim_input", C.c_uint32),
                ("attention_mode", C.c_uint32), ("softmax_base", C.c_uint32), ("en_lin_map", C.c_uint32), ("num_bit", C.c_uint32),
                ("act", Fmt * 8), ("w", Fmt * 8), ("att", Fmt * 8), ("bin", Fmt), ("lin_map", C.c_void_p * 8),
                ("softmax_shift_based", C.c_uint32), ("en_att_scale", C.c_uint32), ("att_scale", C.c_float * 8),
                ("en_non_linearity", C.c_uint32), ("en_pe", C.c_uint32), ("pe_dim_word", C.c_uint32)]


def child(leg, lib_path, k, reps, tmp):
    import numpy as np
    import torch
    lib = C.CDLL(lib_path)
    vp, u32 = C.c_void_p, C.c_uint32
    lib.qmann_answer_i8.restype = C.c_int
    lib.qmann_answer_i8.argtypes = [C.POINTER(Net), vp, Fmt, vp, vp, vp, vp, vp, vp, vp, u32, vp]
    lib.qmann_answer_topk_f32.restype = C.c_int
    lib.qmann_answer_topk_f32.argtypes = [C.POINTER(Net), vp, vp, u32, vp, vp, u32, vp]
    if leg == "B":
        lib.qmann_answer_topk_i8_ws_bytes.restype = C.c_size_t
        lib.qmann_answer_topk_i8_ws_bytes.argtypes = [C.POINTER(Net), u32, u32]
        lib.qmann_answer_topk_i8.restype = C.c_int
        lib.qmann_answer_topk_i8.argtypes = [C.POINTER(Net), vp, Fmt, vp, vp, C.c_size_t, u32, vp, vp, u32, vp]
    dev = torch.device("cuda:0")
    p = lambda t: C.c_void_p(t.data_ptr())
    out = {}
    for name, (B, V, D, Dp) in SHAPES.items():
        rng = np.random.default_rng(0x1870B + V)
        cw = np.zeros((V, Dp), np.int8)
        cw[:, :D] = np.clip(np.rint(rng.normal(0, 6.4, (V, D))), -127, 127)
        w = torch.from_numpy(cw).to(dev)
        u = torch.from_numpy((np.clip(np.rint(rng.normal(0, 20.0, (B, D))), -127, 127) / (1 << FRAC_U)).astype(np.float32)).to(dev)
        net = Net()
        net.n_hop, net.dim_emb, net.dim_emb_pad, net.dim_input = 3, D, Dp, V
        net.attention_mode, net.softmax_base, net.en_lin_map, net.num_bit = 2, 0, 0, 8
        for h in range(3):
            net.act[h] = net.w[h] = net.att[h] = Fmt(7 - FRAC_U, FRAC_U)
        net.bin = Fmt(7 - FRAC_U, FRAC_U)
        wf = Fmt(7 - FRAC_W, FRAC_W)
        top_p = torch.empty((B, k), dtype=torch.float32, device=dev)
        top_i = torch.empty((B, k), dtype=torch.int64 if leg == "A" else torch.int32, device=dev)
        pred = torch.empty(B, dtype=torch.int32, device=dev)
        ws = None
        if leg in ("A", "P"):
            ws = torch.empty((B, V), dtype=torch.float32, device=dev)
            probs = torch.empty((B, V), dtype=torch.float32, device=dev) if leg == "A" else None

            def run():
                rc = lib.qmann_answer_i8(C.byref(net), p(w), wf, p(u), p(ws), None, p(pred), p(probs) if leg == "A" else None, None, None,
                                         B, None)
                if leg == "A":
                    torch.topk(probs, k, dim=1, out=(top_p, top_i))
                return rc
        elif leg == "B":
            need = lib.qmann_answer_topk_i8_ws_bytes(C.byref(net), k, B)
            ws = torch.empty(need, dtype=torch.uint8, device=dev)

            def run():
                return lib.qmann_answer_topk_i8(C.byref(net), p(w), wf, p(u), p(ws), need, k, p(top_i), p(top_p), B, None)
        else:
            wfl = torch.from_numpy((cw[:, :D].astype(np.float32) / (1 << FRAC_W))).to(dev).contiguous()

            def run():
                return lib.qmann_answer_topk_f32(C.byref(net), p(wfl), p(u), k, p(top_i), p(top_p), B, None)
        for _ in range(3):
            rc = run()
            assert rc == 0, (leg, name, rc)
        torch.cuda.synchronize()
        if tmp and leg in ("A", "B"):
            np.save(os.path.join(tmp, f"{leg}_{name}_idx.npy"), top_i.cpu().numpy().astype(np.int64))
            np.save(os.path.join(tmp, f"{leg}_{name}_p.npy"), top_p.cpu().numpy())
        ms = None
        if reps:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                run()
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / reps
        out[name] = dict(ms=ms)
        del w, u, ws
        torch.cuda.empty_cache()
    print(TAG + json.dumps(out), flush=True)


def step(leg, lib_path, a, reps, tmp=""):
    """one GPU step: a fresh child under its own time limit; any failure ends the script"""
    cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", leg, "--lib", lib_path,
           "--k", str(a.k), "--reps", str(reps), "--tmp", tmp]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    if r.returncode != 0:
        sys.exit(f"answer_topk_i8_ab: leg {leg} ended with status {r.returncode}; stopping")
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith(TAG)]
    if not lines:
        sys.exit(f"answer_topk_i8_ab: leg {leg} ended without a result line; stopping")
    print(f"answer_topk_i8_ab: leg {leg} done ({'check' if not reps else 'timed'})", file=sys.stderr, flush=True)
    return json.loads(lines[-1][len(TAG):])


def compare(tmp, k):
    """leg B's indices against leg A's; returns per shape the share of rows compared index by index"""
    import numpy as np
    share = {}
    for name in SHAPES:
        ia, ib = np.load(os.path.join(tmp, f"A_{name}_idx.npy")), np.load(os.path.join(tmp, f"B_{name}_idx.npy"))
        pa, pb = np.load(os.path.join(tmp, f"A_{name}_p.npy")), np.load(os.path.join(tmp, f"B_{name}_p.npy"))
        assert np.allclose(pb, pa, rtol=1e-5, atol=1e-7), f"{name}: probabilities differ"
        distinct = (np.diff(pa, axis=1) < 0).all(1) if k > 1 else np.ones(len(pa), bool)
        assert np.array_equal(ia[distinct, :k - 1], ib[distinct, :k - 1]), f"{name}: indices differ"
        # (the last listed answer: a different index is a tie with an unlisted answer -- the probabilities agree, checked above;
        # torch.topk's choice among them is its own)
        share[name] = float(distinct.mean())
        assert share[name] > 0.5, f"{name}: only {share[name]:.2f} of the rows have pairwise distinct probabilities"
    return share


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib-a"); ap.add_argument("--lib-b", default=os.path.join(ROOT, "q-mann_amd", "lib", "libqmann_hip.so"))
    ap.add_argument("--rounds", type=int, default=5); ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--k", type=int, default=5); ap.add_argument("--step-timeout", type=int, default=120)
    ap.add_argument("--child"); ap.add_argument("--lib"); ap.add_argument("--tmp", default="")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.lib, a.k, a.reps, a.tmp)
    if not a.lib_a:
        sys.exit("answer_topk_i8_ab: --lib-a <the parent commit's libqmann_hip.so> is required")
    if a.rounds < 5:
        print("answer_topk_i8_ab: fewer than 5 rounds: medians and spreads of this run are not to be quoted", file=sys.stderr)
    libs = {"A": a.lib_a, "B": a.lib_b, "P": a.lib_a, "F": a.lib_b}
    with tempfile.TemporaryDirectory() as tmp:
        step("A", a.lib_a, a, 0, tmp), step("B", a.lib_b, a, 0, tmp)
        share = compare(tmp, a.k)
    times = {}
    for _ in range(a.rounds):
        for leg in LEGS:
            for name, r in step(leg, libs[leg], a, a.reps).items():
                times.setdefault(name, {}).setdefault(leg, []).append(r["ms"])
    out = {"tool": "answer_topk_i8_ab", "k": a.k, "rounds": a.rounds, "reps": a.reps, "indices_equal": True, "shapes": {}}
    for name, tv in times.items():
        st = {leg: dict(median_ms=round(statistics.median(t), 4), spread_ms=round(max(t) - min(t), 4)) for leg, t in tv.items()}
        a_ms, b_ms = st["A"]["median_ms"], st["B"]["median_ms"]
        out["shapes"][name] = dict(st, rows_compared_by_index=round(share[name], 4), ratio_a_over_b=round(a_ms / b_ms, 3),
                                   b_beats_a_beyond_spreads=bool(a_ms - b_ms > st["A"]["spread_ms"] + st["B"]["spread_ms"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
