"""Runs ON THE GPU BOX: ranked answers in one call against "all probabilities, then sort", interleaved on one box.

  (A) qmann_answer_f32_serial with probs [n_query][V] of ANOTHER build of the library (the parent commit's, built into a second
      directory) followed by torch.topk(probs, k) -- what a host did before; the baseline is never the code under test;
  (B) qmann_answer_topk_f32 of this tree's library, the same k.

    python3 tools/answer_topk_ab.py --lib-a <parent build>/libqmann_hip.so [--lib-b <this build>] [--rounds 5] [--reps 10] [--k 5]

Shapes: 8 192 queries x V 4 096 x D 256 (one workgroup per query) and 65 536 x V 238 x D 60 (the lane-group kernel); w_ans
N(0, 0.1), u on the Q5.2 grid, e^x softmax.
Every GPU step is a fresh child process under its own `timeout -k 10`; the script stops at the first failing step.  First a
check step per leg: leg B's probabilities must be bit-equal to the values leg A's torch.topk picked (SHA-256 of the bytes; the
indices are not compared -- torch.topk's order among equal probabilities is its own).  Then `rounds` alternating rounds A, B,
A, B ...; a child times `reps` calls between two HIP events after 3 warm-up calls.  Prints one JSON line: per shape and leg the
median over rounds and the spread (max - min) in ms, and whether leg B beats leg A by more than the sum of the two spreads.
The children bind the library themselves (ctypes), so the two builds need not export the same set of symbols."""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import subprocess
import sys

SHAPES = {"q8192_v4096_d256": (8192, 4096, 256, 256), "q65536_v238_d60": (65536, 238, 60, 64)}     # n_query, V, D, Dp
FRAC = 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def child(leg, lib_path, k, reps):
    import numpy as np
    import torch
    lib = C.CDLL(lib_path)
    vp, u32 = C.c_void_p, C.c_uint32
    if leg == "A":
        lib.qmann_answer_f32_serial.restype = C.c_int
        lib.qmann_answer_f32_serial.argtypes = [C.POINTER(Net), vp, vp, vp, vp, vp, vp, vp, u32, vp]
    else:
        lib.qmann_answer_topk_f32.restype = C.c_int
        lib.qmann_answer_topk_f32.argtypes = [C.POINTER(Net), vp, vp, u32, vp, vp, u32, vp]
    dev = torch.device("cuda:0")
    p = lambda t: C.c_void_p(t.data_ptr())
    out = {}
    for name, (B, V, D, Dp) in SHAPES.items():
        rng = np.random.default_rng(0x70B + V)
        w = torch.from_numpy(rng.normal(0, 0.1, (V, D)).astype(np.float32)).to(dev)
        u = torch.from_numpy((np.clip(np.rint(rng.normal(0, 20.0, (B, D))), -127, 127) / (1 << FRAC)).astype(np.float32)).to(dev)
        net = Net()
        net.n_hop, net.dim_emb, net.dim_emb_pad, net.dim_input = 3, D, Dp, V
        net.attention_mode, net.softmax_base, net.en_lin_map, net.num_bit = 2, 0, 0, 8
        for h in range(3):
            net.act[h] = net.w[h] = net.att[h] = Fmt(7 - FRAC, FRAC)
        net.bin = Fmt(7 - FRAC, FRAC)
        top_p = torch.empty((B, k), dtype=torch.float32, device=dev)
        if leg == "A":
            pred = torch.empty(B, dtype=torch.int32, device=dev)
            probs = torch.empty((B, V), dtype=torch.float32, device=dev)
            top_i = torch.empty((B, k), dtype=torch.int64, device=dev)

            def run():
                rc = lib.qmann_answer_f32_serial(C.byref(net), p(w), p(u), None, p(pred), p(probs), None, None, B, None)
                torch.topk(probs, k, dim=1, out=(top_p, top_i))
                return rc
        else:
            top_i = torch.empty((B, k), dtype=torch.int32, device=dev)

            def run():
                return lib.qmann_answer_topk_f32(C.byref(net), p(w), p(u), k, p(top_i), p(top_p), B, None)
        top_p.fill_(float("nan"))
        for _ in range(3):
            rc = run()
            assert rc == 0, (leg, name, rc)
        torch.cuda.synchronize()
        digest = hashlib.sha256(top_p.cpu().numpy().tobytes()).hexdigest()
        ms = None
        if reps:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                run()
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / reps
        out[name] = dict(ms=ms, sha=digest)
        del w, u
        torch.cuda.empty_cache()
    print("ANSWER_TOPK_AB_CHILD " + json.dumps(out), flush=True)


def step(leg, lib_path, a, reps):
    """one GPU step: a fresh child under its own time limit; any failure ends the script"""
    cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", leg, "--lib", lib_path,
           "--k", str(a.k), "--reps", str(reps)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    if r.returncode != 0:
        sys.exit(f"answer_topk_ab: leg {leg} ended with status {r.returncode}; stopping")
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("ANSWER_TOPK_AB_CHILD ")]
    if not lines:
        sys.exit(f"answer_topk_ab: leg {leg} ended without a result line; stopping")
    print(f"answer_topk_ab: leg {leg} done ({'check' if not reps else 'timed'})", file=sys.stderr, flush=True)
    return json.loads(lines[-1][len("ANSWER_TOPK_AB_CHILD "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib-a"); ap.add_argument("--lib-b", default=os.path.join(ROOT, "q-mann_amd", "lib", "libqmann_hip.so"))
    ap.add_argument("--rounds", type=int, default=5); ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--k", type=int, default=5); ap.add_argument("--step-timeout", type=int, default=120)
    ap.add_argument("--child"); ap.add_argument("--lib")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.lib, a.k, a.reps)
    if not a.lib_a:
        sys.exit("answer_topk_ab: --lib-a <the parent commit's libqmann_hip.so> is required")
    if a.rounds < 5:
        print("answer_topk_ab: fewer than 5 rounds: medians and spreads of this run are not to be quoted", file=sys.stderr)
    ca, cb = step("A", a.lib_a, a, 0), step("B", a.lib_b, a, 0)
    for name in SHAPES:
        assert ca[name]["sha"] == cb[name]["sha"], f"{name}: leg B's probabilities differ from the ones torch.topk picked from leg A's"
    times = {}
    for _ in range(a.rounds):
        for leg, lib in (("A", a.lib_a), ("B", a.lib_b)):
            for name, r in step(leg, lib, a, a.reps).items():
                times.setdefault(name, {}).setdefault(leg, []).append(r["ms"])
    out = {"tool": "answer_topk_ab", "k": a.k, "rounds": a.rounds, "reps": a.reps, "top_p_bit_equal": True, "shapes": {}}
    for name, tv in times.items():
        st = {leg: dict(median_ms=round(statistics.median(t), 4), spread_ms=round(max(t) - min(t), 4)) for leg, t in tv.items()}
        a_ms, b_ms = st["A"]["median_ms"], st["B"]["median_ms"]
        out["shapes"][name] = dict(st, ratio_a_over_b=round(a_ms / b_ms, 3),
                                   b_beats_a_beyond_spreads=bool(a_ms - b_ms > st["A"]["spread_ms"] + st["B"]["spread_ms"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
