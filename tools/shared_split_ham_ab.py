"""Runs ON THE GPU BOX: the slot-split shared-plane Hamming hops on packed codes against the unsplit call, interleaved on one box.

  (A) qmann_hops_shared_packed with ANOTHER build of the library (the parent commit's, built into a second directory) -- the
      baseline is never the code under test;
  (B) qmann_hops_shared_split_packed, this tree's library, with the library's own slices ("auto") and 8, 32 and 128 forced.

    python3 tools/shared_split_ham_ab.py --lib-a <parent build>/libqmann_hip.so [--lib-b <this build>] [--rounds 5] [--reps 10]
                                         [--queries 1,8,64,1024,8192]

Shapes: "v0" 10 000 slots x 256 columns x 1 bit, Hamming V0, and "v1" 10 000 x 128 x 8 bits, Hamming V1; Q2.5, key / value /
query / linear-map codes N(0, 40), 3 hops, at every batch size of --queries; and per shape one row that has no leg A, "long"
(200 001 slots: beyond the LDS cap of the unsplit call), at the batch sizes of --long-queries.
Every GPU step is a fresh child process under its own `timeout -k 10`; the script stops at the first failing step.  First a
check step per leg: leg B's u_out must be bit-equal to leg A's (SHA-256 of the bytes) at every batch size and slicing.  Then
`rounds` alternating rounds A, B, A, B ...; a child times `reps` calls of each of its variants between two HIP events after 3
warm-up calls.  Prints one JSON line: per shape, batch size and variant the median over rounds and the spread (max - min) in ms,
the best leg-B variant, whether it beats leg A by more than the sum of the two spreads, and the slices "auto" took.
The children bind the library themselves (ctypes, the entry points they call only), so the two builds need not export the same
set of symbols."""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import subprocess
import sys

H, IWL, FRAC, SIGMA = 3, 2, 5, 40.0
SHAPES = {"v0": dict(mode=10, D=256, Dp=256, nb=1), "v1": dict(mode=11, D=128, Dp=128, nb=8)}
S_SHORT, S_LONG = 10000, 200001
SLICES = (0, 8, 32, 128)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAG = "SHARED_SPLIT_HAM_AB_CHILD "


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


def child(leg, lib_path, queries, long_queries, reps):
    import numpy as np
    import torch
    lib = C.CDLL(lib_path)
    vp, u32, sz = C.c_void_p, C.c_uint32, C.c_size_t
    lib.qmann_pack_bitplanes.restype = C.c_int
    lib.qmann_pack_bitplanes.argtypes = [vp, vp, sz, u32, u32, vp]
    lib.qmann_hops_shared_packed.restype = C.c_int
    lib.qmann_hops_shared_packed.argtypes = [C.POINTER(Net), vp, sz, vp, sz, u32, vp, vp, vp, u32, vp]
    if leg == "B":
        lib.qmann_hops_shared_split_packed.restype = C.c_int
        lib.qmann_hops_shared_split_packed.argtypes = [C.POINTER(Net), vp, sz, vp, sz, u32, vp, vp, vp, u32, u32, vp, sz, vp]
        lib.qmann_hops_shared_split_packed_ws_bytes.restype = sz
        lib.qmann_hops_shared_split_packed_ws_bytes.argtypes = [C.POINTER(Net), u32, u32]
        lib.qmann_hops_shared_split_packed_slices.restype = u32
        lib.qmann_hops_shared_split_packed_slices.argtypes = [C.POINTER(Net), u32, u32]
    dev = torch.device("cuda:0")
    out = {}

    def signmag(c):
        c = c.astype(np.int16)
        return np.where(c < 0, (-c) | 0x80, c).astype(np.uint8).view(np.int8)
    p = lambda t: C.c_void_p(t.data_ptr())
    for sname, sh in SHAPES.items():
        D, Dp, nb = sh["D"], sh["Dp"], sh["nb"]
        rows = [(sname, S_SHORT, queries)] + ([(sname + "_long", S_LONG, long_queries)] if leg == "B" and long_queries else [])
        for row, S, nqs in rows:
            rng = np.random.default_rng(0x4A3ED + S + nb)
            codes = lambda *shape: np.clip(np.rint(rng.normal(0, SIGMA, shape)), -127, 127)
            plane = lambda: np.pad(codes(H, S, D), ((0, 0), (0, 0), (0, Dp - D)))
            key_bytes = torch.from_numpy(signmag(plane())).to(dev)
            planes = torch.empty((H, S, Dp // 64, nb), dtype=torch.int64, device=dev)
            assert lib.qmann_pack_bitplanes(p(key_bytes), p(planes), H * S, Dp, nb, None) == 0
            torch.cuda.synchronize()
            del key_bytes
            vals = torch.from_numpy(signmag(plane())).to(dev)
            lin = [torch.from_numpy(signmag(np.pad(codes(D, D), ((0, 0), (0, Dp - D))))).to(dev) for _ in range(H)]
            u0_all = torch.from_numpy((codes(max(nqs), D) / (1 << FRAC)).astype(np.float32)).to(dev)
            net = Net()
            net.n_hop, net.dim_emb, net.dim_emb_pad, net.dim_input = H, D, Dp, 256
            net.attention_mode, net.softmax_base, net.en_lin_map, net.num_bit = sh["mode"], 0, 1, nb
            for h in range(H):
                net.act[h] = net.w[h] = net.att[h] = Fmt(IWL, FRAC)
                net.lin_map[h] = lin[h].data_ptr()
            net.bin = Fmt(IWL, FRAC)
            ks, vs = S * (Dp // 64) * nb * 8, S * Dp
            for B in nqs:
                u0 = u0_all[:B].contiguous()
                u_out = torch.empty_like(u0)
                variants = {}
                if leg == "A":
                    variants["A"] = lambda: lib.qmann_hops_shared_packed(C.byref(net), p(planes), ks, p(vals), vs, S, p(u0), p(u_out), None, B, None)
                else:
                    nbytes = lib.qmann_hops_shared_split_packed_ws_bytes(C.byref(net), S, B)
                    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
                    for ns in SLICES:
                        variants["B_auto" if ns == 0 else f"B_s{ns}"] = (
                            lambda ns=ns: lib.qmann_hops_shared_split_packed(C.byref(net), p(planes), ks, p(vals), vs, S, p(u0), p(u_out),
                                                                             None, B, ns, p(ws), nbytes, None))
                res = {}
                for vname, run in variants.items():
                    u_out.fill_(float("nan"))
                    for _ in range(3):
                        rc = run()
                        assert rc == 0, (row, B, vname, rc)
                    torch.cuda.synchronize()
                    digest = hashlib.sha256(u_out.cpu().numpy().tobytes()).hexdigest()
                    ms = None
                    if reps:
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(reps):
                            run()
                        e1.record()
                        torch.cuda.synchronize()
                        ms = e0.elapsed_time(e1) / reps
                    res[vname] = dict(ms=ms, sha=digest)
                if leg == "B":
                    res["B_auto"]["slices"] = int(lib.qmann_hops_shared_split_packed_slices(C.byref(net), S, B))
                out[f"{row}_q{B}"] = res
            del planes, vals
            torch.cuda.empty_cache()
    print(TAG + json.dumps(out), flush=True)


def step(leg, lib_path, a, reps):
    """one GPU step: a fresh child under its own time limit; any failure ends the script"""
    cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", leg, "--lib", lib_path,
           "--queries", a.queries, "--long-queries", a.long_queries, "--reps", str(reps)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    if r.returncode != 0:
        sys.exit(f"shared_split_ham_ab: leg {leg} ended with status {r.returncode}; stopping")
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith(TAG)]
    if not lines:
        sys.exit(f"shared_split_ham_ab: leg {leg} ended without a result line; stopping")
    print(f"shared_split_ham_ab: leg {leg} done ({'check' if not reps else 'timed'})", file=sys.stderr, flush=True)
    return json.loads(lines[-1][len(TAG):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib-a"); ap.add_argument("--lib-b", default=os.path.join(ROOT, "q-mann_amd", "lib", "libqmann_hip.so"))
    ap.add_argument("--rounds", type=int, default=5); ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--queries", default="1,8,64,1024,8192"); ap.add_argument("--long-queries", default="1,64")
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--child"); ap.add_argument("--lib")
    a = ap.parse_args()
    ints = lambda s: [int(x) for x in s.split(",") if x]
    if a.child:
        return child(a.child, a.lib, ints(a.queries), ints(a.long_queries), a.reps)
    if not a.lib_a:
        sys.exit("shared_split_ham_ab: --lib-a <the parent commit's libqmann_hip.so> is required")
    if a.rounds < 5:
        print("shared_split_ham_ab: fewer than 5 rounds: medians and spreads of this run are not to be quoted", file=sys.stderr)
    # results first: every variant of leg B must give leg A's bytes (the long rows have no leg A: their variants must agree)
    ca, cb = step("A", a.lib_a, a, 0), step("B", a.lib_b, a, 0)
    for cell, res in cb.items():
        want = ca[cell]["A"]["sha"] if cell in ca else res["B_s8"]["sha"]
        for v, r in res.items():
            assert r["sha"] == want, f"{cell}: u_out of {v} differs from {'leg A' if cell in ca else 'B_s8'}'s"
    times, last_b = {}, None
    for _ in range(a.rounds):
        for leg, lib in (("A", a.lib_a), ("B", a.lib_b)):
            got = step(leg, lib, a, a.reps)
            if leg == "B":
                last_b = got
            for cell, res in got.items():
                for v, r in res.items():
                    times.setdefault(cell, {}).setdefault(v, []).append(r["ms"])
    out = {"tool": "shared_split_ham_ab", "rounds": a.rounds, "reps": a.reps, "u_out_bit_equal": True, "cells": {}}
    for cell, tv in times.items():
        st = {v: dict(median_ms=round(statistics.median(t), 4), spread_ms=round(max(t) - min(t), 4)) for v, t in tv.items()}
        st["B_auto"]["slices"] = last_b[cell]["B_auto"]["slices"]
        legb = {v: r for v, r in st.items() if v.startswith("B_")}
        best = min(legb, key=lambda v: legb[v]["median_ms"])
        o = dict(variants=st, best_b=best)
        if "A" in st:
            a_ms, b_ms = st["A"]["median_ms"], legb[best]["median_ms"]
            o["ratio_a_over_best_b"] = round(a_ms / b_ms, 3)
            o["b_beats_a_beyond_spreads"] = bool(a_ms - b_ms > st["A"]["spread_ms"] + legb[best]["spread_ms"])
            o["auto_beats_a_beyond_spreads"] = bool(a_ms - st["B_auto"]["median_ms"] > st["A"]["spread_ms"] + st["B_auto"]["spread_ms"])
        out["cells"][cell] = o
    print(json.dumps(out))


if __name__ == "__main__":
    main()
