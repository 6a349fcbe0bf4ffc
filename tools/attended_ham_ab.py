"""Runs ON THE GPU BOX: attended slots of the packed Hamming forms in one call against "the probs tap, then sort", interleaved on
one box.  The sibling of tools/attended_ab.py, with the same discipline.

  (A) the packed hop call with only taps.probs set, of ANOTHER build of the library (the parent commit's, built into a second
      directory), followed by torch.topk over the slot axis -- what a host did before; the baseline is never the code under test.
      For V1 a set tap also turns the kernel's threshold shortcut off: that is part of what leg A costs;
  (B) the hop call's _top_packed form of this tree's library, the same k;
  (P) the parent build's plain packed hop call, no taps: B / P is the price of the selection stage.

    python3 tools/attended_ham_ab.py --lib-a <parent build>/libqmann_hip.so [--lib-b <this build>] [--rounds 5] [--reps 10] [--k 5]

Shapes (tools/shared_ham_ab.py's draw: Q5.2, key / value / query / linear-map codes N(0, 40), 3 hops, e^x softmax):
8 192 queries x 10 000 slots x D 256 with V0 on one bit and with V1 on eight (BASELINE config 5), 8 192 x 1 000 x D 60 with V1
on eight bits, all on qmann_hops_shared_packed / qmann_hops_shared_top_packed; 64 x 90 001 x D 128, V0 on one bit, on
qmann_hops_shared_split_packed / qmann_hops_shared_split_top_packed (the library's own slices).
Every GPU step is a fresh child process under its own `timeout -k 10`; the script stops at the first failing step.  First a
check step per leg: leg B's top_p, sorted, must be bit-equal to the k largest values of leg A's probs (SHA-256 of the bytes; the
indices are not compared -- torch.topk's order among equal probabilities is its own), and u_out bit-equal over all three legs.
Then `rounds` alternating rounds A, B, P, A, B, P ...; a child times `reps` calls between two HIP events after 3 warm-up calls.
Prints one JSON line: per shape and leg the median over rounds and the spread (max - min) in ms, A / B, B / P, and whether each
difference exceeds the sum of the two spreads.
The children bind the library themselves (ctypes), so the two builds need not export the same set of symbols."""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import subprocess
import sys

H, IWL, FRAC, SIGMA = 3, 5, 2, 40.0
SHAPES = {"q8192_s10000_d256_v0_b1": dict(B=8192, S=10000, D=256, Dp=256, nb=1, mode=10, split=False),
          "q8192_s10000_d256_v1_b8": dict(B=8192, S=10000, D=256, Dp=256, nb=8, mode=11, split=False),
          "q8192_s1000_d60_v1_b8": dict(B=8192, S=1000, D=60, Dp=64, nb=8, mode=11, split=False),
          "split_q64_s90001_d128_v0_b1": dict(B=64, S=90001, D=128, Dp=128, nb=1, mode=10, split=True)}
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


class Taps(C.Structure):
    _fields_ = [("score_codes", C.c_void_p), ("scores", C.c_void_p), ("probs", C.c_void_p), ("o", C.c_void_p), ("u", C.c_void_p)]


def child(leg, lib_path, k, reps):
    import numpy as np
    import torch
    lib = C.CDLL(lib_path)
    vp, u32, sz = C.c_void_p, C.c_uint32, C.c_size_t
    lib.qmann_pack_bitplanes.restype = C.c_int
    lib.qmann_pack_bitplanes.argtypes = [vp, vp, sz, u32, u32, vp]
    lib.qmann_hops_shared_split_packed_ws_bytes.restype = sz
    lib.qmann_hops_shared_split_packed_ws_bytes.argtypes = [C.POINTER(Net), u32, u32]
    if leg == "B":
        lib.qmann_hops_shared_top_packed.restype = C.c_int
        lib.qmann_hops_shared_top_packed.argtypes = [C.POINTER(Net), vp, sz, vp, sz, u32, vp, vp, u32, vp, vp, u32, vp]
        lib.qmann_hops_shared_split_top_packed.restype = C.c_int
        lib.qmann_hops_shared_split_top_packed.argtypes = [C.POINTER(Net), vp, sz, vp, sz, u32, vp, vp, u32, vp, vp, u32, u32, vp, sz, vp]
    else:
        lib.qmann_hops_shared_packed.restype = C.c_int
        lib.qmann_hops_shared_packed.argtypes = [C.POINTER(Net), vp, sz, vp, sz, u32, vp, vp, vp, u32, vp]
        lib.qmann_hops_shared_split_packed.restype = C.c_int
        lib.qmann_hops_shared_split_packed.argtypes = [C.POINTER(Net), vp, sz, vp, sz, u32, vp, vp, vp, u32, u32, vp, sz, vp]
    dev = torch.device("cuda:0")
    out = {}

    def signmag(c):
        c = c.astype(np.int16)
        return np.where(c < 0, (-c) | 0x80, c).astype(np.uint8).view(np.int8)
    p = lambda t: C.c_void_p(t.data_ptr())
    for name, sh in SHAPES.items():
        B, S, D, Dp, nb, split = sh["B"], sh["S"], sh["D"], sh["Dp"], sh["nb"], sh["split"]
        G = Dp // 64
        rng = np.random.default_rng(0xA77E + S + nb)
        codes = lambda *shape: np.clip(np.rint(rng.normal(0, SIGMA, shape)), -127, 127)
        plane = lambda: np.pad(codes(H, S, D), ((0, 0), (0, 0), (0, Dp - D)))
        key_bytes = torch.from_numpy(signmag(plane())).to(dev)
        keys = torch.empty((H, S, G, nb), dtype=torch.int64, device=dev)
        assert lib.qmann_pack_bitplanes(p(key_bytes), p(keys), H * S, Dp, nb, None) == 0
        del key_bytes
        vals = torch.from_numpy(signmag(plane())).to(dev)
        lin = [torch.from_numpy(signmag(np.pad(codes(D, D), ((0, 0), (0, Dp - D))))).to(dev) for _ in range(H)]
        u0 = torch.from_numpy((codes(B, D) / (1 << FRAC)).astype(np.float32)).to(dev)
        u_out = torch.empty_like(u0)
        net = Net()
        net.n_hop, net.dim_emb, net.dim_emb_pad, net.dim_input = H, D, Dp, 256
        net.attention_mode, net.softmax_base, net.en_lin_map, net.num_bit = sh["mode"], 0, 1, nb
        for h in range(H):
            net.act[h] = net.w[h] = net.att[h] = Fmt(IWL, FRAC)
            net.lin_map[h] = lin[h].data_ptr()
        net.bin = Fmt(IWL, FRAC)
        nbytes = lib.qmann_hops_shared_split_packed_ws_bytes(C.byref(net), S, B) if split else 0
        ks, vs = S * G * nb * 8, S * Dp
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
        top_p = torch.empty((B, H, k), dtype=torch.float32, device=dev)
        if leg == "B":
            top_i = torch.empty((B, H, k), dtype=torch.int32, device=dev)

            def run():
                if split:
                    return lib.qmann_hops_shared_split_top_packed(C.byref(net), p(keys), ks, p(vals), vs, S, p(u0), p(u_out), k, p(top_i),
                                                                  p(top_p), B, 0, p(ws), nbytes, None)
                return lib.qmann_hops_shared_top_packed(C.byref(net), p(keys), ks, p(vals), vs, S, p(u0), p(u_out), k, p(top_i), p(top_p), B, None)
        else:
            taps = None
            if leg == "A":
                probs = torch.empty((H, B, S), dtype=torch.float32, device=dev)
                tk_p = torch.empty((H, B, k), dtype=torch.float32, device=dev)
                tk_i = torch.empty((H, B, k), dtype=torch.int64, device=dev)
                taps = Taps(None, None, probs.data_ptr(), None, None)
            tref = C.byref(taps) if taps is not None else None

            def run():
                if split:
                    rc = lib.qmann_hops_shared_split_packed(C.byref(net), p(keys), ks, p(vals), vs, S, p(u0), p(u_out), tref, B, 0, p(ws), nbytes, None)
                else:
                    rc = lib.qmann_hops_shared_packed(C.byref(net), p(keys), ks, p(vals), vs, S, p(u0), p(u_out), tref, B, None)
                if leg == "A":
                    torch.topk(probs, k, dim=2, out=(tk_p, tk_i))
                return rc
        u_out.fill_(float("nan"))
        for _ in range(3):
            rc = run()
            assert rc == 0, (leg, name, rc)
        torch.cuda.synchronize()
        res = dict(ms=None, sha_u=hashlib.sha256(u_out.cpu().numpy().tobytes()).hexdigest())
        if leg != "P":
            rows = top_p if leg == "B" else tk_p.permute(1, 0, 2).contiguous()                  # -> [B][H][k]
            rows = torch.sort(rows, dim=2, descending=True).values
            res["sha_p"] = hashlib.sha256(rows.cpu().numpy().tobytes()).hexdigest()
        if reps:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                run()
            e1.record()
            torch.cuda.synchronize()
            res["ms"] = e0.elapsed_time(e1) / reps
        out[name] = res
        if leg == "A":
            del probs
        del keys, vals, ws
        torch.cuda.empty_cache()
    print("ATTENDED_HAM_AB_CHILD " + json.dumps(out), flush=True)


def step(leg, lib_path, a, reps):
    """one GPU step: a fresh child under its own time limit; any failure ends the script"""
    cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", leg, "--lib", lib_path,
           "--k", str(a.k), "--reps", str(reps)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    if r.returncode != 0:
        sys.exit(f"attended_ham_ab: leg {leg} ended with status {r.returncode}; stopping")
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("ATTENDED_HAM_AB_CHILD ")]
    if not lines:
        sys.exit(f"attended_ham_ab: leg {leg} ended without a result line; stopping")
    print(f"attended_ham_ab: leg {leg} done ({'check' if not reps else 'timed'})", file=sys.stderr, flush=True)
    return json.loads(lines[-1][len("ATTENDED_HAM_AB_CHILD "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib-a"); ap.add_argument("--lib-b", default=os.path.join(ROOT, "q-mann_amd", "lib", "libqmann_hip.so"))
    ap.add_argument("--rounds", type=int, default=5); ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--k", type=int, default=5); ap.add_argument("--step-timeout", type=int, default=180)
    ap.add_argument("--child"); ap.add_argument("--lib")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.lib, a.k, a.reps)
    if not a.lib_a:
        sys.exit("attended_ham_ab: --lib-a <the parent commit's libqmann_hip.so> is required")
    if a.rounds < 5:
        print("attended_ham_ab: fewer than 5 rounds: medians and spreads of this run are not to be quoted", file=sys.stderr)
    legs = (("A", a.lib_a), ("B", a.lib_b), ("P", a.lib_a))
    chk = {leg: step(leg, lib, a, 0) for leg, lib in legs}
    for name in SHAPES:
        assert chk["A"][name]["sha_p"] == chk["B"][name]["sha_p"], f"{name}: leg B's top_p differ from the k largest of leg A's probs"
        assert chk["A"][name]["sha_u"] == chk["B"][name]["sha_u"] == chk["P"][name]["sha_u"], f"{name}: u_out differs between the legs"
    times = {}
    for _ in range(a.rounds):
        for leg, lib in legs:
            for name, r in step(leg, lib, a, a.reps).items():
                times.setdefault(name, {}).setdefault(leg, []).append(r["ms"])
    out = {"tool": "attended_ham_ab", "k": a.k, "rounds": a.rounds, "reps": a.reps, "top_p_bit_equal": True, "u_out_bit_equal": True,
           "shapes": {}}
    for name, tv in times.items():
        st = {leg: dict(median_ms=round(statistics.median(t), 4), spread_ms=round(max(t) - min(t), 4)) for leg, t in tv.items()}
        ms = {leg: st[leg]["median_ms"] for leg in st}
        sp = {leg: st[leg]["spread_ms"] for leg in st}
        out["shapes"][name] = dict(st, ratio_a_over_b=round(ms["A"] / ms["B"], 3), ratio_b_over_p=round(ms["B"] / ms["P"], 3),
                                   b_beats_a_beyond_spreads=bool(ms["A"] - ms["B"] > sp["A"] + sp["B"]),
                                   b_above_p_beyond_spreads=bool(ms["B"] - ms["P"] > sp["B"] + sp["P"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
