"""Runs ON THE GPU BOX: attended slots per story in one call against "the probs tap, then sort", interleaved on one box.

  (A) qmann_hops_i8 with only taps.probs set, of ANOTHER build of the library (the parent commit's, built into a second
      directory), followed by torch.topk over the slot axis of the [n_hop][n_query][S] view of the tap -- what a host did before;
      the baseline is never the code under test;
  (B) qmann_hops_top_i8 of this tree's library, the same k;
  (P) the parent build's plain qmann_hops_i8, no taps: B / P is the price of the one-wavefront (or streaming) kernel plus the
      selection against the kernels a plain call runs (quad / lean up to 64 slots).

    python3 tools/attended_story_ab.py --lib-a <parent build>/libqmann_hip.so [--lib-b <this build>] [--rounds 5] [--reps 10] [--k 5]

Shapes: bench.py's babi_mem50 (262 144 stories x 50 rows, D 60, fixed-point Q5.2), babi_joint_v1 (the same batch, Hamming V1 on
8 bits) and synth10k_d128_q25 (8 192 x 10 000, D 128, Q2.5), with that workload's code spreads (key / value / query sigmas; the
linear maps N(0, 1) on the weight grid, N(0, 6) codes for the Q2.5 shape), 3 hops, e^x softmax, memories drawn on the device.
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

H = 3
SHAPES = {"babi_mem50": dict(B=262144, S=50, D=60, Dp=64, mode=2, iwl=5, sk=8.0, sv=30.0, su=8.0, wh=4.0),
          "babi_joint_v1": dict(B=262144, S=50, D=60, Dp=64, mode=11, iwl=5, sk=30.0, sv=30.0, su=30.0, wh=4.0),
          "synth10k_d128_q25": dict(B=8192, S=10000, D=128, Dp=128, mode=2, iwl=2, sk=6.0, sv=6.0, su=6.0, wh=6.0)}
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


def child(leg, lib_path, k, reps, only):
    import torch
    lib = C.CDLL(lib_path)
    vp, u32, sz = C.c_void_p, C.c_uint32, C.c_size_t
    if leg == "B":
        lib.qmann_hops_top_i8.restype = C.c_int
        lib.qmann_hops_top_i8.argtypes = [C.POINTER(Net), vp, vp, sz, vp, u32, vp, vp, u32, vp, vp, u32, vp]
    else:
        lib.qmann_hops_i8.restype = C.c_int
        lib.qmann_hops_i8.argtypes = [C.POINTER(Net), vp, vp, sz, vp, u32, vp, vp, vp, u32, vp]
    dev = torch.device("cuda:0")
    out = {}
    p = lambda t: C.c_void_p(t.data_ptr())

    def gauss_i8(shape, sigma, gen, pad_from):
        """sign-magnitude int8 codes of clip(round(N(0, sigma)), +-127), drawn on the device in chunks (bench.py::gauss_i8)"""
        t = torch.empty(shape, dtype=torch.int8, device=dev)
        flat = t.view(-1)
        for a in range(0, flat.numel(), 1 << 28):
            b = min(flat.numel(), a + (1 << 28))
            c = torch.randn(b - a, device=dev, generator=gen, dtype=torch.float32).mul_(sigma).round_().clamp_(-127, 127).to(torch.int8)
            flat[a:b] = torch.where(c < 0, (-c) | -128, c)
        if pad_from < shape[-1]:
            t[..., pad_from:] = 0
        return t
    for name, sh in SHAPES.items():
        if only and name not in only:
            continue
        B, S, D, Dp, frac = sh["B"], sh["S"], sh["D"], sh["Dp"], 7 - sh["iwl"]
        gen = torch.Generator(device=dev)
        gen.manual_seed(0x51A44 + S)
        keys = gauss_i8((H, B * S, Dp), sh["sk"], gen, D)
        vals = gauss_i8((H, B * S, Dp), sh["sv"], gen, D)
        lin = [gauss_i8((D, Dp), sh["wh"], gen, D) for _ in range(H)]
        u0 = (torch.randn((B, D), device=dev, generator=gen) * sh["su"]).round_().clamp_(-127, 127) / float(1 << frac)
        row_off = (torch.arange(B + 1, device=dev, dtype=torch.int64) * S).to(torch.int32)
        u_out = torch.empty_like(u0)
        net = Net()
        net.n_hop, net.dim_emb, net.dim_emb_pad, net.dim_input = H, D, Dp, 256
        net.attention_mode, net.softmax_base, net.en_lin_map, net.num_bit = sh["mode"], 0, 1, 8
        for h in range(H):
            net.act[h] = net.w[h] = net.att[h] = Fmt(sh["iwl"], frac)
            net.lin_map[h] = lin[h].data_ptr()
        net.bin = Fmt(sh["iwl"], frac)
        stride = B * S * Dp
        if leg == "B":
            top_p = torch.empty((B, H, k), dtype=torch.float32, device=dev)
            top_i = torch.empty((B, H, k), dtype=torch.int32, device=dev)

            def run():
                return lib.qmann_hops_top_i8(C.byref(net), p(keys), p(vals), stride, p(row_off), S, p(u0), p(u_out), k, p(top_i), p(top_p), B, None)
        else:
            taps = None
            if leg == "A":
                probs = torch.empty((H, B, S), dtype=torch.float32, device=dev)
                tk_p = torch.empty((H, B, k), dtype=torch.float32, device=dev)
                tk_i = torch.empty((H, B, k), dtype=torch.int64, device=dev)
                taps = Taps(None, None, probs.data_ptr(), None, None)
            tref = C.byref(taps) if taps is not None else None

            def run():
                rc = lib.qmann_hops_i8(C.byref(net), p(keys), p(vals), stride, p(row_off), S, p(u0), p(u_out), tref, B, None)
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
        del keys, vals
        torch.cuda.empty_cache()
    print("ATTENDED_STORY_AB_CHILD " + json.dumps(out), flush=True)


def step(leg, lib_path, a, reps):
    """one GPU step: a fresh child under its own time limit; any failure ends the script"""
    cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", leg, "--lib", lib_path,
           "--k", str(a.k), "--reps", str(reps)] + (["--shapes", a.shapes] if a.shapes else [])
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    if r.returncode != 0:
        sys.exit(f"attended_story_ab: leg {leg} ended with status {r.returncode}; stopping")
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("ATTENDED_STORY_AB_CHILD ")]
    if not lines:
        sys.exit(f"attended_story_ab: leg {leg} ended without a result line; stopping")
    print(f"attended_story_ab: leg {leg} done ({'check' if not reps else 'timed'})", file=sys.stderr, flush=True)
    return json.loads(lines[-1][len("ATTENDED_STORY_AB_CHILD "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib-a"); ap.add_argument("--lib-b", default=os.path.join(ROOT, "q-mann_amd", "lib", "libqmann_hip.so"))
    ap.add_argument("--rounds", type=int, default=5); ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--k", type=int, default=5); ap.add_argument("--step-timeout", type=int, default=180)
    ap.add_argument("--shapes", help="comma-separated subset of: " + ", ".join(SHAPES))
    ap.add_argument("--child"); ap.add_argument("--lib")
    a = ap.parse_args()
    only = a.shapes.split(",") if a.shapes else None
    if a.child:
        return child(a.child, a.lib, a.k, a.reps, only)
    if not a.lib_a:
        sys.exit("attended_story_ab: --lib-a <the parent commit's libqmann_hip.so> is required")
    if a.rounds < 5:
        print("attended_story_ab: fewer than 5 rounds: medians and spreads of this run are not to be quoted", file=sys.stderr)
    legs = (("A", a.lib_a), ("B", a.lib_b), ("P", a.lib_a))
    chk = {leg: step(leg, lib, a, 0) for leg, lib in legs}
    for name in chk["A"]:
        assert chk["A"][name]["sha_p"] == chk["B"][name]["sha_p"], f"{name}: leg B's top_p differ from the k largest of leg A's probs"
        assert chk["A"][name]["sha_u"] == chk["B"][name]["sha_u"] == chk["P"][name]["sha_u"], f"{name}: u_out differs between the legs"
    times = {}
    for _ in range(a.rounds):
        for leg, lib in legs:
            for name, r in step(leg, lib, a, a.reps).items():
                times.setdefault(name, {}).setdefault(leg, []).append(r["ms"])
    out = {"tool": "attended_story_ab", "k": a.k, "rounds": a.rounds, "reps": a.reps, "top_p_bit_equal": True, "u_out_bit_equal": True,
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
