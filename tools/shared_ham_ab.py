"""Runs ON THE GPU BOX: one shared PACKED memory against per-query copies of it, interleaved on one box.  The sibling of
tools/shared_ab.py for the Hamming forms, with the same discipline.

  (A) qmann_hops_packed on n_query copies of the key planes and of the value plane, with ANOTHER build of the library (the
      parent commit's, built into a second directory) -- the baseline is never the code under test;
  (B) qmann_hops_shared_packed on the one memory, this tree's library, for every tile size (queries per workgroup) that fits at
      the shape, forced through QMANN_SHARED_QT, and once with the launcher's own choice ("auto").

    python3 tools/shared_ham_ab.py --lib-a <parent build>/libqmann_hip.so [--lib-b <this build>] [--rounds 5] [--reps 10]
                                   [--shapes config5,d128b8,short] [--queries 8192]

Shapes (3 hops, keys / values / queries / linear map N(0, 40) codes as tests/shared_ham_cases.py draws them):
  config5 = 10 000 x 256, 1 bit, V0 (BASELINE config 5);  d128b8 = 10 000 x 128, 8 bits, V1;  short = 1 000 x 60, 8 bits, V1.
Leg A's copies at 8 192 queries: 63 GB of values + 7.9 GB of planes (config5), 31 + 31 GB (d128b8), 1.6 + 1.6 GB (short).
Every GPU step is a fresh child process under its own `timeout -k 10`; the script stops at the first failing step.  First a
check step per leg: the legs' u_out must be bit-equal (SHA-256 of the bytes) at every shape and tile size.  Then `rounds`
alternating rounds A, B, A, B ...; a child times `reps` launches of each of its variants between two HIP events after 3
warm-up launches.  Prints one JSON line: per shape and variant the median over rounds and the spread (max - min) in ms, the
ratio A / best B, the best tile size, and whether the best B beats A by more than the sum of the two spreads.
The children bind the library themselves (ctypes), so the two builds need not export the same set of symbols."""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import subprocess
import sys

SHAPES = {"config5": dict(S=10000, D=256, Dp=256, nb=1, mode=10), "d128b8": dict(S=10000, D=128, Dp=128, nb=8, mode=11),
          "short": dict(S=1000, D=60, Dp=64, nb=8, mode=11)}
H, IWL, FRAC, SIGMA = 3, 5, 2, 40.0
QTS = (1, 2, 4, 8)
LDS_LIMIT = 160 * 1024 - 1024
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


def child(leg, lib_path, shapes, reps, B):
    import numpy as np
    import torch
    lib = C.CDLL(lib_path)
    vp, u32, sz = C.c_void_p, C.c_uint32, C.c_size_t
    lib.qmann_pack_bitplanes.restype = C.c_int
    lib.qmann_pack_bitplanes.argtypes = [vp, vp, sz, u32, u32, vp]
    lib.qmann_hops_packed.restype = C.c_int
    lib.qmann_hops_packed.argtypes = [C.POINTER(Net), vp, sz, vp, sz, vp, u32, vp, vp, vp, u32, vp]
    if leg == "B":
        lib.qmann_hops_shared_packed.restype = C.c_int
        lib.qmann_hops_shared_packed.argtypes = [C.POINTER(Net), vp, sz, vp, sz, u32, vp, vp, vp, u32, vp]
        lib.qmann_hops_shared_packed_lds_bytes.restype = sz
        lib.qmann_hops_shared_packed_lds_bytes.argtypes = [C.POINTER(Net), u32, u32]
        lib.qmann_hops_shared_packed_tile.restype = u32
        lib.qmann_hops_shared_packed_tile.argtypes = [C.POINTER(Net), u32, u32]
        lib.qmann_tuning_reload.restype = None
    dev = torch.device("cuda:0")
    out = {}

    def signmag(c):
        c = c.astype(np.int16)
        return np.where(c < 0, (-c) | 0x80, c).astype(np.uint8).view(np.int8)
    for name in shapes:
        sh = SHAPES[name]
        S, D, Dp, nb = sh["S"], sh["D"], sh["Dp"], sh["nb"]
        G = Dp // 64
        rng = np.random.default_rng(0x4A33D + S + D)
        codes = lambda *shape: np.clip(np.rint(rng.normal(0, SIGMA, shape)), -127, 127)
        plane = lambda: np.pad(codes(H, S, D), ((0, 0), (0, 0), (0, Dp - D)))
        key_bytes = torch.from_numpy(signmag(plane())).to(dev)
        vals = torch.from_numpy(signmag(plane())).to(dev)
        lin = [torch.from_numpy(signmag(np.pad(codes(D, D), ((0, 0), (0, Dp - D))))).to(dev) for _ in range(H)]
        u0 = torch.from_numpy((codes(B, D) / (1 << FRAC)).astype(np.float32)).to(dev)
        u_out = torch.empty_like(u0)
        p = lambda t: C.c_void_p(t.data_ptr())
        planes = torch.empty((H, S, G, nb), dtype=torch.int64, device=dev)
        assert lib.qmann_pack_bitplanes(p(key_bytes), p(planes), H * S, Dp, nb, None) == 0
        net = Net()
        net.n_hop, net.dim_emb, net.dim_emb_pad, net.dim_input = H, D, Dp, 256
        net.attention_mode, net.softmax_base, net.en_lin_map, net.num_bit = sh["mode"], 0, 1, nb
        for h in range(H):
            net.act[h] = net.w[h] = net.att[h] = Fmt(IWL, FRAC)
            net.lin_map[h] = lin[h].data_ptr()
        net.bin = Fmt(IWL, FRAC)
        variants = {}
        if leg == "A":
            rk = planes.unsqueeze(1).expand(H, B, S, G, nb).reshape(H, B * S, G, nb).contiguous()
            rv = vals.unsqueeze(1).expand(H, B, S, Dp).reshape(H, B * S, Dp).contiguous()
            row_off = torch.arange(0, (B + 1) * S, S, dtype=torch.int32, device=dev)
            variants["A"] = lambda: lib.qmann_hops_packed(C.byref(net), p(rk), B * S * G * nb * 8, p(rv), B * S * Dp, p(row_off), S, p(u0),
                                                          p(u_out), None, B, None)
        else:
            def shared(qt):
                def run():
                    return lib.qmann_hops_shared_packed(C.byref(net), p(planes), S * G * nb * 8, p(vals), S * Dp, S, p(u0), p(u_out), None, B, None)

                def select():
                    if qt:
                        os.environ["QMANN_SHARED_QT"] = str(qt)
                    else:
                        os.environ.pop("QMANN_SHARED_QT", None)
                    lib.qmann_tuning_reload()
                return select, run
            for qt in QTS:
                if lib.qmann_hops_shared_packed_lds_bytes(C.byref(net), S, qt) <= LDS_LIMIT:
                    variants[f"B_qt{qt}"] = shared(qt)
            variants["B_auto"] = shared(0)
        res = {}
        for vname, v in variants.items():
            select, run = v if isinstance(v, tuple) else ((lambda: None), v)
            select()
            u_out.fill_(float("nan"))
            for _ in range(3):
                rc = run()
                assert rc == 0, (vname, rc)
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
                res[vname]["tile"] = int(lib.qmann_hops_shared_packed_tile(C.byref(net), S, B))       # the tile that ran
        out[name] = res
        del key_bytes, vals, planes, variants
        if leg == "A":
            del rk, rv
        torch.cuda.empty_cache()
    print("SHARED_HAM_AB_CHILD " + json.dumps(out), flush=True)


def step(leg, lib_path, shapes, reps, limit, queries):
    """one GPU step: a fresh child under its own time limit; any failure ends the script"""
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", leg, "--lib", lib_path,
           "--shapes", ",".join(shapes), "--reps", str(reps), "--queries", str(queries)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    if r.returncode != 0:
        sys.exit(f"shared_ham_ab: leg {leg} ended with status {r.returncode}; stopping")
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("SHARED_HAM_AB_CHILD ")]
    if not lines:
        sys.exit(f"shared_ham_ab: leg {leg} ended without a result line; stopping")
    print(f"shared_ham_ab: leg {leg} done ({'check' if not reps else 'timed'})", file=sys.stderr, flush=True)
    return json.loads(lines[-1][len("SHARED_HAM_AB_CHILD "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib-a"); ap.add_argument("--lib-b", default=os.path.join(ROOT, "q-mann_amd", "lib", "libqmann_hip.so"))
    ap.add_argument("--rounds", type=int, default=5); ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shapes", default="config5,d128b8,short"); ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--queries", type=int, default=8192)
    ap.add_argument("--child"); ap.add_argument("--lib")
    a = ap.parse_args()
    shapes = a.shapes.split(",")
    if a.child:
        return child(a.child, a.lib, shapes, a.reps, a.queries)
    if not a.lib_a:
        sys.exit("shared_ham_ab: --lib-a <the parent commit's libqmann_hip.so> is required")
    if a.rounds < 5:
        print("shared_ham_ab: fewer than 5 rounds: medians and spreads of this run are not to be quoted", file=sys.stderr)
    # results first: every variant of leg B must give leg A's bytes
    ca = step("A", a.lib_a, shapes, 0, a.step_timeout, a.queries)
    cb = step("B", a.lib_b, shapes, 0, a.step_timeout, a.queries)
    for s in shapes:
        for v, r in cb[s].items():
            assert r["sha"] == ca[s]["A"]["sha"], f"{s}: u_out of {v} differs from leg A's"
    times = {s: {} for s in shapes}
    for _ in range(a.rounds):
        for leg, lib in (("A", a.lib_a), ("B", a.lib_b)):
            got = step(leg, lib, shapes, a.reps, a.step_timeout, a.queries)
            if leg == "B":
                last_b = got
            for s, res in got.items():
                for v, r in res.items():
                    times[s].setdefault(v, []).append(r["ms"])
    out = {"tool": "shared_ham_ab", "rounds": a.rounds, "reps": a.reps, "queries": a.queries, "u_out_bit_equal": True, "shapes": {}}
    for s in shapes:
        st = {v: dict(median_ms=round(statistics.median(t), 4), spread_ms=round(max(t) - min(t), 4)) for v, t in times[s].items()}
        st["B_auto"]["tile"] = last_b[s]["B_auto"]["tile"]
        forced = {v: r for v, r in st.items() if v.startswith("B_qt")}
        best = min(forced, key=lambda v: forced[v]["median_ms"])
        a_ms, b_ms = st["A"]["median_ms"], forced[best]["median_ms"]
        out["shapes"][s] = dict(SHAPES[s], variants=st, best=best, ratio_a_over_best_b=round(a_ms / b_ms, 3),
                                b_beats_a_beyond_spreads=bool(a_ms - b_ms > st["A"]["spread_ms"] + forced[best]["spread_ms"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
