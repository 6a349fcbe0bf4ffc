"""Runs ON THE GPU BOX: float attention (QMANN_ATT_FLOAT) over one shared memory against per-story copies of it, interleaved on one box.

  (A) qmann_hops_i8 (mode 1, k_hops_float) on n_query copies of the planes -- THE YARDSTICK.  It is not the code under test: the
      change that added the shared call left k_hops_float's device code as it was (tools/device_asm_equal.sh), so --lib-a defaults
      to this tree's library; give the parent commit's build (tools/build_variant.sh) to time against that instead;
  (B) qmann_hops_shared_float_i8 on the one memory, for every tile size (queries per workgroup) that fits LDS at the shape, forced
      through QMANN_SHARED_QT, and once with the launcher's own choice ("auto").

    python3 tools/shared_float_ab.py [--lib-a <build>] [--lib-b <build>] [--rounds 5] [--reps 10] [--shapes long,mid,short]

Shapes, 4 096 queries x 3 hops each: long = 10 000 slots x D 128 (31.5 GB of copies for leg A), mid = 1 000 x D 60, short = 200 x
D 60.  Codes N(0, 6) on Q2.5, stock e^x softmax, linear map on.
Every GPU step is a fresh child process under its own `timeout -k 10`; the script stops at the first failing step.  First a check
step per leg: u_out must be bit-equal (SHA-256 of the bytes) at every shape and tile size.  Then `rounds` alternating rounds A, B,
A, B ...; a child times `reps` launches (x 10 at mid, x 40 at short) of each of its variants between two HIP events after 3 warm-up launches.
Prints one JSON line with EVERY round's figure per shape and variant, and per shape the verdict by this rule: the shared call has
WON a shape when its best forced tile is ahead of the per-story call in every round AND the gain of the medians is at least three
times the per-story call's own round-to-round spread (max - min).  Anything else is recorded as not won."""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import subprocess
import sys

# reps_x: the shorter shapes repeat more launches per timing, so that every timed window holds tens of milliseconds of work
SHAPES = {"long": dict(S=10000, D=128, Dp=128, B=4096, reps_x=1), "mid": dict(S=1000, D=60, Dp=64, B=4096, reps_x=10),
          "short": dict(S=200, D=60, Dp=64, B=4096, reps_x=40)}
H, IWL, FRAC, SIGMA = 3, 2, 5, 6.0
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


def child(leg, lib_path, shapes, reps):
    import numpy as np
    import torch
    lib = C.CDLL(lib_path)
    vp, u32 = C.c_void_p, C.c_uint32
    lib.qmann_hops_i8.restype = C.c_int
    lib.qmann_hops_i8.argtypes = [C.POINTER(Net), vp, vp, C.c_size_t, vp, u32, vp, vp, vp, u32, vp]
    if leg == "B":
        lib.qmann_hops_shared_float_i8.restype = C.c_int
        lib.qmann_hops_shared_float_i8.argtypes = [C.POINTER(Net), vp, vp, C.c_size_t, u32, vp, vp, vp, u32, vp]
        lib.qmann_hops_shared_float_lds_bytes.restype = C.c_size_t
        lib.qmann_hops_shared_float_lds_bytes.argtypes = [u32, u32]
        lib.qmann_tuning_reload.restype = None
        lib.qmann_hops_shared_float_tile.restype = u32
        lib.qmann_hops_shared_float_tile.argtypes = [u32, u32]
    dev = torch.device("cuda:0")
    out = {}

    def signmag(c):
        c = c.astype(np.int16)
        return np.where(c < 0, (-c) | 0x80, c).astype(np.uint8).view(np.int8)
    for name in shapes:
        sh = SHAPES[name]
        S, D, Dp, B = sh["S"], sh["D"], sh["Dp"], sh["B"]
        rng = np.random.default_rng(0xF10A7 + S)
        codes = lambda *shape: np.clip(np.rint(rng.normal(0, SIGMA, shape)), -127, 127)
        plane = lambda: np.pad(codes(H, S, D), ((0, 0), (0, 0), (0, Dp - D)))
        keys = torch.from_numpy(signmag(plane())).to(dev)
        vals = torch.from_numpy(signmag(plane())).to(dev)
        lin = [torch.from_numpy(signmag(np.pad(codes(D, D), ((0, 0), (0, Dp - D))))).to(dev) for _ in range(H)]
        u0 = torch.from_numpy((codes(B, D) / (1 << FRAC)).astype(np.float32)).to(dev)
        u_out = torch.empty_like(u0)
        net = Net()
        net.n_hop, net.dim_emb, net.dim_emb_pad, net.dim_input = H, D, Dp, 256
        net.attention_mode, net.softmax_base, net.en_lin_map, net.num_bit = 1, 0, 1, 8
        for h in range(H):
            net.act[h] = net.w[h] = net.att[h] = Fmt(IWL, FRAC)
            net.lin_map[h] = lin[h].data_ptr()
        net.bin = Fmt(IWL, FRAC)
        p = lambda t: C.c_void_p(t.data_ptr())
        variants = {}
        if leg == "A":
            rep = lambda d: d.unsqueeze(1).expand(H, B, S, Dp).reshape(H, B * S, Dp).contiguous()
            rk, rv = rep(keys), rep(vals)
            row_off = torch.arange(0, (B + 1) * S, S, dtype=torch.int32, device=dev)
            variants["A"] = lambda: lib.qmann_hops_i8(C.byref(net), p(rk), p(rv), B * S * Dp, p(row_off), S, p(u0), p(u_out), None, B, None)
        else:
            def shared(qt):
                def run():
                    return lib.qmann_hops_shared_float_i8(C.byref(net), p(keys), p(vals), S * Dp, S, p(u0), p(u_out), None, B, None)

                def select():
                    if qt:
                        os.environ["QMANN_SHARED_QT"] = str(qt)
                    else:
                        os.environ.pop("QMANN_SHARED_QT", None)
                    lib.qmann_tuning_reload()
                return select, run
            for qt in QTS:
                if lib.qmann_hops_shared_float_lds_bytes(S, qt) <= LDS_LIMIT:
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
                n = reps * sh["reps_x"]
                e0.record()
                for _ in range(n):
                    run()
                e1.record()
                torch.cuda.synchronize()
                ms = e0.elapsed_time(e1) / n
            res[vname] = dict(ms=ms, sha=digest)
            if leg == "B":
                res[vname]["tile"] = int(lib.qmann_hops_shared_float_tile(S, B))       # the tile that ran (B_auto: the launcher's choice)
        out[name] = res
        del keys, vals, variants
        if leg == "A":
            del rk, rv
        torch.cuda.empty_cache()
    print("SHARED_FLOAT_AB_CHILD " + json.dumps(out), flush=True)


def step(leg, lib_path, shapes, reps, limit):
    """one GPU step: a fresh child under its own time limit; any failure ends the script"""
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", leg, "--lib", lib_path,
           "--shapes", ",".join(shapes), "--reps", str(reps)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    if r.returncode != 0:
        sys.exit(f"shared_float_ab: leg {leg} ended with status {r.returncode}; stopping")
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("SHARED_FLOAT_AB_CHILD ")]
    if not lines:
        sys.exit(f"shared_float_ab: leg {leg} ended without a result line; stopping")
    print(f"shared_float_ab: leg {leg} done ({'check' if not reps else 'timed'})", file=sys.stderr, flush=True)
    return json.loads(lines[-1][len("SHARED_FLOAT_AB_CHILD "):])


def verdict(a_rounds, b_rounds):
    """the rule of the module text, on the rounds of the per-story call and of ONE shared variant"""
    a_med, b_med = statistics.median(a_rounds), statistics.median(b_rounds)
    a_spread = max(a_rounds) - min(a_rounds)
    ahead = all(b < a for a, b in zip(a_rounds, b_rounds))
    return dict(ahead_in_every_round=ahead, gain_ms=round(a_med - b_med, 4), per_story_spread_ms=round(a_spread, 4),
                won=bool(ahead and a_med - b_med >= 3 * a_spread))


def main():
    here = os.path.join(ROOT, "q-mann_amd", "lib", "libqmann_hip.so")
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib-a", default=here); ap.add_argument("--lib-b", default=here)
    ap.add_argument("--rounds", type=int, default=5); ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shapes", default="long,mid,short"); ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--child"); ap.add_argument("--lib")
    a = ap.parse_args()
    shapes = a.shapes.split(",")
    if a.child:
        return child(a.child, a.lib, shapes, a.reps)
    if a.rounds < 5:
        print("shared_float_ab: fewer than 5 rounds: medians and spreads of this run are not to be quoted", file=sys.stderr)
    # results first: every variant of leg B must give leg A's bytes
    ca, cb = step("A", a.lib_a, shapes, 0, a.step_timeout), step("B", a.lib_b, shapes, 0, a.step_timeout)
    for s in shapes:
        for v, r in cb[s].items():
            assert r["sha"] == ca[s]["A"]["sha"], f"{s}: u_out of {v} differs from leg A's"
    times = {s: {} for s in shapes}
    for _ in range(a.rounds):
        for leg, lib in (("A", a.lib_a), ("B", a.lib_b)):
            got = step(leg, lib, shapes, a.reps, a.step_timeout)
            if leg == "B":
                last_b = got
            for s, res in got.items():
                for v, r in res.items():
                    times[s].setdefault(v, []).append(round(r["ms"], 4))
    out = {"tool": "shared_float_ab", "rounds": a.rounds, "reps": a.reps, "u_out_bit_equal": True, "shapes": {}}
    for s in shapes:
        st = {v: dict(rounds_ms=t, median_ms=round(statistics.median(t), 4), spread_ms=round(max(t) - min(t), 4)) for v, t in times[s].items()}
        st["B_auto"]["tile"] = last_b[s]["B_auto"]["tile"]
        forced = {v: r for v, r in st.items() if v.startswith("B_qt")}
        best = min(forced, key=lambda v: forced[v]["median_ms"])
        out["shapes"][s] = dict(SHAPES[s], variants=st, best=best,
                                ratio_a_over_best_b=round(st["A"]["median_ms"] / forced[best]["median_ms"], 3),
                                best_against_per_story=verdict(times[s]["A"], times[s][best]),
                                auto_against_per_story=verdict(times[s]["A"], times[s]["B_auto"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
