"""Runs ON THE GPU BOX: attended slots for float attention (qmann_hops_top_float_i8 / qmann_hops_shared_top_float_i8) against the
two other ways to the same rows, interleaved on one box.

Per call form -- "story": every query its own copy of the memory (qmann_hops_i8, mode 1); "shared": one memory
(qmann_hops_shared_float_i8, the launcher's tile) -- and per k in (5, 16):
  top     the new call;
  tap     the base call with the `probs` tap, then torch.topk over the tap on the device (the tap is [n_hop][n_query][n_slots]
          for both forms here: the copies have equal lengths);
  plain   the base call alone: what the rows cost on top of the hops.

    python3 tools/attended_float_ab.py [--lib <build>] [--rounds 5] [--reps 10] [--shapes long,mid,short] [--forms story,shared]

Shapes and inputs are those of tools/shared_float_ab.py (4 096 queries x 3 hops; long = 10 000 x 128, mid = 1 000 x 60, short =
200 x 60).  Every round is a fresh child process under its own `timeout -k 10`; inside a round the variants of a shape run one
after the other, each `reps` launches (x 10 at mid, x 40 at short) between two HIP events after 3 warm-up launches; the script
stops at the first failing step.  The first round also checks the rows: the new call's slots must equal torch.topk's wherever
the k + 1 largest probabilities of the row are distinct, and its top_p must be the tap's floats.
Prints one JSON line with every round's figure per shape, form and variant, their medians and spreads, and the ratios
tap / top and top / plain of the medians."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from shared_float_ab import FRAC, H, IWL, SHAPES, SIGMA, Fmt, Net  # noqa: E402

KS = (5, 16)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARK = "ATTENDED_FLOAT_AB_CHILD "


class Taps(C.Structure):
    _fields_ = [("score_codes", C.c_void_p), ("scores", C.c_void_p), ("probs", C.c_void_p), ("o", C.c_void_p), ("u", C.c_void_p)]


def child(lib_path, shapes, forms, reps, check):
    import numpy as np
    import torch
    lib = C.CDLL(lib_path)
    vp, u32, sz = C.c_void_p, C.c_uint32, C.c_size_t
    lib.qmann_hops_i8.argtypes = [C.POINTER(Net), vp, vp, sz, vp, u32, vp, vp, C.POINTER(Taps), u32, vp]
    lib.qmann_hops_top_float_i8.argtypes = [C.POINTER(Net), vp, vp, sz, vp, u32, vp, vp, u32, vp, vp, u32, vp]
    lib.qmann_hops_shared_float_i8.argtypes = [C.POINTER(Net), vp, vp, sz, u32, vp, vp, C.POINTER(Taps), u32, vp]
    lib.qmann_hops_shared_top_float_i8.argtypes = [C.POINTER(Net), vp, vp, sz, u32, vp, vp, u32, vp, vp, u32, vp]
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
        probs = torch.empty((H, B, S), dtype=torch.float32, device=dev)
        taps = Taps(None, None, probs.data_ptr(), None, None)
        net = Net()
        net.n_hop, net.dim_emb, net.dim_emb_pad, net.dim_input = H, D, Dp, 256
        net.attention_mode, net.softmax_base, net.en_lin_map, net.num_bit = 1, 0, 1, 8
        for h in range(H):
            net.act[h] = net.w[h] = net.att[h] = Fmt(IWL, FRAC)
            net.lin_map[h] = lin[h].data_ptr()
        net.bin = Fmt(IWL, FRAC)
        p = lambda t: C.c_void_p(t.data_ptr())
        res = {}
        for form in forms:
            if form == "story":
                rep = lambda d: d.unsqueeze(1).expand(H, B, S, Dp).reshape(H, B * S, Dp).contiguous()
                rk, rv = rep(keys), rep(vals)
                row_off = torch.arange(0, (B + 1) * S, S, dtype=torch.int32, device=dev)
                base = lambda tp: lib.qmann_hops_i8(C.byref(net), p(rk), p(rv), B * S * Dp, p(row_off), S, p(u0), p(u_out), tp, B, None)
                top = lambda k, sl, tp: lib.qmann_hops_top_float_i8(C.byref(net), p(rk), p(rv), B * S * Dp, p(row_off), S, p(u0), p(u_out),
                                                                    k, p(sl), p(tp), B, None)
            else:
                base = lambda tp: lib.qmann_hops_shared_float_i8(C.byref(net), p(keys), p(vals), S * Dp, S, p(u0), p(u_out), tp, B, None)
                top = lambda k, sl, tp: lib.qmann_hops_shared_top_float_i8(C.byref(net), p(keys), p(vals), S * Dp, S, p(u0), p(u_out), k,
                                                                           p(sl), p(tp), B, None)
            variants = {"plain": lambda: base(None)}
            for k in KS:
                sl = torch.empty((B, H, k), dtype=torch.int32, device=dev)
                tp = torch.empty((B, H, k), dtype=torch.float32, device=dev)

                def run_top(k=k, sl=sl, tp=tp):
                    return top(k, sl, tp)

                def run_tap(k=k):
                    rc = base(C.byref(taps))
                    torch.topk(probs, k, dim=2)
                    return rc
                variants[f"top_k{k}"], variants[f"tap_k{k}"] = run_top, run_tap
                if check:
                    assert run_top() == 0 and base(C.byref(taps)) == 0
                    torch.cuda.synchronize()
                    wv, wi = torch.topk(probs, k + 1, dim=2)
                    clear = (wv[:, :, :-1] != wv[:, :, 1:]).all(dim=2).t()                    # [B][H]: the first k + 1 are distinct
                    assert torch.equal(tp.view(torch.int32), torch.gather(probs, 2, sl.permute(1, 0, 2).long()).permute(1, 0, 2).view(torch.int32))
                    assert torch.equal(sl[clear].long(), wi[:, :, :k].permute(1, 0, 2)[clear]) and int(clear.sum()) > 0
            times = {}
            for vname, run in variants.items():
                for _ in range(3):
                    assert run() == 0, vname
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                n = reps * sh["reps_x"]
                e0.record()
                for _ in range(n):
                    run()
                e1.record()
                torch.cuda.synchronize()
                times[vname] = e0.elapsed_time(e1) / n
            res[form] = times
            if form == "story":
                del rk, rv
            del variants
            torch.cuda.empty_cache()
        out[name] = res
    print(MARK + json.dumps(out), flush=True)


def step(lib_path, shapes, forms, reps, check, limit):
    """one round: a fresh child under its own time limit; any failure ends the script"""
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", "--lib", lib_path, "--shapes",
           ",".join(shapes), "--forms", ",".join(forms), "--reps", str(reps)] + (["--check"] if check else [])
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    if r.returncode != 0:
        sys.exit(f"attended_float_ab: a round ended with status {r.returncode}; stopping")
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith(MARK)]
    if not lines:
        sys.exit("attended_float_ab: a round ended without a result line; stopping")
    print("attended_float_ab: round done", file=sys.stderr, flush=True)
    return json.loads(lines[-1][len(MARK):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(ROOT, "q-mann_amd", "lib", "libqmann_hip.so"))
    ap.add_argument("--rounds", type=int, default=5); ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shapes", default="long,mid,short"); ap.add_argument("--forms", default="story,shared")
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--child", action="store_true"); ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    shapes, forms = a.shapes.split(","), a.forms.split(",")
    if a.child:
        return child(a.lib, shapes, forms, a.reps, a.check)
    if a.rounds < 5:
        print("attended_float_ab: fewer than 5 rounds: medians and spreads of this run are not to be quoted", file=sys.stderr)
    times = {}
    for i in range(a.rounds):
        got = step(a.lib, shapes, forms, a.reps, i == 0, a.step_timeout)
        for s, per_form in got.items():
            for f, res in per_form.items():
                for v, ms in res.items():
                    times.setdefault(s, {}).setdefault(f, {}).setdefault(v, []).append(round(ms, 4))
    out = {"tool": "attended_float_ab", "rounds": a.rounds, "reps": a.reps, "rows_checked": True, "shapes": {}}
    for s in shapes:
        out["shapes"][s] = dict(SHAPES[s], forms={})
        for f in forms:
            st = {v: dict(rounds_ms=t, median_ms=round(statistics.median(t), 4), spread_ms=round(max(t) - min(t), 4)) for v, t in times[s][f].items()}
            for k in KS:
                st[f"ratio_tap_over_top_k{k}"] = round(st[f"tap_k{k}"]["median_ms"] / st[f"top_k{k}"]["median_ms"], 3)
                st[f"ratio_top_over_plain_k{k}"] = round(st[f"top_k{k}"]["median_ms"] / st["plain"]["median_ms"], 3)
            out["shapes"][s]["forms"][f] = st
    print(json.dumps(out))


if __name__ == "__main__":
    main()
