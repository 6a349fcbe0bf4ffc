"""Runs ON THE GPU BOX: the stopping hop kernel on a memory that NEVER stops, one build of the library against another (the
parent commit's against this tree's), interleaved on one box.

    python3 tools/scan_stop_ab.py --lib-a <parent build>/libqmann_hip.so [--lib-b <this build>] [--rounds 3] [--reps 10]

Shape: bench.py's synth10k_d128_q25 (8 192 queries x 10 000 slots, D 128, Q2.5, 3 hops, e^x softmax, no taps), so the launch
passes hops_host.h::scan_stop_gate and takes the stopping build.  Every key code is +64 and every query code -64 (-2.0): each
of a row's 128 products clamps at -127 and so does the row's score, a row adds e^(-254/32) = 3.6e-4 to the bound's sum, and the
sum ends at 10 000 e^(-7.94) = 3.6 -- far below 32.5: every hop scans all 10 000 rows and pays every post and every look for
nothing.  All weights are 1 / 10 000 (code 0), the linear map is the identity, so u stays what it was and the three hops are
alike.  (The value plane is never read -- no weight survives -- and is the key plane again, to halve the memory.)
Times qmann_hops_i8, the call QNet.hops makes.  Every GPU step is a fresh child process under its own `timeout -k 10`; the
script stops at the first failing step.  A check step per build first (u_out bit-equal between the two, SHA-256), then `rounds`
alternating rounds A, B; a child times `reps` calls between two HIP events after 3 warm-up calls.
Prints one JSON line: per build the rounds' ms, their median and spread (max - min), B / A, and whether B's median is above A's
by more than A's own spread.
The children bind the library themselves (ctypes), so the two builds need not export the same set of symbols."""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import subprocess
import sys

H, B, S, D, IWL = 3, 8192, 10000, 128, 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Fmt(C.Structure):
    _fields_ = [("iwl", C.c_uint32), ("frac", C.c_uint32)]


# (a copy of q-mann_amd/abi.py::Net -- that module binds the library's symbols when it is imported, which fails against a build
# that lacks the newest ones; check_net_layout() below compares the copy with abi.Net's fields read from that file's text)
class Net(C.Structure):
    _fields_ = [("n_hop", C.c_uint32), ("dim_emb", C.c_uint32), ("dim_emb_pad", C.c_uint32), ("dim_input", C.c_uint32),
                ("attention_mode", C.c_uint32), ("softmax_base", C.c_uint32), ("en_lin_map", C.c_uint32), ("num_bit", C.c_uint32),
                ("act", Fmt * 8), ("w", Fmt * 8), ("att", Fmt * 8), ("bin", Fmt), ("lin_map", C.c_void_p * 8),
                ("softmax_shift_based", C.c_uint32), ("en_att_scale", C.c_uint32), ("att_scale", C.c_float * 8),
                ("en_non_linearity", C.c_uint32), ("en_pe", C.c_uint32), ("pe_dim_word", C.c_uint32)]


def check_net_layout():
    """the fields of abi.py::Net, by name, in order -- taken from the source text, so that nothing is bound"""
    import re
    src = open(os.path.join(ROOT, "q-mann_amd", "abi.py")).read()
    m = re.search(r"class Net\(C\.Structure\):\s*_fields_ = \[(.*?)\]\n", src, re.S)
    assert m, "scan_stop_ab: abi.py::Net not found"
    theirs = re.findall(r'\("(\w+)",\s*([^()]*?(?:\([^()]*\))?[^()]*?)\)', m.group(1))
    ours = [(n, t) for n, t in Net._fields_]
    assert [n for n, _ in theirs] == [n for n, _ in ours], "scan_stop_ab: its copy of abi.Net has other fields than q-mann_amd/abi.py"
    ns = {"C": C, "Fmt": Fmt, "_vp": C.c_void_p, "QMANN_MAX_HOP": int(re.search(r"^QMANN_MAX_HOP = (\d+)", src, re.M).group(1))}
    for (n, expr), (_, t) in zip(theirs, ours):
        assert C.sizeof(eval(expr, ns)) == C.sizeof(t), f"scan_stop_ab: field {n} of its copy of abi.Net has another size"


def child(lib_path, reps):
    import torch
    lib = C.CDLL(lib_path)
    vp, u32, sz = C.c_void_p, C.c_uint32, C.c_size_t
    lib.qmann_hops_i8.restype = C.c_int
    lib.qmann_hops_i8.argtypes = [C.POINTER(Net), vp, vp, sz, vp, u32, vp, vp, vp, u32, vp]
    dev = torch.device("cuda:0")
    frac = 7 - IWL
    p = lambda t: C.c_void_p(t.data_ptr())
    keys = torch.full((H, B * S, D), 64, dtype=torch.int8, device=dev)                  # sign-magnitude: +64
    lin = (torch.eye(D, dtype=torch.int8, device=dev) * (1 << frac)).contiguous()       # the identity on the weight grid
    u0 = torch.full((B, D), -64.0 / (1 << frac), dtype=torch.float32, device=dev)
    row_off = (torch.arange(B + 1, device=dev, dtype=torch.int64) * S).to(torch.int32)
    u_out = torch.full_like(u0, float("nan"))
    net = Net()
    net.n_hop, net.dim_emb, net.dim_emb_pad, net.dim_input = H, D, D, 256
    net.attention_mode, net.softmax_base, net.en_lin_map, net.num_bit = 2, 0, 1, 8
    for h in range(H):
        net.act[h] = net.w[h] = net.att[h] = Fmt(IWL, frac)
        net.lin_map[h] = lin.data_ptr()
    net.bin = Fmt(IWL, frac)

    def run():
        return lib.qmann_hops_i8(C.byref(net), p(keys), p(keys), B * S * D, p(row_off), S, p(u0), p(u_out), None, B, None)
    for _ in range(3):
        rc = run()
        assert rc == 0, rc
    torch.cuda.synchronize()
    got = u_out.cpu().numpy()
    res = dict(ms=None, sha_u=hashlib.sha256(got.tobytes()).hexdigest(), u_is_u0=bool((got == u0.cpu().numpy()).all()))
    if reps:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            run()
        e1.record()
        torch.cuda.synchronize()
        res["ms"] = e0.elapsed_time(e1) / reps
    print("SCAN_STOP_AB_CHILD " + json.dumps(res), flush=True)


def step(leg, lib_path, a, reps):
    """one GPU step: a fresh child under its own time limit; any failure ends the script"""
    cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", "--lib", lib_path,
           "--reps", str(reps)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    if r.returncode != 0:
        sys.exit(f"scan_stop_ab: build {leg} ended with status {r.returncode}; stopping")
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("SCAN_STOP_AB_CHILD ")]
    if not lines:
        sys.exit(f"scan_stop_ab: build {leg} ended without a result line; stopping")
    print(f"scan_stop_ab: build {leg} done ({'check' if not reps else 'timed'})", file=sys.stderr, flush=True)
    return json.loads(lines[-1][len("SCAN_STOP_AB_CHILD "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib-a"); ap.add_argument("--lib-b", default=os.path.join(ROOT, "q-mann_amd", "lib", "libqmann_hip.so"))
    ap.add_argument("--rounds", type=int, default=3); ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--step-timeout", type=int, default=180)
    ap.add_argument("--child", action="store_true"); ap.add_argument("--lib")
    a = ap.parse_args()
    if a.child:
        return child(a.lib, a.reps)
    check_net_layout()
    if not a.lib_a:
        sys.exit("scan_stop_ab: --lib-a <the parent commit's libqmann_hip.so> is required")
    legs = (("A", a.lib_a), ("B", a.lib_b))
    chk = {leg: step(leg, lib, a, 0) for leg, lib in legs}
    assert chk["A"]["sha_u"] == chk["B"]["sha_u"], "u_out differs between the builds"
    assert chk["A"]["u_is_u0"] and chk["B"]["u_is_u0"], "a hop changed u: some read-out was not zero, or the map is not the identity"
    times = {leg: [] for leg, _ in legs}
    for _ in range(a.rounds):
        for leg, lib in legs:
            times[leg].append(round(step(leg, lib, a, a.reps)["ms"], 4))
    st = {leg: dict(rounds_ms=t, median_ms=round(statistics.median(t), 4), spread_ms=round(max(t) - min(t), 4)) for leg, t in times.items()}
    print(json.dumps({"tool": "scan_stop_ab", "shape": f"{B} x {S} slots, D {D}, Q{IWL}.{7 - IWL}, {H} hops, every score -127",
                      "rounds": a.rounds, "reps": a.reps, "u_out_bit_equal": True, "A": st["A"], "B": st["B"],
                      "ratio_b_over_a": round(st["B"]["median_ms"] / st["A"]["median_ms"], 4),
                      "b_slower_beyond_a_spread": bool(st["B"]["median_ms"] - st["A"]["median_ms"] > st["A"]["spread_ms"])}))


if __name__ == "__main__":
    main()
