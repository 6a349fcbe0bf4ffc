#!/usr/bin/env python3
"""bench.py -- throughput of the quantized MemN2N inference hot path on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload NAME] [--full] [--dump-outputs DIR]

One "step" = one pass of the hot path (all hops of every query, then the answer layer) over
one resident batch of synthetic queries.  Prints ONE JSON line (rank 0).

A plain run sets up, runs W warm-up steps and K timed steps of one workload and prints its line: nothing else.
`--full` adds everything beyond the headline figure: the secondary configs under `configs` (below), the >= 2 s
sustained window, the CPU baselines, and (babi_task1_*) the host-input copy / pipelined / 64-story serving legs.
`--dump-outputs DIR` writes what the timed path returned in its last timed step as DIR/<name>.npy (see dump_outputs).

Workloads (config.workload; `--workload NAME` runs one alone):
  synth10k_d128_q25  BASELINE.json configs[3] EXACTLY as SURVEY.md 8(d) words it, one GPU's shard: |memory| = 10 000 slots,
                  D = 128, int8 Q2.5, key / value / query codes clip(round(N(0, 6)), +-127), linear-map codes sigma 6, int8
                  answer matrix [256][128] (the MFMA projection), 3 hops, fixed-point dot attention (ATTENTION_MODE 2),
                  8 192 queries per GPU, per-query memories (62.9 GB).  Default: this is the configuration the north-star
                  roofline target is quoted on.
The DEFAULT line (no --workload) of a --full run carries, beside that headline, one object per BASELINE.json config under `configs`
(each: value, ms_per_step, roofline or "QPS only" as SURVEY.md 8(d) says, cpu_baseline) -- all under the driver's clock:
  mem50     babi_mem50             |memory| = 50 (MAX_SEN_LEN cap), D = 60: the size BASELINE.json's metric string names
                                   (also promoted to top-level keys mem50_queries_per_s / mem50_roofline_frac)
  cfg2      babi_task1_idx         configs[1]: bAbI task 1 (all 1 000 test stories, replicated), 3 hops, int8, dot attention,
                                   whole forward from word indices
  cfg3      babi_joint20_appx_mq   configs[2] as the stock define.h builds it: 20-task joint, ATTENTION_MODE 3, EN_MQ
  cfg4_q52  synth10k_d128          configs[3] at run.sh's default format Q5.2 (codes sigma 3.5, float answer layer)
  cfg5      synth10k_d256_ham      configs[4]: D = 256, binary-code Hamming attention + int8 MFMA output GEMM

N > 1: one rank per GPU.  Either the caller starts the ranks (torch.distributed.run sets WORLD_SIZE /
RANK / LOCAL_RANK) or, when `--gpus N` is given with no WORLD_SIZE in the environment, this script
starts them itself: the parent -- which never touches the GPU -- runs torch.distributed.run as a child
process with N ranks of this same file and exits with its code.  Queries are independent, so the batch
is sharded with no data-path collective (weak scaling: 8 192 queries per GPU); RCCL is used once, to
broadcast the quantized parameters from rank 0 (timed separately).
"""
from __future__ import annotations

import argparse
import importlib.util
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

torch = None                    # imported in main(), after the launcher decision (see self_launch)

ROOT = Path(__file__).resolve().parent
HBM_PEAK_GBS = 8000.0          # MI355X HBM3E spec peak (/opt/skills/guides/MI355X_MICROARCH.md)


def load_pkg():
    if "qmann_amd" in sys.modules:
        return sys.modules["qmann_amd"]
    d = ROOT / "q-mann_amd"
    spec = importlib.util.spec_from_file_location("qmann_amd", d / "__init__.py", submodule_search_locations=[str(d)])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["qmann_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


WORKLOADS = {
    # S slots, D, V, B queries per GPU, attention mode (define.h:10-15; 10 = packed popcount V0), planes,
    # answer layer ("f32" | "i8" = int8 MFMA), sigma of key/query codes and of value codes
    "synth10k_d128": dict(S=10000, D=128, V=256, B=8192, mode=2, nb=8, ans="f32", sk=3.5, sv=30.0, su=3.5),
    # BASELINE.json configs[3] EXACTLY as SURVEY.md 8(d) words it: format Q2.5 (define.h:18-19's commented preset), key / value /
    # query codes clip(round(N(0, 6)), +-127), linear-map codes sigma 6, int8 answer matrix [256][128] (the MFMA projection)
    "synth10k_d128_q25": dict(S=10000, D=128, V=256, B=8192, mode=2, nb=8, ans="i8", sk=6.0, sv=6.0, su=6.0, iwl=2, wh_codes=6.0),
    "synth10k_d256_ham": dict(S=10000, D=256, V=256, B=8192, mode=10, nb=1, ans="i8", sk=30.0, sv=30.0, su=30.0),
    # config 5 with the larger of its two dictionary sizes (V in {256, 4 096}): the int8 MFMA projection is 17 GOP
    "synth10k_d256_ham_v4096": dict(S=10000, D=256, V=4096, B=8192, mode=10, nb=1, ans="i8", sk=30.0, sv=30.0, su=30.0),
    # config 5's other form ("also n = 8 bit-planes"): 8-bit codes, weighted Hamming V1 / plain V0, straight from the int8 keys
    "synth10k_d256_v1_nb8": dict(S=10000, D=256, V=256, B=4096, mode=11, nb=8, ans="i8", sk=30.0, sv=30.0, su=30.0),
    "synth10k_d256_v0_nb8": dict(S=10000, D=256, V=256, B=4096, mode=10, nb=8, ans="i8", sk=30.0, sv=30.0, su=30.0),
    "synth10k_d128_appx": dict(S=10000, D=128, V=256, B=8192, mode=3, nb=8, ans="f32", sk=30.0, sv=30.0, su=30.0),
    "synth10k_d128_float": dict(S=10000, D=128, V=256, B=4096, mode=1, nb=8, ans="f32", sk=3.5, sv=30.0, su=3.5),
    # between the bAbI cap and the long memories: the one-wavefront-workgroup form of the streaming kernel (65..256 slots)
    "synth200_d64": dict(S=200, D=60, V=80, B=131072, mode=2, nb=8, ans="f32", sk=8.0, sv=30.0, su=8.0),
    "synth1000_d64": dict(S=1000, D=60, V=80, B=32768, mode=2, nb=8, ans="f32", sk=8.0, sv=30.0, su=8.0),
    "babi_mem50": dict(S=50, D=60, V=80, B=262144, mode=2, nb=8, ans="f32", sk=8.0, sv=30.0, su=8.0),
    "babi_joint_appx": dict(S=50, D=60, V=256, B=262144, mode=3, nb=8, ans="f32", sk=30.0, sv=30.0, su=30.0),
    # BASELINE.json configs[2] shape with the CPU-spec weighted Hamming score on packed bit planes + popcount
    "babi_joint_v1": dict(S=50, D=60, V=256, B=262144, mode=11, nb=8, ans="f32", sk=30.0, sv=30.0, su=30.0),
    # BASELINE.json configs[1]: real bAbI task-1 stories (the 64-story fixture produced by the reference's
    # sample.c, replicated), 3 hops, int8, EN_MQ formats, the WHOLE forward from bag-of-words input:
    # story + question embedding, hops, answer layer
    "babi_task1_bow": dict(S=10, D=60, V=30, B=262144, mode=2, nb=8, ans="f32", bow=True),
    # the same forward fed with the compact wire format: uint16 word indices instead of float bag-of-words rows
    "babi_task1_idx": dict(S=10, D=60, V=30, B=262144, mode=2, nb=8, ans="f32", bow=True, idx=True),
}
# BASELINE.json configs[2] on REAL data: the 20 bAbI tasks jointly (2 000 test stories, 100 per task, vectorised
# by the reference's sample.c with its joint-task limits; tests/golden/babi_joint20_test2000.npz), replicated;
# the whole forward from word indices through the library's own host object (include/qmann_model.h)
for _n, _m, _nb in (("babi_joint20_v1", 11, 8), ("babi_joint20_v0", 10, 8), ("babi_joint20_appx", 3, 8), ("babi_joint20_fixed", 2, 8)):
    WORKLOADS[_n] = dict(S=64, D=60, V=238, B=262000, mode=_m, nb=_nb, ans="f32", joint=True)
# the same with the embedding matrices tied across the hops as the reference trains them (TYPE_WEIGHT_TYING 2,
# MemN2N/define.h:287; MemN2N.c:1770-1773): the host model then embeds the stories once for all hops
# configs[2] as the reference's stock define.h builds it once ATTENTION_MODE is 3: EN_MQ stays on (hop 0 embeds on Q6.1,
# hop 2 on Q4.3, the attention works on Q5.2 operand words; csrc/ham_common.h "APPX under EN_MQ")
WORKLOADS["babi_joint20_appx_mq"] = dict(S=64, D=60, V=238, B=262000, mode=3, nb=8, ans="f32", joint=True, mq=True)
WORKLOADS["babi_joint20_v1_tied"] = dict(S=64, D=60, V=238, B=262000, mode=11, nb=8, ans="f32", joint=True, tied=True)
# BASELINE.json configs[1] on TRAINED weights: the matrices the reference's unmodified host program trained on bAbI task 1
# through this library (tools/make_trained_fixture.py -> tests/golden/trained_qa1/), the 1 000 real test stories read from the
# record files (replicated), labels from the files: reports queries/s AND the test error, beside the err(test) the reference
# program itself printed for these weights
WORKLOADS["babi_task1_trained"] = dict(S=10, D=60, V=0, B=262000, mode=2, nb=8, ans="f32", trained=True)
# the default line's secondary configs: (key under `configs`, workload, with the >= 1 s sustained window)
HEADLINE = "synth10k_d128_q25"      # BASELINE.json configs[3] exactly as SURVEY.md 8(d) words it
SECONDARY = [("mem50", "babi_mem50", True), ("cfg2", "babi_task1_idx", False), ("cfg3", "babi_joint20_appx_mq", False),
             ("cfg4_q52", "synth10k_d128", False), ("cfg5", "synth10k_d256_ham", False)]
KERNEL_OF_MODE = {1: "k_hops_float", 2: "k_hops_fixed", 3: "k_hops_ham", 10: "k_hops_ham", 11: "k_hops_ham"}


COMM = None                     # parallel.Comm of this rank (N > 1 on GPUs over RCCL), made in main()


def with_bcast(out, bcast):
    """attach the parameter-broadcast record (N > 1) to a result line"""
    if bcast is not None:
        out["param_broadcast_ms"] = bcast["ms"]
        out["param_broadcast"] = bcast
    return out


def data_rank(rank: int) -> int:
    """Which rank's synthetic data this process generates: its own -- or, for a one-rank run that stands in for rank r of
    an N-rank job (tests/test_gpu_dist.py compares the two), QMANN_BENCH_AS_RANK = r."""
    return int(os.environ.get("QMANN_BENCH_AS_RANK", rank))


def shard_report(out, pred, B, rank, world, dev):
    """Which global queries each rank owned ([lo, hi) in rank order: weak scaling, rank r owns [r B, (r + 1) B)) and the CRC-32
    of each rank's last-step predictions (rank 0 collects them; one small all-gather after the timed region)."""
    import zlib
    crc = zlib.crc32(pred.to(torch.int32).cpu().numpy().tobytes())
    r = data_rank(rank)
    if world == 1:
        out["shards"] = [[r * B, (r + 1) * B]]
        out["pred_crc32"] = [crc]
        return
    import torch.distributed as dist
    t = torch.tensor([float(r * B), float((r + 1) * B), float(crc)], dtype=torch.float64, device=dev)
    parts = [torch.empty_like(t) for _ in range(world)]
    dist.all_gather(parts, t)
    m = torch.stack(parts).cpu().numpy()
    out["shards"] = [[int(a), int(b)] for a, b, _ in m]
    out["pred_crc32"] = [int(c) for _, _, c in m]


DUMP_BYTES_MAX = 60_000_000     # --dump-outputs: under 64 MB in all, the .npy headers included


def keep_outputs(args, res, outputs):
    """--dump-outputs: attach what the last timed step returned to its caller (device tensors; main() writes them)"""
    if args.dump_outputs:
        res["_outputs"] = {k: v for k, v in outputs.items() if v is not None}


def dump_outputs(directory, outputs):
    """DIR/<name>.npy per output: float tensors as float32, integer ones as float64 (exact).  Inputs are seeded, so two builds
    run with the same arguments can be compared file by file.  Above DUMP_BYTES_MAX the arrays that have one row per query
    keep a fixed, seeded sample of rows (the same for the same batch size), whose indices go to DIR/sample_rows.npy."""
    d = Path(directory)
    d.mkdir(parents=True, exist_ok=True)
    arrs = {}
    for k, t in outputs.items():
        a = t.detach().cpu().numpy()
        arrs[k] = a.astype(np.float32 if a.dtype.kind == "f" and a.itemsize <= 4 else np.float64)
    n = max((a.shape[0] for a in arrs.values() if a.ndim), default=0)
    per_query = [k for k, a in arrs.items() if a.ndim and a.shape[0] == n]
    total = sum(a.nbytes for a in arrs.values())
    if total > DUMP_BYTES_MAX:
        fixed = total - sum(arrs[k].nbytes for k in per_query)
        row_bytes = sum(arrs[k].nbytes for k in per_query) // n + 8
        rows = np.sort(np.random.default_rng(0x5EED).choice(n, (DUMP_BYTES_MAX - fixed) // row_bytes, replace=False))
        for k in per_query:
            arrs[k] = arrs[k][rows]
        arrs["sample_rows"] = rows.astype(np.float64)
    for k, a in arrs.items():
        np.save(d / f"{k}.npy", np.ascontiguousarray(a))


def _round(x, sig=6):
    if isinstance(x, float):
        return float(f"{x:.{sig}g}")
    if isinstance(x, dict):
        return {k: _round(v, sig) for k, v in x.items()}
    if isinstance(x, list):
        return [_round(v, sig) for v in x]
    return x


def compact(res, primary=False):
    """A result dict reduced to what the driver-timed line needs (the driver keeps a few KB of stdout): numbers to six
    digits, no prose beyond short labels.  `--workload NAME` alone prints the full record."""
    keep_cfg = ("workload", "slots", "dim_emb", "hops", "queries_per_gpu", "format", "attention_mode", "key_row_bytes",
                "answer_layer", "dim_answer", "num_bit", "input", "parallelism")
    keep_roof = ("bound", "kernel", "achieved", "peak", "unit", "frac", "frac_padded_rows", "traffic", "algorithmic_bytes_per_launch", "bytes_per_query",
                 "kernel_ms", "frac_sustained", "frac_by_survey_formula")
    out = {k: res[k] for k in (("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                                "vs_baseline", "dtype", "data") if primary else ("value", "unit", "ms_per_step", "data")) if k in res}
    if not primary:                                        # secondaries: what repeats the headline's constants goes
        keep_cfg = tuple(k for k in keep_cfg if k not in ("parallelism", "hops"))
        keep_roof = tuple(k for k in keep_roof if k not in ("peak", "unit", "frac_by_survey_formula", "algorithmic_bytes_per_launch"))
        out.pop("unit", None)
        if out.get("data") == "synthetic":
            out.pop("data")
        elif "data" in out:
            out["data"] = out["data"][:80]
    out["config"] = {k: v for k, v in res["config"].items() if k in keep_cfg}
    r = res["roofline"]
    out["roofline"] = {k: r[k] for k in keep_roof if k in r}
    if "whole forward" in str(r.get("kernel", "")):
        out["roofline"]["kernel"] = "whole forward"
        out["roofline"]["note"] = "QPS only (SURVEY 8(d): latency-bound size); achieved = input bytes / time"
    elif r.get("traffic") is None:
        out["roofline"]["traffic_note"] = str(r.get("traffic_source") or "no counter pass on these kernel sources")[:60]
    else:
        out["roofline"]["traffic_note"] = "rocprofv3 --pmc FETCH_SIZE pass (profiles/), x2 gfx950 correction"
    c = res.get("cpu_baseline")
    if c:
        out["cpu_baseline"] = {"value": c["value"], "unit": c["unit"], "cores": c["cores"], "kind": c["kind"], "flags": c.get("flags"),
                               "sample": c["sample"][:150 if primary else 100], "one_thread": c.get("one_thread", {}).get("value"),
                               "reference_flags_value": c.get("reference_flags", {}).get("value"),
                               "pred_agree": c.get("pred_agree"), "pred_total": c.get("pred_total")}
    a = res.get("answer_layer")
    if a:
        out["answer_layer"] = {k: a[k] for k in ("ms", "tops", "tflops", "frac_of_int8_peak", "mfma_busy_frac_counters") if k in a}
    if "sustained" in res:
        su = res["sustained"]
        out["sustained"] = {k: su[k] for k in ("steps", "seconds", "queries_per_s", "kernel_ms", "frac") if k in su}
    for k in ("param_broadcast_ms", "param_broadcast", "ranks", "shards", "pred_crc32", "accuracy", "small_batch"):
        if k in res and (primary or k in ("accuracy", "small_batch")):
            out[k] = res[k]
    if "small_batch" in out:
        out["small_batch"] = {k: v for k, v in out["small_batch"].items() if k != "note"}
    if "accuracy" in out:
        out["accuracy"] = {k: out["accuracy"][k] for k in ("test_error_from_labels", "reference_program_err_test", "equals_reference_program")
                           if k in out["accuracy"]}
    return _round(out)


def gauss_i8(shape, sigma, gen, dev, pad_from=None):
    """sign-magnitude int8 codes of clip(round(N(0, sigma)), +-127), generated on the device in chunks."""
    out = torch.empty(shape, dtype=torch.int8, device=dev)
    flat = out.view(-1)
    n = flat.numel()
    chunk = 1 << 28
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        x = torch.randn(b - a, device=dev, generator=gen, dtype=torch.float32)
        c = x.mul_(sigma).round_().clamp_(-127, 127).to(torch.int8)
        flat[a:b] = torch.where(c < 0, (-c) | -128, c)
    if pad_from is not None and pad_from < shape[-1]:
        out[..., pad_from:] = 0
    return out


def make_params(cfg, D, V, seed, wh_sigma=None):
    rng = np.random.default_rng(seed)
    sig = float(os.environ.get("QMANN_BENCH_WH_SIGMA", "1.0")) if wh_sigma is None else wh_sigma   # (env: clamp-density experiments)
    return {"w_h": [rng.normal(0, sig, (D, D)).astype(np.float32) for _ in range(cfg["n_hop"])],
            "w_ans": rng.normal(0, 0.1, (V, D)).astype(np.float32)}


def usable_cores():
    """Threads for the CPU baseline: the cgroup CPU quota when one is set, else the affinity mask capped at
    16 (the GPU pool's documented host share per GPU; the affinity mask there shows the whole host)."""
    import math
    n = max(1, len(os.sched_getaffinity(0)))
    for path, parse in (("/sys/fs/cgroup/cpu.max", lambda t: t.split()),
                        ("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", lambda t: [t.strip(), None])):
        try:
            q, per = parse(open(path).read())
            if q != "max" and int(q) > 0:
                per = int(per) if per else int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
                return max(1, min(n, math.ceil(int(q) / per)))
        except (OSError, ValueError):
            pass
    return min(n, 16)


def cpu_baseline_refport(cfg, wts, pool, what, gpu_preds=None, budget_s=4.0):
    """The CPU baseline SURVEY.md 8(d) / BASELINE.md section 2 prescribe, timed on this box's host cores: the same
    forward composed from the reference's own LIVE C functions (dense_mat_fwd, softmax_fwd, sum_vec_fwd,
    hamming_similarity*: compiled unmodified from the reference tree into oracle/_ref, which travels prebuilt) and
    the port for the ops whose CPU bodies are dead there (oracle/ref_forward.c), at the reference's own flags
    (`gcc -w`, no -O) and at -O2, on one thread (the reference is single-threaded) and on every usable core; a C
    pthread loop, no Python inside the timed region.  pool: (story, question) or (keys, vals, u0) float arrays of
    queries of the SAME batch the GPU ran.  Checker infrastructure used as a reported baseline only.
    Returns None when oracle/_ref is absent (then the caller reports the plain port)."""
    sys.path.insert(0, str(ROOT / "oracle"))
    from pyoracle import Oracle, RefForward, SM_CPU_POW2
    try:
        rfs = {f: RefForward(f) for f in ("O2", "O0")}
    except (FileNotFoundError, OSError):
        return None
    ora = Oracle()
    # the reference's live CPU softmax is the 2^(x - max) form (lib/layer.c:1225); the arithmetic cost equals the e^x form
    m_cpu = ora.make_model({**cfg, "softmax_variant": SM_CPU_POW2}, wts)
    cores = usable_cores()
    res = {}
    for f, rf in rfs.items():
        one = rf.time(m_cpu, pool, 1, budget_s)
        many = rf.time(m_cpu, pool, cores, budget_s)
        res[f] = {"flags": rf.flags, "value": many["qps"], "cores": cores,
                  "sample": f"{many['n']} forwards in {many['secs']:.1f} s on {cores} threads",
                  "one_thread": {"value": one["qps"], "sample": f"{one['n']} forwards in {one['secs']:.1f} s"}}
    out = {"value": res["O2"]["value"], "unit": "queries/s", "cores": cores, "kind": "reference+port",
           "flags": res["O2"]["flags"],
           "sample": f"{what}: pool of {len(pool)} queries of the same batch, {res['O2']['sample']} (C pthread loop)",
           "one_thread": res["O2"]["one_thread"],
           "reference_flags": res["O0"],
           "composition": "reference live C code: dense_mat_fwd, softmax_fwd (its CPU form 2^(x-max)), sum_vec_fwd, "
                          "hamming_similarity{,_w}; port (dead CPU bodies in the reference): dot_mat_vec_fwd, dense_fwd, "
                          "mode-3 attention, arg-max"}
    if gpu_preds is not None:
        # predictions: the GPU ran the e^x softmax (the CUDA form); compare with the port evaluating that same form
        m_gpu = ora.make_model(cfg, wts)
        n = min(len(pool), len(gpu_preds), 64)
        t0, preds = time.perf_counter(), []
        for item in pool[:n]:
            if time.perf_counter() - t0 > 3.0 and preds:
                break
            pr, _ = (ora.forward_mem(m_gpu, *item, taps=()) if len(item) == 3 else ora.forward(m_gpu, *item, taps=()))
            preds.append(pr)
        out["pred_agree"] = int(sum(int(a == b) for a, b in zip(gpu_preds, preds)))
        out["pred_total"] = len(preds)
    return out


def mem_pool(cfg, keys, vals, u0, S, D, n_max=64, bytes_max=2e9):
    """First queries of the resident batch as the float-on-grid arrays the CPU code takes: (keys [H][S][D], vals, u0)."""
    from qmann_amd.model import from_signmag
    H = cfg["n_hop"]
    n = int(max(1, min(u0.shape[0], n_max, bytes_max // max(2 * H * S * D * 4, 1))))

    def inputs(q):
        kf = np.stack([from_signmag(keys[h, q * S:(q + 1) * S, :D].cpu().numpy()).astype(np.float32)
                       / np.float32(1 << cfg["fmt_att"][h][1]) for h in range(H)])
        vf = np.stack([from_signmag(vals[h, q * S:(q + 1) * S, :D].cpu().numpy()).astype(np.float32)
                       / np.float32(1 << cfg["fmt"][h][1]) for h in range(H)])
        return kf, vf, u0[q].cpu().numpy()
    return [inputs(q) for q in range(n)]


def cpu_baseline_port(cfg, wts, pool, what, gpu_preds=None, budget_s=6.0):
    """Fallback when oracle/_ref is absent: the scalar C oracle (-O2) alone, one thread and every usable core
    (Python threads around ctypes calls, which release the GIL)."""
    import threading
    sys.path.insert(0, str(ROOT / "oracle"))
    from pyoracle import Oracle
    ora = Oracle()
    m = ora.make_model(cfg, wts)
    fwd = (lambda it: ora.forward_mem(m, *it, taps=())[0]) if len(pool[0]) == 3 else (lambda it: ora.forward(m, *it, taps=())[0])
    done, t_used, preds = 0, 0.0, []
    while t_used < budget_s or done < 2:
        t0 = time.perf_counter()
        pr = fwd(pool[done % len(pool)])
        t_used += time.perf_counter() - t0
        if done < len(pool):
            preds.append(pr)
        done += 1
    cores = usable_cores()
    counts = [0] * cores
    t_end = time.perf_counter() + budget_s

    def worker(t):
        i = t
        while time.perf_counter() < t_end:
            fwd(pool[i % len(pool)])
            counts[t] += 1
            i += cores
    ths = [threading.Thread(target=worker, args=(t,)) for t in range(cores)]
    t0 = time.perf_counter()
    for th in ths:
        th.start()
    for th in ths:
        th.join()
    wall = time.perf_counter() - t0
    out = {"value": sum(counts) / wall, "unit": "queries/s", "cores": cores, "kind": "port", "flags": "gcc -O2",
           "sample": f"{what}: pool of {len(pool)} queries, {sum(counts)} forwards in {wall:.1f} s on {cores} threads, scalar C oracle "
                     "(oracle/_ref absent: no reference code in this figure)",
           "one_thread": {"value": done / t_used, "sample": f"{done} forwards in {t_used:.1f} s"}}
    if gpu_preds is not None:
        out["pred_agree"] = int(sum(int(a == b) for a, b in zip(gpu_preds, preds)))
        out["pred_total"] = min(len(preds), len(gpu_preds))
    return out


CPU_BUDGET_S = 4.0              # seconds per timed CPU leg (4 legs per workload: -O2 / -O0 x 1 thread / all cores); the default
                                # line's secondary configs use a shorter one so that the whole run stays within minutes


def cpu_baseline(cfg, wts, pool, what, gpu_preds=None):
    return (cpu_baseline_refport(cfg, wts, pool, what, gpu_preds, budget_s=CPU_BUDGET_S)
            or cpu_baseline_port(cfg, wts, pool, what, gpu_preds, budget_s=CPU_BUDGET_S))


def run_bow(args, name, wl, net, cfg, wts, hm, dev, rank, world, model):
    """configs[1]: the full forward from bag-of-words stories (embedding + hops + answer)."""
    use_idx = bool(wl.get("idx"))
    # word indices: ALL 1 000 test stories of qa1 ("real qa1 test set (1 000 queries) + replication"),
    # as the reference's sample.c vectorised them (tests/golden/babi_qa1_test1000_words.npz, oracle/gen_golden.py);
    # float bag-of-words rows: the 64-story fixture of the same set
    g = np.load(ROOT / "tests" / "golden" / ("babi_qa1_test1000_words.npz" if use_idx else "babi_qa1_test64.npz"))
    n_sen = g["n_sen"].astype(np.int64)
    B = args.queries or wl["B"]
    rep = (B + len(n_sen) - 1) // len(n_sen)
    B = rep * len(n_sen)
    ns_all = np.tile(n_sen, rep)
    row_off = torch.from_numpy(np.concatenate([[0], np.cumsum(ns_all)]).astype(np.int32)).to(dev)
    max_slots = int(n_sen.max())
    if use_idx:
        def words16(a8, width=8):
            out = np.full((a8.shape[0], width), 0xFFFF, np.uint16)
            out[:, :a8.shape[1]] = np.where(a8 == 0xFF, 0xFFFF, a8.astype(np.uint16))
            return out
        sw_np, qw_np = words16(g["story_words"]), words16(g["question_words"])
        sw = torch.from_numpy(np.tile(sw_np, (rep, 1)).view(np.int16)).to(dev)
        qw = torch.from_numpy(np.tile(qw_np, (rep, 1)).view(np.int16)).to(dev)
        ans = torch.from_numpy(np.tile(g["answer"].astype(np.int32), rep)).to(dev)
    else:
        story = torch.from_numpy(np.tile(g["story"].astype(np.float32), (rep, 1))).to(dev)
        ques = torch.from_numpy(np.tile(g["question"].astype(np.float32), (rep, 1))).to(dev)
        ans = torch.from_numpy(np.tile(g["answer"].argmax(1).astype(np.int32), rep)).to(dev)
    torch.cuda.synchronize()                                     # hm: the library's own host object, one call per batch

    def step():
        if not use_idx:                                          # float rows in, as the reference's cuda_data_in pools hold them
            pred, cost, match = hm.forward_bow(story, ques, row_off, max_slots, ans)
        else:
            pred, cost, match = hm.forward_words(sw, qw, row_off, max_slots, ans)
        return dict(pred=pred, cost=cost, match=match)

    for _ in range(args.warmup):
        out = step()
    torch.cuda.synchronize()
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    rows = int(row_off[-1])
    bytes_in = rows * cfg["dim_input"] * 4 + B * cfg["dim_input"] * 4           # BoW floats read by the embedding
    if use_idx:
        bytes_in = rows * 8 * 2 + B * 8 * 2                                      # uint16 word lists
    res = {
        "metric": "queries/sec", "value": world * B * args.steps / elapsed, "unit": "queries/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "int8",
        "data": ("bAbI qa1 test set, all 1 000 stories (babi_qa1_test1000_words.npz, vectorised by the reference's sample.c), replicated; seeded random weights"
                 if use_idx else "bAbI qa1 test stories (64-story fixture from the reference's sample.c, replicated), seeded random weights"),
        "config": {"workload": name, "slots": f"{int(n_sen.min())}..{max_slots} (mean {n_sen.mean():.1f})", "stories": len(n_sen),
                   "dim_emb": 60, "dim_input": cfg["dim_input"],
                   "hops": 3, "queries_per_gpu": B, "format": "Q5.2 + EN_MQ weight formats", "attention_mode": 2,
                   "stages": ("one qmann_model_forward_words call: story embedding (int8 MFMA) + question embedding + hops + answer layer" if use_idx
                              else "one qmann_model_forward_bow call: rows -> word lists on the device (irregular rows redone by the float kernels) + the same stages"),
                   "input": "uint16 word indices" if use_idx else "float bag-of-words",
                   "parallelism": f"replicas x{world}, query-sharded"},
        "roofline": {"bound": "hbm", "kernel": "whole forward (latency bound at these sizes)",
                     "achieved": bytes_in * args.steps / elapsed / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": bytes_in * args.steps / elapsed / 1e9 / HBM_PEAK_GBS, "traffic": None},
        "accuracy_note": "random weights: predictions are compared with the oracle, not with labels",
    }
    keep_outputs(args, res, out)
    shard_report(res, out["pred"], B, rank, world, dev)
    # the batched API takes device pointers; when the host owns the stories, one bulk H2D copy per batch
    # (cuda_data_in's role, lib/layer_cuda.cu:3960-4035) precedes it.  Measured from pinned memory, serial
    # with the compute (no overlap): reported beside `value`, never as `value`.  (--full only)
    if rank == 0 and args.full:
        srcs = [t.cpu().pin_memory() for t in ((sw, qw) if use_idx else (story, ques))] + [row_off.cpu().pin_memory(), ans.cpu().pin_memory()]
        dsts = [torch.empty_like(t, device=dev) for t in srcs]
        torch.cuda.synchronize()
        best = 1e9
        for _ in range(5):
            t1 = time.perf_counter()
            for a_, b_ in zip(srcs, dsts):
                b_.copy_(a_, non_blocking=True)
            torch.cuda.synchronize()
            best = min(best, time.perf_counter() - t1)
        step_s = elapsed / args.steps
        res["host_inputs"] = {"bytes_per_step": int(sum(t.numel() * t.element_size() for t in srcs)), "h2d_ms": best * 1e3,
                              "pcie_inclusive_queries_per_s": B / (step_s + best),
                              "note": "pinned host buffers, copy then compute, no overlap"}
        if use_idx:
            # the same with the copy of batch i+1 overlapping the compute of batch i: two HIP streams, two
            # input buffers, events in both directions (every entry point of the library takes a stream)
            cs, ks = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
            hm2 = model.HostModel.from_params(cfg, *hm.params(), device=str(dev), stream=ks.cuda_stream)   # a second replica from the same blob
            bufs = [[torch.empty_like(t, device=dev) for t in srcs] for _ in range(2)]
            copied = [torch.cuda.Event() for _ in range(2)]
            done = [torch.cuda.Event() for _ in range(2)]
            torch.cuda.synchronize()

            def pipelined(n):
                for i in range(n):
                    b = i % 2
                    with torch.cuda.stream(cs):
                        cs.wait_event(done[b])                     # the buffer's previous batch has been consumed
                        for a_, b_ in zip(srcs, bufs[b]):
                            b_.copy_(a_, non_blocking=True)
                        copied[b].record(cs)
                    with torch.cuda.stream(ks):
                        ks.wait_event(copied[b])
                        sw_, qw_, ro_, an_ = bufs[b]
                        o2 = hm2.forward_words(sw_, qw_, ro_, max_slots, an_)
                        done[b].record(ks)
                torch.cuda.synchronize()
                return o2
            pipelined(args.warmup + 1)
            t1 = time.perf_counter()
            o2 = pipelined(args.steps)
            dt = time.perf_counter() - t1
            res["host_inputs"]["overlapped_queries_per_s"] = B * args.steps / dt
            res["host_inputs"]["overlapped_pred_equal"] = bool(torch.equal(o2[0], out["pred"]))
            # SERVING-sized batches: 64 stories per call.  The forward is 6 kernel launches + 3 memsets and never synchronises or
            # allocates once its workspace has its size, so a host can capture it in a HIP graph and replay it per batch
            # (tests/test_gpu_graph.py): per-batch latency, launches one by one against one graph launch
            if not os.environ.get("QMANN_BENCH_NO_SMALL_BATCH"):       # (profile passes: keep the kernel averages those of the full batches)
                nb = 64
                rows_s = int(row_off[nb].item())
                s_sw, s_qw, s_ro, s_an = sw[:rows_s].clone(), qw[:nb].clone(), row_off[:nb + 1].clone(), ans[:nb].clone()
                with torch.cuda.stream(ks):
                    hm2.forward_words(s_sw, s_qw, s_ro, max_slots, s_an)          # (workspace is large enough already: no reallocation)
                ks.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=ks):
                    gp = hm2.forward_words(s_sw, s_qw, s_ro, max_slots, s_an)
                n_it = 300

                def timed(fn):
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    for _ in range(n_it):
                        fn()
                    torch.cuda.synchronize()
                    return (time.perf_counter() - t1) / n_it * 1e6

                def direct():
                    with torch.cuda.stream(ks):
                        hm2.forward_words(s_sw, s_qw, s_ro, max_slots, s_an)
                timed(direct); timed(graph.replay)
                us_d, us_g = timed(direct), timed(graph.replay)
                res["small_batch"] = {"queries": nb, "us_per_batch_direct": us_d, "us_per_batch_graph": us_g,
                                      "pred_equal": bool(torch.equal(gp[0], out["pred"][:nb])),
                                      "note": "back-to-back batches of 64 stories, host clock; graph = one hipGraphLaunch per batch"}
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        offs = np.concatenate([[0], np.cumsum(n_sen)]).astype(np.int64)
        if use_idx:
            V, dd = cfg["dim_input"], int(g["dim_dict"])
            pick = list(range(0, len(n_sen), 5))                          # 200 stories spread over the set
            pool = [(words_to_bow(sw_np[offs[i]:offs[i + 1]], V, dd, True), words_to_bow(qw_np[i:i + 1], V, dd, False)[0]) for i in pick]
            what = f"{len(pick)} of the 1 000 test stories (bag-of-words rows), whole forward"
        else:
            st, qu = g["story"].astype(np.float32), g["question"].astype(np.float32)
            pick = list(range(len(n_sen)))
            pool = [(st[offs[i]:offs[i + 1]], qu[i]) for i in pick]
            what = "the 64 fixture stories (bag-of-words rows), whole forward"
        gp = out["pred"][:len(n_sen)].cpu().numpy()
        res["cpu_baseline"] = cpu_baseline(cfg, wts, pool, what, gpu_preds=[int(gp[i]) for i in pick])
    return res


def words_to_bow(words, V, dim_dict, with_time):
    """uint16 word lists -> the float bag-of-words rows sample.c builds (counts; the time entry is SET to 1)."""
    out = np.zeros((words.shape[0], V), np.float32)
    for r, row in enumerate(words):
        ent = [int(w) for w in row if w != 0xFFFF]
        if with_time and ent:
            t = ent.pop()
            for w in ent:
                out[r, w] += 1.0
            out[r, t] = 1.0
        else:
            for w in ent:
                out[r, w] += 1.0
    return out


def run_joint(args, name, wl, cfg, wts, hm, dev, rank, world, model):
    """configs[2]: 20-task joint bAbI stories, Hamming / dot attention, the whole forward in one library call."""
    g = np.load(ROOT / "tests" / "golden" / "babi_joint20_test2000.npz")
    n_sen = g["n_sen"].astype(np.int64)
    nfix = len(n_sen)
    B = args.queries or wl["B"]
    rep = max(1, B // nfix)
    B = rep * nfix
    sw = torch.from_numpy(np.tile(g["story_words"], (rep, 1)).view(np.int16)).to(dev)
    qw = torch.from_numpy(np.tile(g["question_words"], (rep, 1)).view(np.int16)).to(dev)
    ans = torch.from_numpy(np.tile(g["answer"].astype(np.int32), rep)).to(dev)
    row_off = torch.from_numpy(np.concatenate([[0], np.cumsum(np.tile(n_sen, rep))]).astype(np.int32)).to(dev)
    max_slots = int(n_sen.max())
    torch.cuda.synchronize()
    for _ in range(args.warmup):
        out = hm.forward_words(sw, qw, row_off, max_slots, ans)
    torch.cuda.synchronize()
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = hm.forward_words(sw, qw, row_off, max_slots, ans)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    rows = int(row_off[-1])
    bytes_in = (rows + B) * 16 * 2
    res = {
        "metric": "queries/sec", "value": world * B * args.steps / elapsed, "unit": "queries/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "int8",
        "data": "bAbI 20-task joint test stories (2 000-story fixture made by the reference's sample.c, replicated), seeded random weights",
        "config": {"workload": name, "slots": f"2..{max_slots} (mean {n_sen.mean():.1f})", "dim_emb": cfg["dim_emb"],
                   "dim_input": cfg["dim_input"], "hops": cfg["n_hop"], "queries_per_gpu": B,
                   "format": "Q5.2; weights Q6.1 / Q5.2 / Q4.3 (EN_MQ)" if wl.get("mq") else "Q5.2",
                   "attention_mode": cfg["attention_mode"], "num_bit": cfg.get("num_bit", 8),
                   "stages": "one qmann_model_forward_words call: story embedding (int8 MFMA) + question embedding + hops + answer layer",
                   "weight_tying": "layer-wise (hop 0's embedding matrices on every hop): one shared memory plane" if wl.get("tied") else "none (independent matrices per hop)",
                   "parallelism": f"replicas x{world}, query-sharded"},
        "roofline": {"bound": "hbm", "kernel": "whole forward (issue / latency bound at these sizes)",
                     "achieved": bytes_in * args.steps / elapsed / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": bytes_in * args.steps / elapsed / 1e9 / HBM_PEAK_GBS, "traffic": None},
        "accuracy_note": "random weights: predictions are compared with the oracle, not with labels",
    }
    keep_outputs(args, res, dict(zip(("pred", "cost", "match"), out)))
    shard_report(res, out[0], B, rank, world, dev)
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        V, dd = cfg["dim_input"], int(g["dim_dict"])
        offs = np.concatenate([[0], np.cumsum(n_sen)]).astype(np.int64)
        pick = list(range(0, nfix, max(1, nfix // 200)))[:200]               # spread over the 20 tasks
        pool = [(words_to_bow(g["story_words"][offs[i]:offs[i + 1]], V, dd, True),
                 words_to_bow(g["question_words"][i:i + 1], V, dd, False)[0]) for i in pick]
        gp = out[0][:nfix].cpu().numpy()
        res["cpu_baseline"] = cpu_baseline(cfg, wts, pool, f"{len(pick)} fixture stories spread over the 20 tasks, whole forward",
                                           gpu_preds=[int(gp[i]) for i in pick])
    return res


def run_trained(args, name, wl, dev, rank, world, model, abi, replicate_model):
    """configs[1] with trained weights and labels: the whole forward from word indices, test error from the labels."""
    import tempfile
    tdir = ROOT / "tests" / "golden" / "trained_qa1"
    rec = json.loads((tdir / "reference_run.json").read_text())
    g = np.load(ROOT / "tests" / "golden" / "babi_qa1_en1k_sets.npz")
    with tempfile.TemporaryDirectory() as td:
        tr, te = Path(td) / "train_set", Path(td) / "test_set"
        tr.write_bytes(g["train_set"].tobytes()); te.write_bytes(g["test_set"].tobytes())
        ds = abi.load_dataset(tr, te, 50)                       # include/qmann_dataset.h: record files -> word lists
    V, D, H = ds["dim_input"], 60, 3
    cfg = model.babi_cfg(V, attention_mode=2, softmax_base=0, iwl=int(rec["argv"][3]), n_hop=H, D=D, en_mq=True)
    wts, hm = None, None
    if rank == 0:
        wts = model.load_weights(tdir, cfg)
        hm = model.HostModel(cfg, wts, device=str(dev))
    hm, bcast_ms, bcast_how = replicate_model(hm, cfg, dev, rank, world, COMM, model)
    nq = ds["n_query"]
    B = args.queries or wl["B"]
    rep = max(1, B // nq)
    B = rep * nq
    n_sen = np.diff(ds["row_off"].astype(np.int64))
    sw = torch.from_numpy(np.tile(ds["story_words"], (rep, 1)).view(np.int16)).to(dev)
    qw = torch.from_numpy(np.tile(ds["question_words"], (rep, 1)).view(np.int16)).to(dev)
    ans = torch.from_numpy(np.tile(ds["answer"].astype(np.int64).astype(np.int32), rep)).to(dev)
    row_off = torch.from_numpy(np.concatenate([[0], np.cumsum(np.tile(n_sen, rep))]).astype(np.int32)).to(dev)
    max_slots = int(n_sen.max())
    torch.cuda.synchronize()
    for _ in range(args.warmup):
        out = hm.forward_words(sw, qw, row_off, max_slots, ans)
    torch.cuda.synchronize()
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = hm.forward_words(sw, qw, row_off, max_slots, ans)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    match = int(out[2].item())                                   # the last step's match counter (zeroed per call)
    err = 1.0 - match / B
    pred1 = out[0][:nq].cpu().numpy()
    bytes_in = (int(row_off[-1]) + B) * ds["story_words"].shape[1] * 2
    res = {
        "metric": "queries/sec", "value": world * B * args.steps / elapsed, "unit": "queries/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "int8",
        "data": "bAbI qa1 (en, 1k) test stories read from the record files (1 000, replicated), labels from the files; weights TRAINED by the "
                "reference's unmodified host program through this library (tests/golden/trained_qa1)",
        "config": {"workload": name, "slots": f"2..{max_slots} (mean {n_sen.mean():.1f})", "dim_emb": D, "dim_input": V, "hops": H,
                   "queries_per_gpu": B, "format": "Q5.2 + EN_MQ weight formats", "attention_mode": 2,
                   "stages": "one qmann_model_forward_words call: story embedding (int8 MFMA) + question embedding + hops + answer layer",
                   "parallelism": f"replicas x{world}, query-sharded"},
        "roofline": {"bound": "hbm", "kernel": "whole forward (issue / latency bound at these sizes)",
                     "achieved": bytes_in * args.steps / elapsed / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": bytes_in * args.steps / elapsed / 1e9 / HBM_PEAK_GBS, "traffic": None},
        "accuracy": {"test_error_from_labels": err, "matches": match, "queries": B,
                     "reference_program_err_test": rec["err_test_result_csv"],
                     "equals_reference_program": bool(abs(err - rec["err_test_result_csv"]) < 1e-6),
                     "reference_run": {k: rec[k] for k in ("binary", "argv", "verify_line", "train_error_first_epoch", "train_error_last_epoch", "epochs")},
                     "chance_error": 5.0 / 6.0},
    }
    keep_outputs(args, res, dict(zip(("pred", "cost", "match"), out)))
    shard_report(res, out[0], B, rank, world, dev)
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        offs = ds["row_off"].astype(np.int64)
        pick = list(range(0, nq, 5))
        pool = [(words_to_bow(ds["story_words"][offs[i]:offs[i + 1]], V, ds["dim_dict"], True),
                 words_to_bow(ds["question_words"][i:i + 1], V, ds["dim_dict"], False)[0]) for i in pick]
        res["cpu_baseline"] = cpu_baseline(cfg, wts, pool, f"{len(pick)} of the 1 000 test stories, whole forward, trained weights",
                                           gpu_preds=[int(pred1[i]) for i in pick])
    return with_bcast(res, None if bcast_ms is None else {"ms": bcast_ms, "how": bcast_how, "bytes": hm.params()[1]})


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", default=None, choices=sorted(WORKLOADS),
                    help="one workload alone (default: synth10k_d128_q25 as the headline; with --full + every BASELINE config under `configs`)")
    ap.add_argument("--full", action="store_true",
                    help="beyond the headline figure: secondary configs, sustained window, CPU baselines, host-input and serving legs")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs as DIR/<name>.npy (float32 / float64, <= 64 MB in all)")
    ap.add_argument("--secondary-cpu-s", type=float, default=1.2, help="CPU-baseline seconds per leg for the secondary configs")
    ap.add_argument("--queries", type=int, default=0, help="queries per GPU (default: the workload's)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="(--full) skip the CPU baselines")
    ap.add_argument("--no-secondary", action="store_true", help="(--full) default line: the headline workload only")
    ap.add_argument("--no-sustained", action="store_true", help="(--full) skip the second, longer timing window")
    ap.add_argument("--sustain-s", type=float, default=2.0, help="length of the sustained window in seconds (default 2)")
    args = ap.parse_args(argv)
    if not args.full:                   # a plain run: set-up, warm-up, the timed steps, the line -- nothing else
        args.no_cpu_baseline = args.no_secondary = args.no_sustained = True
    return args


def free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch_command(n_gpus: int, argv, port: int):
    """The child command + environment additions that start `n_gpus` ranks of this file on one node.
    Pure (no process is started): tests/test_bench_launcher.py checks it."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n_gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), str(Path(__file__).resolve()), *argv]
    env = {"HSA_ENABLE_IPC_MODE_LEGACY": "0", "MASTER_ADDR": "127.0.0.1", "QMANN_BENCH_SELF_LAUNCHED": "1"}
    return cmd, env


def self_launch(args, argv):
    """`--gpus N` with no WORLD_SIZE: start the N ranks as a CHILD process tree and pass its output and exit
    code through.  This parent has made no HIP call (torch is not even imported yet), and it never replaces
    itself: a process that has initialised the GPU must not exec another program on this pool."""
    import subprocess
    cmd, extra = launch_command(args.gpus, argv, free_port())
    env = dict(os.environ)
    env.update(extra)
    env.pop("WORLD_SIZE", None)
    return subprocess.run(cmd, env=env).returncode


def main(argv=None):
    global torch
    argv = list(sys.argv[1:] if argv is None else argv)
    args = parse_args(argv)
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args, argv))

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: start one rank per GPU "
                         f"(torch.distributed.run --nproc-per-node {args.gpus}) or leave WORLD_SIZE unset")
    # QMANN_BENCH_PLUMBING=1: no GPU at all -- the launcher / rendezvous / broadcast / timing skeleton over gloo
    # on CPU tensors (the CPU test of the N > 1 host logic; nothing is measured)
    plumbing = os.environ.get("QMANN_BENCH_PLUMBING") == "1"
    # QMANN_BENCH_REHEARSE=1: every rank on cuda:0 over gloo -- rehearses the N > 1 host logic on a one-GPU box
    rehearse = os.environ.get("QMANN_BENCH_REHEARSE") == "1"
    import torch as _torch
    torch = _torch
    backend = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if plumbing:
            dist.init_process_group("gloo")
        elif rehearse:
            local_rank = 0
            torch.cuda.set_device(0)
            dist.init_process_group("gloo")
        else:
            torch.cuda.set_device(local_rank)
            dist.init_process_group("nccl", device_id=torch.device(f"cuda:{local_rank}"))
        backend = dist.get_backend()
    if plumbing:
        out = run_plumbing(args, rank, world)
    else:
        dev = torch.device(f"cuda:{local_rank}")
        torch.cuda.set_device(dev)
        load_pkg()
        global COMM
        comm_info = None
        if world > 1 and not rehearse:
            # the library's own communicator (ncclCommInitRank inside libqmann_hip.so); torch.distributed carried the id
            from qmann_amd.parallel import Comm
            try:
                COMM = Comm(rank, world, local_rank)
                comm_info = COMM.info()
            except Exception as e:                                   # (the line then says so; the blob goes through the process group)
                COMM, comm_info = None, {"error": f"C-level RCCL rendezvous failed: {e}"}
            # every rank must take the same road: one rank without a communicator sends all of them to the process group
            import torch.distributed as dist
            ok = torch.tensor([1 if COMM is not None else 0], device=dev)
            dist.all_reduce(ok, op=dist.ReduceOp.MIN)
            if int(ok.item()) == 0 and COMM is not None:
                COMM.close()
                COMM, comm_info = None, {"error": "another rank could not join the C-level communicator"}
        default_line = args.workload is None
        name = args.workload or HEADLINE
        out = run_workload(args, name, dev, rank, world)
        outputs = out.pop("_outputs", None)
        if args.dump_outputs and rank == 0:
            dump_outputs(args.dump_outputs, outputs)
        # BASELINE.json quotes its metric at |mem| = 50 (the bAbI cap) and sets its target at |mem| = 10 000: the default
        # line's `value` is the 10 000-slot configuration; beside it, under `configs`, one object per BASELINE.json config
        # (SECONDARY above), all timed inside this one driver-clocked run; the |mem| = 50 figures are top-level keys too
        if default_line and not args.no_secondary:
            global CPU_BUDGET_S
            CPU_BUDGET_S = args.secondary_cpu_s
            cfgs = {}
            for key, wname, sus in SECONDARY:
                torch.cuda.empty_cache()
                # (--queries, when given, caps every workload of the line: small rehearsals of the whole line)
                a2 = argparse.Namespace(**{**vars(args), "queries": min(args.queries, WORKLOADS[wname]["B"]) if args.queries else 0,
                                           "no_sustained": args.no_sustained or not sus, "sustain_s": 1.0, "dump_outputs": None})
                try:
                    sec = run_workload(a2, wname, dev, rank, world)
                except Exception as e:                             # one config failing must not cost the line its other five
                    if world > 1:
                        raise                                      # (N > 1: a rank that skipped a workload would leave the others in its collectives)
                    cfgs[key] = {"error": f"{type(e).__name__}: {e}"[:200], "config": {"workload": wname}}
                    continue
                if rank == 0:
                    cfgs[key] = compact(sec)
            if rank == 0:
                out = compact(out, primary=True)
                out["configs"] = cfgs
                m50 = cfgs["mem50"]
                out["config"]["value_is"] = "BASELINE configs[3] as SURVEY 8(d) specifies it (Q2.5, codes N(0,6)), one GPU's shard; BASELINE metric size |mem|=50: mem50_* keys"
                if "value" in m50:
                    out["mem50_queries_per_s"] = m50["value"]
                    out["mem50_roofline_frac"] = m50["roofline"]["frac"]
                    out["mem50_kernel_ms"] = m50["roofline"]["kernel_ms"]
                    out["config"]["mem50"] = {"queries_per_s": m50["value"], "roofline_frac": m50["roofline"]["frac"]}
    if rank == 0:
        if world > 1:
            out["collective"] = {"backend": backend, "world_size_seen": world,
                                 "library": "RCCL over xGMI" if backend == "nccl" else "gloo (rehearsal / plumbing: not RCCL)",
                                 "self_launched": os.environ.get("QMANN_BENCH_SELF_LAUNCHED") == "1"}
            if not plumbing and comm_info:
                out["collective"]["qmann_comm"] = comm_info      # the C-level communicator the parameter broadcast ran on
        print(json.dumps(out), flush=True)
    if COMM is not None:
        COMM.close()
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()


def rank_stats(world, dev, **vals):
    """min / max over ranks of per-rank figures (one small all-gather; rank 0 reports them)."""
    if world == 1:
        return None
    import torch.distributed as dist
    names = sorted(vals)
    t = torch.tensor([float(vals[n]) for n in names], dtype=torch.float64, device=dev)
    parts = [torch.empty_like(t) for _ in range(world)]
    dist.all_gather(parts, t)
    m = torch.stack(parts).cpu().numpy()
    return {n: {"min": float(m[:, i].min()), "max": float(m[:, i].max())} for i, n in enumerate(names)}


def run_plumbing(args, rank, world):
    """The N > 1 host logic with no GPU: rank 0 holds the committed QUANTISED parameter blob of the trained task-1 model
    (tests/golden/trained_qa1/params_q.blob: the bytes qmann_comm_broadcast_params moves on GPUs), it is broadcast once over
    gloo and vetted on every rank with the library's host-side qmann_params_validate; then a barrier-bracketed timed region,
    max over ranks, per-rank statistics.  Measures nothing."""
    import zlib
    load_pkg()
    from qmann_amd import parallel as par
    dev = torch.device("cpu")
    blob_file = ROOT / "tests" / "golden" / "trained_qa1" / "params_q.blob"
    raw, bcast_ms = blob_file.read_bytes() if rank == 0 else None, None
    if world > 1:
        raw, bcast_ms = par.broadcast_blob(raw, rank, world, dev)
    net = par.blob_net(raw)                                          # (validates; the dimensions come out of the blob)
    B = 64
    lo, hi = par.shard_range(B * world, rank, world)
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        pass
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    out = {"metric": "plumbing (nothing measured)", "value": 0.0, "unit": "queries/s", "n_gpus": world,
           "steps": args.steps, "warmup": args.warmup, "ms_per_step": elapsed / max(args.steps, 1) * 1e3,
           "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "int8", "data": "none",
           "config": {"workload": "plumbing", "shard": [lo, hi], "parallelism": f"replicas x{world}, query-sharded",
                      "blob": {"bytes": len(raw), "dim_emb": net["dim_emb"], "dim_input": net["dim_input"], "n_hop": net["n_hop"]}}}
    if bcast_ms is not None:
        out["param_broadcast_ms"] = bcast_ms
        out["param_broadcast"] = {"ms": bcast_ms, "bytes": len(raw), "how": "process-group broadcast of the quantised blob (gloo)"}
    st = rank_stats(world, dev, param_crc32=zlib.crc32(raw), shard_lo=lo, shard_hi=hi, shard_size=hi - lo, rank=rank)
    if st:
        out["ranks"] = st
    return out


def run_workload(args, name, dev, rank, world):
    """One workload: W warm-up steps, K timed steps between barriers, max over ranks; returns the result dict."""
    import qmann_amd.abi as abi
    import qmann_amd.model as model
    from qmann_amd.parallel import replicate_model
    SRC_SHA = sys.modules["qmann_amd"].kernel_sources_sha16()
    if world > 1:
        import torch.distributed as dist

    wl = WORKLOADS[name]
    if wl.get("trained"):
        return run_trained(args, name, wl, dev, rank, world, model, abi, replicate_model)
    S, D, V, mode, nb = wl["S"], wl["D"], wl["V"], wl["mode"], wl["nb"]
    B = args.queries or wl["B"]
    H = 3
    iwl = int(wl.get("iwl", 5))
    frac = 7 - iwl
    sm_base = int(os.environ.get("QMANN_BENCH_SOFTMAX_BASE", "0"))          # (experiments: 1 = 2^x, 2 = exp_plan -- the CPU softmax's bases)
    cfg = model.babi_cfg(V, attention_mode=mode, softmax_base=sm_base, iwl=iwl, n_hop=H, D=D, en_mq=bool(wl.get("bow") or wl.get("mq")))
    cfg["num_bit"] = nb
    if os.environ.get("QMANN_BENCH_NO_LINMAP"):            # experiment: what the in-kernel linear map costs
        cfg["en_lin_map"] = False

    # parameters: created on rank 0 only, turned into the library's model object there, and replicated by ONE broadcast of
    # the model's quantised parameter blob -- qmann_comm_broadcast_params (include/qmann_dist.h: ncclBroadcast inside the
    # library, RCCL over xGMI), the same call a C host makes (examples/forward_sharded.c).  The only collective.
    wts = None
    ans_fmt = (1, 6)
    hm = None
    if rank == 0:
        wts = make_params(cfg, D, V, seed=0x51A44, wh_sigma=(wl["wh_codes"] / (1 << frac)) if "wh_codes" in wl else None)
        rng = np.random.default_rng(0xBAB1)      # embedding matrices (the synthetic-memory workloads carry but do not use them)
        wts["w_q"] = rng.normal(0, 1.0, (D, V)).astype(np.float32)
        wts["w_a"] = [rng.normal(0, 1.0, (D, V)).astype(np.float32) for _ in range(H)]
        wts["w_c"] = [rng.normal(0, 1.0, (D, V)).astype(np.float32) for _ in range(H)]
        if not cfg["en_lin_map"]:
            wts["w_h"] = None
        if wl["ans"] == "i8":                       # answer matrix on an int8 grid -> the MFMA projection is exact
            wts["w_ans"] = (np.clip(np.rint(wts["w_ans"] * 64.0 * 4), -127, 127) / 64.0).astype(np.float32)
        if wl.get("tied"):
            wts["w_a"] = [wts["w_a"][0]] * H
            wts["w_c"] = [wts["w_c"][0]] * H
        hm = model.HostModel(cfg, wts, device=str(dev))
    hm, bcast_ms, bcast_how = replicate_model(hm, cfg, dev, rank, world, COMM, model)
    bcast = None if bcast_ms is None else {"ms": bcast_ms, "how": bcast_how, "bytes": hm.params()[1]}
    if wl.get("joint"):
        return with_bcast(run_joint(args, name, wl, cfg, wts, hm, dev, rank, world, model), bcast)
    net = model.QNet.from_model(cfg, hm)         # hop / answer kernels read the linear maps and W_ans inside hm's blob
    Dp = net.Dp
    w_ans_i8 = net.quantize_i8(net.w_ans, ans_fmt, abi.CODE_TWOS) if wl["ans"] == "i8" else None

    if wl.get("bow"):
        return with_bcast(run_bow(args, name, wl, net, cfg, wts, hm, dev, rank, world, model), bcast)

    # synthetic per-query memories, resident in HBM before the timed region
    gen = torch.Generator(device=dev)
    gen.manual_seed(0x51A44 + data_rank(rank))
    keys = gauss_i8((H, B * S, Dp), wl["sk"], gen, dev, pad_from=D)
    vals = gauss_i8((H, B * S, Dp), wl["sv"], gen, dev, pad_from=D)
    u0 = (torch.randn((B, D), device=dev, generator=gen) * wl["su"]).round_().clamp_(-127, 127) / float(1 << frac)
    row_off = (torch.arange(B + 1, device=dev, dtype=torch.int64) * S).to(torch.int32)
    u_out = torch.empty_like(u0)
    key_row_bytes = Dp
    planes = None
    if mode in (10, 11) and nb < 8:
        planes = net.pack_planes(keys, nb)      # packed binary codes: [H][rows][Dp/64][nb] uint64
        key_row_bytes = Dp // 64 * nb * 8       # (8-bit codes: planes would be no smaller than the bytes, the kernel reads the int8 keys)
    torch.cuda.synchronize()

    def run_hops():
        if planes is not None:
            return net.hops_packed(planes, vals, row_off, S, u0)
        return net.hops(keys, vals, row_off, S, u0, u_out=u_out)

    def run_answer(u):
        if w_ans_i8 is not None:
            return net.answer_i8(u, w_ans_i8, ans_fmt)[0]
        return net.answer(u)[0]

    for _ in range(args.warmup):
        run_answer(run_hops())
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()

    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(args.steps)]
    t0 = time.perf_counter()
    for i in range(args.steps):
        ev[i][0].record()
        u = run_hops()
        ev[i][1].record()
        pred = run_answer(u)
        ev[i][2].record()
    torch.cuda.synchronize()
    elapsed_local = time.perf_counter() - t0                          # this rank's own steps, before it waits for the others
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    # what the caller gets: the final controller state u and the predictions (answer_i8's logits are its workspace)
    step_outputs = {"u": u, "pred": pred}
    if args.dump_outputs:                                             # (u's buffer is written again by the sustained window)
        step_outputs = {k: v.clone() for k, v in step_outputs.items()}

    hop_ms = float(np.mean([e[0].elapsed_time(e[1]) for e in ev]))    # dominant kernel, HIP events
    ans_ms = float(np.mean([e[1].elapsed_time(e[2]) for e in ev]))

    # A second, LONGER window of the same steps (>= 2 s back to back): a fresh box runs the first 0.1 s of a full-rate HBM
    # stream 4-6 % faster than it sustains (clock / power management under 55 % VALU issue on top of the stream), so the
    # short driver-specified window flatters.  Both figures go into the line; DESIGN.md quotes the sustained one first.
    sustained = None
    if not args.no_sustained:
        n_sus = max(args.steps, int(np.ceil(args.sustain_s / max(elapsed_local / args.steps, 1e-6))))
        n_sus = min(n_sus, 20000)
        sev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * n_sus)]
        torch.cuda.synchronize()
        ts = time.perf_counter()
        for i in range(n_sus):
            sev[2 * i].record()
            u = run_hops()
            sev[2 * i + 1].record()
            pred = run_answer(u)
        torch.cuda.synchronize()
        sus_elapsed = time.perf_counter() - ts
        per = np.array([sev[2 * i].elapsed_time(sev[2 * i + 1]) for i in range(n_sus)])
        sustained = {"steps": n_sus, "seconds": sus_elapsed, "ms_per_step": sus_elapsed / n_sus * 1e3,
                     "queries_per_s": world * B * n_sus / sus_elapsed, "kernel_ms": float(per.mean()),
                     "kernel_ms_first_tenth": float(per[: max(1, n_sus // 10)].mean()),
                     "kernel_ms_last_tenth": float(per[-max(1, n_sus // 10):].mean())}
    # ALGORITHMIC bytes: H . |mem| . D key bytes -- the D columns the model has, not the Dp the rows are padded to
    # (D = 60 in 64-byte rows at the bAbI width; at D = 128 / 256 the two are equal).  The padded figure is reported beside it.
    key_row_bytes_alg = key_row_bytes if planes is not None else D
    bytes_per_query = H * S * key_row_bytes_alg                       # key planes: the addressing scan
    bytes_per_query_padded = H * S * key_row_bytes
    if mode == 1:
        bytes_per_query += H * S * D                                  # float read-out streams every value row too
        bytes_per_query_padded += H * S * Dp
    achieved = bytes_per_query * B / (hop_ms * 1e-3) / 1e9
    # HBM traffic from the PMC counters cannot be collected inside this process (rocprofv3 wraps the run): the figure
    # is the one recorded by tools/summarize_profiles.py from a separate `rocprofv3 --pmc FETCH_SIZE` pass of this same
    # command, and the line says so
    traffic, traffic_source = None, None
    tj = ROOT / "profiles" / "traffic.json"
    if tj.exists():
        rec = json.loads(tj.read_text()).get(name)
        if rec and B == wl["B"]:
            # counter figures are quoted only while the kernel sources they were measured on are the loaded library's
            if rec.get("kernel_sources_sha16") == SRC_SHA:
                traffic = rec["traffic_bytes_per_launch"]
                traffic_source = (f"{rec['source']} (a separate rocprofv3 --pmc FETCH_SIZE pass on kernel sources {SRC_SHA}, x2 gfx950 "
                                  "correction; NOT measured in this run)")
            else:
                traffic_source = (f"dropped: {rec['source']} was collected on kernel sources {rec.get('kernel_sources_sha16', '(unstamped)')}, "
                                  f"this library is built from {SRC_SHA}")
    # SURVEY.md 8(d) prices a query at keys + values; the quantised read-out touches only the <= 2^frac surviving
    # value rows (bit-identical to summing all rows), so `achieved` counts the key bytes the scan must stream
    survey_bytes = H * S * (key_row_bytes_alg + D)
    survey_gbs = survey_bytes * B / (hop_ms * 1e-3) / 1e9

    lean = mode != 1 and S <= 64 and Dp == 64 and planes is None
    # (csrc/hops_lean.h::launch_lean: stories of <= 16 rows four to a wavefront; uniform longer ones the four-chunk form with fixed-point scores)
    short_kernel = "k_hops_quad" if (S <= 16 or mode == 2) else "k_hops_lean"
    if mode == 1:
        counted = "keys + values (float read-out streams both)"
    elif lean:
        counted = ("key planes only (the algorithmic figure of the long memories).  The one-wavefront kernel fetches only the value rows "
                   "whose weight code Q(p) is not zero (<= 2^frac per hop) when stories are long next to that bound (mean slots >= 4 . 2^frac: "
                   "this workload at 50 slots), and copies a short story's whole value tile otherwise (`traffic` is then about keys + values)")
    else:
        counted = "key planes only: Q(p) = 0 for all but <= 2^frac rows, the value plane is not streamed"
    if wl["ans"] == "i8":
        answer = {"ms": ans_ms, "int_ops": 2.0 * B * V * D, "tops": 2.0 * B * V * D / (ans_ms * 1e-3) / 1e12,
                  "mfma_int8_peak_tops": 5000.0}
    else:
        answer = {"ms": ans_ms, "kernel": ("k_answer_mfma (float logits from a three-way bf16 split on the matrix cores, within 1e-5)" if V <= 256 and D <= 64
                                           else "k_answer_small (float, serial-order sums)" if V <= 256 else "k_answer (float, serial-order sums)"),
                  "flop": 2.0 * B * V * D, "tflops": 2.0 * B * V * D / (ans_ms * 1e-3) / 1e12}
    out = {
        "metric": "queries/sec", "value": world * B * args.steps / elapsed, "unit": "queries/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "int8", "data": "synthetic",
        "config": {"workload": name, "slots": S, "dim_emb": D, "dim_emb_pad": Dp, "hops": H,
                   "queries_per_gpu": B, "format": f"Q{iwl}.{frac}", "attention_mode": mode,
                   "key_row_bytes": key_row_bytes, "answer_layer": wl["ans"], "dim_answer": V,
                   "parallelism": f"replicas x{world}, query-sharded"},
        "roofline": {"bound": "hbm", "kernel": short_kernel if lean else KERNEL_OF_MODE[mode], "achieved": achieved, "peak": HBM_PEAK_GBS,
                     "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": traffic_source,
                     "algorithmic_bytes_per_launch": bytes_per_query * B, "bytes_per_query": bytes_per_query,
                     "bytes_per_query_padded_rows": bytes_per_query_padded,
                     "frac_padded_rows": bytes_per_query_padded * B / (hop_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                     "bytes_counted": counted,
                     "bytes_per_query_survey_formula": survey_bytes,
                     "frac_by_survey_formula": survey_gbs / HBM_PEAK_GBS,
                     "kernel_ms": hop_ms},
        "answer_layer": answer,
    }
    if wl["ans"] == "i8":
        al = out["answer_layer"]
        al["kernel"] = "k_answer_i8_part + k_answer_i8_combine (one pass: MFMA projection, softmax statistics and arg-max in registers)"
        al["frac_of_int8_peak"] = al["tops"] / 5000.0
        mj = ROOT / "profiles" / "mfma.json"
        if mj.exists():
            rec = json.loads(mj.read_text()).get(name)
            if rec and rec.get("kernel_sources_sha16") == SRC_SHA:   # matrix-pipe occupancy from a separate rocprofv3 --pmc pass of this command on these sources
                al["mfma_busy_frac_counters"] = rec["mfma_busy_frac"]
                al["mfma_counters_source"] = f"{rec['source']} (kernel sources {SRC_SHA}; not measured in this run)"
            elif rec:
                al["mfma_counters_source"] = f"dropped: {rec['source']} was collected on other kernel sources ({rec.get('kernel_sources_sha16', 'unstamped')} != {SRC_SHA})"
    if sustained is not None:
        gbs = bytes_per_query * B / (sustained["kernel_ms"] * 1e-3) / 1e9
        sustained.update(achieved=gbs, frac=gbs / HBM_PEAK_GBS, frac_by_ms_per_step=bytes_per_query * B / (sustained["ms_per_step"] * 1e-3) / 1e9 / HBM_PEAK_GBS,
                         note="same steps as the timed region, run for >= %.1f s back to back on this rank; this rank's figure" % args.sustain_s)
        out["sustained"] = sustained
        out["roofline"]["frac_sustained"] = sustained["frac"]
    st = rank_stats(world, dev, roofline_frac=achieved / HBM_PEAK_GBS, kernel_ms=hop_ms,
                    queries_per_s=B * args.steps / elapsed_local)
    if st:
        out["ranks"] = st
    with_bcast(out, bcast)
    keep_outputs(args, out, step_outputs)
    shard_report(out, pred, B, rank, world, dev)
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        pool = mem_pool(cfg, keys, vals, u0, S, D)
        out["cpu_baseline"] = cpu_baseline(cfg, wts, pool, f"|mem| = {S}, D = {D}, {H} hops + answer layer",
                                           gpu_preds=pred[:len(pool)].cpu().numpy().tolist())
    return out


if __name__ == "__main__":
    main()
