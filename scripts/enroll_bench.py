"""Enrolment workflow on the ragged engine, measured: conversion from (source, target) pairs against conversion from
embeddings the caller already has, and ragged enrolment against one get_speaker_embeddings call per utterance.

    python scripts/enroll_bench.py --out profiles/enroll_bench.json            # all variants, alternated in ONE process
    AVC_HIP_LIB=/path/to/older/libavc_hip.so python scripts/enroll_bench.py    # an older build of the library: the variants it has
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/enroll_bench.py --only pairs --reps 10 --warmup 2
    python scripts/enroll_bench.py --kernel-sums DIR --calls 12                # kernel-time sum per call from that trace

Workload: N = 32 utterances, lengths uniform in [17, 600] frames (seeded), the stock 80-mel config, fp32, weights from the module's
seeded default initialisation.  Every variant is timed with device events around the whole Python call (input concatenation and the
result clones included: what a caller pays), after a warm-up in which every plan is created; the variants take turns inside each
repetition, so that clock and neighbour effects hit all of them alike.  Reported: median, 10th / 90th percentile and minimum in ms.
A library loaded through AVC_HIP_LIB is measured in a process of its own on purpose: two builds in one process would each create
their helper streams, and the second set lands on other hardware queues (include/avc_hip.h, "Conventions")."""
import argparse
import glob
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def kernel_sums(d, calls):
    """Sum of the kernel times of a rocprofv3 --kernel-trace --stats run, per call of the measured function."""
    import csv
    files = sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True))
    if not files:
        raise SystemExit(f"no *kernel_stats.csv under {d}")
    total, launches, top = 0.0, 0, []
    for f in files:
        for row in csv.DictReader(open(f)):
            ns = float(row["TotalDurationNs"])
            total += ns
            launches += int(row["Calls"])
            top.append((ns, row["Name"][:90], int(row["Calls"])))
    top.sort(reverse=True)
    return {"kernel_ms_per_call": total / 1e6 / calls, "launches_per_call": launches / calls, "calls": calls,
            "top": [{"name": n, "ms_per_call": ns / 1e6 / calls, "launches_per_call": c / calls} for ns, n, c in top[:8]]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--lo", type=int, default=17)
    ap.add_argument("--hi", type=int, default=600)
    ap.add_argument("--mels", type=int, default=80)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default=None, help="comma-separated variants (default: every variant the loaded library has)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-sums", default=None, help="summarise a rocprofv3 output directory instead of measuring")
    ap.add_argument("--calls", type=int, default=1, help="--kernel-sums: calls of the measured function in that run (warm-up + reps)")
    a = ap.parse_args()
    if a.kernel_sums:
        res = kernel_sums(a.kernel_sums, a.calls)
        print(json.dumps(res))
        if a.out:
            json.dump(res, open(a.out, "w"), indent=1)
        return

    import torch
    from adaptive_voice_conversion_amd import _lib
    from adaptive_voice_conversion_amd.model import AE
    from bench import stock_config
    if not torch.cuda.is_available():
        raise SystemExit("enroll_bench measures on the GPU; none is visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lib = _lib.load()
    new = hasattr(lib, "avc_forward_ragged_emb")
    torch.manual_seed(0)
    model = AE(stock_config(a.mels)).to(dev)
    model.eval()
    rng = np.random.RandomState(3)
    T = [a.lo] + [int(v) for v in rng.randint(a.lo, a.hi + 1, size=a.n - 1)]
    Tc = [int(v) for v in rng.randint(a.lo, a.hi + 1, size=a.n - 1)] + [a.lo]
    g = torch.Generator().manual_seed(1)
    xs = [torch.randn(t, a.mels, generator=g).to(dev) for t in T]
    cs = [torch.randn(t, a.mels, generator=g).to(dev) for t in Tc]
    cs3 = [c.t()[None].contiguous() for c in cs]   # [1, M, T'] inputs of the uniform speaker plans
    model.set_plan_cache_size(speaker=2 * a.n)     # "plans warm in both": every length keeps its uniform plan

    variants = {"pairs": lambda: model.inference_ragged(xs, cs),
                "enrol_loop": lambda: torch.cat([model.get_speaker_embeddings(c) for c in cs3])}
    if new:
        with torch.no_grad():
            E = model.get_speaker_embeddings_ragged(cs)
            e1 = E[:3].mean(0)
        variants.update({"emb": lambda: model.inference_ragged(xs, emb=E), "emb_one_voice": lambda: model.inference_ragged(xs, emb=e1),
                         "enrol_ragged": lambda: model.get_speaker_embeddings_ragged(cs)})
    names = [v for v in (a.only.split(",") if a.only else variants) if v in variants]
    if not names:
        raise SystemExit(f"none of {a.only} is available in {_lib.LIB_PATH}")
    times = {v: [] for v in names}
    with torch.no_grad():
        for _ in range(a.warmup):
            for v in names:
                variants[v]()
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for v in names:
                e0, e1_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                variants[v]()
                e1_.record()
                e1_.synchronize()
                times[v].append(e0.elapsed_time(e1_))
        checks = {}
        if new and not a.only:   # same numbers, whichever way they were computed (fp32: bit for bit)
            p, q = model.inference_ragged(xs, cs), model.inference_ragged(xs, emb=E)
            checks["emb_equals_pairs"] = all(torch.equal(x, y) for x, y in zip(p, q))
            loop = torch.cat([model.get_speaker_embeddings(c) for c in cs3])
            checks["enrol_ragged_vs_loop_max_abs"] = float((loop - E).abs().max())
    res = {"library": os.path.basename(os.path.dirname(_lib.LIB_PATH)) + "/" + os.path.basename(_lib.LIB_PATH), "has_part_plans": new,
           "device": torch.cuda.get_device_name(0), "n": a.n, "frames_source": sum(T), "frames_target": sum(Tc), "mels": a.mels,
           "compute": model.last_ragged_compute, "reps": a.reps, "warmup": a.warmup, "checks": checks,
           "ms": {v: {"median": float(np.median(t)), "p10": float(np.percentile(t, 10)), "p90": float(np.percentile(t, 90)), "min": float(min(t))}
                  for v, t in times.items()}}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
