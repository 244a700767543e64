"""Ragged fan-out, measured: S sources in V voices each, three ways.

    python scripts/fanout_bench.py --procs 3 --out profiles/fanout_bench.json

Workload: the first 8 source lengths of scripts/enroll_bench.py (17-600 frames, seeded) x 8 voices = 64 outputs, the stock 80-mel config,
fp32, weights from the module's seeded default initialisation.  Variants:
  expanded      inference_ragged(64 sources, emb=[64, c]): every source uploaded and encoded 8 times (the only form before fan-out)
  fanout        inference_ragged(8 sources, emb=[64, c], src_of=...): every source uploaded and encoded once
  decode        decode_ragged(cached latents, emb=[64, c], src_of=...): the content codes come from ONE content_latents_ragged call
                outside the timed region (a sentence cached once, rendered later); `encode` is that call, timed on its own
Protocol of scripts/enroll_bench.py: device events around the whole Python call (input concatenation and result clones included), the
variants take turns inside each repetition, median of --reps after --warmup rounds in which every plan is created; --procs N runs N
fresh processes one after the other and reports each."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def measure(a):
    import torch
    from adaptive_voice_conversion_amd import _lib
    from adaptive_voice_conversion_amd.model import AE
    from bench import stock_config
    if not torch.cuda.is_available():
        raise SystemExit("fanout_bench measures on the GPU; none is visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    _lib.load()
    torch.manual_seed(0)
    model = AE(stock_config(a.mels)).to(dev)
    model.eval()
    rng = np.random.RandomState(3)
    T = ([a.lo] + [int(v) for v in rng.randint(a.lo, a.hi + 1, size=31)])[:a.sources]   # (the lengths of enroll_bench.py, first a.sources)
    S, V = len(T), a.voices
    g = torch.Generator().manual_seed(1)
    xs = [torch.randn(t, a.mels, generator=g).to(dev) for t in T]
    voices = torch.randn(V, model._c_emb, generator=g).to(dev)
    m = [s for s in range(S) for _ in range(V)]
    E = voices.repeat(S, 1)
    xs_exp = [xs[s] for s in m]
    with torch.no_grad():
        zs = model.content_latents_ragged(xs)
    variants = {"expanded": lambda: model.inference_ragged(xs_exp, emb=E),
                "fanout": lambda: model.inference_ragged(xs, emb=E, src_of=m),
                "decode": lambda: model.decode_ragged(zs, E, src_of=m),
                "encode": lambda: model.content_latents_ragged(xs)}
    names = list(variants)
    times = {v: [] for v in names}
    with torch.no_grad():
        for _ in range(a.warmup):
            for v in names:
                variants[v]()
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for v in names:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                variants[v]()
                e1.record()
                e1.synchronize()
                times[v].append(e0.elapsed_time(e1))
        p, q, r = variants["expanded"](), variants["fanout"](), variants["decode"]()
        checks = {"fanout_equals_expanded": all(torch.equal(x, y) for x, y in zip(p, q)),
                  "decode_equals_expanded": all(torch.equal(x, y) for x, y in zip(p, r))}
        ws = {k[0]: int(pl.workspace_floats) for k, (pl, _) in model._ragged.items()}
    return {"device": torch.cuda.get_device_name(0), "sources": S, "voices": V, "frames_sources": sum(T), "frames_expanded": sum(T) * V, "mels": a.mels,
            "compute": model.last_ragged_compute, "reps": a.reps, "warmup": a.warmup, "checks": checks, "workspace_floats": ws,
            "ms": {v: {"median": float(np.median(t)), "p10": float(np.percentile(t, 10)), "p90": float(np.percentile(t, 90)), "min": float(min(t))}
                   for v, t in times.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sources", type=int, default=8)
    ap.add_argument("--voices", type=int, default=8)
    ap.add_argument("--lo", type=int, default=17)
    ap.add_argument("--hi", type=int, default=600)
    ap.add_argument("--mels", type=int, default=80)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--procs", type=int, default=1, help="fresh processes, one after the other")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.procs > 1:
        runs = []
        for _ in range(a.procs):
            cmd = [sys.executable, os.path.abspath(__file__)] + [f"--{k}={getattr(a, k)}" for k in ("sources", "voices", "lo", "hi", "mels", "reps", "warmup")]
            out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600).stdout
            runs.append(json.loads(out.strip().splitlines()[-1]))
        res = {"procs": a.procs, "runs": runs}
    else:
        res = measure(a)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
