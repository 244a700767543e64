"""Training steps on whole utterances drawn from ``RaggedUtteranceFeed``, measured three ways (DESIGN, "The ragged train step"):
  (a) feed_step       ``next(feed)`` + ``Solver.ae_step_ragged(PackedUtterances, lambda_kl, sync=False)`` with K = 8 templates and the caches
                      raised as ``Solver.train_ragged`` raises them: every template warm (plans, workspaces, tables reused);
  (b) list_step       the SAME batches handed over as lists of [T_j, M] views of the packed block to the list path,
                      ``ae_step_ragged(list, lambda_kl, sync=False)``, on a second solver whose plan cache keeps its default of 4: with eight
                      tuples of lengths in random order most steps create three grad plans, their workspaces and a table set, and pack the
                      rows with ``torch.cat`` -- what a loop over random batches paid before the templates;
  (c) cat_pack / gather_launch   the packing alone: ``torch.cat`` of the 32 views against the upload of the 32 first rows + ONE
                      ``avc_gather_utterances`` launch (``next(feed)``), same batches.
The protocol of scripts/ragged_step_bench.py: --procs fresh processes one after the other, device events around the whole Python call, the
variants take turns inside each repetition, median / 10th / 90th percentile / minimum in ms after warm-up.

    python scripts/ragged_feed_bench.py --procs 3 --out profiles/ragged_feed_bench.json

Workload: a synthetic corpus whose lengths are the 32 lengths of scripts/ragged_step_bench.py (17-600 frames) repeated --repeat times (default once: seven distinct templates), the
stock 80-mel config, fp32, N = 32 utterances per step, optimizer applied (both solvers step, each on its own copy of the model)."""
import argparse
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--lo", type=int, default=17)
    ap.add_argument("--hi", type=int, default=600)
    ap.add_argument("--repeat", type=int, default=1, help="copies of the 32 lengths in the corpus (4 or more: all templates become the same tuple)")
    ap.add_argument("--templates", type=int, default=8)
    ap.add_argument("--mels", type=int, default=80)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=24, help="steps before the measurement: enough for every template to be visited")
    ap.add_argument("--out", default=None)
    ap.add_argument("--procs", type=int, default=0)
    ap.add_argument("--timeout", type=float, default=240.0, help="time limit of each child process of --procs, in seconds")
    a = ap.parse_args()
    if a.procs > 0:
        import subprocess
        skip = ("--procs", "--out", "--timeout")
        args = [x for i, x in enumerate(sys.argv[1:]) if x not in skip and sys.argv[i] not in skip]
        recs = []
        for _ in range(a.procs):   # (a child that fails or runs out of time raises: nothing more is started)
            out = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, check=True, stdout=subprocess.PIPE, text=True,
                                 timeout=a.timeout).stdout
            recs.append(json.loads(out.strip().splitlines()[-1]))
        res = {"processes": recs, "median_ms": {v: [r["ms"][v]["median"] for r in recs] for v in recs[0]["ms"]}}
        print(json.dumps(res))
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            json.dump(res, open(a.out, "w"), indent=1)
        return

    import torch
    from adaptive_voice_conversion_amd import _lib
    from adaptive_voice_conversion_amd.device_feed import RaggedUtteranceFeed
    from adaptive_voice_conversion_amd.solver import Solver
    from bench import stock_config
    if not torch.cuda.is_available():
        raise SystemExit("ragged_feed_bench measures on the GPU; none is visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    _lib.load()
    torch.manual_seed(0)
    cfg = stock_config(a.mels)
    ns = lambda: types.SimpleNamespace(store_model_path=None, load_model=False, data_dir=None, logdir="/tmp/avc_ragged_feed_bench_log")
    warm, cold = Solver(cfg, ns()), Solver(cfg, ns())
    K = a.templates
    warm.model.set_ragged_plan_cache(3 * K + 1)   # what Solver.train_ragged does
    warm._rag_tables_cap = K
    rng = np.random.RandomState(3)
    T = [a.lo] + [int(v) for v in rng.randint(a.lo, a.hi + 1, size=a.n - 1)]   # (the lengths of ragged_step_bench.py: same stream)
    g = torch.Generator().manual_seed(1)
    data = {f"u{r}_{j}": torch.randn(t, a.mels, generator=g).numpy() for r in range(a.repeat) for j, t in enumerate(T)}
    feed = RaggedUtteranceFeed(data, a.n, dev, n_templates=K, min_frames=a.lo, seed=0)
    lam_kl = 0.5
    batch = {}

    def gather_launch():
        batch["pk"] = next(feed)
        batch["views"] = list(torch.split(batch["pk"].x, list(batch["pk"].T)))

    def cat_pack():
        return torch.cat(batch["views"]).contiguous()

    def feed_step():
        return warm.ae_step_ragged(batch["pk"], lam_kl, sync=False)

    def list_step():
        return cold.ae_step_ragged(batch["views"], lam_kl, sync=False)

    order = (gather_launch, cat_pack, feed_step, list_step)   # (gather first: the others work on its batch)
    times = {f.__name__: [] for f in order}
    seen = set()
    for _ in range(a.warmup):
        for f in order:
            f()
        seen.add(feed.last_draw[0])
    torch.cuda.synchronize()
    created = {"warm": len(warm.model._ragged), "cold": len(cold.model._ragged)}
    frames = []
    for _ in range(a.reps):
        for f in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            times[f.__name__].append(e0.elapsed_time(e1))
        frames.append(sum(batch["pk"].T))
    res = {"library": os.path.basename(os.path.dirname(_lib.LIB_PATH)) + "/" + os.path.basename(_lib.LIB_PATH),
           "device": torch.cuda.get_device_name(0), "n": a.n, "templates": K, "templates_seen_in_warmup": len(seen),
           "corpus_utterances": len(data), "corpus_frames": int(feed.n_rows), "frames_per_step_mean": float(np.mean(frames)),
           "template_frames": [sum(t) for t in feed.templates], "distinct_templates": len(set(feed.templates)), "mels": a.mels, "compute": "fp32", "reps": a.reps, "warmup": a.warmup,
           "plans_kept": created,
           "ms": {v: {"median": float(np.median(t)), "p10": float(np.percentile(t, 10)), "p90": float(np.percentile(t, 90)), "min": float(min(t))}
                  for v, t in times.items()}}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
