"""Parameter gradients of the ragged speaker encoder, measured: forward + backward of ``speaker_encoder_ragged`` over 32
utterances of different lengths -- ONE ragged launch set each way -- with the speaker encoder's parameters live, the same with the
parameters frozen (what the weight gradients cost on top), and the loop of one uniform ``speaker_encoder(x_b)`` forward + backward per
utterance (B = 1 plans, warm), which is what a caller had to do for a parameter's .grad before.

    python scripts/ragged_speaker_param_grad_bench.py --procs 3 --out profiles/ragged_speaker_param_grad_bench.json
    python scripts/ragged_speaker_param_grad_bench.py --out one.json        # one such process

The protocol of scripts/ragged_grad_bench.py: the 32 target lengths of scripts/enroll_bench.py (17-600 frames), the stock 80-mel config,
fp32, seeded default initialisation; loss = sum(emb * w) with a fixed random w; device events around the whole Python call; the variants
take turns inside each repetition; median, 10th / 90th percentile and minimum in ms.  In variant (b) every utterance is a leaf (the frozen
pass needs something to differentiate); in (a) and (c) the utterances are plain tensors and the parameters' .grad is reset to None before
every call."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--lo", type=int, default=17)
    ap.add_argument("--hi", type=int, default=600)
    ap.add_argument("--mels", type=int, default=80)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default=None, help="comma-separated variants: ragged_params, ragged_frozen, uniform_loop")
    ap.add_argument("--out", default=None)
    ap.add_argument("--procs", type=int, default=0, help="run the measurement in this many fresh child processes, one after the other, and "
                                                         "collect their records ({'processes': [...]}) in --out")
    a = ap.parse_args()
    if a.procs > 0:
        import subprocess
        args = [x for i, x in enumerate(sys.argv[1:]) if x not in ("--procs", "--out") and sys.argv[i] not in ("--procs", "--out")]
        recs = []
        for _ in range(a.procs):
            out = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, check=True, stdout=subprocess.PIPE, text=True).stdout
            recs.append(json.loads(out.strip().splitlines()[-1]))
        res = {"processes": recs,
               "median_ms": {v: [r["ms"][v]["median"] for r in recs] for v in recs[0]["ms"]}}
        print(json.dumps(res))
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            json.dump(res, open(a.out, "w"), indent=1)
        return

    import torch
    from adaptive_voice_conversion_amd import _lib
    from adaptive_voice_conversion_amd.model import AE
    from bench import stock_config
    if not torch.cuda.is_available():
        raise SystemExit("ragged_speaker_param_grad_bench measures on the GPU; none is visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    _lib.load()
    torch.manual_seed(0)
    model = AE(stock_config(a.mels)).to(dev)
    model.eval()
    spk = list(model.speaker_encoder.parameters())
    rng = np.random.RandomState(3)
    rng.randint(a.lo, a.hi + 1, size=a.n - 1)   # (the source lengths of enroll_bench.py: same stream, same target lengths)
    Tc = [int(v) for v in rng.randint(a.lo, a.hi + 1, size=a.n - 1)] + [a.lo]
    g = torch.Generator().manual_seed(1)
    cs = [torch.randn(t, a.mels, generator=g).to(dev) for t in Tc]
    w = torch.randn(a.n, model._c_emb, generator=g).to(dev)
    model._plans.capacity["speaker_train"] = 2 * a.n   # "plans warm": every length keeps its uniform plan
    leaves = [c.clone().requires_grad_(True) for c in cs]     # [T_b, M]: variant (b)
    cs3 = [c.t()[None].contiguous() for c in cs]              # [1, M, T_b]: the uniform speaker plans' input

    def live(on):
        for p in model.parameters():
            p.requires_grad_(on)
            p.grad = None

    def ragged_params():
        live(True)
        (model.speaker_encoder_ragged(cs) * w).sum().backward()

    def ragged_frozen():
        live(False)
        for x in leaves:
            x.grad = None
        (model.speaker_encoder_ragged(leaves) * w).sum().backward()

    def uniform_loop():
        live(True)
        for b, x in enumerate(cs3):
            (model.speaker_encoder(x) * w[b]).sum().backward()

    variants = {"ragged_params": ragged_params, "ragged_frozen": ragged_frozen, "uniform_loop": uniform_loop}
    names = [v for v in (a.only.split(",") if a.only else variants) if v in variants]
    if not names:
        raise SystemExit(f"none of {a.only} is a variant")
    times = {v: [] for v in names}
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
    checks = {}
    if not a.only:   # the same parameter gradients either way (different summation orders: fp32 round-off)
        ragged_params()
        ga = [p.grad.clone() for p in spk]
        uniform_loop()
        rels = [float((x - p.grad).norm() / p.grad.norm()) for x, p in zip(ga, spk)]
        checks["ragged_vs_uniform_worst_rel_l2"] = max(rels)
        checks["lengths"] = Tc
    res = {"library": os.path.basename(os.path.dirname(_lib.LIB_PATH)) + "/" + os.path.basename(_lib.LIB_PATH),
           "device": torch.cuda.get_device_name(0), "n": a.n, "frames_target": sum(Tc), "mels": a.mels, "compute": "fp32", "reps": a.reps,
           "warmup": a.warmup, "checks": checks,
           "ms": {v: {"median": float(np.median(t)), "p10": float(np.percentile(t, 10)), "p90": float(np.percentile(t, 90)), "min": float(min(t))}
                  for v, t in times.items()}}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
