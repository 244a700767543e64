"""Parameter gradients through the ragged content encoder and decoder, measured.  Per network three variants:
  (a) <net>_ragged_live    forward + backward of ``content_encoder_ragged(xs, param_grads=True)`` / ``decoder_ragged(zs, emb,
                           param_grads=True)`` with every parameter of the network live: ONE ragged launch set each way;
  (b) <net>_ragged_frozen  the same call with the parameters frozen and the inputs as leaves (the input-gradient pass that existed);
  (c) <net>_uniform_loop   the loop of one uniform ``content_encoder(x_b)`` / ``decoder(z_b, emb_b)`` forward + backward per utterance
                           with live parameters (B = 1 plans, warm).
The protocol of scripts/ragged_decoder_grad_bench.py and scripts/ragged_content_grad_bench.py.

    python scripts/ragged_param_grad_bench.py --procs 3 --out profiles/ragged_param_grad_bench.json   # three fresh processes, one after the
                                                                                                      # other; all variants alternated in each
    python scripts/ragged_param_grad_bench.py --out one.json                       # one such process

Workload: the 32 source lengths of scripts/enroll_bench.py (17-600 frames), the stock 80-mel config, fp32, weights from the module's seeded
default initialisation; loss = sum(out_j * w_j) with fixed random weights.  Device events around the whole Python call (input
concatenation, autograd bookkeeping, the gradient copies and torch's accumulation into .grad included: what a training loop pays per
step); the variants take turns inside each repetition; median, 10th / 90th percentile and minimum in ms."""
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
    ap.add_argument("--only", default=None, help="comma-separated variants, e.g. decoder_ragged_live,decoder_uniform_loop")
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
        raise SystemExit("ragged_param_grad_bench measures on the GPU; none is visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    _lib.load()
    torch.manual_seed(0)
    model = AE(stock_config(a.mels)).to(dev)
    model.eval()
    rng = np.random.RandomState(3)
    T = [a.lo] + [int(v) for v in rng.randint(a.lo, a.hi + 1, size=a.n - 1)]   # (the source lengths of enroll_bench.py: same stream)
    g = torch.Generator().manual_seed(1)
    xs = [torch.randn(t, a.mels, generator=g).to(dev) for t in T]
    with torch.no_grad():
        mu0, ls0 = model.content_encoder_ragged(xs)
    lat = [int(m.shape[1]) for m in mu0]
    wm, wl = [torch.randn(m.shape, generator=g).to(dev) for m in mu0], [torch.randn(m.shape, generator=g).to(dev) for m in mu0]
    zs = [torch.randn(model._c_lat, n, generator=g).to(dev) for n in lat]
    E = torch.randn(a.n, model._c_emb, generator=g).to(dev)
    with torch.no_grad():
        wd = [torch.randn(o.shape, generator=g).to(dev) for o in model.decode_ragged(zs, E)]
    for mode in ("content_train", "decoder_train"):
        model._plans.capacity[mode] = 2 * a.n   # "plans warm": every length keeps its uniform plan
    x3 = [x.t()[None].contiguous() for x in xs]     # [1, M, T_s]: the uniform plans' input
    z3 = [z[None].contiguous() for z in zs]
    e3 = [E[b:b + 1].contiguous() for b in range(a.n)]
    x_leaves = [x.clone().requires_grad_(True) for x in xs]
    z_leaves = [z.clone().requires_grad_(True) for z in zs]
    e_leaf = E.clone().requires_grad_(True)
    enc_p, dec_p = list(model.content_encoder.parameters()), list(model.decoder.parameters())

    def live(on):
        for p in model.parameters():
            p.requires_grad_(on)
            p.grad = None

    def content_ragged_live():
        live(True)
        mu, ls = model.content_encoder_ragged(xs, param_grads=True)
        (sum((m * v).sum() for m, v in zip(mu, wm)) + sum((s * v).sum() for s, v in zip(ls, wl))).backward()

    def content_ragged_frozen():
        live(False)
        for x in x_leaves:
            x.grad = None
        mu, ls = model.content_encoder_ragged(x_leaves)
        (sum((m * v).sum() for m, v in zip(mu, wm)) + sum((s * v).sum() for s, v in zip(ls, wl))).backward()

    def content_uniform_loop():
        live(True)
        for b, x in enumerate(x3):
            mu, ls = model.content_encoder(x)
            ((mu[0] * wm[b]).sum() + (ls[0] * wl[b]).sum()).backward()

    def decoder_ragged_live():
        live(True)
        outs = model.decoder_ragged(zs, E, param_grads=True)
        sum((o * v).sum() for o, v in zip(outs, wd)).backward()

    def decoder_ragged_frozen():
        live(False)
        e_leaf.grad = None
        for z in z_leaves:
            z.grad = None
        outs = model.decoder_ragged(z_leaves, e_leaf)
        sum((o * v).sum() for o, v in zip(outs, wd)).backward()

    def decoder_uniform_loop():
        live(True)
        for b, z in enumerate(z3):
            (model.decoder(z, e3[b])[0] * wd[b]).sum().backward()

    variants = {f.__name__: f for f in (content_ragged_live, content_ragged_frozen, content_uniform_loop, decoder_ragged_live,
                                        decoder_ragged_frozen, decoder_uniform_loop)}
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
    if not a.only:   # the same gradients either way (different summation orders, statistics from different kernels: fp32 round-off; an
        #              activation decided the other way by the two engines shows as an outlier in a few tensors)
        def grads_of(fn, ps):
            fn()
            torch.cuda.synchronize()
            return [p.grad.detach().clone() for p in ps]
        for net, ps, ra, un in (("content", enc_p, content_ragged_live, content_uniform_loop), ("decoder", dec_p, decoder_ragged_live, decoder_uniform_loop)):
            ga, gu = grads_of(ra, ps), grads_of(un, ps)
            num = sum(float((x - y).norm()) ** 2 for x, y in zip(ga, gu)) ** 0.5
            den = sum(float(y.norm()) ** 2 for y in gu) ** 0.5
            checks[f"{net}_ragged_vs_uniform_whole_gradient_rel_l2"] = num / den
        checks["lengths"] = T
        checks["latent_lengths"] = lat
    res = {"library": os.path.basename(os.path.dirname(_lib.LIB_PATH)) + "/" + os.path.basename(_lib.LIB_PATH),
           "device": torch.cuda.get_device_name(0), "n": a.n, "frames": sum(T), "frames_latent": sum(lat), "mels": a.mels, "compute": "fp32",
           "reps": a.reps, "warmup": a.warmup, "checks": checks,
           "ms": {v: {"median": float(np.median(t)), "p10": float(np.percentile(t, 10)), "p90": float(np.percentile(t, 90)), "min": float(min(t))}
                  for v, t in times.items()}}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
