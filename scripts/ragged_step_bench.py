"""A whole-utterance training step, gradients only (no optimizer), measured three ways:
  (a) step_ragged     ``Solver.ae_step_ragged(utts, lambda_kl, eps, apply=False, sync=False)``: the three ragged grad plans with the
                      packed-row loss kernels between them, gradients written straight into ``model.flat_grads()``;
  (b) step_autograd   the composition that existed: ``content_encoder_ragged(param_grads=True)`` + ``speaker_encoder_ragged`` +
                      ``decoder_ragged(param_grads=True)``, the same eps applied in torch, the loss written in torch on the lists of views,
                      ONE ``backward()`` (every parameter live, ``.grad`` reset before the call);
  (c) step_uniform    32 uniform B = 1 ``forward`` + ``loss`` + ``backward`` calls with warm plans.  The uniform loss needs T % 8 == 0, so
                      utterance j is cropped to 8 floor(T_j / 8) frames there (at least 24; up to 7 frames less work per utterance than
                      (a) and (b)), and every call overwrites the flat gradient buffer (no sum over the utterances).
The protocol of scripts/ragged_param_grad_bench.py.

    python scripts/ragged_step_bench.py --procs 3 --out profiles/ragged_step_bench.json   # three fresh processes, one after the other, each
                                                                                          # under its own time limit; a failure stops the run
    python scripts/ragged_step_bench.py --out one.json                                    # one such process

Workload: the 32 source lengths of scripts/enroll_bench.py (17-600 frames), the stock 80-mel config, fp32, weights from the module's seeded
default initialisation, every utterance its own speaker reference.  Device events around the whole Python call; the variants take turns
inside each repetition; median, 10th / 90th percentile and minimum in ms."""
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
    ap.add_argument("--mels", type=int, default=80)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default=None, help="comma-separated variants, e.g. step_ragged,step_autograd")
    ap.add_argument("--out", default=None)
    ap.add_argument("--procs", type=int, default=0, help="run the measurement in this many fresh child processes, one after the other, and "
                                                         "collect their records ({'processes': [...]}) in --out")
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
        res = {"processes": recs,
               "median_ms": {v: [r["ms"][v]["median"] for r in recs] for v in recs[0]["ms"]}}
        print(json.dumps(res))
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            json.dump(res, open(a.out, "w"), indent=1)
        return

    import torch
    from adaptive_voice_conversion_amd import _lib
    from adaptive_voice_conversion_amd.solver import Solver
    from bench import stock_config
    if not torch.cuda.is_available():
        raise SystemExit("ragged_step_bench measures on the GPU; none is visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    _lib.load()
    torch.manual_seed(0)
    cfg = stock_config(a.mels)
    solver = Solver(cfg, types.SimpleNamespace(store_model_path=None, load_model=False, data_dir=None, logdir="/tmp/avc_ragged_step_bench_log"))
    model = solver.model
    model.eval()
    lam_rec, lam_kl = float(cfg["lambda"]["lambda_rec"]), 0.5
    rng = np.random.RandomState(3)
    T = [a.lo] + [int(v) for v in rng.randint(a.lo, a.hi + 1, size=a.n - 1)]   # (the source lengths of enroll_bench.py: same stream)
    g = torch.Generator().manual_seed(1)
    xs = [torch.randn(t, a.mels, generator=g).to(dev) for t in T]
    with torch.no_grad():
        lat = [int(m.shape[1]) for m in model.content_encoder_ragged(xs)[0]]
    c = model._c_lat
    eps = torch.randn(c * sum(lat), generator=g).to(dev)
    eps_b, o = [], 0
    for n in lat:
        eps_b.append(eps[c * o:c * (o + n)].view(c, n))
        o += n
    x_all = torch.cat([x.t().reshape(-1) for x in xs])
    model._plans.capacity["train"] = 2 * a.n   # "plans warm": every length keeps its uniform plan
    T8 = [max(24, t // 8 * 8) for t in T]   # (24: three latent frames, the least the decoder's reflect padding takes)
    x3 = [torch.cat([x, x])[:t].t()[None].contiguous() for x, t in zip(xs, T8)]     # [1, M, T8_j]: the uniform plans' input
    e3 = [torch.randn(1, c, t // 8, generator=g).to(dev) for t in T8]
    flat, grads = model.flat_parameters(), model.flat_grads()

    def live(on):
        for p in model.parameters():
            p.requires_grad_(on)
            p.grad = None

    def step_ragged():
        return solver.ae_step_ragged(xs, lam_kl, eps=eps, apply=False, sync=False)

    def step_autograd():
        live(True)
        mu, ls = model.content_encoder_ragged(xs, param_grads=True)
        emb = model.speaker_encoder_ragged(xs)
        dec = model.decoder_ragged([m + torch.exp(s / 2) * e for m, s, e in zip(mu, ls, eps_b)], emb, param_grads=True)
        dec_all = torch.cat([d[:, :x.shape[0]].reshape(-1) for d, x in zip(dec, xs)])
        mu_all, ls_all = torch.cat([m.reshape(-1) for m in mu]), torch.cat([s.reshape(-1) for s in ls])
        loss_rec, loss_kl = (dec_all - x_all).abs().mean(), 0.5 * torch.mean(torch.exp(ls_all) + mu_all ** 2 - 1 - ls_all)
        (lam_rec * loss_rec + lam_kl * loss_kl).backward()
        return loss_rec, loss_kl

    def step_uniform():
        for x, e, t in zip(x3, e3, T8):
            plan, ws = model._plan(1, t, t, dev)
            plan.forward(flat, x, None, e, ws)
            plan.loss(x, lam_rec, ws)
            plan.backward(flat, x, None, e, grads, ws, lambda_kl=lam_kl)

    variants = {f.__name__: f for f in (step_ragged, step_autograd, step_uniform)}
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
    if not a.only:   # the same losses and the same whole gradient either way (different summation orders: fp32 round-off)
        ra = step_ragged()
        torch.cuda.synchronize()
        ga = grads.detach().clone()
        au = step_autograd()
        torch.cuda.synchronize()
        num = sum(float((ga[o:o + n].view(s) - p.grad).norm()) ** 2 for (o, n, s), p in zip(model._layout, model.parameters())) ** 0.5
        den = sum(float(p.grad.norm()) ** 2 for p in model.parameters()) ** 0.5
        checks = {"ragged_vs_autograd_whole_gradient_rel_l2": num / den,
                  "loss_rec": [float(ra["loss_rec"]), float(au[0])], "loss_kl": [float(ra["loss_kl"]), float(au[1])],
                  "lengths": T, "latent_lengths": lat}
    res = {"library": os.path.basename(os.path.dirname(_lib.LIB_PATH)) + "/" + os.path.basename(_lib.LIB_PATH),
           "device": torch.cuda.get_device_name(0), "n": a.n, "frames": sum(T), "frames_uniform": sum(T8), "frames_latent": sum(lat),
           "mels": a.mels, "compute": "fp32", "reps": a.reps, "warmup": a.warmup, "checks": checks,
           "ms": {v: {"median": float(np.median(t)), "p10": float(np.percentile(t, 10)), "p90": float(np.percentile(t, 90)), "min": float(min(t))}
                  for v, t in times.items()}}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
