"""Every layer of the bf16 storage engine (compute_dtype "bf16s", AVC_PLAN_BF16S) against ONE rounding.

The whole-plan bf16 bars of tests/test_graded_configs.py are 3e-2 / 1e-1 wide because rounding noise compounds through 13 layers; an
error of 1-3 % made by the plan itself (a wrong ping-pong buffer, a residual taken on the wrong side of a rounding point, a truncating
store, statistics of the wrong tensor, a tile that mixes two short samples) passes them.  Here the compounding is taken out: a training
plan keeps every layer's stored output (``Plan.site``), so each layer is recomputed in float64 FROM THE ENGINE'S OWN STORED INPUT to it
(tests/site_replay.py, oracle.avc_oracle.forced_sites) and its stored output is held to what one correct layer may differ by.

Bounds.  r64 = the float64 layer result on the forced operands, r32 = the float32 torch evaluation of the same layer on the same
operands, ulp(r) = 2^(floor(log2 |r|) - 7), margin = 4 x max over the tensor of |r32 - r64| (fp32 accumulation: the factor allows for
the matrix core's other summation order; split-K adds at most log2 more terms).  The margin is taken over the compared tensor and not
element by element: the fp32 error of ONE element is a random number with density at zero, so the ratio of two correct
implementations' errors at the same element is unbounded -- the worst element of the tensor is the smallest quantity of the twin that
bounds a correct kernel.  [the literal element-by-element share is printed with every case: see the table]
  (a) bf16-stored tensors: |engine - bf16(r64)| <= ulp(r64) + margin per element.  Layers whose every input is an engine tensor
      ("clean": bank members, in_convs, a conv behind a stored activation or a named block output) allow no exception.  Layers behind
      a tensor the replay had to recompute (a1 / unnamed out[l] are not in the site table; the speaker encoder's out[l + 1] too: the
      engine forms it from the conv's UNROUNDED activation, csrc/conv_shared.h:732,738, which no stored tensor holds) see a few inputs
      on the other side of a rounding boundary.  For them the share of elements beyond the bound is capped at 0.5 % -- and the float32
      twin of the replay (bf16(r32) in the engine's place) must itself stay inside that, asserted FIRST: the cap is a condition, not
      a fitted number.  A cap of "3 ulps" on those elements cannot hold for a correct engine: one flipped input moves an output by
      |w| x ulp(input), which is many ulps OF THE OUTPUT wherever the output is small (measured on the MI355X, m80 B = 4: 13.1 /
      14.7 / 17.0 x the bound at 3 - 5 of 32768 elements of the speaker encoder's conv1 outputs, blocks 2 - 4, while the twin of that
      seed stayed below 3).  These sites get their own stated bound instead.  The rounding that cannot be replayed exactly is the store
      of a1 / out[l + 1] (adaptive_voice_conversion_amd/csrc/rowops_pairs.hip:169, csrc/conv_shared.h:510 and :738).  The engine rounded
      ITS fp32 value of such a tensor; that value lies within WINDOW_FACTOR (4) x the float32 twin's worst distance from float64 over the
      same pre-rounding tensor (``_analyse``: the twin runs first and logs them), plus what the residual inside it may differ by.  Where
      the two ends of that window round to different bf16 values the engine's element may be either; that distance travels with the
      tensor, the conv that reads it adds sum |w| x distance to its record as an allowance, and with it NO element may exceed the
      bound.  The share of elements that CONSUME an allowance (beyond the plain bound) is asserted <= 0.5 %, engine and twin; this is
      what a defect trips.  The window is a per-tensor worst case, so small elements are flagged generously: nearly every output
      RECEIVES some allowance and for up to 0.8 of a tensor's elements it at least doubles the bound (printed per tensor as
      "receiving") -- the allowance keeps correct engines from failing, the 0.5 % cap is the check.
      fp32 tensors (dense stack, cond, emb, muls, dec): |engine - r64| <= margin, no ulp term.  The dense stack's float32 twin sums
      term after term like the engine's one accumulator chain (csrc/dense.hip:78): against torch's blocked sgemm the engine's emb sat
      at 1.07 x the margin in one of 384 elements on the fp32 plan.
  (b) rounding mode: mean over the elements of sign(r64) (engine - r64) / ulp(r64) within +-4 / sqrt(12 N) of 0 for every bf16 site
      (round-to-nearest is unbiased, truncation sits at -0.5); elements with |r64| <= margin have no defined sign and stay out; sites
      with N < 4096 are pooled per network.
  (c) the stored mean / rstd of every InstanceNorm site against the float64 statistics OF THE STORED y (eps = 1e-5, avc_common.h
      AVC_IN_EPS): the kernels take them from the rounded values (csrc/conv_shared.h:454-470, csrc/rowops_pairs.hip:96-145), which is
      what the header's "statistics ... stay fp32" means: fp32 arithmetic on the stored tensor.  Margin as above.
  (d) heads: emb, cond, muls, dec (fp32) and z from the engine's muls and eps, from the forced spk_outN / emb / enc_outN / dec_outN.
  (e) the same replay on an fp32 plan, oracle without operand rounding: every tensor within the fp32 margin, zero ulp allowance --
      the replay is proven neutral before it judges bf16.
  (f) local weight gradients after one avc_backward: both operands of decoder.out_conv_layer (dec_outN x d_dec) and of
      content_encoder.mean_layer / std_layer (enc_outN x d_muls) survive the backward pass in named buffers of their own (engine.hip
      allocates out[l], ddec and dmuls once and the backward pass only reads the first two and writes dmuls once; the kernels read the
      bf16 pair copies engine.hip:1593 / :1767 make of d_dec / d_muls, bias gradients are row sums of the same pair tiles,
      conv_wgrad.hip:416).  rel-L2(engine, float64) <= 4 x rel-L2(float32 torch, float64): bf16 x bf16 products are exact in fp32, only
      the summation order separates a correct kernel from this reference.  No other parameter qualifies: every other layer's dy lives
      in the shared dy arena / gradient temporaries and its forward input is not a named buffer.

Worst observed |error| / bound, seed 0 ([sim] = CPU simulator, [gpu] = MI355X; every case prints them per tensor):
  bf16 plan, bf16-stored tensors   clean: 1.000 [sim] 1.000 [gpu]; recomputed input: 0.998 / 0.999, share consuming an allowance
                                   0 [sim], <= 1.5e-4 [gpu, m80 only] (1.000 = exactly one ulp: the other side of a boundary)
  fp32 tensors of both plans       activations and conv outputs 0.72 [sim] 0.89 [gpu], cond 0.92 / 0.85, emb | muls | dec 0.38 / 0.44
                                   (the fp32 plan is (e): no tensor of it is allowed an ulp)
  (b) |mean| / (4 / sqrt(12 N))    0.64 [sim] 0.68 [gpu] over 102 sites and pools
  (c) statistics                   0.53 [sim] 0.59 [gpu]
  (f) weight / bias gradients      rel-L2 engine / twin 1.00 / 1.00 (both are the correctly rounded sums at these sizes)
  share of elements beyond the LITERAL elementwise margin: 5 - 18 % of every fp32 tensor on both backends, 0 of the bf16-stored ones.
Deliberately broken simulator builds (tiny B = 5), not committed: truncating ``bh_pack`` -- (b) at -0.8 .. -8.8 ulp against +-0.016,
(a) 13 - 60 % of the elements of every tensor beyond the bound, (f) 2.9e-3 against 2e-7; norm and activation of the in-epilogue path
taken from the unrounded accumulator, so that conv2 is fed from an activation that never saw y's rounding point -- (a) 12 - 26 % of
the elements of the conv2 outputs (sites 19 - 21, 24, 26) beyond the bound, worst 440 - 1670 x, (c) mean 2.8e-4 against a margin of 0.
"""
import math

import pytest
import torch

from adaptive_voice_conversion_amd.engine import Plan
from oracle import avc_oracle as O
from tests import site_replay as R
from tests.emu_util import backend
from tests.test_engine import flat_params, get_cfg

GPU = pytest.mark.gpu

# (cfg, B, T, tuning): odd batch -> short samples share a tile; 128 channels -> split-K groups, rows of 16 / 32 / 64 frames with the
# InstanceNorm inside the conv epilogue (the default, stated) and in the row kernel; the deepest plan
SHAPES = [("tiny", 5, 32, None), ("tiny128", 3, 64, {"conv_in_fuse": 1}), ("tiny128", 3, 64, {"conv_in_fuse": 0}), ("tiny8", 2, 32, None)]
CASES = [pytest.param("emu", *s) for s in SHAPES] + [pytest.param("gpu", *s, marks=GPU) for s in SHAPES]
CASES.append(pytest.param("gpu", "m80", 4, 128, None, marks=GPU))
SEED = 0
CAP_SHARE = 0.005     # the stated cap of (a)

_RUNS = {}
WINDOW_FACTOR = 4.0   # x the float32 twin's distance from float64, like every other margin here


def _engine(kind, cfgname, B, T, tuning, compute):
    """one training forward (+ loss + backward on a bf16 plan) of a plan; everything the checks take from the workspace, on the CPU
    (read after a synchronise)"""
    lib, dev = backend(kind)
    cfg = get_cfg(cfgname)
    sd = O.make_state_dict(cfg, SEED)
    x, eps = O.make_inputs(cfg, B, T, SEED)
    plan = Plan(cfg, B, T, lib=lib, compute_dtype=compute, tuning=tuning)
    bf16 = compute == "bf16s"
    assert plan.pair_storage == bf16
    params = flat_params(plan, sd, dev)
    ws = torch.full((plan.workspace_floats,), float("nan"), device=dev)
    xd, ed = x.to(dev), eps.to(dev)
    plan.forward(params, xd, None, ed, ws)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    sites, named, res = R.read_workspace(plan, ws, cfg)
    raw = dict(cfg=cfg, sd=sd, x=x, eps=eps, sites=sites, named=named, res=res, bf16=bf16, tag=f"{kind}/{cfgname} B={B} T={T} {tuning or ''}")
    if bf16:   # (f): one backward, then the surviving operands and the three layers' gradients
        plan.loss(xd, cfg["lambda"]["lambda_rec"], ws)
        grads = torch.full((plan.param_floats,), float("nan"), device=dev)
        plan.backward(params, xd, None, ed, grads, ws, lambda_kl=1.0)
        if dev.type == "cuda":
            torch.cuda.synchronize()
        g = grads.cpu()
        Cz, M = cfg["ContentEncoder"]["c_out"], cfg["Decoder"]["c_out"]
        raw["grads"] = {k: g[off:off + n].view(shape).clone() for (off, n, shape), k in zip(plan.param_info, sd)}
        raw["d_dec"] = plan.view(ws, "d_dec", (B, M, plan.out_len)).cpu().clone()
        raw["d_muls"] = plan.view(ws, "d_muls", (B, 2 * Cz, plan.latent_len)).cpu().clone()
        _, named2, _ = R.read_workspace(plan, ws, cfg)
        for k in ("enc_outN", "dec_outN"):   # the forward's tensors are still there
            assert torch.equal(named2[k], named[k]), k
    plan.close()
    return raw


def _engine_tensors(raw):
    """(name, tensor) of every tensor taken from the engine"""
    for i, s in enumerate(raw["sites"]):
        for k in ("act", "y", "mean", "rstd", "cond"):
            if s.get(k) is not None:
                yield f"site {i} {k}", s[k]
    for group in ("named", "res", "grads"):
        for k, v in raw.get(group, {}).items():
            yield f"{group} {k}", v
    for k in ("d_dec", "d_muls"):
        if k in raw:
            yield k, raw[k]


def _analyse(raw):
    """the two replays of one engine run.  The workspace and the gradient buffer start as NaN: a site decoded at the wrong offset, a
    tail a kernel never wrote or a statistics slot left untouched shows here, before a NaN could travel through the forced forward"""
    bad = [n for n, t in _engine_tensors(raw) if not torch.isfinite(t).all()]
    assert not bad, f"non-finite values in what the engine left: {bad}"
    nb = len([k for k in raw["sd"] if k.startswith("speaker_encoder.conv_bank.") and k.endswith(".weight")])
    # spk_out0 is the speaker in_conv's activation buffer itself (engine.hip: out[0] = h0): checked as that site, and here that it IS it
    assert torch.equal(raw["named"]["spk_out0"], raw["sites"][nb]["act"])
    args = (raw["cfg"], raw["sd"], raw["x"], raw["eps"], raw["sites"], raw["named"], raw["res"])
    pre32 = []
    rep32 = R.replay(*args, torch.float32, raw["bf16"], pre_log=pre32)
    # how far the engine's own fp32 value of a tensor the replay recomputes may lie from the float64 one: WINDOW_FACTOR x the float32
    # twin's worst distance over that tensor (k-th recomputed tensor of the forward)
    rep64 = R.replay(*args, torch.float64, raw["bf16"], window=lambda k, t: WINDOW_FACTOR * (pre32[k].double() - t).abs().max())
    assert len(rep64) == len(rep32)
    bad = [f"{r['label']}:{r['what']}" for r in rep64 + rep32 if not (torch.isfinite(r["value"]).all() and torch.isfinite(r["engine"]).all())]
    assert not bad, f"non-finite values in the replay: {bad}"
    return dict(raw, rep64=rep64, rep32=rep32)


def _run(kind, cfgname, B, T, tuning, compute):
    key = (kind, cfgname, B, T, str(tuning), compute)
    if key not in _RUNS:
        _RUNS[key] = _analyse(_engine(kind, cfgname, B, T, tuning, compute))
    return _RUNS[key]


def _over(x, bound):
    """x is NOT within bound -- true for a NaN on either side, which `x > bound` is not"""
    return not (x <= bound)


def _judge(r64, r32, twin, plain=False):
    """(|engine - reference| / bound per element, margin) of one record; twin: the float32 evaluation, rounded where the record is
    stored rounded, in the engine's place.  A NaN error gives an infinite ratio."""
    v64, v32 = r64["value"].double(), r32["value"].double()
    margin = WINDOW_FACTOR * (v32 - v64).abs().max().item()
    if r64["storage"] == 0:
        bound = torch.full_like(v64, margin)
        err = ((v32 if twin else r64["engine"].double()) - v64).abs()
    else:
        bound = R.bf16_ulp(v64) + margin
        if r64.get("allow") is not None and not plain:
            bound = bound + r64["allow"].double()
        err = ((R.to_bf16(v32) if twin else r64["engine"].double()) - R.to_bf16(v64)).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    ratio = torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, float("inf")))
    return ratio, margin


def _check_values(run, whats=("act", "y", "out", "cond", "head")):
    """(a) / (d) / (e) over the records of the given kinds"""
    worst, lines, fails = {}, [], []
    for r64, r32 in zip(run["rep64"], run["rep32"]):
        if r64["what"] not in whats:
            continue
        name = f"{r64['label']}:{r64['what']}{'' if r64['clean'] else '*'}"
        twin, _ = _judge(r64, r32, True)
        ratio, margin = _judge(r64, r32, False)
        n = ratio.numel()
        lit = WINDOW_FACTOR * (r32["value"].double() - r64["value"].double()).abs()      # the literal element-by-element margin, for the record
        if r64["storage"] == 0:
            lit_over = ((r64["engine"].double() - r64["value"].double()).abs() > lit).float().mean().item()
        else:
            lit_over = ((r64["engine"].double() - R.to_bf16(r64["value"].double())).abs() > R.bf16_ulp(r64["value"].double()) + lit).float().mean().item()
        recv = cons = 0.0
        if r64["clean"] or r64["storage"] == 0:
            # (fp32 tensors have no rounding boundary to land on the other side of: no exception either way)
            assert r64.get("allow") is None or r64["storage"] == 0, name
            if _over(twin.max().item(), 1.0):
                fails.append(f"{name}: the float32 twin itself is at {twin.max().item():.3f} x the bound")
            if _over(ratio.max().item(), 1.0):
                fails.append(f"{name}: {int((~(ratio <= 1)).sum())} of {n} elements beyond the bound, worst {ratio.max().item():.3f} x (margin {margin:.2e})")
        else:
            # one rounding + margin + the replay's own uncertainty about the recomputed input (forced_sites: "allow"): no exception;
            # the share of elements that CONSUME that allowance (beyond the plain bound) is capped, for the engine and -- first --
            # for the float32 twin; the share that RECEIVES one is printed
            tshare = (~(_judge(r64, r32, True, plain=True)[0] <= 1)).float().mean().item()
            if _over(tshare, CAP_SHARE) or _over(twin.max().item(), 1.0):
                fails.append(f"{name}: the float32 twin leaves the bound (share beyond the plain bound {tshare:.2e}, worst {twin.max().item():.2f} x): choose another seed")
            plain = _judge(r64, r32, False, plain=True)[0]
            cons = (~(plain <= 1)).float().mean().item()
            # an allowance is received almost everywhere (some input of most outputs sits near a boundary) and is almost everywhere a
            # small fraction of an ulp of the output; "received" counts the elements whose bound it at least doubles
            recv = (r64["allow"].double() > R.bf16_ulp(r64["value"].double()) + margin).float().mean().item() if r64.get("allow") is not None else 0.0
            if _over(cons, CAP_SHARE) or _over(ratio.max().item(), 1.0):
                fails.append(f"{name}: share consuming an allowance {cons:.2e} (cap {CAP_SHARE}, worst {plain.max().item():.2f} x the plain bound); with the "
                             f"allowance: {int((~(ratio <= 1)).sum())} of {n} beyond, worst {ratio.max().item():.3f} x")
        grp = (r64["what"], r64["storage"], r64["clean"])
        w = worst.setdefault(grp, [0.0, 0.0, 0.0, 0, 0.0])
        w[0], w[1], w[2], w[3], w[4] = max(w[0], ratio.max().item()), max(w[1], cons), max(w[2], lit_over), w[3] + 1, max(w[4], recv)
        lines.append(f"    {name:>14} storage {r64['storage']} n {n:7d}  worst {ratio.max().item():.3f}  beyond {int((~(ratio <= 1)).sum()):4d}  "
                     f"twin worst {twin.max().item():.3f}  margin {margin:.2e}  allowance: received {recv:.1e} consumed {cons:.1e}  literal-margin misses {lit_over:.1e}")
    print(f"[{run['tag']}] per tensor, |engine - reference| / bound (* = behind a recomputed input):")
    print("\n".join(lines))
    for (what, st, clean), w in sorted(worst.items(), key=str):
        print(f"[{run['tag']}] {what:>5} storage {st} {'clean' if clean else 'recomputed input'}: {w[3]} tensors, worst ratio {w[0]:.3f}, largest share "
              f"receiving an allowance {w[4]:.2e}, consuming one {w[1]:.2e}, beyond the literal elementwise margin {w[2]:.2e}")
    assert lines
    assert not fails, "\n".join(fails)


def _check_rounding(run):
    """(b)"""
    pools, net, fails = {}, "speaker", []

    def stat(name, d):
        n = d.numel()
        mean, bound = d.mean().item(), 4.0 / math.sqrt(12.0 * n)
        print(f"[{run['tag']}] rounding bias {name:>16}: N {n:7d}  mean {mean:+.5f} ulp  bound +-{bound:.5f}  ({abs(mean) / bound:.2f})")
        if _over(abs(mean), bound):
            fails.append(f"{name}: mean signed rounding error {mean:+.5f} ulp over {n} elements, bound {bound:.5f}")

    for r64, r32 in zip(run["rep64"], run["rep32"]):
        if r64["what"] == "head":
            net = {"emb": "content", "muls": "decoder"}.get(r64["label"], net)
        if r64["what"] not in ("act", "y") or r64["storage"] == 0:
            continue
        v64, eng = r64["value"].double(), r64["engine"].double()
        margin = WINDOW_FACTOR * (r32["value"].double() - v64).abs().max().item()
        keep = v64.abs() > margin
        d = (torch.sign(v64) * (eng - v64) / R.bf16_ulp(v64).clamp_min(1e-300))[keep]
        if d.numel() >= 4096:
            stat(f"site {r64['label']}", d)
        else:
            pools.setdefault(net, []).append(d)
    for net, ds in pools.items():
        stat(f"{net} (pooled)", torch.cat(ds))
    assert not fails, "\n".join(fails)


def _check_stats(run):
    """(c)"""
    fails, worst, n = [], 0.0, 0
    for i, s in enumerate(run["sites"]):
        if s["kind"] != 1:
            continue
        for dt in (torch.float64, torch.float32):
            y = s["y"].to(dt)
            mu = y.mean(-1, keepdim=True)
            rstd = 1.0 / torch.sqrt(((y - mu) ** 2).mean(-1, keepdim=True) + O.IN_EPS)
            if dt == torch.float64:
                m64, r64 = mu, rstd
            else:
                m32, r32 = mu.double(), rstd.double()
        for name, eng, v64, v32 in (("mean", s["mean"], m64, m32), ("rstd", s["rstd"], r64, r32)):
            margin = WINDOW_FACTOR * (v32 - v64).abs().max().item()
            d = (eng.double() - v64).abs()
            err = float("nan") if torch.isnan(d).any() else d.max().item()
            worst = max(worst, err / max(margin, 1e-300) if err else 0.0)
            n += 1
            if _over(err, margin):
                fails.append(f"site {i} {name}: |engine - float64 of the stored y| {err:.3e} > margin {margin:.3e}")
    print(f"[{run['tag']}] statistics of the stored y: worst |error| / margin {worst:.3f}")
    assert n
    assert not fails, "\n".join(fails)


def _rel(a, b):
    return ((a.double() - b).norm() / b.norm()).item()


def _check_wgrads(run):
    """(f)"""
    cfg, named = run["cfg"], run["named"]
    Cz = cfg["ContentEncoder"]["c_out"]
    dm = run["d_muls"]
    layers = [("decoder.out_conv_layer", named["dec_outN"], run["d_dec"]), ("content_encoder.mean_layer", named["enc_outN"], dm[:, :Cz]),
              ("content_encoder.std_layer", named["enc_outN"], dm[:, Cz:])]
    fails = []
    for name, xin, dy in layers:
        ref = {}
        for dt in (torch.float64, torch.float32):
            xr, dyr = xin.to(dt), R.to_bf16(dy.to(dt))      # x is stored bf16; dy is rounded by the pair copy the kernel reads
            ref[dt] = (torch.einsum("bmt,bct->mc", dyr, xr).unsqueeze(2), dyr.sum((0, 2)))
        for which, eng, v64, v32 in zip(("weight", "bias"), (run["grads"][name + ".weight"], run["grads"][name + ".bias"]), ref[torch.float64], ref[torch.float32]):
            e, t = _rel(eng, v64), _rel(v32, v64)
            print(f"[{run['tag']}] {name}.{which}: engine rel-L2 vs float64 {e:.3e}; float32 twin {t:.3e}; ratio {e / max(t, 1e-300):.2f}")
            if _over(e, WINDOW_FACTOR * t):
                fails.append(f"{name}.{which}: {e:.3e} > 4 x {t:.3e}")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("kind,cfgname,B,T,tuning", CASES)
def test_fp32_replay_is_neutral(kind, cfgname, B, T, tuning):
    """(e): the hook, the site reader and the margins on an fp32 plan -- every tensor within the fp32 margin, no ulp anywhere"""
    run = _run(kind, cfgname, B, T, tuning, "fp32")
    assert all(r["storage"] == 0 for r in run["rep64"])
    _check_values(run)


@pytest.mark.parametrize("kind,cfgname,B,T,tuning", CASES)
def test_stored_values_within_one_rounding(kind, cfgname, B, T, tuning):
    """(a) and (d)"""
    run = _run(kind, cfgname, B, T, tuning, "bf16s")
    assert any(r["storage"] == 1 for r in run["rep64"]) and any(s["storage"] == 2 for s in run["sites"])
    _check_values(run)


@pytest.mark.parametrize("kind,cfgname,B,T,tuning", CASES)
def test_stores_round_to_nearest(kind, cfgname, B, T, tuning):
    """(b)"""
    _check_rounding(_run(kind, cfgname, B, T, tuning, "bf16s"))


@pytest.mark.parametrize("kind,cfgname,B,T,tuning", CASES)
def test_statistics_are_those_of_the_stored_tensor(kind, cfgname, B, T, tuning):
    """(c)"""
    _check_stats(_run(kind, cfgname, B, T, tuning, "bf16s"))


@pytest.mark.parametrize("kind,cfgname,B,T,tuning", CASES)
def test_local_weight_gradients_from_surviving_operands(kind, cfgname, B, T, tuning):
    """(f)"""
    _check_wgrads(_run(kind, cfgname, B, T, tuning, "bf16s"))


def _poison(t):
    t[(0,) * t.dim()] = float("nan")


def test_a_nan_fails_every_check():
    """The workspace starts as NaN, so a wrong offset, an unwritten tail or an untouched statistics slot arrives here as a NaN: one NaN
    in anything taken from the engine must fail the run before the replay, and -- should it get past that -- every single check."""
    import copy
    run = _run("emu", *SHAPES[0], "bf16s")
    raw = {k: v for k, v in run.items() if k not in ("rep64", "rep32")}
    kind1 = next(i for i, s in enumerate(run["sites"]) if s["kind"] == 1)

    def poison_site(r):
        r["sites"][kind1]["y"][0, 0, 0] = float("nan")

    def poison_stat(r):
        r["sites"][kind1]["rstd"][0, 0, 0] = float("nan")

    def poison_named(r):
        r["named"]["dec_outN"][-1, -1, -1] = float("nan")

    def poison_res(r):
        r["res"]["muls"][0, 0, 0] = float("nan")

    def poison_grad(r):
        r["grads"]["decoder.out_conv_layer.bias"][0] = float("nan")

    for poison in (poison_site, poison_stat, poison_named, poison_res, poison_grad, lambda r: _poison(r["d_dec"])):
        bad = copy.deepcopy(raw)
        poison(bad)
        with pytest.raises(AssertionError, match="non-finite"):
            _analyse(bad)
    # past the gate: each check on a run whose compared tensors hold one NaN
    bf = next(i for i, r in enumerate(run["rep64"]) if r["storage"] == 1 and r["what"] == "y")
    fp = next(i for i, r in enumerate(run["rep64"]) if r["storage"] == 0)
    for idx in (bf, fp):
        bad = copy.deepcopy(run)
        _poison(bad["rep64"][idx]["engine"])
        with pytest.raises(AssertionError, match="beyond"):
            _check_values(bad)
    for idx in (bf, fp):    # ... and a NaN in the reference value (what a NaN substituted upstream turns every later record into)
        bad = copy.deepcopy(run)
        _poison(bad["rep64"][idx]["value"])
        with pytest.raises(AssertionError, match="bound"):
            _check_values(bad)
    bad = copy.deepcopy(run)
    _poison(bad["rep64"][bf]["engine"])
    with pytest.raises(AssertionError, match="rounding error"):
        _check_rounding(bad)
    for k in ("mean", "rstd"):
        bad = copy.deepcopy(run)
        _poison(bad["sites"][kind1][k])
        with pytest.raises(AssertionError, match=k):
            _check_stats(bad)
    for k in ("decoder.out_conv_layer.weight", "content_encoder.std_layer.bias"):
        bad = copy.deepcopy(run)
        _poison(bad["grads"][k])
        with pytest.raises(AssertionError, match=k.replace(".", r"\.")):
            _check_wgrads(bad)
