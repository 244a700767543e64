"""Parameter gradients of the ragged speaker encoder: a "speaker_pg" RaggedPlan (avc_plan_create_ragged_speaker_grads),
``avc_backward_ragged_params`` and ``AE.speaker_encoder_ragged`` -- d(loss)/d(parameters) over B utterances of different lengths from ONE
ragged launch set, fp32, together with the input gradients.

kind='emu': the CPU lane-level simulation of the same kernels on the tiny config; kind='gpu': the gfx950 library on the stock 80-mel
config.  Length sets: those of tests/test_ragged_enroll.py (17, 64, 65, odd lengths at every level, 600 on the GPU).

Bar (README "Stated tolerances", gradients summed over many frames), per tensor, on the ReLU branch the engine took (read from the saved
activations, ``_relu_masks``):  err(engine, fp64 oracle) <= max(1e-4, 2 x err(fp32 oracle, fp64 oracle)) in rel-L2.  No tensor is filtered
out; a tensor whose reference norm is below 1e-6 of the whole gradient's norm is compared absolutely against that scale, as
``check_param_grads`` does."""
import ctypes

import pytest
import torch

from adaptive_voice_conversion_amd import _lib as L
from adaptive_voice_conversion_amd.engine import Plan, RaggedPlan, cfg_from_dict
from oracle import avc_oracle as O
from tests.emu_util import KINDS, backend
from tests.ragged_oracle import SPK, speaker_masks as _relu_masks, speaker_oracle as _oracle
from tests.redzone import GuardedOutput, guarded_input, guarded_like
from tests.test_engine import flat_params
from tests.test_ragged_enroll import _model, _nan_ws, _setup, _utts
from tests.test_ragged_input_grads import _d_emb, _leaves
from tests.test_submodules import rel

_CACHE = {}


def _pass(kind, seed=9, d_seed=31):
    """forward + backward_params of a speaker_pg plan, NaN-filled workspace and grads -> everything the tests below share (run once per kind
    and left unchanged)"""
    if kind in _CACHE:
        return _CACHE[kind]
    lib, dev, cfg, sd, _, Tc = _setup(kind)
    cs = _utts(Tc, cfg["ContentEncoder"]["c_in"], seed)
    plan = RaggedPlan(cfg, None, Tc, lib=lib, mode="speaker_pg")
    params = flat_params(plan, sd, dev)
    ws = _nan_ws(plan, dev)
    xc = torch.cat(cs).to(dev)
    plan.forward(params, None, xc, ws)
    d = _d_emb(len(Tc), plan.c_emb, d_seed)
    grads = torch.full((plan.param_floats,), float("nan"), device=dev)
    plan.backward_params(params, xc, d.to(dev), grads, ws)
    masks = _relu_masks(plan, ws)
    r64, r32 = _oracle(cfg, sd, cs, masks, d, torch.float64), _oracle(cfg, sd, cs, masks, d, torch.float32)
    out = dict(lib=lib, dev=dev, cfg=cfg, sd=sd, Tc=Tc, cs=cs, plan=plan, params=params, ws=ws, xc=xc, d=d, grads=grads, masks=masks,
               r64=r64, r32=r32, emb=plan.emb(ws).clone(), dxc=plan.d_x_cond(ws).clone())
    _CACHE[kind] = out
    return out


def _tensors(plan, sd, grads):
    """{name: tensor} of the speaker encoder's range of a flat gradient buffer"""
    g = grads.detach().cpu()
    return {k: g[off:off + n].view(shape).double() for (off, n, shape), k in zip(plan.param_info, sd) if k.startswith(SPK)}


def _check(got, r64, r32, tag):
    """the bar of the module docstring on every tensor; returns and prints the worst"""
    scale = sum(float(v.norm()) ** 2 for v in r64.values()) ** 0.5
    worst = (0.0, None, 0.0)
    for k, ref in r64.items():
        g = got[k]
        assert not torch.isnan(g).any(), k
        if float(ref.norm()) < 1e-6 * scale:
            assert float((g - ref).norm()) < 1e-5 * scale, k
            continue
        e, e32 = rel(g, ref), (rel(r32[k], ref) if r32 is not None else 0.0)
        bar = max(1e-4, 2 * e32)
        if e / bar > worst[0]:
            worst = (e / bar, k, e)
        assert e <= bar, (tag, k, e, e32)
    print(f"[{tag}] worst tensor {worst[1]}: rel-L2 {worst[2]:.3e} ({worst[0]:.2f} of its bar)")
    return worst


def _named_grads(model):
    return {k: p.grad.detach().cpu().double() for k, p in model.named_parameters() if k.startswith(SPK) and p.grad is not None}


@pytest.mark.parametrize("kind", KINDS)
def test_parity_with_the_fp64_oracle(kind):
    """1. Every speaker-encoder tensor against the fp64 oracle, through the plan (NaN-filled workspace and grads) and through
    AE.speaker_encoder_ragged."""
    s = _pass(kind)
    _check(_tensors(s["plan"], s["sd"], s["grads"]), s["r64"], s["r32"], f"{kind} plan")
    model = _model(kind, s["lib"], s["dev"], s["cfg"], s["sd"])
    emb = model.speaker_encoder_ragged([c.to(s["dev"]) for c in s["cs"]])
    assert emb.requires_grad and emb.grad_fn is not None
    assert torch.equal(emb.detach(), s["emb"])
    (emb * s["d"].to(s["dev"])).sum().backward()
    _check(_named_grads(model), s["r64"], s["r32"], f"{kind} module")
    for k, p in model.named_parameters():
        assert (p.grad is not None) == k.startswith(SPK), k


@pytest.mark.parametrize("kind", KINDS)
def test_parity_with_the_uniform_path(kind):
    """2. The same tensors against the sum over b of the uniform speaker_encoder(x_b) gradients at B = 1 (torch accumulates them)."""
    s = _pass(kind)
    model = _model(kind, s["lib"], s["dev"], s["cfg"], s["sd"])
    for b, c in enumerate(s["cs"]):
        (model.speaker_encoder(c.t()[None].to(s["dev"])) * s["d"][b].to(s["dev"])).sum().backward()
    uni = _named_grads(model)
    got = _tensors(s["plan"], s["sd"], s["grads"])
    _check(got, uni, None, f"{kind} ragged vs uniform")           # 1e-4 against each other ...
    _check(uni, s["r64"], s["r32"], f"{kind} uniform vs oracle")   # ... and the uniform path under the same bar against the oracle


@pytest.mark.parametrize("kind", KINDS)
def test_only_the_speaker_range_is_written(kind):
    """3. Every speaker tensor is written, every element outside them keeps its NaN; d_x_cond is bit-identical to the existing flagged plan's,
    emb to the unflagged plan's, and avc_backward_ragged on the new plan gives that same d_x_cond."""
    s = _pass(kind)
    plan, lib, dev = s["plan"], s["lib"], s["dev"]
    flags = lib.avc_plan_flags(plan.h)
    assert flags & L.PLAN_PART_GRADS and flags & L.PLAN_INPUT_GRADS and flags & L.PLAN_SPEAKER_ONLY and flags & L.PLAN_RAGGED
    written = torch.zeros(plan.param_floats, dtype=torch.bool)
    for (off, n, _), k in zip(plan.param_info, s["sd"]):
        if k.startswith(SPK):
            written[off:off + n] = True
    nan = torch.isnan(s["grads"].cpu())
    assert not nan[written].any() and nan[~written].all()
    lo, num = ctypes.c_long(), ctypes.c_long()
    assert lib.avc_plan_param_range(plan.h, L.GRADS_SPEAKER, ctypes.byref(lo), ctypes.byref(num)) == 0
    assert not written[:lo.value].any() and not written[lo.value + num.value:].any()
    plain = RaggedPlan(s["cfg"], None, s["Tc"], lib=lib, mode="speaker")
    flagged = RaggedPlan(s["cfg"], None, s["Tc"], lib=lib, mode="speaker", input_grads=True)
    assert plan.workspace_floats > flagged.workspace_floats > plain.workspace_floats
    w0, w1 = _nan_ws(plain, dev), _nan_ws(flagged, dev)
    plain.forward(s["params"], None, s["xc"], w0)
    flagged.forward(s["params"], None, s["xc"], w1)
    flagged.backward(s["params"], s["xc"], s["d"].to(dev), w1)
    assert torch.equal(plain.emb(w0), s["emb"])
    assert torch.equal(flagged.d_x_cond(w1), s["dxc"])
    w2 = _nan_ws(plan, dev)
    plan.forward(s["params"], None, s["xc"], w2)
    plan.backward(s["params"], s["xc"], s["d"].to(dev), w2)   # the frozen pass on the new plan
    assert torch.equal(plan.d_x_cond(w2), s["dxc"])


@pytest.mark.parametrize("kind", KINDS)
def test_reproducible(kind):
    """4. A second pass in the same workspace, and a fresh forward + backward in another NaN-filled workspace, give identical bits."""
    s = _pass(kind)
    plan, dev = s["plan"], s["dev"]
    g1 = torch.full_like(s["grads"], float("nan"))
    plan.backward_params(s["params"], s["xc"], s["d"].to(dev), g1, s["ws"])
    ws = _nan_ws(plan, dev)
    g2 = torch.full_like(s["grads"], float("nan"))
    plan.forward(s["params"], None, s["xc"], ws)
    plan.backward_params(s["params"], s["xc"], s["d"].to(dev), g2, ws)
    for g in (g1, g2):
        assert torch.equal(g.view(torch.int32), s["grads"].view(torch.int32))


@pytest.mark.parametrize("kind", KINDS)
def test_linearity_in_d_emb(kind):
    """5. d_emb zero except in row b: the gradient equals that of a B = 1 plan on utterance b alone (first, middle, last, and the 17- and
    65-frame utterances)."""
    s = _pass(kind)
    plan, dev, Tc = s["plan"], s["dev"], s["Tc"]
    rows = sorted({0, len(Tc) // 2, len(Tc) - 1, Tc.index(17), Tc.index(65)})
    for b in rows:
        d = torch.zeros_like(s["d"])
        d[b] = s["d"][b]
        g = torch.full_like(s["grads"], float("nan"))
        plan.backward_params(s["params"], s["xc"], d.to(dev), g, s["ws"])
        one = RaggedPlan(s["cfg"], None, [Tc[b]], lib=s["lib"], mode="speaker_pg")
        ws1, g1 = _nan_ws(one, dev), torch.full_like(s["grads"], float("nan"))
        x1 = s["cs"][b].to(dev).contiguous()
        one.forward(s["params"], None, x1, ws1)
        one.backward_params(s["params"], x1, s["d"][b][None].to(dev), g1, ws1)
        assert torch.equal(one.emb(ws1)[0], s["emb"][b])
        r64 = _oracle(s["cfg"], s["sd"], [s["cs"][b]], [s["masks"][b]], s["d"][b][None], torch.float64)
        _check(_tensors(plan, s["sd"], g), _tensors(one, s["sd"], g1), None, f"{kind} row {b} (T={Tc[b]}) vs its B=1 plan")
        _check(_tensors(plan, s["sd"], g), r64, None, f"{kind} row {b} (T={Tc[b]}) vs oracle")   # (no fp32 oracle run: the plain 1e-4)


@pytest.mark.parametrize("kind", KINDS)
def test_module_seams(kind):
    """6. Accumulation, frozen parameters, utterances as leaves, a stride-0 d_emb, no_grad, interleaved calls, a second backward, bf16, and
    an SGD step."""
    s = _pass(kind)
    lib, dev, cfg, sd, cs = s["lib"], s["dev"], s["cfg"], s["sd"], s["cs"]
    dd = s["d"].to(dev)
    model = _model(kind, lib, dev, cfg, sd)
    xs = [c.to(dev) for c in cs]
    # accumulation over two backward calls
    (model.speaker_encoder_ragged(xs) * dd).sum().backward()
    once = _named_grads(model)
    (model.speaker_encoder_ragged(xs) * dd).sum().backward()
    for k, g in _named_grads(model).items():
        assert torch.equal(g, once[k] + once[k]), k
    model.zero_grad(set_to_none=True)
    # a frozen parameter gets none; a subset of utterances as leaves gets get_speaker_embeddings_ragged's bits
    names = [k for k, _ in model.named_parameters() if k.startswith(SPK)]
    frozen = names[3]
    dict(model.named_parameters())[frozen].requires_grad_(False)
    leaves = _leaves(cs, dev)
    mixed = [leaves[b] if b % 2 == 0 else xs[b] for b in range(len(cs))]
    (model.speaker_encoder_ragged(mixed) * dd).sum().backward()
    ref_leaves = _leaves(cs, dev)
    ref_mixed = [ref_leaves[b] if b % 2 == 0 else xs[b] for b in range(len(cs))]
    (model.get_speaker_embeddings_ragged(ref_mixed) * dd).sum().backward()
    for b in range(len(cs)):
        if b % 2 == 0:
            assert torch.equal(leaves[b].grad, ref_leaves[b].grad), b
        else:
            assert xs[b].grad is None
    for k, p in model.named_parameters():
        assert (p.grad is not None) == (k.startswith(SPK) and k != frozen), k
    for k, g in _named_grads(model).items():
        assert torch.equal(g, once[k]), k
    dict(model.named_parameters())[frozen].requires_grad_(True)
    model.zero_grad(set_to_none=True)
    # every parameter frozen, utterances live: the frozen pass, same bits
    for p in model.parameters():
        p.requires_grad_(False)
    fl = _leaves(cs, dev)
    e = model.speaker_encoder_ragged(fl)
    assert e.grad_fn is not None
    (e * dd).sum().backward()
    for b in range(0, len(cs), 2):
        assert torch.equal(fl[b].grad, ref_leaves[b].grad)
    assert not model.speaker_encoder_ragged(xs).requires_grad
    for p in model.parameters():
        p.requires_grad_(True)
    # d_emb with batch stride 0
    model.speaker_encoder_ragged(xs).mean(0).sum().backward()
    mean_g = _named_grads(model)
    model.zero_grad(set_to_none=True)
    (model.speaker_encoder_ragged(xs) * torch.full_like(dd, 1.0 / len(cs))).sum().backward()
    for k, g in _named_grads(model).items():
        assert torch.equal(g, mean_g[k]), k
    model.zero_grad(set_to_none=True)
    # no_grad: the forward-only call, no grad plan
    model._ragged.clear()
    with torch.no_grad():
        e0 = model.speaker_encoder_ragged(xs)
    assert not e0.requires_grad and torch.equal(e0, s["emb"])
    assert all(key[0] == "speaker" for key in model._ragged)
    # a forward-only call and a second grad forward between a forward and its backward do not disturb it
    first = model.speaker_encoder_ragged(xs)
    with torch.no_grad():
        model.get_speaker_embeddings_ragged([x * 2 for x in xs])
    second = model.speaker_encoder_ragged([x * 3 for x in xs])
    (first * dd).sum().backward()
    for k, g in _named_grads(model).items():
        assert torch.equal(g, once[k]), k
    with pytest.raises(RuntimeError, match="twice"):
        (first * dd).sum().backward()
    (second * dd).sum().backward()
    model.zero_grad(set_to_none=True)
    # bf16 raises on the grad path
    bf = _model(kind, lib, dev, cfg, sd, compute_dtype="bf16")
    with pytest.raises(RuntimeError, match="fp32 only"):
        bf.speaker_encoder_ragged(xs)
    with torch.no_grad():
        bf.speaker_encoder_ragged(xs)
    # one SGD step on the speaker encoder's parameters
    v0 = model.weights_version()
    (model.speaker_encoder_ragged(xs) * dd).sum().backward()
    torch.optim.SGD(model.speaker_encoder.parameters(), lr=1e-2).step()
    assert model.weights_version() != v0
    with torch.no_grad():
        assert not torch.equal(model.speaker_encoder_ragged(xs), s["emb"])


@pytest.mark.parametrize("kind", KINDS)
def test_refusals(kind):
    """7. avc_backward_ragged_params: -8 on every other kind of plan and under bf16, -1 on a null argument; the existing creators still
    refuse what they refused."""
    s = _pass(kind)
    lib, dev, cfg, Tc = s["lib"], s["dev"], s["cfg"], s["Tc"]
    buf = torch.zeros(64, device=dev)
    p = ctypes.c_void_p(buf.data_ptr())

    def call(plan, **kw):
        a = dict(params=p, x=p, d=p, grads=p, ws=p)
        a.update(kw)
        return lib.avc_backward_ragged_params(plan.h, a["params"], a["x"], a["d"], 4, 1, a["grads"], a["ws"], None)
    T3 = Tc[:3]
    others = [RaggedPlan(cfg, None, T3, lib=lib, mode="speaker"), RaggedPlan(cfg, None, T3, lib=lib, mode="speaker", input_grads=True),
              RaggedPlan(cfg, T3, None, lib=lib, mode="encode", input_grads=True), RaggedPlan(cfg, [3, 5], None, lib=lib, mode="decode_ig"),
              RaggedPlan(cfg, T3, None, lib=lib, mode="fanout", src_of=[0, 2, 2]), RaggedPlan(cfg, T3, T3, lib=lib, mode="pairs"),
              Plan(cfg, 2, 32, 32, lib=lib, mode="speaker_train")]
    for o in others:
        assert call(o) == -8, o.mode
        assert b"avc_plan_create_ragged_speaker_grads" in lib.avc_last_error()
    bf = RaggedPlan(cfg, None, T3, lib=lib, mode="speaker_pg", compute_dtype="bf16")
    assert call(bf) == -8 and b"bf16" in lib.avc_last_error()
    for k in ("params", "x", "d", "grads", "ws"):
        assert call(s["plan"], **{k: None}) == -1, k
    assert lib.avc_backward_ragged_params(None, p, p, p, 4, 1, p, p, None) == -1
    h = ctypes.c_void_p()
    ccfg = cfg_from_dict(cfg)
    lens = (ctypes.c_int * 3)(*T3)
    for flags in (L.PLAN_SPEAKER_ONLY | L.PLAN_PART_GRADS, L.PLAN_SPEAKER_ONLY | L.PLAN_INPUT_GRADS | L.PLAN_PART_GRADS, L.PLAN_INPUT_GRADS,
                  L.PLAN_EMB_INPUT | L.PLAN_INPUT_GRADS):
        assert lib.avc_plan_create_ragged_ex(ctypes.byref(ccfg), 3, lens, lens, flags, None, ctypes.byref(h)) == -1, flags
    assert lib.avc_plan_create_ragged_speaker_grads(ctypes.byref(ccfg), 0, lens, None, ctypes.byref(h)) == -1
    assert lib.avc_plan_create_ragged_speaker_grads(ctypes.byref(ccfg), 3, None, None, ctypes.byref(h)) == -1
    short = (ctypes.c_int * 3)(40, 2, 40)
    assert lib.avc_plan_create_ragged_speaker_grads(ctypes.byref(ccfg), 3, short, None, ctypes.byref(h)) == -6
    with pytest.raises(RuntimeError, match="speaker_pg"):
        others[1].backward_params(s["params"], s["xc"], s["d"].to(dev), s["grads"], s["ws"])


@pytest.mark.parametrize("kind", KINDS)
def test_red_zones(kind):
    """8. Guard bands around params, x_cond, d_emb, grads and the workspace hold for forward + backward of the new plan."""
    s = _pass(kind)
    plan, dev = s["plan"], s["dev"]
    gp, gg, gw = guarded_like(s["params"]), GuardedOutput(plan.param_floats, device=dev), GuardedOutput(plan.workspace_floats, device=dev)
    xc = guarded_input(s["xc"].reshape(-1), device=dev).view(s["xc"].shape)
    d = guarded_input(s["d"].reshape(-1), device=dev).view(s["d"].shape)
    plan.forward(gp.view, None, xc, gw.view)
    plan.backward_params(gp.view, xc, d, gg.view, gw.view)
    for g, name in ((gp, "params"), (gg, "grads"), (gw, "workspace")):
        g.assert_intact(name)
    assert torch.equal(gg.view.view(torch.int32), s["grads"].view(torch.int32))
    assert torch.equal(plan.emb(gw.view), s["emb"]) and torch.equal(plan.d_x_cond(gw.view), s["dxc"])
