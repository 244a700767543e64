"""Parameter gradients of the ragged content encoder: an "encode_pg" RaggedPlan (avc_plan_create_ragged_content_param_grads),
``avc_content_backward_ragged_params`` and ``AE.content_encoder_ragged(xs, param_grads=True)`` -- d(loss)/d(parameters) over S utterances
of different lengths from ONE ragged launch set, fp32, together with the input gradients.

kind='emu': the CPU lane-level simulation of the same kernels on the tiny config; kind='gpu': the gfx950 library on the stock 80-mel
config.  Lengths: 17 (the shortest the reflect-pad rule allows at the last level), 64 / 65 / 66 / 130 (32- and 33-frame chunk edges and odd
rows at several levels), 600 on the GPU only; one utterance alone (S = 1).

Bar (README "Stated tolerances"), per tensor, on the branch the engine took (``content_masks``):  err(engine, fp64 oracle) <= max(1e-4,
2 x err(fp32 oracle, fp64 oracle)) in rel-L2; a tensor whose reference norm is below 1e-6 of the whole gradient's norm -- here the bias
of every conv but the two heads: it feeds an InstanceNorm, its gradient is mathematically zero -- is compared absolutely against that
scale (``tests.ragged_param_oracle.check``).  No tensor is filtered out."""
import ctypes

import pytest
import torch

from adaptive_voice_conversion_amd import _lib as L
from adaptive_voice_conversion_amd.engine import Plan, RaggedPlan, cfg_from_dict
from oracle import avc_oracle as O
from tests.emu_util import KINDS, backend
from tests.ragged_oracle import content_masks
from tests.ragged_param_oracle import ENC, check, content_oracle, flipped, named_grads, tensors, uniform_masks, written_mask
from tests.test_engine import flat_params
from tests.test_ragged_content_grads import _blocks, _d_muls
from tests.test_ragged_enroll import _model, _nan_ws, _utts

LENGTHS = {"emu": [17, 64, 65, 66, 130], "gpu": [17, 64, 65, 66, 130, 600]}
# avc_plan_workspace_floats of the plain "encode" plan and of the flagged one (input_grads=True) over LENGTHS, as they were before the
# parameter-gradient plan existed: the frozen plans' workspaces do not grow
FLOATS = {"emu": (292096, 531520), "gpu": (4331968, 7702720)}
_CACHE = {}


def _cfg(kind):
    lib, dev = backend(kind)
    cfg = O.tiny_config() if kind == "emu" else O.stock_config(80)
    return lib, dev, cfg, O.make_state_dict(cfg, 21)


def _run(kind, T, seed=9, d_seed=31):
    """forward + backward_content_params of an "encode_pg" plan over lengths T, NaN-filled workspace and grads, and both oracles"""
    lib, dev, cfg, sd = _cfg(kind)
    xs = _utts(T, cfg["ContentEncoder"]["c_in"], seed)
    plan = RaggedPlan(cfg, T, None, lib=lib, mode="encode_pg")
    params = flat_params(plan, sd, dev)
    ws = _nan_ws(plan, dev)
    x = torch.cat(xs).to(dev)
    plan.forward(params, x, None, ws)
    d = _d_muls(plan, d_seed)
    grads = torch.full((plan.param_floats,), float("nan"), device=dev)
    plan.backward_content_params(params, x, d.to(dev), grads, ws)
    masks = content_masks(plan, ws, cfg)
    blocks = _blocks(d, plan)
    r64, r32 = content_oracle(cfg, sd, xs, masks, blocks, torch.float64), content_oracle(cfg, sd, xs, masks, blocks, torch.float32)
    return dict(lib=lib, dev=dev, cfg=cfg, sd=sd, T=list(T), xs=xs, plan=plan, params=params, ws=ws, x=x, d=d, grads=grads, masks=masks,
                blocks=blocks, r64=r64, r32=r32, muls=[t.clone() for t in plan.latents(ws)[0] + plan.latents(ws)[1]], dx=plan.d_x(ws).clone())


def _pass(kind):
    """the pass over LENGTHS: run once per kind, shared by the tests and left unchanged"""
    if kind not in _CACHE:
        _CACHE[kind] = _run(kind, LENGTHS[kind])
    return _CACHE[kind]


def _loss(mu, ls, blocks, dev):
    return sum((m * wm[0].to(dev)).sum() + (s * wl[0].to(dev)).sum() for m, s, (wm, wl) in zip(mu, ls, blocks))


@pytest.mark.parametrize("kind", KINDS)
def test_parity_with_the_fp64_oracle(kind):
    """1. Every content-encoder tensor against the fp64 oracle, through the plan (NaN-filled workspace and grads) and through
    AE.content_encoder_ragged(param_grads=True); the other two networks' parameters get nothing."""
    s = _pass(kind)
    check(tensors(s["plan"], s["sd"], s["grads"], ENC), s["r64"], s["r32"], f"{kind} plan")
    model = _model(kind, s["lib"], s["dev"], s["cfg"], s["sd"])
    mu, ls = model.content_encoder_ragged([x.to(s["dev"]) for x in s["xs"]], param_grads=True)
    assert all(t.requires_grad and t.grad_fn is not None for t in mu + ls)
    assert all(torch.equal(a.detach(), b) for a, b in zip(mu + ls, s["muls"]))
    _loss(mu, ls, s["blocks"], s["dev"]).backward()
    check(named_grads(model, ENC), s["r64"], s["r32"], f"{kind} module")
    for k, p in model.named_parameters():
        assert (p.grad is not None) == k.startswith(ENC), k


@pytest.mark.parametrize("kind", KINDS)
def test_one_utterance_alone(kind):
    """1b. S = 1 (65 frames): the same bar."""
    s = _run(kind, [65], seed=5, d_seed=6)
    check(tensors(s["plan"], s["sd"], s["grads"], ENC), s["r64"], s["r32"], f"{kind} S=1")


@pytest.mark.parametrize("kind", KINDS)
def test_parity_with_the_uniform_path(kind):
    """2. The same tensors against the sum over s of the uniform content_encoder(x_s) gradients at B = 1 (torch accumulates them).  Each
    engine is held to the oracle ON ITS OWN BRANCH (the ragged one in test 1, the uniform one here, its branch read from the uniform plans'
    saved rows), so a branch flip can neither hide an error nor fake one; where both took the same branch on every utterance they are
    also within 1e-4 of each other."""
    s = _pass(kind)
    dev = s["dev"]
    model = _model(kind, s["lib"], dev, s["cfg"], s["sd"])
    um = []
    for x, (wm, wl) in zip(s["xs"], s["blocks"]):
        mu, ls = model.content_encoder(x.t()[None].to(dev))
        ((mu * wm.to(dev)).sum() + (ls * wl.to(dev)).sum()).backward()
        um.append(uniform_masks(model, "content_train", x.shape[0], dev))
    uni = named_grads(model, ENC)
    flips = [flipped(a, b) for a, b in zip(s["masks"], um)]
    print(f"[{kind}] activation decisions that differ between the ragged and the uniform engine, per utterance {s['T']}: {flips}")
    if not any(flips):
        check(tensors(s["plan"], s["sd"], s["grads"], ENC), uni, None, f"{kind} ragged vs uniform")
        check(uni, s["r64"], s["r32"], f"{kind} uniform vs oracle")
    else:
        u64, u32 = (content_oracle(s["cfg"], s["sd"], s["xs"], um, s["blocks"], t) for t in (torch.float64, torch.float32))
        check(uni, u64, u32, f"{kind} uniform vs oracle on the uniform engine's branch")


@pytest.mark.parametrize("kind", KINDS)
def test_only_the_content_range_is_written(kind):
    """3. Every content tensor is written, every element outside keeps its NaN; avc_plan_param_range agrees; the flags; the workspaces: new
    plan > flagged plan > plain plan, the latter two what they were."""
    s = _pass(kind)
    plan, lib = s["plan"], s["lib"]
    flags = lib.avc_plan_flags(plan.h)
    assert flags & L.PLAN_PART_GRADS and flags & L.PLAN_INPUT_GRADS and flags & L.PLAN_CONTENT_ONLY and flags & L.PLAN_RAGGED
    written = written_mask(plan, s["sd"], ENC)
    nan = torch.isnan(s["grads"].cpu())
    assert not nan[written].any() and nan[~written].all()
    lo, num = ctypes.c_long(), ctypes.c_long()
    assert lib.avc_plan_param_range(plan.h, L.GRADS_CONTENT, ctypes.byref(lo), ctypes.byref(num)) == 0
    assert written[lo.value:lo.value + num.value].any() and not written[:lo.value].any() and not written[lo.value + num.value:].any()
    plain = RaggedPlan(s["cfg"], s["T"], None, lib=lib, mode="encode")
    flagged = RaggedPlan(s["cfg"], s["T"], None, lib=lib, mode="encode", input_grads=True)
    assert plan.workspace_floats > flagged.workspace_floats > plain.workspace_floats
    assert (plain.workspace_floats, flagged.workspace_floats) == FLOATS[kind]
    assert lib.avc_plan_flags(flagged.h) | L.PLAN_PART_GRADS == flags


@pytest.mark.parametrize("kind", KINDS)
def test_bit_identities(kind):
    """4. The forward equals the flagged plan's; the frozen pass on the new plan equals the frozen pass on the flagged plan; d_x of the params
    pass equals the frozen pass's; two params passes (same workspace, and a fresh NaN-filled one) give equal grads bits."""
    s = _pass(kind)
    plan, dev, params, x, d = s["plan"], s["dev"], s["params"], s["x"], s["d"].to(s["dev"])
    flagged = RaggedPlan(s["cfg"], s["T"], None, lib=s["lib"], mode="encode", input_grads=True)
    w1 = _nan_ws(flagged, dev)
    flagged.forward(params, x, None, w1)
    flagged.backward_content(params, x, d, w1)
    assert all(torch.equal(a, b) for a, b in zip(flagged.latents(w1)[0] + flagged.latents(w1)[1], s["muls"]))
    assert torch.equal(flagged.d_x(w1), s["dx"])
    w2 = _nan_ws(plan, dev)
    plan.forward(params, x, None, w2)
    plan.backward_content(params, x, d, w2)   # the frozen pass on the new plan
    assert torch.equal(plan.d_x(w2), s["dx"])
    g1 = torch.full_like(s["grads"], float("nan"))
    plan.backward_content_params(params, x, d, g1, s["ws"])
    g2 = torch.full_like(s["grads"], float("nan"))
    plan.backward_content_params(params, x, d, g2, w2)
    for g in (g1, g2):
        assert torch.equal(g.view(torch.int32), s["grads"].view(torch.int32))
    assert torch.equal(plan.d_x(w2), s["dx"])


@pytest.mark.parametrize("kind", KINDS)
def test_refusals(kind):
    """5. avc_content_backward_ragged_params: -8 with the creator's name on every other kind of plan, -8 under bf16, -1 on a null argument;
    the old creators and RaggedPlan(mode="decode", input_grads=True) refuse what they refused; the module raises under bf16."""
    s = _pass(kind)
    lib, dev, cfg = s["lib"], s["dev"], s["cfg"]
    buf = torch.zeros(64, device=dev)
    p = ctypes.c_void_p(buf.data_ptr())

    def call(plan, **kw):
        a = dict(params=p, x=p, d=p, grads=p, ws=p)
        a.update(kw)
        return lib.avc_content_backward_ragged_params(plan.h, a["params"], a["x"], a["d"], a["grads"], a["ws"], None)
    T3 = s["T"][:3]
    others = [RaggedPlan(cfg, T3, None, lib=lib, mode="encode"), RaggedPlan(cfg, T3, None, lib=lib, mode="encode", input_grads=True),
              RaggedPlan(cfg, None, T3, lib=lib, mode="speaker_pg"), RaggedPlan(cfg, [3, 5], None, lib=lib, mode="decode_ig"),
              RaggedPlan(cfg, [3, 5], None, lib=lib, mode="decode_pg"), RaggedPlan(cfg, T3, None, lib=lib, mode="fanout", src_of=[0, 2, 2]),
              RaggedPlan(cfg, T3, T3, lib=lib, mode="pairs"), Plan(cfg, 2, 32, 32, lib=lib, mode="content_train")]
    for o in others:
        assert call(o) == -8, o.mode
        assert b"avc_plan_create_ragged_content_param_grads" in lib.avc_last_error()
    bf = RaggedPlan(cfg, T3, None, lib=lib, mode="encode_pg", compute_dtype="bf16")
    assert call(bf) == -8 and b"bf16" in lib.avc_last_error()
    for k in ("params", "x", "d", "grads", "ws"):
        assert call(s["plan"], **{k: None}) == -1, k
    assert lib.avc_content_backward_ragged_params(None, p, p, p, p, p, None) == -1
    h = ctypes.c_void_p()
    ccfg = cfg_from_dict(cfg)
    lens = (ctypes.c_int * 3)(*T3)
    for flags in (L.PLAN_INPUT_GRADS, L.PLAN_EMB_INPUT | L.PLAN_INPUT_GRADS, L.PLAN_SPEAKER_ONLY | L.PLAN_PART_GRADS):
        assert lib.avc_plan_create_ragged_ex(ctypes.byref(ccfg), 3, lens, lens, flags, None, ctypes.byref(h)) == -1, flags
    assert lib.avc_plan_create_ragged_fanout(ctypes.byref(ccfg), 3, lens, 0, None, L.PLAN_CONTENT_ONLY | L.PLAN_PART_GRADS, None, ctypes.byref(h)) == -1
    assert lib.avc_plan_create_ragged_content_param_grads(ctypes.byref(ccfg), 0, lens, None, ctypes.byref(h)) == -1
    assert lib.avc_plan_create_ragged_content_param_grads(ctypes.byref(ccfg), 3, None, None, ctypes.byref(h)) == -1
    short = (ctypes.c_int * 3)(40, 2, 40)
    assert lib.avc_plan_create_ragged_content_param_grads(ctypes.byref(ccfg), 3, short, None, ctypes.byref(h)) == -6
    with pytest.raises(ValueError, match="forward only"):
        RaggedPlan(cfg, [3, 5], None, lib=lib, mode="decode", input_grads=True)
    with pytest.raises(RuntimeError, match="encode_pg"):
        others[1].backward_content_params(s["params"], s["x"], s["d"].to(dev), s["grads"], s["ws"])
    model = _model(kind, lib, dev, cfg, s["sd"], compute_dtype="bf16")
    with pytest.raises(RuntimeError, match="fp32 only"):
        model.content_encoder_ragged([x.to(dev) for x in s["xs"][:2]], param_grads=True)


@pytest.mark.parametrize("kind", KINDS)
def test_default_keeps_the_module_path(kind):
    """6. param_grads=False (the default): with only parameters requiring grad the outputs carry no grad_fn, and the forward bits are those
    of the param_grads=True call; with every content parameter frozen, param_grads=True is the default call."""
    s = _pass(kind)
    model = _model(kind, s["lib"], s["dev"], s["cfg"], s["sd"])
    xs = [x.to(s["dev"]) for x in s["xs"]]
    mu, ls = model.content_encoder_ragged(xs)
    assert not any(t.requires_grad or t.grad_fn is not None for t in mu + ls)
    assert all(torch.equal(a, b) for a, b in zip(mu + ls, s["muls"]))
    assert not any(key[0] == "encode_pg" for key in model._ragged)
    for p in model.content_encoder.parameters():
        p.requires_grad_(False)
    mu, ls = model.content_encoder_ragged(xs, param_grads=True)
    assert not any(t.requires_grad for t in mu + ls)
    with torch.no_grad():
        for p in model.content_encoder.parameters():
            p.requires_grad_(True)
        mu, ls = model.content_encoder_ragged(xs, param_grads=True)
    assert not any(t.requires_grad for t in mu + ls) and all(torch.equal(a, b) for a, b in zip(mu + ls, s["muls"]))
