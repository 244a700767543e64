"""Parameter gradients of the ragged decoder: a "decode_pg" RaggedPlan (avc_plan_create_ragged_decoder_param_grads),
``avc_decoder_backward_ragged_params`` and ``AE.decoder_ragged(zs, emb, param_grads=True)`` -- d(loss)/d(parameters) over N latents of
different lengths from ONE ragged launch set, fp32, together with d(z) and d(emb).  The 2n AdaIN affine Linears run as STRIDED jobs of the
ragged weight-gradient kernel: dy = their slice of frame-major d(cond), x = the caller's emb in place (an expanded single voice included).

kind='emu': the CPU lane-level simulation of the same kernels on the tiny config; kind='gpu': the gfx950 library on the stock 80-mel
config.  Latent lengths: 3 (the minimum for k = 5), 4, 8, 9, 33, 75; one latent alone (N = 1).

Bar (README "Stated tolerances"), per tensor, on the branch the engine took (``decoder_masks``):  err(engine, fp64 oracle) <= max(1e-4,
2 x err(fp32 oracle, fp64 oracle)) in rel-L2; a tensor whose reference norm is below 1e-6 of the whole gradient's norm -- the bias of
every conv but out_conv: it feeds an InstanceNorm / AdaIN, its gradient is mathematically zero -- is compared absolutely against that scale
(``tests.ragged_param_oracle.check``).  No tensor is filtered out."""
import ctypes

import pytest
import torch

from adaptive_voice_conversion_amd import _lib as L
from adaptive_voice_conversion_amd.engine import Plan, RaggedPlan, cfg_from_dict
from oracle import avc_oracle as O
from tests.emu_util import KINDS, backend
from tests.ragged_oracle import decoder_masks
from tests.ragged_param_oracle import DEC, check, decoder_oracle, flipped, named_grads, tensors, uniform_masks, written_mask
from tests.test_engine import flat_params
from tests.test_ragged_decoder_grads import _d_dec, _inputs, _out_blocks
from tests.test_ragged_enroll import _model, _nan_ws

TZ = [3, 4, 8, 9, 33, 75]
# avc_plan_workspace_floats of the plain "decode" plan and of the "decode_ig" plan over TZ, as they were before the parameter-gradient
# plan existed: the frozen plans' workspaces do not grow
FLOATS = {"emu": (180032, 364992), "gpu": (3545984, 5793344)}
_CACHE = {}


def _cfg(kind):
    lib, dev = backend(kind)
    cfg = O.tiny_config() if kind == "emu" else O.stock_config(80)
    return lib, dev, cfg, O.make_state_dict(cfg, 3)


def _run(kind, Tz, one_voice=False, seed=9, d_seed=31):
    """forward + backward_decoder_params of a "decode_pg" plan over latent lengths Tz, NaN-filled workspace and grads, and both oracles;
    one_voice: emb is ONE row read with row stride 0"""
    lib, dev, cfg, sd = _cfg(kind)
    zs, emb = _inputs(cfg, Tz, seed)
    if one_voice:
        emb = emb[:1].expand(len(Tz), -1)
    plan = RaggedPlan(cfg, Tz, None, lib=lib, mode="decode_pg")
    params = flat_params(plan, sd, dev)
    ws = _nan_ws(plan, dev)
    z = torch.cat([t.reshape(-1) for t in zs]).to(dev)
    e = emb[:1].to(dev).expand(len(Tz), -1) if one_voice else emb.to(dev)
    assert e.stride(0) == (0 if one_voice else e.shape[1])
    plan.forward_latents(params, z, plan.c_lat, e, ws)
    d = _d_dec(plan, d_seed)
    grads = torch.full((plan.param_floats,), float("nan"), device=dev)
    plan.backward_decoder_params(params, z, plan.c_lat, e, d.to(dev), grads, ws)
    masks = decoder_masks(plan, ws, cfg)
    blocks = _out_blocks(d, plan)
    r64, r32 = decoder_oracle(cfg, sd, zs, emb, masks, blocks, torch.float64), decoder_oracle(cfg, sd, zs, emb, masks, blocks, torch.float32)
    return dict(lib=lib, dev=dev, cfg=cfg, sd=sd, Tz=list(Tz), zs=zs, emb=emb, plan=plan, params=params, ws=ws, z=z, e=e, d=d, grads=grads,
                masks=masks, blocks=blocks, r64=r64, r32=r32, outs=[t.clone() for t in plan.outputs(ws)], dz=[t.clone() for t in plan.d_z(ws)],
                de=plan.d_emb(ws).clone())


def _pass(kind, one_voice=False):
    """the pass over TZ: run once per kind and voice layout, shared by the tests and left unchanged"""
    if (kind, one_voice) not in _CACHE:
        _CACHE[kind, one_voice] = _run(kind, TZ, one_voice)
    return _CACHE[kind, one_voice]


def _loss(outs, blocks, dev):
    return sum((o * w[0].to(dev)).sum() for o, w in zip(outs, blocks))


@pytest.mark.parametrize("one_voice", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_parity_with_the_fp64_oracle(kind, one_voice):
    """1. Every decoder tensor against the fp64 oracle, through the plan (NaN-filled workspace and grads) and through
    AE.decoder_ragged(param_grads=True), with emb [N, c_emb] and with one voice (row stride 0); the other networks' parameters get nothing."""
    s = _pass(kind, one_voice)
    check(tensors(s["plan"], s["sd"], s["grads"], DEC), s["r64"], s["r32"], f"{kind} plan one_voice={one_voice}")
    model = _model(kind, s["lib"], s["dev"], s["cfg"], s["sd"])
    emb = s["emb"][0] if one_voice else s["emb"]
    outs = model.decoder_ragged([z.to(s["dev"]) for z in s["zs"]], emb.to(s["dev"]), param_grads=True)
    assert all(t.requires_grad and t.grad_fn is not None for t in outs)
    assert all(torch.equal(a.detach(), b) for a, b in zip(outs, s["outs"]))
    _loss(outs, s["blocks"], s["dev"]).backward()
    check(named_grads(model, DEC), s["r64"], s["r32"], f"{kind} module one_voice={one_voice}")
    for k, p in model.named_parameters():
        assert (p.grad is not None) == k.startswith(DEC), k


@pytest.mark.parametrize("kind", KINDS)
def test_one_latent_alone(kind):
    """1b. N = 1 (Tz = 9): the same bar."""
    s = _run(kind, [9], seed=5, d_seed=6)
    check(tensors(s["plan"], s["sd"], s["grads"], DEC), s["r64"], s["r32"], f"{kind} N=1")


@pytest.mark.parametrize("kind", KINDS)
def test_inputs_and_parameters_together(kind):
    """1c. Latents and emb as leaves beside live parameters: their gradients are the frozen pass's bits, the parameters' the plan's."""
    s = _pass(kind)
    dev = s["dev"]
    model = _model(kind, s["lib"], dev, s["cfg"], s["sd"])
    zs = [z.to(dev, copy=True).requires_grad_(True) for z in s["zs"]]   # (copies: the shared inputs stay what they are)
    emb = s["emb"].to(dev, copy=True).requires_grad_(True)
    _loss(model.decoder_ragged(zs, emb, param_grads=True), s["blocks"], dev).backward()
    assert all(torch.equal(z.grad, g) for z, g in zip(zs, s["dz"])) and torch.equal(emb.grad, s["de"])
    got, ref = named_grads(model, DEC), tensors(s["plan"], s["sd"], s["grads"], DEC)
    assert all(torch.equal(got[k], ref[k]) for k in ref)


@pytest.mark.parametrize("kind", KINDS)
def test_parity_with_the_uniform_path(kind):
    """2. The same tensors against the sum over j of the uniform decoder(z_j, emb_j) gradients at B = 1 (torch accumulates them).  Each
    engine is held to the oracle ON ITS OWN BRANCH (the ragged one in test 1, the uniform one here, its branch read from the uniform plans'
    saved rows), so a branch flip can neither hide an error nor fake one; where both took the same branch on every latent they are also
    within 1e-4 of each other.  (They compute the InstanceNorm statistics in different kernels: a pre-activation next to zero can
    fall on either side.  Measured on the MI355X, stock config: the engines differ in ONE activation decision, in the 33-frame latent,
    and in_conv_layer.weight then differs by 2.1e-3 between them while the ragged engine is within 5.8e-6 and the uniform one within
    1.8e-6 of the oracle on its own branch.  On the simulator, tiny config, no decision differs and the two agree to 6.3e-7.)"""
    s = _pass(kind)
    dev = s["dev"]
    model = _model(kind, s["lib"], dev, s["cfg"], s["sd"])
    um = []
    for j, (z, w) in enumerate(zip(s["zs"], s["blocks"])):
        (model.decoder(z[None].to(dev), s["emb"][j][None].to(dev)) * w.to(dev)).sum().backward()
        um.append(uniform_masks(model, "decoder_train", z.shape[1], dev))
    uni = named_grads(model, DEC)
    flips = [flipped(a, b) for a, b in zip(s["masks"], um)]
    print(f"[{kind}] activation decisions that differ between the ragged and the uniform engine, per latent {s['Tz']}: {flips}")
    if not any(flips):
        check(tensors(s["plan"], s["sd"], s["grads"], DEC), uni, None, f"{kind} ragged vs uniform")
        check(uni, s["r64"], s["r32"], f"{kind} uniform vs oracle")
    else:
        u64, u32 = (decoder_oracle(s["cfg"], s["sd"], s["zs"], s["emb"], um, s["blocks"], t) for t in (torch.float64, torch.float32))
        check(uni, u64, u32, f"{kind} uniform vs oracle on the uniform engine's branch")


@pytest.mark.parametrize("kind", KINDS)
def test_only_the_decoder_range_is_written(kind):
    """3. Every decoder tensor is written, every element outside keeps its NaN; avc_plan_param_range agrees; the flags; the workspaces: new
    plan > "decode_ig" plan > plain plan, the latter two what they were."""
    s = _pass(kind)
    plan, lib = s["plan"], s["lib"]
    flags = lib.avc_plan_flags(plan.h)
    assert flags & L.PLAN_PART_GRADS and flags & L.PLAN_INPUT_GRADS and flags & L.PLAN_DECODER_ONLY and flags & L.PLAN_RAGGED
    assert not flags & L.PLAN_FANOUT
    written = written_mask(plan, s["sd"], DEC)
    nan = torch.isnan(s["grads"].cpu())
    assert not nan[written].any() and nan[~written].all()
    lo, num = ctypes.c_long(), ctypes.c_long()
    assert lib.avc_plan_param_range(plan.h, L.GRADS_DECODER, ctypes.byref(lo), ctypes.byref(num)) == 0
    assert written[lo.value:lo.value + num.value].any() and not written[:lo.value].any() and not written[lo.value + num.value:].any()
    plain = RaggedPlan(s["cfg"], TZ, None, lib=lib, mode="decode")
    flagged = RaggedPlan(s["cfg"], TZ, None, lib=lib, mode="decode_ig")
    assert plan.workspace_floats > flagged.workspace_floats > plain.workspace_floats
    assert (plain.workspace_floats, flagged.workspace_floats) == FLOATS[kind]
    assert lib.avc_plan_flags(flagged.h) | L.PLAN_PART_GRADS == flags


@pytest.mark.parametrize("kind", KINDS)
def test_bit_identities(kind):
    """4. The forward equals the "decode_ig" plan's; the frozen pass on the new plan equals the frozen pass on that plan; d_z / d_emb of the
    params pass equal the frozen pass's; two params passes (same workspace, and a fresh NaN-filled one) give equal grads bits."""
    s = _pass(kind)
    plan, dev, params, z, e, d = s["plan"], s["dev"], s["params"], s["z"], s["e"], s["d"].to(s["dev"])

    def same(p, w):
        return all(torch.equal(a, b) for a, b in zip(p.d_z(w), s["dz"])) and torch.equal(p.d_emb(w), s["de"])
    flagged = RaggedPlan(s["cfg"], TZ, None, lib=s["lib"], mode="decode_ig")
    w1 = _nan_ws(flagged, dev)
    flagged.forward_latents(params, z, flagged.c_lat, e, w1)
    flagged.backward_decoder(params, z, flagged.c_lat, e, d, w1)
    assert all(torch.equal(a, b) for a, b in zip(flagged.outputs(w1), s["outs"]))
    assert same(flagged, w1)
    w2 = _nan_ws(plan, dev)
    plan.forward_latents(params, z, plan.c_lat, e, w2)
    plan.backward_decoder(params, z, plan.c_lat, e, d, w2)   # the frozen pass on the new plan
    assert same(plan, w2)
    g1 = torch.full_like(s["grads"], float("nan"))
    plan.backward_decoder_params(params, z, plan.c_lat, e, d, g1, s["ws"])
    g2 = torch.full_like(s["grads"], float("nan"))
    plan.backward_decoder_params(params, z, plan.c_lat, e, d, g2, w2)
    for g in (g1, g2):
        assert torch.equal(g.view(torch.int32), s["grads"].view(torch.int32))
    assert same(plan, w2)


@pytest.mark.parametrize("kind", KINDS)
def test_refusals(kind):
    """5. avc_decoder_backward_ragged_params: -8 with the creator's name on every other kind of plan, -8 under bf16, -1 on a null argument;
    the old creators and RaggedPlan(mode="decode", input_grads=True) refuse what they refused; the module raises under bf16."""
    s = _pass(kind)
    lib, dev, cfg = s["lib"], s["dev"], s["cfg"]
    buf = torch.zeros(64, device=dev)
    p = ctypes.c_void_p(buf.data_ptr())
    zc = s["plan"].c_lat

    def call(plan, **kw):
        a = dict(params=p, z=p, emb=p, d=p, grads=p, ws=p)
        a.update(kw)
        return lib.avc_decoder_backward_ragged_params(plan.h, a["params"], a["z"], zc, a["emb"], 4, 1, a["d"], a["grads"], a["ws"], None)
    T3 = [17, 64, 65]
    others = [RaggedPlan(cfg, [3, 5], None, lib=lib, mode="decode"), RaggedPlan(cfg, [3, 5], None, lib=lib, mode="decode_ig"),
              RaggedPlan(cfg, [3, 5], None, lib=lib, mode="decode", src_of=[1, 0, 1]), RaggedPlan(cfg, None, T3, lib=lib, mode="speaker_pg"),
              RaggedPlan(cfg, T3, None, lib=lib, mode="encode_pg"), RaggedPlan(cfg, T3, None, lib=lib, mode="emb"),
              RaggedPlan(cfg, T3, T3, lib=lib, mode="pairs"), Plan(cfg, 2, 32, 32, lib=lib, mode="decoder_train")]
    for o in others:
        assert call(o) == -8, o.mode
        assert b"avc_plan_create_ragged_decoder_param_grads" in lib.avc_last_error()
    bf = RaggedPlan(cfg, [3, 5], None, lib=lib, mode="decode_pg", compute_dtype="bf16")
    assert call(bf) == -8 and b"bf16" in lib.avc_last_error()
    for k in ("params", "z", "emb", "d", "grads", "ws"):
        assert call(s["plan"], **{k: None}) == -1, k
    assert lib.avc_decoder_backward_ragged_params(None, p, p, zc, p, 4, 1, p, p, p, None) == -1
    assert lib.avc_decoder_backward_ragged_params(s["plan"].h, p, p, zc - 1, p, 4, 1, p, p, p, None) == -1
    assert lib.avc_decoder_backward_ragged_params(s["plan"].h, p, p, zc, p, -4, 1, p, p, p, None) == -1
    h = ctypes.c_void_p()
    ccfg = cfg_from_dict(cfg)
    lens = (ctypes.c_int * 2)(3, 5)
    src = (ctypes.c_int * 2)(0, 1)
    for flags in (L.PLAN_DECODER_ONLY | L.PLAN_INPUT_GRADS, L.PLAN_DECODER_ONLY | L.PLAN_PART_GRADS):
        assert lib.avc_plan_create_ragged_fanout(ctypes.byref(ccfg), 2, lens, 2, src, flags, None, ctypes.byref(h)) == -1, flags
    assert lib.avc_plan_create_ragged_decoder_param_grads(ctypes.byref(ccfg), 0, lens, None, ctypes.byref(h)) == -1
    assert lib.avc_plan_create_ragged_decoder_param_grads(ctypes.byref(ccfg), 2, None, None, ctypes.byref(h)) == -1
    short = (ctypes.c_int * 2)(5, 2)
    assert lib.avc_plan_create_ragged_decoder_param_grads(ctypes.byref(ccfg), 2, short, None, ctypes.byref(h)) == -6
    with pytest.raises(ValueError, match="forward only"):
        RaggedPlan(cfg, [3, 5], None, lib=lib, mode="decode", input_grads=True)
    with pytest.raises(RuntimeError, match="decode_pg"):
        others[1].backward_decoder_params(s["params"], s["z"], zc, s["e"], s["d"].to(dev), s["grads"], s["ws"])
    model = _model(kind, lib, dev, cfg, s["sd"], compute_dtype="bf16")
    with pytest.raises(RuntimeError, match="fp32 only"):
        model.decoder_ragged([z.to(dev) for z in s["zs"][:2]], s["emb"][:2].to(dev), param_grads=True)


@pytest.mark.parametrize("kind", KINDS)
def test_default_keeps_the_module_path(kind):
    """6. param_grads=False (the default): with only parameters requiring grad the outputs carry no grad_fn, and the forward bits are those
    of the param_grads=True call; with every decoder parameter frozen, or under no_grad, param_grads=True is the default call."""
    s = _pass(kind)
    dev = s["dev"]
    model = _model(kind, s["lib"], dev, s["cfg"], s["sd"])
    zs, emb = [z.to(dev) for z in s["zs"]], s["emb"].to(dev)
    outs = model.decoder_ragged(zs, emb)
    assert not any(t.requires_grad or t.grad_fn is not None for t in outs)
    assert all(torch.equal(a, b) for a, b in zip(outs, s["outs"]))
    assert not any(key[0] == "decode_pg" for key in model._ragged)
    for p in model.decoder.parameters():
        p.requires_grad_(False)
    assert not any(t.requires_grad for t in model.decoder_ragged(zs, emb, param_grads=True))
    with torch.no_grad():
        for p in model.decoder.parameters():
            p.requires_grad_(True)
        outs = model.decoder_ragged(zs, emb, param_grads=True)
    assert not any(t.requires_grad for t in outs) and all(torch.equal(a, b) for a, b in zip(outs, s["outs"]))
