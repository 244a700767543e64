"""Input gradients through ragged speaker enrolment: ``AE.get_speaker_embeddings_ragged(x_conds)`` is differentiable with respect to its
inputs -- a "speaker" RaggedPlan with AVC_PLAN_INPUT_GRADS, ``avc_backward_ragged``: the speaker encoder's backward pass over utterances of
different lengths in ONE ragged launch set, fp32, parameters frozen.

kind='emu': the CPU lane-level simulation of the same kernels on the tiny config; kind='gpu': the gfx950 library on the stock 80-mel
config.  Length sets: those of tests/test_ragged_enroll.py (17, 64, 65, odd lengths at every level, 600).

Bar: the project's input-gradient bar, rel-L2 <= 1e-4 per utterance against the fp64 oracle gradient of
``O.speaker_encoder`` on the ReLU branch the engine took (read from the plan's saved activations).  No utterance is filtered out."""
import ctypes

import pytest
import torch

from adaptive_voice_conversion_amd import _lib as L
from adaptive_voice_conversion_amd.engine import RaggedPlan, cfg_from_dict
from oracle import avc_oracle as O
from tests.emu_util import KINDS, backend
from tests.ragged_oracle import speaker_masks as _relu_masks
from tests.test_engine import flat_params
from tests.test_input_grads import oracle_input_grads
from tests.test_ragged_enroll import _model, _nan_ws, _setup, _utts
from tests.test_submodules import rel

BAR = 1e-4


def _leaves(cs, dev):
    return [c.to(dev, copy=True).requires_grad_(True) for c in cs]


def _d_emb(B, C, seed):
    return torch.randn(B, C, generator=torch.Generator().manual_seed(seed))


def _plan_pass(kind, seed=9, d_seed=31):
    """forward + backward of a flagged speaker plan in a NaN-filled workspace -> (plan, ws, params, utterances, d_emb, device, cfg, sd)"""
    lib, dev, cfg, sd, _, Tc = _setup(kind)
    M = cfg["ContentEncoder"]["c_in"]
    cs = _utts(Tc, M, seed)
    plan = RaggedPlan(cfg, None, Tc, lib=lib, mode="speaker", input_grads=True)
    params = flat_params(plan, sd, dev)
    ws = _nan_ws(plan, dev)
    xc = torch.cat(cs).to(dev)
    plan.forward(params, None, xc, ws)
    d = _d_emb(len(Tc), plan.c_emb, d_seed)
    plan.backward(params, xc, d.to(dev), ws)
    return plan, ws, params, cs, d, dev, cfg, sd


def _split(g, lens):
    return list(torch.split(g.detach().cpu(), list(lens)))


@pytest.mark.parametrize("kind", KINDS)
def test_gradient_parity_with_the_fp64_oracle(kind):
    """1. Every utterance a leaf, random d_emb: each .grad against the fp64 oracle gradient of O.speaker_encoder on the engine's own ReLU
    branch, rel-L2 <= 1e-4 per utterance.  Through the plan (NaN-filled workspace) and through the module."""
    plan, ws, params, cs, d, dev, cfg, sd = _plan_pass(kind)
    Tc = plan.T_cond
    grads = _split(plan.d_x_cond(ws), Tc)
    masks = _relu_masks(plan, ws)
    model = _model(kind, backend(kind)[0], dev, cfg, sd)
    leaves = _leaves(cs, dev)
    emb = model.get_speaker_embeddings_ragged(leaves)
    assert emb.requires_grad and emb.grad_fn is not None
    (emb * d.to(dev)).sum().backward()
    worst = 0.0
    for b, c in enumerate(cs):
        fn = lambda x, s: O.speaker_encoder(x, s, cfg)   # noqa: E731
        ref, = oracle_input_grads(fn, [c.t()[None]], sd, masks[b], [d[b][None]])
        ref = ref[0].t()   # [T_b, M]
        assert not torch.isnan(grads[b]).any()
        r_plan, r_mod = rel(grads[b], ref), rel(leaves[b].grad, ref)
        print(f"utterance {b} T={Tc[b]}: rel-L2 plan {r_plan:.3e} module {r_mod:.3e}")
        worst = max(worst, r_plan, r_mod)
        assert leaves[b].grad.shape == c.shape
        assert r_plan <= BAR and r_mod <= BAR, (b, Tc[b], r_plan, r_mod)
        assert torch.equal(leaves[b].grad.cpu(), grads[b])
    print("worst", worst)


@pytest.mark.parametrize("kind", KINDS)
def test_against_the_uniform_path(kind):
    """2. The same gradients against the engine's own get_speaker_embeddings(x_b) at B = 1, rel-L2 <= 1e-4."""
    lib, dev, cfg, sd, _, Tc = _setup(kind)
    M = cfg["ContentEncoder"]["c_in"]
    cs = _utts(Tc, M, 9)
    d = _d_emb(len(Tc), cfg["SpeakerEncoder"]["c_out"], 32)
    model = _model(kind, lib, dev, cfg, sd)
    leaves = _leaves(cs, dev)
    (model.get_speaker_embeddings_ragged(leaves) * d.to(dev)).sum().backward()
    for b, c in enumerate(cs):
        x = c.t()[None].to(dev, copy=True).requires_grad_(True)
        (model.get_speaker_embeddings(x) * d[b].to(dev)).sum().backward()
        r = rel(leaves[b].grad, x.grad[0].t().cpu())
        print(f"utterance {b} T={Tc[b]}: rel-L2 vs uniform {r:.3e}")
        assert r <= BAR, (b, Tc[b], r)


@pytest.mark.parametrize("kind", KINDS)
def test_forward_is_unchanged(kind):
    """3. The embedding on the grad path is bit-equal to the no-grad call; a speaker plan without the flag reports the workspace size it
    had before the flag existed and its output in a NaN-filled workspace is bit-equal to the flagged plan's forward."""
    lib, dev, cfg, sd, _, Tc = _setup(kind)
    M = cfg["ContentEncoder"]["c_in"]
    cs = _utts(Tc, M, 9)
    model = _model(kind, lib, dev, cfg, sd)
    with torch.no_grad():
        ref = model.get_speaker_embeddings_ragged([c.to(dev) for c in cs])
    got = model.get_speaker_embeddings_ragged(_leaves(cs, dev))
    assert got.requires_grad and not ref.requires_grad
    assert torch.equal(got.detach(), ref)
    plain = RaggedPlan(cfg, None, Tc, lib=lib, mode="speaker")
    flagged = RaggedPlan(cfg, None, Tc, lib=lib, mode="speaker", input_grads=True)
    assert lib.avc_plan_flags(flagged.h) & L.PLAN_INPUT_GRADS and not lib.avc_plan_flags(plain.h) & L.PLAN_INPUT_GRADS
    assert flagged.workspace_floats > plain.workspace_floats
    # the unflagged plan's workspace, restated from the layout: weight images, packed activations, dense rows, emb, level tables
    assert plain.workspace_floats == _speaker_plan_floats(cfg, Tc)
    params = flat_params(plain, sd, dev)
    xc = torch.cat(cs).to(dev)
    w0, w1 = _nan_ws(plain, dev), _nan_ws(flagged, dev)
    plain.forward(params, None, xc, w0)
    flagged.forward(params, None, xc, w1)
    assert not torch.isnan(plain.emb(w0)).any()
    assert torch.equal(plain.emb(w0), flagged.emb(w1))
    assert torch.equal(plain.emb(w0), ref)
    with pytest.raises(KeyError):
        plain.buffer("d_x_cond")


def _speaker_plan_floats(cfg, Tc):
    """avc_plan_workspace_floats of an unflagged ragged speaker plan with default tuning, from its documented layout (every allocation
    rounded up to 64 floats): forward weight images [chunk][tap][CK][Mp], Mp = rows rounded up to 128, CK = 32 / 16 / 8 channels per
    chunk for 1 / 2-3 / >= 4 taps; packed activations; dense rows; emb; the level tables (T, off, tiles per level, each padded to 4)."""
    c = cfg["SpeakerEncoder"]
    B = len(Tc)
    r64 = lambda n: (n + 63) // 64 * 64   # noqa: E731
    mp = lambda n: (n + 127) // 128 * 128   # noqa: E731
    ck = lambda k: 8 if k >= 4 else (16 if k >= 2 else 32)   # noqa: E731
    img = lambda co, ci, k: r64(-(-ci // ck(k)) * k * ck(k) * mp(co))   # noqa: E731
    nb = c["bank_size"] // c["bank_scale"]
    CC = nb * c["c_bank"] + c["c_in"]
    n = sum(img(c["c_bank"], c["c_in"], k) for k in range(c["bank_scale"], c["bank_size"] + 1, c["bank_scale"]))
    n += img(c["c_h"], CC, 1)
    n += 2 * c["n_conv_blocks"] * img(c["c_h"], c["c_h"], c["kernel_size"])
    n += 2 * c["n_dense_blocks"] * img(c["c_h"], c["c_h"], 1) + img(c["c_out"], c["c_h"], 1)
    levels = [list(Tc)]
    for s in c["subsample"][:c["n_conv_blocks"]]:
        levels.append([-(-t // s) for t in levels[-1]])
    S = [sum(lv) for lv in levels]
    n += r64(CC * S[0]) + r64(c["c_h"] * S[0])
    for l in range(c["n_conv_blocks"]):
        n += r64(c["c_h"] * S[l]) + 2 * r64(c["c_h"] * S[l + 1])
    n += r64(c["c_h"] * B) * (1 + 3 * c["n_dense_blocks"]) + r64(B * c["c_out"])
    r4 = lambda k: (k + 3) // 4 * 4   # noqa: E731
    n += r64(sum(r4(B) + r4(B + 1) + r4(2 * sum(-(-t // 64) for t in lv)) for lv in levels))
    return n


@pytest.mark.parametrize("kind", KINDS)
def test_reproducible_and_isolated(kind):
    """4. Two consecutive backward passes give identical bits (in a NaN-filled workspace); the gradient of utterance b does not change when
    the other utterances are replaced."""
    plan, ws, params, cs, d, dev, cfg, sd = _plan_pass(kind)
    Tc = plan.T_cond
    first = plan.d_x_cond(ws).clone()
    assert not torch.isnan(first).any()
    xc = torch.cat(cs).to(dev)
    plan.backward(params, xc, d.to(dev), ws)
    assert torch.equal(plan.d_x_cond(ws), first)
    # a fresh forward + backward in another NaN-filled workspace
    ws2 = _nan_ws(plan, dev)
    plan.forward(params, None, xc, ws2)
    plan.backward(params, xc, d.to(dev), ws2)
    assert torch.equal(plan.d_x_cond(ws2), first)
    # every other utterance replaced (same lengths, other content, other d_emb rows): utterance `keep` keeps its gradient bit for bit
    M = cs[0].shape[1]
    other = _utts(Tc, M, 77)
    d2 = _d_emb(len(Tc), plan.c_emb, 78)
    g0 = _split(first, Tc)
    for keep in (0, len(Tc) // 2, len(Tc) - 1):
        mix = [cs[b] if b == keep else other[b] for b in range(len(Tc))]
        dm = d2.clone()
        dm[keep] = d[keep]
        xm = torch.cat(mix).to(dev)
        ws3 = _nan_ws(plan, dev)
        plan.forward(params, None, xm, ws3)
        plan.backward(params, xm, dm.to(dev), ws3)
        g = _split(plan.d_x_cond(ws3), Tc)
        assert torch.equal(g[keep], g0[keep]), keep
        assert not torch.equal(g[(keep + 1) % len(Tc)], g0[(keep + 1) % len(Tc)])


@pytest.mark.parametrize("kind", KINDS)
def test_seams(kind):
    """5. Only a subset of the utterances are leaves; one leaf is a transposed view, one lives on the CPU; d_emb arrives with batch stride 0
    (the loss reads emb.mean(0)) and through the plan as an expanded row; under torch.no_grad() the call stays on the old path."""
    lib, dev, cfg, sd, _, Tc = _setup(kind)
    M = cfg["ContentEncoder"]["c_in"]
    cs = _utts(Tc, M, 9)
    B = len(Tc)
    model = _model(kind, lib, dev, cfg, sd)
    w = torch.randn(cfg["SpeakerEncoder"]["c_out"], generator=torch.Generator().manual_seed(5))
    # reference: every utterance a leaf, the same loss
    full = _leaves(cs, dev)
    (model.get_speaker_embeddings_ragged(full).mean(0) * w.to(dev)).sum().backward()
    # subset: utterances 0 (a transposed view of a [M, T] leaf), 2 (a CPU leaf) and B - 1 require grad
    base0 = cs[0].t().contiguous().to(dev).requires_grad_(True)      # [M, T]
    cpu2 = cs[2].clone().requires_grad_(True)                          # stays on the CPU: _ragged_rows moves it
    last = cs[B - 1].to(dev, copy=True).requires_grad_(True)
    ins = [c.to(dev) for c in cs]
    ins[0], ins[2], ins[B - 1] = base0.t(), cpu2, last
    assert not ins[0].is_contiguous() or Tc[0] == 1
    emb = model.get_speaker_embeddings_ragged(ins)
    assert emb.grad_fn is not None
    (emb.mean(0) * w.to(dev)).sum().backward()
    assert base0.grad.shape == base0.shape and cpu2.grad.shape == cpu2.shape and cpu2.grad.device.type == "cpu"
    assert torch.equal(base0.grad.t().cpu(), full[0].grad.cpu())
    assert torch.equal(cpu2.grad, full[2].grad.cpu())
    assert torch.equal(last.grad.cpu(), full[B - 1].grad.cpu())
    assert all(t.grad is None for i, t in enumerate(ins) if i not in (0, 2, B - 1))
    # the plan reads an expanded row (batch stride 0) and a column view (element stride 2) in place
    plan, ws, params, _, d, _, _, _ = _plan_pass(kind)
    xc = torch.cat(cs).to(dev)
    row = d[0].to(dev)
    plan.backward(params, xc, row[None].expand(B, -1), ws)
    g_exp = plan.d_x_cond(ws).clone()
    plan.backward(params, xc, row[None].expand(B, -1).contiguous(), ws)
    assert torch.equal(plan.d_x_cond(ws), g_exp)
    wide = torch.zeros(B, 2 * plan.c_emb, device=dev)
    wide[:, ::2] = d.to(dev)
    plan.backward(params, xc, wide[:, ::2], ws)
    g_col = plan.d_x_cond(ws).clone()
    plan.backward(params, xc, d.to(dev), ws)
    assert torch.equal(plan.d_x_cond(ws), g_col)
    # no grad: the forward-only path (no grad_fn, no grad plan is created for these lengths)
    n_ig = sum(1 for k in model._ragged if k[0] == "speaker_ig")
    lens2 = list(Tc[:-1])
    with torch.no_grad():
        e = model.get_speaker_embeddings_ragged([c.to(dev, copy=True).requires_grad_(True) for c in cs[:-1]])
    assert e.grad_fn is None and not e.requires_grad
    assert sum(1 for k in model._ragged if k[0] == "speaker_ig") == n_ig
    assert ("speaker", (), tuple(lens2), str(model._flat.device)) in model._ragged
    # inputs that do not require grad, grad enabled: the old path as well
    e2 = model.get_speaker_embeddings_ragged([c.to(dev) for c in cs[:-1]])
    assert e2.grad_fn is None and torch.equal(e2, e)


@pytest.mark.parametrize("kind", KINDS)
def test_a_forward_only_call_between_forward_and_backward_does_not_disturb_the_gradient(kind):
    """The grad plan's workspace is its own: another ragged call (the pooled workspace) and a second grad forward of the same lengths
    between a forward and its backward leave that backward's result unchanged."""
    lib, dev, cfg, sd, T, Tc = _setup(kind)
    M = cfg["ContentEncoder"]["c_in"]
    cs, other = _utts(Tc, M, 9), _utts(Tc, M, 55)
    d = _d_emb(len(Tc), cfg["SpeakerEncoder"]["c_out"], 33).to(dev)
    model = _model(kind, lib, dev, cfg, sd)
    ref = _leaves(cs, dev)
    (model.get_speaker_embeddings_ragged(ref) * d).sum().backward()
    a = _leaves(cs, dev)
    emb_a = model.get_speaker_embeddings_ragged(a)
    with torch.no_grad():
        model.get_speaker_embeddings_ragged([c.to(dev) for c in other])
        model.inference_ragged([x.to(dev) for x in _utts(T, M, 56)], [c.to(dev) for c in other])
    b = _leaves(other, dev)
    emb_b = model.get_speaker_embeddings_ragged(b)   # same lengths, the first backward still pending: a private workspace
    (emb_a * d).sum().backward()
    (emb_b * d).sum().backward()
    assert all(torch.equal(x.grad, y.grad) for x, y in zip(a, ref))
    assert not torch.equal(b[0].grad, a[0].grad)
    with pytest.raises(RuntimeError, match="twice"):
        (emb_a * d).sum().backward()


@pytest.mark.parametrize("kind", KINDS)
def test_refusals(kind):
    """6. What is out of scope is refused with a message that says what to pass."""
    lib, dev, cfg, sd, T, Tc = _setup(kind)
    M = cfg["ContentEncoder"]["c_in"]
    c = cfg_from_dict(cfg)
    arr = ctypes.c_int * len(Tc)
    tun = L.make_tuning(lib)

    def create(flags):
        h = ctypes.c_void_p()
        rc = lib.avc_plan_create_ragged_ex(ctypes.byref(c), len(Tc), arr(*T), arr(*Tc), flags, ctypes.byref(tun), ctypes.byref(h))
        return rc, lib.avc_last_error().decode()

    for flags in (L.PLAN_INPUT_GRADS | L.PLAN_EMB_INPUT, L.PLAN_INPUT_GRADS,
                  L.PLAN_INPUT_GRADS | L.PLAN_EMB_INPUT | L.PLAN_SPEAKER_ONLY):
        rc, msg = create(flags)
        assert rc == -1, flags
        assert "AVC_PLAN_SPEAKER_ONLY" in msg, msg
    with pytest.raises(RuntimeError, match="AVC_PLAN_SPEAKER_ONLY"):
        RaggedPlan(cfg, T, Tc, lib=lib, mode="pairs", input_grads=True)
    with pytest.raises(RuntimeError, match="AVC_PLAN_SPEAKER_ONLY"):
        RaggedPlan(cfg, T, None, lib=lib, mode="emb", input_grads=True)
    # avc_backward_ragged on plans without the flag: -8
    plain = RaggedPlan(cfg, None, Tc, lib=lib, mode="speaker")
    flagged = RaggedPlan(cfg, None, Tc, lib=lib, mode="speaker", input_grads=True)
    params = flat_params(plain, sd, dev)
    xc = torch.cat(_utts(Tc, M, 9)).to(dev)
    d = _d_emb(len(Tc), plain.c_emb, 1).to(dev)
    ws = torch.zeros(flagged.workspace_floats, device=dev)
    P = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    for other in (plain, RaggedPlan(cfg, T, Tc, lib=lib), RaggedPlan(cfg, T, None, lib=lib, mode="emb")):
        rc = lib.avc_backward_ragged(other.h, P(params), P(xc), P(d), d.stride(0), d.stride(1), P(ws), None)
        assert rc == -8
        assert "AVC_PLAN_SPEAKER_ONLY | AVC_PLAN_INPUT_GRADS" in lib.avc_last_error().decode()
    with pytest.raises(RuntimeError, match="input_grads=True"):
        plain.backward(params, xc, d, ws)
    # null arguments
    for args in ((None, P(params), P(xc), P(d), P(ws)), (flagged.h, None, P(xc), P(d), P(ws)), (flagged.h, P(params), None, P(d), P(ws)),
                 (flagged.h, P(params), P(xc), None, P(ws)), (flagged.h, P(params), P(xc), P(d), None)):
        rc = lib.avc_backward_ragged(args[0], args[1], args[2], args[3], d.stride(0), d.stride(1), args[4], None)
        assert rc == -1
        assert "null argument" in lib.avc_last_error().decode()
    # bf16 operand rounding: through the plan (-8) and through the module (a clear error that names the uniform path)
    bf = RaggedPlan(cfg, None, Tc, lib=lib, mode="speaker", input_grads=True, compute_dtype="bf16")
    wsb = torch.zeros(bf.workspace_floats, device=dev)
    bf.forward(params, None, xc, wsb)
    with pytest.raises(RuntimeError, match="fp32"):
        bf.backward(params, xc, d, wsb)
    model = _model(kind, lib, dev, cfg, sd, "bf16")
    with pytest.raises(RuntimeError, match=r"get_speaker_embeddings\(x_b\)"):
        model.get_speaker_embeddings_ragged(_leaves(_utts(Tc, M, 9), dev))
    with torch.no_grad():   # ... and without grad the bf16r call is what it was
        model.get_speaker_embeddings_ragged([t.to(dev) for t in _utts(Tc, M, 9)])
    assert model.last_ragged_compute == "bf16r"
    # inference_ragged keeps its refusal of an emb that requires grad
    fp = _model(kind, lib, dev, cfg, sd)
    e = torch.zeros(len(T), cfg["SpeakerEncoder"]["c_out"], device=dev, requires_grad=True)
    with pytest.raises(RuntimeError, match="forward-only"):
        fp.inference_ragged([x.to(dev) for x in _utts(T, M, 3)], emb=e)
