"""The three networks called on their own -- ``ae.speaker_encoder(x)``, ``ae.content_encoder(x)``, ``ae.decoder(z, cond)`` (the
reference's sub-module calls, model.py:265-277 / 301-323 / 347-371) -- through the engine's part plans, with autograd.

kind='emu': CPU lane-level simulation of the same kernels on tiny instances; kind='gpu': the gfx950 library on the stock configs.
Bars as in test_engine.py: forward atol 2e-5 / rtol 1e-4; per-tensor gradient rel-L2 <= 1e-4 on the engine's own ReLU branch."""
import ctypes

import pytest
import torch

from adaptive_voice_conversion_amd import _lib
from adaptive_voice_conversion_amd.engine import Plan, cfg_from_dict
from adaptive_voice_conversion_amd.model import AE
from oracle import avc_oracle as O
from tests.emu_util import backend
from tests.test_engine import flat_params, get_cfg, zero_grad_bias

GPU = pytest.mark.gpu
NAN = float("nan")


def make_ae(kind, cfg, seed, **kw):
    lib, dev = backend(kind)
    ae = AE(cfg, lib=lib, **kw) if kind == "emu" else AE(cfg, **kw).to(dev)
    sd = O.make_state_dict(cfg, seed)
    ae.load_state_dict(sd)
    return ae, sd, dev


def poison(ae, mode, B, T, dev):
    """Create the (mode, B, T) plan of the AE's cache now and fill its workspace with NaN: every value a call returns was written by it."""
    ae._entry(mode, B, T, T, dev).ws.fill_(NAN)


def rel(a, b):
    return ((a.detach().cpu() - b).norm() / b.norm().clamp_min(1e-30)).item()


def part_ws(ae, mode, B, T, dev):
    e = ae._entry(mode, B, T, T, dev)
    return e.plan, e.ws


def check_part_grads(ae, leaves, part, cfg, tol=1e-4):
    """Gradients of `part`'s parameters vs the oracle leaves' .grad; every other network's parameters keep .grad None."""
    prefix = {"speaker": "speaker_encoder.", "content": "content_encoder.", "decoder": "decoder."}[part]
    worst = 0.0
    # (the analytically-zero bias gradients, SURVEY §8c, are fp32 noise on both sides: bounded relative to the whole part's gradient,
    # whose scale is set by the random upstream gradient here)
    for k, v in leaves.items():   # (a parameter the oracle's loss does not reach: zero gradient, e.g. std_layer for a mu-only loss)
        if v.grad is None:
            v.grad = torch.zeros_like(v)
    scale = sum(leaves[k].grad.norm() ** 2 for k, _ in ae.named_parameters() if k.startswith(prefix)) ** 0.5
    for k, p in ae.named_parameters():
        if not k.startswith(prefix):
            assert p.grad is None, k
            continue
        g, gref = p.grad.detach().cpu(), leaves[k].grad
        assert torch.isfinite(g).all(), k
        if zero_grad_bias(k, cfg):
            assert gref.norm() < 1e-6 * scale and (g - gref).norm() < 1e-6 * scale, (k, gref.norm(), (g - gref).norm(), scale)
            continue
        r = rel(g, gref)
        worst = max(worst, r)
        assert r <= tol, (k, r)
    return worst


FWD_CASES = [("emu", "tiny", 2, 32, False), ("emu", "tiny_lrelu", 3, 40, True), ("emu", "tiny8", 2, 32, False), ("emu", "tiny128", 2, 40, False),
             pytest.param("gpu", "m80", 4, 128, True, marks=GPU), pytest.param("gpu", "m80", 3, 40, False, marks=GPU),
             pytest.param("gpu", "m512", 2, 128, False, marks=GPU)]


@pytest.mark.parametrize("kind,cfgname,B,T,transposed", FWD_CASES)
def test_submodule_forward_vs_oracle(kind, cfgname, B, T, transposed):
    cfg = get_cfg(cfgname)
    ae, sd, dev = make_ae(kind, cfg, 3)
    x, _ = O.make_inputs(cfg, B, T, 3)
    x2, _ = O.make_inputs(cfg, B, T, 9)
    xd = x.to(dev)
    if transposed:
        xd = xd.transpose(1, 2).contiguous().transpose(1, 2)   # collate view, strides (T*M, 1, M)
    Tb = O.latent_len(cfg, T)
    poison(ae, "speaker", B, T, dev)
    poison(ae, "content", B, T, dev)
    with torch.no_grad():
        emb = ae.speaker_encoder(xd)
        mu, ls = ae.content_encoder(xd)
        emb2 = ae.speaker_encoder(x2.to(dev))
    assert emb.shape == (B, cfg["SpeakerEncoder"]["c_out"]) and mu.shape == ls.shape == (B, cfg["ContentEncoder"]["c_out"], Tb)
    torch.testing.assert_close(emb.cpu(), O.speaker_encoder(x, sd, cfg), rtol=1e-4, atol=2e-5)
    omu, ols = O.content_encoder(x, sd, cfg)
    torch.testing.assert_close(mu.cpu(), omu, rtol=1e-4, atol=2e-5)
    torch.testing.assert_close(ls.cpu(), ols, rtol=1e-4, atol=2e-5)
    # a random latent (not an encoder output) as a non-contiguous view with an odd length; the mean of two utterances' embeddings
    Tz = 7
    z = torch.randn(B, Tz, cfg["ContentEncoder"]["c_out"], generator=torch.Generator().manual_seed(5)).transpose(1, 2)
    cond = (emb + emb2) / 2
    poison(ae, "decoder", B, Tz, dev)
    zd = z.to(dev).transpose(1, 2).contiguous().transpose(1, 2) if kind == "gpu" else z
    assert not zd.is_contiguous()
    with torch.no_grad():
        dec = ae.decoder(zd, cond)
    ref = O.decoder(z, cond.cpu(), sd, cfg)
    assert dec.shape == ref.shape
    torch.testing.assert_close(dec.cpu(), ref, rtol=1e-4, atol=2e-5)


@pytest.mark.parametrize("kind,B,T", [("emu", 6, 32), pytest.param("gpu", 256, 128, marks=GPU)])
def test_parts_run_the_whole_plans_kernels(kind, B, T):
    """fp32: decoder(content_encoder(x)[0], speaker_encoder(x)) is bit-identical to AE.inference(x, x), and the parts' training
    forwards to the mu / log_sigma / emb of AE.forward: a branch runs the same kernel instances in a part plan and in a whole plan.
    The emulated case lowers dec_split_min so that its decoder runs as two half-batch chains, as B = 256 does on the GPU."""
    cfg = O.tiny_config() if kind == "emu" else O.stock_config(80)
    ae, sd, dev = make_ae(kind, cfg, 4, tuning={"dec_split_min": 4} if kind == "emu" else None)
    x, eps = O.make_inputs(cfg, B, T, 4)
    x, eps = x.to(dev), eps.to(dev)
    with torch.no_grad():
        ref = ae.inference(x, x)
        dec = ae.decoder(ae.content_encoder(x)[0], ae.speaker_encoder(x))
    assert torch.equal(dec, ref)
    mu, ls, emb, _ = ae(x, eps)
    pmu, pls = ae.content_encoder(x)
    pemb = ae.speaker_encoder(x)
    assert pmu.requires_grad and pemb.requires_grad
    assert torch.equal(pmu, mu) and torch.equal(pls, ls) and torch.equal(pemb, emb)


GRAD_CASES = [("emu", "tiny", 2, 32), ("emu", "tiny_lrelu", 3, 40), pytest.param("gpu", "m80", 4, 128, marks=GPU)]


@pytest.mark.parametrize("kind,cfgname,B,T", GRAD_CASES)
def test_decoder_gradients_vs_oracle(kind, cfgname, B, T):
    cfg = get_cfg(cfgname)
    ae, sd, dev = make_ae(kind, cfg, 6)
    g = torch.Generator().manual_seed(6)
    Tb = O.latent_len(cfg, T)
    z = torch.randn(B, cfg["ContentEncoder"]["c_out"], Tb, generator=g)
    emb = torch.randn(B, cfg["SpeakerEncoder"]["c_out"], generator=g)
    zd, ed = z.to(dev, copy=True).requires_grad_(True), emb.to(dev, copy=True).requires_grad_(True)
    poison(ae, "decoder_train", B, Tb, dev)
    dec = ae.decoder(zd, ed)
    d_dec = torch.randn(dec.shape, generator=g)
    dec.backward(d_dec.to(dev))
    plan, ws = part_ws(ae, "decoder_train", B, Tb, dev)
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    zr, er = z.clone().requires_grad_(True), emb.clone().requires_grad_(True)
    with O.relu_masks([m.cpu() for m in plan.relu_masks(ws)]):
        O.decoder(zr, er, leaves, cfg).backward(d_dec)
    assert rel(zd.grad, zr.grad) <= 1e-4 and rel(ed.grad, er.grad) <= 1e-4, (rel(zd.grad, zr.grad), rel(ed.grad, er.grad))
    check_part_grads(ae, leaves, "decoder", cfg)


@pytest.mark.parametrize("which", ["mu", "log_sigma", "both"])
@pytest.mark.parametrize("kind,cfgname,B,T", GRAD_CASES)
def test_content_encoder_gradients_vs_oracle(kind, cfgname, B, T, which):
    cfg = get_cfg(cfgname)
    ae, sd, dev = make_ae(kind, cfg, 7)
    x, _ = O.make_inputs(cfg, B, T, 7)
    g = torch.Generator().manual_seed(7)
    poison(ae, "content_train", B, T, dev)
    mu, ls = ae.content_encoder(x.to(dev))
    d_mu, d_ls = torch.randn(mu.shape, generator=g), torch.randn(ls.shape, generator=g)
    loss = {"mu": lambda m, s: (m * d_mu.to(m.device)).sum(), "log_sigma": lambda m, s: (s * d_ls.to(s.device)).sum(),
            "both": lambda m, s: (m * d_mu.to(m.device)).sum() + (s * d_ls.to(s.device)).sum()}[which]
    loss(mu, ls).backward()
    plan, ws = part_ws(ae, "content_train", B, T, dev)
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    with O.relu_masks([m.cpu() for m in plan.relu_masks(ws)]):
        loss(*O.content_encoder(x, leaves, cfg)).backward()
    check_part_grads(ae, leaves, "content", cfg)


@pytest.mark.parametrize("kind,cfgname,B,T", GRAD_CASES)
def test_speaker_encoder_gradients_vs_oracle(kind, cfgname, B, T):
    cfg = get_cfg(cfgname)
    ae, sd, dev = make_ae(kind, cfg, 8)
    x, _ = O.make_inputs(cfg, B, T, 8)
    poison(ae, "speaker_train", B, T, dev)
    emb = ae.speaker_encoder(x.to(dev))
    d_emb = torch.randn(emb.shape, generator=torch.Generator().manual_seed(8))
    emb.backward(d_emb.to(dev))
    plan, ws = part_ws(ae, "speaker_train", B, T, dev)
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    with O.relu_masks([m.cpu() for m in plan.relu_masks(ws)]):
        O.speaker_encoder(x, leaves, cfg).backward(d_emb)
    check_part_grads(ae, leaves, "speaker", cfg)


def written_out_step(ae, x, eps, lambda_rec, lambda_kl):
    """AE.forward written out with the sub-modules (reference model.py:380-385) + the loss of solver.py:84-88."""
    mu, ls = ae.content_encoder(x)
    emb = ae.speaker_encoder(x)
    dec = ae.decoder(mu + torch.exp(ls / 2) * eps, emb)
    loss = lambda_rec * (dec - x).abs().mean() + lambda_kl * 0.5 * torch.mean(torch.exp(ls) + mu ** 2 - 1 - ls)
    loss.backward()
    return mu, ls, emb, dec


def whole_step(ae, x, eps, lambda_rec, lambda_kl):
    mu, ls, emb, dec = ae(x, eps)
    loss = lambda_rec * (dec - x).abs().mean() + lambda_kl * 0.5 * torch.mean(torch.exp(ls) + mu ** 2 - 1 - ls)
    loss.backward()
    return mu, ls, emb, dec


@pytest.mark.parametrize("kind,cfgname,B,T,mode", [
    ("emu", "tiny", 2, 32, "fp32"), ("emu", "tiny", 2, 32, "bf16"), ("emu", "tiny", 2, 32, "fp32x3"),
    pytest.param("gpu", "m80", 4, 128, "fp32", marks=GPU), pytest.param("gpu", "m80", 256, 128, "fp32", marks=GPU)])
def test_reference_forward_written_out_matches_ae_forward(kind, cfgname, B, T, mode):
    """Gradients of the reference's AE.forward written out with the three sub-modules == those of AE(x, eps) (_AEFunction) on the
    same inputs.  The encoders' outputs are bit-identical (same kernels); the decoder's input z is computed by torch here and by the
    engine's reparameterisation kernel there (exp rounding may differ in the last bit), so dec gets a tolerance."""
    cfg = get_cfg(cfgname)
    ae, sd, dev = make_ae(kind, cfg, 2, compute_dtype=mode)
    x, eps = O.make_inputs(cfg, B, T, 2)
    x, eps = x.to(dev), eps.to(dev)
    lam = (cfg["lambda"]["lambda_rec"], 1.0)
    parts = written_out_step(ae, x, eps, *lam)
    g_parts = {k: p.grad.detach().clone() for k, p in ae.named_parameters()}
    for p in ae.parameters():
        p.grad = None
    whole = whole_step(ae, x, eps, *lam)
    for a, b in zip(parts[:3], whole[:3]):
        assert torch.equal(a, b)
    torch.testing.assert_close(parts[3], whole[3], rtol=1e-2 if mode == "bf16" else 1e-4, atol=1e-3 if mode == "bf16" else 2e-5)
    tol = 1e-3 if mode == "bf16" else 1e-4
    for k, p in ae.named_parameters():
        gref = p.grad.detach()
        if zero_grad_bias(k, cfg):
            assert (g_parts[k] - gref).norm() < 1e-5, k
            continue
        r = rel(g_parts[k], gref.cpu())
        assert r <= tol, (k, r)


@pytest.mark.parametrize("kind,cfgname,B,T", [("emu", "tiny", 2, 32), pytest.param("gpu", "m80", 4, 128, marks=GPU)])
def test_two_decoder_calls_in_one_graph(kind, cfgname, B, T):
    """The second forward of the same shape before the first one's backward gets a private workspace."""
    cfg = get_cfg(cfgname)
    ae, sd, dev = make_ae(kind, cfg, 11)
    g = torch.Generator().manual_seed(11)
    Tb = O.latent_len(cfg, T)
    z = torch.randn(B, cfg["ContentEncoder"]["c_out"], Tb, generator=g).to(dev)
    ea, eb = (torch.randn(B, cfg["SpeakerEncoder"]["c_out"], generator=g).to(dev) for _ in range(2))
    with torch.no_grad():
        Tout = ae.decoder(z, ea).shape[2]
    d_dec = torch.randn(B, cfg["Decoder"]["c_out"], Tout, generator=g).to(dev)

    def run(pairs):
        for p in ae.parameters():
            p.grad = None
        leaves = [(z.clone().requires_grad_(True), e.clone().requires_grad_(True)) for e in pairs]
        out = sum(ae.decoder(zz, ee) for zz, ee in leaves)
        out.backward(d_dec)
        return [t.grad.clone() for pr in leaves for t in pr], {k: p.grad.clone() for k, p in ae.named_parameters() if p.grad is not None}

    both_in, both_p = run([ea, eb])
    a_in, a_p = run([ea])
    b_in, b_p = run([eb])
    assert set(both_p) == set(a_p) and all(k.startswith("decoder.") for k in both_p)
    for k in both_p:
        ref = a_p[k] + b_p[k]
        assert (both_p[k] - ref).norm() <= 1e-5 * ref.norm() + 1e-7, k
    for got, ref in zip(both_in, a_in + b_in):
        torch.testing.assert_close(got, ref, rtol=1e-5, atol=1e-7)


# ---- C ABI of the part plans (host-side checks + one emulated backward)
def _plan(lib, cfg, B, T, flags):
    h = ctypes.c_void_p()
    rc = lib.avc_plan_create_ex(ctypes.byref(cfg), B, T, T, flags, ctypes.byref(h))
    return rc, h


def test_part_plan_abi_errors_and_sizes():
    lib, _ = backend("emu")
    cfg = cfg_from_dict(O.tiny_config())
    B, T = 2, 32
    Tb = O.latent_len(O.tiny_config(), T)
    S, C, D, G = _lib.PLAN_SPEAKER_ONLY, _lib.PLAN_CONTENT_ONLY, _lib.PLAN_DECODER_ONLY, _lib.PLAN_PART_GRADS
    assert _plan(lib, cfg, B, T, S | C)[0] == -1            # two part flags
    assert _plan(lib, cfg, B, T, C | D | G)[0] == -1
    assert _plan(lib, cfg, B, T, G)[0] == -1                # PART_GRADS without a part
    assert _plan(lib, cfg, B, T, C | G | _lib.PLAN_INFERENCE)[0] == -1
    assert _plan(lib, cfg, B, 2, D)[0] == -6                # the decoder's reflect-pad rule on Tb
    plans = {}
    for name, fl, t in (("whole", 0, T), ("whole_inf", _lib.PLAN_INFERENCE, T), ("spk", S, T), ("spk_g", S | G, T), ("enc", C, T),
                        ("enc_g", C | G, T), ("dec", D, Tb), ("dec_g", D | G, Tb)):
        rc, h = _plan(lib, cfg, B, t, fl)
        assert rc == 0, (name, lib.avc_last_error())
        plans[name] = h
    try:
        ws = {k: lib.avc_plan_workspace_floats(h) for k, h in plans.items()}
        for k in ("spk_g", "enc_g", "dec_g"):
            assert ws[k] < ws["whole"], k
        for k in ("spk", "enc", "dec"):
            assert ws[k] < ws["whole_inf"], k
        assert lib.avc_plan_flags(plans["spk"]) & _lib.PLAN_INFERENCE and not lib.avc_plan_flags(plans["spk_g"]) & _lib.PLAN_INFERENCE
        dcfg = O.tiny_config()["Decoder"]
        up = 1
        for u in dcfg["upsample"][:dcfg["n_conv_blocks"]]:
            up *= u
        assert lib.avc_plan_out_len(plans["dec"]) == Tb * up and lib.avc_plan_latent_len(plans["dec"]) == Tb
        assert lib.avc_plan_param_floats(plans["dec"]) == lib.avc_plan_param_floats(plans["whole"])
        buf = torch.zeros(1 << 20)
        p = ctypes.c_void_p(buf.data_ptr())
        # wrong entry points
        assert lib.avc_decoder_forward(plans["enc"], p, p, 1, 1, 1, p, 1, 1, p, 0, None) == -8
        assert lib.avc_decoder_forward(plans["whole"], p, p, 1, 1, 1, p, 1, 1, p, 0, None) == -8
        assert lib.avc_forward(plans["dec"], p, p, 1, 1, 1, None, 0, 0, 0, None, p, None) == -8
        assert lib.avc_forward_ex(plans["dec_g"], p, p, 1, 1, 1, None, 0, 0, 0, None, p, 0, None) == -8
        assert lib.avc_backward(plans["dec_g"], p, p, 1, 1, 1, None, 0, 0, 0, None, None, None, None, 0.0, p, p, None) == -8
        assert lib.avc_decoder_backward(plans["dec"], p, p, 1, 1, 1, p, 1, 1, None, p, p, None) == -8       # no PART_GRADS
        assert lib.avc_decoder_backward(plans["enc_g"], p, p, 1, 1, 1, p, 1, 1, None, p, p, None) == -8
        for k in ("spk", "enc"):                                                                             # no PART_GRADS
            assert lib.avc_backward(plans[k], p, p, 1, 1, 1, None, 0, 0, 0, None, None, p, p, 0.0, p, p, None) == -8
        # missing / extra upstream buffers
        assert lib.avc_backward(plans["enc_g"], p, p, 1, 1, 1, None, 0, 0, 0, None, p, p, None, 0.0, p, p, None) == -1
        assert lib.avc_backward(plans["enc_g"], p, p, 1, 1, 1, None, 0, 0, 0, None, None, p, p, 0.0, p, p, None) == -1
        assert lib.avc_backward(plans["spk_g"], p, p, 1, 1, 1, None, 0, 0, 0, None, None, None, None, 0.0, p, p, None) == -1
        assert lib.avc_backward(plans["spk_g"], p, p, 1, 1, 1, None, 0, 0, 0, None, None, p, p, 0.0, p, p, None) == -1
        assert lib.avc_decoder_forward(plans["dec"], p, None, 1, 1, 1, p, 1, 1, p, 0, None) == -1
        for k in ("spk_g", "enc_g", "dec_g"):                                                                # no loss on part plans
            assert lib.avc_loss(plans[k], p, 1, 1, 1, 1.0, p, None) == -8
            assert b"part plan" in lib.avc_last_error()
    finally:
        for h in plans.values():
            lib.avc_plan_destroy(h)


@pytest.mark.parametrize("mode,part", [("speaker_train", _lib.GRADS_SPEAKER), ("content_train", _lib.GRADS_CONTENT),
                                       ("decoder_train", _lib.GRADS_DECODER)])
def test_part_backward_writes_only_its_range(mode, part):
    lib, dev = backend("emu")
    cfg = O.tiny_config()
    B, T = 2, 32
    Tb = O.latent_len(cfg, T)
    plan = Plan(cfg, B, Tb if mode == "decoder_train" else T, lib=lib, mode=mode)
    params = flat_params(plan, O.make_state_dict(cfg, 1), dev)
    ws = torch.full((plan.workspace_floats,), NAN)
    grads = torch.full((plan.param_floats,), NAN)
    x, _ = O.make_inputs(cfg, B, T, 1)
    g = torch.Generator().manual_seed(1)
    if mode == "decoder_train":
        z = torch.randn(B, cfg["ContentEncoder"]["c_out"], Tb, generator=g)
        emb = torch.randn(B, cfg["SpeakerEncoder"]["c_out"], generator=g)
        plan.decoder_forward(params, z, emb, ws)
        plan.decoder_backward(params, z, emb, grads, ws, d_dec=torch.randn(B, cfg["Decoder"]["c_out"], plan.out_len, generator=g))
        assert torch.isfinite(plan.view(ws, "d_z", (B, z.shape[1], Tb))).all() and torch.isfinite(plan.view(ws, "d_emb", emb.shape)).all()
    elif mode == "content_train":
        plan.forward(params, x, None, None, ws)
        plan.backward(params, x, None, None, grads, ws, d_muls=torch.randn(B, 2 * cfg["ContentEncoder"]["c_out"], Tb, generator=g), lambda_kl=1.0)
    else:
        plan.forward(params, x, None, None, ws)
        plan.backward(params, x, None, None, grads, ws, d_emb=torch.randn(B, cfg["SpeakerEncoder"]["c_out"], generator=g))
    off, n = plan.param_range(part)
    mine = torch.zeros(plan.param_floats, dtype=torch.bool)
    for o, k, _ in plan.param_info:
        if off <= o < off + n:
            mine[o:o + k] = True
    assert torch.isfinite(grads[mine]).all()
    assert torch.isnan(grads[:off]).all() and torch.isnan(grads[off + n:]).all()
