"""``Solver.ae_step_ragged``: one training step over whole utterances of different lengths -- the three ragged grad plans with the
packed-row loss kernels between them, the gradients written straight into ``model.flat_grads()``, then the fused clip+Adam kernel.

Lengths [17, 65, 66, 130] (those of tests/test_ragged_whole_utterance_step.py).  kind='emu': the CPU lane-level simulation on the tiny
config; kind='gpu': the gfx950 library on the stock 80-mel config.

(a) eps=False, apply=False: dec bit-equal to content_encoder_ragged / speaker_encoder_ragged / decoder_ragged on the same utterances; the
    two losses equal the torch expression of the whole-utterance test within rtol 1e-4.
(b) a fixed non-zero eps, apply=False: EVERY tensor of flat_grads() within the project's bar -- err(engine, fp64 oracle) <= max(1e-4, 2 x
    err(fp32 oracle, fp64 oracle)) in rel-L2, near-zero tensors absolutely (``tests.ragged_param_oracle.check``) -- against
    ``tests.ragged_step_oracle.noisy_step_oracle`` on the engine's own branch (masks from the three plans' workspaces, signs from the
    engine's dec).
(c) apply=True: the parameters after one step are, bit for bit, FusedClipAdam.step on a copy of the model whose flat_grads hold (b)'s.
(d) eps=None draws noise of the right size, differently on every call; bf16, an empty list and a world size of 2 are refused."""
import functools
import types

import pytest
import torch

from adaptive_voice_conversion_amd import solver as solver_module
from adaptive_voice_conversion_amd.model import AE
from adaptive_voice_conversion_amd.optim import FusedClipAdam
from adaptive_voice_conversion_amd.solver import Solver
from oracle import avc_oracle as O
from tests.emu_util import KINDS, backend
from tests.ragged_oracle import content_masks, decoder_masks, speaker_masks
from tests.ragged_param_oracle import DEC, ENC, SPK, check, tensors
from tests.ragged_step_oracle import noisy_step_oracle
from tests.test_ragged_enroll import _utts

T_UTT = [17, 65, 66, 130]
LAMBDA_KL = 0.5


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _setup(kind):
    lib, dev = backend(kind)
    cfg = O.tiny_config() if kind == "emu" else O.stock_config(80)
    sd = O.make_state_dict(cfg, 21)
    return lib, dev, cfg, sd, _utts(T_UTT, cfg["ContentEncoder"]["c_in"], 9)


def _solver(kind, lib, cfg, sd):
    args = types.SimpleNamespace(store_model_path=None, load_model=False, data_dir=None, logdir="/tmp/avc_ragged_step_log")
    s = Solver(cfg, args, lib=lib if kind == "emu" else None)
    s.model.load_state_dict(sd)
    return s


def _eps(cfg, Tz, seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(cfg["ContentEncoder"]["c_out"] * sum(Tz), generator=g)


@functools.lru_cache(maxsize=None)
def _step_b(kind):
    """(b)'s step, shared with (c): the solver after ae_step_ragged(eps, apply=False), its gradients and what the step returned"""
    lib, dev, cfg, sd, xs = _setup(kind)
    s = _solver(kind, lib, cfg, sd)
    Tz = [O.latent_len(cfg, t) for t in T_UTT]
    eps = _eps(cfg, Tz)
    meta = s.ae_step_ragged([x.to(dev) for x in xs], LAMBDA_KL, eps=eps.to(dev), apply=False)
    return s, s.model.flat_grads().detach().clone(), eps, meta


@functools.lru_cache(maxsize=None)
def _step_a(kind):
    """(a)'s step, shared with (d): the solver after ae_step_ragged(eps=False, apply=False), what the step returned and its dec blocks"""
    lib, dev, cfg, sd, xs = _setup(kind)
    s = _solver(kind, lib, cfg, sd)
    before = s.model.flat_parameters().clone()
    meta = s.ae_step_ragged([x.to(dev) for x in xs], LAMBDA_KL, eps=False, apply=False)
    assert set(meta) == {"loss_rec", "loss_kl"} and s.opt.step_count == 0
    assert torch.equal(_bits(s.model.flat_parameters()), _bits(before))
    (pe, ps, pd), (wse, wss, wsd), tab = s._rag_last
    return s, meta, [d.clone() for d in pd.outputs(wsd)]


@pytest.mark.parametrize("kind", KINDS)
def test_forward_and_losses_without_noise(kind):
    lib, dev, cfg, sd, xs = _setup(kind)
    s, meta, dec = _step_a(kind)
    with torch.no_grad():
        mu, ls = s.model.content_encoder_ragged([x.to(dev) for x in xs])
        emb = s.model.speaker_encoder_ragged([x.to(dev) for x in xs])
        ref = s.model.decoder_ragged(mu, emb)
    assert [tuple(d.shape) for d in dec] == [tuple(r.shape) for r in ref]
    for j, (d, r) in enumerate(zip(dec, ref)):
        assert torch.equal(_bits(d), _bits(r)), f"dec of utterance {j} differs from the forward-only ragged calls"
    x_all = torch.cat([x.t().reshape(-1) for x in xs]).to(dev)
    dec_all = torch.cat([d[:, :x.shape[0]].reshape(-1) for d, x in zip(ref, xs)])
    mu_all, ls_all = torch.cat([m.reshape(-1) for m in mu]), torch.cat([v.reshape(-1) for v in ls])
    want = (float((dec_all - x_all).abs().mean()), float(0.5 * torch.mean(torch.exp(ls_all) + mu_all ** 2 - 1 - ls_all)))
    err = [abs(meta[k] - w) / abs(w) for k, w in zip(("loss_rec", "loss_kl"), want)]
    print(f"[{kind}] loss_rec {meta['loss_rec']:.6f} (rel err {err[0]:.2e}), loss_kl {meta['loss_kl']:.6f} (rel err {err[1]:.2e})")
    assert max(err) <= 1e-4, (meta, want)


@pytest.mark.parametrize("kind", KINDS)
def test_every_tensor_gets_its_gradient_with_noise(kind):
    lib, dev, cfg, sd, xs = _setup(kind)
    s, grads, eps, meta = _step_b(kind)
    (pe, ps, pd), (wse, wss, wsd), tab = s._rag_last
    assert list(tab.T) == T_UTT
    c = cfg["ContentEncoder"]["c_out"]
    eb = [eps[c * o:c * (o + t)].view(c, t) for t, o in zip(tab.Tz, [sum(tab.Tz[:i]) for i in range(tab.N)])]
    ms, me, md = speaker_masks(ps, wss), content_masks(pe, wse, cfg), decoder_masks(pd, wsd, cfg)
    masks = [ms[b] + me[b] + md[b] for b in range(len(xs))]
    signs = [torch.sign(d.detach().cpu()[:, :x.shape[0]] - x.t()) for d, x in zip(pd.outputs(wsd), xs)]
    lam_rec = cfg["lambda"]["lambda_rec"]
    r64, rec64, kl64 = noisy_step_oracle(cfg, sd, xs, eb, masks, signs, lam_rec, LAMBDA_KL, torch.float64)
    r32, _, _ = noisy_step_oracle(cfg, sd, xs, eb, masks, signs, lam_rec, LAMBDA_KL, torch.float32)
    got = tensors(pe, sd, grads, (SPK, ENC, DEC))
    assert len(got) == len(sd) == len(r64)   # no tensor is left out
    check(got, r64, r32, f"{kind} ragged train step, {len(r64)} tensors")
    err = (abs(meta["loss_rec"] - rec64) / abs(rec64), abs(meta["loss_kl"] - kl64) / abs(kl64))
    print(f"[{kind}] losses against the fp64 oracle: rel err {err[0]:.2e}, {err[1]:.2e}")
    assert max(err) <= 1e-4


@pytest.mark.parametrize("kind", KINDS)
def test_apply_is_the_fused_optimizer_on_those_gradients(kind):
    lib, dev, cfg, sd, xs = _setup(kind)
    _, grads, eps, meta_b = _step_b(kind)
    s = _solver(kind, lib, cfg, sd)
    meta = s.ae_step_ragged([x.to(dev) for x in xs], LAMBDA_KL, eps=eps.to(dev), apply=True)
    assert set(meta) == {"loss_rec", "loss_kl", "grad_norm"} and s.opt.step_count == 1
    assert (meta["loss_rec"], meta["loss_kl"]) == (meta_b["loss_rec"], meta_b["loss_kl"])
    assert torch.equal(_bits(s.model.flat_grads()), _bits(grads))
    twin = AE(cfg, lib=lib if kind == "emu" else None)
    twin.load_state_dict(sd)
    twin = twin.to(dev)
    twin.flat_grads().copy_(grads)
    o = cfg["optimizer"]
    opt = FusedClipAdam(twin, lr=o["lr"], betas=(o["beta1"], o["beta2"]), amsgrad=o["amsgrad"], weight_decay=o["weight_decay"],
                        lib=lib if kind == "emu" else None)
    gnorm = opt.step(o["grad_norm"])
    assert torch.equal(_bits(s.model.flat_parameters()), _bits(twin.flat_parameters()))
    assert not torch.equal(_bits(s.model.flat_parameters()), _bits(_solver(kind, lib, cfg, sd).model.flat_parameters().to(dev)))   # (it did step)
    assert meta["grad_norm"] == float(gnorm[0])
    for a, b in ((s.opt.m, opt.m), (s.opt.v, opt.v), (s.opt.vmax, opt.vmax)):
        assert torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("kind", KINDS)
def test_drawn_noise_and_refusals(kind, monkeypatch):
    lib, dev, cfg, sd, xs = _setup(kind)
    s, quiet, _ = _step_a(kind)
    utts = [x.to(dev) for x in xs]
    first = s.ae_step_ragged(utts, LAMBDA_KL, apply=False)
    n_lat = cfg["ContentEncoder"]["c_out"] * sum(s._rag_last[2].Tz)
    drawn = s._rag_bufs["eps"][:n_lat].clone()
    assert s._rag_bufs["eps"].numel() >= n_lat and torch.isfinite(drawn).all() and 0.9 < float(drawn.std()) < 1.1
    second = s.ae_step_ragged(utts, LAMBDA_KL, apply=False)
    assert not torch.equal(_bits(s._rag_bufs["eps"][:n_lat]), _bits(drawn))
    assert first["loss_kl"] == quiet["loss_kl"] == second["loss_kl"]           # (the KL term does not see the noise)
    assert len({quiet["loss_rec"], first["loss_rec"], second["loss_rec"]}) == 3
    with pytest.raises(ValueError, match="eps must be"):
        s.ae_step_ragged(utts, LAMBDA_KL, eps=torch.zeros(n_lat + 1, device=dev), apply=False)
    with pytest.raises(ValueError, match="empty list"):
        s.ae_step_ragged([], LAMBDA_KL)
    fake = types.SimpleNamespace(get_world_size=lambda: 2, get_rank=lambda: 0)
    with monkeypatch.context() as m:
        m.setattr(solver_module, "_dist", lambda: fake)
        with pytest.raises(RuntimeError, match="world size 2"):
            s.ae_step_ragged(utts, LAMBDA_KL)
    with monkeypatch.context() as m:
        m.setattr(s.model, "compute_dtype", "bf16")
        with pytest.raises(RuntimeError, match="fp32 only"):
            s.ae_step_ragged(utts, LAMBDA_KL)
    assert s.opt.step_count == 0
