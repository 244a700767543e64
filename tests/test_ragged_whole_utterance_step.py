"""A whole-utterance training step through the three ragged autograd functions: four (source, target) pairs of different lengths,
``content_encoder_ragged(param_grads=True)`` + ``speaker_encoder_ragged`` + ``decoder_ragged(param_grads=True)``, the reference's loss
(solver.py:84-86: L1 + lambda KL, z = mu, no noise) written in torch on the packed outputs, ONE ``backward()`` -- every tensor of the
checkpoint gets its gradient from ragged passes.

kind='emu': the CPU lane-level simulation on the tiny config; kind='gpu': the gfx950 library on the stock 80-mel config.

Bar, per tensor over ALL tensors, on the branch the engine took (activation masks of all three networks from the grad plans' saved rows;
the L1 term's sign(dec - x) from the engine's own output):  err(engine, fp64 oracle summed over the pairs) <= max(1e-4, 2 x err(fp32
oracle, fp64 oracle)) in rel-L2, near-zero tensors absolutely (``tests.ragged_param_oracle.check``)."""
import pytest
import torch

from oracle import avc_oracle as O
from tests.emu_util import KINDS, backend
from tests.ragged_oracle import content_masks, decoder_masks, speaker_masks
from tests.ragged_param_oracle import DEC, ENC, SPK, check, named_grads, step_oracle
from tests.test_ragged_enroll import _model, _utts

T_SRC = [17, 65, 66, 130]
T_TGT = [64, 19, 90, 33]
LAMBDA_KL = 0.5


@pytest.mark.parametrize("kind", KINDS)
def test_one_backward_gives_every_tensor_its_gradient(kind):
    lib, dev = backend(kind)
    cfg = O.tiny_config() if kind == "emu" else O.stock_config(80)
    sd = O.make_state_dict(cfg, 21)
    M = cfg["ContentEncoder"]["c_in"]
    xs, cs = _utts(T_SRC, M, 9), _utts(T_TGT, M, 10)
    model = _model(kind, lib, dev, cfg, sd)
    mu, ls = model.content_encoder_ragged([x.to(dev) for x in xs], param_grads=True)
    emb = model.speaker_encoder_ragged([c.to(dev) for c in cs])
    dec = model.decoder_ragged(mu, emb, param_grads=True)
    # the loss on the packed rows: every frame of every utterance counts once (the decoder's output is cropped to its source's length)
    x_all = torch.cat([x.t().reshape(-1) for x in xs]).to(dev)
    dec_all = torch.cat([d[:, :x.shape[0]].reshape(-1) for d, x in zip(dec, xs)])
    mu_all, ls_all = torch.cat([m.reshape(-1) for m in mu]), torch.cat([s.reshape(-1) for s in ls])
    loss = (dec_all - x_all).abs().mean() + LAMBDA_KL * 0.5 * torch.mean(torch.exp(ls_all) + mu_all ** 2 - 1 - ls_all)
    loss.backward()
    names = [k for k, _ in model.named_parameters()]
    assert len(names) == len(sd)
    for k, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
    # the branch the engine took: the saved rows of the three grad plans (a backward overwrites gradient rows only)
    Tz = tuple(int(m.shape[1]) for m in mu)
    ps, pe, pd = (model._ragged_plan("speaker_pg", (), tuple(T_TGT)), model._ragged_plan("encode_pg", tuple(T_SRC), ()),
                  model._ragged_plan("decode_pg", Tz, ()))
    ms, me, md = speaker_masks(ps[0], ps[1].ws), content_masks(pe[0], pe[1].ws, cfg), decoder_masks(pd[0], pd[1].ws, cfg)
    masks = [ms[b] + me[b] + md[b] for b in range(len(xs))]
    signs = [torch.sign(d.detach().cpu()[:, :x.shape[0]] - x.t()) for d, x in zip(dec, xs)]
    r64 = step_oracle(cfg, sd, xs, cs, masks, signs, LAMBDA_KL, torch.float64)
    r32 = step_oracle(cfg, sd, xs, cs, masks, signs, LAMBDA_KL, torch.float32)
    assert len(r64) == len(sd)
    check(named_grads(model, (SPK, ENC, DEC)), r64, r32, f"{kind} whole-utterance step, {len(r64)} tensors")
