"""fp64 / fp32 oracles of the PARAMETER gradients of the ragged content encoder and decoder, beside ``tests.ragged_oracle.speaker_oracle``,
and what the three test files of those gradients share: the bar, the view of a flat gradient buffer as named tensors, and the oracle of a
whole-utterance training step through all three networks.

Test infrastructure only.  Every oracle runs utterance by utterance on the activation branch the engine took (``content_masks`` /
``decoder_masks`` / ``speaker_masks`` of tests/ragged_oracle.py) and sums the gradients over the utterances."""
import torch

from oracle import avc_oracle as O
from tests.test_submodules import rel

SPK, ENC, DEC = "speaker_encoder.", "content_encoder.", "decoder."


def _leaves(sd, dtype, prefixes):
    return {k: v.to(dtype).clone().requires_grad_(k.startswith(prefixes)) for k, v in sd.items()}


def _grads(leaves, prefixes):
    return {k: v.grad.double() for k, v in leaves.items() if k.startswith(prefixes)}


def content_oracle(cfg, sd, xs, masks, blocks, dtype):
    """{name: d(sum_s <mu_s, wm_s> + <log_sigma_s, wl_s>)/d(parameter)} of O.content_encoder in ``dtype``; xs[s] is [T_s, M], blocks[s] =
    (wm, wl), each [1, c_lat, Tz_s], masks[s] the branch of utterance s."""
    leaves = _leaves(sd, dtype, ENC)
    total = 0
    for x, m, (wm, wl) in zip(xs, masks, blocks):
        with O.relu_masks(m):
            mu, ls = O.content_encoder(x.t()[None].to(dtype), leaves, cfg)
        total = total + (mu * wm.to(dtype)).sum() + (ls * wl.to(dtype)).sum()
    total.backward()
    return _grads(leaves, ENC)


def decoder_oracle(cfg, sd, zs, emb, masks, blocks, dtype):
    """{name: d(sum_j <decoder(z_j, emb_j), w_j>)/d(parameter)} of O.decoder in ``dtype``; zs[j] is [c_lat, Tz_j], emb [N, c_emb] (one row
    per latent; pass an expanded row for one voice), blocks[j] = [1, M, T''_j]."""
    leaves = _leaves(sd, dtype, DEC)
    total = 0
    for j, (z, m, w) in enumerate(zip(zs, masks, blocks)):
        with O.relu_masks(m):
            dec = O.decoder(z[None].to(dtype), emb[j][None].to(dtype), leaves, cfg)
        total = total + (dec * w.to(dtype)).sum()
    total.backward()
    return _grads(leaves, DEC)


def step_oracle(cfg, sd, xs, cs, masks, signs, lam, dtype):
    """{name: d(loss)/d(parameter)} over ALL tensors of a whole-utterance step on the pairs (xs[b], cs[b]): emb = speaker(c_b), (mu, ls) =
    content(x_b), dec = decoder(mu, emb) (z = mu, no noise), loss = mean |dec[:, :T_b] - x_b| + lam * 0.5 * mean(exp(ls) + mu^2 - 1 - ls),
    both means over the PACKED elements of all pairs (solver.py:84-86 on packed rows).  masks[b] = speaker + content + decoder masks of
    pair b in call order; signs[b] = sign(dec - x) the engine's output has ([M, T_b]): the L1 term on the engine's branch."""
    leaves = _leaves(sd, dtype, (SPK, ENC, DEC))
    n_rec = sum(x.numel() for x in xs)
    rec, kl, n_kl = 0, 0, 0
    for x, c, m, s in zip(xs, cs, masks, signs):
        with O.relu_masks(m):
            emb = O.speaker_encoder(c.t()[None].to(dtype), leaves, cfg)
            mu, ls = O.content_encoder(x.t()[None].to(dtype), leaves, cfg)
            dec = O.decoder(mu, emb, leaves, cfg)
        T = x.shape[0]
        rec = rec + ((dec[0, :, :T] - x.t().to(dtype)) * s.to(dtype)).sum()
        kl = kl + (torch.exp(ls) + mu ** 2 - 1 - ls).sum()
        n_kl += mu.numel()
    (rec / n_rec + lam * 0.5 * kl / n_kl).backward()
    return _grads(leaves, (SPK, ENC, DEC))


def tensors(plan, sd, grads, prefixes):
    """{name: tensor} of the tensors under ``prefixes`` out of a flat gradient buffer"""
    g = grads.detach().cpu()
    return {k: g[off:off + n].view(shape).double() for (off, n, shape), k in zip(plan.param_info, sd) if k.startswith(prefixes)}


def named_grads(model, prefixes):
    return {k: p.grad.detach().cpu().double() for k, p in model.named_parameters() if k.startswith(prefixes) and p.grad is not None}


def check(got, r64, r32, tag):
    """The project's bar, per tensor, as ``_check`` of tests/test_ragged_speaker_param_grads.py: err(engine, fp64) <= max(1e-4, 2 x
    err(fp32 oracle, fp64)) in rel-L2 (r32 None: the plain 1e-4); a tensor whose reference norm is below 1e-6 of the whole gradient's norm
    -- the bias of every conv that feeds an InstanceNorm: its gradient is mathematically zero -- is compared absolutely against that
    scale.  No tensor is filtered out.  Returns and prints the worst."""
    assert set(got) == set(r64), (tag, sorted(set(got) ^ set(r64)))
    scale = sum(float(v.norm()) ** 2 for v in r64.values()) ** 0.5
    worst = (0.0, None, 0.0)
    for k, ref in r64.items():
        g = got[k]
        assert not torch.isnan(g).any(), k
        if float(ref.norm()) < 1e-6 * scale:
            assert float((g - ref).norm()) < 1e-5 * scale, (tag, k, float((g - ref).norm()), scale)
            continue
        e, e32 = rel(g, ref), (rel(r32[k], ref) if r32 is not None else 0.0)
        bar = max(1e-4, 2 * e32)
        if e / bar > worst[0]:
            worst = (e / bar, k, e)
        assert e <= bar, (tag, k, e, e32)
    print(f"[{tag}] worst tensor {worst[1]}: rel-L2 {worst[2]:.3e} ({worst[0]:.2f} of its bar)")
    return worst


def uniform_masks(model, mode, T, dev):
    """the activation branch the uniform B = 1 part plan of ``mode`` took in its last pass over T frames (its own saved tensors), as the
    oracle's mask list"""
    e = model._entry(mode, 1, T, T, dev)
    ms = [m.cpu().bool() for m in e.plan.relu_masks(e.ws)]
    assert any(bool(m.any()) for m in ms), "the uniform plan of this shape has not run"
    return ms


def flipped(a, b):
    """activation decisions that differ between two mask lists of one utterance"""
    assert len(a) == len(b)
    return sum(int((x.bool().reshape(y.shape) != y.bool()).sum()) for x, y in zip(a, b))


def written_mask(plan, sd, prefixes):
    w = torch.zeros(plan.param_floats, dtype=torch.bool)
    for (off, n, _), k in zip(plan.param_info, sd):
        if k.startswith(prefixes):
            w[off:off + n] = True
    return w
