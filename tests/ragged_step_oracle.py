"""fp64 / fp32 oracle of ``Solver.ae_step_ragged``: ``tests.ragged_param_oracle.step_oracle`` with the reparameterisation noise and the
loss weights of the training step.  Test infrastructure only."""
import torch

from oracle import avc_oracle as O
from tests.ragged_param_oracle import DEC, ENC, SPK, _grads, _leaves


def noisy_step_oracle(cfg, sd, xs, eps, masks, signs, lambda_rec, lambda_kl, dtype):
    """({name: d(loss)/d(parameter)} over ALL tensors, loss_rec, loss_kl) of one whole-utterance step in which every utterance xs[b]
    ([T_b, M]) is content source AND speaker reference (model.py:376-385 per utterance): emb = speaker(x_b), (mu, ls) = content(x_b),
    z = mu + exp(ls / 2) * eps_b, dec = decoder(z, emb); loss = lambda_rec * mean |dec[:, :T_b] - x_b| + lambda_kl * 0.5 * mean(exp(ls) +
    mu^2 - 1 - ls), both means over the PACKED elements of all utterances (solver.py:84-87 on packed rows).  eps[b]: [c_lat, Tz_b] or None
    (z = mu).  masks[b] = speaker + content + decoder masks of utterance b in call order; signs[b] = sign(dec - x) of the engine's output
    ([M, T_b]): the L1 term on the engine's branch."""
    leaves = _leaves(sd, dtype, (SPK, ENC, DEC))
    n_rec = sum(x.numel() for x in xs)
    rec, kl, n_kl = 0, 0, 0
    for x, e, m, s in zip(xs, eps, masks, signs):
        xb = x.t()[None].to(dtype)
        with O.relu_masks(m):
            emb = O.speaker_encoder(xb, leaves, cfg)
            mu, ls = O.content_encoder(xb, leaves, cfg)
            z = mu if e is None else mu + torch.exp(ls / 2) * e[None].to(dtype)
            dec = O.decoder(z, emb, leaves, cfg)
        T = x.shape[0]
        rec = rec + ((dec[0, :, :T] - x.t().to(dtype)) * s.to(dtype)).sum()
        kl = kl + (torch.exp(ls) + mu ** 2 - 1 - ls).sum()
        n_kl += mu.numel()
    loss_rec, loss_kl = rec / n_rec, 0.5 * kl / n_kl
    (lambda_rec * loss_rec + lambda_kl * loss_kl).backward()
    return _grads(leaves, (SPK, ENC, DEC)), float(loss_rec.detach()), float(loss_kl.detach())
