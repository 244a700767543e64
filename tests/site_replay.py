"""Layer-by-layer replay of a training plan's forward against its own workspace (TEST INFRASTRUCTURE ONLY; the judge is
tests/test_bf16_layer_replay.py, the hook is oracle.avc_oracle.forced_sites).

A training plan keeps every layer's stored output in the workspace (``Plan.site``: the site table in the reference's call order, plus
the named residual outputs and fp32 results).  ``replay`` recomputes each layer in torch FROM THE ENGINE'S OWN STORED INPUT to that
layer, so that what is compared is one layer's arithmetic and not 13 layers of compounding rounding noise.  The same replay runs in
float64 (the reference value r64) and in float32 (the twin whose distance from r64 is the only source of the margins)."""
import contextlib

import torch

from adaptive_voice_conversion_amd.engine import unpack_pairs
from oracle import avc_oracle as O

NAMED = ("spk_out0", "spk_outN", "enc_out0", "enc_outN", "dec_out0", "dec_outN")


def read_site(plan, ws, i):
    """site i as CPU fp32 tensors (``Plan.site``, copied off the workspace)"""
    return {k: (v.detach().cpu().clone() if torch.is_tensor(v) else v) for k, v in plan.site(ws, i).items()}


def read_act(plan, ws, name, B, C, T):
    """a named [B, C, T] activation of the plan: a bf16 pair tensor at the offset an fp32 tensor would have in an fp32 plan"""
    off = plan.buffer(name)
    if plan.pair_storage:
        return unpack_pairs(ws.view(torch.int32)[off:off + B * (C // 2) * T].view(B, C // 2, T)).cpu()
    return ws[off:off + B * C * T].view(B, C, T).cpu().clone()


def read_workspace(plan, ws, cfg):
    """everything the replay takes from the workspace, on the CPU: the sites, the named residual outputs, the fp32 results"""
    B, Tb, To = plan.B, plan.latent_len, plan.out_len
    s, e, d = cfg["SpeakerEncoder"], cfg["ContentEncoder"], cfg["Decoder"]
    Ts = plan.T_cond
    for sub in s["subsample"][:s["n_conv_blocks"]]:
        Ts = -(-Ts // sub)
    sites = [read_site(plan, ws, i) for i in range(plan.num_sites())]
    named = {"spk_out0": read_act(plan, ws, "spk_out0", B, s["c_h"], plan.T_cond), "spk_outN": read_act(plan, ws, "spk_outN", B, s["c_h"], Ts), "enc_out0": read_act(plan, ws, "enc_out0", B, e["c_h"], plan.T),
             "enc_outN": read_act(plan, ws, "enc_outN", B, e["c_h"], Tb), "dec_out0": read_act(plan, ws, "dec_out0", B, d["c_h"], Tb),
             "dec_outN": read_act(plan, ws, "dec_outN", B, d["c_h"], To)}
    res = {"emb": plan.view(ws, "emb", (B, s["c_out"])).cpu().clone(), "muls": plan.view(ws, "muls", (B, 2 * e["c_out"], Tb)).cpu().clone(),
           "dec": plan.view(ws, "dec", (B, d["c_out"], To)).cpu().clone(), "z": read_act(plan, ws, "z", B, d["c_in"], Tb)}
    return sites, named, res


def replay(cfg, sd, x, eps, sites, named, res, dtype, bf16, pre_log=None, window=None):
    """One forced forward in ``dtype``.  bf16: the plan is a bf16 storage plan (conv / Linear operands rounded as O.bf16_operands does,
    stored activations rounded where the engine rounds them); else an fp32 plan (no rounding anywhere).  Returns the report: one record
    per compared tensor, in forward order, {"label", "what", "storage", "clean", "value", "engine", "allow"} with ``value`` in ``dtype``.
    pre_log / window: see forced_sites (the pre-rounding values of the tensors the replay recomputes; how far the engine's may lie)."""
    report = []
    sd_ = {k: v.to(dtype) for k, v in sd.items()}
    x_ = x.to(dtype)
    Cz = cfg["ContentEncoder"]["c_out"]
    with (O.bf16_operands() if bf16 else contextlib.nullcontext()), O.forced_sites(sites, report, named, bf16_storage=bf16, pre_log=pre_log, window=window) as f:
        emb = f.substitute("emb", "head", 0, O.speaker_encoder(x_, sd_, cfg), res["emb"])
        mu, ls = O.content_encoder(x_, sd_, cfg)
        muls = f.substitute("muls", "head", 0, torch.cat((mu, ls), dim=1), res["muls"])
        z = muls[:, :Cz] + torch.exp(muls[:, Cz:] / 2) * eps.to(dtype)      # model.py:383-384, from the ENGINE's mu | log_sigma
        z = f.substitute("z", "out", 1 if bf16 else 0, z, res["z"])
        f.substitute("dec", "head", 0, O.decoder(z, emb, sd_, cfg), res["dec"])
    return report


def bf16_ulp(r):
    """one bf16 ulp at r (8 significand bits): 2 ** (floor(log2 |r|) - 7); 0 at r == 0"""
    m, e = torch.frexp(r.abs())                     # |r| = m 2^e, m in [0.5, 1)
    return torch.where(r == 0, torch.zeros_like(r), torch.ldexp(torch.ones_like(r), e - 8))


def to_bf16(r):
    return r.to(torch.bfloat16).to(r.dtype)
