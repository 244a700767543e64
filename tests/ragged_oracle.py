"""What the ragged test files share to put the fp64 oracle on the engine's own branch: the readers of the activation decisions a ragged
plan took, from its saved tensors (``plan.buffer()``; nothing is recomputed), for ANY member of the architecture family -- levels from the
config's own subsample / upsample lists, ``bank_size // bank_scale`` bank members, any number of dense blocks (none included), ReLU and
LeakyReLU (a saved activation keeps the sign of its pre-activation under either) -- and the oracle gradients driven by them.

Test infrastructure only.  Masks come per utterance, in the oracle's forward call order (``O.relu_masks``)."""
import torch

from oracle import avc_oracle as O

SPK = "speaker_encoder."


def encoder_levels(c, T):
    """lengths per level of an encoder whose config (dict or avc_encoder_cfg) is ``c``: level l + 1 = ceil(level l / subsample[l])"""
    get = c.__getitem__ if isinstance(c, dict) else (lambda k: getattr(c, k))
    lv = [list(T)]
    for l in range(int(get("n_conv_blocks"))):
        s = int(get("subsample")[l])
        lv.append([-(-t // s) for t in lv[-1]])
    return lv


def content_levels(cfg, T):
    return encoder_levels(cfg["ContentEncoder"], T)


def decoder_levels(cfg, Tz):
    d = cfg["Decoder"]
    lv = [list(Tz)]
    for u in d["upsample"][:d["n_conv_blocks"]]:
        lv.append([t * u for t in lv[-1]])
    return lv


def _offsets(levels):
    return [[sum(lv[:b]) for b in range(len(lv))] for lv in levels]


def speaker_masks(plan, ws):
    """Speaker encoder (bank members, in_conv, per block conv1 / conv2, per dense block d1 / d2): ``saved activation > 0`` -- packed
    [channels][T_b] blocks per sample at channels * off[b], dense rows channel-major [C][B]."""
    c = plan.cfg.spk
    nb, Cb, Ch = c.bank_size // c.bank_scale, c.c_bank, c.c_h
    CC = nb * Cb + c.c_in
    levels = encoder_levels(c, plan.T_cond)
    offs = _offsets(levels)

    def rows(name, level, b, ch, c0=0, nc=None):   # channels [c0, c0 + nc) of sample b's block
        T = levels[level][b]
        o = plan.buffer(name) + ch * offs[level][b] + c0 * T
        return (ws[o:o + (nc or ch) * T].view(1, nc or ch, T) > 0).cpu()

    out = []
    for b in range(plan.B):
        m = [rows("spk_cat", 0, b, CC, g * Cb, Cb) for g in range(nb)]
        m.append(rows("spk_h0", 0, b, Ch))
        for l in range(c.n_conv_blocks):
            m.append(rows(f"spk_a1_{l}", l, b, Ch))
            m.append(rows(f"spk_a2_{l}", l + 1, b, Ch))
        for l in range(c.n_dense_blocks):
            for k in ("d1", "d2"):
                o = plan.buffer(f"spk_{k}_{l}")
                m.append((ws[o:o + Ch * plan.B].view(Ch, plan.B)[:, b] > 0).cpu()[None])
        out.append(m)
    return out


def content_masks(plan, ws, cfg):
    """Content encoder (bank members, in_conv-IN, per block IN1, IN2): ``cat > 0`` for the bank, ``saved y > saved row mean`` for every
    InstanceNorm stage (the engine's own sign test for gamma = 1, beta = 0).  Statistics mean[B * C] | rstd[B * C], row b * C + c."""
    c = plan.cfg.enc
    nb, Cb, Ch = c.bank_size // c.bank_scale, c.c_bank, c.c_h
    CC = nb * Cb + c.c_in
    levels = content_levels(cfg, plan.T)
    offs = _offsets(levels)

    def rows(name, level, b, ch, c0=0, nc=None):
        T = levels[level][b]
        o = plan.buffer(name) + ch * offs[level][b] + c0 * T
        return ws[o:o + (nc or ch) * T].view(1, nc or ch, T).cpu()

    def stage(y, st, level, b):
        o = plan.buffer(st) + b * Ch
        mean = ws[o:o + Ch].cpu()
        rstd = ws[o + plan.B * Ch:o + plan.B * Ch + Ch].cpu()
        assert torch.isfinite(mean).all() and torch.isfinite(rstd).all() and (rstd > 0).all()
        return rows(y, level, b, Ch) > mean[None, :, None]

    out = []
    for b in range(plan.B):
        m = [rows("enc_cat", 0, b, CC, g * Cb, Cb) > 0 for g in range(nb)]
        m.append(stage("enc_y0", "enc_st0", 0, b))
        for l in range(c.n_conv_blocks):
            m.append(stage(f"enc_y1_{l}", f"enc_st1_{l}", l, b))
            m.append(stage(f"enc_y2_{l}", f"enc_st2_{l}", l + 1, b))
        out.append(m)
    return out


def decoder_masks(plan, ws, cfg):
    """Decoder (in_conv-IN, per block AdaIN1, AdaIN2) from the saved pre-norm rows, statistics and ws["cond"]: stage 0 ``y0 > mean``; AdaIN
    stages ``h.double() * gamma.double() + beta.double() > 0`` with ``h = (y - mean) * rstd`` in fp32 (the fp64 expression has the sign of
    the kernel's single-rounded fma); the first-stage masks are cross-checked against saved a1 > 0."""
    d = cfg["Decoder"]
    C, n, N = d["c_h"], d["n_conv_blocks"], plan.B
    levels = decoder_levels(cfg, plan.T)
    offs = _offsets(levels)
    csb = 2 * n * 2 * C
    o = plan.buffer("cond")
    cond = ws[o:o + N * csb].view(N, csb).cpu()

    def rows(name, level, b):
        T = levels[level][b]
        o = plan.buffer(name) + C * offs[level][b]
        return ws[o:o + C * T].view(1, C, T).cpu()

    def stats(name, b):
        o = plan.buffer(name) + b * C
        mean, rstd = ws[o:o + C].cpu(), ws[o + N * C:o + N * C + C].cpu()
        assert torch.isfinite(mean).all() and torch.isfinite(rstd).all() and (rstd > 0).all()
        return mean[None, :, None], rstd[None, :, None]

    def ada(y, st, level, b, k):
        mean, rstd = stats(st, b)
        h = (rows(y, level, b) - mean) * rstd
        beta, gamma = cond[b, 2 * k * C:(2 * k + 1) * C], cond[b, (2 * k + 1) * C:(2 * k + 2) * C]
        return h.double() * gamma.double()[None, :, None] + beta.double()[None, :, None] > 0

    out = []
    for b in range(N):
        m = [rows("dec_y0", 0, b) > stats("dec_st0", b)[0]]
        for l in range(n):
            m1 = ada(f"dec_y1_{l}", f"dec_st1_{l}", l, b, 2 * l)
            assert torch.equal(m1, rows(f"dec_a1_{l}", l, b) > 0), (b, l)
            m.append(m1)
            m.append(ada(f"dec_y2_{l}", f"dec_st2_{l}", l + 1, b, 2 * l + 1))
        out.append(m)
    return out


def decoder_oracle(z, e, w, sd, cfg, masks, dtype):
    """(d_z [c_lat, Tz], d_emb [c_emb], d_cond [2n, 2C]) of sum(w . decoder(z, e)) in ``dtype`` on the given branch.  The affine outputs
    are made leaves by a zero weight and a bias that holds the affine output: the forward values are the same."""
    n = cfg["Decoder"]["n_conv_blocks"]
    sdd = {k: v.to(dtype) for k, v in sd.items()}
    z = z.to(dtype)[None].clone().requires_grad_(True)
    e = e.to(dtype)[None]
    conds = []
    for k in range(2 * n):
        W, b = sdd[f"decoder.conv_affine_layers.{k}.weight"], sdd[f"decoder.conv_affine_layers.{k}.bias"]
        c = (e @ W.t() + b)[0].clone().requires_grad_(True)
        conds.append((c, W))
        sdd[f"decoder.conv_affine_layers.{k}.weight"] = torch.zeros_like(W)
        sdd[f"decoder.conv_affine_layers.{k}.bias"] = c
    with O.relu_masks(masks):
        (O.decoder(z, e, sdd, cfg) * w.to(dtype)).sum().backward()
    d_cond = torch.stack([c.grad for c, _ in conds])
    d_emb = sum(c.grad @ W for c, W in conds)
    return z.grad[0].float(), d_emb.float(), d_cond.float()


def speaker_oracle(cfg, sd, cs, masks, d, dtype, inputs=False):
    """{name: d(sum_b <emb_b, d_b>)/d(parameter)} of O.speaker_encoder in ``dtype``, utterance b ([T_b, M]) on the branch masks[b];
    ``inputs``: also the list of d/d(utterance b), [T_b, M], from the same pass."""
    leaves = {k: v.to(dtype).clone().requires_grad_(k.startswith(SPK)) for k, v in sd.items()}
    xs = [c.t()[None].to(dtype).clone().requires_grad_(inputs) for c in cs]
    total = 0
    for b, x in enumerate(xs):
        with O.relu_masks(masks[b]):
            emb = O.speaker_encoder(x, leaves, cfg)
        total = total + (emb * d[b][None].to(dtype)).sum()
    total.backward()
    grads = {k: v.grad.double() for k, v in leaves.items() if k.startswith(SPK)}
    return (grads, [x.grad[0].t().float() for x in xs]) if inputs else grads
