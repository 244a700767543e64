"""Gradients through the ragged decoder: ``AE.decoder_ragged(zs, emb)`` is differentiable with respect to the latents and the embeddings -- a
"decode_ig" RaggedPlan (avc_plan_create_ragged_decoder_grads), ``avc_decoder_backward_ragged``: the decoder's backward pass over latents of
different lengths in ONE ragged launch set, fp32, parameters frozen.  The one new kernel is the AdaIN instance of the ragged InstanceNorm
backward row kernel (rag_instnorm_bwd_kernel<true>: gamma / beta, d(cond), the planar store behind a pixel shuffle).

kind='emu': the CPU lane-level simulation of the same kernels on the tiny config; kind='gpu': the gfx950 library on the stock 80-mel
config.  Latent lengths: those of the source lengths of tests/test_ragged_enroll._setup (GPU: 3, 8, 9, 75, 42, 4, 3, 25, 4, 12, 16, 51 --
three-frame rows with both reflect windows, a 64-frame output = one column tile, 72 frames = eight into the second tile, 600-frame rows of
many 64-lane strides).  No latent is filtered out of any check.

Reference: the fp64 oracle ``O.decoder`` under ``O.relu_masks`` on the branch the engine took, read from the plan's saved buffers and
statistics (nothing is recomputed): stage 0 ``saved y0 > saved mean``; AdaIN stages ``h.double() * gamma.double() + beta.double() > 0``
with ``h = (y - mean) * rstd`` in fp32 (the kernel's __fsub_rn / __fmul_rn; the fp64 expression has the sign of the kernel's
single-rounded fma).  d(cond) of the reference is autograd of the same fp64 pass with respect to the affine outputs.  Never the uniform
B = 1 engine: it computes its statistics in other kernels and may decide a near-zero pre-activation the other way.
Bars (the project's): d_z per latent rel-L2 <= 1e-4; latents of Tz <= 3, every row of d_emb, and every d(cond) stage (d_emb is a linear
map of them: the same rule) max(1e-4, 2 x err(fp32 oracle, fp64 oracle)) computed here on the same branch."""
import copy
import ctypes
import functools
import warnings

import pytest
import torch

from adaptive_voice_conversion_amd import _lib as L
from adaptive_voice_conversion_amd.engine import RaggedPlan
from oracle import avc_oracle as O
from tests.emu_util import KINDS, backend
from tests.ragged_oracle import content_masks, decoder_levels as _levels, decoder_masks as _dec_masks, decoder_oracle as _oracle, speaker_masks
from tests.redzone import guarded_input
from tests.test_engine import flat_params
from tests.test_ragged_enroll import _model, _nan_ws, _setup, _utts
from tests.test_submodules import rel

BAR = 1e-4
SHORT = 3   # latents of at most this many frames: InstanceNorm over three frames is ill-conditioned


def _cfg(kind, act="relu"):
    lib, dev, cfg, _, T, Tc = _setup(kind)
    cfg = copy.deepcopy(cfg)
    for net in ("SpeakerEncoder", "ContentEncoder", "Decoder"):
        cfg[net]["act"] = act
    sub = cfg["ContentEncoder"]["subsample"][:cfg["ContentEncoder"]["n_conv_blocks"]]
    Tz = list(T)
    for s in sub:
        Tz = [-(-t // s) for t in Tz]
    return lib, dev, cfg, O.make_state_dict(cfg, 3), Tz


def _inputs(cfg, Tz, seed):
    g = torch.Generator().manual_seed(seed)
    d = cfg["Decoder"]
    zs = [torch.randn(d["c_in"], t, generator=g) for t in Tz]
    emb = torch.randn(len(Tz), d["c_cond"], generator=g)
    return zs, emb


def _d_dec(plan, seed):
    return torch.randn(plan.n_mels * sum(plan.out_len), generator=torch.Generator().manual_seed(seed))


def _out_blocks(d, plan):
    M, base = plan.n_mels, plan.out_off[0]
    return [d[o - base:o - base + M * n].view(1, M, n) for o, n in zip(plan.out_off, plan.out_len)]


def _pass(kind, act="relu"):
    return _pass_once(kind, act)


@functools.lru_cache(maxsize=None)
def _pass_once(kind, act):
    """forward + backward of a "decode_ig" plan in a NaN-filled workspace, inputs inside NaN guards; shared by the tests, never modified"""
    lib, dev, cfg, sd, Tz = _cfg(kind, act)
    zs, emb = _inputs(cfg, Tz, 9)
    plan = RaggedPlan(cfg, Tz, None, lib=lib, mode="decode_ig")
    params = flat_params(plan, sd, dev)
    ws = _nan_ws(plan, dev)
    z = guarded_input(torch.cat([t.reshape(-1) for t in zs]), device=dev)
    e = guarded_input(emb, device=dev)
    d = _d_dec(plan, 31)
    dg = guarded_input(d, device=dev)
    assert z.is_contiguous() and dg.is_contiguous()
    plan.forward_latents(params, z, plan.c_lat, e, ws)
    plan.backward_decoder(params, z, plan.c_lat, e, dg, ws)
    return plan, ws, params, zs, emb, d, dev, cfg, sd


def _reference(kind, act="relu"):
    return _reference_once(kind, act)


@functools.lru_cache(maxsize=None)
def _reference_once(kind, act):
    """per latent: (d_z, d_emb, d_cond) of the fp64 oracle on the engine's branch and the same of the fp32 oracle; computed once"""
    plan, ws, _, zs, emb, d, _, cfg, sd = _pass(kind, act)
    masks = _dec_masks(plan, ws, cfg)
    out = []
    for b, w in enumerate(_out_blocks(d, plan)):
        out.append((_oracle(zs[b], emb[b], w, sd, cfg, masks[b], torch.float64), _oracle(zs[b], emb[b], w, sd, cfg, masks[b], torch.float32)))
    return out


def _bar(got32, ref):
    return max(BAR, 2 * rel(got32, ref))


@pytest.mark.parametrize("kind", KINDS)
def test_gradient_parity_with_the_fp64_oracle(kind):
    """1. C ABI: d_z per latent and d_emb per row against the fp64 oracle; NaN-filled workspace, guarded inputs; exact extents.
    Measured worst rel-L2: simulator (tiny config) d_z 4.3e-07, d_emb 7.7e-07; MI355X (stock config) d_z 1.08e-05 at Tz = 3 and 1.8e-06 at
    Tz >= 4, d_emb 3.8e-06 (every bar 1e-4: the fp32 oracle's own error is below 5e-5 everywhere)."""
    plan, ws, _, zs, emb, _, _, cfg, _ = _pass(kind)
    assert plan.lib.avc_plan_flags(plan.h) & L.PLAN_INPUT_GRADS and not plan.lib.avc_plan_flags(plan.h) & L.PLAN_FANOUT
    dz, de = [t.cpu() for t in plan.d_z(ws)], plan.d_emb(ws).cpu()
    assert de.shape == emb.shape and torch.isfinite(de).all()
    for t in plan.outputs(ws):
        assert torch.isfinite(t).all()
    for name, n in (("d_z", plan.c_lat * sum(plan.T)), ("d_emb", plan.N * plan.c_emb)):   # exact extents: the allocation's padding stays NaN
        o = plan.buffer(name)
        assert torch.isfinite(ws[o:o + n]).all()
        assert torch.isnan(ws[o + n:o + (n + 63) // 64 * 64]).all(), name
    for b, ((rz, re, _), (fz, fe, _)) in enumerate(_reference(kind)):
        assert dz[b].shape == zs[b].shape and torch.isfinite(dz[b]).all()
        bz = _bar(fz, rz) if plan.T[b] <= SHORT else BAR
        be = _bar(fe, re)
        ez, ee = rel(dz[b], rz), rel(de[b], re)
        print(f"latent {b} Tz={plan.T[b]}: d_z rel-L2 {ez:.3e} bar {bz:.3e}; d_emb rel-L2 {ee:.3e} bar {be:.3e}")
        assert ez <= bz and ee <= be, (b, plan.T[b], ez, bz, ee, be)


@pytest.mark.parametrize("act", ["relu", "lrelu"])
@pytest.mark.parametrize("kind", KINDS)
def test_row_kernel_adain(kind, act):
    """2. The d(cond) the plan leaves, per stage and latent, against autograd of the fp64 pass with respect to the affine outputs; ReLU and
    LeakyReLU.  Every element is written (the workspace started as NaN).  Measured worst rel-L2 on the MI355X: 4.9e-06 (relu and lrelu)."""
    plan, ws, _, _, _, _, _, cfg, _ = _pass(kind, act)
    d = cfg["Decoder"]
    C, n = d["c_h"], d["n_conv_blocks"]
    o = plan.buffer("d_cond")
    dc = ws[o:o + plan.N * 2 * n * 2 * C].view(plan.N, 2 * n, 2 * C).cpu()
    assert torch.isfinite(dc).all()
    for b, ((_, _, rc), (_, _, fc)) in enumerate(_reference(kind, act)):
        for k in range(2 * n):
            bar = _bar(fc[k], rc[k])
            e = rel(dc[b, k], rc[k])
            print(f"latent {b} Tz={plan.T[b]} stage {k} ({act}): d_cond rel-L2 {e:.3e} bar {bar:.3e}")
            assert e <= bar, (b, plan.T[b], k, e, bar)


def _decode_plan_floats(cfg, Tz):
    """avc_plan_workspace_floats of an unflagged "decode" plan with the identity map and default tuning, from its layout as it was before
    the backward pass existed (every allocation rounded up to 64 floats): forward weight images [chunk][tap][CK][Mp] (Mp = rows rounded up to
    128; CK = 32 / 16 / 8 channels per chunk for 1 / 2-3 / >= 4 taps), the stacked bias of the affine layers (32 x Mp), cond, y0, out_0, per
    block y1, a1, y2, out, dec, and the tables (source level: T, off, tiles; the map: T, off; the n + 1 output levels: T, off, tiles)."""
    d = cfg["Decoder"]
    N, C, n, k = len(Tz), d["c_h"], d["n_conv_blocks"], d["kernel_size"]
    r64 = lambda v: (v + 63) // 64 * 64   # noqa: E731
    mp = lambda v: (v + 127) // 128 * 128   # noqa: E731
    ck = lambda t: 8 if t >= 4 else (16 if t >= 2 else 32)   # noqa: E731
    img = lambda co, ci, t: r64(-(-ci // ck(t)) * t * ck(t) * mp(co))   # noqa: E731
    f = img(C, d["c_in"], 1)
    f += sum(img(C, C, k) for _ in range(n)) + sum(img(C * u, C, k) for u in d["upsample"][:n])
    f += img(2 * n * 2 * C, d["c_cond"], 1) + r64(32 * mp(2 * n * 2 * C))
    f += img(d["c_out"], C, 1)
    S = [sum(lv) for lv in _levels(cfg, Tz)]
    f += r64(N * 2 * n * 2 * C) + 2 * r64(C * S[0])
    for l in range(n):
        f += 2 * r64(C * S[l]) + 2 * r64(C * S[l + 1])
    f += r64(d["c_out"] * S[-1])
    r4 = lambda v: (v + 3) // 4 * 4   # noqa: E731
    tab = lambda lv: r4(N) + r4(N + 1) + r4(2 * sum(-(-t // 64) for t in lv))   # noqa: E731
    lv = _levels(cfg, Tz)
    f += r64(tab(lv[0]) + 2 * r4(N) + sum(tab(x) for x in lv))
    return f


@pytest.mark.parametrize("kind", KINDS)
def test_determinism_and_unchanged_forward(kind):
    """3. Two backward passes from one forward give identical bits; the flagged plan's forward equals the unflagged "decode" plan's, bit
    for bit; the unflagged plan's workspace is what it was."""
    plan, ws, params, zs, emb, d, dev, cfg, _ = _pass(kind)
    z, e, dd = torch.cat([t.reshape(-1) for t in zs]).to(dev), emb.to(dev), d.to(dev)
    first_z, first_e = [t.clone() for t in plan.d_z(ws)], plan.d_emb(ws).clone()
    ws2 = _nan_ws(plan, dev)
    plan.forward_latents(params, z, plan.c_lat, e, ws2)
    for _ in range(2):
        plan.backward_decoder(params, z, plan.c_lat, e, dd, ws2)
        assert torch.equal(plan.d_emb(ws2), first_e)
        assert all(torch.equal(a, b) for a, b in zip(plan.d_z(ws2), first_z))
    plain = RaggedPlan(cfg, plan.T, None, lib=plan.lib, mode="decode")
    assert plain.workspace_floats == _decode_plan_floats(cfg, plan.T)
    assert plan.workspace_floats > plain.workspace_floats
    assert plain.out_len == plan.out_len
    w0 = _nan_ws(plain, dev)
    plain.forward_latents(params, z, plain.c_lat, e, w0)
    for a, b in zip(plain.outputs(w0), plan.outputs(ws)):
        assert torch.isfinite(a).all() and torch.equal(a, b)
    with pytest.raises(KeyError):
        plain.buffer("d_z")


@pytest.mark.parametrize("kind", KINDS)
def test_module(kind):
    """4. AE.decoder_ragged: grads of their own shape on every leaf, none on a non-leaf, a single voice gets the sum of the rows, two
    pending forwards of the same lengths, no-grad == decode_ragged, bf16 raises, decode_ragged still refuses."""
    plan, ws, _, zs, emb, d, dev, cfg, sd = _pass(kind)
    lib = backend(kind)[0]
    model = _model(kind, lib, dev, cfg, sd)
    wts = [w[0].to(dev) for w in _out_blocks(d, plan)]
    loss = lambda outs: sum((o * w).sum() for o, w in zip(outs, wts))   # noqa: E731
    leaves = [t.to(dev, copy=True).requires_grad_(True) for t in zs]
    mid = leaves[1] * 1.0   # a non-leaf latent with the same values
    e = emb.to(dev, copy=True).requires_grad_(True)
    outs = model.decoder_ragged([mid if b == 1 else t for b, t in enumerate(leaves)], e)
    assert all(o.requires_grad and o.shape == (plan.n_mels, n) for o, n in zip(outs, plan.out_len))
    # a second grad forward of the same lengths (one voice for all) before the first backward: a private workspace
    zs2, emb2 = _inputs(cfg, plan.T, 77)
    leaves2 = [t.to(dev, copy=True).requires_grad_(True) for t in zs2]
    one = emb2[0].to(dev, copy=True).requires_grad_(True)
    outs2 = model.decoder_ragged(leaves2, one)
    loss(outs).backward()
    loss(outs2).backward()
    dz, de = plan.d_z(ws), plan.d_emb(ws)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")   # (reading .grad of a non-leaf warns)
        assert not mid.is_leaf and mid.grad is None
    for b, t in enumerate(leaves):
        assert t.grad.shape == zs[b].shape and torch.equal(t.grad, dz[b]), b
    assert e.grad.shape == emb.shape and torch.equal(e.grad, de)
    for a, b in zip(outs, plan.outputs(ws)):
        assert torch.equal(a.detach(), b)
    # the second call against a plan-level pass of its own: one voice = the sum of the N rows
    ws2 = _nan_ws(plan, dev)
    z2, e2 = torch.cat([t.reshape(-1) for t in zs2]).to(dev), emb2[:1].to(dev).expand(plan.N, -1)
    plan.forward_latents(flat_params(plan, sd, dev), z2, plan.c_lat, e2, ws2)
    plan.backward_decoder(flat_params(plan, sd, dev), z2, plan.c_lat, e2, d.to(dev), ws2)
    assert one.grad.shape == one.shape
    torch.testing.assert_close(one.grad, plan.d_emb(ws2).sum(0), rtol=1e-5, atol=1e-6 * float(plan.d_emb(ws2).abs().max()) * plan.N)
    assert all(torch.equal(t.grad, g) for t, g in zip(leaves2, plan.d_z(ws2)))
    # without grad: decode_ragged, bit for bit
    with torch.no_grad():
        a = model.decoder_ragged(leaves, e)
    b = model.decode_ragged([t.detach() for t in leaves], e.detach())
    assert all(torch.equal(x, y) and not x.requires_grad for x, y in zip(a, b))
    assert all(torch.equal(x, y) for x, y in zip(b, plan.outputs(ws)))
    with pytest.raises(RuntimeError, match=r"forward-only.*decoder\(z, cond\)"):
        model.decode_ragged(leaves, e.detach())
    with pytest.raises(RuntimeError, match="forward-only"):
        model.inference_ragged(_utts([20, 30], plan.n_mels, 1), emb=torch.zeros(2, plan.c_emb, device=dev, requires_grad=True))
    bf = _model(kind, lib, dev, cfg, sd, "bf16")
    with pytest.raises(RuntimeError, match=r"decoder\(z_b, emb_b\)"):
        bf.decoder_ragged(leaves, e)
    with torch.no_grad():
        bf.decoder_ragged(leaves, e)
    assert bf.last_ragged_compute == "bf16r"


@pytest.mark.parametrize("kind", KINDS)
def test_composition(kind):
    """5. Two utterances through all three ragged grad paths: x.grad and x_cond.grad against the fp64 O.ae_inference on the three plans' own
    branches (bars: 1e-4; the utterance whose latent has <= 3 frames and the speaker side -- it flows through d_emb -- take
    max(1e-4, 2 x err(fp32, fp64))).  Measured on the MI355X: x.grad 1.07e-04 for the 17-frame source (latent of 3 frames; bar 1.68e-04) and
    4.4e-06 for the 90-frame one, x_cond.grad 3.3e-05 / 5.1e-06; simulator: all below 1e-06."""
    lib, dev, cfg, sd, _ = _cfg(kind)
    M = cfg["ContentEncoder"]["c_in"]
    T, Tc = (17, 90), (64, 29)
    xs, cs = _utts(T, M, 5), _utts(Tc, M, 6)
    model = _model(kind, lib, dev, cfg, sd)
    x = [t.to(dev, copy=True).requires_grad_(True) for t in xs]
    c = [t.to(dev, copy=True).requires_grad_(True) for t in cs]
    outs = model.decoder_ragged(model.content_encoder_ragged(x)[0], model.get_speaker_embeddings_ragged(c))
    g = torch.Generator().manual_seed(8)
    wts = [torch.randn(o.shape, generator=g) for o in outs]
    pe, ee = model._ragged_plan("encode_ig", T, ())
    ps, es = model._ragged_plan("speaker_ig", (), Tc)
    pd, ed = model._ragged_plan("decode_ig", tuple(pe.lat_len), ())
    masks = [s + e + d for s, e, d in zip(speaker_masks(ps, es.ws), content_masks(pe, ee.ws, cfg), _dec_masks(pd, ed.ws, cfg))]
    sum((o * w.to(dev)).sum() for o, w in zip(outs, wts)).backward()

    def ref(b, dtype):
        a = xs[b].t()[None].to(dtype).clone().requires_grad_(True)
        k = cs[b].t()[None].to(dtype).clone().requires_grad_(True)
        with O.relu_masks(masks[b]):
            (O.ae_inference(a, k, {n: v.to(dtype) for n, v in sd.items()}, cfg) * wts[b][None].to(dtype)).sum().backward()
        return a.grad[0].t().float(), k.grad[0].t().float()

    for b in range(2):
        (rx, rc), (fx, fc) = ref(b, torch.float64), ref(b, torch.float32)
        bx = _bar(fx, rx) if pe.lat_len[b] <= SHORT else BAR
        bc = _bar(fc, rc)
        ex, ec = rel(x[b].grad, rx), rel(c[b].grad, rc)
        print(f"utterance {b} T={T[b]} T_cond={Tc[b]}: x.grad rel-L2 {ex:.3e} bar {bx:.3e}; x_cond.grad rel-L2 {ec:.3e} bar {bc:.3e}")
        assert x[b].grad.shape == xs[b].shape and c[b].grad.shape == cs[b].shape
        assert ex <= bx and ec <= bc, (b, ex, bx, ec, bc)


@pytest.mark.parametrize("kind", KINDS)
def test_refusals(kind):
    """6. The C boundary: an unflagged plan, a fan-out plan and a bf16 compute mode are refused with -8 and a message naming the creator."""
    plan, ws, params, zs, emb, d, dev, cfg, _ = _pass(kind)
    lib = plan.lib
    z, e, dd = torch.cat([t.reshape(-1) for t in zs]).to(dev), emb.to(dev), d.to(dev)
    P = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731

    def call(p, w):
        return lib.avc_decoder_backward_ragged(p.h, P(params), P(z), p.c_lat, P(e), e.stride(0), e.stride(1), P(dd), P(w), None)

    big = torch.zeros(plan.workspace_floats, device=dev)
    plain = RaggedPlan(cfg, plan.T, None, lib=lib, mode="decode")
    assert call(plain, big) == -8
    assert "not created by avc_plan_create_ragged_decoder_grads" in lib.avc_last_error().decode()
    with pytest.raises(RuntimeError, match="decode_ig"):
        plain.backward_decoder(params, z, plain.c_lat, e, dd, big)
    T = _setup(kind)[4]
    fan = RaggedPlan(cfg, T, None, lib=lib, mode="encode", input_grads=True)   # AVC_PLAN_FANOUT | AVC_PLAN_INPUT_GRADS
    assert lib.avc_plan_flags(fan.h) & L.PLAN_FANOUT
    assert call(fan, torch.zeros(fan.workspace_floats, device=dev)) == -8
    msg = lib.avc_last_error().decode()
    assert "fan-out" in msg and "avc_plan_create_ragged_decoder_grads" in msg
    bf = RaggedPlan(cfg, plan.T, None, lib=lib, mode="decode_ig", compute_dtype="bf16")
    bf.forward_latents(params, z, bf.c_lat, e, big)
    assert call(bf, big) == -8
    msg = lib.avc_last_error().decode()
    assert "bf16" in msg and "avc_plan_create_ragged_decoder_grads" in msg
    assert lib.avc_decoder_backward_ragged(plan.h, P(params), P(z), plan.c_lat, P(e), e.stride(0), e.stride(1), None, P(big), None) == -1
    assert "null argument" in lib.avc_last_error().decode()
    assert torch.isfinite(plan.d_emb(ws)).all()   # (the shared pass is untouched)
