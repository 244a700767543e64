"""Gradients with respect to the input spectrograms (AVC_PLAN_INPUT_GRADS): ``x.requires_grad_()`` followed by a backward gives the
reference's ``x.grad`` through ``AE.forward``, ``AE.inference(x, x_cond)``, ``speaker_encoder``, ``content_encoder`` and
``get_speaker_embeddings``.

kind='emu': CPU lane-level simulation of the same kernels on tiny instances; kind='gpu': the gfx950 library on the stock m80 config.
The oracle runs in fp64 on the engine's own ReLU branch (tests/test_engine.py::branch_matched_oracle) with random upstream weights on
every output; fp32 bar: rel-L2 <= 1e-4 per tensor."""
import ctypes

import pytest
import torch

from adaptive_voice_conversion_amd import _lib
from adaptive_voice_conversion_amd.engine import cfg_from_dict
from oracle import avc_oracle as O
from tests.emu_util import backend
from tests.test_engine import get_cfg, zero_grad_bias
from tests.test_submodules import make_ae, rel

GPU = pytest.mark.gpu


def even_bank_config():
    """bank_size 8, bank_scale 2 (widths 2, 4, 6, 8: every pad asymmetric) and an even kernel_size in both encoders."""
    cfg = O.tiny_config(bank_size=8)
    for k in ("SpeakerEncoder", "ContentEncoder"):
        cfg[k]["bank_scale"] = 2
        cfg[k]["kernel_size"] = 4
    return cfg


def config(name):
    return even_bank_config() if name == "even_bank" else get_cfg(name)


def masks_of(ae, mode, B, T, Tc, dev, rows=None):
    e = ae._entry(mode, B, T, Tc, dev)
    ms = [m.cpu() for m in e.plan.relu_masks(e.ws)]
    return ms if rows is None else [m[rows] for m in ms]


def leaf(t, dev, transposed=False):
    """a leaf that requires grad, on `dev`; transposed: the CollateFn view [B, M, T] with strides (T*M, 1, M) of a [B, T, M] leaf"""
    if transposed:
        base = t.transpose(1, 2).contiguous().to(dev).requires_grad_(True)
        return base, base.transpose(1, 2)
    base = t.to(dev, copy=True).requires_grad_(True)
    return base, base


def grad_of(base, transposed):
    g = base.grad.detach().cpu()
    return g.transpose(1, 2) if transposed else g


def weigh(outs, ws):
    return sum((o * w.to(o.device, o.dtype)).sum() for o, w in zip(outs, ws))


def upstream(outs, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(o.shape, generator=g) for o in outs]


def oracle_input_grads(fn, inputs, sd, masks, ws, dtype=torch.float64):
    """d(sum_i w_i . out_i)/d(inputs) of the oracle function fn(*inputs, sd) in `dtype`, on the given ReLU branch"""
    xs = [t.to(dtype).clone().requires_grad_(True) for t in inputs]
    sdd = {k: v.to(dtype) for k, v in sd.items()}
    with O.relu_masks(masks):
        outs = fn(*xs, sdd)
        outs = outs if isinstance(outs, tuple) else (outs,)
        weigh(outs, ws).backward()
    return [t.grad.float() for t in xs]


def check_param_grads(ae, sd, cfg, fn, inputs, masks, ws, tol=1e-4):
    """every parameter's .grad against the oracle on the same branch (the input-gradient path keeps the parameters' gradients)"""
    leaves = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
    xs = [t.double() for t in inputs]
    with O.relu_masks(masks):
        outs = fn(*xs, leaves)
        outs = outs if isinstance(outs, tuple) else (outs,)
        weigh(outs, ws).backward()
    ref = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).float() for k, v in leaves.items()}
    scale = sum(g.norm() ** 2 for g in ref.values()) ** 0.5
    for k, p in ae.named_parameters():
        gref = ref[k]
        if p.grad is None:
            assert gref.norm() == 0, k
            continue
        if zero_grad_bias(k, cfg) or gref.norm() < 1e-6 * scale:   # (analytically zero here, e.g. the mu head's bias ahead of an IN)
            assert (p.grad.detach().cpu() - gref).norm() < 1e-5 * scale, k
            continue
        assert rel(p.grad, gref) <= tol, (k, rel(p.grad, gref))


def ae_fwd(eps, cfg):
    return lambda x, sd: O.ae_forward(x, eps.to(x.dtype), sd, cfg)


# ---- AE.forward ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,cfgname,B,T,transposed", [
    ("emu", "tiny", 2, 32, False), ("emu", "tiny_lrelu", 3, 40, True), ("emu", "even_bank", 2, 32, False),
    ("emu", "even_bank", 2, 5, False),   # T = bank_size // 2 + 1: the reflect-pad limit of the widest bank conv
    pytest.param("gpu", "m80", 4, 128, True, marks=GPU)])
def test_ae_forward_input_grad(kind, cfgname, B, T, transposed):
    cfg = config(cfgname)
    if T < 8:   # (the encoders' own k = 4 convs need their rows longer than 2 frames: one block, no subsampling)
        for k in ("SpeakerEncoder", "ContentEncoder"):
            cfg[k]["n_conv_blocks"], cfg[k]["subsample"] = 1, [1]
        cfg["Decoder"]["n_conv_blocks"], cfg["Decoder"]["upsample"], cfg["Decoder"]["kernel_size"] = 1, [1], 3
    ae, sd, dev = make_ae(kind, cfg, 21)
    x, eps = O.make_inputs(cfg, B, T, 21)
    base, xd = leaf(x, dev, transposed)
    outs = ae(xd, eps.to(dev))
    ws = upstream(outs, 21)
    weigh(outs, ws).backward()
    masks = masks_of(ae, "ig_train", B, T, T, dev)
    gx, = oracle_input_grads(ae_fwd(eps, cfg), [x], sd, masks, ws)
    r = rel(grad_of(base, transposed), gx)
    assert r <= 1e-4, r
    check_param_grads(ae, sd, cfg, ae_fwd(eps, cfg), [x], masks, ws)


@GPU
def test_ae_forward_input_grad_at_bench_size():
    """B = 256, T = 128 (the bench shape).  x.grad of a sample depends on that sample alone: the oracle checks 6 of the 256, at
    max(1e-4, 2 x its own fp32-vs-fp64 error)."""
    cfg = O.stock_config(80)
    B, T = 256, 128
    ae, sd, dev = make_ae("gpu", cfg, 22)
    x, eps = O.make_inputs(cfg, B, T, 22)
    base, xd = leaf(x, dev)
    outs = ae(xd, eps.to(dev))
    ws = upstream(outs, 22)
    weigh(outs, ws).backward()
    rows = torch.tensor([0, 1, 77, 128, 200, 255])
    masks = masks_of(ae, "ig_train", B, T, T, dev, rows)
    ws_r = [w[rows] for w in ws]
    fn = ae_fwd(eps[rows], cfg)
    g64, = oracle_input_grads(fn, [x[rows]], sd, masks, ws_r)
    g32, = oracle_input_grads(fn, [x[rows]], sd, masks, ws_r, torch.float32)
    bar = max(1e-4, 2 * rel(g32, g64))
    r = rel(base.grad[rows.to(dev)], g64)
    assert r <= bar, (r, bar)


# ---- AE.inference(x, x_cond) --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,cfgname,T,Tc", [("emu", "tiny", 37, 19), ("emu", "even_bank", 33, 21),
                                               pytest.param("gpu", "m80", 100, 77, marks=GPU)])
def test_inference_input_grads(kind, cfgname, T, Tc):
    cfg = config(cfgname)
    B = 2
    ae, sd, dev = make_ae(kind, cfg, 23)
    x, _ = O.make_inputs(cfg, B, T, 23)
    xc, _ = O.make_inputs(cfg, B, Tc, 24)
    bx, xd = leaf(x, dev)
    bc, xcd = leaf(xc, dev, transposed=True)
    dec = ae.inference(xd, xcd)
    with torch.no_grad():
        ref_fwd = ae.inference(x.to(dev), xc.to(dev))
    assert dec.requires_grad
    torch.testing.assert_close(dec.detach(), ref_fwd, rtol=1e-4, atol=2e-5)
    ws = upstream([dec], 23)
    weigh([dec], ws).backward()
    masks = masks_of(ae, "ig_train", B, T, Tc, dev)
    fn = lambda a, c, s: O.ae_inference(a, c, s, cfg)   # noqa: E731
    gx, gc = oracle_input_grads(fn, [x, xc], sd, masks, ws)
    assert rel(bx.grad, gx) <= 1e-4 and rel(grad_of(bc, True), gc) <= 1e-4, (rel(bx.grad, gx), rel(grad_of(bc, True), gc))
    check_param_grads(ae, sd, cfg, fn, [x, xc], masks, ws)


@pytest.mark.parametrize("kind", ["emu", pytest.param("gpu", marks=GPU)])
def test_inference_of_x_with_itself(kind):
    """inference(x, x): both encoders read one leaf; its gradient is the sum of both terms"""
    cfg = get_cfg("tiny" if kind == "emu" else "m80")
    B, T = 2, 40
    ae, sd, dev = make_ae(kind, cfg, 25)
    x, _ = O.make_inputs(cfg, B, T, 25)
    bx, xd = leaf(x, dev)
    dec = ae.inference(xd, xd)
    ws = upstream([dec], 25)
    weigh([dec], ws).backward()
    masks = masks_of(ae, "ig_train", B, T, T, dev)
    gx, = oracle_input_grads(lambda a, s: O.ae_inference(a, a, s, cfg), [x], sd, masks, ws)
    assert rel(bx.grad, gx) <= 1e-4, rel(bx.grad, gx)


@pytest.mark.parametrize("detached", ["x_cond", "x"])
@pytest.mark.parametrize("kind", ["emu", pytest.param("gpu", marks=GPU)])
def test_inference_with_one_side_detached(kind, detached):
    """inference(x, x.detach()) / inference(x.detach(), x): the two arguments share memory but only one is the leaf; x.grad is the
    content path's term alone / the speaker path's term alone"""
    cfg = get_cfg("tiny" if kind == "emu" else "m80")
    B, T = 2, 40
    ae, sd, dev = make_ae(kind, cfg, 30)
    x, _ = O.make_inputs(cfg, B, T, 30)
    bx, xd = leaf(x, dev)
    dec = ae.inference(xd, xd.detach()) if detached == "x_cond" else ae.inference(xd.detach(), xd)
    ws = upstream([dec], 30)
    weigh([dec], ws).backward()
    masks = masks_of(ae, "ig_train", B, T, T, dev)
    gx, gc = oracle_input_grads(lambda a, c, s: O.ae_inference(a, c, s, cfg), [x, x], sd, masks, ws)
    ref = gx if detached == "x_cond" else gc
    assert bx.grad is not None
    assert rel(bx.grad, ref) <= 1e-4, rel(bx.grad, ref)


def test_inference_without_input_grad_stays_forward_only():
    cfg = get_cfg("tiny")
    ae, sd, dev = make_ae("emu", cfg, 26)
    x, _ = O.make_inputs(cfg, 2, 32, 26)
    dec = ae.inference(x, x)   # parameters require grad, the inputs do not
    assert not dec.requires_grad and dec.grad_fn is None
    assert not ae.get_speaker_embeddings(x).requires_grad


# ---- the encoders on their own, every parameter frozen --------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["speaker_encoder", "get_speaker_embeddings", "content_encoder"])
@pytest.mark.parametrize("kind,cfgname,B,T,transposed", [("emu", "tiny", 2, 32, False), ("emu", "even_bank", 3, 24, True),
                                                         pytest.param("gpu", "m80", 4, 128, True, marks=GPU)])
def test_encoder_input_grads_with_frozen_parameters(kind, cfgname, B, T, transposed, entry):
    cfg = config(cfgname)
    ae, sd, dev = make_ae(kind, cfg, 27)
    for p in ae.parameters():
        p.requires_grad_(False)
    x, _ = O.make_inputs(cfg, B, T, 27)
    base, xd = leaf(x, dev, transposed)
    outs = {"speaker_encoder": lambda: ae.speaker_encoder(xd), "get_speaker_embeddings": lambda: ae.get_speaker_embeddings(xd),
            "content_encoder": lambda: ae.content_encoder(xd)}[entry]()
    outs = outs if isinstance(outs, tuple) else (outs,)
    ws = upstream(outs, 27)
    weigh(outs, ws).backward()
    spk = entry != "content_encoder"
    masks = masks_of(ae, "speaker_ig_train" if spk else "content_ig_train", B, T, T, dev)
    fn = (lambda a, s: O.speaker_encoder(a, s, cfg)) if spk else (lambda a, s: O.content_encoder(a, s, cfg))
    gx, = oracle_input_grads(fn, [x], sd, masks, ws)
    r = rel(grad_of(base, transposed), gx)
    assert r <= 1e-4, r
    assert all(p.grad is None for p in ae.parameters())


# ---- the flag changes nothing else; determinism ---------------------------------------------------------------------------------------
def _step(ae, x, eps, ws, want_dx):
    for p in ae.parameters():
        p.grad = None
    xd = x.clone().requires_grad_(want_dx)
    outs = ae(xd, eps)
    weigh(outs, ws).backward()
    return [o.detach().clone() for o in outs], {k: p.grad.clone() for k, p in ae.named_parameters()}, (xd.grad.clone() if want_dx else None)


@pytest.mark.parametrize("kind,cfgname,B,T,compute", [("emu", "tiny", 2, 32, "fp32"), ("emu", "tiny", 2, 32, "bf16"),
                                                      pytest.param("gpu", "m80", 64, 128, "fp32", marks=GPU),
                                                      pytest.param("gpu", "m80", 64, 128, "bf16", marks=GPU)])
def test_flag_keeps_parameter_grads_and_dx_is_reproducible(kind, cfgname, B, T, compute):
    """With the flag the outputs and every parameter gradient are bit-equal to those of the same backward without it; two consecutive
    runs give bit-identical x.grad (multi-stream backward: the encoders on two streams, weight gradients on two more)."""
    cfg = get_cfg(cfgname)
    ae, sd, dev = make_ae(kind, cfg, 28, compute_dtype=compute)
    x, eps = O.make_inputs(cfg, B, T, 28)
    x, eps = x.to(dev), eps.to(dev)
    with torch.no_grad():
        ws = upstream(ae(x, eps), 28)
    o0, g0, _ = _step(ae, x, eps, ws, False)
    o1, g1, dx1 = _step(ae, x, eps, ws, True)
    o2, g2, dx2 = _step(ae, x, eps, ws, True)
    for a, b in zip(o0, o1):
        assert torch.equal(a, b)
    for k in g0:
        assert torch.equal(g0[k], g1[k]) and torch.equal(g1[k], g2[k]), k
    assert torch.isfinite(dx1).all() and torch.equal(dx1, dx2)


# ---- the other compute modes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,cfgname,B,T,compute", [("emu", "tiny", 2, 32, "bf16"), ("emu", "tiny", 2, 32, "fp32x3"),
                                                      pytest.param("gpu", "m80", 4, 128, "bf16", marks=GPU),
                                                      pytest.param("gpu", "m80", 4, 128, "fp32x3", marks=GPU)])
def test_input_grad_in_other_compute_modes(kind, cfgname, B, T, compute):
    """x.grad against the fp64 oracle on the engine's branch: fp32x3 at the fp32 bar; the bf16 storage engine at the worst-tensor bar of
    the BASELINE.md round-4 addendum (rel-L2 <= 1e-1; d(x) sits at the far end of the backward pass, beside the conv bank's gradients)
    and cosine >= 0.9995."""
    cfg = get_cfg(cfgname)
    ae, sd, dev = make_ae(kind, cfg, 29, compute_dtype=compute)
    x, eps = O.make_inputs(cfg, B, T, 29)
    base, xd = leaf(x, dev)
    outs = ae(xd, eps.to(dev))
    assert ae._entry("ig_train", B, T, T, dev).plan.compute_dtype == compute
    ws = upstream(outs, 29)
    weigh(outs, ws).backward()
    gx, = oracle_input_grads(ae_fwd(eps, cfg), [x], sd, masks_of(ae, "ig_train", B, T, T, dev), ws)
    g = base.grad.detach().cpu()
    r = rel(g, gx)
    if compute == "bf16":
        cos = torch.nn.functional.cosine_similarity(g.flatten().double(), gx.flatten().double(), dim=0).item()
        assert r <= 1e-1 and cos >= 0.9995, (r, cos)
    else:
        assert r <= 1e-4, r


# ---- C ABI --------------------------------------------------------------------------------------------------------------------------
def test_input_grads_plan_flags_and_buffers():
    lib, _ = backend("emu")
    cfg = cfg_from_dict(O.tiny_config())
    B, T, Tc = 2, 32, 24
    IG, S, C, D, G, INF = (_lib.PLAN_INPUT_GRADS, _lib.PLAN_SPEAKER_ONLY, _lib.PLAN_CONTENT_ONLY, _lib.PLAN_DECODER_ONLY,
                           _lib.PLAN_PART_GRADS, _lib.PLAN_INFERENCE)

    def create(flags, t=T, tc=Tc):
        h = ctypes.c_void_p()
        return lib.avc_plan_create_ex(ctypes.byref(cfg), B, t, tc, flags, ctypes.byref(h)), h

    for bad in (IG | INF, IG | S, IG | C, IG | D | G):   # no backward through an encoder
        assert create(bad)[0] == -1, bad
    plans = {}
    try:
        for name, fl in (("whole", 0), ("whole_ig", IG), ("spk_ig", S | G | IG), ("enc_ig", C | G | IG)):
            rc, h = create(fl)
            assert rc == 0, (name, lib.avc_last_error())
            plans[name] = h
        buf = {k: {n: lib.avc_plan_buffer(h, n.encode()) for n in ("d_x", "d_x_cond")} for k, h in plans.items()}
        assert buf["whole"] == {"d_x": -1, "d_x_cond": -1}
        assert buf["whole_ig"]["d_x"] >= 0 and buf["whole_ig"]["d_x_cond"] >= 0
        assert buf["spk_ig"]["d_x"] >= 0 and buf["spk_ig"]["d_x_cond"] < 0 and buf["enc_ig"]["d_x"] >= 0 and buf["enc_ig"]["d_x_cond"] < 0
        assert lib.avc_plan_workspace_floats(plans["whole_ig"]) > lib.avc_plan_workspace_floats(plans["whole"])
    finally:
        for h in plans.values():
            lib.avc_plan_destroy(h)
