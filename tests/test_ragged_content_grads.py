"""Input gradients through the ragged content encoder: ``AE.content_encoder_ragged(xs)`` is differentiable with respect to its inputs -- an
"encode" RaggedPlan with ``input_grads=True`` (avc_plan_create_ragged_content_grads), ``avc_content_backward_ragged``: the content
encoder's backward pass over utterances of different lengths in ONE ragged launch set, fp32, parameters frozen.  The one new kernel is the
ragged InstanceNorm backward row kernel (rag_instnorm_bwd_kernel).

kind='emu': the CPU lane-level simulation of the same kernels on the tiny config; kind='gpu': the gfx950 library on the stock 80-mel
config.  Source length sets: those of tests/test_ragged_enroll._setup (17: latent rows of 3 frames; 64 / 65: one column tile and one frame
into the second; odd lengths at every pooling level; 600: rows of many 64-lane strides).  No utterance is filtered out of any check.

Reference: the fp64 oracle gradient of ``O.content_encoder`` on the ReLU branch the engine took, read from the plan: bank ``cat > 0``, every
InstanceNorm stage ``saved y > saved row mean`` (the engine's own sign test for gamma = 1, beta = 0; no statistics are recomputed here).
Bars: utterances of >= 25 frames rel-L2 <= 1e-4 (the project's input-gradient bar); utterances of < 25 frames
max(1e-4, 2 x err(fp32 oracle, fp64 oracle)) computed here on the same branch (InstanceNorm over 3 frames is ill-conditioned: the
project's rule for ill-conditioned sums).  There is no gradient test against the uniform B = 1 engine: the two engines compute the
InstanceNorm statistics in different kernels and may take different ReLU branches at near-zero pre-activations."""
import ctypes
import functools

import pytest
import torch

from adaptive_voice_conversion_amd import _lib as L
from adaptive_voice_conversion_amd.engine import RaggedPlan, cfg_from_dict
from oracle import avc_oracle as O
from tests.emu_util import KINDS, backend
from tests.ragged_oracle import content_levels as _levels, content_masks as _relu_masks
from tests.redzone import GuardedOutput, guarded_input
from tests.test_engine import flat_params
from tests.test_input_grads import oracle_input_grads
from tests.test_ragged_enroll import _model, _nan_ws, _setup, _utts
from tests.test_submodules import rel

BAR = 1e-4
SHORT = 25   # sources of fewer frames reach 3-frame rows at the bottleneck


def _leaves(xs, dev):
    return [x.to(dev, copy=True).requires_grad_(True) for x in xs]


def _d_muls(plan, seed):
    """random upstream weights for mu and log_sigma in the layout of ws["muls"]: block s = [2 c_lat][Tz_s]"""
    return torch.randn(2 * plan.c_lat * sum(plan.lat_len), generator=torch.Generator().manual_seed(seed))


def _blocks(d, plan):
    """per source ([1, c_lat, Tz] weights of mu, of log_sigma) out of a packed d_muls"""
    c, base = plan.c_lat, plan.lat_off[0]
    out = []
    for o, n in zip(plan.lat_off, plan.lat_len):
        blk = d[o - base:o - base + 2 * c * n].view(2 * c, n)
        out.append((blk[:c][None].clone(), blk[c:][None].clone()))
    return out


def _split(g, lens):
    return list(torch.split(g.detach().cpu(), list(lens)))


@functools.lru_cache(maxsize=None)
def _pass(kind, seed=9, d_seed=31):
    """forward + backward of a flagged content plan in a NaN-filled workspace; shared by the tests and never modified
    -> (plan, ws, params, utterances, d_muls, device, cfg, sd)"""
    lib, dev, cfg, sd, T, _ = _setup(kind)
    M = cfg["ContentEncoder"]["c_in"]
    xs = _utts(T, M, seed)
    plan = RaggedPlan(cfg, T, None, lib=lib, mode="encode", input_grads=True)
    params = flat_params(plan, sd, dev)
    ws = _nan_ws(plan, dev)
    x = torch.cat(xs).to(dev)
    plan.forward(params, x, None, ws)
    d = _d_muls(plan, d_seed)
    plan.backward_content(params, x, d.to(dev), ws)
    return plan, ws, params, xs, d, dev, cfg, sd


@functools.lru_cache(maxsize=None)
def _reference(kind, mu_only):
    """Per utterance (fp64 oracle gradient [T_b, M], bar) on the engine's branch, computed once per kind and upstream weights."""
    plan, ws, _, xs, d, _, cfg, sd = _pass(kind)
    masks = _relu_masks(plan, ws, cfg)
    fn = lambda x, s: O.content_encoder(x, s, cfg)   # noqa: E731
    out = []
    for b, (x, (wm, wl)) in enumerate(zip(xs, _blocks(d, plan))):
        w = [wm, torch.zeros_like(wl) if mu_only else wl]
        ref, = oracle_input_grads(fn, [x.t()[None]], sd, masks[b], w)
        bar = BAR
        if plan.T[b] < SHORT:
            r32, = oracle_input_grads(fn, [x.t()[None]], sd, masks[b], w, dtype=torch.float32)
            bar = max(BAR, 2 * rel(r32, ref))
        out.append((ref[0].t(), bar))
    return out


def _module_pass(kind, model, xs, d, dev, mu_only=False, need=None):
    """loss = sum of the weighted latents through AE.content_encoder_ragged -> the leaves (None where an utterance is no leaf)"""
    ins = [x.to(dev, copy=True).requires_grad_(True) if (need is None or b in need) else x.to(dev) for b, x in enumerate(xs)]
    mu, ls = model.content_encoder_ragged(ins)
    plan = model._ragged_plan("encode_ig", tuple(int(x.shape[0]) for x in xs), ())[0]
    loss = 0
    for m, s, (wm, wl) in zip(mu, ls, _blocks(d, plan)):
        loss = loss + (m * wm[0].to(dev)).sum()
        if not mu_only:
            loss = loss + (s * wl[0].to(dev)).sum()
    loss.backward()
    return ins, mu, ls


@pytest.mark.parametrize("kind", KINDS)
def test_gradient_parity_with_the_fp64_oracle(kind):
    """1. Every utterance a leaf, random upstream weights on mu and log_sigma: each gradient against the fp64 oracle on the engine's own
    branch, through the plan (NaN-filled workspace) and through the module; .grad has the leaf's shape and the plan's bits.
    Measured worst rel-L2: simulator (tiny config) 5.4e-07 at T >= 25, 9.6e-07 at T = 17; MI355X (stock config) 1.6e-05 at T >= 25 (T = 25),
    5.4e-05 at T = 17 and 5.2e-05 at T = 19 (bars there 1.0e-4 and 1.04e-4)."""
    plan, ws, params, xs, d, dev, cfg, sd = _pass(kind)
    T = plan.T
    assert lib_flags(plan) & L.PLAN_INPUT_GRADS
    grads = _split(plan.d_x(ws), T)
    model = _model(kind, backend(kind)[0], dev, cfg, sd)
    leaves, mu, ls = _module_pass(kind, model, xs, d, dev)
    assert all(m.requires_grad and m.shape == (plan.c_lat, n) for m, n in zip(mu, plan.lat_len))
    worst = worst_short = 0.0
    for b, (ref, bar) in enumerate(_reference(kind, False)):
        assert torch.isfinite(grads[b]).all()
        r_plan, r_mod = rel(grads[b], ref), rel(leaves[b].grad, ref)
        print(f"utterance {b} T={T[b]}: rel-L2 plan {r_plan:.3e} module {r_mod:.3e} bar {bar:.3e}")
        if T[b] < SHORT:
            worst_short = max(worst_short, r_plan, r_mod)
        else:
            worst = max(worst, r_plan, r_mod)
        assert leaves[b].grad.shape == xs[b].shape
        assert r_plan <= bar and r_mod <= bar, (b, T[b], r_plan, r_mod, bar)
        assert torch.equal(leaves[b].grad.cpu(), grads[b])
    print(f"worst rel-L2: T >= {SHORT}: {worst:.3e}; T < {SHORT}: {worst_short:.3e}")


def lib_flags(plan):
    return plan.lib.avc_plan_flags(plan.h)


@pytest.mark.parametrize("kind", KINDS)
def test_mu_only(kind):
    """2. A loss on mu alone, only every second utterance a leaf: the same bars; utterances that do not require grad get no .grad."""
    plan, _, _, xs, d, dev, cfg, sd = _pass(kind)
    model = _model(kind, backend(kind)[0], dev, cfg, sd)
    need = set(range(0, len(xs), 2))
    ins, _, _ = _module_pass(kind, model, xs, d, dev, mu_only=True, need=need)
    full = _reference(kind, False)
    for b, (ref, bar) in enumerate(_reference(kind, True)):
        if b not in need:
            assert ins[b].grad is None
            continue
        r = rel(ins[b].grad, ref)
        print(f"utterance {b} T={plan.T[b]}: mu-only rel-L2 {r:.3e} bar {bar:.3e}")
        assert ins[b].grad.shape == xs[b].shape
        assert r <= bar, (b, plan.T[b], r, bar)
        assert rel(ins[b].grad, full[b][0]) > 1e-2   # (it is another gradient than the one of test 1)


def _encode_plan_floats(cfg, T):
    """avc_plan_workspace_floats of an unflagged ragged "encode" plan with default tuning, from its documented layout (every allocation
    rounded up to 64 floats): forward weight images [chunk][tap][CK][Mp], Mp = rows rounded up to 128, CK = 32 / 16 / 8 channels per chunk
    for 1 / 2-3 / >= 4 taps; the stacked bias of the two heads (32 x Mp); packed activations (cat, y0, out_0, per block a1, out, y1, y2);
    muls; the level tables (T, off, tiles per level, each padded to 4)."""
    c = cfg["ContentEncoder"]
    B = len(T)
    r64 = lambda n: (n + 63) // 64 * 64   # noqa: E731
    mp = lambda n: (n + 127) // 128 * 128   # noqa: E731
    ck = lambda k: 8 if k >= 4 else (16 if k >= 2 else 32)   # noqa: E731
    img = lambda co, ci, k: r64(-(-ci // ck(k)) * k * ck(k) * mp(co))   # noqa: E731
    nb = c["bank_size"] // c["bank_scale"]
    CC = nb * c["c_bank"] + c["c_in"]
    n = sum(img(c["c_bank"], c["c_in"], k) for k in range(c["bank_scale"], c["bank_size"] + 1, c["bank_scale"]))
    n += img(c["c_h"], CC, 1)
    n += 2 * c["n_conv_blocks"] * img(c["c_h"], c["c_h"], c["kernel_size"])
    n += img(2 * c["c_out"], c["c_h"], 1) + r64(32 * mp(2 * c["c_out"]))
    S = [sum(lv) for lv in _levels(cfg, T)]
    n += r64(CC * S[0]) + 2 * r64(c["c_h"] * S[0])
    for l in range(c["n_conv_blocks"]):
        n += 2 * r64(c["c_h"] * S[l]) + 2 * r64(c["c_h"] * S[l + 1])
    n += r64(2 * cfg["Decoder"]["c_in"] * S[-1])
    r4 = lambda k: (k + 3) // 4 * 4   # noqa: E731
    n += r64(sum(r4(B) + r4(B + 1) + r4(2 * sum(-(-t // 64) for t in lv)) for lv in _levels(cfg, T)))
    return n


@pytest.mark.parametrize("kind", KINDS)
def test_forward_is_unchanged(kind):
    """3. mu / log_sigma on the grad path are bit-equal to the no-grad call, to content_latents_ragged and to the unflagged "encode" plan
    in a NaN-filled workspace; that plan reports the workspace size it had before the backward pass existed, the flagged one a larger."""
    plan, ws, params, xs, _, dev, cfg, sd = _pass(kind)
    lib, T = plan.lib, plan.T
    model = _model(kind, backend(kind)[0], dev, cfg, sd)
    with torch.no_grad():
        mu0, ls0 = model.content_encoder_ragged([x.to(dev) for x in xs])
        lat = model.content_latents_ragged([x.to(dev) for x in xs])
    mu1, ls1 = model.content_encoder_ragged(_leaves(xs, dev))
    assert all(m.requires_grad for m in mu1 + ls1) and not any(m.requires_grad for m in mu0 + ls0)
    plain = RaggedPlan(cfg, T, None, lib=lib, mode="encode")
    assert lib_flags(plan) == lib_flags(plain) | L.PLAN_INPUT_GRADS and not lib_flags(plain) & L.PLAN_INPUT_GRADS
    assert plain.workspace_floats == _encode_plan_floats(cfg, T)
    assert plan.workspace_floats > plain.workspace_floats
    assert plan.lat_len == plain.lat_len
    w0 = _nan_ws(plain, dev)
    plain.forward(params, torch.cat(xs).to(dev), None, w0)
    mu2, ls2 = plain.latents(w0)
    mu3, ls3 = plan.latents(ws)
    for b in range(len(T)):
        assert torch.isfinite(mu2[b]).all() and torch.isfinite(ls2[b]).all()
        for got_mu, got_ls in ((mu0[b], ls0[b]), (mu1[b].detach(), ls1[b].detach()), (mu3[b], ls3[b])):
            assert torch.equal(got_mu, mu2[b]) and torch.equal(got_ls, ls2[b]), b
        assert torch.equal(lat[b], mu2[b])
    with pytest.raises(KeyError):
        plain.buffer("d_x")


@pytest.mark.parametrize("kind", KINDS)
def test_reproducible_and_isolated(kind):
    """4. Two backward passes give identical bits; the gradient of utterance b does not change when the other utterances are replaced; a
    forward-only ragged call (and a second grad forward of the same lengths) between forward and backward does not disturb the gradient."""
    plan, ws, params, xs, d, dev, cfg, sd = _pass(kind)
    T = plan.T
    first = plan.d_x(ws).clone()
    x = torch.cat(xs).to(dev)
    ws2 = _nan_ws(plan, dev)
    plan.forward(params, x, None, ws2)
    plan.backward_content(params, x, d.to(dev), ws2)
    assert torch.equal(plan.d_x(ws2), first)
    plan.backward_content(params, x, d.to(dev), ws2)   # ... and again on the same saved activations
    assert torch.equal(plan.d_x(ws2), first)
    # every other utterance replaced (same lengths, other content, other upstream weights): utterance `keep` keeps its gradient bit for bit
    M = xs[0].shape[1]
    other = _utts(T, M, 77)
    d2 = _d_muls(plan, 78)
    g0 = _split(first, T)
    c, base = plan.c_lat, plan.lat_off[0]
    for keep in (0, len(T) // 2, len(T) - 1):
        mix = [xs[b] if b == keep else other[b] for b in range(len(T))]
        dm = d2.clone()
        o, n = plan.lat_off[keep] - base, 2 * c * plan.lat_len[keep]
        dm[o:o + n] = d[o:o + n]
        xm = torch.cat(mix).to(dev)
        ws3 = _nan_ws(plan, dev)
        plan.forward(params, xm, None, ws3)
        plan.backward_content(params, xm, dm.to(dev), ws3)
        g = _split(plan.d_x(ws3), T)
        assert torch.equal(g[keep], g0[keep]), keep
        assert not torch.equal(g[(keep + 1) % len(T)], g0[(keep + 1) % len(T)])
    # through the module: the grad plan's workspace is its own
    model = _model(kind, backend(kind)[0], dev, cfg, sd)
    a = _leaves(xs, dev)
    mu_a, ls_a = model.content_encoder_ragged(a)
    with torch.no_grad():
        model.content_latents_ragged([t.to(dev) for t in other])
        model.content_encoder_ragged([t.to(dev) for t in other])
    b = _leaves(other, dev)
    mu_b, ls_b = model.content_encoder_ragged(b)   # same lengths, the first backward still pending: a private workspace

    def loss(mu, ls):
        return sum((m * wm[0].to(dev)).sum() + (s * wl[0].to(dev)).sum() for m, s, (wm, wl) in zip(mu, ls, _blocks(d, plan)))

    loss(mu_a, ls_a).backward()
    loss(mu_b, ls_b).backward()
    assert all(torch.equal(t.grad.cpu(), g) for t, g in zip(a, g0))
    assert not torch.equal(b[0].grad, a[0].grad)


@pytest.mark.parametrize("kind", KINDS)
def test_red_zones(kind):
    """5. x and d_muls inside NaN guards, the workspace inside sentinel guards: the guards stay intact, d_x is finite and bit-equal to
    the unguarded run."""
    plan, ws, params, xs, d, dev, cfg, sd = _pass(kind)
    x = guarded_input(torch.cat(xs), device=dev)
    dg = guarded_input(d, device=dev)
    assert x.is_contiguous() and dg.is_contiguous()
    g = GuardedOutput(plan.workspace_floats, device=dev)
    plan.forward(params, x, None, g.view)
    g.assert_intact("by the forward of the content plan with input gradients")
    plan.backward_content(params, x, dg, g.view)
    g.assert_intact("by avc_content_backward_ragged")
    got = plan.d_x(g.view)
    assert torch.isfinite(got).all()
    assert torch.equal(got, plan.d_x(ws))
    for a, b in zip(plan.latents(g.view)[0], plan.latents(ws)[0]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("kind", KINDS)
def test_refusals(kind):
    """6. What is out of scope is refused with a message that says what to pass; the existing entry points refuse what they refused."""
    lib, dev, cfg, sd, T, Tc = _setup(kind)
    M = cfg["ContentEncoder"]["c_in"]
    flagged = RaggedPlan(cfg, T, None, lib=lib, mode="encode", input_grads=True)
    params = flat_params(flagged, sd, dev)
    x = torch.cat(_utts(T, M, 9)).to(dev)
    d = _d_muls(flagged, 1).to(dev)
    ws = torch.zeros(flagged.workspace_floats, device=dev)
    P = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    others = (RaggedPlan(cfg, None, Tc, lib=lib, mode="speaker"), RaggedPlan(cfg, None, Tc, lib=lib, mode="speaker", input_grads=True),
              RaggedPlan(cfg, T, Tc, lib=lib), RaggedPlan(cfg, T, None, lib=lib, mode="emb"), RaggedPlan(cfg, T, None, lib=lib, mode="encode"),
              RaggedPlan(cfg, flagged.lat_len, None, lib=lib, mode="decode"), RaggedPlan(cfg, T, None, lib=lib, mode="fanout"))
    for other in others:
        assert lib.avc_content_backward_ragged(other.h, P(params), P(x), P(d), P(ws), None) == -8, other.mode
        assert "avc_plan_create_ragged_content_grads" in lib.avc_last_error().decode()
        with pytest.raises(RuntimeError, match="input_grads=True"):
            other.backward_content(params, x, d, ws)
    # null arguments
    for args in ((None, P(params), P(x), P(d), P(ws)), (flagged.h, None, P(x), P(d), P(ws)), (flagged.h, P(params), None, P(d), P(ws)),
                 (flagged.h, P(params), P(x), None, P(ws)), (flagged.h, P(params), P(x), P(d), None)):
        assert lib.avc_content_backward_ragged(*args, None) == -1
        msg = lib.avc_last_error().decode()
        assert "null argument" in msg and "avc_plan_create_ragged_content_grads" in msg
    # the speaker encoder's backward keeps refusing every plan that is not a flagged speaker plan, the new one included
    de = torch.zeros(len(T), flagged.c_emb, device=dev)
    assert lib.avc_backward_ragged(flagged.h, P(params), P(x), P(de), de.stride(0), de.stride(1), P(ws), None) == -8
    assert "AVC_PLAN_SPEAKER_ONLY | AVC_PLAN_INPUT_GRADS" in lib.avc_last_error().decode()
    with pytest.raises(RuntimeError, match="mode='speaker'"):
        flagged.backward(params, x, de, ws)
    # bf16 operand rounding: through the plan (-8) and through the module (a clear error that names the uniform path)
    bf = RaggedPlan(cfg, T, None, lib=lib, mode="encode", input_grads=True, compute_dtype="bf16")
    wsb = torch.zeros(bf.workspace_floats, device=dev)
    bf.forward(params, x, None, wsb)
    assert lib.avc_content_backward_ragged(bf.h, P(params), P(x), P(d), P(wsb), None) == -8
    assert "avc_plan_create_ragged_content_grads" in lib.avc_last_error().decode()
    with pytest.raises(RuntimeError, match="fp32"):
        bf.backward_content(params, x, d, wsb)
    model = _model(kind, lib, dev, cfg, sd, "bf16")
    with pytest.raises(RuntimeError, match=r"content_encoder\(x_b\)"):
        model.content_encoder_ragged(_leaves(_utts(T, M, 9), dev))
    with torch.no_grad():   # ... and without grad the bf16r call runs
        model.content_encoder_ragged([t.to(dev) for t in _utts(T, M, 9)])
    assert model.last_ragged_compute == "bf16r"
    # the reflect-pad rule of the forward plan: a 2-frame source
    c = cfg_from_dict(cfg)
    tun = L.make_tuning(lib)
    h = ctypes.c_void_p()
    assert lib.avc_plan_create_ragged_content_grads(ctypes.byref(c), 2, (ctypes.c_int * 2)(64, 2), ctypes.byref(tun), ctypes.byref(h)) == -6
    assert lib.avc_plan_create_ragged_content_grads(ctypes.byref(c), 0, (ctypes.c_int * 2)(64, 2), ctypes.byref(tun), ctypes.byref(h)) == -1
    assert lib.avc_plan_create_ragged_content_grads(ctypes.byref(c), 2, None, ctypes.byref(tun), ctypes.byref(h)) == -1
    # the existing creators refuse the flag where they did
    with pytest.raises(RuntimeError, match="AVC_PLAN_SPEAKER_ONLY"):
        RaggedPlan(cfg, T, Tc, lib=lib, mode="pairs", input_grads=True)
    with pytest.raises(RuntimeError, match="AVC_PLAN_SPEAKER_ONLY"):
        RaggedPlan(cfg, T, None, lib=lib, mode="emb", input_grads=True)
    for mode in ("fanout", "decode"):
        with pytest.raises(ValueError, match="forward only"):
            RaggedPlan(cfg, T, None, lib=lib, mode=mode, input_grads=True)
    hh = ctypes.c_void_p()
    arr = ctypes.c_int * len(T)
    assert lib.avc_plan_create_ragged_fanout(ctypes.byref(c), len(T), arr(*T), 0, None, L.PLAN_CONTENT_ONLY | L.PLAN_INPUT_GRADS, ctypes.byref(tun),
                                             ctypes.byref(hh)) == -1
    # the forward-only calls keep refusing inputs that require grad
    fp = _model(kind, lib, dev, cfg, sd)
    with pytest.raises(RuntimeError, match="forward-only"):
        fp.content_latents_ragged(_leaves(_utts(T, M, 3), dev))
