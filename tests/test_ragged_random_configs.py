"""Property tests of the ragged PART plans and of the four ragged backward passes over the reference's architecture family: the members
``tests/test_engine_random_configs.nets`` draws (kernel sizes 1 / 3 / 4 / 5 / 7, any subsample / upsample order, a speaker encoder whose
pattern differs from the content encoder's, 1 - 8 bank members, c_bank 4 - 12, c_h 8 - 40, n_mels 4 - 20, 0 - 3 dense blocks, ReLU and
LeakyReLU), 1 - 5 utterances whose lengths come from [lo, lo + 40] (lo: the shortest length ``nets`` found legal) or from
{63, 64, 65, 127, 128, 129}, with an odd length wherever a subsample of 2 occurs; plus a fixed list of six anchor configs that does not
need hypothesis.  Derandomised: the same cases every run.  kind='emu': the CPU lane-level simulation; kind='gpu': the gfx950 library.

Per case, fp32, every workspace and gradient buffer filled with NaN before use:
1. forward of every part plan ("speaker", "encode", "decode" from the caller's latents, "emb", "fanout") against the oracle of that
   sub-network per utterance at the forward tolerance (atol 2e-5 / rtol 1e-4), and the bit-identities of DESIGN 3.5 in fp32 and with bf16
   operand rounding: "emb" == "pairs", batch stride 0 == the expanded embedding, fan-out output j == output j of the expanded "emb" plan,
   decode(encode(...)) == both;
2. ``avc_backward_ragged``, ``avc_content_backward_ragged``, ``avc_decoder_backward_ragged`` and ``avc_backward_ragged_params`` against the
   fp64 oracle on the branch the engine took (tests/ragged_oracle.py), per utterance or per tensor
   err <= max(1e-4, 2 x err(fp32 oracle, fp64 oracle)) on the same branch; a tensor whose reference is below 1e-6 of the whole gradient
   is compared absolutely against that scale (tests/test_ragged_speaker_param_grads._check);
3. two passes on one plan give identical bits; the parameter pass leaves every float outside the speaker encoder's range NaN;
4. the forward of a flagged plan equals the unflagged plan's, bit for bit.
A case is left out only where the oracle itself raises its "Padding size ..." error for an utterance: every creator of a plan that runs
that sub-network must then raise as well.  No anchor is rejected; each property test asserts that at most a quarter of its examples are.
Rejected share (it depends on the oracle and the strategy alone): 0 of the 2 / 4 / 6 / 6 simulator examples and 0 of the 6 and of the 24 GPU
examples of each property test (``nets`` already keeps its shortest length legal, and no listed length undercuts a padding).

Measured worst rel-L2 over the anchors and all property examples (worst = largest error / bar; the bar of each of these was 1e-4):
simulator d_x_cond 2.5e-07, speaker parameters 1.6e-06, d_x 1.0e-06, d_z 6.0e-07, d_emb 7.4e-07; MI355X (anchors, 6 and 24 examples)
d_x_cond 2.5e-07, speaker parameters 1.6e-06, d_x 9.7e-07, d_z 6.1e-07, d_emb 1.1e-06.  Every forward comparison passes the forward
tolerance and every bit-identity holds on both."""
import copy

import pytest
import torch

from adaptive_voice_conversion_amd import _lib as L
from adaptive_voice_conversion_amd.engine import RaggedPlan
from oracle import avc_oracle as O
from tests.emu_util import KINDS, backend
from tests.ragged_oracle import content_masks, decoder_masks, decoder_oracle, speaker_masks, speaker_oracle
from tests.test_engine import flat_params
from tests.test_input_grads import oracle_input_grads
from tests.test_ragged_speaker_param_grads import _check as check_tensors, _tensors
from tests.test_submodules import rel

STRICT = dict(rtol=1e-4, atol=2e-5)
BAR = 1e-4
SPECIAL = [63, 64, 65, 127, 128, 129]
SHOWN = ("c_in", "c_h", "c_bank", "bank_size", "kernel_size", "n_conv_blocks", "subsample", "upsample", "n_dense_blocks", "act")
NETS = ("SpeakerEncoder", "ContentEncoder", "Decoder")
STATS = {}   # "<kind> <quantity>" -> [worst error / bar, that error, that bar] over the tests this process has run


def kinds_and_counts(emu, fast, full):
    """``tests.emu_util.KINDS`` crossed with the example counts: ``emu`` on the simulator; on the GPU ``fast`` in the plain ``-m gpu`` run
    and ``full`` behind the ``slow`` mark (the convention of tests/test_engine_random_configs.counts)."""
    out = []
    for k in KINDS:
        if k == "emu":
            out.append(pytest.param("emu", emu, id=f"emu-{emu}"))
        else:
            out.append(pytest.param("gpu", fast, marks=list(k.marks), id=f"gpu-{fast}"))
            out.append(pytest.param("gpu", full, marks=list(k.marks) + [pytest.mark.slow], id=f"gpu-{full}"))
    return pytest.mark.parametrize("kind,examples", out)


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
def _need(cfg):
    return max(cfg["Decoder"]["kernel_size"] // 2 + 2, 8)   # (the rule of `nets`: pad < length, and no InstanceNorm row of < 8 frames)


def _case(cfg, T, Tc, Tz, src_of, seed):
    return dict(cfg=cfg, T=list(T), Tc=list(Tc), Tz=list(Tz), src_of=list(src_of), seed=seed)


def _say(case):
    return (f"CASE T={case['T']} T_cond={case['Tc']} Tz={case['Tz']} src_of={case['src_of']} seed={case['seed']} "
            f"{ {k: {kk: vv for kk, vv in case['cfg'][k].items() if kk in SHOWN} for k in NETS} }")


def _strategy():
    from hypothesis import strategies as st
    from tests.test_engine_random_configs import nets

    def lens(draw, lo, n, odd):
        v = [draw(st.one_of(st.integers(lo, lo + 40), st.sampled_from(SPECIAL))) for _ in range(n)]
        if odd and all(t % 2 == 0 for t in v):
            i = draw(st.integers(0, n - 1))
            v[i] += -1 if v[i] > lo else 1
        return v

    @st.composite
    def cases(draw):
        cfg, _, lo = draw(nets())
        B = draw(st.integers(1, 5))
        T = lens(draw, lo, B, 2 in cfg["ContentEncoder"]["subsample"])
        Tc = lens(draw, lo, B, 2 in cfg["SpeakerEncoder"]["subsample"])
        Tz = lens(draw, _need(cfg), draw(st.integers(1, 5)), False)
        N = draw(st.integers(3, 6))
        src_of = [draw(st.integers(0, B - 1)) for _ in range(N)]
        src_of[-1] = src_of[0]   # one source used twice, by outputs that are not neighbours
        return _case(cfg, T, Tc, Tz, src_of, draw(st.integers(0, 1000)))
    return cases()


def _anchor_cfg(k, sub, up, ssub=None, c_h=16, n_mels=8, c_bank=8, bank_size=4, n_dense=2, act="relu"):
    ssub = list(ssub if ssub is not None else sub)
    cfg = O.tiny_config(n_mels=n_mels, c_h=c_h, c_bank=c_bank, bank_size=bank_size, n_blocks=len(sub), n_dense=n_dense, act=act)
    cfg["ContentEncoder"].update(kernel_size=k, subsample=list(sub))
    cfg["SpeakerEncoder"].update(kernel_size=k, n_conv_blocks=len(ssub), subsample=ssub)
    cfg["Decoder"].update(kernel_size=k, n_conv_blocks=len(up), upsample=list(up))
    return cfg


def _lo(cfg):
    """the shortest length `nets` would return for this config (its loop, from the smallest bottleneck)"""
    down = sdown = 1
    for v in cfg["ContentEncoder"]["subsample"]:
        down *= v
    for v in cfg["SpeakerEncoder"]["subsample"]:
        sdown *= v
    need = _need(cfg)
    T = need * down
    while T // sdown < need or T <= cfg["ContentEncoder"]["bank_size"] // 2 + 1:
        T += down
    return T


ANCHORS = {
    "k3_all2": (_anchor_cfg(3, [2, 2, 2], [2, 2, 2]), 4),
    "k4_lrelu": (_anchor_cfg(4, [1, 2], [1, 2, 1], c_h=32, n_mels=20, c_bank=4, bank_size=3, n_dense=1, act="lrelu"), 4),
    "k7_bank8": (_anchor_cfg(7, [2, 1, 2], [1, 2, 2], c_h=8, n_mels=12, bank_size=8), 4),
    "k1_flat": (_anchor_cfg(1, [1, 1], [1], bank_size=1, n_dense=0), 4),
    "k5_spk16": (_anchor_cfg(5, [1, 2], [2, 1], ssub=[2, 2, 2, 2], c_h=24, n_mels=4, c_bank=12), 4),
    "k3_b1": (_anchor_cfg(3, [2, 1], [1, 2], c_h=40, n_mels=12, bank_size=5, n_dense=3), 1),
}


def _anchor_cases(name):
    """One length set per anchor that contains lo, lo + 1, 64 and 65 (targets in another order; the decoder-only plan the same from its own
    minimum); the B = 1 anchor runs each of the four lengths as a plan of its own."""
    cfg, B = ANCHORS[name]
    lo, lz = _lo(cfg), _need(cfg)
    T, Tc, Tz = [lo, 65, lo + 1, 64], [64, lo + 1, 65, lo], [lz, 65, lz + 1, 64]
    seed = 100 + list(ANCHORS).index(name)
    if B == 1:
        return [_case(cfg, [t], [c], [z], [0, 0, 0], seed + i) for i, (t, c, z) in enumerate(zip(T, Tc, Tz))]
    return [_case(cfg, T, Tc, Tz, [2, 0, 3, 1, 2, 0], seed)]


# ---- helpers -------------------------------------------------------------------------------------------------------------------------
def _utts(lens, M, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(t, M, generator=g) for t in lens]


def _nan(n, dev):
    return torch.full((n,), float("nan"), device=dev)


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _oracle_or_none(fn):
    """fn() -- or None where the reference rejects the shape (its reflect padding needs pad < length)"""
    try:
        return fn()
    except RuntimeError as e:
        assert "Padding size" in str(e), e
        return None


def _must_refuse(say, lib, cfg, *plans):
    """the reference rejects an utterance of this sub-network: every creator that runs it raises too"""
    for mode, T, Tc, kw in plans:
        try:
            RaggedPlan(cfg, T, Tc, lib=lib, mode=mode, **kw)
        except RuntimeError:
            continue
        raise AssertionError(f"{say}: a {mode!r} plan {kw} was created for lengths the reference rejects")


def _note(key, err, bar):
    w = STATS.setdefault(key, [0.0, 0.0, 0.0])
    if err / bar > w[0]:
        w[:] = [err / bar, err, bar]


# ---- 1. forward of the part plans ------------------------------------------------------------------------------------------------------
def _check_forward(kind, case):
    """Forward of the five part plans against the oracle, and the bit-identities in fp32 and bf16r.  Returns False for a rejected case."""
    say = _say(case)
    print(say, flush=True)
    lib, dev = backend(kind)
    cfg, T, Tc, Tz, m, seed = (case[k] for k in ("cfg", "T", "Tc", "Tz", "src_of", "seed"))
    B, N, M = len(T), len(m), cfg["ContentEncoder"]["c_in"]
    C = cfg["ContentEncoder"]["c_out"]
    sd = O.make_state_dict(cfg, seed)
    xs, cs = _utts(T, M, seed + 1), _utts(Tc, M, seed + 2)
    g = torch.Generator().manual_seed(seed + 3)
    zs = [torch.randn(C, t, generator=g) for t in Tz]
    # the oracle of each sub-network per utterance; the voices of every call are speaker embeddings (tests/test_ragged_fanout.py: "Voices")
    E_ref = _oracle_or_none(lambda: torch.stack([O.speaker_encoder(c.t()[None], sd, cfg)[0] for c in cs]))
    lat_ref = _oracle_or_none(lambda: [O.content_encoder(x.t()[None], sd, cfg) for x in xs])
    spk_plans = [("speaker", None, Tc, {}), ("speaker", None, Tc, dict(input_grads=True)), ("speaker_pg", None, Tc, {}), ("pairs", T, Tc, {})]
    src_plans = [("encode", T, None, {}), ("encode", T, None, dict(input_grads=True)), ("emb", T, None, {}), ("fanout", T, None, dict(src_of=m)),
                 ("pairs", T, Tc, {})]
    if E_ref is None or lat_ref is None:
        _must_refuse(say, lib, cfg, *(spk_plans if E_ref is None else []), *(src_plans if lat_ref is None else []))
        return False
    voice = E_ref[:min(B, 3)].mean(0)                  # (for the one-voice call and the caller's latents)
    dec_ref = _oracle_or_none(lambda: [O.decoder(lat_ref[b][0], E_ref[b][None], sd, cfg)[0] for b in range(B)])
    own_ref = _oracle_or_none(lambda: [O.decoder(z[None], voice[None], sd, cfg)[0] for z in zs])
    if dec_ref is None or own_ref is None:
        _must_refuse(say, lib, cfg, *([("emb", T, None, {}), ("fanout", T, None, dict(src_of=m)), ("pairs", T, Tc, {})] if dec_ref is None else []),
                     *([("decode", Tz, None, {}), ("decode_ig", Tz, None, {})] if own_ref is None else []))
        return False
    fan_ref = [O.decoder(lat_ref[s][0], E_ref[j % B][None], sd, cfg)[0] for j, s in enumerate(m)]
    x, xc = torch.cat(xs).to(dev), torch.cat(cs).to(dev)
    close = lambda got, ref, what: torch.testing.assert_close(got.cpu(), ref, msg=lambda t: f"{say}\n{what}: {t}", **STRICT)   # noqa: E731

    for compute in ("fp32", "bf16"):
        fp32 = compute == "fp32"
        mk = lambda mode, t, tc=None, **kw: RaggedPlan(cfg, t, tc, lib=lib, mode=mode, compute_dtype=compute, **kw)   # noqa: E731
        spk = mk("speaker", None, Tc)
        params = flat_params(spk, sd, dev)
        ws_s = _nan(spk.workspace_floats, dev)
        spk.forward(params, None, xc, ws_s)
        E = spk.emb(ws_s).clone()
        pairs = mk("pairs", T, Tc)
        ws_p = _nan(pairs.workspace_floats, dev)
        pairs.forward(params, x, xc, ws_p)
        assert _same(pairs.emb(ws_p), E), (say, compute, "speaker plan != pairs plan")
        embp = mk("emb", T)
        ws_e = _nan(embp.workspace_floats, dev)
        embp.forward_emb(params, x, E, ws_e)
        assert embp.out_len == pairs.out_len == [dr.shape[1] for dr in dec_ref], (say, embp.out_len, pairs.out_len)
        for b, (a, p) in enumerate(zip(embp.outputs(ws_e), pairs.outputs(ws_p))):
            assert torch.isfinite(a).all() and _same(a, p), (say, compute, "emb plan != pairs plan", b)
        # one voice for all: batch stride 0 == the expanded rows
        e1 = E[0]
        ws_1, ws_x = _nan(embp.workspace_floats, dev), _nan(embp.workspace_floats, dev)
        embp.forward_emb(params, x, e1[None].expand(B, -1), ws_1)
        embp.forward_emb(params, x, e1[None].expand(B, -1).contiguous(), ws_x)
        for b, (a, p) in enumerate(zip(embp.outputs(ws_1), embp.outputs(ws_x))):
            assert torch.isfinite(a).all() and _same(a, p), (say, compute, "stride-0 emb != expanded emb", b)
        # fan-out == the expanded emb plan == decode(encode(...))
        Ef = torch.stack([E[j % B] for j in range(N)])
        fan = mk("fanout", T, src_of=m)
        ws_f = _nan(fan.workspace_floats, dev)
        fan.forward_emb(params, x, Ef, ws_f)
        exp = mk("emb", [T[s] for s in m])
        ws_x = _nan(exp.workspace_floats, dev)
        exp.forward_emb(params, torch.cat([xs[s] for s in m]).to(dev), Ef, ws_x)
        enc = mk("encode", T)
        ws_c = _nan(enc.workspace_floats, dev)
        enc.forward(params, x, None, ws_c)
        assert enc.lat_len == fan.lat_len == [r[0].shape[2] for r in lat_ref], (say, enc.lat_len, fan.lat_len)
        dp = mk("decode", enc.lat_len, src_of=m)
        ws_d = _nan(dp.workspace_floats, dev)
        o = enc.buffer("muls")
        dp.forward_latents(params, ws_c[o:o + 2 * C * sum(enc.lat_len)], 2 * C, Ef, ws_d)
        assert fan.out_len == exp.out_len == dp.out_len, (say, fan.out_len, exp.out_len, dp.out_len)
        for j, (a, p, q) in enumerate(zip(fan.outputs(ws_f), exp.outputs(ws_x), dp.outputs(ws_d))):
            assert torch.isfinite(a).all(), (say, compute, "fan-out output", j)
            assert _same(a, p), (say, compute, "fan-out != expanded emb plan", j, m[j], (a - p).abs().max().item())
            assert _same(a, q), (say, compute, "fan-out != decode(encode)", j, m[j], (a - q).abs().max().item())
        for (mu_f, ls_f), (mu_c, ls_c) in zip(zip(*fan.latents(ws_f)), zip(*enc.latents(ws_c))):
            assert _same(mu_f, mu_c) and _same(ls_f, ls_c), (say, compute, "fan-out latents != encode plan's")
        if not fp32:
            continue
        # against the oracle (fp32 only)
        for b in range(B):
            close(E[b], E_ref[b], f"speaker plan, target {b} (T_cond={Tc[b]})")
            close(embp.outputs(ws_e)[b], dec_ref[b], f"emb plan, source {b} (T={T[b]})")
        mu, ls = enc.latents(ws_c)
        for b in range(B):
            close(mu[b], lat_ref[b][0][0], f"encode plan, mu of source {b} (T={T[b]})")
            close(ls[b], lat_ref[b][1][0], f"encode plan, log_sigma of source {b} (T={T[b]})")
        for j, s in enumerate(m):
            close(fan.outputs(ws_f)[j], fan_ref[j], f"fan-out plan, output {j} (source {s}, T={T[s]})")
        own = mk("decode", Tz)
        ws_o = _nan(own.workspace_floats, dev)
        own.forward_latents(params, torch.cat([z.reshape(-1) for z in zs]).to(dev), C, voice.to(dev)[None].expand(len(Tz), -1), ws_o)
        for b, (a, r) in enumerate(zip(own.outputs(ws_o), own_ref)):
            assert tuple(a.shape) == tuple(r.shape), (say, b, a.shape, r.shape)
            close(a, r, f"decode plan, the caller's latent {b} (Tz={Tz[b]})")
    return True


# ---- 2. the backward passes -------------------------------------------------------------------------------------------------------------
def _check_speaker(kind, case):
    """avc_backward_ragged (d_x_cond per utterance) and avc_backward_ragged_params (every speaker tensor, d_x_cond) against the fp64
    oracle; repeatability; NaN outside the speaker's parameter range; flagged == unflagged forward.
    Measured worst rel-L2 (bar 1e-4): d_x_cond 2.5e-07 on the simulator and on the MI355X; parameters 1.6e-06 on both."""
    say = _say(case)
    print(say, flush=True)
    lib, dev = backend(kind)
    cfg, Tc, seed = case["cfg"], case["Tc"], case["seed"]
    B, M = len(Tc), cfg["ContentEncoder"]["c_in"]
    sd = O.make_state_dict(cfg, seed)
    cs = _utts(Tc, M, seed + 2)
    if _oracle_or_none(lambda: [O.speaker_encoder(c.t()[None], sd, cfg) for c in cs]) is None:
        _must_refuse(say, lib, cfg, ("speaker", None, Tc, dict(input_grads=True)), ("speaker_pg", None, Tc, {}))
        return False
    xc = torch.cat(cs).to(dev)
    plain = RaggedPlan(cfg, None, Tc, lib=lib, mode="speaker")
    ig = RaggedPlan(cfg, None, Tc, lib=lib, mode="speaker", input_grads=True)
    pg = RaggedPlan(cfg, None, Tc, lib=lib, mode="speaker_pg")
    params = flat_params(pg, sd, dev)
    d = torch.randn(B, pg.c_emb, generator=torch.Generator().manual_seed(seed + 4))
    dd = d.to(dev)
    w0, w1, w2 = (_nan(p.workspace_floats, dev) for p in (plain, ig, pg))
    plain.forward(params, None, xc, w0)
    ig.forward(params, None, xc, w1)
    pg.forward(params, None, xc, w2)
    assert torch.isfinite(plain.emb(w0)).all(), say
    assert _same(ig.emb(w1), plain.emb(w0)) and _same(pg.emb(w2), plain.emb(w0)), (say, "flagged forward != unflagged forward")
    ig.backward(params, xc, dd, w1)
    g_ig = ig.d_x_cond(w1).clone()
    ig.backward(params, xc, dd, w1)
    assert _same(ig.d_x_cond(w1), g_ig), (say, "avc_backward_ragged: two passes differ")
    grads = _nan(pg.param_floats, dev)
    pg.backward_params(params, xc, dd, grads, w2)
    g_pg = pg.d_x_cond(w2).clone()
    again = _nan(pg.param_floats, dev)
    pg.backward_params(params, xc, dd, again, w2)
    assert _same(again, grads) and _same(pg.d_x_cond(w2), g_pg), (say, "avc_backward_ragged_params: two passes differ")
    import ctypes
    lo, num = ctypes.c_long(), ctypes.c_long()
    assert lib.avc_plan_param_range(pg.h, L.GRADS_SPEAKER, ctypes.byref(lo), ctypes.byref(num)) == 0
    nan = torch.isnan(grads.cpu())
    assert nan[:lo.value].all() and nan[lo.value + num.value:].all(), (say, "a float outside the speaker's parameter range was written")
    masks = speaker_masks(pg, w2)
    assert all(torch.equal(a, b) for ma, mb in zip(masks, speaker_masks(ig, w1)) for a, b in zip(ma, mb)), say
    r64, x64 = speaker_oracle(cfg, sd, cs, masks, d, torch.float64, inputs=True)
    r32, x32 = speaker_oracle(cfg, sd, cs, masks, d, torch.float32, inputs=True)
    for name, got in (("avc_backward_ragged", g_ig), ("avc_backward_ragged_params", g_pg)):
        assert torch.isfinite(got).all(), (say, name)
        for b, gb in enumerate(torch.split(got.cpu(), Tc)):
            bar = max(BAR, 2 * rel(x32[b], x64[b]))
            e = rel(gb, x64[b])
            _note(f"{kind} d_x_cond", e, bar)
            assert e <= bar, (say, name, f"d_x_cond of utterance {b} (T_cond={Tc[b]})", e, bar)
    try:
        worst = check_tensors(_tensors(pg, sd, grads), r64, r32, f"{kind} speaker parameters")
    except AssertionError as e:
        raise AssertionError(f"{say}\n{e}") from e
    if worst[1] is not None:
        _note(f"{kind} speaker parameters", worst[2], worst[2] / worst[0])
    return True


def _check_content(kind, case):
    """avc_content_backward_ragged: d_x per utterance (random d_muls on mu and log_sigma) against the fp64 oracle; repeatability; flagged ==
    unflagged forward.  Measured worst rel-L2 (bar 1e-4): simulator 1.0e-06, MI355X 9.7e-07."""
    say = _say(case)
    print(say, flush=True)
    lib, dev = backend(kind)
    cfg, T, seed = case["cfg"], case["T"], case["seed"]
    M = cfg["ContentEncoder"]["c_in"]
    sd = O.make_state_dict(cfg, seed)
    xs = _utts(T, M, seed + 1)
    if _oracle_or_none(lambda: [O.content_encoder(x.t()[None], sd, cfg) for x in xs]) is None:
        _must_refuse(say, lib, cfg, ("encode", T, None, dict(input_grads=True)))
        return False
    x = torch.cat(xs).to(dev)
    plain = RaggedPlan(cfg, T, None, lib=lib, mode="encode")
    plan = RaggedPlan(cfg, T, None, lib=lib, mode="encode", input_grads=True)
    params = flat_params(plan, sd, dev)
    w0, ws = _nan(plain.workspace_floats, dev), _nan(plan.workspace_floats, dev)
    plain.forward(params, x, None, w0)
    plan.forward(params, x, None, ws)
    c = plan.c_lat
    n = 2 * c * sum(plan.lat_len)
    a, b = plain.buffer("muls"), plan.buffer("muls")
    assert torch.isfinite(w0[a:a + n]).all() and _same(w0[a:a + n], ws[b:b + n]), (say, "flagged forward != unflagged forward")
    d = torch.randn(n, generator=torch.Generator().manual_seed(seed + 5))
    plan.backward_content(params, x, d.to(dev), ws)
    first = plan.d_x(ws).clone()
    plan.backward_content(params, x, d.to(dev), ws)
    assert _same(plan.d_x(ws), first), (say, "avc_content_backward_ragged: two passes differ")
    assert torch.isfinite(first).all(), say
    masks = content_masks(plan, ws, cfg)
    fn = lambda t, s: O.content_encoder(t, s, cfg)   # noqa: E731
    o = 0
    for b, (xb, gb) in enumerate(zip(xs, torch.split(first.cpu(), T))):
        blk = d[o:o + 2 * c * plan.lat_len[b]].view(2 * c, plan.lat_len[b])
        o += blk.numel()
        w = [blk[:c][None], blk[c:][None]]
        r64, = oracle_input_grads(fn, [xb.t()[None]], sd, masks[b], w)
        r32, = oracle_input_grads(fn, [xb.t()[None]], sd, masks[b], w, dtype=torch.float32)
        bar = max(BAR, 2 * rel(r32, r64))
        e = rel(gb, r64[0].t())
        _note(f"{kind} d_x", e, bar)
        assert e <= bar, (say, f"d_x of utterance {b} (T={T[b]})", e, bar)
    return True


def _check_decoder(kind, case):
    """avc_decoder_backward_ragged: d_z per latent and d_emb per row against the fp64 oracle; repeatability; flagged == unflagged forward.
    Measured worst rel-L2 (bar 1e-4): d_z 6.0e-07 / d_emb 7.4e-07 on the simulator, 6.1e-07 / 1.1e-06 on the MI355X."""
    say = _say(case)
    print(say, flush=True)
    lib, dev = backend(kind)
    cfg, Tz, seed = case["cfg"], case["Tz"], case["seed"]
    dcfg = cfg["Decoder"]
    sd = O.make_state_dict(cfg, seed)
    g = torch.Generator().manual_seed(seed + 3)
    zs = [torch.randn(dcfg["c_in"], t, generator=g) for t in Tz]
    emb = torch.randn(len(Tz), dcfg["c_cond"], generator=g)
    if _oracle_or_none(lambda: [O.decoder(z[None], e[None], sd, cfg) for z, e in zip(zs, emb)]) is None:
        _must_refuse(say, lib, cfg, ("decode_ig", Tz, None, {}))
        return False
    plain = RaggedPlan(cfg, Tz, None, lib=lib, mode="decode")
    plan = RaggedPlan(cfg, Tz, None, lib=lib, mode="decode_ig")
    params = flat_params(plan, sd, dev)
    z, e = torch.cat([t.reshape(-1) for t in zs]).to(dev), emb.to(dev)
    w0, ws = _nan(plain.workspace_floats, dev), _nan(plan.workspace_floats, dev)
    plain.forward_latents(params, z, plain.c_lat, e, w0)
    plan.forward_latents(params, z, plan.c_lat, e, ws)
    assert plan.out_len == plain.out_len, say
    for a, b in zip(plain.outputs(w0), plan.outputs(ws)):
        assert torch.isfinite(a).all() and _same(a, b), (say, "flagged forward != unflagged forward")
    M = plan.n_mels
    d = torch.randn(M * sum(plan.out_len), generator=torch.Generator().manual_seed(seed + 6))
    plan.backward_decoder(params, z, plan.c_lat, e, d.to(dev), ws)
    dz, de = [t.clone() for t in plan.d_z(ws)], plan.d_emb(ws).clone()
    plan.backward_decoder(params, z, plan.c_lat, e, d.to(dev), ws)
    assert _same(plan.d_emb(ws), de) and all(_same(a, b) for a, b in zip(plan.d_z(ws), dz)), (say, "avc_decoder_backward_ragged: two passes differ")
    masks = decoder_masks(plan, ws, cfg)
    o = 0
    for b, n in enumerate(plan.out_len):
        w = d[o:o + M * n].view(1, M, n)
        o += M * n
        (rz, re, _), (fz, fe, _) = (decoder_oracle(zs[b], emb[b], w, sd, cfg, masks[b], t) for t in (torch.float64, torch.float32))
        assert torch.isfinite(dz[b]).all() and torch.isfinite(de[b]).all(), (say, b)
        bz, be = max(BAR, 2 * rel(fz, rz)), max(BAR, 2 * rel(fe, re))
        ez, ee = rel(dz[b], rz), rel(de[b], re)
        _note(f"{kind} d_z", ez, bz)
        _note(f"{kind} d_emb", ee, be)
        assert ez <= bz, (say, f"d_z of latent {b} (Tz={Tz[b]})", ez, bz)
        assert ee <= be, (say, f"d_emb of latent {b} (Tz={Tz[b]})", ee, be)
    return True


CHECKS = {"forward": _check_forward, "speaker": _check_speaker, "content": _check_content, "decoder": _check_decoder}
REJECTED = 0.25   # the cap on the share of drawn examples the reference rejects, asserted per property test (measured: 0, module docstring)


def _property(kind, examples, check):
    pytest.importorskip("hypothesis")   # (test-only dependency; the anchors below do not need it)
    from hypothesis import HealthCheck, given, settings
    seen = [0, 0]

    @settings(max_examples=examples, deadline=None, derandomize=True, suppress_health_check=list(HealthCheck))
    @given(_strategy())
    def run(case):
        seen[0] += 1
        seen[1] += not CHECKS[check](kind, copy.deepcopy(case))
    run()
    print(f"{check}: {seen[1]} of {seen[0]} examples rejected by the reference;",
          {k: f"{v[1]:.2e} / {v[2]:.2e}" for k, v in STATS.items() if k.startswith(kind)}, flush=True)
    assert seen[1] <= REJECTED * seen[0], (check, seen)


@kinds_and_counts(2, 6, 24)
def test_part_plan_forwards_over_random_configs(kind, examples):
    _property(kind, examples, "forward")


@kinds_and_counts(4, 6, 24)
def test_speaker_backward_over_random_configs(kind, examples):
    _property(kind, examples, "speaker")


@kinds_and_counts(6, 6, 24)
def test_content_backward_over_random_configs(kind, examples):
    _property(kind, examples, "content")


@kinds_and_counts(6, 6, 24)
def test_decoder_backward_over_random_configs(kind, examples):
    _property(kind, examples, "decoder")


@pytest.mark.parametrize("check", list(CHECKS))
@pytest.mark.parametrize("anchor", list(ANCHORS))
@pytest.mark.parametrize("kind", KINDS)
def test_anchor_configs(kind, anchor, check):
    """The fixed list: no hypothesis, no rejected case."""
    for case in _anchor_cases(anchor):
        assert CHECKS[check](kind, case), ("the reference rejects an anchor", _say(case))
    print({k: f"{v[1]:.2e} / {v[2]:.2e}" for k, v in STATS.items() if k.startswith(kind)}, flush=True)
