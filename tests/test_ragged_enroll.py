"""Enrol a speaker once: the two part plans of the ragged (variable-length) engine -- speaker encoder alone
(AVC_PLAN_SPEAKER_ONLY) and content encoder + decoder from caller-supplied embeddings (AVC_PLAN_EMB_INPUT) -- and what is built on
them: ``AE.get_speaker_embeddings_ragged``, ``AE.inference_ragged(xs, emb=...)``, ``Inferencer.enroll`` /
``convert_batch(sources, emb=...)`` and the command line.  On the CPU simulator build (kind='emu', tiny config) and on the GPU
(kind='gpu', the stock 80-mel config).

Tolerances: the project's forward tolerance (rtol 1e-4, atol 2e-5; README "Stated tolerances").  Embeddings are held to it at every
length (the speaker encoder has no InstanceNorm).  Decoded outputs are held to it for sources of 25 frames and more; a source of
fewer than 25 frames reaches 3-frame rows at the bottleneck, where InstanceNorm is ill-conditioned in fp32 (the oracle's own fp32 and
fp64 runs use up to 1.3x of the strict tolerance there): those get the allowance tests/test_feed_infer.py already makes
(rtol 1e-3, atol 2e-4).  Nothing else is loosened and no case is filtered out."""
import contextlib
import ctypes
import pickle
import types

import numpy as np
import pytest
import torch

from adaptive_voice_conversion_amd import _lib as L
from adaptive_voice_conversion_amd.engine import RaggedPlan, cfg_from_dict
from adaptive_voice_conversion_amd.inference import Inferencer, parse_args
from adaptive_voice_conversion_amd.model import AE
from oracle import avc_oracle as O
from tests.emu_util import KINDS, backend
from tests.test_engine import flat_params

STRICT = dict(rtol=1e-4, atol=2e-5)
SHORT = dict(rtol=1e-3, atol=2e-4)   # sources of fewer than 25 frames only


def _tol(T):
    return SHORT if T < 25 else STRICT


def _setup(kind, seed=21):
    """(lib, device, config, state_dict, source lengths, target lengths): 17 is the shortest length the stock config accepts, 64 / 65 are
    one column tile / one frame into the second, most of the rest are not multiples of 8."""
    lib, dev = backend(kind)
    if kind == "emu":
        cfg = O.tiny_config()
        T = [17, 64, 65, 31, 90, 19, 43]
        Tc = [65, 17, 64, 90, 29, 50, 23]
    else:
        cfg = O.stock_config(80)
        T = [17, 64, 65, 600, 333, 25, 19, 200, 31, 90, 123, 407]
        Tc = [65, 17, 64, 29, 600, 411, 250, 23, 333, 58, 90, 171]
    return lib, dev, cfg, O.make_state_dict(cfg, seed), T, Tc


def _utts(lens, M, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(t, M, generator=g) for t in lens]


def _model(kind, lib, dev, cfg, sd, compute_dtype=None):
    model = AE(cfg, lib=lib if kind == "emu" else None, compute_dtype=compute_dtype)
    model.load_state_dict(sd)
    return model.to(dev)


def _nan_ws(plan, dev):
    return torch.full((plan.workspace_floats,), float("nan"), device=dev)


@pytest.mark.parametrize("kind", KINDS)
def test_speaker_plan_matches_oracle(kind):
    """1. Row b of get_speaker_embeddings_ragged against O.speaker_encoder(x_cond_b), forward tolerance at every length; the plan runs in a
    workspace filled with NaN (every region it reads it has written before)."""
    lib, dev, cfg, sd, _, Tc = _setup(kind)
    M = cfg["ContentEncoder"]["c_in"]
    cs = _utts(Tc, M, 9)
    plan = RaggedPlan(cfg, None, Tc, lib=lib, mode="speaker")
    assert lib.avc_plan_flags(plan.h) & L.PLAN_SPEAKER_ONLY and lib.avc_plan_flags(plan.h) & L.PLAN_RAGGED
    params = flat_params(plan, sd, dev)
    ws = _nan_ws(plan, dev)
    plan.forward(params, None, torch.cat(cs).to(dev), ws)
    emb = plan.emb(ws).cpu()
    assert emb.shape == (len(Tc), cfg["SpeakerEncoder"]["c_out"])
    for b, c in enumerate(cs):
        ref = O.speaker_encoder(c.t()[None], sd, cfg)[0]
        torch.testing.assert_close(emb[b], ref, msg=lambda m: f"target {b} (T_cond={Tc[b]}): {m}", **STRICT)
    # ... and through the module (pooled workspace, plan cache)
    model = _model(kind, lib, dev, cfg, sd)
    got = model.get_speaker_embeddings_ragged([c.to(dev) for c in cs])
    assert model.last_ragged_compute == "fp32"
    assert torch.equal(got.cpu(), emb)


@pytest.mark.parametrize("kind", KINDS)
def test_speaker_plan_is_bit_identical_to_the_whole_ragged_plan(kind):
    """2. fp32: ws["emb"] of a "pairs" plan on (xs, x_conds) equals ws["emb"] of the "speaker" plan on x_conds, bit for bit."""
    lib, dev, cfg, sd, T, Tc = _setup(kind)
    M = cfg["ContentEncoder"]["c_in"]
    xs, cs = _utts(T, M, 9), _utts(Tc, M, 10)
    whole = RaggedPlan(cfg, T, Tc, lib=lib)
    params = flat_params(whole, sd, dev)
    ws = _nan_ws(whole, dev)
    whole.forward(params, torch.cat(xs).to(dev), torch.cat(cs).to(dev), ws)
    part = RaggedPlan(cfg, None, Tc, lib=lib, mode="speaker")
    ws2 = _nan_ws(part, dev)
    part.forward(params, None, torch.cat(cs).to(dev), ws2)
    assert torch.equal(whole.emb(ws).cpu(), part.emb(ws2).cpu())
    assert not torch.isnan(part.emb(ws2)).any()


@pytest.mark.parametrize("compute,expect", [("fp32", "fp32"), ("bf16", "bf16r")])
@pytest.mark.parametrize("kind", KINDS)
def test_conversion_from_embeddings_is_bit_identical_to_pairs(kind, compute, expect):
    """3. inference_ragged(xs, emb=E) with E = get_speaker_embeddings_ragged(x_conds) equals inference_ragged(xs, x_conds), utterance by
    utterance, with torch.equal -- in fp32 and with bf16 operand rounding."""
    lib, dev, cfg, sd, T, Tc = _setup(kind)
    M = cfg["ContentEncoder"]["c_in"]
    xs, cs = [x.to(dev) for x in _utts(T, M, 9)], [c.to(dev) for c in _utts(Tc, M, 10)]
    model = _model(kind, lib, dev, cfg, sd, compute)
    pairs = model.inference_ragged(xs, cs)
    assert model.last_ragged_compute == expect
    E = model.get_speaker_embeddings_ragged(cs)
    assert model.last_ragged_compute == expect
    got = model.inference_ragged(xs, emb=E)
    assert model.last_ragged_compute == expect
    assert len(got) == len(pairs) == len(T)
    for b in range(len(T)):
        assert got[b].shape == pairs[b].shape
        assert torch.equal(got[b], pairs[b]), (b, T[b], Tc[b], (got[b] - pairs[b]).abs().max().item())
    # positional call as before
    again = model.inference_ragged(xs, cs)
    assert all(torch.equal(a, p) for a, p in zip(again, pairs))


@pytest.mark.parametrize("kind", KINDS)
def test_one_voice_for_all(kind):
    """4. emb of shape [c_emb] (batch stride 0 inside the engine) == the expanded, contiguous [B, c_emb] call bit for bit; every result
    against O.decoder(O.content_encoder(x_b)[0], e); e = mean of three embeddings (not the embedding of any one utterance).  Once with a
    non-contiguous column view (element stride != 1)."""
    lib, dev, cfg, sd, T, Tc = _setup(kind)
    M = cfg["ContentEncoder"]["c_in"]
    xs, cs = _utts(T, M, 9), _utts(Tc[:3], M, 10)
    e = torch.stack([O.speaker_encoder(c.t()[None], sd, cfg)[0] for c in cs]).mean(0)
    model = _model(kind, lib, dev, cfg, sd)
    B = len(T)
    one = model.inference_ragged([x.to(dev) for x in xs], emb=e.to(dev))
    full = model.inference_ragged([x.to(dev) for x in xs], emb=e.to(dev).expand(B, -1).contiguous())
    row = model.inference_ragged([x.to(dev) for x in xs], emb=e.to(dev)[None])
    wide = torch.zeros(B, 2 * e.numel(), device=dev)
    wide[:, ::2] = e.to(dev)
    col = wide[:, ::2]
    assert col.stride(1) == 2 and not col.is_contiguous()
    strided = model.inference_ragged([x.to(dev) for x in xs], emb=col)
    for b in range(B):
        assert torch.equal(one[b], full[b]), (b, T[b])
        assert torch.equal(row[b], full[b]), (b, T[b])
        assert torch.equal(strided[b], full[b]), (b, T[b])
        ref = O.decoder(O.content_encoder(xs[b].t()[None], sd, cfg)[0], e[None], sd, cfg)[0]
        assert tuple(one[b].shape) == tuple(ref.shape)
        torch.testing.assert_close(one[b].cpu(), ref, msg=lambda m: f"source {b} (T={T[b]}): {m}", **_tol(T[b]))


@pytest.mark.parametrize("kind", KINDS)
def test_only_the_branch_that_runs_is_constrained(kind):
    """5. The reflect-pad rule per plan: a 2-frame target breaks the speaker plan; an emb plan has no target lengths at all; a 2-frame source
    breaks the emb plan."""
    lib, dev, cfg, sd, _, _ = _setup(kind)
    with pytest.raises(RuntimeError, match="Padding size should be less"):
        RaggedPlan(cfg, None, [40, 2], lib=lib, mode="speaker")
    with pytest.raises(RuntimeError, match="Padding size should be less"):
        RaggedPlan(cfg, [40, 40], [40, 2], lib=lib)
    ok = RaggedPlan(cfg, [40, 40], None, lib=lib, mode="emb")
    assert ok.out_len == [40, 40] and lib.avc_plan_flags(ok.h) & L.PLAN_EMB_INPUT
    assert RaggedPlan(cfg, [2, 2], [40, 40], lib=lib, mode="speaker").B == 2   # T is ignored by a speaker plan
    with pytest.raises(RuntimeError, match="Padding size should be less"):
        RaggedPlan(cfg, [40, 2], None, lib=lib, mode="emb")


@pytest.mark.parametrize("kind", KINDS)
def test_part_plans_are_smaller(kind):
    """6. Same lengths: both part plans need strictly less workspace than the whole plan; the emb plan saves at least the speaker encoder's
    first activation buffer (c_h floats per target frame), which the whole plan allocates and the emb plan does not."""
    lib, dev, cfg, sd, T, Tc = _setup(kind)
    whole = RaggedPlan(cfg, T, Tc, lib=lib).workspace_floats
    spk = RaggedPlan(cfg, None, Tc, lib=lib, mode="speaker").workspace_floats
    emb = RaggedPlan(cfg, T, None, lib=lib, mode="emb").workspace_floats
    assert 0 < spk < whole and 0 < emb < whole
    assert whole - emb >= cfg["SpeakerEncoder"]["c_h"] * sum(Tc)


def _create(lib, cfg, T, Tc, flags, ex=True):
    c = cfg_from_dict(cfg)
    h = ctypes.c_void_p()
    tun = L.make_tuning(lib)
    B = len(T if T is not None else Tc)
    arr = ctypes.c_int * B
    t = arr(*T) if T is not None else None
    tc = arr(*Tc) if Tc is not None else None
    if ex:
        rc = lib.avc_plan_create_ragged_ex(ctypes.byref(c), B, t, tc, flags, ctypes.byref(tun), ctypes.byref(h))
    else:
        rc = lib.avc_plan_create_ragged(ctypes.byref(c), B, t, tc, ctypes.byref(tun), ctypes.byref(h))
    return rc, h


@pytest.mark.parametrize("kind", KINDS)
def test_c_abi_refusals(kind):
    """7. Every refusal by return code and by a word of avc_last_error that names the call.  All of them are decided on the host before any
    launch, so the pointers are never dereferenced."""
    lib, dev, cfg, sd, _, _ = _setup(kind)
    err = lambda: lib.avc_last_error().decode()
    one = ctypes.c_void_p(64)
    T, Tc = [40, 33], [29, 50]
    rc, h = _create(lib, cfg, T, Tc, L.PLAN_SPEAKER_ONLY | L.PLAN_EMB_INPUT)
    assert rc == -1 and "avc_plan_create_ragged_ex" in err() and "exclude each other" in err()
    for bad in (L.PLAN_INFERENCE, L.PLAN_X3, L.PLAN_BF16S, L.PLAN_CONTENT_ONLY, L.PLAN_DECODER_ONLY, L.PLAN_PART_GRADS, L.PLAN_INPUT_GRADS, 1024,
                L.PLAN_EMB_INPUT | L.PLAN_X3):
        rc, h = _create(lib, cfg, T, Tc, bad)
        assert rc == -1 and "avc_plan_create_ragged_ex" in err() and "unknown flag" in err(), (bad, rc, err())
    rc, pe = _create(lib, cfg, T, None, L.PLAN_EMB_INPUT)
    assert rc == 0 and lib.avc_plan_flags(pe) == L.PLAN_INFERENCE | L.PLAN_RAGGED | L.PLAN_EMB_INPUT
    rc, ps = _create(lib, cfg, None, Tc, L.PLAN_SPEAKER_ONLY)
    assert rc == 0 and lib.avc_plan_flags(ps) == L.PLAN_INFERENCE | L.PLAN_RAGGED | L.PLAN_SPEAKER_ONLY
    rc, pw = _create(lib, cfg, T, Tc, 0)
    assert rc == 0 and lib.avc_plan_flags(pw) == L.PLAN_INFERENCE | L.PLAN_RAGGED
    try:
        assert lib.avc_forward_ragged(pe, one, one, one, one, None) == -8 and "avc_forward_ragged_emb" in err()
        for p in (pw, ps):
            assert lib.avc_forward_ragged_emb(p, one, one, one, 1, 1, one, None) == -8
            assert "avc_forward_ragged_emb" in err() and "AVC_PLAN_EMB_INPUT" in err()
        assert lib.avc_forward_ragged_emb(pe, one, one, None, 1, 1, one, None) == -1 and "avc_forward_ragged_emb" in err() and "emb is NULL" in err()
        assert lib.avc_forward_ragged_emb(pe, one, one, one, -1, 1, one, None) == -1 and "strides" in err()
        assert lib.avc_forward_ragged(ps, one, one, None, one, None) == -1 and "avc_forward_ragged" in err() and "x_cond" in err()
        lens, offs = (ctypes.c_int * 2)(), (ctypes.c_long * 2)()
        assert lib.avc_plan_ragged_out(ps, lens, offs) == -8 and "speaker-only" in err()
        lw, ow = (ctypes.c_int * 2)(), (ctypes.c_long * 2)()
        assert lib.avc_plan_ragged_out(pe, lens, offs) == 0 and lib.avc_plan_ragged_out(pw, lw, ow) == 0
        assert list(lens) == list(lw) and lens[0] >= 40 and lens[1] >= 33     # same sources, same converted lengths
        # both part plans take the compute dtype switch of whole ragged plans
        for p in (pe, ps):
            assert lib.avc_plan_set_compute_dtype(p, 1) == 0 and lib.avc_plan_compute_dtype(p) == 1
        # buffers a plan does not have are unknown to it
        assert lib.avc_plan_buffer(pe, b"emb") == -1 and lib.avc_plan_buffer(pe, b"dec") >= 0
        assert lib.avc_plan_buffer(ps, b"dec") == -1 and lib.avc_plan_buffer(ps, b"emb") >= 0
    finally:
        for p in (pe, ps, pw):
            lib.avc_plan_destroy(p)


@pytest.mark.parametrize("kind", KINDS)
def test_flags_zero_is_the_existing_ragged_plan(kind):
    """8. avc_plan_create_ragged and avc_plan_create_ragged_ex(flags = 0): same workspace size, same buffer offsets, same outputs."""
    lib, dev, cfg, sd, T, Tc = _setup(kind)
    M = cfg["ContentEncoder"]["c_in"]
    x, xc = torch.cat(_utts(T, M, 9)).to(dev), torch.cat(_utts(Tc, M, 10)).to(dev)
    rc0, p0 = _create(lib, cfg, T, Tc, 0, ex=False)
    rc1, p1 = _create(lib, cfg, T, Tc, 0, ex=True)
    assert rc0 == 0 and rc1 == 0
    try:
        n = lib.avc_plan_workspace_floats(p0)
        assert n == lib.avc_plan_workspace_floats(p1)
        for name in (b"emb", b"muls", b"dec", b"cond"):
            assert lib.avc_plan_buffer(p0, name) == lib.avc_plan_buffer(p1, name) >= 0
        assert lib.avc_plan_flags(p0) == lib.avc_plan_flags(p1)
        B = len(T)
        outs = []
        params = flat_params(RaggedPlan(cfg, T, Tc, lib=lib), sd, dev)
        for p in (p0, p1):
            lens, offs = (ctypes.c_int * B)(), (ctypes.c_long * B)()
            assert lib.avc_plan_ragged_out(p, lens, offs) == 0
            ws = torch.full((n,), float("nan"), device=dev)
            stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream) if dev.type == "cuda" else None
            with (torch.cuda.device(dev) if dev.type == "cuda" else contextlib.nullcontext()):
                rc = lib.avc_forward_ragged(p, params.data_ptr(), x.data_ptr(), xc.data_ptr(), ws.data_ptr(), stream)
            assert rc == 0, lib.avc_last_error().decode()
            outs.append((list(lens), list(offs), ws.cpu()))
        assert outs[0][0] == outs[1][0] and outs[0][1] == outs[1][1]
        lo, hi = outs[0][1][0], outs[0][1][-1] + M * outs[0][0][-1]
        assert not torch.isnan(outs[0][2][lo:hi]).any()
        assert torch.equal(outs[0][2][lo:hi], outs[1][2][lo:hi])
        eo = lib.avc_plan_buffer(p0, b"emb")
        ne = B * cfg["SpeakerEncoder"]["c_out"]
        assert torch.equal(outs[0][2][eo:eo + ne], outs[1][2][eo:eo + ne])
    finally:
        lib.avc_plan_destroy(p0)
        lib.avc_plan_destroy(p1)


@pytest.mark.parametrize("kind", KINDS)
def test_inferencer_enrols_and_converts(kind, tmp_path):
    """9. Inferencer.enroll == mean of the oracle's embeddings; convert_batch(sources, emb=...) against the oracle through an attr file;
    convert_batch(pairs) as before."""
    lib, dev, cfg, sd, _, _ = _setup(kind, seed=7)
    M = cfg["ContentEncoder"]["c_in"]
    torch.save(sd, tmp_path / "m.ckpt")
    attr = {"mean": np.linspace(-1, 1, M).astype(np.float32), "std": np.linspace(0.5, 2, M).astype(np.float32)}
    with open(tmp_path / "attr.pkl", "wb") as f:
        pickle.dump(attr, f)
    args = types.SimpleNamespace(model=str(tmp_path / "m.ckpt"), attr=str(tmp_path / "attr.pkl"))
    inf = Inferencer(cfg, args, lib=lib if kind == "emu" else None)
    enrol = _utts([65, 17, 43], M, 1)
    e = inf.enroll(enrol)
    ref_e = torch.stack([O.speaker_encoder(u.t()[None], sd, cfg)[0] for u in enrol]).mean(0)
    assert e.shape == ref_e.shape and e.device.type == dev.type
    torch.testing.assert_close(e.cpu(), ref_e, **STRICT)
    T = [37, 64, 19, 31]
    srcs = _utts(T, M, 2)
    outs = inf.convert_batch(srcs, emb=e)
    assert len(outs) == len(srcs)
    for s, o, t in zip(srcs, outs, T):
        ref = O.decoder(O.content_encoder(s.t()[None], sd, cfg)[0], e.cpu()[None], sd, cfg)[0].t()
        assert o.shape == ref.shape and o.device.type == "cpu"
        torch.testing.assert_close(o, ref, msg=lambda m: f"source of {t} frames: {m}", **_tol(t))
    with pytest.raises(ValueError, match="source utterances alone"):
        inf.convert_batch([(srcs[0], enrol[0])], emb=e)
    # pairs: unchanged
    pairs = [(srcs[0], enrol[0]), (srcs[3], enrol[2])]
    for (s, t), o in zip(pairs, inf.convert_batch(pairs)):
        ref = O.ae_inference(s.t()[None], t.t()[None], sd, cfg)[0].t()
        torch.testing.assert_close(o, ref, **STRICT)


def test_command_line_parses_enrolment_options():
    """9 (parser level; no audio files).  A single -t yields what it always has: a string."""
    a = parse_args(["-c", "cfg.yaml", "-m", "m.ckpt", "-s", "src.wav", "-t", "tgt.wav", "-o", "out.wav"])
    assert a.target == "tgt.wav" and a.source == "src.wav" and a.output == "out.wav" and a.sample_rate == 24000
    assert a.save_emb is None and a.emb is None and a.config == "cfg.yaml" and a.model == "m.ckpt" and a.attr is None
    a = parse_args(["-s", "src.wav", "-t", "a.wav", "-target", "b.wav", "-t", "c.wav", "-save_emb", "voice.pt", "-o", "out.wav"])
    assert a.target == ["a.wav", "b.wav", "c.wav"] and a.save_emb == "voice.pt" and a.emb is None
    a = parse_args(["-s", "src.wav", "-emb", "voice.pt", "-o", "out.wav", "-sr", "16000"])
    assert a.target is None and a.emb == "voice.pt" and a.sample_rate == 16000
    a = parse_args(["-t", "a.wav", "-t", "b.wav", "-save_emb", "voice.pt"])   # enrolment only
    assert a.source is None and a.target == ["a.wav", "b.wav"]


@pytest.mark.parametrize("kind", KINDS)
def test_error_paths_say_what_to_pass(kind):
    """10. Neither / both arguments, an emb of the wrong shape, an emb that requires grad."""
    lib, dev, cfg, sd, _, _ = _setup(kind)
    M, C = cfg["ContentEncoder"]["c_in"], cfg["SpeakerEncoder"]["c_out"]
    model = _model(kind, lib, dev, cfg, sd)
    xs = [x.to(dev) for x in _utts([40, 33], M, 3)]
    cs = [x.to(dev) for x in _utts([29, 50], M, 4)]
    with pytest.raises(ValueError, match="exactly one of x_conds"):
        model.inference_ragged(xs)
    with pytest.raises(ValueError, match="exactly one of x_conds"):
        model.inference_ragged(xs, cs, emb=torch.zeros(2, C, device=dev))
    for shape in ((3, C), (2, C + 1), (C + 1,), (2, 1, C)):
        with pytest.raises(ValueError, match=rf"emb must be \[2, {C}\]"):
            model.inference_ragged(xs, emb=torch.zeros(*shape, device=dev))
    e = torch.zeros(C, device=dev, requires_grad=True)
    with pytest.raises(RuntimeError, match=r"forward-only.*decoder\(z, cond\)"):
        model.inference_ragged(xs, emb=e)
    with torch.no_grad():
        out = model.inference_ragged(xs, emb=e)          # nothing to lose without grad
    assert len(out) == 2 and not out[0].requires_grad
    plan = RaggedPlan(cfg, [40, 33], None, lib=lib, mode="emb")
    with pytest.raises(RuntimeError, match="forward_emb"):
        plan.forward(None, None, None, None)
    with pytest.raises(RuntimeError, match="mode 'emb'"):
        RaggedPlan(cfg, [40, 33], [29, 50], lib=lib).forward_emb(None, None, None, None)
    with pytest.raises(ValueError, match="mode must be one of"):
        RaggedPlan(cfg, [40, 33], [29, 50], lib=lib, mode="content")
