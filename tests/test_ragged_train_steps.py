"""``Solver.ae_step_ragged`` beyond its first step: what tests/test_ragged_train_step.py (one solver, one tuple of lengths, one step) cannot
see -- solver buffers sized by an earlier step, grad-plan workspaces that have been used, the 4-entry plan cache and table LRU evicting,
Adam's later steps, the hand-over of the packed weight images to ``ae_step`` -- and the tie of the packed-row loss to the pinned uniform
engine.  kind='emu': the CPU lane-level simulation on the tiny config; kind='gpu': the gfx950 library on the stock 80-mel config.

Length sets (lo = ``tests.test_ragged_random_configs._lo``: 16 tiny, 64 stock):
  A [17, 65, 66, 130]            the set of tests/test_ragged_train_step.py
  B [lo]                         N = 1 at the shortest legal utterance
  C [72, 72, 72]                 equal lengths, multiples of 8 (no crop tail), two 64-frame loss tiles
  D [lo, 57, 121, 57, 129, 200]  T % 8 == 1 (the 7-frame crop tail), a duplicated length, four loss tiles, N = 6; every solver buffer grows
  E [9, 130]                     a fifth tuple: the table LRU evicts (lo + 1 in place of 9 where lo > 9: the oracle's reflect padding)

1. set C: the ragged step IS the uniform step on [3, M, 72] (forward, both losses, every ReLU decision and L1 sign, every gradient tensor),
   and both losses are the pinned oracle's ``torch.mean`` over [B, M, T] / [B, c, Tz] in fp64;
2. A, D, B, C, E, A, A on ONE solver, every solver buffer NaN before each step: after every step bit-equal to a fresh solver that starts
   from the state before that step;
3. ``ae_step`` -> ``ae_step_ragged`` -> ``ae_step`` against a solver that repacks its weight images every step, and the converse;
4. sets B and D against ``tests.ragged_step_oracle.noisy_step_oracle`` at the bar of tests/test_ragged_train_step.py (b);
5. two cycles A, D, B, C, E: the live ``RaggedPlan`` objects and the allocated device memory do not grow."""
import functools
import gc
import weakref

import pytest
import torch

from adaptive_voice_conversion_amd import engine as engine_module
from oracle import avc_oracle as O
from tests.emu_util import KINDS, backend
from tests.ragged_oracle import content_masks, decoder_masks, speaker_masks
from tests.ragged_param_oracle import DEC, ENC, SPK, check, tensors
from tests.ragged_step_oracle import noisy_step_oracle
from tests.test_ragged_enroll import _utts
from tests.test_ragged_random_configs import _lo
from tests.test_ragged_train_step import LAMBDA_KL, _bits, _solver
from tests.test_submodules import rel

FWD = dict(rtol=1e-4, atol=2e-5)   # the forward tolerance
# test 1: one data seed and one noise seed per utterance of set C, found on the host by scanning seeds 1.. in the fp64 oracle (an utterance's
# decisions depend on its own data alone) for the margins the test asserts
C_SEEDS = {"emu": ((14, 32, 44), (1, 1, 3)), "gpu": ((72, 99, 101), (38, 27, 38))}
RELU_MARGIN = {"emu": 2e-5, "gpu": 4e-6}   # (those of oracle/make_golden.py: tiny, stock)


def _cfg(kind):
    return O.tiny_config() if kind == "emu" else O.stock_config(80)


def _sets(cfg):
    lo = _lo(cfg)
    return {"A": [17, 65, 66, 130], "B": [lo], "C": [72, 72, 72], "D": [lo, 57, 121, 57, 129, 200], "E": [9 if lo <= 9 else lo + 1, 130]}


def _n_lat(cfg, T):
    return cfg["ContentEncoder"]["c_out"] * sum(O.latent_len(cfg, t) for t in T)


def _eps(cfg, T, seed):
    return torch.randn(_n_lat(cfg, T), generator=torch.Generator().manual_seed(seed))


def _poison(s):
    """every solver-owned buffer NaN over its whole allocation: ae_step_ragged promises to write them before it reads them"""
    for b in s.__dict__.get("_rag_bufs", {}).values():
        b.fill_(float("nan"))


def _state(s):
    """parameters and optimizer state of a solver, copied"""
    return dict(p=s.model.flat_parameters().detach().clone(), m=s.opt.m.clone(), v=s.opt.v.clone(), vmax=s.opt.vmax.clone(), n=s.opt.step_count)


def _twin(kind, lib, cfg, sd, st):
    """a fresh solver that holds the parameters and the optimizer state ``st``"""
    t = _solver(kind, lib, cfg, sd)
    with torch.no_grad():
        t.model.flat_parameters().copy_(st["p"])
    t.model.weights_changed()
    for name in ("m", "v", "vmax"):
        getattr(t.opt, name).copy_(st[name])
    t.opt.step_count = st["n"]
    return t


def _assert_same_state(a, b, tag):
    sa, sb = _state(a), _state(b)
    assert sa["n"] == sb["n"], tag
    for k in ("p", "m", "v", "vmax"):
        assert torch.equal(_bits(sa[k]), _bits(sb[k])), f"{tag}: {k} differs from the fresh solver's"


def _engine_branch(cfg, s, xs):
    """(masks per utterance in the oracle's call order, sign(dec - x) per utterance, cropped dec blocks) of the solver's last ragged step"""
    (pe, ps, pd), (wse, wss, wsd), tab = s._rag_last
    assert list(tab.T) == [x.shape[0] for x in xs]
    ms, me, md = speaker_masks(ps, wss), content_masks(pe, wse, cfg), decoder_masks(pd, wsd, cfg)
    masks = [ms[b] + me[b] + md[b] for b in range(len(xs))]
    dec = [d.detach().cpu()[:, :x.shape[0]].clone() for d, x in zip(pd.outputs(wsd), xs)]
    return masks, [torch.sign(d - x.t()) for d, x in zip(dec, xs)], dec


def _against_oracle(kind, cfg, sd, s, xs, eps, lambda_kl, meta, grads, tag):
    """(b) of tests/test_ragged_train_step.py: every tensor of ``grads`` at the project's bar against noisy_step_oracle fp64 / fp32 on the
    engine's own branch, both losses against fp64 to rtol 1e-4.  Returns (engine tensors, fp64 tensors, fp32 tensors)."""
    (pe, ps, pd), _, tab = s._rag_last
    c = cfg["ContentEncoder"]["c_out"]
    eb = [eps[c * o:c * (o + t)].view(c, t) for t, o in zip(tab.Tz, [sum(tab.Tz[:i]) for i in range(tab.N)])]
    masks, signs, _ = _engine_branch(cfg, s, xs)
    lam_rec = cfg["lambda"]["lambda_rec"]
    r64, rec64, kl64 = noisy_step_oracle(cfg, sd, xs, eb, masks, signs, lam_rec, lambda_kl, torch.float64)
    r32, _, _ = noisy_step_oracle(cfg, sd, xs, eb, masks, signs, lam_rec, lambda_kl, torch.float32)
    got = tensors(pe, sd, grads, (SPK, ENC, DEC))
    assert len(got) == len(sd) == len(r64)   # no tensor is left out
    check(got, r64, r32, tag)
    err = (abs(meta["loss_rec"] - rec64) / abs(rec64), abs(meta["loss_kl"] - kl64) / abs(kl64))
    print(f"[{tag}] losses against the fp64 oracle: rel err {err[0]:.2e}, {err[1]:.2e}")
    assert max(err) <= 1e-4, (meta, rec64, kl64)
    return got, r64, r32


# ---- 1. equal lengths: the ragged step is the uniform step --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _equal_case(kind):
    """set C's data and its fp64 evaluation by the pinned oracle's ops on the [3, M, 72] batch (host only): utterances, eps [3, c, Tz], the
    two losses as the reference writes them, the oracle's ReLU margin and the worst |dec - x| in units of ten forward tolerances"""
    cfg = _cfg(kind)
    sd = O.make_state_dict(cfg, 21)
    M, c, Tz = cfg["ContentEncoder"]["c_in"], cfg["ContentEncoder"]["c_out"], O.latent_len(cfg, 72)
    xs = [_utts([72], M, seed)[0] for seed in C_SEEDS[kind][0]]
    eps = torch.stack([torch.randn(c * Tz, generator=torch.Generator().manual_seed(seed)).view(c, Tz) for seed in C_SEEDS[kind][1]])
    xb = torch.stack([x.t() for x in xs]).contiguous()
    x64, log = xb.double(), []
    with torch.no_grad(), O.relu_masks(None, log=log):
        mu, ls, emb, dec = O.ae_forward(x64, eps.double(), {k: v.double() for k, v in sd.items()}, cfg)
    rec64 = float(torch.mean(torch.abs(dec - x64)))                          # solver.py:84: the mean over [B, M, T]
    kl64 = float(0.5 * torch.mean(torch.exp(ls) + mu ** 2 - 1 - ls))         # solver.py:85: the mean over [B, c, Tz]
    relu_margin = min(float(p.abs().min()) for p in log)
    l1_margin = float(((dec - x64).abs() / (10 * (FWD["atol"] + FWD["rtol"] * dec.abs()))).min())
    return cfg, sd, xs, xb, eps, rec64, kl64, relu_margin, l1_margin, dec.float()


@pytest.mark.parametrize("kind", KINDS)
def test_equal_lengths_are_the_uniform_step(kind):
    """Set C through ``ae_step_ragged`` and, as a [3, M, 72] batch with the same eps viewed [3, c, Tz], through the uniform train plan the
    way ``ae_step`` drives it (forward, loss, backward; no optimizer step), on two solvers that hold the same state dict.

    The data seeds keep both engines on one branch BY MARGIN, asserted here in the fp64 oracle: every ReLU pre-activation at least 2e-5
    (tiny) / 4e-6 (stock) from 0 and every |dec - x| at least ten forward tolerances (atol 2e-5 + rtol 1e-4 |dec|) from 0.  Seeds (data /
    noise, per utterance) and the margins found: tiny (14, 32, 44) / (1, 1, 3): closest pre-activation 2.98e-5, closest |dec - x| 1.5 x ten
    tolerances; stock (72, 99, 101) / (38, 27, 38): 4.84e-6 and 1.16 x.  A decision that differs between the engines means: change the seed."""
    lib, dev = backend(kind)
    cfg, sd, xs, xb, eps, rec64, kl64, relu_margin, l1_margin, dec64 = _equal_case(kind)
    print(f"[{kind}] fp64 oracle: closest ReLU pre-activation {relu_margin:.3e}, closest |dec - x| {l1_margin:.3f} x ten forward tolerances")
    assert relu_margin >= RELU_MARGIN[kind], f"a ReLU pre-activation {relu_margin:.2e} from 0 in the fp64 oracle: change the seed"
    assert l1_margin >= 1.0, f"a |dec - x| at {l1_margin:.2f} of ten forward tolerances in the fp64 oracle: change the seed"
    M, c = cfg["ContentEncoder"]["c_in"], cfg["ContentEncoder"]["c_out"]
    lam_rec = cfg["lambda"]["lambda_rec"]
    # the ragged engine
    sr = _solver(kind, lib, cfg, sd)
    meta_r = sr.ae_step_ragged([x.to(dev) for x in xs], LAMBDA_KL, eps=eps.reshape(-1).to(dev), apply=False)
    g_r = sr.model.flat_grads().detach().clone()
    masks_r, signs_r, dec_r = _engine_branch(cfg, sr, xs)
    pd = sr._rag_last[0][2]
    assert list(pd.out_len) == [72, 72, 72]   # no crop tail
    # the uniform engine
    su = _solver(kind, lib, cfg, sd)
    model = su.model
    flat, grads = model.flat_parameters(), model.flat_grads()
    plan, ws = model._plan(3, 72, 72, dev)
    assert (plan.latent_len, plan.out_len) == (eps.shape[2], 72)
    xd, ed = xb.to(dev), eps.to(dev)
    plan.forward(flat, xd, None, ed, ws)
    plan.loss(xd, lam_rec, ws)
    plan.backward(flat, xd, None, ed, grads, ws, lambda_kl=LAMBDA_KL)
    loss_u = plan.view(ws, "losses", (2,)).tolist()
    dec_u = plan.view(ws, "dec", (3, M, 72)).detach().cpu().clone()
    masks_u = [m.cpu() for m in plan.relu_masks(ws)]
    g_u = grads.detach().clone()
    # forward and losses
    torch.testing.assert_close(torch.stack(dec_r), dec_u, **FWD)
    torch.testing.assert_close(dec_u, dec64, **FWD)
    loss_r = [meta_r["loss_rec"], meta_r["loss_kl"]]
    err = [abs(a - b) / abs(b) for a, b in ((loss_r[0], loss_u[0]), (loss_r[1], loss_u[1]), (loss_r[0], rec64), (loss_r[1], kl64),
                                            (loss_u[0], rec64), (loss_u[1], kl64))]
    print(f"[{kind}] losses ragged {loss_r}, uniform {loss_u}, fp64 {[rec64, kl64]}: rel err ragged/uniform {max(err[:2]):.2e}, "
          f"ragged/fp64 {max(err[2:4]):.2e}, uniform/fp64 {max(err[4:]):.2e}")
    assert max(err) <= 1e-4, err
    # one branch
    assert all(len(m) == len(masks_u) for m in masks_r)
    flips = sum(int((masks_r[b][i].reshape(mu[b].shape) != mu[b]).sum()) for b in range(3) for i, mu in enumerate(masks_u))
    assert flips == 0, f"{flips} ReLU decisions differ between the ragged and the uniform engine: change the seed"
    signs_u = torch.sign(dec_u - xb)
    flips = int((torch.stack(signs_r) != signs_u).sum())
    assert flips == 0 and bool((signs_u != 0).all()), f"{flips} L1 signs differ between the ragged and the uniform engine: change the seed"
    # gradients: the ragged engine at the project's bar, the two engines within the triangle inequality over that bar
    got_r, r64, r32 = _against_oracle(kind, cfg, sd, sr, xs, eps.reshape(-1), LAMBDA_KL, meta_r, g_r, f"{kind} set C, ragged")
    got_u = tensors(plan, sd, g_u, (SPK, ENC, DEC))
    assert set(got_u) == set(got_r) == set(sd)
    scale = sum(float(v.norm()) ** 2 for v in r64.values()) ** 0.5
    worst = (0.0, None, 0.0)
    for k, ref in r64.items():
        assert not torch.isnan(got_u[k]).any(), k
        d = float((got_r[k] - got_u[k]).norm())
        if float(ref.norm()) < 1e-6 * scale:   # (judged absolutely, as `check` does: twice its 1e-5 of the whole gradient)
            assert d < 2 * 1e-5 * scale, (k, d, scale)
            continue
        bar = 2 * max(1e-4, 2 * rel(r32[k], ref))
        e = d / float(ref.norm())
        if e / bar > worst[0]:
            worst = (e / bar, k, e)
        assert e <= bar, (k, e, bar)
    print(f"[{kind} set C, ragged - uniform] worst tensor {worst[1]}: rel-L2 {worst[2]:.3e} ({worst[0]:.2f} of its bar)")


# ---- 2. a sequence of length sets on one solver --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_sequence_of_length_sets_equals_fresh_solvers(kind):
    """A, D, B, C, E (apply=True), A, A (apply=False, one eps) on one solver whose ``_rag_bufs`` are NaN before every step; after each step
    gradients, losses, grad_norm, parameters and m / v / vmax are bit-equal to a fresh solver started from the state before that step.  Then
    one step with sync=False against the same step with sync=True."""
    lib, dev = backend(kind)
    cfg = _cfg(kind)
    sd = O.make_state_dict(cfg, 21)
    M, sets = cfg["ContentEncoder"]["c_in"], _sets(cfg)
    data = {k: [x.to(dev) for x in _utts(T, M, 30 + i)] for i, (k, T) in enumerate(sets.items())}
    #        set, lambda_kl, eps seed, apply
    steps = [("A", 0.5, 11, True), ("D", 0.25, 12, True), ("B", 1.0, 13, True), ("C", 0.125, 14, True), ("E", 0.75, 15, True),
             ("A", 0.375, 16, False), ("A", 0.375, 16, False)]
    s = _solver(kind, lib, cfg, sd)
    kept = []
    for i, (name, lam, seed, apply) in enumerate(steps):
        tag = f"{kind} step {i} (set {name})"
        eps = _eps(cfg, sets[name], seed).to(dev)
        before = _state(s)
        _poison(s)
        meta = s.ae_step_ragged(data[name], lam, eps=eps, apply=apply)
        g = s.model.flat_grads().detach().clone()
        assert not torch.isnan(g).any() and not torch.isnan(s.model.flat_parameters()).any(), tag
        assert len(s._rag_tables) <= 4 and len(s.model._ragged) <= 4, tag
        t = _twin(kind, lib, cfg, sd, before)
        want = t.ae_step_ragged(data[name], lam, eps=eps, apply=apply)
        assert meta == want and set(meta) == ({"loss_rec", "loss_kl", "grad_norm"} if apply else {"loss_rec", "loss_kl"}), (tag, meta, want)
        assert torch.equal(_bits(g), _bits(t.model.flat_grads())), f"{tag}: gradients differ from the fresh solver's"
        _assert_same_state(s, t, tag)
        assert apply != torch.equal(_bits(before["p"]), _bits(s.model.flat_parameters())), tag   # (it stepped iff asked to)
        kept.append((meta, g))
        del t
    assert s.opt.step_count == 5
    assert kept[5][0] == kept[6][0] and torch.equal(_bits(kept[5][1]), _bits(kept[6][1]))   # used workspaces, rebuilt plans: the same bits
    # sync=False: the device scalars of an identical step
    name, lam, seed = "A", 0.625, 17
    eps = _eps(cfg, sets[name], seed).to(dev)
    before = _state(s)
    _poison(s)
    lazy = s.ae_step_ragged(data[name], lam, eps=eps, sync=False)
    assert set(lazy) == {"loss_rec", "loss_kl", "grad_norm"} and all(torch.is_tensor(v) and v.device.type == dev.type for v in lazy.values())
    lazy = {k: v.detach().cpu().clone() for k, v in lazy.items()}
    t = _twin(kind, lib, cfg, sd, before)
    want = t.ae_step_ragged(data[name], lam, eps=eps, sync=True)
    for k, v in want.items():
        assert torch.equal(_bits(lazy[k].reshape(1)), _bits(torch.tensor([v], dtype=torch.float32))), (k, float(lazy[k]), v)
    _assert_same_state(s, t, f"{kind} sync=False step")
    assert s.opt.step_count == 6


# ---- 3. hand-over between the two step functions -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_handover_between_the_two_step_functions(kind):
    """ae_step, ae_step_ragged(A, apply=True), ae_step on one solver: the third call equals, bit for bit, the same call on a solver with
    ``repack_every_step: true`` that starts from the state before it (weight images packed before the ragged step would show).  And
    ae_step, ae_step_ragged(A, apply=False): the gradients of a fresh solver that holds the same parameters."""
    lib, dev = backend(kind)
    cfg = _cfg(kind)
    sd = O.make_state_dict(cfg, 21)
    M, A = cfg["ContentEncoder"]["c_in"], _sets(cfg)["A"]
    x, eps_u = O.make_inputs(cfg, 2, 64 if kind == "emu" else 128, 4)
    x, eps_u = x.to(dev), eps_u.to(dev)
    utts = [u.to(dev) for u in _utts(A, M, 9)]
    eps_r = _eps(cfg, A, 5).to(dev)
    # uniform, ragged, uniform
    s = _solver(kind, lib, cfg, sd)
    first = s.ae_step(x, LAMBDA_KL, eps=eps_u)
    after_first = _state(s)
    s.ae_step_ragged(utts, LAMBDA_KL, eps=eps_r, apply=True)
    before_third = _state(s)
    assert before_third["n"] == 2 and not torch.equal(_bits(before_third["p"]), _bits(after_first["p"]))
    third = s.ae_step(x, LAMBDA_KL, eps=eps_u)
    r = _twin(kind, lib, dict(cfg, repack_every_step=True), sd, before_third)
    want = r.ae_step(x, LAMBDA_KL, eps=eps_u)
    assert third == want, (third, want)
    assert third != first
    _assert_same_state(s, r, f"{kind} third call")
    assert s.opt.step_count == 3
    del s, r
    # the converse: a ragged step behind a uniform one reads the parameters of now
    s = _solver(kind, lib, cfg, sd)
    assert s.ae_step(x, LAMBDA_KL, eps=eps_u) == first
    s.ae_step_ragged(utts, LAMBDA_KL, eps=eps_r, apply=False)
    t = _twin(kind, lib, cfg, sd, after_first)
    t.ae_step_ragged(utts, LAMBDA_KL, eps=eps_r, apply=False)
    assert torch.equal(_bits(s.model.flat_grads()), _bits(t.model.flat_grads())), "ae_step_ragged behind ae_step: gradients differ from a fresh solver's"
    _assert_same_state(s, t, f"{kind} apply=False")


# ---- 4. edge length sets against the oracle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["B", "D"])
@pytest.mark.parametrize("kind", KINDS)
def test_edge_length_sets_against_the_oracle(kind, name):
    lib, dev = backend(kind)
    cfg = _cfg(kind)
    sd = O.make_state_dict(cfg, 21)
    T = _sets(cfg)[name]
    xs = _utts(T, cfg["ContentEncoder"]["c_in"], 9)
    if name == "D":
        assert T[1] == T[3] == 57 and not torch.equal(xs[1], xs[3])   # the duplicated length, different data
    eps = _eps(cfg, T, 5)
    s = _solver(kind, lib, cfg, sd)
    meta = s.ae_step_ragged([x.to(dev) for x in xs], LAMBDA_KL, eps=eps.to(dev), apply=False)
    _against_oracle(kind, cfg, sd, s, xs, eps, LAMBDA_KL, meta, s.model.flat_grads().detach().clone(), f"{kind} set {name} {T}")


# ---- 5. plans and memory do not accumulate -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_plans_and_memory_do_not_accumulate(kind, monkeypatch):
    """The cycle A, D, B, C, E twice on one solver (apply=False, drawn noise): the RaggedPlan objects alive after each cycle -- weak
    references taken in the constructor -- are equally many and at most 4 (the AE's cache) + 3 (``_rag_last``); on the GPU the second cycle
    leaves no more device memory allocated than the first."""
    lib, dev = backend(kind)
    cfg = _cfg(kind)
    sd = O.make_state_dict(cfg, 21)
    M, sets = cfg["ContentEncoder"]["c_in"], _sets(cfg)
    born, init = [], engine_module.RaggedPlan.__init__

    def counted(self, *a, **kw):
        init(self, *a, **kw)
        born.append(weakref.ref(self))
    monkeypatch.setattr(engine_module.RaggedPlan, "__init__", counted)
    s = _solver(kind, lib, cfg, sd)
    data = {k: [x.to(dev) for x in _utts(T, M, 30 + i)] for i, (k, T) in enumerate(sets.items())}
    live, mem = [], []
    for cycle in range(2):
        for name in "ADBCE":
            meta = s.ae_step_ragged(data[name], LAMBDA_KL, apply=False)
            assert all(v == v and abs(v) != float("inf") for v in meta.values()), (cycle, name, meta)
            assert len(s._rag_tables) <= 4 and len(s.model._ragged) <= 4
        gc.collect()
        live.append(sum(r() is not None for r in born))
        if dev.type == "cuda":
            torch.cuda.synchronize(dev)
            mem.append(torch.cuda.memory_allocated(dev))
    print(f"[{kind}] RaggedPlan objects created {len(born)}, alive after each cycle {live}; device bytes allocated after each cycle {mem}")
    assert len(born) >= 15   # (the wrapped constructor saw the plans of every set)
    assert live[0] == live[1] and live[1] <= 4 + 3, live
    if mem:
        assert mem[1] <= mem[0], mem
