"""``RaggedUtteranceFeed`` (device_feed.py) and the ragged step fed by it.

(1) feed: every block of a batch is the host slice ``data[utt][s : s + T_j]`` bit for bit, with the draws reproduced here from the same
    seed by the rule the class documents; the K templates are fixed, distinct, span the kept lengths; utterances below ``min_frames`` are
    never drawn; two ranks interleave to the single-process draw; equal seeds give equal batches, different seeds different ones.
(2) ``Solver.ae_step_ragged(PackedUtterances)``, one process: gradients and losses bit-equal to the list call on the same rows; over a
    loop of 12 steps on K = 3 templates with the caches raised as ``train_ragged`` raises them the plan objects of a template are the same
    on every visit and device memory stops growing once every template was seen; with the default cache the parameters end bit-equal.
(3) ``train_ragged`` and ``main.py --ragged_feed`` on a tiny pickle (CPU simulation only).

kind='emu': the CPU lane-level simulation on the tiny config; kind='gpu': the gfx950 library on the stock 80-mel config."""
import math
import pickle
import types

import numpy as np
import pytest
import torch
import yaml

from adaptive_voice_conversion_amd.device_feed import PackedUtterances, RaggedUtteranceFeed
from adaptive_voice_conversion_amd.solver import Solver
from oracle import avc_oracle as O
from tests.emu_util import KINDS, backend
from tests.test_ragged_enroll import _utts

T_UTT = [17, 65, 66, 130]
LAMBDA_KL = 0.5
# 14 utterances; "short_a" / "short_b" are below min_frames = 17, "long" is cropped by max_frames = 90
CORPUS_LENS = {"a": 40, "short_a": 5, "b": 17, "c": 90, "d": 33, "long": 140, "e": 64, "f": 65, "short_b": 16, "g": 23, "h": 77, "i": 51,
               "j": 18, "k": 29}
MIN_FRAMES, MAX_FRAMES = 17, 90


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _corpus(M, seed=11):
    g = torch.Generator().manual_seed(seed)
    return {k: torch.randn(n, M, generator=g).numpy() for k, n in CORPUS_LENS.items()}


def _mels(kind):
    return 16 if kind == "emu" else 80


def _feed(kind, data, N, K, seed=3, rank=0, world=1, max_frames=MAX_FRAMES):
    lib, dev = backend(kind)
    return RaggedUtteranceFeed(data, N, dev, n_templates=K, min_frames=MIN_FRAMES, max_frames=max_frames, seed=seed, rank=rank, world_size=world,
                               lib=lib if kind == "emu" else None)


def _host_templates(N, K, W):
    """the documented rule, restated: kept lengths clipped and sorted, slot i at index round(i (U - 1) / (S - 1)), template i % K"""
    L = sorted(min(n, MAX_FRAMES) for n in CORPUS_LENS.values() if n >= MIN_FRAMES)
    U, S = len(L), K * N * W
    slots = [L[int(math.floor(i * (U - 1) / (S - 1) + 0.5))] for i in range(S)]
    return [tuple(slots[k::K]) for k in range(K)]


class _HostDraws:
    """the documented draws, restated on the host: randint(K), then rand(2, N W) in float64"""

    def __init__(self, N, K, W, seed):
        self.templates = _host_templates(N, K, W)
        self.kept = sorted((k for k, n in CORPUS_LENS.items() if n >= MIN_FRAMES), key=lambda k: CORPUS_LENS[k])   # (stable)
        self.gen = torch.Generator().manual_seed(seed)
        self.K = K

    def __next__(self):
        k = int(torch.randint(self.K, (1,), generator=self.gen))
        t = self.templates[k]
        uv = torch.rand(2, len(t), dtype=torch.float64, generator=self.gen)
        picks = []
        for p, slot in enumerate(t):
            cand = [u for u in self.kept if CORPUS_LENS[u] >= slot]
            u = cand[int(float(uv[0, p]) * len(cand))]
            picks.append((u, int(float(uv[1, p]) * (CORPUS_LENS[u] - slot + 1)), slot))
        return k, picks


@pytest.mark.parametrize("kind", KINDS)
def test_blocks_are_the_host_slices_and_templates_are_fixed(kind):
    N, K = 3, 4
    data = _corpus(_mels(kind))
    feed, host = _feed(kind, data, N, K), _HostDraws(N, K, 1, 3)
    assert [tuple(t) for t in feed.templates] == host.templates and len(set(host.templates)) == K
    kept = [n for n in CORPUS_LENS.values() if n >= MIN_FRAMES]
    assert min(min(t) for t in feed.templates) == min(kept) == 17
    assert max(max(t) for t in feed.templates) <= MAX_FRAMES
    seen = set()
    for _ in range(10):
        pk = next(feed)
        k, picks = next(host)
        assert isinstance(pk, PackedUtterances) and pk.T == pk.global_T == host.templates[k]
        assert tuple(pk.x.shape) == (sum(pk.T), _mels(kind)) and pk.x.dtype == torch.float32
        x = pk.x.cpu()
        row = 0
        for u, s, t in picks:
            assert CORPUS_LENS[u] >= MIN_FRAMES and s + t <= CORPUS_LENS[u]
            assert torch.equal(_bits(x[row:row + t]), _bits(torch.from_numpy(data[u][s:s + t]))), (u, s, t)
            row += t
            seen.add(u)
    assert "long" in seen or len(seen) > 4   # (the draws move over the corpus)
    assert not seen & {"short_a", "short_b"}
    with pytest.raises(ValueError, match="min_frames"):
        RaggedUtteranceFeed({"x": data["short_a"]}, 2, backend(kind)[1], lib=backend(kind)[0] if kind == "emu" else None)


@pytest.mark.parametrize("kind", KINDS)
def test_two_ranks_interleave_to_the_single_process_draw(kind):
    N, K = 2, 3
    data = _corpus(_mels(kind))
    one = _feed(kind, data, 2 * N, K)
    r0, r1 = _feed(kind, data, N, K, rank=0, world=2), _feed(kind, data, N, K, rank=1, world=2)
    assert one.templates == r0.templates == r1.templates
    for _ in range(6):
        g, a, b = next(one), next(r0), next(r1)
        assert a.global_T == b.global_T == g.global_T == g.T
        assert a.T == g.T[0::2] and b.T == g.T[1::2]
        blocks = torch.split(g.x.cpu(), list(g.T))
        assert torch.equal(_bits(a.x), _bits(torch.cat(blocks[0::2]))) and torch.equal(_bits(b.x), _bits(torch.cat(blocks[1::2])))


@pytest.mark.parametrize("kind", KINDS)
def test_seeds(kind):
    data = _corpus(_mels(kind))
    a, b, c = _feed(kind, data, 3, 2, seed=5), _feed(kind, data, 3, 2, seed=5), _feed(kind, data, 3, 2, seed=6)
    same, other = True, True
    for _ in range(4):
        pa, pb, pc = next(a), next(b), next(c)
        same &= pa.T == pb.T and torch.equal(_bits(pa.x), _bits(pb.x))
        other &= pa.T == pc.T and torch.equal(_bits(pa.x), _bits(pc.x))
    assert same and not other


# ---- the step fed by packed rows ---------------------------------------------------------------------------------------------------------
def _solver(kind, cfg, sd, tmp=None, **args):
    lib, _ = backend(kind)
    a = types.SimpleNamespace(store_model_path=None, load_model=False, data_dir=None, logdir="/tmp/avc_ragged_feed_log", **args)
    s = Solver(cfg, a, lib=lib if kind == "emu" else None)
    s.model.load_state_dict(sd)
    return s


def _cfg(kind):
    cfg = O.tiny_config() if kind == "emu" else O.stock_config(80)
    return cfg, O.make_state_dict(cfg, 21)


@pytest.mark.parametrize("kind", KINDS)
def test_packed_step_is_bit_equal_to_the_list_step(kind):
    _, dev = backend(kind)
    cfg, sd = _cfg(kind)
    xs = [x.to(dev) for x in _utts(T_UTT, cfg["ContentEncoder"]["c_in"], 9)]
    Tz = [O.latent_len(cfg, t) for t in T_UTT]
    eps = torch.randn(cfg["ContentEncoder"]["c_out"] * sum(Tz), generator=torch.Generator().manual_seed(5)).to(dev)
    a, b = _solver(kind, cfg, sd), _solver(kind, cfg, sd)
    ma = a.ae_step_ragged(xs, LAMBDA_KL, eps=eps, apply=False)
    mb = b.ae_step_ragged(PackedUtterances(torch.cat(xs), T_UTT), LAMBDA_KL, eps=eps, apply=False)
    assert ma == mb and set(mb) == {"loss_rec", "loss_kl"}
    assert torch.equal(_bits(a.model.flat_grads()), _bits(b.model.flat_grads()))
    assert float(a.model.flat_grads().abs().sum()) > 0
    with pytest.raises(ValueError, match="packed"):
        b.ae_step_ragged(PackedUtterances(torch.cat(xs)[:-1], T_UTT), LAMBDA_KL)
    with pytest.raises(ValueError, match="contiguous fp32"):
        b.ae_step_ragged(PackedUtterances(torch.cat(xs).double(), T_UTT), LAMBDA_KL)


def _device_bytes(s, dev):
    """device memory in use: the allocator's count on the GPU; on the CPU, every buffer the step can create -- the plans' workspaces, the
    pooled one, the solver's own buffers and tables"""
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
        return torch.cuda.memory_allocated(dev)
    n = sum(b.numel() for b in s._rag_bufs.values()) + sum(e.ws.numel() for _, e in s.model._ragged.values() if e is not None)
    return 4 * n + 1000 * len(s._rag_tables) + 1000 * len(s.model._ragged)


def _loop(kind, raise_caches, steps=12, K=3):
    _, dev = backend(kind)
    cfg, sd = _cfg(kind)
    torch.manual_seed(1234)   # (the solver's noise generator is seeded from it)
    s = _solver(kind, cfg, sd)
    feed = _feed(kind, _corpus(cfg["ContentEncoder"]["c_in"]), 2, K, seed=8, max_frames=40)   # (short crops: the simulator's time goes with the frames)
    if raise_caches:
        s.model.set_ragged_plan_cache(3 * K + 1)
        s._rag_tables_cap = K
    first, mem, visits = {}, [], []
    for i in range(steps):
        pk = next(feed)
        k = feed.last_draw[0]
        meta = s.ae_step_ragged(pk, LAMBDA_KL)
        assert math.isfinite(meta["loss_rec"]) and math.isfinite(meta["loss_kl"]) and math.isfinite(meta["grad_norm"])
        plans = s._rag_last[0]
        ids = tuple(id(p) for p in plans)
        if raise_caches:
            first.setdefault(k, (ids, plans))   # (the plans are held: an id cannot be reused by a new object)
            assert first[k][0] == ids, f"step {i}: template {k} got new plan objects"
        visits.append(k)
        mem.append(_device_bytes(s, dev))
    return s, visits, mem


@pytest.mark.parametrize("kind", KINDS)
def test_loop_over_templates_reuses_plans_and_memory(kind):
    K = 3
    s, visits, mem = _loop(kind, True)
    assert set(visits) == set(range(K)), visits
    last_first = max(visits.index(k) for k in range(K))
    assert last_first < len(visits) - 1 and len(visits) > len(set(visits))
    assert mem[-1] == mem[last_first], (mem, visits)
    # (two templates whose lengths halve to the same latent lengths share their decoder plan: at most 3 K plans)
    assert 2 * K < len(s.model._ragged) <= 3 * K and len(s._rag_tables) == K
    # the default cache of 4: plans are created over and over, the numbers are the same
    d, visits_d, _ = _loop(kind, False)
    assert visits_d == visits and len(d.model._ragged) <= 4
    assert torch.equal(_bits(d.model.flat_parameters()), _bits(s.model.flat_parameters()))


# ---- loop and command line (CPU simulation) ----------------------------------------------------------------------------------------------
def _tiny_pickle(tmp_path, M):
    g = torch.Generator().manual_seed(2)
    lens = [17, 90, 33, 48, 21, 64, 75, 29, 56, 83, 40, 19]
    data = {f"u{i}": torch.randn(n, M, generator=g).numpy().astype(np.float32) for i, n in enumerate(lens)}
    with open(tmp_path / "train.pkl", "wb") as f:
        pickle.dump(data, f)


def test_train_ragged_saves_a_checkpoint_that_loads(tmp_path, capsys):
    lib, dev = backend("emu")
    cfg = O.tiny_config()
    cfg["data_loader"]["batch_size"] = 2
    _tiny_pickle(tmp_path, cfg["ContentEncoder"]["c_in"])
    args = types.SimpleNamespace(store_model_path=str(tmp_path / "model"), load_model=False, data_dir=str(tmp_path), train_set="train",
                                 logdir=str(tmp_path), ragged_feed=True, ragged_templates=2, ragged_min_frames=17, ragged_max_frames=40,
                                 summary_steps=1, save_steps=3, tag="t")
    s = Solver(cfg, args, lib=lib)
    before = s.model.flat_parameters().clone()
    s.train_ragged(6)
    assert s.opt.step_count == 6 and s.model._ragged_cap == 7 and s._rag_tables_cap == 4
    out = capsys.readouterr().out
    assert "AE:[6/6]" in out and "nan" not in out.lower() and "inf" not in out.lower()
    assert not torch.equal(before, s.model.flat_parameters())
    args2 = types.SimpleNamespace(**{**vars(args), "load_model": True, "load_model_path": str(tmp_path / "model"), "data_dir": None,
                                     "store_model_path": None})
    again = Solver(cfg, args2, lib=lib)
    assert torch.equal(_bits(again.model.flat_parameters()), _bits(s.model.flat_parameters()))
    assert again.opt.step_count == 6


def test_command_line_runs_train_ragged(tmp_path, capsys):
    from adaptive_voice_conversion_amd.main import main
    lib, _ = backend("emu")
    cfg = O.tiny_config()
    cfg["data_loader"]["batch_size"] = 2
    _tiny_pickle(tmp_path, cfg["ContentEncoder"]["c_in"])
    with open(tmp_path / "config.yaml", "w") as f:
        yaml.dump(cfg, f)
    main(["-c", str(tmp_path / "config.yaml"), "-d", str(tmp_path), "-train_set", "train", "-store_model_path", str(tmp_path / "cli"),
          "-logdir", str(tmp_path), "--ragged_feed", "-ragged_templates", "2", "-ragged_max_frames", "40", "-iters", "2"], lib=lib)
    assert "AE:[2/2]" in capsys.readouterr().out
    assert (tmp_path / "cli.ckpt").exists() and (tmp_path / "cli.opt").exists()
