"""``Solver.ae_step_ragged(PackedUtterances)`` with world_size 2 over gloo: global lengths [17, 65, 66, 130], rank 0 takes utterances 0
and 2, rank 1 takes 1 and 3 (tests/ragged_dist_worker.py).  Every rank divides by the GLOBAL counts, so the plain sum of the flat gradient
buffers is the gradient of the global means.

CPU simulation, tiny config: after one step with apply=False the ranks' gradient buffers are bit-identical and ALL tensors meet the bar of
``tests.ragged_param_oracle.check`` against ``noisy_step_oracle`` in fp64 on the four utterances as ONE batch (masks and signs from the
ranks' own workspaces); both ranks return the oracle's losses within 1e-4.  After two steps with apply=True the replicas are bit-identical
and equal the single-process list step on the four utterances by the criteria of tests/test_dist_gloo.py.

GPU, stock config: two processes share GPU 0; replicas bit-identical after two steps, the same grad_norm on both."""
import os
import subprocess
import sys
import types

import pytest
import torch

from tests.ragged_dist_worker import LAMBDA_KL, T_UTT, setup
from tests.test_dist_gloo import _free_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _two_ranks(kind, out_dir, limit):
    """both ranks as child processes, each under its own time limit; both exit codes must be 0"""
    port = _free_port()
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "ragged_dist_worker.py"), kind, str(r), "2", str(port), str(out_dir)],
                              cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    codes, logs = [], []
    for p in procs:
        try:
            logs.append(p.communicate(timeout=limit)[0])
        except subprocess.TimeoutExpired:
            p.kill()
            logs.append(p.communicate()[0])
        codes.append(p.returncode)
    assert codes == [0, 0], (codes, [l[-2000:] for l in logs])
    return [torch.load(os.path.join(out_dir, f"rank{r}.pt")) for r in range(2)]


def test_two_rank_ragged_step_is_the_global_batch_step(tmp_path):
    from adaptive_voice_conversion_amd.solver import Solver
    from tests.emu_util import backend, emu_lib
    from tests.ragged_param_oracle import DEC, ENC, SPK, check, tensors
    from tests.ragged_step_oracle import noisy_step_oracle
    emu_lib()   # (built here once if stale, not by both ranks)
    r0, r1 = _two_ranks("emu", tmp_path, 900)
    assert r0["mine"] == [0, 2] and r1["mine"] == [1, 3]
    assert torch.equal(r0["grads"].view(torch.int32), r1["grads"].view(torch.int32)), "the ranks hold different gradient sums"
    assert r0["meta"] == r1["meta"]
    cfg, sd, xs, eps = setup("emu")
    masks, signs = [None] * 4, [None] * 4
    for r in (r0, r1):
        for b, j in enumerate(r["mine"]):
            masks[j], signs[j] = r["masks"][b], r["signs"][b]
    lam_rec = cfg["lambda"]["lambda_rec"]
    r64, rec64, kl64 = noisy_step_oracle(cfg, sd, xs, eps, masks, signs, lam_rec, LAMBDA_KL, torch.float64)
    r32, _, _ = noisy_step_oracle(cfg, sd, xs, eps, masks, signs, lam_rec, LAMBDA_KL, torch.float32)
    lib, _ = backend("emu")
    args = types.SimpleNamespace(store_model_path=None, load_model=False, data_dir=None, logdir=str(tmp_path))
    s = Solver(cfg, args, lib=lib)
    s.model.load_state_dict(sd)
    got = tensors(types.SimpleNamespace(param_info=s.model._layout), sd, r0["grads"], (SPK, ENC, DEC))
    assert len(got) == len(sd) == len(r64)   # no tensor is left out (70 in the tiny config; the stock config has 166)
    check(got, r64, r32, f"two-rank ragged step, {len(r64)} tensors")
    err = (abs(r0["meta"]["loss_rec"] - rec64) / abs(rec64), abs(r0["meta"]["loss_kl"] - kl64) / abs(kl64))
    print(f"losses against the fp64 oracle: rel err {err[0]:.2e}, {err[1]:.2e}")
    assert max(err) <= 1e-4
    # two applied steps: identical replicas, and the single-process list step on the four utterances
    assert torch.equal(r0["params"].view(torch.int32), r1["params"].view(torch.int32)), "replicas diverged"
    assert r0["steps"][0]["grad_norm"] == r1["steps"][0]["grad_norm"]
    e = torch.cat([b.reshape(-1) for b in eps])
    m0 = s.ae_step_ragged(xs, LAMBDA_KL, eps=e)
    assert r0["steps"][0]["grad_norm"] == pytest.approx(m0["grad_norm"], rel=1e-5)
    assert r0["steps"][0]["loss_rec"] == pytest.approx(m0["loss_rec"], rel=1e-5)
    s.ae_step_ragged(xs, LAMBDA_KL, eps=e)
    diff = (s.model.flat_parameters() - r0["params"]).abs()
    assert (diff > 2e-6).float().mean().item() < 5e-3
    assert diff.max().item() <= 4.2 * cfg["optimizer"]["lr"]


@pytest.mark.gpu
def test_two_ranks_share_one_gpu(tmp_path):
    r0, r1 = _two_ranks("gpu", tmp_path, 120)
    assert torch.equal(r0["params"].view(torch.int32), r1["params"].view(torch.int32)), "replicas diverged"
    assert torch.equal(r0["grads"].view(torch.int32), r1["grads"].view(torch.int32))
    assert [m["grad_norm"] for m in r0["steps"]] == [m["grad_norm"] for m in r1["steps"]]
    assert r0["meta"] == r1["meta"] and T_UTT == [17, 65, 66, 130]
