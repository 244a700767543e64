"""One rank of the two-rank ragged step tests (tests/test_ragged_dist_gloo.py); no tests in this module.

    python tests/ragged_dist_worker.py <kind> <rank> <world> <port> <out_dir>

Global lengths [17, 65, 66, 130]; rank r takes utterances r, r + W, ... with their blocks of one fixed eps.  One step with apply=False
(gradients, losses and -- for the oracle on the engine's own branch -- the ReLU masks and L1 signs of this rank's utterances are saved),
then two steps with apply=True (parameters saved).  kind 'emu': the CPU simulation on the tiny config; 'gpu': gfx950, both ranks on GPU 0."""
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

T_UTT = [17, 65, 66, 130]
LAMBDA_KL = 0.5


def setup(kind):
    """(config, state dict, the four utterances, their eps blocks [c][Tz_j]) -- the same on every rank and in the parent"""
    from oracle import avc_oracle as O
    cfg = O.tiny_config() if kind == "emu" else O.stock_config(80)
    sd = O.make_state_dict(cfg, 21)
    g = torch.Generator().manual_seed(9)
    xs = [torch.randn(t, cfg["ContentEncoder"]["c_in"], generator=g) for t in T_UTT]
    c = cfg["ContentEncoder"]["c_out"]
    g = torch.Generator().manual_seed(5)
    eps = [torch.randn(c, O.latent_len(cfg, t), generator=g) for t in T_UTT]
    return cfg, sd, xs, eps


def main(kind, rank, world, port, out_dir):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from adaptive_voice_conversion_amd.device_feed import PackedUtterances
    from adaptive_voice_conversion_amd.solver import Solver
    from tests.emu_util import backend
    from tests.ragged_oracle import content_masks, decoder_masks, speaker_masks
    lib, dev = backend(kind)
    cfg, sd, xs, eps = setup(kind)
    args = types.SimpleNamespace(store_model_path=None, load_model=False, data_dir=None, logdir=out_dir)
    s = Solver(cfg, args, lib=lib if kind == "emu" else None)
    s.model.load_state_dict(sd)
    mine = list(range(rank, len(T_UTT), world))
    pk = PackedUtterances(torch.cat([xs[j] for j in mine]).to(dev), [T_UTT[j] for j in mine], T_UTT)
    e = torch.cat([eps[j].reshape(-1) for j in mine]).to(dev)
    meta = s.ae_step_ragged(pk, LAMBDA_KL, eps=e, apply=False)
    out = {"meta": meta, "grads": s.model.flat_grads().detach().cpu().clone(), "mine": mine}
    if kind == "emu":
        (pe, ps, pd), (wse, wss, wsd), tab = s._rag_last
        ms, me, md = speaker_masks(ps, wss), content_masks(pe, wse, cfg), decoder_masks(pd, wsd, cfg)
        out["masks"] = [ms[b] + me[b] + md[b] for b in range(len(mine))]
        out["signs"] = [torch.sign(d.detach().cpu()[:, :T_UTT[j]] - xs[j].t()) for d, j in zip(pd.outputs(wsd), mine)]
    out["steps"] = [s.ae_step_ragged(pk, LAMBDA_KL, eps=e) for _ in range(2)]
    out["params"] = s.model.flat_parameters().detach().cpu().clone()
    torch.save(out, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), sys.argv[5])
