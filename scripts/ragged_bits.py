"""Fingerprint of every kind of ragged plan under ONE build of the library: the plan's sizes, the offsets of its named buffers, its
output / latent tables, and a SHA-256 of the whole workspace after each pass from seeded inputs into a zeroed workspace.  Two builds that
lay the workspace out alike and launch the same arithmetic in the same order write identical files (fp32 plans are bit-reproducible,
DESIGN 6), so `cmp` of two outputs is the check a host-side refactor of the planning / launching code has to pass.

  python scripts/ragged_bits.py --lib path/to/libavc_hip.so --config tiny,stock80 --out new.json     (an MI355X)
  python scripts/ragged_bits.py --emu path/to/libavc_emu.so --out new.json                            (the CPU lane-level simulation)
"""
import argparse
import ctypes
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LENGTHS = [17, 64, 65, 129]   # inside one 64-frame column tile, exactly one, one frame into the second, one frame into the third
NAMES = ["emb", "muls", "dec", "cond", "d_x_cond", "d_x", "d_z", "d_emb", "d_cond", "spk_cat", "spk_h0", "enc_cat", "enc_y0", "enc_st0",
         "dec_y0", "dec_st0"]
PER_LEVEL = ["spk_a1", "spk_a2", "spk_d1", "spk_d2", "enc_y1", "enc_y2", "enc_st1", "enc_st2", "dec_y1", "dec_a1", "dec_y2", "dec_st1", "dec_st2"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="the gfx950 library to run under (default: AVC_HIP_LIB, or the package's own)")
    ap.add_argument("--emu", default=None, help="run on the CPU under this build of the lane-level simulation instead")
    ap.add_argument("--config", default="tiny", help="comma-separated: tiny (tests/test_ragged_enroll.py::_setup), stock80")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.lib:
        os.environ["AVC_HIP_LIB"] = a.lib
    import torch
    from adaptive_voice_conversion_amd import _lib
    from adaptive_voice_conversion_amd.engine import RaggedPlan
    from oracle import avc_oracle as O
    lib, dev = (_lib.declare(ctypes.CDLL(a.emu)), torch.device("cpu")) if a.emu else (_lib.load(), torch.device("cuda", 0))

    def rnd(n, seed, scale=1.0):
        return (torch.randn(n, generator=torch.Generator().manual_seed(seed)) * scale).to(dev)

    def run(cfg, mode, T, Tc=None, **kw):
        plan = RaggedPlan(cfg, T, Tc, lib=lib, mode=mode, **kw)
        r = {"workspace_floats": plan.workspace_floats, "param_floats": plan.param_floats, "buffers": {},
             "out_len": plan.out_len, "out_off": plan.out_off, "lat_len": plan.lat_len, "lat_off": plan.lat_off}
        for name in NAMES + [f"{n}_{l}" for n in PER_LEVEL for l in range(8)]:
            try:
                r["buffers"][name] = plan.buffer(name)
            except KeyError:
                pass
        params = rnd(plan.param_floats, 1, 0.05)
        ws = torch.zeros(plan.workspace_floats, device=dev)
        M, N = plan.n_mels, plan.N
        x, xc = rnd(sum(plan.T) * M, 2).view(sum(plan.T), M), rnd(sum(plan.T_cond) * M, 3).view(sum(plan.T_cond), M)
        emb, z = rnd(N * plan.c_emb, 4).view(N, plan.c_emb), rnd(plan.c_lat * sum(plan.T), 5)

        def digest(what):
            if dev.type == "cuda":
                torch.cuda.synchronize()
            r["sha256_" + what] = hashlib.sha256(ws.cpu().numpy().tobytes()).hexdigest()

        grads = torch.zeros(plan.param_floats, device=dev) if mode in ("encode_pg", "decode_pg") else None
        if mode in ("decode", "decode_ig", "decode_pg"):
            plan.forward_latents(params, z, plan.c_lat, emb, ws)
        elif mode in ("emb", "fanout"):
            plan.forward_emb(params, x, emb, ws)
        else:
            plan.forward(params, x if plan.T else None, xc if mode in ("pairs", "speaker") else None, ws)
        digest("forward")
        if mode == "speaker" and plan.input_grads:
            plan.backward(params, xc, rnd(plan.B * plan.c_emb, 6).view(plan.B, plan.c_emb), ws)
        elif mode == "encode" and plan.input_grads:
            plan.backward_content(params, x, rnd(2 * plan.c_lat * sum(plan.lat_len), 7), ws)
        elif mode == "decode_ig":
            plan.backward_decoder(params, z, plan.c_lat, emb, rnd(M * sum(plan.out_len), 8), ws)
        elif mode == "encode_pg":
            plan.backward_content_params(params, x, rnd(2 * plan.c_lat * sum(plan.lat_len), 7), grads, ws)
        elif mode == "decode_pg":
            plan.backward_decoder_params(params, z, plan.c_lat, emb, rnd(M * sum(plan.out_len), 8), grads, ws)
        else:
            return r
        digest("backward")
        if grads is not None:   # (the parameter-gradient kinds: the flat gradient buffer too)
            r["sha256_grads"] = hashlib.sha256(grads.cpu().numpy().tobytes()).hexdigest()
        return r

    res = {}
    for name in a.config.split(","):
        cfg = O.tiny_config() if name == "tiny" else O.stock_config(80)
        T, Tz = LENGTHS, list(LENGTHS)
        for s in list(cfg["ContentEncoder"]["subsample"])[:cfg["ContentEncoder"]["n_conv_blocks"]]:
            Tz = [(t + s - 1) // s for t in Tz]   # the latent lengths of sources of those lengths
        src_of = [3, 0, 0, 2, 1, 3]
        res[name] = {
            "pairs": run(cfg, "pairs", T, T[::-1]),
            "speaker": run(cfg, "speaker", None, T),
            "speaker_ig": run(cfg, "speaker", None, T, input_grads=True),
            "emb": run(cfg, "emb", T),
            "fanout": run(cfg, "fanout", T, src_of=src_of),
            "encode": run(cfg, "encode", T),
            "encode_ig": run(cfg, "encode", T, input_grads=True),
            "decode": run(cfg, "decode", Tz, src_of=src_of),
            "decode_ig": run(cfg, "decode_ig", Tz),
        }
        if hasattr(lib, "avc_plan_create_ragged_content_param_grads"):   # (absent from older builds: their nine kinds compare as they are)
            res[name]["encode_pg"] = run(cfg, "encode_pg", T)
            res[name]["decode_pg"] = run(cfg, "decode_pg", Tz)
    text = json.dumps(res, indent=1, sort_keys=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(hashlib.sha256(text.encode()).hexdigest(), a.out or "")


if __name__ == "__main__":
    main()
