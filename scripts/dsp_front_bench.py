"""A/B of the batched audio edges against the one-utterance-at-a-time loops they replace, on the GPU, in one process.

    python scripts/dsp_front_bench.py --parent-lib PATH/libavc_hip.so [--out profiles/dsp_front_bench.json] [--reps 12]

Workload: 32 synthetic utterances of 1 to 8 s (speech-like bursts with silent ends) at the stock hyper-parameters.
  front   MelDSP.get_spectrograms_batch(wavs)            vs   [get_spectrograms_device(w) for w in wavs] on the PARENT commit's library
  finish  MelDSP._finish_ragged(y, lengths, do_trim)     vs   [_finish(y_b, do_trim) for b] on the parent's library: the de-emphasis, trim and
          read-back behind Griffin-Lim in melspectrogram2wav_batch(do_trim=True, n_iter=0), on the waveforms that call produces
The two sides alternate, every repetition ends in a device synchronise, the first repetitions are discarded; median and spread (min,
max) per side in milliseconds.  Beside the times: library entry-point calls per batch (every one is at least one kernel launch; counted
by a proxy around the library) and host synchronisations per batch (the blocking device-to-host reads the code makes: counted by a
proxy around torch.Tensor.cpu).  The outputs of the two sides are compared bitwise before anything is timed.
"""
import argparse
import collections
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from adaptive_voice_conversion_amd import _lib, dsp as PD   # noqa: E402


class Counting:
    def __init__(self, lib):
        self._lib, self.calls = lib, collections.Counter()

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            self.calls[name] += 1
            return fn(*args)
        return call


def speechlike(n, sr, seed):
    r = np.random.RandomState(seed)
    t = np.arange(n) / sr
    f0 = 120 + 30 * np.sin(2 * np.pi * 0.7 * t)
    ph = 2 * np.pi * np.cumsum(f0) / sr
    y = sum(np.sin(k * ph) / k for k in range(1, 12))
    env = np.clip(np.sin(2 * np.pi * 1.3 * t), 0, None) ** 2
    return (0.3 * env * y + 0.002 * r.randn(n)).astype(np.float32)


def measure(sides, reps, warm=3):
    """sides: {name: fn}; alternates them; returns {name: {median_ms, min_ms, max_ms}}"""
    times = {k: [] for k in sides}
    for i in range(warm + reps):
        for k, fn in sides.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= warm:
                times[k].append(1e3 * (time.perf_counter() - t0))
    return {k: {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v))} for k, v in times.items()}


def counted(dsp, fn):
    """(entry-point calls, blocking device-to-host reads) of one call of fn"""
    dsp.lib.calls.clear()
    syncs = [0]
    cpu = torch.Tensor.cpu

    def counting_cpu(self, *a, **k):
        if self.is_cuda:
            syncs[0] += 1
        return cpu(self, *a, **k)
    torch.Tensor.cpu = counting_cpu
    try:
        fn()
    finally:
        torch.Tensor.cpu = cpu
    return int(sum(dsp.lib.calls.values())), syncs[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True, help="libavc_hip.so built from the parent commit")
    ap.add_argument("--out", default="profiles/dsp_front_bench.json")
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--utterances", type=int, default=32)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dsp_front_bench: needs the GPU")
    hp = PD.Hyperparams
    new = PD.MelDSP(hp, lib=Counting(_lib.load()))
    old = PD.MelDSP(hp, lib=Counting(_lib.declare(ctypes.CDLL(os.path.abspath(args.parent_lib)))))
    r = np.random.RandomState(0)
    secs = r.uniform(1.0, 8.0, args.utterances)
    wavs = [np.concatenate([np.zeros(3000, np.float32), speechlike(int(s * hp.sr), hp.sr, 100 + i), np.zeros(2500, np.float32)]) for i, s in enumerate(secs)]

    def front_new():
        return new.get_spectrograms_batch(wavs)

    def front_old():
        return [old.get_spectrograms_device(w)[0] for w in wavs]
    a, b = front_new(), front_old()
    assert all(torch.equal(x.view(torch.int32), z.view(torch.int32)) for x, z in zip(a, b)), "front ends differ"
    mels = [m.cpu() for m in a]
    Ts = [int(m.shape[0]) for m in mels]
    lengths = [hp.hop_length * (T - 1) for T in Ts]
    # the waveforms melspectrogram2wav_batch(n_iter=0) hands to its finish: Griffin-Lim without iterations on all frames
    amp = new._amplitudes(torch.cat(mels, dim=0))
    mag = new._matmul(new.mel_inv_w, amp)
    toff_h = np.ascontiguousarray(np.concatenate([[0], np.cumsum(Ts)]), dtype=np.int32)
    toff = torch.from_numpy(toff_h).to(new.device)
    Ttot, B = int(sum(Ts)), len(Ts)
    ws = torch.empty(_lib.load().avc_dsp_griffin_lim_ws_floats(Ttot, hp.n_fft, hp.hop_length, hp.win_length), device=new.device)
    y = torch.empty(hp.hop_length * (Ttot - B), device=new.device)
    rc = _lib.load().avc_dsp_griffin_lim_ragged(PD._P(mag), PD._P(toff), ctypes.c_void_p(toff_h.ctypes.data), B, Ttot, hp.n_fft, hp.hop_length, hp.win_length, 0,
                                                PD._P(new.basis_fwd), PD._P(new.basis_inv), PD._P(ws), PD._P(y), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    woff = np.concatenate([[0], np.cumsum(lengths)])

    def finish_new():
        return new._finish_ragged(y, lengths, True)

    def finish_old():
        return [old._finish(y[woff[i]:woff[i + 1]].contiguous(), True) for i in range(B)]
    a, b = finish_new(), finish_old()
    assert all(x.shape == z.shape and np.array_equal(x.view(np.int32), z.view(np.int32)) for x, z in zip(a, b)), "finishes differ"
    res = {"device": torch.cuda.get_device_name(0), "utterances": B, "seconds_of_audio": float(secs.sum()), "frames": Ttot, "reps": args.reps,
           "front": measure({"batched": front_new, "per_utterance_parent": front_old}, args.reps),
           "finish": measure({"batched": finish_new, "per_utterance_parent": finish_old}, args.reps)}
    for stage, fns in (("front", {"batched": (new, front_new), "per_utterance_parent": (old, front_old)}),
                       ("finish", {"batched": (new, finish_new), "per_utterance_parent": (old, finish_old)})):
        for side, (d, fn) in fns.items():
            calls, syncs = counted(d, fn)
            res[stage][side].update(entry_point_calls=calls, host_syncs=syncs)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
