"""One-shot conversion front (reference: inference.py:24-93 ``Inferencer``), the immediate
caller of the hot path.

Kept from the reference: ``Inferencer(config, args)``, ``load_model`` (``args.model`` =
``<path>.ckpt`` state_dict), ``attr`` pickle with per-bin ``mean``/``std``,
``utt_make_frames``, ``normalize`` / ``denormalize``, ``inference_one_utterance(x, x_cond)``.
Added: ``convert_batch`` — many (source, target) pairs of arbitrary, unequal lengths in few engine
calls (pairs are bucketed by shape; the reference only ever runs batch 1); ``enroll`` + ``convert_batch(sources, emb=...)`` —
enrol a target voice once from any number of utterances, then convert whatever comes in without running the speaker encoder again.

The audio front and back end (reference: ``get_spectrograms`` / ``melspectrogram2wav`` of
``preprocess/tacotron/utils.py``, librosa on the CPU there) run on the GPU through ``dsp.MelDSP``:
``inference_from_path`` (inference.py:86-93) reads two wav files and writes the converted one, ``mel2wav`` defaults to the
device-side ``melspectrogram2wav`` when the model has as many mel bins as the DSP hyper-parameters produce (the stock
``config.yaml`` trains on 512-mel features, hyperparams.py:29); a caller-supplied ``mel2wav`` takes precedence, and with
neither the waveform slot of the result is ``None``.
"""
import pickle
from collections import defaultdict

import torch

from .model import AE
from .utils import cc, local_device


class Inferencer(object):
    def __init__(self, config, args, mel2wav=None, lib=None, dsp_hp=None):
        self.config = config
        self.args = args
        self.mel2wav = mel2wav
        self._lib = lib
        self._dsp_hp = dsp_hp   # None: preprocess/tacotron/hyperparams.py's values
        self.build_model()
        if getattr(args, "model", None):
            self.load_model()
        self.attr = None
        if getattr(args, "attr", None):
            with open(args.attr, "rb") as f:
                self.attr = pickle.load(f)
        self._dsp = None

    def dsp(self):
        """The device-side mel <-> waveform DSP (built on first use: its DFT bases take ~30 MB of HBM)."""
        if self._dsp is None:
            from .dsp import Hyperparams, MelDSP
            self._dsp = MelDSP(self._dsp_hp or Hyperparams, device=self.model.flat_parameters().device, lib=self._lib)
        return self._dsp

    def load_model(self):
        dev = self.model.flat_parameters().device
        self.model.load_state_dict(torch.load(f"{self.args.model}", map_location=dev))

    def build_model(self):
        self.model = AE(self.config, lib=self._lib) if self._lib is not None else cc(AE(self.config))
        self.model.eval()

    # ---- inference.py:54-60
    def utt_make_frames(self, x):
        frame_size = self.config["data_loader"]["frame_size"]
        remains = x.size(0) % frame_size
        if remains != 0:
            x = torch.nn.functional.pad(x, (0, remains))
        return x.view(1, x.size(0) // frame_size, frame_size * x.size(1)).transpose(1, 2)

    def denormalize(self, x):
        if self.attr is None:
            return x
        return x * self.attr["std"] + self.attr["mean"]

    def normalize(self, x):
        if self.attr is None:
            return x
        return (x - self.attr["mean"]) / self.attr["std"]

    # ---- inference.py:62-70
    def inference_one_utterance(self, x, x_cond):
        """x: [T, M] source mel, x_cond: [T', M] target-speaker mel (normalised).  Returns (wav | None, mel [T'', M])."""
        dev = self.model.flat_parameters().device
        x = self.utt_make_frames(x.to(dev))
        x_cond = self.utt_make_frames(x_cond.to(dev))
        with torch.no_grad():
            dec = self.model.inference(x, x_cond)
        dec = dec.transpose(1, 2).squeeze(0).detach().cpu().numpy()
        dec = self.denormalize(dec)
        if self.mel2wav is not None:
            wav = self.mel2wav(dec)
        elif getattr(self.args, "source", None) is not None and dec.shape[1] == self.dsp().hp.n_mels:
            wav = self.dsp().melspectrogram2wav(dec)            # inference.py:69
        else:
            wav = None
        return wav, dec

    # ---- inference.py:82-93
    def write_wav_to_file(self, wav_data, output_path):
        from scipy.io.wavfile import write
        write(output_path, rate=int(getattr(self.args, "sample_rate", 24000)), data=wav_data)

    def _mel_from_path(self, path):
        mel, _ = self.dsp().get_spectrograms(path)
        return torch.from_numpy(self.normalize(mel)).float()

    def mels_from_wavs(self, wavs):
        """``_mel_from_path`` for a LIST of wav paths / decoded waveforms in ONE front-end launch set (``MelDSP.get_spectrograms_batch``:
        one upload, one read-back for all the trims) and ``normalize`` on the device.  Returns the list of normalised [T_b, n_mels] float32
        DEVICE tensors, bit-equal to ``_mel_from_path`` per file: the arithmetic runs in the dtype of the attr arrays, as numpy's does."""
        packed, _, toff = self.dsp()._spectrograms_packed(list(wavs))
        if self.attr is not None:
            mean, std = (torch.as_tensor(self.attr[k]).to(packed.device) for k in ("mean", "std"))
            packed = ((packed.to(torch.promote_types(packed.dtype, mean.dtype)) - mean) / std).float()
        return [packed[toff[b]:toff[b + 1]] for b in range(len(toff) - 1)]

    def convert_wavs(self, sources, targets=None, emb=None, src_of=None, do_trim=True, n_iter=None, ragged=False):
        """Wav to wav for many utterances: ``sources`` (and ``targets``, one per source: the voice of pair i) are wav paths or decoded
        waveforms of any lengths.  ONE front-end launch set for all sources and targets (``mels_from_wavs``), the conversion on mels
        that never leave the device in between, and ONE batched back end (``melspectrogram2wav_batch``).
        The conversion of (source, target) pairs: by default every pair goes through the plan ``inference_one_utterance`` runs (the
        uniform plan at batch 1), so the result is what the per-file path gives, to the bit; ``ragged=True`` converts all pairs in ONE
        ragged launch set (``convert_batch``), whose InstanceNorm rows reduce in another order: the mels then agree with the per-file
        path to about 1e-6, not to the bit.  With ``emb`` / ``src_of`` (an enrolled voice, a fan-out) the conversion is the ragged one.
        Returns (list of float32 waveforms, list of converted denormalised mels)."""
        sources = list(sources)
        if (targets is None) == (emb is None):
            raise ValueError("convert_wavs: pass exactly one of targets (one wav per source) and emb (speaker embeddings)")
        if targets is not None:
            targets = list(targets)
            if len(targets) != len(sources):
                raise ValueError(f"convert_wavs: {len(sources)} sources but {len(targets)} targets")
            mels = self.mels_from_wavs(sources + targets)
            pairs = list(zip(mels[:len(sources)], mels[len(sources):]))
            if ragged:
                converted = self.convert_batch(pairs)
            else:
                with torch.no_grad():
                    converted = [self.model.inference(self.utt_make_frames(x), self.utt_make_frames(c)).transpose(1, 2).squeeze(0).cpu()
                                 for x, c in pairs]
        else:
            converted = self.convert_batch(self.mels_from_wavs(sources), emb=emb, src_of=src_of)
        out = [self.denormalize(m.numpy()) for m in converted]
        return self.dsp().melspectrogram2wav_batch(out, do_trim=do_trim, n_iter=n_iter), out

    def inference_from_path(self):
        """The reference's command (one ``-source``, one ``-target``), and the enrolment workflow on top of it: several targets
        (``args.target`` a list: the voice is the mean embedding of the files), ``args.save_emb`` (write the enrolled embedding with
        ``torch.save``; without ``args.source`` nothing is converted), ``args.emb`` (convert with a saved embedding instead of a target).
        Several sources (``args.source`` a list): ``args.output`` is a directory, source ``name.wav`` is written to ``output/name.wav``
        (a repeated name gets its position in front).  Whenever more than one file is read, all of them go through the front end in
        one launch set (``mels_from_wavs``)."""
        dsp = self.dsp()
        if self.model._n_mels != dsp.hp.n_mels:
            raise ValueError(f"the model works on {self.model._n_mels}-mel features, get_spectrograms produces {dsp.hp.n_mels} "
                             "(preprocess/tacotron/hyperparams.py:29)")
        target = getattr(self.args, "target", None)
        targets = list(target) if isinstance(target, (list, tuple)) else ([target] if target is not None else [])
        emb_path, save_emb = getattr(self.args, "emb", None), getattr(self.args, "save_emb", None)
        if emb_path is not None and targets:
            raise ValueError("give either -target (one or several wav files to enrol from) or -emb (a saved embedding), not both")
        if emb_path is None and not targets:
            raise ValueError("a target voice is needed: -target (one or several wav files) or -emb (a saved embedding)")
        source = getattr(self.args, "source", None)
        many = isinstance(source, (list, tuple))
        sources = list(source) if many else ([source] if source is not None else [])
        files = sources + targets
        mels = self.mels_from_wavs(files) if len(files) > 1 else [self._mel_from_path(f) for f in files]   # ONE front-end launch set
        src_mels, tgt_mels = mels[:len(sources)], mels[len(sources):]
        if len(targets) == 1 and emb_path is None and save_emb is None and not many:   # the reference's path (inference.py:86-93)
            conv_wav, conv_mel = self.inference_one_utterance(src_mels[0], tgt_mels[0])
            self.write_wav_to_file(conv_wav, self.args.output)
            return conv_wav, conv_mel
        if emb_path is not None:
            emb = torch.load(emb_path, map_location="cpu")
        else:
            emb = self.enroll(tgt_mels)
        if save_emb is not None:
            torch.save(emb.detach().cpu(), save_emb)
        if not sources:
            return None, None   # enrolment only
        conv_mels = [self.denormalize(m.numpy()) for m in self.convert_batch(src_mels, emb=emb)]
        if self.mel2wav is not None:
            conv_wavs = [self.mel2wav(m) for m in conv_mels]
        else:
            conv_wavs = dsp.melspectrogram2wav_batch(conv_mels) if many else [dsp.melspectrogram2wav(conv_mels[0])]
        if not many:
            self.write_wav_to_file(conv_wavs[0], self.args.output)
            return conv_wavs[0], conv_mels[0]
        for path, wav in zip(self.output_paths(sources, self.args.output), conv_wavs):
            self.write_wav_to_file(wav, path)
        return conv_wavs, conv_mels

    @staticmethod
    def output_paths(sources, out_dir):
        """Where the conversions of several sources go: ``out_dir/<file name of the source>``; a name that occurs twice gets the
        source's position in front (``1_name.wav``).  The directory is created."""
        import os
        os.makedirs(out_dir, exist_ok=True)
        names = [os.path.basename(str(s)) for s in sources]
        return [os.path.join(out_dir, n if names.count(n) == 1 else f"{i}_{n}") for i, n in enumerate(names)]

    def enroll(self, utterances):
        """Enrol a target voice: ``utterances`` are normalised [T, M] mels of ONE speaker, of any (unequal) lengths.  All of them go
        through the speaker encoder in ONE ragged launch set (``AE.get_speaker_embeddings_ragged``); returns the mean of their
        embeddings, [c_emb], on the model's device -- what ``convert_batch(sources, emb=...)`` takes."""
        utterances = list(utterances)
        if not utterances:
            raise ValueError("enroll: at least one utterance is needed")
        with torch.no_grad():
            return self.model.get_speaker_embeddings_ragged(utterances).mean(0)

    def convert_batch_to_wav(self, pairs, max_streams=4, do_trim=True, n_iter=None, emb=None, src_of=None):
        """`convert_batch` + the audio back end: the converted mels are denormalised (inference.py:68) and vocoded by
        `melspectrogram2wav` -- all utterances, whatever their lengths, in ONE batched Griffin-Lim launch set (dsp.MelDSP).
        ``emb`` / ``src_of``: as in ``convert_batch`` (``pairs`` is then the list of sources).
        Returns (list of float32 waveforms, list of converted mels) in input (with ``src_of``: output) order."""
        mels = [self.denormalize(m.numpy()) for m in self.convert_batch(pairs, max_streams, emb=emb, src_of=src_of)]
        return self.dsp().melspectrogram2wav_batch(mels, do_trim=do_trim, n_iter=n_iter), mels   # ONE Griffin-Lim launch set, any lengths

    def convert_grid(self, sources, voices):
        """Every source in every voice: ``sources`` is a list of S [T, M] tensors, ``voices`` a [V, c_emb] tensor of speaker embeddings
        (``enroll``'s results stacked).  ONE fan-out launch set (``convert_batch`` with ``src_of`` = each source V times): every source
        is uploaded and encoded once, whatever V.  Returns ``out[s][v]``, the [T'', M] CPU tensor of source s in voice v."""
        sources = list(sources)
        if not torch.is_tensor(voices) or voices.dim() != 2:
            raise ValueError(f"convert_grid: voices must be a [V, {self.model._c_emb}] tensor of speaker embeddings (one row per voice), got "
                             f"{tuple(voices.shape) if torch.is_tensor(voices) else type(voices)}")
        S, V = len(sources), int(voices.shape[0])
        outs = self.convert_batch(sources, emb=voices.repeat(S, 1), src_of=[s for s in range(S) for _ in range(V)])
        return [outs[s * V:(s + 1) * V] for s in range(S)]

    def convert_batch(self, pairs, max_streams=4, ragged=True, emb=None, src_of=None):
        """pairs: list of (src [T,M], tgt [T',M]) tensors of any lengths.  Default: ONE ragged launch set over all pairs
        (``AE.inference_ragged``: per-sample lengths inside every kernel; real utterances all differ in length, so shape buckets
        would be batches of one).  ``ragged=False``: the round-2 path -- pairs with equal (T, T') share one uniform plan,
        different shapes go out on up to ``max_streams`` HIP streams.  Lengths are never padded: reflect padding and the
        InstanceNorm statistics depend on the true length, so padding would change the result.
        Under ``compute_dtype: bf16`` the ragged path rounds the matrix-product operands to bf16 on fp32 storage ("bf16r"; the bf16
        pair-STORAGE engine of ``AE.inference`` takes uniform shapes only) -- ``self.model.last_ragged_compute`` says which mode ran.
        ``emb`` (an enrolled voice: ``enroll``'s result, [c_emb]; or one embedding per source, [B, c_emb]): ``pairs`` is then the list
        of SOURCES ([T,M] tensors) alone, converted to that voice in one ragged launch set in which the speaker encoder does not run
        (``AE.inference_ragged(xs, emb=...)``).
        ``src_of`` (with ``emb``): fan-out -- output j is source ``src_of[j]`` in the voice of row j of ``emb`` ([len(src_of), c_emb], or
        one voice for all); every source is uploaded and encoded once however often it is named (``AE.inference_ragged(xs, emb=...,
        src_of=...)``; ``convert_grid`` is the S x V form).
        Returns the converted mels ([T'',M] CPU tensors) in input order (with ``src_of``: one per entry of it)."""
        if src_of is not None and emb is None:
            raise ValueError("convert_batch: src_of goes with emb (sources alone, converted from embeddings): enrol the voices first")
        if emb is not None:
            if not ragged:
                raise ValueError("convert_batch(sources, emb=...) runs the ragged plan; ragged=False converts (source, target) pairs")
            srcs = list(pairs)
            if any(isinstance(s, (tuple, list)) for s in srcs):
                raise ValueError("convert_batch(sources, emb=...): pass the source utterances alone ([T, M] tensors), not (source, target) pairs")
            with torch.no_grad():
                outs = self.model.inference_ragged(srcs, emb=emb) if src_of is None else self.model.inference_ragged(srcs, emb=emb, src_of=src_of)
            return [o.t().cpu() for o in outs]
        if ragged:
            with torch.no_grad():
                outs = self.model.inference_ragged([s for s, _ in pairs], [t for _, t in pairs])
            return [o.t().cpu() for o in outs]
        return self._convert_batch_bucketed(pairs, max_streams)

    def _convert_batch_bucketed(self, pairs, max_streams=4):
        dev = self.model.flat_parameters().device
        buckets = defaultdict(list)
        for i, (s, t) in enumerate(pairs):
            buckets[(s.shape[0], t.shape[0])].append(i)
        out = [None] * len(pairs)
        cuda = dev.type == "cuda"
        streams = [torch.cuda.Stream(device=dev) for _ in range(min(max_streams, len(buckets)))] if cuda and len(buckets) > 1 else []
        main = torch.cuda.current_stream(dev) if cuda else None
        results = []
        with torch.no_grad():
            for k, ((_, _), idx) in enumerate(sorted(buckets.items(), key=lambda kv: -kv[0][0] * len(kv[1]))):   # big buckets first
                xs = torch.stack([pairs[i][0] for i in idx]).to(dev).transpose(1, 2)   # [B, M, T] views, no copy
                xc = torch.stack([pairs[i][1] for i in idx]).to(dev).transpose(1, 2)
                if streams:
                    st = streams[k % len(streams)]
                    st.wait_stream(main)                      # inputs were produced on the caller's stream
                    with torch.cuda.stream(st):
                        dec = self.model.inference(xs, xc)    # (one plan + workspace per shape: independent of other buckets)
                        xs.record_stream(st), xc.record_stream(st)
                        for e in self.model._plans.d["inference"].values():   # the workspace may have been allocated on another stream
                            if e.ws is not None:
                                e.ws.record_stream(st)
                else:
                    dec = self.model.inference(xs, xc)
                results.append((idx, dec))
            for st in streams:
                main.wait_stream(st)
            for idx, dec in results:
                dec = dec.transpose(1, 2).cpu()
                for k, i in enumerate(idx):
                    out[i] = dec[k]
        return out


def make_parser():
    """The reference's command line (inference.py:95-109) plus the enrolment options."""
    from argparse import ArgumentParser
    parser = ArgumentParser()
    parser.add_argument('-attr', '-a', help='attr file path')
    parser.add_argument('-config', '-c', help='config file path')
    parser.add_argument('-model', '-m', help='model path')
    parser.add_argument('-source', '-s', action='append',
                        help='source wav path; may be given several times: -output is then a directory that receives one wav per source')
    parser.add_argument('-target', '-t', action='append',
                        help='target wav path; may be given several times: the voice is then enrolled from all of them (mean embedding)')
    parser.add_argument('-output', '-o', help='output wav path (with several -source: output directory)')
    parser.add_argument('-sample_rate', '-sr', help='sample rate', default=24000, type=int)
    parser.add_argument('-save_emb', help='write the enrolled speaker embedding here (torch.save); without -source nothing is converted')
    parser.add_argument('-emb', help='convert with a speaker embedding saved by -save_emb instead of -target')
    return parser


def parse_args(argv=None):
    """A single -target / -source stays the string it has always been; several become a list."""
    args = make_parser().parse_args(argv)
    if args.source is not None and len(args.source) == 1:
        args.source = args.source[0]
    if args.target is not None and len(args.target) == 1:
        args.target = args.target[0]
    return args


def main(argv=None):
    """The reference's command line (inference.py:95-109)."""
    from .config import load_config
    args = parse_args(argv)
    inferencer = Inferencer(config=load_config(args.config), args=args)
    inferencer.inference_from_path()


if __name__ == '__main__':
    main()
