"""The batched audio front and back end (dsp.MelDSP.get_spectrograms_batch / melspectrogram2wav_batch, inference.Inferencer.mels_from_wavs /
convert_wavs, several -source on the command line) against the one-utterance-at-a-time path they replace: BIT-equal per utterance,
because the packed kernels share their bodies with the single ones (tests/test_dsp_ragged_ops.py) and the GEMM columns of an
utterance do not depend on their neighbours.  The front end is also held against oracle/dsp_oracle.py at the bars of
tests/test_dsp.py::test_get_spectrograms_matches_oracle, and its trim indices must be the oracle's -- a fair demand for the utterances
below, which the first test establishes from the oracle alone: every one is cut at both ends and none has a frame within 0.1 dB of
trim's threshold (fp32 frame powers are within 1e-5 relative = 4e-5 dB of the oracle's).

Small hyper-parameters on the simulator, the stock ones on the MI355X; the Inferencer tests run a tiny model at small hyper-parameters
on both.
"""
import collections
import pickle
import types

import numpy as np
import pytest
import torch
from scipy.io import wavfile

from adaptive_voice_conversion_amd import dsp as PD
from adaptive_voice_conversion_amd import inference as INF
from oracle import dsp_oracle as D
from tests.emu_util import KINDS, backend
from tests.test_dsp import hp_for, product_hp, speechlike

# (silent samples in front, speechlike samples, seed); 2500 silent samples behind.  Trimmed lengths (oracle): 3584, 8192, 8704, 9216 at
# 8 kHz; 42496, 25600, 26112, 44032 at 24 kHz
UTTS = {"emu": [(2100, 4000, 30), (1700, 7000, 31), (2600, 7300, 32), (3100, 7900, 33)],
        "gpu": [(3000, 42500, 30), (2200, 30000, 31), (4100, 35000, 32), (3300, 45000, 33)]}
TAIL = 2500


def utterances(kind):
    sr = hp_for(kind).sr
    return [np.concatenate([np.zeros(lead, np.float32), speechlike(n, sr, seed), np.zeros(TAIL, np.float32)]) for lead, n, seed in UTTS[kind]]


def bits(t):
    t = t.detach().cpu().contiguous() if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(t))
    return t.view(torch.int32).numpy()


class CountingLib:
    """the library with a counter per entry point"""

    def __init__(self, lib):
        self._lib, self.calls = lib, collections.Counter()

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            self.calls[name] += 1
            return fn(*args)
        return call


_CACHE = {}


def setup(kind):
    """(MelDSP on a counting library, hyper-parameters, the four utterances, the oracle's trim indices, the oracle's features trimmed
    [(mel, mag)] and untrimmed [mel]), made once per backend"""
    if kind not in _CACHE:
        lib, dev = backend(kind)
        hp = hp_for(kind)
        dsp = PD.MelDSP(product_hp(hp), device=dev, lib=lib)
        dsp.lib = CountingLib(lib)
        ys = utterances(kind)
        _CACHE[kind] = (dsp, hp, ys, [D.trim(y, top_db=hp.top_db)[1] for y in ys], [D.get_spectrograms(y, hp) for y in ys],
                        [D.get_spectrograms(y, hp, do_trim=False)[0] for y in ys])
    return _CACHE[kind]


@pytest.mark.parametrize("kind", ["emu", "gpu"])
def test_the_utterances_are_fair_for_trim(kind):
    """From the oracle alone (no library, no GPU): every utterance of both sets is cut at both ends, the trimmed lengths differ, and no
    frame's level is within 0.1 dB of the threshold."""
    hp = hp_for(kind)
    lengths = set()
    for y in utterances(kind):
        _, (s, e) = D.trim(y, top_db=hp.top_db)
        assert 0 < s < e < len(y)
        lengths.add(e - s)
        yp = np.pad(y.astype(np.float64), 1024, mode="reflect")
        idx = np.arange(2048)[:, None] + 512 * np.arange(1 + (len(yp) - 2048) // 512)[None, :]
        mse = np.mean(yp[idx] ** 2, axis=0)
        db = 10.0 * np.log10(np.maximum(1e-10, mse)) - 10.0 * np.log10(np.maximum(1e-10, mse.max()))
        assert np.abs(db + hp.top_db).min() > 0.1
    assert len(lengths) == 4


@pytest.mark.parametrize("kind", KINDS)
def test_get_spectrograms_batch_equals_single_calls_bitwise(kind):
    """mel and mag, trimmed and untrimmed, of 4 utterances from ONE launch set each == get_spectrograms_device per utterance, to the bit;
    the results are views of one packed buffer.  Launches of the set: one frame-power launch, one fused framing, one magnitude, two
    dB-normalisations, and the STFT and mel GEMMs once per utterance on its column block (8 calls: avc_launch_conv chooses tile and
    split-K from the columns of a launch, so only a launch of T_b columns sums as the single call does; at the stock geometry one
    GEMM over all columns differs from the single calls by up to 4.9e-5 in the mel and 1.7e-4 in the mag, measured on the MI355X) --
    and none of the single-utterance DSP entry points."""
    dsp, hp, ys, _, _, _ = setup(kind)
    single = [dsp.get_spectrograms_device(y) for y in ys]
    single_raw = [dsp.get_spectrograms_device(y, do_trim=False) for y in ys]
    dsp.lib.calls.clear()
    mels, mags = dsp.get_spectrograms_batch(ys, with_mag=True)
    assert dict(dsp.lib.calls) == {"avc_dsp_frame_power_ragged": 1, "avc_dsp_frames_ragged_preemph": 1, "avc_conv1d_fwd": 8, "avc_dsp_magnitude": 1,
                                   "avc_dsp_db_normalize": 2}
    raw, raw_mag = dsp.get_spectrograms_batch(ys, do_trim=False, with_mag=True)
    assert len(mels) == len(mags) == len(raw) == len(raw_mag) == 4
    for b in range(4):
        assert mels[b].shape == single[b][0].shape and mels[b].shape[1] == hp.n_mels and mags[b].shape == single[b][1].shape
        assert np.array_equal(bits(mels[b]), bits(single[b][0])) and np.array_equal(bits(mags[b]), bits(single[b][1])), b
        assert raw[b].shape == single_raw[b][0].shape
        assert np.array_equal(bits(raw[b]), bits(single_raw[b][0])) and np.array_equal(bits(raw_mag[b]), bits(single_raw[b][1])), b
    for b in range(3):                      # views of ONE packed [sum T_b, n_mels] buffer
        assert mels[b + 1].data_ptr() == mels[b].data_ptr() + 4 * mels[b].numel() and mags[b + 1].data_ptr() == mags[b].data_ptr() + 4 * mags[b].numel()


@pytest.mark.parametrize("kind", KINDS)
def test_get_spectrograms_batch_matches_oracle_and_its_trim_indices(kind):
    """The bars of test_get_spectrograms_matches_oracle per utterance (1e-4 absolute on the bins within 80 dB of the peak, 2e-2 on the
    rest) for mag, mel and the untrimmed mel; the trim indices are the oracle's."""
    dsp, hp, ys, want_idx, want, want_raw = setup(kind)
    mels, mags = dsp.get_spectrograms_batch(ys, with_mag=True)
    raw = dsp.get_spectrograms_batch(ys, do_trim=False)
    lengths = [len(y) for y in ys]
    packed = torch.from_numpy(np.concatenate(ys)).to(dsp.device)
    assert dsp._trim_bounds_ragged(packed, lengths, hp.top_db) == want_idx
    for b in range(4):
        rmel, rmag = want[b]
        assert tuple(mels[b].shape) == rmel.shape and tuple(mags[b].shape) == rmag.shape and mels[b].dtype == torch.float32
        assert mels[b].shape[0] == 1 + (want_idx[b][1] - want_idx[b][0]) // hp.hop_length
        for got, ref in ((mags[b], rmag), (mels[b], rmel), (raw[b], want_raw[b])):
            got = got.cpu().numpy()
            loud = ref > ref.max() - 0.8
            assert loud.mean() > 0.2
            np.testing.assert_allclose(got[loud], ref[loud], atol=1e-4)
            np.testing.assert_allclose(got, ref, atol=2e-2)


@pytest.mark.parametrize("kind", KINDS)
def test_max_frames_gives_the_same_tensors_in_two_launch_sets(kind):
    """max_frames = the frames of the last two utterances, which the first three exceed: sets (0, 1) and (2, 3); a cap below every utterance:
    four sets of one.  Same bits, still ONE frame-power launch.
    (The GEMMs run per utterance, so the columns of a launch do not depend on how the list is cut into sets.)"""
    dsp, hp, ys, idx, _, _ = setup(kind)
    mels, mags = dsp.get_spectrograms_batch(ys, with_mag=True)
    T = [int(m.shape[0]) for m in mels]
    assert T[0] + T[1] <= T[2] + T[3] < T[0] + T[1] + T[2]
    for cap, sets in ((T[2] + T[3], 2), (min(T) - 1, 4)):
        dsp.lib.calls.clear()
        m2, g2 = dsp.get_spectrograms_batch(ys, with_mag=True, max_frames=cap)
        assert dsp.lib.calls["avc_dsp_frames_ragged_preemph"] == sets and dsp.lib.calls["avc_dsp_frame_power_ragged"] == 1
        for b in range(4):
            assert np.array_equal(bits(m2[b]), bits(mels[b])) and np.array_equal(bits(g2[b]), bits(mags[b])), (cap, b)


@pytest.mark.parametrize("kind", KINDS)
def test_melspectrogram2wav_batch_with_trim_equals_single_calls_bitwise(kind):
    """3 mels of different lengths, 2 Griffin-Lim iterations, do_trim=True: every waveform == melspectrogram2wav of that mel alone (length
    and samples); so for 2 equally long mels (the uniform Griffin-Lim in front of the same finish).  The finish is ONE de-emphasis launch
    and ONE frame-power launch for the batch."""
    dsp, hp, _, _, want, _ = setup(kind)
    cut = (150, 131, 187) if kind == "emu" else (120, 86, 88)          # hop (T - 1) > 1024 samples: what trim's padding needs
    ragged = [want[b][0][:n] for b, n in enumerate(cut)]
    for mels in (ragged, [ragged[0], want[1][0][:cut[0]]]):
        one = [dsp.melspectrogram2wav(m, do_trim=True, n_iter=2) for m in mels]
        dsp.lib.calls.clear()
        many = dsp.melspectrogram2wav_batch(mels, do_trim=True, n_iter=2)
        assert dsp.lib.calls["avc_dsp_deemphasis_ragged"] == 1 and dsp.lib.calls["avc_dsp_frame_power_ragged"] == 1
        assert dsp.lib.calls["avc_dsp_deemphasis"] == 0 and dsp.lib.calls["avc_dsp_frame_power"] == 0
        assert len(many) == len(mels)
        for a, b in zip(one, many):
            assert a.dtype == b.dtype == np.float32 and a.shape == b.shape and a.size > 0 and np.array_equal(bits(a), bits(b))
        raw = dsp.melspectrogram2wav_batch(mels, do_trim=False, n_iter=2)
        for m, a, b in zip(mels, [dsp.melspectrogram2wav(m, do_trim=False, n_iter=2) for m in mels], raw):
            assert a.shape == b.shape == (hp.hop_length * (len(m) - 1),) and np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("kind", KINDS)
def test_errors_name_the_utterance(kind):
    dsp, hp, ys, _, _, _ = setup(kind)
    with pytest.raises(ValueError, match=r"utterance 1: 1024 samples are too short for the reflect padding of trim"):
        dsp.get_spectrograms_batch([ys[0], ys[1][:1024], ys[2]])
    with pytest.raises(ValueError, match=rf"utterance 2: {hp.n_fft // 2} samples are too short for the reflect padding of the STFT"):
        dsp.get_spectrograms_batch([ys[0], ys[1], ys[2][:hp.n_fft // 2]], do_trim=False)
    with pytest.raises(ValueError, match=r"utterance 0: empty"):
        dsp.get_spectrograms_batch([ys[0][:0], ys[1]])
    if kind == "emu":          # (at the stock geometry trim's padding needs what the STFT's needs: that refusal comes first)
      with pytest.raises(ValueError, match=r"utterance 2: .* too short for the reflect padding of trim"):
        dsp.melspectrogram2wav_batch([np.full((1 + 1100 // hp.hop_length + 2, hp.n_mels), 0.5, np.float32)] * 2 +
                                     [np.full((1024 // hp.hop_length + 1, hp.n_mels), 0.5, np.float32)], n_iter=0)
    assert dsp.get_spectrograms_batch([]) == []


# ---------------------------------------------------------------- Inferencer: a tiny model at small hyper-parameters on both backends
SOURCES = [(2600, 11), (3100, 13)]
TARGETS = [(1900, 12), (2300, 14)]


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("batch_front")


_INF = {}


def inferencer(kind, workdir):
    """(Inferencer, source paths, target paths, directory)"""
    if kind not in _INF:
        from oracle import avc_oracle as O
        lib, dev = backend(kind)
        hp = D.small_hyperparams(n_fft=64, hop=10, win=40, n_mels=16, sr=8000, n_iter=3)
        d = workdir / kind
        d.mkdir()
        cfg = O.tiny_config()
        torch.save(O.make_state_dict(cfg, 7), d / "m.ckpt")
        with open(d / "attr.pkl", "wb") as f:
            pickle.dump({"mean": np.linspace(0.2, 0.6, 16).astype(np.float32), "std": np.linspace(0.1, 0.3, 16).astype(np.float32)}, f)
        paths = []
        for i, (n, seed) in enumerate(SOURCES + TARGETS):
            paths.append(str(d / f"utt{i}.wav"))
            wavfile.write(paths[-1], hp.sr, speechlike(n, hp.sr, seed))          # float32 wav: decoded without quantisation
        args = types.SimpleNamespace(model=str(d / "m.ckpt"), attr=str(d / "attr.pkl"), source=paths[0], target=paths[2], output=str(d / "out.wav"),
                                     sample_rate=hp.sr)
        _INF[kind] = (INF.Inferencer(cfg, args, lib=lib if kind == "emu" else None, dsp_hp=product_hp(hp)), paths[:2], paths[2:], d, cfg, hp)
    return _INF[kind]


@pytest.mark.parametrize("kind", KINDS)
def test_mels_from_wavs_equals_mel_from_path_bitwise(kind, workdir):
    inf, srcs, tgts, _, _, _ = inferencer(kind, workdir)
    many = inf.mels_from_wavs(srcs + tgts)
    assert len(many) == 4
    for path, m in zip(srcs + tgts, many):
        one = inf._mel_from_path(path)
        assert m.dtype == torch.float32 and m.device.type == inf.model.flat_parameters().device.type
        assert tuple(m.shape) == tuple(one.shape) and np.array_equal(bits(m), bits(one)), path


def per_file(inf, src, tgt, ragged):
    """one pair, one file at a time: (waveform, denormalised converted mel) through the uniform plan (inference_one_utterance) or through
    the ragged plan on that pair alone"""
    ms, mt = inf._mel_from_path(src), inf._mel_from_path(tgt)
    if not ragged:
        return inf.inference_one_utterance(ms, mt)
    mel = inf.denormalize(inf.convert_batch([(ms, mt)])[0].numpy())
    return inf.dsp().melspectrogram2wav(mel), mel


@pytest.mark.parametrize("kind", KINDS)
def test_convert_wavs_equals_the_per_file_path(kind, workdir):
    """Two sources, two targets, wav to wav in one front-end launch set and one batched back end == per file: _mel_from_path,
    inference_one_utterance (which vocodes with melspectrogram2wav).  Mels bit for bit, waveforms of equal length and equal samples.
    (convert_wavs converts every pair on the plan inference_one_utterance runs; its ragged=True form is the next test.)"""
    inf, srcs, tgts, _, _, _ = inferencer(kind, workdir)
    wavs, mels = inf.convert_wavs(srcs, tgts)
    assert len(wavs) == len(mels) == 2
    ref = [per_file(inf, srcs[b], tgts[b], ragged=False) for b in range(2)]
    for b, (wav, mel) in enumerate(ref):
        same_len = len(wavs[b]) == len(wav)
        print(f"[{kind}] pair {b}: mel max |diff| {np.abs(mels[b] - mel).max():.3e}; lengths {len(wavs[b])} / {len(wav)}" +
              (f"; waveform max |diff| / peak {np.abs(wavs[b] - wav).max() / np.abs(wav).max():.3e}" if same_len else ""))
    for b, (wav, mel) in enumerate(ref):
        assert mels[b].shape == mel.shape and np.array_equal(bits(mels[b]), bits(mel)), b
        assert wavs[b].shape == wav.shape and np.array_equal(bits(wavs[b]), bits(wav)), b


@pytest.mark.parametrize("kind", KINDS)
def test_convert_wavs_equals_the_per_file_ragged_path_bitwise(kind, workdir):
    """convert_wavs(ragged=True): all pairs in ONE ragged launch set, against the per-file path through the same (ragged) plan --
    _mel_from_path, convert_batch on the one pair, melspectrogram2wav: mels bit for bit, waveforms of equal length and equal samples.
    Against the uniform plan of inference_one_utterance the ragged mels are held to that test's bar of 1e-4 (measured 1.4e-6 on the simulator, 1.8e-6 on the
    MI355X: the InstanceNorm rows reduce in another order, tests/test_dsp.py::test_inference_from_path_wav_to_wav).  And with an enrolled
    voice instead of targets."""
    inf, srcs, tgts, _, _, _ = inferencer(kind, workdir)
    wavs, mels = inf.convert_wavs(srcs, tgts, ragged=True)
    for b in range(2):
        assert np.abs(mels[b] - per_file(inf, srcs[b], tgts[b], ragged=False)[1]).max() <= 1e-4, b
    for b in range(2):
        wav, mel = per_file(inf, srcs[b], tgts[b], ragged=True)
        assert mels[b].shape == mel.shape and np.array_equal(bits(mels[b]), bits(mel)), b
        assert wavs[b].shape == wav.shape and wav.size > 0 and np.array_equal(bits(wavs[b]), bits(wav)), b
    emb = inf.enroll([inf._mel_from_path(t) for t in tgts])
    wavs_e, mels_e = inf.convert_wavs(srcs, emb=emb, n_iter=1)
    want = [inf.denormalize(m.numpy()) for m in inf.convert_batch([inf._mel_from_path(s) for s in srcs], emb=emb)]
    for b in range(2):
        assert np.array_equal(bits(mels_e[b]), bits(want[b])), b
        assert np.array_equal(bits(wavs_e[b]), bits(inf.dsp().melspectrogram2wav(want[b], n_iter=1))), b
    with pytest.raises(ValueError, match="exactly one of targets"):
        inf.convert_wavs(srcs)
    with pytest.raises(ValueError, match="2 sources but 1 targets"):
        inf.convert_wavs(srcs, tgts[:1])


@pytest.mark.parametrize("kind", KINDS)
def test_command_line_with_two_sources_writes_two_files(kind, workdir):
    """-source twice: args.source is a list, -output a directory that receives one wav per source, named like it; the files hold what
    convert_batch from the enrolled target + melspectrogram2wav_batch give.  One -source stays a string and writes the one file."""
    inf0, srcs, tgts, d, cfg, hp = inferencer(kind, workdir)
    lib, _ = backend(kind)
    out = d / "converted"
    args = INF.parse_args(["-model", str(d / "m.ckpt"), "-attr", str(d / "attr.pkl"), "-source", srcs[0], "-source", srcs[1], "-target", tgts[0],
                           "-output", str(out), "-sample_rate", str(hp.sr)])
    assert args.source == srcs and args.target == tgts[0]
    inf = INF.Inferencer(cfg, args, lib=lib if kind == "emu" else None, dsp_hp=product_hp(hp))
    wavs, mels = inf.inference_from_path()
    assert sorted(p.name for p in out.iterdir()) == ["utt0.wav", "utt1.wav"]
    emb = inf.enroll([inf._mel_from_path(tgts[0])])
    for b, name in enumerate(("utt0.wav", "utt1.wav")):
        rate, written = wavfile.read(out / name)
        assert rate == hp.sr and written.dtype == np.float32 and len(written) > 0 and np.array_equal(written, wavs[b])
    want = [inf.denormalize(m.numpy()) for m in inf.convert_batch([inf._mel_from_path(s) for s in srcs], emb=emb)]
    for b in range(2):
        assert np.array_equal(bits(mels[b]), bits(want[b]))
    one = INF.parse_args(["-source", srcs[0], "-target", tgts[0], "-output", str(d / "one.wav")])
    assert one.source == srcs[0] and one.target == tgts[0] and one.output == str(d / "one.wav")
    assert INF.Inferencer.output_paths(["a/x.wav", "b/x.wav", "y.wav"], str(d / "dup")) == [str(d / "dup" / "0_x.wav"), str(d / "dup" / "1_x.wav"),
                                                                                         str(d / "dup" / "y.wav")]
