"""Mel <-> waveform DSP, kernel by kernel (csrc/dsp.hip, csrc/dsp_api.hip, dsp.py): every avc_dsp_* entry point through the C ABI
against numpy float64 (oracle/dsp_oracle.py where it has the function), over a set of window geometries, the shortest accepted
lengths, the clamps of the element-wise kernels and launches whose grid-stride loops run a second pass (dsp_blocks() caps the grid at
4096 x 256 lanes: element 1,048,576 is the first one of the second pass).  tests/test_dsp.py drives the same code through the
composites at one geometry per backend; this file pins the pieces.

Outputs and workspaces sit in sentinel red zones, inputs in NaN red zones (tests/redzone.py).

Bars
  * DFT bases: computed in double and rounded once -> 1 ulp of the float32 closed form.
  * STFT / iSTFT / Griffin-Lim without iterations: the project's 2e-5 of the reference's peak (tests/test_dsp.py header).
  * element-wise kernels with sqrtf / log10f / exp10f: the kernel is fp32 arithmetic of a formula, so the yardstick is the SAME formula
    in numpy float32 against float64 on the same inputs: the worst distance d of the two, then 4 d with a floor of 1 ulp of the output
    (`fp32_bar`).  The distance is relative where the error is (a quotient, a square root, a power of ten), absolute where the formula
    cancels (the normalised dB features live in [1e-8, 1]; y[i] - a y[i-1]).  Measured ratios worst |got - ref| / bar (simulator / MI355X):
    phase 0.25 / 0.25, magnitude 0.25 / 0.31, dB-normalise 0.32 / 0.57, denormalise 0.25 / 0.25, pre-emphasis 0.25 / 0.25 (the simulator's
    arithmetic IS numpy's float32: d / 4 d).
  * de-emphasis: 2e-5 of the peak against scipy.signal.lfilter; at a = 0.999 4 x the error of a sequential float32 recurrence
    (measured: at most 0.53 of that bar on both backends).
  * frame powers: 1e-5 relative (a float32 tree sum of at most 2048 squares).
The phase kernel has no entry point of its own in include/avc_hip.h (Griffin-Lim calls it between the two transforms), so its test
calls the library's launcher `avc_launch_dsp_phase` (csrc/avc_internal.h) by its C++ symbol.
"""
import ctypes

import numpy as np
import pytest
import torch
from scipy import signal

from adaptive_voice_conversion_amd import dsp as PD
from oracle import dsp_oracle as D
from tests.emu_util import KINDS, P, backend
from tests.redzone import GuardedOutput, guarded_input

GPU = pytest.mark.gpu
SMALL = (64, 10, 40)
STOCK = (2048, 300, 1200)
# (n_fft, hop, win): stock-like; win == n_fft; (n_fft - win) odd with hop not dividing win (twice); win = n_fft - 1; another n_fft; hop == win
G = [SMALL, (64, 16, 64), (64, 7, 39), (64, 13, 51), (32, 5, 31), (128, 33, 100), (64, 40, 40)]
G_ALL = G + [pytest.param(STOCK, marks=GPU)]
G_RAGGED = [SMALL, (64, 7, 39), (64, 16, 64), (128, 33, 100)]
PASS = 4096 * 256          # elements of one grid pass of every grid-stride kernel in dsp.hip
REF_DB, MAX_DB = 20.0, 100.0
F32 = np.float32


def ids(g):
    return "x".join(str(v) for v in g) if isinstance(g, tuple) else None


def lengths_of(n_fft, hop):
    return [n_fft // 2 + 1, n_fft // 2 + 2, 9 * hop, 3 * n_fft + 5]


def noise(n, seed):
    return np.random.RandomState(seed).randn(n).astype(F32)


def out_buf(shape, dev):
    return GuardedOutput(shape, device=dev)


def inp(a, dev):
    return guarded_input(torch.from_numpy(np.ascontiguousarray(a)), device=dev)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def untouched(g, before):
    """payload and red zones of a GuardedOutput are what they were (a refused call launches nothing)"""
    return torch.equal(g.buf.view(torch.int32), before)


def snapshot(g):
    return g.buf.view(torch.int32).clone()


def interleave(S):
    """complex [F][T] -> the library's [2F][T] fp32 rows (Re, Im interleaved)"""
    return np.stack([S.real, S.imag], axis=1).reshape(2 * S.shape[0], -1).astype(F32)


def to_complex(spec):
    s = spec.double().cpu().numpy()
    return s[0::2] + 1j * s[1::2]


def ulp(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(F32)).astype(np.float64)


def fp32_bar(ref64, same32, relative):
    """Per-element bar 4 d with a floor of 1 ulp of the output, d = the worst distance of the formula in float32 from float64."""
    ref64 = np.asarray(ref64, dtype=np.float64)
    err = np.abs(same32.astype(np.float64) - ref64)
    if relative:
        nz = ref64 != 0
        d = float((err[nz] / np.abs(ref64[nz])).max()) if nz.any() else 0.0
        return np.maximum(4 * d * np.abs(ref64), ulp(ref64))
    return np.maximum(4 * float(err.max()), ulp(ref64))


def worst(got, ref64, bar):
    return float((np.abs(np.asarray(got, dtype=np.float64) - ref64) / bar).max())


_BASES = {}


def bases(kind, geom):
    """(packed forward, packed inverse, dense forward [2F][win], dense inverse [win][2F]) of a geometry, made once per backend; the
    packed images are re-homed in NaN red zones like every other input"""
    if (kind, geom) not in _BASES:
        lib, dev = backend(kind)
        n_fft, hop, win = geom
        packed, dense = [], []
        for inv in (0, 1):
            sc = out_buf((lib.avc_dsp_basis_scratch_floats(n_fft, win),), dev)
            pk = out_buf((lib.avc_dsp_basis_floats(n_fft, win, inv),), dev)
            assert lib.avc_dsp_make_basis(n_fft, hop, win, inv, P(sc.view), P(pk.view), None) == 0
            sc.assert_intact(f"(avc_dsp_make_basis {geom} inverse={inv}: dense_scratch)")
            pk.assert_intact(f"(avc_dsp_make_basis {geom} inverse={inv}: packed)")
            packed.append(guarded_input(pk.view.clone()))
            dense.append(sc.view.cpu().numpy().reshape((n_fft + 2, win) if inv == 0 else (win, n_fft + 2)).copy())
        _BASES[(kind, geom)] = (packed[0], packed[1], dense[0], dense[1])
    return _BASES[(kind, geom)]


def run_stft(kind, geom, y, B=1):
    """y [B][L] -> the spec [2F][B T] and frames_ws [win][B T] tensors"""
    lib, dev = backend(kind)
    n_fft, hop, win = geom
    y = np.asarray(y, dtype=F32).reshape(B, -1)
    L = y.shape[1]
    T = lib.avc_dsp_num_frames(L, hop)
    frames, spec = out_buf((win, B * T), dev), out_buf((n_fft + 2, B * T), dev)
    assert lib.avc_dsp_stft_batch(P(inp(y, dev)), L, B, n_fft, hop, win, P(bases(kind, geom)[0]), P(frames.view), P(spec.view), None) == 0
    frames.assert_intact(f"(avc_dsp_stft_batch {geom} B={B} L={L}: frames_ws)")
    spec.assert_intact(f"(avc_dsp_stft_batch {geom} B={B} L={L}: spec)")
    return spec.view, frames.view


def run_istft(kind, geom, spec32, B=1):
    """spec32 numpy [2F][B T] -> y tensor [B][hop (T - 1)]"""
    lib, dev = backend(kind)
    n_fft, hop, win = geom
    T = spec32.shape[1] // B
    tf, y = out_buf((win, B * T), dev), out_buf((B, hop * (T - 1)), dev)
    assert lib.avc_dsp_istft_batch(P(inp(spec32, dev)), B, T, n_fft, hop, win, P(bases(kind, geom)[1]), P(tf.view), P(y.view), None) == 0
    tf.assert_intact(f"(avc_dsp_istft_batch {geom} B={B} T={T}: tf_ws)")
    y.assert_intact(f"(avc_dsp_istft_batch {geom} B={B} T={T}: y)")
    return y.view


# ---------------------------------------------------------------- 1. the DFT bases, element by element
def closed_form_bases(n_fft, win):
    """dsp.hip's two bases in float64.  cos / sin come from a table over the n_fft angles 2 pi m / n_fft with the four axis values exact
    (the kernel reduces the angle exactly and calls sincospi), everything else carries numpy's < 1e-16."""
    assert n_fft % 4 == 0
    F, n0, q = n_fft // 2 + 1, (n_fft - win) // 2, n_fft // 4          # n0: librosa's pad_center rounds the left pad DOWN
    assert n0 == int(np.flatnonzero(D.pad_center(np.ones(win), n_fft))[0])
    ang = 2.0 * np.pi * np.arange(n_fft) / n_fft
    c, s = np.cos(ang), np.sin(ang)
    c[[0, q, 2 * q, 3 * q]] = [1.0, 0.0, -1.0, 0.0]
    s[[0, q, 2 * q, 3 * q]] = [0.0, 1.0, 0.0, -1.0]
    w = D.hann_periodic(win)
    m = (np.arange(F)[:, None] * (np.arange(win)[None, :] + n0)) % n_fft          # [F][win]
    fwd = np.empty((2 * F, win))
    fwd[0::2], fwd[1::2] = w * c[m], w * -s[m]
    edge = np.zeros(F, dtype=bool)
    edge[[0, F - 1]] = True
    re = np.where(edge[:, None], c[m], 2.0 * c[m]) / n_fft
    im = np.where(edge[:, None], 0.0, -2.0 * s[m]) / n_fft
    inv = np.empty((win, 2 * F))
    inv[:, 0::2], inv[:, 1::2] = (w * re).T, (w * im).T
    return fwd, inv, w, c[m]


@pytest.mark.parametrize("geom", G_ALL, ids=ids)
@pytest.mark.parametrize("kind", KINDS)
def test_bases_equal_the_closed_form_to_one_ulp(kind, geom):
    """avc_dsp_make_basis' dense_scratch ([2F][win] forward, [win][2F] inverse): the kernel computes in double and rounds once, so
    every element is within 1 ulp of the float32 of the float64 closed form (a window tap of small weight near the edge counts like
    any other: the bar is relative to the element, not to the basis' peak)."""
    n_fft, hop, win = geom
    F = n_fft // 2 + 1
    _, _, dfwd, dinv = bases(kind, geom)
    fwd, inv, w, cm = closed_form_bases(n_fft, win)
    for name, got, ref in (("forward", dfwd, fwd), ("inverse", dinv, inv)):
        ref32 = ref.astype(F32)
        err = np.abs(got.astype(np.float64) - ref32.astype(np.float64))
        bad = err > ulp(ref32)
        assert not bad.any(), (name, geom, int(bad.sum()), np.argwhere(bad)[:4].tolist(), float((err / ulp(ref32)).max()))
    # by name: Im of DC / Nyquist is ignored by irfft, Re of DC / Nyquist counts once (every other bin twice) ...
    assert (dinv[:, 1] == 0).all() and (dinv[:, 2 * F - 1] == 0).all()
    for f in (0, F - 1):
        once = (w * cm[f] / n_fft).astype(F32)
        assert (np.abs(dinv[:, 2 * f].astype(np.float64) - once) <= ulp(once)).all(), f
        if win > 2:
            assert np.abs(dinv[:, 2 * f]).max() < 1.5 * np.abs(once).max()      # factor 1, not 2
    # ... and the forward basis' row 0 (f = 0, Re) is the periodic Hann window itself
    hann = signal.get_window("hann", win, fftbins=True).astype(F32)
    assert (np.abs(dfwd[0].astype(np.float64) - hann) <= ulp(hann)).all()
    assert dfwd[0, 0] == 0 and (win % 2 or dfwd[0, win // 2] == 1)


# ---------------------------------------------------------------- 2. STFT and iSTFT over the geometries
@pytest.mark.parametrize("geom", G_ALL, ids=ids)
@pytest.mark.parametrize("kind", KINDS)
def test_stft_istft_match_oracle_over_geometries_and_lengths(kind, geom):
    """avc_dsp_stft / avc_dsp_istft on Gaussian noise at L = n_fft/2 + 1 (the only length at which dsp_reflect's second branch reaches
    index 0), n_fft/2 + 2, 9 hop and 3 n_fft + 5; the inverse is fed the ORACLE's spectrum.  2e-5 of the reference's peak.
    Worst error / peak per geometry (STFT, iSTFT), the same on the simulator and on the MI355X but for the two figures in brackets:
      64x10x40 1.99e-7 2.04e-7 | 64x16x64 2.57e-7 2.25e-7 (MI355X 1.50e-7) | 64x7x39 2.04e-7 2.25e-7 | 64x13x51 3.21e-7 2.25e-7 |
      32x5x31 1.93e-7 1.76e-7 | 128x33x100 2.09e-7 2.25e-7 | 64x40x40 2.25e-7 3.30e-6 | (MI355X only) 2048x300x1200 7.96e-7 7.06e-7
    (hop == win divides by a window-sum-of-squares that is a single small w^2 next to the frame joints: the tightest case)."""
    n_fft, hop, win = geom
    err_f, err_i = [], []         # (np.max over them: a NaN read out of a red zone must not hide behind Python's max)
    for i, L in enumerate(lengths_of(n_fft, hop)):
        y = noise(L, 100 + i)
        ref = D.stft(y, n_fft, hop, win)
        spec, _ = run_stft(kind, geom, y)
        S = to_complex(spec)
        assert S.shape == ref.shape
        err_f.append(np.abs(S - ref).max() / np.abs(ref).max())
        if ref.shape[1] < 2:
            continue            # one frame: hop (T - 1) = 0 samples, the inverse refuses it (test_geometry_refusals)
        want = D.istft(ref, hop, win)
        back = run_istft(kind, geom, interleave(ref)).cpu().numpy().reshape(-1)
        assert back.shape == want.shape
        err_i.append(np.abs(back - want).max() / np.abs(want).max())
    worst_f, worst_i = float(np.max(err_f)), float(np.max(err_i))
    print(f"[{kind}] {ids(geom)}: STFT {worst_f:.2e} iSTFT {worst_i:.2e} of the reference's peak")
    assert worst_f <= 2e-5 and worst_i <= 2e-5, (worst_f, worst_i)


# ---------------------------------------------------------------- 3. the batch entry points
@pytest.mark.parametrize("geom", G_ALL, ids=ids)
@pytest.mark.parametrize("kind", KINDS)
def test_batch_transforms_equal_single_calls_bitwise(kind, geom):
    """avc_dsp_stft_batch / avc_dsp_istft_batch with B = 3: the utterances are column blocks of one GEMM, whose dot products are the
    ones of the B = 1 calls, so every column block (and every waveform) is bit-equal."""
    n_fft, hop, win = geom
    L = 3 * n_fft + 5
    y = noise(3 * L, 7).reshape(3, L)
    spec3, frames3 = run_stft(kind, geom, y, B=3)
    T = spec3.shape[1] // 3
    refs = []
    for b in range(3):
        spec1, frames1 = run_stft(kind, geom, y[b])
        assert np.array_equal(bits(frames3[:, b * T:(b + 1) * T]), bits(frames1)), b
        assert np.array_equal(bits(spec3[:, b * T:(b + 1) * T]), bits(spec1)), b
        refs.append(D.stft(y[b], n_fft, hop, win))
    cat = np.concatenate([interleave(r) for r in refs], axis=1)
    y3 = run_istft(kind, geom, cat, B=3)
    for b in range(3):
        assert np.array_equal(bits(y3[b]), bits(run_istft(kind, geom, interleave(refs[b]))[0])), b


# ---------------------------------------------------------------- 4. the second pass of the grid-stride loops
def filled_tail(t):
    """the last 4096 elements were written (the payload of a GuardedOutput starts as NaN)"""
    return not bool(torch.isnan(t.reshape(-1)[-4096:]).any())


@pytest.mark.parametrize("kind", KINDS)
def test_second_grid_pass_frames(kind):
    """(64, 4, 64) at L = 68,000: 17,001 frames x 64 taps = 1,088,064 frame elements in one dsp_frames_kernel launch.  The frames are a
    gather, so they are compared bitwise; the spectrum at the bar of the STFT test."""
    geom, L = (64, 4, 64), 68000
    n_fft, hop, win = geom
    y = noise(L, 11)
    spec, frames = run_stft(kind, geom, y)
    T = 1 + L // hop
    assert win * T > PASS + 4096 and filled_tail(frames) and filled_tail(spec)
    yp = np.pad(y, n_fft // 2, mode="reflect")
    want = yp[np.arange(win)[:, None] + (n_fft - win) // 2 + hop * np.arange(T)[None, :]]
    assert np.array_equal(bits(frames), want.view(np.int32))
    ref = D.stft(y, n_fft, hop, win)
    assert np.abs(to_complex(spec) - ref).max() <= 2e-5 * np.abs(ref).max()


@GPU
def test_second_grid_pass_overlap_add():
    """(64, 16, 64) with T = 65,802 frames: 1,052,816 samples from one dsp_ola_kernel launch, through avc_dsp_istft_batch, against the
    oracle's inverse of the oracle's spectrum of noise.  MI355X only: the simulator needs minutes for the 4.3 M-column GEMM in
    front of the kernel (its own second pass runs in test_second_grid_pass_frames and the element-wise cases below)."""
    geom = (64, 16, 64)
    n_fft, hop, win = geom
    L = PASS + 4096 + 16 * 9
    y = noise(L, 12)
    ref = D.stft(y, n_fft, hop, win)
    want = D.istft(ref, hop, win)
    back = run_istft("gpu", geom, interleave(ref))
    assert back.numel() == L > PASS + 4096 and filled_tail(back)
    assert np.abs(back.cpu().numpy().reshape(-1) - want).max() <= 2e-5 * np.abs(want).max()


# ---------------------------------------------------------------- 5. the element-wise kernels
SHAPES = [(1, 1), (3, 5), (33, 257), (80, 255)]
BIG = (2, (PASS + 4096) // 2 + 51)            # 2 x 526,387 = 1,052,774 elements: every kernel's second pass, rows that no pass ends on


def planted(shape, specials, ordinary, seed):
    """arrays of `shape` of ordinary values with every special value planted (one array holding them all, or, for a shape too small
    for that, one array per special value)"""
    n = shape[0] * shape[1]
    r = np.random.RandomState(seed)
    if n >= len(specials):
        a = ordinary(r, n)
        a[r.permutation(n)[:len(specials)]] = specials
        return [a.reshape(shape)]
    return [np.full(shape, v, dtype=F32) for v in specials] + [ordinary(r, n).reshape(shape)]


_PHASE_SYMBOLS = ("_Z20avc_launch_dsp_phasePKfS0_iiPfP12ihipStream_t", "_Z20avc_launch_dsp_phasePKfS0_iiPfPv")   # hipStream_t: HIP's / the simulator's


def phase_launcher(lib):
    for name in _PHASE_SYMBOLS:
        try:
            fn = getattr(lib, name)
        except AttributeError:
            continue
        fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        fn.restype = ctypes.c_int
        return fn
    raise AssertionError("avc_launch_dsp_phase(const float*, const float*, int, int, float*, hipStream_t) is not exported")


def phase_case(shape, seed):
    """est (re, im) and S that hit: est exactly 0; |est| in (0, 1e-8), one of them with a component whose square underflows; |est| = 1e-8;
    S = 0; ordinary values"""
    F, T = shape
    n = F * T
    r = np.random.RandomState(seed)
    re, im = r.randn(n).astype(F32), r.randn(n).astype(F32)
    S = np.abs(r.randn(n)).astype(F32) + F32(0.1)
    sp = [(0.0, 0.0, 1.5), (3e-9, -4e-9, 0.7), (1e-30, 6e-9, 2.0), (-2e-25, 1e-27, 1.0), (1e-8, 0.0, 1.25), (0.0, -1e-8, 0.5), (0.3, -0.4, 0.0),
          (6e-9, 8e-9, 3.0)]
    if n >= len(sp):
        pos = r.permutation(n)[:len(sp)]
        for p, (a, b, c) in zip(pos, sp):
            re[p], im[p], S[p] = a, b, c
        return [(re, im, S)]
    return [(np.full(n, a, F32), np.full(n, b, F32), np.full(n, c, F32)) for a, b, c in sp] + [(re, im, S)]


def check_phase(kind, shape, re, im, S):
    lib, dev = backend(kind)
    launch = phase_launcher(lib)
    F, T = shape
    est = np.stack([re.reshape(F, T), im.reshape(F, T)], axis=1).reshape(2 * F, T)
    Sg = inp(S.reshape(F, T), dev)
    out = out_buf((2 * F, T), dev)
    assert launch(P(inp(est, dev)), P(Sg), F, T, P(out.view), None) == 0
    out.assert_intact(f"(dsp_phase_kernel {shape})")
    got = out.view.cpu().numpy().reshape(F, 2, T)
    sc32 = S / np.maximum(F32(1e-8), np.sqrt(re * re + im * im))
    same32 = np.stack([(re * sc32).reshape(F, T), (im * sc32).reshape(F, T)], axis=1)
    re64, im64, S64 = re.astype(np.float64), im.astype(np.float64), S.astype(np.float64)
    sc64 = S64 / np.maximum(1e-8, np.hypot(re64, im64))
    ref = np.stack([(re64 * sc64).reshape(F, T), (im64 * sc64).reshape(F, T)], axis=1)
    ratio = worst(got, ref, fp32_bar(ref, same32, relative=True))
    # est == nullptr, the first Griffin-Lim iteration: X = S, real
    out0 = out_buf((2 * F, T), dev)
    assert launch(None, P(Sg), F, T, P(out0.view), None) == 0
    out0.assert_intact(f"(dsp_real_to_complex_kernel {shape})")
    got0 = out0.view.cpu().contiguous().view(torch.int32).numpy().reshape(F, 2, T)
    assert np.array_equal(got0[:, 0], S.reshape(F, T).view(np.int32)) and (got0[:, 1] == 0).all()
    return ratio, out, out0


@pytest.mark.parametrize("shape", SHAPES + [BIG], ids=ids)
@pytest.mark.parametrize("kind", KINDS)
def test_phase_kernel(kind, shape):
    """X = S est / max(1e-8, |est|) (dsp_phase_kernel) and X = S (est == nullptr: imaginary rows exactly 0, real rows bit-equal to S).
    An est of exactly 0 gives exactly 0; below the clamp the quotient is S / 1e-8 whatever the squares underflow to.
    Worst |got - ref| / bar: 0.25 on the simulator, 0.25 on the MI355X."""
    ratios = []
    for re, im, S in phase_case(shape, 31):
        ratio, out, out0 = check_phase(kind, shape, re, im, S)
        ratios.append(ratio)
        zero = (re == 0) & (im == 0)
        got = out.view.cpu().numpy().reshape(shape[0], 2, shape[1])
        assert (got[:, 0].reshape(-1)[zero] == 0).all() and (got[:, 1].reshape(-1)[zero] == 0).all()
        if shape == BIG:
            assert 2 * shape[0] * shape[1] > shape[0] * shape[1] > PASS + 4096 and filled_tail(out.view) and filled_tail(out0.view)
    print(f"[{kind}] phase {shape}: worst |got - ref| / bar {np.max(ratios):.3f}")
    assert np.max(ratios) <= 1.0, ratios


# (re, im) whose magnitude is exact in fp32: the squares and their sum are representable, sqrtf is correctly rounded
MAG_EXACT = [(0.0, 0.0, 0.0), (3.0, 4.0, 5.0), (-4.0, 3.0, 5.0), (0.375, -0.5, 0.625), (5.0, 12.0, 13.0), (-24576.0, 32768.0, 40960.0),
             (0.0, -2.5, 2.5)]


@pytest.mark.parametrize("shape", SHAPES + [BIG], ids=ids)
@pytest.mark.parametrize("kind", KINDS)
def test_magnitude_kernel(kind, shape):
    """avc_dsp_magnitude: sqrt(re^2 + im^2).  0 and the 3-4-5 triples (scaled, signed, 5-12-13) are exact.
    Worst |got - ref| / bar: 0.25 on the simulator, 0.31 on the MI355X."""
    lib, dev = backend(kind)
    F, T = shape
    n = F * T
    r = np.random.RandomState(32)
    re, im = ((r.randn(n) * np.exp(3 * r.randn(n))).astype(F32) for _ in range(2))
    cases = [(re, im, None)]
    if n >= len(MAG_EXACT):
        pos = r.permutation(n)[:len(MAG_EXACT)]
        re[pos], im[pos] = [a for a, _, _ in MAG_EXACT], [b for _, b, _ in MAG_EXACT]
        cases = [(re, im, pos)]
    else:
        cases += [(np.full(n, a, F32), np.full(n, b, F32), np.arange(n)) for a, b, _ in MAG_EXACT]
    ratios = []
    for re, im, pos in cases:
        spec = np.stack([re.reshape(F, T), im.reshape(F, T)], axis=1).reshape(2 * F, T)
        out = out_buf((F, T), dev)
        assert lib.avc_dsp_magnitude(P(inp(spec, dev)), 2 * (F - 1), T, P(out.view), None) == 0
        out.assert_intact(f"(avc_dsp_magnitude {shape})")
        got = out.view.cpu().numpy().reshape(-1)
        ref = np.hypot(re.astype(np.float64), im.astype(np.float64))
        ratios.append(worst(got, ref, fp32_bar(ref, np.sqrt(re * re + im * im), relative=True)))
        if pos is not None:
            assert np.array_equal(got[pos], ref[pos].astype(F32)) and (ref[pos] == ref[pos].astype(F32)).all(), (got[pos], ref[pos])
        if shape == BIG:
            assert n > PASS + 4096 and filled_tail(out.view)
    print(f"[{kind}] magnitude {shape}: worst |got - ref| / bar {np.max(ratios):.3f}")
    assert np.max(ratios) <= 1.0, ratios


def db_norm32(x, ref_db, max_db):
    db = F32(20) * np.log10(np.maximum(F32(1e-5), x))
    return np.minimum(np.maximum((db - F32(ref_db) + F32(max_db)) / F32(max_db), F32(1e-8)), F32(1))


def db_norm64(x, ref_db, max_db):
    """utils.py:76-81 as the oracle's get_spectrograms states it"""
    return np.clip((20 * np.log10(np.maximum(1e-5, x.astype(np.float64))) - ref_db + max_db) / max_db, 1e-8, 1)


DB_SPECIALS = [0.0, 1e-6, 1e-5, 1.0000001e-5, 1.0, 1e6]


# (ref_db, max_db): the stock pair, under which the 1e-5 floor (-100 dB -> -0.2) hides behind the 1e-8 clip, and a pair that shows it
# (-100 dB -> 0.2: a floor of 1e-6 would give 0.0 -> 1e-8)
@pytest.mark.parametrize("ref_max", [(REF_DB, MAX_DB), (-20.0, 100.0)], ids=ids)
@pytest.mark.parametrize("shape", SHAPES + [BIG], ids=ids)
@pytest.mark.parametrize("kind", KINDS)
def test_db_normalize_kernel(kind, shape, ref_max):
    """avc_dsp_db_normalize: out[t][c] = clip((20 log10(max(1e-5, in[c][t])) - ref_db + max_db) / max_db, 1e-8, 1), transposed.
    0, 1e-6 and 1e-5 sit on the floor and agree bitwise; 1e6 clips to exactly 1; nothing is below (float32) 1e-8.
    Worst |got - ref| / bar: 0.32 on the simulator, 0.57 on the MI355X."""
    lib, dev = backend(kind)
    C, T = shape
    ref_db, max_db = ref_max

    def ordinary(r, n):
        return np.exp(r.uniform(np.log(1e-6), np.log(1e3), n)).astype(F32)
    ratios = []
    for x in planted(shape, np.array(DB_SPECIALS, dtype=F32), ordinary, 33):
        out = out_buf((T, C), dev)
        assert lib.avc_dsp_db_normalize(P(inp(x, dev)), C, T, ref_db, max_db, P(out.view), None) == 0
        out.assert_intact(f"(avc_dsp_db_normalize {shape})")
        got = out.view.cpu().numpy()
        assert got.shape == (T, C)
        ref = db_norm64(x, ref_db, max_db).T                                           # [C][T] -> [T][C]
        ratios.append(worst(got, ref, fp32_bar(ref, db_norm32(x, ref_db, max_db).T, relative=False)))
        assert (got >= F32(1e-8)).all() and (got <= 1).all()
        xt = x.T
        assert (got[xt == F32(1e6)] == 1).all()
        floor = got[xt <= F32(1e-5)]
        if floor.size:
            want = 1e-8 if ref_db > 0 else 0.2
            assert (floor.view(np.int32) == floor.view(np.int32)[0]).all() and abs(float(floor[0]) - want) <= 1e-7
        if C != T and C * T >= len(DB_SPECIALS):      # the transpose by name: the 1e6 planted at in[c][t] is the 1 at flat t C + c
            c, t = np.argwhere(x == F32(1e6))[0]
            assert got.reshape(-1)[t * C + c] == 1 and ref[t, c] == 1
        if shape == BIG:
            assert C * T > PASS + 4096 and filled_tail(out.view)
    print(f"[{kind}] dB-normalise {shape} {ref_max}: worst |got - ref| / bar {np.max(ratios):.3f}")
    assert np.max(ratios) <= 1.0, ratios


def denorm32(x, ref_db, max_db):
    v = np.minimum(np.maximum(x, F32(0)), F32(1)) * F32(max_db) - F32(max_db) + F32(ref_db)
    return np.power(F32(10), v * F32(0.05))


def denorm64(x, ref_db, max_db):
    """utils.py:95-98 as the oracle's melspectrogram2wav states it"""
    return np.power(10.0, ((np.clip(x.astype(np.float64), 0, 1) * max_db) - max_db + ref_db) * 0.05)


DENORM_SPECIALS = [-0.5, 0.0, 1.0, 1.5]


@pytest.mark.parametrize("shape", SHAPES + [BIG], ids=ids)
@pytest.mark.parametrize("kind", KINDS)
def test_denormalize_kernel(kind, shape):
    """avc_dsp_denormalize_amp: out[c][t] = 10^(0.05 (clip(in[t][c], 0, 1) max_db - max_db + ref_db)), transposed back.  An input below 0
    gives the bits of the result at 0, one above 1 the bits of the result at 1.
    Worst |got - ref| / bar: 0.25 on the simulator, 0.25 on the MI355X."""
    lib, dev = backend(kind)
    C, T = shape
    ratios, at = [], {}
    for x in planted((T, C), np.array(DENORM_SPECIALS, dtype=F32), lambda r, n: r.uniform(-0.1, 1.1, n).astype(F32), 34):
        out = out_buf((C, T), dev)
        assert lib.avc_dsp_denormalize_amp(P(inp(x, dev)), C, T, REF_DB, MAX_DB, P(out.view), None) == 0
        out.assert_intact(f"(avc_dsp_denormalize_amp {shape})")
        got = out.view.cpu().numpy()
        ref = denorm64(x, REF_DB, MAX_DB).T
        ratios.append(worst(got, ref, fp32_bar(ref, denorm32(x, REF_DB, MAX_DB).T, relative=True)))
        for v in DENORM_SPECIALS:
            sel = got[x.T == F32(v)]
            if sel.size:
                at.setdefault(v, set()).update(sel.view(np.int32).tolist())
        assert len(set(got[x.T <= 0].view(np.int32).tolist())) <= 1 and len(set(got[x.T >= 1].view(np.int32).tolist())) <= 1
        if shape == BIG:
            assert C * T > PASS + 4096 and filled_tail(out.view)
    assert at[-0.5] == at[0.0] and at[1.5] == at[1.0] and len(at[0.0]) == 1 and len(at[1.0]) == 1, at
    print(f"[{kind}] denormalise {shape}: worst |got - ref| / bar {np.max(ratios):.3f}")
    assert np.max(ratios) <= 1.0, ratios


@pytest.mark.parametrize("L", [1, 2, 255, 33 * 257, PASS + 4096 + 101])
@pytest.mark.parametrize("kind", KINDS)
def test_preemphasis_kernel(kind, L):
    """avc_dsp_preemphasis: out[0] = y[0], out[i] = y[i] - a y[i-1].  a = 0 is a bit-equal copy; a = 0.97 at the fp32 bar (absolute: the
    difference cancels); y == out is refused with -1 and writes nothing.
    Worst |got - ref| / bar: 0.25 on the simulator, 0.25 on the MI355X."""
    lib, dev = backend(kind)
    y = noise(L, 35)
    yg = inp(y, dev)
    out = out_buf((L,), dev)
    assert lib.avc_dsp_preemphasis(P(yg), L, 0.0, P(out.view), None) == 0
    out.assert_intact("(avc_dsp_preemphasis a=0)")
    assert np.array_equal(bits(out.view), y.view(np.int32))
    out = out_buf((L,), dev)
    assert lib.avc_dsp_preemphasis(P(yg), L, 0.97, P(out.view), None) == 0
    out.assert_intact("(avc_dsp_preemphasis a=0.97)")
    y64 = y.astype(np.float64)
    ref = np.append(y64[0], y64[1:] - 0.97 * y64[:-1])                    # utils.py:60 as the oracle states it
    same32 = np.append(y[0], y[1:] - F32(0.97) * y[:-1]).astype(F32)
    got = out.view.cpu().numpy()
    assert got[0] == y[0]
    ratio = worst(got, ref, fp32_bar(ref, same32, relative=False))
    if L > PASS:
        assert filled_tail(out.view)
    inplace = GuardedOutput((L,), device=dev, init=torch.from_numpy(y))
    before = snapshot(inplace)
    assert lib.avc_dsp_preemphasis(P(inplace.view), L, 0.97, P(inplace.view), None) == -1
    assert untouched(inplace, before)
    print(f"[{kind}] pre-emphasis L={L}: worst |got - ref| / bar {ratio:.3f}")
    assert ratio <= 1.0


# ---------------------------------------------------------------- 6. de-emphasis
DEEMPH_L = [1, 2, 1023, 1024, 1025, 2047, 2049, 5003]     # one workgroup of 1024 lanes: fewer samples than lanes, one each, runs of 2, 3 and 5


def run_deemph(kind, x, a, inplace=False):
    lib, dev = backend(kind)
    L = len(x)
    if inplace:
        out = GuardedOutput((L,), device=dev, init=torch.from_numpy(x))
        src = out.view
    else:
        out, src = out_buf((L,), dev), inp(x, dev)
    assert lib.avc_dsp_deemphasis(P(src), L, a, P(out.view), None) == 0
    out.assert_intact(f"(avc_dsp_deemphasis L={L} a={a} inplace={inplace})")
    return out.view.cpu().numpy()


@pytest.mark.parametrize("L", DEEMPH_L)
@pytest.mark.parametrize("kind", KINDS)
def test_deemphasis_against_lfilter(kind, L):
    """avc_dsp_deemphasis against scipy.signal.lfilter([1], [1, -a]) in float64 at a = 0.97, 0, -0.5: 2e-5 of the peak; a = 0 copies the
    input bit for bit.  a = 0.999 (a pole 30 times closer to the unit circle): 4 x the error of the plain sequential float32
    recurrence (with the float32 coefficient the library receives) on the same input.  Worst error / bar over the lengths: 0.53 on the
    simulator and on the MI355X (L = 2049), 8.4e-6 of the peak.  Most of both errors is the rounding of 0.999 to float32; against the
    filter with the ROUNDED coefficient (printed, not asserted) the blocked scan is up to 6.8 times the sequential recurrence
    (1.2e-4 against 1.8e-5 at L = 2049, 4.4e-6 of the peak): its carry weights a^(j+1) are built by repeated fp32 multiplication."""
    x = noise(L, 40 + L % 7)
    x64 = x.astype(np.float64)
    for a in (0.97, 0.0, -0.5):
        ref = signal.lfilter([1], [1, -a], x64)
        got = run_deemph(kind, x, a)
        assert np.abs(got - ref).max() <= 2e-5 * np.abs(ref).max(), (a, np.abs(got - ref).max() / np.abs(ref).max())
        if a == 0.0:
            assert np.array_equal(got.view(np.int32), x.view(np.int32))
    a32 = F32(0.999)                                          # what the library receives (and the float32 recurrence uses)
    ref = signal.lfilter([1], [1, -0.999], x64)
    seq, v = np.empty(L, F32), F32(0)
    for i in range(L):
        v = F32(x[i] + F32(a32 * v))
        seq[i] = v
    bar = 4 * np.abs(seq.astype(np.float64) - ref).max()
    got = run_deemph(kind, x, 0.999)
    err = np.abs(got - ref).max()
    # reported, not asserted: the same two errors against the filter with the ROUNDED coefficient, i.e. the arithmetic alone
    ref32 = signal.lfilter([1], [1, -float(a32)], x64)
    e_k, e_s = np.abs(got - ref32).max(), np.abs(seq.astype(np.float64) - ref32).max()
    print(f"[{kind}] de-emphasis L={L} a=0.999: error {err:.3e} = {err / np.abs(ref).max():.2e} of the peak, bar {bar:.3e}, ratio "
          f"{err / bar if bar else 0.0:.3f}; arithmetic alone: kernel {e_k:.3e}, sequential float32 {e_s:.3e}")
    assert err <= bar, (err, bar)


@pytest.mark.parametrize("kind", KINDS)
def test_deemphasis_in_place_equals_out_of_place(kind):
    """x == out at L = 2049 (runs of 3): every lane reads x[i] before it writes out[i] and the carry pass touches out alone."""
    x = noise(2049, 41)
    assert np.array_equal(run_deemph(kind, x, 0.97, inplace=True).view(np.int32), run_deemph(kind, x, 0.97).view(np.int32))


# ---------------------------------------------------------------- 7. frame power and trim
def oracle_mse(y, frame_length, hop):
    """the frame powers of oracle/dsp_oracle.py's trim (its first four lines)"""
    yp = np.pad(np.asarray(y, dtype=np.float64), frame_length // 2, mode="reflect")
    n_frames = 1 + (len(yp) - frame_length) // hop
    idx = np.arange(frame_length)[:, None] + hop * np.arange(n_frames)[None, :]
    return np.mean(yp[idx] ** 2, axis=0)


def margin_db(y, top_db, frame_length, hop):
    """distance of the frame closest to trim's threshold from it, in dB"""
    mse = oracle_mse(y, frame_length, hop)
    db = 10.0 * np.log10(np.maximum(1e-10, mse)) - 10.0 * np.log10(np.maximum(1e-10, mse.max()))
    return float(np.abs(db + top_db).min())


_DSP = {}


def small_dsp(kind):
    if kind not in _DSP:
        lib, dev = backend(kind)
        hp = D.small_hyperparams()
        _DSP[kind] = PD.MelDSP(type("HP", (PD.Hyperparams,), {k: getattr(hp, k) for k in ("sr", "n_fft", "hop_length", "win_length", "n_mels", "n_iter")}),
                               device=dev, lib=lib)
    return _DSP[kind]


@pytest.mark.parametrize("frame_length", [2, 7, 255, 256, 257, 2048])
@pytest.mark.parametrize("kind", KINDS)
def test_frame_power_and_trim(kind, frame_length):
    """avc_dsp_frame_power over frame lengths around the 256 lanes of its block (fewer taps than lanes, one each, one more, 8 each), hops
    1, 3, 512, at the shortest accepted signal (L = frame_length/2 + 1: the reflection reaches index 0) and 3 frame_length + 1: 1e-5
    relative to the oracle's frame powers.  L = frame_length/2 is refused with -6.  MelDSP.trim picks the oracle's indices on the same
    signals (Gaussian noise: every frame is far above the -60 dB threshold, asserted)."""
    lib, dev = backend(kind)
    dsp = small_dsp(kind)
    for L in (frame_length // 2 + 1, 3 * frame_length + 1):
        y = noise(L, 50 + frame_length % 11)
        yg = inp(y, dev)
        for hop in (1, 3, 512):
            nf = 1 + (L + 2 * (frame_length // 2) - frame_length) // hop        # what fits the padded signal (librosa's framing)
            out = out_buf((nf,), dev)
            assert lib.avc_dsp_frame_power(P(yg), L, frame_length, hop, P(out.view), None) == 0
            out.assert_intact(f"(avc_dsp_frame_power L={L} frame_length={frame_length} hop={hop})")
            ref = oracle_mse(y, frame_length, hop)
            assert ref.shape == (nf,)
            np.testing.assert_allclose(out.view.cpu().numpy(), ref, rtol=1e-5, atol=0)
            assert margin_db(y, 60, frame_length, hop) > 3
            got, idx = dsp.trim(y, top_db=60, frame_length=frame_length, hop_length=hop)
            want, widx = D.trim(y, top_db=60, frame_length=frame_length, hop_length=hop)
            assert idx == widx and np.array_equal(got.cpu().numpy(), want)
    L = frame_length // 2
    out = out_buf((L + 1,), dev)
    before = snapshot(out)
    assert lib.avc_dsp_frame_power(P(inp(noise(L, 1), dev)), L, frame_length, 1, P(out.view), None) == -6
    assert untouched(out, before)


def trim_signals(frame_length, hop):
    """name -> (signal, top_db): 10 frames, the last one partial"""
    L = 9 * hop + hop // 10
    quiet = (1e-4 * np.random.RandomState(60).randn(L)).astype(F32)            # -80 dB under the bursts
    first, last = quiet.copy(), quiet.copy()
    n = min(100, frame_length // 2)
    first[:n] += 1.0                                                         # frame 0 is samples [-frame_length/2, frame_length/2)
    last[9 * hop - n // 2:9 * hop + n // 2] += 1.0                             # frame 9 is centred on sample 9 hop
    return {"zero": np.zeros(L, F32), "constant": np.full(L, 0.5, F32), "first": first, "last": last}


@pytest.mark.parametrize("frames", [(256, 512), (2048, 512)], ids=ids)
@pytest.mark.parametrize("kind", KINDS)
def test_trim_of_silence_constant_and_bursts(kind, frames):
    """MelDSP.trim against the oracle's trim on an all-zero signal, a constant one, and one loud burst in the first / the last frame
    over a floor 80 dB below (frames of 256 at hop 512 do not overlap: exactly one frame is loud; frames of 2048 overlap: the burst's
    neighbours are loud too).  No frame power is within 3 dB of the threshold (asserted), so fp32 cannot flip an index.

    The all-zero signal: every frame power is clamped to 1e-10 and so is the maximum they are compared with, as librosa's power_to_db
    does with `amin`, so every frame is 0 dB from the loudest and NOTHING is cut: the oracle returns the whole signal and (0, L), and
    so must the product (its `(0, 0)` / empty branch needs a signal without a single finite frame power)."""
    frame_length, hop = frames
    dsp = small_dsp(kind)
    sig = trim_signals(frame_length, hop)
    L = len(sig["zero"])
    idxs = {}
    for name, y in sig.items():
        assert margin_db(y, 60, frame_length, hop) > 3, name
        got, idx = dsp.trim(y, top_db=60, frame_length=frame_length, hop_length=hop)
        want, widx = D.trim(y, top_db=60, frame_length=frame_length, hop_length=hop)
        assert idx == widx and got.numel() == len(want) and np.array_equal(got.cpu().numpy(), want), (name, idx, widx)
        idxs[name] = idx
    assert idxs["zero"] == (0, L) and idxs["constant"] == (0, L)
    assert idxs["first"][0] == 0 and idxs["first"][1] < L and idxs["last"][0] > 0 and idxs["last"][1] == L
    if frame_length <= hop:
        assert idxs["first"] == (0, hop) and idxs["last"] == (9 * hop, L)


# ---------------------------------------------------------------- 8. ragged Griffin-Lim
def ragged_lengths(n_fft, hop):
    Tmin = (n_fft // 2) // hop + 2                     # the fewest frames with hop (T - 1) > n_fft / 2
    assert hop * (Tmin - 1) > n_fft // 2 >= hop * (Tmin - 2)
    return Tmin, [Tmin, 57, Tmin, Tmin + 1, 23, Tmin, 40, Tmin + 2, 31, Tmin, Tmin, Tmin + 19, Tmin, 64, Tmin, Tmin + 5, Tmin]


def geom_hp(geom, n_mels=8):
    return D.small_hyperparams(n_fft=geom[0], hop=geom[1], win=geom[2], n_mels=n_mels)


def run_ragged(kind, geom, S, toff_host, n_iter, toff_dev=None, expect=0):
    """avc_dsp_griffin_lim_ragged on S [F][Ttot]; returns the packed waveforms (or, for a refusal, checks that nothing was written)"""
    lib, dev = backend(kind)
    n_fft, hop, win = geom
    B, Ttot = len(toff_host) - 1, S.shape[1]
    fwd, inv = bases(kind, geom)[:2]
    toff_host = np.ascontiguousarray(toff_host, dtype=np.int32)
    toff = torch.from_numpy(toff_host if toff_dev is None else np.ascontiguousarray(toff_dev, dtype=np.int32)).to(dev)
    ws = out_buf((lib.avc_dsp_griffin_lim_ws_floats(Ttot, n_fft, hop, win),), dev)
    y = out_buf((hop * (Ttot - B),), dev)
    before = snapshot(y), snapshot(ws)
    rc = lib.avc_dsp_griffin_lim_ragged(P(inp(S, dev)), P(toff), ctypes.c_void_p(toff_host.ctypes.data), B, Ttot, n_fft, hop, win, n_iter,
                                        P(fwd), P(inv), P(ws.view), P(y.view), None)
    assert rc == expect, (rc, expect)
    ws.assert_intact(f"(avc_dsp_griffin_lim_ragged {geom}: ws)")
    y.assert_intact(f"(avc_dsp_griffin_lim_ragged {geom}: y)")
    if expect != 0:
        assert untouched(y, before[0]) and untouched(ws, before[1])
        return None
    return y.view.cpu().numpy()


@pytest.mark.parametrize("geom", G_RAGGED, ids=ids)
@pytest.mark.parametrize("kind", KINDS)
def test_ragged_griffin_lim_of_seventeen_utterances(kind, geom):
    """B = 17 utterances, the shortest accepted one first, last and in between (dsp_find's binary search over toff sees runs of equal
    and of very unequal lengths): after 2 iterations through melspectrogram2wav_batch every waveform is BIT-equal to its
    single-utterance call; without iterations avc_dsp_griffin_lim_ragged is within 2e-5 of the peak of the oracle's griffin_lim (the
    project's bar for the transforms: the de-emphasis behind them in melspectrogram2wav has a bar of its own above)."""
    lib, dev = backend(kind)
    n_fft, hop, win = geom
    hp = geom_hp(geom)
    dsp = PD.MelDSP(type("HP", (PD.Hyperparams,), {k: getattr(hp, k) for k in ("sr", "n_fft", "hop_length", "win_length", "n_mels", "n_iter")}),
                    device=dev, lib=lib)
    Tmin, Ts = ragged_lengths(n_fft, hop)
    r = np.random.RandomState(70)
    mels = [r.uniform(0.3, 1.0, (T, hp.n_mels)).astype(F32) for T in Ts]
    many = dsp.melspectrogram2wav_batch(mels, do_trim=False, n_iter=2)
    assert len(many) == len(Ts)
    for b, m in enumerate(mels):
        one = dsp.melspectrogram2wav(m, do_trim=False, n_iter=2)
        assert one.shape == many[b].shape == (hop * (Ts[b] - 1),) and np.array_equal(one.view(np.int32), many[b].view(np.int32)), b
    F = n_fft // 2 + 1
    S = np.abs(r.randn(F, sum(Ts))).astype(F32) + F32(0.05)
    toff = np.concatenate([[0], np.cumsum(Ts)])
    y = run_ragged(kind, geom, S, toff, 0)
    errs = []
    for b, T in enumerate(Ts):
        want = D.griffin_lim(S[:, toff[b]:toff[b + 1]].astype(np.float64), hp, n_iter=0)
        got = y[hop * (toff[b] - b):hop * (toff[b] - b) + hop * (T - 1)]
        errs.append(np.abs(got - want).max() / np.abs(want).max())
    worst_r = float(np.max(errs))
    print(f"[{kind}] ragged Griffin-Lim {ids(geom)}: worst error {worst_r:.2e} of the peak")
    assert worst_r <= 2e-5


@pytest.mark.parametrize("kind", KINDS)
def test_ragged_griffin_lim_refusals(kind):
    """avc_dsp_griffin_lim_ragged validates the HOST offsets before it launches anything: output and workspace keep their fill."""
    geom = SMALL
    n_fft, hop, win = geom
    Tmin, _ = ragged_lengths(n_fft, hop)
    Ts = [Tmin, 9, Tmin + 1]
    good = np.concatenate([[0], np.cumsum(Ts)])
    Ttot = int(good[-1])
    S = np.abs(noise((n_fft // 2 + 1) * Ttot, 71)).reshape(-1, Ttot)
    assert run_ragged(kind, geom, S, good, 0) is not None
    bad = good.copy(); bad[0] = 1
    run_ragged(kind, geom, S, bad, 0, toff_dev=good, expect=-1)                    # toff_host[0] != 0
    bad = good.copy(); bad[-1] = Ttot - 1
    run_ragged(kind, geom, S, bad, 0, toff_dev=good, expect=-1)                    # toff_host[B] != Ttot
    bad = good.copy(); bad[1], bad[2] = good[2], good[1]
    run_ragged(kind, geom, S, bad, 0, toff_dev=good, expect=-1)                    # a decreasing pair
    bad = np.array([0, 1, Ttot - Tmin, Ttot])
    run_ragged(kind, geom, S, bad, 0, toff_dev=good, expect=-1)                    # T_b = 1
    bad = np.array([0, Tmin - 1, Ttot - Tmin, Ttot])
    run_ragged(kind, geom, S, bad, 0, toff_dev=good, expect=-6)                    # hop (T_b - 1) <= n_fft / 2
    run_ragged(kind, geom, S, good, -1, expect=-1)


# ---------------------------------------------------------------- 9. geometry refusals
BAD_GEOMETRIES = {"odd n_fft": (63, 10, 40), "n_fft = 2": (2, 1, 2), "win > n_fft": (64, 10, 65), "win = 1": (64, 1, 1), "hop = 0": (64, 0, 40),
                  "hop > win": (64, 41, 40)}


@pytest.mark.parametrize("kind", KINDS)
def test_geometry_refusals(kind):
    """Every entry point that takes a geometry returns -1 for one dsp_geom_ok rejects, for a null pointer in any pointer argument, for
    T = 1 frames to invert and for n_iter = -1 -- before it launches anything: all caller memory keeps its fill."""
    lib, dev = backend(kind)
    n_fft, hop, win = SMALL
    fwd, inv = bases(kind, SMALL)[:2]
    B, L = 2, 3 * n_fft + 5
    T = 1 + L // hop
    F2 = n_fft + 2
    yin, spec_in = inp(noise(B * L, 80).reshape(B, L), dev), inp(noise(F2 * B * T, 81).reshape(F2, B * T), dev)
    S_in = inp(np.abs(noise((F2 // 2) * B * T, 82)).reshape(F2 // 2, B * T), dev)
    n = max(F2 * B * T, B * L, int(lib.avc_dsp_griffin_lim_ws_floats(B * T, n_fft, hop, win)), int(lib.avc_dsp_basis_floats(n_fft, win, 0)))
    bufs = [out_buf((n,), dev) for _ in range(2)]
    a, b = bufs
    before = [snapshot(g) for g in bufs]

    def refused(rc, what):
        assert rc == -1, (what, rc)
        for g, s in zip(bufs, before):
            assert untouched(g, s), what

    def stft(g=SMALL, y=yin, basis=fwd, frames=a.view, spec=b.view):
        return lib.avc_dsp_stft_batch(P(y), L, B, g[0], g[1], g[2], P(basis), P(frames), P(spec), None)

    def istft(g=SMALL, spec=spec_in, basis=inv, tf=a.view, y=b.view, T=T):
        return lib.avc_dsp_istft_batch(P(spec), B, T, g[0], g[1], g[2], P(basis), P(tf), P(y), None)

    def gl(g=SMALL, S=S_in, bf=fwd, bi=inv, ws=a.view, y=b.view, n_iter=1, T=T):
        return lib.avc_dsp_griffin_lim_batch(P(S), B, T, g[0], g[1], g[2], n_iter, P(bf), P(bi), P(ws), P(y), None)

    for name, g in BAD_GEOMETRIES.items():
        for inverse in (0, 1):
            refused(lib.avc_dsp_make_basis(g[0], g[1], g[2], inverse, P(a.view), P(b.view), None), f"make_basis {name}")
        refused(stft(g=g), f"stft_batch {name}")
        refused(istft(g=g), f"istft_batch {name}")
        refused(gl(g=g), f"griffin_lim_batch {name}")
    for fn, args in ((stft, ("y", "basis", "frames", "spec")), (istft, ("spec", "basis", "tf", "y")), (gl, ("S", "bf", "bi", "ws", "y"))):
        for arg in args:
            refused(fn(**{arg: None}), f"{fn.__name__} {arg} = nullptr")
    refused(lib.avc_dsp_make_basis(n_fft, hop, win, 0, None, P(b.view), None), "make_basis dense_scratch = nullptr")
    refused(lib.avc_dsp_make_basis(n_fft, hop, win, 0, P(a.view), None, None), "make_basis packed = nullptr")
    refused(istft(T=1), "istft_batch T = 1")
    refused(gl(T=1), "griffin_lim_batch T = 1")
    refused(gl(n_iter=-1), "griffin_lim_batch n_iter = -1")
    assert stft() == 0 and istft() == 0 and gl() == 0          # the same calls with nothing wrong are accepted
    for g in bufs:
        g.assert_intact("(accepted calls)")


