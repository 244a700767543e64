"""The packed, many-utterance kernels of the two audio edges (csrc/dsp_ragged.hip; entry points in csrc/dsp_api.hip), each through the
C ABI against the single-utterance entry point called per utterance:

  avc_dsp_frame_power_ragged      ==  avc_dsp_frame_power per utterance
  avc_dsp_frames_ragged_preemph   ==  avc_dsp_preemphasis, then the frames workspace of avc_dsp_stft, per (trimmed) utterance
  avc_dsp_deemphasis_ragged       ==  avc_dsp_deemphasis per utterance

BITWISE: each pair of kernels calls one shared inline (csrc/dsp_shared.h) on the same samples, so there is no tolerance.  The framing
is also held against float64 (numpy.pad(reflect) of the pre-emphasised sub-run) at the pre-emphasis bar of tests/test_dsp_ops.py
(`fp32_bar`, absolute).  Outputs sit in sentinel red zones, waveforms in NaN red zones (tests/redzone.py); refused calls must leave
every output dword as it was.  Geometries: G_RAGGED of tests/test_dsp_ops.py, plus the stock one on the MI355X.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests.emu_util import KINDS, P, backend
from tests.test_dsp_ops import F32, G_RAGGED, PASS, STOCK, filled_tail, fp32_bar, ids, inp, noise, out_buf, run_stft, snapshot, untouched, worst

GPU = pytest.mark.gpu
GEOMS = G_RAGGED + [pytest.param(STOCK, marks=GPU)]
A = 0.97


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def lengths5(n_fft, hop):
    """the shortest accepted length, one more, two equal ones, one that is no multiple of the hop"""
    return [n_fft // 2 + 1, n_fft // 2 + 2, 9 * hop, 9 * hop, 3 * n_fft + 5]


def H(a):
    return ctypes.c_void_p(a.ctypes.data)


def table(a, dtype, dev):
    """(host array, device tensor) of an offset table"""
    h = np.ascontiguousarray(a, dtype=dtype)
    return h, torch.from_numpy(h.copy()).to(dev)


def offsets(lengths):
    return np.concatenate([[0], np.cumsum(lengths)])


def packed_noise(lengths, seed):
    return [noise(n, seed + 13 * i) for i, n in enumerate(lengths)]


# ---------------------------------------------------------------- frame powers
def power_frames(L, frame_length, hop):
    return 1 + (L - (frame_length & 1)) // hop


def run_power_ragged(kind, ys, frame_length, hop, woff_host=None, poff_host=None, expect=0):
    lib, dev = backend(kind)
    lengths = [len(y) for y in ys]
    woff_h, woff = table(offsets(lengths), np.int64, dev)
    poff_h, poff = table(offsets([power_frames(n, frame_length, hop) for n in lengths]), np.int32, dev)
    if woff_host is not None:
        woff_h = np.ascontiguousarray(woff_host, dtype=np.int64)
    if poff_host is not None:
        poff_h = np.ascontiguousarray(poff_host, dtype=np.int32)
    out = out_buf((int(poff[-1]),), dev)
    before = snapshot(out)
    src = inp(np.concatenate(ys), dev)          # (held in a name: the library reads it after the argument list is built)
    rc = lib.avc_dsp_frame_power_ragged(P(src), P(woff), H(woff_h), P(poff), H(poff_h), len(ys), frame_length, hop, P(out.view), None)
    assert rc == expect, (rc, expect)
    out.assert_intact(f"(avc_dsp_frame_power_ragged frame_length={frame_length} hop={hop} lengths={lengths})")
    if expect != 0:
        assert untouched(out, before)
        return None
    return out.view, poff_h


@pytest.mark.parametrize("geom", GEOMS, ids=ids)
@pytest.mark.parametrize("kind", KINDS)
def test_frame_power_ragged_equals_single_calls_bitwise(kind, geom):
    """B = 1 and the B = 5 set, frame lengths n_fft and n_fft - 1 (the odd-frame_length count), hops hop and 1: every utterance's powers
    are the bits of avc_dsp_frame_power on that utterance alone, at out[poff[b] ..]."""
    lib, dev = backend(kind)
    n_fft, hop, _ = geom
    for lengths in ([3 * n_fft + 5], lengths5(n_fft, hop)):
        ys = packed_noise(lengths, 200)
        for frame_length in (n_fft, n_fft - 1):
            for h in ((hop, 1) if len(lengths) > 1 else (hop,)):
                got, poff = run_power_ragged(kind, ys, frame_length, h)
                for b, y in enumerate(ys):
                    nf = power_frames(len(y), frame_length, h)
                    one, src = out_buf((nf,), dev), inp(y, dev)
                    assert lib.avc_dsp_frame_power(P(src), len(y), frame_length, h, P(one.view), None) == 0
                    one.assert_intact("(avc_dsp_frame_power)")
                    assert poff[b + 1] - poff[b] == nf
                    assert np.array_equal(bits(got[poff[b]:poff[b + 1]]), bits(one.view)), (lengths, frame_length, h, b)


# ---------------------------------------------------------------- framing with the pre-emphasis fused in
def run_frames_ragged(kind, geom, ys, bounds, woff_host=None, toff_host=None, bounds_host=None, expect=0):
    """ys: the untrimmed utterances, bounds: [(s_b, e_b)].  Returns the frames tensor [win][Ttot] and toff."""
    lib, dev = backend(kind)
    n_fft, hop, win = geom
    lengths = [len(y) for y in ys]
    woff_h, woff = table(offsets(lengths), np.int64, dev)
    toff_h, toff = table(offsets([1 + (e - s) // hop for s, e in bounds]), np.int32, dev)
    bnd_h, bnd = table(np.asarray(bounds).reshape(-1), np.int64, dev)
    if woff_host is not None:
        woff_h = np.ascontiguousarray(woff_host, dtype=np.int64)
    if toff_host is not None:
        toff_h = np.ascontiguousarray(toff_host, dtype=np.int32)
    if bounds_host is not None:
        bnd_h = np.ascontiguousarray(np.asarray(bounds_host).reshape(-1), dtype=np.int64)
    frames = out_buf((win, int(toff[-1])), dev)
    before = snapshot(frames)
    src = inp(np.concatenate(ys), dev)
    rc = lib.avc_dsp_frames_ragged_preemph(P(src), P(woff), H(woff_h), P(toff), H(toff_h), P(bnd), H(bnd_h), len(ys), n_fft, hop, win, A,
                                           P(frames.view), None)
    assert rc == expect, (rc, expect)
    frames.assert_intact(f"(avc_dsp_frames_ragged_preemph {geom} lengths={lengths} bounds={bounds})")
    if expect != 0:
        assert untouched(frames, before)
        return None
    return frames.view, toff_h


def single_frames(kind, geom, y):
    """avc_dsp_preemphasis, then the frames workspace of avc_dsp_stft, on one (already trimmed) utterance"""
    lib, dev = backend(kind)
    pre, src = out_buf((len(y),), dev), inp(y, dev)
    assert lib.avc_dsp_preemphasis(P(src), len(y), A, P(pre.view), None) == 0
    pre.assert_intact("(avc_dsp_preemphasis)")
    return run_stft(kind, geom, pre.view.cpu().numpy())[1]


def frames64(geom, y):
    """(float64 frames of numpy.pad(reflect) of the pre-emphasised y, the same formula in float32)"""
    n_fft, hop, win = geom
    T = 1 + len(y) // hop
    idx = np.arange(win)[:, None] + (n_fft - win) // 2 + hop * np.arange(T)[None, :]
    y64 = y.astype(np.float64)
    pre64 = np.append(y64[0], y64[1:] - A * y64[:-1])
    pre32 = np.append(y[0], y[1:] - F32(A) * y[:-1]).astype(F32)
    return np.pad(pre64, n_fft // 2, mode="reflect")[idx], np.pad(pre32, n_fft // 2, mode="reflect")[idx]


def check_frames(kind, geom, ys, bounds):
    got, toff = run_frames_ragged(kind, geom, ys, bounds)
    ratios = []
    for b, (y, (s, e)) in enumerate(zip(ys, bounds)):
        cols = got[:, toff[b]:toff[b + 1]]
        one = single_frames(kind, geom, y[s:e])
        assert cols.shape == one.shape and np.array_equal(bits(cols), bits(one)), (geom, b, s, e)
        ref, same32 = frames64(geom, y[s:e])
        ratios.append(worst(cols.cpu().numpy(), ref, fp32_bar(ref, same32, relative=False)))
    return float(np.max(ratios))


@pytest.mark.parametrize("geom", GEOMS, ids=ids)
@pytest.mark.parametrize("kind", KINDS)
def test_frames_ragged_preemph_equals_single_calls_bitwise_and_fp64(kind, geom):
    """B = 1; the B = 5 set untrimmed; and the same five TRIMMED lengths cut out of longer utterances with non-zero bounds (s odd with e at
    the end; s = 0 with e one short of the end; s odd with e one short; two more): the reflection must use e - s, the first trimmed sample
    must not see the one in front of it, and no read may leave [s, e) (the neighbours of every sub-run are other utterances' noise).
    Bit-equal to pre-emphasis + framing of the single path; against float64 at the absolute fp32 bar of the pre-emphasis test."""
    n_fft, hop, _ = geom
    L5 = lengths5(n_fft, hop)
    ratios = [check_frames(kind, geom, packed_noise([3 * n_fft + 5], 300), [(0, 3 * n_fft + 5)]),
              check_frames(kind, geom, packed_noise(L5, 310), [(0, n) for n in L5])]
    cuts = [(1, 0), (0, 1), (3, 1), (7, 2), (5, 0)]                     # (s_b, samples dropped at the end)
    ys = packed_noise([n + s + d for n, (s, d) in zip(L5, cuts)], 320)
    bounds = [(s, s + n) for n, (s, d) in zip(L5, cuts)]
    assert bounds[0][0] % 2 == 1 and bounds[1][1] == len(ys[1]) - 1 and bounds[2][0] % 2 == 1 and bounds[2][1] == len(ys[2]) - 1
    ratios.append(check_frames(kind, geom, ys, bounds))
    print(f"[{kind}] fused framing {ids(geom)}: worst |got - ref| / bar {max(ratios):.3f}")
    assert max(ratios) <= 1.0, ratios


@pytest.mark.parametrize("kind", KINDS)
def test_frames_ragged_preemph_second_grid_pass(kind):
    """(64, 4, 64) with three trimmed utterances of 17,004 frames together: 1,088,256 frame elements, more than the 4096 x 256 lanes
    of one pass of the grid-stride loop."""
    geom = (64, 4, 64)
    lengths = [40003, 20002, 8005]
    bounds = [(3, 40003), (0, 20001), (1, 8005)]
    ys = packed_noise(lengths, 330)
    got, toff = run_frames_ragged(kind, geom, ys, bounds)
    assert got.numel() > PASS + 4096 and filled_tail(got)
    for b, (y, (s, e)) in enumerate(zip(ys, bounds)):
        assert np.array_equal(bits(got[:, toff[b]:toff[b + 1]]), bits(single_frames(kind, geom, y[s:e]))), b


# ---------------------------------------------------------------- de-emphasis
def run_deemph_ragged(kind, xs, a, woff_host=None, inplace=False, expect=0):
    lib, dev = backend(kind)
    lengths = [len(x) for x in xs]
    woff_h, woff = table(offsets(lengths), np.int64, dev)
    if woff_host is not None:
        woff_h = np.ascontiguousarray(woff_host, dtype=np.int64)
    cat = np.concatenate(xs)
    if inplace:
        from tests.redzone import GuardedOutput
        out = GuardedOutput((len(cat),), device=dev, init=torch.from_numpy(cat))
        src = out.view
    else:
        out, src = out_buf((len(cat),), dev), inp(cat, dev)
    before = snapshot(out)
    rc = lib.avc_dsp_deemphasis_ragged(P(src), P(woff), H(woff_h), len(xs), a, P(out.view), None)
    assert rc == expect, (rc, expect)
    out.assert_intact(f"(avc_dsp_deemphasis_ragged lengths={lengths})")
    if expect != 0:
        assert untouched(out, before)
        return None
    return out.view


def check_deemph(kind, lengths, seed):
    lib, dev = backend(kind)
    xs = packed_noise(lengths, seed)
    got = run_deemph_ragged(kind, xs, A)
    same = run_deemph_ragged(kind, xs, A, inplace=True)
    assert np.array_equal(bits(got), bits(same))
    off = offsets(lengths)
    for b, x in enumerate(xs):
        one, src = out_buf((len(x),), dev), inp(x, dev)
        assert lib.avc_dsp_deemphasis(P(src), len(x), A, P(one.view), None) == 0
        one.assert_intact("(avc_dsp_deemphasis)")
        assert np.array_equal(bits(got[off[b]:off[b + 1]]), bits(one.view)), (lengths, b)


@pytest.mark.parametrize("geom", GEOMS, ids=ids)
@pytest.mark.parametrize("kind", KINDS)
def test_deemphasis_ragged_equals_single_calls_bitwise(kind, geom):
    """B = 1 and the B = 5 set (a carry that leaked from one utterance into the next would change every sample behind the joint), and, at
    the first geometry, lengths around the 1024 lanes of the workgroup (runs of 1, 2, 3 and 5 samples per lane; fewer samples than
    lanes).  Out of place and in place."""
    n_fft, hop, _ = geom
    check_deemph(kind, [3 * n_fft + 5], 400)
    check_deemph(kind, lengths5(n_fft, hop), 410)
    if geom == G_RAGGED[0] or geom == STOCK:
        check_deemph(kind, [1, 2, 1023, 1024, 1025, 2049, 5003], 420)


# ---------------------------------------------------------------- refusals
@pytest.mark.parametrize("kind", KINDS)
def test_ragged_edge_refusals_leave_outputs_untouched(kind):
    """The library validates the HOST copies before it launches anything (the device copies are the good ones throughout): a table that
    is not monotone -1; toff disagreeing with the bounds -1; an utterance of n_fft / 2 samples after trimming -6; an utterance of
    frame_length / 2 samples for the powers -6.  The accepted twin of every call runs first."""
    geom = G_RAGGED[0]
    n_fft, hop, win = geom
    lengths = [n_fft // 2 + 1, 9 * hop, 3 * n_fft + 5]
    ys = packed_noise(lengths, 500)
    woff = offsets(lengths)
    swapped = woff.copy(); swapped[1], swapped[2] = woff[2], woff[1]          # decreasing pair
    flat = woff.copy(); flat[1] = 0                                           # an empty utterance
    nonzero = woff.copy(); nonzero[0] = 1
    full = [(0, n) for n in lengths]
    # powers
    assert run_power_ragged(kind, ys, n_fft, hop) is not None
    for bad in (swapped, flat, nonzero):
        run_power_ragged(kind, ys, n_fft, hop, woff_host=bad, expect=-1)
    poff = offsets([power_frames(n, n_fft, hop) for n in lengths])
    bad = poff.copy(); bad[1] += 1
    run_power_ragged(kind, ys, n_fft, hop, poff_host=bad, expect=-1)
    bad = poff.copy(); bad[1], bad[2] = poff[2], poff[1]
    run_power_ragged(kind, ys, n_fft, hop, poff_host=bad, expect=-1)
    short = [noise(n_fft // 2, 501), ys[1], ys[2]]                            # L_0 = frame_length / 2
    run_power_ragged(kind, short, n_fft, hop, expect=-6)
    run_power_ragged(kind, [ys[1], ys[2], noise((n_fft - 1) // 2, 502)], n_fft - 1, hop, expect=-6)
    # framing
    assert run_frames_ragged(kind, geom, ys, full) is not None
    for bad in (swapped, flat, nonzero):
        run_frames_ragged(kind, geom, ys, full, woff_host=bad, expect=-1)
    toff = offsets([1 + n // hop for n in lengths])
    bad = toff.copy(); bad[2] -= 1
    run_frames_ragged(kind, geom, ys, full, toff_host=bad, expect=-1)         # toff disagrees with the bounds
    bad = toff.copy(); bad[1], bad[2] = toff[2], toff[1]
    run_frames_ragged(kind, geom, ys, full, toff_host=bad, expect=-1)         # not monotone
    trimmed = [(0, lengths[0]), (hop, 9 * hop), full[2]]                      # 8 hop samples: one frame fewer than toff says
    run_frames_ragged(kind, geom, ys, full, bounds_host=trimmed, expect=-1)
    run_frames_ragged(kind, geom, ys, full, bounds_host=[full[0], (5, 4), full[2]], expect=-1)                 # e < s
    run_frames_ragged(kind, geom, ys, full, bounds_host=[full[0], (0, 9 * hop + 1), full[2]], expect=-1)       # e past the utterance
    at_half = [(1, 1 + n_fft // 2), full[1], full[2]]                         # n_fft / 2 samples after trimming, toff consistent with it
    run_frames_ragged(kind, geom, ys, at_half, expect=-6)
    # de-emphasis
    assert run_deemph_ragged(kind, ys, A) is not None
    for bad in (swapped, flat, nonzero):
        run_deemph_ragged(kind, ys, A, woff_host=bad, expect=-1)
