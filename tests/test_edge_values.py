"""Edge VALUES (the rest of the suite covers shapes, strides and red zones at unit-scale ``randn``):

A. fp32 -> bf16 conversion, value by value, against ``torch.Tensor.to(torch.bfloat16)``: exact ties, values that round up to Inf, signed
   zeros, infinities, NaNs with low payloads, subnormals -- through ``avc_to_pairs`` and through the bf16 operand mode of the conv.
B. InstanceNorm / AdaIN rows that are badly conditioned (|mean| / std up to 1e4), constant, zero or carry one spike, in every
   implementation with an op-level entry point, against the oracle's restatement evaluated in fp64 on the same fp32 inputs.
C. clip + Adam with a zero / overflowing / NaN / Inf gradient and over many steps, against ``torch.optim.Adam`` + ``clip_grad_norm_``.
D. Power-of-two scale invariance of the convolutions: every rounding commutes with a power of two, so a hidden flush, clamp or saturation
   away from unit scale shows as a changed bit.

kind='emu' = CPU lane-level simulator, kind='gpu' = the gfx950 library through the C ABI; every case runs on both.

Bounds of part B (nothing is fitted to a kernel).  Per row, with y the fp32 row, rstd64 / xh64 its fp64 statistics:

    d_xh  = (4 + log2 T) * 2^-24 * max|y_row| * rstd64            (pairwise-summation bound on the mean, through the subtraction and the gain)
    |out - out64| <= tol_existing + d_xh * |gamma|                  tol_existing = rtol 1e-5 / atol 2e-5 of tests/test_ops_rowops.py

Backward, dy = rstd * gamma * (gm - mean(gm) - xh * mean(gm * xh)) with every xh of the row shifted by at most d_xh:

    |dy - dy64| <= tol_existing_bwd + rstd64 * |gamma| * d_xh * (mean|gm * xh| + (|xh| + d_xh) * mean|gm|)
    |dgamma - dgamma64| <= tol_existing_dcond + d_xh * sum|gm|      (dbeta = sum gm does not depend on the mean)

(the d_xh^2 term matters for constant rows: xh64 = 0 there and the gain is 1 / sqrt(eps) = 316).  An element whose fp64 pre-activation lies
within its own bound of zero may take either branch of the activation: it is compared on the branch the kernel took, and outside the
constant / zero rows at most 1 % of the elements may be such elements.  The fp32 torch oracle itself is held to the same bound in the same
test, so a bound that is too tight shows without a GPU."""
import ctypes
import math

import numpy as np
import pytest
import torch

from adaptive_voice_conversion_amd.engine import RaggedPlan
from oracle import avc_oracle as O
from tests.emu_util import KINDS, P, backend
from tests.test_bf16_pairs import from_pairs, from_planar, to_pairs, to_planar
from tests.test_engine import flat_params
from tests.test_input_grads import oracle_input_grads
from tests.test_submodules import rel
from tests.test_ops_conv import conv_fwd, pack, pack_x3

GPU = pytest.mark.gpu


def f32(words):
    return torch.from_numpy(np.array(words, dtype=np.uint32).view(np.float32).copy())


def bits32(t):
    return t.contiguous().view(torch.int32)


def bf16_bits(t):
    """the 16 bits of a bf16-representable fp32 tensor"""
    return (bits32(t) >> 16) & 0xFFFF


# =====================================================================================================================
# A. bf16 conversion conformance
# =====================================================================================================================
def _tie_words():
    out = []
    for e in (-100, -1, 0, 100):
        for sign in (0, 0x80000000):
            for odd in (0, 0x00010000):
                base = sign | ((e + 127) << 23) | odd
                out += [base | 0x8000, base | 0x7FFF, base | 0x8001]   # the exact tie (even / odd upper half), tie - 1 ulp, tie + 1 ulp
    return out


FINITE_WORDS = _tie_words() + [0x7F7F7FFF, 0xFF7F7FFF, 0x00000000, 0x80000000]      # ... stays finite; +-0
TO_INF_WORDS = [0x7F7FFFFF, 0x7F7F8000, 0xFF7FFFFF, 0xFF7F8000, 0x7F800000, 0xFF800000]   # RNE rounds the first four to Inf; +-Inf
NAN_WORDS = [0x7FC00000, 0x7F800001, 0x7FFFFFFF, 0xFFC00001]
# fp32 subnormals (and the largest one, which rounds up to the smallest normal): {RNE value, zero of the same sign} is accepted
SUBNORMAL_WORDS = [0x00000001, 0x00007FFF, 0x00008000, 0x00008001, 0x00018000, 0x00400000, 0x007F8000, 0x007FFFFF,
                   0x80000001, 0x80008000, 0x80018000, 0x80400000, 0x807FFFFF]


def _check_bf16(got_bits, src, what, zero_sign=True, subnormal=False):
    """got_bits: int32 tensor of bf16 words, src: the fp32 inputs (same shape).  Finite results and infinities bit for bit (zero_sign =
    False: zeros by value, see test_bf16_conversion_in_the_conv_operand_mode), NaN in -> any NaN out."""
    ref = src.to(torch.bfloat16).to(torch.float32)
    ref_bits = bf16_bits(ref)
    nan_in = torch.isnan(src)
    is_nan_out = ((got_bits & 0x7F80) == 0x7F80) & ((got_bits & 0x007F) != 0)
    assert bool((is_nan_out == nan_in).all()), f"{what}: NaN in <-> NaN out fails for inputs " \
        f"{[hex(w & 0xFFFFFFFF) for w in bits32(src)[is_nan_out != nan_in].flatten().tolist()[:8]]} -> " \
        f"{[hex(w) for w in got_bits[is_nan_out != nan_in].flatten().tolist()[:8]]}"
    ok = nan_in | (got_bits == ref_bits)
    if not zero_sign:
        ok |= ((got_bits & 0x7FFF) == 0) & ((ref_bits & 0x7FFF) == 0)
    if subnormal:   # a flushed subnormal keeps its sign
        ok |= got_bits == ((bits32(src) >> 16) & 0x8000)
    bad = ~ok
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} wrong; inputs {[hex(w & 0xFFFFFFFF) for w in bits32(src)[bad].flatten().tolist()[:8]]} -> " \
        f"{[hex(w) for w in got_bits[bad].flatten().tolist()[:8]]}, expected {[hex(w) for w in ref_bits[bad].flatten().tolist()[:8]]}"
    return got_bits


def _flush_report(kind, what, got_bits, src):
    rne = bf16_bits(src.to(torch.bfloat16).to(torch.float32))
    flushed = ((got_bits & 0x7FFF) == 0) & ((rne & 0x7FFF) != 0)
    print(f"[{kind} {what}] fp32 subnormal inputs: {int(flushed.sum())} of {flushed.numel()} flushed to zero, the rest round to nearest even")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("table", ["normal", "subnormal"])
def test_bf16_conversion_in_to_pairs(kind, table):
    """avc_to_pairs (bh_pack): the table tiled over a [2, 16, 64] tensor, every element checked."""
    lib, dev = backend(kind)
    words = SUBNORMAL_WORDS if table == "subnormal" else FINITE_WORDS + TO_INF_WORDS + NAN_WORDS
    B, C, T = 2, 16, 64
    vals = f32(words)
    x = vals.repeat(B * C * T // len(words) + 1)[:B * C * T].reshape(B, C, T).contiguous()
    xd = x.to(dev)
    dst = torch.zeros(B, C // 2, T, dtype=torch.int32, device=dev)
    assert lib.avc_to_pairs(P(xd), xd.stride(0), xd.stride(1), xd.stride(2), B, C, T, P(dst), None) == 0
    p = dst.cpu()
    got = torch.empty(B, C, T, dtype=torch.int32)
    got[:, 0::2] = p & 0xFFFF
    got[:, 1::2] = (p >> 16) & 0xFFFF
    _check_bf16(got, x, f"{kind} avc_to_pairs", subnormal=table == "subnormal")
    if table == "subnormal":
        _flush_report(kind, "avc_to_pairs", got, x)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("table", ["normal", "subnormal"])
def test_bf16_conversion_in_the_conv_operand_mode(kind, table):
    """avc_conv1d_fwd with bf16 operand rounding (avc_pack_bf16x4) and a 1x1 identity weight, Cin = Cout = 16, T = 64, zero bias: the output
    is the rounded input, the one-term products being exact in the fp32 accumulator.  Two things follow from the sum the conv still is:
    (1) out[c] = sum_c' x[c'] * w[c][c'] multiplies a non-finite x[c'] by the zeros of the other rows (Inf * 0 = NaN), so sample 0 carries
    ONE table value per frame (frame t: channel t % 16, zeros elsewhere) and only that element is checked; sample 1 carries the values
    whose rounding is finite in every element.  (2) the accumulator starts at +0 and (+0) + (-0) = +0: a zero comes out as a zero, its
    sign is the sum's, not the conversion's (avc_to_pairs above pins the sign)."""
    lib, dev = backend(kind)
    C, T = 16, 64
    sub = table == "subnormal"
    words = SUBNORMAL_WORDS if sub else FINITE_WORDS + TO_INF_WORDS + NAN_WORDS
    assert len(words) <= T
    vals = f32(words)
    dense = f32(SUBNORMAL_WORDS if sub else FINITE_WORDS)
    x = torch.zeros(2, C, T)
    t_idx = torch.arange(T)
    col = vals[t_idx % len(words)]
    x[0, t_idx % C, t_idx] = col
    x[1] = dense.repeat(C * T // len(dense) + 1)[:C * T].reshape(C, T)
    w = torch.eye(C).reshape(C, C, 1).contiguous()
    b = torch.zeros(C)
    assert lib.avc_set_tuning(b"compute", 1) == 0
    try:
        out, _ = conv_fwd(lib, dev, x.to(dev), w.to(dev), b.to(dev))
    finally:
        lib.avc_set_tuning(b"compute", 0)
    out = out.cpu()
    assert bool(((bits32(out) & 0xFFFF) == 0).all()), "the identity conv of bf16 operands left low mantissa bits"
    got0 = bf16_bits(out[0, t_idx % C, t_idx])
    _check_bf16(got0, col, f"{kind} conv bf16 operands (one value per frame)", zero_sign=False, subnormal=sub)
    got1 = bf16_bits(out[1])
    _check_bf16(got1, x[1], f"{kind} conv bf16 operands (dense)", zero_sign=False, subnormal=sub)
    if sub:
        _flush_report(kind, "conv bf16 operands", got1, x[1])


# =====================================================================================================================
# B. InstanceNorm at ill-conditioned and degenerate rows
# =====================================================================================================================
SLOPE = {0: None, 1: 0.0, 2: 0.01}
FWD_TOL = dict(rtol=1e-5, atol=2e-5)      # tests/test_ops_rowops.py
BWD_TOL = dict(rtol=2e-4, atol=2e-5)
DCOND_TOL = dict(rtol=1e-4, atol=1e-4)
PAIR_ULP = 2.0 ** -8                      # tests/test_bf16_pairs.py close_bf16: one bf16 ulp of the stored value
PAIR_FWD_TOL = dict(rtol=PAIR_ULP, atol=2e-5)
PAIR_BWD_TOL = dict(rtol=PAIR_ULP, atol=1e-4)
PAIR_DCOND_TOL = dict(rtol=2e-4, atol=2e-4)
BAND_CAP = 0.01
RATIOS = {}    # worst error / bound per (kind, kernel), printed by the tests (DESIGN.md section 6 quotes them)


def family_rows(R, T, seed):
    """R rows of T frames cycling through the families; returns (rows [R, T], exempt [R]: constant / zero rows, where every element sits
    at the activation's kink)."""
    g = torch.Generator().manual_seed(seed)
    fams = [("i", 1.0, 100.0), ("i", 0.03, -300.0), ("i", 1.0, -1e4), ("i", 20.0, 2e5), ("ii", 3.0), ("ii", 0.1), ("ii", -1000.0), ("iii",),
            ("iv", 0), ("iv", T - 1), ("iv", T // 2), ("i", 1.0, 30.0)]     # (the last one survives bf16 storage as a non-constant row)
    rows, exempt = [], []
    for r in range(R):
        f = fams[r % len(fams)]
        if f[0] == "i":
            rows.append(torch.randn(T, generator=g) * f[1] + f[2])
        elif f[0] == "ii":
            rows.append(torch.full((T,), f[1]))
        elif f[0] == "iii":
            rows.append(torch.zeros(T))
        else:
            v = torch.randn(T, generator=g)
            v[f[1]] = 1e4
            rows.append(v)
        exempt.append(f[0] in ("ii", "iii"))
    return torch.stack(rows), torch.tensor(exempt)


def in_ref64(y, gamma, beta):
    """the oracle's restatement (O.instance_norm + O.append_cond) in fp64 on the fp32 rows y [B, C, T]; gamma / beta [B, C] or None"""
    T = y.shape[-1]
    y64 = y.double()
    mean = y64.mean(-1, keepdim=True)
    var = ((y64 - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + O.IN_EPS)
    xh = (y64 - mean) * rstd
    G = torch.ones_like(mean) if gamma is None else gamma.double()[:, :, None]
    Bt = torch.zeros_like(mean) if beta is None else beta.double()[:, :, None]
    d_xh = (4 + math.log2(T)) * 2.0 ** -24 * y64.abs().amax(-1, keepdim=True) * rstd
    return dict(mean=mean, rstd=rstd, xh=xh, pre=xh * G + Bt, G=G, d_xh=d_xh, T=T)


def check_in_fwd(tag, got, R, relu, exempt, rtol, atol):
    """got [B, C, T] (fp32 or fp64) against the fp64 reference R; returns the activation mask the kernel used (all True without one)."""
    got = got.double()
    pre, extra = R["pre"], R["d_xh"] * R["G"].abs()
    slope = SLOPE[relu]
    if slope is None:
        ref, mask, band = pre, torch.ones_like(pre, dtype=torch.bool), torch.zeros_like(pre, dtype=torch.bool)
    else:
        band = pre.abs() <= atol + rtol * pre.abs() + extra
        mask = torch.where(band, got > 0, pre > 0)
        ref = torch.where(mask, pre, slope * pre)
    tol = atol + rtol * ref.abs() + extra
    err = (got - ref).abs()
    ratio = (err / tol).max().item()
    RATIOS[tag] = max(RATIOS.get(tag, 0.0), ratio)
    ex = exempt.reshape(pre.shape[0], pre.shape[1])
    share = band[~ex].double().mean().item() if bool((~ex).any()) else 0.0
    print(f"[{tag}] T={R['T']} act={relu}: worst |err| / bound {ratio:.3f}; {share * 100:.2f} % of the elements in the branch band")
    assert torch.isfinite(got).all(), tag
    assert ratio <= 1.0, f"{tag}: |err| / bound = {ratio:.3f} at {np.unravel_index(int((err / tol).argmax()), err.shape)}"
    assert share <= BAND_CAP, f"{tag}: {share * 100:.2f} % of the elements within their bound of the activation's kink (change the seed)"
    return mask


def in_bwd_ref64(R, gout, mask, relu):
    slope = SLOPE[relu]
    g = gout.double()
    gm = g if slope is None else torch.where(mask, g, slope * g)
    xh, rstd, G, d = R["xh"], R["rstd"], R["G"], R["d_xh"]
    dbeta, dgamma = gm.sum(-1), (gm * xh).sum(-1)
    dy = rstd * G * (gm - gm.mean(-1, keepdim=True) - xh * (gm * xh).mean(-1, keepdim=True))
    dy_extra = rstd * G.abs() * d * ((gm * xh).abs().mean(-1, keepdim=True) + (xh.abs() + d) * gm.abs().mean(-1, keepdim=True))
    dgamma_extra = d[..., 0] * gm.abs().sum(-1)
    return dy, dy_extra, dbeta, dgamma, dgamma_extra


def check_in_bwd(tag, dy, dbeta, dgamma, R, gout, mask, relu, tol, dcond_tol):
    dy64, dy_extra, dbeta64, dgamma64, dgamma_extra = in_bwd_ref64(R, gout, mask, relu)
    bound = tol["atol"] + tol["rtol"] * dy64.abs() + dy_extra
    ratio = ((dy.double() - dy64).abs() / bound).max().item()
    RATIOS[tag] = max(RATIOS.get(tag, 0.0), ratio)
    print(f"[{tag}] T={R['T']} act={relu}: worst |err| / bound {ratio:.3f}")
    assert torch.isfinite(dy).all(), tag
    assert ratio <= 1.0, f"{tag}: dy |err| / bound = {ratio:.3f}"
    if dbeta is not None:
        rb = ((dbeta.double() - dbeta64).abs() / (dcond_tol["atol"] + dcond_tol["rtol"] * dbeta64.abs())).max().item()
        rg = ((dgamma.double() - dgamma64).abs() / (dcond_tol["atol"] + dcond_tol["rtol"] * dgamma64.abs() + dgamma_extra)).max().item()
        assert rb <= 1.0 and rg <= 1.0, f"{tag}: dbeta {rb:.3f}, dgamma {rg:.3f} of their bounds"


def oracle32(y, cond, relu):
    v = O.instance_norm(y)
    if cond is not None:
        v = O.append_cond(v, cond)
    if relu == 1:
        v = torch.relu(v)
    elif relu == 2:
        v = torch.nn.functional.leaky_relu(v, 0.01)
    return v


def _cond(B, C, affine, g):
    """AdaIN rows [B, 3 * 2C] (the kernel reads the slice at 2C: beta | gamma), or None"""
    if not affine:
        return None, 0, None, None
    cond_all = torch.randn(B, 3 * 2 * C, generator=g)
    off = 2 * C
    return cond_all, off, cond_all[:, off + C:off + 2 * C], cond_all[:, off:off + C]


ROW_CASES = [(T, affine, relu) for T in (16, 128, 19, 100) for affine, relu in ((False, 1), (True, 1), (True, 2), (False, 2), (True, 0))]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("T,affine,relu", ROW_CASES)
def test_instnorm_rows_at_ill_conditioned_values(kind, T, affine, relu):
    """avc_instnorm_fwd / _bwd: the fast path (T = 16, 128) and the generic path (T = 19, 100); 24 rows = every family at least twice.
    The backward is given the activation mask read off the forward's OUTPUT, so it also fails when the backward kernel recomputes another
    decision from the saved statistics than the forward took.  It did on the GPU at T = 100 (constant row 3.0: forward 2.1e-5 > 0 in
    all 100 frames, backward 0; |err| / bound = 4997): the forward's `sum * (1 / T)` was contracted into `y - mean`, so it normalised by
    an unrounded mean and saved the rounded one.  The kernels divide since."""
    lib, dev = backend(kind)
    B, C = 3, 8
    rows, exempt = family_rows(B * C, T, 100 + T)
    y = rows.reshape(B, C, T)
    g = torch.Generator().manual_seed(T + 7 * relu + affine)
    cond_all, off, gamma, beta = _cond(B, C, affine, g)
    R = in_ref64(y, gamma, beta)
    cond32 = cond_all[:, off:off + 2 * C] if affine else None
    check_in_fwd("oracle fp32 instnorm_fwd", oracle32(y, cond32, relu), R, relu, exempt, **FWD_TOL)
    yd = y.to(dev)
    cd = cond_all.to(dev) if affine else None
    out = torch.full((B, C, T), float("nan"), device=dev)
    mean = torch.full((B * C,), float("nan"), device=dev)
    rstd = torch.full((B * C,), float("nan"), device=dev)
    rc = lib.avc_instnorm_fwd(P(yd), B, C, T, P(cd), cd.stride(0) if affine else 0, off, relu, None, 0, 0, P(out), P(mean), P(rstd), None)
    assert rc == 0, rc
    path = "fast" if T in (16, 128) else "generic"
    mask = check_in_fwd(f"{kind} instnorm_fwd {path}", out.cpu(), R, relu, exempt, **FWD_TOL)
    mean_bound = 1e-5 + 1e-5 * R["mean"].abs() + R["d_xh"] / R["rstd"]
    assert bool(((mean.cpu().double().view(B, C, 1) - R["mean"]).abs() <= mean_bound).all())
    # backward from the statistics the forward saved
    gout = torch.randn(B, C, T, generator=g)
    gd = gout.to(dev)
    dy = torch.full((B, C, T), float("nan"), device=dev)
    dcond = torch.zeros(B, 3 * 2 * C, device=dev)
    rc = lib.avc_instnorm_bwd(P(gd), P(yd), P(mean), P(rstd), B, C, T, P(cd), cd.stride(0) if affine else 0, off, relu, P(dy),
                              P(dcond if affine else None), dcond.stride(0), off, None)
    assert rc == 0, rc
    dc = dcond.cpu()
    check_in_bwd(f"{kind} instnorm_bwd {path}", dy.cpu(), dc[:, off:off + C] if affine else None, dc[:, off + C:off + 2 * C] if affine else None,
                 R, gout, mask, relu, BWD_TOL, DCOND_TOL)
    # ... and the fp32 autograd of the oracle against the same bound (on the branch it took itself)
    yg = y.clone().requires_grad_(True)
    o32 = oracle32(yg, cond32, relu)
    (dy32,) = torch.autograd.grad(o32, yg, gout)
    m32 = check_in_fwd("oracle fp32 instnorm_fwd", o32.detach(), R, relu, exempt, **FWD_TOL)
    check_in_bwd("oracle fp32 instnorm_bwd", dy32, None, None, R, gout, m32, relu, BWD_TOL, DCOND_TOL)


PAIR_ROW_CASES = [(T, planar, affine, relu) for T, planar in ((12, 0), (64, 0), (64, 1)) for affine, relu in ((False, 1), (True, 1), (True, 2))]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("T,planar,affine,relu", PAIR_ROW_CASES)
def test_instnorm_pair_rows_at_ill_conditioned_values(kind, T, planar, affine, relu):
    """avc_instnorm_fwd_pairs / _bwd_pairs, C = 6: the same formula on the bf16-rounded rows (what the kernel reads), plus one bf16 ulp of
    the stored value (the output is rounded once on store), the term tests/test_bf16_pairs.py states."""
    lib, dev = backend(kind)
    B, C = 3, 6
    rows, exempt = family_rows(B * C, T, 200 + T)
    y = rows.reshape(B, C, T).to(torch.bfloat16).to(torch.float32)
    # bf16 keeps 8 bits: a row of |mean| / std = 1e4 (and 0.03 * randn - 300, whose ulp is 2) is CONSTANT once stored, family (ii)
    exempt = (y.amax(-1) == y.amin(-1)).reshape(-1)
    assert 0 < int((~exempt).sum()) < exempt.numel()
    g = torch.Generator().manual_seed(T + 7 * relu + affine)
    cond_all, off, gamma, beta = _cond(B, C, affine, g)
    R = in_ref64(y, gamma, beta)
    check_in_fwd("oracle fp32 instnorm_fwd (bf16 rows)", oracle32(y, cond_all[:, off:off + 2 * C] if affine else None, relu), R, relu, exempt,
                 **FWD_TOL)
    yd = (to_planar(y) if planar else to_pairs(y)).to(dev)
    cd = cond_all.to(dev) if affine else None
    out = torch.zeros(B, C // 2, T, dtype=torch.int32, device=dev)
    mean = torch.full((B * C,), float("nan"), device=dev)
    rstd = torch.full((B * C,), float("nan"), device=dev)
    rc = lib.avc_instnorm_fwd_pairs(P(yd), B, C, T, P(cd), cd.stride(0) if affine else 0, off, relu, None, 0, 0, planar, P(out), P(mean), P(rstd),
                                    None)
    assert rc == 0, rc
    mask = check_in_fwd(f"{kind} instnorm_fwd_pairs", from_pairs(out.cpu()), R, relu, exempt, **PAIR_FWD_TOL)
    gout = torch.randn(B, C, T, generator=g).to(torch.bfloat16).to(torch.float32)
    gd = to_pairs(gout).to(dev)
    dy = torch.zeros_like(yd)
    dcond = torch.zeros(B, 3 * 2 * C, device=dev)
    rc = lib.avc_instnorm_bwd_pairs(P(gd), P(yd), P(mean), P(rstd), B, C, T, P(cd), cd.stride(0) if affine else 0, off, relu, planar, P(dy),
                                    P(dcond if affine else None), dcond.stride(0), off, None)
    assert rc == 0, rc
    got = from_planar(dy.cpu()) if planar else from_pairs(dy.cpu())
    dc = dcond.cpu()
    check_in_bwd(f"{kind} instnorm_bwd_pairs", got, dc[:, off:off + C] if affine else None, dc[:, off + C:off + 2 * C] if affine else None,
                 R, gout, mask, relu, PAIR_BWD_TOL, PAIR_DCOND_TOL)


# the two shortest rows of IN_FWD_CASES / IN_BWD_CASES (tests/test_redzone_ops.py) that take the fused path: rows of 16 and of 32 frames.
# B is cut to 3 samples: a silent one (constant rows = the bias), a random one (family (i): the bias is the offset), one with a spike.
CONV_IN_FWD = [(24, 64, 16, 5, 1, 1, True, 2), (16, 40, 32, 5, 1, 1, False, 1)]       # Cin, Cout, Tin, KS, stride, ops, affine, relu
CONV_IN_BWD = [(64, 24, 16, 5, 1, 4, True, 2), (40, 16, 32, 5, 1, 1, True, 1)]        # Cin (rows), Cout, T, KS, stride, res_mode, affine, relu
BIAS_CYCLE = [100.0, -1e4, 3.0, 0.1, -1000.0, 0.0, 2e3, -30.0]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fuse", [1, 0])
@pytest.mark.parametrize("Cin,Cout,Tin,KS,stride,ops,affine,relu", CONV_IN_FWD)
def test_conv_in_fwd_at_ill_conditioned_values(kind, fuse, Cin, Cout, Tin, KS, stride, ops, affine, relu):
    """avc_conv1d_in_fwd, the fused epilogue (conv_shared.h) and the two-launch path on the same inputs.  The offsets come in through the
    conv BIAS, so the conv's output rows carry them: sample 0 is silent (every row constant = its bias: 100, -1e4, 3, 0.1, -1000, 0, ...),
    sample 1 is randn (unit-scale rows on those offsets: |mean| / std up to 1e4), sample 2 is randn with one input frame of 1e4.  The
    reference is evaluated on the rows y the call itself returns (the conv is pinned by tests/test_ops_conv.py); y is checked to be the
    fp32 conv + bias to the tolerance stated there, relative to the row's scale."""
    import tests.test_conv_in_fuse as CF
    lib, dev = backend(kind)
    B = 3
    g = torch.Generator().manual_seed(Tin + 3)
    x = torch.randn(B, Cin, Tin, generator=g)
    x[0] = 0.0
    x[2, 1, Tin // 3] = 1e4
    w = torch.randn(Cout, Cin, KS, generator=g) / (Cin * KS) ** 0.5
    b = torch.tensor([BIAS_CYCLE[c % len(BIAS_CYCLE)] for c in range(Cout)])
    C = Cout // ops
    cond = torch.randn(B, 4 * C + 8, generator=g) if affine else None
    cond_off = 2 * C + 8 if affine else 0
    d = lambda t: None if t is None else t.to(dev)
    assert lib.avc_set_tuning(b"conv_in_fuse", fuse) == 0
    try:
        y, out, mean, rstd, fused = CF.run(lib, dev, d(x), d(w), d(b), stride, ops, d(cond), cond_off, relu, None, 0)
    finally:
        lib.avc_set_tuning(b"conv_in_fuse", 1)
    assert fused == fuse
    y = y.cpu()
    y_ref = O.pad_conv(x.double(), w.double(), b.double(), stride)
    scale = y_ref.abs().amax(-1, keepdim=True)
    assert bool(((y.double() - y_ref).abs() <= 2e-5 + 1e-5 * scale).all())
    assert bool((y[0] == b[:, None]).all()), "a silent segment does not give constant rows"
    gamma = cond[:, cond_off + C:cond_off + 2 * C] if affine else None
    beta = cond[:, cond_off:cond_off + C] if affine else None
    R = in_ref64(y, gamma, beta)
    exempt = torch.zeros(B, C, dtype=torch.bool)
    exempt[0] = True
    c32 = cond[:, cond_off:cond_off + 2 * C] if affine else None
    check_in_fwd("oracle fp32 instnorm_fwd (conv rows)", oracle32(y, c32, relu), R, relu, exempt, **FWD_TOL)
    check_in_fwd(f"{kind} conv1d_in_fwd {'fused' if fuse else 'two launches'}", out.cpu(), R, relu, exempt, **FWD_TOL)
    mean_bound = 1e-5 + 1e-5 * R["mean"].abs() + R["d_xh"] / R["rstd"]
    assert bool(((mean.cpu().double().view(B, C, 1) - R["mean"]).abs() <= mean_bound).all())


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fuse", [1, 0])
@pytest.mark.parametrize("Cin,Cout,T,KS,stride,res_mode,affine,relu", CONV_IN_BWD)
def test_conv_dgrad_in_bwd_at_ill_conditioned_values(kind, fuse, Cin, Cout, T, KS, stride, res_mode, affine, relu):
    """avc_conv1d_dgrad_in_bwd: the saved forward rows y are the families (statistics from avc_instnorm_fwd on them, the forward's own), the
    reference is evaluated on the g the call returns (the input gradient + join is pinned by tests/test_ops_conv.py)."""
    lib, dev = backend(kind)
    B = 3
    rows, exempt = family_rows(B * Cin, T, 300 + T)
    y = rows.reshape(B, Cin, T)
    g = torch.Generator().manual_seed(T + 11)
    Tdy = O.pad_conv(torch.zeros(1, Cin, T), torch.zeros(Cout, Cin, KS), None, stride).shape[2]
    w = (torch.randn(Cout, Cin, KS, generator=g) / (Cin * KS) ** 0.5).to(dev)
    dy = torch.randn(B, Cout, Tdy, generator=g).to(dev)
    cond = torch.randn(B, 2 * Cin + 6, generator=g) if affine else None
    coff = 6 if affine else 0
    Tres = {0: 0, 1: T, 3: T // 2, 4: 2 * T}[res_mode]
    res = torch.randn(B, Cin, Tres, generator=g).to(dev) if res_mode else None
    yd, cd = y.to(dev), (cond.to(dev) if affine else None)
    out = torch.full((B, Cin, T), float("nan"), device=dev)
    mean = torch.full((B * Cin,), float("nan"), device=dev)
    rstd = torch.full((B * Cin,), float("nan"), device=dev)
    assert lib.avc_instnorm_fwd(P(yd), B, Cin, T, P(cd), cd.stride(0) if affine else 0, coff, relu, None, 0, 0, P(out), P(mean), P(rstd), None) == 0
    gamma = cond[:, coff + Cin:coff + 2 * Cin] if affine else None
    beta = cond[:, coff:coff + Cin] if affine else None
    R = in_ref64(y, gamma, beta)
    mask = check_in_fwd(f"{kind} instnorm_fwd fast", out.cpu(), R, relu, exempt, **FWD_TOL)
    wpd = pack(lib, dev, [w], 1)
    gout = torch.full((B, Cin, T), float("nan"), device=dev)
    dyo = torch.full((B, Cin, T), float("nan"), device=dev)
    dcond = torch.zeros(B, 2 * Cin + 6, device=dev)
    fused = ctypes.c_int(-1)
    assert lib.avc_set_tuning(b"conv_in_fuse", fuse) == 0
    try:
        rc = lib.avc_conv1d_dgrad_in_bwd(P(dy), dy.stride(0), dy.stride(1), 1, 1, B, Cout, Tdy, P(wpd), Cin, KS, stride, T, P(gout), P(res),
                                         res_mode, Tres, P(yd), P(mean), P(rstd), P(cd), cd.stride(0) if affine else 0, coff, relu, P(dyo),
                                         P(dcond if affine else None), dcond.stride(0) if affine else 0, coff, ctypes.byref(fused), None)
    finally:
        lib.avc_set_tuning(b"conv_in_fuse", 1)
    assert rc == 0, rc
    assert fused.value == fuse
    dc = dcond.cpu()
    check_in_bwd(f"{kind} conv1d_dgrad_in_bwd {'fused' if fuse else 'two launches'}", dyo.cpu(), dc[:, coff:coff + Cin] if affine else None,
                 dc[:, coff + Cin:coff + 2 * Cin] if affine else None, R, gout.cpu(), mask, relu, BWD_TOL, DCOND_TOL)


def _ragged_content_plan(kind, xs):
    """the ragged CONTENT encoder with a backward pass over the utterances xs, forward done in a NaN-filled workspace"""
    lib, dev = backend(kind)
    cfg = O.tiny_config()
    sd = O.make_state_dict(cfg, 21)
    plan = RaggedPlan(cfg, [int(x.shape[0]) for x in xs], None, lib=lib, mode="encode", input_grads=True)
    params = flat_params(plan, sd, dev)
    ws = torch.full((plan.workspace_floats,), float("nan"), device=dev)
    x = torch.cat(xs).to(dev)
    plan.forward(params, x, None, ws)
    return plan, params, x, ws, cfg, sd, dev


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("offset", [0.0, 300.0])
def test_ragged_instnorm_rows_at_offset_inputs(kind, offset):
    """rag_instnorm_fwd_kernel (ragged_rows.hip: one wavefront per row at the row's own length), lengths [17, 65].  The speaker encoder has
    no InstanceNorm (model.py:237-277), so a speaker-only plan never reaches these kernels: the rows run through the ragged CONTENT
    encoder, whose workspace names the in_conv's pre-norm rows ("enc_y0"), the statistics the forward saved ("enc_st0") and the rows of
    the next conv ("enc_y1_0").  Input mels offset by a constant put every pre-norm row on an offset; utterance 1 is silent apart from the
    offset (constant rows).  Three links:
    1. the saved statistics against the fp64 statistics of the very rows they were taken from;
    2. the rows the BACKWARD will recompute from them -- act(in_xhat(y, saved mean, saved rstd)), two rounded fp32 operations, restated
       here bit for bit -- against the fp64 formula under the bound of part B;
    3. the forward really stored THOSE rows: the next conv of them (fp64) equals "enc_y1_0" to the rounding of an fp32 sum of n = Cin * k
       terms, n * 2^-24 * sum|term| (1e-5 for n = 160) + 2e-5.  A forward that normalises by another mean than it saves (the contracted
       sum * (1 / T)) moves a constant row of height c by up to 316 * ulp(c) / 2 and fails here at offset 300."""
    xs = [torch.randn(17, 16, generator=torch.Generator().manual_seed(5)) + offset, torch.full((65, 16), offset)]
    plan, params, x, ws, cfg, sd, dev = _ragged_content_plan(kind, xs)
    T, S, C = plan.T, len(xs), cfg["ContentEncoder"]["c_h"]
    assert xs[0].shape[1] == cfg["ContentEncoder"]["c_in"]
    wsc = ws.cpu()
    y_off, st_off, y1_off = plan.buffer("enc_y0"), plan.buffer("enc_st0"), plan.buffer("enc_y1_0")
    assert min(y_off, st_off, y1_off) >= 0
    w1, b1 = sd["content_encoder.first_conv_layers.0.weight"], sd["content_encoder.first_conv_layers.0.bias"]
    o = 0
    for s in range(S):
        y = wsc[y_off + C * o:y_off + C * (o + T[s])].reshape(1, C, T[s])
        y1 = wsc[y1_off + C * o:y1_off + C * (o + T[s])].reshape(1, C, T[s])
        o += T[s]
        R = in_ref64(y, None, None)
        mean32, rstd32 = wsc[st_off + s * C:st_off + (s + 1) * C].view(1, C, 1), wsc[st_off + S * C + s * C:st_off + S * C + (s + 1) * C].view(1, C, 1)
        mean, rstd = mean32.double(), rstd32.double()
        mean_bound = 1e-5 + 1e-5 * R["mean"].abs() + R["d_xh"] / R["rstd"]
        rm = ((mean - R["mean"]).abs() / mean_bound).max().item()
        # rstd = (var + eps)^-1/2 with var taken about a mean that is off by at most e = d_xh / rstd64: var grows by at most e^2
        e2 = (R["d_xh"] / R["rstd"]) ** 2
        rstd_lo = 1.0 / torch.sqrt(1.0 / R["rstd"] ** 2 + e2)
        rr = ((rstd - R["rstd"]).abs() / (1e-5 + 1e-4 * R["rstd"] + (R["rstd"] - rstd_lo))).max().item()
        tag = f"{kind} rag_instnorm_fwd statistics"
        RATIOS[tag] = max(RATIOS.get(tag, 0.0), rm, rr)
        print(f"[{tag}] T={T[s]} offset={offset}: mean {rm:.3f}, rstd {rr:.3f} of their bounds; max |mean| * rstd = "
              f"{(R['mean'].abs() * R['rstd']).max().item():.1f}")
        assert rm <= 1.0 and rr <= 1.0
        out = torch.relu((y - mean32) * rstd32)     # in_xhat, in_preact(gamma = 1, beta = 0) and ReLU of avc_common.h in fp32
        exempt = (y.amax(-1) == y.amin(-1)).reshape(-1)
        assert bool(exempt.all()) == (s == 1)
        check_in_fwd(f"{kind} rag_instnorm_fwd rows", out, R, 1, exempt, **FWD_TOL)
        y1_ref = O.pad_conv(out.double(), w1.double(), b1.double(), 1)
        n = w1.shape[1] * w1.shape[2]
        y1_bound = 2e-5 + n * 2.0 ** -24 * O.pad_conv(out.double(), w1.double().abs(), b1.double().abs(), 1)
        r1 = ((y1.double() - y1_ref).abs() / y1_bound).max().item()
        print(f"[{kind} rag_instnorm_fwd stored rows -> next conv] T={T[s]} offset={offset}: worst |err| / bound {r1:.3f}")
        assert r1 <= 1.0, f"the forward did not store act(in_xhat(y, saved mean, saved rstd)): next conv off by {r1:.1f} bounds (T = {T[s]})"


@pytest.mark.parametrize("kind", KINDS)
def test_ragged_instnorm_bwd_at_offset_inputs(kind):
    """rag_instnorm_bwd_kernel through avc_content_backward_ragged, lengths [17, 65], mels = randn + 300 (every pre-norm row of the in_conv
    on an offset of some hundred standard deviations).  Reference and bar are those of tests/test_ragged_content_grads.py: the fp64 oracle
    gradient on the branch the engine's backward took (saved y > saved mean), rel-L2 <= max(1e-4, 2 x err(fp32 oracle, fp64 oracle)) on that
    same branch -- the project's rule for ill-conditioned sums, applied to both lengths here."""
    from tests.test_ragged_content_grads import BAR, _blocks, _d_muls, _relu_masks, _split
    g = torch.Generator().manual_seed(6)
    xs = [torch.randn(t, 16, generator=g) + 300.0 for t in (17, 65)]
    plan, params, x, ws, cfg, sd, dev = _ragged_content_plan(kind, xs)
    d = _d_muls(plan, 31)
    plan.backward_content(params, x, d.to(dev), ws)
    grads = _split(plan.d_x(ws), plan.T)
    masks = _relu_masks(plan, ws, cfg)
    fn = lambda v, s_: O.content_encoder(v, s_, cfg)   # noqa: E731
    for b, (xb, (wm, wl)) in enumerate(zip(xs, _blocks(d, plan))):
        ref, = oracle_input_grads(fn, [xb.t()[None]], sd, masks[b], [wm, wl])
        r32, = oracle_input_grads(fn, [xb.t()[None]], sd, masks[b], [wm, wl], dtype=torch.float32)
        bar = max(BAR, 2 * rel(r32, ref))
        e = rel(grads[b], ref[0].t())
        print(f"[{kind} rag_instnorm_bwd d_x] T={plan.T[b]}: rel-L2 {e:.2e}, bar {bar:.2e} (fp32 oracle {rel(r32, ref):.2e})")
        assert torch.isfinite(grads[b]).all() and e <= bar, (b, e, bar)


# =====================================================================================================================
# C. clip + Adam edge steps
# =====================================================================================================================
# the C ABI takes its hyper-parameters as fp32; torch gets those very values (0.999f is 0.99900001287..., and 1 - beta2 differs from 0.001 by 1.3e-5)
LR, B1, B2, EPS, MAXN = (float(np.float32(v)) for v in (5e-4, 0.9, 0.999, 1e-8, 5.0))
WD = float(np.float32(1e-4))


class _AdamPair:
    """the kernel and torch.optim.Adam + clip_grad_norm_ side by side on one flat parameter vector"""

    def __init__(self, lib, dev, n, amsgrad, wd, seed=3):
        self.lib, self.dev, self.n, self.amsgrad, self.wd = lib, dev, n, amsgrad, wd
        p0 = torch.randn(n, generator=torch.Generator().manual_seed(seed))
        self.p_ref = p0.clone().requires_grad_(True)
        self.opt = torch.optim.Adam([self.p_ref], lr=LR, betas=(B1, B2), eps=EPS, amsgrad=amsgrad, weight_decay=wd)
        self.p = p0.clone().to(dev)
        self.m, self.v, self.vmax = (torch.zeros(n, device=dev) for _ in range(3))
        self.ws = torch.zeros(lib.avc_clip_adam_ws_floats(n), device=dev)
        self.gn = torch.full((1,), -1.0, device=dev)

    def step(self, grad, step):
        self.p_ref.grad = grad.clone()
        gn_ref = torch.nn.utils.clip_grad_norm_([self.p_ref], MAXN)
        self.opt.step()
        gbuf = grad.clone().to(self.dev)
        rc = self.lib.avc_clip_adam_step(P(self.p), P(gbuf), P(self.m), P(self.v), P(self.vmax), self.n, step, LR, B1, B2, EPS, self.wd,
                                         int(self.amsgrad), MAXN, 1.0, 1, P(self.ws), P(self.gn), None)
        assert rc == 0, rc
        return self.gn.item(), gn_ref.item(), gbuf.cpu()

    def state(self):
        st = self.opt.state[self.p_ref]
        return st["exp_avg"], st["exp_avg_sq"], st.get("max_exp_avg_sq")

    def compare(self, equal_nan=False, steps=1):
        """parameters at the tolerance of test_clip_adam_matches_torch; m / v / vmax are running fp32 sums that both sides round twice a
        step (each at most 2^-24 relative), in their own order: steps * 4 * 2^-24 relative, and no less than the 1e-5 of the parameters"""
        m_ref, v_ref, vmax_ref = self.state()
        rs = max(1e-5, steps * 4 * 2.0 ** -24)
        torch.testing.assert_close(self.p.cpu(), self.p_ref.detach(), rtol=1e-5, atol=1e-6, equal_nan=equal_nan)
        # (m is a SIGNED running sum: its rounding error scales with the terms, not with what is left after they cancel)
        m_scale = m_ref[torch.isfinite(m_ref)].abs().max().item() if bool(torch.isfinite(m_ref).any()) else 0.0
        torch.testing.assert_close(self.m.cpu(), m_ref, rtol=rs, atol=1e-9 + rs * m_scale, equal_nan=equal_nan)
        torch.testing.assert_close(self.v.cpu(), v_ref, rtol=rs, atol=1e-12, equal_nan=equal_nan)
        if self.amsgrad:
            torch.testing.assert_close(self.vmax.cpu(), vmax_ref, rtol=rs, atol=1e-12, equal_nan=equal_nan)


ADAM = [(n, ams) for n in (4099, 4096) for ams in (True, False)]     # scalar and 16-byte paths


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,amsgrad", ADAM)
def test_clip_adam_zero_gradient(kind, n, amsgrad):
    """step 1 with an all-zero gradient: the reported norm is exactly 0, nothing is clipped (coef = min(5 / 1e-6, 1) = 1), the parameters
    move by the weight decay alone -- and not at all without it."""
    lib, dev = backend(kind)
    for wd in (WD, 0.0):
        a = _AdamPair(lib, dev, n, amsgrad, wd)
        p0 = a.p.cpu().clone()
        gn, gn_ref, gclip = a.step(torch.zeros(n), 1)
        assert gn == 0.0 and gn_ref == 0.0
        assert bool((gclip == 0).all())
        a.compare()
        if wd == 0.0:
            assert torch.equal(a.p.cpu(), p0)
        else:
            assert bool((a.p.cpu() != p0).all())


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,amsgrad", ADAM)
def test_clip_adam_squared_norm_overflows_fp32(kind, n, amsgrad):
    """1e20 per element: the squares (1e40) overflow fp32.  torch's fp32 vector norm and the kernel's sum of squares both give +Inf, the
    clip coefficient 5 / (Inf + 1e-6) is 0 in both, every clipped gradient is 1e20 * 0 = 0 and the step is the weight decay's alone:
    finite parameters, equal to torch's."""
    lib, dev = backend(kind)
    a = _AdamPair(lib, dev, n, amsgrad, WD)
    gn, gn_ref, gclip = a.step(torch.full((n,), 1e20), 1)
    print(f"[{kind} clip_adam overflow] kernel norm {gn}, torch fp32 norm {gn_ref}")
    assert gn == gn_ref == float("inf")
    assert torch.equal(gclip, a.p_ref.grad) and bool((gclip == 0).all())
    assert torch.isfinite(a.p).all()
    a.compare()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,amsgrad", ADAM)
def test_clip_adam_nan_gradient_poisons_everything(kind, n, amsgrad):
    """One NaN gradient element: clip_grad_norm_ gives a NaN norm and a NaN coefficient, so the reference turns EVERY parameter, m and v
    into NaN -- a step that cannot go unnoticed.  The kernel must not clip by 1 instead and train on."""
    lib, dev = backend(kind)
    a = _AdamPair(lib, dev, n, amsgrad, WD)
    grad = torch.randn(n, generator=torch.Generator().manual_seed(9)) * 0.01
    grad[n // 3] = float("nan")
    gn, gn_ref, gclip = a.step(grad, 1)
    assert math.isnan(gn) and math.isnan(gn_ref)
    m_ref, v_ref, vmax_ref = a.state()
    assert torch.isnan(a.p_ref).all() and torch.isnan(m_ref).all() and torch.isnan(v_ref).all()     # the reference
    assert torch.isnan(gclip).all()
    assert torch.isnan(a.p).all() and torch.isnan(a.m).all() and torch.isnan(a.v).all()
    if amsgrad:
        assert torch.isnan(vmax_ref).all() and torch.isnan(a.vmax).all()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,amsgrad", ADAM)
def test_clip_adam_inf_gradient(kind, n, amsgrad):
    """One +Inf element: the norm is Inf, the coefficient 0 in both; Inf * 0 = NaN poisons that one element, the others step by the weight
    decay alone."""
    lib, dev = backend(kind)
    a = _AdamPair(lib, dev, n, amsgrad, WD)
    grad = torch.randn(n, generator=torch.Generator().manual_seed(9)) * 0.01
    grad[n - 2] = float("inf")
    gn, gn_ref, gclip = a.step(grad, 1)
    assert gn == gn_ref == float("inf")
    torch.testing.assert_close(gclip, a.p_ref.grad, rtol=0, atol=0, equal_nan=True)
    assert int(torch.isnan(a.p).sum()) == 1 and bool(torch.isnan(a.p[n - 2]))
    a.compare(equal_nan=True)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,amsgrad", ADAM)
def test_clip_adam_300_steps_and_a_late_step(kind, n, amsgrad):
    """300 steps of small random gradients (every 7th one clips), compared at every 50th step, then ONE call with step = 100000 (torch's
    step counter set to 99999 first): the bias corrections 1 - beta^step are taken on the host in double precision."""
    lib, dev = backend(kind)
    a = _AdamPair(lib, dev, n, amsgrad, WD)
    g = torch.Generator().manual_seed(17)
    for step in range(1, 301):
        grad = torch.randn(n, generator=g) * ((0.3 if step % 7 == 0 else 0.01) / (n / 5000) ** 0.5)
        gn, gn_ref, _ = a.step(grad, step)
        if step % 50 == 0 or step == 1:
            assert gn == pytest.approx(gn_ref, rel=1e-5)
            a.compare(steps=step)
    a.opt.state[a.p_ref]["step"] = torch.tensor(99999.0)
    a.step(torch.randn(n, generator=g) * 0.01, 100000)
    a.compare(steps=301)


# =====================================================================================================================
# D. power-of-two scale invariance of the convolutions
# =====================================================================================================================
SCALE_SHAPES = [(2, 20, 33, 19, 5, 1), (2, 64, 128, 64, 5, 1), (3, 16, 32, 20, 5, 2)]     # every tail; whole tiles; strided
# fp32, bf16 operands, the three-term bf16 split, bf16 pair storage.  The split-bf16 conv instance takes k = 5 layers whose reduction
# channels are a multiple of 16 (include/avc_hip.h): (20 -> 33) has no such instance in either direction, so "x3" runs there for the
# weight gradient only (the wgrad_x3 knob), as do the pair instances, which take even channel counts.
SCALE_MODES = ["fp32", "bf16r", "x3", "pairs"]


def _eligible(mode, op, Cin, Cout):
    if mode == "x3" and op != "wgrad":
        return (Cout if op == "dgrad" else Cin) % 16 == 0
    if mode == "pairs":
        return Cin % 2 == 0 and Cout % 2 == 0
    return True


def _scale_cases():
    return [pytest.param(*s, mode, op, id=f"{'-'.join(map(str, s))}-{mode}-{op}") for s in SCALE_SHAPES for mode in SCALE_MODES
            for op in ("fwd", "dgrad", "wgrad") if _eligible(mode, op, s[1], s[2])]


class _mode:
    def __init__(self, lib, mode):
        self.lib, self.mode = lib, mode

    def __enter__(self):
        if self.mode == "bf16r":
            assert self.lib.avc_set_tuning(b"compute", 1) == 0
        elif self.mode == "pairs":
            assert self.lib.avc_set_tuning(b"op_compute_dtype", 3) == 0
        elif self.mode == "x3":
            assert self.lib.avc_set_tuning(b"wgrad_x3", 1) == 0

    def __exit__(self, *a):
        self.lib.avc_set_tuning(b"op_compute_dtype", 0)
        self.lib.avc_set_tuning(b"wgrad_x3", 0)


def _run_conv(lib, dev, mode, op, a, w_or_dy, bias, Cin, Cout, T, KS, stride):
    """one launch; returns fp32 CPU tensors (pair outputs decoded: exact).  fwd: a = x, w_or_dy = w; dgrad: a = dy, w_or_dy = w;
    wgrad: a = x, w_or_dy = dy -> (dW, db)."""
    B = a.shape[0]
    pairs = mode == "pairs"
    tile = 97 if mode == "x3" else 0
    enc = (lambda t: to_pairs(t).to(dev)) if pairs else (lambda t: t.to(dev))
    Tout = O.pad_conv(torch.zeros(1, Cin, T), torch.zeros(Cout, Cin, KS), None, stride).shape[2]
    with _mode(lib, mode):
        if op == "fwd":
            wd = w_or_dy.to(dev)
            wp = pack_x3(lib, dev, wd, 0) if mode == "x3" else pack(lib, dev, [wd], 0)
            xd, bd = enc(a), bias.to(dev)
            out = torch.zeros(B, Cout // 2, Tout, dtype=torch.int32, device=dev) if pairs else torch.full((B, Cout, Tout), float("nan"), device=dev)
            rc = lib.avc_conv1d_fwd(P(xd), xd.stride(0), xd.stride(1), 1, B, Cin, T, P(wp), P(bd), Cout, KS, stride, 0, P(out), out.stride(0),
                                    out.stride(1), 1, 1, None, 0, 0, 0, 0, 0, None, tile, None)
            assert rc == 0, rc
            return (from_pairs(out.cpu()) if pairs else out.cpu(),)
        if op == "dgrad":
            wd = w_or_dy.to(dev)
            wpd = pack_x3(lib, dev, wd, 1) if mode == "x3" else pack(lib, dev, [wd], 1)
            dyd = enc(a)
            dx = torch.zeros(B, Cin // 2, T, dtype=torch.int32, device=dev) if pairs else torch.full((B, Cin, T), float("nan"), device=dev)
            rc = lib.avc_conv1d_dgrad(P(dyd), dyd.stride(0), dyd.stride(1), 1, 1, B, Cout, Tout, P(wpd), Cin, KS, stride, T, P(dx), dx.stride(0),
                                      dx.stride(1), 1, None, 0, 0, 0, 0, 0, None, None, tile, None)
            assert rc == 0, rc
            return (from_pairs(dx.cpu()) if pairs else dx.cpu(),)
        xd, dyd = enc(a), enc(w_or_dy)
        ws = torch.full((lib.avc_conv1d_wgrad_ws_floats(B, Cin, Cout, Tout, KS),), float("nan"), device=dev)
        dW = torch.full((Cout, Cin, KS), float("nan"), device=dev)
        db = torch.full((Cout,), float("nan"), device=dev)
        rc = lib.avc_conv1d_wgrad(P(xd), xd.stride(0), xd.stride(1), 1, P(dyd), dyd.stride(0), dyd.stride(1), 1, 1, B, Cin, Cout, T, Tout, KS,
                                  stride, P(dW), P(db), P(ws), None)
        assert rc == 0, rc
        return dW.cpu(), db.cpu()


def _same_bits(a, b, what):
    assert torch.isfinite(a).all(), what
    ne = bits32(a) != bits32(b)
    assert not bool(ne.any()), f"{what}: {int(ne.sum())} of {ne.numel()} elements differ, first {a[ne][:4].tolist()} vs {b[ne][:4].tolist()}"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,Cin,Cout,T,KS,stride,mode,op", _scale_cases())
def test_conv_power_of_two_scale_invariance(kind, B, Cin, Cout, T, KS, stride, mode, op):
    """For k = -40 and +40: (2^k x, 2^-k w, bias) gives the bits of (x, w, bias), and (2^k x, w, 2^k bias) gives 2^k times them; the input
    gradient likewise with dy in x's place, the weight gradient with (2^k x, 2^-k dy) and (2^k x, dy); the bias gradient is 2^-k (1) times
    the unscaled one.  Multiplying by a power of two is exact and commutes with every rounding (fp32, bf16, each term of the three-term
    bf16 split) as long as nothing overflows or goes subnormal, and nothing does here: operands are randn at unit scale (|v| > 2^-20
    for all but one in 10^6), so at 2^-40 the smallest operand is about 2^-60, the third bf16 term of a unit-scale value about 2^-56 and
    a product of two such terms about 2^-112 > 2^-126; at 2^40 the largest accumulated value is about 2^40 * 2^6 << 2^127."""
    lib, dev = backend(kind)
    g = torch.Generator().manual_seed(B * 100 + T)
    x = torch.randn(B, Cin, T, generator=g)
    w = torch.randn(Cout, Cin, KS, generator=g) / (Cin * KS) ** 0.5
    bias = torch.randn(Cout, generator=g)
    Tout = O.pad_conv(torch.zeros(1, Cin, T), torch.zeros(Cout, Cin, KS), None, stride).shape[2]
    dy = torch.randn(B, Cout, Tout, generator=g)
    run = lambda a, b_, bi: _run_conv(lib, dev, mode, op, a, b_, bi, Cin, Cout, T, KS, stride)
    first = {"fwd": x, "dgrad": dy, "wgrad": x}[op]
    second = {"fwd": w, "dgrad": w, "wgrad": dy}[op]
    base = run(first, second, bias)
    for k in (-40, 40):
        s, si = 2.0 ** k, 2.0 ** -k
        tag = f"{kind} {mode} {op} k={k}"
        got = run(first * s, second * si, bias)
        _same_bits(got[0], base[0], f"{tag} (2^k a, 2^-k b)")
        if op == "wgrad":
            _same_bits(got[1], base[1] * si, f"{tag} bias gradient of 2^-k dy")
        got = run(first * s, second, bias * s)
        _same_bits(got[0], base[0] * s, f"{tag} (2^k a, b, 2^k bias)")
        if op == "wgrad":
            _same_bits(got[1], base[1], f"{tag} bias gradient of dy")
