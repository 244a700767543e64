"""Red-zone twins of the op-level kernel tests: every input sits in NaN red zones, every output / scratch buffer in sentinel red zones
(tests/redzone.py), the result is compared with the same torch restatement at the same tolerance as the entry point's own test
(tests/test_ops_conv.py, test_ops_rowops.py, test_conv_in_fuse.py, test_bf16_pairs.py), and every guard is asserted intact.

What this adds to those tests: a write past an output (partial tiles, 16-byte stores over a row end, a *_ws_floats that is a unit
short), a read past an input (clamped lanes, stale tiles), and a write into the gap of a strided view (gap 4: aligned row stride,
gap 3: odd row stride -- enabled for both backends only where the kernel addresses rows with scalar accesses or checks the strides
before it takes a vector path: conv_gemm.hip stages x with dword DMA and stores through conv_store_frag element by element,
conv_wgrad.hip's wg_wide16 and rowops.hip's to_pairs test sxb / sxc % 4).  The conv + InstanceNorm calls take strides for x / dy only
(y, out, res, g_out, dy_out are contiguous by their ABI): the strided operand goes through the same dword DMA, the 64-byte row stores
touch contiguous tensors.  kind='emu': the CPU lane-level simulator; kind='gpu': gfx950."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import avc_oracle as O
from tests import test_bf16_pairs as BP
from tests import test_conv_in_fuse as CF
from tests import test_ops_conv as OC
from tests import test_ops_rowops as RO
from tests.emu_util import KINDS, P, backend
from tests.redzone import GuardedOutput, guarded_input, guarded_like


def rows(table, pred=lambda v: True):
    """the non-GPU rows of an existing test's table"""
    return [tuple(e) for e in table if not hasattr(e, "marks") and pred(tuple(e))]


def with_gaps(cases, gapped):
    """every case at gap 0, the cases in `gapped` (indices) also at gap 4 and gap 3"""
    out = [c + (0,) for c in cases]
    for i in gapped:
        out += [cases[i] + (4,), cases[i] + (3,)]
    return out


def tout(T, KS, stride):
    padL, padR = KS // 2, (KS // 2 - 1 if KS % 2 == 0 else KS // 2)
    return (T + padL + padR - KS) // stride + 1


class Guards(list):
    def new(self, shape, dev, gap=0, dtype=torch.float32, init=None):
        self.append(GuardedOutput(shape, gap=gap, dtype=dtype, device=dev, init=init))
        return self[-1]

    def check(self, msg):
        for i, g in enumerate(self):
            g.assert_intact(f"({msg}, guarded buffer #{i} of shape {g.shape})")


def pair_image_finite(img):
    """a bf16 pair weight image: neither half of any dword is Inf / NaN"""
    b = img.view(torch.int32)
    return bool((((b >> 7) & 0xFF) != 0xFF).all() and (((b >> 23) & 0xFF) != 0xFF).all())


def rz_pack(lib, dev, ws, dgrad, pairs=False):
    """avc_pack_weight with the sources in NaN red zones and the image in sentinel red zones; returns the image RE-HOMED inside a NaN red
    zone, so that a conv that reads past avc_packed_weight_floats meets NaN."""
    Cout, Cin, KS = ws[0].shape[0] * len(ws), ws[0].shape[1], (ws[0].shape[2] if ws[0].dim() == 3 else 1)
    n = lib.avc_packed_weight_floats(Cout, Cin, KS, dgrad)
    assert n > 0
    srcs = [guarded_input(w, device=dev) for w in ws]
    dst = GuardedOutput((n,), device=dev)
    arr = (ctypes.c_void_p * len(ws))(*[w.data_ptr() for w in srcs])
    assert lib.avc_pack_weight(arr, len(ws), ws[0].shape[0], Cout, Cin, KS, dgrad, P(dst.view), None) == 0
    dst.assert_intact(f"(avc_pack_weight {Cout}x{Cin}x{KS} dgrad={dgrad} pairs={pairs})")
    assert pair_image_finite(dst.view) if pairs else bool(torch.isfinite(dst.view).all()), "the weight image is not fully written"
    return guarded_input(dst.view.clone())


def rz_pack_x3(lib, dev, w, dgrad):
    Cout, Cin, KS = w.shape
    n = lib.avc_packed_weight_floats_x3(Cout, Cin, KS, dgrad)
    assert n > 0
    dst = GuardedOutput((n,), device=dev)
    assert lib.avc_pack_weight_x3(P(guarded_input(w, device=dev)), Cout, Cin, KS, dgrad, P(dst.view), None) == 0
    dst.assert_intact(f"(avc_pack_weight_x3 {Cout}x{Cin}x{KS} dgrad={dgrad})")
    assert pair_image_finite(dst.view), "the split-bf16 weight image is not fully written"
    return guarded_input(dst.view.clone())


# ---------------------------------------------------------------------------------------------------------------
# weight images
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("KS", [1, 2, 5, 8])
@pytest.mark.parametrize("Cin", [5, 20, 44])
@pytest.mark.parametrize("Cout", [7, 33, 130])
def test_pack_weight_stays_inside_its_image(kind, Cout, Cin, KS):
    """Forward and dgrad images, fp32 and (op_compute_dtype 3) bf16 pair images; two stacked sources where Cout is even."""
    lib, dev = backend(kind)
    g = torch.Generator().manual_seed(Cout * 100 + Cin * 10 + KS)
    w = torch.randn(Cout, Cin, KS, generator=g)
    for dgrad in (0, 1):
        rz_pack(lib, dev, [w], dgrad)
        with BP.op_dtype(lib, 3):
            rz_pack(lib, dev, [w], dgrad, pairs=True)
    if Cout % 2 == 0:
        rz_pack(lib, dev, [w[:Cout // 2].contiguous(), w[Cout // 2:].contiguous()], 0)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("Cout,Cin,KS", [(48, 40, 1), (130, 80, 1), (32, 16, 5), (48, 32, 5), (144, 32, 5)])
def test_pack_weight_x3_stays_inside_its_image(kind, Cout, Cin, KS):
    lib, dev = backend(kind)
    w = torch.randn(Cout, Cin, KS, generator=torch.Generator().manual_seed(Cout + Cin))
    for dgrad in (0, 1):
        rz_pack_x3(lib, dev, w, dgrad)


# ---------------------------------------------------------------------------------------------------------------
# forward conv
# ---------------------------------------------------------------------------------------------------------------
def rz_conv_fwd(lib, dev, x, w, b, stride=1, act=0, tile=0, res=None, res_mode=0, ops=1, gap=0, transposed=False, wp=None, msg=""):
    B, Cin, Tin = x.shape
    Cout, _, KS = w.shape
    if wp is None:
        wp = rz_pack(lib, dev, [w], 0)
    To = tout(Tin, KS, stride)
    xg = guarded_input(x.transpose(1, 2).contiguous(), gap, dev).transpose(1, 2) if transposed else guarded_input(x, gap, dev)
    bg = guarded_input(b, device=dev)
    G = Guards()
    out = G.new((B, Cout // ops, To * ops), dev, gap)
    out2 = G.new((B, Cout // ops, To * ops), dev, gap) if res is not None else None
    rg = guarded_input(res, gap, dev) if res is not None else None
    rb, rc_, rt, Tres = (rg.stride(0), rg.stride(1), rg.stride(2), rg.shape[2]) if res is not None else (0, 0, 0, 0)
    rc = lib.avc_conv1d_fwd(P(xg), xg.stride(0), xg.stride(1), xg.stride(2), B, Cin, Tin, P(wp), P(bg), Cout, KS, stride, act, P(out.view),
                            out.view.stride(0), out.view.stride(1), out.view.stride(2), ops, P(rg), res_mode, rb, rc_, rt, Tres,
                            P(out2.view) if out2 else None, tile, None)
    assert rc == 0, rc
    G.check(f"avc_conv1d_fwd {msg} gap={gap}")
    return out.view.cpu(), (out2.view.cpu() if out2 else None)


FWD_CASES = rows(OC.FWD, lambda v: v[6] != 0) + [(1, 5, 7, 9, 3, 1, 0), (3, 13, 33, 65, 5, 1, 0), (2, 3, 70, 31, 7, 2, 0), (4, 9, 17, 6, 4, 1, 0)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,Cin,Cout,T,KS,stride,tile,gap", with_gaps(FWD_CASES, [1, 10, 17]))
def test_conv_fwd_in_red_zones(kind, B, Cin, Cout, T, KS, stride, tile, gap):
    lib, dev = backend(kind)
    g = torch.Generator().manual_seed(B * 1000 + T)
    x = torch.randn(B, Cin, T, generator=g)
    w = torch.randn(Cout, Cin, KS, generator=g) / (Cin * KS) ** 0.5
    b = torch.randn(Cout, generator=g)
    ref = torch.relu(O.pad_conv(x, w, b, stride))
    out, _ = rz_conv_fwd(lib, dev, x, w, b, stride, act=1, tile=tile, gap=gap, msg=f"{(B, Cin, Cout, T, KS, stride, tile)}")
    torch.testing.assert_close(out, ref, rtol=1e-5, atol=2e-5)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("gap", [0, 4, 3])
@pytest.mark.parametrize("res_mode,stride", [(2, 2), (1, 1)])
def test_conv_fwd_transposed_view_and_residual_joins_in_red_zones(kind, res_mode, stride, gap):
    """the collate view (strides (T*M, 1, M)) as input; out2 = out + [avg-pooled] residual"""
    lib, dev = backend(kind)
    g = torch.Generator().manual_seed(7)
    B, Cin, Cout, T = 2, 16, 32, 22
    x = torch.randn(B, T, Cin, generator=g).transpose(1, 2)
    w = torch.randn(Cout, Cin, 5, generator=g) / 9
    b = torch.randn(Cout, generator=g)
    res = torch.randn(B, Cout, T, generator=g)
    y = torch.relu(O.pad_conv(x, w, b, stride))
    out, out2 = rz_conv_fwd(lib, dev, x, w, b, stride, act=1, tile=11, res=res, res_mode=res_mode, gap=gap, transposed=True, msg="transposed + residual")
    torch.testing.assert_close(out, y, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(out2, y + (O.avg_pool_ceil(res, 2) if res_mode == 2 else res), rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("gap", [0, 4, 3])
def test_conv_fwd_pixel_shuffle_store_in_red_zones(kind, gap):
    lib, dev = backend(kind)
    g = torch.Generator().manual_seed(8)
    x = torch.randn(2, 16, 12, generator=g)
    w = torch.randn(64, 16, 5, generator=g) / 9
    b = torch.randn(64, generator=g)
    ref = O.pixel_shuffle_1d(O.pad_conv(x, w, b), 2)
    out, _ = rz_conv_fwd(lib, dev, x, w, b, 1, act=0, tile=11, ops=2, gap=gap, msg="pixel shuffle")
    torch.testing.assert_close(out, ref, rtol=1e-5, atol=1e-5)


# ---------------------------------------------------------------------------------------------------------------
# input gradient
# ---------------------------------------------------------------------------------------------------------------
def rz_conv_dgrad(lib, dev, dy, w, stride, T, tile=0, res=None, res_mode=0, mask=None, gap=0, wpd=None, msg=""):
    B, Cout, Tdy = dy.shape
    _, Cin, KS = w.shape
    if wpd is None:
        wpd = rz_pack(lib, dev, [w], 1)
    dyg = guarded_input(dy, gap, dev)
    G = Guards()
    dx = G.new((B, Cin, T), dev, gap)
    dx2 = G.new((B, Cin, T), dev, gap) if mask is not None else None
    mg = guarded_input(mask, gap, dev) if mask is not None else None     # (the mask is read at the OUTPUT's offsets: same geometry)
    rg = guarded_input(res, gap, dev) if res is not None else None
    rb, rc_, rt, Tres = (rg.stride(0), rg.stride(1), rg.stride(2), rg.shape[2]) if res is not None else (0, 0, 0, 0)
    rc = lib.avc_conv1d_dgrad(P(dyg), dyg.stride(0), dyg.stride(1), dyg.stride(2), 1, B, Cout, Tdy, P(wpd), Cin, KS, stride, T, P(dx.view),
                              dx.view.stride(0), dx.view.stride(1), dx.view.stride(2), P(rg), res_mode, rb, rc_, rt, Tres,
                              P(dx2.view) if dx2 else None, P(mg), tile, None)
    assert rc == 0, rc
    G.check(f"avc_conv1d_dgrad {msg} gap={gap}")
    return dx.view.cpu(), (dx2.view.cpu() if dx2 else None)


DG_CASES = rows(OC.DG, lambda v: v[6] != 0)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,Cin,Cout,T,KS,stride,tile,gap", with_gaps(DG_CASES, [1, 11, 16]))
def test_conv_dgrad_in_red_zones(kind, B, Cin, Cout, T, KS, stride, tile, gap):
    lib, dev = backend(kind)
    g = torch.Generator().manual_seed(B * 77 + T)
    x = torch.randn(B, Cin, T, generator=g, requires_grad=True)
    w = torch.randn(Cout, Cin, KS, generator=g) / (Cin * KS) ** 0.5
    y = O.pad_conv(x, w, None, stride)
    dy = torch.randn(y.shape, generator=g)
    (dx_ref,) = torch.autograd.grad(y, x, dy)
    dx, _ = rz_conv_dgrad(lib, dev, dy, w, stride, T, tile, gap=gap, msg=f"{(B, Cin, Cout, T, KS, stride, tile)}")
    torch.testing.assert_close(dx, dx_ref, rtol=1e-5, atol=2e-5)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("gap", [0, 4, 3])
@pytest.mark.parametrize("res_mode", [3, 4])
def test_conv_dgrad_join_and_mask_in_red_zones(kind, res_mode, gap):
    """dx = dgrad(dy) + the adjoint of the pool (3) / of the nearest x2 upsample (4) applied to g_next; dx2 = dx * (a_prev > 0)"""
    lib, dev = backend(kind)
    g = torch.Generator().manual_seed(11)
    B, C, T = 2, 32, 21
    w = torch.randn(C, C, 5, generator=g) / 12
    dy = torch.randn(B, C, T, generator=g)
    gnext = torch.randn(B, C, (T + 1) // 2 if res_mode == 3 else 2 * T, generator=g)
    a_prev = torch.randn(B, C, T, generator=g)
    x = torch.randn(B, C, T, generator=g, requires_grad=True)
    side = O.avg_pool_ceil(x, 2) if res_mode == 3 else x.repeat_interleave(2, dim=2)
    (ref,) = torch.autograd.grad([O.pad_conv(x, w, None, 1), side], x, [dy, gnext])
    dx, dx2 = rz_conv_dgrad(lib, dev, dy, w, 1, T, 11, res=gnext, res_mode=res_mode, mask=a_prev, gap=gap, msg=f"join {res_mode} + mask")
    torch.testing.assert_close(dx, ref, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(dx2, ref * (a_prev > 0), rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("T,ck", [(16, 16), (32, 32)])
def test_conv_with_deeper_chunks_in_red_zones(kind, T, ck):
    lib, dev = backend(kind)
    assert lib.avc_set_tuning(b"conv_ck5", ck) == 0
    try:
        g = torch.Generator().manual_seed(T)
        B, C = 5, 128
        x = torch.randn(B, C, T, generator=g, requires_grad=True)
        w = torch.randn(C, C, 5, generator=g) / (C * 5) ** 0.5
        b = torch.randn(C, generator=g)
        y = O.pad_conv(x, w, b, 1)
        dy = torch.randn(y.shape, generator=g)
        (dx_ref,) = torch.autograd.grad(y, x, dy)
        out, _ = rz_conv_fwd(lib, dev, x.detach(), w, b, 1, act=0, tile=11, msg=f"conv_ck5={ck}")
        torch.testing.assert_close(out, y.detach(), rtol=1e-5, atol=2e-5)
        dx, _ = rz_conv_dgrad(lib, dev, dy, w, 1, T, 11, msg=f"conv_ck5={ck}")
        torch.testing.assert_close(dx, dx_ref, rtol=1e-5, atol=2e-5)
    finally:
        lib.avc_set_tuning(b"conv_ck5", 8)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,Cin,Cout,T,stride", rows(OC.X3))
def test_conv_x3_tile_97_in_red_zones(kind, B, Cin, Cout, T, stride):
    """the split-bf16 kernel (tile code 97, its own weight image): forward and input gradient against the fp32 convolution"""
    lib, dev = backend(kind)
    KS = 5
    if stride < 0:
        KS, stride = 1, 1
    g = torch.Generator().manual_seed(B * 31 + T)
    x = torch.randn(B, Cin, T, generator=g)
    w = torch.randn(Cout, Cin, KS, generator=g) / (Cin * KS) ** 0.5
    b = torch.randn(Cout, generator=g)
    y32 = O.pad_conv(x, w, b, stride)
    out, _ = rz_conv_fwd(lib, dev, x, w, b, stride, act=0, tile=97, wp=rz_pack_x3(lib, dev, w, 0), msg="x3")
    torch.testing.assert_close(out, y32, rtol=1e-5, atol=2e-5)
    dy = torch.randn(y32.shape, generator=g)
    xg = x.clone().requires_grad_(True)
    (dx32,) = torch.autograd.grad(O.pad_conv(xg, w, None, stride), xg, dy)
    dx, _ = rz_conv_dgrad(lib, dev, dy, w, stride, T, 97, wpd=rz_pack_x3(lib, dev, w, 1), msg="x3")
    torch.testing.assert_close(dx, dx32, rtol=1e-5, atol=2e-5)


# ---------------------------------------------------------------------------------------------------------------
# weight gradient: dW, db and the scratch of avc_conv1d_wgrad_ws_floats
# ---------------------------------------------------------------------------------------------------------------
def rz_conv_wgrad(lib, dev, x, dy, Cout, KS, stride, gap=0, msg=""):
    B, Cin, T = x.shape
    To = dy.shape[2]
    xg, dyg = guarded_input(x, gap, dev), guarded_input(dy, gap, dev)
    G = Guards()
    ws = G.new((lib.avc_conv1d_wgrad_ws_floats(B, Cin, Cout, To, KS),), dev)
    dW = G.new((Cout, Cin, KS) if x.dtype == torch.float32 else (Cout, 2 * Cin, KS), dev)
    db = G.new((Cout,), dev)
    Cin_ = dW.shape[1]
    rc = lib.avc_conv1d_wgrad(P(xg), xg.stride(0), xg.stride(1), xg.stride(2), P(dyg), dyg.stride(0), dyg.stride(1), dyg.stride(2), 1, B, Cin_,
                              Cout, T, To, KS, stride, P(dW.view), P(db.view), P(ws.view), None)
    assert rc == 0, rc
    G.check(f"avc_conv1d_wgrad {msg} gap={gap} (buffers: scratch, dW, db)")
    return dW.view.cpu(), db.view.cpu()


def check_wgrad(lib, dev, B, Cin, Cout, T, KS, stride, gap=0):
    g = torch.Generator().manual_seed(B * 31 + T)
    x = torch.randn(B, Cin, T, generator=g)
    w = (torch.randn(Cout, Cin, KS, generator=g) / (Cin * KS) ** 0.5).requires_grad_(True)
    b = torch.zeros(Cout, requires_grad=True)
    y = O.pad_conv(x, w, b, stride)
    dy = torch.randn(y.shape, generator=g)
    dw_ref, _ = torch.autograd.grad(y, [w, b], dy)
    db_ref = dy.double().sum((0, 2)).float()      # (fp64: see tests/test_ops_conv.py)
    dW, db = rz_conv_wgrad(lib, dev, x, dy, Cout, KS, stride, gap, msg=f"{(B, Cin, Cout, T, KS, stride)}")
    torch.testing.assert_close(dW, dw_ref, rtol=1e-4, atol=1e-5 * max(1.0, dw_ref.abs().max().item()))
    torch.testing.assert_close(db, db_ref, rtol=1e-4, atol=1e-4)


WG_CASES = rows(OC.WG) + [(20, 16, 32, 5, 5, 2), (40, 8, 32, 5, 8, 1), (24, 16, 32, 7, 7, 2), (33, 16, 32, 1, 1, 1)]   # + the many-short-samples table


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,Cin,Cout,T,KS,stride,gap", with_gaps(WG_CASES, [1, 11, 15]))
def test_conv_wgrad_in_red_zones(kind, B, Cin, Cout, T, KS, stride, gap):
    lib, dev = backend(kind)
    check_wgrad(lib, dev, B, Cin, Cout, T, KS, stride, gap)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("knob,B,Cin,Cout,T,KS", [("wgrad_cw8", 3, 64, 128, 40, 5), ("wgrad_cw8", 2, 64, 128, 64, 5), ("wgrad_x3", 2, 16, 32, 32, 5),
                                                  ("wgrad_x3", 3, 64, 64, 64, 5), ("wgrad_x3", 2, 80, 32, 33, 4), ("wgrad_x3", 2, 16, 32, 70, 6),
                                                  ("wgrad_x3", 2, 8, 32, 19, 8), ("wgrad_x3", 2, 130, 40, 40, 1)])
def test_conv_wgrad_opt_in_instances_in_red_zones(kind, knob, B, Cin, Cout, T, KS):
    lib, dev = backend(kind)
    assert lib.avc_set_tuning(knob.encode(), 1) == 0
    try:
        check_wgrad(lib, dev, B, Cin, Cout, T, KS, 1)
    finally:
        lib.avc_set_tuning(knob.encode(), 0)


# ---------------------------------------------------------------------------------------------------------------
# conv + InstanceNorm in one call, forward and backward
# ---------------------------------------------------------------------------------------------------------------
IN_FWD_CASES = rows(CF.CASES) + [(3, 16, 32, 19, 5, 1, 1, True, 1, 1, 0)]    # + rows of 19 frames: two launches


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,Cin,Cout,Tin,KS,stride,ops,affine,relu,res_mode,want_fused,gap", with_gaps(IN_FWD_CASES, [0, 1, 2, 4, 8]))
def test_conv_in_fwd_in_red_zones(kind, B, Cin, Cout, Tin, KS, stride, ops, affine, relu, res_mode, want_fused, gap):
    """gap: x is a strided view with NaN after every row (rows of 64 / 32 / 16 frames fused, the pixel-shuffling conv, rows of 24 in two launches)"""
    lib, dev = backend(kind)
    g = torch.Generator().manual_seed(B * 13 + Tin)
    x = torch.randn(B, Cin, Tin, generator=g)
    w = torch.randn(Cout, Cin, KS, generator=g) / (Cin * KS) ** 0.5
    b = torch.randn(Cout, generator=g)
    C, T = Cout // ops, tout(Tin, KS, stride) * ops
    cond = torch.randn(B, 4 * C + 8, generator=g) if affine else None
    cond_off = 2 * C + 8 if affine else 0
    Tres = {0: 0, 1: T, 2: (Tin if stride == 2 else 2 * T), 5: T // 2}[res_mode]
    res = torch.randn(B, C, Tres, generator=g) if res_mode else None
    y_ref, o_ref = CF.reference(x, w, b, stride, ops, cond, cond_off, relu, res, res_mode)
    gi = lambda t: None if t is None else guarded_input(t, device=dev)
    wp = rz_pack(lib, dev, [w], 0)
    xg, bg, cg, rg = guarded_input(x, gap, dev), gi(b), gi(cond), gi(res)
    G = Guards()
    y, out, mean, rstd = G.new((B, C, T), dev), G.new((B, C, T), dev), G.new((B * C,), dev), G.new((B * C,), dev)
    fused = ctypes.c_int(-1)
    rc = lib.avc_conv1d_in_fwd(P(xg), xg.stride(0), xg.stride(1), xg.stride(2), B, Cin, Tin, P(wp), P(bg), Cout, KS, stride, ops, P(y.view), P(cg),
                               cg.stride(0) if affine else 0, cond_off, relu, P(rg), res_mode, Tres, P(out.view), P(mean.view), P(rstd.view),
                               ctypes.byref(fused), None)
    assert rc == 0, rc
    assert fused.value == want_fused
    G.check(f"avc_conv1d_in_fwd fused={fused.value} gap={gap} (buffers: y, out, mean, rstd)")
    torch.testing.assert_close(y.view.cpu(), y_ref, rtol=1e-5, atol=2e-5)
    torch.testing.assert_close(out.view.cpu(), o_ref, rtol=1e-4, atol=2e-5)
    torch.testing.assert_close(mean.view.cpu().view(B, C), y_ref.mean(2), rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(rstd.view.cpu().view(B, C), 1.0 / torch.sqrt(y_ref.var(2, unbiased=False) + 1e-5), rtol=1e-4, atol=1e-5)


IN_BWD_CASES = rows(CF.BWD_CASES) + [(3, 32, 16, 24, 5, 1, 1, True, 1, 0), (3, 32, 16, 19, 5, 1, 0, True, 2, 0)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,Cin,Cout,T,KS,stride,res_mode,affine,relu,want_fused,gap", with_gaps(IN_BWD_CASES, [0, 1, 2, 3, 8]))
def test_conv_dgrad_in_bwd_in_red_zones(kind, B, Cin, Cout, T, KS, stride, res_mode, affine, relu, want_fused, gap):
    """The guarded call against the two-launch path in plain buffers (pinned to autograd by tests/test_ops_conv.py and
    tests/test_ops_rowops.py), at the bars of tests/test_conv_in_fuse.py: g bit for bit, dy / dcond to summation order.  dcond is a
    channel slice of a wider row whose other floats hold the sentinel.  gap: dy is a strided view (NaN after every row) in the guarded
    call and an ordinary tensor of the same strides in the plain one."""
    lib, dev = backend(kind)
    g = torch.Generator().manual_seed(B * 7 + T)
    Tdy = tout(T, KS, stride)
    w = torch.randn(Cout, Cin, KS, generator=g) / (Cin * KS) ** 0.5
    dy = torch.randn(B, Cout, Tdy, generator=g)
    y = torch.randn(B, Cin, T, generator=g)
    mean = y.mean(2).reshape(-1)
    rstd = (1.0 / torch.sqrt(y.var(2, unbiased=False) + 1e-5)).reshape(-1)
    cond = torch.randn(B, 2 * Cin + 6, generator=g) if affine else None
    coff = 6 if affine else 0
    Tres = {0: 0, 1: T, 3: T // 2, 4: 2 * T}[res_mode]
    res = torch.randn(B, Cin, Tres, generator=g) if res_mode else None

    def go(guard):
        gi = (lambda t: None if t is None else guarded_input(t, device=dev)) if guard else (lambda t: None if t is None else t.to(dev))
        wpd = rz_pack(lib, dev, [w], 1) if guard else OC.pack(lib, dev, [w.to(dev)], 1)
        dyg = guarded_input(dy, gap, dev) if guard else torch.cat([dy, torch.zeros(B, Cout, gap)], 2).to(dev)[..., :Tdy]
        yg, mg, sg, cg, rg = gi(y), gi(mean), gi(rstd), gi(cond), gi(res)
        G = Guards()
        gout, dyo = G.new((B, Cin, T), dev), G.new((B, Cin, T), dev)
        dcond = G.new((B, 2 * Cin), dev, gap=6, init=torch.zeros(B, 2 * Cin)) if affine else None   # rows of 2 Cin + 6 floats, the slice starts at float 6 of its row
        dcp = ctypes.c_void_p(dcond.view.data_ptr() - 4 * coff) if affine else None
        fused = ctypes.c_int(-1)
        rc = lib.avc_conv1d_dgrad_in_bwd(P(dyg), dyg.stride(0), dyg.stride(1), 1, 1, B, Cout, Tdy, P(wpd), Cin, KS, stride, T, P(gout.view), P(rg),
                                         res_mode, Tres, P(yg), P(mg), P(sg), P(cg), cg.stride(0) if affine else 0, coff, relu, P(dyo.view),
                                         dcp, dcond.view.stride(0) if affine else 0, coff, ctypes.byref(fused), None)
        assert rc == 0, rc
        if guard:
            G.check(f"avc_conv1d_dgrad_in_bwd fused={fused.value} gap={gap} (buffers: g_out, dy_out, dcond slice)")
        return gout.view.cpu(), dyo.view.cpu(), (dcond.view.cpu() if affine else None), fused.value

    g1, d1, c1, fused = go(True)
    assert fused == want_fused
    assert lib.avc_set_tuning(b"conv_in_fuse", 0) == 0
    try:
        g2, d2, c2, fused2 = go(False)
    finally:
        lib.avc_set_tuning(b"conv_in_fuse", 1)
    assert fused2 == 0
    assert torch.isfinite(d1).all() and torch.isfinite(g1).all()
    assert torch.equal(g1, g2)
    torch.testing.assert_close(d1, d2, rtol=1e-4, atol=1e-5 * max(d2.abs().max().item(), 1.0))
    if affine:
        torch.testing.assert_close(c1, c2, rtol=1e-4, atol=1e-4)


# ---------------------------------------------------------------------------------------------------------------
# InstanceNorm / AdaIN rows
# ---------------------------------------------------------------------------------------------------------------
IN_ROWS = rows(RO.IN_CASES) + [(1, 3, 301, True, 0), (5, 7, 2, True, 1), (2, 3, 36, True, 2)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,C,T,affine,res_mode", IN_ROWS)
def test_instnorm_fwd_bwd_in_red_zones(kind, B, C, T, affine, res_mode):
    lib, dev = backend(kind)
    g = torch.Generator().manual_seed(T * 10 + B)
    y = (torch.randn(B, C, T, generator=g) * 2 + 0.5).requires_grad_(True)
    cond_all = torch.randn(B, 3 * 2 * C, generator=g)
    off = 2 * C
    cond = cond_all[:, off:off + 2 * C].clone().requires_grad_(True) if affine else None
    res = {0: None, 1: torch.randn(B, C, T, generator=g), 2: torch.randn(B, C, 2 * T - (1 if T % 2 == 1 else 0), generator=g),
           5: torch.randn(B, C, T // 2, generator=g)}[res_mode]
    Tres = res.shape[2] if res is not None else 0
    ref = RO.ref_block(y, cond, True, res, res_mode)
    yd, cd = guarded_input(y.detach(), device=dev), guarded_input(cond_all, device=dev)
    rd = guarded_input(res, device=dev) if res is not None else None
    G = Guards()
    out, mean, rstd = G.new((B, C, T), dev), G.new((B * C,), dev), G.new((B * C,), dev)
    rc = lib.avc_instnorm_fwd(P(yd), B, C, T, P(cd if affine else None), cd.stride(0), off, 1, P(rd), res_mode, Tres, P(out.view), P(mean.view),
                              P(rstd.view), None)
    assert rc == 0
    G.check("avc_instnorm_fwd (buffers: out, mean, rstd)")
    torch.testing.assert_close(out.view.cpu(), ref.detach(), rtol=1e-5, atol=2e-5)
    torch.testing.assert_close(mean.view.cpu().view(B, C), y.detach().mean(-1), rtol=1e-5, atol=1e-5)
    # rstd = 1 / sqrt(var + eps): the fp64 value; the kernel's two-pass fp32 variance carries a few ulp of the T-term sums (tests/test_conv_in_fuse.py
    # holds the fused epilogue's rstd to the same bar)
    torch.testing.assert_close(rstd.view.cpu().view(B, C), (1.0 / torch.sqrt(y.detach().double().var(-1, unbiased=False) + 1e-5)).float(), rtol=1e-4, atol=1e-5)
    gout = torch.randn(B, C, T, generator=g)
    grads = torch.autograd.grad(ref, [y] + ([cond] if affine else []), gout)
    G2 = Guards()
    dy = G2.new((B, C, T), dev)
    # dcond: the channel slice [off, off + 2C) of rows of 6C floats; everything outside the slice is sentinel
    dcond = G2.new((B, 2 * C), dev, gap=4 * C, init=torch.zeros(B, 2 * C))
    dcp = ctypes.c_void_p(dcond.view.data_ptr() - 4 * off)
    gd = guarded_input(gout, device=dev)
    md, sd = guarded_input(mean.view.clone()), guarded_input(rstd.view.clone())
    rc = lib.avc_instnorm_bwd(P(gd), P(yd), P(md), P(sd), B, C, T, P(cd if affine else None), cd.stride(0), off, 1, P(dy.view),
                              dcp if affine else None, dcond.view.stride(0), off, None)
    assert rc == 0
    G2.check("avc_instnorm_bwd (buffers: dy, dcond slice)")
    torch.testing.assert_close(dy.view.cpu(), grads[0], rtol=2e-4, atol=2e-5)
    if affine:
        torch.testing.assert_close(dcond.view.cpu(), grads[1], rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("planar", [0, 1])
@pytest.mark.parametrize("T", [4, 12, 64, 132])
@pytest.mark.parametrize("C", [2, 6, 34])
def test_pairs_instnorm_fwd_bwd_in_red_zones(kind, C, T, planar):
    lib, dev = backend(kind)
    B = 2
    res_mode = {4: 0, 12: 1, 64: 5, 132: 2}[T]
    g = torch.Generator().manual_seed(T * 10 + C)
    y = BP.bf16r(torch.randn(B, C, T, generator=g) * 2 + 0.5).requires_grad_(True)
    cond_all = torch.randn(B, 3 * 2 * C, generator=g)
    off = 2 * C
    cond = cond_all[:, off:off + 2 * C].clone().requires_grad_(True)
    res = {0: None, 1: torch.randn(B, C, T, generator=g), 2: torch.randn(B, C, 2 * T, generator=g), 5: torch.randn(B, C, T // 2, generator=g)}[res_mode]
    res = BP.bf16r(res) if res is not None else None
    Tres = res.shape[2] if res is not None else 0
    ref = BP.ref_block(y, cond, res, res_mode)
    yd = guarded_input(BP.to_planar(y.detach()) if planar else BP.to_pairs(y.detach()), device=dev)
    cd = guarded_input(cond_all, device=dev)
    rd = guarded_input(BP.to_pairs(res), device=dev) if res is not None else None
    G = Guards()
    out, mean, rstd = G.new((B, C // 2, T), dev, dtype=torch.int32), G.new((B * C,), dev), G.new((B * C,), dev)
    rc = lib.avc_instnorm_fwd_pairs(P(yd), B, C, T, P(cd), cd.stride(0), off, 1, P(rd), res_mode, Tres, planar, P(out.view), P(mean.view), P(rstd.view), None)
    assert rc == 0, rc
    G.check("avc_instnorm_fwd_pairs (buffers: out, mean, rstd)")
    got = BP.from_pairs(out.view.cpu())
    assert torch.isfinite(got).all()
    BP.close_bf16(got, ref.detach(), atol=2e-5)
    torch.testing.assert_close(mean.view.cpu().view(B, C), y.detach().mean(-1), rtol=1e-5, atol=1e-5)
    gout = BP.bf16r(torch.randn(B, C, T, generator=g))
    grads = torch.autograd.grad(ref, [y, cond], gout)
    G2 = Guards()
    dy = G2.new(tuple(yd.shape), dev, dtype=torch.int32)
    dcond = G2.new((B, 2 * C), dev, gap=4 * C, init=torch.zeros(B, 2 * C))
    dcp = ctypes.c_void_p(dcond.view.data_ptr() - 4 * off)
    gd = guarded_input(BP.to_pairs(gout), device=dev)
    md, sd = guarded_input(mean.view.clone()), guarded_input(rstd.view.clone())
    rc = lib.avc_instnorm_bwd_pairs(P(gd), P(yd), P(md), P(sd), B, C, T, P(cd), cd.stride(0), off, 1, planar, P(dy.view), dcp, dcond.view.stride(0), off, None)
    assert rc == 0, rc
    G2.check("avc_instnorm_bwd_pairs (buffers: dy, dcond slice)")
    got = BP.from_planar(dy.view.cpu()) if planar else BP.from_pairs(dy.view.cpu())
    assert torch.isfinite(got).all()
    BP.close_bf16(got, grads[0], atol=1e-4)
    torch.testing.assert_close(dcond.view.cpu(), grads[1], rtol=2e-4, atol=2e-4)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("gap", [0, 4, 3])
@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("B,C,T", [(2, 6, 9), (1, 34, 64), (3, 2, 132)])
def test_to_pairs_in_red_zones(kind, B, C, T, transposed, gap):
    lib, dev = backend(kind)
    x = torch.randn(B, C, T, generator=torch.Generator().manual_seed(3))
    xg = guarded_input(x.transpose(1, 2).contiguous(), gap, dev).transpose(1, 2) if transposed else guarded_input(x, gap, dev)
    dst = GuardedOutput((B, C // 2, T), dtype=torch.int32, device=dev)
    assert lib.avc_to_pairs(P(xg), xg.stride(0), xg.stride(1), xg.stride(2), B, C, T, P(dst.view), None) == 0
    dst.assert_intact("(avc_to_pairs)")
    torch.testing.assert_close(BP.from_pairs(dst.view.cpu()), BP.bf16r(x), rtol=0, atol=0)


# ---------------------------------------------------------------------------------------------------------------
# op-level convs with bf16 operands (compute 1), pair tensors (3) and pair operands with fp32 outputs (4)
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_conv_bf16_operand_mode_in_red_zones(kind):
    lib, dev = backend(kind)
    B, Cin, Cout, T, KS, stride = 2, 40, 32, 32, 5, 1
    g = torch.Generator().manual_seed(7 * B + T)
    x = torch.randn(B, Cin, T, generator=g)
    w = torch.randn(Cout, Cin, KS, generator=g) / (Cin * KS) ** 0.5
    b = torch.randn(Cout, generator=g)
    lib.avc_set_tuning(b"compute", 1)
    try:
        out, _ = rz_conv_fwd(lib, dev, x, w, b, stride, act=1, msg="compute 1")
        torch.testing.assert_close(out, torch.relu(O.pad_conv(BP.bf16r(x), BP.bf16r(w), b, stride)), rtol=1e-4, atol=1e-5)
        wr = w.clone().requires_grad_(True)
        y = O.pad_conv(BP.bf16r(x), wr, None, stride)
        dy = torch.randn(y.shape, generator=g)
        (dw_ref,) = torch.autograd.grad(y, [wr], BP.bf16r(dy))
        dW, db = rz_conv_wgrad(lib, dev, x, dy, Cout, KS, stride, msg="compute 1")
        torch.testing.assert_close(dW, dw_ref, rtol=1e-4, atol=1e-5 * max(1.0, dw_ref.abs().max().item()))
        torch.testing.assert_close(db, dy.sum((0, 2)), rtol=1e-4, atol=1e-4)
        xg = x.clone().requires_grad_(True)
        (dx_ref,) = torch.autograd.grad(O.pad_conv(xg, w, None, stride), [xg], dy)
        dx, _ = rz_conv_dgrad(lib, dev, dy, w, stride, T, 0, msg="compute 1")
        err = ((dx - dx_ref).norm() / dx_ref.norm()).item()
        assert 1e-5 < err < 1e-2, err
    finally:
        lib.avc_set_tuning(b"compute", 0)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("gap", [0, 4, 3])
def test_pair_convs_in_red_zones(kind, gap):
    """compute 3: pair tensors in and out (strides in dwords), forward + input gradient + weight gradient; compute 4: the forward with
    an fp32 output.  Shapes of tests/test_bf16_pairs.py."""
    lib, dev = backend(kind)
    B, Cin, Cout, T, KS, stride = 2, 32, 32, 32, 5, 1
    g = torch.Generator().manual_seed(B * 1000 + T)
    x = torch.randn(B, Cin, T, generator=g)
    w = torch.randn(Cout, Cin, KS, generator=g) / (Cin * KS) ** 0.5
    b = torch.randn(Cout, generator=g)
    ref = torch.relu(O.pad_conv(BP.bf16r(x).double(), BP.bf16r(w).double(), b.double(), stride)).float()
    for dtype in (3, 4):
        with BP.op_dtype(lib, dtype):
            wp = rz_pack(lib, dev, [w], 0, pairs=True)
            xp, bg = guarded_input(BP.to_pairs(x), gap, dev), guarded_input(b, device=dev)
            out = GuardedOutput((B, Cout // 2, T), gap, torch.int32, dev) if dtype == 3 else GuardedOutput((B, Cout, T), gap, device=dev)
            rc = lib.avc_conv1d_fwd(P(xp), xp.stride(0), xp.stride(1), 1, B, Cin, T, P(wp), P(bg), Cout, KS, stride, 1, P(out.view), out.view.stride(0),
                                    out.view.stride(1), 1, 1, None, 0, 0, 0, 0, 0, None, 11, None)
        assert rc == 0, rc
        out.assert_intact(f"(pair conv forward, compute {dtype}, gap {gap})")
        if dtype == 3:
            got = BP.from_pairs(out.view.cpu())
            assert torch.isfinite(got).all()
            BP.close_bf16(got, ref)
        else:
            torch.testing.assert_close(out.view.cpu(), ref, rtol=1e-4, atol=1e-4)
    # input gradient
    x64 = torch.randn(B, Cin, T, generator=g, dtype=torch.float64, requires_grad=True)
    y = O.pad_conv(x64, BP.bf16r(w).double(), None, stride)
    dy = torch.randn(y.shape, generator=g)
    (dx_ref,) = torch.autograd.grad(y, x64, BP.bf16r(dy).double())
    with BP.op_dtype(lib, 3):
        wpd = rz_pack(lib, dev, [w], 1, pairs=True)
        dyp = guarded_input(BP.to_pairs(dy), gap, dev)
        dx = GuardedOutput((B, Cin // 2, T), gap, torch.int32, dev)
        rc = lib.avc_conv1d_dgrad(P(dyp), dyp.stride(0), dyp.stride(1), 1, 1, B, Cout, T, P(wpd), Cin, KS, stride, T, P(dx.view), dx.view.stride(0),
                                  dx.view.stride(1), 1, None, 0, 0, 0, 0, 0, None, None, 11, None)
    assert rc == 0, rc
    dx.assert_intact(f"(pair conv dgrad, gap {gap})")
    got = BP.from_pairs(dx.view.cpu())
    assert torch.isfinite(got).all()
    BP.close_bf16(got, dx_ref.float(), atol=2e-3)
    # weight gradient
    w64 = (torch.randn(Cout, Cin, KS, generator=g, dtype=torch.float64) / (Cin * KS) ** 0.5).requires_grad_(True)
    b64 = torch.zeros(Cout, dtype=torch.float64, requires_grad=True)
    y = O.pad_conv(BP.bf16r(x).double(), w64, b64, stride)
    dw_ref, db_ref = torch.autograd.grad(y, [w64, b64], BP.bf16r(dy).double())
    with BP.op_dtype(lib, 3):
        dW, db = rz_conv_wgrad(lib, dev, BP.to_pairs(x), BP.to_pairs(dy), Cout, KS, stride, gap, msg="pairs")
    torch.testing.assert_close(dW, dw_ref.float(), rtol=1e-4, atol=1e-5 * max(1.0, dw_ref.abs().max().item()))
    torch.testing.assert_close(db, db_ref.float(), rtol=1e-4, atol=1e-4)


# ---------------------------------------------------------------------------------------------------------------
# segment feed, optimizer step
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("M,T", [(5, 37), (16, 24)])
def test_gather_segments_in_red_zones(kind, M, T):
    """out[b, m, t] = corpus[starts[b] + t, m]; the corpus sits in a NaN red zone and one segment ends on its last row"""
    lib, dev = backend(kind)
    n_rows = T + 29
    corpus = torch.randn(n_rows, M, generator=torch.Generator().manual_seed(M))
    starts = torch.tensor([n_rows - T, 0, 7, 29, 1], dtype=torch.int64)
    cg = guarded_input(corpus, device=dev)
    out = GuardedOutput((len(starts), M, T), device=dev)
    # starts (int64) sits between valid row indices (0): an index read past its B entries can only produce a segment past out's B, i.e. a
    # breached guard, never a wild address
    sg = torch.zeros(len(starts) + 128, dtype=torch.int64)
    sg[64:64 + len(starts)] = starts
    sg = sg.to(dev)[64:64 + len(starts)]
    assert lib.avc_gather_segments(P(cg), n_rows, M, P(sg), len(starts), T, P(out.view), None) == 0
    out.assert_intact("(avc_gather_segments)")
    ref = torch.stack([corpus[s:s + T].t() for s in starts.tolist()])
    assert torch.equal(out.view.cpu(), ref)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("write_clipped", [0, 1])
@pytest.mark.parametrize("n", [1, 3, 1023, 4097])
def test_clip_adam_step_in_red_zones(kind, n, write_clipped):
    """Two steps (the second one clips) against torch.optim.Adam at the bars of tests/test_ops_rowops.py; p, g, m, v, vmax, the scratch
    of avc_clip_adam_ws_floats and gnorm_out guarded.  write_clipped = 0 leaves g bit-unchanged."""
    lib, dev = backend(kind)
    g = torch.Generator().manual_seed(3)
    p0 = torch.randn(n, generator=g)
    p_ref = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([p_ref], lr=5e-4, betas=(0.9, 0.999), amsgrad=True, weight_decay=1e-4)
    G = Guards()
    z = torch.zeros(n)
    p, m, v, vmax = G.new((n,), dev, init=p0), G.new((n,), dev, init=z), G.new((n,), dev, init=z), G.new((n,), dev, init=z)
    ws = G.new((lib.avc_clip_adam_ws_floats(n),), dev, init=torch.zeros(lib.avc_clip_adam_ws_floats(n)))
    gn = G.new((1,), dev)
    for step in (1, 2):
        grad = torch.randn(n, generator=g) * ((30.0 if step == 2 else 0.01) / n ** 0.5)   # step 2 clips (max_norm 5)
        p_ref.grad = grad.clone()
        gn_ref = torch.nn.utils.clip_grad_norm_([p_ref], 5.0)
        opt.step()
        gbuf = G.new((n,), dev, init=grad)
        rc = lib.avc_clip_adam_step(P(p.view), P(gbuf.view), P(m.view), P(v.view), P(vmax.view), n, step, 5e-4, 0.9, 0.999, 1e-8, 1e-4, 1, 5.0, 1.0,
                                    write_clipped, P(ws.view), P(gn.view), None)
        assert rc == 0
        G.check(f"avc_clip_adam_step n={n} step={step} (buffers: p, m, v, vmax, scratch, gnorm, g...)")
        assert gn.view.item() == pytest.approx(grad.double().norm().item(), rel=2e-6)
        assert gn.view.item() == pytest.approx(gn_ref.item(), rel=1e-5)
        if write_clipped:
            torch.testing.assert_close(gbuf.view.cpu(), p_ref.grad, rtol=1e-5, atol=1e-7)
        else:
            assert torch.equal(gbuf.view.cpu().view(torch.int32), grad.view(torch.int32)), "write_clipped = 0 changed g"
        torch.testing.assert_close(p.view.cpu(), p_ref.detach(), rtol=1e-5, atol=1e-6)


# ---------------------------------------------------------------------------------------------------------------
# DSP: framing and element-wise ops at the simulator's small hyper-parameters and an odd signal length
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_dsp_ops_in_red_zones(kind):
    from oracle import dsp_oracle as D
    from scipy import signal
    from tests.test_dsp import speechlike
    lib, dev = backend(kind)
    hp = D.small_hyperparams()
    n_fft, hop, win, F = hp.n_fft, hp.hop_length, hp.win_length, hp.n_fft // 2 + 1
    L = 437
    y = speechlike(L, hp.sr)
    yt = torch.from_numpy(y.astype(np.float32))
    # bases
    basis = []
    for inv in (0, 1):
        G = Guards()
        scratch = G.new((lib.avc_dsp_basis_scratch_floats(n_fft, win),), dev)
        packed = G.new((lib.avc_dsp_basis_floats(n_fft, win, inv),), dev)
        assert lib.avc_dsp_make_basis(n_fft, hop, win, inv, P(scratch.view), P(packed.view), None) == 0
        G.check(f"avc_dsp_make_basis inverse={inv} (buffers: scratch, basis)")
        assert torch.isfinite(packed.view).all()
        basis.append(guarded_input(packed.view.clone()))
    # stft
    T = lib.avc_dsp_num_frames(L, hop)
    G = Guards()
    frames, spec = G.new((win * T,), dev), G.new((2 * F, T), dev)
    yg = guarded_input(yt, device=dev)
    assert lib.avc_dsp_stft(P(yg), L, n_fft, hop, win, P(basis[0]), P(frames.view), P(spec.view), None) == 0
    G.check("avc_dsp_stft (buffers: frames_ws, spec)")
    ref = D.stft(y, n_fft, hop, win)
    s = spec.view.double().cpu().numpy()
    S = s[0::2] + 1j * s[1::2]
    assert S.shape == ref.shape
    assert np.abs(S - ref).max() <= 2e-5 * np.abs(ref).max()
    # istft of the oracle's spectrum
    G = Guards()
    tf, back = G.new((win * T,), dev), G.new((hop * (T - 1),), dev)
    sg = guarded_input(torch.from_numpy(np.stack([ref.real, ref.imag], axis=1).reshape(2 * F, -1).astype(np.float32)), device=dev)
    assert lib.avc_dsp_istft(P(sg), T, n_fft, hop, win, P(basis[1]), P(tf.view), P(back.view), None) == 0
    G.check("avc_dsp_istft (buffers: tf_ws, y)")
    want = D.istft(ref, hop, win)
    np.testing.assert_allclose(back.view.cpu().numpy(), want, atol=2e-5 * np.abs(want).max())
    # magnitude
    mag = GuardedOutput((F, T), device=dev)
    assert lib.avc_dsp_magnitude(P(sg), n_fft, T, P(mag.view), None) == 0
    mag.assert_intact("(avc_dsp_magnitude)")
    np.testing.assert_allclose(mag.view.cpu().numpy(), np.abs(ref), rtol=1e-5, atol=1e-6 * np.abs(ref).max())
    # dB normalisation [C][T] -> [T][C] and back to amplitudes [T][C] -> [C][T]
    amp = np.abs(ref).astype(np.float32) + 1e-3
    norm = GuardedOutput((T, F), device=dev)
    assert lib.avc_dsp_db_normalize(P(guarded_input(torch.from_numpy(amp), device=dev)), F, T, float(hp.ref_db), float(hp.max_db), P(norm.view), None) == 0
    norm.assert_intact("(avc_dsp_db_normalize)")
    want = np.clip((20 * np.log10(np.maximum(1e-5, amp.astype(np.float64))) - hp.ref_db + hp.max_db) / hp.max_db, 1e-8, 1).T
    np.testing.assert_allclose(norm.view.cpu().numpy(), want, atol=1e-4)
    den = GuardedOutput((F, T), device=dev)
    assert lib.avc_dsp_denormalize_amp(P(guarded_input(torch.from_numpy(want.astype(np.float32)), device=dev)), F, T, float(hp.ref_db), float(hp.max_db),
                                       P(den.view), None) == 0
    den.assert_intact("(avc_dsp_denormalize_amp)")
    want_amp = np.power(10.0, 0.05 * (np.clip(want.astype(np.float32).astype(np.float64), 0, 1) * hp.max_db - hp.max_db + hp.ref_db)).T
    np.testing.assert_allclose(den.view.cpu().numpy(), want_amp, rtol=1e-4)
    # pre- / de-emphasis, frame power
    pre = GuardedOutput((L,), device=dev)
    assert lib.avc_dsp_preemphasis(P(yg), L, 0.97, P(pre.view), None) == 0
    pre.assert_intact("(avc_dsp_preemphasis)")
    y32 = y.astype(np.float32).astype(np.float64)
    np.testing.assert_allclose(pre.view.cpu().numpy(), np.append(y32[0], y32[1:] - 0.97 * y32[:-1]), atol=2e-6 * np.abs(y).max())
    de = GuardedOutput((L,), device=dev)
    assert lib.avc_dsp_deemphasis(P(yg), L, 0.97, P(de.view), None) == 0
    de.assert_intact("(avc_dsp_deemphasis)")
    want = signal.lfilter([1], [1, -0.97], y32)
    np.testing.assert_allclose(de.view.cpu().numpy(), want, atol=2e-5 * np.abs(want).max())
    fl, fh = 64, 16
    nf = lib.avc_dsp_num_frames(L, fh)
    pw = GuardedOutput((nf,), device=dev)
    assert lib.avc_dsp_frame_power(P(yg), L, fl, fh, P(pw.view), None) == 0
    pw.assert_intact("(avc_dsp_frame_power)")
    yp = np.pad(y32, fl // 2, mode="reflect")
    idx = np.arange(fl)[:, None] + fh * np.arange(nf)[None, :]
    np.testing.assert_allclose(pw.view.cpu().numpy(), np.mean(yp[idx] ** 2, axis=0), rtol=1e-4)
