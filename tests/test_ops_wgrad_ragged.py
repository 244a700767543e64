"""avc_conv1d_wgrad_ragged (csrc/conv_wgrad_ragged.hip): the Conv1d weight / bias gradient over packed rows of UNEQUAL length, against torch
fp64 autograd of conv1d(reflect_pad(x_b)) per sample, summed.

kind='emu': the CPU lane-level simulation of the same kernel; kind='gpu': the gfx950 library.  Shapes: the smallest at which this kernel
can go wrong -- its tile is 64 co x 64 ci and its K-chunk 32 frames of one sample, so lengths sit inside / at / one past a chunk edge and a
forward conv tile edge (31, 32, 33, 63, 64, 65), next to the shortest legal length of the tap count; channel counts are no multiple of the
MFMA block (16, 40, 48) and two cases cross the 64-channel tile in ci and in co (80, 72); the first channel of both operands is non-zero
and the unused channels of every block hold NaN.  B = 7 with these lengths is 14-18 chunks: split three or four ways through the slots;
B = 1 runs unsplit and writes dW / db directly.

Bar: rel-L2 <= 1e-5 per tensor against fp64.  Where it comes from: the products run on the fp32 MFMA, an fp32 fma chain along K (one
rounding per product, u = 6e-8); K = sum of the output lengths <= 353 here, a random-sign sum of K terms carries a relative error of about
sqrt(K) u = 1.1e-6 and the slot sums add a few u: 1e-5 leaves a factor of about eight and is the figure the equal-length comparison with
avc_conv1d_wgrad uses."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests.emu_util import KINDS, P, backend
from tests.redzone import GuardedOutput, guarded_input
from tests.test_submodules import rel

BAR = 1e-5
EDGES = [31, 32, 33, 63, 64, 65]


def _ints(v):
    return (ctypes.c_int * len(v))(*v)


def _case(k, stride, Cin, Cout, T, db=True, xpad=(3, 5), ypad=(2, 1), seed=0):
    """Packed operands with xpad / ypad = (channels in front, channels behind) of NaN around the used channels of every block."""
    g = torch.Generator().manual_seed(1000 * k + 10 * stride + len(T) + seed)
    xC, xc0 = xpad[0] + Cin + xpad[1], xpad[0]
    dyC, dyc0 = ypad[0] + Cout + ypad[1], ypad[0]
    xs = [torch.randn(Cin, t, generator=g) for t in T]
    dys = [torch.randn(Cout, -(-t // stride), generator=g) for t in T]

    def pack(blocks, C, c0):
        out = []
        for b in blocks:
            full = torch.full((C, b.shape[1]), float("nan"))
            full[c0:c0 + b.shape[0]] = b
            out.append(full.reshape(-1))
        return torch.cat(out)
    return dict(k=k, stride=stride, Cin=Cin, Cout=Cout, T=list(T), db=db, xC=xC, xc0=xc0, dyC=dyC, dyc0=dyc0, xs=xs, dys=dys,
                x=pack(xs, xC, xc0), dy=pack(dys, dyC, dyc0))


def _reference(c):
    """fp64: sum over the samples of the autograd gradient of <conv1d(reflect_pad(x_b), W) + b, dy_b>"""
    k, s = c["k"], c["stride"]
    w = torch.zeros(c["Cout"], c["Cin"], k, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(c["Cout"], dtype=torch.float64, requires_grad=True)
    loss = 0
    for x, dy in zip(c["xs"], c["dys"]):
        xp = F.pad(x.double()[None], (k // 2, k // 2 - 1 if k % 2 == 0 else k // 2), mode="reflect") if k > 1 else x.double()[None]
        y = F.conv1d(xp, w, b, stride=s)
        assert y.shape[2] == dy.shape[1]
        loss = loss + (y[0] * dy.double()).sum()
    return torch.autograd.grad(loss, [w, b])


def _run(lib, dev, c, x=None, dy=None, dW=None, db=None, ws=None):
    n = lib.avc_conv1d_wgrad_ragged_ws_floats(len(c["T"]), _ints(c["T"]), c["Cin"], c["Cout"], c["k"], c["stride"])
    assert n > 0
    x = c["x"].to(dev) if x is None else x
    dy = c["dy"].to(dev) if dy is None else dy
    dW = torch.full((c["Cout"], c["Cin"], c["k"]), float("nan"), device=dev) if dW is None else dW
    db = (torch.full((c["Cout"],), float("nan"), device=dev) if c["db"] else None) if db is None else db
    ws = torch.full((n,), float("nan"), device=dev) if ws is None else ws
    rc = lib.avc_conv1d_wgrad_ragged(P(x), c["xC"], c["xc0"], P(dy), c["dyC"], c["dyc0"], len(c["T"]), _ints(c["T"]), c["Cin"], c["Cout"],
                                     c["k"], c["stride"], P(dW), P(db), P(ws), None)
    assert rc == 0, rc
    return dW, db, n


def _check(c, dW, db, tag):
    rw, rb = _reference(c)
    assert not torch.isnan(dW).any()
    e = rel(dW.cpu(), rw)
    print(f"[{tag}] k={c['k']} s={c['stride']} {c['Cin']}->{c['Cout']} T={c['T']}: dW rel-L2 {e:.3e}", end="")
    assert e <= BAR, e
    if db is not None:
        assert not torch.isnan(db).any()
        eb = rel(db.cpu(), rb)
        print(f", db rel-L2 {eb:.3e}", end="")
        assert eb <= BAR, eb
    print()


CIN = [16, 40, 48, 16, 40, 48, 16, 40]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("k", range(1, 9))
def test_mixed_lengths_every_tap_count(kind, k, stride):
    """1. B = 7: the six chunk / tile edges and the shortest legal length of the tap count (pad < T), odd lengths under stride 2, even k =
    asymmetric pads, a non-zero first channel in NaN-padded blocks; db present for odd k, NULL for even k."""
    lib, dev = backend(kind)
    c = _case(k, stride, CIN[k - 1], 32 if k % 2 else 48, EDGES + [k // 2 + 1], db=bool(k % 2))
    dW, db, _ = _run(lib, dev, c)
    _check(c, dW, db, kind)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k,stride,Cin,Cout,T,db", [(5, 1, 40, 32, [65], True), (4, 2, 16, 48, [33], False), (8, 2, 48, 32, [5], True),
                                                    (1, 1, 16, 32, [1], True), (3, 2, 80, 72, [64, 17, 65, 31, 130], True),
                                                    (2, 1, 80, 72, [199], False)])
def test_single_samples_and_tiles_across_64_channels(kind, k, stride, Cin, Cout, T, db):
    """1. B = 1 (unsplit: the kernel writes dW / db itself), the shortest legal lengths alone, and the shapes that cross the 64-channel
    tile in ci and co."""
    lib, dev = backend(kind)
    c = _case(k, stride, Cin, Cout, T, db=db)
    dW, dbv, _ = _run(lib, dev, c)
    _check(c, dW, dbv, kind)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k,stride,T", [(5, 2, EDGES + [3]), (8, 1, [65])])
def test_red_zones(kind, k, stride, T):
    """2. Guard bands around x, dy, dW, db and the workspace are intact after the call (split and unsplit); the NaN-filled outputs are
    fully written; operands in NaN surroundings give a clean result."""
    lib, dev = backend(kind)
    c = _case(k, stride, 40, 48, T, xpad=(0, 0), ypad=(0, 0))
    n = lib.avc_conv1d_wgrad_ragged_ws_floats(len(T), _ints(T), 40, 48, k, stride)
    gW, gb, gws = GuardedOutput((48, 40, k), device=dev), GuardedOutput(48, device=dev), GuardedOutput(n, device=dev)
    dW, db, _ = _run(lib, dev, c, x=guarded_input(c["x"], device=dev), dy=guarded_input(c["dy"], device=dev), dW=gW.view, db=gb.view, ws=gws.view)
    _check(c, dW, db, kind)
    for g, name in ((gW, "dW"), (gb, "db"), (gws, "workspace")):
        g.assert_intact(name)


@pytest.mark.parametrize("kind", KINDS)
def test_two_calls_give_identical_bits(kind):
    """3. No atomics, a fixed order: a second call into fresh NaN-filled buffers repeats every bit."""
    lib, dev = backend(kind)
    c = _case(5, 2, 40, 48, EDGES + [17])
    a = _run(lib, dev, c)
    b = _run(lib, dev, c)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k,stride,B,T", [(5, 1, 3, 64), (5, 2, 3, 65), (4, 1, 2, 33), (1, 1, 4, 40)])
def test_equal_lengths_match_the_uniform_weight_gradient(kind, k, stride, B, T):
    """4. With equal lengths the packed layout is a contiguous [B, C, T] tensor: the result matches avc_conv1d_wgrad on the same data within
    1e-5 rel-L2 (not bit-equal: the K order differs)."""
    lib, dev = backend(kind)
    Cin, Cout = 40, 48
    c = _case(k, stride, Cin, Cout, [T] * B, xpad=(0, 0), ypad=(0, 0))
    dW, db, _ = _run(lib, dev, c)
    To = -(-T // stride)
    x, dy = c["x"].view(B, Cin, T).to(dev), c["dy"].view(B, Cout, To).to(dev)
    ws = torch.full((lib.avc_conv1d_wgrad_ws_floats(B, Cin, Cout, To, k),), float("nan"), device=dev)
    uW, ub = torch.full((Cout, Cin, k), float("nan"), device=dev), torch.full((Cout,), float("nan"), device=dev)
    assert lib.avc_conv1d_wgrad(P(x), x.stride(0), x.stride(1), 1, P(dy), dy.stride(0), dy.stride(1), 1, 1, B, Cin, Cout, T, To, k, stride,
                                P(uW), P(ub), P(ws), None) == 0
    ew, eb = rel(dW.cpu(), uW.cpu()), rel(db.cpu(), ub.cpu())
    print(f"[{kind}] k={k} s={stride} B={B} T={T}: ragged vs uniform dW {ew:.3e} db {eb:.3e}")
    assert ew <= 1e-5 and eb <= 1e-5


@pytest.mark.parametrize("kind", KINDS)
def test_refusals(kind):
    """A sample not longer than its left pad is the reference's padding error (-6); bad arguments are -1."""
    lib, dev = backend(kind)
    assert lib.avc_conv1d_wgrad_ragged_ws_floats(2, _ints([40, 2]), 16, 32, 5, 1) == -1
    buf = torch.zeros(64, device=dev)
    args = lambda T, k, s, Cin=16: (P(buf), 16, 0, P(buf), 32, 0, len(T), _ints(T), Cin, 32, k, s, P(buf), None, P(buf), None)   # noqa: E731
    assert lib.avc_conv1d_wgrad_ragged(*args([40, 2], 5, 1)) == -6
    assert lib.avc_conv1d_wgrad_ragged(*args([40], 9, 1)) == -1
    assert lib.avc_conv1d_wgrad_ragged(*args([40], 5, 3)) == -1
    assert lib.avc_conv1d_wgrad_ragged(*args([40], 5, 1, Cin=17)) == -1   # more channels than a block has
