"""avc_linear_wgrad_strided (csrc/conv_wgrad_ragged.hip, the STRIDED one-sample job): a Linear's weight / bias gradient over N rows read
through element strides, dW[co][ci] = sum_n dy(n, co) x(n, ci), db[co] = sum_n dy(n, co), against fp64.

kind='emu': the CPU lane-level simulation of the same kernel; kind='gpu': the gfx950 library.  Shapes: N in {1, 2, 31, 32, 33, 65} sits
inside / at / one past the 32-row K-chunk; (Cin, Cout) in {(128, 256), (80, 100), (70, 64)} are whole 64 x 64 tiles, partial tiles on both
axes, and a partial ci tile beside a whole co tile.  x is read row-major [N][Cin] (channel stride 1: the staging loop runs along
channels), column-major [Cin][N] (row stride 1: along rows) and as ONE row with row stride 0 (an expanded single voice); dy is
frame-major [N][Cout] rows with a NaN gap behind every row, the way a layer's slice lies in the decoder's d(cond).  One more case than the
list above, N = 300 at (128, 256): ten chunks, the only one here that is split (two slots) and goes through the reduce launch.

Bar: rel-L2 <= 1e-5 per tensor against fp64, the figure tests/test_ops_wgrad_ragged.py uses for the packed op and derives there (fp32 MFMA
products, an fp32 chain along K <= 300 rows: sqrt(K) u = 1e-6).

At packed strides (x [Cin][N], dy [Cout][N], row stride 1) the job shares the packed kernel's walk -- same chunks of 32, same MFMA chain,
same slots -- so the result equals avc_conv1d_wgrad_ragged at B = 1, T = [N], KS = 1 BIT FOR BIT (test 3)."""
import ctypes

import pytest
import torch

from tests.emu_util import KINDS, P, backend
from tests.redzone import GuardedOutput, guarded_input
from tests.test_submodules import rel

BAR = 1e-5
NS = [1, 2, 31, 32, 33, 65]
SHAPES = [(128, 256), (80, 100), (70, 64)]
GAP = 24   # NaN floats behind every dy row (and every row-major x row)


def _operands(N, Cin, Cout, layout, dev, seed=0):
    """(x view, sxn, sxc, dy view, syn, syc, x [N, Cin] fp64, dy [N, Cout] fp64): every view inside NaN red zones"""
    g = torch.Generator().manual_seed(7 * N + Cin + Cout + seed)
    dy = torch.randn(N, Cout, generator=g)
    dyv = guarded_input(dy, gap=GAP, device=dev)
    if layout == "bcast":
        x1 = torch.randn(1, Cin, generator=g)
        xv, sxn, sxc, x = guarded_input(x1, device=dev), 0, 1, x1.expand(N, Cin)
    elif layout == "row":
        x = torch.randn(N, Cin, generator=g)
        xv = guarded_input(x, gap=GAP, device=dev)
        sxn, sxc = xv.stride(0), 1
    else:   # "col": [Cin][N], rows contiguous
        x = torch.randn(N, Cin, generator=g)
        xv = guarded_input(x.t().contiguous(), device=dev)
        sxn, sxc = 1, xv.stride(0)
    return xv, sxn, sxc, dyv, dyv.stride(0), 1, x.double(), dy.double()


def _run(lib, dev, N, Cin, Cout, xv, sxn, sxc, dyv, syn, syc, with_db=True):
    n = lib.avc_linear_wgrad_strided_ws_floats(N, Cin, Cout)
    assert n > 0
    gW, gb, gws = GuardedOutput((Cout, Cin), device=dev), GuardedOutput(Cout, device=dev), GuardedOutput(n, device=dev)
    rc = lib.avc_linear_wgrad_strided(P(xv), sxn, sxc, P(dyv), syn, syc, N, Cin, Cout, P(gW.view), P(gb.view) if with_db else None, P(gws.view),
                                      None)
    assert rc == 0, rc
    for gd, name in ((gW, "dW"), (gb, "db"), (gws, "workspace")):
        gd.assert_intact(name)
    return gW.view, gb.view


def _check(dW, db, x, dy, tag):
    rw, rb = dy.t() @ x, dy.sum(0)
    assert not torch.isnan(dW).any() and not torch.isnan(db).any(), tag
    ew, eb = rel(dW.cpu(), rw), rel(db.cpu(), rb)
    print(f"[{tag}] dW rel-L2 {ew:.3e}, db rel-L2 {eb:.3e}")
    assert ew <= BAR and eb <= BAR, (tag, ew, eb)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("layout", ["row", "col", "bcast"])
@pytest.mark.parametrize("Cin,Cout", SHAPES)
def test_against_fp64(kind, Cin, Cout, layout):
    """1. Every N of the list at every shape and x layout, dy frame-major; operands and outputs behind red zones (a read outside poisons the
    result, a write outside trips the sentinel); the NaN-filled outputs are fully written."""
    lib, dev = backend(kind)
    for N in NS + ([300] if (Cin, Cout) == SHAPES[0] else []):
        xv, sxn, sxc, dyv, syn, syc, x, dy = _operands(N, Cin, Cout, layout, dev)
        dW, db = _run(lib, dev, N, Cin, Cout, xv, sxn, sxc, dyv, syn, syc)
        _check(dW, db, x, dy, f"{kind} {layout} N={N} {Cin}->{Cout}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N", [33, 300])
def test_two_calls_give_identical_bits(kind, N):
    """2. No atomics, a fixed order: a second call into fresh NaN-filled buffers repeats every bit (unsplit and split); db may be NULL."""
    lib, dev = backend(kind)
    Cin, Cout = SHAPES[0]
    ops = _operands(N, Cin, Cout, "row", dev)
    a = _run(lib, dev, N, Cin, Cout, *ops[:6])
    b = _run(lib, dev, N, Cin, Cout, *ops[:6])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    c = _run(lib, dev, N, Cin, Cout, *ops[:6], with_db=False)
    assert torch.equal(a[0], c[0]) and torch.isnan(c[1]).all()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N", [1, 33, 65, 300])
@pytest.mark.parametrize("Cin,Cout", SHAPES[:2])
def test_packed_strides_equal_the_packed_op_bit_for_bit(kind, Cin, Cout, N):
    """3. x [Cin][N] and dy [Cout][N] with row stride 1: the shared walk -- equal bits with avc_conv1d_wgrad_ragged at B = 1, KS = 1."""
    lib, dev = backend(kind)
    g = torch.Generator().manual_seed(N + Cin)
    x, dy = torch.randn(Cin, N, generator=g).to(dev), torch.randn(Cout, N, generator=g).to(dev)
    dW, db = _run(lib, dev, N, Cin, Cout, x, 1, N, dy, 1, N)
    T = (ctypes.c_int * 1)(N)
    n = lib.avc_conv1d_wgrad_ragged_ws_floats(1, T, Cin, Cout, 1, 1)
    pW, pb = torch.full((Cout, Cin, 1), float("nan"), device=dev), torch.full((Cout,), float("nan"), device=dev)
    ws = torch.full((n,), float("nan"), device=dev)
    assert lib.avc_conv1d_wgrad_ragged(P(x), Cin, 0, P(dy), Cout, 0, 1, T, Cin, Cout, 1, 1, P(pW), P(pb), P(ws), None) == 0
    assert torch.equal(dW.contiguous().view(torch.int32), pW.view(Cout, Cin).view(torch.int32))
    assert torch.equal(db.contiguous().view(torch.int32), pb.view(torch.int32))


@pytest.mark.parametrize("kind", KINDS)
def test_refusals(kind):
    """Bad arguments are -1: a null operand, non-positive sizes, a negative stride, operands spanning 2^31 elements or more."""
    lib, dev = backend(kind)
    buf = torch.zeros(64, device=dev)
    p = P(buf)
    ok = dict(x=p, sxn=4, sxc=1, dy=p, syn=4, syc=1, N=2, Cin=4, Cout=4, dW=p, db=None, ws=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.avc_linear_wgrad_strided(a["x"], a["sxn"], a["sxc"], a["dy"], a["syn"], a["syc"], a["N"], a["Cin"], a["Cout"], a["dW"], a["db"],
                                            a["ws"], None)
    assert call() == 0
    for k in ("x", "dy", "dW", "ws"):
        assert call(**{k: None}) == -1, k
    for kw in (dict(N=0), dict(Cin=0), dict(Cout=0), dict(sxn=-1), dict(syc=-1), dict(sxn=1 << 31), dict(syn=1 << 30, N=3)):
        assert call(**kw) == -1, kw
    assert lib.avc_linear_wgrad_strided_ws_floats(0, 4, 4) == -1 and lib.avc_linear_wgrad_strided_ws_floats(2, 4, 4) > 0
