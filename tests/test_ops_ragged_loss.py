"""Op-level tests of the loss side of a ragged training step (csrc/ragged_loss.hip): avc_reparam_ragged, avc_loss_ragged,
avc_latent_bwd_ragged on packed rows, no plan.  Every input sits in NaN red zones, every output / scratch buffer in sentinel red zones
(tests/redzone.py), like tests/test_redzone_ops.py.

Shapes: utterance lengths T = [1, 7, 8, 63, 64, 65, 130] with output blocks T'' = 8 ceil(T / 8) -- the empty and the full (7-frame) crop
tail, a one-frame utterance, both sides of the 64-frame tile edge, three tiles -- and latents Tz = ceil(T / 8); M in {16 (the tiny
config's), 80, 512 (three lengths)}, c in {32 (tiny), 128}.

Bars: d_dec BITWISE against where(t < T_j, sign(dec - x) * float32(lambda_rec / n_rec), 0) with no NaN left (every element is written);
the two losses against an fp64 evaluation at rtol 1e-4 (the project's forward tolerance; fp32 block sums over at most ~1e5 terms are far
inside it); z and d_muls per element against fp64 at atol 2e-5 / rtol 1e-4, and with eps = NULL bitwise against mu and against the
formulas evaluated one fp32 torch operation at a time; two calls give identical bits.

kind='emu': the CPU lane-level simulator; kind='gpu': gfx950."""
import ctypes

import pytest
import torch

from tests.emu_util import KINDS, P, backend
from tests.redzone import GuardedOutput, guarded_input

T_ALL = [1, 7, 8, 63, 64, 65, 130]
CASES = [(16, 32, T_ALL), (80, 128, T_ALL), (512, 32, [7, 65, 130])]
LAMBDA_REC, LAMBDA_KL = 10.0, 0.37


def _prefix(v):
    return [sum(v[:i]) for i in range(len(v))]


def _bits(t):
    return t.contiguous().view(torch.int32)


class _Case:
    """inputs of one (M, c, lengths) case on the CPU, and their guarded device copies"""

    def __init__(self, dev, M, c, T):
        g = torch.Generator().manual_seed(M * 1000 + c + len(T))
        self.dev, self.M, self.c, self.T, self.N = dev, M, c, list(T), len(T)
        self.Tpp = [8 * ((t + 7) // 8) for t in T]
        self.Tz = [(t + 7) // 8 for t in T]
        self.out_off = _prefix([M * t for t in self.Tpp])
        self.n_rec, self.n_kl = M * sum(T), c * sum(self.Tz)
        self.x = torch.randn(sum(T), M, generator=g)
        self.dec = torch.randn(M * sum(self.Tpp), generator=g)
        for j in range(self.N):   # a few exact ties: sign(0) = 0
            self.block(self.dec, j)[0, 0] = self.x[_prefix(T)[j], 0]
        self.muls = 0.5 * torch.randn(2 * self.n_kl, generator=g)
        self.eps = torch.randn(self.n_kl, generator=g)
        self.d_z = torch.randn(self.n_kl, generator=g)
        gi = lambda t: guarded_input(t, device=dev)
        i32 = lambda v: gi(torch.tensor(v, dtype=torch.int32))
        self.g_x, self.g_dec, self.g_muls, self.g_eps, self.g_dz = gi(self.x), gi(self.dec), gi(self.muls), gi(self.eps), gi(self.d_z)
        self.T_dev, self.xoff_dev, self.len_dev = i32(self.T), i32(_prefix(self.T)), i32(self.Tpp)
        self.Tz_dev, self.offz_dev = i32(self.Tz), i32(_prefix(self.Tz))
        self.off_dev = gi(torch.tensor(self.out_off, dtype=torch.int64).view(torch.int32)).view(torch.int64)   # (guarded as dwords)

    def block(self, flat, j):
        o = self.out_off[j]
        return flat[o:o + self.M * self.Tpp[j]].view(self.M, self.Tpp[j])

    def mu_ls(self, dtype=torch.float32):
        """(mu, ls) as flat tensors in the z / eps layout"""
        mu, ls, c = [], [], self.c
        for tz, oz in zip(self.Tz, _prefix(self.Tz)):
            b = self.muls[2 * c * oz:2 * c * (oz + tz)]
            mu.append(b[:c * tz])
            ls.append(b[c * tz:])
        return torch.cat(mu).to(dtype), torch.cat(ls).to(dtype)

    def as_muls(self, a, b):
        """flat (mu-like, ls-like) in the z layout -> the muls layout"""
        out, c = [], self.c
        for tz, oz in zip(self.Tz, _prefix(self.Tz)):
            out += [a[c * oz:c * (oz + tz)], b[c * oz:c * (oz + tz)]]
        return torch.cat(out)


def _exp32(t):
    """The fp32 exponential of the platform the kernel ran on, as an fp32 torch tensor: a bitwise comparison can only be made against the same
    exponential.  On the GPU that is torch's own device kernel.  On the CPU the simulated kernel calls libm's expf, and torch.exp is a
    vectorised exponential of its own whose last bit differs from libm's in about 1 % of the elements (measured: 23 of 2752), also where
    it is handed one element at a time -- so the CPU reference takes expf from libm; every other operation of the formula stays an fp32
    torch operation."""
    if t.is_cuda:
        return torch.exp(t)
    import ctypes.util
    libm = ctypes.CDLL(ctypes.util.find_library("m"))
    libm.expf.restype, libm.expf.argtypes = ctypes.c_float, [ctypes.c_float]
    return torch.tensor([libm.expf(v) for v in t.reshape(-1).tolist()], dtype=torch.float32).view(t.shape)


def _ids(cases):
    return [f"M{m}-c{c}-N{len(t)}" for m, c, t in cases]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("M,c,T", CASES, ids=_ids(CASES))
def test_loss_ragged(kind, M, c, T):
    lib, dev = backend(kind)
    k = _Case(dev, M, c, T)
    nws = lib.avc_loss_ragged_ws_floats(k.N, max(k.Tpp))
    assert nws == 2 * k.N * ((max(k.Tpp) + 63) // 64)

    def run():
        d_dec, losses, ws = GuardedOutput(k.dec.numel(), device=dev), GuardedOutput(2, device=dev), GuardedOutput(nws, device=dev)
        rc = lib.avc_loss_ragged(P(k.g_dec), P(k.len_dev), P(k.off_dev), P(k.g_x), P(k.T_dev), P(k.xoff_dev), k.N, M, max(k.Tpp), P(k.g_muls),
                                 P(k.Tz_dev), P(k.offz_dev), c, k.n_rec, k.n_kl, LAMBDA_REC, P(d_dec.view), P(losses.view), P(ws.view), None)
        assert rc == 0
        for gd, name in ((d_dec, "d_dec"), (losses, "losses"), (ws, "ws")):
            gd.assert_intact(f"(avc_loss_ragged M={M} c={c}, {name})")
        return d_dec.view.cpu(), losses.view.cpu(), ws.view.cpu()
    d_dec, losses, ws = run()
    assert not torch.isnan(d_dec).any(), "an element of d_dec was not written"
    assert not torch.isnan(ws).any(), "a partial sum was not written"
    scale = torch.tensor(LAMBDA_REC / k.n_rec, dtype=torch.float64).to(torch.float32)   # divided in double, rounded once
    ref = torch.zeros_like(k.dec)
    rec = 0.0
    for j, (t, xo) in enumerate(zip(k.T, _prefix(k.T))):
        d = k.block(k.dec, j)[:, :t] - k.x[xo:xo + t].t()
        k.block(ref, j)[:, :t] = torch.where(d > 0, scale, torch.where(d < 0, -scale, torch.zeros(())))
        rec += float((k.block(k.dec, j)[:, :t].double() - k.x[xo:xo + t].t().double()).abs().sum())
    assert torch.equal(_bits(d_dec), _bits(ref)), f"d_dec differs in {int((_bits(d_dec) != _bits(ref)).sum())} element(s)"
    mu, ls = k.mu_ls(torch.float64)
    want = torch.tensor([rec / k.n_rec, 0.5 * float((torch.exp(ls) + mu ** 2 - 1 - ls).mean())], dtype=torch.float64)
    err = ((losses.double() - want).abs() / want.abs()).tolist()
    print(f"[{kind} M={M} c={c} N={k.N}] loss_rec {losses[0]:.7f} (rel err {err[0]:.2e}), loss_kl {losses[1]:.7f} (rel err {err[1]:.2e})")
    assert max(err) <= 1e-4, (losses.tolist(), want.tolist())
    d2, l2, w2 = run()
    assert torch.equal(_bits(d2), _bits(d_dec)) and torch.equal(_bits(l2), _bits(losses)) and torch.equal(_bits(w2), _bits(ws))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("M,c,T", CASES, ids=_ids(CASES))
def test_reparam_ragged(kind, M, c, T):
    lib, dev = backend(kind)
    k = _Case(dev, M, c, T)

    def run(eps):
        z = GuardedOutput(k.n_kl, device=dev)
        assert lib.avc_reparam_ragged(P(k.g_muls), P(eps), k.N, P(k.Tz_dev), P(k.offz_dev), max(k.Tz), c, P(z.view), None) == 0
        z.assert_intact(f"(avc_reparam_ragged c={c} eps={'yes' if eps is not None else 'NULL'})")
        return z.view.cpu()
    z = run(k.g_eps)
    mu, ls = k.mu_ls(torch.float64)
    want = mu + torch.exp(ls / 2) * k.eps.double()
    print(f"[{kind} c={c} N={k.N}] z: max abs err {float((z.double() - want).abs().max()):.2e}")
    torch.testing.assert_close(z.double(), want, atol=2e-5, rtol=1e-4)
    assert torch.equal(_bits(run(k.g_eps)), _bits(z))
    z0 = run(None)
    assert torch.equal(_bits(z0), _bits(k.mu_ls()[0])), "eps = NULL: z is not mu"
    assert torch.equal(_bits(run(None)), _bits(z0))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("M,c,T", CASES, ids=_ids(CASES))
def test_latent_bwd_ragged(kind, M, c, T):
    lib, dev = backend(kind)
    k = _Case(dev, M, c, T)
    lk = LAMBDA_KL / k.n_kl

    def run(eps):
        d = GuardedOutput(2 * k.n_kl, device=dev)
        assert lib.avc_latent_bwd_ragged(P(k.g_muls), P(eps), P(k.g_dz), k.N, P(k.Tz_dev), P(k.offz_dev), max(k.Tz), c, lk, P(d.view), None) == 0
        d.assert_intact(f"(avc_latent_bwd_ragged c={c} eps={'yes' if eps is not None else 'NULL'})")
        return d.view.cpu()
    d = run(k.g_eps)
    assert not torch.isnan(d).any()
    lk32 = float(torch.tensor(lk, dtype=torch.float32))   # what the C ABI's float argument holds
    mu, ls = k.mu_ls(torch.float64)
    dz, eps = k.d_z.double(), k.eps.double()
    want = k.as_muls(lk32 * mu + dz, lk32 * 0.5 * (torch.exp(ls) - 1) + dz * eps * 0.5 * torch.exp(ls / 2))
    print(f"[{kind} c={c} N={k.N}] d_muls: max abs err {float((d.double() - want).abs().max()):.2e}")
    torch.testing.assert_close(d.double(), want, atol=2e-5, rtol=1e-4)
    assert torch.equal(_bits(run(k.g_eps)), _bits(d))
    # eps = NULL: the two formulas, one fp32 torch operation at a time on the kernel's device
    d0 = run(None)
    mu32, ls32 = (t.to(dev) for t in k.mu_ls())
    l32 = torch.tensor(lk, dtype=torch.float32, device=dev)
    want0 = k.as_muls((l32 * mu32 + k.d_z.to(dev)).cpu(), ((l32 * 0.5) * (_exp32(ls32) - 1.0)).cpu())
    assert torch.equal(_bits(d0), _bits(want0)), f"eps = NULL: d_muls differs in {int((_bits(d0) != _bits(want0)).sum())} element(s)"
    assert torch.equal(_bits(run(None)), _bits(d0))


@pytest.mark.parametrize("which", ["emu", "product"])
def test_bad_arguments_are_refused_before_any_launch(which):
    """-1 for a null argument or a bad count (host-side checks: no GPU needed)"""
    from adaptive_voice_conversion_amd import _lib
    lib = backend("emu")[0] if which == "emu" else _lib.load()
    one = ctypes.c_void_p(16)   # never dereferenced
    assert lib.avc_loss_ragged_ws_floats(0, 64) == -1 and lib.avc_loss_ragged_ws_floats(3, 0) == -1 and lib.avc_loss_ragged_ws_floats(70000, 64) == -1
    assert lib.avc_loss_ragged_ws_floats(3, 130) == 2 * 3 * 3
    assert lib.avc_reparam_ragged(None, one, 2, one, one, 4, 8, one, None) == -1
    assert lib.avc_reparam_ragged(one, one, 0, one, one, 4, 8, one, None) == -1
    assert lib.avc_reparam_ragged(one, one, 2, one, one, 0, 8, one, None) == -1
    assert lib.avc_reparam_ragged(one, one, 2, one, one, 4, 8, None, None) == -1
    assert lib.avc_latent_bwd_ragged(one, one, None, 2, one, one, 4, 8, 0.1, one, None) == -1
    assert lib.avc_latent_bwd_ragged(one, one, one, 2, one, one, 4, 0, 0.1, one, None) == -1
    ok = [one, one, one, one, one, one, 2, 80, 64, one, one, one, 8, 100, 100, 1.0, one, one, one, None]
    for i, bad in ((0, None), (2, None), (5, None), (6, 0), (7, 0), (8, 0), (9, None), (12, 0), (13, 0), (14, 0), (16, None), (17, None), (18, None)):
        args = list(ok)
        args[i] = bad
        assert lib.avc_loss_ragged(*args) == -1, i
