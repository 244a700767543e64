"""Whole, part and ragged plans inside red zones (tests/redzone.py).

Every pass runs twice on the same backend: once in plain buffers, as tests/test_engine.py and its siblings run it (they pin the values
to the oracle; the inputs have the strides of the second run, so that every launcher picks the same kernel instance), and once with
the workspace and the flat gradient buffer inside sentinel red zones, the flat parameter buffer inside NaN red zones with NaN also in
the alignment padding between its tensors, every input in NaN red zones and x as the collate view
(strides (T*M, 1, M)).  The same kernels run on the same values, so every named result must be BIT-identical between the two runs;
every red zone must be intact; the gradients must be finite over every avc_plan_param_info range; and every float of `grads` that the
plan does not own -- the other networks' ranges of a part plan and ALL alignment padding -- must still hold the sentinel the buffer was
pre-filled with (the engine writes tensors only: no pass zeroes or touches the padding)."""
import pytest
import torch

from adaptive_voice_conversion_amd import _lib
from adaptive_voice_conversion_amd.engine import Plan, RaggedPlan
from oracle import avc_oracle as O
from tests.emu_util import backend
from tests.redzone import SENTINEL, GuardedOutput, guarded_input
from tests.test_engine import flat_params, get_cfg

GPU = pytest.mark.gpu
BOTH = ["emu", pytest.param("gpu", marks=GPU)]


class Layout:
    """the buffers of one run: plain (guard = False) or inside red zones"""

    def __init__(self, plan, sd, dev, guard):
        self.plan, self.dev, self.guard, self.outs = plan, dev, guard, []
        if guard:
            flat = torch.full((plan.param_floats,), float("nan"))      # NaN also in the alignment padding between the tensors
            for (off, n, shape), (k, v) in zip(plan.param_info, sd.items()):
                assert n == v.numel() and tuple(shape) == tuple(v.shape), k
                flat[off:off + n] = v.reshape(-1)
            self.params = guarded_input(flat, device=dev)
            self.ws = self.out((plan.workspace_floats,))
        else:
            self.params = flat_params(plan, sd, dev)
            self.ws = torch.full((plan.workspace_floats,), float("nan"), device=dev)
        self.grads = None

    def out(self, shape, init=None):
        self.outs.append(GuardedOutput(shape, device=self.dev, init=init))
        return self.outs[-1].view

    def inp(self, t, gap=0, collate=False):
        if t is None:
            return None
        if not self.guard:
            # the SAME strides as in the guarded run, in an ordinary tensor: several launchers choose their kernel instance by the strides
            # (avc_launch_loss sums four frames per thread only when x has unit time stride; the weight gradient stages 16-byte rows only
            # when the row strides are multiples of four), and another instance sums in another order
            if collate:
                return t.transpose(1, 2).contiguous().to(self.dev).transpose(1, 2)
            if gap:
                wide = torch.zeros(tuple(t.shape[:-1]) + (t.shape[-1] + gap,), dtype=t.dtype)
                wide[..., :t.shape[-1]] = t
                return wide.to(self.dev)[..., :t.shape[-1]]
            return t.to(self.dev)
        if collate:     # [B, M, T] handed over as the transposed view of a [B, T, M] tensor
            return guarded_input(t.transpose(1, 2).contiguous(), gap, self.dev).transpose(1, 2)
        return guarded_input(t, gap, self.dev)

    def make_grads(self):
        n = self.plan.param_floats
        if self.guard:
            self.grads = self.out((n,), init=torch.full((n,), SENTINEL, dtype=torch.int32).view(torch.float32))
        else:
            self.grads = torch.full((n,), float("nan"), device=self.dev)
        return self.grads

    def check(self, what, owned=None):
        """red zones intact; gradients finite over the owned tensors; every other float of grads still the sentinel"""
        for i, g in enumerate(self.outs):
            g.assert_intact(f"({what}: guarded buffer #{i} of {g.shape[0]} floats; #0 is the workspace)")
        if self.grads is None:
            return
        plan, g = self.plan, self.grads.cpu()
        mine = torch.zeros(plan.param_floats, dtype=torch.bool)
        lo, hi = owned if owned is not None else (0, plan.param_floats)
        for o, k, _ in plan.param_info:
            if lo <= o < hi:
                mine[o:o + k] = True
        assert torch.isfinite(g[mine]).all(), f"{what}: non-finite gradients"
        if self.guard:
            other = g.view(torch.int32)[~mine]
            bad = (other != SENTINEL).nonzero()
            assert bad.numel() == 0, (f"{what}: {bad.numel()} floats of grads outside the plan's tensors were written, first at float "
                                      f"{int((~mine).nonzero()[bad[0, 0]].item())}")

    def untouched_behind(self, end, what):
        """The floats from `end` (one past a result) to the next 64-float boundary still hold the NaN the workspace was pre-filled with.
        Every workspace region starts on a 64-float boundary (avc_plan::alloc, csrc/engine.hip), and the C ABI names only some regions,
        so this allocation padding is all of the workspace behind a result that is known to belong to nobody: a store one element
        past the result's last row lands exactly there.  Returns the number of floats checked."""
        hi = min((end + 63) // 64 * 64, self.plan.workspace_floats)
        bits = self.ws[end:hi].cpu().view(torch.int32)
        bad = (bits != 0x7FC00000).nonzero()
        assert bad.numel() == 0, f"{what}: {bad.numel()} float(s) behind the result were written, first at +{int(bad[0, 0])} (bits 0x{int(bits[bad[0, 0]]) & 0xFFFFFFFF:08X})"
        return hi - end

    def named(self, names):
        """{name: bits} of workspace regions (name -> shape)"""
        return {k: self.plan.view(self.ws, k, shp).cpu().clone() for k, shp in names.items()}


def same_bits(plain, guarded, what):
    assert plain.keys() == guarded.keys()
    for k in plain:
        a, b = plain[k].contiguous().view(torch.int32), guarded[k].contiguous().view(torch.int32)
        assert torch.isfinite(plain[k]).all(), (what, k)
        assert torch.equal(a, b), f"{what}: {k} differs between the plain and the red-zone run ({int((a != b).sum())} of {a.numel()} floats)"


def grad_bits(lay, owned=None):
    g = lay.grads.cpu()
    lo, hi = owned if owned is not None else (0, lay.plan.param_floats)
    return {f"grad[{i}]": g[o:o + n].clone() for i, (o, n, _) in enumerate(lay.plan.param_info) if lo <= o < hi}


TRAIN = [
    # kind, config, B, T, mode, compute
    ("emu", "tiny_lrelu", 3, 40, "train", "fp32"), ("emu", "tiny_lrelu", 3, 40, "ig_train", "fp32"),
    ("emu", "tiny", 2, 32, "train", "fp32"), ("emu", "tiny", 2, 32, "ig_train", "fp32"),
    ("emu", "tiny", 2, 32, "train", "bf16s"), ("emu", "tiny", 2, 32, "train", "fp32x3"),
    pytest.param("gpu", "tiny_lrelu", 3, 40, "train", "fp32", marks=GPU), pytest.param("gpu", "tiny_lrelu", 3, 40, "ig_train", "fp32", marks=GPU),
    pytest.param("gpu", "tiny", 2, 32, "train", "fp32", marks=GPU), pytest.param("gpu", "tiny", 2, 32, "ig_train", "fp32", marks=GPU),
    pytest.param("gpu", "tiny", 2, 32, "train", "bf16s", marks=GPU), pytest.param("gpu", "tiny", 2, 32, "train", "fp32x3", marks=GPU),
    pytest.param("gpu", "m80", 2, 40, "train", "fp32", marks=GPU), pytest.param("gpu", "m80", 2, 40, "ig_train", "fp32", marks=GPU),
]


@pytest.mark.parametrize("kind,cfgname,B,T,mode,compute", TRAIN)
def test_training_plan_in_red_zones(kind, cfgname, B, T, mode, compute):
    """forward + avc_loss + avc_backward.  With AVC_PLAN_INPUT_GRADS ("ig_train") the speaker encoder reads an x_cond of its own, so that
    both ws["d_x"] and ws["d_x_cond"] are produced."""
    lib, dev = backend(kind)
    cfg = get_cfg(cfgname)
    sd = O.make_state_dict(cfg, 4)
    x, eps = O.make_inputs(cfg, B, T, 4)
    xc = O.make_inputs(cfg, B, T, 9)[0] if mode == "ig_train" else None
    plan = Plan(cfg, B, T, lib=lib, mode=mode, compute_dtype=compute, tuning={"conv_x3": 2} if compute == "fp32x3" else None)
    M, Cz = cfg["Decoder"]["c_out"], cfg["ContentEncoder"]["c_out"]
    names = {"muls": (B, 2 * Cz, plan.latent_len), "emb": (B, cfg["SpeakerEncoder"]["c_out"]), "dec": (B, M, plan.out_len), "losses": (2,)}
    if mode == "ig_train":
        names.update({"d_x": (B, M, T), "d_x_cond": (B, M, T)})
    res = []
    for guard in (False, True):
        lay = Layout(plan, sd, dev, guard)
        xd, xcd, ed = lay.inp(x, collate=True), lay.inp(xc, collate=True), lay.inp(eps)
        plan.forward(lay.params, xd, xcd, ed, lay.ws)
        plan.loss(xd, cfg["lambda"]["lambda_rec"], lay.ws)
        plan.backward(lay.params, xd, xcd, ed, lay.make_grads(), lay.ws, lambda_kl=1.0)
        lay.check(f"{cfgname} B={B} T={T} {mode} {compute}")
        res.append({**lay.named(names), **grad_bits(lay)})
    same_bits(res[0], res[1], f"{cfgname} B={B} T={T} {mode} {compute}")


@pytest.mark.parametrize("kind,cfgname,Ts,Tc", [("emu", "tiny", 37, 19), pytest.param("gpu", "tiny", 37, 19, marks=GPU),
                                                pytest.param("gpu", "m80", 37, 19, marks=GPU)])
def test_inference_plan_in_red_zones(kind, cfgname, Ts, Tc):
    lib, dev = backend(kind)
    cfg = get_cfg(cfgname)
    sd = O.make_state_dict(cfg, 7)
    x, xc = O.make_inputs(cfg, 1, Ts, 7)[0], O.make_inputs(cfg, 1, Tc, 14)[0]
    plan = Plan(cfg, 1, Ts, Tc, lib=lib, mode="inference")
    names = {"muls": (1, 2 * cfg["ContentEncoder"]["c_out"], plan.latent_len), "emb": (1, cfg["SpeakerEncoder"]["c_out"]),
             "dec": (1, cfg["Decoder"]["c_out"], plan.out_len)}
    res = []
    for guard in (False, True):
        lay = Layout(plan, sd, dev, guard)
        plan.forward(lay.params, lay.inp(x, collate=True), lay.inp(xc, collate=True), None, lay.ws)
        lay.check(f"inference T={Ts} T_cond={Tc}")
        res.append(lay.named(names))
    same_bits(res[0], res[1], "inference")


@pytest.mark.parametrize("kind", BOTH)
@pytest.mark.parametrize("mode,part,zgap", [("speaker_train", _lib.GRADS_SPEAKER, 0), ("content_train", _lib.GRADS_CONTENT, 0),
                                            ("decoder_train", _lib.GRADS_DECODER, 4), ("decoder_train", _lib.GRADS_DECODER, 3)])
def test_part_plan_in_red_zones(kind, mode, part, zgap):
    """AVC_PLAN_PART_GRADS plans: the backward writes exactly its branch's avc_plan_param_range of grads, nothing else (include/avc_hip.h).
    The decoder reads z through a strided view (zgap 4: aligned row stride, the 16-byte staging of the weight gradient stays on; zgap 3:
    odd row stride) and ONE embedding for all samples (seb = 0)."""
    lib, dev = backend(kind)
    cfg = O.tiny_config()
    B, T = 2, 32
    Tb = O.latent_len(cfg, T)
    sd = O.make_state_dict(cfg, 1)
    x = O.make_inputs(cfg, B, T, 1)[0]
    g = torch.Generator().manual_seed(1)
    Cz, Ce, M = cfg["ContentEncoder"]["c_out"], cfg["SpeakerEncoder"]["c_out"], cfg["Decoder"]["c_out"]
    z, emb1 = torch.randn(B, Cz, Tb, generator=g), torch.randn(1, Ce, generator=g)
    plan = Plan(cfg, B, Tb if mode == "decoder_train" else T, lib=lib, mode=mode)
    d_dec, d_muls, d_emb = torch.randn(B, M, plan.out_len, generator=g), torch.randn(B, 2 * Cz, Tb, generator=g), torch.randn(B, Ce, generator=g)
    off, n = plan.param_range(part)
    res = []
    for guard in (False, True):
        lay = Layout(plan, sd, dev, guard)
        if mode == "decoder_train":
            zd, ed = lay.inp(z, gap=zgap), lay.inp(emb1).expand(B, -1)
            plan.decoder_forward(lay.params, zd, ed, lay.ws)
            plan.decoder_backward(lay.params, zd, ed, lay.make_grads(), lay.ws, d_dec=lay.inp(d_dec))
            names = {"dec": (B, M, plan.out_len), "d_z": (B, Cz, Tb), "d_emb": (B, Ce)}
        elif mode == "content_train":
            xd = lay.inp(x, collate=True)
            plan.forward(lay.params, xd, None, None, lay.ws)
            plan.backward(lay.params, xd, None, None, lay.make_grads(), lay.ws, d_muls=lay.inp(d_muls), lambda_kl=1.0)
            names = {"muls": (B, 2 * Cz, Tb)}
        else:
            xd = lay.inp(x, collate=True)
            plan.forward(lay.params, xd, None, None, lay.ws)
            plan.backward(lay.params, xd, None, None, lay.make_grads(), lay.ws, d_emb=lay.inp(d_emb))
            names = {"emb": (B, Ce)}
        lay.check(mode, owned=(off, off + n))
        res.append({**lay.named(names), **grad_bits(lay, (off, off + n))})
    same_bits(res[0], res[1], mode)


RT, RTC = [17, 64, 65, 31], [65, 17, 40, 64]


def _ragged_inputs(cfg, lens, seed):
    return torch.cat([O.make_inputs(cfg, 1, t, seed + i)[0][0].t().contiguous() for i, t in enumerate(lens)])      # [sum T][M]


@pytest.mark.parametrize("kind", BOTH)
def test_ragged_whole_plan_in_red_zones(kind):
    """The outputs of avc_plan_ragged_out tile ws["dec"] exactly: utterance b is the [M][out_len[b]] block at out_off[b], the blocks follow
    one another without overlap or hole from the start of "dec", and nothing behind the last block is written.  With these lengths dec
    ends on a 64-float boundary, so there is no allocation padding to inspect: what follows it to the end of the workspace is the
    plan's table upload (avc_plan_create_ragged_ex allocates rag_tab last, right behind dec; the ABI does not name it).  Those tables
    are a function of the plan alone, so after two passes over DIFFERENT inputs the workspace behind dec must hold the same bits: a
    store past the last output would leave input-dependent values there."""
    lib, dev = backend(kind)
    cfg = O.tiny_config()
    sd = O.make_state_dict(cfg, 3)
    x, xc = _ragged_inputs(cfg, RT, 20), _ragged_inputs(cfg, RTC, 40)
    plan = RaggedPlan(cfg, RT, RTC, lib=lib)
    M = plan.n_mels
    at = plan.buffer("dec")
    for o, n in sorted(zip(plan.out_off, plan.out_len)):
        assert o == at, "the ragged outputs do not tile dec"
        at += M * n
    res, tails = [], []
    for guard in (False, True):
        lay = Layout(plan, sd, dev, guard)
        plan.forward(lay.params, lay.inp(x), lay.inp(xc), lay.ws)
        lay.check("ragged whole plan")
        lay.untouched_behind(at, "ragged whole plan, behind the last output of dec")
        tails.append(lay.ws[at:].cpu().view(torch.int32).clone())
        res.append({**{f"dec[{b}]": o.cpu().clone() for b, o in enumerate(plan.outputs(lay.ws))}, "emb": plan.emb(lay.ws).cpu().clone()})
    same_bits(res[0], res[1], "ragged whole plan")
    lay = Layout(plan, sd, dev, True)
    plan.forward(lay.params, lay.inp(_ragged_inputs(cfg, RT, 60)), lay.inp(_ragged_inputs(cfg, RTC, 80)), lay.ws)
    other = torch.cat([o.cpu().reshape(-1) for o in plan.outputs(lay.ws)])
    assert not torch.equal(other, torch.cat([res[1][f"dec[{b}]"].reshape(-1) for b in range(len(RT))]))       # really other values
    tails.append(lay.ws[at:].cpu().view(torch.int32).clone())
    assert tails[0].numel() > 0 and torch.equal(tails[0], tails[1]) and torch.equal(tails[1], tails[2]), \
        "the workspace behind the last ragged output depends on the inputs: something was stored past dec"


@pytest.mark.parametrize("kind", BOTH)
def test_ragged_part_plans_in_red_zones(kind):
    """SPEAKER_ONLY, EMB_INPUT with one embedding for all utterances (seb = 0), and SPEAKER_ONLY | INPUT_GRADS with avc_backward_ragged
    reading d_emb through a column view (element stride 2, NaN in the columns between); d_x_cond is exactly [sum T_cond][M]."""
    lib, dev = backend(kind)
    cfg = O.tiny_config()
    sd = O.make_state_dict(cfg, 3)
    x, xc = _ragged_inputs(cfg, RT, 20), _ragged_inputs(cfg, RTC, 40)
    B, g = len(RT), torch.Generator().manual_seed(5)
    spk = RaggedPlan(cfg, None, RTC, lib=lib, mode="speaker")
    ig = RaggedPlan(cfg, None, RTC, lib=lib, mode="speaker", input_grads=True)
    embp = RaggedPlan(cfg, RT, None, lib=lib, mode="emb")
    emb1 = torch.randn(1, spk.c_emb, generator=g)
    wide = torch.full((B, 2 * spk.c_emb), float("nan"))
    wide[:, ::2] = torch.randn(B, spk.c_emb, generator=g)
    res = {"spk": [], "ig": [], "emb": []}
    for guard in (False, True):
        lay = Layout(spk, sd, dev, guard)
        spk.forward(lay.params, None, lay.inp(xc), lay.ws)
        lay.check("ragged speaker plan")
        res["spk"].append({"emb": spk.emb(lay.ws).cpu().clone()})
        lay = Layout(ig, sd, dev, guard)
        xcd = lay.inp(xc)
        ig.forward(lay.params, None, xcd, lay.ws)
        ig.backward(lay.params, xcd, lay.inp(wide)[:, ::2], lay.ws)
        lay.check("ragged speaker plan with input gradients")
        d = ig.d_x_cond(lay.ws)
        end = ig.buffer("d_x_cond") + sum(RTC) * ig.n_mels          # d_x_cond is exactly [sum T_cond][M]: nothing behind it is written
        assert end % 64 != 0 and lay.untouched_behind(end, "ragged input gradients, behind d_x_cond") > 0
        res["ig"].append({"emb": ig.emb(lay.ws).cpu().clone(), "d_x_cond": d.cpu().clone()})
        lay = Layout(embp, sd, dev, guard)
        embp.forward_emb(lay.params, lay.inp(x), lay.inp(emb1).expand(B, -1), lay.ws)
        lay.check("ragged emb-input plan")
        last = max(zip(embp.out_off, embp.out_len))
        lay.untouched_behind(last[0] + embp.n_mels * last[1], "ragged emb-input plan, behind the last output of dec")
        res["emb"].append({f"dec[{b}]": o.cpu().clone() for b, o in enumerate(embp.outputs(lay.ws))})
    for k, (a, b) in res.items():
        same_bits(a, b, f"ragged {k} plan")
