"""Drop-in ``AE`` module (reference surface: model.py:373-395) backed by libavc_hip.so.

What is kept identical to the reference: constructor signature ``AE(config)``,
sub-module / parameter names (the 166-key ``state_dict`` of SURVEY.md §8b),
registration order (so ``parameters()`` feeds torch optimizers in the same
order), default initialisation (same nn.Conv1d / nn.Linear constructors in the
same order => same tensors under the same ``torch.manual_seed``), and the
methods ``forward / inference / get_speaker_embeddings``.

What is different: no torch op computes anything.  All parameters alias ONE flat
fp32 buffer (and all gradients another) laid out as the C plan dictates, and
forward/backward are single calls into the gfx950 engine.  The three sub-modules
are callable with the reference's signatures (``speaker_encoder(x)``,
``content_encoder(x)``, ``decoder(z, cond)``); each runs a part plan of the engine
through its owning ``AE``.
"""
import weakref

import torch
import torch.nn as nn

from .engine import Plan, cfg_from_dict


def _bank_kernels(c):
    return list(range(c["bank_scale"], c["bank_size"] + 1, c["bank_scale"]))


class _ParamHolder(nn.Module):
    """A network of the reference: its parameter containers, and a ``forward`` that runs the engine's part plan of this network
    through the owning ``AE`` (the plans, workspaces and the flat parameter buffer are the AE's)."""

    def extra_repr(self):
        return "parameters only; compute runs in libavc_hip.so"

    def _owner(self):
        ref = self.__dict__.get("_ae_ref")   # a weakref, set by AE.__init__: NOT a registered sub-module (state_dict / parameters unchanged)
        ae = ref() if ref is not None else None
        if ae is None:
            raise RuntimeError(f"{type(self).__name__} computes through the AE that owns it (its parameters alias the AE's flat buffer); "
                               "construct it as part of AE(config)")
        return ae


class SpeakerEncoder(_ParamHolder):
    """Parameter layout of model.py:209-235."""

    def __init__(self, c_in, c_h, c_out, kernel_size, bank_size, bank_scale, c_bank, n_conv_blocks, n_dense_blocks,
                 subsample, act, dropout_rate):
        super().__init__()
        ks = range(bank_scale, bank_size + 1, bank_scale)
        self.conv_bank = nn.ModuleList(nn.Conv1d(c_in, c_bank, kernel_size=k) for k in ks)
        self.in_conv_layer = nn.Conv1d(c_bank * (bank_size // bank_scale) + c_in, c_h, kernel_size=1)
        self.first_conv_layers = nn.ModuleList(nn.Conv1d(c_h, c_h, kernel_size=kernel_size) for _ in range(n_conv_blocks))
        self.second_conv_layers = nn.ModuleList(
            nn.Conv1d(c_h, c_h, kernel_size=kernel_size, stride=s) for s, _ in zip(subsample, range(n_conv_blocks)))
        self.first_dense_layers = nn.ModuleList(nn.Linear(c_h, c_h) for _ in range(n_dense_blocks))
        self.second_dense_layers = nn.ModuleList(nn.Linear(c_h, c_h) for _ in range(n_dense_blocks))
        self.output_layer = nn.Linear(c_h, c_out)

    def forward(self, x):
        """model.py:265-277: x [B, M, T] -> emb [B, c_out]."""
        return self._owner()._speaker_forward(x)


class ContentEncoder(_ParamHolder):
    """Parameter layout of model.py:279-299."""

    def __init__(self, c_in, c_h, c_out, kernel_size, bank_size, bank_scale, c_bank, n_conv_blocks, subsample, act,
                 dropout_rate):
        super().__init__()
        ks = range(bank_scale, bank_size + 1, bank_scale)
        self.conv_bank = nn.ModuleList(nn.Conv1d(c_in, c_bank, kernel_size=k) for k in ks)
        self.in_conv_layer = nn.Conv1d(c_bank * (bank_size // bank_scale) + c_in, c_h, kernel_size=1)
        self.first_conv_layers = nn.ModuleList(nn.Conv1d(c_h, c_h, kernel_size=kernel_size) for _ in range(n_conv_blocks))
        self.second_conv_layers = nn.ModuleList(
            nn.Conv1d(c_h, c_h, kernel_size=kernel_size, stride=s) for s, _ in zip(subsample, range(n_conv_blocks)))
        self.mean_layer = nn.Conv1d(c_h, c_out, kernel_size=1)
        self.std_layer = nn.Conv1d(c_h, c_out, kernel_size=1)

    def forward(self, x):
        """model.py:301-323: x [B, M, T] -> (mu, log_sigma), [B, c_out, Tb] each."""
        return self._owner()._content_forward(x)


class Decoder(_ParamHolder):
    """Parameter layout of model.py:325-345 (sn=False only)."""

    def __init__(self, c_in, c_cond, c_h, c_out, kernel_size, n_conv_blocks, upsample, act, sn, dropout_rate):
        super().__init__()
        self.in_conv_layer = nn.Conv1d(c_in, c_h, kernel_size=1)
        self.first_conv_layers = nn.ModuleList(nn.Conv1d(c_h, c_h, kernel_size=kernel_size) for _ in range(n_conv_blocks))
        self.second_conv_layers = nn.ModuleList(
            nn.Conv1d(c_h, c_h * up, kernel_size=kernel_size) for _, up in zip(range(n_conv_blocks), upsample))
        self.conv_affine_layers = nn.ModuleList(nn.Linear(c_cond, c_h * 2) for _ in range(n_conv_blocks * 2))
        self.out_conv_layer = nn.Conv1d(c_h, c_out, kernel_size=1)

    def forward(self, z, cond):
        """model.py:347-371: z [B, c_in, Tb], cond [B, c_cond] -> dec [B, c_out, Tb * prod(upsample)]."""
        return self._owner()._decoder_forward(z, cond)


class _Token:
    """Liveness marker of one autograd forward: while it is alive and not yet consumed, the workspace it
    was run in holds activations a pending backward() needs."""
    __slots__ = ("done", "__weakref__")

    def __init__(self):
        self.done = False


class _Entry:
    """One cached (plan, workspace)."""
    __slots__ = ("plan", "ws", "pending")

    def __init__(self, plan, ws):
        self.plan, self.ws, self.pending = plan, ws, None

    def busy(self):
        t = self.pending() if self.pending is not None else None
        return t is not None and not t.done


class _PlanCache:
    """Bounded LRU of launch plans + workspaces keyed by (mode, B, T, T_cond, device).  An evicted plan is
    destroyed (avc_plan_destroy releases its helper streams / events) and its workspace goes back to
    torch's caching allocator -- real inference traffic sees a new (T, T') for almost every utterance."""

    def __init__(self, capacity):
        from collections import OrderedDict
        self.capacity = dict(capacity)
        self.d = {m: OrderedDict() for m in self.capacity}
        self.zombies = []   # evicted while a pending backward still needed them: closed as soon as that backward ran (or its graph died)

    def _retire(self, e):
        if e.busy():
            self.zombies.append(e)   # the plan (streams, events) and its workspace stay alive for the pending backward ...
        else:
            e.plan.close()
            e.ws = None

    def sweep(self):
        """... and are released here, on the next cache access after that backward consumed them."""
        live = []
        for e in self.zombies:
            if e.busy():
                live.append(e)
            else:
                e.plan.close()
                e.ws = None
        self.zombies = live

    def get(self, mode, key, factory):
        if self.zombies:
            self.sweep()
        lru = self.d[mode]
        hit = lru.get(key)
        if hit is None:
            hit = lru[key] = factory()
            while len(lru) > self.capacity[mode]:
                _, old = lru.popitem(last=False)
                self._retire(old)
        else:
            lru.move_to_end(key)
        return hit

    def clear(self):
        for lru in self.d.values():
            for e in lru.values():
                self._retire(e)
            lru.clear()
        self.sweep()

    def __len__(self):
        return sum(len(v) for v in self.d.values())


class _AEFunction(torch.autograd.Function):
    """Autograd seam for drop-in use with arbitrary torch losses/optimizers.

    The engine saves its activations in the plan's workspace.  Each autograd forward marks the workspace
    it ran in as pending until its backward() has consumed it; a second autograd forward of the same shape
    that arrives meanwhile (micro-batches, an extra evaluation pass with grad enabled) gets a private
    workspace instead of overwriting the saved activations.  no_grad / inference / embedding calls run in
    separate forward-only plans and never touch a training workspace.  When x requires grad the pass runs in a plan whose backward
    also computes x.grad (AVC_PLAN_INPUT_GRADS: both encoders' terms)."""

    @staticmethod
    def forward(ctx, ae, x, eps, *params):
        mode = "ig_train" if ctx.needs_input_grad[1] else "train"
        entry = ae._entry(mode, x.shape[0], x.shape[2], x.shape[2], x.device)
        plan, ws = entry.plan, entry.ws
        if entry.busy():
            ws = torch.zeros(plan.workspace_floats, dtype=torch.float32, device=x.device)   # private to this forward
        token = _Token()
        if ws is entry.ws:
            import weakref
            entry.pending = weakref.ref(token)
        plan.forward(ae._flat, x, None, eps, ws)
        ctx.ae, ctx.plan, ctx.ws, ctx.token = ae, plan, ws, token
        ctx.save_for_backward(x, eps)
        muls, emb, dec = ae._outputs(plan, ws)
        C = muls.shape[1] // 2
        return muls[:, :C].clone(), muls[:, C:].clone(), emb.clone(), dec.clone()

    @staticmethod
    def backward(ctx, d_mu, d_ls, d_emb, d_dec):
        ae, plan, ws = ctx.ae, ctx.plan, ctx.ws
        if ctx.token.done:
            raise RuntimeError("AE: backward through the same forward twice (the engine keeps one set of saved activations)")
        if plan.h is None:
            raise RuntimeError("AE: the launch plan of this forward was released (model moved / cache cleared) before backward()")
        x, eps = ctx.saved_tensors
        B = x.shape[0]
        C, Tb = ae._c_lat, plan.latent_len
        d_muls = torch.zeros(B, 2 * C, Tb, device=x.device, dtype=torch.float32)
        if d_mu is not None:
            d_muls[:, :C] = d_mu
        if d_ls is not None:
            d_muls[:, C:] = d_ls
        d_dec = (torch.zeros(B, ae._n_mels, plan.out_len, device=x.device) if d_dec is None else d_dec).contiguous().float()
        d_emb = None if d_emb is None else d_emb.contiguous().float()
        g = torch.empty_like(ae._flat)
        plan.backward(ae._flat, x, None, eps, g, ws, d_dec=d_dec, d_muls=d_muls, d_emb=d_emb, lambda_kl=0.0)
        ctx.token.done = True
        dx = plan.view(ws, "d_x", tuple(x.shape)).clone() if ctx.needs_input_grad[1] else None
        grads = tuple(g[off:off + n].view(shape) for off, n, shape in ae._layout)
        return (None, dx, None) + grads


class _InferenceFunction(torch.autograd.Function):
    """AE.inference(x, x_cond) (model.py:387-391) with autograd, for inputs that require grad (adversarial perturbations of the target
    utterance, saliency maps): a whole plan with AVC_PLAN_INPUT_GRADS, no reparameterisation (eps = None: z = mu).  Returns d(x),
    d(x_cond) and the parameters' gradients.  x_cond may be x itself: the engine then sums both encoders' terms into d(x)."""

    @staticmethod
    def forward(ctx, ae, x, x_cond, *params):
        B, T, Tc = x.shape[0], x.shape[2], x_cond.shape[2]
        entry = ae._entry("ig_train", B, T, Tc, x.device)
        plan, ws = entry.plan, entry.ws
        if entry.busy():
            ws = torch.zeros(plan.workspace_floats, dtype=torch.float32, device=x.device)   # private to this forward
        token = _Token()
        if ws is entry.ws:
            entry.pending = weakref.ref(token)
        same = x_cond is x   # one autograd input read by both encoders (x.detach() or another view of its memory is a separate input)
        plan.forward(ae._flat, x, None if same else x_cond, None, ws)
        ctx.ae, ctx.plan, ctx.ws, ctx.token, ctx.same = ae, plan, ws, token, same
        ctx.save_for_backward(x, x_cond)
        return ae._outputs(plan, ws)[2].clone()

    @staticmethod
    def backward(ctx, d_dec):
        _PartFunction._check(ctx)
        x, x_cond = ctx.saved_tensors
        ae, plan, ws = ctx.ae, ctx.plan, ctx.ws
        g = torch.empty_like(ae._flat)
        plan.backward(ae._flat, x, None if ctx.same else x_cond, None, g, ws, d_dec=d_dec.contiguous().float(), lambda_kl=0.0)
        ctx.token.done = True
        dx = plan.view(ws, "d_x", tuple(x.shape)).clone() if (ctx.needs_input_grad[1] or ctx.same) else None
        dxc = None if ctx.same else (plan.view(ws, "d_x_cond", tuple(x_cond.shape)).clone() if ctx.needs_input_grad[2] else None)
        grads = tuple(g[off:off + n].view(shape) for off, n, shape in ae._layout)
        return (None, dx, dxc) + grads


class _PartFunction(torch.autograd.Function):
    """Shared steps of the three sub-module seams (the pattern of _AEFunction): a part plan of the training flavour ("*_train") from the
    AE's plan cache, a private workspace when the cached one still holds a pending backward's activations, and the gradients of THIS
    network's parameters only (the part backward writes exactly that range of the flat gradient buffer)."""

    @staticmethod
    def _begin(ctx, ae, mode, B, T, device):
        return _PartFunction._attach(ctx, ae, ae._entry(mode, B, T, T, device), device)

    @staticmethod
    def _attach(ctx, ae, entry, device):
        plan, ws = entry.plan, entry.ws
        if entry.busy():
            ws = torch.zeros(plan.workspace_floats, dtype=torch.float32, device=device)   # private to this forward
        token = _Token()
        if ws is entry.ws:
            entry.pending = weakref.ref(token)
        ctx.ae, ctx.plan, ctx.ws, ctx.token = ae, plan, ws, token
        return plan, ws

    @staticmethod
    def _check(ctx):
        if ctx.token.done:
            raise RuntimeError("AE: backward through the same forward twice (the engine keeps one set of saved activations)")
        if ctx.plan.h is None:
            raise RuntimeError("AE: the launch plan of this forward was released (model moved / cache cleared) before backward()")

    @staticmethod
    def _grads(ctx, g, part):
        ctx.token.done = True
        lo, hi = ctx.ae._part_index[part]
        return tuple(g[off:off + n].view(shape) for off, n, shape in ctx.ae._layout[lo:hi])


class _SpeakerFunction(_PartFunction):
    """SpeakerEncoder.forward (model.py:265-277) with autograd; x gets its gradient when it requires one (a plan with
    AVC_PLAN_INPUT_GRADS)."""

    @staticmethod
    def forward(ctx, ae, x, *params):
        B, T = x.shape[0], x.shape[2]
        plan, ws = _PartFunction._begin(ctx, ae, "speaker_ig_train" if ctx.needs_input_grad[1] else "speaker_train", B, T, x.device)
        plan.forward(ae._flat, x, None, None, ws)
        ctx.save_for_backward(x)
        return plan.view(ws, "emb", (B, ae._c_emb)).clone()

    @staticmethod
    def backward(ctx, d_emb):
        _PartFunction._check(ctx)
        x, = ctx.saved_tensors
        g = torch.empty_like(ctx.ae._flat)
        ctx.plan.backward(ctx.ae._flat, x, None, None, g, ctx.ws, d_emb=d_emb.contiguous().float())
        dx = ctx.plan.view(ctx.ws, "d_x", tuple(x.shape)).clone() if ctx.needs_input_grad[1] else None
        return (None, dx) + _PartFunction._grads(ctx, g, "speaker")


class _RaggedFunction(_PartFunction):
    """Shared steps of the ragged functions with autograd with respect to their inputs (RaggedPlans with ``input_grads``): the function's
    inputs and outputs are PACKED tensors -- torch's own autograd carries their gradients through the concatenation, device moves and
    views to every leaf that requires grad.  Parameters are frozen: they get no gradient here (the sub-modules on uniform shapes have
    them)."""

    @staticmethod
    def _begin(ctx, ae, mode, T, Tc, device):
        return _PartFunction._attach(ctx, ae, ae._ragged_plan(mode, T, Tc)[1], device)

    @staticmethod
    def _finish(ctx):
        ctx.token.done = True


class _RaggedSpeakerFunction(_RaggedFunction):
    """``AE.get_speaker_embeddings_ragged`` (a "speaker" RaggedPlan with ``input_grads``): from the packed [sum T, M] tensor
    ``_ragged_rows`` builds from the utterances to the [B, c_emb] embeddings."""

    @staticmethod
    def forward(ctx, ae, xc, Tc):
        plan, ws = _RaggedFunction._begin(ctx, ae, "speaker_ig", (), Tc, xc.device)
        plan.forward(ae._flat, None, xc, ws)
        ctx.save_for_backward(xc)
        return plan.emb(ws).clone()

    @staticmethod
    def backward(ctx, d_emb):
        _PartFunction._check(ctx)
        xc, = ctx.saved_tensors
        if d_emb.dtype != torch.float32:
            d_emb = d_emb.float()
        ctx.plan.backward(ctx.ae._flat, xc, d_emb, ctx.ws)
        _RaggedFunction._finish(ctx)
        return None, ctx.plan.d_x_cond(ctx.ws).clone(), None


class _RaggedSpeakerParamFunction(_RaggedFunction):
    """``AE.speaker_encoder_ragged`` with live parameters (a "speaker_pg" RaggedPlan): the pattern of ``_SpeakerFunction`` on packed rows --
    the speaker encoder's parameters are inputs of the function, their gradients and the packed input gradient come from ONE ragged
    backward pass (``avc_backward_ragged_params``)."""

    @staticmethod
    def forward(ctx, ae, xc, Tc, *params):
        plan, ws = _RaggedFunction._begin(ctx, ae, "speaker_pg", (), Tc, xc.device)
        plan.forward(ae._flat, None, xc, ws)
        ctx.save_for_backward(xc)
        return plan.emb(ws).clone()

    @staticmethod
    def backward(ctx, d_emb):
        _PartFunction._check(ctx)
        xc, = ctx.saved_tensors
        if d_emb.dtype != torch.float32:
            d_emb = d_emb.float()
        g = torch.empty_like(ctx.ae._flat)
        ctx.plan.backward_params(ctx.ae._flat, xc, d_emb, g, ctx.ws)
        dxc = ctx.plan.d_x_cond(ctx.ws).clone() if ctx.needs_input_grad[1] else None
        return (None, dxc, None) + _PartFunction._grads(ctx, g, "speaker")


class _RaggedContentFunction(_RaggedFunction):
    """``AE.content_encoder_ragged`` (an "encode" RaggedPlan with ``input_grads``): from the packed [sum T, M] tensor to the packed
    latents -- block s is [2 c_lat][Tz_s], mu rows then log_sigma rows, the layout of ws["muls"].  The caller's per-utterance mu /
    log_sigma are views of that output, so torch's own autograd gathers their gradients into the packed d_muls the plan reads."""

    @staticmethod
    def forward(ctx, ae, x, T):
        plan, ws = _RaggedFunction._begin(ctx, ae, "encode_ig", T, (), x.device)
        plan.forward(ae._flat, x, None, ws)
        ctx.save_for_backward(x)
        o = plan.lat_off[0]
        return ws[o:o + 2 * plan.c_lat * sum(plan.lat_len)].clone()

    @staticmethod
    def backward(ctx, d_muls):
        _PartFunction._check(ctx)
        x, = ctx.saved_tensors
        ctx.plan.backward_content(ctx.ae._flat, x, d_muls.float().contiguous(), ctx.ws)
        _RaggedFunction._finish(ctx)
        return None, ctx.plan.d_x(ctx.ws).clone(), None


class _RaggedDecoderFunction(_RaggedFunction):
    """``AE.decoder_ragged`` (a "decode_ig" RaggedPlan): from the packed latents (block s = [c_lat][Tz_s]) and the [N, c_emb] embeddings
    (an expanded single voice included, whose rows torch's own autograd sums) to the packed [M][T''_j] blocks."""

    @staticmethod
    def forward(ctx, ae, z, e, Tz):
        plan, ws = _RaggedFunction._begin(ctx, ae, "decode_ig", Tz, (), z.device)
        plan.forward_latents(ae._flat, z, plan.c_lat, e, ws)
        ctx.save_for_backward(z, e)
        o = plan.out_off[0]
        return ws[o:o + plan.n_mels * sum(plan.out_len)].clone()

    @staticmethod
    def backward(ctx, d_dec):
        _PartFunction._check(ctx)
        z, e = ctx.saved_tensors
        plan, ws = ctx.plan, ctx.ws
        plan.backward_decoder(ctx.ae._flat, z, plan.c_lat, e, d_dec.float().contiguous(), ws)
        _RaggedFunction._finish(ctx)
        o = plan.buffer("d_z")
        return None, ws[o:o + plan.c_lat * sum(plan.T)].clone(), plan.d_emb(ws).clone(), None


class _RaggedContentParamFunction(_RaggedFunction):
    """``AE.content_encoder_ragged(param_grads=True)`` (an "encode_pg" RaggedPlan): ``_RaggedContentFunction`` with the content encoder's
    parameters as inputs of the function -- their gradients and the packed input gradient come from ONE ragged backward pass
    (``avc_content_backward_ragged_params``), the pattern of ``_RaggedSpeakerParamFunction``."""

    @staticmethod
    def forward(ctx, ae, x, T, *params):
        plan, ws = _RaggedFunction._begin(ctx, ae, "encode_pg", T, (), x.device)
        plan.forward(ae._flat, x, None, ws)
        ctx.save_for_backward(x)
        o = plan.lat_off[0]
        return ws[o:o + 2 * plan.c_lat * sum(plan.lat_len)].clone()

    @staticmethod
    def backward(ctx, d_muls):
        _PartFunction._check(ctx)
        x, = ctx.saved_tensors
        g = torch.empty_like(ctx.ae._flat)
        ctx.plan.backward_content_params(ctx.ae._flat, x, d_muls.float().contiguous(), g, ctx.ws)
        dx = ctx.plan.d_x(ctx.ws).clone() if ctx.needs_input_grad[1] else None
        return (None, dx, None) + _PartFunction._grads(ctx, g, "content")


class _RaggedDecoderParamFunction(_RaggedFunction):
    """``AE.decoder_ragged(param_grads=True)`` (a "decode_pg" RaggedPlan): ``_RaggedDecoderFunction`` with the decoder's parameters as inputs
    of the function; one ragged backward pass (``avc_decoder_backward_ragged_params``) gives their gradients, d(z) and d(emb)."""

    @staticmethod
    def forward(ctx, ae, z, e, Tz, *params):
        plan, ws = _RaggedFunction._begin(ctx, ae, "decode_pg", Tz, (), z.device)
        plan.forward_latents(ae._flat, z, plan.c_lat, e, ws)
        ctx.save_for_backward(z, e)
        o = plan.out_off[0]
        return ws[o:o + plan.n_mels * sum(plan.out_len)].clone()

    @staticmethod
    def backward(ctx, d_dec):
        _PartFunction._check(ctx)
        z, e = ctx.saved_tensors
        plan, ws = ctx.plan, ctx.ws
        g = torch.empty_like(ctx.ae._flat)
        plan.backward_decoder_params(ctx.ae._flat, z, plan.c_lat, e, d_dec.float().contiguous(), g, ws)
        o = plan.buffer("d_z")
        dz = ws[o:o + plan.c_lat * sum(plan.T)].clone() if ctx.needs_input_grad[1] else None
        de = plan.d_emb(ws).clone() if ctx.needs_input_grad[2] else None
        return (None, dz, de, None) + _PartFunction._grads(ctx, g, "decoder")


class _ContentFunction(_PartFunction):
    """ContentEncoder.forward (model.py:301-323) with autograd; x gets its gradient when it requires one (a plan with
    AVC_PLAN_INPUT_GRADS)."""

    @staticmethod
    def forward(ctx, ae, x, *params):
        B, T = x.shape[0], x.shape[2]
        plan, ws = _PartFunction._begin(ctx, ae, "content_ig_train" if ctx.needs_input_grad[1] else "content_train", B, T, x.device)
        plan.forward(ae._flat, x, None, None, ws)
        ctx.save_for_backward(x)
        muls = plan.view(ws, "muls", (B, 2 * ae._c_lat, plan.latent_len))
        return muls[:, :ae._c_lat].clone(), muls[:, ae._c_lat:].clone()

    @staticmethod
    def backward(ctx, d_mu, d_ls):
        _PartFunction._check(ctx)
        x, = ctx.saved_tensors
        ae, plan = ctx.ae, ctx.plan
        C = ae._c_lat
        d_muls = torch.zeros(x.shape[0], 2 * C, plan.latent_len, device=x.device, dtype=torch.float32)
        if d_mu is not None:
            d_muls[:, :C] = d_mu
        if d_ls is not None:
            d_muls[:, C:] = d_ls
        g = torch.empty_like(ae._flat)
        plan.backward(ae._flat, x, None, None, g, ctx.ws, d_muls=d_muls, lambda_kl=0.0)
        dx = plan.view(ctx.ws, "d_x", tuple(x.shape)).clone() if ctx.needs_input_grad[1] else None
        return (None, dx) + _PartFunction._grads(ctx, g, "content")


class _DecoderFunction(_PartFunction):
    """Decoder.forward(z, cond) (model.py:347-371) with autograd: gradients for z, cond and the decoder's parameters."""

    @staticmethod
    def forward(ctx, ae, z, cond, *params):
        plan, ws = _PartFunction._begin(ctx, ae, "decoder_train", z.shape[0], z.shape[2], z.device)
        plan.decoder_forward(ae._flat, z, cond, ws)
        ctx.save_for_backward(z, cond)   # (the engine reads them again in place: the in_conv's and the affine GEMM's weight gradients)
        return plan.view(ws, "dec", (z.shape[0], ae._n_mels, plan.out_len)).clone()

    @staticmethod
    def backward(ctx, d_dec):
        _PartFunction._check(ctx)
        z, cond = ctx.saved_tensors
        ae, plan, ws = ctx.ae, ctx.plan, ctx.ws
        B = z.shape[0]
        g = torch.empty_like(ae._flat)
        plan.decoder_backward(ae._flat, z, cond, g, ws, d_dec=d_dec.contiguous().float())
        dz = plan.view(ws, "d_z", (B, ae._c_lat, plan.latent_len)).clone() if ctx.needs_input_grad[1] else None
        dcond = plan.view(ws, "d_emb", (B, ae._c_emb)).clone() if ctx.needs_input_grad[2] else None
        return (None, dz, dcond) + _PartFunction._grads(ctx, g, "decoder")


class AE(nn.Module):
    """model.py:373-395."""

    def __init__(self, config, lib=None, compute_dtype=None, tuning=None):
        """``compute_dtype`` ("fp32" default | "bf16" (bf16 storage engine) | "bf16r" (fp32 storage, bf16 operands) | "fp32x3"; also read
        from ``config["compute_dtype"]``; engine.Plan documents the modes) is an
        extension over the reference: the precision of the conv / Linear matrix products (engine.Plan).
        ``tuning``: {avc_tuning field: value} captured by every plan of this module (A/B measurements, tests)."""
        super().__init__()
        self.config = config
        self._lib = lib
        self._tuning = dict(tuning or {})
        self.compute_dtype = compute_dtype or (config.get("compute_dtype") if isinstance(config, dict) else None) or "fp32"
        cfg_from_dict(config)  # validates (raises on sn / lrelu / dropout)
        self.speaker_encoder = SpeakerEncoder(**config["SpeakerEncoder"])
        self.content_encoder = ContentEncoder(**config["ContentEncoder"])
        self.decoder = Decoder(**config["Decoder"])
        # each network reaches this AE through a weak reference in its __dict__: not a registered sub-module, no reference cycle
        for m in (self.speaker_encoder, self.content_encoder, self.decoder):
            object.__setattr__(m, "_ae_ref", weakref.ref(self))
        self._n_mels = int(config["ContentEncoder"]["c_in"])
        self._c_lat = int(config["ContentEncoder"]["c_out"])
        self._c_emb = int(config["SpeakerEncoder"]["c_out"])
        # flat layout: state_dict order, every tensor 16-byte aligned (must equal the C plan's, checked in _plan)
        self._layout, off = [], 0
        for p in self.parameters():
            self._layout.append((off, p.numel(), tuple(p.shape)))
            off += (p.numel() + 3) // 4 * 4
        # [lo, hi) of each network's entries in _layout (registration order: speaker encoder, content encoder, decoder)
        n_spk, n_enc = len(list(self.speaker_encoder.parameters())), len(list(self.content_encoder.parameters()))
        self._part_index = {"speaker": (0, n_spk), "content": (n_spk, n_spk + n_enc), "decoder": (n_spk + n_enc, len(self._layout))}
        self._flat = torch.zeros(off, dtype=torch.float32)
        with torch.no_grad():
            for (o, n, _), p in zip(self._layout, self.parameters()):
                self._flat[o:o + n] = p.detach().reshape(-1)
        self._gflat = None
        self._bump = 0
        self._alias()
        # train: the regular batch + the short last batch of an epoch; inference / speaker: a few recent shapes
        self._plans = _PlanCache({"train": 2, "inference": 8, "speaker": 4,
                                  # sub-module calls (part plans): forward-only / with backward
                                  "content": 4, "decoder": 4, "speaker_train": 2, "content_train": 2, "decoder_train": 2,
                                  # ... and the plans whose backward also computes the inputs' gradients (inputs that require grad)
                                  "ig_train": 2, "speaker_ig_train": 2, "content_ig_train": 2})
        # (mode, lengths, device[, src_of]) -> (RaggedPlan, None | _Entry), a few most recent; mode: "pairs" | "speaker" | "emb" | "fanout" |
        # "encode" | "decode" | "speaker_ig" (the
        # speaker plan with input gradients; the key carries the flag, and only it has an _Entry: a workspace of its own)
        self._ragged = {}
        # how many of them (`ragged_plan_cache` in the config; set_ragged_plan_cache): a training loop over K length templates needs
        # 3 K grad plans to stay (Solver.train_ragged raises the bound), everything else lives with a few
        self._ragged_cap = max(1, int((config.get("ragged_plan_cache") if isinstance(config, dict) else None) or 4))
        self._ragged_ws = None   # the one workspace the forward-only plans share
        self.last_ragged_compute = None

    # ---- flat storage ------------------------------------------------------
    def _alias(self):
        self._bump = getattr(self, "_bump", 0) + 1   # the parameters may point at new storage: any "weights already packed" promise is void
        for (o, n, shape), p in zip(self._layout, self.parameters()):
            p.data = self._flat[o:o + n].view(shape)
            if self._gflat is not None:
                p.grad = self._gflat[o:o + n].view(shape)

    def _apply(self, fn, recurse=True):
        new = fn(self._flat)
        if new.dtype != torch.float32:
            raise NotImplementedError("the engine stores fp32 master parameters")
        self._flat = new.contiguous()
        if self._gflat is not None:
            self._gflat = fn(self._gflat).contiguous()
        self._alias()
        self._plans.clear()
        for plan, _ in getattr(self, "_ragged", {}).values():
            plan.close()
        self._ragged = {}
        self._ragged_ws = None
        return self

    def flat_parameters(self):
        return self._flat

    def weights_version(self):
        """Changes whenever PyTorch saw an in-place write to the parameters (flat buffer or any parameter view): what
        Solver.ae_step compares to decide whether the weight images it packed behind its last optimizer step are still current."""
        return (self._flat._version, self._bump, sum(p._version for p in self.parameters()))

    def weights_changed(self):
        """Tell the engine that the parameters were modified behind PyTorch's back (in-place through `.data`, a foreign kernel)."""
        self._bump += 1

    def flat_grads(self):
        if self._gflat is None or self._gflat.device != self._flat.device:
            self._gflat = torch.zeros_like(self._flat)
            self._alias()
        return self._gflat

    def load_state_dict(self, state_dict, strict=True, **kw):
        out = super().load_state_dict(state_dict, strict=strict, **kw)  # copies into the aliased views
        self.weights_changed()   # (the version counters see the copies too; this does not depend on it)
        return out

    # ---- plans ---------------------------------------------------------------
    def _entry(self, mode, B, T, Tc, device):
        key = (int(B), int(T), int(Tc), str(device))

        def make():
            plan = Plan(self.config, B, T, Tc, lib=self._lib, compute_dtype=self._compute_for(mode), mode=mode, device=device, tuning=self._tuning)
            if [(o, n) for o, n, _ in plan.param_info] != [(o, n) for o, n, _ in self._layout]:
                raise RuntimeError("flat parameter layout of the C plan differs from the module's")
            return _Entry(plan, torch.zeros(plan.workspace_floats, dtype=torch.float32, device=device))
        return self._plans.get(mode, key, make)

    def _compute_for(self, mode):
        """ONE rounding model per compute mode and use: under ``compute_dtype: bf16`` the TRAINING plans run the bf16 pair-storage engine
        (BASELINE configs[2]); every forward-only plan -- ``AE.inference``, ``get_speaker_embeddings``, no-grad forwards -- rounds the
        operands of the matrix products to bf16 on fp32 storage ("bf16r"), which is what the ragged plan of ``inference_ragged`` /
        ``Inferencer.convert_batch`` runs and what the uniform plan falls back to at lengths outside the pair kernels anyway: the same
        utterance converts to the same numbers (to fp32 summation order) whichever entry point it comes through.
        ``inference_compute_dtype`` in the config overrides it (e.g. "bf16s": pair storage for uniform inference batches, faster, its own
        rounding points)."""
        cd = str(self.compute_dtype).lower()
        if not (mode == "train" or mode.endswith("_train")) and cd in ("bf16", "bfloat16"):   # (sub-module part plans: "*_train" train)
            return (self.config.get("inference_compute_dtype") if isinstance(self.config, dict) else None) or "bf16r"
        return self.compute_dtype

    def _plan(self, B, T, Tc, device, mode="train"):
        e = self._entry(mode, B, T, Tc, device)
        return e.plan, e.ws

    def set_plan_cache_size(self, train=None, inference=None, speaker=None):
        """How many (shape, device) launch plans + workspaces each mode keeps (LRU)."""
        for k, v in (("train", train), ("inference", inference), ("speaker", speaker)):
            if v is not None:
                self._plans.capacity[k] = max(1, int(v))

    def set_ragged_plan_cache(self, n):
        """How many ragged plans of all modes (with the workspaces the grad plans own) are kept, most recently used last (the config's
        ``ragged_plan_cache``, default 4).  Takes effect when the next plan is created; a smaller bound evicts then."""
        self._ragged_cap = max(1, int(n))

    def _outputs(self, plan, ws):
        B = plan.B
        muls = plan.view(ws, "muls", (B, 2 * self._c_lat, plan.latent_len))
        emb = plan.view(ws, "emb", (B, self._c_emb))
        dec = plan.view(ws, "dec", (B, self._n_mels, plan.out_len))
        return muls, emb, dec

    def _check_device(self, x):
        if x.device != self._flat.device:
            raise RuntimeError(f"input on {x.device} but parameters on {self._flat.device}")

    @staticmethod
    def _prep(x):
        if x.dtype != torch.float32:
            x = x.float()
        return x

    # ---- reference surface ---------------------------------------------------
    def forward(self, x, eps=None):
        """model.py:380-385; ``eps`` may be injected for parity tests."""
        x = self._prep(x)
        self._check_device(x)
        B, T = x.shape[0], x.shape[2]
        grad = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters()))
        mode = ("ig_train" if x.requires_grad else "train") if grad else "inference"   # (the plan _AEFunction runs in)
        if eps is None:
            Tb = self._plan(B, T, T, x.device, mode)[0].latent_len
            eps = torch.randn(B, self._c_lat, Tb, device=x.device, dtype=torch.float32)
        eps = eps.contiguous()
        if grad:
            return _AEFunction.apply(self, x, eps, *self.parameters())
        plan, ws = self._plan(B, T, T, x.device, "inference")   # forward-only workspace: never a training one
        plan.forward(self._flat, x, None, eps, ws)
        muls, emb, dec = self._outputs(plan, ws)
        C = self._c_lat
        return muls[:, :C].clone(), muls[:, C:].clone(), emb.clone(), dec.clone()

    def inference(self, x, x_cond):
        """model.py:387-391: decoder(mu(x), speaker(x_cond)); lengths may differ."""
        x, x_cond = self._prep(x), self._prep(x_cond)
        self._check_device(x)
        if torch.is_grad_enabled() and (x.requires_grad or x_cond.requires_grad):
            self._check_device(x_cond)
            return _InferenceFunction.apply(self, x, x_cond, *self.parameters())
        plan, ws = self._plan(x.shape[0], x.shape[2], x_cond.shape[2], x.device, "inference")
        plan.forward(self._flat, x, x_cond, None, ws)
        return self._outputs(plan, ws)[2].clone()

    def _ragged_plan(self, mode, T, Tc, src_of=None):
        """(RaggedPlan, pooled workspace) for a tuple of lengths; a few most recent plans of all modes are kept.  modes "speaker_ig",
        "encode_ig", "decode_ig" (the speaker / content / decoder plan with input gradients) and "speaker_pg", "encode_pg", "decode_pg"
        (the plans whose backward also computes their network's parameter gradients) return (RaggedPlan, _Entry) instead: such a plan owns its workspace, which holds the saved
        activations between a forward and its backward and is never the pooled one.  ``src_of`` (a tuple; "fanout" / "decode" plans):
        the source of every output, part of the key."""
        from .engine import RaggedPlan
        dev = self._flat.device
        key = (mode, T, Tc, str(dev)) if src_of is None else (mode, T, Tc, str(dev), src_of)
        hit = self._ragged.get(key)
        if hit is None:
            # compute_dtype "bf16" -> "bf16r" here: the pair-STORAGE engine takes uniform shapes only; ragged plans round the operands of
            # the matrix products to bf16 on fp32 storage (engine.RaggedPlan).  The mode that ran is reported in `last_ragged_compute`.
            ig = mode in ("speaker_ig", "encode_ig", "decode_ig", "speaker_pg", "encode_pg", "decode_pg")
            plan = RaggedPlan(self.config, T, Tc, lib=self._lib, compute_dtype="bf16r" if str(self.compute_dtype).lower().startswith(("bf16", "bfloat16")) else "fp32", device=dev,
                              tuning=self._tuning, mode=mode[:-3] if (ig and mode not in ("decode_ig", "speaker_pg", "encode_pg", "decode_pg")) else mode,
                              input_grads=ig, src_of=src_of)
            if [(o, n) for o, n, _ in plan.param_info] != [(o, n) for o, n, _ in self._layout]:
                raise RuntimeError("flat parameter layout of the C plan differs from the module's")
            hit = self._ragged[key] = (plan, _Entry(plan, torch.zeros(plan.workspace_floats, dtype=torch.float32, device=dev)) if ig else None)
            while len(self._ragged) > self._ragged_cap:
                old = self._ragged.pop(next(iter(self._ragged)))
                if old[1] is None:   # (a grad plan may still be needed by a pending backward -- also one that ran in a private workspace, which
                    old[0].close()   # the entry does not track: it is never closed here, RaggedPlan.__del__ releases it once no graph holds it)
        else:
            self._ragged[key] = self._ragged.pop(key)   # most recently used last
        plan = hit[0]
        if hit[1] is not None:
            return plan, hit[1]
        # ONE pooled workspace for all ragged plans (real traffic almost never repeats a tuple of lengths: a fresh multi-hundred-MB
        # torch.zeros per call was most of the cold-path cost): every region a forward pass reads it has written before, in that pass
        ws = self._ragged_ws
        if ws is None or ws.device != dev or ws.numel() < plan.workspace_floats:
            ws = self._ragged_ws = torch.zeros(int(plan.workspace_floats * 1.25) + 1024, dtype=torch.float32, device=dev)
        self.last_ragged_compute = plan.compute_dtype
        return plan, ws

    def _ragged_rows(self, ts, name):
        dev = self._flat.device
        ts = list(ts)
        if not ts:
            raise ValueError(f"{name}: an empty list of utterances")
        for t in ts:
            if t.dim() != 2 or t.shape[1] != self._n_mels:
                raise ValueError(f"{name}: every utterance must be a [T, {self._n_mels}] tensor (frames as rows), got {tuple(t.shape)}")
        return tuple(int(t.shape[0]) for t in ts), torch.cat([self._prep(t).to(dev) for t in ts]).contiguous()

    def _no_grad_inputs(self, call, ts, what, instead):
        if torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in ts):
            raise RuntimeError(f"{call} is forward-only: {what} requires grad and its gradient would be lost.  Use the differentiable "
                               f"uniform path {instead} or pass detached tensors")

    def _src_map(self, call, src_of, S):
        try:
            m = tuple(int(j) for j in src_of)
        except (TypeError, ValueError):
            raise ValueError(f"{call}: src_of must be a list of source indices (output j is decoded from source src_of[j])") from None
        if not m or any(not 0 <= j < S for j in m):
            raise ValueError(f"{call}: src_of must be a non-empty list of source indices in [0, {S}) (there are {S} sources), got {list(m)}")
        return m

    def _voices(self, call, emb, N, what, detach=True):
        C = self._c_emb
        if not torch.is_tensor(emb):
            raise ValueError(f"{call}: emb must be a tensor of shape [{N}, {C}] or [{C}]")
        e = self._prep(emb.detach() if detach else emb).to(self._flat.device)
        if e.dim() == 1 and e.shape[0] == C:
            e = e[None]
        if e.dim() != 2 or e.shape[1] != C or e.shape[0] not in (1, N):
            raise ValueError(f"{call}: emb must be [{N}, {C}] (one row per {what}), or [{C}] / [1, {C}] (one voice for all "
                             f"{N} outputs); got {tuple(emb.shape)}")
        return e.expand(N, C) if e.shape[0] == 1 else e   # batch stride 0: the engine reads the one row N times

    def inference_ragged(self, xs, x_conds=None, emb=None, src_of=None):
        """Batched ``inference`` over utterances of DIFFERENT lengths in ONE launch set (engine.RaggedPlan; the reference converts
        one utterance per call, inference.py:62-70).  xs / x_conds: lists of [T_b, M] / [T'_b, M] tensors (frames as rows -- what
        ``utt_make_frames`` views); returns the list of converted [M, T''_b] tensors, result b == inference(x_b, x_cond_b).

        Exactly one of ``x_conds`` and ``emb``.  ``emb``: speaker embeddings the caller already has (``get_speaker_embeddings_ragged``,
        a mean over enrolment utterances, a point between two speakers) -- [B, c_emb], one row per source, or [c_emb] / [1, c_emb]: one
        voice for all sources (read with batch stride 0, never expanded in memory).  The speaker encoder then does not run at all;
        result b == decoder(content_encoder(x_b)[0], emb_b), bit-identical in fp32 to the ``x_conds`` call those embeddings came from.
        Forward only, like the ``x_conds`` form: an ``emb`` that requires grad is refused while grad is enabled.

        ``src_of`` (with ``emb`` only): FAN-OUT.  ``src_of[j]`` is the source of output j (any order, repeats and unused sources
        legal), ``emb`` is [N, c_emb] with N = len(src_of) (or one voice for all), and N tensors come back: output j ==
        decoder(content_encoder(xs[src_of[j]])[0], emb_j), bit-identical to ``inference_ragged([xs[src_of[j]] ...], emb=emb)`` --
        but every source is uploaded and encoded ONCE, and the decoder's voice-independent first stage runs once per source (a
        "fanout" RaggedPlan).  Without ``src_of`` the call is what it was (an "emb" plan)."""
        if src_of is not None:
            if emb is None or x_conds is not None:
                raise ValueError("inference_ragged: src_of goes with emb (speaker embeddings, [len(src_of), c_emb] or [c_emb]) and without x_conds: "
                                 "enrol the voices first (get_speaker_embeddings_ragged)")
            if torch.is_tensor(emb):
                self._no_grad_inputs("inference_ragged", [emb], "emb", "decoder(z, cond) -- ae.decoder(ae.content_encoder(x)[0], emb) --")
            self._no_grad_inputs("inference_ragged(..., src_of=...)", list(xs), "a source", "decoder(content_encoder(x)[0], emb)")
            T, x = self._ragged_rows(xs, "xs")
            m = self._src_map("inference_ragged", src_of, len(T))
            e = self._voices("inference_ragged", emb, len(m), "output: len(src_of) rows")
            plan, ws = self._ragged_plan("fanout", T, (), m)
            plan.forward_emb(self._flat, x, e, ws)
            return [o.clone() for o in plan.outputs(ws)]
        if (x_conds is None) == (emb is None):
            raise ValueError("inference_ragged: pass exactly one of x_conds (a list of target utterances, [T'_b, M] each) and "
                             "emb (speaker embeddings, [B, c_emb] or [c_emb])")
        if emb is None:
            T, x = self._ragged_rows(xs, "xs")
            Tc, xc = self._ragged_rows(x_conds, "x_conds")
            if len(T) != len(Tc):
                raise ValueError(f"inference_ragged: {len(T)} sources but {len(Tc)} targets")
            plan, ws = self._ragged_plan("pairs", T, Tc)
            plan.forward(self._flat, x, xc, ws)
            return [o.clone() for o in plan.outputs(ws)]
        if not torch.is_tensor(emb):
            raise ValueError(f"inference_ragged: emb must be a tensor of shape [B, {self._c_emb}] or [{self._c_emb}]")
        if torch.is_grad_enabled() and emb.requires_grad:
            raise RuntimeError("inference_ragged is forward-only: emb requires grad and its gradient would be lost.  Use the differentiable "
                               "uniform path decoder(z, cond) -- ae.decoder(ae.content_encoder(x)[0], emb) -- or pass emb.detach()")
        T, x = self._ragged_rows(xs, "xs")
        B, C = len(T), self._c_emb
        e = self._prep(emb.detach()).to(self._flat.device)
        if e.dim() == 1 and e.shape[0] == C:
            e = e[None]
        if e.dim() != 2 or e.shape[1] != C or e.shape[0] not in (1, B):
            raise ValueError(f"inference_ragged: emb must be [{B}, {C}] (one row per source), or [{C}] / [1, {C}] (one voice for all "
                             f"{B} sources); got {tuple(emb.shape)}")
        if e.shape[0] == 1:
            e = e.expand(B, C)   # batch stride 0: the engine reads the one row B times
        plan, ws = self._ragged_plan("emb", T, ())
        plan.forward_emb(self._flat, x, e, ws)
        return [o.clone() for o in plan.outputs(ws)]

    def content_latents_ragged(self, xs):
        """The content codes of utterances of DIFFERENT lengths in ONE launch set (an "encode" RaggedPlan: the content encoder alone):
        xs is a list of [T_s, M] tensors; returns the list of mu [c_lat, Tz_s] (Tz_s = ceil(T_s / 8) for the stock config), mu_s ==
        content_encoder(x_s)[0], bit-identical to what ``inference_ragged`` computes inside.  Keep them and render them later, in any
        voice, with ``decode_ragged``.  Forward only: sources that require grad are refused while grad is enabled."""
        self._no_grad_inputs("content_latents_ragged", list(xs), "a source", "content_encoder(x)")
        T, x = self._ragged_rows(xs, "xs")
        plan, ws = self._ragged_plan("encode", T, ())
        plan.forward(self._flat, x, None, ws)
        return [mu.clone() for mu in plan.latents(ws)[0]]

    @staticmethod
    def _latent_views(muls, plan):
        """(list of mu, list of log_sigma) [c_lat, Tz_s] views of the packed (mu | log_sigma) blocks a ragged content function returns"""
        c, base = plan.c_lat, plan.lat_off[0]
        mu = [muls[o - base:o - base + c * n].view(c, n) for o, n in zip(plan.lat_off, plan.lat_len)]
        ls = [muls[o - base + c * n:o - base + 2 * c * n].view(c, n) for o, n in zip(plan.lat_off, plan.lat_len)]
        return mu, ls

    def content_encoder_ragged(self, xs, param_grads=False):
        """``content_encoder`` over utterances of DIFFERENT lengths in ONE launch set: xs is a list of [T_s, M] tensors (frames as rows);
        returns (list of mu [c_lat, Tz_s], list of log_sigma [c_lat, Tz_s]), entry s == content_encoder(x_s), bit-identical to
        ``content_latents_ragged``.

        Differentiable with respect to its inputs: with grad enabled and at least one utterance that requires grad, the results are
        views of ONE packed tensor with a ``grad_fn``, and a backward gives every such utterance a ``.grad`` of its own shape [T_s, M]
        (utterances that do not require grad get none).  The backward pass of all utterances is ONE ragged launch set in fp32
        (``RaggedPlan(mode="encode", input_grads=True)``); the parameters are frozen on this path (their gradients:
        ``content_encoder(x)`` on uniform shapes).  Grad plans have a workspace of their OWN (see ``get_speaker_embeddings_ragged``); a
        second grad forward of the same lengths while a backward is pending gets a private workspace.  Under ``compute_dtype: bf16`` the
        grad path raises: use the uniform ``content_encoder(x_b)``.  Without grad the call runs the pooled forward-only "encode" plan.

        ``param_grads=True``: differentiable with respect to the content encoder's PARAMETERS as well.  With grad enabled the results
        carry a ``grad_fn`` when a content-encoder parameter or an utterance requires grad; a backward gives every such parameter its
        ``.grad`` (accumulated as torch accumulates; the other two networks' parameters get nothing) and every such utterance its own --
        all from ONE ragged backward pass in fp32 (``RaggedPlan(mode="encode_pg")``, avc_content_backward_ragged_params).  When no
        parameter requires grad the call is the default one, with its bits.  The default (False) is unchanged: it stays forward-only
        while only parameters require grad."""
        T, x = self._ragged_rows(xs, "xs")
        if param_grads and torch.is_grad_enabled():
            lo, hi = self._part_index["content"]
            params = list(self.parameters())[lo:hi]
            if any(p.requires_grad for p in params):
                if str(self.compute_dtype).lower().startswith(("bf16", "bfloat16")):
                    raise RuntimeError("content_encoder_ragged: gradients through the ragged path are fp32 only, and compute_dtype is "
                                       f"{self.compute_dtype!r} (ragged plans then run 'bf16r', a forward-only rounding model).  Use the uniform path "
                                       "content_encoder(x_b) per utterance, or call under torch.no_grad()")
                muls = _RaggedContentParamFunction.apply(self, x, T, *params)
                return self._latent_views(muls, self._ragged_plan("encode_pg", T, ())[0])
        if torch.is_grad_enabled() and x.requires_grad:
            if str(self.compute_dtype).lower().startswith(("bf16", "bfloat16")):
                raise RuntimeError("content_encoder_ragged: input gradients through the ragged path are fp32 only, and compute_dtype is "
                                   f"{self.compute_dtype!r} (ragged plans then run 'bf16r', a forward-only rounding model).  Use the uniform path "
                                   "content_encoder(x_b) per utterance, or detach the inputs")
            muls = _RaggedContentFunction.apply(self, x, T)
            return self._latent_views(muls, self._ragged_plan("encode_ig", T, ())[0])
        plan, ws = self._ragged_plan("encode", T, ())
        plan.forward(self._flat, x, None, ws)
        mu, ls = plan.latents(ws)
        return [m.clone() for m in mu], [l.clone() for l in ls]

    def decode_ragged(self, zs, emb, src_of=None):
        """The decoder alone over latents of DIFFERENT lengths in ONE launch set (a "decode" RaggedPlan): zs is a list of
        [c_lat, Tz_s] tensors (``content_latents_ragged``'s, or any other), emb is [N, c_emb] or [c_emb] / [1, c_emb], ``src_of[j]`` the
        latent of output j (None: one output per latent, in order).  Returns N tensors [M, T''_j], output j == decoder(zs[src_of[j]],
        emb_j); with the latents of ``content_latents_ragged(xs)`` bit-identical to ``inference_ragged(xs, emb=emb, src_of=src_of)``.
        Forward only: latents or embeddings that require grad are refused while grad is enabled."""
        zs = list(zs)
        if not zs:
            raise ValueError("decode_ragged: an empty list of latents")
        for z in zs:
            if not torch.is_tensor(z) or z.dim() != 2 or z.shape[0] != self._c_lat:
                raise ValueError(f"decode_ragged: every latent must be a [{self._c_lat}, Tz] tensor, got {tuple(z.shape) if torch.is_tensor(z) else type(z)}")
        self._no_grad_inputs("decode_ragged", zs + [emb], "a latent or emb", "decoder(z, cond)")
        dev = self._flat.device
        Tz = tuple(int(z.shape[1]) for z in zs)
        m = self._src_map("decode_ragged", src_of if src_of is not None else range(len(zs)), len(zs))
        e = self._voices("decode_ragged", emb, len(m), "output")
        z = torch.cat([self._prep(z.detach()).to(dev).reshape(-1) for z in zs])   # block s = [c_lat][Tz_s], frames contiguous
        plan, ws = self._ragged_plan("decode", Tz, (), m)
        plan.forward_latents(self._flat, z, self._c_lat, e, ws)
        return [o.clone() for o in plan.outputs(ws)]

    def decoder_ragged(self, zs, emb, param_grads=False):
        """``decoder`` over latents of DIFFERENT lengths in ONE launch set: zs is a list of [c_lat, Tz_s] tensors, emb is [N, c_emb]
        (one row per latent) or [c_emb] / [1, c_emb] (one voice for all); returns N tensors [M, T''_j], output j == decoder(zs[j], emb_j),
        bit-identical to ``decode_ragged(zs, emb)``.

        Differentiable with respect to its inputs: with grad enabled and a latent or ``emb`` that requires grad, the results are views of
        ONE packed tensor with a ``grad_fn``, and a backward gives every latent leaf a ``.grad`` of its own shape [c_lat, Tz_s] and ``emb``
        one of its own shape (a single voice gets the sum over the N outputs).  The backward pass of all latents is ONE ragged launch set
        in fp32 (``RaggedPlan(mode="decode_ig")``); the parameters are frozen on this path (their gradients: ``decoder(z, cond)`` on
        uniform shapes).  Grad plans have a workspace of their OWN (see ``get_speaker_embeddings_ragged``); a second grad forward of the
        same lengths while a backward is pending gets a private workspace.  There is no ``src_of`` on the grad path: to render one latent
        in several voices pass ``[zs[j] for j in src_of]`` -- torch's autograd sums the gradients of a repeated latent.  Under
        ``compute_dtype: bf16`` the grad path raises: use the uniform ``decoder(z_b, emb_b)``.  Without grad the call is
        ``decode_ragged(zs, emb)``.

        ``param_grads=True``: differentiable with respect to the decoder's PARAMETERS as well (fine-tuning the decoder to a voice on whole
        utterances).  With grad enabled the results carry a ``grad_fn`` when a decoder parameter, a latent or ``emb`` requires grad; a
        backward gives every such parameter its ``.grad`` (accumulated as torch accumulates; the other two networks' parameters get
        nothing) and the inputs theirs -- all from ONE ragged backward pass in fp32 (``RaggedPlan(mode="decode_pg")``,
        avc_decoder_backward_ragged_params).  When no parameter requires grad the call is the default one, with its bits.  The default
        (False) is unchanged: it stays forward-only while only parameters require grad."""
        zs = list(zs)
        params = ()
        if param_grads and torch.is_grad_enabled():
            lo, hi = self._part_index["decoder"]
            params = list(self.parameters())[lo:hi]
            if not any(p.requires_grad for p in params):
                params = ()
        need = torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in zs + [emb])
        if not need and not params:
            return self.decode_ragged(zs, emb)
        for z in zs:
            if not torch.is_tensor(z) or z.dim() != 2 or z.shape[0] != self._c_lat:
                raise ValueError(f"decoder_ragged: every latent must be a [{self._c_lat}, Tz] tensor, got {tuple(z.shape) if torch.is_tensor(z) else type(z)}")
        if str(self.compute_dtype).lower().startswith(("bf16", "bfloat16")):
            raise RuntimeError("decoder_ragged: input gradients through the ragged path are fp32 only, and compute_dtype is "
                               f"{self.compute_dtype!r} (ragged plans then run 'bf16r', a forward-only rounding model).  Use the uniform path "
                               "decoder(z_b, emb_b) per utterance, or detach the inputs")
        dev = self._flat.device
        Tz = tuple(int(z.shape[1]) for z in zs)
        e = self._voices("decoder_ragged", emb, len(zs), "latent", detach=False)
        z = torch.cat([self._prep(z).to(dev).reshape(-1) for z in zs])   # block s = [c_lat][Tz_s], frames contiguous
        if params:
            dec = _RaggedDecoderParamFunction.apply(self, z, e, Tz, *params)
        else:
            dec = _RaggedDecoderFunction.apply(self, z, e, Tz)
        plan = self._ragged_plan("decode_pg" if params else "decode_ig", Tz, ())[0]
        M, base = plan.n_mels, plan.out_off[0]
        return [dec[o - base:o - base + M * n].view(M, n) for o, n in zip(plan.out_off, plan.out_len)]

    def get_speaker_embeddings_ragged(self, x_conds):
        """``get_speaker_embeddings`` (model.py:393-395) over utterances of DIFFERENT lengths in ONE launch set: x_conds is a list of
        [T'_b, M] tensors (frames as rows, the layout ``inference_ragged`` takes); returns [B, c_emb], row b ==
        get_speaker_embeddings(x_cond_b).  Only the speaker encoder runs (a "speaker" RaggedPlan).

        Differentiable with respect to its inputs: with grad enabled and at least one utterance that requires grad, the result carries a
        ``grad_fn`` and a backward gives every such utterance a ``.grad`` of its own shape [T'_b, M] (transposed / strided views and
        utterances on another device included; utterances that do not require grad get none).  The backward pass of all utterances is
        ONE ragged launch set in fp32 (``RaggedPlan(mode="speaker", input_grads=True)``); the parameters are frozen on this path
        (their gradients: ``speaker_encoder(x)`` on uniform shapes).  Grad plans have a workspace of their OWN, apart from the pooled
        workspace of the forward-only ragged calls: no other ragged call can overwrite the saved activations between this forward and
        its backward, and a second grad forward of the same lengths before that backward gets a private workspace.  Under
        ``compute_dtype: bf16`` the grad path raises (ragged plans then round operands to bf16, a forward-only model): use the uniform
        ``get_speaker_embeddings(x_b)``.  Without grad the call is the forward-only one, bit for bit."""
        Tc, xc = self._ragged_rows(x_conds, "x_conds")
        if torch.is_grad_enabled() and xc.requires_grad:
            if str(self.compute_dtype).lower().startswith(("bf16", "bfloat16")):
                raise RuntimeError("get_speaker_embeddings_ragged: input gradients through the ragged path are fp32 only, and compute_dtype is "
                                   f"{self.compute_dtype!r} (ragged plans then run 'bf16r', a forward-only rounding model).  Use the uniform path "
                                   "get_speaker_embeddings(x_b) / speaker_encoder(x_b) per utterance, or detach the inputs")
            return _RaggedSpeakerFunction.apply(self, xc, Tc)
        plan, ws = self._ragged_plan("speaker", (), Tc)
        plan.forward(self._flat, None, xc, ws)
        return plan.emb(ws).clone()

    def speaker_encoder_ragged(self, x_conds):
        """``speaker_encoder(x)`` (the sub-module call) over utterances of DIFFERENT lengths in ONE launch set, the ragged counterpart beside
        ``content_encoder_ragged`` and ``decoder_ragged``: x_conds is a list of [T'_b, M] tensors; returns [B, c_emb], bit-identical to
        ``get_speaker_embeddings_ragged(x_conds)``.

        Differentiable with respect to the speaker encoder's PARAMETERS and to its inputs: with grad enabled the result carries a
        ``grad_fn`` when a speaker-encoder parameter or an utterance requires grad.  A backward then gives every speaker-encoder parameter
        that requires grad its ``.grad`` (accumulated as torch accumulates; the other two networks' parameters get nothing) and every
        utterance that requires grad its own -- all from ONE ragged backward pass in fp32 (``RaggedPlan(mode="speaker_pg")``,
        avc_backward_ragged_params).  When no parameter requires grad the frozen pass of ``get_speaker_embeddings_ragged`` runs, with its
        bits.  Workspace ownership, a second grad forward before a pending backward and the ``compute_dtype: bf16`` refusal are those of
        ``get_speaker_embeddings_ragged``, which itself is unchanged: it stays forward-only while only parameters require grad."""
        lo, hi = self._part_index["speaker"]
        params = list(self.parameters())[lo:hi]
        if not (torch.is_grad_enabled() and any(p.requires_grad for p in params)):
            return self.get_speaker_embeddings_ragged(x_conds)
        Tc, xc = self._ragged_rows(x_conds, "x_conds")
        if str(self.compute_dtype).lower().startswith(("bf16", "bfloat16")):
            raise RuntimeError("speaker_encoder_ragged: gradients through the ragged path are fp32 only, and compute_dtype is "
                               f"{self.compute_dtype!r} (ragged plans then run 'bf16r', a forward-only rounding model).  Use the uniform path "
                               "speaker_encoder(x_b) per utterance, or call under torch.no_grad()")
        return _RaggedSpeakerParamFunction.apply(self, xc, Tc, *params)

    # ---- the three networks called on their own (SpeakerEncoder / ContentEncoder / Decoder.forward) --------
    def _part_grad(self, part, *inputs):
        lo, hi = self._part_index[part]
        return torch.is_grad_enabled() and (any(p.requires_grad for p in list(self.parameters())[lo:hi]) or
                                            any(t.requires_grad for t in inputs))

    def _speaker_forward(self, x):
        x = self._prep(x)
        self._check_device(x)
        if self._part_grad("speaker", x):
            return _SpeakerFunction.apply(self, x, *self.speaker_encoder.parameters())
        plan, ws = self._plan(x.shape[0], x.shape[2], x.shape[2], x.device, "speaker")
        plan.forward(self._flat, x, None, None, ws)
        return plan.view(ws, "emb", (x.shape[0], self._c_emb)).clone()

    def _content_forward(self, x):
        x = self._prep(x)
        self._check_device(x)
        if self._part_grad("content", x):
            return _ContentFunction.apply(self, x, *self.content_encoder.parameters())
        plan, ws = self._plan(x.shape[0], x.shape[2], x.shape[2], x.device, "content")
        plan.forward(self._flat, x, None, None, ws)
        muls = plan.view(ws, "muls", (x.shape[0], 2 * self._c_lat, plan.latent_len))
        return muls[:, :self._c_lat].clone(), muls[:, self._c_lat:].clone()

    def _decoder_forward(self, z, cond):
        z, cond = self._prep(z), self._prep(cond)
        self._check_device(z)
        self._check_device(cond)
        if z.dim() != 3 or z.shape[1] != self._c_lat or cond.dim() != 2 or cond.shape != (z.shape[0], self._c_emb):
            raise ValueError(f"Decoder: z must be [B, {self._c_lat}, Tb] and cond [B, {self._c_emb}], got {tuple(z.shape)} and {tuple(cond.shape)}")
        if self._part_grad("decoder", z, cond):
            return _DecoderFunction.apply(self, z, cond, *self.decoder.parameters())
        plan, ws = self._plan(z.shape[0], z.shape[2], z.shape[2], z.device, "decoder")
        plan.decoder_forward(self._flat, z, cond, ws)
        return plan.view(ws, "dec", (z.shape[0], self._n_mels, plan.out_len)).clone()

    def get_speaker_embeddings(self, x):
        """model.py:393-395: only the speaker encoder runs (a speaker-only plan).  An x that requires grad takes the autograd path of
        ``speaker_encoder(x)``."""
        x = self._prep(x)
        self._check_device(x)
        if torch.is_grad_enabled() and x.requires_grad:
            return self._speaker_forward(x)
        plan, ws = self._plan(x.shape[0], x.shape[2], x.shape[2], x.device, "speaker")
        plan.forward(self._flat, x, x, None, ws)
        return plan.view(ws, "emb", (x.shape[0], self._c_emb)).clone()
