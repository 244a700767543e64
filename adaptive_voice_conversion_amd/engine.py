"""Thin Python handle on the C-ABI launch plan (include/avc_hip.h).

PyTorch is plumbing here: it owns device memory and the stream; every kernel is
launched by libavc_hip.so.
"""
import contextlib
import ctypes

import torch

from . import _lib
from ._lib import DecoderCfg, EncoderCfg, ModelCfg


ACTS = {"relu": 0, "lrelu": 1}   # model.py:93-99 get_act: nn.ReLU / nn.LeakyReLU (slope 0.01)
_warned = set()


def _warn_once(key, msg):
    if key not in _warned:
        _warned.add(key)
        import warnings
        warnings.warn(msg, RuntimeWarning, stacklevel=3)


def _act_code(name, c):
    """model.py:93-99 get_act: 'relu' -> ReLU, 'lrelu' -> LeakyReLU, ANYTHING ELSE -> ReLU as well (the reference's fallback branch).
    The same here, with a warning: a config with e.g. act: 'elu' trains as ReLU in the reference too."""
    act = c.get("act", "relu")
    if act not in ACTS:
        _warn_once(("act", name, str(act)), f"{name}.act={act!r}: the reference's get_act (model.py:93-99) maps every string other than "
                                            "'relu' / 'lrelu' to nn.ReLU(); so does this engine.")
        return ACTS["relu"]
    return ACTS[act]


def _check_common(name, c):
    if float(c.get("dropout_rate", 0)) != 0.0:
        raise NotImplementedError(f"{name}.dropout_rate={c['dropout_rate']}: only 0 (config.yaml default) is implemented")


def cfg_from_dict(config) -> ModelCfg:
    """config.yaml:1-36 -> avc_model_cfg.  Unsupported options fail loudly."""
    m = ModelCfg()
    for key, dst, dense in (("SpeakerEncoder", m.spk, True), ("ContentEncoder", m.enc, False)):
        c = config[key]
        _check_common(key, c)
        for f in ("c_in", "c_h", "c_out", "kernel_size", "bank_size", "bank_scale", "c_bank", "n_conv_blocks"):
            setattr(dst, f, int(c[f]))
        dst.n_dense_blocks = int(c["n_dense_blocks"]) if dense else 0
        dst.act = _act_code(key, c)
        if dst.n_conv_blocks > _lib.MAX_BLOCKS:
            raise NotImplementedError("more than 8 conv blocks")
        for i, s in enumerate(list(c["subsample"])[: dst.n_conv_blocks]):
            dst.subsample[i] = int(s)
    d = config["Decoder"]
    _check_common("Decoder", d)
    if d.get("sn", False):
        raise NotImplementedError("Decoder.sn=True (spectral norm) is not implemented; config.yaml default is False")
    for f in ("c_in", "c_cond", "c_h", "c_out", "kernel_size", "n_conv_blocks"):
        setattr(m.dec, f, int(d[f]))
    m.dec.act = _act_code("Decoder", d)
    for i, s in enumerate(list(d["upsample"])[: m.dec.n_conv_blocks]):
        m.dec.upsample[i] = int(s)
    return m


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream(t):
    if t.is_cuda:
        return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)
    return None


def _on(t):
    """Make the tensor's device the current HIP device for the duration of a C-ABI call: the library
    launches on (and its plans create helper streams on) whatever device is current."""
    return torch.cuda.device(t.device) if (t is not None and t.is_cuda) else contextlib.nullcontext()


def unpack_pairs(p):
    """bf16 pair tensor (int32 [B, C/2, T]: channel 2p in the low half, 2p + 1 in the high half) -> fp32 [B, C, T]"""
    lo = (p & 0xFFFF).to(torch.int16).view(torch.bfloat16).to(torch.float32)
    hi = ((p >> 16) & 0xFFFF).to(torch.int16).view(torch.bfloat16).to(torch.float32)
    return torch.stack((lo, hi), dim=2).reshape(p.shape[0], 2 * p.shape[1], p.shape[2])


def unpack_planar(p):
    """natural bf16 rows (int32 [B, C, T/2]: frames 2i, 2i + 1 per dword) -> fp32 [B, C, T]"""
    lo = (p & 0xFFFF).to(torch.int16).view(torch.bfloat16).to(torch.float32)
    hi = ((p >> 16) & 0xFFFF).to(torch.int16).view(torch.bfloat16).to(torch.float32)
    return torch.stack((lo, hi), dim=3).reshape(p.shape[0], p.shape[1], 2 * p.shape[2])


def _param_info(lib, h):
    """(number of parameter tensors, [(offset, numel, shape)] of each in the flat parameter buffer) of a plan handle"""
    info = []
    for i in range(lib.avc_plan_num_params(h)):
        off, n, dims = ctypes.c_long(), ctypes.c_long(), (ctypes.c_int * 3)()
        lib.avc_plan_param_info(h, i, ctypes.byref(off), ctypes.byref(n), ctypes.byref(dims))
        info.append((off.value, n.value, tuple(d for d in dims if d > 0)))
    return len(info), info


def _ints(v):
    return (ctypes.c_int * len(v))(*v) if v else None


def _packed(t, n, name, what, ws, at_least=False):
    """t: a contiguous fp32 tensor of n (at_least: or more) elements on the workspace's device; what: its layout, for the message"""
    if t.dtype != torch.float32 or t.device != ws.device or not t.is_contiguous() or (t.numel() < n if at_least else t.numel() != n):
        raise ValueError(f"{name} must be a contiguous fp32 tensor of {'at least ' if at_least else ''}{n} elements on {ws.device}{what}")


def _blocks(ws, off, c, lens):
    """list of [c, len] views of the blocks that lie back to back in the workspace from float offset ``off``"""
    out = []
    for n in lens:
        out.append(ws[off:off + c * n].view(c, n))
        off += c * n
    return out


class Plan:
    """One (B, T, T_cond) launch plan.  ``lib`` defaults to the gfx950 library;
    tests may inject the CPU lane-level simulation build instead."""

    MODES = {"train": 0, "inference": _lib.PLAN_INFERENCE, "speaker": _lib.PLAN_INFERENCE | _lib.PLAN_SPEAKER_ONLY,
             "content": _lib.PLAN_INFERENCE | _lib.PLAN_CONTENT_ONLY, "decoder": _lib.PLAN_INFERENCE | _lib.PLAN_DECODER_ONLY,
             "speaker_train": _lib.PLAN_SPEAKER_ONLY | _lib.PLAN_PART_GRADS, "content_train": _lib.PLAN_CONTENT_ONLY | _lib.PLAN_PART_GRADS,
             "decoder_train": _lib.PLAN_DECODER_ONLY | _lib.PLAN_PART_GRADS,
             # ... whose backward also leaves d(loss)/d(x) in ws["d_x"] (and d(loss)/d(x_cond) in ws["d_x_cond"])
             "ig_train": _lib.PLAN_INPUT_GRADS, "speaker_ig_train": _lib.PLAN_SPEAKER_ONLY | _lib.PLAN_PART_GRADS | _lib.PLAN_INPUT_GRADS,
             "content_ig_train": _lib.PLAN_CONTENT_ONLY | _lib.PLAN_PART_GRADS | _lib.PLAN_INPUT_GRADS}
    COMPUTE = {"fp32": 0, "float32": 0, "f32": 0, "fp32x3": 0, "f32x3": 0, "bf16": 3, "bfloat16": 3, "bf16s": 3, "bf16_storage": 3,
               "bf16r": 1, "bf16_operands": 1}

    def __init__(self, config, B, T, T_cond=None, lib=None, compute_dtype="fp32", mode="train", device=None, tuning=None):
        """compute_dtype: "fp32" (default, the reference's precision);
        "bf16" = BASELINE config 3's precision on the bf16 STORAGE engine (AVC_PLAN_BF16S: activations and activation gradients are bf16
        channel-pair tensors in HBM and LDS, v_mfma_f32_32x32x16_bf16 products, fp32 accumulation / statistics / parameters / optimizer);
        shapes the pair kernels do not take (odd channel counts, frame counts that are not multiples of 4 at some level) fall back to
        "bf16r" -- ``plan.compute_dtype`` says which one the plan runs; "bf16s" = the storage engine or an error;
        "bf16r" = fp32 storage, conv / Linear operands rounded to bf16 as they enter the matrix core (round 2's bf16 mode);
        "fp32x3" = fp32-accurate products from three bf16 terms per operand on the bf16 matrix core for the big k = 5 convs and the
        whole-chunk weight gradients (opt-in; csrc/conv_x3.hip), exact fp32 everywhere else.
        mode: "train" (forward + loss + backward), "inference" (forward only: the workspace holds no gradient,
        slab or dy buffers) or "speaker" (only the speaker encoder runs, AE.get_speaker_embeddings); part plans of ONE network
        (SpeakerEncoder / ContentEncoder / Decoder.forward, model.py:265-277 / 301-323 / 347-371): "speaker", "content" and "decoder"
        run forward only, "speaker_train", "content_train" and "decoder_train" also their backward; "ig_train", "speaker_ig_train" and
        "content_ig_train" are "train" / "speaker_train" / "content_train" whose backward also computes the input gradients.  A decoder plan takes
        T = the latent length Tb of its input z and runs through ``decoder_forward`` / ``decoder_backward``.
        device: the plan's helper streams are created on it (default: the current device).
        tuning: {avc_tuning field: value} overrides of the launch heuristics / diagnostic switches the plan captures
        (A/B measurements and tests; include/avc_hip.h).  The library has no process-wide knobs."""
        self.lib = lib if lib is not None else _lib.load()
        self.cfg = cfg_from_dict(config)
        self.B, self.T, self.T_cond = int(B), int(T), int(T_cond or T)
        self.mode = mode
        flags = self.MODES[mode]
        h = ctypes.c_void_p()
        dev = torch.device(device) if device is not None else None
        key = str(compute_dtype).lower()
        if key not in self.COMPUTE:
            raise ValueError(f"compute_dtype must be one of {sorted(self.COMPUTE)}, got {compute_dtype!r}")
        x3 = key in ("fp32x3", "f32x3")
        if x3:
            flags |= _lib.PLAN_X3
        bh = self.COMPUTE[key] == 3
        strict = key in ("bf16s", "bf16_storage")
        self.tuning = dict(tuning or {})
        tun = _lib.make_tuning(self.lib, self.tuning)
        with (torch.cuda.device(dev) if (dev is not None and dev.type == "cuda") else contextlib.nullcontext()):
            rc = self.lib.avc_plan_create_tuned(ctypes.byref(self.cfg), self.B, self.T, self.T_cond, flags | (_lib.PLAN_BF16S if bh else 0),
                                                ctypes.byref(tun), ctypes.byref(h))
            if rc == _lib.ERR_PAIR_SHAPE and bh and not strict:
                # a shape outside the pair kernels (and nothing else: every other failure is reported): the operand-rounding bf16 mode takes
                # any shape.  The numerics (and the speed) of "bf16" then differ between shapes of the same model -- say so, once per shape class.
                _warn_once(("bf16r", self.T % 4, self.T_cond % 4),
                           f"compute_dtype 'bf16': B={self.B}, T={self.T}, T_cond={self.T_cond} is outside the bf16 storage engine "
                           f"({self.lib.avc_last_error().decode()}); this plan runs 'bf16r' (fp32 storage, operands rounded to bf16) instead. "
                           "Pass compute_dtype='bf16s' to make this an error.")
                bh = False
                rc = self.lib.avc_plan_create_tuned(ctypes.byref(self.cfg), self.B, self.T, self.T_cond, flags, ctypes.byref(tun), ctypes.byref(h))
        if rc != 0:
            raise RuntimeError(self.lib.avc_last_error().decode())
        self.h = h
        operand_bf16 = (self.COMPUTE[key] in (1, 3)) and not bh
        self.compute_dtype = "fp32x3" if x3 else ("bf16" if bh else ("bf16r" if operand_bf16 else "fp32"))
        self.pair_storage = bh
        if not bh and self.lib.avc_plan_set_compute_dtype(h, 1 if operand_bf16 else 0) != 0:
            raise RuntimeError(self.lib.avc_last_error().decode())
        self.num_params, self.param_info = _param_info(self.lib, h)
        self.param_floats = self.lib.avc_plan_param_floats(h)
        self.workspace_floats = self.lib.avc_plan_workspace_floats(h)
        self.out_len = self.lib.avc_plan_out_len(h)
        self.latent_len = self.lib.avc_plan_latent_len(h)

    def close(self):
        """avc_plan_destroy: releases the plan's helper streams / events (the workspace is the caller's)."""
        if getattr(self, "h", None):
            self.lib.avc_plan_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def param_range(self, part):
        """(offset, numel) of a part of the flat parameter / gradient buffer (_lib.GRADS_*)."""
        off, n = ctypes.c_long(), ctypes.c_long()
        if self.lib.avc_plan_param_range(self.h, int(part), ctypes.byref(off), ctypes.byref(n)) != 0:
            raise ValueError(part)
        return off.value, n.value

    def stream_wait_grads(self, part, stream):
        """Make ``stream`` (a torch.cuda.Stream) wait until that part of the gradients of the last
        ``backward`` call is final (data-parallel overlap).  Returns False when the plan has no helper
        streams / events (nothing was ordered: the caller must wait for the stream backward ran on)."""
        rc = self.lib.avc_plan_stream_wait_grads(self.h, int(part), ctypes.c_void_p(stream.cuda_stream))
        if rc == -9:
            return False
        self._chk(rc)
        return True

    def set_single_stream(self, on):
        """Profiling aid: every kernel of this plan on the caller's stream."""
        self._chk(self.lib.avc_plan_set_single_stream(self.h, int(bool(on))))

    def buffer(self, name):
        off = self.lib.avc_plan_buffer(self.h, name.encode())
        if off < 0:
            raise KeyError(name)
        return off

    def view(self, ws, name, shape):
        off = self.buffer(name)
        n = 1
        for s in shape:
            n *= s
        return ws[off:off + n].view(*shape)

    def num_sites(self):
        return self.lib.avc_plan_num_relu_sites(self.h)

    def site(self, ws, i):
        """Site i of the plan's site table (avc_plan_relu_site; the reference's forward call order) decoded from the workspace as fp32
        tensors (views where the storage is fp32): {"kind", "storage", "B", "C", "T"} plus
        kind 0: "act" [B, C, T] -- the stored activation ([B, C] for the dense stack's channel-major [C][B] rows);
        kind 1: "y" [B, C, T] -- the stored pre-norm conv output, "mean" / "rstd" [B, C, 1], "cond" [B, 2 C] (shift | scale) or None.
        storage 0: fp32; 1: bf16 pair tensor; 2: natural ("planar") bf16 rows behind a pixel-shuffling conv."""
        from ._lib import ReluSite
        s = ReluSite()
        if self.lib.avc_plan_relu_site(self.h, i, ctypes.byref(s)) != 0:
            raise IndexError(i)
        B, Cc, T = s.B, s.C, s.T
        out = {"kind": s.kind, "storage": int(s.storage), "B": B, "C": Cc, "T": T}
        wi = ws.view(torch.int32)
        if s.kind == 0:
            if s.storage == 1:
                act = unpack_pairs(torch.as_strided(wi, (B, Cc // 2, T), (s.sb, s.sc, s.st), s.act_off))
            else:
                act = torch.as_strided(ws, (B, Cc, T), (s.sb, s.sc, s.st), s.act_off)
            out["act"] = act.reshape(B, Cc) if (T == 1 and s.st == 0) else act
            return out
        if s.storage == 1:
            y = unpack_pairs(wi[s.y_off:s.y_off + B * (Cc // 2) * T].view(B, Cc // 2, T))
        elif s.storage == 2:
            y = unpack_planar(wi[s.y_off:s.y_off + B * Cc * (T // 2)].view(B, Cc, T // 2))
        else:
            y = ws[s.y_off:s.y_off + B * Cc * T].view(B, Cc, T)
        out["y"] = y
        out["mean"] = ws[s.stat_off:s.stat_off + B * Cc].view(B, Cc, 1)
        out["rstd"] = ws[s.stat_off + B * Cc:s.stat_off + 2 * B * Cc].view(B, Cc, 1)
        out["cond"] = torch.as_strided(ws, (B, 2 * Cc), (s.cond_sb, 1), s.cond_off) if s.cond_off >= 0 else None
        return out

    def relu_masks(self, ws):
        """0/1 masks of every ReLU of the last forward, in the reference's call order, computed
        from the engine's own saved tensors (diagnostics / branch-matched gradient checks)."""
        out = []
        for i in range(self.num_sites()):
            s = self.site(ws, i)
            if s["kind"] == 0:
                out.append(s["act"] > 0)
                continue
            Cc = s["C"]
            xh = ((s["y"] - s["mean"]) * s["rstd"]).double()      # the same two fp32 roundings as the kernel
            if s["cond"] is not None:
                cond = s["cond"].double()
                w = xh * cond[:, Cc:, None] + cond[:, :Cc, None]   # exact in fp64 -> same sign as the fp32 fma
            else:
                w = xh
            out.append(w > 0)
        return out

    def _chk(self, rc):
        if rc != 0:
            raise RuntimeError(f"libavc: {self.lib.avc_last_error().decode()}")

    def forward(self, params, x, x_cond, eps, ws, weights_packed=False):
        """weights_packed: the weight images in ``ws`` are current (``pack_weights(params, ws)`` ran after the last change of ``params``):
        the pass then opens with its first convolution instead of the pack launch."""
        xc = x if x_cond is None else x_cond
        with _on(ws):
            self._chk(self.lib.avc_forward_ex(self.h, _ptr(params), _ptr(x), x.stride(0), x.stride(1), x.stride(2), _ptr(xc),
                                              xc.stride(0), xc.stride(1), xc.stride(2), _ptr(eps), _ptr(ws),
                                              _lib.FWD_WEIGHTS_PACKED if weights_packed else 0, _stream(ws)))

    def pack_weights(self, params, ws):
        """Every weight tensor -> the plan's LDS-image order, ONE launch (a training loop calls this right behind its optimizer step)."""
        with _on(ws):
            self._chk(self.lib.avc_plan_pack_weights(self.h, _ptr(params), _ptr(ws), _stream(ws)))

    def loss(self, x, lambda_rec, ws):
        with _on(ws):
            self._chk(self.lib.avc_loss(self.h, _ptr(x), x.stride(0), x.stride(1), x.stride(2), float(lambda_rec), _ptr(ws), _stream(ws)))

    def backward(self, params, x, x_cond, eps, grads, ws, d_dec=None, d_muls=None, d_emb=None, lambda_kl=0.0):
        """x_cond None: both encoders read x (AE.forward; with AVC_PLAN_INPUT_GRADS ws["d_x"] then holds both encoders' terms)."""
        sc = (0, 0, 0) if x_cond is None else x_cond.stride()
        with _on(ws):
            self._chk(self.lib.avc_backward(self.h, _ptr(params), _ptr(x), x.stride(0), x.stride(1), x.stride(2), _ptr(x_cond),
                                            sc[0], sc[1], sc[2], _ptr(eps), _ptr(d_dec), _ptr(d_muls),
                                            _ptr(d_emb), float(lambda_kl), _ptr(grads), _ptr(ws), _stream(ws)))


    def decoder_forward(self, params, z, emb, ws, weights_packed=False):
        """Decoder.forward(z, emb) (model.py:347-371) on a decoder plan: z [B, c_in, Tb] and emb [B, c_cond] (fp32, any strides) are
        read in place; the result is ws["dec"]."""
        with _on(ws):
            self._chk(self.lib.avc_decoder_forward(self.h, _ptr(params), _ptr(z), z.stride(0), z.stride(1), z.stride(2), _ptr(emb), emb.stride(0),
                                                   emb.stride(1), _ptr(ws), _lib.FWD_WEIGHTS_PACKED if weights_packed else 0, _stream(ws)))

    def decoder_backward(self, params, z, emb, grads, ws, d_dec=None):
        """Its backward ("decoder_train" plans, after decoder_forward with the same z / emb): the decoder's range of ``grads``,
        ws["d_z"] [B, c_in, Tb] and ws["d_emb"] [B, c_cond].  d_dec: [B, M, Tout] contiguous (None = ws["d_dec"])."""
        with _on(ws):
            self._chk(self.lib.avc_decoder_backward(self.h, _ptr(params), _ptr(z), z.stride(0), z.stride(1), z.stride(2), _ptr(emb), emb.stride(0),
                                                    emb.stride(1), _ptr(d_dec), _ptr(grads), _ptr(ws), _stream(ws)))


class RaggedPlan:
    """Launch plan of ONE pass over B utterances of DIFFERENT lengths (avc_plan_create_ragged_ex).  Nothing is padded.  Forward only,
    except a "speaker" or an "encode" plan created with ``input_grads=True``, a "decode_ig" and a "speaker_pg" plan (below).

    mode "pairs" (default): B (source, target) pairs through all three networks, the batched form of
    ``Inferencer.inference_one_utterance`` (inference.py:54-70); result b equals ``AE.inference(x_b, x_cond_b)`` (model.py:387-391).
    mode "speaker": only the speaker encoder, over B target utterances of lengths ``T_cond`` (``T`` is ignored and may be None):
    ``forward(params, None, x_cond, ws)``, then ``emb(ws)`` is the [B, c_cond] result (AE.get_speaker_embeddings, model.py:393-395).
    mode "emb": content encoder + decoder over B sources of lengths ``T`` (``T_cond`` is ignored), the speaker embeddings come from the
    caller: ``forward_emb(params, x, emb, ws)``; result b equals ``decoder(content_encoder(x_b)[0], emb_b)``.
    The part plans pack only their networks' weights and their workspaces are smaller; in fp32 a branch computes bit for bit what it
    computes in the "pairs" plan over the same lengths.

    ``mode="speaker", input_grads=True`` (AVC_PLAN_INPUT_GRADS): the plan also has a backward pass with respect to its input, parameters
    frozen, fp32 only: after ``forward(params, None, x_cond, ws)``, ``backward(params, x_cond, d_emb, ws)`` leaves d(loss)/d(x_cond) in
    ``d_x_cond(ws)``, [sum T_cond, M] like x_cond.  Its forward is bit-identical to the plan without the flag; its workspace is larger
    (input-gradient weight images, gradient temporaries).

    ``mode="encode", input_grads=True`` (avc_plan_create_ragged_content_grads): the content encoder alone with a backward pass with
    respect to its input, parameters frozen, fp32 only: after ``forward(params, x, None, ws)``, ``backward_content(params, x, d_muls, ws)``
    leaves d(loss)/d(x) in ``d_x(ws)``, [sum T, M] like x.  d_muls has the layout of the (mu | log_sigma) blocks ``latents(ws)`` views.
    Forward bit-identical to the plan without the flag; a larger workspace (weight images, row statistics, gradient rows).

    FAN-OUT (avc_plan_create_ragged_fanout; forward only): the decoder's sample count is its own.  ``T`` are the lengths of S sources,
    ``src_of`` maps each of N outputs to its source (any order, repeats and unused sources legal; None = the identity), ``B`` stays
    the number of sources and ``N`` is the number of outputs (``out_len`` has N entries).
    mode "fanout": content encoder over the S sources ONCE, decoder over the N outputs: ``forward_emb(params, x, emb, ws)`` with x
    [sum T, M] (each source once) and emb [N, c_cond]; output j equals ``decoder(content_encoder(x_{src_of[j]})[0], emb_j)``.
    mode "encode": the content encoder alone (``src_of`` must be None): ``forward(params, x, None, ws)``, then ``latents(ws)``.
    mode "decode": the decoder alone from the caller's latents; ``T`` are the LATENT lengths: ``forward_latents(params, z, zc, emb, ws)``.

    mode "decode_ig" (avc_plan_create_ragged_decoder_grads; ``input_grads`` is implied): the "decode" plan with the identity map
    (output j from latent j, no ``src_of``) and a backward pass with respect to its two inputs, parameters frozen, fp32 only: after
    ``forward_latents(params, z, zc, emb, ws)``, ``backward_decoder(params, z, zc, emb, d_dec, ws)`` leaves d(loss)/d(z) in ``d_z(ws)``
    and d(loss)/d(emb) in ``d_emb(ws)``.  Forward bit-identical to the "decode" plan; a larger workspace (weight images, row statistics,
    d(cond), gradient rows).

    mode "speaker_pg" (avc_plan_create_ragged_speaker_grads; ``input_grads`` is implied): the "speaker" plan with input gradients whose
    backward pass can also compute the speaker encoder's PARAMETER gradients: ``backward_params(params, x_cond, d_emb, grads, ws)`` writes
    them into the flat buffer ``grads`` and leaves ``d_x_cond(ws)``; ``backward`` stays the frozen pass.  (A mode of its own, like
    "decode_ig": ``mode="speaker", input_grads=True`` keeps its plan, workspace size and launches.)  ``buffer()`` names of the saved rows: "dec_y0", "dec_y1_<l>", "dec_a1_<l>", "dec_y2_<l>", their statistics
    "dec_st0", "dec_st1_<l>", "dec_st2_<l>", and "cond" / "d_cond".  (``mode="decode", input_grads=True`` keeps raising: fan-out plans,
    with their free ``src_of``, are forward only.)

    modes "encode_pg" (avc_plan_create_ragged_content_param_grads) and "decode_pg" (avc_plan_create_ragged_decoder_param_grads;
    ``input_grads`` is implied): the ``mode="encode", input_grads=True`` / "decode_ig" plans whose backward pass can also compute the
    network's PARAMETER gradients: ``backward_content_params(params, x, d_muls, grads, ws)`` / ``backward_decoder_params(params, z, zc,
    emb, d_dec, grads, ws)`` write them into the flat buffer ``grads`` and leave ``d_x(ws)`` / ``d_z(ws)`` and ``d_emb(ws)``;
    ``backward_content`` / ``backward_decoder`` stay the frozen passes.  Forwards and frozen passes are bit-identical to the older plans';
    those keep their workspace sizes and launches."""

    MODES = {"pairs": 0, "speaker": _lib.PLAN_SPEAKER_ONLY, "emb": _lib.PLAN_EMB_INPUT}
    FAN_MODES = {"fanout": 0, "encode": _lib.PLAN_CONTENT_ONLY, "decode": _lib.PLAN_DECODER_ONLY}
    # mode -> (which of T / T_cond are its lengths, whether src_of is allowed, (creator, flags) of the forward-only plan,
    #          (creator, flags) with input_grads); None: there is no such plan
    _EX, _FAN, _IG = "avc_plan_create_ragged_ex", "avc_plan_create_ragged_fanout", _lib.PLAN_INPUT_GRADS
    KINDS = {"pairs": ("both", False, ("avc_plan_create_ragged", 0), (_EX, _IG)),
             "speaker": ("T_cond", False, (_EX, MODES["speaker"]), (_EX, MODES["speaker"] | _IG)),
             "emb": ("T", False, (_EX, MODES["emb"]), (_EX, MODES["emb"] | _IG)),
             "fanout": ("T", True, (_FAN, FAN_MODES["fanout"]), None),
             "encode": ("T", False, (_FAN, FAN_MODES["encode"]), ("avc_plan_create_ragged_content_grads", 0)),
             "decode": ("T", True, (_FAN, FAN_MODES["decode"]), None),
             "decode_ig": ("T", False, None, ("avc_plan_create_ragged_decoder_grads", 0)),
             "speaker_pg": ("T_cond", False, None, ("avc_plan_create_ragged_speaker_grads", 0)),
             "encode_pg": ("T", False, None, ("avc_plan_create_ragged_content_param_grads", 0)),
             "decode_pg": ("T", False, None, ("avc_plan_create_ragged_decoder_param_grads", 0))}

    def __init__(self, config, T, T_cond=None, lib=None, compute_dtype="fp32", device=None, tuning=None, mode="pairs", input_grads=False,
                 src_of=None):
        self.lib = lib if lib is not None else _lib.load()
        self.cfg = cfg_from_dict(config)
        if mode not in self.KINDS:
            raise ValueError(f"mode must be one of {sorted(self.MODES) + sorted(self.FAN_MODES) + ['decode_ig', 'speaker_pg', 'encode_pg', 'decode_pg']}, got {mode!r}")
        lengths, takes_src_of, plain, with_grads = self.KINDS[mode]
        self.mode = mode
        self.input_grads = bool(input_grads) or plain is None
        self.src_of = None
        if src_of is not None and not takes_src_of:
            raise ValueError(f"src_of belongs to plans of mode 'fanout' or 'decode' (this one is {mode!r})")
        if self.input_grads and with_grads is None:
            raise ValueError("fan-out plans are forward only (input_grads belongs to mode='speaker')")
        creator, flags = with_grads if self.input_grads else plain
        if not hasattr(self.lib, creator):   # (an older library)
            raise RuntimeError(f"the loaded library has no {creator}")
        if lengths == "T_cond":
            if T_cond is None:
                raise ValueError(f"a {mode!r} plan takes the target lengths as T_cond (T is ignored)")
            self.T, self.T_cond = [], [int(t) for t in T_cond]
        elif lengths == "both":
            self.T = [int(t) for t in T]
            self.T_cond = [int(t) for t in (T_cond if T_cond is not None else T)]
            if len(self.T) != len(self.T_cond):
                raise ValueError("T and T_cond must be equally long, non-empty lists")
        else:
            self.T, self.T_cond = [int(t) for t in (T if T is not None else [])], []
        self.B = len(self.T) or len(self.T_cond)
        if takes_src_of:
            self.src_of = [int(j) for j in (src_of if src_of is not None else range(self.B))]
            if not self.src_of or any(not 0 <= j < self.B for j in self.src_of):
                raise ValueError(f"src_of must be a non-empty list of source indices in [0, {self.B}), got {self.src_of}")
        if not self.B:
            raise ValueError("T and T_cond must be equally long, non-empty lists")
        key = str(compute_dtype).lower()
        if key not in ("fp32", "float32", "f32", "bf16", "bfloat16", "bf16r", "bf16_operands"):
            raise ValueError("ragged plans compute in fp32 or bf16 (operand rounding: the pair-storage engine takes uniform shapes)")
        h = ctypes.c_void_p()
        tun = _lib.make_tuning(self.lib, tuning)
        self.N = len(self.src_of) if self.src_of is not None else (0 if mode in ("encode", "encode_pg") else self.B)
        lens = _ints(self.T)
        args = {"avc_plan_create_ragged": (lens, _ints(self.T_cond)), self._EX: (lens, _ints(self.T_cond), flags),
                self._FAN: (lens, self.N, _ints(self.src_of), flags)}.get(creator, (_ints(self.T_cond) if lengths == "T_cond" else lens,))
        # (the *_grads creators take their one list of lengths alone)
        dev = torch.device(device) if device is not None else None
        with (torch.cuda.device(dev) if (dev is not None and dev.type == "cuda") else contextlib.nullcontext()):
            rc = getattr(self.lib, creator)(ctypes.byref(self.cfg), self.B, *args, ctypes.byref(tun), ctypes.byref(h))
        if rc != 0:
            raise RuntimeError(self.lib.avc_last_error().decode())
        self.h = h
        bf = key in ("bf16", "bfloat16", "bf16r", "bf16_operands")
        self.compute_dtype = "bf16r" if bf else "fp32"
        if self.lib.avc_plan_set_compute_dtype(h, 1 if bf else 0) != 0:
            raise RuntimeError(self.lib.avc_last_error().decode())
        self.param_floats = self.lib.avc_plan_param_floats(h)
        self.workspace_floats = self.lib.avc_plan_workspace_floats(h)
        self.num_params, self.param_info = _param_info(self.lib, h)
        self.out_len, self.out_off = [], []
        if mode not in ("speaker", "speaker_pg", "encode", "encode_pg"):
            lens, offs = (ctypes.c_int * self.N)(), (ctypes.c_long * self.N)()
            if self.lib.avc_plan_ragged_out(h, lens, offs) != 0:
                raise RuntimeError(self.lib.avc_last_error().decode())
            self.out_len, self.out_off = list(lens), list(offs)
        self.lat_len, self.lat_off = [], []   # per SOURCE: latent frames and the float offset of its (mu | log_sigma) block in ws["muls"]
        if mode not in ("speaker", "speaker_pg", "decode", "decode_ig", "decode_pg") and hasattr(self.lib, "avc_plan_ragged_latents"):
            lens, offs = (ctypes.c_int * self.B)(), (ctypes.c_long * self.B)()
            if self.lib.avc_plan_ragged_latents(h, lens, offs) != 0:
                raise RuntimeError(self.lib.avc_last_error().decode())
            self.lat_len, self.lat_off = list(lens), list(offs)
        self.n_mels = int(self.cfg.enc.c_in)
        self.c_emb = int(self.cfg.dec.c_cond)
        self.c_lat = int(self.cfg.dec.c_in)

    close = Plan.close
    __del__ = Plan.__del__
    _chk = Plan._chk
    buffer = Plan.buffer

    def _rows(self, t, lens, name):
        if t.dim() != 2 or t.shape[0] != sum(lens) or t.shape[1] != self.n_mels or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous [{sum(lens)}, {self.n_mels}] tensor")

    def forward(self, params, x, x_cond, ws):
        """x / x_cond: the utterances back to back as rows of frames, [sum T, M] contiguous fp32 (x_cond None = x).
        A "speaker" plan reads x_cond only (pass x = None)."""
        if self.mode in ("emb", "fanout"):
            raise RuntimeError(f"an {self.mode!r} plan has no speaker encoder: call forward_emb(params, x, emb, ws)")
        if self.mode in ("decode", "decode_ig", "decode_pg"):
            raise RuntimeError("a 'decode' plan starts from latents: call forward_latents(params, z, zc, emb, ws)")
        if self.mode in ("encode", "encode_pg"):
            if x_cond is not None:
                raise ValueError("an 'encode' plan runs the content encoder alone: forward(params, x, None, ws)")
            self._rows(x, self.T, "x")
        elif self.mode in ("speaker", "speaker_pg"):
            if x_cond is None:
                raise ValueError("a 'speaker' plan reads x_cond: forward(params, None, x_cond, ws)")
            self._rows(x_cond, self.T_cond, "x_cond")
            x = None
        else:
            self._rows(x, self.T, "x")
            if x_cond is not None:
                self._rows(x_cond, self.T_cond, "x_cond")
        with _on(ws):
            self._chk(self.lib.avc_forward_ragged(self.h, _ptr(params), _ptr(x), _ptr(x_cond), _ptr(ws), _stream(ws)))

    def forward_emb(self, params, x, emb, ws):
        """"emb" plans: x as in ``forward``; emb: fp32 [B, c_cond] on the workspace's device, read in place whatever its (non-negative)
        strides -- an ``expand``-ed [1, c_cond] row (batch stride 0) is ONE embedding for all utterances and is never materialised.
        "fanout" plans: x holds each source once, emb is [N, c_cond], one row per output."""
        if self.mode not in ("emb", "fanout"):
            raise RuntimeError(f"forward_emb needs a plan of mode 'emb' or 'fanout' (this one is {self.mode!r}: call "
                               f"{'forward_latents' if self.mode == 'decode' else 'forward'})")
        self._rows(x, self.T, "x")
        emb = self._strided_rows(emb, self.N, "emb", ws)
        with _on(ws):
            self._chk(self.lib.avc_forward_ragged_emb(self.h, _ptr(params), _ptr(x), _ptr(emb), emb.stride(0), emb.stride(1), _ptr(ws), _stream(ws)))

    def _strided_rows(self, t, rows, name, ws):
        """t: fp32 [rows, c_cond] on the workspace's device, read in place through its strides (a copy where one is negative)"""
        if t.dim() != 2 or tuple(t.shape) != (rows, self.c_emb) or t.dtype != torch.float32 or t.device != ws.device:
            raise ValueError(f"{name} must be an fp32 [{rows}, {self.c_emb}] tensor on {ws.device}")
        return t.contiguous() if (t.stride(0) < 0 or t.stride(1) < 0) else t

    def forward_latents(self, params, z, zc, emb, ws):
        """"decode" plans: z holds the S latent blocks back to back, block s = [zc][T[s]] fp32 (frames contiguous) at float offset
        zc * sum(T[:s]); the first c_lat channels of a block are read in place.  zc = c_lat: mu-only blocks; zc = 2 c_lat: the
        ws["muls"] region of a plan with a content encoder over the same sources, passed as it is.  emb: [N, c_cond] as in ``forward_emb``."""
        if self.mode not in ("decode", "decode_ig", "decode_pg"):
            raise RuntimeError(f"forward_latents needs a plan of mode 'decode' (this one is {self.mode!r})")
        z, zc, emb = self._latents(z, zc, emb, ws)
        with _on(ws):
            self._chk(self.lib.avc_decoder_forward_ragged(self.h, _ptr(params), _ptr(z), zc, _ptr(emb), emb.stride(0), emb.stride(1), _ptr(ws),
                                                          _stream(ws)))

    def _latents(self, z, zc, emb, ws):
        zc = int(zc)
        if zc < self.c_lat:
            raise ValueError(f"zc must be at least {self.c_lat} ({self.c_lat}: mu-only blocks; {2 * self.c_lat}: mu | log_sigma blocks), got {zc}")
        _packed(z, zc * sum(self.T), "z", "", ws, at_least=True)
        return z, zc, self._strided_rows(emb, self.N, "emb", ws)

    def backward_decoder(self, params, z, zc, emb, d_dec, ws):
        """``mode="decode_ig"`` plans, after ``forward_latents(params, z, zc, emb, ws)`` in the same workspace: d(loss)/d(z) and
        d(loss)/d(emb) from d_dec = d(loss)/d(dec): fp32, contiguous, n_mels * sum(out_len) elements on the workspace's device, block j =
        [n_mels][out_len[j]] at element n_mels * sum(out_len[:j]) -- the layout of the workspace region ``outputs(ws)`` views.  The results
        are ``d_z(ws)`` and ``d_emb(ws)``.  No parameter gradients; two calls give identical bits."""
        if self.mode not in ("decode_ig", "decode_pg"):
            raise RuntimeError("backward_decoder needs RaggedPlan(mode='decode_ig') "
                               f"(this one: mode={self.mode!r}, input_grads={self.input_grads})")
        z, zc, emb = self._latents(z, zc, emb, ws)
        _packed(d_dec, self.n_mels * sum(self.out_len), "d_dec", " (the layout of the plan's output blocks)", ws)
        with _on(ws):
            self._chk(self.lib.avc_decoder_backward_ragged(self.h, _ptr(params), _ptr(z), zc, _ptr(emb), emb.stride(0), emb.stride(1), _ptr(d_dec),
                                                           _ptr(ws), _stream(ws)))

    def d_z(self, ws):
        """list of [c_lat, T[s]] views of d(loss)/d(z_s) in the workspace (after ``backward_decoder``)"""
        return _blocks(ws, self.buffer("d_z"), self.c_lat, self.T)

    def d_emb(self, ws):
        """[N, c_cond] view of d(loss)/d(emb) in the workspace (after ``backward_decoder``): one row per output, always dense"""
        off = self.buffer("d_emb")
        return ws[off:off + self.N * self.c_emb].view(self.N, self.c_emb)

    def latents(self, ws):
        """(list of mu, list of log_sigma): per SOURCE [c_lat, lat_len[s]] views of the content codes in the workspace (plans that run
        the content encoder; avc_plan_ragged_latents)"""
        if not self.lat_len:
            raise RuntimeError(f"a plan of mode {self.mode!r} has no content codes (or the loaded library has no avc_plan_ragged_latents)")
        both = _blocks(ws, self.lat_off[0], 2 * self.c_lat, self.lat_len)   # (mu rows, then log_sigma rows)
        return [b[:self.c_lat] for b in both], [b[self.c_lat:] for b in both]

    def backward(self, params, x_cond, d_emb, ws):
        """``mode="speaker", input_grads=True`` plans, after ``forward(params, None, x_cond, ws)`` in the same workspace: d(loss)/d(x_cond)
        from d_emb = d(loss)/d(emb), fp32 [B, c_cond] on the workspace's device, read in place whatever its (non-negative) strides (an
        expanded row included).  The result is ``d_x_cond(ws)``.  No parameter gradients; two calls give identical bits."""
        if not (self.mode in ("speaker", "speaker_pg") and self.input_grads):
            raise RuntimeError("backward needs RaggedPlan(mode='speaker', input_grads=True): ragged plans are forward-only otherwise "
                               f"(this one: mode={self.mode!r}, input_grads={self.input_grads})")
        self._rows(x_cond, self.T_cond, "x_cond")
        d_emb = self._strided_rows(d_emb, self.B, "d_emb", ws)
        with _on(ws):
            self._chk(self.lib.avc_backward_ragged(self.h, _ptr(params), _ptr(x_cond), _ptr(d_emb), d_emb.stride(0), d_emb.stride(1), _ptr(ws),
                                                   _stream(ws)))

    def backward_params(self, params, x_cond, d_emb, grads, ws):
        """``mode="speaker_pg"`` plans, after ``forward(params, None, x_cond, ws)`` in the same workspace: ``backward`` plus
        d(loss)/d(parameters) of the speaker encoder, from the same pass.  ``grads``: a flat fp32 buffer of ``param_floats`` elements on the
        workspace's device; the pass overwrites every speaker-encoder tensor in it (weights and biases) and nothing else.
        ``d_x_cond(ws)`` is what ``backward`` leaves there, bit for bit.  fp32 only; two calls give identical bits."""
        if self.mode != "speaker_pg":
            raise RuntimeError("backward_params needs RaggedPlan(mode='speaker_pg') "
                               f"(this one: mode={self.mode!r}, input_grads={self.input_grads})")
        self._rows(x_cond, self.T_cond, "x_cond")
        d_emb = self._strided_rows(d_emb, self.B, "d_emb", ws)
        _packed(grads, self.param_floats, "grads", " (the flat parameter layout)", ws, at_least=True)
        with _on(ws):
            self._chk(self.lib.avc_backward_ragged_params(self.h, _ptr(params), _ptr(x_cond), _ptr(d_emb), d_emb.stride(0), d_emb.stride(1),
                                                          _ptr(grads), _ptr(ws), _stream(ws)))

    def backward_content(self, params, x, d_muls, ws):
        """``mode="encode", input_grads=True`` plans, after ``forward(params, x, None, ws)`` in the same workspace: d(loss)/d(x) from
        d_muls = d(loss)/d(mu | log_sigma): fp32, contiguous, 2 c_lat * sum(lat_len) elements on the workspace's device, block s =
        [2 c_lat][lat_len[s]] (mu rows, then log_sigma rows) at element 2 c_lat * sum(lat_len[:s]) -- the layout of the workspace region
        ``latents(ws)`` views.  The result is ``d_x(ws)``.  No parameter gradients; two calls give identical bits."""
        if not (self.mode in ("encode", "encode_pg") and self.input_grads):
            raise RuntimeError("backward_content needs RaggedPlan(mode='encode', input_grads=True) "
                               f"(this one: mode={self.mode!r}, input_grads={self.input_grads})")
        self._rows(x, self.T, "x")
        _packed(d_muls, 2 * self.c_lat * sum(self.lat_len), "d_muls", " (the layout of the plan's latent blocks)", ws)
        with _on(ws):
            self._chk(self.lib.avc_content_backward_ragged(self.h, _ptr(params), _ptr(x), _ptr(d_muls), _ptr(ws), _stream(ws)))

    def backward_content_params(self, params, x, d_muls, grads, ws):
        """``mode="encode_pg"`` plans, after ``forward(params, x, None, ws)`` in the same workspace: ``backward_content`` plus
        d(loss)/d(parameters) of the content encoder, from the same pass (avc_content_backward_ragged_params).  ``grads``: a flat fp32
        buffer of ``param_floats`` elements on the workspace's device; the pass overwrites every content-encoder tensor in it (weights and
        biases) and nothing else.  ``d_x(ws)`` is what ``backward_content`` leaves there, bit for bit.  fp32 only; two calls give
        identical bits."""
        if self.mode != "encode_pg":
            raise RuntimeError("backward_content_params needs RaggedPlan(mode='encode_pg') "
                               f"(this one: mode={self.mode!r}, input_grads={self.input_grads})")
        self._rows(x, self.T, "x")
        _packed(d_muls, 2 * self.c_lat * sum(self.lat_len), "d_muls", " (the layout of the plan's latent blocks)", ws)
        _packed(grads, self.param_floats, "grads", " (the flat parameter layout)", ws, at_least=True)
        with _on(ws):
            self._chk(self.lib.avc_content_backward_ragged_params(self.h, _ptr(params), _ptr(x), _ptr(d_muls), _ptr(grads), _ptr(ws), _stream(ws)))

    def backward_decoder_params(self, params, z, zc, emb, d_dec, grads, ws):
        """``mode="decode_pg"`` plans, after ``forward_latents(params, z, zc, emb, ws)`` in the same workspace: ``backward_decoder`` plus
        d(loss)/d(parameters) of the decoder, from the same pass (avc_decoder_backward_ragged_params).  z, zc and emb must be the
        forward's: the in_conv's and the AdaIN affine Linears' weight gradients READ them (emb in place through its strides, an expanded
        single voice included).  ``grads`` as for ``backward_content_params``: every decoder tensor is overwritten, nothing else.
        ``d_z(ws)`` and ``d_emb(ws)`` are what ``backward_decoder`` leaves there, bit for bit.  fp32 only; two calls give identical bits."""
        if self.mode != "decode_pg":
            raise RuntimeError("backward_decoder_params needs RaggedPlan(mode='decode_pg') "
                               f"(this one: mode={self.mode!r}, input_grads={self.input_grads})")
        z, zc, emb = self._latents(z, zc, emb, ws)
        _packed(d_dec, self.n_mels * sum(self.out_len), "d_dec", " (the layout of the plan's output blocks)", ws)
        _packed(grads, self.param_floats, "grads", " (the flat parameter layout)", ws, at_least=True)
        with _on(ws):
            self._chk(self.lib.avc_decoder_backward_ragged_params(self.h, _ptr(params), _ptr(z), zc, _ptr(emb), emb.stride(0), emb.stride(1),
                                                                  _ptr(d_dec), _ptr(grads), _ptr(ws), _stream(ws)))

    def d_x(self, ws):
        """[sum T, M] view of d(loss)/d(x) in the workspace (after ``backward_content``): rows of frames, utterance after utterance"""
        off = self.buffer("d_x")
        n = sum(self.T)
        return ws[off:off + n * self.n_mels].view(n, self.n_mels)

    def d_x_cond(self, ws):
        """[sum T_cond, M] view of d(loss)/d(x_cond) in the workspace (after ``backward``): rows of frames, utterance after utterance"""
        off = self.buffer("d_x_cond")
        n = sum(self.T_cond)
        return ws[off:off + n * self.n_mels].view(n, self.n_mels)

    def emb(self, ws):
        """[B, c_cond] view of the speaker embeddings in the workspace ("pairs" and "speaker" plans)"""
        off = self.buffer("emb")
        return ws[off:off + self.B * self.c_emb].view(self.B, self.c_emb)

    def outputs(self, ws):
        """list of [M, out_len[b]] views of the converted utterances in the workspace"""
        return _blocks(ws, self.out_off[0], self.n_mels, self.out_len) if self.out_len else []


class RaggedLossTables:
    """The device tables the loss-side calls of a ragged training step read (avc_reparam_ragged, avc_loss_ragged, avc_latent_bwd_ragged),
    built ONCE per tuple of lengths and kept with the plans: ``T`` frames of every utterance, ``out_len`` / ``out_off`` of the decoder plan
    (avc_plan_ragged_out; the offsets are stored relative to the first block), ``Tz`` latent frames.  int32 (out_off: int64) on ``device``;
    building them is the only host-to-device copy of the loss side."""

    def __init__(self, T, out_len, out_off, Tz, device):
        self.T, self.out_len, self.Tz = [int(t) for t in T], [int(t) for t in out_len], [int(t) for t in Tz]
        self.N = len(self.T)
        if not self.N or len(self.out_len) != self.N or len(self.Tz) != self.N or len(out_off) != self.N:
            raise ValueError("T, out_len, out_off and Tz must be equally long, non-empty lists")
        if any(t < 1 for t in self.T + self.Tz) or any(o < t for o, t in zip(self.out_len, self.T)):
            raise ValueError("every length must be at least 1 and every output block at least as long as its utterance")
        self.out_off = [int(o) - int(out_off[0]) for o in out_off]
        prefix = lambda v: [sum(v[:i]) for i in range(len(v))]
        self.sum_T, self.sum_out, self.sum_Tz = sum(self.T), sum(self.out_len), sum(self.Tz)
        self.T_max, self.Tz_max = max(self.out_len), max(self.Tz)
        ints = torch.tensor(self.T + prefix(self.T) + self.out_len + self.Tz + prefix(self.Tz), dtype=torch.int32).to(device)
        N = self.N
        self.T_dev, self.xoff_dev, self.out_len_dev, self.Tz_dev, self.offz_dev = (ints[i * N:(i + 1) * N] for i in range(5))
        self.out_off_dev = torch.tensor(self.out_off, dtype=torch.int64).to(device)
        self.device = ints.device

    def dec_floats(self, M):
        """floats from the first output block to the end of the last"""
        return self.out_off[-1] + M * self.out_len[-1]


def _rl_check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed: {rc}")


def reparam_ragged(lib, muls, eps, tab, c, z):
    """z = mu + exp(log_sigma / 2) * eps on packed latent blocks (avc_reparam_ragged): muls = the ws["muls"] region of a ragged plan with a
    content encoder (block s = [2 c][Tz_s]), eps / z blocks [c][Tz_s]; eps None: z = mu.  Overwrites z; only enqueues."""
    n = c * tab.sum_Tz
    _packed(muls, 2 * n, "muls", " (mu | log_sigma blocks)", muls, at_least=True)
    _packed(z, n, "z", "", muls, at_least=True)
    if eps is not None:
        _packed(eps, n, "eps", " (one value per latent element)", muls)
    with _on(muls):
        _rl_check(lib.avc_reparam_ragged(_ptr(muls), _ptr(eps), tab.N, _ptr(tab.Tz_dev), _ptr(tab.offz_dev), tab.Tz_max, c, _ptr(z), _stream(muls)),
                  "avc_reparam_ragged")


def loss_ragged_ws_floats(lib, tab):
    n = lib.avc_loss_ragged_ws_floats(tab.N, tab.T_max)
    if n < 0:
        raise RuntimeError("avc_loss_ragged_ws_floats: bad counts")
    return n


def loss_ragged(lib, dec, x, muls, tab, M, c, lambda_rec, d_dec, losses, ws, n_rec=None, n_kl=None):
    """L1 + KL loss of a ragged step and d(lambda_rec * loss_rec)/d(dec) (avc_loss_ragged): dec = the output region of the decoder plan
    (block j = [M][out_len_j]), x = the packed [sum T, M] rows, muls as in ``reparam_ragged``.  Overwrites d_dec (every element of every
    block: the crop tail gets zeros), losses[0:2] = (loss_rec, loss_kl) and ws (``loss_ragged_ws_floats``); only enqueues.
    n_rec / n_kl: the normalisers of the two means, default the counts of THESE rows (M sum T, c sum Tz); a data-parallel rank passes the
    counts of all ranks' rows and gets its share of the global means, which then add up over the ranks."""
    nd = tab.dec_floats(M)
    _packed(dec, nd, "dec", " (the layout of the decoder plan's output blocks)", dec, at_least=True)
    _packed(d_dec, nd, "d_dec", " (the layout of the decoder plan's output blocks)", dec, at_least=True)
    _packed(x, tab.sum_T * M, "x", " (the packed rows)", dec)
    _packed(muls, 2 * c * tab.sum_Tz, "muls", " (mu | log_sigma blocks)", dec, at_least=True)
    _packed(losses, 2, "losses", "", dec, at_least=True)
    _packed(ws, loss_ragged_ws_floats(lib, tab), "ws", "", dec, at_least=True)
    with _on(dec):
        _rl_check(lib.avc_loss_ragged(_ptr(dec), _ptr(tab.out_len_dev), _ptr(tab.out_off_dev), _ptr(x), _ptr(tab.T_dev), _ptr(tab.xoff_dev), tab.N, M,
                                      tab.T_max, _ptr(muls), _ptr(tab.Tz_dev), _ptr(tab.offz_dev), c, int(tab.sum_T * M if n_rec is None else n_rec),
                                      int(tab.sum_Tz * c if n_kl is None else n_kl),
                                      float(lambda_rec), _ptr(d_dec), _ptr(losses), _ptr(ws), _stream(dec)), "avc_loss_ragged")


def latent_bwd_ragged(lib, muls, eps, d_z, tab, c, lambda_kl_over_n, d_muls):
    """d(loss)/d(mu | log_sigma) from the KL term and from d_z (avc_latent_bwd_ragged); eps None: the z = mu step.  Overwrites d_muls (the
    layout of muls); only enqueues."""
    n = c * tab.sum_Tz
    _packed(muls, 2 * n, "muls", " (mu | log_sigma blocks)", muls, at_least=True)
    _packed(d_z, n, "d_z", "", muls, at_least=True)
    _packed(d_muls, 2 * n, "d_muls", " (the layout of muls)", muls, at_least=True)
    if eps is not None:
        _packed(eps, n, "eps", " (one value per latent element)", muls)
    with _on(muls):
        _rl_check(lib.avc_latent_bwd_ragged(_ptr(muls), _ptr(eps), _ptr(d_z), tab.N, _ptr(tab.Tz_dev), _ptr(tab.offz_dev), tab.Tz_max, c,
                                            float(lambda_kl_over_n), _ptr(d_muls), _stream(muls)), "avc_latent_bwd_ragged")
