"""Training driver with the reference's surface (solver.py:16-118): ``Solver(config,
args)``, ``ae_step(data, lambda_kl)``, ``train(n)``, ``save_model`` /
``load_model`` with the same ``<path>.ckpt`` / ``<path>.opt`` files.

``ae_step`` is ONE engine pass: forward, L1+KL loss, backward, (RCCL all-reduce
of the flat gradient buffer when torch.distributed is initialised), fused
clip+Adam — no torch op on the hot path and no host sync unless the caller asks
for Python floats.
"""
import os

import torch
import yaml

from .data_utils import PickleDataset, get_data_loader
from .model import AE
from .optim import FusedClipAdam
from .utils import Logger, cc, infinite_iter, local_device


def _dist():
    import torch.distributed as dist
    return dist if (dist.is_available() and dist.is_initialized()) else None


class Solver(object):
    def __init__(self, config, args, lib=None):
        self.config = config
        self.args = args
        self._lib = lib
        self.logger = Logger(getattr(args, "logdir", "./log"))
        if getattr(args, "data_dir", None):
            self.get_data_loaders()
        self.build_model()
        if getattr(args, "store_model_path", None):
            self.save_config()
        if getattr(args, "load_model", False):
            self.load_model()

    # ---- checkpoints (solver.py:39-55) ---------------------------------------
    # The reference is single-process.  Under data parallelism the replicas are identical, so only rank 0
    # writes -- to a temporary file that is renamed into place (a reader never sees a truncated
    # checkpoint) -- and every rank waits for it.
    @staticmethod
    def _rank():
        d = _dist()
        return d.get_rank() if d is not None else 0

    @staticmethod
    def _atomic_save(obj, path):
        tmp = f"{path}.tmp.{os.getpid()}"
        torch.save(obj, tmp)
        os.replace(tmp, path)

    def save_model(self, iteration=None):
        if self._rank() == 0:
            self._atomic_save(self.model.state_dict(), f"{self.args.store_model_path}.ckpt")
            self._atomic_save(self.opt.state_dict(), f"{self.args.store_model_path}.opt")
        d = _dist()
        if d is not None and d.get_world_size() > 1:
            d.barrier()

    def save_config(self):
        if self._rank() != 0:
            return
        for suffix, obj in ((".config.yaml", self.config), (".args.yaml", vars(self.args))):
            path = f"{self.args.store_model_path}{suffix}"
            tmp = f"{path}.tmp.{os.getpid()}"
            with open(tmp, "w") as f:
                yaml.dump(obj, f)
            os.replace(tmp, path)

    def load_model(self):
        """solver.py:50-54 loads the model AND the optimizer state, unconditionally: a missing ``.opt`` raises, as it does there.
        ``args.load_opt = False`` opts out (a bare ``.ckpt`` such as the published vctk_model.ckpt: fresh optimizer state)."""
        dev = self.model.flat_parameters().device
        self.model.load_state_dict(torch.load(f"{self.args.load_model_path}.ckpt", map_location=dev))
        if getattr(self.args, "load_opt", True):
            self.opt.load_state_dict(torch.load(f"{self.args.load_model_path}.opt", map_location=dev))

    # ---- data (solver.py:57-68) ----------------------------------------------
    def get_data_loaders(self):
        d = self.args.data_dir
        if getattr(self.args, "ragged_feed", False):
            from .device_feed import RaggedUtteranceFeed
            rank, world = 0, 1
            dd = _dist()
            if dd is not None:
                rank, world = dd.get_rank(), dd.get_world_size()
            dev = local_device() if self._lib is None else torch.device("cpu")   # (an injected library: the CPU simulation of the tests)
            self.ragged_iter = RaggedUtteranceFeed.from_files(
                os.path.join(d, f"{self.args.train_set}.pkl"), self.config["data_loader"]["batch_size"], dev,
                n_templates=getattr(self.args, "ragged_templates", 8), min_frames=getattr(self.args, "ragged_min_frames", 17),
                max_frames=getattr(self.args, "ragged_max_frames", None), seed=0, rank=rank, world_size=world,   # ONE stream of draws, shared
                lib=self._lib)
            return
        if getattr(self.args, "device_feed", False):
            from .device_feed import DeviceSegmentFeed
            rank, world = 0, 1
            dd = _dist()
            if dd is not None:
                rank, world = dd.get_rank(), dd.get_world_size()
            self.train_iter = DeviceSegmentFeed.from_files(
                os.path.join(d, f"{self.args.train_set}.pkl"), os.path.join(d, self.args.train_index_file),
                self.config["data_loader"]["segment_size"], self.config["data_loader"]["batch_size"], local_device(),
                shuffle=self.config["data_loader"]["shuffle"], seed=0, rank=rank, world_size=world,   # disjoint shards of ONE permutation
                lib=self._lib)
            return
        self.train_dataset = PickleDataset(os.path.join(d, f"{self.args.train_set}.pkl"),
                                           os.path.join(d, self.args.train_index_file),
                                           segment_size=self.config["data_loader"]["segment_size"])
        self.train_loader = get_data_loader(self.train_dataset, frame_size=self.config["data_loader"]["frame_size"],
                                            batch_size=self.config["data_loader"]["batch_size"],
                                            shuffle=self.config["data_loader"]["shuffle"], num_workers=4, drop_last=False)
        self.train_iter = infinite_iter(self.train_loader)

    # ---- model + optimizer (solver.py:70-79) -----------------------------------
    def build_model(self):
        if self.config["data_loader"].get("frame_size", 1) != 1:
            raise NotImplementedError("data_loader.frame_size != 1")
        tuning = getattr(self.args, "tuning", None)
        self.model = cc(AE(self.config, lib=self._lib, tuning=tuning)) if self._lib is None else AE(self.config, lib=self._lib, tuning=tuning)
        o = self.config["optimizer"]
        self.opt = FusedClipAdam(self.model, lr=o["lr"], betas=(o["beta1"], o["beta2"]), amsgrad=o["amsgrad"],
                                 weight_decay=o["weight_decay"], lib=self._lib)
        d = _dist()
        if d is not None and d.get_world_size() > 1:  # identical replicas: rank 0's init wins
            d.broadcast(self.model.flat_parameters(), src=0)
            self.model.weights_changed()   # (a collective writes the flat buffer without touching the views' version counters)
        # reparameterisation noise (model.py:383): every rank draws from its OWN generator stream
        self._eps_gen = None
        self._comm_stream = None
        self._wire = None   # persistent bf16 gradient bucket (allreduce_dtype: bf16)
        self.measure_allreduce = False
        self._ar_events = []

    # ---- one training step (solver.py:81-97) -------------------------------------
    def _eps_generator(self, device):
        if self._eps_gen is None or self._eps_gen.device != device:
            self._eps_gen = torch.Generator(device=device)
            self._eps_gen.manual_seed(torch.initial_seed() + 7919 * self._rank())
        return self._eps_gen

    def _draw_eps(self, B, C, Tb, device):
        return torch.randn(B, C, Tb, device=device, dtype=torch.float32, generator=self._eps_generator(device))

    def _allreduce_grads(self, d, plan, grads):
        """SUM over ranks of the flat gradient buffer (RCCL over xGMI when the backend is "nccl"); the 1/W of the
        mean is folded into the optimizer kernel.  Three buckets in the order avc_backward finishes them: the decoder's range
        and the speaker encoder's range are reduced on a communication stream under the rest of the backward pass
        (avc_plan_stream_wait_grads), the content encoder's range once the whole backward is done."""
        from . import _lib
        # compute_dtype bf16 (BASELINE configs[2]: "bf16 compute, fp32 master and optimizer state"): the bucket travels as
        # bf16 too -- 9.8 MB instead of 19.6 MB per step over xGMI; `allreduce_dtype: fp32` in the config keeps
        # the wire fp32.  The sum of W bf16-rounded gradients carries a relative error of ~2^-9 per element, the same order as
        # the bf16 matrix products that produced them.
        wire_bf16 = self.config.get("allreduce_dtype", "bf16" if str(self.config.get("compute_dtype", "fp32")).lower() .startswith(("bf16", "bfloat16")) else "fp32") == "bf16"

        def reduce(seg, wire):
            if wire is None:
                d.all_reduce(seg)
                return
            wire.copy_(seg)            # persistent bf16 bucket: no per-step allocation
            d.all_reduce(wire)
            seg.copy_(wire)
        parts = [plan.param_range(k) for k in (_lib.GRADS_DECODER, _lib.GRADS_SPEAKER, _lib.GRADS_CONTENT)]
        # `allreduce_buckets` (config; default 3): 3 = decoder | speaker encoder | content encoder, the first two under the backward pass;
        # 2 = decoder under the backward pass, the two encoders (one contiguous range: the head of the flat buffer) after it -- one
        # collective launch fewer on a step this short; 1 = the whole buffer after the backward pass (no overlap)
        nb = int(self.config.get("allreduce_buckets", 3))
        early = [(_lib.GRADS_DECODER, parts[0]), (_lib.GRADS_SPEAKER, parts[1])]
        late = [parts[2]]
        if nb <= 2:
            lo = min(parts[1][0], parts[2][0])
            hi = max(parts[1][0] + parts[1][1], parts[2][0] + parts[2][1])
            if hi - lo != parts[1][1] + parts[2][1]:   # (the two encoders are not adjacent in this plan: keep them apart)
                late = [parts[1], parts[2]]
            else:
                late = [(lo, hi - lo)]
            early = early[:1]
        if nb <= 1:
            early, late = [], [(0, grads.numel())]
        wire = None
        if wire_bf16:
            if self._wire is None or self._wire.device != grads.device or self._wire.numel() != grads.numel():
                self._wire = torch.empty(grads.numel(), dtype=torch.bfloat16, device=grads.device)
            wire = self._wire
        w = (lambda o, n: wire[o:o + n]) if wire is not None else (lambda o, n: None)
        if not grads.is_cuda:
            for _, (o, n) in early:
                reduce(grads[o:o + n], w(o, n))
            for (o, n) in late:
                reduce(grads[o:o + n], w(o, n))
            return
        if self._comm_stream is None or self._comm_stream.device != grads.device:
            self._comm_stream = torch.cuda.Stream(device=grads.device)
        cs, main = self._comm_stream, torch.cuda.current_stream(grads.device)
        # Buckets in the order the backward pass finishes them (avc_backward: decoder -> speaker encoder's branch -> content encoder's
        # longer branch): the early ones are reduced on the communication stream UNDER the rest of the backward, only the late one(s)
        # start after it.
        for k, (o, n) in early:
            if not plan.stream_wait_grads(k, cs):
                cs.wait_stream(main)               # a plan without helper streams / events: order behind the whole backward
            with torch.cuda.stream(cs):
                reduce(grads[o:o + n], w(o, n))
        cs.wait_stream(main)                       # the whole backward (avc_backward joins its helper streams into main)
        with torch.cuda.stream(cs):
            for (o, n) in late:
                reduce(grads[o:o + n], w(o, n))
        # the time the compute stream WAITS here is the all-reduce the schedule could not hide: measured when asked for
        # (Solver.measure_allreduce = True; bench.py --gpus N reports the mean as config.exposed_allreduce_ms)
        if getattr(self, "measure_allreduce", False):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(main)
            main.wait_stream(cs)
            e1.record(main)
            self._ar_events.append((e0, e1))
        else:
            main.wait_stream(cs)

    def exposed_allreduce_ms(self, last=None):
        """Mean time per step the compute stream waited for the gradient all-reduce (needs measure_allreduce = True; synchronises)."""
        ev = self._ar_events[-last:] if last else self._ar_events
        if not ev:
            return None
        torch.cuda.synchronize()
        return sum(a.elapsed_time(b) for a, b in ev) / len(ev)

    def ae_step(self, data, lambda_kl, eps=None, sync=True):
        model = self.model
        flat = model.flat_parameters()
        x = data if data.device == flat.device else data.to(flat.device, non_blocking=True)
        if x.dtype != torch.float32:
            x = x.float()
        B, _, T = x.shape
        plan, ws = model._plan(B, T, T, x.device)
        if eps is None:
            eps = self._draw_eps(B, model._c_lat, plan.latent_len, x.device)  # model.py:383
        grads = model.flat_grads()
        # the weight images in `ws` are current iff the last thing that touched the parameters was OUR optimizer step followed by
        # pack_weights into this very workspace: torch's version counters (of the flat buffer and of every parameter view) see every
        # other in-place change -- load_state_dict, a torch optimizer, user code.  (In-place edits through `.data` bypass the counters,
        # as they bypass autograd's own checks: call AE.weights_changed() after those.)
        # Fail-safe side: the promise is made ONLY here, behind our own optimizer step + pack_weights, and AE voids it on _alias /
        # _apply / load_state_dict / weights_changed(); `repack_every_step: true` in the config gives it up altogether, and
        # `verify_packed_weights: true` (debug: one host sync per step) compares a checksum of the parameters with the one taken when
        # the images were packed and raises on a silent edit.
        pk = getattr(self, "_packed", None)
        packed = (pk is not None and pk[0] is plan and pk[1] is ws and pk[2] is flat and pk[3] == model.weights_version()
                  and not self.config.get("repack_every_step", False))
        if packed and self.config.get("verify_packed_weights", False):
            if self._param_fingerprint(flat) != pk[4]:
                raise RuntimeError("the parameters changed behind the version counters since the weight images were packed "
                                   "(in-place edit through .data, a foreign kernel, a collective): call AE.weights_changed() after such writes")
        plan.forward(flat, x, None, eps, ws, weights_packed=packed)
        plan.loss(x, self.config["lambda"]["lambda_rec"], ws)
        plan.backward(flat, x, None, eps, grads, ws, lambda_kl=float(lambda_kl))
        prescale = 1.0
        d = _dist()
        if d is not None and (d.get_world_size() > 1 or self.config.get("allreduce_world1", False)):
            # (world_size 1: nothing to reduce -- and no bf16 round trip of the gradients; `allreduce_world1: true` keeps the
            # collective path for tests that exercise it with one rank)
            self._allreduce_grads(d, plan, grads)
            prescale = 1.0 / d.get_world_size()
        gnorm = self.opt.step(self.config["optimizer"]["grad_norm"], grad_prescale=prescale)
        plan.pack_weights(flat, ws)    # the next step opens with its first convolution (engine.Plan.forward, weights_packed)
        self._packed = (plan, ws, flat, model.weights_version(),
                        self._param_fingerprint(flat) if self.config.get("verify_packed_weights", False) else None)
        losses = plan.view(ws, "losses", (2,))
        if not sync:
            return {"loss_rec": losses[0], "loss_kl": losses[1], "grad_norm": gnorm[0]}
        vals = torch.cat([losses, gnorm]).tolist()  # one D2H sync (the reference does .item() x2, solver.py:94-95)
        return {"loss_rec": vals[0], "loss_kl": vals[1], "grad_norm": vals[2]}

    # ---- one training step over whole utterances of different lengths ----------------
    def _rag_buf(self, name, n, device):
        """the first n floats of a buffer this Solver owns; it grows on demand and is reused from step to step"""
        bufs = self.__dict__.setdefault("_rag_bufs", {})
        b = bufs.get(name)
        if b is None or b.device != device or b.numel() < n:
            b = bufs[name] = torch.empty(int(n * 1.25) + 64, dtype=torch.float32, device=device)
        return b[:n]

    def _rag_state(self, T):
        """(three grad plans with the workspaces this step runs in, RaggedLossTables) of a tuple of lengths.  The plans are the AE's
        ("encode_pg", "speaker_pg", "decode_pg" of AE._ragged_plan: the ones the ragged autograd functions use); a workspace that still holds
        the activations of a pending autograd backward is left alone and the step runs in a private one, as _PartFunction._attach does."""
        from .engine import RaggedLossTables
        model = self.model
        dev = model.flat_parameters().device
        pe, ee = model._ragged_plan("encode_pg", T, ())
        ps, es = model._ragged_plan("speaker_pg", (), T)
        Tz = tuple(pe.lat_len)
        pd, ed = model._ragged_plan("decode_pg", Tz, ())
        wss = [e.ws if not e.busy() else torch.zeros(p.workspace_floats, dtype=torch.float32, device=dev) for p, e in ((pe, ee), (ps, es), (pd, ed))]
        tabs = self.__dict__.setdefault("_rag_tables", {})
        key = (T, str(dev))
        tab = tabs.pop(key, None)
        if tab is None:
            tab = RaggedLossTables(T, pd.out_len, pd.out_off, Tz, dev)
        tabs[key] = tab   # most recently used last
        while len(tabs) > getattr(self, "_rag_tables_cap", 4):
            tabs.pop(next(iter(tabs)))
        return (pe, ps, pd), wss, tab

    def _latent_frames(self, T):
        """latent frames of an utterance of T frames: the content encoder halves (rounding up) at every block that subsamples -- the
        ``lat_len`` of a content plan, computed on the host for lengths this rank holds no plan of (the other ranks' utterances)"""
        ce = self.config["ContentEncoder"]
        for s in ce["subsample"][:ce["n_conv_blocks"]]:
            if s > 1:
                T = -(-T // s)
        return T

    def _packed_rows(self, batch):
        """the checks ``AE._ragged_rows`` makes, on a batch that is packed already: (T, x) with x used in place"""
        model = self.model
        x, T = batch.x, batch.T
        M, dev = model._n_mels, model.flat_parameters().device
        if not T or any(t < 1 for t in T) or any(t < 1 for t in batch.global_T):
            raise ValueError("ae_step_ragged: a PackedUtterances needs at least one utterance and lengths of at least 1")
        if not torch.is_tensor(x) or x.dim() != 2 or x.shape[1] != M or x.shape[0] != sum(T):
            raise ValueError(f"ae_step_ragged: PackedUtterances.x must be the packed [sum T, {M}] = [{sum(T)}, {M}] rows (frames as rows), got "
                             f"{tuple(x.shape) if torch.is_tensor(x) else type(x).__name__}")
        if x.dtype != torch.float32 or not x.is_contiguous():
            raise ValueError(f"ae_step_ragged: PackedUtterances.x must be contiguous fp32, got {x.dtype}, strides {tuple(x.stride())}")
        if x.device != dev:
            raise RuntimeError(f"ae_step_ragged: PackedUtterances.x on {x.device} but parameters on {dev}")
        return T, x

    def _allreduce_ragged(self, d, grads, losses):
        """SUM over ranks of the flat gradient buffer, ONE bucket behind the whole backward (every rank divided by the global counts, so the
        sum IS the global-mean gradient: no 1/W anywhere), in the wire format of ``allreduce_dtype``; then of the two loss floats (always
        fp32: they are reported, not stepped on)."""
        if self.config.get("allreduce_dtype", "fp32") == "bf16":
            if self._wire is None or self._wire.device != grads.device or self._wire.numel() != grads.numel():
                self._wire = torch.empty(grads.numel(), dtype=torch.bfloat16, device=grads.device)
            self._wire.copy_(grads)
            d.all_reduce(self._wire)
            grads.copy_(self._wire)
        else:
            d.all_reduce(grads)
        d.all_reduce(losses)

    def ae_step_ragged(self, utts, lambda_kl, eps=None, sync=True, apply=True):
        """``ae_step`` over whole utterances of DIFFERENT lengths: ``utts`` is a list of [T_j, M] tensors (frames as rows, what
        ``AE.inference_ragged`` takes); every utterance is both content source and speaker reference, as ``model(x)`` in the reference's
        ae_step (solver.py:83, model.py:376-385).  The loss is the reference's on the packed rows: mean |dec[:, :T_j] - x_j| over all kept
        elements, 0.5 mean(exp(ls) + mu^2 - 1 - ls) over all latent elements, z = mu + exp(ls / 2) * eps.

        One pass through the three ragged grad plans ("encode_pg", "speaker_pg", "decode_pg") with the packed-row loss kernels between them
        (avc_reparam_ragged, avc_loss_ragged, avc_latent_bwd_ragged).  The three backward passes write their networks' ranges of
        ``model.flat_grads()`` directly -- together the whole buffer -- and the fused clip+Adam kernel reads it from there: no temporary
        gradient buffer, no ``.grad`` accumulation, no copy of a workspace region.  z, eps, d_dec, d_muls, the loss workspace and the
        length tables belong to this Solver, grow on demand and are reused.

        eps: None draws c_lat * sum(Tz) values from this rank's own generator (as ``ae_step``); a tensor of that many fp32 elements (block j
        = [c_lat][Tz_j], back to back) is used as given; False: no noise (z = mu).  apply=False stops before the optimizer: parameters and
        optimizer state stay untouched, the gradients stay in ``model.flat_grads()`` and no "grad_norm" is returned.  sync=False returns
        device scalars without waiting.  fp32 only (``compute_dtype`` bf16 is refused); a list is for one process only: a world size above
        1 is refused (the per-rank means over packed rows do not average to the global mean).

        ``utts`` may also be the ``PackedUtterances`` of a ``RaggedUtteranceFeed``: its ``x`` is used in place (no ``torch.cat``), and the
        two means are taken over ``global_T``, the lengths of ALL ranks' utterances: n_rec = M sum(global_T) and n_kl = c sum(Tz) go to the
        loss kernels in place of this rank's counts, so every rank computes its exact share of the global-mean gradient.  Any world size
        is accepted: the flat gradient buffer is summed over the ranks behind the three backward passes (one bucket, the wire format of
        ``allreduce_dtype``, no 1/W in the optimizer), and so are the two losses -- every rank returns the global means.  With one
        process and global_T == T the gradients are bit-equal to the list call's on the same rows."""
        from .engine import latent_bwd_ragged, loss_ragged, loss_ragged_ws_floats, reparam_ragged
        model = self.model
        if str(model.compute_dtype).lower().startswith(("bf16", "bfloat16")):
            raise RuntimeError(f"ae_step_ragged: the ragged gradient passes are fp32 only, and compute_dtype is {model.compute_dtype!r}; "
                               "train on equal-length segments with ae_step")
        from .device_feed import PackedUtterances
        d = _dist()
        packed = isinstance(utts, PackedUtterances)
        if packed:
            T, x = self._packed_rows(utts)
        else:
            if d is not None and d.get_world_size() > 1:
                raise RuntimeError(f"ae_step_ragged: one process only (world size {d.get_world_size()}) for a list of utterances: the means over "
                                   "each rank's packed rows do not average to the mean over all ranks' rows; pass the PackedUtterances of a "
                                   "RaggedUtteranceFeed (they carry all ranks' lengths), or train on equal-length segments with ae_step")
            utts = list(utts)
            if not utts:
                raise ValueError("ae_step_ragged: an empty list of utterances")
            T, x = model._ragged_rows(utts, "utts")
        flat, grads = model.flat_parameters(), model.flat_grads()
        dev = flat.device
        (pe, ps, pd), (wse, wss, wsd), tab = self._rag_state(T)
        lib, c, M = pe.lib, pe.c_lat, pe.n_mels
        n_lat = c * tab.sum_Tz
        n_rec, n_kl = M * tab.sum_T, n_lat   # the normalisers of the two means: the counts of all ranks' rows
        if packed:
            if [self._latent_frames(t) for t in T] != list(tab.Tz):
                raise RuntimeError("ae_step_ragged: the host rule for latent lengths disagrees with the content plan's")
            n_rec, n_kl = M * sum(utts.global_T), c * sum(self._latent_frames(t) for t in utts.global_T)
        if eps is None:
            eps = self._rag_buf("eps", n_lat, dev).normal_(generator=self._eps_generator(dev))   # model.py:383
        elif eps is False:
            eps = None
        else:
            if not torch.is_tensor(eps) or eps.numel() != n_lat or eps.dtype != torch.float32:
                raise ValueError(f"ae_step_ragged: eps must be an fp32 tensor of {n_lat} elements (block j = [{c}][Tz_j], Tz = {tab.Tz}), "
                                 "None (draw it) or False (no noise)")
            eps = eps.to(dev).contiguous().view(-1)
        pe.forward(flat, x, None, wse)
        ps.forward(flat, None, x, wss)
        muls = wse[pe.lat_off[0]:pe.lat_off[0] + 2 * n_lat]
        z = self._rag_buf("z", n_lat, dev)
        reparam_ragged(lib, muls, eps, tab, c, z)
        emb = ps.emb(wss)   # read in place from the speaker plan's workspace
        pd.forward_latents(flat, z, c, emb, wsd)
        n_dec = M * tab.sum_out
        dec = wsd[pd.out_off[0]:pd.out_off[0] + n_dec]
        d_dec, losses = self._rag_buf("d_dec", n_dec, dev), self._rag_buf("losses", 2, dev)
        loss_ragged(lib, dec, x, muls, tab, M, c, self.config["lambda"]["lambda_rec"], d_dec, losses,
                    self._rag_buf("loss_ws", loss_ragged_ws_floats(lib, tab), dev), n_rec=n_rec, n_kl=n_kl)
        pd.backward_decoder_params(flat, z, c, emb, d_dec, grads, wsd)
        o = pd.buffer("d_z")
        d_muls = self._rag_buf("d_muls", 2 * n_lat, dev)
        latent_bwd_ragged(lib, muls, eps, wsd[o:o + n_lat], tab, c, float(lambda_kl) / n_kl, d_muls)
        pe.backward_content_params(flat, x, d_muls, grads, wse)
        ps.backward_params(flat, x, pd.d_emb(wsd), grads, wss)
        self._rag_last = ((pe, ps, pd), (wse, wss, wsd), tab)   # (the workspaces of the last step: saved rows, dec)
        if packed and d is not None and (d.get_world_size() > 1 or self.config.get("allreduce_world1", False)):
            self._allreduce_ragged(d, grads, losses)
        if not apply:
            if not sync:
                return {"loss_rec": losses[0], "loss_kl": losses[1]}
            vals = losses.tolist()   # one D2H sync
            return {"loss_rec": vals[0], "loss_kl": vals[1]}
        gnorm = self.opt.step(self.config["optimizer"]["grad_norm"])
        model.weights_changed()   # (the kernel writes the flat buffer behind torch's version counters: ae_step's packed weight images are stale)
        if not sync:
            return {"loss_rec": losses[0], "loss_kl": losses[1], "grad_norm": gnorm[0]}
        vals = torch.cat([losses, gnorm]).tolist()  # one D2H sync
        return {"loss_rec": vals[0], "loss_kl": vals[1], "grad_norm": vals[2]}

    @staticmethod
    def _param_fingerprint(flat):
        """Position-dependent fingerprint of the flat parameter buffer (`verify_packed_weights`): the BITS of every element, multiplied by an odd
        per-position weight, summed modulo 2^64.  A plain sum misses sum-preserving edits -- two swapped weights, a permuted row."""
        bits = flat.view(torch.int32).to(torch.int64)
        pos = torch.arange(bits.numel(), device=bits.device, dtype=torch.int64)
        return int(((bits + 0x9E3779B9) * (2 * pos + 1)).sum().item())

    def kl_weight(self, iteration):
        """solver.py:101-104 linear annealing."""
        lam = self.config["lambda"]["lambda_kl"]
        if iteration >= self.config["annealing_iters"]:
            return lam
        return lam * (iteration + 1) / self.config["annealing_iters"]

    def train(self, n_iterations):
        for iteration in range(n_iterations):
            lambda_kl = self.kl_weight(iteration)
            data = next(self.train_iter)
            meta = self.ae_step(data, lambda_kl)
            if iteration % self.args.summary_steps == 0:
                self.logger.scalars_summary(f"{self.args.tag}/ae_train", meta, iteration)
            print(f"AE:[{iteration + 1}/{n_iterations}], loss_rec={meta['loss_rec']:.2f}, "
                  f"loss_kl={meta['loss_kl']:.2f}, lambda={lambda_kl:.1e}     ", end="\r")
            if (iteration + 1) % self.args.save_steps == 0 or iteration + 1 == n_iterations:
                self.save_model(iteration=iteration)
                print()

    def train_ragged(self, n_iterations):
        """``train`` on whole utterances: batches from ``self.ragged_iter`` (a ``RaggedUtteranceFeed``; ``--ragged_feed``), steps by
        ``ae_step_ragged``.  The feed repeats K tuples of lengths, and the step keeps three grad plans with their workspaces and one
        table set per tuple: the model's ragged plan cache is raised to 3 K + 1 and this solver's table cache to K, so that after each
        template's first visit nothing is created any more."""
        feed = self.ragged_iter
        K = int(feed.n_templates)
        self.model.set_ragged_plan_cache(max(self.model._ragged_cap, 3 * K + 1))
        self._rag_tables_cap = max(getattr(self, "_rag_tables_cap", 4), K)
        for iteration in range(n_iterations):
            lambda_kl = self.kl_weight(iteration)
            meta = self.ae_step_ragged(next(feed), lambda_kl)
            if iteration % self.args.summary_steps == 0:
                self.logger.scalars_summary(f"{self.args.tag}/ae_train", meta, iteration)
            print(f"AE:[{iteration + 1}/{n_iterations}], loss_rec={meta['loss_rec']:.2f}, "
                  f"loss_kl={meta['loss_kl']:.2f}, lambda={lambda_kl:.1e}     ", end="\r")
            if (iteration + 1) % self.args.save_steps == 0 or iteration + 1 == n_iterations:
                self.save_model(iteration=iteration)
                print()
