"""Device-resident segment feed.

The reference slices 128-frame segments out of a pickled ``{utt: [T, M]}`` dict in 4 DataLoader
worker processes and copies every batch host->device (data_utils.py:43-57, solver.py:57-68,82).
At >3e4 segments/s that feed is the bottleneck, while a whole normalised mel corpus fits the
288 GB of one MI355X many times over.  ``DeviceSegmentFeed`` uploads the corpus once as one
``[sum_T, M]`` tensor; a batch is ONE launch of the library's gather kernel
(``avc_gather_segments``, csrc/rowops.hip): it reads the B x T corpus rows coalesced along the mel axis and
writes the ``[B, M, T]`` tensor with the time axis contiguous -- the values ``CollateFn`` produces
(data_utils.py:14-22), in the layout every first-layer loader of the engine reads with unit stride (the
reference's collate result is a transposed *view*, strides (T*M, 1, M); the engine accepts both).

Data parallelism: all ranks draw the SAME permutation per epoch (same seed) and rank r takes elements
r, r+W, r+2W, ... of it, so the shards are disjoint and of equal size (the < W left-over samples of an
epoch are dropped; every rank must run the same number of steps for the gradient all-reduce).

``RaggedUtteranceFeed`` is the same corpus for the step over WHOLE utterances of different lengths (``Solver.ae_step_ragged``): a batch
is ONE launch of ``avc_gather_utterances`` (csrc/ragged_feed.hip) into the frame-major packed rows the ragged plans read, handed over as
a ``PackedUtterances``.
"""
import ctypes
import json
import pickle

import numpy as np
import torch

from . import _lib


class DeviceSegmentFeed:
    def __init__(self, data, indexes, segment_size, batch_size, device, shuffle=True, seed=0, rank=0, world_size=1, lib=None):
        """data: {utt_id: float32 [T, M]}; indexes: [[utt_id, t], ...] (the reference's sample index JSON)."""
        self.segment_size, self.batch_size, self.shuffle = int(segment_size), int(batch_size), shuffle
        self.rank, self.world = int(rank), int(world_size)
        if not (0 <= self.rank < self.world):
            raise ValueError("rank must be in [0, world_size)")
        self.lib = lib if lib is not None else _lib.load()
        offs, chunks, pos = {}, [], 0
        for k, v in data.items():
            v = np.asarray(v, dtype=np.float32)
            offs[k] = pos
            pos += v.shape[0]
            chunks.append(v)
        self.corpus = torch.from_numpy(np.concatenate(chunks, axis=0)).to(device).contiguous()   # [sum_T, M], resident
        self.n_mels = int(self.corpus.shape[1])
        starts = [offs[u] + int(t) for u, t in indexes]
        if any(s + self.segment_size > pos for s in starts):
            raise ValueError("a segment runs past the end of the corpus")
        self.starts = torch.tensor(starts, dtype=torch.long, device=self.corpus.device)
        self.gen = torch.Generator(device="cpu").manual_seed(seed)
        self._perm, self._cursor = None, 0

    @classmethod
    def from_files(cls, pickle_path, sample_index_path, segment_size, batch_size, device, **kw):
        with open(pickle_path, "rb") as f:
            data = pickle.load(f)
        with open(sample_index_path, "r") as f:
            indexes = json.load(f)
        return cls(data, indexes, segment_size, batch_size, device, **kw)

    def shard_size(self):
        return self.starts.numel() // self.world if self.world > 1 else self.starts.numel()

    def __len__(self):
        return (self.shard_size() + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        return self

    def _new_epoch(self):
        n = self.starts.numel()
        perm = torch.randperm(n, generator=self.gen) if self.shuffle else torch.arange(n)
        if self.world > 1:
            perm = perm[: (n // self.world) * self.world][self.rank::self.world]
        self._perm = perm.to(self.starts.device)
        self._cursor = 0

    def gather(self, sel):
        """[len(sel), M, T] contiguous batch for the sample indices ``sel`` (a device int64 tensor)."""
        st = self.starts[sel].contiguous()
        B, M, T = int(st.numel()), self.n_mels, self.segment_size
        out = torch.empty(B, M, T, dtype=torch.float32, device=self.corpus.device)
        P = lambda t: ctypes.c_void_p(t.data_ptr())
        cuda = self.corpus.is_cuda
        stream = ctypes.c_void_p(torch.cuda.current_stream(self.corpus.device).cuda_stream) if cuda else None
        with (torch.cuda.device(self.corpus.device) if cuda else _null()):
            rc = self.lib.avc_gather_segments(P(self.corpus), self.corpus.shape[0], M, P(st), B, T, P(out), stream)
        if rc != 0:
            raise RuntimeError(f"avc_gather_segments failed: {rc}")
        return out

    def __next__(self):
        """Infinite iterator (utils.py:28-35 infinite_iter over a shuffling DataLoader); the last batch of an
        epoch may be short (drop_last is ignored by the reference, data_utils.py:24-27)."""
        if self._perm is None or self._cursor >= self._perm.numel():
            self._new_epoch()
        sel = self._perm[self._cursor:self._cursor + self.batch_size]
        self._cursor += self.batch_size
        return self.gather(sel)


class PackedUtterances:
    """One batch of ``RaggedUtteranceFeed``, what ``Solver.ae_step_ragged`` takes in place of a list of tensors: ``x`` the packed
    [sum T, M] fp32 rows of this rank (utterance j = rows [T_j][M] at row sum T[:j]), ``T`` this rank's tuple of lengths, ``global_T``
    the lengths of all ranks' utterances of the step (equal to ``T`` in a single process): the loss means are taken over those."""
    __slots__ = ("x", "T", "global_T")

    def __init__(self, x, T, global_T=None):
        self.x = x
        self.T = tuple(int(t) for t in T)
        self.global_T = self.T if global_T is None else tuple(int(t) for t in global_T)


class RaggedUtteranceFeed:
    """Device-resident feed of WHOLE utterances (or crops of them) of different lengths for ``Solver.ae_step_ragged``: the corpus of
    ``DeviceSegmentFeed`` ([sum_T, M], uploaded once), a batch is one small upload of N first rows and ONE launch of
    ``avc_gather_utterances`` (csrc/ragged_feed.hip) into a packed block this feed owns.

    Length templates.  The ragged step keeps plans, workspaces and tables per tuple of lengths, so the tuples must repeat: the feed fixes
    K = ``n_templates`` GLOBAL tuples at construction.  The utterances of at least ``min_frames`` frames are kept, their lengths clipped to
    ``max_frames`` and sorted, L_0 <= ... <= L_{U-1}; of S = K N W slots, slot i has the length at index round(i (U - 1) / (S - 1)) (halves
    up) and belongs to template i % K -- every template spans the whole distribution of lengths and all carry about the same number of
    frames; slot 0 is the shortest kept utterance.  Within a template (its N W slots in ascending order) rank r takes positions r, r + W,
    ...: the ranks carry about the same number of frames too.

    A step draws, from the CPU generator all ranks seed alike: the template, ``randint(K)``; then ``rand(2, N W)`` in float64, u and v:
    slot p of the template takes utterance number floor(u_p n_p) of the n_p kept utterances that are at least as long as the slot (in
    order of length, then of appearance in ``data``) and crops it at frame floor(v_p (len - slot + 1)).  Every rank draws all N W slots
    and keeps its own, so the batches do not depend on ``world_size``.  ``__next__`` returns a ``PackedUtterances`` whose ``x`` is the
    template's own buffer: it is overwritten by the next visit of that template (in stream order), which is all a training loop needs.
    The iterator is infinite."""

    def __init__(self, data, batch_size, device, n_templates=8, min_frames=17, max_frames=None, seed=0, rank=0, world_size=1, lib=None):
        self.batch_size, self.n_templates = int(batch_size), int(n_templates)
        self.rank, self.world = int(rank), int(world_size)
        self.min_frames = int(min_frames)
        if not (0 <= self.rank < self.world):
            raise ValueError("rank must be in [0, world_size)")
        if self.batch_size < 1 or self.n_templates < 1 or self.min_frames < 1:
            raise ValueError("batch_size, n_templates and min_frames must be at least 1")
        self.lib = lib if lib is not None else _lib.load()
        if not hasattr(self.lib, "avc_gather_utterances"):
            raise RuntimeError("this build of the library has no avc_gather_utterances: rebuild it (csrc/build.sh)")
        ids, first, lens, chunks, pos = [], [], [], [], 0
        for k, v in data.items():
            v = np.asarray(v, dtype=np.float32)
            ids.append(k)
            first.append(pos)
            lens.append(int(v.shape[0]))
            pos += v.shape[0]
            chunks.append(v)
        kept = [i for i, n in enumerate(lens) if n >= self.min_frames]
        if not kept:
            raise ValueError(f"no utterance of the corpus has min_frames = {self.min_frames} frames or more")
        self.max_frames = max(lens[i] for i in kept) if max_frames is None else int(max_frames)
        if self.max_frames < self.min_frames:
            raise ValueError("max_frames must be at least min_frames")
        self.corpus = torch.from_numpy(np.concatenate(chunks, axis=0)).to(device).contiguous()   # [sum_T, M], resident
        self.n_rows, self.n_mels = int(self.corpus.shape[0]), int(self.corpus.shape[1])
        kept.sort(key=lambda i: lens[i])   # (stable: equal lengths stay in order of appearance)
        self.utt_ids = [ids[i] for i in kept]
        self._first = np.asarray([first[i] for i in kept], dtype=np.int64)
        self._len = np.asarray([lens[i] for i in kept], dtype=np.int64)
        L = np.minimum(self._len, self.max_frames)   # still ascending
        U, K, NW = len(kept), self.n_templates, self.batch_size * self.world
        S = K * NW
        slots = [int(L[(2 * i * (U - 1) + (S - 1)) // (2 * (S - 1))]) if S > 1 else int(L[0]) for i in range(S)]
        self.templates = [tuple(slots[k::K]) for k in range(K)]                     # global tuples, N W lengths each
        self._lo = [np.searchsorted(self._len, np.asarray(t), side="left") for t in self.templates]   # first kept utterance long enough
        dev = self.corpus.device
        self._state = []
        for t in self.templates:
            mine = t[self.rank::self.world]
            xoff = [sum(mine[:j]) for j in range(len(mine))]
            tabs = torch.tensor(list(mine) + xoff, dtype=torch.int32).to(dev)
            N = len(mine)
            self._state.append({"T": mine, "T_dev": tabs[:N], "xoff_dev": tabs[N:], "T_max": max(mine),
                                "starts": torch.zeros(N, dtype=torch.int64, device=dev),
                                "x": torch.empty(sum(mine), self.n_mels, dtype=torch.float32, device=dev)})
        self.gen = torch.Generator(device="cpu").manual_seed(seed)
        self.last_draw = None   # (template, kept-utterance numbers, crop frames) of all N W slots of the last step

    @classmethod
    def from_files(cls, pickle_path, batch_size, device, **kw):
        with open(pickle_path, "rb") as f:
            data = pickle.load(f)
        return cls(data, batch_size, device, **kw)

    def __iter__(self):
        return self

    def draw(self):
        """(template k, kept-utterance number and crop frame of each of its N W slots): the host side of a step"""
        k = int(torch.randint(self.n_templates, (1,), generator=self.gen))
        t = np.asarray(self.templates[k], dtype=np.int64)
        uv = torch.rand(2, len(t), dtype=torch.float64, generator=self.gen).numpy()
        lo = self._lo[k]
        n = len(self._len) - lo
        utt = lo + np.minimum((uv[0] * n).astype(np.int64), n - 1)
        room = self._len[utt] - t + 1
        crop = np.minimum((uv[1] * room).astype(np.int64), room - 1)
        return k, utt, crop

    def __next__(self):
        k, utt, crop = self.draw()
        self.last_draw = (k, utt, crop)
        st = self._state[k]
        rows = (self._first[utt] + crop)[self.rank::self.world]
        cuda = self.corpus.is_cuda
        host = torch.empty(len(rows), dtype=torch.int64, pin_memory=cuda)
        host.numpy()[:] = rows
        st["starts"].copy_(host, non_blocking=True)
        P = lambda t: ctypes.c_void_p(t.data_ptr())
        stream = ctypes.c_void_p(torch.cuda.current_stream(self.corpus.device).cuda_stream) if cuda else None
        with (torch.cuda.device(self.corpus.device) if cuda else _null()):
            rc = self.lib.avc_gather_utterances(P(self.corpus), self.n_rows, self.n_mels, P(st["starts"]), P(st["T_dev"]), P(st["xoff_dev"]),
                                                len(rows), st["T_max"], P(st["x"]), stream)
        if rc != 0:
            raise RuntimeError(f"avc_gather_utterances failed: {rc}")
        return PackedUtterances(st["x"], st["T"], self.templates[k])


class _null:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False
