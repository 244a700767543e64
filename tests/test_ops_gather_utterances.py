"""avc_gather_utterances (csrc/ragged_feed.hip): whole utterances out of the resident corpus into the packed rows of the ragged step,
in red zones (tests/redzone.py).  out must equal ``torch.cat`` of the corpus slices bit for bit; the guards around out, the corpus and the
three tables must stay as they were.

Shapes: M = 5 (rows of 20 bytes: a run starts on a 16-byte boundary only where its first row is a multiple of 4 on that side, so both copy
paths and the n % 4 tail of the wide one run), the tiny config's mel count, 80 (65 frames = 5200 floats: two workgroups per run).  Lengths
{1, 31, 32, 33, 65}: packed-row offsets 0, 1, 32, 64, 97.  Utterance 0 starts at corpus row 0, utterance 4 ends on the last corpus row;
utterances 0 and 2 are aligned on both sides at every M, 1 and 4 on neither at M = 5, 3 on the destination side only.  T_max is passed
larger than the longest utterance: workgroups past the end of every run.  kind='emu': the CPU lane-level simulation, kind='gpu': gfx950."""
import pytest
import torch

from oracle import avc_oracle as O
from tests.emu_util import KINDS, P, backend
from tests.redzone import GuardedOutput, guarded_input

N_ROWS = 120
LENGTHS = (1, 31, 32, 33, 65)
STARTS = (0, 5, 8, 13, N_ROWS - 65)
TINY_M = int(O.tiny_config()["ContentEncoder"]["c_in"])


def _table(values, dtype, fill, dev):
    """(view of the N entries, whole buffer): the table in the middle of a buffer of `fill` entries -- an entry the kernel's own bounds check
    rejects (a negative start, a length past any corpus), so a read past the table copies nothing rather than from a wild address"""
    buf = torch.full((len(values) + 128,), fill, dtype=dtype)
    buf[64:64 + len(values)] = torch.tensor(values, dtype=dtype)
    buf = buf.to(dev)
    return buf[64:64 + len(values)], buf


def _run(kind, M, lengths, starts, t_max_extra):
    lib, dev = backend(kind)
    corpus = torch.randn(N_ROWS, M, generator=torch.Generator().manual_seed(100 + M))
    xoff = [sum(lengths[:j]) for j in range(len(lengths))]
    cg = guarded_input(corpus, device=dev)
    out = GuardedOutput((sum(lengths), M), device=dev)
    (st, st_buf), (tt, tt_buf), (xo, xo_buf) = (_table(starts, torch.int64, -1, dev), _table(lengths, torch.int32, 2 ** 30, dev),
                                               _table(xoff, torch.int32, 0, dev))
    before = [b.clone() for b in (st_buf, tt_buf, xo_buf)]
    rc = lib.avc_gather_utterances(P(cg), N_ROWS, M, P(st), P(tt), P(xo), len(lengths), max(lengths) + t_max_extra, P(out.view), None)
    assert rc == 0
    out.assert_intact(f"(avc_gather_utterances, M = {M})")
    ref = torch.cat([corpus[s:s + t] for s, t in zip(starts, lengths)])
    got = out.view.cpu()
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), f"{int((got != ref).sum())} elements differ"
    for b, a, name in zip(before, (st_buf, tt_buf, xo_buf), ("starts", "T", "xoff")):
        assert torch.equal(b.cpu(), a.cpu()), f"the {name} table or its surroundings changed"
    assert torch.equal(cg.cpu(), corpus)   # (the corpus is read-only)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("M", [5, TINY_M, 80])
def test_gather_utterances_in_red_zones(kind, M):
    assert STARTS[0] == 0 and STARTS[4] + LENGTHS[4] == N_ROWS
    if M == 5:   # both paths: runs aligned on both sides, on one side, on neither
        xoff = [sum(LENGTHS[:j]) for j in range(5)]
        both = [(s * M) % 4 == 0 and (x * M) % 4 == 0 for s, x in zip(STARTS, xoff)]
        assert both == [True, False, True, False, False]
    _run(kind, M, LENGTHS, STARTS, 7)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("M", [5, 80])
def test_gather_one_utterance(kind, M):
    _run(kind, M, (33,), (3,), 0)
    _run(kind, M, (33,), (N_ROWS - 33,), 0)


@pytest.mark.parametrize("kind", KINDS)
def test_an_utterance_outside_the_corpus_is_left_out(kind):
    """the kernel's own bounds check: rows that are not all inside the corpus are neither read nor written"""
    lib, dev = backend(kind)
    M, lengths, starts = 5, (4, 6, 3), (2, N_ROWS - 5, -1)
    corpus = torch.randn(N_ROWS, M, generator=torch.Generator().manual_seed(3))
    cg = guarded_input(corpus, device=dev)
    out = GuardedOutput((sum(lengths), M), device=dev)
    st, tt, xo = (torch.tensor(v, dtype=d).to(dev) for v, d in ((starts, torch.int64), (lengths, torch.int32), ((0, 4, 10), torch.int32)))
    assert lib.avc_gather_utterances(P(cg), N_ROWS, M, P(st), P(tt), P(xo), 3, 6, P(out.view), None) == 0
    out.assert_intact("(an utterance past the corpus)")
    got = out.view.cpu()
    assert torch.equal(got[:4], corpus[2:6]) and bool(torch.isnan(got[4:]).all())   # (the payload starts as NaN: blocks 1 and 2 untouched)


@pytest.mark.parametrize("kind", KINDS)
def test_bad_arguments_are_refused(kind):
    lib, dev = backend(kind)
    M = 5
    corpus = torch.zeros(N_ROWS, M).to(dev)
    out = torch.zeros(8, M).to(dev)
    st, tt, xo = torch.zeros(1, dtype=torch.int64).to(dev), torch.full((1,), 8, dtype=torch.int32).to(dev), torch.zeros(1, dtype=torch.int32).to(dev)
    args = [P(corpus), N_ROWS, M, P(st), P(tt), P(xo), 1, 8, P(out), None]
    for i in (0, 3, 4, 5, 8):
        bad = list(args)
        bad[i] = None
        assert lib.avc_gather_utterances(*bad) == -1, f"null pointer argument {i}"
    for i, v in ((6, 0), (6, 65536), (7, 0), (2, 0), (1, 0)):
        bad = list(args)
        bad[i] = v
        assert lib.avc_gather_utterances(*bad) == -1, f"argument {i} = {v}"
    assert lib.avc_gather_utterances(*args) == 0
