"""Red zones for kernel tests: tensors handed to the library sit inside larger buffers whose surroundings are checked.

No sanitizer sees the kernels (the simulator has no bounds checking, the GPU has none we may use), so the tests carry their own:
  - an INPUT is a view into a buffer that is NaN everywhere else: a read past the tensor (or into the gap between two rows of a
    strided view) poisons the result, which the value comparison of the test then reports;
  - an OUTPUT (or scratch / in-place buffer) is a view into a buffer whose surroundings hold a sentinel bit pattern, compared BITWISE
    afterwards: a write past the tensor (or into a gap) is reported with its offset.
Geometry: `PAD` floats in front and behind (8 KiB: more than two conv tiles of one row), `gap` floats after every innermost row (row
stride T + gap).  PAD is a multiple of 64 floats, so the view has the alignment of a fresh torch tensor and the kernels take the same
vector paths as in an unguarded run.  dtype float32, or int32 for the dword tensors of the bf16 pair storage (`void*` in the C ABI).
Works on CPU (simulator) and cuda tensors.  No tests in this module."""
import torch

PAD = 2048
# A quiet NaN with a payload in both halves: no kernel produces it (arithmetic yields the canonical NaN 0x7FC00000), it is NaN as fp32 and
# as either bf16 half of a pair dword, so a guard that is READ poisons what is computed from it too.
SENTINEL = 0x7FD57FD5
_BF16_NAN_PAIR = 0x7FC07FC0   # "NaN" payload fill of a dword tensor: both bf16 halves NaN


def _geometry(shape, gap):
    shape = tuple(int(s) for s in shape)
    T = shape[-1] if shape else 1
    rows = 1
    for s in shape[:-1]:
        rows *= s
    pitch = T + int(gap)
    strides, acc = [], pitch
    for s in reversed(shape[:-1]):
        strides.append(acc)
        acc *= s
    strides = tuple(reversed(strides)) + (1,)
    return shape, rows, T, pitch, strides, PAD + rows * pitch + PAD


def _new_buffer(total, dtype, sentinel, device):
    i32 = torch.full((total,), SENTINEL if sentinel else (0x7FC00000 if dtype == torch.float32 else _BF16_NAN_PAIR), dtype=torch.int32)
    return i32.view(dtype).to(device)


def guarded_input(t, gap=0, device=None):
    """A view with t's values (float32 or int32 dwords) inside a buffer that is NaN everywhere else: PAD in front and behind, `gap`
    after every innermost row.  For a transposed view (the collate view, strides (T*M, 1, M)) guard the contiguous [B, T, M] tensor
    and transpose the result."""
    device = t.device if device is None else device
    shape, rows, T, pitch, strides, total = _geometry(t.shape, gap)
    buf = _new_buffer(total, t.dtype, False, device)
    view = torch.as_strided(buf, shape, strides, PAD)
    view.copy_(t.to(device))
    return view


class GuardedOutput:
    """An output / scratch / in-place buffer of `shape` inside sentinel red zones.  `.view` goes to the library; the payload starts as NaN
    (unwritten elements stay visible) or as a copy of `init`.  A 1-D shape is the flat form (workspaces, parameter and gradient buffers)."""

    def __init__(self, shape, gap=0, dtype=torch.float32, device="cpu", init=None):
        if isinstance(shape, int):
            shape = (shape,)
        self.shape, self.rows, self.T, self.pitch, strides, total = _geometry(shape, gap)
        self.buf = _new_buffer(total, dtype, True, device)
        self.view = torch.as_strided(self.buf, self.shape, strides, PAD)
        if init is not None:
            self.view.copy_(init.to(device))
        else:
            self.view.fill_(float("nan") if dtype == torch.float32 else _BF16_NAN_PAIR)
        guard = torch.ones(total, dtype=torch.bool)
        torch.as_strided(guard, self.shape, strides, PAD).fill_(False)
        self._guard = guard.to(device)

    def assert_intact(self, msg=""):
        """Every pad and gap dword still holds the sentinel, compared bitwise."""
        bits = self.buf.view(torch.int32)
        bad = (bits != SENTINEL) & self._guard
        if bool(bad.any()):
            idx = int(bad.nonzero()[0].item())
            val = self.buf[idx].item()
            rel = idx - PAD
            where = "in front of the payload" if rel < 0 else (
                "behind the payload" if rel >= self.rows * self.pitch else f"in the gap of row {rel // self.pitch} (column {rel % self.pitch} of a {self.T}-float row)")
            raise AssertionError(f"red zone breached {msg}: {int(bad.sum())} dword(s) changed; first at offset {rel:+d} from the payload's first element "
                                 f"({where}), new value {val!r} (bits 0x{int(bits[idx].item()) & 0xFFFFFFFF:08X})")


def guarded_like(t, gap=0, device=None):
    """GuardedOutput whose payload starts as a copy of t (in-place operands: parameters, optimizer state)."""
    return GuardedOutput(tuple(t.shape), gap=gap, dtype=t.dtype, device=t.device if device is None else device, init=t)
