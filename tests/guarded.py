"""Guard bands and poisoned scratch around caller-owned buffers (test aid; imported like replay_tap.py and _devcopy.py).

An Arena is ONE uint8 allocation filled with a poison byte. carve() hands out tensor views of it whose first byte is 256-byte
aligned and whose last byte is followed IMMEDIATELY by at least guard_bytes of poison (no rounding of the size: the first
guard byte of a u8 tensor of 257 elements is byte 257); at least guard_bytes of poison precede it too. check() lists every
guard byte that no longer holds the poison. The guards of neighbouring buffers do not overlap, so a violation names the buffer
whose edge was crossed.

Poison patterns (POISONS): 0xFF bytes are NaN as f32 / bf16 / f64, -1 as int64 and 255 as u8; 0x00 bytes are the zeroes a
kernel may wrongly rely on; 0x7B bytes are a large finite f32 / bf16 (about 1.3e36), which survives a max() or a compare that
drops NaNs. A result that is bit-identical under all three did not read the bytes.

The guard width is a condition, not a measurement: it must exceed the store footprint of one workgroup of any kernel under
test (the largest is a 256 x 128 f32 tile row set, well under 1 MiB); a longer overrun meets the next buffer's guard first.
"""
from collections import namedtuple

import torch

NAN, ZERO, BIG = 0xFF, 0x00, 0x7B
POISONS = (NAN, ZERO, BIG)
ALIGN = 256

Violation = namedtuple("Violation", "name side nbytes first last")
Violation.__doc__ = """A changed guard region: `side` is "before" or "behind"; `first` / `last` are the offsets of the first and
the last changed byte relative to the buffer edge (before: -1 is the byte in front of the first element; behind: +1 is the
byte after the last element)."""


def _align_up(n, a=ALIGN):
    return (n + a - 1) // a * a


class Arena:
    def __init__(self, device, guard_bytes=1 << 20, capacity_bytes=64 << 20, fill=NAN):
        self.guard_bytes = int(guard_bytes)
        self.fill = fill
        self.mem = torch.full((int(capacity_bytes) + ALIGN,), fill, dtype=torch.uint8, device=device)
        self._base = (-self.mem.data_ptr()) % ALIGN             # offset of the first 256-byte aligned byte
        self._top = self._base                                  # everything in front of _top is handed out (or guard)
        self.bufs = []                                          # (name, first byte, one past the last byte)

    def reset(self, fill):
        """Forget every carved buffer and refill the whole arena (guards included) with another poison."""
        self.fill = fill
        self.mem.fill_(fill)
        self._top = self._base
        self.bufs = []

    def carve(self, shape, dtype, fill=None, name=None):
        """A tensor view of `shape` / `dtype`. fill: None leaves the arena's poison in it, an int is a byte pattern, a tensor
        is copied in (same element count and dtype)."""
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        n = 1
        for s in shape:
            n *= s
        nbytes = n * torch.empty((), dtype=dtype).element_size()
        start = _align_up(self._top - self._base + self.guard_bytes) + self._base
        end = start + nbytes
        if end + self.guard_bytes > self.mem.numel():
            raise MemoryError("arena of %d bytes is full (%d buffers carved)" % (self.mem.numel(), len(self.bufs)))
        self._top = end + self.guard_bytes
        self.bufs.append((name or "buf%d" % len(self.bufs), start, end))
        view = self.mem[start:end].view(dtype).reshape(shape)
        if isinstance(fill, torch.Tensor):
            assert fill.dtype == dtype and fill.numel() == n, (fill.dtype, dtype, fill.numel(), n)
            view.copy_(fill.reshape(shape))
        elif fill is not None:
            self.mem[start:end].fill_(fill)
        return view

    def put(self, t, name=None):
        """A carved copy of tensor `t`."""
        return self.carve(t.shape, t.dtype, fill=t, name=name)

    def check(self):
        """[] if every guard byte still holds the poison, else one Violation per changed guard region."""
        out = []
        G = self.guard_bytes
        for name, start, end in self.bufs:
            for side, lo, edge in (("before", start - G, start), ("behind", end, end - 1)):
                bad = (self.mem[lo:lo + G] != self.fill).nonzero()
                if bad.numel():
                    out.append(Violation(name, side, int(bad.numel()), int(bad[0]) + lo - edge, int(bad[-1]) + lo - edge))
        return out


def _as_words(buf, pat):
    """(`buf` flat as integers of its element width, the poison byte `pat` repeated to that width): one compare per element."""
    b = buf.reshape(-1)
    dt = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[b.element_size()]
    word = int.from_bytes(bytes([pat]) * b.element_size(), "little", signed=b.element_size() > 1)
    return b.view(dt), word


def written(buf, pat):
    """bool per element of `buf`: does any of its bytes differ from the poison byte `pat`?"""
    words, word = _as_words(buf, pat)
    return words != word


def last_written(buf, pat):
    """One past the index of the last element of `buf` that differs from the poison byte `pat`; 0 if none does."""
    w = written(buf, pat)
    if not bool(w.any()):
        return 0
    return w.numel() - int(w.flip(0).to(torch.uint8).argmax())       # (argmax: the first maximum, i.e. the LAST written one)


def high_water(buf_a, buf_b, pat_a, pat_b):
    """One past the index of the last element that differs from its poison in either of two runs of the same call on scratch
    poisoned with pat_a (buf_a) and pat_b (buf_b); 0 if neither run wrote anything. A written value can equal one poison by
    chance; it cannot equal two different ones. (The last element of a union is the later of the two last elements: a test that
    cannot keep both buffers takes max(last_written(...)) over its runs.)"""
    assert pat_a != pat_b and buf_a.numel() == buf_b.numel()
    return max(last_written(buf_a, pat_a), last_written(buf_b, pat_b))


def bits(t):
    """The bytes of a tensor or NumPy array as a flat uint8 host tensor: torch.equal on them is equality bit for bit."""
    if not isinstance(t, torch.Tensor):
        import numpy as np
        t = torch.from_numpy(np.ascontiguousarray(t))
    return t.detach().contiguous().reshape(-1).view(torch.uint8).cpu()


# One arena per test module, grown on demand, freed by the module's `free_arena` fixture when the module is done.
_arenas = {}


def arena(owner, need_bytes, nbufs, fill, guard_bytes=1 << 20):
    """The arena of test module `owner` (its __name__), reset to `fill`, with room for `nbufs` buffers of `need_bytes` in all;
    replaced by a larger one when a case needs it."""
    cap = need_bytes + nbufs * (2 * guard_bytes + 2 * ALIGN)
    a = _arenas.get(owner)
    if a is None or a.mem.numel() < cap + ALIGN or a.guard_bytes != guard_bytes:
        _arenas.pop(owner, None)
        del a
        _arenas[owner] = Arena("cuda", guard_bytes=guard_bytes, capacity_bytes=cap, fill=fill)
    else:
        _arenas[owner].reset(fill)
    return _arenas[owner]


def release(owner):
    """Drop the arena of `owner` and hand its memory back to the device."""
    if _arenas.pop(owner, None) is not None and torch.cuda.is_available():
        torch.cuda.empty_cache()
