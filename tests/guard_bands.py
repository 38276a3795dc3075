"""Operands carved out of larger buffers, shared by tests/checks/guard_stress.py, tests/checks/guard_fused.py and
tests/test_guard_bands_host.py.

A ``Carved`` region is ``nbytes`` inside a byte buffer, ``off`` bytes past a 256-byte-aligned address, with a band of a fill byte on
either side:
  * an OUTPUT (or scratch) region keeps ``PAT`` = 0xA5 in its bands; ``guards_ok()`` says whether a call left them alone. The band
    behind it is ``after`` bytes long - at least ``G``, and for the fused entry points at least the bytes the output would have at the
    entry point's largest row count (``after_band``), so that a store addressed with a padded row count, a padded column count or a
    wrong part offset lands inside the band and not in some other allocation;
  * an INPUT region gets bands of ``NAN_PAT`` = 0xFF: NaN as fp16, bf16 and fp32, -1 ("no adapter" / "no expert") as an id. A read
    outside the operand that reaches the result shows up as a NaN or a changed row.
What the bands cannot see: a read outside an operand that does not reach the result, and a store further away than the band.

Offsets: ``offset_for(align, rng)`` is an odd multiple of ``align`` - the region then has exactly the alignment its contract names
and no more; ``random_offset(align, rng)`` is guard_stress.py's random multiple in [0, 31]; ``place(align, rng)`` takes either, half
and half."""
import torch

G = 8192  # guard bytes on each side (the band behind an output may be longer: after_band)
PAT = 0xA5
NAN_PAT = 0xFF
MAX_OFF = 512  # offsets stay below this many bytes


def offset_for(align, rng):
    """A byte offset that is a multiple of ``align`` and not of ``2 * align``."""
    return align * (2 * rng.randint(0, 15) + 1)


def random_offset(align, rng):
    return align * rng.randint(0, 31)


def place(align, rng):
    """Half the draws: exactly ``align``; the other half: a random multiple of ``align`` in [0, 31]."""
    return offset_for(align, rng) if rng.random() < 0.5 else random_offset(align, rng)


def after_band(nbytes_at_largest_row_count):
    """Bytes of the band behind an output: at least G, at least the output's size at the entry point's largest row count."""
    return max(G, int(nbytes_at_largest_row_count))


class Carved:
    """nbytes inside a guarded buffer, starting `off` bytes past a 256-byte-aligned address."""

    def __init__(self, nbytes, off, device="cuda", after=G, fill=PAT):
        assert 0 <= off <= MAX_OFF and after >= G
        self.fill = fill
        self.buf = torch.full((G + 256 + MAX_OFF + nbytes + after,), fill, dtype=torch.uint8, device=device)
        base = self.buf.data_ptr()
        self.start = G + (-base - G) % 256 + off
        self.nbytes = nbytes
        self.after = self.buf.numel() - self.start - nbytes
        self.view = self.buf[self.start:self.start + nbytes]

    def ptr(self):
        return self.view.data_ptr()

    def put(self, t):
        self.view.copy_(t.contiguous().view(-1).view(torch.uint8))
        return self

    def as_tensor(self, dtype, shape):
        return self.view.view(dtype).view(*shape)  # (only when the offset keeps torch's alignment rule for the dtype)

    def bytes(self):
        return self.view.clone()

    def bands(self):
        return self.buf[:self.start], self.buf[self.start + self.nbytes:]

    def guards_ok(self):
        lo, hi = self.bands()
        return bool((lo == self.fill).all()) and bool((hi == self.fill).all())


def carve_in(t, rng, elt=None, device="cuda", fill=PAT, off=None):
    elt = elt or t.element_size()
    c = Carved(t.numel() * t.element_size(), elt * rng.randint(0, 31) if off is None else off, device=device, fill=fill)
    return c.put(t)


def carve_out(nbytes, rng, elt, device="cuda", after=G, off=None):
    return Carved(nbytes, elt * rng.randint(0, 31) if off is None else off, device=device, after=after)


def read(c, dtype, n):
    return c.bytes().view(dtype)[:n] if c.nbytes else torch.empty(0, dtype=dtype, device=c.buf.device)
