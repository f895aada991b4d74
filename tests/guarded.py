"""Guard bands around device (or CPU) buffers: does a call stay inside the buffers it was given, at any legal alignment?

A kernel that loads or stores a few items outside its buffers changes no output value when the buffers sit in the middle of a larger
allocation, so a test of values alone never sees it.  Here every buffer is a view into one larger allocation:

  guarded_input(array, pad_items, offset_items)     the payload, NaN on both sides (float payloads; a fixed odd bit pattern for
                                                    integer payloads): a read outside that reaches an output turns it into NaN,
                                                    even through a zero tap or a zero window value
  guarded_output(n_items, dtype, pad_items, offset_items)
                                                    interior pre-filled with NaN (an item the call never wrote shows), a finite
                                                    sentinel bit pattern on both sides (a store outside shows)
  prefill_output(view, prior)                       the accumulate form of a call adds into its output: the interior then holds a prior
                                                    result, not NaN (an item the call skipped shows in the values: it still holds the prior)
  check_guards(whole, view)                         pads bit for bit as they were made, interior of an output all written and
                                                    finite; raises GuardError naming the first violated item.  interior=False: the pads
                                                    only (an output the call writes in part, such as the rows of a pitched copy)

The view's data pointer is `offset_items` items past a 16-byte boundary, so an offset of one complex64 item gives a buffer
that is 8-byte but not 16-byte aligned.  Plain module (no fixtures); takes a torch device, so it runs on CPU tensors too
(tests/test_guarded.py proves there that each kind of stray access is caught).
"""
import numpy as np
import torch

SENTINEL = 0x5A5A5A5B   # pads of an output and of an integer input: odd, finite as float32 (1.5368e16), no byte repeats with period 1
NAN_BITS = 0x7FC00000   # pads of a float input, interior of an output before the call: quiet NaN as float32

_TORCH_OF = {np.dtype(np.complex64): torch.complex64, np.dtype(np.float32): torch.float32, np.dtype(np.int32): torch.int32,
             np.dtype(np.int8): torch.int8}
_FLOAT = (torch.complex64, torch.float32)


class GuardError(AssertionError):
    """where: 'before' / 'after' (a pad was changed) or 'interior' (an output item unwritten or not finite).  index: the item, counted
    from the first item of the payload (negative before it, >= n_items after it).  distance: items between it and the payload (1 = the
    item next to the payload, 0 inside)."""

    def __init__(self, name, where, index, distance, n_items, detail):
        self.where, self.index, self.distance, self.n_items = where, int(index), int(distance), int(n_items)
        super().__init__("%s: %s item %d of a %d-item payload (%s%s)" % (
            name, {"before": "stray store before the buffer at", "after": "stray store after the buffer at",
                   "interior": "unwritten or non-finite output"}[where], self.index, self.n_items,
            "%d item(s) from the payload, " % self.distance if where != "interior" else "", detail))


def pad_items(itemsize, unit_items=0):
    """Items of padding on each side: max(64 KiB, one frame or block of the operation), at most 1 MiB.  64 KiB is two 4096-value
    frame groups, the largest unit a one-pass kernel moves per step; a stray row of a multi-pass size lands one frame apart."""
    nbytes = min(max(64 << 10, int(unit_items) * itemsize), 1 << 20)
    return (nbytes + itemsize - 1) // itemsize


def _pattern(nbytes, bits, device):
    """nbytes bytes of the 32-bit pattern, phase-locked to byte 0 of the allocation"""
    return torch.full(((nbytes + 3) // 4,), bits, dtype=torch.int32, device=device).view(torch.uint8)[:nbytes]


def _alloc(n_items, tdtype, pad, offset_items, pad_bits, device):
    isz = torch.empty(0, dtype=tdtype).element_size()
    nbytes = n_items * isz
    total = (2 * pad * isz + nbytes + 32 + 3) // 4 * 4
    whole = _pattern(total, pad_bits, device)
    # first byte of the payload: at least `pad` items in, `offset_items` items past a 16-byte boundary of the address space
    start = pad * isz
    start += (offset_items * isz - (whole.data_ptr() + start)) % 16
    assert (whole.data_ptr() + start) % 16 == (offset_items * isz) % 16 and start % isz == 0
    view = whole[start:start + nbytes].view(tdtype)
    whole._guard = {"bits": pad_bits, "start": start, "nbytes": nbytes, "itemsize": isz, "dtype": tdtype}
    return whole, view


def guarded_input(array, pad_items, offset_items=0, device="cpu"):
    """(whole, view): `array` (numpy; complex64, float32, int32 or int8) as a view `offset_items` items past a 16-byte boundary inside
    one larger allocation; NaN (float payloads) or SENTINEL (integer payloads) everywhere else."""
    array = np.ascontiguousarray(array).reshape(-1)
    tdtype = _TORCH_OF[array.dtype]
    whole, view = _alloc(array.size, tdtype, int(pad_items), int(offset_items), NAN_BITS if tdtype in _FLOAT else SENTINEL, device)
    view.copy_(torch.from_numpy(array))
    whole._guard["kind"] = "input"
    return whole, view


def guarded_output(n_items, dtype, pad_items, offset_items=0, device="cpu"):
    """(whole, view): an output of n_items items of numpy `dtype`; the interior holds NaN bit patterns until the call writes it, the
    pads hold SENTINEL."""
    tdtype = _TORCH_OF[np.dtype(dtype)]
    whole, view = _alloc(int(n_items), tdtype, int(pad_items), int(offset_items), SENTINEL, device)
    g = whole._guard
    whole[g["start"]:g["start"] + g["nbytes"]] = _pattern(g["nbytes"], NAN_BITS, device) if g["start"] % 4 == 0 else 0xFF
    g["kind"] = "output"
    return whole, view


def prefill_output(view, prior):
    """Overwrite the NaN interior of a guarded_output with `prior` (numpy, same dtype and item count): what an accumulating call adds into.
    The pads are untouched, so a store outside still shows; returns the view."""
    prior = np.ascontiguousarray(prior).reshape(-1)
    assert _TORCH_OF[prior.dtype] == view.dtype and prior.size == view.numel(), "the prior is not an output of this buffer"
    view.copy_(torch.from_numpy(prior))
    return view


def _first_bad(mask):
    idx = torch.nonzero(mask)
    return None if idx.numel() == 0 else int(idx[0, 0])


def check_guards(whole, view, name="buffer", interior=True):
    """Raises GuardError unless both pads of `whole` still hold their bit pattern and, for an output (unless interior=False), every
    interior item was written and is finite.  The first violated item is named: stores before the buffer are reported nearest the
    payload first."""
    g = whole._guard
    start, nbytes, isz = g["start"], g["nbytes"], g["itemsize"]
    assert view.data_ptr() - whole.data_ptr() == start and view.numel() * view.element_size() == nbytes, "not the view of this allocation"
    n_items = nbytes // isz
    expect = _pattern(whole.numel(), g["bits"], whole.device)
    if start % 4 == 0 and (start + nbytes) % 4 == 0:  # the usual case: the pads are whole 32-bit words, compared as int32
        bad, u = whole.view(torch.int32) != expect.view(torch.int32), 4
    else:
        bad, u = whole != expect, 1
    after = _first_bad(bad[(start + nbytes) // u:])
    lo = torch.nonzero(bad[:start // u])
    before = None if lo.numel() == 0 else int(lo[-1, 0]) * u + (u - 1)  # (last byte of the last changed word)
    after = None if after is None else after * u
    if before is not None:
        d = (start - 1 - before) // isz + 1
        raise GuardError(name, "before", -d, d, n_items, "byte %d of the allocation" % before)
    if after is not None:
        d = after // isz + 1
        raise GuardError(name, "after", n_items + d - 1, d, n_items, "byte %d of the allocation" % (start + nbytes + after))
    if g["kind"] != "output" or not interior:
        return
    if g["dtype"] in _FLOAT:
        flat = view.view(torch.float32) if g["dtype"] == torch.float32 else torch.view_as_real(view).reshape(-1)
        per_item = flat.numel() // n_items if n_items else 1
        k = _first_bad(~torch.isfinite(flat))
        if k is not None:
            raise GuardError(name, "interior", k // per_item, 0, n_items, "value %r" % (flat[k].item(),))
    else:
        raw = whole[start:start + nbytes]
        unwritten = _pattern(nbytes, NAN_BITS, whole.device) if start % 4 == 0 else torch.full_like(raw, 0xFF)
        same = (raw == unwritten).view(n_items, isz).all(dim=1) if n_items else raw.new_zeros(0, dtype=torch.bool)
        k = _first_bad(same)
        if k is not None:
            raise GuardError(name, "interior", k, 0, n_items, "still holds the pre-fill pattern")


def to_numpy(view):
    """The payload on the host as a flat numpy array of its own dtype."""
    return view.detach().cpu().numpy().reshape(-1)
