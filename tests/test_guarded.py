"""The guarded-buffer helper (tests/guarded.py) catches what it is for: plain torch-CPU stand-ins for a kernel that strays by one item
are each reported with the right item.  This is the evidence that tests/test_device_bounds_gpu.py can fail; nothing is ever broken or
placed at the end of an allocation on the GPU to show it.

The stand-in operation is y[i] = x[i] + h * x[i + 1] for i < n - 1 and y[n - 1] = x[n - 1], with h = 0: the shape of a filter whose
last tap is zero-padded.  A stand-in that also applies the tap at i = n - 1 reads one item past its input; with a float payload the
NaN there reaches the output through the zero tap (NaN * 0 = NaN).  With an integer payload there is no NaN: the pad's bit pattern
times zero is zero, so a stray read through a zero weight cannot show; it shows, like on the GPU, in the comparison of the values
with the reference as soon as the weight is not zero (h = 1 below)."""
import numpy as np
import pytest
import torch

from guarded import GuardError, NAN_BITS, SENTINEL, check_guards, guarded_input, guarded_output, pad_items, prefill_output, to_numpy

DTYPES = [np.complex64, np.float32, np.int32]
N = 1000


def _payload(dtype, n, seed=0):
    rng = np.random.default_rng(seed)
    if dtype == np.complex64:
        return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    if dtype == np.float32:
        return rng.standard_normal(n).astype(np.float32)
    return rng.integers(-1000, 1000, n).astype(np.int32)


def _past(view, k):
    """the view extended by k items past its end, as a kernel's pointer arithmetic sees it"""
    return torch.as_strided(view, (view.numel() + k,), (1,))


def _item_before(view):
    return torch.as_strided(view, (1,), (1,), view.storage_offset() - 1)


def _correct(x, y, n, h=0):
    y[:n - 1] = x[:n - 1] + h * x[1:n]
    y[n - 1] = x[n - 1]


def _writes_one_after(x, y, n, h=0):
    _correct(x, y, n, h)
    _past(y, 1)[n] = x[0]


def _writes_one_before(x, y, n, h=0):
    _correct(x, y, n, h)
    _item_before(y)[0] = x[0]


def _leaves_last_unwritten(x, y, n, h=0):
    y[:n - 1] = x[:n - 1] + h * x[1:n]


def _reads_one_past_input(x, y, n, h=0):
    y[:n] = x[:n] + h * _past(x, 1)[1:n + 1]


def _reference(a, h=0):
    r = a.copy()
    r[:-1] += a.dtype.type(h) * a[1:]
    return r


def _run(standin, dtype, off_in, off_out, h=0, device="cpu"):
    a = _payload(dtype, N)
    pad = pad_items(np.dtype(dtype).itemsize)
    xw, x = guarded_input(a, pad, off_in, device)
    yw, y = guarded_output(N, dtype, pad, off_out, device)
    standin(x, y, N, h)
    check_guards(xw, x, "input")
    check_guards(yw, y, "output")
    return to_numpy(y), _reference(a, h)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("off_in,off_out", [(0, 0), (1, 0), (0, 1), (1, 1)])
class TestStandIns:
    def test_layout(self, dtype, off_in, off_out):
        isz = np.dtype(dtype).itemsize
        pad = pad_items(isz)
        assert pad * isz == 64 << 10 and pad_items(8, 1 << 21) * 8 == 1 << 20 and pad_items(8, 16384) * 8 == 128 << 10
        xw, x = guarded_input(_payload(dtype, N), pad, off_in)
        yw, y = guarded_output(N, dtype, pad, off_out)
        assert x.data_ptr() % 16 == off_in * isz % 16 and y.data_ptr() % 16 == off_out * isz % 16
        for whole, view in ((xw, x), (yw, y)):
            lo = view.data_ptr() - whole.data_ptr()
            assert lo >= pad * isz and whole.numel() - lo - N * isz >= pad * isz  # at least the pad on either side
        words = xw.view(torch.int32)
        assert int(words[0]) == (SENTINEL if dtype == np.int32 else NAN_BITS) and int(yw.view(torch.int32)[0]) == SENTINEL
        with pytest.raises(GuardError) as e:  # nothing written yet: item 0 still holds the pre-fill
            check_guards(yw, y)
        assert (e.value.where, e.value.index) == ("interior", 0)

    def test_correct_standin_passes(self, dtype, off_in, off_out):
        got, ref = _run(_correct, dtype, off_in, off_out)
        assert np.array_equal(got, ref)
        got, ref = _run(_correct, dtype, off_in, off_out, h=1)
        assert np.array_equal(got, ref)

    def test_store_one_item_after_the_end(self, dtype, off_in, off_out):
        with pytest.raises(GuardError) as e:
            _run(_writes_one_after, dtype, off_in, off_out)
        assert (e.value.where, e.value.index, e.value.distance) == ("after", N, 1)
        assert "output" in str(e.value) and "item %d" % N in str(e.value)

    def test_store_one_item_before_the_start(self, dtype, off_in, off_out):
        with pytest.raises(GuardError) as e:
            _run(_writes_one_before, dtype, off_in, off_out)
        assert (e.value.where, e.value.index, e.value.distance) == ("before", -1, 1)
        assert "item -1" in str(e.value)

    def test_last_item_unwritten(self, dtype, off_in, off_out):
        with pytest.raises(GuardError) as e:
            _run(_leaves_last_unwritten, dtype, off_in, off_out)
        assert (e.value.where, e.value.index, e.value.distance) == ("interior", N - 1, 0)

    def test_read_one_item_past_the_input(self, dtype, off_in, off_out):
        if dtype != np.int32:  # through a ZERO weight: only the NaN shows it
            with pytest.raises(GuardError) as e:
                _run(_reads_one_past_input, dtype, off_in, off_out, h=0)
            assert (e.value.where, e.value.index) == ("interior", N - 1)
            with pytest.raises(GuardError):
                _run(_reads_one_past_input, dtype, off_in, off_out, h=1)
            return
        # integer payload: no NaN exists; the pad's bit pattern reaches the output through a weight that is not zero and the
        # comparison with the reference names the item
        got, ref = _run(_reads_one_past_input, dtype, off_in, off_out, h=1)
        assert np.flatnonzero(got != ref).tolist() == [N - 1]
        assert got[N - 1] == np.int32(ref[N - 1] + np.int32(SENTINEL))


def test_far_strays_and_input_pads_are_seen():
    """a store a whole frame group (4096 items) away, on either side, and a store into the input's pad"""
    a = _payload(np.complex64, N)
    pad = pad_items(8)
    for k, where in ((4096, "after"), (-4096, "before")):
        yw, y = guarded_output(N, np.complex64, pad, 1)
        y.copy_(torch.from_numpy(a))
        torch.as_strided(y, (1,), (1,), y.storage_offset() + (N - 1 + k if k > 0 else k))[0] = 1.0
        with pytest.raises(GuardError) as e:
            check_guards(yw, y)
        assert (e.value.where, e.value.distance, e.value.index) == (where, 4096, N - 1 + k if k > 0 else k)
    xw, x = guarded_input(a, pad, 1)
    check_guards(xw, x)
    _past(x, 3)[N + 2] = 0.0
    with pytest.raises(GuardError) as e:
        check_guards(xw, x, "input")
    assert (e.value.where, e.value.index, e.value.distance) == ("after", N + 2, 3)


def test_nan_written_into_the_interior_is_reported():
    yw, y = guarded_output(N, np.float32, pad_items(4), 1)
    y.fill_(1.0)
    check_guards(yw, y)
    y[17] = float("inf")
    with pytest.raises(GuardError) as e:
        check_guards(yw, y)
    assert (e.value.where, e.value.index) == ("interior", 17)
    with pytest.raises(AssertionError):
        check_guards(yw, y[1:])  # not the view this allocation was made for


# ------------------------------------------------------------- what tests/test_xengine_bounds_gpu.py adds: int8 payloads, pre-filled outputs

def _sum_standin(x, n, stray):
    """stand-in for a correlator's integer sum over an int8 payload: the int32 sum of n (+ stray) bytes from the start of the view"""
    return int(_past(x, stray)[:n + stray].to(torch.int32).sum())


@pytest.mark.parametrize("n,off", [(1000, 0), (1000, 4), (1000, 12), (1001, 0), (1003, 8), (1002, 1), (999, 3)])
def test_int8_payload_a_read_one_byte_outside_changes_the_sum(n, off):
    """every byte of the integer sentinel is non-zero (5B 5A 5A 5A), so ONE stray int8 sample on either side changes an exact integer sum,
    whatever the phase of the pattern at the payload's edge; and check_guards compares pads that are not whole 32-bit words (odd payload
    sizes, offsets that are no multiple of 4) byte by byte"""
    assert all(b != 0 for b in SENTINEL.to_bytes(4, "little"))
    a = np.random.default_rng(n + off).integers(-128, 128, n, dtype=np.int64).astype(np.int8)
    xw, x = guarded_input(a, pad_items(1, 77), off)
    assert x.dtype == torch.int8 and x.data_ptr() % 16 == off and np.array_equal(to_numpy(x), a)
    check_guards(xw, x, "input")
    want = int(a.astype(np.int64).sum())
    assert _sum_standin(x, n, 0) == want
    assert _sum_standin(x, n, 1) != want                                                   # one byte past the end
    before = int(torch.as_strided(x, (n + 1,), (1,), x.storage_offset() - 1).to(torch.int32).sum())
    assert before != want                                                                  # one byte before the start
    # a store into either pad of the int8 input is seen too, at the byte next to the payload
    for k, where, index in ((n, "after", n), (-1, "before", -1)):
        xw, x = guarded_input(a, pad_items(1, 77), off)
        torch.as_strided(x, (1,), (1,), x.storage_offset() + k)[0] = 0
        with pytest.raises(GuardError) as e:
            check_guards(xw, x, "input")
        assert (e.value.where, e.value.index, e.value.distance) == (where, index, 1)


@pytest.mark.parametrize("dtype", [np.complex64, np.int32], ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("off_out", [0, 1])
def test_prefilled_output_still_reports_a_store_into_either_pad(dtype, off_out):
    """the accumulate form: the interior holds a prior result instead of NaN; a correct accumulating stand-in passes, one that also stores one
    item before or after the buffer is reported, and an item it skipped shows in the values (it still holds the prior)"""
    a = _payload(dtype, N)
    prior = (a[::-1] * 3).astype(dtype)
    pad = pad_items(np.dtype(dtype).itemsize)

    def accumulate(y, skip_last=False):
        m = N - 1 if skip_last else N
        y[:m] += torch.from_numpy(a)[:m]

    yw, y = guarded_output(N, dtype, pad, off_out)
    assert prefill_output(y, prior) is y
    accumulate(y)
    check_guards(yw, y, "output")
    assert np.array_equal(to_numpy(y), prior + a)
    for k, where, index in ((N, "after", N), (-1, "before", -1)):
        yw, y = guarded_output(N, dtype, pad, off_out)
        prefill_output(y, prior)
        accumulate(y)
        torch.as_strided(y, (1,), (1,), y.storage_offset() + k)[0] = 1
        with pytest.raises(GuardError) as e:
            check_guards(yw, y, "output")
        assert (e.value.where, e.value.index, e.value.distance) == (where, index, 1)
    yw, y = guarded_output(N, dtype, pad, off_out)
    prefill_output(y, prior)
    accumulate(y, skip_last=True)
    check_guards(yw, y, "output")  # (finite everywhere: the guards cannot see it ...)
    assert np.flatnonzero(to_numpy(y) != prior + a).tolist() == [N - 1]  # (... the comparison with the reference does)
    with pytest.raises(AssertionError):
        prefill_output(y, prior[:-1])


def test_pads_only_check_of_a_partly_written_output():
    """interior=False (the destination of a pitched copy: the gaps between its rows are never written): the pads are still compared"""
    yw, y = guarded_output(N, np.int8, pad_items(1), 0)
    y[:10] = 1
    with pytest.raises(GuardError) as e:
        check_guards(yw, y)
    assert e.value.where == "interior"
    check_guards(yw, y, interior=False)
    _past(y, 1)[N] = 1
    with pytest.raises(GuardError) as e:
        check_guards(yw, y, interior=False)
    assert (e.value.where, e.value.index) == ("after", N)
