"""CPU tests of tests/_merge_views.py: the views test_gpu_merge_alignment.py hands to the merge lie where it says, and the margin
check sees one changed byte on either side of a view."""
import pytest
import torch

import _merge_views as mv

DTYPES = [torch.uint8, torch.uint16, torch.float32, torch.float64]
IDS = ["u8", "u16", "f32", "f64"]


def _host(dtype, shape=(2, 3, 5, 7)):
    n = 1
    for s in shape:
        n *= s
    ramp = torch.arange(n, dtype=torch.float64).reshape(shape)
    if dtype in (torch.uint8, torch.uint16):
        return (ramp % 251 + 1).to(torch.int16).view(torch.uint16) if dtype == torch.uint16 else (ramp % 251 + 1).to(torch.uint8)
    return (ramp + 0.5).to(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("lead", [0, 1, 2, 3, 4, 8, 17])
def test_interior_places_the_view(dtype, lead):
    host = _host(dtype)
    size = host.element_size()
    view, buf = mv.interior(host, lead, "cpu")
    guard = 256 // size
    assert guard == mv.guard_elems(dtype)
    assert buf.data_ptr() % 256 == 0 and buf.dtype == (torch.int16 if dtype == torch.uint16 else dtype)
    assert view.dtype == dtype and view.shape == host.shape and view.is_contiguous()
    assert (view.data_ptr() - buf.data_ptr()) == (guard + lead) * size
    assert view.data_ptr() % 256 == (lead * size) % 256 and view.data_ptr() % 16 == (lead * size) % 16
    assert buf.numel() == 2 * guard + lead + host.numel() + 19
    alias = buf.dtype
    assert torch.equal(view.view(alias), host.view(alias))
    # the view IS the buffer's memory: what is written through it shows in the buffer, nothing else changes
    assert mv.margins_untouched(buf, lead, host.numel())
    view.view(alias).reshape(-1)[0] = 0
    assert int(buf[guard + lead]) == 0 and mv.margins_untouched(buf, lead, host.numel())


def test_interior_offsets_per_dtype():
    """One element, and the width that suits half a packet but not the packet: the residues the GPU tests rely on."""
    want = {(torch.uint8, 1): 1, (torch.uint8, 2): 2, (torch.uint8, 4): 4, (torch.uint16, 1): 2, (torch.uint16, 2): 4,
            (torch.float32, 1): 4, (torch.float32, 2): 8, (torch.float32, 4): 0, (torch.float64, 1): 8, (torch.float64, 2): 0,
            (torch.float64, 4): 0}
    for (dtype, lead), mod16 in want.items():
        view, buf = mv.interior(_host(dtype, (3, 4, 8)), lead, "cpu")
        assert view.data_ptr() % 16 == mod16, (dtype, lead)
        assert view.data_ptr() % 256 == lead * view.element_size(), (dtype, lead)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_margins_untouched_sees_one_byte(dtype):
    host = _host(dtype, (3, 5, 7))
    n, lead, tail = host.numel(), 3, 19
    size = host.element_size()
    first = (mv.guard_elems(dtype) + lead) * size          # byte offset of the view
    last = first + n * size                                # ... and of the first byte behind it
    total = (2 * mv.guard_elems(dtype) + lead + n + tail) * size
    for at in (first - 1, last, first - size, last + size - 1, 0, total - 1, first - 17, last + 16):
        view, buf = mv.interior(host, lead, "cpu", tail=tail)
        assert mv.margins_untouched(buf, lead, n)
        raw = buf.view(torch.uint8)
        assert raw.numel() == total
        raw[at] ^= 0x40
        assert not mv.margins_untouched(buf, lead, n), at
        raw[at] ^= 0x40
        assert mv.margins_untouched(buf, lead, n), at
    # bytes inside the view are no margin
    view, buf = mv.interior(host, lead, "cpu", tail=tail)
    for at in (first, last - 1):
        buf.view(torch.uint8)[at] ^= 0x40
    assert mv.margins_untouched(buf, lead, n)
    with pytest.raises(ValueError):
        mv.margins_untouched(buf, lead, buf.numel())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_sentinel_like_and_fully_written(dtype):
    view, buf = mv.sentinel_like((3, 5, 7), dtype, 1, "cpu")
    n = view.numel()
    assert view.dtype == dtype and bool((view == mv.SENTINEL).all())
    assert mv.margins_untouched(buf, 1, n) and not mv.fully_written(buf, 1, n)
    view.fill_(0.25)
    assert mv.fully_written(buf, 1, n) and mv.margins_untouched(buf, 1, n)
    view.reshape(-1)[n - 1] = mv.SENTINEL                   # one element the kernel skipped
    assert not mv.fully_written(buf, 1, n)
    # a negative zero is not the sentinel's pattern, and neither is a value that merely compares equal after rounding
    view.fill_(-0.0)
    assert mv.fully_written(buf, 1, n)


def test_fill_can_be_chosen_and_unknown_dtypes_are_refused():
    host = _host(torch.uint8, (2, 3, 4))
    view, buf = mv.interior(host, 1, "cpu", fill=7)
    assert mv.margins_untouched(buf, 1, host.numel(), fill=7) and not mv.margins_untouched(buf, 1, host.numel())
    with pytest.raises(TypeError):
        mv.interior(torch.zeros(4, dtype=torch.int32), 1, "cpu")
    with pytest.raises(ValueError):
        mv.interior(host, -1, "cpu")
