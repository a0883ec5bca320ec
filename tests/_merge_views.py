"""Helpers of tests/test_gpu_merge_alignment.py (importable without a GPU; tests/test_merge_views_host.py covers them).

``interior`` puts a tensor at a chosen distance from a 256-byte boundary inside a larger buffer that holds a sentinel bit pattern
everywhere else, ``margins_untouched`` / ``fully_written`` read that pattern back, and ``merge_batch`` / ``merge_batches`` call
ct_hdr_merge_batch / ct_hdr_merge_batches with every pointer taken from the caller: the ``ops`` fronts allocate their own
outputs, and where an output lies is what those tests are about."""
import ctypes

import torch

BOUNDARY = 256          # bytes: every lead is relative to such a boundary (more than any packet of the merge kernels)
SENTINEL = -7.25        # float buffers: finite, so a margin that was read and merged would also show as a changed value
_SENTINEL_CODE = {torch.uint8: 0xA5, torch.uint16: 0xA5A5 - 0x10000}    # (uint16 through its int16 alias)
_BITS = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
DTYPES = (torch.uint8, torch.uint16, torch.float32, torch.float64)


def _alias(dtype):
    """torch has no uint16 fill / copy / compare kernels: such buffers are held as int16."""
    return torch.int16 if dtype == torch.uint16 else dtype


def _element_size(dtype):
    return torch.empty((), dtype=dtype).element_size()


def guard_elems(dtype):
    """Elements of one whole 256-byte block: what ``interior`` keeps on either side of a view besides ``lead`` and ``tail``."""
    return BOUNDARY // _element_size(dtype)


def default_fill(dtype):
    if dtype not in DTYPES:
        raise TypeError(f"{dtype}: uint8, uint16, float32 or float64")
    return _SENTINEL_CODE.get(dtype, SENTINEL)


def _pattern(dtype, fill):
    """The bit pattern of ``fill`` in a buffer of (the alias of) ``dtype``, as an integer of that width."""
    return int(torch.tensor([fill], dtype=_alias(dtype)).view(_BITS[_element_size(dtype)]).item())


def interior(host, lead_elems, device, tail=19, fill=None):
    """``host`` (uint8, uint16, float32 or float64) on ``device`` as a contiguous view that starts ``lead_elems`` elements behind a
    256-byte boundary of a larger buffer whose every other element holds ``fill`` (default: ``default_fill``).  -> (view, buffer):
    ``buffer`` is flat, of the alias dtype (int16 for uint16), starts at a 256-byte boundary and holds one block of 256 bytes +
    ``lead_elems`` elements in front of the view and ``tail`` elements + one such block behind it."""
    if host.dtype not in DTYPES:
        raise TypeError(f"{host.dtype}: uint8, uint16, float32 or float64")
    if lead_elems < 0 or tail < 0:
        raise ValueError("lead_elems and tail are element counts")
    alias, size, guard = _alias(host.dtype), host.element_size(), guard_elems(host.dtype)
    fill = default_fill(host.dtype) if fill is None else fill
    n = host.numel()
    total = 2 * guard + lead_elems + n + tail
    raw = torch.full((total + guard,), fill, dtype=alias, device=device)        # one more block: the allocation may start anywhere
    skip = (-raw.data_ptr() % BOUNDARY) // size
    assert (raw.data_ptr() + skip * size) % BOUNDARY == 0, "allocations are aligned to their element"
    buffer = raw[skip:skip + total]
    first = guard + lead_elems
    buffer[first:first + n].copy_(host.contiguous().view(alias).reshape(-1).to(device))
    view = buffer.view(host.dtype)[first:first + n].view(host.shape)
    assert view.is_contiguous() and buffer.data_ptr() % BOUNDARY == 0
    assert view.data_ptr() % 16 == (lead_elems * size) % 16 and view.data_ptr() - buffer.data_ptr() == first * size
    return view, buffer


def sentinel_like(shape, dtype, lead_elems, device, tail=19, fill=None):
    """An output or state array for a kernel to write: ``interior`` of a tensor that itself holds the sentinel everywhere."""
    fill = default_fill(dtype) if fill is None else fill
    return interior(torch.full(tuple(shape), fill, dtype=_alias(dtype)).view(dtype), lead_elems, device, tail, fill)


def _same_bits(part, dtype, fill):
    return part.view(_BITS[_element_size(dtype)]) == _pattern(dtype, default_fill(dtype) if fill is None else fill)


def _dtype_of(buffer):
    return torch.uint16 if buffer.dtype == torch.int16 else buffer.dtype


def margins_untouched(buffer, lead, n, fill=None):
    """Do both margins of a ``buffer`` of ``interior(..., lead, ...)`` around its view of ``n`` elements still hold the sentinel,
    bit for bit?"""
    dtype = _dtype_of(buffer)
    first = guard_elems(dtype) + lead
    if first + n > buffer.numel():
        raise ValueError("the view does not lie inside the buffer")
    return bool(_same_bits(buffer[:first], dtype, fill).all()) and bool(_same_bits(buffer[first + n:], dtype, fill).all())


def all_sentinel(buffer, fill=None):
    """Does the whole buffer, view included, still hold the sentinel (a refused call wrote nothing)?"""
    return bool(_same_bits(buffer, _dtype_of(buffer), fill).all())


def fully_written(buffer, lead, n, fill=None):
    """Does no element of the view hold the sentinel any more?"""
    dtype = _dtype_of(buffer)
    first = guard_elems(dtype) + lead
    return not bool(_same_bits(buffer[first:first + n], dtype, fill).any())


# ---- ct_hdr_merge_batch / ct_hdr_merge_batches with the caller's pointers ------------------------------------------------------
def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _merge_tail(stack, layout, std_mode, std_value, exposures, n_exposures, lut, interp, gaussian_weight, state, mean_out, std_out, flags):
    """The arguments both entry points share behind the stack(s), and what they point to (kept alive by the caller's frame)."""
    from clair_torch_amd import _native as nv
    from clair_torch_amd import ops
    dev = stack.device
    c = ops._chw(stack, layout)[0]
    geom = ops._geometry(stack, None, layout)
    icrf, lut_keep = ops._icrf_struct(lut, interp, c)
    exposure_dev = ops._exposures_to_device(exposures, n_exposures, dev)
    mean_state, sumw_state, var_state = state if state is not None else (None, None, None)
    args = (ctypes.byref(geom), ops._STD[std_mode], float(std_value), _ptr(exposure_dev), ctypes.byref(icrf),
            nv.WEIGHT_GAUSS if gaussian_weight else nv.WEIGHT_NONE, _ptr(mean_state), _ptr(sumw_state), _ptr(var_state), _ptr(mean_out),
            _ptr(std_out), int(flags), ops._stream(dev))
    return args, (geom, icrf, lut_keep, exposure_dev)


def merge_batch(stack, exposures, *, max_code=None, std=None, std_mode="none", std_value=0.0, lut=None, interp="linear",
                gaussian_weight=True, layout="nchw", state=None, mean_out=None, std_out=None, flags=0):
    """ct_hdr_merge_batch on exactly these tensors -> its status.  ``stack`` (B,C,H,W) or (B,H,W,C) by ``layout``; ``std`` the
    explicit uncertainties (then ``std_mode`` is "explicit"); ``state`` None or (mean, sumw, var | None); ``flags`` the CT_MERGE_*
    word as it is (nothing is added)."""
    from clair_torch_amd import _native as nv
    from clair_torch_amd import ops
    if std is not None:
        std_mode = "explicit"
    b = stack.shape[0]
    tail, keep = _merge_tail(stack, layout, std_mode, std_value, exposures, b, lut, interp, gaussian_weight, state, mean_out, std_out, flags)
    with torch.cuda.device(stack.device):
        rc = nv.load().ct_hdr_merge_batch(_ptr(stack), ops._DTYPE[stack.dtype], float(ops._default_max_code(stack, max_code) or 1.0), b,
                                          tail[0], _ptr(std), *tail[1:])
    del keep
    return rc


def merge_batches(stacks, exposures, *, max_code=None, stds=None, std_mode="none", std_value=0.0, lut=None, interp="linear",
                  gaussian_weight=True, layout="nchw", state=None, mean_out=None, std_out=None, flags=0):
    """ct_hdr_merge_batches on exactly these tensors -> its status.  ``stacks`` / ``stds``: lists, one entry per batch;
    ``exposures``: the times of all batches, one after the other."""
    from clair_torch_amd import _native as nv
    from clair_torch_amd import ops
    if stds is not None:
        std_mode = "explicit"
    sizes = [int(t.shape[0]) for t in stacks]
    k = len(stacks)
    s0 = stacks[0]
    tail, keep = _merge_tail(s0, layout, std_mode, std_value, exposures, sum(sizes), lut, interp, gaussian_weight, state, mean_out,
                             std_out, flags)
    with torch.cuda.device(s0.device):
        rc = nv.load().ct_hdr_merge_batches(ops._pointers(stacks), ops._pointers(stds), (ctypes.c_int32 * k)(*sizes), k, ops._DTYPE[s0.dtype],
                                            float(ops._default_max_code(s0, max_code) or 1.0), *tail)
    del keep
    return rc
