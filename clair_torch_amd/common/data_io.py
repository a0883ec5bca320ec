"""ICRF curve text I/O with the reference's on-disk conventions (clair_torch/common/data_io.py:23-100): by default
the file holds the curve as (L, C) columns in BGR order; in memory the model wants (C, L) rows in RGB order.

Image output (clair_torch/common/data_io.py:207-238): ``save_image`` with the reference's signature.  The array it
writes -- cast to the file's dtype, (H, W, C), a 3-channel image reversed to BGR -- is made on the device for float32 /
float64 device tensors (``ops.export_cv``), so the device-to-host copy already carries the final bytes; the encoder is
``cv2.imwrite`` when OpenCV is installed, or any ``writer`` callable.  Decoding (``load_image``, video frames) is not part
of this package."""
from pathlib import Path
from typing import Callable, Optional, Sequence

import numpy as np
import torch

from .enums import ChannelOrder, DimensionOrder
from .typecheck import expect


def _validate_input_txt(path: Path):
    # clair_torch/validation/io_checks.py: existence, file-ness and suffix, with the reference's error types
    if not path.exists():
        raise FileNotFoundError(f"File {path} doesn't exist.")
    if not path.is_file():
        raise ValueError(f"Expected a filepath, got {path}")
    if path.suffix != ".txt":
        raise ValueError(f"Expected .txt filetype, got {path.suffix}")


def load_icrf_txt(path, source_channel_order: ChannelOrder = ChannelOrder.BGR,
                  source_dimension_order: DimensionOrder = DimensionOrder.BSC) -> torch.Tensor:
    """Load an ICRF as a float32 (C, L) RGB tensor (reference data_io.py:23-62)."""
    expect(path, (str, Path), "path")
    expect(source_channel_order, ChannelOrder, "source_channel_order")
    expect(source_dimension_order, DimensionOrder, "source_dimension_order")
    path = Path(path)
    _validate_input_txt(path)
    try:
        data = torch.from_numpy(np.loadtxt(path)).float()
    except Exception as e:
        raise IOError(f"Failed to load NumPy array from {path}: {e}")
    if source_dimension_order == DimensionOrder.BSC:
        data = torch.transpose(data, 0, 1)
    if source_channel_order == ChannelOrder.BGR:
        data = data[[2, 1, 0], :]
    return data


def save_icrf_txt(icrf: torch.Tensor, path, target_channel_order: ChannelOrder = ChannelOrder.BGR,
                  target_dimension_order: DimensionOrder = DimensionOrder.BSC) -> None:
    """Save a (C, L) RGB ICRF tensor (reference data_io.py:65-100)."""
    expect(icrf, torch.Tensor, "icrf")
    expect(path, (str, Path), "path")
    expect(target_channel_order, ChannelOrder, "target_channel_order")
    expect(target_dimension_order, DimensionOrder, "target_dimension_order")
    path = Path(path)
    data = icrf.detach().cpu()
    if target_channel_order == ChannelOrder.BGR:
        data = data[[2, 1, 0], :]
    if target_dimension_order == DimensionOrder.BSC:
        data = torch.transpose(data, 0, 1)
    try:
        np.savetxt(path, data.numpy())
    except Exception:
        raise IOError(f"Couldn't save data to path {path}")


def _host_cv_array(tensor: torch.Tensor, dtype: np.dtype) -> np.ndarray:
    # data_io.py:225-234, verbatim
    if tensor.is_cuda:
        tensor = tensor.cpu()
    array = tensor.detach().numpy().astype(dtype=dtype)
    if array.ndim == 3:
        array = np.transpose(array, (1, 2, 0))
        if array.shape[2] == 3:
            array = array[:, :, [2, 1, 0]]
    return array


_DEVICE_EXPORT = {np.dtype("float32"): torch.float32, np.dtype("float64"): torch.float64}


def image_to_cv_array(tensor: torch.Tensor, dtype: np.dtype = np.dtype("float64")) -> np.ndarray:
    """The array ``save_image`` passes to ``cv.imwrite`` for ``tensor`` (C, H, W) or (H, W) (reference data_io.py:225-234).

    A float32 / float64 device tensor asked for as float32 / float64 is cast, interleaved and reversed by ``ops.export_cv``
    on the device and crosses to the host once, into pinned memory, in its final form; the returned array is a view of
    that memory.  Everything else (CPU tensors, other dtypes) goes through the reference's host expression."""
    expect(tensor, torch.Tensor, "tensor")
    dtype = np.dtype(dtype)
    if not (tensor.is_cuda and tensor.dtype in _DEVICE_EXPORT.values() and dtype in _DEVICE_EXPORT and tensor.ndim in (2, 3)):
        return _host_cv_array(tensor, dtype)
    from .. import ops
    out = ops.export_cv(tensor.detach().contiguous(), _DEVICE_EXPORT[dtype])
    host = torch.empty(out.shape, dtype=out.dtype, pin_memory=True)
    host.copy_(out, non_blocking=True)
    torch.cuda.current_stream(tensor.device).synchronize()
    return host.numpy()


def save_image(tensor: torch.Tensor, image_save_path, dtype: np.dtype = np.dtype("float64"),
               params: Optional[Sequence[int]] = None, writer: Optional[Callable] = None) -> None:
    """Save a (C, H, W) or (H, W) tensor as an image file (reference data_io.py:207-238).

    ``writer`` (extension): a callable ``(path_str, array, params) -> bool`` used in place of ``cv2.imwrite``, e.g. where
    OpenCV is not installed."""
    expect(tensor, torch.Tensor, "tensor")
    expect(image_save_path, (str, Path), "image_save_path")
    image_save_path = Path(image_save_path)
    if writer is None:
        try:
            import cv2
        except ImportError as e:
            raise ImportError("save_image needs OpenCV (cv2.imwrite), which is not installed: install opencv-python or "
                              "pass writer=, a callable (path_str, array, params) -> bool") from e
        writer = cv2.imwrite
    elif not callable(writer):
        raise TypeError(f"writer must be callable, got {type(writer)}")
    image_save_path.parent.mkdir(parents=True, exist_ok=True)
    if not image_save_path.parent.exists():
        raise IOError(f"Couldn't create the directory structure for path {image_save_path}")
    array = image_to_cv_array(tensor, dtype)
    success = writer(str(image_save_path), array, params or [])
    if not success:
        raise IOError(f"Failed to save image to {image_save_path}")
