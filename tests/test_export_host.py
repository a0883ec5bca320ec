"""The save path without a GPU (clair_torch/common/data_io.py:207-238): image_to_cv_array on CPU tensors is the
reference's host expression, save_image creates directories, hands the array to the writer and reports its failure, and
ct_export_cv is declared, exported and validates its arguments before any launch."""
import builtins
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def reference_cv_array(tensor, dtype):
    """data_io.py:228-234."""
    array = tensor.detach().numpy().astype(dtype=dtype)
    if array.ndim == 3:
        array = np.transpose(array, (1, 2, 0))
        if array.shape[2] == 3:
            array = array[:, :, [2, 1, 0]]
    return array


@pytest.mark.parametrize("dst", ["float32", "float64"])
@pytest.mark.parametrize("src", [torch.float32, torch.float64])
@pytest.mark.parametrize("shape", [(3, 5, 7), (1, 5, 7), (2, 5, 7), (4, 5, 7), (5, 7)])
def test_image_to_cv_array_on_cpu_is_the_reference_expression(shape, src, dst):
    from clair_torch_amd.common import image_to_cv_array
    rng = np.random.default_rng(len(shape) + shape[0])
    t = torch.from_numpy(rng.standard_normal(shape) * 10.0 ** rng.integers(-30, 30, size=shape)).to(src)
    want = reference_cv_array(t, np.dtype(dst))
    got = image_to_cv_array(t, np.dtype(dst))
    assert isinstance(got, np.ndarray) and got.dtype == np.dtype(dst) and got.shape == want.shape
    assert got.shape == ((shape[1], shape[2], shape[0]) if len(shape) == 3 else shape)
    assert np.array_equal(got, want)
    if shape[0] == 3 and len(shape) == 3:
        assert np.array_equal(got[..., 0], t[2].numpy().astype(dst))  # BGR


def test_image_to_cv_array_default_dtype_and_integer_dtype():
    from clair_torch_amd.common import image_to_cv_array
    t = torch.arange(3 * 4 * 5, dtype=torch.float32).view(3, 4, 5)
    assert image_to_cv_array(t).dtype == np.float64
    got = image_to_cv_array(t, np.dtype("uint16"))  # integer files keep the host expression
    assert got.dtype == np.uint16 and np.array_equal(got, reference_cv_array(t, np.dtype("uint16")))


def test_save_image_with_a_recording_writer(tmp_path):
    from clair_torch_amd.common import save_image
    calls = []

    def writer(path, array, params):
        calls.append((path, array, params))
        return True

    t = torch.from_numpy(np.random.default_rng(0).random((3, 5, 7)))
    target = tmp_path / "a" / "b" / "image.tif"
    assert save_image(t, target, writer=writer) is None
    assert target.parent.is_dir()
    save_image(t, str(tmp_path / "c" / "image.tif"), np.dtype("float32"), [259, 1], writer=writer)  # str paths too
    assert (tmp_path / "c").is_dir()
    (p0, a0, k0), (p1, a1, k1) = calls
    assert isinstance(p0, str) and p0 == str(target) and k0 == []
    assert a0.dtype == np.float64 and np.array_equal(a0, reference_cv_array(t, np.dtype("float64")))
    assert p1 == str(tmp_path / "c" / "image.tif") and k1 == [259, 1]
    assert a1.dtype == np.float32 and np.array_equal(a1, reference_cv_array(t, np.dtype("float32")))
    with pytest.raises(IOError, match="Failed to save"):
        save_image(t, tmp_path / "d" / "image.tif", writer=lambda path, array, params: False)


def test_save_image_without_writer_and_without_opencv(tmp_path, monkeypatch):
    from clair_torch_amd.common import save_image
    real_import = builtins.__import__

    def no_cv2(name, *args, **kwargs):
        if name == "cv2" or name.startswith("cv2."):
            raise ImportError("No module named 'cv2'")
        return real_import(name, *args, **kwargs)

    monkeypatch.setattr(builtins, "__import__", no_cv2)
    with pytest.raises(ImportError, match="writer") as info:
        save_image(torch.zeros(3, 2, 2), tmp_path / "x.tif")
    assert "cv2" in str(info.value) or "OpenCV" in str(info.value)


def test_alias_package_resolves_the_save_path():
    import clair_torch.common.data_io as alias_io
    import clair_torch_amd.common as common
    assert alias_io.save_image is common.save_image
    assert alias_io.image_to_cv_array is common.image_to_cv_array


@pytest.fixture(scope="module")
def lib():
    from clair_torch_amd import build, _native
    build.build()
    return _native.load()


def test_ct_export_cv_is_declared_exported_and_validates(lib):
    from clair_torch_amd import _native as nv
    header = open(os.path.join(ROOT, "include", "clair_hip.h")).read()
    assert re.search(r"\bint\s+ct_export_cv\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    assert "ct_export_cv" in nv.EXPORTS and hasattr(lib, "ct_export_cv")
    assert lib.ct_abi_version() == 3
    fake = ctypes.c_void_p(0x1000)  # never dereferenced: validation fails first
    invalid = -1
    assert lib.ct_export_cv(fake, 0, fake, 0, 1, 0, 16, 0, None) == invalid   # channels = 0
    assert lib.ct_export_cv(fake, 0, fake, 0, 1, -3, 16, 1, None) == invalid
    assert lib.ct_export_cv(None, 0, fake, 0, 1, 3, 16, 1, None) == invalid   # null pointers
    assert lib.ct_export_cv(fake, 1, None, 1, 1, 3, 16, 1, None) == invalid
    assert lib.ct_export_cv(fake, 0, fake, 0, -1, 3, 16, 1, None) == invalid  # negative sizes
    assert lib.ct_export_cv(fake, 0, fake, 0, 1, 3, -16, 1, None) == invalid
    assert lib.ct_export_cv(ctypes.c_void_p(0x1004), 1, fake, 1, 1, 3, 16, 1, None) == invalid  # float64 at 4 (mod 8)
    # nothing to do: no launch
    assert lib.ct_export_cv(fake, 0, fake, 0, 0, 3, 16, 1, None) == 0
    assert lib.ct_export_cv(fake, 0, fake, 0, 4, 3, 0, 1, None) == 0
    # more elements than can be addressed / than one grid covers
    too_large = -5
    assert lib.ct_export_cv(fake, 0, fake, 0, 1 << 40, 3, 1 << 40, 1, None) == too_large
    assert lib.ct_export_cv(fake, 0, fake, 0, 1 << 20, 2, 1 << 20, 0, None) == too_large
    assert lib.ct_export_cv(fake, 0, fake, 0, 1, 3, 1 << 36, 1, None) == too_large


def test_export_shape_and_cpu_refusal():
    from clair_torch_amd import ops
    assert ops.export_shape((5, 7)) == (5, 7)
    assert ops.export_shape((3, 5, 7)) == (5, 7, 3)
    assert ops.export_shape((2, 3, 5, 7)) == (2, 5, 7, 3)
    with pytest.raises(ValueError):
        ops.export_shape((7,))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.export_cv(torch.zeros(3, 4, 4))
