"""The fused ingest without a GPU: the project's Normalize / ClampAlongDims classes on the CPU are the reference's recorded
float32 output bit for bit (tests/golden/ingest.npz pins the specification of ct_ingest_transform), ``fusable_ingest``
accepts and refuses what its grammar says, the code-route recognisers answer as before, and ct_ingest_transform is
declared, exported and validates its arguments before any launch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from _util import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# ---- the specification: the classes on the CPU against the reference's recorded output --------------------------------
@pytest.mark.parametrize("name", ["u8_255_16", "u16_65535_256", "u16_4095_64_pm1"])
def test_normalize_class_on_cpu_is_the_reference_bit_for_bit(name):
    from clair_torch_amd.common.transforms import CastTo, Normalize
    g = golden("ingest")
    mx, mn, lo, hi = g[name + "_params"].tolist()
    n = 256 if name.startswith("u8") else 65536
    codes = torch.from_numpy(np.arange(n).astype(np.uint8 if n == 256 else np.uint16))
    got = Normalize(int(mx), int(mn), (lo, hi))(CastTo("float32")(codes))
    assert got.dtype == torch.float32 and np.array_equal(_bits(got.numpy()), _bits(g[name]))
    # ... and the step-by-step float32 sequence the kernel is specified by
    x = np.arange(n, dtype=np.float32)
    t = (x - np.float32(mn)) / np.float32(mx - mn)
    t = t * np.float32(hi - lo) + np.float32(lo)
    assert t.dtype == np.float32 and np.array_equal(_bits(t), _bits(g[name]))


def test_clamp_class_on_cpu_is_the_reference_bit_for_bit():
    from clair_torch_amd.common.transforms import ClampAlongDims
    g = golden("ingest")
    start, end, steps = g["clamp_ramp"].tolist()
    ramp = torch.linspace(start, end, int(steps), dtype=torch.float32)
    x = torch.stack([ramp, ramp, ramp]).view(1, 3, 1, -1)
    pairs = [tuple(p) for p in g["clamp_pairs"].tolist()]
    for dim in (1, -3, (1,)):
        got = ClampAlongDims(dim, pairs)(x)
        assert np.array_equal(_bits(got.numpy()), _bits(g["clamp_per_channel"]))
    want = torch.stack([x[:, c].clamp(min=pairs[c][0], max=pairs[c][1]) for c in range(3)], dim=1)
    assert np.array_equal(_bits(want.numpy()), _bits(g["clamp_per_channel"]))
    got = ClampAlongDims(0, pairs[1])(x)
    assert np.array_equal(_bits(got.numpy()), _bits(g["clamp_single_pair"]))


# ---- the recogniser ---------------------------------------------------------------------------------------------------
def _t():
    from clair_torch_amd.common import transforms
    return transforms


PAIRS3 = [(0.0, 1.0), (0.125, 0.7), (-0.25, 0.3333)]


def test_fusable_ingest_accepts_the_grammar():
    T = _t()
    u16 = torch.zeros((2, 3, 4, 6), dtype=torch.uint16)
    raw = torch.zeros((2, 4, 6, 3), dtype=torch.uint8)
    f32 = torch.zeros((2, 3, 4, 6), dtype=torch.float32)
    cast, cv = T.CastTo("float32"), T.CvToTorch()

    plan = T.fusable_ingest(u16, [cast, T.Normalize(4095, 64), T.ClampAlongDims(1, PAIRS3)])
    assert plan == T.IngestPlan("nchw", 1, (("affine", 64, 4031, 1.0, 0.0), ("clamp", PAIRS3)))
    plan = T.fusable_ingest(u16, [None, cast, None, T.Normalize(1023, 0, (-1, 1))])
    assert plan.stages == (("affine", 0, 1023, 2, -1),)
    plan = T.fusable_ingest(u16, [cast, T.Normalize(16383.0, 63.5, (0.1, 0.9))])
    assert plan.stages == (("affine", 63.5, 16383.0 - 63.5, 0.9 - 0.1, 0.1),)
    # raw frames behind CvToTorch, the downscale in every position after it
    sd = T.StridedDownscale(3)
    for ts in ([cv, sd, cast, T.Normalize(255, 16)], [cv, cast, sd, T.Normalize(255, 16)], [cv, cast, T.Normalize(255, 16), sd]):
        assert T.fusable_ingest(raw, ts) == T.IngestPlan("nhwc_bgr", 3, (("affine", 16, 239, 1.0, 0.0),))
    assert T.fusable_ingest(raw, [cv, cast, T.ClampAlongDims(-3, PAIRS3)]).layout == "nhwc_bgr"
    # the identity cast on float32 input, a repeated cast, a single pair on any dim, clamp -> normalize -> clamp, 4 stages
    assert T.fusable_ingest(f32, [T.Normalize(2.0, 0.5)]).stages == (("affine", 0.5, 1.5, 1.0, 0.0),)
    assert T.fusable_ingest(f32, [cast, T.Normalize(2.0, 0.5), cast]) is not None
    for dim in (0, 2, 3, (0, 1), (2, 3)):
        assert T.fusable_ingest(f32, [T.ClampAlongDims(dim, (0.25, 0.75))]).stages == (("clamp", [(0.25, 0.75)]),)
    four = [T.ClampAlongDims(1, PAIRS3), T.Normalize(1.0, 0.0, (0, 255)), T.ClampAlongDims((1,), PAIRS3), T.Normalize(255, 0)]
    assert len(T.fusable_ingest(u16, [cast] + four).stages) == 4
    # per-channel pairs for 1, 2 and 4 channels; a single pair for any channel count
    for c in (1, 2, 4):
        assert T.fusable_ingest(torch.zeros((1, c, 2, 2)), [T.ClampAlongDims(1, PAIRS3[:1] * c)]) is not None
    assert T.fusable_ingest(torch.zeros((1, 5, 2, 2)), [T.ClampAlongDims(1, (0.0, 1.0))]) is not None
    # StridedDownscale(1) is a downscale that selects everything
    assert T.fusable_ingest(u16, [T.StridedDownscale(1), cast, T.Normalize(4095, 64)]).step == 1


def test_fusable_ingest_refuses():
    T = _t()
    u16 = torch.zeros((2, 3, 4, 6), dtype=torch.uint16)
    raw = torch.zeros((2, 4, 6, 3), dtype=torch.uint8)
    f32 = torch.zeros((2, 3, 4, 6), dtype=torch.float32)
    cast, cv, norm = T.CastTo("float32"), T.CvToTorch(), T.Normalize(4095, 64)

    class Identity(T.BaseTransform):
        def __call__(self, x):
            return x

    class MyNormalize(T.Normalize):  # a subclass may compute anything
        pass

    refused = {
        "integer input without CastTo": (u16, [norm]),
        "integer input, clamp before the cast": (u16, [T.ClampAlongDims(1, PAIRS3), cast, norm]),
        "integer input, the cast after the arithmetic": (u16, [norm, cast]),
        "CastTo(float64)": (u16, [T.CastTo("float64"), norm]),
        "CastTo(float32) then float64": (u16, [cast, norm, T.CastTo("float64")]),
        "CastTo to a device": (u16, [T.CastTo("float32", device="cpu"), norm]),
        "CastTo without a dtype": (u16, [T.CastTo(), norm]),
        "Normalize(None, 0)": (u16, [cast, T.Normalize(None, 0)]),
        "Normalize(4095, None)": (u16, [cast, T.Normalize(4095, None)]),
        "Normalize with a tensor bound": (u16, [cast, T.Normalize(torch.tensor(4095.0), 0)]),
        "zero range": (u16, [cast, T.Normalize(64, 64)]),
        "clamp on dim (0, 1)": (u16, [cast, T.ClampAlongDims((0, 1), PAIRS3 * 2)]),
        "clamp on a spatial dim": (u16, [cast, T.ClampAlongDims(2, [(0.0, 1.0)] * 4)]),
        "clamp on the last dim": (u16, [cast, T.ClampAlongDims(-1, [(0.0, 1.0)] * 6)]),
        "clamp on the batch dim": (u16, [cast, T.ClampAlongDims(0, [(0.0, 1.0)] * 2)]),
        "pair count != C": (u16, [cast, T.ClampAlongDims(1, PAIRS3[:2])]),
        "clamp bound None": (u16, [cast, T.ClampAlongDims(1, (None, 1.0))]),
        "5 stages": (u16, [cast] + [norm] * 5),
        "no arithmetic stage": (u16, [cast]),
        "CvToTorch not leading": (raw, [cast, cv, norm]),
        "CvToTorch twice": (raw, [cv, cv, cast, norm]),
        "CvToTorch on a planar float stack": (f32, [cv, norm]),
        "downscale in front of CvToTorch": (raw, [T.StridedDownscale(2), cv, cast, norm]),
        "two downscales": (u16, [T.StridedDownscale(2), cast, norm, T.StridedDownscale(2)]),
        "StridedDownscale(0)": (u16, [T.StridedDownscale(0), cast, norm]),
        "C = 5 with per-channel pairs": (torch.zeros((1, 5, 2, 2)), [T.ClampAlongDims(1, [(0.0, 1.0)] * 5)]),
        "another transform class": (u16, [cast, norm, Identity()]),
        "a subclass of a recognised class": (u16, [cast, MyNormalize(4095, 64)]),
        "TorchToCv": (f32, [norm, T.TorchToCv()]),
        "3-D input": (f32[0], [norm]),
        "float64 input": (f32.double(), [cast, norm]),
        "int32 input": (torch.zeros((2, 3, 4, 6), dtype=torch.int32), [cast, norm]),
        "non-contiguous input": (f32.permute(0, 1, 3, 2), [norm]),
        "empty list": (f32, []),
    }
    for what, (images, ts) in refused.items():
        assert T.fusable_ingest(images, ts) is None, what


def test_declined_lists_behave_as_before_on_the_torch_route():
    """stage_images on a CPU 'device' exercises the routing alone: a list the recogniser declines runs the classes."""
    T = _t()
    from clair_torch_amd.inference._staging import stage_images
    cpu = torch.device("cpu")
    u16 = torch.from_numpy(np.arange(2 * 3 * 4 * 6, dtype=np.uint16).reshape(2, 3, 4, 6) * 300)
    cast = T.CastTo("float32")
    with pytest.raises(ValueError, match="range is zero"):
        stage_images(u16, cpu, [cast, T.Normalize(64, 64)])
    with pytest.raises(ValueError, match="min/max pairs"):
        stage_images(u16, cpu, [cast, T.Normalize(4095, 64), T.ClampAlongDims(1, PAIRS3[:2])])
    got, max_code, _ = stage_images(u16, cpu, [cast, T.Normalize(None, 0)])
    assert max_code is None and torch.equal(got, u16.to(torch.float32) / float(u16.to(torch.float32).max()))
    got, max_code, layout = stage_images(u16, cpu, [cast, T.Normalize(4095, 64), T.ClampAlongDims(2, [(0.0, 1.0)] * 4)])
    assert max_code is None and layout == "nchw" and got.dtype == torch.float32


def test_code_route_recognisers_answer_as_before():
    T = _t()
    cast, cv, sd = T.CastTo("float32"), T.CvToTorch(), T.StridedDownscale(2)
    for dtype, mx in ((torch.uint8, 255), (torch.uint16, 65535), (torch.uint16, 4095)):
        planar, raw = torch.zeros((2, 3, 4, 6), dtype=dtype), torch.zeros((2, 4, 6, 3), dtype=dtype)
        norm = T.Normalize(mx, 0)
        assert T.fusable_code_normalisation(planar, [cast, norm]) == float(mx)
        assert T.fusable_layout(raw, [cv, cast, norm])[0] == "nhwc_bgr"
        assert T.fusable_code_normalisation(raw, T.fusable_layout(raw, [cv, cast, norm])[1]) == float(mx)
        for ts in ([sd, cast, norm], [cast, sd, norm], [cast, norm, sd]):
            step, rest = T.fusable_downscale(ts)
            assert step == 2 and rest == [cast, norm]
            step, rest = T.fusable_downscale([cv] + ts, raw)
            assert step == 2 and rest == [cv, cast, norm]
    # what the fused ingest takes is not the code form
    planar = torch.zeros((2, 3, 4, 6), dtype=torch.uint16)
    for ts in ([cast, T.Normalize(4095, 64)], [cast, T.Normalize(4095, 0, (-1, 1))],
               [cast, T.Normalize(4095, 0), T.ClampAlongDims(1, PAIRS3)]):
        assert T.fusable_code_normalisation(planar, ts) is None
        assert T.fusable_downscale([sd] + ts) == (None, [sd] + ts)
        assert T.fusable_ingest(planar, ts) is not None and T.fusable_ingest(planar, [sd] + ts).step == 2


# ---- the C ABI -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from clair_torch_amd import build, _native
    build.build()
    return _native.load()


def _stages(*kinds, lo=(0.0, 0.0, 0.0, 0.0), hi=(1.0, 1.0, 1.0, 1.0)):
    from clair_torch_amd import _native as nv
    arr = (nv.IngestStage * max(len(kinds), 1))()
    for k, kind in enumerate(kinds):
        arr[k].kind, arr[k].sub, arr[k].div, arr[k].mul, arr[k].add = kind, 64.0, 4031.0, 1.0, 0.0
        for c in range(4):
            arr[k].lo[c], arr[k].hi[c] = lo[c], hi[c]
    return arr


def test_ct_ingest_transform_is_declared_exported_and_validates(lib):
    from clair_torch_amd import _native as nv
    from clair_torch_amd import build
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "clair_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+ct_ingest_transform\s*\(", header)
    assert re.search(r"#define\s+CT_ABI_VERSION\s+3\b", header)
    assert "ct_ingest_transform" in nv.EXPORTS and hasattr(lib, "ct_ingest_transform")
    assert "ct_ingest.hip" in build.SOURCES
    assert lib.ct_abi_version() == 3 and nv.ABI_VERSION == 3
    assert ctypes.sizeof(nv.IngestStage) == 4 + 4 * 4 + 2 * 4 * 4
    U8, U16, F32, NCHW, NHWC, BGR = nv.DTYPE_U8, nv.DTYPE_U16, nv.DTYPE_F32, nv.LAYOUT_NCHW, nv.LAYOUT_NHWC, nv.LAYOUT_NHWC_BGR
    fake = ctypes.c_void_p(0x1000)  # never dereferenced: validation fails first
    one = _stages(nv.INGEST_AFFINE)
    call = lib.ct_ingest_transform
    invalid, unsupported, too_large = -1, -2, -5
    assert call(fake, 3, NCHW, 1, 3, 16, one, 1, fake, None) == invalid      # dtype
    assert call(fake, -1, NCHW, 1, 3, 16, one, 1, fake, None) == invalid
    assert call(fake, U16, 3, 1, 3, 16, one, 1, fake, None) == invalid       # layout
    assert call(fake, U16, NCHW, 1, 0, 16, one, 1, fake, None) == invalid    # channels
    assert call(fake, U16, NCHW, -1, 3, 16, one, 1, fake, None) == invalid   # negative sizes
    assert call(fake, U16, NCHW, 1, 3, -16, one, 1, fake, None) == invalid
    assert call(fake, U16, NCHW, 1, 3, 16, one, 5, fake, None) == invalid    # stage count
    assert call(fake, U16, NCHW, 1, 3, 16, one, -1, fake, None) == invalid
    assert call(fake, U16, NCHW, 1, 3, 16, None, 1, fake, None) == invalid   # stages missing
    assert call(fake, U16, NCHW, 1, 3, 16, _stages(7), 1, fake, None) == invalid  # unknown kind
    assert call(None, U16, NCHW, 1, 3, 16, one, 1, fake, None) == invalid    # null pointers
    assert call(fake, U16, NCHW, 1, 3, 16, one, 1, None, None) == invalid
    assert call(ctypes.c_void_p(0x1001), U16, NCHW, 1, 3, 16, one, 1, fake, None) == invalid  # uint16 at an odd address
    assert call(ctypes.c_void_p(0x1002), F32, NCHW, 1, 3, 16, one, 1, fake, None) == invalid
    assert call(fake, U8, NCHW, 1, 3, 16, one, 1, ctypes.c_void_p(0x1002), None) == invalid
    # not built: interleaved with C != 3, per-channel pairs for more than 4 channels
    assert call(fake, U8, NHWC, 1, 4, 16, one, 1, fake, None) == unsupported
    assert call(fake, U8, BGR, 1, 1, 16, one, 1, fake, None) == unsupported
    by_channel = _stages(nv.INGEST_CLAMP, lo=(0.0, 0.1, 0.0, 0.0))
    assert call(fake, F32, NCHW, 1, 5, 16, by_channel, 1, fake, None) == unsupported
    # nothing to do: no launch (no stage at all is the cast alone and valid)
    assert call(fake, U16, NCHW, 0, 3, 16, one, 1, fake, None) == 0
    assert call(fake, U16, BGR, 4, 3, 0, one, 1, fake, None) == 0
    assert call(fake, U16, NCHW, 0, 3, 16, None, 0, fake, None) == 0
    # more elements than can be addressed / planes than are counted
    assert call(fake, U16, NCHW, 1 << 40, 3, 1 << 40, one, 1, fake, None) == too_large
    assert call(fake, U8, NCHW, 1 << 31, 3, 1, by_channel, 1, fake, None) == too_large
    assert call(fake, U8, BGR, 1 << 32, 3, 1, one, 1, fake, None) == too_large
    assert call(fake, U8, NCHW, 1, 1, 1 << 58, one, 1, fake, None) == too_large


def test_ops_ingest_transform_front_end_without_a_device():
    from clair_torch_amd import ops
    assert ops.ingest_shape((2, 3, 5, 7)) == (2, 3, 5, 7)
    assert ops.ingest_shape((2, 5, 7, 3), "nhwc_bgr") == (2, 3, 5, 7)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.ingest_transform(torch.zeros((1, 3, 4, 4)), [("affine", 0.0, 1.0, 1.0, 0.0)])


def test_fake_kernel_of_the_custom_op():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from clair_torch_amd import torch_ops
    stages = torch_ops.flatten_ingest_stages([("affine", 64, 4031, 1.0, 0.0), ("clamp", PAIRS3)], 3)
    assert len(stages) == 26 and stages[13] == 1.0 and stages[18:21] == [0.0, 0.125, -0.25]
    with FakeTensorMode():
        out = torch.ops.clair_hip.ingest_transform(torch.empty((2, 5, 7, 3), dtype=torch.uint16), stages, "nhwc_bgr")
        assert tuple(out.shape) == (2, 3, 5, 7) and out.dtype == torch.float32
