"""The data-dependent Normalize on the device, without a GPU: the project's Normalize class with ``max_val`` / ``min_val``
None is the reference's recorded output bit for bit on the CPU (tests/golden/ingest_data.npz, the specification of
ct_ingest_extrema + ct_ingest_transform_data), ``fusable_ingest_data`` accepts and refuses what its grammar says while
``fusable_ingest`` keeps declining those lists, ``stage_images`` on a CPU device still runs the classes, and the three new
entry points are declared, exported and validate their arguments before any launch."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

from _util import GOLDEN, golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS3 = [(0.0, 1.0), (0.125, 0.7), (-0.25, 0.3333)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _t():
    from clair_torch_amd.common import transforms
    return transforms


def _golden_cases():
    sys.path.insert(0, GOLDEN)
    try:
        import make_golden_ingest_data as gen  # numpy only at import; the reference is needed by its main() alone
    finally:
        sys.path.remove(GOLDEN)
    return gen


# ---- the specification ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["u16_default", "u8_none_0", "u16_4095_none_pm1", "f32_default_range", "f32_none_min"])
def test_normalize_class_with_none_bounds_on_cpu_is_the_reference_bit_for_bit(name):
    T = _t()
    gen = _golden_cases()
    _, _, _, _, mx, mn, rng = gen.CASES[name]
    raw = torch.from_numpy(gen.stack(name))
    want = golden("ingest_data")[name]
    got = T.Normalize(mx, mn, rng)(T.CastTo("float32")(raw))
    assert got.dtype == torch.float32 and np.array_equal(_bits(got.numpy()), _bits(want))
    # ... and the step-by-step float32 sequence the two kernels are specified by
    x = gen.stack(name).astype(np.float32)
    sub = x.min() if mn is None else np.float32(mn)
    top = x.max() if mx is None else np.float32(mx)
    div = np.float32(top - sub)
    t = (x - sub) / div
    t = t * np.float32(rng[1] - rng[0]) + np.float32(rng[0])
    assert t.dtype == np.float32 and np.array_equal(_bits(t), _bits(want))


# ---- the recogniser ---------------------------------------------------------------------------------------------------
def test_fusable_ingest_data_accepts_the_grammar_and_fusable_ingest_declines_it():
    T = _t()
    u16 = torch.zeros((2, 3, 4, 6), dtype=torch.uint16)
    raw = torch.zeros((2, 4, 6, 3), dtype=torch.uint8)
    f32 = torch.zeros((2, 3, 4, 6), dtype=torch.float32)
    cast, cv = T.CastTo("float32"), T.CvToTorch()
    data = ("affine_data", 1.0, 0.0)
    Plan = T.DataIngestPlan
    n4095 = ("affine", 64, 4031, 1.0, 0.0)
    accepted = [
        (u16, [cast, T.Normalize()], Plan("nchw", 1, False, (data,), (), None, None)),
        (u16, [cast, T.Normalize(None, 0)], Plan("nchw", 1, False, (data,), (), 0, None)),
        (u16, [cast, T.Normalize(4095, None)], Plan("nchw", 1, False, (data,), (), None, 4095)),
        (u16, [None, cast, T.Normalize(None, None, (-1, 1))], Plan("nchw", 1, False, (("affine_data", 2, -1),), (), None, None)),
        (f32, [T.Normalize(max_val=None, min_val=0.5, target_range=(0.1, 0.9))],
         Plan("nchw", 1, False, (("affine_data", 0.9 - 0.1, 0.1),), (), 0.5, None)),
        # a prefix, a suffix, both; four stages in all
        (u16, [cast, T.Normalize(4095, 64), T.Normalize()], Plan("nchw", 1, False, (n4095, data), (n4095,), None, None)),
        (u16, [cast, T.Normalize(), T.ClampAlongDims(1, PAIRS3)], Plan("nchw", 1, False, (data, ("clamp", PAIRS3)), (), None, None)),
        (u16, [cast, T.ClampAlongDims(1, PAIRS3), T.Normalize(4095, 64), T.Normalize(None, 0), T.ClampAlongDims(0, (0.1, 0.9))],
         Plan("nchw", 1, False, (("clamp", PAIRS3), n4095, data, ("clamp", [(0.1, 0.9)])), (("clamp", PAIRS3), n4095), 0, None)),
        (u16, [cast, T.Normalize(4095, 64), T.Normalize(4095, 64), T.Normalize(4095, 64), T.Normalize()],
         Plan("nchw", 1, False, (n4095, n4095, n4095, data), (n4095, n4095, n4095), None, None)),
        # raw frames behind a leading CvToTorch
        (raw, [cv, cast, T.Normalize(None, 0)], Plan("nhwc_bgr", 1, False, (data,), (), 0, None)),
        # the downscale on either side of the data-dependent stage
        (u16, [T.StridedDownscale(2), cast, T.Normalize()], Plan("nchw", 2, True, (data,), (), None, None)),
        (u16, [cast, T.StridedDownscale(3), T.Normalize()], Plan("nchw", 3, True, (data,), (), None, None)),
        (u16, [cast, T.Normalize(), T.StridedDownscale(2)], Plan("nchw", 2, False, (data,), (), None, None)),
        (u16, [cast, T.Normalize(4095, 64), T.StridedDownscale(2), T.Normalize(), T.ClampAlongDims(1, PAIRS3)],
         Plan("nchw", 2, True, (n4095, data, ("clamp", PAIRS3)), (n4095,), None, None)),
        (u16, [cast, T.Normalize(), T.ClampAlongDims(1, PAIRS3), T.StridedDownscale(2)],
         Plan("nchw", 2, False, (data, ("clamp", PAIRS3)), (), None, None)),
        (raw, [cv, T.StridedDownscale(2), cast, T.Normalize()], Plan("nhwc_bgr", 2, True, (data,), (), None, None)),
        (raw, [cv, cast, T.Normalize(), T.StridedDownscale(2)], Plan("nhwc_bgr", 2, False, (data,), (), None, None)),
    ]
    for k, (images, ts, want) in enumerate(accepted):
        assert T.fusable_ingest_data(images, ts) == want, k
        assert T.fusable_ingest(images, ts) is None, k
        assert T.fusable_code_normalisation(images, [t for t in ts if t is not None]) is None, k
    assert T.INGEST_MAX_STAGES == 4


def test_fusable_ingest_data_refuses():
    T = _t()
    u16 = torch.zeros((2, 3, 4, 6), dtype=torch.uint16)
    raw = torch.zeros((2, 4, 6, 3), dtype=torch.uint8)
    f32 = torch.zeros((2, 3, 4, 6), dtype=torch.float32)
    cast, cv, norm, free = T.CastTo("float32"), T.CvToTorch(), T.Normalize(4095, 64), T.Normalize()

    class MyNormalize(T.Normalize):  # a subclass may compute anything
        pass

    class Identity(T.BaseTransform):
        def __call__(self, x):
            return x

    refused = {
        "no data-dependent stage (fusable_ingest's list)": (u16, [cast, norm]),
        "the code form": (u16, [cast, T.Normalize(4095, 0)]),
        "two data-dependent Normalizes": (u16, [cast, free, T.Normalize(None, 0)]),
        "a subclass": (u16, [cast, MyNormalize()]),
        "a tensor bound": (u16, [cast, T.Normalize(None, torch.tensor(0.0))]),
        "a bool bound": (u16, [cast, T.Normalize(None, False)]),
        "five stages": (u16, [cast, norm, norm, norm, norm, free]),
        "integer input without CastTo": (u16, [free]),
        "the cast behind the arithmetic": (u16, [free, cast]),
        "CastTo(float64)": (u16, [T.CastTo("float64"), free]),
        "CastTo to a device": (u16, [T.CastTo("float32", device="cpu"), free]),
        "a constant stage with a zero range": (u16, [cast, T.Normalize(64, 64), free]),
        "a target range that is no pair of numbers": (u16, [cast, T.Normalize(None, None, (0.0, None))]),
        "clamp on a spatial dim": (u16, [cast, free, T.ClampAlongDims(2, [(0.0, 1.0)] * 4)]),
        "pair count != C": (u16, [cast, free, T.ClampAlongDims(1, PAIRS3[:2])]),
        "another transform class": (u16, [cast, free, Identity()]),
        "CvToTorch not leading": (raw, [cast, cv, free]),
        "downscale in front of CvToTorch": (raw, [T.StridedDownscale(2), cv, cast, free]),
        "two downscales": (u16, [T.StridedDownscale(2), cast, free, T.StridedDownscale(2)]),
        "StridedDownscale(0)": (u16, [T.StridedDownscale(0), cast, free]),
        "3-D input": (f32[0], [free]),
        "float64 input": (f32.double(), [cast, free]),
        "non-contiguous input": (f32.permute(0, 1, 3, 2), [free]),
        "empty list": (f32, []),
    }
    for what, (images, ts) in refused.items():
        assert T.fusable_ingest_data(images, ts) is None, what


def test_stage_images_on_a_cpu_device_still_runs_the_classes():
    T = _t()
    from clair_torch_amd.inference._staging import stage_images
    cpu = torch.device("cpu")
    rng = np.random.default_rng(3)
    u16 = torch.from_numpy(rng.integers(0, 5000, size=(2, 3, 6, 8)).astype(np.uint16))
    cast = T.CastTo("float32")
    for ts in ([cast, T.Normalize()], [cast, T.Normalize(None, 0)], [cast, T.Normalize(4095, None, (-1, 1))],
               [cast, T.StridedDownscale(2), T.Normalize()], [cast, T.Normalize(), T.StridedDownscale(2)],
               [cast, T.Normalize(4095, 64), T.Normalize(), T.ClampAlongDims(1, PAIRS3)]):
        assert T.fusable_ingest_data(u16, ts) is not None
        want = u16
        for t in ts:
            want = t(want)
        got, max_code, _ = stage_images(u16, cpu, ts)
        assert max_code is None and got.dtype == torch.float32 and got.is_contiguous()
        assert np.array_equal(_bits(got.numpy()), _bits(want.contiguous().numpy()))
    with pytest.raises(ValueError, match="range is zero"):
        stage_images(torch.full((1, 3, 2, 2), 7, dtype=torch.uint8), cpu, [cast, T.Normalize()])


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


def test_new_entry_points_are_declared_exported_and_validate(lib):
    from clair_torch_amd import _native as nv
    from clair_torch_amd import build
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "clair_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint64_t\s+ct_ingest_extrema_workspace\s*\(\s*void\s*\)", header)
    assert re.search(r"\bint\s+ct_ingest_extrema\s*\(", header) and re.search(r"\bint\s+ct_ingest_transform_data\s*\(", header)
    assert re.search(r"#define\s+CT_ABI_VERSION\s+3\b", header)
    assert re.search(r"#define\s+CT_INGEST_AFFINE_DATA\s+2\b", header)
    assert re.search(r"#define\s+CT_EXTREMA_MIN\s+1\b", header) and re.search(r"#define\s+CT_EXTREMA_MAX\s+2\b", header)
    for name in ("ct_ingest_extrema_workspace", "ct_ingest_extrema", "ct_ingest_transform_data"):
        assert name in nv.EXPORTS and hasattr(lib, name), name
    assert "ct_extrema.hip" in build.SOURCES and "ct_ingest.hip" in build.SOURCES
    assert lib.ct_abi_version() == 3 and nv.ABI_VERSION == 3
    assert ctypes.sizeof(nv.IngestStage) == 4 + 4 * 4 + 2 * 4 * 4  # the layout of ct_ingest_stage is what it was
    assert (nv.INGEST_AFFINE_DATA, nv.EXTREMA_MIN, nv.EXTREMA_MAX) == (2, 1, 2)
    U8, U16, F32, NCHW, NHWC, BGR = nv.DTYPE_U8, nv.DTYPE_U16, nv.DTYPE_F32, nv.LAYOUT_NCHW, nv.LAYOUT_NHWC, nv.LAYOUT_NHWC_BGR
    invalid, unsupported, too_large = -1, -2, -5
    fake = ctypes.c_void_p(0x1000)  # never dereferenced: validation fails first
    none, one, data = _stages(), _stages(nv.INGEST_AFFINE), _stages(nv.INGEST_AFFINE_DATA)
    ws_bytes = lib.ct_ingest_extrema_workspace()
    assert ws_bytes > 0 and ws_bytes % 16 == 0

    def extrema(src=fake, dtype=U16, layout=NCHW, n=1, c=3, plane=16, prefix=none, n_prefix=0, from_data=3, ws=fake,
                ws_size=ws_bytes, consts=fake):
        return lib.ct_ingest_extrema(src, dtype, layout, n, c, plane, prefix, n_prefix, from_data, 0.0, 1.0, ws, ws_size, consts, None)

    assert extrema(dtype=3) == invalid and extrema(dtype=-1) == invalid
    assert extrema(layout=3) == invalid
    assert extrema(c=0) == invalid and extrema(n=-1) == invalid and extrema(plane=-16) == invalid
    assert extrema(prefix=one, n_prefix=4) == invalid            # at most 3 stages can stand in front of the fourth
    assert extrema(prefix=one, n_prefix=-1) == invalid
    assert extrema(prefix=None, n_prefix=1) == invalid
    assert extrema(prefix=_stages(7), n_prefix=1) == invalid
    assert extrema(prefix=data, n_prefix=1) == invalid           # the prefix is constant
    assert extrema(from_data=0) == invalid and extrema(from_data=4) == invalid and extrema(from_data=-1) == invalid
    assert extrema(n=0) == invalid and extrema(plane=0) == invalid   # an empty stack has no extrema
    assert extrema(src=None) == invalid
    assert extrema(src=ctypes.c_void_p(0x1001)) == invalid       # uint16 at an odd address
    assert extrema(src=ctypes.c_void_p(0x1002), dtype=F32) == invalid
    assert extrema(ws=None) == invalid and extrema(ws=ctypes.c_void_p(0x1008)) == invalid
    assert extrema(ws_size=ws_bytes - 1) == invalid and extrema(ws_size=0) == invalid
    assert extrema(consts=None) == invalid and extrema(consts=ctypes.c_void_p(0x1002)) == invalid
    assert extrema(dtype=U8, layout=NHWC, c=4) == unsupported and extrema(dtype=U8, layout=BGR, c=1) == unsupported
    by_channel = _stages(nv.INGEST_CLAMP, lo=(0.0, 0.1, 0.0, 0.0))
    assert extrema(dtype=F32, c=5, prefix=by_channel, n_prefix=1) == unsupported
    assert extrema(n=1 << 40, plane=1 << 40) == too_large
    assert extrema(dtype=U8, n=1 << 31, plane=1, prefix=by_channel, n_prefix=1) == too_large

    def ingest(src=fake, dtype=U16, layout=NCHW, n=1, c=3, plane=16, stages=data, n_stages=1, dst=fake, consts=fake):
        return lib.ct_ingest_transform_data(src, dtype, layout, n, c, plane, stages, n_stages, dst, consts, None)

    assert ingest(dtype=3) == invalid and ingest(layout=3) == invalid and ingest(c=0) == invalid
    assert ingest(n=-1) == invalid and ingest(plane=-16) == invalid
    assert ingest(n_stages=5) == invalid and ingest(stages=None) == invalid and ingest(stages=_stages(7)) == invalid
    assert ingest(stages=_stages(nv.INGEST_AFFINE_DATA, nv.INGEST_AFFINE_DATA), n_stages=2) == invalid   # two data stages
    assert ingest(stages=_stages(nv.INGEST_AFFINE, nv.INGEST_AFFINE_DATA, nv.INGEST_CLAMP, nv.INGEST_AFFINE_DATA), n_stages=4) == invalid
    assert ingest(consts=None) == invalid and ingest(consts=ctypes.c_void_p(0x1002)) == invalid
    assert ingest(consts=None, n=0) == invalid                     # ... whatever the size of the stack
    assert ingest(src=None) == invalid and ingest(dst=None) == invalid
    assert ingest(src=ctypes.c_void_p(0x1001)) == invalid and ingest(dst=ctypes.c_void_p(0x1002), dtype=U8) == invalid
    assert ingest(dtype=U8, layout=NHWC, c=4) == unsupported
    assert ingest(dtype=F32, c=5, stages=_stages(nv.INGEST_AFFINE_DATA, nv.INGEST_CLAMP, lo=(0.0, 0.1, 0.0, 0.0)), n_stages=2) == unsupported
    assert ingest(n=0) == 0 and ingest(layout=BGR, n=4, plane=0) == 0   # nothing to do: no launch
    assert ingest(n=0, stages=one) == 0                            # no data stage is a valid list too
    assert ingest(n=1 << 40, plane=1 << 40) == too_large
    # the old entry point refuses the new kind
    assert lib.ct_ingest_transform(fake, U16, NCHW, 1, 3, 16, data, 1, fake, None) == invalid
    assert lib.ct_ingest_transform(fake, U16, NCHW, 0, 3, 16, data, 1, fake, None) == invalid
    assert lib.ct_ingest_transform(fake, U16, NCHW, 0, 3, 16, one, 1, fake, None) == 0


def test_ops_front_end_without_a_device():
    from clair_torch_amd import ops
    host = torch.zeros((1, 3, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.ingest_extrema(host)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.ingest_transform_data(host, [("affine_data", 1.0, 0.0)])
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.ingest_transform(host, [("affine_data", 1.0, 0.0)], consts=torch.zeros(4))
    assert ops.data_stage_prefix([("affine", 64, 4031, 1.0, 0.0), ("affine_data", 1.0, 0.0), ("clamp", [(0.0, 1.0)])]) == \
        [("affine", 64, 4031, 1.0, 0.0)]
    with pytest.raises(ValueError):
        ops.data_stage_prefix([("affine", 64, 4031, 1.0, 0.0)])
    with pytest.raises(ValueError):
        ops.data_stage_prefix([("affine_data", 1.0, 0.0), ("affine_data", 1.0, 0.0)])
    assert ops.ZERO_RANGE == "Normalization range is zero (min == max); cannot normalize."


def test_fake_kernel_of_the_custom_op():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from clair_torch_amd import torch_ops
    prefix = torch_ops.flatten_ingest_stages([("affine", 64, 4031, 1.0, 0.0)], 3)
    with FakeTensorMode():
        frames = torch.empty((2, 5, 7, 3), dtype=torch.uint16)
        for args in ((frames, [], "nhwc_bgr", None, None), (frames, prefix, "nhwc_bgr", 0.0, None), (frames, prefix, "nhwc", None, 4095.0)):
            out = torch.ops.clair_hip.ingest_extrema(*args)
            assert tuple(out.shape) == (4,) and out.dtype == torch.float32
