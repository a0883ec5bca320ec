"""The fused chain + linearization without a GPU: ct_linearize_ingest is declared, exported and validates every argument
before any launch, and ``pipeline_route`` -- the one decision of linearize_dataset_generator between its pipelined and its
frame-by-frame route -- answers for CPU probes what the module docstring says."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, UNSUPPORTED = 0, -1, -2
PAIRS3 = [(0.0, 1.0), (0.125, 0.7), (-0.25, 0.3333)]


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


def _geom(c=3, h=4, w=4, layout=0, h_global=None, row_offset=0):
    from clair_torch_amd import _native as nv
    return nv.Geometry(channels=c, h_tile=h, width=w, h_global=h if h_global is None else h_global, row_offset=row_offset,
                       image_stride=c * h * w, layout=layout)


def test_ct_linearize_ingest_is_declared_and_exported(lib):
    from clair_torch_amd import _native as nv
    from clair_torch_amd import build
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "clair_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+ct_linearize_ingest\s*\(", header)
    assert re.search(r"#define\s+CT_ABI_VERSION\s+3\b", header)
    assert "ct_linearize_ingest" in nv.EXPORTS and hasattr(lib, "ct_linearize_ingest")
    assert "ct_linearize_ingest.hip" in build.SOURCES
    assert lib.ct_abi_version() == 3 and nv.ABI_VERSION == 3
    assert len(lib.ct_linearize_ingest.argtypes) == 13


def test_ct_linearize_ingest_validates_before_any_launch(lib):
    from clair_torch_amd import _native as nv
    U8, U16, F32 = nv.DTYPE_U8, nv.DTYPE_U16, nv.DTYPE_F32
    NCHW, NHWC, BGR = nv.LAYOUT_NCHW, nv.LAYOUT_NHWC, nv.LAYOUT_NHWC_BGR
    fake = ctypes.c_void_p(0x1000)  # never dereferenced: validation fails first, or there is nothing to launch
    icrf = nv.Icrf(lut_dev=0x2000, n_points=256, interp=nv.INTERP_LINEAR)
    one, two = _stages(nv.INGEST_AFFINE), _stages(nv.INGEST_AFFINE, nv.INGEST_CLAMP)

    def call(frames=fake, dtype=U16, n=1, geom=None, stages=one, n_stages=1, std=None, std_mode=nv.STD_NONE, model=icrf,
             lin=fake, std_out=fake):
        geom = _geom() if geom is None else geom
        return lib.ct_linearize_ingest(frames, dtype, n, ctypes.byref(geom), stages, n_stages, std, std_mode, 0.05,
                                       ctypes.byref(model), lin, std_out, None)

    # nothing to do: CT_OK without a launch, for a valid list, for no list at all (the cast alone), in every layout
    assert call(n=0) == OK
    assert call(n=0, stages=two, n_stages=2) == OK
    assert call(n=0, stages=None, n_stages=0) == OK
    assert call(n=0, geom=_geom(layout=BGR), dtype=U8) == OK
    assert call(n=0, std_mode=nv.STD_MULTIPLIER, std_out=None) == OK
    # the stage list
    assert call(stages=_stages(nv.INGEST_AFFINE_DATA)) == INVALID
    assert call(n=0, stages=_stages(nv.INGEST_AFFINE, nv.INGEST_AFFINE_DATA), n_stages=2) == INVALID
    assert call(stages=_stages(*[nv.INGEST_AFFINE] * 5), n_stages=5) == INVALID
    assert call(n_stages=-1) == INVALID
    assert call(stages=_stages(7)) == INVALID
    assert call(stages=None, n_stages=1) == INVALID
    # dtype, layout, geometry
    assert call(dtype=3) == INVALID and call(dtype=-1) == INVALID
    assert call(geom=_geom(layout=3)) == INVALID and call(geom=_geom(layout=-1)) == INVALID
    assert call(geom=_geom(c=0)) == INVALID and call(geom=_geom(h=0)) == INVALID
    assert call(geom=_geom(h=4, h_global=3)) == INVALID and call(geom=_geom(h=4, h_global=6, row_offset=3)) == INVALID
    assert call(n=-1) == INVALID
    # not built: interleaved with C != 3, per-channel pairs for more than 4 channels
    assert call(geom=_geom(c=4, layout=NHWC), dtype=U8) == UNSUPPORTED
    assert call(geom=_geom(c=1, layout=BGR), dtype=U8) == UNSUPPORTED
    by_channel = _stages(nv.INGEST_CLAMP, lo=(0.0, 0.1, 0.0, 0.0))
    assert call(geom=_geom(c=5), dtype=F32, stages=by_channel) == UNSUPPORTED
    assert call(n=0, geom=_geom(c=5), dtype=F32, stages=_stages(nv.INGEST_CLAMP)) == OK  # one pair for all: any C
    # the model and the uncertainty mode, as ct_linearize_std
    assert call(model=nv.Icrf(lut_dev=0x2000, n_points=256, interp=7)) == INVALID
    assert call(model=nv.Icrf(lut_dev=None, n_points=256, interp=nv.INTERP_LINEAR)) == INVALID
    assert call(model=nv.Icrf(lut_dev=0x2000, n_points=1, interp=nv.INTERP_LINEAR)) == INVALID
    assert call(std_mode=4) == INVALID and call(std_mode=-1) == INVALID
    assert call(std_mode=nv.STD_EXPLICIT, std=None) == INVALID
    lookup = nv.Icrf(lut_dev=0x2000, n_points=256, interp=nv.INTERP_LOOKUP)
    assert call(model=lookup, std_mode=nv.STD_MULTIPLIER) == nv.ERR_NO_GRADIENT_PATH
    assert call(n=0, model=lookup) == OK
    assert call(model=nv.Icrf(lut_dev=0x2000, n_points=1 << 20, interp=nv.INTERP_CATMULL)) == -5  # the LUT exceeds the LDS
    assert call(geom=_geom(h=1 << 15, w=1 << 15)) == -5                                            # 2^31 elements per image
    # pointers with n_frames > 0: what ct_linearize_std gives for them
    g, std_geom = _geom(), _geom()
    want = lib.ct_linearize_std(None, U16, 4095.0, 1, ctypes.byref(std_geom), None, nv.STD_NONE, 0.0, ctypes.byref(icrf), fake, fake, None)
    assert want == INVALID and call(frames=None) == want
    want = lib.ct_linearize_std(fake, U16, 4095.0, 1, ctypes.byref(std_geom), None, nv.STD_NONE, 0.0, ctypes.byref(icrf), None, fake, None)
    assert want == INVALID and call(lin=None) == want
    assert call(frames=ctypes.c_void_p(0x1001)) == INVALID                  # uint16 at an odd address
    assert call(lin=ctypes.c_void_p(0x1002)) == INVALID and call(std_out=ctypes.c_void_p(0x1002)) == INVALID
    del g


def _T():
    from clair_torch_amd.common import transforms
    return transforms


def test_pipeline_route():
    T = _T()
    from clair_torch_amd.inference.linearization import pipeline_route
    u16 = torch.zeros((1, 3, 4, 6), dtype=torch.uint16)
    raw = torch.zeros((1, 4, 6, 3), dtype=torch.uint16)
    f32 = torch.zeros((1, 3, 4, 6), dtype=torch.float32)
    cast, cv, sd = T.CastTo("float32"), T.CvToTorch(), T.StridedDownscale(2)
    black = [cast, T.Normalize(4095, 64)]
    clamped = black + [T.ClampAlongDims(1, PAIRS3)]
    pair = [cast, T.Normalize(65535, 0)]

    class Unknown(T.BaseTransform):
        def __call__(self, x):
            return x

    def route(probe, ts, planar=False, dark=False):
        return pipeline_route(probe, T.plan_staging(probe, ts, planar=planar), dark)

    pipelined = {
        "the code pair": (u16, pair, False),
        "the code pair on raw frames": (raw, [cv] + pair, False),
        "float32 without a list": (f32, [], False),
        "a black level": (u16, black, False),
        "a black level and a clamp": (u16, clamped, False),
        "a target range": (u16, [cast, T.Normalize(4095, 0, (-1.0, 1.0))], False),
        "raw frames behind CvToTorch": (raw, [cv] + black, False),
        "raw frames behind CvToTorch, clamped": (raw, [cv] + clamped, False),
        "the code pair on raw frames with explicit std images": (raw, [cv] + pair, True),
        "a black level with explicit std images": (u16, black, True),
        "float32 pixels with a list": (f32, [T.Normalize(2.0, 0.5)], False),
    }
    for what, (probe, ts, planar) in pipelined.items():
        assert route(probe, ts, planar) == "pipelined", what
        assert route(probe, ts, planar, dark=True) == "frame_by_frame", what + ", dark field"
    assert T.plan_staging(raw, [cv] + pair, planar=True).route == "ingest"   # planar=True turns the pair into an ingest plan
    assert T.plan_staging(u16, clamped).route == "ingest" and T.plan_staging(u16, pair).route == "code"
    frame_by_frame = {
        "the code pair with a downscale": (u16, [sd] + pair, False),
        "a black level with a downscale": (u16, [sd] + black, False),
        "a clamp with a downscale": (u16, clamped + [sd], False),
        "raw frames with a downscale": (raw, [cv, sd] + black, False),
        "raw frames, explicit std, a downscale": (raw, [cv] + pair + [sd], True),
        "a data-dependent Normalize": (u16, [cast, T.Normalize()], False),
        "an unknown transform class": (u16, black + [Unknown()], False),
        "an unknown transform class alone on float32": (f32, [Unknown()], False),
        "integer codes without a list": (u16, [], False),
        "a 3-D probe": (f32[0], [], False),
    }
    for what, (probe, ts, planar) in frame_by_frame.items():
        assert route(probe, ts, planar) == "frame_by_frame", what
        assert route(probe, ts, planar, dark=True) == "frame_by_frame", what + ", dark field"
    # on a device the data-dependent list is route "ingest_data": still frame by frame (its extrema are per stack there)
    plan = T.StagingPlan("ingest_data", source_layout="nchw", stages=(("affine_data", 1.0, 0.0),))
    assert pipeline_route(u16, plan, False) == "frame_by_frame"


def test_front_end_without_a_device():
    from clair_torch_amd import ops
    lut = torch.stack([torch.linspace(0, 1, 16)] * 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.linearize_ingest_frames(torch.zeros((1, 3, 4, 4)), [("affine", 0.0, 1.0, 1.0, 0.0)], lut)


def test_fake_kernel_of_the_custom_op():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from clair_torch_amd import torch_ops
    stages = torch_ops.flatten_ingest_stages([("affine", 64, 4031, 1.0, 0.0), ("clamp", PAIRS3)], 3)
    with FakeTensorMode():
        lin, sd = torch.ops.clair_hip.linearize_ingest(torch.empty((2, 5, 7, 3), dtype=torch.uint16), stages, torch.empty((3, 64)),
                                                       "linear", None, "multiplier", 0.05, "nhwc_bgr")
        assert tuple(lin.shape) == tuple(sd.shape) == (2, 3, 5, 7) and lin.dtype == sd.dtype == torch.float32
