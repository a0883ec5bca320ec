"""StridedDownscale lists on the linearize pipeline, without a GPU: for the plan linearize_dataset_generator makes --
``plan_staging(..., step_in_kernel=True)``: the step is ct_linearize_ingest_strided's to apply -- ``pipeline_route`` /
``pipeline_data_route`` send a list with a downscale to the pipeline (the data-dependent one only when the Normalize stands
in front of the downscale); for a plan that leaves the step to the staging they answer what they always did;
ct_linearize_ingest_strided is declared, bound and refuses every malformed call before any launch, and the ops front checks
its arguments."""
import ctypes
import dataclasses
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS3 = [(0.0, 1.0), (0.1, 0.9), (0.0, 0.5)]


@pytest.fixture(scope="module")
def lib():
    from clair_torch_amd import build, _native
    build.build()
    return _native.load()


def _T():
    from clair_torch_amd.common import transforms
    return transforms


def test_pipeline_route_takes_downscale_lists():
    T = _T()
    from clair_torch_amd.inference.linearization import pipeline_route
    u16 = torch.zeros((1, 3, 7, 13), dtype=torch.uint16)
    raw = torch.zeros((1, 7, 13, 3), dtype=torch.uint16)
    cast, cv, sd = T.CastTo("float32"), T.CvToTorch(), T.StridedDownscale(2)
    black = [cast, T.Normalize(4095, 64)]
    lists = {
        "the code pair": (u16, [cast, T.Normalize(65535, 0), sd], "code"),
        "the code pair, downscale first": (u16, [sd, cast, T.Normalize(65535, 0)], "code"),
        "a black level and a clamp": (u16, black + [T.ClampAlongDims(1, PAIRS3), sd], "ingest"),
        "a black level, downscale in the middle": (u16, [cast, sd, T.Normalize(4095, 64)], "ingest"),
        "raw BGR frames": (raw, [cv, sd] + black, "ingest"),
    }
    for what, (probe, ts, route) in lists.items():
        for planar in (False, True):
            staged = T.plan_staging(probe, ts, planar=planar)  # the step is the staging's: what every other caller plans
            assert not staged.step_in_kernel and pipeline_route(probe, staged, False) == "frame_by_frame", what
            plan = T.plan_staging(probe, ts, planar=planar, step_in_kernel=True)  # the generator's plan
            assert plan == dataclasses.replace(staged, step_in_kernel=True), what
            assert plan.route == route and plan.step == 2, what
            assert pipeline_route(probe, plan, False) == "pipelined", what
            assert pipeline_route(probe, plan, True) == "frame_by_frame", what + ", dark field"


def test_pipeline_data_route_needs_the_normalize_in_front_of_the_downscale():
    T = _T()
    from clair_torch_amd.inference.linearization import pipeline_data_route, pipeline_route
    u16 = torch.zeros((1, 3, 7, 13), dtype=torch.uint16)
    cast, sd = T.CastTo("float32"), T.StridedDownscale(2)
    staged = T.plan_staging(u16, [cast, T.Normalize(), sd], on_device=True)
    assert not staged.step_in_kernel and pipeline_data_route(u16, staged, False) == "frame_by_frame"
    behind = T.plan_staging(u16, [cast, T.Normalize(), sd], on_device=True, step_in_kernel=True)
    assert behind == dataclasses.replace(staged, step_in_kernel=True)
    assert behind.route == "ingest_data" and behind.step == 2 and not behind.step_first
    assert pipeline_route(u16, behind, False) == "frame_by_frame"  # the first decision still leaves it to the second
    assert pipeline_data_route(u16, behind, False) == "pipelined"
    assert pipeline_data_route(u16, behind, True) == "frame_by_frame"  # a dark field
    front = T.plan_staging(u16, [cast, sd, T.Normalize()], on_device=True, step_in_kernel=True)
    assert front.route == "ingest_data" and front.step == 2 and front.step_first
    assert pipeline_data_route(u16, front, False) == "frame_by_frame"  # extrema of the selected pixels
    assert pipeline_data_route(u16, front, True) == "frame_by_frame"
    # the flag is about a step: plans without one, and the torch route, never carry it
    for ts in ([cast, T.Normalize(4095, 64)], [cast, T.Normalize(65535, 0)], [cast, T.Normalize()], [sd]):
        assert not T.plan_staging(u16, ts, on_device=True, step_in_kernel=True).step_in_kernel, ts


def test_symbol_is_declared_and_bound(lib):
    from clair_torch_amd import _native as nv
    header = open(os.path.join(ROOT, "include", "clair_hip.h")).read()
    assert re.search(r"\bint\s+ct_linearize_ingest_strided\s*\(", header)
    assert re.search(r"#define\s+CT_ABI_VERSION\s+3\b", header)
    assert "ct_linearize_ingest_strided" in nv.EXPORTS and hasattr(lib, "ct_linearize_ingest_strided")
    assert lib.ct_abi_version() == 3 and nv.ABI_VERSION == 3
    assert len(lib.ct_linearize_ingest_strided.argtypes) == 15
    assert "ct_linearize_ingest_strided.hip" in __import__("clair_torch_amd.build", fromlist=["SOURCES"]).SOURCES


def test_refuses_before_any_launch(lib):
    """Never-dereferenced pointers: every call returns from validation.  The order is ct_linearize_ingest's, with the step and
    the row band in front of the stage list."""
    from clair_torch_amd import _native as nv
    INVALID, UNSUPPORTED, NO_GRAD, TOO_LARGE = (nv.ERR_INVALID_ARGUMENT, nv.ERR_UNSUPPORTED, nv.ERR_NO_GRADIENT_PATH,
                                                nv.ERR_TOO_LARGE)
    fake = ctypes.c_void_p(0x1000)
    affine = (nv.IngestStage * 1)()
    affine[0].kind, affine[0].sub, affine[0].div, affine[0].mul, affine[0].add = nv.INGEST_AFFINE, 64.0, 4031.0, 1.0, 0.0
    data = (nv.IngestStage * 1)()
    data[0].kind, data[0].mul, data[0].add = nv.INGEST_AFFINE_DATA, 1.0, 0.0

    def geom(**kw):
        a = dict(channels=3, h_tile=7, width=13, h_global=7, row_offset=0, image_stride=3 * 7 * 13, layout=nv.LAYOUT_NCHW)
        a.update(kw)
        return nv.Geometry(**a)

    def call(g=None, step=2, stages=affine, n_stages=1, std=None, std_mode=nv.STD_NONE, interp=nv.INTERP_LINEAR, lut=fake,
             n_points=16, frames=fake, lin=fake, std_out=fake, consts=None, dtype=nv.DTYPE_U16, n=2):
        g = g or geom()
        icrf = nv.Icrf(lut_dev=lut, n_points=n_points, interp=interp)
        return lib.ct_linearize_ingest_strided(frames, dtype, n, ctypes.byref(g), step, stages, n_stages, std, std_mode, 0.05,
                                               ctypes.byref(icrf), lin, std_out, consts, None)

    assert call(step=0) == INVALID and call(step=-3) == INVALID
    # a row band behind a downscale: the phase of the band is not carried
    assert call(g=geom(h_tile=4, h_global=7, row_offset=0, image_stride=3 * 4 * 13)) == INVALID
    assert call(g=geom(h_tile=4, h_global=7, row_offset=3, image_stride=3 * 4 * 13)) == INVALID
    assert call(interp=nv.INTERP_LOOKUP, std_mode=nv.STD_CONSTANT) == NO_GRAD
    assert call(interp=nv.INTERP_LOOKUP, std_mode=nv.STD_CONSTANT, frames=None) == NO_GRAD  # pointers come last
    assert call(std_mode=nv.STD_EXPLICIT, std=None) == INVALID
    assert call(stages=data) == INVALID                       # AFFINE_DATA without constants
    assert call(stages=data, consts=ctypes.c_void_p(0x1002)) == INVALID
    assert call(n_stages=5) == INVALID and call(n_stages=-1) == INVALID
    assert call(dtype=7) == INVALID and call(n=-1) == INVALID
    assert call(g=geom(layout=nv.LAYOUT_NHWC, channels=4, image_stride=4 * 7 * 13)) == UNSUPPORTED
    assert call(g=geom(image_stride=10)) == INVALID
    assert call(g=geom(h_tile=0, h_global=0)) == INVALID
    assert call(n_points=20000, interp=nv.INTERP_CATMULL) == TOO_LARGE
    assert call(n=0, frames=None, lin=None) == 0              # nothing to do
    assert call(frames=None) == INVALID and call(lin=None) == INVALID
    assert call(frames=ctypes.c_void_p(0x1001)) == INVALID and call(lin=ctypes.c_void_p(0x1002)) == INVALID
    assert call(std_out=ctypes.c_void_p(0x1002)) == INVALID


def test_ops_front_checks_without_a_device(monkeypatch):
    """The checks of the front that need no device: CPU tensors stand in for device tensors (the device check is taken out)
    and the library is never reached."""
    from clair_torch_amd import ops
    monkeypatch.setattr(ops, "_require_device", lambda t, name: None)
    monkeypatch.setattr(ops.nv, "load", lambda: pytest.fail("the library was reached"))
    frames = torch.zeros((2, 3, 7, 13), dtype=torch.uint16)
    lut = torch.linspace(0, 1, 16).repeat(3, 1)
    stages = [("affine", 64.0, 4031.0, 1.0, 0.0)]
    for step in (0, -1, True, 2.0):
        with pytest.raises(ValueError, match="step"):
            ops.linearize_ingest_frames_strided(frames, step, stages, lut)
    good = (torch.empty((2, 3, 4, 7)), torch.empty((2, 3, 4, 7)))
    for bad in ((torch.empty((2, 3, 7, 13)), good[1]), (good[0], torch.empty((2, 3, 4, 6))), (None, good[1])):
        with pytest.raises(ValueError, match="out"):
            ops.linearize_ingest_frames_strided(frames, 2, stages, lut, out=bad)
    with pytest.raises(ValueError, match="std must be"):  # explicit uncertainties arrive at the downscaled shape
        ops.linearize_ingest_frames_strided(frames, 2, stages, lut, std=torch.zeros((2, 3, 7, 13)))
    with pytest.raises(ValueError, match="consts"):
        ops.linearize_ingest_frames_strided(frames, 2, [("affine_data", 1.0, 0.0)], lut, consts=torch.zeros((3, 4)))
    with pytest.raises(ValueError, match="affine"):
        ops.linearize_ingest_frames_strided(frames, 2, [("affine_data", 1.0, 0.0)], lut)
    with pytest.raises(ValueError, match="layout"):
        ops.linearize_ingest_frames_strided(frames, 2, stages, lut, layout="nhwc")
    assert ops.linearize_ingest_frames_strided(frames[:0], 2, stages, lut)[0].shape == (0, 3, 4, 7)
