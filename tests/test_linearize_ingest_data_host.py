"""The data-dependent Normalize of the streamed linearization without a GPU: ct_ingest_extrema_frames (one set of constants
per frame of a stack) and ct_linearize_ingest_data (the fused chain + ICRF pass that reads them per frame) are declared,
exported and refuse every malformed call before any launch; ``pipeline_data_route`` -- the second, separate decision of
linearize_dataset_generator -- answers what its docstring says while ``pipeline_route`` answers what it always did; the
``ops`` fronts refuse constants of the wrong shape or dtype."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, UNSUPPORTED, TOO_LARGE = 0, -1, -2, -5


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


def test_the_three_symbols_are_declared_and_exported(lib):
    from clair_torch_amd import _native as nv
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "clair_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint64_t\s+ct_ingest_extrema_frames_workspace\s*\(\s*int64_t\s+n_frames\s*\)", header)
    assert re.search(r"\bint\s+ct_ingest_extrema_frames\s*\(", header)
    assert re.search(r"\bint\s+ct_linearize_ingest_data\s*\(", header)
    assert re.search(r"#define\s+CT_ABI_VERSION\s+3\b", header)
    for name in ("ct_ingest_extrema_frames_workspace", "ct_ingest_extrema_frames", "ct_linearize_ingest_data"):
        assert name in nv.EXPORTS and hasattr(lib, name), name
    assert lib.ct_abi_version() == 3 and nv.ABI_VERSION == 3
    for name, n_args in (("ct_ingest_extrema_frames", 15), ("ct_linearize_ingest_data", 14)):
        declared = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", header).group(1)
        assert len(getattr(lib, name).argtypes) == len(declared.split(",")) == n_args, name
    # the existing entry points keep their signatures
    assert len(lib.ct_linearize_ingest.argtypes) == 13 and len(lib.ct_ingest_extrema.argtypes) == 15
    # a workspace holds at least one 16-byte partial per frame, and enough workgroups for one frame to fill the device
    assert lib.ct_ingest_extrema_frames_workspace(1) >= lib.ct_ingest_extrema_workspace()
    for n in (1, 2, 5, 16, 4096, 65535):
        assert lib.ct_ingest_extrema_frames_workspace(n) >= 16 * n and lib.ct_ingest_extrema_frames_workspace(n) % 16 == 0, n
    assert lib.ct_ingest_extrema_frames_workspace(0) == 0 and lib.ct_ingest_extrema_frames_workspace(65536) == 0


def test_ct_ingest_extrema_frames_refuses_before_any_launch(lib):
    from clair_torch_amd import _native as nv
    U8, U16, F32 = nv.DTYPE_U8, nv.DTYPE_U16, nv.DTYPE_F32
    NCHW, NHWC, BGR = nv.LAYOUT_NCHW, nv.LAYOUT_NHWC, nv.LAYOUT_NHWC_BGR
    BOTH = nv.EXTREMA_MIN | nv.EXTREMA_MAX
    fake, ws, consts = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x2000), ctypes.c_void_p(0x3000)
    one = _stages(nv.INGEST_AFFINE)

    def call(src=fake, dtype=U16, layout=NCHW, n=5, c=3, plane=35, prefix=None, n_prefix=0, from_data=BOTH, workspace=ws,
             ws_bytes=None, out=consts):
        if ws_bytes is None:
            ws_bytes = lib.ct_ingest_extrema_frames_workspace(max(n, 1))
        return lib.ct_ingest_extrema_frames(src, dtype, layout, n, c, plane, prefix, n_prefix, from_data, 0.0, 1.0, workspace,
                                            ws_bytes, out, None)

    # NULL or misaligned pointers
    assert call(src=None) == INVALID and call(out=None) == INVALID and call(workspace=None) == INVALID
    assert call(src=ctypes.c_void_p(0x1001)) == INVALID                          # uint16 at an odd address
    assert call(src=ctypes.c_void_p(0x1002), dtype=F32) == INVALID
    assert call(out=ctypes.c_void_p(0x3002)) == INVALID
    assert call(workspace=ctypes.c_void_p(0x2008)) == INVALID                    # 16-byte alignment
    # nothing depends on the data; bits that are no bound
    assert call(from_data=0) == INVALID and call(from_data=4) == INVALID and call(from_data=-1) == INVALID
    # an empty stack (torch raises on the extrema of an empty tensor)
    assert call(n=0) == INVALID and call(plane=0) == INVALID and call(n=-1) == INVALID
    # a workspace one byte short, for several frame counts
    for n in (1, 5, 16, 300):
        assert call(n=n, ws_bytes=lib.ct_ingest_extrema_frames_workspace(n) - 1) == INVALID, n
    # the prefix: constant stages only, at most CT_EXTREMA_MAX_PREFIX
    assert call(prefix=_stages(nv.INGEST_AFFINE_DATA), n_prefix=1) == INVALID
    assert call(prefix=_stages(nv.INGEST_AFFINE, nv.INGEST_AFFINE_DATA), n_prefix=2) == INVALID
    assert call(prefix=_stages(*[nv.INGEST_AFFINE] * 4), n_prefix=4) == INVALID
    assert call(prefix=None, n_prefix=1) == INVALID and call(prefix=one, n_prefix=-1) == INVALID
    assert call(prefix=_stages(7), n_prefix=1) == INVALID
    # dtype, layout, channels
    assert call(dtype=3) == INVALID and call(layout=3) == INVALID and call(c=0) == INVALID
    # an interleaved layout with C != 3; per-channel pairs for more than 4 channels
    assert call(layout=NHWC, c=4, dtype=U8) == UNSUPPORTED and call(layout=BGR, c=1, dtype=U8) == UNSUPPORTED
    by_channel = _stages(nv.INGEST_CLAMP, lo=(0.0, 0.1, 0.0, 0.0))
    assert call(c=5, dtype=F32, prefix=by_channel, n_prefix=1) == UNSUPPORTED
    # more frames than the grid indexes, more elements than 64-bit byte offsets hold
    assert call(n=65536, ws_bytes=1 << 30) == TOO_LARGE
    assert call(n=4, plane=1 << 60, ws_bytes=1 << 30) == TOO_LARGE
    # ... and the single-stack entry point answers the same for what they share
    def stack(**kw):
        a = dict(src=fake, dtype=U16, layout=NCHW, n=5, c=3, plane=35, prefix=None, n_prefix=0, from_data=BOTH)
        a.update(kw)
        return lib.ct_ingest_extrema(a["src"], a["dtype"], a["layout"], a["n"], a["c"], a["plane"], a["prefix"], a["n_prefix"],
                                     a["from_data"], 0.0, 1.0, ws, lib.ct_ingest_extrema_workspace(), consts, None)
    for kw in (dict(src=None), dict(from_data=0), dict(n=0), dict(plane=0), dict(layout=NHWC, c=4, dtype=U8), dict(dtype=3),
               dict(prefix=_stages(nv.INGEST_AFFINE_DATA), n_prefix=1)):
        assert call(**kw) == stack(**kw), kw


def test_ct_linearize_ingest_data_refuses_before_any_launch(lib):
    from clair_torch_amd import _native as nv
    U8, U16, F32 = nv.DTYPE_U8, nv.DTYPE_U16, nv.DTYPE_F32
    NHWC, BGR = nv.LAYOUT_NHWC, nv.LAYOUT_NHWC_BGR
    fake, consts = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x3000)
    icrf = nv.Icrf(lut_dev=0x2000, n_points=256, interp=nv.INTERP_LINEAR)
    data = _stages(nv.INGEST_AFFINE_DATA)

    def call(frames=fake, dtype=U16, n=1, geom=None, stages=data, n_stages=1, std=None, std_mode=nv.STD_NONE, model=icrf,
             lin=fake, std_out=fake, k=consts):
        geom = _geom() if geom is None else geom
        return lib.ct_linearize_ingest_data(frames, dtype, n, ctypes.byref(geom), stages, n_stages, std, std_mode, 0.05,
                                            ctypes.byref(model), lin, std_out, k, None)

    # nothing to do: CT_OK without a launch -- one data stage, a data stage among constant ones, none at all
    assert call(n=0) == OK
    assert call(n=0, stages=_stages(nv.INGEST_AFFINE, nv.INGEST_AFFINE_DATA, nv.INGEST_CLAMP), n_stages=3) == OK
    assert call(n=0, stages=_stages(nv.INGEST_AFFINE), n_stages=1) == OK
    assert call(n=0, geom=_geom(layout=BGR), dtype=U8) == OK
    # two AFFINE_DATA stages; such a stage without constants; misaligned constants
    assert call(n=0, stages=_stages(nv.INGEST_AFFINE_DATA, nv.INGEST_AFFINE_DATA), n_stages=2) == INVALID
    assert call(stages=_stages(nv.INGEST_AFFINE_DATA, nv.INGEST_CLAMP, nv.INGEST_AFFINE_DATA), n_stages=3) == INVALID
    assert call(k=None) == INVALID and call(n=0, k=None) == INVALID
    assert call(k=ctypes.c_void_p(0x3002)) == INVALID and call(n=0, k=ctypes.c_void_p(0x3001)) == INVALID
    # NULL or misaligned pointers with n_frames > 0
    assert call(frames=None) == INVALID and call(lin=None) == INVALID
    assert call(frames=ctypes.c_void_p(0x1001)) == INVALID
    assert call(lin=ctypes.c_void_p(0x1002)) == INVALID and call(std_out=ctypes.c_void_p(0x1002)) == INVALID
    assert call(std_mode=nv.STD_EXPLICIT, std=None) == INVALID
    # the stage list, the geometry, the model: as ct_linearize_ingest
    assert call(stages=_stages(*[nv.INGEST_AFFINE] * 5), n_stages=5) == INVALID and call(stages=None, n_stages=1) == INVALID
    assert call(dtype=3) == INVALID and call(geom=_geom(layout=3)) == INVALID and call(geom=_geom(h=0)) == INVALID
    assert call(geom=_geom(h=4, h_global=6, row_offset=3)) == INVALID and call(n=-1) == INVALID
    assert call(geom=_geom(c=4, layout=NHWC), dtype=U8) == UNSUPPORTED
    assert call(geom=_geom(c=1, layout=BGR), dtype=U8) == UNSUPPORTED
    assert call(model=nv.Icrf(lut_dev=0x2000, n_points=1, interp=nv.INTERP_LINEAR)) == INVALID
    lookup = nv.Icrf(lut_dev=0x2000, n_points=256, interp=nv.INTERP_LOOKUP)
    assert call(model=lookup, std_mode=nv.STD_MULTIPLIER) == nv.ERR_NO_GRADIENT_PATH
    assert call(geom=_geom(h=1 << 15, w=1 << 15)) == TOO_LARGE


def test_ct_linearize_ingest_still_refuses_affine_data(lib):
    from clair_torch_amd import _native as nv
    fake = ctypes.c_void_p(0x1000)
    icrf = nv.Icrf(lut_dev=0x2000, n_points=256, interp=nv.INTERP_LINEAR)
    geom = _geom()
    for n in (0, 1):
        for stages, k in ((_stages(nv.INGEST_AFFINE_DATA), 1), (_stages(nv.INGEST_AFFINE, nv.INGEST_AFFINE_DATA), 2)):
            assert lib.ct_linearize_ingest(fake, nv.DTYPE_U16, n, ctypes.byref(geom), stages, k, None, nv.STD_NONE, 0.0,
                                           ctypes.byref(icrf), fake, fake, None) == INVALID


def _T():
    from clair_torch_amd.common import transforms
    return transforms


def test_pipeline_data_route():
    T = _T()
    from clair_torch_amd.inference.linearization import pipeline_data_route, pipeline_route
    u8 = torch.zeros((1, 3, 4, 6), dtype=torch.uint8)
    u16 = torch.zeros((1, 3, 4, 6), dtype=torch.uint16)
    raw = torch.zeros((1, 4, 6, 3), dtype=torch.uint16)
    f32 = torch.zeros((1, 3, 4, 6), dtype=torch.float32)
    stages = (("affine_data", 1.0, 0.0),)

    def plan(**kw):
        a = dict(source_layout="nchw", stages=stages, prefix=())
        a.update(kw)
        return T.StagingPlan("ingest_data", **a)

    for what, probe, p in (("uint16", u16, plan()), ("uint8", u8, plan()), ("float32", f32, plan()),
                           ("raw BGR frames", raw, plan(source_layout="nhwc_bgr")),
                           ("a fixed minimum", u16, plan(min_val=64.0)), ("a fixed maximum", u16, plan(max_val=4095.0)),
                           ("a prefix and a clamp", u16, plan(stages=(("affine", 64.0, 4031.0, 1.0, 0.0),) + stages + (("clamp", [(0.0, 1.0)]),),
                                                                prefix=(("affine", 64.0, 4031.0, 1.0, 0.0),)))):
        assert pipeline_data_route(probe, p, False) == "pipelined", what
        assert pipeline_data_route(probe, p, True) == "frame_by_frame", what + ", dark field"
        assert pipeline_route(probe, p, False) == "frame_by_frame", what + ": pipeline_route answers what it always did"
    assert pipeline_data_route(u16, plan(step=2), False) == "frame_by_frame"
    assert pipeline_data_route(u16, plan(step=2, step_first=True), False) == "frame_by_frame"
    assert pipeline_data_route(u16[0], plan(), False) == "frame_by_frame"                       # a 3-D probe
    assert pipeline_data_route(torch.zeros((1, 3, 4, 6), dtype=torch.float64), plan(), False) == "frame_by_frame"
    # plans of the other routes are not this function's: "torch" (what a CPU probe with Normalize() plans as), "ingest", "code"
    cast = T.CastTo("float32")
    for ts in ([cast, T.Normalize()], [cast, T.Normalize(), T.Normalize()], [], [cast, T.Normalize(4095, 64)],
               [cast, T.Normalize(65535, 0)]):
        for probe in (u16, f32):
            p = T.plan_staging(probe, ts)
            assert p.route != "ingest_data"
            assert pipeline_data_route(probe, p, False) == "frame_by_frame", (ts, p.route)
    assert T.plan_staging(u16, [cast, T.Normalize()]).route == "torch"
    # the generator plans its host probe as the batch on the device is planned: route "ingest_data"
    for probe, ts, layout in ((u16, [cast, T.Normalize()], "nchw"), (f32, [T.Normalize(None, 0.25)], "nchw"),
                              (raw, [T.CvToTorch(), cast, T.Normalize(None, 64), T.ClampAlongDims(1, [(0.0, 1.0)] * 3)], "nhwc_bgr")):
        for planar in (False, True):
            p = T.plan_staging(probe, ts, planar=planar, on_device=True)
            assert p.route == "ingest_data" and p.source_layout == layout and p.step == 1
            assert pipeline_data_route(probe, p, False) == "pipelined" and pipeline_route(probe, p, False) == "frame_by_frame"
    staged = T.plan_staging(u16, [cast, T.Normalize(), T.StridedDownscale(2)], on_device=True)
    assert staged.route == "ingest_data" and pipeline_data_route(u16, staged, False) == "frame_by_frame"
    assert T.plan_staging(u16, [cast, T.Normalize(), T.Normalize()], on_device=True).route == "torch"
    assert T.plan_staging(u16, [cast, T.Normalize(65535, 0)], on_device=True).route == "code"      # the other routes are
    assert T.plan_staging(u16, [cast, T.Normalize(4095, 64)], on_device=True).route == "ingest"    # what they were
    assert pipeline_route(u16, T.plan_staging(u16, [cast, T.Normalize()]), False) == "frame_by_frame"


def test_ops_fronts_refuse_malformed_constants(monkeypatch):
    """The checks of the fronts that need no device: CPU tensors stand in for device tensors (the device check is taken
    out), every call is refused before the library is asked for anything."""
    from clair_torch_amd import ops
    monkeypatch.setattr(ops, "_require_device", lambda t, name: None)
    frames = torch.zeros((5, 3, 4, 6), dtype=torch.uint16)
    lut = torch.stack([torch.linspace(0, 1, 16)] * 3)
    stages = [("affine_data", 1.0, 0.0)]
    with pytest.raises(ValueError):
        ops.linearize_ingest_frames(frames, stages, lut, "linear")                                  # no consts
    with pytest.raises(ValueError):
        ops.linearize_ingest_frames(frames, [("affine", 0.0, 1.0, 1.0, 0.0)] + stages, lut, "linear", consts=None)
    for bad in (torch.zeros((4,)), torch.zeros((4, 4)), torch.zeros((5, 2)), torch.zeros((5, 4, 1)), torch.zeros((20,)),
                torch.zeros((4, 5)).t()):
        with pytest.raises(ValueError):
            ops.linearize_ingest_frames(frames, stages, lut, "linear", consts=bad)
    for bad in (torch.zeros((5, 4), dtype=torch.float64), torch.zeros((5, 4), dtype=torch.int32)):
        with pytest.raises((ValueError, TypeError)):
            ops.linearize_ingest_frames(frames, stages, lut, "linear", consts=bad)
    with pytest.raises(ValueError):                                                                   # two data stages
        ops.linearize_ingest_frames(frames, stages * 2, lut, "linear", consts=torch.zeros((5, 4)))
    # ingest_extrema_frames: both bounds given, a data stage in the prefix, too long a prefix, an empty stack, a bad out
    with pytest.raises(ValueError):
        ops.ingest_extrema_frames(frames, (), "nchw", 0.0, 1.0)
    with pytest.raises(ValueError):
        ops.ingest_extrema_frames(frames, stages)
    with pytest.raises(ValueError):
        ops.ingest_extrema_frames(frames, [("affine", 0.0, 1.0, 1.0, 0.0)] * 4)
    with pytest.raises(RuntimeError):
        ops.ingest_extrema_frames(frames[:0])
    with pytest.raises(ValueError):
        ops.ingest_extrema_frames(frames, layout="nhwc")                                             # (F,H,W,3) expected


def test_front_end_without_a_device():
    from clair_torch_amd import ops
    lut = torch.stack([torch.linspace(0, 1, 16)] * 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.ingest_extrema_frames(torch.zeros((2, 3, 4, 4)))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.linearize_ingest_frames(torch.zeros((2, 3, 4, 4)), [("affine_data", 1.0, 0.0)], lut, consts=torch.zeros((2, 4)))


def test_fake_kernels_of_the_custom_ops():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from clair_torch_amd import torch_ops
    prefix = torch_ops.flatten_ingest_stages([("affine", 64, 4031, 1.0, 0.0)], 3)
    stages = torch_ops.flatten_ingest_stages([("affine", 64, 4031, 1.0, 0.0), ("affine_data", 2.0, -1.0)], 3)
    with FakeTensorMode():
        frames = torch.empty((5, 6, 7, 3), dtype=torch.uint16)
        consts = torch.ops.clair_hip.ingest_extrema_frames(frames, prefix, "nhwc_bgr", None, 4095.0)
        assert tuple(consts.shape) == (5, 4) and consts.dtype == torch.float32
        lin, sd = torch.ops.clair_hip.linearize_ingest_data(frames, stages, consts, torch.empty((3, 64)), "linear", None,
                                                            "multiplier", 0.05, "nhwc_bgr")
        assert tuple(lin.shape) == tuple(sd.shape) == (5, 3, 6, 7) and lin.dtype == sd.dtype == torch.float32
    # the existing schema is untouched: linearize_ingest takes no constants
    assert "consts" not in str(torch.ops.clair_hip.linearize_ingest.default._schema)
