"""The fused chain + merge without a GPU: ct_hdr_merge_ingest_batch is declared, exported and validates every argument
before any launch; the opt-in staging hands the chain over unexecuted for "ingest" / "ingest_data" plans and leaves every
other result alone; the custom op has a fake kernel."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, UNSUPPORTED, NO_GRADIENT, TOO_LARGE = 0, -1, -2, -4, -5


@pytest.fixture(scope="module")
def lib():
    from clair_torch_amd import build, _native
    build.build()
    return _native.load()


def _stages(*kinds):
    from clair_torch_amd import _native as nv
    arr = (nv.IngestStage * max(len(kinds), 1))()
    for k, kind in enumerate(kinds):
        arr[k].kind, arr[k].sub, arr[k].div, arr[k].mul, arr[k].add = kind, 64.0, 959.0, 1.0, 0.0
        for c in range(4):
            arr[k].lo[c], arr[k].hi[c] = 0.0, 1.0
    return arr


def _geom(c=3, h=4, w=4, layout=0, h_global=None, row_offset=0):
    from clair_torch_amd import _native as nv
    return nv.Geometry(channels=c, h_tile=h, width=w, h_global=h if h_global is None else h_global, row_offset=row_offset,
                       image_stride=c * h * w, layout=layout)


def test_ct_hdr_merge_ingest_batch_is_declared_and_exported(lib):
    from clair_torch_amd import _native as nv
    from clair_torch_amd import build
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "clair_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+ct_hdr_merge_ingest_batch\s*\(", header)
    assert re.search(r"#define\s+CT_ABI_VERSION\s+3\b", header)
    assert "ct_hdr_merge_ingest_batch" in nv.EXPORTS and hasattr(lib, "ct_hdr_merge_ingest_batch")
    assert "ct_merge_ingest.hip" in build.SOURCES and "ct_merge_ingest.hpp" in build.HEADERS
    assert lib.ct_abi_version() == 3 and nv.ABI_VERSION == 3
    assert len(lib.ct_hdr_merge_ingest_batch.argtypes) == 20


def test_ct_hdr_merge_ingest_batch_validates_before_any_launch(lib):
    from clair_torch_amd import _native as nv
    U8, U16, F32 = nv.DTYPE_U8, nv.DTYPE_U16, nv.DTYPE_F32
    NHWC, BGR = nv.LAYOUT_NHWC, nv.LAYOUT_NHWC_BGR
    FIRST, FINAL = nv.MERGE_FIRST_BATCH, nv.MERGE_FINALIZE
    fake = ctypes.c_void_p(0x1000)  # never dereferenced: validation fails first, or there is nothing to launch
    linear = nv.Icrf(lut_dev=0x2000, n_points=256, interp=nv.INTERP_LINEAR)
    one = _stages(nv.INGEST_AFFINE)

    def call(frames=None, dtype=U16, batch=2, geom=None, stages=one, n_stages=1, consts=None, std=None, std_mode=nv.STD_NONE,
             expo=None, model=linear, weight=nv.WEIGHT_GAUSS, state=(None, None, None), mean_out=fake, std_out=fake,
             flags=FIRST | FINAL):
        geom = _geom() if geom is None else geom
        return lib.ct_hdr_merge_ingest_batch(frames, dtype, batch, ctypes.byref(geom), stages, n_stages, consts, std, std_mode, 0.05,
                                             expo, ctypes.byref(model), weight, state[0], state[1], state[2], mean_out, std_out,
                                             flags, None)

    # the frames and the exposure times are NULL in every call below: whatever is documented comes before they matter
    # nothing to do: CT_OK without a launch
    assert call(batch=0) == OK
    assert call(batch=0, stages=None, n_stages=0) == OK
    assert call(geom=_geom(h=0)) == OK and call(geom=_geom(w=0), dtype=U8) == OK
    assert call(batch=0, geom=_geom(layout=BGR), std_mode=nv.STD_MULTIPLIER) == OK
    assert call(batch=0, stages=_stages(nv.INGEST_AFFINE_DATA), consts=fake) == OK
    # with something to do, the NULL frames are what is wrong
    assert call() == INVALID and call(frames=fake) == INVALID          # (then the NULL exposure times)
    assert call(frames=ctypes.c_void_p(0x1001), expo=fake) == INVALID   # uint16 at an odd address
    # dtype, layout, geometry
    assert call(dtype=3) == INVALID and call(dtype=-1) == INVALID
    assert call(dtype=F32) == UNSUPPORTED
    assert call(geom=_geom(layout=3)) == INVALID and call(geom=_geom(layout=-1)) == INVALID
    assert call(geom=_geom(c=0)) == INVALID and call(batch=-1) == INVALID
    assert call(geom=_geom(h=4, h_global=3)) == INVALID and call(geom=_geom(h=4, h_global=6, row_offset=3)) == INVALID
    assert call(geom=_geom(h=1 << 15, w=1 << 15)) == TOO_LARGE
    # the stage list
    assert call(stages=_stages(*[nv.INGEST_AFFINE] * 5), n_stages=5) == INVALID
    assert call(n_stages=-1) == INVALID and call(stages=None, n_stages=1) == INVALID and call(stages=_stages(7)) == INVALID
    assert call(stages=_stages(nv.INGEST_AFFINE_DATA)) == INVALID                                    # without consts_dev
    assert call(stages=_stages(nv.INGEST_AFFINE_DATA, nv.INGEST_AFFINE_DATA), n_stages=2, consts=fake) == INVALID
    assert call(batch=0, stages=_stages(nv.INGEST_AFFINE, nv.INGEST_AFFINE_DATA), n_stages=2, consts=fake) == OK
    assert call(consts=ctypes.c_void_p(0x1002)) == INVALID
    # not built: interleaved with C != 3
    assert call(geom=_geom(c=4, layout=NHWC)) == UNSUPPORTED and call(geom=_geom(c=1, layout=BGR), dtype=U8) == UNSUPPORTED
    # the flags this entry point does not take
    for flag in (nv.MERGE_F64_MOMENTS, nv.MERGE_REFERENCE_ORDER, nv.MERGE_OUT_AS_INPUT):
        assert call(flags=FIRST | FINAL | flag) == UNSUPPORTED, flag
    # ... and the modes ct_hdr_merge_batch sends to the reference-order kernel, unless the closed form is asked for
    for interp in (nv.INTERP_LOOKUP, nv.INTERP_CATMULL):
        model = nv.Icrf(lut_dev=0x2000, n_points=256, interp=interp)
        for std_mode in (nv.STD_CONSTANT, nv.STD_MULTIPLIER):
            assert call(model=model, std_mode=std_mode) == UNSUPPORTED
            assert call(batch=0, model=model, std_mode=std_mode, flags=FIRST | FINAL | nv.MERGE_CLOSED_FORM) == OK
        assert call(batch=0, model=model) == OK   # without uncertainties they are closed-form anyway
    # the model, the modes, the state: as ct_hdr_merge_batch
    lookup = nv.Icrf(lut_dev=0x2000, n_points=256, interp=nv.INTERP_LOOKUP)
    assert call(model=lookup, std_mode=nv.STD_MULTIPLIER, weight=nv.WEIGHT_NONE) == NO_GRADIENT
    assert call(model=lookup, std_mode=nv.STD_MULTIPLIER, weight=nv.WEIGHT_NONE, flags=FIRST | FINAL | nv.MERGE_CLOSED_FORM) == NO_GRADIENT
    assert call(model=nv.Icrf(lut_dev=0x2000, n_points=256, interp=7)) == INVALID
    assert call(model=nv.Icrf(lut_dev=None, n_points=256, interp=nv.INTERP_LINEAR)) == INVALID
    assert call(model=nv.Icrf(lut_dev=0x2000, n_points=1, interp=nv.INTERP_LINEAR)) == INVALID
    assert call(model=nv.Icrf(lut_dev=0x2000, n_points=1 << 20, interp=nv.INTERP_CATMULL)) == TOO_LARGE   # the LUT exceeds the LDS
    assert call(std_mode=4) == INVALID and call(std_mode=-1) == INVALID and call(weight=2) == INVALID
    assert call(flags=FIRST) == INVALID and call(flags=FINAL) == INVALID                      # no state: one batch only
    assert call(batch=0, flags=0, state=(fake, fake, None)) == OK
    assert call(batch=0, flags=0, state=(fake, fake, None), std_mode=nv.STD_CONSTANT) == INVALID   # no variance state
    assert call(mean_out=None) == INVALID and call(std_out=None, std_mode=nv.STD_CONSTANT) == INVALID
    assert call(frames=fake, expo=fake, std_mode=nv.STD_EXPLICIT, std=None) == INVALID
    short = _geom()
    short.image_stride = 47
    assert call(geom=short) == INVALID


def _T():
    from clair_torch_amd.common import transforms
    return transforms


class _Recorder:
    """Stands in for clair_torch_amd.ops inside the staging: records the calls, returns tagged tensors."""

    def __init__(self):
        self.calls = []

    def strided_downscale(self, images, step, layout="nchw"):
        self.calls.append(("downscale", step, layout))
        return images if step == 1 else (images[:, :, ::step, ::step] if layout == "nchw" else images[:, ::step, ::step]).contiguous()

    def ingest_transform(self, images, stages, layout="nchw", consts=None):
        self.calls.append(("ingest", tuple(stages), layout, consts is not None))
        return torch.zeros((images.shape[0], 3, 1, 1))

    def ingest_extrema(self, images, prefix, layout, min_val, max_val):
        self.calls.append(("extrema", tuple(images.shape), tuple(prefix), layout, min_val, max_val))
        return torch.tensor([0.0, 1.0, 0.0, 1.0])

    def check_ingest_consts(self, consts):
        self.calls.append(("check",))


def test_deferred_staging(monkeypatch):
    T = _T()
    from clair_torch_amd.inference import _staging
    cast, cv = T.CastTo("float32"), T.CvToTorch()
    u16 = torch.arange(2 * 3 * 4 * 6, dtype=torch.int32).reshape(2, 3, 4, 6).to(torch.uint16)
    raw = torch.zeros((2, 4, 6, 3), dtype=torch.uint16)
    cpu = torch.device("cpu")

    def stage(batch, ts, **kw):
        rec = _Recorder()
        monkeypatch.setattr(_staging, "ops", rec)
        return _staging.stage_images(batch, cpu, ts, **kw), rec.calls

    # "ingest": deferred -- the raw frames, the plan's stages and source layout, no ct_ingest_transform
    black = [cast, T.Normalize(1023, 64)]
    for batch, ts, layout in ((u16, black, "nchw"), (raw, [cv] + black, "nhwc_bgr")):
        plan = T.plan_staging(batch, ts)
        assert plan.route == "ingest" and plan.source_layout == layout
        (d, max_code, lay), calls = stage(batch, ts, defer_ingest=True)
        assert isinstance(d, _staging.DeferredIngest) and max_code is None and lay == "nchw"
        assert d.frames.dtype == torch.uint16 and torch.equal(d.frames.view(torch.int16), batch.view(torch.int16))
        assert d.stages == plan.stages and d.layout == layout and d.consts is None
        assert [c[0] for c in calls] == ["downscale"]
        (out, max_code, lay), calls = stage(batch, ts)   # the default: executed, as ever
        assert isinstance(out, torch.Tensor) and out.dtype == torch.float32 and [c[0] for c in calls] == ["downscale", "ingest"]
    # ... behind the StridedDownscale compaction where the plan has one
    (d, _, _), calls = stage(u16, [T.StridedDownscale(2)] + black + [T.ClampAlongDims(1, [(0.0, 1.0)] * 3)], defer_ingest=True)
    assert isinstance(d, _staging.DeferredIngest) and tuple(d.frames.shape) == (2, 3, 2, 3) and len(d.stages) == 2
    assert calls == [("downscale", 2, "nchw")]
    # "ingest_data" (the plan needs a CUDA batch to be chosen: hand it over directly): the extrema, their check, no transform
    data_plan = T.StagingPlan("ingest_data", source_layout="nchw", step=2, step_first=False, stages=(("affine_data", 1.0, 0.0),),
                              prefix=(), min_val=None, max_val=None)
    monkeypatch.setattr(_staging, "plan_staging", lambda images, ts, planar=False: data_plan)
    (d, max_code, lay), calls = stage(u16, [cast, T.Normalize(), T.StridedDownscale(2)], defer_ingest=True)
    assert isinstance(d, _staging.DeferredIngest) and d.consts is not None and d.stages == data_plan.stages and d.layout == "nchw"
    assert tuple(d.frames.shape) == (2, 3, 2, 3) and max_code is None and lay == "nchw"
    assert [c[0] for c in calls] == ["extrema", "downscale", "check"] and calls[0][1] == (2, 3, 4, 6)   # extrema of the full stack
    (out, _, _), calls = stage(u16, [cast, T.Normalize(), T.StridedDownscale(2)])
    assert isinstance(out, torch.Tensor) and [c[0] for c in calls] == ["extrema", "downscale", "ingest", "check"]
    monkeypatch.undo()
    # "code" and "torch" plans: the opt-in changes nothing
    pair = [cast, T.Normalize(65535, 0)]
    f32 = torch.rand((2, 3, 4, 6))

    class Unknown(T.BaseTransform):
        def __call__(self, x):
            return x * 2

    for batch, ts, route in ((u16, pair, "code"), (raw, [cv] + pair, "code"), (f32, [], "torch"), (f32, [Unknown()], "torch"),
                             (u16, black + [Unknown()], "torch")):
        assert T.plan_staging(batch, ts).route == route
        plain = _staging.stage_images(batch, cpu, ts)
        opted = _staging.stage_images(batch, cpu, ts, defer_ingest=True)
        assert isinstance(opted[0], torch.Tensor) and opted[1:] == plain[1:] and opted[0].dtype == plain[0].dtype
        same = opted[0].view(torch.int16) == plain[0].view(torch.int16) if plain[0].dtype == torch.uint16 else opted[0] == plain[0]
        assert bool(same.all())


def test_plan_staging_is_as_before():
    T = _T()
    cast, cv = T.CastTo("float32"), T.CvToTorch()
    u16 = torch.zeros((1, 3, 4, 6), dtype=torch.uint16)
    raw = torch.zeros((1, 4, 6, 3), dtype=torch.uint16)
    assert T.plan_staging(u16, [cast, T.Normalize(65535, 0)]) == T.StagingPlan("code", "nchw", 1, max_code=65535.0, source_layout="nchw")
    assert T.plan_staging(raw, [cv, cast, T.Normalize(4095, 0)]) == T.StagingPlan("code", "nhwc_bgr", 1, max_code=4095.0,
                                                                                  source_layout="nhwc_bgr")
    assert T.plan_staging(u16, [cast, T.Normalize(1023, 64)]) == T.StagingPlan("ingest", source_layout="nchw", step=1,
                                                                              stages=(("affine", 64, 959, 1.0, 0.0),))
    assert T.plan_staging(raw, [cv, cast, T.Normalize(1023, 64)], planar=True).source_layout == "nhwc_bgr"
    assert T.plan_staging(u16, [cast, T.Normalize()]) == T.StagingPlan("torch")   # a CPU batch: the classes run
    assert T.plan_staging(u16, []) == T.StagingPlan("torch", no_transforms=True)


def test_front_end_without_a_device():
    from clair_torch_amd import ops
    lut = torch.stack([torch.linspace(0, 1, 16)] * 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.hdr_merge_ingest_batch(torch.zeros((2, 3, 4, 4), dtype=torch.uint8), [("affine", 0.0, 1.0, 1.0, 0.0)],
                                   torch.tensor([1.0, 2.0]), lut=lut)


def test_fake_kernel_of_the_custom_op():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from clair_torch_amd import torch_ops
    stages = torch_ops.flatten_ingest_stages([("affine", 64, 959, 1.0, 0.0), ("clamp", [(0.0, 1.0)]), ("affine_data", 2.0, -1.0)], 3)
    assert len(stages) == 39 and stages[26:31] == [2.0, 0.0, 0.0, 2.0, -1.0]
    frames = torch.zeros((1, 2, 2, 3), dtype=torch.uint8)
    assert torch_ops._listed_ingest_stages(frames, stages, "nhwc_bgr")[2] == ("affine_data", 2.0, -1.0)
    with FakeTensorMode():
        frames, expo, lut = torch.empty((4, 5, 7, 3), dtype=torch.uint16), torch.empty((4,), dtype=torch.float64), torch.empty((3, 64))
        mean, sd = torch.ops.clair_hip.hdr_merge_ingest_batch(frames, stages, expo, lut, "linear", True, None, "multiplier", 0.05,
                                                              "nhwc_bgr", 0, 0, False, torch.empty((4,)))
        assert tuple(mean.shape) == tuple(sd.shape) == (3, 5, 7) and mean.dtype == torch.float64 and sd.dtype == torch.float32
        mean, sd = torch.ops.clair_hip.hdr_merge_ingest_batch(torch.empty((4, 1, 5, 7), dtype=torch.uint8), stages[:13], expo, None, "linear",
                                                              False, None, "none", 0.0)
        assert tuple(mean.shape) == (1, 5, 7) and sd.numel() == 0
        sigma = torch.empty((4, 3, 5, 7))
        mean, sd = torch.ops.clair_hip.hdr_merge_ingest_batch(frames, stages[:13], expo, lut, "linear", True, sigma, "none", 0.0, "nhwc")
        assert tuple(sd.shape) == (3, 5, 7)
