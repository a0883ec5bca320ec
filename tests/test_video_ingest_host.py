"""The fused chain + video statistics without a GPU: ct_video_stats_ingest_batch is declared, exported and validates every
argument before any launch; compute_video_mean_and_std hands a black-level chain on raw codes to the fused front and
everything else to what it called before; the front end has no CPU path."""
import ctypes
import os
import re

import pytest
import torch
from torch.utils.data import DataLoader

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, UNSUPPORTED, TOO_LARGE = 0, -1, -2, -5


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


def test_ct_video_stats_ingest_batch_is_declared_and_exported(lib):
    from clair_torch_amd import _native as nv
    from clair_torch_amd import build
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "clair_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+ct_video_stats_ingest_batch\s*\(", header)
    assert re.search(r"#define\s+CT_ABI_VERSION\s+3\b", header)
    assert "ct_video_stats_ingest_batch" in nv.EXPORTS and hasattr(lib, "ct_video_stats_ingest_batch")
    assert "ct_stats_ingest.hip" in build.SOURCES and "ct_stats_merge.hpp" in build.HEADERS
    assert lib.ct_abi_version() == 3 and nv.ABI_VERSION == 3
    assert len(lib.ct_video_stats_ingest_batch.argtypes) == 12


def test_ct_video_stats_ingest_batch_validates_before_any_launch(lib):
    from clair_torch_amd import _native as nv
    U8, U16, F32 = nv.DTYPE_U8, nv.DTYPE_U16, nv.DTYPE_F32
    NHWC, BGR = nv.LAYOUT_NHWC, nv.LAYOUT_NHWC_BGR
    fake = ctypes.c_void_p(0x1000)  # never dereferenced: validation fails first, or there is nothing to launch
    linear = nv.Icrf(lut_dev=0x2000, n_points=256, interp=nv.INTERP_LINEAR)
    none = nv.Icrf(lut_dev=None, n_points=0, interp=nv.INTERP_NONE)
    one = _stages(nv.INGEST_AFFINE)

    def call(frames=None, dtype=U16, batch=2, geom=None, stages=one, n_stages=1, consts=None, model=linear, before=0.0,
             mean=fake, m2=fake):
        geom = _geom() if geom is None else geom
        return lib.ct_video_stats_ingest_batch(frames, dtype, batch, ctypes.byref(geom), stages, n_stages, consts,
                                               ctypes.byref(model), before, mean, m2, None)

    # the frames are NULL in every call that is not about them: whatever is documented comes before they matter
    # nothing to do: CT_OK without a launch
    assert call(batch=0) == OK and call(batch=0, model=none) == OK
    assert call(batch=0, stages=None, n_stages=0) == OK
    assert call(geom=_geom(h=0)) == OK and call(geom=_geom(w=0), dtype=U8) == OK
    assert call(batch=0, geom=_geom(layout=BGR)) == OK and call(batch=0, geom=_geom(layout=NHWC), dtype=U8) == OK
    assert call(batch=0, stages=_stages(nv.INGEST_AFFINE_DATA), consts=fake) == OK
    assert call(batch=0, mean=None, m2=None) == OK
    # with something to do: NULL or misaligned frames, a NULL state
    assert call() == INVALID
    assert call(frames=ctypes.c_void_p(0x1001)) == INVALID                # uint16 at an odd address
    assert call(frames=fake, mean=None) == INVALID and call(frames=fake, m2=None) == INVALID
    assert call(frames=fake, mean=ctypes.c_void_p(0x1002)) == INVALID and call(frames=fake, m2=ctypes.c_void_p(0x1001)) == INVALID
    # dtype, layout, geometry
    assert call(dtype=3) == INVALID and call(dtype=-1) == INVALID
    assert call(dtype=F32) == UNSUPPORTED and call(dtype=F32, batch=0) == UNSUPPORTED
    assert call(geom=_geom(layout=3)) == INVALID and call(geom=_geom(layout=-1)) == INVALID
    assert call(geom=_geom(c=0)) == INVALID and call(batch=-1) == INVALID
    assert call(geom=_geom(h=-1)) == INVALID and call(geom=_geom(w=-1)) == INVALID
    assert call(geom=_geom(h=4, h_global=3)) == INVALID and call(geom=_geom(h=4, h_global=6, row_offset=3)) == INVALID
    assert call(geom=_geom(h=4, h_global=6, row_offset=-1)) == INVALID
    assert call(geom=_geom(h=1 << 15, w=1 << 15)) == TOO_LARGE
    short = _geom()
    short.image_stride = 47
    assert call(geom=short) == INVALID
    # the stage list
    assert call(stages=_stages(*[nv.INGEST_AFFINE] * 5), n_stages=5) == INVALID
    assert call(n_stages=-1) == INVALID and call(stages=None, n_stages=1) == INVALID and call(stages=_stages(7)) == INVALID
    assert call(stages=_stages(nv.INGEST_AFFINE_DATA)) == INVALID                                    # without consts_dev
    assert call(stages=_stages(nv.INGEST_AFFINE_DATA, nv.INGEST_AFFINE_DATA), n_stages=2, consts=fake) == INVALID
    assert call(batch=0, stages=_stages(nv.INGEST_AFFINE, nv.INGEST_AFFINE_DATA), n_stages=2, consts=fake) == OK
    assert call(consts=ctypes.c_void_p(0x1002)) == INVALID
    # not built: interleaved with C != 3; per-channel clamp pairs for more than four channels
    assert call(geom=_geom(c=4, layout=NHWC)) == UNSUPPORTED and call(geom=_geom(c=1, layout=BGR), dtype=U8) == UNSUPPORTED
    by_channel = _stages(nv.INGEST_CLAMP)
    by_channel[0].hi[2] = 0.5
    assert call(geom=_geom(c=5), stages=by_channel) == UNSUPPORTED and call(batch=0, geom=_geom(c=4), stages=by_channel) == OK
    # the model, and its LUT against the LDS
    assert call(model=nv.Icrf(lut_dev=0x2000, n_points=256, interp=7)) == INVALID
    assert call(model=nv.Icrf(lut_dev=0x2000, n_points=256, interp=-1)) == INVALID
    assert call(model=nv.Icrf(lut_dev=None, n_points=256, interp=nv.INTERP_LINEAR)) == INVALID
    assert call(model=nv.Icrf(lut_dev=0x2000, n_points=1, interp=nv.INTERP_LINEAR)) == INVALID
    assert call(model=nv.Icrf(lut_dev=0x2000, n_points=1 << 20, interp=nv.INTERP_CATMULL)) == TOO_LARGE
    assert call(batch=0, model=nv.Icrf(lut_dev=0x2000, n_points=160 * 1024 // (3 * 16), interp=nv.INTERP_CATMULL)) == OK
    assert call(batch=0, model=nv.Icrf(lut_dev=0x2000, n_points=160 * 1024 // (3 * 16) + 1, interp=nv.INTERP_CATMULL)) == TOO_LARGE
    # the frame count so far
    assert call(before=-1.0) == INVALID and call(before=float("nan")) == INVALID and call(batch=0, before=12.0) == OK


def _T():
    from clair_torch_amd.common import transforms
    return transforms


class _Recorder:
    """Stands in for clair_torch_amd.ops inside compute_video_mean_and_std and its staging: records the calls."""

    def __init__(self):
        self.calls = []

    def strided_downscale(self, images, step, layout="nchw"):
        assert step == 1
        return images

    def ingest_shape(self, shape, layout="nchw"):
        from clair_torch_amd import ops
        return ops.ingest_shape(shape, layout)

    def ingest_transform(self, images, stages, layout="nchw", consts=None):
        from clair_torch_amd import ops
        self.calls.append(("ingest_transform", images.dtype, tuple(stages), layout))
        return torch.zeros(ops.ingest_shape(tuple(images.shape), layout))

    def video_stats_batch(self, frames, mean, m2, frames_before, *, lut=None, interp=None, max_code=None, layout="nchw"):
        self.calls.append(("video_stats_batch", frames.dtype, tuple(mean.shape), frames_before, max_code, layout))
        mean.zero_(), m2.zero_()

    def video_stats_ingest_batch(self, frames, stages, mean, m2, frames_before, *, lut=None, interp=None, tile=None, layout="nchw",
                                 consts=None):
        self.calls.append(("video_stats_ingest_batch", frames.dtype, tuple(stages), tuple(mean.shape), frames_before, layout))
        mean.zero_(), m2.zero_()


def _loader(frames):
    from clair_torch_amd.datasets import StackDataset, custom_collate

    class Frames(StackDataset):  # raw frames of any layout (StackDataset itself insists on (N,C,H,W))
        def __init__(self):
            self.values, self.stds, self.exposure_times = frames, None, [1.0] * len(frames)
            self.files = list(range(len(frames)))
            from clair_torch_amd.common.enums import MissingStdMode
            self.missing_std_mode, self.materialize_std, self.std_hint = MissingStdMode.NONE, False, None

        def __len__(self):
            return len(self.exposure_times)

    return DataLoader(Frames(), batch_size=2, shuffle=False, collate_fn=custom_collate)


def test_compute_video_mean_and_std_routes(monkeypatch):
    T = _T()
    from clair_torch_amd.inference import _staging, inferential_statistics as vs
    cpu = torch.device("cpu")
    monkeypatch.setattr(vs, "resolve_device", lambda device: cpu)
    u16 = torch.arange(4 * 3 * 2 * 5, dtype=torch.int32).reshape(4, 3, 2, 5).to(torch.uint16)
    raw = torch.zeros((4, 2, 5, 3), dtype=torch.uint16)
    f32 = torch.rand((4, 3, 2, 5))
    black = [T.CastTo("float32"), T.Normalize(1023, 64)]
    stages = (("affine", 64, 959, 1.0, 0.0),)

    def run(frames, chain, **kw):
        rec = _Recorder()
        monkeypatch.setattr(vs, "ops", rec)
        monkeypatch.setattr(_staging, "ops", rec)
        mean, std = vs.compute_video_mean_and_std(_loader(frames), "cuda", None, gpu_transforms=chain, **kw)
        assert mean.dtype == torch.float32 and tuple(mean.shape) == (3, 2, 5)
        return rec.calls

    # a black level on raw codes: the fused front, batch after batch, never ct_ingest_transform; the state is planar
    for frames, chain, layout in ((u16, black, "nchw"), (raw, [T.CvToTorch()] + black, "nhwc_bgr")):
        for kw in ({}, {"fused_ingest": True}):
            assert run(frames, chain, **kw) == [("video_stats_ingest_batch", torch.uint16, stages, (3, 2, 5), 0, layout),
                                                ("video_stats_ingest_batch", torch.uint16, stages, (3, 2, 5), 2, layout)]
        # fused_ingest=False: the two launches, as before
        for kw in ({"fused_ingest": False},):
            assert run(frames, chain, **kw) == [("ingest_transform", torch.uint16, stages, layout),
                                                ("video_stats_batch", torch.float32, (3, 2, 5), 0, None, "nchw"),
                                                ("ingest_transform", torch.uint16, stages, layout),
                                                ("video_stats_batch", torch.float32, (3, 2, 5), 2, None, "nchw")]
    # route "code" and float32 frames: what they always did, with either flag
    pair = [T.CastTo("float32"), T.Normalize(255, 0)]
    for flag in (True, False):
        assert run(u16, pair, fused_ingest=flag) == [("video_stats_batch", torch.uint16, (3, 2, 5), 0, 255.0, "nchw"),
                                                     ("video_stats_batch", torch.uint16, (3, 2, 5), 2, 255.0, "nchw")]
        assert run(f32, None, fused_ingest=flag) == [("video_stats_batch", torch.float32, (3, 2, 5), 0, None, "nchw"),
                                                     ("video_stats_batch", torch.float32, (3, 2, 5), 2, None, "nchw")]
        # float32 frames behind a chain (route "ingest"): there is no copy to save, the chain is executed first
        assert T.plan_staging(f32[:2], black).route == "ingest"
        assert run(f32, black, fused_ingest=flag) == [("ingest_transform", torch.float32, stages, "nchw"),
                                                      ("video_stats_batch", torch.float32, (3, 2, 5), 0, None, "nchw"),
                                                      ("ingest_transform", torch.float32, stages, "nchw"),
                                                      ("video_stats_batch", torch.float32, (3, 2, 5), 2, None, "nchw")]


def test_front_end_without_a_device():
    from clair_torch_amd import ops
    state = torch.zeros((3, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.video_stats_ingest_batch(torch.zeros((2, 3, 4, 4), dtype=torch.uint8), [("affine", 0.0, 1.0, 1.0, 0.0)], state,
                                     state.clone(), 0)
