"""Several video batches per launch without a GPU: ct_video_stats_batches and ct_video_stats_ingest_batches are declared,
exported and validate every batch before any launch; compute_video_mean_and_std queues staged batches for them only when
``batches_per_launch`` asks for it; the front ends have no CPU path."""
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


def test_entry_points_are_declared_and_exported(lib):
    from clair_torch_amd import _native as nv
    from clair_torch_amd import build, ops
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "clair_hip.h")).read(), flags=re.S)
    for name, n_args in (("ct_video_stats_batches", 12), ("ct_video_stats_ingest_batches", 14)):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header)
        assert name in nv.EXPORTS and hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == n_args
        declared = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", header, flags=re.S).group(1)
        assert len(declared.split(",")) == n_args
    assert re.search(r"#define\s+CT_ABI_VERSION\s+3\b", header)
    assert re.search(r"#define\s+CT_STATS_MAX_BATCHES\s+16\b", header) and re.search(r"#define\s+CT_STATS_REQUIRE_ONE_LAUNCH\s+1u", header)
    assert nv.STATS_MAX_BATCHES == 16 and nv.STATS_REQUIRE_ONE_LAUNCH == 1 and ops.MAX_STATS_BATCHES == 16
    assert "ct_stats_multi.hip" in build.SOURCES and "ct_stats_ingest_multi.hip" in build.SOURCES
    assert "ct_stats_kernel.hpp" in build.HEADERS
    assert lib.ct_abi_version() == 3 and nv.ABI_VERSION == 3


def _arrays(frames, sizes):
    k = max(len(sizes), 1)
    return (ctypes.c_void_p * k)(*frames), (ctypes.c_int32 * k)(*sizes)


FAKE = 0x1000  # never dereferenced: validation fails first, there is nothing to launch, or the route is refused


@pytest.mark.parametrize("form", ["code", "ingest"])
def test_batches_validate_before_any_launch(lib, form):
    from clair_torch_amd import _native as nv
    U8, U16, F32 = nv.DTYPE_U8, nv.DTYPE_U16, nv.DTYPE_F32
    ONE = nv.STATS_REQUIRE_ONE_LAUNCH
    linear = nv.Icrf(lut_dev=0x2000, n_points=256, interp=nv.INTERP_LINEAR)
    one = _stages(nv.INGEST_AFFINE)
    fake = ctypes.c_void_p(FAKE)

    def call(sizes=(2, 3), frames=None, dtype=U16, geom=None, stages=one, n_stages=1, consts=None, model=linear, before=0.0,
             mean=fake, m2=fake, flags=ONE, n=None, null_frames=False, null_sizes=False, max_code=1023.0):
        geom = _geom() if geom is None else geom
        frames = [FAKE] * len(sizes) if frames is None else frames
        f_arr, s_arr = _arrays(frames, sizes)
        c_arr = None if consts is None else (ctypes.c_void_p * len(consts))(*consts)
        n = len(sizes) if n is None else n
        f_arr, s_arr = (None if null_frames else f_arr), (None if null_sizes else s_arr)
        if form == "code":
            return lib.ct_video_stats_batches(f_arr, s_arr, n, dtype, max_code, ctypes.byref(geom), ctypes.byref(model), before,
                                              mean, m2, flags, None)
        return lib.ct_video_stats_ingest_batches(f_arr, s_arr, n, dtype, ctypes.byref(geom), stages, n_stages, c_arr,
                                                 ctypes.byref(model), before, mean, m2, flags, None)

    # the list itself
    assert call(sizes=(), n=0) == INVALID and call(sizes=(1,) * 17) == INVALID and call(n=-1) == INVALID
    assert call(null_frames=True) == INVALID and call(null_sizes=True) == INVALID
    # nothing to do: CT_OK without a launch, with or without a state
    assert call(sizes=(0, 0, 0)) == OK and call(sizes=(0,)) == OK and call(sizes=(0,) * 16, mean=None, m2=None) == OK
    assert call(sizes=(0, 0), frames=[None, None], before=12.0) == OK
    # a negative size in any position
    for sizes in ((-1, 2), (2, -1), (0, 0, -3)):
        assert call(sizes=sizes) == INVALID
    # what cannot run as one launch is refused instead, with the flag: a batch of more than 32 frames
    assert call(sizes=(33, 2)) == UNSUPPORTED and call(sizes=(2, 0, 33)) == UNSUPPORTED
    assert call(sizes=(32, 33), mean=None) == INVALID  # ... but only after every batch has been judged
    # a NULL state or NULL frames with work to do, in any position
    assert call(mean=None) == INVALID and call(m2=None) == INVALID
    assert call(sizes=(0, 2), mean=None) == INVALID
    assert call(frames=[FAKE, None]) == INVALID and call(sizes=(0, 2, 2), frames=[None, FAKE, None]) == INVALID
    # the single-batch refusals through any batch position (empty batches are judged too)
    for sizes in ((2, 3), (0, 2, 3), (0, 0)):
        assert call(sizes=sizes, dtype=7) in (INVALID, UNSUPPORTED) and call(sizes=sizes, dtype=-1) in (INVALID, UNSUPPORTED)
        assert call(sizes=sizes, geom=_geom(layout=3)) == INVALID and call(sizes=sizes, geom=_geom(layout=-1)) == INVALID
        assert call(sizes=sizes, geom=_geom(c=0)) == INVALID and call(sizes=sizes, geom=_geom(h=-1)) == INVALID
        assert call(sizes=sizes, geom=_geom(h=4, h_global=3)) == INVALID
        assert call(sizes=sizes, geom=_geom(h=4, h_global=6, row_offset=3)) == INVALID
        assert call(sizes=sizes, geom=_geom(h=1 << 15, w=1 << 15)) == TOO_LARGE
        short = _geom()
        short.image_stride = 47
        assert call(sizes=sizes, geom=short) == INVALID
        assert call(sizes=sizes, model=nv.Icrf(lut_dev=0x2000, n_points=256, interp=7)) == INVALID
        assert call(sizes=sizes, model=nv.Icrf(lut_dev=None, n_points=256, interp=nv.INTERP_LINEAR)) == INVALID
        assert call(sizes=sizes, model=nv.Icrf(lut_dev=0x2000, n_points=1, interp=nv.INTERP_LINEAR)) == INVALID
        assert call(sizes=sizes, model=nv.Icrf(lut_dev=0x2000, n_points=1 << 20, interp=nv.INTERP_CATMULL)) == TOO_LARGE  # the LDS
        assert call(sizes=sizes, before=-1.0) == INVALID
    if form == "code":
        assert call(dtype=7) == UNSUPPORTED and call(max_code=0.0) == UNSUPPORTED  # as ct_video_stats_batch answers them
        assert call(dtype=F32, sizes=(33, 2)) == UNSUPPORTED and call(dtype=U8, sizes=(0, 0), max_code=255.0) == OK
    else:
        assert call(dtype=7) == INVALID and call(dtype=F32) == UNSUPPORTED and call(dtype=F32, sizes=(0, 0)) == UNSUPPORTED
        assert call(before=float("nan")) == INVALID and call(sizes=(0, 0), before=float("nan")) == INVALID
        assert call(frames=[FAKE, FAKE + 1]) == INVALID  # uint16 at an odd address
        assert call(mean=ctypes.c_void_p(FAKE + 2)) == INVALID
        # the stage list and the constants
        assert call(stages=_stages(*[nv.INGEST_AFFINE] * 5), n_stages=5) == INVALID and call(stages=None, n_stages=1) == INVALID
        data = _stages(nv.INGEST_AFFINE_DATA)
        assert call(stages=data) == INVALID and call(stages=data, consts=[FAKE, None]) == INVALID  # a data stage without constants
        assert call(stages=data, consts=[FAKE, FAKE + 2]) == INVALID                              # misaligned constants
        assert call(sizes=(0, 0), stages=data, consts=[FAKE, FAKE]) == OK
        assert call(geom=_geom(c=4, layout=nv.LAYOUT_NHWC)) == UNSUPPORTED
        # batches with and without constants cannot share a launch
        assert call(consts=[FAKE, None]) == UNSUPPORTED and call(sizes=(2, 0, 2), consts=[None, FAKE, FAKE]) == UNSUPPORTED
        assert call(sizes=(0, 0, 0), consts=[None, FAKE, None]) == OK


def test_the_two_forms_differ_where_their_single_batch_entry_points_do(lib):
    """What the code form and the ingest form of the batch list do NOT share, told apart by status alone (nothing launches):
    the code form looks at a batch's pointers before the geometry, batch by batch, and has no empty image; the ingest form
    judges every batch first, then answers an empty image, and only then looks at pointers."""
    from clair_torch_amd import _native as nv
    ONE = nv.STATS_REQUIRE_ONE_LAUNCH
    linear = nv.Icrf(lut_dev=0x2000, n_points=256, interp=nv.INTERP_LINEAR)
    above_lds = nv.Icrf(lut_dev=0x2000, n_points=1 << 20, interp=nv.INTERP_CATMULL)
    huge = _geom(h=1 << 15, w=1 << 15)
    one = _stages(nv.INGEST_AFFINE)

    def code(sizes, frames, geom=None, model=linear, mean=FAKE, m2=FAKE, flags=ONE):
        f_arr, s_arr = _arrays(frames, sizes)
        return lib.ct_video_stats_batches(f_arr, s_arr, len(sizes), nv.DTYPE_U16, 1023.0, ctypes.byref(geom or _geom()), ctypes.byref(model),
                                          0.0, ctypes.c_void_p(mean), ctypes.c_void_p(m2), flags, None)

    def ingest(sizes, frames, geom=None, model=linear, mean=FAKE, m2=FAKE, flags=ONE):
        f_arr, s_arr = _arrays(frames, sizes)
        return lib.ct_video_stats_ingest_batches(f_arr, s_arr, len(sizes), nv.DTYPE_U16, ctypes.byref(geom or _geom()), one, 1, None,
                                                 ctypes.byref(model), 0.0, ctypes.c_void_p(mean), ctypes.c_void_p(m2), flags, None)

    # a lone empty batch is a list of one in the code form (the single-batch entry point refuses a size of 0), with the list's
    # LDS test; the ingest form hands it to its single-batch entry point, which takes a size of 0 and tests the LDS itself
    for flags in (0, ONE):
        assert code((0,), [None], mean=None, m2=None, flags=flags) == OK and ingest((0,), [None], mean=None, m2=None, flags=flags) == OK
        assert code((0,), [None], model=above_lds, flags=flags) == TOO_LARGE and ingest((0,), [None], model=above_lds, flags=flags) == TOO_LARGE
        assert code((0,), [None], geom=_geom(c=0), flags=flags) == INVALID and ingest((0,), [None], geom=_geom(c=0), flags=flags) == INVALID
    # a lone batch with frames goes to the single-batch entry point in both: its refusals, in its order
    assert code((2,), [None], geom=huge) == INVALID and ingest((2,), [None], geom=huge) == TOO_LARGE
    assert code((2,), [FAKE], model=above_lds) == TOO_LARGE and ingest((2,), [FAKE], model=above_lds) == TOO_LARGE
    # pointers against geometry: the code form refuses the missing pointer of batch 0 before it looks at the image, and the
    # image (in batch 0's turn) before the missing pointer of batch 1; the ingest form judges every batch before any pointer
    assert code((2, 3), [None, FAKE], geom=huge) == INVALID and code((2, 3), [FAKE, FAKE], geom=huge, mean=None) == INVALID
    assert code((2, 3), [FAKE, None], geom=huge) == TOO_LARGE and code((0, 3), [None, None], geom=huge, mean=None) == TOO_LARGE
    assert code((2, 3), [None, FAKE], model=above_lds) == INVALID and code((2, 3), [FAKE, None], model=above_lds) == TOO_LARGE
    for frames in ([None, FAKE], [FAKE, None], [None, None]):
        assert ingest((2, 3), frames, geom=huge) == TOO_LARGE and ingest((2, 3), frames, model=above_lds) == TOO_LARGE
        assert ingest((2, 3), frames, geom=huge, mean=None, m2=None) == TOO_LARGE
        assert ingest((2, 3), frames) == INVALID
    # an empty image: CT_OK in the ingest form before any pointer is looked at, with or without the flag, whatever the sizes
    # (33 frames included: there is nothing to refuse a launch for); the code form has no empty image
    for geom in (_geom(h=0), _geom(w=0)):
        for flags in (0, ONE):
            for sizes in ((2, 3), (0, 2), (33, 2), (2,), (0, 0)):
                assert ingest(sizes, [None] * len(sizes), geom=geom, mean=None, m2=None, flags=flags) == OK
                assert code(sizes, [FAKE] * len(sizes), geom=geom, flags=flags) == INVALID
    assert ingest((2, -1), [None, None], geom=_geom(h=0), mean=None) == INVALID  # ... but after every batch has been judged
    # more than 32 frames with the flag: refused only where two batches have frames, and after the pointers
    assert code((33, 0, 2), [FAKE, None, FAKE]) == UNSUPPORTED and ingest((33, 0, 2), [FAKE, None, FAKE]) == UNSUPPORTED
    assert code((33, 0, 2), [FAKE, None, None]) == INVALID and ingest((33, 0, 2), [FAKE, None, None]) == INVALID


def _T():
    from clair_torch_amd.common import transforms
    return transforms


class _Recorder:
    """Stands in for clair_torch_amd.ops inside compute_video_mean_and_std and its staging: records the calls."""

    def __init__(self, grouped=True):
        self.calls = []
        if not grouped:  # what the recorder of tests/test_video_ingest_host.py has: the single-batch methods alone
            self.video_stats_batches = self.video_stats_ingest_batches = None

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

    def video_stats_batches(self, frames_list, mean, m2, frames_before, *, lut=None, interp=None, max_code=None, layout="nchw"):
        self.calls.append(("video_stats_batches", [(f.dtype, f.shape[0]) for f in frames_list], tuple(mean.shape), frames_before,
                           max_code, layout))
        mean.zero_(), m2.zero_()

    def video_stats_ingest_batches(self, frames_list, stages, mean, m2, frames_before, *, lut=None, interp=None, tile=None,
                                   layout="nchw", consts=None):
        self.calls.append(("video_stats_ingest_batches", [(f.dtype, f.shape[0]) for f in frames_list], tuple(stages),
                           tuple(mean.shape), frames_before, layout, consts))
        mean.zero_(), m2.zero_()


def _loader(frames, batch_size=2):
    from clair_torch_amd.datasets import StackDataset, custom_collate

    class Frames(StackDataset):  # raw frames of any layout (StackDataset itself insists on (N,C,H,W))
        def __init__(self):
            self.values, self.stds, self.exposure_times = frames, None, [1.0] * len(frames)
            self.files = list(range(len(frames)))
            from clair_torch_amd.common.enums import MissingStdMode
            self.missing_std_mode, self.materialize_std, self.std_hint = MissingStdMode.NONE, False, None

        def __len__(self):
            return len(self.exposure_times)

    return DataLoader(Frames(), batch_size=batch_size, shuffle=False, collate_fn=custom_collate)


@pytest.fixture
def run(monkeypatch):
    from clair_torch_amd.inference import _staging, inferential_statistics as vs
    monkeypatch.setattr(vs, "resolve_device", lambda device: torch.device("cpu"))

    def run(loader, chain, grouped=True, **kw):
        rec = _Recorder(grouped)
        monkeypatch.setattr(vs, "ops", rec)
        monkeypatch.setattr(_staging, "ops", rec)
        mean, std = vs.compute_video_mean_and_std(loader, "cuda", None, gpu_transforms=chain, **kw)
        assert mean.dtype == torch.float32 and tuple(mean.shape) == (3, 2, 5)
        return rec.calls

    return run


def test_default_is_one_launch_per_batch(run):
    """batches_per_launch omitted or 1: the calls tests/test_video_ingest_host.py asserts, and no grouped method is touched."""
    T = _T()
    u16 = torch.arange(4 * 3 * 2 * 5, dtype=torch.int32).reshape(4, 3, 2, 5).to(torch.uint16)
    raw = torch.zeros((4, 2, 5, 3), dtype=torch.uint16)
    f32 = torch.rand((4, 3, 2, 5))
    black = [T.CastTo("float32"), T.Normalize(1023, 64)]
    pair = [T.CastTo("float32"), T.Normalize(255, 0)]
    stages = (("affine", 64, 959, 1.0, 0.0),)
    for kw in ({}, {"batches_per_launch": 1}):
        for frames, chain, layout in ((u16, black, "nchw"), (raw, [T.CvToTorch()] + black, "nhwc_bgr")):
            assert run(_loader(frames), chain, grouped=False, **kw) == [
                ("video_stats_ingest_batch", torch.uint16, stages, (3, 2, 5), 0, layout),
                ("video_stats_ingest_batch", torch.uint16, stages, (3, 2, 5), 2, layout)]
            assert run(_loader(frames), chain, grouped=False, fused_ingest=False, **kw) == [
                ("ingest_transform", torch.uint16, stages, layout), ("video_stats_batch", torch.float32, (3, 2, 5), 0, None, "nchw"),
                ("ingest_transform", torch.uint16, stages, layout), ("video_stats_batch", torch.float32, (3, 2, 5), 2, None, "nchw")]
        assert run(_loader(u16), pair, grouped=False, **kw) == [("video_stats_batch", torch.uint16, (3, 2, 5), 0, 255.0, "nchw"),
                                                                ("video_stats_batch", torch.uint16, (3, 2, 5), 2, 255.0, "nchw")]
        assert run(_loader(f32), black, grouped=False, **kw) == [
            ("ingest_transform", torch.float32, stages, "nchw"), ("video_stats_batch", torch.float32, (3, 2, 5), 0, None, "nchw"),
            ("ingest_transform", torch.float32, stages, "nchw"), ("video_stats_batch", torch.float32, (3, 2, 5), 2, None, "nchw")]


def test_grouped_routes(run):
    T = _T()
    u16 = torch.arange(10 * 3 * 2 * 5, dtype=torch.int32).reshape(10, 3, 2, 5).to(torch.uint16)
    raw = torch.zeros((10, 2, 5, 3), dtype=torch.uint16)
    f32 = torch.rand((10, 3, 2, 5))
    black = [T.CastTo("float32"), T.Normalize(1023, 64)]
    pair = [T.CastTo("float32"), T.Normalize(255, 0)]
    stages = (("affine", 64, 959, 1.0, 0.0),)
    four, one = [(torch.uint16, 2)] * 4, [(torch.uint16, 2)]
    # 5 batches of 2 in groups of 4: one call of 4 batches, then one of 1 with the 8 frames before it
    for frames, chain, layout in ((u16, black, "nchw"), (raw, [T.CvToTorch()] + black, "nhwc_bgr")):
        assert run(_loader(frames), chain, batches_per_launch=4) == [
            ("video_stats_ingest_batches", four, stages, (3, 2, 5), 0, layout, None),
            ("video_stats_ingest_batches", one, stages, (3, 2, 5), 8, layout, None)]
    assert run(_loader(u16), pair, batches_per_launch=4) == [("video_stats_batches", four, (3, 2, 5), 0, 255.0, "nchw"),
                                                             ("video_stats_batches", one, (3, 2, 5), 8, 255.0, "nchw")]
    assert run(_loader(u16), pair, batches_per_launch=16) == [("video_stats_batches", [(torch.uint16, 2)] * 5, (3, 2, 5), 0, 255.0, "nchw")]
    assert run(_loader(u16), pair, batches_per_launch=2) == [("video_stats_batches", [(torch.uint16, 2)] * 2, (3, 2, 5), k, 255.0, "nchw")
                                                             for k in (0, 4)] + [("video_stats_batches", one, (3, 2, 5), 8, 255.0, "nchw")]
    # fused_ingest=False, and float32 frames behind a chain: ct_ingest_transform per batch, the float32 stacks grouped
    f4, f1 = [(torch.float32, 2)] * 4, [(torch.float32, 2)]
    for frames, kw in ((u16, {"fused_ingest": False}), (f32, {})):
        tr = ("ingest_transform", frames.dtype, stages, "nchw")
        assert run(_loader(frames), black, batches_per_launch=4, **kw) == [
            tr, tr, tr, tr, ("video_stats_batches", f4, (3, 2, 5), 0, None, "nchw"), tr, ("video_stats_batches", f1, (3, 2, 5), 8, None, "nchw")]


def test_a_key_change_flushes(run):
    """The last batch of a loader is shorter -- still the same key (the frame shape, not the batch size) -- but a change of
    dtype mid-stream ends the group."""
    T = _T()
    from clair_torch_amd.datasets import custom_collate
    pair = [T.CastTo("float32"), T.Normalize(255, 0)]
    u16 = torch.zeros((5, 3, 2, 5), dtype=torch.uint16)
    assert run(_loader(u16), pair, batches_per_launch=4) == [
        ("video_stats_batches", [(torch.uint16, 2), (torch.uint16, 2), (torch.uint16, 1)], (3, 2, 5), 0, 255.0, "nchw")]

    class Mixed(torch.utils.data.Dataset):  # two uint8 batches, then two uint16 ones, then a uint8 one
        kinds = [torch.uint8] * 4 + [torch.uint16] * 4 + [torch.uint8] * 2
        stacks = {k: torch.zeros((10, 3, 2, 5), dtype=k) for k in (torch.uint8, torch.uint16)}  # (batches are views, as StackDataset's)
        files = list(range(10))

        def __len__(self):
            return 10

        def __getitem__(self, i):
            return i, self.stacks[self.kinds[i]][i], None, {"exposure_time": 1.0}

    loader = DataLoader(Mixed(), batch_size=2, shuffle=False, collate_fn=custom_collate)
    calls = run(loader, pair, batches_per_launch=4)
    assert calls == [("video_stats_batches", [(torch.uint8, 2)] * 2, (3, 2, 5), 0, 255.0, "nchw"),
                     ("video_stats_batches", [(torch.uint16, 2)] * 2, (3, 2, 5), 4, 255.0, "nchw"),
                     ("video_stats_batches", [(torch.uint8, 2)], (3, 2, 5), 8, 255.0, "nchw")]


def test_batches_per_launch_range(run):
    u16 = torch.zeros((4, 3, 2, 5), dtype=torch.uint16)
    for bad in (0, 17, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="batches_per_launch"):
            run(_loader(u16), None, batches_per_launch=bad)


def test_front_ends_without_a_device():
    from clair_torch_amd import ops
    state = torch.zeros((3, 4, 4))
    frames = [torch.zeros((2, 3, 4, 4), dtype=torch.uint8) for _ in range(2)]
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.video_stats_batches(frames, state, state.clone(), 0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.video_stats_ingest_batches(frames, [("affine", 0.0, 1.0, 1.0, 0.0)], state, state.clone(), 0)
    for front, args in ((ops.video_stats_batches, ()), (ops.video_stats_ingest_batches, ([],))):
        with pytest.raises(ValueError, match="non-empty"):
            front([], *args, state, state.clone(), 0)
        with pytest.raises(ValueError, match="at most 16"):
            front(frames * 9, *args, state, state.clone(), 0)
