"""ct_linearize_ingest_strided on the device: a StridedDownscale, a gpu_transforms chain and the linearization in one pass
over the raw frames.
  1. ``ops.linearize_ingest_frames_strided(x, s, ...)``  ==  ``ops.linearize_ingest_frames(ops.strided_downscale(x, s), ...)``
     bit for bit: every dtype and layout, every model and uncertainty mode, a per-channel clamp, per-frame constants, steps
     that leave one row, planes that are no multiple of 4 (unaligned planes) or of 3 (the LUT-row rule), an output buffer
     that starts 4 bytes behind a packet boundary;
  2. against the float64 references of tests/_linearize_refs.py on the host-sliced frames, at that module's tolerances;
  3. every uint8 / uint16 code through the one-stage chain x / max_code  ==  ``ops.linearize_frames(..., max_code=...)``: what
     lets a code pair with a downscale take the pipeline;
  4. the refusals;
  5. linearize_dataset_generator with a StridedDownscale takes the pipeline and yields what it yields for host-sliced frames
     without the downscale."""
import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

import _linearize_refs as R

pytestmark = pytest.mark.gpu

F = 3
SHAPES = [(7, 13), (8, 16), (5, 3)]
STEPS = [1, 2, 3, 5, 9]
CLAMP3 = [(0.0, 1.0), (0.125, 0.7), (-0.25, 0.3333)]
_NP = {"u8": np.uint8, "u16": np.uint16, "f32": np.float32}
# (sub, div) of the black-level stage per dtype: codes below the black level and above the white level occur
_AFFINE = {"u8": (16.0, 200.0), "u16": (4096.0, 52000.0), "f32": (0.05, 0.9)}
# (model, uncertainty mode)
MODES = [("lookup", "none"), ("linear", "none"), ("linear", "constant"), ("linear", "explicit"), ("catmull", "multiplier"),
         ("catmull", "explicit"), (None, "multiplier"), (None, "explicit")]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from clair_torch_amd import _native
    _native.load()
    return torch.device("cuda:0")


def _lut(points=64):
    return np.stack([np.linspace(0, 1, points, dtype=np.float32) ** np.float32(p) for p in (2.2, 2.4, 2.6)])


def _frames(rng, dtype, h, w, n=F):
    """Planar (n, 3, h, w) host frames."""
    if dtype == "f32":
        return (rng.random((n, 3, h, w)) * 1.2 - 0.1).astype(np.float32)
    return rng.integers(0, 256 if dtype == "u8" else 65536, size=(n, 3, h, w)).astype(_NP[dtype])


def _in_layout(planar, layout):
    """Planar host frames as the stack the kernel reads: itself, or the (n, h, w, 3) BGR frames of an OpenCV reader."""
    if layout == "nchw":
        return np.ascontiguousarray(planar)
    return np.ascontiguousarray(planar[:, ::-1].transpose(0, 2, 3, 1))


def _stages(dtype):
    sub, div = _AFFINE[dtype]
    return [("affine", sub, div, 1.0, 0.0), ("clamp", CLAMP3)]


def _host_chain(planar, dtype):
    """The stages of ``_stages`` in float32 on planar host frames, every operation rounded on its own."""
    sub, div = (np.float32(v) for v in _AFFINE[dtype])
    v = (planar.astype(np.float32) - sub) / div
    v = v * np.float32(1.0) + np.float32(0.0)
    lo = np.array([p[0] for p in CLAMP3], dtype=np.float32).reshape(1, 3, 1, 1)
    hi = np.array([p[1] for p in CLAMP3], dtype=np.float32).reshape(1, 3, 1, 1)
    return np.minimum(np.maximum(v, lo), hi).astype(np.float32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _std_args(std_mode, sigma_dev):
    if std_mode == "explicit":
        return dict(std=sigma_dev)
    return dict(std_mode=std_mode, std_value={"none": 0.0, "constant": R.STD_CONSTANT, "multiplier": R.STD_MULTIPLIER}[std_mode])


def test_the_shapes_cover_unaligned_planes_and_the_row_quirk():
    planes = {(-(-h // s)) * (-(-w // s)) for h, w in SHAPES for s in STEPS}
    assert any(p % 4 for p in planes) and any(p % 3 for p in planes) and 1 in {-(-h // 9) for h, _ in SHAPES}
    assert any(p % 4 and p % 3 and p > 4 for p in planes)


@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("hw", SHAPES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_equals_downscale_then_linearize_ingest(dev, hw, step):
    from clair_torch_amd import ops
    h, w = hw
    ho, wo = -(-h // step), -(-w // step)
    rng = np.random.default_rng(1000 * h + 10 * w + step)
    lut = torch.from_numpy(_lut()).to(dev)
    sigma = torch.from_numpy((0.001 + 0.02 * rng.random((F, 3, ho, wo))).astype(np.float32)).to(dev)
    for dtype in ("u8", "u16", "f32"):
        planar = _frames(rng, dtype, h, w)
        for layout in ("nchw", "nhwc_bgr"):
            x = torch.from_numpy(_in_layout(planar, layout)).to(dev)
            small = ops.strided_downscale(x, step, layout)
            for interp, std_mode in MODES:
                what = (dtype, layout, interp, std_mode)
                kw = dict(layout=layout, **_std_args(std_mode, sigma))
                lut_arg = lut if interp is not None else None
                want = ops.linearize_ingest_frames(small, _stages(dtype), lut_arg, interp, **kw)
                got = ops.linearize_ingest_frames_strided(x, step, _stages(dtype), lut_arg, interp, **kw)
                assert tuple(got[0].shape) == (F, 3, ho, wo), what
                assert _same(got[0], want[0]) and _same(got[1], want[1]), what
                lin_only = ops.linearize_ingest_frames_strided(x, step, _stages(dtype), lut_arg, interp, want_std=False, **kw)
                assert lin_only[1] is None and _same(lin_only[0], want[0]), what
            # per-frame constants of a data-dependent Normalize in front of the downscale: extrema of the FULL frames
            data = [("affine_data", 1.0, 0.0), ("clamp", CLAMP3)]
            consts = ops.ingest_extrema_frames(x, (), layout)
            want = ops.linearize_ingest_frames(small, data, lut, "linear", layout=layout, std=sigma, consts=consts)
            got = ops.linearize_ingest_frames_strided(x, step, data, lut, "linear", layout=layout, std=sigma, consts=consts)
            assert _same(got[0], want[0]) and _same(got[1], want[1]), (dtype, layout, "consts")
            # an output pair that starts 4 bytes behind a packet boundary: slot 0 holds three elements of every first plane
            n = F * 3 * ho * wo
            bufs = [torch.full((n + 1,), float("nan"), device=dev) for _ in range(2)]
            out = tuple(b[1:].view(F, 3, ho, wo) for b in bufs)
            assert out[0].data_ptr() % 16 == 4
            ops.linearize_ingest_frames_strided(x, step, data, lut, "linear", layout=layout, std=sigma, consts=consts, out=out)
            assert _same(out[0], want[0]) and _same(out[1], want[1]), (dtype, layout, "offset outputs")
            assert all(torch.isnan(b[0]).item() for b in bufs)  # the element in front of the outputs is untouched


@pytest.mark.parametrize("layout", ["nchw", "nhwc_bgr"])
def test_several_workgroups_per_plane(dev, layout):
    """133 x 261 at step 2: planes of 67 * 131 = 8777 elements (1 mod 4, 2 mod 3) span three workgroups of 4096 elements,
    and every output row ends inside a thread's group of 4."""
    from clair_torch_amd import ops
    rng = np.random.default_rng(31)
    x = torch.from_numpy(_in_layout(_frames(rng, "u16", 133, 261, n=2), layout)).to(dev)
    lut = torch.from_numpy(_lut()).to(dev)
    sigma = torch.from_numpy((0.001 + 0.02 * rng.random((2, 3, 67, 131))).astype(np.float32)).to(dev)
    small = ops.strided_downscale(x, 2, layout)
    for interp in ("linear", "catmull"):
        want = ops.linearize_ingest_frames(small, _stages("u16"), lut, interp, layout=layout, std=sigma)
        got = ops.linearize_ingest_frames_strided(x, 2, _stages("u16"), lut, interp, layout=layout, std=sigma)
        assert _same(got[0], want[0]) and _same(got[1], want[1]), interp


@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("hw", SHAPES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_against_the_float64_reference(dev, hw, step):
    """The host slices x[..., ::s, ::s] and runs the chain in float32; the float64 reference linearizes that."""
    from clair_torch_amd import ops
    h, w = hw
    rng = np.random.default_rng(7000 + 1000 * h + 10 * w + step)
    lut_host = _lut()
    lut = torch.from_numpy(lut_host).to(dev)
    for dtype, layout in (("u16", "nchw"), ("u8", "nhwc_bgr"), ("f32", "nhwc_bgr"), ("f32", "nchw")):
        planar = _frames(rng, dtype, h, w)
        x = torch.from_numpy(_in_layout(planar, layout)).to(dev)
        pixels = _host_chain(np.ascontiguousarray(planar[..., ::step, ::step]), dtype)
        explicit = (0.001 + 0.02 * rng.random(pixels.shape)).astype(np.float32)
        for interp, std_mode in MODES:
            sigma = {"none": None, "constant": np.full(pixels.shape, R.STD_CONSTANT, dtype=np.float32),
                     "multiplier": pixels * np.float32(R.STD_MULTIPLIER), "explicit": explicit}[std_mode]
            lin_ref, std_ref = R.linearize_f64(pixels, sigma, lut_host, interp)
            got = ops.linearize_ingest_frames_strided(x, step, _stages(dtype), lut if interp is not None else None, interp,
                                                      layout=layout, **_std_args(std_mode, torch.from_numpy(explicit).to(dev)))
            what = f"strided {dtype} {layout} {interp} {std_mode} {h}x{w} step {step}"
            R.check(got[0].cpu().numpy(), lin_ref, ("lin", interp), "lin " + what)
            if std_mode == "none":
                assert not got[1].any(), what
            else:
                R.check(got[1].cpu().numpy(), std_ref, ("std", interp), "std " + what)


@pytest.mark.parametrize("layout", ["nchw", "nhwc_bgr"])
@pytest.mark.parametrize("dtype", ["u8", "u16"])
def test_every_code_through_the_one_stage_chain_equals_the_code_route(dev, dtype, layout):
    """All 256 / 65 536 codes at the selected positions of a frame (junk between them), every code in every channel: the
    chain ("affine", 0, max_code, 1, 0) gives the bits of ct_linearize_std's folded normalisation -- value and
    uncertainty, every model.  This is what lets ``[CastTo, Normalize(max_code, 0)]`` with a StridedDownscale take the
    pipelined route of linearize_dataset_generator."""
    from clair_torch_amd import ops
    side, max_code = (16, 255.0) if dtype == "u8" else (256, 65535.0)
    step = 2
    rng = np.random.default_rng(11)
    grid = np.arange(side * side, dtype=np.int64).reshape(1, 1, side, side)
    codes = np.concatenate([grid, grid[..., ::-1, :], grid[..., ::-1]], axis=1).astype(_NP[dtype])  # (1, 3, side, side)
    full = rng.integers(0, side * side, size=(1, 3, side * step - 1, side * step)).astype(_NP[dtype])
    full[..., ::step, ::step] = codes
    x = torch.from_numpy(_in_layout(full, layout)).to(dev)
    small = torch.from_numpy(_in_layout(codes, layout)).to(dev)
    lut = torch.from_numpy(_lut(256)).to(dev)
    chain = [("affine", 0, max_code, 1, 0)]
    for interp, std_mode in (("lookup", "none"), ("linear", "multiplier"), ("linear", "constant"), ("catmull", "multiplier"),
                             (None, "multiplier")):
        kw = dict(std_mode=std_mode, std_value=0.05, layout=layout)
        lut_arg = lut if interp is not None else None
        want = ops.linearize_frames(small, lut_arg, interp, max_code=max_code, **kw)
        got = ops.linearize_ingest_frames_strided(x, step, chain, lut_arg, interp, **kw)
        assert _same(got[0], want[0]) and _same(got[1], want[1]), (interp, std_mode)


def test_refusals(dev):
    from clair_torch_amd import ops
    x = torch.zeros((2, 3, 8, 16), dtype=torch.uint16, device=dev)
    lut = torch.from_numpy(_lut()).to(dev)
    stages = _stages("u16")
    with pytest.raises(ValueError):  # a row band behind a downscale
        ops.linearize_ingest_frames_strided(x, 2, stages, lut, tile=ops.TileGeometry(h_global=16, row_offset=4))
    with pytest.raises(ValueError):
        ops.linearize_ingest_frames_strided(x, 2, stages, lut, tile=ops.TileGeometry(h_global=16, row_offset=0))
    with pytest.raises(RuntimeError, match="does not have a grad_fn"):  # LOOKUP with uncertainties
        ops.linearize_ingest_frames_strided(x, 2, stages, lut, "lookup", std_mode="constant", std_value=0.01)
    with pytest.raises(ValueError, match="step"):
        ops.linearize_ingest_frames_strided(x, 0, stages, lut)
    for shape in ((2, 3, 8, 16), (2, 3, 4, 7), (2, 4, 8, 3)):
        bad = torch.empty(shape, device=dev)
        with pytest.raises(ValueError, match="out"):
            ops.linearize_ingest_frames_strided(x, 2, stages, lut, out=(bad, torch.empty((2, 3, 4, 8), device=dev)))
    with pytest.raises(ValueError, match="std must be"):  # explicit uncertainties of the source shape
        ops.linearize_ingest_frames_strided(x, 2, stages, lut, std=torch.zeros((2, 3, 8, 16), device=dev))
    # step 1 with a row band is ct_linearize_ingest's band
    band = ops.TileGeometry(h_global=16, row_offset=4)
    want = ops.linearize_ingest_frames(x, stages, lut, "linear", tile=band, std_mode="constant", std_value=0.01)
    got = ops.linearize_ingest_frames_strided(x, 1, stages, lut, "linear", tile=band, std_mode="constant", std_value=0.01)
    assert _same(got[0], want[0]) and _same(got[1], want[1])


def test_the_registered_op(dev):
    from clair_torch_amd import ops, torch_ops  # noqa: F401 - registers clair_hip::
    rng = np.random.default_rng(5)
    x = torch.from_numpy(_frames(rng, "u16", 7, 13)).to(dev)
    lut = torch.from_numpy(_lut()).to(dev)
    flat = [0.0, 4096.0, 52000.0, 1.0, 0.0] + [0.0] * 8
    got = torch.ops.clair_hip.linearize_ingest_strided(x, 3, flat, lut, "linear", None, "multiplier", 0.05)
    want = ops.linearize_ingest_frames_strided(x, 3, [("affine", 4096.0, 52000.0, 1.0, 0.0)], lut, "linear", std_mode="multiplier",
                                               std_value=0.05)
    assert _same(got[0], want[0]) and _same(got[1], want[1]) and tuple(got[0].shape) == (F, 3, 3, 5)


# ---- linearize_dataset_generator ---------------------------------------------------------------------------------------------
N, H, W, STEP = 7, 9, 14, 2
HO, WO = 5, 7


def _T():
    from clair_torch_amd.common import transforms
    return transforms


def _model(dev, lut):
    from clair_torch_amd.common.enums import InterpMode
    from clair_torch_amd.models import ICRFModelDirect
    return ICRFModelDirect(icrf=torch.from_numpy(lut), interpolation_mode=InterpMode.LINEAR).to(dev)


def _dataset(values, times, stds=None, hint=None):
    """Planar (N,3,H,W) frames or (N,H,W,3) BGR frames as an OpenCV reader hands them over, with planar uncertainty images
    of any shape or a std hint (StackDataset itself insists on (N,C,H,W) values of one shape with their uncertainties)."""
    from clair_torch_amd.common.enums import MissingStdMode
    from clair_torch_amd.datasets import StackDataset

    class Frames(StackDataset):
        def __init__(self):
            self.values, self.stds, self.exposure_times = values, stds, times
            self.files, self.std_hint = list(range(len(times))), hint
            self.missing_std_mode = MissingStdMode.NONE if hint is None else MissingStdMode.MULTIPLIER
            self.missing_std_value, self.materialize_std = (0.0 if hint is None else hint[1]), hint is None

        def __len__(self):
            return len(self.exposure_times)

    return Frames()


def _refuse(*args, **kwargs):
    raise AssertionError("the list took the frame-by-frame route")
    yield  # pragma: no cover - a generator, like the function it stands in for


def _codes(rng):
    """(N,3,H,W) uint16 codes whose extrema per frame sit at positions a step of 2 selects, so that a data-dependent
    Normalize in front of the downscale (extrema of the full frame) and one fed the host-sliced frame (extrema of the
    selected pixels) form the same constants."""
    codes = rng.integers(500, 60000, size=(N, 3, H, W)).astype(np.uint16)
    for k in range(N):
        codes[k, 0, 0, 0] = 100 + k
        codes[k, 1, 2, 4] = 64000 + 10 * k
    return codes


@pytest.fixture(scope="module")
def stream_case():
    rng = np.random.default_rng(77)
    codes = _codes(rng)
    return dict(codes=codes, sliced=np.ascontiguousarray(codes[..., ::STEP, ::STEP]),
                sigma=(0.001 + 0.02 * rng.random((N, 3, HO, WO))).astype(np.float32),
                flat=(0.6 + 0.4 * rng.random((3, HO, WO))).astype(np.float32),
                flat_std=(0.01 * rng.random((3, HO, WO))).astype(np.float32), lut=_lut(256))


def _lists(T, chain_kind):
    cast = T.CastTo("float32")
    return {"black_level": [cast, T.Normalize(60000, 256), T.ClampAlongDims(1, CLAMP3)],
            "code_pair": [cast, T.Normalize(65535, 0)],
            "data_normalize": [cast, T.Normalize()]}[chain_kind]


@pytest.mark.parametrize("group_bytes", [1 << 20, 2 * 4 * 3 * HO * WO * 2], ids=["1MB", "groups_of_2"])
@pytest.mark.parametrize("extra", ["multiplier", "explicit_std", "flat_field", "cv_output"])
@pytest.mark.parametrize("frames_kind", ["planar", "raw_bgr"])
@pytest.mark.parametrize("chain_kind", ["black_level", "code_pair", "data_normalize"])
def test_generator_with_a_downscale_equals_host_sliced_frames(dev, monkeypatch, stream_case, chain_kind, frames_kind, extra,
                                                              group_bytes):
    """7 frames of 9x14x3 uint16 with StridedDownscale(2) behind the list take the pipeline (the frame-by-frame route is made
    to raise; on the parent commit it is the route these lists take) -- in one group at the default-sized 1 MB budget, in
    groups of 2 with ring re-use (3 slots, 4 groups) at the smaller one -- and yield, frame for frame, what the same
    generator yields for the host-sliced frames without the downscale."""
    T = _T()
    from clair_torch_amd.datasets import ArtefactStack, custom_collate
    from clair_torch_amd.inference import linearization, linearize_dataset_generator
    cs = stream_case
    model = _model(dev, cs["lut"])
    times = [float(k + 1) for k in range(N)]
    chain = _lists(T, chain_kind)
    lead = [T.CvToTorch()] if frames_kind == "raw_bgr" else []
    shape = (lambda a: _in_layout(a, "nhwc_bgr")) if frames_kind == "raw_bgr" else np.ascontiguousarray
    stds = torch.from_numpy(cs["sigma"]) if extra == "explicit_std" else None
    hint = ("multiplier", 0.05) if extra == "multiplier" else None
    ff = ArtefactStack(torch.from_numpy(cs["flat"]), torch.from_numpy(cs["flat_std"])) if extra == "flat_field" else None
    layout = "cv" if extra == "cv_output" else "planar"

    def run(values, transforms):
        ds = _dataset(torch.from_numpy(shape(values)), times, stds, hint)
        loader = DataLoader(ds, batch_size=1, shuffle=False, collate_fn=custom_collate)
        return list(linearize_dataset_generator(loader, "cuda", model, flatfield_dataset=ff, gpu_transforms=transforms,
                                                output_layout=layout))

    monkeypatch.setattr(linearization, "_GROUP_BYTES", group_bytes)
    want = run(cs["sliced"], lead + chain)
    with monkeypatch.context() as m:
        m.setattr(linearization, "_frame_by_frame", _refuse)
        got = run(cs["codes"], lead + chain + [T.StridedDownscale(STEP)])
    assert len(got) == len(want) == N
    out_shape = (HO, WO, 3) if layout == "cv" else (3, HO, WO)
    for k in range(N):
        assert got[k][0].device.type == "cpu" and tuple(got[k][0].shape) == tuple(got[k][1].shape) == out_shape
        assert float(got[k][2]["exposure_time"]) == times[k]
        assert _same(got[k][0], want[k][0]) and _same(got[k][1], want[k][1]), k
    assert not torch.equal(got[0][0], got[1][0])  # the frames differ, so the order is checked


def test_generator_refuses_full_size_uncertainty_images(dev, stream_case):
    T = _T()
    from clair_torch_amd.datasets import custom_collate
    from clair_torch_amd.inference import linearize_dataset_generator
    cs = stream_case
    ds = _dataset(torch.from_numpy(cs["codes"]), [float(k + 1) for k in range(N)], torch.full((N, 3, H, W), 0.01))
    loader = DataLoader(ds, batch_size=1, shuffle=False, collate_fn=custom_collate)
    ts = [T.CastTo("float32"), T.Normalize(60000, 256), T.StridedDownscale(STEP)]
    with pytest.raises(ValueError, match="downscaled shape"):
        next(iter(linearize_dataset_generator(loader, "cuda", _model(dev, cs["lut"]), gpu_transforms=ts)))


def test_generator_zero_range_frame_raises_at_its_position(dev, monkeypatch, stream_case):
    """Frame 4 of 7 constant, groups of 2, Normalize() in front of the downscale: frames 0 to 3 arrive with the bits of the
    host-sliced run, then the reference's ValueError, and nothing of frame 4's group behind it."""
    T = _T()
    from clair_torch_amd import ops
    from clair_torch_amd.datasets import custom_collate
    from clair_torch_amd.inference import linearization, linearize_dataset_generator
    cs = stream_case
    codes = cs["codes"].copy()
    codes[4] = 777
    model = _model(dev, cs["lut"])
    chain = [T.CastTo("float32"), T.Normalize()]

    def run(values, transforms):
        ds = _dataset(torch.from_numpy(values), [float(k + 1) for k in range(N)], hint=("multiplier", 0.05))
        loader = DataLoader(ds, batch_size=1, shuffle=False, collate_fn=custom_collate)
        seen = []
        try:
            for item in linearize_dataset_generator(loader, "cuda", model, gpu_transforms=transforms):
                seen.append(item)
        except ValueError as e:
            return seen, e
        return seen, None

    monkeypatch.setattr(linearization, "_GROUP_BYTES", 2 * 4 * 3 * HO * WO * 2)
    want, want_err = run(np.ascontiguousarray(codes[..., ::STEP, ::STEP]), chain)
    with monkeypatch.context() as m:
        m.setattr(linearization, "_frame_by_frame", _refuse)
        got, err = run(codes, chain + [T.StridedDownscale(STEP)])
    for seen, e in ((got, err), (want, want_err)):
        assert isinstance(e, ValueError) and str(e) == ops.ZERO_RANGE and len(seen) == 4
    for k in range(4):
        assert float(got[k][2]["exposure_time"]) == float(k + 1)
        assert _same(got[k][0], want[k][0]) and _same(got[k][1], want[k][1]), k
