"""The staging plan without a GPU: ``plan_staging`` picks, for every batch kind and transform list of a small corpus, the
route the entry points took before the plan existed, and ``stage_images`` issues the same device calls in the same order.

How ``EXPECTED`` was made (repeatable at the commit before ``plan_staging``): for every entry of the corpus below the old
two-step staging -- ``stage_images`` asked for the layout, followed, for a caller with explicit std / dark-field images
that got an interleaved stack back, by its second, planar staging -- ran on these CPU tensors with the four recording
stubs of ``_stubs`` in place of the ``ops`` calls and ``is_cuda`` answering True (``_OnDevice``).  The route was read off
the recorded calls (an extrema call: "ingest_data"; else a transform call: "ingest"; else a max_code: "code"; else
"torch"), step and step_first off the downscale call and its position, and for the ``planar`` column the calls of the
discarded first staging (none, or its one downscale) were dropped.  On plain CPU tensors the same run gave the same table
with every "ingest_data" cell replaced by the bare torch route."""
import pytest
import torch

from clair_torch_amd import ops
from clair_torch_amd.common import transforms as T
from clair_torch_amd.inference._staging import stage_images


class _OnDevice(torch.Tensor):
    """A CPU tensor that answers ``is_cuda`` with True: the one device property the route choice reads."""
    is_cuda = property(lambda self: True)


def _batches():
    out = {}
    for name, dtype in (("u8", torch.uint8), ("u16", torch.uint16), ("f32", torch.float32)):
        base = (torch.arange(2 * 3 * 6 * 10, dtype=torch.float32) * 7 % 251 + 1).to(dtype)
        out[name + "_planar"] = base.view(2, 3, 6, 10)
        out[name + "_raw"] = base.view(2, 6, 10, 3)
    out["u8_strided"] = out["u8_planar"].permute(0, 1, 3, 2)      # (2,3,10,6), not contiguous
    out["u16_3d"] = out["u16_planar"][0]                           # (3,6,10)
    return out


class _MyNormalize(T.Normalize):
    pass


class _Identity(T.BaseTransform):
    def __call__(self, x):
        return x


def _lists():
    cast, cv, sd, free = T.CastTo("float32"), T.CvToTorch(), T.StridedDownscale(2), T.Normalize()
    norm = T.Normalize(255, 0)
    return {
        "pair_255": [cast, norm],
        "pair_4095": [cast, T.Normalize(4095, 0)],
        "pair_65535": [cast, T.Normalize(65535, 0)],
        "cv_pair": [cv, cast, norm],
        "sd_pair": [sd, cast, norm],
        "pair_sd": [cast, norm, sd],
        "cv_sd_pair": [cv, sd, cast, norm],
        "cv_pair_sd": [cv, cast, norm, sd],
        "black_level": [cast, T.Normalize(4095, 64)],
        "cv_black_level": [cv, cast, T.Normalize(4095, 64)],
        "channel_clamp": [cast, norm, T.ClampAlongDims(1, [(0.0, 1.0), (0.125, 0.7), (-0.25, 0.3333)])],
        "data_both": [cast, free],
        "data_max": [cast, T.Normalize(None, 0)],
        "cv_data_both": [cv, cast, free],
        "sd_data": [sd, cast, free],
        "data_sd": [cast, free, sd],
        "two_data": [cast, free, T.Normalize(None, 0, (0.0, 2.0))],
        "float64": [T.CastTo("float64"), norm],
        "subclass": [cast, _MyNormalize(255, 0)],
        "identity": [cast, norm, _Identity()],
        "empty": [],
    }


# list -> batches -> "route layout step step_first max_code | device calls in order [!exception of stage_images]"; a pair
# where planar=False and planar=True differ.  Calls: D<step>:<layout> ops.strided_downscale, X<prefix stages>:<layout>
# [min_val,max_val] ops.ingest_extrema, T<stages>[c = with consts]:<layout> ops.ingest_transform, C ops.check_ingest_consts.
EXPECTED = {
    "pair_255": {
        "u8_planar u8_raw u16_planar u16_raw u8_strided u16_3d": "code nchw 1 0 255.0",
        "f32_planar f32_raw": "ingest nchw 1 0 None | D1:nchw T1:nchw",
    },
    "pair_4095": {
        "u8_planar u8_raw u16_planar u16_raw u8_strided u16_3d": "code nchw 1 0 4095.0",
        "f32_planar f32_raw": "ingest nchw 1 0 None | D1:nchw T1:nchw",
    },
    "pair_65535": {
        "u8_planar u8_raw u16_planar u16_raw u8_strided u16_3d": "code nchw 1 0 65535.0",
        "f32_planar f32_raw": "ingest nchw 1 0 None | D1:nchw T1:nchw",
    },
    "cv_pair": {
        "u8_planar u16_planar f32_planar u8_strided u16_3d": "torch nchw 1 0 None | !ValueError",
        "u8_raw u16_raw":
            ("code nhwc_bgr 1 0 255.0",
             "ingest nchw 1 0 None | D1:nhwc_bgr T1:nhwc_bgr"),
        "f32_raw": "torch nchw 1 0 None",
    },
    "sd_pair": {
        "u8_planar u8_raw u16_planar u16_raw u8_strided": "code nchw 2 0 255.0 | D2:nchw",
        "f32_planar f32_raw": "ingest nchw 2 0 None | D2:nchw T1:nchw",
        "u16_3d": "torch nchw 1 0 None",
    },
    "pair_sd": {
        "u8_planar u8_raw u16_planar u16_raw u8_strided": "code nchw 2 0 255.0 | D2:nchw",
        "f32_planar f32_raw": "ingest nchw 2 0 None | D2:nchw T1:nchw",
        "u16_3d": "torch nchw 1 0 None",
    },
    "cv_sd_pair": {
        "u8_planar u16_planar f32_planar u8_strided u16_3d": "torch nchw 1 0 None | !ValueError",
        "u8_raw u16_raw":
            ("code nhwc_bgr 2 0 255.0 | D2:nhwc_bgr",
             "ingest nchw 2 0 None | D2:nhwc_bgr T1:nhwc_bgr"),
        "f32_raw": "torch nchw 1 0 None",
    },
    "cv_pair_sd": {
        "u8_planar u16_planar f32_planar u8_strided u16_3d": "torch nchw 1 0 None | !ValueError",
        "u8_raw u16_raw":
            ("code nhwc_bgr 2 0 255.0 | D2:nhwc_bgr",
             "ingest nchw 2 0 None | D2:nhwc_bgr T1:nhwc_bgr"),
        "f32_raw": "torch nchw 1 0 None",
    },
    "black_level": {
        "u8_planar u8_raw u16_planar u16_raw f32_planar f32_raw": "ingest nchw 1 0 None | D1:nchw T1:nchw",
        "u8_strided u16_3d": "torch nchw 1 0 None",
    },
    "cv_black_level": {
        "u8_planar u16_planar f32_planar u8_strided u16_3d": "torch nchw 1 0 None | !ValueError",
        "u8_raw u16_raw": "ingest nchw 1 0 None | D1:nhwc_bgr T1:nhwc_bgr",
        "f32_raw": "torch nchw 1 0 None",
    },
    "channel_clamp": {
        "u8_planar u16_planar f32_planar": "ingest nchw 1 0 None | D1:nchw T2:nchw",
        "u8_raw u16_raw f32_raw u16_3d": "torch nchw 1 0 None | !ValueError",
        "u8_strided": "torch nchw 1 0 None",
    },
    "data_both": {
        "u8_planar u8_raw u16_planar u16_raw f32_planar f32_raw":
            "ingest_data nchw 1 0 None | X0:nchw[None,None] D1:nchw T1c:nchw C",
        "u8_strided u16_3d": "torch nchw 1 0 None",
    },
    "data_max": {
        "u8_planar u8_raw u16_planar u16_raw f32_planar f32_raw":
            "ingest_data nchw 1 0 None | X0:nchw[0,None] D1:nchw T1c:nchw C",
        "u8_strided u16_3d": "torch nchw 1 0 None",
    },
    "cv_data_both": {
        "u8_planar u16_planar f32_planar u8_strided u16_3d": "torch nchw 1 0 None | !ValueError",
        "u8_raw u16_raw": "ingest_data nchw 1 0 None | X0:nhwc_bgr[None,None] D1:nhwc_bgr T1c:nhwc_bgr C",
        "f32_raw": "torch nchw 1 0 None",
    },
    "sd_data": {
        "u8_planar u8_raw u16_planar u16_raw f32_planar f32_raw":
            "ingest_data nchw 2 1 None | D2:nchw X0:nchw[None,None] T1c:nchw C",
        "u8_strided u16_3d": "torch nchw 1 0 None",
    },
    "data_sd": {
        "u8_planar u8_raw u16_planar u16_raw f32_planar f32_raw":
            "ingest_data nchw 2 0 None | X0:nchw[None,None] D2:nchw T1c:nchw C",
        "u8_strided u16_3d": "torch nchw 1 0 None",
    },
    "two_data": {
        "u8_planar u8_raw u16_planar u16_raw f32_planar f32_raw u8_strided u16_3d": "torch nchw 1 0 None",
    },
    "float64": {
        "u8_planar u8_raw u16_planar u16_raw f32_planar f32_raw u8_strided u16_3d": "torch nchw 1 0 None",
    },
    "subclass": {
        "u8_planar u8_raw u16_planar u16_raw u8_strided u16_3d": "code nchw 1 0 255.0",
        "f32_planar f32_raw": "torch nchw 1 0 None",
    },
    "identity": {
        "u8_planar u8_raw u16_planar u16_raw f32_planar f32_raw u8_strided u16_3d": "torch nchw 1 0 None",
    },
    "empty": {
        "u8_planar u8_raw u16_planar u16_raw u8_strided u16_3d": "torch nchw 1 0 None | !TypeError",
        "f32_planar f32_raw": "torch nchw 1 0 None",
    },
}


def _cells():
    batches, lists = _batches(), _lists()
    assert set(EXPECTED) == set(lists)
    for lname, groups in EXPECTED.items():
        assert sorted(" ".join(groups).split()) == sorted(batches), lname  # the whole cross product, every batch once
        for names, want in groups.items():
            for bname in names.split():
                for planar, cell in zip((False, True), (want, want) if isinstance(want, str) else want):
                    plan, _, calls = cell.partition(" | ")
                    yield (lname, bname, planar), batches[bname], lists[lname], plan.split(), calls


def _fields(plan):
    return [plan.route, plan.layout, str(plan.step), str(int(plan.step_first)), str(plan.max_code)]


def test_plan_staging_routes():
    torch_route = ["torch", "nchw", "1", "0", "None"]
    for key, x, ts, want, _ in _cells():
        assert _fields(T.plan_staging(x.as_subclass(_OnDevice), ts, planar=key[2])) == want, key
        # a CPU "device": the classes run where the extrema would have been taken on the device
        assert _fields(T.plan_staging(x, ts, planar=key[2])) == (torch_route if want[0] == "ingest_data" else want), key
        assert not key[2] or want[1] == "nchw", key


@pytest.fixture
def calls(monkeypatch):
    """Recording stubs in place of the four ``ops`` calls of the staging."""
    seq = []

    def downscale(stack, step, layout="nchw", out=None):
        seq.append(f"D{step}:{layout}")
        return (stack[..., ::step, ::step] if layout == "nchw" else stack[:, ::step, ::step]).contiguous()

    def transform(stack, stages, layout="nchw", out=None, consts=None):
        seq.append(f"T{len(stages)}{'c' if consts is not None else ''}:{layout}")
        return torch.zeros(ops.ingest_shape(tuple(stack.shape), layout))

    def extrema(stack, prefix_stages=(), layout="nchw", min_val=None, max_val=None):
        seq.append(f"X{len(prefix_stages)}:{layout}[{min_val},{max_val}]")
        return torch.ones(4)

    monkeypatch.setattr(ops, "strided_downscale", downscale)
    monkeypatch.setattr(ops, "ingest_transform", transform)
    monkeypatch.setattr(ops, "ingest_extrema", extrema)
    monkeypatch.setattr(ops, "check_ingest_consts", lambda consts: seq.append("C"))
    return seq


def test_stage_images_issues_the_recorded_device_calls(calls):
    cpu = torch.device("cpu")
    raw = _batches()["u8_raw"].as_subclass(_OnDevice)
    out = stage_images(raw, cpu, _lists()["cv_sd_pair"], planar=True)
    assert calls == ["D2:nhwc_bgr", "T1:nhwc_bgr"]  # one downscale, one ingest: nothing is staged twice
    assert out[1] is None and out[2] == "nchw" and tuple(out[0].shape) == (2, 3, 3, 5)
    for key, x, ts, want, want_calls in _cells():
        del calls[:]
        try:
            images, max_code, layout = stage_images(x.as_subclass(_OnDevice), cpu, ts, planar=key[2])
            assert [layout, str(max_code)] == [want[1], want[4]], key
            assert images.dtype == (x.dtype if want[0] == "code" else torch.float32), key
        except (TypeError, ValueError, RuntimeError) as e:
            calls.append("!" + type(e).__name__)
        assert " ".join(calls) == want_calls, key


def test_integer_images_without_a_normalize_keep_their_message():
    with pytest.raises(TypeError, match="integer images reached the kernel without a Normalize transform; pass"):
        stage_images(_batches()["u16_planar"], torch.device("cpu"), [])
