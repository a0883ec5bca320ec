"""CPU tests: which front of clair_torch_amd.ops the streamed linearization sends a run of a ring slot's frames to, with which
slice of the slot's buffers and which keywords.  The five fronts are replaced by recorders and the slot by a stand-in of small CPU
tensors (a group of 4 frames of 3 x 4 x 6); nothing is launched.

A call is written (front, a, b, arguments): the run is frames [a:b] of the slot, and the arguments are bound to the front's own
signature with its defaults filled in, so that a keyword left out and one passed with its default value are the same call.  Tensors
are named after the slot's buffer they are a slice of ("std[1:3]"), dark pairs ("dark2", "dark_std2") after their frame.

``_DARK_RUNS`` (front and range of every run) and ``_DARK_ROWS`` (two cases with every argument) were recorded from
``_linearize_dark_runs`` before it was given ``_linearize_run``: ``test_dark_runs`` passes against that version and this one.  The
rows of ``_plain_rows`` are written out by hand from the branch that stood inline in ``_pipelined`` at that commit
(inference/linearization.py:327-341: strided, ingest with or without per-frame constants, else ``linearize_frames``), which could not
be called on its own."""
import inspect
from types import SimpleNamespace

import pytest
import torch

from clair_torch_amd import ops
from clair_torch_amd.inference import linearization

FRONTS = ("linearize_frames", "linearize_ingest_frames", "linearize_ingest_frames_strided", "linearize_dark_frames",
          "linearize_dark_ingest_frames")
SIGNATURES = {name: inspect.signature(getattr(ops, name)) for name in FRONTS}
GROUP, CHW = 4, (3, 4, 6)
STAGES = (("affine", 64.0, 1000.0, 1.0, 0.0),)
M = "matched"
PATTERNS = {"all": [M, M, M, M], "none": [None] * 4, "ends": [M, None, None, M], "second": [None, M]}


def _slot(frame_shape=CHW, dtype=torch.uint16):
    return SimpleNamespace(frames=torch.zeros((GROUP,) + frame_shape, dtype=dtype), std=torch.zeros((GROUP,) + CHW),
                           lin_out=torch.zeros((GROUP,) + CHW), std_out=torch.zeros((GROUP,) + CHW),
                           consts=torch.zeros((GROUP, 4)))


class Recorder:
    def __init__(self, monkeypatch, slot, named):
        self.slot, self.named, self.calls = slot, named, []
        for front in FRONTS:
            monkeypatch.setattr(ops, front, self._front(front))

    def _plain(self, v):
        if isinstance(v, torch.Tensor):
            for name, t in self.named.items():
                if v is t:
                    return name
            for name, buf in vars(self.slot).items():
                if v.untyped_storage().data_ptr() == buf.untyped_storage().data_ptr():
                    a = v.storage_offset() // buf[0].numel()
                    assert tuple(v.shape[1:]) == tuple(buf.shape[1:]) and v.is_contiguous()
                    return f"{name}[{a}:{a + v.shape[0]}]"
            raise AssertionError("a tensor that is neither the slot's nor a named one")
        if isinstance(v, (list, tuple)) and any(isinstance(e, torch.Tensor) for e in v):
            return [self._plain(e) for e in v]
        return v

    def _front(self, front):
        def call(*args, **kw):
            bound = SIGNATURES[front].bind(*args, **kw)
            bound.apply_defaults()
            frames = self._plain(bound.arguments.pop("frames"))
            a, b = (int(n) for n in frames[len("frames["):-1].split(":"))
            self.calls.append((front, a, b, {k: self._plain(v) for k, v in bound.arguments.items()}))
            return bound.arguments["out"]
        return call


def _row(front, a, b, *args, **kw):
    """The call ``front(frames[a:b], *args, **kw)`` as the recorder writes it."""
    bound = SIGNATURES[front].bind("frames", *args, **kw)
    bound.apply_defaults()
    del bound.arguments["frames"]
    return front, a, b, {k: list(v) if k in ("out", "darks", "dark_stds") else v for k, v in bound.arguments.items()}


def _out(a, b):
    return f"lin_out[{a}:{b}]", f"std_out[{a}:{b}]"


def _pairs(pattern, named):
    pairs = []
    for i, m in enumerate(pattern):
        if m is not None:
            named[f"dark{i}"], named[f"dark_std{i}"] = torch.zeros(CHW), torch.zeros(CHW)
        pairs.append(None if m is None else (named[f"dark{i}"], named[f"dark_std{i}"]))
    return pairs


# ---- a dark pipeline: (route, pair pattern) -> the runs of _linearize_dark_runs, recorded
def _dark(a, b):
    return dict(darks=[f"dark{i}" for i in range(a, b)], dark_stds=[f"dark_std{i}" for i in range(a, b)])


def _dark_row(front, a, b, with_std):
    """The call of ``front`` on frames [a:b] of a dark pipeline with all its arguments."""
    kw = dict(std=f"std[{a}:{b}]" if with_std else None, std_mode="explicit" if with_std else "multiplier", std_value=0.0 if with_std else 0.5,
              out=_out(a, b))
    if front == "linearize_frames":
        return _row(front, a, b, "lut", "catmull", max_code=4095.0, want_std=True, **kw)
    if front == "linearize_dark_frames":
        return _row(front, a, b, *_dark(a, b).values(), "lut", "catmull", max_code=4095.0, **kw)
    if front == "linearize_ingest_frames":
        return _row(front, a, b, STAGES, "lut", "catmull", want_std=True, layout="nhwc_bgr", **kw)
    return _row(front, a, b, STAGES, *_dark(a, b).values(), "lut", "catmull", layout="nhwc_bgr", **kw)


_DARK_RUNS = {
    ("code", "all"): [("linearize_dark_frames", 0, 4)],
    ("code", "none"): [("linearize_frames", 0, 4)],
    ("code", "ends"): [("linearize_dark_frames", 0, 1), ("linearize_frames", 1, 3), ("linearize_dark_frames", 3, 4)],
    ("code", "second"): [("linearize_frames", 0, 1), ("linearize_dark_frames", 1, 2)],
    ("chain", "all"): [("linearize_dark_ingest_frames", 0, 4)],
    ("chain", "none"): [("linearize_ingest_frames", 0, 4)],
    ("chain", "ends"): [("linearize_dark_ingest_frames", 0, 1), ("linearize_ingest_frames", 1, 3), ("linearize_dark_ingest_frames", 3, 4)],
    ("chain", "second"): [("linearize_ingest_frames", 0, 1), ("linearize_dark_ingest_frames", 1, 2)],
}
# two of them with every argument written out, as the recorder saw them
_DARK_ROWS = {
    ("code", "ends", False): [
        ("linearize_dark_frames", 0, 1, dict(darks=["dark0"], dark_stds=["dark_std0"], lut="lut", interp="catmull", std=None, std_mode="multiplier",
                                             std_value=0.5, max_code=4095.0, threshold=0.05, alpha=50.0, out=["lin_out[0:1]", "std_out[0:1]"])),
        ("linearize_frames", 1, 3, dict(lut="lut", interp="catmull", std=None, std_mode="multiplier", std_value=0.5, max_code=4095.0, want_std=True,
                                        tile=None, layout="nchw", out=["lin_out[1:3]", "std_out[1:3]"])),
        ("linearize_dark_frames", 3, 4, dict(darks=["dark3"], dark_stds=["dark_std3"], lut="lut", interp="catmull", std=None, std_mode="multiplier",
                                             std_value=0.5, max_code=4095.0, threshold=0.05, alpha=50.0, out=["lin_out[3:4]", "std_out[3:4]"]))],
    ("chain", "ends", True): [
        ("linearize_dark_ingest_frames", 0, 1, dict(stages=STAGES, darks=["dark0"], dark_stds=["dark_std0"], lut="lut", interp="catmull",
                                                    std="std[0:1]", std_mode="explicit", std_value=0.0, layout="nhwc_bgr",
                                                    out=["lin_out[0:1]", "std_out[0:1]"], threshold=0.05, alpha=50.0)),
        ("linearize_ingest_frames", 1, 3, dict(stages=STAGES, lut="lut", interp="catmull", std="std[1:3]", std_mode="explicit", std_value=0.0,
                                               want_std=True, tile=None, layout="nhwc_bgr", out=["lin_out[1:3]", "std_out[1:3]"], consts=None)),
        ("linearize_dark_ingest_frames", 3, 4, dict(stages=STAGES, darks=["dark3"], dark_stds=["dark_std3"], lut="lut", interp="catmull",
                                                    std="std[3:4]", std_mode="explicit", std_value=0.0, layout="nhwc_bgr",
                                                    out=["lin_out[3:4]", "std_out[3:4]"], threshold=0.05, alpha=50.0))],
}


def _dark_runs(monkeypatch, route, pattern, with_std):
    slot = _slot(CHW if route == "code" else (4, 6, 3))
    named = dict(lut=torch.zeros(3, 16))
    pairs = _pairs(PATTERNS[pattern], named)
    rec = Recorder(monkeypatch, slot, named)
    std_mode, std_value = ("explicit", 0.0) if with_std else ("multiplier", 0.5)
    back = linearization._linearize_dark_runs(slot, len(pairs), pairs, with_std, named["lut"], "catmull", std_mode, std_value, 4095.0,
                                              None if route == "code" else (STAGES, "nhwc_bgr"))
    assert [rec._plain(v) for v in back] == list(_out(0, len(pairs)))
    return rec.calls


@pytest.mark.parametrize("with_std", (False, True))
@pytest.mark.parametrize("pattern", list(PATTERNS))
@pytest.mark.parametrize("route", ("code", "chain"))
def test_dark_runs(monkeypatch, route, pattern, with_std):
    calls = _dark_runs(monkeypatch, route, pattern, with_std)
    assert calls == [_dark_row(front, a, b, with_std) for front, a, b in _DARK_RUNS[(route, pattern)]]
    if (route, pattern, with_std) in _DARK_ROWS:
        assert calls == _DARK_ROWS[(route, pattern, with_std)]


# ---- no dark field: the single run [0:k] of _pipelined, by hand from the inline branch at linearization.py:327-341 of the parent
def _plain_rows(case, with_std, k):
    std_kw = dict(std=f"std[0:{k}]" if with_std else None, std_mode="explicit" if with_std else "constant", std_value=0.0 if with_std else 0.01)
    if case == "code pair":                # :339-341
        return [_row("linearize_frames", 0, k, "lut", "linear", max_code=4095.0, want_std=True, layout="nhwc_bgr", out=_out(0, k), **std_kw)]
    args = dict(want_std=True, layout="nhwc_bgr", out=_out(0, k), consts=f"consts[0:{k}]" if case == "ingest with constants" else None, **std_kw)   # :332-333
    if case == "step 2":                   # :334-335
        return [_row("linearize_ingest_frames_strided", 0, k, 2, STAGES, "lut", "linear", **args)]
    return [_row("linearize_ingest_frames", 0, k, STAGES, "lut", "linear", **args)]      # :337


@pytest.mark.parametrize("k", (4, 3))
@pytest.mark.parametrize("with_std", (False, True))
@pytest.mark.parametrize("case", ("code pair", "ingest chain", "ingest with constants", "step 2"))
def test_run_without_a_dark_field(monkeypatch, case, with_std, k):
    slot = _slot((4, 6, 3))
    named = dict(lut=torch.zeros(3, 16))
    rec = Recorder(monkeypatch, slot, named)
    std_mode, std_value = ("explicit", 0.0) if with_std else ("constant", 0.01)
    back = linearization._linearize_run(slot, 0, k, with_std, named["lut"], "linear", std_mode, std_value, 4095.0,
                                        stages=None if case == "code pair" else STAGES, layout="nhwc_bgr", step=2 if case == "step 2" else 1,
                                        consts=slot.consts[:k] if case == "ingest with constants" else None)
    assert [rec._plain(v) for v in back] == list(_out(0, k))
    assert rec.calls == _plain_rows(case, with_std, k)


def test_an_unmatched_run_is_the_run_without_a_dark_field(monkeypatch):
    """An unmatched run of a dark pipeline makes the calls a group without a dark field makes with no constants and step 1."""
    for route in ("code", "chain"):
        unmatched = _dark_runs(monkeypatch, route, "none", True)
        slot = _slot(CHW if route == "code" else (4, 6, 3))
        named = dict(lut=torch.zeros(3, 16))
        rec = Recorder(monkeypatch, slot, named)
        linearization._linearize_run(slot, 0, 4, True, named["lut"], "catmull", "explicit", 0.0, 4095.0,
                                     **({} if route == "code" else dict(stages=STAGES, layout="nhwc_bgr")))
        assert rec.calls == unmatched
