"""CPU tests: what the seven HDR-merge fronts of clair_torch_amd.ops hand to the library.  ``nv.load()`` is replaced by an object
whose ``ct_hdr_merge_*`` attributes record their arguments and answer with a scripted status; ``ops._require_device``,
``ops._stream`` and ``torch.cuda.device`` are patched here so that CPU tensors go through.  Nothing is launched.

Two records, both taken from ops.py before the fronts were given one shared launch tail -- they are the contract:
``_ARGUMENTS`` (below) is every argument of one call per front and list length, pointers named after the tensor passed in;
``_CALLS`` is, for every front under every status script ([OK], [ERR_UNSUPPORTED, OK], [ERR_UNSUPPORTED]: "ok", "no, ok", "no") and
keyword combination, the entry points called, the flag word and state pointers of each call, ``state.batches`` afterwards and what
comes back."""
import contextlib
import ctypes
import itertools

import pytest
import torch

from clair_torch_amd import _native as nv
from clair_torch_amd import ops

CPU = torch.device("cpu")
OK, UNSUPPORTED = 0, nv.ERR_UNSUPPORTED
AFF = ("affine", 64.0, 1000.0, 1.0, 0.0)
DATA = ("affine_data", 1.0, 0.0)
FRAMES = 2      # per batch
ENTRY_POINTS = ("ct_hdr_merge_batch", "ct_hdr_merge_batches", "ct_hdr_merge_dark_batch", "ct_hdr_merge_dark_batches",
                "ct_hdr_merge_ingest_batch", "ct_hdr_merge_ingest_batches", "ct_hdr_merge_dark_ingest_batches")
FRONTS = ("hdr_merge_batch", "hdr_merge_batches", "hdr_merge_dark_batch", "hdr_merge_dark_batches", "hdr_merge_ingest_batch",
          "hdr_merge_ingest_batches", "hdr_merge_dark_ingest_batches")
LIST_FRONTS = tuple(f for f in FRONTS if f.endswith("batches"))
HAS_FIRST = ("hdr_merge_dark_batches", "hdr_merge_dark_ingest_batches")


class Library:
    """Stands for the loaded library: every ct_hdr_merge_* entry point records (name, arguments as plain values) and returns the
    next status of ``script`` (the last one again once the script is used up)."""

    def __init__(self, script, names):
        self.script, self.names, self.calls = list(script), names, []
        for entry in ENTRY_POINTS:
            setattr(self, entry, self._recorder(entry))

    @staticmethod
    def ct_error_string(rc):
        return f"status {rc}".encode()

    def _plain(self, a):
        if a is None or isinstance(a, (int, float)):
            return a
        if isinstance(a, ctypes.c_void_p):
            return None if a.value is None else self.names.get(a.value, "buffer")
        if isinstance(a, ctypes.Array) and a._type_ is ctypes.c_void_p:
            return [None if v is None else self.names.get(v, "buffer") for v in a]
        if isinstance(a, ctypes.Array) and a._type_ is ctypes.c_int32:
            return list(a)
        if isinstance(a, ctypes.Array):
            return f"{a._type_.__name__}[{len(a)}]"
        return "&"      # ctypes.byref(...)

    def _recorder(self, entry):
        def call(*args):
            plain = [self._plain(a) for a in args]
            sizes = next((list(a) for a in args if isinstance(a, ctypes.Array) and a._type_ is ctypes.c_int32), [FRAMES])
            # the exposure times stand ten from the end in every entry point, in front of the model; read back from the pointer
            exposures = list((ctypes.c_double * sum(sizes)).from_address(args[-10].value))
            self.calls.append(dict(entry=entry, args=plain, sizes=sizes, exposures=exposures))
            return self.script.pop(0) if len(self.script) > 1 else self.script[0]
        return call


def _inputs(k):
    """k batches of 2 x 3 x 4 x 6 uint16 frames with everything a front can take beside them, and the names of their pointers."""
    t = dict(
        frames=[torch.zeros((2, 3, 4, 6), dtype=torch.uint16) for _ in range(k)],
        exposures=[torch.tensor([0.5 + i, 2.0 + i]) for i in range(k)],
        darks=[torch.zeros((2, 3, 4, 6)) for _ in range(k)],
        dark_stds=[torch.zeros((2, 3, 4, 6)) for _ in range(k)],
        stds=[torch.zeros((2, 3, 4, 6)) for _ in range(k)],
        halos=[torch.zeros((2, 3, 2, 6), dtype=torch.uint16) for _ in range(k)],
        consts=[torch.zeros(4) for _ in range(k)],
        lut=[torch.linspace(0.0, 1.0, 16).repeat(3, 1)])
    names = {v.data_ptr(): f"{name}[{i}]" for name, values in t.items() for i, v in enumerate(values)}
    assert len(names) == sum(len(v) for v in t.values())
    return t, names


def _call(front, t, k, rich, **kw):
    """``front`` on the first k batches of ``t``; ``rich``: with explicit stds, halo rows and constants where it takes them."""
    one = not front.endswith("batches")
    pick = (lambda name: t[name][0]) if one else (lambda name: t[name][:k])
    kw.setdefault("lut", t["lut"][0])
    if rich:
        kw["std" if one else "stds"] = pick("stds")
    elif "dark" not in front:
        kw.update(std_mode="constant", std_value=0.05)
    if "ingest" in front:
        if rich:
            kw["consts"] = pick("consts")
        positional = (pick("frames"), [AFF, DATA] if rich else [AFF], pick("exposures"))
    else:
        positional = (pick("frames"), pick("exposures"))
    if "dark" in front:
        positional += (pick("darks"), pick("dark_stds"))
        if rich:
            kw["halo" if one else "halos"] = pick("halos")
            kw["tile"] = ops.TileGeometry(h_global=12, row_offset=4)
    return getattr(ops, front)(*positional, **kw)


@pytest.fixture()
def through(monkeypatch):
    """-> run(front, script, k, rich, state, **keywords) = (the recorded calls, state.batches afterwards | None, what came back)."""
    monkeypatch.setattr(ops, "_require_device", lambda t, name: None)
    monkeypatch.setattr(ops, "_stream", lambda device: None)
    monkeypatch.setattr(torch.cuda, "device", lambda device: contextlib.nullcontext())

    def run(front, script, k=1, rich=False, state="none", **kw):
        t, names = _inputs(k)
        lib = Library(script, names)
        monkeypatch.setattr(ops.nv, "load", lambda: lib)
        st = None
        if state != "none":
            st = ops.MergeState((3, 4, 6), CPU, True)
            st.batches = 0 if state == "fresh" else 2
            names.update({st.mean.data_ptr(): "state.mean", st.sumw.data_ptr(): "state.sumw", st.var.data_ptr(): "state.var"})
        try:
            out = _call(front, t, k, rich, state=st, **kw)
            back = "none" if out is None else "pair" if (isinstance(out, tuple) and len(out) == 2) else repr(out)
            if out is not None:
                assert tuple(out[0].shape) == (3, 4, 6) and out[0].dtype == torch.float64
                assert out[1] is not None and tuple(out[1].shape) == (3, 4, 6) and out[1].dtype == torch.float32
        except Exception as e:    # noqa: BLE001 -- the type and the message are what is recorded
            back = f"{type(e).__name__}: {e}"
        return lib.calls, (None if st is None else st.batches), back

    return run


# ---- every argument of one call per front -------------------------------------------------------------------------------------------
# case: (entry point after "ct_hdr_merge_", its arguments in the order include/clair_hip.h declares them, the exposure times read back).
# "&": a struct by reference; "buffer": memory the front made itself (the outputs, the staged exposure times); None: a NULL pointer.
# The flag word 3 is FIRST_BATCH | FINALIZE; every call returned (mean, std).
_ARGUMENTS = {
    'hdr_merge_batch/k1/plain':
        ('batch', ['frames[0]', 1, 65535.0, 2, '&', None, 1, 0.05, 'buffer', '&', 1, None, None, None, 'buffer', 'buffer', 3, None], [0.5,
        2.0]),
    'hdr_merge_batch/k1/rich':
        ('batch', ['frames[0]', 1, 65535.0, 2, '&', 'stds[0]', 3, 0.0, 'buffer', '&', 1, None, None, None, 'buffer', 'buffer', 3, None],
        [0.5, 2.0]),
    'hdr_merge_batches/k1/plain':
        ('batch', ['frames[0]', 1, 65535.0, 2, '&', None, 1, 0.05, 'buffer', '&', 1, None, None, None, 'buffer', 'buffer', 3, None], [0.5,
        2.0]),
    'hdr_merge_batches/k1/rich':
        ('batch', ['frames[0]', 1, 65535.0, 2, '&', 'stds[0]', 3, 0.0, 'buffer', '&', 1, None, None, None, 'buffer', 'buffer', 3, None],
        [0.5, 2.0]),
    'hdr_merge_batches/k3/plain':
        ('batches', [['frames[0]', 'frames[1]', 'frames[2]'], None, [2, 2, 2], 3, 1, 65535.0, '&', 1, 0.05, 'buffer', '&', 1, 'buffer',
        'buffer', 'buffer', 'buffer', 'buffer', 3, None], [0.5, 2.0, 1.5, 3.0, 2.5, 4.0]),
    'hdr_merge_batches/k3/rich':
        ('batches', [['frames[0]', 'frames[1]', 'frames[2]'], ['stds[0]', 'stds[1]', 'stds[2]'], [2, 2, 2], 3, 1, 65535.0, '&', 3, 0.0,
        'buffer', '&', 1, 'buffer', 'buffer', 'buffer', 'buffer', 'buffer', 3, None], [0.5, 2.0, 1.5, 3.0, 2.5, 4.0]),
    'hdr_merge_dark_batch/k1/plain':
        ('dark_batch', ['frames[0]', 1, 65535.0, 2, '&', None, None, 0, 0.0, 'darks[0]', 'dark_stds[0]', 2, 0.05, 50.0, 'buffer', '&', 1,
        None, None, None, 'buffer', 'buffer', 3, None], [0.5, 2.0]),
    'hdr_merge_dark_batch/k1/rich':
        ('dark_batch', ['frames[0]', 1, 65535.0, 2, '&', 'halos[0]', 'stds[0]', 3, 0.0, 'darks[0]', 'dark_stds[0]', 2, 0.05, 50.0, 'buffer',
        '&', 1, None, None, None, 'buffer', 'buffer', 3, None], [0.5, 2.0]),
    'hdr_merge_dark_batches/k1/plain':
        ('dark_batch', ['frames[0]', 1, 65535.0, 2, '&', None, None, 0, 0.0, 'darks[0]', 'dark_stds[0]', 2, 0.05, 50.0, 'buffer', '&', 1,
        None, None, None, 'buffer', 'buffer', 3, None], [0.5, 2.0]),
    'hdr_merge_dark_batches/k1/rich':
        ('dark_batch', ['frames[0]', 1, 65535.0, 2, '&', 'halos[0]', 'stds[0]', 3, 0.0, 'darks[0]', 'dark_stds[0]', 2, 0.05, 50.0, 'buffer',
        '&', 1, None, None, None, 'buffer', 'buffer', 3, None], [0.5, 2.0]),
    'hdr_merge_dark_batches/k3/plain':
        ('dark_batches', [['frames[0]', 'frames[1]', 'frames[2]'], [2, 2, 2], 3, 1, 65535.0, '&', [None, None, None], None, 0, 0.0,
        ['darks[0]', 'darks[1]', 'darks[2]'], ['dark_stds[0]', 'dark_stds[1]', 'dark_stds[2]'], [2, 2, 2], 0.05, 50.0, 'buffer', '&', 1,
        None, None, None, 'buffer', 'buffer', 3, None], [0.5, 2.0, 1.5, 3.0, 2.5, 4.0]),
    'hdr_merge_dark_batches/k3/rich':
        ('dark_batches', [['frames[0]', 'frames[1]', 'frames[2]'], [2, 2, 2], 3, 1, 65535.0, '&', ['halos[0]', 'halos[1]', 'halos[2]'],
        ['stds[0]', 'stds[1]', 'stds[2]'], 3, 0.0, ['darks[0]', 'darks[1]', 'darks[2]'], ['dark_stds[0]', 'dark_stds[1]', 'dark_stds[2]'],
        [2, 2, 2], 0.05, 50.0, 'buffer', '&', 1, None, None, None, 'buffer', 'buffer', 3, None], [0.5, 2.0, 1.5, 3.0, 2.5, 4.0]),
    'hdr_merge_ingest_batch/k1/plain':
        ('ingest_batch', ['frames[0]', 1, 2, '&', 'IngestStage[1]', 1, None, None, 1, 0.05, 'buffer', '&', 1, None, None, None, 'buffer',
        'buffer', 3, None], [0.5, 2.0]),
    'hdr_merge_ingest_batch/k1/rich':
        ('ingest_batch', ['frames[0]', 1, 2, '&', 'IngestStage[2]', 2, 'consts[0]', 'stds[0]', 3, 0.0, 'buffer', '&', 1, None, None, None,
        'buffer', 'buffer', 3, None], [0.5, 2.0]),
    'hdr_merge_ingest_batches/k1/plain':
        ('ingest_batch', ['frames[0]', 1, 2, '&', 'IngestStage[1]', 1, None, None, 1, 0.05, 'buffer', '&', 1, None, None, None, 'buffer',
        'buffer', 3, None], [0.5, 2.0]),
    'hdr_merge_ingest_batches/k1/rich':
        ('ingest_batch', ['frames[0]', 1, 2, '&', 'IngestStage[2]', 2, 'consts[0]', 'stds[0]', 3, 0.0, 'buffer', '&', 1, None, None, None,
        'buffer', 'buffer', 3, None], [0.5, 2.0]),
    'hdr_merge_ingest_batches/k3/plain':
        ('ingest_batches', [['frames[0]', 'frames[1]', 'frames[2]'], [2, 2, 2], 3, 1, '&', 'IngestStage[1]', 1, None, None, 1, 0.05,
        'buffer', '&', 1, None, None, None, 'buffer', 'buffer', 131, None], [0.5, 2.0, 1.5, 3.0, 2.5, 4.0]),
    'hdr_merge_ingest_batches/k3/rich':
        ('ingest_batches', [['frames[0]', 'frames[1]', 'frames[2]'], [2, 2, 2], 3, 1, '&', 'IngestStage[2]', 2, ['consts[0]', 'consts[1]',
        'consts[2]'], ['stds[0]', 'stds[1]', 'stds[2]'], 3, 0.0, 'buffer', '&', 1, None, None, None, 'buffer', 'buffer', 131, None], [0.5,
        2.0, 1.5, 3.0, 2.5, 4.0]),
    'hdr_merge_dark_ingest_batches/k1/plain':
        ('dark_ingest_batches', [['frames[0]'], [2], 1, 1, '&', 'IngestStage[1]', 1, None, [None], None, 0, 0.0, ['darks[0]'],
        ['dark_stds[0]'], [2], 0.05, 50.0, 'buffer', '&', 1, None, None, None, 'buffer', 'buffer', 3, None], [0.5, 2.0]),
    'hdr_merge_dark_ingest_batches/k1/rich':
        ('dark_ingest_batches', [['frames[0]'], [2], 1, 1, '&', 'IngestStage[2]', 2, ['consts[0]'], ['halos[0]'], ['stds[0]'], 3, 0.0,
        ['darks[0]'], ['dark_stds[0]'], [2], 0.05, 50.0, 'buffer', '&', 1, None, None, None, 'buffer', 'buffer', 3, None], [0.5, 2.0]),
    'hdr_merge_dark_ingest_batches/k3/plain':
        ('dark_ingest_batches', [['frames[0]', 'frames[1]', 'frames[2]'], [2, 2, 2], 3, 1, '&', 'IngestStage[1]', 1, None, [None, None,
        None], None, 0, 0.0, ['darks[0]', 'darks[1]', 'darks[2]'], ['dark_stds[0]', 'dark_stds[1]', 'dark_stds[2]'], [2, 2, 2], 0.05, 50.0,
        'buffer', '&', 1, None, None, None, 'buffer', 'buffer', 3, None], [0.5, 2.0, 1.5, 3.0, 2.5, 4.0]),
    'hdr_merge_dark_ingest_batches/k3/rich':
        ('dark_ingest_batches', [['frames[0]', 'frames[1]', 'frames[2]'], [2, 2, 2], 3, 1, '&', 'IngestStage[2]', 2, ['consts[0]',
        'consts[1]', 'consts[2]'], ['halos[0]', 'halos[1]', 'halos[2]'], ['stds[0]', 'stds[1]', 'stds[2]'], 3, 0.0, ['darks[0]', 'darks[1]',
        'darks[2]'], ['dark_stds[0]', 'dark_stds[1]', 'dark_stds[2]'], [2, 2, 2], 0.05, 50.0, 'buffer', '&', 1, None, None, None, 'buffer',
        'buffer', 3, None], [0.5, 2.0, 1.5, 3.0, 2.5, 4.0]),
}


def _argument_cases():
    for front in FRONTS:
        for k in ((1, 3) if front in LIST_FRONTS else (1,)):
            for rich in (False, True):
                yield f"{front}/k{k}/{'rich' if rich else 'plain'}", front, k, rich


@pytest.mark.parametrize("case,front,k,rich", list(_argument_cases()), ids=[c[0] for c in _argument_cases()])
def test_arguments_that_reach_the_library(through, case, front, k, rich):
    calls, _, back = through(front, [OK], k=k, rich=rich)
    assert back == "pair" and len(calls) == 1
    assert (calls[0]["entry"][len("ct_hdr_merge_"):], calls[0]["args"], calls[0]["exposures"]) == _ARGUMENTS[case]


# ---- flag words, state pointers, retries and what comes back, under every status script ----------------------------------------------
SCRIPTS = {"ok": [OK], "no, ok": [UNSUPPORTED, OK], "no": [UNSUPPORTED]}
REFERENCE_ORDER_BITS = {None: 0, True: nv.MERGE_REFERENCE_ORDER, False: nv.MERGE_CLOSED_FORM}
# (front after "hdr_merge_", script, k, finalize, require_one_launch, first): what happened without a state, with a fresh MergeState
# and with one that holds two batches, each as "<calls> > <what came back> <state.batches afterwards>".  A call is
# "<entry point after ct_hdr_merge_, = for the front's own>/<flag word>/<state pointers>": "-" NULL, "s" the caller's MergeState, "f"
# a fresh one the front made.  Came back: the pair, none, "refused" (NativeLibraryError naming the entry point called last), or
# "no state: <what>" (ValueError before any call).  Recorded with reference_order=None; True and False only add their flag bit to
# every call (asserted for all three).
_CALLS = {
    ('batch', 'ok', 1, True, None, None): ('=/3/--- > pair', '=/3/sss > pair 1', '=/2/sss > pair 3'),
    ('batch', 'ok', 1, False, None, None): ('> no state: needs', '=/1/sss > none 1', '=/0/sss > none 3'),
    ('batch', 'no, ok', 1, True, None, None): ('=/3/--- > refused', '=/3/sss > refused 0', '=/2/sss > refused 2'),
    ('batch', 'no, ok', 1, False, None, None): ('> no state: needs', '=/1/sss > refused 0', '=/0/sss > refused 2'),
    ('batch', 'no', 1, True, None, None): ('=/3/--- > refused', '=/3/sss > refused 0', '=/2/sss > refused 2'),
    ('batch', 'no', 1, False, None, None): ('> no state: needs', '=/1/sss > refused 0', '=/0/sss > refused 2'),
    ('batches', 'ok', 1, True, False, None): ('batch/3/--- > pair', 'batch/3/sss > pair 1', 'batch/2/sss > pair 3'),
    ('batches', 'ok', 1, True, True, None): ('batch/3/--- > pair', 'batch/3/sss > pair 1', 'batch/2/sss > pair 3'),
    ('batches', 'ok', 1, False, False, None): ('> no state: needs', 'batch/1/sss > none 1', 'batch/0/sss > none 3'),
    ('batches', 'ok', 1, False, True, None): ('> no state: needs', 'batch/1/sss > none 1', 'batch/0/sss > none 3'),
    ('batches', 'ok', 3, True, False, None): ('=/3/fff > pair', '=/3/sss > pair 3', '=/2/sss > pair 5'),
    ('batches', 'ok', 3, True, True, None): ('=/131/fff > pair', '=/131/sss > pair 3', '=/130/sss > pair 5'),
    ('batches', 'ok', 3, False, False, None): ('> no state: needs', '=/1/sss > none 3', '=/0/sss > none 5'),
    ('batches', 'ok', 3, False, True, None): ('> no state: needs', '=/129/sss > none 3', '=/128/sss > none 5'),
    ('batches', 'no, ok', 1, True, False, None): ('batch/3/--- > refused', 'batch/3/sss > refused 0', 'batch/2/sss > refused 2'),
    ('batches', 'no, ok', 1, True, True, None): ('batch/3/--- > refused', 'batch/3/sss > refused 0', 'batch/2/sss > refused 2'),
    ('batches', 'no, ok', 1, False, False, None): ('> no state: needs', 'batch/1/sss > refused 0', 'batch/0/sss > refused 2'),
    ('batches', 'no, ok', 1, False, True, None): ('> no state: needs', 'batch/1/sss > refused 0', 'batch/0/sss > refused 2'),
    ('batches', 'no, ok', 3, True, False, None): ('=/3/fff > refused', '=/3/sss > refused 0', '=/2/sss > refused 2'),
    ('batches', 'no, ok', 3, True, True, None): ('=/131/fff > refused', '=/131/sss > refused 0', '=/130/sss > refused 2'),
    ('batches', 'no, ok', 3, False, False, None): ('> no state: needs', '=/1/sss > refused 0', '=/0/sss > refused 2'),
    ('batches', 'no, ok', 3, False, True, None): ('> no state: needs', '=/129/sss > refused 0', '=/128/sss > refused 2'),
    ('batches', 'no', 1, True, False, None): ('batch/3/--- > refused', 'batch/3/sss > refused 0', 'batch/2/sss > refused 2'),
    ('batches', 'no', 1, True, True, None): ('batch/3/--- > refused', 'batch/3/sss > refused 0', 'batch/2/sss > refused 2'),
    ('batches', 'no', 1, False, False, None): ('> no state: needs', 'batch/1/sss > refused 0', 'batch/0/sss > refused 2'),
    ('batches', 'no', 1, False, True, None): ('> no state: needs', 'batch/1/sss > refused 0', 'batch/0/sss > refused 2'),
    ('batches', 'no', 3, True, False, None): ('=/3/fff > refused', '=/3/sss > refused 0', '=/2/sss > refused 2'),
    ('batches', 'no', 3, True, True, None): ('=/131/fff > refused', '=/131/sss > refused 0', '=/130/sss > refused 2'),
    ('batches', 'no', 3, False, False, None): ('> no state: needs', '=/1/sss > refused 0', '=/0/sss > refused 2'),
    ('batches', 'no', 3, False, True, None): ('> no state: needs', '=/129/sss > refused 0', '=/128/sss > refused 2'),
    ('dark_batch', 'ok', 1, True, None, None): ('=/3/--- > pair', '=/3/sss > pair 1', '=/2/sss > pair 3'),
    ('dark_batch', 'ok', 1, False, None, None): ('> no state: needs', '=/1/sss > none 1', '=/0/sss > none 3'),
    ('dark_batch', 'no, ok', 1, True, None, None): ('=/3/--- > refused', '=/3/sss > refused 0', '=/2/sss > refused 2'),
    ('dark_batch', 'no, ok', 1, False, None, None): ('> no state: needs', '=/1/sss > refused 0', '=/0/sss > refused 2'),
    ('dark_batch', 'no', 1, True, None, None): ('=/3/--- > refused', '=/3/sss > refused 0', '=/2/sss > refused 2'),
    ('dark_batch', 'no', 1, False, None, None): ('> no state: needs', '=/1/sss > refused 0', '=/0/sss > refused 2'),
    ('dark_batches', 'ok', 1, True, False, None): ('dark_batch/3/--- > pair', 'dark_batch/3/sss > pair 1', 'dark_batch/2/sss > pair 3'),
    ('dark_batches', 'ok', 1, True, False, True): ('=/3/--- > pair', '=/3/sss > pair 1', '=/3/sss > pair 3'),
    ('dark_batches', 'ok', 1, True, False, False): ('=/2/--- > pair', '=/2/sss > pair 1', '=/2/sss > pair 3'),
    ('dark_batches', 'ok', 1, True, True, None): ('dark_batch/3/--- > pair', 'dark_batch/3/sss > pair 1', 'dark_batch/2/sss > pair 3'),
    ('dark_batches', 'ok', 1, True, True, True): ('=/131/--- > pair', '=/131/sss > pair 1', '=/131/sss > pair 3'),
    ('dark_batches', 'ok', 1, True, True, False): ('=/130/--- > pair', '=/130/sss > pair 1', '=/130/sss > pair 3'),
    ('dark_batches', 'ok', 1, False, False, None): ('> no state: needs', 'dark_batch/1/sss > none 1', 'dark_batch/0/sss > none 3'),
    ('dark_batches', 'ok', 1, False, False, True): ('> no state: needs', '=/1/sss > none 1', '=/1/sss > none 3'),
    ('dark_batches', 'ok', 1, False, False, False): ('> no state: needs', '=/0/sss > none 1', '=/0/sss > none 3'),
    ('dark_batches', 'ok', 1, False, True, None): ('> no state: needs', 'dark_batch/1/sss > none 1', 'dark_batch/0/sss > none 3'),
    ('dark_batches', 'ok', 1, False, True, True): ('> no state: needs', '=/129/sss > none 1', '=/129/sss > none 3'),
    ('dark_batches', 'ok', 1, False, True, False): ('> no state: needs', '=/128/sss > none 1', '=/128/sss > none 3'),
    ('dark_batches', 'ok', 3, True, False, None): ('=/3/--- > pair', '=/3/sss > pair 3', '=/2/sss > pair 5'),
    ('dark_batches', 'ok', 3, True, False, True): ('=/3/--- > pair', '=/3/sss > pair 3', '=/3/sss > pair 5'),
    ('dark_batches', 'ok', 3, True, False, False): ('=/2/--- > pair', '=/2/sss > pair 3', '=/2/sss > pair 5'),
    ('dark_batches', 'ok', 3, True, True, None): ('=/131/--- > pair', '=/131/sss > pair 3', '=/130/sss > pair 5'),
    ('dark_batches', 'ok', 3, True, True, True): ('=/131/--- > pair', '=/131/sss > pair 3', '=/131/sss > pair 5'),
    ('dark_batches', 'ok', 3, True, True, False): ('=/130/--- > pair', '=/130/sss > pair 3', '=/130/sss > pair 5'),
    ('dark_batches', 'ok', 3, False, False, None): ('> no state: needs', '=/1/sss > none 3', '=/0/sss > none 5'),
    ('dark_batches', 'ok', 3, False, False, True): ('> no state: needs', '=/1/sss > none 3', '=/1/sss > none 5'),
    ('dark_batches', 'ok', 3, False, False, False): ('> no state: needs', '=/0/sss > none 3', '=/0/sss > none 5'),
    ('dark_batches', 'ok', 3, False, True, None): ('> no state: needs', '=/129/sss > none 3', '=/128/sss > none 5'),
    ('dark_batches', 'ok', 3, False, True, True): ('> no state: needs', '=/129/sss > none 3', '=/129/sss > none 5'),
    ('dark_batches', 'ok', 3, False, True, False): ('> no state: needs', '=/128/sss > none 3', '=/128/sss > none 5'),
    ('dark_batches', 'no, ok', 1, True, False, None): ('dark_batch/3/--- > refused', 'dark_batch/3/sss > refused 0', 'dark_batch/2/sss > refused 2'),
    ('dark_batches', 'no, ok', 1, True, False, True): ('=/3/--- =/3/fff > pair', '=/3/sss > refused 0', '=/3/sss > refused 2'),
    ('dark_batches', 'no, ok', 1, True, False, False): ('=/2/--- =/2/fff > pair', '=/2/sss > refused 0', '=/2/sss > refused 2'),
    ('dark_batches', 'no, ok', 1, True, True, None): ('dark_batch/3/--- > refused', 'dark_batch/3/sss > refused 0', 'dark_batch/2/sss > refused 2'),
    ('dark_batches', 'no, ok', 1, True, True, True): ('=/131/--- > refused', '=/131/sss > refused 0', '=/131/sss > refused 2'),
    ('dark_batches', 'no, ok', 1, True, True, False): ('=/130/--- > refused', '=/130/sss > refused 0', '=/130/sss > refused 2'),
    ('dark_batches', 'no, ok', 1, False, False, None): ('> no state: needs', 'dark_batch/1/sss > refused 0', 'dark_batch/0/sss > refused 2'),
    ('dark_batches', 'no, ok', 1, False, False, True): ('> no state: needs', '=/1/sss > refused 0', '=/1/sss > refused 2'),
    ('dark_batches', 'no, ok', 1, False, False, False): ('> no state: needs', '=/0/sss > refused 0', '=/0/sss > refused 2'),
    ('dark_batches', 'no, ok', 1, False, True, None): ('> no state: needs', 'dark_batch/1/sss > refused 0', 'dark_batch/0/sss > refused 2'),
    ('dark_batches', 'no, ok', 1, False, True, True): ('> no state: needs', '=/129/sss > refused 0', '=/129/sss > refused 2'),
    ('dark_batches', 'no, ok', 1, False, True, False): ('> no state: needs', '=/128/sss > refused 0', '=/128/sss > refused 2'),
    ('dark_batches', 'no, ok', 3, True, False, None): ('=/3/--- =/3/fff > pair', '=/3/sss > refused 0', '=/2/sss > refused 2'),
    ('dark_batches', 'no, ok', 3, True, False, True): ('=/3/--- =/3/fff > pair', '=/3/sss > refused 0', '=/3/sss > refused 2'),
    ('dark_batches', 'no, ok', 3, True, False, False): ('=/2/--- =/2/fff > pair', '=/2/sss > refused 0', '=/2/sss > refused 2'),
    ('dark_batches', 'no, ok', 3, True, True, None): ('=/131/--- > refused', '=/131/sss > refused 0', '=/130/sss > refused 2'),
    ('dark_batches', 'no, ok', 3, True, True, True): ('=/131/--- > refused', '=/131/sss > refused 0', '=/131/sss > refused 2'),
    ('dark_batches', 'no, ok', 3, True, True, False): ('=/130/--- > refused', '=/130/sss > refused 0', '=/130/sss > refused 2'),
    ('dark_batches', 'no, ok', 3, False, False, None): ('> no state: needs', '=/1/sss > refused 0', '=/0/sss > refused 2'),
    ('dark_batches', 'no, ok', 3, False, False, True): ('> no state: needs', '=/1/sss > refused 0', '=/1/sss > refused 2'),
    ('dark_batches', 'no, ok', 3, False, False, False): ('> no state: needs', '=/0/sss > refused 0', '=/0/sss > refused 2'),
    ('dark_batches', 'no, ok', 3, False, True, None): ('> no state: needs', '=/129/sss > refused 0', '=/128/sss > refused 2'),
    ('dark_batches', 'no, ok', 3, False, True, True): ('> no state: needs', '=/129/sss > refused 0', '=/129/sss > refused 2'),
    ('dark_batches', 'no, ok', 3, False, True, False): ('> no state: needs', '=/128/sss > refused 0', '=/128/sss > refused 2'),
    ('dark_batches', 'no', 1, True, False, None): ('dark_batch/3/--- > refused', 'dark_batch/3/sss > refused 0', 'dark_batch/2/sss > refused 2'),
    ('dark_batches', 'no', 1, True, False, True): ('=/3/--- =/3/fff > refused', '=/3/sss > refused 0', '=/3/sss > refused 2'),
    ('dark_batches', 'no', 1, True, False, False): ('=/2/--- =/2/fff > refused', '=/2/sss > refused 0', '=/2/sss > refused 2'),
    ('dark_batches', 'no', 1, True, True, None): ('dark_batch/3/--- > refused', 'dark_batch/3/sss > refused 0', 'dark_batch/2/sss > refused 2'),
    ('dark_batches', 'no', 1, True, True, True): ('=/131/--- > refused', '=/131/sss > refused 0', '=/131/sss > refused 2'),
    ('dark_batches', 'no', 1, True, True, False): ('=/130/--- > refused', '=/130/sss > refused 0', '=/130/sss > refused 2'),
    ('dark_batches', 'no', 1, False, False, None): ('> no state: needs', 'dark_batch/1/sss > refused 0', 'dark_batch/0/sss > refused 2'),
    ('dark_batches', 'no', 1, False, False, True): ('> no state: needs', '=/1/sss > refused 0', '=/1/sss > refused 2'),
    ('dark_batches', 'no', 1, False, False, False): ('> no state: needs', '=/0/sss > refused 0', '=/0/sss > refused 2'),
    ('dark_batches', 'no', 1, False, True, None): ('> no state: needs', 'dark_batch/1/sss > refused 0', 'dark_batch/0/sss > refused 2'),
    ('dark_batches', 'no', 1, False, True, True): ('> no state: needs', '=/129/sss > refused 0', '=/129/sss > refused 2'),
    ('dark_batches', 'no', 1, False, True, False): ('> no state: needs', '=/128/sss > refused 0', '=/128/sss > refused 2'),
    ('dark_batches', 'no', 3, True, False, None): ('=/3/--- =/3/fff > refused', '=/3/sss > refused 0', '=/2/sss > refused 2'),
    ('dark_batches', 'no', 3, True, False, True): ('=/3/--- =/3/fff > refused', '=/3/sss > refused 0', '=/3/sss > refused 2'),
    ('dark_batches', 'no', 3, True, False, False): ('=/2/--- =/2/fff > refused', '=/2/sss > refused 0', '=/2/sss > refused 2'),
    ('dark_batches', 'no', 3, True, True, None): ('=/131/--- > refused', '=/131/sss > refused 0', '=/130/sss > refused 2'),
    ('dark_batches', 'no', 3, True, True, True): ('=/131/--- > refused', '=/131/sss > refused 0', '=/131/sss > refused 2'),
    ('dark_batches', 'no', 3, True, True, False): ('=/130/--- > refused', '=/130/sss > refused 0', '=/130/sss > refused 2'),
    ('dark_batches', 'no', 3, False, False, None): ('> no state: needs', '=/1/sss > refused 0', '=/0/sss > refused 2'),
    ('dark_batches', 'no', 3, False, False, True): ('> no state: needs', '=/1/sss > refused 0', '=/1/sss > refused 2'),
    ('dark_batches', 'no', 3, False, False, False): ('> no state: needs', '=/0/sss > refused 0', '=/0/sss > refused 2'),
    ('dark_batches', 'no', 3, False, True, None): ('> no state: needs', '=/129/sss > refused 0', '=/128/sss > refused 2'),
    ('dark_batches', 'no', 3, False, True, True): ('> no state: needs', '=/129/sss > refused 0', '=/129/sss > refused 2'),
    ('dark_batches', 'no', 3, False, True, False): ('> no state: needs', '=/128/sss > refused 0', '=/128/sss > refused 2'),
    ('ingest_batch', 'ok', 1, True, None, None): ('=/3/--- > pair', '=/3/sss > pair 1', '=/2/sss > pair 3'),
    ('ingest_batch', 'ok', 1, False, None, None): ('> no state: needs', '=/1/sss > none 1', '=/0/sss > none 3'),
    ('ingest_batch', 'no, ok', 1, True, None, None): ('=/3/--- > refused', '=/3/sss > refused 0', '=/2/sss > refused 2'),
    ('ingest_batch', 'no, ok', 1, False, None, None): ('> no state: needs', '=/1/sss > refused 0', '=/0/sss > refused 2'),
    ('ingest_batch', 'no', 1, True, None, None): ('=/3/--- > refused', '=/3/sss > refused 0', '=/2/sss > refused 2'),
    ('ingest_batch', 'no', 1, False, None, None): ('> no state: needs', '=/1/sss > refused 0', '=/0/sss > refused 2'),
    ('ingest_batches', 'ok', 1, True, False, None): ('ingest_batch/3/--- > pair', 'ingest_batch/3/sss > pair 1', 'ingest_batch/2/sss > pair 3'),
    ('ingest_batches', 'ok', 1, True, True, None): ('ingest_batch/3/--- > pair', 'ingest_batch/3/sss > pair 1', 'ingest_batch/2/sss > pair 3'),
    ('ingest_batches', 'ok', 1, False, False, None): ('> no state: needs', 'ingest_batch/1/sss > none 1', 'ingest_batch/0/sss > none 3'),
    ('ingest_batches', 'ok', 1, False, True, None): ('> no state: needs', 'ingest_batch/1/sss > none 1', 'ingest_batch/0/sss > none 3'),
    ('ingest_batches', 'ok', 3, True, False, None): ('=/131/--- > pair', '=/3/sss > pair 3', '=/2/sss > pair 5'),
    ('ingest_batches', 'ok', 3, True, True, None): ('=/131/--- > pair', '=/131/sss > pair 3', '=/130/sss > pair 5'),
    ('ingest_batches', 'ok', 3, False, False, None): ('> no state: needs', '=/1/sss > none 3', '=/0/sss > none 5'),
    ('ingest_batches', 'ok', 3, False, True, None): ('> no state: needs', '=/129/sss > none 3', '=/128/sss > none 5'),
    ('ingest_batches', 'no, ok', 1, True, False, None): ('ingest_batch/3/--- > refused', 'ingest_batch/3/sss > refused 0', 'ingest_batch/2/sss > refused 2'),
    ('ingest_batches', 'no, ok', 1, True, True, None): ('ingest_batch/3/--- > refused', 'ingest_batch/3/sss > refused 0', 'ingest_batch/2/sss > refused 2'),
    ('ingest_batches', 'no, ok', 1, False, False, None): ('> no state: needs', 'ingest_batch/1/sss > refused 0', 'ingest_batch/0/sss > refused 2'),
    ('ingest_batches', 'no, ok', 1, False, True, None): ('> no state: needs', 'ingest_batch/1/sss > refused 0', 'ingest_batch/0/sss > refused 2'),
    ('ingest_batches', 'no, ok', 3, True, False, None): ('=/131/--- =/3/fff > pair', '=/3/sss > refused 0', '=/2/sss > refused 2'),
    ('ingest_batches', 'no, ok', 3, True, True, None): ('=/131/--- > refused', '=/131/sss > refused 0', '=/130/sss > refused 2'),
    ('ingest_batches', 'no, ok', 3, False, False, None): ('> no state: needs', '=/1/sss > refused 0', '=/0/sss > refused 2'),
    ('ingest_batches', 'no, ok', 3, False, True, None): ('> no state: needs', '=/129/sss > refused 0', '=/128/sss > refused 2'),
    ('ingest_batches', 'no', 1, True, False, None): ('ingest_batch/3/--- > refused', 'ingest_batch/3/sss > refused 0', 'ingest_batch/2/sss > refused 2'),
    ('ingest_batches', 'no', 1, True, True, None): ('ingest_batch/3/--- > refused', 'ingest_batch/3/sss > refused 0', 'ingest_batch/2/sss > refused 2'),
    ('ingest_batches', 'no', 1, False, False, None): ('> no state: needs', 'ingest_batch/1/sss > refused 0', 'ingest_batch/0/sss > refused 2'),
    ('ingest_batches', 'no', 1, False, True, None): ('> no state: needs', 'ingest_batch/1/sss > refused 0', 'ingest_batch/0/sss > refused 2'),
    ('ingest_batches', 'no', 3, True, False, None): ('=/131/--- =/3/fff > refused', '=/3/sss > refused 0', '=/2/sss > refused 2'),
    ('ingest_batches', 'no', 3, True, True, None): ('=/131/--- > refused', '=/131/sss > refused 0', '=/130/sss > refused 2'),
    ('ingest_batches', 'no', 3, False, False, None): ('> no state: needs', '=/1/sss > refused 0', '=/0/sss > refused 2'),
    ('ingest_batches', 'no', 3, False, True, None): ('> no state: needs', '=/129/sss > refused 0', '=/128/sss > refused 2'),
    ('dark_ingest_batches', 'ok', 1, True, False, None): ('=/3/--- > pair', '=/3/sss > pair 1', '=/2/sss > pair 3'),
    ('dark_ingest_batches', 'ok', 1, True, False, True): ('=/3/--- > pair', '=/3/sss > pair 1', '=/3/sss > pair 3'),
    ('dark_ingest_batches', 'ok', 1, True, False, False): ('=/2/--- > pair', '=/2/sss > pair 1', '=/2/sss > pair 3'),
    ('dark_ingest_batches', 'ok', 1, True, True, None): ('=/131/--- > pair', '=/131/sss > pair 1', '=/130/sss > pair 3'),
    ('dark_ingest_batches', 'ok', 1, True, True, True): ('=/131/--- > pair', '=/131/sss > pair 1', '=/131/sss > pair 3'),
    ('dark_ingest_batches', 'ok', 1, True, True, False): ('=/130/--- > pair', '=/130/sss > pair 1', '=/130/sss > pair 3'),
    ('dark_ingest_batches', 'ok', 1, False, False, None): ('> no state: needs', '=/1/sss > none 1', '=/0/sss > none 3'),
    ('dark_ingest_batches', 'ok', 1, False, False, True): ('> no state: needs', '=/1/sss > none 1', '=/1/sss > none 3'),
    ('dark_ingest_batches', 'ok', 1, False, False, False): ('> no state: needs', '=/0/sss > none 1', '=/0/sss > none 3'),
    ('dark_ingest_batches', 'ok', 1, False, True, None): ('> no state: needs', '=/129/sss > none 1', '=/128/sss > none 3'),
    ('dark_ingest_batches', 'ok', 1, False, True, True): ('> no state: needs', '=/129/sss > none 1', '=/129/sss > none 3'),
    ('dark_ingest_batches', 'ok', 1, False, True, False): ('> no state: needs', '=/128/sss > none 1', '=/128/sss > none 3'),
    ('dark_ingest_batches', 'ok', 3, True, False, None): ('=/3/--- > pair', '=/3/sss > pair 3', '=/2/sss > pair 5'),
    ('dark_ingest_batches', 'ok', 3, True, False, True): ('=/3/--- > pair', '=/3/sss > pair 3', '=/3/sss > pair 5'),
    ('dark_ingest_batches', 'ok', 3, True, False, False): ('=/2/--- > pair', '=/2/sss > pair 3', '=/2/sss > pair 5'),
    ('dark_ingest_batches', 'ok', 3, True, True, None): ('=/131/--- > pair', '=/131/sss > pair 3', '=/130/sss > pair 5'),
    ('dark_ingest_batches', 'ok', 3, True, True, True): ('=/131/--- > pair', '=/131/sss > pair 3', '=/131/sss > pair 5'),
    ('dark_ingest_batches', 'ok', 3, True, True, False): ('=/130/--- > pair', '=/130/sss > pair 3', '=/130/sss > pair 5'),
    ('dark_ingest_batches', 'ok', 3, False, False, None): ('> no state: needs', '=/1/sss > none 3', '=/0/sss > none 5'),
    ('dark_ingest_batches', 'ok', 3, False, False, True): ('> no state: needs', '=/1/sss > none 3', '=/1/sss > none 5'),
    ('dark_ingest_batches', 'ok', 3, False, False, False): ('> no state: needs', '=/0/sss > none 3', '=/0/sss > none 5'),
    ('dark_ingest_batches', 'ok', 3, False, True, None): ('> no state: needs', '=/129/sss > none 3', '=/128/sss > none 5'),
    ('dark_ingest_batches', 'ok', 3, False, True, True): ('> no state: needs', '=/129/sss > none 3', '=/129/sss > none 5'),
    ('dark_ingest_batches', 'ok', 3, False, True, False): ('> no state: needs', '=/128/sss > none 3', '=/128/sss > none 5'),
    ('dark_ingest_batches', 'no, ok', 1, True, False, None): ('=/3/--- > refused', '=/3/sss > refused 0', '=/2/sss > refused 2'),
    ('dark_ingest_batches', 'no, ok', 1, True, False, True): ('=/3/--- > refused', '=/3/sss > refused 0', '=/3/sss > refused 2'),
    ('dark_ingest_batches', 'no, ok', 1, True, False, False): ('=/2/--- > refused', '=/2/sss > refused 0', '=/2/sss > refused 2'),
    ('dark_ingest_batches', 'no, ok', 1, True, True, None): ('=/131/--- > refused', '=/131/sss > refused 0', '=/130/sss > refused 2'),
    ('dark_ingest_batches', 'no, ok', 1, True, True, True): ('=/131/--- > refused', '=/131/sss > refused 0', '=/131/sss > refused 2'),
    ('dark_ingest_batches', 'no, ok', 1, True, True, False): ('=/130/--- > refused', '=/130/sss > refused 0', '=/130/sss > refused 2'),
    ('dark_ingest_batches', 'no, ok', 1, False, False, None): ('> no state: needs', '=/1/sss > refused 0', '=/0/sss > refused 2'),
    ('dark_ingest_batches', 'no, ok', 1, False, False, True): ('> no state: needs', '=/1/sss > refused 0', '=/1/sss > refused 2'),
    ('dark_ingest_batches', 'no, ok', 1, False, False, False): ('> no state: needs', '=/0/sss > refused 0', '=/0/sss > refused 2'),
    ('dark_ingest_batches', 'no, ok', 1, False, True, None): ('> no state: needs', '=/129/sss > refused 0', '=/128/sss > refused 2'),
    ('dark_ingest_batches', 'no, ok', 1, False, True, True): ('> no state: needs', '=/129/sss > refused 0', '=/129/sss > refused 2'),
    ('dark_ingest_batches', 'no, ok', 1, False, True, False): ('> no state: needs', '=/128/sss > refused 0', '=/128/sss > refused 2'),
    ('dark_ingest_batches', 'no, ok', 3, True, False, None): ('=/3/--- =/3/fff > pair', '=/3/sss > refused 0', '=/2/sss > refused 2'),
    ('dark_ingest_batches', 'no, ok', 3, True, False, True): ('=/3/--- =/3/fff > pair', '=/3/sss > refused 0', '=/3/sss > refused 2'),
    ('dark_ingest_batches', 'no, ok', 3, True, False, False): ('=/2/--- =/2/fff > pair', '=/2/sss > refused 0', '=/2/sss > refused 2'),
    ('dark_ingest_batches', 'no, ok', 3, True, True, None): ('=/131/--- > refused', '=/131/sss > refused 0', '=/130/sss > refused 2'),
    ('dark_ingest_batches', 'no, ok', 3, True, True, True): ('=/131/--- > refused', '=/131/sss > refused 0', '=/131/sss > refused 2'),
    ('dark_ingest_batches', 'no, ok', 3, True, True, False): ('=/130/--- > refused', '=/130/sss > refused 0', '=/130/sss > refused 2'),
    ('dark_ingest_batches', 'no, ok', 3, False, False, None): ('> no state: needs', '=/1/sss > refused 0', '=/0/sss > refused 2'),
    ('dark_ingest_batches', 'no, ok', 3, False, False, True): ('> no state: needs', '=/1/sss > refused 0', '=/1/sss > refused 2'),
    ('dark_ingest_batches', 'no, ok', 3, False, False, False): ('> no state: needs', '=/0/sss > refused 0', '=/0/sss > refused 2'),
    ('dark_ingest_batches', 'no, ok', 3, False, True, None): ('> no state: needs', '=/129/sss > refused 0', '=/128/sss > refused 2'),
    ('dark_ingest_batches', 'no, ok', 3, False, True, True): ('> no state: needs', '=/129/sss > refused 0', '=/129/sss > refused 2'),
    ('dark_ingest_batches', 'no, ok', 3, False, True, False): ('> no state: needs', '=/128/sss > refused 0', '=/128/sss > refused 2'),
    ('dark_ingest_batches', 'no', 1, True, False, None): ('=/3/--- > refused', '=/3/sss > refused 0', '=/2/sss > refused 2'),
    ('dark_ingest_batches', 'no', 1, True, False, True): ('=/3/--- > refused', '=/3/sss > refused 0', '=/3/sss > refused 2'),
    ('dark_ingest_batches', 'no', 1, True, False, False): ('=/2/--- > refused', '=/2/sss > refused 0', '=/2/sss > refused 2'),
    ('dark_ingest_batches', 'no', 1, True, True, None): ('=/131/--- > refused', '=/131/sss > refused 0', '=/130/sss > refused 2'),
    ('dark_ingest_batches', 'no', 1, True, True, True): ('=/131/--- > refused', '=/131/sss > refused 0', '=/131/sss > refused 2'),
    ('dark_ingest_batches', 'no', 1, True, True, False): ('=/130/--- > refused', '=/130/sss > refused 0', '=/130/sss > refused 2'),
    ('dark_ingest_batches', 'no', 1, False, False, None): ('> no state: needs', '=/1/sss > refused 0', '=/0/sss > refused 2'),
    ('dark_ingest_batches', 'no', 1, False, False, True): ('> no state: needs', '=/1/sss > refused 0', '=/1/sss > refused 2'),
    ('dark_ingest_batches', 'no', 1, False, False, False): ('> no state: needs', '=/0/sss > refused 0', '=/0/sss > refused 2'),
    ('dark_ingest_batches', 'no', 1, False, True, None): ('> no state: needs', '=/129/sss > refused 0', '=/128/sss > refused 2'),
    ('dark_ingest_batches', 'no', 1, False, True, True): ('> no state: needs', '=/129/sss > refused 0', '=/129/sss > refused 2'),
    ('dark_ingest_batches', 'no', 1, False, True, False): ('> no state: needs', '=/128/sss > refused 0', '=/128/sss > refused 2'),
    ('dark_ingest_batches', 'no', 3, True, False, None): ('=/3/--- =/3/fff > refused', '=/3/sss > refused 0', '=/2/sss > refused 2'),
    ('dark_ingest_batches', 'no', 3, True, False, True): ('=/3/--- =/3/fff > refused', '=/3/sss > refused 0', '=/3/sss > refused 2'),
    ('dark_ingest_batches', 'no', 3, True, False, False): ('=/2/--- =/2/fff > refused', '=/2/sss > refused 0', '=/2/sss > refused 2'),
    ('dark_ingest_batches', 'no', 3, True, True, None): ('=/131/--- > refused', '=/131/sss > refused 0', '=/130/sss > refused 2'),
    ('dark_ingest_batches', 'no', 3, True, True, True): ('=/131/--- > refused', '=/131/sss > refused 0', '=/131/sss > refused 2'),
    ('dark_ingest_batches', 'no', 3, True, True, False): ('=/130/--- > refused', '=/130/sss > refused 0', '=/130/sss > refused 2'),
    ('dark_ingest_batches', 'no', 3, False, False, None): ('> no state: needs', '=/1/sss > refused 0', '=/0/sss > refused 2'),
    ('dark_ingest_batches', 'no', 3, False, False, True): ('> no state: needs', '=/1/sss > refused 0', '=/1/sss > refused 2'),
    ('dark_ingest_batches', 'no', 3, False, False, False): ('> no state: needs', '=/0/sss > refused 0', '=/0/sss > refused 2'),
    ('dark_ingest_batches', 'no', 3, False, True, None): ('> no state: needs', '=/129/sss > refused 0', '=/128/sss > refused 2'),
    ('dark_ingest_batches', 'no', 3, False, True, True): ('> no state: needs', '=/129/sss > refused 0', '=/129/sss > refused 2'),
    ('dark_ingest_batches', 'no', 3, False, True, False): ('> no state: needs', '=/128/sss > refused 0', '=/128/sss > refused 2'),
}


def _matrix_cases():
    for (front, script, k, finalize, one_launch, first), cells in _CALLS.items():
        for state, cell in zip(("none", "fresh", "running"), cells):
            for ref in (None, True, False):
                kw = dict(finalize=finalize, reference_order=ref)
                if one_launch is not None:
                    kw["require_one_launch"] = one_launch
                if f"hdr_merge_{front}" in HAS_FIRST:
                    kw["first"] = first
                yield f"hdr_merge_{front}", script, k, state, kw, cell


def test_every_combination_is_recorded():
    want = set()
    for front in FRONTS:
        lists = front in LIST_FRONTS
        want |= set(itertools.product([front[len("hdr_merge_"):]], SCRIPTS, (1, 3) if lists else (1,), (True, False),
                                      (False, True) if lists else (None,), (None, True, False) if front in HAS_FIRST else (None,)))
    assert set(_CALLS) == want


def _cell(front, calls, k, ref, batches, back):
    """The calls a front made in the notation of ``_CALLS``, the reference-order bit taken off every flag word."""
    own = front[len("hdr_merge_"):]
    words = []
    for c in calls:
        entry = c["entry"][len("ct_hdr_merge_"):]
        state = "".join("-" if p is None else "s" if str(p).startswith("state.") else "f" for p in c["args"][-7:-4])
        assert c["args"][-2] & 48 == REFERENCE_ORDER_BITS[ref] and c["sizes"] == [FRAMES] * k
        # what a retry repeats: every argument but the state pointers and the flag word
        assert c["args"][:-7] + c["args"][-4:-2] == calls[0]["args"][:-7] + calls[0]["args"][-4:-2] and c["exposures"] == calls[0]["exposures"]
        words.append(f"{'=' if entry == own else entry}/{c['args'][-2] - REFERENCE_ORDER_BITS[ref]}/{state}")
    if back.startswith("NativeLibraryError"):
        assert back == f"NativeLibraryError: {calls[-1]['entry']}: status {UNSUPPORTED} (code {UNSUPPORTED})"
        back = "refused"
    elif back.startswith("ValueError: a non-final ") and back.endswith(" needs a MergeState"):
        back = "no state: " + back.split()[4]
    return " ".join(words + [">", back] + ([] if batches is None else [str(batches)]))


@pytest.mark.parametrize("front", FRONTS)
def test_flags_states_and_retries(through, front):
    wrong = {}
    for f, script, k, state, kw, cell in _matrix_cases():
        if f == front:
            calls, batches, back = through(f, SCRIPTS[script], k=k, state=state, **kw)
            got = _cell(f, calls, k, kw["reference_order"], batches, back)
            if got != cell:
                wrong[(script, k, state, tuple(kw.items()))] = (got, cell)
    assert not wrong, f"{len(wrong)} combinations differ; the first: {next(iter(wrong.items()))}"
